#!/usr/bin/env python3
"""What the transverse surfaces (shear modulus, Poisson's ratio, compressibility) of a batch of
stiffness matrices cost on the device: the fused kernels (``eelg_transverse_props`` /
``eelg_transverse_props_bwd``) against the composed torch form (``cholesky_ex``,
``cholesky_inverse``, the quadratic forms as einsums, ``min`` / ``max``), forward alone and
forward + backward.

Inputs: ``--batches`` (default 32 and 256) squares of random symmetric matrices (the shape of
``matrix_power_2`` outputs) and ``--dirs`` (default 250) unit directions.  Per batch size and
variant, fused and composed alternating window by window for ``--rounds`` rounds in one process:

* device time: HIP events around one call, the queue drained before each;
* host time: host clock over a window of ``--reps`` calls without a synchronise inside (what the
  caller's thread spends), and the window's wall time with the synchronise.

One JSON line per batch size; ``--out`` (default ``profiles/transverse_summary.md``) gets the table.

usage: python tools/transverse_bench.py [--batches 32 256] [--dirs 250] [--rounds 5] [--reps 20] [--warmup 3]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "energy-equiv-lattice-gnn_amd"))

import torch  # noqa: E402

from gnn import transverse  # noqa: E402
from gnn.metrics import metric_directions  # noqa: E402


def med(ms):
    return {"ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
            "n": len(ms)}


def section(nb, dirs, args):
    gen = torch.Generator().manual_seed(nb)
    s = torch.randn(nb, 6, 6, generator=gen)
    s = (s + s.transpose(1, 2)) / 2
    c = (s @ s).to(dirs.device)
    gp = torch.randn(nb, 7, generator=gen).to(dirs.device)
    gp[:, 6] = 0
    gt = (torch.randn(nb, dirs.shape[0], 5, generator=gen) / dirs.shape[0]).to(dirs.device)

    def call(fused, backward):
        transverse.FUSED = fused
        if not backward:
            with torch.no_grad():
                return transverse.transverse_properties(c, dirs)
        x = c.detach().requires_grad_(True)
        props, t = transverse.transverse_properties(x, dirs)[:2]
        return props, t, torch.autograd.grad([props, t], [x], [gp, gt])[0]
    out = {"section": "transverse", "batch": nb, "n_dirs": int(dirs.shape[0])}
    for mode, backward in (("forward", False), ("forward_backward", True)):
        res = {k: {"device": [], "host": [], "wall": []} for k in ("fused", "composed")}
        for fused in (True, False):
            for _ in range(args.warmup):
                call(fused, backward)
        torch.cuda.synchronize()
        for _ in range(args.rounds):
            for name, fused in (("fused", True), ("composed", False)):
                for _ in range(args.reps):
                    torch.cuda.synchronize()
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    call(fused, backward)
                    b.record()
                    torch.cuda.synchronize()
                    res[name]["device"].append(a.elapsed_time(b))
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.reps):
                    call(fused, backward)
                t1 = time.perf_counter()
                torch.cuda.synchronize()
                t2 = time.perf_counter()
                res[name]["host"].append((t1 - t0) * 1e3 / args.reps)
                res[name]["wall"].append((t2 - t0) * 1e3 / args.reps)
        o = {}
        for name, r in res.items():
            o[name] = {"device_ms": med(r["device"]), "host_ms_per_call": med(r["host"]),
                       "wall_ms_per_call": med(r["wall"])}
        o["device_speedup"] = round(o["composed"]["device_ms"]["ms"] / o["fused"]["device_ms"]["ms"], 2)
        o["host_speedup"] = round(o["composed"]["host_ms_per_call"]["ms"] / o["fused"]["host_ms_per_call"]["ms"], 2)
        out[mode] = o
    f, k = [x.detach() for x in call(True, True)], [x.detach() for x in call(False, True)]
    transverse.FUSED = True
    ok = f[0][:, 6] == 1
    out["spd_graphs"] = int(ok.sum())
    out["max_diff"] = {
        "G (relative)": float(((f[1] - k[1])[ok][:, :, :2].abs() / k[1][ok][:, :, :2].abs()).max()),
        "nu (absolute)": float((f[1] - k[1])[ok][:, :, 2:4].abs().max()),
        "gradient": float(((f[2] - k[2])[ok].abs().amax(dim=(1, 2)) / k[2][ok].abs().amax(dim=(1, 2))).max())}
    return out


def table(rows, device):
    lines = ["# Transverse surfaces: fused kernels against the composed torch form", "",
             f"`tools/transverse_bench.py` on {device}; medians, ms per call.  Device: HIP events around one call; "
             "host: the caller's thread over a window of calls without a synchronise inside.", "",
             "| B | P | pass | variant | device ms | host ms | wall ms |", "|---|---|---|---|---|---|---|"]
    for r in rows:
        for mode in ("forward", "forward_backward"):
            for name in ("fused", "composed"):
                v = r[mode][name]
                lines.append(f"| {r['batch']} | {r['n_dirs']} | {mode.replace('_', ' + ')} | {name} | "
                             f"{v['device_ms']['ms']:.4f} | {v['host_ms_per_call']['ms']:.4f} | "
                             f"{v['wall_ms_per_call']['ms']:.4f} |")
    lines += ["", "| B | pass | device speed-up | host speed-up |", "|---|---|---|---|"]
    for r in rows:
        for mode in ("forward", "forward_backward"):
            lines.append(f"| {r['batch']} | {mode.replace('_', ' + ')} | {r[mode]['device_speedup']} | "
                         f"{r[mode]['host_speedup']} |")
    lines += ["", "Largest difference fused against composed (gradient relative to each graph's largest entry): "
              + "; ".join(f"B = {r['batch']}: " + ", ".join(f"{k} {v:.1e}" for k, v in r["max_diff"].items())
                          for r in rows) + ".", ""]
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[32, 256])
    ap.add_argument("--dirs", type=int, default=250)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "transverse_summary.md"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("transverse_bench: needs a HIP device")
    dirs = metric_directions(args.dirs, seed=0, device="cuda")
    device = torch.cuda.get_device_name(0)
    print(json.dumps({"section": "setup", "device": device, "torch_threads": torch.get_num_threads()}), flush=True)
    rows = []
    for nb in args.batches:
        rows.append(section(nb, dirs, args))
        print(json.dumps(rows[-1]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(table(rows, device))


if __name__ == "__main__":
    main()
