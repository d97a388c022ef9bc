#!/usr/bin/env python3
"""What the tail of a design iteration costs on the device: the fused step (``eelg_design_step``, one
launch) against the composed torch form (``design_step_composed``: tie, check, normalise, step,
clamp, rescale as a chain of small torch ops with ``scatter_reduce_`` / ``index_add_`` for the
per-graph values).

Shapes: ``--batches`` (default 32 and 256) lattices of 64 nodes / 256 directed edges, and the
benchmark's config-2 batch (32 lattices of 1024 nodes / 4096 edges; ``--no-config2`` leaves it out).
Gradients and momenta are random; both forms update private copies in place.  Per shape, fused and
composed alternating window by window for ``--rounds`` rounds:

* device time: HIP events around one call, the queue drained before each;
* host time: host clock over a window of ``--reps`` calls without a synchronise inside (what the
  caller's thread spends), and the window's wall time with the synchronise;
* launches: device operations one call dispatches (the fused step: its one kernel, from
  ``ops.TIMER``; the composed form: the ATen operations torch dispatches, each at least one launch);
* host synchronisations torch reports for one call (``torch.cuda.set_sync_debug_mode``).

One JSON line per shape; ``--out`` (default ``profiles/design_summary.md``) gets the table, ahead of
whatever follows the marker line ``## Accuracy`` in the existing file.

usage: python tools/design_bench.py [--batches 32 256] [--rounds 5] [--reps 20] [--warmup 3]
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
from torch.utils._python_dispatch import TorchDispatchMode  # noqa: E402

from gnn import SyntheticLattices, collate, design, ops  # noqa: E402

HYPER = dict(step_r=2.0 ** -11, step_pos=2.0 ** -8, beta=0.5, r_min=2.0 ** -9, r_max=2.0 ** -4, move_limit=2.0 ** -4,
             keep_volume=True)


class CountOps(TorchDispatchMode):
    def __init__(self):
        super().__init__()
        self.n = 0

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        self.n += 1
        return func(*args, **(kwargs or {}))


def med(ms):
    return {"ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
            "n": len(ms)}


def count_syncs(fn):
    """Host synchronisations torch reports for one call (``set_sync_debug_mode``), or None."""
    import warnings
    try:
        torch.cuda.set_sync_debug_mode("warn")
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            fn()
        return sum("synchroniz" in str(x.message) for x in w)
    except Exception:                          # the mode is not available in this build
        return None
    finally:
        torch.cuda.set_sync_debug_mode("default")


def section(nb, nodes, edges, args):
    ds = SyntheticLattices(nb, nodes, edges, 1234)
    b = collate([ds[g] for g in range(nb)]).to("cuda")
    lay = design.design_layout(b)
    gen = torch.Generator().manual_seed(nb)
    n, e = lay.n_nodes, lay.n_edges
    first = torch.minimum(lay.partner.long(), torch.arange(e, device="cuda"))
    g_pos, g_r = torch.randn(n, 3, generator=gen).cuda(), torch.randn(e, generator=gen).cuda()
    pos0, r0, shifts = b.positions.contiguous(), b.edge_attr.reshape(-1).contiguous(), b.shifts.contiguous()
    v0 = design.strut_volume(b, lay)
    state = {}

    def reset():
        state.update(pos=pos0.clone(), r=r0.clone(), m_pos=torch.zeros_like(pos0), m_r=torch.zeros_like(r0),
                     vol=torch.empty(nb, device="cuda"), flag=torch.zeros(nb, dtype=torch.int32, device="cuda"))

    def call(fused):
        design.FUSED = fused
        return design.design_step(lay, g_pos, g_r, state["pos"], state["r"], pos0, state["m_pos"], state["m_r"], shifts, v0,
                                  inplace=True, vol=state["vol"], flag=state["flag"], **HYPER)
    out = {"section": "design_step", "batch": nb, "nodes": nodes, "edges": edges}
    res = {k: {"device": [], "host": [], "wall": []} for k in ("fused", "composed")}
    reset()
    for fused in (True, False):
        for _ in range(args.warmup):
            call(fused)
    torch.cuda.synchronize()
    for _ in range(args.rounds):
        for name, fused in (("fused", True), ("composed", False)):
            reset()
            for _ in range(args.reps):
                torch.cuda.synchronize()
                a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                call(fused)
                z.record()
                torch.cuda.synchronize()
                res[name]["device"].append(a.elapsed_time(z))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.reps):
                call(fused)
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            res[name]["host"].append((t1 - t0) * 1e3 / args.reps)
            res[name]["wall"].append((t2 - t0) * 1e3 / args.reps)
    for name, r in res.items():
        out[name] = {"device_ms": med(r["device"]), "host_ms_per_call": med(r["host"]),
                     "wall_ms_per_call": med(r["wall"])}
    out["device_speedup"] = round(out["composed"]["device_ms"]["ms"] / out["fused"]["device_ms"]["ms"], 2)
    out["host_speedup"] = round(out["composed"]["host_ms_per_call"]["ms"] / out["fused"]["host_ms_per_call"]["ms"], 2)
    out["host_syncs_per_call"] = {"fused": count_syncs(lambda: call(True)), "composed": count_syncs(lambda: call(False))}
    # launches: the fused step's kernel records, the composed form's dispatched ATen operations
    ops.TIMER.enabled, ops.TIMER.records = True, {}
    with CountOps() as fused_ops:
        call(True)
    kernels = len(ops.TIMER.records.get("design_step", []))
    ops.TIMER.enabled, ops.TIMER.records = False, {}
    with CountOps() as composed_ops:
        call(False)
    out["launches"] = {"fused": kernels + fused_ops.n, "composed": composed_ops.n}
    # one step from the same state, both forms
    reset()
    f = [t.clone() for t in call(True)]
    reset()
    c = [t.clone() for t in call(False)]
    design.FUSED = True
    names = ("pos", "r", "m_pos", "m_r", "vol")
    out["max_rel_diff"] = {k: float((x - y).abs().max() / y.abs().max()) for k, x, y in zip(names, f, c)}
    out["flags_equal"] = bool(torch.equal(f[5], c[5]))
    return out


def table(rows, device):
    lines = ["# Design step: the fused kernel against the composed torch form", "",
             f"`tools/design_bench.py` on {device}; medians, ms per step.  Device: HIP events around one call; host: the "
             "caller's thread over a window of calls without a synchronise inside; launches: the fused step's kernel, "
             "the ATen operations the composed form dispatches (each at least one launch); syncs: host synchronisations "
             "torch reports for one call.", "",
             "| B | nodes / edges per graph | variant | device ms | host ms | wall ms | launches | syncs |",
             "|---|---|---|---|---|---|---|---|"]
    for r in rows:
        for name in ("fused", "composed"):
            v = r[name]
            lines.append(f"| {r['batch']} | {r['nodes']} / {r['edges']} | {name} | {v['device_ms']['ms']:.4f} | "
                         f"{v['host_ms_per_call']['ms']:.4f} | {v['wall_ms_per_call']['ms']:.4f} | "
                         f"{r['launches'][name]} | {r['host_syncs_per_call'][name]} |")
    lines += ["", "| B | nodes / edges per graph | device speed-up | host speed-up |", "|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r['batch']} | {r['nodes']} / {r['edges']} | {r['device_speedup']} | {r['host_speedup']} |")
    lines += ["", "Largest difference fused against composed after one step (relative to the column's largest entry): "
              + "; ".join(f"B = {r['batch']}, {r['nodes']} nodes: " + ", ".join(f"{k} {v:.1e}" for k, v in r["max_rel_diff"].items())
                          for r in rows) + ".", ""]
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[32, 256])
    ap.add_argument("--no-config2", action="store_true")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "design_summary.md"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("design_bench: needs a HIP device")
    device = torch.cuda.get_device_name(0)
    print(json.dumps({"section": "setup", "device": device, "torch_threads": torch.get_num_threads()}), flush=True)
    shapes = [(nb, 64, 256) for nb in args.batches] + ([] if args.no_config2 else [(32, 1024, 4096)])
    rows = []
    for nb, nodes, edges in shapes:
        rows.append(section(nb, nodes, edges, args))
        print(json.dumps(rows[-1]), flush=True)
    if args.out:
        tail = ""
        if os.path.exists(args.out):
            old = open(args.out).read()
            if "## Accuracy" in old:
                tail = old[old.index("## Accuracy"):]
        with open(args.out, "w") as f:
            f.write(table(rows, device) + ("\n" + tail if tail else ""))


if __name__ == "__main__":
    main()
