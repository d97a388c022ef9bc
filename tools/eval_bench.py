#!/usr/bin/env python3
"""What one evaluation pass costs: the ``no_grad`` forward, the stiffness metrics (the fused
``eelg_stiffness_metrics`` launch against the composed torch form: cartesian rank-4 tensor, two
einsums, two ``torch.linalg.eigvalsh``) and the whole ``gnn.evaluate`` pass.

``EnergyEquivGNN`` at the config-2 shape (lmax 4, 4 passes, batch ``--batch``) over ``--graphs``
synthetic lattices fed by ``DeviceLoader``.  One process, shared warm-up.  Sections, one JSON line
each:

1. ``forward``: ``model(batch)`` under ``no_grad`` on fresh ``DeviceLoader`` batches; windows of
   ``--reps`` batches, one synchronise at the end of each, ms per batch.
2. ``metrics``: the metrics of one batch's predictions (``[batch, 6, 6]``, 250 directions, scale
   10), fused and composed alternating window by window for ``--rounds`` rounds.  Per variant the
   device time (HIP events around the call, the queue drained before each pair) and the host
   time (host clock over a window of ``--reps`` calls without a synchronise inside: what the
   caller's thread spends; then the window's wall time with the synchronise), and the number of
   host synchronisations torch reports for one call (``torch.cuda.set_sync_debug_mode``).
3. ``evaluate``: ``gnn.evaluate`` over the whole loader, fused and composed metrics alternating,
   wall ms per pass and per batch, and the largest difference between the two tables.

usage: python tools/eval_bench.py [--graphs 256] [--batch 32] [--rounds 5] [--reps 20] [--warmup 3]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "energy-equiv-lattice-gnn_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from gnn import DeviceDataset, DeviceLoader, metrics  # noqa: E402
from gnn.synthetic import SyntheticLattices  # noqa: E402
from loader_bench import egnn_params, endless, rotatable  # noqa: E402


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


def metric_section(pred, target, dirs, args):
    out = {"section": "metrics", "batch": int(pred.shape[0]), "n_dirs": int(dirs.shape[0]), "scale": 10.0}
    res = {k: {"device": [], "host": [], "wall": []} for k in ("fused", "composed")}
    buf = torch.empty(pred.shape[0], 16, device=pred.device)

    def call(fused):
        metrics.FUSED = fused
        return metrics.stiffness_metrics(pred, target, dirs, 10.0, out=buf)
    for fused in (True, False):
        for _ in range(args.warmup):
            call(fused)
    torch.cuda.synchronize()
    for _ in range(args.rounds):
        for name, fused in (("fused", True), ("composed", False)):
            for _ in range(args.reps):
                torch.cuda.synchronize()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                call(fused)
                b.record()
                torch.cuda.synchronize()
                res[name]["device"].append(a.elapsed_time(b))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.reps):
                call(fused)
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            res[name]["host"].append((t1 - t0) * 1e3 / args.reps)
            res[name]["wall"].append((t2 - t0) * 1e3 / args.reps)
    metrics.FUSED = True
    for name, r in res.items():
        out[name] = {"device_ms": med(r["device"]), "host_ms_per_call": med(r["host"]),
                     "wall_ms_per_call": med(r["wall"])}
    out["device_speedup"] = round(out["composed"]["device_ms"]["ms"] / out["fused"]["device_ms"]["ms"], 2)
    out["host_speedup"] = round(out["composed"]["host_ms_per_call"]["ms"] / out["fused"]["host_ms_per_call"]["ms"], 2)
    out["host_syncs_per_call"] = {"fused": count_syncs(lambda: call(True)), "composed": count_syncs(lambda: call(False))}
    fused_rows = call(True).clone()
    comp_rows = call(False).clone()
    metrics.FUSED = True
    # scalar columns relative to the composed value, eigenvalues to the matrix's largest |eigenvalue|
    diff = (fused_rows - comp_rows).abs().double()
    ref = comp_rows.abs().double()
    out["max_rel_diff"] = {"scalars": float((diff[:, :4] / ref[:, :4]).max()),
                           "target_eig": float((diff[:, 4:10] / ref[:, 4:10].max(dim=1, keepdim=True).values).max()),
                           "predicted_eig": float((diff[:, 10:] / ref[:, 10:].max(dim=1, keepdim=True).values).max())}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", type=int, default=256)
    ap.add_argument("--nodes", type=int, default=1024)
    ap.add_argument("--edges", type=int, default=4096)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("eval_bench: needs a HIP device")
    dev = "cuda"
    ds = SyntheticLattices(args.graphs, args.nodes, args.edges, 1234)
    dds = DeviceDataset([rotatable(ds[g]) for g in range(args.graphs)], dev)
    from gnn.model import EnergyEquivGNN
    torch.manual_seed(0)
    model = EnergyEquivGNN(egnn_params(dds.max_edge_radius)).to(dev)
    print(json.dumps({"section": "setup", "graphs": args.graphs, "nodes": args.nodes, "edges": args.edges,
                      "batch": args.batch, "device": torch.cuda.get_device_name(0),
                      "torch_threads": torch.get_num_threads()}), flush=True)

    # 1. the no_grad forward on fresh batches
    it = endless(DeviceLoader(dds, args.batch, drop_last=True))
    with torch.no_grad():
        for _ in range(args.warmup):
            pred = model(next(it))["stiffness"]
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.rounds):
            t0 = time.perf_counter()
            for _ in range(args.reps):
                batch = next(it)
                pred = model(batch)["stiffness"]
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3 / args.reps)
    print(json.dumps({"section": "forward", "batch": args.batch, "reps": args.reps, **med(ms),
                      "graphs_per_s": round(args.batch / statistics.median(ms) * 1e3, 1)}), flush=True)

    # 2. the metrics of one batch
    dirs = metrics.metric_directions(250, seed=0, device=dev)
    print(json.dumps(metric_section(pred.detach(), batch.stiffness, dirs, args)), flush=True)

    # 3. the whole pass
    loader = DeviceLoader(dds, args.batch)
    res = {"fused": [], "composed": []}
    tables = {}
    for r in range(args.rounds + 1):
        for name, fused in (("fused", True), ("composed", False)):
            metrics.FUSED = fused
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            tables[name] = metrics.evaluate(model, loader, "test", seed=0)
            dt = (time.perf_counter() - t0) * 1e3
            if r:                         # round 0 is the warm-up
                res[name].append(dt)
    metrics.FUSED = True
    out = {"section": "evaluate", "graphs": args.graphs, "batches": len(loader)}
    for name, v in res.items():
        out[name] = {"pass_ms": med(v), "per_batch_ms": round(statistics.median(v) / len(loader), 4)}
    f, c = tables["fused"], tables["composed"]
    out["max_rel_diff"] = {k: float(np.abs(f[k] - c[k]).max() / np.abs(c[k]).max())
                           for k in ("loss", "mseloss", "dir_loss", "mean_stiffness", "target_eig", "predicted_eig")}
    out["aggr_fused"] = {k: round(v, 6) for k, v in metrics.aggr_errors(f).items()}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
