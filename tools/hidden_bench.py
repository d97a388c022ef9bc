#!/usr/bin/env python3
"""Training step of the even-hidden model next to the full model, in one process.

Both models at the config-2 shape (32 graphs x 1024 nodes / 4096 edges, 4 layers, lmax 4,
correlation 3, fp32 storage): hidden ``32x0e+32x2e+32x4e`` (readout ``16x0e+16x2e+16x4e``) and
the reference's ``32x0e+..+32x4e``.  One step = forward + relative-MSE loss + backward +
grad-norm clip 10 + AdamW(amsgrad), as ``bench.py`` times it on one device.  The two models'
steps alternate (even, full, even, full, ...) after a shared warm-up, each step timed with
device events; the median of ``--reps`` steps is reported per model, with graphs/s and the
even / full ratio, as one JSON line.

usage: python tools/hidden_bench.py [--reps 20] [--warmup 5] [--graphs 32]
"""
import argparse
import json
import os
import statistics
import sys
from argparse import Namespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "energy-equiv-lattice-gnn_amd"))

import torch  # noqa: E402

from gnn import EnergyEquivGNN, kernel_sets  # noqa: E402
from gnn.data import collate  # noqa: E402
from gnn.synthetic import SyntheticLattices  # noqa: E402
from gnn.train import stiffness_loss  # noqa: E402


def make_params(ls, layers, lmax, correlation, max_edge_radius):
    return Namespace(lmax=lmax, hidden_irreps=kernel_sets.hidden_irreps_str(lmax, 32, ls),
                     readout_irreps=kernel_sets.hidden_irreps_str(lmax, 16, ls), num_edge_bases=6,
                     interaction_reduction="sum", interaction_bias=True, agg_norm_const=4.0,
                     inter_MLP_dim=64, inter_MLP_layers=3, correlation=correlation,
                     global_reduction="mean", message_passes=layers,
                     positive_function="matrix_power_2", max_edge_radius=max_edge_radius)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--graphs", type=int, default=32)
    ap.add_argument("--nodes", type=int, default=1024)
    ap.add_argument("--edges", type=int, default=4096)
    ap.add_argument("--layers", type=int, default=4)
    ap.add_argument("--lmax", type=int, default=4)
    ap.add_argument("--correlation", type=int, default=3)
    args = ap.parse_args()
    dev = "cuda"
    ds = SyntheticLattices(args.graphs, args.nodes, args.edges, 1234)
    batch = collate([ds[g] for g in range(args.graphs)]).to(dev)
    full_ls, even_ls = kernel_sets.hidden_lists(args.lmax)[:2]
    steps = {}
    for key, ls in (("even", even_ls), ("full", full_ls)):
        torch.manual_seed(0)
        model = EnergyEquivGNN(make_params(ls, args.layers, args.lmax, args.correlation,
                                           ds.max_edge_radius)).to(dev)
        plist = list(model.parameters())
        opt = torch.optim.AdamW(plist, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, amsgrad=True,
                                weight_decay=1e-8, fused=True)
        model.edge_graph(batch)

        def step(model=model, opt=opt, plist=plist):
            opt.zero_grad(set_to_none=True)
            loss = stiffness_loss(model(batch)["stiffness"], batch.stiffness)
            loss.backward()
            torch.nn.utils.clip_grad_norm_(plist, 10.0)
            opt.step()
            return loss
        steps[key] = (step, model)
    for _ in range(args.warmup):
        for key in ("even", "full"):
            steps[key][0]()
    torch.cuda.synchronize()
    times = {"even": [], "full": []}
    loss = {}
    for _ in range(args.reps):
        for key in ("even", "full"):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            loss[key] = steps[key][0]()
            b.record()
            torch.cuda.synchronize()
            times[key].append(a.elapsed_time(b))
    out = {"shape": f"{args.graphs} x {args.nodes} nodes / {args.edges} edges, {args.layers} layers, "
                    f"lmax {args.lmax}, correlation {args.correlation}, fp32",
           "reps": args.reps, "warmup": args.warmup}
    for key in ("even", "full"):
        ms = statistics.median(times[key])
        model = steps[key][1]
        out[key] = {"hidden_irreps": model.params.hidden_irreps, "step_ms": round(ms, 3),
                    "min_ms": round(min(times[key]), 3), "max_ms": round(max(times[key]), 3),
                    "graphs_per_s": round(args.graphs / ms * 1e3, 1),
                    "parameters": sum(p.numel() for p in model.parameters()),
                    "loss": round(float(loss[key].item()), 6)}
    out["even_over_full_step"] = round(out["even"]["step_ms"] / out["full"]["step_ms"], 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
