#!/usr/bin/env python3
"""Training step of EnergyEquivGNN with interaction_reduction='pna': the fused segment kernels
against the composition of earlier ops, with 'max' and 'sum' beside them for scale.

Models: lmax 4, hidden 32 channels, 2 and 4 message passes (``--layers``), at 32 graphs x 1024
nodes / 4096 edges, ``agg_norm_const = degree_stats`` of the batch.  One step = forward +
relative-MSE loss + backward + grad-norm clip 10 + AdamW(amsgrad), as ``bench.py`` times it on
one device.  Variants: 'pna' on ``eelg_segment_pna_fwd`` / ``_bwd`` (``pna_fused``), 'pna' with
``EELG_PNA_FUSED=0`` (``pna_composed``: segment sums, order reductions, torch elementwise ops and
the [N, D, 12] stack), 'max' and 'sum'.  After a shared warm-up the variants alternate step by
step in one process for ``--rounds`` rounds of ``--reps`` steps, each step timed with device
events; per variant the median step, graphs/s and the peak of
``torch.cuda.max_memory_allocated`` over its own steps are reported, one JSON line per model.
``--kernels`` adds a line with the two kernels timed alone at the batch's shape and the bytes
they move.

usage: python tools/pna_bench.py [--layers 2 4] [--rounds 3] [--reps 5] [--warmup 3] [--kernels]
       [--no-composed]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "energy-equiv-lattice-gnn_amd"))

import torch  # noqa: E402

from argparse import Namespace  # noqa: E402

from gnn import _lib, degree_stats, ops  # noqa: E402
from gnn.data import collate  # noqa: E402
from gnn.model import EnergyEquivGNN  # noqa: E402
from gnn.synthetic import SyntheticLattices  # noqa: E402
from gnn.train import stiffness_loss  # noqa: E402


def _params(layers, reduction, norm, rmax):
    ir = lambda mul: "+".join(f"{mul}x{l}{'e' if l % 2 == 0 else 'o'}" for l in range(5))  # noqa: E731
    return Namespace(lmax=4, hidden_irreps=ir(32), readout_irreps=ir(16), num_edge_bases=6,
                     interaction_reduction=reduction, interaction_bias=True, agg_norm_const=norm,
                     inter_MLP_dim=64, inter_MLP_layers=3, correlation=3, global_reduction="mean",
                     message_passes=layers, positive_function="matrix_power_2", max_edge_radius=rmax)


def _timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts)


def kernel_times(csr, width, reps, warmup):
    """the two kernels alone on the batch's receiver CSR; bytes: forward reads src and writes
    out + 4 saved [N, D] buffers, backward reads src, grad_out and the 4 saved buffers and
    writes grad_src (a segment longer than 4 rows is read a second time by the forward,
    normally from the caches: not counted)"""
    lib = _lib.load()
    e, n = csr.num_edges, csr.num_nodes
    dev = csr.sender.device
    src, g = torch.randn(e, width, device=dev), torch.randn(n, width, device=dev)
    coef = torch.randn(n, 4, device=dev)
    out, mean, std = (torch.empty(n, width, device=dev) for _ in range(3))
    amin, amax = (torch.empty(n, width, device=dev, dtype=torch.int32) for _ in range(2))
    gs = torch.empty_like(src)
    part = torch.empty(lib.eelg_segment_pna_parts(width), n * 4, device=dev)
    P, s = _lib.ptr, _lib.stream(src)
    nd, ed = n * width * 4, e * width * 4
    calls = {
        "segment_pna_fwd": (ed + 5 * nd, lambda: lib.eelg_segment_pna_fwd(
            P(src), P(csr.rowptr), P(coef), n, width, P(out), P(mean), P(std), P(amin), P(amax), s)),
        "segment_pna_bwd": (2 * ed + 5 * nd, lambda: lib.eelg_segment_pna_bwd(
            P(src), P(csr.rowptr), P(coef), P(mean), P(std), P(amin), P(amax), P(g), n, width, P(gs),
            P(part), s)),
    }
    res = {"shape": f"N {n}, E {e}, width {width}"}
    for name, (nbytes, fn) in calls.items():
        ms = _timed(fn, reps, warmup)
        res[name] = {"ms": round(ms, 4), "mbytes": round(nbytes / 1e6, 1),
                     "gbytes_per_s": round(nbytes / (ms * 1e-3) / 1e9, 1)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, nargs="+", default=[2, 4])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--graphs", type=int, default=32)
    ap.add_argument("--nodes", type=int, default=1024)
    ap.add_argument("--edges", type=int, default=4096)
    ap.add_argument("--kernels", action="store_true", help="also time the two kernels alone")
    ap.add_argument("--no-composed", action="store_true", help="skip EELG_PNA_FUSED=0")
    args = ap.parse_args()
    dev = "cuda"
    ds = SyntheticLattices(args.graphs, args.nodes, args.edges, 1234)
    cpu_batch = collate([ds[g] for g in range(args.graphs)])
    stats = degree_stats(cpu_batch.edge_index, cpu_batch.node_attrs.shape[0])
    batch = cpu_batch.to(dev)
    variants = [("pna_fused", "pna", True)] + ([] if args.no_composed else [("pna_composed", "pna", False)]) \
        + [("max", "max", True), ("sum", "sum", True)]
    for layers in args.layers:
        models, opts = {}, {}
        for red in ("pna", "max", "sum"):
            torch.manual_seed(0)
            m = EnergyEquivGNN(_params(layers, red, stats if red == "pna" else 4.0, ds.max_edge_radius)).to(dev)
            models[red] = m
            opts[red] = torch.optim.AdamW(list(m.parameters()), lr=1e-3, betas=(0.9, 0.999), eps=1e-8,
                                          amsgrad=True, weight_decay=1e-8, fused=True)

        def step(red, fused):
            ops.PNA_FUSED = fused
            m, opt = models[red], opts[red]
            opt.zero_grad(set_to_none=True)
            loss = stiffness_loss(m(batch)["stiffness"], batch.stiffness)
            loss.backward()
            torch.nn.utils.clip_grad_norm_(list(m.parameters()), 10.0)
            opt.step()
            return loss

        for _ in range(args.warmup):
            for _, red, fused in variants:
                step(red, fused)
        torch.cuda.synchronize()
        times = {k: [[] for _ in range(args.rounds)] for k, _, _ in variants}
        peak = {k: 0 for k, _, _ in variants}
        loss = {}
        for rnd in range(args.rounds):
            for _ in range(args.reps):
                for key, red, fused in variants:
                    torch.cuda.synchronize()
                    torch.cuda.reset_peak_memory_stats()
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    loss[key] = step(red, fused)
                    b.record()
                    torch.cuda.synchronize()
                    times[key][rnd].append(a.elapsed_time(b))
                    peak[key] = max(peak[key], torch.cuda.max_memory_allocated())
        ops.PNA_FUSED = True
        out = {"shape": f"{args.graphs} x {args.nodes} nodes / {args.edges} edges, lmax 4, 32 channels, "
                        f"{layers} passes, fp32", "layers": layers, "degree_stats": stats,
               "rounds": args.rounds, "reps": args.reps, "warmup": args.warmup}
        for key, _, _ in variants:
            flat = [t for r in times[key] for t in r]
            ms = statistics.median(flat)
            out[key] = {"step_ms": round(ms, 3), "min_ms": round(min(flat), 3),
                        "round_medians_ms": [round(statistics.median(r), 3) for r in times[key]],
                        "graphs_per_s": round(args.graphs / ms * 1e3, 1),
                        "max_memory_allocated_mib": round(peak[key] / 2 ** 20, 1),
                        "loss": round(float(loss[key].item()), 6)}
        if "pna_composed" in out:
            out["fused_over_composed_step"] = round(out["pna_fused"]["step_ms"] / out["pna_composed"]["step_ms"], 4)
            out["fused_over_composed_memory"] = round(
                out["pna_fused"]["max_memory_allocated_mib"] / out["pna_composed"]["max_memory_allocated_mib"], 4)
        print(json.dumps(out), flush=True)
        del models, opts
        torch.cuda.empty_cache()
    if args.kernels:
        csr = EnergyEquivGNN.edge_graph(batch, strut=False)
        print(json.dumps({"kernels": kernel_times(csr, 7360, 10, 3)}), flush=True)


if __name__ == "__main__":
    main()
