#!/usr/bin/env python3
"""The training step's tail, composed against fused: bench.py's step() rule restated
(``stiffness_loss`` + ``clip_grad_norm_`` + ``torch.optim.AdamW(fused=True)`` + ``zero_grad``)
against ``gnn.trainer.Trainer``'s step (``FlatAdamW``, and the fused loss with --fused-loss), run
alternately in ONE process on the config-2 shape (32 graphs x 1024 nodes x 4096 edges, 4 layers,
lmax 4), each arm on its own copy of the model.

Per arm and feed it prints ms per training batch of every round (synchronised wall time over
--steps batches), the host's enqueue time per batch (tools/hosttime.py's method: one batch after a
full drain, timed before the next synchronisation) and the synchronising calls in one batch
(torch.cuda.set_sync_debug_mode('warn')).  Feeds: the resident batch, and with --fresh a fresh
``DeviceLoader`` batch per step.

usage (GPU box):
  python tools/train_bench.py [--steps 20] [--pairs 3] [--accumulate 1 4] [--fresh] [--fused-loss]
  rocprofv3 --kernel-trace --stats -d DIR -- python tools/train_bench.py --tail ARM --steps N
The second form runs ONLY the tail of the step N times (the loss on a fixed prediction, its
backward, and clip + optimizer + zeroing over gradients that are re-attached by reference, which
launches nothing), so every kernel in the trace belongs to the tail: the launches per step are the
difference of the trace's total calls between two N, divided by the difference in N."""
import argparse
import json
import os
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "energy-equiv-lattice-gnn_amd")]

import torch  # noqa: E402


def build(fused_loss: bool, acc: int, fused_optimizer: bool):
    import bench
    from argparse import Namespace
    from gnn import EnergyEquivGNN
    from gnn.train import LightningWrappedModel
    from gnn.trainer import Trainer
    ds = build.ds
    params = bench.make_params(4, ds.max_edge_radius)
    torch.manual_seed(0)
    module = LightningWrappedModel(EnergyEquivGNN, Namespace(**vars(params), fused_loss=fused_loss)).cuda()
    tr = Trainer(accumulate_grad_batches=acc, gradient_clip_val=10.0, log_every_n_steps=10 ** 6,
                 fused_optimizer=fused_optimizer)
    tr._setup(module)
    tr._t0 = time.monotonic()
    return module, tr


def composed_arm(acc: int):
    """bench.py's step(): one batch; every ``acc`` batches clip + AdamW(fused) + zero_grad"""
    from gnn.train import stiffness_loss
    module, tr = build(False, acc, False)
    model, plist = module.model, list(module.model.parameters())
    p = module.params
    opt = torch.optim.AdamW(plist, lr=p.lr, betas=(p.beta1, 0.999), eps=p.epsilon, amsgrad=p.amsgrad,
                            weight_decay=p.weight_decay, fused=True)
    state = {"k": 0}

    def batch_step(b):
        loss = stiffness_loss(model(b)["stiffness"], b.stiffness)
        (loss if acc == 1 else loss * (1.0 / acc)).backward()
        state["k"] += 1
        if state["k"] % acc == 0:
            torch.nn.utils.clip_grad_norm_(plist, 10.0)
            opt.step()
            opt.zero_grad(set_to_none=True)
        return loss
    return batch_step


def trainer_arm(acc: int, fused_loss: bool):
    module, tr = build(fused_loss, acc, True)

    def batch_step(b):
        return tr._train_batch(module, b, 0, 10 ** 9)
    return batch_step


def timed(step, feed, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        step(feed())
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


def host_time(step, feed, n):
    out = []
    for _ in range(n):
        b = feed()
        torch.cuda.synchronize()
        t = time.perf_counter()
        step(b)
        out.append((time.perf_counter() - t) * 1e3)
    torch.cuda.synchronize()
    out.sort()
    return out[len(out) // 2]


def syncs(step, feed, acc):
    b = [feed() for _ in range(acc)]
    torch.cuda.synchronize()
    with warnings.catch_warnings(record=True) as ws:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        for x in b:
            step(x)
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    # (the first set_sync_debug_mode call of a process warns that the mode is a prototype feature)
    hits = [w for w in ws if "synchroniz" in str(w.message).lower() and "prototype" not in str(w.message)]
    return {"per_batch": len(hits) / acc, "at": sorted({f"{os.path.basename(w.filename)}:{w.lineno}" for w in hits})}


def tail_only(arm: str, steps: int):
    """only the tail, ``steps`` times (for a kernel trace)"""
    from gnn.train import stiffness_loss
    from gnn.ops import stiffness_loss_fused
    fused = arm != "composed"
    module, tr = build(arm == "fused+loss", 1, fused)
    plist = list(module.model.parameters())
    batch = build.batch
    loss = stiffness_loss(module.model(batch)["stiffness"], batch.stiffness)
    loss.backward()
    grads = [p.grad.detach().clone() for p in plist]
    pred0 = module.model(batch)["stiffness"].detach()
    if not fused:
        p = module.params
        opt = torch.optim.AdamW(plist, lr=p.lr, betas=(p.beta1, 0.999), eps=p.epsilon, amsgrad=p.amsgrad,
                                weight_decay=p.weight_decay, fused=True)
    torch.cuda.synchronize()
    for _ in range(steps):
        pred = pred0.clone().requires_grad_(True)          # (one copy kernel per step in every arm)
        if arm == "fused+loss":
            stiffness_loss_fused(pred, batch.stiffness)[0].backward()
        else:
            stiffness_loss(pred, batch.stiffness).backward()
        for q, g in zip(plist, grads):
            q.grad = g
        if fused:
            tr.optimizer.step()
        else:
            torch.nn.utils.clip_grad_norm_(plist, 10.0)
            opt.step()
            opt.zero_grad(set_to_none=True)
    torch.cuda.synchronize()
    print(json.dumps({"tail": arm, "steps": steps}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20, help="training batches per timed round")
    ap.add_argument("--pairs", type=int, default=3, help="alternating (composed, fused) rounds after the warm-up pair")
    ap.add_argument("--accumulate", type=int, nargs="+", default=[1, 4])
    ap.add_argument("--fresh", action="store_true", help="also feed a fresh DeviceLoader batch per step")
    ap.add_argument("--fused-loss", action="store_true", help="the Trainer arm with params.fused_loss")
    ap.add_argument("--tail", choices=["composed", "fused", "fused+loss"], default=None)
    args = ap.parse_args()
    from gnn import DeviceDataset, DeviceLoader, EnergyEquivGNN
    from gnn.data import collate
    from gnn.synthetic import SyntheticLattices
    build.ds = ds = SyntheticLattices(32, 1024, 4096, 1234)
    build.batch = batch = collate([ds[g] for g in range(32)]).to("cuda")
    EnergyEquivGNN.edge_graph(batch)
    if args.tail:
        return tail_only(args.tail, args.steps)
    feeds = {"resident": lambda: batch}
    if args.fresh:
        loader = DeviceLoader(DeviceDataset(ds, "cuda"), 32)
        ids = list(range(32))
        feeds["fresh DeviceLoader batch"] = lambda: loader.assemble(ids)
    for acc in args.accumulate:
        arms = {"composed": composed_arm(acc),
                "trainer" + ("+fused_loss" if args.fused_loss else ""): trainer_arm(acc, args.fused_loss)}
        for fname, feed in feeds.items():
            rounds = {k: [] for k in arms}
            for r in range(args.pairs + 1):                  # round 0 is the discarded warm-up pair
                for k, step in arms.items():
                    ms = timed(step, feed, args.steps)
                    if r:
                        rounds[k].append(round(ms, 3))
            host = {k: round(host_time(step, feed, 8 * acc), 3) for k, step in arms.items()}
            sy = {k: syncs(step, feed, acc) for k, step in arms.items()}
            print(json.dumps({"accumulate_grad_batches": acc, "feed": fname, "steps_per_round": args.steps,
                              "ms_per_batch": rounds, "host_ms_per_batch_median": host,
                              "syncs_per_batch": sy}), flush=True)


if __name__ == "__main__":
    main()
