#!/usr/bin/env python
"""Ledger of the host launch paths in ``gnn/ops.py``: fixed-seed forward / backward passes through
every branch the autograd wrappers take, each recorded as the sha256 of every output and gradient
(raw bytes on the host) and the ``ops.TIMER`` name -> count map of the pass.  Two trees that run
the same kernels with the same operands in the same order write equal ledgers:

    python tools/op_ledger.py --out ledger.json        # run in each tree, compare the files
    python tools/op_ledger.py --compare a.json b.json  # lists the entries that differ
"""
import argparse
import hashlib
import json
import os
import sys
from argparse import Namespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "energy-equiv-lattice-gnn_amd"), ROOT]
DEV = "cuda:0"
HID4 = "32x0e+32x1o+32x2e+32x3o+32x4e"


def compare(a_path: str, b_path: str) -> int:
    a, b = (json.load(open(p)) for p in (a_path, b_path))
    bad = sorted(k for k in set(a) | set(b) if a.get(k) != b.get(k))
    for k in bad:
        ha, hb = a.get(k, {}).get("sha256", {}), b.get(k, {}).get("sha256", {})
        diff = sorted(n for n in set(ha) | set(hb) if ha.get(n) != hb.get(n))
        print(f"DIFF {k}: tensors {diff}; launches equal: "
              f"{a.get(k, {}).get('launches') == b.get(k, {}).get('launches')}")
    print(f"{len(a)} / {len(b)} cases, {len(bad)} differ")
    return 1 if bad else 0


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="op_ledger.json")
    ap.add_argument("--compare", nargs=2, metavar="JSON")
    args = ap.parse_args()
    if args.compare:
        return compare(*args.compare)

    import torch
    from gnn import EnergyEquivGNN, SyntheticLattices, _lib, collate, ops, torch_ops  # noqa: F401
    from gnn.mace import SymmetricContraction
    from gnn.train import stiffness_loss

    ledger, models = {}, {}
    ops.TIMER.enabled = True

    def rand(*shape, seed, grad=False, dtype=torch.float32):
        t = torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(DEV).to(dtype)
        return t.requires_grad_(grad)

    def record(name, fn, **switches):
        """run ``fn`` -> {tensor name: tensor} under the module switches and enter it"""
        old = {k: getattr(ops, k) for k in switches}
        for k, v in switches.items():
            setattr(ops, k, v)
        ops.TIMER.records = {}
        try:
            tensors = fn()
            torch.cuda.synchronize()
        finally:
            for k, v in old.items():
                setattr(ops, k, v)
        sha = {k: hashlib.sha256(t.detach().cpu().reshape(-1).view(torch.uint8).numpy().tobytes()).hexdigest()
               for k, t in tensors.items() if t is not None}
        ledger[name] = {"sha256": sha, "launches": {k: len(v) for k, v in sorted(ops.TIMER.records.items())}}

    ds = SyntheticLattices(2, 24, 96, seed=7)

    def model(lmax, storage):
        if (lmax, storage) not in models:
            irreps = ["+".join(f"{m}x{l}{'eo'[l % 2]}" for l in range(lmax + 1)) for m in (32, 16)]
            p = Namespace(lmax=lmax, hidden_irreps=irreps[0], readout_irreps=irreps[1], num_edge_bases=6,
                          interaction_reduction="sum", interaction_bias=True, agg_norm_const=4.0,
                          inter_MLP_dim=64, inter_MLP_layers=3, correlation=3, global_reduction="mean",
                          message_passes=2, positive_function="matrix_power_2",
                          max_edge_radius=ds.max_edge_radius, storage_dtype=storage)
            torch.manual_seed(0)
            models[lmax, storage] = EnergyEquivGNN(p).to(DEV)
        return models[lmax, storage]

    def grads(mod, out):
        for k, v in mod.named_parameters():
            out["grad." + k], v.grad = v.grad, None
        return out

    def step(lmax, storage, geometry=False):               # (a) one training step of the model
        m, b = model(lmax, storage), collate([ds[0], ds[1]]).to(DEV)
        EnergyEquivGNN.edge_graph(b)                        # collate-time: the CSR and the strut map
        b.positions.requires_grad_(geometry)
        c = m(b)["stiffness"]
        loss = stiffness_loss(c, b.stiffness)
        loss.backward()
        return grads(m, {"stiffness": c, "loss": loss, "grad.positions": b.positions.grad})

    def layer(storage):                                     # (b), (c) interaction block + product
        m, b = model(4, storage), collate([ds[0], ds[1]]).to(DEV)
        csr = EnergyEquivGNN.edge_graph(b)
        lay = m.stiffness_head.layers[1]
        sh, feats = ops.edge_embed(b.positions, csr, b.shifts[csr.perm], b.edge_attr[csr.perm].reshape(-1),
                                   4, 6, 0.6, ds.max_edge_radius)
        x = rand(csr.num_nodes, 800, seed=1, grad=True)
        y = lay(x, csr, sh, feats)
        y.backward(rand(*y.shape, seed=2))
        return grads(lay, {"y": y, "grad.x": x.grad})

    for storage in ("float32", "bfloat16"):
        for lmax in (4, 2):
            for strut in (True, False):
                record(f"a/step/lmax{lmax}/{storage}/strut{int(strut)}",
                       lambda: step(lmax, storage), STRUT_WEIGHTS=strut)
        for sw in (dict(TP_BWF=True), dict(TP_BWC=4), dict(TP_BWD_SENDER=True), dict(TP_BWD_SPOS=True)):
            record(f"b/layer/{storage}/{sw}", lambda: layer(storage), **sw)
    for lmax in (4, 2):
        record(f"a/step/lmax{lmax}/float32/geometry", lambda: step(lmax, "float32", True))
    for sw in (dict(RADIAL_CHAIN=False), dict(OVERLAP=False),
               dict(SC_CMAJOR_ON_SIDE=True, SC_COEF_ON_SIDE=True)):
        record(f"c/layer/float32/{sw}", lambda: layer("float32"), **sw)

    e = 67                                                  # (d) the radial MLP alone
    pair = torch.arange(e) ^ 1
    pair[e - 1] = e - 1                                     # edges (0, 1), (2, 3), ...; the last alone
    smap = ops.StrutMap(pair.to(DEV), (torch.arange(e) // 2).to(torch.int32).to(DEV),
                        torch.arange(0, e, 2).to(DEV), (e + 1) // 2)

    def radial(n_out, shared, frozen=False):
        torch.manual_seed(n_out)
        mlp = torch.nn.Sequential(torch.nn.Linear(12, 64), torch.nn.SiLU(), torch.nn.Linear(64, 64),
                                  torch.nn.SiLU(), torch.nn.Linear(64, n_out, bias=False)).to(DEV)
        mlp.requires_grad_(not frozen)
        feats = torch.rand(smap.n_rows, 12, generator=torch.Generator().manual_seed(3)).to(DEV)[smap.row.long()]
        feats.requires_grad_(frozen)
        g = rand(e, n_out, seed=4)
        if shared:
            sw = ops.radial_mlp_shared(feats, mlp, smap)
            w, sw.box.gw = sw.w, g                          # per edge, as tp_bwd leaves it
            sw.token.backward(torch.zeros(1, device=DEV))
        else:
            w = ops.radial_mlp(feats, mlp)
            w.backward(g)
        return grads(mlp, {"w": w, "grad.feats": feats.grad})

    for n_out in (160, 36):
        for shared in (False, True):
            record(f"d/radial/{n_out}/shared{int(shared)}", lambda: radial(n_out, shared))
        real, ops._radial_chunks = ops._radial_chunks, lambda e, *a: [(0, 24), (24, 48), (48, e)]
        record(f"d/radial/{n_out}/three_ranges", lambda: radial(n_out, False))
        ops._radial_chunks = real
        record(f"d/radial/{n_out}/frozen", lambda: radial(n_out, False, frozen=True))

    def custom_tp(bf):                                      # (e) the torch.library ops
        b = collate([ds[0], ds[1]]).to(DEV)
        csr = EnergyEquivGNN.edge_graph(b)
        idx, info, _ = _lib.tp_config("tpB_l4")
        x, sh = rand(csr.num_nodes, info["din"], seed=5, grad=True), rand(csr.num_edges, info["nsh"], seed=6)
        w = rand(csr.num_edges, info["wn"], seed=7, dtype=torch.bfloat16 if bf else torch.float32, grad=True)
        a = torch.ops.eelg.tp_interaction(x, sh, w, csr.sender, csr.receiver, csr.rowptr, csr.sperm,
                                          csr.srowptr, idx, 0.25)
        a.backward(rand(*a.shape, seed=8))
        return {"agg": a, "grad.x": x.grad, "grad.w": w.grad}

    def symcon(want_x, want_c):
        torch.manual_seed(3)
        sc = SymmetricContraction(HID4, HID4, 3).to(DEV)
        idx, info = sc._config()
        x, coef = rand(33, 800, seed=9, grad=want_x), sc.coefficients().detach().requires_grad_(want_c)
        y = ops.symmetric_contraction(x, coef, idx, info, 32)
        y.backward(rand(*y.shape, seed=10))
        return {"y": y, "grad.x": x.grad, "grad.coef": coef.grad}

    for bf in (False, True):
        record(f"e/torch_ops.tp_interaction/bf16={bf}", lambda: custom_tp(bf))
    for want in ((True, False), (False, True), (True, True)):
        record(f"e/symmetric_contraction/x{int(want[0])}coef{int(want[1])}", lambda: symcon(*want))

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(ledger, f, indent=1, sort_keys=True)
    print(f"{len(ledger)} cases -> {args.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
