#!/usr/bin/env python
"""Ledger of the host launch paths in ``gnn/``: fixed-seed forward / backward passes through
every branch the autograd wrappers, the linears, the gate and the optimizer take, each recorded
as the sha256 of every output and gradient (raw bytes on the host), the ``ops.TIMER`` name ->
count map of the pass and the ordered error labels handed to ``_lib.check`` (one per launch).
Two trees that run the same kernels with the same operands in the same order write equal ledgers:

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
              f"{a.get(k, {}).get('launches') == b.get(k, {}).get('launches')}; labels equal: "
              f"{a.get(k, {}).get('labels') == b.get(k, {}).get('labels')}")
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
    from gnn import EnergyEquivGNN, SyntheticLattices, _lib, collate, dense, o3, ops, torch_ops  # noqa: F401
    from gnn.mace import SymmetricContraction
    from gnn.optim import FlatAdamW
    from gnn.train import stiffness_loss

    ledger, models, labels = {}, {}, []
    ops.TIMER.enabled = True
    real_check = _lib.check

    def check(rc, what):                                    # every launch passes its label here
        labels.append(what)
        return real_check(rc, what)
    _lib.check = check

    def rand(*shape, seed, grad=False, dtype=torch.float32):
        t = torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(DEV).to(dtype)
        return t.requires_grad_(grad)

    def record(name, fn, **switches):
        """run ``fn`` -> {tensor name: tensor} under the module switches and enter it"""
        old = {k: getattr(ops, k) for k in switches}
        for k, v in switches.items():
            setattr(ops, k, v)
        ops.TIMER.records = {}
        del labels[:]
        try:
            tensors = fn()
            torch.cuda.synchronize()
        finally:
            for k, v in old.items():
                setattr(ops, k, v)
        sha = {k: hashlib.sha256(t.detach().cpu().reshape(-1).view(torch.uint8).numpy().tobytes()).hexdigest()
               for k, t in tensors.items() if t is not None}
        ledger[name] = {"sha256": sha, "launches": {k: len(v) for k, v in sorted(ops.TIMER.records.items())},
                        "labels": list(labels)}

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

    H3, WIDE, NARROW = "32x0e+32x1o+32x2e", "160x0e+160x1o", "32x0e+32x1o"

    def o3_linear(irr_in, irr_out, biases=False, residual=False, live_out=None):    # (f) o3.Linear
        torch.manual_seed(11)
        lin = o3.Linear(irr_in, irr_out, biases=biases).to(DEV)
        if live_out is not None:
            lin.set_live(None, live_out)
        x = rand(33, lin.irreps_in.dim, seed=12, grad=True)
        r = rand(33, lin.irreps_out.dim, seed=13, grad=True) if residual else None
        y = lin(x, residual=r, live=live_out is not None)
        y.backward(rand(*y.shape, seed=14))
        return grads(lin, {"y": y, "grad.x": x.grad, "grad.residual": None if r is None else r.grad})

    def o3_mailbox():                                       # the layer residual through two linears
        torch.manual_seed(15)
        up, down = o3.Linear(NARROW, WIDE).to(DEV), o3.Linear(WIDE, NARROW, biases=True).to(DEV)
        h, mb = rand(33, 128, seed=16, grad=True), o3.GradMailbox()
        y = down(up(h, grad_mailbox=mb), residual=h, grad_mailbox=mb)
        y.backward(rand(*y.shape, seed=17))
        out = {"y": y, "grad.h": h.grad}
        out.update({"up." + k: v for k, v in grads(up, {}).items()})
        out.update({"down." + k: v for k, v in grads(down, {}).items()})
        return out

    for biases in (False, True):
        record(f"f/o3.Linear/k32/biases{int(biases)}", lambda: o3_linear(H3, H3, biases))
    record("f/o3.Linear/k160", lambda: o3_linear(WIDE, NARROW, True))
    record("f/o3.Linear/k160/residual", lambda: o3_linear(WIDE, NARROW, True, residual=True))
    record("f/o3.Linear/k160/mailbox", o3_mailbox)
    record("f/o3.Linear/k32/live_out", lambda: o3_linear(H3, H3, True, True, ((0, 0, 32), (2, 0, 32))))

    def dense_linear(cls, k, n_out, n):                     # (g) dense.Linear / SmallInLinear
        torch.manual_seed(21)
        lin = cls(k, n_out).to(DEV)
        x = rand(n, k, seed=22, grad=cls is dense.Linear)
        y = lin(x)
        y.backward(rand(*y.shape, seed=23))
        return grads(lin, {"y": y, "grad.x": x.grad})

    for k, n_out, n in ((128, 64, 33), (128, 64, 4097), (128, 128, 33), (48, 40, 33)):
        record(f"g/dense.Linear/{k}to{n_out}/n{n}", lambda: dense_linear(dense.Linear, k, n_out, n))
    record("g/dense.SmallInLinear/3to32/n33", lambda: dense_linear(dense.SmallInLinear, 3, 32, 33))

    def gate(live):                                         # (h) the readout Gate
        g = o3.Gate("16x0e", "16x0e", "8x1o+8x2e")
        if live:
            g.set_live(gated=(0,))
        x = rand(5, g.live.in_dim if live else g.irreps_in.dim, seed=31, grad=True)
        y = g(x, live=live)
        y.backward(rand(*y.shape, seed=32))
        return {"y": y, "grad.x": x.grad}

    for live in (False, True):
        record(f"h/Gate/live{int(live)}", lambda: gate(live))

    rowptr = torch.tensor([0, 3, 3, 8, 9, 14, 15, 20], dtype=torch.int32).to(DEV)   # (i) ops.py
    perm = torch.randperm(20, generator=torch.Generator().manual_seed(41)).to(torch.int32).to(DEV)

    def seg_sum(width, dtype, idx):
        return {"out": ops.segment_sum_csr(rand(20, width, seed=42, dtype=dtype), rowptr, 7, idx=idx)}

    def seg_order(reduce):
        src = rand(20, 6, seed=43, grad=True)
        out = ops.segment_order(src, rowptr, 7, reduce)
        out.backward(rand(7, 6, seed=44))
        return {"out": out, "grad.src": src.grad}

    def symcon_table():
        torch.manual_seed(45)
        hid = "16x0e+16x1o+16x2e"
        sc = SymmetricContraction(hid, hid, 4).to(DEV)
        x, coef = rand(33, 16 * 9, seed=46, grad=True), sc.coefficients().detach().requires_grad_(True)
        y = ops.symmetric_contraction_table(x, coef, sc._table)
        y.backward(rand(*y.shape, seed=47))
        return {"y": y, "grad.x": x.grad, "grad.coef": coef.grad}

    def symcon_coef():
        torch.manual_seed(48)
        sc = SymmetricContraction(HID4, HID4, 3).to(DEV)
        coef = sc.coefficients()
        coef.backward(rand(*coef.shape, seed=49))
        return grads(sc, {"coef": coef})

    def sum_rows():
        wide, out = rand(9, 20, seed=51), torch.zeros(7, device=DEV)
        ops.sum_rows(wide[:, 11:18], out=out, scale=0.5)
        return {"contiguous3d": ops.sum_rows(rand(5, 3, 7, seed=50)), "strided": ops.sum_rows(wide[:, 4:11]),
                "out": out}

    def embed(geometry):
        b = collate([ds[0], ds[1]]).to(DEV)
        csr = EnergyEquivGNN.edge_graph(b)
        b.positions.requires_grad_(geometry)
        sh, feats = ops.edge_embed(b.positions, csr, b.shifts[csr.perm], b.edge_attr[csr.perm].reshape(-1),
                                   4, 6, 0.6, ds.max_edge_radius)
        if geometry:
            ((sh * rand(*sh.shape, seed=52)).sum() + (feats * rand(*feats.shape, seed=53)).sum()).backward()
        return {"sh": sh, "feats": feats, "grad.positions": b.positions.grad}

    for width in (6, 260):
        for tag, dtype, idx in (("fp32", torch.float32, None), ("bf16", torch.bfloat16, None),
                                ("idx", torch.float32, perm)):
            record(f"i/segment_sum_csr/{width}/{tag}", lambda: seg_sum(width, dtype, idx))
    for reduce in ("max", "min", "mul"):
        record(f"i/segment_order/{reduce}", lambda: seg_order(reduce))
    record("i/symmetric_contraction_table", symcon_table)
    record("i/split_bf16x3", lambda: {"parts": ops.split_bf16x3(rand(33, 7, seed=54))})
    record("i/sum_rows", sum_rows)
    record("i/symcon_coefficients", symcon_coef)
    for geometry in (False, True):
        record(f"i/edge_embed/geometry{int(geometry)}", lambda: embed(geometry))

    def adamw():                                            # (j) two fused optimizer steps
        ps = [torch.nn.Parameter(rand(*shape, seed=60 + i)) for i, shape in enumerate(((5, 3), (8,), (4, 4)))]
        opt = FlatAdamW(ps, lr=1e-2, max_norm=1.0)
        for it in range(2):
            for i, p in enumerate(ps):
                p.grad = rand(*p.shape, seed=70 + 3 * it + i)
            opt.step()
        out = {f"p{i}": p for i, p in enumerate(ps)}
        out.update(m=opt.flat_m, v=opt.flat_v, state=opt._row())
        return out

    record("j/FlatAdamW", adamw)

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(ledger, f, indent=1, sort_keys=True)
    print(f"{len(ledger)} cases -> {args.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
