"""Even-parity hidden irreps on the HIP path (``tpB_l2_h02``, ``tpB_l3_h02``, ``tpB_l4_h024``)
against the fp64 CPU oracle.  The CPU part is ``test_even_hidden.py``.

Bounds are the project's standing ones (tests/test_gpu_parity.py, test_gpu_geometry.py,
test_gpu_bf16.py):
* kernel and block level: max |dev - ref| <= 1e-5 of the reference's largest entry;
* model level, fp32: stiffness and loss <= 1e-4, every parameter gradient <= 1e-5 of its own
  largest entry; geometry gradients <= 1e-5;
* bf16 storage (mul 32): kernels against the fp32 kernels fed the same bf16-rounded weights
  <= 1e-2; model against the oracle 2e-2 (stiffness, loss, every parameter gradient relative
  to its own largest entry), the bf16 bound of tests/test_gpu_bf16.py.
Shapes are the smallest at which these kernels take every path: E = 1 / 129 / 300 edges on 50
nodes (partial half-wave blocks, a node without in-edges = an empty receiver segment, a node
without out-edges = an empty sender segment, the pad row), and 3 nodes without any edge.
Every output buffer of a direct C-ABI call starts as NaN."""
import functools

import pytest
import torch

from helpers import batch, batch_to, copy_params, params, record_parity

import oracle.blocks as ob
import oracle.mace as omace
import oracle.model as omodel
import oracle.o3 as oo3
from oracle.train import stiffness_loss as oracle_loss

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-5
INV = 0.25

SETS = {"tpB_l2_h02": (2, (0, 2)), "tpB_l3_h02": (3, (0, 2)), "tpB_l4_h024": (4, (0, 2, 4))}
KERNEL_CASES = [("tpB_l2_h02", 32), ("tpB_l3_h02", 32), ("tpB_l4_h024", 32), ("tpB_l2_h02", 16),
                ("tpB_l4_h024", 64)]
GRAPHS = [(50, 1), (50, 129), (50, 300), (3, 0)]


def rel_err(a, b):
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    assert a.shape == b.shape, (a.shape, b.shape)
    if b.numel() == 0:                      # E = 0: the edge-sized outputs are empty
        return 0.0
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def irreps_of(ls, mul):
    return "+".join(f"{mul}x{l}{'e' if l % 2 == 0 else 'o'}" for l in ls)


def set_name(name, mul):
    return name if mul == 32 else f"{name}_m{mul}"


@functools.lru_cache(maxsize=None)
def graph(n, e):
    """``e`` directed edges without self loops on ``n`` nodes; for n = 50 node 48 receives
    nothing and node 49 sends nothing"""
    gen = torch.Generator().manual_seed(100 * n + e)
    if e == 0:
        return torch.zeros(2, 0, dtype=torch.long)
    send_pool = torch.arange(n - 1)                                        # never n - 1
    recv_pool = torch.tensor([i for i in range(n) if i != n - 2])          # never n - 2
    s = send_pool[torch.randint(len(send_pool), (e,), generator=gen)]
    r = recv_pool[torch.randint(len(recv_pool), (e,), generator=gen)]
    r = torch.where(r == s, (r + 1) % (n - 2), r)
    ei = torch.stack([s, r])
    assert (n - 2) not in ei[1] and (n - 1) not in ei[0] and not bool((ei[0] == ei[1]).any())
    return ei


@functools.lru_cache(maxsize=None)
def tp_reference(name, mul, n, e):
    """fp64: the oracle's TensorProduct over the edges + the receiver sum / norm, and its
    gradients for a random cotangent (computed once per case, shared, never written to)"""
    lmax, ls = SETS[name]
    node, sh_ir = oo3.Irreps(irreps_of(ls, mul)), oo3.Irreps.spherical_harmonics(lmax)
    target = (sh_ir * mul).sort()[0].simplify()
    mid, instr = omace.tp_out_irreps_with_instructions(node, sh_ir, target)
    tp = oo3.TensorProduct(node, sh_ir, mid, instr).double()
    gen = torch.Generator().manual_seed(7 * n + e + mul)
    ei = graph(n, e)
    x = torch.randn(n, node.dim, generator=gen, dtype=torch.float64, requires_grad=True)
    vec = torch.randn(e, 3, generator=gen, dtype=torch.float64)
    sh = oo3.spherical_harmonics(lmax, vec).detach().requires_grad_(True)
    w = torch.randn(e, tp.weight_numel, generator=gen, dtype=torch.float64, requires_grad=True)
    g = torch.randn(n, mid.dim, generator=gen, dtype=torch.float64)
    if e:
        agg = INV * torch.zeros(n, mid.dim, dtype=torch.float64).index_add_(0, ei[1], tp(x[ei[0]], sh, w))
        gx, gsh, gw = torch.autograd.grad(agg, [x, sh, w], g)
    else:
        agg, gx, gsh, gw = torch.zeros(n, mid.dim), torch.zeros(n, node.dim), sh.detach(), w.detach()
    return dict(ei=ei, x=x.detach(), sh=sh.detach(), w=w.detach(), g=g, agg=agg.detach(), gx=gx, gsh=gsh,
                gw=gw, dims=(node.dim, mid.dim, tp.weight_numel, sh_ir.dim))


def device_case(name, mul, n, e):
    from gnn import _lib, ops
    ref = tp_reference(name, mul, n, e)
    idx, info, _ = _lib.tp_config(set_name(name, mul))
    assert (info["din"], info["dmid"], info["wn"], info["nsh"]) == ref["dims"]
    csr = ops.EdgeCSR.build(ref["ei"].to(DEV), n)
    perm = csr.perm.cpu()
    nsh, nshp = info["nsh"], ops.sh_row_stride(info["nsh"])
    sh = torch.zeros(e, nshp, device=DEV)
    sh[:, :nsh] = ref["sh"][perm].float().to(DEV)
    x = ref["x"].float().to(DEV).contiguous()
    w = ref["w"][perm].float().to(DEV).contiguous()
    g = ref["g"].float().to(DEV).contiguous()
    return ref, idx, info, csr, perm, x, sh, w, g


def nan(*shape, dtype=torch.float32):
    return torch.full(shape, float("nan"), device=DEV, dtype=dtype)


@pytest.mark.parametrize("n,e", GRAPHS)
@pytest.mark.parametrize("name,mul", KERNEL_CASES)
def test_tp_kernels_match_the_oracle(name, mul, n, e):
    """tp_fwd, tp_bwd (grad_w; grad_x after the sender sum), tp_bws and tp_bwd_sh of a new set
    through the C ABI, 1e-5 of the largest entry of the fp64 reference"""
    from gnn import _lib, ops
    ref, idx, info, csr, perm, x, sh, w, g = device_case(name, mul, n, e)
    lib = _lib.load()
    din, dmid, wn, nsh = ref["dims"]
    st = _lib.stream(x)
    agg = nan(n, dmid)
    _lib.check(lib.eelg_tp_fwd(idx, _lib.ptr(x), _lib.ptr(sh), _lib.ptr(w), _lib.ptr(csr.sender),
                               _lib.ptr(csr.rowptr), n, INV, _lib.ptr(agg), st), "tp_fwd")
    gw, gxe = nan(e, wn), nan(e, din)
    _lib.check(lib.eelg_tp_bwd(idx, _lib.ptr(x), _lib.ptr(sh), _lib.ptr(w), _lib.ptr(csr.sender),
                               _lib.ptr(csr.receiver), e, _lib.ptr(g), INV, _lib.ptr(gw), _lib.ptr(gxe),
                               st), "tp_bwd")
    gx = ops.segment_sum_csr(gxe, csr.srowptr, n, idx=csr.sperm)
    gws, gxs = nan(e, wn), nan(n, din)
    _lib.check(lib.eelg_tp_bwd_sender(idx, _lib.ptr(x), _lib.ptr(sh), _lib.ptr(w), _lib.ptr(csr.sperm),
                                      _lib.ptr(csr.srowptr), _lib.ptr(csr.receiver), n, _lib.ptr(g), INV,
                                      _lib.ptr(gws), _lib.ptr(gxs), st), "tp_bwd_sender")
    gsh = nan(e, sh.shape[1])
    _lib.check(lib.eelg_tp_bwd_sh(idx, _lib.ptr(x), None, _lib.ptr(w), _lib.ptr(csr.sender),
                                  _lib.ptr(csr.receiver), e, _lib.ptr(g), INV, _lib.ptr(gsh), st), "tp_bwd_sh")
    torch.cuda.synchronize()
    for t in (agg, gw, gxe, gx, gws, gxs, gsh):
        assert torch.isfinite(t).all()
    errs = dict(fwd=rel_err(agg, ref["agg"]), bwd_gw=rel_err(gw, ref["gw"][perm]), bwd_gx=rel_err(gx, ref["gx"]),
                bws_gw=rel_err(gws, ref["gw"][perm]), bws_gx=rel_err(gxs, ref["gx"]),
                bwd_sh=rel_err(gsh[:, :nsh], ref["gsh"][perm]))
    print(f"{set_name(name, mul)} N {n} E {e}: {errs}")
    record_parity(f"even_kernel_{set_name(name, mul)}_n{n}_e{e}", **errs)
    for k, v in errs.items():
        assert v < TOL, (k, v)
    assert torch.equal(gsh[:, nsh:], torch.zeros_like(gsh[:, nsh:]))       # pad columns
    if n == 50:
        assert torch.equal(agg[n - 2], torch.zeros_like(agg[0]))           # no in-edge
        assert torch.equal(gxs[n - 1], torch.zeros_like(gxs[0]))           # no out-edge
        assert torch.equal(gx[n - 1], torch.zeros_like(gx[0]))


def test_config_indices_and_the_fused_backward():
    """the new sets follow every earlier set in the lookup (earlier indices unchanged), carry no
    fused backward (the library's usual error, and ``tp_linear_fusable`` False), and serve the
    bf16 entry points at mul 32 only"""
    from gnn import _lib, cg, ops
    from gnn.blocks import TensorProductInteractionBlock
    from gnn.irreps import Irreps
    lib = _lib.load()
    old = [f"tp{a}_l{lmax}{sfx}" for sfx in ("", "_m16", "_m64") for lmax in (1, 2, 3, 4) for a in "AB"]
    assert [lib.eelg_tp_find(nm.encode()) for nm in old] == list(range(24))
    new = [set_name(nm, mul) for mul in (32, 16, 64) for nm in SETS]
    assert [lib.eelg_tp_find(nm.encode()) for nm in new] == list(range(24, 33))
    for nm in new:
        idx = lib.eelg_tp_find(nm.encode())
        assert lib.eelg_tp_bwf_slot(idx, 0, None, None, None) == -2
        assert lib.eelg_tp_bwd_fused(idx, *([None] * 6), 0, None, None, INV, None, None, None) == -2
        assert lib.eelg_tp_bwd_fused_bf16(idx, *([None] * 6), 0, None, None, INV, None, None, None) == -2
        assert b"not generated" in lib.eelg_last_error()
        if nm.endswith(("_m16", "_m64")):       # bf16 storage: mul 32 only, an error before any launch
            assert lib.eelg_tp_fwd_bf16(idx, *([None] * 5), 4, INV, None, None) == -2
    sh = Irreps.spherical_harmonics(4)
    blk = TensorProductInteractionBlock("32x0e+32x2e+32x4e", sh, "12x0e", (sh * 32).sort()[0].simplify(), 4.0)
    idx, info = blk._config()
    assert idx == lib.eelg_tp_find(b"tpB_l4_h024") and info["npaths"] == 24 and info["wn"] == 768
    assert info["din"] == 480 and info["dmid"] == 4288
    assert ops.tp_linear_fusable(idx, blk.linear, cg.tp_paths(blk.irreps_in, sh, blk.irreps_out)) is False
    assert blk._bwf(idx) is False


@pytest.mark.parametrize("name", list(SETS))
def test_tp_bf16_storage_matches_the_fp32_kernels(name):
    """the ``_bw`` kernels (forward, edge-order and sender-order backward) against the fp32
    kernels fed the same bf16-rounded weights: 1e-2 (tests/test_gpu_bf16.py)"""
    from gnn import ops
    n, e = 50, 300
    ref, idx, info, csr, perm, x, sh, w, g = device_case(name, 32, n, e)
    wb = w.to(torch.bfloat16)
    sh = sh[:, :info["nsh"]]
    saved = ops.TP_BWD_SENDER
    out = {}
    try:
        for key, ww, sender in (("f32", wb.float(), False), ("bf_edge", wb, False), ("bf_sender", wb, True)):
            ops.TP_BWD_SENDER = sender
            xx = x.clone().requires_grad_(True)
            ww = ww.clone().requires_grad_(True)
            agg = ops.tp_interaction(xx, sh, ww, csr, idx, info, INV)
            (agg * g).sum().backward()
            out[key] = (agg.detach(), xx.grad, ww.grad)
    finally:
        ops.TP_BWD_SENDER = saved
    a32, gx32, gw32 = out["f32"]
    for key in ("bf_edge", "bf_sender"):
        a, gx, gw = out[key]
        assert gw.dtype == torch.bfloat16 and a.dtype == torch.float32 and gx.dtype == torch.float32
        errs = dict(fwd=rel_err(a, a32), grad_x=rel_err(gx, gx32), grad_w=rel_err(gw, gw32))
        print(f"{name} bf16 {key}: {errs}")
        record_parity(f"even_bf16_{name}_{key}", **errs)
        for k, v in errs.items():
            assert v < 1e-2, (key, k, v)


# ---------------------------------------------------------------------------
# block level
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("reduction", ["sum", "add", "mean", "max", "min", "mul"])
def test_interaction_block_every_reduction(reduction):
    """TensorProductInteractionBlock, lmax 2, hidden 32x0e+32x2e, E = 300 (one node without
    in-edges: the empty segment of max / min / mul)"""
    from gnn.blocks import REDUCTIONS, TensorProductInteractionBlock
    assert reduction in REDUCTIONS and len(REDUCTIONS) == 6
    n, e, lmax = 50, 300, 2
    hid, sh_ir = irreps_of((0, 2), 32), oo3.Irreps.spherical_harmonics(lmax)
    target = str((sh_ir * 32).sort()[0].simplify())
    torch.manual_seed(0)
    o = ob.TensorProductInteractionBlock(hid, sh_ir, "12x0e", target, 4.0, reduction, True).double()
    m = TensorProductInteractionBlock(hid, str(sh_ir), "12x0e", target, 4.0, reduction, True).to(DEV)
    copy_params(o, m)
    ei = graph(n, e)
    gen = torch.Generator().manual_seed(3)
    x = torch.randn(n, 192, generator=gen, dtype=torch.float64)
    sh = oo3.spherical_harmonics(lmax, torch.randn(e, 3, generator=gen, dtype=torch.float64))
    ef = torch.rand(e, 12, generator=gen, dtype=torch.float64)
    xo = x.clone().requires_grad_(True)
    yo, _ = o(xo, sh, ef, ei)
    go = torch.randn(yo.shape, generator=gen, dtype=torch.float64)
    (yo * go).sum().backward()
    xm = x.float().to(DEV).requires_grad_(True)
    ym, _ = m(xm, sh.float().to(DEV), ef.float().to(DEV), ei.to(DEV))
    (ym * go.float().to(DEV)).sum().backward()
    po = dict(o.named_parameters())
    errs = dict(out=rel_err(ym, yo), grad_x=rel_err(xm.grad, xo.grad),
                grad_params=max(rel_err(pm.grad, po[k].grad) for k, pm in m.named_parameters()))
    print(f"even interaction block {reduction}: {errs}")
    record_parity(f"even_block_{reduction}", **errs)
    assert all(pm.grad is not None for pm in m.parameters())
    for k, v in errs.items():
        assert v < TOL, (k, v)


@functools.lru_cache(maxsize=None)
def _product_pair():
    full, even = irreps_of(range(5), 32), irreps_of((0, 2, 4), 32)
    from gnn.blocks import EquivariantProductBlock
    torch.manual_seed(1)
    o = ob.EquivariantProductBlock(full, even, 3, use_sc=False).double()
    m = EquivariantProductBlock(full, even, 3, use_sc=False).to(DEV)
    copy_params(o, m)
    return o, m


@pytest.mark.parametrize("n", [1, 129, 2051])
def test_product_block_with_even_outputs_as_its_own_set(n):
    """EquivariantProductBlock(interaction irreps -> 32x0e+32x2e+32x4e, correlation 3): the
    contraction runs ``sc_l4_c3_o024`` as the module's only set.  n = 2051: two node ranges of
    the streaming coefficient gradient (ranges taken from the full set's term-group sets)."""
    from gnn import _lib
    o, m = _product_pair()
    sc = m.symmetric_contractions
    idx, info = sc._config()
    assert sc._live is None and _lib.sc_outputs(idx) == (0, 2, 4)
    assert idx == _lib.sc_config("sc_l4_c3_o024")[0]
    full_idx = _lib.sc_config("sc_l4_c3")[0]
    lib = _lib.load()
    assert lib.eelg_sc_bwd_coef_parts(idx, n, 32) == lib.eelg_sc_bwd_coef_parts(full_idx, n, 32)
    assert lib.eelg_sc_bwd_coef_parts(idx, n, 32) == (2 if n == 2051 else 1)
    for p in list(o.parameters()) + list(m.parameters()):
        p.grad = None
    gen = torch.Generator().manual_seed(n)
    x = torch.randn(n, 800, generator=gen, dtype=torch.float64)
    xo = x.clone().requires_grad_(True)
    yo = o(xo, None)
    go = torch.randn(yo.shape, generator=gen, dtype=torch.float64)
    (yo * go).sum().backward()
    xm = x.float().to(DEV).requires_grad_(True)
    ym = m(xm, None)
    assert ym.shape == (n, 480)
    (ym * go.float().to(DEV)).sum().backward()
    torch.cuda.synchronize()
    po = dict(o.named_parameters())
    gerr = {k: rel_err(pm.grad, po[k].grad) for k, pm in m.named_parameters()}
    errs = dict(out=rel_err(ym, yo), grad_x=rel_err(xm.grad, xo.grad),
                grad_coef=max(v for k, v in gerr.items() if "contractions" in k),
                grad_linear=max(v for k, v in gerr.items() if "contractions" not in k))
    print(f"even product block n {n}: {errs}")
    record_parity(f"even_product_n{n}", **errs)
    for k, v in errs.items():
        assert v < TOL, (k, v)


# ---------------------------------------------------------------------------
# model level
# ---------------------------------------------------------------------------
MODEL_CASES = [  # (lmax, hidden l, mul, readout: "even" | "full", correlation, storage)
    (4, (0, 2, 4), 32, "even", 3, "float32"),
    (4, (0, 2, 4), 32, "full", 3, "float32"),
    (3, (0, 2), 32, "even", 3, "float32"),
    (3, (0, 2), 32, "even", 3, "bfloat16"),
    (2, (0, 2), 16, "even", 3, "float32"),
    (2, (0, 2), 64, "even", 3, "float32"),
    (2, (0, 2), 32, "even", 1, "float32"),
    (2, (0, 2), 32, "full", 2, "float32"),
]


def _params(lmax, ls, mul, readout, corr, rmax, **kw):
    return params(2, lmax=lmax, correlation=corr, max_edge_radius=rmax, hidden_irreps=irreps_of(ls, mul),
                  readout_irreps=irreps_of(ls if readout == "even" else range(lmax + 1), 16), **kw)


@pytest.mark.parametrize("lmax,ls,mul,readout,corr,storage", MODEL_CASES)
def test_model_matches_the_oracle_and_overlap_is_bitwise(lmax, ls, mul, readout, corr, storage):
    from gnn import ops
    from gnn.model import EnergyEquivGNN
    from gnn.train import stiffness_loss
    b, rmax = batch(2, 12, 40)
    bd = b.to(DEV)
    p = _params(lmax, ls, mul, readout, corr, rmax)
    torch.manual_seed(0)
    o = omodel.EnergyEquivGNN(p).double()
    bo = batch_to(b, "cpu", torch.float64)
    co = o(bo)["stiffness"]
    lo = oracle_loss(co, bo.stiffness)
    lo.backward()
    p.storage_dtype = storage
    saved = ops.OVERLAP
    runs = {}
    try:
        # one model per mode: a parameter's gradient accumulator belongs to the stream of its
        # first backward
        for flag in (True, False):
            ops.OVERLAP = flag
            m = EnergyEquivGNN(p).to(DEV)
            copy_params(o, m)
            assert m.stiffness_head.live_pruned is False
            cm = m(bd)["stiffness"]
            lm = stiffness_loss(cm, bd.stiffness)
            lm.backward()
            torch.cuda.synchronize()
            runs[flag] = (m, cm.detach(), lm.detach())
    finally:
        ops.OVERLAP = saved
    m, cm, lm = runs[True]
    po = dict(o.named_parameters())
    assert all(q.grad is not None for q in m.parameters())
    assert all(torch.isfinite(q.grad).all() for q in m.parameters())
    gerr = {k: rel_err(q.grad, po[k].grad) for k, q in m.named_parameters()}
    worst = max(gerr, key=gerr.get)
    errs = dict(stiffness=rel_err(cm, co), loss=abs(lm.item() - lo.item()) / abs(lo.item()),
                grad_params=gerr[worst])
    print(f"even model lmax {lmax} mul {mul} readout {readout} corr {corr} {storage}: {errs} ({worst})")
    record_parity(f"even_model_l{lmax}_m{mul}_{readout}_c{corr}_{storage}", **errs)
    bf = storage == "bfloat16"
    assert errs["stiffness"] < (2e-2 if bf else 1e-4)
    assert errs["loss"] <= (2e-2 if bf else 1e-4)
    for k, v in gerr.items():
        assert v < (2e-2 if bf else TOL), (k, v)
    # stream overlap on == in line, bitwise
    m0, c0, l0 = runs[False]
    assert torch.equal(c0, cm) and torch.equal(l0, lm)
    for (k, q), q0 in zip(m.named_parameters(), m0.parameters()):
        assert torch.equal(q.grad, q0.grad), k


def test_stiffness_sensitivity_of_the_even_model():
    """positions, radii and shifts within 1e-5 of the oracle's autograd for a random cotangent
    (lmax 4, 32x0e+32x2e+32x4e); the position gradient sums to zero per graph (translation
    invariance) within 1e-5 of its largest entry"""
    from gnn import EnergyEquivGNN, stiffness_sensitivity
    geom = ("positions", "edge_attr", "shifts")
    b, rmax = batch(2, 12, 40)
    p = _params(4, (0, 2, 4), 32, "even", 3, rmax)
    torch.manual_seed(0)
    o = omodel.EnergyEquivGNN(p).double()
    m = EnergyEquivGNN(p).to(DEV)
    copy_params(o, m)
    bo = batch_to(b, "cpu", torch.float64)
    for k in geom:
        setattr(bo, k, getattr(bo, k).detach().clone().requires_grad_(True))
    co = o(bo)["stiffness"]
    cot = torch.randn(co.shape, generator=torch.Generator().manual_seed(11), dtype=torch.float64)
    ref = torch.autograd.grad(co, [getattr(bo, k) for k in geom], grad_outputs=cot)
    bd = b.to(DEV)
    out = stiffness_sensitivity(m, bd, cot.float().to(DEV))
    errs = {k: rel_err(out[k], r) for k, r in zip(geom, ref)}
    gp = out["positions"]
    per_graph = torch.zeros(bd.num_graphs, 3, device=DEV).index_add_(0, bd.batch, gp)
    errs["translation"] = float(per_graph.abs().max() / gp.abs().max())
    print(f"even stiffness_sensitivity: stiffness {rel_err(out['stiffness'], co):.2e} {errs}")
    record_parity("even_stiffness_sensitivity", stiffness=rel_err(out["stiffness"], co), **errs)
    assert rel_err(out["stiffness"], co) < 1e-4
    for k, v in errs.items():
        assert v <= TOL, (k, v)
    for k in geom:
        assert out[k].shape == getattr(bd, k).shape
    assert all(q.grad is None for q in m.parameters())


def test_state_dict_round_trip_on_the_device():
    """the reference's U_matrix_* buffers of the even outputs are emitted and load back strictly"""
    from gnn.model import EnergyEquivGNN
    p = _params(2, (0, 2), 32, "even", 2, 0.05)
    torch.manual_seed(0)
    o = omodel.EnergyEquivGNN(p)
    m = EnergyEquivGNN(p).to(DEV)
    sd = m.state_dict()
    assert set(sd) == set(o.state_dict())
    assert sum("U_matrix_" in k for k in sd) == 2 * 2 * 2
    m.load_state_dict(sd, strict=True)
    m.load_state_dict(o.state_dict(), strict=True)
    o.load_state_dict(sd, strict=True)


def test_unsupported_list_raises_at_construction():
    """(0, 2) at lmax 4 is no generated list: NotImplementedError when the model is built (on
    the host, before any launch), naming the supported lists"""
    from gnn.model import EnergyEquivGNN
    with pytest.raises(NotImplementedError) as ei:
        EnergyEquivGNN(params(2, lmax=4, hidden_irreps="32x0e+32x2e", readout_irreps="16x0e+16x2e"))
    assert "32x0e+32x2e+32x4e" in str(ei.value)
