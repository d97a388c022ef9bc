"""'pna' interaction reduction on the device (``eelg_segment_pna_fwd`` / ``_bwd``,
``ops.segment_pna``, the interaction block and the model) against the fp64 restatement of
``tests/helpers_pna.py``.

Tolerances: 1e-5 of the largest entry for a kernel against fp64 on the same fp32 inputs (DESIGN
section 2's per-kernel tolerance), 1e-6 between the two fp32 implementations and on the exactly
representable tie data, 1e-4 for the model's stiffness (the model tolerance of the other
reductions).
"""
import ctypes
import functools

import pytest
import torch

from helpers import batch, batch_to, copy_params, params, record_parity
from helpers_pna import (first_extremes, pna_aggregates, pna_oracle_block, pna_oracle_model, pna_ref)

import oracle.mace as omace
import oracle.model as omodel
import oracle.o3 as oo3
from oracle.train import stiffness_loss as oracle_loss

pytestmark = pytest.mark.gpu
DEV = "cuda"
SIZES = [3, 0, 5, 1, 4, 0, 2, 70, 1, 6]     # empty, single, far longer than a wave, last non-empty
AVG_LOG = 1.6


def rel_err(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def _segments():
    sizes = torch.tensor(SIZES)
    rowptr = torch.zeros(len(SIZES) + 1, dtype=torch.int32)
    rowptr[1:] = torch.cumsum(sizes, 0)
    index = torch.repeat_interleave(torch.arange(len(SIZES)), sizes)
    return rowptr, index


@functools.lru_cache(maxsize=None)
def _case(width, ties=False):
    """inputs (fp32, CPU) and the fp64 restatement's out / grad_src / grad W, computed once"""
    rowptr, index = _segments()
    n, e = len(SIZES), int(rowptr[-1])
    gen = torch.Generator().manual_seed(100 + width + (7 if ties else 0))
    if ties:
        src = (torch.randint(-2, 3, (e, width), generator=gen).float() * 0.5)
    else:
        src = torch.randn(e, width, generator=gen)
    w = torch.randn(1, 12, generator=gen)
    g = torch.randn(n, width, generator=gen)
    route = first_extremes(src.double(), index, n) if ties else None
    xs, ws = src.double().requires_grad_(True), w.double().requires_grad_(True)
    out = pna_ref(xs, index, n, ws, AVG_LOG, route)
    out.backward(g.double())
    return dict(rowptr=rowptr, index=index, n=n, src=src, w=w, g=g, route=route,
                out=out.detach(), grad_src=xs.grad, grad_w=ws.grad)


def _run(c, fused=True, monkeypatch=None):
    from gnn import ops
    if monkeypatch is not None:
        monkeypatch.setattr(ops, "PNA_FUSED", fused)
    src = c["src"].to(DEV).requires_grad_(True)
    w = c["w"].to(DEV).requires_grad_(True)
    args = ops.PNAArgs()
    out = ops.segment_pna(src, c["rowptr"].to(DEV), c["n"], w, AVG_LOG, args=args)
    out.backward(c["g"].to(DEV))
    torch.cuda.synchronize()
    return out.detach(), src.grad, w.grad, args


def _abi(c):
    """both entry points called directly on NaN-poisoned output buffers"""
    from gnn import _lib, ops
    lib = _lib.load()
    src, g = c["src"].to(DEV), c["g"].to(DEV)
    rowptr = c["rowptr"].to(DEV)
    n, width = c["n"], src.shape[1]
    coef = (ops.pna_scalers(rowptr, AVG_LOG)[:, None, :] * c["w"].to(DEV).view(4, 3)[None]).sum(-1).contiguous()
    nan = float("nan")
    out, mean, std = (torch.full((n, width), nan, device=DEV) for _ in range(3))
    amin, amax = (torch.full((n, width), -7, device=DEV, dtype=torch.int32) for _ in range(2))
    _lib.check(lib.eelg_segment_pna_fwd(_lib.ptr(src), _lib.ptr(rowptr), _lib.ptr(coef), n, width,
                                        _lib.ptr(out), _lib.ptr(mean), _lib.ptr(std), _lib.ptr(amin),
                                        _lib.ptr(amax), _lib.stream(out)), "segment_pna_fwd")
    parts = lib.eelg_segment_pna_parts(width)
    gs = torch.full_like(src, nan)
    part = torch.full((parts, n * 4), nan, device=DEV)
    _lib.check(lib.eelg_segment_pna_bwd(_lib.ptr(src), _lib.ptr(rowptr), _lib.ptr(coef), _lib.ptr(mean),
                                        _lib.ptr(std), _lib.ptr(amin), _lib.ptr(amax), _lib.ptr(g), n, width,
                                        _lib.ptr(gs), _lib.ptr(part), _lib.stream(gs)), "segment_pna_bwd")
    torch.cuda.synchronize()
    return dict(out=out, mean=mean, std=std, amin=amin, amax=amax, gs=gs, part=part, parts=parts)


@pytest.mark.parametrize("width", [21, 64, 7360])
def test_kernels_match_fp64(width):
    """scalar form (21), float4 form in one span (64) and in several spans with the partials
    summed (7360): out, grad_src and grad W against fp64 on the same fp32 data"""
    c = _case(width)
    out, gs, gw, args = _run(c)
    raw = _abi(c)
    # every element of every output buffer is written, and the op returns what the kernels wrote
    for k in ("out", "mean", "std", "gs", "part"):
        assert torch.isfinite(raw[k]).all(), k
    assert int(raw["amin"].min()) >= -1 and int(raw["amax"].min()) >= -1
    assert torch.equal(raw["out"], out) and torch.equal(raw["gs"], gs)
    assert torch.equal(raw["amin"], args.argmin) and torch.equal(raw["amax"], args.argmax)
    assert raw["parts"] == -(-(width // 4 if width % 4 == 0 else width) // 512)
    aggs, deg = pna_aggregates(c["src"].double(), c["index"], c["n"])
    errs = dict(out=rel_err(out, c["out"]), grad_src=rel_err(gs, c["grad_src"]), grad_w=rel_err(gw, c["grad_w"]),
                mean=rel_err(raw["mean"], aggs[0]), std=rel_err(raw["std"], aggs[3]))
    print(f"segment_pna width {width}: {errs}")
    record_parity(f"segment_pna_w{width}", **errs)
    # the extremes are decided on identical values: the kept rows are the fp64 ones
    amin, amax = first_extremes(c["src"].double()[:, :8], c["index"], c["n"])
    assert torch.equal(args.argmin[:, :8].long().cpu(), amin)
    assert torch.equal(args.argmax[:, :8].long().cpu(), amax)
    empty = deg == 0
    assert (args.argmin[empty.to(DEV)] == -1).all() and (args.argmax[empty.to(DEV)] == -1).all()
    for k, v in errs.items():
        assert v < 1e-5, (k, v)


@pytest.mark.parametrize("width", [21, 64])
def test_ties_keep_the_first_extreme(width):
    """values from {-1, -0.5, 0, 0.5, 1}: argmin / argmax are the first extreme of the segment in
    CSR order, and the gradients are those of the restatement routed there"""
    c = _case(width, ties=True)
    out, gs, gw, args = _run(c)
    amin, amax = c["route"]
    assert torch.equal(args.argmin.long().cpu(), amin)
    assert torch.equal(args.argmax.long().cpu(), amax)
    errs = dict(out=rel_err(out, c["out"]), grad_src=rel_err(gs, c["grad_src"]), grad_w=rel_err(gw, c["grad_w"]))
    print(f"segment_pna ties width {width}: {errs}")
    record_parity(f"segment_pna_ties_w{width}", **errs)
    for k, v in errs.items():
        assert v < 1e-6, (k, v)


@pytest.mark.parametrize("width", [21, 64])
def test_fused_matches_the_composition(width, monkeypatch):
    c = _case(width)
    out, gs, gw, args = _run(c, True, monkeypatch)
    out0, gs0, gw0, args0 = _run(c, False, monkeypatch)
    assert torch.equal(args.argmin, args0.argmin) and torch.equal(args.argmax, args0.argmax)
    errs = dict(out=rel_err(out, out0), grad_src=rel_err(gs, gs0), grad_w=rel_err(gw, gw0))
    print(f"segment_pna fused vs composed width {width}: {errs}")
    record_parity(f"segment_pna_fused_vs_composed_w{width}", **errs)
    for k, v in errs.items():
        assert v < 1e-6, (k, v)


@pytest.mark.parametrize("width", [21, 7360])
def test_forward_and_backward_are_bitwise_repeatable(width):
    c = _case(width)
    a, b = _run(c), _run(c)
    for x, y in zip(a[:3], b[:3]):
        assert torch.equal(x, y)


def test_memory_stays_within_three_times_the_messages(monkeypatch):
    """N 2048, E 8192 (degree 4), width 256: forward + backward of the fused op allocate out and
    four saved [N, D] buffers (1.25 x src) and grad_src (1 x); the composition with its [N, D, 12]
    stack does not fit the same bound"""
    from gnn import ops
    n, deg, width = 2048, 4, 256
    rowptr = (torch.arange(n + 1, dtype=torch.int32) * deg).to(DEV)
    gen = torch.Generator().manual_seed(5)
    src = torch.randn(n * deg, width, generator=gen).to(DEV).requires_grad_(True)
    g = torch.randn(n, width, generator=gen).to(DEV)
    w = torch.randn(1, 12, generator=gen).to(DEV).requires_grad_(True)
    scalers = ops.pna_scalers(rowptr, AVG_LOG)
    bound = 3 * src.numel() * 4
    peaks = {}
    for fused in (True, False):
        monkeypatch.setattr(ops, "PNA_FUSED", fused)
        src.grad = w.grad = None
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = ops.segment_pna(src, rowptr, n, w, AVG_LOG, scalers=scalers)
        out.backward(g)
        torch.cuda.synchronize()
        peaks[fused] = torch.cuda.max_memory_allocated() - base
        del out
    print(f"segment_pna peak / src bytes: fused {peaks[True] / (bound / 3):.2f}, "
          f"composed {peaks[False] / (bound / 3):.2f}")
    record_parity("segment_pna_memory", fused=peaks[True] / (bound / 3), composed=peaks[False] / (bound / 3))
    assert peaks[True] <= bound, peaks
    assert peaks[False] > bound, peaks


def _block_inputs(b, rmax, din, seed=1):
    torch.manual_seed(seed)
    n = b.node_attrs.shape[0]
    x = torch.randn(n, din, dtype=torch.float64)
    vec, ln = omace.get_edge_vectors_and_lengths(b.positions.double(), b.edge_index, b.shifts.double())
    sh = oo3.spherical_harmonics(4, vec)
    ef = torch.cat([oo3.soft_one_hot_linspace(ln.squeeze(-1), 0, 0.6, 6),
                    oo3.soft_one_hot_linspace(b.edge_attr.double().squeeze(-1), 0, rmax, 6)], 1)
    return x, sh, ef


def _pair(b, rmax, **kw):
    """(fp64 oracle with the restated aggregation, device model) with equal parameters"""
    from gnn import degree_stats
    from gnn.model import EnergyEquivGNN
    stats = degree_stats(b.edge_index, b.node_attrs.shape[0])
    torch.manual_seed(0)
    o = omodel.EnergyEquivGNN(params(2, max_edge_radius=rmax, agg_norm_const=1.0, **kw)).double()
    pna_oracle_model(o, stats["log"])
    m = EnergyEquivGNN(params(2, max_edge_radius=rmax, interaction_reduction="pna", agg_norm_const=stats,
                              **kw)).to(DEV)
    copy_params(o, m)
    return o, m, stats


def test_interaction_block_exact_up_to_proven_ties(monkeypatch):
    """The method of ``test_gpu_api.py::test_interaction_max_min_exact_up_to_proven_ties`` for
    both extremes at once: the device's kept rows are captured, the fp32 message error ``e_msg``
    is measured, every kept row that is not the fp64 extreme must be within 2 ``e_msg`` of it, and
    forward, grad_x and every parameter gradient (``pna.post_pn.weight`` included) match the
    restatement routed through the device's kept rows at 1e-5, with no exclusions."""
    from gnn import ops
    b, rmax = batch(4, 50, 200, 1234)
    o, m, stats = _pair(b, rmax)
    o_int, m_int = o.stiffness_head.layers[1].interaction, m.stiffness_head.layers[1].interaction
    x, sh, ef = _block_inputs(b, rmax, 800)
    cap = {}
    seg_pna, per_edge = ops.segment_pna, ops.per_edge_csr

    def spy_per_edge(csr):
        cap["perm"] = csr.perm.long().cpu()
        return per_edge(csr)

    def spy_pna(src, rowptr32, n_rows, weight, avg_log, scalers=None, args=None):
        a = ops.PNAArgs()
        out = seg_pna(src, rowptr32, n_rows, weight, avg_log, scalers=scalers, args=a)
        cap.update(amin=a.argmin.long().cpu(), amax=a.argmax.long().cpu(),
                   msg_dev=src.detach().double().cpu(), avg_log=avg_log)
        return out

    monkeypatch.setattr(ops, "per_edge_csr", spy_per_edge)
    monkeypatch.setattr(ops, "segment_pna", spy_pna)
    xm = x.float().to(DEV).requires_grad_(True)
    bd = b.to(DEV)
    ym, _ = m_int(xm, sh.float().to(DEV), ef.float().to(DEV), bd.edge_index)
    torch.manual_seed(3)
    go = torch.randn(ym.shape, dtype=torch.float64)
    (ym * go.float().to(DEV)).sum().backward()
    assert cap["avg_log"] == stats["log"]

    # CSR positions -> rows of the oracle's message tensor (original edge order)
    perm = cap["perm"]
    kept = [torch.where(a >= 0, perm[a.clamp_min(0)], a) for a in (cap["amin"], cap["amax"])]
    route, ocap = {}, {}
    pna_oracle_block(o_int, stats["log"], route=route, capture=ocap)
    route["args"] = tuple(kept)
    xo = x.clone().requires_grad_(True)
    yo, _ = o_int(xo, sh, ef, b.edge_index)
    (yo * go).sum().backward()

    msg = ocap["msg"]
    e_msg = float((cap["msg_dev"] - msg[perm]).abs().max())
    scale = float(msg.abs().max())
    aggs, _ = pna_aggregates(msg, ocap["index"], kept[0].shape[0])
    worst_margin, n_flip = 0.0, 0
    for best, k in ((aggs[1], kept[0]), (aggs[2], kept[1])):
        chosen = torch.where(k >= 0, torch.gather(msg, 0, k.clamp_min(0)), torch.zeros_like(best))
        margin = (best - chosen).abs()
        worst_margin = max(worst_margin, float(margin.max()))
        n_flip += int((margin > 0).sum())
    po = dict(o_int.named_parameters())
    gerr = {name: rel_err(pm.grad, po[name].grad) for name, pm in m_int.named_parameters()}
    assert "pna.post_pn.weight" in gerr
    print(f"pna block: out {rel_err(ym, yo):.2e}, grad_x {rel_err(xm.grad, xo.grad):.2e}, params {gerr}, "
          f"e_msg {e_msg / scale:.2e}, ties {n_flip}, margin {worst_margin / scale:.2e}")
    record_parity("interaction_reduce_pna", out_routed=rel_err(ym, yo),
                  grad_x=rel_err(xm.grad, xo.grad), grad_params=max(gerr.values()),
                  msg_err=e_msg / scale, tie_set=n_flip, tie_margin_max=worst_margin / scale)
    assert e_msg < 1e-5 * scale, e_msg / scale
    assert worst_margin <= 2 * e_msg, (n_flip, worst_margin, e_msg)
    assert rel_err(ym, yo) < 1e-5
    assert rel_err(xm.grad, xo.grad) < 1e-5
    for name, e in gerr.items():
        assert e < 1e-5, (name, e)


@pytest.mark.parametrize("mul,lmax,correlation", [(32, 4, 3), (16, 2, 2)])
def test_model_trains_with_pna(mul, lmax, correlation):
    """2 layers with the batch's own degree statistics: the stiffness against the fp64
    restatement (unrouted: the value is continuous in the choice of the kept row), finite
    gradients everywhere, and an optimiser step that moves ``post_pn.weight``"""
    from gnn.train import stiffness_loss
    b, rmax = batch(4, 50, 200, 77)
    hidden = "+".join(f"{mul}x{l}{'e' if l % 2 == 0 else 'o'}" for l in range(lmax + 1))
    o, m, stats = _pair(b, rmax, lmax=lmax, correlation=correlation, hidden_irreps=hidden)
    bo = batch_to(b, "cpu", torch.float64)
    with torch.no_grad():
        co = o(bo)["stiffness"]
        lo = oracle_loss(co, bo.stiffness)
    bd = b.to(DEV)
    opt = torch.optim.AdamW(m.parameters(), lr=1e-3)
    cm = m(bd)["stiffness"]
    lm = stiffness_loss(cm, bd.stiffness)
    lm.backward()
    err = rel_err(cm, co)
    print(f"pna model mul {mul} lmax {lmax}: stiffness {err:.2e}, loss {lm.item():.6g} vs {lo.item():.6g}")
    record_parity(f"model_pna_mul{mul}_l{lmax}", stiffness=err,
                  loss=abs(lm.item() - lo.item()) / abs(lo.item()))
    assert err < 1e-4
    keys = [f"stiffness_head.layers.{i}.interaction.pna.post_pn.weight" for i in (0, 1)]
    named = dict(m.named_parameters())
    for name, p in named.items():
        assert p.grad is not None and torch.isfinite(p.grad).all(), name
    before = [named[k].detach().clone() for k in keys]
    opt.step()
    torch.cuda.synchronize()
    for k, w0 in zip(keys, before):
        assert not torch.equal(named[k].detach(), w0), k


@pytest.mark.parametrize("kw,tol", [(dict(storage_dtype="bfloat16"), 2e-2),
                                    (dict(hidden_irreps="32x0e+32x2e+32x4e"), 1e-4)])
def test_pna_composes_as_max_does(kw, tol):
    """what 'max' runs with, 'pna' runs with (the per-edge messages are the same call): bf16
    storage of the edge tensors (against the fp64 restatement at the bf16 tolerance of
    ``test_gpu_bf16.py``) and an even hidden list"""
    from gnn.train import stiffness_loss
    b, rmax = batch(4, 50, 200, 77)
    okw = {k: v for k, v in kw.items() if k != "storage_dtype"}
    o, _, stats = _pair(b, rmax, **okw)
    from gnn.model import EnergyEquivGNN
    m = EnergyEquivGNN(params(2, max_edge_radius=rmax, interaction_reduction="pna", agg_norm_const=stats,
                              **kw)).to(DEV)
    copy_params(o, m)
    with torch.no_grad():
        co = o(batch_to(b, "cpu", torch.float64))["stiffness"]
    bd = b.to(DEV)
    cm = m(bd)["stiffness"]
    stiffness_loss(cm, bd.stiffness).backward()
    err = rel_err(cm, co)
    print(f"pna model {kw}: stiffness {err:.2e}")
    record_parity("model_pna_" + "_".join(map(str, kw.values())), stiffness=err)
    assert err < tol
    for name, p in m.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), name


def test_bad_arguments_return_an_error_code():
    """null coef / out and n_rows < 0 are refused before any launch"""
    from gnn import _lib
    lib = _lib.load()
    c = _case(21)
    raw = _abi(c)
    src, rowptr = c["src"].to(DEV), c["rowptr"].to(DEV)
    coef = torch.ones(c["n"], 4, device=DEV)
    null = ctypes.c_void_p(0)
    good = [_lib.ptr(src), _lib.ptr(rowptr), _lib.ptr(coef), c["n"], 21, _lib.ptr(raw["out"]),
            _lib.ptr(raw["mean"]), _lib.ptr(raw["std"]), _lib.ptr(raw["amin"]), _lib.ptr(raw["amax"]),
            _lib.stream(src)]
    before = raw["out"].clone()
    for pos, bad in ((2, null), (5, null), (3, -1), (4, 0)):
        a = list(good)
        a[pos] = bad
        assert lib.eelg_segment_pna_fwd(*a) == -2, pos
        assert b"segment_pna_fwd" in lib.eelg_last_error()
    g = c["g"].to(DEV)
    part = torch.empty(raw["parts"], c["n"] * 4, device=DEV)
    goodb = [_lib.ptr(src), _lib.ptr(rowptr), _lib.ptr(coef), _lib.ptr(raw["mean"]), _lib.ptr(raw["std"]),
             _lib.ptr(raw["amin"]), _lib.ptr(raw["amax"]), _lib.ptr(g), c["n"], 21, _lib.ptr(raw["gs"]),
             _lib.ptr(part), _lib.stream(src)]
    for pos, bad in ((2, null), (10, null), (8, -1)):
        a = list(goodb)
        a[pos] = bad
        assert lib.eelg_segment_pna_bwd(*a) == -2, pos
        assert b"segment_pna_bwd" in lib.eelg_last_error()
    assert lib.eelg_segment_pna_parts(0) == -2
    torch.cuda.synchronize()
    assert torch.equal(raw["out"], before)
