"""Live outputs of the last layer on the device.

Kernel level: every generated live-output contraction set against the full set of the same
coupling and correlation, on the same ``x`` and coefficients -- forward = the live columns of
the full forward; grad-x and the coefficient gradient = the full set's when its ``grad_out``
is zero on the dead columns.  The two evaluate the same polynomial terms in another order, so
the bound is 1e-5 of the largest entry, not bitwise.  Output buffers are NaN before each call.

Model level: the switch on against the switch off (fresh model, same seed) and against the
fp64 oracle at the standing model tolerances (stiffness / loss 1e-4, every parameter gradient
1e-5 of its own largest entry; bf16 storage 2e-2), with the dead slices of the gradients exact
zeros and no ``.grad`` None.
"""
from __future__ import annotations

import ctypes
import functools

import pytest
import torch

import oracle.model as omodel
from oracle.train import stiffness_loss as oracle_loss

from gnn import _lib, cg, kernel_sets, ops
from helpers import batch, batch_to, copy_params, params
from test_live_outputs import LIVE, live_rows

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")


def rel_err(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


# ---------------------------------------------------------------------------
# kernel level
# ---------------------------------------------------------------------------
def _nan(*shape):
    return torch.full(shape, NAN, device=DEV, dtype=torch.float32)


def _run_set(cfg, info, mul, x, coef, g):
    """forward, grad-x and the coefficient gradient of one set through the C ABI, every
    output buffer NaN first: (out, grad_x, grad_coef[mul, nterms])"""
    lib = _lib.load()
    n = x.shape[0]
    s = _lib.stream(x)
    out = _nan(n, mul * info["Dout"])
    _lib.check(lib.eelg_sc_fwd_rows(cfg, _lib.ptr(x), x.shape[1], _lib.ptr(coef), n, mul,
                                    _lib.ptr(out), out.shape[1], s), "sc_fwd")
    gx = _nan(n, mul * info["D"])
    xt, gt = _nan(mul * info["D"], n), _nan(mul * info["Dout"], n)
    _lib.check(lib.eelg_sc_bwd_x_rows(cfg, _lib.ptr(x), x.shape[1], _lib.ptr(coef), _lib.ptr(g),
                                      g.shape[1], n, mul, _lib.ptr(gx), _lib.ptr(xt), _lib.ptr(gt), s),
               "sc_bwd_x")
    parts = int(lib.eelg_sc_bwd_coef_parts(cfg, n, mul))
    part = _nan(parts, mul, info["coef_ld"])
    _lib.check(lib.eelg_sc_bwd_coef(cfg, _lib.ptr(xt), _lib.ptr(gt), n, mul, info["coef_chunk"],
                                    _lib.ptr(part), s), "sc_bwd_coef")
    return out, gx, part[:, :, :info["nterms"]].sum(0)


@functools.lru_cache(maxsize=None)
def _pair(lmax, corr):
    """(full cfg, full info, live cfg, live info, live rows of the full plan, live columns)"""
    full_ls, ls = tuple(range(lmax + 1)), LIVE[lmax]
    fi, finfo, _ = _lib.sc_config(kernel_sets.sc_set_name(lmax, corr))
    li, linfo, lsig = _lib.sc_config(kernel_sets.sc_set_name(lmax, corr, ls))
    coupling = kernel_sets.coupling_str(lmax)
    assert lsig == cg.fnv1a64(cg.sc_signature(coupling, ls, corr))
    assert _lib.sc_outputs(li) == ls and _lib.sc_outputs(fi) == full_ls
    arr = (ctypes.c_int * len(ls))(*ls)
    assert _lib.load().eelg_sc_find_outputs(fi, ctypes.cast(arr, ctypes.c_void_p), len(ls)) == li
    _, rows, _ = live_rows(coupling, full_ls, ls, corr)
    assert linfo["nterms"] == len(rows) and linfo["Dout"] == sum(2 * l + 1 for l in ls)
    return fi, finfo, li, linfo, rows


def _live_columns(lmax, mul):
    """columns of the full set's mul-major output rows that belong to a live l"""
    cols, off = [], 0
    for l in range(lmax + 1):
        w = mul * (2 * l + 1)
        if l in LIVE[lmax]:
            cols += list(range(off, off + w))
        off += w
    return torch.tensor(cols, device=DEV)


SETS = [(lmax, corr, 32) for lmax in (1, 2, 3, 4) for corr in (1, 2, 3)] + [(2, 3, 16), (4, 2, 64)]


# n: 1 / 129 / 300 cover partial 128-node tiles of forward and grad-x; 1 / 300 / 2051 a ragged
# chunk and a second node range of the streaming coefficient gradient
@pytest.mark.parametrize("n", [1, 129, 300, 2051])
@pytest.mark.parametrize("lmax,corr,mul", SETS)
def test_live_set_matches_the_full_set(lmax, corr, mul, n):
    fi, finfo, li, linfo, rows = _pair(lmax, corr)
    gen = torch.Generator().manual_seed(1000 * lmax + 10 * corr + n)
    x = torch.randn(n, mul * finfo["D"], generator=gen).to(DEV)
    cf = torch.zeros(mul, finfo["coef_ld"])
    cf[:, :finfo["nterms"]] = torch.randn(mul, finfo["nterms"], generator=gen)
    cl = torch.zeros(mul, linfo["coef_ld"])
    cl[:, :len(rows)] = cf[:, rows]
    cf, cl = cf.to(DEV), cl.to(DEV)
    cols = _live_columns(lmax, mul)
    gl = torch.randn(n, mul * linfo["Dout"], generator=gen).to(DEV)
    gf = torch.zeros(n, mul * finfo["Dout"], device=DEV)
    gf[:, cols] = gl
    out_f, gx_f, gc_f = _run_set(fi, finfo, mul, x, cf, gf)
    out_l, gx_l, gc_l = _run_set(li, linfo, mul, x, cl, gl)
    errs = dict(fwd=rel_err(out_l, out_f[:, cols]), grad_x=rel_err(gx_l, gx_f),
                grad_coef=rel_err(gc_l, gc_f[:, rows]))
    print(f"sc l{lmax} c{corr} mul {mul} n {n}: {errs}")
    assert all(torch.isfinite(t).all() for t in (out_l, gx_l, gc_l))
    for k, v in errs.items():
        assert v < 1e-5, (k, v)


@pytest.mark.parametrize("lmax,corr", [(4, 3), (3, 3)])
def test_live_set_sums_over_the_full_sets_node_ranges(lmax, corr):
    """The streaming coefficient gradient leaves one partial per node range.  A live set has
    fewer term-group sets than its full set and would by itself choose more ranges (lmax 4 at
    32,768 nodes: 7 against 4); it takes the full set's, so a coefficient is the same sum of
    the same partials in both: bitwise equal, at a node count where the two would differ."""
    fi, finfo, li, linfo, rows = _pair(lmax, corr)
    lib, mul = _lib.load(), 32
    for n in (8300, 32768, 160000):
        assert lib.eelg_sc_bwd_coef_parts(li, n, mul) == lib.eelg_sc_bwd_coef_parts(fi, n, mul)
    n = 8300
    assert lib.eelg_sc_bwd_coef_parts(fi, n, mul) > 2
    gen = torch.Generator().manual_seed(7)
    x = torch.randn(n, mul * finfo["D"], generator=gen).to(DEV)
    cf = torch.zeros(mul, finfo["coef_ld"])
    cf[:, :finfo["nterms"]] = torch.randn(mul, finfo["nterms"], generator=gen)
    cl = torch.zeros(mul, linfo["coef_ld"])
    cl[:, :len(rows)] = cf[:, rows]
    cols = _live_columns(lmax, mul)
    gl = torch.randn(n, mul * linfo["Dout"], generator=gen).to(DEV)
    gf = torch.zeros(n, mul * finfo["Dout"], device=DEV)
    gf[:, cols] = gl
    out_f, gx_f, gc_f = _run_set(fi, finfo, mul, x, cf.to(DEV), gf)
    out_l, gx_l, gc_l = _run_set(li, linfo, mul, x, cl.to(DEV), gl)
    assert torch.equal(gc_l, gc_f[:, rows])
    assert torch.equal(out_l, out_f[:, cols]) and torch.equal(gx_l, gx_f)


@pytest.mark.parametrize("lmax,corr", [(4, 3), (2, 1)])
def test_wrong_row_width_is_an_error_not_a_launch(lmax, corr):
    fi, finfo, li, linfo, _ = _pair(lmax, corr)
    lib, mul, n = _lib.load(), 32, 5
    x = torch.randn(n, mul * linfo["D"], device=DEV)
    coef = torch.zeros(mul, linfo["coef_ld"], device=DEV)
    wide = _nan(n, mul * finfo["Dout"])          # the full set's row, not the live set's
    rc = lib.eelg_sc_fwd_rows(li, _lib.ptr(x), x.shape[1], _lib.ptr(coef), n, mul, _lib.ptr(wide),
                              wide.shape[1], _lib.stream(x))
    assert rc == -2 and b"sc_fwd" in lib.eelg_last_error()
    gx = _nan(n, mul * linfo["D"])
    rc = lib.eelg_sc_bwd_x_rows(li, _lib.ptr(x), x.shape[1], _lib.ptr(coef), _lib.ptr(wide),
                                wide.shape[1], n, mul, _lib.ptr(gx), None, None, _lib.stream(x))
    assert rc == -2
    rc = lib.eelg_sc_fwd_rows(fi, _lib.ptr(x), x.shape[1] - 4, _lib.ptr(coef), n, mul, _lib.ptr(wide),
                              wide.shape[1], _lib.stream(x))
    assert rc == -2
    torch.cuda.synchronize()
    assert torch.isnan(wide).all() and torch.isnan(gx).all()      # nothing ran
    with pytest.raises(ValueError):
        ops.symmetric_contraction(torch.randn(n, mul * finfo["D"] + 4, device=DEV), coef, li, linfo, mul)


@pytest.mark.parametrize("n", [3, 70])
def test_linear_residual_with_its_own_layout(n):
    """compact output over some irreps + the residual in full rows; the added gradient in
    compact rows on a full grad-x (the other slots add an exact zero).  The same module called
    plainly still computes every irrep."""
    from gnn.irreps import Irreps
    from gnn.o3 import GradMailbox, Linear
    hid = Irreps("32x0e+32x1o+32x2e")
    torch.manual_seed(3)
    ref, lin = Linear(hid, hid).to(DEV), Linear(hid, hid).to(DEV)
    up_ref, up = Linear(hid, hid).to(DEV), Linear(hid, hid).to(DEV)
    with torch.no_grad():
        lin.weight.copy_(ref.weight)
        up.weight.copy_(up_ref.weight)
    live = ((0, 0, 32), (2, 0, 32))
    lin.set_live(live, live)
    cols = torch.cat([torch.arange(0, 32), torch.arange(128, 288)]).to(DEV)
    h = torch.randn(n, hid.dim, device=DEV)
    gy = torch.randn(n, len(cols), device=DEV)

    def run(first, last, compact):
        hh = h.clone().requires_grad_(True)
        mb = GradMailbox()
        mid = first(hh, grad_mailbox=mb)
        y = last(mid[:, cols] if compact else mid, residual=hh, grad_mailbox=mb, live=compact)
        y = y if compact else y[:, cols]
        y.backward(gy)
        return y, hh.grad

    y0, g0 = run(up_ref, ref, False)
    y1, g1 = run(up, lin, True)
    assert rel_err(y1, y0) < 1e-5 and rel_err(g1, g0) < 1e-5
    assert rel_err(lin.weight.grad, ref.weight.grad) < 1e-5
    assert rel_err(up.weight.grad, up_ref.weight.grad) < 1e-5
    assert float(lin.weight.grad[1024:2048].abs().max()) == 0.0      # the 1o block: exact zeros
    assert rel_err(lin(h), ref(h)) < 1e-5 and lin(h).shape[1] == hid.dim


# ---------------------------------------------------------------------------
# model level
# ---------------------------------------------------------------------------
def _hidden(lmax, mul):
    return "+".join(f"{mul}x{l}{'e' if l % 2 == 0 else 'o'}" for l in range(lmax + 1))


def _models(p, monkeypatch):
    """(fp64 oracle, device model with the switch on, device model with it off), same weights"""
    from gnn.model import EnergyEquivGNN
    torch.manual_seed(0)
    o = omodel.EnergyEquivGNN(p).double()
    out = []
    for on in (True, False):
        monkeypatch.setattr(ops, "LIVE_OUT", on)
        torch.manual_seed(0)
        m = EnergyEquivGNN(p).to(DEV)
        copy_params(o, m)
        assert m.stiffness_head.live_pruned == on
        out.append(m)
    return o, out[0], out[1]


def _dead_masks(m, lmax):
    """name -> bool mask of the parameter entries that cannot reach the stiffness for the
    reference head: everything of an odd l in the last layer's contraction and product linear
    and in the readout, and the gate scalars of the odd-l gated irreps"""
    head = m.stiffness_head
    last = len(head.layers) - 1
    masks = {}
    pre = f"stiffness_head.layers.{last}.product."
    for n, q in m.named_parameters():
        if n.startswith(pre + "symmetric_contractions.contractions."):
            l = int(n[len(pre + "symmetric_contractions.contractions."):].split("x")[1][0])
            if l % 2:
                masks[n] = torch.ones_like(q, dtype=torch.bool)

    def by_instruction(lin, dead_cols=None):
        mask = torch.zeros(lin.weight_numel, dtype=torch.bool)
        for (i, o), w0 in zip(lin.instructions, lin._w_offs):
            mi, mo = lin.irreps_in[i].mul, lin.irreps_out[o].mul
            blk = torch.zeros(mi, mo, dtype=torch.bool)
            if lin.irreps_in[i].ir.l % 2:
                blk[:] = True
            if dead_cols is not None and o == 0:
                blk[:, dead_cols] = True
            mask[w0: w0 + mi * mo] = blk.reshape(-1)
        return mask.to(DEV)

    ro = head.nonlin_readout
    masks[pre + "linear.weight"] = by_instruction(head.layers[last].product.linear)
    # linear_1's 0e output slot: the scalars, then one run of gates per gated irrep l = 1 .. lmax
    ns = ro.equivariant_nonlin.irreps_scalars.dim
    dead_cols, c = [], ns
    for mul, ir in ro.equivariant_nonlin.irreps_gated:
        if ir.l % 2:
            dead_cols += list(range(c, c + mul))
        c += mul
    masks["stiffness_head.nonlin_readout.linear_1.weight"] = by_instruction(ro.linear_1, dead_cols)
    masks["stiffness_head.nonlin_readout.linear_2.weight"] = by_instruction(ro.linear_2)
    return {k: v for k, v in masks.items() if bool(v.any())}


CASES = [(layers, lmax, 32) for layers in (1, 2) for lmax in (1, 2, 4)] + [(1, 2, 16), (2, 2, 16)]


@pytest.mark.parametrize("layers,lmax,mul", CASES)
def test_model_switch_on_matches_switch_off_and_the_oracle(layers, lmax, mul, monkeypatch):
    from gnn.train import stiffness_loss
    b, rmax = batch(2, 50, 200, seed=1234)
    p = params(layers, lmax=lmax, max_edge_radius=rmax, hidden_irreps=_hidden(lmax, mul))
    o, m_on, m_off = _models(p, monkeypatch)
    assert set(m_on.state_dict()) == set(m_off.state_dict())
    bo = batch_to(b, "cpu", torch.float64)
    co = o(bo)["stiffness"]
    lo = oracle_loss(co, bo.stiffness)
    lo.backward()
    res = []
    for m in (m_on, m_off):
        bd = b.to(DEV)
        c = m(bd)["stiffness"]
        loss = stiffness_loss(c, bd.stiffness)
        loss.backward()
        res.append((c, loss))
    (c1, l1), (c0, l0) = res
    assert all(q.grad is not None for q in m_on.parameters())
    g_off = dict((n, q.grad) for n, q in m_off.named_parameters())
    po = dict(o.named_parameters())
    ab = max(rel_err(q.grad, g_off[n]) for n, q in m_on.named_parameters())
    worst = max(rel_err(q.grad, po[n].grad) for n, q in m_on.named_parameters())
    print(f"L{layers} lmax {lmax} mul {mul}: on/off stiffness {rel_err(c1, c0):.2e} loss "
          f"{abs(l1.item() - l0.item()) / abs(l0.item()):.2e} grads {ab:.2e}; oracle stiffness "
          f"{rel_err(c1, co):.2e} loss {abs(l1.item() - lo.item()) / abs(lo.item()):.2e} grads {worst:.2e}")
    assert rel_err(c1, c0) < 1e-5
    assert abs(l1.item() - l0.item()) <= 1e-5 * abs(l0.item())
    assert ab < 1e-5
    masks = _dead_masks(m_on, lmax)
    assert masks
    grads = dict((n, q.grad) for n, q in m_on.named_parameters())
    for n, mask in masks.items():
        assert float(grads[n][mask.reshape(grads[n].shape)].abs().max()) == 0.0, n
    assert rel_err(c1, co) < 1e-4
    assert abs(l1.item() - lo.item()) <= 1e-4 * abs(lo.item())
    assert worst < 1e-5


def test_model_bf16_storage_lmax3(monkeypatch):
    from gnn.model import EnergyEquivGNN
    from gnn.train import stiffness_loss
    b, rmax = batch(2, 50, 200, seed=1234)
    p = params(2, lmax=3, max_edge_radius=rmax)
    torch.manual_seed(0)
    o = omodel.EnergyEquivGNN(p).double()
    p.storage_dtype = "bfloat16"
    monkeypatch.setattr(ops, "LIVE_OUT", True)
    m = EnergyEquivGNN(p).to(DEV)
    copy_params(o, m)
    assert m.stiffness_head.live_pruned
    bo = batch_to(b, "cpu", torch.float64)
    co = o(bo)["stiffness"]
    lo = oracle_loss(co, bo.stiffness)
    lo.backward()
    bd = b.to(DEV)
    cm = m(bd)["stiffness"]
    lm = stiffness_loss(cm, bd.stiffness)
    lm.backward()
    po = dict(o.named_parameters())
    names = [n for n, _ in m.named_parameters()]
    gm = torch.cat([q.grad.double().cpu().reshape(-1) for _, q in m.named_parameters()])
    go = torch.cat([po[n].grad.reshape(-1) for n in names])
    print(f"bf16 lmax 3: stiffness {rel_err(cm, co):.2e} grads {rel_err(gm, go):.2e}")
    assert rel_err(cm, co) < 2e-2
    assert abs(lm.item() - lo.item()) <= 2e-2 * abs(lo.item())
    assert rel_err(gm, go) < 2e-2
    for n, mask in _dead_masks(m, 3).items():
        g = dict(m.named_parameters())[n].grad
        assert float(g[mask.reshape(g.shape)].abs().max()) == 0.0, n


def test_stiffness_sensitivity_with_live_outputs(monkeypatch):
    from gnn import stiffness_sensitivity
    b, rmax = batch(2, 50, 200, seed=1234)
    o, m_on, m_off = _models(params(2, lmax=2, correlation=2, max_edge_radius=rmax), monkeypatch)
    keys = ("positions", "edge_attr", "shifts")
    bo = batch_to(b, "cpu", torch.float64)
    for k in keys:
        setattr(bo, k, getattr(bo, k).detach().clone().requires_grad_(True))
    co = o(bo)["stiffness"]
    cot = torch.randn(co.shape, generator=torch.Generator().manual_seed(11), dtype=torch.float64)
    ref = torch.autograd.grad(co, [getattr(bo, k) for k in keys], grad_outputs=cot)
    on = stiffness_sensitivity(m_on, b.to(DEV), cot.float().to(DEV))
    off = stiffness_sensitivity(m_off, b.to(DEV), cot.float().to(DEV))
    assert rel_err(on["stiffness"], co) < 1e-4
    for k, r in zip(keys, ref):
        print(f"sensitivity {k}: oracle {rel_err(on[k], r):.2e} on/off {rel_err(on[k], off[k]):.2e}")
        assert rel_err(on[k], r) < 1e-5, k
        assert rel_err(on[k], off[k]) < 1e-5, k
    assert all(q.grad is None for q in m_on.parameters())


def test_overlap_stays_bitwise_equal_to_in_line(monkeypatch):
    """the side-stream step and the in-line step of the pruned model: the same bits"""
    from gnn.model import EnergyEquivGNN
    from gnn.train import stiffness_loss
    b, rmax = batch(2, 50, 200, seed=1234)
    p = params(2, lmax=4, max_edge_radius=rmax)
    monkeypatch.setattr(ops, "LIVE_OUT", True)
    got = []
    for overlap in (True, False):
        monkeypatch.setattr(ops, "OVERLAP", overlap)
        torch.manual_seed(0)
        m = EnergyEquivGNN(p).to(DEV)
        bd = b.to(DEV)
        c = m(bd)["stiffness"]
        stiffness_loss(c, bd.stiffness).backward()
        torch.cuda.synchronize()
        got.append((c, [q.grad for q in m.parameters()]))
    assert torch.equal(got[0][0], got[1][0])
    for a, r in zip(got[0][1], got[1][1]):
        assert torch.equal(a, r)
