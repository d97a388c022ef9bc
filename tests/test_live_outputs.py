"""Live outputs of the last layer (CPU part): which irreps of the last message-passing layer
can reach the stiffness linear, the live-output contraction plans, and the oracle's own zero
gradients.  The device tests are in ``test_gpu_live_outputs.py``."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import oracle.model as omodel
from oracle.train import stiffness_loss as oracle_loss

from gnn import cg, kernel_sets
from gnn.irreps import Irreps
from gnn.o3 import Linear
from helpers import batch, batch_to, params

LIVE = {1: (0,), 2: (0, 2), 3: (0, 2), 4: (0, 2, 4)}


def live_rows(coupling, full_ls, ls, corr):
    """rows of the full plan whose output component belongs to an l of ``ls`` and, per such
    row, its output component in the compact rows of ``ls``"""
    full = cg.symcon_plan(coupling, tuple(full_ls), corr)
    start, o = {}, 0
    for l in full_ls:
        start[l] = o
        o += 2 * l + 1
    comp, k = {}, 0
    for l in ls:
        for m in range(2 * l + 1):
            comp[start[l] + m] = k
            k += 1
    rows = [r for r, (_, _, out) in enumerate(full.terms) if out in comp]
    return full, rows, [comp[full.terms[r][2]] for r in rows]


@pytest.mark.parametrize("lmax", [1, 2, 3, 4])
def test_reference_head_live_irreps(lmax):
    from gnn.model import GNN_Head
    head = GNN_Head(params(2, lmax=lmax, correlation=2))
    assert tuple(ir.l for _, ir in head.live_irreps) == LIVE[lmax]
    assert kernel_sets.LIVE_OUT[lmax] == LIVE[lmax]
    assert head.live_pruned
    sc = head.layers[-1].product.symmetric_contractions
    assert sc._live == LIVE[lmax]
    # only the last layer has a live form, and only GNN_Head.forward asks for it
    assert all(layer.product.symmetric_contractions._live is None for layer in head.layers[:-1])
    assert all(layer.product.linear.live is None for layer in head.layers[:-1])
    assert head.layers[-1].product.linear.live is not None


def test_everything_live_selects_the_full_set():
    """a final linear that reads every irrep: all irreps live, the full set, nothing pruned"""
    from gnn.model import GNN_Head, readout_liveness
    p = params(2, lmax=2, correlation=2)
    head = GNN_Head(p)                       # the switch is on: the reference head is pruned
    assert head.live_pruned
    ro, prod = head.nonlin_readout, head.layers[-1].product
    full_sig = head.layers[0].product.symmetric_contractions._sig
    # the same head with a final linear that reads 1o as well, its live forms cleared
    head.linear = Linear(Irreps(p.readout_irreps), Irreps("2x0e+1x1o+2x2e"), biases=True)
    prod.symmetric_contractions.restrict_outputs(None)
    for lin in (prod.linear, ro.linear_1, ro.linear_2):
        lin.set_live(None, None)
    ro.equivariant_nonlin.set_live(None, None)
    live = readout_liveness(ro, head.linear)
    assert live["hidden"] == (0, 1, 2) and live["gate_gated"] == (0, 1)
    assert live["lin1_out"] == Linear.full_pieces(ro.linear_1.irreps_out)
    assert not head._prune(live)             # the path under test: everything is live
    sc = prod.symmetric_contractions
    assert sc._live is None and sc._sig == full_sig
    assert prod.linear.live is None and ro.linear_1.live is None and ro.linear_2.live is None
    assert ro.equivariant_nonlin.live is None and head.linear.live is None
    # and a head that reads only part of an otherwise generated list prunes to exactly that
    head.linear = Linear(Irreps(p.readout_irreps), Irreps("2x0e+2x2e"), biases=True)
    assert head._prune(readout_liveness(ro, head.linear)) and sc._live == (0, 2)


def test_switch_off_keeps_the_full_computation(monkeypatch):
    from gnn import ops
    from gnn.model import GNN_Head
    monkeypatch.setattr(ops, "LIVE_OUT", False)
    head = GNN_Head(params(2, lmax=2, correlation=2))
    assert not head.live_pruned
    assert tuple(ir.l for _, ir in head.live_irreps) == (0, 2)      # derived all the same
    assert head.layers[-1].product.symmetric_contractions._live is None
    assert head.nonlin_readout.linear_1.live is None
    assert head.nonlin_readout.equivariant_nonlin.live is None


def test_check_sc_accepts_exactly_the_generated_output_lists():
    hid = Irreps(kernel_sets.hidden_irreps_str(4))
    kernel_sets.check_sc(hid, (0, 1, 2, 3, 4), 3)
    kernel_sets.check_sc(hid, (0, 2, 4), 3)
    for ls in [(0, 2), (0, 4), (0, 1, 2), (2, 4)]:
        with pytest.raises(NotImplementedError, match=r"\(0, 2, 4\)"):
            kernel_sets.check_sc(hid, ls, 3)
    # correlation 4 is table-driven and keeps the full outputs
    hid3 = Irreps(kernel_sets.hidden_irreps_str(3))
    kernel_sets.check_sc(hid3, (0, 1, 2, 3), 4)
    with pytest.raises(NotImplementedError):
        kernel_sets.check_sc(hid3, (0, 2), 4)
    assert kernel_sets.sc_set_name(4, 3, (0, 2, 4)) == "sc_l4_c3_o024"
    assert kernel_sets.sc_set_name(4, 3) == "sc_l4_c3"


@pytest.mark.parametrize("lmax,corr", [(2, 3), (3, 3), (4, 3), (4, 1), (4, 2)])
def test_live_plan_is_the_full_plan_restricted(lmax, corr):
    coupling = kernel_sets.coupling_str(lmax)
    full_ls, ls = tuple(range(lmax + 1)), LIVE[lmax]
    full, rows, comps = live_rows(coupling, full_ls, ls, corr)
    live = cg.symcon_plan(coupling, ls, corr)
    # the same terms in the same relative order of (monomial, output)
    assert len(live.terms) == len(rows)
    for (nu, cls, o), r, c in zip(live.terms, rows, comps):
        fnu, fcls, _ = full.terms[r]
        assert (nu, cls, o) == (fnu, fcls, c)
    # ubig rows equal on the live weight columns; zero on the dead ones
    cols, k0 = [], 0
    for l, nu, k in full.weight_blocks:
        if l in ls:
            cols += list(range(k0, k0 + k))
        k0 += k
    dead = sorted(set(range(k0)) - set(cols))
    assert [(l, nu, k) for l, nu, k in full.weight_blocks if l in ls] == list(live.weight_blocks)
    assert np.array_equal(full.ubig[np.ix_(rows, cols)], live.ubig)
    assert not full.ubig[np.ix_(rows, dead)].any()
    if (lmax, corr) == (4, 3):
        assert (len(full.terms), len(live.terms)) == (7519, 4521)


def test_module_uses_those_rows_and_keeps_every_weight_block():
    from gnn.mace import SymmetricContraction
    hid = Irreps(kernel_sets.hidden_irreps_str(2))
    sc = SymmetricContraction(hid, hid, 3)
    names = [n for n, _ in sc.named_parameters()]
    k_total = sc.weight_matrix().shape[0]
    assert sc.restrict_outputs((0, 2))
    _, rows, _ = live_rows(kernel_sets.coupling_str(2), (0, 1, 2), (0, 2), 3)
    assert sc._live_rows.tolist() == rows
    assert [n for n, _ in sc.named_parameters()] == names
    assert sc.weight_matrix().shape[0] == k_total and sc.u_sym.shape[1] == k_total
    assert sc.coefficients().shape == (32, sc.u_sym.shape[0])     # a plain call: every term
    coef = sc.coefficients(live=True)             # CPU form: [mul, live terms]
    assert coef.shape == (32, len(rows))
    coef.square().sum().backward()
    for n, q in sc.named_parameters():
        assert q.grad is not None
        assert (float(q.grad.abs().max()) == 0.0) == ("32x1o" in n), n
    assert not sc.restrict_outputs((0, 1))        # not a generated list: no live form
    assert sc._live is None
    assert sc.restrict_outputs((0, 2)) and sc._live == (0, 2)
    assert sc.restrict_outputs(None) and sc._live is None


def test_pruned_linear_descriptors():
    """pieces -> descriptors: offsets into the compact rows, the weight block's own stride"""
    lin = Linear(Irreps("32x0e+32x1o+32x2e"), Irreps("48x0e+16x1o+16x2e"))
    full = (lin._fwd_desc.n_slots, lin._bw_desc.n_ins, lin._in_dim, lin._out_dim)
    assert full == (3, 3, 32 * 9, 48 + 16 * 8) and not lin._pruned and lin._fwd_desc.res_row == 0
    assert lin.live is None
    lin.set_live(((0, 0, 32), (2, 0, 32)), ((0, 0, 16), (0, 32, 16), (2, 0, 16)))
    live = lin.live
    assert live._pruned and (live._in_dim, live._out_dim) == (32 * 6, 32 + 80)
    d = live._fwd_desc
    assert d.n_slots == 3 and d.res_row == lin.irreps_out.dim
    assert [(d.slot[s].y_off, d.slot[s].n_out, d.slot[s].d, d.slot[s].r_off) for s in range(3)] == [
        (0, 16, 1, 0), (16, 16, 1, 32), (32, 16, 5, 48 + 48)]
    s1 = d.slot[1].src[0]
    assert (s1.x_off, s1.k, s1.w_off, s1.ldk, s1.ldj) == (0, 32, 32, 48, 1)
    s2 = d.slot[2].src[0]
    assert (s2.x_off, s2.k, s2.w_off, s2.ldk) == (32, 32, 32 * 48 + 32 * 16, 16)
    w = live._bw_desc
    assert w.n_ins == 3 and [w.ins[t].ldw for t in range(3)] == [48, 48, 0]
    assert not live._bw_covers
    # the module itself is as it was: a plain call computes everything
    assert (lin._fwd_desc.n_slots, lin._bw_desc.n_ins, lin._in_dim, lin._out_dim) == full
    assert lin._bw_covers and not lin._pruned
    assert [n for n, _ in lin.named_parameters()] == ["weight"]
    lin.set_live(None, None)
    assert lin.live is None
    lin.set_live(Linear.full_pieces(lin.irreps_in), Linear.full_pieces(lin.irreps_out))
    assert lin.live is None                      # everything live: no variant


@pytest.mark.parametrize("lmax", [2, 4])
def test_oracle_zero_gradients_are_exactly_the_dead_contraction_weights(lmax):
    b, rmax = batch(2, 24, 96, seed=7)
    torch.manual_seed(0)
    o = omodel.EnergyEquivGNN(params(2, lmax=lmax, max_edge_radius=rmax)).double()
    bo = batch_to(b, "cpu", torch.float64)
    oracle_loss(o(bo)["stiffness"], bo.stiffness).backward()
    zero = {n for n, q in o.named_parameters() if float(q.grad.abs().max()) == 0.0}
    last = "stiffness_head.layers.1.product.symmetric_contractions.contractions."
    want = {n for n, _ in o.named_parameters()
            if n.startswith(last) and int(n[len(last):].split("x")[1][0]) not in LIVE[lmax]}
    assert want and zero == want
