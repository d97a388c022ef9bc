"""Geometry gradients of the HIP path (d stiffness / d positions, strut radii, shifts) vs
autograd of the fp64 CPU oracle, which tests/test_geometry_oracle.py checks against finite
differences.

Tolerance: the project's standing rule (tests/test_gpu_parity.py): every gradient within 1e-5
of its own largest entry, stiffness within 1e-4.  The oracle's own fp32 run differs from its
fp64 run by 4e-7 .. 1.4e-6 on these shapes, so the rule leaves about 7x over fp32 rounding.
Achieved errors are recorded with ``helpers.record_parity``."""
import pytest
import torch

from helpers import batch, batch_to, copy_params, params, record_parity

import oracle.mace as omace
import oracle.model as omodel
import oracle.o3 as oo3
from oracle.train import stiffness_loss as oracle_loss

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-5


def rel_err(a, b):
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def _hidden(lmax, mul):
    return "+".join(f"{mul}x{l}{'e' if l % 2 == 0 else 'o'}" for l in range(lmax + 1))


# ---------------------------------------------------------------------------
# 1. edge_embed backward
# ---------------------------------------------------------------------------
def _random_edges(n_nodes, n_edges, gen, isolated):
    """directed edges without self loops among the nodes other than ``isolated``"""
    nodes = torch.tensor([i for i in range(n_nodes) if i != isolated])
    s = nodes[torch.randint(len(nodes), (n_edges,), generator=gen)]
    r = nodes[torch.randint(len(nodes), (n_edges,), generator=gen)]
    r = torch.where(r == s, nodes[(torch.searchsorted(nodes, r) + 1) % len(nodes)], r)
    return torch.stack([s, r])


def _oracle_embed(pos, ei, shifts, rad, lmax, nb, rmax):
    vec, ln = omace.get_edge_vectors_and_lengths(pos, ei, shifts)
    sh = oo3.spherical_harmonics(lmax, vec)
    feats = torch.cat([oo3.soft_one_hot_linspace(ln.squeeze(-1), 0, 0.6, nb),
                       oo3.soft_one_hot_linspace(rad.squeeze(-1), 0, rmax, nb)], 1)
    return sh, feats


@pytest.mark.parametrize("nb", [2, 6, 8])
@pytest.mark.parametrize("lmax", [1, 2, 3, 4])
def test_edge_embed_backward_matches_oracle(lmax, nb):
    """E = 300 (two 256-thread blocks, the second with a tail) on 40 nodes, node 39 without
    edges (its gradient is exactly 0), and E = 1."""
    from gnn import ops
    rmax = 0.05
    gen = torch.Generator().manual_seed(100 * lmax + nb)
    for n_nodes, n_edges, isolated in ((40, 300, 39), (3, 1, 2)):
        ei = _random_edges(n_nodes, n_edges, gen, isolated)
        pos = (0.5 * torch.rand(n_nodes, 3, generator=gen, dtype=torch.float64)).requires_grad_(True)
        shifts = (0.1 * (torch.rand(n_edges, 3, generator=gen, dtype=torch.float64) - 0.5)).requires_grad_(True)
        rad = (rmax * (0.1 + 0.9 * torch.rand(n_edges, 1, generator=gen, dtype=torch.float64))).requires_grad_(True)
        sh, feats = _oracle_embed(pos, ei, shifts, rad, lmax, nb, rmax)
        gs = torch.randn(sh.shape, generator=gen, dtype=torch.float64)
        gf = torch.randn(feats.shape, generator=gen, dtype=torch.float64)
        ref = torch.autograd.grad((sh * gs).sum() + (feats * gf).sum(), [pos, shifts, rad])

        csr = ops.EdgeCSR.build(ei.to(DEV), n_nodes)
        pd = pos.detach().float().to(DEV).requires_grad_(True)
        sd = shifts.detach().float().to(DEV).requires_grad_(True)
        rd = rad.detach().float().to(DEV).requires_grad_(True)
        sh_d, f_d = ops.edge_embed(pd, csr, ops.permute_rows(sd, csr.perm),
                                   ops.permute_rows(rd, csr.perm).reshape(-1), lmax, nb, 0.6, rmax)
        perm = csr.perm.cpu()
        assert rel_err(sh_d, sh[perm]) < TOL and rel_err(f_d, feats[perm]) < TOL
        got = torch.autograd.grad((sh_d * gs[perm].float().to(DEV)).sum()
                                  + (f_d * gf[perm].float().to(DEV)).sum(), [pd, sd, rd])
        errs = {k: rel_err(g, r) for k, g, r in zip(("positions", "shifts", "radii"), got, ref)}
        print(f"edge_embed_bwd lmax {lmax} nb {nb} E {n_edges}: {errs}")
        record_parity(f"edge_embed_bwd_l{lmax}_nb{nb}_E{n_edges}", **errs)
        for k, v in errs.items():
            assert v < TOL, (k, n_edges)
        assert torch.equal(got[0][isolated], torch.zeros(3, device=DEV))
        assert got[1].shape == sd.shape and got[2].shape == rd.shape


# ---------------------------------------------------------------------------
# 2. input gradient of the radial MLP
# ---------------------------------------------------------------------------
def _mlp(n_feat, hidden, n_hidden, n_out):
    mods = [torch.nn.Linear(n_feat, hidden), torch.nn.SiLU()]
    for _ in range(n_hidden - 1):
        mods += [torch.nn.Linear(hidden, hidden), torch.nn.SiLU()]
    mods.append(torch.nn.Linear(hidden, n_out, bias=False))
    return torch.nn.Sequential(*mods)


@pytest.mark.parametrize("n_feat", [12, 32])
@pytest.mark.parametrize("n_hidden", [1, 2, 3])
@pytest.mark.parametrize("hidden", [32, 64])
def test_radial_input_gradient_matches_sequential_autograd(hidden, n_hidden, n_feat):
    """E = 1, 129 (a 128-edge tile and one edge) and 300 (not a multiple of the 8-edge groups);
    with the weights frozen (only ``eelg_radial_bwd_gh`` + ``eelg_radial_bwd_x`` run) the
    feature gradient is bitwise the same."""
    import copy
    from gnn import ops
    torch.manual_seed(7 * hidden + 3 * n_hidden + n_feat)
    ref_mlp = _mlp(n_feat, hidden, n_hidden, 40).double()
    dev_mlp = copy.deepcopy(ref_mlp).float().to(DEV)
    for e in (1, 129, 300):
        x = torch.rand(e, n_feat, dtype=torch.float64).requires_grad_(True)
        y = ref_mlp(x)
        g = torch.randn_like(y)
        (ref,) = torch.autograd.grad((y * g).sum(), [x], retain_graph=True)
        xd = x.detach().float().to(DEV).requires_grad_(True)
        yd = ops.radial_mlp(xd, dev_mlp)
        assert rel_err(yd, y) < TOL
        (got,) = torch.autograd.grad((yd * g.float().to(DEV)).sum(), [xd], retain_graph=True)
        # the weight gradients still come out when the features require grad too
        (yd * g.float().to(DEV)).sum().backward()
        (y * g).sum().backward()
        werr = max(rel_err(pd.grad, pr.grad) for pd, pr in zip(dev_mlp.parameters(), ref_mlp.parameters()))
        for p in list(dev_mlp.parameters()) + list(ref_mlp.parameters()):
            p.grad = None
        err = rel_err(got, ref)
        print(f"radial_bwd_x hidden {hidden} layers {n_hidden} n_feat {n_feat} E {e}: {err:.2e} (weights {werr:.2e})")
        record_parity(f"radial_bwd_x_h{hidden}_n{n_hidden}_f{n_feat}_E{e}", grad_feats=err, grad_params=werr)
        assert err < TOL and werr < TOL
        for p in dev_mlp.parameters():
            p.requires_grad_(False)
        xf = x.detach().float().to(DEV).requires_grad_(True)
        (gotf,) = torch.autograd.grad((ops.radial_mlp(xf, dev_mlp) * g.float().to(DEV)).sum(), [xf])
        for p in dev_mlp.parameters():
            p.requires_grad_(True)
        assert torch.equal(gotf, got)


def test_radial_fallback_shape_differentiates_through_radial_weights():
    """inter_MLP_dim 48 runs the torch Sequential on the device: autograd gives the gradient"""
    import copy
    from gnn.model import EnergyEquivGNN
    torch.manual_seed(0)
    m = EnergyEquivGNN(params(2, lmax=1, correlation=1, inter_MLP_dim=48)).to(DEV)
    blk = m.stiffness_head.layers[0].interaction
    assert not blk._radial_hip
    ref_mlp = copy.deepcopy(blk.conv_tp_weights).double().cpu()
    x = torch.rand(129, 12, dtype=torch.float64).requires_grad_(True)
    y = ref_mlp(x)
    g = torch.randn_like(y)
    (ref,) = torch.autograd.grad((y * g).sum(), [x])
    xd = x.detach().float().to(DEV).requires_grad_(True)
    (got,) = torch.autograd.grad((blk.radial_weights(xd) * g.float().to(DEV)).sum(), [xd])
    assert rel_err(got, ref) < TOL


# ---------------------------------------------------------------------------
# 3. interaction block: grad_sh and grad_feats
# ---------------------------------------------------------------------------
def _hand_graph():
    """13 nodes, 37 directed edges: node 11 has no in-edges, node 12 no out-edges; the odd edge
    count leaves a half-wave without an edge at the end of the SH-gradient kernel's range"""
    gen = torch.Generator().manual_seed(5)
    send, recv = [], []
    for e in range(37):
        s = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11][e % 12]            # never 12
        r = [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 0, 12, 5][(5 * e + 3) % 13]  # never 11
        if r == s:
            r = (r + 1) % 11
        send.append(s)
        recv.append(r)
    ei = torch.tensor([send, recv])
    assert 11 not in recv and 12 not in send and ei.shape == (2, 37)
    pos = 0.5 * torch.rand(13, 3, generator=gen, dtype=torch.float64)
    shifts = 0.1 * (torch.rand(37, 3, generator=gen, dtype=torch.float64) - 0.5)
    rad = 0.05 * (0.1 + 0.9 * torch.rand(37, 1, generator=gen, dtype=torch.float64))
    return ei, pos, shifts, rad


_BLOCK_CASES = [  # (lmax, mul, layer, reduction)
    (4, 32, 0, "sum"), (4, 32, 1, "sum"), (1, 32, 1, "sum"), (2, 32, 1, "sum"), (3, 32, 1, "sum"),
    (2, 16, 0, "sum"), (2, 16, 1, "sum"), (2, 64, 0, "sum"), (2, 64, 1, "sum"),
    (2, 32, 1, "mean"), (2, 32, 1, "max"), (4, 32, 1, "mean"), (4, 32, 1, "max"),
]


@pytest.mark.parametrize("lmax,mul,layer,reduction", _BLOCK_CASES)
def test_interaction_block_sh_and_feature_gradients(lmax, mul, layer, reduction):
    """Same pairing as test_gpu_parity.test_interaction_block_fwd_bwd, with the SH and the edge
    features requiring grad; also the pad columns of the C-ABI call's grad_sh rows."""
    from gnn import _lib, ops
    from gnn.model import EnergyEquivGNN
    ei, pos, shifts, rad = _hand_graph()
    rmax = 0.05
    p = params(2, lmax=lmax, correlation=1, hidden_irreps=_hidden(lmax, mul), max_edge_radius=rmax,
               interaction_reduction=reduction)
    torch.manual_seed(0)
    o = omodel.EnergyEquivGNN(p).double()
    m = EnergyEquivGNN(p).to(DEV)
    copy_params(o, m)
    o_int = o.stiffness_head.layers[layer].interaction
    m_int = m.stiffness_head.layers[layer].interaction
    sh, ef = _oracle_embed(pos, ei, shifts, rad, lmax, 6, rmax)
    torch.manual_seed(1)
    x = torch.randn(13, o_int._node_feats_irreps.dim, dtype=torch.float64)
    xo, sho, efo = (t.detach().clone().requires_grad_(True) for t in (x, sh, ef))
    yo, _ = o_int(xo, sho, efo, ei)
    go = torch.randn_like(yo)
    (yo * go).sum().backward()
    xm, shm, efm = (t.detach().float().to(DEV).requires_grad_(True) for t in (x, sh, ef))
    ym, _ = m_int(xm, shm, efm, ei.to(DEV))
    (ym * go.float().to(DEV)).sum().backward()
    po = dict(o_int.named_parameters())
    errs = dict(out=rel_err(ym, yo), grad_x=rel_err(xm.grad, xo.grad), grad_sh=rel_err(shm.grad, sho.grad),
                grad_feats=rel_err(efm.grad, efo.grad),
                grad_params=max(rel_err(pm.grad, po[n].grad) for n, pm in m_int.named_parameters()))
    print(f"interaction block lmax {lmax} mul {mul} layer {layer} {reduction}: {errs}")
    record_parity(f"geom_block_l{lmax}_m{mul}_layer{layer}_{reduction}", **errs)
    for k, v in errs.items():
        assert v < TOL, k

    # the C ABI: rows are written whole, pad columns 0 (the buffer starts as NaN)
    idx, info = m_int._config()
    csr = ops.EdgeCSR.build(ei.to(DEV), 13)
    nsh, nshp = info["nsh"], ops.sh_row_stride(info["nsh"])
    w = torch.randn(37, info["wn"], device=DEV)
    gagg = torch.randn(13, info["dmid"], device=DEV)
    out = torch.full((37, nshp), float("nan"), device=DEV)
    xs = x.float().to(DEV).contiguous()
    _lib.check(_lib.load().eelg_tp_bwd_sh(idx, _lib.ptr(xs), None, _lib.ptr(w), _lib.ptr(csr.sender),
                                          _lib.ptr(csr.receiver), 37, _lib.ptr(gagg), 0.25, _lib.ptr(out),
                                          _lib.stream(out)), "tp_bwd_sh")
    assert torch.isfinite(out).all()
    assert torch.equal(out[:, nsh:], torch.zeros(37, nshp - nsh, device=DEV))
    # and no launch, no error for an empty edge set
    assert _lib.load().eelg_tp_bwd_sh(idx, None, None, None, None, None, 0, None, 0.25, None,
                                      _lib.stream(out)) == 0
    assert _lib.load().eelg_tp_bwd_sh(10 ** 6, None, None, None, None, None, 0, None, 0.25, None,
                                      _lib.stream(out)) < 0


# ---------------------------------------------------------------------------
# 4. model level
# ---------------------------------------------------------------------------
_GEOM = ("positions", "edge_attr", "shifts")


def _model_pair(p):
    from gnn.model import EnergyEquivGNN
    torch.manual_seed(0)
    o = omodel.EnergyEquivGNN(p).double()
    m = EnergyEquivGNN(p).to(DEV)
    copy_params(o, m)
    return o, m


def _with_geometry_grad(b):
    for k in _GEOM:
        setattr(b, k, getattr(b, k).detach().clone().requires_grad_(True))
    return b


@pytest.mark.parametrize("message_passes,lmax,correlation,mul",
                         [(2, 4, 3, 32), (2, 3, 3, 32), (2, 1, 1, 32), (2, 2, 2, 16), (2, 2, 2, 64)])
def test_model_geometry_and_parameter_gradients_match_oracle(message_passes, lmax, correlation, mul):
    from gnn.model import EnergyEquivGNN
    from gnn.train import stiffness_loss
    b, rmax = batch(2, 24, 96, seed=7)
    p = params(message_passes, lmax=lmax, correlation=correlation, max_edge_radius=rmax,
               hidden_irreps=_hidden(lmax, mul))
    o, m = _model_pair(p)
    bo = _with_geometry_grad(batch_to(b, "cpu", torch.float64))
    co = o(bo)["stiffness"]
    oracle_loss(co, bo.stiffness).backward()
    bd = _with_geometry_grad(b.to(DEV))
    cm = m(bd)["stiffness"]
    stiffness_loss(cm, bd.stiffness).backward()
    po = dict(o.named_parameters())
    errs = {k: rel_err(getattr(bd, k).grad, getattr(bo, k).grad) for k in _GEOM}
    errs["grad_params"] = max(rel_err(pm.grad, po[n].grad) for n, pm in m.named_parameters())
    gp = bd.positions.grad
    per_graph = torch.zeros(bd.num_graphs, 3, device=DEV).index_add_(0, bd.batch, gp)
    errs["translation"] = float(per_graph.abs().max() / gp.abs().max())
    print(f"model mp {message_passes} lmax {lmax} corr {correlation} mul {mul}: stiffness {rel_err(cm, co):.2e} {errs}")
    record_parity(f"geom_model_mp{message_passes}_l{lmax}_c{correlation}_m{mul}", stiffness=rel_err(cm, co), **errs)
    assert rel_err(cm, co) < 1e-4
    for k, v in errs.items():
        assert v < TOL, k
    for k in _GEOM:
        assert getattr(bd, k).grad.shape == getattr(bd, k).shape
    # the parameter gradients are those of the training step (geometry without grad), bitwise;
    # a second model with the same weights: a gradient accumulator belongs to its first backward
    torch.manual_seed(0)
    m2 = EnergyEquivGNN(p).to(DEV)
    copy_params(o, m2)
    b2 = b.to(DEV)
    c2 = m2(b2)["stiffness"]
    stiffness_loss(c2, b2.stiffness).backward()
    assert torch.equal(c2, cm)
    for (n, q), q2 in zip(m.named_parameters(), m2.parameters()):
        assert torch.equal(q.grad, q2.grad), n


# ---------------------------------------------------------------------------
# 5. the public helper
# ---------------------------------------------------------------------------
def test_stiffness_sensitivity_matches_oracle_and_is_deterministic():
    from gnn import stiffness_sensitivity
    b, rmax = batch(2, 24, 96, seed=7)
    o, m = _model_pair(params(2, lmax=2, correlation=2, max_edge_radius=rmax))
    bo = _with_geometry_grad(batch_to(b, "cpu", torch.float64))
    co = o(bo)["stiffness"]
    cot = torch.randn(co.shape, generator=torch.Generator().manual_seed(11), dtype=torch.float64)
    ref = torch.autograd.grad(co, [getattr(bo, k) for k in _GEOM], grad_outputs=cot, retain_graph=True)
    bd = b.to(DEV)
    before = {k: getattr(bd, k) for k in _GEOM}
    out = stiffness_sensitivity(m, bd, cot.float().to(DEV))
    assert set(out) == {"stiffness", "positions", "edge_attr", "shifts"}
    assert rel_err(out["stiffness"], co) < 1e-4
    errs = {k: rel_err(out[k], r) for k, r in zip(_GEOM, ref)}
    print(f"stiffness_sensitivity: {errs}")
    record_parity("stiffness_sensitivity", **errs)
    for k, v in errs.items():
        assert v < TOL, k
        assert out[k].shape == getattr(bd, k).shape
    assert all(q.grad is None for q in m.parameters())
    for k in _GEOM:                                  # the batch is as it was
        assert getattr(bd, k) is before[k] and not before[k].requires_grad
    again = stiffness_sensitivity(m, bd, cot.float().to(DEV))
    for k in out:
        assert torch.equal(out[k], again[k]), k
    # default cotangent: all ones; frozen parameters change nothing
    ones = stiffness_sensitivity(m, bd)
    for q in m.parameters():
        q.requires_grad_(False)
    frozen = stiffness_sensitivity(m, bd)
    ref1 = torch.autograd.grad(co.sum(), [getattr(bo, k) for k in _GEOM])
    for k, r in zip(_GEOM, ref1):
        assert rel_err(ones[k], r) < TOL, k
        assert torch.equal(ones[k], frozen[k]), k


# ---------------------------------------------------------------------------
# 6. the training path is what it was
# ---------------------------------------------------------------------------
def test_training_path_launches_no_geometry_kernel_and_overlap_stays_bitwise():
    from gnn import ops
    from gnn.model import EnergyEquivGNN
    from gnn.train import stiffness_loss
    b, rmax = batch(2, 24, 96, seed=7)
    bd = b.to(DEV)
    p = params(2, lmax=2, correlation=2, max_edge_radius=rmax)
    saved, outs = ops.OVERLAP, []
    timer = ops.TIMER
    try:
        for flag in (False, True):
            ops.OVERLAP = flag
            torch.manual_seed(0)
            m = EnergyEquivGNN(p).to(DEV)
            timer.records.clear()
            timer.enabled = True
            c = m(bd)["stiffness"]
            stiffness_loss(c, bd.stiffness).backward()
            torch.cuda.synchronize()
            timer.enabled = False
            names = list(timer.records)
            assert any(n.startswith("tp_bwd[") for n in names), names
            for n in names:
                assert not any(k in n for k in ("tp_bwd_sh", "radial_bwd_x", "edge_embed_bwd")), n
            outs.append((c.detach().clone(), [q.grad.clone() for q in m.parameters()]))
        # and with geometry requiring grad the three launches are there, by these names (a fresh
        # model: a parameter's gradient accumulator belongs to the stream of its first backward)
        torch.manual_seed(0)
        m = EnergyEquivGNN(p).to(DEV)
        timer.records.clear()
        timer.enabled = True
        bg = _with_geometry_grad(b.to(DEV))
        stiffness_loss(m(bg)["stiffness"], bg.stiffness).backward()
        torch.cuda.synchronize()
        timer.enabled = False
        names = list(timer.records)
        for k in ("tp_bwd_sh", "radial_bwd_x", "edge_embed_bwd"):
            assert any(k in n for n in names), (k, names)
    finally:
        ops.OVERLAP = saved
        timer.enabled = False
        timer.records.clear()
    assert torch.equal(outs[0][0], outs[1][0])
    for g0, g1 in zip(outs[0][1], outs[1][1]):
        assert torch.equal(g0, g1)


def test_radii_only_gradient_launches_no_sh_gradient():
    """Only ``edge_attr`` requires grad: the SH carry no grad, so no ``tp_bwd_sh`` runs; the
    radius gradient is the one of the full geometry backward, within the same bound."""
    from gnn import ops
    from gnn.train import stiffness_loss
    b, rmax = batch(2, 24, 96, seed=7)
    o, m = _model_pair(params(2, lmax=2, correlation=2, max_edge_radius=rmax))
    bo = batch_to(b, "cpu", torch.float64)
    bo.edge_attr = bo.edge_attr.detach().clone().requires_grad_(True)
    oracle_loss(o(bo)["stiffness"], bo.stiffness).backward()
    bd = b.to(DEV)
    bd.edge_attr = bd.edge_attr.detach().clone().requires_grad_(True)
    timer = ops.TIMER
    try:
        timer.records.clear()
        timer.enabled = True
        stiffness_loss(m(bd)["stiffness"], bd.stiffness).backward()
        torch.cuda.synchronize()
        names = list(timer.records)
    finally:
        timer.enabled = False
        timer.records.clear()
    assert not any("tp_bwd_sh" in n for n in names), names
    for k in ("radial_bwd_x", "edge_embed_bwd"):
        assert any(k in n for n in names), (k, names)
    assert bd.positions.grad is None and bd.shifts.grad is None
    err = rel_err(bd.edge_attr.grad, bo.edge_attr.grad)
    record_parity("geom_radii_only", edge_attr=err)
    assert err < TOL


# ---------------------------------------------------------------------------
# 7. bf16 storage has no geometry gradients
# ---------------------------------------------------------------------------
def test_bf16_storage_with_geometry_grad_raises():
    from gnn.model import EnergyEquivGNN
    b, rmax = batch(2, 24, 96, seed=7)
    torch.manual_seed(0)
    m = EnergyEquivGNN(params(2, lmax=2, correlation=2, max_edge_radius=rmax,
                              storage_dtype="bfloat16")).to(DEV)
    bd = b.to(DEV)
    bd.positions = bd.positions.detach().clone().requires_grad_(True)
    with pytest.raises(NotImplementedError, match="storage"):
        m(bd)
    # without grad the bf16 model runs as before
    bd.positions = bd.positions.detach()
    assert torch.isfinite(m(bd)["stiffness"]).all()
