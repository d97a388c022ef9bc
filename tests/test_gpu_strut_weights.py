"""One radial weight row per strut (``ops.StrutMap``, EELG_STRUT_WEIGHTS) against the per-edge path.

* the TP kernels with the per-edge row index (``eelg_tp_fwd_rows`` / ``eelg_tp_bwd_rows``) against
  the same kernels on the expanded per-edge weights ``w_s[row]``: bitwise;
* the radial MLP on shared rows against the per-edge MLP: forward rows bitwise; every parameter
  gradient against an fp64 torch evaluation, the shared path's error at most 1.5 x the per-edge
  path's own error + 1e-7 of the gradient's scale (the project's criterion for a re-ordered
  fp32 sum, profiles/HISTORY.md round 4) -- and, since the backward runs per edge in edge order
  and only indexes the shared pre-activations, bitwise equal to the per-edge path's;
* the model with the switch on against off: stiffness, loss and every gradient bitwise (the
  radial gradients also by the criterion above against the fp64 oracle).
"""
import functools
from argparse import Namespace

import pytest
import torch

from helpers import batch_to, copy_params, params
from gnn import ops
from gnn.data import collate
from gnn.synthetic import SyntheticLattices

pytestmark = pytest.mark.gpu
DEV = "cuda"


# ---------------------------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------------------------
def _random_map(e: int, seed: int, alone: int = 1) -> ops.StrutMap:
    """a StrutMap that pairs random edges and leaves ``alone`` (+ one if the rest is odd) unpaired"""
    g = torch.Generator().manual_seed(seed)
    order = torch.randperm(e, generator=g)
    alone = min(e, alone + ((e - alone) % 2 if e > alone else 0))
    partner = torch.arange(e)
    rest = order[alone:]
    a, b = rest[0::2], rest[1::2]
    partner[a], partner[b] = b, a
    ar = torch.arange(e)
    is_rep = partner >= ar
    rep = torch.nonzero(is_rep).reshape(-1)
    row = (torch.cumsum(is_rep.long(), 0) - 1)[torch.minimum(partner, ar)]
    return ops.StrutMap(partner.to(DEV), row.to(torch.int32).to(DEV), rep.to(DEV), int(rep.shape[0]))


@functools.lru_cache(maxsize=None)
def _model(lmax: int, storage: str):
    from gnn.model import EnergyEquivGNN
    torch.manual_seed(0)
    return EnergyEquivGNN(params(2, lmax=lmax, storage_dtype=storage)).to(DEV)


def _degree_graph(n: int) -> torch.Tensor:
    """receiver i has in-degree (i + 1) % 6 (0..5, zero-degree receivers included); 5 for n = 1"""
    deg = torch.tensor([5]) if n == 1 else (torch.arange(n) + 1) % 6
    rcv = torch.repeat_interleave(torch.arange(n), deg)
    snd = torch.randint(0, n, (int(deg.sum()),), generator=torch.Generator().manual_seed(n))
    return torch.stack([snd, rcv])


# ---------------------------------------------------------------------------------------------
# 1. map: partners have bitwise-equal feature rows from eelg_edge_embed
# ---------------------------------------------------------------------------------------------
def test_partner_feature_rows_are_bitwise_equal():
    from gnn.model import EnergyEquivGNN
    ds = SyntheticLattices(2, 40, 160, seed=11)
    b = collate([ds[0], ds[1]]).to(DEV)
    csr = EnergyEquivGNN.edge_graph(b)
    m = csr.strut
    assert m is not None and m.n_rows == csr.num_edges // 2
    _, feats = ops.edge_embed(b.positions, csr, b.shifts[csr.perm], b.edge_attr[csr.perm].reshape(-1),
                              4, 6, 0.6, ds.max_edge_radius)
    partner = m.partner.to(DEV)
    assert torch.equal(feats[partner].view(torch.int32), feats.view(torch.int32))
    assert torch.equal(partner[partner], torch.arange(csr.num_edges, device=DEV))


def test_partner_feature_rows_of_the_periodic_graphs():
    """the two 5-node periodic graphs of test_strut_map (two images between one node pair, a strut
    to a node's own image): S = E / 2 and partners' eelg_edge_embed rows are bitwise equal"""
    from gnn.model import EnergyEquivGNN
    from test_strut_map import PERIODIC, _graph
    b = collate([_graph(PERIODIC, seed=1), _graph(PERIODIC, seed=2)]).to(DEV)
    csr = EnergyEquivGNN.edge_graph(b)
    m = csr.strut
    partner = m.partner.to(DEV)
    assert m.n_rows == csr.num_edges // 2 and bool((partner != torch.arange(csr.num_edges, device=DEV)).all())
    _, feats = ops.edge_embed(b.positions, csr, b.shifts[csr.perm], b.edge_attr[csr.perm].reshape(-1),
                              2, 6, 2.0, 0.05)
    assert torch.equal(feats[partner].view(torch.int32), feats.view(torch.int32))
    assert torch.equal(feats[m.rep][m.row.long()].view(torch.int32), feats.view(torch.int32))


# ---------------------------------------------------------------------------------------------
# 2. TP kernels with the row index == the same kernels on the expanded weights, bitwise
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", ["float32", "bfloat16"])
@pytest.mark.parametrize("lmax,layer", [(4, 1), (4, 0), (2, 1)])
@pytest.mark.parametrize("n", [1, 17, 130])
def test_tp_kernels_with_row_index_bitwise(n, lmax, layer, storage):
    blk = _model(lmax, storage).stiffness_head.layers[layer].interaction
    cfg, info = blk._config()
    dt = blk.storage_dtype
    ei = _degree_graph(n).to(DEV)
    csr = ops.EdgeCSR.build(ei, n)
    e = csr.num_edges
    assert n == 1 or e % 8 != 0          # tp_bwd: 8 half-waves of one edge per block, a ragged last one
    smap = _random_map(e, seed=e, alone=2)
    torch.manual_seed(e)
    x = torch.randn(n, info["din"], device=DEV)
    sh = torch.randn(e, info["nsh"], device=DEV)
    w_s = torch.randn(smap.n_rows, info["wn"], device=DEV).to(dt)
    go = torch.randn(n, info["dmid"], device=DEV)
    row = smap.row.long()

    x1 = x.clone().requires_grad_(True)
    w1 = w_s[row].clone().requires_grad_(True)               # the expanded per-edge weights
    agg1 = ops.tp_interaction(x1, sh, w1, csr, cfg, info, 0.25)
    agg1.backward(go)

    x2 = x.clone().requires_grad_(True)
    box = ops._GradBox()
    token = torch.zeros(1, device=DEV, requires_grad=True)
    agg2 = ops.tp_interaction(x2, sh, ops.StrutWeights(w_s, smap, token, box), csr, cfg, info, 0.25)
    agg2.backward(go)
    torch.cuda.synchronize()

    def bits(t):
        return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)
    assert torch.equal(bits(agg2), bits(agg1))
    assert torch.equal(bits(x2.grad), bits(x1.grad))
    gw = box.gw                                           # per edge, in edge order: no mapping back
    assert gw.shape == (e, info["wn"]) and gw.dtype == dt
    assert torch.equal(bits(gw), bits(w1.grad))

    # the plain C entry points, without autograd: per-edge grad_w and gxe rows compared directly
    lib = ops._lib.load()
    p = ops._lib.ptr
    bwd = lib.eelg_tp_bwd_rows_bf16 if dt == torch.bfloat16 else lib.eelg_tp_bwd_rows
    shp = ops.padded_sh(sh)
    outs = []
    for w_arg, idx in ((w1.detach().contiguous(), None), (w_s, smap.row)):
        gw_c = torch.empty(e, info["wn"], device=DEV, dtype=dt)
        gxe = torch.empty(e, info["din"], device=DEV, dtype=dt)
        ops._lib.check(bwd(cfg, p(x), p(shp), p(w_arg), p(idx), p(csr.sender), p(csr.receiver), None, e,
                           p(go), 0.25, p(gw_c), p(gxe), ops._lib.stream(x)), "tp_bwd")
        outs.append((gw_c, gxe))
    torch.cuda.synchronize()
    assert torch.equal(bits(outs[1][0]), bits(outs[0][0])) and torch.equal(bits(outs[1][1]), bits(outs[0][1]))
    assert torch.equal(bits(outs[1][0]), bits(gw))


# ---------------------------------------------------------------------------------------------
# 3. radial MLP on shared rows
# ---------------------------------------------------------------------------------------------
def _mlp(n_out, seed):
    torch.manual_seed(seed)
    last = torch.nn.Linear(64, n_out, bias=False)
    torch.nn.init.xavier_uniform_(last.weight, gain=10)
    return torch.nn.Sequential(torch.nn.Linear(12, 64), torch.nn.SiLU(), torch.nn.Linear(64, 64),
                               torch.nn.SiLU(), last)


def _criterion(shared, unshared, ref, name):
    """|shared - ref| <= 1.5 |unshared - ref| + 1e-7 max|ref| (max norms); prints the figures"""
    ref = ref.detach().double().cpu()
    es = float((shared.detach().double().cpu() - ref).abs().max())
    eu = float((unshared.detach().double().cpu() - ref).abs().max())
    scale = float(ref.abs().max())
    print(f"{name}: shared err {es:.3e}, per-edge err {eu:.3e}, scale {scale:.3e}")
    assert es <= 1.5 * eu + 1e-7 * scale, (name, es, eu, scale)


@pytest.mark.parametrize("s_rows,n_out", [(1, 160), (33, 1344), (129, 160), (300, 1344),
                                          (33, 36)])      # 36: no multiple of 8, zero-padded width
def test_radial_mlp_shared_rows(s_rows, n_out):
    # S pairs (E = 2S paired edges) and one unpaired edge with a row of its own
    e = 2 * s_rows + 1
    smap = _random_map(e, seed=s_rows, alone=1)
    n_rows = s_rows + 1
    assert smap.n_rows == n_rows and int((smap.partner == torch.arange(e, device=DEV)).sum()) == 1
    row = smap.row.long()
    torch.manual_seed(s_rows)
    feats_s = (torch.rand(n_rows, 12, dtype=torch.float64) * 0.9).float().double()   # fp32 values
    feats = feats_s.to(DEV)[row]                                     # partners: equal rows
    g = torch.randn(e, n_out, dtype=torch.float64).float().double()
    ref = _mlp(n_out, seed=s_rows).double()
    (ref(feats.double().cpu()) * g).sum().backward()
    gd = g.float().to(DEV)

    per_edge = _mlp(n_out, seed=s_rows).to(DEV)
    y = ops.radial_mlp(feats.float(), per_edge)
    y.backward(gd)

    shared = _mlp(n_out, seed=s_rows).to(DEV)
    sw = ops.radial_mlp_shared(feats.float(), shared, smap)
    assert sw.w.shape == (n_rows, n_out) and not sw.w.requires_grad
    assert torch.equal(sw.w[row].view(torch.int32), y.detach().view(torch.int32))
    sw.box.gw = gd.clone()                                           # per edge, as tp_bwd leaves it
    sw.token.backward(torch.zeros(1, device=DEV))
    torch.cuda.synchronize()
    assert sw.box.gw is None
    pr = dict(ref.named_parameters())
    pu = dict(per_edge.named_parameters())
    for name, p in shared.named_parameters():
        _criterion(p.grad, pu[name].grad, pr[name].grad, f"S={s_rows} {name}")
        # the backward keeps every sum in edge order, so the two paths agree to the bit
        assert torch.equal(p.grad.view(torch.int32), pu[name].grad.view(torch.int32)), name


# ---------------------------------------------------------------------------------------------
# 4. model level: switch on against off
# ---------------------------------------------------------------------------------------------
def _small_params(max_edge_radius) -> Namespace:
    return params(2, lmax=2, max_edge_radius=max_edge_radius)


def _run_model(m, b, on: bool, monkeypatch, geometry: bool = False):
    """(stiffness, loss, grads, position grad, shared-MLP calls) of one forward / backward"""
    from gnn.train import stiffness_loss
    monkeypatch.setattr(ops, "STRUT_WEIGHTS", on)
    calls = []
    real = ops.radial_mlp_shared
    monkeypatch.setattr(ops, "radial_mlp_shared", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    for p in m.parameters():
        p.grad = None
    bd = b.to(DEV)
    if geometry:
        bd.positions.requires_grad_(True)
    m.edge_graph(bd)                  # ahead of the step, as bench.py does: the strut map is made here
    c = m(bd)["stiffness"]
    loss = stiffness_loss(c, bd.stiffness)
    loss.backward()
    torch.cuda.synchronize()
    grads = {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}
    return c.detach(), loss.detach(), grads, bd.positions.grad, len(calls)


@pytest.fixture(scope="module")
def small():
    """the 2-layer lmax-2 model on 2 graphs x 12 nodes, with the fp64 oracle's gradients"""
    import oracle.model as omodel
    from oracle.train import stiffness_loss as oracle_loss
    from gnn.model import EnergyEquivGNN
    ds = SyntheticLattices(2, 12, 48, seed=7)
    b = collate([ds[0], ds[1]])
    p = _small_params(ds.max_edge_radius)
    torch.manual_seed(0)
    o = omodel.EnergyEquivGNN(p).double()
    m = EnergyEquivGNN(p).to(DEV)
    copy_params(o, m)
    bo = batch_to(b, "cpu", torch.float64)
    oracle_loss(o(bo)["stiffness"], bo.stiffness).backward()
    og = {k: v.grad.detach() for k, v in o.named_parameters() if v.grad is not None}
    return m, b, og


def test_model_switch_on_equals_off(small, monkeypatch):
    m, b, og = small
    c0, l0, g0, _, n0 = _run_model(m, b, False, monkeypatch)
    c1, l1, g1, _, n1 = _run_model(m, b, True, monkeypatch)
    assert n0 == 0 and n1 == 2                    # both layers took the shared rows
    assert torch.equal(c1.view(torch.int32), c0.view(torch.int32))
    assert torch.equal(l1.view(torch.int32), l0.view(torch.int32))
    assert set(g1) == set(g0)
    for k in g0:
        if "conv_tp_weights" in k:
            _criterion(g1[k], g0[k], og[k], k)
        assert torch.equal(g1[k].view(torch.int32), g0[k].view(torch.int32)), k


def test_model_geometry_gradients_keep_per_edge_weights(small, monkeypatch):
    m, b, _ = small
    c0, l0, g0, gp0, _ = _run_model(m, b, False, monkeypatch, geometry=True)
    c1, l1, g1, gp1, n1 = _run_model(m, b, True, monkeypatch, geometry=True)
    assert n1 == 0
    assert torch.equal(c1, c0) and torch.equal(l1, l0) and torch.equal(gp1, gp0)
    for k in g0:
        assert torch.equal(g1[k], g0[k]), k


def test_model_unpaired_batch_equals_off(small, monkeypatch):
    m, b, _ = small
    half = []
    ds = SyntheticLattices(2, 12, 48, seed=7)
    for g in range(2):
        d = ds[g]
        k = d.edge_index.shape[1] // 2            # the generator lists all struts one way, then back
        half.append(type(d)(positions=d.positions, node_attrs=d.node_attrs, edge_index=d.edge_index[:, :k],
                            shifts=d.shifts[:k], edge_attr=d.edge_attr[:k], stiffness=d.stiffness))
    b1 = collate(half)
    c0, l0, g0, _, _ = _run_model(m, b1, False, monkeypatch)
    c1, l1, g1, _, n1 = _run_model(m, b1, True, monkeypatch)
    assert n1 == 0                                # S = E: the per-edge path
    assert torch.equal(c1, c0) and torch.equal(l1, l0)
    for k in g0:
        assert torch.equal(g1[k], g0[k]), k
