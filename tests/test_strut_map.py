"""The strut map (``ops.build_strut_map``, ``EnergyEquivGNN.edge_graph``): which receiver-sorted
edges are the two directions of one strut and so share a row of radial weights.  The builder is
plain torch, so these run on the CPU; the GPU part (bitwise-equal ``eelg_edge_embed`` feature rows
of partners) is in ``test_gpu_strut_weights.py``.
"""
import torch

from gnn import ops
from gnn.data import Data, collate
from gnn.model import EnergyEquivGNN


def _graph(struts, n=5, seed=0, both=True):
    """``struts``: (sender, receiver, shift, radius) -> a Data with every strut in both
    directions (``both``), the reverse with the negated shift and the same radius"""
    g = torch.Generator().manual_seed(seed)
    pos = torch.rand(n, 3, generator=g)
    snd, rcv, sh, rad = [], [], [], []
    for s, r, shift, radius in struts:
        snd.append(s), rcv.append(r), sh.append(shift), rad.append([radius])
    if both:
        for s, r, shift, radius in struts:
            snd.append(r), rcv.append(s), sh.append([-c for c in shift]), rad.append([radius])
    return Data(positions=pos, node_attrs=torch.ones(n, 1),
                edge_index=torch.tensor([snd, rcv], dtype=torch.int64),
                shifts=torch.tensor(sh, dtype=torch.float32).reshape(-1, 3),
                edge_attr=torch.tensor(rad, dtype=torch.float32).reshape(-1, 1),
                stiffness=torch.eye(6).unsqueeze(0))


# 5 nodes, periodic: two images of a strut between nodes 0 and 1, a strut from node 2 to its
# own image, struts across the cell faces
PERIODIC = [(0, 1, [0.0, 0.0, 0.0], 0.01), (0, 1, [1.0, 0.0, 0.0], 0.01), (1, 2, [0.0, 0.0, 0.0], 0.02),
            (2, 3, [0.0, 1.0, 0.0], 0.03), (3, 4, [0.0, 0.0, 0.0], 0.02), (4, 0, [0.0, 0.0, -1.0], 0.04),
            (2, 2, [1.0, 0.0, 0.0], 0.05)]


def _map(batch):
    csr = EnergyEquivGNN.edge_graph(batch)
    assert csr.strut is not None
    return csr, csr.strut


def _vectors(batch, csr):
    s, r = csr.sender.long(), csr.receiver.long()
    return (batch.positions[r] - batch.positions[s]) + batch.shifts[csr.perm]


def _check_consistent(batch, csr, m):
    e = csr.num_edges
    ar = torch.arange(e)
    assert m.row.dtype == torch.int32 and m.row.shape == (e,)
    assert torch.equal(m.partner[m.partner], ar)                      # an involution
    row = m.row.long()
    assert int(row.max()) + 1 == m.n_rows == m.rep.shape[0]
    assert torch.equal(row[m.rep], torch.arange(m.n_rows))            # rep: each row's first edge
    assert torch.equal(m.rep, torch.sort(m.rep)[0]) and bool((m.rep <= m.partner[m.rep]).all())
    paired = m.partner != ar
    assert torch.equal(row[m.partner], row)                           # partners share the row
    # a row holds a pair or a single edge, nothing else
    cnt = torch.zeros(m.n_rows, dtype=torch.int64).index_add_(0, row, torch.ones(e, dtype=torch.int64))
    assert torch.equal(cnt[row], 1 + paired.long())
    # what pairs them: swapped endpoints, exactly negated vectors, bitwise-equal radii
    v = _vectors(batch, csr)
    p = m.partner
    rad = batch.edge_attr[csr.perm].reshape(-1)
    assert torch.equal(csr.sender[p][paired], csr.receiver[paired])
    assert torch.equal(csr.receiver[p][paired], csr.sender[paired])
    assert torch.equal(v[p][paired], -v[paired])
    assert torch.equal(rad[p].view(torch.int32), rad.view(torch.int32))
    # hence bitwise-equal lengths, the only geometry the radial features read
    ln = v.pow(2).sum(1).sqrt()
    assert torch.equal(ln[p].view(torch.int32), ln.view(torch.int32))


def test_periodic_graphs_pair_every_strut():
    b = collate([_graph(PERIODIC, seed=1), _graph(PERIODIC, seed=2)])
    csr, m = _map(b)
    assert csr.num_edges == 4 * len(PERIODIC)
    assert m.n_rows == csr.num_edges // 2
    assert bool((m.partner != torch.arange(csr.num_edges)).all())
    _check_consistent(b, csr, m)
    # the two images between nodes 0 and 1 are told apart by their vectors: four edges, two rows
    s, r = csr.sender, csr.receiver
    img = torch.nonzero(((s == 0) & (r == 1)) | ((s == 1) & (r == 0))).reshape(-1)
    assert img.numel() == 4 and len(set(m.row[img].tolist())) == 2


def test_one_directional_and_unequal_radii_keep_their_rows():
    g = _graph(PERIODIC[:4], seed=3)
    # one one-directional edge, and a pair whose two directions carry different radii
    g.edge_index = torch.cat([g.edge_index, torch.tensor([[3, 1, 4], [4, 4, 1]])], 1)
    g.shifts = torch.cat([g.shifts, torch.zeros(3, 3)])
    g.edge_attr = torch.cat([g.edge_attr, torch.tensor([[0.02], [0.03], [0.035]])])
    b = collate([g])
    csr, m = _map(b)
    e = csr.num_edges
    assert e == 11 and m.n_rows == 4 + 3
    _check_consistent(b, csr, m)
    own = torch.nonzero(m.partner == torch.arange(e)).reshape(-1)
    assert sorted(zip(csr.sender[own].tolist(), csr.receiver[own].tolist())) == [(1, 4), (3, 4), (4, 1)]


def test_duplicate_edges_stay_alone():
    # the same directed edge twice has no unique partner: all four keep their own rows
    g = _graph([(0, 1, [0.0, 0.0, 0.0], 0.01), (0, 1, [0.0, 0.0, 0.0], 0.01)], n=2)
    b = collate([g])
    csr, m = _map(b)
    assert m.n_rows == csr.num_edges == 4
    _check_consistent(b, csr, m)


def test_zero_and_one_edge():
    g0 = _graph([], n=3)
    g0.edge_index = torch.zeros(2, 0, dtype=torch.int64)
    csr, m = _map(collate([g0]))
    assert csr.num_edges == 0 and m.n_rows == 0 and m.row.numel() == 0
    b1 = collate([_graph([(0, 1, [0.0, 0.0, 0.0], 0.01)], n=2, both=False)])
    csr, m = _map(b1)
    assert m.n_rows == 1 and m.row.tolist() == [0] and m.rep.tolist() == [0]
    _check_consistent(b1, csr, m)


def test_changed_geometry_rebuilds_the_map():
    b = collate([_graph(PERIODIC, seed=4)])
    csr, m = _map(b)
    assert EnergyEquivGNN.edge_graph(b) is csr                        # cached
    b.positions = b.positions.clone()                                 # same edge_index, new tensor
    csr2, m2 = _map(b)
    assert csr2 is csr and m2 is not m and m2.n_rows == m.n_rows     # one CSR, a new map
    b.edge_attr[0] += 0.001                                           # in place: the version counter
    csr3, m3 = _map(b)
    assert m3 is not m2 and m3.n_rows == m.n_rows + 1


def test_switch_off_builds_no_map(monkeypatch):
    monkeypatch.setattr(ops, "STRUT_WEIGHTS", False)
    b = collate([_graph(PERIODIC, seed=5)])
    assert EnergyEquivGNN.edge_graph(b).strut is None


def test_predicate_needs_enough_pairs():
    """``ops.strut_rows``: no map, a map without pairs or a switched-off path give per-edge weights"""
    mlp = torch.nn.Sequential(torch.nn.Linear(12, 64), torch.nn.SiLU(), torch.nn.Linear(64, 64),
                              torch.nn.SiLU(), torch.nn.Linear(64, 160, bias=False))
    b = collate([_graph(PERIODIC, seed=6)])
    csr, m = _map(b)
    assert ops.strut_rows(csr, "sum", torch.float32, mlp) is m
    assert ops.strut_rows(csr, "mean", torch.float32, mlp) is m
    assert ops.strut_rows(csr, "max", torch.float32, mlp) is None
    assert ops.strut_rows(csr, "pna", torch.float32, mlp) is None
    feats = torch.zeros(csr.num_edges, 12, requires_grad=True)
    assert ops.strut_rows(csr, "sum", torch.float32, mlp, feats) is None     # geometry gradients
    one_way = collate([_graph(PERIODIC, seed=6, both=False)])
    csr1, m1 = _map(one_way)
    assert m1.n_rows == csr1.num_edges and ops.strut_rows(csr1, "sum", torch.float32, mlp) is None


def test_the_step_builds_no_map(monkeypatch):
    """the model's own call in a step (``build=False``) takes the map an earlier call left and
    never builds one; callers with and without ``strut`` share one CSR"""
    calls = []
    real = ops.build_strut_map
    monkeypatch.setattr(ops, "build_strut_map", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    b = collate([_graph(PERIODIC, seed=7), _graph(PERIODIC[:5], seed=8)])
    csr = EnergyEquivGNN.edge_graph(b, build=False)
    assert csr.strut is None and not calls                    # a fresh batch: per-edge weights
    assert EnergyEquivGNN.edge_graph(b, strut=False) is csr and not calls
    m = EnergyEquivGNN.edge_graph(b).strut                    # ahead of the steps: built once
    assert m is not None and len(calls) == 1
    assert EnergyEquivGNN.edge_graph(b, build=False) is csr and csr.strut is m and len(calls) == 1
    _check_consistent(b, csr, m)
    b.shifts = b.shifts.clone()                               # other tensors: the step drops the map
    assert EnergyEquivGNN.edge_graph(b, build=False).strut is None and len(calls) == 1


def test_edge_attr_of_several_columns_gets_no_map():
    """``edge_ft`` forms such as 'L,r' give ``edge_attr`` [E, 2]: not one radius per edge, so no
    map and per-edge weights, and nothing raises (``RotateLat`` on such an item included)"""
    from gnn.lattice_data import RotateLat
    g = _graph(PERIODIC, seed=9)
    g.edge_attr = torch.cat([g.edge_attr, 2 * g.edge_attr], 1)
    g.stiffness = torch.zeros(1, 3, 3, 3, 3)
    g.compliance = torch.zeros(1, 3, 3, 3, 3)
    g.rel_dens, g.name = 0.01, "g"
    r = RotateLat(rotate=True, generator=torch.Generator().manual_seed(0))(g)
    assert r.edge_attr.shape == (14, 2)
    b = collate([r, RotateLat(rotate=False)(g)])
    assert EnergyEquivGNN.edge_graph(b).strut is None
