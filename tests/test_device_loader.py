"""Host side of the device-resident dataset / loader (``gnn/device_data.py``): the Mandel rotation
and the batched random rotations, the packing arithmetic (per-graph CSR pieces, concatenated with
offsets == the collated batch's CSR, exactly) and the loader's order.  No device is needed."""
import numpy as np
import pytest
import torch

from helpers_device_loader import SEL, collated, five_graphs


@pytest.fixture(scope="module")
def items():
    return five_graphs()


@pytest.fixture(scope="module")
def packed(items):
    from gnn.device_data import pack_graphs
    return pack_graphs(items)


def _rotations(n, seed):
    from gnn.lattice_data import rand_rotations
    return rand_rotations(n, torch.Generator().manual_seed(seed))


def test_mandel_rotation_is_orthogonal_and_matches_the_cartesian_route():
    from gnn.lattice_data import cart4_to_mandel, mandel_rotation, mandel_to_cart4
    rng = np.random.default_rng(0)
    qs = _rotations(8, 3).numpy()
    ms = mandel_rotation(qs)
    assert ms.shape == (8, 6, 6) and ms.dtype == np.float64
    assert np.abs(ms @ ms.transpose(0, 2, 1) - np.eye(6)).max() < 1e-12
    assert np.array_equal(mandel_rotation(np.eye(3)), np.eye(6))
    for q, m in zip(qs, ms):
        a = rng.normal(size=(6, 6))
        c = a @ a.T / 6 + 0.5 * np.eye(6)
        want = cart4_to_mandel(np.einsum("ijkl,ai,bj,ck,dl->abcd", mandel_to_cart4(c), q, q, q, q))
        assert np.abs(m @ c @ m.T - want).max() < 1e-12 * np.abs(want).max()
    # torch in, torch out
    mt = mandel_rotation(torch.from_numpy(qs[0]))
    assert torch.is_tensor(mt) and mt.dtype == torch.float64 and np.array_equal(mt.numpy(), ms[0])


def test_rand_rotations_are_proper_and_replayable():
    q = _rotations(64, 11)
    assert q.shape == (64, 3, 3) and q.dtype == torch.float64
    assert float((q.transpose(1, 2) @ q - torch.eye(3, dtype=torch.float64)).abs().max()) < 1e-12
    assert float((torch.linalg.det(q) - 1).abs().max()) < 1e-12
    assert torch.equal(q, _rotations(64, 11))
    assert not torch.equal(q, _rotations(64, 12))


def test_device_dataset_refuses_a_cpu_device(items):
    from gnn import DeviceDataset
    with pytest.raises(RuntimeError, match="runs only on a HIP device"):
        DeviceDataset(items, "cpu")


def test_assemble_refuses_cpu_packed_graphs(packed):
    from gnn import DeviceLoader
    with pytest.raises(RuntimeError, match="runs only on a HIP device"):
        DeviceLoader(packed, 2).assemble([0, 1])


def test_packed_pieces_are_each_graphs_own_csr(items, packed):
    from gnn.data import build_edge_csr
    from gnn.lattice_data import RotateLat
    t = packed.tensors
    assert len(packed) == 5
    assert packed.node_ptr.tolist() == [0, 17, 41, 72, 73, 80]
    assert t["perm"].dtype == t["sperm"].dtype == t["rowend"].dtype == t["sender"].dtype == torch.int32
    for g, d in enumerate(items):
        n0, n1, e0, e1 = *packed.node_ptr[g:g + 2], *packed.edge_ptr[g:g + 2]
        assert (n1 - n0, e1 - e0) == (d.num_nodes, d.num_edges)
        csr = build_edge_csr(d.edge_index, d.num_nodes)
        assert torch.equal(t["perm"][e0:e1].long(), csr["perm"])
        assert torch.equal(t["sperm"][e0:e1], csr["sperm"])
        assert torch.equal(t["rowend"][n0:n1], csr["rowptr"][1:])
        assert torch.equal(t["srowend"][n0:n1], csr["srowptr"][1:])
        assert torch.equal(t["sender"][e0:e1].long(), d.edge_index[0])
        assert torch.equal(t["receiver"][e0:e1].long(), d.edge_index[1])
        assert torch.equal(t["positions"][n0:n1], d.positions) and torch.equal(t["shifts"][e0:e1], d.shifts)
        plain = RotateLat(rotate=False)(d)          # the Mandel targets, bitwise
        assert torch.equal(t["stiffness"][g], plain.stiffness[0])
        assert torch.equal(t["compliance"][g], plain.compliance[0])
    # the isolated-node graph: repeated row ends in the middle and at the end
    iso = t["rowend"][73:80].tolist()
    # (nodes 2, 4 and 6 receive nothing)
    assert iso[2] == iso[1] and iso[4] == iso[3] and iso[6] == iso[5] == 12
    assert packed.names == [d.name for d in items]
    assert packed.rel_dens.dtype == np.float32 and packed.rel_dens.shape == (5,)


def test_concatenated_pieces_with_offsets_are_the_collated_csr(items, packed):
    """What ``eelg_batch_assemble`` computes, in numpy: for a selection with a repeat the local
    CSR pieces plus the output offsets equal ``collate(...).csr`` exactly."""
    want = collated(items, SEL)
    t = {k: v.numpy() for k, v in packed.tensors.items()}
    perm, sperm, snd, rcv, rowptr, srowptr, ei = [], [], [], [], [0], [0], []
    noff = eoff = 0
    for g in SEL:
        n0, n1, e0, e1 = *packed.node_ptr[g:g + 2], *packed.edge_ptr[g:g + 2]
        p = t["perm"][e0:e1].astype(np.int64)
        perm.append(p + eoff)
        sperm.append(t["sperm"][e0:e1] + eoff)
        snd.append(t["sender"][e0:e1][p] + noff)
        rcv.append(t["receiver"][e0:e1][p] + noff)
        rowptr.extend((t["rowend"][n0:n1] + eoff).tolist())
        srowptr.extend((t["srowend"][n0:n1] + eoff).tolist())
        ei.append(np.stack([t["sender"][e0:e1], t["receiver"][e0:e1]]).astype(np.int64) + noff)
        noff += n1 - n0
        eoff += e1 - e0
    assert np.array_equal(np.concatenate(ei, 1), want.edge_index.numpy())
    got = {"perm": np.concatenate(perm), "sperm": np.concatenate(sperm), "sender": np.concatenate(snd),
           "receiver": np.concatenate(rcv), "rowptr": np.asarray(rowptr), "srowptr": np.asarray(srowptr)}
    for k, v in got.items():
        assert np.array_equal(v, want.csr[k].numpy()), k


def test_degree_stats_and_max_edge_radius_are_the_whole_sets(items, packed):
    from gnn import degree_stats
    b = collated(items, range(5))
    assert packed.degree_stats() == degree_stats(b.edge_index, b.node_attrs.shape[0])
    assert packed.max_edge_radius == float(b.edge_attr.max())


def test_pack_time_checks(items):
    import copy
    from gnn.device_data import _check_extents, pack_graphs
    empty = copy.copy(items[3])
    empty.positions, empty.node_attrs = torch.zeros(0, 3), torch.zeros(0, 1)
    with pytest.raises(ValueError, match="no nodes"):
        pack_graphs([items[0], empty])
    wide = copy.copy(items[4])
    wide.edge_attr = torch.cat([wide.edge_attr, wide.edge_attr], 1)
    with pytest.raises(ValueError, match="field widths"):
        pack_graphs([items[0], wide])
    with pytest.raises(ValueError, match="2\\*\\*31"):
        _check_extents(2 ** 31, 5)
    with pytest.raises(ValueError, match="2\\*\\*31"):
        _check_extents(5, 2 ** 31)
    _check_extents(2 ** 31 - 1, 2 ** 31 - 1)


def test_mandel_targets_are_taken_as_they_are():
    """Synthetic lattices carry [1, 6, 6] Mandel targets, a tensor rel_dens and no compliance."""
    from gnn import SyntheticLattices, collate
    from gnn.device_data import pack_graphs
    ds = SyntheticLattices(3, 12, 48, seed=5)
    p = pack_graphs([ds[g] for g in range(3)])
    b = collate([ds[g] for g in range(3)])
    assert torch.equal(p.tensors["stiffness"], b.stiffness) and "compliance" not in p.tensors
    assert np.array_equal(p.rel_dens, b.rel_dens.numpy())
    assert p.max_edge_radius == ds.max_edge_radius


class _Names:
    """A dataset whose items collate to their own index (``DataLoader`` goes through collate)."""

    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        from gnn.data import Data
        return Data(node_attrs=torch.ones(1, 1), edge_index=torch.zeros(2, 0, dtype=torch.long), gid=int(i))


def test_order_is_the_cpu_loaders(packed):
    from gnn import DataLoader, DeviceLoader
    from gnn.device_data import epoch_batches
    ref = DataLoader(_Names(5), 2, shuffle=True, seed=9)
    dl = DeviceLoader(packed, 2, shuffle=True, seed=9)
    assert len(dl) == len(ref) == 3
    epochs = []
    for epoch in range(2):
        want = [b.gid.tolist() for b in ref]
        got = [ids.tolist() for ids in dl.order(epoch)]
        assert got == want and [len(g) for g in got] == [2, 2, 1]      # ragged last batch
        epochs.append(got)
    assert epochs[0] != epochs[1]
    # unshuffled, drop_last
    assert [i.tolist() for i in epoch_batches(5, 2)] == [[0, 1], [2, 3], [4]]
    assert [i.tolist() for i in epoch_batches(5, 2, drop_last=True)] == [[0, 1], [2, 3]]
    assert len(DeviceLoader(packed, 2, drop_last=True)) == 2
    with pytest.raises(ValueError):
        epoch_batches(5, 2, rank=2, world=2)


def test_rank_blocks_follow_shard_indices():
    from gnn.device_data import epoch_batches
    from gnn.parallel import shard_indices
    n, per, world = 23, 3, 2
    order = np.random.default_rng(4 + 1).permutation(n)
    for drop_last, steps in ((True, 3), (False, 4)):
        for rank in range(world):
            got = epoch_batches(n, per, shuffle=True, seed=4, epoch=1, rank=rank, world=world,
                                drop_last=drop_last)
            assert len(got) == steps
            for step, ids in enumerate(got):
                assert ids.tolist() == order[shard_indices(n, rank, world, per, step)].tolist()


def test_loader_rotations_are_replayable(packed):
    from gnn import DeviceLoader
    a, b = DeviceLoader(packed, 2, seed=3, rotate=True), DeviceLoader(packed, 2, seed=3, rotate=True)
    assert torch.equal(a.rotations(1, 2, 4), b.rotations(1, 2, 4))
    assert not torch.equal(a.rotations(1, 2, 4), a.rotations(1, 3, 4))
    assert not torch.equal(a.rotations(1, 2, 4), a.rotations(0, 2, 4))
