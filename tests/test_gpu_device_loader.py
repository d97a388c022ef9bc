"""``DeviceDataset`` / ``DeviceLoader`` on the device (``csrc/eelg_batch.hip``) against the CPU data
path it replaces: ``collate([RotateLat(...)(d) for d in selection]).to('cuda')``.

* no rotation / identity rotation: every field and all six CSR tensors bitwise equal, dtypes too;
* rotation: positions, shifts, stiffness and compliance against ``RotateLat(Q)`` evaluated in
  fp64 on the CPU, 1e-5 of each tensor's largest entry (the per-kernel bound for
  order-of-operations differences); everything else bitwise.
  Achieved on MI355X: positions 7.9e-08, shifts 7.4e-08, stiffness 1.5e-07, compliance 1.5e-07;
* the model fed by either batch gives bitwise equal stiffness, loss and parameter gradients, and
  a rotated batch rotates the prediction (5e-4, as ``test_rotatelat_rotates_the_prediction``).
"""
import ctypes

import numpy as np
import pytest
import torch

from helpers import params, record_parity
from helpers_device_loader import SEL, collated, five_graphs

pytestmark = pytest.mark.gpu
DEV = "cuda"
_FIELDS = ("positions", "node_attrs", "edge_index", "shifts", "edge_attr", "stiffness", "compliance",
           "rel_dens", "batch", "ptr")
_CSR = {"perm": torch.int64, "rowptr": torch.int32, "sender": torch.int32, "receiver": torch.int32,
        "sperm": torch.int32, "srowptr": torch.int32}


@pytest.fixture(scope="module")
def items():
    return five_graphs()


@pytest.fixture(scope="module")
def loader(items):
    from gnn import DeviceDataset, DeviceLoader
    return DeviceLoader(DeviceDataset(items, DEV), 2)


@pytest.fixture(scope="module")
def rotations():
    from gnn.lattice_data import rand_rotations
    return rand_rotations(len(SEL), torch.Generator().manual_seed(21))


def assert_same_batch(got, want, skip=()):
    """``got`` (device-assembled) equals ``want`` (CPU-collated, moved to the device) bitwise."""
    for k in _FIELDS:
        if k in skip:
            continue
        a, b = got[k], want[k]
        assert a.dtype == b.dtype and a.shape == b.shape and a.device == b.device, k
        assert torch.equal(a, b), k
    assert got.name == want.name and got.num_graphs == want.num_graphs
    for k, dt in _CSR.items():
        a, b = got.csr[k], want.csr[k].to(DEV)
        assert a.dtype == b.dtype == dt and a.shape == b.shape, k
        assert torch.equal(a, b), k


@pytest.mark.parametrize("sel", [SEL, [1], [3], [0, 1, 2, 3, 4], [3, 3], [4, 3]],
                         ids=["repeat", "one", "no_edges", "all", "no_edges_twice", "ends_empty"])
def test_unrotated_batch_is_bitwise_the_collated_one(items, loader, sel):
    want = collated(items, sel).to(DEV)
    got = loader.assemble(sel)
    assert_same_batch(got, want)
    assert got.rotation is None and got.graph_ids.tolist() == list(sel)


def test_identity_rotation_is_bitwise_the_unrotated_batch(items, loader):
    want = collated(items, SEL).to(DEV)
    assert_same_batch(loader.assemble(SEL, Q=torch.eye(3, dtype=torch.float64)), want)
    got = loader.assemble(SEL, Q=torch.eye(3).expand(len(SEL), 3, 3).to(DEV))     # device rotations
    assert_same_batch(got, want)
    assert got.rotation.shape == (len(SEL), 3, 3) and got.rotation.dtype == torch.float32


def test_rotated_batch_matches_rotatelat_in_fp64(items, loader, rotations):
    import copy
    items64 = []
    for d in items:
        e = copy.copy(d)
        for k in ("positions", "shifts", "stiffness", "compliance"):
            e[k] = d[k].double()
        items64.append(e)
    want = collated(items64, SEL, rotations)
    plain = collated(items, SEL).to(DEV)
    got = loader.assemble(SEL, Q=rotations)
    errs = {}
    for k in ("positions", "shifts", "stiffness", "compliance"):
        w = want[k]
        assert w.dtype == torch.float64 and got[k].dtype == torch.float32 and got[k].shape == w.shape
        errs[k] = float((got[k].double().cpu() - w).abs().max() / w.abs().max())
    print("device loader rotation errors", errs)
    record_parity("device_loader_rotation", **errs)
    assert_same_batch(got, plain, skip=("positions", "shifts", "stiffness", "compliance"))
    assert not torch.equal(got.positions, plain.positions)
    for k, v in errs.items():
        assert v < 1e-5, (k, v)


def _model(items):
    from gnn.model import EnergyEquivGNN
    rmax = float(max(float(d.edge_attr.max()) for d in items if d.num_edges))
    torch.manual_seed(0)
    return EnergyEquivGNN(params(2, lmax=2, max_edge_radius=rmax)).to(DEV)


def _step(m, b):
    from gnn.train import stiffness_loss
    m.zero_grad(set_to_none=True)
    c = m(b)["stiffness"]
    loss = stiffness_loss(c, b.stiffness)
    loss.backward()
    return c.detach().clone(), loss.detach().clone(), {k: p.grad.clone() for k, p in m.named_parameters()
                                                       if p.grad is not None}


def test_model_is_bitwise_the_same_on_either_batch(items, loader):
    m = _model(items)
    c0, l0, g0 = _step(m, collated(items, SEL).to(DEV))
    c1, l1, g1 = _step(m, loader.assemble(SEL))
    assert torch.equal(c0, c1) and torch.equal(l0, l1)
    assert g0.keys() == g1.keys() and len(g0) > 0
    for k in g0:
        assert torch.equal(g0[k], g1[k]), k


def test_rotated_batch_rotates_the_prediction(items, loader, rotations):
    from gnn.lattice_data import mandel_rotation
    m = _model(items)
    with torch.no_grad():
        c0 = m(loader.assemble(SEL))["stiffness"].double().cpu().numpy()
        c1 = m(loader.assemble(SEL, Q=rotations))["stiffness"].double().cpu().numpy()
    mq = mandel_rotation(rotations.numpy())
    want = mq @ c0 @ mq.transpose(0, 2, 1)
    err = float(np.abs(c1 - want).max() / np.abs(want).max())
    print("rotated prediction error", err)
    record_parity("device_loader_equivariance", stiffness=err)
    assert err < 5e-4, err


def test_two_loaders_with_one_seed_give_identical_batches(items):
    from gnn import DeviceDataset, DeviceLoader
    dds = DeviceDataset(items, DEV)
    a = DeviceLoader(dds, 2, shuffle=True, seed=5, rotate=True)
    b = DeviceLoader(dds, 2, shuffle=True, seed=5, rotate=True)
    epochs = []
    for _ in range(2):
        ids = []
        for x, y in zip(a, b):
            assert_same_batch(x, y)
            assert torch.equal(x.rotation, y.rotation) and x.graph_ids.tolist() == y.graph_ids.tolist()
            ids.append(x.graph_ids.tolist())
        assert [len(i) for i in ids] == [2, 2, 1] and sorted(sum(ids, [])) == [0, 1, 2, 3, 4]
        epochs.append((ids, x.rotation.clone()))
    assert epochs[0][0] != epochs[1][0] and not torch.equal(epochs[0][1], epochs[1][1])


def test_assembly_sorts_nothing_and_never_waits(items, loader, rotations, monkeypatch):
    from gnn import ops
    want = collated(items, SEL).to(DEV)
    loader.assemble(SEL)                               # library loaded, descriptors cached

    def refuse(*a, **k):
        raise AssertionError("the batch assembly may not sort, search or read a device tensor back")
    for name in ("sort", "argsort", "searchsorted", "bincount"):
        monkeypatch.setattr(torch, name, refuse)
    for name in ("item", "tolist", "sort", "argsort", "cpu"):
        monkeypatch.setattr(torch.Tensor, name, refuse)
    monkeypatch.setattr(ops.TIMER, "enabled", True)
    monkeypatch.setattr(ops.TIMER, "records", {})
    got = loader.assemble(SEL)
    launches = {k: len(v) for k, v in ops.TIMER.records.items()}
    rot = loader.assemble(SEL, Q=rotations)
    monkeypatch.undo()
    assert launches == {"batch_assemble": 1, "mandel_rotate": 2}
    assert_same_batch(got, want)
    assert rot.rotation is not None


def test_c_abi_guards(loader):
    from gnn import _lib
    lib = _lib.load()
    src = loader._source()
    out = _lib.BatchOut()
    stream = _lib.stream(torch.zeros(1, device=DEV))
    # a zero-graph selection is a no-op, whatever the pointers
    assert lib.eelg_batch_assemble(ctypes.byref(src), None, None, 0, 0, 0, ctypes.byref(out), stream) == 0
    assert lib.eelg_mandel_rotate(None, 5, None, None, 0, None, stream) == 0
    # a bad width is refused before anything is launched: the outputs keep their contents
    good = loader.assemble([0])
    buf = {k: torch.full_like(getattr(good, k), 7) for k in ("positions", "node_attrs", "batch", "ptr",
                                                              "edge_index", "shifts", "edge_attr")}
    buf.update({k: torch.full_like(v, 7) for k, v in good.csr.items()})
    for k, v in buf.items():
        setattr(out, k, v.data_ptr())
    table = torch.tensor([[0, 17], [0, int(good.edge_index.shape[1])], [0, 0], [0, 0]], dtype=torch.int32,
                         device=DEV)
    for field, value in (("node_w", 0), ("edge_w", _lib.BATCH_MAXW + 1)):
        bad = _lib.BatchSrc.from_buffer_copy(src)
        setattr(bad, field, value)
        rc = lib.eelg_batch_assemble(ctypes.byref(bad), _lib.ptr(table), None, 1, 17,
                                     int(good.edge_index.shape[1]), ctypes.byref(out), stream)
        assert rc == -2 and b"width" in lib.eelg_last_error()
    assert lib.eelg_batch_assemble(ctypes.byref(src), _lib.ptr(table), None, 1, -1, 0, ctypes.byref(out),
                                   stream) == -2
    assert lib.eelg_mandel_rotate(None, 5, None, None, 1, None, stream) == -2
    torch.cuda.synchronize()
    assert all(bool((v == 7).all()) for v in buf.values())
    # and the well-formed call fills them
    assert lib.eelg_batch_assemble(ctypes.byref(src), _lib.ptr(table), None, 1, 17,
                                   int(good.edge_index.shape[1]), ctypes.byref(out), stream) == 0
    assert torch.equal(buf["positions"], good.positions) and torch.equal(buf["perm"], good.csr["perm"])
