"""``eelg_stiffness_metrics`` (``csrc/eelg_metrics.hip``) on the device.

Accuracy is measured against the fp64 restatement (``helpers_metrics.reference64``) over the
hostile pairs (every matrix of the hostile set as target against every other one as prediction,
90 graphs): per column group the largest error over the set, scalar columns relative to the
graph's own fp64 value, eigenvalues relative to the matrix's largest |eigenvalue|.  Bound: 4x the
same figure of the composed fp32 torch form evaluated on the CPU on the same inputs (none of the
kernel's code; the margin for a second fp32 summation order, as ``test_gpu_nnconv``).

Measured on MI355X, largest ratio fused / baseline over n_dirs in {1, 63, 64, 65, 250} and scale in
{1, 10} (every case in profiles/eval_summary.md): mseloss 1.20 (1.6e-7 / 1.3e-7), loss 0.94,
dir_loss 1.85 (n_dirs = 1, where one pair nearly cancels: 8.1e-6 / 4.4e-6; <= 1.19 otherwise),
mean_stiffness 1.87 (4.3e-7 / 2.3e-7), eigenvalues 0.23 (3.9e-8 .. 6.0e-8 / 2.6e-7 .. 3.0e-7).
Fused against composed on the device: <= 4.0e-7.

Everything else is bitwise: a graph's row does not depend on the batch around it, on its
position, on the run, or on the upper triangle (eigenvalue columns); a NaN stays in its row.
"""
import numpy as np
import pytest
import torch

from helpers import params, record_parity
from helpers_metrics import GROUPS, directions, hostile_pairs, normalised_errors, reference64

pytestmark = pytest.mark.gpu
DEV = "cuda"
N_DIRS = (1, 63, 64, 65, 250)        # below, at and above one direction per lane; the reference's 250
_CASES = {}


def case(n_dirs: int, scale: float = 1.0):
    """Inputs, fp64 reference, CPU baseline errors and the fused rows of the 90 hostile pairs:
    computed once per (n_dirs, scale) and shared, never modified."""
    key = (n_dirs, scale)
    if key not in _CASES:
        from gnn.metrics import stiffness_metrics, stiffness_metrics_composed
        pred, target = hostile_pairs()
        d = directions(n_dirs)
        ref = reference64(pred, target, d, scale)
        base = normalised_errors(stiffness_metrics_composed(pred, target, d, scale), ref)
        rows = stiffness_metrics(pred.to(DEV), target.to(DEV), d.to(DEV), scale)
        _CASES[key] = dict(pred=pred.to(DEV), target=target.to(DEV), dirs=d.to(DEV), ref=ref, base=base,
                           rows=rows)
    return _CASES[key]


@pytest.mark.parametrize("n_dirs,scale", [(1, 1.0), (63, 1.0), (64, 10.0), (65, 1.0), (250, 1.0), (250, 10.0)])
def test_hostile_pairs_within_4x_of_the_composed_cpu_form(n_dirs, scale):
    c = case(n_dirs, scale)
    assert c["rows"].shape == (90, 16) and c["rows"].dtype == torch.float32
    got = normalised_errors(c["rows"], c["ref"])
    print(f"stiffness metrics n_dirs={n_dirs} scale={scale}: fused", got, "composed on CPU", c["base"])
    record_parity(f"stiffness_metrics_p{n_dirs}_s{int(scale)}", fused=got, composed_cpu=c["base"])
    eig = c["rows"][:, 4:].cpu()
    assert bool((eig[:, :6].diff(dim=1) >= 0).all()) and bool((eig[:, 6:].diff(dim=1) >= 0).all())
    for k in GROUPS:
        assert got[k] <= 4 * c["base"][k], (k, got[k], c["base"][k])


@pytest.mark.parametrize("n_dirs", N_DIRS)
@pytest.mark.parametrize("n_graphs", [1, 3, 65])
def test_a_row_is_bitwise_independent_of_batch_and_position(n_graphs, n_dirs):
    """Graphs 7 .. 7 + n_graphs of the 90 pairs, launched on their own (so at other positions, in
    another batch size; n_graphs = 1: alone): bitwise the rows of the 90-graph launch, on two runs."""
    from gnn.metrics import stiffness_metrics
    c = case(n_dirs)
    sl = slice(7, 7 + n_graphs)
    a = stiffness_metrics(c["pred"][sl], c["target"][sl], c["dirs"])
    b = stiffness_metrics(c["pred"][sl], c["target"][sl], c["dirs"])
    assert a.shape == (n_graphs, 16)
    assert torch.equal(a, b)
    assert torch.equal(a, c["rows"][sl])


def test_out_slice_of_a_sentinel_buffer():
    from gnn.metrics import stiffness_metrics
    c = case(65)
    buf = torch.full((90 + 5, 16), 7.0, device=DEV)
    got = stiffness_metrics(c["pred"], c["target"], c["dirs"], out=buf[2:92])
    assert got.data_ptr() == buf[2:92].data_ptr()
    assert torch.equal(buf[2:92], c["rows"])
    assert bool((buf[:2] == 7).all()) and bool((buf[92:] == 7).all())
    with pytest.raises(ValueError):
        stiffness_metrics(c["pred"], c["target"], c["dirs"], out=buf[:90, :8])


def test_upper_triangle_is_ignored_by_the_eigenvalues():
    from gnn.metrics import stiffness_metrics
    c = case(65)
    pred, target = c["pred"].clone(), c["target"].clone()
    iu = torch.triu_indices(6, 6, 1, device=DEV)
    pred[:, iu[0], iu[1]] = pred[:, iu[0], iu[1]] * 1.5 + 3.0
    target[:, iu[0], iu[1]] = -target[:, iu[0], iu[1]]
    rows = stiffness_metrics(pred, target, c["dirs"])
    assert torch.equal(rows[:, 4:], c["rows"][:, 4:])
    assert not torch.equal(rows[:, :4], c["rows"][:, :4])


def test_nan_stays_in_its_row():
    """Graph 3: the whole prediction NaN; graph 5: one NaN in the prediction's lower triangle;
    graph 8: one NaN in its upper triangle.  The launch returns; the prediction-dependent columns
    of those graphs are NaN (the eigenvalues of graph 8 are not: the entry is not read), their
    target-only columns and every other row are bitwise unchanged."""
    from gnn.metrics import stiffness_metrics
    c = case(250)
    pred = c["pred"].clone()
    pred[3] = float("nan")
    pred[5, 4, 2] = float("nan")
    pred[8, 1, 4] = float("nan")
    rows = stiffness_metrics(pred, c["target"], c["dirs"])
    torch.cuda.synchronize()
    keep = torch.ones(90, dtype=torch.bool, device=DEV)
    keep[[3, 5, 8]] = False
    assert torch.equal(rows[keep], c["rows"][keep])
    for g in (3, 5, 8):
        assert bool(torch.isnan(rows[g, :3]).all())
        assert torch.equal(rows[g, 3:10], c["rows"][g, 3:10])
    assert bool(torch.isnan(rows[3, 10:]).all()) and bool(torch.isnan(rows[5, 10:]).all())
    assert torch.equal(rows[8, 10:], c["rows"][8, 10:])


@pytest.mark.parametrize("n_dirs,scale", [(65, 1.0), (250, 10.0)])
def test_fused_agrees_with_composed_on_the_device(n_dirs, scale, monkeypatch):
    """EELG_METRICS_FUSED=0 (the composed torch form on the device) against the fused kernel,
    normalised like the errors against fp64, within the same bound."""
    from gnn import metrics
    c = case(n_dirs, scale)
    monkeypatch.setattr(metrics, "FUSED", False)
    comp = metrics.stiffness_metrics(c["pred"], c["target"], c["dirs"], scale)
    monkeypatch.undo()
    assert comp.is_cuda and comp.shape == (90, 16)
    diff = {}
    rows, comp64 = c["rows"].double().cpu(), comp.double().cpu()
    for k, sl in GROUPS.items():
        mag = c["ref"][:, sl].abs().max(dim=1, keepdim=True).values
        diff[k] = float(((rows[:, sl] - comp64[:, sl]).abs() / mag).max())
    print(f"fused against composed on the device n_dirs={n_dirs} scale={scale}", diff)
    record_parity(f"stiffness_metrics_fused_vs_composed_p{n_dirs}_s{int(scale)}", **diff)
    for k in GROUPS:
        assert diff[k] <= 4 * c["base"][k], (k, diff[k], c["base"][k])


def test_c_abi_guards():
    from gnn import _lib
    lib = _lib.load()
    c = case(65)
    stream = _lib.stream(c["pred"])
    fn = lib.eelg_stiffness_metrics
    # zero graphs: a no-op, whatever the pointers and the direction count
    assert fn(None, None, None, 0, 65, 1.0, None, stream) == 0
    assert fn(None, None, None, 0, 0, 1.0, None, stream) == 0
    out = torch.full((3, 16), 7.0, device=DEV)
    p, t, d, o = (_lib.ptr(c["pred"]), _lib.ptr(c["target"]), _lib.ptr(c["dirs"]), _lib.ptr(out))
    for args, word in (((None, t, d, 3, 65, 1.0, o), b"null"), ((p, None, d, 3, 65, 1.0, o), b"null"),
                       ((p, t, None, 3, 65, 1.0, o), b"null"), ((p, t, d, 3, 65, 1.0, None), b"null"),
                       ((p, t, d, -1, 65, 1.0, o), b"graphs"), ((p, t, d, 3, 0, 1.0, o), b"directions"),
                       ((p, t, d, 3, -5, 1.0, o), b"directions")):
        assert fn(*args, stream) == -2
        assert word in lib.eelg_last_error()
    torch.cuda.synchronize()
    assert bool((out == 7).all())
    # and the well-formed call fills them
    assert fn(p, t, d, 3, 65, 1.0, o, stream) == 0
    assert torch.equal(out, c["rows"][:3])


# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def five():
    from gnn import DeviceDataset, DeviceLoader, EnergyEquivGNN, LightningWrappedModel
    from helpers_device_loader import five_graphs
    items = five_graphs()
    rmax = float(max(float(d.edge_attr.max()) for d in items if d.num_edges))
    torch.manual_seed(0)
    wrapped = LightningWrappedModel(EnergyEquivGNN, params(max_edge_radius=rmax)).to(DEV)
    return wrapped, DeviceLoader(DeviceDataset(items, DEV), 2)


def test_evaluate_is_bitwise_obtain_errors_over_predict_step(five, monkeypatch):
    from gnn import ops
    from gnn.metrics import evaluate, metric_directions, obtain_errors
    wrapped, loader = five
    with torch.no_grad():
        results = [wrapped.predict_step(b, i) for i, b in enumerate(loader)]
    want = obtain_errors(results, "test", directions=metric_directions(250, seed=0, device=DEV))
    monkeypatch.setattr(ops.TIMER, "enabled", True)
    monkeypatch.setattr(ops.TIMER, "records", {})
    table = evaluate(wrapped.model, loader, "test", seed=0)
    launches = len(ops.TIMER.records.get("stiffness_metrics", []))
    monkeypatch.undo()
    assert len(loader) == 3 and launches == 3
    assert len(table) == 5 and table.name.tolist() == want.name.tolist() and table.tag.tolist() == ["test"] * 5
    assert np.array_equal(table.rel_dens, want.rel_dens) and table.rel_dens.dtype == want.rel_dens.dtype
    for k in ("mean_stiffness", "loss", "mseloss", "dir_loss", "target_eig", "predicted_eig"):
        assert table[k].dtype == np.float32 and np.array_equal(table[k], want[k]), k
    assert np.isfinite(table.predicted_eig).all() and float(table.loss.min()) > 0
    # scale 10 on both matrices against the fp64 restatement of the same predictions
    pred = torch.cat([r[0]["stiffness"] for r in results])
    target = torch.cat([r[1]["stiffness"] for r in results])
    ref = reference64(pred, target, metric_directions(250, seed=0), 10.0)
    got = np.concatenate([table.mseloss[:, None], table.loss[:, None], table.dir_loss[:, None],
                          table.mean_stiffness[:, None], table.target_eig, table.predicted_eig], axis=1)
    errs = normalised_errors(torch.from_numpy(got), ref)
    assert max(errs.values()) < 1e-5, errs          # the per-kernel bound


def test_metric_call_and_validation_step_never_wait(five, monkeypatch):
    from gnn.metrics import metric_directions, stiffness_metrics, validation_metrics
    wrapped, loader = five
    batch = loader.assemble([0, 4])
    d = metric_directions(250, seed=0, device=DEV)
    with torch.no_grad():
        pred = wrapped.model(batch)["stiffness"]
    buf = torch.zeros(5, 16, device=DEV)
    want = stiffness_metrics(pred, batch.stiffness, d, 10.0)

    def refuse(*a, **k):
        raise AssertionError("the metrics may not read a device tensor back")
    for name in ("item", "tolist", "cpu"):
        monkeypatch.setattr(torch.Tensor, name, refuse)
    stiffness_metrics(pred, batch.stiffness, d, 10.0, out=buf[1:3])
    val = validation_metrics(pred, batch.stiffness, d)
    monkeypatch.undo()
    assert torch.equal(buf[1:3], want)
    assert val["val_loss"].is_cuda and val["val_loss"].dim() == 0 and val["val_stiff_dir_loss"].dim() == 0
    loss = wrapped.validation_step(batch, 0, directions=d)
    assert torch.equal(loss, val["val_loss"])
    assert torch.equal(wrapped.val_metrics["val_stiff_dir_loss"], val["val_stiff_dir_loss"])
    want_loss = torch.nn.functional.mse_loss(pred, batch.stiffness)
    torch.testing.assert_close(loss, want_loss, rtol=1e-5, atol=0)
