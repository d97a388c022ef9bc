"""``eelg_transverse_props`` / ``eelg_transverse_props_bwd`` (``csrc/eelg_transverse.hip``) and the
transverse keywords of ``gnn.property_sensitivity`` / ``gnn.optimize_design`` on the device.

Accuracy is measured against the rank-4 fp64 restatement (``helpers_transverse.reference``) over the
17 matrices of ``spd_set()`` (condition numbers 4 .. 1e4), normalised as ``test_transverse`` says.
Bound: 4x the same figure of the restatement run in fp32 on the CPU on the same inputs (none of the
kernel's code), at least 4 fp32 ulps of the column's largest magnitude; gradient and ``n_ext`` matrix
by matrix, without the excluded pairs and the rounding-decided extremes ``test_transverse`` names.

Measured on MI355X, fused / fp32 restatement on the CPU, P in {1, 63, 64, 65, 250}: G_lo, G_hi, G_min,
G_max <= 5.9e-8 against 5.1e-6 .. 5.4e-5 (ratio <= 0.010); nu_lo, nu_hi, nu_min, nu_max <= 4.6e-7 against
8.0e-6 .. 3.2e-4 (<= 0.015); beta, beta_min, beta_max <= 5.1e-8 against 2.9e-6 .. 1.3e-5 (<= 0.007);
gradient per matrix <= 3.8e-7 against 4.9e-8 .. 1.1 (ratio <= 0.80, where the baseline itself is at
4e-7; 0.26 .. 0.60 for P other than 64); n_ext <= 5.6e-8 against 4.7e-8 .. 0.92; excluded pairs 0, 2, 2, 2
and 5.  Fused against composed on the device: rows bitwise equal, gradient <= 1.3e-7, n_ext 1.9e-9.
``property_sensitivity`` with transverse weights, fused against the composed form's autograd through
the same model: positions, radii and shifts bitwise equal; baseline (the fp32 CPU restatement's
cotangent through ``stiffness_sensitivity``) 3.3e-7 / 3.7e-7 / 4.7e-7.

Everything else is bitwise: a graph's rows and gradient do not depend on the batch around it, on
its position or on the run; a matrix that is not positive definite stays in its row.
"""
import pytest
import torch

from helpers import record_parity
from helpers_metrics import directions
from helpers_transverse import (bad_batch, bounds, check_bad_batch, check_tie, cotangents, crystal_directions, errors,
                                excluded, gradient, gradient_error, normal_error, reference, reference_fn, spd_set,
                                tie_case, within)

pytestmark = pytest.mark.gpu
DEV = "cuda"
N_DIRS = (1, 63, 64, 65, 250)        # below, at and above one direction per lane; the metrics' 250
_CASES = {}


def fused(c, d, gp, gt):
    from gnn.transverse import transverse_properties
    x = c.clone().requires_grad_(True)
    props, t, arg, n_ext = transverse_properties(x, d)
    outs, gs = ([props, t], [gp, gt]) if t.shape[1] else ([props], [gp])
    g, = torch.autograd.grad(outs, [x], gs)
    return props.detach(), t.detach(), arg, n_ext, g


def case(n_dirs: int):
    """Inputs, fp64 truth, CPU fp32 baseline errors, cotangents and the fused rows and gradient of
    the SPD set: computed once per direction count and shared, never modified."""
    if n_dirs not in _CASES:
        c, d = spd_set(), directions(n_dirs)
        ref = reference(c, d)
        b32 = reference(c, d, torch.float32)
        gp, gt = cotangents(ref)
        gref = gradient(reference_fn(torch.float64), c.double(), d, gp, gt)
        gbase = gradient_error(gradient(reference_fn(torch.float32), c, d, gp, gt), gref)
        n32 = b32["normals"][torch.arange(17)[:, None], b32["arg"][:, :4], torch.arange(4)[None]]
        cd, dd, gpd, gtd = c.to(DEV), d.to(DEV), gp.float().to(DEV), gt.float().to(DEV)
        props, t, arg, n_ext, g = fused(cd, dd, gpd, gtd)
        _CASES[n_dirs] = dict(c=cd, d=dd, ref=ref, base=errors(b32["props"], b32["t_dir"], ref), gp=gpd, gt=gtd,
                              gref=gref, gbase=gbase, nbase=normal_error(n32, b32["arg"], ref), props=props, t=t,
                              arg=arg, n_ext=n_ext, g=g)
    return _CASES[n_dirs]


@pytest.mark.parametrize("n_dirs", N_DIRS)
def test_spd_set_forward_within_4x_of_the_fp32_restatement(n_dirs):
    k = case(n_dirs)
    props, t, arg, n_ext = k["props"], k["t"], k["arg"], k["n_ext"]
    assert props.shape == (17, 7) and t.shape == (17, n_dirs, 5) and arg.shape == (17, 6) and n_ext.shape == (17, 4, 3)
    assert props.dtype == t.dtype == n_ext.dtype == torch.float32 and arg.dtype == torch.int32 and props.is_cuda
    assert bool((props[:, 6] == 1).all())
    for i, src in enumerate((0, 1, 2, 3, 4, 4)):
        col = t[:, :, src]
        assert torch.equal(props[:, i], col.max(dim=1).values if i & 1 else col.min(dim=1).values)
        first = (col == props[:, i:i + 1]).int().argmax(dim=1)
        assert torch.equal(arg[:, i].long(), first)
    out = excluded(k["ref"])
    assert int(out.sum()) <= 0.1 * out.numel()
    got, bound = errors(props, t, k["ref"]), bounds(k["base"], k["ref"])
    nerr = normal_error(n_ext, arg, k["ref"])
    print(f"transverse properties n_dirs={n_dirs}: fused", got, "fp32 restatement on CPU", k["base"], "n_ext",
          float(nerr.max()), "baseline", k["nbase"].tolist(), "excluded", int(out.sum()))
    record_parity(f"transverse_props_p{n_dirs}", fused=got, reference_fp32_cpu=k["base"], n_ext=float(nerr.max()))
    for name, v in got.items():
        assert v <= bound[name], (name, v, bound[name])
    assert within(nerr, k["nbase"]), (nerr, k["nbase"])
    unit = n_ext.double().norm(dim=2).cpu()
    assert float((unit - 1).abs().max()) < 1e-6
    along = (n_ext.double() * k["d"].double()[arg[:, :4].long()]).sum(dim=2).abs().cpu()
    assert float(along.max()) < 1e-6


@pytest.mark.parametrize("n_dirs", N_DIRS)
def test_spd_set_gradient_within_4x_and_exactly_symmetric(n_dirs):
    k = case(n_dirs)
    assert k["g"].shape == (17, 6, 6) and k["g"].dtype == torch.float32
    assert torch.equal(k["g"], k["g"].transpose(1, 2))
    err = gradient_error(k["g"], k["gref"])
    print(f"transverse gradient n_dirs={n_dirs}: fused", err.tolist(), "fp32 autograd through the restatement",
          k["gbase"].tolist())
    record_parity(f"transverse_grad_p{n_dirs}", fused=float(err.max()), reference_fp32_cpu=float(k["gbase"].max()))
    assert within(err, k["gbase"]), (err, k["gbase"])
    # with the cotangents of the excluded pairs and of the rounding-decided extremes: finite, symmetric
    gp, gt = cotangents(k["ref"], keep_excluded=True)
    g_all = fused(k["c"], k["d"], gp.float().to(DEV), gt.float().to(DEV))[4]
    assert bool(torch.isfinite(g_all).all()) and torch.equal(g_all, g_all.transpose(1, 2))


@pytest.mark.parametrize("n_dirs", (65, 250))
@pytest.mark.parametrize("n_graphs", [1, 3, 17])
def test_rows_and_gradient_are_bitwise_independent_of_batch_and_position(n_graphs, n_dirs):
    """Every graph alone (n_graphs = 1: each of the 17 in turn; 3: graphs 5 .. 8; 17: the set again)
    against the 17-graph launch, on two runs, and inside a 65-graph batch made by repeating the set."""
    k = case(n_dirs)
    want = (k["props"], k["t"], k["arg"], k["n_ext"], k["g"])
    slices = [slice(b, b + 1) for b in range(17)] if n_graphs == 1 else [slice(5, 8)] if n_graphs == 3 else [slice(0, 17)]
    for sl in slices:
        a = fused(k["c"][sl], k["d"], k["gp"][sl], k["gt"][sl])
        b = fused(k["c"][sl], k["d"], k["gp"][sl], k["gt"][sl])
        for x, y, w in zip(a, b, want):
            assert torch.equal(x, y) and torch.equal(x, w[sl])
    if n_graphs == 17:
        idx = torch.arange(65, device=DEV) % 17
        big = fused(k["c"][idx], k["d"], k["gp"][idx], k["gt"][idx])
        for x, w in zip(big, want):
            assert x.shape[0] == 65 and torch.equal(x, w[idx])


def test_without_directions_everything_is_nan_and_the_gradient_zero():
    c = case(65)["c"]
    props, t, arg, n_ext, g = fused(c, torch.zeros(0, 3, device=DEV), torch.ones(17, 7, device=DEV), None)
    assert t.shape == (17, 0, 5) and bool(torch.isnan(props[:, :6]).all()) and bool((props[:, 6] == 1).all())
    assert bool((arg == -1).all()) and bool(torch.isnan(n_ext).all()) and bool((g == 0).all())


def test_axis_and_tied_directions_against_fp64():
    """The 26 axes, face and body diagonals of the cube (zero and tied components in the frame's axis
    choice), each beside its negative: values and the transverse vector against the restatement."""
    from gnn.transverse import transverse_properties
    c, d = spd_set(), crystal_directions().float()
    ref = reference(c, d)
    b32 = reference(c, d, torch.float32)
    props, t, arg, n_ext = transverse_properties(c.to(DEV), d.to(DEV))
    got, bound = errors(props, t, ref), bounds(errors(b32["props"], b32["t_dir"], ref), ref)
    print("crystal directions: fused", got)
    for name, v in got.items():
        assert v <= bound[name], (name, v, bound[name])
    assert torch.equal(t[:, 0::2], t[:, 1::2])                     # d and -d: bitwise the same row
    assert bool(torch.isfinite(n_ext).all())


def test_first_extreme_takes_the_tie_and_its_gradient():
    from gnn.transverse import transverse_properties
    c, d = tie_case()
    check_tie(transverse_properties, c.to(DEV), d.to(DEV))


def test_a_matrix_that_is_not_positive_definite_stays_in_its_row():
    from gnn.transverse import transverse_properties
    c, keep, good = bad_batch()
    check_bad_batch(transverse_properties, c.to(DEV), keep, good.to(DEV), directions(65).to(DEV),
                    sync=torch.cuda.synchronize)


@pytest.mark.parametrize("n_dirs", (65, 250))
def test_fused_agrees_with_composed_on_the_device(n_dirs, monkeypatch):
    """EELG_TRANSVERSE_FUSED=0 (the composed torch form on the device) against the fused kernels,
    normalised like the errors against fp64, within the same bounds."""
    from gnn import transverse
    k = case(n_dirs)
    monkeypatch.setattr(transverse, "FUSED", False)
    x = k["c"].clone().requires_grad_(True)
    props, t, arg, n_ext = transverse.transverse_properties(x, k["d"])
    g, = torch.autograd.grad([props, t], [x], [k["gp"], k["gt"]])
    monkeypatch.undo()
    assert props.is_cuda and props.shape == (17, 7) and t.shape == (17, n_dirs, 5)
    assert torch.equal(props[:, 6], k["props"][:, 6]) and torch.equal(arg, k["arg"])
    fake = dict(k["ref"], props=k["props"].double().cpu(), t_dir=k["t"].double().cpu())
    diff = errors(props, t, fake)
    gdiff = gradient_error(g, k["g"])
    ndiff = float(torch.minimum((n_ext - k["n_ext"]).norm(dim=2), (n_ext + k["n_ext"]).norm(dim=2))[
        ~excluded(k["ref"]).to(DEV).gather(1, k["arg"][:, :4].long())].max())
    print(f"fused against composed on the device n_dirs={n_dirs}", diff, "gradient", gdiff.tolist(), "n_ext", ndiff)
    record_parity(f"transverse_fused_vs_composed_p{n_dirs}", gradient=float(gdiff.max()), n_ext=ndiff, **diff)
    bound = bounds(k["base"], k["ref"])
    for name, v in diff.items():
        assert v <= bound[name], (name, v, bound[name])
    assert within(gdiff, k["gbase"]) and ndiff <= max(4 * float(k["nbase"].min()), 4 * 2.0 ** -23)


def test_outputs_in_slices_of_sentinel_buffers_and_c_abi_guards():
    from gnn import _lib
    lib = _lib.load()
    k = case(65)
    stream = _lib.stream(k["c"])
    fwd, bwd = lib.eelg_transverse_props, lib.eelg_transverse_props_bwd
    # zero graphs: a no-op, whatever the pointers and the direction count
    assert fwd(None, None, 0, 65, None, None, None, None, None, stream) == 0
    assert bwd(None, None, None, None, None, None, 0, 65, None, stream) == 0
    props = torch.full((21, 7), 7.0, device=DEV)
    t = torch.full((21, 65, 5), 7.0, device=DEV)
    arg = torch.full((21, 6), 7, dtype=torch.int32, device=DEV)
    n_ext = torch.full((21, 12), 7.0, device=DEV)
    s = torch.full((21, 21), 7.0, dtype=torch.float64, device=DEV)
    g = torch.full((21, 36), 7.0, device=DEV)
    P = _lib.ptr
    c, d, gp, gt = P(k["c"]), P(k["d"]), P(k["gp"]), P(k["gt"])
    po, to, ao, no, so, go = P(props[2:]), P(t[2:]), P(arg[2:]), P(n_ext[2:]), P(s[2:]), P(g[2:])
    odd = _lib._P(s[2:].data_ptr() + 4)
    good = (c, d, 17, 65, po, to, ao, no, so)
    for pos, value, word in ((0, None, b"null"), (1, None, b"null"), (4, None, b"null"), (5, None, b"null"),
                             (6, None, b"null"), (7, None, b"null"), (8, None, b"null"), (8, odd, b"aligned"),
                             (2, -1, b"graphs"), (3, -5, b"directions")):
        args = list(good)
        args[pos] = value
        assert fwd(*args, stream) == -2
        assert word in lib.eelg_last_error()
    good = (so, d, po, ao, gp, gt, 17, 65, go)
    for pos, value, word in ((0, None, b"null"), (0, odd, b"aligned"), (1, None, b"null"), (2, None, b"null"),
                             (3, None, b"null"), (4, None, b"null"), (8, None, b"null"), (6, -1, b"graphs"),
                             (7, -1, b"directions")):
        args = list(good)
        args[pos] = value
        assert bwd(*args, stream) == -2
        assert word in lib.eelg_last_error()
    torch.cuda.synchronize()
    for buf in (props, t, arg, n_ext, s, g):
        assert bool((buf == 7).all())
    # the well-formed calls fill rows 2 .. 19 and nothing else
    assert fwd(c, d, 17, 65, po, to, ao, no, so, stream) == 0
    assert bwd(so, d, po, ao, gp, gt, 17, 65, go, stream) == 0
    torch.cuda.synchronize()
    assert torch.equal(props[2:19], k["props"]) and torch.equal(t[2:19], k["t"]) and torch.equal(arg[2:19], k["arg"])
    assert torch.equal(n_ext[2:19].view(17, 4, 3), k["n_ext"]) and torch.equal(g[2:19].view(17, 6, 6), k["g"])
    for buf in (props, t, arg, n_ext, s, g):
        assert bool((buf[:2] == 7).all()) and bool((buf[19:] == 7).all())
    # a NULL t_dir cotangent is a zero one
    assert bwd(so, d, po, ao, gp, None, 17, 65, go, stream) == 0
    want = fused(k["c"], k["d"], k["gp"], torch.zeros_like(k["gt"]))[4]
    assert torch.equal(g[2:19].view(17, 6, 6), want)


def test_validation_and_no_host_synchronisation(monkeypatch):
    from gnn.transverse import transverse_properties
    k = case(65)
    for bad in ((k["c"][0], k["d"]), (k["c"], k["d"][:, :2]), (k["c"], k["d"].cpu()), (k["c"].long(), k["d"]),
                (k["c"], None)):
        with pytest.raises(ValueError):
            transverse_properties(*bad)

    def refuse(*a, **kw):
        raise AssertionError("the transverse properties may not read a device tensor back")
    for name in ("item", "tolist", "cpu"):
        monkeypatch.setattr(torch.Tensor, name, refuse)
    got = fused(k["c"], k["d"], k["gp"], k["gt"])
    monkeypatch.undo()
    for x, want in zip(got, (k["props"], k["t"], k["arg"], k["n_ext"], k["g"])):
        assert torch.equal(x, want)


# ---------------------------------------------------------------------------------------------
def design_case():
    """The end-to-end batch of ``test_gpu_design`` (3 graphs of 10 nodes / 30 edges, the HIP model
    with the fp64 oracle's weights), 16 directions and weights on nu_min, G_min and four t_dir entries."""
    if "design" not in _CASES:
        from test_gpu_design import E2E, end_to_end
        from gnn import TRANSVERSE_COLUMNS
        k = end_to_end()
        bd = k["b"].to(DEV)
        d = directions(16).to(DEV)
        tw = torch.zeros(3, 7, device=DEV)
        tw[:, TRANSVERSE_COLUMNS.index("nu_min")] = 1.0
        tw[:, TRANSVERSE_COLUMNS.index("G_min")] = -0.5             # negative: stiffen the softest shear
        tw[:, TRANSVERSE_COLUMNS.index("spd")] = 3.0                # no effect
        tdw = torch.zeros(3, 16, 5, device=DEV)
        tdw[0, 2, 1], tdw[1, 7, 3], tdw[2, 11, 4], tdw[2, 0, 0] = 0.25, -0.5, 2.0, 0.125
        _CASES["design"] = dict(m=k["m"], bd=bd, d=d, tw=tw, tdw=tdw, w=torch.zeros(3, 12, device=DEV),
                                hyper={key: v for key, v in E2E.items() if key != "r_max"}, r_max=E2E["r_max"])
    return _CASES["design"]


def test_property_sensitivity_with_transverse_weights(monkeypatch):
    """Fused against the composed form's autograd through the same model, per geometry gradient
    relative to its largest entry.  Bound: 4x the deviation of the fp32 CPU restatement's cotangent fed
    through ``stiffness_sensitivity`` (the baseline of ``test_gpu_elastic``), at least 4 fp32 ulps."""
    from gnn import ops, property_sensitivity, stiffness_sensitivity, transverse
    k = design_case()
    m, bd, d, tw, tdw, w = (k[key] for key in ("m", "bd", "d", "tw", "tdw", "w"))
    geom = ("positions", "edge_attr", "shifts")
    monkeypatch.setattr(ops.TIMER, "enabled", True)
    monkeypatch.setattr(ops.TIMER, "records", {})
    out = property_sensitivity(m, bd, w, d, transverse_weights=tw, transverse_dir_weights=tdw)
    launches = {key: len(ops.TIMER.records.get(key, [])) for key in ("transverse_props", "transverse_props_bwd")}
    monkeypatch.undo()
    assert launches == {"transverse_props": 1, "transverse_props_bwd": 1}
    assert set(out) == {"stiffness", "properties", "e_dir", "transverse", "t_dir", "positions", "edge_attr", "shifts"}
    assert out["transverse"].shape == (3, 7) and out["t_dir"].shape == (3, 16, 5) and not out["t_dir"].requires_grad
    assert bool((out["transverse"][:, 6] == 1).all())
    monkeypatch.setattr(transverse, "FUSED", False)
    comp = property_sensitivity(m, bd, w, d, transverse_weights=tw, transverse_dir_weights=tdw)
    monkeypatch.undo()
    x = out["stiffness"].cpu().clone().requires_grad_(True)
    r32 = reference(x, d.cpu(), torch.float32)
    cot, = torch.autograd.grad((tw.cpu() * r32["props"]).sum() + (tdw.cpu() * r32["t_dir"]).sum(), x)
    base_out = stiffness_sensitivity(m, bd, cot.to(DEV))

    def rel(a, r):
        return float((a - r).abs().max() / r.abs().max())
    got = {key: rel(out[key], comp[key]) for key in geom}
    base = {key: rel(base_out[key], comp[key]) for key in geom}
    print("property_sensitivity with transverse weights: fused against composed", got, "baseline", base)
    record_parity("transverse_property_sensitivity", fused=got, baseline=base)
    for key in geom:
        assert got[key] <= max(4 * base[key], 4 * 2.0 ** -23), (key, got[key], base[key])
    # only the weights on the transverse rows count: the same call without them gives other gradients,
    # and both keywords None is today's call
    plain = property_sensitivity(m, bd, w, d)
    assert set(plain) == {"stiffness", "properties", "e_dir", "positions", "edge_attr", "shifts"}
    assert bool((plain["positions"] == 0).all()) and float(out["positions"].abs().max()) > 0
    with pytest.raises(ValueError):
        property_sensitivity(m, bd, w, None, transverse_weights=tw)
    with pytest.raises(ValueError):
        property_sensitivity(m, bd, w, d, transverse_weights=tw[:, :6])


def test_optimize_design_with_transverse_weights(monkeypatch):
    from gnn import design, optimize_design, property_sensitivity
    from gnn.design import design_layout, design_step, strut_volume
    k = design_case()
    m, bd, d, tw, tdw, hyper = (k[key] for key in ("m", "bd", "d", "tw", "tdw", "hyper"))
    res = optimize_design(m, bd, directions=d, transverse_weights=tw, transverse_dir_weights=tdw, steps=3, **hyper)
    assert res.objective.shape == (4, 3) and res.volume.shape == (4, 3) and res.flags.shape == (3, 3)
    assert bool(torch.isfinite(res.objective).all()) and bool(torch.isfinite(res.volume).all()) and not bool(res.flags.any())
    assert bool(torch.isfinite(res.batch.positions).all()) and bool(torch.isfinite(res.batch.edge_attr).all())
    sens = property_sensitivity(m, bd, k["w"], d, transverse_weights=tw, transverse_dir_weights=tdw)
    want = (tw * sens["transverse"]).sum(dim=1) + (tdw * sens["t_dir"]).sum(dim=(1, 2))
    assert torch.allclose(res.objective[0], want, rtol=1e-6, atol=0)
    # the first step is bitwise one design_step by hand from property_sensitivity's gradient
    lay = design_layout(bd)
    one = optimize_design(m, bd, directions=d, transverse_weights=tw, transverse_dir_weights=tdw, steps=1, **hyper)
    pos, r = bd.positions.clone(), bd.edge_attr.reshape(-1).clone()
    out = design_step(lay, sens["positions"], sens["edge_attr"].reshape(-1), pos, r, pos, torch.zeros_like(pos),
                      torch.zeros_like(r), bd.shifts, strut_volume(bd, lay), **dict(hyper, r_max=k["r_max"]))
    assert torch.equal(one.batch.positions, out[0]) and torch.equal(one.batch.edge_attr.reshape(-1), out[1])
    assert torch.equal(one.volume[1], out[4])
    # nothing inside the loop reads the device
    real_layout = design.design_layout

    def refuse(*a, **kw):
        raise AssertionError("the design loop may not read a device tensor back")

    def layout_then_refuse(batch_):
        lay_ = real_layout(batch_)
        for name in ("item", "tolist", "cpu"):
            monkeypatch.setattr(torch.Tensor, name, refuse)
        return lay_
    monkeypatch.setattr(design, "design_layout", layout_then_refuse)
    again = design.optimize_design(m, bd, directions=d, transverse_weights=tw, transverse_dir_weights=tdw, steps=3,
                                   **hyper)
    monkeypatch.undo()
    assert torch.equal(again.objective, res.objective) and torch.equal(again.batch.positions, res.batch.positions)
    with pytest.raises(ValueError):
        optimize_design(m, bd, target=torch.zeros(3, 6, 6, device=DEV), transverse_weights=tw, directions=d, steps=1,
                        **hyper)
    with pytest.raises(ValueError):
        optimize_design(m, bd, transverse_weights=tw, steps=1, **hyper)
