"""``eelg_elastic_props`` / ``eelg_elastic_props_bwd`` (``csrc/eelg_elastic.hip``) and
``gnn.property_sensitivity`` on the device.

Accuracy is measured against the rank-4 fp64 restatement (``helpers_elastic.reference``) over the
17 matrices of ``spd_set()`` (condition numbers 4 .. 1e4): per column the largest error over the
set, relative to the graph's own fp64 value (``A_U``: to ``A_U + 6``; ``nu_H``: absolute); the
gradient per matrix relative to that matrix's largest fp64 gradient entry.  Bound: 4x the same
figure of the restatement run in fp32 on the CPU on the same inputs (none of the kernel's code; the
margin for a second fp32 summation order, as ``test_gpu_metrics``).

Measured on MI355X, ratio fused / baseline, the same for every P in {1, 63, 64, 65, 250} to the
digits shown unless noted: K_V 0.68 (4.4e-8 / 6.4e-8), G_V 0.22, K_R 0.004 (4.9e-8 / 1.3e-5),
G_R 0.003, K_H 0.19, G_H 0.29, E_H 0.28, nu_H 0.31, A_U 0.003, E_min 0.003 .. 0.004, E_max 0.004 ..
0.008, E_dir 0.003 .. 0.004 (5.9e-8 / 1.4e-5 .. 2.3e-5).  Gradient: 1.5e-7 / 3.2e-4 (P = 1), 4.7e-6 /
1.9e-4 (63), 3.4e-6 / 3.5e-4 (64), 1.5e-6 / 2.8e-4 (65), 6.2e-6 / 8.8e-4 (250), 1.8e-6 / 3.6e-4 (no
directions): ratio <= 0.024.  Fused against composed on the device: rows bitwise equal (A_U to
1.5e-16 of A_U + 6), gradient 1.2e-6 (P = 65) and 4.3e-6 (P = 250).  ``property_sensitivity``
against the fp64 oracle (kappa_2 of the three stiffnesses 33 .. 58): positions 1.7e-6, radii 1.6e-6,
shifts 3.1e-6; baseline (fp32 CPU restatement's cotangent through ``stiffness_sensitivity``)
2.0e-6 / 1.9e-6 / 3.5e-6: ratio 0.84 .. 0.89.

Everything else is bitwise: a graph's row and gradient do not depend on the batch around it, on
its position or on the run; a matrix that is not positive definite stays in its row.
"""
import pytest
import torch

from helpers import batch, batch_to, copy_params, params, record_parity
from helpers_elastic import (bad_batch, check_bad_batch, check_tie, cotangents, errors, gradient, gradient_error,
                             reference, spd_set, tie_case)
from helpers_metrics import directions

pytestmark = pytest.mark.gpu
DEV = "cuda"
N_DIRS = (1, 63, 64, 65, 250)        # below, at and above one direction per lane; the metrics' 250
_CASES = {}


def case(n_dirs: int):
    """Inputs, fp64 truth, CPU fp32 baseline errors, cotangents and the fused rows and gradient of
    the SPD set: computed once per direction count and shared, never modified."""
    if n_dirs not in _CASES:
        from gnn.elastic import elastic_properties
        c = spd_set()
        d = directions(n_dirs) if n_dirs else None
        d64 = d.double() if n_dirs else None
        rp, re_ = reference(c.double(), d64)
        base = errors(*reference(c, d), rp, re_)
        gp, ge = cotangents(rp, re_)
        gref = gradient(reference, c.double(), d64, gp, ge)
        gbase = gradient_error(gradient(reference, c, d, gp, ge), gref)
        cd, dd = c.to(DEV), d.to(DEV) if n_dirs else None
        x = cd.clone().requires_grad_(True)
        props, e = elastic_properties(x, dd)
        outs, gs = [props], [gp.float().to(DEV)]
        if n_dirs:
            outs.append(e)
            gs.append(ge.float().to(DEV))
        g, = torch.autograd.grad(outs, [x], gs)
        _CASES[n_dirs] = dict(c=cd, d=dd, ref=(rp, re_), base=base, gp=gs[0], ge=gs[1] if n_dirs else None, gref=gref,
                              gbase=gbase, props=props.detach(), e=e.detach(), g=g)
    return _CASES[n_dirs]


def fused(c, d, gp, ge):
    from gnn.elastic import elastic_properties
    x = c.clone().requires_grad_(True)
    props, e = elastic_properties(x, d)
    outs, gs = ([props, e], [gp, ge]) if ge is not None else ([props], [gp])
    g, = torch.autograd.grad(outs, [x], gs)
    return props.detach(), e.detach(), g


@pytest.mark.parametrize("n_dirs", N_DIRS)
def test_spd_set_forward_within_4x_of_the_fp32_restatement(n_dirs):
    k = case(n_dirs)
    assert k["props"].shape == (17, 12) and k["e"].shape == (17, n_dirs)
    assert k["props"].dtype == k["e"].dtype == torch.float32 and k["props"].is_cuda
    assert bool((k["props"][:, 11] == 1).all())
    assert torch.equal(k["props"][:, 9], k["e"].min(dim=1).values)
    assert torch.equal(k["props"][:, 10], k["e"].max(dim=1).values)
    got = errors(k["props"], k["e"], *k["ref"])
    print(f"elastic properties n_dirs={n_dirs}: fused", got, "fp32 restatement on CPU", k["base"])
    record_parity(f"elastic_props_p{n_dirs}", fused=got, reference_fp32_cpu=k["base"])
    for name, v in got.items():
        assert v <= 4 * k["base"][name], (name, v, k["base"][name])


@pytest.mark.parametrize("n_dirs", N_DIRS)
def test_spd_set_gradient_within_4x_and_exactly_symmetric(n_dirs):
    k = case(n_dirs)
    assert k["g"].shape == (17, 6, 6) and k["g"].dtype == torch.float32
    assert torch.equal(k["g"], k["g"].transpose(1, 2))
    err = gradient_error(k["g"], k["gref"])
    print(f"elastic gradient n_dirs={n_dirs}: fused {err:.2e}, fp32 autograd through the restatement {k['gbase']:.2e}")
    record_parity(f"elastic_grad_p{n_dirs}", fused=err, reference_fp32_cpu=k["gbase"])
    assert err <= 4 * k["gbase"], (err, k["gbase"])


@pytest.mark.parametrize("n_dirs", (65, 250))
@pytest.mark.parametrize("n_graphs", [1, 3])
def test_row_and_gradient_are_bitwise_independent_of_batch_and_position(n_graphs, n_dirs):
    """Graphs 5 .. 5 + n_graphs of the set launched on their own (other positions, another batch
    size; n_graphs = 1: alone): bitwise the rows and gradients of the 17-graph launch, on two runs;
    and the same inside a 65-graph batch made by repeating the set."""
    k = case(n_dirs)
    sl = slice(5, 5 + n_graphs)
    a = fused(k["c"][sl], k["d"], k["gp"][sl], k["ge"][sl])
    b = fused(k["c"][sl], k["d"], k["gp"][sl], k["ge"][sl])
    for x, y, want in zip(a, b, (k["props"][sl], k["e"][sl], k["g"][sl])):
        assert torch.equal(x, y) and torch.equal(x, want)
    idx = torch.arange(65, device=DEV) % 17
    big = fused(k["c"][idx], k["d"], k["gp"][idx], k["ge"][idx])
    for x, want in zip(big, (k["props"][idx], k["e"][idx], k["g"][idx])):
        assert x.shape[0] == 65 and torch.equal(x, want)


def test_without_directions_the_gradient_flows_through_the_scalar_columns():
    from gnn.elastic import elastic_properties
    k0, k = case(0), case(65)
    assert k0["e"].shape == (17, 0) and bool(torch.isnan(k0["props"][:, 9:11]).all())
    assert torch.equal(k0["props"][:, :9], k["props"][:, :9]) and torch.equal(k0["props"][:, 11], k["props"][:, 11])
    assert torch.equal(k0["g"], k0["g"].transpose(1, 2)) and bool(torch.isfinite(k0["g"]).all())
    err = gradient_error(k0["g"], k0["gref"])
    record_parity("elastic_grad_p0", fused=err, reference_fp32_cpu=k0["gbase"])
    assert err <= 4 * k0["gbase"], (err, k0["gbase"])
    # an empty [0, 3] direction tensor is the same call
    x = k0["c"].clone().requires_grad_(True)
    props, e = elastic_properties(x, torch.zeros(0, 3, device=DEV))
    g, = torch.autograd.grad(props, x, k0["gp"])
    assert e.shape == (17, 0) and torch.equal(g, k0["g"])
    assert torch.equal(props[:, :9], k0["props"][:, :9])


def test_first_extreme_takes_the_tie_and_its_gradient():
    from gnn.elastic import elastic_properties
    c, axes = tie_case()
    x = c.to(DEV).requires_grad_(True)
    props, e = elastic_properties(x, axes.to(DEV))
    g_max, = torch.autograd.grad(props[0, 10], x)
    check_tie(props.cpu(), e.cpu(), g_max.cpu())


def test_a_matrix_that_is_not_positive_definite_stays_in_its_row():
    from gnn.elastic import elastic_properties
    c, keep, good = bad_batch()
    check_bad_batch(elastic_properties, c.to(DEV), keep, good.to(DEV), directions(65).to(DEV),
                    sync=torch.cuda.synchronize)


@pytest.mark.parametrize("n_dirs", (65, 250))
def test_fused_agrees_with_composed_on_the_device(n_dirs, monkeypatch):
    """EELG_ELASTIC_FUSED=0 (the composed torch form on the device) against the fused kernels,
    normalised like the errors against fp64, within the same bounds."""
    from gnn import elastic
    k = case(n_dirs)
    monkeypatch.setattr(elastic, "FUSED", False)
    x = k["c"].clone().requires_grad_(True)
    props, e = elastic.elastic_properties(x, k["d"])
    g, = torch.autograd.grad([props, e], [x], [k["gp"], k["ge"]])
    monkeypatch.undo()
    assert props.is_cuda and props.shape == (17, 12) and e.shape == (17, n_dirs)
    assert torch.equal(props[:, 11], k["props"][:, 11])
    rp, re_ = k["ref"]
    diff = {}
    for i, name in enumerate(("K_V", "G_V", "K_R", "G_R", "K_H", "G_H", "E_H", "nu_H", "A_U", "E_min", "E_max")):
        scale = torch.ones(17, dtype=torch.float64) if name == "nu_H" else \
            (rp[:, i] + 6 if name == "A_U" else rp[:, i]).abs()
        diff[name] = float(((props.detach()[:, i] - k["props"][:, i]).double().cpu().abs() / scale).max())
    diff["E_dir"] = float(((e.detach() - k["e"]).double().cpu().abs() / re_.abs()).max())
    gdiff = float(((g - k["g"]).double().cpu().abs().amax(dim=(1, 2)) / k["gref"].abs().amax(dim=(1, 2))).max())
    print(f"fused against composed on the device n_dirs={n_dirs}", diff, f"gradient {gdiff:.2e}")
    record_parity(f"elastic_fused_vs_composed_p{n_dirs}", gradient=gdiff, **diff)
    for name, v in diff.items():
        assert v <= 4 * k["base"][name], (name, v, k["base"][name])
    assert gdiff <= 4 * k["gbase"], (gdiff, k["gbase"])


def test_outputs_in_slices_of_sentinel_buffers_and_c_abi_guards():
    from gnn import _lib
    lib = _lib.load()
    k = case(65)
    stream = _lib.stream(k["c"])
    fwd, bwd = lib.eelg_elastic_props, lib.eelg_elastic_props_bwd
    # zero graphs: a no-op, whatever the pointers and the direction count
    assert fwd(None, None, 0, 65, None, None, None, stream) == 0
    assert bwd(None, None, None, None, None, None, 0, 65, None, stream) == 0
    props = torch.full((17 + 4, 12), 7.0, device=DEV)
    e = torch.full((17 + 4, 65), 7.0, device=DEV)
    s = torch.full((17 + 4, 36), 7.0, device=DEV)
    g = torch.full((17 + 4, 36), 7.0, device=DEV)
    P = _lib.ptr
    c, d = P(k["c"]), P(k["d"])
    po, eo, so, go = P(props[2:]), P(e[2:]), P(s[2:]), P(g[2:])
    gp, ge = P(k["gp"]), P(k["ge"])
    for args, word in (((None, d, 17, 65, po, eo, so), b"null"), ((c, None, 17, 65, po, eo, so), b"null"),
                       ((c, d, 17, 65, None, eo, so), b"null"), ((c, d, 17, 65, po, None, so), b"null"),
                       ((c, d, 17, 65, po, eo, None), b"null"), ((c, d, -1, 65, po, eo, so), b"graphs"),
                       ((c, d, 17, -5, po, eo, so), b"directions")):
        assert fwd(*args, stream) == -2
        assert word in lib.eelg_last_error()
    for args, word in (((None, d, eo, po, gp, ge, 17, 65, go), b"null"), ((so, None, eo, po, gp, ge, 17, 65, go), b"null"),
                       ((so, d, None, po, gp, ge, 17, 65, go), b"null"), ((so, d, eo, None, gp, ge, 17, 65, go), b"null"),
                       ((so, d, eo, po, None, ge, 17, 65, go), b"null"), ((so, d, eo, po, gp, ge, 17, 65, None), b"null"),
                       ((so, d, eo, po, gp, ge, -1, 65, go), b"graphs"), ((so, d, eo, po, gp, ge, 17, -1, go), b"directions")):
        assert bwd(*args, stream) == -2
        assert word in lib.eelg_last_error()
    torch.cuda.synchronize()
    for buf in (props, e, s, g):
        assert bool((buf == 7).all())
    # the well-formed calls fill rows 2 .. 19 and nothing else
    assert fwd(c, d, 17, 65, po, eo, so, stream) == 0
    assert bwd(so, d, eo, po, gp, ge, 17, 65, go, stream) == 0
    torch.cuda.synchronize()
    assert torch.equal(props[2:19], k["props"]) and torch.equal(e[2:19], k["e"])
    assert torch.equal(g[2:19].view(17, 6, 6), k["g"])
    assert torch.equal(s[2:19].view(17, 6, 6), s[2:19].view(17, 6, 6).transpose(1, 2))
    eye = (s[2:19].view(17, 6, 6).double() @ k["c"].double()).cpu()
    assert float((eye - torch.eye(6, dtype=torch.float64)).abs().max()) < 1e-2      # kappa 1e4 x fp32 storage
    for buf in (props, e, s, g):
        assert bool((buf[:2] == 7).all()) and bool((buf[19:] == 7).all())
    # a NULL e_dir cotangent is a zero one
    assert bwd(so, d, eo, po, gp, None, 17, 65, go, stream) == 0
    _, _, want = fused(k["c"], k["d"], k["gp"], torch.zeros_like(k["ge"]))
    assert torch.equal(g[2:19].view(17, 6, 6), want)


def test_validation_and_no_host_synchronisation(monkeypatch):
    from gnn.elastic import elastic_properties
    k = case(65)
    for bad in ((k["c"][0], k["d"]), (k["c"], k["d"][:, :2]), (k["c"], k["d"].cpu()), (k["c"].long(), k["d"])):
        with pytest.raises(ValueError):
            elastic_properties(*bad)

    def refuse(*a, **kw):
        raise AssertionError("the elastic properties may not read a device tensor back")
    for name in ("item", "tolist", "cpu"):
        monkeypatch.setattr(torch.Tensor, name, refuse)
    got = fused(k["c"], k["d"], k["gp"], k["ge"])
    monkeypatch.undo()
    for x, want in zip(got, (k["props"], k["e"], k["g"])):
        assert torch.equal(x, want)


# ---------------------------------------------------------------------------------------------
def test_property_sensitivity_against_the_fp64_oracle(monkeypatch):
    """``property_sensitivity`` end to end: weights on E_H, A_U, E_min and eight e_dir entries.
    Truth: the fp64 oracle model, the rank-4 restatement and autograd to positions, radii and
    shifts.  Baseline: the CPU fp32 restatement's autograd applied to the HIP model's stiffness,
    its cotangent fed through ``stiffness_sensitivity``.  Bound: 4x the baseline, per gradient,
    relative to the gradient's largest fp64 entry."""
    import oracle.model as omodel
    from gnn import EnergyEquivGNN, ops, property_sensitivity, stiffness_sensitivity
    geom = ("positions", "edge_attr", "shifts")
    b, rmax = batch(3, 10, 30, seed=3)
    p = params(2, lmax=2, correlation=2, max_edge_radius=rmax)
    torch.manual_seed(2)
    saved = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        o = omodel.EnergyEquivGNN(p).double()
    finally:
        torch.set_default_dtype(saved)
    m = EnergyEquivGNN(p).to(DEV)
    copy_params(o, m)
    bo = batch_to(b, "cpu", torch.float64)
    for key in geom:
        setattr(bo, key, getattr(bo, key).detach().clone().requires_grad_(True))
    co = o(bo)["stiffness"]
    kappa = torch.linalg.cond(co.detach())
    assert float(kappa.max()) <= 1e3, kappa          # from the oracle alone: a well-conditioned case
    d = directions(16)
    rp, re_ = reference(co, d.double())
    gen = torch.Generator().manual_seed(13)
    w = torch.zeros(3, 12, dtype=torch.float64)
    for col in (6, 8, 9):                            # E_H, A_U, E_min
        scale = (rp[:, col].detach() + 6 if col == 8 else rp[:, col].detach()).abs()
        w[:, col] = torch.randn(3, generator=gen, dtype=torch.float64) / scale
    dw = torch.zeros(3, 16, dtype=torch.float64)
    rows, cols = torch.tensor([0, 0, 0, 1, 1, 2, 2, 2]), torch.tensor([0, 5, 15, 3, 9, 1, 7, 12])
    dw[rows, cols] = torch.randn(8, generator=gen, dtype=torch.float64) / re_.detach()[rows, cols].abs()
    ref = torch.autograd.grad((w * rp).sum() + (dw * re_).sum(), [getattr(bo, key) for key in geom])

    bd = b.to(DEV)
    before = {key: getattr(bd, key) for key in geom}
    monkeypatch.setattr(ops.TIMER, "enabled", True)
    monkeypatch.setattr(ops.TIMER, "records", {})
    out = property_sensitivity(m, bd, w.float().to(DEV), d.to(DEV), dw.float().to(DEV))
    launches = {key: len(ops.TIMER.records.get(key, [])) for key in ("elastic_props", "elastic_props_bwd")}
    monkeypatch.undo()
    assert launches == {"elastic_props": 1, "elastic_props_bwd": 1}
    assert set(out) == {"stiffness", "properties", "e_dir", "positions", "edge_attr", "shifts"}
    assert out["properties"].shape == (3, 12) and out["e_dir"].shape == (3, 16)
    assert not out["properties"].requires_grad and bool((out["properties"][:, 11] == 1).all())
    assert all(q.grad is None for q in m.parameters()) and all(q.requires_grad for q in m.parameters())
    for key in geom:                                  # the batch is as it was
        assert getattr(bd, key) is before[key] and not before[key].requires_grad
        assert out[key].shape == getattr(bd, key).shape

    # baseline: the same model gradient path, the properties' cotangent from fp32 CPU autograd
    x = out["stiffness"].cpu().clone().requires_grad_(True)
    bp, be = reference(x, d)
    cot, = torch.autograd.grad((w.float() * bp).sum() + (dw.float() * be).sum(), x)
    base_out = stiffness_sensitivity(m, bd, cot.to(DEV))
    assert torch.equal(base_out["stiffness"], out["stiffness"])

    def rel(a, r):
        return float((a.detach().double().cpu() - r).abs().max() / r.abs().max())
    got = {key: rel(out[key], r) for key, r in zip(geom, ref)}
    base = {key: rel(base_out[key], r) for key, r in zip(geom, ref)}
    perr = errors(out["properties"], out["e_dir"], rp, re_)
    print(f"property_sensitivity: kappa {kappa.tolist()} fused {got} baseline {base} properties {perr}")
    record_parity("property_sensitivity", fused=got, baseline=base, kappa=float(kappa.max()))
    for key in geom:
        assert got[key] <= 4 * base[key], (key, got[key], base[key])
    again = property_sensitivity(m, bd, w.float().to(DEV), d.to(DEV), dw.float().to(DEV))
    for key in out:
        assert torch.equal(out[key], again[key]), key
    with pytest.raises(ValueError):
        property_sensitivity(m, bd, w[:, :11].float().to(DEV), d.to(DEV))
    with pytest.raises(ValueError):
        property_sensitivity(m, bd, w.float().to(DEV), None, dw.float().to(DEV))
