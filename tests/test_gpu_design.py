"""``eelg_strut_volume`` / ``eelg_design_step`` (``csrc/eelg_design.hip``) and ``gnn.optimize_design``
on the device.

Truth: the fp64 restatement of ``helpers_design`` (per-graph loops; the end-to-end case adds the fp64
oracle model and autograd).  The batch is the four graphs of ``helpers_design.design_graphs`` (2, 70,
257 and 31 edges; the last two with edges that have no unique partner), and each of them alone.
Error of an output column: the largest absolute error over the batch relative to the column's
largest fp64 value.  Bound: 4x the same figure of ``design_step_composed`` run in fp32 on the CPU on
the same inputs, at least 4 fp32 ulps of that value -- the project's margin for a second fp32
evaluation order (``test_gpu_metrics``, ``test_gpu_elastic``).

Measured on MI355X, fused / fp32 composed form on the CPU (ratio), four-graph batch: pos 4.7e-8 / 4.7e-8,
m_pos 4.9e-8 / 4.9e-8, m_r 3.3e-8 / 3.3e-8 (1.0: the same roundings, bitwise the same values), r 9.9e-8 /
2.1e-7 (0.48), vol 1.4e-7 / 6.4e-7 (0.22); ``eelg_strut_volume`` 6.7e-9 / 1.5e-7.  Each graph alone: r
5.8e-8 / 5.3e-8 (1.09, the 2-edge graph), 9.2e-8 / 9.2e-8, 1.0e-7 / 2.1e-7, 1.0e-7 / 1.1e-7; vol 7.9e-8 /
2.4e-7, 7.2e-8 / 7.2e-8, 1.4e-7 / 6.4e-7, 1.1e-7 / 1.1e-7; the other columns ratio 1.0.  Fused against
composed on the device: pos, m_pos, m_r bitwise equal, r 1.8e-8 (1.9e-7 with all clamps binding: the
rescale's one-ulp volume difference), vol 7.3e-8.  ``optimize_design`` over 5 steps against the fp64
oracle loop (kappa_2 <= 133, J falls 21x / 16x / 7x): objective 3.7e-6, volume 1.3e-7, r 3.4e-7, pos
1.5e-7; baseline (``stiffness_sensitivity`` + the fp32 composed step on the CPU) 7.3e-6 / 3.3e-7 /
7.4e-7 / 1.5e-7.

Everything else is bitwise: a graph's outputs do not depend on the batch around it, on its position
or on the run, and the two directions of a strut leave with equal radii.
"""
import copy
import ctypes

import numpy as np
import pytest
import torch

from helpers import batch, copy_params, params, record_parity
from helpers_design import (COLUMNS, HYPER, arrays, as_dict, bounds, column_errors, design_batch, oracle_design_loop,
                            partners, ref_of, ref_volume, step_inputs)

pytestmark = pytest.mark.gpu
DEV = "cuda"
STEP_KEYS = ("g_pos", "g_r", "pos", "r", "pos0", "m_pos", "m_r", "shifts", "v0")
SUBSETS = ((0, 1, 2, 3), (0,), (1,), (2,), (3,))
_CASES = {}


def graph_inputs(which):
    """The fp32 step inputs of the graphs ``which`` (in that order), cut out of the four-graph
    batch's inputs: a graph has the same inputs in whatever batch it stands."""
    if "all" not in _CASES:
        b = design_batch()
        _CASES["all"] = (step_inputs(b), arrays(b))
    inp, a = _CASES["all"]
    out = {}
    for k, v in inp.items():
        ptr = a["node_ptr"] if v.shape[0] == 96 else a["edge_ptr"] if v.shape[0] == 360 else np.arange(5)
        out[k] = torch.cat([v[ptr[g]:ptr[g + 1]] for g in which])
    return out


def case(which=SUBSETS[0]):
    """Batch, layouts (CPU and device), inputs, fp64 truth, the fp32 CPU composed form's errors and the
    fused step's outputs for the graphs ``which``: computed once, shared, never modified."""
    if which not in _CASES:
        from gnn.design import design_layout, design_step, design_step_composed, strut_volume, strut_volume_composed
        b = design_batch(which)
        inp = graph_inputs(which)
        ref = ref_of(b, inp)
        base = column_errors(as_dict(design_step_composed(design_layout(b), *(inp[k] for k in STEP_KEYS), **HYPER)), ref)
        bd = b.to(DEV)
        lay = design_layout(bd)
        dinp = {k: v.to(DEV) for k, v in inp.items()}
        out = as_dict(design_step(lay, *(dinp[k] for k in STEP_KEYS), **HYPER))
        vref = ref_volume(arrays(b))
        vbase = float(np.abs(strut_volume_composed(b).double().numpy() - vref).max() / vref.max())
        _CASES[which] = dict(b=b, bd=bd, lay=lay, inp=inp, dinp=dinp, ref=ref, base=base, out=out, vref=vref,
                             vbase=vbase, vol=strut_volume(bd, lay))
    return _CASES[which]


def fused(k, **hyper):
    from gnn.design import design_step
    h = dict(HYPER)
    h.update(hyper)
    return as_dict(design_step(k["lay"], *(k["dinp"][key] for key in STEP_KEYS), **h))


@pytest.mark.parametrize("which", SUBSETS)
def test_step_and_volume_within_4x_of_the_fp32_composed_form(which):
    k = case(which)
    out = k["out"]
    assert all(out[c].is_cuda and out[c].dtype == torch.float32 for c in COLUMNS) and out["flag"].dtype == torch.int32
    assert out["flag"].tolist() == [0] * len(which)
    for key in ("pos", "r", "m_pos", "m_r"):                     # the functional form leaves its inputs alone
        assert torch.equal(k["dinp"][key].cpu(), k["inp"][key])
    err, lim = column_errors(out, k["ref"]), bounds(k["base"], k["ref"])
    verr = float(np.abs(k["vol"].double().cpu().numpy() - k["vref"]).max() / k["vref"].max())
    vlim = max(4 * k["vbase"], 4 * float(np.spacing(np.float32(k["vref"].max()))) / float(k["vref"].max()))
    print(f"design step {which}: fused", err, "fp32 composed on CPU", k["base"], f"strut volume {verr:.2e} / {k['vbase']:.2e}")
    record_parity("design_step_" + "".join(map(str, which)), fused=err, composed_fp32_cpu=k["base"],
                  ratio={c: err[c] / k["base"][c] if k["base"][c] else None for c in COLUMNS},
                  strut_volume=verr, strut_volume_composed_fp32_cpu=k["vbase"])
    for c in COLUMNS:
        assert err[c] <= lim[c], (c, err[c], lim[c])
    assert verr <= vlim, (verr, vlim)
    # all three clamps binding, and no rescale
    for hyper in ({"r_min": 0.0146484375, "r_max": 0.0400390625, "move_limit": 2.0 ** -8}, {"keep_volume": False}):
        from gnn.design import design_layout, design_step_composed
        h = dict(HYPER)
        h.update(hyper)
        ref = ref_of(k["b"], k["inp"], **hyper)
        cpu = as_dict(design_step_composed(design_layout(k["b"]), *(k["inp"][key] for key in STEP_KEYS), **h))
        got = fused(k, **hyper)
        err, lim = column_errors(got, ref), bounds(column_errors(cpu, ref), ref)
        for c in COLUMNS:
            assert err[c] <= lim[c], (hyper, c, err[c], lim[c])
        if "r_min" in hyper and len(which) > 1:
            lo, hi = k["dinp"]["pos0"] - 2.0 ** -8, k["dinp"]["pos0"] + 2.0 ** -8
            assert float(got["r"].min()) == hyper["r_min"] and float(got["r"].max()) == hyper["r_max"]
            assert bool(((got["pos"] >= lo) & (got["pos"] <= hi)).all())
            assert bool((got["pos"] == lo).any()) and bool((got["pos"] == hi).any())


def test_graphs_are_bitwise_independent_of_batch_position_and_run():
    full = case()
    a = arrays(full["b"])
    again = fused(full)
    for c in COLUMNS + ("flag",):
        assert torch.equal(again[c], full["out"][c]), c
    p = torch.from_numpy(a["partner"]).to(DEV)
    assert torch.equal(full["out"]["r"], full["out"]["r"][p]) and torch.equal(full["out"]["m_r"], full["out"]["m_r"][p])
    assert int((p != torch.arange(360, device=DEV)).sum()) == 356

    def rows(out, col, ptrs, g):
        ptr = ptrs["node_ptr"] if col in ("pos", "m_pos") else ptrs["edge_ptr"] if col in ("r", "m_r") else np.arange(9)
        return out[col][ptr[g]:ptr[g + 1]]
    for which in ((0,), (1,), (2,), (3,), (3, 2, 1, 0), (2, 0, 2, 3, 1)):
        k = case(which)
        aw = arrays(k["b"])
        for slot, g in enumerate(which):
            for c in COLUMNS:
                assert torch.equal(rows(k["out"], c, aw, slot), rows(full["out"], c, a, g)), (which, g, c)
            assert float(k["vol"][slot]) == float(full["vol"][g])


def test_a_graph_with_a_gradient_that_is_not_finite_is_left_alone():
    k = case()
    a = arrays(k["b"])
    for where, idx, value in (("g_r", a["edge_ptr"][2] + 256, float("nan")), ("g_pos", a["node_ptr"][2] * 3 + 4, float("inf")),
                              ("g_r", a["edge_ptr"][2] + 1, float("-inf"))):
        bad = dict(k, dinp=dict(k["dinp"], **{where: k["dinp"][where].clone()}))
        bad["dinp"][where].view(-1)[idx] = value
        out = fused(bad)
        assert out["flag"].tolist() == [0, 0, 1, 0]
        e0, e1, n0, n1 = a["edge_ptr"][2], a["edge_ptr"][3], a["node_ptr"][2], a["node_ptr"][3]
        for col, lo, hi in (("pos", n0, n1), ("m_pos", n0, n1), ("r", e0, e1), ("m_r", e0, e1)):
            assert torch.equal(out[col][lo:hi], k["dinp"][col][lo:hi]), col
            keep = torch.ones(out[col].shape[0], dtype=torch.bool, device=DEV)
            keep[lo:hi] = False
            assert torch.equal(out[col][keep], k["out"][col][keep]), col
        assert float(out["vol"][2]) == float(k["vol"][2])            # its current volume, as strut_volume gives it
        assert torch.equal(out["vol"][[0, 1, 3]], k["out"]["vol"][[0, 1, 3]])


def test_zero_gradient_and_the_current_volume_move_nothing():
    k = case()
    still = dict(k, dinp=dict(k["dinp"], g_pos=torch.zeros(96, 3, device=DEV), g_r=torch.zeros(360, device=DEV), v0=k["vol"]))
    out = fused(still)
    for col in ("pos", "r", "m_pos", "m_r"):
        assert torch.equal(out[col], k["dinp"][col]), col
    assert torch.equal(out["vol"], k["vol"]) and out["flag"].tolist() == [0, 0, 0, 0]


def test_outputs_in_slices_of_sentinel_buffers_and_c_abi_guards():
    from gnn import _lib
    lib = _lib.load()
    k = case()
    lay, d = k["lay"], k["dinp"]
    stream = _lib.stream(d["pos"])
    P = _lib.ptr
    hn, he = ctypes.addressof(lay.host_node_ptr), ctypes.addressof(lay.host_edge_ptr)
    bufs = {c: torch.full((d[c].numel() + 10,), 7.0, device=DEV) for c in ("pos", "r", "m_pos", "m_r")}
    bufs["vol"] = torch.full((4 + 10,), 7.0, device=DEV)
    bufs["vol0"] = torch.full((4 + 10,), 7.0, device=DEV)
    flag = torch.full((4 + 10,), 7, dtype=torch.int32, device=DEV)

    def fill():
        for c in ("pos", "r", "m_pos", "m_r"):
            bufs[c][5:-5] = d[c].reshape(-1)
    fill()
    geo = [P(bufs[c][5:]) for c in ("pos", "r", "m_pos", "m_r")]
    hyper = [HYPER[c] for c in ("step_r", "step_pos", "beta", "r_min", "r_max", "move_limit")] + [1]

    def step(**kw):
        a = dict(g_pos=P(d["g_pos"]), g_r=P(d["g_r"]), pos=geo[0], r=geo[1], pos0=P(d["pos0"]), m_pos=geo[2], m_r=geo[3],
                 partner=P(lay.partner), node_ptr=P(lay.node_ptr), edge_ptr=P(lay.edge_ptr), hn=hn, he=he,
                 shifts=P(d["shifts"]), send=P(lay.send), recv=P(lay.recv), v0=P(d["v0"]), nb=4, n=96, e=360,
                 hyper=hyper, vol=P(bufs["vol"][5:]), flag=P(flag[5:]))
        a.update(kw)
        return lib.eelg_design_step(a["g_pos"], a["g_r"], a["pos"], a["r"], a["pos0"], a["m_pos"], a["m_r"], a["partner"],
                                    a["node_ptr"], a["edge_ptr"], a["hn"], a["he"], a["shifts"], a["send"], a["recv"],
                                    a["v0"], a["nb"], a["n"], a["e"], *a["hyper"], a["vol"], a["flag"], stream)

    def volume(**kw):
        a = dict(pos=P(d["pos"]), r=P(d["r"]), shifts=P(d["shifts"]), send=P(lay.send), recv=P(lay.recv),
                 node_ptr=P(lay.node_ptr), edge_ptr=P(lay.edge_ptr), hn=hn, he=he, nb=4, n=96, e=360, vol=P(bufs["vol0"][5:]))
        a.update(kw)
        return lib.eelg_strut_volume(a["pos"], a["r"], a["shifts"], a["send"], a["recv"], a["node_ptr"], a["edge_ptr"],
                                     a["hn"], a["he"], a["nb"], a["n"], a["e"], a["vol"], stream)
    down = (ctypes.c_int * 5)(0, 2, 72, 71, 360)               # decreases
    short = (ctypes.c_int * 5)(0, 2, 72, 329, 359)             # does not end at the edge count
    late = (ctypes.c_int * 5)(1, 2, 72, 329, 360)              # does not start at 0
    null = ctypes.c_void_p(0)
    for kw, word in [({name: null}, b"null") for name in ("g_pos", "g_r", "pos", "r", "pos0", "m_pos", "m_r", "partner",
                                                          "node_ptr", "edge_ptr", "hn", "he", "shifts", "send", "recv",
                                                          "v0", "vol", "flag")] + \
            [({"nb": 0}, b"graphs"), ({"nb": -3}, b"graphs"), ({"e": -1}, b"graphs"),
             ({"he": ctypes.addressof(down)}, b"never decrease"), ({"he": ctypes.addressof(short)}, b"never decrease"),
             ({"hn": ctypes.addressof(late)}, b"never decrease"), ({"e": 361}, b"never decrease"),
             ({"hyper": hyper[:3] + [0.05, 0.05] + hyper[5:]}, b"r_min"), ({"hyper": hyper[:5] + [-1.0, 1]}, b"move_limit")]:
        assert step(**kw) == -2, kw
        assert word in lib.eelg_last_error(), (kw, lib.eelg_last_error())
    for kw, word in [({name: null}, b"null") for name in ("pos", "r", "shifts", "send", "recv", "node_ptr", "edge_ptr", "hn",
                                                          "he", "vol")] + \
            [({"nb": 0}, b"graphs"), ({"he": ctypes.addressof(down)}, b"never decrease"), ({"n": 95}, b"never decrease")]:
        assert volume(**kw) == -2, kw
        assert word in lib.eelg_last_error(), (kw, lib.eelg_last_error())
    # no edges: the step launches nothing, whatever the geometry pointers
    zero = (ctypes.c_int * 5)(0, 0, 0, 0, 0)
    assert step(e=0, he=ctypes.addressof(zero), g_r=null, r=null, m_r=null, partner=null, shifts=null, send=null,
                recv=null) == 0
    torch.cuda.synchronize()
    assert bool((flag == 7).all()) and bool((bufs["vol"] == 7).all()) and bool((bufs["vol0"] == 7).all())
    for c in ("pos", "r", "m_pos", "m_r"):
        assert torch.equal(bufs[c][5:-5], d[c].reshape(-1)) and bool((bufs[c][:5] == 7).all()) and bool((bufs[c][-5:] == 7).all())
    # the well-formed calls fill their rows and nothing else
    assert volume() == 0 and step() == 0
    torch.cuda.synchronize()
    for c in ("pos", "r", "m_pos", "m_r"):
        assert torch.equal(bufs[c][5:-5], k["out"][c].reshape(-1)), c
    assert torch.equal(bufs["vol"][5:9], k["out"]["vol"]) and torch.equal(bufs["vol0"][5:9], k["vol"])
    assert flag[5:9].tolist() == [0, 0, 0, 0]
    for c, buf in list(bufs.items()) + [("flag", flag)]:
        n = 4 if c in ("vol", "vol0", "flag") else d[c].numel()
        assert bool((buf[:5] == 7).all()) and bool((buf[5 + n:] == 7).all()), c


def test_fused_agrees_with_composed_on_the_device(monkeypatch):
    """EELG_DESIGN_FUSED=0 (the composed torch form on the device) against the fused kernel: entries
    on a clamp are equal, the rest within the bound of the parity test."""
    from gnn import design
    k = case()
    for hyper in ({}, {"r_min": 0.0146484375, "r_max": 0.0400390625, "move_limit": 2.0 ** -8}):
        h = dict(HYPER)
        h.update(hyper)
        got = fused(k, **hyper)
        monkeypatch.setattr(design, "FUSED", False)
        comp = as_dict(design.design_step(k["lay"], *(k["dinp"][key] for key in STEP_KEYS), **h))
        vol = design.strut_volume(k["bd"], k["lay"])
        monkeypatch.undo()
        assert comp["r"].is_cuda and comp["flag"].tolist() == got["flag"].tolist()
        ref = ref_of(k["b"], k["inp"], **hyper)
        cpu = as_dict(design.design_step_composed(design.design_layout(k["b"]), *(k["inp"][key] for key in STEP_KEYS), **h))
        lim = bounds(column_errors(cpu, ref), ref)
        diff = {c: float((comp[c] - got[c]).double().abs().max().cpu() / np.abs(ref[c]).max()) for c in COLUMNS}
        print("fused against composed on the device", hyper, diff)
        record_parity("design_fused_vs_composed" + ("_clamped" if hyper else ""), **diff)
        for c in COLUMNS:
            assert diff[c] <= lim[c], (c, diff[c], lim[c])
        on_r = (comp["r"] == h["r_min"]) | (comp["r"] == h["r_max"])
        on_p = (comp["pos"] == k["dinp"]["pos0"] - h["move_limit"]) | (comp["pos"] == k["dinp"]["pos0"] + h["move_limit"])
        if hyper:
            assert int(on_r.sum()) > 50 and int(on_p.sum()) > 50
        assert torch.equal(comp["r"][on_r], got["r"][on_r]) and torch.equal(comp["pos"][on_p], got["pos"][on_p])
        vdiff = float((vol - k["vol"]).double().abs().max().cpu() / k["vref"].max())
        assert vdiff <= max(4 * k["vbase"], 4 * 2.0 ** -23), vdiff


# ---------------------------------------------------------------------------------------------
E2E = dict(step_r=2.0 ** -11, step_pos=2.0 ** -8, beta=0.5, r_min=2.0 ** -9, r_max=2.0 ** -4, move_limit=2.0 ** -4,
           keep_volume=True)


def end_to_end():
    """Three graphs of 10 nodes / 30 edges, the HIP model with the fp64 oracle's weights, a target
    the oracle predicts on a perturbed geometry (radii +-25 %, positions +-0.02), and the fp64 design
    loop of the oracle alone.  Seeds and step sizes were picked on the CPU from that loop."""
    if "e2e" not in _CASES:
        import oracle.model as omodel
        from gnn import EnergyEquivGNN
        from helpers import batch_to
        b, _ = batch(3, 10, 30, seed=4)
        p = params(2, lmax=2, correlation=2, max_edge_radius=E2E["r_max"])
        torch.manual_seed(2)
        saved = torch.get_default_dtype()
        torch.set_default_dtype(torch.float64)
        try:
            o = omodel.EnergyEquivGNN(p).double()
        finally:
            torch.set_default_dtype(saved)
        m = EnergyEquivGNN(p).to(DEV)
        copy_params(o, m)
        gen = torch.Generator().manual_seed(17)
        bo = batch_to(b, "cpu", torch.float64)
        part = torch.from_numpy(partners(b))
        first = torch.minimum(part, torch.arange(part.shape[0]))
        bo.edge_attr = bo.edge_attr * (1 + 0.25 * torch.randn(part.shape[0], 1, generator=gen, dtype=torch.float64))[first]
        bo.positions = bo.positions + 0.02 * torch.randn(bo.positions.shape, generator=gen, dtype=torch.float64)
        with torch.no_grad():
            target = o(bo)["stiffness"]
        truth = oracle_design_loop(o, b, target, 5, **E2E)
        _CASES["e2e"] = dict(b=b, m=m, target=target, truth=truth)
    return _CASES["e2e"]


def test_the_oracle_loop_descends_without_binding_a_clamp():
    """The precondition of the end-to-end comparison, from the oracle alone."""
    t = end_to_end()["truth"]
    print("oracle design loop: J", t["objective"].tolist(), "kappa", t["kappa"])
    assert (t["objective"][5] < t["objective"][0]).all() and not t["bound"] and t["kappa"] <= 1e3
    assert float(np.abs(t["volume"] / t["volume"][0] - 1).max()) <= 1e-13


def test_optimize_design_follows_the_fp64_oracle_loop():
    """``optimize_design`` on the device against the oracle's loop: objective and volume histories
    and the final geometry within 4x the deviation of the same loop run with
    ``stiffness_sensitivity``'s gradients and the fp32 composed step on the CPU."""
    from gnn import optimize_design, stiffness_sensitivity
    from gnn.design import design_layout, design_step_composed, strut_volume_composed
    k = end_to_end()
    b, m, truth = k["b"], k["m"], k["truth"]
    tgt = k["target"].float().to(DEV)
    bd = b.to(DEV)
    before = {key: getattr(bd, key) for key in ("positions", "edge_attr", "shifts")}
    saved = {key: t.clone() for key, t in before.items()}
    weights = [q.detach().clone() for q in m.parameters()]
    res = optimize_design(m, bd, target=tgt, steps=5, **{key: v for key, v in E2E.items() if key != "r_max"})
    assert res.objective.shape == (6, 3) and res.volume.shape == (6, 3) and res.flags.shape == (5, 3)
    assert res.objective.is_cuda and res.flags.dtype == torch.int32 and not bool(res.flags.any())
    for key, t in before.items():                                  # the input batch is as it was
        assert getattr(bd, key) is t and torch.equal(t, saved[key])
    assert res.batch is not bd and res.batch.shifts is bd.shifts and res.batch.edge_index is bd.edge_index
    assert res.batch.positions.shape == bd.positions.shape and res.batch.edge_attr.shape == bd.edge_attr.shape
    assert all(q.requires_grad and q.grad is None for q in m.parameters())
    assert all(torch.equal(q, w) for q, w in zip(m.parameters(), weights))
    part = torch.from_numpy(partners(b)).to(DEV)
    assert torch.equal(res.batch.edge_attr, res.batch.edge_attr[part])

    # baseline: the HIP model's gradients through stiffness_sensitivity, the step composed in fp32 on the CPU
    lay = design_layout(b)
    pos0, r, shifts = b.positions.clone(), b.edge_attr.reshape(-1).clone(), b.shifts.clone()
    pos, m_pos, m_r = pos0.clone(), torch.zeros(30, 3), torch.zeros(90)
    v0 = strut_volume_composed(b, lay)
    inv = 1.0 / (tgt * tgt).sum(dim=(1, 2))
    work = copy.copy(bd)
    obj, vols = [], [v0]
    for _ in range(5):
        work.positions, work.edge_attr = pos.to(DEV), r.reshape(-1, 1).to(DEV)
        c = m(work)["stiffness"].detach()
        obj.append((0.5 * ((c - tgt) ** 2).sum(dim=(1, 2)) * inv).cpu())
        g = stiffness_sensitivity(m, work, (c - tgt) * inv[:, None, None])
        pos, r, m_pos, m_r, vol, _ = design_step_composed(lay, g["positions"].cpu(), g["edge_attr"].reshape(-1).cpu(), pos, r,
                                                          pos0, m_pos, m_r, shifts, v0, **E2E)
        vols.append(vol)
    work.positions, work.edge_attr = pos.to(DEV), r.reshape(-1, 1).to(DEV)
    c = m(work)["stiffness"].detach()
    obj.append((0.5 * ((c - tgt) ** 2).sum(dim=(1, 2)) * inv).cpu())

    def dev(x, ref):
        return float(np.abs(x.detach().double().cpu().numpy().reshape(ref.shape) - ref).max() / np.abs(ref).max())
    got = dict(objective=dev(res.objective, truth["objective"]), volume=dev(res.volume, truth["volume"]),
               r=dev(res.batch.edge_attr, truth["r"]), pos=dev(res.batch.positions, truth["pos"]))
    base = dict(objective=dev(torch.stack(obj), truth["objective"]), volume=dev(torch.stack(vols), truth["volume"]),
                r=dev(r, truth["r"]), pos=dev(pos, truth["pos"]))
    print("optimize_design against the oracle loop", got, "baseline", base)
    record_parity("optimize_design", fused=got, baseline=base, kappa=truth["kappa"])
    for key in got:
        assert got[key] <= 4 * base[key], (key, got[key], base[key])
    # the volume stays at V0 within the volume's bound
    v = res.volume.double().cpu().numpy()
    assert float(np.abs(v / v[0] - 1).max()) <= 4 * max(base["volume"], 2.0 ** -23)
    assert dev(res.volume[0], truth["volume"][0]) <= 4 * 2.0 ** -23
    # and the run is bitwise repeatable
    again = optimize_design(m, bd, target=tgt, steps=5, **{key: v for key, v in E2E.items() if key != "r_max"})
    assert torch.equal(again.objective, res.objective) and torch.equal(again.volume, res.volume)
    assert torch.equal(again.batch.positions, res.batch.positions) and torch.equal(again.batch.edge_attr, res.batch.edge_attr)


def test_no_host_synchronisation_and_one_step_launch_per_iteration(monkeypatch):
    from gnn import design, ops
    k = end_to_end()
    bd = k["b"].to(DEV)
    tgt = k["target"].float().to(DEV)
    hyper = {key: v for key, v in E2E.items() if key != "r_max"}
    want = design.optimize_design(k["m"], bd, target=tgt, steps=3, **hyper)
    real_layout = design.design_layout

    def refuse(*a, **kw):
        raise AssertionError("the design loop may not read a device tensor back")

    def layout_then_refuse(batch_):
        """set-up may read the host; everything after it may not"""
        lay = real_layout(batch_)
        for name in ("item", "tolist", "cpu"):
            monkeypatch.setattr(torch.Tensor, name, refuse)
        return lay
    monkeypatch.setattr(design, "design_layout", layout_then_refuse)
    monkeypatch.setattr(ops.TIMER, "enabled", True)
    monkeypatch.setattr(ops.TIMER, "records", {})
    res = design.optimize_design(k["m"], bd, target=tgt, steps=3, **hyper)
    launches = {key: len(v) for key, v in ops.TIMER.records.items() if key in ("design_step", "strut_volume")}
    monkeypatch.undo()
    assert launches == {"design_step": 3, "strut_volume": 1}
    assert torch.equal(res.objective, want.objective) and torch.equal(res.volume, want.volume)
    assert torch.equal(res.batch.positions, want.batch.positions) and res.flags.shape == (3, 3)


def test_linear_objective_maximising_the_hill_modulus():
    from gnn import ELASTIC_COLUMNS, optimize_design, property_sensitivity
    from helpers_metrics import directions
    k = end_to_end()
    bd = k["b"].to(DEV)
    w = torch.zeros(3, 12, device=DEV)
    w[:, ELASTIC_COLUMNS.index("E_H")] = -1.0                     # negative: maximise
    d = directions(16).to(DEV)
    dw = torch.zeros(3, 16, device=DEV)
    dw[:, 2] = -0.25
    hyper = {key: v for key, v in E2E.items() if key != "r_max"}
    res = optimize_design(k["m"], bd, weights=w, directions=d, dir_weights=dw, steps=3, **hyper)
    assert res.objective.shape == (4, 3) and res.volume.shape == (4, 3) and res.flags.shape == (3, 3)
    assert bool(torch.isfinite(res.objective).all()) and bool(torch.isfinite(res.volume).all()) and not bool(res.flags.any())
    assert bool(torch.isfinite(res.batch.positions).all()) and bool(torch.isfinite(res.batch.edge_attr).all())
    sens = property_sensitivity(k["m"], bd, w, d, dw)
    want = (w * torch.nan_to_num(sens["properties"])).sum(dim=1) + (dw * sens["e_dir"]).sum(dim=1)
    assert torch.allclose(res.objective[0], want, rtol=1e-6, atol=0)
    # the first step's gradient is property_sensitivity's, bitwise: one step by hand from it gives the same geometry
    from gnn.design import design_layout, design_step, strut_volume
    lay = design_layout(bd)
    one = optimize_design(k["m"], bd, weights=w, directions=d, dir_weights=dw, steps=1, **hyper)
    pos, r = bd.positions.clone(), bd.edge_attr.reshape(-1).clone()
    out = design_step(lay, sens["positions"], sens["edge_attr"].reshape(-1), pos, r, pos, torch.zeros_like(pos),
                      torch.zeros_like(r), bd.shifts, strut_volume(bd, lay), **dict(hyper, r_max=E2E["r_max"]))
    assert torch.equal(one.batch.positions, out[0]) and torch.equal(one.batch.edge_attr.reshape(-1), out[1])
    assert torch.equal(one.volume[1], out[4])
    with pytest.raises(ValueError):
        optimize_design(k["m"], bd, target=k["target"].float().to(DEV), weights=w, steps=1, **hyper)
    with pytest.raises(ValueError):
        optimize_design(k["m"], bd, steps=1, **hyper)
