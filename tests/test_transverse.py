"""``gnn.transverse`` on the CPU: the closed forms against a brute-force scan of the rank-4
expressions, the composed torch form against the rank-4 fp64 restatement
(``helpers_transverse.reference``) and against known answers, its gradient, the semantics of a
matrix that is not positive definite, the arithmetic of ``csrc/eelg_transverse.h`` compiled into a
sanitized host program, and the C ABI's declarations.

Bounds: per column 4x the error the restatement makes when it is run in fp32 on the CPU on the same
inputs (none of the code under test; the project's margin for a second fp32 summation order, as
``test_elastic``), at least 4 fp32 ulps of the column's largest magnitude; the gradient likewise
against fp32 autograd through the restatement.  Errors are normalised per graph: a G entry by its
own fp64 value, a nu entry absolutely, a beta entry by the graph's largest |beta|.

The gradient and ``n_ext`` comparisons leave out the (matrix, direction) pairs with fp64 R_G <= 1e-9
M_G or R_nu E <= 1e-9 (5 of 4,250 on ``spd_set()`` x ``directions(250)``, all on the isotropic matrix,
which is rounded to fp32 and so keeps an anisotropy of 4e-8; at most 10 % may be left out), and the
cotangent of an extreme whose two best directions lie within 1e-6 in fp64: there the direction that
takes the gradient is decided by the rounding of the fp32 values.  Gradient and ``n_ext`` are bounded
matrix by matrix: the fp32 restatement loses the isotropic matrix's gradient altogether (0.8 of its
largest entry), and a bound from the set's largest baseline error would check nothing.

Measured on ``spd_set()`` with 250 directions, composed form / fp32 restatement: G_min 4.2e-8 /
7.9e-6, G_max 5.3e-8 / 1.6e-5, nu_min 3.3e-7 / 2.6e-5, nu_max 4.0e-7 / 8.1e-5, beta_min 2.5e-8 /
4.8e-6, beta_max 4.5e-8 / 8.0e-6, G_lo 5.9e-8 / 8.3e-6, G_hi 5.9e-8 / 3.4e-5, nu_lo 4.4e-7 / 8.8e-5,
nu_hi 4.2e-7 / 1.2e-4, beta 5.1e-8 / 8.0e-6; gradient per matrix <= 1.9e-7 / 2.1e-7 .. 4.0e-4 (0.82 on
the isotropic matrix); n_ext <= 5.6e-8 / 5.3e-8 .. 4.3e-7 (0.34).  The host program gives the same rows
to the digits shown and the gradient to <= 1.3e-7: both work in fp64 inside and round the results to
fp32."""
import math
import os
import re
import shutil
import subprocess

import pytest
import torch

from helpers_elastic import ISOTROPIC, cubic
from helpers_metrics import directions, isotropic
from helpers_transverse import (COLUMNS, DIR_COLUMNS, bad_batch, bounds, check_bad_batch, check_tie, cotangents,
                                crystal_directions, errors, excluded, gradient, gradient_error, normal_error, reference,
                                reference_fn, scan, spd_set, tie_case, within)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "energy-equiv-lattice-gnn_amd")
CSRC = os.path.join(PKG, "csrc")
_CASE = {}


def case():
    """The SPD set with 250 directions: fp64 truth, fp32 CPU baseline errors, cotangents and both
    gradients; computed once, shared, never modified."""
    if not _CASE:
        c, d = spd_set(), directions(250)
        ref = reference(c, d)
        b32 = reference(c, d, torch.float32)
        gp, gt = cotangents(ref)
        gref = gradient(reference_fn(torch.float64), c.double(), d, gp, gt)
        gbase = gradient_error(gradient(reference_fn(torch.float32), c, d, gp, gt), gref)
        n32 = b32["normals"][torch.arange(17)[:, None], b32["arg"][:, :4], torch.arange(4)[None]]
        _CASE.update(c=c, d=d, ref=ref, base=errors(b32["props"], b32["t_dir"], ref), gp=gp, gt=gt, gref=gref,
                     gbase=gbase, nbase=normal_error(n32, b32["arg"], ref))
    return _CASE


def test_columns_and_exports():
    import gnn
    from gnn import transverse
    assert transverse.TRANSVERSE_COLUMNS == COLUMNS and transverse.TRANSVERSE_DIR_COLUMNS == DIR_COLUMNS
    for name in ("TRANSVERSE_COLUMNS", "TRANSVERSE_DIR_COLUMNS", "transverse_properties",
                 "transverse_properties_composed"):
        assert getattr(gnn, name) is getattr(transverse, name)


def test_closed_forms_bracket_a_scan_of_32768_angles():
    """Restatement and composed form against the brute-force scan on 17 matrices x 26 directions.  The
    scan samples a sinusoid of amplitude R at spacing pi / K in its phase's half, so it misses an
    extreme by at most R (pi / K)^2 / 2; the closed form may differ from it by that plus 1e-12 of the
    value, and must not lie inside the scanned range."""
    from gnn.transverse import transverse_properties_composed
    c, d = spd_set().double(), crystal_directions()
    k = 32768
    got = scan(c, d, k)
    ref = reference(c, d)
    comp = transverse_properties_composed(c, d)[1]
    miss = 0.5 * (math.pi / k) ** 2
    for name, t in (("restatement", ref["t_dir"]), ("composed", comp)):
        inv_lo, inv_hi = 1 / t[:, :, 0], 1 / t[:, :, 1]          # 1 / G_lo is the largest 1 / G
        amp_g = 0.5 * (inv_lo - inv_hi)
        amp_n = 0.5 * (t[:, :, 3] - t[:, :, 2])
        for closed, scanned, amp, sign in ((inv_lo, got["inv_g_max"], amp_g, 1), (inv_hi, got["inv_g_min"], amp_g, -1),
                                           (t[:, :, 3], got["nu_max"], amp_n, 1), (t[:, :, 2], got["nu_min"], amp_n, -1)):
            gap = sign * (closed - scanned)                     # >= 0: the closed form is outside the range
            tol = 1e-12 * closed.abs()
            assert bool((gap >= -tol).all()), (name, float((gap + tol).min()))
            assert bool((gap <= amp * miss + tol).all()), (name, float((gap - amp * miss - tol).max()))


def test_known_answers_cubic_auxetic_and_isotropic():
    from gnn.transverse import transverse_properties
    s2, s3 = math.sqrt(2.0), math.sqrt(3.0)
    d = torch.tensor([[1 / s2, 1 / s2, 0], [1.0, 0, 0], [1 / s3, 1 / s3, 1 / s3], [0.6, 0, 0.8]], dtype=torch.float64)
    c = torch.from_numpy(cubic(2.0, 1.6, 0.3))[None].requires_grad_(True)
    props, t, arg, n_ext = transverse_properties(c, d)
    s11 = (2.0 + 1.6) / ((2.0 - 1.6) * (2.0 + 2 * 1.6))
    s12 = -1.6 / ((2.0 - 1.6) * (2.0 + 2 * 1.6))
    s44 = 1 / 0.3
    j = s11 - s12 - s44 / 2
    want = [1 / (2 * (s11 - s12)), 1 / s44, -(s12 + j / 2) / (s11 - j / 2), -s12 / (s11 - j / 2), s11 + 2 * s12]
    assert abs(want[0] - 0.2) < 1e-15 and abs(want[1] - 0.3) < 1e-15 and abs(want[2] - 0.26829268) < 1e-8
    assert abs(want[3] - 0.58536585) < 1e-8 and abs(want[4] - 0.19230769) < 1e-8
    assert float((t[0, 0] - torch.tensor(want, dtype=torch.float64)).abs().max()) < 1e-12
    # [100] and [111]: the transverse plane is isotropic, both extremes coincide
    for p in (1, 2):
        assert abs(float(t[0, p, 0] - t[0, p, 1])) < 1e-12 and abs(float(t[0, p, 2] - t[0, p, 3])) < 1e-12
        g, = torch.autograd.grad(t[0, p, :4].sum(), c, retain_graph=True)
        assert bool(torch.isfinite(g).all()) and float((g - g.transpose(1, 2)).abs().max()) < 1e-12
    assert abs(float(t[0, 1, 0]) - 0.3) < 1e-12 and abs(float(t[0, 1, 2]) + s12 / s11) < 1e-12
    assert props[0, :6].tolist() == [float(t[0, :, 0].min()), float(t[0, :, 1].max()), float(t[0, :, 2].min()),
                                     float(t[0, :, 3].max()), float(t[0, :, 4].min()), float(t[0, :, 4].max())]
    assert int(arg[0, 0]) == 0 and int(arg[0, 2]) == 0
    flat = torch.tensor([1 / s2, -1 / s2, 0], dtype=torch.float64)
    assert abs(abs(float(n_ext[0, 0] @ flat)) - 1) < 1e-12      # the soft shear and nu_min of [110] are along [1-10]
    assert abs(abs(float(n_ext[0, 2] @ flat)) - 1) < 1e-12

    # auxetic: nu([110], [1-10]) = -(S12 + J / 2) / (S11 - J / 2) < 0 for (C11, C12, C44) = (1, 0.6, 1.5)
    aux = torch.from_numpy(cubic(1.0, 0.6, 1.5))[None]
    a11 = (1.0 + 0.6) / ((1.0 - 0.6) * (1.0 + 1.2))
    a12 = -0.6 / ((1.0 - 0.6) * (1.0 + 1.2))
    ja = a11 - a12 - 1 / (2 * 1.5)
    nu_flat = -(a12 + ja / 2) / (a11 - ja / 2)
    assert nu_flat < -0.1
    dd = torch.cat([directions(9).double(), d[:1]])
    props, t, arg, n_ext = transverse_properties(aux, dd)
    assert abs(float(props[0, 2]) - nu_flat) < 1e-12 and int(arg[0, 2]) == 9
    assert abs(abs(float(n_ext[0, 2] @ flat)) - 1) < 1e-9
    assert abs(float(n_ext[0, 2] @ dd[9])) < 1e-12 and abs(float(n_ext[0, 2].norm()) - 1) < 1e-12

    # isotropic: G = mu, nu = lam / (2 (lam + mu)), beta = (1 - 2 nu) / E in every direction
    lam, mu = 1.5, 0.7
    d65 = directions(65).double()
    d65 = d65 / d65.norm(dim=1, keepdim=True)
    props, t, _, _ = transverse_properties(torch.from_numpy(isotropic(lam, mu))[None], d65)
    nu = lam / (2 * (lam + mu))
    young = mu * (3 * lam + 2 * mu) / (lam + mu)
    for col, v in zip(range(5), (mu, mu, nu, nu, (1 - 2 * nu) / young)):
        assert float((t[0, :, col] - v).abs().max()) < 1e-12, col
    assert float(props[0, 6]) == 1.0


def test_composed_form_within_4x_of_the_fp32_restatement():
    from gnn.transverse import transverse_properties
    k = case()
    out = excluded(k["ref"])
    print("excluded pairs", int(out.sum()), "of", out.numel(), "on the isotropic matrix", int(out[ISOTROPIC].sum()))
    assert out.shape == (17, 250) and int(out.sum()) <= 0.1 * out.numel()
    props, t, arg, n_ext = transverse_properties(k["c"], k["d"])             # CPU tensors: the composed form
    assert props.shape == (17, 7) and t.shape == (17, 250, 5) and arg.shape == (17, 6) and n_ext.shape == (17, 4, 3)
    assert props.dtype == t.dtype == n_ext.dtype == torch.float32 and arg.dtype == torch.int32
    assert bool((props[:, 6] == 1).all())
    for i, src in enumerate((0, 1, 2, 3, 4, 4)):
        col = t[:, :, src]
        assert torch.equal(props[:, i], col.max(dim=1).values if i & 1 else col.min(dim=1).values)
        assert torch.equal(col.gather(1, arg[:, i:i + 1].long())[:, 0], props[:, i])
    got, bound = errors(props, t, k["ref"]), bounds(k["base"], k["ref"])
    nerr = normal_error(n_ext, arg, k["ref"])
    print("composed form against fp64", got, "fp32 restatement", k["base"], "n_ext", nerr, k["nbase"])
    for name, v in got.items():
        assert v <= bound[name], (name, v, bound[name])
    assert within(nerr, k["nbase"]), (nerr, k["nbase"])
    # no directions: [B, 0, 5], NaN extremes, arg -1
    p0, t0, a0, n0 = transverse_properties(k["c"], k["d"][:0])
    assert t0.shape == (17, 0, 5) and bool(torch.isnan(p0[:, :6]).all()) and bool((p0[:, 6] == 1).all())
    assert bool((a0 == -1).all()) and bool(torch.isnan(n0).all())


def test_gradient_of_the_composed_form_within_4x_and_symmetric():
    from gnn.transverse import transverse_properties
    k = case()
    g = gradient(transverse_properties, k["c"], k["d"], k["gp"], k["gt"])
    assert g.shape == (17, 6, 6) and g.dtype == torch.float32
    assert torch.equal(g, g.transpose(1, 2))
    err = gradient_error(g, k["gref"])
    print("gradient of the composed form", err, "fp32 autograd through the restatement", k["gbase"])
    assert within(err, k["gbase"]), (err, k["gbase"])
    # with the excluded pairs' cotangents too: finite and symmetric
    gp, gt = cotangents(k["ref"], keep_excluded=True)
    g_all = gradient(transverse_properties, k["c"], k["d"], gp, gt)
    assert bool(torch.isfinite(g_all).all()) and torch.equal(g_all, g_all.transpose(1, 2))


@pytest.mark.parametrize("index", [0, 2, 11])                 # no cubic matrix: its beta is the same everywhere
def test_gradcheck_of_the_composed_form(index):
    from gnn.transverse import transverse_properties_composed
    c = spd_set()[index:index + 1].double().requires_grad_(True)
    d = directions(7).double()

    def fn(x):
        return transverse_properties_composed(x, d)[:2]
    assert torch.autograd.gradcheck(fn, (c,), eps=1e-7, atol=1e-6, rtol=1e-5)


def test_first_extreme_takes_the_tie_and_its_gradient():
    from gnn.transverse import transverse_properties
    check_tie(transverse_properties, *tie_case())


def test_a_matrix_that_is_not_positive_definite_stays_in_its_row():
    from gnn.transverse import transverse_properties
    c, keep, good = bad_batch()
    check_bad_batch(transverse_properties, c, keep, good, directions(65))


def test_arguments_are_validated():
    from gnn.transverse import transverse_properties, transverse_properties_composed
    c, d = spd_set(), directions(5)
    for fn in (transverse_properties, transverse_properties_composed):
        for bad in ((c[0], d), (c[:, :5], d), (c, d[:, :2]), (c, d[0]), (c.long(), d), (c, None)):
            with pytest.raises(ValueError):
                fn(*bad)


def test_design_keywords_are_validated():
    from gnn.design import _property_cotangents
    w = torch.zeros(2, 12)
    with pytest.raises(ValueError):
        _property_cotangents(w, None, None, transverse_weights=torch.zeros(2, 7))
    c = spd_set()[:2].clone().requires_grad_(True)
    d = directions(5)
    with pytest.raises(ValueError):
        _property_cotangents(w, d, None, transverse_weights=torch.zeros(2, 6))(c)
    with pytest.raises(ValueError):
        _property_cotangents(w, d, None, transverse_dir_weights=torch.zeros(2, 5, 4))(c)
    tw = torch.zeros(2, 7)
    tw[:, 2] = 1.0
    extra, outputs, grads = _property_cotangents(w, d, None, transverse_weights=tw)(c)
    assert set(extra) == {"properties", "e_dir", "transverse", "t_dir"} and len(outputs) == len(grads) == 2
    assert extra["transverse"].shape == (2, 7) and extra["t_dir"].shape == (2, 5, 5)
    plain = _property_cotangents(w, d, None)(c)
    assert set(plain[0]) == {"properties", "e_dir"} and len(plain[1]) == 1


# ---------------------------------------------------------------------------------------------
def _compiler():
    for cxx in (os.environ.get("CXX"), "c++", "g++", "clang++"):
        if cxx and shutil.which(cxx):
            return shutil.which(cxx)
    return None


def test_host_program_sanitized_on_the_set(tmp_path):
    """``csrc/eelg_transverse.h`` in a stand-alone program built with the address and
    undefined-behaviour sanitizers, forward and backward, on the SPD set (250, 65 and 0 directions),
    the tie and the non-SPD cases, against fp64 under the bounds of this file."""
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no C++ compiler")
    exe = str(tmp_path / "transverse_host")
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", CSRC, "-o", exe,
                    os.path.join(ROOT, "tests", "transverse_host_main.cpp")], check=True)

    def rows(t):
        return "\n".join(" ".join(f"{x:.9g}" for x in r) for r in t.flatten(1).tolist())

    def run(c, d, gp=None, gt=None, from_file=False):
        n, p = c.shape[0], d.shape[0]
        text = f"{n} {p} {int(gp is not None)}\n{rows(c)}\n{rows(d)}\n"
        if gp is not None:
            text += f"{rows(gp.float())}\n{rows(gt.float())}\n"
        if from_file:
            (tmp_path / "input.txt").write_text(text)
            r = subprocess.run([exe, str(tmp_path / "input.txt")], capture_output=True, text=True)
        else:
            r = subprocess.run([exe], input=text, capture_output=True, text=True)
        assert r.returncode == 0 and not r.stderr, r.stderr
        lines = r.stdout.split("\n")
        per = 5 if gp is not None else 4
        parse = lambda s: [float(x) for x in s.split()]                      # noqa: E731
        props = torch.tensor([parse(lines[per * g]) for g in range(n)], dtype=torch.float32)
        t = torch.tensor([parse(lines[per * g + 1]) for g in range(n)], dtype=torch.float32).reshape(n, p, 5)
        arg = torch.tensor([[int(x) for x in lines[per * g + 2].split()] for g in range(n)], dtype=torch.int32)
        n_ext = torch.tensor([parse(lines[per * g + 3]) for g in range(n)], dtype=torch.float32).reshape(n, 4, 3)
        grad = None
        if gp is not None:
            grad = torch.tensor([parse(lines[per * g + 4]) for g in range(n)], dtype=torch.float32).reshape(n, 6, 6)
        return props, t, arg, n_ext, grad

    def host(x, d):
        """the host program as a differentiable function of ``x``"""
        class Fn(torch.autograd.Function):
            @staticmethod
            def forward(ctx, xx):
                ctx.xx = xx.detach()
                out = run(ctx.xx, d)[:4]
                ctx.mark_non_differentiable(out[2], out[3])
                return out

            @staticmethod
            def backward(ctx, gpp, gtt, _a, _n):
                gpp = torch.zeros(ctx.xx.shape[0], 7) if gpp is None else gpp
                gtt = torch.zeros(ctx.xx.shape[0], d.shape[0], 5) if gtt is None else gtt
                return run(ctx.xx, d, gpp, gtt)[4]
        return Fn.apply(x)
    k = case()
    props, t, arg, n_ext, g = run(k["c"], k["d"], k["gp"], k["gt"])
    got, bound = errors(props, t, k["ref"]), bounds(k["base"], k["ref"])
    gerr, nerr = gradient_error(g, k["gref"]), normal_error(n_ext, arg, k["ref"])
    print("host program against fp64", got, "gradient", gerr, "n_ext", nerr)
    for name, v in got.items():
        assert v <= bound[name], (name, v, bound[name])
    assert within(gerr, k["gbase"]) and within(nerr, k["nbase"])
    assert torch.equal(g, g.transpose(1, 2)) and bool((props[:, 6] == 1).all())
    again = run(k["c"], k["d"], k["gp"], k["gt"], from_file=True)
    assert all(torch.equal(a, b) for a, b in zip((props, t, arg, n_ext, g), again))
    # the composed form agrees to rounding of the fp32 results
    from gnn.transverse import transverse_properties
    cp, ct, ca, cn = transverse_properties(k["c"], k["d"])
    assert torch.equal(ca, arg)
    assert float(((cp[:, :6] - props[:, :6]).abs() / props[:, :6].abs()).max()) <= 2.0 ** -22
    assert float(((ct - t).abs() / t.abs()).max()) <= 2.0 ** -22 and float((cn - n_ext).abs().max()) <= 2.0 ** -22
    # every cotangent, the excluded pairs' too: finite and symmetric
    gp_all, gt_all = cotangents(k["ref"], keep_excluded=True)
    g_all = run(k["c"], k["d"], gp_all, gt_all)[4]
    assert bool(torch.isfinite(g_all).all()) and torch.equal(g_all, g_all.transpose(1, 2))
    # 65 directions (a second pass of lane 0 only) and none
    d65 = directions(65)
    r65 = reference(k["c"], d65)
    b65 = reference(k["c"], d65, torch.float32)
    p65, t65 = run(k["c"], d65)[:2]
    bound65 = bounds(errors(b65["props"], b65["t_dir"], r65), r65)
    for name, v in errors(p65, t65, r65).items():
        assert v <= bound65[name], (name, v, bound65[name])
    p0, t0, a0, n0, g0 = run(k["c"], d65[:0], k["gp"], k["gt"][:, :0])
    assert t0.shape == (17, 0, 5) and bool(torch.isnan(p0[:, :6]).all()) and bool((a0 == -1).all())
    assert bool(torch.isnan(n0).all()) and bool((g0 == 0).all())
    check_tie(host, *tie_case())
    c, keep, good = bad_batch()
    check_bad_batch(host, c, keep, good, d65)


@pytest.mark.parametrize("name", ["eelg_transverse_props", "eelg_transverse_props_bwd"])
def test_entry_points_declared_as_bound(name):
    from gnn import _lib
    text = open(os.path.join(ROOT, "include", "eelg.h")).read()
    found = re.findall(r"\b(?:int|long long)\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
    assert len(found) == 1, name
    args = [a.strip() for a in found[0].split(",") if a.strip()]
    assert name in _lib._SIGS and name in _lib.EXPORTED_SYMBOLS
    bound = _lib._SIGS[name][0]
    assert len(args) == len(bound), (args, bound)
    for a, b in zip(args, bound):             # pointers as addresses, counts as int
        assert (b is _lib._P) == ("*" in a) and (b is _lib._I) == a.startswith("int "), (a, b)
    assert re.search(r"#define\s+EELG_TRANSVERSE_COLS\s+7\b", text) and _lib.TRANSVERSE_COLS == 7
    assert re.search(r"#define\s+EELG_TRANSVERSE_DIR_COLS\s+5\b", text) and _lib.TRANSVERSE_DIR_COLS == 5
    src = open(os.path.join(CSRC, "eelg_transverse.hip")).read()
    assert re.search(r"\b" + name + r"\s*\(", src)
    assert "eelg_transverse.o" in open(os.path.join(CSRC, "Makefile")).read()
