"""``gnn.elastic`` on the CPU: the composed torch form of the elastic properties against the rank-4
fp64 restatement (``helpers_elastic.reference``) and against known answers, its gradient, the
semantics of a matrix that is not positive definite, the arithmetic of ``csrc/eelg_elastic.h``
compiled into a sanitized host program, and the C ABI's declarations.

Bounds: per column 4x the error the restatement makes when it is run in fp32 on the CPU on the same
inputs (none of the code under test; the project's margin for a second fp32 summation order, as
``test_gpu_metrics``); the gradient likewise against fp32 autograd through the restatement.
Measured on ``spd_set()`` with 250 directions, composed form / baseline: K_V 4.4e-8 / 6.4e-8,
G_V 4.5e-8 / 2.0e-7, K_R 4.9e-8 / 7.3e-6, G_R 3.6e-8 / 5.7e-6, Hill columns <= 4.8e-8 / 8.4e-8 ..
1.6e-7, A_U 3.3e-8 / 6.2e-6, E_min 3.8e-8 / 7.6e-6, E_max 5.1e-8 / 1.6e-5, E_dir 5.8e-8 / 1.6e-5;
gradient 1.9e-6 / 8.8e-4 (the kappa = 3.6e3 square is the worst matrix of both).  The host program
gives the same figures as the composed form to the digits shown: both work in fp64 inside and round
the results to fp32."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from helpers_elastic import (COLUMNS, ISOTROPIC, bad_batch, check_bad_batch, check_tie, cotangents, cubic, errors,
                             gradient, gradient_error, reference, spd_set, tie_case)
from helpers_metrics import directions, isotropic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "energy-equiv-lattice-gnn_amd")
CSRC = os.path.join(PKG, "csrc")
_CASE = {}


def case():
    """The SPD set with 250 directions: fp64 truth, fp32 CPU baseline errors, cotangents and both
    gradients; computed once, shared, never modified."""
    if not _CASE:
        c, d = spd_set(), directions(250)
        rp, re_ = reference(c.double(), d.double())
        bp, be = reference(c, d)
        gp, ge = cotangents(rp, re_)
        gref = gradient(reference, c.double(), d.double(), gp, ge)
        gbase = gradient_error(gradient(reference, c, d, gp, ge), gref)
        _CASE.update(c=c, d=d, ref=(rp, re_), base=errors(bp, be, rp, re_), gp=gp, ge=ge, gref=gref, gbase=gbase)
    return _CASE


def test_columns_and_exports():
    import gnn
    from gnn import design, elastic
    assert elastic.ELASTIC_COLUMNS == COLUMNS and len(COLUMNS) == 12
    for name in ("ELASTIC_COLUMNS", "elastic_properties", "elastic_properties_composed"):
        assert getattr(gnn, name) is getattr(elastic, name)
    assert gnn.property_sensitivity is design.property_sensitivity


def test_the_set_is_positive_definite():
    c = spd_set()
    assert c.shape == (17, 6, 6) and c.dtype == torch.float32 and torch.equal(c, c.transpose(1, 2))
    kappa = np.linalg.cond(c.double().numpy())
    assert float(torch.linalg.eigvalsh(c.double()).min()) > 0 and 4 < kappa.min() and kappa.max() < 1.01e4
    assert torch.equal(c[ISOTROPIC], torch.from_numpy(isotropic(1.5, 0.7)).float())


def test_composed_form_within_4x_of_the_fp32_restatement():
    from gnn.elastic import elastic_properties
    k = case()
    props, e = elastic_properties(k["c"], k["d"])              # CPU tensors: the composed form
    assert props.shape == (17, 12) and e.shape == (17, 250) and props.dtype == e.dtype == torch.float32
    assert bool((props[:, 11] == 1).all())
    assert torch.equal(props[:, 9], e.min(dim=1).values) and torch.equal(props[:, 10], e.max(dim=1).values)
    got = errors(props, e, *k["ref"])
    print("composed form against fp64", got, "fp32 restatement", k["base"])
    for name, v in got.items():
        assert v <= 4 * k["base"][name], (name, v, k["base"][name])
    # without directions: [B, 0], NaN extremes, the nine scalar columns unchanged
    p0, e0 = elastic_properties(k["c"])
    assert e0.shape == (17, 0) and bool(torch.isnan(p0[:, 9:11]).all())
    assert torch.equal(p0[:, :9], props[:, :9]) and torch.equal(p0[:, 11], props[:, 11])


def test_known_answers_isotropic_and_cubic():
    from gnn.elastic import elastic_properties
    lam, mu = 1.5, 0.7
    d = directions(65).double()
    d = d / d.norm(dim=1, keepdim=True)           # unit to fp64: E scales with |d|^-4
    p, e = elastic_properties(torch.from_numpy(isotropic(lam, mu))[None], d)
    young = mu * (3 * lam + 2 * mu) / (lam + mu)
    want = {"K_V": lam + 2 * mu / 3, "K_R": lam + 2 * mu / 3, "K_H": lam + 2 * mu / 3, "G_V": mu, "G_R": mu,
            "G_H": mu, "E_H": young, "nu_H": lam / (2 * (lam + mu)), "A_U": 0.0, "E_min": young, "E_max": young,
            "spd": 1.0}
    for i, name in enumerate(COLUMNS):
        assert abs(float(p[0, i]) - want[name]) < 1e-12, name
    assert float((e - young).abs().max()) < 1e-12
    # cubic (C11, C12, C44) = (3, 1, 0.4): E[100] = 1 / S11 = 2.5, E[111] = 10 / 9, A_U = 1.08
    axes = torch.tensor([[1.0, 0, 0], [0, 1.0, 0], [1, 1, 1], [1, -1, 1]], dtype=torch.float64)
    axes = axes / axes.norm(dim=1, keepdim=True)
    p, e = elastic_properties(torch.from_numpy(cubic(3.0, 1.0, 0.4))[None], axes)
    assert float((e[0] - torch.tensor([2.5, 2.5, 10 / 9, 10 / 9], dtype=torch.float64)).abs().max()) < 1e-12
    zener = 2 * 0.4 / (3.0 - 1.0)
    assert abs(float(p[0, 8]) - 1.2 * (zener ** 0.5 - zener ** -0.5) ** 2) < 1e-12
    assert abs(float(p[0, 8]) - 1.08) < 1e-12
    assert float(p[0, 9]) == float(e[0].min()) and float(p[0, 10]) == float(e[0].max())
    assert abs(float(p[0, 0]) - 5 / 3) < 1e-12 and abs(float(p[0, 2]) - 5 / 3) < 1e-12  # K = (C11 + 2 C12) / 3


def test_first_extreme_takes_the_tie_and_its_gradient():
    from gnn.elastic import elastic_properties
    c, axes = tie_case()
    c.requires_grad_(True)
    p, e = elastic_properties(c, axes)
    g_max, = torch.autograd.grad(p[0, 10], c)
    check_tie(p, e, g_max)


@pytest.mark.parametrize("index", [2, ISOTROPIC, 11])
def test_gradcheck_of_the_composed_form(index):
    from gnn.elastic import elastic_properties_composed
    c = spd_set()[index:index + 1].double().requires_grad_(True)
    d = directions(7).double()

    def fn(x):
        p, e = elastic_properties_composed(x, d)
        cols = p[:, :9] if index == ISOTROPIC else p[:, :11]      # every direction ties: no extremes
        return cols, e
    assert torch.autograd.gradcheck(fn, (c,), eps=1e-7, atol=1e-6, rtol=1e-5)


def test_gradient_of_the_composed_form_within_4x_and_symmetric():
    from gnn.elastic import elastic_properties
    k = case()
    g = gradient(elastic_properties, k["c"], k["d"], k["gp"], k["ge"])
    assert g.shape == (17, 6, 6) and g.dtype == torch.float32
    assert torch.equal(g, g.transpose(1, 2))
    err = gradient_error(g, k["gref"])
    print(f"gradient of the composed form {err:.2e}, fp32 autograd through the restatement {k['gbase']:.2e}")
    assert err <= 4 * k["gbase"], (err, k["gbase"])
    # an input that is not symmetric: the function of its symmetric part, the same gradient
    # (in fp64, where fp32 entries +- an fp32 skew part add up exactly)
    skew = torch.randn(17, 6, 6, generator=torch.Generator().manual_seed(1))
    skew = (0.1 * (skew - skew.transpose(1, 2))).double()
    c64, d64 = k["c"].double(), k["d"].double()
    assert torch.equal(0.5 * ((c64 + skew) + (c64 + skew).transpose(1, 2)), c64)
    assert torch.equal(gradient(elastic_properties, c64 + skew, d64, k["gp"], k["ge"]),
                       gradient(elastic_properties, c64, d64, k["gp"], k["ge"]))


def test_a_matrix_that_is_not_positive_definite_stays_in_its_row():
    from gnn.elastic import elastic_properties
    c, keep, good = bad_batch()
    check_bad_batch(elastic_properties, c, keep, good, directions(65))


def test_arguments_are_validated():
    from gnn.elastic import elastic_properties, elastic_properties_composed
    c, d = spd_set(), directions(5)
    for fn in (elastic_properties, elastic_properties_composed):
        for bad in ((c[0], d), (c[:, :5], d), (c, d[:, :2]), (c, d[0]), (c.long(), d)):
            with pytest.raises(ValueError):
                fn(*bad)


# ---------------------------------------------------------------------------------------------
def _compiler():
    for cxx in (os.environ.get("CXX"), "c++", "g++", "clang++"):
        if cxx and shutil.which(cxx):
            return shutil.which(cxx)
    return None


def test_host_program_sanitized_on_the_set(tmp_path):
    """``csrc/eelg_elastic.h`` in a stand-alone program built with the address and
    undefined-behaviour sanitizers, forward and backward, on the SPD set (250, 65 and 0 directions)
    and the non-SPD cases, against fp64 under the bounds of this file."""
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no C++ compiler")
    exe = str(tmp_path / "elastic_host")
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", CSRC, "-o", exe,
                    os.path.join(ROOT, "tests", "elastic_host_main.cpp")], check=True)

    def rows(t):
        return "\n".join(" ".join(f"{x:.9g}" for x in r) for r in t.flatten(1).tolist())

    def run(c, d, gp=None, ge=None, from_file=False):
        n, p = c.shape[0], d.shape[0]
        text = f"{n} {p} {int(gp is not None)}\n{rows(c)}\n{rows(d)}\n"
        if gp is not None:
            text += f"{rows(gp.float())}\n{rows(ge.float())}\n"
        if from_file:
            (tmp_path / "input.txt").write_text(text)
            r = subprocess.run([exe, str(tmp_path / "input.txt")], capture_output=True, text=True)
        else:
            r = subprocess.run([exe], input=text, capture_output=True, text=True)
        assert r.returncode == 0 and not r.stderr, r.stderr
        lines = r.stdout.split("\n")
        per = 3 if gp is not None else 2
        parse = lambda s: [float(x) for x in s.split()]                      # noqa: E731
        props = torch.tensor([parse(lines[per * g]) for g in range(n)], dtype=torch.float32)
        e = torch.tensor([parse(lines[per * g + 1]) for g in range(n)], dtype=torch.float32).reshape(n, p)
        grad = None
        if gp is not None:
            grad = torch.tensor([parse(lines[per * g + 2]) for g in range(n)], dtype=torch.float32).reshape(n, 6, 6)
        return props, e, grad
    k = case()
    props, e, g = run(k["c"], k["d"], k["gp"], k["ge"])
    got, gerr = errors(props, e, *k["ref"]), gradient_error(g, k["gref"])
    print("host program against fp64", got, f"gradient {gerr:.2e}")
    for name, v in got.items():
        assert v <= 4 * k["base"][name], (name, v, k["base"][name])
    assert gerr <= 4 * k["gbase"], (gerr, k["gbase"])
    assert torch.equal(g, g.transpose(1, 2)) and bool((props[:, 11] == 1).all())
    assert torch.equal(props[:, 9], e.min(dim=1).values) and torch.equal(props[:, 10], e.max(dim=1).values)
    again = run(k["c"], k["d"], k["gp"], k["ge"], from_file=True)
    assert all(torch.equal(a, b) for a, b in zip((props, e, g), again))
    # 65 directions (a second pass of lane 0 only) and none
    d65 = directions(65)
    r65 = reference(k["c"].double(), d65.double())
    b65 = errors(*reference(k["c"], d65), *r65)
    p65, e65, _ = run(k["c"], d65)
    for name, v in errors(p65, e65, *r65).items():
        assert v <= 4 * b65[name], (name, v, b65[name])
    p0, e0, g0 = run(k["c"], d65[:0], k["gp"], k["ge"][:, :0])
    assert e0.shape == (17, 0) and bool(torch.isnan(p0[:, 9:11]).all()) and torch.equal(p0[:, :9], props[:, :9])
    assert bool(torch.isfinite(g0).all()) and torch.equal(g0, g0.transpose(1, 2))
    # the tie: the first of three equal directions is the extreme
    c_tie, axes = tie_case()
    gp_tie = torch.zeros(1, 12)
    gp_tie[0, 10] = 1.0
    pt, et, gt = run(c_tie, axes, gp_tie, torch.zeros(1, 4))
    check_tie(pt, et, gt)

    # not positive definite: the flag, NaN, the Voigt terms alone and exact zeros
    c, keep, good = bad_batch()

    def host(x, d):
        """the host program as a differentiable function of ``x`` for ``check_bad_batch``"""
        class Fn(torch.autograd.Function):
            @staticmethod
            def forward(ctx, xx):
                ctx.xx = xx.detach()
                p, ee, _ = run(ctx.xx, d)
                return p, ee

            @staticmethod
            def backward(ctx, gpp, gee):
                return run(ctx.xx, d, gpp, gee)[2]
        return Fn.apply(x)
    check_bad_batch(host, c, keep, good, directions(65))


@pytest.mark.parametrize("name", ["eelg_elastic_props", "eelg_elastic_props_bwd"])
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
    assert re.search(r"#define\s+EELG_ELASTIC_COLS\s+12\b", text) and _lib.ELASTIC_COLS == 12
    src = open(os.path.join(CSRC, "eelg_elastic.hip")).read()
    assert re.search(r"\b" + name + r"\s*\(", src)
    assert "eelg_elastic.o" in open(os.path.join(CSRC, "Makefile")).read()
