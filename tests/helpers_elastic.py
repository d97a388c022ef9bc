"""Rank-4 restatement of the elastic properties (``gnn.elastic``) and the SPD matrix set of the
elastic tests.  The restatement symmetrises C, forms the cartesian rank-4 stiffness and compliance
with ``helpers_mandel.mandel_to_cart4`` and ``torch.linalg.inv`` and evaluates
    K_V = C_iijj / 9, G_V = (3 C_ijij - C_iijj) / 30, K_R = 1 / S_iijj,
    G_R = 15 / (6 S_ijij - 2 S_iijj), E_p = 1 / (S_ijkl d_i d_j d_k d_l);
run in fp64 it is the truth, run in fp32 on the CPU the baseline of the bounds.  None of the code
under test is used: the shared checks below take the implementation as an argument."""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np
import torch

from helpers_mandel import mandel_to_cart4
from helpers_metrics import hostile_set

COLUMNS = ("K_V", "G_V", "K_R", "G_R", "K_H", "G_H", "E_H", "nu_H", "A_U", "E_min", "E_max", "spd")
ISOTROPIC = 5                     # index of the isotropic matrix in spd_set(): every direction ties


def cubic(c11: float, c12: float, c44: float) -> np.ndarray:
    """Mandel matrix of a cubic material (shear diagonal 2 C44)."""
    c = np.zeros((6, 6))
    c[:3, :3] = c12
    c[np.arange(3), np.arange(3)] = c11
    c[np.arange(3, 6), np.arange(3, 6)] = 2 * c44
    return c


def spd_set() -> torch.Tensor:
    """[17, 6, 6] fp32, symmetric positive definite: matrices 0-5, 8 and 9 of the hostile set (random
    SPD, diagonal, isotropic, scales 1e-4 and 1e5), two cubic matrices, four squares of random
    symmetric matrices (the shape of ``matrix_power_2`` outputs) and three matrices with condition
    numbers 1e2, 1e3 and 1e4."""
    h = hostile_set().double().numpy()
    mats = [h[i] for i in (0, 1, 2, 3, 4, 5, 8, 9)]
    mats += [cubic(3.0, 1.0, 0.4), cubic(1.0, 0.6, 1.5)]
    rng = np.random.default_rng(7)
    for _ in range(4):
        s = rng.normal(size=(6, 6))
        s = (s + s.T) / 2
        mats.append(s @ s)
    for kappa in (1e2, 1e3, 1e4):
        q, _ = np.linalg.qr(rng.normal(size=(6, 6)))
        m = q @ np.diag(np.geomspace(1.0, kappa, 6)) @ q.T
        mats.append((m + m.T) / 2)
    out = torch.from_numpy(np.stack(mats)).float()
    return (out + out.transpose(1, 2)) / 2


def reference(c: torch.Tensor, dirs: Optional[torch.Tensor]):
    """``(props [B, 12], e_dir [B, P])`` in ``c``'s dtype, differentiable in ``c``."""
    a = 0.5 * (c + c.transpose(1, 2))
    s = torch.linalg.inv(a)
    c4, s4 = mandel_to_cart4(a), mandel_to_cart4(s)
    c_iijj, c_ijij = torch.einsum("biijj->b", c4), torch.einsum("bijij->b", c4)
    s_iijj, s_ijij = torch.einsum("biijj->b", s4), torch.einsum("bijij->b", s4)
    kv, gv = c_iijj / 9, (3 * c_ijij - c_iijj) / 30
    kr, gr = 1 / s_iijj, 15 / (6 * s_ijij - 2 * s_iijj)
    kh, gh = (kv + kr) / 2, (gv + gr) / 2
    eh = 9 * kh * gh / (3 * kh + gh)
    nu = (3 * kh - 2 * gh) / (2 * (3 * kh + gh))
    au = 5 * gv / gr + kv / kr - 6
    nb = c.shape[0]
    if dirs is not None and dirs.shape[0]:
        d = dirs.to(c.dtype)
        e = 1 / torch.einsum("bijkl,pi,pj,pk,pl->bp", s4, d, d, d, d)
        emin, emax = e.min(dim=1).values, e.max(dim=1).values
    else:
        e = c.new_zeros((nb, 0))
        emin = emax = c.new_full((nb,), float("nan"))
    spd = (torch.linalg.eigvalsh(a.detach().double()).min(dim=1).values > 0).to(c.dtype)
    return torch.stack([kv, gv, kr, gr, kh, gh, eh, nu, au, emin, emax, spd], dim=1), e


def errors(props: torch.Tensor, e_dir: torch.Tensor, ref_props: torch.Tensor, ref_e: torch.Tensor) -> Dict[str, float]:
    """Per column (and for ``E_dir``) the largest error over the graphs: relative to the graph's own
    fp64 value, except ``A_U`` (relative to ``A_U + 6``: its absolute size explodes with the
    condition number, and it is zero for an isotropic matrix) and ``nu_H`` (absolute)."""
    p, r = props.detach().double().cpu(), ref_props.detach().double().cpu()
    out = {}
    for i, k in enumerate(COLUMNS[:11]):
        if torch.isnan(r[:, i]).all():            # E_min / E_max without directions
            continue
        scale = torch.ones_like(r[:, i]) if k == "nu_H" else (r[:, i] + 6 if k == "A_U" else r[:, i]).abs()
        out[k] = float(((p[:, i] - r[:, i]).abs() / scale).max())
    if ref_e.shape[1]:
        e, re = e_dir.detach().double().cpu(), ref_e.detach().double().cpu()
        out["E_dir"] = float(((e - re).abs() / re.abs()).max())
    return out


def cotangents(ref_props: torch.Tensor, ref_e: torch.Tensor, seed: int = 5):
    """``(g_props [B, 12], g_e_dir [B, P])`` fp64: ``randn`` from a fixed CPU generator, each divided
    by |property| (``e_dir``: by E P; ``A_U``: by ``A_U + 6`` as in ``errors``, since ``A_U`` itself is
    zero to rounding for the isotropic matrix), so that every column weighs alike.  Zero on the ``spd`` column,
    on ``E_min`` / ``E_max`` where there are no directions, and on ``E_min`` / ``E_max`` of a graph all
    of whose directions tie to 1e-6 (the isotropic matrix: the first extreme is decided by rounding)."""
    gen = torch.Generator().manual_seed(seed)
    r, re = ref_props.detach().double(), ref_e.detach().double()
    scale = r.abs()
    scale[:, 8] = (r[:, 8] + 6).abs()
    gp = torch.randn(r.shape, generator=gen, dtype=torch.float64) / scale
    gp[:, 11] = 0
    n_dirs = int(re.shape[1])
    ge = torch.randn(re.shape, generator=gen, dtype=torch.float64) / (re.abs() * max(n_dirs, 1))
    if n_dirs:
        ties = (re.max(dim=1).values - re.min(dim=1).values) <= 1e-6 * re.abs().max(dim=1).values
        gp[ties, 9:11] = 0
    else:
        gp[:, 9:11] = 0
    return gp, ge


def gradient(fn, c: torch.Tensor, dirs, g_props: torch.Tensor, g_e: torch.Tensor) -> torch.Tensor:
    """Gradient of ``sum(g_props * props) + sum(g_e * e_dir)`` of ``fn(c, dirs)`` w.r.t. ``c``."""
    x = c.detach().clone().requires_grad_(True)
    props, e = fn(x, dirs)
    outs, gs = [props], [g_props.to(device=props.device, dtype=props.dtype)]
    if e.shape[1]:
        outs.append(e)
        gs.append(g_e.to(device=e.device, dtype=e.dtype))
    return torch.autograd.grad(outs, [x], gs)[0]


def gradient_error(g: torch.Tensor, ref: torch.Tensor) -> float:
    """For each matrix the largest error relative to that matrix's largest fp64 gradient entry;
    the maximum over the set."""
    g, ref = g.detach().double().cpu(), ref.detach().double().cpu()
    big = ref.abs().amax(dim=(1, 2))
    return float(((g - ref).abs().amax(dim=(1, 2)) / big).max())


# ---- cases and assertions shared by the CPU and the device tests (``fn`` is the implementation) ----
def bad_batch():
    """SPD matrices 0, 11, 16 of the set with the indefinite matrix of the hostile set at position
    1 and an all-NaN matrix at position 3; (batch, positions of the good graphs, their matrices)."""
    good = spd_set()[[0, 11, 16]]
    c = torch.stack([good[0], hostile_set()[7], good[1], torch.full((6, 6), float("nan")), good[2]])
    return c, [0, 2, 4], good


def tie_case():
    """diag(2, 2, 2, 1, 1, 1) with the directions [010], [100], [001], [111]: the three axes give
    bitwise the same E = 2 (the largest), so E_max is entry 0 and its gradient is that of [010]
    alone: 1 at entry (1, 1), nothing at (0, 0) and (2, 2)."""
    c = torch.diag(torch.tensor([2.0, 2, 2, 1, 1, 1]))[None]
    axes = torch.cat([torch.eye(3)[[1, 0, 2]], torch.full((1, 3), 3 ** -0.5)])
    return c, axes


def check_tie(props, e, g_max):
    props, e = props.detach(), e.detach()
    assert float(e[0, 0]) == float(e[0, 1]) == float(e[0, 2]) == float(props[0, 10]) == 2.0
    assert float(props[0, 9]) == float(e[0, 3]) and abs(float(e[0, 3]) - 1.2) < 1e-6
    want = torch.zeros(6, 6)
    want[1, 1] = 1.0
    assert float((g_max[0].float().cpu() - want).abs().max()) < 1e-6, g_max


def check_bad_batch(fn, c, keep, good, d, sync=lambda: None):
    """The assertions of the non-SPD semantics, shared with the device test: ``fn`` is the
    implementation, graphs 1 (indefinite) and 3 (all NaN) of ``c`` are the bad ones."""
    x = c.clone().requires_grad_(True)
    props, e = props_live, e_live = fn(x, d)
    y = good.clone().requires_grad_(True)
    props_good, e_good = fn(y, d)
    gen = torch.Generator().manual_seed(3)
    gp = torch.randn(5, 12, generator=gen).to(c.device)
    gp[:, 11] = 0
    ge = torch.randn(5, d.shape[0], generator=gen).to(c.device)
    g, = torch.autograd.grad([props, e], [x], [gp, ge], retain_graph=True)
    g_good, = torch.autograd.grad([props_good, e_good], [y], [gp[keep], ge[keep]])
    sync()
    props, e = props.detach(), e.detach()
    assert props[:, 11].tolist() == [1, 0, 1, 0, 1]
    for b in (1, 3):
        assert bool(torch.isnan(props[b, 2:11]).all()) and bool(torch.isnan(e[b]).all())
    assert bool(torch.isfinite(props[1, :2]).all())
    a = c[1].double().cpu()
    assert abs(float(props[1, 0]) - float(a[:3, :3].sum() / 9)) < 1e-6
    # the good graphs are what they are without the bad ones, rows and gradients
    assert torch.equal(props[keep], props_good) and torch.equal(e[keep], e_good)
    assert torch.equal(g[keep], g_good) and bool(torch.isfinite(g[keep]).all())
    # cotangents on NaN columns give exact zeros: what is left is the Voigt terms' gradient
    voigt = torch.zeros(6, 6, dtype=torch.float64)
    k_v, g_v = float(gp[1, 0]), float(gp[1, 1])
    voigt[:3, :3] = k_v / 9 - g_v / 30
    voigt[range(3), range(3)] = k_v / 9 + g_v / 15
    voigt[range(3, 6), range(3, 6)] = g_v / 10
    assert float((g[1].double().cpu() - voigt).abs().max()) < 1e-6 and bool(torch.isfinite(g).all())
    only_nan = gp.clone()
    only_nan[:, :2] = 0
    g2, = torch.autograd.grad([props_live, e_live], [x], [only_nan, ge])
    sync()
    assert bool((g2[1] == 0).all()) and bool((g2[3] == 0).all())
