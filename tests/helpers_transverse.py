"""Rank-4 restatement of the transverse elastic surfaces (``gnn.transverse``), the brute-force scan
that validates the closed forms, and the cases and error measures the transverse tests share.

With the cartesian rank-4 compliance S (``helpers_mandel.mandel_to_cart4`` of ``torch.linalg.inv``),
a direction d and n = cos(th) t1 + sin(th) t2 in a frame (t1, t2) built here by Gram-Schmidt (not
by the cross products of the code under test):
    1 / G(d, n) = 4 S'_1212 = 4 S_ijkl d_i n_j d_k n_l,  nu(d, n) = -S'_1122 / S'_1111,
    beta(d) = S_ijkk d_i d_j.
``reference`` takes the extremes over th from the mean and amplitude of the sinusoid in 2 th;
``scan`` evaluates the same two expressions on K angles and takes the extremes it finds.  Run in fp64
``reference`` is the truth, run in fp32 on the CPU the baseline of the bounds.  Nothing here imports
``gnn.transverse``: the shared checks take the implementation as an argument."""
from __future__ import annotations

import math
from typing import Dict

import numpy as np
import torch

from helpers_elastic import spd_set                            # noqa: F401  (re-exported)
from helpers_mandel import mandel_to_cart4
from helpers_metrics import hostile_set

COLUMNS = ("G_min", "G_max", "nu_min", "nu_max", "beta_min", "beta_max", "spd")
DIR_COLUMNS = ("G_lo", "G_hi", "nu_lo", "nu_hi", "beta")
SOURCE = (0, 1, 2, 3, 4, 4)          # column of t_dir whose extreme is column i of props
EXCLUDE = 1e-9                       # pairs with R_G <= EXCLUDE M_G or R_nu E <= EXCLUDE: no gradient / n_ext check
TIE = 1e-6                           # extremes whose two best directions lie this close: no cotangent


def crystal_directions() -> torch.Tensor:
    """[26, 3] fp64 unit vectors: the 3 axes, the 6 face diagonals and the 4 body diagonals of the
    cube, each followed by its negative (axes: two zero components tie for the frame's axis; body
    diagonals: all three tie)."""
    rows = []
    for v in ([1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 0], [1, -1, 0], [1, 0, 1], [1, 0, -1], [0, 1, 1], [0, 1, -1],
              [1, 1, 1], [1, 1, -1], [1, -1, 1], [-1, 1, 1]):
        rows += [v, [-x for x in v]]
    d = torch.tensor(rows, dtype=torch.float64)
    return d / d.norm(dim=1, keepdim=True)


def _own_frame(d: torch.Tensor):
    """Gram-Schmidt on the axis d has least of: u = normalize(e_k - (e_k . d) d / |d|^2), and v =
    normalize(d x u).  Returned as (v, |d| u): the directions are given in fp32 and so are unit to 6e-8
    only, and the functions are defined (``include/eelg.h``) on the transverse vectors cos(th) t1 +
    sin(th) t2 with |t1| = 1 and |t2| = |d|, an ellipse with its long axis in the plane of d and e_k.
    A frame with other lengths changes A11 - A22 by 1e-7 of M_G, more than the whole anisotropy of
    the nearly isotropic matrix of the set."""
    k = d.abs().argmin(dim=1)
    e = torch.nn.functional.one_hot(k, 3).to(d.dtype)
    u = e - (e * d).sum(dim=1, keepdim=True) * d / (d * d).sum(dim=1, keepdim=True)
    u = u / u.norm(dim=1, keepdim=True)
    v = torch.cross(d, u, dim=1)
    return v / v.norm(dim=1, keepdim=True), d.norm(dim=1, keepdim=True) * u


def _amplitude(p, q):
    """sqrt(p^2 + q^2) with a zero gradient where it is zero."""
    x = p * p + q * q
    pos = x > 0
    return torch.where(pos, torch.sqrt(torch.where(pos, x, torch.ones_like(x))), torch.zeros_like(x))


def reference(c: torch.Tensor, dirs: torch.Tensor, dtype=torch.float64) -> Dict[str, torch.Tensor]:
    """``props`` [B, 7], ``t_dir`` [B, P, 5], ``arg`` [B, 6], ``normals`` [B, P, 4, 3] (the transverse
    vector of G_lo, G_hi, nu_lo, nu_hi of every pair) and the two degeneracy measures ``ratio_g`` =
    R_G / M_G and ``ratio_nu`` = R_nu E [B, P], all computed in ``dtype``; differentiable in ``c``."""
    c, d = c.to(dtype), dirs.to(dtype)
    a = 0.5 * (c + c.transpose(1, 2))
    s4 = mandel_to_cart4(torch.linalg.inv(a))
    nb, n_dirs = c.shape[0], d.shape[0]
    spd = (torch.linalg.eigvalsh(a.detach().double()).min(dim=1).values > 0).to(dtype)
    if n_dirs == 0:
        nan = c.new_full((nb, 6), float("nan"))
        return dict(props=torch.cat([nan, spd[:, None]], dim=1), t_dir=c.new_zeros((nb, 0, 5)),
                    arg=torch.full((nb, 6), -1, dtype=torch.long), normals=c.new_zeros((nb, 0, 4, 3)),
                    ratio_g=c.new_zeros((nb, 0)), ratio_nu=c.new_zeros((nb, 0)))
    t1, t2 = _own_frame(d)
    q11 = torch.einsum("bijkl,pi,pj,pk,pl->bp", s4, d, t1, d, t1)
    q22 = torch.einsum("bijkl,pi,pj,pk,pl->bp", s4, d, t2, d, t2)
    q12 = torch.einsum("bijkl,pi,pj,pk,pl->bp", s4, d, t1, d, t2)
    p11 = torch.einsum("bijkl,pi,pj,pk,pl->bp", s4, d, d, t1, t1)
    p22 = torch.einsum("bijkl,pi,pj,pk,pl->bp", s4, d, d, t2, t2)
    p12 = torch.einsum("bijkl,pi,pj,pk,pl->bp", s4, d, d, t1, t2)
    s1111 = torch.einsum("bijkl,pi,pj,pk,pl->bp", s4, d, d, d, d)
    mean_g, amp_g = 2 * (q11 + q22), 2 * _amplitude(q11 - q22, 2 * q12)           # of 1 / G
    mean_n, amp_n = (p11 + p22) / 2, _amplitude((p11 - p22) / 2, p12)             # of S'_1122
    beta = torch.einsum("bijkk,pi,pj->bp", s4, d, d)
    t_dir = torch.stack([1 / (mean_g + amp_g), 1 / (mean_g - amp_g), -(mean_n + amp_n) / s1111,
                         -(mean_n - amp_n) / s1111, beta], dim=2)
    cols, args = [], []
    for i in range(6):
        col = t_dir[:, :, SOURCE[i]]
        at = col.detach().argmax(dim=1) if i & 1 else col.detach().argmin(dim=1)
        cols.append(col.gather(1, at[:, None])[:, 0])
        args.append(at)
    with torch.no_grad():
        normals = []
        for phase in (torch.atan2(2 * q12, q11 - q22), torch.atan2(p12, (p11 - p22) / 2)):
            for shift in (0.0, math.pi / 2):
                th = (0.5 * phase + shift)[:, :, None]
                normals.append(torch.cos(th) * t1[None] + torch.sin(th) * t2[None])
        normals = torch.stack(normals, dim=2)
    return dict(props=torch.stack(cols + [spd], dim=1), t_dir=t_dir, arg=torch.stack(args, dim=1), normals=normals,
                ratio_g=(amp_g / mean_g).detach(), ratio_nu=(amp_n / s1111).detach())


def scan(c: torch.Tensor, dirs: torch.Tensor, k: int = 32768) -> Dict[str, torch.Tensor]:
    """Brute force in fp64: 4 S'_1212 and -S'_1122 / S'_1111 on the ``k`` transverse angles th = pi q / k
    (both have period pi in th), their smallest and largest value per (matrix, direction) [B, P]:
    ``inv_g_min, inv_g_max, nu_min, nu_max``."""
    c, d = c.double(), dirs.double()
    s4 = mandel_to_cart4(torch.linalg.inv(0.5 * (c + c.transpose(1, 2))))
    t1, t2 = _own_frame(d)
    th = math.pi * torch.arange(k, dtype=torch.float64) / k
    n = torch.cos(th)[None, :, None] * t1[:, None] + torch.sin(th)[None, :, None] * t2[:, None]       # [P, k, 3]
    out = {key: [] for key in ("inv_g_min", "inv_g_max", "nu_min", "nu_max")}
    for b in range(c.shape[0]):
        shear = torch.einsum("ijkl,pi,pk->pjl", s4[b], d, d)
        lateral = torch.einsum("ijkl,pi,pj->pkl", s4[b], d, d)
        s1111 = torch.einsum("pkl,pk,pl->p", lateral, d, d)
        inv_g = 4 * torch.einsum("pjl,pqj,pql->pq", shear, n, n)
        nu = -torch.einsum("pkl,pqk,pql->pq", lateral, n, n) / s1111[:, None]
        out["inv_g_min"].append(inv_g.min(dim=1).values)
        out["inv_g_max"].append(inv_g.max(dim=1).values)
        out["nu_min"].append(nu.min(dim=1).values)
        out["nu_max"].append(nu.max(dim=1).values)
    return {key: torch.stack(v) for key, v in out.items()}


def excluded(ref: Dict[str, torch.Tensor]) -> torch.Tensor:
    """[B, P] bool: the pairs whose fp64 R_G <= 1e-9 M_G or R_nu E <= 1e-9, where the direction of the
    hypot's gradient and the transverse vector are rounding noise."""
    return (ref["ratio_g"] <= EXCLUDE) | (ref["ratio_nu"] <= EXCLUDE)


def _scales(ref: Dict[str, torch.Tensor]):
    """Per graph what an error is taken relative to: a G entry to its own fp64 value, a nu entry to 1
    (absolute: nu crosses zero), a beta entry to the graph's largest |beta| (beta may cross zero)."""
    t = ref["t_dir"].detach().double()
    big_beta = t[:, :, 4].abs().amax(dim=1, keepdim=True).expand(-1, t.shape[1])
    st = torch.stack([t[:, :, 0], t[:, :, 1], torch.ones_like(big_beta), torch.ones_like(big_beta), big_beta], dim=2).abs()
    p = ref["props"].detach().double()
    sp = torch.stack([p[:, 0], p[:, 1], torch.ones_like(p[:, 0]), torch.ones_like(p[:, 0]), big_beta[:, 0], big_beta[:, 0]],
                     dim=1).abs()
    return sp, st


def errors(props: torch.Tensor, t_dir: torch.Tensor, ref: Dict[str, torch.Tensor]) -> Dict[str, float]:
    """Per column of ``props`` and of ``t_dir`` the largest error over the set, normalised as
    ``_scales`` says."""
    sp, st = _scales(ref)
    p, t = props.detach().double().cpu(), t_dir.detach().double().cpu()
    rp, rt = ref["props"].detach().double(), ref["t_dir"].detach().double()
    out = {name: float(((p[:, i] - rp[:, i]).abs() / sp[:, i]).max()) for i, name in enumerate(COLUMNS[:6])}
    out.update({name: float(((t[:, :, i] - rt[:, :, i]).abs() / st[:, :, i]).max()) for i, name in enumerate(DIR_COLUMNS)})
    return out


def bounds(base: Dict[str, float], ref: Dict[str, torch.Tensor]) -> Dict[str, float]:
    """4x the baseline's error, at least 4 fp32 ulps of the column's largest (normalised) magnitude:
    1 for the G and beta columns, the largest |nu| for the nu columns."""
    sp, st = _scales(ref)
    rp, rt = ref["props"].detach().double(), ref["t_dir"].detach().double()
    out = {}
    for i, name in enumerate(COLUMNS[:6]):
        top = np.float32((rp[:, i].abs() / sp[:, i]).max())
        out[name] = max(4.0 * base[name], 4.0 * float(np.spacing(top)))
    for i, name in enumerate(DIR_COLUMNS):
        top = np.float32((rt[:, :, i].abs() / st[:, :, i]).max())
        out[name] = max(4.0 * base[name], 4.0 * float(np.spacing(top)))
    return out


def cotangents(ref: Dict[str, torch.Tensor], seed: int = 5, keep_excluded: bool = False):
    """``(g_props [B, 7], g_t_dir [B, P, 5])`` fp64: ``randn`` from a fixed CPU generator divided by the
    scale of ``_scales`` (``t_dir``: and by P), so that every column weighs alike.  Zero on ``spd``;
    unless ``keep_excluded``, zero on the excluded pairs, on an extreme taken at an excluded pair, and
    on an extreme whose two best directions lie within ``TIE`` of each other in fp64 (which of them is
    first is decided by the rounding of the fp32 values, and the gradient goes to one alone)."""
    gen = torch.Generator().manual_seed(seed)
    sp, st = _scales(ref)
    nb, n_dirs = st.shape[0], st.shape[1]
    gp = torch.zeros(nb, 7, dtype=torch.float64)
    gp[:, :6] = torch.randn(nb, 6, generator=gen, dtype=torch.float64) / sp
    gt = torch.randn(nb, n_dirs, 5, generator=gen, dtype=torch.float64) / (st * max(n_dirs, 1))
    if keep_excluded:
        return gp, gt
    out = excluded(ref)
    gt[out] = 0
    t = ref["t_dir"].detach().double()
    for i in range(6):
        col = t[:, :, SOURCE[i]]
        at = ref["arg"][:, i]
        gp[out.gather(1, at[:, None])[:, 0], i] = 0
        if n_dirs > 1:
            best = torch.sort(col, dim=1, descending=bool(i & 1)).values
            gp[(best[:, 0] - best[:, 1]).abs() <= TIE * sp[:, i], i] = 0
    return gp, gt


def gradient(fn, c: torch.Tensor, dirs: torch.Tensor, g_props: torch.Tensor, g_t_dir: torch.Tensor) -> torch.Tensor:
    """Gradient of ``sum(g_props * props) + sum(g_t_dir * t_dir)`` of ``fn(c, dirs)`` w.r.t. ``c``; ``fn``
    returns ``(props, t_dir, ...)``."""
    x = c.detach().clone().requires_grad_(True)
    props, t_dir = fn(x, dirs)[:2]
    outs, gs = [props], [g_props.to(device=props.device, dtype=props.dtype)]
    if t_dir.shape[1]:
        outs.append(t_dir)
        gs.append(g_t_dir.to(device=t_dir.device, dtype=t_dir.dtype))
    return torch.autograd.grad(outs, [x], gs)[0]


def reference_fn(dtype):
    """``reference`` as an ``fn(c, dirs)`` for ``gradient``."""
    def fn(c, dirs):
        r = reference(c, dirs, dtype)
        return r["props"], r["t_dir"]
    return fn


def gradient_error(g: torch.Tensor, ref: torch.Tensor) -> torch.Tensor:
    """[B]: for each matrix the largest error relative to that matrix's largest fp64 gradient entry.
    The bounds are taken matrix by matrix: the fp32 baseline loses the nearly isotropic matrix's
    gradient altogether (the unit vector of its hypot is rounding noise in fp32), and a bound from the
    set's largest baseline error would check nothing."""
    g, ref = g.detach().double().cpu(), ref.detach().double().cpu()
    return (g - ref).abs().amax(dim=(1, 2)) / ref.abs().amax(dim=(1, 2))


def within(err: torch.Tensor, base: torch.Tensor, floor: float = 4 * 2.0 ** -23) -> bool:
    """Matrix by matrix: at most 4x the baseline, at least 4 fp32 ulps of 1 allowed."""
    return bool((err <= torch.clamp(4 * base, min=floor)).all())


def normal_error(n_ext: torch.Tensor, arg: torch.Tensor, ref: Dict[str, torch.Tensor]) -> torch.Tensor:
    """[B]: the largest distance, up to the sign of the vector, between ``n_ext`` [B, 4, 3] and the fp64
    transverse vector (normalised) of the pair ``arg`` names, over the pairs that are not excluded."""
    n, at = n_ext.detach().double().cpu(), arg.detach().long().cpu()
    out, worst = excluded(ref), torch.zeros(n.shape[0], dtype=torch.float64)
    for b in range(n.shape[0]):
        for i in range(4):
            p = int(at[b, i])
            if out[b, p]:
                continue
            want = ref["normals"][b, p, i].double()
            want = want / want.norm()
            worst[b] = max(float(worst[b]), float(torch.minimum((n[b, i] - want).norm(), (n[b, i] + want).norm())))
    return worst


# ---- cases and assertions shared by the CPU and the device tests (``fn`` is the implementation) ----
def bad_batch():
    """SPD matrices 0, 11, 16, 2 of the set with, between them, the indefinite matrix of the hostile
    set, an all-NaN matrix and a matrix with an infinite entry; (batch, positions of the good graphs,
    their matrices)."""
    good = spd_set()[[0, 11, 16, 2]]
    inf = spd_set()[3].clone()
    inf[2, 2] = float("inf")
    c = torch.stack([good[0], hostile_set()[7], good[1], torch.full((6, 6), float("nan")), good[2], inf, good[3]])
    return c, [0, 2, 4, 6], good


def check_bad_batch(fn, c, keep, good, d, sync=lambda: None):
    """Bad rows are NaN with ``spd`` 0 and ``arg`` -1 and pass exactly zero back whatever their
    cotangents; the good rows and their gradients are bitwise what they are alone."""
    bad = [b for b in range(c.shape[0]) if b not in keep]
    x = c.clone().requires_grad_(True)
    props, t_dir, arg, n_ext = fn(x, d)
    y = good.clone().requires_grad_(True)
    alone = fn(y, d)
    gen = torch.Generator().manual_seed(3)
    gp = torch.randn(c.shape[0], 7, generator=gen).to(c.device)
    gt = torch.randn(c.shape[0], d.shape[0], 5, generator=gen).to(c.device)
    g, = torch.autograd.grad([props, t_dir], [x], [gp, gt], retain_graph=True)
    g_alone, = torch.autograd.grad([alone[0], alone[1]], [y], [gp[keep], gt[keep]])
    poison = gp.clone()
    poison[bad] = float("nan")
    g2, = torch.autograd.grad([props, t_dir], [x], [poison, gt])
    sync()
    assert props[:, 6].tolist() == [1.0 if b in keep else 0.0 for b in range(c.shape[0])]
    for b in bad:
        assert bool(torch.isnan(props[b, :6]).all()) and bool(torch.isnan(t_dir[b]).all())
        assert bool(torch.isnan(n_ext[b]).all()) and arg[b].tolist() == [-1] * 6
        assert bool((g[b] == 0).all()) and bool((g2[b] == 0).all())
    for got, want in zip((props, t_dir, arg, n_ext), alone):
        assert torch.equal(got.detach()[keep], want.detach())
    assert torch.equal(g[keep], g_alone) and torch.equal(g2[keep], g_alone) and bool(torch.isfinite(g).all())


def tie_case():
    """The cubic matrix (2, 1.6, 0.3) with 72 random directions in which index 70 repeats index 3 and
    index 71 is its negative, and cotangents that single out the six extremes: the extremes that fall
    on the repeated direction must name index 3 and send their gradient there alone."""
    from helpers_elastic import cubic
    from helpers_metrics import directions
    d = directions(72).clone()
    d[3] = torch.tensor([1.0, 1.0, 0.0]) / math.sqrt(2.0)         # G_min, nu_min and nu_max of this matrix
    d[70] = d[3]
    d[71] = -d[3]
    return torch.from_numpy(cubic(2.0, 1.6, 0.3)).float()[None], d


def check_tie(fn, c, d):
    x = c.clone().requires_grad_(True)
    props, t_dir, arg, _ = fn(x, d)
    assert torch.equal(t_dir[0, 3], t_dir[0, 70]) and torch.equal(t_dir[0, 3], t_dir[0, 71])
    # (beta of a cubic matrix is the same in every direction: its extremes are left to rounding)
    hit = [i for i in range(4) if float(props[0, i]) == float(t_dir[0, 3, SOURCE[i]])]
    assert {0, 2} <= set(hit), (hit, props)           # G_min = 0.2 and nu_min of [110] are global extremes
    for i in hit:
        assert int(arg[0, i]) == 3, (i, arg)
        g_ext, = torch.autograd.grad(props[0, i], x, retain_graph=True)
        g_dir, = torch.autograd.grad(t_dir[0, 3, SOURCE[i]], x, retain_graph=True)
        assert torch.equal(g_ext, g_dir) and float(g_ext.abs().max()) > 0
