"""Shear modulus, Poisson's ratio and linear compressibility surfaces of predicted stiffness
matrices, differentiable in the stiffness: the properties of a pair of orthogonal directions that
``gnn.elastic`` (averages, and ``E`` of one direction) does not have.

For a unit direction ``d`` and a unit ``n`` orthogonal to it, with ``S`` the inverse of the symmetric
part of the Mandel stiffness, ``G(d, n) = 1 / (4 S'_1212)``, ``nu(d, n) = -S'_1122 / S'_1111`` and
``beta(d) = S_ijkk d_i d_j``.  Both ``1 / G`` and ``nu`` are a mean plus one sinusoid in twice the
transverse angle, so their extremes over ``n`` are closed forms (``include/eelg.h`` states them): no
angular search.  ``transverse_properties`` gives, per graph and direction, the row
``TRANSVERSE_DIR_COLUMNS`` (the smallest and largest ``G`` and ``nu`` over the transverse circle and
``beta``), per graph the row ``TRANSVERSE_COLUMNS`` (their extremes over the directions: ``nu_min <
0`` says the lattice is auxetic in some plane), the direction index of each extreme and the
transverse vector ``n`` at which it is taken.  A graph whose matrix is not positive definite has
``spd`` 0 and NaN everywhere else; its NaN entries take cotangents without passing anything on.

On a HIP device it is an ``autograd.Function`` over ``eelg_transverse_props`` and
``eelg_transverse_props_bwd`` (``csrc/eelg_transverse.hip``): one launch each way, no host
synchronisation, bitwise repeatable.  On CPU tensors, or with ``EELG_TRANSVERSE_FUSED=0``, it is
``transverse_properties_composed``, the plain torch form: the second implementation, the timing
baseline and the CPU path.  ``gnn.design.property_sensitivity`` and ``optimize_design`` take
weights on both rows.
"""
from __future__ import annotations

import math
import os
from typing import Tuple

import torch

from . import _lib
from .elastic import _check, _mandel_directions

TRANSVERSE_COLUMNS = ("G_min", "G_max", "nu_min", "nu_max", "beta_min", "beta_max", "spd")
TRANSVERSE_DIR_COLUMNS = ("G_lo", "G_hi", "nu_lo", "nu_hi", "beta")
# column of a direction's row whose extreme is column i of a property row
_SOURCE = (0, 1, 2, 3, 4, 4)
# two fused launches on a HIP device (1), or the composed torch form everywhere (0)
FUSED = os.environ.get("EELG_TRANSVERSE_FUSED", "1") != "0"


def _frame(d: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """``(t1, t2)`` [P, 3]: j the first index of the smallest |d_j|, t1 = normalize(d x e_j),
    t2 = d x t1."""
    ad = d.abs()
    j = torch.zeros(d.shape[0], dtype=torch.long, device=d.device)
    m = ad[:, 0]
    for k in (1, 2):
        less = ad[:, k] < m
        j = torch.where(less, torch.full_like(j, k), j)
        m = torch.where(less, ad[:, k], m)
    e = torch.nn.functional.one_hot(j, 3).to(d.dtype)
    t1 = torch.cross(d, e, dim=1)
    t1 = t1 / t1.norm(dim=1, keepdim=True)
    return t1, torch.cross(d, t1, dim=1)


def _mandel_sym(x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """``[P, 6]``: M(sym(x (x) y))."""
    h = math.sqrt(0.5)
    return torch.stack([x[:, 0] * y[:, 0], x[:, 1] * y[:, 1], x[:, 2] * y[:, 2],
                        h * (x[:, 1] * y[:, 2] + x[:, 2] * y[:, 1]), h * (x[:, 0] * y[:, 2] + x[:, 2] * y[:, 0]),
                        h * (x[:, 0] * y[:, 1] + x[:, 1] * y[:, 0])], dim=-1)


def _hypot(p: torch.Tensor, q: torch.Tensor) -> torch.Tensor:
    """``hypot(p, q)`` whose gradient is ``(p dp + q dq) / R`` and exactly 0 where ``R == 0``
    (``torch.hypot`` gives NaN there)."""
    r = torch.hypot(p, q).detach()
    safe = torch.where(r > 0, r, torch.ones_like(r))
    cp, cq = (p / safe).detach(), (q / safe).detach()
    lin = p * cp + q * cq
    return r + (lin - lin.detach())


def _first_extreme(e: torch.Tensor, largest: bool):
    """The extreme of every row, gathered at its first index (the gradient goes there alone), and
    that index."""
    ext = e.max(dim=1, keepdim=True).values if largest else e.min(dim=1, keepdim=True).values
    first = (e == ext).to(torch.int32).argmax(dim=1, keepdim=True)
    return e.gather(1, first)[:, 0], first[:, 0]


def transverse_properties_composed(c: torch.Tensor, directions: torch.Tensor
                                   ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """``(props [B, 7], t_dir [B, P, 5], arg [B, 6] int32, n_ext [B, 4, 3])`` in ``C``'s dtype, in
    plain torch: ``cholesky_ex`` / ``cholesky_inverse`` as ``elastic_properties_composed``, the six
    quadratic forms as einsums, NaN masking and the first-extreme ``min`` / ``max``.  fp64 inside,
    rounded to ``C``'s dtype at the end.  A graph that is not positive definite is factorised as the
    identity and masked afterwards, so its NaN entries pass no gradient on."""
    _check(c, directions, "transverse_properties_composed")
    if directions is None:
        raise ValueError("transverse_properties_composed: directions [P, 3] are required (P may be 0)")
    dt, dev = c.dtype, c.device
    a = 0.5 * (c.double() + c.double().transpose(1, 2))
    nb, n_dirs = int(a.shape[0]), int(directions.shape[0])
    with torch.no_grad():
        info = torch.linalg.cholesky_ex(a)[1]
        spd = (info == 0) & torch.isfinite(a).all(dim=2).all(dim=1)
    if n_dirs == 0:
        nan = torch.full((nb, 6), float("nan"), dtype=dt, device=dev)
        return (torch.cat([nan, spd.to(dt)[:, None]], dim=1), torch.full((nb, 0, 5), float("nan"), dtype=dt, device=dev),
                torch.full((nb, 6), -1, dtype=torch.int32, device=dev),
                torch.full((nb, 4, 3), float("nan"), dtype=dt, device=dev))
    eye = torch.eye(6, dtype=a.dtype, device=dev)
    safe = torch.where(spd[:, None, None], a, eye)
    s = torch.cholesky_inverse(torch.linalg.cholesky_ex(safe)[0])
    s = 0.5 * (s + s.transpose(1, 2))

    d = directions.detach().double()
    t1, t2 = _frame(d)
    m_a = _mandel_directions(d)
    m_t1, m_t2 = _mandel_sym(d, t1), _mandel_sym(d, t2)
    b1, b2, x = _mandel_sym(t1, t1), _mandel_sym(t2, t2), _mandel_sym(t1, t2)

    def form(u, v):
        return torch.einsum("pi,bij,pj->bp", u, s, v)
    a11, a22, a12 = form(m_t1, m_t1), form(m_t2, m_t2), form(m_t1, m_t2)
    m_g, p_g, q_g = 2.0 * (a11 + a22), a11 - a22, 2.0 * a12
    r_g = 2.0 * _hypot(p_g, q_g)
    u = torch.einsum("bij,pj->bpi", s, m_a)
    young = 1.0 / torch.einsum("bpi,pi->bp", u, m_a)
    bb1, bb2, q_n = (torch.einsum("bpi,pi->bp", u, v) for v in (b1, b2, x))
    m_n, p_n = 0.5 * (bb1 + bb2), 0.5 * (bb1 - bb2)
    r_n = _hypot(p_n, q_n)
    t64 = torch.stack([1.0 / (m_g + r_g), 1.0 / (m_g - r_g), -young * (m_n + r_n), -young * (m_n - r_n),
                       (u[:, :, 0] + u[:, :, 1]) + u[:, :, 2]], dim=2)
    nan = torch.full((), float("nan"), dtype=a.dtype, device=dev)
    # the extremes are those of the values that are returned
    t_dir = torch.where(spd[:, None, None], t64, nan).to(dt)
    cols, args = zip(*(_first_extreme(t_dir[:, :, _SOURCE[i]], bool(i & 1)) for i in range(6)))
    props = torch.stack(list(cols) + [spd.to(dt)], dim=1)
    arg = torch.where(spd[:, None], torch.stack(args, dim=1), torch.full((), -1, dtype=torch.long, device=dev))

    with torch.no_grad():
        normals = []
        for i in range(4):
            at = args[i][:, None]
            p, q = ((p_g, q_g) if i < 2 else (p_n, q_n))
            p, q = p.gather(1, at)[:, 0], q.gather(1, at)[:, 0]
            zero = torch.zeros_like(p)
            th = 0.5 * torch.where(torch.hypot(p, q) == 0, zero, torch.atan2(q, p))
            cs, sn = torch.cos(th), torch.sin(th)
            c1, c2 = (-sn, cs) if i & 1 else (cs, sn)
            normals.append(c1[:, None] * t1[args[i]] + c2[:, None] * t2[args[i]])
        n_ext = torch.where(spd[:, None, None], torch.stack(normals, dim=1), nan).to(dt)
    return props, t_dir, arg.to(torch.int32), n_ext


class _TransverseProps(torch.autograd.Function):
    @staticmethod
    def forward(ctx, c, directions):
        nb, n_dirs = int(c.shape[0]), int(directions.shape[0])
        c32 = c.detach().to(torch.float32).contiguous()
        d32 = directions.detach().to(torch.float32).contiguous() if n_dirs else None
        dev = c.device
        props = torch.empty((nb, len(TRANSVERSE_COLUMNS)), dtype=torch.float32, device=dev)
        t_dir = torch.empty((nb, n_dirs, len(TRANSVERSE_DIR_COLUMNS)), dtype=torch.float32, device=dev)
        arg = torch.empty((nb, 6), dtype=torch.int32, device=dev)
        n_ext = torch.empty((nb, 4, 3), dtype=torch.float32, device=dev)
        s = torch.empty((nb, 21), dtype=torch.float64, device=dev)
        with torch.cuda.device(dev):
            _lib.launch("transverse_props", _lib.load().eelg_transverse_props, c32, d32, nb, n_dirs, props,
                         t_dir if n_dirs else None, arg, n_ext, s, on=c32, timed="transverse_props")
        ctx.save_for_backward(s, d32, props, arg)
        ctx.in_dtype = c.dtype
        ctx.n_dirs = n_dirs
        ctx.mark_non_differentiable(arg, n_ext)
        return props, t_dir, arg, n_ext

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_props, g_t_dir, _g_arg, _g_n_ext):
        s, d32, props, arg = ctx.saved_tensors
        nb, n_dirs = int(props.shape[0]), ctx.n_dirs
        if g_props is None:
            g_props = torch.zeros_like(props)
        g_props = g_props.to(torch.float32).contiguous()
        if g_t_dir is not None:
            g_t_dir = g_t_dir.to(torch.float32).contiguous()
        g_c = torch.empty((nb, 6, 6), dtype=torch.float32, device=s.device)
        with torch.cuda.device(s.device):
            _lib.launch("transverse_props_bwd", _lib.load().eelg_transverse_props_bwd, s, d32, props, arg, g_props,
                         g_t_dir if n_dirs else None, nb, n_dirs, g_c, on=s, timed="transverse_props_bwd")
        return g_c.to(ctx.in_dtype), None


def transverse_properties(c: torch.Tensor, directions: torch.Tensor
                          ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """``(props [B, 7], t_dir [B, P, 5], arg [B, 6] int32, n_ext [B, 4, 3])`` of the Mandel
    stiffness ``C`` ``[B, 6, 6]`` over the unit ``directions`` ``[P, 3]``: the rows
    ``TRANSVERSE_COLUMNS`` and ``TRANSVERSE_DIR_COLUMNS``, the direction index of ``G_min, G_max,
    nu_min, nu_max, beta_min, beta_max`` (the first on a tie; -1 where the extreme is NaN) and the
    transverse unit vector at which the first four are taken (defined up to its sign).
    Differentiable in ``C`` through ``props`` and ``t_dir`` (the gradient is symmetric; the ``spd``
    column has none); ``arg``, ``n_ext`` and ``directions`` carry no gradient.  P = 0: ``t_dir`` is
    ``[B, 0, 5]`` and the extremes are NaN.  On a HIP tensor the results are fp32 (two fused launches
    on the tensor's device and current stream); the composed form returns ``C``'s dtype."""
    _check(c, directions, "transverse_properties")
    if directions is None:
        raise ValueError("transverse_properties: directions [P, 3] are required (P may be 0)")
    if not (FUSED and c.is_cuda):
        return transverse_properties_composed(c, directions)
    return _TransverseProps.apply(c, directions)
