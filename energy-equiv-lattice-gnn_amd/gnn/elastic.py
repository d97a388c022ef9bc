"""Elastic properties of predicted stiffness matrices, differentiable in the stiffness.

``elastic_properties`` gives, per graph, the row ``ELASTIC_COLUMNS`` (the Voigt / Reuss / Hill bulk
and shear moduli, the Hill Young's modulus and Poisson's ratio, the universal anisotropy index, the
extremes of the directional Young's modulus and the positive-definiteness flag) and the directional
Young's modulus ``E(d) = 1 / (m(d)^T S m(d))`` over a set of unit directions, ``S`` the inverse of
the symmetric part of the Mandel stiffness (``include/eelg.h`` states every formula).  A graph whose
matrix is not positive definite has ``spd`` 0, ``K_V`` and ``G_V``, and NaN everywhere else; its NaN
entries take cotangents without passing anything on, so it cannot poison the batch's gradient.

On a HIP device it is an ``autograd.Function`` over ``eelg_elastic_props`` and
``eelg_elastic_props_bwd`` (``csrc/eelg_elastic.hip``): one launch each way, no rank-4 tensor, no
solver-library call, no host synchronisation, bitwise repeatable.  On CPU tensors, or with
``EELG_ELASTIC_FUSED=0``, it is ``elastic_properties_composed``, the plain torch form: the second
implementation, the timing baseline and the CPU path.  With ``gnn.design.property_sensitivity`` the
gradient continues to node positions and strut radii.
"""
from __future__ import annotations

import math
import os
from typing import Optional, Tuple

import torch

from . import _lib

ELASTIC_COLUMNS = ("K_V", "G_V", "K_R", "G_R", "K_H", "G_H", "E_H", "nu_H", "A_U", "E_min", "E_max", "spd")
# two fused launches on a HIP device (1), or the composed torch form everywhere (0)
FUSED = os.environ.get("EELG_ELASTIC_FUSED", "1") != "0"


def _mandel_directions(directions: torch.Tensor) -> torch.Tensor:
    """``[P, 6]``: m(d) = (d1^2, d2^2, d3^2, r2 d2 d3, r2 d1 d3, r2 d1 d2)."""
    d1, d2, d3 = directions.unbind(-1)
    r2 = math.sqrt(2.0)
    return torch.stack([d1 * d1, d2 * d2, d3 * d3, r2 * d2 * d3, r2 * d1 * d3, r2 * d1 * d2], dim=-1)


def _abc(m: torch.Tensor):
    a = m[:, 0, 0] + m[:, 1, 1] + m[:, 2, 2]
    b = m[:, 1, 0] + m[:, 2, 0] + m[:, 2, 1]
    c = m[:, 3, 3] + m[:, 4, 4] + m[:, 5, 5]
    return a, b, c


def _first_extreme(e: torch.Tensor, largest: bool) -> torch.Tensor:
    """The extreme of every row, gathered at its first index (the gradient goes there alone)."""
    ext = e.max(dim=1, keepdim=True).values if largest else e.min(dim=1, keepdim=True).values
    first = (e == ext).to(torch.int32).argmax(dim=1, keepdim=True)
    return e.gather(1, first)[:, 0]


def _check(c: torch.Tensor, directions: Optional[torch.Tensor], who: str) -> None:
    if c.dim() != 3 or tuple(c.shape[1:]) != (6, 6):
        raise ValueError(f"{who}: C {tuple(c.shape)}, expected [B, 6, 6]")
    if not c.is_floating_point():
        raise ValueError(f"{who}: C must be a floating-point tensor, got {c.dtype}")
    if directions is not None:
        if directions.dim() != 2 or directions.shape[1] != 3:
            raise ValueError(f"{who}: directions {tuple(directions.shape)}, expected [P, 3]")
        if directions.device != c.device:
            raise ValueError(f"{who}: C and directions must share a device")


def elastic_properties_composed(c: torch.Tensor, directions: Optional[torch.Tensor] = None
                                ) -> Tuple[torch.Tensor, torch.Tensor]:
    """``(props [B, 12], e_dir [B, P])`` in ``C``'s dtype, in plain torch: ``cholesky_ex`` for the
    flag, ``cholesky_inverse``, the Mandel contractions, NaN masking and the first-extreme ``min`` /
    ``max``.  Like the kernel it works in fp64 inside (an fp32 Cholesky inverse loses several times
    what LAPACK's fp32 inverse does on the compliance) and rounds the results to ``C``'s dtype.  A
    graph that is not positive definite is factorised as the identity and masked afterwards, so
    its NaN entries pass no gradient on."""
    _check(c, directions, "elastic_properties_composed")
    dt = c.dtype
    a = 0.5 * (c.double() + c.double().transpose(1, 2))
    nb = int(a.shape[0])
    with torch.no_grad():
        info = torch.linalg.cholesky_ex(a)[1]
        spd = (info == 0) & torch.isfinite(a).all(dim=2).all(dim=1)
    eye = torch.eye(6, dtype=a.dtype, device=a.device)
    safe = torch.where(spd[:, None, None], a, eye)
    s = torch.cholesky_inverse(torch.linalg.cholesky_ex(safe)[0])
    s = 0.5 * (s + s.transpose(1, 2))
    sa, sb, sc = _abc(s)

    def voigt(m):
        ca, cb, cc = _abc(m)
        return (ca + 2.0 * cb) / 9.0, (ca - cb + 1.5 * cc) / 15.0
    kv_out, gv_out = voigt(a)
    # the Hill columns and A_U take the Voigt pair of the matrix that was factorised: a NaN K_V
    # would turn the zero cotangent of a masked column into NaN on its way back
    kv, gv = voigt(safe)
    kr = 1.0 / (sa + 2.0 * sb)
    gr = 15.0 / (4.0 * sa - 4.0 * sb + 6.0 * sc)
    kh, gh = 0.5 * (kv + kr), 0.5 * (gv + gr)
    den = 3.0 * kh + gh
    eh = 9.0 * kh * gh / den
    nu = (3.0 * kh - 2.0 * gh) / (2.0 * den)
    au = 5.0 * gv / gr + kv / kr - 6.0
    nan = torch.full((), float("nan"), dtype=a.dtype, device=a.device)
    n_dirs = 0 if directions is None else int(directions.shape[0])
    if n_dirs:
        m = _mandel_directions(directions.detach().double())
        e = 1.0 / torch.einsum("pi,bij,pj->bp", m, s, m)
        # the extremes are those of the values that are returned
        e = torch.where(spd[:, None], e, nan).to(dt)
        emin, emax = _first_extreme(e, False), _first_extreme(e, True)
    else:
        e = torch.full((nb, 0), float("nan"), dtype=dt, device=a.device)
        emin = emax = torch.full((nb,), float("nan"), dtype=dt, device=a.device)
    masked = [torch.where(spd, v, nan) for v in (kr, gr, kh, gh, eh, nu, au)]
    props = torch.stack([kv_out.to(dt), gv_out.to(dt)] + [v.to(dt) for v in masked] + [emin, emax, spd.to(dt)], dim=1)
    return props, e


class _ElasticProps(torch.autograd.Function):
    @staticmethod
    def forward(ctx, c, directions):
        nb = int(c.shape[0])
        n_dirs = 0 if directions is None else int(directions.shape[0])
        c32 = c.detach().to(torch.float32).contiguous()
        d32 = directions.detach().to(torch.float32).contiguous() if n_dirs else None
        props = torch.empty((nb, len(ELASTIC_COLUMNS)), dtype=torch.float32, device=c.device)
        e_dir = torch.empty((nb, n_dirs), dtype=torch.float32, device=c.device)
        s = torch.empty((nb, 6, 6), dtype=torch.float32, device=c.device)
        with torch.cuda.device(c.device):
            _lib.launch("elastic_props", _lib.load().eelg_elastic_props, c32, d32, nb, n_dirs, props,
                         e_dir if n_dirs else None, s, on=c32, timed="elastic_props")
        ctx.save_for_backward(s, d32, e_dir, props)
        ctx.in_dtype = c.dtype
        return props, e_dir

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_props, g_e_dir):
        s, d32, e_dir, props = ctx.saved_tensors
        nb, n_dirs = int(e_dir.shape[0]), int(e_dir.shape[1])
        if g_props is None:
            g_props = torch.zeros_like(props)
        g_props = g_props.to(torch.float32).contiguous()
        if g_e_dir is not None:
            g_e_dir = g_e_dir.to(torch.float32).contiguous()
        g_c = torch.empty((nb, 6, 6), dtype=torch.float32, device=s.device)
        with torch.cuda.device(s.device):
            _lib.launch("elastic_props_bwd", _lib.load().eelg_elastic_props_bwd, s, d32,
                         e_dir if n_dirs else None, props, g_props, g_e_dir if n_dirs else None, nb, n_dirs, g_c,
                         on=s, timed="elastic_props_bwd")
        return g_c.to(ctx.in_dtype), None


def elastic_properties(c: torch.Tensor, directions: Optional[torch.Tensor] = None
                       ) -> Tuple[torch.Tensor, torch.Tensor]:
    """``(props [B, 12], e_dir [B, P])``: the rows ``ELASTIC_COLUMNS`` of the Mandel stiffness ``C``
    ``[B, 6, 6]`` and its Young's modulus along the unit ``directions`` ``[P, 3]``.  Differentiable
    in ``C`` (the gradient is symmetric; the ``spd`` column has none); ``directions`` are constants.
    ``directions=None``: P = 0, ``e_dir`` is ``[B, 0]`` and ``E_min`` / ``E_max`` are NaN.  On a
    HIP tensor the results are fp32 (two fused launches on the tensor's device and current stream);
    the composed form returns ``C``'s dtype."""
    _check(c, directions, "elastic_properties")
    if not (FUSED and c.is_cuda):
        return elastic_properties_composed(c, directions)
    return _ElasticProps.apply(c, directions)
