"""The yardstick of the geometry-gradient tests (tests/test_gpu_geometry.py): autograd of the
fp64 CPU oracle w.r.t. node positions, strut radii and periodic shifts, checked here against
finite differences and the invariances it must have.  No GPU.

Bounds: a central difference with eps = 1e-5 in fp64 has truncation error O(eps^2) = 1e-10
relative and rounding error ~ 1e-16 / eps = 1e-11 of the loss, so 1e-6 relative on the
directional derivative is loose by two orders (measured 5e-9); the invariances are exact up to
fp64 summation (1e-12; measured 2e-15)."""
import torch

from helpers import batch, batch_to, params

import oracle.model as omodel
from oracle.train import stiffness_loss as oracle_loss


def _setup():
    b, rmax = batch(2, 12, 48, seed=7)
    torch.manual_seed(0)
    o = omodel.EnergyEquivGNN(params(2, lmax=2, correlation=2, max_edge_radius=rmax)).double()
    return o, batch_to(b, "cpu", torch.float64)


def _loss(o, bo):
    return oracle_loss(o(bo)["stiffness"], bo.stiffness)


def _grads(o, bo):
    for k in ("positions", "edge_attr", "shifts"):
        setattr(bo, k, getattr(bo, k).detach().clone().requires_grad_(True))
    gp, gr, gs = torch.autograd.grad(_loss(o, bo), [bo.positions, bo.edge_attr, bo.shifts])
    for k in ("positions", "edge_attr", "shifts"):
        setattr(bo, k, getattr(bo, k).detach())
    return gp, gr, gs


def test_oracle_geometry_gradients_match_finite_differences():
    o, bo = _setup()
    gp, gr, _ = _grads(o, bo)
    g = torch.Generator().manual_seed(3)
    eps = 1e-5
    for key, grad in (("positions", gp), ("edge_attr", gr)):
        base = getattr(bo, key)
        d = torch.randn(base.shape, generator=g, dtype=torch.float64)
        d /= d.norm()
        with torch.no_grad():
            setattr(bo, key, base + eps * d)
            lp = _loss(o, bo).item()
            setattr(bo, key, base - eps * d)
            lm = _loss(o, bo).item()
            setattr(bo, key, base)
        fd = (lp - lm) / (2 * eps)
        ad = float((grad * d).sum())
        print(f"{key}: autograd {ad:.12e} central difference {fd:.12e} rel {abs(fd - ad) / abs(ad):.2e}")
        assert abs(fd - ad) <= 1e-6 * abs(ad), key


def test_oracle_position_gradient_is_translation_invariant_and_the_scatter_of_the_shift_gradient():
    o, bo = _setup()
    gp, _, gs = _grads(o, bo)
    per_graph = torch.zeros(bo.num_graphs, 3, dtype=torch.float64).index_add_(0, bo.batch, gp)
    print("per-graph sum / max:", float(per_graph.abs().max() / gp.abs().max()))
    assert per_graph.abs().max() <= 1e-12 * gp.abs().max()
    send, recv = bo.edge_index
    scat = torch.zeros_like(gp).index_add_(0, recv, gs).index_add_(0, send, -gs)
    assert (gp - scat).abs().max() <= 1e-12 * gp.abs().max()
