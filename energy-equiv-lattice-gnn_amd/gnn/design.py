"""Design sensitivities of the stiffness surrogate: gradients of the predicted 6 x 6 stiffness
w.r.t. the lattice geometry (node positions, strut radii, periodic shifts).

The gradients run on the HIP backward path of the model (``eelg_tp_bwd_sh``,
``eelg_radial_bwd_x``, ``eelg_edge_embed_bwd`` and the kernels the training backward uses);
they are deterministic (no atomics) and fp32.  Second derivatives are not built.
"""
from __future__ import annotations

import copy
from typing import Dict, Optional

import torch

GEOMETRY_KEYS = ("positions", "edge_attr", "shifts")


def stiffness_sensitivity(model, batch, cotangent: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
    """``{'stiffness', 'positions', 'edge_attr', 'shifts'}``: the model's stiffness [B, 6, 6]
    (detached) and the gradients of ``sum(cotangent * stiffness)`` w.r.t. ``batch.positions``
    [N, 3], ``batch.edge_attr`` [E, 1] (strut radii) and ``batch.shifts`` [E, 3], each in the
    caller's node / edge order.  ``cotangent``: [B, 6, 6], default all ones.

    Only the geometry is differentiated (``torch.autograd.grad``, with the parameters frozen
    while the call runs): parameters get no ``.grad`` and the radial MLP's weight-gradient
    kernels do not run.  ``batch`` is not modified: the model sees a shallow copy whose geometry
    tensors are fresh leaves.

    Not thread-safe with respect to ``model``: ``requires_grad`` of its parameters is switched off
    for the duration of the call and restored afterwards, so no other thread may train or
    differentiate the same model object meanwhile."""
    work = copy.copy(batch)
    leaves = []
    for k in GEOMETRY_KEYS:
        leaf = getattr(batch, k).detach().clone().requires_grad_(True)
        setattr(work, k, leaf)
        leaves.append(leaf)
    # parameters are frozen for the duration of the call: an autograd function decides what to
    # compute from the requires_grad of its inputs at forward time, so this is what skips the
    # weight-gradient launches (DESIGN.md "Geometry gradients" lists the ones that remain)
    thawed = [p for p in model.parameters() if p.requires_grad]
    try:
        for p in thawed:
            p.requires_grad_(False)
        with torch.enable_grad():
            c = model(work)["stiffness"]
            if cotangent is None:
                cotangent = torch.ones_like(c)
            if cotangent.shape != c.shape:
                raise ValueError(f"cotangent {tuple(cotangent.shape)} does not match the stiffness "
                                 f"{tuple(c.shape)}")
            grads = torch.autograd.grad(c, leaves, grad_outputs=cotangent.to(c.dtype))
    finally:
        for p in thawed:
            p.requires_grad_(True)
    out = {"stiffness": c.detach()}
    out.update(zip(GEOMETRY_KEYS, grads))
    return out
