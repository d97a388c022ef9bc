"""Design sensitivities of the stiffness surrogate: gradients of the predicted 6 x 6 stiffness
w.r.t. the lattice geometry (node positions, strut radii, periodic shifts).

The gradients run on the HIP backward path of the model (``eelg_tp_bwd_sh``,
``eelg_radial_bwd_x``, ``eelg_edge_embed_bwd`` and the kernels the training backward uses);
they are deterministic (no atomics) and fp32.  Second derivatives are not built.
``property_sensitivity`` starts the same backward from the elastic properties of the stiffness
(``gnn.elastic``: moduli, Poisson's ratio, anisotropy, directional Young's modulus).
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
    def cotangents(c):
        cot = torch.ones_like(c) if cotangent is None else cotangent
        if cot.shape != c.shape:
            raise ValueError(f"cotangent {tuple(cot.shape)} does not match the stiffness "
                             f"{tuple(c.shape)}")
        return {}, [c], [cot.to(c.dtype)]
    return _geometry_gradients(model, batch, cotangents)


def property_sensitivity(model, batch, weights: torch.Tensor, directions: Optional[torch.Tensor] = None,
                         dir_weights: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
    """``{'stiffness', 'properties', 'e_dir', 'positions', 'edge_attr', 'shifts'}``: the model's
    stiffness [B, 6, 6], its elastic properties [B, 12] (``gnn.elastic.ELASTIC_COLUMNS``) and
    directional Young's moduli [B, P] over ``directions`` [P, 3] (all detached), and the gradients of
    ``sum(weights * properties) + sum(dir_weights * e_dir)`` w.r.t. the geometry, as
    ``stiffness_sensitivity`` returns them: "how does E along [111] change if I move this node or
    thicken this strut".

    ``weights``: [B, 12], zero in the ``spd`` column (a flag has no gradient; the caller's tensor is
    not read back to check, a non-zero weight there has no effect).  ``dir_weights``: [B, P] or
    None.  One model forward, one backward, no host synchronisation.  A graph whose predicted
    stiffness is not positive definite contributes the gradient of its ``K_V`` / ``G_V`` terms
    alone.  Frozen parameters, the untouched ``batch`` and thread safety: as
    ``stiffness_sensitivity``."""
    from .elastic import ELASTIC_COLUMNS, elastic_properties
    n_dirs = 0 if directions is None else int(directions.shape[0])
    if dir_weights is not None and directions is None:
        raise ValueError("property_sensitivity: dir_weights without directions")

    def cotangents(c):
        nb = int(c.shape[0])
        if tuple(weights.shape) != (nb, len(ELASTIC_COLUMNS)):
            raise ValueError(f"property_sensitivity: weights {tuple(weights.shape)}, expected "
                             f"[{nb}, {len(ELASTIC_COLUMNS)}]")
        if dir_weights is not None and tuple(dir_weights.shape) != (nb, n_dirs):
            raise ValueError(f"property_sensitivity: dir_weights {tuple(dir_weights.shape)}, expected "
                             f"[{nb}, {n_dirs}]")
        props, e_dir = elastic_properties(c, None if directions is None else directions.to(c.device))
        outputs, grads = [props], [weights.to(device=props.device, dtype=props.dtype)]
        if dir_weights is not None:
            outputs.append(e_dir)
            grads.append(dir_weights.to(device=e_dir.device, dtype=e_dir.dtype))
        return {"properties": props.detach(), "e_dir": e_dir.detach()}, outputs, grads
    return _geometry_gradients(model, batch, cotangents)


def _geometry_gradients(model, batch, cotangents) -> Dict[str, torch.Tensor]:
    """One model forward on fresh geometry leaves with the parameters frozen, and one backward.
    ``cotangents(stiffness)`` returns ``(extra results, outputs, their cotangents)``."""
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
            extra, outputs, grad_outputs = cotangents(c)
            grads = torch.autograd.grad(outputs, leaves, grad_outputs=grad_outputs)
    finally:
        for p in thawed:
            p.requires_grad_(True)
    out = {"stiffness": c.detach()}
    out.update(extra)
    out.update(zip(GEOMETRY_KEYS, grads))
    return out
