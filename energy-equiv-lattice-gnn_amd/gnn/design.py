"""Design sensitivities of the stiffness surrogate: gradients of the predicted 6 x 6 stiffness
w.r.t. the lattice geometry (node positions, strut radii, periodic shifts).

The gradients run on the HIP backward path of the model (``eelg_tp_bwd_sh``,
``eelg_radial_bwd_x``, ``eelg_edge_embed_bwd`` and the kernels the training backward uses);
they are deterministic (no atomics) and fp32.  Second derivatives are not built.
``property_sensitivity`` starts the same backward from the elastic properties of the stiffness
(``gnn.elastic``: moduli, Poisson's ratio, anisotropy, directional Young's modulus; ``gnn.transverse``:
the shear, Poisson's ratio and compressibility surfaces).

``optimize_design`` closes the loop: it changes strut radii and node positions down those gradients
at constant strut volume.  The tail of an iteration -- tie the two directions of every strut, check
the gradient, normalise, heavy-ball step inside the box bounds, rescale to the volume -- is one
deterministic launch per iteration (``eelg_design_step``, ``csrc/eelg_design.hip``), and nothing
inside the loop waits for the device.  ``design_step_composed`` / ``strut_volume_composed`` are the
same functions in plain torch: the second implementation, the timing baseline and the CPU path
(``EELG_DESIGN_FUSED=0`` selects them on the device).
"""
from __future__ import annotations

import contextlib
import copy
import ctypes
import os
from dataclasses import dataclass
from typing import Dict, Optional, Tuple

import torch

from . import _lib

# one fused launch per design step on a HIP device (1), or the composed torch form everywhere (0)
FUSED = os.environ.get("EELG_DESIGN_FUSED", "1") != "0"

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
                         dir_weights: Optional[torch.Tensor] = None, *,
                         transverse_weights: Optional[torch.Tensor] = None,
                         transverse_dir_weights: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
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
    ``stiffness_sensitivity``.

    ``transverse_weights`` [B, 7] (``gnn.transverse.TRANSVERSE_COLUMNS``; its ``spd`` column as
    above) and ``transverse_dir_weights`` [B, P, 5] (``TRANSVERSE_DIR_COLUMNS``) over the same
    ``directions`` add ``sum(transverse_weights * transverse) + sum(transverse_dir_weights * t_dir)``
    to the objective: "how does the most negative Poisson's ratio change if I thicken this strut".
    With either of them the result gains ``'transverse'`` [B, 7] and ``'t_dir'`` [B, P, 5] (detached)
    and the call two more launches; a graph that is not positive definite contributes nothing through
    them.  With both ``None`` nothing changes."""
    return _geometry_gradients(model, batch, _property_cotangents(
        weights, directions, dir_weights, transverse_weights=transverse_weights,
        transverse_dir_weights=transverse_dir_weights))


def _property_cotangents(weights, directions, dir_weights, who: str = "property_sensitivity", *,
                         transverse_weights=None, transverse_dir_weights=None):
    """The ``cotangents`` function of ``sum(weights * properties) + sum(dir_weights * e_dir)`` plus,
    where given, the same two sums over the transverse rows."""
    from .elastic import ELASTIC_COLUMNS, elastic_properties
    n_dirs = 0 if directions is None else int(directions.shape[0])
    if dir_weights is not None and directions is None:
        raise ValueError(f"{who}: dir_weights without directions")
    transverse = transverse_weights is not None or transverse_dir_weights is not None
    if transverse and directions is None:
        raise ValueError(f"{who}: transverse_weights / transverse_dir_weights without directions")

    def cotangents(c):
        nb = int(c.shape[0])
        if tuple(weights.shape) != (nb, len(ELASTIC_COLUMNS)):
            raise ValueError(f"{who}: weights {tuple(weights.shape)}, expected "
                             f"[{nb}, {len(ELASTIC_COLUMNS)}]")
        if dir_weights is not None and tuple(dir_weights.shape) != (nb, n_dirs):
            raise ValueError(f"{who}: dir_weights {tuple(dir_weights.shape)}, expected "
                             f"[{nb}, {n_dirs}]")
        props, e_dir = elastic_properties(c, None if directions is None else directions.to(c.device))
        outputs, grads = [props], [weights.to(device=props.device, dtype=props.dtype)]
        if dir_weights is not None:
            outputs.append(e_dir)
            grads.append(dir_weights.to(device=e_dir.device, dtype=e_dir.dtype))
        extra = {"properties": props.detach(), "e_dir": e_dir.detach()}
        if transverse:
            from .transverse import TRANSVERSE_COLUMNS, TRANSVERSE_DIR_COLUMNS, transverse_properties
            for name, w, shape in (("transverse_weights", transverse_weights, (nb, len(TRANSVERSE_COLUMNS))),
                                   ("transverse_dir_weights", transverse_dir_weights,
                                    (nb, n_dirs, len(TRANSVERSE_DIR_COLUMNS)))):
                if w is not None and tuple(w.shape) != shape:
                    raise ValueError(f"{who}: {name} {tuple(w.shape)}, expected {list(shape)}")
            t_props, t_dir, _, _ = transverse_properties(c, directions.to(c.device))
            for out, w in ((t_props, transverse_weights), (t_dir, transverse_dir_weights)):
                if w is not None:
                    outputs.append(out)
                    grads.append(w.to(device=out.device, dtype=out.dtype))
            extra.update(transverse=t_props.detach(), t_dir=t_dir.detach())
        return extra, outputs, grads
    return cotangents


def _geometry_gradients(model, batch, cotangents) -> Dict[str, torch.Tensor]:
    """One model forward on fresh geometry leaves with the parameters frozen, and one backward.
    ``cotangents(stiffness)`` returns ``(extra results, outputs, their cotangents)``."""
    with _frozen(model):
        return _forward_backward(model, batch, cotangents)


@contextlib.contextmanager
def _frozen(model):
    """The parameters are frozen inside: an autograd function decides what to compute from the
    requires_grad of its inputs at forward time, so this is what skips the weight-gradient launches
    (DESIGN.md "Geometry gradients" lists the ones that remain)."""
    thawed = [p for p in model.parameters() if p.requires_grad]
    try:
        for p in thawed:
            p.requires_grad_(False)
        yield
    finally:
        for p in thawed:
            p.requires_grad_(True)


def _forward_backward(model, batch, cotangents) -> Dict[str, torch.Tensor]:
    """``_geometry_gradients`` inside ``_frozen(model)``: ``optimize_design`` freezes once and calls
    this every iteration."""
    work = copy.copy(batch)
    leaves = []
    for k in GEOMETRY_KEYS:
        leaf = getattr(batch, k).detach().clone().requires_grad_(True)
        setattr(work, k, leaf)
        leaves.append(leaf)
    with torch.enable_grad():
        c = model(work)["stiffness"]
        extra, outputs, grad_outputs = cotangents(c)
        grads = torch.autograd.grad(outputs, leaves, grad_outputs=grad_outputs)
    out = {"stiffness": c.detach()}
    out.update(extra)
    out.update(zip(GEOMETRY_KEYS, grads))
    return out


# ---------------------------------------------------------------------------------------------
# gradient-based design at constant strut volume
# ---------------------------------------------------------------------------------------------
@dataclass
class DesignLayout:
    """What a design step needs to know about a batch besides its geometry (``design_layout``),
    in the caller's node / edge order: ``partner`` [E] (the other direction of the same strut, or
    the edge itself), ``send`` / ``recv`` [E], ``node_ptr`` / ``edge_ptr`` [B + 1] (int32, on the
    batch's device), the graph of every node and edge (int64, for the composed form), and the two
    ``ptr`` rows once more in host memory, where the launch checks them."""
    partner: torch.Tensor
    send: torch.Tensor
    recv: torch.Tensor
    node_ptr: torch.Tensor
    edge_ptr: torch.Tensor
    node_graph: torch.Tensor
    edge_graph: torch.Tensor
    n_graphs: int
    n_nodes: int
    n_edges: int
    host_node_ptr: ctypes.Array
    host_edge_ptr: ctypes.Array


@dataclass
class DesignResult:
    """``optimize_design``'s result.  ``batch``: a shallow copy of the input with new ``positions``
    and ``edge_attr``.  ``objective`` [steps + 1, B]: the objective per graph before every step and
    after the last.  ``volume`` [steps + 1, B]: the strut volume likewise (row 0: the volume that is
    kept).  ``flags`` [steps, B] int32: non-zero where a step left a graph as it was (1: its
    gradient was not finite).  All on the batch's device; the function itself never reads them."""
    batch: object
    objective: torch.Tensor
    volume: torch.Tensor
    flags: torch.Tensor


def design_layout(batch) -> DesignLayout:
    """The ``DesignLayout`` of ``batch``: set-up work, done once per design run (a sort for the
    strut pairs and a few host reads).  Raises ``ValueError`` unless every graph's edges are
    contiguous in the caller's order, graph after graph, and ``edge_attr`` is one radius per edge."""
    from . import ops
    from .model import EnergyEquivGNN
    pos, ei = batch.positions, batch.edge_index
    dev = pos.device
    n, e, nb = int(pos.shape[0]), int(ei.shape[1]), int(batch.num_graphs)
    if pos.dim() != 2 or pos.shape[1] != 3 or tuple(batch.shifts.shape) != (e, 3):
        raise ValueError(f"design_layout: positions {tuple(pos.shape)}, shifts {tuple(batch.shifts.shape)}; "
                         f"expected [N, 3] and [{e}, 3]")
    if batch.edge_attr.numel() != e:
        raise ValueError(f"design_layout: edge_attr {tuple(batch.edge_attr.shape)} is not one radius per edge "
                         f"({e} edges)")
    node_ptr = batch.ptr.detach().to("cpu", torch.int64)
    if nb < 1 or tuple(node_ptr.shape) != (nb + 1,) or int(node_ptr[0]) != 0 or int(node_ptr[-1]) != n \
            or bool((node_ptr[1:] < node_ptr[:-1]).any()):
        raise ValueError(f"design_layout: batch.ptr does not split {n} nodes into {nb} graphs")
    node_graph = batch.batch.detach().to(torch.int64)
    send, recv = ei[0].detach().to(torch.int64), ei[1].detach().to(torch.int64)
    eg = node_graph[send]
    eg_host = eg.cpu()
    if not torch.equal(eg_host, node_graph[recv].cpu()):
        raise ValueError("design_layout: an edge joins nodes of two graphs")
    if bool((eg_host[1:] < eg_host[:-1]).any()):
        raise ValueError("design_layout: the edges of a graph are not contiguous in edge_index (graph after "
                         "graph); reorder the edges before designing")
    edge_ptr = torch.searchsorted(eg_host, torch.arange(nb + 1, dtype=torch.int64))
    csr = EnergyEquivGNN.edge_graph(batch, strut=False)
    perm = csr.perm.to(torch.int64)
    smap = ops.build_strut_map(pos, csr.sender, csr.receiver, batch.shifts[perm], batch.edge_attr.reshape(-1)[perm])
    partner = torch.empty(e, dtype=torch.int64, device=dev)
    partner[perm] = perm[smap.partner.to(torch.int64)]

    def i32(t):
        return t.to(device=dev, dtype=torch.int32).contiguous()

    def host(t):
        return (ctypes.c_int * (nb + 1))(*[int(v) for v in t.tolist()])
    return DesignLayout(i32(partner), i32(send), i32(recv), i32(node_ptr), i32(edge_ptr), node_graph.contiguous(),
                        eg.contiguous(), nb, n, e, host(node_ptr), host(edge_ptr))


def _volume_composed(pos, r, shifts, layout: DesignLayout) -> torch.Tensor:
    s, t = layout.send.long(), layout.recv.long()
    vx, vy, vz = (pos[t] - pos[s] + shifts).unbind(1)
    length = torch.sqrt(vx * vx + vy * vy + vz * vz)
    vol = torch.zeros(layout.n_graphs, dtype=pos.dtype, device=pos.device)
    return 0.5 * vol.index_add_(0, layout.edge_graph, r * r * length)


def _geometry_of(batch, dtype=None):
    pos = batch.positions.detach()
    dtype = pos.dtype if dtype is None else dtype
    return (pos.to(dtype).contiguous(), batch.edge_attr.detach().reshape(-1).to(dtype).contiguous(),
            batch.shifts.detach().to(dtype).contiguous())


def strut_volume_composed(batch, layout: Optional[DesignLayout] = None) -> torch.Tensor:
    """``strut_volume`` in plain torch, on any device, in the dtype of ``batch.positions``."""
    layout = design_layout(batch) if layout is None else layout
    return _volume_composed(*_geometry_of(batch), layout)


def strut_volume(batch, layout: Optional[DesignLayout] = None) -> torch.Tensor:
    """``V[g] = 1/2 sum_e r_e^2 L_e`` over the directed edges of graph g ([B]): the strut volume,
    which is the relative density up to pi and the cell volume.  On a HIP batch one launch of
    ``eelg_strut_volume`` (fp32, bitwise repeatable); on a CPU batch, or with
    ``EELG_DESIGN_FUSED=0``, ``strut_volume_composed``.  Not differentiable.  ``layout``: the
    batch's ``design_layout`` where the caller has one (building it reads the host)."""
    layout = design_layout(batch) if layout is None else layout
    if not (FUSED and batch.positions.is_cuda):
        return _volume_composed(*_geometry_of(batch), layout)
    pos, r, shifts = _geometry_of(batch, torch.float32)
    return _volume_fused(pos, r, shifts, layout)


def _volume_fused(pos, r, shifts, layout: DesignLayout, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    vol = torch.empty(layout.n_graphs, dtype=torch.float32, device=pos.device) if out is None else out
    with torch.cuda.device(pos.device):
        _lib.launch("strut_volume", _lib.load().eelg_strut_volume, pos, r, shifts, layout.send, layout.recv,
                     layout.node_ptr, layout.edge_ptr, ctypes.addressof(layout.host_node_ptr),
                     ctypes.addressof(layout.host_edge_ptr), layout.n_graphs, layout.n_nodes, layout.n_edges, vol,
                     on=vol, timed="strut_volume")
    return vol


def _check_step(layout, g_pos, g_r, pos, r, pos0, m_pos, m_r, shifts, v0, r_min, r_max, move_limit, who):
    n, e, nb = layout.n_nodes, layout.n_edges, layout.n_graphs
    for name, t, shape in (("g_pos", g_pos, (n, 3)), ("g_r", g_r, (e,)), ("pos", pos, (n, 3)), ("r", r, (e,)),
                           ("pos0", pos0, (n, 3)), ("m_pos", m_pos, (n, 3)), ("m_r", m_r, (e,)),
                           ("shifts", shifts, (e, 3)), ("v0", v0, (nb,))):
        if tuple(t.shape) != shape:
            raise ValueError(f"{who}: {name} {tuple(t.shape)}, expected {list(shape)}")
        if t.dtype != pos.dtype or t.device != pos.device:
            raise ValueError(f"{who}: {name} is {t.dtype} on {t.device}, pos {pos.dtype} on {pos.device}")
    if not r_min < r_max:
        raise ValueError(f"{who}: r_min {r_min} must lie below r_max {r_max}")
    if not move_limit >= 0:
        raise ValueError(f"{who}: move_limit {move_limit} must not be negative")


def design_step_composed(layout: DesignLayout, g_pos, g_r, pos, r, pos0, m_pos, m_r, shifts, v0, *,
                         step_r: float = 0.0, step_pos: float = 0.0, beta: float = 0.0, r_min: float, r_max: float,
                         move_limit: float, keep_volume: bool = True
                         ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """``design_step`` in plain torch, on any device, in ``pos``'s dtype: a chain of some 150 small
    torch operations, the per-graph values by ``scatter_reduce_`` / ``index_add_`` (atomics on the
    device, so its volume is not bitwise repeatable there).  Always returns new tensors."""
    _check_step(layout, g_pos, g_r, pos, r, pos0, m_pos, m_r, shifts, v0, r_min, r_max, move_limit,
                "design_step_composed")
    nb, eg, ng = layout.n_graphs, layout.edge_graph, layout.node_graph
    partner = layout.partner.long()
    own = partner == torch.arange(layout.n_edges, device=partner.device)
    gt = torch.where(own, g_r, g_r + g_r[partner])

    def per_graph(values, index, reduce):          # [B] from per-row values (zero-initialised)
        return torch.zeros(nb, dtype=values.dtype, device=values.device).scatter_reduce_(0, index, values, reduce)
    fin_e, fin_n = torch.isfinite(gt), torch.isfinite(g_pos).all(dim=1)
    bad = (per_graph((~fin_e).to(pos.dtype), eg, "sum") + per_graph((~fin_n).to(pos.dtype), ng, "sum")) > 0
    zero = torch.zeros((), dtype=pos.dtype, device=pos.device)
    big_r = per_graph(torch.where(fin_e, gt.abs(), zero), eg, "amax")
    big_p = per_graph(torch.where(fin_n, g_pos.abs().amax(dim=1), zero), ng, "amax")

    def move(g, big, index, step, x, m, lo, hi):
        moves = ~bad & (big > 0) if step != 0 else torch.zeros_like(bad)
        one = torch.ones((), dtype=pos.dtype, device=pos.device)
        div = torch.where(big > 0, big, one)[index]
        sel = moves[index]
        if g.dim() == 2:
            div, sel = div[:, None], sel[:, None]
        m_new = beta * m + g / div
        x_new = torch.minimum(torch.maximum(x - step * m_new, lo), hi)
        return torch.where(sel, x_new, x), torch.where(sel, m_new, m)
    lo_r = torch.full((), r_min, dtype=pos.dtype, device=pos.device)
    hi_r = torch.full((), r_max, dtype=pos.dtype, device=pos.device)
    pos1, m_pos1 = move(g_pos, big_p, ng, step_pos, pos, m_pos, pos0 - move_limit, pos0 + move_limit)
    r1, m_r1 = move(gt, big_r, eg, step_r, r, m_r, lo_r, hi_r)
    vol = _volume_composed(pos1, r1, shifts, layout)
    if keep_volume:
        ok = ~bad & (v0 > 0) & (vol > 0) & torch.isfinite(v0) & torch.isfinite(vol)
        scale = torch.where(ok, torch.sqrt(v0 / torch.where(ok, vol, torch.ones_like(vol))), torch.ones_like(vol))
        r1 = torch.where(~bad[eg], torch.minimum(torch.maximum(r1 * scale[eg], lo_r), hi_r), r1)
        vol = _volume_composed(pos1, r1, shifts, layout)
    return pos1, r1, m_pos1, m_r1, vol, bad.to(torch.int32)


def design_step(layout: DesignLayout, g_pos, g_r, pos, r, pos0, m_pos, m_r, shifts, v0, *, step_r: float = 0.0,
                step_pos: float = 0.0, beta: float = 0.0, r_min: float, r_max: float, move_limit: float,
                keep_volume: bool = True, inplace: bool = False, vol: Optional[torch.Tensor] = None,
                flag: Optional[torch.Tensor] = None):
    """One design step: ``(pos, r, m_pos, m_r, vol [B], flag [B] int32)`` from the gradients
    ``g_pos`` [N, 3], ``g_r`` [E] of an objective to minimise, the geometry ``pos`` / ``r``, the
    initial positions ``pos0``, the momenta and the volume ``v0`` [B] to keep, all in the caller's
    order (``layout``: ``design_layout`` of the batch).  Per graph, as ``include/eelg.h`` states it:

    1. the two directions of a strut share the sum of their two radius gradients (bitwise);
    2. a graph with a gradient entry that is not finite is left as it is, flag 1;
    3. each group (radii, positions) is divided by its largest absolute entry; a group whose maximum
       or step size is 0 does not move;
    4. ``m = beta m + g / G``, ``x = clamp(x - step m)``: radii into ``[r_min, r_max]``, positions
       into ``pos0 +- move_limit``; ``step_*`` is the largest move of an iteration from rest;
    5. with ``keep_volume`` the radii are multiplied by ``sqrt(v0 / V)`` and clamped once more, one
       pass: where a clamp binds the volume may miss ``v0``.

    On HIP tensors one launch of ``eelg_design_step`` (fp32, bitwise repeatable, a graph's result
    independent of the batch around it), which reads nothing back.  ``inplace=True`` updates
    ``pos``, ``r``, ``m_pos``, ``m_r`` themselves (contiguous fp32) and writes into the rows ``vol``
    / ``flag`` where given; otherwise the inputs are left alone.  On CPU tensors, or with
    ``EELG_DESIGN_FUSED=0``, ``design_step_composed``."""
    if not (FUSED and pos.is_cuda):
        out = design_step_composed(layout, g_pos, g_r, pos, r, pos0, m_pos, m_r, shifts, v0, step_r=step_r,
                                   step_pos=step_pos, beta=beta, r_min=r_min, r_max=r_max, move_limit=move_limit,
                                   keep_volume=keep_volume)
        if not inplace:
            return out
        for dst, src in zip((pos, r, m_pos, m_r), out[:4]):
            dst.copy_(src)
        ret_vol = out[4] if vol is None else vol.copy_(out[4])
        ret_flag = out[5] if flag is None else flag.copy_(out[5])
        return pos, r, m_pos, m_r, ret_vol, ret_flag
    _check_step(layout, g_pos, g_r, pos, r, pos0, m_pos, m_r, shifts, v0, r_min, r_max, move_limit, "design_step")
    if pos.dtype != torch.float32:
        raise ValueError(f"design_step: the fused step is fp32, got {pos.dtype}")
    if not inplace:
        pos, r, m_pos, m_r = (t.clone(memory_format=torch.contiguous_format) for t in (pos, r, m_pos, m_r))
    nb = layout.n_graphs
    vol = torch.empty(nb, dtype=torch.float32, device=pos.device) if vol is None else vol
    flag = torch.zeros(nb, dtype=torch.int32, device=pos.device) if flag is None else flag
    for name, t in (("pos", pos), ("r", r), ("m_pos", m_pos), ("m_r", m_r), ("vol", vol), ("flag", flag)):
        if not t.is_contiguous():
            raise ValueError(f"design_step: {name} must be contiguous")
    if tuple(vol.shape) != (nb,) or vol.dtype != torch.float32 or tuple(flag.shape) != (nb,) \
            or flag.dtype != torch.int32:
        raise ValueError(f"design_step: vol / flag must be [{nb}] float32 / int32")
    with torch.cuda.device(pos.device):
        _lib.launch("design_step", _lib.load().eelg_design_step, g_pos.contiguous(), g_r.contiguous(), pos, r,
                     pos0.contiguous(), m_pos, m_r, layout.partner, layout.node_ptr, layout.edge_ptr,
                     ctypes.addressof(layout.host_node_ptr), ctypes.addressof(layout.host_edge_ptr), shifts.contiguous(),
                     layout.send, layout.recv, v0.contiguous(), nb, layout.n_nodes, layout.n_edges, float(step_r),
                     float(step_pos), float(beta), float(r_min), float(r_max), float(move_limit), int(bool(keep_volume)),
                     vol, flag, on=pos, timed="design_step")
    return pos, r, m_pos, m_r, vol, flag


def optimize_design(model, batch, *, target: Optional[torch.Tensor] = None, weights: Optional[torch.Tensor] = None,
                    directions: Optional[torch.Tensor] = None, dir_weights: Optional[torch.Tensor] = None,
                    transverse_weights: Optional[torch.Tensor] = None,
                    transverse_dir_weights: Optional[torch.Tensor] = None, steps: int, step_r: float = 0.0, step_pos: float = 0.0, beta: float = 0.0, r_min: float,
                    r_max: Optional[float] = None, move_limit: float, keep_volume: bool = True) -> DesignResult:
    """Change the strut radii and node positions of every lattice of ``batch`` to lower an
    objective of its predicted stiffness ``C``, ``steps`` iterations of ``design_step`` at constant
    strut volume.  The objective, per graph, is one of

    * ``target`` [B, 6, 6]: ``J = 1/2 |C - C*|_F^2 / |C*|_F^2``;
    * ``weights`` [B, 12] and / or ``dir_weights`` [B, P] over ``directions`` [P, 3]:
      ``J = sum(weights * properties) + sum(dir_weights * e_dir)`` with the meaning they have in
      ``property_sensitivity`` (a zero weight skips its column, NaN or not); negative weights
      maximise.  ``transverse_weights`` [B, 7] and / or ``transverse_dir_weights`` [B, P, 5] add
      ``sum(transverse_weights * transverse) + sum(transverse_dir_weights * t_dir)`` likewise: a
      negative weight on ``nu_min`` asks for a more auxetic lattice, a negative weight on ``G_min``
      stiffens the softest shear.

    ``step_r`` / ``step_pos``: the largest change of a radius / a position component per iteration
    from rest (0: that group stays); ``beta``: heavy-ball momentum; radii stay in ``[r_min, r_max]``
    (``r_max`` defaults to ``model.max_edge_radius``, beyond which the radius embedding is flat) and
    positions within ``move_limit`` of where they started.

    Set-up (once; reads the host): ``design_layout`` -- ``ValueError`` unless every graph's edges are
    contiguous -- the strut pairs of the initial geometry and the volume to keep.  Each iteration
    is one model forward and one geometry backward (``stiffness_sensitivity``'s path, parameters
    frozen), the objective's cotangent in a few [B, .] ops and one ``design_step`` launch; it sorts
    nothing, builds no CSR and never waits for the device.  One more forward gives the final
    objective.  ``batch`` and its tensors are untouched; the parameters end as they were, without
    ``.grad``.  bf16 storage raises ``NotImplementedError``, as the geometry gradients do.  Thread
    safety: as ``stiffness_sensitivity``."""
    from .model import EnergyEquivGNN, storage_dtype
    who = "optimize_design"
    nb = int(batch.num_graphs)
    transverse = transverse_weights is not None or transverse_dir_weights is not None
    linear = weights is not None or dir_weights is not None or transverse
    if target is not None and linear:
        raise ValueError(f"{who}: give either target or weights / dir_weights / transverse weights, not both")
    if target is None and not linear:
        raise ValueError(f"{who}: give an objective: target, or weights / dir_weights / transverse weights")
    if target is not None and tuple(target.shape) != (nb, 6, 6):
        raise ValueError(f"{who}: target {tuple(target.shape)}, expected [{nb}, 6, 6]")
    if directions is not None and (directions.dim() != 2 or directions.shape[1] != 3):
        raise ValueError(f"{who}: directions {tuple(directions.shape)}, expected [P, 3]")
    if linear:
        from .elastic import ELASTIC_COLUMNS
        if weights is None:
            like = next(w for w in (dir_weights, transverse_weights, transverse_dir_weights) if w is not None)
            weights = torch.zeros(nb, len(ELASTIC_COLUMNS), dtype=like.dtype, device=like.device)
        if tuple(weights.shape) != (nb, len(ELASTIC_COLUMNS)):
            raise ValueError(f"{who}: weights {tuple(weights.shape)}, expected [{nb}, {len(ELASTIC_COLUMNS)}]")
        if dir_weights is not None and (directions is None or tuple(dir_weights.shape) != (nb, int(directions.shape[0]))):
            raise ValueError(f"{who}: dir_weights {tuple(dir_weights.shape)} need directions [P, 3] and the shape "
                             f"[{nb}, P]")
    r_max = float(model.max_edge_radius) if r_max is None else float(r_max)
    r_min, move_limit, steps = float(r_min), float(move_limit), int(steps)
    if not r_min < r_max:
        raise ValueError(f"{who}: r_min {r_min} must lie below r_max {r_max}")
    if not move_limit >= 0 or steps < 0 or step_r < 0 or step_pos < 0:
        raise ValueError(f"{who}: move_limit {move_limit}, steps {steps}, step_r {step_r}, step_pos {step_pos} "
                         "must not be negative")
    if storage_dtype(model.params) != torch.float32:
        raise NotImplementedError(f"{who}: geometry gradients are built for fp32 storage only, not "
                                  "storage_dtype='bfloat16'")

    # ---- set-up: host reads are allowed here and nowhere below
    layout = design_layout(batch)
    dev = batch.positions.device
    pos0, r, shifts = _geometry_of(batch, torch.float32)
    pos, r = pos0.clone(), r.clone()
    m_pos, m_r = torch.zeros_like(pos), torch.zeros_like(r)
    work = copy.copy(batch)
    work.positions, work.edge_attr, work.shifts = pos, r.view(-1, 1), shifts
    if dev.type == "cuda":
        # a CSR object of its own, so that no strut map of the input's geometry is used or dropped
        csr = copy.copy(EnergyEquivGNN.edge_graph(batch, strut=False))
        csr.strut = None
        work._eelg_csr = csr
    fused = FUSED and dev.type == "cuda"
    v0 = _volume_fused(pos, r, shifts, layout) if fused else _volume_composed(pos, r, shifts, layout)
    objective = torch.empty(steps + 1, nb, dtype=torch.float32, device=dev)
    volume = torch.zeros(steps + 1, nb, dtype=torch.float32, device=dev)     # (a batch without edges keeps 0)
    flags = torch.zeros(steps, nb, dtype=torch.int32, device=dev)
    volume[0] = v0

    if target is not None:
        tgt = target.detach().to(device=dev, dtype=torch.float32)
        inv = 1.0 / (tgt * tgt).sum(dim=(1, 2))

        def value(c):
            d = c.detach() - tgt
            return d, 0.5 * (d * d).sum(dim=(1, 2)) * inv

        def cotangents(c):
            d, j = value(c)
            return {"objective": j}, [c], [d * inv[:, None, None]]
    else:
        inner = _property_cotangents(weights, directions, dir_weights, who, transverse_weights=transverse_weights,
                                     transverse_dir_weights=transverse_dir_weights)

        def weighted(w, v):
            return torch.where(w != 0, w * v, torch.zeros_like(v)).flatten(1).sum(dim=1)

        def cotangents(c):
            extra, outputs, grads = inner(c)
            j = weighted(grads[0], extra["properties"])
            rest = list(grads[1:])
            for given, key in ((dir_weights, "e_dir"), (transverse_weights, "transverse"),
                               (transverse_dir_weights, "t_dir")):
                if given is not None:
                    j = j + weighted(rest.pop(0), extra[key])
            extra["objective"] = j
            return extra, outputs, grads

    with _frozen(model):
        for t in range(steps):
            out = _forward_backward(model, work, cotangents)
            objective[t] = out["objective"]
            design_step(layout, out["positions"], out["edge_attr"].reshape(-1), pos, r, pos0, m_pos, m_r, shifts, v0,
                        step_r=step_r, step_pos=step_pos, beta=beta, r_min=r_min, r_max=r_max,
                        move_limit=move_limit, keep_volume=keep_volume, inplace=True, vol=volume[t + 1],
                        flag=flags[t])
        with torch.no_grad():
            objective[steps] = cotangents(model(work)["stiffness"])[0]["objective"]
    result = copy.copy(batch)
    result.positions = pos.to(batch.positions.dtype)
    result.edge_attr = r.to(batch.edge_attr.dtype).view_as(batch.edge_attr)
    if hasattr(work, "_eelg_csr"):
        result._eelg_csr = work._eelg_csr
    return DesignResult(result, objective, volume, flags)
