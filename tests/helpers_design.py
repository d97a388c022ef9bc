"""The lattice design step restated in fp64 as per-graph Python / numpy loops, straight from the
formulas of the step (``include/eelg.h``), and the small batches the design tests run on.  Nothing
here imports ``gnn.design``: strut pairs, graph ranges, the volume and the step are all worked out
again from the raw arrays."""
from __future__ import annotations

import numpy as np
import torch

from gnn.data import Data, collate
from gnn.synthetic import make_lattice

THREADS = 256                       # include/eelg.h EELG_DESIGN_THREADS
# every hyper-parameter is exactly representable in fp32, so fp32 and fp64 runs take the same ones
HYPER = dict(step_r=2.0 ** -9, step_pos=2.0 ** -6, beta=0.75, r_min=2.0 ** -8, r_max=2.0 ** -4,
             move_limit=2.0 ** -5, keep_volume=True)
COLUMNS = ("pos", "r", "m_pos", "m_r", "vol")
_GRAPHS = []


def _with_extra_edge(d: Data, edge: int, radius=None) -> Data:
    """``d`` with a copy of directed edge ``edge`` appended (``radius``: the copy's own radius)."""
    rad = d.edge_attr[edge:edge + 1] if radius is None else torch.full((1, 1), radius)
    return Data(positions=d.positions, node_attrs=d.node_attrs,
                edge_index=torch.cat([d.edge_index, d.edge_index[:, edge:edge + 1]], dim=1),
                shifts=torch.cat([d.shifts, d.shifts[edge:edge + 1]]), edge_attr=torch.cat([d.edge_attr, rad]),
                stiffness=d.stiffness, rel_dens=d.rel_dens, name=d.name)


def design_graphs():
    """Four lattices chosen for where a one-workgroup-per-graph kernel can break: 2 edges (one strut);
    70 edges (no multiple of 64); 257 edges (one more than the workgroup's threads: 128 struts and a
    directed edge with a radius of its own, so it has no partner); 10 nodes / 30 edges + an exact
    duplicate of edge 3 (the duplicate, the original and their reverse have no unique partner)."""
    if not _GRAPHS:
        _GRAPHS.extend([make_lattice(2, 2, 11), make_lattice(20, 70, 12),
                        _with_extra_edge(make_lattice(64, THREADS, 13), 5, radius=0.03125),
                        _with_extra_edge(make_lattice(10, 30, 14), 3)])
        assert [g.edge_index.shape[1] for g in _GRAPHS] == [2, 70, THREADS + 1, 31]
    return _GRAPHS


def design_batch(which=(0, 1, 2, 3)):
    return collate([design_graphs()[i] for i in which])


def arrays(batch) -> dict:
    """The batch as numpy arrays (geometry fp64 with the batch's values) with the graph ranges and
    the strut pairs worked out here."""
    pos = batch.positions.detach().cpu().double().numpy()
    r = batch.edge_attr.detach().cpu().double().numpy().reshape(-1)
    shifts = batch.shifts.detach().cpu().double().numpy()
    send, recv = (batch.edge_index[i].cpu().numpy().astype(np.int64) for i in (0, 1))
    node_graph = batch.batch.cpu().numpy()
    nb = int(batch.num_graphs)
    node_ptr = np.searchsorted(node_graph, np.arange(nb + 1))
    edge_graph = node_graph[send]
    assert (np.diff(edge_graph) >= 0).all()
    edge_ptr = np.searchsorted(edge_graph, np.arange(nb + 1))
    return dict(pos=pos, r=r, shifts=shifts, send=send, recv=recv, node_ptr=node_ptr, edge_ptr=edge_ptr, n_graphs=nb,
                partner=partners(batch))


def partners(batch) -> np.ndarray:
    """partner[e]: the one edge with swapped endpoints, the negated fp32 edge vector and the same
    fp32 radius, if e's own description and that one each occur exactly once; else e."""
    pos = batch.positions.detach().cpu().float().numpy()
    sh = batch.shifts.detach().cpu().float().numpy()
    rad = batch.edge_attr.detach().cpu().float().numpy().reshape(-1)
    send, recv = (batch.edge_index[i].cpu().numpy() for i in (0, 1))
    vec = (pos[recv] - pos[send]) + sh + np.float32(0.0)            # + 0: -0.0 counts as +0.0
    neg = -vec + np.float32(0.0)
    e = len(send)
    out = np.arange(e)
    for i in range(e):
        same = (send == send[i]) & (recv == recv[i]) & (vec == vec[i]).all(axis=1) & (rad == rad[i])
        back = (send == recv[i]) & (recv == send[i]) & (vec == neg[i]).all(axis=1) & (rad == rad[i])
        if same.sum() == 1 and back.sum() == 1:
            out[i] = int(np.nonzero(back)[0][0])
    return out


def ref_volume(a: dict, pos=None, r=None) -> np.ndarray:
    pos = a["pos"] if pos is None else pos
    r = a["r"] if r is None else r
    vol = np.zeros(a["n_graphs"])
    for g in range(a["n_graphs"]):
        for e in range(a["edge_ptr"][g], a["edge_ptr"][g + 1]):
            v = pos[a["recv"][e]] - pos[a["send"][e]] + a["shifts"][e]
            vol[g] += 0.5 * r[e] ** 2 * np.sqrt(v @ v)
    return vol


def ref_step(a: dict, g_pos, g_r, pos, r, pos0, m_pos, m_r, v0, *, step_r, step_pos, beta, r_min, r_max, move_limit,
             keep_volume) -> dict:
    """One design step in fp64, graph by graph, element by element."""
    g_pos, g_r, pos, r, pos0, m_pos, m_r, v0 = (np.array(x, dtype=np.float64) for x in
                                                (g_pos, g_r, pos, r, pos0, m_pos, m_r, v0))
    partner = a["partner"]
    flag = np.zeros(a["n_graphs"], dtype=np.int32)
    vol = np.zeros(a["n_graphs"])
    for g in range(a["n_graphs"]):
        n0, n1, e0, e1 = a["node_ptr"][g], a["node_ptr"][g + 1], a["edge_ptr"][g], a["edge_ptr"][g + 1]
        tied = {e: g_r[e] + g_r[partner[e]] if partner[e] != e else g_r[e] for e in range(e0, e1)}
        everything = list(tied.values()) + list(g_pos[n0:n1].reshape(-1))
        if not np.isfinite(everything).all():
            flag[g] = 1
            continue
        big_r = max([abs(v) for v in tied.values()], default=0.0)
        big_p = float(np.abs(g_pos[n0:n1]).max()) if n1 > n0 else 0.0
        if big_r > 0 and step_r != 0:
            for e in range(e0, e1):
                m_r[e] = beta * m_r[e] + tied[e] / big_r
                r[e] = min(max(r[e] - step_r * m_r[e], r_min), r_max)
        if big_p > 0 and step_pos != 0:
            for i in range(n0, n1):
                for c in range(3):
                    m_pos[i, c] = beta * m_pos[i, c] + g_pos[i, c] / big_p
                    pos[i, c] = min(max(pos[i, c] - step_pos * m_pos[i, c], pos0[i, c] - move_limit),
                                    pos0[i, c] + move_limit)
    vol = ref_volume(a, pos, r)
    if keep_volume:
        for g in range(a["n_graphs"]):
            if flag[g] == 0 and vol[g] > 0 and v0[g] > 0:
                scale = np.sqrt(v0[g] / vol[g])
                for e in range(a["edge_ptr"][g], a["edge_ptr"][g + 1]):
                    r[e] = min(max(r[e] * scale, r_min), r_max)
        vol = ref_volume(a, pos, r)
    return dict(pos=pos, r=r, m_pos=m_pos, m_r=m_r, vol=vol, flag=flag)


def step_inputs(batch, seed: int = 5) -> dict:
    """fp32 inputs of a step on ``batch``: gradients (the two directions of a strut get different
    radius gradients), momenta from an earlier step (equal in both directions of a strut), the
    initial positions a little away from the current ones, and the volume to keep 3 % off the
    current one.  Torch tensors on the CPU."""
    gen = torch.Generator().manual_seed(seed)
    n, e = batch.positions.shape[0], batch.edge_index.shape[1]
    partner = torch.from_numpy(partners(batch))
    first = torch.minimum(partner, torch.arange(e))
    pos = batch.positions.clone()
    vol = torch.from_numpy(ref_volume(arrays(batch))).float()
    return dict(g_pos=torch.randn(n, 3, generator=gen) * 3.0, g_r=torch.randn(e, generator=gen) * 40.0, pos=pos,
                r=batch.edge_attr.reshape(-1).clone(),
                pos0=pos + (torch.rand(n, 3, generator=gen) - 0.5) * HYPER["move_limit"],
                m_pos=torch.randn(n, 3, generator=gen) * 0.3, m_r=(torch.randn(e, generator=gen) * 0.3)[first],
                shifts=batch.shifts.clone(), v0=vol * 1.03)


def ref_of(batch, inp: dict, **hyper) -> dict:
    """``ref_step`` on the fp64 values of the fp32 inputs ``inp``."""
    h = dict(HYPER)
    h.update(hyper)
    a = arrays(batch)
    return ref_step(a, *(inp[k].double().numpy() for k in ("g_pos", "g_r", "pos", "r", "pos0", "m_pos", "m_r", "v0")),
                    **h)


def column_errors(got: dict, ref: dict) -> dict:
    """Per output column: the largest absolute error over the batch relative to the column's largest
    fp64 value."""
    out = {}
    for k in COLUMNS:
        x = got[k].detach().double().cpu().numpy() if torch.is_tensor(got[k]) else np.asarray(got[k], dtype=np.float64)
        out[k] = float(np.abs(x - ref[k]).max() / np.abs(ref[k]).max())
    return out


def bounds(base: dict, ref: dict) -> dict:
    """4x the baseline's error, at least 4 fp32 ulps of the column's largest value (relative)."""
    out = {}
    for k in COLUMNS:
        top = np.float32(np.abs(ref[k]).max())
        out[k] = max(4.0 * base[k], 4.0 * float(np.spacing(top)) / float(top))
    return out


def as_dict(out) -> dict:
    """``(pos, r, m_pos, m_r, vol, flag)`` as a dict."""
    return dict(zip(COLUMNS + ("flag",), out))


def oracle_design_loop(o, batch, target, steps: int, **hyper) -> dict:
    """The design loop in fp64 from the oracle alone: the oracle model ``o`` (fp64, CPU), autograd
    to positions and radii, ``ref_step``.  ``target`` [B, 6, 6] fp64.  Returns the objective and
    volume histories [steps + 1, B], the final geometry, whether a clamp ever bound and the largest
    condition number of a predicted stiffness."""
    from helpers import batch_to
    a = arrays(batch)
    work = batch_to(batch, "cpu", torch.float64)
    pos0, r = a["pos"].copy(), a["r"].copy()
    pos = pos0.copy()
    m_pos, m_r = np.zeros_like(pos), np.zeros_like(r)
    v0 = ref_volume(a)
    inv = 1.0 / (target * target).sum(dim=(1, 2))
    objective, volume, kappa, bound = [], [v0], 0.0, False

    def evaluate(with_grad: bool):
        nonlocal kappa
        work.positions = torch.from_numpy(pos.copy()).requires_grad_(with_grad)
        work.edge_attr = torch.from_numpy(r.copy()).reshape(-1, 1).requires_grad_(with_grad)
        c = o(work)["stiffness"]
        kappa = max(kappa, float(torch.linalg.cond(c.detach()).max()))
        j = 0.5 * ((c - target) ** 2).sum(dim=(1, 2)) * inv
        objective.append(j.detach().numpy().copy())
        if with_grad:
            return torch.autograd.grad(j.sum(), [work.positions, work.edge_attr])
    for _ in range(steps):
        g_pos, g_r = evaluate(True)
        out = ref_step(a, g_pos.numpy(), g_r.numpy().reshape(-1), pos, r, pos0, m_pos, m_r, v0, **hyper)
        pos, r, m_pos, m_r = out["pos"], out["r"], out["m_pos"], out["m_r"]
        bound = bound or bool((r <= hyper["r_min"]).any() or (r >= hyper["r_max"]).any()
                              or (np.abs(pos - pos0) >= hyper["move_limit"]).any())
        volume.append(out["vol"])
        assert not out["flag"].any()
    with torch.no_grad():
        evaluate(False)
    return dict(objective=np.stack(objective), volume=np.stack(volume), pos=pos, r=r, bound=bound, kappa=kappa)
