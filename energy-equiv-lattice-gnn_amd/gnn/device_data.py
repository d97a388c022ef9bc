"""Device-resident dataset and loader: the whole dataset is packed once into flat HIP tensors
and a batch is assembled by ``eelg_batch_assemble`` / ``eelg_mandel_rotate`` (``csrc/eelg_batch.hip``)
-- a gather with offsets, one 3x3 multiply per position / shift row and a 6x6 congruence per
target -- instead of ``RotateLat`` per sample, a CPU ``collate`` and two sorts per batch
(``scripts/train_utils.py:114-146``, PyG collation, ``gnn.data.build_edge_csr``).

Why no batch needs a sort: the receiver-sorted CSR of a collated batch is the concatenation of
the per-graph CSRs plus offsets.  Graph g's receivers are all smaller than graph g + 1's and its
edges come first, so a stable sort by receiver (and the stable sort by sender over that order)
never interleaves graphs.  The per-graph pieces are built once, at pack time.

``pack_graphs`` is the host-side packer (CPU tensors, no device needed); ``DeviceDataset`` moves
its result to a HIP device; ``DeviceLoader`` iterates ``Batch`` objects that are drop-in for every
model of the package (``batch.csr`` is the dict ``EnergyEquivGNN.edge_graph`` accepts).
"""
from __future__ import annotations

from typing import Dict, Iterator, List, Optional, Sequence

import numpy as np
import torch

from . import _lib
from .data import Batch, build_edge_csr
from .lattice_data import cart4_to_mandel, rand_rotations

_LIMIT = 2 ** 31
_NODE_T = ("positions", "node_attrs", "rowend", "srowend")
_EDGE_T = ("sender", "receiver", "shifts", "edge_attr", "perm", "sperm")


def _check_extents(total_nodes: int, total_edges: int) -> None:
    if total_nodes >= _LIMIT or total_edges >= _LIMIT:
        raise ValueError(f"{total_nodes} nodes / {total_edges} edges: the packed tensors are indexed "
                         f"with int32, both counts must stay below 2**31")


def _mandel_target(t: torch.Tensor, what: str) -> torch.Tensor:
    """[1, 3, 3, 3, 3] cartesian (converted on the item's own tensor, as ``RotateLat`` does) or
    [1, 6, 6] / [6, 6] Mandel (taken as it is) -> [6, 6] fp32."""
    if t.dim() >= 4 and tuple(t.shape[-4:]) == (3, 3, 3, 3):
        t = cart4_to_mandel(t)
    if tuple(t.shape[-2:]) != (6, 6) or t.numel() != 36:
        raise ValueError(f"{what} of shape {tuple(t.shape)}: expected [1, 3, 3, 3, 3] or [1, 6, 6]")
    return t.reshape(6, 6).to(torch.float32)


class PackedGraphs:
    """Flat tensors of a whole dataset (see ``pack_graphs``) plus host copies of the extents."""

    def __init__(self, tensors: Dict[str, torch.Tensor], node_ptr: np.ndarray, edge_ptr: np.ndarray,
                 names: Optional[List], rel_dens: Optional[np.ndarray], max_edge_radius: float,
                 degree_stats: Dict[str, float]):
        self.tensors = tensors
        self.node_ptr, self.edge_ptr = node_ptr, edge_ptr          # int64 [G + 1], host
        self.names = names
        self.rel_dens = rel_dens                                   # fp32 [G] or [G, k], host
        self.max_edge_radius = max_edge_radius
        self._degree_stats = degree_stats

    def __len__(self) -> int:
        return int(self.node_ptr.shape[0]) - 1

    num_graphs = property(__len__)

    @property
    def device(self) -> torch.device:
        return self.tensors["positions"].device

    def degree_stats(self) -> Dict[str, float]:
        """``gnn.degree_stats`` of the collation of all graphs (the in-degrees are the row lengths
        of the per-graph CSRs, in the collation's node order)."""
        return dict(self._degree_stats)

    def to(self, device) -> "PackedGraphs":
        t = {k: v.to(device) for k, v in self.tensors.items()}
        return PackedGraphs(t, self.node_ptr, self.edge_ptr, self.names, self.rel_dens,
                            self.max_edge_radius, self._degree_stats)


def pack_graphs(items: Sequence) -> PackedGraphs:
    """Pack untransformed ``Data`` items into flat CPU tensors:

    * node rows ``positions [sumN, 3]``, ``node_attrs [sumN, F]``; edge rows in each graph's own
      edge order: LOCAL ``sender`` / ``receiver`` (int32), ``shifts [sumE, 3]``, ``edge_attr [sumE, A]``;
    * each graph's local CSR from ``build_edge_csr``: ``perm`` / ``sperm`` (int32 [sumE]) and the row
      ends ``rowend = rowptr[1:]``, ``srowend = srowptr[1:]`` (int32 [sumN]);
    * ``stiffness`` (and ``compliance`` when the items carry it) as Mandel ``[G, 6, 6]`` fp32;
    * host extents ``node_ptr`` / ``edge_ptr`` [G + 1], ``names``, ``rel_dens``.
    """
    items = list(items)
    if not items:
        raise ValueError("pack_graphs: no graphs")
    nn = [int(d.node_attrs.shape[0]) for d in items]
    ne = [int(d.edge_index.shape[1]) for d in items]
    for g, n in enumerate(nn):
        if n < 1:
            raise ValueError(f"graph {g} has no nodes")
    node_ptr = np.concatenate([[0], np.cumsum(nn, dtype=np.int64)]).astype(np.int64)
    edge_ptr = np.concatenate([[0], np.cumsum(ne, dtype=np.int64)]).astype(np.int64)
    _check_extents(int(node_ptr[-1]), int(edge_ptr[-1]))
    first = items[0]
    has_comp = "compliance" in first and torch.is_tensor(first.compliance)
    has_rel = "rel_dens" in first and first.rel_dens is not None
    has_name = "name" in first
    cols: Dict[str, list] = {k: [] for k in _NODE_T + _EDGE_T + ("stiffness",)}
    if has_comp:
        cols["compliance"] = []
    indeg = []
    for g, d in enumerate(items):
        n, e = nn[g], ne[g]
        for key, rows, width in (("positions", n, 3), ("shifts", e, 3)):
            if tuple(d[key].shape) != (rows, width):
                raise ValueError(f"graph {g}: {key} of shape {tuple(d[key].shape)}, expected {(rows, width)}")
        for key, rows, ref in (("node_attrs", n, first.node_attrs), ("edge_attr", e, first.edge_attr)):
            t = d[key]
            if t.dim() != 2 or t.shape[0] != rows or t.shape[1] != ref.shape[1]:
                raise ValueError(f"graph {g}: {key} of shape {tuple(t.shape)}; every graph needs "
                                 f"[{rows}, {ref.shape[1]}] (the field widths of graph 0)")
        if (("compliance" in d and torch.is_tensor(d.compliance)) != has_comp
                or ("rel_dens" in d and d.rel_dens is not None) != has_rel):
            raise ValueError(f"graph {g}: compliance / rel_dens must be carried by all graphs or by none")
        ei = d.edge_index.long()
        if e and (int(ei.min()) < 0 or int(ei.max()) >= n):
            raise ValueError(f"graph {g}: edge_index outside [0, {n})")
        csr = build_edge_csr(ei, n)
        cols["positions"].append(d.positions.float())
        cols["node_attrs"].append(d.node_attrs.float())
        cols["sender"].append(ei[0].to(torch.int32))
        cols["receiver"].append(ei[1].to(torch.int32))
        cols["shifts"].append(d.shifts.float())
        cols["edge_attr"].append(d.edge_attr.float())
        cols["perm"].append(csr["perm"].to(torch.int32))
        cols["sperm"].append(csr["sperm"])
        cols["rowend"].append(csr["rowptr"][1:])
        cols["srowend"].append(csr["srowptr"][1:])
        indeg.append(csr["rowptr"][1:] - csr["rowptr"][:-1])
        cols["stiffness"].append(_mandel_target(d.stiffness, "stiffness"))
        if has_comp:
            cols["compliance"].append(_mandel_target(d.compliance, "compliance"))
    tensors = {k: (torch.stack(v) if k in ("stiffness", "compliance") else torch.cat(v)).contiguous()
               for k, v in cols.items()}
    rel = None
    if has_rel:
        # what collate makes of the field: python numbers -> [G], tensors stacked on a new axis
        vals = [d.rel_dens for d in items]
        rel_t = torch.stack([v.reshape(-1) for v in vals]) if torch.is_tensor(vals[0]) else torch.tensor(vals)
        rel = rel_t.to(torch.float32).numpy().copy()
    deg = torch.cat(indeg).double()
    stats = {"lin": float(deg.mean()), "log": float(torch.log(deg + 1.0).mean())}
    rmax = float(tensors["edge_attr"].max()) if tensors["edge_attr"].numel() else 0.0
    return PackedGraphs(tensors, node_ptr, edge_ptr, [d.name for d in items] if has_name else None,
                        rel, rmax, stats)


class DeviceDataset(PackedGraphs):
    """``dataset`` (any indexable collection of untransformed ``Data`` items, e.g.
    ``GLAMM_Dataset(...).items`` after ``scale_targets`` or ``SyntheticLattices``) packed once into
    flat tensors on the HIP ``device``; ``indices`` selects and orders the graphs taken."""

    def __init__(self, dataset, device, indices: Optional[Sequence[int]] = None):
        dev = torch.device(device)
        if dev.type != "cuda":
            raise RuntimeError("the DeviceDataset / DeviceLoader batch assembly runs only on a HIP device "
                               f"(got device {str(dev)!r}); there is no CPU path")
        idx = range(len(dataset)) if indices is None else indices
        p = pack_graphs([dataset[int(i)] for i in idx]).to(dev)
        super().__init__(p.tensors, p.node_ptr, p.edge_ptr, p.names, p.rel_dens, p.max_edge_radius,
                         p._degree_stats)


def epoch_batches(num_items: int, batch_size: int, shuffle: bool = False, seed: int = 0, epoch: int = 0,
                  rank: int = 0, world: int = 1, drop_last: bool = False) -> List[np.ndarray]:
    """The graph ids of every batch of one epoch on ``rank`` (host arithmetic only).

    The epoch's order is ``gnn.data.DataLoader``'s: ``np.random.default_rng(seed + epoch)``'s
    permutation when ``shuffle``.  A global batch is ``batch_size * world`` consecutive graphs of
    that order and ``rank`` takes its ``rank``-th contiguous block of ``batch_size`` (the rule of
    ``parallel.shard_indices``).  ``world == 1``: the last batch is ragged unless ``drop_last``.
    ``world > 1``: a ragged last global batch wraps round to the start of the order
    (``shard_indices``' modulo), so every rank gets ``batch_size`` graphs at every step."""
    if batch_size < 1 or world < 1 or not 0 <= rank < world:
        raise ValueError(f"batch_size {batch_size}, rank {rank}, world {world}")
    order = np.arange(num_items, dtype=np.int64)
    if shuffle:
        order = np.random.default_rng(seed + epoch).permutation(num_items).astype(np.int64)
    glob = batch_size * world
    steps = num_items // glob if drop_last else (num_items + glob - 1) // glob
    out = []
    for s in range(steps):
        base = s * glob + rank * batch_size
        if world == 1:
            out.append(order[base: base + batch_size])
        else:
            out.append(order[(base + np.arange(batch_size)) % num_items])
    return out


class DeviceLoader:
    """Iterates ``Batch`` objects assembled on the device from a ``DeviceDataset``.

    Fields: those of ``collate(...).to(device)`` (``positions``, ``node_attrs``, ``edge_index``,
    ``shifts``, ``edge_attr``, ``stiffness``, optional ``compliance`` / ``rel_dens`` / ``name``,
    ``batch``, ``ptr``, ``num_graphs``, ``csr``) plus ``graph_ids`` (dataset indices, host int64)
    and ``rotation`` (the ``[B, 3, 3]`` fp32 device tensor used, or ``None``).

    Per batch the host does numpy arithmetic on the extents and one pinned, non-blocking copy of
    the slot table (and rotations); the device runs at most three launches on the current
    stream.  Nothing is sorted and nothing waits for the device.  With ``rotate`` the rotations
    of step ``s`` of epoch ``e`` come from ``rand_rotations`` seeded by (seed, e, s, rank)."""

    def __init__(self, dds: PackedGraphs, batch_size: int, shuffle: bool = False, seed: int = 0,
                 rotate: bool = False, rank: int = 0, world: int = 1, drop_last: bool = False):
        self.dds, self.batch_size, self.shuffle, self.seed = dds, int(batch_size), shuffle, int(seed)
        self.rotate, self.rank, self.world, self.drop_last = rotate, int(rank), int(world), drop_last
        self.epoch = 0
        epoch_batches(len(dds), self.batch_size, rank=self.rank, world=self.world)   # validates
        self._src = None

    def __len__(self) -> int:
        glob = self.batch_size * self.world
        n = len(self.dds)
        return n // glob if self.drop_last else (n + glob - 1) // glob

    def order(self, epoch: int) -> List[np.ndarray]:
        """Graph ids of every batch of ``epoch`` on this rank (no device work)."""
        return epoch_batches(len(self.dds), self.batch_size, self.shuffle, self.seed, epoch, self.rank,
                             self.world, self.drop_last)

    def rotations(self, epoch: int, step: int, n: int) -> torch.Tensor:
        """The fp64 ``[n, 3, 3]`` rotations of (``epoch``, ``step``): replayable."""
        state = np.random.SeedSequence([self.seed, epoch, step, self.rank]).generate_state(1, np.uint64)
        gen = torch.Generator().manual_seed(int(state[0]) & 0x7FFFFFFFFFFFFFFF)
        return rand_rotations(n, gen)

    def __iter__(self) -> Iterator[Batch]:
        epoch = self.epoch
        self.epoch += 1
        for step, ids in enumerate(self.order(epoch)):
            yield self.assemble(ids, self.rotations(epoch, step, len(ids)) if self.rotate else None)

    # ------------------------------------------------------------------------------------------
    def _source(self) -> "_lib.BatchSrc":
        if self._src is None:
            t = self.dds.tensors
            s = _lib.BatchSrc()
            for k in _NODE_T + _EDGE_T:
                setattr(s, k, t[k].data_ptr() or None)
            s.node_w, s.edge_w = t["node_attrs"].shape[1], t["edge_attr"].shape[1]
            s.total_nodes, s.total_edges = int(self.dds.node_ptr[-1]), int(self.dds.edge_ptr[-1])
            self._src = s
        return self._src

    def assemble(self, graph_ids, Q=None) -> Batch:
        """The collated batch of the graphs ``graph_ids`` (host integers; repeats allowed), each
        rotated by its ``Q`` (``[B, 3, 3]``, or one ``[3, 3]`` for all; host or device, any float
        dtype, used in fp32) or left as stored when ``Q`` is ``None``."""
        dds = self.dds
        dev = dds.device
        if dev.type != "cuda":
            raise RuntimeError("the DeviceDataset / DeviceLoader batch assembly runs only on a HIP device "
                               "(the graphs are packed on the CPU); build a DeviceDataset on 'cuda'")
        if torch.is_tensor(graph_ids):
            if graph_ids.is_cuda:
                raise TypeError("graph_ids are host integers (the batch's sizes come from the host extents)")
            graph_ids = graph_ids.numpy()
        ids = np.ascontiguousarray(np.asarray(graph_ids, dtype=np.int64).reshape(-1))
        nb = int(ids.shape[0])
        if nb < 1:
            raise ValueError("assemble: empty selection")
        if int(ids.min()) < 0 or int(ids.max()) >= len(dds):
            raise IndexError(f"graph ids outside [0, {len(dds)})")
        sn, se = dds.node_ptr[ids], dds.edge_ptr[ids]
        on = np.concatenate([[0], np.cumsum(dds.node_ptr[ids + 1] - sn)])
        oe = np.concatenate([[0], np.cumsum(dds.edge_ptr[ids + 1] - se)])
        n_nodes, n_edges = int(on[-1]), int(oe[-1])
        _check_extents(n_nodes, n_edges)
        # one staging buffer: slot table [4, B + 1] | graph ids [B] | rel_dens | rotations [B, 9]
        ld = nb + 1
        rel = dds.rel_dens[ids] if dds.rel_dens is not None else None
        q_host = None
        q_dev = None
        if Q is not None:
            if torch.is_tensor(Q) and Q.is_cuda:
                q_dev = Q.to(device=dev, dtype=torch.float32)
                q_dev = (q_dev.expand(nb, 3, 3) if q_dev.dim() == 2 else q_dev).contiguous()
            else:
                q_host = Q.detach().numpy() if torch.is_tensor(Q) else np.asarray(Q)
                q_host = np.broadcast_to(q_host.astype(np.float32), (nb, 3, 3))
            if tuple((q_dev if q_dev is not None else q_host).shape) != (nb, 3, 3):
                raise ValueError(f"Q must be [3, 3] or [{nb}, 3, 3]")
        o_rel = 4 * ld + nb
        o_rot = o_rel + (rel.size if rel is not None else 0)
        stage = np.zeros(o_rot + (9 * nb if q_host is not None else 0), dtype=np.int32)
        stage[0:ld], stage[ld:2 * ld] = on, oe
        stage[2 * ld:2 * ld + nb], stage[3 * ld:3 * ld + nb] = sn, se
        stage[4 * ld:o_rel] = ids
        if rel is not None:
            stage[o_rel:o_rot] = rel.reshape(-1).view(np.int32)
        if q_host is not None:
            stage[o_rot:] = np.ascontiguousarray(q_host).reshape(-1).view(np.int32)
        sdev = torch.from_numpy(stage).pin_memory().to(dev, non_blocking=True)
        if q_host is not None:
            q_dev = sdev[o_rot:].view(torch.float32).view(nb, 3, 3)

        t = dds.tensors
        f32, i32, i64 = torch.float32, torch.int32, torch.int64

        def new(shape, dtype):
            return torch.empty(shape, device=dev, dtype=dtype)
        b = Batch()
        b.positions = new((n_nodes, 3), f32)
        b.node_attrs = new((n_nodes, t["node_attrs"].shape[1]), f32)
        b.edge_index = new((2, n_edges), i64)
        b.shifts = new((n_edges, 3), f32)
        b.edge_attr = new((n_edges, t["edge_attr"].shape[1]), f32)
        b.stiffness = new((nb, 6, 6), f32)
        if "compliance" in t:
            b.compliance = new((nb, 6, 6), f32)
        if rel is not None:
            b.rel_dens = sdev[o_rel:o_rot].view(torch.float32).view(rel.shape)
        if dds.names is not None:
            b.name = [dds.names[i] for i in ids]
        b.batch = new((n_nodes,), i64)
        b.ptr = new((nb + 1,), i64)
        b.num_graphs = nb
        b.csr = {"perm": new((n_edges,), i64), "rowptr": new((n_nodes + 1,), i32),
                 "sender": new((n_edges,), i32), "receiver": new((n_edges,), i32),
                 "sperm": new((n_edges,), i32), "srowptr": new((n_nodes + 1,), i32)}
        b.graph_ids = ids
        b.rotation = q_dev
        out = _lib.BatchOut()
        for k in ("positions", "node_attrs", "batch", "ptr", "edge_index", "shifts", "edge_attr"):
            setattr(out, k, getattr(b, k).data_ptr() or None)
        for k in ("rowptr", "srowptr", "perm", "sperm", "sender", "receiver"):
            setattr(out, k, b.csr[k].data_ptr() or None)
        lib = _lib.load()
        with torch.cuda.device(dev):
            _lib.launch("batch_assemble", lib.eelg_batch_assemble, self._source(), sdev, q_dev, nb, n_nodes,
                         n_edges, out, on=b.positions, timed="batch_assemble")
            sel = sdev[4 * ld:o_rel]
            for key in ("stiffness", "compliance"):
                if key in t:
                    _lib.launch("mandel_rotate", lib.eelg_mandel_rotate, t[key], len(dds), sel, q_dev, nb,
                                 getattr(b, key), on=b.positions, timed="mandel_rotate")
        return b
