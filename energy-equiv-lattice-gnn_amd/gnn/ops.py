"""PyTorch autograd wrappers over the C ABI (``include/eelg.h``).

Every op requires HIP device tensors and launches on the current stream.
There is no eager/CPU fallback: a missing library or a CPU tensor raises.
"""
from __future__ import annotations

import contextlib
import ctypes
import math
import os
import weakref
from dataclasses import dataclass
from typing import Dict, Optional

import torch

from . import _lib


# the one launch path and its timer live in the leaf module; these names stay for callers
KernelTimer, TIMER, _launch = _lib.KernelTimer, _lib.TIMER, _lib.launch

# side-stream overlap of independent work (radial MLPs, symmetric-contraction coefficient
# chain and its gradient); EELG_OVERLAP=0 runs everything in line on the current stream
OVERLAP = os.environ.get("EELG_OVERLAP", "1") != "0"
# GNN_Head: the last layer and the readout compute only the irreps the stiffness linear can
# read (1), or everything as the reference does (0)
LIVE_OUT = os.environ.get("EELG_LIVE_OUT", "1") != "0"
SC_CMAJOR_ON_SIDE = os.environ.get("EELG_SC_CMAJOR_SIDE", "0") != "0"   # measured equal; fused keeps fewer bytes
# the contraction's coefficient gradient on the coefficient side stream (1) or in line (0)
SC_COEF_ON_SIDE = os.environ.get("EELG_SC_COEF_SIDE", "1") != "0"
# radial MLP backward (hidden 64): the chain kernel + weight gradients on the linear kernels (1),
# or the fused small-layer kernel with per-workgroup partials (0)
RADIAL_CHAIN = os.environ.get("EELG_RADIAL_CHAIN", "1") != "0"
# TP backward in sender order (eelg_tp_bwd_sender) instead of per-edge gxe + sender segment sum:
# "1" always, "0" never (default), "auto" for bf16 storage only.  fp32: measured slower (r02s1:
# tp_bws 1.40 ms vs tp_bwd 1.05 + sender sum 0.16 ms; 1832 vs 1862 graphs/s) -- each edge
# gathers its receiver's 29 KB grad_agg row out of receiver order.  bf16 storage (config 5):
# equal speed in round 2 (r02s2: 912.1 vs 912.4 graphs/s), so "auto" was the default, summing
# grad_x in fp32 instead of from per-edge terms rounded to bf16; with round 3-6's edge kernel
# (deeper prefetch, XCD-ordered blocks) the edge path is faster (r08m, two alternating pairs:
# 1145.6 / 1143.7 vs 1130.0 / 1127.9 graphs/s; tp_bwd 1.90 vs tp_bws 2.23 ms per launch)
_TBS = os.environ.get("EELG_TP_BWD_SENDER", "0")
TP_BWD_SENDER = None if _TBS == "auto" else _TBS != "0"
# edge-order backward: gxe rows stored at their sender-order position (eelg_tp_bwd_sorted), so
# the sender sum reads them contiguously instead of gathering through sperm.  Bitwise-equal
# results; measured equal (r02s3: sender sum 169 -> 137 us, tp_bwd 1036 -> 1128 us from the
# scattered row stores; 1844 / 1855 vs 1844 / 1847 graphs/s), so off by default.
TP_BWD_SPOS = os.environ.get("EELG_TP_BWD_SPOS", "0") != "0"
# fused backward of the interaction's output linear and the TP (eelg_tp_bwd_fused): the
# linear's grad-x [N, dmid] is computed per receiver tile into LDS inside the TP backward instead
# of being written to HBM by the linear and read back by tp_bwd.  Measured slower (r09c kbench:
# 1.10 ms vs 0.68 + 0.32 ms for tp_bwd + the linear's grad-x; r09a step 2002 vs ~2190 graphs/s):
# the per-tile MFMA stage is latency-bound at the occupancy its LDS block allows.  Off by default.
TP_BWF = os.environ.get("EELG_TP_BWF", "0") != "0"
# the output linear's grad-x and tp_bwd in C node chunks (C > 1): each chunk's grad_agg rows
# (N / C x 29 KB) are read back by tp_bwd right after the linear wrote them, from the 256 MB
# MALL instead of HBM (chunk edge ranges from one host read of the CSR, cached per graph).
# Bitwise equal to the one-pass kernels; measured slower (r09g, same box, default 2205 / 2200
# graphs/s: C 4 2171, C 8 2121, C 16 2007) -- each extra launch pair adds two kernel tails.
TP_BWC = int(os.environ.get("EELG_TP_BWC", "0"))
# one radial weight row per strut instead of one per directed edge (StrutMap, strut_rows): the
# two directions of a strut have bitwise-equal edge features, so the radial MLP runs on the S
# representative rows and tp_fwd / tp_bwd index them (eelg_tp_fwd_rows / eelg_tp_bwd_rows).
# 0 keeps the per-edge path (A/B runs, tests)
STRUT_WEIGHTS = os.environ.get("EELG_STRUT_WEIGHTS", "1") != "0"
_SIDE: Dict[tuple, "torch.cuda.Stream"] = {}


def side_stream(device, which: int = 0) -> "torch.cuda.Stream":
    """Side stream ``which`` of ``device``: 0 = radial MLPs, 1 = contraction coefficients,
    2 = linear weight gradients."""
    idx = torch.device(device).index
    idx = torch.cuda.current_device() if idx is None else idx
    if (idx, which) not in _SIDE:
        _SIDE[(idx, which)] = torch.cuda.Stream(device=torch.device("cuda", idx))
    return _SIDE[(idx, which)]


def _require_device(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise RuntimeError("the EnergyEquivGNN hot path runs only on a HIP device "
                               "(got a CPU tensor); move the model and batch to 'cuda'")


def _f32(t: torch.Tensor) -> torch.Tensor:
    if t.dtype != torch.float32:
        raise TypeError(f"expected float32, got {t.dtype}")
    return t.contiguous()


def _a16(t: torch.Tensor) -> torch.Tensor:
    """contiguous fp32 with a 16-byte aligned data pointer (float4 row access), copying a
    misaligned view"""
    t = _f32(t)
    return t if t.data_ptr() % 16 == 0 else t.clone()


def _i32(t: torch.Tensor) -> torch.Tensor:
    return t.to(torch.int32).contiguous()


# ---------------------------------------------------------------------------
# edge graph in receiver-sorted order
# ---------------------------------------------------------------------------
@dataclass
class StrutMap:
    """Which receiver-sorted edges are the two directions of one strut (``build_strut_map``).

    ``partner`` [E] int64: the edge with swapped endpoints, the exactly negated edge vector and
    the bitwise-equal radius, or the edge itself when there is none (or no unique one); it defines
    the map and nothing on the hot path reads it.  Paired edges share weight row ``row[e]``; every
    other edge has a row of its own.  ``row`` [E] int32 is the index ``eelg_tp_fwd_rows`` /
    ``eelg_tp_bwd_rows`` / ``eelg_radial_bwd_chain_rows`` take.  ``rep`` [S] int64: the
    representative (first) edge of each row, ascending."""
    partner: torch.Tensor
    row: torch.Tensor
    rep: torch.Tensor
    n_rows: int

    @property
    def num_edges(self) -> int:
        return int(self.row.shape[0])

    def rep_rows(self, feats: torch.Tensor) -> torch.Tensor:
        """``feats[rep]`` [S, n_feat], gathered once per feature tensor: every layer's radial MLP
        of a forward reads the same rows.  The memo holds ``feats`` weakly and its version."""
        memo = getattr(self, "_rep_rows", None)
        if memo is not None and memo[0]() is feats and memo[1] == feats._version:
            return memo[2]
        rows = feats[self.rep]
        self._rep_rows = (weakref.ref(feats), feats._version, rows)
        return rows


def _key_bits(v: torch.Tensor) -> torch.Tensor:
    """fp32 -> int64 bit patterns with -0.0 folded into +0.0 (``x + 0.0``)"""
    return (v + 0.0).contiguous().view(torch.int32).to(torch.int64)


def build_strut_map(pos: torch.Tensor, sender: torch.Tensor, receiver: torch.Tensor,
                    shifts_sorted: torch.Tensor, radius_sorted: torch.Tensor) -> StrutMap:
    """``StrutMap`` of a batch (plain torch, any device; one host sync for the row count).

    Edge e's key is (sender, receiver, edge vector, radius) with the vector formed as
    ``eelg_edge_embed`` forms it, ``(pos[r] - pos[s]) + shift`` in fp32; its partner is the
    edge whose key is (receiver, sender, -vector, radius).  The negation is exact in IEEE
    arithmetic, so partners have bitwise-equal lengths and hence bitwise-equal edge features.
    Several images of a strut between one node pair differ in their vectors and pair up
    separately.  An edge whose key, or whose partner's key, occurs more than once stays alone."""
    e = int(sender.shape[0])
    dev = sender.device
    ar = torch.arange(e, device=dev)
    if e == 0:
        z = torch.zeros(0, device=dev, dtype=torch.int64)
        return StrutMap(z, z.to(torch.int32), z, 0)
    s, r = sender.long(), receiver.long()
    pos = pos.detach().to(torch.float32)
    vec = (pos[r] - pos[s]) + shifts_sorted.detach().to(torch.float32)
    rad = _key_bits(radius_sorted.detach().to(torch.float32).reshape(e, 1))
    fwd = torch.cat([s[:, None], r[:, None], _key_bits(vec), rad], 1)
    rev = torch.cat([r[:, None], s[:, None], _key_bits(-vec), rad], 1)
    _, inv = torch.unique(torch.cat([fwd, rev]), dim=0, return_inverse=True)
    kf, kr = inv[:e], inv[e:]
    nk = int(inv.max()) + 1
    cnt = torch.zeros(nk, device=dev, dtype=torch.int64).index_add_(0, kf, torch.ones_like(kf))
    owner = torch.full((nk,), -1, device=dev, dtype=torch.int64)
    owner[kf] = ar                                  # read only where the key has one owner
    cand = owner[kr]
    ok = (cnt[kf] == 1) & (cnt[kr] == 1) & (cand >= 0)
    partner = torch.where(ok, cand, ar)
    is_rep = partner >= ar
    rep = torch.nonzero(is_rep).reshape(-1)
    row_of = torch.cumsum(is_rep.to(torch.int64), 0) - 1
    row = row_of[torch.minimum(partner, ar)].to(torch.int32)
    return StrutMap(partner, row.contiguous(), rep, int(rep.shape[0]))


@dataclass
class EdgeCSR:
    """Edges in receiver-sorted order.

    ``perm`` maps the sorted order back to the caller's edge order
    (``sorted_edge_j = original_edge[perm[j]]``).  ``rowptr`` is the receiver
    CSR; ``sperm`` / ``srowptr`` group the sorted edges by sender.  ``strut``: the batch's
    ``StrutMap`` where ``EnergyEquivGNN.edge_graph`` built one."""
    perm: torch.Tensor
    sender: torch.Tensor
    receiver: torch.Tensor
    rowptr: torch.Tensor
    sperm: torch.Tensor
    srowptr: torch.Tensor
    num_nodes: int
    strut: Optional[StrutMap] = None

    @property
    def num_edges(self) -> int:
        return int(self.sender.shape[0])

    def sender_pos(self) -> torch.Tensor:
        """[E] int32 inverse of ``sperm``: the sender-order position of each edge (cached)."""
        sp = getattr(self, "_spos", None)
        if sp is None:
            sp = torch.empty_like(self.sperm)
            sp[self.sperm.long()] = torch.arange(self.sperm.shape[0], device=self.sperm.device,
                                                 dtype=self.sperm.dtype)
            self._spos = sp
        return sp

    @staticmethod
    def from_dict(d: Dict, num_nodes: int) -> "EdgeCSR":
        return EdgeCSR(d["perm"], d["sender"], d["receiver"], d["rowptr"], d["sperm"],
                       d["srowptr"], num_nodes)

    @staticmethod
    def build(edge_index: torch.Tensor, num_nodes: int) -> "EdgeCSR":
        from .data import build_edge_csr
        return EdgeCSR.from_dict(build_edge_csr(edge_index, num_nodes), num_nodes)


# ---------------------------------------------------------------------------
# edge embedding.  In training positions and radii are data and this is one launch
# outside autograd; when any of them requires grad it is an autograd function whose backward
# is eelg_edge_embed_bwd + two segment sums (geometry gradients)
# ---------------------------------------------------------------------------
def edge_embed(pos, csr: EdgeCSR, shifts_sorted, radius_sorted, lmax: int, nb: int,
               len_end: float, rad_end: float):
    _require_device(pos, shifts_sorted, radius_sorted)
    if torch.is_grad_enabled() and (pos.requires_grad or shifts_sorted.requires_grad
                                    or radius_sorted.requires_grad):
        return _EdgeEmbed.apply(pos, shifts_sorted, radius_sorted, csr, lmax, nb, float(len_end),
                                float(rad_end))
    return _edge_embed_fwd(pos, csr, shifts_sorted, radius_sorted, lmax, nb, len_end, rad_end)


def _edge_embed_fwd(pos, csr: EdgeCSR, shifts_sorted, radius_sorted, lmax: int, nb: int,
                    len_end: float, rad_end: float):
    e = csr.num_edges
    nsh = (lmax + 1) ** 2
    sh = torch.empty(e, sh_row_stride(nsh), device=pos.device, dtype=torch.float32)
    feats = torch.empty(e, 2 * nb, device=pos.device, dtype=torch.float32)
    _launch("edge_embed", _lib.load().eelg_edge_embed, _f32(pos), csr.sender, csr.receiver,
            _f32(shifts_sorted), _f32(radius_sorted), e, lmax, nb, float(len_end), float(rad_end),
            sh, feats, on=sh)
    return sh[:, :nsh], feats          # [E, nsh] view of the padded rows the TP kernels read


class _EdgeEmbed(torch.autograd.Function):
    """``edge_embed`` over (positions, sorted shifts, sorted radii).  Backward: one thread per
    edge turns (grad_sh, grad_feats) into the edge vector's gradient and the radius gradient
    (``eelg_edge_embed_bwd``); the node gradient is the receiver sum minus the sender sum of the
    edge-vector gradients (``eelg_segment_sum_csr`` twice: fixed order, no atomics)."""

    @staticmethod
    def forward(ctx, pos, shifts_sorted, radius_sorted, csr: EdgeCSR, lmax, nb, len_end, rad_end):
        pos, shifts_sorted, radius_sorted = _f32(pos), _f32(shifts_sorted), _f32(radius_sorted)
        ctx.save_for_backward(pos, shifts_sorted, radius_sorted)
        ctx.csr, ctx.args = csr, (lmax, nb, len_end, rad_end)
        sh, feats = _edge_embed_fwd(pos, csr, shifts_sorted, radius_sorted, lmax, nb, len_end, rad_end)
        if not (ctx.needs_input_grad[0] or ctx.needs_input_grad[1]):
            # only the radii require grad: the SH do not depend on them, so they carry no grad and
            # the layers launch no tp_bwd_sh for a gradient nobody reads
            ctx.mark_non_differentiable(sh)
        return sh, feats

    @staticmethod
    def backward(ctx, gsh, gfeats):
        pos, shifts, radius = ctx.saved_tensors
        csr = ctx.csr
        lmax, nb, len_end, rad_end = ctx.args
        e = csr.num_edges
        gsh, gfeats = _strided_rows(gsh), _f32(gfeats)
        gvec = torch.empty(e, 4, device=pos.device, dtype=torch.float32)
        grad = torch.empty(e, device=pos.device, dtype=torch.float32)
        _launch("edge_embed_bwd", _lib.load().eelg_edge_embed_bwd, pos, csr.sender, csr.receiver,
                shifts, radius, e, lmax, nb, len_end, rad_end, gsh,
                int(gsh.stride(0)) if e else (lmax + 1) ** 2, gfeats, gvec, grad, on=gvec,
                timed="edge_embed_bwd")
        gpos = None
        if ctx.needs_input_grad[0]:
            n = csr.num_nodes
            if e:
                gpos = (segment_sum_csr(gvec, csr.rowptr, n)
                        - segment_sum_csr(gvec, csr.srowptr, n, idx=csr.sperm))[:, :3]
            else:
                gpos = torch.zeros_like(pos)
        return (gpos, gvec[:, :3] if ctx.needs_input_grad[1] else None,
                grad.view_as(radius) if ctx.needs_input_grad[2] else None, None, None, None, None, None)


def _strided_rows(t: torch.Tensor) -> torch.Tensor:
    """fp32 rows with unit column stride (a column slice of padded rows passes as it is)"""
    if t.dtype != torch.float32:
        raise TypeError(f"expected float32, got {t.dtype}")
    if t.dim() == 2 and t.stride(1) == 1 and t.stride(0) >= t.shape[1]:
        return t
    return t.contiguous()


class _PermuteRows(torch.autograd.Function):
    """``t[perm]`` for a permutation ``perm``; the backward writes every row back to its place
    (a plain scatter without accumulation, where indexing's autograd runs an accumulating
    index_put)."""

    @staticmethod
    def forward(ctx, t, perm):
        ctx.save_for_backward(perm)
        return t[perm]

    @staticmethod
    def backward(ctx, g):
        (perm,) = ctx.saved_tensors
        out = torch.empty_like(g)
        out[perm] = g
        return out, None


def permute_rows(t: torch.Tensor, perm: torch.Tensor) -> torch.Tensor:
    """``t[perm]`` (``perm`` a permutation of the rows), differentiable without accumulation"""
    if torch.is_grad_enabled() and t.requires_grad:
        return _PermuteRows.apply(t, perm)
    return t[perm]


def sh_row_stride(nsh: int) -> int:
    """SH rows are padded to 16 bytes in HBM (float4 loads in the TP kernels)."""
    return (nsh + 3) // 4 * 4


def padded_sh(sh: torch.Tensor) -> torch.Tensor:
    """The padded-row buffer behind ``sh`` ([E, nsh]): the tensor itself when it is already a
    view of padded rows (as ``edge_embed`` returns), else a padded copy."""
    nsh = sh.shape[1]
    nshp = sh_row_stride(nsh)
    if (sh.dtype == torch.float32 and sh.stride() == (nshp, 1) and sh.storage_offset() == 0
            and sh.untyped_storage().nbytes() >= sh.shape[0] * nshp * 4):
        return sh
    out = torch.zeros(sh.shape[0], nshp, device=sh.device, dtype=torch.float32)
    out[:, :nsh] = sh
    return out[:, :nsh]


# ---------------------------------------------------------------------------
# CSR segmented sum
# ---------------------------------------------------------------------------
def segment_sum_csr(src, rowptr, n_rows: int, idx=None, row_scale=None, scale: float = 1.0):
    """fp32 output; ``src`` is fp32, or bf16 (widened exactly, fp32 accumulation)."""
    _require_device(src)
    bf = src.dtype == torch.bfloat16
    src = src.contiguous() if bf else _f32(src)
    width = src[0].numel() if src.shape[0] > 0 else int(torch.tensor(src.shape[1:]).prod())
    out = torch.empty((n_rows,) + tuple(src.shape[1:]), device=src.device, dtype=torch.float32)
    lib = _lib.load()
    fn = lib.eelg_segment_sum_csr_bf16 if bf else lib.eelg_segment_sum_csr
    _launch("segment_sum_csr", fn, src, rowptr, idx, row_scale, float(scale), n_rows, int(width), out,
            on=out)
    return out


def segment_sum_long(src: torch.Tensor, rowptr: torch.Tensor, n_rows: int,
                     row_scale: Optional[torch.Tensor] = None, scale: float = 1.0) -> torch.Tensor:
    """``segment_sum_csr`` for few long segments (graph pooling): each segment is split
    into pieces summed in parallel, then combined in a fixed order (deterministic)."""
    _require_device(src)
    src = _f32(src)
    width = src.shape[1]
    n_split = max(1, min(64, -(-2048 // max(n_rows, 1))))
    work = torch.empty(n_rows, n_split, width, device=src.device, dtype=torch.float32)
    out = torch.empty(n_rows, width, device=src.device, dtype=torch.float32)
    _launch("segment_sum_split", _lib.load().eelg_segment_sum_split, src, rowptr, None, row_scale,
            float(scale), n_rows, width, n_split, work, out, on=out, timed="segment_sum_split")
    return out


class _SegmentMean(torch.autograd.Function):
    """Per-graph mean/sum pool over sorted ``batch`` (``gnn/model.py:100-106``)."""

    @staticmethod
    def forward(ctx, src, ptr32, batch, inv_cnt):
        ctx.save_for_backward(batch, inv_cnt)
        n_rows = ptr32.shape[0] - 1
        if src.shape[0] >= 64 * max(n_rows, 1):          # long segments: split them
            return segment_sum_long(src, ptr32, n_rows, row_scale=inv_cnt)
        return segment_sum_csr(src, ptr32, n_rows, row_scale=inv_cnt)

    @staticmethod
    def backward(ctx, g):
        batch, inv_cnt = ctx.saved_tensors
        return (g * inv_cnt[:, None])[batch], None, None, None


def graph_pool(src, batch, num_graphs: int, reduce: str = "mean"):
    _require_device(src)
    # ``batch`` is sorted (PyG collation), so the segment bounds are a searchsorted: no
    # device -> host sync (bincount sizes its output from the data and would stall the host)
    bounds = torch.arange(num_graphs + 1, device=batch.device, dtype=batch.dtype)
    ptr = torch.searchsorted(batch, bounds).to(torch.int32)
    cnt = (ptr[1:] - ptr[:-1]).to(torch.int64)
    if reduce == "mean":
        inv = 1.0 / cnt.clamp_min(1).to(torch.float32)
    elif reduce in ("sum", "add"):
        inv = torch.ones(num_graphs, device=src.device, dtype=torch.float32)
    elif reduce in ("max", "min", "mul"):
        return segment_pool_order(src, ptr, num_graphs, reduce)
    else:
        raise ValueError(f"global_reduction {reduce!r} not supported "
                         "(torch_scatter reduces: sum, add, mean, max, min, mul)")
    return _SegmentMean.apply(src, ptr, batch, inv)


_ORDER_OPS = {"max": 0, "min": 1, "mul": 2}


class _SegmentOrder(torch.autograd.Function):
    """torch_scatter ``scatter(..., reduce='max'|'min'|'mul')`` over CSR segments of ``src``
    rows (``eelg_segment_order``).  max / min: the first extreme of a segment is kept and the
    whole gradient goes to it (torch_scatter's scatter_max / scatter_min arg); empty segments
    give 0 (max / min) or 1 (mul), as torch_scatter fills rows that receive nothing."""

    @staticmethod
    def forward(ctx, src, rowptr, n_rows: int, op: int, covered: bool):
        src = _f32(src)
        width = src.shape[1]
        out = torch.empty(n_rows, width, device=src.device, dtype=torch.float32)
        arg = (torch.empty(n_rows, width, device=src.device, dtype=torch.int32)
               if op != _ORDER_OPS["mul"] else None)
        _launch("segment_order", _lib.load().eelg_segment_order, src, rowptr, n_rows, width, op, out,
                arg, on=out)
        ctx.save_for_backward(src, rowptr, arg)
        ctx.n_rows, ctx.op, ctx.covered = n_rows, op, covered
        return out

    @staticmethod
    def backward(ctx, g):
        src, rowptr, arg = ctx.saved_tensors
        g = _f32(g)
        # every row of every segment is written; rows outside all segments must read 0
        gs = torch.empty_like(src) if ctx.covered else torch.zeros_like(src)
        _launch("segment_order_bwd", _lib.load().eelg_segment_order_bwd, src, rowptr, arg, g,
                ctx.n_rows, src.shape[1], ctx.op, gs, on=gs)
        return gs, None, None, None, None


def segment_order(src, rowptr32, n_rows: int, reduce: str, covered: bool = False):
    """``reduce`` in max / min / mul over the CSR segments ``rowptr32`` (int32, [n_rows + 1]).
    ``covered``: the segments cover every row of ``src`` (the backward then skips a zero fill)."""
    _require_device(src)
    if reduce not in _ORDER_OPS:
        raise ValueError(f"segment_order: reduce {reduce!r} (max, min, mul)")
    return _SegmentOrder.apply(src, rowptr32, n_rows, _ORDER_OPS[reduce], covered)


def segment_pool_order(src, ptr32, num_graphs: int, reduce: str):
    """Per-graph max / min / mul pool (``gnn/model.py:100-106`` passes any torch_scatter
    reduce) over the sorted ``batch`` segments ``ptr32``."""
    return segment_order(src, ptr32, num_graphs, reduce)


# ---------------------------------------------------------------------------
# principal-neighbourhood aggregation (interaction_reduction = 'pna')
# ---------------------------------------------------------------------------
# the fused segment kernels (1), or the composition of the segment sums, the order reductions
# and torch elementwise ops with the reference's [N, D, 12] stack (0): the memory / time
# baseline and a second implementation (tools/pna_bench.py, tests/test_gpu_pna.py)
PNA_FUSED = os.environ.get("EELG_PNA_FUSED", "1") != "0"
PNA_EPS = 1e-5


def pna_scalers(rowptr32: torch.Tensor, avg_log: float) -> torch.Tensor:
    """[N, 3] fp32 degree scalers of ``PNASimple`` (``gnn/pna.py:20-31``) from the in-degree of
    the CSR: identity 1, amplification ``log(deg + 1) / avg_log``, attenuation
    ``avg_log / log(deg + 1)`` (1 where ``deg == 0``)."""
    deg = (rowptr32[1:] - rowptr32[:-1]).to(torch.float32)
    lg = torch.log(deg + 1.0)
    amp = lg / float(avg_log)
    att = torch.where(deg == 0, torch.ones_like(lg), float(avg_log) / lg.clamp_min(1e-30))
    return torch.stack([torch.ones_like(lg), amp, att], 1).contiguous()


class PNAArgs:
    """The rows ``segment_pna`` kept as minimum / maximum: ``argmin`` / ``argmax`` [n_rows, width]
    int32 positions in ``src`` (-1 for an empty segment), filled by the call they were passed to."""
    argmin: Optional[torch.Tensor] = None
    argmax: Optional[torch.Tensor] = None


class _SegmentPNA(torch.autograd.Function):
    """``PNASimple.forward`` (``gnn/blocks.py:817-848``) over CSR segments of ``src`` rows on
    ``eelg_segment_pna_fwd`` / ``_bwd``.  The 12 weights enter through the per-receiver
    coefficients ``coef[n, k] = sum_s W[3k + s] scalers[n, s]``; their gradient is the fixed-order
    column sum of ``grad_coef[n, k] scalers[n, s]`` (``sum_rows``).  Saved: ``src`` and four
    [n_rows, width] buffers; nothing 12-fold is formed."""

    @staticmethod
    def forward(ctx, src, weight, rowptr, scalers, n_rows: int, args):
        src = _a16(src)
        width = src.shape[1]
        dev = src.device
        w43 = weight.detach().to(torch.float32).reshape(4, 3)
        coef = (scalers[:, None, :] * w43[None]).sum(-1).contiguous()       # [N, 4]
        out = torch.empty(n_rows, width, device=dev, dtype=torch.float32)
        mean, std = torch.empty_like(out), torch.empty_like(out)
        amin = torch.empty(n_rows, width, device=dev, dtype=torch.int32)
        amax = torch.empty_like(amin)
        # no edges: the kernel reads no row of src, but takes no null pointer
        s = src if src.numel() else torch.zeros(4, device=dev, dtype=torch.float32)
        _launch("segment_pna_fwd", _lib.load().eelg_segment_pna_fwd, s, rowptr, coef, n_rows, width,
                out, mean, std, amin, amax, on=out, timed="segment_pna_fwd")
        if args is not None:
            args.argmin, args.argmax = amin, amax
        ctx.save_for_backward(src, rowptr, scalers, coef, mean, std, amin, amax)
        ctx.n_rows, ctx.wshape = n_rows, weight.shape
        return out

    @staticmethod
    def backward(ctx, g):
        src, rowptr, scalers, coef, mean, std, amin, amax = ctx.saved_tensors
        g = _a16(g)
        n_rows, width = ctx.n_rows, src.shape[1]
        lib = _lib.load()
        parts = lib.eelg_segment_pna_parts(width)
        gs = torch.empty_like(src)      # every row is in one segment: written once, no zero fill
        part = torch.empty(parts, n_rows * 4, device=src.device, dtype=torch.float32)
        s = src if src.numel() else torch.zeros(4, device=src.device, dtype=torch.float32)
        o = gs if gs.numel() else torch.empty(4, device=src.device, dtype=torch.float32)
        _launch("segment_pna_bwd", lib.eelg_segment_pna_bwd, s, rowptr, coef, mean, std, amin, amax,
                g, n_rows, width, o, part, on=part, timed="segment_pna_bwd")
        gw = None
        if ctx.needs_input_grad[1]:
            gcoef = (part[0] if parts == 1 else sum_rows(part)).view(n_rows, 4)
            # grad W[3k + s] = sum_n grad_coef[n, k] scalers[n, s], rows summed in a fixed order
            gw = sum_rows((gcoef[:, :, None] * scalers[:, None, :]).reshape(n_rows, 12)).view(ctx.wshape)
        return (gs if ctx.needs_input_grad[0] else None), gw, None, None, None, None


class _SegmentSum(torch.autograd.Function):
    """``segment_sum_csr`` over segments that cover the rows of ``src``, differentiable in
    ``src`` (the backward repeats each segment's gradient row over its rows)."""

    @staticmethod
    def forward(ctx, src, rowptr, n_rows: int):
        ctx.save_for_backward(rowptr)
        ctx.n_src = src.shape[0]
        return segment_sum_csr(src, rowptr, n_rows)

    @staticmethod
    def backward(ctx, g):
        (rowptr,) = ctx.saved_tensors
        return g[_segment_index(rowptr, ctx.n_src)], None, None


def _segment_index(rowptr: torch.Tensor, n_src: int) -> torch.Tensor:
    """[n_src] int64 segment of every row (the segments cover the rows)"""
    deg = (rowptr[1:] - rowptr[:-1]).long()
    return torch.repeat_interleave(torch.arange(deg.shape[0], device=rowptr.device), deg,
                                   output_size=n_src)


def _segment_pna_composed(src, rowptr32, n_rows: int, weight, scalers, args):
    """``segment_pna`` from the ops that predate the fused kernels, autograd through all of it:
    four [N, D] aggregates, the [N, D, 12] stack of their scaled copies as the reference forms it
    (``gnn/blocks.py:835-847``), then the 12 weights.  The variance is centred like the kernel's."""
    src = _f32(src)
    idx = _segment_index(rowptr32, src.shape[0])
    deg = (rowptr32[1:] - rowptr32[:-1]).to(torch.float32)
    inv = (1.0 / deg.clamp_min(1.0))[:, None]
    mean = _SegmentSum.apply(src, rowptr32, n_rows) * inv
    d = src - mean[idx]
    std = torch.sqrt(_SegmentSum.apply(d * d, rowptr32, n_rows) * inv + PNA_EPS)
    mn = _SegmentOrder.apply(src, rowptr32, n_rows, _ORDER_OPS["min"], True)
    mx = _SegmentOrder.apply(src, rowptr32, n_rows, _ORDER_OPS["max"], True)
    if args is not None:            # the kept positions, from the same kernel on the same rows
        kept = {}
        for op in ("min", "max"):
            kept[op] = torch.empty(n_rows, src.shape[1], device=src.device, dtype=torch.int32)
            val = torch.empty(n_rows, src.shape[1], device=src.device, dtype=torch.float32)
            _launch("segment_order", _lib.load().eelg_segment_order, src.detach(), rowptr32, n_rows,
                    src.shape[1], _ORDER_OPS[op], val, kept[op], on=val)
        args.argmin, args.argmax = kept["min"], kept["max"]
    stack = torch.stack([a * scalers[:, None, s] for a in (mean, mn, mx, std) for s in range(3)], 2)
    return (stack * weight.reshape(12)).sum(-1)


def segment_pna(src, rowptr32, n_rows: int, weight, avg_log: float, scalers=None,
                args: Optional[PNAArgs] = None):
    """``PNASimple(avg_deg={'log': avg_log}).forward`` (``gnn/blocks.py:817-848``) of the rows
    ``src`` [E, width] over the CSR segments ``rowptr32`` (int32, [n_rows + 1], covering every row):
    ``out[n, c] = sum_k sum_s W[0, 3k + s] scale_s(deg_n) agg_k[n, c]`` with ``agg`` = (mean, min,
    max, std) and ``scale`` = (identity, amplification, attenuation); ``weight`` is the [1, 12]
    weight of ``post_pn``.  min / max keep the first extreme of a segment and route their whole
    gradient there; an empty segment gives ``coef_std * sqrt(1e-5)``.  ``scalers``:
    ``pna_scalers(rowptr32, avg_log)`` computed ahead (cached per graph by the block).  ``args``:
    a ``PNAArgs`` that receives the kept positions.  Differentiable in ``src`` and ``weight``;
    the backward is bitwise repeatable."""
    _require_device(src, weight)
    if src.dim() != 2 or src.shape[1] < 1:
        raise ValueError(f"segment_pna: src [E, width >= 1] expected, got {tuple(src.shape)}")
    if weight.numel() != 12:
        raise ValueError(f"segment_pna: the weight of Linear(12, 1), got {tuple(weight.shape)}")
    if rowptr32.dtype != torch.int32 or rowptr32.shape[0] != n_rows + 1:
        raise ValueError("segment_pna: rowptr32 is the int32 CSR [n_rows + 1]")
    if scalers is None:
        scalers = pna_scalers(rowptr32, avg_log)
    if not PNA_FUSED:
        return _segment_pna_composed(src, rowptr32, n_rows, weight, scalers, args)
    return _SegmentPNA.apply(src, weight, rowptr32.contiguous(), scalers, n_rows, args)


# ---------------------------------------------------------------------------
# fused interaction: gather -> uvu tensor product -> segmented sum / norm
# ---------------------------------------------------------------------------
class _TPInteraction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, sh, w, csr: EdgeCSR, cfg: int, info: Dict[str, int], inv_norm: float):
        # w: fp32, or bf16 storage (BASELINE config 5; fp32 arithmetic in the kernels)
        agg, x, sh, w = _tp_fwd(x, sh, w, csr, cfg, info, inv_norm)
        ctx.save_for_backward(x, sh, w)
        ctx.csr, ctx.cfg, ctx.info, ctx.inv_norm = csr, cfg, info, inv_norm
        return agg

    @staticmethod
    def backward(ctx, g):
        x, sh, w = ctx.saved_tensors
        return _tp_bwd(x, sh, w, ctx.csr, ctx.cfg, ctx.info, ctx.inv_norm, g,
                       want_sh=ctx.needs_input_grad[1]) + (None,) * 4


def _tp_bwd(x, sh, w, csr: EdgeCSR, cfg: int, info, inv_norm: float, g, want_sh: bool = False):
    """(grad_x, grad_sh or None, grad_w) of the interaction over per-edge weights, from the
    operands as ``_tp_fwd`` returned them: in sender order (``TP_BWD_SENDER``) or in edge order"""
    g = _f32(g)
    gw = torch.empty_like(w)                       # same storage type as w
    # the SH gradient (geometry gradients only): its own kernel, one padded row per edge
    gsh = _tp_bwd_sh(x, w, csr, cfg, info, inv_norm, g) if want_sh else None
    if TP_BWD_SENDER if TP_BWD_SENDER is not None else w.dtype == torch.bfloat16:
        return _tp_bwd_sender(x, sh, w, csr, cfg, info, inv_norm, g, gw), gsh, gw
    return _tp_bwd_edges(x, sh, w, csr, cfg, info, inv_norm, g, gw), gsh, gw


def _tp_bwd_sender(x, sh, w, csr: EdgeCSR, cfg: int, info, inv_norm: float, g, gw):
    """the sender-order launch: grad_x summed per sender in registers, no gxe round trip"""
    gx = torch.empty(csr.num_nodes, info["din"], device=x.device, dtype=torch.float32)
    lib = _lib.load()
    bws = lib.eelg_tp_bwd_sender_bf16 if w.dtype == torch.bfloat16 else lib.eelg_tp_bwd_sender
    _launch("tp_bwd_sender", bws, cfg, x, sh, w, csr.sperm, csr.srowptr, csr.receiver,
            csr.num_nodes, g, float(inv_norm), gw, gx, on=gx, timed=f"tp_bwd_sender[din={info['din']}]")
    return gx


def _tp_bwd_launch(x, sh, w, csr: EdgeCSR, cfg: int, info, inv_norm: float, g, gw, gxe,
                   row=None, spos=None, chunk=None) -> None:
    """THE edge-order backward launch (``eelg_tp_bwd_rows[_bf16]``): per-edge ``gw`` and ``gxe``
    ([E, wn] / [E, din], of ``w``'s dtype) from ``g`` [N, dmid].  ``row``: the weight row of each
    edge (``StrutMap.row``; None: ``w`` is per edge).  ``spos``: where each edge's ``gxe`` row
    goes (``EdgeCSR.sender_pos``; None: in place).  ``chunk`` = (n0, e0, e1): only the edges
    e0:e1, whose receivers start at node n0, ``g`` holding the rows from n0 on; the receiver
    indices are global, so ``g``'s address is offset back by n0 rows."""
    lib = _lib.load()
    bwd = lib.eelg_tp_bwd_rows_bf16 if w.dtype == torch.bfloat16 else lib.eelg_tp_bwd_rows
    e, per_edge = csr.num_edges, (sh, w, row, csr.sender, csr.receiver, g, gw, gxe)
    if chunk is not None:
        n0, e0, e1 = chunk
        e, esz = e1 - e0, w.element_size()
        off = (4 * e0 * sh.stride(0), esz * e0 * info["wn"], 4 * e0, 4 * e0, 4 * e0,
               -4 * n0 * info["dmid"], esz * e0 * info["wn"], esz * e0 * info["din"])
        per_edge = [None if t is None else t.data_ptr() + o for t, o in zip(per_edge, off)]
    sh, w, row, sender, receiver, g, gw, gxa = per_edge
    _launch("tp_bwd", bwd, cfg, x, sh, w, row, sender, receiver, spos, e, g, float(inv_norm), gw,
            gxa, on=gxe, timed=f"tp_bwd[din={info['din']}]")


def _tp_sender_sum(gxe, csr: EdgeCSR, spos=None):
    """grad_x [N, din] fp32: the sender segment sum of the per-edge ``gxe`` rows, which lie in
    sender order when the launch stored them through ``spos``, else gathered through ``sperm``"""
    return segment_sum_csr(gxe, csr.srowptr, csr.num_nodes, idx=None if spos is not None else csr.sperm)


def _tp_bwd_edges(x, sh, w, csr: EdgeCSR, cfg: int, info, inv_norm: float, g, gw, row=None):
    """grad_x of the edge-order backward (launch + sender sum, ``TP_BWD_SPOS`` read here); the
    per-edge weight gradient goes to ``gw``"""
    gxe = torch.empty(csr.num_edges, info["din"], device=x.device, dtype=w.dtype)
    spos = csr.sender_pos() if TP_BWD_SPOS else None
    _tp_bwd_launch(x, sh, w, csr, cfg, info, inv_norm, g, gw, gxe, row=row, spos=spos)
    return _tp_sender_sum(gxe, csr, spos)


def _tp_bwd_sh(x, w, csr: EdgeCSR, cfg: int, info, inv_norm: float, g):
    """``eelg_tp_bwd_sh``: grad of the interaction w.r.t. its SH operand, [E, nsh] (a view of the
    padded rows the kernel writes, pad = 0)"""
    if w.dtype != torch.float32:
        raise NotImplementedError("the SH gradient of the interaction takes fp32 TP weights; "
                                  "bf16 storage (storage_dtype='bfloat16') has no geometry gradients")
    e, nsh = csr.num_edges, info["nsh"]
    gsh = torch.empty(e, sh_row_stride(nsh), device=x.device, dtype=torch.float32)
    _launch("tp_bwd_sh", _lib.load().eelg_tp_bwd_sh, cfg, x, None, w, csr.sender, csr.receiver, e,
            g, float(inv_norm), gsh, on=gsh, timed=f"tp_bwd_sh[din={info['din']}]")
    return gsh[:, :nsh]


class StrutWeights:
    """The radial weights of a layer as one row per strut (``radial_mlp_shared``): ``w`` [S, W]
    (no autograd edge), the ``smap`` that indexes it, and the hand-over of its gradient.  The
    per-edge ``grad_w`` [E, W] that ``eelg_tp_bwd_rows`` writes is not of ``w``'s shape (and summing
    it per pair would be a new pass over an edge-sized tensor), so it cannot travel as ``w``'s
    autograd gradient: the TP backward leaves it in ``box.gw`` and returns
    a gradient for the one-element ``token`` instead, which is the radial MLP's differentiable
    output and so triggers (and orders, across streams) the MLP backward that takes ``gw``.

    Limits of this hand-over: one ``StrutWeights`` feeds exactly one ``tp_interaction`` and one
    backward pass (a second backward over a retained graph raises in the MLP's backward, which
    finds the box empty); with every MLP parameter frozen the token needs no gradient and the TP
    backward keeps nothing in the box."""

    def __init__(self, w, smap: StrutMap, token, box: "_GradBox"):
        self.w, self.smap, self.token, self.box = w, smap, token, box


class _GradBox:
    """where the TP backward leaves the per-edge ``grad_w`` for the radial MLP's backward (the
    two autograd nodes hold the box, not each other's tensors)"""
    gw: Optional[torch.Tensor] = None


_ZERO1: Dict[str, torch.Tensor] = {}


def _zero1(device) -> torch.Tensor:
    """a constant one-element zero on ``device`` (the token's gradient; never written)"""
    key = str(device)
    if key not in _ZERO1:
        _ZERO1[key] = torch.zeros(1, device=device, dtype=torch.float32)
    return _ZERO1[key]


class _TPInteractionRows(torch.autograd.Function):
    """``_TPInteraction`` over shared weight rows (``StrutWeights``): same kernels with the
    per-edge row index, bitwise the results of the expanded per-edge ``w[row]``."""

    @staticmethod
    def forward(ctx, x, sh, token, sw: StrutWeights, csr: EdgeCSR, cfg: int, info, inv_norm: float):
        agg, x, sh, w = _tp_fwd(x, sh, sw.w, csr, cfg, info, inv_norm, sw.smap)
        ctx.save_for_backward(x, sh, w)
        ctx.smap, ctx.box = sw.smap, sw.box
        ctx.csr, ctx.cfg, ctx.info, ctx.inv_norm = csr, cfg, info, inv_norm
        return agg

    @staticmethod
    def backward(ctx, g):
        x, sh, w = ctx.saved_tensors
        csr, info = ctx.csr, ctx.info
        gw = torch.empty(csr.num_edges, info["wn"], device=x.device, dtype=w.dtype)  # per edge, as ever
        gx = _tp_bwd_edges(x, sh, w, csr, ctx.cfg, info, ctx.inv_norm, _f32(g), gw, row=ctx.smap.row)
        if ctx.needs_input_grad[2]:                 # else nobody will take it: keep nothing alive
            ctx.box.gw = gw
        return gx, None, (_zero1(x.device) if ctx.needs_input_grad[2] else None), None, None, None, None, None


def tp_interaction(x, sh, w, csr: EdgeCSR, cfg: int, info: Dict[str, int], inv_norm: float):
    """``w``: the per-edge weights [E, W], or ``StrutWeights`` (one row per strut)"""
    if isinstance(w, StrutWeights):
        _require_device(x, sh, w.w)
        return _TPInteractionRows.apply(x, sh, w.token, w, csr, cfg, info, inv_norm)
    _require_device(x, sh, w)
    return _TPInteraction.apply(x, sh, w, csr, cfg, info, inv_norm)


def strut_rows(csr: EdgeCSR, reduce: str, storage, mlp: torch.nn.Sequential,
               *edge_tensors) -> Optional[StrutMap]:
    """THE predicate of the shared-row path: the ``StrutMap`` to compute a layer's radial
    weights on (``radial_mlp_shared``), or None for per-edge weights.  Shared rows serve the
    default training path only: the switch on, a map on the CSR that pairs some edges, the
    fused 'sum' / 'add' / 'mean' interaction with the per-edge backward (none of EELG_TP_BWF /
    EELG_TP_BWC / EELG_TP_BWD_SENDER), no geometry gradients (``edge_tensors``: the SH and the
    edge features), and the chain form of the MLP backward (hidden 64, one launch range)."""
    smap = csr.strut
    if not STRUT_WEIGHTS or smap is None or smap.num_edges != csr.num_edges:
        return None
    if smap.n_rows == 0 or smap.n_rows >= csr.num_edges:       # no pair: nothing to share
        return None
    if reduce not in ("sum", "add", "mean") or TP_BWF or TP_BWC > 1:
        return None
    if TP_BWD_SENDER or (TP_BWD_SENDER is None and storage == torch.bfloat16):
        return None
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in edge_tensors):
        return None
    lins = [m for m in mlp if isinstance(m, torch.nn.Linear)]
    if not RADIAL_CHAIN or any(m.out_features != 64 for m in lins[:-1]):
        return None
    n_out = -(-lins[-1].out_features // 8) * 8
    es = 2 if storage == torch.bfloat16 else 4
    if len(_radial_chunks(csr.num_edges, n_out, es, 64, len(lins) - 1)) != 1:
        return None
    return smap


def _tp_fwd(x, sh, w, csr: EdgeCSR, cfg: int, info: Dict[str, int], inv_norm: float,
            smap: Optional[StrutMap] = None):
    """tp_fwd launch with the input checks of ``_TPInteraction``; returns (agg, x, sh, w) with
    the operands as the kernels read them.  ``smap``: ``w`` holds its ``n_rows`` shared rows."""
    bf = w.dtype == torch.bfloat16
    x = _a16(x)
    if bf:
        w = w.contiguous()
        w = w if w.data_ptr() % 16 == 0 else w.clone()
    else:
        w = _a16(w)
    if sh.dtype != torch.float32:
        raise TypeError(f"expected float32 SH, got {sh.dtype}")
    sh = padded_sh(sh)
    n = x.shape[0]
    if x.shape[1] != info["din"] or sh.shape[1] != info["nsh"] or w.shape[1] != info["wn"]:
        raise ValueError(f"shape mismatch: x {tuple(x.shape)} sh {tuple(sh.shape)} "
                         f"w {tuple(w.shape)} vs config {info}")
    w_rows = csr.num_edges if smap is None else smap.n_rows
    if sh.shape[0] != csr.num_edges or w.shape[0] != w_rows or n != csr.num_nodes:
        raise ValueError("edge/node counts do not match the CSR")
    if smap is not None and smap.num_edges != csr.num_edges:
        raise ValueError("the strut map is not of this CSR")
    n_out = csr.rowptr.shape[0] - 1
    agg = torch.empty(n_out, info["dmid"], device=x.device, dtype=torch.float32)
    lib = _lib.load()
    fwd = lib.eelg_tp_fwd_rows_bf16 if bf else lib.eelg_tp_fwd_rows
    _launch("tp_fwd", fwd, cfg, x, sh, w, smap.row if smap is not None else None, csr.sender,
            csr.rowptr, n_out, float(inv_norm), agg, on=agg, timed=f"tp_fwd[din={info['din']}]")
    return agg, x, sh, w


def tp_linear_fusable(cfg: int, lin, paths) -> bool:
    """whether ``eelg_tp_bwd_fused`` serves ``lin(tp_interaction(...))`` for TP config ``cfg``:
    generated for it (mul 32), and its slot table (weight offset, alpha, gy offset per TP slot)
    equals what ``lin`` (an ``o3.Linear`` over the TP's output irreps) computes.  ``paths``:
    ``cg.tp_paths`` of the block (slot, l3, out_off).  Cached on the linear, per config (not by
    ``id()``: a freed linear's id can be reused by a new one)."""
    cache = lin.__dict__.setdefault("_bwf_ok", {})
    if cfg not in cache:
        cache[cfg] = _bwf_table_matches(cfg, lin, paths)
    return cache[cfg]


def _bwf_table_matches(cfg: int, lin, paths) -> bool:
    lib = _lib.load()
    wo, al, go = ctypes.c_int(), ctypes.c_float(), ctypes.c_int()
    if lin.bias_slots and any(lin.irreps_out[o].ir.l != 0 for o in lin.bias_slots):
        return False
    ins_of_in = {}
    for t, (i, o) in enumerate(lin.instructions):
        if i in ins_of_in:                 # an input block read by two outputs: not the TP layout
            return False
        ins_of_in[i] = (t, o)
    for p in paths:
        if lib.eelg_tp_bwf_slot(cfg, p.slot, ctypes.byref(wo), ctypes.byref(al), ctypes.byref(go)) != 0:
            return False
        hit = None
        for i, (mul, ir) in enumerate(lin.irreps_in):
            lo = lin._in_off[i]
            if lo <= p.out_off < lo + mul * ir.dim and ir.l == p.l3:
                hit = i
                break
        if hit is None or hit not in ins_of_in:
            return False
        t, o = ins_of_in[hit]
        d = 2 * p.l3 + 1
        q, rem = divmod(p.out_off - lin._in_off[hit], 32 * d)
        mo = lin.irreps_out[o].mul
        if rem or mo != 32 or p.mul != 32:
            return False
        if (wo.value != lin._w_offs[t] + q * 32 * mo or go.value != lin._out_off[o]
                or abs(al.value - lin.alpha[t]) > 1e-6 * lin.alpha[t]):
            return False
    return True


class _TPInteractionLinear(torch.autograd.Function):
    """``lin(tp_interaction(x, sh, w))``: the forward runs tp_fwd and the linear as two kernels;
    the backward runs the linear's weight / bias gradients (side stream) and ONE fused kernel
    for the TP's grad-x / grad-w from the linear's output gradient (``eelg_tp_bwd_fused``)."""

    @staticmethod
    def forward(ctx, x, sh, w, lw, lb, csr: EdgeCSR, cfg: int, info: Dict[str, int],
                inv_norm: float, lin, side, chunks: int = 0):
        agg, x, sh, w = _tp_fwd(x, sh, w, csr, cfg, info, inv_norm)
        y = lin._fwd(agg, lw, lb)
        ctx.save_for_backward(x, sh, w, agg, lw)
        ctx.csr, ctx.cfg, ctx.info, ctx.inv_norm, ctx.lin, ctx.side = csr, cfg, info, inv_norm, lin, side
        ctx.chunks = chunks
        return y

    @staticmethod
    def backward(ctx, gy):
        x, sh, w, agg, lw = ctx.saved_tensors
        csr, info, lin, side = ctx.csr, ctx.info, ctx.lin, ctx.side
        gy = _a16(gy)
        want_w, want_b = ctx.needs_input_grad[3], ctx.needs_input_grad[4]
        gW = gb = None
        if want_w or want_b:
            if side is None:
                gW = lin._bwd_w(agg, gy) if want_w else None
                gb = lin._bwd_bias(gy) if want_b else None
            else:
                side.wait_stream(torch.cuda.current_stream(gy.device))
                agg.record_stream(side)
                gy.record_stream(side)
                with torch.cuda.stream(side):
                    gW = lin._bwd_w(agg, gy) if want_w else None
                    gb = lin._bwd_bias(gy) if want_b else None
        gw = torch.empty_like(w)
        if ctx.chunks > 1:
            return _tp_linear_bwd_chunked(ctx, x, sh, w, lw, gy, gw) + (gW, gb) + (None,) * 7
        lwc = lw.detach().contiguous()
        if lwc.data_ptr() % 16:
            lwc = lwc.clone()
        gxe = torch.empty(csr.num_edges, info["din"], device=x.device, dtype=w.dtype)
        lib = _lib.load()
        bwf = lib.eelg_tp_bwd_fused_bf16 if w.dtype == torch.bfloat16 else lib.eelg_tp_bwd_fused
        _launch("tp_bwd_fused", bwf, ctx.cfg, x, sh, w, csr.sender, csr.receiver, csr.rowptr,
                csr.num_nodes, gy, lwc, float(ctx.inv_norm), gw, gxe, on=gxe,
                timed=f"tp_bwf[din={info['din']}]")
        return _tp_sender_sum(gxe, csr), None, gw, gW, gb, None, None, None, None, None, None, None


def _chunk_bounds(csr: EdgeCSR, chunks: int):
    """[(n0, n1, e0, e1)]: ``chunks`` receiver ranges of about equal edge counts (one host read
    of rowptr, cached on the CSR)"""
    key = ("_chunks", chunks)
    hit = getattr(csr, "_chunk_cache", None)
    if hit is not None and hit[0] == key:
        return hit[1]
    rp = csr.rowptr.cpu()
    n, e = csr.num_nodes, csr.num_edges
    bounds, n0 = [], 0
    for c in range(1, chunks + 1):
        n1 = n if c == chunks else int(torch.searchsorted(rp, torch.tensor(e * c // chunks, dtype=rp.dtype)))
        n1 = max(n0, min(n, n1))
        if n1 > n0:
            bounds.append((n0, n1, int(rp[n0]), int(rp[n1])))
        n0 = n1
    csr._chunk_cache = (key, bounds)
    return bounds


def _tp_linear_bwd_chunked(ctx, x, sh, w, lw, gy, gw):
    """the unfused kernels (linear grad-x, tp_bwd) per receiver chunk: grad_agg of a chunk is
    consumed while it is still in the MALL; tp_bwd's receiver indices are global, so its grad_agg
    pointer is offset back by the chunk's first row"""
    csr, info, lin = ctx.csr, ctx.info, ctx.lin
    gxe = torch.empty(csr.num_edges, info["din"], device=x.device, dtype=w.dtype)
    for n0, n1, e0, e1 in _chunk_bounds(csr, ctx.chunks):
        gagg = lin._bwd_x(gy[n0:n1], lw)
        if e1 > e0:
            _tp_bwd_launch(x, sh, w, csr, ctx.cfg, info, ctx.inv_norm, gagg, gw, gxe, chunk=(n0, e0, e1))
    return _tp_sender_sum(gxe, csr), None, gw


def tp_interaction_linear(x, sh, w, csr: EdgeCSR, cfg: int, info: Dict[str, int],
                          inv_norm: float, lin, chunks: int = 0):
    """``lin(tp_interaction(x, sh, w, csr, cfg, info, inv_norm))`` with the fused backward;
    the caller checks ``tp_linear_fusable`` first.  ``lin``'s weight / bias gradients run on
    its side stream as ``o3.Linear.forward`` arranges them."""
    _require_device(x, sh, w)
    from .o3 import _OnStream
    lw, lb = lin.weight, lin.bias
    side = None
    if OVERLAP and x.is_cuda and torch.is_grad_enabled() and lw.requires_grad:
        side = side_stream(x.device, 2)
        with torch.cuda.stream(side):
            lw = _OnStream.apply(lw, side)
            if lb is not None:
                lb = _OnStream.apply(lb, side)
    return _TPInteractionLinear.apply(x, sh, w, lw, lb, csr, cfg, info, inv_norm, lin, side, chunks)


def per_edge_csr(csr: EdgeCSR) -> EdgeCSR:
    """The same edges with every edge its own receiver segment (``rowptr = 0..E``,
    ``receiver = e``): ``tp_interaction`` over it returns the per-edge messages
    ``conv_tp(x[sender], sh, w) * inv_norm`` as ``[E, dmid]`` rows in receiver-sorted order, and
    its backward reads one grad row per edge.  The sender CSR (grad-x) is the base graph's.
    Cached on ``csr``."""
    pe = getattr(csr, "_per_edge", None)
    if pe is None:
        e = csr.num_edges
        ar = torch.arange(e + 1, device=csr.rowptr.device, dtype=torch.int32)
        pe = EdgeCSR(csr.perm, csr.sender, ar[:e], ar, csr.sperm, csr.srowptr, csr.num_nodes)
        csr._per_edge = pe
    return pe


def in_degree_scale(csr: EdgeCSR) -> torch.Tensor:
    """[N] fp32 ``1 / max(in-degree, 1)`` (torch_scatter 'mean' divides by the clamped count);
    cached on ``csr``."""
    s = getattr(csr, "_inv_deg", None)
    if s is None:
        deg = (csr.rowptr[1:] - csr.rowptr[:-1]).to(torch.float32)
        s = 1.0 / deg.clamp_min(1.0)
        csr._inv_deg = s
    return s


# ---------------------------------------------------------------------------
# symmetric contraction
# ---------------------------------------------------------------------------
class _SymCon(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, coef, cfg: int, info: Dict[str, int], mul: int, side=None):
        x, coef = _a16(x), _a16(coef)
        n = x.shape[0]
        # rows of mul channels x D (Dout) components; info's x_row / out_row are those of mul 32
        if x.shape[1] != mul * info["D"] or coef.shape != (mul, info["coef_ld"]):
            raise ValueError(f"shape mismatch: x {tuple(x.shape)} coef {tuple(coef.shape)} vs mul {mul}, {info}")
        out = torch.empty(n, mul * info["Dout"], device=x.device, dtype=torch.float32)
        _launch("sc_fwd", _lib.load().eelg_sc_fwd_rows, cfg, x, x.shape[1], coef, n, mul, out,
                out.shape[1], on=out, timed="sc_fwd")
        ctx.save_for_backward(x, coef)
        ctx.cfg, ctx.info, ctx.mul, ctx.side = cfg, info, mul, side
        return out

    @staticmethod
    def backward(ctx, g):
        x, coef = ctx.saved_tensors
        g = _a16(g)
        n = x.shape[0]
        if g.shape[1] != ctx.mul * ctx.info["Dout"]:
            raise ValueError(f"grad_out {tuple(g.shape)} vs mul {ctx.mul}, {ctx.info}")
        lib = _lib.load()
        gx = gcoef = None
        want_x, want_c = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        # the coefficient gradient reads channel-major copies of x / grad_out, which grad-x
        # writes from the tiles it stages anyway
        if want_c:
            xt = torch.empty(ctx.mul * ctx.info["D"], n, device=x.device, dtype=torch.float32)
            gt = torch.empty(ctx.mul * ctx.info["Dout"], n, device=x.device, dtype=torch.float32)
        # with a side stream, the channel-major transposes move there with the coef-grad
        # (off the main chain); in line, grad-x writes them from the tiles it stages anyway
        cm_side = want_c and ctx.side is not None and SC_CMAJOR_ON_SIDE
        if cm_side:
            # launched before grad-x: the transposes need only x and grad_out, and run beside it
            side = ctx.side
            side.wait_stream(torch.cuda.current_stream(x.device))
            for t in (x, g, xt, gt):
                t.record_stream(side)
            with torch.cuda.stream(side):
                _sc_cmajor_pair(ctx.cfg, x, g, n, ctx.mul, xt, gt)
        if want_x:
            gx = torch.empty_like(x)
            fuse = want_c and not cm_side
            _launch("sc_bwd_x", lib.eelg_sc_bwd_x_rows, ctx.cfg, x, x.shape[1], coef, g, g.shape[1],
                    n, ctx.mul, gx, xt if fuse else None, gt if fuse else None, on=gx,
                    timed="sc_bwd_x")
        if want_c:
            if not (want_x or cm_side):
                _sc_cmajor_pair(ctx.cfg, x, g, n, ctx.mul, xt, gt, timed="sc_cmajor")
            chunk = ctx.info["coef_chunk"]          # nodes per streamed (LDS-staged) chunk
            nch = int(lib.eelg_sc_bwd_coef_parts(ctx.cfg, n, ctx.mul))   # partial rows (node ranges)
            part = torch.empty(nch, ctx.mul, ctx.info["coef_ld"], device=x.device, dtype=torch.float32)
            if ctx.info["coef_ld"] != ctx.info["nterms"]:
                part[:, :, ctx.info["nterms"]:].zero_()   # the kernel writes terms < nterms
            side = ctx.side if (SC_COEF_ON_SIDE or cm_side) else None
            if side is not None:
                # the coefficient gradient runs on the side stream, where its consumer (the
                # coefficient chain's backward) runs too; the main stream goes on meanwhile
                if not cm_side:
                    side.wait_stream(torch.cuda.current_stream(x.device))
                for t in (xt, gt, part):
                    t.record_stream(side)
            with torch.cuda.stream(side) if side is not None else contextlib.nullcontext():
                _launch("sc_bwd_coef", lib.eelg_sc_bwd_coef, ctx.cfg, xt, gt, n, ctx.mul, chunk, part,
                        on=part, timed="sc_bwd_coef")
                gcoef = sum_rows(part)
        return gx, gcoef, None, None, None, None


def _sc_cmajor_pair(cfg: int, x, g, n: int, mul: int, xt, gt, timed: Optional[str] = None) -> None:
    """the channel-major copies ``xt`` of ``x`` and ``gt`` of ``g`` (``eelg_sc_cmajor``, two
    launches on the current stream under one timer)"""
    fn = _lib.load().eelg_sc_cmajor
    tok = TIMER.start(timed) if timed is not None else None
    for which, src, dst in ((0, x, xt), (1, g, gt)):
        _launch("sc_cmajor", fn, cfg, which, src, n, mul, dst, on=dst)
    TIMER.stop(tok)


def symmetric_contraction(x, coef, cfg: int, info: Dict[str, int], mul: int, side=None):
    """``side``: the stream ``coef`` was produced on (its backward's stream); the
    coefficient gradient is then computed there."""
    _require_device(x, coef)
    return _SymCon.apply(x, coef, cfg, info, mul, side)


class ScgTable:
    """Term table of a symmetric contraction for the table-driven kernels (``eelg_scg_*``,
    correlation 4): ``plan`` = ``cg.symcon_plan`` (terms sorted by output component), ``ls_in``
    / ``ls_out`` the coupling / output l's (one block of ``mul`` channels each, mul-major)."""

    def __init__(self, plan, ls_in, ls_out, mul: int):
        d = _lib.ScgDesc()
        D = sum(2 * l + 1 for l in ls_in)
        Dout = sum(2 * l + 1 for l in ls_out)
        if D > _lib.SCG_MAXD or Dout > _lib.SCG_MAXD:
            raise NotImplementedError(f"table-driven contraction: {D} / {Dout} components per channel "
                                      f"(at most {_lib.SCG_MAXD})")
        d.D, d.Dout, d.mul, d.nterms = D, Dout, mul, len(plan.terms)

        def layout(ls, base, stride):
            a, off = 0, 0
            for l in ls:
                for m in range(2 * l + 1):
                    base[a], stride[a] = mul * off + m, 2 * l + 1
                    a += 1
                off += 2 * l + 1
        layout(ls_in, d.xb, d.xs)
        layout(ls_out, d.ob, d.os)
        self.ldc = max(64, -(-len(plan.terms) // 64) * 64)
        packed, outs = [], []
        for q, (nu, cls, o) in enumerate(plan.terms):
            idx = [i if i >= 0 else D for i in cls] + [D] * (4 - len(cls))
            if len(idx) != 4:
                raise ValueError(f"term {cls}: more than four factors")
            packed.append(idx[0] | idx[1] << 8 | idx[2] << 16 | idx[3] << 24)
            outs.append(o)
        if outs != sorted(outs):
            raise ValueError("table-driven contraction: terms must be sorted by output component")
        for q in range(Dout + 1):
            d.orow[q] = sum(1 for o in outs if o < q)
        pad = self.ldc - len(packed)
        packed += [D | D << 8 | D << 16 | D << 24] * pad
        outs += [Dout] * pad
        self.desc, self.D, self.Dout, self.mul = d, D, Dout, mul
        self._terms = torch.tensor(packed, dtype=torch.int64).to(torch.int32)
        self._outs = torch.tensor(outs, dtype=torch.int32)
        self._dev = {}

    def on(self, device):
        key = str(device)
        if key not in self._dev:
            self._dev[key] = (self._terms.to(device), self._outs.to(device))
        return self._dev[key]


class _SymConTable(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, coef, tab: ScgTable):
        x, coef = _f32(x), _f32(coef)
        n = x.shape[0]
        if x.shape[1] != tab.mul * tab.D or coef.shape != (tab.mul, tab.ldc):
            raise ValueError(f"shape mismatch: x {tuple(x.shape)} coef {tuple(coef.shape)} vs mul "
                             f"{tab.mul}, D {tab.D}, ldc {tab.ldc}")
        terms, _ = tab.on(x.device)
        out = torch.empty(n, tab.mul * tab.Dout, device=x.device, dtype=torch.float32)
        _launch("scg_fwd", _lib.load().eelg_scg_fwd, tab.desc, terms, x, x.shape[1], coef, tab.ldc, n,
                out, out.shape[1], on=out)
        ctx.save_for_backward(x, coef)
        ctx.tab = tab
        return out

    @staticmethod
    def backward(ctx, g):
        x, coef = ctx.saved_tensors
        tab = ctx.tab
        g = _f32(g)
        n = x.shape[0]
        lib = _lib.load()
        terms, outs = tab.on(x.device)
        gx = gcoef = None
        if ctx.needs_input_grad[0]:
            gx = torch.empty_like(x)
            _launch("scg_bwd_x", lib.eelg_scg_bwd_x, tab.desc, terms, x, x.shape[1], coef, tab.ldc, g,
                    g.shape[1], n, gx, on=gx)
        if ctx.needs_input_grad[1]:
            nch = max(1, -(-n // _lib.SCG_CHUNK))
            part = torch.zeros(nch, tab.mul, tab.ldc, device=x.device, dtype=torch.float32)
            _launch("scg_bwd_coef", lib.eelg_scg_bwd_coef, tab.desc, terms, outs, tab.ldc, x,
                    x.shape[1], g, g.shape[1], n, part, on=part)
            gcoef = sum_rows(part)
        return gx, gcoef, None


def symmetric_contraction_table(x, coef, tab: ScgTable):
    """The table-driven contraction (correlation 4): ``x`` [N, mul*D] rows, ``coef`` [mul, tab.ldc]."""
    _require_device(x, coef)
    return _SymConTable.apply(x, coef, tab)


# ---------------------------------------------------------------------------
# radial MLP (conv_tp_weights, gnn/blocks.py:537-549)
# ---------------------------------------------------------------------------
def _wgrad(g: torch.Tensor, x: torch.Tensor, chunk: int = 512) -> torch.Tensor:
    """g^T @ x over a long row dimension as a split-K batched GEMM + fixed-order sum (the CGC
    models' weight gradients, gnn/cgc.py; library GEMMs pick no split-K for
    [64 x 131072] @ [131072 x 64] and run on a few CUs)."""
    e = g.shape[0]
    c = e // chunk
    acc = torch.promote_types(g.dtype, torch.float32)     # bf16 operands: fp32 sums
    out = None
    if c > 1:
        m = c * chunk
        prod = torch.bmm(g[:m].view(c, chunk, -1).transpose(1, 2), x[:m].view(c, chunk, -1))
        out = sum_rows(prod) if prod.dtype == torch.float32 else prod.sum(0, dtype=acc)
        g, x = g[m:], x[m:]
    if g.shape[0]:
        rest = (g.t() @ x).to(acc)
        out = rest if out is None else out + rest
    return out if out is not None else torch.zeros(g.shape[1], x.shape[1], device=g.device,
                                                   dtype=acc)


def split_bf16x3(t: torch.Tensor) -> torch.Tensor:
    """[3, *t.shape] bf16 parts of an fp32 tensor with t == parts.sum(0) exactly
    (``eelg_split_bf16x3``): the operand form of the fp32-accurate bf16 MFMA GEMMs."""
    _require_device(t)
    t = _f32(t)
    parts = torch.empty((3,) + tuple(t.shape), device=t.device, dtype=torch.bfloat16)
    _launch("split_bf16x3", _lib.load().eelg_split_bf16x3, t, t.numel(), parts, on=parts)
    return parts


def sum_rows(part: torch.Tensor, out: torch.Tensor = None, scale: float = 1.0) -> torch.Tensor:
    """``scale * part.sum(0)`` on the device in a fixed order (``eelg_sum_rows``): ``part`` is
    [rows, ...] with contiguous trailing dims, or a 2-D view whose rows are strided (a column
    block of a wider tensor: the bias gradient of one output slot).  ``out`` (contiguous,
    ``part.shape[1:]``) receives the sum when given."""
    _require_device(part)
    if part.dtype != torch.float32:
        raise TypeError(f"sum_rows: float32 expected, got {part.dtype}")
    rows = part.shape[0]
    if part.dim() == 2 and part.stride(1) == 1:
        ld, cols = part.stride(0), part.shape[1]
    else:
        part = part.contiguous()
        cols = math.prod(part.shape[1:])
        ld = cols
    if out is None:
        out = torch.empty(part.shape[1:], device=part.device, dtype=torch.float32)
    lib = _lib.load()
    nw = lib.eelg_sum_rows_work(rows, cols)
    work = torch.empty(nw, device=part.device, dtype=torch.float32) if nw else None
    _launch("sum_rows", lib.eelg_sum_rows, part, max(ld, cols), rows, cols, float(scale), out, work, nw,
            on=out)
    return out


def _radial_desc(params, n_feat: int):
    n_hidden = (len(params) - 1) // 2
    hidden = params[0].shape[0]
    n_out = params[-1].shape[0]
    d = _lib.RadialDesc()
    d.n_feat, d.hidden, d.n_hidden, d.n_out = n_feat, hidden, n_hidden, n_out
    for i in range(n_hidden):
        d.w[i] = params[2 * i].data_ptr()
        d.b[i] = params[2 * i + 1].data_ptr()
    return d


def _radial_padded(params, n_feat: int, g=None):
    """(desc, W_o, g, n_out) as the kernels take them: they read the output width in whole 16-B
    pieces of bf16 (a multiple of 8, as every generated TP weight count is), so another width
    ``n_out`` runs on zero-padded W_o rows, zero-padded columns of the output gradient ``g`` and
    ``desc.n_out`` = the padded width"""
    d = _radial_desc(params, n_feat)
    wo, n_out = params[-1], d.n_out
    pad = -n_out % 8
    if pad:
        wo = torch.cat([wo, wo.new_zeros(pad, wo.shape[1])])
        if g is not None:
            g = torch.cat([g, g.new_zeros(g.shape[0], pad)], 1)
        d.n_out = n_out + pad
    return d, wo, g, n_out


def _radial_plan(ec: int, n_out: int):
    """(partial rows of the small-layer gradients, of the W_o gradient) the backward kernels
    write for ``ec`` edges (``eelg_radial_plan``)"""
    npart, ns = ctypes.c_int(), ctypes.c_int()
    _lib.check(_lib.load().eelg_radial_plan(ec, n_out, ctypes.byref(npart), ctypes.byref(ns)),
               "radial_plan")
    return npart.value, ns.value


def _radial_chunks(e: int, n_out: int, out_es: int, hidden: int, n_hidden: int):
    """Edge ranges under the radial kernels' 2 GiB per-stream limit (their buffer descriptors
    use 32-bit byte offsets): ``E * n_out * out_es`` for the [E, W] output / its gradient and
    ``E * hidden * n_hidden * 4`` for the saved pre-activations.  One range below the limit."""
    per_edge = max(n_out * out_es, hidden * n_hidden * 4, 1)
    cap = ((1 << 31) - 1) // per_edge // 128 * 128
    if cap <= 0:
        raise ValueError(f"radial MLP: one edge row ({per_edge} B) exceeds the 2 GiB stream limit")
    return [(a, min(a + cap, e)) for a in range(0, e, cap)] or [(0, 0)]


class _RadialMLP(torch.autograd.Function):
    """Linear(+bias)-SiLU-...-Linear(no bias) on edge features as one fused HIP kernel
    (``eelg_radial_fwd``: hidden layers on fp32 MFMA, the output layer fp32-accurate on bf16
    MFMA with split operands, hidden activations in LDS, only the pre-activations and the
    [E, W] output reach HBM), backward as three (``eelg_radial_bwd``).  The features carry no
    grad in training (they come from eelg_edge_embed); when they do (geometry
    gradients) one more launch, ``eelg_radial_bwd_x``, walks the hidden layers back from the
    grad_h the backward leaves, and with every weight frozen the weight-gradient launches are
    skipped (``eelg_radial_bwd_gh`` alone).  Edge sets past the kernels' 2 GiB per-stream limit
    run as several launches (``_radial_chunks``)."""

    @staticmethod
    def forward(ctx, feats, out_dtype, *params):
        _require_device(feats)
        feats = _f32(feats)
        params = tuple(_f32(p) for p in params)
        e, nf = feats.shape
        d, wo, _, n_out = _radial_padded(params, nf)
        if wo.shape[1] != d.hidden or any(p.shape[0] != d.hidden for p in params[:-1]):
            raise ValueError("radial MLP: hidden widths differ between layers")
        wp = d.n_out
        out = torch.empty(e, wp, device=feats.device, dtype=out_dtype)
        wo_parts = split_bf16x3(wo)                  # [3, n_out, hidden]: the output layer's B operand
        lib = _lib.load()
        chunks = _radial_chunks(e, d.n_out, out.element_size(), d.hidden, d.n_hidden)
        zs = []
        for a, b in chunks:
            z = torch.empty(d.n_hidden, b - a, d.hidden, device=feats.device, dtype=torch.float32)
            _launch("radial_fwd", lib.eelg_radial_fwd, feats[a:b], b - a, d, wo_parts,
                    int(out_dtype == torch.bfloat16), z, out[a:b], on=feats)
            zs.append(z)
        ctx.chunks = chunks
        ctx.save_for_backward(feats, *params, *zs)
        ctx.n_params = len(params)
        return out if wp == n_out else out[:, :n_out]

    @staticmethod
    def backward(ctx, g):
        feats, *rest = ctx.saved_tensors
        params, zs = rest[:ctx.n_params], rest[ctx.n_params:]
        e, nf = feats.shape
        d, wo, g, n_out = _radial_padded(params, nf, g)
        g = g.contiguous()
        if g.data_ptr() % 16:
            g = g.clone()
        lib = _lib.load()
        wot_parts = split_bf16x3(wo.t().contiguous())             # [3, hidden, n_out]
        h = d.hidden
        # grad of the features (geometry gradients only), filled per chunk from its grad_h
        gfe = torch.empty_like(feats) if ctx.needs_input_grad[0] else None
        if not any(ctx.needs_input_grad[2:]):
            # every weight frozen: grad_h = grad_w W_o alone, then the chain down to the features
            for (a, b), z in zip(ctx.chunks, zs):
                if gfe is None or b == a:
                    continue
                grad_h = torch.empty(b - a, h, device=g.device, dtype=torch.float32)
                _launch("radial_bwd_gh", lib.eelg_radial_bwd_gh, g[a:b], int(g.dtype == torch.bfloat16),
                        b - a, d, wot_parts, grad_h, on=g)
                _radial_bwd_x(grad_h, d, z, gfe[a:b])
            return (gfe, None) + (None,) * len(params)
        if RADIAL_CHAIN and h == 64:
            return _RadialMLP._backward_chain(ctx, g, feats, params, zs, d, wot_parts, n_out, gfe)
        n_small = h * nf + h + (d.n_hidden - 1) * (h * h + h)
        small, gwo = None, None
        for (a, b), z in zip(ctx.chunks, zs):
            ec = b - a
            npart, ns = _radial_plan(ec, d.n_out)
            part_h = torch.empty(npart, n_small, device=g.device, dtype=torch.float32)
            part_wo = torch.empty(ns, d.n_out, h, device=g.device, dtype=torch.float32)
            grad_h = torch.empty(ec, h, device=g.device, dtype=torch.float32)
            if ec == 0:
                part_h.zero_()
                part_wo.zero_()
            _launch("radial_bwd", lib.eelg_radial_bwd, g[a:b], int(g.dtype == torch.bfloat16), ec, d,
                    wot_parts, z, feats[a:b], grad_h, part_h, part_wo, on=g)
            if gfe is not None and ec:
                _radial_bwd_x(grad_h, d, z, gfe[a:b])
            sm, wo = sum_rows(part_h), sum_rows(part_wo)
            small = sm if small is None else small + sm
            gwo = wo if gwo is None else gwo + wo
        grads, off = [], 0
        for p in params[:-1]:
            grads.append(small[off: off + p.numel()].view_as(p))
            off += p.numel()
        return (gfe, None, *grads, _trim_rows(gwo, n_out))

    @staticmethod
    def _backward_chain(ctx, g, feats, params, zs, d, wot_parts, n_out, gfe=None):
        """``_radial_bwd_chain`` per edge range, the ranges' gradients added in range order"""
        acc = gwo = None
        for (a, b), z in zip(ctx.chunks, zs):
            grads, wo = _radial_bwd_chain(g[a:b], feats[a:b], params, z, d, wot_parts,
                                          None if gfe is None else gfe[a:b])
            acc = grads if acc is None else [s + t for s, t in zip(acc, grads)]
            gwo = wo if gwo is None else gwo + wo
        return (gfe, None, *acc, _trim_rows(gwo, n_out))


def _trim_rows(gwo, n_out: int):
    """grad W_o without the rows of a zero-padded width"""
    return gwo if gwo.shape[0] == n_out else gwo[:n_out].contiguous()


def _radial_bwd_chain(g, feats, params, z, d, wot_parts, gfe=None, smap: Optional[StrutMap] = None):
    """The chain backward of one edge range (hidden 64): ``eelg_radial_bwd_chain`` leaves gz_n and
    the hidden-layer inputs; the weight gradients gz_n^T h_n are long-K reductions on the linear
    weight-gradient kernel and the bias gradients column sums (``eelg_sum_rows``), all in a fixed
    order.  ``g`` [E_c, d.n_out], ``feats`` [E_c, n_feat], ``z`` the saved pre-activations of the
    range, or with ``smap`` of its shared rows, edge e's at row ``smap.row[e]``
    (``eelg_radial_bwd_chain_rows``).  ``gfe``: receives the feature gradient.  Returns
    ([grad w_0, grad b_0, ...], grad W_o of the padded width); zeros for an empty range."""
    from . import dense
    lib = _lib.load()
    ec, h, nh, dev = g.shape[0], d.hidden, d.n_hidden, g.device
    bf = int(g.dtype == torch.bfloat16)
    part_wo = torch.empty(_radial_plan(ec, d.n_out)[1], d.n_out, h, device=dev, dtype=torch.float32)
    grad_h = torch.empty(ec, h, device=dev, dtype=torch.float32)
    gz = torch.empty(nh, ec, h, device=dev, dtype=torch.float32)
    hin = torch.empty(max(nh - 1, 1), ec, h, device=dev, dtype=torch.float32)
    if ec == 0:
        part_wo.zero_()
    if smap is None:
        _launch("radial_bwd_chain", lib.eelg_radial_bwd_chain, g, bf, ec, d, wot_parts, z, grad_h,
                gz, hin, part_wo, on=g)
    else:
        zlast = torch.empty(ec, h, device=dev, dtype=torch.float32)
        _launch("radial_bwd_chain_rows", lib.eelg_radial_bwd_chain_rows, g, bf, ec, smap.row,
                smap.n_rows, d, wot_parts, z, grad_h, gz, hin, zlast, part_wo, on=g)
    if gfe is not None and ec:
        _radial_bwd_x(grad_h, d, z, gfe)
    grads = []
    for n in range(nh):
        x_n = feats if n == 0 else hin[n - 1]
        w_n, b_n = params[2 * n], params[2 * n + 1]
        grads.append(dense.linear_bwd_w(x_n, gz[n]).view_as(w_n) if ec else torch.zeros_like(w_n))
        grads.append(sum_rows(gz[n]).view_as(b_n) if ec else torch.zeros_like(b_n))
    return grads, sum_rows(part_wo)


def _radial_bwd_x(grad_h, d, z, out) -> None:
    """``eelg_radial_bwd_x`` of one edge chunk: ``out`` [E_c, n_feat] rows of the feature gradient"""
    _launch("radial_bwd_x", _lib.load().eelg_radial_bwd_x, grad_h, grad_h.shape[0], d, z, out,
            on=out, timed="radial_bwd_x")


class _RadialMLPShared(torch.autograd.Function):
    """``_RadialMLP`` on the ``S`` representative feature rows of a ``StrutMap`` (hidden 64, the
    chain backward, one launch range: ``strut_rows``).  Outputs the ``StrutWeights``' ``w`` [S, W]
    (non-differentiable) and its token; the backward takes the per-edge ``grad_w`` [E, W] from
    the ``StrutWeights`` and runs ``_RadialMLP``'s chain backward over the E edges in edge order,
    the kernels reading edge e's saved pre-activations at row ``smap.row[e]``
    (``eelg_radial_bwd_chain_rows``).  Every per-edge quantity is bitwise the per-edge MLP's and
    every sum keeps its order, so the parameter gradients are bitwise those of ``_RadialMLP``."""

    @staticmethod
    def forward(ctx, feats, out_dtype, smap: StrutMap, box: _GradBox, *params):
        _require_device(feats)
        feats = _f32(feats)
        feats_s = smap.rep_rows(feats)               # [S, n_feat]: the only new pass
        params = tuple(_f32(p) for p in params)
        s_rows, nf = feats_s.shape
        d, wo, _, n_out = _radial_padded(params, nf)
        wp = d.n_out
        if d.hidden != 64 or any(p.shape[0] != 64 for p in params[:-1]) or wo.shape[1] != 64:
            raise ValueError("radial MLP on shared rows: hidden width 64 only")
        out = torch.empty(s_rows, wp, device=feats.device, dtype=out_dtype)
        z = torch.empty(d.n_hidden, s_rows, d.hidden, device=feats.device, dtype=torch.float32)
        _launch("radial_fwd", _lib.load().eelg_radial_fwd, feats_s, s_rows, d, split_bf16x3(wo),
                int(out_dtype == torch.bfloat16), z, out, on=feats)
        token = torch.empty(1, device=feats.device, dtype=torch.float32)
        w = out if wp == n_out else out[:, :n_out].contiguous()
        ctx.box, ctx.smap = box, smap
        ctx.save_for_backward(feats, z, *params)
        ctx.mark_non_differentiable(w)
        ctx.set_materialize_grads(False)             # no [S, W] zeros for w's absent gradient
        return w, token

    @staticmethod
    def backward(ctx, _gw_unused, _gtoken):
        feats, z, *params = ctx.saved_tensors
        g, ctx.box.gw = ctx.box.gw, None
        if g is None:
            raise RuntimeError("radial MLP on shared rows: no weight gradient was handed over "
                               "(the interaction's backward has not run, or ran twice)")
        g.record_stream(torch.cuda.current_stream(g.device))     # made on the TP's stream
        d, wo, g, n_out = _radial_padded(params, feats.shape[1], g)
        grads, gwo = _radial_bwd_chain(g, feats, params, z, d, split_bf16x3(wo.t().contiguous()),
                                       smap=ctx.smap)
        return (None, None, None, None, *grads, _trim_rows(gwo, n_out))


def _radial_params(mlp: torch.nn.Sequential) -> list:
    """the parameters of ``mlp`` = [Linear(bias), SiLU]*k + [Linear(no bias)] in kernel order"""
    mods = list(mlp)
    params = []
    for i, mod in enumerate(mods):
        if isinstance(mod, torch.nn.Linear):
            last = i == len(mods) - 1
            if last != (mod.bias is None):
                raise ValueError("radial MLP: expected biases on hidden layers only")
            params.append(mod.weight)
            if not last:
                params.append(mod.bias)
        elif not isinstance(mod, torch.nn.SiLU):
            raise ValueError(f"radial MLP: unsupported module {type(mod).__name__}")
    return params


def radial_mlp_shared(feats: torch.Tensor, mlp: torch.nn.Sequential, smap: StrutMap,
                      out_dtype: torch.dtype = torch.float32) -> StrutWeights:
    """``radial_mlp`` computed once per row of ``smap`` (``strut_rows`` decides where this
    applies): the ``StrutWeights`` that ``tp_interaction`` takes in place of [E, W] weights."""
    if smap.n_rows == 0:
        raise ValueError("radial MLP on shared rows: the map has no rows")
    box = _GradBox()
    tok = TIMER.start("radial_mlp_fwd")
    w, token = _RadialMLPShared.apply(_f32(feats), out_dtype, smap, box, *_radial_params(mlp))
    TIMER.stop(tok)
    return StrutWeights(w, smap, token, box)


def radial_mlp(feats: torch.Tensor, mlp: torch.nn.Sequential,
               out_dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """Apply ``mlp`` = [Linear(bias), SiLU]*k + [Linear(no bias)] with the fused backward.
    ``out_dtype`` bf16: the [E, W] output (the TP weights) is stored in bf16."""
    params = _radial_params(mlp)
    tok = TIMER.start("radial_mlp_fwd")
    out = _RadialMLP.apply(_f32(feats), out_dtype, *params)
    TIMER.stop(tok)
    return out


# ---------------------------------------------------------------------------
# symmetric-contraction coefficients coef = (U_sym @ W)^T with a sparse U_sym
# ---------------------------------------------------------------------------
class SparseRows:
    """CSR of a fixed matrix and of its transpose (device int32 / fp32)."""

    def __init__(self, dense: torch.Tensor):
        d = dense.detach().to(torch.float64).cpu()
        self.shape = tuple(d.shape)
        for name, m in (("a", d), ("t", d.t())):
            nz = m != 0
            rowptr = torch.zeros(m.shape[0] + 1, dtype=torch.int32)
            rowptr[1:] = torch.cumsum(nz.sum(1), 0).to(torch.int32)
            r, c = torch.nonzero(nz, as_tuple=True)
            setattr(self, name, (rowptr, c.to(torch.int32), m[r, c].to(torch.float32)))
        self._dev = {}

    def on(self, device):
        key = str(device)
        if key not in self._dev:
            self._dev[key] = tuple(tuple(t.to(device) for t in trip) for trip in (self.a, self.t))
        return self._dev[key]


def _spmm(trip, n_rows, B, ldb_r, ldb_c, n_cols, out, ldo_r, ldo_c):
    rp, col, val = trip
    _launch("csr_spmm", _lib.load().eelg_csr_spmm, rp, col, val, n_rows, B, ldb_r, ldb_c, n_cols, out,
            ldo_r, ldo_c, on=out)


class _SymConCoef(torch.autograd.Function):
    """coef[c, t] = sum_k U[t, k] W[k, c]  ([mul, ld], the layout the sc kernels read: rows
    padded to ``ld`` >= nterms, the padding zero)."""

    @staticmethod
    def forward(ctx, w, sp: SparseRows, ld: int):
        _require_device(w)
        w = _f32(w)
        nt, nk = sp.shape
        mul = w.shape[1]
        a, t = sp.on(w.device)
        coef = torch.empty(mul, ld, device=w.device, dtype=torch.float32)
        if ld != nt:
            coef[:, nt:].zero_()
        _spmm(a, nt, w, mul, 1, mul, coef, 1, ld)                 # out[t, c] at c*ld + t
        ctx.sp, ctx.mul = sp, mul
        return coef

    @staticmethod
    def backward(ctx, g):
        g = _f32(g)
        sp, mul = ctx.sp, ctx.mul
        nt, nk = sp.shape
        a, t = sp.on(g.device)
        gt = g.t().contiguous()                                   # [ld, mul]: coalesced over c
        gw = torch.empty(nk, mul, device=g.device, dtype=torch.float32)
        _spmm(t, nk, gt, mul, 1, mul, gw, mul, 1)                 # reads rows t < nterms only
        return gw, None, None


def symcon_coefficients(w: torch.Tensor, sp: SparseRows, ld: Optional[int] = None) -> torch.Tensor:
    """[mul, ld] coefficients (``ld``: the contraction config's ``coef_ld``; default nterms)."""
    return _SymConCoef.apply(w, sp, sp.shape[0] if ld is None else ld)


# ---------------------------------------------------------------------------------------------
# the training loss and its gradient in one launch (csrc/eelg_optim.hip)
LOSS_FUSED = os.environ.get("EELG_LOSS_FUSED", "1") != "0"


class _StiffnessLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target, grad_scale: float):
        _require_device(pred, target)
        nb = int(target.shape[0])
        p2 = _f32(pred).reshape(nb, -1)
        t2 = _f32(target).reshape(nb, -1)
        n = int(t2.shape[1])
        out = torch.empty(2, device=pred.device, dtype=torch.float32)
        grad = torch.empty_like(p2)
        with torch.cuda.device(pred.device):
            _launch("stiffness_loss", _lib.load().eelg_stiffness_loss, p2, t2, nb, n,
                    float(grad_scale), out, grad, on=pred, timed="stiffness_loss")
        ctx.save_for_backward(grad)
        ctx.shape = pred.shape
        loss, mean = out[0], out[1]
        ctx.mark_non_differentiable(mean)
        return loss, mean

    @staticmethod
    def backward(ctx, g_loss, g_mean):
        (grad,) = ctx.saved_tensors
        return (grad * g_loss).view(ctx.shape), None, None


def stiffness_loss_fused(pred: torch.Tensor, target: torch.Tensor, grad_scale: float = 1.0):
    """``(loss, stiffness_loss_mean)`` of ``LightningWrappedModel.training_step``
    (``scripts/train_utils.py:52-60``) as 0-dim device tensors: ``loss = 100 * mean_b(mean_ij
    (C - C^)^2 / mean_ij C^2)``, ``stiffness_loss_mean = mean_b mean_ij (C - C^)^2`` (logged only,
    no gradient).  ``pred`` / ``target``: ``[B, 6, 6]`` or ``[B, 21]``.

    ``loss`` carries its unscaled value; its BACKWARD gives ``grad_scale`` times the gradient
    (``grad_scale = 1 / accumulate_grad_batches``: the division Lightning applies between
    ``training_step`` and ``backward`` is folded into the launch, and the backward is one
    elementwise multiply by the incoming scalar).  On CPU tensors, or with ``EELG_LOSS_FUSED=0``,
    the composed torch form with the same contract."""
    if tuple(pred.shape) != tuple(target.shape) or pred.dim() < 2:
        raise ValueError(f"stiffness_loss_fused: pred {tuple(pred.shape)}, target {tuple(target.shape)}")
    if LOSS_FUSED and pred.is_cuda:
        return _StiffnessLoss.apply(pred, target.detach(), float(grad_scale))
    dims = tuple(range(1, target.dim()))
    per_graph = torch.nn.functional.mse_loss(pred, target, reduction="none").mean(dim=dims)
    loss = 100 * (per_graph / target.pow(2).mean(dim=dims)).mean()
    if grad_scale != 1.0:     # value unscaled, gradient scaled
        loss = loss.detach() + (loss - loss.detach()) * grad_scale
    return loss, per_graph.detach().mean()
