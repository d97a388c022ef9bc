"""Device-side equivalents of the e3nn modules the hot path uses.

* ``Linear``  -- ``o3.Linear`` (path normalisation 'element', 0e biases zero-init),
  parameter ``weight`` flat in e3nn instruction order (i_in major, i_out minor),
  so ``state_dict`` keys/shapes match the reference (``gnn/blocks.py:516-521``).
  Channel mixing is a per-irrep GEMM on the mul axis.
* ``Gate``    -- ``nn.Gate`` with normalize2mom(SiLU) (``gnn/blocks.py:268-274``).
* ``TensorProduct`` -- holds the 'uvu' instruction table of ``o3.TensorProduct``
  (``gnn/blocks.py:528-535``); its arithmetic is the fused HIP interaction.
"""
from __future__ import annotations

import ctypes
import math
import os
from collections import Counter
from typing import List, Optional, Tuple

import torch

from . import _lib, cg, ops
from .irreps import Irreps

# grad-W launch shape: target workgroups and a cap on the node slices (partials)
# r04ac kbench: 1024 / 64 -> 4096 / 128 takes grad-W 7360 -> 800 from 0.324 to 0.264 ms and
# 800 -> 800 from 0.056 to 0.049 ms (a grid of about one round left the D = 9 tiles, 9x the
# bytes per node of D = 1, as the tail); the step is unchanged (these run on a side stream)
LINW_WG = int(os.environ.get("EELG_LINW_WG", "4096"))
LINW_MAX_SLICES = int(os.environ.get("EELG_LINW_MAX_SLICES", "128"))
# forward / grad-x of the eligible linears on bf16 MFMA with fp32-accurate split operands (1),
# or on the fp32 MFMA kernels (0).  Only descriptors whose every slot sums K >= LIN_X6_MINK take
# it: r04b kbench, 7360->800 fwd (K 160..320) 0.261 vs 0.290 ms fp32; K = 32 (the 800->800
# linears, every grad-x of the 7360->800) 0.056-0.391 vs 0.050-0.325 ms -- one 32-wide chunk per
# group leaves the split and LDS B-fragment reads unamortised
LIN_X6 = os.environ.get("EELG_LIN_X6", "1") != "0"
LIN_X6_MINK = int(os.environ.get("EELG_LIN_X6_MINK", "128"))
# the readout Gate as fused HIP passes (1) or torch elementwise ops (0)
GATE_FUSED = os.environ.get("EELG_GATE_FUSED", "1") != "0"


# ---------------------------------------------------------------------------
# launch helpers of the eelg_linear_* kernels, shared by this module's Linear and dense.Linear
# ---------------------------------------------------------------------------
def linw_slices(n: int, tiles: int) -> Tuple[int, int]:
    """The grad-W node slices of ``n`` rows over ``tiles`` 32x32 weight tiles: (slices, nodes per
    slice) for ~LINW_WG workgroups in total, (node slices) x (tiles); each slice leaves one
    partial weight gradient that the sum reads back."""
    slices = max(1, min((n + 31) // 32, -(-LINW_WG // tiles), LINW_MAX_SLICES))
    nps = -(-n // slices)
    return -(-n // nps), nps


def linear_bwd_w(label: str, desc, x, x_row: int, gy, gy_row: int, n: int, tiles: int, numel: int,
                 covers: bool = True) -> torch.Tensor:
    """``eelg_linear_bwd_w`` over the slices of ``linw_slices`` and the fixed-order sum of its
    partials, flat [numel].  ``covers``: the descriptor writes every entry (else they start 0)."""
    slices, nps = linw_slices(n, tiles)
    part = (torch.empty if covers else torch.zeros)(slices, numel, device=x.device, dtype=torch.float32)
    _lib.launch(label, _lib.load().eelg_linear_bwd_w, x, x_row, gy, gy_row, n, nps, part, slices,
                numel, desc, on=part)
    return ops.sum_rows(part)


def packable(desc) -> bool:
    """the descriptor qualifies for eelg_linear_fwd_pk (whole 32-wide K chunks and column
    tiles, d odd <= 9, 16-B aligned slot offsets; the row alignment is checked per call)"""
    for s in range(desc.n_slots):
        sl = desc.slot[s]
        if sl.n_src == 0 or sl.n_out % 32 or sl.y_off % 4 or sl.d not in (1, 3, 5, 7, 9):
            return False
        if sl.bias_off >= 0 and sl.d != 1:
            return False
        ks = sum(sl.src[t].k for t in range(sl.n_src))
        if ks > 320 or ks < LIN_X6_MINK:
            return False
        for t in range(sl.n_src):
            if sl.src[t].k % 32 or sl.src[t].x_off % 4:
                return False
    return True


def takes_packed(desc, switch: bool, x_row: int, out_row: int, x_at: int, out_at: int,
                 res_at: Optional[int] = None, desc_ok: Optional[bool] = None) -> bool:
    """A call runs on eelg_linear_fwd_pk: the switch is on, the descriptor is ``packable``
    (``desc_ok``: that answer where the caller keeps it), rows are whole float4, the operands at
    addresses ``x_at`` / ``out_at`` / ``res_at`` are 16-B aligned and an added operand has the
    output's own rows."""
    return bool(switch and x_row % 4 == 0 and out_row % 4 == 0 and x_at % 16 == 0 and out_at % 16 == 0
                and (res_at is None or (res_at % 16 == 0 and desc.res_row == 0))
                and (packable(desc) if desc_ok is None else desc_ok))


def pack_weights(label: str, desc, weight) -> torch.Tensor:
    """the split, alpha-scaled bf16 weights of ``desc`` in the packed kernel's layout"""
    lib = _lib.load()
    pk = torch.empty(3, int(lib.eelg_linear_pack_size(ctypes.byref(desc))), device=weight.device,
                     dtype=torch.bfloat16)
    _lib.launch(label, lib.eelg_linear_pack, weight, desc, pk, on=pk)
    return pk


def linear_apply(prefix: str, label: str, desc, switch: bool, x, x_row: int, weight, bias, res,
                 n: int, out, out_row: int, desc_ok: Optional[bool] = None, packed=None) -> None:
    """``out = x B (+ bias) (+ res)`` over ``desc``: the packed kernel where ``takes_packed``
    (labels ``prefix``_pack / ``prefix``_fwd_pk), else ``eelg_linear_fwd_res`` under ``label``.
    ``packed()`` hands over the packed weights a caller caches; None packs them on this call."""
    if takes_packed(desc, switch, x_row, out_row, x.data_ptr(), out.data_ptr(),
                    None if res is None else res.data_ptr(), desc_ok):
        pk = packed() if packed is not None else pack_weights(prefix + "_pack", desc, weight)
        _lib.launch(prefix + "_fwd_pk", _lib.load().eelg_linear_fwd_pk, x, x_row, pk, bias, res, n,
                    out, out_row, desc, on=out)
    else:
        _lib.launch(label, _lib.load().eelg_linear_fwd_res, x, x_row, weight, bias, res, n, out,
                    out_row, desc, on=out)


def _output_mask(irreps_out, covered) -> torch.Tensor:
    """e3nn 0.5 ``output_mask``: 1 on the output irreps some instruction writes, else 0."""
    if not irreps_out.dim:
        return torch.ones(0)
    return torch.cat([torch.full((mul * ir.dim,), 1.0 if o in covered else 0.0)
                      for o, (mul, ir) in enumerate(irreps_out)])


def _accept_output_mask(state_dict, key: str, irreps_out, covered, error_msgs) -> None:
    """e3nn's ``Linear`` / ``TensorProduct`` register an ``output_mask`` buffer (1 on the output
    irreps some instruction writes).  Reference checkpoints may carry it: it is derived data,
    so it is accepted and checked against this module's instructions, not stored."""
    m = state_dict.pop(key, None)
    if m is None:
        return
    want = _output_mask(irreps_out, covered)
    if tuple(m.shape) != tuple(want.shape) or not torch.equal(m.detach().cpu().float() != 0, want != 0):
        error_msgs.append(f"{key}: output mask does not match the module's instructions")


def _accept_empty(state_dict, key: str, error_msgs) -> None:
    """e3nn registers ``torch.Tensor()`` placeholders (``register_buffer('weight' | 'bias',
    torch.Tensor())``) where a module has no internal weight / bias: a ``TensorProduct`` with
    external weights, a bias-less ``Linear``, the Gate's ``ElementwiseTensorProduct``.  They
    are accepted when empty; anything else would be a weight this module does not have."""
    t = state_dict.pop(key, None)
    if t is not None and t.numel() != 0:
        error_msgs.append(f"{key}: expected e3nn's empty placeholder buffer, got shape "
                          f"{tuple(t.shape)}")


def _emit_e3nn_buffers(state_dict, prefix: str, entries) -> None:
    """``state_dict()`` carries e3nn's derived buffers (output masks, empty placeholders) under
    the reference's names, so a checkpoint of this model loads strictly into the reference."""
    for name, t in entries:
        state_dict[prefix + name] = t


class _OnStream(torch.autograd.Function):
    """Identity (a view) applied while ``stream`` is current, so that autograd runs its
    backward -- and the gradient accumulation of the parameter behind it -- on ``stream``."""

    @staticmethod
    def forward(ctx, t, stream):
        return t.view_as(t)

    @staticmethod
    def backward(ctx, g):
        return g, None


class GradMailbox:
    """Hands the layer residual's gradient from the linear that adds the residual (forward
    ``residual=h``) to the linear that reads ``h`` first (``linear_up``), whose grad-x kernel
    adds it in its epilogue: autograd would otherwise sum the two gradient contributions of
    ``h`` in a separate pass over [N, 800].  Backward order is fixed by the data flow (the
    residual's linear is downstream of ``linear_up``), so the deposit precedes the collection."""

    def __init__(self):
        self.grad = None
        # the deposited gradient's row layout: None = the residual's own rows, else the
        # (slot, first channel, channels) pieces of the depositing linear's compact output
        self.pieces = None


class _IrrepsLinearFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, lin: "Linear", side=None, residual=None, mailbox=None):
        ctx.save_for_backward(x, weight)
        ctx.lin, ctx.side, ctx.mailbox = lin, side, mailbox
        ctx.deposit = residual is not None
        return lin._fwd(x, weight, bias, residual)

    @staticmethod
    def backward(ctx, gy):
        x, weight = ctx.saved_tensors
        lin, side, mb = ctx.lin, ctx.side, ctx.mailbox
        gy = gy.contiguous()
        gres = gy if ctx.needs_input_grad[5] else None      # y = linear(x) + residual
        if gres is not None and mb is not None:
            # added by the collecting linear (compact rows: with the pieces they cover; the
            # residual's other irreps get no gradient from here, an exact zero)
            mb.grad, mb.pieces, gres = gres, (lin._out_pieces if lin._pruned else None), None
        elif gres is not None and lin._pruned:
            gres = lin._expand_out(gres)                    # autograd sums full residual rows
        extra = pieces = None
        if mb is not None and not ctx.deposit:
            extra, pieces, mb.grad, mb.pieces = mb.grad, mb.pieces, None, None
        gx = lin._bwd_x(gy, weight, extra, pieces) if ctx.needs_input_grad[0] else None
        want_w, want_b = ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        if side is None or not (want_w or want_b):
            gw = lin._bwd_w(x, gy) if want_w else None
            gb = lin._bwd_bias(gy) if want_b else None
            return gx, gw, gb, None, None, gres, None
        # weight / bias gradients on the side stream the parameters' views were made on:
        # their consumers (the views' backward, the accumulation) run there as well, and
        # the main stream carries on with grad-x
        side.wait_stream(torch.cuda.current_stream(x.device))
        x.record_stream(side)
        gy.record_stream(side)
        with torch.cuda.stream(side):
            gw = lin._bwd_w(x, gy) if want_w else None
            gb = lin._bwd_bias(gy) if want_b else None
        return gx, gw, gb, None, None, gres, None


class _LinearKernels:
    """Descriptors and launches of an ``o3.Linear`` over given pieces of its rows: the
    ``Linear`` module itself (every slot whole), and its live variant (``_LiveLinear``)."""

    def invalidate_packed(self) -> None:
        """forget the packed split weights (after a write the version counter does not see)"""
        if hasattr(self, "_pk_cache"):
            self._pk_cache.clear()

    # -- live pieces ------------------------------------------------------------
    @staticmethod
    def full_pieces(irreps):
        """the row layout as pieces (slot, first channel, channels): every slot, whole"""
        return tuple((s, 0, mul) for s, (mul, _) in enumerate(irreps))

    @staticmethod
    def _piece_offsets(irreps, pieces):
        """(offset of each piece in the compact row that holds exactly ``pieces``, row width)"""
        offs, off = [], 0
        for s, _, cnt in pieces:
            offs.append(off)
            off += cnt * irreps[s].ir.dim
        return offs, off

    def _set_pieces(self, in_pieces=None, out_pieces=None) -> None:
        """The pieces of the input / output rows this object computes: ``(slot, first channel,
        channels)`` in row order, None = every slot whole.  The input (output) rows are then
        compact: exactly the listed pieces, ``[N, sum channels * (2l+1)]``.  Only the weight
        entries joining a live input piece to a live output piece are read, and the gradient
        of every other entry of ``weight`` / ``bias`` is an exact zero; parameter shapes and
        layout do not change.  With both None this is the plain ``o3.Linear``."""
        full_in, full_out = self.full_pieces(self.irreps_in), self.full_pieces(self.irreps_out)
        self._in_pieces = full_in if in_pieces is None else tuple(tuple(p) for p in in_pieces)
        self._out_pieces = full_out if out_pieces is None else tuple(tuple(p) for p in out_pieces)
        for irreps, pieces in ((self.irreps_in, self._in_pieces), (self.irreps_out, self._out_pieces)):
            if list(pieces) != sorted(pieces) or any(
                    c0 < 0 or cnt <= 0 or c0 + cnt > irreps[s].mul for s, c0, cnt in pieces):
                raise ValueError(f"live pieces {pieces} do not fit {irreps}")
        self._pruned = self._in_pieces != full_in or self._out_pieces != full_out
        self._in_poff, self._in_dim = self._piece_offsets(self.irreps_in, self._in_pieces)
        self._out_poff, self._out_dim = self._piece_offsets(self.irreps_out, self._out_pieces)
        self._build_descriptors()

    def _expand_out(self, g: torch.Tensor) -> torch.Tensor:
        """compact output rows -> full ``irreps_out`` rows, zeros elsewhere"""
        full = g.new_zeros(g.shape[0], self.irreps_out.dim)
        for (s, c0, cnt), off in zip(self._out_pieces, self._out_poff):
            d = self.irreps_out[s].ir.dim
            f0 = self._out_off[s] + c0 * d
            full[:, f0: f0 + cnt * d] = g[:, off: off + cnt * d]
        return full

    # -- descriptor tables for the C ABI (built by _set_pieces) ------------------
    def _build_descriptors(self):
        w_offs, off = {}, 0
        for i, o in self.instructions:
            w_offs[(i, o)] = off
            off += self.irreps_in[i].mul * self.irreps_out[o].mul
        self._w_offs = [w_offs[io] for io in self.instructions]
        alpha = dict(zip(self.instructions, self.alpha))
        b_offs, boff = {}, 0
        for o in self.bias_slots:
            b_offs[o] = boff
            boff += self.irreps_out[o].mul
        self._b_offs = b_offs
        ipc, opc = self._in_pieces, self._out_pieces
        # the live (input piece, output piece) pairs: weight block of channels [a, a + ca) x
        # [b, b + cb) of instruction (i, o), first entry w0, row stride mo
        pairs = []
        for pi, (i, a, ca) in enumerate(ipc):
            for qi, (o, b, cb) in enumerate(opc):
                if (i, o) in w_offs:
                    mo = self.irreps_out[o].mul
                    pairs.append((pi, qi, ca, cb, w_offs[(i, o)] + a * mo + b, mo, alpha[(i, o)]))
        self._live_pairs = pairs

        def slots(n_slots, dims, muls, offs, srcs, bias, roffs):
            if n_slots > _lib.LIN_MAXSLOT:
                raise NotImplementedError("too many irreps slots for eelg_linear")
            desc = _lib.LinDesc()
            desc.n_slots = n_slots
            desc.max_jt = max((m + 31) // 32 for m in muls)
            self_max_d = max(dims)
            for s in range(n_slots):
                sl = desc.slot[s]
                sl.y_off, sl.n_out, sl.d = offs[s], muls[s], dims[s]
                sl.bias_off = bias.get(s, -1)
                sl.r_off = roffs[s]
                if len(srcs[s]) > _lib.LIN_MAXSRC:
                    raise NotImplementedError("too many sources for one irreps slot")
                sl.n_src = len(srcs[s])
                for t, (xo, k, wo, ldk, ldj, a) in enumerate(srcs[s]):
                    sl.src[t].x_off, sl.src[t].k, sl.src[t].w_off = xo, k, wo
                    sl.src[t].ldk, sl.src[t].ldj, sl.src[t].alpha = ldk, ldj, a
            return desc, self_max_d

        out_srcs = [[] for _ in opc]
        in_srcs = [[] for _ in ipc]
        for pi, qi, ca, cb, w0, mo, a in pairs:
            out_srcs[qi].append((self._in_poff[pi], ca, w0, mo, 1, a))
            in_srcs[pi].append((self._out_poff[qi], cb, w0, 1, mo, a))
        # a residual operand has the full irreps_out rows: each output piece's place in them
        res_off = [self._out_off[o] + b * self.irreps_out[o].ir.dim for o, b, _ in opc]
        self._fwd_desc, self._fwd_maxd = slots(
            len(opc), [self.irreps_out[o].ir.dim for o, _, _ in opc], [cb for _, _, cb in opc],
            self._out_poff, out_srcs,
            {qi: b_offs[o] + b for qi, (o, b, _) in enumerate(opc) if o in b_offs}, res_off)
        if self._out_pieces != self.full_pieces(self.irreps_out):
            self._fwd_desc.res_row = self.irreps_out.dim
        self._bx_desc, self._bx_maxd = slots(
            len(ipc), [self.irreps_in[i].ir.dim for i, _, _ in ipc], [ca for _, _, ca in ipc],
            self._in_poff, in_srcs, {}, [0] * len(ipc))
        self._bx_res = {}
        if len(pairs) > _lib.LINW_MAXINS:
            raise NotImplementedError("too many instructions for eelg_linear_bwd_w")
        wd = _lib.LinWDesc()
        wd.n_ins = len(pairs)
        wd.max_jt = max([(cb + 31) // 32 for _, _, _, cb, _, _, _ in pairs] or [1])
        wd.max_ut = max([(ca + 31) // 32 for _, _, ca, _, _, _, _ in pairs] or [1])
        for t, (pi, qi, ca, cb, w0, mo, a) in enumerate(pairs):
            e = wd.ins[t]
            e.x_off, e.k, e.g_off = self._in_poff[pi], ca, self._out_poff[qi]
            e.n_out, e.d, e.w_off, e.alpha = cb, self.irreps_in[ipc[pi][0]].ir.dim, w0, a
            e.ldw = 0 if mo == cb else mo
        self._bw_desc = wd
        self._pk_ok = {"fwd": self._packable(self._fwd_desc), "bx": self._packable(self._bx_desc)}
        self._pk_cache = {}
        self._bw_maxd = max([self.irreps_in[ipc[pi][0]].ir.dim for pi, *_ in pairs] or [1])
        # the node slices of grad-W follow the whole linear's tile count, not the live pairs':
        # each weight entry is then summed over the same slices whatever else is live
        self._bw_slice_tiles = sum(((self.irreps_in[i].mul + 31) // 32) * ((self.irreps_out[o].mul + 31) // 32)
                                   for i, o in self.instructions) or 1
        # every weight entry is written by grad-W (else the partial sums start from zeros)
        self._bw_covers = sum(ca * cb for _, _, ca, cb, _, _, _ in pairs) == self.weight_numel

    def _bx_desc_with(self, pieces):
        """the grad-x descriptor for an added gradient in compact rows of ``pieces`` (pieces of
        this linear's input irreps): slots the pieces do not cover add nothing"""
        hit = self._bx_res.get(pieces)
        if hit is not None:
            return hit
        offs, width = self._piece_offsets(self.irreps_in, pieces)
        where = dict(zip(pieces, offs))
        desc = _lib.LinDesc.from_buffer_copy(self._bx_desc)
        desc.res_row = width
        if set(pieces) - set(self._in_pieces):
            raise NotImplementedError(f"added gradient pieces {pieces} are no input pieces "
                                      f"{self._in_pieces} of this linear")
        for s, pc in enumerate(self._in_pieces):
            desc.slot[s].r_off = where.get(pc, -1)
        self._bx_res[pieces] = (desc, width)
        return desc, width

    _packable = staticmethod(packable)

    def _packed(self, which: str, weight):
        """split, alpha-scaled weights of descriptor ``which`` ('fwd' or 'bx') for the packed
        kernel, rebuilt when the weight changes (cached per weight version).  A write through
        ``weight.data`` does not bump the version counter: such writers call
        ``invalidate_packed()`` (``parallel.broadcast_parameters`` and ``load_state_dict`` do)."""
        key = (weight.data_ptr(), weight._version, weight.device)
        hit = self._pk_cache.get(which)
        if hit is not None and hit[0] == key:
            return hit[1]
        desc = self._fwd_desc if which == "fwd" else self._bx_desc
        pk = pack_weights("linear_pack", desc, weight)
        self._pk_cache[which] = (key, pk)
        return pk

    # -- launches ---------------------------------------------------------------
    def _fwd(self, x, weight, bias, residual=None):
        n = x.shape[0]
        y = torch.empty(n, self._out_dim, device=x.device, dtype=torch.float32)
        self._fwd_desc.max_rows = n * self._fwd_maxd
        # (the residual has the full irreps_out rows, also when y holds the live pieces only)
        want = (n, self.irreps_out.dim)
        if residual is not None and (tuple(residual.shape) != want or residual.dtype != torch.float32
                                     or not residual.is_contiguous()):
            raise ValueError(f"residual {tuple(residual.shape)} {residual.dtype}: expected a "
                             f"contiguous float32 {want}")
        linear_apply("linear", "linear_fwd", self._fwd_desc, LIN_X6, x, self._in_dim, weight, bias,
                     residual, n, y, self._out_dim, self._pk_ok["fwd"],
                     lambda: self._packed("fwd", weight.detach()))
        return y

    def _bwd_x(self, gy, weight, extra=None, extra_pieces=None):
        """grad-x; ``extra`` (e.g. a residual's gradient) is added in the epilogue: rows of this
        linear's input layout, or compact rows of ``extra_pieces`` (its other slots add zero)"""
        n = gy.shape[0]
        gx = torch.empty(n, self._in_dim, device=gy.device, dtype=torch.float32)
        desc, width = self._bx_desc, self._in_dim
        if extra is not None and extra_pieces is not None and tuple(extra_pieces) != self._in_pieces:
            desc, width = self._bx_desc_with(tuple(extra_pieces))
        desc.max_rows = n * self._bx_maxd
        if extra is not None:
            extra = extra.contiguous()
            if tuple(extra.shape) != (n, width) or extra.dtype != torch.float32:
                raise ValueError(f"linear grad-x: added gradient {tuple(extra.shape)} does not "
                                 f"match {(n, width)}")
        linear_apply("linear", "linear_bwd_x", desc, LIN_X6, gy, self._out_dim, weight, None, extra,
                     n, gx, self._in_dim, self._pk_ok["bx"],
                     lambda: self._packed("bx", weight.detach()))
        return gx

    def _bwd_w(self, x, gy):
        n = x.shape[0]
        if not self._live_pairs:
            return torch.zeros(self.weight_numel, device=x.device, dtype=torch.float32)
        self._bw_desc.max_rows = n * self._bw_maxd
        # (a pruned linear writes the live weight entries only: the others sum exact zeros)
        return linear_bwd_w("linear_bwd_w", self._bw_desc, x, self._in_dim, gy, self._out_dim, n,
                            self._bw_slice_tiles, self.weight_numel, self._bw_covers)

    def _bwd_bias(self, gy):
        nb = sum(self.irreps_out[o].mul for o in self.bias_slots)
        live = [(self._b_offs[o] + b, off, cnt) for (o, b, cnt), off in zip(self._out_pieces, self._out_poff)
                if o in self._b_offs]
        out = (torch.empty if sum(c for _, _, c in live) == nb else torch.zeros)(
            nb, device=gy.device, dtype=torch.float32)
        for k, off, cnt in live:
            ops.sum_rows(gy[:, off: off + cnt], out=out[k: k + cnt])
        return out


class _LiveLinear(_LinearKernels):
    """A ``Linear`` restricted to pieces of its rows (``Linear.set_live``): its own descriptors
    over compact rows, the module's parameters."""

    def __init__(self, lin: "Linear", in_pieces, out_pieces):
        for k in ("irreps_in", "irreps_out", "instructions", "alpha", "weight_numel", "bias_slots",
                  "_in_off", "_out_off"):
            setattr(self, k, getattr(lin, k))
        self._set_pieces(in_pieces, out_pieces)


class Linear(_LinearKernels, torch.nn.Module):
    """e3nn ``o3.Linear`` on mul-major rows; HIP kernels (``eelg_linear_*``): forward and grad-x
    on bf16 MFMA with fp32-accurate split operands where the irreps qualify
    (``eelg_linear_fwd_pk``), fp32 MFMA otherwise and for grad-W."""

    def __init__(self, irreps_in, irreps_out, internal_weights: bool = True,
                 shared_weights: bool = True, biases: bool = False):
        super().__init__()
        self.irreps_in, self.irreps_out = Irreps(irreps_in), Irreps(irreps_out)
        self.instructions: List[Tuple[int, int]] = [
            (i, o) for i, (_, a) in enumerate(self.irreps_in)
            for o, (_, b) in enumerate(self.irreps_out) if a == b]
        fan = Counter()
        for i, o in self.instructions:
            fan[o] += self.irreps_in[i].mul
        self.alpha = [1.0 / math.sqrt(fan[o]) for _, o in self.instructions]
        self.weight_numel = sum(self.irreps_in[i].mul * self.irreps_out[o].mul
                                for i, o in self.instructions)
        self.weight = torch.nn.Parameter(torch.randn(self.weight_numel))
        self.bias_slots = [o for o, (_, ir) in enumerate(self.irreps_out)
                           if biases and ir.l == 0 and ir.p == 1]
        nb = sum(self.irreps_out[o].mul for o in self.bias_slots)
        if nb:
            self.bias = torch.nn.Parameter(torch.zeros(nb))
        else:
            self.register_parameter("bias", None)
        self._in_off, self._out_off = self.irreps_in.offsets(), self.irreps_out.offsets()
        self._set_pieces(None, None)
        self.live = None             # the variant over live pieces (set_live), used on request
        self._register_state_dict_hook(Linear._emit_derived)

    def _covered(self):
        # e3nn 0.5 masks by the weight instructions only (not the bias instructions)
        return {o for _, o in self.instructions}

    @staticmethod
    def _emit_derived(module, state_dict, prefix, local_metadata):
        ents = [("output_mask", _output_mask(module.irreps_out, module._covered()))]
        if module.bias is None:
            ents.append(("bias", torch.Tensor()))
        _emit_e3nn_buffers(state_dict, prefix, ents)

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys,
                              unexpected_keys, error_msgs):
        _accept_output_mask(state_dict, prefix + "output_mask", self.irreps_out,
                            self._covered(), error_msgs)
        if self.bias is None:
            _accept_empty(state_dict, prefix + "bias", error_msgs)
        super()._load_from_state_dict(state_dict, prefix, local_metadata, strict, missing_keys,
                                      unexpected_keys, error_msgs)
        self.invalidate_packed()

    def invalidate_packed(self) -> None:
        super().invalidate_packed()
        if getattr(self, "live", None) is not None:
            self.live.invalidate_packed()

    def set_live(self, in_pieces=None, out_pieces=None) -> None:
        """Prepare the variant that ``forward(..., live=True)`` runs: only the listed pieces
        ``(slot, first channel, channels)`` of the input / output rows (None: all), compact
        rows, exact zero gradients for the weight entries it does not read
        (``_LinearKernels._set_pieces``).  A plain call computes everything as before."""
        self.live = None
        if in_pieces is not None or out_pieces is not None:
            live = _LiveLinear(self, in_pieces, out_pieces)
            self.live = live if live._pruned else None


    def forward(self, x: torch.Tensor, residual: torch.Tensor = None,
                grad_mailbox: "GradMailbox" = None, live: bool = False) -> torch.Tensor:
        """``o3.Linear``; with ``residual`` returns ``linear(x) + residual`` with the add in the
        kernel epilogue (the layer residual of ``gnn/model.py:92-96``).  ``grad_mailbox``
        shared by the residual-adding linear and the first linear reading the residual moves
        the residual's gradient into that linear's grad-x epilogue (``GradMailbox``)."""
        ops._require_device(x)
        # live: the variant of set_live (compact rows of the live pieces) where one is set
        k = self.live if (live and self.live is not None) else self
        if x.shape[-1] != k._in_dim:
            raise ValueError(f"Linear expects [..., {k._in_dim}], got {tuple(x.shape)}")
        weight, bias = self.weight, self.bias
        side = None
        if ops.OVERLAP and x.is_cuda and torch.is_grad_enabled() and weight.requires_grad:
            side = ops.side_stream(x.device, 2)
            with torch.cuda.stream(side):
                weight = _OnStream.apply(weight, side)
                if bias is not None:
                    bias = _OnStream.apply(bias, side)
        if residual is not None:
            ops._require_device(residual)
            residual = ops._f32(residual)
        return _IrrepsLinearFn.apply(ops._f32(x), weight, bias, k, side, residual, grad_mailbox)


class _GatePlan:
    """The slots a Gate pass runs over: ``scalars`` / ``gated`` slot indices (None: all).  Rows
    are compact: the live scalars, the gates of the live gated slots (one per channel, in slot
    order), the live gated slots."""

    def __init__(self, gate: "Gate", scalars=None, gated=None):
        ns, ng = len(gate.irreps_scalars), len(gate.irreps_gated)
        self.scalars = tuple(range(ns)) if scalars is None else tuple(scalars)
        self.gated = tuple(range(ng)) if gated is None else tuple(gated)
        self.pruned = self.scalars != tuple(range(ns)) or self.gated != tuple(range(ng))
        self.irreps_scalars = Irreps([tuple(gate.irreps_scalars[i]) for i in self.scalars])
        self.irreps_gated = Irreps([tuple(gate.irreps_gated[i]) for i in self.gated])
        self.n_gates = self.irreps_gated.num_irreps
        self.in_dim = self.irreps_scalars.dim + self.n_gates + self.irreps_gated.dim
        self.out_dim = self.irreps_scalars.dim + self.irreps_gated.dim
        self.cst = gate.cst
        self._gdesc = None

    def desc(self):
        if self._gdesc is None:
            d = _lib.GateDesc()
            d.n_scal, d.n_gates, d.n_blk = self.irreps_scalars.dim, self.n_gates, len(self.irreps_gated)
            for b, (mul, ir) in enumerate(self.irreps_gated):
                d.blk_mul[b], d.blk_dim[b] = mul, ir.dim
            self._gdesc = d
        return self._gdesc

    def fits_kernel(self) -> bool:
        return (len(self.irreps_gated) <= _lib.GATE_MAXBLK and self.irreps_gated.dim <= _lib.GATE_MAXGATED
                and self.n_gates <= _lib.GATE_MAXGATES)


class _GateFn(torch.autograd.Function):
    """e3nn ``nn.Gate`` as two fused HIP passes (``eelg_gate_fwd`` / ``eelg_gate_bwd``)."""

    @staticmethod
    def forward(ctx, x, plan: _GatePlan):
        y = torch.empty(x.shape[0], plan.out_dim, device=x.device, dtype=torch.float32)
        _lib.launch("gate_fwd", _lib.load().eelg_gate_fwd, x, x.shape[0], plan.desc(), float(plan.cst),
                    y, on=y)
        ctx.save_for_backward(x)
        ctx.plan = plan
        return y

    @staticmethod
    def backward(ctx, gy):
        (x,) = ctx.saved_tensors
        gy = gy.contiguous()
        gx = torch.empty_like(x)
        _lib.launch("gate_bwd", _lib.load().eelg_gate_bwd, x, gy, x.shape[0], ctx.plan.desc(),
                    float(ctx.plan.cst), gx, on=gx)
        return gx, None


class Gate(torch.nn.Module):
    def __init__(self, irreps_scalars, irreps_gates, irreps_gated):
        super().__init__()
        self.irreps_scalars = Irreps(irreps_scalars)
        self.irreps_gates = Irreps(irreps_gates)
        self.irreps_gated = Irreps(irreps_gated)
        assert self.irreps_gates.num_irreps == self.irreps_gated.num_irreps
        self.irreps_in = self.irreps_scalars + self.irreps_gates + self.irreps_gated
        self.irreps_out = self.irreps_scalars + self.irreps_gated
        self.cst = cg.silu_normalize2mom()
        self._plan = _GatePlan(self)
        self.live = None             # the plan over live slots (set_live), used on request
        self._register_state_dict_hook(Gate._emit_derived)

    def set_live(self, scalars=None, gated=None) -> None:
        """Prepare the pass that ``forward(x, live=True)`` runs: over the listed slots of
        ``irreps_scalars`` and of ``irreps_gated`` (each gated slot with its gates) only, on
        compact rows (``_GatePlan``).  A plain call computes everything as before."""
        plan = _GatePlan(self, scalars, gated)
        self.live = plan if plan.pruned else None

    # e3nn's Gate multiplies with an ElementwiseTensorProduct submodule ``mul`` (external
    # weights: an empty ``weight`` placeholder, and an output mask over the gated irreps)
    @staticmethod
    def _emit_derived(module, state_dict, prefix, local_metadata):
        g = module.irreps_gated
        _emit_e3nn_buffers(state_dict, prefix, [
            ("mul.weight", torch.Tensor()),
            ("mul.output_mask", _output_mask(g, set(range(len(g)))))])

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys,
                              unexpected_keys, error_msgs):
        _accept_output_mask(state_dict, prefix + "mul.output_mask", self.irreps_gated,
                            set(range(len(self.irreps_gated))), error_msgs)
        _accept_empty(state_dict, prefix + "mul.weight", error_msgs)
        super()._load_from_state_dict(state_dict, prefix, local_metadata, strict, missing_keys,
                                      unexpected_keys, error_msgs)

    def _desc(self):
        return self._plan.desc()

    def _fits_kernel(self) -> bool:
        return self._plan.fits_kernel()

    def forward(self, x, live: bool = False):
        plan = self.live if (live and self.live is not None) else self._plan
        if x.shape[-1] != plan.in_dim:
            raise ValueError(f"Gate expects [..., {plan.in_dim}], got {tuple(x.shape)}")
        # the fused HIP passes cover gates up to the kernels' table sizes; wider readouts use
        # the torch form below (the readout tail is outside the HIP hot path)
        if x.is_cuda and x.dtype == torch.float32 and GATE_FUSED and plan.fits_kernel():
            return _GateFn.apply(ops._f32(x), plan)
        # one torch.split instead of per-block slices: its backward is a single cat, where
        # slice backwards would each zero-fill a full [n, dim_in] gradient and add it up
        # (six zero-fill + add pairs per gate; the values are identical either way)
        gated = [mul * ir.dim for mul, ir in plan.irreps_gated]
        pieces = torch.split(x, [plan.irreps_scalars.dim, plan.n_gates] + gated, dim=1)
        act = torch.nn.functional.silu
        scalars = self.cst * act(pieces[0])
        gates = torch.split(self.cst * act(pieces[1]), [mul for mul, _ in plan.irreps_gated], dim=1)
        out = [scalars]
        for (mul, ir), blk, g in zip(plan.irreps_gated, pieces[2:], gates):
            out.append((blk.reshape(-1, mul, ir.dim) * g[:, :, None]).reshape(-1, mul * ir.dim))
        return torch.cat(out, dim=1)


class TensorProduct(torch.nn.Module):
    """Instruction table of the 'uvu' ``o3.TensorProduct`` (no parameters)."""

    def __init__(self, irreps_in1, irreps_in2, irreps_out, instructions):
        super().__init__()
        self.irreps_in1, self.irreps_in2 = Irreps(irreps_in1), Irreps(irreps_in2)
        self.irreps_out = Irreps(irreps_out)
        self.instructions = list(instructions)
        self.weight_numel = sum(self.irreps_in1[i1].mul * self.irreps_in2[i2].mul
                                for i1, i2, *_ in self.instructions)
        self._register_state_dict_hook(TensorProduct._emit_derived)

    # external (per-edge) weights: e3nn holds an empty ``weight`` placeholder buffer
    @staticmethod
    def _emit_derived(module, state_dict, prefix, local_metadata):
        _emit_e3nn_buffers(state_dict, prefix, [
            ("weight", torch.Tensor()),
            ("output_mask", _output_mask(module.irreps_out, {ins[2] for ins in module.instructions}))])

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys,
                              unexpected_keys, error_msgs):
        _accept_output_mask(state_dict, prefix + "output_mask", self.irreps_out,
                            {ins[2] for ins in self.instructions}, error_msgs)
        _accept_empty(state_dict, prefix + "weight", error_msgs)
        super()._load_from_state_dict(state_dict, prefix, local_metadata, strict, missing_keys,
                                      unexpected_keys, error_msgs)
