"""NNConv benchmark model on the HIP path.

``NNConvNet`` mirrors scripts/benchmark_models/nnconv_models.py:8-87 and ``NNConv`` the PyG
layer it builds (``NNConv(D, D, nn, aggr='add', root_weight=False)``, :32-44), with the
reference's parameter names.  PyG has the edge MLP emit a ``D x D`` matrix per edge and
multiplies ``x[sender]`` by it, which materialises ``[E, D*D]`` three times over (forward,
saved for backward, gradient).  Here the MLP's last Linear + ReLU and the per-edge product are
one fused kernel (``eelg_nnconv_fwd``) and two backward kernels (``eelg_nnconv_bwd_edge`` /
``eelg_nnconv_bwd_w``) that keep the matrices in MFMA accumulators; the largest tensors are
``[E, D]``.  The MLP's first two layers (5 -> D -> D) are ordinary modules, so autograd
carries the kernels' ``grad_h`` on to their parameters and to the edge inputs (geometry).
"""
from __future__ import annotations

import os
from argparse import Namespace
from typing import Dict, Optional, Tuple

import torch

from . import _lib, dense, ops
from .blocks import EdgeIndex, as_csr, mat_square
from .cgc import INDS_VAL

# 1 (default): the fused kernels.  0: the same layer as the materialised torch formulation on
# the device ([E, D*D] formed, as PyG does), for A/B timing only.
NNCONV_FUSED = os.environ.get("EELG_NNCONV_FUSED", "1") != "0"


class _NNConvFn(torch.autograd.Function):
    """agg[n] = sum_{e: recv(e) = n} sum_i x[sender(e), i] relu(h[e] W3_i^T + b3_i), edges in CSR
    order.  Z is recomputed in the backward; saved: x, h and the weights."""

    @staticmethod
    def forward(ctx, x, h, w3, b3, csr: ops.EdgeCSR):
        x, h, w3, b3 = ops._a16(x), ops._a16(h), ops._a16(w3), ops._a16(b3)
        n, d = x.shape
        e = csr.num_edges
        if h.shape != (e, d) or w3.shape != (d * d, d) or b3.shape != (d * d,) or n != csr.num_nodes:
            raise ValueError(f"NNConv shapes: x {tuple(x.shape)}, h {tuple(h.shape)}, w3 {tuple(w3.shape)}, "
                             f"b3 {tuple(b3.shape)}, csr {csr.num_nodes} nodes / {e} edges")
        msg = torch.empty(e, d, device=x.device, dtype=torch.float32)
        ops._launch("nnconv_fwd", _lib.load().eelg_nnconv_fwd, x, h, w3, b3, csr.sender, e, d, msg,
                    on=msg, timed="nnconv_fwd")
        ctx.save_for_backward(x, h, w3, b3)
        ctx.csr = csr
        return ops.segment_sum_csr(msg, csr.rowptr, n)

    @staticmethod
    def backward(ctx, g):
        x, h, w3, b3 = ctx.saved_tensors
        csr = ctx.csr
        n, d = x.shape
        e = csr.num_edges
        g = ops._a16(g)
        lib = _lib.load()
        gxe = torch.empty(e, d, device=x.device, dtype=torch.float32)
        gh = torch.empty(e, d, device=x.device, dtype=torch.float32)
        ops._launch("nnconv_bwd_edge", lib.eelg_nnconv_bwd_edge, x, h, w3, b3, csr.sender,
                    csr.receiver, e, d, g, gxe, gh, on=g, timed="nnconv_bwd_edge")
        gx = ops.segment_sum_csr(gxe, csr.srowptr, n, idx=csr.sperm)   # per-sender sums
        gw3 = gb3 = None
        if ctx.needs_input_grad[2] or ctx.needs_input_grad[3]:
            nparts = int(lib.eelg_nnconv_bwd_w_parts(e, d))
            if nparts < 0:
                _lib.check(nparts, "nnconv_bwd_w_parts")
            if nparts == 0:
                tot = torch.zeros(d * d * (d + 1), device=x.device, dtype=torch.float32)
            else:
                part = torch.empty(nparts, d * d * (d + 1), device=x.device, dtype=torch.float32)
                ops._launch("nnconv_bwd_w", lib.eelg_nnconv_bwd_w, x, h, w3, b3, csr.sender,
                            csr.receiver, e, d, g, part, on=g, timed="nnconv_bwd_w")
                tot = ops.sum_rows(part)          # the edge splits' partials, fixed order
            gw3, gb3 = tot[:d * d * d].view(d * d, d), tot[d * d * d:]
        return gx, gh, gw3, gb3, None


def nnconv_materialised(x: torch.Tensor, h: torch.Tensor, w3: torch.Tensor, b3: torch.Tensor,
                        csr: ops.EdgeCSR) -> Tuple[torch.Tensor, torch.Tensor]:
    """The same sums as PyG writes them (plain torch on the device, ``[E, D, D]`` formed):
    returns (agg, Z) with Z the pre-activation ``[E, D, D]``."""
    d = x.shape[1]
    z = torch.nn.functional.linear(h, w3, b3).view(-1, d, d)
    msg = torch.matmul(x[csr.sender.long()].unsqueeze(1), torch.relu(z)).squeeze(1)
    agg = torch.zeros_like(x).index_add_(0, csr.receiver.long(), msg)
    return agg, z


def _edge_mlp(d: int) -> torch.nn.Sequential:
    """nn of nnconv_models.py:33-41: Linear(5, D)-ReLU-Linear(D, D)-ReLU-Linear(D, D*D)-ReLU.
    Modules 4 and 5 only hold the parameters / mark the ReLU: they run inside the kernels."""
    return torch.nn.Sequential(dense.SmallInLinear(5, d), torch.nn.ReLU(),
                               dense.Linear(d, d), torch.nn.ReLU(),
                               torch.nn.Linear(d, d * d), torch.nn.ReLU())


class NNConv(torch.nn.Module):
    """PyG ``NNConv(D, D, nn, aggr='add', root_weight=False, bias=True)`` with the edge MLP
    ``nn`` of the reference model; parameters ``nn.0.*``, ``nn.2.*``, ``nn.4.*``, ``bias``.
    ``forward(x, edge_index, edge_ft)``; ``edge_index`` may be an ``ops.EdgeCSR`` (then
    ``edge_ft`` [E, 5] is in CSR edge order)."""

    def __init__(self, channels: int, nn: Optional[torch.nn.Sequential] = None):
        super().__init__()
        d = int(channels)
        if d not in _lib.NNC_WIDTHS:
            raise NotImplementedError(f"NNConv: width {d} is not built; the fused kernels exist for "
                                      f"D in {_lib.NNC_WIDTHS} (include/eelg.h EELG_NNC_MAXD)")
        nn = _edge_mlp(d) if nn is None else nn
        lins = [nn[i] for i in (0, 2, 4)] if len(nn) == 6 else []
        if (len(lins) != 3 or tuple(lins[1].weight.shape) != (d, d) or lins[0].weight.shape[0] != d
                or tuple(lins[2].weight.shape) != (d * d, d)
                or not all(isinstance(nn[i], torch.nn.ReLU) for i in (1, 3, 5))):
            raise NotImplementedError("NNConv: nn must be Linear(F, D)-ReLU-Linear(D, D)-ReLU-"
                                      "Linear(D, D*D)-ReLU (the reference model's edge MLP)")
        self.channels = d
        self.nn = nn
        self.bias = torch.nn.Parameter(torch.zeros(d))

    def forward(self, x: torch.Tensor, edge_index: EdgeIndex, edge_ft: torch.Tensor) -> torch.Tensor:
        ops._require_device(x, edge_ft)
        csr, edge_ft = as_csr(edge_index, x.shape[0], edge_ft)
        h = self.nn[3](self.nn[2](self.nn[1](self.nn[0](edge_ft))))
        w3, b3 = self.nn[4].weight, self.nn[4].bias
        if NNCONV_FUSED:
            agg = _NNConvFn.apply(x, h, w3, b3, csr)
        else:
            agg = nnconv_materialised(x, h, w3, b3, csr)[0]
        return agg + self.bias


def _edge_inputs(batch, csr: ops.EdgeCSR) -> torch.Tensor:
    """[edge vector | length | strut radius] in CSR edge order; the vector is NOT normalised
    (nnconv_models.py:66-70 calls get_edge_vectors_and_lengths with normalize=False)."""
    pos = batch.positions
    vec = pos[csr.receiver.long()] - pos[csr.sender.long()] + batch.shifts[csr.perm]
    ln = torch.linalg.norm(vec, dim=-1, keepdim=True)
    return torch.cat([vec, ln, batch.edge_attr[csr.perm]], dim=1)


class NNConvNet(torch.nn.Module):
    """``nnconv_models.py:8-87``: node embedding, ``message_passes`` x ``h + relu(conv(h))``,
    global mean pool, SELU head to 21 values -> symmetric 6x6 -> ``positive``."""

    def __init__(self, params: Namespace):
        super().__init__()
        self.register_buffer("indices", torch.tensor(INDS_VAL))
        self.dim_inner = int(params.hidden_irreps)
        self.num_mp = params.message_passes
        d = self.dim_inner
        self.node_ft_embedding = dense.SmallInLinear(1, d)
        self.conv_list = torch.nn.ModuleList([NNConv(d) for _ in range(self.num_mp)])
        self.seq = torch.nn.Sequential(dense.Linear(d, 128), torch.nn.SELU(),
                                       dense.Linear(128, 64), torch.nn.SELU(),
                                       dense.Linear(64, 32), torch.nn.SELU(),
                                       dense.Linear(32, 21))
        self.params = params

    def forward(self, batch) -> Dict[str, torch.Tensor]:
        from .model import EnergyEquivGNN
        ops._require_device(batch.positions, batch.node_attrs)
        csr = EnergyEquivGNN.edge_graph(batch, strut=False)
        edge_ft = _edge_inputs(batch, csr)
        h = self.node_ft_embedding(batch.node_attrs)
        for conv in self.conv_list:
            h = h + torch.relu(conv(h, csr, edge_ft))
        a = self.seq(ops.graph_pool(h, batch.batch, batch.num_graphs, "mean"))[:, self.indices]
        if self.params.positive == "square":
            return {"stiffness": mat_square(a)}
        if self.params.positive == "none":
            return {"stiffness": a}
        raise NotImplementedError(self.params.positive)


__all__ = ["NNConv", "NNConvNet", "nnconv_materialised", "NNCONV_FUSED"]
