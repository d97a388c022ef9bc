"""Plain-torch restatement of the NNConv benchmark model (PyG ``NNConv`` with ``aggr='add'``,
``root_weight=False``, ``bias=True`` and the reference's edge MLP) for the parity tests, in
whatever dtype its parameters have (the tests use fp64), plus the ReLU-kink slack of the layer's
gradients.  A gather, ``view(-1, D, D)``, ``matmul`` and ``index_add_``; nothing from ``gnn``."""
from __future__ import annotations

from argparse import Namespace
from typing import Dict

import torch

INDICES = [[0, 1, 2, 3, 4, 5],
           [1, 6, 7, 8, 9, 10],
           [2, 7, 11, 12, 13, 14],
           [3, 8, 12, 15, 16, 17],
           [4, 9, 13, 16, 18, 19],
           [5, 10, 14, 17, 19, 20]]


def nnconv_params(hidden: int = 32, passes: int = 3, positive: str = "square") -> Namespace:
    return Namespace(hidden_irreps=hidden, message_passes=passes, positive=positive)


class NNConvRef(torch.nn.Module):
    """out[n] = sum_{e: recv(e) = n} x[sender(e)] @ relu(nn(edge_ft)[e].view(D, D)) + bias"""

    def __init__(self, d: int, n_edge_ft: int = 5):
        super().__init__()
        self.d = d
        self.nn = torch.nn.Sequential(torch.nn.Linear(n_edge_ft, d), torch.nn.ReLU(),
                                      torch.nn.Linear(d, d), torch.nn.ReLU(),
                                      torch.nn.Linear(d, d * d), torch.nn.ReLU())
        self.bias = torch.nn.Parameter(torch.zeros(d))

    def forward(self, x, edge_index, edge_ft, full: bool = False):
        """``full``: also return the intermediates (z1, h1, z2, h, Z [E, D, D] pre-activation)"""
        sender, receiver = edge_index
        z1 = self.nn[0](edge_ft)
        h1 = torch.relu(z1)
        z2 = self.nn[2](h1)
        h = torch.relu(z2)
        z = self.nn[4](h).view(-1, self.d, self.d)
        msg = torch.matmul(x[sender].unsqueeze(1), torch.relu(z)).squeeze(1)
        out = torch.zeros_like(x).index_add_(0, receiver, msg) + self.bias
        if full:
            return out, {"z1": z1, "h1": h1, "z2": z2, "h": h, "Z": z}
        return out


class NNConvNetRef(torch.nn.Module):
    """The model: embedding, ``h + relu(conv(h))`` per pass, mean pool, SELU head, 6x6."""

    def __init__(self, params: Namespace):
        super().__init__()
        self.register_buffer("indices", torch.tensor(INDICES))
        d = params.hidden_irreps
        self.node_ft_embedding = torch.nn.Linear(1, d)
        self.conv_list = torch.nn.ModuleList([NNConvRef(d) for _ in range(params.message_passes)])
        self.seq = torch.nn.Sequential(torch.nn.Linear(d, 128), torch.nn.SELU(),
                                       torch.nn.Linear(128, 64), torch.nn.SELU(),
                                       torch.nn.Linear(64, 32), torch.nn.SELU(),
                                       torch.nn.Linear(32, 21))
        self.params = params

    def forward(self, batch) -> Dict[str, torch.Tensor]:
        sender, receiver = batch.edge_index
        pos = batch.positions
        vec = pos[receiver] - pos[sender] + batch.shifts          # not normalised
        ln = torch.linalg.norm(vec, dim=-1, keepdim=True)
        edge_ft = torch.cat([vec, ln, batch.edge_attr], dim=1)
        h = self.node_ft_embedding(batch.node_attrs)
        for conv in self.conv_list:
            h = h + torch.relu(conv(h, batch.edge_index, edge_ft))
        pooled = torch.zeros(batch.num_graphs, h.shape[1], dtype=h.dtype).index_add_(0, batch.batch, h)
        cnt = torch.bincount(batch.batch, minlength=batch.num_graphs).clamp_min(1).to(h.dtype)
        c = self.seq(pooled / cnt[:, None])[:, self.indices]
        if self.params.positive == "square":
            return {"stiffness": torch.linalg.matrix_power(c, 2)}
        if self.params.positive == "none":
            return {"stiffness": c}
        raise NotImplementedError(self.params.positive)


def ambiguous(z: torch.Tensor, margin: float = 1e-5) -> torch.Tensor:
    """A = {|Z| < margin * max|Z|}: the entries whose sign an fp32 evaluation may get wrong"""
    z = z.detach().double()
    return z.abs() < margin * z.abs().max()


@torch.no_grad()
def kink_slack(layer: NNConvRef, x, edge_index, edge_ft, inter, gout, amb) -> Dict[str, torch.Tensor]:
    """Per gradient entry, the sum over the ambiguous elements ``amb`` [E, D, D] of Z of the
    absolute contribution of each to that entry, for the loss ``(out * gout).sum()``.  An element
    a = (e, i, o) on the other side of the ReLU kink adds or removes dZ_a = x[sender(e), i]
    gout[recv(e), o]; it enters grad W3[i*D+o, :] (times h[e]), grad b3[i*D+o], grad h[e] (times
    W3[i*D+o, :]) and, through grad h[e] and the two ReLU layers below, the gradients of their
    weights and of edge_ft[e]: each chain evaluated signed for a alone, then |.| and summed over a.
    grad x holds relu(Z) itself (continuous): |Z_a| |gout|; grad bias does not depend on Z.
    Keys: the layer's parameter names, ``x`` and ``edge_ft``."""
    d = layer.d
    sender, receiver = edge_index
    f64 = torch.float64
    x, edge_ft, gout = x.detach().to(f64), edge_ft.detach().to(f64), gout.detach().to(f64)
    w1, w2, w3 = (layer.nn[i].weight.detach().to(f64) for i in (0, 2, 4))
    h, h1 = inter["h"].detach().to(f64), inter["h1"].detach().to(f64)
    m2, m1 = (inter["z2"] > 0).to(f64), (inter["z1"] > 0).to(f64)
    zabs = inter["Z"].detach().to(f64).abs()
    out = {k: torch.zeros_like(p, dtype=f64) for k, p in layer.named_parameters()}
    out["x"], out["edge_ft"] = torch.zeros_like(x), torch.zeros_like(edge_ft)
    idx = amb.nonzero()
    for c in range(0, idx.shape[0], 256):
        e, i, o = idx[c:c + 256].unbind(1)
        q = i * d + o
        dz = x[sender[e], i] * gout[receiver[e], o]                       # [M]
        out["nn.4.weight"].index_put_((q,), (dz[:, None] * h[e]).abs(), accumulate=True)
        out["nn.4.bias"].index_put_((q,), dz.abs(), accumulate=True)
        cz2 = dz[:, None] * w3[q] * m2[e]                                 # [M, D]: grad z2[e] from a
        out["nn.2.weight"] += (cz2[:, :, None] * h1[e][:, None, :]).abs().sum(0)
        out["nn.2.bias"] += cz2.abs().sum(0)
        cz1 = (cz2 @ w2) * m1[e]
        out["nn.0.weight"] += (cz1[:, :, None] * edge_ft[e][:, None, :]).abs().sum(0)
        out["nn.0.bias"] += cz1.abs().sum(0)
        out["edge_ft"].index_put_((e,), (cz1 @ w1).abs(), accumulate=True)
        out["x"].index_put_((sender[e], i), zabs[e, i, o] * gout[receiver[e], o].abs(), accumulate=True)
    return out
