"""fp64 restatement of the 'pna' interaction reduction (``PNASimple``, reference
``gnn/blocks.py:817-848`` with ``gnn/pna.py``) and its pairing with the oracle block.

``pna_ref`` is written from the semantics, with plain torch ops over an ``index`` (receiver of
every message) and no CSR:
  mean = sum / max(deg, 1); min / max = the extreme (0 for a receiver without messages);
  std = sqrt(relu(mean(m^2) - mean^2) + 1e-5);
  out = sum_k sum_s W[0, 3k + s] scale_s(deg) agg_k,  k over (mean, min, max, std),
  s over (identity, log(deg + 1) / avg_log, avg_log / log(deg + 1) [1 at deg 0]).
``route = (argmin, argmax)`` ([n, D] rows of ``m``, -1 for none) forces the kept rows instead of
the extremes: the whole gradient of min / max then goes where the caller says.
"""
from __future__ import annotations

import torch

import oracle.blocks as oblocks

AGGS = ("mean", "min", "max", "std")
SCALERS = ("identity", "amplification", "attenuation")


def pna_aggregates(m, index, n, route=None):
    """(mean, min, max, std) [n, D] and the in-degree [n] of messages ``m`` [E, D]"""
    d = m.shape[1]
    deg = torch.zeros(n, dtype=m.dtype).index_add_(0, index, torch.ones(index.shape[0], dtype=m.dtype))
    cnt = deg.clamp_min(1.0)[:, None]
    idx = index[:, None].expand(-1, d)
    mean = torch.zeros(n, d, dtype=m.dtype).scatter_add(0, idx, m) / cnt
    msq = torch.zeros(n, d, dtype=m.dtype).scatter_add(0, idx, m * m) / cnt
    std = torch.sqrt(torch.relu(msq - mean * mean) + 1e-5)
    if route is None:
        # include_self=False: rows that receive nothing keep the 0 they start with
        mn = torch.zeros(n, d, dtype=m.dtype).scatter_reduce(0, idx, m, "amin", include_self=False)
        mx = torch.zeros(n, d, dtype=m.dtype).scatter_reduce(0, idx, m, "amax", include_self=False)
    else:
        amin, amax = route
        mn = torch.where(amin >= 0, torch.gather(m, 0, amin.clamp_min(0)), torch.zeros(n, d, dtype=m.dtype))
        mx = torch.where(amax >= 0, torch.gather(m, 0, amax.clamp_min(0)), torch.zeros(n, d, dtype=m.dtype))
    return (mean, mn, mx, std), deg


def pna_scalers(deg, avg_log):
    """[n, 3] (identity, amplification, attenuation)"""
    lg = torch.log(deg + 1.0)
    att = torch.where(deg == 0, torch.ones_like(lg), avg_log / lg.clamp_min(1e-300))
    return torch.stack([torch.ones_like(lg), lg / avg_log, att], 1)


def pna_ref(m, index, n, weight, avg_log, route=None):
    """``PNASimple.forward``: ``weight`` is the [1, 12] weight of ``Linear(12, 1, bias=False)``"""
    aggs, deg = pna_aggregates(m, index, n, route)
    sc = pna_scalers(deg, avg_log)
    w = weight.reshape(12)
    out = torch.zeros_like(aggs[0])
    for k in range(4):
        for s in range(3):
            out = out + w[3 * k + s] * sc[:, s, None] * aggs[k]
    return out


def first_extremes(m, index, n):
    """(argmin, argmax) [n, D] int64: the FIRST row of ``m`` (lowest position) that attains each
    receiver's extreme, -1 for a receiver without messages (a plain loop: test sizes only)"""
    d = m.shape[1]
    amin = torch.full((n, d), -1, dtype=torch.long)
    amax = torch.full((n, d), -1, dtype=torch.long)
    for e in range(m.shape[0]):
        r = int(index[e])
        for a, better in ((amin, torch.lt), (amax, torch.gt)):
            cur = a[r]
            take = (cur < 0) | better(m[e], torch.gather(m, 0, cur.clamp_min(0)[None])[0])
            a[r] = torch.where(take, torch.full_like(cur, e), cur)
    return amin, amax


class _PostPN(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.post_pn = torch.nn.Linear(12, 1, bias=False)


def pna_oracle_block(o_int, avg_log, route=None, capture=None):
    """Make an ``oracle.blocks.TensorProductInteractionBlock`` built with reduce 'sum' aggregate
    with ``pna_ref``: it gains the parameter ``pna.post_pn.weight`` (so parameter names pair with
    the device block's), its ``/ agg_norm_const`` becomes ``/ 1``, and during its forward the
    module's ``scatter_sum`` is ``pna_ref``.  ``route``: a dict that may hold ``'args'`` =
    (argmin, argmax) as rows of the block's message tensor (original edge order);
    ``capture``: a dict that receives ``msg`` and ``index`` of the last forward."""
    assert o_int.reduce in ("sum", "add")
    if not hasattr(o_int, "pna"):
        o_int.pna = _PostPN().to(next(o_int.parameters()).dtype)
    o_int.agg_norm_const = 1.0
    inner = type(o_int).forward

    def forward(*a, **k):
        saved = oblocks.scatter_sum

        def agg(msg, index, n):
            if capture is not None:
                capture["msg"], capture["index"] = msg.detach(), index
            return pna_ref(msg, index, n, o_int.pna.post_pn.weight, avg_log,
                           None if route is None else route.get("args"))

        oblocks.scatter_sum = agg
        try:
            return inner(o_int, *a, **k)
        finally:
            oblocks.scatter_sum = saved

    o_int.forward = forward
    return o_int


def pna_oracle_model(o, avg_log):
    """every interaction block of an oracle ``EnergyEquivGNN`` built with 'sum'"""
    for layer in o.stiffness_head.layers:
        pna_oracle_block(layer.interaction, avg_log)
    return o
