"""Adversarial edge graphs for the tensor-product kernels, and their fp64 reference.

The generated interaction kernels (``tp_fwd``, ``tp_bwd``, ``tp_bws``, ``tp_bwd_sh``, ``tp_bwf``)
walk the graph: two receiver ranges per wave, a 2-deep LDS-DMA ring, sender ranges, receiver
tiles dealt over half-waves, an XCD-grouped 1-D grid over edge blocks.  Every entry of the
catalogue below is a small valid graph (``N <= ~150``, ``E <= ~700``) built *from the walking
constants* so that it keeps hitting the same corner when a constant changes:

* ``H``  = ``nph``: receivers per half-wave of ``tp_fwd``;
* ``T``  = ``2 * fwpb * nph``: receivers per ``tp_fwd`` tile (one workgroup);
* ``R``  = ``bwf_r``: receivers per ``tp_bwf`` tile;
* ``EB`` = ``8 * beph``: edges per ``tp_bwd`` block;  ``SB`` = 8 senders per ``tp_bws`` block;
* ``NBUF``: the depth of ``tp_fwd``'s LDS-DMA ring.

The constants come from the generator (``csrc/gen_kernels.py``), which writes them into the
config table the launchers read (``eelg_tp_cfg::nph / beph / fwpb / bwf_r``); the C ABI's
``eelg_tp_info`` does not report them, so there is no second source to disagree with.

``tests/test_graph_catalogue.py`` asserts, from degree vectors alone, that each entry has the
property its name claims; ``tests/test_gpu_tp_graphs.py`` runs the kernels on them.

Plain functions, no fixtures.  Nothing here needs a GPU.
"""
from __future__ import annotations

import functools
import os
import sys
import zlib
from typing import Dict, Tuple

import torch

_CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                     "energy-equiv-lattice-gnn_amd", "csrc")
if _CSRC not in sys.path:
    sys.path.insert(0, _CSRC)

INV = 0.25               # inv_norm of every call (1 / agg_norm_const of the default model)
HUB_EDGES = 600
ONE_SIDED_EDGES = 37

# kernel set -> (SH lmax, the l of the node irreps, channels): tpA = 32x0e nodes (layer 0),
# tpB = the hidden irreps (gnn/kernel_sets.py)
SETS: Dict[str, Tuple[int, Tuple[int, ...], int]] = {
    "tpA_l4": (4, (0,), 32),
    "tpA_l3": (3, (0,), 32),
    "tpB_l4": (4, (0, 1, 2, 3, 4), 32),
    "tpB_l3": (3, (0, 1, 2, 3), 32),
    "tpB_l2": (2, (0, 1, 2), 32),
    "tpB_l1": (1, (0, 1), 32),
    "tpB_l4_m16": (4, (0, 1, 2, 3, 4), 16),
    "tpB_l4_m64": (4, (0, 1, 2, 3, 4), 64),
    "tpB_l4_h024": (4, (0, 2, 4), 32),
}


@functools.lru_cache(maxsize=None)
def constants() -> Dict[str, int]:
    """the walking constants of the generated TP kernels (see the module docstring)"""
    import gen_kernels as gk
    nph, fwpb = gk.TP_NPH, gk.TP_FWD_WPB
    beph = gk.RETIRED_KNOBS["EELG_TP_BWD_EPH"]          # the one emitted form: 1 edge per half-wave
    return dict(H=nph, T=2 * fwpb * nph, R=gk.TP_BWF_R, EB=8 * beph, SB=8, NBUF=gk.TP_FWD_NBUF)


def _gen(name: str) -> torch.Generator:
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


def _edges(snd, rcv) -> torch.Tensor:
    ei = torch.stack([torch.as_tensor(snd, dtype=torch.long), torch.as_tensor(rcv, dtype=torch.long)])
    return ei.reshape(2, -1)


def _shuffled(ei: torch.Tensor, name: str) -> torch.Tensor:
    """arbitrary edge order: the CSR builder, not the catalogue, sorts"""
    return ei[:, torch.randperm(ei.shape[1], generator=_gen(name + "/order"))]


def _from_in_degrees(deg, name: str) -> torch.Tensor:
    """``deg[i]`` edges into node i from random senders"""
    deg = torch.as_tensor(deg, dtype=torch.long)
    rcv = torch.repeat_interleave(torch.arange(deg.shape[0]), deg)
    snd = torch.randint(0, deg.shape[0], (int(rcv.shape[0]),), generator=_gen(name))
    return _shuffled(_edges(snd, rcv), name)


# ---------------------------------------------------------------------------
# the entries: name -> (n_nodes, edge_index [2, E] int64)
# ---------------------------------------------------------------------------
def empty():
    return constants()["T"] + 1, torch.zeros(2, 0, dtype=torch.long)


def empty1():
    return 1, torch.zeros(2, 0, dtype=torch.long)


def self1():
    return 1, torch.zeros(2, 1, dtype=torch.long)


def hub_in():
    """the last receiver of a first half-wave takes 600 edges; nobody else receives"""
    c = constants()
    n = 2 * c["T"] + 3
    deg = torch.zeros(n, dtype=torch.long)
    deg[c["T"] + c["H"] - 1] = HUB_EDGES
    return n, _from_in_degrees(deg, "hub_in")


def hub_out():
    """one sender sends 600 edges to random receivers; nobody else sends"""
    c = constants()
    n = 2 * c["T"] + 3
    rcv = torch.randint(0, n, (HUB_EDGES,), generator=_gen("hub_out"))
    snd = torch.full((HUB_EDGES,), c["SB"] + 3)         # second tp_bws block, an odd slot
    return n, _shuffled(_edges(snd, rcv), "hub_out")


def first_only():
    n = 3 * constants()["T"] + 1
    deg = torch.zeros(n, dtype=torch.long)
    deg[0] = ONE_SIDED_EDGES
    return n, _from_in_degrees(deg, "first_only")


def last_only():
    """the last tile holds one node: its second half-wave has n0 == n1 == n_nodes"""
    n = 3 * constants()["T"] + 1
    deg = torch.zeros(n, dtype=torch.long)
    deg[n - 1] = ONE_SIDED_EDGES
    return n, _from_in_degrees(deg, "last_only")


def gaps_empty_runs():
    """the [a, b) runs of empty receivers of ``gaps``: lengths 1, 2, 3 (across a half-wave
    boundary), 4 (across a tile boundary), H + 1 (all of half-wave 5 and the node before it)
    and T (all of tile 4)"""
    c = constants()
    h, t = c["H"], c["T"]
    runs = [(2, 3), (4, 6), (h - 1, h + 2), (t - 2, t + 2), (5 * h - 1, 6 * h), (4 * t, 5 * t)]
    for (a0, b0), (a1, b1) in zip(runs, runs[1:]):
        assert b0 < a1, "the runs must stay apart: revisit the positions for these constants"
    return runs, 5 * t + 5


def gaps():
    runs, n = gaps_empty_runs()
    pool = (1, 2, 3, 9)
    deg = torch.tensor([pool[(3 * i + 3) % 4] for i in range(n)])
    for a, b in runs:
        deg[a:b] = 0
    return n, _from_in_degrees(deg, "gaps")


def _ones(n: int, name: str):
    perm = torch.randperm(n, generator=_gen(name))
    return n, _shuffled(_edges(torch.arange(n), perm), name)


def ones():
    """a random permutation: in- and out-degree 1 everywhere; 9 tiles, a grid rounded up to 16"""
    return _ones(8 * constants()["T"] + 5, "ones")


def ones_full():
    """E = 8 EB: full edge blocks, a block count that is a multiple of 8"""
    return _ones(8 * constants()["EB"], "ones_full")


def ones_plus1():
    """E = 7 EB + 1: one edge in the last block"""
    return _ones(7 * constants()["EB"] + 1, "ones_plus1")


def ones_minus1():
    """E = 7 EB - 1: the last block one edge short, 7 blocks"""
    return _ones(7 * constants()["EB"] - 1, "ones_minus1")


def short():
    """every half-wave range holds NBUF - 1 edges (fewer than the ring depth), all into one
    receiver whose position inside the half varies"""
    c = constants()
    h, halves = c["H"], 2 * 4
    n = halves * h
    deg = torch.zeros(n, dtype=torch.long)
    for k in range(halves):
        deg[k * h + (3 * k + 1) % h] = c["NBUF"] - 1
    return n, _from_in_degrees(deg, "short")


def seesaw():
    """tile 0: half 0 one edge, half 1 a hundred; tile 1 the reverse; tile 2 empty"""
    c = constants()
    h, t = c["H"], c["T"]
    n = 3 * t
    g = _gen("seesaw/deg")
    deg = torch.zeros(n, dtype=torch.long)
    deg[3] = 1
    deg[t + h + 2] = 1
    for lo in (h, t):                                   # the loaded halves: 100 edges spread over them
        r = lo + torch.randint(0, h, (100,), generator=g)
        deg += torch.bincount(r, minlength=n)
    return n, _from_in_degrees(deg, "seesaw")


MULTI_PAIRS = ((1, 2), (5, 9), (-1, 0))                 # (sender, receiver), 5 parallel edges each
MULTI_BOTH_WAYS = (3, 4)


def multi():
    """a self loop on every node, three pairs with 5 parallel edges, one pair in both directions"""
    n = constants()["T"] + 3
    snd, rcv = list(range(n)), list(range(n))
    for s, r in MULTI_PAIRS:
        snd += [s % n] * 5
        rcv += [r % n] * 5
    a, b = MULTI_BOTH_WAYS
    snd += [a, b]
    rcv += [b, a]
    return n, _shuffled(_edges(snd, rcv), "multi")


def lattice():
    """the control: one SyntheticLattices batch, 3 graphs x 40 nodes / 160 edges"""
    from gnn.data import collate
    from gnn.synthetic import SyntheticLattices
    ds = SyntheticLattices(3, 40, 160, seed=77)
    b = collate([ds[0], ds[1], ds[2]])
    return int(b.positions.shape[0]), b.edge_index.clone()


CATALOGUE = {f.__name__: f for f in (empty, empty1, self1, hub_in, hub_out, first_only, last_only, gaps,
                                     ones, short, seesaw, multi, lattice, ones_full, ones_plus1,
                                     ones_minus1)}
# the entries every kernel set runs (the walking code is shared; the per-set arithmetic differs)
CORE = ("hub_in", "gaps", "last_only", "short", "multi")


@functools.lru_cache(maxsize=None)
def graph(name: str) -> Tuple[int, torch.Tensor]:
    n, ei = CATALOGUE[name]()
    assert ei.dtype == torch.long and ei.shape[0] == 2
    assert ei.numel() == 0 or (0 <= int(ei.min()) and int(ei.max()) < n)
    return n, ei


def degrees(name: str):
    """(in-degree, out-degree) [N] int64"""
    n, ei = graph(name)
    return torch.bincount(ei[1], minlength=n), torch.bincount(ei[0], minlength=n)


# ---------------------------------------------------------------------------
# shared weight rows (the `_rows` kernels): edge e reads weight row ``row[e]``
# ---------------------------------------------------------------------------
ROW_MAPS = ("id", "one", "pairs")


@functools.lru_cache(maxsize=None)
def row_map(name: str, which: str) -> Tuple[torch.Tensor, int]:
    """(row [E] int64 in the catalogue's edge order, the number of rows S): ``id`` every edge its
    own row, ``one`` every edge row 0, ``pairs`` random pairs of edges share a row and about a
    third of the edges stay alone"""
    e = int(graph(name)[1].shape[1])
    if which == "id":
        return torch.arange(e), e
    if which == "one":
        return torch.zeros(e, dtype=torch.long), min(e, 1)
    assert which == "pairs"
    order = torch.randperm(e, generator=_gen(name + "/pairs"))
    k = e // 3                                          # k pairs, e - 2k edges alone
    row_of = torch.cat([torch.arange(k), torch.arange(k), torch.arange(k, e - k)])
    row = torch.empty(e, dtype=torch.long)
    row[order] = row_of
    return row, e - k


# ---------------------------------------------------------------------------
# the fp64 reference
# ---------------------------------------------------------------------------
def irreps_of(ls, mul: int) -> str:
    return "+".join(f"{mul}x{l}{'e' if l % 2 == 0 else 'o'}" for l in ls)


@functools.lru_cache(maxsize=None)
def oracle_tp(set_name: str):
    """(the oracle's TensorProduct in fp64, (din, dmid, wn, nsh)) of a kernel set"""
    import oracle.mace as omace
    import oracle.o3 as oo3
    lmax, ls, mul = SETS[set_name]
    node, sh_ir = oo3.Irreps(irreps_of(ls, mul)), oo3.Irreps.spherical_harmonics(lmax)
    target = (sh_ir * mul).sort()[0].simplify()
    mid, instr = omace.tp_out_irreps_with_instructions(node, sh_ir, target)
    tp = oo3.TensorProduct(node, sh_ir, mid, instr).double()
    return tp, (node.dim, mid.dim, tp.weight_numel, sh_ir.dim)


def bf16_round(t: torch.Tensor) -> torch.Tensor:
    """fp64 -> the fp64 value of its bf16 rounding (through fp32, as the model stores weights)"""
    return t.float().to(torch.bfloat16).double()


@functools.lru_cache(maxsize=None)
def tp_inputs(set_name: str, name: str, bf16: bool = False):
    """fp64 operands of one (set, graph): x [N, din], sh [E, nsh], the weight rows ws [E, wn]
    (bf16-rounded for bf16 storage; a row map reads its first S rows) and the cotangent g
    [N, dmid].  Shared, never written to."""
    import oracle.o3 as oo3
    n, ei = graph(name)
    e = int(ei.shape[1])
    lmax = SETS[set_name][0]
    din, dmid, wn, nsh = oracle_tp(set_name)[1]
    gen = _gen(f"{set_name}/{name}")
    x = torch.randn(n, din, generator=gen, dtype=torch.float64)
    sh = oo3.spherical_harmonics(lmax, torch.randn(e, 3, generator=gen, dtype=torch.float64)).detach()
    ws = torch.randn(e, wn, generator=gen, dtype=torch.float64)
    g = torch.randn(n, dmid, generator=gen, dtype=torch.float64)
    return dict(n=n, e=e, ei=ei, x=x, sh=sh.reshape(e, nsh), ws=bf16_round(ws) if bf16 else ws, g=g)


def _evaluate(tp, ei, n, x, sh, w, g):
    """agg = INV * index_add over receivers of tp(x[sender], sh, w), its gradients for the
    cotangent g by autograd (grad-x per edge, then summed per sender), and the per-row
    absolute-sum scales; any floating type"""
    e = int(ei.shape[1])
    din, dmid = x.shape[1], g.shape[1]
    if e == 0:
        z = lambda *s: torch.zeros(*s, dtype=x.dtype)  # noqa: E731
        return dict(agg=z(n, dmid), s_agg=z(n, dmid), gx=z(n, din), s_gx=z(n, din), gxe=z(0, din),
                    gsh=torch.zeros_like(sh), gw=torch.zeros_like(w))
    xe = x[ei[0]].clone().requires_grad_(True)           # per edge: the gradient is gxe
    she, we = sh.clone().requires_grad_(True), w.clone().requires_grad_(True)
    msg = tp(xe, she, we)
    agg = INV * torch.zeros(n, dmid, dtype=x.dtype).index_add_(0, ei[1], msg)
    gxe, gsh, gw = torch.autograd.grad(agg, [xe, she, we], g)
    msg = msg.detach()
    zero = torch.zeros(n, din, dtype=x.dtype)
    return dict(agg=agg.detach(),
                s_agg=INV * torch.zeros(n, dmid, dtype=x.dtype).index_add_(0, ei[1], msg.abs()),
                gx=zero.clone().index_add_(0, ei[0], gxe), s_gx=zero.clone().index_add_(0, ei[0], gxe.abs()),
                gxe=gxe, gsh=gsh, gw=gw)


@functools.lru_cache(maxsize=None)
def tp_reference(set_name: str, name: str, rows: str = "id", bf16: bool = False):
    """fp64 reference of one (set, graph, row map, storage), in the catalogue's edge order:
    ``agg`` [N, dmid], ``gx`` [N, din], per edge ``gxe`` / ``gsh`` / ``gw`` (the gradient of each
    edge's own copy ``ws[row[e]]``, which is what the kernels store), and the scales ``s_agg`` =
    INV * sum over in-edges of |message| and ``s_gx`` = sum over out-edges of |gxe|.  Computed once
    per case and shared; never written to."""
    tp, _ = oracle_tp(set_name)
    d = tp_inputs(set_name, name, bf16)
    row, s = row_map(name, rows)
    out = _evaluate(tp, d["ei"], d["n"], d["x"], d["sh"], d["ws"][row], d["g"])
    out.update(row=row, n_rows=s)
    return out


BF16_ROUND = 2.0 ** -8      # one round-to-nearest to bf16 (8-bit significand)


def row_error(out, ref, scale, bf_term=None):
    """worst over the rows of max_j (|out - ref| - 2^-8 bf_term)+ / scale[i]; a row whose scale
    is zero must be reproduced exactly"""
    out = out.detach().double().cpu()
    assert out.shape == ref.shape, (out.shape, ref.shape)
    if out.numel() == 0:
        return 0.0
    d = (out - ref).abs()
    if bf_term is not None:
        d = (d - BF16_ROUND * bf_term.abs()).clamp_min(0.0)
    err = d.amax(1)
    live = scale > 0
    assert bool((err[~live] == 0).all()), "a row of zero scale is not reproduced exactly"
    return float((err[live] / scale[live]).max()) if bool(live.any()) else 0.0


def tp_restatement(set_name: str, name: str):
    """the same operation restated in fp32 on the CPU (the oracle's module and operands cast to
    float32) against the fp64 reference: the worst per-row error of the aggregate relative to the
    row's largest reference entry and to its absolute-sum scale, of grad-x to its scale, and of the
    per-edge grad_w / grad_sh rows to their largest reference entries"""
    tp, _ = oracle_tp(set_name)
    d = tp_inputs(set_name, name)
    ref = tp_reference(set_name, name)
    f = lambda t: t.float()  # noqa: E731
    tp32 = type(tp)(tp.irreps_in1, tp.irreps_in2, tp.irreps_out, tp.instructions).float()
    got = _evaluate(tp32, d["ei"], d["n"], f(d["x"]), f(d["sh"]), f(d["ws"]), f(d["g"]))

    def worst(a, b, scale):
        err, sc = (a.double() - b).abs().amax(1), scale.amax(1)
        live = sc > 0
        return float((err[live] / sc[live]).max()) if bool(live.any()) else 0.0
    return dict(agg_vs_row_max=worst(got["agg"], ref["agg"], ref["agg"].abs()),
                agg_vs_abs_sum=worst(got["agg"], ref["agg"], ref["s_agg"]),
                gx_vs_abs_sum=worst(got["gx"], ref["gx"], ref["s_gx"]),
                gw_vs_row_max=worst(got["gw"], ref["gw"], ref["gw"].abs()),
                gsh_vs_row_max=worst(got["gsh"], ref["gsh"], ref["gsh"].abs()))


def brute_force(set_name: str, name: str, rows: str = "id"):
    """``agg`` and ``gx`` by a plain Python loop over the edges, one oracle call per edge (small
    sets only): the check of the vectorised reference's indexing"""
    tp, (din, dmid, wn, nsh) = oracle_tp(set_name)
    d = tp_inputs(set_name, name)
    row, _ = row_map(name, rows)
    ei, n = d["ei"], d["n"]
    agg = torch.zeros(n, dmid, dtype=torch.float64)
    gx = torch.zeros(n, din, dtype=torch.float64)
    for k in range(d["e"]):
        s, r = int(ei[0, k]), int(ei[1, k])
        xs = d["x"][s:s + 1].clone().requires_grad_(True)
        m = INV * tp(xs, d["sh"][k:k + 1], d["ws"][int(row[k])][None])
        agg[r] += m[0].detach()
        gx[s] += torch.autograd.grad(m, xs, d["g"][r:r + 1])[0][0]
    return agg, gx
