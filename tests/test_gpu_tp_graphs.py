"""The tensor-product kernels on the adversarial graph catalogue (``helpers_graphs.py``; its CPU
part is ``test_graph_catalogue.py``) against the fp64 oracle, through the C ABI.

Criteria, per row (a wrong low-degree row must not hide under a hub row):
* a row without in-edges (``agg``) or out-edges (grad-x) is exact zeros, bit for bit;
* fp32 storage: ``max_j |out[i, j] - ref[i, j]| <= 1e-5 * S[i]`` with ``S[i]`` the row's
  absolute-sum scale (``agg``: INV * sum over in-edges of |message|; grad-x: sum over out-edges of
  |gxe|; the largest column of it) or, for the per-edge outputs ``grad_w`` / ``gxe`` /
  ``grad_sh``, the row's largest reference magnitude.  1e-5 is the project's kernel tolerance
  (``TOL`` of test_gpu_even_hidden.py); the fp32 restatement of the operation on the CPU stays
  near 1e-6 of the row maximum and 2e-7 of the absolute-sum scale on the 600-edge hub
  (profiles/tp_graph_parity.md), which leaves about 10x for another summation order;
* bf16 storage: the weights are rounded to bf16 first and the reference is computed from the
  rounded values; ``agg`` is fp32 and keeps the fp32 criterion; ``grad_w`` / ``gxe`` are stored
  through ``eelg_f2bf``, which is ``(__bf16)f``: round to nearest even, so one rounding of the
  fp64 value, ``2^-8 |ref|`` per element, is allowed on top of the fp32 term; grad-x summed from
  bf16 rows gets ``2^-8`` times the sender's sum of |gxe| per element (the sender-order kernel sums
  in fp32 registers and keeps the fp32 criterion);
* every kernel run twice on ``hub_in`` and ``seesaw`` gives bitwise equal outputs.

Guards: every float tensor a kernel reads or writes has one extra row before and after it
(NaN; the kernels get the pointer to row 1, still 16-byte aligned since every row length is a
multiple of 16 B); outputs start as NaN.  After the launch the guard rows of the outputs still
hold the NaN fill bit for bit (no stray store past either end) and the interiors are finite
everywhere (every element written, no out-of-range input row folded in).  The index arrays
``sender`` / ``receiver`` / ``sperm`` / ``wrow`` / ``spos`` carry one guard entry on each side
holding the valid index 0, so a stray index read shows as a wrong number, never as a fault.

The block-level tests run the switchable paths (``TP_BWF``, ``TP_BWC``, ``TP_BWD_SENDER``,
``TP_BWD_SPOS``) on the same graphs with the criteria of test_gpu_tp_fused.py."""
import ctypes
import functools

import pytest
import torch

import helpers_graphs as hg
from helpers import params, record_parity

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-5
INV = hg.INV

FULL = [("tpB_l4", "float32"), ("tpB_l4", "bfloat16"), ("tpA_l4", "float32")]
CORE = [("tpA_l3", "float32"), ("tpB_l3", "float32"), ("tpB_l2", "float32"), ("tpB_l1", "float32"),
        ("tpB_l4_m16", "float32"), ("tpB_l4_m64", "float32"), ("tpB_l4_h024", "float32"),
        ("tpB_l3", "bfloat16")]
CASES = ([(s, st, g) for s, st in FULL for g in hg.CATALOGUE]
         + [(s, st, g) for s, st in CORE for g in hg.CORE])
BLOCK_GRAPHS = ["hub_in", "hub_out", "gaps", "last_only", "seesaw", "multi"]


def _id(case):
    return "-".join(case)


# ---------------------------------------------------------------------------
# guarded device tensors
# ---------------------------------------------------------------------------
class Guarded:
    """``rows`` rows of ``cols`` elements between two guard rows; ``p`` points to row 1"""

    def __init__(self, rows, cols, dtype, fill, data=None):
        self.buf = torch.full((rows + 2, cols), fill, device=DEV, dtype=dtype)
        self.fill = torch.full((cols,), fill, device=DEV, dtype=dtype)
        if data is not None:
            assert tuple(data.shape) == (rows, cols)
            self.buf[1:rows + 1] = data.to(device=DEV, dtype=dtype)
        self.t = self.buf[1:rows + 1]
        row_bytes = cols * self.buf.element_size()
        addr = self.buf.data_ptr() + row_bytes
        assert rows == 0 or self.t.data_ptr() == addr
        if dtype.is_floating_point:
            assert row_bytes % 16 == 0 and addr % 16 == 0, (rows, cols, dtype)
        self.p = ctypes.c_void_p(addr)

    def guards_intact(self):
        bits = {2: torch.int16, 4: torch.int32}[self.buf.element_size()]
        want = self.fill.view(bits)
        return bool(torch.equal(self.buf[0].view(bits), want) and torch.equal(self.buf[-1].view(bits), want))


def g_in(t):
    return Guarded(t.shape[0], t.shape[1], t.dtype, float("nan"), t)


def g_out(rows, cols, dtype=torch.float32):
    return Guarded(rows, cols, dtype, float("nan"))


def g_idx(t):
    """an int32 index array between two guard entries that hold the valid index 0"""
    assert t.dtype == torch.int32 and t.dim() == 1
    return Guarded(t.shape[0], 1, torch.int32, 0, t.reshape(-1, 1))


def check_output(g: Guarded, what):
    assert g.guards_intact(), f"{what}: a guard row was written"
    assert bool(torch.isfinite(g.t).all()), f"{what}: an element was not written, or NaN was read"


# ---------------------------------------------------------------------------
# one (set, storage, graph) on the device; shared, never written to
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def device_case(set_name, storage, name):
    from gnn import _lib, ops
    bf = storage == "bfloat16"
    wdt = torch.bfloat16 if bf else torch.float32
    d = hg.tp_inputs(set_name, name, bf)
    idx, info, _ = _lib.tp_config(set_name)
    assert (info["din"], info["dmid"], info["wn"], info["nsh"]) == hg.oracle_tp(set_name)[1]
    n, e = d["n"], d["e"]
    csr = ops.EdgeCSR.build(d["ei"].to(DEV), n)
    perm = csr.perm.cpu()
    nsh, nshp = info["nsh"], ops.sh_row_stride(info["nsh"])
    sh = torch.zeros(e, nshp)
    sh[:, :nsh] = d["sh"][perm].float()
    c = dict(set=set_name, bf=bf, wdt=wdt, name=name, idx=idx, info=info, n=n, e=e, csr=csr, perm=perm,
             nsh=nsh, nshp=nshp, x=g_in(d["x"].float()), sh=g_in(sh), g=g_in(d["g"].float()),
             w=g_in(d["ws"][perm].to(wdt)),          # bf16 storage: ws is rounded already, so exact
             sender=g_idx(csr.sender), receiver=g_idx(csr.receiver), sperm=g_idx(csr.sperm),
             spos=g_idx(csr.sender_pos()), rows={})
    for m in hg.ROW_MAPS:
        row, s = hg.row_map(name, m)
        # the shared rows stay in the catalogue's edge order, so the identity map, too, is a
        # permutation on the device: sorted edge e reads row perm[e]
        c["rows"][m] = (g_in(d["ws"][:s].to(wdt)), g_idx(row[perm].to(torch.int32).to(DEV)))
    din, dout = hg.degrees(name)
    c["no_in"], c["no_out"] = din == 0, dout == 0
    return c


def _sum_gxe(c, gxe, sorted_rows):
    from gnn import ops
    csr = c["csr"]
    return ops.segment_sum_csr(gxe.t, csr.srowptr, c["n"], idx=None if sorted_rows else csr.sperm)


def run_kernels(c, which):
    """launch the kernels named in ``which`` on fresh NaN outputs; -> {kernel: {output: Guarded | tensor}}"""
    from gnn import _lib
    lib = _lib.load()
    idx, info, csr, n, e, bf = c["idx"], c["info"], c["csr"], c["n"], c["e"], c["bf"]
    din, dmid, wn = info["din"], info["dmid"], info["wn"]
    sfx = "_bf16" if bf else ""
    fn = lambda nm: getattr(lib, nm + sfx)  # noqa: E731
    st = _lib.stream(c["x"].buf)
    P = _lib.ptr
    out = {}
    for k in which:
        if k == "fwd":
            agg = g_out(n, dmid)
            _lib.check(fn("eelg_tp_fwd")(idx, c["x"].p, c["sh"].p, c["w"].p, c["sender"].p, P(csr.rowptr), n,
                                         INV, agg.p, st), k)
            out[k] = dict(agg=agg)
        elif k in ("bwd", "bwd_sorted"):
            gw, gxe = g_out(e, wn, c["wdt"]), g_out(e, din, c["wdt"])
            if k == "bwd":
                _lib.check(fn("eelg_tp_bwd")(idx, c["x"].p, c["sh"].p, c["w"].p, c["sender"].p, c["receiver"].p,
                                             e, c["g"].p, INV, gw.p, gxe.p, st), k)
            else:
                _lib.check(fn("eelg_tp_bwd_sorted")(idx, c["x"].p, c["sh"].p, c["w"].p, c["sender"].p,
                                                    c["receiver"].p, c["spos"].p, e, c["g"].p, INV, gw.p,
                                                    gxe.p, st), k)
            out[k] = dict(gw=gw, gxe=gxe, gx=_sum_gxe(c, gxe, k == "bwd_sorted"))
        elif k == "bws":
            gw, gx = g_out(e, wn, c["wdt"]), g_out(n, din)
            _lib.check(fn("eelg_tp_bwd_sender")(idx, c["x"].p, c["sh"].p, c["w"].p, c["sperm"].p,
                                                P(csr.srowptr), c["receiver"].p, n, c["g"].p, INV, gw.p,
                                                gx.p, st), k)
            out[k] = dict(gw=gw, gx_direct=gx)
        elif k == "bwd_sh":
            gsh = g_out(e, c["nshp"])
            _lib.check(lib.eelg_tp_bwd_sh(idx, c["x"].p, None, c["w"].p, c["sender"].p, c["receiver"].p, e,
                                          c["g"].p, INV, gsh.p, st), k)
            out[k] = dict(gsh=gsh)
        elif k.startswith("fwd_rows_"):
            ws, wrow = c["rows"][k[len("fwd_rows_"):]]
            agg = g_out(n, dmid)
            _lib.check(fn("eelg_tp_fwd_rows")(idx, c["x"].p, c["sh"].p, ws.p, wrow.p, c["sender"].p,
                                              P(csr.rowptr), n, INV, agg.p, st), k)
            out[k] = dict(agg=agg)
        elif k.startswith("bwd_rows_"):
            ws, wrow = c["rows"][k[len("bwd_rows_"):]]
            gw, gxe = g_out(e, wn, c["wdt"]), g_out(e, din, c["wdt"])
            _lib.check(fn("eelg_tp_bwd_rows")(idx, c["x"].p, c["sh"].p, ws.p, wrow.p, c["sender"].p,
                                              c["receiver"].p, None, e, c["g"].p, INV, gw.p, gxe.p, st), k)
            out[k] = dict(gw=gw, gxe=gxe, gx=_sum_gxe(c, gxe, False))
        else:
            raise KeyError(k)
    torch.cuda.synchronize()
    return out


def plain_kernels(c):
    return ["fwd", "bwd", "bwd_sorted", "bws"] + ([] if c["bf"] else ["bwd_sh"])


# ---------------------------------------------------------------------------
# the criteria
# ---------------------------------------------------------------------------
row_error = hg.row_error


def zero_bits(t, rows):
    """rows ``rows`` (bool mask, CPU) of the fp32 tensor ``t`` are +0.0 bit for bit"""
    sel = t[rows.to(t.device)]
    return bool((sel.contiguous().view(torch.int32) == 0).all())


def check_kernels(c, ref, outs):
    """guards + per-row criteria of every output in ``outs``; -> {kernel: {output: error}}"""
    perm, nsh, bf = c["perm"], c["nsh"], c["bf"]
    csr = c["csr"]
    spos = csr.sender_pos().long().cpu()
    per_edge = lambda t: t[perm]  # noqa: E731
    errs = {}
    for k, o in outs.items():
        e_k = {}
        for name, val in o.items():
            if isinstance(val, Guarded):
                check_output(val, f"{k}.{name}")
                t = val.t
            else:
                t = val
                assert bool(torch.isfinite(t).all()), f"{k}.{name}"
            stored_bf = t.dtype == torch.bfloat16
            if name == "agg":
                assert t.dtype == torch.float32
                e_k[name] = row_error(t, ref["agg"], ref["s_agg"].amax(1))
                assert zero_bits(t, c["no_in"]), f"{k}: a receiver without in-edges is not +0"
            elif name in ("gx", "gx_direct"):
                # gx: the sender sum of the stored gxe rows (bf16 rows: one rounding per term)
                from_bf = bf and name == "gx"
                e_k[name] = row_error(t, ref["gx"], ref["s_gx"].amax(1), ref["s_gx"] if from_bf else None)
                assert zero_bits(t, c["no_out"]), f"{k}: a sender without out-edges is not +0"
            elif name == "gw":
                r = per_edge(ref["gw"])
                e_k[name] = row_error(t, r, r.abs().amax(1), r if stored_bf else None)
            elif name == "gxe":
                r = per_edge(ref["gxe"])
                got = t[spos.to(t.device)] if k == "bwd_sorted" else t
                e_k[name] = row_error(got, r, r.abs().amax(1), r if stored_bf else None)
            elif name == "gsh":
                r = per_edge(ref["gsh"])
                e_k[name] = row_error(t[:, :nsh], r, r.abs().amax(1))
                assert bool((t[:, nsh:].contiguous().view(torch.int32) == 0).all()), "SH pad columns"
            else:
                raise KeyError(name)
        errs[k] = e_k
    return errs


def record_and_assert(c, errs):
    tag = f"tp_graph_{c['set']}{'_bf16' if c['bf'] else ''}_{c['name']}"
    for k, e_k in errs.items():
        print(f"{tag}_{k}: " + ", ".join(f"{n} {v:.2e}" for n, v in e_k.items()))
        record_parity(f"{tag}_{k}", **e_k)
    for k, e_k in errs.items():
        for n, v in e_k.items():
            assert v <= TOL, (tag, k, n, v)


# ---------------------------------------------------------------------------
# kernel level
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_tp_kernels_match_the_oracle_per_row(case):
    """tp_fwd, tp_bwd (+ the sender sum through sperm), tp_bwd with sender-order rows (+ the
    index-free sender sum), tp_bws and tp_bwd_sh (fp32), or their bf16-storage entry points"""
    set_name, storage, name = case
    c = device_case(set_name, storage, name)
    ref = hg.tp_reference(set_name, name, "id", c["bf"])
    outs = run_kernels(c, plain_kernels(c))
    record_and_assert(c, check_kernels(c, ref, outs))
    # the two edge-order forms run the same arithmetic: the sender sums agree bit for bit
    assert torch.equal(outs["bwd"]["gx"], outs["bwd_sorted"]["gx"])
    assert torch.equal(outs["bwd"]["gw"].t, outs["bwd_sorted"]["gw"].t)


@pytest.mark.parametrize("rows", hg.ROW_MAPS)
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_tp_rows_kernels_match_the_oracle_per_row(case, rows):
    """eelg_tp_fwd_rows / eelg_tp_bwd_rows (shared weight rows) against the same fp64
    computation on ``w_s[row]``: every edge its own row (in another order than the edges), every
    edge on row 0, random pairs plus edges alone"""
    set_name, storage, name = case
    c = device_case(set_name, storage, name)
    ref = hg.tp_reference(set_name, name, rows, c["bf"])
    outs = run_kernels(c, [f"fwd_rows_{rows}", f"bwd_rows_{rows}"])
    record_and_assert(c, check_kernels(c, ref, outs))


@pytest.mark.parametrize("name", ["hub_in", "seesaw"])
@pytest.mark.parametrize("set_name,storage", FULL)
def test_tp_kernels_are_bitwise_repeatable(set_name, storage, name):
    c = device_case(set_name, storage, name)
    which = plain_kernels(c) + [f"{k}_rows_{m}" for m in hg.ROW_MAPS for k in ("fwd", "bwd")]
    a, b = run_kernels(c, which), run_kernels(c, which)
    for k in which:
        for n, va in a[k].items():
            ta, tb = (va.t, b[k][n].t) if isinstance(va, Guarded) else (va, b[k][n])
            bits = {2: torch.int16, 4: torch.int32}[ta.element_size()]
            assert torch.equal(ta.contiguous().view(bits), tb.contiguous().view(bits)), (k, n)


def test_the_criteria_notice_one_edge_in_the_wrong_row():
    """what a walking bug would do, done to the input instead: tp_fwd gets a (valid) receiver CSR
    in which one boundary is moved by one edge.  On ``gaps`` the last in-edge of a low-degree
    receiver lands in its neighbour: far above the per-row bound.  On ``hub_in`` the hub's last
    edge lands in the empty receiver after it: the row of zero scale is not exact any more."""
    import dataclasses
    for name in ("gaps", "hub_in"):
        c = device_case("tpB_l4", "float32", name)
        ref = hg.tp_reference("tpB_l4", name)
        din, _ = hg.degrees(name)
        i = next(k for k in range(c["n"] - 1) if din[k] > 0 and (din[k + 1] > 0) == (name == "gaps"))
        rowptr = c["csr"].rowptr.clone()
        rowptr[i + 1] -= 1
        moved = dict(c, csr=dataclasses.replace(c["csr"], rowptr=rowptr))
        outs = run_kernels(moved, ["fwd"])
        if name == "gaps":
            assert check_kernels(c, ref, outs)["fwd"]["agg"] > 1e3 * TOL
        else:
            with pytest.raises(AssertionError, match="zero scale"):
                check_kernels(c, ref, outs)


# ---------------------------------------------------------------------------
# the switchable paths on the same graphs
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", BLOCK_GRAPHS)
@pytest.mark.parametrize("set_name", ["tpB_l4", "tpA_l4"])
def test_autograd_switches_match_the_c_abi(set_name, name):
    """``ops.TP_BWD_SENDER`` and ``ops.TP_BWD_SPOS`` through ``ops.tp_interaction``'s autograd:
    bitwise the results of ``eelg_tp_bwd_sender`` / ``eelg_tp_bwd_sorted`` called directly"""
    from gnn import ops
    c = device_case(set_name, "float32", name)
    direct = run_kernels(c, ["fwd", "bwd_sorted", "bws"])
    sh = torch.zeros(c["e"], c["nshp"], device=DEV)
    sh.copy_(c["sh"].t)
    saved = ops.TP_BWD_SENDER, ops.TP_BWD_SPOS
    try:
        for sender, spos, k, gxn in ((True, False, "bws", "gx_direct"), (False, True, "bwd_sorted", "gx")):
            ops.TP_BWD_SENDER, ops.TP_BWD_SPOS = sender, spos
            x = c["x"].t.clone().requires_grad_(True)
            w = c["w"].t.clone().requires_grad_(True)
            agg = ops.tp_interaction(x, sh[:, :c["nsh"]], w, c["csr"], c["idx"], c["info"], INV)
            (agg * c["g"].t).sum().backward()
            torch.cuda.synchronize()
            assert torch.equal(agg.detach(), direct["fwd"]["agg"].t)
            gx = direct[k][gxn]
            assert torch.equal(x.grad, gx.t if isinstance(gx, Guarded) else gx), k
            assert torch.equal(w.grad, direct[k]["gw"].t), k
    finally:
        ops.TP_BWD_SENDER, ops.TP_BWD_SPOS = saved


def rel_err(a, b):
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


@functools.lru_cache(maxsize=None)
def _model():
    from gnn.model import EnergyEquivGNN
    torch.manual_seed(0)
    return EnergyEquivGNN(params(2, lmax=4)).to(DEV)


@functools.lru_cache(maxsize=None)
def _block_inputs(layer, name):
    blk = _model().stiffness_head.layers[layer].interaction
    n, ei = hg.graph(name)
    e = ei.shape[1]
    gen = torch.Generator().manual_seed(17 + layer + e)
    r = lambda *s: torch.randn(*s, generator=gen).to(DEV)  # noqa: E731
    return (blk, r(n, blk.irreps_in.dim), r(e, 25), torch.rand(e, 12, generator=gen).to(DEV), ei.to(DEV),
            r(n, blk.irreps_out.dim))


def _run_block(blk, x, sh, ef, ei, go, fused=False, chunks=0):
    from gnn import ops
    saved = ops.TP_BWF, ops.TP_BWC
    ops.TP_BWF, ops.TP_BWC = fused, chunks
    try:
        for p in blk.parameters():
            p.grad = None
        xd = x.clone().requires_grad_(True)
        y, _ = blk(xd, sh, ef, ei)
        (y * go).sum().backward()
        torch.cuda.synchronize()
        return y.detach(), xd.grad, {k: p.grad.clone() for k, p in blk.named_parameters()}
    finally:
        ops.TP_BWF, ops.TP_BWC = saved


@pytest.mark.parametrize("name", BLOCK_GRAPHS)
@pytest.mark.parametrize("layer", [1, 0], ids=["tpB_l4", "tpA_l4"])
def test_fused_and_chunked_backward_on_the_catalogue(layer, name):
    """``eelg_tp_bwd_fused`` against the unfused path (forward and the output linear's weight /
    bias gradients bitwise, the rest 1e-5 of each tensor's largest entry: the criterion of
    test_gpu_tp_fused.py), and the receiver-chunked backward (3 and 8 chunks: bounds inside empty
    runs and right after a hub) bitwise equal to one pass"""
    blk, x, sh, ef, ei, go = _block_inputs(layer, name)
    idx, _ = blk._config()
    assert blk._bwf(idx), "fused path not generated / not matching the linear"
    y_ref, gx_ref, gp_ref = _run_block(blk, x, sh, ef, ei, go)
    assert bool(torch.isfinite(y_ref).all() and torch.isfinite(gx_ref).all())
    y, gx, gp = _run_block(blk, x, sh, ef, ei, go, fused=True)
    assert torch.equal(y, y_ref)
    errs = dict(grad_x=rel_err(gx, gx_ref))
    for k in gp_ref:
        if k.startswith("linear."):
            assert torch.equal(gp[k], gp_ref[k]), k
        else:
            errs[k] = rel_err(gp[k], gp_ref[k])
    record_parity(f"tp_graph_block_{'tpB_l4' if layer else 'tpA_l4'}_{name}_bwf", **errs)
    for k, v in errs.items():
        assert v < TOL, (k, v)
    for chunks in (3, 8):
        y, gx, gp = _run_block(blk, x, sh, ef, ei, go, chunks=chunks)
        assert torch.equal(y, y_ref) and torch.equal(gx, gx_ref), chunks
        for k in gp_ref:
            assert torch.equal(gp[k], gp_ref[k]), (chunks, k)
