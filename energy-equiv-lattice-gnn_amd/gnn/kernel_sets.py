"""The irreps structures ``libeelg.so`` has generated kernels for (single source of truth: the
generator ``csrc/gen_kernels.py`` builds exactly these, and the modules check their structure
against them at construction, so an unsupported ``params`` fails when the model is built, with
the supported list, not at the first forward).

Reference ``params`` space (``gnn/model.py:31-42``, ``gnn/mace.py:112-177``): ``lmax`` (SH),
``hidden_irreps``, ``correlation``.  Generated here:

* tensor product: SH lmax 1..4, node irreps ``{mul}x0e`` (first layer) or one of the hidden
  irreps of ``HIDDEN_LS`` (later layers): every natural-parity l up to the SH lmax
  (``{mul}x0e+{mul}x1o+...``, sets ``tpB_l4``), or the even l only (``{mul}x0e+{mul}x2e+{mul}x4e``,
  sets ``tpB_l4_h024``: all the stiffness head reads);
* symmetric contraction: the same lmax, outputs = those hidden irreps, correlation 1..3
  generated; correlation 4 (the reference's ``filter_ir_mid`` coupling) runs the table-driven
  kernels (``csrc/eelg_scg.hip``) for SH lmax <= 3 (``TABLE_LMAX``: at lmax 4 the reference's
  own ``U_matrix_4`` is a [9, 25, 25, 25, 25, K] tensor, gigabytes, and so is its host build);
* live-output contraction sets (``LIVE_OUT``): for every SH lmax and correlation 1..3, the same
  contraction with only the output l that the stiffness head reads from the last layer
  (``sc_l4_c3_o024``); ``check_sc`` accepts exactly these output lists and the full ones;
* ``mul`` (channels per irrep) in ``MULS``: one lane per channel in the interaction kernels, a
  half-wave per 32 channels (mul = 64: two channel groups; mul = 16: half a half-wave).  The
  reference default and the benchmark configurations are 32; bf16 storage of the edge tensors
  (BASELINE config 5) is generated for 32 only.
"""
from __future__ import annotations

from typing import Tuple

MUL = 32
MULS = (16, 32, 64)
LMAX = (1, 2, 3, 4)
CORRELATIONS = (1, 2, 3)
TABLE_CORRELATIONS = (4,)
TABLE_LMAX = 3
# the live-output contraction sets (generated beside the full ones, correlation 1..3): per SH
# lmax, the output l that the stiffness head ``Linear(readout, "2x0e+2x2e+1x4e")`` can read
# from the last layer (``model.live_output_irreps`` derives them from the module structure;
# these are the lists the generator builds, not a rule the model applies)
LIVE_OUT = {1: (0,), 2: (0, 2), 3: (0, 2), 4: (0, 2, 4)}
# the hidden l lists generated per SH lmax (``hidden_irreps`` = mul channels of each listed l,
# natural parity): the full list first, then the even one (= LIVE_OUT[lmax]).  A further list
# (say a hidden lmax below the SH lmax) is one more entry here: the set names, the generator
# and the checks below follow this table.
HIDDEN_LS = {
    1: ((0, 1), (0,)),
    2: ((0, 1, 2), (0, 2)),
    3: ((0, 1, 2, 3), (0, 2)),
    4: ((0, 1, 2, 3, 4), (0, 2, 4)),
}


def natural(l: int) -> str:
    return f"{l}{'e' if l % 2 == 0 else 'o'}"


def hidden_irreps_str(lmax: int, mul: int = MUL, ls: Tuple[int, ...] = None) -> str:
    """``mul`` channels of every l in ``ls`` (default: every l up to ``lmax``)"""
    return "+".join(f"{mul}x{natural(l)}" for l in (range(lmax + 1) if ls is None else ls))


def hidden_lists(lmax: int) -> Tuple[Tuple[int, ...], ...]:
    """the hidden l lists generated for an SH lmax, the full one first"""
    return HIDDEN_LS.get(lmax, ())


def tp_set_name(lmax: int, ls: Tuple[int, ...] = None) -> str:
    """the tensor-product set of hidden l list ``ls`` x SH(lmax): ``tpB_l4`` (every l up to
    lmax), ``tpA_l4`` (scalars only: also the first layer's set) or ``tpB_l4_h024``"""
    if ls is None or tuple(ls) == tuple(range(lmax + 1)):
        return f"tpB_l{lmax}"
    if tuple(ls) == (0,):
        return f"tpA_l{lmax}"
    return f"tpB_l{lmax}_h" + "".join(str(l) for l in ls)


def tp_hidden_sets():
    """(set name, SH lmax, hidden l list) of the sets beyond ``tpA_l*`` / ``tpB_l*``"""
    return tuple((tp_set_name(lmax, ls), lmax, ls) for lmax in LMAX for ls in hidden_lists(lmax)[1:]
                 if ls != (0,))


def coupling_str(lmax: int) -> str:
    return "+".join(natural(l) for l in range(lmax + 1))


def sc_set_name(lmax: int, corr: int, ls: Tuple[int, ...] = None) -> str:
    """``sc_l4_c3`` (every output l up to lmax) or ``sc_l4_c3_o024`` (the listed output l)"""
    base = f"sc_l{lmax}_c{corr}"
    if ls is None or tuple(ls) == tuple(range(lmax + 1)):
        return base
    return base + "_o" + "".join(str(l) for l in ls)


def sc_output_lists(lmax: int) -> Tuple[Tuple[int, ...], ...]:
    """the output l lists generated for a coupling lmax: all of them, the live subset, and the
    hidden l lists of ``HIDDEN_LS`` (a product block's outputs are the hidden irreps; today the
    even list is the live one), each once, the full list first"""
    full = tuple(range(lmax + 1))
    out = [full]
    for ls in (LIVE_OUT.get(lmax),) + tuple(hidden_lists(lmax)):
        if ls is not None and ls not in out:
            out.append(ls)
    return tuple(out)


def supported_text() -> str:
    lists = "; ".join(f"lmax {k}: " + " or ".join(f"'{hidden_irreps_str(k, MUL, ls)}'" for ls in v)
                      for k, v in HIDDEN_LS.items())
    return (f"generated kernel sets: SH lmax in {LMAX} with hidden_irreps of equal channel counts "
            f"(mul in {MULS}; shown for {MUL}) and one of the l lists {lists}; "
            f"correlation in {CORRELATIONS}; correlation "
            f"{TABLE_CORRELATIONS[0]} (table-driven) for SH lmax <= {TABLE_LMAX}; contraction "
            f"outputs: every l up to the SH lmax, or (correlation in {CORRELATIONS}) the live "
            f"lists " + ", ".join(f"lmax {k}: l in {v}" for k, v in LIVE_OUT.items()))


def mul_of(irreps) -> int:
    """the channel count of an all-equal-mul irreps (0 when the muls differ)"""
    muls = {m for m, _ in irreps}
    return muls.pop() if len(muls) == 1 else 0


def check_tp(node, sh, target) -> None:
    """Raise NotImplementedError unless the interaction (node irreps x SH -> target) is a
    generated tensor-product set."""
    lmax = sh.lmax
    mul = mul_of(node)
    ok = (lmax in LMAX and mul in MULS and str(sh) == str(_sh(lmax))
          and str(node) in (f"{mul}x0e",) + tuple(hidden_irreps_str(lmax, mul, ls)
                                                   for ls in hidden_lists(lmax))
          and str(target) == coupling_target(lmax, mul))
    if not ok:
        raise NotImplementedError(
            f"no HIP tensor-product kernels for {node} x {sh} -> {target}; {supported_text()}")


def check_sc(irreps_in, ls: Tuple[int, ...], correlation: int) -> None:
    """Raise NotImplementedError unless the symmetric contraction is a generated set (or a
    table-driven one: correlation 4)."""
    lmax = irreps_in.lmax
    mul = mul_of(irreps_in)
    ok = (lmax in LMAX and mul in MULS and str(irreps_in) == hidden_irreps_str(lmax, mul)
          and tuple(ls) in sc_output_lists(lmax)
          and (correlation in CORRELATIONS
               or (correlation in TABLE_CORRELATIONS and lmax <= TABLE_LMAX
                   and tuple(ls) == tuple(range(lmax + 1)))))
    if not ok:
        raise NotImplementedError(
            f"no HIP symmetric-contraction kernels for {irreps_in} -> l in {tuple(ls)}, "
            f"correlation {correlation}; {supported_text()}")


def coupling_target(lmax: int, mul: int = MUL) -> str:
    """The interaction irreps ``(SH * mul).sort().simplify()`` (``gnn/model.py:36-37``)."""
    return hidden_irreps_str(lmax, mul)


def _sh(lmax: int):
    from .irreps import Irreps
    return Irreps.spherical_harmonics(lmax)


def table_driven(correlation: int) -> bool:
    """the contraction runs the table-driven kernels (eelg_scg_*) instead of a generated set"""
    return correlation in TABLE_CORRELATIONS
