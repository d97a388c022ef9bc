"""Even-parity hidden irreps (``hidden_irreps='32x0e+32x2e+32x4e'`` at SH lmax 4, ``0e+2e`` at
lmax 2 / 3), CPU part: the structure table of ``gnn/kernel_sets.py``, construction of the HIP
model against the fp64 oracle's module tree, the generator's new sets, and the oracle's own
equivariance with these params.  The device tests are in ``test_gpu_even_hidden.py``."""
from __future__ import annotations

import os
import re
import sys

import pytest
import torch

import oracle.model as omodel

from gnn import cg, kernel_sets
from gnn.irreps import Irreps
from helpers import batch, batch_to, params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "energy-equiv-lattice-gnn_amd", "csrc")
if CSRC not in sys.path:
    sys.path.insert(0, CSRC)

import gen_kernels as gk  # noqa: E402

EVEN = {2: (0, 2), 3: (0, 2), 4: (0, 2, 4)}
NEW_SETS = {"tpB_l2_h02": (2, (0, 2)), "tpB_l3_h02": (3, (0, 2)), "tpB_l4_h024": (4, (0, 2, 4))}


def irreps_of(ls, mul):
    return "+".join(f"{mul}x{l}{'e' if l % 2 == 0 else 'o'}" for l in ls)


def test_table_lists_and_set_names():
    for lmax in kernel_sets.LMAX:
        full, even = kernel_sets.hidden_lists(lmax)
        assert full == tuple(range(lmax + 1)) and even == kernel_sets.LIVE_OUT[lmax]
        assert kernel_sets.tp_set_name(lmax, full) == f"tpB_l{lmax}"
        assert kernel_sets.hidden_irreps_str(lmax, 16) == irreps_of(range(lmax + 1), 16)
    assert kernel_sets.tp_set_name(1, (0,)) == "tpA_l1"           # the first layer's set serves it
    assert {n: (lm, ls) for n, lm, ls in kernel_sets.tp_hidden_sets()} == NEW_SETS
    assert kernel_sets.hidden_irreps_str(4, 32, (0, 2, 4)) == "32x0e+32x2e+32x4e"


@pytest.mark.parametrize("mul", kernel_sets.MULS)
@pytest.mark.parametrize("lmax", [2, 3, 4])
def test_checks_accept_the_even_structures(lmax, mul):
    sh = Irreps.spherical_harmonics(lmax)
    target = Irreps(kernel_sets.coupling_target(lmax, mul))
    assert str((sh * mul).sort()[0].simplify()) == str(target)
    kernel_sets.check_tp(Irreps(irreps_of(EVEN[lmax], mul)), sh, target)
    kernel_sets.check_tp(Irreps(irreps_of(range(lmax + 1), mul)), sh, target)
    for corr in kernel_sets.CORRELATIONS:
        kernel_sets.check_sc(target, EVEN[lmax], corr)
    with pytest.raises(NotImplementedError):      # table-driven path: full outputs only
        kernel_sets.check_sc(target, EVEN[lmax], 4)


@pytest.mark.parametrize("lmax,node", [
    (4, "32x0e+32x2e"),              # (0, 2) at lmax 4: not a generated list
    (4, "32x0e+16x2e+32x4e"),        # mixed channel counts
    (4, "32x1o+32x3o"),              # odd only
    (4, "32x2e+32x4e"),              # no 0e
    (2, "32x0e+32x1o"),              # a hidden lmax below the SH lmax
    (3, "32x0e+32x2e+32x4e"),        # beyond the SH lmax
    (4, "24x0e+24x2e+24x4e"),        # a channel count that is not generated
])
def test_checks_reject_other_structures_and_name_the_lists(lmax, node):
    sh = Irreps.spherical_harmonics(lmax)
    with pytest.raises(NotImplementedError) as ei:
        kernel_sets.check_tp(Irreps(node), sh, Irreps(kernel_sets.coupling_target(lmax, 32)))
    msg = str(ei.value)
    assert "'32x0e+32x2e+32x4e'" in msg and "'32x0e+32x2e'" in msg
    assert "'32x0e+32x1o+32x2e+32x3o+32x4e'" in msg


def test_unsupported_lists_fail_when_the_model_is_built():
    from gnn import EnergyEquivGNN
    for mp in (1, 2):
        with pytest.raises(NotImplementedError) as ei:
            EnergyEquivGNN(params(mp, lmax=4, hidden_irreps="32x0e+32x2e", readout_irreps="16x0e+16x2e"))
        assert "32x0e+32x2e+32x4e" in str(ei.value)
    with pytest.raises(NotImplementedError):
        EnergyEquivGNN(params(2, lmax=4, hidden_irreps="32x0e+16x2e+32x4e"))
    with pytest.raises(NotImplementedError):          # correlation 4: full outputs only
        EnergyEquivGNN(params(2, lmax=2, hidden_irreps="32x0e+32x2e", correlation=4))


CASES = [(4, (0, 2, 4), 32), (3, (0, 2), 32), (2, (0, 2), 16)]


@pytest.mark.parametrize("full_readout", [False, True])
@pytest.mark.parametrize("lmax,ls,mul", CASES)
def test_model_constructs_like_the_oracle(lmax, ls, mul, full_readout):
    """fails without the feature: ``check_tp`` raised NotImplementedError for these params"""
    from gnn import EnergyEquivGNN
    readout = irreps_of(range(lmax + 1) if full_readout else ls, 16)
    p = params(2, lmax=lmax, correlation=2, hidden_irreps=irreps_of(ls, mul), readout_irreps=readout)
    torch.manual_seed(0)
    m = EnergyEquivGNN(p)
    o = omodel.EnergyEquivGNN(p)
    assert ([(n, tuple(q.shape)) for n, q in m.named_parameters()]
            == [(n, tuple(q.shape)) for n, q in o.named_parameters()])
    head = m.stiffness_head
    # everything the hidden irreps hold is live: nothing pruned, no live form prepared
    assert head.live_pruned is False
    assert tuple(ir.l for _, ir in head.live_irreps) == ls
    for layer in head.layers:
        sc = layer.product.symmetric_contractions
        assert sc._live is None and sc._ls == ls and layer.product.linear.live is None
    ro = head.nonlin_readout
    assert ro.linear_1.live is None and ro.linear_2.live is None and ro.equivariant_nonlin.live is None
    # later layers: the new interaction structure, found by its signature under the new name
    inter = head.layers[1].interaction
    assert str(inter.irreps_in) == irreps_of(ls, mul)
    sd_m, sd_o = m.state_dict(), o.state_dict()
    assert set(sd_m) == set(sd_o)
    u_keys = [k for k in sd_m if "U_matrix_" in k]
    assert len(u_keys) == 2 * len(ls) * 2                       # layers x outputs x correlation
    for k in u_keys:
        assert tuple(sd_m[k].shape) == tuple(sd_o[k].shape), k
        assert torch.allclose(sd_m[k].double(), sd_o[k].double(), rtol=0, atol=1e-6), k
    # and it loads back strictly, both ways
    m.load_state_dict(sd_m, strict=True)
    m.load_state_dict(sd_o, strict=True)
    o.load_state_dict(sd_m, strict=True)


def _generated(tmp_path, name):
    with open(os.path.join(tmp_path, name)) as f:
        return f.read()


@pytest.fixture(scope="module")
def gen_dirs(tmp_path_factory):
    """the generator run twice in temporary directories: as committed, and with the hidden-list
    table restricted to the full lists (= before the even sets)"""
    new = str(tmp_path_factory.mktemp("gen_new"))
    old = str(tmp_path_factory.mktemp("gen_full_only"))
    gk.main(new)
    saved = kernel_sets.HIDDEN_LS
    kernel_sets.HIDDEN_LS = {k: v[:1] for k, v in saved.items()}
    try:
        assert kernel_sets.tp_hidden_sets() == ()
        gk.main(old)
    finally:
        kernel_sets.HIDDEN_LS = saved
    return new, old


def test_generator_emits_the_new_sets(gen_dirs):
    new, _ = gen_dirs
    geom = _generated(new, "eelg_gen_geom_hid.hip")
    for mul in kernel_sets.MULS:
        sfx = "" if mul == 32 else f"_m{mul}"
        src = _generated(new, f"eelg_gen_hid_m{mul}.hip")
        assert f"eelg_tp_hid_table_m{mul}(int* n)" in src and "eelg_tp_pad[" in src
        assert "tp_bwf" not in src                               # the fused backward is not widened
        rows = re.findall(r'^  \{"(\w+)", (\d+), (\d+), (\d+), (\d+), .*?0x([0-9a-f]{16})ULL, (.*)\},$',
                          src, re.M)
        assert [r[0] for r in rows] == [n + sfx for n in NEW_SETS]
        for name, din, dmid, wn, nsh, sig, tail in rows:
            lmax, ls = NEW_SETS[name[: -len(sfx)] if sfx else name]
            node, sh = Irreps(irreps_of(ls, mul)), Irreps.spherical_harmonics(lmax)
            target = (sh * mul).sort()[0].simplify()
            assert int(sig, 16) == cg.fnv1a64(cg.tp_signature(node, sh, target))
            paths = cg.tp_paths(node, sh, target)
            mid = cg.tp_out_irreps_with_instructions(node, sh, target)[0]
            assert (int(din), int(dmid), int(wn), int(nsh)) == (node.dim, mid.dim, sum(p.mul for p in paths), sh.dim)
            for k in ("tp_fwd_", "tp_bwd_", "tp_bws_"):
                assert re.search(rf"void {k}{name}\(", src), k + name
                assert (k + name) in tail
            bw = [f"tp_fwd_{name}_bw", f"tp_bwd_{name}_bw", f"tp_bws_{name}_bw"]
            for k in bw:                                         # bf16 storage: mul 32 only
                assert (re.search(rf"void {k}\(", src) is not None) == (mul == 32), k
            assert tail.endswith("nullptr, nullptr") and ", nullptr, nullptr, 4, " in tail   # no tp_bwf
            assert re.search(rf"void tp_bwd_sh_{name}\(", geom)
            assert f'{{"{name}", {(int(nsh) + 3) // 4 * 4}, tp_bwd_sh_{name}}}' in geom
    # the lmax-4 even set at mul 32: the sizes the feature is about
    row = [r for r in re.findall(r'^  \{"tpB_l4_h024", (\d+), (\d+), (\d+), \d+, \d+, (\d+),',
                                 _generated(new, "eelg_gen_hid_m32.hip"), re.M)]
    assert row == [("480", "4288", "768", "24")]


@pytest.mark.parametrize("mul", kernel_sets.MULS)
@pytest.mark.parametrize("name", sorted(NEW_SETS))
def test_forward_row_chunks_of_the_new_sets_stay_in_bounds(name, mul, monkeypatch):
    """the LDS-DMA chunk lists of the new sets' tp_fwd pass the checks of test_gen_tp_glds.py
    (every x block, the SH row and the weight slices moved once, 16-byte aligned, inside their
    rows; the per-lane descriptors reproduce the list)"""
    import test_gen_tp_glds as glds
    monkeypatch.setattr(gk, "tp_configs", gk.tp_hidden_configs)
    glds.test_chunk_lists_cover_the_rows_once_and_stay_in_bounds(name, mul)
    if mul == 32:
        glds.test_lane_descriptors_reproduce_the_chunk_list(name)


def test_old_generated_files_are_unchanged_by_the_new_sets(gen_dirs):
    new, old = gen_dirs
    old_names = sorted(os.listdir(old))
    assert old_names == sorted(["eelg_gen.hip", "eelg_gen_m16.hip", "eelg_gen_m64.hip", "eelg_gen_geom.hip",
                                "eelg_gen_live_m16.hip", "eelg_gen_live_m32.hip", "eelg_gen_live_m64.hip"])
    for name in old_names:
        assert _generated(new, name) == _generated(old, name), name
    assert sorted(set(os.listdir(new)) - set(old_names)) == [
        "eelg_gen_geom_hid.hip", "eelg_gen_hid_m16.hip", "eelg_gen_hid_m32.hip", "eelg_gen_hid_m64.hip"]


@pytest.mark.parametrize("lmax,ls,mul", [(4, (0, 2, 4), 16), (2, (0, 2), 16)])
def test_oracle_even_model_is_equivariant(lmax, ls, mul):
    """rotating positions and shifts rotates the predicted stiffness (fp64, 1e-9 of its largest
    entry; ``positive_function='none'`` so that the raw prediction is compared too)"""
    from helpers_mandel import rotate_mandel
    b, rmax = batch(2, 10, 30, seed=3)
    for pf in ("none", "matrix_power_2"):
        p = params(2, lmax=lmax, correlation=2, max_edge_radius=rmax, hidden_irreps=irreps_of(ls, mul),
                   readout_irreps=irreps_of(ls, 8), positive_function=pf)
        torch.manual_seed(0)
        # built with fp64 as the default type: the oracle's constants (U matrices, the change of
        # basis Q) are then fp64 too; built in fp32 and converted they carry 1e-8 of rounding
        saved = torch.get_default_dtype()
        torch.set_default_dtype(torch.float64)
        try:
            o = omodel.EnergyEquivGNN(p).double()
        finally:
            torch.set_default_dtype(saved)
        bo = batch_to(b, "cpu", torch.float64)
        q = torch.linalg.qr(torch.randn(3, 3, dtype=torch.float64, generator=torch.Generator().manual_seed(4)))[0]
        if torch.det(q) < 0:
            q[:, 0] = -q[:, 0]
        with torch.no_grad():
            c = o(bo)["stiffness"]
            br = batch_to(b, "cpu", torch.float64)
            br.positions = bo.positions @ q.T
            br.shifts = bo.shifts @ q.T
            cr = o(br)["stiffness"]
        want = rotate_mandel(c, q)
        assert float(c.abs().max()) > 0
        assert float((cr - want).abs().max()) <= 1e-9 * float(want.abs().max()), pf
