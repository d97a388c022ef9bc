"""The adversarial graph catalogue of ``helpers_graphs.py`` (no GPU needed): every entry has the
property its name claims, computed from its degree vectors and the kernels' walking constants,
so a change of ``nph`` / ``fwpb`` / ``bwf_r`` or of a builder cannot quietly turn a hostile graph
into a tame one; the CSR builder agrees with an independent numpy construction on every entry;
and the vectorised fp64 reference agrees with a loop over the edges."""
import numpy as np
import pytest
import torch

import helpers_graphs as hg

C = hg.constants()
H, T, R, EB, SB, NBUF = (C[k] for k in ("H", "T", "R", "EB", "SB", "NBUF"))
NAMES = list(hg.CATALOGUE)


def _half_sums(deg):
    """in-edges per half-wave range [kH, (k+1)H), padded to whole tiles"""
    d = deg.numpy()
    d = np.concatenate([d, np.zeros(-len(d) % T, dtype=d.dtype)])
    return d.reshape(-1, H).sum(1)


def _zero_runs(deg):
    """maximal [a, b) runs of zeros"""
    runs, a = [], None
    for i, v in enumerate(list(deg.numpy()) + [1]):
        if v == 0 and a is None:
            a = i
        elif v != 0 and a is not None:
            runs.append((a, i))
            a = None
    return runs


def test_constants_are_the_generators():
    import gen_kernels as gk
    assert H == gk.TP_NPH and T == 2 * gk.TP_FWD_WPB * gk.TP_NPH and R == gk.TP_BWF_R
    assert NBUF >= 2 and H >= 4 and T % H == 0 and T % R == 0
    # the launchers' literals (eelg_capi.hip): 8 half-waves per tp_bwd block, (n + 7) / 8 tp_bws blocks
    assert EB % 8 == 0 and SB == 8


@pytest.mark.parametrize("name", NAMES)
def test_entry_is_a_small_valid_graph(name):
    n, ei = hg.graph(name)
    assert 1 <= n <= 150 and ei.shape[1] <= 700
    assert ei.dtype == torch.long and ei.shape[0] == 2
    if ei.shape[1]:
        assert int(ei.min()) >= 0 and int(ei.max()) < n
    din, dout = hg.degrees(name)
    assert int(din.sum()) == int(dout.sum()) == ei.shape[1]


def test_empty_and_self_loop():
    assert hg.graph("empty")[0] == T + 1 and hg.graph("empty")[1].shape == (2, 0)
    assert hg.graph("empty1")[0] == 1 and hg.graph("empty1")[1].shape == (2, 0)
    n, ei = hg.graph("self1")
    assert n == 1 and ei.tolist() == [[0], [0]]


def test_hub_in():
    n, ei = hg.graph("hub_in")
    din, dout = hg.degrees("hub_in")
    hub = T + H - 1
    assert n == 2 * T + 3 and n % T == 3
    assert int(din[hub]) == hg.HUB_EDGES == int(din.sum()) and hg.HUB_EDGES >= 100 * NBUF
    assert hub % T == H - 1                         # the last receiver of a first half-wave
    hs = _half_sums(din)
    k = hub // H
    assert k % 2 == 0 and hs[k] >= 100 and hs[k + 1] == 0     # 600 : 0 inside one wave
    assert hs[:k].sum() == 0 and hs[k + 1:].sum() == 0        # whole tiles of empties around it
    runs = _zero_runs(din)
    assert (0, hub) in runs and (hub + 1, n) in runs and hub >= 3 and n - hub - 1 >= 3
    # one tp_bwf tile holds all the edges
    assert int(din[hub // R * R: hub // R * R + R].sum()) == hg.HUB_EDGES
    assert int((dout > 0).sum()) > SB               # senders in more than one tp_bws block


def test_hub_out():
    n, ei = hg.graph("hub_out")
    din, dout = hg.degrees("hub_out")
    assert int(dout.max()) == hg.HUB_EDGES == ei.shape[1] and int((dout > 0).sum()) == 1
    assert int((din > 0).sum()) > n // 2            # receivers all over
    assert int(dout.argmax()) >= SB                 # not the first tp_bws block


@pytest.mark.parametrize("name,node", [("first_only", 0), ("last_only", -1)])
def test_one_sided(name, node):
    n, ei = hg.graph(name)
    din, _ = hg.degrees(name)
    assert n == 3 * T + 1 and n % T == 1            # the last tile holds one node:
    assert min((n - 1) // T * T + H, n) == n        # its second half starts at n_nodes
    assert int(din[node]) == hg.ONE_SIDED_EDGES == ei.shape[1] > NBUF
    assert int((din > 0).sum()) == 1


def test_gaps():
    n, ei = hg.graph("gaps")
    din, _ = hg.degrees("gaps")
    runs = _zero_runs(din)
    assert runs == hg.gaps_empty_runs()[0]
    assert {b - a for a, b in runs} >= {1, 2, 3, 4, H + 1}
    assert set(din[din > 0].tolist()) == {1, 2, 3, 9}
    crosses = lambda a, b, m: any(a < k < b for k in range(m, n, m))  # noqa: E731
    # a run of >= 3 crosses a half-wave boundary that is no tile boundary; one crosses a tile boundary
    assert any(b - a >= 3 and any(a < k < b and k % T for k in range(H, n, H)) for a, b in runs)
    assert any(b - a >= 3 and crosses(a, b, T) for a, b in runs)
    hs = _half_sums(din)
    halves = [k for k in range(len(hs)) if hs[k] == 0]
    assert any(hs[k] == 0 and hs[k ^ 1] > 0 for k in halves)            # an empty half beside a loaded one
    tiles = [t for t in range(len(hs) * H // T) if hs[t * (T // H):(t + 1) * (T // H)].sum() == 0]
    assert tiles and all(0 < t < (n - 1) // T for t in tiles)           # an empty tile between loaded ones
    # tp_bwf: some R-receiver tile without any edge
    assert any(int(din[a:a + R].sum()) == 0 for a in range(0, n, R))
    assert int(din[0]) > 0 and int(din[n - 1]) > 0


def test_ones_and_the_edge_block_residues():
    for name in ("ones", "ones_full", "ones_plus1", "ones_minus1"):
        din, dout = hg.degrees(name)
        assert bool((din == 1).all()) and bool((dout == 1).all()), name
    n = hg.graph("ones")[0]
    assert n == 8 * T + 5 and -(-n // T) == 9 and -(-9 // 8) * 8 == 16
    es = [int(hg.graph(k)[1].shape[1]) for k in NAMES]
    assert {e % EB for e in es} >= {0, 1, EB - 1}
    assert {-(-e // EB) % 8 for e in es if e} >= {0, 1, 7}      # XCD rounding of tp_bwd_grid
    assert {e % EB for e in es if -(-e // EB) % 8 == 0 and e} >= {0, 1}


def test_short():
    din, _ = hg.degrees("short")
    hs = _half_sums(din)
    assert len(hs) >= 4 and all(0 < v < NBUF for v in hs)
    pos = {int(i) % H for i in torch.nonzero(din).reshape(-1)}
    assert len(pos) >= 4 and {0, H - 1} & pos        # varying positions, an end of a half among them


def test_seesaw():
    n, _ = hg.graph("seesaw")
    hs = _half_sums(hg.degrees("seesaw")[0])
    per_tile = T // H
    assert per_tile == 2 and n == 3 * T
    assert list(hs) == [1, 100, 100, 1, 0, 0]


def test_multi():
    n, ei = hg.graph("multi")
    pairs = [tuple(p) for p in ei.t().tolist()]
    count = {p: pairs.count(p) for p in set(pairs)}
    assert all(count[(i, i)] == 1 for i in range(n))
    fives = [p for p, c in count.items() if c == 5]
    assert sorted(fives) == sorted((s % n, r % n) for s, r in hg.MULTI_PAIRS) and len(fives) == 3
    a, b = hg.MULTI_BOTH_WAYS
    assert count[(a, b)] == 1 and count[(b, a)] == 1
    assert ei.shape[1] == n + 15 + 2 and n % T and n > T


def test_lattice_is_the_control():
    n, ei = hg.graph("lattice")
    din, dout = hg.degrees("lattice")
    assert n == 120 and ei.shape[1] == 480
    assert int(din.min()) >= 2 and int(din.max()) <= 12 and torch.equal(din, dout)
    assert bool((ei[0] // 40 == ei[1] // 40).all())             # three separate graphs


def test_row_maps():
    for name in NAMES:
        e = hg.graph(name)[1].shape[1]
        for which in hg.ROW_MAPS:
            row, s = hg.row_map(name, which)
            assert row.shape == (e,) and (e == 0 or (int(row.min()) == 0 and int(row.max()) == s - 1))
            assert len(set(row.tolist())) == s
    row, s = hg.row_map("gaps", "pairs")
    cnt = torch.bincount(row)
    assert set(cnt.tolist()) == {1, 2} and int((cnt == 2).sum()) == row.shape[0] // 3
    assert torch.equal(hg.row_map("gaps", "id")[0], torch.arange(row.shape[0]))
    assert hg.row_map("gaps", "one")[1] == 1 and hg.row_map("empty", "one")[1] == 0


@pytest.mark.parametrize("name", NAMES)
def test_build_edge_csr_against_numpy(name):
    """``gnn.data.build_edge_csr`` promises: ``perm`` sorts by receiver, stably; ``sperm`` sorts the
    receiver-sorted edges by sender, stably; the two CSRs; ``sender_pos`` inverts ``sperm``"""
    from gnn import ops
    from gnn.data import build_edge_csr
    n, ei = hg.graph(name)
    e = ei.shape[1]
    d = build_edge_csr(ei, n)
    snd, rcv = ei[0].numpy(), ei[1].numpy()
    perm = d["perm"].numpy()
    assert sorted(perm.tolist()) == list(range(e))
    np.testing.assert_array_equal(perm, np.argsort(rcv, kind="stable"))
    receiver, sender = d["receiver"].numpy(), d["sender"].numpy()
    assert d["receiver"].dtype == d["sender"].dtype == d["rowptr"].dtype == d["sperm"].dtype == torch.int32
    np.testing.assert_array_equal(receiver, rcv[perm])
    np.testing.assert_array_equal(sender, snd[perm])
    assert bool((np.diff(receiver) >= 0).all())
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(rcv, minlength=n))])
    srowptr = np.concatenate([[0], np.cumsum(np.bincount(snd, minlength=n))])
    np.testing.assert_array_equal(d["rowptr"].numpy(), rowptr)
    np.testing.assert_array_equal(d["srowptr"].numpy(), srowptr)
    for i in range(n):                              # equal receivers keep the original order
        assert (np.diff(perm[rowptr[i]:rowptr[i + 1]]) > 0).all()
    sperm = d["sperm"].numpy()
    assert sorted(sperm.tolist()) == list(range(e))
    np.testing.assert_array_equal(sperm, np.argsort(sender, kind="stable"))
    for i in range(n):                              # grouped by sender, ascending inside a group
        seg = sperm[srowptr[i]:srowptr[i + 1]]
        assert (sender[seg] == i).all() and (np.diff(seg) > 0).all()
    csr = ops.EdgeCSR.build(ei, n)
    spos = csr.sender_pos().numpy()
    np.testing.assert_array_equal(spos[sperm], np.arange(e))
    np.testing.assert_array_equal(sperm[spos], np.arange(e))


@pytest.mark.parametrize("set_name,name,rows", [("tpB_l1", "gaps", "id"), ("tpB_l1", "multi", "id"),
                                                ("tpB_l1", "multi", "pairs"), ("tpB_l1", "gaps", "one")])
def test_reference_against_a_loop_over_the_edges(set_name, name, rows):
    ref = hg.tp_reference(set_name, name, rows)
    agg, gx = hg.brute_force(set_name, name, rows)
    n, ei = hg.graph(name)
    for got, want, scale in ((ref["agg"], agg, ref["s_agg"]), (ref["gx"], gx, ref["s_gx"])):
        err = (got - want).abs().amax(1)
        assert bool((err <= 1e-13 * scale.amax(1)).all())        # fp64, another summation order
    din, dout = hg.degrees(name)
    assert bool((ref["agg"][din == 0] == 0).all()) and bool((ref["s_agg"][din == 0] == 0).all())
    assert bool((ref["gx"][dout == 0] == 0).all()) and bool((ref["s_gx"][dout == 0] == 0).all())
    assert bool((ref["s_agg"][din > 0].amax(1) > 0).all())
    assert bool((ref["s_agg"] + 1e-300 >= ref["agg"].abs() * (1 - 1e-12)).all())
    # grad-x is the sender sum of the per-edge rows, grad_w / grad_sh are per edge
    e = ei.shape[1]
    assert ref["gxe"].shape[0] == ref["gw"].shape[0] == ref["gsh"].shape[0] == e
    want = torch.zeros_like(gx).index_add_(0, ei[0], ref["gxe"])
    assert torch.equal(ref["gx"], want)


def test_reference_of_an_empty_graph_and_bf16_rounding():
    ref = hg.tp_reference("tpB_l1", "empty")
    assert ref["agg"].shape[0] == T + 1 and not ref["agg"].any() and ref["gw"].shape[0] == 0
    d32, d16 = hg.tp_inputs("tpB_l1", "multi"), hg.tp_inputs("tpB_l1", "multi", True)
    assert torch.equal(d16["ws"], hg.bf16_round(d32["ws"])) and torch.equal(d16["x"], d32["x"])
    rel = ((d16["ws"] - d32["ws"]).abs() / d32["ws"].abs()).max()
    assert 2.0 ** -10 < float(rel) <= 2.0 ** -8      # one round-to-nearest of an 8-bit significand


def test_per_row_criterion_sees_what_the_global_one_hides():
    """``row_error`` on ``hub_in``-like numbers: an error of 1e-3 of a low-degree row's own scale
    is 1e-6 of the tensor's largest entry beside a hub row a thousand times larger, and a stray
    value in a row that must be zero is an assertion, not a ratio"""
    ref = torch.ones(4, 8, dtype=torch.float64)
    ref[2] *= 1000.0                                             # the hub row
    ref[3] = 0.0                                                 # no in-edge
    scale = ref.abs().amax(1)
    out = ref.clone()
    assert hg.row_error(out, ref, scale) == 0.0
    out[0, 5] += 1e-3
    assert float((out - ref).abs().max() / ref.abs().max()) < 1e-5      # the global measure passes it
    assert hg.row_error(out, ref, scale) == pytest.approx(1e-3)
    out = ref.clone()
    out[3, 0] = 1e-30
    with pytest.raises(AssertionError):
        hg.row_error(out, ref, scale)
    # bf16 storage: one rounding of the reference is free, a second one is not
    ref = torch.randn(16, 32, generator=torch.Generator().manual_seed(0), dtype=torch.float64)
    scale = ref.abs().amax(1)
    assert hg.row_error(hg.bf16_round(ref), ref, scale, bf_term=ref) == 0.0
    assert hg.row_error(ref * (1 + 3 * hg.BF16_ROUND), ref, scale, bf_term=ref) > 1e-3
