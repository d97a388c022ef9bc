"""'pna' interaction reduction, host side: the fp64 restatement against answers worked by hand,
construction and state_dict names, ``degree_stats``, and the C declarations against the
binding.  The kernels themselves are tested on the device in ``test_gpu_pna.py``."""
import math
import os
import re

import pytest
import torch

from helpers import params
from helpers_pna import first_extremes, pna_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A = 1.6
STATS = {"lin": 4.0, "log": A}


def _one_hot(j):
    w = torch.zeros(1, 12, dtype=torch.float64)
    w[0, j] = 1.0
    return w


def test_known_answers_two_messages_and_weight_order():
    """One receiver, messages 1 and 3: mean 2, min 1, max 3, std sqrt(1 + 1e-5); deg 2 gives
    the scalers 1, log(3) / A, A / log(3).  A one-hot weight at 3k + s picks aggregate k
    (mean, min, max, std) times scaler s (identity, amplification, attenuation)."""
    m = torch.tensor([[1.0], [3.0]], dtype=torch.float64)
    index = torch.tensor([0, 0])
    aggs = (2.0, 1.0, 3.0, math.sqrt(1.0 + 1e-5))
    scal = (1.0, math.log(3.0) / A, A / math.log(3.0))
    for k in range(4):
        for s in range(3):
            got = float(pna_ref(m, index, 1, _one_hot(3 * k + s), A))
            assert got == pytest.approx(aggs[k] * scal[s], rel=1e-14), (k, s)
    w = torch.arange(1.0, 13.0, dtype=torch.float64).view(1, 12)
    want = sum(float(w[0, 3 * k + s]) * aggs[k] * scal[s] for k in range(4) for s in range(3))
    assert float(pna_ref(m, index, 1, w, A)) == pytest.approx(want, rel=1e-14)


def test_known_answer_empty_receiver():
    """No messages: mean = min = max = 0 and std = sqrt(1e-5); amplification is log(1) / A = 0
    and attenuation is 1, so only W[9] and W[11] reach the output."""
    m = torch.tensor([[1.0], [3.0]], dtype=torch.float64)
    index = torch.tensor([1, 1])
    w = torch.arange(1.0, 13.0, dtype=torch.float64).view(1, 12)
    out = pna_ref(m, index, 2, w, A)
    assert float(out[0]) == pytest.approx((10.0 + 12.0) * math.sqrt(1e-5), rel=1e-14)
    for j in range(12):
        got = float(pna_ref(m, index, 2, _one_hot(j), A)[0])
        want = math.sqrt(1e-5) if j in (9, 11) else 0.0
        assert got == pytest.approx(want, rel=1e-14, abs=0.0), j


def test_routed_restatement_and_first_extremes():
    """ties: the first row of the segment is the kept one, and routing through the kept rows
    sends the whole min / max gradient there"""
    m = torch.tensor([[1.0, 0.5], [1.0, -1.0], [0.0, 0.5], [1.0, 0.5]], dtype=torch.float64)
    index = torch.tensor([0, 0, 0, 2])
    amin, amax = first_extremes(m, index, 3)
    assert amin.tolist() == [[2, 1], [-1, -1], [3, 3]]
    assert amax.tolist() == [[0, 0], [-1, -1], [3, 3]]
    w = torch.zeros(1, 12, dtype=torch.float64)
    w[0, 6] = 1.0                                   # max x identity
    x = m.clone().requires_grad_(True)
    out = pna_ref(x, index, 3, w, A, route=(amin, amax))
    assert torch.equal(out.detach(), torch.tensor([[1.0, 0.5], [0.0, 0.0], [1.0, 0.5]], dtype=torch.float64))
    out.sum().backward()
    assert x.grad.tolist() == [[1.0, 1.0], [0.0, 0.0], [0.0, 0.0], [1.0, 1.0]]


def _block(agg_norm_const, reduce="pna"):
    from gnn.blocks import TensorProductInteractionBlock
    from gnn.irreps import Irreps
    sh = Irreps.spherical_harmonics(2)
    tgt = (sh * 32).sort()[0].simplify()
    return TensorProductInteractionBlock("32x0e+32x1o+32x2e", sh, "12x0e", tgt, agg_norm_const, reduce)


def test_block_takes_a_mapping_and_owns_post_pn():
    from gnn.blocks import INTERACTION_REDUCTIONS
    assert "pna" in INTERACTION_REDUCTIONS
    b = _block(STATS)
    names = dict(b.named_parameters())
    assert tuple(names["pna.post_pn.weight"].shape) == (1, 12)
    assert not any(k.startswith("pna.") and k != "pna.post_pn.weight" for k in b.state_dict())
    assert b.pna.avg_deg["log"] == A
    _block({"log": 2.0})                             # 'lin' is unused and may be absent
    _block(STATS, "PNA")


def test_block_refuses_a_number_and_a_mapping_without_log():
    with pytest.raises(NotImplementedError, match="pna"):
        _block(4.0)
    with pytest.raises(NotImplementedError, match="mapping"):
        _block(4.0)
    with pytest.raises(Exception, match="log"):
        _block({"lin": 4.0})
    # every other reduce keeps the number
    assert _block(4.0, "max").agg_norm_const == 4.0 and not hasattr(_block(4.0, "max"), "pna")


def test_model_state_dict_names_and_strict_round_trip():
    from gnn import EnergyEquivGNN
    p = params(2, interaction_reduction="pna", agg_norm_const=dict(STATS))
    torch.manual_seed(0)
    m = EnergyEquivGNN(p)
    sd = m.state_dict()
    for i in (0, 1):
        key = f"stiffness_head.layers.{i}.interaction.pna.post_pn.weight"
        assert key in sd and tuple(sd[key].shape) == (1, 12)
    torch.manual_seed(1)
    m2 = EnergyEquivGNN(p)
    key = "stiffness_head.layers.1.interaction.pna.post_pn.weight"
    assert not torch.equal(m2.state_dict()[key], sd[key])
    m2.load_state_dict(sd, strict=True)
    assert torch.equal(m2.state_dict()[key], sd[key])
    # the same network with 'sum' has every other key and no pna ones
    ps = params(2)
    other = set(EnergyEquivGNN(ps).state_dict())
    assert set(sd) - other == {f"stiffness_head.layers.{i}.interaction.pna.post_pn.weight" for i in (0, 1)}
    assert other <= set(sd)


def test_degree_stats_on_a_hand_made_graph():
    from gnn import degree_stats
    # receivers: node 0 three times, node 1 once, node 2 never, node 3 twice
    ei = torch.tensor([[1, 2, 3, 0, 0, 1], [0, 0, 0, 1, 3, 3]])
    st = degree_stats(ei, 4)
    assert set(st) == {"lin", "log"}
    assert st["lin"] == pytest.approx(6 / 4)
    assert st["log"] == pytest.approx((math.log(4) + math.log(2) + 0.0 + math.log(3)) / 4)
    assert degree_stats(torch.zeros(2, 0, dtype=torch.long), 3) == {"lin": 0.0, "log": 0.0}


@pytest.mark.parametrize("name", ["eelg_segment_pna_fwd", "eelg_segment_pna_bwd", "eelg_segment_pna_parts"])
def test_entry_points_declared_as_bound(name):
    from gnn import _lib
    text = open(os.path.join(ROOT, "include", "eelg.h")).read()
    found = re.findall(r"\b(?:int|long long)\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
    assert len(found) == 1, name
    n_args = len([a for a in found[0].split(",") if a.strip()])
    assert name in _lib._SIGS and name in _lib.EXPORTED_SYMBOLS
    assert n_args == len(_lib._SIGS[name][0]), (n_args, _lib._SIGS[name][0])
    src = open(os.path.join(ROOT, "energy-equiv-lattice-gnn_amd", "csrc", "eelg_pna.hip")).read()
    assert re.search(r"\b" + name + r"\s*\(", src)
    assert "eelg_pna.o" in open(os.path.join(ROOT, "energy-equiv-lattice-gnn_amd", "csrc", "Makefile")).read()
