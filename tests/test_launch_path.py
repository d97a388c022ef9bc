"""The one launch path and the linear launch helpers (CPU): the names ``ops`` re-exports are the
objects of ``_lib``, the shared packed-path rule is ``dense``'s former condition, and the grad-W
slice plan is its formula.  No library call, no launch."""
import itertools

import pytest

from gnn import _lib, dense, o3, ops


def test_ops_reexports_the_launcher_of_lib():
    assert ops.TIMER is _lib.TIMER and ops.KernelTimer is _lib.KernelTimer
    assert ops._launch is _lib.launch


@pytest.mark.parametrize("switch", [True, False])
def test_shared_packed_rule_is_the_dense_condition(switch):
    """``o3.takes_packed`` on ``dense._slot_desc``'s one-slot descriptor (forward and grad-x
    strides) against the condition ``dense`` used to spell out, over aligned and misaligned
    operands."""
    for k, n_out, extra in itertools.product((32, 96, 128, 160, 320, 352), (32, 40, 64), (0, 2)):
        x_row = k + extra
        for x_at, y_at, res_at in ((64, 128, None), (64, 128, 256), (68, 128, None), (64, 136, None),
                                   (64, 128, 264)):
            want = bool(switch and k % 32 == 0 and o3.LIN_X6_MINK <= k <= 320 and n_out % 32 == 0
                        and x_row % 4 == 0 and x_at % 16 == 0 and y_at % 16 == 0
                        and (res_at is None or res_at % 16 == 0))
            for bias, (ldk, ldj) in itertools.product((False, True), ((1, k), (k, 1))):
                desc = dense._slot_desc(n_out, k, 0, ldk, ldj, bias, 33)
                assert o3.takes_packed(desc, switch, x_row, n_out, x_at, y_at, res_at) is want, \
                    (k, n_out, x_row, x_at, y_at, res_at, bias)


def test_packed_rule_reads_the_k_threshold_at_call_time(monkeypatch):
    desc = dense._slot_desc(32, 32, 0, 1, 32, False, 33)
    assert not o3.takes_packed(desc, True, 32, 32, 0, 0)
    monkeypatch.setattr(o3, "LIN_X6_MINK", 0)
    assert o3.takes_packed(desc, True, 32, 32, 0, 0)


@pytest.mark.parametrize("n,tiles", [(1, 1), (33, 4), (4097, 8), (32768, 625), (10 ** 6, 1)])
def test_grad_w_slice_plan_is_the_formula(n, tiles):
    slices = max(1, min((n + 31) // 32, -(-o3.LINW_WG // tiles), o3.LINW_MAX_SLICES))
    nps = -(-n // slices)
    slices = -(-n // nps)
    assert o3.linw_slices(n, tiles) == (slices, nps)
    assert slices * nps >= n > (slices - 1) * nps
