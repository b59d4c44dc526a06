"""The reference of the expert capacity (tests/capacity_ref.py) against hand-worked cases, and the committed input families against planted
faults: every fault of R.FAULTS must change the keep mask on at least one (family, shape, capacity, policy) the GPU tests use -- a fault no
input exposes means the inputs are too weak, and the test says so.  No GPU."""
from fractions import Fraction

import numpy as np
import pytest

from tests import capacity_ref as R

F32 = np.float32


def test_capacity_in_rationals():
    assert R.capacity(1.25, 2, 7, 4) == 5                 # 1.25 * 2 * 7 / 4 = 4.375
    assert R.capacity(Fraction(5, 4), 2, 7, 4) == 5
    assert R.capacity(1, 2, 8, 4) == 4 and R.capacity(1.0, 1, 9, 4) == 3
    assert R.capacity(0.001, 1, 7, 4) == 1 and R.capacity(100, 1, 7, 4) == 7      # the floors at 1 and S
    assert R.capacity(Fraction(1, 3), 3, 1 << 40, 1 << 3) == 1 << 37              # exact where a float product would round


def test_selection_by_hand():
    p = np.array([[0.5, 0.3, 0.2], [0.2, 0.2, 0.6], [0.25, 0.5, 0.25]], F32)
    assert R.select_mask(p, 1).tolist() == [[True, False, False], [False, False, True], [False, True, False]]
    assert R.select_mask(p, 2).tolist() == [[True, True, False], [True, False, True], [True, True, False]]      # equal scores: expert order
    b = np.array([0.0, 0.0, 0.35], F32)
    assert R.select_mask(p, 1, b).tolist() == [[False, False, True], [False, False, True], [False, False, True]]


def test_order_policy_by_hand():
    # k = 1, expert 0 selected by the frames 0, 1, 3, 4; expert 1 by 2, 5
    p = np.array([[0.6, 0.4], [0.9, 0.1], [0.2, 0.8], [0.7, 0.3], [0.8, 0.2], [0.1, 0.9]], F32)
    r = R.reference(p, 1, 2, R.ORDER)
    assert r["demand"].tolist() == [4, 2] and r["kept_count"].tolist() == [2, 2]
    assert np.nonzero(r["keep"][:, 0])[0].tolist() == [0, 1] and np.nonzero(r["keep"][:, 1])[0].tolist() == [2, 5]
    assert r["last"].tolist() == [1, 5] and np.isneginf(r["thr"]).all()
    assert r["cap_scale"][:, 0].tolist() == [1, 1, 0, 0, 0, 0]
    r = R.reference(p, 1, 4, R.ORDER)
    assert np.array_equal(r["keep"], r["m"]) and r["last"].tolist() == [5, 5]


def test_priority_policy_by_hand():
    p = np.array([[0.6, 0.4], [0.9, 0.1], [0.2, 0.8], [0.7, 0.3], [0.8, 0.2], [0.1, 0.9]], F32)
    r = R.reference(p, 1, 2, R.PRIORITY)
    assert np.nonzero(r["keep"][:, 0])[0].tolist() == [1, 4]                     # 0.9 and 0.8
    assert r["thr"][0] == F32(0.8) and r["last"][0] == 4 and np.isneginf(r["thr"][1]) and r["last"][1] == 5
    # ties at the threshold in frame order: the frames 0, 1, 2, 3 hold 0.7, budget 2 -> frames 0, 1; L = 1
    q = np.array([[0.7, 0.3]] * 4 + [[0.9, 0.1]], F32)
    r = R.reference(q, 1, 3, R.PRIORITY)
    assert np.nonzero(r["keep"][:, 0])[0].tolist() == [0, 1, 4] and r["thr"][0] == F32(0.7) and r["last"][0] == 1
    # k = 2: the priority is per pair -- expert 1 is every frame's second choice and ranks the frames on p[s, 1] alone
    t = np.array([[0.5, 0.3, 0.2], [0.6, 0.35, 0.05], [0.55, 0.25, 0.2]], F32)
    r = R.reference(t, 2, 1, R.PRIORITY)
    assert r["keep"].tolist() == [[False, False, False], [True, True, False], [False, False, False]]
    # a multiplier enters cap_scale, not the ranking; a frame that lost every pair has a zero row
    mix = np.array([[2.0, 0.0, 1.0]] * 3, F32)
    r = R.reference(t, 2, 1, R.PRIORITY, mix=mix)
    assert r["cap_scale"].tolist() == [[0, 0, 0], [2.0, 0.0, 0], [0, 0, 0]]
    w = R.dropped_weights(np.where(r["m"], t, 0).astype(F32), r["m"], r["keep"])
    assert w.tolist() == [[0, 0, 0], [F32(0.6), F32(0.35), 0], [0, 0, 0]] and not np.signbit(w).any()


def test_unselected_frames_do_not_count_against_the_budget():
    # expert 0 has the largest column value in frame 0, which did not select it (the bias moved frame 0 to expert 1)
    p = np.array([[0.55, 0.45], [0.5, 0.1], [0.45, 0.2]], F32)
    b = np.array([0.0, 0.2], F32)
    m = R.select_mask(p, 1, b)
    assert m[:, 0].tolist() == [False, True, True]
    r = R.reference(p, 1, 1, R.PRIORITY, b=b)
    assert r["keep"][:, 0].tolist() == [False, True, False] and r["keep"][:, 1].tolist() == [True, False, False]
    assert r["thr"][0] == F32(0.5) and r["last"][0] == 1


CASES = [(S, E, k) for S in (2, 65, 257) for E in (2, 4, 16) for k in (1, 2) if k < E]


def _inputs():
    """every (family, S, E, k, bias, p, m, c, policy) the fault check looks at: the sub-op test's families at three of its sizes"""
    for name in R.FAMILIES:
        for S, E, k in CASES:
            p = R.family(name, S, E)
            for b in (None, R.bias_for(E)):
                m = R.select_mask(p, k, b)
                for c in R.capacities(m):
                    for policy in (R.ORDER, R.PRIORITY):
                        yield name, S, E, k, b, p, m, c, policy


@pytest.mark.parametrize("fault", R.FAULTS)
def test_every_planted_fault_is_exposed_by_a_committed_input(fault):
    exposed = set()
    for name, S, E, k, b, p, m, c, policy in _inputs():
        if fault == "capacity_off_by_one" and c == S:
            continue
        if not np.array_equal(R.keep_mask(p, m, c, policy, b=b, fault=fault), R.keep_mask(p, m, c, policy)):
            exposed.add(name)
    assert exposed, f"no committed input exposes the planted fault `{fault}`: the input families are too weak"
    print(fault, "exposed by", sorted(exposed))


def test_the_families_show_drops_slack_and_threshold_ties():
    """Each family but `balanced` drops a pair and leaves an expert within its budget in one and the same case; `balanced` drops nothing at
    its own max demand; `tie_at_c` has equal values at the ranks c and c + 1; `underflow` selects exact zeros."""
    for name in R.FAMILIES:
        both = tie = zero_sel = False
        for S, E, k in CASES:
            p = R.family(name, S, E)
            m = R.select_mask(p, k)
            zero_sel |= bool((p[m] == 0).any())
            for c in R.capacities(m):
                r = R.reference(p, k, c, R.PRIORITY)
                d, s = R.drops_and_slack(r, c)
                both |= d and s
                tie |= d and R.has_threshold_tie(p, m, c)
                if c >= m.sum(0).max():
                    assert not d, (name, S, E, k, c)
        assert both or name == "balanced", f"{name}: no case with a dropped pair and an expert within its budget"
        assert tie or name != "tie_at_c", "tie_at_c: no column with equal values at the ranks c and c + 1"
        assert zero_sel or name != "underflow", "underflow: no selected probability is exactly 0"
    S, E = 64, 4
    m = R.select_mask(R.family("balanced", S, E), 2)
    assert m.sum(0).tolist() == [32] * 4
