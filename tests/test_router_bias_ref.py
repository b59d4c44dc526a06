"""The reference of aux-loss-free expert balancing (tests/router_bias_ref.py) checked against itself, without a GPU: each planted fault --
the bias in the weights, a flipped update sign, counts not cleared, tot == 0 rows moved, columns >= E touched, the selection taken from a
later bias -- makes the check that guards it fail; and the fixtures of the GPU tests do what those tests need, on the oracle's router: the
bias draw changes the selection in over a quarter of the frames and leaves some, the tie is exact and decided by expert order, and the
reference recurrence alone narrows the load spread of the skewed site."""
import numpy as np
import pytest
import torch

from tests import router_bias_ref as R
from tests.topk_ref import topk_mask


def _probs(S=40, E=4, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.softmax(torch.randn(S, E, generator=g), dim=-1), 0.3 * torch.randn(E, generator=g)


@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("renorm", [True, False])
def test_reference_weights_pass_and_biased_weights_fail(k, renorm):
    p, b = _probs()
    assert bool(R.changed_frames(p, b, k).any())
    R.check_weights(R.weights(p, b, k, renorm), p, b, k, renorm)
    m = R.select_mask(p, b, k)
    w = m * (p + b)                                       # fault: the bias added to the weights as well as the selection
    w = w / w.sum(-1, keepdim=True) if renorm else w
    if not (k == 1 and renorm):                           # (k = 1 renormalised: the one kept weight is 1 whatever it was formed from)
        with pytest.raises(AssertionError):
            R.check_weights(w, p, b, k, renorm)
    with pytest.raises(AssertionError):                   # fault: no bias at all
        R.check_weights(R.weights(p, torch.zeros_like(b), k, renorm), p, b, k, renorm)


@pytest.mark.parametrize("k", [1, 2])
def test_selection_from_a_later_bias_fails(k):
    p, b = _probs(seed=1)
    later = b + 0.2 * torch.randn(b.shape, generator=torch.Generator().manual_seed(2))
    assert not torch.equal(R.select_mask(p, b, k), R.select_mask(p, later, k))
    with pytest.raises(AssertionError):
        R.check_weights(R.weights(p, later, k, False), p, b, k, False)


def _tables(n=3, seed=0):
    rng = np.random.default_rng(seed)
    E = [4, 2, 16][:n]
    bias = np.full((n, R.ROW), np.nan, np.float32)
    counts = np.full((n, R.ROW), np.nan, np.float32)
    for i, e in enumerate(E):
        bias[i, :e] = rng.standard_normal(e).astype(np.float32) * 0.01
        counts[i, :e] = rng.integers(0, 50, e).astype(np.float32)
    counts[1, :2] = 0.0                                   # a tot == 0 row
    return bias, counts, E


def test_update_rule():
    bias, counts, E = _tables()
    b1, c1 = R.update(bias, counts, E, 1e-3)
    R.check_update(bias, counts, E, 1e-3, b1, c1)
    e = E[0]
    mean = counts[0, :e].sum() / e
    for f in range(e):                                    # overloaded experts go down, underloaded ones up, by exactly one fp32 addition
        step = np.float32(-1e-3) if counts[0, f] > mean else (np.float32(1e-3) if counts[0, f] < mean else np.float32(0))
        assert b1[0, f] == np.float32(bias[0, f] + step)
    assert np.array_equal(b1[1].view(np.uint32), bias[1].view(np.uint32)) and np.all(c1[1, :2] == 0)
    assert np.all(c1[0, :e] == 0) and np.all(np.isnan(b1[0, e:])) and np.all(np.isnan(c1[0, e:]))
    b0, c0 = R.update(bias, counts, E, 0.0)               # rate 0: the bias keeps its values, the counts are still consumed
    assert np.array_equal(b0[0, :e], bias[0, :e]) and np.all(c0[0, :e] == 0)
    bt, _ = R.update(np.zeros((1, R.ROW), np.float32), np.array([[3, 3, 1, 5] + [0] * 12], np.float32), [4], 0.5)
    assert list(bt[0, :4]) == [0.0, 0.0, 0.5, -0.5]       # a two-way tie at the mean: sign(0) = 0


def _faulty_update(fault):
    def run(bias, counts, E, rate):
        b, c = R.update(bias, counts, E, rate)
        if fault == "sign":
            b0 = np.array(bias, np.float32)
            for i, e in enumerate(E):
                b[i, :e] = b0[i, :e] - (b[i, :e] - b0[i, :e])
        elif fault == "not_cleared":
            c = np.array(counts, np.float32)
        elif fault == "empty_row_moved":
            for i, e in enumerate(E):
                if np.array(counts, np.float32)[i, :e].sum() == 0:
                    b[i, :e] += np.float32(rate)
        elif fault == "columns_past_E":
            for i, e in enumerate(E):
                c[i, e:] = 0.0
        return b, c
    return run


@pytest.mark.parametrize("fault", ["sign", "not_cleared", "empty_row_moved", "columns_past_E"])
def test_planted_update_faults_fail(fault):
    bias, counts, E = _tables()
    b1, c1 = _faulty_update(fault)(bias, counts, E, 1e-3)
    with pytest.raises(AssertionError):
        R.check_update(bias, counts, E, 1e-3, b1, c1)


@pytest.mark.parametrize("which", ["tile_fast", "e16"])
@pytest.mark.parametrize("k", [1, 2])
def test_selection_fixture_on_the_oracle_router(which, k):
    """What tests/test_router_bias_gpu.py asserts on the library's own softmax, shown here for the oracle's: the draw is worth testing."""
    cfg, S, P, B, X, Y, noise, b0 = R.selection_case(which)
    p = R.router_probs(P, X, Y, noise)
    b, a, c = R.with_tie(p, b0, k)
    sc = p[0] + b
    assert float(sc[a]) == float(sc[c]) and a != c
    kept = R.select_mask(p, b, k)[0]
    assert kept[min(a, c)] == 1 and kept[max(a, c)] == 0, "equal scores: the expert with the smaller index is kept"
    ch = R.changed_frames(p, b, k)
    assert 4 * int(ch.sum()) >= S and int((~ch).sum()) >= 1, (int(ch.sum()), S)


def test_trajectory_fixture_narrows_the_spread_on_the_oracle_router():
    cfg, S, P, B, X, Y, noise = R.trajectory_case()
    p = R.router_probs(P, X, Y, noise)
    after, loads = R.trajectory([p] * R.TRAJ_ROUNDS, cfg.E, R.TRAJ_K, R.TRAJ_RATE)
    assert R.spread(loads[-1]) < R.spread(loads[0])
    assert int(np.argmax(loads[0])) == 0 and after[-1][0] < 0          # the skewed expert is the overloaded one and is pushed down
    m0 = topk_mask(p, R.TRAJ_K)
    assert np.array_equal(loads[0], (R.counts_of(m0) / (S * R.TRAJ_K)).double().numpy())      # round 1 selects with a zero bias
