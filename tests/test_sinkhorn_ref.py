"""The reference of Sinkhorn-balanced top-k routing (tests/sinkhorn_ref.py) checked against itself, without a GPU: the selection against
torch.topk on tie-free rows, the fp32 emulation of the rounds within the GPU tests' bound on v, each planted fault caught by the same
comparison and bound the GPU tests use, on their own inputs, and the property the method exists for: the largest expert share falls."""
import numpy as np
import pytest
import torch

from tests import sinkhorn_ref as R

# (S, E, k, n) of the fault checks: n <= 4 -- at n = 8 the iteration has converged and a round fewer moves log v by under 5e-6
CASES = [(320, 4, 1, 3), (77, 3, 1, 2), (640, 16, 2, 4)]


@pytest.mark.parametrize("S,E,k,n", CASES)
def test_fp32_emulation_stays_within_the_bound_and_the_faultless_emulation_passes(S, E, k, n):
    p = R.family("skewed", S, E)
    ref = R.scale_fp64(p, n)
    err32 = R.log_error(R.scale_fp32(p, n), ref)
    print(f"(S, E, n) = ({S}, {E}, {n}): fp32 emulation {err32:.2e} from fp64, bound {R.v_bound(S, E, n):.2e}")
    assert err32 <= 4e-6 and err32 <= R.v_bound(S, E, n)
    for renorm in (0, 1):
        got = R.emulate(p, k, n, renorm, R.mix_for(S, E))
        R.check_scale(p, n, got["v"], ref)
        R.check_selection(p, got["v"], k, renorm, R.mix_for(S, E), got["choice"], got["count"], got["w"])


@pytest.mark.parametrize("fault", R.SCALE_FAULTS)
@pytest.mark.parametrize("S,E,k,n", CASES)
def test_planted_faults_in_the_rounds_exceed_the_bound_on_v(S, E, k, n, fault):
    p = R.family("skewed", S, E)
    ref = R.scale_fp64(p, n)
    bad = R.scale_fp64(p, n, fault)
    moved = float(np.abs(np.log(bad / ref)).max())
    print(f"(S, E, n) = ({S}, {E}, {n}) {fault}: log v moves by {moved:.2e}, bound {R.v_bound(S, E, n):.2e}")
    with pytest.raises(AssertionError):
        R.check_scale(p, n, bad.astype(np.float32), ref)


@pytest.mark.parametrize("fault", R.SELECT_FAULTS)
def test_planted_faults_in_the_selection_fail_the_checker(fault):
    S, E, k, n = CASES[0] if fault != "tie_reversed" else (320, 4, 2, 3)
    p = R.family("uniform" if fault == "tie_reversed" else "skewed", S, E)
    mix = R.mix_for(S, E)
    for renorm in (0, 1):
        good = R.emulate(p, k, n, renorm, mix)
        R.check_selection(p, good["v"], k, renorm, mix, good["choice"], good["count"], good["w"])
    bad = R.emulate(p, k, n, 1, mix, fault=fault)
    with pytest.raises(AssertionError):
        R.check_selection(p, bad["v"], k, 1, mix, bad["choice"], bad["count"], bad["w"])
    if fault == "kept_from_q":                            # ... and at k = 2, where only the 1e-6 comparison of the weights can see it
        p = R.family("skewed", 640, 16)
        bad = R.emulate(p, 2, 4, 1, None, fault=fault)
        with pytest.raises(AssertionError):
            R.check_selection(p, bad["v"], 2, 1, None, w=bad["w"])


@pytest.mark.parametrize("name", R.FAMILIES)
def test_selection_rules_on_every_family(name):
    for S, E in ((1, 2), (63, 3), (65, 4), (257, 16)):
        p = R.family(name, S, E)
        for n in (1, 3):
            v64 = R.scale_fp64(p, n)
            assert np.all(np.isfinite(v64)) and np.all(v64 > 0) and np.all(v64 <= R.FLT_MAX)
            v = v64.astype(np.float32)
            for k in sorted({1, E - 1}):
                m = R.select_mask(p, v, k)
                assert np.array_equal(m.sum(1), np.full(S, k))
                assert np.array_equal(R.mask_of_bits(R.bits_of(m), E), m)
                if name == "uniform":
                    assert m[:, :k].all(), "all ties: the first k experts"
                if name == "zero_column" and k < E - 1:
                    assert not m[:, E // 2].any(), "0 * v = 0 keeps a column of zeros last"
                if name == "skewed":                      # (no ties in q on this input: torch.topk names the same experts)
                    q = torch.from_numpy((p * v[None, :]).astype(np.float32))
                    want = np.zeros((S, E), bool)
                    want[np.arange(S)[:, None], torch.topk(q, k, dim=1).indices.numpy()] = True
                    assert np.array_equal(m, want)
                w = R.weights(p, m, 1)
                assert np.allclose(w.sum(1), 1.0, atol=1e-6)


def test_balancing_lowers_the_largest_expert_share():
    S, E, k, n = CASES[0]
    p = R.family("skewed", S, E)
    plain = R.largest_share(R.select_mask(p, np.ones(E, np.float32), k))
    balanced = R.largest_share(R.select_mask(p, R.scale_fp64(p, n).astype(np.float32), k))
    print(f"(S, E, k, n) = ({S}, {E}, {k}, {n}): largest expert share {plain:.2f} -> {balanced:.2f}")
    assert plain >= 0.45 and balanced <= 0.30, (plain, balanced)


def test_weights_and_kept_rules():
    p = np.array([[0.5, 0.25, 0.25], [0.125, 0.125, 0.75]], np.float32)
    v = np.array([1.0, 4.0, 1.0], np.float32)             # q = [[0.5, 1, 0.25], [0.125, 0.5, 0.75]]
    m = R.select_mask(p, v, 2)
    assert m.tolist() == [[True, True, False], [False, True, True]]
    assert R.kept_of(p, m).tolist() == [0.75, 0.875]      # the UNSCALED p
    assert R.weights(p, m, 0).tolist() == [[0.5, 0.25, 0.0], [0.0, 0.125, 0.75]]
    assert np.allclose(R.weights(p, m, 1), [[2 / 3, 1 / 3, 0], [0, 1 / 7, 6 / 7]], atol=1e-7)
    assert R.select_mask(np.full((1, 3), 0.5, np.float32), np.ones(3, np.float32), 2).tolist() == [[True, True, False]]
