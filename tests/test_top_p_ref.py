"""Self-checks of the top-p reference (tests/top_p_ref.py), no GPU: the properties of the rule on every input family, the exact
threshold cases, k_min = k_max = k against tests/topk_ref.py, the reports' sums, the sweep family reaching every prefix length, and every
planted fault caught by the checker the GPU tests call, on the GPU tests' own inputs."""
import numpy as np
import pytest
import torch

from tests import top_p_ref as R
from tests.topk_ref import topk_mask, topk_weights

SHAPES = [(S, E) for S in (63, 257, 300) for E in (2, 3, 4, 16)]


@pytest.mark.parametrize("S,E", SHAPES)
def test_properties_on_every_family(S, E):
    for name in R.FAMILIES:
        p = R.family(name, S, E)
        assert p.shape == (S, E) and p.dtype == np.float32 and np.all(p >= 0)
        for P in R.THRESHOLDS:
            for k_min, k_max in R.k_ranges(E):
                what = f"{name} S={S} E={E} P={P} k=[{k_min}, {k_max}]"
                ref = R.emulate(p, P, k_min, k_max, 1)
                m = ref["mask"]
                try:
                    R.check_properties(p, P, k_min, k_max, m)
                except AssertionError as err:
                    raise AssertionError(f"{what}: {err}") from err
                assert int(ref["khist"].sum()) == S, what
                assert int(ref["count"].sum()) == int((np.arange(E + 1) * ref["khist"]).sum()), what
                assert np.array_equal(R.mask_of_bits(ref["choice"], E), m), what
                assert np.abs(ref["w"].sum(1, dtype=np.float64) - 1).max() <= (E + 1) * 2.0 ** -24, what + ": renormalised weights do not sum to 1"
                assert np.abs(R.load_of(m).sum(dtype=np.float64) - 1) <= E * 2.0 ** -24, what


def test_threshold_ties_are_decided_by_the_fp32_comparison():
    """[.5, .25, .25]: the prefix masses are .5, .75, 1 exactly.  P = .5 takes one expert (c_1 >= P), the fp32 number above .5 two,
    P = .75 two, the number above .75 three; equal probabilities enter in expert order."""
    p = np.array([[.5, .25, .25], [.25, .5, .25], [.25, .25, .5]], np.float32)
    up = lambda x: float(np.nextafter(np.float32(x), np.float32(2)))
    assert R.k_of(p, .5).tolist() == [1, 1, 1]
    assert R.k_of(p, up(.5)).tolist() == [2, 2, 2]
    assert R.k_of(p, .75).tolist() == [2, 2, 2]
    assert R.k_of(p, up(.75)).tolist() == [3, 3, 3]
    assert R.k_of(p, 1.0).tolist() == [3, 3, 3]
    assert R.bits_of(R.select_mask(p, .75)).tolist() == [0b011, 0b011, 0b101]      # the first of the two .25 comes in
    assert R.k_of(p, up(.5), k_max=1).tolist() == [1, 1, 1] and R.k_of(p, .5, k_min=2).tolist() == [2, 2, 2]
    assert R.k_of(np.full((1, 4), .25, np.float32), 1e-30).tolist() == [1]
    short = np.full((1, 3), np.float32(1) / np.float32(3), np.float32)             # an fp32 row that may not reach 1: k* = E either way
    assert R.k_of(short, 1.0).tolist() == [3]
    fam = R.family("threshold_tie", 12, 4)
    assert set(R.k_of(fam, .5).tolist()) == {1} and set(R.k_of(fam, up(.5)).tolist()) == {2} and set(R.k_of(fam, .75).tolist()) == {2}


@pytest.mark.parametrize("S,E", SHAPES)
def test_fixed_k_is_plain_topk(S, E):
    """k_min = k_max = k: the mask of tests/topk_ref.py, whatever P says, and its weights"""
    for name in R.FAMILIES:
        p = R.family(name, S, E)
        pt = torch.from_numpy(p)
        for k in sorted({1, 2, E - 1, E}):
            if not 1 <= k <= E:
                continue
            want = topk_mask(pt, k).numpy().astype(bool)
            for P in (1e-30, 0.75, 1.0):
                assert np.array_equal(R.select_mask(p, P, k, k), want), (name, k, P)
            if k < E:
                w = topk_weights(pt, k, True).numpy()
                got = R.weights(p, want, 1)
                assert np.abs(got - w).max() <= 4 * 2.0 ** -24, (name, k)


@pytest.mark.parametrize("S", [63, 257, 300])
@pytest.mark.parametrize("E", [2, 3, 4, 16])
def test_the_sweep_family_reaches_every_prefix_length(S, E):
    """at P = 0.95 frames with every k in 1 .. E occur: a comparison on this family covers every prefix length"""
    kh = R.khist_of(R.select_mask(R.family("sweep", S, E), 0.95))
    assert kh[0] == 0 and np.all(kh[1:] > 0), kh


@pytest.mark.parametrize("fault", R.FAULTS)
def test_planted_faults_are_caught(fault):
    caught = 0
    for S, E in ((63, 3), (257, 4), (300, 16)):
        mix = R.mix_for(S, E)
        for name in R.FAMILIES:
            p = R.family(name, S, E)
            for P in R.THRESHOLDS:
                for k_min, k_max in R.k_ranges(E):
                    bad = R.emulate(p, P, k_min, k_max, 1, mix, fault=fault)
                    good = R.emulate(p, P, k_min, k_max, 1, mix)
                    R.check_selection(p, P, k_min, k_max, 1, mix, good["choice"], good["count"], good["khist"], good["w"])
                    try:
                        R.check_selection(p, P, k_min, k_max, 1, mix, bad["choice"], bad["count"], bad["khist"], bad["w"])
                    except AssertionError:
                        caught += 1
    assert caught > 0, f"the checker does not see the fault `{fault}` on any input"
