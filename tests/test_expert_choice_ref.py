"""The reference of expert-choice gating (tests/expert_choice_ref.py) checked against itself, without a GPU: the selection against
torch.sort(stable=True), the (T, L) identity, a numpy emulation of the kernels' algorithm (4 x 8-bit radix select on the ordered key, an
ordered tie pass in chunks) that equals the reference on every input family, each planted fault caught by the checker the GPU tests call,
the site reference against tests/topk_ref.py where both apply, and the S = 300 fixture's condition on the oracle's router."""
import numpy as np
import pytest
import torch

from tests import expert_choice_ref as R
from tests import router_bias_ref as RB
from tests.topk_ref import topk_forward

SIZES = [(1, 1), (2, 3), (63, 4), (64, 16), (65, 3), (255, 4), (256, 1), (257, 16), (1023, 3), (1025, 4)]


@pytest.mark.parametrize("name", R.FAMILIES)
def test_reference_selection_is_torch_stable_sort_and_the_two_words_describe_it(name):
    for S, E in SIZES:
        p, extra = R.family(name, S, E)
        for c in sorted(set(R.standard_capacities(S, E) + extra)):
            m = R.choice_mask(p, c)
            order = torch.sort(torch.from_numpy(p), dim=0, descending=True, stable=True).indices[:c]      # (c, E)
            want = np.zeros((S, E), bool)
            want[order.numpy(), np.arange(E)[None, :]] = True
            assert np.array_equal(m, want), (name, S, E, c)
            T, L = R.thr_last(p, c)
            assert np.array_equal(R.mask_from_words(p, T, L), m), (name, S, E, c)
            assert np.array_equal(m.sum(0), np.full(E, c))
            assert np.array_equal(R.mask_of_bits(R.bits_of(m), E), m)


def test_uniform_columns_select_the_first_c_frames():
    p, _ = R.family("uniform", 300, 4)
    m = R.choice_mask(p, 75)
    assert m[:75].all() and not m[75:].any()
    T, L = R.thr_last(p, 75)
    assert np.all(T == np.float32(0.25)) and np.all(L == 74)


@pytest.mark.parametrize("chunk", [256, 64, 1024])
@pytest.mark.parametrize("name", R.FAMILIES)
def test_emulation_of_the_kernels_equals_the_reference(name, chunk):
    for S, E in SIZES:
        p, extra = R.family(name, S, E)
        mix = R.mix_for(S, E)
        for c in sorted(set(R.standard_capacities(S, E) + extra)):
            for renorm in R.RENORMS.get(name, (0, 1)):
                got = R.emulate(p, c, renorm, mix, chunk=chunk)
                R.check_subop(p, c, renorm, mix, **got)


def test_ordered_key_orders_like_the_values():
    v = np.array([-np.inf, -3.5, -1e-40, -0.0, 0.0, 1e-40, 0.25, 1.0, np.inf], np.float32)
    k = R.ordered_key(v).astype(np.int64)
    assert k[3] == k[4] and np.all(np.diff(np.delete(k, 3)) > 0)
    for x in v:
        back = R.unkey(R.ordered_key(np.array([x], np.float32))[0])
        assert back == x


def _fault_input(fault):
    """(p, c, renorm, mix) on which the planted fault shows"""
    if fault in ("tie_high", "ge_for_gt"):
        p, _ = R.family("two_valued", 300, 4)
        return p, 8, 0, None
    if fault == "chunk_reset":                            # the tie group runs over 255 | 256; the wanted tie lies behind the boundary
        p, _ = R.family("two_valued", 300, 4)
        return p, 3 + 260, 0, None
    if fault == "raw_bits":
        p, _ = R.family("signed", 300, 4)
        return p, 75, 0, None
    if fault in ("kept_all", "weight_on_empty"):
        p, _ = R.family("softmax", 300, 4)
        return p, 75, 1, R.mix_for(300, 4)
    p, _ = R.family("softmax", 300, 4)                    # c_plus_one, other_column
    return p, 75, 0, None


@pytest.mark.parametrize("fault", R.FAULTS)
def test_planted_faults_fail_the_checker(fault):
    p, c, renorm, mix = _fault_input(fault)
    R.check_subop(p, c, renorm, mix, **R.emulate(p, c, renorm, mix))          # the faultless emulation passes on this input
    if fault == "weight_on_empty":
        assert R.served_counts(R.choice_mask(p, c))[0] > 0, "no frame without an expert: the fault cannot show"
    with pytest.raises(AssertionError):
        R.check_subop(p, c, renorm, mix, **R.emulate(p, c, renorm, mix, fault=fault))


def test_weights_rules():
    p = np.array([[0.5, 0.5], [0.25, 0.75], [0.125, 0.875]], np.float32)
    m = R.choice_mask(p, 1)                               # expert 0 takes frame 0, expert 1 frame 2: frame 1 has no expert
    assert m.tolist() == [[True, False], [False, False], [False, True]]
    assert R.weights(p, m, 0).tolist() == [[0.5, 0.0], [0.0, 0.0], [0.0, 0.875]]
    assert R.weights(p, m, 1).tolist() == [[1.0, 0.0], [0.0, 0.0], [0.0, 1.0]]
    assert R.weights(p, m, 1, np.full((3, 2), 2.0, np.float32)).tolist() == [[2.0, 0.0], [0.0, 0.0], [0.0, 2.0]]
    assert [R.capacity(k, S, E) for k, S, E in ((1, 300, 4), (2, 3, 4), (0.5, 3, 4), (4, 7, 4), (1, 1, 16), (1.5, 10, 4))] == [75, 2, 1, 7, 1, 4]


def _small_site():
    from oracle import avmoe_oracle as O
    cfg = O.AdapterConfig(Cx=32, Nx=10, Cy=24, Ny=7, E_m=2, E_s=2, reduction=4, groups=2, K=4, variant="avs", lb_loss=True)
    S = 6
    P, B = O.init_params(cfg, seed=3)
    g = torch.Generator().manual_seed(1)
    X, Y = 0.3 * torch.randn(S, cfg.Nx, cfg.Cx, generator=g), 0.3 * torch.randn(S, cfg.Ny, cfg.Cy, generator=g)
    noise = torch.randn(S, cfg.E, generator=g)
    dO, dP = torch.randn(S, cfg.Nx, cfg.Cx, generator=g), torch.randn(S, cfg.E, generator=g)
    return cfg, S, P, B, X, Y, noise, dO, dP


def test_site_reference_agrees_with_the_topk_reference_where_both_apply():
    cfg, S, P, B, X, Y, noise, dO, dP = _small_site()
    p = RB.router_probs(P, X, Y, noise).numpy()
    mask = R.choice_mask(p, 1)                            # four experts take one of six frames each
    assert R.served_counts(mask)[0] >= 2, "no frame without an expert in this draw"
    via_topk = R.site_reference(cfg, P, B, X, Y, dO, dP, 0.5, mask, 0, noise=noise)
    mt = torch.from_numpy(mask).float()
    own = R.ec_grads(cfg, P, B, X, Y, dO, dP, 0.5, mt, 0, noise=noise)
    own["out"] = R.ec_forward(P, B, X, Y, cfg, mt, 0, noise=noise)["out"]
    for kk, v in via_topk.items():
        assert torch.allclose(own[kk], v, rtol=1e-5, atol=1e-6 * float(v.abs().max()) + 1e-12), kk
    # renorm: finite everywhere (no 0 / 0 on the frames no expert took), rows of w sum to 1 or 0, and with every frame served it is the
    # top-k reference's renormalised mixture for the same selection
    ren = R.ec_forward(P, B, X, Y, cfg, mt, 1, noise=noise)
    rows = ren["w"].sum(-1)
    assert bool(torch.isfinite(ren["out"]).all()) and all(abs(float(r) - t) < 1e-6 for r, t in zip(rows, mask.any(1).astype(float)))
    g = R.ec_grads(cfg, P, B, X, Y, dO, dP, 0.5, mt, 1, noise=noise)
    assert all(bool(torch.isfinite(v).all()) for v in g.values())
    full = torch.from_numpy(R.choice_mask(p, S - 1)).float()
    assert bool(full.sum(-1).min() >= 1)
    a = R.ec_forward(P, B, X, Y, cfg, full, 1, noise=noise)["out"]
    b = topk_forward(P, B, X, Y, cfg, 1, True, training=True, noise=noise, update_buffers=False, sel=full)["out"]
    assert torch.allclose(a, b, rtol=1e-5, atol=1e-7)


def test_s300_fixture_leaves_frames_without_and_with_several_experts_on_the_oracle_router():
    cfg, S, P, B, X, Y, noise, c = R.s300_inputs()
    assert (S, c, cfg.E) == (300, 75, 4)
    p = RB.router_probs(P, X, Y, noise).numpy()
    none, many = R.served_counts(R.choice_mask(p, c))
    print(f"S = 300, c = 75: {none} frames without an expert, {many} with two or more")
    assert none * 16 >= S and many * 16 >= S
