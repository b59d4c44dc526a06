"""tests/prodigy_ref.py against things that are not itself: a two-step example computed by hand, Adam without bias correction, the
scale invariance of the rule, the monotonicity of d -- and the checker against an fp32 emulation of the device's operation order with
one fault planted at a time: it must pass the emulation as it is and catch every fault."""
import math

import numpy as np
import pytest

from tests import prodigy_ref as ref

B1, B2, EPS = 0.9, 0.999, 1e-8


def test_two_steps_of_a_scalar_by_hand():
    """x0 = 1, gradients 2 then 1, lr = 4, d0 = 1/4, b1 = 1/2, b2 = 3/4, eps = 0, no decay.
    step 0: d = 1/4, step = lr d = 1, c = step d / d0 = 1.  d g = 1/2: m = 1/4, v = 1/4 * 1/4 = 1/16, s = 2.  x = x0, so the dot product
            is 0: num = 0, den = 2, d_hat = 0 and d stays d0.  x = 1 - 1 * (1/4) / (1/4) = 0.
    step 1: d g = 1/4: m = 1/8 + 1/8 = 1/4, v = 3/64 + 1/64 = 1/16, s = 2 beta3 + 1.  dot = c g (x0 - x) = 1, num = 1,
            den = 2 beta3 + 1, d_hat = 1 / (2 sqrt(3/4) + 1) = 0.366... > 1/4, so d = d_hat.  x = 0 - 1 = -1."""
    beta3 = math.sqrt(0.75)
    opt = ref.Prodigy64([np.array([1.0])], lr=4.0, betas=(0.5, 0.75), eps=0.0, d0=0.25)
    opt.step([np.array([2.0])])
    assert (opt.m[0][0], opt.v[0][0], opt.s[0][0], opt.p[0][0]) == (0.25, 0.0625, 2.0, 0.0)
    assert (opt.num, opt.den, opt.d_hat, opt.d) == (0.0, 2.0, 0.0, 0.25)
    opt.step([np.array([1.0])])
    assert (opt.m[0][0], opt.v[0][0], opt.p[0][0]) == (0.25, 0.0625, -1.0)
    assert opt.s[0][0] == pytest.approx(2 * beta3 + 1, rel=1e-15) and opt.num == 1.0 and opt.den == pytest.approx(2 * beta3 + 1, rel=1e-15)
    assert opt.d == pytest.approx(1.0 / (2 * beta3 + 1), rel=1e-15) and opt.d == opt.d_hat == opt.d_max and 0.366 < opt.d < 0.3661
    # the same two steps through the checker's own element rule and finalize rule
    K = ref.consts(d=0.25, d0=0.25, b1=0.5, b2=0.75, eps=0.0)
    one = lambda x: np.array([x], dtype=np.float32)
    r = ref.range64(dict(p=one(0.0), g=one(1.0), m=one(0.25), v=one(0.0625), s=one(2.0), x0=one(1.0), lr=4.0, wd=0.0), K)
    assert (r["m"][0], r["v"][0], r["p"][0], r["dot"][0]) == (0.25, 0.0625, -1.0, 1.0) and r["l1"][0] == pytest.approx(2 * beta3 + 1, rel=1e-7)
    blk = ref.finalize64({"d": 0.25, "d_max": 0.25, "d_hat": 0.0, "num": 0.0, "den": 2.0}, 1.0, 2 * beta3 + 1, K)
    assert blk["d"] == pytest.approx(opt.d, rel=1e-15) and blk["num"] == 1.0


def test_a_frozen_d_is_adam_without_bias_correction():
    """d0 = 1 and growth = 1: d stays 1, c = step, and p, m, v follow the few-line recurrence at rate lr"""
    rng = np.random.default_rng(0)
    p0, lr, wd = rng.standard_normal(7), 3e-3, 1e-2
    opt = ref.Prodigy64([p0], lr=lr, betas=(B1, B2), eps=EPS, weight_decay=wd, d0=1.0, growth=1.0)
    p, m, v = p0.copy(), np.zeros(7), np.zeros(7)
    for _ in range(5):
        g = rng.standard_normal(7)
        opt.step([g])
        gr = g + wd * p
        m = B1 * m + (1 - B1) * gr
        v = B2 * v + (1 - B2) * gr * gr
        p = p - lr * m / (np.sqrt(v) + EPS)
        assert opt.d == 1.0
        np.testing.assert_allclose(opt.p[0], p, rtol=1e-14, atol=0)
        np.testing.assert_allclose(opt.m[0], m, rtol=1e-14, atol=0)
        np.testing.assert_allclose(opt.v[0], v, rtol=1e-14, atol=0)


def test_with_eps_zero_the_scale_of_the_gradients_does_not_matter():
    rng = np.random.default_rng(1)
    p0 = rng.standard_normal(9)
    base = rng.standard_normal(9)
    gs = [base + 0.3 * rng.standard_normal(9) for _ in range(8)]
    a = ref.Prodigy64([p0], lr=1.0, betas=(B1, B2), eps=0.0)
    b = ref.Prodigy64([p0], lr=1.0, betas=(B1, B2), eps=0.0)
    for g in gs:
        a.step([g])
        b.step([1024.0 * g])
    assert a.d > a.d0
    assert b.d == pytest.approx(a.d, rel=1e-12)
    np.testing.assert_allclose(b.p[0], a.p[0], rtol=1e-11, atol=1e-300)


def least_squares(seed=2, rows=48, cols=12, noise=0.05):
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((rows, cols))
    b = A @ rng.standard_normal(cols) + noise * rng.standard_normal(rows)
    return A, b, rng


def test_d_never_falls_on_a_noisy_least_squares_problem():
    A, b, rng = least_squares()
    opt = ref.Prodigy64([np.zeros(A.shape[1])], lr=1.0, betas=(B1, B2), eps=EPS)
    loss0, ds = 0.5 * float(np.mean((A @ opt.p[0] - b) ** 2)), [opt.d]
    for _ in range(300):
        rows = rng.integers(0, A.shape[0], 8)                # a noisy gradient: a mini-batch of the rows
        g = A[rows].T @ (A[rows] @ opt.p[0] - b[rows]) / 8
        opt.step([g])
        ds.append(opt.d)
    assert all(y >= x for x, y in zip(ds, ds[1:])) and ds[-1] > 1e3 * ds[0]
    assert 0.5 * float(np.mean((A @ opt.p[0] - b) ** 2)) < 0.1 * loss0


# ---------------------------------------------------------------------------------------------------------------------
SIZES = (5, 1025, 2049)                                      # a tail only, two blocks, three blocks
D0 = ref.f32(1e-3)                                           # the block holds fp32 values


def fresh(rng):
    ranges = []
    for i, n in enumerate(SIZES):
        p = rng.standard_normal(n).astype(np.float32)
        z = np.zeros(n, dtype=np.float32)
        ranges.append(dict(p=p, g=z, m=z.copy(), v=z.copy(), s=z.copy(), x0=p.copy(), e=p.copy(), lr=1.0 if i else 0.5, wd=1e-2))
    return {"ranges": ranges, "block": {"d": D0, "d_max": D0, "d_hat": 0.0, "num": 0.0, "den": 0.0, "d_prev": D0}}


def with_grads(state, rng, base):
    for r, b in zip(state["ranges"], base):
        r["g"] = (b + 0.3 * rng.standard_normal(b.size)).astype(np.float32)
    return state


def advance(state, K, mutate=None):
    after = ref.emulate_step(state, K, mutate)
    nxt = {"ranges": [dict(r) for r in after["ranges"]], "block": dict(after["block"], d_prev=state["block"]["d"])}
    return after, nxt


@pytest.mark.parametrize("decoupled,safeguard,growth,ema", [(False, False, None, None), (True, True, 2.0, 0.9)])
def test_the_checker_passes_the_emulation_and_catches_every_planted_fault(decoupled, safeguard, growth, ema):
    rng = np.random.default_rng(3)
    state = fresh(rng)
    base = [rng.standard_normal(n) for n in SIZES]
    kw = dict(d0=D0, b1=B1, b2=B2, eps=EPS, gscale=0.5, lr_factor=0.75, decoupled=decoupled, safeguard=safeguard, growth=growth, ema_decay=ema)
    seen = []
    for k in range(6):
        with_grads(state, rng, base)
        K = ref.consts(d=state["block"]["d"], **kw)
        after, nxt = advance(state, K)
        used = ref.check_step(state, after, K)
        assert all(0.0 <= v <= 1.0 for v in used.values()), used
        risen = state["block"]["d"] > state["block"]["d_prev"]
        for fault in ("drop_block_sum", "p_after", "no_beta3", "stale_d"):
            if (fault == "stale_d" and not risen) or (fault == "no_beta3" and state["block"]["num"] == 0.0):
                continue                                      # the fault changes nothing at this step
            bad, _ = advance(state, K, fault)
            with pytest.raises(AssertionError):
                ref.check_step(state, bad, K)
            seen.append(fault)
        Ks = ref.consts(d=state["block"]["d"], skip=True, **kw)
        held, _ = advance(state, Ks)
        assert ref.check_step(state, held, Ks) == {}
        bad, _ = advance(state, Ks, "s_on_skip")
        with pytest.raises(AssertionError):
            ref.check_step(state, bad, Ks)
        state = nxt
    assert state["block"]["d"] > 2 * D0                    # d did rise, so "stale_d" was a fault at some step
    assert {"drop_block_sum", "p_after", "no_beta3", "stale_d"} <= set(seen)


def test_the_underflow_rule_drops_the_adam_term():
    """d g so small that (d g)^2 is 0 in fp32, and eps = 0: the denominator is 0 and p keeps its value, in the emulation and in the
    reference; m, s and the sums advance"""
    K = ref.consts(d=1e-6, d0=1e-6, b1=B1, b2=B2, eps=0.0)
    one = lambda x: np.array([x, x], dtype=np.float32)
    state = {"ranges": [dict(p=one(1.0), g=one(1e-30), m=one(0.0), v=one(0.0), s=one(0.0), x0=one(1.0), lr=1.0, wd=0.0)],
             "block": {"d": K.d, "d_max": K.d, "d_hat": 0.0, "num": 0.0, "den": 0.0}}
    after = ref.emulate_step(state, K)
    assert after["ranges"][0]["v"][0] == 0.0 and after["ranges"][0]["m"][0] != 0.0 and after["ranges"][0]["p"][0] == 1.0
    r = ref.range64(state["ranges"][0], K)
    assert r["p"][0] == 1.0 and r["s"][0] > 0.0
