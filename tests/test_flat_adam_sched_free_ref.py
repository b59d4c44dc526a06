"""The fp64 reference of schedule-free AdamW (tests/sched_free_ref.py) checked on the host, before a device is asked: against an
independent fp64 spelling of the rule in the in-place-y form the schedulefree package uses (no x is stored there: it is recovered as
(y - (1 - b1) z) / b1), the closed forms of the uniform average, FlatAdam.sf_weights_next against the reference's scalar rule, and the
checker against an fp32 emulation of the kernel with one planted fault per quantity."""
import numpy as np
import pytest

from avmoe_amd.train import FlatAdam, LRSchedule
from tests import sched_free_ref as ref

B1, B2, EPS = 0.9, 0.999, 1e-8


def in_place_y(y0, grad_fn, steps, lr, wd, decoupled, factor, r=0.0, lr_power=2.0):
    """the package's spelling: y and z only, y.lerp_(z, c); y += lr (b1 (1 - c) - 1) q; z -= lr q -> [(y, z, x recovered)] per step"""
    y, z, v = y0.copy(), y0.copy(), np.zeros_like(y0)
    weight_sum, f_max, out = 0.0, 0.0, []
    for k in range(steps):
        f = factor(k)
        f_max = max(f_max, f)
        w = float(k + 1) ** r * f_max ** lr_power
        weight_sum += w
        c = w / weight_sum if weight_sum > 0.0 else 0.0
        g = grad_fn(y, k)
        gr = g if decoupled else g + wd * y
        v = B2 * v + (1.0 - B2) * gr * gr
        q = gr / (np.sqrt(v) / np.sqrt(1.0 - B2 ** (k + 1)) + EPS)
        if decoupled:
            q = q + wd * y
        y = y + c * (z - y)
        y = y + lr * f * (B1 * (1.0 - c) - 1.0) * q
        z = z - lr * f * q
        out.append((y.copy(), z.copy(), (y - (1.0 - B1) * z) / B1))
    return out


@pytest.mark.parametrize("decoupled", [False, True], ids=["coupled", "adamw"])
def test_the_explicit_form_equals_the_in_place_y_form_on_a_noisy_quadratic(decoupled):
    """300 steps of a seeded 50-dimensional quadratic with gradient noise and a 20-step warm-up from factor 0: y, z and the recovered x
    of both spellings agree to 1e-12"""
    rng = np.random.default_rng(11)
    A = rng.standard_normal((50, 50)) / 7.0
    H, target = A.T @ A + 0.1 * np.eye(50), rng.standard_normal(50)
    noise = rng.standard_normal((300, 50))
    grad = lambda y, k: H @ (y - target) + 0.3 * noise[k]
    sched = LRSchedule(warmup_steps=20, warmup_start=0.0)
    y0 = rng.standard_normal(50)
    opt = ref.SchedFree64([y0], lr=3e-2, betas=(B1, B2), eps=EPS, weight_decay=1e-2, decoupled=decoupled)
    other = in_place_y(y0, grad, 300, 3e-2, 1e-2, decoupled, sched.factor)
    worst = 0.0
    for k in range(300):
        opt.step([grad(opt.y[0], k)], lr_factor=sched.factor(k))
        for a, b in zip((opt.y[0], opt.z[0], opt.x[0]), other[k]):
            worst = max(worst, float(np.abs(a - b).max()))
    print(f"explicit x / z / y form against the in-place-y form, 300 steps: {worst:.3g}")
    assert worst <= 1e-12
    loss = lambda w: 0.5 * float((w - target) @ H @ (w - target))
    assert loss(opt.x[0]) < 0.05 * loss(y0)                  # and the average did go where the problem's solution is


def test_with_r_zero_and_a_constant_factor_x_is_the_uniform_mean_of_z():
    rng = np.random.default_rng(3)
    opt = ref.SchedFree64([rng.standard_normal(17)], lr=1e-2, betas=(B1, B2), eps=EPS)
    zs = []
    for n in range(1, 41):
        opt.step([rng.standard_normal(17)])
        zs.append(opt.z[0].copy())
        assert abs(opt.c - 1.0 / n) <= 1e-15
        assert float(np.abs(opt.x[0] - np.mean(zs, axis=0)).max()) <= 1e-13
    # and with r = 1 the weights are 1, 2, 3, ...: c_n = n / (n (n + 1) / 2)
    opt = ref.SchedFree64([np.zeros(3)], r=1.0, lr_power=0.0)
    for n in range(1, 20):
        opt.step([np.ones(3)])
        assert abs(opt.c - 2.0 / (n + 1)) <= 1e-15


SCALAR_CASES = [dict(r=0.0, lr_power=2.0, sched=None), dict(r=0.0, lr_power=2.0, sched=LRSchedule(warmup_steps=3, warmup_start=0.0)),
                dict(r=1.0, lr_power=0.0, sched=LRSchedule(warmup_steps=3, warmup_start=0.0)),
                dict(r=0.5, lr_power=1.5, sched=LRSchedule(warmup_steps=4, warmup_start=0.25, decay_kind="cosine", total_steps=9))]


@pytest.mark.parametrize("case", SCALAR_CASES, ids=["plain", "from_zero", "r1_p0", "fractional"])
def test_sf_weights_next_is_the_references_scalar_rule(case):
    """the host's copy against weights64 over 12 steps: weight_sum within its bound, f_max exact, c and d within theirs -- and the values
    the rule's text promises: c = 1, d = 0 at the first step with a positive weight; c = 0, d = 1 while weight_sum is 0"""
    blk = {"weight_sum": 0.0, "f_max": 0.0, "c": 0.0, "d": 0.0}
    for n in range(1, 13):
        f = 1.0 if case["sched"] is None else ref.f32(case["sched"].factor(n - 1))
        want = ref.weights64(blk, n, f, case["r"], case["lr_power"])
        ws, f_max, c, d = FlatAdam.sf_weights_next(blk["weight_sum"], blk["f_max"], n, f, case["r"], case["lr_power"])
        assert f_max == want["f_max"] and abs(ws - want["weight_sum"]) <= want["b_weight_sum"]
        assert abs(c - want["c"]) <= want["b_c"] and abs(d - want["d"]) <= want["b_d"]
        assert c == ref.f32(c) and d == ref.f32(d)
        if blk["weight_sum"] == 0.0:
            assert (c, d) == ((1.0, 0.0) if ws > 0.0 else (0.0, 1.0)), (n, c, d)
        blk = {"weight_sum": ws, "f_max": f_max, "c": c, "d": d}
    if case["sched"] is None:
        assert blk["weight_sum"] == 12.0 and blk["c"] == ref.f32(1.0 / 12.0)
    if case["lr_power"] == 0.0:                              # pow(0, 0) = 1: a factor of 0 still counts with weight n^r
        assert blk["weight_sum"] == 78.0
    assert FlatAdam.sf_weights_next(0.0, 0.0, 1, 0.0) == (0.0, 0.0, 0.0, 1.0)      # warmup_start = 0: f = 0, weight_sum stays 0, c = 0


def _problem(decoupled, seed=0):
    """two ranges of the sizes a table block splits at, three steps in: every buffer holds values of a running optimization"""
    rng = np.random.default_rng(seed)
    F = np.float32
    ranges = []
    for n, lr in ((1030, 3e-3), (5, 1e-2)):
        y = rng.standard_normal(n).astype(F)
        z = (y + 0.01 * rng.standard_normal(n)).astype(F)
        x = (y + 0.01 * rng.standard_normal(n)).astype(F)
        ranges.append({"y": y, "z": z, "x": x, "v": (0.1 * rng.random(n)).astype(F), "g": rng.standard_normal(n).astype(F), "lr": lr, "wd": 1e-2})
    before = {"ranges": ranges, "block": {"weight_sum": 2.25, "f_max": 0.75, "c": ref.f32(1.0 / 3.0), "d": ref.f32(2.0 / 3.0)},
              "ema_decay": ref.f32(2.0 / 3.0)}
    n, f = 4, 1.0
    K = ref.consts(B1, B2, EPS, bc2_sqrt=np.sqrt(1.0 - np.float64(np.float32(B2)) ** n), d=0.0, gscale=0.5, lr_factor=f, decoupled=decoupled)
    return before, K, n, f


@pytest.mark.parametrize("decoupled", [False, True], ids=["coupled", "adamw"])
def test_the_checker_accepts_the_emulated_kernel_and_rejects_every_planted_fault(decoupled):
    """without the second half, a checker that passes everything shows nothing"""
    before, K, n, f = _problem(decoupled)
    good = ref.emulate_step(before, K, n, f, 0.0, 2.0)
    K.d = ref.f32(good["block"]["d"])
    used = ref.check_step(before, good, K, n, f, 0.0, 2.0)
    assert set(used) == {"v", "z", "x", "y", "weight_sum", "c", "d"} and all(0.0 <= val <= 1.0 for val in used.values()), used
    assert max(used[k] for k in ref.QUANTITIES) > 0.01        # the bounds are not so wide that a correct kernel uses none of them
    hit = {}
    for fault in ref.MUTATIONS:
        bad = ref.emulate_step(before, K, n, f, 0.0, 2.0, mutate=fault)
        Kb = ref.consts(K.b1, K.b2, K.eps, K.bc2_sqrt, bad["block"]["d"], K.gscale, K.lr_factor, K.decoupled)
        with pytest.raises(AssertionError) as info:
            ref.check_step(before, bad, Kb, n, f, 0.0, 2.0)
        hit[fault] = info.value.args[0][0]
    # each fault is caught at the quantity it damages first
    assert hit["d_is_c"] == "x" and hit["y_old_x"] == "y" and hit["no_bc2"] == "z" and hit["v_first_beta"] == "v", hit
    assert hit["decay_at_z"] == ("z" if decoupled else "v") and hit["sum_keeps"] == "weight_sum" and hit["c_is_d"] == "c", hit


def test_a_skipped_step_must_leave_every_bit_and_a_near_subnormal_moment_is_refused():
    before, K, n, f = _problem(False)
    K.skip = True
    same = ref.emulate_step(before, K, n, f, 0.0, 2.0)
    assert ref.check_step(before, same, K, n, f, 0.0, 2.0) == {}
    for key in ("y", "z", "v", "x"):
        moved = {"ranges": [dict(r) for r in same["ranges"]], "block": same["block"], "ema_decay": same["ema_decay"]}
        moved["ranges"][1][key] = moved["ranges"][1][key].copy()
        moved["ranges"][1][key][2] = np.nextafter(moved["ranges"][1][key][2], np.float32(9))
        with pytest.raises(AssertionError, match="skipped"):
            ref.check_step(before, moved, K, n, f, 0.0, 2.0)
    with pytest.raises(AssertionError, match="skipped"):
        ref.check_step(before, dict(same, block=dict(same["block"], c=0.25)), K, n, f, 0.0, 2.0)
    with pytest.raises(AssertionError, match="skipped"):
        ref.check_step(before, dict(same, ema_decay=0.25), K, n, f, 0.0, 2.0)
    K.skip = False
    tiny = {"ranges": [dict(before["ranges"][1], g=np.full(5, 1e-20, np.float32), v=np.zeros(5, np.float32))], "block": before["block"],
            "ema_decay": before["ema_decay"]}
    Kd = ref.consts(K.b1, K.b2, K.eps, K.bc2_sqrt, K.d, 1.0, 1.0, True)
    with pytest.raises(ref.Refused):
        ref.range64(tiny["ranges"][0], Kd)
