"""The fp64 reference and checker of FlatAdam's schedule-free AdamW (include/avmoe.h, avmoe_opt_sf_step; csrc/adam_elem.h: sf_elem;
csrc/opt_sched_free.hip: kk_opt_sf_weights, kk_opt_sf_update).  One step is recomputed in fp64 from exactly the fp32 values the device
held BEFORE it -- y (the parameter; behind a perturbation the held value), g, z (exp_avg), v (exp_avg_sq) and x (the shadow) of every
range, the words of the state block and of the 32-byte schedule-free block, the range's rate and decay -- and every element of v, z, x
and y and the block's weight_sum, c and d are held to the bounds below.  Nothing here reads the device: the caller hands over numpy
arrays and Python floats.

The rule (K: the scalars of a step; r: a range; n = applied_steps after the step; f = lr_factor under a schedule, else 1):
    f_max = max(f_max, f) ;  w = n^r * f_max^lr_power ;  weight_sum += w ;  c = w / weight_sum (0 where it is not > 0) ;  d = 1 - c
    coupled: gr = gscale g + wd y         decoupled: gr = gscale g
    v = b2 v + (1 - b2) gr^2
    q = gr / (sqrt(v) / bc2_sqrt + eps)   decoupled: q = q + wd y
    z = z - (lr_r f) q ;  x = d x + (1 - d) z ;  y = b1 x + (1 - b1) z
A skipped step changes nothing (behind a perturbation: the parameter takes the held value back).

The scalars and the elements are checked apart: the block's words against the rule from the block before the step, the elements against
the rule with the fp32 d the block holds AFTER the step (the operand the update kernel read; its own error is the block's check).

The rounding count, from the kernel text, with u = 2^-24 (half an fp32 ulp, relative); only first-order terms are counted and every
count gets one u more for the terms of higher order.  G is the magnitude gr is formed from: |gscale g| decoupled, |gscale g| + |wd y|
coupled (the sum may cancel, so errors are relative to G, not to |gr|).
    gr    1 rounding decoupled; fl(wd y) and the fused multiply-add coupled                                       <= 2 u G
    v     fl(1 - b2): 1 ;  fl(. gr): gr's 2 and 1 ;  fl(. gr): 2 and 1 ;  the fma: 1 on the result -- 8, bound 9:
                                                                     |v - v64| <= 9 u V,  V = b2 v + (1 - b2) G^2   (+ 2^-149)
    den   sqrt(v) moves by at most |v - v64| / sqrt(v64); then the root, the division by bc2_sqrt and the addition of eps round:
          3, bound 4:                                                |den - den64| <= b_v / (sqrt(v64) bc2_sqrt) + 4 u den64 =: b_den
    q     gr's 2 u G over den64, den's error times |gr64| / den64^2, the quotient's rounding: with Q = G / den64
                                                                     |q - q64| <= 3 u Q + Q b_den / den64   (bound: 4 u Q + ...)
          decoupled: fl(wd y) and the sum, on Qd = Q + |wd y|:       2 u Qd more
    z     step = fl(lr_r f): 1 ;  fl(step q): 1 ;  the difference: 1 on |z| + step Qd -- with q's own error, bound one u more:
                                                                     |z - z64| <= step b_q + 3 u step Qd + u (|z| + step Qd)
    x     fl(1 - d), fl(. z), the fma: 3 on X = |d x| + (1 - d) |z64|, bound 4, and (1 - d) times z's bound
    y     fl(1 - b1), fl(. z), the fma: 3 on Y = |b1 x64| + (1 - b1) |z64|, bound 4, and b1 times x's bound, (1 - b1) times z's
    weight_sum   in double.  The device's pow is held to 16 ulp each (OpenCL's bound for a double pow), their product 1, the sum 1; the
          reference's own pow, product and sum 4:                    |ws - ws64| <= 2^-53 (36 w + 2 ws64)
    c     the quotient in double and weight_sum's error: 2^-47 c at most; its rounding to fp32: u c
    d     1 - c in double: 2^-53 and c's 2^-47 c; its rounding to fp32: u |1 - c|
    f_max a maximum of fp32 values: exact
The bounds hold where no operand is subnormal: the checker refuses a step with a v64 below 2^-90 that does not round to 0 in fp32 (the
only input it refuses); v's bound carries one subnormal quantum, 2^-149, for a v that does round to 0.
"""
from types import SimpleNamespace

import numpy as np

U = 2.0 ** -24
BOUNDS = {"gr": 2 * U, "v": 9 * U, "den": 4 * U, "q": 4 * U, "q_decay": 2 * U, "z_step": 3 * U, "z": U, "x": 4 * U, "y": 4 * U}
D53, D47 = 2.0 ** -53, 2.0 ** -47
QUANTITIES = ("v", "z", "x", "y")


class Refused(ValueError):
    """a step outside the range the bounds hold in: a second moment that is subnormal in fp32, or near it"""


def f32(x):
    return float(np.float32(x))


def consts(b1, b2, eps, bc2_sqrt, d, gscale=1.0, lr_factor=1.0, decoupled=False, skip=False):
    """the scalars of one step as the fp32 values the device reads (gscale: fp32(grad_scale * clip_coef); d: the block's after the step)"""
    return SimpleNamespace(b1=f32(b1), b2=f32(b2), eps=f32(eps), bc2_sqrt=f32(bc2_sqrt), d=f32(d), gscale=f32(gscale), lr_factor=f32(lr_factor),
                           decoupled=bool(decoupled), skip=bool(skip))


def weights64(block, n, f, r, lr_power):
    """the scalar rule in fp64 from the block's words before the step -> the words after it (c and d NOT rounded) and their bounds"""
    f_max = max(f32(block["f_max"]), f32(f))
    w = float(np.power(np.float64(n), np.float64(f32(r))) * np.power(np.float64(f_max), np.float64(f32(lr_power))))
    ws = float(block["weight_sum"]) + w
    c = w / ws if ws > 0.0 else 0.0
    d = 1.0 - c
    return {"weight_sum": ws, "f_max": f_max, "c": c, "d": d,
            "b_weight_sum": D53 * (36.0 * w + 2.0 * ws), "b_c": (U + D47) * c, "b_d": U * abs(d) + D47 * c + D53}


def range64(r, K):
    """One range of one applied step in fp64.  r: {"y", "g", "z", "v", "x"}: fp32 arrays as stored before the step, "lr", "wd": the
    range's fp32 rate and decay.  -> the new values and the bound of each."""
    y, g, z, v, x = (np.asarray(r[k], dtype=np.float64).reshape(-1) for k in ("y", "g", "z", "v", "x"))
    lr, wd, d = f32(r["lr"]), f32(r["wd"]), K.d
    step = lr * K.lr_factor
    if K.decoupled:
        gr, G = K.gscale * g, np.abs(K.gscale * g)
    else:
        gr, G = K.gscale * g + wd * y, np.abs(K.gscale * g) + np.abs(wd * y)
    v1, V = K.b2 * v + (1.0 - K.b2) * gr * gr, K.b2 * v + (1.0 - K.b2) * G * G
    if bool(((v1.astype(np.float32) > 0) & (v1 < 2.0 ** -90)).any()):
        raise Refused("a second moment is subnormal in fp32 or near it: outside the range the bounds hold in")
    b_v = BOUNDS["v"] * V + 2.0 ** -149
    root = np.sqrt(v1)
    den = root / K.bc2_sqrt + K.eps
    b_den = np.where(root > 0, b_v / (np.where(root > 0, root, 1.0) * K.bc2_sqrt), np.sqrt(b_v) / K.bc2_sqrt) + BOUNDS["den"] * den
    q, Q = gr / den, G / den
    b_q = BOUNDS["q"] * Q + Q * b_den / den
    Qd = Q
    if K.decoupled:
        q, Qd = q + wd * y, Q + np.abs(wd * y)
        b_q = b_q + BOUNDS["q_decay"] * Qd
    z1 = z - step * q
    b_z = step * b_q + BOUNDS["z_step"] * step * Qd + BOUNDS["z"] * (np.abs(z) + step * Qd)
    x1 = d * x + (1.0 - d) * z1
    b_x = BOUNDS["x"] * (np.abs(d * x) + (1.0 - d) * np.abs(z1)) + (1.0 - d) * b_z
    y1 = K.b1 * x1 + (1.0 - K.b1) * z1
    b_y = BOUNDS["y"] * (np.abs(K.b1 * x1) + (1.0 - K.b1) * np.abs(z1)) + K.b1 * b_x + (1.0 - K.b1) * b_z
    return dict(v=v1, z=z1, x=x1, y=y1, b_v=b_v, b_z=b_z, b_x=b_x, b_y=b_y)


def _frac(err, bound):
    """-> the worst fraction of its bound an error uses; asserts err <= bound, and err == 0 where the bound is 0"""
    err, bound = np.asarray(err, dtype=np.float64).reshape(-1), np.asarray(bound, dtype=np.float64).reshape(-1)
    bad = ~(err <= bound)
    assert not bool(bad.any()), (int(bad.sum()), int(np.argmax(bad)), float(err[bad].max()), float(bound[bad].max()))
    pos = bound > 0
    return float((err[pos] / bound[pos]).max()) if bool(pos.any()) else 0.0


def _same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float32).reshape(-1), np.asarray(b, dtype=np.float32).reshape(-1)
    return np.array_equal(a.view(np.int32), b.view(np.int32))


def check_step(before, after, K, n, f, r, lr_power):
    """One step of the whole optimizer.  before / after: {"ranges": [{"y", "g", "z", "v", "x", "lr", "wd"}, ...] in table order,
    "block": {"weight_sum", "f_max", "c", "d"}, "ema_decay": the state block's word}.  K: consts(...) with K.d == after["block"]["d"] on
    an applied step; n: applied_steps after the step; f: the step's schedule factor (1 without one); r, lr_power: the run's constants.
    A skipped step: every array, every word of the block and the state block's ema_decay keep their bits (y: it holds the value the
    step started from).  An applied step: every bound of the module docstring.
    -> {"v", "z", "x", "y", "weight_sum", "c", "d": the worst fraction of the bound that was used}; raises Refused for the one input the
    bounds do not cover."""
    if K.skip:
        for i, (a, b) in enumerate(zip(before["ranges"], after["ranges"])):
            for k in ("y", "z", "v", "x"):
                assert _same_bits(a[k], b[k]), ("a skipped step wrote", k, "of range", i)
        for k in ("weight_sum", "f_max", "c", "d"):
            assert before["block"][k] == after["block"][k], ("a skipped step wrote the block's", k)
        assert _same_bits(before["ema_decay"], after["ema_decay"]), "a skipped step wrote the state block's ema_decay"
        return {}
    used = {k: 0.0 for k in QUANTITIES + ("weight_sum", "c", "d")}
    want, got = weights64(before["block"], n, f, r, lr_power), after["block"]
    assert f32(got["f_max"]) == want["f_max"], ("f_max", got["f_max"], want["f_max"])
    for k in ("weight_sum", "c", "d"):
        try:
            used[k] = _frac(abs(float(got[k]) - want[k]), want["b_" + k])
        except AssertionError as exc:
            raise AssertionError((k, got[k], want[k]) + exc.args) from None
    assert f32(got["d"]) == K.d, ("the elements are checked with the block's d", got["d"], K.d)
    assert _same_bits(after["ema_decay"], got["d"]), ("the state block's ema_decay is the block's d", after["ema_decay"], got["d"])
    for i, (a, b) in enumerate(zip(before["ranges"], after["ranges"])):
        ref = range64(a, K)
        for k in QUANTITIES:
            dev = np.asarray(b[k], dtype=np.float64).reshape(-1)
            try:
                used[k] = max(used[k], _frac(np.abs(dev - ref[k]), ref["b_" + k]))
            except AssertionError as exc:
                raise AssertionError((k, "range", i, dev.size) + exc.args) from None
    return used


# ---------------------------------------------------------------------------------------------------------------------
MUTATIONS = ("d_is_c", "y_old_x", "no_bc2", "decay_at_z", "v_first_beta", "sum_keeps", "c_is_d")


def emulate_step(before, K, n, f, r, lr_power, mutate=None):
    """The device's step with correctly rounded fp32 operations on the host, in the kernel's operation order (the fused multiply-adds
    are evaluated in fp64 and rounded once) -> `after` as check_step takes it; K.d is ignored (the emulation forms its own).  Used by
    the CPU tests of this checker.  `mutate` plants one fault: "d_is_c" (the average takes c where it should take d), "y_old_x" (y is
    formed from the x before the step), "no_bc2" (the second moment's bias correction is dropped), "decay_at_z" (the decay term is
    taken at z, not at y), "v_first_beta" (v decays with b1), "sum_keeps" (weight_sum is not advanced), "c_is_d" (the block's c and d
    change places)."""
    F = np.float32

    def fma(a, b, c):
        return (np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64) + np.asarray(c, dtype=np.float64)).astype(F)

    blk = dict(before["block"])
    if K.skip:
        return {"ranges": [dict(r_) for r_ in before["ranges"]], "block": blk, "ema_decay": before["ema_decay"]}
    f_max = max(F(blk["f_max"]), F(f))
    w = float(np.power(np.float64(n), np.float64(F(r))) * np.power(np.float64(f_max), np.float64(F(lr_power))))
    ws = float(blk["weight_sum"]) + w
    c64 = w / ws if ws > 0.0 else 0.0
    c, d = F(c64), F(1.0 - c64)
    if mutate == "sum_keeps":
        ws = float(blk["weight_sum"])
    if mutate == "c_is_d":
        c, d = d, c
    d_used = c if mutate == "d_is_c" else d
    b1, b2, eps, gscale = F(K.b1), F(K.b2), F(K.eps), F(K.gscale)
    bc2 = F(1) if mutate == "no_bc2" else F(K.bc2_sqrt)
    out = []
    for r_ in before["ranges"]:
        y, g, z, v, x = (np.asarray(r_[k], dtype=F).reshape(-1) for k in ("y", "g", "z", "v", "x"))
        lr, wd = F(r_["lr"]), F(r_["wd"])
        step = F(lr * F(K.lr_factor))
        at = z if mutate == "decay_at_z" else y
        gr = (g * gscale).astype(F) if K.decoupled else fma(gscale, g, (wd * at).astype(F))
        bv = b1 if mutate == "v_first_beta" else b2
        v1 = fma(bv, v, (((F(1) - bv) * gr).astype(F) * gr).astype(F))
        q = (gr / ((np.sqrt(v1).astype(F) / bc2).astype(F) + eps).astype(F)).astype(F)
        if K.decoupled:
            q = (q + (wd * at).astype(F)).astype(F)
        z1 = (z - (step * q).astype(F)).astype(F)
        x1 = fma(d_used, x, ((F(1) - d_used) * z1).astype(F))
        y1 = fma(b1, x if mutate == "y_old_x" else x1, ((F(1) - b1) * z1).astype(F))
        out.append(dict(r_, y=y1, z=z1, v=v1, x=x1))
    return {"ranges": out, "block": {"weight_sum": ws, "f_max": float(f_max), "c": float(c), "d": float(d)}, "ema_decay": float(d)}


# ---------------------------------------------------------------------------------------------------------------------
class SchedFree64:
    """The rule in the explicit x / z / y form as a plain fp64 optimizer over a list of numpy arrays (one rate and decay for all): the
    trajectory the behaviour tests compare against.  No rounding anywhere."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, decoupled=False, r=0.0, lr_power=2.0):
        self.y = [np.array(p, dtype=np.float64) for p in params]
        self.z = [p.copy() for p in self.y]
        self.x = [p.copy() for p in self.y]
        self.v = [np.zeros_like(p) for p in self.y]
        self.lr, (self.b1, self.b2), self.eps, self.wd, self.decoupled = lr, betas, eps, weight_decay, decoupled
        self.r, self.lr_power = r, lr_power
        self.n, self.weight_sum, self.f_max, self.c = 0, 0.0, 0.0, 0.0

    def step(self, grads, lr_factor=1.0, gscale=1.0):
        self.n += 1
        self.f_max = max(self.f_max, lr_factor)
        w = float(self.n) ** self.r * self.f_max ** self.lr_power
        self.weight_sum += w
        self.c = w / self.weight_sum if self.weight_sum > 0.0 else 0.0
        d, bc2_sqrt = 1.0 - self.c, np.sqrt(1.0 - self.b2 ** self.n)
        for i, g in enumerate(grads):
            y = self.y[i]
            gr = gscale * np.asarray(g, dtype=np.float64) + (0.0 if self.decoupled else self.wd * y)
            self.v[i] = self.b2 * self.v[i] + (1.0 - self.b2) * gr * gr
            q = gr / (np.sqrt(self.v[i]) / bc2_sqrt + self.eps)
            if self.decoupled:
                q = q + self.wd * y
            self.z[i] = self.z[i] - self.lr * lr_factor * q
            self.x[i] = d * self.x[i] + (1.0 - d) * self.z[i]
            self.y[i] = self.b1 * self.x[i] + (1.0 - self.b1) * self.z[i]
