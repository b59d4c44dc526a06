"""The fp64 reference and checker of FlatAdam's Prodigy learning-rate estimation (include/avmoe.h, avmoe_opt_prodigy_step;
csrc/adam_elem.h: prodigy_elem; csrc/opt_kernels.hip: kk_opt_prodigy_update, kk_opt_prodigy_finalize).  One step is recomputed in fp64
from exactly the fp32 values the device held BEFORE it -- p, g, m, v, s, x0 (and the shadow) of every range, the words of the state block
and of the Prodigy block, the range's rate and decay -- and every element of m, v, s, p (and the shadow), both sums of every
1024-element block, and num, den, d_hat, d_max and d are held to the bounds below.  Nothing here reads the device: the caller hands over
numpy arrays and Python floats.

The rule (K: the scalars of a step; r: a range):
    step = (lr_r * lr_factor) * d ;  c = step * (d / d0)      (safeguard_warmup: c = d * (d / d0))
    coupled: gr = gscale g + wd p         decoupled: gr = gscale g, and p <- p (1 - step wd) before the Adam term
    m = b1 m + (1 - b1) d gr ;  v = b2 v + (1 - b2) (d gr)^2 ;  s = beta3 s + c gr
    dot = sum c gr (x0 - p), p before the step ;  l1 = sum |s|, s after it
    p = p - step m / (sqrt(v) + d eps)        dropped where fp32(v) == 0 and fp32(d eps) == 0 (the header's underflow rule)
    num = beta3 num + dot ;  den = l1 ;  d_hat = d_coef num / den (left when den is not > 0 or a term is not finite)
    d_max = max(d_max, d_hat) ;  d = min(d_max, d growth)   (without growth: d_max)
A skipped step changes nothing.

The rounding count, from the kernel text, with u = 2^-24 (half an fp32 ulp, relative).  G is the magnitude gr is formed from:
|gscale g| decoupled, |gscale g| + |wd p| coupled (the sum may cancel, so errors are relative to G, not to |gr|).
    gr    1 rounding decoupled; fl(wd p) and the fused multiply-add coupled: 2                                    <= 2 u G
    step  fl(lr lr_factor), fl(. d): 2 ;  d / d0: 1 ;  c = fl(step dd0): 4 in all
    dg    fl(d gr): 3 u d G ;  cg = fl(c gr): 4 + 2 + 1 = 7 u c G
    m     fl(1 - b1), fl(. dg), the fma: 3 + 3 = 6                 |m - m64| <= 7 u M,  M = |b1 m| + (1 - b1) d G
    v     fl(1 - b2), fl(. dg), fl(. dg), the fma: 4 + 3 + 3 = 10  |v - v64| <= 12 u V, V = b2 v + (1 - b2) (d G)^2
    s     cg and the fma: 8                                        |s - s64| <= 9 u S,  S = |beta3 s| + c G
    dot   per element (double)cg * (x0 - p), the difference and the product exact to 2^-53: 7 u c G |x0 - p|; a block's sum within
          8 u sum c G |x0 - p| (double additions in another order than the reference's: 2^-53 relative per addition, invisible)
    l1    a block's sum within 9 u sum S
    p     A = step m / den, den = sqrt(v) + d eps.  v is a sum of non-negative terms: 12 u relative, 6 u after the root, the root,
          fl(d eps), the sum: den within 9 u.  step 2, fl(step m) 1, the quotient 1 (2 allowed): with m's 7 u M and |m64| <= M,
          |A - A64| <= (7 + 9 + 5) u step M / den64 <= 24 u step M / den64.  decoupled: fl(step wd), fl(1 - .), fl(p .): 3 u |p| (step wd < 1)
          and the difference, 1 u (|p| + |A|):                     |p - p64| <= 4 u |p| + 24 u step M / den64
    e     the shadow, fma(dec, e, fl(fl(1 - dec) p_new)): 3 roundings on |dec e| + (1 - dec) |p64|, plus (1 - dec) times p's bound
    num   the sum of the blocks' dot bounds, plus 2^-50 (|beta3 num| + sum c G |x0 - p|) for the double additions;  den likewise
    d_hat d_coef (num_bound / den64 + |num64| den_bound / den64^2) and its rounding to fp32, u |d_hat64|
    d_max, d   max and min are 1-Lipschitz: d_hat's bound; with growth fl(d growth), u more
The bounds hold where no operand is subnormal: the checker refuses a step with a v64 below 2^-90 that does not round to 0 in fp32; one
that does is the underflow rule's case, and v's bound carries one subnormal quantum, 2^-149, for it.
"""
from types import SimpleNamespace

import numpy as np

U = 2.0 ** -24
BOUNDS = {"m": 7 * U, "v": 12 * U, "s": 9 * U, "dot": 8 * U, "l1": 9 * U, "p_decay": 4 * U, "p_adam": 24 * U, "e": 3 * U}
BLOCK = 1024
F32_MAX = 3.4028234663852886e38


def f32(x):
    return float(np.float32(x))


def beta3_of(beta2):
    """fp32(sqrt((double)fp32(beta2))): what avmoe_opt_prodigy_step hands its kernels"""
    return f32(np.sqrt(np.float64(np.float32(beta2))))


def consts(d, d0, b1, b2, eps, gscale=1.0, lr_factor=1.0, decoupled=False, safeguard=False, d_coef=1.0, growth=None, skip=False,
           ema_decay=None):
    """the scalars of one step as the fp32 values the device reads (gscale: fp32(grad_scale * clip_coef))"""
    return SimpleNamespace(d=f32(d), d0=f32(d0), b1=f32(b1), b2=f32(b2), beta3=beta3_of(b2), eps=f32(eps), gscale=f32(gscale),
                           lr_factor=f32(lr_factor), decoupled=bool(decoupled), safeguard=bool(safeguard), d_coef=f32(d_coef),
                           growth=None if growth is None else f32(growth), skip=bool(skip),
                           ema_decay=None if ema_decay is None else f32(ema_decay))


def range64(r, K):
    """One range of one applied step in fp64.  r: {"p", "g", "m", "v", "s", "x0" (and "e")}: fp32 arrays as stored before the step, "lr",
    "wd": the range's fp32 rate and decay.  -> the new values, the per-element terms of both sums, and the bound of each."""
    p, g, m, v, s, x0 = (np.asarray(r[k], dtype=np.float64).reshape(-1) for k in ("p", "g", "m", "v", "s", "x0"))
    lr, wd, d = f32(r["lr"]), f32(r["wd"]), K.d
    step = lr * K.lr_factor * d
    c = (d if K.safeguard else step) * (d / K.d0)
    if K.decoupled:
        gr, G, pd = K.gscale * g, np.abs(K.gscale * g), p * (1.0 - step * wd)
    else:
        gr, G, pd = K.gscale * g + wd * p, np.abs(K.gscale * g) + np.abs(wd * p), p
    dg = d * gr
    m1, M = K.b1 * m + (1.0 - K.b1) * dg, np.abs(K.b1 * m) + (1.0 - K.b1) * d * G
    v1, V = K.b2 * v + (1.0 - K.b2) * dg * dg, K.b2 * v + (1.0 - K.b2) * (d * G) ** 2
    if bool(((v1.astype(np.float32) > 0) & (v1 < 2.0 ** -90)).any()):
        raise ValueError("a second moment is subnormal in fp32 or near it: outside the range the bounds hold in")
    cg = c * gr
    s1, S = K.beta3 * s + cg, np.abs(K.beta3 * s) + c * G
    dot, DT = cg * (x0 - p), c * G * np.abs(x0 - p)
    den32 = np.sqrt(v1.astype(np.float32)).astype(np.float64) + f32(d * K.eps)          # the header's rule, on fp32 values
    live = den32 > 0
    den = np.where(live, np.sqrt(v1) + d * K.eps, 1.0)
    A = np.where(live, step * m1 / den, 0.0)
    p1 = pd - A
    out = dict(m=m1, v=v1, s=s1, p=p1, dot=dot, l1=np.abs(s1),
               b_m=BOUNDS["m"] * M, b_v=BOUNDS["v"] * V + 2.0 ** -149, b_s=BOUNDS["s"] * S, b_dot=BOUNDS["dot"] * DT, b_l1=BOUNDS["l1"] * S,
               b_p=BOUNDS["p_decay"] * np.abs(p) + np.where(live, BOUNDS["p_adam"] * step * M / den, 0.0), mag_dot=DT, mag_l1=S)
    if K.ema_decay is not None:
        e, dec = np.asarray(r["e"], dtype=np.float64).reshape(-1), K.ema_decay
        out["e"] = dec * e + (1.0 - dec) * p1
        out["b_e"] = BOUNDS["e"] * (np.abs(dec * e) + (1.0 - dec) * np.abs(p1)) + (1.0 - dec) * out["b_p"]
    return out


def block_sums64(ref):
    """the two sums of every 1024-element block of one range and their bounds -> four arrays of ceil(n / 1024)"""
    n = ref["dot"].size
    edges = np.arange(0, n, BLOCK)
    if n == 0:
        return (np.zeros(0),) * 4
    return tuple(np.add.reduceat(ref[k], edges) for k in ("dot", "l1", "b_dot", "b_l1"))


def finalize64(block, sum_dot, sum_abs, K):
    """the finalize rule in fp64 from the block's words before the step -> the words after it (no rounding of d_hat)"""
    num, den = K.beta3 * block["num"] + sum_dot, sum_abs
    d_hat = block["d_hat"]
    if den > 0.0 and np.isfinite(num) and np.isfinite(den) and abs(K.d_coef * num / den) <= F32_MAX:
        d_hat = K.d_coef * num / den
    d_max = max(block["d_max"], d_hat)
    d = d_max if K.growth is None else min(d_max, block["d"] * K.growth)
    return {"d": d, "d_max": d_max, "d_hat": d_hat, "num": num, "den": den}


def _frac(err, bound):
    """-> the worst fraction of its bound an error uses; asserts err <= bound, and err == 0 where the bound is 0"""
    err, bound = np.asarray(err, dtype=np.float64).reshape(-1), np.asarray(bound, dtype=np.float64).reshape(-1)
    bad = ~(err <= bound)
    assert not bool(bad.any()), (int(bad.sum()), int(np.argmax(bad)), float(err[bad].max()), float(bound[bad].max()))
    pos = bound > 0
    return float((err[pos] / bound[pos]).max()) if bool(pos.any()) else 0.0


def check_step(before, after, K):
    """One step of the whole optimizer.  before / after: {"ranges": [{"p", "g", "m", "v", "s", "x0", ("e"), "lr", "wd"}, ...] in table
    order, "block": {"d", "d_max", "d_hat", "num", "den"}}; `after` also "sums": a (n_blocks, 2) array, the workspace behind the step
    (None: not looked at, as after a skipped step).  K: consts(...) with K.d == before["block"]["d"].
    A skipped step: every array and every word of the block keeps its bits.  An applied step: every bound of the module docstring.
    -> {"m", "v", "s", "p", ("e"), "dot", "l1", "num", "den", "d_hat", "d": the worst fraction of the bound that was used}."""
    assert f32(before["block"]["d"]) == K.d, ("the step's d is the block's", before["block"]["d"], K.d)
    names = ("p", "m", "v", "s", "x0") + (("e",) if K.ema_decay is not None else ())
    if K.skip:
        for i, (a, b) in enumerate(zip(before["ranges"], after["ranges"])):
            for k in names:
                x, y = np.asarray(a[k], dtype=np.float32).reshape(-1), np.asarray(b[k], dtype=np.float32).reshape(-1)
                assert np.array_equal(x.view(np.int32), y.view(np.int32)), ("a skipped step wrote", k, "of range", i)
        for k in ("d", "d_max", "d_hat", "num", "den"):
            assert before["block"][k] == after["block"][k], ("a skipped step wrote the block's", k)
        return {}
    used = {k: 0.0 for k in ("m", "v", "s", "p", "dot", "l1") + (("e",) if K.ema_decay is not None else ())}
    sums, row = after.get("sums"), 0
    tot = {"dot": 0.0, "l1": 0.0, "b_dot": 0.0, "b_l1": 0.0, "mag_dot": 0.0, "mag_l1": 0.0}
    for i, (a, b) in enumerate(zip(before["ranges"], after["ranges"])):
        ref = range64(a, K)
        assert np.array_equal(np.asarray(a["x0"]).reshape(-1), np.asarray(b["x0"]).reshape(-1)), ("x0 is only read", i)
        for k in used:
            if k in ("dot", "l1"):
                continue
            got = np.asarray(b[k], dtype=np.float64).reshape(-1)
            try:
                used[k] = max(used[k], _frac(np.abs(got - ref[k]), ref["b_" + k]))
            except AssertionError as exc:
                raise AssertionError((k, "range", i, got.size) + exc.args) from None
        bd, bl, bbd, bbl = block_sums64(ref)
        if sums is not None:
            dev = np.asarray(sums[row:row + bd.size], dtype=np.float64).reshape(-1, 2)
            try:
                used["dot"] = max(used["dot"], _frac(np.abs(dev[:, 0] - bd), bbd))
                used["l1"] = max(used["l1"], _frac(np.abs(dev[:, 1] - bl), bbl))
            except AssertionError as exc:
                raise AssertionError(("block sums", "range", i) + exc.args) from None
        row += bd.size
        for k, x in (("dot", bd), ("l1", bl), ("b_dot", bbd), ("b_l1", bbl)):
            tot[k] += float(x.sum())
        tot["mag_dot"] += float(ref["mag_dot"].sum())
        tot["mag_l1"] += float(ref["mag_l1"].sum())
    if sums is not None:
        assert row == len(sums), ("block count", row, len(sums))
    blk0, blk1 = before["block"], after["block"]
    want = finalize64(blk0, tot["dot"], tot["l1"], K)
    b_num = tot["b_dot"] + 2.0 ** -50 * (abs(K.beta3 * blk0["num"]) + tot["mag_dot"])
    b_den = tot["b_l1"] + 2.0 ** -50 * tot["mag_l1"]
    try:
        used["num"] = _frac(abs(blk1["num"] - want["num"]), b_num)
        used["den"] = _frac(abs(blk1["den"] - want["den"]), b_den)
    except AssertionError as exc:
        raise AssertionError(("num / den", blk1["num"], want["num"], blk1["den"], want["den"]) + exc.args) from None
    if want["den"] > 0.0:
        b_hat = K.d_coef * (b_num / want["den"] + abs(want["num"]) * b_den / want["den"] ** 2) + U * abs(want["d_hat"])
    else:
        b_hat = 0.0
    b_d = b_hat + (U * abs(want["d"]) if K.growth is not None else 0.0)
    try:
        used["d_hat"] = _frac(abs(blk1["d_hat"] - want["d_hat"]), b_hat)
        _frac(abs(blk1["d_max"] - want["d_max"]), b_hat)
        used["d"] = _frac(abs(blk1["d"] - want["d"]), b_d)
    except AssertionError as exc:
        raise AssertionError(("d_hat / d_max / d", blk1, want) + exc.args) from None
    assert blk1["d"] >= blk0["d"] and blk1["d_max"] >= blk0["d_max"], ("d never falls", blk0, blk1)
    return used


# ---------------------------------------------------------------------------------------------------------------------
def emulate_step(before, K, mutate=None):
    """The device's step with correctly rounded fp32 operations on the host, in the kernel's operation order (the fused multiply-adds
    are evaluated in fp64 and rounded once) -> `after` as check_step takes it.  Used by the CPU tests of this checker.  `mutate` plants
    one fault: "drop_block_sum" (finalize leaves the last block's sums out), "p_after" (the dot product reads p after the step),
    "stale_d" (the update uses before["block"]["d_prev"] in place of d), "no_beta3" (num = num + sum_dot), "s_on_skip" (a skipped
    step advances s)."""
    F = np.float32

    def fma(a, b, c):
        return (np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64) + np.asarray(c, dtype=np.float64)).astype(F)

    blk = dict(before["block"])
    d = F(blk["d_prev"]) if mutate == "stale_d" else F(K.d)
    b1, b2, beta3, eps, gscale, d0 = F(K.b1), F(K.b2), F(K.beta3), F(K.eps), F(K.gscale), F(K.d0)
    out, sums = [], []
    for r in before["ranges"]:
        p, g, m, v, s, x0 = (np.asarray(r[k], dtype=F).reshape(-1) for k in ("p", "g", "m", "v", "s", "x0"))
        lr, wd = F(r["lr"]), F(r["wd"])
        step = F(F(lr * F(K.lr_factor)) * d)
        c = F((d if K.safeguard else step) * F(d / d0))
        gr = (g * gscale).astype(F) if K.decoupled else fma(gscale, g, (wd * p).astype(F))
        cg = (c * gr).astype(F)
        if K.skip:
            s1 = fma(beta3, s, cg) if mutate == "s_on_skip" else s
            out.append(dict(r, p=p, m=m, v=v, s=s1, x0=x0))
            continue
        dg = (d * gr).astype(F)
        pd = (p * F(F(1) - F(step * wd))).astype(F) if K.decoupled else p
        m1 = fma(b1, m, ((F(1) - b1) * dg).astype(F))
        v1 = fma(b2, v, (((F(1) - b2) * dg).astype(F) * dg).astype(F))
        s1 = fma(beta3, s, cg)
        den = (np.sqrt(v1).astype(F) + F(d * eps)).astype(F)
        live = den > 0
        q = np.where(live, ((step * m1).astype(F) / np.where(live, den, F(1))).astype(F), F(0)).astype(F)
        p1 = np.where(live, (pd - q).astype(F), pd).astype(F)
        pdot = p1 if mutate == "p_after" else p
        dot = cg.astype(np.float64) * (x0.astype(np.float64) - pdot.astype(np.float64))
        l1 = np.abs(s1).astype(np.float64)
        new = dict(r, p=p1, m=m1, v=v1, s=s1, x0=x0)
        if K.ema_decay is not None:
            dec = F(K.ema_decay)
            new["e"] = fma(dec, np.asarray(r["e"], dtype=F).reshape(-1), ((F(1) - dec) * p1).astype(F))
        out.append(new)
        for b0 in range(0, p.size, BLOCK):
            sums.append((dot[b0:b0 + BLOCK].sum(), l1[b0:b0 + BLOCK].sum()))
    if K.skip:
        return {"ranges": out, "block": {k: blk[k] for k in ("d", "d_max", "d_hat", "num", "den")}, "sums": None}
    sums = np.asarray(sums, dtype=np.float64).reshape(-1, 2)
    used = sums[:-1] if mutate == "drop_block_sum" else sums
    sd, sa = float(used[:, 0].sum()), float(used[:, 1].sum())
    num = (1.0 if mutate == "no_beta3" else float(beta3)) * blk["num"] + sd
    d_hat, d_max, dn = F(blk["d_hat"]), F(blk["d_max"]), F(blk["d"])
    if sa > 0.0 and np.isfinite(num) and np.isfinite(sa) and abs(float(F(K.d_coef)) * num / sa) <= F32_MAX:
        d_hat = F(float(F(K.d_coef)) * num / sa)
    d_max = max(d_max, d_hat)
    dn = d_max if K.growth is None else min(d_max, F(dn * F(K.growth)))
    return {"ranges": out, "sums": sums, "block": {"d": float(dn), "d_max": float(d_max), "d_hat": float(d_hat), "num": num, "den": sa}}


# ---------------------------------------------------------------------------------------------------------------------
class Prodigy64:
    """The rule as a plain fp64 optimizer over a list of numpy arrays (one rate and decay for all): the trajectory the behaviour tests
    compare against.  No rounding anywhere, no underflow rule (fp64 does not underflow on these problems)."""

    def __init__(self, params, lr=1.0, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, decoupled=False, d0=1e-6, d_coef=1.0, growth=None,
                 safeguard=False):
        self.p = [np.array(x, dtype=np.float64) for x in params]
        self.x0 = [x.copy() for x in self.p]
        self.m, self.v, self.s = ([np.zeros_like(x) for x in self.p] for _ in range(3))
        self.lr, (self.b1, self.b2), self.eps, self.wd, self.decoupled = lr, betas, eps, weight_decay, decoupled
        self.d0, self.d_coef, self.growth, self.safeguard = d0, d_coef, growth, safeguard
        self.beta3 = float(np.sqrt(self.b2))
        self.d = self.d_max = d0
        self.d_hat = self.num = self.den = 0.0

    def step(self, grads, lr_factor=1.0, gscale=1.0):
        d, step = self.d, self.lr * lr_factor * self.d
        c = (d if self.safeguard else step) * (d / self.d0)
        dot = l1 = 0.0
        for i, g in enumerate(grads):
            p = self.p[i]
            gr = gscale * np.asarray(g, dtype=np.float64) + (0.0 if self.decoupled else self.wd * p)
            dot += float((c * gr * (self.x0[i] - p)).sum())
            if self.decoupled:
                p = p * (1.0 - step * self.wd)
            self.m[i] = self.b1 * self.m[i] + (1.0 - self.b1) * d * gr
            self.v[i] = self.b2 * self.v[i] + (1.0 - self.b2) * (d * gr) ** 2
            self.s[i] = self.beta3 * self.s[i] + c * gr
            l1 += float(np.abs(self.s[i]).sum())
            self.p[i] = p - step * self.m[i] / (np.sqrt(self.v[i]) + d * self.eps)
        self.num, self.den = self.beta3 * self.num + dot, l1
        if self.den > 0.0 and np.isfinite(self.num) and np.isfinite(self.den):
            self.d_hat = self.d_coef * self.num / self.den
        self.d_max = max(self.d_max, self.d_hat)
        self.d = self.d_max if self.growth is None else min(self.d_max, d * self.growth)
