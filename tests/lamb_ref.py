"""The fp64 checker of FlatAdam's layer-wise trust ratios (include/avmoe.h, avmoe_opt_lamb_step; csrc/adam_elem.h: lamb_dir, lamb_next):
one applied step is recomputed in fp64 from exactly the fp32 values the device held -- p before the step, m and v after it (the update
direction is formed from the STORED moments), the words of the state block, the range's rate and decay, and for the parameters the
device's own ratio word -- and every parameter, every element is held to the bounds below.  Nothing here reads the device: the caller
hands over CPU tensors.

The rounding count, from the kernel text, with u = 2^-24 (half an fp32 ulp, relative).  lamb_dir forms, every operation rounded to fp32,
    a = fl(m / bc1)                    1
    s = fl(sqrt(v))                    2
    b = fl(s / bc2_sqrt)               3
    c = fl(b + eps)                    4
    u = fl(a / c)                      5      coupled decay: five roundings in u
    t = fl(wd * p) ; u = fl(u + t)     6, 7   decoupled decay: seven, the decay term and its addition
The square root and the divisions are allowed one ulp (2 u) rather than half: at most 3 u more.  Every rounding acts on a positive sum or
on a factor, so |u - u64| <= about (5 + 3) u |u64| coupled; decoupled the last addition can cancel, and its error is relative to
|quotient| + |wd p| rather than to |u64| -- per element.  The bounds:

    w_norm   sum of (double)p^2 over the range, square root, rounded to fp32: within 2 fp32 ulp of the fp64 norm (the order of the
             double additions differs from the reference's: ~1e-16 relative, invisible in fp32; one ulp for the rounding, one to spare)
    u_norm   within 8 u relative of the fp64 norm of u64: a norm is a positive combination, so the element-wise relative errors do not
             add up beyond their maximum -- decoupled that maximum is relative to |quotient| + |wd p|, which the test's parameters keep
             within the bound (weight decay 1e-2: the decay term is a small part of u)
    ratio    within 10 u relative of w64 / u64: the two norms' errors (up to 8 u + 1 u) and the one rounding of the quotient; exactly
             1.0 for a range that is not adapted, has zero weights or a zero update; exactly fp32(trust_clip) where the fp64 ratio
             exceeds the clamp by more than the bound (within it either answer is right)
    p        every element within 12 u (|p| + |D64|) of p - D64, D64 = lr * lr_factor * (the device's own ratio word) * u64:
             seven roundings in u, fl(lr * lr_factor), fl(. * ratio), fl(step * u): ten acting on |D64| (three of them may be a whole
             ulp: the bound keeps 12), and the subtraction, one acting on |p - D64| <= |p| + |D64|
"""
import numpy as np
import torch

U = 2.0 ** -24
BOUNDS = {"w_norm_ulp": 2, "u_norm": 8 * U, "ratio": 10 * U, "p": 12 * U}


def f32(x):
    return float(np.float32(x))


def ulps(a, b):
    return abs(int(np.float32(a).view(np.int32)) - int(np.float32(b).view(np.int32)))


def direction64(p, m, v, wd, bc1, bc2_sqrt, eps, decoupled):
    """u in fp64 from fp32 operands (tensors and Python floats that are fp32 values)"""
    u = (m.double() / bc1) / (v.double().sqrt() / bc2_sqrt + eps)
    return u + wd * p.double() if decoupled else u


def check_range(p0, p1, m1, v1, w_norm, u_norm, ratio, lr, lr_factor, wd, bc1, bc2_sqrt, eps, decoupled, adapted, clip):
    """One range of one applied step.  p0: the parameter before the step (fp32 CPU tensor), p1, m1, v1: parameter and moments after it;
    w_norm, u_norm, ratio: the device's report words (Python floats); lr, wd, bc1, bc2_sqrt, eps, lr_factor: the fp32 values the device
    read, as Python floats; clip: fp32(trust_clip) or None.  Asserts every bound of the module docstring and returns the fraction of each
    bound that was used, {"w_norm": ulps / 2, "u_norm": ..., "ratio": ... or None for a special case, "p": ...}, and which case the
    ratio was ("off", "zero_w", "zero_u", "clamped", "free", "edge")."""
    n = p0.numel()
    u64 = direction64(p0, m1, v1, wd, bc1, bc2_sqrt, eps, decoupled)
    wn64, un64 = float(p0.double().pow(2).sum().sqrt()), float(u64.pow(2).sum().sqrt())
    used = {}
    w_ulp = ulps(w_norm, wn64)
    assert w_ulp <= BOUNDS["w_norm_ulp"], ("w_norm", n, w_norm, wn64, w_ulp)
    used["w_norm"] = w_ulp / BOUNDS["w_norm_ulp"]
    du = abs(u_norm - un64)
    assert du <= BOUNDS["u_norm"] * un64, ("u_norm", n, u_norm, un64, du / max(un64, 1e-300) / U)
    used["u_norm"] = du / (BOUNDS["u_norm"] * un64) if un64 > 0 else 0.0
    used["ratio"] = None
    if not adapted:
        case = "off"
        assert ratio == 1.0, ("a range that is not adapted", n, ratio)
    elif wn64 == 0.0 or un64 == 0.0:
        case = "zero_w" if wn64 == 0.0 else "zero_u"
        assert ratio == 1.0, (case, n, ratio)
    else:
        r64 = wn64 / un64
        if clip is not None and r64 > clip * (1 + BOUNDS["ratio"]):
            case = "clamped"
            assert ratio == clip, ("clamp", n, ratio, clip, r64)
        elif clip is not None and r64 >= clip * (1 - BOUNDS["ratio"]):
            case = "edge"
            assert ratio == clip or abs(ratio - r64) <= BOUNDS["ratio"] * r64, ("at the clamp", n, ratio, clip, r64)
        else:
            case = "free"
            dr = abs(ratio - r64)
            assert dr <= BOUNDS["ratio"] * r64, ("ratio", n, ratio, r64, dr / r64 / U)
            used["ratio"] = dr / (BOUNDS["ratio"] * r64)
    d64 = (float(lr) * float(lr_factor) * float(ratio)) * u64
    want = p0.double() - d64
    err = (p1.double() - want).abs()
    bound = BOUNDS["p"] * (p0.double().abs() + d64.abs())
    bad = err > bound
    assert not bool(bad.any()), ("p", n, int(bad.sum()), float((err - bound).max()))
    frac = err / bound.clamp_min(1e-300)
    used["p"] = float(torch.where(bound > 0, frac, torch.zeros_like(frac)).max()) if n else 0.0
    assert bool((err[bound == 0] == 0).all())                # a zero bound (p == 0 and no update) leaves the element as it was
    return used, case


def emulate_step(p, g, m, v, lr, lr_factor, wd, b1, b2, eps, bc1, bc2_sqrt, gscale, decoupled, adapted, clip):
    """The device's step of one range with correctly rounded fp32 operations on the host (numpy float32 arrays in, fp32 scalars as
    np.float32): -> p', m', v', w_norm, u_norm, ratio.  The fused multiply-adds are evaluated in fp64 and rounded once (exact for fp32
    operands up to a double rounding, which fp64's 29 spare bits make vanishingly rare).  Used by the CPU test of this checker."""
    F = np.float32
    p, g, m, v = (np.asarray(x, dtype=F) for x in (p, g, m, v))
    lr, lr_factor, wd, b1, b2, eps, bc1, bc2_sqrt, gscale = (F(x) for x in (lr, lr_factor, wd, b1, b2, eps, bc1, bc2_sqrt, gscale))

    def fma(a, b, c):
        return (np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64) + np.asarray(c, dtype=np.float64)).astype(F)

    gr = (g * gscale).astype(F) if decoupled else fma(gscale, g, (wd * p).astype(F))
    m1 = fma(b1, m, (F(1) - b1) * gr)
    v1 = fma(b2, v, ((F(1) - b2) * gr).astype(F) * gr)
    u = ((m1 / bc1).astype(F) / ((np.sqrt(v1).astype(F) / bc2_sqrt).astype(F) + eps).astype(F)).astype(F)
    if decoupled:
        u = (u + (wd * p).astype(F)).astype(F)
    wn, un = np.sqrt(np.sum(p.astype(np.float64) ** 2)), np.sqrt(np.sum(u.astype(np.float64) ** 2))
    q = 1.0
    if adapted and wn > 0 and un > 0 and np.isfinite(wn) and np.isfinite(un):
        q = wn / un
        if clip is not None and q > float(F(clip)):
            q = float(F(clip))
    ratio = F(q)
    step = F(F(lr * lr_factor) * ratio)
    p1 = (p - (step * u).astype(F)).astype(F)
    return p1, m1, v1, float(F(wn)), float(F(un)), float(ratio)
