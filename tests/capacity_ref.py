"""Reference of the expert capacity behind top-k routing (include/avmoe.h at avmoe_moe_forward_capacity / avmoe_router_capacity), written
from the header's formulas in numpy: the selection m of the top-k form (on p, or on the ONE fp32 sum p + b), the keep mask under both
policies by stable sorts, demand, kept_count, cap_scale and the two words per expert.  Integer and ordering logic only: the top-k weights
themselves come from the existing references (tests/topk_ref.py, tests/router_bias_ref.py).  `fault=` plants one of FAULTS into the keep
mask; tests/test_capacity_ref.py shows that the committed input families expose each of them.  check_* raise AssertionError."""
import math
from fractions import Fraction

import numpy as np

ORDER, PRIORITY = 0, 1
NEG_INF = np.float32(-np.inf)


def capacity(f, k, S, E):
    """c = min(S, max(1, ceil(f k S / E))), exactly"""
    return min(S, max(1, math.ceil(Fraction(f) * Fraction(k) * S / E)))


def select_mask(p, k, b=None):
    """(S, E) bool: the k experts of every frame with the highest score -- p, or the ONE fp32 sum p + b --, higher score first, equal
    scores in expert order: what topk_select / topk_select_biased mark."""
    p = np.asarray(p, np.float32)
    sc = p if b is None else (p + np.asarray(b, np.float32)[None, :]).astype(np.float32)
    order = np.argsort(-sc.astype(np.float64), axis=1, kind="stable")      # (fp64: -x is exact, the order is fp32's)
    m = np.zeros(p.shape, bool)
    np.put_along_axis(m, order[:, :k], True, axis=1)
    return m


FAULTS = ("capacity_off_by_one", "ties_reversed", "rank_on_renorm", "rank_on_biased", "count_all_frames", "policies_exchanged")


def keep_mask(p, m, c, policy, b=None, fault=None):
    """(S, E) bool: the pairs of m each expert keeps.  policy ORDER: the first c selecting frames in frame order; PRIORITY: the c selecting
    frames with the largest p[s, e] (the unbiased, unscaled p), equal values in frame order.  demand <= c: everything.
    fault: one of FAULTS, planted for the self-checks (b: the bias `rank_on_biased` ranks with)."""
    p = np.asarray(p, np.float32)
    m = np.asarray(m, bool)
    S, E = p.shape
    assert 1 <= c <= S and policy in (ORDER, PRIORITY)
    if fault == "policies_exchanged":
        policy = 1 - policy
    if fault == "capacity_off_by_one":
        c = c + 1
    val = p.astype(np.float64)
    if fault == "rank_on_renorm":
        with np.errstate(divide="ignore", invalid="ignore"):
            val = np.nan_to_num(val / np.where(m, val, 0.0).sum(1, keepdims=True))
    if fault == "rank_on_biased" and b is not None:
        val = (p + np.asarray(b, np.float32)[None, :]).astype(np.float32).astype(np.float64)
    keep = np.zeros((S, E), bool)
    for e in range(E):
        pool = np.arange(S) if fault == "count_all_frames" else np.nonzero(m[:, e])[0]      # frames that compete for the budget, in frame order
        if policy == PRIORITY:
            v = val[pool, e]
            pool = pool[np.argsort(-v, kind="stable")] if fault != "ties_reversed" else pool[::-1][np.argsort(-v[::-1], kind="stable")]
        elif fault == "ties_reversed":
            pool = pool[::-1]
        keep[pool[:c], e] = True
    return keep & m


def words(p, m, keep, c, policy):
    """(T (E,) float32, L (E,) int64): the two words per expert.  Within the budget: -Inf, S - 1.  ORDER: T = -Inf, L = the c-th selecting
    frame.  PRIORITY: T = the c-th largest p among the selecting frames, L = the largest kept frame among those equal to T."""
    p = np.asarray(p, np.float32)
    S, E = p.shape
    T, L = np.full(E, NEG_INF, np.float32), np.full(E, S - 1, np.int64)
    for e in range(E):
        if m[:, e].sum() <= c:
            continue
        kf = np.nonzero(keep[:, e])[0]
        if policy == ORDER:
            L[e] = kf.max()
        else:
            T[e] = p[kf, e].min()
            L[e] = kf[p[kf, e] == T[e]].max()
    return T, L


def keep_from_words(p, m, T, L, policy):
    """keep = m && s <= L (ORDER) | m && (p > T || (p == T && s <= L)) (PRIORITY): the mask from the two words per expert"""
    p = np.asarray(p, np.float32)
    s = np.arange(p.shape[0])[:, None]
    T, L = np.asarray(T, np.float32)[None, :], np.asarray(L, np.int64)[None, :]
    return m & ((s <= L) if policy == ORDER else ((p > T) | ((p == T) & (s <= L))))


def bits_of(mask):
    mask = np.asarray(mask, bool)
    return (mask.astype(np.int64) << np.arange(mask.shape[1])[None, :]).sum(1).astype(np.int32)


def mask_of_bits(bits, E):
    return ((np.asarray(bits).astype(np.int64)[:, None] >> np.arange(E)[None, :]) & 1).astype(bool)


def cap_scale_of(keep, mix=None):
    """(S, E) float32: keep ? (mix or 1) : +0"""
    one = np.ones(keep.shape, np.float32) if mix is None else np.asarray(mix, np.float32)
    return np.where(keep, one, np.float32(0)).astype(np.float32)


def reference(p, k, c, policy, b=None, mix=None):
    """dict(m, keep, demand, kept_count, cap_scale, thr, last) of p (S, E) at top-k k, capacity c"""
    p = np.asarray(p, np.float32)
    m = select_mask(p, k, b)
    keep = keep_mask(p, m, c, policy)
    demand = m.sum(0).astype(np.int32)
    T, L = words(p, m, keep, c, policy)
    assert np.array_equal(keep_from_words(p, m, T, L, policy), keep), "the reference's own identity"
    assert np.array_equal(keep.sum(0), np.minimum(demand, c)), "the reference's own count"
    return dict(m=m, keep=keep, demand=demand, kept_count=keep.sum(0).astype(np.int32), cap_scale=cap_scale_of(keep, mix), thr=T, last=L)


def dropped_weights(w_in, m, keep):
    """w after the call: the dropped entries SET to +0.0f, every other entry the bits it had"""
    return np.where(m & ~keep, np.float32(0), np.asarray(w_in, np.float32)).astype(np.float32)


def check_outputs(ref, E, kept=None, demand=None, kept_count=None, cap_scale=None, thr=None, last=None, w=None, w_in=None):
    """What the library must return, bit for bit, against reference(...)"""
    if kept is not None:
        assert np.all(np.asarray(kept).astype(np.int64) >> E == 0), "bits above E are set"
        assert np.array_equal(mask_of_bits(kept, E), ref["keep"]), "kept is not the reference's keep mask"
    if demand is not None:
        assert np.array_equal(np.asarray(demand, np.int32), ref["demand"]), f"demand {demand} is not {ref['demand']}"
    if kept_count is not None:
        assert np.array_equal(np.asarray(kept_count, np.int32), ref["kept_count"]), f"kept_count {kept_count} is not {ref['kept_count']}"
    if cap_scale is not None:
        assert np.array_equal(np.asarray(cap_scale, np.float32).view(np.uint32), ref["cap_scale"].view(np.uint32)), "cap_scale is not keep ? mix : +0"
    if thr is not None:
        assert np.array_equal(np.asarray(thr, np.float32).view(np.uint32), ref["thr"].view(np.uint32)), f"thr {thr} is not {ref['thr']}"
    if last is not None:
        assert np.array_equal(np.asarray(last).astype(np.int64), ref["last"]), f"last {last} is not {ref['last']}"
    if w is not None:
        want = dropped_weights(w_in, ref["m"], ref["keep"])
        assert np.array_equal(np.asarray(w, np.float32).view(np.uint32), want.view(np.uint32)), "w: a dropped entry is not +0.0f, or another entry moved"


# ---- input families of the sub-op (shared by the CPU self-checks and the GPU tests) --------------------------------------------------
FAMILIES = ("random", "equal", "one_wins", "balanced", "tie_at_c", "underflow")


def family(name, S, E, seed=0):
    """p (S, E) float32 numpy, finite and non-negative"""
    rng = np.random.default_rng(1000 * seed + 31 * S + E)

    def softmax(z):
        z = z.astype(np.float32)
        ez = np.exp(z - z.max(1, keepdims=True))
        return (ez / ez.sum(1, keepdims=True)).astype(np.float32)
    if name == "random":                                  # what a router produces
        return softmax(2.0 * rng.standard_normal((S, E)))
    if name == "equal":                                   # every entry equal: ties alone decide
        return np.full((S, E), np.float32(1.0) / np.float32(E), np.float32)
    if name == "one_wins":                                # expert 0 wins every frame: heavy overflow
        z = rng.standard_normal((S, E))
        z[:, 0] += 8.0
        return softmax(z)
    if name == "balanced":                                # frame s prefers the experts s, s + 1, ... (mod E): demand as even as S allows
        z = np.zeros((S, E))
        for j in range(E):
            z[np.arange(S), (np.arange(S) + j) % E] = -1.5 * j
        return softmax(z)
    if name == "tie_at_c":                                # few distinct values: the c-th and (c + 1)-th of a column are equal at most c
        return (rng.integers(1, 5, size=(S, E)).astype(np.float32) / np.float32(16)).astype(np.float32)
    if name == "underflow":                               # the softmax underflows to exact zeros beside the winner
        p = softmax(150.0 * rng.standard_normal((S, E)))
        assert (p == 0).any() or S * E < 8
        return p
    raise KeyError(name)


def bias_for(E, seed=0):
    return (0.3 * np.random.default_rng(seed + 11).standard_normal(E)).astype(np.float32)


def mix_for(S, E, seed=0):
    """(S, E) float32 multiplier with exact zeros and ordinary values"""
    rng = np.random.default_rng(seed + 5)
    mix = rng.choice(np.array([0.0, 1.0, 1.25, 2.0], np.float32), size=(S, E)).astype(np.float32)
    mix[S - 1, E - 1] = 0.0
    return mix


def capacities(m):
    """the capacities a selection is checked at: 1, max demand - 1, max demand, S"""
    S = m.shape[0]
    d = int(m.sum(0).max())
    return sorted({c for c in (1, d - 1, d, S) if 1 <= c <= S})


def drops_and_slack(ref, c):
    """(some pair was dropped, some expert stayed within its budget) of one case"""
    return bool((ref["m"] & ~ref["keep"]).any()), bool((ref["demand"] <= c).any())


def has_threshold_tie(p, m, c):
    """does some column hold equal values at ranks c and c + 1 among its selecting frames?"""
    for e in range(p.shape[1]):
        v = np.sort(p[m[:, e], e])[::-1]
        if len(v) > c and v[c - 1] == v[c]:
            return True
    return False
