"""Reference of Sinkhorn-balanced top-k routing (include/avmoe.h at avmoe_moe_forward_sinkhorn / avmoe_router_sinkhorn), written from the
header's formulas in numpy: the column scale v in fp64 (and, to measure what fp32 alone costs, the same iteration in numpy fp32 with
pairwise sums), the selection in fp32 from a GIVEN v exactly as defined -- one fp32 multiplication, a stable descending sort per frame,
kept added in expert order --, the weights, the input families of the sub-op checks, plantable faults, and the checkers the GPU tests
call.  check_* raise AssertionError; tests/test_sinkhorn_ref.py shows that they catch each planted fault on the GPU tests' own inputs.
The site forward and its gradients for a given mask are tests/expert_choice_ref.site_reference (a mask with exactly k experts per frame)."""
import numpy as np

FLT_MAX = float(np.finfo(np.float32).max)
EPS = 2.0 ** -24


# ---- the column scale -------------------------------------------------------------------------------------------------------------------
def scale_fp64(p, iters, fault=None):
    """(E,) float64: v after `iters` rounds of  u_s = 1 / sum_e p[s, e] v_e ,  v_e = (S / E) / sum_s p[s, e] u_s  from v = 1; a column
    whose sum is 0 gets the largest finite fp32.  fault: 'one_fewer' (a round short), 'drop_frame' (the last frame left out of the column
    sums), 'swap_steps' (row step and column step exchanged: the rows are normalised to S / E and the columns to 1.  Merely taking the column
    step first is no fault: from v = 1 the first row step of a softmax is the identity, so that order runs the same iteration)."""
    p = np.asarray(p, np.float32).astype(np.float64)
    S, E = p.shape
    n = iters - 1 if fault == "one_fewer" else iters
    v = np.ones(E)
    rows = S - 1 if fault == "drop_frame" else S

    to_row, to_col = (S / E, 1.0) if fault == "swap_steps" else (1.0, S / E)
    for _ in range(n):
        u = to_row / (p * v[None, :]).sum(1)
        col = (p[:rows] * u[:rows, None]).sum(0)
        with np.errstate(divide="ignore"):
            v = np.minimum(np.where(col > 0, to_col / np.where(col > 0, col, 1.0), FLT_MAX), FLT_MAX)
    return v


def scale_fp32(p, iters):
    """(E,) float32: the same rounds with every operation in numpy fp32, the sums pairwise (numpy's, along a contiguous axis): the error
    that the number format alone leaves in a tree-summed iteration."""
    p = np.asarray(p, np.float32)
    S, E = p.shape
    v = np.ones(E, np.float32)
    target = np.float32(S) / np.float32(E)
    for _ in range(iters):
        u = np.float32(1) / (p * v[None, :]).sum(1, dtype=np.float32)
        col = np.ascontiguousarray((p * u[:, None]).T).sum(1, dtype=np.float32)
        with np.errstate(divide="ignore"):
            v = np.minimum(target / col, np.float32(FLT_MAX)).astype(np.float32)
    return v


def log_error(v, ref):
    """max_e |log(v_e / ref_e)|; an entry the reference clamps to the largest finite fp32 must be exactly that"""
    v, ref = np.asarray(v, np.float64), np.asarray(ref, np.float64)
    assert np.all(np.isfinite(v)) and np.all(v > 0), f"v is not finite and positive: {v}"
    clamp = ref >= FLT_MAX
    assert np.array_equal(v[clamp], ref[clamp]), "a column of zeros does not get the largest finite fp32"
    return float(np.abs(np.log(v[~clamp] / ref[~clamp])).max()) if (~clamp).any() else 0.0


def v_bound(S, E, iters):
    """2 n (S + E + 4) 2^-24: every half-step is a sum of at most max(S, E) positive terms plus a product and a division, each with a
    relative error of at most (terms + 2) 2^-24 in any summation order; the Sinkhorn map does not expand the Hilbert projective metric,
    so the errors of the n rounds add, and the last column step fixes the scale."""
    return 2.0 * iters * (S + E + 4) * EPS


def check_scale(p, iters, v, ref=None):
    """v (E,) against the fp64 reference within v_bound -> the measured error"""
    S, E = np.asarray(p).shape
    err = log_error(v, scale_fp64(p, iters) if ref is None else ref)
    assert err <= v_bound(S, E, iters), f"max |log(v / v_fp64)| = {err:.3e} above 2 n (S + E + 4) 2^-24 = {v_bound(S, E, iters):.3e}"
    return err


# ---- the selection, from a given v ------------------------------------------------------------------------------------------------------
def select_mask(p, v, k, fault=None):
    """(S, E) bool: the k experts with the largest q = p * v (ONE fp32 multiplication) per frame, equal q in expert order.
    fault: 'add' (ranked on p + v), 'tie_reversed' (equal q in reverse expert order)."""
    p, v = np.asarray(p, np.float32), np.asarray(v, np.float32)
    S, E = p.shape
    assert 1 <= k < E
    q = (p + v[None, :]).astype(np.float32) if fault == "add" else (p * v[None, :]).astype(np.float32)
    if fault == "tie_reversed":
        order = E - 1 - np.argsort(-q[:, ::-1].astype(np.float64), axis=1, kind="stable")
    else:
        order = np.argsort(-q.astype(np.float64), axis=1, kind="stable")      # (fp64: -x is exact, the order is fp32's)
    m = np.zeros((S, E), bool)
    m[np.arange(S)[:, None], order[:, :k]] = True
    return m


def kept_of(p, mask, v=None):
    """(S,) float32: the sum of the kept UNSCALED p, added in expert order in fp32 (v given: the planted fault, kept formed from q)"""
    p = np.asarray(p, np.float32)
    src = p if v is None else (p * np.asarray(v, np.float32)[None, :]).astype(np.float32)
    kept = np.zeros(p.shape[0], np.float32)
    for e in range(p.shape[1]):
        kept = np.where(mask[:, e], (kept + src[:, e]).astype(np.float32), kept)
    return kept


def weights(p, mask, renorm, mix=None, kept=None):
    """(S, E) float32: w = m p, or m p / kept; then times mix"""
    p = np.asarray(p, np.float32)
    w = np.where(mask, p, np.float32(0))
    if renorm:
        kept = kept_of(p, mask) if kept is None else kept
        with np.errstate(divide="ignore", invalid="ignore"):
            w = np.where(mask, (p / kept[:, None]).astype(np.float32), np.float32(0))
    if mix is not None:
        w = (w * np.asarray(mix, np.float32)).astype(np.float32)
    return w.astype(np.float32)


def bits_of(mask):
    mask = np.asarray(mask, bool)
    return (mask.astype(np.int64) << np.arange(mask.shape[1])[None, :]).sum(1).astype(np.int32)


def mask_of_bits(bits, E):
    return ((np.asarray(bits).astype(np.int64)[:, None] >> np.arange(E)[None, :]) & 1).astype(bool)


def check_selection(p, v, k, renorm, mix, choice=None, count=None, w=None):
    """What the second launch must return for p (S, E) and the kernel's OWN v: choice and count exact; w bit for bit without renorm
    (w == (m p) mix) and, with it, exactly 0 off the mask and within 1e-6 of the largest weight on it -- one division, as
    tests/router_bias_ref.check_weights allows the top-k weights -- and for k = 1 exactly mix on the mask (x / x = 1: kept IS the kept p).
    No near-tie exclusions: the reference ranks on the same fp32 products."""
    p = np.asarray(p, np.float32)
    S, E = p.shape
    m = select_mask(p, v, k)
    if choice is not None:
        assert np.all(np.asarray(choice).astype(np.int64) >> E == 0), "bits above E are set"
        got = mask_of_bits(choice, E)
        assert np.array_equal(got.sum(1), np.full(S, k)), "not exactly k experts per frame"
        assert np.array_equal(got, m), "choice is not the k largest p v per frame (ties in expert order)"
    if count is not None:
        assert np.array_equal(np.asarray(count).astype(np.int64), m.sum(0)), f"count {count} is not the selection's {m.sum(0)}"
    if w is not None:
        w = np.asarray(w, np.float32)
        ref = weights(p, m, renorm, mix)
        if not renorm:
            assert np.array_equal(w.view(np.uint32), ref.view(np.uint32)), "w is not (m p) mix bit for bit"
        else:
            assert np.all(w[~m] == 0), "a non-zero weight off the mask"
            assert np.all(np.isfinite(w)), "a weight is not finite"
            err = np.abs(w.astype(np.float64) - ref.astype(np.float64))
            assert float(err.max()) <= 1e-6 * float(np.abs(ref).max()), "w is not m p / kept (times mix), kept from the unscaled p"
            if k == 1:
                assert np.array_equal(w.view(np.uint32), ref.view(np.uint32)), "k = 1: w is not exactly mix on the mask (kept is not the kept p)"
    return m


# ---- the kernels' arithmetic in numpy, with plantable faults ------------------------------------------------------------------------------
SCALE_FAULTS = ("one_fewer", "drop_frame", "swap_steps")
SELECT_FAULTS = ("add", "tie_reversed", "kept_from_q")


def emulate(p, k, iters, renorm, mix=None, fault=None):
    """dict(v, choice, count, w) as the two launches form them (v: the fp64 rounds rounded to fp32 -- the summation order of the kernel is
    not modelled, the bound on v does not depend on it)"""
    p = np.asarray(p, np.float32)
    v = scale_fp64(p, iters, fault if fault in SCALE_FAULTS else None).astype(np.float32)
    m = select_mask(p, v, k, fault if fault in ("add", "tie_reversed") else None)
    kept = kept_of(p, m, v if fault == "kept_from_q" else None)
    return dict(v=v, choice=bits_of(m), count=m.sum(0).astype(np.int32), w=weights(p, m, renorm, mix, kept=kept))


# ---- input families (shared by the CPU self-checks and the GPU tests) -----------------------------------------------------------------
FAMILIES = ("skewed", "uniform", "zero_column", "onehot")


def skewed_logits(S, E, seed=0):
    """1.5 N(0, 1) plus a per-expert slope from 2 to 0: the plain top-k selection is clearly unbalanced"""
    rng = np.random.default_rng(1000 * seed + 7 * S + E)
    return (1.5 * rng.standard_normal((S, E)) + np.linspace(2.0, 0.0, E)[None, :]).astype(np.float32)


def softmax32(lg):
    lg = np.asarray(lg, np.float32)
    ex = np.exp(lg - lg.max(1, keepdims=True)).astype(np.float32)
    return (ex / ex.sum(1, keepdims=True, dtype=np.float32)).astype(np.float32)


def family(name, S, E, seed=0):
    """(S, E) float32.  'skewed': the softmax of skewed_logits; 'uniform': every entry 1 / E (all ties); 'zero_column': skewed with one
    column of zeros (its v is the clamp); 'onehot': every row one-hot at the skewed logits' argmax."""
    lg = skewed_logits(S, E, seed)
    if name == "skewed":
        return softmax32(lg)
    if name == "uniform":
        return np.full((S, E), np.float32(1) / np.float32(E), np.float32)
    if name == "zero_column":
        z = E // 2
        lg = lg.copy()
        lg[:, z] = -np.inf
        p = softmax32(lg)
        assert np.all(p[:, z] == 0)
        return p
    if name == "onehot":
        p = np.zeros((S, E), np.float32)
        p[np.arange(S), lg.argmax(1)] = 1
        return p
    raise KeyError(name)


def mix_for(S, E, seed=0):
    """an (S, E) multiplier with zeros, a negative entry and values beside 1"""
    rng = np.random.default_rng(50 + seed + S + E)
    mix = rng.choice(np.array([0.0, 1.25, 2.0, 0.5], np.float32), size=(S, E)).astype(np.float32)
    mix[0, 0] = -1.5
    return mix


def largest_share(mask):
    """the largest share of the routing slots one expert holds"""
    c = np.asarray(mask, bool).sum(0)
    return float(c.max()) / float(c.sum())
