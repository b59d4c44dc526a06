"""Reference of top-p routing (include/avmoe.h at avmoe_moe_forward_top_p / avmoe_router_top_p), written from the header's semantics in
numpy: per frame the ranks (higher p first, equal p in expert order), the running mass in rank order with one sequential np.float32
addition per step, k* = the first prefix whose mass reaches P in an fp32 comparison (E when none does), the clamp to [k_min, k_max], the
mask, kept added in expert order, the weights, the three reports and the auxiliary load; the input families of the checks; plantable
faults; and the checkers the GPU tests call.  check_* raise AssertionError; tests/test_top_p_ref.py shows that they catch each planted
fault.  The site forward and its gradients for a given mask are tests/expert_choice_ref.site_reference (through tests/topk_ref.py)."""
import numpy as np

FAULTS = ("gt_for_ge", "tie_reversed", "no_k_min", "no_k_max", "mass_in_expert_order", "kept_in_rank_order", "khist_shifted")


def ranks_of(p, fault=None):
    """(S, E) int: rank[s, e] = the experts that come before e -- higher p first, equal p in expert order (fault 'tie_reversed': in
    reverse expert order).  For numbers the order of `>` / `==`: -0 and +0 are equal."""
    p = np.asarray(p, np.float32)
    E = p.shape[1]
    e = np.arange(E)
    tie = (e[None, None, :] > e[None, :, None]) if fault == "tie_reversed" else (e[None, None, :] < e[None, :, None])
    before = (p[:, None, :] > p[:, :, None]) | ((p[:, None, :] == p[:, :, None]) & tie)
    return before.sum(-1)


def k_of(p, P, k_min=1, k_max=None, fault=None, ranks=None):
    """(S,) int: k_s.  The running mass is c_j = fl(c_(j-1) + p_(j)) in rank order (fault 'mass_in_expert_order': in expert order), k* the
    smallest j with c_j >= P in fp32 (fault 'gt_for_ge': > P), E when none.  ranks: ranks_of(p) when the caller has it already (it
    depends on p alone)."""
    p = np.asarray(p, np.float32)
    S, E = p.shape
    k_max = E if k_max is None else k_max
    assert 1 <= k_min <= k_max <= E
    P = np.float32(P)
    order = np.argsort(ranks_of(p, fault) if ranks is None else ranks, axis=1, kind="stable")      # order[s, j] = the expert of rank j (the ranks are a permutation)
    if fault == "mass_in_expert_order":
        order = np.tile(np.arange(E), (S, 1))
    ranked = np.take_along_axis(p, order, axis=1)
    c = np.zeros(S, np.float32)
    ks = np.full(S, E, np.int64)
    open_ = np.ones(S, bool)
    for j in range(E):
        c = (c + ranked[:, j]).astype(np.float32)                      # ONE fp32 addition per step
        hit = open_ & ((c > P) if fault == "gt_for_ge" else (c >= P))
        ks[hit] = j + 1
        open_ &= ~hit
    lo = 1 if fault == "no_k_min" else k_min
    hi = E if fault == "no_k_max" else k_max
    return np.minimum(np.maximum(ks, lo), hi)


def select_mask(p, P, k_min=1, k_max=None, fault=None, ranks=None):
    """(S, E) bool: m[s, e] = rank(e) < k_s"""
    ranks = ranks_of(p, fault) if ranks is None else ranks
    return ranks < k_of(p, P, k_min, k_max, fault, ranks)[:, None]


def kept_of(p, mask, ranks=None):
    """(S,) float32: the sum of the kept p, added in expert order in fp32 (ranks given: the planted fault, added in rank order)"""
    p = np.asarray(p, np.float32)
    S, E = p.shape
    cols = np.tile(np.arange(E), (S, 1)) if ranks is None else np.argsort(ranks, axis=1, kind="stable")
    kept = np.zeros(S, np.float32)
    for j in range(E):
        e = cols[:, j]
        pe, me = p[np.arange(S), e], np.asarray(mask)[np.arange(S), e]
        kept = np.where(me, (kept + pe).astype(np.float32), kept)
    return kept


def weights(p, mask, renorm, mix=None, kept=None):
    """(S, E) float32: w = m p, or m p / kept (one fp32 division); then times mix (one fp32 multiplication)"""
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


def khist_of(mask):
    """(E + 1,) int: khist[j] = the frames with k_s = j"""
    mask = np.asarray(mask, bool)
    return np.bincount(mask.sum(1), minlength=mask.shape[1] + 1).astype(np.int32)


def load_of(mask):
    """(E,) float32: count_e / sum_e count_e -- integers below 2^24, exact in fp32; one fp32 division"""
    c = np.asarray(mask, bool).sum(0).astype(np.float32)
    return (c / c.sum(dtype=np.float32)).astype(np.float32)


def emulate(p, P, k_min, k_max, renorm, mix=None, fault=None, ranks=None):
    """dict(mask, choice, count, khist, w) as the header defines them (or with one planted fault)"""
    p = np.asarray(p, np.float32)
    m = select_mask(p, P, k_min, k_max, fault, ranks)
    kept = kept_of(p, m, ranks_of(p) if fault == "kept_in_rank_order" else None)
    kh = khist_of(m)
    if fault == "khist_shifted":
        kh = np.roll(kh, 1)
    return dict(mask=m, choice=bits_of(m), count=m.sum(0).astype(np.int32), khist=kh, w=weights(p, m, renorm, mix, kept=kept))


def check_selection(p, P, k_min, k_max, renorm, mix, choice=None, count=None, khist=None, w=None, ranks=None):
    """What the kernels must return for p (S, E): choice, count, khist and w EXACT (w bit for bit: kept is a sum in expert order, the
    division and the multiplication by mix are single correctly rounded fp32 operations).  No near-tie exclusions: the reference forms the
    same fp32 sums.  -> the mask"""
    p = np.asarray(p, np.float32)
    S, E = p.shape
    ref = emulate(p, P, k_min, k_max, renorm, mix, ranks=ranks)
    m = ref["mask"]
    if choice is not None:
        assert np.all(np.asarray(choice).astype(np.int64) >> E == 0), "bits above E are set"
        got = mask_of_bits(choice, E)
        n = got.sum(1)
        assert n.min() >= k_min and n.max() <= k_max, f"a frame with {n.min()} or {n.max()} experts, outside [{k_min}, {k_max}]"
        assert np.array_equal(got, m), "choice is not the smallest ranked prefix reaching P (ties in expert order), clamped to [k_min, k_max]"
    if count is not None:
        assert np.array_equal(np.asarray(count).astype(np.int64), m.sum(0)), f"count {count} is not the selection's {m.sum(0)}"
    if khist is not None:
        assert np.array_equal(np.asarray(khist).astype(np.int64), ref["khist"]), f"khist {khist} is not the selection's {ref['khist']}"
    if w is not None:
        w = np.asarray(w, np.float32)
        assert np.all(w[~m] == 0), "a non-zero weight off the mask"
        assert np.array_equal(w.view(np.uint32), ref["w"].view(np.uint32)), "w is not m p / kept (or m p), times mix, bit for bit"
    return m


def check_properties(p, P, k_min, k_max, mask):
    """the properties of the rule itself, from p and the mask alone: k_s in [k_min, k_max]; the kept experts are a prefix of the ranking;
    the kept mass (added in rank order) reaches P unless k_max clamped; dropping the last kept expert falls below P unless k_min clamped"""
    p = np.asarray(p, np.float32)
    S, E = p.shape
    P = np.float32(P)
    mask = np.asarray(mask, bool)
    ks = mask.sum(1)
    assert ks.min() >= k_min and ks.max() <= k_max, "k_s outside [k_min, k_max]"
    rk = ranks_of(p)
    assert np.array_equal(mask, rk < ks[:, None]), "the kept experts are not a prefix of the ranking"
    ranked = np.take_along_axis(p, np.argsort(rk, axis=1, kind="stable"), axis=1)
    c = np.zeros((S, E + 1), np.float32)
    for j in range(E):
        c[:, j + 1] = (c[:, j] + ranked[:, j]).astype(np.float32)
    mass, short = c[np.arange(S), ks], c[np.arange(S), ks - 1]
    assert np.all((mass >= P) | (ks == k_max) | (ks == E)), "a kept mass below P without the k_max clamp"
    assert np.all((short < P) | (ks == k_min)), "not minimal: the prefix without its last expert reaches P, and k_min does not ask for it"


# ---- input families (shared by the CPU self-checks and the GPU tests) -----------------------------------------------------------------
FAMILIES = ("uniform", "onehot", "skewed", "zero_column", "threshold_tie", "sweep")


def softmax32(lg):
    lg = np.asarray(lg, np.float32)
    ex = np.exp(lg - lg.max(1, keepdims=True)).astype(np.float32)
    return (ex / ex.sum(1, keepdims=True, dtype=np.float32)).astype(np.float32)


def skewed_logits(S, E, seed=0):
    rng = np.random.default_rng(1000 * seed + 7 * S + E)
    return (1.5 * rng.standard_normal((S, E)) + np.linspace(2.0, 0.0, E)[None, :]).astype(np.float32)


def sweep_logits(S, E):
    """randn . linspace(0, 12, S): from a uniform frame to a one-hot one"""
    return (np.random.default_rng(0).standard_normal((S, E)) * np.linspace(0.0, 12.0, S)[:, None]).astype(np.float32)


def family(name, S, E, seed=0):
    """(S, E) float32.  'uniform': every entry 1 / E (all ties); 'onehot': every row one-hot at the skewed logits' argmax; 'skewed': the
    softmax of skewed_logits; 'zero_column': skewed with one column of zeros; 'threshold_tie': rows of exact binary fractions whose
    prefix masses hit .5 and .75 exactly -- [.5, .25, .25, 0 ...] rotated by the frame index, every other row [.25, .5, .25, 0 ...]
    (E = 2: [.5, .5] and [.75, .25]); 'sweep': the softmax of sweep_logits."""
    if name == "uniform":
        return np.full((S, E), np.float32(1) / np.float32(E), np.float32)
    if name == "sweep":
        return softmax32(sweep_logits(S, E))
    if name == "threshold_tie":
        p = np.zeros((S, E), np.float32)
        a = np.array([.5, .25, .25] if E >= 3 else [.5, .5], np.float32)
        b = np.array([.25, .5, .25] if E >= 3 else [.75, .25], np.float32)
        for s in range(S):
            row = np.zeros(E, np.float32)
            src = a if s % 2 == 0 else b
            row[:len(src)] = src
            p[s] = np.roll(row, (s // 2) % E)
        return p
    lg = skewed_logits(S, E, seed)
    if name == "skewed":
        return softmax32(lg)
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


# the thresholds of the checks: the smallest that still takes one expert, the exact prefix masses of 'threshold_tie' and the fp32 number
# just above .5, a usual setting, and 1 (where an fp32 row sum may fall short: k* = E)
THRESHOLDS = (1e-30, 0.5, float(np.nextafter(np.float32(0.5), np.float32(1))), 0.75, 0.95, 1.0)


def k_ranges(E):
    """(k_min, k_max) of the checks: (1, E), (2, E - 1) where valid, (E, E)"""
    return [(1, E)] + ([(2, E - 1)] if 2 <= E - 1 else []) + [(E, E)]


def mix_for(S, E, seed=0):
    """an (S, E) multiplier with zeros, a negative entry and values beside 1"""
    rng = np.random.default_rng(50 + seed + S + E)
    mix = rng.choice(np.array([0.0, 1.25, 2.0, 0.5], np.float32), size=(S, E)).astype(np.float32)
    mix[0, 0] = -1.5
    return mix
