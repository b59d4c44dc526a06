"""Reference of expert-choice gating (include/avmoe.h at avmoe_moe_forward_choice / avmoe_expert_choice), written from the header's
formulas in numpy / torch: the selection by a stable descending sort per column, the two words (T_e, L_e) that describe it, the weights
under both renorm settings (kept added in expert order in fp32; a frame no expert took has weights 0), the site forward and its gradients
by autograd, the input families of the sub-op checks, a numpy emulation of the kernel's algorithm (radix select on the ordered key, one
ordered tie pass) with plantable faults, and the checker the GPU tests call.  check_* raise AssertionError; tests/test_expert_choice_ref.py
shows that the checker catches each planted fault."""
import math
from fractions import Fraction

import numpy as np
import torch
import torch.nn.functional as F

from oracle import avmoe_oracle as O
from tests.topk_ref import topk_forward, topk_grads


# ---- the selection --------------------------------------------------------------------------------------------------------------------
def choice_mask(p, c):
    """(S, E) bool numpy: column e is True on the c frames with the highest p[:, e] -- a stable descending sort: higher value first,
    equal values in frame order."""
    p = np.asarray(p, np.float32)
    S, E = p.shape
    assert 1 <= c <= S
    m = np.zeros((S, E), bool)
    for e in range(E):
        order = np.argsort(-p[:, e].astype(np.float64), kind="stable")      # (fp64: -x is exact, the order is fp32's)
        m[order[:c], e] = True
    return m


def thr_last(p, c):
    """(T (E,) float32, L (E,) int64): T_e the c-th largest value of column e, L_e the largest frame taken among the frames equal to T_e."""
    p = np.asarray(p, np.float32)
    m = choice_mask(p, c)
    T = np.array([p[m[:, e], e].min() for e in range(p.shape[1])], np.float32)
    L = np.array([np.nonzero(m[:, e] & (p[:, e] == T[e]))[0].max() for e in range(p.shape[1])], np.int64)
    return T, L


def mask_from_words(p, T, L):
    """m[s, e] = (p[s, e] > T_e) || (p[s, e] == T_e && s <= L_e): the mask from the two words per expert."""
    p = np.asarray(p, np.float32)
    s = np.arange(p.shape[0])[:, None]
    T, L = np.asarray(T, np.float32)[None, :], np.asarray(L, np.int64)[None, :]
    return (p > T) | ((p == T) & (s <= L))


def bits_of(mask):
    """(S,) int32: bit e set where mask[s, e]"""
    mask = np.asarray(mask, bool)
    return (mask.astype(np.int64) << np.arange(mask.shape[1])[None, :]).sum(1).astype(np.int32)


def mask_of_bits(bits, E):
    return ((np.asarray(bits).astype(np.int64)[:, None] >> np.arange(E)[None, :]) & 1).astype(bool)


def weights(p, mask, renorm, mix=None):
    """(S, E) float32: w = m p, or m p / kept with kept = sum_e m p added in expert order in fp32 and w = 0 on a frame no expert took;
    then times mix."""
    p = np.asarray(p, np.float32)
    mask = np.asarray(mask, bool)
    w = np.where(mask, p, np.float32(0))
    if renorm:
        kept = np.zeros(p.shape[0], np.float32)
        for e in range(p.shape[1]):
            kept = np.where(mask[:, e], (kept + p[:, e]).astype(np.float32), kept)
        with np.errstate(divide="ignore", invalid="ignore"):
            w = np.where(mask, (p / kept[:, None]).astype(np.float32), np.float32(0))
    if mix is not None:
        w = (w * np.asarray(mix, np.float32)).astype(np.float32)
    return w.astype(np.float32)


def capacity(k, S, E):
    """c = min(S, max(1, ceil(k S / E))), exactly"""
    return min(S, max(1, math.ceil(Fraction(k) * S / E)))


# ---- the checker of the sub-op's outputs ------------------------------------------------------------------------------------------------
def reference(p, c):
    """(mask, T, L) of p at capacity c, computed once for the checks that share it"""
    m = choice_mask(p, c)
    T, L = thr_last(p, c)
    assert np.array_equal(mask_from_words(p, T, L), m), "the reference's own identity"
    return m, T, L


def check_subop(p, c, renorm, mix, choice=None, thr=None, last=None, w=None, ref=None):
    """What avmoe_expert_choice must return for p (S, E), capacity c: choice / thr / last bit for bit; w bit for bit without renorm
    (w == (m p) mix), and with it exactly 0 (either sign) off the mask and within 1e-6 of the largest weight on it -- one division, as
    tests/router_bias_ref.check_weights allows the top-k weights.  ref: reference(p, c), when the caller already has it."""
    p = np.asarray(p, np.float32)
    S, E = p.shape
    m, T, L = ref if ref is not None else reference(p, c)
    if choice is not None:
        got = mask_of_bits(choice, E)
        assert np.all(np.asarray(choice).astype(np.int64) >> E == 0), "bits above E are set"
        assert np.array_equal(got.sum(0), np.full(E, c)), f"not {c} frames per expert: {got.sum(0)}"
        assert np.array_equal(got, m), "choice is not the c highest frames per expert (ties in frame order)"
    if thr is not None:
        assert np.array_equal(np.asarray(thr, np.float32).view(np.uint32), T.view(np.uint32)), f"thr {thr} is not the c-th largest {T}"
    if last is not None:
        assert np.array_equal(np.asarray(last).astype(np.int64), L), f"last {last} is not {L}"
    if w is not None:
        w = np.asarray(w, np.float32)
        ref = weights(p, m, renorm, mix)
        if not renorm:
            assert np.array_equal(w.view(np.uint32), ref.view(np.uint32)), "w is not (m p) mix bit for bit"
        else:
            assert np.all(w[~m] == 0), "a non-zero weight off the mask (a frame no expert took has weights 0)"
            nan = np.isnan(ref)                           # (0 / 0 by the formula: every expert that took the frame has p = 0 there)
            assert np.array_equal(np.isnan(w), nan), "NaN where the formula has none, or none where it has 0 / 0"
            assert np.all(np.isfinite(w[~nan])), "an infinite weight"
            scale = float(np.abs(ref[~nan]).max()) if (~nan).any() else 0.0
            err = np.abs(w[~nan].astype(np.float64) - ref[~nan].astype(np.float64))
            assert err.size == 0 or float(err.max()) <= 1e-6 * scale, "w is not m p / kept (times mix)"


# ---- input families of the sub-op (shared by the CPU emulation checks and the GPU tests) ----------------------------------------------
FAMILIES = ("softmax", "uniform", "two_valued", "low_byte", "high_byte", "ascending", "descending", "mostly_zero", "signed")
RENORMS = {"signed": (0,)}           # family -> renorm settings checked (default both): a kept sum of mixed signs may cancel to 0


def standard_capacities(S, E):
    return sorted({c for c in (1, 2, -(-S // E), S - 1, S) if 1 <= c <= S})


def family(name, S, E, seed=0):
    """(p (S, E) float32 numpy, [further capacities the family is made for])"""
    rng = np.random.default_rng(1000 * seed + 17 * S + E)
    if name == "softmax":                                 # what a router produces
        z = rng.standard_normal((S, E)).astype(np.float32)
        ez = np.exp(z - z.max(1, keepdims=True))
        return (ez / ez.sum(1, keepdims=True)).astype(np.float32), []
    if name == "uniform":                                 # all equal: the first c frames
        return np.full((S, E), np.float32(1.0) / np.float32(E), np.float32), []
    if name == "two_valued":
        # even columns: 0.75 on a group of up to 12 frames that straddles 1023 | 1024 (S >= 1025) or 255 | 256 (S >= 257), 0.25 elsewhere:
        # c <= group: T = 0.75 and L inside the group.  odd columns: 0.75 on three frames, 0.25 elsewhere: c > 3 puts the threshold in the
        # 0.25 group, which runs over every chunk and wave boundary.
        a = 1018 if S >= 1025 else (250 if S >= 257 else S // 3)
        n = min(a + 12, S) - a
        p = np.full((S, E), 0.25, np.float32)
        for e in range(E):
            if e % 2 == 0:
                p[a:a + n, e] = 0.75
            else:
                p[[0, S // 2, S - 1], e] = 0.75
        extra = [n, n - 1, n + 3, 3 + 260, 3 + 1030]
        return p, sorted({c for c in extra if 1 <= c <= S})
    if name in ("low_byte", "high_byte"):
        p = np.empty((S, E), np.float32)
        for e in range(E):
            i = rng.permutation(S).astype(np.uint32)
            if name == "low_byte":                        # 0x3F000000 + i: the first three radix passes see one bin
                p[:, e] = (np.uint32(0x3F000000) + (i & np.uint32(255))).view(np.float32)
            else:                                         # only the highest byte differs (1 .. 124: positive, 16 of them add up below the largest fp32)
                p[:, e] = (((i % np.uint32(124) + np.uint32(1)) << np.uint32(24)) | np.uint32(0x00400000)).view(np.float32)
        return p, []
    if name in ("ascending", "descending"):
        col = (np.arange(S, dtype=np.float32) + 1) / np.float32(S + 1)
        col = col if name == "ascending" else col[::-1]
        return np.repeat(col[:, None], E, 1).astype(np.float32).copy(), []
    if name == "mostly_zero":                             # 80 % exact zeros, c above the non-zero count
        p = rng.random((S, E)).astype(np.float32)
        p[rng.random((S, E)) < 0.8] = 0.0
        nz = int((p != 0).sum(0).max())
        return p, sorted({c for c in (nz + 1, nz + 3) if 1 <= c <= S})
    if name == "signed":                                  # a caller's matrix with negative entries: the ordered key, not the raw bits
        return rng.standard_normal((S, E)).astype(np.float32), []
    raise KeyError(name)


def mix_for(S, E, seed=0):
    """(S, E) float32 multiplier with exact zeros, a negative entry and ordinary values"""
    rng = np.random.default_rng(seed + 5)
    mix = rng.choice(np.array([0.0, 1.0, 1.25, 2.0], np.float32), size=(S, E)).astype(np.float32)
    mix[0, 0] = -1.5
    mix[S - 1, E - 1] = 0.0
    return mix


# ---- numpy emulation of the kernels (csrc/expert_choice.hip), with plantable faults -------------------------------------------------
def ordered_key(p, raw=False):
    """order-preserving uint32 key of fp32 values (-0 and +0 share one); raw: the bits themselves (a planted fault)"""
    u = np.asarray(p, np.float32).view(np.uint32).copy()
    if raw:
        return u
    u[u == np.uint32(0x80000000)] = 0
    neg = (u & np.uint32(0x80000000)) != 0
    return np.where(neg, ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def unkey(k):
    k = np.uint32(k)
    u = (k & np.uint32(0x7FFFFFFF)) if (k & np.uint32(0x80000000)) else ~k
    return np.array([u], np.uint32).view(np.float32)[0]


def emulate_select(col, c, chunk=256, fault=None):
    """(T float32, L int) of one column: exact radix select of the c-th largest ordered key, most significant byte first (4 x 8 bits, a
    256-bin histogram and a descending bin scan per byte), then one ordered pass in chunks of `chunk` frames with a running count of
    key == T: the frame that holds the `need`-th tie is L."""
    key = ordered_key(col, raw=fault == "raw_bits")
    need = c + 1 if fault == "c_plus_one" else c
    need = min(need, len(key))
    prefix, mask = np.uint32(0), np.uint32(0)
    for shift in (24, 16, 8, 0):
        hit = (key & mask) == prefix
        hist = np.bincount(((key[hit] >> np.uint32(shift)) & np.uint32(255)).astype(np.int64), minlength=256)
        for b in range(255, -1, -1):
            if need <= hist[b]:
                prefix |= np.uint32(b << shift)
                break
            need -= hist[b]
        mask |= np.uint32(0xFF << shift)
    base, last = 0, -1
    for s0 in range(0, len(key), chunk):
        flag = key[s0:s0 + chunk] == prefix
        if fault == "chunk_reset":
            base = 0
        rank = base + np.cumsum(flag)
        at = np.nonzero(flag & (rank == need))[0]
        if len(at):
            last = s0 + int(at[0])
        base += int(flag.sum())
        if base >= need and fault != "chunk_reset":
            break
    T = unkey(prefix) if fault != "raw_bits" else np.array([prefix], np.uint32).view(np.float32)[0]
    if fault == "tie_high":                               # the ties taken from the highest frames: L is then the FIRST frame taken
        ties = np.nonzero(key == prefix)[0]
        last = int(ties[len(ties) - need])
    return np.float32(T), last


FAULTS = ("tie_high", "c_plus_one", "ge_for_gt", "other_column", "chunk_reset", "raw_bits", "kept_all", "weight_on_empty")


def emulate(p, c, renorm, mix=None, chunk=256, fault=None):
    """dict(choice, thr, last, w) as the two kernels produce them; `fault`: one of FAULTS planted"""
    p = np.asarray(p, np.float32)
    S, E = p.shape
    TL = [emulate_select(p[:, e], c, chunk, fault) for e in range(E)]
    T = np.array([t for t, _ in TL], np.float32)
    L = np.array([l for _, l in TL], np.int64)
    Tm = np.roll(T, 1) if fault == "other_column" else T
    s = np.arange(S)[:, None]
    kp, kt = ordered_key(p.reshape(-1)).reshape(S, E), ordered_key(Tm)[None, :]
    if fault == "ge_for_gt":
        m = kp >= kt
    elif fault == "tie_high":
        m = (kp > kt) | ((kp == kt) & (s >= L[None, :]))
    else:
        m = (kp > kt) | ((kp == kt) & (s <= L[None, :]))
    w = weights(p, m, renorm, None)
    if renorm and fault == "kept_all":
        kept = np.zeros(S, np.float32)
        for e in range(E):
            kept = (kept + p[:, e]).astype(np.float32)
        w = np.where(m, (p / kept[:, None]).astype(np.float32), np.float32(0))
    if renorm and fault == "weight_on_empty":
        w = np.where(m.any(1)[:, None], w, p)
    if mix is not None:
        w = (w * np.asarray(mix, np.float32)).astype(np.float32)
    return dict(choice=bits_of(m), thr=T, last=L, w=w.astype(np.float32))


# ---- the site: forward and gradients given the mask -------------------------------------------------------------------------------------
def ec_forward(P, B, X, Y, cfg, mask, renorm, mix=None, training=True, noise=None, mha_keep=None):
    """The site with expert-choice weights for the given (S, E) 0 / 1 mask (which carries no gradient) -> dict(out, probs, lb, z, w):
    tests/topk_ref.topk_forward with its own mixture line, because topk_weights divides 0 / 0 on a frame no expert took."""
    Wc = P["conv_adapter.weight"][:, :, 0, 0]
    Yt = torch.einsum("nm,smc->snc", Wc, Y) + P["conv_adapter.bias"][None, :, None]
    Yf = Yt @ P["fc.weight"].t() + P["fc.bias"]
    rin = torch.cat([X.mean(dim=1), Yf.mean(dim=1)], dim=-1)
    h = F.relu(rin @ P["router.0.weight"].t() + P["router.0.bias"])
    h = F.relu(h @ P["router.2.weight"].t() + P["router.2.bias"])
    logits = h @ P["router.4.weight"].t() + P["router.4.bias"]
    if noise is not None:
        logits = logits + noise
    probs = F.softmax(logits, dim=-1)
    m = torch.as_tensor(mask).to(device=probs.device, dtype=probs.dtype)
    w = m * probs
    if renorm:
        kept = w.sum(-1, keepdim=True)
        some = m.sum(-1, keepdim=True) > 0
        w = torch.where(some, w / torch.where(some, kept, torch.ones_like(kept)), torch.zeros_like(w))
    if mix is not None:
        w = w * torch.as_tensor(mix).to(device=w.device, dtype=w.dtype)
    out = torch.zeros_like(X)
    for j, pre in enumerate(cfg.expert_prefixes()):       # every expert on every frame, as in the dense site
        o = O.expert_forward(P, B, pre, X, Yf, cfg, j < cfg.E_m, training, None, mha_keep)
        out = out + w[:, j].reshape(-1, 1, 1) * o
    lb = O.load_balancing_loss(probs) if cfg.lb_loss else torch.zeros((), dtype=X.dtype)
    z = (torch.logsumexp(logits.float(), dim=-1) ** 2).mean()
    return dict(out=out, probs=probs, lb=lb, z=z, w=w)


def ec_grads(cfg, P, B, X, Y, dO, dP, lb_weight, mask, renorm, mix=None, aux_grad=None, load=None, training=True, noise=None):
    """Gradients of <out, dO> + <probs, dP> + lb_weight lb + g_z z + g_b E sum_e load_e mean_s p_se (load a constant: the dense site's
    k' = 1 share) -> {'X', 'Y', parameter key: gradient}; dO / dP / aux_grad None = that term absent."""
    Pg = {kk: v.detach().clone().requires_grad_(True) for kk, v in P.items()}
    Xg, Yg = X.detach().clone().requires_grad_(True), Y.detach().clone().requires_grad_(True)
    fwd = ec_forward(Pg, B, Xg, Yg, cfg, mask, renorm, mix, training=training, noise=noise)
    loss = torch.zeros((), dtype=torch.float32, device=X.device)
    if dO is not None:
        loss = loss + (fwd["out"] * dO).sum()
    if dP is not None:
        loss = loss + (fwd["probs"] * dP).sum()
    if cfg.lb_loss and lb_weight:
        loss = loss + lb_weight * fwd["lb"]
    if aux_grad is not None:
        g_z, g_b = aux_grad
        loss = loss + g_z * fwd["z"] + g_b * cfg.E * (torch.as_tensor(load).to(fwd["probs"]) * fwd["probs"].mean(0)).sum()
    keys = ["X", "Y"] + list(Pg)
    gs = torch.autograd.grad(loss, [Xg, Yg] + list(Pg.values()), allow_unused=True)
    ref = {"X": Xg, "Y": Yg, **Pg}
    return {kk: (g.detach() if g is not None else torch.zeros_like(ref[kk])) for kk, g in zip(keys, gs)}


def site_reference(cfg, P, B, X, Y, dO, dP, lb_weight, mask, renorm, mix=None, aux_grad=None, load=None, noise=None):
    """{'out', 'X', 'Y', parameter key} of the site for the given mask.  Without renorm, multiplier and auxiliary terms this is
    tests/topk_ref.py's top-k reference with sel = mask (its weights are then m p for any k < E); everything else goes through ec_forward."""
    mt = torch.as_tensor(np.asarray(mask)).to(torch.float32)
    if not renorm and mix is None and aux_grad is None:
        ref = topk_grads(cfg, P, B, X, Y, dO, dP, lb_weight, True, 1, False, noise=noise, sel=mt)
        ref["out"] = topk_forward(P, B, X, Y, cfg, 1, False, training=True, noise=noise, update_buffers=False, sel=mt)["out"]
        return ref
    ref = ec_grads(cfg, P, B, X, Y, dO, dP, lb_weight, mt, renorm, mix, aux_grad, load, noise=noise)
    ref["out"] = ec_forward(P, B, X, Y, cfg, mt, renorm, mix, noise=noise)["out"].detach()
    return ref


def s300_inputs():
    """(cfg, S, P, B, X, Y, noise, c) of the S = 300 site check: tests/router_bias_ref.selection_case('tile_fast') with its logit noise
    rescaled to 0.5, and c = S / E = 75.  A freshly initialised router hardly moves with the frame, so the noise decides the routing: at
    scale 0.5 the oracle's softmax leaves dozens of frames without an expert and dozens with two or more (tests/test_expert_choice_ref.py
    asserts at least S / 16 of each)."""
    from tests import router_bias_ref as R
    cfg, S, P, B, X, Y, noise, _ = R.selection_case("tile_fast")
    return cfg, S, P, B, X, Y, 0.5 * noise, S // cfg.E


def served_counts(mask):
    """(frames with no expert, frames with two or more)"""
    n = np.asarray(mask, bool).sum(1)
    return int((n == 0).sum()), int((n >= 2).sum())
