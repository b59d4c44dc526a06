"""Checker of the mixture regularisers' draw (avmoe_mix_drop_draw, include/avmoe.h): a from-scratch numpy Philox-4x32-10 and the
(seed, calls, S, E, p, q) -> (S, E) multiplier built on it.  Nothing here imports the library.

Philox-4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC 2011): ten rounds of
    hi0:lo0 = M0 * c0    hi1:lo1 = M1 * c2    (c0, c1, c2, c3) <- (hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0)
with the key bumped by (W0, W1) between rounds (nine bumps).  KAT_ZERO is the output for an all-zero counter and key; it was confirmed by
two independent routes before it was committed: this numpy code and a plain C++ transcription written from the paper's round function
both produce it, and it is the vector the Random123 distribution lists for philox4x32 with ten rounds."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
KAT_ZERO = (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)
FRAME_WORD = 0xFFFFFFFF          # counter word 3 of a frame's own draw (no expert group e / 4 reaches it)
MAX_E = 16


def philox4x32_10(counter, key):
    """counter: four arrays (or ints) of 32-bit words, key: two -> four uint32 arrays of the broadcast shape."""
    c = [np.asarray(x, dtype=np.uint64) & np.uint64(0xFFFFFFFF) for x in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    mask, sh = np.uint64(0xFFFFFFFF), np.uint64(32)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]      # 32 x 32 -> 64 bits: no overflow in uint64
        hi0, lo0, hi1, lo1 = p0 >> sh, p0 & mask, p1 >> sh, p1 & mask
        c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return tuple(x.astype(np.uint32) for x in c)


def uniform24(x):
    """(x >> 8) * 2^-24: a uniform in [0, 1) on a 2^-24 grid, exact in fp32"""
    return (np.asarray(x, dtype=np.uint32) >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)


def keep_scale(rate):
    """fl(1 / (1 - rate)) in fp32: what a kept frame / pair is scaled by"""
    return np.float32(1.0) / (np.float32(1.0) - np.float32(rate))


def draws(seed, calls, S, E):
    """The uniforms behind one call: (ua (S,), ub (S, E)) fp32."""
    assert 1 <= E <= MAX_E and S >= 1
    key = (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    c0, c1 = calls & 0xFFFFFFFF, (calls >> 32) & 0xFFFFFFFF
    s = np.arange(S, dtype=np.uint64)
    G = (E + 3) // 4
    lanes = philox4x32_10((c0, c1, s[:, None], np.arange(G, dtype=np.uint64)[None, :]), key)      # each (S, G)
    ub = uniform24(np.stack(lanes, axis=-1).reshape(S, 4 * G)[:, :E])                              # lane e % 4 of group e / 4
    ua = uniform24(philox4x32_10((c0, c1, s, FRAME_WORD), key)[0])
    return ua, ub


def mix_scale(seed, calls, S, E, p, q):
    """m[s, e] = a[s] b[s, e] in fp32: a = 0 where ua < p else fl(1 / (1 - p)); b = 0 where ub < q else fl(1 / (1 - q))."""
    ua, ub = draws(seed, calls, S, E)
    a = np.where(ua < np.float32(p), np.float32(0), keep_scale(p)).astype(np.float32)
    b = np.where(ub < np.float32(q), np.float32(0), keep_scale(q)).astype(np.float32)
    return (a[:, None] * b).astype(np.float32)


# ---- the masked mixture itself, composed from the oracle's pieces (as tests/topk_ref.py composes the top-k mixture) ----------------
def masked_forward(P, B, X, Y, cfg, m, k=None, renorm=True, training=True, noise=None):
    """out = sum_e m[s, e] w[s, e] expert_e(x)[s] with w the dense softmax (k None or E) or the top-k weights: the multiplier comes
    BEHIND top-k.  Any floating dtype (the tensors decide) -> dict(out, probs, w, experts (E, S, N, C))."""
    import torch
    import torch.nn.functional as F
    from oracle import avmoe_oracle as O
    from tests.topk_ref import topk_weights
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
    w = topk_weights(probs, k, renorm)
    ex = [O.expert_forward(P, B, pre, X, Yf, cfg, j < cfg.E_m, training, None, None) for j, pre in enumerate(cfg.expert_prefixes())]
    mw = m.to(w.dtype) * w
    out = torch.zeros_like(X)
    for j, o in enumerate(ex):
        out = out + mw[:, j].reshape(-1, 1, 1) * o
    return dict(out=out, probs=probs, w=w, experts=torch.stack(ex))


def hand_mask(S, E, p=0.25, q=0.5):
    """A hand-made multiplier with every case in it: frame 0 dropped whole (a = 0), frame 1 kept but with every expert dropped, the other
    frames a fixed pattern of kept / dropped pairs; kept values fl(fl(1 / (1 - p)) fl(1 / (1 - q))).  -> (S, E) fp32 numpy"""
    keep = np.float32(keep_scale(p) * keep_scale(q))
    m = np.zeros((S, E), dtype=np.float32)
    for s in range(2, S):
        for e in range(E):
            if (s * 7 + e * 3) % 4 != 0 or e == s % E:
                m[s, e] = keep
    return m
