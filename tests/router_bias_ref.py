"""Reference of aux-loss-free expert balancing (include/avmoe.h at avmoe_moe_forward_bias / avmoe_router_bias_update): the selection on
p + b, the weights from the unbiased p, the selection counts, the bias update and the recurrence of forward + update -- in fp32 torch /
numpy, written from the header's formulas.  `topk_forward(..., sel=)` / `topk_grads(..., sel=)` of tests/topk_ref.py with
sel = select_mask(p, b, k) are the reference of the site call itself.  The check_* functions raise AssertionError; tests/test_router_bias_ref.py
shows that each of them catches the fault it is there for."""
import numpy as np
import torch
import torch.nn.functional as F

from tests.topk_ref import topk_mask

ROW = 16              # AVMOE_MAX_EXPERTS: the row length of the balancer's bias / counts tables


def router_probs(P, X, Y, noise=None):
    """(S, E) fp32: the dense softmax of the site's router (the remap and router lines of oracle.avmoe_oracle.moe_forward)."""
    Wc = P["conv_adapter.weight"][:, :, 0, 0]
    Yt = torch.einsum("nm,smc->snc", Wc, Y) + P["conv_adapter.bias"][None, :, None]
    Yf = Yt @ P["fc.weight"].t() + P["fc.bias"]
    rin = torch.cat([X.mean(dim=1), Yf.mean(dim=1)], dim=-1)
    h = F.relu(rin @ P["router.0.weight"].t() + P["router.0.bias"])
    h = F.relu(h @ P["router.2.weight"].t() + P["router.2.bias"])
    logits = h @ P["router.4.weight"].t() + P["router.4.bias"]
    return F.softmax(logits if noise is None else logits + noise, dim=-1)


def select_mask(p, b, k):
    """(S, E) 0 / 1 fp32: the k experts of every frame with the highest score p + b -- ONE fp32 addition -- higher score first, equal
    scores in expert order (topk_mask's rule on the scores)."""
    p = p.detach().to(torch.float32)
    return topk_mask(p + torch.as_tensor(b, dtype=torch.float32, device=p.device)[None, :], k)


def weights(p, b, k, renorm):
    """(S, E) fp32 mixture weights: m p / sum(m p) or m p with m = select_mask -- the bias is in the selection alone."""
    p = p.detach().to(torch.float32)
    w = select_mask(p, b, k) * p
    return w / w.sum(-1, keepdim=True) if renorm else w


def counts_of(mask):
    """(E,) fp32: the number of frames that selected each expert (integers)."""
    return mask.to(torch.float32).sum(0)


def update(bias, counts, E, rate):
    """avmoe_router_bias_update on (n, 16) tables -> (bias, counts) after the call, as new fp32 numpy arrays.  Per row i with E_i in
    [1, 16]: tot = sum of the first E_i counts in expert order; tot == 0: untouched; else d_e = tot - E_i c_e, bias_e += rate (d_e > 0) /
    -= rate (d_e < 0) / nothing, c_e = 0.  Columns >= E_i are copied through untouched, whatever they hold."""
    bias = np.array(bias, dtype=np.float32, copy=True).reshape(-1, ROW)
    counts = np.array(counts, dtype=np.float32, copy=True).reshape(-1, ROW)
    r = np.float32(rate)
    for i, e in enumerate(E):
        e = int(e)
        if not 1 <= e <= ROW:
            continue
        tot = np.float32(0.0)
        for f in range(e):
            tot = np.float32(tot + counts[i, f])
        if tot == 0:
            continue
        for f in range(e):
            d = np.float32(tot - np.float32(np.float32(e) * counts[i, f]))
            if d > 0:
                bias[i, f] = np.float32(bias[i, f] + r)
            elif d < 0:
                bias[i, f] = np.float32(bias[i, f] - r)
            counts[i, f] = 0.0
    return bias, counts


def trajectory(p_rounds, E, k, rate, b0=None):
    """The recurrence of `forward, step()` on ONE site whose softmax in round t is p_rounds[t] ((S, E) fp32): returns
    (bias_after [T, E] fp32 numpy, load [T, E] float64 numpy) -- the bias after every round's update and every round's share of the
    selections, each round selecting with the bias the round BEFORE left."""
    b = np.zeros((1, ROW), np.float32)
    if b0 is not None:
        b[0, :E] = np.asarray(b0, np.float32)
    after, loads = [], []
    for p in p_rounds:
        m = select_mask(p, torch.from_numpy(b[0, :E].copy()), k)
        c = np.zeros((1, ROW), np.float32)
        c[0, :E] = counts_of(m).cpu().numpy()
        loads.append(c[0, :E].astype(np.float64) / (p.shape[0] * k))
        b, _ = update(b, c, [E], rate)
        after.append(b[0, :E].copy())
    return np.stack(after), np.stack(loads)


def spread(load):
    return float(load.max() - load.min())


# ---- checks (what the GPU tests assert, stated once) -------------------------------------------------------------------------------
def check_weights(w, p, b, k, renorm):
    """w (S, E): nonzero exactly on select_mask(p, b, k), for EVERY frame, and equal to the unbiased weights there (renorm: 1e-6
    relative -- one division; otherwise bit-equal to p)."""
    w, p = w.detach().cpu().to(torch.float32), p.detach().cpu().to(torch.float32)
    m = select_mask(p, torch.as_tensor(b).cpu(), k)
    assert torch.equal((w != 0).to(torch.float32), m), "the kept experts are not the k highest p + b"
    ref = weights(p, torch.as_tensor(b).cpu(), k, renorm)
    if renorm:
        assert float((w - ref).abs().max()) <= 1e-6 * float(ref.abs().max()), "weights are not m p / sum(m p) of the unbiased p"
    else:
        assert torch.equal(w, ref), "weights are not m p of the unbiased p"


def check_update(bias0, counts0, E, rate, bias1, counts1):
    """(bias1, counts1) are, bit for bit, update(bias0, counts0): NaN sentinels in columns >= E and untouched tot == 0 rows included."""
    rb, rc = update(bias0, counts0, E, rate)
    got_b, got_c = np.asarray(bias1, np.float32).reshape(-1, ROW), np.asarray(counts1, np.float32).reshape(-1, ROW)
    assert np.array_equal(got_b.view(np.uint32), rb.view(np.uint32)), "bias after the update differs from the reference"
    assert np.array_equal(got_c.view(np.uint32), rc.view(np.uint32)), "counts after the update differ from the reference"


# ---- the fixtures of the selection and trajectory checks (shared by the CPU pre-checks and the GPU tests) --------------------------
def selection_case(which):
    """(cfg, S, P, B, X, Y, noise, b0) of the exact-selection check.  'tile_fast': the tile_fast family's configuration (fp32) at
    S = 300 frames, so that the one-block count loop strides past 256; 'e16': E_m = E_s = 8 (AVMOE_MAX_EXPERTS) at S = 5.  A freshly
    initialised router hardly moves with the frame (its probabilities spread by ~3e-4), so the frames get the AVS logit noise at scale 1;
    the bias scales (0.2 / 0.05) are chosen on the ORACLE's router (tests/test_router_bias_ref.py checks them there) so that the biased
    selection differs from the unbiased one in well over a quarter of the frames and agrees in some."""
    from oracle import avmoe_oracle as O
    from tests.topk_families import family_config
    if which == "tile_fast":
        cfg, S, scale = family_config("tile_fast")[0], 300, 0.2
    else:
        cfg = O.AdapterConfig(Cx=64, Nx=40, Cy=48, Ny=24, reduction=4, groups=2, K=8, variant="avs", E_m=8, E_s=8, lb_loss=True)
        S, scale = 5, 0.05
    P, B = O.init_params(cfg, seed=3)
    g = torch.Generator().manual_seed(17)
    X = 0.3 * torch.randn(S, cfg.Nx, cfg.Cx, generator=g)
    Y = 0.3 * torch.randn(S, cfg.Ny, cfg.Cy, generator=g)
    noise = torch.randn(S, cfg.E, generator=g)
    b0 = scale * torch.randn(cfg.E, generator=torch.Generator().manual_seed(6))
    return cfg, S, P, B, X, Y, noise, b0


def with_tie(p, b, k, frame=0):
    """b with ONE entry changed so that, in `frame`, the experts at ranks k - 1 and k of the biased order (the last kept one, a, and the
    first dropped one, c) have EXACTLY equal fp32 scores p + b: the tie rule (expert order) then decides which of the two is kept.
    Returns (b', a, c).  c's bias is raised to t - p_c with t = fl(p_a + b_a), then stepped by single ulps until fl(p_c + b_c) == t."""
    p = p.detach().cpu().to(torch.float32)
    b = torch.as_tensor(b, dtype=torch.float32).clone()
    sc = (p[frame] + b).numpy()
    order = sorted(range(len(sc)), key=lambda e: (-sc[e], e))
    a, c = order[k - 1], order[k]
    t, pc = np.float32(sc[a]), np.float32(p[frame, c].item())
    bc = np.float32(t - pc)
    for _ in range(64):
        s = np.float32(pc + bc)
        if s == t:
            break
        bc = np.nextafter(bc, np.float32(np.inf if s < t else -np.inf), dtype=np.float32)
    assert np.float32(pc + bc) == t, "no fp32 bias gives an exact tie here"
    b[c] = float(bc)
    return b, a, c


def changed_frames(p, b, k):
    """(S,) bool: the frames whose biased selection differs from the unbiased one."""
    p = p.detach().cpu().to(torch.float32)
    return (select_mask(p, b, k) != topk_mask(p, k)).any(dim=1)


TRAJ_ROUNDS, TRAJ_RATE, TRAJ_K, TRAJ_SKEW = 50, 0.01, 2, 1.0


def trajectory_case():
    """(cfg, S, P, B, X, Y, noise) of the trajectory check: a small AVS site with fixed parameters whose router is deliberately skewed --
    TRAJ_SKEW added to row 0 of router.4.bias, so expert 0 is selected far too often -- and frames spread out by logit noise.  With rate
    TRAJ_RATE the reference recurrence alone brings the spread max_e load - min_e load of round TRAJ_ROUNDS below that of round 1
    (tests/test_router_bias_ref.py checks this on the oracle's router): a property of the reference, not a tuned number."""
    from oracle import avmoe_oracle as O
    cfg = O.AdapterConfig(Cx=64, Nx=72, Cy=48, Ny=40, reduction=4, groups=2, K=32, variant="avs", E_m=2, E_s=2, lb_loss=True)
    S = 64
    P, B = O.init_params(cfg, seed=11)
    P = dict(P)
    bias = P["router.4.bias"].clone()
    bias[0] += TRAJ_SKEW
    P["router.4.bias"] = bias
    g = torch.Generator().manual_seed(29)
    X = 0.3 * torch.randn(S, cfg.Nx, cfg.Cx, generator=g)
    Y = 0.3 * torch.randn(S, cfg.Ny, cfg.Cy, generator=g)
    noise = torch.randn(S, cfg.E, generator=g)
    return cfg, S, P, B, X, Y, noise
