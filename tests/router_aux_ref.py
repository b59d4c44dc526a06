"""Reference of the router auxiliary losses (include/avmoe.h at avmoe_moe_forward_aux): fp64 torch autograd on
oracle.avmoe_oracle.moe_forward (dense mixture) or tests/topk_ref.topk_forward (top-k mixture).  Neither returns the router logits, so
they are rebuilt inside the autograd graph from what the forward does return -- rin = cat(X.mean(1), Yf.mean(1)), the three router
layers from P, plus the noise -- and z, load and balance are formed from them by their definitions.  Shared by the host and GPU checks.

Inputs (`make_case`): `load` is discrete, so a comparison only means something where no frame's selection is a near tie.  The cases
give every frame its own offset (the router sees token MEANS: without it all frames route alike), scale router.4.weight so that the
logits spread, and walk the seed on the CPU until every frame's gap between its k'-th and (k'+1)-th probability is >= MARGIN in this
fp64 reference.  The tests assert that margin; no frame and no case is left out."""
import torch
import torch.nn.functional as F

from oracle import avmoe_oracle as O
from tests.topk_ref import topk_forward, topk_mask

MARGIN = 1e-4


def k_eff(E, k):
    """k' of the load: k when top-k gating is active (0 < k < E), else 1."""
    return k if (k is not None and 0 < k < E) else 1


def router_logits(P, X, Yf, noise=None):
    rin = torch.cat([X.mean(dim=1), Yf.mean(dim=1)], dim=-1)
    h = F.relu(rin @ P["router.0.weight"].t() + P["router.0.bias"])
    h = F.relu(h @ P["router.2.weight"].t() + P["router.2.bias"])
    logits = h @ P["router.4.weight"].t() + P["router.4.bias"]
    return logits + noise if noise is not None else logits


def remap(P, Y):
    Wc = P["conv_adapter.weight"][:, :, 0, 0]
    Yt = torch.einsum("nm,smc->snc", Wc, Y) + P["conv_adapter.bias"][None, :, None]
    return Yt @ P["fc.weight"].t() + P["fc.bias"]


def aux_of_logits(logits, k):
    """-> dict(z, balance, load (E,), counts (E,) = load * S * k', margin = the smallest gap over the frames, lse, probs)."""
    S, E = logits.shape
    kp = k_eff(E, k)
    lse = torch.logsumexp(logits, dim=-1)
    z = (lse ** 2).mean()
    p = F.softmax(logits, dim=-1)
    counts = topk_mask(p, kp).sum(dim=0)                 # (no gradient: topk_mask detaches)
    load = counts / (S * kp)
    balance = E * (load * p.mean(dim=0)).sum()
    srt = p.detach().sort(dim=-1, descending=True).values
    margin = float((srt[:, kp - 1] - srt[:, kp]).min()) if E > kp else float("inf")
    return dict(z=z, balance=balance, load=load, counts=counts, margin=margin, lse=lse, probs=p)


def _f64(d):
    return {k: (v.double() if v.is_floating_point() else v) for k, v in d.items()}


def aux_reference(cfg, P, B, X, Y, k=None, renorm=True, training=True, noise=None, mha_keep=None,
                  dO=None, dP=None, lb_weight=0.0, g_z=0.0, g_b=0.0, grads=True):
    """fp64 forward values and (grads=True) the gradients of  <out, dO> + <probs, dP> + lb_weight * lb + g_z * z + g_b * balance.
    -> (values: dict(out, probs, idx, lb, z, balance, load, counts, margin), gradients: {'X', 'Y', parameter key: gradient} or None)"""
    Pg = {kk: v.detach().double().clone().requires_grad_(grads) for kk, v in P.items()}
    Bd = _f64(B)
    Xg, Yg = X.detach().double().clone().requires_grad_(grads), Y.detach().double().clone().requires_grad_(grads)
    nz = noise.double() if noise is not None else None
    keep = {kk: v.double() for kk, v in mha_keep.items()} if mha_keep else mha_keep
    topk = k is not None and 0 < k < cfg.E
    if topk:
        fwd = topk_forward(Pg, Bd, Xg, Yg, cfg, k, renorm, training=training, noise=nz, update_buffers=False, mha_keep=keep)
        Yf = remap(Pg, Yg)                                # (topk_forward does not return Yf: the same two lines of the oracle)
    else:
        fwd = O.moe_forward(Pg, Bd, Xg, Yg, cfg, training=training, noise=nz, update_buffers=False, mha_keep=keep)
        Yf = fwd["Yf"]
    a = aux_of_logits(router_logits(Pg, Xg, Yf, nz), k)
    vals = dict(out=fwd["out"].detach(), probs=fwd["probs"].detach(), idx=fwd["idx"], lb=fwd["lb"].detach(), z=a["z"].detach(),
                balance=a["balance"].detach(), load=a["load"].detach(), counts=a["counts"].detach(), margin=a["margin"])
    if not grads:
        return vals, None
    loss = g_z * a["z"] + g_b * a["balance"]
    if dO is not None:
        loss = loss + (fwd["out"] * dO.double()).sum()
    if dP is not None:
        loss = loss + (fwd["probs"] * dP.double()).sum()
    if cfg.lb_loss and lb_weight:
        loss = loss + lb_weight * fwd["lb"]
    keys = ["X", "Y"] + list(Pg)
    gs = torch.autograd.grad(loss, [Xg, Yg] + list(Pg.values()), allow_unused=True)
    ref = {"X": Xg, "Y": Yg, **Pg}
    return vals, {kk: (g.detach() if g is not None else torch.zeros_like(ref[kk])) for kk, g in zip(keys, gs)}


def make_case(cfg, S, k=None, noise=False, seed=0, router_scale=8.0, tries=50, margin=MARGIN, round_bf16=False):
    """Synthetic site of `cfg` with S frames whose selection is clear in the fp64 reference: -> dict(P, B, X, Y, noise, seed, light).
    `light`: z / balance / load / counts / margin of the reference from the remap and router lines alone (no expert runs: what the
    forward checks at many frames need).  round_bf16: X and Y are bf16 values (a bf16 site sees exactly them).
    Deterministic (CPU generator); raises if no seed in [seed, seed + tries) gives the margin."""
    for sd in range(seed, seed + tries):
        P, B = O.init_params(cfg, seed=sd)
        P = dict(P)
        P["router.4.weight"] = P["router.4.weight"] * router_scale
        g = torch.Generator().manual_seed(1000 + sd)
        X = 0.5 * torch.randn(S, cfg.Nx, cfg.Cx, generator=g) + torch.randn(S, 1, cfg.Cx, generator=g)      # + a per-frame offset
        Y = 0.5 * torch.randn(S, cfg.Ny, cfg.Cy, generator=g) + torch.randn(S, 1, cfg.Cy, generator=g)
        nz = 0.5 * torch.randn(S, cfg.E, generator=g) if noise else None                                    # (scaled up like the router)
        if round_bf16:
            X, Y = X.to(torch.bfloat16).float(), Y.to(torch.bfloat16).float()
        with torch.no_grad():
            a = aux_of_logits(router_logits(_f64(P), X.double(), remap(_f64(P), Y.double()), nz.double() if noise else None), k)
        if a["margin"] >= margin:
            return dict(P=P, B=B, X=X, Y=Y, noise=nz, seed=sd, light=a)
    raise RuntimeError(f"make_case: no seed in [{seed}, {seed + tries}) separates every frame's selection by {margin}")


def scalar_close(got, ref, what=""):
    """the bar tests/test_moe_forward_gpu.py applies to lb"""
    got, ref = float(got), float(ref)
    assert abs(got - ref) < 1e-4 * max(1.0, abs(ref)), f"{what}: {got} vs {ref}"


def check_aux(aux, load, vals, S, E, k, what=""):
    """aux = [z, balance] and load against the reference values: the scalars at the lb bar, load * S * k' as exact integers."""
    kp = k_eff(E, k)
    scalar_close(aux[0], vals["z"], what + "/z")
    scalar_close(aux[1], vals["balance"], what + "/balance")
    cnt = load.double().cpu() * (S * kp)
    assert torch.equal(cnt.round().to(torch.int64), vals["counts"].round().to(torch.int64)), f"{what}/load: {cnt} vs {vals['counts']}"
    assert float((cnt - cnt.round()).abs().max()) < 1e-3 and abs(float(load.double().sum()) - 1.0) < 1e-6, f"{what}/load: {cnt}"
