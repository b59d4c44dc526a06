"""Reference of the top-k gated mixture (include/avmoe.h at avmoe_moe_forward_topk), composed from the oracle's pieces: the remap and
router lines of oracle.avmoe_oracle.moe_forward, its expert_forward and load_balancing_loss -- with the top-k weights in the mixture
line.  Differentiated by autograd.  Shared by the host and GPU checks of the top-k gating."""
import torch
import torch.nn.functional as F

from oracle import avmoe_oracle as O


def topk_mask(probs, k):
    """(S, E) float 0 / 1: the k most probable experts of every frame -- higher probability first, equal probabilities in expert order
    (the order of avmoe_router_topk).  No gradient."""
    p = probs.detach()
    E = p.shape[-1]
    e = torch.arange(E, device=p.device)
    before = (p[:, None, :] > p[:, :, None]) | ((p[:, None, :] == p[:, :, None]) & (e[None, None, :] < e[None, :, None]))
    rank = before.sum(-1)                               # rank[s, e] = experts that come before e
    return (rank < k).to(probs.dtype)


def topk_weights(probs, k, renorm, sel=None):
    """The mixture weights w of the top-k gating (k None or E: the dense softmax itself).  sel: an (S, E) 0 / 1 selection to use instead
    of the one made from `probs` (a bf16 evaluation of the reference then keeps the experts the checked run kept)."""
    if k is None or k >= probs.shape[-1]:
        return probs
    m = topk_mask(probs, k) if sel is None else sel.to(probs.dtype)
    w = m * probs
    return w / w.sum(-1, keepdim=True) if renorm else w


def topk_forward(P, B, X, Y, cfg, k, renorm=True, training=True, noise=None, update_buffers=True, mha_keep=None, sel=None):
    """oracle.moe_forward with the mixture weights of the top-k gating -> dict(out, probs (dense), idx, lb (on the dense softmax), w,
    new_buffers)."""
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
    idx = torch.argmax(probs, dim=-1)
    w = topk_weights(probs, k, renorm, sel)
    new_buffers = {} if (training and update_buffers and cfg.use_bn) else None
    out = torch.zeros_like(X)
    for j, pre in enumerate(cfg.expert_prefixes()):     # every expert on every frame, as in the dense site
        o = O.expert_forward(P, B, pre, X, Yf, cfg, j < cfg.E_m, training, new_buffers, mha_keep)
        out = out + w[:, j].reshape(-1, 1, 1) * o
    lb = O.load_balancing_loss(probs) if cfg.lb_loss else torch.zeros((), dtype=X.dtype)
    if new_buffers is not None:
        for pre in cfg.expert_prefixes():
            for bn in ("bn1", "bn2"):
                new_buffers[f"{pre}.{bn}.num_batches_tracked"] = B[f"{pre}.{bn}.num_batches_tracked"] + 1
    return dict(out=out, probs=probs, idx=idx, lb=lb, w=w, new_buffers=new_buffers)


def topk_grads(cfg, P, B, X, Y, dO, dP, lb_weight, training, k, renorm, noise=None, mha_keep=None, sel=None):
    """Gradients of <out, dO> + <probs, dP> + lb_weight * lb of the top-k forward -> {'X', 'Y', parameter key: gradient}; dO / dP None
    = that term absent; sel: see topk_weights."""
    Pg = {kk: v.detach().clone().requires_grad_(True) for kk, v in P.items()}
    Xg = X.detach().clone().requires_grad_(True)
    Yg = Y.detach().clone().requires_grad_(True)
    fwd = topk_forward(Pg, B, Xg, Yg, cfg, k, renorm, training=training, noise=noise, update_buffers=False, mha_keep=mha_keep, sel=sel)
    loss = torch.zeros((), dtype=X.dtype, device=X.device)
    if dO is not None:
        loss = loss + (fwd["out"] * dO).sum()
    if dP is not None:
        loss = loss + (fwd["probs"] * dP).sum()
    if cfg.lb_loss and lb_weight:
        loss = loss + lb_weight * fwd["lb"]
    keys = ["X", "Y"] + list(Pg)
    gs = torch.autograd.grad(loss, [Xg, Yg] + list(Pg.values()), allow_unused=True)
    ref = {"X": Xg, "Y": Yg, **Pg}
    return {kk: (g.detach() if g is not None else torch.zeros_like(ref[kk])) for kk, g in zip(keys, gs)}


def k_values(E):
    """The k of the checks: {1, 2, E} within [1, E]."""
    return sorted({k for k in (1, 2, E) if 1 <= k <= E})
