"""Oracle gradients of a loss that includes the routing probabilities:  <out, dO> + <probs, dP> + w * lb  (any of the three terms may
be absent), by autograd through oracle.avmoe_oracle.moe_forward.  Shared by the host and GPU checks of avmoe_moe_backward_ex."""
import torch

from oracle import avmoe_oracle as O


def oracle_grads(cfg, P, B, X, Y, dO, dP, lb_weight, training, noise=None, mha_keep=None):
    """-> {'X', 'Y', every parameter key: gradient}; dO / dP None = that term absent."""
    Pg = {k: v.detach().clone().requires_grad_(True) for k, v in P.items()}
    Xg = X.detach().clone().requires_grad_(True)
    Yg = Y.detach().clone().requires_grad_(True)
    fwd = O.moe_forward(Pg, B, Xg, Yg, cfg, training=training, noise=noise, update_buffers=False, mha_keep=mha_keep)
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
    return {k: (g.detach() if g is not None else torch.zeros_like(ref[k])) for k, g in zip(keys, gs)}


def cases(cfg, S, seed):
    """(label, dO?, dP, lb_weight) of the checks: every term together, probs alone, the load-balancing loss alone (where the site has one)."""
    g = torch.Generator().manual_seed(seed)
    dP = torch.randn(S, cfg.E, generator=g)
    out = [("full", True, dP, 0.7 if cfg.lb_loss else 0.0), ("probs_only", False, dP, 0.0)]
    if cfg.lb_loss:
        out.append(("lb_only", False, None, 1.3))
        out.append(("probs_lb", False, dP, 0.6))
    return out


def expert_keys(grads):
    return [k for k in grads if k.startswith(("multimodal_experts.", "singlemodal_experts."))]


def assert_close(got, ref, rtol, floor_frac=1e-3, what=""):
    """max |got - ref| <= rtol * max(max|ref|, floor_frac * the largest gradient of the set), per tensor.  The tiny tensors (scalar gates,
    the E-element router bias: each number one sum over every token of terms of both signs, where a relative error measures the
    cancellation) are judged together as one vector."""
    tiny = [k for k, v in ref.items() if v.numel() <= 16]
    pairs = {k: (got[k].detach().double().cpu(), r.double().cpu()) for k, r in ref.items() if k not in tiny}
    if tiny:
        pairs["<tiny tensors>"] = (torch.cat([got[k].detach().double().cpu().reshape(-1) for k in tiny]),
                                   torch.cat([ref[k].double().cpu().reshape(-1) for k in tiny]))
    gmax = max(float(r.abs().max()) for _, r in pairs.values())
    bad = {}
    for k, (g, r) in pairs.items():
        e = float((g - r).abs().max())
        s = float(r.abs().max())
        if not e <= rtol * max(s, floor_frac * gmax):
            bad[k] = (e, s)
    assert not bad, f"{what}: gradient mismatch (err, scale): {bad}"
