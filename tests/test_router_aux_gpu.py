"""Router auxiliary losses (z-loss, Switch balance loss) on the GPU: avmoe_moe_forward_aux / avmoe_moe_backward_aux against the fp64
reference of tests/router_aux_ref.py, the facade (`router_aux`, `last_router_aux`, `router_aux_total`) and AdapterPair.

Shapes: small sites like those of tests/test_adapters_gpu.py.  What the new code can get wrong: S = 1, 3 and 300 frames (300 is more
than the one-block reduction has threads and no multiple of its stride), E = 2, 4 and 8 experts, and an exact tie.
Bars (read from existing tests): fp32 gradients router_grad_util.assert_close at rtol 1e-3 (test_backward_ex_fp32_matches_oracle);
bf16 sites a relative norm of 1e-2 per tensor (test_router_only_backward_bf16); z, balance and lb 1e-4 * max(1, |ref|)
(tests/test_moe_forward_gpu.py); load * S * k' exact integers."""
import copy
import ctypes as C

import pytest
import torch

from avmoe_amd import _capi as capi
from avmoe_amd import _capi_moe as cm
from oracle import avmoe_oracle as O
from tests.moe_gpu_util import MoeRun
from tests.router_grad_util import assert_close, expert_keys
from tests.router_aux_ref import MARGIN, aux_reference, check_aux, k_eff, make_case, scalar_close
from tests.test_adapters_api import build_module

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _cfg(E_m=2, E_s=2, lb=True):
    return O.AdapterConfig(Cx=64, Nx=150, Cy=48, Ny=80, E_m=E_m, E_s=E_s, reduction=4, groups=2, K=8, variant="avs", lb_loss=lb)


MODES = {"dense": (0, True), "k2_renorm": (2, True), "k1_switch": (1, False)}
_CASES = {}


def _case(E_m=2, E_s=2, S=4, mode="dense", noise=True, **kw):
    """one reference case per key, made once and shared (never modified)"""
    key = (E_m, E_s, S, mode, noise, tuple(sorted(kw.items())))
    if key not in _CASES:
        _CASES[key] = (_cfg(E_m, E_s), make_case(_cfg(E_m, E_s), S, MODES[mode][0], noise=noise, seed=11, **kw))
    return _CASES[key]


class AuxRun(MoeRun):
    def __init__(self, cfg, case, bf16=False):
        super().__init__(cfg, case["P"], case["B"], case["X"], case["Y"], bf16=bf16, training=True, noise=case["noise"])

    def forward_aux(self, k, renorm, aux=True, entry="aux"):
        """entry 'aux': avmoe_moe_forward_aux (aux False: with aux == NULL); 'old': avmoe_moe_forward / _forward_topk.  Each call starts
        from the buffers of the case (a training forward advances the BatchNorm statistics)."""
        L, E = self.L, self.cfg.E
        bufs = {kk: v.clone() for kk, v in self.buffers.items()}
        ptrs = cm.make_ptrs({**self.params, **bufs, **self.keep}, self.cfg.E_m, self.cfg.E_s)
        out, probs = torch.full_like(self.X, float("nan")), torch.full((self.S, E), float("nan"), device=DEV)
        idx, lb = torch.full((self.S,), -1, device=DEV, dtype=torch.int64), torch.full((1,), float("nan"), device=DEV)
        ax, load = torch.full((2,), float("nan"), device=DEV), torch.full((E,), float("nan"), device=DEV)
        head = (C.byref(self.desc), self.X.data_ptr(), self.Y.data_ptr(), C.byref(ptrs), self.noise.data_ptr() if self.noise is not None else None)
        outs = (out.data_ptr(), probs.data_ptr(), idx.data_ptr(), lb.data_ptr())
        ws = (self.saved.data_ptr(), self.scratch.data_ptr(), torch.cuda.current_stream().cuda_stream)
        if entry == "aux":
            st = L.avmoe_moe_forward_aux(*head, k, int(renorm), *outs, ax.data_ptr() if aux else None, load.data_ptr() if aux else None, *ws)
        elif k == 0:
            st = L.avmoe_moe_forward(*head, *outs, *ws)
        else:
            st = L.avmoe_moe_forward_topk(*head, k, int(renorm), *outs, *ws)
        capi.check(st, "forward")
        torch.cuda.synchronize()
        assert self.guards_intact()
        return dict(out=out.float().cpu(), probs=probs.cpu(), idx=idx.cpu(), lb=lb.cpu(), aux=ax.cpu(), load=load.cpu())

    def backward_aux(self, dO, dP, w, ag, parts=(0,), entry="aux"):
        """after a forward: avmoe_moe_backward_aux ('ex': avmoe_moe_backward_ex) -> {'X', 'Y', parameter key: gradient} on the CPU;
        parts: the sections, run one after the other into the same outputs"""
        L = self.L
        dOd = dO.to(DEV, self.tdt).contiguous() if dO is not None else None
        dPd = dP.to(DEV, torch.float32).contiguous() if dP is not None else None
        agd = torch.tensor([float(ag[0]), float(ag[1])], device=DEV) if ag is not None else None
        dX, dY = torch.full_like(self.X, float("nan")), torch.full_like(self.Y, float("nan"))
        grads = {kk: torch.full_like(v, float("nan")) for kk, v in self.params.items()}
        gptrs = cm.make_ptrs(grads, self.cfg.E_m, self.cfg.E_s)
        lbw = torch.full((1,), float(w), device=DEV)
        for p in parts:
            head = (C.byref(self.desc), self.X.data_ptr(), self.Y.data_ptr(), C.byref(self.ptrs), dOd.data_ptr() if dOd is not None else None,
                    dPd.data_ptr() if dPd is not None else None, lbw.data_ptr())
            tail = (self.saved.data_ptr(), self.scratch.data_ptr(), dX.data_ptr(), dY.data_ptr(), C.byref(gptrs), p,
                    torch.cuda.current_stream().cuda_stream)
            if entry == "aux":
                st = L.avmoe_moe_backward_aux(*head, agd.data_ptr() if agd is not None else None, *tail)
            else:
                st = L.avmoe_moe_backward_ex(*head, *tail)
            capi.check(st, "backward")
        torch.cuda.synchronize()
        assert self.guards_intact()
        g = {kk: v.cpu() for kk, v in grads.items()}
        g["X"], g["Y"] = dX.float().cpu(), dY.float().cpu()
        return g


# ---- C ABI forward --------------------------------------------------------------------------------
FWD = [(2, 2, 4, "dense"), (2, 2, 4, "k2_renorm"), (2, 2, 4, "k1_switch"), (2, 2, 1, "k1_switch"), (2, 2, 3, "k2_renorm"),
       (2, 2, 300, "dense"), (2, 2, 300, "k2_renorm"), (1, 1, 5, "k1_switch"), (1, 1, 5, "k2_renorm"), (4, 4, 7, "k2_renorm")]


@pytest.mark.parametrize("E_m,E_s,S,mode", FWD)
def test_forward_aux_matches_reference_and_leaves_the_outputs_alone(E_m, E_s, S, mode):
    """(sites with the load-balancing loss and logit noise; E = 2 with k = 2 is k == E: the dense mixture, k' = 1)"""
    cfg, case = _case(E_m, E_s, S, mode)
    k, renorm = MODES[mode]
    ref = case["light"]
    assert ref["margin"] >= MARGIN
    run = AuxRun(cfg, case)
    got = run.forward_aux(k, renorm)
    check_aux(got["aux"], got["load"], ref, S, cfg.E, k, f"{mode}/S={S}/E={cfg.E}")
    lb_ref = -torch.log(ref["probs"].mean(dim=0)).sum()
    scalar_close(got["lb"], lb_ref, "lb")
    again = run.forward_aux(k, renorm)                                   # repeat: bit for bit
    null = run.forward_aux(k, renorm, aux=False)
    old = run.forward_aux(0 if k == cfg.E else k, renorm, entry="old")
    assert torch.equal(got["aux"], again["aux"]) and torch.equal(got["load"], again["load"])
    assert bool(torch.isnan(null["aux"]).all()) and bool(torch.isnan(null["load"]).all())
    for key in ("out", "probs", "idx", "lb"):
        assert torch.equal(got[key], old[key]) and torch.equal(null[key], old[key]), key


def test_exact_tie_follows_expert_order_like_router_topk():
    """router.4.weight zeroed, equal biases: every probability is exactly 1 / E; load must be the choice of avmoe_router_topk."""
    cfg, case = _case(2, 2, 5, "dense", noise=False)
    case = dict(case, P=dict(case["P"]))
    case["P"]["router.4.weight"] = torch.zeros_like(case["P"]["router.4.weight"])
    case["P"]["router.4.bias"] = torch.full_like(case["P"]["router.4.bias"], 0.25)
    run = AuxRun(cfg, case)
    for k in (0, 2, 3):
        got = run.forward_aux(k, True)
        assert bool((got["probs"] == got["probs"][0, 0]).all())
        kp = k_eff(cfg.E, k)
        sel = torch.empty(5, kp, device=DEV, dtype=torch.int64)
        pd = got["probs"].to(DEV)
        capi.check(run.L.avmoe_router_topk(pd.data_ptr(), 5, cfg.E, kp, sel.data_ptr(), None), "topk")
        torch.cuda.synchronize()
        want = torch.bincount(sel.cpu().reshape(-1), minlength=cfg.E).float() / (5 * kp)
        assert torch.equal(got["load"], want) and torch.equal(want, torch.tensor([1.0 / kp] * kp + [0.0] * (cfg.E - kp)))
        scalar_close(got["aux"][1], 1.0, "balance at a uniform router")


# ---- C ABI backward -------------------------------------------------------------------------------
# (label, dOut?, dprobs?, lb weight, [g_z, g_balance])
BWD = [("full", True, True, 0.7, (0.9, -1.1)), ("aux_only", False, False, 0.0, (0.9, -1.1)), ("z_only", False, False, 0.0, (1.3, 0.0)),
       ("balance_only", False, False, 0.0, (0.0, 0.8))]


@pytest.mark.parametrize("mode", list(MODES))
def test_backward_aux_fp32_matches_reference(mode):
    cfg, case = _case(2, 2, 4, mode)
    k, renorm = MODES[mode]
    g = torch.Generator().manual_seed(23)
    dO, dP = torch.randn(case["X"].shape, generator=g), torch.randn(4, cfg.E, generator=g)
    run = AuxRun(cfg, case)
    run.forward_aux(k, renorm)
    for label, with_out, with_p, w, ag in BWD:
        vals, ref = aux_reference(cfg, case["P"], case["B"], case["X"], case["Y"], k, renorm, noise=case["noise"],
                                  dO=dO if with_out else None, dP=dP if with_p else None, lb_weight=w, g_z=ag[0], g_b=ag[1])
        assert vals["margin"] >= MARGIN
        got = run.backward_aux(dO if with_out else None, dP if with_p else None, w, ag)
        assert_close(got, ref, rtol=1e-3, what=f"{mode}/{label}")
        assert float(ref["router.0.weight"].abs().max()) > 0.0
        if not with_out:
            assert all(float(got[kk].abs().max()) == 0.0 for kk in expert_keys(got)), "expert gradients must be exactly 0 without dOut"
        again = run.backward_aux(dO if with_out else None, dP if with_p else None, w, ag)      # repeat: bit for bit
        for kk, v in got.items():
            assert torch.equal(v, again[kk]), (label, kk)


@pytest.mark.parametrize("S,mode", [(1, "k1_switch"), (3, "k2_renorm")])
def test_backward_aux_few_frames(S, mode):
    cfg, case = _case(2, 2, S, mode)
    k, renorm = MODES[mode]
    run = AuxRun(cfg, case)
    run.forward_aux(k, renorm)
    vals, ref = aux_reference(cfg, case["P"], case["B"], case["X"], case["Y"], k, renorm, noise=case["noise"], g_z=0.9, g_b=-1.1)
    assert vals["margin"] >= MARGIN
    assert_close(run.backward_aux(None, None, 0.0, (0.9, -1.1)), ref, rtol=1e-3, what=f"S={S}")


def test_backward_aux_sections_equal_the_whole_and_null_is_backward_ex():
    cfg, case = _case(2, 2, 4, "k2_renorm")
    g = torch.Generator().manual_seed(29)
    dO, dP = torch.randn(case["X"].shape, generator=g), torch.randn(4, cfg.E, generator=g)
    run = AuxRun(cfg, case)
    run.forward_aux(2, True)
    whole = run.backward_aux(dO, dP, 0.7, (0.9, -1.1))
    parts = run.backward_aux(dO, dP, 0.7, (0.9, -1.1), parts=(1, 2, 4))
    for kk, v in whole.items():
        assert torch.equal(v, parts[kk]), kk
    ex = run.backward_aux(dO, dP, 0.7, None, entry="ex")
    null = run.backward_aux(dO, dP, 0.7, None)
    zero = run.backward_aux(dO, dP, 0.7, (0.0, 0.0))
    for kk, v in ex.items():
        assert torch.equal(v, null[kk]), kk
        assert not kk.startswith("router") or float((v - whole[kk]).abs().max()) > 0.0, kk      # (the terms do change the router's gradients)
    assert_close(zero, {kk: v.double() for kk, v in ex.items()}, rtol=1e-6, what="zero aux_grad")


def test_aux_only_backward_bf16():
    """bf16 tokens, the router-only path: against the fp64 reference on the bf16-rounded inputs.  The frames' selections are separated
    by 5e-2 here: the router sees means of bf16 products (2^-8 relative), not the reference's fp64 ones."""
    cfg, case = _case(2, 2, 4, "k2_renorm", margin=5e-2, round_bf16=True)
    run = AuxRun(cfg, case, bf16=True)
    got = run.forward_aux(2, True)
    vals, ref = aux_reference(cfg, case["P"], case["B"], case["X"], case["Y"], 2, True, noise=case["noise"], g_z=0.9, g_b=-1.1)
    assert vals["margin"] >= 5e-2
    assert torch.equal((got["load"].double() * 8).round().long(), vals["counts"].round().long())
    grads = run.backward_aux(None, None, 0.0, (0.9, -1.1))
    for kk, r in ref.items():
        if float(r.norm()) == 0.0:
            assert float(grads[kk].abs().max()) == 0.0, kk
            continue
        rel = float((grads[kk].double() - r).norm() / r.norm())
        assert rel <= 1e-2, (kk, rel)


# ---- module level -----------------------------------------------------------------------------------
def _module(cfg, case, **attrs):
    m = build_module("avs", cfg).to(DEV)
    m.load_state_dict({**case["P"], **case["B"]}, strict=True)
    m.train(True)
    for kk, v in attrs.items():
        setattr(m, kk, v)
    return m


def _module_grads(m, X, Y):
    g = {"X": X.grad.float().cpu(), "Y": Y.grad.float().cpu()}
    for kk, v in m.named_parameters():
        g[kk] = v.grad.cpu() if v.grad is not None else torch.zeros_like(v).cpu()
    return g


def _prof_families(fn):
    L = capi.lib()
    torch.cuda.synchronize()
    L.avmoe_prof_reset()
    L.avmoe_prof_enable(1)
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        L.avmoe_prof_enable(0)
    rep = capi.prof_report()
    L.avmoe_prof_reset()
    return {r["name"]: r["calls"] for r in rep}


def _site_call(m, X, Y):
    return m(X.permute(0, 2, 1).unsqueeze(-1), Y.permute(0, 2, 1).unsqueeze(-1), is_training=False)


@pytest.mark.parametrize("mode", ["dense", "k2_renorm"])
def test_module_task_plus_aux_matches_reference(mode):
    from avmoe_amd.train import router_aux_total
    cfg, case = _case(2, 2, 4, mode, noise=False)
    k, renorm = MODES[mode]
    m = _module(cfg, case, router_aux=True, router_top_k=k or None, router_top_k_renorm=renorm)
    dO = torch.randn(case["X"].shape, generator=torch.Generator().manual_seed(31))
    vals, ref = aux_reference(cfg, case["P"], case["B"], case["X"], case["Y"], k, renorm, dO=dO, g_z=0.03, g_b=0.4)
    assert vals["margin"] >= MARGIN
    X, Y = case["X"].to(DEV).requires_grad_(True), case["Y"].to(DEV).requires_grad_(True)
    out = _site_call(m, X, Y)[0]
    aux = m.last_router_aux
    assert aux.z_loss.shape == () and aux.balance_loss.shape == () and aux.z_loss.dtype == torch.float32
    assert aux.z_loss.grad_fn is not None and aux.balance_loss.grad_fn is not None and not aux.load.requires_grad
    check_aux(torch.stack([aux.z_loss, aux.balance_loss]).detach().cpu(), aux.load.cpu(), vals, 4, cfg.E, k, mode)
    loss = (out.squeeze(-1).permute(0, 2, 1) * dO.to(DEV)).sum() + router_aux_total([m], 0.03, 0.4)
    loss.backward()
    assert_close(_module_grads(m, X, Y), ref, rtol=1e-3, what=mode)
    m.router_aux = False                                         # off again: the next forward clears the results
    _site_call(m, X.detach(), Y.detach())
    assert m.last_router_aux is None


def test_aux_total_alone_takes_the_router_only_backward():
    from avmoe_amd.train import router_aux_total
    cfg, case = _case(2, 2, 4, "k2_renorm", noise=False)
    m = _module(cfg, case, router_aux=True, router_top_k=2)
    _, ref = aux_reference(cfg, case["P"], case["B"], case["X"], case["Y"], 2, True, g_z=0.5, g_b=2.0)
    X, Y = case["X"].to(DEV).requires_grad_(True), case["Y"].to(DEV).requires_grad_(True)
    _site_call(m, X, Y)
    fams = _prof_families(router_aux_total([m], 0.5, 2.0).backward)
    got = _module_grads(m, X, Y)
    assert_close(got, ref, rtol=1e-3, what="aux total")
    assert all(float(got[kk].abs().max()) == 0.0 for kk in expert_keys(got))
    # the router-only backward: no expert, Gram or token-space family (as tests/test_router_grad_gpu.py asks of a probs-only loss)
    assert {"k_router_bwd", "k_ro_y", "k_ro_dx"} <= set(fams), fams
    other = {kk: v for kk, v in fams.items() if not kk.startswith(("k_router_bwd", "k_ro_"))}
    assert all(kk.startswith("gemm_") and not kk.startswith(("gemm_stream", "gemm_tokpair")) for kk in other), fams
    assert sum(other.values()) <= 4, fams


def _pair_sites():
    kw = dict(E_m=2, E_s=2, groups=2, K=8, variant="avs", lb_loss=True, reduction=4)
    ca, cb = O.AdapterConfig(Cx=64, Nx=72, Cy=48, Ny=40, **kw), O.AdapterConfig(Cx=48, Nx=40, Cy=64, Ny=72, **kw)
    torch.manual_seed(5)
    sa, sb = build_module("avs", ca).to(DEV).train(), build_module("avs", cb).to(DEV).train()
    with torch.no_grad():
        for m in (sa, sb):
            m.router[4].weight.mul_(8.0)
            for kk, p in m.named_parameters():
                if kk.endswith(("gate", "gate_av")):
                    p.fill_(0.3)
    for m in (sa, sb):
        m.router_top_k = 2
    g = torch.Generator().manual_seed(9)
    S = 4
    fa = (0.5 * torch.randn(S, ca.Cx, ca.Nx, 1, generator=g) + torch.randn(S, ca.Cx, 1, 1, generator=g)).to(DEV)
    fv = (0.5 * torch.randn(S, cb.Cx, cb.Nx, 1, generator=g) + torch.randn(S, cb.Cx, 1, 1, generator=g)).to(DEV)
    ga, gv = torch.randn(S, ca.Cx, ca.Nx, 1, generator=g).to(DEV), torch.randn(S, cb.Cx, cb.Nx, 1, generator=g).to(DEV)
    return sa, sb, fa, fv, ga, gv


def _pair_step(a, b, pair, red, bufs, fa, fv, ga, gv, outs, aux_w):
    """one forward + backward of the two sites (pair None: two site calls) -> (outputs, aux results, token grads, parameter grads)"""
    from avmoe_amd.train import router_aux_total
    for m, bb in zip((a, b), bufs):
        if pair is None or red is None:
            m.zero_grad(set_to_none=True)
        m.load_state_dict({**m.state_dict(), **bb})
    torch.manual_seed(77)
    xa, xv = fa.clone().requires_grad_(True), fv.clone().requires_grad_(True)
    if pair is not None:
        if red is not None:
            red.begin(sync=True)
        oa, ia, pa, la, ov, iv, pv, lv = pair(xa, xv, is_training=True)
    else:
        oa, ia, pa, la, ov, iv, pv, lv = (*a(xa, xv, is_training=True), *b(xv, xa, is_training=True))
    auxs = [m.last_router_aux for m in (a, b)]
    tensors, grads = [0.7 * la + 1.3 * lv], [None]
    if outs:
        tensors += [oa, ov]; grads += [ga, gv]
    if aux_w is not None:
        tensors.append(router_aux_total([a, b], *aux_w)); grads.append(None)
    torch.autograd.backward(tensors, grads)
    if pair is not None and red is not None:
        red.finish()
    res = [t.detach().clone() for t in (oa, ov, pa, pv, la, lv)]
    ax = [None if x is None else tuple(t.detach().clone() for t in x) for x in auxs]
    return res, ax, (xa.grad.clone(), xv.grad.clone()), {f"{i}.{kk}": p.grad.clone() for i, m in enumerate((a, b)) for kk, p in m.named_parameters()}


@pytest.mark.parametrize("sinks", [False, True])
@pytest.mark.parametrize("concurrent", [False, True])
@pytest.mark.parametrize("outs", [True, False])
def test_adapter_pair_with_aux_equals_two_sites(outs, concurrent, sinks):
    """The pair against two site calls: the forward results (aux and load among them) and the router's own parameter gradients bit for
    bit; token gradients and the other parameter gradients at the bars of tests/test_router_grad_gpu.py's pair test (the pair adds
    the two sites' token gradients in another order, and its two-stream mode asks for the shared-GPU launch forms)."""
    from avmoe_amd.adapters import AdapterPair
    from avmoe_amd.dp import AdapterGradReducer
    sa, sb, fa, fv, ga, gv = _pair_sites()
    for m in (sa, sb):
        m.router_aux = True
    ra, rb = copy.deepcopy(sa), copy.deepcopy(sb)
    assert ra.router_aux and rb.router_top_k == 2
    red = AdapterGradReducer([p for m in (sa, sb) for p in m.parameters()], sites=[sa, sb]) if sinks else None
    bufs = [{kk: b.clone() for kk, b in m.named_buffers()} for m in (sa, sb)]
    ref = _pair_step(ra, rb, None, None, bufs, fa, fv, ga, gv, outs, (0.05, 0.6))
    got = _pair_step(sa, sb, AdapterPair(sa, sb, concurrent=concurrent), red, bufs, fa, fv, ga, gv, outs, (0.05, 0.6))
    for r_, g_ in zip(ref[0][2:], got[0][2:]):                   # probs, lb
        assert torch.equal(r_, g_)
    for r_, g_ in zip(ref[1], got[1]):
        assert all(torch.equal(x, y) for x, y in zip(r_, g_)), (r_, g_)
    for r_, g_ in zip(ref[2], got[2]):
        assert float((r_ - g_).abs().max()) <= 1e-5 * float(r_.abs().max())
    for kk, r_ in ref[3].items():
        if ".router." in kk and not sinks:
            assert torch.equal(r_, got[3][kk]), kk
        assert float((r_ - got[3][kk]).abs().max()) <= 1e-4 * max(float(r_.abs().max()), 1e-6), kk


@pytest.mark.parametrize("concurrent", [False, True])
def test_pair_with_aux_on_but_unused_is_the_pair_without(concurrent):
    """router_aux = True with no gradient sent to the losses against router_aux = False: outputs and gradients bit for bit."""
    from avmoe_amd.adapters import AdapterPair
    sa, sb, fa, fv, ga, gv = _pair_sites()
    bufs = [{kk: b.clone() for kk, b in m.named_buffers()} for m in (sa, sb)]
    pair = AdapterPair(sa, sb, concurrent=concurrent)
    off = _pair_step(sa, sb, pair, None, bufs, fa, fv, ga, gv, True, None)
    assert off[1] == [None, None]
    for m in (sa, sb):
        m.router_aux = True
    on = _pair_step(sa, sb, pair, None, bufs, fa, fv, ga, gv, True, None)
    assert all(x is not None for x in on[1])
    for r_, g_ in zip(off[0] + list(off[2]), on[0] + list(on[2])):
        assert torch.equal(r_, g_)
    for kk, r_ in off[3].items():
        assert torch.equal(r_, on[3][kk]), kk
