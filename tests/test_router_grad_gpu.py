"""Differentiable routing probabilities on the GPU: avmoe_moe_backward_ex (dprobs, and dOut = NULL -> the router-only backward) against
autograd through the oracle, the module facade (MoEAdapterAVS's probs carry a grad_fn), AdapterPair with a probs term, and the
dprobs = NULL path bit for bit equal to avmoe_moe_backward."""
import copy
import ctypes as C

import pytest
import torch

from avmoe_amd import _capi as capi
from avmoe_amd import _capi_moe as cm
from oracle import avmoe_oracle as O
from tests.golden_util import golden_names, load_golden, split_params, mha_keep_of
from tests.moe_gpu_util import MoeRun
from tests.router_grad_util import oracle_grads, cases, expert_keys, assert_close
from tests.test_adapters_api import build_module

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _run_ex(run, dO, dP, lb_weight):
    """avmoe_moe_backward_ex on a MoeRun after its forward: {'X', 'Y', parameter key: gradient} on the CPU"""
    L = run.L
    dOd = dO.to(DEV, run.tdt).contiguous() if dO is not None else None
    dPd = dP.to(DEV, torch.float32).contiguous() if dP is not None else None
    dX, dY = torch.full_like(run.X, float("nan")), torch.full_like(run.Y, float("nan"))
    grads = {k: torch.full_like(v, float("nan")) for k, v in run.params.items()}
    gptrs = cm.make_ptrs(grads, run.cfg.E_m, run.cfg.E_s)
    lbw = torch.full((1,), float(lb_weight), device=DEV)
    st = L.avmoe_moe_backward_ex(C.byref(run.desc), run.X.data_ptr(), run.Y.data_ptr(), C.byref(run.ptrs),
                                 dOd.data_ptr() if dOd is not None else None, dPd.data_ptr() if dPd is not None else None,
                                 lbw.data_ptr(), run.saved.data_ptr(), run.scratch.data_ptr(), dX.data_ptr(), dY.data_ptr(),
                                 C.byref(gptrs), 0, torch.cuda.current_stream().cuda_stream)
    capi.check(st, "avmoe_moe_backward_ex")
    torch.cuda.synchronize()
    g = {k: v.cpu() for k, v in grads.items()}
    g["X"], g["Y"] = dX.float().cpu(), dY.float().cpu()
    return g


def _fixture(name):
    meta, cfg, t = load_golden(name)
    P, B = split_params(t)
    return meta, cfg, t, P, B, bool(meta["module_train"]), (t["noise"].contiguous() if "noise" in t else None), mha_keep_of(t)


@pytest.mark.parametrize("name", list(golden_names()))
def test_backward_ex_fp32_matches_oracle(name):
    meta, cfg, t, P, B, training, noise, keep = _fixture(name)
    X, Y = t["X"], t["Y"]
    g = torch.Generator().manual_seed(21)
    for label, with_out, dP, w in cases(cfg, X.shape[0], 5):
        dO = torch.randn(X.shape, generator=g) if with_out else None
        ref = oracle_grads(cfg, P, B, X, Y, dO, dP, w, training, noise, keep)
        run = MoeRun(cfg, P, B, X, Y, bf16=False, training=training, noise=noise, mha_keep=keep).forward()
        got = _run_ex(run, dO, dP, w)
        assert run.guards_intact()
        assert_close(got, ref, rtol=1e-3, what=f"{name}/{label}")
        if not with_out:
            assert all(float(got[k].abs().max()) == 0.0 for k in expert_keys(got)), "expert gradients must be exactly 0 without dOut"


@pytest.mark.parametrize("name", ["ave_train", "avs_train_nonoise", "avvp_train", "avs_v2_train", "avqa_train"])
def test_router_only_backward_bf16(name):
    """bf16 tokens: the router-only backward against the fp32 oracle on the bf16-rounded inputs, relative norm within the 1e-2 floor of
    the bf16 budget (tests/golden_util.py::bf16_budget_violations) -- nothing in this path has a bf16 product, only bf16 token I/O."""
    meta, cfg, t, P, B, training, noise, keep = _fixture(name)
    Xb, Yb = t["X"].to(torch.bfloat16).float(), t["Y"].to(torch.bfloat16).float()
    for label, with_out, dP, w in cases(cfg, Xb.shape[0], 6):
        if with_out:
            continue
        ref = oracle_grads(cfg, P, B, Xb, Yb, None, dP, w, training, noise, keep)
        run = MoeRun(cfg, P, B, Xb, Yb, bf16=True, training=training, noise=noise, mha_keep=keep).forward()
        got = _run_ex(run, None, dP, w)
        for k, r in ref.items():
            if float(r.norm()) == 0.0:
                assert float(got[k].abs().max()) == 0.0, (name, label, k)
                continue
            rel = float((got[k] - r).norm() / r.norm())
            assert rel <= 1e-2, (name, label, k, rel)


@pytest.mark.parametrize("name,bf16", [("ave_train", True), ("avs_train_noise", False), ("avvp_train", True)])
def test_ex_without_dprobs_is_bitwise_backward(name, bf16):
    meta, cfg, t, P, B, training, noise, keep = _fixture(name)
    g = torch.Generator().manual_seed(4)
    dO = torch.randn(t["X"].shape, generator=g)
    w = float(meta["lb_weight"])
    run = MoeRun(cfg, P, B, t["X"], t["Y"], bf16=bf16, training=training, noise=noise, mha_keep=keep).forward()
    ref = run.backward(dO, lb_weight=w)
    got = _run_ex(run, dO, None, w)
    for k, r in ref.items():
        assert torch.equal(r.float(), got[k]), k


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


def _avs_module(cfg, P, B, training):
    m = build_module("avs", cfg).to(DEV)
    m.load_state_dict({**P, **B}, strict=True)
    m.train(training)
    return m


def _module_grads(m, X, Y):
    g = {"X": X.grad.cpu(), "Y": Y.grad.cpu()}
    for k, v in m.named_parameters():
        g[k] = v.grad.cpu() if v.grad is not None else torch.zeros_like(v).cpu()
    return g


@pytest.mark.parametrize("terms", ["full", "probs_only", "lb_only"])
def test_avs_module_probs_are_differentiable(terms):
    meta, cfg, t, P, B, training, _noise, _keep = _fixture("avs_train_nonoise")
    m = _avs_module(cfg, P, B, training)
    S = t["X"].shape[0]
    g = torch.Generator().manual_seed(8)
    dO = t["grad_out"] if terms == "full" else None
    dP = torch.randn(S, cfg.E, generator=g) if terms != "lb_only" else None
    w = 0.01 if terms != "probs_only" else 0.0
    ref = oracle_grads(cfg, P, B, t["X"], t["Y"], dO, dP, w, training)
    X, Y = t["X"].to(DEV).requires_grad_(True), t["Y"].to(DEV).requires_grad_(True)
    out, idx, probs, lb = m(X.permute(0, 2, 1).unsqueeze(-1), Y.permute(0, 2, 1).unsqueeze(-1), is_training=False)
    assert probs.requires_grad and probs.grad_fn is not None and probs.shape == (S, 1, cfg.E)
    assert not idx.requires_grad
    loss = torch.zeros((), device=DEV)
    if dO is not None:
        loss = loss + (out.squeeze(-1).permute(0, 2, 1) * dO.to(DEV)).sum()
    if dP is not None:
        loss = loss + (probs * dP.to(DEV).unsqueeze(1)).sum()
    if w:
        loss = loss + w * lb
    fams = _prof_families(loss.backward)
    got = _module_grads(m, X, Y)
    assert_close(got, ref, rtol=1e-3, what=terms)
    if terms == "full":
        return
    assert all(float(got[k].abs().max()) == 0.0 for k in expert_keys(got))
    # the router-only backward: no expert, Gram or token-space family; the router's small GEMMs and dWf are the only GEMMs
    assert {"k_router_bwd", "k_ro_y", "k_ro_dx"} <= set(fams), fams
    allowed = ("k_router_bwd", "k_ro_")
    other = {k: v for k, v in fams.items() if not k.startswith(allowed)}
    assert all(k.startswith("gemm_") and not k.startswith(("gemm_stream", "gemm_tokpair")) for k in other), fams
    assert sum(other.values()) <= 4, fams      # (drin, dW1, dWf + its split-K reduce)


def test_probs_loss_reaches_parameters_through_module():
    """Without the feature a probs-only loss raised 'does not require grad'; now it trains the router and the remap."""
    meta, cfg, t, P, B, training, _n, _k = _fixture("avs_train_nonoise")
    m = _avs_module(cfg, P, B, training)
    X = t["X"].to(DEV)
    Y = t["Y"].to(DEV)
    _, _, probs, _ = m(X.permute(0, 2, 1).unsqueeze(-1), Y.permute(0, 2, 1).unsqueeze(-1), is_training=False)
    ent = -(probs * probs.clamp_min(1e-9).log()).sum()           # router entropy
    ent.backward()
    assert float(m.router[0].weight.grad.abs().max()) > 0 and float(m.fc.weight.grad.abs().max()) > 0
    assert float(m.conv_adapter.weight.grad.abs().max()) > 0


def _cfg2_pair_cfgs(small):
    kw = dict(E_m=2, E_s=2, groups=2, K=32, variant="avs", lb_loss=True)
    if small:       # an fp32 pair of generic shape
        return O.AdapterConfig(Cx=64, Nx=72, Cy=48, Ny=40, reduction=4, **kw), O.AdapterConfig(Cx=48, Nx=40, Cy=64, Ny=72, reduction=4, **kw)
    # the cfg-2 site shapes (audio 1024 x 768 tokens, visual 196 x 768, bottleneck 64 in two groups) with the AVS signature (probs returned)
    return O.AdapterConfig(Cx=768, Nx=1024, Cy=768, Ny=196, reduction=12, **kw), O.AdapterConfig(Cx=768, Nx=196, Cy=768, Ny=1024, reduction=12, **kw)


@pytest.mark.parametrize("sinks", [False, True])
@pytest.mark.parametrize("concurrent", [False, True])
@pytest.mark.parametrize("shape", ["cfg2_bf16", "small_f32"])
@pytest.mark.parametrize("outs", ["both", "none"])
def test_adapter_pair_with_probs_term_equals_two_sites(shape, concurrent, sinks, outs):
    from avmoe_amd.adapters import AdapterPair
    from avmoe_amd.dp import AdapterGradReducer
    bf16 = shape == "cfg2_bf16"
    ca, cb = _cfg2_pair_cfgs(not bf16)
    dt = torch.bfloat16 if bf16 else torch.float32
    torch.manual_seed(5)
    sa, sb = build_module("avs", ca).to(DEV).train(), build_module("avs", cb).to(DEV).train()
    with torch.no_grad():
        for m in (sa, sb):
            for k, p in m.named_parameters():
                if k.endswith(("gate", "gate_av")):
                    p.fill_(0.3)
    ra, rb = copy.deepcopy(sa), copy.deepcopy(sb)
    red = AdapterGradReducer([p for m in (sa, sb) for p in m.parameters()], sites=[sa, sb]) if sinks else None
    g = torch.Generator().manual_seed(9)
    S = 4
    fa = (0.5 * torch.randn(S, ca.Cx, ca.Nx, 1, generator=g)).to(DEV, dt)
    fv = (0.5 * torch.randn(S, cb.Cx, cb.Nx, 1, generator=g)).to(DEV, dt)
    ga, gv = torch.randn(S, ca.Cx, ca.Nx, 1, generator=g).to(DEV, dt), torch.randn(S, cb.Cx, cb.Nx, 1, generator=g).to(DEV, dt)
    pa_g, pv_g = torch.randn(S, 1, ca.E, generator=g).to(DEV), torch.randn(S, 1, cb.E, generator=g).to(DEV)
    bufs = [{k: b.clone() for k, b in m.named_buffers()} for m in (sa, sb)]

    def run(a, b, pair):
        for m, bb in zip((a, b), bufs):
            if pair is None or red is None:               # (a site with a gradient sink keeps its views of the bucket: red.begin resets them)
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
        assert pa.requires_grad and pv.requires_grad
        if outs == "both":
            torch.autograd.backward([oa, ov, pa, pv, 0.7 * la + 1.3 * lv], [ga, gv, pa_g, pv_g, None])
        else:
            torch.autograd.backward([pa, pv, 0.7 * la + 1.3 * lv], [pa_g, pv_g, None])
        if pair is not None and red is not None:
            red.finish()
        return (xa.grad.float(), xv.grad.float()), [p.grad.clone() for m in (a, b) for p in m.parameters()]

    ref = run(ra, rb, None)
    got = run(sa, sb, AdapterPair(sa, sb, concurrent=concurrent))
    ttol = 2e-2 if bf16 else 1e-5
    for r_, g_ in zip(ref[0], got[0]):
        assert float((r_ - g_).abs().max()) <= ttol * float(r_.abs().max())
    for r_, g_ in zip(ref[1], got[1]):
        assert float((r_ - g_).abs().max()) <= 1e-4 * max(float(r_.abs().max()), 1e-6)
