"""Top-k gating of the mixture on the GPU (avmoe_moe_forward_topk, include/avmoe.h): the C ABI against autograd through tests/topk_ref.py
on every fixture (fp32; bf16 within its budget), probs / idx bit-equal to the dense forward, k = E bit-equal to the dense entry points,
the four bottleneck-space kernel families, AdapterPair and the router-only backward with top-k sites, the module facade and a captured
graph of a top-k pair step."""
import contextlib
import copy
import ctypes as C

import pytest
import torch

from avmoe_amd import _capi as capi
from avmoe_amd import _capi_moe as cm
from oracle import avmoe_oracle as O
from tests.golden_util import golden_names, load_golden, split_params, mha_keep_of
from tests.moe_gpu_util import MoeRun
from tests.router_grad_util import cases, assert_close
from tests.test_adapters_api import build_module
from tests.topk_families import FAMILIES, family_config, plan_family
from tests.topk_ref import topk_forward, topk_grads, topk_mask, k_values

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _forward_topk(run, k, renorm):
    st = run.L.avmoe_moe_forward_topk(C.byref(run.desc), run.X.data_ptr(), run.Y.data_ptr(), C.byref(run.ptrs),
                                      run.noise.data_ptr() if run.noise is not None else None, k, int(renorm), run.out.data_ptr(),
                                      run.probs.data_ptr(), run.idx.data_ptr(), run.lb.data_ptr(), run.saved.data_ptr(), run.scratch.data_ptr(),
                                      torch.cuda.current_stream().cuda_stream)
    capi.check(st, "avmoe_moe_forward_topk")
    torch.cuda.synchronize()
    return run


def _backward_ex(run, dO, dP, lb_weight):
    """avmoe_moe_backward_ex after the forward: {'X', 'Y', parameter key: gradient} on the CPU (dO None: the router-only backward)"""
    dOd = dO.to(DEV, run.tdt).contiguous() if dO is not None else None
    dPd = dP.to(DEV, torch.float32).contiguous() if dP is not None else None
    dX, dY = torch.full_like(run.X, float("nan")), torch.full_like(run.Y, float("nan"))
    grads = {k: torch.full_like(v, float("nan")) for k, v in run.params.items()}
    gptrs = cm.make_ptrs(grads, run.cfg.E_m, run.cfg.E_s)
    lbw = torch.full((1,), float(lb_weight), device=DEV)
    st = run.L.avmoe_moe_backward_ex(C.byref(run.desc), run.X.data_ptr(), run.Y.data_ptr(), C.byref(run.ptrs),
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


def _close(got, ref, rtol, what):
    err = float((got.double() - ref.double()).abs().max())
    assert err <= rtol * max(float(ref.abs().max()), 1e-6), f"{what}: err {err} scale {float(ref.abs().max())}"


@pytest.mark.parametrize("name", list(golden_names()))
def test_topk_fp32_matches_reference(name):
    """k in {1, 2} (< E), both renorm settings, every gradient term (dO, dP, lb; without dO: the router-only backward)."""
    meta, cfg, t, P, B, training, noise, keep = _fixture(name)
    X, Y = t["X"], t["Y"]
    dense = MoeRun(cfg, P, B, X, Y, bf16=False, training=training, noise=noise, mha_keep=keep).forward()
    g = torch.Generator().manual_seed(23)
    for k in [k for k in k_values(cfg.E) if k < cfg.E]:
        for renorm in (True, False):
            what = f"{name}/k={k}/renorm={renorm}"
            ref = topk_forward(P, B, X, Y, cfg, k, renorm, training=training, noise=noise, mha_keep=keep)
            for label, with_out, dP, w in cases(cfg, X.shape[0], 7):
                run = _forward_topk(MoeRun(cfg, P, B, X, Y, bf16=False, training=training, noise=noise, mha_keep=keep), k, renorm)
                _close(run.out.cpu(), ref["out"], 1e-3, what + "/out")
                assert torch.equal(run.probs, dense.probs) and torch.equal(run.idx, dense.idx), what + ": probs / idx not the dense ones"
                assert torch.equal(run.lb, dense.lb), what + ": lb not the dense one"
                if training and cfg.use_bn:               # BatchNorm running statistics advance exactly as in the dense site
                    for kk, v in run.buffers.items():
                        assert torch.equal(v, dense.buffers[kk]), (what, kk)
                dO = torch.randn(X.shape, generator=g) if with_out else None
                refg = topk_grads(cfg, P, B, X, Y, dO, dP, w, training, k, renorm, noise, keep)
                got = _backward_ex(run, dO, dP, w)
                assert run.guards_intact()
                assert_close(got, refg, rtol=1e-3, floor_frac=1e-2, what=f"{what}/{label}")


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("name", list(golden_names()))
def test_topk_k_equals_E_is_the_dense_site_bitwise(name, bf16):
    meta, cfg, t, P, B, training, noise, keep = _fixture(name)
    g = torch.Generator().manual_seed(4)
    dO, dP = torch.randn(t["X"].shape, generator=g), torch.randn(t["X"].shape[0], cfg.E, generator=g)
    w = float(meta["lb_weight"])
    ref = MoeRun(cfg, P, B, t["X"], t["Y"], bf16=bf16, training=training, noise=noise, mha_keep=keep).forward()
    rg = _backward_ex(ref, dO, dP, w)
    for renorm in (True, False):
        run = _forward_topk(MoeRun(cfg, P, B, t["X"], t["Y"], bf16=bf16, training=training, noise=noise, mha_keep=keep), cfg.E, renorm)
        for a, b in ((run.out, ref.out), (run.probs, ref.probs), (run.idx, ref.idx), (run.lb, ref.lb)):
            assert torch.equal(a, b), name
        got = _backward_ex(run, dO, dP, w)
        for kk, v in rg.items():
            assert torch.equal(got[kk], v), (name, renorm, kk)


def _eager_bf16(cfg, P, B, Xb, Yb, dO, dP, w, training, k, renorm, noise, keep, sel):
    """The top-k reference evaluated eagerly on the GPU under torch.autocast(bfloat16) -- matmuls in bf16, softmax / norms in fp32: what
    bf16 does to this computation (tests/golden_util.py::bf16_budget_violations for the dense site) -- with the selection `sel`."""
    d = lambda t: None if t is None else t.to(DEV)
    Pd, Bd = {kk: v.to(DEV) for kk, v in P.items()}, {kk: v.to(DEV) for kk, v in B.items()}
    kd = None if keep is None else {kk: v.to(DEV) for kk, v in keep.items()}
    with torch.autocast("cuda", dtype=torch.bfloat16):
        g = topk_grads(cfg, Pd, Bd, d(Xb), d(Yb), d(dO), d(dP), w, training, k, renorm, d(noise), kd, sel=d(sel))
        g["out"] = topk_forward(Pd, Bd, d(Xb), d(Yb), cfg, k, renorm, training=training, noise=d(noise), update_buffers=False, mha_keep=kd,
                                sel=d(sel))["out"].detach()
    return {kk: v.float().cpu() for kk, v in g.items()}


def _dense_bf16(run, cfg, P, B, Xb, Yb, dO, dP, w, training, noise, keep):
    """(what the dense site's kernels computed, its fp32 reference) on the same bf16 inputs -- the second anchor of _bf16_budget."""
    got = _backward_ex(run, dO, dP, w)
    got["out"] = run.out.float().cpu()
    ref = topk_grads(cfg, P, B, Xb, Yb, dO, dP, w, training, None, True, noise, keep)
    ref["out"] = topk_forward(P, B, Xb, Yb, cfg, None, training=training, noise=noise, update_buffers=False, mha_keep=keep)["out"]
    return got, ref


def _bf16_budget(got, ref, eager, dense, what, floor=1e-2, factor=2.0):
    """The project's bf16 budget (tests/golden_util.py::bf16_budget_violations: floor 1 %, factor 2) against the fp32 reference `ref`,
    per tensor:  relnorm(got) <= max(floor, factor * relnorm(eager bf16), factor * relnorm(dense site));  structurally zero tensors
    (norm < 1e-6 of the largest) in absolute terms, max(1e-4 of the largest norm, factor * either anchor's error); the tiny tensors
    (gates, router bias) as one vector with a 3 % floor.
    The second anchor, dense = (the dense site's kernels, their fp32 reference) on the same bf16 inputs, holds top-k to the error the
    same kernels already have without it: the eager anchor alone moves with the draw -- on avs_v1_train the dense site itself is 3.7 %
    off on dX against 1.0 % eager, and on avs_train_noise expert 0's gradients are 2.8 % off dense (3.8 % eager) and 3.2 % off at k = 2,
    where eager happens to fall to 1.2 %.  A wrong weight or selection is O(1); the fp32 checks hold the semantics to 1e-3."""
    tiny = [kk for kk, v in ref.items() if v.numel() <= 16]

    def views(dct, like):
        out = {kk: dct[kk].float().cpu() for kk in like if kk not in tiny}
        if tiny:
            out["<tiny>"] = torch.cat([dct[kk].float().cpu().reshape(-1) for kk in tiny])
        return out
    g, r, e = views(got, ref), views(ref, ref), views(eager, ref)
    dg, dr = views(dense[0], ref), views(dense[1], ref)
    nmax = max(float(v.norm()) for v in r.values())
    bad = {}
    for kk, rv in r.items():
        err, err_e = float((g[kk] - rv).norm()), float((e[kk] - rv).norm())
        err_d, n_d = float((dg[kk] - dr[kk]).norm()), float(dr[kk].norm())
        if kk != "<tiny>" and float(rv.norm()) < 1e-6 * nmax:
            if err > max(1e-4 * nmax, factor * err_e, factor * err_d):
                bad[kk] = ("structurally zero", err / nmax, err_e / nmax, err_d / nmax)
            continue
        rel, rel_e = err / float(rv.norm()), err_e / float(rv.norm())
        rel_d = err_d / n_d if n_d > 1e-6 * nmax else 0.0
        if rel > max(3e-2 if kk == "<tiny>" else floor, factor * rel_e, factor * rel_d):
            bad[kk] = (rel, rel_e, rel_d)
    assert not bad, f"{what}: bf16 budget exceeded (err, eager bf16 err, dense site err): {bad}"


@pytest.mark.parametrize("name", ["ave_train", "avqa_train", "avvp_train", "avs_train_noise", "avs_v2_train", "avs_v1_train", "ave_eval",
                                  "avs_k87_train", "ave_wide_train"])
def test_topk_bf16_within_budget(name):
    meta, cfg, t, P, B, training, noise, keep = _fixture(name)
    Xb, Yb = t["X"].to(torch.bfloat16).float(), t["Y"].to(torch.bfloat16).float()
    g = torch.Generator().manual_seed(12)
    dO = torch.randn(Xb.shape, generator=g).to(torch.bfloat16).float()
    dP = torch.randn(Xb.shape[0], cfg.E, generator=g)
    w = 0.5 if cfg.lb_loss else 0.0
    dense = MoeRun(cfg, P, B, Xb, Yb, bf16=True, training=training, noise=noise, mha_keep=keep).forward()
    dense_pair = _dense_bf16(dense, cfg, P, B, Xb, Yb, dO, dP, w, training, noise, keep)
    for k in [k for k in k_values(cfg.E) if k < cfg.E]:
        sel = topk_mask(dense.probs.cpu(), k)              # the experts the kernels keep (from the probabilities they computed)
        for renorm in (True, False):
            run = _forward_topk(MoeRun(cfg, P, B, Xb, Yb, bf16=True, training=training, noise=noise, mha_keep=keep), k, renorm)
            assert torch.equal(run.probs, dense.probs) and torch.equal(run.idx, dense.idx)
            got = _backward_ex(run, dO, dP, w)
            got["out"] = run.out.float().cpu()
            ref = topk_grads(cfg, P, B, Xb, Yb, dO, dP, w, training, k, renorm, noise, keep, sel=sel)
            ref["out"] = topk_forward(P, B, Xb, Yb, cfg, k, renorm, training=training, noise=noise, update_buffers=False, mha_keep=keep,
                                      sel=sel)["out"]
            eager = _eager_bf16(cfg, P, B, Xb, Yb, dO, dP, w, training, k, renorm, noise, keep, sel)
            _bf16_budget(got, ref, eager, dense_pair, f"{name}/k={k}/renorm={renorm}")


def _prof_names(fn):
    L = capi.lib()
    torch.cuda.synchronize()
    L.avmoe_prof_reset()
    L.avmoe_prof_enable(1)
    try:
        out = fn()
        torch.cuda.synchronize()
    finally:
        L.avmoe_prof_enable(0)
    names = [r["name"] for r in capi.prof_report()]
    L.avmoe_prof_reset()
    return out, names


@pytest.mark.parametrize("family", list(FAMILIES))
def test_topk_in_every_kernel_family(family):
    """One shape per bottleneck-space kernel family (tests/topk_families.py): the plan puts it on that family, and the streaming form
    runs (profiler scopes "... (stream)") exactly in the tile_stream case."""
    cfg, S, bf16 = family_config(family)
    assert plan_family(cfg, S, bf16) == ("tile_fast" if family == "tile_stream" else family)
    P, B = O.init_params(cfg, seed=3)
    g = torch.Generator().manual_seed(17)
    X = 0.3 * torch.randn(S, cfg.Nx, cfg.Cx, generator=g)
    Y = 0.3 * torch.randn(S, cfg.Ny, cfg.Cy, generator=g)
    if bf16:
        X, Y = X.to(torch.bfloat16).float(), Y.to(torch.bfloat16).float()
    dO = torch.randn(S, cfg.Nx, cfg.Cx, generator=g).to(torch.bfloat16).float()
    dP = torch.randn(S, cfg.E, generator=g)
    hooks = capi.test_hooks(capi.HOOK_KFS_FORCE) if family == "tile_stream" else contextlib.nullcontext()
    with hooks:
        dense = MoeRun(cfg, P, B, X, Y, bf16=bf16, training=True).forward()
        dense_pair = _dense_bf16(dense, cfg, P, B, X, Y, dO, dP, 0.5, True, None, None) if bf16 else None
        for k, renorm in ((1, True), (1, False), (2, True)):     # k = 1: zero weights for all but one expert of every frame
            def step():
                run = _forward_topk(MoeRun(cfg, P, B, X, Y, bf16=bf16, training=True), k, renorm)
                return run, _backward_ex(run, dO, dP, 0.5)
            (run, got), names = _prof_names(step)
            assert run.guards_intact()
            assert any(n.endswith("(stream)") for n in names) == (family == "tile_stream"), names
            assert torch.equal(run.probs, dense.probs) and torch.equal(run.idx, dense.idx)
            got["out"] = run.out.float().cpu()
            sel = topk_mask(dense.probs.cpu(), k)
            ref = topk_grads(cfg, P, B, X, Y, dO, dP, 0.5, True, k, renorm, sel=sel)
            ref["out"] = topk_forward(P, B, X, Y, cfg, k, renorm, training=True, update_buffers=False, sel=sel)["out"]
            what = f"{family}/k={k}/renorm={renorm}"
            if bf16:
                _bf16_budget(got, ref, _eager_bf16(cfg, P, B, X, Y, dO, dP, 0.5, True, k, renorm, None, None, sel), dense_pair, what)
            else:
                out_ref = ref.pop("out")
                _close(got.pop("out"), out_ref, 1e-3, what + "/out")
                assert_close(got, ref, rtol=1e-3, floor_frac=1e-2, what=what)


def _pair_cfgs(small):
    kw = dict(E_m=2, E_s=2, groups=2, K=32, variant="avs", lb_loss=True)
    if small:
        return O.AdapterConfig(Cx=64, Nx=72, Cy=48, Ny=40, reduction=4, **kw), O.AdapterConfig(Cx=48, Nx=40, Cy=64, Ny=72, reduction=4, **kw)
    return O.AdapterConfig(Cx=768, Nx=1024, Cy=768, Ny=196, reduction=12, **kw), O.AdapterConfig(Cx=768, Nx=196, Cy=768, Ny=1024, reduction=12, **kw)


@pytest.mark.parametrize("concurrent", [False, True])
@pytest.mark.parametrize("shape", ["cfg2_bf16", "small_f32"])
@pytest.mark.parametrize("outs", ["both", "none"])
def test_adapter_pair_with_topk_sites_equals_two_sites(shape, concurrent, outs):
    """Both backward sections (two streams) and the back-to-back pair (fused dX + dY path) with top-k sites; outs = none: the router-only
    backward of both sites."""
    from avmoe_amd.adapters import AdapterPair
    bf16 = shape == "cfg2_bf16"
    ca, cb = _pair_cfgs(not bf16)
    dt = torch.bfloat16 if bf16 else torch.float32
    torch.manual_seed(5)
    sa, sb = build_module("avs", ca).to(DEV).train(), build_module("avs", cb).to(DEV).train()
    sa.router_top_k, sb.router_top_k, sb.router_top_k_renorm = 2, 1, False
    with torch.no_grad():
        for m in (sa, sb):
            for k, p in m.named_parameters():
                if k.endswith(("gate", "gate_av")):
                    p.fill_(0.3)
    ra, rb = copy.deepcopy(sa), copy.deepcopy(sb)
    g = torch.Generator().manual_seed(9)
    S = 4
    fa = (0.5 * torch.randn(S, ca.Cx, ca.Nx, 1, generator=g)).to(DEV, dt)
    fv = (0.5 * torch.randn(S, cb.Cx, cb.Nx, 1, generator=g)).to(DEV, dt)
    ga, gv = torch.randn(S, ca.Cx, ca.Nx, 1, generator=g).to(DEV, dt), torch.randn(S, cb.Cx, cb.Nx, 1, generator=g).to(DEV, dt)
    pa_g, pv_g = torch.randn(S, 1, ca.E, generator=g).to(DEV), torch.randn(S, 1, cb.E, generator=g).to(DEV)
    bufs = [{k: b.clone() for k, b in m.named_buffers()} for m in (sa, sb)]

    def run(a, b, pair):
        for m, bb in zip((a, b), bufs):
            m.zero_grad(set_to_none=True)
            m.load_state_dict({**m.state_dict(), **bb})
        torch.manual_seed(77)
        xa, xv = fa.clone().requires_grad_(True), fv.clone().requires_grad_(True)
        if pair is not None:
            oa, ia, pa, la, ov, iv, pv, lv = pair(xa, xv, is_training=True)
        else:
            oa, ia, pa, la, ov, iv, pv, lv = (*a(xa, xv, is_training=True), *b(xv, xa, is_training=True))
        if outs == "both":
            torch.autograd.backward([oa, ov, pa, pv, 0.7 * la + 1.3 * lv], [ga, gv, pa_g, pv_g, None])
        else:
            torch.autograd.backward([pa, pv, 0.7 * la + 1.3 * lv], [pa_g, pv_g, None])
        return (oa.detach().float(), ov.detach().float()), (xa.grad.float(), xv.grad.float()), [p.grad.clone() for m in (a, b) for p in m.parameters()]

    ref = run(ra, rb, None)
    got = run(sa, sb, AdapterPair(sa, sb, concurrent=concurrent))
    ttol = 2e-2 if bf16 else 1e-5                         # (two streams: CU-exclusive launches, another BatchNorm summation order)
    for r_, g_ in zip(ref[0] + ref[1], got[0] + got[1]):
        assert float((r_ - g_).abs().max()) <= ttol * float(r_.abs().max())
    for r_, g_ in zip(ref[2], got[2]):
        assert float((r_ - g_).abs().max()) <= 1e-4 * max(float(r_.abs().max()), 1e-6)
    for (ka, va), (kb, vb) in zip(list(sa.named_buffers()) + list(sb.named_buffers()), list(ra.named_buffers()) + list(rb.named_buffers())):
        assert torch.allclose(va.double(), vb.double(), rtol=1e-4, atol=1e-6), ka


MODULES = {"ave": "ave_train", "avqa": "avqa_train", "avvp": "avvp_train", "avs": "avs_train_noise"}


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("which", list(MODULES))
def test_module_facade_topk(which, training):
    """Each facade class with router_top_k = 2 against topk_ref (AVS: with its logit noise in training), and its BatchNorm running
    statistics / num_batches_tracked after a training step equal to those of the dense module."""
    meta, cfg, t, P, B, _tr, _noise, _keep = _fixture(MODULES[which])
    m = build_module(which, cfg).to(DEV)
    m.load_state_dict({**P, **B}, strict=True)
    m.train(training)
    md = copy.deepcopy(m)
    m.router_top_k, m.router_top_k_renorm = 2, True
    S = t["X"].shape[0]
    X, Y = t["X"].to(DEV).requires_grad_(True), t["Y"].to(DEV).requires_grad_(True)
    x4, y4 = X.permute(0, 2, 1).unsqueeze(-1), Y.permute(0, 2, 1).unsqueeze(-1)
    noise = None
    torch.manual_seed(123)
    if which == "avs":
        out, idx, probs, lb = m(x4, y4, is_training=training)
        if training:
            torch.manual_seed(123)
            noise = (torch.randn(S, cfg.E, device=DEV) * 0.01).cpu()
    elif which == "avvp":
        out, lb = m(x4, y4)
    else:
        out, idx = m(x4, y4)
    G = t["grad_out"]
    (out.squeeze(-1).permute(0, 2, 1) * G.to(DEV)).sum().backward()
    ref = topk_forward(P, B, t["X"], t["Y"], cfg, 2, True, training=training, noise=noise, update_buffers=False)
    _close(out.squeeze(-1).permute(0, 2, 1).detach().cpu(), ref["out"], 1e-3, which)
    refg = topk_grads(cfg, P, B, t["X"], t["Y"], G, None, 0.0, training, 2, True, noise)
    got = {"X": X.grad.cpu(), "Y": Y.grad.cpu()}
    for k, v in m.named_parameters():
        got[k] = v.grad.cpu() if v.grad is not None else torch.zeros_like(v).cpu()
    assert_close(got, refg, rtol=1e-3, floor_frac=1e-2, what=which)
    # the dense module on the same call: identical running statistics and counters
    torch.manual_seed(123)
    if which == "avs":
        md(x4.detach(), y4.detach(), is_training=training)
    else:
        md(x4.detach(), y4.detach())
    torch.cuda.synchronize()
    for (k, v), (_, vd) in zip(m.named_buffers(), md.named_buffers()):
        assert torch.equal(v, vd), (which, k)


def test_captured_graph_replay_of_a_topk_pair_step():
    """Forward (top-k) + backward of both sites of a pair through the C ABI, captured into a graph on one stream: the replay is bit-identical
    to the eager calls (tests/test_graph_capture_gpu.py for the dense site)."""
    kw = dict(reduction=2, groups=2, K=32, variant="avs", lb_loss=True)
    ca = O.AdapterConfig(Cx=128, Nx=150, Cy=64, Ny=50, **kw)
    cb = O.AdapterConfig(Cx=64, Nx=50, Cy=128, Ny=150, **kw)
    S = 4
    g = torch.Generator().manual_seed(0)
    Xa = 0.3 * torch.randn(S, ca.Nx, ca.Cx, generator=g)
    Xb = 0.3 * torch.randn(S, cb.Nx, cb.Cx, generator=g)
    runs = []
    for cfg, X, Y, seed, k in ((ca, Xa, Xb, 1, 2), (cb, Xb, Xa, 2, 1)):
        P, B = O.init_params(cfg, seed=seed)
        r = _forward_topk(MoeRun(cfg, P, B, X, Y, bf16=True, training=False), k, True)
        r.top_k = k
        r.backward(torch.randn(S, cfg.Nx, cfg.Cx, generator=g))
        runs.append(r)
    L = capi.lib()
    refs = [(r.out.clone(), r.dX.clone(), r.dY.clone(), {k: v.clone() for k, v in r.grads.items()}) for r in runs]

    def calls(stream):
        for r in runs:
            capi.check(L.avmoe_moe_forward_topk(C.byref(r.desc), r.X.data_ptr(), r.Y.data_ptr(), C.byref(r.ptrs), None, r.top_k, 1,
                                                r.out.data_ptr(), r.probs.data_ptr(), r.idx.data_ptr(), r.lb.data_ptr(),
                                                r.saved.data_ptr(), r.scratch.data_ptr(), stream), "forward_topk")
        for r in runs:
            capi.check(L.avmoe_moe_backward(C.byref(r.desc), r.X.data_ptr(), r.Y.data_ptr(), C.byref(r.ptrs), r.dOut.data_ptr(), None,
                                            r.saved.data_ptr(), r.scratch.data_ptr(), r.dX.data_ptr(), r.dY.data_ptr(), C.byref(r.gptrs),
                                            stream), "backward")

    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        calls(s.cuda_stream)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        calls(torch.cuda.current_stream().cuda_stream)
    for r in runs:
        for t_ in (r.out, r.dX, r.dY, *r.grads.values()):
            t_.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for r, (o, dx, dy, gr) in zip(runs, refs):
        assert torch.equal(r.out, o) and torch.equal(r.dX, dx) and torch.equal(r.dY, dy)
        for k, v in r.grads.items():
            assert torch.equal(v, gr[k]), k


def test_dual_backbone_loop_with_topk_sites_equals_site_by_site():
    """DualBackboneLoop hands each site's top-k setting through its AdapterPairs: the loop equals the site-by-site schedule run with the
    same (top-k) modules (the pattern of tests/test_blocks_gpu.py, fp32), and differs from the dense sites."""
    from torch import nn
    from avmoe_amd.blocks import DualBackboneLoop
    from tests.test_blocks import Stage, restated_loop
    from tests.test_blocks_gpu import VisBlock, AudBlock, Merge
    torch.manual_seed(5)
    S, Cv, Nv, Ca, Na = 3, 64, 144, 48, 256
    dims = [(Cv, Nv, Ca, Na), (2 * Cv, Nv // 4, 2 * Ca, Na // 4)]
    sv = [Stage(nn.ModuleList([VisBlock(c), VisBlock(c)]).to(DEV), Merge(c).to(DEV)) for c, _, _, _ in dims]
    sa = [Stage(nn.ModuleList([AudBlock(c), AudBlock(c)]).to(DEV), Merge(c).to(DEV)) for _, _, c, _ in dims]
    sites = {k: [] for k in ("a1", "v1", "a2", "v2")}
    for i, (cv, nv, ca, na) in enumerate(dims):
        for pos in ("1", "2", "1", "2"):                          # two adapted blocks per stage
            a = build_module("ave", O.AdapterConfig(Cx=ca, Nx=na, Cy=cv, Ny=nv, reduction=4, groups=2, K=8)).to(DEV).train()
            v = build_module("ave", O.AdapterConfig(Cx=cv, Nx=nv, Cy=ca, Ny=na, reduction=4, groups=2, K=8)).to(DEV).train()
            with torch.no_grad():
                for m in (a, v):
                    for k, p in m.named_parameters():
                        if k.endswith(("gate", "gate_av")):
                            p.fill_(0.3)
            a.router_top_k, v.router_top_k = 2, (1 if i else 2)          # per-site settings, renormalised and Switch style
            v.router_top_k_renorm = bool(i)
            sites["a" + pos].append(a); sites["v" + pos].append(v)
    all_sites = [m for k in sites for m in sites[k]]
    bufs = [{k: b.clone() for k, b in m.named_buffers()} for m in all_sites]
    g = torch.Generator().manual_seed(1)
    f_v0 = (0.5 * torch.randn(S, Nv, Cv, generator=g)).to(DEV)
    f_a0 = (0.5 * torch.randn(S, Na, Ca, generator=g)).to(DEV)
    g_v = torch.randn(S, Nv // 16, 4 * Cv, generator=g).to(DEV)
    g_a = torch.randn(S, Na // 16, 4 * Ca, generator=g).to(DEV)

    def run(fused):
        for m, bb in zip(all_sites, bufs):
            m.zero_grad(); m.load_state_dict({**m.state_dict(), **bb})
        f_v, f_a = f_v0.clone().requires_grad_(True), f_a0.clone().requires_grad_(True)
        if fused:
            ov, oa, rec = DualBackboneLoop(sites["a1"], sites["v1"], sites["a2"], sites["v2"], num_skip=1)(sv, sa, f_v, f_a)
            rec = rec.to_dict()
        else:
            ov, oa, rec = restated_loop(sv, sa, f_v, f_a, sites, 1, True, True)
        torch.autograd.backward([ov, oa], [g_v, g_a])
        return ov.detach(), oa.detach(), rec, f_v.grad, f_a.grad, [p.grad.clone() for m in all_sites for p in m.parameters()]

    ref, got = run(False), run(True)
    assert got[2] == ref[2]
    gscale = max(float(x.abs().max()) for x in ref[5])
    for what, a, b, floor in [("f_v", ref[0], got[0], 0.0), ("f_a", ref[1], got[1], 0.0), ("d f_v", ref[3], got[3], 0.0),
                              ("d f_a", ref[4], got[4], 0.0)] + [(f"site param {i}", a, b, 1e-2 * gscale) for i, (a, b) in enumerate(zip(ref[5], got[5]))]:
        assert float((a - b).abs().max()) <= 1e-4 * (max(float(a.abs().max()), floor) + 1e-12), what
    for m in all_sites:
        m.router_top_k = None
    dense = run(True)
    assert float((dense[0] - got[0]).abs().max()) > 1e-3 * float(got[0].abs().max()), "top-k had no effect in the loop"
