"""The mixture regularisers on the GPU: the draw kernel (avmoe_mix_drop_draw, csrc/mix_drop.hip) against the Philox reference of
tests/mix_drop_ref.py, the site call with a multiplier on the mixture weights (avmoe_moe_forward_reg / _backward_reg) against the host
twin and against the library's own per-expert outputs, and the facade (drop_path, expert_dropout).

Shapes: (A) the smallest AVE training fixture shape (ave_train: 6 frames of 40 x 96 tokens, 4 experts), fp32; (B) one bf16 site of the
cfg-2 form with 4 x 520 = 2080 tokens, just over the 2048-token line behind which the bottleneck-space passes run in their streamed form."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

from avmoe_amd import _capi as capi
from avmoe_amd import _capi_moe as cm
from oracle import avmoe_oracle as O
from tests import mix_drop_ref as R
from tests.golden_util import load_golden, split_params
from tests.moe_gpu_util import MoeRun, make_desc
from tests.test_adapters_api import build_module

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
BAD_ARG = -1
_CACHE = {}


def _ptr(t):
    return t.data_ptr() if t is not None else None


# ---- the draw -------------------------------------------------------------------------------------------------------------------------
def _state(seed, calls):
    s = lambda v: v - (1 << 64) if v >= (1 << 63) else v
    return torch.tensor([s(seed), s(calls)], dtype=torch.int64, device=DEV)


def _draw(state, S, E, p, q, mix):
    return capi.lib().avmoe_mix_drop_draw(_ptr(state), S, E, p, q, _ptr(mix), torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize("p,q", [(0.25, 0.5), (0.0, 0.3), (0.4, 0.0)])
def test_draw_equals_the_reference(p, q):
    """Every S in {1, 3, 20} and E in {1, 2, 4, 16}: two launches equal mix_drop_ref at calls and calls + 1, bit for bit, `calls` advances
    by exactly 1 per launch (across the 2^32 boundary of its low word too), nothing past S E floats is written, and the two draws differ."""
    seed = 0xC0FFEE1234567891
    for S in (1, 3, 20):
        for E in (1, 2, 4, 16):
            for calls in (0, (1 << 32) - 1):
                st = _state(seed, calls)
                for step in range(2):
                    buf = torch.full((S * E + 64,), -7.0, device=DEV)
                    assert _draw(st, S, E, p, q, buf) == 0
                    torch.cuda.synchronize()
                    got = buf[:S * E].reshape(S, E).cpu().numpy()
                    assert np.array_equal(got, R.mix_scale(seed, calls + step, S, E, p, q)), (S, E, calls, step)
                    assert bool((buf[S * E:] == -7.0).all())
                    assert st.cpu().tolist() == _state(seed, calls + step + 1).cpu().tolist()
                    if step == 0:
                        first = got
                if S * E >= 80:                               # (80 draws: two equal masks would be a 2^-60 event at these rates)
                    assert not np.array_equal(first, got)


def test_draw_statistics():
    """64 launches at S = 20, E = 4: the drop frequency of the 5120 pairs (q alone) and of the 1280 frames (p alone) within five standard
    deviations of a binomial share, 5 sqrt(r (1 - r) / n), of the rate."""
    S, E, n_launch = 20, 4, 64
    for p, q in ((0.0, 0.3), (0.2, 0.0)):
        st = _state(20240607, 0)
        bufs = torch.empty(n_launch, S, E, device=DEV)
        for i in range(n_launch):
            assert _draw(st, S, E, p, q, bufs[i]) == 0
        torch.cuda.synchronize()
        assert int(st[1]) == n_launch
        m = bufs.cpu()
        if q:
            f, r, n = float((m == 0).float().mean()), q, n_launch * S * E
        else:
            assert bool(((m == 0).all(-1) | (m != 0).all(-1)).all())          # whole frames
            f, r, n = float((m[..., 0] == 0).float().mean()), p, n_launch * S
        print(f"drop frequency {f:.4f} at rate {r} over {n} draws (bound {5 * (r * (1 - r) / n) ** 0.5:.4f})")
        assert abs(f - r) <= 5 * (r * (1 - r) / n) ** 0.5


def test_draw_refusals_launch_nothing():
    S, E = 5, 4
    st = _state(11, 3)
    buf = torch.full((S * E,), -7.0, device=DEV)
    nan = float("nan")
    for args in ((st, S, E, 1.0, 0.1, buf), (st, S, E, 0.1, 1.0, buf), (st, S, E, -0.1, 0.1, buf), (st, S, E, 0.1, -1e-3, buf),
                 (st, S, E, nan, 0.1, buf), (st, S, E, 0.1, nan, buf), (st, S, 17, 0.1, 0.1, buf), (st, S, 0, 0.1, 0.1, buf),
                 (st, 0, E, 0.1, 0.1, buf), (None, S, E, 0.1, 0.1, buf), (st, S, E, 0.1, 0.1, None)):
        assert _draw(*args) == BAD_ARG, args[1:5]
        assert capi.lib().avmoe_last_error()
    torch.cuda.synchronize()
    assert st.cpu().tolist() == [11, 3] and bool((buf == -7.0).all())
    assert _draw(st, S, E, 0.0, 0.0, buf) == 0                  # both rates 0 is served: all ones, and it counts
    torch.cuda.synchronize()
    assert bool((buf == 1.0).all()) and st.cpu().tolist() == [11, 4]


# ---- the site call through the C ABI --------------------------------------------------------------------------------------------------
class Site(MoeRun):
    """One site on the GPU; every call starts from the site's own BatchNorm buffers, poisoned workspaces and sentinel-filled outputs."""

    def __init__(self, cfg, P, B, X, Y, bf16):
        super().__init__(cfg, P, B, X, Y, bf16=bf16, training=True)
        self.stream = torch.cuda.current_stream().cuda_stream
        g = torch.Generator().manual_seed(41)
        self.dO = torch.randn(X.shape, generator=g).to(DEV, self.tdt).contiguous()
        self.dP = torch.randn(self.S, cfg.E, generator=g).to(DEV)

    def forward_by(self, entry, mix=None, k=0, renorm=1, prior=None):
        """entry "aux" / "reg" -> dict(out, probs, idx, lb, buffers); prior: `out` starts as this tensor and the call accumulates into it"""
        self.bufs = {kk: v.clone() for kk, v in self.buffers.items()}
        self.ptrs = cm.make_ptrs({**self.params, **self.bufs}, self.cfg.E_m, self.cfg.E_s)
        self.saved.fill_(0xFF)
        self.scratch.fill_(0xFF)
        nan = float("nan")
        self.out = prior.clone() if prior is not None else torch.full_like(self.X, nan)
        self.probs, self.idx = torch.full((self.S, self.cfg.E), nan, device=DEV), torch.full((self.S,), -7, device=DEV, dtype=torch.int64)
        self.lb = torch.full((1,), nan, device=DEV)
        self.desc.accumulate_out = int(prior is not None)
        head = (C.byref(self.desc), self.X.data_ptr(), self.Y.data_ptr(), C.byref(self.ptrs), None, k, renorm)
        tail = (self.out.data_ptr(), self.probs.data_ptr(), self.idx.data_ptr(), self.lb.data_ptr(), None, None, self.saved.data_ptr(),
                self.scratch.data_ptr(), self.stream)
        if entry == "aux":
            assert mix is None
            st = self.L.avmoe_moe_forward_aux(*head, *tail)
        else:
            st = self.L.avmoe_moe_forward_reg(*head, _ptr(mix), *tail)
        self.desc.accumulate_out = 0
        capi.check(st, "forward " + entry)
        torch.cuda.synchronize()
        assert self.guards_intact()
        return dict(out=self.out.clone(), probs=self.probs.clone(), idx=self.idx.clone(), lb=self.lb.clone(),
                    buffers={kk: v.clone() for kk, v in self.bufs.items()})

    def backward_by(self, entry, mix=None, dO=True, dprobs=True):
        """after forward_by -> {X, Y, parameter key: gradient} (fp32 on the CPU)"""
        dX, dY = torch.full_like(self.X, float("nan")), torch.full_like(self.Y, float("nan"))
        grads = {kk: torch.full_like(v, float("nan")) for kk, v in self.params.items()}
        gptrs = cm.make_ptrs(grads, self.cfg.E_m, self.cfg.E_s)
        head = (C.byref(self.desc), self.X.data_ptr(), self.Y.data_ptr(), C.byref(self.ptrs), self.dO.data_ptr() if dO else None,
                self.dP.data_ptr() if dprobs else None, None, None)
        tail = (self.saved.data_ptr(), self.scratch.data_ptr(), dX.data_ptr(), dY.data_ptr(), C.byref(gptrs), 0, self.stream)
        if entry == "aux":
            assert mix is None
            st = self.L.avmoe_moe_backward_aux(*head, *tail)
        else:
            st = self.L.avmoe_moe_backward_reg(*head, _ptr(mix), *tail)
        capi.check(st, "backward " + entry)
        torch.cuda.synchronize()
        assert self.guards_intact()
        return {**{kk: v.cpu() for kk, v in grads.items()}, "X": dX.float().cpu(), "Y": dY.float().cpu()}

    def step(self, entry, mix=None, k=0, renorm=1):
        f = self.forward_by(entry, mix, k, renorm)
        return f, self.backward_by(entry, mix)


def _tuned(use_bn=True):
    return O.AdapterConfig(Cx=768, Nx=520, Cy=768, Ny=64, reduction=12, groups=2, K=32, E_m=2, E_s=2, use_bn=use_bn)


def _site(which):
    """A: the fixture, fp32 ; B: the cfg-2 form in bf16, 2080 tokens ; B_nobn: B without BatchNorm.  Built once, inputs never modified."""
    if which not in _CACHE:
        if which == "A":
            meta, cfg, t = load_golden("ave_train")
            P, B = split_params(t)
            _CACHE[which] = Site(cfg, P, B, t["X"], t["Y"], bf16=False)
        else:
            cfg = _tuned(use_bn=which == "B")
            P, B = O.init_params(cfg, seed=3)
            g = torch.Generator().manual_seed(4)
            X, Y = 0.3 * torch.randn(4, cfg.Nx, cfg.Cx, generator=g), 0.3 * torch.randn(4, cfg.Ny, cfg.Cy, generator=g)
            _CACHE[which] = Site(cfg, P, B, X, Y, bf16=True)
    return _CACHE[which]


def _mask(site):
    return torch.from_numpy(R.hand_mask(site.S, site.cfg.E)).to(DEV)      # frame 0 dropped whole, frame 1 without any expert


def _same(a, b, what):
    for kk, v in a.items():
        if isinstance(v, dict):
            _same(v, b[kk], what + "/" + kk)
        else:
            assert torch.equal(v, b[kk]), f"{what}: {kk} differs"


@pytest.mark.parametrize("which,k", [("A", 0), ("A", 2), ("B", 0), ("B", 2)])
def test_all_ones_multiplier_equals_null(which, k):
    """out, probs, idx, lb, the advanced running statistics and every gradient: bit for bit"""
    site = _site(which)
    ones = torch.ones(site.S, site.cfg.E, device=DEV)
    f0, g0 = site.step("reg", None, k)
    f1, g1 = site.step("reg", ones, k)
    assert bool(torch.isfinite(f0["out"].float()).all()) and all(bool(torch.isfinite(v).all()) for v in g0.values())
    _same(f0, f1, "forward")
    _same(g0, g1, "backward")


@pytest.mark.parametrize("which,k", [("A", 0), ("A", 2), ("B", 0)])
def test_null_multiplier_is_the_older_entry_point(which, k):
    """avmoe_moe_forward_reg / _backward_reg with mix_scale = NULL == avmoe_moe_forward_aux / _backward_aux, `saved` included"""
    site = _site(which)
    f0, g0 = site.step("aux", None, k)
    sv0 = site.saved.clone()
    f1, g1 = site.step("reg", None, k)
    _same(f0, f1, "forward")
    _same(g0, g1, "backward")
    assert torch.equal(sv0, site.saved)


@pytest.fixture(scope="module")
def host():
    from avmoe_amd import build as b
    L = C.CDLL(b.build_host(verbose=False))
    L.avmoe_host_last_error.restype = C.c_char_p
    head = [C.POINTER(cm.MoeDesc), C.c_void_p, C.c_void_p, C.POINTER(cm.MoePtrs), C.c_void_p]
    L.avmoe_host_moe_forward_reg.restype = L.avmoe_host_moe_backward_reg.restype = C.c_int
    L.avmoe_host_moe_forward_reg.argtypes = head + [C.c_int32, C.c_int32] + [C.c_void_p] * 8
    L.avmoe_host_moe_backward_reg.argtypes = head + [C.c_void_p] * 8 + [C.POINTER(cm.MoePtrs), C.c_int32, C.c_int32]
    return L


def _host_step(H, site, mix, k, renorm):
    """the host twin on the site's inputs with the same multiplier -> (out, {gradients})"""
    cfg, S = site.cfg, site.S
    X, Y = site.X.float().cpu().contiguous(), site.Y.float().cpu().contiguous()
    params = {kk: v.cpu().contiguous() for kk, v in site.params.items()}
    bufs = {kk: v.cpu().clone().contiguous() for kk, v in site.buffers.items()}
    ptrs = cm.make_ptrs({**params, **bufs}, cfg.E_m, cfg.E_s)
    desc = make_desc(cfg, S, False, True)
    m = mix.cpu().contiguous()
    out = torch.empty_like(X)
    assert H.avmoe_host_moe_forward_reg(C.byref(desc), X.data_ptr(), Y.data_ptr(), C.byref(ptrs), None, k, renorm, m.data_ptr(), out.data_ptr(),
                                        None, None, None, None, None, None) == 0, H.avmoe_host_last_error()
    grads = {kk: torch.zeros_like(v) for kk, v in params.items()}
    gp = cm.make_ptrs(grads, cfg.E_m, cfg.E_s)
    dX, dY = torch.empty_like(X), torch.empty_like(Y)
    dO, dP = site.dO.float().cpu().contiguous(), site.dP.cpu().contiguous()
    assert H.avmoe_host_moe_backward_reg(C.byref(desc), X.data_ptr(), Y.data_ptr(), C.byref(ptrs), None, dO.data_ptr(), dP.data_ptr(), None, None,
                                         m.data_ptr(), None, dX.data_ptr(), dY.data_ptr(), C.byref(gp), k, renorm) == 0, H.avmoe_host_last_error()
    return out, {**grads, "X": dX, "Y": dY}


def _against_host(site, H, mix, k, renorm):
    """the bar of tests/test_host_vs_hip_gpu.py: out within 1e-3 (max-abs relative), every gradient within 1e-3 of max(its own largest
    entry, 1e-3 of the largest gradient entry of the site)"""
    f, got = site.step("reg", mix, k, renorm)
    out_h, ref = _host_step(H, site, mix, k, renorm)
    err = float((f["out"].float().cpu() - out_h).abs().max() / out_h.abs().max())
    gmax = max(float(v.abs().max()) for v in ref.values())
    errs = {kk: float((got[kk] - v).abs().max()) for kk, v in ref.items()}
    print(f"k={k} renorm={renorm}: out rel err {err:.3e}; worst gradient err / bar "
          f"{max(e / (1e-3 * max(float(ref[kk].abs().max()), 1e-3 * gmax)) for kk, e in errs.items()):.3f}")
    assert err < 1e-3
    bad = {kk: e for kk, e in errs.items() if e > 1e-3 * max(float(ref[kk].abs().max()), 1e-3 * gmax)}
    assert not bad, bad
    return f


def test_masked_site_against_the_host_twin(host):
    """A, fp32, a multiplier with a fully dropped frame (0) and a frame that lost every expert (1): out, dX, dY and every parameter gradient
    against the host twin; the rows of those frames in `out` exactly zero -- and with accumulation exactly the prior content --; probs,
    idx, lb and the BatchNorm running statistics bit-equal to the dense call."""
    site = _site("A")
    mix = _mask(site)
    f = _against_host(site, host, mix, 0, 1)
    assert bool((f["out"][:2] == 0).all()) and bool((f["out"][2:] != 0).any())
    dense = site.forward_by("aux")
    for kk in ("probs", "idx", "lb"):
        assert torch.equal(f[kk], dense[kk]), kk
    _same(f["buffers"], dense["buffers"], "running statistics")
    assert not torch.equal(f["out"], dense["out"])
    prior = torch.randn(site.X.shape, generator=torch.Generator().manual_seed(8)).to(DEV)
    acc = site.forward_by("reg", mix, prior=prior)
    assert torch.equal(acc["out"][:2], prior[:2])
    assert float((acc["out"][2:] - (prior[2:] + f["out"][2:])).abs().max()) <= 2.0 ** -22 * float(prior.abs().max() + f["out"].abs().max())


@pytest.mark.parametrize("renorm", [1, 0])
def test_topk_then_the_multiplier_against_the_host_twin(host, renorm):
    """top-k = 2 of 4 experts: the weights are top-k first, then the multiplier (the host twin applies them in that order)"""
    site = _site("A")
    f = _against_host(site, host, _mask(site), 2, renorm)
    assert bool((f["out"][:2] == 0).all())


def _expert_outputs(site):
    """(E, S, N, C) fp32: the library's own per-expert outputs (avmoe_expert_forward_cross / _uni), each from the site's own buffers"""
    outs = []
    for e in range(site.cfg.E):
        bufs = {kk: v.clone() for kk, v in site.buffers.items()}
        ptrs = cm.make_ptrs({**site.params, **bufs}, site.cfg.E_m, site.cfg.E_s)
        o = torch.full_like(site.X, float("nan"))
        fn, j = (site.L.avmoe_expert_forward_cross, e) if e < site.cfg.E_m else (site.L.avmoe_expert_forward_uni, e - site.cfg.E_m)
        capi.check(fn(C.byref(site.desc), site.X.data_ptr(), site.Y.data_ptr(), C.byref(ptrs), j, o.data_ptr(), site.saved.data_ptr(),
                      site.scratch.data_ptr(), site.stream), "expert_forward")
        torch.cuda.synchronize()
        outs.append(o.float())
    return torch.stack(outs)


def test_masked_bf16_site_against_its_own_masked_expert_sum():
    """B, bf16, streamed passes: out against sum_e m w expert_e accumulated in fp32 from the library's own per-expert outputs and its own
    probs -- the bar tests/test_moe_vs_oracle_midsize_gpu.py gives a bf16 site's out (1e-2, max-abs relative).  Dropped frames: zeros."""
    site = _site("B")
    mix = _mask(site)
    f = site.forward_by("reg", mix)
    ex = _expert_outputs(site)
    ref = ((mix * f["probs"]).t().reshape(site.cfg.E, site.S, 1, 1) * ex).sum(0)
    err = float((f["out"].float() - ref).abs().max() / ref.abs().max())
    print(f"bf16 masked out against the masked expert sum: {err:.3e}")
    assert err < 1e-2
    assert bool((f["out"][:2] == 0).all()) and float(ref[2:].abs().max()) > 0


def test_dropped_frames_get_only_the_router_term_without_batchnorm():
    """B without BatchNorm, bf16.  Nothing couples the frames then, so the dX / dY rows of a frame whose multipliers are all 0 carry the
    router's term alone: they are checked against the router-only backward (dOut = NULL) of the same call -- two bf16 roundings apart at
    most (each path rounds its fp32 value once), 2^-7 of the row's largest entry -- and every token of such a frame has the same dX row.
    (WITH train-mode BatchNorm the statement does not hold: the dropped frame's tokens still enter the batch statistics and the kept frames'
    gradients reach them through those -- tests/test_mix_drop_ref.py pins that term to central differences on the host twin.)"""
    site = _site("B_nobn")
    mix = _mask(site)
    site.forward_by("reg", mix)
    full = site.backward_by("reg", mix)
    site.forward_by("reg", mix)                               # (the same call again: the full backward has used the workspaces)
    router = site.backward_by("reg", mix, dO=False)
    for s in (0, 1):
        for t in ("X", "Y"):
            tol = 2.0 ** -7 * float(router[t][s].abs().max())
            assert float(router[t][s].abs().max()) > 0 and float((full[t][s] - router[t][s]).abs().max()) <= tol, (s, t)
        assert float((full["X"][s] - full["X"][s, :1]).abs().max()) == 0.0
    assert float((full["X"][2] - router["X"][2]).abs().max()) > 2.0 ** -7 * float(router["X"][2].abs().max())


# ---- the facade -----------------------------------------------------------------------------------------------------------------------
def _module(p, q, seed=None, name="ave_train"):
    meta, cfg, t = load_golden(name)
    P, B = split_params(t)
    m = build_module(meta["which"], cfg).to(DEV)
    m.load_state_dict({**P, **B}, strict=True)
    m.drop_path, m.expert_dropout = p, q
    if seed is not None:
        m.mix_seed = seed
    x4 = t["X"].to(DEV).permute(0, 2, 1).unsqueeze(-1)
    y4 = t["Y"].to(DEV).permute(0, 2, 1).unsqueeze(-1)
    return m, cfg, x4, y4, t


def test_facade_draws_a_fresh_mask_every_training_forward():
    m, cfg, x4, y4, t = _module(0.25, 0.5, seed=777)
    m.train()
    assert m.last_mix_scale is None and m.mix_calls == 0
    S, masks = x4.shape[0], []
    for i in range(2):
        out, _ = m(x4, y4)
        masks.append(m.last_mix_scale.clone())
        assert np.array_equal(masks[-1].cpu().numpy(), R.mix_scale(777, i, S, cfg.E, 0.25, 0.5))
        dropped = (masks[-1] == 0).all(-1)
        assert bool((out.squeeze(-1).permute(0, 2, 1)[dropped] == 0).all())
    assert not torch.equal(masks[0], masks[1]) and m.mix_calls == 2
    m.drop_path = m.expert_dropout = 0.0
    m(x4, y4)
    assert m.last_mix_scale is None and m.mix_calls == 2


def test_facade_refuses_a_backward_after_another_training_forward():
    m, cfg, x4, y4, t = _module(0.25, 0.5, seed=5)
    m.train()
    out1, _ = m(x4.clone().requires_grad_(True), y4)
    m(x4, y4)
    with pytest.raises(capi.AvmoeError, match="another training forward"):
        out1.sum().backward()


def test_facade_eval_mode_ignores_the_settings():
    m, cfg, x4, y4, t = _module(0.5, 0.5, seed=1)
    plain = copy.deepcopy(m)
    plain.drop_path = plain.expert_dropout = 0.0
    m.eval(), plain.eval()
    a, ia = m(x4, y4)
    b, ib = plain(x4, y4)
    assert torch.equal(a, b) and torch.equal(ia, ib) and m.last_mix_scale is None and m.mix_calls == 0


@pytest.mark.parametrize("mode", ["two_streams", "one_stream", "one_stream_add_to"])
def test_adapter_pair_equals_two_separate_calls_given_the_same_seeds(mode):
    """Each site's own setting and seed decide its draw, in the pair as in a call of its own: the masks are equal bit for bit, outputs and
    gradients to the bars tests/test_router_topk_gpu.py holds a pair to (fp32: 1e-5 on the tensors, 1e-4 on the parameter gradients)."""
    from avmoe_amd.adapters import AdapterPair
    kw = dict(E_m=2, E_s=2, groups=2, K=32, variant="ave", reduction=4)
    ca, cb = O.AdapterConfig(Cx=64, Nx=72, Cy=48, Ny=40, **kw), O.AdapterConfig(Cx=48, Nx=40, Cy=64, Ny=72, **kw)
    torch.manual_seed(5)
    sa, sb = build_module("ave", ca).to(DEV).train(), build_module("ave", cb).to(DEV).train()
    with torch.no_grad():
        for m in (sa, sb):
            for kk, p in m.named_parameters():
                if kk.endswith(("gate", "gate_av")):
                    p.fill_(0.3)
    sa.drop_path, sa.expert_dropout, sb.expert_dropout = 0.3, 0.2, 0.5
    ra, rb = copy.deepcopy(sa), copy.deepcopy(sb)
    for m, seed in ((sa, 101), (sb, 202), (ra, 101), (rb, 202)):
        m.mix_seed = seed
    g = torch.Generator().manual_seed(9)
    S = 6
    fa, fv = (0.5 * torch.randn(S, ca.Cx, ca.Nx, 1, generator=g)).to(DEV), (0.5 * torch.randn(S, cb.Cx, cb.Nx, 1, generator=g)).to(DEV)
    ga, gv = torch.randn(S, ca.Cx, ca.Nx, 1, generator=g).to(DEV), torch.randn(S, cb.Cx, cb.Nx, 1, generator=g).to(DEV)
    base = [torch.randn(S, c.Nx, c.Cx, generator=g).to(DEV) for c in (ca, cb)] if mode.endswith("add_to") else None
    xa, xv = fa.clone().requires_grad_(True), fv.clone().requires_grad_(True)
    oa, _ = ra(xa, xv)
    ov, _ = rb(xv, xa)
    if base is not None:
        oa, ov = oa + base[0].permute(0, 2, 1).unsqueeze(-1), ov + base[1].permute(0, 2, 1).unsqueeze(-1)
    torch.autograd.backward([oa, ov], [ga, gv])
    ya, yv = fa.clone().requires_grad_(True), fv.clone().requires_grad_(True)
    pair = AdapterPair(sa, sb, concurrent=mode == "two_streams")
    pa, _, pv, _ = pair(ya, yv, add_to=tuple(b.clone() for b in base) if base is not None else (None, None))
    torch.autograd.backward([pa, pv], [ga, gv])
    torch.cuda.synchronize()
    assert torch.equal(sa.last_mix_scale, ra.last_mix_scale) and torch.equal(sb.last_mix_scale, rb.last_mix_scale)
    assert bool((sa.last_mix_scale == 0).any()) and not torch.equal(sa.last_mix_scale, sb.last_mix_scale)
    for r_, g_ in ((oa, pa), (ov, pv), (xa.grad, ya.grad), (xv.grad, yv.grad)):
        assert float((r_ - g_).detach().abs().max()) <= 1e-5 * float(r_.detach().abs().max())
    for (kk, pr), (_, pg) in zip(list(ra.named_parameters()) + list(rb.named_parameters()), list(sa.named_parameters()) + list(sb.named_parameters())):
        assert float((pr.grad - pg.grad).abs().max()) <= 1e-4 * max(float(pr.grad.abs().max()), 1e-6), kk


def test_captured_facade_step_draws_a_fresh_mask_on_every_replay():
    """Forward + backward of a site with both regularisers through the facade, captured with torch.cuda.graph on one stream.  The draw's
    counter lives on the device, so three replays give three different masks; and every replay is, bit for bit, the eager C-ABI call
    (avmoe_moe_forward_reg / _backward_reg) made with the mask read back from that replay.

    (Three replays matter beyond the mask: the site backward clears its accumulators with a kernel of the library because the runtime's memset
    node, which it used before, cleared them on the first replay of a graph only -- csrc/moe_backward.cpp: MEMSET0.)"""
    m, cfg, x4, y4, t = _module(0.25, 0.5, seed=31337)
    m.train()
    m.shared_gpu = False                                      # (the capture stream is the only one at work: the launches of the eager call)
    P, B = split_params(t)
    G = t["grad_out"].to(DEV)
    X = t["X"].to(DEV).requires_grad_(True)
    Y = t["Y"].to(DEV).requires_grad_(True)

    def step():
        out, _ = m(X.permute(0, 2, 1).unsqueeze(-1), Y.permute(0, 2, 1).unsqueeze(-1))
        out = out.squeeze(-1).permute(0, 2, 1)
        out.backward(G)
        return out

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):                                    # warm-up on the capture stream: the site's state block and tensors exist
            step()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    X.grad = Y.grad = None
    m.zero_grad(set_to_none=True)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        out = step()
    torch.cuda.synchronize()
    calls0 = m.mix_calls                                      # capturing launches nothing
    assert calls0 == 2
    site = Site(cfg, P, B, t["X"], t["Y"], bf16=False)
    site.dO = G.contiguous()
    masks = []
    for i in range(3):
        graph.replay()
        torch.cuda.synchronize()
        mask = m.last_mix_scale.clone()
        assert np.array_equal(mask.cpu().numpy(), R.mix_scale(31337, calls0 + i, X.shape[0], cfg.E, 0.25, 0.5))
        masks.append(mask)
        f = site.forward_by("reg", mask)
        ref = site.backward_by("reg", mask, dprobs=False)
        assert torch.equal(out.detach(), f["out"]), i
        assert torch.equal(X.grad.cpu(), ref["X"]), i
        assert torch.equal(Y.grad.cpu(), ref["Y"]), i
        for kk, p in m.named_parameters():
            assert torch.equal(p.grad.cpu(), ref[kk]), (i, kk)
    assert m.mix_calls == calls0 + 3
    assert not torch.equal(masks[0], masks[1]) and not torch.equal(masks[1], masks[2]) and not torch.equal(masks[0], masks[2])
