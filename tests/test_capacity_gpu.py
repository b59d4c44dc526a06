"""Expert capacity behind top-k routing on the GPU (avmoe_moe_forward_capacity / avmoe_router_capacity, include/avmoe.h).  The sub-op alone,
exact: kept, demand, kept_count, cap_scale, thr, last and w against tests/capacity_ref.py at the wave, block and chunk edges of the select
kernel, sentinel words behind every output, every call made twice.  Whole sites: the reports exact from the library's own softmax, and the
call bit-equal -- outputs, the whole saved workspace, the BatchNorm statistics, every gradient -- to avmoe_moe_forward_bias with
mix_scale := the cap_scale it wrote.  And what surrounds it: capacity S, later forwards on the same workspace, the profiler's names, the
facade, a balancer beside it, AdapterPair, a captured graph, the CapacityMeter.  Every comparison in this file is exact."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

from avmoe_amd import _capi as capi
from avmoe_amd.adapters import router_capacity
from avmoe_amd.train import CapacityMeter, RouterBiasBalancer
from tests import capacity_ref as R
from tests.moe_gpu_util import MoeRun
from tests.test_adapters_api import build_module
from tests.test_expert_choice_gpu import _backward, _module, _module_psm_w, _nothing, _site_data, _words
from tests.test_router_topk_gpu import _forward_topk, _pair_cfgs, _prof_names
from tests.topk_families import FAMILIES

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
NAN = float("nan")
PAD = 64                                              # sentinel words behind every output of the sub-op
INT_SENTINEL = -0x5A5A5A5B
OUTPUTS = ("w", "cap_scale", "kept", "demand", "kept_count", "thr", "last")
POLICIES = (R.ORDER, R.PRIORITY)


def _p(t):
    return t.data_ptr() if t is not None else None


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV) if a is not None else None


# ---- 1. the sub-op alone, exact -------------------------------------------------------------------------------------------------------
def _subop(pd, S, E, k, bd, c, policy, mixd, w_in, want=OUTPUTS):
    """one avmoe_router_capacity call -> {name: numpy output}; every output has PAD sentinel words behind it, which must survive"""
    f32 = lambda n: torch.full((n + PAD,), NAN, device=DEV)
    i32 = lambda n: torch.full((n + PAD,), INT_SENTINEL, dtype=torch.int32, device=DEV)
    size = {"w": S * E, "cap_scale": S * E, "kept": S, "demand": E, "kept_count": E, "thr": E, "last": E}
    bufs = {n: (f32 if n in ("w", "cap_scale", "thr") else i32)(size[n]) for n in OUTPUTS}
    bufs["w"][:S * E] = w_in.reshape(-1)                  # in and out
    arg = lambda n: bufs[n].data_ptr() if n in want else None
    st = capi.lib().avmoe_router_capacity(pd.data_ptr(), S, E, k, _p(bd), c, policy, _p(mixd), arg("w"), arg("cap_scale"), arg("kept"),
                                          arg("demand"), arg("kept_count"), arg("thr"), arg("last"), _stream())
    capi.check(st, "avmoe_router_capacity")
    torch.cuda.synchronize()
    out = {}
    for n in OUTPUTS:
        host = bufs[n].cpu().numpy()
        tail = host[size[n]:]
        assert (np.isnan(tail).all() if host.dtype == np.float32 else (tail == INT_SENTINEL).all()), f"{n}: written past its end"
        if n in want:
            out[n] = host[:size[n]].reshape(S, E) if n in ("w", "cap_scale") else host[:size[n]]
        elif n != "w":
            assert (np.isnan(host).all() if host.dtype == np.float32 else (host == INT_SENTINEL).all()), f"{n}: written though NULL"
    return out


def _subop_twice(*a, what="", **kw):
    """the call made twice: the same bytes in every output"""
    first, again = _subop(*a, **kw), _subop(*a, **kw)
    for n, v in first.items():
        assert v.tobytes() == again[n].tobytes(), f"{what}: {n} differs between two identical calls"
    return first


@pytest.mark.parametrize("S", [1, 2, 63, 64, 65, 255, 256, 257, 1023, 1025, 4099])
def test_subop_is_exact_on_every_input_family(S):
    """E in {2, 4, 16}, k in {1, 2}, both policies, c in {1, max demand - 1, max demand, S} from the reference on the same input; every
    family plain and with a bias and a multiplier that has zeros.  From S = 63 on every family but `balanced` must show, in one and the
    same case, a dropped pair and an expert within its budget: a vacuous input fails here."""
    seen = {name: False for name in R.FAMILIES}
    for E in (2, 4, 16):
        mix, b = R.mix_for(S, E), R.bias_for(E)
        for k in (1, 2):
            if k >= E:
                continue
            for name in R.FAMILIES:
                p = R.family(name, S, E)
                pd = _dev(p)
                for bias, mx in ((None, None), (b, mix), (None, mix)):
                    m = R.select_mask(p, k, bias)
                    w_in = (np.where(m, p, np.float32(0)) * (mx if mx is not None else np.float32(1))).astype(np.float32)
                    bd, mixd, wd = _dev(bias), _dev(mx), _dev(w_in)
                    for c in R.capacities(m):
                        for policy in POLICIES:
                            what = f"{name} S={S} E={E} k={k} c={c} policy={policy} bias={bias is not None} mix={mx is not None}"
                            ref = R.reference(p, k, c, policy, b=bias, mix=mx)
                            got = _subop_twice(pd, S, E, k, bd, c, policy, mixd, wd, what=what)
                            try:
                                R.check_outputs(ref, E, w_in=w_in, **got)
                            except AssertionError as err:
                                raise AssertionError(f"{what}: {err}") from err
                            d, s = R.drops_and_slack(ref, c)
                            seen[name] |= d and s
                            if name == "balanced" and c >= int(ref["demand"].max()):
                                assert not d, what
    if S >= 63:
        weak = [n for n, ok in seen.items() if not ok and n != "balanced"]
        assert not weak, f"S={S}: no case of {weak} shows a dropped pair beside an expert within its budget"


def test_subop_every_optional_output_can_be_null_on_its_own():
    S, E, k, c = 300, 4, 2, 40
    p, b, mix = R.family("random", S, E), R.bias_for(E), R.mix_for(S, E)
    m = R.select_mask(p, k, b)
    w_in = (np.where(m, p, np.float32(0)) * mix).astype(np.float32)
    pd, bd, mixd, wd = _dev(p), _dev(b), _dev(mix), _dev(w_in)
    for policy in POLICIES:
        ref = R.reference(p, k, c, policy, b=b, mix=mix)
        assert R.drops_and_slack(ref, c)[0]
        for leave in OUTPUTS:
            got = _subop(pd, S, E, k, bd, c, policy, mixd, wd, want=tuple(n for n in OUTPUTS if n != leave))
            R.check_outputs(ref, E, w_in=w_in, **got)
        for only in OUTPUTS:
            R.check_outputs(ref, E, w_in=w_in, **_subop(pd, S, E, k, bd, c, policy, mixd, wd, want=(only,)))
        _subop(pd, S, E, k, bd, c, policy, mixd, wd, want=())


# ---- 2. whole sites ---------------------------------------------------------------------------------------------------------------------
def _aux_bufs(run, aux):
    run.aux, run.load = (torch.full((2,), NAN, device=DEV), torch.full((run.cfg.E,), NAN, device=DEV)) if aux else (None, None)


def _forward_bias(run, k, renorm, mix=None, bias=None, count=None, aux=False):
    """avmoe_moe_forward_bias on a MoeRun (mix: a DEVICE tensor or None)"""
    _aux_bufs(run, aux)
    run.mix = mix
    st = run.L.avmoe_moe_forward_bias(C.byref(run.desc), run.X.data_ptr(), run.Y.data_ptr(), C.byref(run.ptrs), _p(run.noise), k, int(renorm),
                                      _p(mix), _p(bias), _p(count), run.out.data_ptr(), run.probs.data_ptr(), run.idx.data_ptr(),
                                      run.lb.data_ptr(), _p(run.aux), _p(run.load), run.saved.data_ptr(), run.scratch.data_ptr(), _stream())
    capi.check(st, "avmoe_moe_forward_bias")
    torch.cuda.synchronize()
    return run


def _forward_capacity(run, k, renorm, c, policy, mix=None, bias=None, count=None, aux=False):
    """avmoe_moe_forward_capacity on a MoeRun; run.cap_scale / kept / demand / kept_count receive its reports (sentinels behind each)"""
    _aux_bufs(run, aux)
    S, E = run.S, run.cfg.E
    run.mix = mix
    run.cap_scale = torch.full((S * E + PAD,), NAN, device=DEV)
    run.kept = torch.full((S + PAD,), INT_SENTINEL, dtype=torch.int32, device=DEV)
    run.demand = torch.full((E + PAD,), INT_SENTINEL, dtype=torch.int32, device=DEV)
    run.kept_count = torch.full((E + PAD,), INT_SENTINEL, dtype=torch.int32, device=DEV)
    st = run.L.avmoe_moe_forward_capacity(C.byref(run.desc), run.X.data_ptr(), run.Y.data_ptr(), C.byref(run.ptrs), _p(run.noise), k, int(renorm),
                                          _p(mix), _p(bias), _p(count), c, policy, run.cap_scale.data_ptr(), run.kept.data_ptr(),
                                          run.demand.data_ptr(), run.kept_count.data_ptr(), run.out.data_ptr(), run.probs.data_ptr(),
                                          run.idx.data_ptr(), run.lb.data_ptr(), _p(run.aux), _p(run.load), run.saved.data_ptr(),
                                          run.scratch.data_ptr(), _stream())
    capi.check(st, "avmoe_moe_forward_capacity")
    torch.cuda.synchronize()
    assert bool(torch.isnan(run.cap_scale[S * E:]).all()) and all(bool((t[n:] == INT_SENTINEL).all()) for t, n in
                                                                   ((run.kept, S), (run.demand, E), (run.kept_count, E))), "a report written past its end"
    return run


def _psm(run):
    S, E = run.S, run.cfg.E
    return _words(run, "psm", torch.float32)[:S * E].reshape(S, E).numpy()


def _same_call(run, ref, what):
    """every output, the whole saved workspace (weights, psm, lse, mode words, BatchNorm tables) and the running statistics, bit for bit"""
    for n in ("out", "probs", "idx", "lb", "aux", "load"):
        a, b = getattr(run, n), getattr(ref, n)
        assert (a is None and b is None) or torch.equal(a, b), f"{what}: {n} differs"
    assert torch.equal(run.saved, ref.saved), f"{what}: the saved workspaces differ"
    for kk, v in run.buffers.items():
        assert torch.equal(v, ref.buffers[kk]), (what, kk)


def _same_grads(got, ref, what):
    for kk, v in ref.items():
        assert torch.equal(got[kk].contiguous().view(torch.int32), v.contiguous().view(torch.int32)), (what, kk)


def _crowded(noise):
    """the case's logit noise with expert 0 pushed to the top of every frame: its demand is S, so a capacity below S drops pairs"""
    noise = noise.clone()
    noise[:, 0] += 4.0
    return noise


# (policy, multiplier, bias and counts, auxiliary losses, dOut)
VARIANTS = ((R.ORDER, False, False, False, True), (R.PRIORITY, True, True, True, True), (R.ORDER, True, False, True, False),
            (R.PRIORITY, False, True, False, True))
SITES = [(w, None) for w in FAMILIES] + [("s300", False), ("s300", True), ("e16", False), ("e16", True)]


@pytest.mark.parametrize("which,force_bf16", SITES, ids=[w if f is None else f"{w}-{'bf16' if f else 'fp32'}" for w, f in SITES])
def test_site_call_equals_the_bias_call_with_cap_scale(which, force_bf16):
    cfg, S, bf16, P, B, X, Y, noise, _caps, dO, dP = _site_data(which)
    if force_bf16 is not None:
        bf16 = force_bf16
        if bf16:
            X, Y = X.to(torch.bfloat16).float(), Y.to(torch.bfloat16).float()
    E, k = cfg.E, 2
    noise = _crowded(noise)
    variants = VARIANTS[:2] if which == "s300" else VARIANTS
    with (capi.test_hooks(capi.HOOK_KFS_FORCE) if which == "tile_stream" else _nothing()):
        mk = lambda: MoeRun(cfg, P, B, X, Y, bf16=bf16, noise=noise)
        for policy, with_mix, with_bias, with_aux, with_out in variants:
            renorm = int(policy == R.PRIORITY)
            what = f"{which}/bf16={bf16}/policy={policy}/mix={with_mix}/bias={with_bias}/aux={with_aux}/dOut={with_out}"
            mix_np = R.mix_for(S, E) if with_mix else None
            b_np = (0.05 * R.bias_for(E)).astype(np.float32) if with_bias else None
            mixd, bd = _dev(mix_np), _dev(b_np)
            cnt = lambda: torch.zeros(E, device=DEV) if with_bias else None
            plain = _forward_bias(mk(), k, renorm, mixd, bd, None, aux=with_aux)      # the top-k call on the same data: its demand sets c
            m0 = R.select_mask(_psm(plain), k, b_np)
            c = int(m0.sum(0).max()) - 1
            assert c >= 1, what
            cnt_run = cnt()
            run = _forward_capacity(mk(), k, renorm, c, policy, mixd, bd, cnt_run, aux=with_aux)
            assert run.guards_intact(), what
            psm = _psm(run)
            ref = R.reference(psm, k, c, policy, b=b_np, mix=mix_np)
            dropped = int((ref["m"] & ~ref["keep"]).sum())
            print(f"{what}: c = {c}, demand {ref['demand'].tolist()}, {dropped} pairs dropped")
            assert dropped > 0, what + ": nothing was dropped"
            R.check_outputs(ref, E, kept=run.kept[:S].cpu().numpy(), demand=run.demand[:E].cpu().numpy(),
                            kept_count=run.kept_count[:E].cpu().numpy(), cap_scale=run.cap_scale[:S * E].cpu().numpy().reshape(S, E))
            w = _words(run, "probs", torch.float32)[:S * E].reshape(S, E).numpy()
            off = ref["m"] & ~ref["keep"]
            assert (w[off].view(np.uint32) == 0).all(), what + ": a dropped pair's weight is not +0.0f"
            lost = ~ref["keep"].any(1)                    # frames that lost every pair: output exactly 0
            if lost.any():
                assert float(run.out[_dev(lost)].float().abs().max()) == 0.0, what + ": out != 0 on a frame that lost every pair"
            if with_bias:
                assert torch.equal(cnt_run.cpu(), torch.from_numpy(ref["demand"].astype(np.float32))), what + ": select_count is not the demand"
            # the same call through the existing path: avmoe_moe_forward_bias with mix_scale := cap_scale
            cs = run.cap_scale[:S * E].clone()
            cnt_same = cnt()
            same = _forward_bias(mk(), k, renorm, cs, bd, cnt_same, aux=with_aux)
            _same_call(run, same, what)
            assert not with_bias or torch.equal(cnt_run, cnt_same)
            for n in ("probs", "idx", "lb", "aux", "load"):      # ... and what a capacity leaves alone is the plain top-k call's
                a_, b_ = getattr(run, n), getattr(plain, n)
                assert (a_ is None and b_ is None) or torch.equal(a_, b_), f"{what}: {n} is not the top-k call's"
            if (_words(plain, "probs", torch.float32)[:S * E].reshape(S, E).numpy()[off] != 0).any():      # (the multiplier may have zeroed them already)
                assert not torch.equal(run.out, plain.out), what + ": the capacity changed nothing"
            ag = (0.9, -1.1) if with_aux else None
            g_run = _backward(run, dO if with_out else None, dP, 0.5, ag, cs)
            g_same = _backward(same, dO if with_out else None, dP, 0.5, ag, cs)
            assert run.guards_intact(), what
            _same_grads(g_run, g_same, what)


@pytest.mark.parametrize("which", ["tile_fast", "e16"])
def test_capacity_S_is_the_topk_call_bitwise(which):
    """c = S drops nothing: every output, the saved workspace and every gradient are those of the top-k call run with a multiplier of ones"""
    cfg, S, bf16, P, B, X, Y, noise, _caps, dO, dP = _site_data(which)
    E, k = cfg.E, 2
    ones = torch.ones(S * E, device=DEV)
    for policy in POLICIES:
        mk = lambda: MoeRun(cfg, P, B, X, Y, bf16=bf16, noise=noise)
        ref = _forward_bias(mk(), k, 1, ones, None, None, aux=True)
        run = _forward_capacity(mk(), k, 1, S, policy, None, None, None, aux=True)
        m = R.select_mask(_psm(run), k)
        assert np.array_equal(R.mask_of_bits(run.kept[:S].cpu().numpy(), E), m)
        assert np.array_equal(run.demand[:E].cpu().numpy(), m.sum(0)) and torch.equal(run.demand[:E], run.kept_count[:E])
        _same_call(run, ref, f"{which}/policy={policy}")
        _same_grads(_backward(run, dO, dP, 0.5, (0.9, -1.1), run.cap_scale[:S * E].clone()), _backward(ref, dO, dP, 0.5, (0.9, -1.1), ones), which)


# ---- 3. surrounding behaviour -----------------------------------------------------------------------------------------------------------
def _small():
    cfg, S, bf16, P, B, X, Y, noise, caps, dO, dP = _site_data("tile_fast")
    return cfg, S, P, B, X, Y, _crowded(noise), dO, dP


def test_a_later_plain_forward_on_the_same_workspace_leaves_no_trace():
    cfg, S, P, B, X, Y, noise, dO, dP = _small()
    mk = lambda: MoeRun(cfg, P, B, X, Y, noise=noise, training=False)      # (eval-mode BatchNorm: a second forward sees the same statistics)
    for later in ("dense", "topk"):
        fwd = (lambda r: r.forward()) if later == "dense" else (lambda r: _forward_topk(r, 2, True))
        ref = fwd(mk())
        ref_saved = ref.saved.clone()                     # (before the backward, which works in parts of it)
        rg = _backward(ref, dO, dP, 0.5)
        run = _forward_capacity(mk(), 2, 1, 1, R.PRIORITY, _dev(R.mix_for(S, cfg.E)))
        assert int(run.kept_count[:cfg.E].sum()) < int(run.demand[:cfg.E].sum())
        fwd(run)
        assert torch.equal(run.out, ref.out)
        assert later == "dense" or torch.equal(run.saved, ref_saved)      # (a dense forward leaves psm alone: the top-k one rewrites all of it)
        _same_grads(_backward(run, dO, dP, 0.5), rg, later)


def test_profiler_names_three_more_in_the_forward_none_in_the_backward():
    cfg, S, P, B, X, Y, noise, dO, dP = _small()
    ones = torch.ones(S * cfg.E, device=DEV)
    r_reg, names_reg = _prof_names(lambda: _forward_bias(MoeRun(cfg, P, B, X, Y, noise=noise), 2, 1, ones))
    r_cap, names_cap = _prof_names(lambda: _forward_capacity(MoeRun(cfg, P, B, X, Y, noise=noise), 2, 1, 1, R.ORDER))
    new = [n for n in names_cap if n not in names_reg]
    assert set(names_reg) <= set(names_cap) and sorted(new) == ["k_cap_apply", "k_cap_mask", "k_cap_select"], new
    _, back_reg = _prof_names(lambda: _backward(r_reg, dO, dP, 0.5, None, ones))
    _, back_cap = _prof_names(lambda: _backward(r_cap, dO, dP, 0.5, None, r_cap.cap_scale))
    assert back_cap == back_reg, "the backward of a capacity forward adds no launch"


def _tokens4(X, Y):
    x4 = X.to(DEV).permute(0, 2, 1).unsqueeze(-1).contiguous().requires_grad_(True)
    y4 = Y.to(DEV).permute(0, 2, 1).unsqueeze(-1).contiguous().requires_grad_(True)
    return x4, y4


def test_facade_training_with_expert_dropout_eval_mode_and_the_meter():
    cfg, S, P, B, X, Y, noise, dO, dP = _small()
    E, k = cfg.E, 2
    m = _module(cfg, P, B)
    x4, y4 = _tokens4(X, Y)
    m.train()
    m.router_top_k = k
    m(x4, y4, is_training=True)
    assert m.last_capacity is None
    m.router_capacity_factor, m.router_capacity_policy, m.expert_dropout = 0.5, "priority", 0.4
    c = router_capacity(0.5, k, S, E)
    assert c == R.capacity(0.5, k, S, E) and c < S
    meter = CapacityMeter([m])
    torch.manual_seed(3)
    tot_d, tot_k, dropped = np.zeros(E, np.int64), np.zeros(E, np.int64), 0
    for i in range(3):
        out, idx, probs, lb = m(x4 if i == 0 else (x4 * (1.0 + 0.5 * i)).detach(), y4, is_training=True)
        rep = m.last_capacity
        assert rep.capacity == c and rep.kept.shape == (S,) and rep.demand.dtype == torch.int32 and not rep.kept.requires_grad
        psm, w = _module_psm_w(m, S, E)
        mix = m.__dict__["_mix_last"].cpu().numpy()
        ref = R.reference(psm, k, c, R.PRIORITY, mix=mix)
        R.check_outputs(ref, E, kept=rep.kept.cpu().numpy(), demand=rep.demand.cpu().numpy(), kept_count=rep.kept_count.cpu().numpy())
        assert (w[ref["m"] & ~ref["keep"]].view(np.uint32) == 0).all() and np.array_equal(w != 0, ref["keep"] & (mix != 0) & (psm != 0))
        assert np.array_equal(probs.reshape(S, E).detach().cpu().numpy(), psm)
        tot_d += ref["demand"]
        tot_k += ref["kept_count"]
        dropped += int((ref["m"] & ~ref["keep"]).sum())
        if i == 0:
            torch.autograd.backward([out, lb], [torch.randn_like(out), None])
            assert bool(torch.isfinite(x4.grad).all()) and float(x4.grad.abs().max()) > 0
            assert all(bool(torch.isfinite(p_.grad).all()) for p_ in m.parameters() if p_.grad is not None)
    assert dropped > 0, "the training forwards dropped nothing"
    # eval mode: the plain top-k call unless the eval factor is set; the meter counts training forwards only
    m.eval()
    with torch.no_grad():
        out_e = m(x4, y4, is_training=False)[0]
        assert m.last_capacity is None
        m.router_capacity_factor = None
        out_p = m(x4, y4, is_training=False)[0]
        assert torch.equal(out_e, out_p), "eval mode without an eval factor is not the plain top-k call"
        m.router_capacity_factor, m.router_capacity_eval_factor = 0.5, 0.25
        out_c = m(x4, y4, is_training=False)[0]
    rep = m.last_capacity
    assert rep is not None and rep.capacity == router_capacity(0.25, k, S, E)
    psm, w = _module_psm_w(m, S, E)
    ref = R.reference(psm, k, rep.capacity, R.PRIORITY)
    R.check_outputs(ref, E, kept=rep.kept.cpu().numpy(), demand=rep.demand.cpu().numpy(), kept_count=rep.kept_count.cpu().numpy())
    assert (ref["m"] & ~ref["keep"]).any() and not torch.equal(out_c, out_p)
    assert meter.calls == [3] and np.array_equal(meter.demand[0].cpu().numpy(), tot_d) and np.array_equal(meter.kept[0].cpu().numpy(), tot_k)
    want = np.where(tot_d > 0, (tot_d - tot_k) / np.maximum(tot_d, 1), 0.0)
    assert np.array_equal(meter.overflow()[0].numpy(), want)
    meter.reset()
    assert int(meter.demand[0].sum()) == 0
    meter.close()


def test_a_bias_balancer_beside_the_capacity_counts_demand():
    cfg, S, P, B, X, Y, noise, dO, dP = _small()
    E, k = cfg.E, 2
    m = _module(cfg, P, B)
    x4, y4 = _tokens4(X, Y)
    m.train()
    m.router_top_k, m.router_capacity_factor = k, 0.5
    bal = RouterBiasBalancer([m], rate=0.05)
    with torch.no_grad():
        bal.bias[0, :E] = torch.tensor((0.05 * R.bias_for(E)).tolist(), device=DEV)
    out = m(x4, y4, is_training=True)[0]
    rep = m.last_capacity
    psm, _w = _module_psm_w(m, S, E)
    ref = R.reference(psm, k, rep.capacity, R.ORDER, b=bal.bias[0, :E].cpu().numpy())
    R.check_outputs(ref, E, kept=rep.kept.cpu().numpy(), demand=rep.demand.cpu().numpy(), kept_count=rep.kept_count.cpu().numpy())
    assert torch.equal(bal.counts[0, :E].cpu(), torch.from_numpy(ref["demand"].astype(np.float32))), "the balancer does not see the demand"
    assert (ref["m"] & ~ref["keep"]).any()
    out.backward(torch.randn_like(out))
    before = bal.bias.clone()
    bal.step()
    torch.cuda.synchronize()
    assert not torch.equal(bal.bias, before) and float(bal.counts.abs().max()) == 0.0
    bal.detach()


def test_adapter_pair_with_capacity_sites_equals_two_sites():
    """The back-to-back pair (one stream: the launches of two separate site calls) with capacity sites: the reports, the outputs and every
    gradient are those of the two sites called one after the other."""
    from avmoe_amd.adapters import AdapterPair
    ca, cb = _pair_cfgs(True)
    torch.manual_seed(5)
    sa, sb = build_module("avs", ca).to(DEV).train(), build_module("avs", cb).to(DEV).train()
    for m_, pol in ((sa, "order"), (sb, "priority")):
        m_.router_top_k, m_.router_capacity_factor, m_.router_capacity_policy = 2, 0.5, pol
    with torch.no_grad():
        for m in (sa, sb):
            for kk, p in m.named_parameters():
                if kk.endswith(("gate", "gate_av")):
                    p.fill_(0.3)
    ra, rb = copy.deepcopy(sa), copy.deepcopy(sb)
    g = torch.Generator().manual_seed(9)
    S = 8
    fa = (0.5 * torch.randn(S, ca.Cx, ca.Nx, 1, generator=g)).to(DEV)
    fv = (0.5 * torch.randn(S, cb.Cx, cb.Nx, 1, generator=g)).to(DEV)
    ga, gv = torch.randn(S, ca.Cx, ca.Nx, 1, generator=g).to(DEV), torch.randn(S, cb.Cx, cb.Nx, 1, generator=g).to(DEV)
    bufs = [{kk: b.clone() for kk, b in m.named_buffers()} for m in (sa, sb)]

    def run(a, b, pair):
        for m, bb_ in zip((a, b), bufs):
            m.zero_grad(set_to_none=True)
            m.load_state_dict({**m.state_dict(), **bb_})
        torch.manual_seed(77)
        xa, xv = fa.clone().requires_grad_(True), fv.clone().requires_grad_(True)
        if pair is not None:
            oa, ia, pa_, la, ov, iv, pv_, lv = pair(xa, xv, is_training=True)
        else:
            oa, ia, pa_, la, ov, iv, pv_, lv = (*a(xa, xv, is_training=True), *b(xv, xa, is_training=True))
        reps = tuple(None if m.last_capacity is None else tuple(t.clone() for t in m.last_capacity[1:]) for m in (a, b))
        torch.autograd.backward([oa, ov, 0.7 * la + 1.3 * lv], [ga, gv, None])
        return ((oa.detach(), ov.detach()), (xa.grad, xv.grad), [p.grad.clone() for m in (a, b) for p in m.parameters()], reps)

    ref = run(ra, rb, None)
    got = run(sa, sb, AdapterPair(sa, sb, concurrent=False))
    for r_, g_ in zip(ref[3], got[3]):
        assert all(torch.equal(x_, y_) for x_, y_ in zip(r_, g_)), "the pair's capacity reports are not the single sites'"
    for rep in got[3]:
        assert int(rep[2].sum()) < int(rep[1].sum()), "a site of the pair dropped nothing"
    for i, (r_, g_) in enumerate(zip(ref[0] + ref[1] + tuple(ref[2]), got[0] + got[1] + tuple(got[2]))):
        assert torch.equal(r_, g_), i
    got2 = run(sa, sb, AdapterPair(sa, sb, concurrent=True))      # two streams: the same selection, reports and all
    for r_, g_ in zip(ref[3], got2[3]):
        assert all(torch.equal(x_, y_) for x_, y_ in zip(r_, g_)), "the two-stream pair's capacity reports are not the single sites'"
    sa.router_capacity_factor = sb.router_capacity_factor = None      # the capacity did something: the plain top-k pair differs
    plain = run(sa, sb, AdapterPair(sa, sb, concurrent=False))
    assert plain[3] == (None, None) and not torch.equal(plain[0][0], got[0][0])


def test_captured_facade_step_with_a_capacity_replays_bitwise():
    """One small single-stream site through the FACADE -- which allocates cap_scale and the reports in every call -- with a capacity, a meter
    attached, forward + backward captured with torch.cuda.graph: three replays equal the eager step bit for bit in the output, the
    reports, the token and the parameter gradients, and the meter has counted every replay."""
    from tests.golden_util import load_golden, split_params
    meta, cfg, t = load_golden("ave_train")
    P, B = split_params(t)
    m = build_module(meta["which"], cfg).to(DEV)
    m.load_state_dict({**P, **B}, strict=True)
    m.train()
    m.shared_gpu = False
    m.router_top_k, m.router_capacity_factor, m.router_capacity_policy = 1, 0.5, "priority"
    meter = CapacityMeter([m])
    G = t["grad_out"].to(DEV)
    X, Y = t["X"].to(DEV).requires_grad_(True), t["Y"].to(DEV).requires_grad_(True)

    def step():
        out, _ = m(X.permute(0, 2, 1).unsqueeze(-1), Y.permute(0, 2, 1).unsqueeze(-1))
        out = out.squeeze(-1).permute(0, 2, 1)
        out.backward(G)
        return out

    def clear():
        X.grad = Y.grad = None
        m.zero_grad(set_to_none=True)

    def snapshot(out):
        torch.cuda.synchronize()
        return [out.detach().clone()] + [t_.clone() for t_ in m.last_capacity[1:]] + [X.grad.clone(), Y.grad.clone()] + \
               [p_.grad.clone() for p_ in m.parameters()]

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):                                # warm-up on the capture stream
            step()
            clear()
        eager = snapshot(step())
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    demand, kept = eager[2].cpu().numpy().astype(np.int64), eager[3].cpu().numpy().astype(np.int64)
    assert kept.sum() < demand.sum() and float(eager[0].abs().max()) > 0, (demand, kept)
    clear()
    meter.reset()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        out = step()
    for i in range(3):
        graph.replay()
        for j, (a_, b_) in enumerate(zip(snapshot(out), eager)):
            assert torch.equal(a_, b_), (i, j)
    assert np.array_equal(meter.demand[0].cpu().numpy(), 3 * demand) and np.array_equal(meter.kept[0].cpu().numpy(), 3 * kept)
    meter.close()
