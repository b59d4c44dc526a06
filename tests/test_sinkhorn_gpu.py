"""Sinkhorn-balanced top-k routing on the GPU (avmoe_moe_forward_sinkhorn / avmoe_router_sinkhorn, include/avmoe.h).  The sub-op alone:
the column scale v against the fp64 reference of tests/sinkhorn_ref.py within 2 n (S + E + 4) 2^-24 -- at S = 4099 also within 8 x the
error of the reference's own fp32 run --, and, GIVEN the kernel's v, the mask, the bitmask, the counts and the weights exact, with NaN
sentinels behind every output and every call made twice.  Whole sites in the four bottleneck-space kernel families, at S = 300 and at
E = 16: everything but the weights bit-equal to avmoe_moe_forward_reg, the mode words, outputs and gradients against the eager reference
given the kernel's mask.  And what surrounds it: a later plain forward on the same workspace, the profiler's names, the facade, AdapterPair,
a captured step."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

from avmoe_amd import _capi as capi
from avmoe_amd import _capi_moe as cm
from avmoe_amd.train import sinkhorn_scale, sinkhorn_topk
from tests import expert_choice_ref as ER
from tests import sinkhorn_ref as R
from tests import test_expert_choice_gpu as EC        # (as a module: its helpers, not its tests)
from tests.moe_gpu_util import MoeRun
from tests.router_grad_util import assert_close
from tests.test_adapters_api import build_module
from tests.test_router_topk_gpu import _bf16_budget, _close, _dense_bf16, _forward_topk, _pair_cfgs, _prof_names
from tests.topk_families import FAMILIES

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
NAN = float("nan")
PAD = 64                                              # sentinel words behind every output of the sub-op
INT_SENTINEL = -0x5A5A5A5B
SIZES = {"w": lambda S, E: S * E, "choice": lambda S, E: S, "count": lambda S, E: E, "v": lambda S, E: E}


def _p(t):
    return t.data_ptr() if t is not None else None


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ---- 1. the sub-op alone ----------------------------------------------------------------------------------------------------------------
def _subop(pd, S, E, k, renorm, iters, mixd, want=("w", "choice", "count")):
    """one avmoe_router_sinkhorn call -> {name: numpy output}; every output has PAD sentinel words behind it, which must survive"""
    bufs = {"w": torch.full((S * E + PAD,), NAN, device=DEV), "choice": torch.full((S + PAD,), INT_SENTINEL, dtype=torch.int32, device=DEV),
            "count": torch.full((E + PAD,), INT_SENTINEL, dtype=torch.int32, device=DEV), "v": torch.full((E + PAD,), NAN, device=DEV)}
    want = tuple(want) + ("v",)
    arg = lambda n: bufs[n].data_ptr() if n in want else None
    st = capi.lib().avmoe_router_sinkhorn(pd.data_ptr(), S, E, k, renorm, iters, _p(mixd), arg("w"), arg("choice"), arg("count"), arg("v"), _stream())
    capi.check(st, "avmoe_router_sinkhorn")
    torch.cuda.synchronize()
    out = {}
    for n, size in SIZES.items():
        host = bufs[n].cpu().numpy()
        tail = host[size(S, E) if n in want else 0:]
        assert (np.isnan(tail).all() if host.dtype == np.float32 else (tail == INT_SENTINEL).all()), f"{n}: written past its end (or though NULL)"
        if n in want:
            out[n] = host[:size(S, E)].reshape(S, E) if n == "w" else host[:size(S, E)]
    return out


def _subop_twice(pd, S, E, k, renorm, iters, mixd, what, **kw):
    """the call made twice: the same bits in v, w, choice and count"""
    first, again = _subop(pd, S, E, k, renorm, iters, mixd, **kw), _subop(pd, S, E, k, renorm, iters, mixd, **kw)
    for n, v in first.items():
        assert v.tobytes() == again[n].tobytes(), f"{what}: {n} differs between two identical calls (renorm {renorm}, multiplier {mixd is not None})"
    return first


@pytest.mark.parametrize("S", [1, 2, 63, 64, 65, 257, 1023, 1025, 4099])
def test_subop_scale_within_the_bound_and_selection_exact(S):
    """E in {2, 3, 4, 16}, k in {1, E - 1}, n in {1, 3}, every input family: v within the bound (S = 4099: also within 8 x the reference's
    own fp32 error -- the kernel sums short serial runs before its tree), and given the kernel's v everything else exact."""
    worst = {}
    for E in (2, 3, 4, 16):
        mix = R.mix_for(S, E)
        mixd = torch.from_numpy(mix).to(DEV)
        for name in R.FAMILIES:
            p = R.family(name, S, E)
            pd = torch.from_numpy(p).to(DEV)
            for n in (1, 3):
                ref64 = R.scale_fp64(p, n)
                for k in sorted({1, E - 1}):
                    what = f"{name} S={S} E={E} k={k} n={n}"
                    try:
                        first = _subop_twice(pd, S, E, k, 0, n, None, what)
                        err = R.check_scale(p, n, first["v"], ref64)
                        if S == 4099:
                            err32 = R.log_error(R.scale_fp32(p, n), ref64)
                            print(f"{what}: max |log(v / v_fp64)| = {err:.3e}, the reference in fp32 {err32:.3e}, bound {R.v_bound(S, E, n):.3e}")
                            assert err <= 8 * err32, f"v is {err:.3e} from fp64, above 8 x the fp32 reference's {err32:.3e}"
                        worst[(E, n)] = max(worst.get((E, n), 0.0), err)
                        R.check_selection(p, first["v"], k, 0, None, first["choice"], first["count"], first["w"])
                        if name == "uniform":
                            assert (first["choice"] == (1 << k) - 1).all(), "all ties: the first k experts"
                        if name == "zero_column":
                            assert first["v"][E // 2] == np.float32(R.FLT_MAX), "the clamp"
                        for renorm, m_np, m_d, want in ((1, None, None, ("w",)), (1, mix, mixd, ("w", "count")), (0, mix, mixd, ("w", "choice"))):
                            got = _subop_twice(pd, S, E, k, renorm, n, m_d, what, want=want)
                            assert got["v"].tobytes() == first["v"].tobytes(), "v depends on what else was asked for"
                            R.check_selection(p, got["v"], k, renorm, m_np, got.get("choice"), got.get("count"), got["w"])
                    except AssertionError as err_:
                        raise AssertionError(f"{what}: {err_}") from err_
    print(f"S = {S}: worst max |log(v / v_fp64)| per (E, n): " + ", ".join(f"{kk}: {v:.2e}" for kk, v in sorted(worst.items())))


@pytest.mark.parametrize("E", [2, 16])
def test_subop_on_both_sides_of_the_lds_resident_limit(E):
    """kk_sk_scale keeps p in the LDS while 272 floats of reduction scratch and S rows of E | 1 floats fit in 152 KB, else it reads p from
    global memory in every round: the largest S of the first form and the smallest of the second (E = 16: 2272 / 2273 -- the largest
    dynamic LDS request --, E = 2: 12880 / 12881), same bound, same exact selection."""
    limit = (152 * 1024 // 4 - 272) // (E | 1)
    for S in (limit, limit + 1):
        p = R.family("skewed", S, E)
        pd = torch.from_numpy(p).to(DEV)
        for n in (1, 3):
            got = _subop_twice(pd, S, E, E - 1, 1, n, None, f"S={S} E={E} n={n}")
            err = R.check_scale(p, n, got["v"])
            err32 = R.log_error(R.scale_fp32(p, n), R.scale_fp64(p, n))
            print(f"S={S} E={E} n={n}: max |log(v / v_fp64)| = {err:.3e}, the reference in fp32 {err32:.3e}, bound {R.v_bound(S, E, n):.3e}")
            R.check_selection(p, got["v"], E - 1, 1, None, got["choice"], got["count"], got["w"])


def test_subop_as_functions_and_v_alone():
    """train.sinkhorn_scale / sinkhorn_topk are the sub-op with v / choice asked for; v alone runs the first launch only."""
    S, E, k, n = 320, 4, 1, 3
    p = R.family("skewed", S, E)
    pd = torch.from_numpy(p).to(DEV)
    v = sinkhorn_scale(pd, n)
    assert v.dtype == torch.float32 and v.shape == (E,)
    R.check_scale(p, n, v.cpu().numpy())
    alone = _subop(pd, S, E, k, 0, n, None, want=())
    assert alone["v"].tobytes() == v.cpu().numpy().tobytes()
    m = sinkhorn_topk(pd, k, n)
    assert m.dtype == torch.bool and m.shape == (S, E) and np.array_equal(m.cpu().numpy(), R.select_mask(p, v.cpu().numpy(), k))
    plain, balanced = R.largest_share(R.select_mask(p, np.ones(E, np.float32), k)), R.largest_share(m.cpu().numpy())
    print(f"largest expert share {plain:.2f} -> {balanced:.2f}")
    assert plain >= 0.45 and balanced <= 0.30
    with pytest.raises(capi.AvmoeError, match="top_k"):
        sinkhorn_topk(pd, E, n)
    with pytest.raises(capi.AvmoeError, match="iters"):
        sinkhorn_scale(pd, 65)


# ---- 2. whole sites ---------------------------------------------------------------------------------------------------------------------
ITERS = 3


def _forward_reg(run, k, renorm, mix=None, aux=False):
    """avmoe_moe_forward_reg: the plain top-k call with the same arguments"""
    run.aux, run.load = (torch.full((2,), NAN, device=DEV), torch.full((run.cfg.E,), NAN, device=DEV)) if aux else (None, None)
    run.mix = torch.as_tensor(mix).to(DEV, torch.float32).contiguous() if mix is not None else None
    st = run.L.avmoe_moe_forward_reg(C.byref(run.desc), run.X.data_ptr(), run.Y.data_ptr(), C.byref(run.ptrs), _p(run.noise), k, int(renorm),
                                     _p(run.mix), run.out.data_ptr(), run.probs.data_ptr(), run.idx.data_ptr(), run.lb.data_ptr(), _p(run.aux),
                                     _p(run.load), run.saved.data_ptr(), run.scratch.data_ptr(), _stream())
    capi.check(st, "avmoe_moe_forward_reg")
    torch.cuda.synchronize()
    return run


def _forward_sinkhorn(run, k, renorm, iters=ITERS, mix=None, aux=False, sync=True):
    """avmoe_moe_forward_sinkhorn on a MoeRun; run.choice / run.count receive the reports"""
    run.aux, run.load = (torch.full((2,), NAN, device=DEV), torch.full((run.cfg.E,), NAN, device=DEV)) if aux else (None, None)
    run.choice = torch.full((run.S + PAD,), INT_SENTINEL, dtype=torch.int32, device=DEV)
    run.count = torch.full((run.cfg.E + PAD,), INT_SENTINEL, dtype=torch.int32, device=DEV)
    run.mix = torch.as_tensor(mix).to(DEV, torch.float32).contiguous() if mix is not None else None
    st = run.L.avmoe_moe_forward_sinkhorn(C.byref(run.desc), run.X.data_ptr(), run.Y.data_ptr(), C.byref(run.ptrs), _p(run.noise), k, int(renorm),
                                          iters, _p(run.mix), run.out.data_ptr(), run.probs.data_ptr(), run.idx.data_ptr(), run.lb.data_ptr(),
                                          _p(run.aux), _p(run.load), run.choice.data_ptr(), run.count.data_ptr(), run.saved.data_ptr(),
                                          run.scratch.data_ptr(), _stream())
    capi.check(st, "avmoe_moe_forward_sinkhorn")
    if sync:
        torch.cuda.synchronize()
    return run


def _check_selection(run, k, renorm, iters, mix):
    """the mode words, v within the bound on the library's own psm, and mask / counts / weights exact given that v -> the mask"""
    S, E = run.S, run.cfg.E
    psm, w = EC._psm_w(run)
    mode = EC._words(run, "mode", torch.int32).numpy()
    assert (mode[0], mode[1], mode[2], mode[3], mode[5]) == (k, int(renorm), 2, 0, iters), mode[:6]
    v = mode[16:16 + E].copy().view(np.float32)
    R.check_scale(psm, iters, v)
    choice, count = run.choice.cpu().numpy(), run.count.cpu().numpy()
    assert (choice[S:] == INT_SENTINEL).all() and (count[E:] == INT_SENTINEL).all(), "choice / count written past their ends"
    return R.check_selection(psm, v, k, renorm, mix, choice[:S], count[:E], w)


# (k, renorm, multiplier, auxiliary gradients, dOut): a router-only backward and backwards with a multiplier among them
VARIANTS = ((1, 0, False, False, True), (2, 1, True, True, True), (2, 1, False, True, False), (1, 0, True, False, False))


@pytest.mark.parametrize("which", list(FAMILIES) + ["s300", "e16"])
def test_site_with_sinkhorn_routing(which):
    cfg, S, bf16, P, B, X, Y, noise, _caps, dO, dP = EC._site_data(which)
    E = cfg.E
    with (capi.test_hooks(capi.HOOK_KFS_FORCE) if which == "tile_stream" else EC._nothing()):
        mk = lambda: MoeRun(cfg, P, B, X, Y, bf16=bf16, noise=noise)
        dense_pair = _dense_bf16(mk().forward(), cfg, P, B, X, Y, dO, dP, 0.5, True, noise, None) if bf16 else None
        for k, renorm, with_mix, with_aux, with_out in VARIANTS:
            what = f"{which}/k={k}/renorm={renorm}/mix={with_mix}/aux={with_aux}/dOut={with_out}"
            mix = ER.mix_for(S, E) if with_mix else None
            plain = _forward_reg(mk(), k, renorm, mix, aux=True)
            run = _forward_sinkhorn(mk(), k, renorm, ITERS, mix, aux=True)
            assert run.guards_intact(), what
            assert np.array_equal(EC._psm_w(run)[0], plain.probs.cpu().numpy()), what + ": psm is not the dense softmax"
            mask = _check_selection(run, k, renorm, ITERS, mix)
            if which == "s300":
                before, after = R.largest_share(R.select_mask(EC._psm_w(run)[0], np.ones(E, np.float32), k)), R.largest_share(mask)
                print(f"{what}: largest expert share {before:.2f} -> {after:.2f}")
                assert after <= before
            for n in ("probs", "idx", "lb", "aux", "load"):
                assert torch.equal(getattr(run, n), getattr(plain, n)), f"{what}: {n} is not avmoe_moe_forward_reg's"
            for kk, v in run.buffers.items():             # BatchNorm running statistics: the plain call's, bit for bit
                assert torch.equal(v, plain.buffers[kk]), (what, kk)
            for nb in EC.BN_BATCH:                        # ... and the batch statistics the forward left in its workspace
                assert torch.equal(EC._raw(run, nb), EC._raw(plain, nb)), f"{what}: BatchNorm batch statistics `{nb}` are not the plain call's"
            load = plain.load.cpu()
            ag = (0.9, -1.1) if with_aux else None
            got = EC._backward(run, dO if with_out else None, dP, 0.5, ag, run.mix)
            assert run.guards_intact(), what
            got["out"] = run.out.float().cpu()
            ref = ER.site_reference(cfg, P, B, X, Y, dO if with_out else None, dP, 0.5, mask, renorm, mix, ag, load, noise=noise)
            if bf16:
                eager = EC._eager_bf16_ec(cfg, P, B, X, Y, dO if with_out else None, dP, 0.5, mask, renorm, mix, ag, load, noise)
                _bf16_budget(got, ref, eager, dense_pair if with_out else (ref, ref), what)
            else:
                _close(got.pop("out"), ref.pop("out"), 1e-3, what + "/out")
                assert_close(got, ref, rtol=1e-3, floor_frac=1e-2, what=what)


# ---- 3. surrounding behaviour -----------------------------------------------------------------------------------------------------------
def test_a_later_plain_topk_forward_on_the_same_workspace_switches_the_mode_off():
    cfg, S, P, B, X, Y, noise, dO, dP = EC._small()
    mk = lambda: MoeRun(cfg, P, B, X, Y, noise=noise, training=False)      # (eval-mode BatchNorm: a second forward sees the same statistics)
    ref = _forward_topk(mk(), 2, True)
    rg = EC._backward(ref, dO, dP, 0.5)
    run = _forward_sinkhorn(mk(), 2, 1, ITERS, ER.mix_for(S, cfg.E))
    mode = EC._words(run, "mode", torch.int32)
    assert mode[2] == 2 and mode[5] == ITERS
    sk_out = run.out.clone()
    _forward_topk(run, 2, True)
    mode = EC._words(run, "mode", torch.int32)
    assert (int(mode[0]), int(mode[1]), int(mode[2]), int(mode[5])) == (2, 1, 0, 0), mode[:6]
    assert torch.equal(run.out, ref.out) and not torch.equal(run.out, sk_out)
    got = EC._backward(run, dO, dP, 0.5)
    for kk, v in rg.items():
        assert torch.equal(got[kk], v), kk


def test_profiler_names_two_more_in_the_forward_none_in_the_backward():
    cfg, S, P, B, X, Y, noise, dO, dP = EC._small()
    r_reg, names_reg = _prof_names(lambda: _forward_reg(MoeRun(cfg, P, B, X, Y, noise=noise), 2, 1))
    r_sk, names_sk = _prof_names(lambda: _forward_sinkhorn(MoeRun(cfg, P, B, X, Y, noise=noise), 2, 1))
    new = [n for n in names_sk if n not in names_reg]
    assert set(names_reg) <= set(names_sk) and sorted(new) == ["k_sk_apply", "k_sk_scale"], new
    _, back_reg = _prof_names(lambda: EC._backward(r_reg, dO, dP, 0.5))
    _, back_sk = _prof_names(lambda: EC._backward(r_sk, dO, dP, 0.5))
    assert back_sk == back_reg, "the backward of a Sinkhorn forward adds no launch"


def _tokens4(X, Y):
    x4 = X.to(DEV).permute(0, 2, 1).unsqueeze(-1).contiguous().requires_grad_(True)
    y4 = Y.to(DEV).permute(0, 2, 1).unsqueeze(-1).contiguous().requires_grad_(True)
    return x4, y4


def _module_mode(m):
    desc, saved = m.__dict__["_last_saved"]
    off = next(o for n, _r, o, _b in cm.buffer_table(capi.lib(), desc) if n == "mode")
    torch.cuda.synchronize()
    return saved[off:off + 256].view(torch.int32).cpu().numpy()


def test_facade_training_with_expert_dropout_eval_fallback_and_eval_on():
    cfg, S, P, B, X, Y, noise, dO, dP = EC._small()
    E = cfg.E
    m = EC._module(cfg, P, B)
    x4, y4 = _tokens4(X, Y)
    m.train()
    m.router_top_k, m.router_top_k_renorm = 2, True
    m(x4, y4, is_training=True)
    assert m.last_sinkhorn is None
    m.router_sinkhorn, m.expert_dropout, m.router_aux = 4, 0.4, True
    torch.manual_seed(3)
    out, idx, probs, lb = m(x4, y4, is_training=True)
    rep = m.last_sinkhorn
    assert rep.scale.dtype == torch.float32 and rep.scale.shape == (E,) and rep.count.dtype == torch.int32 and rep.count.shape == (E,)
    assert rep.choice.dtype == torch.int32 and rep.choice.shape == (S,) and not rep.scale.requires_grad
    psm, w = EC._module_psm_w(m, S, E)
    mode = _module_mode(m)
    assert (mode[0], mode[1], mode[2], mode[5]) == (2, 1, 2, 4)
    v = rep.scale.cpu().numpy()
    assert np.array_equal(mode[16:16 + E].view(np.uint32), v.view(np.uint32)), "last_sinkhorn.scale is not the words the forward used"
    R.check_scale(psm, 4, v)
    mix = m.__dict__["_mix_last"].cpu().numpy()
    assert (mix == 0).any() and (mix != 0).any(), "the expert-dropout draw shows nothing"
    R.check_selection(psm, v, 2, 1, mix, rep.choice.cpu().numpy(), rep.count.cpu().numpy(), w)
    assert int(rep.count.sum()) == 2 * S
    assert np.array_equal(probs.reshape(S, E).detach().cpu().numpy(), psm) and m.last_router_aux is not None
    torch.autograd.backward([out, lb], [torch.randn_like(out), None])
    assert bool(torch.isfinite(x4.grad).all()) and float(x4.grad.abs().max()) > 0
    assert all(bool(torch.isfinite(p_.grad).all()) for p_ in m.parameters() if p_.grad is not None)
    # eval mode: plain top-k, bit for bit (a balanced assignment depends on the rest of the batch)
    m.eval()
    with torch.no_grad():
        out_e = m(x4, y4, is_training=False)[0]
        assert m.last_sinkhorn is None and _module_mode(m)[2] == 0
        m.router_sinkhorn = None
        out_p = m(x4, y4, is_training=False)[0]
        assert torch.equal(out_e, out_p), "eval mode with router_sinkhorn set is not the plain top-k site"
        # ... unless router_sinkhorn_eval keeps it on: the C ABI's call on the same inputs
        m.router_sinkhorn, m.router_sinkhorn_eval = 4, True
        out_s = m(x4, y4, is_training=False)[0]
    rep = m.last_sinkhorn
    assert rep is not None and _module_mode(m)[2] == 2
    psm, w = EC._module_psm_w(m, S, E)
    R.check_selection(psm, rep.scale.cpu().numpy(), 2, 1, None, rep.choice.cpu().numpy(), rep.count.cpu().numpy(), w)
    sd = {kk: v.detach().cpu() for kk, v in m.state_dict().items()}      # (the training forwards above moved the BatchNorm statistics)
    run = _forward_sinkhorn(MoeRun(cfg, {kk: sd[kk] for kk in P}, {kk: sd[kk] for kk in B}, X, Y, training=False), 2, 1, 4)
    _close(out_s.squeeze(-1).permute(0, 2, 1).float().cpu(), run.out.float().cpu(), 1e-6, "eval-mode facade against the C ABI")
    assert torch.equal(rep.choice, run.choice[:S])


def test_adapter_pair_with_sinkhorn_sites_equals_two_sites():
    from avmoe_amd.adapters import AdapterPair
    ca, cb = _pair_cfgs(True)
    torch.manual_seed(5)
    sa, sb = build_module("avs", ca).to(DEV).train(), build_module("avs", cb).to(DEV).train()
    sa.router_top_k, sb.router_top_k, sb.router_top_k_renorm = 2, 1, False
    sa.router_sinkhorn, sb.router_sinkhorn = 3, 2
    with torch.no_grad():
        for m in (sa, sb):
            for kk, p in m.named_parameters():
                if kk.endswith(("gate", "gate_av")):
                    p.fill_(0.3)
    ra, rb = copy.deepcopy(sa), copy.deepcopy(sb)
    g = torch.Generator().manual_seed(9)
    S = 12
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
        torch.autograd.backward([oa, ov, 0.7 * la + 1.3 * lv], [ga, gv, None])
        torch.cuda.synchronize()
        reports = tuple(None if m.last_sinkhorn is None else tuple(t.clone() for t in m.last_sinkhorn) for m in (a, b))
        return ((oa.detach().float(), ov.detach().float()), (xa.grad.float(), xv.grad.float()), [p.grad.clone() for m in (a, b) for p in m.parameters()],
                reports)

    ref = run(ra, rb, None)
    for concurrent in (True, False):                      # two-stream and one-stream mode
        got = run(sa, sb, AdapterPair(sa, sb, concurrent=concurrent))
        for r_, g_ in zip(ref[3], got[3]):
            assert all(torch.equal(x_, y_) for x_, y_ in zip(r_, g_)), "the pair's scale / count / choice are not the two sites'"
        assert int(got[3][0][1].sum()) == 2 * S and int(got[3][1][1].sum()) == S
        for r_, g_ in zip(ref[0] + ref[1], got[0] + got[1]):
            assert float((r_ - g_).abs().max()) <= 1e-5 * float(r_.abs().max())
        for r_, g_ in zip(ref[2], got[2]):
            assert float((r_ - g_).abs().max()) <= 1e-4 * max(float(r_.abs().max()), 1e-6)


def test_captured_facade_step_with_sinkhorn_replays_bitwise():
    """One small single-stream site through the FACADE -- which allocates the report tensors in every call -- with Sinkhorn routing,
    forward + backward captured with torch.cuda.graph on one stream as tests/test_expert_choice_gpu.py captures its step: three replays
    equal the eager step bit for bit in the output, the three reports, the token and the parameter gradients."""
    from tests.golden_util import load_golden, split_params
    meta, cfg, t = load_golden("ave_train")
    P, B = split_params(t)
    m = build_module(meta["which"], cfg).to(DEV)
    m.load_state_dict({**P, **B}, strict=True)
    m.train()
    m.shared_gpu = False
    m.router_top_k, m.router_top_k_renorm, m.router_sinkhorn = 1, True, 3
    G = t["grad_out"].to(DEV)
    X, Y = t["X"].to(DEV).requires_grad_(True), t["Y"].to(DEV).requires_grad_(True)
    S = X.shape[0]

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
        return [out.detach().clone()] + [x_.clone() for x_ in m.last_sinkhorn] + [X.grad.clone(), Y.grad.clone()] + [p_.grad.clone() for p_ in m.parameters()]

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):                                # warm-up on the capture stream
            step()
            clear()
        eager = snapshot(step())
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    bits = R.mask_of_bits(eager[3].cpu().numpy(), cfg.E)
    assert (bits.sum(1) == 1).all() and np.array_equal(bits.sum(0), eager[2].cpu().numpy()) and float(eager[0].abs().max()) > 0
    clear()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        out = step()
    for i in range(3):
        graph.replay()
        for j, (a_, b_) in enumerate(zip(snapshot(out), eager)):
            assert torch.equal(a_, b_), (i, j)
