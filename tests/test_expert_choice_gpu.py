"""Expert-choice gating on the GPU (avmoe_moe_forward_choice / avmoe_expert_choice, include/avmoe.h).  The sub-op alone, exact: choice,
thr, last and w against tests/expert_choice_ref.py on inputs made to break a selection kernel, with NaN sentinels behind every output and
every call made twice.  Whole sites in the four bottleneck-space kernel families, at S = 300 and at E = 16: the mask, the mode words and
the weights exact from the library's own softmax, outputs and gradients against the reference given that mask, everything but the
weights bit-equal to the dense call.  And what surrounds it: later forwards on the same workspace, the profiler's names, the facade,
AdapterPair, a captured graph."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

from avmoe_amd import _capi as capi
from avmoe_amd import _capi_moe as cm
from avmoe_amd.train import expert_choice_mask
from oracle import avmoe_oracle as O
from tests import expert_choice_ref as R
from tests import router_bias_ref as RB
from tests.moe_gpu_util import MoeRun
from tests.router_grad_util import assert_close
from tests.test_adapters_api import build_module
from tests.test_router_topk_gpu import _bf16_budget, _close, _dense_bf16, _forward_topk, _pair_cfgs, _prof_names
from tests.topk_families import FAMILIES, family_config

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
NAN = float("nan")
PAD = 64                                              # sentinel words behind every output of the sub-op
INT_SENTINEL = -0x5A5A5A5B


def _p(t):
    return t.data_ptr() if t is not None else None


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ---- 1. the sub-op alone, exact -------------------------------------------------------------------------------------------------------
def _subop(pd, S, E, c, renorm, mixd, want=("w", "choice", "thr", "last")):
    """one avmoe_expert_choice call -> {name: numpy output}; every output has PAD sentinel words behind it, which must survive"""
    bufs = {"w": torch.full((S * E + PAD,), NAN, device=DEV), "choice": torch.full((S + PAD,), INT_SENTINEL, dtype=torch.int32, device=DEV),
            "thr": torch.full((E + PAD,), NAN, device=DEV), "last": torch.full((E + PAD,), INT_SENTINEL, dtype=torch.int32, device=DEV)}
    arg = lambda n: bufs[n].data_ptr() if n in want else None
    st = capi.lib().avmoe_expert_choice(pd.data_ptr(), S, E, c, renorm, _p(mixd), arg("w"), arg("choice"), arg("thr"), arg("last"), _stream())
    capi.check(st, "avmoe_expert_choice")
    torch.cuda.synchronize()
    out = {}
    for n, size in (("w", S * E), ("choice", S), ("thr", E), ("last", E)):
        host = bufs[n].cpu().numpy()
        tail = host[size if n in want else 0:]
        assert (np.isnan(tail).all() if host.dtype == np.float32 else (tail == INT_SENTINEL).all()), f"{n}: written past its end (or though NULL)"
        if n in want:
            out[n] = host[:size].reshape(S, E) if n == "w" else host[:size]
    return out


def _subop_twice(pd, S, E, c, renorm, mixd, what, **kw):
    """the call made twice: the same bytes in every output"""
    first, again = _subop(pd, S, E, c, renorm, mixd, **kw), _subop(pd, S, E, c, renorm, mixd, **kw)
    for n, v in first.items():
        assert v.tobytes() == again[n].tobytes(), f"{what}: {n} differs between two identical calls (renorm {renorm}, multiplier {mixd is not None})"
    return first


@pytest.mark.parametrize("S", [1, 2, 63, 64, 65, 255, 256, 257, 1023, 1025, 4099])
def test_subop_is_exact_on_every_input_family(S):
    """E in {1, 3, 4, 16}, c in {1, 2, ceil(S / E), S - 1, S} and the capacities a family is made for; per (input, c) one full call made
    (all four outputs), then the weights under renorm and with a multiplier (zeros, a negative entry) with the other outputs NULL; every
    call is made twice and must give the same bytes."""
    for E in (1, 3, 4, 16):
        mix = R.mix_for(S, E)
        mixd = torch.from_numpy(mix).to(DEV)
        for name in R.FAMILIES:
            p, extra = R.family(name, S, E)
            pd = torch.from_numpy(p).to(DEV)
            for c in sorted(set(R.standard_capacities(S, E) + extra)):
                what = f"{name} S={S} E={E} c={c}"
                ref = R.reference(p, c)
                first = _subop_twice(pd, S, E, c, 0, None, what)
                try:
                    R.check_subop(p, c, 0, None, ref=ref, **first)
                    if name == "uniform":
                        assert (first["choice"][:c] == (1 << E) - 1).all() and (first["choice"][c:] == 0).all(), "all equal: the first c frames"
                    for renorm in R.RENORMS.get(name, (0, 1)):
                        for m_np, m_d in ((None, None), (mix, mixd)):
                            if renorm == 0 and m_np is None:
                                continue
                            got = _subop_twice(pd, S, E, c, renorm, m_d, what, want=("w",) if renorm else ("w", "choice"))
                            R.check_subop(p, c, renorm, m_np, ref=ref, **got)
                except AssertionError as err:
                    raise AssertionError(f"{what}: {err}") from err


def test_subop_as_a_function_and_the_outputs_alone():
    """train.expert_choice_mask is the sub-op with only `choice` asked for; thr / last alone (no second launch) are the same words."""
    S, E, c = 300, 4, 75
    p, _ = R.family("softmax", S, E)
    pd = torch.from_numpy(p).to(DEV)
    m = expert_choice_mask(pd, c)
    assert m.dtype == torch.bool and m.shape == (S, E) and np.array_equal(m.cpu().numpy(), R.choice_mask(p, c))
    R.check_subop(p, c, 0, None, **_subop(pd, S, E, c, 0, None, want=("thr", "last")))
    R.check_subop(p, c, 0, None, **_subop(pd, S, E, c, 0, None, want=("choice",)))
    with pytest.raises(capi.AvmoeError, match="capacity"):
        expert_choice_mask(pd, S + 1)


# ---- 2. whole sites ---------------------------------------------------------------------------------------------------------------------
def _forward_choice(run, c, renorm, mix=None, aux=False, sync=True):
    """avmoe_moe_forward_choice on a MoeRun; run.choice receives the bitmask"""
    if aux:
        run.aux, run.load = torch.full((2,), NAN, device=DEV), torch.full((run.cfg.E,), NAN, device=DEV)
    else:
        run.aux = run.load = None
    run.choice = torch.full((run.S + PAD,), INT_SENTINEL, dtype=torch.int32, device=DEV)
    run.mix = torch.as_tensor(mix).to(DEV, torch.float32).contiguous() if mix is not None else None
    st = run.L.avmoe_moe_forward_choice(C.byref(run.desc), run.X.data_ptr(), run.Y.data_ptr(), C.byref(run.ptrs), _p(run.noise), c, int(renorm),
                                        _p(run.mix), run.out.data_ptr(), run.probs.data_ptr(), run.idx.data_ptr(), run.lb.data_ptr(), _p(run.aux),
                                        _p(run.load), run.choice.data_ptr(), run.saved.data_ptr(), run.scratch.data_ptr(), _stream())
    capi.check(st, "avmoe_moe_forward_choice")
    if sync:
        torch.cuda.synchronize()
    return run


def _forward_aux(run, aux=True):
    """the dense call with the auxiliary losses: avmoe_moe_forward_aux, top_k = 0"""
    run.aux, run.load = (torch.full((2,), NAN, device=DEV), torch.full((run.cfg.E,), NAN, device=DEV)) if aux else (None, None)
    st = run.L.avmoe_moe_forward_aux(C.byref(run.desc), run.X.data_ptr(), run.Y.data_ptr(), C.byref(run.ptrs), _p(run.noise), 0, 1,
                                     run.out.data_ptr(), run.probs.data_ptr(), run.idx.data_ptr(), run.lb.data_ptr(), _p(run.aux), _p(run.load),
                                     run.saved.data_ptr(), run.scratch.data_ptr(), _stream())
    capi.check(st, "avmoe_moe_forward_aux")
    torch.cuda.synchronize()
    return run


def _backward(run, dO, dP, lb_weight, aux_grad=None, mix=None):
    """avmoe_moe_backward_aux -- avmoe_moe_backward_reg when the forward used a multiplier -- -> {'X', 'Y', parameter key: gradient}"""
    dOd = dO.to(DEV, run.tdt).contiguous() if dO is not None else None
    dPd = dP.to(DEV, torch.float32).contiguous() if dP is not None else None
    ag = torch.tensor(aux_grad, dtype=torch.float32, device=DEV) if aux_grad is not None else None
    dX, dY = torch.full_like(run.X, NAN), torch.full_like(run.Y, NAN)
    grads = {kk: torch.full_like(v, NAN) for kk, v in run.params.items()}
    gptrs = cm.make_ptrs(grads, run.cfg.E_m, run.cfg.E_s)
    lbw = torch.full((1,), float(lb_weight), device=DEV)
    head = (C.byref(run.desc), run.X.data_ptr(), run.Y.data_ptr(), C.byref(run.ptrs), _p(dOd), _p(dPd), lbw.data_ptr(), _p(ag))
    tail = (run.saved.data_ptr(), run.scratch.data_ptr(), dX.data_ptr(), dY.data_ptr(), C.byref(gptrs), 0, _stream())
    if mix is not None:
        capi.check(run.L.avmoe_moe_backward_reg(*head, mix.data_ptr(), *tail), "avmoe_moe_backward_reg")
    else:
        capi.check(run.L.avmoe_moe_backward_aux(*head, *tail), "avmoe_moe_backward_aux")
    torch.cuda.synchronize()
    g = {kk: v.cpu() for kk, v in grads.items()}
    g["X"], g["Y"] = dX.float().cpu(), dY.float().cpu()
    return g


def _words(run, name, dtype):
    region, off, nbytes = run.table[name]
    assert region == 0
    return run.saved[off:off + nbytes].view(dtype).cpu()


BN_BATCH = ("mz", "Szz", "bn1", "bn2")                # moe_plan.h: batch means / second moments of the bottleneck, the BatchNorm-1 / -2 tables


def _raw(run, name):
    """buffer `name` of the workspace, byte for byte"""
    region, off, nbytes = run.table[name]
    return (run.saved if region == 0 else run.scratch)[off:off + nbytes].cpu()


def _psm_w(run):
    S, E = run.S, run.cfg.E
    return (_words(run, "psm", torch.float32)[:S * E].reshape(S, E).numpy(), _words(run, "probs", torch.float32)[:S * E].reshape(S, E).numpy())


def _check_selection(run, c, renorm, mix):
    """mask, mode words and weights exact on every frame against the reference evaluated on the library's own psm -> the mask"""
    E = run.cfg.E
    psm, w = _psm_w(run)
    m, T, L = ref = R.reference(psm, c)
    choice = run.choice.cpu().numpy()
    assert (choice[run.S:] == INT_SENTINEL).all(), "choice written past S"
    R.check_subop(psm, c, renorm, mix, choice=choice[:run.S], w=w, ref=ref)
    mode = _words(run, "mode", torch.int32).numpy()
    assert (mode[0], mode[1], mode[2], mode[3], mode[4]) == (E, 0, 0, c, int(renorm)), mode[:5]
    assert np.array_equal(mode[32:32 + E].view(np.uint32), T.view(np.uint32)), "mode[32 + e] is not the bits of T_e"
    assert np.array_equal(mode[48:48 + E].astype(np.int64), L), "mode[48 + e] is not L_e"
    return m


def _site_data(which):
    """(cfg, S, bf16, P, B, X, Y, noise, [capacities], dO, dP) of a site case"""
    if which in FAMILIES:
        cfg, S, bf16 = family_config(which)
        P, B = O.init_params(cfg, seed=3)
        g = torch.Generator().manual_seed(17)
        X = 0.3 * torch.randn(S, cfg.Nx, cfg.Cx, generator=g)
        Y = 0.3 * torch.randn(S, cfg.Ny, cfg.Cy, generator=g)
        noise, caps = torch.randn(S, cfg.E, generator=g), [1]
    elif which == "s300":
        cfg, S, P, B, X, Y, noise, c = R.s300_inputs()
        bf16, caps = False, [c]
    else:
        cfg, S, P, B, X, Y, noise, _ = RB.selection_case("e16")
        bf16, caps = False, [1, 2]
    if bf16:
        X, Y = X.to(torch.bfloat16).float(), Y.to(torch.bfloat16).float()
    g = torch.Generator().manual_seed(23)
    dO = torch.randn(S, cfg.Nx, cfg.Cx, generator=g).to(torch.bfloat16).float()
    dP = torch.randn(S, cfg.E, generator=g)
    return cfg, S, bf16, P, B, X, Y, noise, caps, dO, dP


def _eager_bf16_ec(cfg, P, B, X, Y, dO, dP, w, mask, renorm, mix, aux_grad, load, noise):
    """the reference evaluated eagerly on the GPU under torch.autocast(bfloat16) with the same mask: the first anchor of _bf16_budget"""
    d = lambda t: None if t is None else torch.as_tensor(t).to(DEV)
    Pd, Bd = {kk: v.to(DEV) for kk, v in P.items()}, {kk: v.to(DEV) for kk, v in B.items()}
    mt = torch.as_tensor(np.asarray(mask)).to(DEV, torch.float32)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        g = R.ec_grads(cfg, Pd, Bd, d(X), d(Y), d(dO), d(dP), w, mt, renorm, d(mix), aux_grad, d(load), noise=d(noise))
        g["out"] = R.ec_forward(Pd, Bd, d(X), d(Y), cfg, mt, renorm, d(mix), noise=d(noise))["out"].detach()
    return {kk: v.float().cpu() for kk, v in g.items()}


# (renorm, multiplier, auxiliary gradients, dOut)
VARIANTS = ((0, False, False, True), (1, True, True, True), (1, False, True, False), (0, True, False, False))


@pytest.mark.parametrize("which", list(FAMILIES) + ["s300", "e16"])
def test_site_with_expert_choice(which):
    cfg, S, bf16, P, B, X, Y, noise, caps, dO, dP = _site_data(which)
    E = cfg.E
    with (capi.test_hooks(capi.HOOK_KFS_FORCE) if which == "tile_stream" else _nothing()):
        mk = lambda: MoeRun(cfg, P, B, X, Y, bf16=bf16, noise=noise)
        dense = _forward_aux(mk())
        plain = mk().forward()
        dense_pair = _dense_bf16(plain, cfg, P, B, X, Y, dO, dP, 0.5, True, noise, None) if bf16 else None
        load = dense.load.cpu()
        for c in caps:
            for renorm, with_mix, with_aux, with_out in VARIANTS:
                what = f"{which}/c={c}/renorm={renorm}/mix={with_mix}/aux={with_aux}/dOut={with_out}"
                mix = R.mix_for(S, E) if with_mix else None
                run = _forward_choice(mk(), c, renorm, mix, aux=True)
                assert run.guards_intact(), what
                psm = _psm_w(run)[0]
                assert np.array_equal(psm, dense.probs.cpu().numpy()), what + ": psm is not the dense softmax"
                mask = _check_selection(run, c, renorm, mix)
                if which == "s300":
                    none, many = R.served_counts(mask)
                    print(f"{what}: {none} frames without an expert, {many} with two or more")
                    assert none * 16 >= S and many * 16 >= S, (none, many)
                    assert float(run.out[torch.from_numpy(~mask.any(1)).to(DEV)].abs().max()) == 0.0, "out[s] != 0 on a frame no expert took"
                for n in ("probs", "idx", "lb", "aux", "load"):
                    assert torch.equal(getattr(run, n), getattr(dense, n)), f"{what}: {n} is not the dense call's"
                for kk, v in run.buffers.items():         # BatchNorm running statistics: the dense call's, bit for bit
                    assert torch.equal(v, dense.buffers[kk]), (what, kk)
                for nb in BN_BATCH:                       # ... and the batch statistics the forward left in its workspace
                    assert torch.equal(_raw(run, nb), _raw(dense, nb)), f"{what}: BatchNorm batch statistics `{nb}` are not the dense call's"
                ag = (0.9, -1.1) if with_aux else None
                got = _backward(run, dO if with_out else None, dP, 0.5, ag, run.mix)
                assert run.guards_intact(), what
                got["out"] = run.out.float().cpu()
                ref = R.site_reference(cfg, P, B, X, Y, dO if with_out else None, dP, 0.5, mask, renorm, mix, ag, load, noise=noise)
                if bf16:
                    eager = _eager_bf16_ec(cfg, P, B, X, Y, dO if with_out else None, dP, 0.5, mask, renorm, mix, ag, load, noise)
                    if with_out:
                        _bf16_budget(got, ref, eager, dense_pair, what)
                    else:                                 # (the dense anchor was taken with dOut: the router-only case keeps the eager one)
                        _bf16_budget(got, ref, eager, (ref, ref), what)
                else:
                    _close(got.pop("out"), ref.pop("out"), 1e-3, what + "/out")
                    assert_close(got, ref, rtol=1e-3, floor_frac=1e-2, what=what)


@pytest.mark.parametrize("which", list(FAMILIES) + ["s300", "e16"])
def test_capacity_S_is_the_dense_call_bitwise(which):
    """capacity == S without renorm and without a multiplier: every output (out, probs, idx, lb, aux, load), the BatchNorm statistics and
    every gradient (dO, dprobs, lb and auxiliary terms) are the dense call's bits."""
    cfg, S, bf16, P, B, X, Y, noise, caps, dO, dP = _site_data(which)
    with (capi.test_hooks(capi.HOOK_KFS_FORCE) if which == "tile_stream" else _nothing()):
        ref = _forward_aux(MoeRun(cfg, P, B, X, Y, bf16=bf16, noise=noise))
        plain = MoeRun(cfg, P, B, X, Y, bf16=bf16, noise=noise).forward()      # (avmoe_moe_forward itself gives the same out / probs / idx / lb)
        run = _forward_choice(MoeRun(cfg, P, B, X, Y, bf16=bf16, noise=noise), S, 0, aux=True)
        assert (run.choice[:S].cpu().numpy() == (1 << cfg.E) - 1).all()
        for n in ("out", "probs", "idx", "lb", "aux", "load"):
            assert torch.equal(getattr(run, n), getattr(ref, n)), n
        for n in ("out", "probs", "idx", "lb"):
            assert torch.equal(getattr(run, n), getattr(plain, n)), n
        for kk, v in run.buffers.items():
            assert torch.equal(v, ref.buffers[kk]), kk
        for nb in BN_BATCH:
            assert torch.equal(_raw(run, nb), _raw(ref, nb)), nb
        rg = _backward(ref, dO, dP, 0.5, (0.9, -1.1))
        got = _backward(run, dO, dP, 0.5, (0.9, -1.1))
        for kk, v in rg.items():
            assert torch.equal(got[kk], v), kk


class _nothing:
    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False


# ---- 3. surrounding behaviour -----------------------------------------------------------------------------------------------------------
def _small():
    cfg, S, bf16, P, B, X, Y, noise, caps, dO, dP = _site_data("tile_fast")
    return cfg, S, P, B, X, Y, noise, dO, dP


def test_a_later_dense_or_topk_forward_on_the_same_workspace_switches_the_choice_off():
    cfg, S, P, B, X, Y, noise, dO, dP = _small()
    mk = lambda: MoeRun(cfg, P, B, X, Y, noise=noise, training=False)      # (eval-mode BatchNorm: a second forward sees the same statistics)
    for later in ("dense", "topk"):
        fwd = (lambda r: r.forward()) if later == "dense" else (lambda r: _forward_topk(r, 2, True))
        ref = fwd(mk())
        rg = _backward(ref, dO, dP, 0.5)
        run = _forward_choice(mk(), 1, 1, R.mix_for(S, cfg.E))
        assert _words(run, "mode", torch.int32)[3] == 1
        fwd(run)
        mode = _words(run, "mode", torch.int32)
        assert mode[3] == 0 and mode[4] == 0 and mode[0] == (0 if later == "dense" else 2), mode[:5]
        assert torch.equal(run.out, ref.out)
        got = _backward(run, dO, dP, 0.5)
        for kk, v in rg.items():
            assert torch.equal(got[kk], v), (later, kk)


def test_profiler_names_two_more_in_the_forward_none_in_the_backward():
    cfg, S, P, B, X, Y, noise, dO, dP = _small()

    def reg(run):
        st = run.L.avmoe_moe_forward_reg(C.byref(run.desc), run.X.data_ptr(), run.Y.data_ptr(), C.byref(run.ptrs), _p(run.noise), 0, 1, None,
                                         run.out.data_ptr(), run.probs.data_ptr(), run.idx.data_ptr(), run.lb.data_ptr(), None, None,
                                         run.saved.data_ptr(), run.scratch.data_ptr(), _stream())
        capi.check(st, "avmoe_moe_forward_reg")
        return run
    r_aux, names_aux = _prof_names(lambda: _forward_aux(MoeRun(cfg, P, B, X, Y, noise=noise), aux=False))
    r_reg, names_reg = _prof_names(lambda: reg(MoeRun(cfg, P, B, X, Y, noise=noise)))
    assert names_aux == names_reg, "with the option off a forward runs avmoe_moe_forward_reg's launches"
    r_ch, names_ch = _prof_names(lambda: _forward_choice(MoeRun(cfg, P, B, X, Y, noise=noise), 1, 1))
    new = [n for n in names_ch if n not in names_reg]
    assert set(names_reg) <= set(names_ch) and 1 <= len(new) <= 2, new
    _, back_reg = _prof_names(lambda: _backward(r_reg, dO, dP, 0.5))
    _, back_ch = _prof_names(lambda: _backward(r_ch, dO, dP, 0.5))
    assert back_ch == back_reg, "the backward of a choice forward adds no launch"


def _module(cfg, P, B):
    m = build_module("avs", cfg).to(DEV)
    m.load_state_dict({**P, **B}, strict=True)
    from avmoe_amd.debug import keep_saved
    keep_saved(m)
    return m


def _module_psm_w(m, S, E):
    desc, saved = m.__dict__["_last_saved"]
    t = {n: (o, nb) for n, _r, o, nb in cm.buffer_table(capi.lib(), desc)}
    torch.cuda.synchronize()
    get = lambda n: saved[t[n][0]:t[n][0] + t[n][1]].view(torch.float32)[:S * E].reshape(S, E).cpu().numpy()
    return get("psm"), get("probs")


def test_facade_training_with_expert_dropout_and_eval_mode():
    cfg, S, P, B, X, Y, noise, dO, dP = _small()
    E = cfg.E
    m = _module(cfg, P, B)
    x4 = X.to(DEV).permute(0, 2, 1).unsqueeze(-1).contiguous().requires_grad_(True)
    y4 = Y.to(DEV).permute(0, 2, 1).unsqueeze(-1).contiguous().requires_grad_(True)
    m.train()
    m(x4, y4, is_training=True)
    assert m.last_expert_choice is None
    m.router_expert_choice, m.router_expert_choice_renorm, m.expert_dropout = 2, True, 0.4
    c = R.capacity(2, S, E)
    torch.manual_seed(3)
    out, idx, probs, lb = m(x4, y4, is_training=True)
    bits = m.last_expert_choice
    assert bits.dtype == torch.int32 and bits.shape == (S,) and not bits.requires_grad
    psm, w = _module_psm_w(m, S, E)
    mix = m.__dict__["_mix_last"].cpu().numpy()
    assert (mix == 0).any() and (mix != 0).any(), "the expert-dropout draw shows nothing"
    R.check_subop(psm, c, 1, mix, choice=bits.cpu().numpy(), w=w)
    assert np.array_equal(probs.reshape(S, E).detach().cpu().numpy(), psm)
    torch.autograd.backward([out, lb], [torch.randn_like(out), None])
    assert bool(torch.isfinite(x4.grad).all()) and float(x4.grad.abs().max()) > 0
    assert all(bool(torch.isfinite(p_.grad).all()) for p_ in m.parameters() if p_.grad is not None)
    # eval mode: the choice still applies (an evaluation depends on the batch), the multiplier does not; equal to the C ABI on the same inputs
    m.eval()
    m.router_expert_choice_renorm = False
    with torch.no_grad():
        out_e = m(x4, y4, is_training=False)[0]
    psm, w = _module_psm_w(m, S, E)
    R.check_subop(psm, c, 0, None, choice=m.last_expert_choice.cpu().numpy(), w=w)
    sd = {kk: v.detach().cpu() for kk, v in m.state_dict().items()}      # (the training forwards above moved the BatchNorm statistics)
    run = _forward_choice(MoeRun(cfg, {kk: sd[kk] for kk in P}, {kk: sd[kk] for kk in B}, X, Y, training=False), c, 0)
    _close(out_e.squeeze(-1).permute(0, 2, 1).float().cpu(), run.out.float().cpu(), 1e-6, "eval-mode facade against the C ABI")
    m.router_expert_choice = None
    with torch.no_grad():
        m(x4, y4, is_training=False)
    assert m.last_expert_choice is None


def test_adapter_pair_with_choice_sites_equals_two_sites():
    from avmoe_amd.adapters import AdapterPair
    ca, cb = _pair_cfgs(True)
    torch.manual_seed(5)
    sa, sb = build_module("avs", ca).to(DEV).train(), build_module("avs", cb).to(DEV).train()
    sa.router_expert_choice, sb.router_expert_choice, sb.router_expert_choice_renorm = 2, 1, True
    with torch.no_grad():
        for m in (sa, sb):
            for kk, p in m.named_parameters():
                if kk.endswith(("gate", "gate_av")):
                    p.fill_(0.3)
    ra, rb = copy.deepcopy(sa), copy.deepcopy(sb)
    g = torch.Generator().manual_seed(9)
    S = 4
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
        return ((oa.detach().float(), ov.detach().float()), (xa.grad.float(), xv.grad.float()), [p.grad.clone() for m in (a, b) for p in m.parameters()],
                tuple(None if m.last_expert_choice is None else m.last_expert_choice.clone() for m in (a, b)))

    ref = run(ra, rb, None)
    got = run(sa, sb, AdapterPair(sa, sb, concurrent=True))
    for r_, g_ in zip(ref[3], got[3]):
        assert torch.equal(r_, g_)
    ea, eb = ca.E, cb.E
    assert int(sum(bin(int(v) & 0xFFFF).count("1") for v in got[3][0].cpu())) == ea * R.capacity(2, S, ea)
    assert int(sum(bin(int(v) & 0xFFFF).count("1") for v in got[3][1].cpu())) == eb * R.capacity(1, S, eb)
    for r_, g_ in zip(ref[0] + ref[1], got[0] + got[1]):
        assert float((r_ - g_).abs().max()) <= 1e-5 * float(r_.abs().max())
    for r_, g_ in zip(ref[2], got[2]):
        assert float((r_ - g_).abs().max()) <= 1e-4 * max(float(r_.abs().max()), 1e-6)
    sa.router_expert_choice = sb.router_expert_choice = None      # the choice did something: the dense pair differs
    plain = run(sa, sb, AdapterPair(sa, sb, concurrent=True))
    assert plain[3] == (None, None)
    assert float((plain[0][0] - got[0][0]).abs().max()) > 1e-3 * float(got[0][0].abs().max()), "the choice had no effect on the pair"


def test_captured_facade_step_with_expert_choice_replays_bitwise():
    """One small single-stream site through the FACADE -- which allocates the bitmask tensor in every call -- with expert choice
    (renormalised), forward + backward captured with torch.cuda.graph on one stream as tests/test_mix_drop_gpu.py captures its step:
    three replays equal the eager step bit for bit in the output, the bitmask, the token and the parameter gradients.  Training-mode
    BatchNorm: the outputs depend on the batch statistics only, the running statistics just move on."""
    from tests.golden_util import load_golden, split_params
    meta, cfg, t = load_golden("ave_train")
    P, B = split_params(t)
    m = build_module(meta["which"], cfg).to(DEV)
    m.load_state_dict({**P, **B}, strict=True)
    m.train()
    m.shared_gpu = False
    m.router_expert_choice, m.router_expert_choice_renorm = 1, True
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
        return [out.detach().clone(), m.last_expert_choice.clone(), X.grad.clone(), Y.grad.clone()] + [p_.grad.clone() for p_ in m.parameters()]

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):                                # warm-up on the capture stream
            step()
            clear()
        eager = snapshot(step())
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    bits = R.mask_of_bits(eager[1].cpu().numpy(), cfg.E)
    assert (bits.sum(0) == R.capacity(1, S, cfg.E)).all() and float(eager[0].abs().max()) > 0
    clear()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        out = step()
    for i in range(3):
        graph.replay()
        for j, (a_, b_) in enumerate(zip(snapshot(out), eager)):
            assert torch.equal(a_, b_), (i, j)
