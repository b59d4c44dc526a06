"""Top-p routing on the GPU (avmoe_moe_forward_top_p / avmoe_router_top_p, include/avmoe.h).  The sub-op alone: the mask, the bitmask,
the counts, the histogram and the weights EXACT against tests/top_p_ref.py on the same p, with NaN / integer sentinels behind every output,
NULL outputs untouched and every call made twice; k_min = k_max = k against avmoe_router_topk.  Whole sites in the four bottleneck-space
kernel families, at S = 300 and at E = 16: everything but the weights bit-equal to avmoe_moe_forward_reg, the mode words, outputs and
gradients against the eager reference given the mask the reference computes from the kernel's own probs (no margin condition, no case
skipped), fixed k against the plain top-k and dense calls bit for bit, load / balance against the reference's count shares.  And what
surrounds it: the router-only backward, a later plain forward on the same workspace, the profiler's names, the facade in both modes,
AdapterPair, TopPMeter, a captured step."""
import copy
import ctypes as C
import math
from fractions import Fraction

import numpy as np
import pytest
import torch

from avmoe_amd import _capi as capi
from avmoe_amd.train import TopPMeter, top_p_mask
from tests import expert_choice_ref as ER
from tests import top_p_ref as R
from tests import test_expert_choice_gpu as EC        # (as a module: its helpers, not its tests)
from tests.moe_gpu_util import MoeRun
from tests.router_aux_ref import scalar_close
from tests.router_grad_util import assert_close
from tests.test_adapters_api import build_module
from tests.test_router_topk_gpu import _bf16_budget, _close, _dense_bf16, _forward_topk, _pair_cfgs, _prof_names
from tests.test_sinkhorn_gpu import _forward_reg, _module_mode, _tokens4
from tests.topk_families import FAMILIES

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
NAN = float("nan")
PAD = 64                                              # sentinel words behind every output
INT_SENTINEL = -0x5A5A5A5B
SIZES = {"w": lambda S, E: S * E, "choice": lambda S, E: S, "count": lambda S, E: E, "khist": lambda S, E: E + 1}
ALL = ("w", "choice", "count", "khist")


def _p(t):
    return t.data_ptr() if t is not None else None


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _bits(x):
    return np.float32(x).view(np.int32)


# ---- 1. the sub-op alone ----------------------------------------------------------------------------------------------------------------
def _subop(pd, S, E, P, k_min, k_max, renorm, mixd, want=ALL):
    """one avmoe_router_top_p call -> {name: numpy output}; every output has PAD sentinel words behind it, which must survive, and an
    output not asked for is passed as NULL"""
    bufs = {"w": torch.full((S * E + PAD,), NAN, device=DEV), "choice": torch.full((S + PAD,), INT_SENTINEL, dtype=torch.int32, device=DEV),
            "count": torch.full((E + PAD,), INT_SENTINEL, dtype=torch.int32, device=DEV),
            "khist": torch.full((E + 1 + PAD,), INT_SENTINEL, dtype=torch.int32, device=DEV)}
    arg = lambda n: bufs[n].data_ptr() if n in want else None
    st = capi.lib().avmoe_router_top_p(pd.data_ptr(), S, E, P, k_min, k_max, renorm, _p(mixd), arg("w"), arg("choice"), arg("count"), arg("khist"),
                                       _stream())
    capi.check(st, "avmoe_router_top_p")
    torch.cuda.synchronize()
    out = {}
    for n, size in SIZES.items():
        host = bufs[n].cpu().numpy()
        tail = host[size(S, E) if n in want else 0:]
        assert (np.isnan(tail).all() if host.dtype == np.float32 else (tail == INT_SENTINEL).all()), f"{n}: written past its end (or though NULL)"
        if n in want:
            out[n] = host[:size(S, E)].reshape(S, E) if n == "w" else host[:size(S, E)]
    return out


def _subop_twice(pd, S, E, P, k_min, k_max, renorm, mixd, what, **kw):
    """the call made twice: the same bits in every output"""
    first, again = _subop(pd, S, E, P, k_min, k_max, renorm, mixd, **kw), _subop(pd, S, E, P, k_min, k_max, renorm, mixd, **kw)
    for n, v in first.items():
        assert v.tobytes() == again[n].tobytes(), f"{what}: {n} differs between two identical calls (renorm {renorm}, multiplier {mixd is not None})"
    return first


# what else is asked for beside the full call: (multiplier, outputs) -- among them the counts without a bitmask (the count launch then
# selects on p itself), the counts alone (one launch) and the bitmask alone
PARTIAL = ((False, ("w",)), (True, ("w", "count", "khist")), (True, ("w", "choice")), (True, ("count",)), (False, ("choice", "khist")))


@pytest.mark.parametrize("S", [1, 2, 63, 64, 65, 257, 1025, 4099])
def test_subop_is_exact_on_every_input_family(S):
    """E in {2, 3, 4, 16}, every family, every threshold, (k_min, k_max) in {(1, E), (2, E - 1), (E, E)}: the full call with one renorm
    setting and a partial call with the other (both settings and both multiplier settings meet every family, E and threshold)."""
    n = 0
    for E in (2, 3, 4, 16):
        mix = R.mix_for(S, E)
        mixd = torch.from_numpy(mix).to(DEV)
        for name in R.FAMILIES:
            p = R.family(name, S, E)
            pd = torch.from_numpy(p).to(DEV)
            ranks = R.ranks_of(p)
            for P in R.THRESHOLDS:
                for k_min, k_max in R.k_ranges(E):
                    n += 1
                    renorm = n & 1
                    what = f"{name} S={S} E={E} P={P} k=[{k_min}, {k_max}]"
                    try:
                        got = _subop_twice(pd, S, E, P, k_min, k_max, renorm, None, what)
                        m = R.check_selection(p, P, k_min, k_max, renorm, None, got["choice"], got["count"], got["khist"], got["w"], ranks=ranks)
                        if name == "uniform" and E != 3:      # 1 / E and its multiples are exact: k* = ceil(P E) in rationals, all ties
                            k = min(max(math.ceil(Fraction(float(np.float32(P))) * E), k_min), k_max)
                            assert (got["choice"] == (1 << k) - 1).all(), f"all ties: the first {k} experts"
                        with_mix, want = PARTIAL[(n // 2) % len(PARTIAL)]
                        part = _subop_twice(pd, S, E, P, k_min, k_max, 1 - renorm, mixd if with_mix else None, what, want=want)
                        R.check_selection(p, P, k_min, k_max, 1 - renorm, mix if with_mix else None, part.get("choice"), part.get("count"),
                                          part.get("khist"), part.get("w"), ranks=ranks)
                        assert int(got["khist"].sum()) == S and int(got["count"].sum()) == int(m.sum())
                    except AssertionError as err_:
                        raise AssertionError(f"{what}: {err_}") from err_
    if S in (63, 257):                                    # the comparison above saw every prefix length (tests/test_top_p_ref.py asserts it of the reference)
        for E in (2, 3, 4, 16):
            kh = _subop(torch.from_numpy(R.family("sweep", S, E)).to(DEV), S, E, 0.95, 1, E, 0, None, want=("khist",))["khist"]
            assert kh[0] == 0 and (kh[1:] > 0).all(), (E, kh)


@pytest.mark.parametrize("E", [2, 3, 4, 16])
def test_fixed_k_is_the_selection_of_router_topk_and_the_weights_of_topk(E):
    """k_min = k_max = k, whatever P says: the experts of avmoe_router_topk, and w = m p / kept with kept added in expert order"""
    S = 257
    for name in R.FAMILIES:
        p = R.family(name, S, E)
        pd = torch.from_numpy(p).to(DEV)
        for k in sorted({1, 2, E - 1, E}):
            if not 1 <= k <= E:
                continue
            idx = torch.empty(S, k, dtype=torch.int64, device=DEV)
            capi.check(capi.lib().avmoe_router_topk(pd.data_ptr(), C.c_int64(S), C.c_int32(E), C.c_int32(k), idx.data_ptr(), _stream()), "avmoe_router_topk")
            want = np.zeros((S, E), bool)
            want[np.arange(S)[:, None], idx.cpu().numpy()] = True
            for P in (1e-30, 0.75, 1.0):
                got = _subop_twice(pd, S, E, P, k, k, 1, None, f"{name} E={E} k={k} P={P}")
                assert np.array_equal(R.mask_of_bits(got["choice"], E), want), (name, k, P)
                assert np.array_equal(got["w"].view(np.uint32), R.weights(p, want, 1).view(np.uint32)), (name, k, P)
                assert got["khist"][k] == S and got["khist"].sum() == S


def test_subop_as_a_function():
    S, E = 300, 4
    p = R.family("sweep", S, E)
    pd = torch.from_numpy(p).to(DEV)
    m = top_p_mask(pd, 0.95)
    assert m.dtype == torch.bool and m.shape == (S, E) and np.array_equal(m.cpu().numpy(), R.select_mask(p, 0.95))
    m = top_p_mask(pd.reshape(3, 100, E), 0.75, k_min=2, k_max=3)
    assert np.array_equal(m.cpu().numpy(), R.select_mask(p, 0.75, 2, 3))
    with pytest.raises(capi.AvmoeError, match="top_p"):
        top_p_mask(pd, 1.5)
    with pytest.raises(capi.AvmoeError, match="k_max"):
        top_p_mask(pd, 0.5, k_max=E + 1)


# ---- 2. whole sites ---------------------------------------------------------------------------------------------------------------------
def _forward_top_p(run, P, k_min, k_max, renorm, mix=None, aux=False, sync=True, reports=ALL[1:]):
    """avmoe_moe_forward_top_p on a MoeRun; run.choice / run.count / run.khist receive the reports (None: passed as NULL)"""
    E = run.cfg.E
    run.aux, run.load = (torch.full((2,), NAN, device=DEV), torch.full((E,), NAN, device=DEV)) if aux else (None, None)
    for n, size in (("choice", run.S), ("count", E), ("khist", E + 1)):
        setattr(run, n, torch.full((size + PAD,), INT_SENTINEL, dtype=torch.int32, device=DEV) if n in reports else None)
    run.mix = torch.as_tensor(mix).to(DEV, torch.float32).contiguous() if mix is not None else None
    st = run.L.avmoe_moe_forward_top_p(C.byref(run.desc), run.X.data_ptr(), run.Y.data_ptr(), C.byref(run.ptrs), _p(run.noise), P, k_min, k_max,
                                       int(renorm), _p(run.mix), run.out.data_ptr(), run.probs.data_ptr(), run.idx.data_ptr(), run.lb.data_ptr(),
                                       _p(run.aux), _p(run.load), _p(run.choice), _p(run.count), _p(run.khist), run.saved.data_ptr(),
                                       run.scratch.data_ptr(), _stream())
    capi.check(st, "avmoe_moe_forward_top_p")
    if sync:
        torch.cuda.synchronize()
    return run


def _check_mode(mode, P, k_min, k_max, renorm):
    assert (mode[0], mode[1], mode[2], mode[3], mode[4], mode[5]) == (k_max, int(renorm), 3, 0, 0, 0), mode[:6]
    assert mode[16] == _bits(P) and mode[17] == k_min, mode[16:18]


def _check_selection(run, P, k_min, k_max, renorm, mix):
    """the mode words, and mask / reports / weights exact against the reference evaluated on the library's own psm -> the mask"""
    S, E = run.S, run.cfg.E
    psm, w = EC._psm_w(run)
    _check_mode(EC._words(run, "mode", torch.int32).numpy(), P, k_min, k_max, renorm)
    rep = {}
    for n, size in (("choice", S), ("count", E), ("khist", E + 1)):
        t = getattr(run, n)
        if t is not None:
            host = t.cpu().numpy()
            assert (host[size:] == INT_SENTINEL).all(), f"{n} written past its end"
            rep[n] = host[:size]
    return R.check_selection(psm, P, k_min, k_max, renorm, mix, rep.get("choice"), rep.get("count"), rep.get("khist"), w)


def _variants(E):
    """(P, k_min, k_max, renorm, multiplier, auxiliary gradients, dOut): a router-only backward and backwards with a multiplier among them"""
    return ((0.75, 1, E, 1, False, False, True), (0.5, 2, E - 1, 1, True, True, True), (0.95, 1, E, 0, False, True, False),
            (0.75, 1, 2, 0, True, False, False))


@pytest.mark.parametrize("which", list(FAMILIES) + ["s300", "e16"])
def test_site_with_top_p_routing(which):
    cfg, S, bf16, P_, B, X, Y, noise, _caps, dO, dP = EC._site_data(which)
    E = cfg.E
    with (capi.test_hooks(capi.HOOK_KFS_FORCE) if which == "tile_stream" else EC._nothing()):
        mk = lambda: MoeRun(cfg, P_, B, X, Y, bf16=bf16, noise=noise)
        dense_pair = _dense_bf16(mk().forward(), cfg, P_, B, X, Y, dO, dP, 0.5, True, noise, None) if bf16 else None
        for i, (P, k_min, k_max, renorm, with_mix, with_aux, with_out) in enumerate(_variants(E)):
            what = f"{which}/P={P}/k=[{k_min}, {k_max}]/renorm={renorm}/mix={with_mix}/aux={with_aux}/dOut={with_out}"
            mix = ER.mix_for(S, E) if with_mix else None
            plain = _forward_reg(mk(), E, 0, mix, aux=True)
            run = _forward_top_p(mk(), P, k_min, k_max, renorm, mix, aux=True, reports=ALL[1:] if i != 2 else ("count", "khist"))
            assert run.guards_intact(), what
            psm = EC._psm_w(run)[0]
            assert np.array_equal(psm, plain.probs.cpu().numpy()), what + ": psm is not the dense softmax"
            mask = _check_selection(run, P, k_min, k_max, renorm, mix)
            kh = R.khist_of(mask)
            print(f"{what}: khist {kh.tolist()}")
            if which == "s300" and (k_min, k_max) == (1, E):
                assert (kh[1:] > 0).sum() >= 2, "every frame took the same number of experts: the case shows no dynamic k"
            for n in ("probs", "idx", "lb"):
                assert torch.equal(getattr(run, n), getattr(plain, n)), f"{what}: {n} is not avmoe_moe_forward_reg's"
            assert torch.equal(run.aux[0], plain.aux[0]), what + ": z is not avmoe_moe_forward_reg's"
            for kk, v in run.buffers.items():             # BatchNorm running statistics: the plain call's, bit for bit
                assert torch.equal(v, plain.buffers[kk]), (what, kk)
            for nb in EC.BN_BATCH:                        # ... and the batch statistics the forward left in its workspace
                assert torch.equal(EC._raw(run, nb), EC._raw(plain, nb)), f"{what}: BatchNorm batch statistics `{nb}` are not the plain call's"
            # load / balance: the share of the routing slots actually handed out
            load = run.load.cpu()
            assert np.array_equal(load.numpy().view(np.uint32), R.load_of(mask).view(np.uint32)), f"{what}: load {load} is not count / sum count"
            assert torch.equal(EC._words(run, "load", torch.float32)[:E], load), what + ": the saved load is not the reported one"
            scalar_close(run.aux[1].item(), E * float((load.double().numpy() * psm.astype(np.float64).mean(0)).sum()), what + "/balance")
            ag = (0.9, -1.1) if with_aux else None
            got = EC._backward(run, dO if with_out else None, dP, 0.5, ag, run.mix)
            assert run.guards_intact(), what
            got["out"] = run.out.float().cpu()
            ref = ER.site_reference(cfg, P_, B, X, Y, dO if with_out else None, dP, 0.5, mask, renorm, mix, ag, load, noise=noise)
            if bf16:
                eager = EC._eager_bf16_ec(cfg, P_, B, X, Y, dO if with_out else None, dP, 0.5, mask, renorm, mix, ag, load, noise)
                _bf16_budget(got, ref, eager, dense_pair if with_out else (ref, ref), what)
            else:
                _close(got.pop("out"), ref.pop("out"), 1e-3, what + "/out")
                assert_close(got, ref, rtol=1e-3, floor_frac=1e-2, what=what)


@pytest.mark.parametrize("which", list(FAMILIES) + ["s300", "e16"])
def test_fixed_k_is_the_plain_topk_call_and_k_E_the_dense_call_bitwise(which):
    """k_min = k_max = k: avmoe_moe_forward_reg(top_k = k) bit for bit in out, the weights, the auxiliary losses (count / (S k) either way)
    and every gradient (dO, dprobs, lb and the auxiliary terms).  k_min = k_max = E without renorm: avmoe_moe_forward bit for bit."""
    cfg, S, bf16, P_, B, X, Y, noise, _caps, dO, dP = EC._site_data(which)
    E = cfg.E
    with (capi.test_hooks(capi.HOOK_KFS_FORCE) if which == "tile_stream" else EC._nothing()):
        mk = lambda: MoeRun(cfg, P_, B, X, Y, bf16=bf16, noise=noise)
        for k, renorm, with_mix in ((1, 0, False), (2, 1, True), (E - 1, 1, False)):
            mix = ER.mix_for(S, E) if with_mix else None
            ref = _forward_reg(mk(), k, renorm, mix, aux=True)
            run = _forward_top_p(mk(), 0.9, k, k, renorm, mix, aux=True)
            for n in ("out", "probs", "idx", "lb"):
                assert torch.equal(getattr(run, n), getattr(ref, n)), (k, n)
            assert torch.equal(run.aux[0], ref.aux[0]) and torch.equal(run.load, ref.load), "fixed k: z and the load are the top-k call's too"
            assert torch.equal(EC._raw(run, "probs"), EC._raw(ref, "probs")), "the mixture weights are not top-k's bits"
            assert int(run.khist[k]) == S
            rg = EC._backward(ref, dO, dP, 0.5, (0.9, -1.1), ref.mix)
            got = EC._backward(run, dO, dP, 0.5, (0.9, -1.1), run.mix)
            for kk, v in rg.items():
                assert torch.equal(got[kk], v), (k, kk)
        plain = mk().forward()
        run = _forward_top_p(mk(), 0.5, E, E, 0)
        assert (run.choice[:S].cpu().numpy() == (1 << E) - 1).all() and int(run.khist[E]) == S
        for n in ("out", "probs", "idx", "lb"):
            assert torch.equal(getattr(run, n), getattr(plain, n)), n
        for kk, v in run.buffers.items():
            assert torch.equal(v, plain.buffers[kk]), kk
        rg, got = EC._backward(plain, dO, dP, 0.5), EC._backward(run, dO, dP, 0.5)
        for kk, v in rg.items():
            assert torch.equal(got[kk], v), kk


# ---- 3. surrounding behaviour -----------------------------------------------------------------------------------------------------------
def test_router_only_backward_serves_a_top_p_forward():
    """dOut == NULL: the gradients of <probs, dP> + lb + the auxiliary terms alone, against the reference given the mask; the same bits
    as the full backward's router part would need no multiplier: the call takes none"""
    cfg, S, P_, B, X, Y, noise, dO, dP = EC._small()
    run = _forward_top_p(MoeRun(cfg, P_, B, X, Y, noise=noise), 0.75, 1, cfg.E, 1, aux=True)
    mask = _check_selection(run, 0.75, 1, cfg.E, 1, None)
    got = EC._backward(run, None, dP, 0.5, (0.9, -1.1))
    ref = ER.site_reference(cfg, P_, B, X, Y, None, dP, 0.5, mask, 1, None, (0.9, -1.1), run.load.cpu(), noise=noise)
    ref.pop("out")
    assert_close(got, ref, rtol=1e-3, floor_frac=1e-2, what="router-only")


def test_a_later_plain_forward_on_the_same_workspace_switches_the_mode_off():
    cfg, S, P_, B, X, Y, noise, dO, dP = EC._small()
    mk = lambda: MoeRun(cfg, P_, B, X, Y, noise=noise, training=False)      # (eval-mode BatchNorm: a second forward sees the same statistics)
    for later in ("dense", "topk"):
        fwd = (lambda r: r.forward()) if later == "dense" else (lambda r: _forward_topk(r, 2, True))
        ref = fwd(mk())
        rg = EC._backward(ref, dO, dP, 0.5)
        run = _forward_top_p(mk(), 0.75, 1, 3, 1, ER.mix_for(S, cfg.E))
        _check_mode(EC._words(run, "mode", torch.int32).numpy(), 0.75, 1, 3, 1)
        tp_out = run.out.clone()
        fwd(run)
        mode = EC._words(run, "mode", torch.int32)
        assert (int(mode[0]), int(mode[1]), int(mode[2])) == ((0, 1, 0) if later == "dense" else (2, 1, 0)), mode[:6]
        assert torch.equal(run.out, ref.out) and not torch.equal(run.out, tp_out)
        got = EC._backward(run, dO, dP, 0.5)
        for kk, v in rg.items():
            assert torch.equal(got[kk], v), (later, kk)


def test_profiler_names_at_most_two_more_in_the_forward_none_in_the_backward():
    cfg, S, P_, B, X, Y, noise, dO, dP = EC._small()
    E = cfg.E
    r_reg, names_reg = _prof_names(lambda: _forward_reg(MoeRun(cfg, P_, B, X, Y, noise=noise), E, 0))
    r_tp, names_tp = _prof_names(lambda: _forward_top_p(MoeRun(cfg, P_, B, X, Y, noise=noise), 0.75, 1, E, 1))
    new = [n for n in names_tp if n not in names_reg]
    assert set(names_reg) <= set(names_tp) and sorted(new) == ["k_top_p_apply", "k_top_p_count"], new
    _, names_one = _prof_names(lambda: _forward_top_p(MoeRun(cfg, P_, B, X, Y, noise=noise), 0.75, 1, E, 1, reports=("choice",)))
    assert [n for n in names_one if n not in names_reg] == ["k_top_p_apply"], "the count launch runs without count or khist asked for"
    _, back_reg = _prof_names(lambda: EC._backward(r_reg, dO, dP, 0.5))
    _, back_tp = _prof_names(lambda: EC._backward(r_tp, dO, dP, 0.5))
    assert back_tp == back_reg, "the backward of a top-p forward adds no launch"


def test_facade_in_training_and_eval_mode_with_a_meter():
    cfg, S, P_, B, X, Y, noise, dO, dP = EC._small()
    E = cfg.E
    m = EC._module(cfg, P_, B)
    x4, y4 = _tokens4(X, Y)
    m.train()
    m(x4, y4, is_training=True)
    assert m.last_top_p is None
    m.router_top_p, m.router_top_p_min_k, m.router_top_k, m.router_top_k_renorm = 0.75, 1, 3, True
    m.expert_dropout, m.router_aux = 0.4, True
    meter = TopPMeter([m])
    torch.manual_seed(3)
    out, idx, probs, lb = m(x4, y4, is_training=True)
    rep = m.last_top_p
    assert [t.dtype for t in rep] == [torch.int32] * 3 and [tuple(t.shape) for t in rep] == [(S,), (E,), (E + 1,)]
    psm, w = EC._module_psm_w(m, S, E)
    _check_mode(_module_mode(m), 0.75, 1, 3, 1)
    mix = m.__dict__["_mix_last"].cpu().numpy()
    assert (mix == 0).any() and (mix != 0).any(), "the expert-dropout draw shows nothing"
    mask = R.check_selection(psm, 0.75, 1, 3, 1, mix, rep.choice.cpu().numpy(), rep.count.cpu().numpy(), rep.khist.cpu().numpy(), w)
    assert np.array_equal(probs.reshape(S, E).detach().cpu().numpy(), psm)
    ra = m.last_router_aux
    assert np.array_equal(ra.load.detach().cpu().numpy().view(np.uint32), R.load_of(mask).view(np.uint32))
    torch.autograd.backward([out, lb + ra.z_loss + ra.balance_loss], [torch.randn_like(out), None])
    assert bool(torch.isfinite(x4.grad).all()) and float(x4.grad.abs().max()) > 0
    assert all(bool(torch.isfinite(p_.grad).all()) for p_ in m.parameters() if p_.grad is not None)
    # eval mode: the same rule (per frame, independent of the batch), no multiplier; equal to the C ABI on the same inputs; k_max = E without router_top_k
    m.eval()
    m.router_top_k, m.router_top_p_min_k, m.router_top_k_renorm = None, 2, False
    with torch.no_grad():
        out_e = m(x4, y4, is_training=False)[0]
    rep_e = m.last_top_p
    psm, w = EC._module_psm_w(m, S, E)
    _check_mode(_module_mode(m), 0.75, 2, E, 0)
    mask_e = R.check_selection(psm, 0.75, 2, E, 0, None, rep_e.choice.cpu().numpy(), rep_e.count.cpu().numpy(), rep_e.khist.cpu().numpy(), w)
    sd = {kk: v.detach().cpu() for kk, v in m.state_dict().items()}      # (the training forward above moved the BatchNorm statistics)
    run = _forward_top_p(MoeRun(cfg, {kk: sd[kk] for kk in P_}, {kk: sd[kk] for kk in B}, X, Y, training=False), 0.75, 2, E, 0)
    _close(out_e.squeeze(-1).permute(0, 2, 1).float().cpu(), run.out.float().cpu(), 1e-6, "eval-mode facade against the C ABI")
    assert torch.equal(rep_e.choice, run.choice[:S])
    # the meter against a host count of the two calls
    assert meter.calls == [2]
    assert meter.khist[0].cpu().tolist() == (R.khist_of(mask).astype(np.int64) + R.khist_of(mask_e)).tolist()
    assert meter.count[0].cpu().tolist() == (mask.sum(0) + mask_e.sum(0)).tolist()
    assert meter.mean_experts()[0] == pytest.approx((mask.sum() + mask_e.sum()) / (2 * S))
    meter.reset()
    assert meter.mean_experts() == [None]
    meter.close()
    m.router_top_p = None
    with torch.no_grad():
        m(x4, y4, is_training=False)
    assert m.last_top_p is None and _module_mode(m)[2] == 0 and meter.calls == [0]


def test_adapter_pair_with_top_p_sites_equals_two_sites():
    from avmoe_amd.adapters import AdapterPair
    ca, cb = _pair_cfgs(True)
    torch.manual_seed(5)
    sa, sb = build_module("avs", ca).to(DEV).train(), build_module("avs", cb).to(DEV).train()
    sa.router_top_p, sb.router_top_p, sb.router_top_k, sb.router_top_k_renorm, sb.router_top_p_min_k = 0.9, 0.6, 3, False, 2
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
        reports = tuple(tuple(t.clone() for t in m.last_top_p) for m in (a, b))
        return ((oa.detach().float(), ov.detach().float()), (xa.grad.float(), xv.grad.float()), [p.grad.clone() for m in (a, b) for p in m.parameters()],
                reports)

    ref = run(ra, rb, None)
    for concurrent in (True, False):                      # two-stream and one-stream mode
        got = run(sa, sb, AdapterPair(sa, sb, concurrent=concurrent))
        for r_, g_ in zip(ref[3], got[3]):
            assert all(torch.equal(x_, y_) for x_, y_ in zip(r_, g_)), "the pair's choice / count / khist are not the two sites'"
        for (choice, count, khist), lo, hi in zip(got[3], (1, 2), (4, 3)):
            assert int(khist.sum()) == S and int(khist[:lo].sum()) == 0 and int(khist[hi + 1:].sum()) == 0
            assert int(count.sum()) == int((khist * torch.arange(khist.numel(), device=DEV)).sum())
        for r_, g_ in zip(ref[0] + ref[1], got[0] + got[1]):
            assert float((r_ - g_).abs().max()) <= 1e-5 * float(r_.abs().max())
        for r_, g_ in zip(ref[2], got[2]):
            assert float((r_ - g_).abs().max()) <= 1e-4 * max(float(r_.abs().max()), 1e-6)


def test_captured_facade_step_with_top_p_replays_with_equal_reports():
    """One small single-stream site through the FACADE -- which allocates the report tensors in every call -- with top-p routing, forward +
    backward captured with torch.cuda.graph on one stream as tests/test_expert_choice_gpu.py captures its step: two replays equal the eager
    step bit for bit in the output, the three reports, the token and the parameter gradients."""
    from tests.golden_util import load_golden, split_params
    meta, cfg, t = load_golden("ave_train")
    P_, B = split_params(t)
    m = build_module(meta["which"], cfg).to(DEV)
    m.load_state_dict({**P_, **B}, strict=True)
    m.train()
    m.shared_gpu = False
    m.router_top_p, m.router_top_k_renorm = 0.6, True
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
        return [out.detach().clone()] + [x_.clone() for x_ in m.last_top_p] + [X.grad.clone(), Y.grad.clone()] + [p_.grad.clone() for p_ in m.parameters()]

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
    assert np.array_equal(bits.sum(0), eager[2].cpu().numpy()) and np.array_equal(R.khist_of(bits), eager[3].cpu().numpy())
    assert (bits.sum(1) >= 1).all() and float(eager[0].abs().max()) > 0
    clear()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        out = step()
    for i in range(2):
        graph.replay()
        for j, (a_, b_) in enumerate(zip(snapshot(out), eager)):
            assert torch.equal(a_, b_), (i, j)
