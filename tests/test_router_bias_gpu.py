"""Aux-loss-free expert balancing on the GPU (avmoe_moe_forward_bias / avmoe_router_bias_update, include/avmoe.h): the selection exact on
every frame from the library's own softmax, outputs and gradients of the four bottleneck-space kernel families against tests/topk_ref.py
with sel = the k highest p + b, the neutral elements, a backward that does not see later bias updates, the counts, the update kernel bit
for bit against tests/router_bias_ref.py, the trajectory of forward + step, AdapterPair, a captured graph and two ranks over gloo."""
import copy
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from avmoe_amd import _capi as capi
from avmoe_amd import _capi_moe as cm
from avmoe_amd.train import RouterBiasBalancer
from oracle import avmoe_oracle as O
from tests import router_bias_ref as R
from tests.moe_gpu_util import MoeRun
from tests.router_aux_ref import scalar_close
from tests.router_grad_util import assert_close
from tests.test_adapters_api import build_module
from tests.test_router_bias_host import _bias_for
from tests.test_router_topk_gpu import _bf16_budget, _close, _dense_bf16, _eager_bf16, _pair_cfgs, _prof_names
from tests.topk_families import FAMILIES, family_config
from tests.topk_ref import topk_forward, topk_grads

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")


def _p(t):
    return t.data_ptr() if t is not None else None


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _forward_bias(run, k, renorm, bias=None, count=None, aux=False, entry="bias", sync=True):
    """avmoe_moe_forward_bias on a MoeRun (entry 'reg': avmoe_moe_forward_reg with the same arguments less the two new ones)"""
    if aux:
        run.aux, run.load = torch.full((2,), NAN, device=DEV), torch.full((run.cfg.E,), NAN, device=DEV)
    else:
        run.aux = run.load = None
    head = (C.byref(run.desc), run.X.data_ptr(), run.Y.data_ptr(), C.byref(run.ptrs), _p(run.noise), k, int(renorm), None)
    tail = (run.out.data_ptr(), run.probs.data_ptr(), run.idx.data_ptr(), run.lb.data_ptr(), _p(run.aux), _p(run.load), run.saved.data_ptr(),
            run.scratch.data_ptr(), _stream())
    if entry == "reg":
        capi.check(run.L.avmoe_moe_forward_reg(*head, *tail), "avmoe_moe_forward_reg")
    else:
        capi.check(run.L.avmoe_moe_forward_bias(*head, _p(bias), _p(count), *tail), "avmoe_moe_forward_bias")
    if sync:
        torch.cuda.synchronize()
    return run


def _backward(run, dO, dP, lb_weight, aux_grad=None):
    """avmoe_moe_backward_aux after the forward -> {'X', 'Y', parameter key: gradient} on the CPU"""
    dOd = dO.to(DEV, run.tdt).contiguous() if dO is not None else None
    dPd = dP.to(DEV, torch.float32).contiguous() if dP is not None else None
    ag = torch.tensor(aux_grad, dtype=torch.float32, device=DEV) if aux_grad is not None else None
    dX, dY = torch.full_like(run.X, NAN), torch.full_like(run.Y, NAN)
    grads = {kk: torch.full_like(v, NAN) for kk, v in run.params.items()}
    gptrs = cm.make_ptrs(grads, run.cfg.E_m, run.cfg.E_s)
    lbw = torch.full((1,), float(lb_weight), device=DEV)
    st = run.L.avmoe_moe_backward_aux(C.byref(run.desc), run.X.data_ptr(), run.Y.data_ptr(), C.byref(run.ptrs), _p(dOd), _p(dPd), lbw.data_ptr(),
                                      _p(ag), run.saved.data_ptr(), run.scratch.data_ptr(), dX.data_ptr(), dY.data_ptr(), C.byref(gptrs), 0, _stream())
    capi.check(st, "avmoe_moe_backward_aux")
    torch.cuda.synchronize()
    g = {kk: v.cpu() for kk, v in grads.items()}
    g["X"], g["Y"] = dX.float().cpu(), dY.float().cpu()
    return g


def _words(run, name, dtype):
    """buffer `name` of `saved`, raw, as a CPU tensor of `dtype`"""
    region, off, nbytes = run.table[name]
    assert region == 0
    return run.saved[off:off + nbytes].view(dtype).cpu()


def _psm_w(run):
    S, E = run.S, run.cfg.E
    return _words(run, "psm", torch.float32)[:S * E].reshape(S, E), _words(run, "probs", torch.float32)[:S * E].reshape(S, E)


def _check_mode(run, k, renorm, bias):
    mode = _words(run, "mode", torch.int32)
    E = run.cfg.E
    assert mode[0] == k and mode[1] == int(renorm)
    if bias is None:
        assert mode[2] == 0
    else:
        assert mode[2] == 1 and torch.equal(mode[16:16 + E], bias.detach().cpu().view(torch.int32)), "mode does not hold the bits of the bias"


# ---- 1. the selection, exact, on every frame --------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("which", ["tile_fast", "e16"])
def test_selection_is_exactly_the_k_highest_p_plus_b_on_every_frame(which, k):
    """S = 300 (the one-block count loop strides past 256) on the tile_fast configuration, and E = 16 = AVMOE_MAX_EXPERTS at S = 5.
    Renorm off, no multiplier: w != 0 must be topk_mask(psm + b, k) from the library's own psm for EVERY frame, and w = m p bit for bit."""
    cfg, S, P, B, X, Y, noise, b0 = R.selection_case(which)
    first = _forward_bias(MoeRun(cfg, P, B, X, Y, noise=noise), k, False, b0.to(DEV))
    psm0, _ = _psm_w(first)
    b, a, c = R.with_tie(psm0, b0, k)                     # frame 0: the last kept and the first dropped expert get EXACTLY equal scores
    bd, count = b.to(DEV), torch.zeros(cfg.E, device=DEV)
    run = _forward_bias(MoeRun(cfg, P, B, X, Y, noise=noise), k, False, bd, count)
    psm, w = _psm_w(run)
    assert run.guards_intact() and torch.equal(psm, psm0), "the softmax does not depend on the bias"
    R.check_weights(w, psm, b, k, False)                  # every frame, no margin: the selection repeats bit for bit from psm and b
    _check_mode(run, k, False, b)
    sc = psm[0] + b
    assert float(sc[a]) == float(sc[c]) and w[0, min(a, c)] != 0 and w[0, max(a, c)] == 0, "equal scores: expert order decides"
    ch = R.changed_frames(psm, b, k)
    print(f"{which} k={k}: {int(ch.sum())} of {S} frames change their selection; tie in frame 0 between experts {a} and {c} at score {float(sc[a])!r}")
    assert 4 * int(ch.sum()) >= S and int((~ch).sum()) >= 1, f"the draw shows nothing: {int(ch.sum())} of {S} frames changed"
    assert torch.equal(count.cpu(), R.counts_of(R.select_mask(psm, b, k)))
    assert torch.equal(run.probs.cpu(), psm) and torch.equal(run.idx.cpu(), psm.argmax(-1)), "probs / idx are the unbiased softmax's"


# ---- 2. outputs and gradients in every kernel family ------------------------------------------------------------------------------
def _family_data(family, bf16):
    cfg, S, _ = family_config(family)
    P, B = O.init_params(cfg, seed=3)
    g = torch.Generator().manual_seed(17)
    X = 0.3 * torch.randn(S, cfg.Nx, cfg.Cx, generator=g)
    Y = 0.3 * torch.randn(S, cfg.Ny, cfg.Cy, generator=g)
    if bf16:
        X, Y = X.to(torch.bfloat16).float(), Y.to(torch.bfloat16).float()
    dO = torch.randn(S, cfg.Nx, cfg.Cx, generator=g).to(torch.bfloat16).float()
    dP = torch.randn(S, cfg.E, generator=g)
    return cfg, S, P, B, X, Y, dO, dP


@pytest.mark.parametrize("family", list(FAMILIES))
def test_bias_fp32_in_every_kernel_family(family):
    """k = 1 without renormalisation, and k = 2 renormalised with the router auxiliary losses on: load is the biased mask's column share
    exactly, balance = E sum_e load_e P_e, and its gradient -- d balance / d p_se = E load_e / S, the load carries none -- is that of
    <probs, g_b E load / S>, which topk_grads forms."""
    cfg, S, P, B, X, Y, dO, dP = _family_data(family, False)
    dense = MoeRun(cfg, P, B, X, Y).forward()
    for k, renorm, aux in ((1, False, False), (2, True, True)):
        what = f"{family}/k={k}/renorm={renorm}"
        b = _bias_for(dense.probs.cpu(), k, 3 + k)
        sel = R.select_mask(dense.probs.cpu(), b, k)
        run = _forward_bias(MoeRun(cfg, P, B, X, Y), k, renorm, b.to(DEV), None, aux=aux)
        assert torch.equal(run.probs, dense.probs) and torch.equal(run.idx, dense.idx) and torch.equal(run.lb, dense.lb)
        psm, w = _psm_w(run)
        assert torch.equal(psm, dense.probs.cpu())
        R.check_weights(w, psm, b, k, renorm)
        _check_mode(run, k, renorm, b)
        dPr, ag = dP, None
        if aux:
            load = R.counts_of(sel) / (S * k)
            assert torch.equal(run.load.cpu(), load), what + ": load is not the biased selection's share"
            scalar_close(run.aux[1], cfg.E * float((load.double() * psm.double().mean(0)).sum()), what + "/balance")
            g_b = -1.1
            ag, dPr = (0.0, g_b), dP + g_b * cfg.E * load[None, :] / S
        got = _backward(run, dO, dP, 0.5, ag)
        assert run.guards_intact()
        ref = topk_grads(cfg, P, B, X, Y, dO, dPr, 0.5, True, k, renorm, sel=sel)
        _close(run.out.float().cpu(), topk_forward(P, B, X, Y, cfg, k, renorm, training=True, update_buffers=False, sel=sel)["out"], 1e-3, what + "/out")
        assert_close(got, ref, rtol=1e-3, floor_frac=1e-2, what=what)


def test_bias_bf16_streaming_family_within_budget():
    """The tile_stream family in bf16 by the budget method of tests/test_router_topk_gpu.py: against eager bf16 and the unbiased dense site."""
    cfg, S, P, B, X, Y, dO, dP = _family_data("tile_stream", True)
    with capi.test_hooks(capi.HOOK_KFS_FORCE):
        dense = MoeRun(cfg, P, B, X, Y, bf16=True).forward()
        dense_pair = _dense_bf16(dense, cfg, P, B, X, Y, dO, dP, 0.5, True, None, None)
        for k, renorm in ((1, False), (2, True)):
            b = _bias_for(dense.probs.cpu(), k, 3 + k)
            sel = R.select_mask(dense.probs.cpu(), b, k)
            (run, got), names = _prof_names(lambda: (lambda r: (r, _backward(r, dO, dP, 0.5)))(
                _forward_bias(MoeRun(cfg, P, B, X, Y, bf16=True), k, renorm, b.to(DEV))))
            assert run.guards_intact() and any(n.endswith("(stream)") for n in names), names
            R.check_weights(_psm_w(run)[1], dense.probs.cpu(), b, k, renorm)
            got["out"] = run.out.float().cpu()
            ref = topk_grads(cfg, P, B, X, Y, dO, dP, 0.5, True, k, renorm, sel=sel)
            ref["out"] = topk_forward(P, B, X, Y, cfg, k, renorm, training=True, update_buffers=False, sel=sel)["out"]
            _bf16_budget(got, ref, _eager_bf16(cfg, P, B, X, Y, dO, dP, 0.5, True, k, renorm, None, None, sel), dense_pair,
                         f"tile_stream/k={k}/renorm={renorm}")


# ---- 3. neutral elements ------------------------------------------------------------------------------------------------------------
def _small():
    cfg, S, P, B, X, Y, dO, dP = _family_data("tile_fast", False)
    noise = torch.randn(S, cfg.E, generator=torch.Generator().manual_seed(2))
    return cfg, S, P, B, X, Y, dO, dP, noise


def test_zero_bias_and_null_are_the_unbiased_call_bitwise():
    cfg, S, P, B, X, Y, dO, dP, noise = _small()

    def step(entry, bias):
        run = _forward_bias(MoeRun(cfg, P, B, X, Y, noise=noise), 2, True, bias, None, aux=True, entry=entry)
        return run, _backward(run, dO, dP, 0.5, (0.9, -1.1))
    (ref, gref), names_reg = _prof_names(lambda: step("reg", None))
    (nul, gnul), names_null = _prof_names(lambda: step("bias", None))
    assert names_null == names_reg, "NULL / NULL must run avmoe_moe_forward_reg's launches"
    zer, gzer = step("bias", torch.zeros(cfg.E, device=DEV))
    _check_mode(ref, 2, True, None), _check_mode(nul, 2, True, None), _check_mode(zer, 2, True, torch.zeros(cfg.E))
    for run, g in ((nul, gnul), (zer, gzer)):
        for a_, b_ in ((run.out, ref.out), (run.probs, ref.probs), (run.idx, ref.idx), (run.lb, ref.lb), (run.aux, ref.aux), (run.load, ref.load)):
            assert torch.equal(a_, b_)
        assert all(torch.equal(x, y) for x, y in zip(_psm_w(run), _psm_w(ref)))
        for kk, v in gref.items():
            assert torch.equal(g[kk], v), kk


def test_bias_on_a_dense_mixture_is_refused():
    cfg, S, P, B, X, Y, dO, dP, noise = _small()
    run = MoeRun(cfg, P, B, X, Y)
    b = torch.zeros(cfg.E, device=DEV)
    for k in (0, cfg.E):
        with pytest.raises(capi.AvmoeError, match="select_bias"):
            _forward_bias(run, k, True, b)
    m = build_module("avs", cfg).to(DEV)
    bal = RouterBiasBalancer([m])
    x4, y4 = X.to(DEV).permute(0, 2, 1).unsqueeze(-1), Y.to(DEV).permute(0, 2, 1).unsqueeze(-1)
    for top_k in (None, cfg.E):
        m.router_top_k = top_k
        with pytest.raises(ValueError, match="router_select_bias"):
            m(x4, y4, is_training=True)
    bal.detach()
    m(x4, y4, is_training=True)                           # the dense site runs again


# ---- 4. the backward does not see later updates -----------------------------------------------------------------------------------
def test_backward_reads_the_bias_its_forward_used():
    cfg, S, P, B, X, Y, dO, dP, noise = _small()
    L = capi.lib()
    k, E = 2, cfg.E
    dense = MoeRun(cfg, P, B, X, Y, noise=noise).forward()
    b = _bias_for(dense.probs.cpu(), k, 5)
    later = -b
    assert bool((R.select_mask(dense.probs.cpu(), b, k) != R.select_mask(dense.probs.cpu(), later, k)).any()), "the later bias selects alike"
    grads = []
    Et = torch.tensor([E], dtype=torch.int32, device=DEV)
    for overwrite in (False, True):
        bias, counts = torch.zeros(1, 16, device=DEV), torch.zeros(1, 16, device=DEV)
        bias[0, :E] = b.to(DEV)
        run = _forward_bias(MoeRun(cfg, P, B, X, Y, noise=noise), k, True, bias[0, :E], counts[0, :E], aux=True)
        if overwrite:                                     # the live tensor moves on: other values, then a balancer step on top
            bias[0, :E] = later.to(DEV)
            capi.check(L.avmoe_router_bias_update(bias.data_ptr(), counts.data_ptr(), Et.data_ptr(), 1, 0.05, _stream()), "avmoe_router_bias_update")
            torch.cuda.synchronize()
            assert not torch.equal(bias[0, :E].cpu(), b) and float(counts.sum()) == 0.0
        _check_mode(run, k, True, b)
        grads.append(_backward(run, dO, dP, 0.5, (0.9, -1.1)))
    for kk, v in grads[0].items():
        assert torch.equal(grads[1][kk], v), f"{kk}: the backward followed the live bias"


# ---- 5. counts ----------------------------------------------------------------------------------------------------------------------
def test_counts_add_up_in_training_and_stay_put_in_eval():
    cfg, S, P, B, X, Y, dO, dP, noise = _small()
    k = 2
    m = build_module("avs", cfg).to(DEV)
    m.load_state_dict({**P, **B}, strict=True)
    m.router_top_k, m.router_top_k_renorm = k, False
    from avmoe_amd.debug import keep_saved
    keep_saved(m)
    bal = RouterBiasBalancer([m], rate=1e-3)
    x4, y4 = X.to(DEV).permute(0, 2, 1).unsqueeze(-1), Y.to(DEV).permute(0, 2, 1).unsqueeze(-1)
    m.eval()
    probs = m(x4, y4, is_training=False)[2].reshape(S, cfg.E).cpu()
    b = _bias_for(probs, k, 9)
    bal.bias[0, :cfg.E] = b.to(DEV)

    def psm_w():
        desc, saved = m.__dict__["_last_saved"]
        t = {n: (o, nb) for n, _r, o, nb in cm.buffer_table(capi.lib(), desc)}
        torch.cuda.synchronize()
        get = lambda n: saved[t[n][0]:t[n][0] + t[n][1]].view(torch.float32)[:S * cfg.E].reshape(S, cfg.E).cpu()
        return get("psm"), get("probs")
    m(x4, y4, is_training=False)                          # eval: the bias is applied, nothing is counted
    psm, w = psm_w()
    R.check_weights(w, psm, b, k, False)
    assert float(bal.counts.abs().sum()) == 0.0
    m.train()
    want = torch.zeros(cfg.E)
    for seed in (1, 2):                                   # two training forwards (the AVS logit noise differs): the two masks' column sums
        torch.manual_seed(seed)
        m(x4, y4, is_training=True)
        psm, w = psm_w()
        R.check_weights(w, psm, b, k, False)
        want += R.counts_of(R.select_mask(psm, b, k))
    assert torch.equal(bal.counts[0, :cfg.E].cpu(), want) and float(want.sum()) == 2 * S * k
    assert torch.equal(bal.loads()[0].cpu(), want / want.sum())
    m.router_select_count = None                          # no count pointer: the tensor is left alone (and the bias still applies)
    m(x4, y4, is_training=True)
    R.check_weights(psm_w()[1], psm_w()[0], b, k, False)
    assert torch.equal(bal.counts[0, :cfg.E].cpu(), want) and float(bal.counts[0, cfg.E:].abs().sum()) == 0.0


# ---- 6. the update kernel alone -------------------------------------------------------------------------------------------------------
def _update_tables(n, e_shift, seed):
    rng = np.random.default_rng(seed)
    E = [(2, 4, 8, 16)[(i + e_shift) % 4] for i in range(n)]
    if n >= 8:
        E[5], E[6] = 0, 17                                # rows the kernel must skip
    bias = np.full((n, 16), np.nan, np.float32)
    counts = np.full((n, 16), np.nan, np.float32)
    for i, e in enumerate(E):
        e_ = min(max(e, 0), 16)
        bias[i, :e_] = (rng.standard_normal(e_) * 0.01).astype(np.float32)
        pat = i % 5
        if pat == 0:
            c = np.full(e_, 7.0)                          # balanced: nothing moves, the counts are cleared
        elif pat == 1:
            c = np.zeros(e_); c[rng.integers(0, max(e_, 1))] = 320.0      # all on one expert
        elif pat == 2:
            c = np.zeros(e_)                              # tot == 0: the row is left alone
        elif pat == 3:
            c = np.full(e_, 5.0); c[0] += 3; c[-1] -= 3   # two-way ties at the mean for the experts between (E >= 3)
        else:
            c = rng.integers(0, 1000, e_).astype(np.float64)
        counts[i, :e_] = c.astype(np.float32)
    return bias, counts, E


@pytest.mark.parametrize("rate", [1e-3, 0.0])
@pytest.mark.parametrize("n", [1, 3, 48])
def test_update_kernel_matches_the_reference_bitwise(n, rate):
    L = capi.lib()
    for e_shift in (range(4) if n == 1 else (0, 1)):
        for seed in range(5 if n == 1 else 1):            # (n = 1: every count pattern on the one row)
            bias, counts, E = _update_tables(5 if n == 1 else n, e_shift, seed)
            if n == 1:
                bias, counts, E = bias[seed:seed + 1].copy(), counts[seed:seed + 1].copy(), E[seed:seed + 1]
            Et = torch.tensor(E, dtype=torch.int32, device=DEV)
            outs = []
            for _ in range(2):                            # two identical calls: identical bytes
                bt, ct = torch.from_numpy(bias).to(DEV), torch.from_numpy(counts).to(DEV)
                capi.check(L.avmoe_router_bias_update(bt.data_ptr(), ct.data_ptr(), Et.data_ptr(), len(E), rate, _stream()), "avmoe_router_bias_update")
                torch.cuda.synchronize()
                outs.append((bt.cpu().numpy(), ct.cpu().numpy()))
            assert outs[0][0].tobytes() == outs[1][0].tobytes() and outs[0][1].tobytes() == outs[1][1].tobytes()
            R.check_update(bias, counts, E, rate, *outs[0])
            for i, e in enumerate(E):
                if 1 <= e <= 16:
                    assert np.all(outs[0][1][i, :e] == 0), "counts are zero afterwards"
                    assert np.all(np.isnan(outs[0][0][i, e:])) and np.all(np.isnan(outs[0][1][i, e:])), "columns >= E were touched"
            bt, ct = torch.from_numpy(bias).to(DEV), torch.from_numpy(counts).to(DEV)      # refusals write nothing
            for args in ((bt.data_ptr(), ct.data_ptr(), Et.data_ptr(), 0, 1e-3), (bt.data_ptr(), ct.data_ptr(), Et.data_ptr(), len(E), -1e-3),
                         (bt.data_ptr(), ct.data_ptr(), Et.data_ptr(), len(E), NAN), (None, ct.data_ptr(), Et.data_ptr(), len(E), 1e-3)):
                assert L.avmoe_router_bias_update(*args, _stream()) == -1
            torch.cuda.synchronize()
            assert bt.cpu().numpy().tobytes() == bias.tobytes() and ct.cpu().numpy().tobytes() == counts.tobytes()


# ---- 7. trajectory ------------------------------------------------------------------------------------------------------------------
def test_trajectory_follows_the_reference_recurrence_and_narrows_the_spread():
    cfg, S, P, B, X, Y, noise = R.trajectory_case()
    E, k = cfg.E, R.TRAJ_K
    m = build_module("avs", cfg).to(DEV)
    m.load_state_dict({**P, **B}, strict=True)
    bal = RouterBiasBalancer([m], rate=R.TRAJ_RATE)
    run = MoeRun(cfg, P, B, X, Y, noise=noise, training=False)      # fixed parameters: eval-mode BatchNorm, the same softmax every round
    biases, counts, psms = [], [], []
    for t in range(R.TRAJ_ROUNDS):
        _forward_bias(run, k, True, m.router_select_bias, m.router_select_count, sync=False)
        if t in (0, R.TRAJ_ROUNDS - 1):
            psms.append(_psm_w(run)[0])
        counts.append(bal.counts[0, :E].clone())
        bal.step()
        biases.append(bal.bias[0, :E].clone())
    torch.cuda.synchronize()
    assert torch.equal(psms[0], psms[1])
    after, loads = R.trajectory([psms[0]] * R.TRAJ_ROUNDS, E, k, R.TRAJ_RATE)
    got = np.stack([b.cpu().numpy() for b in biases])
    assert got.view(np.uint32).tolist() == after.view(np.uint32).tolist(), "the bias left the reference recurrence"
    got_loads = np.stack([c.cpu().numpy().astype(np.float64) / (S * k) for c in counts])
    assert np.array_equal(got_loads, loads)
    print(f"load round 1 {got_loads[0]} spread {R.spread(got_loads[0])}; round {R.TRAJ_ROUNDS} {got_loads[-1]} spread {R.spread(got_loads[-1])}; "
          f"bias {got[-1]}")
    assert R.spread(got_loads[-1]) < R.spread(got_loads[0]), (got_loads[0], got_loads[-1])
    assert float(bal.counts.abs().sum()) == 0.0


# ---- 8. the facade: AdapterPair, a captured graph -----------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["cfg2_bf16", "small_f32"])
def test_adapter_pair_with_biased_sites_equals_two_sites(shape):
    from avmoe_amd.adapters import AdapterPair
    bf16 = shape == "cfg2_bf16"
    ca, cb = _pair_cfgs(not bf16)
    dt = torch.bfloat16 if bf16 else torch.float32
    torch.manual_seed(5)
    sa, sb = build_module("avs", ca).to(DEV).train(), build_module("avs", cb).to(DEV).train()
    sa.router_top_k, sb.router_top_k, sb.router_top_k_renorm = 2, 1, False
    with torch.no_grad():
        for m in (sa, sb):
            for kk, p in m.named_parameters():
                if kk.endswith(("gate", "gate_av")):
                    p.fill_(0.3)
    ra, rb = copy.deepcopy(sa), copy.deepcopy(sb)
    g = torch.Generator().manual_seed(9)
    S = 4
    fa = (0.5 * torch.randn(S, ca.Cx, ca.Nx, 1, generator=g)).to(DEV, dt)
    fv = (0.5 * torch.randn(S, cb.Cx, cb.Nx, 1, generator=g)).to(DEV, dt)
    ga, gv = torch.randn(S, ca.Cx, ca.Nx, 1, generator=g).to(DEV, dt), torch.randn(S, cb.Cx, cb.Nx, 1, generator=g).to(DEV, dt)
    bufs = [{kk: b.clone() for kk, b in m.named_buffers()} for m in (sa, sb)]
    with torch.no_grad():                                 # the unbiased probabilities, to draw a bias that changes the selection
        pa = sa.eval()(fa, fv, is_training=False)[2].reshape(S, -1).float().cpu()
        pb = sb.eval()(fv, fa, is_training=False)[2].reshape(S, -1).float().cpu()
    sa.train(), sb.train()
    ba, bb = _bias_for(pa, 2, 1), _bias_for(pb, 1, 2)
    bal_s, bal_r = RouterBiasBalancer([sa, sb]), RouterBiasBalancer([ra, rb])
    for bal in (bal_s, bal_r):
        bal.bias[0, :ca.E], bal.bias[1, :cb.E] = ba.to(DEV), bb.to(DEV)
    assert sa.router_select_bias.data_ptr() != sb.router_select_bias.data_ptr()      # the two sites of a pair write different rows

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
        return (oa.detach().float(), ov.detach().float()), (xa.grad.float(), xv.grad.float()), [p.grad.clone() for m in (a, b) for p in m.parameters()]

    ref = run(ra, rb, None)
    got = run(sa, sb, AdapterPair(sa, sb, concurrent=True))
    ttol = 2e-2 if bf16 else 1e-5
    for r_, g_ in zip(ref[0] + ref[1], got[0] + got[1]):
        assert float((r_ - g_).abs().max()) <= ttol * float(r_.abs().max())
    for r_, g_ in zip(ref[2], got[2]):
        assert float((r_ - g_).abs().max()) <= 1e-4 * max(float(r_.abs().max()), 1e-6)
    for bal in (bal_s, bal_r):                            # every frame counted k times, in each site's own row
        assert float(bal.counts[0].sum()) == 2 * S and float(bal.counts[1].sum()) == 1 * S
    # the bias did something: the unbiased pair differs
    bal_s.detach()
    plain = run(sa, sb, AdapterPair(sa, sb, concurrent=True))
    assert float((plain[0][0] - got[0][0]).abs().max()) > 1e-3 * float(got[0][0].abs().max()), "the bias had no effect on the pair"


def test_captured_graph_of_forward_backward_and_step_replays_bitwise():
    """Forward (biased top-k, counting) + backward of two sites + ONE avmoe_router_bias_update, captured on one stream: three replays equal
    three eager steps bit for bit in bias, counts, outputs and gradients (built as tests/test_graph_capture_gpu.py builds its pair step)."""
    kw = dict(reduction=2, groups=2, K=32, variant="avs", lb_loss=True)
    ca = O.AdapterConfig(Cx=128, Nx=150, Cy=64, Ny=50, **kw)
    cb = O.AdapterConfig(Cx=64, Nx=50, Cy=128, Ny=150, **kw)
    S, rate = 4, 0.02
    L = capi.lib()
    g = torch.Generator().manual_seed(0)
    Xa = 0.3 * torch.randn(S, ca.Nx, ca.Cx, generator=g)
    Xb = 0.3 * torch.randn(S, cb.Nx, cb.Cx, generator=g)
    bias, counts = torch.zeros(2, 16, device=DEV), torch.zeros(2, 16, device=DEV)
    Et = torch.tensor([ca.E, cb.E], dtype=torch.int32, device=DEV)
    runs = []
    for i, (cfg, X, Y, seed, k) in enumerate(((ca, Xa, Xb, 1, 2), (cb, Xb, Xa, 2, 1))):
        P, B = O.init_params(cfg, seed=seed)
        r = MoeRun(cfg, P, B, X, Y, bf16=True, training=False, noise=torch.randn(S, cfg.E, generator=g))
        r.top_k, r.b, r.c = k, bias[i, :cfg.E], counts[i, :cfg.E]
        _forward_bias(r, k, True, r.b, r.c)
        r.backward(torch.randn(S, cfg.Nx, cfg.Cx, generator=g))
        runs.append(r)

    def calls(stream):
        for r in runs:
            capi.check(L.avmoe_moe_forward_bias(C.byref(r.desc), r.X.data_ptr(), r.Y.data_ptr(), C.byref(r.ptrs), r.noise.data_ptr(), r.top_k, 1,
                                                None, r.b.data_ptr(), r.c.data_ptr(), r.out.data_ptr(), r.probs.data_ptr(), r.idx.data_ptr(),
                                                r.lb.data_ptr(), None, None, r.saved.data_ptr(), r.scratch.data_ptr(), stream), "forward_bias")
        for r in runs:
            capi.check(L.avmoe_moe_backward(C.byref(r.desc), r.X.data_ptr(), r.Y.data_ptr(), C.byref(r.ptrs), r.dOut.data_ptr(), None,
                                            r.saved.data_ptr(), r.scratch.data_ptr(), r.dX.data_ptr(), r.dY.data_ptr(), C.byref(r.gptrs),
                                            stream), "backward")
        capi.check(L.avmoe_router_bias_update(bias.data_ptr(), counts.data_ptr(), Et.data_ptr(), 2, rate, stream), "bias_update")

    def snapshot():
        torch.cuda.synchronize()
        return [bias.clone(), counts.clone()] + [t.clone() for r in runs for t in (r.out, r.dX, r.dY, *r.grads.values())]

    def reset():
        bias.zero_(), counts.zero_()
        for r in runs:
            for t_ in (r.out, r.dX, r.dY, *r.grads.values()):
                t_.zero_()
        torch.cuda.synchronize()

    s = torch.cuda.Stream()
    reset()
    eager = []
    with torch.cuda.stream(s):
        for _ in range(3):
            calls(s.cuda_stream)
            eager.append(snapshot())
    assert not torch.equal(eager[0][0], eager[2][0]), "the bias did not move between the steps"
    reset()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        calls(torch.cuda.current_stream().cuda_stream)
    reset()
    for step in range(3):
        graph.replay()
        for i, (a_, b_) in enumerate(zip(snapshot(), eager[step])):
            assert torch.equal(a_, b_), (step, i)


# ---- 9. two ranks ---------------------------------------------------------------------------------------------------------------------
def _rank_worker(rank, world, port, out):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        sys.path.insert(0, ROOT)
        cfg = O.AdapterConfig(Cx=64, Nx=72, Cy=48, Ny=40, reduction=4, groups=2, K=32, variant="avs", E_m=2, E_s=2, lb_loss=True)
        torch.manual_seed(0)                              # identical parameters on every rank
        m = build_module("avs", cfg).to(DEV).train()
        m.router_top_k = 2
        bal = RouterBiasBalancer([m], rate=1e-3)
        g = torch.Generator().manual_seed(100 + rank)     # the ranks see different clips; per-frame offsets spread the routing out
        S = 6
        x = (0.5 * torch.randn(S, cfg.Cx, cfg.Nx, 1, generator=g) + 2.0 * torch.randn(S, cfg.Cx, 1, 1, generator=g)).to(DEV)
        y = (0.5 * torch.randn(S, cfg.Cy, cfg.Ny, 1, generator=g) + 2.0 * torch.randn(S, cfg.Cy, 1, 1, generator=g)).to(DEV)
        m(x, y, is_training=True)
        own = bal.counts.clone().cpu()
        bal.step()
        torch.cuda.synchronize()
        out[rank] = (own.numpy(), bal.bias.cpu().numpy(), bal.counts.cpu().numpy())
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_two_ranks_make_the_same_update_from_the_summed_counts():
    import torch.multiprocessing as mp
    from tests.test_dp_gpu_gloo import _free_port
    world = 2
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_rank_worker, args=(world, _free_port(), out), nprocs=world, join=True)
    res = dict(out)
    assert sorted(res) == [0, 1]
    (c0, b0, z0), (c1, b1, z1) = res[0], res[1]
    print(f"counts rank 0 {c0[0, :4]} rank 1 {c1[0, :4]} bias {b0[0, :4]}")
    assert c0[0, :4].sum() == 12 and c1[0, :4].sum() == 12 and not np.array_equal(c0, c1), "the ranks' clips select alike: the test shows nothing"
    assert b0.tobytes() == b1.tobytes(), "the ranks' biases differ"
    R.check_update(np.zeros((1, 16), np.float32), c0 + c1, [4], 1e-3, b0, z0)
    assert np.all(z1 == 0)
