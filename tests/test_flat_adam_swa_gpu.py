"""Stochastic weight averaging in FlatAdam on the device (avmoe_amd.train.FlatAdam(swa_start=..., swa_freq=...), LRSchedule(swa_start=...);
include/avmoe.h: avmoe_opt_swa, avmoe_opt_grad_norm_swa) on the two-bucket model of tests/test_flat_adam_ema_gpu.py -- parameter lengths
1, 3, 4, 5, 1023, 1024, 1025 and 2049, the tail and block-boundary cases of the kernels.  T = 24 steps, the average starts at applied step
N = 5 and takes every c = 3rd step from there: steps 5, 8, ..., 23, seven models.

Tolerance of the average against the fp64 mean of the parameters' snapshots at the averaging steps: the update is the exponential
average's, shadow' = fma(d, shadow, fl(fl(1 - d) * p)), so the bound is the one tests/test_flat_adam_ema_gpu.py derives for it --
at most 5 u A per step (u = 2^-24, A = max|p|), taken as 6, of which 2 u A are for a d that is one fp32 rounding away from the exact
k / (k + 1) the mean is defined by; errors do not grow under a convex combination, and a step with d = 1 or d = 0 adds none:
|shadow - mean| <= 6 T u A.  (A host emulation of the kernel's arithmetic at T = 64 gave 1.2e-7 against a bound of 3.2e-5.)
The fp64 mean itself against torch's AveragedModel in double, fed the same snapshots: AveragedModel's running form rounds a subtraction,
a division and an addition per model, each at most 2^-53 * 2 A, and the stacked mean a sum of m values: 8 m 2^-53 A for m models.

Learning-rate factor: the criterion of tests/test_flat_adam_schedule_gpu.py, 1 fp32 ulp of float32(LRSchedule.factor(n)).
Everything that is the same kernels on the same bits is held to bit-equality."""
import copy
import io

import numpy as np
import pytest
import torch

from tests.test_flat_adam_device_gpu import ulps
from tests.test_flat_adam_ema_gpu import (LR, MAX_NORM, WD, assert_flats_equal, bits, clone_params, flats, grads, make_opt, make_params,
                                          set_grads)

pytestmark = pytest.mark.gpu

T, N, FREQ = 24, 5, 3
AVG_STEPS = [n for n in range(1, T + 1) if n >= N and (n - N) % FREQ == 0]
U = 2.0 ** -24


def f32(x):
    return float(np.float32(x))


def f32_bits(x):
    return int(np.float32(x).view(np.int32))


def swa_at(n, start=N, freq=FREQ):
    from avmoe_amd.train import FlatAdam
    return FlatAdam.swa_decay_at(n, start, freq)


def lr_sched(**kw):
    from avmoe_amd.train import LRSchedule
    base = dict(warmup_steps=3, warmup_start=0.1, decay_kind="cosine", total_steps=30, min_factor=0.05)
    base.update(kw)
    return LRSchedule(**base)


def swa_sched(kind="cos"):
    return lr_sched(swa_start=6, swa_factor=0.25, swa_anneal_steps=5, swa_anneal=kind)


def poison(p):
    p.grad.view(-1)[p.numel() // 2] = float("inf")


# ---------------------------------------------------------------------------------------------------------------------
OPTION_SETS = {"clip": dict(max_grad_norm=MAX_NORM),
               "adamw": dict(weight_decay=WD, decoupled_weight_decay=True),
               "skip": dict(weight_decay=WD, max_grad_norm=MAX_NORM, skip_nonfinite=True),
               "schedule": dict(weight_decay=WD, lr_schedule="cosine")}


@pytest.mark.parametrize("name", list(OPTION_SETS))
def test_the_uniform_average_does_not_touch_the_step(name):
    """parameters, moments (alignment padding included) and every word of the state block but the decay after T steps, against the same
    optimizer with ema_decay=0.9: the update kernel is the same, only the rule for d differs.  "skip" holds one step back in both runs."""
    from avmoe_amd import _capi_moe as cm
    dev = torch.device("cuda:0")
    kw = dict(OPTION_SETS[name])
    if kw.get("lr_schedule"):
        kw["lr_schedule"] = lr_sched()
    a = make_params(dev)
    b = clone_params(a)
    gs = grads(T, dev)
    _, oa = make_opt(a, swa_start=N, swa_freq=FREQ, **kw)
    _, ob = make_opt(b, ema_decay=0.9, **kw)
    assert oa._flags & cm.OPT_SWA and not oa._flags & cm.OPT_EMA and ob._flags == (oa._flags & ~cm.OPT_SWA) | cm.OPT_EMA
    for k in range(T):
        set_grads(a, gs[k]); set_grads(b, gs[k])
        if name == "skip" and k == 9:
            poison(a[6]); poison(b[6])
        oa.step(); ob.step()
    assert_flats_equal(flats(oa, "pmv"), flats(ob, "pmv"), name)
    sa, sb = oa.state_block, ob.state_block
    assert set(sa) == set(sb)
    for field in sa:
        if field != "ema_decay":
            assert torch.equal(sa[field].cpu(), sb[field].cpu()), (name, field)
            assert sa[field].dtype == torch.int64 or torch.equal(bits(sa[field]), bits(sb[field])), (name, field)
    applied = T - (name == "skip")
    assert int(oa.applied_steps.item()) == applied and int(oa.skipped_steps.item()) == (name == "skip")
    assert float(oa.last_ema_decay.item()) == swa_at(applied)
    assert any(not torch.equal(x, y) for x, y in zip(oa.ema_params, ob.ema_params))       # two different averages
    if name == "schedule":
        assert int(bits(sa["lr_factor"]).item()) != 0
    else:
        assert int(bits(sa["lr_factor"]).item()) == 0        # never written without a schedule


@pytest.mark.parametrize("start,freq", [(N, FREQ), (1, 1), (T, 7)])
def test_the_decay_on_the_device_is_swa_decay_at_bit_for_bit(start, freq):
    dev = torch.device("cuda:0")
    a = make_params(dev)
    gs = grads(T, dev)
    _, opt = make_opt(a, swa_start=start, swa_freq=freq)
    assert int(bits(opt.last_ema_decay).item()) == 0
    seen = []
    for k in range(T):
        set_grads(a, gs[k]); opt.step()
        got = opt.last_ema_decay
        assert got.dtype == torch.float32 and got.is_cuda
        assert int(bits(got).item()) == f32_bits(swa_at(k + 1, start, freq)), (k + 1, float(got.item()))
        seen.append(float(got.item()))
    if (start, freq) == (N, FREQ):
        assert seen[:5] == [0.0] * 5 and seen[5:8] == [1.0, 1.0, 0.5] and seen[-2:] == [f32(6.0 / 7.0), 1.0]
    if (start, freq) == (1, 1):
        assert seen == [f32(k / (k + 1.0)) for k in range(T)]


def test_the_average_is_the_mean_of_the_snapshots_and_torchs_averaged_model():
    """below N the shadows ARE the parameters; from N on they are the fp64 mean of the snapshots at the averaging steps within the bound
    of the module docstring; and that mean is what torch's AveragedModel holds after the same snapshots"""
    from avmoe_amd.train import FlatAdam
    from torch.optim.swa_utils import AveragedModel
    dev = torch.device("cuda:0")
    a = make_params(dev)
    gs = grads(T, dev)
    _, opt = make_opt(a, weight_decay=WD, max_grad_norm=MAX_NORM, swa_start=N, swa_freq=FREQ)
    holder = torch.nn.ParameterList([torch.nn.Parameter(p.detach().double().cpu()) for p in opt.params])
    swa_model = None
    for e, p in zip(opt.ema_params, opt.params):
        assert torch.equal(bits(e), bits(p.data))             # seeded with the parameters
    snaps, A, worst, checked = [], 0.0, 0.0, 0
    for k in range(T):
        set_grads(a, gs[k]); opt.step()
        n = k + 1
        snap = [p.detach().cpu().clone() for p in opt.params]        # fp32 snapshots
        A = max(A, max(float(s.abs().max()) for s in snap))
        if n in AVG_STEPS:
            snaps.append([s.double() for s in snap])
            with torch.no_grad():
                for h, s in zip(holder, snap):
                    h.copy_(s.double())
            if swa_model is None:
                swa_model = AveragedModel(holder)            # torch's first update_parameters copies: n_averaged = 0
            swa_model.update_parameters(holder)
        if n < N:
            for e, s in zip(opt.ema_params, snap):
                assert torch.equal(e.cpu(), s), n
            continue
        bound = 6 * T * U * A
        for i, e in enumerate(opt.ema_params):
            mean = torch.stack([s[i] for s in snaps]).mean(0)
            err = float((e.double().cpu() - mean).abs().max())
            worst, checked = max(worst, err), checked + 1
            assert err <= bound, (n, i, e.numel(), err, bound)
    m = len(snaps)
    assert m == len(AVG_STEPS) == 7 == FlatAdam.swa_n_averaged_at(T, N, FREQ) == int(swa_model.n_averaged)
    print(f"uniform average over {m} of {T} steps: |shadow - fp64 mean| max {worst:.3e}, bound {6 * T * U * A:.3e} (A = {A:.4f})")
    assert checked == (T - N + 1) * len(opt.params) and worst > 0.0       # fp32 against fp64: not the same arithmetic
    for i, q in enumerate(swa_model.module):
        mean = torch.stack([s[i] for s in snaps]).mean(0)
        assert q.dtype == torch.float64
        assert float((q.detach() - mean).abs().max()) <= 8 * m * 2.0 ** -53 * A, i


def test_skipped_step_leaves_average_decay_and_factor_alone_and_averaging_resumes_a_step_later():
    dev = torch.device("cuda:0")
    a = make_params(dev)
    b = clone_params(a)
    gs = grads(T, dev)
    kw = dict(weight_decay=WD, max_grad_norm=MAX_NORM, skip_nonfinite=True, swa_start=N, swa_freq=FREQ, lr_schedule=swa_sched())
    _, oa = make_opt(a, **kw)
    _, ob = make_opt(b, **kw)                                # b never sees the poisoned gradient
    s = kw["lr_schedule"]
    for k in range(T):
        set_grads(a, gs[k])
        if k == 7:                                          # the call that would have been applied step 8, an averaging step
            poison(a[6])
            before, d_before, f_before = flats(oa), bits(oa.last_ema_decay), bits(oa.last_lr_factor)
            assert float(oa.last_ema_decay.item()) == swa_at(7) == 1.0
            oa.step()
            assert_flats_equal(before, flats(oa), "skipped step")
            assert torch.equal(d_before, bits(oa.last_ema_decay)) and torch.equal(f_before, bits(oa.last_lr_factor))
            assert int(oa.applied_steps.item()) == 7 and int(oa.skipped_steps.item()) == 1 and oa.t == 8
            assert int(oa.state_block["skip"].item()) == 1
            set_grads(a, gs[k]); oa.step()                  # the same gradient, finite: now it is applied step 8
            assert float(oa.last_ema_decay.item()) == swa_at(8) == 0.5
            assert ulps(float(oa.last_lr_factor.item()), f32(s.factor(7))) <= 1
        else:
            oa.step()
        set_grads(b, gs[k]); ob.step()
    assert_flats_equal(flats(oa), flats(ob), "the run around the skipped step")
    assert int(oa.applied_steps.item()) == T == int(ob.applied_steps.item()) and int(ob.skipped_steps.item()) == 0
    for field in ("ema_decay", "lr_factor"):
        assert torch.equal(bits(oa.state_block[field]), bits(ob.state_block[field])), field


def test_captured_step_averages_on_replay_over_the_whole_run():
    dev = torch.device("cuda:0")
    a = make_params(dev)
    b = clone_params(a)
    gs = grads(T, dev)
    kw = dict(weight_decay=WD, max_grad_norm=MAX_NORM, skip_nonfinite=True, swa_start=N, swa_freq=FREQ, lr_schedule=swa_sched("linear"))
    _, oa = make_opt(a, **kw)
    _, ob = make_opt(b, **kw)
    start = flats(ob)
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    eager = []
    with torch.cuda.stream(st):                              # the eager run (it also loads the kernels before the capture)
        for k in range(T):
            set_grads(a, gs[k]); oa.step()
            eager.append((bits(oa.last_ema_decay), bits(oa.last_lr_factor)))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=st):                 # one stream, a linear graph
        ob.step()
    torch.cuda.synchronize()
    assert int(ob.applied_steps.item()) == 0                 # capturing runs nothing
    assert_flats_equal(start, flats(ob), "capture")
    for k in range(T):
        set_grads(b, gs[k])
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(bits(ob.last_ema_decay), eager[k][0]) and torch.equal(bits(ob.last_lr_factor), eager[k][1]), k
        assert float(ob.last_ema_decay.item()) == swa_at(k + 1), k
    assert int(ob.applied_steps.item()) == T and int(ob.skipped_steps.item()) == 0
    assert_flats_equal(flats(oa), flats(ob), "graph replay")
    assert len({int(e[0].item()) for e in eager}) == 2 + len(AVG_STEPS) - 1       # 0, 1 and k / (k + 1) for k = 1 .. 6


def test_resume_from_step_11_is_bit_equal_shadows_included():
    from avmoe_amd.train import LRSchedule
    dev = torch.device("cuda:0")
    a = make_params(dev)
    b = clone_params(a)
    gs = grads(T, dev)
    s = swa_sched()
    kw = dict(weight_decay=WD, max_grad_norm=MAX_NORM, decoupled_weight_decay=True, skip_nonfinite=True)
    _, oa = make_opt(a, swa_start=N, swa_freq=FREQ, lr_schedule=s, **kw)
    for k in range(T):
        set_grads(a, gs[k]); oa.step()
    _, ob = make_opt(b, swa_start=N, swa_freq=FREQ, lr_schedule=s, **kw)
    for k in range(11):
        set_grads(b, gs[k]); ob.step()
    sd = ob.state_dict()
    buf = io.BytesIO()
    torch.save(sd, buf)
    buf.seek(0)
    sd2 = torch.load(buf)
    extra = sd2["flat_adam"]
    assert extra["swa_start"] == N and extra["swa_freq"] == FREQ and extra["applied_steps"] == 11 and "ema_decay" not in extra
    assert {k: extra["lr_schedule"][k] for k in ("swa_start", "swa_factor", "swa_anneal_steps", "swa_anneal")} == \
        dict(swa_start=6, swa_factor=0.25, swa_anneal_steps=5, swa_anneal="cos")
    assert LRSchedule(**extra["lr_schedule"]) == s
    for e, p, view in zip(extra["ema"], ob.params, ob.ema_params):
        assert e.device.type == "cpu" and e.shape == p.shape and torch.equal(e, view.cpu())
    for g in sd2["param_groups"]:                           # "lr" is the rate of the next step, through the new factor
        assert g["lr"] == g["initial_lr"] * s.factor(11) and f32(s.factor(11)) == 0.25
    # a fresh reducer + optimizer over the parameters as the interrupted run left them, built with OTHER constants: the saved ones win
    _, oc = make_opt(b, swa_start=2, swa_freq=1, lr_schedule=lr_sched(), **kw)
    oc.load_state_dict(sd2)
    assert (oc.swa_start, oc.swa_freq) == (N, FREQ) and oc.lr_schedule == s and oc.t == 11 and int(oc.applied_steps.item()) == 11
    assert float(oc.last_ema_decay.item()) == swa_at(11) and float(oc.last_lr_factor.item()) == f32(s.factor(10))
    for k in range(11, T):
        set_grads(b, gs[k]); oc.step()
    assert_flats_equal(flats(oa), flats(oc), "resumed run")
    assert int(oc.applied_steps.item()) == T
    for field in ("ema_decay", "lr_factor", "total_norm", "clip_coef", "bc1", "bc2_sqrt"):
        assert torch.equal(bits(oa.state_block[field]), bits(oc.state_block[field])), field
    # torch loads it
    topt = torch.optim.AdamW(ob.torch_param_groups(), lr=LR, weight_decay=WD)
    topt.load_state_dict(sd2)
    assert all(float(st["step"]) == 11.0 for st in topt.state.values())
    # a dict without the averaging keys loads as it did: the averages start again from the current parameters
    bare = copy.deepcopy(sd2)
    for key in ("ema", "swa_start", "swa_freq"):
        del bare["flat_adam"][key]
    _, od = make_opt(clone_params(b), swa_start=N, swa_freq=FREQ, lr_schedule=s, **kw)
    with torch.no_grad():
        for e in od.ema_params:
            e.add_(1.0)
    od.load_state_dict(bare)
    assert all(torch.equal(bits(e), bits(p.data)) for e, p in zip(od.ema_params, od.params))
    assert (od.swa_start, od.swa_freq) == (N, FREQ) and int(od.applied_steps.item()) == 11
    # a dict saved with the uniform average does not load into an optimizer that keeps none, or the exponential one
    for other in (dict(), dict(ema_decay=0.9)):
        _, oe = make_opt(clone_params(b), lr_schedule=s, **other, **kw)
        with pytest.raises(ValueError, match="swa_start"):
            oe.load_state_dict(sd2)
    bad = copy.deepcopy(sd2)
    bad["flat_adam"]["ema"][3] = torch.zeros(2, 3)
    with pytest.raises(ValueError, match="parameter index 3"):
        od.load_state_dict(bad)


@pytest.mark.parametrize("kind", ["cos", "linear"])
def test_device_factor_follows_the_swa_learning_rate(kind):
    """N' = 6, A = 5 behind a warm-up and a cosine decay: after step number n (n = 0 first) the state block holds f(n) to 1 fp32 ulp"""
    dev = torch.device("cuda:0")
    a = make_params(dev)
    gs = grads(T, dev)
    s = swa_sched(kind)
    _, opt = make_opt(a, lr_schedule=s, max_grad_norm=MAX_NORM)
    worst, exact = 0, 0
    for n in range(T):
        set_grads(a, gs[n]); opt.step()
        got, want = float(opt.last_lr_factor.item()), f32(s.factor(n))
        d = ulps(got, want)
        worst, exact = max(worst, d), exact + (d == 0)
        assert d <= 1, (kind, n, got, want)
    print(f"swa lr, {kind}: {T} steps, worst distance {worst} ulp, {exact} bit-equal; last factor {got!r}")
    assert got == s.swa_factor == 0.25                       # the plateau from step N' + A on
    assert f32(s.factor(6)) == f32(lr_sched().factor(6)) and f32(s.factor(8)) != f32(lr_sched().factor(8))       # annealing starts AT base(N')
    assert opt.last_lr_factor.dtype == torch.float32 and opt.last_lr_factor.is_cuda


def test_a_swa_factor_of_one_from_step_zero_is_the_unscheduled_step():
    """swa_factor = 1 with no base decay and N' = 0 is the factor 1 on every step: bit-equal to the step without a schedule.  Here the
    schedule is the SWA part alone, and the uniform average is off: each half of avmoe_opt_swa works without the other."""
    from avmoe_amd import _capi_moe as cm
    from avmoe_amd.train import LRSchedule
    dev = torch.device("cuda:0")
    a = make_params(dev)
    b = clone_params(a)
    gs = grads(T, dev)
    kw = dict(weight_decay=WD, max_grad_norm=MAX_NORM, decoupled_weight_decay=True)
    _, oa = make_opt(a, lr_schedule=LRSchedule(swa_start=0, swa_factor=1.0, swa_anneal_steps=4), **kw)
    _, ob = make_opt(b, **kw)
    assert oa._flags == ob._flags | cm.OPT_LR_SCHEDULE | cm.OPT_SWA_LR
    for k in range(8):
        set_grads(a, gs[k]); oa.step()
        set_grads(b, gs[k]); ob.step()
        assert float(oa.last_lr_factor.item()) == 1.0
    assert_flats_equal(flats(oa, "pmv"), flats(ob, "pmv"), "factor 1")
    assert float(oa.state_block["clip_coef"].item()) < 1.0 and int(bits(oa.state_block["ema_decay"]).item()) == 0


def test_buffer_shadows_are_the_mean_of_the_buffers_snapshots():
    """ema_buffers under the uniform average: the buffers are rewritten before every step, as a forward pass does, and their shadows are
    the fp64 mean of what they held at the averaging steps within the bound of the module docstring (A = max|b|).  One buffer is a view
    that is only 4-byte aligned, with guard elements either side."""
    from tests.test_flat_adam_ema_buffers_gpu import BUF_SIZES, UNALIGNED, Buffers
    dev = torch.device("cuda:0")
    a, gs, bufs = make_params(dev), grads(T, dev), Buffers(dev)
    assert bufs.tensors[BUF_SIZES.index(UNALIGNED)].data_ptr() % 16 == 4
    g = torch.Generator().manual_seed(300)
    vals = [[0.5 + 2.0 * torch.randn(n, generator=g) for n in BUF_SIZES] for _ in range(T)]
    _, opt = make_opt(a, weight_decay=WD, max_grad_norm=MAX_NORM, swa_start=N, swa_freq=FREQ, ema_buffers=bufs.pairs)
    guards = bufs.guards()
    A = max(float(v.abs().max()) for stepvals in vals for v in stepvals)
    bound = 6 * T * U * A
    kept, worst = [], 0.0
    for k in range(T):
        bufs.write([v.to(dev) for v in vals[k]])
        set_grads(a, gs[k]); opt.step()
        n = k + 1
        if n in AVG_STEPS:
            kept.append(vals[k])
        for i, e in enumerate(opt.ema_buffers):
            if n < N:
                assert torch.equal(e.cpu().reshape(-1), vals[k][i]), (n, i)
                continue
            mean = torch.stack([v[i].double() for v in kept]).mean(0)
            err = float((e.double().cpu().reshape(-1) - mean).abs().max())
            worst = max(worst, err)
            assert err <= bound, (n, BUF_SIZES[i], err, bound)
    print(f"buffer shadows over {len(kept)} of {T} steps: |shadow - fp64 mean| max {worst:.3e}, bound {bound:.3e} (A = {A:.4f})")
    assert len(kept) == 7 and worst > 0.0
    assert torch.equal(guards, bufs.guards()) and int(bufs.counter.item()) == 41
    for t, v in zip(bufs.tensors, vals[-1]):                 # the buffers themselves are only read
        assert torch.equal(t.cpu().reshape(-1), v)


# ---------------------------------------------------------------------------------------------------------------------
class SiteA(torch.nn.Module):
    """one adapter site of the register-resident BatchNorm shape (128 channels in 2 groups, bottleneck 64, 32 latent tokens, one
    cross-modal and one unimodal expert) under the reference's checkpoint key"""

    def __init__(self):
        super().__init__()
        from oracle import avmoe_oracle as O
        from tests.test_adapters_api import build_module
        cfg = O.AdapterConfig(Cx=128, Nx=150, Cy=64, Ny=50, reduction=2, groups=2, K=32, E_m=1, E_s=1)
        self.audio_adapter_blocks_p1 = torch.nn.ModuleList([build_module("ave", cfg)])


def _site_model(seed, dev=None):
    torch.manual_seed(seed)
    model = SiteA()
    with torch.no_grad():                                    # the reference's zero gates make the output 0 whatever the statistics are
        for k, p in model.named_parameters():
            if k.endswith(("gate", "gate_av")):
                p.fill_(0.4)
    return model if dev is None else model.to(dev).train()


def _site_forward(model, batch):
    return model.audio_adapter_blocks_p1[0](*batch)


def test_end_to_end_swa_then_bn_reestimation_then_the_averaged_checkpoint():
    """8 training steps of a site with swa_start=3 and the BatchNorm statistics averaged along, torch's update_bn for the averaged
    weights (reestimate_bn), and the checkpoint: a fresh site loaded from adapter_state_dict(model, ema=opt) computes, in eval mode, the
    bits the model computes inside ema_weights()"""
    from avmoe_amd.dp import AdapterGradReducer
    from avmoe_amd.train import FlatAdam, adapter_state_dict, load_adapters, reestimate_bn
    dev = torch.device("cuda:0")
    model = _site_model(0, dev)
    site = model.audio_adapter_blocks_p1[0]
    red = AdapterGradReducer(list(site.parameters()), sites=[site])
    opt = FlatAdam(red, lr=LR, weight_decay=WD, max_grad_norm=1.0, swa_start=3, ema_buffers=model)
    g = torch.Generator().manual_seed(9)
    draw = lambda *shape: torch.randn(*shape, generator=g).to(dev)
    for _ in range(8):
        X, Y, G = draw(4, 128, 150, 1), draw(4, 64, 50, 1), draw(4, 128, 150, 1)
        red.begin(sync=True)
        site(X, Y)[0].backward(G)
        red.finish()
        opt.step()
        red.zero_grad()
    assert int(opt.applied_steps.item()) == 8 and float(opt.last_ema_decay.item()) == f32(5.0 / 6.0)
    assert FlatAdam.swa_n_averaged_at(8, 3) == 6
    assert any(not torch.equal(e, p.data) for e, p in zip(opt.ema_params, opt.params))
    batches = [(draw(4, 128, 150, 1), draw(4, 64, 50, 1)) for _ in range(3)]
    raw = {k: v.detach().clone() for k, v in model.state_dict().items()}
    before = [e.clone() for e in opt.ema_buffers]
    assert reestimate_bn(model, batches, _site_forward, ema=opt) == 3
    for k, v in model.state_dict().items():                  # the raw model is what it was
        assert torch.equal(v, raw[k]), k
    assert all(not torch.equal(e, old) for e, old in zip(opt.ema_buffers, before))
    sd = adapter_state_dict(model, ema=opt)
    fresh = _site_model(1)
    res = load_adapters(fresh, sd)
    assert not res.unexpected_keys and not [k for k in res.missing_keys if "adapter" in k]
    fresh = fresh.to(dev).eval()
    model.eval()
    with torch.no_grad():
        with opt.ema_weights():
            out_avg = _site_forward(model, batches[0])[0].clone()
        out_raw = _site_forward(model, batches[0])[0]
        out_fresh = _site_forward(fresh, batches[0])[0]
    assert torch.equal(bits(out_avg), bits(out_fresh)) and float(out_avg.abs().max()) > 0
    assert not torch.equal(out_avg, out_raw)                 # and the averaged model is not the raw one
