"""FlatAdam's per-step learning-rate schedule on the device (avmoe_amd.train.LRSchedule, include/avmoe.h: avmoe_opt_grad_norm_sched) on the
two-bucket model of tests/test_flat_adam_device_gpu.py: the factor the finalize kernel writes, the trajectory against torch's optimizer +
scheduler chain, the unscheduled path left as it was, skipped steps, graph capture and resume.

Tolerances.  Factor: 1 fp32 ulp of float32(LRSchedule.factor(n)) -- the kernel evaluates the same closed form in double from the same
fp32 constants and rounds once; the bound covers that rounding plus at most one double-ulp difference between the device's and the host's
cos / pow.  Adam arithmetic against torch: the bar of tests/test_flat_adam_device_gpu.py, 1e-6 * max|p| + 2e-3 * lr per parameter and step
with the parameters re-synchronised after each step, lr being the scheduled rate of that step.  Everything that is the same kernels on
the same bits is held to bit-equality."""
import copy
import io
import warnings

import numpy as np
import pytest
import torch

from tests.test_flat_adam_device_gpu import (LR, LR_X, WD, assert_flats_equal, bits, fixed_grads, flats, make_model, make_opt, set_grads,
                                             tol, ulps)

pytestmark = pytest.mark.gpu


def sched_of(kind, **kw):
    from avmoe_amd.train import LRSchedule
    return LRSchedule(decay_kind=kind, **kw)


def f32(x):
    return float(np.float32(x))


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,kw", [("cosine", dict(warmup_steps=40, warmup_start=0.1, total_steps=170, min_factor=0.05)),
                                     ("linear", dict(warmup_steps=25, warmup_start=0.0, total_steps=180, min_factor=0.0)),
                                     ("step", dict(warmup_steps=10, warmup_start=0.3, step_size=17, gamma=0.7)),
                                     ("none", dict(warmup_steps=150, warmup_start=0.01))])
def test_device_factor_is_within_one_ulp_of_the_closed_form(kind, kw):
    """200 steps across warm-up, decay and the plateau: after step number n (n = 0 first) the state block holds f(n)"""
    dev = torch.device("cuda:0")
    model = make_model(dev)
    s = sched_of(kind, **kw)
    _, opt = make_opt(model, lr_schedule=s, max_grad_norm=50.0)
    set_grads(model, fixed_grads(model, 1, dev)[0])
    worst, exact = 0, 0
    for n in range(200):
        opt.step()
        got, want = float(opt.last_lr_factor.item()), f32(s.factor(n))
        d = ulps(got, want)
        worst, exact = max(worst, d), exact + (d == 0)
        assert d <= 1, (kind, n, got, want)
    print(f"{kind}: 200 steps, worst distance {worst} ulp, {exact} bit-equal; last factor {got!r}")
    assert int(opt.applied_steps.item()) == 200 and opt.last_lr_factor.dtype == torch.float32 and opt.last_lr_factor.is_cuda
    if kind in ("cosine", "linear"):
        assert got == s.min_factor                           # the plateau is exact: cos(pi) = -1, c / D = 1


@pytest.mark.parametrize("decoupled", [False, True])
@pytest.mark.parametrize("clip", [False, True])
def test_scheduled_trajectory_matches_torch_optimizer_and_scheduler_chain(clip, decoupled):
    """torch.optim.Adam / AdamW stepped by SequentialLR(LinearLR, CosineAnnealingLR).  CosineAnnealingLR takes ONE eta_min for all groups
    and the two groups here need min_factor times their own rate, so each group has its own torch optimizer and chain; the clipping is one
    clip_grad_norm_ over all parameters, as in a training loop."""
    from torch.optim.lr_scheduler import CosineAnnealingLR, LinearLR, SequentialLR
    dev = torch.device("cuda:0")
    ref = make_model(dev)
    fused = copy.deepcopy(ref)
    W, total = 3, 8
    s = sched_of("cosine", warmup_steps=W, warmup_start=0.25, total_steps=total, min_factor=0.1)
    n_steps = total + 1                                     # n = 0 .. total; beyond it torch's cosine is periodic and no reference
    grads = fixed_grads(ref, n_steps, dev)
    max_norm = 20.0                                         # random gradients over 31 632 elements: norm about 178, so every step clips
    cls = torch.optim.AdamW if decoupled else torch.optim.Adam
    topts, chains = [], []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                     # SequentialLR's own use of the deprecated epoch argument
        for params, lr0 in ((list(ref.site.parameters()), LR), (list(ref.extra), LR_X)):
            o = cls(params, lr=lr0, weight_decay=WD)
            topts.append(o)
            chains.append(SequentialLR(o, [LinearLR(o, start_factor=s.warmup_start, end_factor=1.0, total_iters=W),
                                           CosineAnnealingLR(o, T_max=total - W, eta_min=s.min_factor * lr0)], milestones=[W]))
    kw = dict(max_grad_norm=max_norm) if clip else {}
    red, fopt = make_opt(fused, weight_decay=WD, decoupled_weight_decay=decoupled, lr_schedule=s, **kw)
    for n in range(n_steps):
        f = s.factor(n)
        for o, lr0 in zip(topts, (LR, LR_X)):               # the chain does walk lr0 * f(n) (1e-9: tests/test_flat_adam_schedule_api.py)
            assert abs(o.param_groups[0]["lr"] - lr0 * f) <= 1e-9 * lr0 * f, (n, o.param_groups[0]["lr"], lr0 * f)
        for p, gr in zip(ref.all_params(), grads[n]):
            p.grad = gr.clone()
        set_grads(fused, grads[n])
        if clip:
            total_norm = torch.nn.utils.clip_grad_norm_(ref.all_params(), max_norm)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            for o, c in zip(topts, chains):
                o.step(); c.step()
        fopt.step()
        if clip:
            got = float(fopt.last_grad_norm.item())
            assert abs(got - float(total_norm)) <= 1e-5 * float(total_norm) and float(fopt.state_block["clip_coef"].item()) < 1.0
        assert ulps(float(fopt.last_lr_factor.item()), f32(f)) <= 1, n
        with torch.no_grad():
            worst = 0.0
            for (k, p), q in zip(list(ref.named_parameters()), [q for _, q in fused.named_parameters()]):
                lr_now = (LR_X if any(p is e for e in ref.extra) else LR) * f
                err = float((p - q).abs().max())
                worst = max(worst, err / tol(p, lr_now))
                assert err <= tol(p, lr_now), (n, k, err, tol(p, lr_now))
                q.copy_(p)
        print(f"step n={n} (clip={clip}, decoupled={decoupled}): factor {f:.6f}, worst error / bound = {worst:.3f}")
    assert int(fopt.applied_steps.item()) == n_steps


# ---------------------------------------------------------------------------------------------------------------------
def raw_step(opt, entry):
    """one step of `opt` through the C entry points themselves, without the schedule flag"""
    from avmoe_amd import _capi as capi
    L = capi.lib()
    stream = torch.cuda.current_stream().cuda_stream
    n, flags = len(opt.params), opt._flags
    scale = opt.grad_scale * float(getattr(opt.reducer, "grad_scale", 1.0))
    args = (opt._table_ptr, n, opt._n_blocks, opt._partials_ptr, opt._state_ptr, scale, opt.max_grad_norm or 0.0, flags, opt.betas[0], opt.betas[1],
            stream)
    if entry == "grad_norm":
        capi.check(L.avmoe_opt_grad_norm(*args), "avmoe_opt_grad_norm")
    else:                                                   # the new entry point, flag off: `sched` is not read
        capi.check(L.avmoe_opt_grad_norm_sched(*args, None), "avmoe_opt_grad_norm_sched")
    capi.check(L.avmoe_opt_adam_step(opt._table_ptr, n, opt._n_blocks, opt._state_ptr, opt.betas[0], opt.betas[1], opt.eps, scale, flags, stream),
               "avmoe_opt_adam_step")
    opt.t += 1


def test_without_a_schedule_nothing_changes_and_a_schedule_of_one_is_bit_equal_to_none():
    from avmoe_amd import _capi as capi
    from avmoe_amd import _capi_moe as cm
    dev = torch.device("cuda:0")
    models = [make_model(dev)]
    models += [copy.deepcopy(models[0]) for _ in range(3)]
    grads = fixed_grads(models[0], 5, dev)
    kw = dict(weight_decay=WD, max_grad_norm=20.0, decoupled_weight_decay=True, skip_nonfinite=True, step_size=2, gamma=0.5)
    opts = [make_opt(m, **kw)[1] for m in models[:3]]
    opts.append(make_opt(models[3], lr_schedule=sched_of("none", warmup_steps=0), **kw)[1])
    assert [o._flags & cm.OPT_LR_SCHEDULE for o in opts] == [0, 0, 0, cm.OPT_LR_SCHEDULE]
    for k in range(5):
        for m in models:
            set_grads(m, grads[k])
        opts[0].step()                                      # FlatAdam without lr_schedule
        raw_step(opts[1], "grad_norm")                      # the entry points it used before the schedule existed
        raw_step(opts[2], "grad_norm_sched")                # the new one with the flag off
        opts[3].step()                                      # decay_kind none, no warm-up: f = 1
        for o in opts:
            o.epoch_end()
        for i in (1, 2, 3):
            assert_flats_equal(flats(opts[0]), flats(opts[i]), f"step {k}, variant {i}")
            assert torch.equal(bits(opts[0].last_grad_norm), bits(opts[i].last_grad_norm))
    for o in opts[:3]:                                      # the word that was reserved[0] is never written without the flag
        assert int(o.state_block["lr_factor"].view(torch.int32).item()) == 0
        with pytest.raises(capi.AvmoeError):
            o.last_lr_factor
    assert float(opts[3].last_lr_factor.item()) == 1.0 and float(opts[0].state_block["clip_coef"].item()) < 1.0
    assert all(int(o.applied_steps.item()) == 5 for o in opts)


def test_skipped_step_holds_the_schedule_back():
    dev = torch.device("cuda:0")
    a = make_model(dev)
    b = copy.deepcopy(a)
    grads = fixed_grads(a, 4, dev)
    s = sched_of("linear", warmup_steps=2, warmup_start=0.2, total_steps=6, min_factor=0.1)
    kw = dict(weight_decay=WD, skip_nonfinite=True, max_grad_norm=20.0, lr_schedule=s)
    _, oa = make_opt(a, **kw)
    _, ob = make_opt(b, **kw)                                # b never sees the poisoned gradient
    for k in (0, 1):
        set_grads(a, grads[k]); oa.step()
        set_grads(b, grads[k]); ob.step()
    assert ulps(float(oa.last_lr_factor.item()), f32(s.factor(1))) <= 1
    set_grads(a, grads[2])
    victim = a.all_params()[3]
    victim.grad.view(-1)[victim.numel() // 2] = float("inf")
    before, f_before = flats(oa), bits(oa.last_lr_factor)
    oa.step()
    assert_flats_equal(before, flats(oa), "skipped step")
    assert torch.equal(f_before, bits(oa.last_lr_factor))    # the factor stays what the last applied step used
    assert int(oa.skipped_steps.item()) == 1 and int(oa.applied_steps.item()) == 2 and oa.t == 3
    set_grads(a, grads[3]); oa.step()                        # applied step number 2 for both: f(2), not f(3)
    set_grads(b, grads[3]); ob.step()
    assert s.factor(2) != s.factor(3)
    assert ulps(float(oa.last_lr_factor.item()), f32(s.factor(2))) <= 1
    assert torch.equal(bits(oa.last_lr_factor), bits(ob.last_lr_factor))
    assert_flats_equal(flats(oa), flats(ob), "the step after the skip")
    assert int(oa.skipped_steps.item()) == 1 and int(oa.applied_steps.item()) == 3 and int(ob.skipped_steps.item()) == 0


# ---------------------------------------------------------------------------------------------------------------------
def test_captured_step_follows_the_schedule_on_replay():
    dev = torch.device("cuda:0")
    a = make_model(dev)
    b = copy.deepcopy(a)
    W, total, n_steps = 3, 7, 9                             # replays cross warm-up -> decay (n = 3) and decay -> plateau (n = 7)
    s = sched_of("cosine", warmup_steps=W, warmup_start=0.1, total_steps=total, min_factor=0.05)
    grads = fixed_grads(a, n_steps, dev)
    kw = dict(weight_decay=WD, max_grad_norm=20.0, skip_nonfinite=True, lr_schedule=s)
    _, oa = make_opt(a, **kw)
    _, ob = make_opt(b, **kw)
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    eager = []
    with torch.cuda.stream(st):                              # the eager run (it also loads the kernels before the capture)
        for k in range(n_steps):
            set_grads(a, grads[k]); oa.step()
            eager.append(bits(oa.last_lr_factor))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=st):
        ob.step()
    torch.cuda.synchronize()
    assert int(ob.applied_steps.item()) == 0                 # capturing runs nothing
    for k in range(n_steps):
        set_grads(b, grads[k])
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(bits(ob.last_lr_factor), eager[k]), k
        assert ulps(float(ob.last_lr_factor.item()), f32(s.factor(k))) <= 1, k
    assert int(ob.applied_steps.item()) == n_steps and int(ob.skipped_steps.item()) == 0
    assert_flats_equal(flats(oa), flats(ob), "graph replay")
    assert torch.equal(bits(oa.last_grad_norm), bits(ob.last_grad_norm))
    assert len({int(e.item()) for e in eager}) >= total      # and the factor did move from replay to replay


def test_resume_continues_the_schedule_bit_for_bit_and_torch_loads_the_dict():
    from avmoe_amd.train import LRSchedule
    dev = torch.device("cuda:0")
    a = make_model(dev)
    b = copy.deepcopy(a)
    s = sched_of("cosine", warmup_steps=2, warmup_start=0.1, total_steps=7, min_factor=0.05)
    kw = dict(weight_decay=WD, step_size=2, gamma=0.5, max_grad_norm=20.0, decoupled_weight_decay=True, skip_nonfinite=True)
    grads = fixed_grads(a, 6, dev)
    _, oa = make_opt(a, lr_schedule=s, **kw)
    for k in range(6):
        set_grads(a, grads[k]); oa.step(); oa.epoch_end()
    _, ob = make_opt(b, lr_schedule=s, **kw)
    for k in range(3):
        set_grads(b, grads[k]); ob.step(); ob.epoch_end()
    sd = ob.state_dict()
    buf = io.BytesIO()
    torch.save(sd, buf)
    buf.seek(0)
    sd2 = torch.load(buf)
    assert sd2["flat_adam"] == sd["flat_adam"] and sd2["param_groups"] == sd["param_groups"]
    assert LRSchedule(**sd2["flat_adam"]["lr_schedule"]) == s and sd2["flat_adam"]["applied_steps"] == 3 and sd2["flat_adam"]["epoch"] == 3
    lr0s = [lr0 for lr0, _ in ob._groups()]
    assert sorted(lr0s) == sorted((LR, LR_X)) and ob.decay == 0.5
    for g_, lr0 in zip(sd2["param_groups"], lr0s):           # the rate of the NEXT step, and the base rate a torch scheduler keeps
        assert g_["initial_lr"] == lr0 and g_["lr"] == lr0 * 0.5 * s.factor(3)
    # a fresh optimizer over the parameters as the interrupted run left them, built with ANOTHER schedule: the saved one replaces it
    _, oc = make_opt(b, lr_schedule=LRSchedule(warmup_steps=100, warmup_start=0.5), **kw)
    oc.load_state_dict(sd2)
    assert oc.lr_schedule == s and oc.t == 3 and oc.epoch == 3 and int(oc.applied_steps.item()) == 3
    assert float(oc.last_lr_factor.item()) == f32(s.factor(2))
    for k in range(3, 6):
        set_grads(b, grads[k]); oc.step(); oc.epoch_end()
    assert_flats_equal(flats(oa), flats(oc), "resumed run")
    assert int(oc.applied_steps.item()) == 6 and torch.equal(bits(oa.last_lr_factor), bits(oc.last_lr_factor))
    assert torch.equal(bits(oa.last_grad_norm), bits(oc.last_grad_norm))
    # torch loads it: an AdamW over FlatAdam's groups takes the moments, the step count and the scheduled rate
    topt = torch.optim.AdamW(ob.torch_param_groups(), lr=LR, weight_decay=WD)
    topt.load_state_dict(sd2)
    for g_, lr0 in zip(topt.param_groups, lr0s):
        assert g_["lr"] == lr0 * 0.5 * s.factor(3) and g_["initial_lr"] == lr0
    assert all(float(st["step"]) == 3.0 for st in topt.state.values()) and len(topt.state) == len(ob.params)
    # a dict without initial_lr (a torch optimizer that never had a scheduler): its lr is taken as the base rate, not divided by f
    bare = copy.deepcopy(sd2)
    for g_ in bare["param_groups"]:
        g_["lr"] = g_.pop("initial_lr")
    _, oe = make_opt(copy.deepcopy(b), lr_schedule=s, **kw)
    oe.load_state_dict(bare)
    assert [lr0 for lr0, _ in oe._groups()] == [lr0 / 0.5 for lr0 in lr0s] and oe.lr_schedule == s
    # and a plain-path optimizer cannot take a schedule over
    _, od = make_opt(copy.deepcopy(b))
    with pytest.raises(ValueError, match="lr_schedule"):
        od.load_state_dict(sd2)
