"""Host side of FlatAdam's per-step learning-rate schedule (include/avmoe.h: avmoe_opt_schedule, avmoe_opt_grad_norm_sched;
avmoe_amd.train.LRSchedule): the closed form against torch's own schedulers on a CPU optimizer, the argument checks of both layers
(they precede any launch, so host pointers are enough and no GPU is needed), and the layouts the binding relies on.

Tolerance of the closed form: 1e-9 relative.  torch's chainable forms are recursive in fp64 (each step multiplies the previous rate by a
ratio); over n <= 1e4 steps their drift is bounded by n * 2^-52 ~ 2e-12, and the bar leaves two orders of magnitude over that.

Two places where torch is not the reference.  (1) Beyond total_steps torch's CosineAnnealingLR swings back up (it is periodic); the
schedule here is defined with c = min(u, D) and stays at min_factor, which is asserted directly.  (2) The device holds warmup_start,
min_factor and gamma as fp32, LRSchedule rounds them at construction, and the torch schedulers are built from the schedule's own
(rounded) fields: the comparison is about the form, not about 0.1 against float32(0.1)."""
import ctypes as C
import math
import warnings

import pytest
import torch

from avmoe_amd import _capi
from avmoe_amd import _capi_moe as cm
from avmoe_amd.train import LRSchedule

BAD_ARG = -1
LR0 = 3e-3
REL = 1e-9


def torch_lrs(make_sched, n_steps):
    """the learning rate torch uses at step 0, 1, ..., n_steps - 1 (optimizer.step() then scheduler.step(), as in a training loop)"""
    p = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.SGD([p], lr=LR0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                     # SequentialLR's own use of the deprecated epoch argument
        sched = make_sched(opt)
        out = []
        for _ in range(n_steps):
            out.append(opt.param_groups[0]["lr"])
            opt.step()
            sched.step()
    return out


def with_warmup(sched, decay):
    """the torch chain of a schedule: LinearLR warm-up (none for W = 0), then `decay(optimizer)`"""
    from torch.optim.lr_scheduler import LinearLR, SequentialLR
    W = sched.warmup_steps
    if W == 0:
        return decay
    return lambda o: SequentialLR(o, [LinearLR(o, start_factor=sched.warmup_start, end_factor=1.0, total_iters=W), decay(o)], milestones=[W])


def assert_close(sched, want, upto, what):
    worst = 0.0
    for n in range(upto):
        got = LR0 * sched.factor(n)
        err = abs(got - want[n]) / max(abs(want[n]), 1e-300) if want[n] != got else 0.0
        worst = max(worst, err)
        assert err <= REL, (what, n, got, want[n])
    print(f"{what}: worst relative difference to torch over {upto} steps {worst:.3e}")


COSINE_CASES = [(0, 1000, 1.0, 0.0), (100, 1000, 0.125, 0.1), (500, 4000, 0.01, 0.05), (1, 2, 0.5, 0.5), (300, 3000, 0.1, 0.0), (1000, 10000, 0.25, 0.001)]


@pytest.mark.parametrize("W,total,s0,fmin", COSINE_CASES)
def test_warmup_cosine_matches_sequential_linear_cosine(W, total, s0, fmin):
    from torch.optim.lr_scheduler import CosineAnnealingLR
    s = LRSchedule(warmup_steps=W, warmup_start=s0, decay_kind="cosine", total_steps=total, min_factor=fmin)
    D = total - W
    want = torch_lrs(with_warmup(s, lambda o: CosineAnnealingLR(o, T_max=D, eta_min=s.min_factor * LR0)), total + 1)
    assert_close(s, want, total + 1, f"cosine W={W} total={total}")
    assert s.factor(0) == (s.warmup_start if W else 1.0) and s.factor(W) == 1.0
    for n in (total, total + 1, total + D, 3 * total + 7):   # the plateau: torch's cosine is periodic, this one is not
        assert s.factor(n) == s.min_factor, n


@pytest.mark.parametrize("W,total,s0,fmin", [(0, 1000, 1.0, 0.0), (100, 1000, 0.125, 0.1), (500, 4000, 0.01, 0.05), (1, 2, 0.5, 0.5), (200, 2500, 0.3, 0.25)])
def test_warmup_linear_matches_linear_lr(W, total, s0, fmin):
    from torch.optim.lr_scheduler import LinearLR
    s = LRSchedule(warmup_steps=W, warmup_start=s0, decay_kind="linear", total_steps=total, min_factor=fmin)
    D = total - W
    n_steps = total + 500                                   # LinearLR holds its end factor, like the schedule
    want = torch_lrs(with_warmup(s, lambda o: LinearLR(o, start_factor=1.0, end_factor=s.min_factor, total_iters=D)), n_steps)
    assert_close(s, want, n_steps, f"linear W={W} total={total}")
    assert s.factor(total) == s.min_factor and s.factor(total + 10 ** 6) == s.min_factor


@pytest.mark.parametrize("W,step_size,gamma,s0", [(0, 30, 0.1, 1.0), (50, 100, 0.5, 0.2), (7, 1, 0.999, 0.5), (250, 1000, 0.3, 0.0625)])
def test_warmup_step_matches_step_lr(W, step_size, gamma, s0):
    from torch.optim.lr_scheduler import StepLR
    s = LRSchedule(warmup_steps=W, warmup_start=s0, decay_kind="step", step_size=step_size, gamma=gamma)
    n_steps = W + min(6 * step_size, 4000)
    want = torch_lrs(with_warmup(s, lambda o: StepLR(o, step_size=step_size, gamma=s.gamma)), n_steps)
    assert_close(s, want, n_steps, f"step W={W} step_size={step_size}")


def test_no_decay_is_one_after_the_warmup_and_the_constants_are_fp32():
    s = LRSchedule(warmup_steps=4, warmup_start=0.1)
    assert [s.factor(n) for n in (4, 5, 10 ** 9)] == [1.0, 1.0, 1.0]
    assert LRSchedule().factor(0) == 1.0 and LRSchedule().factor(12345) == 1.0
    import numpy as np
    assert s.warmup_start == float(np.float32(0.1)) and s.factor(0) == s.warmup_start
    t = LRSchedule(decay_kind="step", step_size=2, gamma=0.1, min_factor=0.3)
    assert t.gamma == float(np.float32(0.1)) and t.min_factor == float(np.float32(0.3))
    assert LRSchedule(**{**t.__dict__}) == t                # rounding twice changes nothing: the saved fields rebuild the schedule
    assert LRSchedule(decay_kind=1, total_steps=5).decay_kind == "cosine"        # AVMOE_SCHED_* numbers are accepted too


BAD = [dict(warmup_steps=-1), dict(total_steps=-1), dict(step_size=-1),
       dict(decay_kind="cosine", warmup_steps=10, total_steps=10), dict(decay_kind="linear", warmup_steps=10, total_steps=9),
       dict(decay_kind="cosine"), dict(decay_kind="linear", warmup_steps=0, total_steps=0),
       dict(warmup_start=-0.1), dict(warmup_start=1.5), dict(warmup_start=float("nan")),
       dict(min_factor=-0.1), dict(min_factor=1.01), dict(min_factor=float("nan")),
       dict(decay_kind="step", step_size=0), dict(decay_kind="step"),
       dict(gamma=0.0), dict(gamma=-0.5), dict(gamma=1.5), dict(gamma=float("nan")), dict(decay_kind="step", step_size=3, gamma=0.0)]


@pytest.mark.parametrize("kw", BAD, ids=[",".join(f"{k}={v}" for k, v in kw.items()) for kw in BAD])
def test_bad_schedules_raise_in_python(kw):
    with pytest.raises(ValueError):
        LRSchedule(**kw)


def test_unknown_decay_kind_and_wrong_type_raise():
    with pytest.raises(ValueError):
        LRSchedule(decay_kind="exponential")
    with pytest.raises(ValueError):
        LRSchedule(decay_kind=9)
    with pytest.raises(ValueError):
        LRSchedule(warmup_steps=2.5)
    from avmoe_amd.dp import AdapterGradReducer
    from avmoe_amd.train import FlatAdam
    red = AdapterGradReducer([torch.nn.Parameter(torch.zeros(7))])
    with pytest.raises(TypeError):
        FlatAdam(red, lr_schedule=dict(warmup_steps=3))
    with pytest.raises(_capi.AvmoeError):                    # the schedule selects the device path, which has no CPU fallback
        FlatAdam(red, lr_schedule=LRSchedule(warmup_steps=3))


# ---- the C entry point -------------------------------------------------------------------------------------------------
def _buf(nbytes):
    raw = C.create_string_buffer(nbytes + 64)
    return raw, (C.addressof(raw) + 63) & ~63


def _err():
    msg = _capi.lib().avmoe_last_error()
    return msg.decode() if msg else ""


def _c_sched(**kw):
    f = dict(warmup_steps=0, warmup_start=0.0, decay_kind=0, total_steps=0, min_factor=0.0, gamma=1.0, step_size=0)
    f.update(kw)
    if isinstance(f["decay_kind"], str):
        f["decay_kind"] = cm.SCHED_KINDS[f["decay_kind"]]
    return cm.OptSchedule(**f)


def test_header_declares_and_library_exports_the_schedule_entry_point():
    L = _capi.lib()
    assert "avmoe_opt_grad_norm_sched" in _capi.exported_symbols() and hasattr(L, "avmoe_opt_grad_norm_sched")
    assert L.avmoe_abi_version() == 11
    assert cm.OPT_LR_SCHEDULE == 8 and cm.SCHED_KINDS == {"none": 0, "cosine": 1, "linear": 2, "step": 3}
    header = open(_capi.HEADER_PATH).read()
    assert "AVMOE_OPT_LR_SCHEDULE = 8" in header
    assert "AVMOE_SCHED_NONE = 0, AVMOE_SCHED_COSINE = 1, AVMOE_SCHED_LINEAR = 2, AVMOE_SCHED_STEP = 3" in header


def test_state_block_is_still_64_bytes_and_has_lr_factor():
    assert cm.OPT_STATE_BYTES == 64
    assert cm.OPT_STATE_FIELDS["lr_factor"] == (36, "float32")           # in place of reserved[0], right after `skip`
    assert cm.OPT_STATE_FIELDS["skip"] == (32, "int32")
    spans = sorted((o, o + (8 if dt == "int64" else 4)) for o, dt in cm.OPT_STATE_FIELDS.values())
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])) and spans[-1][1] <= 64      # no two fields overlap, all inside the block
    lay = cm.OptLayout()
    raw, base = _buf(4096)
    r = (cm.OptRange * 1)()
    r[0].param, r[0].grad, r[0].exp_avg, r[0].exp_avg_sq, r[0].n, r[0].lr = base, base + 64, base + 128, base + 192, 4, 1e-3
    assert _capi.lib().avmoe_opt_workspace_bytes(r, 1, C.byref(lay)) > 0 and lay.state_bytes == 64
    assert C.sizeof(cm.OptSchedule) == 40 and C.sizeof(cm.OptRange) == 48
    assert [(n, getattr(cm.OptSchedule, n).offset) for n, _ in cm.OptSchedule._fields_] == [
        ("warmup_steps", 0), ("warmup_start", 8), ("decay_kind", 12), ("total_steps", 16), ("min_factor", 24), ("gamma", 28), ("step_size", 32)]
    s = LRSchedule(warmup_steps=5, warmup_start=0.25, decay_kind="step", total_steps=9, min_factor=0.5, step_size=3, gamma=0.75).c_struct()
    assert (s.warmup_steps, s.warmup_start, s.decay_kind, s.total_steps, s.min_factor, s.gamma, s.step_size) == (5, 0.25, 3, 9, 0.5, 0.75, 3)


C_BAD = [dict(warmup_steps=-1), dict(total_steps=-1), dict(step_size=-1),
         dict(decay_kind="cosine", warmup_steps=10, total_steps=10), dict(decay_kind="linear", warmup_steps=10, total_steps=9),
         dict(warmup_start=-0.1), dict(warmup_start=1.5), dict(warmup_start=float("nan")),
         dict(min_factor=-0.1), dict(min_factor=1.01), dict(min_factor=float("nan")),
         dict(decay_kind="step", step_size=0),
         dict(gamma=0.0), dict(gamma=-0.5), dict(gamma=1.5), dict(gamma=float("nan")),
         dict(decay_kind=7)]


def test_schedule_validation_precedes_any_launch():
    """host pointers everywhere: a call that got as far as a launch would fault or fail, these all return an argument error first"""
    L = _capi.lib()
    raw, base = _buf(4096)
    table, partials, state = base, base + 1024, base + 2048
    flags = cm.OPT_CLIP | cm.OPT_LR_SCHEDULE

    def call(sched, flags=flags, state=state, b1=0.9):
        ref = None if sched is None else C.byref(sched)
        return L.avmoe_opt_grad_norm_sched(table, 2, 2, partials, state, 1.0, 1.0, flags, b1, 0.999, None, ref)

    for kw in C_BAD:
        assert call(_c_sched(**kw)) == BAD_ARG, kw
        assert _err(), kw
    assert call(None) == BAD_ARG and _err()                 # the flag without a schedule
    good = _c_sched(decay_kind="cosine", warmup_steps=3, total_steps=9, warmup_start=0.5)
    assert call(good, flags=flags | 64) == BAD_ARG and _err()            # the checks of avmoe_opt_grad_norm still apply
    assert call(good, state=None) == BAD_ARG and _err()
    assert call(good, b1=1.0) == BAD_ARG and _err()
    # avmoe_opt_grad_norm has no schedule argument: it refuses the flag; avmoe_opt_adam_step knows it (and fails on something else here)
    assert L.avmoe_opt_grad_norm(table, 2, 2, partials, state, 1.0, 1.0, flags, 0.9, 0.999, None) == BAD_ARG and "unknown flag" in _err()
    assert L.avmoe_opt_adam_step(table, 2, 2, state, 0.9, 0.999, -1.0, 1.0, flags, None) == BAD_ARG and "unknown flag" not in _err()
    assert L.avmoe_opt_adam_step(table, 2, 2, state, 0.9, 0.999, 1e-8, 1.0, flags | 16, None) == BAD_ARG and "unknown flag" in _err()


def test_factor_at_exactly_representable_points():
    """where every intermediate is exact in binary the closed form gives the exact value"""
    s = LRSchedule(warmup_steps=10, warmup_start=0.5, decay_kind="linear", total_steps=110, min_factor=0.0)
    assert s.factor(0) == 0.5 and s.factor(5) == 0.75 and s.factor(10) == 1.0 and s.factor(60) == 0.5 and s.factor(110) == 0.0
    assert math.isclose(s.factor(35), 0.75, rel_tol=1e-15)
