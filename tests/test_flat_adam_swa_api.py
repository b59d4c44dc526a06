"""Host side of stochastic weight averaging in FlatAdam (include/avmoe.h: avmoe_opt_swa, avmoe_opt_grad_norm_swa, AVMOE_OPT_SWA,
AVMOE_OPT_SWA_LR; avmoe_amd.train.FlatAdam(swa_start=..., swa_freq=...), LRSchedule(swa_start=..., ...)): the symbol and layouts the
binding relies on, the argument checks of both layers (they precede any launch, so host pointers and a NULL stream are enough and no GPU
is needed), the closed form of the uniform average's decay, and the closed form of the annealed learning rate against torch's own
LambdaLR -> SWALR chain.

Tolerance of the learning rate against torch: 1e-12 relative.  Both sides are a few double operations; torch recovers the rate it
anneals from by a division by (1 - alpha_prev) each step, which amplifies a rounding error by at most 1 / (1 - alpha_prev), about 160 at
20 annealing steps; the largest difference seen was 3.8e-16."""
import ctypes as C
import math
import warnings

import numpy as np
import pytest
import torch

from avmoe_amd import _capi
from avmoe_amd import _capi_moe as cm
from avmoe_amd.train import FlatAdam, LRSchedule

BAD_ARG = -1


def _buf(nbytes):
    raw = C.create_string_buffer(nbytes + 64)
    return raw, (C.addressof(raw) + 63) & ~63


def _err():
    msg = _capi.lib().avmoe_last_error()
    return msg.decode() if msg else ""


def f32(x):
    return float(np.float32(x))


def test_header_declares_and_library_exports_the_swa_entry_point():
    L = _capi.lib()
    assert "avmoe_opt_grad_norm_swa" in _capi.exported_symbols() and hasattr(L, "avmoe_opt_grad_norm_swa")
    assert L.avmoe_abi_version() == 11
    assert (cm.OPT_SWA, cm.OPT_SWA_LR) == (64, 128)
    header = open(_capi.HEADER_PATH).read()
    assert "AVMOE_OPT_SWA = 64, AVMOE_OPT_SWA_LR = 128" in header and "typedef struct avmoe_opt_swa" in header
    assert "AVMOE_SWA_ANNEAL_COS = 0, AVMOE_SWA_ANNEAL_LINEAR = 1" in header and cm.SWA_ANNEAL_KINDS == {"cos": 0, "linear": 1}
    # 32 bytes without padding; the header declares the fields in the binding's order
    assert C.sizeof(cm.OptSwa) == 32
    offs = [(n, getattr(cm.OptSwa, n).offset, getattr(cm.OptSwa, n).size) for n, _ in cm.OptSwa._fields_]
    assert offs == [("start", 0, 8), ("lr_start", 8, 8), ("freq", 16, 4), ("anneal_steps", 20, 4), ("lr_factor", 24, 4), ("anneal_kind", 28, 4)]
    block = header[header.index("typedef struct avmoe_opt_swa {"):header.index("} avmoe_opt_swa;")]
    pos = [block.index(f" {n};") for n, _ in cm.OptSwa._fields_]
    assert pos == sorted(pos)
    for line, ctype in (("int64_t start;", 8), ("int64_t lr_start;", 8), ("int32_t freq;", 4), ("int32_t anneal_steps;", 4), ("float lr_factor;", 4),
                        ("int32_t anneal_kind;", 4)):
        assert line in block, line
    # the older constants keep their layouts
    assert C.sizeof(cm.OptSchedule) == 40 and C.sizeof(cm.OptEma) == 8


def test_state_block_is_still_64_bytes_with_its_words_where_they_are():
    assert cm.OPT_STATE_BYTES == 64
    assert cm.OPT_STATE_FIELDS == {"total_norm": (0, "float32"), "clip_coef": (4, "float32"), "bc1": (8, "float32"), "bc2_sqrt": (12, "float32"),
                                   "applied_steps": (16, "int64"), "skipped_steps": (24, "int64"), "skip": (32, "int32"),
                                   "lr_factor": (36, "float32"), "ema_decay": (40, "float32")}
    header = open(_capi.HEADER_PATH).read()
    block = header[header.index("typedef struct avmoe_opt_state"):header.index("} avmoe_opt_state;")]
    assert block.index("float lr_factor;") < block.index("float ema_decay;") < block.index("int32_t reserved[5];")
    lay = cm.OptLayout()
    raw, base = _buf(4096)
    r = (cm.OptRange * 1)()
    r[0].param, r[0].grad, r[0].exp_avg, r[0].exp_avg_sq, r[0].n, r[0].lr = base, base + 64, base + 128, base + 192, 4, 1e-3
    assert _capi.lib().avmoe_opt_workspace_bytes(r, 1, C.byref(lay)) > 0 and lay.state_bytes == 64


def _good(**kw):
    base = dict(start=5, freq=3, lr_start=6, anneal_steps=5, lr_factor=0.1, anneal_kind=0)
    base.update(kw)
    return cm.OptSwa(**base)


def test_swa_validation_precedes_any_launch():
    """host pointers everywhere: a call that got as far as a launch would fault or fail, these all return an argument error first"""
    L = _capi.lib()
    raw, base = _buf(8192)
    table, partials, state, report = base, base + 1024, base + 2048, base + 4096
    both = cm.OPT_CLIP | cm.OPT_SWA | cm.OPT_SWA_LR

    def norm(swa, flags=both, sched=None, ema=None, state=state):
        return L.avmoe_opt_grad_norm_swa(table, 2, 2, partials, state, 1.0, 1.0, flags, 0.9, 0.999, None, None if sched is None else C.byref(sched),
                                         None if ema is None else C.byref(ema), report, None if swa is None else C.byref(swa))

    # a flag without the struct
    for flags in (cm.OPT_SWA, cm.OPT_SWA_LR, both):
        assert norm(None, flags=flags) == BAD_ARG and "avmoe_opt_swa" in _err(), flags
    # every field, named in the message
    for field, values in (("start", (0, -1)), ("freq", (0, -2)), ("lr_start", (-1,)), ("anneal_steps", (-1,)),
                          ("lr_factor", (-0.1, 1.5, float("nan"), float("inf"))), ("anneal_kind", (2, -1, 7))):
        for v in values:
            assert norm(_good(**{field: v})) == BAD_ARG and field in _err(), (field, v, _err())
    # each half is checked under its own flag
    off_avg = _good(start=0, freq=0)
    assert norm(off_avg, flags=cm.OPT_CLIP | cm.OPT_SWA) == BAD_ARG and "start" in _err()
    off_lr = _good(lr_start=-1, anneal_steps=-1, lr_factor=2.0, anneal_kind=9)
    assert norm(off_lr, flags=cm.OPT_CLIP | cm.OPT_SWA_LR) == BAD_ARG and "lr_start" in _err()
    # the uniform average and the exponential one are alternatives
    ema = cm.OptEma(decay=0.9, warmup=10.0)
    assert norm(_good(), flags=both | cm.OPT_EMA, ema=ema) == BAD_ARG and "AVMOE_OPT_EMA" in _err()
    assert norm(_good(), flags=cm.OPT_SWA | cm.OPT_EMA, ema=ema) == BAD_ARG and "AVMOE_OPT_EMA" in _err()
    # what the entry points before it refuse: the schedule's flag without a schedule, a bad schedule, a flag nobody knows, the report's
    assert norm(_good(), flags=both | cm.OPT_LR_SCHEDULE) == BAD_ARG and "schedule" in _err()
    assert norm(_good(), flags=both | cm.OPT_LR_SCHEDULE, sched=cm.OptSchedule(warmup_steps=-1, gamma=1.0)) == BAD_ARG and _err()
    assert norm(_good(), flags=both | 256) == BAD_ARG and "unknown flag" in _err()
    assert L.avmoe_opt_grad_norm_swa(table, 2, 2, partials, state, 1.0, 1.0, both | cm.OPT_REPORT, 0.9, 0.999, None, None, None, None,
                                     C.byref(_good())) == BAD_ARG and "report" in _err()
    assert norm(_good(), state=None) == BAD_ARG and _err()


def test_the_older_entry_points_still_refuse_both_flags():
    L = _capi.lib()
    raw, base = _buf(8192)
    table, partials, state, shadows, report = base, base + 1024, base + 2048, base + 4096, base + 6144
    sched, ema = cm.OptSchedule(gamma=1.0), cm.OptEma(decay=0.9, warmup=10.0)
    for flag in (cm.OPT_SWA, cm.OPT_SWA_LR):
        flags = cm.OPT_CLIP | flag
        assert L.avmoe_opt_grad_norm(table, 2, 2, partials, state, 1.0, 1.0, flags, 0.9, 0.999, None) == BAD_ARG and "unknown flag" in _err()
        assert L.avmoe_opt_grad_norm_sched(table, 2, 2, partials, state, 1.0, 1.0, flags | cm.OPT_LR_SCHEDULE, 0.9, 0.999, None,
                                           C.byref(sched)) == BAD_ARG and "unknown flag" in _err()
        assert L.avmoe_opt_grad_norm_ema(table, 2, 2, partials, state, 1.0, 1.0, flags | cm.OPT_EMA, 0.9, 0.999, None, None,
                                         C.byref(ema)) == BAD_ARG and "unknown flag" in _err()
        assert L.avmoe_opt_grad_norm_report(table, 2, 2, partials, state, 1.0, 1.0, flags | cm.OPT_REPORT, 0.9, 0.999, None, None, None,
                                            report) == BAD_ARG and "unknown flag" in _err()
        assert L.avmoe_opt_adam_step(table, 2, 2, state, 0.9, 0.999, 1e-8, 1.0, flags, None) == BAD_ARG and "unknown flag" in _err()
        assert L.avmoe_opt_adam_step_ema(table, 2, 2, state, 0.9, 0.999, 1e-8, 1.0, flags, None, shadows) == BAD_ARG and "unknown flag" in _err()


def test_swa_decay_at_is_the_uniform_average_in_double_rounded_to_fp32():
    at, count = FlatAdam.swa_decay_at, FlatAdam.swa_n_averaged_at
    N, c = 5, 3
    for n in range(0, N):
        assert at(n, N, c) == 0.0 and count(n, N, c) == 0
    for n in range(N, 200):
        k, r = divmod(n - N, c)
        if r == 0:
            assert at(n, N, c) == f32(k / (k + 1.0)), n
        else:
            assert at(n, N, c) == 1.0, n
        assert count(n, N, c) == k + 1
    assert at(5, 5, 3) == 0.0 and at(8, 5, 3) == 0.5 and at(11, 5, 3) == f32(2.0 / 3.0) and at(6, 5, 3) == 1.0 and at(7, 5, 3) == 1.0
    assert [at(n, 1) for n in (1, 2, 3, 4)] == [0.0, 0.5, f32(2.0 / 3.0), 0.75]      # freq defaults to 1: every step from the first
    assert at(10 ** 12 + 1, 1, 1) == 1.0 and at(2 ** 24 + 5, 5, 1) == f32(2.0 ** 24 / (2.0 ** 24 + 1.0))      # k / (k + 1) rounds to 1 far out
    assert count(24, 5, 3) == 7 and count(5, 5, 3) == 1 and count(7, 5, 3) == 1 and count(8, 5, 3) == 2
    assert isinstance(at(8, 5, 3), float) and isinstance(count(8, 5, 3), int)
    for bad in (dict(start=0), dict(start=-2), dict(start=1.5), dict(start=None), dict(start=True), dict(freq=0), dict(freq=-1), dict(freq=2.5),
                dict(start=float("nan")), dict(freq=float("inf")), dict(freq=2 ** 31)):
        with pytest.raises(ValueError):
            at(7, **{"start": 5, "freq": 3, **bad})
        with pytest.raises(ValueError):
            count(7, **{"start": 5, "freq": 3, **bad})


def _torch_chain(s, n_steps, lr0=0.05):
    """the rates of torch's own schedulers driven as the class docstring says: LambdaLR(base) stepped once per step until step swa_start
    is due, SWALR constructed then and stepped once per step from there"""
    from torch.optim.lr_scheduler import LambdaLR
    from torch.optim.swa_utils import SWALR
    p = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.SGD([p], lr=lr0)
    base = LRSchedule(warmup_steps=s.warmup_steps, warmup_start=s.warmup_start, decay_kind=s.decay_kind, total_steps=s.total_steps,
                      min_factor=s.min_factor, step_size=s.step_size, gamma=s.gamma)
    out = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        sch = LambdaLR(opt, base.factor)
        for n in range(n_steps):
            if n == s.swa_start:
                sch = SWALR(opt, swa_lr=s.swa_factor * lr0, anneal_epochs=s.swa_anneal_steps, anneal_strategy=s.swa_anneal)
            out.append(opt.param_groups[0]["lr"])          # the rate step n is taken with
            opt.step()
            sch.step()
    return out


@pytest.mark.parametrize("kind", ["cos", "linear"])
@pytest.mark.parametrize("start", [1, 7, 25])
@pytest.mark.parametrize("anneal", [0, 1, 5, 20])
def test_factor_is_torchs_lambda_lr_then_swalr(anneal, start, kind):
    lr0, worst = 0.05, 0.0
    for base in (dict(warmup_steps=4, warmup_start=0.1, decay_kind="cosine", total_steps=40, min_factor=0.05), dict()):
        s = LRSchedule(swa_start=start, swa_factor=0.3, swa_anneal_steps=anneal, swa_anneal=kind, **base)
        want = _torch_chain(s, 60, lr0)
        for n in range(60):
            got = lr0 * s.factor(n)
            rel = abs(got - want[n]) / abs(want[n])
            worst = max(worst, rel)
            assert rel <= 1e-12, (base, n, got, want[n], rel)
        assert f32(s.factor(start + anneal)) == s.swa_factor == f32(s.factor(10 ** 9))       # the plateau, as the device rounds it
    print(f"A = {anneal}, N' = {start}, {kind}: worst relative difference to torch {worst:.2e}")


def test_a_schedule_without_the_swa_fields_is_what_it_was():
    kw = dict(warmup_steps=3, warmup_start=0.1, decay_kind="cosine", total_steps=10, min_factor=0.05)
    s = LRSchedule(**kw)
    assert s.swa_start is None
    W, s0, fmin, D = 3, f32(0.1), f32(0.05), 7
    for n in range(30):
        want = s0 + (1.0 - s0) * n / W if n < W else fmin + (1.0 - fmin) * 0.5 * (1.0 + math.cos(math.pi * min(n - W, D) / D))
        assert s.factor(n) == want, n
    for kind, more in (("linear", dict(total_steps=9)), ("step", dict(step_size=4, gamma=0.5)), ("none", dict())):
        a = LRSchedule(warmup_steps=2, decay_kind=kind, **more)
        b = LRSchedule(warmup_steps=2, decay_kind=kind, swa_start=10 ** 6, swa_factor=0.5, **more)      # the SWA part far away
        assert [a.factor(n) for n in range(40)] == [b.factor(n) for n in range(40)]
        assert bytes(a.c_struct()) == bytes(b.c_struct())
    c = s.c_struct()
    assert C.sizeof(c) == 40 and bytes(c) == bytes(cm.OptSchedule(warmup_steps=3, warmup_start=0.1, decay_kind=1, total_steps=10, min_factor=0.05,
                                                                   gamma=1.0, step_size=0))
    w = cm.OptSwa()
    assert s.fill_swa(w) is False and bytes(w) == bytes(32)
    t = LRSchedule(swa_start=0, swa_factor=0.25, swa_anneal_steps=7, swa_anneal="linear")               # the SWA part alone is a schedule
    assert t.fill_swa(w) is True and (w.lr_start, w.anneal_steps, w.lr_factor, w.anneal_kind) == (0, 7, 0.25, 1) and (w.start, w.freq) == (0, 0)
    assert t.factor(0) == 1.0 and t.factor(7) == 0.25 and t.factor(3) == 1.0 + (0.25 - 1.0) * (3 / 7)
    import dataclasses
    assert LRSchedule(**dataclasses.asdict(t)) == t and set(dataclasses.asdict(t)) >= {"swa_start", "swa_factor", "swa_anneal_steps", "swa_anneal"}


BAD_SCHED = [dict(swa_start=-1), dict(swa_start=1.5), dict(swa_start=True), dict(swa_start=3, swa_factor=1.1), dict(swa_start=3, swa_factor=-0.1),
             dict(swa_start=3, swa_factor=float("nan")), dict(swa_start=3, swa_anneal_steps=-1), dict(swa_start=3, swa_anneal_steps=0.5),
             dict(swa_start=3, swa_anneal="step"), dict(swa_start=3, swa_anneal=1)]


@pytest.mark.parametrize("kw", BAD_SCHED, ids=[",".join(f"{k}={v}" for k, v in kw.items()) for kw in BAD_SCHED])
def test_bad_schedule_arguments_raise_value_error(kw):
    with pytest.raises(ValueError, match="swa_"):
        LRSchedule(**kw)


BAD_CTOR = [dict(swa_start=5, ema_decay=0.9), dict(swa_freq=0), dict(swa_start=5, swa_freq=0), dict(swa_start=0), dict(swa_start=-3),
            dict(swa_start=2.5), dict(swa_start=5, swa_freq=-1), dict(swa_start=5, swa_freq=1.5), dict(swa_start=True)]


@pytest.mark.parametrize("kw", BAD_CTOR, ids=[",".join(f"{k}={v}" for k, v in kw.items()) for kw in BAD_CTOR])
def test_bad_constructor_arguments_raise_value_error(kw):
    from avmoe_amd.dp import AdapterGradReducer
    red = AdapterGradReducer([torch.nn.Parameter(torch.zeros(7))])
    with pytest.raises(ValueError, match="swa_"):
        FlatAdam(red, **kw)


def test_swa_selects_the_device_path_and_buffers_accept_it():
    from avmoe_amd.dp import AdapterGradReducer
    import inspect
    red = AdapterGradReducer([torch.nn.Parameter(torch.zeros(7))])
    with pytest.raises(_capi.AvmoeError):                    # a good value gets as far as the buckets: the device path has no CPU fallback
        FlatAdam(red, swa_start=5, swa_freq=3)
    with pytest.raises(_capi.AvmoeError):                    # ema_buffers with swa_start passes the "needs an average" check
        FlatAdam(red, swa_start=5, ema_buffers=[("b", torch.zeros(3))])
    with pytest.raises(ValueError, match="ema_buffers needs"):
        FlatAdam(red, ema_buffers=[("b", torch.zeros(3))])
    sig = inspect.signature(FlatAdam.__init__).parameters
    assert sig["swa_start"].default is None and sig["swa_freq"].default == 1
    assert "Stochastic weight averaging" in FlatAdam.__doc__
