"""Host side of schedule-free AdamW in FlatAdam (include/avmoe.h: avmoe_opt_sf_step; avmoe_amd.train.FlatAdam(schedule_free=True,
sf_r=..., sf_lr_power=...)): the symbol and the layouts the binding relies on, the argument checks of both layers (they precede any
launch, so host pointers and a NULL stream are enough and no GPU is needed), and the host halves of state_dict() / load_state_dict()
(what is written, what a dict of either kind does to an optimizer of either kind; the round trip on the device is the GPU test's)."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest
import torch

from avmoe_amd import _capi
from avmoe_amd import _capi_moe as cm
from avmoe_amd.train import FlatAdam

BAD_ARG, ALIGNMENT = -1, -3


def _buf(nbytes):
    raw = C.create_string_buffer(nbytes + 64)
    return raw, (C.addressof(raw) + 63) & ~63


def _err():
    msg = _capi.lib().avmoe_last_error()
    return msg.decode() if msg else ""


def test_header_declares_and_library_exports_the_entry_point():
    L = _capi.lib()
    header = open(_capi.HEADER_PATH).read()
    assert "avmoe_opt_sf_step" in _capi.exported_symbols() and hasattr(L, "avmoe_opt_sf_step") and "avmoe_opt_sf_step(" in header
    assert L.avmoe_abi_version() == 11
    for name in ("avmoe_opt_sf_state", "avmoe_opt_sf"):
        assert f"typedef struct {name} " in header, name
    assert C.sizeof(cm.OptSfState) == 32 and C.sizeof(cm.OptSf) == 8
    assert {k: o for k, (o, _dt) in cm.OPT_SF_FIELDS.items()} == {k: getattr(cm.OptSfState, k).offset for k in ("weight_sum", "f_max", "c", "d")}
    assert cm.OPT_SF_FIELDS == {"weight_sum": (0, "float64"), "f_max": (8, "float32"), "c": (12, "float32"), "d": (16, "float32")}
    assert (cm.OptSf.r.offset, cm.OptSf.lr_power.offset) == (0, 4)
    block = header[header.index("typedef struct avmoe_opt_sf_state"):header.index("} avmoe_opt_sf_state;")]
    assert [ln.split(";")[0].strip() for ln in block.splitlines()[1:]] == ["double weight_sum", "float f_max", "float c", "float d",
                                                                          "int32_t reserved[3]"]
    # no flag was added, the range and the state block are what they were
    assert (cm.OPT_CLIP | cm.OPT_SKIP_NONFINITE | cm.OPT_DECOUPLED_DECAY | cm.OPT_LR_SCHEDULE | cm.OPT_EMA | cm.OPT_REPORT | cm.OPT_SWA
            | cm.OPT_SWA_LR) == 255
    assert C.sizeof(cm.OptRange) == 48 and cm.OPT_STATE_BYTES == 64
    state = header[header.index("typedef struct avmoe_opt_state"):header.index("} avmoe_opt_state;")]
    assert "int32_t reserved[5];" in state and "avmoe_opt_sf_step" in state      # the field's comment names the one step call that writes it
    # the kernels exist once, under the names a trace shows, and the rule is spelled once
    csrc = os.path.join(os.path.dirname(_capi.HEADER_PATH), "..", "avmoe_amd", "csrc")
    src = open(os.path.join(csrc, "opt_sched_free.hip")).read()
    assert src.count("__global__ void __launch_bounds__(64) kk_opt_sf_weights(") == 1
    assert src.count("__global__ void __launch_bounds__(256) kk_opt_sf_update(") == 1
    elem = open(os.path.join(csrc, "adam_elem.h")).read()
    assert elem.count("void sf_elem(") == 1 and elem.count("void sf_quad(") == 1 and "sf_elem" not in src.split("namespace avmoe {")[1]
    for other in ("opt_kernels.hip", "opt_muon.hip", "opt_muon_large.hip", "train_kernels.hip"):
        assert "kk_opt_sf_" not in open(os.path.join(csrc, other)).read(), other


def _calls():
    L = _capi.lib()
    raw, base = _buf(12288)
    table, state, x, hold, block = (base + 2048 * k for k in range(5))
    good = cm.OptSf(r=0.0, lr_power=2.0)

    def sf(table=table, state=state, flags=cm.OPT_CLIP, b1=0.9, b2=0.999, eps=1e-8, gs=1.0, n_ranges=2, n_blocks=2, x=x, hold=hold, consts=good,
           block=block):
        return L.avmoe_opt_sf_step(table, n_ranges, n_blocks, state, b1, b2, eps, gs, flags, None, x, hold, None if consts is None else C.byref(consts),
                                   block)

    def ema(table=table, state=state, flags=cm.OPT_CLIP, b1=0.9, b2=0.999, eps=1e-8, gs=1.0, n_ranges=2, n_blocks=2):
        return L.avmoe_opt_adam_step_ema(table, n_ranges, n_blocks, state, b1, b2, eps, gs, flags, None, x)

    def sam(table=table, state=state, flags=cm.OPT_CLIP, b1=0.9, b2=0.999, eps=1e-8, gs=1.0, n_ranges=2, n_blocks=2, hold=hold):
        return L.avmoe_opt_adam_step_sam(table, n_ranges, n_blocks, state, b1, b2, eps, gs, flags, None, x, hold)

    return raw, dict(table=table, state=state, x=x, hold=hold, block=block), sf, ema, sam


# what avmoe_opt_adam_step_ema / _sam refuse with flags the schedule-free step accepts too
REFUSALS = [dict(state=None), dict(state=8), dict(table=None), dict(table=8), dict(n_ranges=-1), dict(n_blocks=-1),
            dict(b1=1.0), dict(b2=-0.1), dict(b1=float("nan")), dict(eps=-1.0), dict(eps=float("nan")), dict(gs=float("nan")),
            dict(flags=cm.OPT_CLIP | cm.OPT_REPORT), dict(flags=cm.OPT_SWA), dict(flags=cm.OPT_SWA_LR), dict(flags=256)]


def _resolve(kw, ptrs):
    """an integer for a pointer argument is an offset from the good pointer"""
    return {k: (ptrs[k] + v if k in ptrs and isinstance(v, int) else v) for k, v in kw.items()}


def test_sf_step_refuses_what_the_update_entry_points_refuse():
    """with hold: everything avmoe_opt_adam_step_sam refuses; without: everything avmoe_opt_adam_step_ema refuses -- the same status and,
    the function's name apart, the same message, before any launch (host pointers: a launch would fault)"""
    raw, ptrs, sf, ema, sam = _calls()
    for kw in REFUSALS:
        kw = _resolve(kw, ptrs)
        want = sam(**kw)
        assert want in (BAD_ARG, ALIGNMENT), kw
        msg = _err().replace("avmoe_opt_adam_step_sam", "")
        assert sf(**kw) == want, kw
        assert "avmoe_opt_sf_step" in _err() and _err().replace("avmoe_opt_sf_step", "") == msg, kw
        want = ema(**kw)
        assert want in (BAD_ARG, ALIGNMENT), kw
        msg = _err().replace("avmoe_opt_adam_step_ema", "")
        assert sf(hold=None, **kw) == want, kw
        assert "avmoe_opt_sf_step" in _err() and _err().replace("avmoe_opt_sf_step", "") == msg, kw
    assert sf(hold=ptrs["hold"] + 4) == ALIGNMENT and "hold" in _err() and "avmoe_opt_sf_step" in _err()
    # the averaging is implied: its flag is not one of this entry point's
    assert sf(flags=cm.OPT_EMA) == BAD_ARG and "avmoe_opt_sf_step: unknown flag" in _err()
    assert sf(flags=cm.OPT_CLIP | cm.OPT_SKIP_NONFINITE | cm.OPT_DECOUPLED_DECAY | cm.OPT_LR_SCHEDULE, block=None) == BAD_ARG and "block" in _err()


BAD_CONSTS = [dict(r=-1.0), dict(r=-1e-30), dict(r=float("nan")), dict(r=float("inf")), dict(lr_power=-0.5), dict(lr_power=float("nan")),
              dict(lr_power=float("inf")), dict(lr_power=float("-inf"))]


def test_sf_step_refuses_its_own_arguments_before_any_launch():
    raw, ptrs, sf, ema, sam = _calls()
    for hold in (ptrs["hold"], None):
        for name in ("x", "consts", "block"):
            assert sf(hold=hold, **{name: None}) == BAD_ARG and "NULL" in _err() and "avmoe_opt_sf_step" in _err(), name
        for kw in BAD_CONSTS:
            c = dict(r=0.0, lr_power=2.0)
            c.update(kw)
            assert sf(hold=hold, consts=cm.OptSf(**c)) == BAD_ARG and "avmoe_opt_sf_step: " + next(iter(kw)) in _err(), kw
        for off in (4, 2):
            assert sf(hold=hold, x=ptrs["x"] + off) == ALIGNMENT and "pointer array" in _err() and "avmoe_opt_sf_step" in _err(), off
        for off in (4, 8, 12):
            assert sf(hold=hold, block=ptrs["block"] + off) == ALIGNMENT and "block" in _err() and "avmoe_opt_sf_step" in _err(), off
        # NULL and bad constants come before alignment, and the shared checks before both
        assert sf(hold=hold, x=None, block=ptrs["block"] + 4) == BAD_ARG
        assert sf(hold=hold, consts=cm.OptSf(r=-1.0, lr_power=2.0), block=ptrs["block"] + 4) == BAD_ARG
        assert sf(hold=hold, x=None, eps=-1.0) == BAD_ARG and "eps" in _err()
    # good constants at their edges pass the checks: both 0, both large -- refused only for what follows them
    for c in (dict(r=0.0, lr_power=0.0), dict(r=1.0, lr_power=0.0), dict(r=8.0, lr_power=16.0)):
        assert sf(consts=cm.OptSf(**c), block=ptrs["block"] + 4) == ALIGNMENT and "block" in _err(), c


def test_the_older_entry_points_keep_their_refusals():
    """the option got no flag: 256 stays unknown everywhere"""
    L = _capi.lib()
    raw, base = _buf(8192)
    table, partials, state, shadows, report = base, base + 1024, base + 2048, base + 4096, base + 6144
    assert L.avmoe_opt_grad_norm_swa(table, 2, 2, partials, state, 1.0, 1.0, cm.OPT_CLIP | 256, 0.9, 0.999, None, None, None, report,
                                     None) == BAD_ARG and "unknown flag" in _err()
    assert L.avmoe_opt_adam_step_ema(table, 2, 2, state, 0.9, 0.999, 1e-8, 1.0, 256, None, shadows) == BAD_ARG and "unknown flag" in _err()
    assert L.avmoe_opt_adam_step_ema(table, 2, 0, state, 0.9, 0.999, 1e-8, 1.0, cm.OPT_CLIP, None, None) == 0


def _reducer():
    from avmoe_amd.dp import AdapterGradReducer
    w, b = torch.nn.Parameter(torch.zeros(3, 4)), torch.nn.Parameter(torch.zeros(7))
    return AdapterGradReducer([w, b]), w, b


BAD_CTOR = [dict(schedule_free=1), dict(schedule_free=None), dict(schedule_free="yes"),
            dict(schedule_free=True, sf_r=-1.0), dict(schedule_free=True, sf_r=float("nan")), dict(schedule_free=True, sf_r=float("inf")),
            dict(schedule_free=True, sf_r=None), dict(schedule_free=True, sf_r=True),
            dict(schedule_free=True, sf_lr_power=-2.0), dict(schedule_free=True, sf_lr_power=float("nan")),
            dict(schedule_free=True, sf_lr_power=float("inf")), dict(schedule_free=True, sf_lr_power=1e60), dict(schedule_free=True, sf_lr_power="2"),
            dict(sf_r=1.0), dict(sf_lr_power=0.0),
            dict(schedule_free=True, ema_decay=0.99), dict(schedule_free=True, swa_start=5), dict(schedule_free=True, trust_ratio=True),
            dict(schedule_free=True, prodigy=True), dict(schedule_free=True, muon=True), dict(schedule_free=True, muon=True, muon_large=True),
            dict(schedule_free=True, ema_decay=0.9, trust_ratio=True)]


@pytest.mark.parametrize("kw", BAD_CTOR, ids=[",".join(f"{k}={v}" for k, v in kw.items()) for kw in BAD_CTOR])
def test_bad_constructor_arguments_raise_value_error_before_anything_is_touched(kw):
    red, w, b = _reducer()
    ptrs = (w.data_ptr(), b.data_ptr())
    with pytest.raises(ValueError, match="schedule_free"):
        FlatAdam(red, **kw)
    assert (w.data_ptr(), b.data_ptr()) == ptrs


def test_schedule_free_selects_the_device_path_and_composes_with_the_rest():
    from avmoe_amd.train import LRSchedule
    for kw in (dict(schedule_free=True), dict(schedule_free=True, sf_r=1.0, sf_lr_power=0.0),
               dict(schedule_free=True, max_grad_norm=1.0, skip_nonfinite=True, decoupled_weight_decay=True, weight_decay=0.01,
                    lr_schedule=LRSchedule(warmup_steps=3), report_grad_norms=True, sam_rho=0.05)):
        red, w, b = _reducer()
        with pytest.raises(_capi.AvmoeError):                # a good value gets as far as the buckets: the device path has no CPU fallback
            FlatAdam(red, **kw)
    sig = inspect.signature(FlatAdam.__init__).parameters
    assert sig["schedule_free"].default is False and sig["sf_r"].default == 0.0 and sig["sf_lr_power"].default == 2.0
    doc = FlatAdam.__doc__
    assert "Schedule-free" in doc and "schedule_free=True" in doc and "StepLR" in doc and "reestimate_bn" in doc
    assert FlatAdam._check_sf(True, 0, 2) == (True, 0.0, 2.0) and FlatAdam._check_sf(True, 0.1, 1.5) == (True, float(np.float32(0.1)), 1.5)
    assert FlatAdam._check_sf(False, 0.0, 2.0) == (False, 0.0, 2.0)
    for name in ("sf_c", "sf_weight_sum", "sf_lr_max", "sf_z", "sf_weights_next"):
        assert hasattr(FlatAdam, name), name
    # the accessors of the average name the option that would have built it
    bare = object.__new__(FlatAdam)
    bare.ema_decay = bare.swa_start = None
    bare.schedule_free = False
    for what in (lambda: bare.ema_params, lambda: bare.last_ema_decay, bare.swap_ema, lambda: bare.sf_c, lambda: bare.sf_z):
        with pytest.raises(_capi.AvmoeError, match="schedule_free"):
            what()
    with pytest.raises(ValueError, match="schedule_free"):
        bare._collect_buffers([("bn.running_mean", torch.zeros(4))], None)


def _host_optimizer(on, n=2):
    """the host half of an optimizer: what _save_sf / _check_saved_sf / _check_saved_average read, with the block's views on the CPU"""
    opt = object.__new__(FlatAdam)
    opt.ema_decay, opt.ema_warmup, opt.swa_start, opt.swa_freq = None, 10.0, None, 1
    opt.schedule_free, opt.sf_r, opt.sf_lr_power = on, 0.0, 2.0
    opt._recs = [type("R", (), {"p": torch.zeros(3)})() for _ in range(n)]
    if on:
        blk = torch.zeros(32, dtype=torch.uint8)
        opt._sf_views = {k: blk[o:o + (8 if dt == "float64" else 4)].view(getattr(torch, dt))[0] for k, (o, dt) in cm.OPT_SF_FIELDS.items()}
        opt._ema_views = [torch.full((3,), float(i)) for i in range(n)]
    return opt


def test_state_dict_keys_and_the_load_rules_in_both_directions():
    on, off = _host_optimizer(True), _host_optimizer(False)
    on._sf_views["weight_sum"].fill_(3.0); on._sf_views["f_max"].fill_(1.0); on._sf_views["c"].fill_(1.0 / 3.0); on._sf_views["d"].fill_(2.0 / 3.0)
    extra = {}
    on._save_sf(extra)
    on._save_average(extra)
    assert {"schedule_free", "sf_r", "sf_lr_power", "sf_weight_sum", "sf_lr_max", "sf_c", "ema"} <= set(extra)
    assert extra["schedule_free"] is True and (extra["sf_r"], extra["sf_lr_power"], extra["sf_weight_sum"], extra["sf_lr_max"]) == (0.0, 2.0, 3.0, 1.0)
    assert extra["sf_c"] == float(np.float32(1.0 / 3.0)) and len(extra["ema"]) == 2 and torch.equal(extra["ema"][1], torch.ones(3))
    assert "ema_decay" not in extra and "swa_start" not in extra
    # saved with the option -> built with it: the constants, the block's words and x come back
    consts, blk = on._check_saved_sf(dict(extra, sf_r=1.0, sf_lr_power=0.5))
    assert consts == (1.0, 0.5) and blk == {"weight_sum": 3.0, "f_max": 1.0, "c": extra["sf_c"], "d": float(np.float32(2.0 / 3.0))}
    saved, none = on._check_saved_average(extra)
    assert none is None and len(saved) == 2
    # saved with the option -> built without it: refused, naming the option
    with pytest.raises(ValueError, match="schedule_free"):
        off._check_saved_sf(extra)
    # saved without the option -> built with it: nothing to restore, z, x and the block are re-seeded; averages of another kind are not x
    for other in ({}, {"ema_decay": 0.9, "ema_warmup": 10.0, "ema": [torch.zeros(3)] * 2}, {"swa_start": 4, "swa_freq": 1, "ema": [torch.zeros(3)] * 2}):
        if "swa_start" in other:
            with pytest.raises(ValueError, match="swa_start"):       # (the uniform average's own rule: it needs an optimizer built with it)
                on._check_saved_average(other)
        else:
            assert on._check_saved_sf(other) is None and on._check_saved_average(other) is None
    assert off._check_saved_sf({}) is None
    # a damaged dict is refused before anything is written
    for bad in (dict(sf_r=-1.0), dict(sf_lr_power=float("nan")), dict(sf_weight_sum=float("inf")), dict(sf_weight_sum=-1.0), dict(sf_c=1.5),
                dict(sf_lr_max=float("nan")), dict(ema=None), dict(sf_d=2.0)):
        with pytest.raises(ValueError, match="sf_|schedule_free"):
            on._check_saved_sf(dict(extra, **bad))
    with pytest.raises(ValueError, match="averaged parameters"):
        on._check_saved_average(dict(extra, ema=[torch.zeros(3)]))
