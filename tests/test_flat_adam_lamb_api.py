"""Host side of the layer-wise trust ratios in FlatAdam (include/avmoe.h: avmoe_opt_lamb_bytes, avmoe_opt_lamb_step;
avmoe_amd.train.FlatAdam(trust_ratio=..., trust_clip=...)): the symbols and the layouts the binding relies on, the size function, the
argument checks of both layers (they precede any launch, so host pointers and a NULL stream are enough and no GPU is needed) and the
host's copy of the rule."""
import ctypes as C
import inspect
import math

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


def test_header_declares_and_library_exports_the_two_entry_points():
    L = _capi.lib()
    header = open(_capi.HEADER_PATH).read()
    assert f"AVMOE_ERR_BAD_ARG = {BAD_ARG}," in header and f"AVMOE_ERR_ALIGNMENT = {ALIGNMENT}," in header
    for name in ("avmoe_opt_lamb_bytes", "avmoe_opt_lamb_step"):
        assert name in _capi.exported_symbols() and hasattr(L, name), name
    assert L.avmoe_abi_version() == 11
    assert "typedef struct avmoe_opt_lamb_header" in header and "typedef struct avmoe_opt_lamb_layout" in header
    assert C.sizeof(cm.OptLambHeader) == 16 and C.sizeof(cm.OptLambLayout) == 2 * C.sizeof(C.c_size_t)
    # no flag was added, the range and the state block are what they were
    assert (cm.OPT_CLIP | cm.OPT_SKIP_NONFINITE | cm.OPT_DECOUPLED_DECAY | cm.OPT_LR_SCHEDULE | cm.OPT_EMA | cm.OPT_REPORT | cm.OPT_SWA
            | cm.OPT_SWA_LR) == 255
    assert C.sizeof(cm.OptRange) == 48 and cm.OPT_STATE_BYTES == 64
    block = header[header.index("typedef struct avmoe_opt_state"):header.index("} avmoe_opt_state;")]
    assert "int32_t reserved[5];" in block


def test_the_size_function_on_good_and_bad_counts():
    L = _capi.lib()
    lay = cm.OptLambLayout()
    for n_ranges, n_blocks in ((0, 0), (1, 1), (3, 5), (13, 80), (466, 4000), (5, 0)):
        total = L.avmoe_opt_lamb_bytes(n_ranges, n_blocks, C.byref(lay))
        assert lay.workspace_bytes % 16 == 0 and lay.report_bytes % 16 == 0
        assert lay.workspace_bytes >= 16 * max(n_blocks, 1) and lay.workspace_bytes < 16 * max(n_blocks, 1) + 16      # two doubles per block
        assert lay.report_bytes >= 16 + 12 * n_ranges and lay.report_bytes < 16 + 12 * n_ranges + 16                 # header + three floats per range
        assert total == lay.workspace_bytes + lay.report_bytes
        assert L.avmoe_opt_lamb_bytes(n_ranges, n_blocks, None) == total
    lay.workspace_bytes = lay.report_bytes = 7
    for n_ranges, n_blocks in ((-1, 0), (0, -1), (-5, -5), (1, 1 << 31)):
        assert L.avmoe_opt_lamb_bytes(n_ranges, n_blocks, C.byref(lay)) == 0 and "avmoe_opt_lamb_bytes" in _err(), (n_ranges, n_blocks)
    assert lay.workspace_bytes == 7 and lay.report_bytes == 7               # a refused call leaves the layout alone


def _calls():
    L = _capi.lib()
    raw, base = _buf(16384)
    table, state, shadows, hold, limits, ws, report = (base + 2048 * k for k in range(7))

    def lamb(table=table, state=state, flags=cm.OPT_CLIP, shadows=shadows, b1=0.9, b2=0.999, eps=1e-8, gs=1.0, n_ranges=2, n_blocks=2, hold=hold,
             limits=limits, ws=ws, report=report):
        return L.avmoe_opt_lamb_step(table, n_ranges, n_blocks, state, b1, b2, eps, gs, flags, None, shadows, hold, limits, ws, report)

    def ema(table=table, state=state, flags=cm.OPT_CLIP, shadows=shadows, b1=0.9, b2=0.999, eps=1e-8, gs=1.0, n_ranges=2, n_blocks=2):
        return L.avmoe_opt_adam_step_ema(table, n_ranges, n_blocks, state, b1, b2, eps, gs, flags, None, shadows)

    def sam(table=table, state=state, flags=cm.OPT_CLIP, shadows=shadows, b1=0.9, b2=0.999, eps=1e-8, gs=1.0, n_ranges=2, n_blocks=2, hold=hold):
        return L.avmoe_opt_adam_step_sam(table, n_ranges, n_blocks, state, b1, b2, eps, gs, flags, None, shadows, hold)

    return raw, dict(table=table, state=state, shadows=shadows, hold=hold, limits=limits, ws=ws, report=report), lamb, ema, sam


REFUSALS = [dict(state=None), dict(state=8), dict(table=None), dict(table=8), dict(n_ranges=-1), dict(n_blocks=-1),
            dict(b1=1.0), dict(b2=-0.1), dict(b1=float("nan")), dict(eps=-1.0), dict(eps=float("nan")), dict(gs=float("nan")),
            dict(flags=cm.OPT_CLIP | cm.OPT_REPORT), dict(flags=cm.OPT_SWA), dict(flags=cm.OPT_SWA_LR), dict(flags=256),
            dict(flags=cm.OPT_EMA, shadows=None), dict(flags=cm.OPT_EMA, shadows=4)]


def _resolve(kw, ptrs):
    """an integer for a pointer argument is an offset from the good pointer"""
    return {k: (ptrs[k] + v if k in ptrs and isinstance(v, int) else v) for k, v in kw.items()}


def test_lamb_step_refuses_what_the_update_entry_points_refuse():
    """with hold: everything avmoe_opt_adam_step_sam refuses; without: everything avmoe_opt_adam_step_ema refuses -- the same status and,
    the function's name apart, the same message, before any launch (host pointers: a launch would fault)"""
    raw, ptrs, lamb, ema, sam = _calls()
    for kw in REFUSALS:
        kw = _resolve(kw, ptrs)
        want = sam(**kw)
        assert want in (BAD_ARG, ALIGNMENT), kw
        msg = _err().replace("avmoe_opt_adam_step_sam", "")
        assert lamb(**kw) == want, kw
        assert _err().replace("avmoe_opt_lamb_step", "") == msg, kw
        want = ema(**kw)
        assert want in (BAD_ARG, ALIGNMENT), kw
        msg = _err().replace("avmoe_opt_adam_step_ema", "")
        assert lamb(hold=None, **kw) == want, kw
        assert _err().replace("avmoe_opt_lamb_step", "") == msg, kw
    assert lamb(hold=ptrs["hold"] + 4) == ALIGNMENT and "hold" in _err()
    assert sam(hold=ptrs["hold"] + 4) == ALIGNMENT


def test_lamb_step_refuses_its_own_arguments_before_any_launch():
    raw, ptrs, lamb, ema, sam = _calls()
    for hold in (ptrs["hold"], None):
        for name in ("limits", "ws", "report"):
            assert lamb(hold=hold, **{name: None}) == BAD_ARG and "NULL" in _err(), name
        assert lamb(hold=hold, limits=ptrs["limits"] + 2) == ALIGNMENT and "limits" in _err()
        for off in (4, 2):
            assert lamb(hold=hold, ws=ptrs["ws"] + off) == ALIGNMENT and "workspace" in _err(), off
        for off in (4, 8, 12):
            assert lamb(hold=hold, report=ptrs["report"] + off) == ALIGNMENT and "report" in _err(), off
        assert lamb(hold=hold, n_blocks=-1) == BAD_ARG
        # NULL comes before alignment, and the shared checks before both
        assert lamb(hold=hold, limits=None, report=ptrs["report"] + 4) == BAD_ARG
        assert lamb(hold=hold, limits=None, eps=-1.0) == BAD_ARG and "eps" in _err()
        # nothing to launch: the good call returns OK without a GPU, shadows may be NULL without the average
        assert lamb(hold=hold, n_ranges=0, n_blocks=0, shadows=None) == 0


def test_the_older_entry_points_keep_their_refusals():
    """the trust ratio got no flag: 256 stays unknown everywhere, and the update entry points refuse what they refused"""
    L = _capi.lib()
    raw, base = _buf(8192)
    table, partials, state, shadows, report = base, base + 1024, base + 2048, base + 4096, base + 6144
    assert L.avmoe_opt_grad_norm_swa(table, 2, 2, partials, state, 1.0, 1.0, cm.OPT_CLIP | 256, 0.9, 0.999, None, None, None, report,
                                     None) == BAD_ARG and "unknown flag" in _err()
    assert L.avmoe_opt_grad_norm_report(table, 2, 2, partials, state, 1.0, 1.0, cm.OPT_SWA, 0.9, 0.999, None, None, None, report) == BAD_ARG \
        and "unknown flag" in _err()
    assert L.avmoe_opt_adam_step(table, 2, 2, state, 0.9, 0.999, 1e-8, 1.0, 256, None) == BAD_ARG and "unknown flag" in _err()
    assert L.avmoe_opt_adam_step(table, 2, 2, state, 0.9, 0.999, 1e-8, 1.0, cm.OPT_EMA, None) == BAD_ARG and "unknown flag" in _err()
    assert L.avmoe_opt_adam_step_ema(table, 2, 2, state, 0.9, 0.999, 1e-8, 1.0, 256, None, shadows) == BAD_ARG and "unknown flag" in _err()
    assert L.avmoe_opt_adam_step_ema(table, 2, 2, state, 0.9, 0.999, 1e-8, 1.0, cm.OPT_EMA, None, None) == BAD_ARG and "shadow" in _err()
    assert L.avmoe_opt_adam_step_sam(table, 2, 2, state, 0.9, 0.999, 1e-8, 1.0, cm.OPT_CLIP, None, None, None) == BAD_ARG and "hold" in _err()
    assert L.avmoe_opt_adam_step_sam(table, 2, 2, state, 0.9, 0.999, -1.0, 1.0, cm.OPT_CLIP, None, None, shadows) == BAD_ARG and "eps" in _err()
    assert L.avmoe_opt_adam_step_ema(table, 2, 0, state, 0.9, 0.999, 1e-8, 1.0, cm.OPT_CLIP, None, None) == 0


def _reducer():
    from avmoe_amd.dp import AdapterGradReducer
    w, b = torch.nn.Parameter(torch.zeros(3, 4)), torch.nn.Parameter(torch.zeros(7))
    return AdapterGradReducer([w, b]), w, b


BAD_CTOR = [dict(trust_ratio=1), dict(trust_ratio=None), dict(trust_ratio="yes"), dict(trust_ratio=0.5),
            dict(trust_ratio=True, trust_clip=0.0), dict(trust_ratio=True, trust_clip=-1.0), dict(trust_ratio=True, trust_clip=float("nan")),
            dict(trust_ratio=True, trust_clip=1e-60), dict(trust_clip=10.0), dict(trust_ratio=False, trust_clip=10.0)]


@pytest.mark.parametrize("kw", BAD_CTOR, ids=[",".join(f"{k}={v}" for k, v in kw.items()) for kw in BAD_CTOR])
def test_bad_constructor_arguments_raise_value_error_before_anything_is_touched(kw):
    red, w, b = _reducer()
    ptrs = (w.data_ptr(), b.data_ptr())
    with pytest.raises(ValueError, match="trust_"):
        FlatAdam(red, **kw)
    assert (w.data_ptr(), b.data_ptr()) == ptrs


@pytest.mark.parametrize("value", [1, 0, None, "no", 1.0])
def test_a_groups_trust_ratio_must_be_a_bool(value):
    red, w, b = _reducer()
    ptrs = (w.data_ptr(), b.data_ptr())
    with pytest.raises(ValueError, match="trust_ratio"):
        FlatAdam(red, trust_ratio=True, param_groups=[{"params": [w], "trust_ratio": value}])
    assert (w.data_ptr(), b.data_ptr()) == ptrs


def test_trust_ratio_selects_the_device_path():
    for kw in (dict(trust_ratio=True), dict(trust_ratio=True, trust_clip=10.0)):
        red, w, b = _reducer()
        with pytest.raises(_capi.AvmoeError):                # a good value gets as far as the buckets: the device path has no CPU fallback
            FlatAdam(red, param_groups=[{"params": [b], "trust_ratio": True}], **kw)
    sig = inspect.signature(FlatAdam.__init__).parameters
    assert sig["trust_ratio"].default is False and sig["trust_clip"].default is None
    assert "Layer-wise trust ratios" in FlatAdam.__doc__ and "NOT bit-equal" in FlatAdam.__doc__
    assert FlatAdam._check_trust(True, 10.0) == (True, 10.0) and FlatAdam._check_trust(False, None) == (False, None)
    assert FlatAdam._check_trust(True, 0.1) == (True, float(np.float32(0.1)))
    for name in ("last_trust_ratios", "last_param_norms", "last_update_norms", "trust_ratio_of", "adapted"):
        assert hasattr(FlatAdam, name), name


def test_the_hosts_copy_of_the_rule():
    f = FlatAdam.trust_ratio_of
    # a zero norm on either side, a norm that is not finite: exactly 1
    for w, u in ((0.0, 1.0), (1.0, 0.0), (0.0, 0.0), (float("inf"), 1.0), (1.0, float("inf")), (float("nan"), 1.0), (1.0, float("nan")),
                 (float("inf"), float("inf"))):
        assert f(w, u) == 1.0 and f(w, u, clip=0.5) == 1.0, (w, u)
    # no clamp: the double quotient, rounded once to fp32
    for w, u in ((3.0, 7.0), (1e-3, 12.5), (123.456, 1e-4), (float(np.float32(0.1)), float(np.float32(0.3)))):
        got = f(w, u)
        assert got == float(np.float32(np.float64(w) / np.float64(u))) and got == float(np.float32(got)), (w, u)
    # the clamp, held as fp32
    assert f(10.0, 1.0, clip=4.0) == 4.0 and f(10.0, 1.0, clip=40.0) == 10.0
    assert f(10.0, 1.0, clip=0.1) == float(np.float32(0.1))
    assert f(1.0, 3.0, clip=10.0) == float(np.float32(1.0 / 3.0))
    assert math.isfinite(f(1.0, 3.0))
