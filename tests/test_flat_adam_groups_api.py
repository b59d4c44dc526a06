"""Host side of FlatAdam's per-range gradient norms (include/avmoe.h: AVMOE_OPT_REPORT, avmoe_opt_report_header, avmoe_opt_report_bytes,
avmoe_opt_grad_norm_report; avmoe_amd.train.FlatAdam(report_grad_norms=...)) and of the per-group weight decay: the symbols and layouts the
binding relies on and the argument checks, which precede any launch, so host pointers and a NULL stream are enough and no GPU is needed."""
import ctypes as C
import inspect

import pytest
import torch

from avmoe_amd import _capi
from avmoe_amd import _capi_moe as cm
from avmoe_amd.train import FlatAdam

BAD_ARG, ALIGNMENT = -1, -3
NEW = ("avmoe_opt_report_bytes", "avmoe_opt_grad_norm_report")


def _buf(nbytes):
    raw = C.create_string_buffer(nbytes + 64)
    return raw, (C.addressof(raw) + 63) & ~63


def _err():
    msg = _capi.lib().avmoe_last_error()
    return msg.decode() if msg else ""


def test_header_declares_and_library_exports_the_report_entry_points():
    L = _capi.lib()
    for name in NEW:
        assert name in _capi.exported_symbols() and hasattr(L, name), name
    assert L.avmoe_abi_version() == 11
    assert cm.OPT_REPORT == 32
    header = open(_capi.HEADER_PATH).read()
    assert "AVMOE_OPT_REPORT = 32" in header and "typedef struct avmoe_opt_report_header" in header
    block = header[header.index("typedef struct avmoe_opt_state"):header.index("} avmoe_opt_state;")]
    assert "int32_t reserved[5];" in block               # the state block gave nothing up for the report


def test_layouts_are_unchanged_and_the_report_header_is_16_bytes():
    assert cm.OPT_STATE_BYTES == 64 and C.sizeof(cm.OptRange) == 48
    assert C.sizeof(cm.OptReportHeader) == 16
    offs = [(n, getattr(cm.OptReportHeader, n).offset) for n, _ in cm.OptReportHeader._fields_]
    assert offs == [("first_nonfinite", 0), ("n_ranges", 4), ("reserved", 8)]
    lay = cm.OptLayout()
    raw, base = _buf(4096)
    r = (cm.OptRange * 1)()
    r[0].param, r[0].grad, r[0].exp_avg, r[0].exp_avg_sq, r[0].n, r[0].lr = base, base + 64, base + 128, base + 192, 4, 1e-3
    assert _capi.lib().avmoe_opt_workspace_bytes(r, 1, C.byref(lay)) > 0 and lay.state_bytes == 64


@pytest.mark.parametrize("n", [0, 1, 5])
def test_report_bytes_is_header_plus_the_floats_rounded_to_16(n):
    assert _capi.lib().avmoe_opt_report_bytes(n) == 16 + ((4 * n + 15) // 16) * 16


def test_report_bytes_refuses_a_negative_count():
    assert _capi.lib().avmoe_opt_report_bytes(-1) == 0 and "negative" in _err()


def test_report_validation_precedes_any_launch():
    """host pointers everywhere: a call that got as far as a launch would fault or fail, these all return an argument error first"""
    L = _capi.lib()
    raw, base = _buf(8192)
    table, partials, state, report = base, base + 1024, base + 2048, base + 4096
    flags = cm.OPT_CLIP | cm.OPT_REPORT

    def norm(report=report, flags=flags, state=state):
        return L.avmoe_opt_grad_norm_report(table, 2, 2, partials, state, 1.0, 1.0, flags, 0.9, 0.999, None, None, None, report)

    assert norm(report=None) == BAD_ARG and "report" in _err()
    assert norm(report=report + 8) == ALIGNMENT and "report" in _err()
    # it knows every flag: those of the older entry points still need what they needed there
    assert norm(flags=flags | cm.OPT_EMA) == BAD_ARG and "EMA" in _err()
    assert norm(flags=flags | cm.OPT_LR_SCHEDULE) == BAD_ARG and "schedule" in _err()
    assert norm(flags=flags | 64) == BAD_ARG and "unknown flag" in _err()
    assert norm(state=None) == BAD_ARG and _err()
    # the flag at the older entry points is an unknown flag
    good = cm.OptEma(decay=0.9, warmup=10.0)
    assert L.avmoe_opt_grad_norm_ema(table, 2, 2, partials, state, 1.0, 1.0, flags | cm.OPT_EMA, 0.9, 0.999, None, None,
                                     C.byref(good)) == BAD_ARG and "unknown flag" in _err()
    assert L.avmoe_opt_grad_norm(table, 2, 2, partials, state, 1.0, 1.0, flags, 0.9, 0.999, None) == BAD_ARG and "unknown flag" in _err()


def test_the_option_selects_the_device_path_and_its_accessors_need_it():
    from avmoe_amd.dp import AdapterGradReducer
    red = AdapterGradReducer([torch.nn.Parameter(torch.zeros(7))])
    with pytest.raises(_capi.AvmoeError):                    # the option gets as far as the buckets: the device path has no CPU fallback
        FlatAdam(red, report_grad_norms=True)
    assert inspect.signature(FlatAdam.__init__).parameters["report_grad_norms"].default is False
    for name in ("last_param_grad_norms", "first_nonfinite_param", "param_names"):
        assert hasattr(FlatAdam, name), name
