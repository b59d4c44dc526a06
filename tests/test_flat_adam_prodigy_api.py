"""Host side of Prodigy learning-rate estimation in FlatAdam (include/avmoe.h: avmoe_opt_prodigy_bytes, avmoe_opt_prodigy_step;
avmoe_amd.train.FlatAdam(prodigy=..., prodigy_d0=..., ...)): the symbols and the layouts the binding relies on, the size function, the
argument checks of both layers (they precede any launch, so host pointers and a NULL stream are enough and no GPU is needed) and the
host's copy of the finalize rule."""
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
    for name in ("avmoe_opt_prodigy_bytes", "avmoe_opt_prodigy_step"):
        assert name in _capi.exported_symbols() and hasattr(L, name) and name + "(" in header, name
    assert L.avmoe_abi_version() == 11
    for name in ("avmoe_opt_prodigy_state", "avmoe_opt_prodigy", "avmoe_opt_prodigy_layout"):
        assert f"typedef struct {name} " in header, name
    assert C.sizeof(cm.OptProdigyState) == 32 and C.sizeof(cm.OptProdigy) == 16 and C.sizeof(cm.OptProdigyLayout) == 2 * C.sizeof(C.c_size_t)
    assert {k: o for k, (o, _dt) in cm.OPT_PRODIGY_FIELDS.items()} == \
        {k: getattr(cm.OptProdigyState, k).offset for k in ("d", "d_max", "d_hat", "num", "den")}
    block = header[header.index("typedef struct avmoe_opt_prodigy_state"):header.index("} avmoe_opt_prodigy_state;")]
    assert [ln.split(";")[0].strip() for ln in block.splitlines()[1:]] == ["float d", "float d_max", "float d_hat", "int32_t reserved",
                                                                          "double num", "double den"]
    # no flag was added, the range and the state block are what they were
    assert (cm.OPT_CLIP | cm.OPT_SKIP_NONFINITE | cm.OPT_DECOUPLED_DECAY | cm.OPT_LR_SCHEDULE | cm.OPT_EMA | cm.OPT_REPORT | cm.OPT_SWA
            | cm.OPT_SWA_LR) == 255
    assert C.sizeof(cm.OptRange) == 48 and cm.OPT_STATE_BYTES == 64
    # the kernels exist once, under the names a trace shows
    src = open(_capi.HEADER_PATH.replace("include/avmoe.h", "avmoe_amd/csrc/opt_kernels.hip")).read()
    assert src.count("__global__ void __launch_bounds__(256) kk_opt_prodigy_update(") == 1
    assert src.count("__global__ void __launch_bounds__(256) kk_opt_prodigy_finalize(") == 1


def test_the_size_function_on_good_and_bad_counts():
    L = _capi.lib()
    lay = cm.OptProdigyLayout()
    for n_blocks in (0, 1, 5, 80, 4000):
        total = L.avmoe_opt_prodigy_bytes(n_blocks, C.byref(lay))
        assert lay.workspace_bytes % 16 == 0 and lay.block_bytes == 32
        assert lay.workspace_bytes == 16 * max(n_blocks, 1)                   # two doubles per block
        assert total == lay.workspace_bytes + lay.block_bytes and L.avmoe_opt_prodigy_bytes(n_blocks, None) == total
    lay.workspace_bytes = lay.block_bytes = 7
    for n_blocks in (-1, -5, 1 << 31):
        assert L.avmoe_opt_prodigy_bytes(n_blocks, C.byref(lay)) == 0 and "avmoe_opt_prodigy_bytes" in _err(), n_blocks
    assert lay.workspace_bytes == 7 and lay.block_bytes == 7                  # a refused call leaves the layout alone


def _calls():
    L = _capi.lib()
    raw, base = _buf(20480)
    table, state, shadows, hold, x0, s, block, ws = (base + 2048 * k for k in range(8))
    good = cm.OptProdigy(d0=1e-6, d_coef=1.0, growth=0.0, safeguard_warmup=0)

    def prodigy(table=table, state=state, flags=cm.OPT_CLIP, shadows=shadows, b1=0.9, b2=0.999, eps=1e-8, gs=1.0, n_ranges=2, n_blocks=2, hold=hold,
                x0=x0, s=s, consts=good, block=block, ws=ws):
        return L.avmoe_opt_prodigy_step(table, n_ranges, n_blocks, state, b1, b2, eps, gs, flags, None, shadows, hold, x0, s,
                                        None if consts is None else C.byref(consts), block, ws)

    def ema(table=table, state=state, flags=cm.OPT_CLIP, shadows=shadows, b1=0.9, b2=0.999, eps=1e-8, gs=1.0, n_ranges=2, n_blocks=2):
        return L.avmoe_opt_adam_step_ema(table, n_ranges, n_blocks, state, b1, b2, eps, gs, flags, None, shadows)

    def sam(table=table, state=state, flags=cm.OPT_CLIP, shadows=shadows, b1=0.9, b2=0.999, eps=1e-8, gs=1.0, n_ranges=2, n_blocks=2, hold=hold):
        return L.avmoe_opt_adam_step_sam(table, n_ranges, n_blocks, state, b1, b2, eps, gs, flags, None, shadows, hold)

    return raw, dict(table=table, state=state, shadows=shadows, hold=hold, x0=x0, s=s, block=block, ws=ws), prodigy, ema, sam


REFUSALS = [dict(state=None), dict(state=8), dict(table=None), dict(table=8), dict(n_ranges=-1), dict(n_blocks=-1),
            dict(b1=1.0), dict(b2=-0.1), dict(b1=float("nan")), dict(eps=-1.0), dict(eps=float("nan")), dict(gs=float("nan")),
            dict(flags=cm.OPT_CLIP | cm.OPT_REPORT), dict(flags=cm.OPT_SWA), dict(flags=cm.OPT_SWA_LR), dict(flags=256),
            dict(flags=cm.OPT_EMA, shadows=None), dict(flags=cm.OPT_EMA, shadows=4)]


def _resolve(kw, ptrs):
    """an integer for a pointer argument is an offset from the good pointer"""
    return {k: (ptrs[k] + v if k in ptrs and isinstance(v, int) else v) for k, v in kw.items()}


def test_prodigy_step_refuses_what_the_update_entry_points_refuse():
    """with hold: everything avmoe_opt_adam_step_sam refuses; without: everything avmoe_opt_adam_step_ema refuses -- the same status and,
    the function's name apart, the same message, before any launch (host pointers: a launch would fault)"""
    raw, ptrs, prodigy, ema, sam = _calls()
    for kw in REFUSALS:
        kw = _resolve(kw, ptrs)
        want = sam(**kw)
        assert want in (BAD_ARG, ALIGNMENT), kw
        msg = _err().replace("avmoe_opt_adam_step_sam", "")
        assert prodigy(**kw) == want, kw
        assert _err().replace("avmoe_opt_prodigy_step", "") == msg, kw
        want = ema(**kw)
        assert want in (BAD_ARG, ALIGNMENT), kw
        msg = _err().replace("avmoe_opt_adam_step_ema", "")
        assert prodigy(hold=None, **kw) == want, kw
        assert _err().replace("avmoe_opt_prodigy_step", "") == msg, kw
    assert prodigy(hold=ptrs["hold"] + 4) == ALIGNMENT and "hold" in _err()


BAD_CONSTS = [dict(d0=0.0), dict(d0=-1e-6), dict(d0=float("nan")), dict(d0=float("inf")), dict(d_coef=0.0), dict(d_coef=-1.0),
              dict(d_coef=float("nan")), dict(d_coef=float("inf")), dict(growth=0.5), dict(growth=-1.0), dict(growth=float("nan")),
              dict(growth=float("inf")), dict(safeguard_warmup=2), dict(safeguard_warmup=-1)]


def test_prodigy_step_refuses_its_own_arguments_before_any_launch():
    raw, ptrs, prodigy, ema, sam = _calls()
    for hold in (ptrs["hold"], None):
        for name in ("x0", "s", "consts", "block", "ws"):
            assert prodigy(hold=hold, **{name: None}) == BAD_ARG and "NULL" in _err(), name
        for kw in BAD_CONSTS:
            c = dict(d0=1e-6, d_coef=1.0, growth=0.0, safeguard_warmup=0)
            c.update(kw)
            assert prodigy(hold=hold, consts=cm.OptProdigy(**c)) == BAD_ARG and next(iter(kw)).split("_w")[0] in _err(), kw
        for name in ("x0", "s"):
            assert prodigy(hold=hold, **{name: ptrs[name] + 4}) == ALIGNMENT and "pointer array" in _err(), name
        for off in (4, 8, 12):
            assert prodigy(hold=hold, block=ptrs["block"] + off) == ALIGNMENT and "block" in _err(), off
        for off in (4, 2):
            assert prodigy(hold=hold, ws=ptrs["ws"] + off) == ALIGNMENT and "workspace" in _err(), off
        # NULL and bad constants come before alignment, and the shared checks before both
        assert prodigy(hold=hold, x0=None, block=ptrs["block"] + 4) == BAD_ARG
        assert prodigy(hold=hold, consts=cm.OptProdigy(d0=0.0, d_coef=1.0), ws=ptrs["ws"] + 4) == BAD_ARG
        assert prodigy(hold=hold, x0=None, eps=-1.0) == BAD_ARG and "eps" in _err()
    # good constants at their edges pass the checks: growth exactly 1, the safeguard on -- refused only for what follows them
    for c in (dict(growth=1.0), dict(growth=8.0), dict(safeguard_warmup=1), dict(d0=1.0, d_coef=0.5)):
        base = dict(d0=1e-6, d_coef=1.0, growth=0.0, safeguard_warmup=0)
        base.update(c)
        assert prodigy(consts=cm.OptProdigy(**base), ws=ptrs["ws"] + 4) == ALIGNMENT and "workspace" in _err(), c


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


BAD_CTOR = [dict(prodigy=1), dict(prodigy=None), dict(prodigy="yes"),
            dict(prodigy=True, prodigy_d0=0.0), dict(prodigy=True, prodigy_d0=-1.0), dict(prodigy=True, prodigy_d0=float("nan")),
            dict(prodigy=True, prodigy_d0=float("inf")), dict(prodigy=True, prodigy_d0=1e-60),
            dict(prodigy=True, prodigy_d_coef=0.0), dict(prodigy=True, prodigy_d_coef=float("nan")), dict(prodigy=True, prodigy_d_coef=-2.0),
            dict(prodigy=True, prodigy_growth=0.5), dict(prodigy=True, prodigy_growth=float("nan")), dict(prodigy=True, prodigy_growth=float("inf")),
            dict(prodigy=True, prodigy_safeguard_warmup=1), dict(prodigy=True, prodigy_safeguard_warmup=None),
            dict(prodigy_d0=1e-3), dict(prodigy_d_coef=2.0), dict(prodigy_growth=2.0), dict(prodigy_safeguard_warmup=True),
            dict(prodigy=True, trust_ratio=True), dict(prodigy=True, trust_ratio=True, trust_clip=10.0)]


@pytest.mark.parametrize("kw", BAD_CTOR, ids=[",".join(f"{k}={v}" for k, v in kw.items()) for kw in BAD_CTOR])
def test_bad_constructor_arguments_raise_value_error_before_anything_is_touched(kw):
    red, w, b = _reducer()
    ptrs = (w.data_ptr(), b.data_ptr())
    with pytest.raises(ValueError, match="prodigy"):
        FlatAdam(red, **kw)
    assert (w.data_ptr(), b.data_ptr()) == ptrs


def test_prodigy_selects_the_device_path():
    for kw in (dict(prodigy=True), dict(prodigy=True, prodigy_d0=1e-3, prodigy_d_coef=2.0, prodigy_growth=1.0, prodigy_safeguard_warmup=True)):
        red, w, b = _reducer()
        with pytest.raises(_capi.AvmoeError):                # a good value gets as far as the buckets: the device path has no CPU fallback
            FlatAdam(red, lr=1.0, **kw)
    sig = inspect.signature(FlatAdam.__init__).parameters
    assert sig["prodigy"].default is False and sig["prodigy_d0"].default == 1e-6 and sig["prodigy_d_coef"].default == 1.0
    assert sig["prodigy_growth"].default is None and sig["prodigy_safeguard_warmup"].default is False
    assert "Learning-rate estimation" in FlatAdam.__doc__ and "NO bias correction" in FlatAdam.__doc__
    assert FlatAdam._check_prodigy(True, 1e-6, 1.0, None, False) == (True, float(np.float32(1e-6)), 1.0, None, False)
    assert FlatAdam._check_prodigy(True, 0.1, 3, 1, True) == (True, float(np.float32(0.1)), 3.0, 1.0, True)
    assert FlatAdam._check_prodigy(False, 1e-6, 1.0, None, False)[0] is False
    for name in ("prodigy_d", "prodigy_d_hat", "prodigy_x0", "prodigy_s", "prodigy_d_next"):
        assert hasattr(FlatAdam, name), name


def test_the_hosts_copy_of_the_finalize_rule():
    f = FlatAdam.prodigy_d_next
    b2 = 0.999
    beta3 = float(np.float32(math.sqrt(float(np.float32(b2)))))
    # step 0 of a run: x = x0, the dot product is 0, d stays d0
    got = f(1e-6, 1e-6, 0.0, 0.0, 0.0, 5.0, np.float32(b2))
    assert got == {"d": 1e-6, "d_max": 1e-6, "d_hat": 0.0, "num": 0.0, "den": 5.0}
    # num = beta3 num + sum_dot in double; d_hat = fp32(d_coef num / den); d rises to it
    got = f(1.0, 1.0, 0.0, 2.0, 3.0, 0.5, np.float32(b2), d_coef=0.5)
    assert got["num"] == beta3 * 2.0 + 3.0 and got["den"] == 0.5
    assert got["d_hat"] == float(np.float32(0.5 * got["num"] / 0.5)) and got["d"] == got["d_max"] == got["d_hat"] > 1.0
    # growth limits the rise and d_max keeps the estimate; growth 1 freezes d
    got = f(1.0, 1.0, 0.0, 0.0, 100.0, 1.0, b2, growth=2.0)
    assert (got["d"], got["d_max"], got["d_hat"]) == (2.0, 100.0, 100.0)
    assert f(1.0, 1.0, 0.0, 0.0, 100.0, 1.0, b2, growth=1.0)["d"] == 1.0
    # a smaller or negative estimate never lowers d
    got = f(1.0, 1.0, 0.25, 0.0, -3.0, 1.0, b2)
    assert (got["d"], got["d_max"], got["d_hat"]) == (1.0, 1.0, -3.0)
    # den == 0, or a term that is not finite: d_hat stays as it is; num and den are written
    for sd, sa in ((1.0, 0.0), (float("inf"), 1.0), (float("nan"), 1.0), (1.0, float("inf")), (1e39, 1e-3)):
        got = f(1.0, 1.5, 0.25, 0.0, sd, sa, b2)
        assert (got["d"], got["d_max"], got["d_hat"]) == (1.5, 1.5, 0.25), (sd, sa)
        assert got["den"] == sa or math.isnan(sa)
