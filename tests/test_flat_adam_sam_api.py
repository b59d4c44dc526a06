"""Host side of sharpness-aware minimization in FlatAdam (include/avmoe.h: avmoe_opt_sam_state, avmoe_opt_sam_perturb,
avmoe_opt_adam_step_sam; avmoe_amd.train.FlatAdam(sam_rho=..., sam_adaptive=...), hold_bn_stats): the symbols and the layout the binding
relies on, the argument checks of both layers (they precede any launch, so host pointers and a NULL stream are enough and no GPU is
needed), and the BatchNorm context on torch's own modules."""
import ctypes as C
import inspect

import pytest
import torch

from avmoe_amd import _capi
from avmoe_amd import _capi_moe as cm
from avmoe_amd.train import FlatAdam, hold_bn_stats

BAD_ARG, ALIGNMENT = -1, -3


def _buf(nbytes):
    raw = C.create_string_buffer(nbytes + 64)
    return raw, (C.addressof(raw) + 63) & ~63


def _err():
    msg = _capi.lib().avmoe_last_error()
    return msg.decode() if msg else ""


def test_status_codes_are_the_headers():
    header = open(_capi.HEADER_PATH).read()
    assert f"AVMOE_ERR_BAD_ARG = {BAD_ARG}," in header and f"AVMOE_ERR_ALIGNMENT = {ALIGNMENT}," in header
    L = _capi.lib()
    raw, base = _buf(1024)
    assert L.avmoe_opt_swap_ema(None, 0, 0, base, None) == BAD_ARG               # a NULL table is the bad argument ...
    assert L.avmoe_opt_swap_ema(base + 4, 0, 0, base, None) == ALIGNMENT         # ... and a misaligned one the alignment error


def test_header_declares_and_library_exports_the_two_entry_points():
    L = _capi.lib()
    for name in ("avmoe_opt_sam_perturb", "avmoe_opt_adam_step_sam"):
        assert name in _capi.exported_symbols() and hasattr(L, name), name
    assert L.avmoe_abi_version() == 11
    header = open(_capi.HEADER_PATH).read()
    assert "typedef struct avmoe_opt_sam_state" in header
    assert C.sizeof(cm.OptSamState) == 16
    offs = [(n, getattr(cm.OptSamState, n).offset, getattr(cm.OptSamState, n).size) for n, _ in cm.OptSamState._fields_]
    assert offs == [("norm", 0, 4), ("scale", 4, 4), ("nonfinite", 8, 4), ("reserved", 12, 4)]
    block = header[header.index("typedef struct avmoe_opt_sam_state {"):header.index("} avmoe_opt_sam_state;")]
    pos = [block.index(line) for line in ("float norm;", "float scale;", "int32_t nonfinite;", "int32_t reserved;")]
    assert pos == sorted(pos)
    # no flag was added: 256 is nobody's
    assert (cm.OPT_CLIP | cm.OPT_SKIP_NONFINITE | cm.OPT_DECOUPLED_DECAY | cm.OPT_LR_SCHEDULE | cm.OPT_EMA | cm.OPT_REPORT | cm.OPT_SWA
            | cm.OPT_SWA_LR) == 255
    assert "= 256" not in header[header.index("optimizer with device-side state"):header.index("---- test hooks")]


def test_state_block_is_still_64_bytes_with_its_reserved_words():
    assert cm.OPT_STATE_BYTES == 64
    assert cm.OPT_STATE_FIELDS == {"total_norm": (0, "float32"), "clip_coef": (4, "float32"), "bc1": (8, "float32"), "bc2_sqrt": (12, "float32"),
                                   "applied_steps": (16, "int64"), "skipped_steps": (24, "int64"), "skip": (32, "int32"),
                                   "lr_factor": (36, "float32"), "ema_decay": (40, "float32")}
    header = open(_capi.HEADER_PATH).read()
    block = header[header.index("typedef struct avmoe_opt_state"):header.index("} avmoe_opt_state;")]
    assert "int32_t reserved[5];" in block
    lay = cm.OptLayout()
    raw, base = _buf(4096)
    r = (cm.OptRange * 1)()
    r[0].param, r[0].grad, r[0].exp_avg, r[0].exp_avg_sq, r[0].n, r[0].lr = base, base + 64, base + 128, base + 192, 4, 1e-3
    assert _capi.lib().avmoe_opt_workspace_bytes(r, 1, C.byref(lay)) > 0 and lay.state_bytes == 64


def test_perturb_validation_precedes_any_launch():
    """host pointers everywhere: a call that got as far as a launch would fault or fail, these all return an argument error first"""
    L = _capi.lib()
    raw, base = _buf(8192)
    table, partials, sam, hold = base, base + 1024, base + 2048, base + 4096

    def perturb(table=table, partials=partials, sam=sam, hold=hold, rho=0.05, adaptive=0, n_ranges=2, n_blocks=2, grad_scale=1.0):
        return L.avmoe_opt_sam_perturb(table, n_ranges, n_blocks, partials, sam, grad_scale, rho, adaptive, hold, None)

    # NULL pointers
    for kw in (dict(table=None), dict(partials=None), dict(sam=None), dict(hold=None)):
        assert perturb(**kw) == BAD_ARG and _err(), kw
    # rho negative, NaN, infinite
    for rho in (-0.1, -1e-30, float("nan"), float("inf"), float("-inf")):
        assert perturb(rho=rho) == BAD_ARG and "rho" in _err(), rho
    # adaptive is a 0 / 1 switch
    for adaptive in (2, -1, 256):
        assert perturb(adaptive=adaptive) == BAD_ARG and "adaptive" in _err(), adaptive
    # the sam block: 16-byte aligned, a bad argument like the state block's
    for off in (4, 8, 12):
        assert perturb(sam=sam + off) == BAD_ARG and "16-byte" in _err(), off
    # the hold array and the table: alignment errors
    assert perturb(hold=hold + 4) == ALIGNMENT and "hold" in _err()
    for off in (4, 8):
        assert perturb(table=table + off) == ALIGNMENT and "table" in _err(), off
    # what every launch refuses: negative counts, a NaN gradient scale
    assert perturb(n_ranges=-1) == BAD_ARG and perturb(n_blocks=-1) == BAD_ARG
    assert perturb(grad_scale=float("nan")) == BAD_ARG and "grad_scale" in _err()


def test_step_sam_refuses_what_step_ema_refuses_and_a_null_hold():
    L = _capi.lib()
    raw, base = _buf(8192)
    table, state, shadows, hold = base, base + 2048, base + 4096, base + 6144

    def ema_call(table=table, state=state, flags=cm.OPT_CLIP, shadows=shadows, b1=0.9, b2=0.999, eps=1e-8, gs=1.0, n_ranges=2, n_blocks=2, **_kw):
        return L.avmoe_opt_adam_step_ema(table, n_ranges, n_blocks, state, b1, b2, eps, gs, flags, None, shadows)

    def sam_call(table=table, state=state, flags=cm.OPT_CLIP, shadows=shadows, b1=0.9, b2=0.999, eps=1e-8, gs=1.0, n_ranges=2, n_blocks=2, hold=hold):
        return L.avmoe_opt_adam_step_sam(table, n_ranges, n_blocks, state, b1, b2, eps, gs, flags, None, shadows, hold)

    refusals = [dict(state=None), dict(state=state + 8), dict(table=None), dict(table=table + 8), dict(n_ranges=-1), dict(n_blocks=-1),
                dict(b1=1.0), dict(b2=-0.1), dict(b1=float("nan")), dict(eps=-1.0), dict(eps=float("nan")), dict(gs=float("nan")),
                dict(flags=cm.OPT_CLIP | cm.OPT_REPORT), dict(flags=cm.OPT_SWA), dict(flags=cm.OPT_SWA_LR), dict(flags=256),
                dict(flags=cm.OPT_EMA, shadows=None), dict(flags=cm.OPT_EMA, shadows=shadows + 4)]
    for kw in refusals:
        want = ema_call(**kw)
        assert want in (BAD_ARG, ALIGNMENT), kw
        msg = _err().replace("avmoe_opt_adam_step_ema", "")
        assert sam_call(**kw) == want, kw
        assert _err().replace("avmoe_opt_adam_step_sam", "") == msg, kw
    # without AVMOE_OPT_EMA the shadows may be NULL, the hold array never
    assert sam_call(hold=None) == BAD_ARG and "hold" in _err()
    assert sam_call(hold=None, shadows=None) == BAD_ARG and "hold" in _err()
    assert sam_call(hold=None, flags=cm.OPT_EMA) == BAD_ARG and "hold" in _err()
    assert sam_call(hold=hold + 4) == ALIGNMENT and "hold" in _err()
    # n_blocks == 0 launches nothing: the good call returns OK without a GPU
    assert sam_call(n_blocks=0, shadows=None) == 0
    assert L.avmoe_opt_adam_step_ema(table, 2, 0, state, 0.9, 0.999, 1e-8, 1.0, cm.OPT_CLIP, None, None) == 0


def test_the_older_entry_points_keep_their_refusals():
    """SAM got no flag: value 256 stays unknown everywhere, avmoe_opt_grad_norm_swa included"""
    L = _capi.lib()
    raw, base = _buf(8192)
    table, partials, state, shadows, report = base, base + 1024, base + 2048, base + 4096, base + 6144
    assert L.avmoe_opt_grad_norm_swa(table, 2, 2, partials, state, 1.0, 1.0, cm.OPT_CLIP | 256, 0.9, 0.999, None, None, None, report,
                                     None) == BAD_ARG and "unknown flag" in _err()
    assert L.avmoe_opt_adam_step(table, 2, 2, state, 0.9, 0.999, 1e-8, 1.0, 256, None) == BAD_ARG and "unknown flag" in _err()
    assert L.avmoe_opt_adam_step_ema(table, 2, 2, state, 0.9, 0.999, 1e-8, 1.0, 256, None, shadows) == BAD_ARG and "unknown flag" in _err()
    assert L.avmoe_opt_adam_step(table, 2, 2, state, 0.9, 0.999, 1e-8, 1.0, cm.OPT_EMA, None) == BAD_ARG and "unknown flag" in _err()


BAD_CTOR = [dict(sam_rho=-0.05), dict(sam_rho=float("nan")), dict(sam_rho=float("inf")), dict(sam_rho=float("-inf")), dict(sam_rho=1e39),
            dict(sam_adaptive=True), dict(sam_rho=None, sam_adaptive=True)]


@pytest.mark.parametrize("kw", BAD_CTOR, ids=[",".join(f"{k}={v}" for k, v in kw.items()) for kw in BAD_CTOR])
def test_bad_constructor_arguments_raise_value_error(kw):
    from avmoe_amd.dp import AdapterGradReducer
    red = AdapterGradReducer([torch.nn.Parameter(torch.zeros(7))])
    with pytest.raises(ValueError, match="sam_"):
        FlatAdam(red, **kw)


def test_sam_selects_the_device_path():
    from avmoe_amd.dp import AdapterGradReducer
    red = AdapterGradReducer([torch.nn.Parameter(torch.zeros(7))])
    for kw in (dict(sam_rho=0.05), dict(sam_rho=0.0), dict(sam_rho=0.5, sam_adaptive=True)):
        with pytest.raises(_capi.AvmoeError):                # a good value gets as far as the buckets: the device path has no CPU fallback
            FlatAdam(red, **kw)
    sig = inspect.signature(FlatAdam.__init__).parameters
    assert sig["sam_rho"].default is None and sig["sam_adaptive"].default is False
    assert "Sharpness-aware minimization" in FlatAdam.__doc__
    assert FlatAdam._check_sam(0.05, False) == (float(torch.tensor(0.05, dtype=torch.float32)), False)
    for name in ("sam_perturb", "sam_restore", "perturbed", "last_sam_norm", "last_sam_scale", "sam_nonfinite"):
        assert hasattr(FlatAdam, name), name


class _Net(torch.nn.Module):
    def __init__(self, momentum=0.1):
        super().__init__()
        self.a = torch.nn.BatchNorm1d(5, momentum=momentum)
        self.b = torch.nn.Sequential(torch.nn.Linear(5, 3), torch.nn.BatchNorm1d(3, momentum=0.3))

    def forward(self, x):
        return self.b(self.a(x))


def test_hold_bn_stats_on_torchs_own_batchnorm():
    torch.manual_seed(0)
    net = _Net().train()
    net(torch.randn(8, 5))                                   # the statistics have moved once
    before = {k: v.clone() for k, v in net.state_dict().items()}
    x = torch.randn(8, 5) * 3 + 1
    with hold_bn_stats(net) as inside:
        assert inside is net and net.a.momentum == 0.0 and net.b[1].momentum == 0.0
        held = net(x)
    assert net.a.momentum == 0.1 and net.b[1].momentum == 0.3
    for k, v in net.state_dict().items():
        if k.endswith("num_batches_tracked"):
            assert int(v) == int(before[k]) + 1, k           # the counter still advances, as torch's does
        else:
            assert torch.equal(v, before[k]), k
    free = net(x)                                            # the same batch outside: batch statistics normalise both alike
    assert torch.equal(held, free)
    assert not torch.equal(net.a.running_mean, before["a.running_mean"])
    with pytest.raises(KeyError):                            # restored when the body raises
        with hold_bn_stats(net):
            raise KeyError("backward failed")
    assert net.a.momentum == 0.1 and net.b[1].momentum == 0.3
    mixed = _Net()
    mixed.b[1].momentum = None
    with pytest.raises(ValueError, match="momentum=None"):
        with hold_bn_stats(mixed):
            pass
    assert mixed.a.momentum == 0.1 and mixed.b[1].momentum is None       # nothing was touched
