"""Host side of the optimizer with device-side state (include/avmoe.h: avmoe_opt_*): the entry points are declared and exported, every
argument error is reported before any launch (so host pointers are enough and no GPU is needed), and the workspace query grows with the
range list in 16-byte steps."""
import ctypes as C

import pytest

from avmoe_amd import _capi
from avmoe_amd import _capi_moe as cm

BAD_ARG, ALIGNMENT = -1, -3
NAMES = ("avmoe_opt_workspace_bytes", "avmoe_opt_table_build", "avmoe_opt_grad_norm", "avmoe_opt_adam_step")


def _buf(nbytes):
    """a 64-byte aligned host buffer (never dereferenced as device memory: validation comes first)"""
    raw = C.create_string_buffer(nbytes + 64)
    base = (C.addressof(raw) + 63) & ~63
    return raw, base


def _ranges(lengths, base, lr=1e-3, wd=0.0):
    arr = (cm.OptRange * len(lengths))()
    off = 0
    for r, n in zip(arr, lengths):
        r.param, r.grad, r.exp_avg, r.exp_avg_sq = base + off, base + off + 64, base + off + 128, base + off + 192
        r.n, r.lr, r.weight_decay = n, lr, wd
        off += 256
    return arr


def _err():
    msg = _capi.lib().avmoe_last_error()
    return msg.decode() if msg else ""


def test_header_declares_and_library_exports_the_entry_points():
    L = _capi.lib()
    declared = _capi.exported_symbols()
    for name in NAMES:
        assert name in declared, name
        assert hasattr(L, name), name
    assert L.avmoe_abi_version() == 11
    assert C.sizeof(cm.OptRange) == 48 and cm.OPT_STATE_BYTES == 64


def test_workspace_query_grows_with_the_ranges_and_is_16_byte_granular():
    L = _capi.lib()
    raw, base = _buf(1 << 16)
    prev_total, prev_table = 0, 0
    for lengths in ([1], [1, 2], [1, 2, 7], [1, 2, 7, 130], [1, 2, 7, 130, 5000], [1, 2, 7, 130, 5000, 1 << 20]):
        lay = cm.OptLayout()
        total = L.avmoe_opt_workspace_bytes(_ranges(lengths, base), len(lengths), C.byref(lay))
        assert total == lay.state_bytes + lay.table_bytes + lay.partial_bytes > 0
        assert lay.state_bytes == 64 and lay.state_bytes % 16 == 0 and lay.table_bytes % 16 == 0 and lay.partial_bytes % 16 == 0
        assert lay.n_blocks == sum(-(-n // 1024) for n in lengths)
        assert lay.table_bytes >= 16 + 48 * len(lengths) + 8 * lay.n_blocks and lay.partial_bytes >= 8 * lay.n_blocks
        assert total > prev_total and lay.table_bytes > prev_table
        prev_total, prev_table = total, lay.table_bytes
        assert L.avmoe_opt_workspace_bytes(_ranges(lengths, base), len(lengths), None) == total       # layout is optional
    assert L.avmoe_opt_workspace_bytes(None, 0, None) == 64 + 16 + 16                                  # an empty optimizer still has a state block


def test_table_image_lists_every_block_of_every_range():
    import struct
    L = _capi.lib()
    raw, base = _buf(1 << 16)
    lengths = [1, 2, 7, 130, 2500]
    rs = _ranges(lengths, base, lr=0.25, wd=0.5)
    lay = cm.OptLayout()
    L.avmoe_opt_workspace_bytes(rs, len(lengths), C.byref(lay))
    img = C.create_string_buffer(lay.table_bytes)
    assert L.avmoe_opt_table_build(rs, len(lengths), img, lay.table_bytes) == 0, _err()
    magic, n_ranges, n_blocks = struct.unpack_from("<Iiq", img.raw, 0)
    assert (n_ranges, n_blocks) == (5, 7)
    for i, n in enumerate(lengths):
        p, g, m, v, nn, lr, wd = struct.unpack_from("<QQQQqff", img.raw, 16 + 48 * i)
        assert (p, g, m, v, nn, lr, wd) == (rs[i].param, rs[i].grad, rs[i].exp_avg, rs[i].exp_avg_sq, n, 0.25, 0.5)
    blocks = [struct.unpack_from("<ii", img.raw, 16 + 48 * 5 + 8 * b) for b in range(7)]
    assert blocks == [(0, 0), (1, 0), (2, 0), (3, 0), (4, 0), (4, 1), (4, 2)]
    assert L.avmoe_opt_table_build(rs, len(lengths), img, lay.table_bytes - 16) == -4 and _err()       # AVMOE_ERR_WORKSPACE


def test_range_list_validation():
    L = _capi.lib()
    raw, base = _buf(4096)
    img = C.create_string_buffer(4096)
    lay = cm.OptLayout()

    def both(rs, n, want):
        assert L.avmoe_opt_workspace_bytes(rs, n, C.byref(lay)) == 0 and _err()
        assert L.avmoe_opt_table_build(rs, n, img, 4096) == want and _err()

    both(None, 2, BAD_ARG)                                  # NULL range list
    both(_ranges([4], base), -1, BAD_ARG)                   # negative range count
    both(_ranges([4, -1], base), 2, BAD_ARG)                # negative length
    for field in ("param", "grad", "exp_avg", "exp_avg_sq"):
        rs = _ranges([4, 4], base)
        setattr(rs[1], field, None)
        both(rs, 2, BAD_ARG)                                # NULL pointer in a range
        rs = _ranges([4, 4], base)
        setattr(rs[1], field, getattr(rs[1], field) + 4)
        both(rs, 2, ALIGNMENT)                              # a range that does not start 16-byte aligned
    assert L.avmoe_opt_table_build(_ranges([4], base), 1, None, 4096) == BAD_ARG and _err()


@pytest.mark.parametrize("entry", ["norm", "step"])
def test_launch_argument_validation_precedes_any_launch(entry):
    """host pointers everywhere: a call that got as far as a launch would fault or fail, these all return an argument error first"""
    L = _capi.lib()
    raw, base = _buf(4096)
    table, partials, state = base, base + 1024, base + 2048

    def call(table=table, partials=partials, state=state, n_ranges=2, n_blocks=2, max_norm=1.0, flags=cm.OPT_CLIP, b1=0.9, b2=0.999):
        if entry == "norm":
            return L.avmoe_opt_grad_norm(table, n_ranges, n_blocks, partials, state, 1.0, max_norm, flags, b1, b2, None)
        return L.avmoe_opt_adam_step(table, n_ranges, n_blocks, state, b1, b2, 1e-8, 1.0, flags, None)

    cases = [dict(table=None), dict(state=None), dict(n_ranges=-1), dict(n_blocks=-1), dict(state=state + 8), dict(b1=1.0), dict(b1=-0.1),
             dict(b2=1.0), dict(b2=float("nan")), dict(flags=64)]
    if entry == "norm":
        cases += [dict(max_norm=-1.0), dict(max_norm=float("nan")), dict(partials=None)]
    for kw in cases:
        assert call(**kw) == BAD_ARG, kw
        assert _err(), kw
    assert call(table=table + 8) == ALIGNMENT and _err()
    if entry == "norm":
        assert call(partials=partials + 4) == ALIGNMENT and _err()


def test_flat_adam_refuses_cpu_buckets_and_bad_options():
    """no CPU fallback on either path, and a negative clip threshold is an error at construction"""
    import torch
    from avmoe_amd.dp import AdapterGradReducer
    from avmoe_amd.train import FlatAdam
    p = torch.nn.Parameter(torch.zeros(7))
    red = AdapterGradReducer([p])
    with pytest.raises(_capi.AvmoeError):
        FlatAdam(red, max_grad_norm=1.0)
    with pytest.raises(ValueError):
        FlatAdam(red, max_grad_norm=-1.0)
