"""Host side of FlatAdam's averaged buffers (include/avmoe.h: avmoe_opt_buffer, avmoe_opt_buffer_table_bytes / _build, avmoe_opt_ema_buffers,
avmoe_opt_swap_buffers; avmoe_amd.train.FlatAdam(ema_buffers=...)): the symbols and the record layout the binding relies on, the argument
checks of both layers (they precede any launch, so host pointers and a NULL stream are enough and no GPU is needed), and the table image the
two host functions build."""
import ctypes as C
import struct

import pytest
import torch

from avmoe_amd import _capi
from avmoe_amd import _capi_moe as cm
from avmoe_amd.train import FlatAdam

BAD_ARG, ALIGNMENT, WORKSPACE = -1, -3, -4
NEW = ("avmoe_opt_buffer_table_bytes", "avmoe_opt_buffer_table_build", "avmoe_opt_ema_buffers", "avmoe_opt_swap_buffers")
LENGTHS = (1, 1024, 1025, 2049)


def _buf(nbytes):
    raw = C.create_string_buffer(nbytes + 64)
    return raw, (C.addressof(raw) + 63) & ~63


def _err():
    msg = _capi.lib().avmoe_last_error()
    return msg.decode() if msg else ""


def _records(lengths, base):
    """host records: buffer i one element into a 64-byte slot (4-byte aligned only), its shadow 16-byte aligned; the addresses are never
    dereferenced by the table functions"""
    recs = (cm.OptBuffer * len(lengths))()
    for i, n in enumerate(lengths):
        recs[i].buffer, recs[i].shadow, recs[i].n = base + 64 * i + 4, base + 4096 + 16 * i, n
    return recs


def test_header_declares_and_library_exports_the_buffer_entry_points():
    L = _capi.lib()
    for name in NEW:
        assert name in _capi.exported_symbols() and hasattr(L, name), name
    assert L.avmoe_abi_version() == 11
    header = open(_capi.HEADER_PATH).read()
    assert "typedef struct avmoe_opt_buffer" in header
    assert C.sizeof(cm.OptBuffer) == 24
    assert [(n, getattr(cm.OptBuffer, n).offset) for n, _ in cm.OptBuffer._fields_] == [("buffer", 0), ("shadow", 8), ("n", 16)]
    assert cm.OPT_STATE_FIELDS["ema_decay"] == (40, "float32") and cm.OPT_STATE_BYTES == 64      # what the new kernel reads: unchanged
    assert C.sizeof(cm.OptRange) == 48                        # the range table is what it was


def test_table_image_has_one_block_per_1024_elements_of_one_buffer():
    L = _capi.lib()
    raw, base = _buf(8192)
    recs = _records(LENGTHS, base)
    nb = C.c_int64(-1)
    nbytes = L.avmoe_opt_buffer_table_bytes(recs, len(LENGTHS), C.byref(nb))
    assert nb.value == 1 + 1 + 2 + 3
    assert nbytes == (16 + 24 * len(LENGTHS) + 8 * nb.value + 15) // 16 * 16         # header, records, map; rounded up to 16
    assert L.avmoe_opt_buffer_table_bytes(recs, len(LENGTHS), None) == nbytes          # the count is optional
    img = C.create_string_buffer(b"\xff" * (nbytes + 16), nbytes + 16)
    assert L.avmoe_opt_buffer_table_build(recs, len(LENGTHS), img, nbytes) == 0, _err()
    data = img.raw
    assert data[nbytes:] == b"\xff" * 16                      # nothing past the image
    magic, n_buffers, n_blocks = struct.unpack_from("<Iiq", data, 0)
    assert magic == int.from_bytes(b"BTPO", "little") and n_buffers == len(LENGTHS) and n_blocks == 7
    for i, n in enumerate(LENGTHS):
        assert struct.unpack_from("<QQq", data, 16 + 24 * i) == (recs[i].buffer, recs[i].shadow, n)
    bmap = [struct.unpack_from("<ii", data, 16 + 24 * len(LENGTHS) + 8 * b) for b in range(n_blocks)]
    assert bmap == [(0, 0), (1, 0), (2, 0), (2, 1), (3, 0), (3, 1), (3, 2)]
    # no buffers, and a buffer without elements: a table with no blocks
    assert L.avmoe_opt_buffer_table_bytes(None, 0, C.byref(nb)) == 16 and nb.value == 0
    assert L.avmoe_opt_buffer_table_build(None, 0, img, 16) == 0
    assert struct.unpack_from("<Iiq", img.raw, 0) == (magic, 0, 0)
    empty = _records((0, 5), base)
    assert L.avmoe_opt_buffer_table_bytes(empty, 2, C.byref(nb)) == 16 + 48 + 8 + 8 and nb.value == 1
    assert L.avmoe_opt_buffer_table_build(empty, 2, img, nbytes) == 0
    assert struct.unpack_from("<ii", img.raw, 16 + 48) == (1, 0)


def test_table_functions_refuse_bad_records():
    L = _capi.lib()
    raw, base = _buf(8192)
    img, nb = C.create_string_buffer(4096), C.c_int64(0)

    def both(recs, n, want, word):
        assert L.avmoe_opt_buffer_table_bytes(recs, n, C.byref(nb)) == 0 and word in _err(), _err()
        assert L.avmoe_opt_buffer_table_build(recs, n, img, 4096) == want and word in _err(), _err()

    both(_records(LENGTHS, base), -1, BAD_ARG, "negative")
    both(None, 2, BAD_ARG, "NULL")
    r = _records(LENGTHS, base); r[2].n = -5
    both(r, 4, BAD_ARG, "buffer 2")
    r = _records(LENGTHS, base); r[1].buffer = None
    both(r, 4, BAD_ARG, "buffer 1")
    r = _records(LENGTHS, base); r[3].shadow = None
    both(r, 4, BAD_ARG, "buffer 3")
    r = _records(LENGTHS, base); r[0].buffer = base + 2
    both(r, 4, ALIGNMENT, "4-byte")
    r = _records(LENGTHS, base); r[1].shadow = base + 4096 + 8
    both(r, 4, ALIGNMENT, "16-byte")
    good = _records(LENGTHS, base)
    need = L.avmoe_opt_buffer_table_bytes(good, 4, None)
    assert L.avmoe_opt_buffer_table_build(good, 4, None, need) == BAD_ARG and "image" in _err()
    assert L.avmoe_opt_buffer_table_build(good, 4, img, need - 1) == WORKSPACE and "needed" in _err()


def test_launch_validation_precedes_any_launch():
    """host pointers everywhere: a call that got as far as a launch would fault or fail, these all return an argument error first"""
    L = _capi.lib()
    raw, base = _buf(4096)
    table, state = base, base + 2048
    assert L.avmoe_opt_ema_buffers(None, 2, 2, state, None) == BAD_ARG and "table" in _err()
    assert L.avmoe_opt_ema_buffers(table, 2, 2, None, None) == BAD_ARG and "state" in _err()
    assert L.avmoe_opt_ema_buffers(table, 2, 2, state + 8, None) == BAD_ARG and "state" in _err()
    assert L.avmoe_opt_ema_buffers(table, -1, 2, state, None) == BAD_ARG and "count" in _err()
    assert L.avmoe_opt_ema_buffers(table, 2, -1, state, None) == BAD_ARG and "count" in _err()
    assert L.avmoe_opt_ema_buffers(table + 8, 2, 2, state, None) == ALIGNMENT and "aligned" in _err()
    assert L.avmoe_opt_ema_buffers(table, 0, 0, state, None) == 0            # nothing to do is no error, and no launch
    assert L.avmoe_opt_swap_buffers(None, 2, 2, None) == BAD_ARG and "table" in _err()
    assert L.avmoe_opt_swap_buffers(table, -1, 2, None) == BAD_ARG and "count" in _err()
    assert L.avmoe_opt_swap_buffers(table, 2, -1, None) == BAD_ARG and "count" in _err()
    assert L.avmoe_opt_swap_buffers(table + 4, 2, 2, None) == ALIGNMENT and "aligned" in _err()
    assert L.avmoe_opt_swap_buffers(table, 0, 0, None) == 0


def _reducer():
    from avmoe_amd.dp import AdapterGradReducer
    return AdapterGradReducer([torch.nn.Parameter(torch.zeros(7))])


class _Stats(torch.nn.Module):
    def __init__(self, **buffers):
        super().__init__()
        for k, v in buffers.items():
            self.register_buffer(k, v)


BAD_BUFFERS = {
    "float64": lambda: [("running_mean", torch.zeros(4, dtype=torch.float64))],
    "float16": lambda: [("running_mean", torch.zeros(4, dtype=torch.float16))],
    "bfloat16_in_a_module": lambda: _Stats(count=torch.zeros((), dtype=torch.int64), running_var=torch.ones(4, dtype=torch.bfloat16)),
    "not_contiguous": lambda: [("running_mean", torch.zeros(4, 6).t())],
    "strided": lambda: _Stats(running_mean=torch.zeros(8)[::2]),
    "another_device": lambda: [("running_mean", torch.zeros(4, device="meta"))],
}


@pytest.mark.parametrize("name", list(BAD_BUFFERS))
def test_bad_buffers_raise_value_error(name):
    with pytest.raises(ValueError, match="running_"):
        FlatAdam(_reducer(), ema_decay=0.9, ema_buffers=BAD_BUFFERS[name]())


def test_ema_buffers_needs_ema_decay_and_good_ones_reach_the_device_path():
    import inspect
    good = _Stats(running_mean=torch.zeros(4), num_batches_tracked=torch.zeros((), dtype=torch.int64))
    with pytest.raises(ValueError, match="ema_decay"):
        FlatAdam(_reducer(), ema_buffers=good)
    with pytest.raises(ValueError, match="ema_decay"):
        FlatAdam(_reducer(), max_grad_norm=1.0, ema_buffers=[("running_mean", torch.zeros(4))])
    with pytest.raises(_capi.AvmoeError):                    # good values get as far as the buckets: the device path has no CPU fallback
        FlatAdam(_reducer(), ema_decay=0.9, ema_buffers=good)
    assert inspect.signature(FlatAdam.__init__).parameters["ema_buffers"].default is None
    for name in ("ema_buffers", "ema_buffer_names"):
        assert isinstance(getattr(FlatAdam, name), property), name
