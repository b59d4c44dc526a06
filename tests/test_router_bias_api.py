"""Aux-loss-free expert balancing, the part that needs no GPU: the new symbols in both libraries and both headers under ABI 11, the
workspace plan unchanged (the buffer table and avmoe_moe_saved_bytes of the four tests/topk_families.py shapes as they were before the
feature; the bias travels in the spare words of `mode`), every refusal of avmoe_moe_forward_bias / avmoe_router_bias_update that needs no
launch, and the facade: the sites' two plain attributes, RouterBiasBalancer's tables, its state_dict round trip, detach()."""
import ctypes as C
import math
import os
import zlib

import pytest
import torch

from avmoe_amd import _capi
from avmoe_amd import _capi_moe as cm
from avmoe_amd.train import RouterBiasBalancer
from oracle import avmoe_oracle as O
from tests.moe_gpu_util import make_desc
from tests.test_adapters_api import build_module
from tests.topk_families import FAMILIES, family_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("avmoe_moe_forward_bias", "avmoe_router_bias_update")
NEW_HOST = ("avmoe_host_moe_forward_bias", "avmoe_host_moe_backward_bias")
CFG = O.AdapterConfig(Cx=32, Nx=10, Cy=24, Ny=7, E_m=2, E_s=2, reduction=4, groups=2, K=4, variant="avs", lb_loss=True)
S = 6
ERR_BAD_ARG = -1                                      # AVMOE_ERR_BAD_ARG
# family -> (avmoe_moe_saved_bytes, avmoe_moe_scratch_bytes, buffers, crc32 of repr(buffer table)) of the commit before this feature
PLAN_BEFORE = {"tile_stream": (6846720, 357754112, 126, 3847475530), "tile_fast": (3256064, 16566272, 126, 3635936380),
               "tile_gen": (18749184, 183384320, 126, 2013049438), "tile_kernels": (792320, 16154368, 126, 781902942)}


def test_both_libraries_and_headers_carry_the_new_symbols_under_abi_11():
    from avmoe_amd import build as b
    L = _capi.lib()
    syms = _capi.exported_symbols()
    for s in NEW:
        assert hasattr(L, s) and s in syms, s
    assert L.avmoe_abi_version() == 11 and L.avmoe_site_bias
    H = C.CDLL(b.build_host(verbose=False))
    for s in NEW_HOST:
        assert hasattr(H, s), s
    with open(os.path.join(ROOT, "include", "avmoe.h")) as f:
        head = f.read()
    with open(os.path.join(ROOT, "include", "avmoe_host.h")) as f:
        host_head = f.read()
    assert all(s + "(" in head for s in NEW) and all(s + "(" in host_head for s in NEW_HOST)
    assert "#define AVMOE_ABI_VERSION 11\n" in head


def test_ctypes_signatures_are_registered():
    L = _capi.lib()
    assert L.avmoe_moe_forward_bias.restype is C.c_int and len(L.avmoe_moe_forward_bias.argtypes) == 19
    assert L.avmoe_moe_forward_bias.argtypes[5:7] == [C.c_int32, C.c_int32]
    assert L.avmoe_router_bias_update.restype is C.c_int
    assert L.avmoe_router_bias_update.argtypes == [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_float, C.c_void_p]


@pytest.mark.parametrize("family", list(FAMILIES))
def test_workspace_plan_is_the_one_before_the_feature(family):
    L = _capi.lib()
    cfg, S_, bf16 = family_config(family)
    d = make_desc(cfg, S_, bf16, True)
    table = cm.buffer_table(L, d)
    assert [n for n, _r, _o, _b in table[-4:]] == ["psm", "mode", "lse", "load"]
    assert dict((n, b) for n, _r, _o, b in table)["mode"] == 256          # 64 four-byte words: [0] k, [1] renorm, [2] bias used, [16, 32) its bits
    got = (L.avmoe_moe_saved_bytes(C.byref(d)), L.avmoe_moe_scratch_bytes(C.byref(d)), len(table), zlib.crc32(repr(table).encode()))
    assert got == PLAN_BEFORE[family]


def _forward_bias(L, d, ptrs, k, bias, count, X=C.c_void_p(8), out=C.c_void_p(8), saved=C.c_void_p(8)):
    one = C.c_void_p(8)                                   # never dereferenced: every call here fails before a launch
    return L.avmoe_moe_forward_bias(C.byref(d), X, one, C.byref(ptrs), None, k, 1, None, bias, count, out, one, one, one, None, None,
                                    saved, one, None)


def test_forward_bias_refusals_without_a_launch():
    L = _capi.lib()
    d = make_desc(CFG, S, False, True)
    ptrs = cm.MoePtrs()
    one = C.c_void_p(8)
    for k in (0, CFG.E):                                  # a dense mixture has no selection
        assert _forward_bias(L, d, ptrs, k, one, None) == ERR_BAD_ARG and b"select_bias" in L.avmoe_last_error()
        assert _forward_bias(L, d, ptrs, k, one, one) == ERR_BAD_ARG and b"select_bias" in L.avmoe_last_error()
    for k in (-1, CFG.E + 1):
        assert _forward_bias(L, d, ptrs, k, one, one) == ERR_BAD_ARG and b"top_k" in L.avmoe_last_error()
    for kw in (dict(X=None), dict(out=None), dict(saved=None)):
        assert _forward_bias(L, d, ptrs, 2, one, one, **kw) == ERR_BAD_ARG and b"null pointer" in L.avmoe_last_error()
    bad = make_desc(CFG, S, False, True)
    bad.E_m = bad.E_s = 0
    assert _forward_bias(L, bad, ptrs, 1, one, one) != 0 and b"expert count" in L.avmoe_last_error()


def test_bias_update_refusals_without_a_launch():
    L = _capi.lib()
    one = C.c_void_p(8)
    for args in ((None, one, one), (one, None, one), (one, one, None)):
        assert L.avmoe_router_bias_update(*args, 1, 1e-3, None) == ERR_BAD_ARG and b"null pointer" in L.avmoe_last_error()
    for n in (0, -3):
        assert L.avmoe_router_bias_update(one, one, one, n, 1e-3, None) == ERR_BAD_ARG and b"n_sites" in L.avmoe_last_error()
    for rate in (-1e-3, math.inf, -math.inf, math.nan):
        assert L.avmoe_router_bias_update(one, one, one, 1, rate, None) == ERR_BAD_ARG and b"rate" in L.avmoe_last_error()


def _sites():
    torch.manual_seed(0)
    a = build_module("avs", CFG)
    b = build_module("avs", O.AdapterConfig(Cx=32, Nx=10, Cy=24, Ny=7, E_m=1, E_s=1, reduction=4, groups=2, K=4, variant="avs"))
    return a, b


def test_sites_default_to_none_and_the_balancer_hands_out_rows():
    a, b = _sites()
    assert a.router_select_bias is None and a.router_select_count is None
    keys = [list(m.state_dict().keys()) for m in (a, b)]
    bufs = [[k for k, _ in m.named_buffers()] for m in (a, b)]
    bal = RouterBiasBalancer([a, b], rate=5e-3)
    assert bal.E == [4, 2] and bal.bias.shape == bal.counts.shape == (2, 16) and bal.E_table.dtype == torch.int32
    assert [list(m.state_dict().keys()) for m in (a, b)] == keys          # plain attributes: no parameter, no buffer, no key
    assert [[k for k, _ in m.named_buffers()] for m in (a, b)] == bufs
    for i, (m, e) in enumerate(zip((a, b), (4, 2))):
        assert m.router_select_bias.shape == (e,) and m.router_select_bias.data_ptr() == bal.bias[i].data_ptr()
        assert m.router_select_count.shape == (e,) and m.router_select_count.data_ptr() == bal.counts[i].data_ptr()
    assert all(float(l.sum()) == 0.0 for l in bal.loads())
    bal.counts[0, :4] = torch.tensor([3.0, 1.0, 0.0, 4.0])
    assert torch.equal(bal.loads()[0], torch.tensor([3.0, 1.0, 0.0, 4.0]) / 8) and float(bal.counts[0, :4].sum()) == 8.0      # not cleared
    with pytest.raises(_capi.AvmoeError):                 # no CPU fallback
        bal.step()
    bal.detach()
    assert all(m.router_select_bias is None and m.router_select_count is None for m in (a, b))


def test_balancer_state_dict_round_trip_and_refusals():
    a, b = _sites()
    bal = RouterBiasBalancer([a, b], rate=5e-3)
    bal.bias[0, :4] = torch.tensor([0.01, -0.02, 0.0, 0.03])
    bal.counts[1, :2] = torch.tensor([7.0, 5.0])
    sd = bal.state_dict()
    assert set(sd) == {"bias", "counts", "E", "rate"} and sd["E"] == [4, 2] and sd["rate"] == 5e-3
    a2, b2 = _sites()
    other = RouterBiasBalancer([a2, b2], rate=1e-3)
    view = a2.router_select_bias
    other.load_state_dict(sd)
    assert torch.equal(other.bias, bal.bias) and torch.equal(other.counts, bal.counts) and other.rate == 5e-3
    assert torch.equal(view, bal.bias[0, :4]) and a2.router_select_bias is view      # loaded in place: the sites' views follow
    with pytest.raises(ValueError):                       # another E list
        RouterBiasBalancer([b2, a2]).load_state_dict(sd)
    for rate in (-1.0, math.nan, math.inf, True, "x"):
        with pytest.raises(ValueError):
            RouterBiasBalancer([a], rate=rate)
    with pytest.raises(ValueError):
        RouterBiasBalancer([])


def test_a_library_without_the_symbols_is_refused(monkeypatch):
    a, _ = _sites()
    bal = RouterBiasBalancer([a])
    monkeypatch.setattr(_capi.lib(), "avmoe_site_bias", False, raising=False)
    with pytest.raises(_capi.AvmoeError, match="predates"):
        bal.step()
