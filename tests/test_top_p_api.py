"""Top-p routing, the part that needs no GPU: the two new symbols exported and declared under ABI 11, their ctypes signatures, the
workspace plan unchanged, every refusal of avmoe_moe_forward_top_p / avmoe_router_top_p that needs no launch, and the facade: the sites'
settings and their validation, the mutual exclusions, a library without the symbols, last_top_p before any call, pickling, and the
TopPMeter's arithmetic on reports made by hand."""
import ctypes as C
import os
import pickle
import zlib

import pytest
import torch

from avmoe_amd import _capi
from avmoe_amd import _capi_moe as cm
from avmoe_amd import adapters
from avmoe_amd.train import RouterBiasBalancer, TopPMeter, top_p_mask
from oracle import avmoe_oracle as O
from tests.moe_gpu_util import make_desc
from tests.test_adapters_api import build_module
from tests.test_router_bias_api import PLAN_BEFORE
from tests.topk_families import FAMILIES, family_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("avmoe_moe_forward_top_p", "avmoe_router_top_p")
CFG = O.AdapterConfig(Cx=32, Nx=10, Cy=24, Ny=7, E_m=2, E_s=2, reduction=4, groups=2, K=4, variant="avs", lb_loss=True)
S = 6
ERR_BAD_ARG = -1                                      # AVMOE_ERR_BAD_ARG
NAN = float("nan")


def test_the_library_and_the_header_carry_the_new_symbols_under_abi_11():
    L = _capi.lib()
    syms = _capi.exported_symbols()
    for s in NEW:
        assert hasattr(L, s) and s in syms, s
    assert L.avmoe_abi_version() == 11 and L.avmoe_site_top_p is True
    with open(os.path.join(ROOT, "include", "avmoe.h")) as f:
        head = f.read()
    assert all("int " + s + "(" in head for s in NEW)
    assert "#define AVMOE_ABI_VERSION 11\n" in head


def test_ctypes_signatures_are_registered():
    L = _capi.lib()
    assert L.avmoe_moe_forward_top_p.restype is C.c_int and len(L.avmoe_moe_forward_top_p.argtypes) == 22
    assert L.avmoe_moe_forward_top_p.argtypes[5:9] == [C.c_float, C.c_int32, C.c_int32, C.c_int32]
    assert L.avmoe_router_top_p.restype is C.c_int
    assert L.avmoe_router_top_p.argtypes == [C.c_void_p, C.c_int64, C.c_int32, C.c_float, C.c_int32, C.c_int32, C.c_int32] + [C.c_void_p] * 6


@pytest.mark.parametrize("family", list(FAMILIES))
def test_workspace_plan_is_the_one_before_the_feature(family):
    L = _capi.lib()
    cfg, S_, bf16 = family_config(family)
    d = make_desc(cfg, S_, bf16, True)
    table = cm.buffer_table(L, d)
    got = (L.avmoe_moe_saved_bytes(C.byref(d)), L.avmoe_moe_scratch_bytes(C.byref(d)), len(table), zlib.crc32(repr(table).encode()))
    assert got == PLAN_BEFORE[family]


def _forward_top_p(L, d, ptrs, P, k_min, k_max, X=C.c_void_p(8), out=C.c_void_p(8), saved=C.c_void_p(8)):
    one = C.c_void_p(8)                                   # never dereferenced: every call here fails before a launch
    return L.avmoe_moe_forward_top_p(C.byref(d), X, one, C.byref(ptrs), None, P, k_min, k_max, 1, None, out, one, one, one, None, None, one,
                                     one, one, saved, one, None)


def test_forward_top_p_refusals_without_a_launch():
    L = _capi.lib()
    d = make_desc(CFG, S, False, True)
    ptrs = cm.MoePtrs()
    E = CFG.E
    for P in (0.0, -0.5, 1.0000001, 2.0, NAN, float("inf"), -0.0):
        assert _forward_top_p(L, d, ptrs, P, 1, E) == ERR_BAD_ARG and b"top_p" in L.avmoe_last_error(), P
    for k in (0, -1, E + 1):
        assert _forward_top_p(L, d, ptrs, 0.9, k, E) == ERR_BAD_ARG and b"k_min" in L.avmoe_last_error(), k
        assert _forward_top_p(L, d, ptrs, 0.9, 1, k) == ERR_BAD_ARG and b"k_max" in L.avmoe_last_error(), k
    assert _forward_top_p(L, d, ptrs, 0.9, 3, 2) == ERR_BAD_ARG and b"above k_max" in L.avmoe_last_error()
    for kw in (dict(X=None), dict(out=None), dict(saved=None)):
        assert _forward_top_p(L, d, ptrs, 0.9, 1, E, **kw) == ERR_BAD_ARG and b"null pointer" in L.avmoe_last_error()
    one_expert = make_desc(CFG, S, False, True)
    one_expert.E_m, one_expert.E_s = 1, 0
    assert _forward_top_p(L, one_expert, ptrs, 0.9, 1, 1) == ERR_BAD_ARG and b"E 1 not in [2, 16]" in L.avmoe_last_error()
    bad = make_desc(CFG, S, False, True)
    bad.E_m = bad.E_s = 0
    assert _forward_top_p(L, bad, ptrs, 0.9, 1, 1) != 0 and b"expert count" in L.avmoe_last_error()


def test_router_top_p_refusals_without_a_launch():
    L = _capi.lib()
    one, far = C.c_void_p(1 << 20), C.c_void_p(1 << 30)
    call = lambda p, S_, E, P, k_min, k_max, w=far: L.avmoe_router_top_p(p, S_, E, P, k_min, k_max, 1, None, w, None, None, None, None)
    assert call(None, 8, 4, 0.9, 1, 4) == ERR_BAD_ARG and b"null pointer" in L.avmoe_last_error()
    for S_ in (0, -5, 1 << 31):
        assert call(one, S_, 4, 0.9, 1, 4) == ERR_BAD_ARG and b"S " in L.avmoe_last_error(), S_
    for E in (0, 1, -1, 17):
        assert call(one, 8, E, 0.9, 1, 1) == ERR_BAD_ARG and b"E " in L.avmoe_last_error(), E
    for P in (0.0, -1.0, 1.5, NAN, -NAN):
        assert call(one, 8, 4, P, 1, 4) == ERR_BAD_ARG and b"top_p" in L.avmoe_last_error(), P
    for k in (0, -1, 5):
        assert call(one, 8, 4, 0.9, k, 4) == ERR_BAD_ARG and b"k_min" in L.avmoe_last_error(), k
        assert call(one, 8, 4, 0.9, 1, k) == ERR_BAD_ARG and b"k_max" in L.avmoe_last_error(), k
    assert call(one, 8, 4, 0.9, 4, 3) == ERR_BAD_ARG and b"above k_max" in L.avmoe_last_error()
    nbytes = 8 * 4 * 4
    for w in (one.value, one.value + 4, one.value + nbytes - 4, one.value - nbytes + 4):
        assert call(one, 8, 4, 0.9, 1, 4, w=C.c_void_p(w)) == ERR_BAD_ARG and b"overlaps" in L.avmoe_last_error(), w


def test_settings_default_to_off_are_validated_and_pickle():
    torch.manual_seed(0)
    m = build_module("avs", CFG)
    keys = list(m.state_dict().keys())
    assert m.router_top_p is None and m.router_top_p_min_k == 1 and m.last_top_p is None
    for p in (1e-30, 0.5, 0.95, 1, 1.0, None):
        m.router_top_p = p
        assert m.router_top_p == p and (p is None or isinstance(m.router_top_p, float))
    for p in (0, 0.0, -0.1, 1.0000001, 2, NAN, float("inf"), True, "0.9", 1e-60):      # (1e-60 is 0 in fp32, the number format of the call)
        with pytest.raises(ValueError, match="router_top_p"):
            m.router_top_p = p
    assert m.router_top_p is None                         # a refused value leaves the setting alone
    for k in (1, 2, 16):
        m.router_top_p_min_k = k
        assert m.router_top_p_min_k == k
    for k in (0, -1, 1.5, 2.0, True, None, "2"):
        with pytest.raises(ValueError, match="router_top_p_min_k"):
            m.router_top_p_min_k = k
    assert m.router_top_p_min_k == 16
    assert list(m.state_dict().keys()) == keys            # plain attributes: no parameter, no buffer, no key
    m.router_top_p, m.router_top_p_min_k = 0.9, 2
    back = pickle.loads(pickle.dumps(m))
    assert (back.router_top_p, back.router_top_p_min_k) == (0.9, 2) and back.last_top_p is None
    del back.__dict__["_router_top_p"], back.__dict__["_router_top_p_min_k"]      # a module pickled before the settings existed
    assert back.router_top_p is None and back.router_top_p_min_k == 1
    opt_site = build_module("avs", CFG)
    opt_site.opt.router_top_p, opt_site.opt.router_top_p_min_k = 0.75, 2
    again = adapters.MoEAdapterAVS(input_dim=CFG.Cx, output_dim=CFG.Cx, adapter_kind="bottleneck", dim_list=None, layer_idx=0, opt=opt_site.opt,
                                   conv_dim_in=CFG.Ny, conv_dim_out=CFG.Nx, linear_in=CFG.Cy, linear_out=CFG.Cx, reduction_factor=CFG.reduction,
                                   use_bn=CFG.use_bn, use_gate=CFG.use_gate, num_tk=CFG.K)
    assert again.router_top_p == 0.75 and again.router_top_p_min_k == 2 and again.last_top_p is None


def _tokens():
    g = torch.Generator().manual_seed(0)
    return torch.randn(S, CFG.Cx, CFG.Nx, 1, generator=g), torch.randn(S, CFG.Cy, CFG.Ny, 1, generator=g)


def test_excludes_the_other_selection_stages_before_anything_runs():
    torch.manual_seed(0)
    m = build_module("avs", CFG)
    x, y = _tokens()
    m.router_top_p = 0.9
    for k in (None, 2, CFG.E):                            # with or without a k_max: consistent settings, CPU tokens are then what is refused
        m.router_top_k = k
        for training in (True, False):
            m.train(training)
            with pytest.raises(_capi.AvmoeError, match="GPU"):
                m(x, y, is_training=training)
    m.train()
    m.router_top_k, m.router_top_p_min_k = 2, 3           # k_min above k_max
    with pytest.raises(ValueError, match="router_top_p_min_k"):
        m(x, y, is_training=True)
    m.router_top_k, m.router_top_p_min_k = None, CFG.E + 1
    with pytest.raises(ValueError, match="router_top_p_min_k"):
        m(x, y, is_training=True)
    m.router_top_p_min_k = 1
    m.router_expert_choice = 1
    with pytest.raises(ValueError, match="router_top_p does not combine with router_expert_choice"):
        m(x, y, is_training=True)
    m.router_expert_choice = None
    m.router_top_k, m.router_sinkhorn = 2, 3
    with pytest.raises(ValueError, match="router_top_p does not combine with router_sinkhorn"):
        m(x, y, is_training=True)
    m.eval()                                              # (reported in eval mode too, where Sinkhorn itself would be off)
    with pytest.raises(ValueError, match="router_top_p does not combine with router_sinkhorn"):
        m(x, y, is_training=False)
    m.train()
    m.router_sinkhorn = None
    m.router_capacity_factor = 1.5
    with pytest.raises(ValueError, match="router_top_p does not combine with router_capacity_factor"):
        m(x, y, is_training=True)
    m.router_capacity_factor = None
    bal = RouterBiasBalancer([m])
    with pytest.raises(ValueError, match="router_top_p does not combine with router_select_bias"):
        m(x, y, is_training=True)
    m.router_select_bias = None                           # the counts alone conflict too
    with pytest.raises(ValueError, match="router_top_p does not combine with router_select_bias"):
        m(x, y, is_training=False)
    bal.detach()
    with pytest.raises(_capi.AvmoeError, match="GPU"):
        m(x, y, is_training=True)
    assert m.last_top_p is None


def test_a_library_without_the_symbols_is_refused(monkeypatch):
    torch.manual_seed(0)
    m = build_module("avs", CFG)
    m.router_top_p = 0.9
    x, y = _tokens()
    monkeypatch.setattr(_capi.lib(), "avmoe_site_top_p", False, raising=False)
    with pytest.raises(_capi.AvmoeError, match="predates"):
        m(x, y, is_training=True)
    with pytest.raises(_capi.AvmoeError, match="predates"):
        top_p_mask(torch.rand(8, 4), 0.9)
    monkeypatch.undo()
    with pytest.raises(_capi.AvmoeError, match="GPU"):    # with the symbols: a CPU tensor is what is refused
        top_p_mask(torch.rand(8, 4), 0.9)


def test_top_p_meter_totals_and_means():
    torch.manual_seed(0)
    a, b = build_module("avs", CFG), build_module("avs", CFG)
    with pytest.raises(ValueError, match="no sites"):
        TopPMeter([])
    meter = TopPMeter([a, b])
    assert meter.mean_experts() == [None, None]
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32)
    rep = adapters.TopPReport(i32(1, 3, 15, 1), i32(4, 2, 1, 1), i32(0, 2, 1, 0, 1))      # 4 frames: k = 1, 2, 4, 1 -> 8 slots
    meter.update(a, rep)
    meter.update(0, rep)
    big = adapters.TopPReport(i32(0), i32((1 << 31) - 1, 0, 0, 0), i32(0, (1 << 31) - 1, 0, 0, 0))
    meter.update(b, big)
    meter.update(b, big)                                  # the totals are int64: two such calls do not wrap
    assert meter.calls == [2, 2]
    assert meter.khist[0].tolist() == [0, 4, 2, 0, 2] and meter.count[0].tolist() == [8, 4, 2, 2]
    assert meter.count[1][0].item() == (1 << 32) - 2
    assert meter.mean_experts() == [2.0, 1.0]
    meter.reset()
    assert meter.khist[0].tolist() == [0] * 5 and meter.count[1].tolist() == [0] * 4 and meter.calls == [0, 0]
    assert meter.mean_experts() == [None, None]
    assert a.__dict__["_top_p_meters"] == [meter]
    assert "_top_p_meters" not in pickle.loads(pickle.dumps(a)).__dict__      # per-process bookkeeping does not travel
    meter.close()
    assert a.__dict__["_top_p_meters"] == [] and b.__dict__["_top_p_meters"] == []
