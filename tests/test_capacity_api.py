"""Expert capacity behind top-k routing, the part that needs no GPU: the two new symbols exported and declared under ABI 11, their ctypes
signatures, the workspace plan unchanged, every refusal of avmoe_moe_forward_capacity / avmoe_router_capacity that needs no launch, and
the facade: the sites' settings and their validation, router_capacity() in rationals, the mutual exclusions, a library without the
symbols, last_capacity before any call, and the CapacityMeter's arithmetic on reports made by hand."""
import ctypes as C
import os
import pickle
import zlib
from fractions import Fraction

import pytest
import torch

from avmoe_amd import _capi
from avmoe_amd import _capi_moe as cm
from avmoe_amd import adapters
from avmoe_amd.adapters import CapacityReport, router_capacity
from avmoe_amd.train import CapacityMeter, RouterBiasBalancer
from oracle import avmoe_oracle as O
from tests import capacity_ref as R
from tests.moe_gpu_util import make_desc
from tests.test_adapters_api import build_module
from tests.test_router_bias_api import PLAN_BEFORE
from tests.topk_families import FAMILIES, family_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("avmoe_moe_forward_capacity", "avmoe_router_capacity")
CFG = O.AdapterConfig(Cx=32, Nx=10, Cy=24, Ny=7, E_m=2, E_s=2, reduction=4, groups=2, K=4, variant="avs", lb_loss=True)
S = 6
ERR_BAD_ARG = -1                                      # AVMOE_ERR_BAD_ARG


def test_the_library_and_the_header_carry_the_new_symbols_under_abi_11():
    L = _capi.lib()
    syms = _capi.exported_symbols()
    for s in NEW:
        assert hasattr(L, s) and s in syms, s
    assert L.avmoe_abi_version() == 11 and L.avmoe_site_capacity is True
    with open(os.path.join(ROOT, "include", "avmoe.h")) as f:
        head = f.read()
    assert all("int " + s + "(" in head for s in NEW)
    assert "#define AVMOE_ABI_VERSION 11\n" in head
    assert "PER PAIR" in head                             # the header says what priority means for k > 1


def test_ctypes_signatures_are_registered():
    L = _capi.lib()
    f = L.avmoe_moe_forward_capacity
    assert f.restype is C.c_int and len(f.argtypes) == 25
    assert f.argtypes[5:7] == [C.c_int32] * 2 and f.argtypes[7:10] == [C.c_void_p] * 3 and f.argtypes[10:12] == [C.c_int32] * 2
    assert L.avmoe_router_capacity.restype is C.c_int
    assert L.avmoe_router_capacity.argtypes == [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_int32] + [C.c_void_p] * 9


@pytest.mark.parametrize("family", list(FAMILIES))
def test_workspace_plan_is_the_one_before_the_feature(family):
    L = _capi.lib()
    cfg, S_, bf16 = family_config(family)
    d = make_desc(cfg, S_, bf16, True)
    table = cm.buffer_table(L, d)
    got = (L.avmoe_moe_saved_bytes(C.byref(d)), L.avmoe_moe_scratch_bytes(C.byref(d)), len(table), zlib.crc32(repr(table).encode()))
    assert got == PLAN_BEFORE[family]
    rbw = next(b for n, _r, _o, b in table if n == "rbw")   # the forward keeps S + 32 words in this buffer of the router backward
    assert rbw >= 4 * (S_ + 32)


def _forward_capacity(L, d, ptrs, k, c, policy, cap_scale=C.c_void_p(8), X=C.c_void_p(8), out=C.c_void_p(8), saved=C.c_void_p(8)):
    one = C.c_void_p(8)                                   # never dereferenced: every call here fails before a launch
    return L.avmoe_moe_forward_capacity(C.byref(d), X, one, C.byref(ptrs), None, k, 1, None, None, None, c, policy, cap_scale, None, None, None,
                                        out, one, one, one, None, None, saved, one, None)


def test_forward_capacity_refusals_without_a_launch():
    L = _capi.lib()
    d = make_desc(CFG, S, False, True)
    ptrs = cm.MoePtrs()
    for k in (0, -1, CFG.E, CFG.E + 1):
        assert _forward_capacity(L, d, ptrs, k, 2, 0) == ERR_BAD_ARG and b"top_k" in L.avmoe_last_error(), k
    for c in (0, -1, S + 1, 1 << 20):
        assert _forward_capacity(L, d, ptrs, 2, c, 0) == ERR_BAD_ARG and b"capacity" in L.avmoe_last_error(), c
    for pol in (-1, 2, 7):
        assert _forward_capacity(L, d, ptrs, 2, 2, pol) == ERR_BAD_ARG and b"policy" in L.avmoe_last_error(), pol
    assert _forward_capacity(L, d, ptrs, 2, 2, 1, cap_scale=None) == ERR_BAD_ARG and b"cap_scale" in L.avmoe_last_error()
    for kw in (dict(X=None), dict(out=None), dict(saved=None)):
        assert _forward_capacity(L, d, ptrs, 2, 2, 0, **kw) == ERR_BAD_ARG and b"null pointer" in L.avmoe_last_error()


def test_router_capacity_refusals_without_a_launch():
    L = _capi.lib()
    one, far = C.c_void_p(1 << 20), C.c_void_p(1 << 30)
    call = lambda p, S_, E, k, c, pol, w=far: L.avmoe_router_capacity(p, S_, E, k, None, c, pol, None, w, None, None, None, None, None, None, None)
    assert call(None, 8, 4, 2, 2, 0) == ERR_BAD_ARG and b"null pointer" in L.avmoe_last_error()
    for S_ in (0, -5, 1 << 31):
        assert call(one, S_, 4, 1, 1, 0) == ERR_BAD_ARG and b"S " in L.avmoe_last_error(), S_
    for E in (0, 1, -1, 17):
        assert call(one, 8, E, 1, 1, 0) == ERR_BAD_ARG and b"E " in L.avmoe_last_error(), E
    for k in (0, -1, 4, 5):
        assert call(one, 8, 4, k, 1, 0) == ERR_BAD_ARG and b"top_k" in L.avmoe_last_error(), k
    for c in (0, -1, 9):
        assert call(one, 8, 4, 2, c, 0) == ERR_BAD_ARG and b"capacity" in L.avmoe_last_error(), c
    for pol in (-1, 2):
        assert call(one, 8, 4, 2, 2, pol) == ERR_BAD_ARG and b"policy" in L.avmoe_last_error(), pol
    nbytes = 8 * 4 * 4
    for w in (one.value, one.value + 4, one.value + nbytes - 4, one.value - nbytes + 4):
        assert call(one, 8, 4, 2, 2, 0, w=C.c_void_p(w)) == ERR_BAD_ARG and b"overlaps" in L.avmoe_last_error(), w


def test_router_capacity_in_rationals():
    assert router_capacity(1.25, 2, 7, 4) == 5            # 4.375 rounded up
    assert router_capacity(Fraction(5, 4), 2, 7, 4) == 5 and router_capacity(1, 2, 8, 4) == 4 and router_capacity(2, 1, 8, 4) == 4
    assert router_capacity(1e-9, 1, 7, 4) == 1 and router_capacity(50, 2, 7, 4) == 7      # the floors at 1 and S
    assert router_capacity(Fraction(1, 3), 3, 1 << 40, 1 << 3) == 1 << 37
    for f, k, S_, E in ((1.25, 2, 7, 4), (0.5, 1, 300, 16), (3, 2, 5, 16), (1.0, 1, 1, 2)):
        assert router_capacity(f, k, S_, E) == R.capacity(f, k, S_, E)


def test_settings_default_to_off_and_are_validated():
    torch.manual_seed(0)
    m = build_module("avs", CFG)
    keys = list(m.state_dict().keys())
    assert m.router_capacity_factor is None and m.router_capacity_policy == "order" and m.router_capacity_eval_factor is None
    assert m.last_capacity is None
    for name in ("router_capacity_factor", "router_capacity_eval_factor"):
        for f in (1, 1.25, 0.5, Fraction(5, 4), None):
            setattr(m, name, f)
            assert getattr(m, name) == f
        for f in (0, -1.0, float("inf"), float("nan"), True, "1.25", 1j):
            with pytest.raises(ValueError, match=name):
                setattr(m, name, f)
        assert getattr(m, name) is None                   # a refused value leaves the setting alone
    for v in ("priority", "order"):
        m.router_capacity_policy = v
        assert m.router_capacity_policy == v
    for v in ("random", 0, None, "Order"):
        with pytest.raises(ValueError, match="router_capacity_policy"):
            m.router_capacity_policy = v
    assert list(m.state_dict().keys()) == keys            # plain attributes: no parameter, no buffer, no key
    m.router_capacity_factor, m.router_capacity_policy, m.router_capacity_eval_factor = 1.5, "priority", 2.0
    back = pickle.loads(pickle.dumps(m))
    assert (back.router_capacity_factor, back.router_capacity_policy, back.router_capacity_eval_factor) == (1.5, "priority", 2.0)
    for kk in ("_router_capacity_factor", "_router_capacity_policy", "_router_capacity_eval_factor"):      # a module pickled before the settings existed
        del back.__dict__[kk]
    assert back.router_capacity_factor is None and back.router_capacity_policy == "order" and back.router_capacity_eval_factor is None
    assert back.last_capacity is None
    opt_site = build_module("avs", CFG)
    opt_site.opt.router_capacity_factor, opt_site.opt.router_capacity_policy, opt_site.opt.router_capacity_eval_factor = 1.25, "priority", 2
    again = adapters.MoEAdapterAVS(input_dim=CFG.Cx, output_dim=CFG.Cx, adapter_kind="bottleneck", dim_list=None, layer_idx=0, opt=opt_site.opt,
                                   conv_dim_in=CFG.Ny, conv_dim_out=CFG.Nx, linear_in=CFG.Cy, linear_out=CFG.Cx, reduction_factor=CFG.reduction,
                                   use_bn=CFG.use_bn, use_gate=CFG.use_gate, num_tk=CFG.K)
    assert (again.router_capacity_factor, again.router_capacity_policy, again.router_capacity_eval_factor) == (1.25, "priority", 2)


def _tokens():
    g = torch.Generator().manual_seed(0)
    return torch.randn(S, CFG.Cx, CFG.Nx, 1, generator=g), torch.randn(S, CFG.Cy, CFG.Ny, 1, generator=g)


def test_needs_top_k_and_excludes_choice_and_sinkhorn_before_anything_runs():
    torch.manual_seed(0)
    m = build_module("avs", CFG)
    x, y = _tokens()
    m.router_capacity_factor = 1.0
    for k in (None, CFG.E):                               # a dense mixture has no selection to bound
        m.router_top_k = k
        with pytest.raises(ValueError, match="router_top_k"):
            m(x, y, is_training=True)
    m.router_top_k = 2
    with pytest.raises(_capi.AvmoeError, match="GPU"):    # consistent settings: CPU tokens are then what is refused
        m(x, y, is_training=True)
    m.eval()
    with pytest.raises(_capi.AvmoeError, match="GPU"):
        m(x, y, is_training=False)
    m.router_top_k = None                                 # the settings are checked in eval mode too, whatever the eval factor
    with pytest.raises(ValueError, match="router_top_k"):
        m(x, y, is_training=False)
    m.router_top_k = 2
    m.train()
    m.router_sinkhorn = 3
    with pytest.raises(ValueError, match="router_sinkhorn"):
        m(x, y, is_training=True)
    m.router_sinkhorn = None
    m.router_top_k, m.router_expert_choice = None, 1
    with pytest.raises(ValueError):
        m(x, y, is_training=True)
    m.router_top_k = 2
    with pytest.raises(ValueError, match="router_expert_choice"):
        m(x, y, is_training=True)
    m.router_expert_choice = None
    bal = RouterBiasBalancer([m])                         # a selection bias and its counts combine with a capacity
    with pytest.raises(_capi.AvmoeError, match="GPU"):
        m(x, y, is_training=True)
    bal.detach()
    m.drop_path, m.expert_dropout, m.router_aux = 0.1, 0.2, True      # and so do the regularisers and the auxiliary losses
    with pytest.raises(_capi.AvmoeError, match="GPU"):
        m(x, y, is_training=True)
    assert m.last_capacity is None


def test_a_library_without_the_symbols_is_refused(monkeypatch):
    torch.manual_seed(0)
    m = build_module("avs", CFG)
    m.router_top_k, m.router_capacity_factor = 2, 1.0
    x, y = _tokens()
    monkeypatch.setattr(_capi.lib(), "avmoe_site_capacity", False, raising=False)
    with pytest.raises(_capi.AvmoeError, match="predates avmoe_moe_forward_capacity"):
        m(x, y, is_training=True)
    monkeypatch.undo()
    with pytest.raises(_capi.AvmoeError, match="GPU"):
        m(x, y, is_training=True)


def _report(c, demand, kept_count):
    i32 = lambda v: torch.tensor(v, dtype=torch.int32)
    return CapacityReport(c, torch.zeros(1, dtype=torch.int32), i32(demand), i32(kept_count))


def test_capacity_meter_arithmetic_on_hand_made_reports():
    a, b = build_module("avs", CFG), build_module("avs", CFG)
    with pytest.raises(ValueError):
        CapacityMeter([])
    meter = CapacityMeter([a, b])
    assert meter.overflow() == [None, None]
    meter.update(a, _report(3, [5, 3, 0, 4], [3, 3, 0, 3]))
    meter.update(0, _report(3, [7, 1, 0, 4], [3, 1, 0, 3]))
    meter.update(b, _report(2, [(1 << 31) - 1, 2, 2, 2], [2, 2, 2, 2]))
    meter.update(b, _report(2, [(1 << 31) - 1, 2, 2, 2], [2, 2, 2, 2]))      # int64 totals: two int32 maxima do not wrap
    assert meter.demand[0].dtype == torch.int64 and meter.demand[0].tolist() == [12, 4, 0, 8] and meter.kept[0].tolist() == [6, 4, 0, 6]
    assert meter.demand[1].tolist() == [(1 << 32) - 2, 4, 4, 4] and meter.calls == [2, 2]
    ov = meter.overflow()
    assert ov[0].tolist() == [0.5, 0.0, 0.0, 0.25]        # 0 where nothing selected the expert
    assert ov[1][0].item() == pytest.approx(1.0 - 4.0 / ((1 << 32) - 2)) and ov[1][1:].tolist() == [0.0, 0.0, 0.0]
    meter.reset()
    assert meter.demand[0].tolist() == [0] * 4 and meter.kept[1].tolist() == [0] * 4 and meter.calls == [0, 0]
    assert meter.overflow()[0].tolist() == [0.0] * 4
    assert a.__dict__["_capacity_meters"] == [meter]
    assert "_capacity_meters" not in pickle.loads(pickle.dumps(a)).__dict__      # per-process bookkeeping does not travel
    meter.close()
    assert a.__dict__["_capacity_meters"] == [] and b.__dict__["_capacity_meters"] == []
