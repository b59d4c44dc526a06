"""Sinkhorn-balanced top-k routing, the part that needs no GPU: the two new symbols exported and declared under ABI 11, their ctypes
signatures, the workspace plan unchanged, every refusal of avmoe_moe_forward_sinkhorn / avmoe_router_sinkhorn that needs no launch, and the
facade: the sites' settings and their validation, the mutual exclusions, a library without the symbols, last_sinkhorn before any call."""
import ctypes as C
import os
import zlib

import pytest
import torch

from avmoe_amd import _capi
from avmoe_amd import _capi_moe as cm
from avmoe_amd import adapters
from avmoe_amd.train import RouterBiasBalancer, sinkhorn_scale, sinkhorn_topk
from oracle import avmoe_oracle as O
from tests.moe_gpu_util import make_desc
from tests.test_adapters_api import build_module
from tests.test_router_bias_api import PLAN_BEFORE
from tests.topk_families import FAMILIES, family_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("avmoe_moe_forward_sinkhorn", "avmoe_router_sinkhorn")
CFG = O.AdapterConfig(Cx=32, Nx=10, Cy=24, Ny=7, E_m=2, E_s=2, reduction=4, groups=2, K=4, variant="avs", lb_loss=True)
S = 6
ERR_BAD_ARG = -1                                      # AVMOE_ERR_BAD_ARG


def test_the_library_and_the_header_carry_the_new_symbols_under_abi_11():
    L = _capi.lib()
    syms = _capi.exported_symbols()
    for s in NEW:
        assert hasattr(L, s) and s in syms, s
    assert L.avmoe_abi_version() == 11 and L.avmoe_site_sinkhorn
    with open(os.path.join(ROOT, "include", "avmoe.h")) as f:
        head = f.read()
    assert all("int " + s + "(" in head for s in NEW)
    assert "#define AVMOE_ABI_VERSION 11\n" in head


def test_ctypes_signatures_are_registered():
    L = _capi.lib()
    assert L.avmoe_moe_forward_sinkhorn.restype is C.c_int and len(L.avmoe_moe_forward_sinkhorn.argtypes) == 20
    assert L.avmoe_moe_forward_sinkhorn.argtypes[5:8] == [C.c_int32] * 3
    assert L.avmoe_router_sinkhorn.restype is C.c_int
    assert L.avmoe_router_sinkhorn.argtypes == [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32] + [C.c_void_p] * 6


@pytest.mark.parametrize("family", list(FAMILIES))
def test_workspace_plan_is_the_one_before_the_feature(family):
    L = _capi.lib()
    cfg, S_, bf16 = family_config(family)
    d = make_desc(cfg, S_, bf16, True)
    table = cm.buffer_table(L, d)
    got = (L.avmoe_moe_saved_bytes(C.byref(d)), L.avmoe_moe_scratch_bytes(C.byref(d)), len(table), zlib.crc32(repr(table).encode()))
    assert got == PLAN_BEFORE[family]


def _forward_sinkhorn(L, d, ptrs, k, iters, X=C.c_void_p(8), out=C.c_void_p(8), saved=C.c_void_p(8)):
    one = C.c_void_p(8)                                   # never dereferenced: every call here fails before a launch
    return L.avmoe_moe_forward_sinkhorn(C.byref(d), X, one, C.byref(ptrs), None, k, 1, iters, None, out, one, one, one, None, None, one, one,
                                        saved, one, None)


def test_forward_sinkhorn_refusals_without_a_launch():
    L = _capi.lib()
    d = make_desc(CFG, S, False, True)
    ptrs = cm.MoePtrs()
    for k in (0, -1, CFG.E, CFG.E + 1):
        assert _forward_sinkhorn(L, d, ptrs, k, 3) == ERR_BAD_ARG and b"top_k" in L.avmoe_last_error(), k
    for n in (0, -1, 65, 1 << 20):
        assert _forward_sinkhorn(L, d, ptrs, 2, n) == ERR_BAD_ARG and b"iters" in L.avmoe_last_error(), n
    for kw in (dict(X=None), dict(out=None), dict(saved=None)):
        assert _forward_sinkhorn(L, d, ptrs, 2, 3, **kw) == ERR_BAD_ARG and b"null pointer" in L.avmoe_last_error()
    bad = make_desc(CFG, S, False, True)
    bad.E_m = bad.E_s = 0
    assert _forward_sinkhorn(L, bad, ptrs, 1, 3) != 0 and b"expert count" in L.avmoe_last_error()


def test_router_sinkhorn_refusals_without_a_launch():
    L = _capi.lib()
    one, far = C.c_void_p(1 << 20), C.c_void_p(1 << 30)
    call = lambda p, S_, E, k, n, w=far, v=far: L.avmoe_router_sinkhorn(p, S_, E, k, 1, n, None, w, None, None, v, None)
    assert call(None, 8, 4, 2, 3) == ERR_BAD_ARG and b"null pointer" in L.avmoe_last_error()
    assert call(one, 8, 4, 2, 3, v=None) == ERR_BAD_ARG and b"null pointer" in L.avmoe_last_error()
    for S_ in (0, -5, 1 << 31):
        assert call(one, S_, 4, 1, 3) == ERR_BAD_ARG and b"S " in L.avmoe_last_error(), S_
    for E in (0, 1, -1, 17):
        assert call(one, 8, E, 1, 3) == ERR_BAD_ARG and b"E " in L.avmoe_last_error(), E
    for k in (0, -1, 4, 5):
        assert call(one, 8, 4, k, 3) == ERR_BAD_ARG and b"top_k" in L.avmoe_last_error(), k
    for n in (0, -1, 65):
        assert call(one, 8, 4, 2, n) == ERR_BAD_ARG and b"iters" in L.avmoe_last_error(), n
    nbytes = 8 * 4 * 4
    for w in (one.value, one.value + 4, one.value + nbytes - 4, one.value - nbytes + 4):
        assert call(one, 8, 4, 2, 3, w=C.c_void_p(w)) == ERR_BAD_ARG and b"overlaps" in L.avmoe_last_error(), w


def test_settings_default_to_off_and_are_validated():
    torch.manual_seed(0)
    m = build_module("avs", CFG)
    keys = list(m.state_dict().keys())
    assert m.router_sinkhorn is None and m.router_sinkhorn_eval is False and m.last_sinkhorn is None
    for n in (1, 3, 64, None):
        m.router_sinkhorn = n
        assert m.router_sinkhorn == n
    for n in (0, -1, 65, 2.5, 3.0, True, "3"):
        with pytest.raises(ValueError, match="router_sinkhorn"):
            m.router_sinkhorn = n
    assert m.router_sinkhorn is None                      # a refused value leaves the setting alone
    m.router_sinkhorn_eval = 1
    assert m.router_sinkhorn_eval is True
    assert list(m.state_dict().keys()) == keys            # plain attributes: no parameter, no buffer, no key
    del m.__dict__["_router_sinkhorn"], m.__dict__["_router_sinkhorn_eval"]      # a module pickled before the settings existed
    assert m.router_sinkhorn is None and m.router_sinkhorn_eval is False
    opt_site = build_module("avs", CFG)
    opt_site.opt.router_sinkhorn, opt_site.opt.router_sinkhorn_eval = 4, True
    again = adapters.MoEAdapterAVS(input_dim=CFG.Cx, output_dim=CFG.Cx, adapter_kind="bottleneck", dim_list=None, layer_idx=0, opt=opt_site.opt,
                                   conv_dim_in=CFG.Ny, conv_dim_out=CFG.Nx, linear_in=CFG.Cy, linear_out=CFG.Cx, reduction_factor=CFG.reduction,
                                   use_bn=CFG.use_bn, use_gate=CFG.use_gate, num_tk=CFG.K)
    assert again.router_sinkhorn == 4 and again.router_sinkhorn_eval is True and again.last_sinkhorn is None


def _tokens():
    g = torch.Generator().manual_seed(0)
    return torch.randn(S, CFG.Cx, CFG.Nx, 1, generator=g), torch.randn(S, CFG.Cy, CFG.Ny, 1, generator=g)


def test_needs_top_k_and_excludes_the_other_balancers_before_anything_runs():
    torch.manual_seed(0)
    m = build_module("avs", CFG)
    x, y = _tokens()
    m.router_sinkhorn = 3
    for k in (None, CFG.E):                               # a dense mixture has no selection to balance
        m.router_top_k = k
        with pytest.raises(ValueError, match="router_top_k"):
            m(x, y, is_training=True)
    m.router_top_k = 2
    with pytest.raises(_capi.AvmoeError, match="GPU"):    # consistent settings: CPU tokens are then what is refused
        m(x, y, is_training=True)
    m.eval()
    with pytest.raises(_capi.AvmoeError, match="GPU"):
        m(x, y, is_training=False)
    m.train()
    m.router_expert_choice = 1
    with pytest.raises(ValueError):
        m(x, y, is_training=True)
    m.router_expert_choice = None
    bal = RouterBiasBalancer([m])
    with pytest.raises(ValueError, match="router_sinkhorn"):
        m(x, y, is_training=True)
    m.router_select_bias = None                           # the counts alone conflict too
    with pytest.raises(ValueError, match="router_sinkhorn"):
        m(x, y, is_training=False)
    bal.detach()
    with pytest.raises(_capi.AvmoeError, match="GPU"):
        m(x, y, is_training=True)
    assert m.last_sinkhorn is None


def test_a_library_without_the_symbols_is_refused(monkeypatch):
    torch.manual_seed(0)
    m = build_module("avs", CFG)
    m.router_top_k, m.router_sinkhorn = 2, 3
    x, y = _tokens()
    monkeypatch.setattr(_capi.lib(), "avmoe_site_sinkhorn", False, raising=False)
    with pytest.raises(_capi.AvmoeError, match="predates"):
        m(x, y, is_training=True)
    with pytest.raises(_capi.AvmoeError, match="predates"):
        sinkhorn_scale(torch.rand(8, 4), 3)
    with pytest.raises(_capi.AvmoeError, match="predates"):
        sinkhorn_topk(torch.rand(8, 4), 2, 3)
    monkeypatch.undo()
    with pytest.raises(_capi.AvmoeError, match="GPU"):    # with the symbols: a CPU tensor is what is refused
        sinkhorn_scale(torch.rand(8, 4), 3)
    with pytest.raises(_capi.AvmoeError, match="GPU"):
        sinkhorn_topk(torch.rand(8, 4), 2, 3)
