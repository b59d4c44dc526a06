"""Expert-choice gating, the part that needs no GPU: the two new symbols exported and declared under ABI 11, their ctypes signatures,
every refusal of avmoe_moe_forward_choice / avmoe_expert_choice that needs no launch, and the facade: the sites' settings and their
validation, the capacity rule, the mutual exclusions, a library without the symbols."""
import ctypes as C
import math
import os
from fractions import Fraction

import pytest
import torch

from avmoe_amd import _capi
from avmoe_amd import _capi_moe as cm
from avmoe_amd import adapters
from avmoe_amd.train import RouterBiasBalancer, expert_choice_mask
from oracle import avmoe_oracle as O
from tests import expert_choice_ref as R
from tests.moe_gpu_util import make_desc
from tests.test_adapters_api import build_module

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("avmoe_moe_forward_choice", "avmoe_expert_choice")
CFG = O.AdapterConfig(Cx=32, Nx=10, Cy=24, Ny=7, E_m=2, E_s=2, reduction=4, groups=2, K=4, variant="avs", lb_loss=True)
S = 6
ERR_BAD_ARG = -1                                      # AVMOE_ERR_BAD_ARG


def test_the_library_and_the_header_carry_the_new_symbols_under_abi_11():
    L = _capi.lib()
    syms = _capi.exported_symbols()
    for s in NEW:
        assert hasattr(L, s) and s in syms, s
    assert L.avmoe_abi_version() == 11 and L.avmoe_site_choice
    with open(os.path.join(ROOT, "include", "avmoe.h")) as f:
        head = f.read()
    assert all("int " + s + "(" in head for s in NEW)
    assert "#define AVMOE_ABI_VERSION 11\n" in head


def test_ctypes_signatures_are_registered():
    L = _capi.lib()
    assert L.avmoe_moe_forward_choice.restype is C.c_int and len(L.avmoe_moe_forward_choice.argtypes) == 18
    assert L.avmoe_moe_forward_choice.argtypes[5:7] == [C.c_int32, C.c_int32]
    assert L.avmoe_expert_choice.restype is C.c_int
    assert L.avmoe_expert_choice.argtypes == [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32] + [C.c_void_p] * 6


def _forward_choice(L, d, ptrs, capacity, X=C.c_void_p(8), out=C.c_void_p(8), saved=C.c_void_p(8)):
    one = C.c_void_p(8)                                   # never dereferenced: every call here fails before a launch
    return L.avmoe_moe_forward_choice(C.byref(d), X, one, C.byref(ptrs), None, capacity, 0, None, out, one, one, one, None, None, one,
                                      saved, one, None)


def test_forward_choice_refusals_without_a_launch():
    L = _capi.lib()
    d = make_desc(CFG, S, False, True)
    ptrs = cm.MoePtrs()
    for c in (0, -1, S + 1, 1 << 30):
        assert _forward_choice(L, d, ptrs, c) == ERR_BAD_ARG and b"capacity" in L.avmoe_last_error(), c
    for kw in (dict(X=None), dict(out=None), dict(saved=None)):
        assert _forward_choice(L, d, ptrs, 2, **kw) == ERR_BAD_ARG and b"null pointer" in L.avmoe_last_error()
    bad = make_desc(CFG, S, False, True)
    bad.E_m = bad.E_s = 0
    assert _forward_choice(L, bad, ptrs, 1) != 0 and b"expert count" in L.avmoe_last_error()


def test_expert_choice_refusals_without_a_launch():
    L = _capi.lib()
    one = C.c_void_p(8)
    call = lambda p, S_, E, c: L.avmoe_expert_choice(p, S_, E, c, 0, None, one, one, one, one, None)
    assert call(None, 8, 4, 2) == ERR_BAD_ARG and b"null pointer" in L.avmoe_last_error()
    for S_ in (0, -5):
        assert call(one, S_, 4, 1) == ERR_BAD_ARG and b"S " in L.avmoe_last_error()
    for E in (0, -1, 17):
        assert call(one, 8, E, 2) == ERR_BAD_ARG and b"E " in L.avmoe_last_error()
    for c in (0, -1, 9):
        assert call(one, 8, 4, c) == ERR_BAD_ARG and b"capacity" in L.avmoe_last_error()


def test_settings_default_to_off_and_are_validated():
    torch.manual_seed(0)
    m = build_module("avs", CFG)
    keys = list(m.state_dict().keys())
    assert m.router_expert_choice is None and m.router_expert_choice_renorm is False and m.last_expert_choice is None
    for k in (1, 2, 4, 1.5, 0.25, Fraction(3, 2), None):
        m.router_expert_choice = k
        assert m.router_expert_choice == k
    for k in (0, -1, 4.5, 5, True, "2", math.nan, math.inf):
        with pytest.raises(ValueError, match="router_expert_choice"):
            m.router_expert_choice = k
    assert m.router_expert_choice is None                 # a refused value leaves the setting alone
    m.router_expert_choice_renorm = 1
    assert m.router_expert_choice_renorm is True
    assert list(m.state_dict().keys()) == keys            # plain attributes: no parameter, no buffer, no key
    opt_site = build_module("avs", CFG)
    opt_site.opt.router_expert_choice, opt_site.opt.router_expert_choice_renorm = 2, True
    again = adapters.MoEAdapterAVS(input_dim=CFG.Cx, output_dim=CFG.Cx, adapter_kind="bottleneck", dim_list=None, layer_idx=0, opt=opt_site.opt,
                                   conv_dim_in=CFG.Ny, conv_dim_out=CFG.Nx, linear_in=CFG.Cy, linear_out=CFG.Cx, reduction_factor=CFG.reduction,
                                   use_bn=CFG.use_bn, use_gate=CFG.use_gate, num_tk=CFG.K)
    assert again.router_expert_choice == 2 and again.router_expert_choice_renorm is True


def test_capacity_is_evaluated_exactly():
    cap = adapters.expert_choice_capacity
    assert [cap(k, S_, E) for k, S_, E in ((1, 300, 4), (2, 3, 4), (0.5, 3, 4), (4, 7, 4), (1, 1, 16), (1.5, 10, 4), (Fraction(1, 3), 9, 3))] \
        == [75, 2, 1, 7, 1, 4, 1]
    assert cap(0.1, 10, 1) == 2                           # Fraction(0.1) is a hair above 1 / 10: the ceiling is taken of the exact product
    assert cap(Fraction(1, 10), 10, 1) == 1
    for k, S_, E in ((1, 300, 4), (2.5, 77, 16), (3, 5, 4)):
        assert cap(k, S_, E) == R.capacity(k, S_, E)


def _tokens():
    g = torch.Generator().manual_seed(0)
    return torch.randn(S, CFG.Cx, CFG.Nx, 1, generator=g), torch.randn(S, CFG.Cy, CFG.Ny, 1, generator=g)


def test_mutual_exclusions_raise_before_anything_runs():
    torch.manual_seed(0)
    m = build_module("avs", CFG)
    x, y = _tokens()
    m.router_expert_choice = 1
    m.router_top_k = 2
    with pytest.raises(ValueError, match="router_expert_choice"):
        m(x, y, is_training=True)
    m.router_top_k = CFG.E                                # k = E is the dense mixture: no conflict; CPU tokens are then what is refused
    with pytest.raises(_capi.AvmoeError, match="GPU"):
        m(x, y, is_training=True)
    m.router_top_k = None
    bal = RouterBiasBalancer([m])
    with pytest.raises(ValueError, match="router_expert_choice"):
        m(x, y, is_training=True)
    m.router_select_bias = None                           # the counts alone conflict too
    with pytest.raises(ValueError, match="router_expert_choice"):
        m(x, y, is_training=False)
    bal.detach()
    with pytest.raises(_capi.AvmoeError, match="GPU"):
        m(x, y, is_training=True)


def test_a_library_without_the_symbols_is_refused(monkeypatch):
    torch.manual_seed(0)
    m = build_module("avs", CFG)
    m.router_expert_choice = 1
    x, y = _tokens()
    monkeypatch.setattr(_capi.lib(), "avmoe_site_choice", False, raising=False)
    with pytest.raises(_capi.AvmoeError, match="predates"):
        m(x, y, is_training=True)
    with pytest.raises(_capi.AvmoeError, match="predates"):
        expert_choice_mask(torch.rand(8, 4), 2)
    monkeypatch.undo()
    with pytest.raises(_capi.AvmoeError, match="GPU"):    # with the symbols: a CPU tensor is what is refused
        expert_choice_mask(torch.rand(8, 4), 2)
