"""Top-k gating of the mixture, host side: the `opt` fields and module attributes of the facade, their validation, unchanged state_dict
keys, and the new symbols in the built libraries."""
import ctypes as C

import pytest

from avmoe_amd import _capi
from avmoe_amd import adapters
from tests.golden_util import load_golden
from tests.test_adapters_api import build_module, _opt

FIXTURES = {"ave": "ave_train", "avqa": "avqa_train", "avvp": "avvp_train", "avs": "avs_train_noise"}


def _module(which, **opt_fields):
    _, cfg, _ = load_golden(FIXTURES[which])
    o = _opt(cfg)
    for k, v in opt_fields.items():
        setattr(o, k, v)
    common = dict(input_dim=cfg.Cx, output_dim=cfg.Cx, adapter_kind="bottleneck", dim_list=None, layer_idx=0, opt=o,
                  conv_dim_in=cfg.Ny, conv_dim_out=cfg.Nx, linear_in=cfg.Cy, linear_out=cfg.Cx)
    if which == "ave":
        return adapters.MoEAdapter(reduction_factor=cfg.reduction, use_bn=cfg.use_bn, use_gate=cfg.use_gate, num_tk=cfg.K, **common), cfg
    if which == "avs":
        return adapters.MoEAdapterAVS(reduction_factor=cfg.reduction, use_bn=cfg.use_bn, use_gate=cfg.use_gate, num_tk=cfg.K, **common), cfg
    if which == "avqa":
        return adapters.MoEAdapterAVQA(reduction_factor=cfg.reduction, use_bn=cfg.use_bn, use_gate=cfg.use_gate, **common), cfg
    return adapters.MoEAdapterAVVP(**common), cfg


@pytest.mark.parametrize("which", list(FIXTURES))
def test_opt_fields_become_attributes(which):
    m, cfg = _module(which)
    assert m.router_top_k is None and m.router_top_k_renorm is True          # absent: the dense mixture
    m, _ = _module(which, router_top_k=None)
    assert m.router_top_k is None
    m, _ = _module(which, router_top_k=2, router_top_k_renorm=False)
    assert m.router_top_k == 2 and m.router_top_k_renorm is False
    m, _ = _module(which, router_top_k=cfg.E)
    assert m.router_top_k == cfg.E


@pytest.mark.parametrize("which", list(FIXTURES))
def test_bad_k_is_rejected(which):
    _, cfg = _module(which)
    for k in (0, -1, cfg.E + 1, 1.5, "2", True):
        with pytest.raises(ValueError):
            _module(which, router_top_k=k)
    m, _ = _module(which)
    for k in (0, cfg.E + 1, 2.0, False):
        with pytest.raises(ValueError):
            m.router_top_k = k
    assert m.router_top_k is None                  # a refused value leaves the attribute as it was


def test_attributes_may_be_reassigned():
    m, cfg = _module("ave", router_top_k=1)
    m.router_top_k = 2
    m.router_top_k_renorm = 0
    assert m.router_top_k == 2 and m.router_top_k_renorm is False
    m.router_top_k = None
    assert m.router_top_k is None
    import numpy as np
    m.router_top_k = np.int64(cfg.E)               # any integral type
    assert m.router_top_k == cfg.E and type(m.router_top_k) is int


@pytest.mark.parametrize("which", list(FIXTURES))
def test_state_dict_keys_unchanged(which):
    _, cfg, _ = load_golden(FIXTURES[which])
    dense = build_module("avs" if which == "avs" else which, cfg)
    m, _ = _module(which, router_top_k=1, router_top_k_renorm=False)
    assert list(m.state_dict().keys()) == list(dense.state_dict().keys())
    m.load_state_dict(dense.state_dict(), strict=True)


def test_deepcopy_keeps_the_setting():
    import copy
    m, _ = _module("avs", router_top_k=2, router_top_k_renorm=False)
    c = copy.deepcopy(m)
    assert c.router_top_k == 2 and c.router_top_k_renorm is False


def test_library_exports_topk_entry_point():
    L = _capi.lib()
    assert hasattr(L, "avmoe_moe_forward_topk")
    assert "avmoe_moe_forward_topk" in _capi.exported_symbols()
    assert L.avmoe_abi_version() == 11


def test_topk_entry_point_validates_k_without_a_gpu():
    """top_k outside [1, E] is refused before anything is launched (the checks need no device)."""
    from avmoe_amd import _capi_moe as cm
    from tests.moe_gpu_util import make_desc
    _, cfg, _ = load_golden("ave_train")
    L = _capi.lib()
    d = make_desc(cfg, 6, False, True)
    ptrs = cm.MoePtrs()
    one = C.c_void_p(8)                             # never dereferenced: the call fails on top_k first
    for k in (0, cfg.E + 1):
        st = L.avmoe_moe_forward_topk(C.byref(d), one, one, C.byref(ptrs), None, k, 1, one, one, one, one, one, one, None)
        assert st != 0 and b"top_k" in L.avmoe_last_error()


def test_host_library_exports_topk_entry_points():
    from avmoe_amd import build as b
    L = C.CDLL(b.build_host(verbose=False))
    assert hasattr(L, "avmoe_host_moe_forward_topk") and hasattr(L, "avmoe_host_moe_backward_topk")


def test_module_pickled_without_the_setting_stays_dense():
    """A whole module pickled before top-k existed has neither attribute in its __dict__: it unpickles to the dense mixture."""
    import pickle
    m, _ = _module("ave", router_top_k=2, router_top_k_renorm=False)
    st = m.__getstate__()
    st.pop("_router_top_k"); st.pop("_router_top_k_renorm")
    old = adapters.MoEAdapter.__new__(adapters.MoEAdapter)
    old.__setstate__(st)
    assert old.router_top_k is None and old.router_top_k_renorm is True
    again = pickle.loads(pickle.dumps(old))
    assert again.router_top_k is None and again.router_top_k_renorm is True


@pytest.mark.parametrize("family", ["tile_stream", "tile_fast", "tile_gen", "tile_kernels"])
def test_family_shapes_plan_onto_their_family(family):
    """The shapes the GPU checks of top-k gating run per bottleneck-space kernel family land on that family (tile_stream: the
    register-resident shape, whose streaming form is picked at launch)."""
    from tests.topk_families import family_config, plan_family
    cfg, S, bf16 = family_config(family)
    assert plan_family(cfg, S, bf16) == ("tile_fast" if family == "tile_stream" else family)
