"""Cumulative BatchNorm statistics (avmoe_moe_desc.bn_momentum < 0 = torch's momentum=None, include/avmoe.h) on the host twin
(avmoe_amd/csrc/host_moe.cpp): T training forwards against the oracle called step by step with bn_momentum = 1 / t and the buffers
carried along; the refusal of a missing counter.  CPU only."""
import ctypes as C
import dataclasses

import pytest
import torch

from avmoe_amd import _capi_moe as cm
from oracle import avmoe_oracle as O
from tests.golden_util import load_golden, split_params
from tests.moe_gpu_util import make_desc

T = 4


@pytest.fixture(scope="module")
def host():
    from avmoe_amd import build as b
    try:
        L = C.CDLL(b.build_host(verbose=False))
    except Exception as e:             # no g++ / libgomp on this box: the checker library is test infrastructure, not the product
        pytest.skip(f"libavmoe_host.so cannot be built here: {e}")
    L.avmoe_host_last_error.restype = C.c_char_p
    L.avmoe_host_moe_forward.restype = C.c_int
    L.avmoe_host_moe_forward.argtypes = [C.POINTER(cm.MoeDesc), C.c_void_p, C.c_void_p, C.POINTER(cm.MoePtrs), C.c_void_p] + [C.c_void_p] * 5
    return L


def _reset(B):
    out = {}
    for k, v in B.items():
        leaf = k.rsplit(".", 1)[-1]
        out[k] = torch.ones_like(v) if leaf == "running_var" else torch.zeros_like(v)
    return out


def _inputs(t, steps):
    g = torch.Generator().manual_seed(1234)
    return [(0.5 * torch.randn(t["X"].shape, generator=g), 0.5 * torch.randn(t["Y"].shape, generator=g)) for _ in range(steps)]


def _forward(host, desc, ptrs, X, Y, cfg, noise=None):
    S = X.shape[0]
    out, probs, idx, lb = torch.empty_like(X), torch.empty(S, cfg.E), torch.empty(S, dtype=torch.int64), torch.zeros(1)
    return host.avmoe_host_moe_forward(C.byref(desc), X.data_ptr(), Y.data_ptr(), C.byref(ptrs), noise.data_ptr() if noise is not None else None,
                                       out.data_ptr(), probs.data_ptr(), idx.data_ptr(), lb.data_ptr(), None)


@pytest.mark.parametrize("name", ["ave_train", "avvp_train"])
def test_host_cumulative_average_matches_the_oracle_step_by_step(host, name):
    meta, cfg, t = load_golden(name)
    P, B = split_params(t)
    assert cfg.use_bn
    params = {k: v.clone().contiguous() for k, v in P.items()}
    bufs = {k: v.contiguous() for k, v in _reset(B).items()}                       # means 0, variances 1, counters 0
    ptrs = cm.make_ptrs({**params, **bufs}, cfg.E_m, cfg.E_s)
    desc = make_desc(cfg, t["X"].shape[0], False, True)
    desc.bn_momentum = -1.0
    ref = _reset(B)
    for step, (X, Y) in enumerate(_inputs(t, T), 1):
        assert _forward(host, desc, ptrs, X, Y, cfg) == 0, host.avmoe_host_last_error()
        r = O.moe_forward(P, ref, X, Y, dataclasses.replace(cfg, bn_momentum=1.0 / step), training=True)
        ref = r["new_buffers"]
        for k, v in bufs.items():
            if v.is_floating_point():
                assert torch.allclose(v, ref[k], rtol=1e-5, atol=1e-6), (step, k)
            else:
                assert int(v) == step == int(ref[k]), (step, k)
    assert all(int(v) == T for k, v in bufs.items() if not v.is_floating_point())


def test_host_first_cumulative_step_equals_momentum_one(host):
    meta, cfg, t = load_golden("ave_train")
    P, B = split_params(t)
    X, Y = _inputs(t, 1)[0]
    got = []
    for mom in (-1.0, 1.0):
        bufs = {k: v.contiguous() for k, v in _reset(B).items()}
        ptrs = cm.make_ptrs({**{k: v.contiguous() for k, v in P.items()}, **bufs}, cfg.E_m, cfg.E_s)
        desc = make_desc(cfg, X.shape[0], False, True)
        desc.bn_momentum = mom
        assert _forward(host, desc, ptrs, X, Y, cfg) == 0, host.avmoe_host_last_error()
        got.append(bufs)
    assert all(torch.equal(got[0][k], got[1][k]) for k in got[0])


@pytest.mark.parametrize("missing", ["bn1", "bn2"])
def test_host_cumulative_average_refuses_a_missing_counter(host, missing):
    meta, cfg, t = load_golden("ave_train")
    P, B = split_params(t)
    bufs = {k: v.contiguous() for k, v in _reset(B).items()}
    before = {k: v.clone() for k, v in bufs.items()}
    gone = f"{cfg.expert_prefixes()[1]}.{missing}.num_batches_tracked"
    ptrs = cm.make_ptrs({**{k: v.contiguous() for k, v in P.items()}, **{k: v for k, v in bufs.items() if k != gone}}, cfg.E_m, cfg.E_s)
    desc = make_desc(cfg, t["X"].shape[0], False, True)
    desc.bn_momentum = -1.0
    X, Y = _inputs(t, 1)[0]
    assert _forward(host, desc, ptrs, X, Y, cfg) == -1
    msg = host.avmoe_host_last_error().decode()
    assert f"{missing}_nbt" in msg and "expert 1" in msg, msg
    assert all(torch.equal(v, before[k]) for k, v in bufs.items()), "a refused call writes nothing"
    desc.training = 0                                     # eval mode ignores the field: the same pointers are served
    assert _forward(host, desc, ptrs, X, Y, cfg) == 0, host.avmoe_host_last_error()
