"""The selection bias of aux-loss-free expert balancing on the host (CPU) twin (avmoe_host_moe_forward_bias / _backward_bias,
include/avmoe_host.h) against autograd through tests/topk_ref.py with sel = the k highest p + b: forward and every gradient at the
tolerances of tests/test_router_topk_host.py, on two fixtures, k in {1, 2}, both renorm settings; the counts and the biased load; NULL /
NULL and a bias of zeros bit for bit avmoe_host_moe_forward_reg; a bias on a dense mixture refused."""
import ctypes as C

import pytest
import torch

from avmoe_amd import _capi_moe as cm
from tests.router_grad_util import cases, assert_close
from tests.router_bias_ref import select_mask, counts_of, changed_frames
from tests.test_router_topk_host import _Site, _close
from tests.topk_ref import topk_forward, topk_grads

FIXTURES = ["ave_train", "avs_train_noise"]


@pytest.fixture(scope="module")
def host():
    from avmoe_amd import build as b
    L = C.CDLL(b.build_host(verbose=False))
    L.avmoe_host_last_error.restype = C.c_char_p
    head = [C.POINTER(cm.MoeDesc), C.c_void_p, C.c_void_p, C.POINTER(cm.MoePtrs), C.c_void_p]
    L.avmoe_host_moe_forward_reg.restype = L.avmoe_host_moe_forward_bias.restype = L.avmoe_host_moe_backward_bias.restype = C.c_int
    L.avmoe_host_moe_forward_reg.argtypes = head + [C.c_int32, C.c_int32] + [C.c_void_p] * 8
    L.avmoe_host_moe_forward_bias.argtypes = head + [C.c_int32, C.c_int32] + [C.c_void_p] * 10
    L.avmoe_host_moe_backward_bias.argtypes = head + [C.c_void_p] * 9 + [C.POINTER(cm.MoePtrs), C.c_int32, C.c_int32]
    return L


def _forward(L, s, k, renorm, bias=None, count=None, entry="bias"):
    """-> (out, probs, idx, lb, aux, load, buffers after the call) of avmoe_host_moe_forward_bias (entry 'reg': _forward_reg)"""
    ptrs, bufs = s.ptrs()
    E = s.cfg.E
    out, probs = torch.full_like(s.X, float("nan")), torch.full((s.S, E), float("nan"))
    idx, lb = torch.full((s.S,), -1, dtype=torch.int64), torch.full((1,), float("nan"))
    aux, load = torch.full((2,), float("nan")), torch.full((E,), float("nan"))
    head = (C.byref(s.desc), s.X.data_ptr(), s.Y.data_ptr(), C.byref(ptrs), s.np(), k, int(renorm), None)
    tail = (out.data_ptr(), probs.data_ptr(), idx.data_ptr(), lb.data_ptr(), aux.data_ptr(), load.data_ptr(), None)
    if entry == "reg":
        st = L.avmoe_host_moe_forward_reg(*head, *tail)
    else:
        st = L.avmoe_host_moe_forward_bias(*head, bias.data_ptr() if bias is not None else None,
                                           count.data_ptr() if count is not None else None, *tail)
    assert st == 0, L.avmoe_host_last_error()
    return out, probs, idx, lb, aux, load, bufs


def _backward(L, s, dO, dP, w, k, renorm, bias):
    ptrs, _ = s.ptrs()
    grads = {kk: torch.full_like(v, float("nan")) for kk, v in s.params.items()}
    gptrs = cm.make_ptrs(grads, s.cfg.E_m, s.cfg.E_s)
    dX, dY = torch.full_like(s.X, float("nan")), torch.full_like(s.Y, float("nan"))
    lbg = torch.tensor([w])
    dPc = dP.contiguous() if dP is not None else None
    st = L.avmoe_host_moe_backward_bias(C.byref(s.desc), s.X.data_ptr(), s.Y.data_ptr(), C.byref(ptrs), s.np(),
                                        dO.data_ptr() if dO is not None else None, dPc.data_ptr() if dPc is not None else None,
                                        lbg.data_ptr() if s.cfg.lb_loss else None, None, None, bias.data_ptr() if bias is not None else None,
                                        None, dX.data_ptr(), dY.data_ptr(), C.byref(gptrs), k, int(renorm))
    assert st == 0, L.avmoe_host_last_error()
    return {**grads, "X": dX, "Y": dY}


def _bias_for(probs, k, seed):
    """The fixtures' frames are routed nearly alike, so a random bias either changes no frame or all of them.  This one mirrors the
    experts' mean probabilities about their mean, plus a little noise -- the order of the scores is roughly reversed -- and it must change
    some frame's selection (asserted)."""
    g = torch.Generator().manual_seed(seed)
    pbar = probs.mean(0)
    b = (-2.0 * (pbar - pbar.mean()) + 0.1 * pbar.std() * torch.randn(probs.shape[1], generator=g)).contiguous()
    assert bool(changed_frames(probs, b, k).any()), "the bias changes no selection: the test would show nothing"
    return b


@pytest.mark.parametrize("name", FIXTURES)
def test_host_bias_matches_reference(host, name):
    s = _Site(name)
    cfg = s.cfg
    g = torch.Generator().manual_seed(41)
    dense = _forward(host, s, 0, True, entry="reg")
    for k in (1, 2):
        b = _bias_for(dense[1], k, 7 + k)
        sel = select_mask(dense[1], b, k)                 # from the twin's own probabilities: no selection margin needed
        for renorm in (True, False):
            what = f"{name}/k={k}/renorm={renorm}"
            count = torch.tensor([3.0] * cfg.E)
            out, probs, idx, lb, aux, load, bufs = _forward(host, s, k, renorm, b, count)
            ref = topk_forward(s.P, s.B, s.X, s.Y, cfg, k, renorm, training=s.training, noise=s.noise, mha_keep=s.keep, sel=sel)
            _close(out, ref["out"], 1e-4, what + "/out")
            _close(probs, ref["probs"], 1e-5, what + "/probs")
            assert torch.equal(probs, dense[1]) and torch.equal(idx, dense[2]) and torch.equal(lb, dense[3]), what + ": probs / idx / lb not dense"
            assert torch.equal(count, 3.0 + counts_of(sel)), what + ": counts are added to, as integers"
            assert torch.equal(load, counts_of(sel) / (s.S * k)), what + ": load is the biased selection's"
            for kk, v in bufs.items():
                assert torch.equal(v, dense[6][kk]), (what, kk)
            for label, with_out, dP, w in cases(cfg, s.S, 5):
                dO = torch.randn(s.X.shape, generator=g) if with_out else None
                refg = topk_grads(cfg, s.P, s.B, s.X, s.Y, dO, dP, w, s.training, k, renorm, s.noise, s.keep, sel=sel)
                got = _backward(host, s, dO, dP, w, k, renorm, b)
                assert_close(got, refg, rtol=1e-4, floor_frac=1e-2, what=f"{what}/{label}")


def test_host_null_and_zero_bias_are_the_reg_entry_point_bitwise(host):
    s = _Site("avs_train_noise")
    E = s.cfg.E
    g = torch.Generator().manual_seed(3)
    dO, dP = torch.randn(s.X.shape, generator=g), torch.randn(s.S, E, generator=g)
    for k, renorm in ((0, True), (2, True), (1, False)):
        ref = _forward(host, s, k, renorm, entry="reg")
        variants = [None] + ([torch.zeros(E)] if k else [])
        for b in variants:
            got = _forward(host, s, k, renorm, b, None)
            for a_, r_ in zip(got[:6], ref[:6]):
                assert torch.equal(a_, r_) or (torch.isnan(a_).all() and torch.isnan(r_).all()), (k, renorm)
            ga, gr = _backward(host, s, dO, dP, 0.7, k, renorm, b), _backward(host, s, dO, dP, 0.7, k, renorm, None)
            for kk, v in gr.items():
                assert torch.equal(ga[kk], v), (k, renorm, kk)


def test_host_refuses_a_bias_on_a_dense_mixture(host):
    s = _Site("ave_train")
    ptrs, _ = s.ptrs()
    E = s.cfg.E
    out, b = torch.empty_like(s.X), torch.zeros(E)
    for k in (0, E):
        st = host.avmoe_host_moe_forward_bias(C.byref(s.desc), s.X.data_ptr(), s.Y.data_ptr(), C.byref(ptrs), None, k, 1, None, b.data_ptr(),
                                              None, out.data_ptr(), None, None, None, None, None, None)
        assert st == -1 and b"select_bias" in host.avmoe_host_last_error()
