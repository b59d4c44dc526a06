"""Top-k gating of the mixture on the host (CPU) twin (avmoe_host_moe_forward_topk / avmoe_host_moe_backward_topk, include/avmoe_host.h)
against autograd through tests/topk_ref.py on every committed fixture: forward out / probs / idx / lb and the gradients of
<out, dO> + <probs, dP> + w * lb, for k in {1, 2, E} and both renorm settings; k = E bit for bit the dense entry points; an exact tie
keeps the first k experts."""
import ctypes as C

import pytest
import torch

from avmoe_amd import _capi_moe as cm
from oracle import avmoe_oracle as O
from tests.golden_util import golden_names, load_golden, split_params, mha_keep_of
from tests.moe_gpu_util import make_desc
from tests.router_grad_util import cases, assert_close
from tests.topk_ref import topk_forward, topk_grads, k_values


@pytest.fixture(scope="module")
def host():
    from avmoe_amd import build as b
    L = C.CDLL(b.build_host(verbose=False))
    L.avmoe_host_last_error.restype = C.c_char_p
    L.avmoe_host_moe_forward.restype = C.c_int
    L.avmoe_host_moe_forward.argtypes = [C.POINTER(cm.MoeDesc), C.c_void_p, C.c_void_p, C.POINTER(cm.MoePtrs)] + [C.c_void_p] * 6
    L.avmoe_host_moe_forward_topk.restype = C.c_int
    L.avmoe_host_moe_forward_topk.argtypes = [C.POINTER(cm.MoeDesc), C.c_void_p, C.c_void_p, C.POINTER(cm.MoePtrs), C.c_void_p,
                                              C.c_int32, C.c_int32] + [C.c_void_p] * 5
    L.avmoe_host_moe_backward_ex.restype = C.c_int
    L.avmoe_host_moe_backward_ex.argtypes = [C.POINTER(cm.MoeDesc), C.c_void_p, C.c_void_p, C.POINTER(cm.MoePtrs)] + [C.c_void_p] * 7 + \
                                            [C.POINTER(cm.MoePtrs)]
    L.avmoe_host_moe_backward_topk.restype = C.c_int
    L.avmoe_host_moe_backward_topk.argtypes = [C.POINTER(cm.MoeDesc), C.c_void_p, C.c_void_p, C.POINTER(cm.MoePtrs)] + [C.c_void_p] * 7 + \
                                              [C.POINTER(cm.MoePtrs), C.c_int32, C.c_int32]
    return L


class _Site:
    """One fixture on the host: parameters, buffers (cloned per forward: a training forward advances them) and pointer structs."""

    def __init__(self, name, zero_router_out=False):
        meta, cfg, t = load_golden(name)
        P, B = split_params(t)
        if zero_router_out:
            P = dict(P)
            P["router.4.weight"], P["router.4.bias"] = torch.zeros_like(P["router.4.weight"]), torch.zeros_like(P["router.4.bias"])
        self.cfg, self.P, self.B = cfg, P, B
        self.training = bool(meta["module_train"])
        self.X, self.Y = t["X"].contiguous(), t["Y"].contiguous()
        self.S = self.X.shape[0]
        self.noise = t["noise"].contiguous() if "noise" in t else None
        self.keep = mha_keep_of(t)
        self.desc = make_desc(cfg, self.S, False, self.training)
        self.kp = {f"{pre}.{cm.SA_KEEP}": v.to(torch.float32).contiguous() for pre, v in (self.keep or {}).items()}
        self.params = {k: v.clone().contiguous() for k, v in P.items()}

    def ptrs(self):
        bufs = {k: v.clone().contiguous() for k, v in self.B.items()}
        return cm.make_ptrs({**self.params, **bufs, **self.kp}, self.cfg.E_m, self.cfg.E_s), bufs

    def np(self):
        return self.noise.data_ptr() if self.noise is not None else None

    def forward(self, L, k=None, renorm=True):
        """-> (out, probs, idx, lb, buffers after the call); k None: avmoe_host_moe_forward."""
        ptrs, bufs = self.ptrs()
        out = torch.full_like(self.X, float("nan"))
        probs = torch.full((self.S, self.cfg.E), float("nan"))
        idx = torch.full((self.S,), -1, dtype=torch.int64)
        lb = torch.full((1,), float("nan"))
        if k is None:
            st = L.avmoe_host_moe_forward(C.byref(self.desc), self.X.data_ptr(), self.Y.data_ptr(), C.byref(ptrs), self.np(), out.data_ptr(),
                                          probs.data_ptr(), idx.data_ptr(), lb.data_ptr(), None)
        else:
            st = L.avmoe_host_moe_forward_topk(C.byref(self.desc), self.X.data_ptr(), self.Y.data_ptr(), C.byref(ptrs), self.np(), k, int(renorm),
                                               out.data_ptr(), probs.data_ptr(), idx.data_ptr(), lb.data_ptr(), None)
        assert st == 0, L.avmoe_host_last_error()
        return out, probs, idx, lb, bufs

    def backward(self, L, dO, dP, w, k=None, renorm=True):
        """-> {'X', 'Y', parameter key: gradient}; k None: avmoe_host_moe_backward_ex."""
        ptrs, _ = self.ptrs()
        grads = {kk: torch.full_like(v, float("nan")) for kk, v in self.params.items()}
        gptrs = cm.make_ptrs(grads, self.cfg.E_m, self.cfg.E_s)
        dX, dY = torch.full_like(self.X, float("nan")), torch.full_like(self.Y, float("nan"))
        lbg = torch.tensor([w])
        dPc = dP.contiguous() if dP is not None else None
        args = (C.byref(self.desc), self.X.data_ptr(), self.Y.data_ptr(), C.byref(ptrs), self.np(), dO.data_ptr() if dO is not None else None,
                dPc.data_ptr() if dPc is not None else None, lbg.data_ptr() if self.cfg.lb_loss else None, None, dX.data_ptr(), dY.data_ptr(),
                C.byref(gptrs))
        st = L.avmoe_host_moe_backward_ex(*args) if k is None else L.avmoe_host_moe_backward_topk(*args, k, int(renorm))
        assert st == 0, L.avmoe_host_last_error()
        return {**grads, "X": dX, "Y": dY}


def _close(got, ref, rtol, what):
    err = float((got.double() - ref.double()).abs().max())
    assert err <= rtol * max(float(ref.abs().max()), 1e-6), f"{what}: err {err}"


@pytest.mark.parametrize("name", list(golden_names()))
def test_host_topk_matches_reference(host, name):
    s = _Site(name)
    cfg = s.cfg
    g = torch.Generator().manual_seed(31)
    for k in [k for k in k_values(cfg.E) if k < cfg.E]:
        for renorm in (True, False):
            what = f"{name}/k={k}/renorm={renorm}"
            out, probs, idx, lb, bufs = s.forward(host, k, renorm)
            ref = topk_forward(s.P, s.B, s.X, s.Y, cfg, k, renorm, training=s.training, noise=s.noise, mha_keep=s.keep)
            _close(out, ref["out"], 1e-4, what + "/out")
            _close(probs, ref["probs"], 1e-5, what + "/probs")
            assert torch.equal(idx, ref["idx"]), what
            _close(lb, ref["lb"].reshape(1), 1e-5, what + "/lb")
            dense = s.forward(host)
            assert torch.equal(probs, dense[1]) and torch.equal(idx, dense[2]) and torch.equal(lb, dense[3]), what + ": probs / idx / lb not dense"
            for kk, v in bufs.items():                   # the BatchNorm running statistics advance exactly as in the dense site
                assert torch.equal(v, dense[4][kk]), (what, kk)
            for label, with_out, dP, w in cases(cfg, s.S, 5):
                dO = torch.randn(s.X.shape, generator=g) if with_out else None
                refg = topk_grads(cfg, s.P, s.B, s.X, s.Y, dO, dP, w, s.training, k, renorm, s.noise, s.keep)
                got = s.backward(host, dO, dP, w, k, renorm)
                # (floor 1 % of the largest gradient: an expert kept in one or two frames has structurally ~0 gradients -- ln_before.bias
                # in front of a train-mode BatchNorm -- whose fp32 cancellation error is judged against that floor)
                assert_close(got, refg, rtol=1e-4, floor_frac=1e-2, what=f"{what}/{label}")


@pytest.mark.parametrize("name", list(golden_names()))
def test_host_topk_k_equals_E_is_dense(host, name):
    s = _Site(name)
    E = s.cfg.E
    dense = s.forward(host)
    g = torch.Generator().manual_seed(3)
    dO, dP = torch.randn(s.X.shape, generator=g), torch.randn(s.S, E, generator=g)
    dgr = s.backward(host, dO, dP, 0.7)
    for renorm in (True, False):
        got = s.forward(host, E, renorm)
        for a, b in zip(got[:4], dense[:4]):
            assert torch.equal(a, b), name
        gg = s.backward(host, dO, dP, 0.7, E, renorm)
        for kk, v in dgr.items():
            assert torch.equal(gg[kk], v), (name, kk)


def test_host_topk_rejects_bad_k(host):
    s = _Site("ave_train")
    ptrs, _ = s.ptrs()
    out, probs, idx, lb = torch.empty_like(s.X), torch.empty(s.S, s.cfg.E), torch.empty(s.S, dtype=torch.int64), torch.empty(1)
    for k in (0, -1, s.cfg.E + 1):
        st = host.avmoe_host_moe_forward_topk(C.byref(s.desc), s.X.data_ptr(), s.Y.data_ptr(), C.byref(ptrs), None, k, 1, out.data_ptr(),
                                              probs.data_ptr(), idx.data_ptr(), lb.data_ptr(), None)
        assert st != 0 and b"top_k" in host.avmoe_host_last_error()


@pytest.mark.parametrize("renorm", [True, False])
def test_host_topk_exact_tie_keeps_first_experts(host, renorm):
    """Router output layer zeroed: every frame's probabilities are exactly uniform, so the first k experts (in expert order) are kept."""
    s = _Site("ave_train", zero_router_out=True)
    cfg, E, k = s.cfg, s.cfg.E, 2
    out, probs, idx, _, _ = s.forward(host, k, renorm)
    assert bool((probs == probs[0, 0]).all()) and bool((idx == 0).all())
    w = torch.zeros(E)
    w[:k] = (1.0 / k) if renorm else (1.0 / E)
    ref = torch.zeros_like(s.X)
    Yf = O.moe_forward(s.P, s.B, s.X, s.Y, cfg, training=s.training, update_buffers=False)["Yf"]
    for j, pre in enumerate(cfg.expert_prefixes()):
        ref = ref + w[j] * O.expert_forward(s.P, s.B, pre, s.X, Yf, cfg, j < cfg.E_m, s.training, None)
    _close(out, ref, 1e-4, "tie")
    ref2 = topk_forward(s.P, s.B, s.X, s.Y, cfg, k, renorm, training=s.training)
    assert torch.equal(ref2["w"], w.expand(s.S, E)), "topk_ref: ties in expert order"
