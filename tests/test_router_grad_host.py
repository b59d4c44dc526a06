"""The host (CPU) twin of avmoe_moe_backward_ex (include/avmoe_host.h): gradients of <out, dO> + <probs, dP> + w * lb on every committed
fixture against autograd through the oracle -- with dOut = NULL (out gets no gradient) too."""
import ctypes as C

import pytest
import torch

from avmoe_amd import _capi_moe as cm
from tests.golden_util import golden_names, load_golden, split_params, mha_keep_of
from tests.moe_gpu_util import make_desc
from tests.router_grad_util import oracle_grads, cases, expert_keys, assert_close


@pytest.fixture(scope="module")
def host():
    from avmoe_amd import build as b
    L = C.CDLL(b.build_host(verbose=False))
    L.avmoe_host_last_error.restype = C.c_char_p
    L.avmoe_host_moe_backward_ex.restype = C.c_int
    L.avmoe_host_moe_backward_ex.argtypes = [C.POINTER(cm.MoeDesc), C.c_void_p, C.c_void_p, C.POINTER(cm.MoePtrs)] + [C.c_void_p] * 7 + \
                                            [C.POINTER(cm.MoePtrs)]
    return L


@pytest.mark.parametrize("name", list(golden_names()))
def test_host_backward_ex_matches_oracle(host, name):
    meta, cfg, t = load_golden(name)
    P, B = split_params(t)
    training = bool(meta["module_train"])
    X, Y = t["X"].contiguous(), t["Y"].contiguous()
    S = X.shape[0]
    noise = t["noise"].contiguous() if "noise" in t else None
    keep = mha_keep_of(t)
    desc = make_desc(cfg, S, False, training)
    kp = {f"{pre}.{cm.SA_KEEP}": v.to(torch.float32).contiguous() for pre, v in (keep or {}).items()}
    params = {k: v.clone().contiguous() for k, v in P.items()}
    bufs = {k: v.clone().contiguous() for k, v in B.items()}
    ptrs = cm.make_ptrs({**params, **bufs, **kp}, cfg.E_m, cfg.E_s)
    g = torch.Generator().manual_seed(21)
    for label, with_out, dP, w in cases(cfg, S, 5):
        dO = torch.randn(X.shape, generator=g) if with_out else None
        ref = oracle_grads(cfg, P, B, X, Y, dO, dP, w, training, noise, keep)
        grads = {k: torch.full_like(v, float("nan")) for k, v in params.items()}
        gptrs = cm.make_ptrs(grads, cfg.E_m, cfg.E_s)
        dX, dY = torch.full_like(X, float("nan")), torch.full_like(Y, float("nan"))
        lbg = torch.tensor([w])
        dPc = dP.contiguous() if dP is not None else None
        st = host.avmoe_host_moe_backward_ex(C.byref(desc), X.data_ptr(), Y.data_ptr(), C.byref(ptrs), noise.data_ptr() if noise is not None else None,
                                             dO.data_ptr() if dO is not None else None, dPc.data_ptr() if dPc is not None else None,
                                             lbg.data_ptr() if cfg.lb_loss else None, None, dX.data_ptr(), dY.data_ptr(), C.byref(gptrs))
        assert st == 0, host.avmoe_host_last_error()
        got = {**grads, "X": dX, "Y": dY}
        assert_close(got, ref, rtol=1e-4, what=f"{name}/{label}")
        if not with_out:
            assert all(float(got[k].abs().max()) == 0.0 for k in expert_keys(got)), "expert gradients must be exactly 0 without dOut"
