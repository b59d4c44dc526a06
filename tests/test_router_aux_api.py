"""Router auxiliary losses (z-loss, Switch balance loss), the part that needs no GPU: the new symbols and their ctypes signatures, the
host (CPU) twin avmoe_host_moe_forward_aux / _backward_aux against the fp64 reference of tests/router_aux_ref.py (dense, k = 2 renorm,
k = 1 Switch style; with and without noise; with the load-balancing loss), aux == NULL / aux_grad == NULL bit for bit the existing host
entry points, and the facade (`router_aux`, `last_router_aux`, `router_aux_total`)."""
import ctypes as C

import pytest
import torch

from avmoe_amd import _capi
from avmoe_amd import _capi_moe as cm
from avmoe_amd import adapters
from oracle import avmoe_oracle as O
from tests.moe_gpu_util import make_desc
from tests.router_grad_util import assert_close, expert_keys
from tests.router_aux_ref import MARGIN, aux_reference, check_aux, make_case
from tests.test_adapters_api import build_module, _opt

NEW = ("avmoe_moe_forward_aux", "avmoe_moe_backward_aux")
NEW_HOST = ("avmoe_host_moe_forward_aux", "avmoe_host_moe_backward_aux")
CFG = O.AdapterConfig(Cx=32, Nx=10, Cy=24, Ny=7, E_m=2, E_s=2, reduction=4, groups=2, K=4, variant="avs", lb_loss=True)
S = 6
# (label, top_k for the entry point, renorm)
MODES = [("dense", 0, True), ("k2_renorm", 2, True), ("k1_switch", 1, False)]


def test_library_exports_the_new_symbols_under_abi_11():
    L = _capi.lib()
    syms = _capi.exported_symbols()
    for s in NEW:
        assert hasattr(L, s) and s in syms
    assert L.avmoe_abi_version() == 11


def test_ctypes_signatures_are_registered():
    L = _capi.lib()
    assert L.avmoe_moe_forward_aux.restype is C.c_int and len(L.avmoe_moe_forward_aux.argtypes) == 16
    assert L.avmoe_moe_forward_aux.argtypes[5:7] == [C.c_int32, C.c_int32]
    assert L.avmoe_moe_backward_aux.restype is C.c_int and len(L.avmoe_moe_backward_aux.argtypes) == 15
    assert L.avmoe_moe_backward_aux.argtypes[13] is C.c_int32


def test_forward_aux_validates_k_without_a_gpu():
    L = _capi.lib()
    d = make_desc(CFG, S, False, True)
    ptrs = cm.MoePtrs()
    one = C.c_void_p(8)                             # never dereferenced: the call fails on top_k first
    for k in (-1, CFG.E + 1):
        st = L.avmoe_moe_forward_aux(C.byref(d), one, one, C.byref(ptrs), None, k, 1, one, one, one, one, one, one, one, one, None)
        assert st != 0 and b"top_k" in L.avmoe_last_error()


def test_plan_lists_the_new_regions_after_the_old_ones():
    L = _capi.lib()
    names = [n for n, _r, _o, _b in cm.buffer_table(L, make_desc(CFG, S, False, True))]
    assert names[-2:] == ["lse", "load"] and names[-4:-2] == ["psm", "mode"]
    table = {n: (r, b) for n, r, _o, b in cm.buffer_table(L, make_desc(CFG, S, False, True))}
    assert table["lse"] == (0, 4 * S) and table["load"][0] == 0 and table["load"][1] >= 4 * CFG.E


@pytest.fixture(scope="module")
def host():
    from avmoe_amd import build as b
    L = C.CDLL(b.build_host(verbose=False))
    for s in NEW_HOST:
        assert hasattr(L, s), s
    L.avmoe_host_last_error.restype = C.c_char_p
    head = [C.POINTER(cm.MoeDesc), C.c_void_p, C.c_void_p, C.POINTER(cm.MoePtrs)]
    L.avmoe_host_moe_forward.argtypes = head + [C.c_void_p] * 6
    L.avmoe_host_moe_forward_topk.argtypes = head + [C.c_void_p, C.c_int32, C.c_int32] + [C.c_void_p] * 5
    L.avmoe_host_moe_forward_aux.argtypes = head + [C.c_void_p, C.c_int32, C.c_int32] + [C.c_void_p] * 7
    L.avmoe_host_moe_backward_ex.argtypes = head + [C.c_void_p] * 7 + [C.POINTER(cm.MoePtrs)]
    L.avmoe_host_moe_backward_topk.argtypes = head + [C.c_void_p] * 7 + [C.POINTER(cm.MoePtrs), C.c_int32, C.c_int32]
    L.avmoe_host_moe_backward_aux.argtypes = head + [C.c_void_p] * 8 + [C.POINTER(cm.MoePtrs), C.c_int32, C.c_int32]
    for f in ("forward", "forward_topk", "forward_aux", "backward_ex", "backward_topk", "backward_aux"):
        getattr(L, "avmoe_host_moe_" + f).restype = C.c_int
    return L


class _HostSite:
    def __init__(self, case, cfg=CFG):
        self.cfg, self.P, self.B = cfg, case["P"], case["B"]
        self.X, self.Y, self.noise = case["X"].contiguous(), case["Y"].contiguous(), case["noise"]
        self.S = self.X.shape[0]
        self.desc = make_desc(cfg, self.S, False, True)
        self.params = {k: v.clone().contiguous() for k, v in self.P.items()}

    def ptrs(self):
        bufs = {k: v.clone().contiguous() for k, v in self.B.items()}
        return cm.make_ptrs({**self.params, **bufs}, self.cfg.E_m, self.cfg.E_s), bufs

    def np(self):
        return self.noise.data_ptr() if self.noise is not None else None

    def forward(self, L, k, renorm, entry="aux", want_aux=True):
        """entry 'aux': avmoe_host_moe_forward_aux; 'old': avmoe_host_moe_forward (k == 0) / _forward_topk"""
        ptrs, bufs = self.ptrs()
        out, probs = torch.full_like(self.X, float("nan")), torch.full((self.S, self.cfg.E), float("nan"))
        idx, lb = torch.full((self.S,), -1, dtype=torch.int64), torch.full((1,), float("nan"))
        aux, load = torch.full((2,), float("nan")), torch.full((self.cfg.E,), float("nan"))
        head = (C.byref(self.desc), self.X.data_ptr(), self.Y.data_ptr(), C.byref(ptrs), self.np())
        tail = (out.data_ptr(), probs.data_ptr(), idx.data_ptr(), lb.data_ptr())
        if entry == "aux":
            st = L.avmoe_host_moe_forward_aux(*head, k, int(renorm), *tail, aux.data_ptr() if want_aux else None,
                                              load.data_ptr() if want_aux else None, None)
        elif k == 0:
            st = L.avmoe_host_moe_forward(*head, *tail, None)
        else:
            st = L.avmoe_host_moe_forward_topk(*head, k, int(renorm), *tail, None)
        assert st == 0, L.avmoe_host_last_error()
        return dict(out=out, probs=probs, idx=idx, lb=lb, aux=aux, load=load, bufs=bufs)

    def backward(self, L, k, renorm, dO, dP, w, ag, entry="aux"):
        ptrs, _ = self.ptrs()
        grads = {kk: torch.full_like(v, float("nan")) for kk, v in self.params.items()}
        gptrs = cm.make_ptrs(grads, self.cfg.E_m, self.cfg.E_s)
        dX, dY = torch.full_like(self.X, float("nan")), torch.full_like(self.Y, float("nan"))
        lbg = torch.tensor([float(w)])
        agt = torch.tensor([float(ag[0]), float(ag[1])]) if ag is not None else None
        dPc = dP.contiguous() if dP is not None else None
        head = (C.byref(self.desc), self.X.data_ptr(), self.Y.data_ptr(), C.byref(ptrs), self.np(), dO.data_ptr() if dO is not None else None,
                dPc.data_ptr() if dPc is not None else None, lbg.data_ptr() if self.cfg.lb_loss else None)
        tail = (None, dX.data_ptr(), dY.data_ptr(), C.byref(gptrs))
        if entry == "aux":
            st = L.avmoe_host_moe_backward_aux(*head, agt.data_ptr() if agt is not None else None, *tail, k, int(renorm))
        elif k == 0:
            st = L.avmoe_host_moe_backward_ex(*head, *tail)
        else:
            st = L.avmoe_host_moe_backward_topk(*head, *tail, k, int(renorm))
        assert st == 0, L.avmoe_host_last_error()
        return {**grads, "X": dX, "Y": dY}


@pytest.mark.parametrize("noise", [False, True])
@pytest.mark.parametrize("label,k,renorm", MODES)
def test_host_twin_matches_reference(host, label, k, renorm, noise):
    case = make_case(CFG, S, k, noise=noise, seed=3)
    s = _HostSite(case)
    g = torch.Generator().manual_seed(17)
    dO, dP = torch.randn(s.X.shape, generator=g), torch.randn(S, CFG.E, generator=g)
    vals, _ = aux_reference(CFG, s.P, s.B, s.X, s.Y, k, renorm, noise=s.noise, grads=False)
    assert vals["margin"] >= MARGIN
    got = s.forward(host, k, renorm)
    check_aux(got["aux"], got["load"], vals, S, CFG.E, k, label)
    assert float((got["lb"] - vals["lb"]).abs()) < 1e-4 * max(1.0, abs(float(vals["lb"])))
    for what, with_out, dp, w, ag in [("full", True, dP, 0.7, (0.9, -1.1)), ("aux_only", False, None, 0.0, (0.9, -1.1)),
                                      ("z_only", False, None, 0.0, (1.3, 0.0)), ("balance_only", False, None, 0.0, (0.0, 0.8))]:
        _, ref = aux_reference(CFG, s.P, s.B, s.X, s.Y, k, renorm, noise=s.noise, dO=dO if with_out else None, dP=dp, lb_weight=w,
                               g_z=ag[0], g_b=ag[1])
        grads = s.backward(host, k, renorm, dO if with_out else None, dp, w, ag)
        assert_close(grads, ref, rtol=1e-3, what=f"{label}/noise={noise}/{what}")
        if not with_out:
            assert all(float(grads[kk].abs().max()) == 0.0 for kk in expert_keys(grads))
        if what in ("z_only", "balance_only"):
            assert float(ref["router.0.weight"].abs().max()) > 0.0      # (the term does reach the router)


@pytest.mark.parametrize("label,k,renorm", MODES)
def test_host_null_aux_is_the_existing_entry_points(host, label, k, renorm):
    s = _HostSite(make_case(CFG, S, k, noise=True, seed=3))
    g = torch.Generator().manual_seed(5)
    dO, dP = torch.randn(s.X.shape, generator=g), torch.randn(S, CFG.E, generator=g)
    old, new, with_aux = s.forward(host, k, renorm, "old"), s.forward(host, k, renorm, "aux", want_aux=False), s.forward(host, k, renorm)
    for key in ("out", "probs", "idx", "lb"):
        assert torch.equal(old[key], new[key]) and torch.equal(old[key], with_aux[key]), key
    assert bool(torch.isnan(new["aux"]).all()) and bool(torch.isnan(new["load"]).all())      # untouched
    for kk, v in old["bufs"].items():
        assert torch.equal(v, new["bufs"][kk]), kk
    go, gn = s.backward(host, k, renorm, dO, dP, 0.7, None, "old"), s.backward(host, k, renorm, dO, dP, 0.7, None, "aux")
    for kk, v in go.items():
        assert torch.equal(v, gn[kk]), kk


# ---- facade ---------------------------------------------------------------------------------------
def _module(**opt_fields):
    o = _opt(CFG)
    for k, v in opt_fields.items():
        setattr(o, k, v)
    return adapters.MoEAdapterAVS(input_dim=CFG.Cx, output_dim=CFG.Cx, adapter_kind="bottleneck", dim_list=None, layer_idx=0, opt=o,
                                  conv_dim_in=CFG.Ny, conv_dim_out=CFG.Nx, linear_in=CFG.Cy, linear_out=CFG.Cx,
                                  reduction_factor=CFG.reduction, use_bn=CFG.use_bn, use_gate=CFG.use_gate, num_tk=CFG.K)


def test_attribute_defaults_validates_and_follows_opt():
    m = _module()
    assert m.router_aux is False and m.last_router_aux is None
    assert _module(router_aux=True).router_aux is True
    m.router_aux = True
    assert m.router_aux is True
    for bad in (1, 0, None, "yes", 1.0):
        with pytest.raises(ValueError):
            m.router_aux = bad
        with pytest.raises(ValueError):
            _module(router_aux=bad)
    assert m.router_aux is True                      # a refused value leaves the attribute as it was
    m.router_aux = False
    assert m.router_aux is False


def test_state_dict_keys_unchanged_and_setting_survives_copies():
    import copy
    import pickle
    dense, m = build_module("avs", CFG), _module(router_aux=True)
    assert list(m.state_dict().keys()) == list(dense.state_dict().keys())
    m.load_state_dict(dense.state_dict(), strict=True)
    assert copy.deepcopy(m).router_aux is True and pickle.loads(pickle.dumps(m)).router_aux is True
    st = m.__getstate__()
    st.pop("_router_aux")                            # a module pickled before the setting existed
    old = adapters.MoEAdapterAVS.__new__(adapters.MoEAdapterAVS)
    old.__setstate__(st)
    assert old.router_aux is False and old.last_router_aux is None


def test_router_aux_total_raises_without_results():
    from avmoe_amd.train import router_aux_total
    m = _module(router_aux=True)                     # (on, but no forward ran)
    with pytest.raises(ValueError):
        router_aux_total([m], 1e-3, 1e-2)
    with pytest.raises(ValueError):
        router_aux_total([], 1e-3, 1e-2)
    a = adapters.RouterAux(torch.tensor(2.0, requires_grad=True), torch.tensor(3.0, requires_grad=True), torch.ones(4) / 4)
    m.__dict__["_last_router_aux"] = a
    tot = router_aux_total([m, m], 0.5, 2.0)
    assert float(tot.detach()) == pytest.approx(2 * (0.5 * 2.0 + 2.0 * 3.0)) and tot.requires_grad
    with pytest.raises(ValueError):
        router_aux_total([m, _module()], 0.5, 2.0)
