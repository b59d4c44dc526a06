"""The mixture regularisers without a GPU: the Philox reference of the draw and the multiplier built on it (tests/mix_drop_ref.py), the
host (CPU) twin with a multiplier (avmoe_host_moe_forward_reg / _backward_reg, include/avmoe_host.h), and the facade's settings."""
import ctypes as C
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

from avmoe_amd import _capi_moe as cm
from tests import mix_drop_ref as R
from tests.golden_util import load_golden, split_params
from tests.moe_gpu_util import make_desc

FIXTURE = "ave_train"        # the smallest AVE training shape of tests/golden (6 frames, 40 x 96 tokens; ave_e1p1_train has the shape with 2 experts, this one 4)


# ---- the generator ------------------------------------------------------------------------------------------------------------------
def test_philox_known_answers():
    """All-zero counter and key: the published vector.  Two more (all ones; the digits of pi) as produced by BOTH this numpy code and a
    plain C++ transcription of the round function written independently of it."""
    assert tuple(int(x) for x in R.philox4x32_10((0, 0, 0, 0), (0, 0))) == R.KAT_ZERO == (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)
    ones = 0xFFFFFFFF
    assert tuple(int(x) for x in R.philox4x32_10((ones,) * 4, (ones,) * 2)) == (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)
    got = R.philox4x32_10((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0))
    assert tuple(int(x) for x in got) == (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)


def test_philox_is_vectorised_consistently():
    s = np.arange(7, dtype=np.uint64)
    lanes = R.philox4x32_10((5, 9, s[:, None], np.arange(3, dtype=np.uint64)[None, :]), (11, 13))
    for i in range(7):
        for g in range(3):
            one = R.philox4x32_10((5, 9, i, g), (11, 13))
            assert all(int(lanes[j][i, g]) == int(one[j]) for j in range(4))


# ---- the multiplier -----------------------------------------------------------------------------------------------------------------
def test_mask_off_is_all_ones():
    assert np.array_equal(R.mix_scale(7, 3, 20, 4, 0.0, 0.0), np.ones((20, 4), dtype=np.float32))


def test_mask_q_close_to_one_drops_nearly_all():
    m = R.mix_scale(7, 0, 64, 16, 0.0, 0.999)
    assert m.dtype == np.float32 and (m == 0).mean() > 0.98          # 1024 pairs, 1 expected to survive: > 20 surviving has probability < 1e-18


@pytest.mark.parametrize("p,q", [(0.1, 0.0), (0.0, 0.3), (0.25, 0.5), (0.3, 0.7)])
def test_mask_kept_values_are_exact(p, q):
    m = R.mix_scale(0x0123456789ABCDEF, (1 << 32) + 5, 33, 7, p, q)
    keep = np.float32(np.float32(1) / (np.float32(1) - np.float32(p))) * np.float32(np.float32(1) / (np.float32(1) - np.float32(q)))
    assert m.dtype == np.float32 and set(np.unique(m)) <= {np.float32(0), np.float32(keep)}
    ua, ub = R.draws(0x0123456789ABCDEF, (1 << 32) + 5, 33, 7)
    assert np.array_equal(m != 0, (ua[:, None] >= np.float32(p)) & (ub >= np.float32(q)))
    if q == 0.0:                                                       # drop_path alone: whole frames
        assert all(len(set(row)) == 1 for row in m.tolist())


def test_mask_depends_on_seed_calls_and_not_on_the_other_extent():
    a = R.mix_scale(1, 0, 20, 4, 0.2, 0.4)
    assert not np.array_equal(a, R.mix_scale(2, 0, 20, 4, 0.2, 0.4)) and not np.array_equal(a, R.mix_scale(1, 1, 20, 4, 0.2, 0.4))
    assert not np.array_equal(a, R.mix_scale(1, 1 << 32, 20, 4, 0.2, 0.4))          # the counter's high word counts
    assert np.array_equal(a[:3], R.mix_scale(1, 0, 3, 4, 0.2, 0.4))                 # a frame's draw does not depend on S
    assert np.array_equal(a[:, :2] != 0, R.mix_scale(1, 0, 20, 2, 0.2, 0.4) != 0)   # nor an expert's on E (same group, same lane)


# ---- the host twin ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host():
    from avmoe_amd import build as b
    L = C.CDLL(b.build_host(verbose=False))
    L.avmoe_host_last_error.restype = C.c_char_p
    head = [C.POINTER(cm.MoeDesc), C.c_void_p, C.c_void_p, C.POINTER(cm.MoePtrs), C.c_void_p]
    L.avmoe_host_moe_forward_aux.restype = L.avmoe_host_moe_forward_reg.restype = C.c_int
    L.avmoe_host_moe_forward_aux.argtypes = head + [C.c_int32, C.c_int32] + [C.c_void_p] * 7
    L.avmoe_host_moe_forward_reg.argtypes = head + [C.c_int32, C.c_int32] + [C.c_void_p] * 8
    L.avmoe_host_moe_backward_aux.restype = L.avmoe_host_moe_backward_reg.restype = C.c_int
    L.avmoe_host_moe_backward_aux.argtypes = head + [C.c_void_p] * 7 + [C.POINTER(cm.MoePtrs), C.c_int32, C.c_int32]
    L.avmoe_host_moe_backward_reg.argtypes = head + [C.c_void_p] * 8 + [C.POINTER(cm.MoePtrs), C.c_int32, C.c_int32]
    return L


class HostSite:
    """The fixture on the host twin; every call starts from the fixture's own buffers."""

    def __init__(self, name=FIXTURE):
        self.meta, self.cfg, self.t = load_golden(name)
        self.P, self.B = split_params(self.t)
        self.X, self.Y = self.t["X"].contiguous(), self.t["Y"].contiguous()
        self.S, self.E = self.X.shape[0], self.cfg.E
        self.desc = make_desc(self.cfg, self.S, False, True)
        self.params = {k: v.clone().contiguous() for k, v in self.P.items()}

    def ptrs(self):
        bufs = {k: v.clone().contiguous() for k, v in self.B.items()}
        return cm.make_ptrs({**self.params, **bufs}, self.cfg.E_m, self.cfg.E_s), bufs

    def forward(self, L, mix="null", k=0, renorm=1, noise=None):
        """mix "null": avmoe_host_moe_forward_aux ; None: _reg with NULL ; a tensor: _reg with it -> (out, probs, idx, buffers after)"""
        ptrs, bufs = self.ptrs()
        out, probs = torch.full_like(self.X, float("nan")), torch.full((self.S, self.E), float("nan"))
        idx = torch.full((self.S,), -1, dtype=torch.int64)
        head = (C.byref(self.desc), self.X.data_ptr(), self.Y.data_ptr(), C.byref(ptrs), noise.data_ptr() if noise is not None else None, k, renorm)
        tail = (out.data_ptr(), probs.data_ptr(), idx.data_ptr(), None, None, None, None)
        if isinstance(mix, str):
            st = L.avmoe_host_moe_forward_aux(*head, *tail)
        else:
            st = L.avmoe_host_moe_forward_reg(*head, mix.data_ptr() if mix is not None else None, *tail)
        assert st == 0, L.avmoe_host_last_error()
        return out, probs, idx, bufs

    def backward(self, L, dO, dP, mix="null", k=0, renorm=1):
        ptrs, _ = self.ptrs()
        grads = {kk: torch.full_like(v, float("nan")) for kk, v in self.params.items()}
        gptrs = cm.make_ptrs(grads, self.cfg.E_m, self.cfg.E_s)
        dX, dY = torch.full_like(self.X, float("nan")), torch.full_like(self.Y, float("nan"))
        head = (C.byref(self.desc), self.X.data_ptr(), self.Y.data_ptr(), C.byref(ptrs), None, dO.data_ptr(), dP.data_ptr() if dP is not None else None, None, None)
        tail = (None, dX.data_ptr(), dY.data_ptr(), C.byref(gptrs), k, renorm)
        if isinstance(mix, str):
            st = L.avmoe_host_moe_backward_aux(*head, *tail)
        else:
            st = L.avmoe_host_moe_backward_reg(*head, mix.data_ptr() if mix is not None else None, *tail)
        assert st == 0, L.avmoe_host_last_error()
        return {**grads, "X": dX, "Y": dY}


@pytest.fixture(scope="module")
def site():
    return HostSite()


def _onehot_noise(S, E, e):
    n = torch.zeros(S, E)
    n[:, e] = 3.0e4               # softmax returns exactly 1 for the expert and 0 for the others
    return n


@pytest.mark.parametrize("k,renorm", [(0, 1), (2, 1), (2, 0)])
def test_host_forward_with_a_mask_is_the_masked_sum_of_its_own_experts(host, site, k, renorm):
    """out = sum_e m w expert_e, assembled from the twin's OWN pieces: expert_e(x) from a forward whose router is pushed to an exact
    one-hot (train-mode BatchNorm: an expert's output does not depend on the weights), w from the call without a multiplier
    (dense: probs; top-k: formed from probs by the rule of tests/topk_ref.py)."""
    from tests.topk_ref import topk_weights
    S, E = site.S, site.E
    m = torch.from_numpy(R.hand_mask(S, E))
    out, probs, idx, bufs = site.forward(host, m, k, renorm)
    dense = site.forward(host, "null", k, renorm)
    assert torch.equal(probs, dense[1]) and torch.equal(idx, dense[2])
    for kk, v in bufs.items():                                        # the BatchNorm running statistics advance as in the site without
        assert torch.equal(v, dense[3][kk]), kk
    experts = [site.forward(host, "null", 0, 1, noise=_onehot_noise(S, E, e))[0] for e in range(E)]
    w = topk_weights(probs, k or None, bool(renorm))
    ref = torch.zeros_like(out, dtype=torch.float64)
    for e in range(E):
        ref += (m[:, e].double() * w[:, e].double()).reshape(-1, 1, 1) * experts[e].double()
    # fp32 accumulation of E products per element against fp64: E + 2 roundings of 2^-24 each, relative to the largest term
    assert float((out.double() - ref).abs().max()) <= (E + 2) * 2.0 ** -24 * float(max(x.abs().max() for x in experts)) * float((m * w).max())
    assert bool((out[0] == 0).all()) and bool((out[1] == 0).all())    # the dropped frame and the frame that lost every expert: exact zeros
    assert not torch.equal(out, dense[0])


def test_host_all_ones_mask_and_null_reproduce_the_fixture_bit_for_bit(host, site):
    S, E = site.S, site.E
    ones = torch.ones(S, E)
    g = torch.Generator().manual_seed(5)
    dO, dP = torch.randn(site.X.shape, generator=g), torch.randn(S, E, generator=g)
    for k, renorm in ((0, 1), (2, 1), (2, 0)):
        base = site.forward(host, "null", k, renorm)
        gb = site.backward(host, dO, dP, "null", k, renorm)
        for mix in (ones, None):
            got = site.forward(host, mix, k, renorm)
            assert all(torch.equal(a, b) for a, b in zip(got[:3], base[:3]))
            assert all(torch.equal(v, base[3][kk]) for kk, v in got[3].items())
            gg = site.backward(host, dO, dP, mix, k, renorm)
            for kk, v in gb.items():
                assert torch.equal(gg[kk], v), (k, renorm, kk)
    out = site.forward(host, ones)[0]                                 # ... and the fixture itself, at the bar of tests/test_host_golden.py
    ref = site.t["out"]
    assert float((out - ref).abs().max() / ref.abs().max()) < 2e-5


@pytest.mark.parametrize("k,renorm", [(0, 1), (2, 1), (2, 0)])
def test_host_backward_with_a_mask_against_central_differences(host, site, k, renorm):
    """The hand-written reverse pass with a multiplier against central differences of L = <out, dO> + <probs, dP> evaluated in fp64
    (tests/mix_drop_ref.py::masked_forward on the fp64-cast fixture): per tensor, the derivative along two random directions -- and
    along every element for the tensors of at most 16 elements -- against the same projection of the twin's gradient.  Bar: that of
    tests/test_router_topk_host.py for the router path (rtol 1e-4, floor 1 % of the largest entry of the set).  h = 1e-6 in fp64: the
    differences' own error is ~h^2 |L'''| + 2^-53 |L| / h ~ 1e-9 relative, far below the bar."""
    S, E, cfg = site.S, site.E, site.cfg
    m = torch.from_numpy(R.hand_mask(S, E))
    g = torch.Generator().manual_seed(17)
    dO, dP = torch.randn(site.X.shape, generator=g), torch.randn(S, E, generator=g)
    got = site.backward(host, dO, dP, m, k, renorm)
    P64 = {kk: v.double() for kk, v in site.P.items()}
    B64 = {kk: (v.double() if v.is_floating_point() else v) for kk, v in site.B.items()}
    base = {"X": site.X.double(), "Y": site.Y.double(), **P64}
    dO64, dP64, m64 = dO.double(), dP.double(), m.double()

    def loss(override):
        t = {**base, **override}
        f = R.masked_forward({kk: t[kk] for kk in P64}, B64, t["X"], t["Y"], cfg, m64, k or None, bool(renorm), training=True)
        return float((f["out"] * dO64).sum() + (f["probs"] * dP64).sum())

    h = 1e-6
    ref, mine = {}, {}
    for kk, v in base.items():
        if v.numel() <= 16:
            dirs = [torch.zeros_like(v).reshape(-1).index_fill_(0, torch.tensor([i]), 1.0).reshape(v.shape) for i in range(v.numel())]
        else:
            dirs = [torch.randn(v.shape, generator=g, dtype=torch.float64) for _ in range(2)]
        ref[kk] = torch.tensor([(loss({kk: v + h * d}) - loss({kk: v - h * d})) / (2 * h) for d in dirs])
        mine[kk] = torch.tensor([float((got[kk].double() * d).sum()) for d in dirs])
    gmax = max(float(r.abs().max()) for r in ref.values())
    bad = {kk: (float((mine[kk] - r).abs().max()), float(r.abs().max())) for kk, r in ref.items()
           if not float((mine[kk] - r).abs().max()) <= 1e-4 * max(float(r.abs().max()), 1e-2 * gmax)}
    assert not bad, bad
    # Train-mode BatchNorm couples the frames: the tokens of the dropped frame (0) and of the frame without experts (1) still enter the
    # batch statistics, so the kept frames' gradients reach them THROUGH the statistics -- their dX is more than the router's broadcast
    # term.  The derivative along a direction that lives on those two frames alone pins that term to the central differences.
    d = torch.zeros_like(base["X"])
    d[:2] = torch.randn(d[:2].shape, generator=g, dtype=torch.float64)
    r = (loss({"X": base["X"] + h * d}) - loss({"X": base["X"] - h * d})) / (2 * h)
    assert abs(float((got["X"].double() * d).sum()) - r) <= 1e-4 * max(abs(r), 1e-2 * gmax)
    assert float((got["X"][0] - got["X"][0, :1]).abs().max()) > 0.0


def test_host_dropped_frames_get_only_the_router_term_without_batchnorm(host):
    """Without BatchNorm nothing couples the frames: a frame whose multipliers are all 0 sends exactly zero through the experts, and its
    dX / dY are those of the reverse pass with dOut = 0 (the router's term alone: the same row for every token of X)."""
    site = HostSite("ave_nobn")
    S, E = site.S, site.E
    m = torch.from_numpy(R.hand_mask(S, E))
    g = torch.Generator().manual_seed(23)
    dO, dP = torch.randn(site.X.shape, generator=g), torch.randn(S, E, generator=g)
    got = site.backward(host, dO, dP, m)
    router = site.backward(host, torch.zeros_like(dO), dP, m)
    for s in (0, 1):
        assert torch.equal(got["X"][s], router["X"][s]) and torch.equal(got["Y"][s], router["Y"][s]), s
        assert float((got["X"][s] - got["X"][s, :1]).abs().max()) == 0.0 and float(got["X"][s].abs().max()) > 0.0
    assert not torch.equal(got["X"][2], router["X"][2])


# ---- the facade, with no library loaded ----------------------------------------------------------------------------------------------
def _opt(**kw):
    return NS(num_conv_group=2, is_before_layernorm=1, is_post_layernorm=1, is_self_attention=0, num_multimodal_experts=2,
              num_singlemodal_experts=2, use_load_balacing_loss=0, **kw)


def _module(**kw):
    from avmoe_amd.adapters import MoEAdapter
    return MoEAdapter(96, 96, "bottleneck", None, 0, reduction_factor=8, opt=_opt(**kw), num_tk=8, conv_dim_in=56, conv_dim_out=40, linear_in=64,
                      linear_out=96)


def test_facade_settings_defaults_and_options():
    m = _module()
    assert m.drop_path == 0.0 and m.expert_dropout == 0.0 and m.last_mix_scale is None and m.mix_calls == 0
    m = _module(adapter_drop_path=0.1, adapter_expert_dropout=0.25)
    assert m.drop_path == 0.1 and m.expert_dropout == 0.25
    m.drop_path, m.expert_dropout = 0, np.float32(0.5)
    assert m.drop_path == 0.0 and m.expert_dropout == 0.5 and type(m.expert_dropout) is float


@pytest.mark.parametrize("name", ["drop_path", "expert_dropout"])
@pytest.mark.parametrize("bad", [1.0, 1.5, -0.01, float("nan"), True, "0.1", None])
def test_facade_refuses_bad_rates(name, bad):
    m = _module()
    with pytest.raises(ValueError, match=name):
        setattr(m, name, bad)
    assert getattr(m, name) == 0.0                                    # a refused value leaves the setting as it was
    with pytest.raises(ValueError, match=name):
        _module(**{"adapter_" + name: bad if bad is not None else 2})


def test_facade_seeds():
    a, b = _module(), _module()
    assert a.mix_seed != b.mix_seed and 0 <= a.mix_seed < 2 ** 64     # two sites do not share their draws
    assert a.mix_seed == a.mix_seed
    a.mix_seed = 2 ** 64 - 1
    assert a.mix_seed == 2 ** 64 - 1
    for bad in (-1, 2 ** 64, 1.5, True, "7"):
        with pytest.raises(ValueError, match="mix_seed"):
            a.mix_seed = bad
    a.mix_seed = None
    assert a.mix_seed != 2 ** 64 - 1


def test_facade_settings_are_not_state_and_travel_with_copies():
    import copy
    import pickle
    plain, m = _module(), _module(adapter_drop_path=0.2, adapter_expert_dropout=0.3)
    assert list(m.state_dict().keys()) == list(plain.state_dict().keys()) and not [k for k, _ in m.named_buffers() if "mix" in k]
    m.mix_seed = 99
    for c in (copy.deepcopy(m), pickle.loads(pickle.dumps(m))):
        assert (c.drop_path, c.expert_dropout, c.mix_seed) == (0.2, 0.3, 99) and c.last_mix_scale is None


def test_pair_and_loop_pass_each_sites_setting_through():
    """AdapterPair and DualBackboneLoop hold the sites themselves (shared, not copied): each site's own setting is what its call reads."""
    from avmoe_amd.adapters import AdapterPair
    a, b = _module(adapter_drop_path=0.1), _module(adapter_expert_dropout=0.4)
    pair = AdapterPair(a, b)
    assert pair.site_a is a and pair.site_b is b and (pair.site_a.drop_path, pair.site_b.expert_dropout) == (0.1, 0.4)
    a.drop_path = 0.3
    assert pair.site_a.drop_path == 0.3
