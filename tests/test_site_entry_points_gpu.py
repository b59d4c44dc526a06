"""The site entry points of the C ABI are one forward and one backward (csrc/capi.cpp): the superset entry point with every option
off IS the older entry point, bit for bit -- which is what lets the facade always call avmoe_moe_forward_aux / avmoe_moe_backward_aux.

Called through ctypes directly, on the two smallest committed fixtures that cover the cases: ave_e1p1_train (a cross-modal expert, E = 2)
and avs_train_noise (E = 4, so top_k = 1 gates; logit noise and the load-balancing loss), in fp32 and bf16.  Every call starts from the
fixture's buffers, freshly poisoned workspaces and zeroed gradient buffers, so no equality hinges on what an earlier call left behind."""
import ctypes as C

import pytest
import torch

from avmoe_amd import _capi_moe as cm
from tests.golden_util import load_golden, split_params
from tests.moe_gpu_util import MoeRun

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
BAD_ARG, UNSUPPORTED = -1, -2
SITES = ("ave_e1p1_train", "avs_train_noise")
_FIXTURES = {}


def _ptr(t):
    return t.data_ptr() if t is not None else None


class Site(MoeRun):
    def __init__(self, name, bf16):
        if name not in _FIXTURES:                                      # loaded once, never modified
            _FIXTURES[name] = load_golden(name)
        meta, cfg, t = _FIXTURES[name]
        P, B = split_params(t)
        super().__init__(cfg, P, B, t["X"], t["Y"], bf16=bf16, training=True, noise=t.get("noise"))
        self.dO = t["grad_out"].to(DEV, self.tdt).contiguous()
        self.lbw = torch.full((1,), float(meta["lb_weight"]), device=DEV)
        self.stream = torch.cuda.current_stream().cuda_stream

    def fresh(self, sentinel=float("nan")):
        """the fixture's buffers again, the workspaces poisoned, every output filled with `sentinel`"""
        self.bufs = {k: v.clone() for k, v in self.buffers.items()}
        self.ptrs = cm.make_ptrs({**self.params, **self.bufs}, self.cfg.E_m, self.cfg.E_s)
        self.saved.fill_(0xFF)
        self.scratch.fill_(0xFF)
        self.out = torch.full_like(self.X, sentinel)
        self.probs = torch.full((self.S, self.cfg.E), sentinel, device=DEV)
        self.idx = torch.full((self.S,), -7, device=DEV, dtype=torch.int64)
        self.lb = torch.full((1,), sentinel, device=DEV)

    def forward_by(self, entry, k=0, renorm=1, policy=0, iters=1, cap_scale=True):
        """one forward from a fresh state -> (status, {out, probs, idx, lb, saved, buffers} as raw bytes on the CPU).  The newer entry
        points run with their own options off (mix_scale, select_bias, select_count, aux and load NULL); "capacity" with a capacity of S
        frames under `policy`, its cap_scale (S, E) and kept (S) left on the object (cap_scale = False: passed as NULL); "sinkhorn" with
        `iters` rounds"""
        self.fresh()
        self.cap_scale = torch.full((self.S, self.cfg.E), float("nan"), device=DEV)
        self.kept = torch.full((self.S,), -7, device=DEV, dtype=torch.int32)
        head = (C.byref(self.desc), self.X.data_ptr(), self.Y.data_ptr(), C.byref(self.ptrs), _ptr(self.noise))
        outs = (self.out.data_ptr(), self.probs.data_ptr(), self.idx.data_ptr(), self.lb.data_ptr())
        ws = (self.saved.data_ptr(), self.scratch.data_ptr(), self.stream)
        if entry == "plain":
            st = self.L.avmoe_moe_forward(*head, *outs, *ws)
        elif entry == "topk":
            st = self.L.avmoe_moe_forward_topk(*head, k, renorm, *outs, *ws)
        elif entry == "aux":
            st = self.L.avmoe_moe_forward_aux(*head, k, renorm, *outs, None, None, *ws)
        elif entry == "reg":
            st = self.L.avmoe_moe_forward_reg(*head, k, renorm, None, *outs, None, None, *ws)
        elif entry == "bias":
            st = self.L.avmoe_moe_forward_bias(*head, k, renorm, None, None, None, *outs, None, None, *ws)
        elif entry == "capacity":
            st = self.L.avmoe_moe_forward_capacity(*head, k, renorm, None, None, None, self.S, policy, _ptr(self.cap_scale if cap_scale else None),
                                                   self.kept.data_ptr(), None, None, *outs, None, None, *ws)
        else:
            assert entry == "sinkhorn"
            st = self.L.avmoe_moe_forward_sinkhorn(*head, k, renorm, iters, None, *outs, None, None, None, None, *ws)
        torch.cuda.synchronize()
        assert self.guards_intact()
        res = dict(out=self.out, probs=self.probs, idx=self.idx, lb=self.lb, saved=self.saved,
                   buffers=torch.cat([v.reshape(-1) for _, v in sorted(self.bufs.items())]))
        return st, {n: v.contiguous().view(torch.uint8).cpu() for n, v in res.items()}

    def backward_by(self, entry, sections=(0,), dO=True, sentinel=0.0):
        """the plain forward from a fresh state, then the backward's sections through `entry` into gradient buffers filled with `sentinel`
        -> ([status per section], {X, Y, parameter key: gradient} as raw bytes on the CPU)"""
        st, _ = self.forward_by("plain")
        assert st == 0
        self.ws_before = (self.saved.clone(), self.scratch.clone())
        dX, dY = torch.full_like(self.X, sentinel), torch.full_like(self.Y, sentinel)
        grads = {k: torch.full_like(v, sentinel) for k, v in self.params.items()}
        gptrs = cm.make_ptrs(grads, self.cfg.E_m, self.cfg.E_s)
        head = (C.byref(self.desc), self.X.data_ptr(), self.Y.data_ptr(), C.byref(self.ptrs), self.dO.data_ptr() if dO else None)
        tail = (self.saved.data_ptr(), self.scratch.data_ptr(), dX.data_ptr(), dY.data_ptr(), C.byref(gptrs))
        sts = []
        for parts in sections:
            if entry == "whole":
                assert parts == 0
                sts.append(self.L.avmoe_moe_backward(*head, self.lbw.data_ptr(), *tail, self.stream))
            elif entry == "part":
                sts.append(self.L.avmoe_moe_backward_part(*head, self.lbw.data_ptr(), *tail, parts, self.stream))
            elif entry == "ex":
                sts.append(self.L.avmoe_moe_backward_ex(*head, None, self.lbw.data_ptr(), *tail, parts, self.stream))
            else:
                sts.append(self.L.avmoe_moe_backward_aux(*head, None, self.lbw.data_ptr(), None, *tail, parts, self.stream))
        torch.cuda.synchronize()
        assert self.guards_intact()
        g = dict(grads, X=dX, Y=dY)
        return sts, {n: v.contiguous().view(torch.uint8).cpu() for n, v in g.items()}


def _same(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), f"{what}: {k} differs"


@pytest.fixture(scope="module", params=[(n, b) for n in SITES for b in (False, True)], ids=lambda p: f"{p[0]}-{'bf16' if p[1] else 'fp32'}")
def site(request):
    return Site(*request.param)


def test_dense_forward_is_one_forward(site):
    """avmoe_moe_forward == _forward_topk(k = E) == _forward_aux(k = 0, aux = NULL), the dense site's renorm passed as 1: out, probs, idx, lb,
    the advanced BatchNorm buffers and the whole of `saved` (mode word included)"""
    st0, plain = site.forward_by("plain")
    st1, topk = site.forward_by("topk", site.cfg.E, 1)
    st2, aux = site.forward_by("aux", 0, 1)
    assert (st0, st1, st2) == (0, 0, 0)
    assert not torch.isnan(site.out.float()).any()
    _same(plain, topk, "forward vs forward_topk(k = E)")
    _same(plain, aux, "forward vs forward_aux(k = 0)")
    for entry in ("reg", "bias"):                                      # ... == _reg(mix NULL) == _bias(mix, bias, count NULL)
        st, got = site.forward_by(entry, 0, 1)
        assert st == 0
        _same(aux, got, f"forward_aux vs forward_{entry} (k = 0, every option NULL)")


@pytest.mark.parametrize("renorm", [0, 1])
def test_top1_forward_is_one_forward(site, renorm):
    """_forward_topk(k = 1, renorm) == _forward_aux(k = 1, renorm, aux = NULL) -- and k = 1 does gate: it is not the dense output"""
    st0, topk = site.forward_by("topk", 1, renorm)
    st1, aux = site.forward_by("aux", 1, renorm)
    assert (st0, st1) == (0, 0)
    _same(topk, aux, f"forward_topk vs forward_aux (k = 1, renorm = {renorm})")
    _, dense = site.forward_by("plain")
    assert not torch.equal(dense["out"], topk["out"]) and torch.equal(dense["probs"], topk["probs"])
    for entry in ("reg", "bias"):                                      # ... == _reg(mix NULL) == _bias(mix, bias, count NULL)
        st, got = site.forward_by(entry, 1, renorm)
        assert st == 0
        _same(aux, got, f"forward_aux vs forward_{entry} (k = 1, renorm = {renorm}, every option NULL)")
    # ... == _capacity(capacity = S: nothing is dropped) under either policy.  Capacity works in `scratch`, which is not compared; its own
    # outputs: every kept word is the frame's one selected expert (k = 1: the first maximum of the softmax, idx), cap_scale its one-hot
    want_kept = (1 << site.idx).to(torch.int32)
    want_scale = torch.nn.functional.one_hot(site.idx, site.cfg.E).float()
    for policy in (0, 1):
        st, got = site.forward_by("capacity", 1, renorm, policy=policy)
        assert st == 0
        _same(aux, got, f"forward_aux vs forward_capacity (k = 1, renorm = {renorm}, capacity = S, policy {policy})")
        assert torch.equal(site.kept, want_kept), policy
        assert torch.equal(site.cap_scale, want_scale), policy


def test_whole_backward_is_one_backward(site):
    """avmoe_moe_backward == _part(0) == _ex(dprobs = NULL) == _aux(dprobs = NULL, aux_grad = NULL): dX, dY, every parameter gradient"""
    sts, whole = site.backward_by("whole")
    assert sts == [0]
    assert all(bool(torch.isfinite(v.view(torch.float32 if k not in ("X", "Y") else site.tdt).float()).all()) for k, v in whole.items())
    for entry in ("part", "ex", "aux"):
        sts, got = site.backward_by(entry)
        assert sts == [0]
        _same(whole, got, f"backward vs backward_{entry}")


def test_sectioned_backward_is_one_backward(site):
    """the sequence 1 | 32, 8, 64, 16 through _part == the same sequence through _aux"""
    seq = (1 | 32, 8, 64, 16)
    sts0, part = site.backward_by("part", seq)
    sts1, aux = site.backward_by("aux", seq)
    assert sts0 == [0] * 4 and sts1 == [0] * 4
    _same(part, aux, "sections through backward_part vs backward_aux")


def test_refusals_keep_their_status_and_launch_nothing(site):
    """_topk(k = 0), _sinkhorn(iters = 0), _capacity(cap_scale = NULL): BAD_ARG ; _part(dOut = NULL): BAD_ARG ; _ex(dOut = NULL, parts = 1):
    UNSUPPORTED -- every output keeps its sentinel"""
    for entry, k, opts in (("topk", 0, {}), ("sinkhorn", 1, dict(iters=0)), ("capacity", 1, dict(cap_scale=False))):
        st, res = site.forward_by(entry, k, 1, **opts)
        assert st == BAD_ARG, entry
        assert bool(torch.isnan(site.out.float()).all()) and bool(torch.isnan(site.probs).all()) and bool(torch.isnan(site.lb).all()), entry
        assert bool((site.idx == -7).all()) and bool((res["saved"] == 0xFF).all()) and bool((site.scratch == 0xFF).all()), entry
        assert bool(torch.isnan(site.cap_scale).all()) and bool((site.kept == -7).all()), entry
        for b, v in site.bufs.items():
            assert torch.equal(v, site.buffers[b]), (entry, b)
    for entry, parts, want in (("part", 0, BAD_ARG), ("ex", 1, UNSUPPORTED)):
        sts, g = site.backward_by(entry, (parts,), dO=False, sentinel=float("nan"))
        assert sts == [want], (entry, sts)
        assert torch.equal(site.saved, site.ws_before[0]) and torch.equal(site.scratch, site.ws_before[1]), entry      # as the forward left them
        for k, v in g.items():
            assert bool(torch.isnan(v.view(site.tdt if k in ("X", "Y") else torch.float32).float()).all()), (entry, k)
