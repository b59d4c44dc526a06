"""Sharpness-aware minimization in FlatAdam on the device (avmoe_amd.train.FlatAdam(sam_rho=..., sam_adaptive=...), hold_bn_stats;
include/avmoe.h: avmoe_opt_sam_perturb, avmoe_opt_adam_step_sam) on the two-bucket model of tests/test_flat_adam_ema_gpu.py, whose
parameter lengths are the tail and block-boundary cases of the kernels (a block serves 1024 elements, a thread four): 1, 3, 4, 5, 1023,
1024, 1025 and 2049 elements.  g1 (seed 5) is the gradient that perturbs, g2 (seed 6) the one the step applies.

Tolerance of the perturbation against fp64 (test_the_perturbation_against_fp64_from_the_devices_own_scale).  The kernel computes, in
fp32 with every operation rounded (u = 2^-24, half an ulp, relative),
    plain:     e = fl(scale * fl(g * gs))                             two roundings
    adaptive:  e = fl(fl(scale * fl(p * p)) * fl(g * gs))             four roundings
    p' = fl(p + e)                                                   one more
and the reference evaluates the same expression in fp64 from the same fp32 inputs and the device's own fp32 `scale` word.  Each
rounding in e is a relative error of at most u, so |e - e64| <= ((1 + u)^4 - 1) |e64| < 4.01 u |e64|; the sum adds at most
u |p + e| <= u (|p| + |e|).  Together |p' - p64| <= 4.01 u |e64| + u (|p| + 1.01 |e64|) < u |p| + 5.1 u |e64|: four roundings in e
and one in the sum.  The bound asserted is 8 u (|p| + |e64|) = 8 * 2^-24 * (|p| + |e64|), which covers that with room for the
element-wise maximum (5.1 < 8) and is about twice what the plain form (two roundings in e) can reach.

Everything that is the same kernels on the same bits is held to bit-equality."""
import copy

import numpy as np
import pytest
import torch

from tests.test_flat_adam_device_gpu import ulps
from tests.test_flat_adam_ema_gpu import (LR, MAX_NORM, WD, assert_flats_equal, bits, clone_params, flats, grads, make_opt, make_params,
                                          padding_mask, set_grads)
from tests.test_flat_adam_swa_gpu import OPTION_SETS as SWA_OPTION_SETS, lr_sched, poison

pytestmark = pytest.mark.gpu

RHO, STEPS, U = 0.05, 6, 2.0 ** -24
OPTION_SETS = dict(SWA_OPTION_SETS, ema=dict(weight_decay=WD, max_grad_norm=MAX_NORM, ema_decay=0.9))


def f32(x):
    return float(np.float32(x))


def f32_bits(x):
    return int(np.float32(x).view(np.int32))


def options(name):
    kw = dict(OPTION_SETS[name])
    if kw.get("lr_schedule"):
        kw["lr_schedule"] = lr_sched()
    return kw


def sam_step(opt, params, g1, g2):
    set_grads(params, g1)
    opt.sam_perturb()
    set_grads(params, g2)
    opt.step()


def assert_state_blocks_equal(oa, ob, what=""):
    sa, sb = oa.state_block, ob.state_block
    assert set(sa) == set(sb)
    for field in sa:
        assert torch.equal(bits(sa[field]) if sa[field].dtype != torch.int64 else sa[field].cpu(),
                           bits(sb[field]) if sb[field].dtype != torch.int64 else sb[field].cpu()), (what, field)


def hold_views(opt):
    return [r.view("h") for r in opt._recs]


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("adaptive", [False, True], ids=["sam", "asam"])
@pytest.mark.parametrize("name", list(OPTION_SETS))
def test_the_step_ignores_the_perturbation(name, adaptive):
    """A: g1, sam_perturb(), g2, step().  B, without SAM, from the same parameters: g2, step().  After 6 steps parameters, both moments
    (alignment padding included), the averages and every word of the state block are bit-equal.  "skip" holds step 4 back in both."""
    dev = torch.device("cuda:0")
    kw = options(name)
    a = make_params(dev)
    b = clone_params(a)
    g1s, g2s = grads(STEPS, dev, seed=5), grads(STEPS, dev, seed=6)
    _, oa = make_opt(a, sam_rho=RHO, sam_adaptive=adaptive, **kw)
    _, ob = make_opt(b, **kw)
    assert oa._flags == ob._flags and oa.sam_rho == f32(RHO) and ob.sam_rho is None
    for k in range(STEPS):
        set_grads(a, g1s[k])
        before = [p.detach().clone() for p in oa.params]
        oa.sam_perturb()
        assert oa.perturbed
        assert any(not torch.equal(p.data, q) for p, q in zip(oa.params, before))      # the weights did move
        set_grads(a, g2s[k]); set_grads(b, g2s[k])
        if name == "skip" and k == 3:
            poison(a[6]); poison(b[6])
        oa.step(); ob.step()
        assert not oa.perturbed
    assert_flats_equal(flats(oa, "pmve"), flats(ob, "pmve"), name)
    assert_state_blocks_equal(oa, ob, name)
    applied = STEPS - (name == "skip")
    assert int(oa.applied_steps.item()) == applied and int(oa.skipped_steps.item()) == (name == "skip") and oa.t == STEPS
    assert int(oa.sam_nonfinite.item()) == 0 and float(oa.last_sam_scale.item()) > 0


@pytest.mark.parametrize("adaptive", [False, True], ids=["sam", "asam"])
def test_the_perturbation_against_fp64_from_the_devices_own_scale(adaptive):
    """the bound of the module docstring, hold == the original parameters, the norm and the scale word"""
    dev = torch.device("cuda:0")
    gs = 0.75
    a = make_params(dev)
    g1 = grads(1, dev, seed=5)[0]
    red, opt = make_opt(a, sam_rho=RHO, sam_adaptive=adaptive, grad_scale=gs)
    p0 = [p.detach().clone() for p in opt.params]
    pad_before = [s["p"][padding_mask(b, dev)].clone() for b, s in zip(red.buckets, opt.state)]
    set_grads(a, g1)
    opt.sam_perturb()
    torch.cuda.synchronize()
    norm, scale = opt.last_sam_norm, opt.last_sam_scale
    assert norm.dtype == torch.float32 and norm.is_cuda and scale.dtype == torch.float32 and opt.sam_nonfinite.dtype == torch.int32
    norm, scale = float(norm.item()), float(scale.item())
    assert int(opt.sam_nonfinite.item()) == 0
    # the norm: of g * gs, adaptive of fl(|p| * g) * gs (the fp32 product the header defines), summed in fp64
    sq = 0.0
    for p, q in zip(opt.params, p0):
        t = (q.abs() * p.grad) if adaptive else p.grad
        sq += float((t.double() * gs).pow(2).sum())
    norm64 = float(np.sqrt(sq))
    print(f"adaptive {adaptive}: norm {norm!r} fp64 {norm64!r} ({ulps(norm, norm64)} ulp), scale {scale!r}")
    assert ulps(norm, norm64) <= 2
    assert f32_bits(scale) == f32_bits(f32(RHO) / (float(np.float64(np.float32(norm))) + 1e-12))
    worst = 0.0
    for p, q, h in zip(opt.params, p0, hold_views(opt)):
        assert torch.equal(bits(h), bits(q))                 # hold is the original, bit for bit
        g64, q64 = p.grad.double() * gs, q.double()
        e64 = scale * (q64 * q64) * g64 if adaptive else scale * g64
        err = (p.detach().double() - (q64 + e64)).abs()
        bound = 8 * U * (q64.abs() + e64.abs())
        worst = max(worst, float((err / bound.clamp_min(1e-300)).max()))
        assert bool((err <= bound).all()), (p.numel(), float((err - bound).max()))
        assert not torch.equal(p.data, q)
    print(f"adaptive {adaptive}: worst |p_dev - p64| / bound = {worst:.3f}")
    for b, s, old in zip(red.buckets, opt.state, pad_before):      # alignment padding belongs to no range
        pad = padding_mask(b, dev)
        assert torch.equal(bits(s["p"][pad]), bits(old)) and float(s["h"][pad].abs().max()) == 0.0
    if not adaptive:                                        # the norm pass and the summation are the step's own
        c = clone_params(make_params(dev))
        _, oc = make_opt(c, report_grad_norms=True, grad_scale=gs)
        set_grads(c, g1)
        oc.step()
        assert int(bits(oc.last_grad_norm).item()) == f32_bits(norm)
    opt.sam_restore()


def test_a_zero_and_a_poisoned_first_gradient():
    dev = torch.device("cuda:0")
    kw = dict(weight_decay=WD, max_grad_norm=MAX_NORM, skip_nonfinite=True)
    g2s = grads(2, dev, seed=6)
    for adaptive in (False, True):
        a = make_params(dev)
        b = clone_params(a)
        _, oa = make_opt(a, sam_rho=RHO, sam_adaptive=adaptive, **kw)
        _, ob = make_opt(b, **kw)
        # a zero gradient: scale * 0 is 0 and every bit stays
        start = flats(oa, "pmv")
        set_grads(a, [torch.zeros_like(p) for p in a])
        oa.sam_perturb()
        assert_flats_equal(start, flats(oa, "pmv"), "zero gradient")
        assert int(oa.sam_nonfinite.item()) == 0 and float(oa.last_sam_norm.item()) == 0.0
        assert f32_bits(float(oa.last_sam_scale.item())) == f32_bits(f32(RHO) / 1e-12)
        set_grads(a, g2s[0]); set_grads(b, g2s[0])
        oa.step(); ob.step()
        assert_flats_equal(flats(oa, "pmv"), flats(ob, "pmv"), "step after a zero perturbation")
        # an Inf in g1: nothing moves, the flag says so, and the step on a finite g2 is B's
        start = flats(oa, "pmv")
        set_grads(a, grads(1, dev, seed=5)[0])
        poison(a[6])
        oa.sam_perturb()
        assert int(oa.sam_nonfinite.item()) == 1 and float(oa.last_sam_scale.item()) == 0.0
        assert not np.isfinite(float(oa.last_sam_norm.item()))
        assert_flats_equal(start, flats(oa, "pmv"), "poisoned gradient")
        for h, p in zip(hold_views(oa), oa.params):          # hold is still written
            assert torch.equal(bits(h), bits(p.data))
        set_grads(a, g2s[1]); set_grads(b, g2s[1])
        oa.step(); ob.step()
        assert_flats_equal(flats(oa, "pmv"), flats(ob, "pmv"), "step after a poisoned perturbation")
        assert_state_blocks_equal(oa, ob)
        assert int(oa.applied_steps.item()) == 2 and int(oa.skipped_steps.item()) == 0


@pytest.mark.parametrize("adaptive", [False, True], ids=["sam", "asam"])
def test_a_skipped_step_restores(adaptive):
    dev = torch.device("cuda:0")
    a = make_params(dev)
    _, opt = make_opt(a, sam_rho=RHO, sam_adaptive=adaptive, weight_decay=WD, max_grad_norm=MAX_NORM, skip_nonfinite=True, ema_decay=0.9)
    g1s, g2s = grads(2, dev, seed=5), grads(2, dev, seed=6)
    sam_step(opt, a, g1s[0], g2s[0])                         # one applied step: moments and averages are not zero
    before = flats(opt, "pmve")
    set_grads(a, g1s[1])
    opt.sam_perturb()
    assert any(not torch.equal(x[0], s["p"]) for x, s in zip(before, opt.state))
    set_grads(a, g2s[1])
    poison(a[6])
    opt.step()
    assert not opt.perturbed
    assert_flats_equal(before, flats(opt, "pmve"), "skipped step")
    assert int(opt.skipped_steps.item()) == 1 and int(opt.applied_steps.item()) == 1 and int(opt.state_block["skip"].item()) == 1


def test_restore_gives_the_originals_back_and_the_guards_hold():
    from avmoe_amd import _capi as capi
    from avmoe_amd.train import adapter_state_dict, save_adapters
    dev = torch.device("cuda:0")
    a = make_params(dev)
    _, opt = make_opt(a, sam_rho=RHO, weight_decay=WD, ema_decay=0.9)
    g1s, g2s = grads(2, dev, seed=5), grads(2, dev, seed=6)
    sam_step(opt, a, g1s[0], g2s[0])
    sd = opt.state_dict()
    before = flats(opt, "pmve")
    with pytest.raises(RuntimeError, match="without a perturbation"):
        opt.sam_restore()
    set_grads(a, g1s[1])
    opt.sam_perturb()
    assert opt.perturbed
    with pytest.raises(RuntimeError, match="perturbed"):
        opt.sam_perturb()
    model = torch.nn.Linear(2, 2)
    for call in (opt.swap_ema, opt.state_dict, lambda: opt.load_state_dict(sd), lambda: adapter_state_dict(model, ema=opt),
                 lambda: save_adapters(model, "/nonexistent/never_written.pt", ema=opt)):
        with pytest.raises(RuntimeError, match="perturbed"):
            call()
    with pytest.raises(RuntimeError, match="perturbed"):
        with opt.ema_weights():
            pass
    assert opt.perturbed and any(not torch.equal(x[0], s["p"]) for x, s in zip(before, opt.state))
    opt.sam_restore()
    assert not opt.perturbed
    assert_flats_equal(before, flats(opt, "pmve"), "sam_restore")
    with opt.ema_weights():                                  # and the guarded calls work again
        pass
    opt.state_dict()
    set_grads(a, g2s[1]); opt.step()                         # a step without a perturbation is the plain step
    assert int(opt.applied_steps.item()) == 2
    _, plain = make_opt(clone_params(a), weight_decay=WD, max_grad_norm=MAX_NORM)
    for what in (plain.sam_perturb, plain.sam_restore, lambda: plain.last_sam_norm, lambda: plain.last_sam_scale, lambda: plain.sam_nonfinite):
        with pytest.raises(capi.AvmoeError, match="sam_rho"):
            what()
    assert plain.perturbed is False


def test_captured_perturbation_and_step_replay_bit_equal_to_the_eager_run():
    dev = torch.device("cuda:0")
    a = make_params(dev)
    b = clone_params(a)
    n_steps = 5
    g1s, g2s = grads(n_steps, dev, seed=5), grads(n_steps, dev, seed=6)
    kw = dict(sam_rho=RHO, weight_decay=WD, max_grad_norm=MAX_NORM, skip_nonfinite=True, ema_decay=0.9)
    _, oa = make_opt(a, **kw)
    _, ob = make_opt(b, **kw)
    start = flats(ob, "pmve")
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    eager = []
    with torch.cuda.stream(st):                              # the eager run (it also loads the kernels before the capture)
        for k in range(n_steps):
            sam_step(oa, a, g1s[k], g2s[k])
            eager.append((bits(oa.last_sam_norm), bits(oa.last_sam_scale), bits(oa.last_grad_norm)))
    torch.cuda.synchronize()
    g_perturb, g_step = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
    with torch.cuda.graph(g_perturb, stream=st):
        ob.sam_perturb()
    assert ob.perturbed
    with torch.cuda.graph(g_step, stream=st):
        ob.step()
    torch.cuda.synchronize()
    assert not ob.perturbed and int(ob.applied_steps.item()) == 0      # capturing runs nothing
    assert_flats_equal(start, flats(ob, "pmve"), "capture")
    for k in range(n_steps):
        set_grads(b, g1s[k])
        torch.cuda.synchronize()
        g_perturb.replay()
        torch.cuda.synchronize()
        assert torch.equal(bits(ob.last_sam_norm), eager[k][0]) and torch.equal(bits(ob.last_sam_scale), eager[k][1]), k
        set_grads(b, g2s[k])
        torch.cuda.synchronize()
        g_step.replay()
        torch.cuda.synchronize()
        assert torch.equal(bits(ob.last_grad_norm), eager[k][2]), k
    assert int(ob.applied_steps.item()) == n_steps
    assert_flats_equal(flats(oa, "pmve"), flats(ob, "pmve"), "graph replay")
    assert_state_blocks_equal(oa, ob, "graph replay")
    assert len({int(e[0].item()) for e in eager}) == n_steps  # the norm did change from replay to replay


def test_resume_continues_bit_equal_and_a_dict_without_the_keys_loads():
    dev = torch.device("cuda:0")
    a = make_params(dev)
    b = clone_params(a)
    g1s, g2s = grads(STEPS, dev, seed=5), grads(STEPS, dev, seed=6)
    kw = dict(weight_decay=WD, max_grad_norm=MAX_NORM, skip_nonfinite=True, lr_schedule=lr_sched())
    _, oa = make_opt(a, sam_rho=RHO, sam_adaptive=True, **kw)
    _, ob = make_opt(b, sam_rho=RHO, sam_adaptive=True, **kw)
    for k in range(3):
        sam_step(oa, a, g1s[k], g2s[k])
        sam_step(ob, b, g1s[k], g2s[k])
    sd = ob.state_dict()
    extra = sd["flat_adam"]
    assert extra["sam_rho"] == f32(RHO) and extra["sam_adaptive"] is True
    assert not any(isinstance(v, torch.Tensor) for k, v in extra.items() if k.startswith("sam_"))      # no tensor state
    # a fresh reducer + optimizer built with OTHER constants: the saved ones win
    _, oc = make_opt(b, sam_rho=0.5, sam_adaptive=False, **kw)
    oc.load_state_dict(copy.deepcopy(sd))
    assert oc.sam_rho == f32(RHO) and oc.sam_adaptive is True and int(oc.applied_steps.item()) == 3
    for k in range(3, STEPS):
        set_grads(a, g1s[k]); set_grads(b, g1s[k])
        oa.sam_perturb(); oc.sam_perturb()
        assert_flats_equal(flats(oa, "ph"), flats(oc, "ph"), "the perturbed weights after the resume", "ph")
        assert torch.equal(bits(oa.last_sam_scale), bits(oc.last_sam_scale))
        set_grads(a, g2s[k]); set_grads(b, g2s[k])
        oa.step(); oc.step()
    assert_flats_equal(flats(oa, "pmv"), flats(oc, "pmv"), "resumed run")
    assert_state_blocks_equal(oa, oc, "resumed run")
    # a dict without the keys (a run that had no SAM): the constructor's stay
    bare = copy.deepcopy(sd)
    del bare["flat_adam"]["sam_rho"], bare["flat_adam"]["sam_adaptive"]
    _, od = make_opt(clone_params(b), sam_rho=0.5, **kw)
    od.load_state_dict(bare)
    assert od.sam_rho == 0.5 and od.sam_adaptive is False and int(od.applied_steps.item()) == 3
    # an optimizer without SAM ignores saved ones, and a bad saved value is refused
    _, oe = make_opt(clone_params(b), **kw)
    oe.load_state_dict(copy.deepcopy(sd))
    assert oe.sam_rho is None and int(oe.applied_steps.item()) == 3
    bad = copy.deepcopy(sd)
    bad["flat_adam"]["sam_rho"] = -1.0
    with pytest.raises(ValueError, match="sam_rho"):
        od.load_state_dict(bad)


# ---------------------------------------------------------------------------------------------------------------------
class SitePair(torch.nn.Module):
    """an audio and a visual AVE adapter site of fixture size: each adapts its own tokens with the other modality's"""

    def __init__(self):
        super().__init__()
        from oracle import avmoe_oracle as O
        from tests.test_adapters_api import build_module
        self.audio_adapter_blocks_p1 = torch.nn.ModuleList([build_module("ave", O.AdapterConfig(Cx=64, Nx=50, Cy=48, Ny=20, reduction=4, groups=2, K=6))])
        self.vis_adapter_blocks_p1 = torch.nn.ModuleList([build_module("ave", O.AdapterConfig(Cx=48, Nx=20, Cy=64, Ny=50, reduction=4, groups=2, K=6))])

    def sites(self):
        return [self.audio_adapter_blocks_p1[0], self.vis_adapter_blocks_p1[0]]

    def forward(self, X, Y):
        return self.audio_adapter_blocks_p1[0](X, Y)[0], self.vis_adapter_blocks_p1[0](Y, X)[0]


def test_the_recipe_on_an_ave_site_pair_with_gradient_sinks():
    """the recipe of INTEGRATION.md on two sites whose gradients arrive through the reducer's sinks: the second forward sees the
    perturbed weights, the held pass leaves every BatchNorm statistic alone, and the step is the plain one with the second gradient"""
    from avmoe_amd.dp import AdapterGradReducer
    from avmoe_amd.train import FlatAdam, hold_bn_stats
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = SitePair()
    with torch.no_grad():                                    # the reference's zero gates make the output 0 whatever the weights are
        for k, p in model.named_parameters():
            if k.endswith(("gate", "gate_av")):
                p.fill_(0.4)
    model = model.to(dev).train()
    twin = copy.deepcopy(model)
    params = [p for s in model.sites() for p in s.parameters()]
    red = AdapterGradReducer(params, sites=model.sites())
    assert len(red.sinks) == 2
    opt = FlatAdam(red, lr=LR, weight_decay=WD, max_grad_norm=1.0, sam_rho=RHO)
    tred = AdapterGradReducer([p for s in twin.sites() for p in s.parameters()], sites=twin.sites())
    topt = FlatAdam(tred, lr=LR, weight_decay=WD, max_grad_norm=1.0)
    g = torch.Generator().manual_seed(3)
    draw = lambda *shape: torch.randn(*shape, generator=g).to(dev)
    X, Y = draw(4, 64, 50, 1), draw(4, 48, 20, 1)
    GX, GY = draw(4, 64, 50, 1), draw(4, 48, 20, 1)

    def loss(outs):
        return (outs[0] * GX).sum() + (outs[1] * GY).sum()

    for step in range(2):
        red.begin(sync=True)
        first = model(X, Y)
        loss(first).backward()
        red.finish()
        opt.sam_perturb()
        red.zero_grad(lazy=True)
        red.begin(sync=True)
        stats = {k: v.clone() for k, v in model.named_buffers() if "running_" in k}
        counts = {k: int(v) for k, v in model.named_buffers() if k.endswith("num_batches_tracked")}
        assert len(stats) >= 8 and counts
        with hold_bn_stats(model):
            second = model(X, Y)
            loss(second).backward()
        red.finish()
        for a, b in zip(first, second):                      # the sites read the perturbed weights through their cached pointers
            assert not torch.equal(a, b) and bool(torch.isfinite(b).all())
        for k, v in model.named_buffers():
            if k in stats:
                assert torch.equal(v, stats[k]), k
            elif k in counts:
                assert int(v) == counts[k] + 1, k            # the counters still advance, as torch's do
        with torch.no_grad():
            for tb, b in zip(tred.buckets, red.buckets):     # the twin gets the second-pass gradient and takes the plain step
                assert tb.flat.numel() == b.flat.numel()
                tb.flat.copy_(b.flat)
        opt.step()
        topt.step()
        assert not opt.perturbed
        for p, q in zip(opt.params, topt.params):
            assert p.shape == q.shape and torch.equal(bits(p.data), bits(q.data)), step
        red.zero_grad(lazy=True)
    assert int(opt.applied_steps.item()) == 2 and int(topt.applied_steps.item()) == 2
    assert all(m.momentum == 0.1 for m in model.modules() if isinstance(m, torch.nn.modules.batchnorm._BatchNorm))
