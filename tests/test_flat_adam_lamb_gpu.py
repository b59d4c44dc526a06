"""Layer-wise trust ratios in FlatAdam on the device (avmoe_amd.train.FlatAdam(trust_ratio=..., trust_clip=...); include/avmoe.h:
avmoe_opt_lamb_step) on two buckets of plain parameters, the smallest that reach every path of the three kernels (a block serves 1024
elements, a thread four, and a lane of the ratio kernel more than one block only from 65 blocks on):
    2-D of 1, 3, 4, 5, 1023, 1024, 1025 and 2049 elements; one of 260 x 257 (66 blocks); two 1-D ones of 5 and 1024 elements and a
    zeros(1) gate (not adapted by default); a 2-D parameter that is all zero.
The parameters are drawn at different scales (0.05 ... 20) so that the ratios spread around the clamp of 2.  Gradients are seeded, 4
steps, so that moments and bias corrections are not trivial.  Two ranges are special on purpose: the all-zero parameter gets zero
gradients until the last step (its weights have norm 0 when the checked step starts), and the 5-element 2-D parameter has weight decay 0
and zero gradients throughout (its update has norm 0).

The fp64 bounds and the rounding count they come from are tests/lamb_ref.py's.  Everything that is the same kernels on the same bits is
held to bit-equality.  AVMOE_LAMB_MARGINS=<file> appends the worst observed fraction of each bound to that file."""
import copy
import os

import numpy as np
import pytest
import torch

from tests import lamb_ref
from tests.test_flat_adam_ema_gpu import assert_flats_equal, bits, flats, padding_mask, set_grads
from tests.test_flat_adam_swa_gpu import lr_sched, poison

pytestmark = pytest.mark.gpu

SHAPES = ((260, 257), (1, 1), (1, 3), (2, 2), (1, 5), (3, 341), (32, 32), (25, 41), (3, 683), (5,), (1024,), (1,), (3, 5))
SCALES = (1.0, 0.5, 20.0, 4.0, 1.0, 0.05, 20.0, 0.5, 4.0, 1.0, 1.0, 0.0, 0.0)
ZERO_U, GATE, ZERO_W = 4, 11, 12                 # indices into SHAPES: the zero-update range, the gate, the all-zero 2-D parameter
LR, LR_X, WD, CLIP, RHO = 3e-3, 1e-2, 1e-2, 2.0, 0.05
STEPS = 4
MAX_NORM = 20.0                                  # random gradients over 74 000 elements: norm about 270, so every step clips
BUCKET_MB = 4 * 67000 / (1 << 20)                # the twelve small ones fill the first bucket, 260 x 257 the second
_GRADS = {}


def make_params(dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter((torch.randn(s, generator=g) * c).to(dev)) for s, c in zip(SHAPES, SCALES)]


def clone_params(params):
    return [torch.nn.Parameter(p.detach().clone()) for p in params]


def make_opt(params, groups=None, **kw):
    from avmoe_amd.dp import AdapterGradReducer
    from avmoe_amd.train import FlatAdam
    red = AdapterGradReducer(params, bucket_mb=BUCKET_MB)
    assert len(red.buckets) == 2 and sorted(p.numel() for b in red.buckets for p in b.params) == sorted(int(np.prod(s)) for s in SHAPES)
    kw.setdefault("lr", LR)
    groups = [{"params": params[1:4], "lr": LR_X}, {"params": [params[ZERO_U]], "weight_decay": 0.0}] + list(groups or [])
    return red, FlatAdam(red, param_groups=groups, **kw)


def grads(dev, seed=5):
    """STEPS seeded gradient sets, drawn once per seed on the host and shared; the device copies belong to the calling test"""
    if seed not in _GRADS:
        g = torch.Generator().manual_seed(seed)
        steps = [[torch.randn(s, generator=g) for s in SHAPES] for _ in range(STEPS)]
        for k, step in enumerate(steps):
            step[ZERO_U].zero_()
            if k < STEPS - 1:
                step[ZERO_W].zero_()
        _GRADS[seed] = steps
    return [[t.to(dev) for t in step] for step in _GRADS[seed]]


def trust(opt):
    return tuple(bits(t) for t in (opt.last_param_norms, opt.last_update_norms, opt.last_trust_ratios))


def assert_state_blocks_equal(oa, ob, what=""):
    sa, sb = oa.state_block, ob.state_block
    assert set(sa) == set(sb)
    for field in sa:
        assert torch.equal(sa[field].cpu() if sa[field].dtype == torch.int64 else bits(sa[field]),
                           sb[field].cpu() if sb[field].dtype == torch.int64 else bits(sb[field])), (what, field)


def settings(name, decoupled):
    kw = dict(weight_decay=WD, decoupled_weight_decay=decoupled, trust_ratio=True, trust_clip=CLIP)
    if name == "composed":
        kw.update(lr_schedule=lr_sched(warmup_steps=6), ema_decay=0.9, max_grad_norm=MAX_NORM)      # the 4th step is inside the warm-up
    if name == "sam":
        kw.update(sam_rho=RHO, skip_nonfinite=True)
    return kw


def step(opt, params, g2, g1=None):
    if g1 is not None:
        set_grads(params, g1)
        opt.sam_perturb()
    set_grads(params, g2)
    opt.step()


def record_margins(tag, worst):
    line = tag + ": " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items())
    print(line)
    path = os.environ.get("AVMOE_LAMB_MARGINS")
    if path:
        with open(path, "a") as fh:
            fh.write(line + "\n")


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("decoupled", [False, True], ids=["coupled", "decoupled"])
@pytest.mark.parametrize("name", ["plain", "composed", "sam"])
def test_the_last_step_against_fp64_from_its_own_operands(name, decoupled):
    """tests/lamb_ref.py: norms, ratio and every element of every parameter of the 4th step, recomputed in fp64 from the fp32 values
    the device held; alignment padding of p, m, v and the shadows keeps its bits"""
    dev = torch.device("cuda:0")
    a = make_params(dev)
    red, opt = make_opt(a, **settings(name, decoupled))
    assert opt.trust_ratio is True and opt.trust_clip == CLIP
    assert opt.adapted == [p.dim() >= 2 for p in opt.params] and len(opt.params) == len(SHAPES)
    g2s, g1s = grads(dev, seed=5), grads(dev, seed=6)
    for k in range(STEPS - 1):
        step(opt, a, g2s[k], g1s[k] if name == "sam" else None)
    p0 = [p.detach().cpu().clone() for p in opt.params]                    # behind sam_perturb() the held value: taken before it
    pads = [padding_mask(b, dev) for b in red.buckets]
    keys = "pmve" if name == "composed" else "pmv"
    pad_before = [[s[k][pad].clone() for k in keys] for s, pad in zip(opt.state, pads)]
    step(opt, a, g2s[-1], g1s[-1] if name == "sam" else None)
    torch.cuda.synchronize()
    for s, pad, old in zip(opt.state, pads, pad_before):
        assert int(pad.sum()) > 0
        for k, o in zip(keys, old):
            assert torch.equal(bits(s[k][pad]), bits(o)), ("alignment padding", k)
    sb = {k: v.item() for k, v in opt.state_block.items()}
    assert sb["applied_steps"] == STEPS and sb["skip"] == 0
    assert (sb["clip_coef"] < 1.0) == (name == "composed")
    lr_factor = float(sb["lr_factor"]) if name == "composed" else 1.0
    assert opt.last_trust_ratios.dtype == torch.float32 and opt.last_trust_ratios.is_cuda and opt.last_trust_ratios.numel() == len(SHAPES)
    w_norms, u_norms, ratios = (t.cpu().tolist() for t in (opt.last_param_norms, opt.last_update_norms, opt.last_trust_ratios))
    worst, cases = {"w_norm": 0.0, "u_norm": 0.0, "ratio": 0.0, "p": 0.0}, {}
    assert len(opt.params) == len(SHAPES)
    for i, (p, si, off, lr0, wd) in enumerate((r.p, r.bucket, r.off, r.lr0, r.wd) for r in opt._recs):
        s, n = opt.state[si], p.numel()
        m1, v1 = (s[k][off:off + n].view_as(p).cpu() for k in "mv")
        used, case = lamb_ref.check_range(p0[i], p.detach().cpu(), m1, v1, w_norms[i], u_norms[i], ratios[i], lamb_ref.f32(lr0), lr_factor,
                                          lamb_ref.f32(wd), float(sb["bc1"]), float(sb["bc2_sqrt"]), lamb_ref.f32(opt.eps), decoupled,
                                          opt.adapted[i], lamb_ref.f32(CLIP))
        cases.setdefault(case, []).append(tuple(p.shape))
        for k, v in used.items():
            if v is not None:
                worst[k] = max(worst[k], v)
        if case == "free":        # the host's copy of the rule, from the fp32 norms (each within u of the double one: 2 ulp, and a rounding)
            assert lamb_ref.ulps(ratios[i], type(opt).trust_ratio_of(w_norms[i], u_norms[i], CLIP)) <= 3
    print(cases)
    # every case of the rule was met: not adapted, zero weights, zero update, clamped, not clamped
    assert sorted(cases["off"]) == sorted(s for s in SHAPES if len(s) < 2)
    assert cases["zero_w"] == [SHAPES[ZERO_W]] and cases["zero_u"] == [SHAPES[ZERO_U]]
    assert len(cases.get("clamped", [])) >= 2 and len(cases.get("free", [])) >= 2 and (260, 257) in cases["free"] + cases.get("clamped", [])
    record_margins(f"{name} {'decoupled' if decoupled else 'coupled'}", worst)


@pytest.mark.parametrize("decoupled", [True, False], ids=["decoupled", "coupled"])
def test_the_moments_are_adams(decoupled):
    """decoupled decay: m and v do not depend on p, and are bit-equal to a FlatAdam's without the option after every one of the 4 steps;
    coupled: after the first step, from equal parameters.  The state block and last_grad_norm agree too (the option writes neither)."""
    dev = torch.device("cuda:0")
    kw = dict(weight_decay=WD, decoupled_weight_decay=decoupled, max_grad_norm=MAX_NORM, skip_nonfinite=True)
    a = make_params(dev)
    b = clone_params(a)
    _, oa = make_opt(a, trust_ratio=True, **kw)
    _, ob = make_opt(b, **kw)
    assert oa._flags == ob._flags
    gs = grads(dev)
    for k in range(STEPS if decoupled else 1):
        step(oa, a, gs[k]); step(ob, b, gs[k])
        assert_flats_equal(flats(oa, "mv"), flats(ob, "mv"), k, "mv")
        assert_state_blocks_equal(oa, ob, k)
        assert torch.equal(bits(oa.last_grad_norm), bits(ob.last_grad_norm))
    assert any(not torch.equal(x["p"], y["p"]) for x, y in zip(oa.state, ob.state))      # the update itself is another one
    assert int(oa.applied_steps.item()) == (STEPS if decoupled else 1) and int(oa.skipped_steps.item()) == 0 and oa.t == ob.t


def test_a_skipped_step_leaves_every_bit():
    dev = torch.device("cuda:0")
    a = make_params(dev)
    _, opt = make_opt(a, weight_decay=WD, max_grad_norm=MAX_NORM, skip_nonfinite=True, ema_decay=0.9, trust_ratio=True)
    gs = grads(dev)
    step(opt, a, gs[0]); step(opt, a, gs[1])
    before, report = flats(opt, "pmve"), opt._trust_report.clone()
    set_grads(a, gs[2])
    poison(a[6])
    opt.step()
    assert_flats_equal(before, flats(opt, "pmve"), "skipped step")
    assert torch.equal(report, opt._trust_report)
    assert int(opt.skipped_steps.item()) == 1 and int(opt.applied_steps.item()) == 2 and int(opt.state_block["skip"].item()) == 1
    step(opt, a, gs[3])                                       # and the run goes on
    assert int(opt.applied_steps.item()) == 3 and not torch.equal(report, opt._trust_report)


@pytest.mark.parametrize("decoupled", [False, True], ids=["coupled", "decoupled"])
def test_the_step_behind_a_perturbation_is_the_step_without_it(decoupled):
    """A: g1, sam_perturb(), g2, step().  B, without SAM: g2, step().  Parameters, moments, averages, the trust report and the state block
    are bit-equal after every step; a skipped step of A restores the held weights."""
    dev = torch.device("cuda:0")
    kw = dict(weight_decay=WD, decoupled_weight_decay=decoupled, max_grad_norm=MAX_NORM, skip_nonfinite=True, ema_decay=0.9, trust_ratio=True,
              trust_clip=CLIP)
    a = make_params(dev)
    b = clone_params(a)
    _, oa = make_opt(a, sam_rho=RHO, **kw)
    _, ob = make_opt(b, **kw)
    g2s, g1s = grads(dev, seed=5), grads(dev, seed=6)
    for k in range(STEPS):
        set_grads(a, g1s[k])
        before = flats(oa, "p")
        oa.sam_perturb()
        assert oa.perturbed and any(not torch.equal(x[0], s["p"]) for x, s in zip(before, oa.state))
        set_grads(a, g2s[k]); set_grads(b, g2s[k])
        if k == 2:
            poison(a[6]); poison(b[6])
        oa.step(); ob.step()
        assert not oa.perturbed
        assert_flats_equal(flats(oa, "pmve"), flats(ob, "pmve"), k)
        assert all(torch.equal(x, y) for x, y in zip(trust(oa), trust(ob))), k
        if k == 2:
            assert_flats_equal(before, flats(oa, "p"), "a skipped step restores", "p")
    assert_state_blocks_equal(oa, ob)
    assert int(oa.applied_steps.item()) == STEPS - 1 and int(oa.skipped_steps.item()) == 1


def test_a_captured_step_replays_bit_equal_to_the_eager_run():
    dev = torch.device("cuda:0")
    kw = dict(weight_decay=WD, decoupled_weight_decay=True, max_grad_norm=MAX_NORM, skip_nonfinite=True, ema_decay=0.9, lr_schedule=lr_sched(),
              trust_ratio=True, trust_clip=CLIP)
    a = make_params(dev)
    b = clone_params(a)
    _, oa = make_opt(a, **kw)
    _, ob = make_opt(b, **kw)
    gs = grads(dev)
    start = flats(ob, "pmve")
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    eager = []
    with torch.cuda.stream(st):                              # the eager run (it also loads the kernels before the capture)
        for k in range(STEPS):
            step(oa, a, gs[k])
            eager.append(trust(oa))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=st):
        ob.step()
    torch.cuda.synchronize()
    assert int(ob.applied_steps.item()) == 0                  # capturing runs nothing
    assert_flats_equal(start, flats(ob, "pmve"), "capture")
    for k in range(STEPS):
        set_grads(b, gs[k])
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(x, y) for x, y in zip(trust(ob), eager[k])), k
    assert int(ob.applied_steps.item()) == STEPS
    assert_flats_equal(flats(oa, "pmve"), flats(ob, "pmve"), "graph replay")
    assert_state_blocks_equal(oa, ob, "graph replay")
    assert len({tuple(e[2].tolist()) for e in eager}) == STEPS           # the ratios did change from replay to replay


def test_resume_continues_bit_equal_and_torch_loads_the_dict():
    dev = torch.device("cuda:0")
    kw = dict(weight_decay=WD, decoupled_weight_decay=True, max_grad_norm=MAX_NORM, ema_decay=0.9, trust_ratio=True)
    a = make_params(dev)
    b = clone_params(a)
    _, oa = make_opt(a, trust_clip=CLIP, **kw)
    _, ob = make_opt(b, trust_clip=CLIP, **kw)
    gs = grads(dev)
    for k in range(2):
        step(oa, a, gs[k]); step(ob, b, gs[k])
    sd = ob.state_dict()
    extra = sd["flat_adam"]
    assert extra["trust_ratio"] is True and extra["trust_clip"] == CLIP
    assert not any(isinstance(v, torch.Tensor) for k, v in extra.items() if k.startswith("trust_"))      # no tensor state
    _, oc = make_opt(b, trust_clip=0.5, **kw)                # a fresh reducer + optimizer built with ANOTHER clamp: the saved one wins
    oc.load_state_dict(copy.deepcopy(sd))
    assert oc.trust_clip == CLIP and int(oc.applied_steps.item()) == 2
    for k in range(2, STEPS):
        step(oa, a, gs[k]); step(oc, b, gs[k])
        assert all(torch.equal(x, y) for x, y in zip(trust(oa), trust(oc))), k
    assert_flats_equal(flats(oa, "pmve"), flats(oc, "pmve"), "resumed run")
    assert_state_blocks_equal(oa, oc, "resumed run")
    # a dict without the keys loads as before and leaves the constructor's clamp; an optimizer without the option ignores saved ones,
    # and its own dict is what it was
    bare = copy.deepcopy(sd)
    del bare["flat_adam"]["trust_ratio"], bare["flat_adam"]["trust_clip"]
    _, od = make_opt(clone_params(b), trust_clip=0.5, **kw)
    od.load_state_dict(bare)
    assert od.trust_clip == 0.5 and int(od.applied_steps.item()) == 2
    kw.pop("trust_ratio")
    _, oe = make_opt(clone_params(b), **kw)
    oe.load_state_dict(copy.deepcopy(sd))
    assert oe.trust_ratio is False and int(oe.applied_steps.item()) == 2
    assert not any(k.startswith("trust_") for k in oe.state_dict()["flat_adam"])
    torch.optim.AdamW(ob.torch_param_groups()).load_state_dict(copy.deepcopy(sd))
    from avmoe_amd import _capi as capi
    for what in (lambda: oe.last_trust_ratios, lambda: oe.last_param_norms, lambda: oe.last_update_norms):
        with pytest.raises(capi.AvmoeError, match="trust_ratio"):
            what()


def test_a_groups_override_and_the_invariants_of_the_first_step():
    """"trust_ratio": False on a 2-D parameter gives ratio exactly 1.0 and True on a 1-D one adapts it; last_grad_norm, the counters and
    every word of the state block are what a run without the option gives on the same gradients at step 1"""
    dev = torch.device("cuda:0")
    kw = dict(weight_decay=WD, max_grad_norm=MAX_NORM, skip_nonfinite=True, lr_schedule=lr_sched())
    a = make_params(dev)
    b = clone_params(a)
    _, oa = make_opt(a, groups=[{"params": [a[0], a[6]], "trust_ratio": False}, {"params": [a[10]], "trust_ratio": True}], trust_ratio=True, **kw)
    _, ob = make_opt(b, **kw)
    override = {id(a[0]): False, id(a[6]): False, id(a[10]): True}
    assert oa.adapted == [override.get(id(p), p.dim() >= 2) for p in oa.params] and ob.trust_ratio is False
    gs = grads(dev)
    step(oa, a, gs[0]); step(ob, b, gs[0])
    ratios = dict(zip((id(p) for p in oa.params), oa.last_trust_ratios.tolist()))
    assert ratios[id(a[0])] == 1.0 and ratios[id(a[6])] == 1.0 and ratios[id(a[9])] == 1.0 and ratios[id(a[GATE])] == 1.0
    assert ratios[id(a[10])] != 1.0 and ratios[id(a[7])] != 1.0
    assert_state_blocks_equal(oa, ob, "step 1")
    assert torch.equal(bits(oa.last_grad_norm), bits(ob.last_grad_norm)) and float(oa.last_grad_norm.item()) > MAX_NORM
    assert int(oa.applied_steps.item()) == 1 and int(oa.skipped_steps.item()) == 0 and oa.t == 1


def test_the_averages_follow_the_fp64_recurrence():
    """with ema_decay the shadows stay within 6 T 2^-24 max|p| of the fp64 recurrence over the parameter snapshots (the bound of
    tests/test_flat_adam_ema_gpu.py: the average's own arithmetic is unchanged)"""
    from avmoe_amd.train import FlatAdam
    dev = torch.device("cuda:0")
    a = make_params(dev)
    _, opt = make_opt(a, weight_decay=WD, decoupled_weight_decay=True, max_grad_norm=MAX_NORM, ema_decay=0.9, trust_ratio=True, trust_clip=CLIP)
    gs = grads(dev)
    ref = [p.detach().double().cpu() for p in opt.params]
    A = max(float(r.abs().max()) for r in ref)
    for k in range(STEPS):
        step(opt, a, gs[k])
        d = FlatAdam.ema_decay_at(k + 1, 0.9, 10.0)
        assert int(bits(opt.last_ema_decay).item()) == int(np.float32(d).view(np.int32))
        for i, p in enumerate(opt.params):
            p64 = p.detach().double().cpu()
            ref[i] = d * ref[i] + (1.0 - d) * p64
            A = max(A, float(p64.abs().max()), float(opt.ema_params[i].abs().max()))
    bound = 6 * STEPS * 2.0 ** -24 * A
    for i, (e, r) in enumerate(zip(opt.ema_params, ref)):
        err = float((e.double().cpu() - r).abs().max())
        assert err <= bound, (i, e.numel(), err, bound)
    for p, e in zip(opt.params, opt.ema_params):             # and the average did move, behind the parameters
        if p.numel() > 5:
            assert not torch.equal(e, p.data)


def test_a_launch_that_does_not_match_touches_nothing():
    """the guards of the three kernels: a table whose header is not this launch's (a stale image: wrong magic), a range count that is not
    the table's (pointer arrays made for another table), and a shadow entry that cannot take 16-byte accesses (that range alone is left
    out, moments included) leave parameters, moments, averages and the report bit for bit"""
    from avmoe_amd import _capi as capi
    from avmoe_amd import _capi_moe as cm
    dev = torch.device("cuda:0")
    a = make_params(dev)
    _, opt = make_opt(a, weight_decay=WD, max_grad_norm=MAX_NORM, ema_decay=0.9, trust_ratio=True, trust_clip=CLIP)
    gs = grads(dev)
    step(opt, a, gs[0])
    before, report = flats(opt, "pmve"), opt._trust_report.clone()
    set_grads(a, gs[1])
    magic = opt._ws[cm.OPT_STATE_BYTES:cm.OPT_STATE_BYTES + 4].clone()
    opt._ws[cm.OPT_STATE_BYTES:cm.OPT_STATE_BYTES + 4] = 0
    opt.step()                                                # finalize still counts the step; the table's kernels refuse
    opt._ws[cm.OPT_STATE_BYTES:cm.OPT_STATE_BYTES + 4] = magic
    assert_flats_equal(before, flats(opt, "pmve"), "stale table")
    assert torch.equal(report, opt._trust_report)
    L, n = capi.lib(), len(opt.params)
    stream = torch.cuda.current_stream().cuda_stream

    def call(n_ranges, shadows):
        capi.check(L.avmoe_opt_lamb_step(opt._table_ptr, n_ranges, opt._n_blocks, opt._state_ptr, opt.betas[0], opt.betas[1], opt.eps, 1.0,
                                         cm.OPT_CLIP | cm.OPT_EMA, stream, shadows.data_ptr(), None, opt._trust_limits.data_ptr(),
                                         opt._trust_ws.data_ptr(), opt._trust_report.data_ptr()), "avmoe_opt_lamb_step")

    call(n - 1, opt._shadow_ptrs)
    assert_flats_equal(before, flats(opt, "pmve"), "another range count")
    assert torch.equal(report, opt._trust_report)
    bent = opt._shadow_ptrs.clone()
    victim = max(range(n), key=lambda i: opt.params[i].numel())          # the 66-block range
    bent[victim] += 4
    call(n, bent)
    torch.cuda.synchronize()
    p, si, off = opt._recs[victim].p, opt._recs[victim].bucket, opt._recs[victim].off
    for k, (old, s) in zip("pmve", zip(before[si], (opt.state[si][k] for k in "pmve"))):
        assert torch.equal(bits(old[off:off + p.numel()]), bits(s[off:off + p.numel()])), ("the range with the bent shadow entry", k)
    other = 1 - si
    assert not torch.equal(before[other][0], opt.state[other]["p"])      # the other ranges took their step
    assert not torch.equal(report, opt._trust_report)
