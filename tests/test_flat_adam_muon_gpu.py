"""Orthogonalised momentum in FlatAdam on the device (avmoe_amd.train.FlatAdam(muon=...); include/avmoe.h: avmoe_opt_muon_step,
avmoe_opt_muon_ns) on two buckets of plain parameters, 4 seeded steps:
    orthogonalised: (4, 32), (87, 200) and (200, 87) (either orientation, 87 is no multiple of 16, 18 table blocks each), (16, 16),
    (3, 7), a conv weight (24, 6, 1, 1), (128, 130) (the largest short side, two chunks of its long side) and (2, 3);
    Adam: (130, 129) (short side above 128), two 1-D ones of 5 and 1024 elements and a zeros(1) gate.
The fp64 reference and the fp32 yardstick of the bounds are tests/muon_ref.py's.  Everything that is the same kernels on the same bits
is held to bit-equality.  AVMOE_MUON_MARGINS=<file> appends the worst observed fraction of each bound to that file."""
import copy
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import muon_ref as R
from tests.test_flat_adam_ema_gpu import assert_flats_equal, bits, flats, padding_mask, set_grads
from tests.test_flat_adam_lamb_gpu import assert_state_blocks_equal, clone_params
from tests.test_flat_adam_swa_gpu import lr_sched, poison

pytestmark = pytest.mark.gpu

SHAPES = ((4, 32), (87, 200), (5,), (16, 16), (3, 7), (24, 6, 1, 1), (1024,), (1,), (200, 87), (130, 129), (128, 130), (2, 3))
ORTHO = [len(s) >= 2 and min(s[0], int(np.prod(s[1:]))) <= 128 for s in SHAPES]
GATE = 7
LR, LR_X, WD, RHO, MU = 3e-3, 1e-2, 1e-2, 0.05, 0.95
STEPS = 4
MAX_NORM = 20.0                                  # random gradients over 70 000 elements: norm about 265, so every step clips
BUCKET_MB = 4 * 40000 / (1 << 20)                # (2, 3), (128, 130), (130, 129) fill one bucket, the other nine the second
NS_FACTOR = 5.54                                 # the factor of the sub-op's bound: twice the worst ratio seen on an MI355X (2.77 at 3 x 7;
                                                 # DESIGN_CURRENT.md section 4b has every shape's), tightened from the 8 the bound started with
_GRADS = {}
EPS32 = 2.0 ** -24


def f32(x):
    return float(np.float32(x))


def make_params(dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter((torch.randn(s, generator=g) * (0.0 if i == GATE else 0.5)).to(dev)) for i, s in enumerate(SHAPES)]


def make_opt(params, groups=None, **kw):
    from avmoe_amd.dp import AdapterGradReducer
    from avmoe_amd.train import FlatAdam
    red = AdapterGradReducer(params, bucket_mb=BUCKET_MB)
    assert len(red.buckets) == 2 and sorted(p.numel() for b in red.buckets for p in b.params) == sorted(int(np.prod(s)) for s in SHAPES)
    kw.setdefault("lr", LR)
    groups = [{"params": params[1:4], "lr": LR_X}, {"params": [params[4]], "weight_decay": 0.0}] + list(groups or [])
    return red, FlatAdam(red, param_groups=groups, **kw)


def grads(dev, seed=5):
    """STEPS seeded gradient sets, drawn once per seed on the host and shared; the device copies belong to the calling test"""
    if seed not in _GRADS:
        g = torch.Generator().manual_seed(seed)
        _GRADS[seed] = [[torch.randn(s, generator=g) for s in SHAPES] for _ in range(STEPS)]
    return [[t.to(dev) for t in step] for step in _GRADS[seed]]


def settings(name, decoupled):
    kw = dict(weight_decay=WD, decoupled_weight_decay=decoupled, muon=True)
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


def muon_out(opt):
    """the bits of everything the option leaves beside p, m, v, e: the work buffers and the report"""
    return [bits(s["o"]) for s in opt.state] + [opt._muon_report.clone()]


def record_margins(tag, worst):
    line = tag + ": " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items())
    print(line)
    path = os.environ.get("AVMOE_MUON_MARGINS")
    if path:
        with open(path, "a") as fh:
            fh.write(line + "\n")


# ---- 1. the sub-op ---------------------------------------------------------------------------------------------------
NS_SHAPES = [(4, 32), (1, 64), (16, 16), (32, 128), (87, 200), (200, 87), (768, 32), (128, 128), (128, 1000), (96, 1536), (3, 7)]
KINDS = ("gauss", "lowrank", "rowscale", "zeros")
POISON = 0x7fc0dead                              # a NaN with a payload, as int32


@pytest.mark.parametrize("shape", NS_SHAPES, ids=[f"{r}x{c}" for r, c in NS_SHAPES])
def test_the_iteration_alone_against_fp64(shape):
    """avmoe_opt_muon_ns on four matrices of one shape (Gaussian; rank d/4 plus 1e-3 noise; rows scaled by exp(2 N(0,1)) 1e-4; zeros) in
    one work buffer with poisoned gaps: every element within NS_FACTOR max(max|O32 - O64|, 1e-5 rms(O64)) of the fp64 result of the same fp32
    input, zeros give zeros, no NaN, and nothing outside the matrices is written"""
    from avmoe_amd import _capi as capi
    from avmoe_amd import _capi_moe as cm
    dev = torch.device("cuda:0")
    L = capi.lib()
    rows, cols = shape
    n = rows * cols
    stride = (n + 3) // 4 * 4 + 20                                         # 16-byte aligned slices with a gap of at least 20 words
    rng = np.random.default_rng(rows * 10007 + cols)
    ins = [R.inputs(kind, rows, cols, rng) for kind in KINDS]
    host = np.full(8 + stride * len(KINDS), POISON, dtype=np.int32)
    for k, x in enumerate(ins):
        host[8 + k * stride:8 + k * stride + n] = x.reshape(-1).view(np.int32)
    buf = torch.from_numpy(host).to(dev)
    assert buf.data_ptr() % 16 == 0
    mats = (cm.OptMuonMat * len(KINDS))()
    for k, m in enumerate(mats):
        m.range, m.rows, m.cols = k, rows, cols
    lay = cm.OptMuonLayout()
    assert L.avmoe_opt_muon_bytes(len(KINDS), 0, len(KINDS), C.byref(lay)) > 0
    img = torch.zeros(int(lay.table_bytes), dtype=torch.uint8)
    capi.check(L.avmoe_opt_muon_table_build(None, len(KINDS), mats, len(KINDS), img.data_ptr(), int(lay.table_bytes)), "avmoe_opt_muon_table_build")
    image = img.to(dev)
    ptrs = torch.tensor([buf.data_ptr() + 4 * (8 + k * stride) for k in range(len(KINDS))], dtype=torch.int64).to(dev)
    capi.check(L.avmoe_opt_muon_ns(image.data_ptr(), len(KINDS), ptrs.data_ptr(), 5, torch.cuda.current_stream().cuda_stream), "avmoe_opt_muon_ns")
    torch.cuda.synchronize()
    out = buf.cpu().numpy()
    inside = np.zeros(out.size, dtype=bool)
    worst = 0.0
    for k, (kind, x) in enumerate(zip(KINDS, ins)):
        sl = slice(8 + k * stride, 8 + k * stride + n)
        inside[sl] = True
        o = out[sl].view(np.float32).reshape(rows, cols).astype(np.float64)
        assert np.isfinite(o).all(), kind
        if kind == "zeros":
            assert not o.any()
            continue
        o64, tol = R.ns_tolerance(x, 5, NS_FACTOR)
        err = float(np.max(np.abs(o - o64)))
        print(f"{shape} {kind}: err {err:.3e} of {tol:.3e} (rms {R.rms(o64):.3e})")
        worst = max(worst, err / tol)
        assert err <= tol, (kind, err, tol)
        assert np.linalg.svd(o, compute_uv=False).max() <= 1.25, kind
    assert (out[~inside] == POISON).all()
    record_margins(f"ns {rows}x{cols}", {"O": worst * NS_FACTOR})          # in units of the yardstick max(|O32 - O64|, 1e-5 rms)


# ---- 2. the last step from its own operands --------------------------------------------------------------------------
def _fma32(a, b, c):
    """fp32 fused multiply-add of fp32 arrays: the product of two fp32 values is exact in double, one rounding after the sum (double
    rounding can move the last bit in rare cases: comparisons against it allow one ulp)"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def _device_u(p0, m0, g, mu, wd, gscale, decoupled, nesterov):
    """m and u as kk_opt_muon_update forms them (muon_elem), operation by operation in fp32"""
    mu, wd, gscale = np.float32(mu), np.float32(wd), np.float32(gscale)
    gr = g * gscale if decoupled else _fma32(np.full_like(g, gscale), g, wd * p0)
    t = (np.float32(1.0) - mu) * gr
    m1 = _fma32(np.full_like(m0, mu), m0, t)
    return m1, (_fma32(np.full_like(m1, mu), m1, t) if nesterov else m1)


@pytest.mark.parametrize("decoupled", [False, True], ids=["coupled", "decoupled"])
@pytest.mark.parametrize("name", ["plain", "composed", "sam"])
def test_the_last_step_against_fp64_from_its_own_operands(name, decoupled):
    """m, ||u||_F, O and every element of every orthogonalised parameter of the 4th step from the fp32 values the device held: m within
    an ulp of its fp32 restatement, the norm within 1e-6 (three roundings per element of u, one of the report), O within the sub-op's
    bound for the u the device formed, w within that bound times lr s plus 2 ulp of w (the decay factor, its product, the step's
    product and the difference: four roundings of half an ulp).  Alignment padding of p, m, v, o and the shadows keeps its bits."""
    dev = torch.device("cuda:0")
    a = make_params(dev)
    red, opt = make_opt(a, **settings(name, decoupled))
    assert opt.muon is True and len(opt.params) == len(SHAPES)
    assert opt.orthogonalized == [ORTHO[SHAPES.index(tuple(p.shape))] for p in opt.params]
    g2s, g1s = grads(dev, seed=5), grads(dev, seed=6)
    for k in range(STEPS - 1):
        step(opt, a, g2s[k], g1s[k] if name == "sam" else None)
    p0 = [p.detach().cpu().numpy().copy() for p in opt.params]             # behind sam_perturb() the held value: taken before it
    m0 = [r.view("m").cpu().numpy().copy() for r in opt._recs]
    pads = [padding_mask(b, dev) for b in red.buckets]
    keys = "pmvoe" if name == "composed" else "pmvo"
    pad_before = [[s[k][pad].clone() for k in keys] for s, pad in zip(opt.state, pads)]
    step(opt, a, g2s[-1], g1s[-1] if name == "sam" else None)
    torch.cuda.synchronize()
    for s, pad, old in zip(opt.state, pads, pad_before):
        assert int(pad.sum()) > 0
        for k, o in zip(keys, old):
            assert torch.equal(bits(s[k][pad]), bits(o)), ("alignment padding", k)
    sb = {k: v.item() for k, v in opt.state_block.items()}
    assert sb["applied_steps"] == STEPS and sb["skip"] == 0 and (sb["clip_coef"] < 1.0) == (name == "composed")
    lr_factor = f32(sb["lr_factor"]) if name == "composed" else 1.0
    gscale = f32(np.float32(opt.grad_scale) * np.float32(sb["clip_coef"]))
    norms, scales = opt.last_muon_norms.cpu().tolist(), opt.muon_scales
    assert opt.last_muon_norms.dtype == torch.float32 and opt.last_muon_norms.is_cuda and len(norms) == len(SHAPES)
    worst = {"m": 0.0, "norm": 0.0, "O": 0.0, "w": 0.0}
    seen = 0
    for i, (p, si, off, lr0, wd) in enumerate((r.p, r.bucket, r.off, r.lr0, r.wd) for r in opt._recs):
        s, n = opt.state[si], p.numel()
        assert not s["v"][off:off + n].any() or not opt.orthogonalized[i]  # exp_avg_sq of an orthogonalised parameter stays zero
        if not opt.orthogonalized[i]:
            assert opt.last_muon_updates[i] is None and norms[i] == 0.0 and scales[i] == 0.0
            continue
        seen += 1
        g = g2s[-1][SHAPES.index(tuple(p.shape))].cpu().numpy()
        m1_dev = s["m"][off:off + n].view_as(p).cpu().numpy()
        O_dev = opt.last_muon_updates[i].cpu().numpy().astype(np.float64)
        assert O_dev.shape == tuple(p.shape)
        m1, u = _device_u(p0[i], m0[i], g, MU, wd, gscale, decoupled, True)
        tol_m = np.spacing(np.abs(m1)) + 1e-45
        worst["m"] = max(worst["m"], float(np.max(np.abs(m1_dev.astype(np.float64) - m1) / tol_m)))
        assert (np.abs(m1_dev.astype(np.float64) - m1) <= tol_m).all(), (i, "m")
        # the same momentum from the reference in fp64: the restatement above is the rule
        ref = R.step(p0[i], m0[i], g, lr=f32(np.float32(f32(lr0)) * np.float32(lr_factor)), wd=f32(wd), mu=f32(MU), nesterov=True,
                     scale=opt.muon_scale, decoupled=decoupled, gscale=gscale)
        assert np.max(np.abs(ref["m"] - m1)) <= 4 * EPS32 * max(np.max(np.abs(ref["m"])), 1e-30)
        nrm = float(np.sqrt(np.sum(u.astype(np.float64) ** 2)))
        worst["norm"] = max(worst["norm"], abs(norms[i] - nrm) / (1e-6 * nrm))
        assert abs(norms[i] - nrm) <= 1e-6 * nrm and abs(nrm - ref["norm"]) <= 1e-6 * nrm, (i, norms[i], nrm)
        o64, tol = R.ns_tolerance(R.as_matrix(u), opt.muon_ns_steps, NS_FACTOR)
        o64 = o64.reshape(p.shape)
        err = float(np.max(np.abs(O_dev - o64)))
        worst["O"] = max(worst["O"], err / tol)
        assert err <= tol, (i, tuple(p.shape), "O", err, tol)
        lr = f32(np.float32(f32(lr0)) * np.float32(lr_factor))
        assert abs(scales[i] - ref["s"]) <= 1e-7 * ref["s"]
        w64 = p0[i].astype(np.float64) * (1.0 - lr * f32(wd)) if decoupled else p0[i].astype(np.float64)
        w64 = w64 - lr * scales[i] * o64
        w_dev = p.detach().cpu().numpy().astype(np.float64)
        tol_w = tol * lr * scales[i] + 2.0 * np.spacing(np.maximum(np.abs(p0[i]), np.abs(w64).astype(np.float32)))
        worst["w"] = max(worst["w"], float(np.max(np.abs(w_dev - w64) / tol_w)))
        assert (np.abs(w_dev - w64) <= tol_w).all(), (i, tuple(p.shape), "w")
        assert not np.array_equal(w_dev, p0[i].astype(np.float64))          # and the parameter did move
    assert seen == sum(ORTHO) == 8
    record_margins(f"step {name} {'decoupled' if decoupled else 'coupled'}", worst)


# ---- 3. nothing else moves -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("decoupled", [False, True], ids=["coupled", "decoupled"])
def test_the_other_parameters_take_adams_bits(decoupled):
    """the mixed model against a run without the option on the same gradients: the parameters that are not orthogonalised, their
    moments and their shadows are bit-equal after every one of the 4 steps, the state block too; exp_avg_sq of the others stays zero"""
    dev = torch.device("cuda:0")
    kw = dict(weight_decay=WD, decoupled_weight_decay=decoupled, max_grad_norm=MAX_NORM, skip_nonfinite=True, ema_decay=0.9, lr_schedule=lr_sched())
    a = make_params(dev)
    b = clone_params(a)
    _, oa = make_opt(a, muon=True, **kw)
    _, ob = make_opt(b, **kw)
    assert oa._flags == ob._flags
    gs = grads(dev)
    for k in range(STEPS):
        step(oa, a, gs[k]); step(ob, b, gs[k])
        for i, ((p, si, off), (q, sj, offb)) in enumerate(zip(((r.p, r.bucket, r.off) for r in oa._recs), ((r.p, r.bucket, r.off) for r in ob._recs))):
            assert p.shape == q.shape
            n = p.numel()
            if oa.orthogonalized[i]:
                assert not oa.state[si]["v"][off:off + n].any()
                assert not torch.equal(oa.state[si]["p"][off:off + n], ob.state[sj]["p"][offb:offb + n])      # another step
                continue
            for key in "pmve":
                assert torch.equal(bits(oa.state[si][key][off:off + n]), bits(ob.state[sj][key][offb:offb + n])), (k, i, key)
        assert_state_blocks_equal(oa, ob, k)
    assert int(oa.applied_steps.item()) == STEPS


def test_every_group_switched_off_is_the_optimizer_without_the_option():
    dev = torch.device("cuda:0")
    kw = dict(weight_decay=WD, max_grad_norm=MAX_NORM, skip_nonfinite=True, ema_decay=0.9)
    a = make_params(dev)
    b = clone_params(a)
    off = [{"params": a[1:4], "lr": LR_X, "muon": False}, {"params": a[:1] + a[4:], "muon": False}]      # (a group without "lr" takes the default)
    _, oa = make_opt(a, groups=off, muon=True, **kw)
    _, ob = make_opt(b, **kw)
    assert oa.orthogonalized == [False] * len(SHAPES) and oa.muon_scales == [0.0] * len(SHAPES)
    gs = grads(dev)
    for k in range(STEPS):
        step(oa, a, gs[k]); step(ob, b, gs[k])
    assert_flats_equal(flats(oa, "pmve"), flats(ob, "pmve"), "all off")
    assert_state_blocks_equal(oa, ob, "all off")
    assert all(not s["o"].any() for s in oa.state) and not oa.last_muon_norms.any()


# ---- 4. skipping -----------------------------------------------------------------------------------------------------
def test_a_skipped_step_leaves_every_bit():
    dev = torch.device("cuda:0")
    a = make_params(dev)
    _, opt = make_opt(a, weight_decay=WD, max_grad_norm=MAX_NORM, skip_nonfinite=True, ema_decay=0.9, muon=True)
    gs = grads(dev)
    step(opt, a, gs[0]); step(opt, a, gs[1])
    before, out = flats(opt, "pmveo"), muon_out(opt)
    set_grads(a, gs[2])
    poison(a[1])
    opt.step()
    assert_flats_equal(before, flats(opt, "pmveo"), "skipped step", "pmveo")
    assert all(torch.equal(x, y) for x, y in zip(out, muon_out(opt)))
    assert int(opt.skipped_steps.item()) == 1 and int(opt.applied_steps.item()) == 2 and int(opt.state_block["skip"].item()) == 1
    step(opt, a, gs[3])                                       # and the run goes on
    assert int(opt.applied_steps.item()) == 3 and not all(torch.equal(x, y) for x, y in zip(out, muon_out(opt)))


@pytest.mark.parametrize("decoupled", [False, True], ids=["coupled", "decoupled"])
def test_the_step_behind_a_perturbation_is_the_step_without_it(decoupled):
    """A: g1, sam_perturb(), g2, step().  B, without SAM: g2, step().  Everything is bit-equal after every step; a skipped step of A
    restores the held weights and nothing else"""
    dev = torch.device("cuda:0")
    kw = dict(weight_decay=WD, decoupled_weight_decay=decoupled, max_grad_norm=MAX_NORM, skip_nonfinite=True, ema_decay=0.9, muon=True)
    a = make_params(dev)
    b = clone_params(a)
    _, oa = make_opt(a, sam_rho=RHO, **kw)
    _, ob = make_opt(b, **kw)
    g2s, g1s = grads(dev, seed=5), grads(dev, seed=6)
    for k in range(STEPS):
        set_grads(a, g1s[k])
        before = flats(oa, "pmveo")
        oa.sam_perturb()
        assert oa.perturbed and any(not torch.equal(x[0], s["p"]) for x, s in zip(before, oa.state))
        set_grads(a, g2s[k]); set_grads(b, g2s[k])
        if k == 2:
            poison(a[1]); poison(b[1])
        oa.step(); ob.step()
        assert not oa.perturbed
        assert_flats_equal(flats(oa, "pmveo"), flats(ob, "pmveo"), k, "pmveo")
        assert all(torch.equal(x, y) for x, y in zip(muon_out(oa), muon_out(ob))), k
        if k == 2:
            assert_flats_equal(before, flats(oa, "pmveo"), "a skipped step restores", "pmveo")
    assert_state_blocks_equal(oa, ob)
    assert int(oa.applied_steps.item()) == STEPS - 1 and int(oa.skipped_steps.item()) == 1


# ---- 5. capture and repetition ---------------------------------------------------------------------------------------
def test_a_captured_step_replays_bit_equal_to_the_eager_run_and_runs_repeat():
    dev = torch.device("cuda:0")
    kw = dict(weight_decay=WD, decoupled_weight_decay=True, max_grad_norm=MAX_NORM, skip_nonfinite=True, ema_decay=0.9, lr_schedule=lr_sched(), muon=True)
    a = make_params(dev)
    b, c = clone_params(a), clone_params(a)
    _, oa = make_opt(a, **kw)
    _, ob = make_opt(b, **kw)
    _, oc = make_opt(c, **kw)
    gs = grads(dev)
    start = flats(ob, "pmveo")
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    eager = []
    with torch.cuda.stream(st):                              # the eager run (it also loads the kernels before the capture)
        for k in range(STEPS):
            step(oa, a, gs[k])
            eager.append(muon_out(oa))
    torch.cuda.synchronize()
    for k in range(STEPS):                                    # a second eager run: the same bits
        step(oc, c, gs[k])
        assert all(torch.equal(x, y) for x, y in zip(muon_out(oc), eager[k])), k
    assert_flats_equal(flats(oa, "pmveo"), flats(oc, "pmveo"), "two eager runs", "pmveo")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=st):
        ob.step()
    torch.cuda.synchronize()
    assert int(ob.applied_steps.item()) == 0                  # capturing runs nothing
    assert_flats_equal(start, flats(ob, "pmveo"), "capture", "pmveo")
    for k in range(STEPS):
        set_grads(b, gs[k])
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(x, y) for x, y in zip(muon_out(ob), eager[k])), k
    assert int(ob.applied_steps.item()) == STEPS
    assert_flats_equal(flats(oa, "pmveo"), flats(ob, "pmveo"), "graph replay", "pmveo")
    assert_state_blocks_equal(oa, ob, "graph replay")
    assert not torch.equal(eager[0][-1], eager[-1][-1])       # the norms did change from replay to replay


# ---- 6. resume -------------------------------------------------------------------------------------------------------
def test_resume_continues_bit_equal_and_torch_loads_the_dict():
    dev = torch.device("cuda:0")
    kw = dict(weight_decay=WD, decoupled_weight_decay=True, max_grad_norm=MAX_NORM, ema_decay=0.9, muon=True)
    a = make_params(dev)
    b = clone_params(a)
    _, oa = make_opt(a, muon_momentum=0.9, muon_ns_steps=4, muon_scale="original", **kw)
    _, ob = make_opt(b, muon_momentum=0.9, muon_ns_steps=4, muon_scale="original", **kw)
    gs = grads(dev)
    for k in range(2):
        step(oa, a, gs[k]); step(ob, b, gs[k])
    sd = ob.state_dict()
    extra = sd["flat_adam"]
    assert extra["muon"] is True and extra["muon_momentum"] == f32(0.9) and extra["muon_ns_steps"] == 4 and extra["muon_scale"] == "original"
    assert extra["muon_nesterov"] is True and extra["muon_max_numel"] == 262144
    assert not any(isinstance(v, torch.Tensor) for k, v in extra.items() if k.startswith("muon"))       # no tensor state: exp_avg is the momentum
    for i, on in enumerate(ob.orthogonalized):
        if on:
            assert not sd["state"][i]["exp_avg_sq"].any() and sd["state"][i]["exp_avg"].any()
    _, oc = make_opt(b, **kw)                                 # a fresh reducer + optimizer built with the defaults: the saved constants win
    oc.load_state_dict(copy.deepcopy(sd))
    assert (oc.muon_momentum, oc.muon_ns_steps, oc.muon_scale, oc.muon_nesterov) == (f32(0.9), 4, "original", True)
    assert int(oc.applied_steps.item()) == 2
    for k in range(2, STEPS):
        step(oa, a, gs[k]); step(oc, b, gs[k])
        assert all(torch.equal(x[-1], y[-1]) for x, y in [(muon_out(oa), muon_out(oc))]), k
    assert_flats_equal(flats(oa, "pmve"), flats(oc, "pmve"), "resumed run")
    assert_state_blocks_equal(oa, oc, "resumed run")
    torch.optim.AdamW(ob.torch_param_groups()).load_state_dict(copy.deepcopy(sd))
    bare = copy.deepcopy(sd)                                  # a dict without the keys loads as before and leaves the constructor's constants
    for key in [k for k in bare["flat_adam"] if k.startswith("muon")]:
        del bare["flat_adam"][key]
    _, od = make_opt(clone_params(b), **kw)
    od.load_state_dict(bare)
    assert od.muon_momentum == f32(0.95) and od.muon_ns_steps == 5 and int(od.applied_steps.item()) == 2
    kw.pop("muon")
    _, oe = make_opt(clone_params(b), **kw)
    with pytest.raises(ValueError, match="muon"):
        oe.load_state_dict(copy.deepcopy(sd))
    from avmoe_amd import _capi as capi
    for what in (lambda: oe.last_muon_updates, lambda: oe.last_muon_norms):
        with pytest.raises(capi.AvmoeError, match="muon"):
            what()
    assert oe.orthogonalized == [False] * len(SHAPES)


# ---- 7. a real site --------------------------------------------------------------------------------------------------
def test_the_updates_of_a_real_site_are_nearly_orthogonal():
    from avmoe_amd.dp import AdapterGradReducer
    from avmoe_amd.train import FlatAdam
    from tests.test_flat_adam_muon_api import small_site, small_site_orthogonalized
    dev = torch.device("cuda:0")
    m = small_site().to(dev)
    named = [(n, p) for n, p in m.named_parameters() if p.requires_grad]
    red = AdapterGradReducer([p for _, p in named])
    opt = FlatAdam(red, lr=1e-3, muon=True, weight_decay=0.01, decoupled_weight_decay=True, max_grad_norm=1.0)
    name_of = {id(p): n for n, p in named}
    want = small_site_orthogonalized(m)
    assert opt.orthogonalized == [want[name_of[id(p)]] for p in opt.params] and sum(opt.orthogonalized) >= 13
    g = torch.Generator().manual_seed(3)
    with torch.no_grad():
        for p in opt.params:
            p.grad.copy_(torch.randn(p.shape, generator=g).to(dev))
    before = [p.detach().clone() for p in opt.params]
    opt.step()
    torch.cuda.synchronize()
    norms = opt.last_muon_norms.cpu()
    for i, (p, o) in enumerate(zip(opt.params, opt.last_muon_updates)):
        if o is None:
            assert norms[i] == 0.0
            continue
        mat = o.detach().cpu().double().reshape(p.shape[0], -1)
        sv = torch.linalg.svdvals(mat)
        assert torch.isfinite(mat).all() and float(sv.max()) <= 1.25, (name_of[id(p)], float(sv.max()))
        assert float(sv.max()) >= 0.3 and norms[i] > 0.0 and not torch.equal(p.detach(), before[i]), name_of[id(p)]


# ---- 8. guards -------------------------------------------------------------------------------------------------------
def test_a_launch_that_does_not_match_touches_nothing():
    """a table whose header is not this launch's (wrong magic), a matrix image whose header is not (wrong magic), another range count,
    another matrix count and a work entry that cannot take 16-byte accesses (that matrix alone is left out by both launches) leave
    parameters, moments, averages, work buffers and the report bit for bit; bad arguments return their codes before any launch"""
    from avmoe_amd import _capi as capi
    from avmoe_amd import _capi_moe as cm
    dev = torch.device("cuda:0")
    a = make_params(dev)
    _, opt = make_opt(a, weight_decay=WD, max_grad_norm=MAX_NORM, ema_decay=0.9, muon=True)
    gs = grads(dev)
    step(opt, a, gs[0])
    before, out = flats(opt, "pmveo"), muon_out(opt)
    set_grads(a, gs[1])
    magic = opt._ws[cm.OPT_STATE_BYTES:cm.OPT_STATE_BYTES + 4].clone()
    opt._ws[cm.OPT_STATE_BYTES:cm.OPT_STATE_BYTES + 4] = 0
    opt.step()                                                # finalize still counts the step; the table's kernels refuse
    opt._ws[cm.OPT_STATE_BYTES:cm.OPT_STATE_BYTES + 4] = magic
    assert_flats_equal(before, flats(opt, "pmveo"), "stale table", "pmveo")
    assert all(torch.equal(x, y) for x, y in zip(out, muon_out(opt)))
    L, n, nm = capi.lib(), len(opt.params), len(opt._muon_order)
    stream = torch.cuda.current_stream().cuda_stream

    def call(n_ranges=n, n_mats=nm, image=None, work=None, want=0):
        got = L.avmoe_opt_muon_step(opt._table_ptr, n_ranges, opt._n_blocks, opt._state_ptr, opt.betas[0], opt.betas[1], opt.eps, 1.0,
                                    cm.OPT_CLIP | cm.OPT_EMA, stream, opt._shadow_ptrs.data_ptr(), None,
                                    (opt._muon_image if image is None else image).data_ptr(), n_mats,
                                    (opt._muon_work_ptrs if work is None else work).data_ptr(), C.byref(opt._muon_c), opt._muon_ws.data_ptr(),
                                    opt._muon_report.data_ptr())
        assert got == want, (got, capi.lib().avmoe_last_error())

    stale = opt._muon_image.clone()
    stale[:4] = 0
    call(image=stale)
    call(n_ranges=n - 1)
    call(n_mats=nm - 1)
    torch.cuda.synchronize()
    assert_flats_equal(before, flats(opt, "pmveo"), "stale image / other counts", "pmveo")
    assert all(torch.equal(x, y) for x, y in zip(out, muon_out(opt)))
    opt._muon_c.ns_steps = 17
    call(want=-1)
    opt._muon_c.ns_steps = 5
    call(image=opt._muon_image[8:], want=-3)
    assert_flats_equal(before, flats(opt, "pmveo"), "refused calls", "pmveo")
    bent = opt._muon_work_ptrs.clone()
    victim = next(i for i, p in enumerate(opt.params) if tuple(p.shape) == (87, 200))
    bent[victim] += 4
    call(work=bent)
    torch.cuda.synchronize()
    p, si, off = opt._recs[victim].p, opt._recs[victim].bucket, opt._recs[victim].off
    for k, (old, s) in zip("pmveo", zip(before[si], (opt.state[si][k] for k in "pmveo"))):
        assert torch.equal(bits(old[off:off + p.numel()]), bits(s[off:off + p.numel()])), ("the matrix with the bent work entry", k)
    q, sj, offq = next((r.p, r.bucket, r.off) for r in opt._recs if tuple(r.p.shape) == (200, 87))
    assert not torch.equal(before[sj][0][offq:offq + q.numel()], opt.state[sj]["p"][offq:offq + q.numel()])      # the others took their step
