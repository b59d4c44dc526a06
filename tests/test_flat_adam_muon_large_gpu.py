"""Orthogonalised momentum for the large matrices in FlatAdam on the device (avmoe_amd.train.FlatAdam(muon=True, muon_large=True);
include/avmoe.h: avmoe_opt_muon_step_large, avmoe_opt_muon_ns_large) on a model of plain parameters in two or more buckets:
    large: (144, 160), (256, 160) (rows > cols), a conv weight (144, 160, 1, 1), (160, 144) (the class of 144 x 160 after orientation,
    at another offset of another bucket) and (129, 130) (just above the small kernel's limit, padded in both directions);
    small: (4, 32), (87, 200), (2, 3);  Adam: two 1-D ones of 5 and 1024 elements and a zeros(1) gate.
The fp64 reference and the fp32 yardstick of the bounds are tests/muon_ref.py's.  Everything that is the same kernels on the same bits is
held to bit-equality.  AVMOE_MUON_MARGINS=<file> appends the worst observed fraction of each bound to that file."""
import copy
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest
import torch

from tests import muon_ref as R
from tests.test_flat_adam_ema_gpu import assert_flats_equal, bits, flats, padding_mask, set_grads
from tests.test_flat_adam_lamb_gpu import assert_state_blocks_equal, clone_params
from tests.test_flat_adam_muon_gpu import record_margins
from tests.test_flat_adam_swa_gpu import lr_sched, poison

pytestmark = pytest.mark.gpu

SHAPES = ((4, 32), (144, 160), (5,), (256, 160), (87, 200), (144, 160, 1, 1), (1024,), (1,), (160, 144), (129, 130), (2, 3))
PATHS = ["small", "large", None, "large", "small", "large", None, None, "large", "large", "small"]
GATE = 7
LR, LR_X, WD, RHO, MU = 3e-3, 1e-2, 1e-2, 0.05, 0.95
STEPS = 3
MAX_NORM = 20.0                                  # random gradients over 145 000 elements: norm about 380, so every step clips
BUCKET_MB = 4 * 80000 / (1 << 20)
# The factor of the sub-op's bound, in yardsticks max(max|O32 - O64|, 1e-5 rms(O64)) (muon_ref.ns_tolerance).  The bound started at the
# project's 8; the worst ratio seen on an MI355X is 2.385 (at 129 x 130; DESIGN_CURRENT.md section 4b has every shape's,
# profiles/r24_flat_adam_muon_large_margins.txt the record), below 4, so the held bound is twice it.
NS_FACTOR = 4.77
_GRADS = {}
EPS32 = 2.0 ** -24


def f32(x):
    return float(np.float32(x))


def make_params(dev, seed=0, shapes=SHAPES):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter((torch.randn(s, generator=g) * (0.0 if s == (1,) else 0.5)).to(dev)) for s in shapes]


def make_opt(params, groups=None, **kw):
    from avmoe_amd.dp import AdapterGradReducer
    from avmoe_amd.train import FlatAdam
    red = AdapterGradReducer(params, bucket_mb=BUCKET_MB)
    assert len(red.buckets) >= 2
    kw.setdefault("lr", LR)
    groups = [{"params": params[1:4], "lr": LR_X}, {"params": [params[4]], "weight_decay": 0.0}] + list(groups or [])
    return red, FlatAdam(red, param_groups=groups, **kw)


def grads(dev, seed=5, shapes=SHAPES):
    """STEPS seeded gradient sets, drawn once per seed on the host and shared; the device copies belong to the calling test"""
    key = (seed, shapes)
    if key not in _GRADS:
        g = torch.Generator().manual_seed(seed)
        _GRADS[key] = [[torch.randn(s, generator=g) for s in shapes] for _ in range(STEPS)]
    return [[t.to(dev) for t in step] for step in _GRADS[key]]


def step(opt, params, g2, g1=None):
    if g1 is not None:
        set_grads(params, g1)
        opt.sam_perturb()
    set_grads(params, g2)
    opt.step()


def muon_out(opt):
    """the bits of everything the option leaves beside p, m, v, e: the work buffers and both reports"""
    out = [bits(s["o"]) for s in opt.state] + [opt._muon_report.clone()]
    if opt._muon_large_order:
        out.append(opt._muon_large_report.clone())
    return out


def same(xs, ys):
    return len(xs) == len(ys) and all(torch.equal(x, y) for x, y in zip(xs, ys))


LARGE_KW = dict(muon=True, muon_large=True)


# ---- 1. the sub-op ---------------------------------------------------------------------------------------------------
NS_SHAPES = [(129, 130), (136, 136), (144, 160), (256, 160), (160, 256), (200, 1000), (128, 4096), (144, 160, 1, 1)]
KINDS = ("gauss", "lowrank", "rowscale", "zeros")
POISON = 0x7fc0dead                              # a NaN with a payload, as int32


def ns_large(mats, steps=5):
    """avmoe_opt_muon_ns_large on fp32 matrices [(rows, cols) arrays] laid into one buffer with poisoned gaps of different lengths (so
    that equal shapes lie at non-uniform offsets) -> (the outputs, the classes [(d, L, count, ksplit)]); nothing outside is written"""
    from avmoe_amd import _capi as capi
    from avmoe_amd import _capi_moe as cm
    dev = torch.device("cuda:0")
    L = capi.lib()
    offs, at = [], 8
    for k, x in enumerate(mats):
        offs.append(at)
        at += (x.size + 3) // 4 * 4 + 20 + 4 * ((7 * k) % 5)
    host = np.full(at, POISON, dtype=np.int32)
    for o, x in zip(offs, mats):
        host[o:o + x.size] = x.reshape(-1).view(np.int32)
    buf = torch.from_numpy(host).to(dev)
    assert buf.data_ptr() % 16 == 0
    arr = (cm.OptMuonMat * len(mats))()
    for k, (m, x) in enumerate(zip(arr, mats)):
        m.range, m.rows, m.cols = k, x.shape[0], x.shape[1]
    lay = cm.OptMuonLargeLayout()
    assert L.avmoe_opt_muon_large_bytes(len(mats), arr, len(mats), C.byref(lay)) > 0, L.avmoe_last_error()
    img = torch.zeros(int(lay.table_bytes), dtype=torch.uint8)
    capi.check(L.avmoe_opt_muon_large_table_build(None, len(mats), arr, len(mats), None, 0, img.data_ptr(), int(lay.table_bytes)),
               "avmoe_opt_muon_large_table_build")
    cls = (cm.OptMuonClass * int(lay.n_classes))()
    assert L.avmoe_opt_muon_large_classes(img.data_ptr(), cls, int(lay.n_classes), None) == lay.n_classes
    image = img.to(dev)
    ws = torch.from_numpy(np.full(int(lay.workspace_bytes) // 4, POISON, dtype=np.int32)).to(dev)      # needs no initialisation
    ptrs = torch.tensor([buf.data_ptr() + 4 * o for o in offs], dtype=torch.int64).to(dev)
    capi.check(L.avmoe_opt_muon_ns_large(image.data_ptr(), img.data_ptr(), len(mats), ptrs.data_ptr(), steps, ws.data_ptr(),
                                         torch.cuda.current_stream().cuda_stream), "avmoe_opt_muon_ns_large")
    torch.cuda.synchronize()
    out = buf.cpu().numpy()
    inside = np.zeros(out.size, dtype=bool)
    outs = []
    for o, x in zip(offs, mats):
        inside[o:o + x.size] = True
        outs.append(out[o:o + x.size].view(np.float32).reshape(x.shape).astype(np.float64))
    assert (out[~inside] == POISON).all()
    return outs, [(c.d, c.L, c.count, c.ksplit) for c in cls]


def check_ns(tag, kinds, ins, outs):
    worst = 0.0
    for kind, x, o in zip(kinds, ins, outs):
        assert np.isfinite(o).all(), (tag, kind)
        if kind == "zeros":
            assert not o.any()
            continue
        o64, tol = R.ns_tolerance(x, 5, NS_FACTOR)
        err = float(np.max(np.abs(o - o64)))
        print(f"{tag} {kind}: err {err:.3e} of {tol:.3e} (rms {R.rms(o64):.3e})")
        worst = max(worst, err / tol)
        assert err <= tol, (tag, kind, err, tol)
        assert np.linalg.svd(o, compute_uv=False).max() <= 1.25, (tag, kind)
    return worst


@pytest.mark.parametrize("shape", NS_SHAPES, ids=["x".join(str(v) for v in s) for s in NS_SHAPES])
def test_the_iteration_alone_against_fp64(shape):
    """avmoe_opt_muon_ns_large on four matrices of one shape (Gaussian; rank d/4 plus 1e-3 noise; rows scaled by exp(2 N(0,1)) 1e-4;
    zeros): one class of four at non-uniform offsets.  Every element within NS_FACTOR max(max|O32 - O64|, 1e-5 rms(O64)) of the fp64
    result of the same fp32 input, zeros give zeros, no NaN out of a poisoned workspace, and nothing outside the matrices is written"""
    from avmoe_amd.train import FlatAdam
    rows, cols = FlatAdam.muon_large_shape_of(torch.empty(shape))
    rng = np.random.default_rng(rows * 10007 + cols + len(shape))
    ins = [R.inputs(kind, rows, cols, rng) for kind in KINDS]
    outs, classes = ns_large(ins)
    assert [c[:3] for c in classes] == [(min(rows, cols), max(rows, cols), len(KINDS))]
    assert (classes[0][3] > 1) == (shape == (128, 4096))                   # the one shape here whose Gram product splits its K
    worst = check_ns("x".join(str(v) for v in shape), KINDS, ins, outs)
    record_margins("ns_large " + "x".join(str(v) for v in shape), {"O": worst * NS_FACTOR})      # in units of the yardstick


def test_two_classes_in_one_call_against_fp64():
    """three 144 x 160 beside one 256 x 160 in one call: two classes, one of more than one matrix, at non-uniform bucket offsets"""
    rng = np.random.default_rng(77)
    kinds = ("gauss", "lowrank", "gauss", "rowscale")
    ins = [R.inputs(kinds[0], 144, 160, rng), R.inputs(kinds[1], 144, 160, rng), R.inputs(kinds[2], 256, 160, rng), R.inputs(kinds[3], 144, 160, rng)]
    outs, classes = ns_large(ins)
    assert [c[:3] for c in classes] == [(144, 160, 3), (160, 256, 1)]
    worst = check_ns("3 x 144x160 + 256x160", kinds, ins, outs)
    record_margins("ns_large 3x(144x160)+256x160", {"O": worst * NS_FACTOR})


# ---- 2. one step from its own operands -------------------------------------------------------------------------------
def _round_mid(r, exact):
    """the fp32 value of `exact` (a Fraction) where its double rounding r sits on the midpoint of two fp32 values"""
    x = np.float32(r)
    lo, hi = (np.nextafter(x, np.float32(-np.inf)), x) if float(x) > r else (x, np.nextafter(x, np.float32(np.inf)))
    mid = Fraction(float(r))
    return x if exact == mid else (hi if exact > mid else lo)


def _fma32(a, b, c):
    """fp32 fused multiply-add of fp32 arrays, exactly: the product of two fp32 values is exact in double and the sum is rounded to
    double once; rounding that to fp32 is the fused result unless the double sits exactly on the midpoint of two fp32 values, where
    the exact sum (rationals) decides"""
    a, b, c = (np.ascontiguousarray(np.broadcast_to(np.asarray(x, dtype=np.float32), np.broadcast(a, b, c).shape)) for x in (a, b, c))
    r = a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)
    out = r.astype(np.float32)
    low = r.view(np.int64) & ((1 << 29) - 1)
    for idx in map(tuple, np.argwhere(low == (1 << 28))):
        out[idx] = _round_mid(float(r[idx]), Fraction(float(a[idx])) * Fraction(float(b[idx])) + Fraction(float(c[idx])))
    return out


def _device_u(p0, m0, g, mu, wd, gscale, decoupled, nesterov):
    """m and u as kk_opt_muon_update forms them (muon_elem), operation by operation in fp32"""
    mu, wd, gscale = np.float32(mu), np.float32(wd), np.float32(gscale)
    gr = g * gscale if decoupled else _fma32(gscale, g, wd * p0)
    t = (np.float32(1.0) - mu) * gr
    m1 = _fma32(mu, m0, t)
    return m1, (_fma32(mu, m1, t) if nesterov else m1)


CASES = [(name, dec, nes, sc) for name in ("plain",) for dec in (False, True) for nes in (True, False) for sc in ("match_rms_adamw", "original")] + \
        [("composed", False, True, "match_rms_adamw"), ("composed", True, True, "original")]


@pytest.mark.parametrize("name,decoupled,nesterov,scale", CASES,
                         ids=[f"{n}-{'decoupled' if d else 'coupled'}-{'nesterov' if v else 'plain_momentum'}-{s}" for n, d, v, s in CASES])
def test_one_step_against_fp64_from_its_own_operands(name, decoupled, nesterov, scale):
    """the second step of every large matrix from the fp32 values the device held: m equals its fp32 restatement bit for bit, the norm
    is within 1e-6, O within the sub-op's bound for the u the device formed, w within that bound times lr s plus 2 ulp of w (the
    bounds of tests/test_flat_adam_muon_gpu.py's step test).  "composed": schedule (inside its warm-up), average and clipping on;
    the shadow follows fma(d, shadow, (1 - d) w) bit for bit.  Alignment padding of p, m, v, o and the shadows keeps its bits."""
    dev = torch.device("cuda:0")
    a = make_params(dev)
    kw = dict(weight_decay=WD, decoupled_weight_decay=decoupled, muon_nesterov=nesterov, muon_scale=scale, **LARGE_KW)
    if name == "composed":
        kw.update(lr_schedule=lr_sched(warmup_steps=6), ema_decay=0.9, max_grad_norm=MAX_NORM)
    red, opt = make_opt(a, **kw)
    assert opt.muon_paths == [PATHS[SHAPES.index(tuple(p.shape))] for p in opt.params]
    assert opt.orthogonalized == [x is not None for x in opt.muon_paths]
    gs = grads(dev)
    step(opt, a, gs[0])
    p0 = [p.detach().cpu().numpy().copy() for p in opt.params]
    m0 = [r.view("m").cpu().numpy().copy() for r in opt._recs]
    e0 = [r.view("e").cpu().numpy().copy() for r in opt._recs] if name == "composed" else None
    pads = [padding_mask(b, dev) for b in red.buckets]
    keys = "pmvoe" if name == "composed" else "pmvo"
    pad_before = [[s[k][pad].clone() for k in keys] for s, pad in zip(opt.state, pads)]
    step(opt, a, gs[1])
    torch.cuda.synchronize()
    for s, pad, old in zip(opt.state, pads, pad_before):
        for k, o in zip(keys, old):
            assert torch.equal(bits(s[k][pad]), bits(o)), ("alignment padding", k)
    assert sum(int(pad.sum()) for pad in pads) > 0
    sb = {k: v.item() for k, v in opt.state_block.items()}
    assert sb["applied_steps"] == 2 and sb["skip"] == 0 and (sb["clip_coef"] < 1.0) == (name == "composed")
    lr_factor = f32(sb["lr_factor"]) if name == "composed" else 1.0
    assert (lr_factor < 1.0) == (name == "composed")                      # the schedule's factor is in the step
    gscale = f32(np.float32(opt.grad_scale) * np.float32(sb["clip_coef"]))
    norms, scales = opt.last_muon_norms.cpu().tolist(), opt.muon_scales
    worst = {"norm": 0.0, "O": 0.0, "w": 0.0}
    seen = 0
    for i, rec in enumerate(opt._recs):
        p, s, off, n = rec.p, opt.state[rec.bucket], rec.off, rec.p.numel()
        if opt.muon_paths[i] != "large":
            continue
        seen += 1
        assert not s["v"][off:off + n].any()                               # exp_avg_sq of an orthogonalised parameter stays zero
        g = gs[1][SHAPES.index(tuple(p.shape))].cpu().numpy()
        m1_dev = s["m"][off:off + n].view_as(p).cpu().numpy()
        O_dev = opt.last_muon_updates[i].cpu().numpy().astype(np.float64)
        assert O_dev.shape == tuple(p.shape)
        m1, u = _device_u(p0[i], m0[i], g, MU, rec.wd, gscale, decoupled, nesterov)
        assert np.array_equal(m1_dev.view(np.int32), m1.view(np.int32)), (i, "m")
        lr = f32(np.float32(f32(rec.lr0)) * np.float32(lr_factor))
        ref = R.step(p0[i], m0[i], g, lr=lr, wd=f32(rec.wd), mu=f32(MU), nesterov=nesterov, scale=scale, decoupled=decoupled, gscale=gscale)
        assert np.max(np.abs(ref["m"] - m1)) <= 4 * EPS32 * max(np.max(np.abs(ref["m"])), 1e-30)       # the restatement is the rule
        nrm = float(np.sqrt(np.sum(u.astype(np.float64) ** 2)))
        worst["norm"] = max(worst["norm"], abs(norms[i] - nrm) / (1e-6 * nrm))
        assert abs(norms[i] - nrm) <= 1e-6 * nrm and abs(nrm - ref["norm"]) <= 1e-6 * nrm, (i, norms[i], nrm)
        o64, tol = R.ns_tolerance(R.as_matrix(u), opt.muon_ns_steps, NS_FACTOR)
        o64 = o64.reshape(p.shape)
        err = float(np.max(np.abs(O_dev - o64)))
        worst["O"] = max(worst["O"], err / tol)
        assert err <= tol, (i, tuple(p.shape), "O", err, tol)
        rows, cols = R.as_matrix(u).shape
        assert abs(scales[i] - ref["s"]) <= 1e-7 * ref["s"] and abs(scales[i] - R.scale_of(rows, cols, scale)) <= 1e-7 * scales[i]
        w64 = p0[i].astype(np.float64) * (1.0 - lr * f32(rec.wd)) if decoupled else p0[i].astype(np.float64)
        w64 = w64 - lr * scales[i] * o64
        w_dev32 = p.detach().cpu().numpy()
        w_dev = w_dev32.astype(np.float64)
        tol_w = tol * lr * scales[i] + 2.0 * np.spacing(np.maximum(np.abs(p0[i]), np.abs(w64).astype(np.float32)))
        worst["w"] = max(worst["w"], float(np.max(np.abs(w_dev - w64) / tol_w)))
        assert (np.abs(w_dev - w64) <= tol_w).all(), (i, tuple(p.shape), "w")
        assert not np.array_equal(w_dev32, p0[i])                          # and the parameter did move
        if name == "composed":
            d = np.float32(sb["ema_decay"])
            e1 = _fma32(d, e0[i], (np.float32(1.0) - d) * w_dev32)
            assert np.array_equal(rec.view("e").cpu().numpy().view(np.int32), e1.view(np.int32)), (i, "shadow")
    assert seen == PATHS.count("large") == 5
    record_margins(f"step_large {name} {'decoupled' if decoupled else 'coupled'} {'nesterov' if nesterov else 'momentum'} {scale}", worst)


# ---- 3. nothing else moves -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("decoupled", [False, True], ids=["coupled", "decoupled"])
def test_every_parameter_that_is_not_large_keeps_the_bits_of_muon_alone(decoupled):
    """muon_large=True against muon=True on the same gradients: the small matrices, the Adam ranges, their moments, work buffers and
    shadows are bit-equal after every step, the state block too; the large ones take another step"""
    dev = torch.device("cuda:0")
    kw = dict(weight_decay=WD, decoupled_weight_decay=decoupled, max_grad_norm=MAX_NORM, skip_nonfinite=True, ema_decay=0.9, lr_schedule=lr_sched())
    a = make_params(dev)
    b = clone_params(a)
    _, oa = make_opt(a, **LARGE_KW, **kw)
    _, ob = make_opt(b, muon=True, **kw)
    assert oa._flags == ob._flags and ob.muon_large is False and "large" not in ob.muon_paths
    assert [x == "small" for x in oa.muon_paths] == ob.orthogonalized
    gs = grads(dev)
    for k in range(STEPS):
        step(oa, a, gs[k]); step(ob, b, gs[k])
        for i, (ra, rb) in enumerate(zip(oa._recs, ob._recs)):
            assert ra.p.shape == rb.p.shape
            if oa.muon_paths[i] == "large":
                assert not ra.view("v").any() and not torch.equal(ra.view("p"), rb.view("p"))
                continue
            for key in "pmve" + ("o" if oa.muon_paths[i] == "small" else ""):
                assert torch.equal(bits(ra.view(key)), bits(rb.view(key))), (k, i, key)
        assert torch.equal(oa._muon_report, ob._muon_report), k
        assert_state_blocks_equal(oa, ob, k)
    assert int(oa.applied_steps.item()) == STEPS


def test_without_a_large_matrix_the_step_is_muon_alone():
    """a model whose matrices all fit the small rule: muon_large=True selects nothing more, calls avmoe_opt_muon_step and leaves the bits
    of muon=True everywhere"""
    dev = torch.device("cuda:0")
    shapes = tuple(s for s, path in zip(SHAPES, PATHS) if path != "large") + ((128, 130),)
    kw = dict(weight_decay=WD, max_grad_norm=MAX_NORM, skip_nonfinite=True, ema_decay=0.9, lr=LR)
    from avmoe_amd.dp import AdapterGradReducer
    from avmoe_amd.train import FlatAdam
    a = make_params(dev, shapes=shapes)
    b = clone_params(a)
    oa = FlatAdam(AdapterGradReducer(a, bucket_mb=BUCKET_MB), **LARGE_KW, **kw)
    ob = FlatAdam(AdapterGradReducer(b, bucket_mb=BUCKET_MB), muon=True, **kw)
    assert oa.muon_paths == [None if x is False else "small" for x in ob.orthogonalized] and oa._muon_large_order == []
    assert not hasattr(oa, "_muon_large_image")               # nothing of the large path is built: _update calls avmoe_opt_muon_step
    gs = grads(dev, shapes=shapes)
    for k in range(STEPS):
        step(oa, a, gs[k]); step(ob, b, gs[k])
        assert_flats_equal(flats(oa, "pmveo"), flats(ob, "pmveo"), k, "pmveo")
        assert same(muon_out(oa), muon_out(ob))
    assert_state_blocks_equal(oa, ob)


# ---- 4. skipping, SAM ------------------------------------------------------------------------------------------------
def test_a_skipped_step_leaves_every_bit():
    dev = torch.device("cuda:0")
    a = make_params(dev)
    _, opt = make_opt(a, weight_decay=WD, max_grad_norm=MAX_NORM, skip_nonfinite=True, ema_decay=0.9, **LARGE_KW)
    gs = grads(dev)
    step(opt, a, gs[0])
    before, out = flats(opt, "pmveo"), muon_out(opt)
    assert len(out) == len(opt.state) + 2
    set_grads(a, gs[1])
    poison(a[1])
    opt.step()
    assert_flats_equal(before, flats(opt, "pmveo"), "skipped step", "pmveo")
    assert same(out, muon_out(opt))
    assert int(opt.skipped_steps.item()) == 1 and int(opt.applied_steps.item()) == 1 and int(opt.state_block["skip"].item()) == 1
    step(opt, a, gs[2])                                       # and the run goes on
    assert int(opt.applied_steps.item()) == 2 and not same(out, muon_out(opt))
    assert not torch.equal(out[-1], muon_out(opt)[-1])        # the large report moved


@pytest.mark.parametrize("decoupled", [False, True], ids=["coupled", "decoupled"])
def test_the_step_behind_a_perturbation_is_the_step_without_it(decoupled):
    """A: g1, sam_perturb(), g2, step().  B, without SAM: g2, step().  Everything is bit-equal after every step; a skipped step of A
    restores the held weights and nothing else"""
    dev = torch.device("cuda:0")
    kw = dict(weight_decay=WD, decoupled_weight_decay=decoupled, max_grad_norm=MAX_NORM, skip_nonfinite=True, ema_decay=0.9, **LARGE_KW)
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
        if k == 1:
            poison(a[1]); poison(b[1])
        oa.step(); ob.step()
        assert not oa.perturbed
        assert_flats_equal(flats(oa, "pmveo"), flats(ob, "pmveo"), k, "pmveo")
        assert same(muon_out(oa), muon_out(ob)), k
        if k == 1:
            assert_flats_equal(before, flats(oa, "pmveo"), "a skipped step restores", "pmveo")
    assert_state_blocks_equal(oa, ob)
    assert int(oa.applied_steps.item()) == STEPS - 1 and int(oa.skipped_steps.item()) == 1


# ---- 5. capture and repetition ---------------------------------------------------------------------------------------
def test_a_captured_step_replays_bit_equal_to_the_eager_run_and_runs_repeat():
    dev = torch.device("cuda:0")
    kw = dict(weight_decay=WD, decoupled_weight_decay=True, max_grad_norm=MAX_NORM, skip_nonfinite=True, ema_decay=0.9, lr_schedule=lr_sched(), **LARGE_KW)
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
        assert same(muon_out(oc), eager[k]), k
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
        assert same(muon_out(ob), eager[k]), k
    assert int(ob.applied_steps.item()) == STEPS
    assert_flats_equal(flats(oa, "pmveo"), flats(ob, "pmveo"), "graph replay", "pmveo")
    assert_state_blocks_equal(oa, ob, "graph replay")
    assert not torch.equal(eager[0][-1], eager[-1][-1])       # the large norms did change from replay to replay


# ---- 6. resume -------------------------------------------------------------------------------------------------------
def test_resume_continues_bit_equal():
    dev = torch.device("cuda:0")
    kw = dict(weight_decay=WD, decoupled_weight_decay=True, max_grad_norm=MAX_NORM, ema_decay=0.9)
    a = make_params(dev)
    b = clone_params(a)
    _, oa = make_opt(a, muon_momentum=0.9, muon_ns_steps=4, muon_large_max_numel=1 << 20, **LARGE_KW, **kw)
    _, ob = make_opt(b, muon_momentum=0.9, muon_ns_steps=4, muon_large_max_numel=1 << 20, **LARGE_KW, **kw)
    gs = grads(dev)
    step(oa, a, gs[0]); step(ob, b, gs[0])
    sd = ob.state_dict()
    extra = sd["flat_adam"]
    assert extra["muon"] is True and extra["muon_large"] is True and extra["muon_large_max_numel"] == 1 << 20 and extra["muon_ns_steps"] == 4
    for i, path in enumerate(ob.muon_paths):
        if path == "large":
            assert not sd["state"][i]["exp_avg_sq"].any() and sd["state"][i]["exp_avg"].any()
    _, oc = make_opt(b, muon_large_max_numel=1 << 20, **LARGE_KW, **kw)      # a fresh reducer + optimizer: the saved constants win
    oc.load_state_dict(copy.deepcopy(sd))
    assert (oc.muon_momentum, oc.muon_ns_steps) == (f32(0.9), 4) and int(oc.applied_steps.item()) == 1
    for k in range(1, STEPS):
        step(oa, a, gs[k]); step(oc, b, gs[k])
        assert torch.equal(muon_out(oa)[-1], muon_out(oc)[-1]) and torch.equal(muon_out(oa)[-2], muon_out(oc)[-2]), k
    assert_flats_equal(flats(oa, "pmve"), flats(oc, "pmve"), "resumed run")
    assert_state_blocks_equal(oa, oc, "resumed run")
    _, od = make_opt(clone_params(b), muon=True, **kw)        # built without the option: the large matrices' exp_avg is no Adam moment
    with pytest.raises(ValueError, match="muon_large"):
        od.load_state_dict(copy.deepcopy(sd))
    bare = copy.deepcopy(sd)                                  # a dict without the keys loads as before
    for key in ("muon_large", "muon_large_max_numel"):
        del bare["flat_adam"][key]
    _, oe = make_opt(clone_params(b), **LARGE_KW, **kw)
    oe.load_state_dict(bare)
    assert oe.muon_large is True and int(oe.applied_steps.item()) == 1


# ---- 7. a real site --------------------------------------------------------------------------------------------------
def test_the_large_updates_of_a_real_site_are_nearly_orthogonal():
    """one step on the AVE variant at C = 256 with 144 x 160 tokens: conv_adapter (144 x 160 x 1 x 1) and fc (256 x 160) take the large
    path; their applied directions have singular values in the band tests/test_flat_adam_muon_gpu.py holds the small matrices to"""
    from avmoe_amd.dp import AdapterGradReducer
    from avmoe_amd.train import FlatAdam
    from tests.golden_util import load_golden
    from tests.test_adapters_api import _opt
    from tests.test_flat_adam_muon_api import VARIANTS
    dev = torch.device("cuda:0")
    _, cfg, _ = load_golden("ave_train")
    cls, kw = VARIANTS["ave"]
    m = cls(input_dim=256, output_dim=256, adapter_kind="bottleneck", dim_list=None, layer_idx=0, opt=_opt(cfg), conv_dim_in=160, conv_dim_out=144,
            linear_in=160, linear_out=256, **kw).to(dev)
    named = [(n, p) for n, p in m.named_parameters() if p.requires_grad]
    red = AdapterGradReducer([p for _, p in named])
    opt = FlatAdam(red, lr=1e-3, weight_decay=0.01, decoupled_weight_decay=True, max_grad_norm=1.0, **LARGE_KW)
    name_of = {id(p): n for n, p in named}
    large = sorted(name_of[id(p)] for p, path in zip(opt.params, opt.muon_paths) if path == "large")
    assert large == ["conv_adapter.weight", "fc.weight"] and "small" in opt.muon_paths and None in opt.muon_paths
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
            assert norms[i] == 0.0 and opt.muon_paths[i] is None
            continue
        mat = o.detach().cpu().double().reshape(p.shape[0], -1)
        sv = torch.linalg.svdvals(mat)
        assert torch.isfinite(mat).all() and float(sv.max()) <= 1.25, (name_of[id(p)], float(sv.max()))
        assert float(sv.max()) >= 0.3 and norms[i] > 0.0 and not torch.equal(p.detach(), before[i]), name_of[id(p)]


# ---- 8. guards -------------------------------------------------------------------------------------------------------
def test_a_launch_that_does_not_match_its_large_image_touches_nothing():
    """a large image whose header is not this launch's (wrong magic) leaves parameters, moments, averages, work buffers and both
    reports bit for bit -- the table walk included, which would otherwise give the large ranges Adam's step; a large matrix whose
    work entry cannot take 16-byte accesses is left out by every launch while the others take their step"""
    from avmoe_amd import _capi as capi
    from avmoe_amd import _capi_moe as cm
    dev = torch.device("cuda:0")
    a = make_params(dev)
    _, opt = make_opt(a, weight_decay=WD, max_grad_norm=MAX_NORM, ema_decay=0.9, **LARGE_KW)
    gs = grads(dev)
    step(opt, a, gs[0])
    before, out = flats(opt, "pmveo"), muon_out(opt)
    set_grads(a, gs[1])
    good = opt._muon_large_image
    opt._muon_large_image = good.clone()
    opt._muon_large_image[:4] = 0
    opt.step()                                                # finalize still counts the step; every update launch refuses
    torch.cuda.synchronize()
    opt._muon_large_image = good
    assert_flats_equal(before, flats(opt, "pmveo"), "stale large image", "pmveo")
    assert same(out, muon_out(opt))
    L, n = capi.lib(), len(opt.params)
    bent = opt._muon_work_ptrs.clone()
    victim = next(i for i, p in enumerate(opt.params) if tuple(p.shape) == (256, 160))
    bent[victim] += 4
    got = L.avmoe_opt_muon_step_large(opt._table_ptr, n, opt._n_blocks, opt._state_ptr, opt.betas[0], opt.betas[1], opt.eps, 1.0,
                                      cm.OPT_CLIP | cm.OPT_EMA, torch.cuda.current_stream().cuda_stream, opt._shadow_ptrs.data_ptr(), None,
                                      opt._muon_image.data_ptr(), len(opt._muon_order), bent.data_ptr(), C.byref(opt._muon_c),
                                      opt._muon_ws.data_ptr(), opt._muon_report.data_ptr(), good.data_ptr(), opt._muon_large_host.data_ptr(),
                                      len(opt._muon_large_order), opt._muon_large_ws.data_ptr(), opt._muon_large_report.data_ptr())
    assert got == 0, capi.lib().avmoe_last_error()
    torch.cuda.synchronize()
    rec = opt._recs[victim]
    for k, old in zip("pmveo", before[rec.bucket]):
        assert torch.equal(bits(old[rec.off:rec.off + rec.p.numel()]), bits(opt.state[rec.bucket][k][rec.off:rec.off + rec.p.numel()])), ("bent work entry", k)
    other = next(r for r in opt._recs if tuple(r.p.shape) == (160, 144))
    assert not torch.equal(before[other.bucket][0][other.off:other.off + other.p.numel()], other.view("p").reshape(-1))      # the others took their step
