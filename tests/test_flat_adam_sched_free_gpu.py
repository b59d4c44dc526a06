"""Schedule-free AdamW in FlatAdam on the device (avmoe_amd.train.FlatAdam(schedule_free=True, ...); include/avmoe.h: avmoe_opt_sf_step)
on the two-bucket model of the other optimizer tests, the smallest that reaches every path of the update kernel (a block serves 1024
elements, a thread four):
    1, 3, 4, 5, 1023, 1024, 1025 and 2049 elements -- the ranges of 1 and 3 elements are served by the scalar tail alone, 1025 and 2049
    end in a block of one element, 2049 has three blocks; two parameter groups with different rates.
The gradients are the closed-form integer formula of tests/test_flat_adam_flag_matrix_gpu.py (copied, not imported): multiples of 2^-8
in [-4, 4), the same on every machine.

The fp64 bounds and the rounding count they come from are tests/sched_free_ref.py's.  Everything that is the same kernels on the same
bits is held to bit-equality.  AVMOE_SF_MARGINS=<file> appends the worst observed fraction of each bound per option set to that file."""
import copy
import os

import numpy as np
import pytest
import torch

from tests import sched_free_ref as ref
from tests.test_flat_adam_ema_gpu import assert_flats_equal, bits, flats, padding_mask, set_grads

pytestmark = pytest.mark.gpu

SIZES = (1, 3, 4, 5, 1023, 1024, 1025, 2049)
SHAPES = {4: (2, 2), 1024: (32, 32)}
LR, LR_X, WD, WD_X, GRAD_SCALE, RHO = 3e-3, 1e-2, 1e-2, 3e-2, 0.5, 0.05
BUCKET_MB = 17200 / (1 << 20)                    # 4300 elements: 2049 + 1025 + 1024 (padded to 64s: 4224) fill the first bucket
STEPS = 6
MAX_NORM = 1.0                                   # the scaled gradients' norm is above 50 at every step: every step clips
POISONED, INF_PARAM = 3, 6                       # the step of the "clip_skip_adamw" and "sam" runs whose gradient carries an Inf, and where
BUF_SIZES = (1, 5, 1030)                         # the fake BatchNorm statistics of the "ema_buffers" run


def values(step):
    """one tensor per parameter: ((a k + b step) / 128 mod 2048 - 1024) / 256 over the running element index k, multiples of 2^-8 in [-4, 4)"""
    out, k0 = [], 0
    for n in SIZES:
        k = torch.arange(k0 + 1, k0 + n + 1, dtype=torch.int64)
        h = (k * 2654435761 + (step + 2) * 40503) // 128 % 2048 - 1024
        out.append((h.to(torch.float32) / 256.0).reshape(SHAPES.get(n, (n,))))
        k0 += n
    return out


def make_params(dev):
    return [torch.nn.Parameter((0.25 * v).to(dev)) for v in values(-1)]


def clone_params(params):
    return [torch.nn.Parameter(p.detach().clone()) for p in params]


def grads(dev, step, first=False):
    """the gradient of step `step` (first: the one sam_perturb() sees before it)"""
    return [g.to(dev) for g in values(step + 1 + (100 if first else 0))]


def warmup():
    from avmoe_amd.train import LRSchedule
    return LRSchedule(warmup_steps=3, warmup_start=0.0)


def make_opt(params, groups="lr", **kw):
    from avmoe_amd.dp import AdapterGradReducer
    from avmoe_amd.train import FlatAdam
    red = AdapterGradReducer(params, bucket_mb=BUCKET_MB)
    assert len(red.buckets) == 2 and sorted(p.numel() for b in red.buckets for p in b.params) == sorted(SIZES)
    kw.setdefault("lr", LR)
    kw.setdefault("weight_decay", WD)
    kw.setdefault("grad_scale", GRAD_SCALE)
    kw.setdefault("schedule_free", True)
    group = {"params": params[:4], "lr": LR_X}
    if groups == "lr_wd":
        group["weight_decay"] = WD_X
    return red, FlatAdam(red, param_groups=[group], **kw)


OPTION_SETS = {
    "plain": dict(),
    "clip_skip_adamw": dict(max_grad_norm=MAX_NORM, skip_nonfinite=True, decoupled_weight_decay=True),
    "coupled_groups": dict(groups="lr_wd", max_grad_norm=MAX_NORM, report_grad_norms=True),
    "schedule": dict(lr_schedule="warmup", decoupled_weight_decay=True),
    "b1_zero": dict(betas=(0.0, 0.999), max_grad_norm=MAX_NORM),
    "r1_p0": dict(sf_r=1.0, sf_lr_power=0.0, lr_schedule="warmup"),
    "ema_buffers": dict(ema_buffers="fake", decoupled_weight_decay=True),
    "sam": dict(sam_rho=RHO, skip_nonfinite=True, max_grad_norm=MAX_NORM),
}


def settings(name, dev):
    kw, bufs = dict(OPTION_SETS[name]), None
    if kw.get("lr_schedule") == "warmup":
        kw["lr_schedule"] = warmup()
    if kw.get("ema_buffers") == "fake":
        g = torch.Generator().manual_seed(4)
        bufs = [torch.randn(n, generator=g).to(dev) for n in BUF_SIZES]
        kw["ema_buffers"] = [(f"bn{i}.running_mean", t) for i, t in enumerate(bufs)]
    return kw, bufs


def block_of(opt):
    return {k: v.item() for k, v in opt.sf_block.items()}


def block_bits(opt):
    return opt._sf_block.clone()


def snapshot(opt):
    """every range's arrays as the device holds them now, in table order (y: the parameter), the block and the state block's decay word"""
    ranges = []
    for rec in opt._recs:
        s, n, off = opt.state[rec.bucket], rec.p.numel(), rec.off
        r = {k: s[src][off:off + n].cpu().numpy().copy() for k, src in (("y", "p"), ("g", "g"), ("z", "m"), ("v", "v"), ("x", "e"))}
        r["lr"], r["wd"] = rec.lr0 * opt.decay, rec.wd
        ranges.append(r)
    return {"ranges": ranges, "block": block_of(opt), "ema_decay": float(opt.last_ema_decay.item())}


def step(opt, params, dev, k, sam=False, bad=False):
    """step k; -> the operands as stored before it (behind a perturbation: the held weights, taken before it)"""
    held = None
    if sam:
        set_grads(params, grads(dev, k, first=True))
        held = snapshot(opt)
        opt.sam_perturb()
    set_grads(params, grads(dev, k))
    if bad:
        params[INF_PARAM].grad.view(-1)[params[INF_PARAM].numel() // 2] = float("inf")
    before = snapshot(opt)
    if held is not None:
        for r, h in zip(before["ranges"], held["ranges"]):
            r["y"] = h["y"]
    opt.step()
    return before


def consts_of(opt, after, name):
    sb = {k: v.item() for k, v in opt.state_block.items()}
    K = ref.consts(b1=opt.betas[0], b2=opt.betas[1], eps=opt.eps, bc2_sqrt=sb["bc2_sqrt"], d=after["block"]["d"],
                   gscale=ref.f32(np.float32(opt.grad_scale) * np.float32(sb["clip_coef"])),
                   lr_factor=sb["lr_factor"] if opt.lr_schedule is not None else 1.0, decoupled=opt.decoupled_weight_decay, skip=bool(sb["skip"]))
    return K, int(sb["applied_steps"]), (ref.f32(sb["lr_factor"]) if opt.lr_schedule is not None else 1.0)


def record(line):
    print(line)
    path = os.environ.get("AVMOE_SF_MARGINS")
    if path:
        with open(path, "a") as fh:
            fh.write(line + "\n")


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(OPTION_SETS))
def test_every_step_against_fp64_from_the_operands_stored_before_it(name):
    """tests/sched_free_ref.py's check_step after each of the six steps: every element of v, z, x and y and the block's weight_sum, c and
    d (no element is left out, and the checker refused no step); x == z after the first applied step and, with b1 = 0, y == z after
    every step, bit for bit; the buffers' shadows within the average's own three roundings; alignment padding keeps its bits"""
    dev = torch.device("cuda:0")
    a = make_params(dev)
    kw, bufs = settings(name, dev)
    red, opt = make_opt(a, **kw)
    assert opt.schedule_free is True and len(opt.params) == len(SIZES) and opt._n_blocks == 11
    assert all(torch.equal(z, p.data) and torch.equal(x, p.data) for z, x, p in zip(opt.sf_z, opt.ema_params, opt.params))
    assert not opt._sf_block.any() and opt.sf_c.is_cuda and opt.sf_c.dtype == torch.float32 and opt.sf_weight_sum.dtype == torch.float64
    pads = [padding_mask(b, dev) for b in red.buckets]
    keys = [k for k in ("p", "m", "v", "e", "h") if k in opt.state[0]]
    pad_before = [[s[k][pad].clone() for k in keys] for s, pad in zip(opt.state, pads)]
    worst, refused, skipped, host_blk = {}, 0, 0, {"weight_sum": 0.0, "f_max": 0.0, "c": 0.0, "d": 0.0}
    for k in range(STEPS):
        bad = k == POISONED and name in ("clip_skip_adamw", "sam")
        if bufs is not None:                                  # what the forward passes before this step have left
            for i, t in enumerate(bufs):
                t.add_(0.01 * (k + 1) * (i + 1))
            shadows_before = [e.double().cpu().numpy() for e in opt.ema_buffers]
        before = step(opt, a, dev, k, sam=name == "sam", bad=bad)
        torch.cuda.synchronize()
        after = snapshot(opt)
        K, n, f = consts_of(opt, after, name)
        assert K.skip == bad and not opt.perturbed
        skipped += int(bad)
        assert n == k + 1 - skipped
        try:
            used = ref.check_step(before, after, K, n, f, opt.sf_r, opt.sf_lr_power)
        except ref.Refused:
            refused += 1
            continue
        for key, val in used.items():
            worst[key] = max(worst.get(key, 0.0), val)
        if not K.skip:
            # the host's copy of the scalar rule, from its own words: the device's block within the reference's bounds of it
            ws, f_max, c, d = type(opt).sf_weights_next(host_blk["weight_sum"], host_blk["f_max"], n, f, opt.sf_r, opt.sf_lr_power)
            host_blk = {"weight_sum": ws, "f_max": f_max, "c": c, "d": d}
            got = after["block"]
            assert got["f_max"] == f_max and abs(got["weight_sum"] - ws) <= 2.0 ** -45 * ws and abs(got["c"] - c) <= 2 * ref.U * c \
                and abs(got["d"] - d) <= 2 * ref.U, (got, host_blk)
            assert float(opt.sf_c.item()) == got["c"] and float(opt.sf_lr_max.item()) == got["f_max"]
            assert float(opt.last_ema_decay.item()) == got["d"] and float(opt.sf_weight_sum.item()) == got["weight_sum"]
            if n == 1:                                        # c = 1 and d = 0 (from factor 0 with lr_power > 0: c = 0, d = 1, and z has not moved): x is z
                assert (got["c"], got["d"]) == ((0.0, 1.0) if name == "schedule" else (1.0, 0.0))
                assert_flats_equal(flats(opt, "m"), flats(opt, "e"), "x == z after the first applied step", "x")
            if name == "b1_zero":
                assert_flats_equal(flats(opt, "p"), flats(opt, "m"), ("y == z with b1 = 0", k), "y")
            if bufs is not None:
                for s0, e, t in zip(shadows_before, opt.ema_buffers, bufs):
                    b64, dd = t.double().cpu().numpy(), K.d
                    want = dd * s0 + (1.0 - dd) * b64
                    err = np.abs(e.double().cpu().numpy() - want)
                    assert (err <= 4 * ref.U * (np.abs(dd * s0) + (1.0 - dd) * np.abs(b64))).all(), ("a buffer's shadow", k)
    assert refused == 0                                       # the cap is fail-closed: these gradients never produce a near-subnormal moment
    for s, pad, old in zip(opt.state, pads, pad_before):
        assert int(pad.sum()) > 0
        for key, o in zip(keys, old):
            assert torch.equal(bits(s[key][pad]), bits(o)), ("alignment padding", key)
    assert int(opt.applied_steps.item()) == STEPS - skipped and int(opt.skipped_steps.item()) == skipped
    if opt.report_grad_norms:                                 # the report's launch rides behind finalize as it does without the option
        norms = opt.last_param_grad_norms.double()
        assert int(opt.first_nonfinite_param.item()) == -1 and abs(float(norms.pow(2).sum().sqrt()) / float(opt.last_grad_norm.item()) - 1.0) < 1e-6
    assert set(worst) == {"v", "z", "x", "y", "weight_sum", "c", "d"} and max(worst.values()) <= 1.0
    assert any(not torch.equal(x, p.data) for x, p in zip(opt.ema_params, opt.params)) or name == "b1_zero"      # x and y did part
    record(f"{name}: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


@pytest.mark.parametrize("sam", [False, True], ids=["plain", "sam"])
def test_a_skipped_step_changes_no_byte(sam):
    """one Inf with skip_nonfinite: every bucket buffer, the 32-byte block and the state block's decay word keep their bytes; behind a
    perturbation the held weights come back bit for bit"""
    dev = torch.device("cuda:0")
    a = make_params(dev)
    bufs = [torch.randn(n).to(dev) for n in BUF_SIZES]
    _, opt = make_opt(a, max_grad_norm=MAX_NORM, skip_nonfinite=True, lr_schedule=warmup(),
                      ema_buffers=[(f"b{i}", t) for i, t in enumerate(bufs)], **(dict(sam_rho=RHO) if sam else {}))
    for k in range(3):
        step(opt, a, dev, k, sam=sam)
    before, blk, word = flats(opt, "pmve"), block_bits(opt), bits(opt.last_ema_decay)
    shadows = [bits(e) for e in opt.ema_buffers]
    assert float(opt.sf_weight_sum.item()) > 0.0 and int(word.item()) != 0
    step(opt, a, dev, 3, sam=sam, bad=True)
    assert_flats_equal(before, flats(opt, "pmve"), "skipped step", "pmve")      # under SAM: the held weights came back
    assert torch.equal(blk, block_bits(opt)) and torch.equal(word, bits(opt.last_ema_decay)) and not opt.perturbed
    assert all(torch.equal(s, bits(e)) for s, e in zip(shadows, opt.ema_buffers))
    assert int(opt.skipped_steps.item()) == 1 and int(opt.applied_steps.item()) == 3 and int(opt.state_block["skip"].item()) == 1
    step(opt, a, dev, 4, sam=sam)                             # and the run goes on
    assert int(opt.applied_steps.item()) == 4 and not torch.equal(blk, block_bits(opt))


def test_two_identical_runs_agree_bit_for_bit():
    dev = torch.device("cuda:0")
    kw = dict(max_grad_norm=MAX_NORM, decoupled_weight_decay=True, lr_schedule=warmup())
    a = make_params(dev)
    b = clone_params(a)
    _, oa = make_opt(a, **kw)
    _, ob = make_opt(b, **kw)
    for k in range(STEPS):
        step(oa, a, dev, k); step(ob, b, dev, k)
        assert torch.equal(block_bits(oa), block_bits(ob)), k
    assert_flats_equal(flats(oa, "pmve"), flats(ob, "pmve"), "second run", "pmve")
    assert float(oa.sf_c.item()) < 0.5


def test_a_captured_step_replays_bit_equal_to_the_eager_run():
    dev = torch.device("cuda:0")
    kw = dict(max_grad_norm=MAX_NORM, skip_nonfinite=True, decoupled_weight_decay=True, lr_schedule=warmup())
    a = make_params(dev)
    b = clone_params(a)
    _, oa = make_opt(a, **kw)
    _, ob = make_opt(b, **kw)
    start = flats(ob, "pmve")
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    eager = []
    with torch.cuda.stream(st):                              # the eager run (it also loads the kernels before the capture)
        for k in range(3):
            step(oa, a, dev, k)
            eager.append(block_bits(oa))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=st):
        ob.step()
    torch.cuda.synchronize()
    assert int(ob.applied_steps.item()) == 0 and not ob._sf_block.any()      # capturing runs nothing
    assert_flats_equal(start, flats(ob, "pmve"), "capture", "pmve")
    for k in range(3):
        set_grads(b, grads(dev, k))
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(block_bits(ob), eager[k]), k
    assert int(ob.applied_steps.item()) == 3
    assert_flats_equal(flats(oa, "pmve"), flats(ob, "pmve"), "graph replay", "pmve")
    assert len({tuple(e.tolist()) for e in eager}) == 3       # the block changed from replay to replay


def test_resume_continues_bit_equal_and_the_load_rules_hold():
    dev = torch.device("cuda:0")
    kw = dict(max_grad_norm=MAX_NORM, decoupled_weight_decay=True, lr_schedule=warmup())
    a = make_params(dev)
    b = clone_params(a)
    _, oa = make_opt(a, **kw)
    _, ob = make_opt(b, **kw)
    for k in range(3):
        step(oa, a, dev, k); step(ob, b, dev, k)
    sd = ob.state_dict()
    extra = sd["flat_adam"]
    assert extra["schedule_free"] is True and (extra["sf_r"], extra["sf_lr_power"]) == (0.0, 2.0) and extra["sf_c"] == float(ob.sf_c.item())
    assert extra["sf_weight_sum"] == float(ob.sf_weight_sum.item()) > 0.0 and extra["sf_lr_max"] == float(ob.sf_lr_max.item())
    assert len(extra["ema"]) == len(SIZES) and all(torch.equal(e, x.cpu()) for e, x in zip(extra["ema"], ob.ema_params))
    assert all(torch.equal(sd["state"][i]["exp_avg"], z.cpu()) for i, z in enumerate(ob.sf_z))      # torch's format: exp_avg is z
    c = clone_params(b)                                      # the model as saved (y); the optimizer built with OTHER constants: the saved ones win
    _, oc = make_opt(c, **dict(kw, sf_r=1.0, sf_lr_power=0.0))
    assert not torch.equal(oc.sf_z[7], ob.sf_z[7])           # built from the trained weights: z is y there, not the run's
    oc.load_state_dict(copy.deepcopy(sd))
    assert (oc.sf_r, oc.sf_lr_power) == (0.0, 2.0) and torch.equal(block_bits(oc), block_bits(ob))
    assert torch.equal(bits(oc.last_ema_decay), bits(ob.last_ema_decay))
    for k in range(3, STEPS):
        step(oa, a, dev, k); step(oc, c, dev, k)
        assert torch.equal(block_bits(oa), block_bits(oc)), k
    assert_flats_equal(flats(oa, "pmve"), flats(oc, "pmve"), "resumed run", "pmve")
    # a dict without the option keeps exp_avg_sq and the counters, re-seeds z = x = the current parameters and zeroes the block
    plain_params = clone_params(b)
    _, oplain = make_opt(plain_params, schedule_free=False, **kw)
    for k in range(2):
        set_grads(plain_params, grads(dev, k))
        oplain.step()
    d = clone_params(plain_params)
    _, od = make_opt(d, **kw)
    od._sf_block.fill_(7)
    od.state[0]["m"].fill_(1.0); od.state[0]["e"].fill_(2.0)
    od.load_state_dict(oplain.state_dict())
    assert not od._sf_block.any() and int(od.applied_steps.item()) == 2 and int(bits(od.last_ema_decay).item()) == 0
    assert all(torch.equal(z, p.data) and torch.equal(x, p.data) for z, x, p in zip(od.sf_z, od.ema_params, od.params))
    assert_flats_equal(flats(od, "v"), flats(oplain, "v"), "exp_avg_sq is kept", "v")
    step(od, d, dev, 2)
    assert float(od.sf_c.item()) == 1.0 and int(od.applied_steps.item()) == 3      # the average starts again from the first step after the load
    # and a dict saved with the option does not load into an optimizer built without it
    with pytest.raises(ValueError, match="schedule_free"):
        oplain.load_state_dict(copy.deepcopy(sd))


def test_the_average_is_served_by_the_averaging_machinery_unchanged():
    """swap_ema() twice restores every byte; inside ema_weights() the parameters are x; adapter_state_dict(model, ema=opt) returns x"""
    from avmoe_amd.train import adapter_state_dict
    dev = torch.device("cuda:0")
    a = make_params(dev)
    model = torch.nn.Module()
    model.adapter = torch.nn.ParameterList(a)
    _, opt = make_opt(a, max_grad_norm=MAX_NORM)
    for k in range(3):
        step(opt, a, dev, k)
    before = flats(opt, "pmve")
    xs, ys = [x.clone() for x in opt.ema_params], [p.detach().clone() for p in opt.params]
    assert any(not torch.equal(x, y) for x, y in zip(xs, ys))
    where = {id(p): i for i, p in enumerate(opt.params)}      # the optimizer holds the parameters in the reducer's order, the model in its own
    mine = [xs[where[id(p)]].cpu() for p in a]
    sd = adapter_state_dict(model, ema=opt)
    assert len(sd) == len(SIZES) and all(torch.equal(sd[f"adapter.{i}"], x) for i, x in enumerate(mine))
    with opt.ema_weights():
        assert all(torch.equal(bits(p.data), bits(x)) for p, x in zip(opt.params, xs))
        assert all(torch.equal(bits(e), bits(y)) for e, y in zip(opt.ema_params, ys))
        with pytest.raises(RuntimeError):
            opt.step()
        inside = adapter_state_dict(model, ema=opt)
        assert all(torch.equal(inside[f"adapter.{i}"], x) for i, x in enumerate(mine))
    assert_flats_equal(before, flats(opt, "pmve"), "ema_weights()", "pmve")
    opt.swap_ema(); opt.swap_ema()
    assert_flats_equal(before, flats(opt, "pmve"), "swap_ema() twice", "pmve")
    assert float(opt.last_ema_decay.item()) == float(opt.sf_block["d"].item()) == ref.f32(2.0 / 3.0)


def test_a_launch_that_does_not_match_its_table_writes_nothing():
    """the entry point called directly with n_ranges one off: the defined refusal -- both kernels compare the count with the table's
    header before they dereference anything"""
    from avmoe_amd import _capi as capi
    from avmoe_amd import _capi_moe as cm
    dev = torch.device("cuda:0")
    a = make_params(dev)
    _, opt = make_opt(a, max_grad_norm=MAX_NORM, sam_rho=RHO)
    for k in range(2):
        step(opt, a, dev, k)
    set_grads(a, grads(dev, 2))
    before, blk, word = flats(opt, "pmve"), block_bits(opt), bits(opt.last_ema_decay)
    held = [s["h"].clone() for s in opt.state]
    L, n = capi.lib(), len(opt.params)
    stream = torch.cuda.current_stream().cuda_stream
    for off in (-1, 1):
        for hold in (None, opt._hold_ptrs.data_ptr()):
            capi.check(L.avmoe_opt_sf_step(opt._table_ptr, n + off, opt._n_blocks, opt._state_ptr, opt.betas[0], opt.betas[1], opt.eps, GRAD_SCALE,
                                           cm.OPT_CLIP, stream, opt._shadow_ptrs.data_ptr(), hold, cm.C.byref(opt._sf_c),
                                           opt._sf_block.data_ptr()), "avmoe_opt_sf_step")
    torch.cuda.synchronize()
    assert_flats_equal(before, flats(opt, "pmve"), "a launch for another range count", "pmve")
    assert torch.equal(blk, block_bits(opt)) and torch.equal(word, bits(opt.last_ema_decay))
    assert all(torch.equal(bits(h), bits(s["h"])) for h, s in zip(held, opt.state))
    step(opt, a, dev, 2)                                      # the matching launch does step
    assert not torch.equal(blk, block_bits(opt)) and int(opt.applied_steps.item()) == 3
