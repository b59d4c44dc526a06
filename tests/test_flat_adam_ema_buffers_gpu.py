"""FlatAdam's averaged buffers on the device (avmoe_amd.train.FlatAdam(ema_buffers=...); include/avmoe.h: avmoe_opt_buffer_table_*,
avmoe_opt_ema_buffers, avmoe_opt_swap_buffers) on the two-bucket toy reducer of tests/test_flat_adam_ema_gpu.py plus fake buffers whose
lengths are the tail and block-boundary cases of the kernels (a block serves 1024 elements of one buffer, a thread four of them, 256 apart):
1, 3, 4, 5, 63, 64, 65, 1023, 1024, 1025 and 2049 elements.  The one of 1025 elements is a view that starts one element into a larger tensor, so
its address is 4-byte aligned and no more, and the elements either side of it are guards; an int64 counter rides in the list and must never
be touched.  The buffers are rewritten with fresh seeded values before each of T = 6 steps, as the forward passes of a training step do.

Tolerance of a shadow against an fp64 recurrence on the host (test_shadows_follow_the_fp64_recurrence): the kernel computes
    shadow' = fma(d, shadow, fl(fl(1 - d) * b))
which is the parameter average's expression (one helper in csrc/adam_elem.h) with the buffer b in the parameter's place, and with the same
fp32 d as the reference (FlatAdam.ema_decay_at).  The bound is therefore the one tests/test_flat_adam_ema_gpu.py derives for the parameter
average, with A = max|b| over every value the buffers ever held: at most 5 u A per step (u = 2^-24), taken as 6, errors not growing under
a convex combination: |shadow - ref| <= 6 T u A after T steps.

Everything that is the same kernels on the same bits is held to bit-equality."""
import copy

import pytest
import torch

from tests.test_flat_adam_ema_gpu import (DECAY, LR, MAX_NORM, WD, OneSite, assert_flats_equal, bits, clone_params, decay_at, flats, grads,
                                          make_opt, make_params, sched, set_grads)

pytestmark = pytest.mark.gpu

BUF_SIZES = (1, 3, 4, 5, 63, 64, 65, 1023, 1024, 1025, 2049)
BUF_SHAPES = {4: (2, 2), 1024: (4, 256)}         # two of them not one-dimensional: the views must take the buffer's shape
UNALIGNED = 1025                                 # this one is a view one element into a larger tensor
T = 6
_VALUES = {}


class Buffers:
    """the fake buffers: `pairs` is what goes to FlatAdam(ema_buffers=...) -- the fp32 tensors, the int64 counter between them, and one of
    them a second time under another name (held once: de-duplicated by address)"""

    def __init__(self, dev, seed=0):
        self.big = torch.full((UNALIGNED + 2,), 7.25, device=dev)
        self.tensors = []
        for n in BUF_SIZES:
            self.tensors.append(self.big[1:1 + n] if n == UNALIGNED else torch.empty(BUF_SHAPES.get(n, (n,)), device=dev))
        self.counter = torch.tensor(41, dtype=torch.int64, device=dev)
        self.names = [f"bn{n}.running_mean" for n in BUF_SIZES]
        self.pairs = list(zip(self.names, self.tensors))
        self.pairs.insert(3, ("bn3.num_batches_tracked", self.counter))
        self.pairs.append(("alias_of_bn5", self.tensors[3]))
        self.write(values(dev, seed)[0])
        assert self.tensors[BUF_SIZES.index(UNALIGNED)].data_ptr() % 16 == 4

    def write(self, vals):
        with torch.no_grad():
            for t, v in zip(self.tensors, vals):
                t.copy_(v.view_as(t))

    def guards(self):
        return bits(torch.stack([self.big[0], self.big[-1]]))

    def snapshot(self):
        return [bits(t) for t in self.tensors]


def values(dev, seed=0):
    """seeded buffer values, [T + 1][buffer]: drawn once per seed on the host and shared; entry 0 is what the buffers hold at construction,
    entry k what they hold before step k.  Means near 0.5 with spread 2, like running statistics that move."""
    if seed not in _VALUES:
        g = torch.Generator().manual_seed(100 + seed)
        _VALUES[seed] = [[0.5 + 2.0 * torch.randn(n, generator=g) for n in BUF_SIZES] for _ in range(T + 1)]
    return [[v.to(dev) for v in step] for step in _VALUES[seed]]


def shadow_bits(opt):
    return [bits(e) for e in opt.ema_buffers]


def assert_bits_equal(a, b, what=""):
    assert len(a) == len(b), what
    for i, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(x, y), (what, i, BUF_SIZES[i])


def step(opt, params, bufs, gs, vals, k):
    """step k + 1: the forward's fresh statistics, the backward's gradients, the optimizer"""
    bufs.write(vals[k + 1])
    set_grads(params, gs[k])
    opt.step()


def test_buffers_are_collected_once_by_address_and_counters_are_left_out():
    dev = torch.device("cuda:0")
    bufs = Buffers(dev)
    _, opt = make_opt(make_params(dev), ema_decay=DECAY, ema_buffers=bufs.pairs)
    assert opt.ema_buffer_names == bufs.names and len(opt.ema_buffers) == len(BUF_SIZES)
    ptrs = set()
    for e, t in zip(opt.ema_buffers, bufs.tensors):          # seeded from the buffers; one flat allocation, each shadow 16-byte aligned
        assert e.shape == t.shape and e.dtype == torch.float32 and e.device == t.device and torch.equal(bits(e), bits(t))
        assert e.data_ptr() % 16 == 0
        ptrs.add(e.data_ptr())
    assert len(ptrs) == len(BUF_SIZES)
    lo, hi = opt._ebuf_flat.data_ptr(), opt._ebuf_flat.data_ptr() + 4 * opt._ebuf_flat.numel()
    assert all(lo <= e.data_ptr() and e.data_ptr() + 4 * e.numel() <= hi for e in opt.ema_buffers)
    assert opt._ebuf_blocks == sum((n + 1023) // 1024 for n in BUF_SIZES)
    _, plain = make_opt(make_params(dev), ema_decay=DECAY)   # without the option: no names, and the views raise
    assert plain.ema_buffer_names == []
    with pytest.raises(Exception):
        plain.ema_buffers


@pytest.mark.parametrize("warmup", [1.0, 10.0])
def test_shadows_follow_the_fp64_recurrence(warmup):
    """the bound of the module docstring; warm-up 1 is the constant decay 0.9, warm-up 10 the ratio (1 + n) / (10 + n) for all six steps"""
    dev = torch.device("cuda:0")
    a, gs, vals, bufs = make_params(dev), grads(T, dev), values(dev), Buffers(dev)
    _, opt = make_opt(a, weight_decay=WD, max_grad_norm=MAX_NORM, ema_decay=DECAY, ema_warmup=warmup, ema_buffers=bufs.pairs)
    ref = [v.double().cpu() for v in vals[0]]
    A = max(float(v.abs().max()) for stepvals in vals for v in stepvals)
    seen = set()
    for k in range(T):
        step(opt, a, bufs, gs, vals, k)
        d = decay_at(k + 1, DECAY, warmup)
        seen.add(d)
        assert float(opt.last_ema_decay.item()) == d
        ref = [d * r + (1.0 - d) * v.double().cpu() for r, v in zip(ref, vals[k + 1])]
    assert len(seen) == (1 if warmup == 1.0 else T)
    bound = 6 * T * 2.0 ** -24 * A
    worst = 0.0
    for n, e, r in zip(BUF_SIZES, opt.ema_buffers, ref):
        err = float((e.double().cpu().reshape(-1) - r).abs().max())
        worst = max(worst, err)
        print(f"warm-up {warmup}: buffer of {n} elements, |shadow - ref| max {err:.3e}, bound {bound:.3e} (A = {A:.4f})")
        assert err <= bound, (n, err, bound)
    assert worst > 0.0                                       # fp32 against fp64: not the same arithmetic


def test_a_step_reads_the_buffers_and_writes_only_the_shadows():
    dev = torch.device("cuda:0")
    a, gs, vals, bufs = make_params(dev), grads(T, dev), values(dev), Buffers(dev)
    _, opt = make_opt(a, ema_decay=DECAY, ema_warmup=10.0, ema_buffers=bufs.pairs)
    guards = bufs.guards()
    ptrs = [t.data_ptr() for t in bufs.tensors]
    for k in range(2):
        bufs.write(vals[k + 1])
        set_grads(a, gs[k])
        before, shadows = bufs.snapshot(), shadow_bits(opt)
        opt.step()
        assert_bits_equal(before, bufs.snapshot(), "the buffers themselves")
        assert torch.equal(guards, bufs.guards()), "memory around the unaligned view"
        assert int(bufs.counter.item()) == 41
        assert all(not torch.equal(x, y) for x, y in zip(shadows, shadow_bits(opt)))      # and every shadow did move
    assert [t.data_ptr() for t in bufs.tensors] == ptrs


OPTION_SETS = {"plain": dict(),
               "clip_skip": dict(weight_decay=WD, max_grad_norm=MAX_NORM, skip_nonfinite=True),
               "adamw_schedule": dict(weight_decay=WD, decoupled_weight_decay=True, lr_schedule="cosine"),
               "report": dict(weight_decay=WD, report_grad_norms=True)}


@pytest.mark.parametrize("name", list(OPTION_SETS))
def test_the_buffer_average_changes_nothing_else(name):
    """parameters, moments, parameter averages (alignment padding included) and every word of the state block after T steps, against the
    same optimizer without ema_buffers"""
    dev = torch.device("cuda:0")
    kw = dict(OPTION_SETS[name])
    if kw.get("lr_schedule"):
        kw["lr_schedule"] = sched()
    a = make_params(dev)
    b = clone_params(a)
    gs, vals, bufs = grads(T, dev), values(dev), Buffers(dev)
    _, oa = make_opt(a, ema_decay=DECAY, ema_warmup=10.0, ema_buffers=bufs.pairs, **kw)
    _, ob = make_opt(b, ema_decay=DECAY, ema_warmup=10.0, **kw)
    assert oa._flags == ob._flags
    for k in range(T):
        step(oa, a, bufs, gs, vals, k)
        set_grads(b, gs[k]); ob.step()
    assert_flats_equal(flats(oa), flats(ob), name)
    sa, sb = oa.state_block, ob.state_block
    assert set(sa) == set(sb)
    raw_a = oa._ws[:64].clone().view(torch.int32)
    raw_b = ob._ws[:64].clone().view(torch.int32)
    assert torch.equal(raw_a, raw_b), (name, raw_a.tolist(), raw_b.tolist())      # every word of the 64-byte block
    assert int(oa.applied_steps.item()) == T
    if name == "report":
        assert torch.equal(bits(oa.last_param_grad_norms), bits(ob.last_param_grad_norms))
        assert int(oa.first_nonfinite_param.item()) == int(ob.first_nonfinite_param.item()) == -1
    assert all(not torch.equal(bits(e), bits(t)) for e, t in zip(oa.ema_buffers, bufs.tensors))     # the shadows trail the buffers


def test_skipped_step_leaves_the_shadows_alone():
    dev = torch.device("cuda:0")
    a, gs, vals, bufs = make_params(dev), grads(T, dev), values(dev), Buffers(dev)
    _, opt = make_opt(a, weight_decay=WD, max_grad_norm=MAX_NORM, skip_nonfinite=True, ema_decay=DECAY, ema_warmup=10.0, ema_buffers=bufs.pairs)
    for k in range(2):
        step(opt, a, bufs, gs, vals, k)
    before, fl = shadow_bits(opt), flats(opt)
    bufs.write(vals[3])
    set_grads(a, gs[2])
    a[6].grad.view(-1)[a[6].numel() // 2] = float("nan")
    opt.step()
    assert int(opt.skipped_steps.item()) == 1 and int(opt.applied_steps.item()) == 2 and int(opt.state_block["skip"].item()) == 1
    assert_bits_equal(before, shadow_bits(opt), "skipped step")
    assert_flats_equal(fl, flats(opt), "skipped step")
    set_grads(a, gs[2]); opt.step()                           # the next good step averages again
    assert int(opt.applied_steps.item()) == 3
    assert all(not torch.equal(x, y) for x, y in zip(before, shadow_bits(opt)))


def test_swap_exchanges_buffers_and_shadows_in_place_and_back():
    dev = torch.device("cuda:0")
    a, gs, vals, bufs = make_params(dev), grads(T, dev), values(dev), Buffers(dev)
    _, opt = make_opt(a, weight_decay=WD, ema_decay=DECAY, ema_warmup=10.0, ema_buffers=bufs.pairs)
    for k in range(3):
        step(opt, a, bufs, gs, vals, k)
    b0, s0, fl, guards = bufs.snapshot(), shadow_bits(opt), flats(opt), bufs.guards()
    ptrs = [t.data_ptr() for t in bufs.tensors]
    assert all(not torch.equal(x, y) for x, y in zip(b0, s0))
    opt.swap_ema()
    assert_bits_equal(bufs.snapshot(), s0, "buffers after one swap")
    assert_bits_equal(shadow_bits(opt), b0, "shadows after one swap")
    assert [t.data_ptr() for t in bufs.tensors] == ptrs       # exchanged in place
    assert torch.equal(guards, bufs.guards()) and int(bufs.counter.item()) == 41
    opt.swap_ema()
    assert_bits_equal(bufs.snapshot(), b0, "buffers after two swaps")
    assert_bits_equal(shadow_bits(opt), s0, "shadows after two swaps")
    assert_flats_equal(fl, flats(opt), "after two swaps")
    assert torch.equal(guards, bufs.guards()) and int(bufs.counter.item()) == 41
    with opt.ema_weights():                                  # the context swaps weights and buffers together
        assert_bits_equal(bufs.snapshot(), s0, "inside the context")
        for p, e in zip(opt.params, opt.ema_params):
            assert not torch.equal(p.data, e)
        with pytest.raises(RuntimeError, match="swapped"):
            opt.step()
    assert_bits_equal(bufs.snapshot(), b0, "after the context")
    assert_bits_equal(shadow_bits(opt), s0, "after the context")
    assert_flats_equal(fl, flats(opt), "after the context")


def test_captured_step_averages_the_buffers_on_replay():
    dev = torch.device("cuda:0")
    a = make_params(dev)
    b = clone_params(a)
    n_steps = 3
    gs, vals = grads(T, dev), values(dev)
    bufs_a, bufs_b = Buffers(dev), Buffers(dev)
    kw = dict(weight_decay=WD, max_grad_norm=MAX_NORM, skip_nonfinite=True, ema_decay=DECAY, ema_warmup=10.0)
    _, oa = make_opt(a, ema_buffers=bufs_a.pairs, **kw)
    _, ob = make_opt(b, ema_buffers=bufs_b.pairs, **kw)
    start = shadow_bits(ob)
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):                              # the eager run (it also loads the kernels before the capture)
        for k in range(n_steps):
            step(oa, a, bufs_a, gs, vals, k)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=st):
        ob.step()
    torch.cuda.synchronize()
    assert int(ob.applied_steps.item()) == 0                 # capturing runs nothing
    assert_bits_equal(start, shadow_bits(ob), "capture")
    seen = [start]
    for k in range(n_steps):
        bufs_b.write(vals[k + 1])
        set_grads(b, gs[k])
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        seen.append(shadow_bits(ob))
        assert not torch.equal(seen[-1][-1], seen[-2][-1]), k  # the shadows did move from replay to replay
    assert int(ob.applied_steps.item()) == n_steps
    assert_bits_equal(shadow_bits(oa), shadow_bits(ob), "graph replay")
    assert_flats_equal(flats(oa), flats(ob), "graph replay")
    assert_bits_equal(bufs_a.snapshot(), bufs_b.snapshot(), "the buffers")


def test_resume_restores_the_shadows_and_continues_bit_equal():
    dev = torch.device("cuda:0")
    a = make_params(dev)
    b = clone_params(a)
    gs, vals = grads(T, dev), values(dev)
    bufs_a, bufs_b = Buffers(dev), Buffers(dev)
    kw = dict(weight_decay=WD, max_grad_norm=MAX_NORM, skip_nonfinite=True, ema_decay=DECAY, ema_warmup=10.0)
    _, oa = make_opt(a, ema_buffers=bufs_a.pairs, **kw)
    for k in range(T):
        step(oa, a, bufs_a, gs, vals, k)
    _, ob = make_opt(b, ema_buffers=bufs_b.pairs, **kw)
    for k in range(3):
        step(ob, b, bufs_b, gs, vals, k)
    sd = ob.state_dict()
    extra = sd["flat_adam"]
    assert extra["ema_buffer_names"] == bufs_b.names and len(extra["ema_buffers"]) == len(BUF_SIZES)
    for e, view, t in zip(extra["ema_buffers"], ob.ema_buffers, bufs_b.tensors):
        assert e.device.type == "cpu" and e.shape == t.shape and torch.equal(e, view.cpu())
    # a fresh reducer + optimizer over the parameters and buffers as the interrupted run left them
    _, oc = make_opt(b, ema_buffers=bufs_b.pairs, **kw)
    assert_bits_equal(shadow_bits(oc), bufs_b.snapshot(), "seeded from the buffers until the dict arrives")
    oc.load_state_dict(sd)
    assert_bits_equal(shadow_bits(oc), shadow_bits(ob), "restored")
    for k in range(3, T):
        step(oc, b, bufs_b, gs, vals, k)
    assert_bits_equal(shadow_bits(oa), shadow_bits(oc), "resumed run")
    assert_flats_equal(flats(oa), flats(oc), "resumed run")
    # a dict without the buffer averages: they start again from the current buffers
    bare = copy.deepcopy(sd)
    for key in ("ema_buffers", "ema_buffer_names"):
        del bare["flat_adam"][key]
    with torch.no_grad():
        for e in oc.ema_buffers:
            e.add_(1.0)
    oc.load_state_dict(bare)
    assert_bits_equal(shadow_bits(oc), bufs_b.snapshot(), "re-seeded")
    assert int(oc.applied_steps.item()) == 3
    # a wrong shape, and a wrong count, name the buffer
    bad = copy.deepcopy(sd)
    bad["flat_adam"]["ema_buffers"][4] = torch.zeros(2, 3)
    with pytest.raises(ValueError, match="bn63.running_mean"):
        oc.load_state_dict(bad)
    bad = copy.deepcopy(sd)
    del bad["flat_adam"]["ema_buffers"][-1]
    with pytest.raises(ValueError, match="bn1.running_mean"):
        oc.load_state_dict(bad)
    # and an optimizer without the option ignores saved ones
    _, od = make_opt(clone_params(b), **kw)
    od.load_state_dict(sd)
    assert od.ema_buffer_names == [] and "ema_buffers" not in od.state_dict()["flat_adam"]


def test_evaluation_with_averaged_weights_runs_on_averaged_statistics():
    """one BatchNorm site (fp32, the smallest fixture shape of tests/test_adapters_gpu.py), three training steps with ema_buffers=model: the
    eval-mode forward inside ema_weights() is the eval-mode forward of a freshly built site loaded from the averaged checkpoint"""
    from avmoe_amd.dp import AdapterGradReducer
    from avmoe_amd.train import FlatAdam, adapter_state_dict, load_adapters
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = OneSite()
    with torch.no_grad():
        for k, p in model.named_parameters():
            if k.endswith(("gate", "gate_av")):
                p.fill_(0.4)
    model = model.to(dev).train()
    site = model.audio_adapter_blocks_p1[0]
    red = AdapterGradReducer(list(site.parameters()), sites=[site])
    opt = FlatAdam(red, lr=LR, weight_decay=WD, max_grad_norm=1.0, ema_decay=DECAY, ema_warmup=1.0, ema_buffers=model)
    stats = {k: v for k, v in model.named_buffers() if v.is_floating_point()}
    assert opt.ema_buffer_names == list(stats) and len(stats) > 0 and any(not v.is_floating_point() for _, v in model.named_buffers())
    g = torch.Generator().manual_seed(9)

    def batch():
        return torch.randn(4, 64, 50, 1, generator=g).to(dev), torch.randn(4, 48, 20, 1, generator=g).to(dev)

    for _ in range(3):
        X, Y = batch()
        G = torch.randn(4, 64, 50, 1, generator=g).to(dev)
        red.begin(sync=True)
        site(X, Y)[0].backward(G)
        red.finish()
        opt.step()
        red.zero_grad()
    model.eval()
    X, Y = batch()
    raw = {k: v.detach().clone() for k, v in model.state_dict().items()}
    ptrs = {k: v.data_ptr() for k, v in model.named_buffers()}
    with torch.no_grad():
        out_raw = site(X, Y)[0].clone()
        with opt.ema_weights():
            out_avg = site(X, Y)[0].clone()
            inside = {k: v.detach().clone() for k, v in stats.items()}
            sd_inside = adapter_state_dict(model, ema=opt)
    sd = adapter_state_dict(model, ema=opt)
    for k, v in model.state_dict().items():                  # after the block: weights and running statistics as before it, bit for bit
        assert torch.equal(v, raw[k]) and (v.dtype != torch.float32 or torch.equal(bits(v), bits(raw[k]))), k
    assert {k: v.data_ptr() for k, v in model.named_buffers()} == ptrs               # no module._buffers entry was re-bound
    n_means = 0
    for k, e in zip(opt.ema_buffer_names, opt.ema_buffers):
        assert torch.equal(bits(inside[k]), bits(e)), k       # inside, the buffers held the averages
        assert torch.equal(sd[k], e.cpu()) and torch.equal(sd_inside[k], e.cpu()), k      # named_buffers() names are the checkpoint's keys
        if k.endswith("running_mean"):
            assert not torch.equal(e, stats[k]), k            # and the averages are not the raw statistics: a no-op would be noticed
            n_means += 1
    assert n_means > 0
    for k, v in sd.items():                                  # counters as they are
        if k.endswith("num_batches_tracked"):
            assert int(v) == 3 and torch.equal(v, raw[k].cpu()), k
    torch.manual_seed(1)
    other = OneSite()
    res = load_adapters(other, sd)
    assert not res.unexpected_keys and not [k for k in res.missing_keys if "adapter" in k]
    other = other.to(dev).eval()
    with torch.no_grad():
        out_other = other.audio_adapter_blocks_p1[0](X, Y)[0]
    assert torch.equal(bits(out_avg), bits(out_other))
    assert not torch.equal(out_avg, out_raw)                 # the averaged model is another model
