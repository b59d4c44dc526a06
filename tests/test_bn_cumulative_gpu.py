"""Cumulative BatchNorm statistics on the device: avmoe_moe_desc.bn_momentum < 0 = torch's momentum=None (include/avmoe.h).  In a
training-mode forward every running statistic becomes (1 - f) r + f x with f = 1 / (n + 1), n the BatchNorm's own counter before the
call; the statistic kernels only read the counters and one launch behind them bumps them (csrc/fwd_kernels.hip: k_bn_count), so f
cannot depend on which thread got to a counter first.

Shapes, the smallest that reach each property:
    A  Cx=128 Nx=150 Cy=64 Ny=50 r=2 g=2 K=32, one cross-modal + one unimodal expert, 4 frames: the tuned register-resident shape
    B  A with two experts of each kind: per-expert counters
    C  Cx=128 Nx=77 Cy=96 Ny=50 r=4 g=2 K=8, 7 frames: the generalised / any-shape families
    D  A in bf16 with Nx=600 (2400 tokens: the streaming forms are eligible)

Tolerance of T cumulative steps against the fp64 mean of the batch statistics x_t (which the kernels themselves computed: T forwards
with momentum 1.0, each from a reset -- (1 - 1) r + 1 x is x exactly).  With u = 2^-24 (half an fp32 ulp, relative) and A the largest
|x_t| of the buffer, a step r' = (1 - f) r + f x makes at most 4 roundings of relative size u on magnitudes <= A (f itself, 1 - f, the
two products) and one on the sum: 5 u A, taken as 6.  The step is a convex combination (0 < f <= 1), so an error already in r is
multiplied by 1 - f < 1 and the per-step errors add without growing: |r - mean_t x_t| <= 6 T u A.  (The bound
tests/test_flat_adam_ema_gpu.py derives for the same expression shape.)  From a counter that starts at n0 > 0 the reset value r0 keeps
a weight, so there A also covers |r0| and the reference is the fp64 recurrence with f = 1 / (n0 + t).

Everything that is the same kernels on the same bits is held to bit-equality."""
import ctypes as C
import dataclasses

import pytest
import torch

from avmoe_amd import _capi as capi
from avmoe_amd import _capi_moe as cm
from oracle import avmoe_oracle as O

pytestmark = pytest.mark.gpu

T = 5
U = 2.0 ** -24
_A = dict(Cx=128, Nx=150, Cy=64, Ny=50, reduction=2, groups=2, K=32)
SHAPES = {        # name -> (config, frames, bf16)
    "A": (O.AdapterConfig(E_m=1, E_s=1, **_A), 4, False),
    "B": (O.AdapterConfig(E_m=2, E_s=2, **_A), 4, False),
    "C": (O.AdapterConfig(Cx=128, Nx=77, Cy=96, Ny=50, reduction=4, groups=2, K=8), 7, False),
    "D": (O.AdapterConfig(E_m=1, E_s=1, **{**_A, "Nx": 600}), 4, True),
}
_CACHE = {}


class Site:
    """a MoeRun in training mode with the BatchNorm counters in its pointer set, T seeded inputs, and the reset of update_bn"""

    def __init__(self, shape, counters=True):
        from tests.moe_gpu_util import MoeRun
        self.cfg, self.S, self.bf16 = SHAPES[shape]
        cfg = self.cfg
        self.P, B = O.init_params(cfg, seed=1)
        g = torch.Generator().manual_seed(7)
        self.inputs = [(0.3 * torch.randn(self.S, cfg.Nx, cfg.Cx, generator=g), 0.3 * torch.randn(self.S, cfg.Ny, cfg.Cy, generator=g))
                       for _ in range(T)]
        self.run = MoeRun(cfg, self.P, B, *self.inputs[0], bf16=self.bf16, training=True)
        self.counters = {k: torch.zeros((), dtype=torch.int64, device=self.run.dev) for k, v in B.items() if not v.is_floating_point()}
        assert len(self.counters) == 2 * cfg.E
        if counters:
            self.run.ptrs = cm.make_ptrs({**self.run.params, **self.run.buffers, **self.counters}, cfg.E_m, cfg.E_s)

    def reset(self, start=0):
        for k, v in self.run.buffers.items():
            v.fill_(1.0) if k.endswith("running_var") else v.zero_()
        for v in self.counters.values():
            v.fill_(start)

    def load(self, t):
        X, Y = self.inputs[t]
        self.run.X.copy_(X.to(self.run.dev, self.run.tdt))
        self.run.Y.copy_(Y.to(self.run.dev, self.run.tdt))

    def forward(self, t, momentum):
        self.load(t)
        self.run.desc.bn_momentum = momentum
        self.run.forward()

    def stats(self):
        return {k: v.clone() for k, v in self.run.buffers.items()}

    def counts(self):
        return {k: int(v) for k, v in self.counters.items()}

    def cumulative(self, start=0, steps=T):
        self.reset(start)
        for t in range(steps):
            self.forward(t, -1.0)
        return self.stats()


def site_of(shape):
    """the site of a shape with its batch statistics x_t (momentum 1.0, each from a reset) and one cumulative run: computed once"""
    if shape not in _CACHE:
        s = Site(shape)
        xs = []
        for t in range(T):
            s.reset()
            s.forward(t, 1.0)
            xs.append(s.stats())
        cum = s.cumulative()
        _CACHE[shape] = (s, xs, cum, s.counts())
    return _CACHE[shape]


def bits(t):
    return t.detach().clone().view(torch.int32)


@pytest.mark.parametrize("shape", list(SHAPES))
def test_first_cumulative_step_is_the_momentum_one_step_bit_for_bit(shape):
    s, xs, _cum, _n = site_of(shape)
    s.reset()
    s.forward(0, -1.0)
    got = s.stats()
    assert all(n == 1 for n in s.counts().values()), s.counts()
    for k, v in got.items():
        assert torch.isfinite(v).all(), k
        assert torch.equal(bits(v), bits(xs[0][k])), k
    assert any(float(v.abs().max()) > 0 for k, v in got.items() if k.endswith("running_mean"))      # the statistics were written at all


@pytest.mark.parametrize("shape", list(SHAPES))
def test_cumulative_steps_average_the_batch_statistics(shape):
    s, xs, cum, counts = site_of(shape)
    assert counts == {k: T for k in s.counters}, counts                     # every counter of every expert
    worst = 0.0
    for k, r in cum.items():
        mean = torch.stack([x[k].double() for x in xs]).mean(dim=0)
        A = max(float(x[k].abs().max()) for x in xs)
        err = float((r.double() - mean).abs().max())
        print(f"{shape} {k}: err {err:.3e}  bound {6 * T * U * A:.3e}")
        assert err <= 6 * T * U * A, (k, err, 6 * T * U * A)
        worst = max(worst, err)
    assert worst > 0.0                                                      # fp32 against fp64: not the same arithmetic


@pytest.mark.parametrize("shape", ["B", "C"])
def test_result_does_not_depend_on_who_reads_the_counter_first(shape):
    s, xs, cum, _n = site_of(shape)
    for _ in range(3):                                                      # repeated: the same bits
        again = s.cumulative()
        for k, v in again.items():
            assert torch.equal(bits(v), bits(cum[k])), k
    start = 41                                                              # f = 1/42 .. 1/46: a thread that saw n + 1 would use 1/43 .. 1/47
    got = s.cumulative(start)
    assert s.counts() == {k: start + T for k in s.counters}
    for k, r in got.items():
        r0 = 1.0 if k.endswith("running_var") else 0.0
        ref = torch.full_like(xs[0][k], r0, dtype=torch.float64)
        for t in range(T):
            f = 1.0 / (start + t + 1)
            ref = (1.0 - f) * ref + f * xs[t][k].double()
        A = max(r0, max(float(x[k].abs().max()) for x in xs))
        err = float((r.double() - ref).abs().max())
        print(f"{shape} {k} from {start}: err {err:.3e}  bound {6 * T * U * A:.3e}")
        assert err <= 6 * T * U * A, (k, err, 6 * T * U * A)


def test_cumulative_steps_match_the_oracle_step_by_step():
    s, _xs, _cum, _n = site_of("A")
    cfg = s.cfg
    s.reset()
    ref = {**{k: v.cpu().clone() for k, v in s.run.buffers.items()}, **{k: v.cpu().clone() for k, v in s.counters.items()}}
    for t in range(4):
        s.forward(t, -1.0)
        r = O.moe_forward(s.P, ref, *s.inputs[t], dataclasses.replace(cfg, bn_momentum=1.0 / (t + 1)), training=True)
        ref = r["new_buffers"]
        for k, v in s.run.buffers.items():
            assert torch.allclose(v.cpu(), ref[k], rtol=2e-4, atol=2e-5), (t, k)
        assert s.counts() == {k: int(ref[k]) for k in s.counters} and int(ref[next(iter(s.counters))]) == t + 1


def test_fixed_momentum_is_undisturbed_and_no_mode_writes_past_its_workspace():
    s, _xs, _cum, _n = site_of("A")
    s.reset()
    s.forward(0, 0.1)
    s.forward(1, 0.1)
    assert s.counts() == {k: 2 for k in s.counters}
    assert torch.isfinite(s.run.out).all() and all(torch.isfinite(v).all() for v in s.run.buffers.values())
    for k, v in s.run.buffers.items():                                      # two steps of 0.1 from (0, 1): far from the batch statistics
        if k.endswith("running_var"):
            assert float(v.min()) > 0.8
    assert s.run.guards_intact()
    s.cumulative(steps=2)
    assert s.run.guards_intact() and torch.isfinite(s.run.out).all()


def test_cumulative_mode_without_counters_is_refused_before_anything_runs():
    s = Site("A", counters=False)
    run = s.run
    s.reset()
    before = s.stats()
    run.out.fill_(-77.0)
    run.desc.bn_momentum = -1.0
    torch.cuda.synchronize()

    def call():
        return run.L.avmoe_moe_forward(C.byref(run.desc), run.X.data_ptr(), run.Y.data_ptr(), C.byref(run.ptrs), None, run.out.data_ptr(),
                                       run.probs.data_ptr(), run.idx.data_ptr(), run.lb.data_ptr(), run.saved.data_ptr(), run.scratch.data_ptr(),
                                       torch.cuda.current_stream().cuda_stream)
    assert call() == -1
    assert b"bn1_nbt" in run.L.avmoe_last_error() and b"expert 0" in run.L.avmoe_last_error()
    some = dict(list(s.counters.items())[:1])                               # expert 0's bn1 counter alone: its bn2 counter is named
    assert next(iter(some)).endswith("multimodal_experts.0.bn1.num_batches_tracked")
    run.ptrs = cm.make_ptrs({**run.params, **run.buffers, **some}, s.cfg.E_m, s.cfg.E_s)
    assert call() == -1 and b"bn2_nbt" in run.L.avmoe_last_error()
    torch.cuda.synchronize()
    assert bool((run.out == -77.0).all())
    assert all(torch.equal(v, before[k]) for k, v in s.stats().items()) and s.counts() == {k: 0 for k in s.counters}


def test_cumulative_training_forward_is_captured_and_replayed():
    s = Site("A")
    run = s.run
    run.desc.bn_momentum = -1.0
    eager = []
    s.reset()
    for t in range(3):
        s.forward(t, -1.0)
        eager.append(run.out.clone())
    eager_stats, eager_counts = s.stats(), s.counts()

    def call(stream):
        capi.check(run.L.avmoe_moe_forward(C.byref(run.desc), run.X.data_ptr(), run.Y.data_ptr(), C.byref(run.ptrs), None, run.out.data_ptr(),
                                           run.probs.data_ptr(), run.idx.data_ptr(), run.lb.data_ptr(), run.saved.data_ptr(),
                                           run.scratch.data_ptr(), stream), "forward")

    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        call(st.cuda_stream)                                                # warm-up on the capture stream
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=st):
        call(torch.cuda.current_stream().cuda_stream)
    s.reset()                                                               # the counters live on the device: the graph holds no factor
    for t in range(3):
        s.load(t)
        run.out.zero_()
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(bits(run.out), bits(eager[t])), t
    assert s.counts() == eager_counts == {k: 3 for k in s.counters}
    for k, v in s.stats().items():
        assert torch.equal(bits(v), bits(eager_stats[k])), k
