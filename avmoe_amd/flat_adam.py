"""The optimizer of the training loop, MI355X-side; `avmoe_amd.train` imports both names back:

  * `FlatAdam`              -- torch.optim.Adam semantics as ONE HIP kernel per flat gradient bucket of an
                               `AdapterGradReducer` (parameters are re-pointed to views of a flat buffer with the bucket's
                               layout), StepLR-style decay; replaces optimizer.step() at main_trans_v3.py:136-138,322-323.
                               Opt-in: global-norm clipping, AdamW, skipping of non-finite steps with the optimizer state on
                               the device (three launches per step for all buckets, graph-capturable); state_dict() /
                               load_state_dict() in torch.optim.Adam's format; an exponential moving average of the weights kept
                               by the update kernel itself, swapped in for evaluation and written by `save_adapters(ema=opt)`,
                               BatchNorm running statistics averaged and swapped with them (`ema_buffers=model`);
                               stochastic weight averaging (`swa_start` / `swa_freq`: torch's AveragedModel as that same average
                               with a uniform rule, SWALR as a part of `LRSchedule`), still without a launch more;
                               per-group weight decay; opt-in per-parameter gradient norms and the first non-finite parameter;
                               sharpness-aware minimization (`sam_rho`, `sam_adaptive`: `sam_perturb()` between the two backward
                               passes of a step, the unperturbed weights kept on the device and restored exactly by `step()`);
                               layer-wise trust ratios (`trust_ratio`), Prodigy learning-rate estimation (`prodigy`),
                               orthogonalised momentum (`muon`) and schedule-free AdamW (`schedule_free`: no run length in the
                               recipe, the evaluated average kept where the averages are)
  * `LRSchedule`            -- a per-step learning-rate schedule (linear warm-up, then cosine / linear / step decay) that FlatAdam's
                               device path evaluates on the device from its own step counter

Host logic around a few small C-ABI entry points (avmoe_adam_step, avmoe_opt_grad_norm_swa / avmoe_opt_adam_step[_ema|_sam] /
avmoe_opt_lamb_step / avmoe_opt_prodigy_step / avmoe_opt_muon_step / avmoe_opt_sf_step / avmoe_opt_swap_ema / avmoe_opt_sam_perturb,
avmoe_opt_ema_buffers / avmoe_opt_swap_buffers); nothing falls back to the CPU for GPU tensors.

A parameter is one `_ParamRecord` in `FlatAdam._recs` (its bucket, offset, rate, decay and per-option settings); a per-element side
buffer of an option (the averages "e", SAM's hold "h", Prodigy's "x0" and "s", Muon's work buffer "o") is one more flat tensor per
bucket with the bucket's layout, reached through `rec.view(key)` / `rec.ptr(key)`."""
from __future__ import annotations

import contextlib
import ctypes as C
import dataclasses
import math
import struct
from itertools import chain
from typing import Dict, List, Optional

import torch

from . import _capi as capi
from . import _capi_moe as cm

_SWA_FLAGS = cm.OPT_SWA | cm.OPT_SWA_LR                   # the flags that make the norm call read avmoe_opt_swa
_NORM_ONLY_FLAGS = cm.OPT_REPORT | _SWA_FLAGS             # the flags the update launch does not know
_AVERAGE_FLAGS = cm.OPT_EMA | cm.OPT_SWA                  # either makes the update launch advance the averages


# ---------------------------------------------------------------------------------------------------------------------
def _f32(x: float) -> float:
    return struct.unpack("f", struct.pack("f", x))[0]


@dataclasses.dataclass
class LRSchedule:
    """A per-step learning-rate schedule as a factor f(n) on every learning rate, n = the number of steps applied before this one (the
    first step has n = 0): avmoe_opt_schedule of include/avmoe.h.

        n <  warmup_steps:  f = warmup_start + (1 - warmup_start) * n / warmup_steps
        after, with u = n - warmup_steps, D = total_steps - warmup_steps, c = min(u, D):
            "cosine"  f = min_factor + (1 - min_factor) * (1 + cos(pi c / D)) / 2
            "linear"  f = 1 - (1 - min_factor) * c / D
            "step"    f = gamma ** (u // step_size)
            "none"    f = 1

    Cosine and linear stay at min_factor from total_steps on.  The device holds warmup_start, min_factor and gamma as fp32 and
    evaluates f in double from them; the constructor therefore rounds these three to fp32 (0.1 becomes 0.10000000149...), so that
    `factor(n)` is the very function the kernel computes and agrees with it to the final fp32 rounding.  A bad schedule raises
    ValueError here, with the rules the library checks again.

    The SWA learning rate (torch.optim.swa_utils.SWALR; avmoe_opt_swa of include/avmoe.h).  `swa_start=N` (None: off, and `factor` is
    the closed form above) anneals the factor from step N on to the constant `swa_factor` over `swa_anneal_steps` steps; with base(n)
    the closed form above:

        n <  N:  f = base(n)
        n >= N:  f0 = base(N), t = 1 if swa_anneal_steps == 0 else min(1, (n - N) / swa_anneal_steps),
                 alpha = t ("linear") or (1 - cos(pi t)) / 2 ("cos"), f = f0 + (swa_factor - f0) * alpha

    -- what SWALR(optimizer, swa_lr=swa_factor * lr0, anneal_epochs=swa_anneal_steps, anneal_strategy=swa_anneal) gives when it is
    constructed as step N is due, after a LambdaLR(base) stepped until then, and stepped once per applied step (its recursion in closed
    form).  `swa_factor` is held as fp32 like the other factors.  A schedule of the SWA part alone (no warm-up, decay_kind "none":
    base = 1) is valid."""
    warmup_steps: int = 0
    warmup_start: float = 0.0
    decay_kind: str = "none"
    total_steps: int = 0
    min_factor: float = 0.0
    step_size: int = 0
    gamma: float = 1.0
    swa_start: Optional[int] = None
    swa_factor: float = 1.0
    swa_anneal_steps: int = 0
    swa_anneal: str = "cos"

    def __post_init__(self):
        kinds = cm.SCHED_KINDS
        if isinstance(self.decay_kind, int) and not isinstance(self.decay_kind, bool) and self.decay_kind in kinds.values():
            self.decay_kind = {v: k for k, v in kinds.items()}[self.decay_kind]
        if self.decay_kind not in kinds:
            raise ValueError(f"decay_kind must be one of {sorted(kinds)}, not {self.decay_kind!r}")
        for name in ("warmup_steps", "total_steps", "step_size"):
            v = getattr(self, name)
            if isinstance(v, bool) or int(v) != v or v < 0:
                raise ValueError(f"{name} must be an integer >= 0, not {v!r}")
            setattr(self, name, int(v))
        for name in ("warmup_start", "min_factor"):
            v = float(getattr(self, name))
            if not (0.0 <= v <= 1.0):
                raise ValueError(f"{name} must be in [0, 1], not {v!r}")
            setattr(self, name, _f32(v))
        g = float(self.gamma)
        if not (0.0 < g <= 1.0) or _f32(g) == 0.0:
            raise ValueError(f"gamma must be in (0, 1], not {g!r}")
        self.gamma = _f32(g)
        if self.decay_kind in ("cosine", "linear") and self.total_steps <= self.warmup_steps:
            raise ValueError(f"a {self.decay_kind} decay needs total_steps > warmup_steps, not {self.total_steps} <= {self.warmup_steps}")
        if self.decay_kind == "step" and self.step_size <= 0:
            raise ValueError("a step decay needs step_size > 0")
        for name in ("swa_start", "swa_anneal_steps"):
            v = getattr(self, name)
            if v is None and name == "swa_start":
                continue
            if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or int(v) != v or v < 0:
                raise ValueError(f"{name} must be an integer >= 0, not {v!r}")
            setattr(self, name, int(v))
        if self.swa_anneal_steps > 2 ** 31 - 1:
            raise ValueError(f"swa_anneal_steps must fit 32 bits, not {self.swa_anneal_steps!r}")
        v = float(self.swa_factor)
        if not (0.0 <= v <= 1.0):
            raise ValueError(f"swa_factor must be in [0, 1], not {self.swa_factor!r}")
        self.swa_factor = _f32(v)
        if self.swa_anneal not in cm.SWA_ANNEAL_KINDS:
            raise ValueError(f"swa_anneal must be one of {sorted(cm.SWA_ANNEAL_KINDS)}, not {self.swa_anneal!r}")

    def factor(self, n: int) -> float:
        """f(n) in Python float (double), the closed form of the class docstring in the operation order of the kernel"""
        n, N = int(n), self.swa_start
        if N is None or n < N:
            return self._base(n)
        f0, t = self._base(N), 1.0
        if self.swa_anneal_steps > 0:
            t = min((n - N) / self.swa_anneal_steps, 1.0)
        alpha = t if self.swa_anneal == "linear" else (1.0 - math.cos(math.pi * t)) / 2.0
        return f0 + (self.swa_factor - f0) * alpha

    def _base(self, n: int) -> float:
        """the factor without the SWA part"""
        W = self.warmup_steps
        if n < W:
            return self.warmup_start + (1.0 - self.warmup_start) * n / W
        u = n - W
        if self.decay_kind == "none":
            return 1.0
        if self.decay_kind == "step":
            return self.gamma ** (u // self.step_size)
        D = self.total_steps - W
        c = min(u, D)
        if self.decay_kind == "cosine":
            return self.min_factor + (1.0 - self.min_factor) * 0.5 * (1.0 + math.cos(math.pi * c / D))
        return 1.0 - (1.0 - self.min_factor) * c / D

    def c_struct(self) -> "cm.OptSchedule":
        return cm.OptSchedule(warmup_steps=self.warmup_steps, warmup_start=self.warmup_start, decay_kind=cm.SCHED_KINDS[self.decay_kind],
                              total_steps=self.total_steps, min_factor=self.min_factor, gamma=self.gamma, step_size=self.step_size)

    def fill_swa(self, w: "cm.OptSwa") -> bool:
        """writes the learning-rate half of avmoe_opt_swa into `w`; -> whether the schedule has one (AVMOE_OPT_SWA_LR)"""
        if self.swa_start is None:
            return False
        w.lr_start, w.anneal_steps, w.lr_factor = self.swa_start, self.swa_anneal_steps, self.swa_factor
        w.anneal_kind = cm.SWA_ANNEAL_KINDS[self.swa_anneal]
        return True


# ---------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass(eq=False)
class _ParamRecord:
    """one parameter of a FlatAdam; `FlatAdam._recs` holds them in the reducer's order, the index order of `params` and state_dict()"""
    p: torch.nn.Parameter
    bucket: int                                          # index into FlatAdam.state
    off: int                                             # the parameter's offset in each flat buffer of that bucket, in elements
    lr0: float                                           # its group's base rate (before StepLR decay and schedule)
    wd: float                                            # its weight decay
    adapted: bool                                        # whether its step takes its trust ratio (trust_ratio)
    muon_shape: Optional[tuple]                          # (rows, cols) of an orthogonalised parameter, None for the others (muon)
    muon_path: Optional[str]                             # "small": the one-workgroup kernel, "large": the tiled engine (muon_large), or None
    state: list = dataclasses.field(repr=False)          # FlatAdam.state itself: what view() and ptr() look the buffers up in

    def view(self, key: str) -> torch.Tensor:
        """the parameter's part of its bucket's flat buffer `key` ("p", "g", "m", "v" or a side buffer), shaped like the parameter"""
        return self.state[self.bucket][key][self.off:self.off + self.p.numel()].view_as(self.p)

    def ptr(self, key: str) -> int:
        """the byte address of that part"""
        return self.state[self.bucket][key].data_ptr() + 4 * self.off


class FlatAdam:
    """Adam over the flat fp32 buckets of an AdapterGradReducer: per bucket ONE kernel updates parameters, exp_avg and
    exp_avg_sq in place (avmoe_adam_step).  Parameters of a bucket are moved into one flat buffer with the bucket's layout
    (`param.data` become views of it), so values, state_dict keys and autograd are unchanged.

        red = AdapterGradReducer(params, sites=sites)
        opt = FlatAdam(red, lr=args.lr, step_size=args.decay_epoch, gamma=args.decay)
        ...  red.begin(sync); loss.backward(); red.finish()
        if sync: opt.step(); red.zero_grad()
        opt.epoch_end()                      # StepLR.step()

    The device path.  With any of `max_grad_norm`, `decoupled_weight_decay`, `skip_nonfinite` set, a step is three launches for ALL buckets
    (include/avmoe.h, "optimizer with device-side state"): the squared-gradient sums of every parameter element in double, a one-block
    finalize that writes norm, clip factor, skip flag, step counters and bias corrections into a 64-byte state block on the device, and
    one Adam / AdamW update that reads them (without clipping and skipping: finalize + update).  No host synchronisation, no allocation
    and no step-dependent host scalar, so `step()` can be captured by torch.cuda.graph (one stream, linear) and replayed; the plain path
    bakes the bias correction of `self.t` into its kernel arguments and is not capturable in a meaningful way.  The clip factor is
    applied inside the update: the gradient buckets are NOT rescaled (torch.nn.utils.clip_grad_norm_ rescales `.grad` in place).  The
    norm covers the parameters the reducer holds, alignment padding excluded; parameters outside the reducer (a partly frozen site that
    falls back to autograd accumulation, anything not handed to AdapterGradReducer) are neither clipped nor counted.  Under data
    parallelism call `red.finish()` first: the norm is then that of the averaged gradient, identical on every rank.
    `last_grad_norm`, `applied_steps`, `skipped_steps` are DEVICE tensors (views of the state block): reading them is the caller's sync.

    A per-step schedule.  `lr_schedule=LRSchedule(...)` (it selects the device path too) multiplies every learning rate by f(applied_steps):
    the finalize launch evaluates f in double from the counter it already advances and leaves it in the state block (`last_lr_factor`),
    the update reads it.  Still three launches and no step-dependent host scalar, so a captured step follows the schedule on replay; a
    skipped step does not advance it.  It composes multiplicatively with the per-epoch StepLR (`step_size` / `gamma`, `epoch_end()`) and
    the per-group rates, which stay in the range table.

    Weight averaging.  `ema_decay=d` (it selects the device path too) keeps an exponential moving average of every parameter the reducer
    holds in one more flat buffer per bucket, seeded with the parameters at construction.  The finalize launch computes this step's decay
    d_n = min(d, (1 + n) / (ema_warmup + n)) from n = applied_steps after the step (`ema_decay_at`; `last_ema_decay` on the device), and
    the thread of the update launch that has just produced an element's new value p also writes ema = fma(d_n, ema, (1 - d_n) * p).
    Still three launches, capturable, and a skipped step leaves the average alone.  `ema_params` are views of the averages shaped like
    `params`; `swap_ema()` exchanges parameters and averages in one launch and `with opt.ema_weights():` does so around an evaluation;
    `adapter_state_dict(model, ema=opt)` / `save_adapters(..., ema=opt)` write the averaged values.  `state_dict()` carries the
    averages under "flat_adam" ("ema": CPU tensors in `params` order, "ema_decay", "ema_warmup"); `load_state_dict()` restores them, and
    a dict without them re-seeds the averages from the current parameters.  NOT averaged: parameters outside the reducer.

    Averaged buffers.  `ema_buffers=model` (or an iterable of (name, tensor); it needs `ema_decay`) averages the model's floating-point
    buffers -- the BatchNorm running means and variances, which an evaluation runs on -- along with the weights: timm's ModelEmaV2 on the
    device.  The buffers stay where they are (`module._buffers[...]` is never re-bound: the sites cache those addresses and their forward
    kernels write them in place); each has a shadow in one flat fp32 allocation, seeded from the buffer at construction.  A step is ONE
    launch more, whatever the number of buffers (avmoe_opt_ema_buffers behind the update, same stream): it reads this step's d_n and the
    skip flag from the state block and computes shadow = fma(d_n, shadow, (1 - d_n) * buffer) -- the parameter average's expression --
    from the values the forward passes before this step have left.  No step-dependent host scalar, capturable; a skipped step leaves the
    shadows alone; the buffers themselves are only read.  `swap_ema()` / `ema_weights()` exchange buffers and shadows too (a second
    launch, in place), so an evaluation inside runs the averaged weights on averaged statistics, and `adapter_state_dict(model, ema=opt)`
    writes the averaged value of every buffer the optimizer holds.  Integer buffers (`num_batches_tracked`) are never averaged and never
    swapped.  `ema_buffers` are views of the shadows shaped like the buffers, `ema_buffer_names` their names; `state_dict()` carries them
    under "flat_adam" ("ema_buffers": CPU tensors, "ema_buffer_names"), `load_state_dict()` restores them, and a dict without them
    re-seeds the shadows from the current buffers.  Without the option the calls and launches of a step are what they were.

    Stochastic weight averaging.  `swa_start=N, swa_freq=c` (torch.optim.swa_utils.AveragedModel on the device; it selects the device
    path too, and is the alternative to `ema_decay`: giving both raises ValueError) keeps the UNIFORM average of the parameters after the
    applied steps N, N + c, N + 2c, ... -- the average over the tail of a run that SWA is defined by, which no decay below 1 expresses.
    It is the exponential average's machinery with another rule for the decay: with n = applied_steps after the step, the finalize
    launch writes d = 0 for n < N (the average follows the parameters: an "averaged" checkpoint taken early holds the raw weights),
    d = k / (k + 1) with k = (n - N) / c on an averaging step (AveragedModel.update_parameters after optimizer.step() with
    n_averaged = k; the first one copies the parameters) and d = 1 between two of them (the average keeps its value); `swa_decay_at` /
    `swa_n_averaged_at` are the host's copies, `last_ema_decay` the value on the device.  The number of models averaged is a function of
    applied_steps alone: no counter more, a skipped step advances nothing, a captured step averages on replay, the launches of a step
    are those of `ema_decay`.  `ema_params`, `swap_ema()`, `ema_weights()`, `ema_buffers=` (the buffers' shadows get the same d),
    `adapter_state_dict(model, ema=opt)`, `save_adapters(..., ema=opt)` and `reestimate_bn(model, batches, ema=opt)` -- torch's
    update_bn for the averaged weights -- serve the uniform average unchanged.  The SWA learning rate is the schedule's part:
    `LRSchedule(..., swa_start=, swa_factor=, swa_anneal_steps=, swa_anneal=)`; either may be used without the other.  `state_dict()`
    carries "swa_start" / "swa_freq" beside the averages ("ema") and `load_state_dict()` restores them; a dict with them does not load
    into an optimizer built without `swa_start` (ValueError), one without them re-seeds the averages from the current parameters.

    Per-parameter gradient norms.  `report_grad_norms=True` (it selects the device path too) adds ONE launch behind the finalize launch:
    a wave per parameter adds the block sums the norm pass has left anyway, in a fixed order, and writes the parameter's gradient norm
    into a report buffer on the device; the lowest index of a parameter whose norm is Inf or NaN goes into its header.  The norm pass then
    runs on every step, so `last_grad_norm` is the true norm also without clipping and skipping (the clip factor stays exactly 1, and
    parameters, moments and averages get the bits they get without the option).  `last_param_grad_norms` (fp32, `len(params)`, in `params`
    order) and `first_nonfinite_param` (int32, -1 for none) are DEVICE tensors, views of the report: both are rewritten by every step, a
    skipped one included, and by every replay of a captured step.  The norms are those of gradient * grad_scale before clipping -- under
    data parallelism after `red.finish()`, like `last_grad_norm`.  `param_names(model)` gives the names to index with:

        opt = FlatAdam(red, skip_nonfinite=True, report_grad_norms=True); names = opt.param_names(model)
        ...
        if int(opt.skipped_steps) > seen: print("skipped by", names[int(opt.first_nonfinite_param)])

    Sharpness-aware minimization.  `sam_rho=rho` (SAM, Foret et al. 2021; `sam_adaptive=True`: ASAM, Kwon et al. 2021; it selects the
    device path too) lets a step use the gradient at w + e, the worst point of the rho-ball around the weights that a first gradient g
    points to: e = rho g / ||g||, adaptive e = rho w^2 g / || |w| g ||.  A step is then two backward passes with `sam_perturb()` between
    them:

        red.begin(sync); loss_fn(model(batch)).backward(); red.finish()
        opt.sam_perturb()                                   # w <- w + e, the originals kept on the device
        red.zero_grad(lazy=True); red.begin(sync)
        with hold_bn_stats(model): loss_fn(model(batch)).backward()
        red.finish(); opt.step()                            # w restored exactly, then Adam with the gradient at w + e

    `sam_perturb()` is three launches for ALL buckets (include/avmoe.h, avmoe_opt_sam_perturb): the norm pass of the step over the first
    gradient (adaptive: over |w| g), a one-block finalize that leaves norm, scale = rho / (norm + 1e-12) and a non-finite flag in a
    16-byte block on the device, and one pass that copies every parameter into a flat HOLD buffer per bucket (the bucket's layout once
    more, like the averages) and adds e in place -- the sites see the perturbed weights through the pointers they cache.  It uses the
    gradient scale of `step()`.  The `step()` behind it makes its usual norm call on the SECOND gradient (clipping, skipping, schedule,
    averages: all unchanged) and then ONE update launch that reads every parameter from the hold buffer and writes it to the parameter:
    the weights the update starts from are the unperturbed ones bit for bit (a copy, where w + e - e would drift), parameters, moments
    and averages get the bits a step without SAM gets from the same gradient, and the launches of a step are those without SAM.  A step
    that is skipped (`skip_nonfinite`) still writes the held weights back.  A first gradient that is not finite perturbs nothing
    (`sam_nonfinite` is 1, `last_sam_scale` 0) and the step goes on as usual; a zero one leaves every bit.  No host synchronisation and
    no step-dependent host scalar: both calls can be captured into graphs.  `step()` without a `sam_perturb()` before it is the step
    without SAM, with the same calls -- SAM on every k-th step is the caller's `if`.  `sam_restore()` abandons a perturbation in one
    launch.  `perturbed` is host state; `last_sam_norm`, `last_sam_scale`, `sam_nonfinite` are DEVICE views of the 16-byte block.  While
    perturbed, `swap_ema()`, `ema_weights()`, `state_dict()`, `load_state_dict()`, a second `sam_perturb()` and
    `adapter_state_dict(..., ema=opt)` / `save_adapters(..., ema=opt)` raise RuntimeError.  `state_dict()` carries "sam_rho" and
    "sam_adaptive" under "flat_adam" (the hold buffers are transient: no tensor state) and `load_state_dict()` into an optimizer built
    with `sam_rho` restores them; a dict without them loads as before.  The second pass must not advance the BatchNorm running
    statistics a second time, and on perturbed weights: run it inside `hold_bn_stats(model)`.
    Under data parallelism `sam_perturb()` after `red.finish()` perturbs with the averaged gradient, identically on every rank -- two
    all-reduces per step; after `red.begin(sync=False)` for the first pass each rank perturbs with its own gradient (m-sharpness), which
    is safe because the weights come back from the hold buffers and not by subtraction: the ranks' weights agree again after `step()`.
    NOT covered: the plain (non-device) path, a per-group rho, parameters outside the reducer.

    Layer-wise trust ratios.  `trust_ratio=True` (LAMB, You et al. 2020; it selects the device path too) rescales every adapted
    parameter's step by ||w|| / ||u||, the norm of the parameter over the norm of its update direction -- the tool for batch sizes far
    above the one a recipe was tuned at, where Adam with a linearly scaled rate fails.  Per parameter, with g' = g * grad_scale * clip
    factor and the moments formed exactly as without the option:

        coupled decay:                    u = m_hat / (sqrt(v_hat) + eps)              (the decay joined the gradient, as in Adam)
        decoupled_weight_decay (LAMB):    u = m_hat / (sqrt(v_hat) + eps) + wd * w
        ratio = ||w|| / ||u||; 1 where either norm is 0 or not finite; min(ratio, trust_clip) with `trust_clip`
        w = w - lr * lr_factor * ratio * u

    with w the weights before the step (behind `sam_perturb()` the held ones, for the norm too) and the bias corrections of Adam, as in
    the paper and in NVIDIA's implementation.  Adapted by default: parameters with `dim() >= 2` -- conv / linear weights and
    `my_tokens`.  Not adapted: gates, biases, BatchNorm / LayerNorm weights -- scalars and vectors whose norm says nothing about a step
    size (the gates start at exactly 0); they take ratio exactly 1 through the same kernels.  A `param_groups` entry may carry
    "trust_ratio": True | False for its parameters.  The recipe: `FlatAdam(red, lr=..., weight_decay=0.01, decoupled_weight_decay=True,
    trust_ratio=True, max_grad_norm=1.0, lr_schedule=LRSchedule(warmup_steps=...))`.
    A step is the unchanged norm call and then THREE launches in place of the update (include/avmoe.h, avmoe_opt_lamb_step): the moments
    with per-block sums of u^2 and w^2 in double, a wave per parameter that adds them in a fixed order and writes norms and ratio, and
    the update, which recomputes u from the stored moments by the same helper -- 5 launches with clipping or skipping on, no host
    synchronisation, no step-dependent host scalar, capturable; a host implementation needs two norms per tensor per step.  The moments
    are bit-equal to Adam's from the same inputs; the parameters are NOT bit-equal to the Adam update even at ratio 1, because u is
    formed in another order of operations (tests hold it to an fp64 bound from its own operands).  Schedule, averages, averaged
    buffers, skipping, per-parameter gradient norms and SAM compose unchanged.  `last_trust_ratios`, `last_param_norms`,
    `last_update_norms` are fp32 DEVICE views (`len(params)`, `params` order) of the last applied step; `adapted` is host state;
    `trust_ratio_of(w_norm, u_norm, clip)` is the host's copy of the rule.  `state_dict()` carries "trust_ratio" / "trust_clip" under
    "flat_adam" (no tensors), `load_state_dict()` into an optimizer built with the option restores the clamp, a dict without them loads
    as before.  Under data parallelism the gradients agree on every rank after `red.finish()`, and so do moments, norms and ratios: no
    communication is added.  NOT covered: the plain (non-device) path, parameters outside the reducer.

    Learning-rate estimation.  `prodigy=True` (Prodigy, Mishchenko & Defazio 2024; it selects the device path too) replaces the base
    rate by an estimate d that the step maintains: every rate -- `lr`, a group's "lr", times the schedule's factor -- is a MULTIPLIER of
    d (default use: `lr=1.0`; the reference's lr / lr_mlp ratio between groups keeps its meaning).  With g' the gradient as the update
    sees it (scale, clip factor, coupled decay), step = lr * lr_factor * d and c = step * d / d0 (`prodigy_safeguard_warmup`:
    c = d * d / d0):

        m = b1 m + (1 - b1) d g' ;  v = b2 v + (1 - b2) (d g')^2 ;  s = beta3 s + c g'          beta3 = sqrt(b2)
        num = beta3 num + sum c g' (x0 - w) ;  den = sum |s| ;  d_hat = d_coef num / den
        w = w - step m / (sqrt(v) + d eps)
        d_max = max(d_max, d_hat) ;  d = min(d_max, d * growth)        (without `prodigy_growth`: d = d_max)

    with w the weights before the step (behind `sam_perturb()` the held ones) and x0 the weights when the optimizer was built or its
    state loaded.  d starts at `prodigy_d0` and never falls; step k uses d_k.  There is NO bias correction, as in the paper: use
    `lr_schedule=LRSchedule(warmup_steps=...)`, and `prodigy_safeguard_warmup=True` with it.  The recipe: `FlatAdam(red, lr=1.0,
    prodigy=True, weight_decay=0.01, decoupled_weight_decay=True, max_grad_norm=1.0, lr_schedule=LRSchedule(warmup_steps=...))`.
    A step is the unchanged norm call and then TWO launches in place of the update (include/avmoe.h, avmoe_opt_prodigy_step): the update
    with per-block sums of both reductions in double, and one block that adds them in a fixed order and writes d for the next step --
    no host synchronisation, no step-dependent host scalar, capturable; a host implementation needs a dot product and an L1 norm over
    every tensor and a host read of d per step.  One flat x0 and one flat s buffer per bucket, with the bucket's layout.  Clipping,
    skipping (a skipped step leaves d, num, s and everything else bit for bit), both decays, schedule, averages, averaged buffers,
    per-parameter gradient norms and SAM compose unchanged; `trust_ratio` together with it raises ValueError (two rules for the step
    size).  `prodigy_d`, `prodigy_d_hat` are fp32 DEVICE scalars (views of the 32-byte Prodigy block; `prodigy_d` is the d of the NEXT
    step), `prodigy_x0`, `prodigy_s` lists of DEVICE views in `params` order; `prodigy_d_next(...)` is the host's copy of the finalize
    rule.  `state_dict()` carries the constants, "prodigy_d" / "prodigy_d_max" / "prodigy_d_hat" / "prodigy_num" / "prodigy_den",
    "prodigy_x0" and "prodigy_s" under "flat_adam"; `load_state_dict()` restores them, a dict without them re-seeds (x0 = the CURRENT
    parameters, s = 0, d = d0: load the model first), and a dict saved with the option does not load into an optimizer built without
    it (ValueError).  Under data parallelism the gradients agree on every rank after `red.finish()` and the parameters start equal, so
    x0, s, both sums and d agree too: no communication is added (verified on one rank).  NOT covered: `trust_ratio` together with it,
    bias correction, the plain (non-device) path, parameters outside the reducer.

    Orthogonalised momentum.  `muon=True` (Muon, Jordan et al. 2024; torch.optim.Muon's rule with the iteration in fp32; it selects the
    device path too) steps the small hidden matrices -- the experts' down_sampler / up_sampler, the latent tokens, the router's Linear
    layers -- along the nearest semi-orthogonal matrix of their momentum.  A parameter is orthogonalised when `dim() >= 2` and, with
    rows = shape[0], cols = numel // rows (a conv weight flattened), min(rows, cols) <= 128 and numel <= `muon_max_numel`
    (`muon_shape_of`, `muon_select`); a group's "muon": True | False overrides, True on a parameter that does not fit raises ValueError
    naming it.  Every other parameter takes the unchanged Adam / AdamW step, bit for bit.  With g' the gradient as the update sees it
    (scale, clip factor, coupled decay), mu = `muon_momentum` and w the weights before the step (behind `sam_perturb()` the held ones):

        m = mu m + (1 - mu) g' ;  u = (1 - mu) g' + mu m   (`muon_nesterov`; else u = m)         m lives in exp_avg, exp_avg_sq stays zero
        X = u / (||u||_F + 1e-7) ;  `muon_ns_steps` times  X <- a X + (b A + c A A) X,  A = X X^T      (a, b, c) = (3.4445, -4.7750, 2.0315)
        s = 0.2 sqrt(max(rows, cols))   ("match_rms_adamw": the recipe's Adam learning rates keep their meaning)
          = sqrt(max(1, rows / cols))   (`muon_scale="original"`)
        w = w (1 - lr lr_factor wd)   (decoupled decay only) ;  w = w - (lr lr_factor s) X

    without a bias correction; `betas` and `eps` keep serving the other parameters; a zero u gives a zero step.  The recipe:
    `FlatAdam(red, lr=args.lr, muon=True, weight_decay=0.01, decoupled_weight_decay=True, max_grad_norm=1.0)`.  A step is the unchanged
    norm call and then TWO launches in place of the update whatever the number of parameters (include/avmoe.h, avmoe_opt_muon_step):
    one over the table that updates the other parameters and leaves m, u and per-block sums of u^2, and one with a workgroup per
    matrix that keeps the Gram matrix in LDS, streams the matrix through it and applies the step -- no host synchronisation, no
    step-dependent host scalar, capturable; a host implementation needs about fifteen small GEMM launches per matrix.  One flat work
    buffer per bucket, with the bucket's layout.  Clipping, skipping (a skipped step leaves every bit; behind a perturbation it writes
    the held weights back and nothing else), both decays, schedule, averages, averaged buffers, per-parameter gradient norms and SAM
    compose unchanged; `trust_ratio` or `prodigy` together with it raises ValueError.  `orthogonalized` and `muon_scales` are host lists
    in `params` order, `last_muon_updates` DEVICE views of the applied direction X per parameter (None where not orthogonalised),
    `last_muon_norms` an fp32 DEVICE tensor of ||u||_F.  `state_dict()` keeps torch's format (exp_avg is the momentum) and carries the
    constants under "flat_adam"; a dict saved with the option does not load into an optimizer built without it (ValueError).  Under
    data parallelism the gradients agree on every rank after `red.finish()` and so does every step: no communication is added
    (verified on one rank only).  NOT covered here: a short side above 128 (`muon_large` below), a matrix split across workgroups, the plain (non-device) path,
    an iteration in bf16 and with it torch.optim.Muon's bits.

    The large matrices.  `muon=True, muon_large=True` also orthogonalises what the small rule declines -- for its short side or for its
    numel: every site's conv_adapter and fc, the "v1" attention projections, a 128 x 4096 matrix -- where min(rows, cols) <= 2048
    (`MUON_LARGE_MAX_DIM`) and numel <= `muon_large_max_numel` (`muon_large_shape_of`, `muon_select_paths`; `muon_paths` says "small" |
    "large" | None per parameter).  The small rule stays first and keeps its kernel and its bits; a group's "muon": True on a parameter
    only the large path fits is accepted.  The rule is the one above, exactly; only the three products of an iteration differ: they run
    on the library's tiled engine with fp32 operands in three-plane form (5.8e-9 relative per product; include/avmoe.h,
    avmoe_opt_muon_step_large).  The matrices are grouped into classes of equal (short side, long side); one launch normalises and
    packs all of them into a staging area that gives each class a uniform batch stride, three engine launches per class and iteration
    run batched over the class, one launch applies decay, update and shadow: 2 + 1 + 3 * ns_steps * classes (+ the engine's split-K
    reduces) + 1 launches behind the norm call (avmoe_opt_muon_step's two when no parameter is large), no allocation, no host
    synchronisation, no step-dependent host scalar, capturable.  Clipping, skipping, both decays, schedule, averages, SAM and
    `orthogonalized`, `muon_scales`, `last_muon_updates`, `last_muon_norms` cover large matrices like small ones.  `state_dict()`
    carries "muon_large" and "muon_large_max_numel"; a dict saved with the option does not load into an optimizer built without it
    (ValueError), one without it loads as before.  A library without the entry point raises AvmoeError.  The data-parallel statement
    above holds unchanged (documented from the code, verified on one rank only).  NOT covered: a short side above 2048.

    Schedule-free.  `schedule_free=True` (Schedule-Free AdamW, Defazio et al. 2024, "The Road Less Scheduled"; it selects the device
    path too) removes the run length from the recipe: a constant rate after a warm-up, and the weights one evaluates are as good as a
    tuned decay's at whatever step the run stops.  Three sequences per parameter: z, the base sequence that takes the steps (it lives in
    exp_avg); x, the running average of z that is evaluated (it lives in the shadow buffers of the averages); and y, an interpolation
    of the two at which the gradient is taken -- the parameter as the sites see it.  With g' the gradient as the update sees it
    (scale, clip factor, coupled decay at y), n = applied_steps after the step and f the schedule's factor (1 without one):

        f_max = max(f_max, f) ;  w = n^sf_r * f_max^sf_lr_power ;  weight_sum += w ;  c = w / weight_sum ;  d = 1 - c
        v = b2 v + (1 - b2) g'^2 ;  u = g' / (sqrt(v_hat) + eps)     (decoupled_weight_decay: u = u + wd * y)
        z = z - lr * f * u ;  x = d x + c z ;  y = b1 x + (1 - b1) z

    There is no momentum buffer and no first-moment bias correction: betas[0] is the interpolation.  The first applied step has c = 1
    and x = z exactly; betas[0] = 0 gives y = z exactly; with sf_r = 0 and a constant factor x is the uniform mean of z.  The recipe:
    `FlatAdam(red, lr=args.lr, schedule_free=True, weight_decay=0.01, decoupled_weight_decay=True, max_grad_norm=1.0,
    lr_schedule=LRSchedule(warmup_steps=...))` -- a warm-up and NO decay.  The protocol: train on the parameters as they are (y), and
    evaluate or checkpoint inside `with opt.ema_weights():` after `reestimate_bn(model, batches, ema=opt)` -- the swap is the averages'
    exact exchange launch, not a back-conversion from y, and it gives every byte back.
    A step is the unchanged norm call (without the averages' flags) and then TWO launches in place of the update whatever the number of
    parameters (include/avmoe.h, avmoe_opt_sf_step): one thread advances weight_sum, f_max, c and d in a 32-byte block on the device
    from the counters the finalize launch has just written, and one table walk reads y, the gradient, z, v and x and writes y, z, v and
    x -- the norm call + 2, no host synchronisation, no step-dependent host scalar, capturable; a host implementation needs a handful
    of foreach passes per step and two full passes over the weights at every train / eval switch.  Clipping, skipping (a skipped step
    leaves every bit, the block included; behind a perturbation it writes the held weights back and nothing else), both decays, the
    schedule, per-group rates and decays, per-parameter gradient norms, SAM (y is then the held value) and `ema_buffers=` (the buffers'
    shadows take the same d) compose unchanged; `ema_decay`, `swa_start`, `trust_ratio`, `prodigy` or `muon` together with it raise
    ValueError.  `ema_params`, `swap_ema()`, `ema_weights()`, `last_ema_decay` (= d), `adapter_state_dict(model, ema=opt)`,
    `save_adapters(..., ema=opt)` and `reestimate_bn(model, batches, ema=opt)` serve x unchanged.  `schedule_free`, `sf_r`,
    `sf_lr_power` are host attributes; `sf_c` (fp32), `sf_weight_sum` (fp64), `sf_lr_max` (fp32) DEVICE views of the block; `sf_z`
    DEVICE views of z in `params` order; `sf_weights_next(...)` is the host's copy of the scalar rule.  `state_dict()` keeps torch's
    format (exp_avg is z) and carries "schedule_free", "sf_r", "sf_lr_power", "sf_weight_sum", "sf_lr_max", "sf_c" (and "sf_d") under
    "flat_adam", with x in the "ema" list; `load_state_dict()` restores them; a dict saved with the option does not load into an
    optimizer built without it (ValueError); one without it keeps exp_avg_sq and the counters, re-seeds z = x = the CURRENT parameters
    and zeroes the block, so load the model first.  Under data parallelism the gradients agree on every rank after `red.finish()` and
    so does every step: no communication is added (verified on one rank only).  NOT covered: the per-epoch StepLR decay (`step_size`
    / `gamma`) scales the rate through the range table but is not part of f, so it does not enter the averaging weights; the plain
    (non-device) path; parameters outside the reducer (neither stepped nor averaged); the schedulefree package's bits (its bias
    correction rides in the rate and its weights use lr_max: another order of operations).

    Resuming.  `state_dict()` / `load_state_dict()` speak torch.optim.Adam's format: `state[i] = {"step", "exp_avg", "exp_avg_sq"}` (CPU
    tensors shaped like the parameter), `param_groups` with lr / betas / eps / weight_decay / params, plus one extra key "flat_adam" (t, epoch,
    counters, options, the schedule) that torch ignores.  With a schedule a group's "lr" is the rate of the NEXT step, lr0 * decay *
    f(applied_steps), and "initial_lr" stays lr0 -- what a torch optimizer + scheduler pair saves; nothing but `applied_steps` is needed
    to continue the schedule.  Index i is the position of the parameter in `opt.params` -- the order in which the reducer
    holds the parameters: bucket by bucket, inside a bucket the sites in reverse execution order with each site's parameters in its
    grad_layout() order, then the plain parameters in reverse order.  A torch optimizer built as
    `torch.optim.AdamW(opt.torch_param_groups())` (or `Adam`) loads the dict, and a dict from such an optimizer loads here.
    """

    def __init__(self, reducer, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0,
                 step_size: Optional[int] = None, gamma: float = 0.1, grad_scale: float = 1.0, param_groups=None,
                 max_grad_norm: Optional[float] = None, decoupled_weight_decay: bool = False, skip_nonfinite: bool = False,
                 lr_schedule: Optional[LRSchedule] = None, ema_decay: Optional[float] = None, ema_warmup: float = 10.0,
                 report_grad_norms: bool = False, ema_buffers=None, swa_start: Optional[int] = None, swa_freq: int = 1,
                 sam_rho: Optional[float] = None, sam_adaptive: bool = False, trust_ratio: bool = False,
                 trust_clip: Optional[float] = None, prodigy: bool = False, prodigy_d0: float = 1e-6, prodigy_d_coef: float = 1.0,
                 prodigy_growth: Optional[float] = None, prodigy_safeguard_warmup: bool = False, muon: bool = False,
                 muon_momentum: float = 0.95, muon_nesterov: bool = True, muon_ns_steps: int = 5, muon_scale: str = "match_rms_adamw",
                 muon_max_numel: int = 262144, muon_large: bool = False, muon_large_max_numel: int = 1 << 23,
                 schedule_free: bool = False, sf_r: float = 0.0, sf_lr_power: float = 2.0):
        """max_grad_norm: clip the global gradient norm to it (None: off).  decoupled_weight_decay: torch.optim.AdamW instead of Adam's L2
        term.  skip_nonfinite: a step whose gradient norm is Inf / NaN changes nothing and is counted in `skipped_steps`.  lr_schedule: a
        per-step LRSchedule evaluated on the device.  ema_decay: keep an exponential moving average of the parameters with this decay in
        [0, 1), warmed up over `ema_warmup` >= 1 (1: constant decay); both are held as fp32.  report_grad_norms: every step also leaves
        each parameter's gradient norm and the index of the first non-finite one on the device (`last_param_grad_norms`,
        `first_nonfinite_param`).  swa_start: keep the uniform average of the parameters over the applied steps swa_start,
        swa_start + swa_freq, ... (integers >= 1, steps counted from 1; class docstring, "Stochastic weight averaging") in place of the
        exponential one: giving it together with `ema_decay` raises ValueError.  sam_rho: the radius rho >= 0 (held as fp32) of
        sharpness-aware minimization, `sam_perturb()` between two backward passes (class docstring); sam_adaptive: its adaptive form
        (ValueError without `sam_rho`).  trust_ratio: layer-wise trust ratios (LAMB; class docstring): every adapted parameter's step is
        scaled by ||w|| / ||update||, computed on the device; trust_clip: the largest ratio allowed (a finite number > 0, held as fp32;
        None: no clamp; ValueError without `trust_ratio`).  prodigy: Prodigy learning-rate estimation (class docstring): every rate is a
        multiplier of an estimate d kept on the device; prodigy_d0 > 0: its start, prodigy_d_coef > 0: a factor on the estimate,
        prodigy_growth >= 1 or None: the largest factor d may grow by per step, prodigy_safeguard_warmup: leave the rate out of a step's
        weight in the estimate (all held as fp32; ValueError for a bad value, for one given without `prodigy`, and for `prodigy` with
        `trust_ratio`).  muon: orthogonalised momentum for the small hidden matrices (class docstring): a parameter with `dim() >= 2`
        whose short side is at most 128 and whose numel is at most `muon_max_numel` steps along the nearest semi-orthogonal matrix of
        its momentum; muon_momentum in [0, 1) (held as fp32), muon_nesterov, muon_ns_steps in 1..16, muon_scale "match_rms_adamw" |
        "original" (ValueError for a bad value, for one given without `muon`, and for `muon` with `trust_ratio` or `prodigy`).
        muon_large: also orthogonalise the matrices the small rule declines, on the tiled engine (class docstring, "The large
        matrices"): short side at most 2048 and numel at most `muon_large_max_numel` (ValueError for a non-bool, without `muon`, for a
        bad `muon_large_max_numel` or one given without `muon_large`).
        schedule_free: schedule-free AdamW (class docstring, "Schedule-free"): a constant rate, the gradient taken at an interpolation of
        a base sequence and its running average, which `ema_params` / `ema_weights()` serve; sf_r >= 0 and sf_lr_power >= 0 (held as
        fp32): a step's weight in the average grows like n^sf_r * (largest schedule factor so far)^sf_lr_power (ValueError for a bad
        value, for one given without `schedule_free`, and for `schedule_free` with `ema_decay`, `swa_start`, `trust_ratio`, `prodigy`
        or `muon`).
        Any of the twelve selects the device path (class docstring); with all at their
        defaults step() is the per-bucket avmoe_adam_step path.  ema_buffers: a torch.nn.Module (its named_buffers()) or an iterable of (name, tensor) to average
        and swap with the weights; needs `ema_decay`, `swa_start` or `schedule_free`.  Floating-point buffers must be contiguous fp32 on the optimizer's GPU (ValueError
        otherwise); integer and empty ones are left out, and a tensor listed twice (same address) is held once.
        param_groups: the list `select_trainable` returns ({"params": p, "lr": ...} per parameter, as handed to
        torch.optim.Adam at AVE/main_trans_v3.py:313-322): each parameter is stepped with ITS group's learning rate (the
        reference's `lr_mlp` for the classifier head vs `lr` for the adapters); parameters not listed use `lr`.  A group may also
        carry "weight_decay" (the AdamW recipe {"params": biases_and_norms, "weight_decay": 0.0}): it applies to that group's parameters,
        on both paths, coupled and decoupled; parameters not listed, or listed without the key, use `weight_decay`.  `betas` and `eps`
        stay per optimizer: a group's own are ignored.  On the plain path, neighbouring parameters of a bucket with the same rate and
        decay share one kernel launch (an adapter site is one range).  With `trust_ratio` a group may carry "trust_ratio": True | False,
        which overrides the default (adapted: `dim() >= 2`) for that group's parameters.  With `muon` a group may carry
        "muon": True | False likewise; True on a parameter that does not fit raises ValueError naming it."""
        self.reducer, self.lr0, self.betas, self.eps, self.wd = reducer, lr, betas, eps, weight_decay
        self.step_size, self.gamma, self.grad_scale = step_size, gamma, grad_scale
        self.t, self.epoch = 0, 0
        self.state = []
        if max_grad_norm is not None and not (float(max_grad_norm) >= 0.0):
            raise ValueError("max_grad_norm must be >= 0")
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.decoupled_weight_decay, self.skip_nonfinite = bool(decoupled_weight_decay), bool(skip_nonfinite)
        if lr_schedule is not None and not isinstance(lr_schedule, LRSchedule):
            raise TypeError("lr_schedule must be an avmoe_amd.train.LRSchedule")
        self.lr_schedule = lr_schedule
        self.ema_decay, self.ema_warmup = self._check_ema(ema_decay, ema_warmup)
        self.swa_start, self.swa_freq = self._check_swa(swa_start, swa_freq)
        if self.swa_start is not None and self.ema_decay is not None:
            raise ValueError("swa_start and ema_decay are alternatives: the optimizer keeps one average of the weights")
        self._swapped = False                            # the parameters currently hold the averages (swap_ema / ema_weights)
        self.sam_rho, self.sam_adaptive = self._check_sam(sam_rho, sam_adaptive)
        self._perturbed = False                          # the parameters currently hold w + e, the hold buffers w (sam_perturb)
        self.trust_ratio, self.trust_clip = self._check_trust(trust_ratio, trust_clip)
        self.prodigy, self.prodigy_d0, self.prodigy_d_coef, self.prodigy_growth, self.prodigy_safeguard_warmup = \
            self._check_prodigy(prodigy, prodigy_d0, prodigy_d_coef, prodigy_growth, prodigy_safeguard_warmup)
        if self.prodigy and self.trust_ratio:
            raise ValueError("prodigy and trust_ratio are two rules for the step size: choose one")
        self.muon, self.muon_momentum, self.muon_nesterov, self.muon_ns_steps, self.muon_scale, self.muon_max_numel = \
            self._check_muon(muon, muon_momentum, muon_nesterov, muon_ns_steps, muon_scale, muon_max_numel)
        self.muon_large, self.muon_large_max_numel = self._check_muon_large(muon_large, muon_large_max_numel, self.muon)
        if self.muon and (self.trust_ratio or self.prodigy):
            raise ValueError("muon and trust_ratio / prodigy are different rules for the step: choose one")
        self.schedule_free, self.sf_r, self.sf_lr_power = self._check_sf(schedule_free, sf_r, sf_lr_power)
        if self.schedule_free:
            other = [k for k, on in (("ema_decay", self.ema_decay is not None), ("swa_start", self.swa_start is not None),
                                     ("trust_ratio", self.trust_ratio), ("prodigy", self.prodigy), ("muon", self.muon)) if on]
            if other:
                raise ValueError(f"schedule_free and {' / '.join(other)} do not combine: schedule_free keeps its own average in the shadow "
                                 "buffers and its own rule for the step")
        for grp in (param_groups or []):                 # before anything is touched
            if "trust_ratio" in grp and not isinstance(grp["trust_ratio"], bool):
                raise ValueError(f"a parameter group's \"trust_ratio\" must be True or False, not {grp['trust_ratio']!r}")
        self._muon_paths_of([], param_groups)            # the groups' "muon" keys, likewise
        self.report_grad_norms = bool(report_grad_norms)
        self._ebufs = self._collect_buffers(ema_buffers, reducer)      # [(name, tensor)]: the buffers averaged with the weights
        self._recs: List[_ParamRecord] = []              # one record per parameter, in the reducer's order
        lr_of, wd_of, adapt_of = {}, {}, {}
        for grp in (param_groups or []):
            ps = grp["params"]
            for p in ([ps] if isinstance(ps, torch.Tensor) else ps):
                lr_of[id(p)] = float(grp.get("lr", lr))
                if "trust_ratio" in grp:
                    adapt_of[id(p)] = grp["trust_ratio"]
                if "weight_decay" in grp:
                    wd_of[id(p)] = float(grp["weight_decay"])
        for b in reducer.buckets:
            flat_g = b.flat
            if not flat_g.is_cuda:
                raise capi.AvmoeError("FlatAdam updates GPU buckets (no CPU fallback)")
            flat_p = torch.zeros_like(flat_g)
            for p in b.params:                           # parameter offsets = offsets of their .grad views in the bucket
                off = (p.grad.data_ptr() - flat_g.data_ptr()) // 4
                view = flat_p[off:off + p.numel()].view_as(p)
                view.copy_(p.data)
                p.data = view
                if view.data_ptr() % 16:
                    raise capi.AvmoeError("FlatAdam: a re-pointed parameter is not 16-byte aligned (the GEMM engine needs "
                                          "aligned operands); build the reducer with aligned buckets (avmoe_amd.dp)")
                path, shape = (self._muon_paths_of([p], param_groups)[0] or (None, None)) if self.muon else (None, None)
                self._recs.append(_ParamRecord(
                    p=p, bucket=len(self.state), off=off, lr0=lr_of.get(id(p), float(lr)), wd=wd_of.get(id(p), weight_decay),
                    adapted=adapt_of.get(id(p), p.dim() >= 2), muon_shape=shape, muon_path=path, state=self.state))
            self.state.append(dict(p=flat_p, g=flat_g, m=torch.zeros_like(flat_g), v=torch.zeros_like(flat_g), ranges=None))
        if self._averaging:                              # the averages: the bucket's layout once more, padding zero
            self._add_side_buffer("e", clone=True)
        if self.sam_rho is not None:                     # the hold buffers: the bucket's layout once more, written by every sam_perturb()
            self._add_side_buffer("h")
        if self.prodigy:                                 # x0 and the running gradient sum: the bucket's layout twice more, padding zero
            self._add_side_buffer("x0", clone=True)
            self._add_side_buffer("s")
        if self.muon:                                    # the work buffer: the bucket's layout once more; holds O after a step
            self._add_side_buffer("o")
        if self.schedule_free:                           # z lives in exp_avg and starts, like the average x, at the parameters
            self._seed_sf()
        self._rebuild_plain_ranges()
        self._device = self.max_grad_norm is not None or self.decoupled_weight_decay or self.skip_nonfinite or lr_schedule is not None \
            or self._averaging or self.report_grad_norms or self.sam_rho is not None or self.trust_ratio \
            or self.prodigy or self.muon or self.schedule_free
        if self._device:
            self._build_device_state()

    # ---- what every option shares ---------------------------------------------------------------------------------
    @staticmethod
    def _need(on, what, option):
        """an accessor or call `what` of an option that is off raises"""
        if not on:
            raise capi.AvmoeError(f"FlatAdam.{what} needs {option}")

    @staticmethod
    def _lib_with(symbol, feature, named=None):
        """the library, which must export `symbol`: one built before `feature` (named by its entry point) is refused"""
        L = capi.lib()
        if not hasattr(L, symbol):
            raise capi.AvmoeError(f"this libavmoe_hip.so lacks {feature} ({named or symbol}): rebuild it")
        return L

    def _add_side_buffer(self, key, clone=False):
        """a per-element side buffer: one more flat tensor per bucket with the bucket's layout, a clone of the parameters (padding zero)
        or zeros"""
        for s in self.state:
            s[key] = s["p"].clone() if clone else torch.zeros_like(s["p"])

    def _side_views(self, key, what):
        """-> (the views of side buffer `key` in `params` order, the int64 device array of one pointer per range, beside the range table)"""
        ptrs = [r.ptr(key) for r in self._recs]
        if any(q % 16 for q in ptrs):
            raise capi.AvmoeError(f"FlatAdam: {what} range is not 16-byte aligned")
        return [r.view(key) for r in self._recs], torch.tensor(ptrs, dtype=torch.int64).to(self._dev)

    # ---- the weight average ---------------------------------------------------------------------------------------
    @staticmethod
    def _check_ema(decay, warmup):
        """-> (decay, warmup) as the fp32 values the device holds, or (None, warmup) when the average is off"""
        w = float(warmup)
        if not (w >= 1.0) or math.isinf(w):
            raise ValueError(f"ema_warmup must be a finite number >= 1, not {warmup!r}")
        if decay is None:
            return None, _f32(w)
        d = float(decay)
        if not (0.0 <= d < 1.0) or _f32(d) >= 1.0:
            raise ValueError(f"ema_decay must be in [0, 1) (as fp32), not {decay!r}")
        return _f32(d), _f32(w)

    @staticmethod
    def ema_decay_at(n: int, decay: float, warmup: float = 10.0) -> float:
        """d_n = min(decay, (1 + n) / (warmup + n)) for n applied steps, this one included (the first step has n = 1): the finalize
        kernel's closed form on the host -- in double from the fp32 constants, rounded once to fp32 -- and equal to it bit for bit."""
        d, w = FlatAdam._check_ema(decay, warmup)
        if d is None:
            raise ValueError("ema_decay_at needs a decay")
        n = int(n)
        return _f32(min(d, (1.0 + n) / (w + n)))

    @staticmethod
    def _check_swa(start, freq):
        """-> (start, freq) as integers, or (None, freq) when the uniform average is off"""
        for name, v in (("swa_start", start), ("swa_freq", freq)):
            if v is None and name == "swa_start":
                continue
            if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or int(v) != v or v < 1:
                raise ValueError(f"{name} must be an integer >= 1, not {v!r}")
        if int(freq) > 2 ** 31 - 1:
            raise ValueError(f"swa_freq must fit 32 bits, not {freq!r}")
        return (None if start is None else int(start)), int(freq)

    @staticmethod
    def swa_n_averaged_at(n: int, start: int, freq: int = 1) -> int:
        """the number of models in the uniform average after n applied steps: the steps start, start + freq, ... up to n (torch's
        AveragedModel.n_averaged)"""
        start, freq = FlatAdam._check_swa(start, freq)
        if start is None:
            raise ValueError("swa_n_averaged_at needs a start")
        n = int(n)
        return 0 if n < start else (n - start) // freq + 1

    @staticmethod
    def swa_decay_at(n: int, start: int, freq: int = 1) -> float:
        """the decay d of the uniform average for n applied steps, this one included (the first step has n = 1): 0 below `start` (the
        average follows the parameters), k / (k + 1) where this step is the k-th averaged one after the first, k = (n - start) / freq,
        and exactly 1 between two averaged steps.  The finalize kernel's closed form on the host -- formed in double, rounded once to
        fp32 -- and equal to it bit for bit."""
        start, freq = FlatAdam._check_swa(start, freq)
        if start is None:
            raise ValueError("swa_decay_at needs a start")
        n = int(n)
        if n < start:
            return 0.0
        if (n - start) % freq:
            return 1.0
        k = float((n - start) // freq)
        return _f32(k / (k + 1.0))

    @property
    def _averaging(self) -> bool:
        """the optimizer keeps an average of the weights: the exponential one (ema_decay), the uniform one (swa_start) or schedule-free
        AdamW's x (schedule_free)"""
        return self.ema_decay is not None or self.swa_start is not None or self.schedule_free

    def _decay_at(self, n: int) -> float:
        """the decay word of the state block after n applied steps, by the rule of the average that is on"""
        if self.swa_start is not None:
            return self.swa_decay_at(n, self.swa_start, self.swa_freq)
        return self.ema_decay_at(n, self.ema_decay, self.ema_warmup)

    def _collect_buffers(self, spec, reducer):
        """`ema_buffers` -> [(name, tensor)] of what is averaged: contiguous fp32, on the buckets' device, not empty, one per address"""
        if spec is None:
            return []
        if not self._averaging:
            raise ValueError("ema_buffers needs ema_decay, swa_start or schedule_free: the buffers are averaged with the decay of the weight "
                             "average")
        items = spec.named_buffers() if isinstance(spec, torch.nn.Module) else spec
        dev = reducer.buckets[0].flat.device if reducer.buckets else None
        out, seen = [], set()
        for name, t in items:
            if not isinstance(t, torch.Tensor):
                raise TypeError(f"ema_buffers: {name!r} is no tensor")
            if not t.is_floating_point() or t.numel() == 0:      # counters (num_batches_tracked) are never averaged and never swapped
                continue
            if t.dtype != torch.float32:
                raise ValueError(f"ema_buffers: buffer {name!r} is {t.dtype}, the average is kept in float32")
            if not t.is_contiguous():
                raise ValueError(f"ema_buffers: buffer {name!r} is not contiguous")
            if dev is not None and t.device != dev:
                raise ValueError(f"ema_buffers: buffer {name!r} is on {t.device}, the optimizer's buckets on {dev}")
            if t.data_ptr() in seen:
                continue
            seen.add(t.data_ptr())
            out.append((str(name), t))
        return out

    @property
    def ema_buffers(self) -> List[torch.Tensor]:
        """the averaged buffers as DEVICE tensors shaped like the buffers, in `ema_buffer_names` order: views of the one flat shadow
        allocation (inside `ema_weights()` they hold the raw buffers)"""
        self._need(self._ebufs, "ema_buffers", "ema_buffers")
        return list(self._ebuf_views)

    @property
    def ema_buffer_names(self) -> List[str]:
        """the names of the buffers the optimizer averages, as `named_buffers()` (or the caller's pairs) gave them"""
        return [name for name, _ in self._ebufs]

    def _build_buffer_table(self):
        """the shadows (ONE flat fp32 allocation, each 16-byte aligned, seeded from the buffers) and the buffer table on the device"""
        L = self._lib_with("avmoe_opt_swap_buffers", "the averaged buffers", "avmoe_opt_ema_buffers")
        offs, total = [], 0
        for _name, t in self._ebufs:
            offs.append(total)
            total += (t.numel() + 3) & ~3
        self._ebuf_flat = torch.zeros(total, dtype=torch.float32, device=self._dev)
        self._ebuf_views = [self._ebuf_flat[o:o + t.numel()].view_as(t) for o, (_n, t) in zip(offs, self._ebufs)]
        recs = (cm.OptBuffer * len(self._ebufs))()
        for r, (_name, t), v in zip(recs, self._ebufs, self._ebuf_views):
            r.buffer, r.shadow, r.n = t.data_ptr(), v.data_ptr(), t.numel()
        nb = C.c_int64(0)
        nbytes = L.avmoe_opt_buffer_table_bytes(recs, len(recs), C.byref(nb))
        if nbytes == 0:
            capi.check(-1, "avmoe_opt_buffer_table_bytes")
        img = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
        capi.check(L.avmoe_opt_buffer_table_build(recs, len(recs), img.data_ptr(), nbytes), "avmoe_opt_buffer_table_build")
        self._ebuf_table = torch.empty(nbytes, dtype=torch.uint8, device=self._dev)
        self._ebuf_table.copy_(img, non_blocking=True)
        self._ebuf_args = (self._ebuf_table.data_ptr(), len(recs), int(nb.value))      # table, n_buffers, n_blocks of both launches
        self._ebuf_blocks = int(nb.value)
        self._seed_buffer_shadows()

    def _seed_buffer_shadows(self):
        with torch.no_grad():
            for v, (_name, t) in zip(self._ebuf_views, self._ebufs):
                v.copy_(t)

    @property
    def ema_params(self) -> List[torch.Tensor]:
        """the averages as DEVICE tensors shaped like `params` and in that order: views of the shadow buffers (inside `ema_weights()`
        they hold the raw parameters)"""
        self._need(self._averaging, "ema_params", "ema_decay, swa_start or schedule_free")
        return list(self._ema_views)

    @property
    def last_ema_decay(self) -> torch.Tensor:
        """fp32 DEVICE scalar: the decay d_n the last applied step averaged with (a skipped step leaves it).  A view of the state block,
        like `last_lr_factor`; only with `ema_decay` or `swa_start` (there: 0 before the average starts, k / (k + 1) on an averaging
        step, 1 between two)."""
        self._need(self._averaging, "last_ema_decay", "ema_decay, swa_start or schedule_free")
        return self._state_view("ema_decay")

    def swap_ema(self):
        """Exchanges every parameter the optimizer holds with its average: ONE launch on the current stream, no copy and no
        synchronisation.  Call it again to swap back; until then step(), state_dict() and load_state_dict() raise.  With `ema_buffers` a
        second launch exchanges the buffers (BatchNorm running statistics) with their averages, in place: no `module._buffers` entry is
        re-bound.  Without it buffers stay as they are."""
        self._need(self._averaging, "swap_ema", "ema_decay, swa_start or schedule_free")
        self._not_perturbed("swap_ema()")
        stream = self._exchange(self._shadow_ptrs)
        if self._ebufs:
            capi.check(capi.lib().avmoe_opt_swap_buffers(*self._ebuf_args, stream),
                       "avmoe_opt_swap_buffers")
        self._swapped = not self._swapped

    def _exchange(self, ptrs):
        """ONE launch on the current stream (avmoe_opt_swap_ema) that exchanges every parameter with its range of the side buffer the
        device array `ptrs` points into: the averages (swap_ema) or the hold buffers (sam_restore); -> the stream"""
        stream = torch.cuda.current_stream(self._dev).cuda_stream
        capi.check(capi.lib().avmoe_opt_swap_ema(self._table_ptr, len(self._recs), self._n_blocks, ptrs.data_ptr(), stream), "avmoe_opt_swap_ema")
        return stream

    @contextlib.contextmanager
    def ema_weights(self):
        """`with opt.ema_weights(): evaluate(model)` -- the model's parameters are the averages inside (swap_ema), the raw weights again
        after it, also when the body raises.  step() inside raises.  With `ema_buffers` the BatchNorm running statistics are their
        averages inside too, and what the raw weights' forward passes left again after it; without the option they are not averaged, and
        an evaluation inside sees the raw weights' statistics."""
        self._need(self._averaging, "ema_weights", "ema_decay, swa_start or schedule_free")
        self._not_swapped("ema_weights()")
        self._not_perturbed("ema_weights()")
        self.swap_ema()
        try:
            yield self
        finally:
            self.swap_ema()

    def _save_average(self, extra):
        """state_dict(): the averages ("ema") with the constants of the rule that is on"""
        if self.ema_decay is not None:
            extra.update(ema_decay=self.ema_decay, ema_warmup=self.ema_warmup, ema=[e.detach().cpu().clone() for e in self._ema_views])
        if self.swa_start is not None:                   # the uniform average: the same "ema" list, with the constants that say so
            extra.update(swa_start=self.swa_start, swa_freq=self.swa_freq, ema=[e.detach().cpu().clone() for e in self._ema_views])
        if self.schedule_free:                           # x: the same "ema" list, beside the keys _save_sf writes
            extra.update(ema=[e.detach().cpu().clone() for e in self._ema_views])

    def _check_saved_average(self, extra):
        """load_state_dict(): -> (saved averages, the saved constants of this optimizer's rule), or None where the averages are re-seeded"""
        if extra.get("swa_start") is not None and self.swa_start is None:
            raise ValueError("the state dict carries a uniform weight average (swa_start), which this optimizer does not keep: build it "
                             "with swa_start (the saved swa_start / swa_freq then replace the constructor's)")
        # averages of the other kind (an exponential average's into a uniform one, or the reverse) are not this optimizer's: re-seed
        own_kind = (extra.get("swa_start") is not None) == (self.swa_start is not None) \
            and (extra.get("schedule_free") is True) == self.schedule_free
        saved = extra.get("ema") if self._averaging and own_kind else None
        if saved is None:
            return None
        if len(saved) != len(self._recs):
            raise ValueError(f"state dict has {len(saved)} averaged parameters, this optimizer {len(self._recs)}")
        for i, (e, r) in enumerate(zip(saved, self._recs)):
            if tuple(e.shape) != tuple(r.p.shape):
                raise ValueError(f"parameter index {i}: ema has shape {tuple(e.shape)}, the parameter {tuple(r.p.shape)}")
        if self.swa_start is not None:
            return saved, self._check_swa(extra["swa_start"], extra.get("swa_freq", self.swa_freq))
        if self.schedule_free:                           # x has no constants of its own: _check_saved_sf reads the rule's
            return saved, None
        return saved, self._check_ema(self.ema_decay if extra.get("ema_decay") is None else extra["ema_decay"],
                                      self.ema_warmup if extra.get("ema_warmup") is None else extra["ema_warmup"])

    def _apply_saved_average(self, payload, applied):
        if payload is not None:
            saved, consts = payload
            if self.swa_start is not None:
                self._set_swa(*consts)
            elif not self.schedule_free:
                self._set_ema(*consts)
            for view, e in zip(self._ema_views, saved):
                view.copy_(e.to(torch.float32))
        else:                                            # no averages in the dict: start them from the parameters as they are now
            for s in self.state:
                s["e"].copy_(s["p"])
        if not self.schedule_free:                       # (there the word is the block's d: _apply_saved_sf writes it)
            self._views["ema_decay"].fill_(self._decay_at(applied) if applied > 0 else 0.0)

    def _save_buffers(self, extra):
        extra.update(ema_buffers=[v.detach().cpu().clone() for v in self._ebuf_views], ema_buffer_names=self.ema_buffer_names)

    def _check_saved_buffers(self, extra):
        """load_state_dict(): -> the saved buffer averages, or None where the shadows are re-seeded"""
        saved = extra.get("ema_buffers") if self._ebufs else None
        if saved is not None:
            names = self.ema_buffer_names
            if len(saved) != len(names):
                raise ValueError(f"state dict has {len(saved)} averaged buffers, this optimizer {len(names)} (first: {names[0]!r})")
            for name, e, (_n, t) in zip(names, saved, self._ebufs):
                if tuple(e.shape) != tuple(t.shape):
                    raise ValueError(f"buffer {name!r}: the saved average has shape {tuple(e.shape)}, the buffer {tuple(t.shape)}")
        return saved

    def _apply_saved_buffers(self, saved):
        if saved is not None:
            for view, e in zip(self._ebuf_views, saved):
                view.copy_(e.to(torch.float32))
        else:                                            # no buffer averages in the dict: start them from the buffers as they are now
            self._seed_buffer_shadows()

    def _not_swapped(self, what):
        if self._swapped:
            raise RuntimeError(f"FlatAdam.{what} while the averaged weights are swapped in (swap_ema / ema_weights): swap back first")

    # ---- sharpness-aware minimization -----------------------------------------------------------------------------
    @staticmethod
    def _check_sam(rho, adaptive):
        """-> (rho as the fp32 value the device gets, adaptive), or (None, False) when SAM is off"""
        if rho is None:
            if adaptive:
                raise ValueError("sam_adaptive needs sam_rho: the adaptive perturbation has a radius too")
            return None, False
        r = float(rho)
        if not (r >= 0.0) or math.isinf(r) or r > 3.4028234663852886e38:
            raise ValueError(f"sam_rho must be a finite number >= 0 (as fp32), not {rho!r}")
        return _f32(r), bool(adaptive)

    def _not_perturbed(self, what):
        if self._perturbed:
            raise RuntimeError(f"FlatAdam.{what} while the weights are perturbed (sam_perturb): call step() or sam_restore() first")

    def _save_sam(self, extra):
        extra.update(sam_rho=self.sam_rho, sam_adaptive=self.sam_adaptive)       # constants only: the hold buffers are transient

    def _check_saved_sam(self, extra):
        """load_state_dict(): -> the saved (sam_rho, sam_adaptive), or None where the constructor's stay"""
        if self.sam_rho is not None and extra.get("sam_rho") is not None:
            return self._check_sam(extra["sam_rho"], extra.get("sam_adaptive", self.sam_adaptive))
        return None

    def _apply_saved_sam(self, consts):
        if consts is not None:
            self.sam_rho, self.sam_adaptive = consts

    def _build_sam(self):
        """the device array of one hold pointer per range, beside the shadows', and the 16-byte block sam_perturb()'s finalize writes"""
        self._lib_with("avmoe_opt_adam_step_sam", "sharpness-aware minimization", "avmoe_opt_sam_perturb")
        self._hold_ptrs = self._side_views("h", "a hold")[1]
        self._sam_block = torch.zeros(C.sizeof(cm.OptSamState), dtype=torch.uint8, device=self._dev)
        self._sam_views = {"norm": self._sam_block[0:4].view(torch.float32)[0], "scale": self._sam_block[4:8].view(torch.float32)[0],
                           "nonfinite": self._sam_block[8:12].view(torch.int32)[0]}

    @property
    def perturbed(self) -> bool:
        """host state: sam_perturb() has moved the weights and neither step() nor sam_restore() has brought them back yet"""
        return self._perturbed

    @property
    def last_sam_norm(self) -> torch.Tensor:
        """fp32 DEVICE scalar: the norm of (gradient * grad_scale) the last sam_perturb() saw (adaptive: of |w| * gradient * grad_scale).
        A view of the 16-byte SAM block: `.item()` is the caller's synchronisation.  Only with `sam_rho`."""
        self._need(self.sam_rho is not None, "last_sam_norm", "sam_rho")
        return self._sam_views["norm"]

    @property
    def last_sam_scale(self) -> torch.Tensor:
        """fp32 DEVICE scalar: rho / (norm + 1e-12) of the last sam_perturb(), formed in double and rounded once; 0 where the norm was
        not finite.  Only with `sam_rho`."""
        self._need(self.sam_rho is not None, "last_sam_scale", "sam_rho")
        return self._sam_views["scale"]

    @property
    def sam_nonfinite(self) -> torch.Tensor:
        """int32 DEVICE scalar: 1 where the last sam_perturb() found a norm that is Inf or NaN and left the weights as they were."""
        self._need(self.sam_rho is not None, "sam_nonfinite", "sam_rho")
        return self._sam_views["nonfinite"]

    def sam_perturb(self):
        """Moves every parameter the optimizer holds to w + e with the gradient the buckets hold now (class docstring, "Sharpness-aware
        minimization") and keeps w in the hold buffers: three launches on the current stream, no synchronisation.  The next step()
        updates w; sam_restore() gives w back without a step.  A second call before either raises RuntimeError."""
        self._need(self.sam_rho is not None, "sam_perturb()", "sam_rho")
        self._not_swapped("sam_perturb()")
        self._not_perturbed("sam_perturb()")
        scale = self.grad_scale * float(getattr(self.reducer, "grad_scale", 1.0))        # what step() hands its kernels
        stream = torch.cuda.current_stream(self._dev).cuda_stream
        capi.check(capi.lib().avmoe_opt_sam_perturb(self._table_ptr, len(self._recs), self._n_blocks, self._partials_ptr,
                                                    self._sam_block.data_ptr(), scale, self.sam_rho, int(self.sam_adaptive),
                                                    self._hold_ptrs.data_ptr(), stream), "avmoe_opt_sam_perturb")
        self._perturbed = True

    def sam_restore(self):
        """Abandons a perturbation: ONE launch on the current stream (avmoe_opt_swap_ema with the hold buffers) gives every parameter
        its unperturbed value back bit for bit.  Raises RuntimeError when the weights are not perturbed."""
        self._need(self.sam_rho is not None, "sam_restore()", "sam_rho")
        if not self._perturbed:
            raise RuntimeError("FlatAdam.sam_restore() without a perturbation: call sam_perturb() first")
        self._exchange(self._hold_ptrs)
        self._perturbed = False

    def _update(self, L, stream, n, scale, flags, shadows):
        """the update launch of a device step: avmoe_opt_adam_step_ema, or behind a sam_perturb() avmoe_opt_adam_step_sam, which reads
        the parameters from the hold buffers and so brings the unperturbed weights back; with `trust_ratio` avmoe_opt_lamb_step (three
        launches in place of one), with `prodigy` avmoe_opt_prodigy_step, with `muon` avmoe_opt_muon_step and with `schedule_free`
        avmoe_opt_sf_step (two each) serve both cases: they take the hold pointers only behind a sam_perturb()"""
        hold = self._hold_ptrs.data_ptr() if self._perturbed else None
        if self.muon:
            entry, tail = L.avmoe_opt_muon_step, (hold, self._muon_image.data_ptr(), len(self._muon_order), self._muon_work_ptrs.data_ptr(),
                                                  C.byref(self._muon_c), self._muon_ws.data_ptr(), self._muon_report.data_ptr())
            if self._muon_large_order:                   # only then: without a large matrix a step is avmoe_opt_muon_step's two launches
                entry = L.avmoe_opt_muon_step_large
                tail += (self._muon_large_image.data_ptr(), self._muon_large_host.data_ptr(), len(self._muon_large_order),
                         self._muon_large_ws.data_ptr(), self._muon_large_report.data_ptr())
        elif self.prodigy:
            entry, tail = L.avmoe_opt_prodigy_step, (hold, self._prodigy_x0_ptrs.data_ptr(), self._prodigy_s_ptrs.data_ptr(),
                                                     C.byref(self._prodigy_c), self._prodigy_block.data_ptr(), self._prodigy_ws.data_ptr())
        elif self.schedule_free:                         # x is required, whatever the flags: the shadows' place takes it
            entry, shadows, tail = L.avmoe_opt_sf_step, self._shadow_ptrs.data_ptr(), (hold, C.byref(self._sf_c), self._sf_block.data_ptr())
        elif self.trust_ratio:
            entry, tail = L.avmoe_opt_lamb_step, (hold, self._trust_limits.data_ptr(), self._trust_ws.data_ptr(), self._trust_report.data_ptr())
        elif self._perturbed:
            entry, tail = L.avmoe_opt_adam_step_sam, (hold,)
        else:
            entry, tail = L.avmoe_opt_adam_step_ema, ()
        capi.check(entry(self._table_ptr, n, self._n_blocks, self._state_ptr, self.betas[0], self.betas[1], self.eps, scale, flags, stream,
                         shadows, *tail), entry.__name__)
        self._perturbed = False

    # ---- layer-wise trust ratios ----------------------------------------------------------------------------------
    @staticmethod
    def _check_trust(on, clip):
        """-> (trust_ratio, trust_clip as the fp32 value the device gets or None)"""
        if not isinstance(on, bool):
            raise ValueError(f"trust_ratio must be True or False, not {on!r}")
        if clip is None:
            return on, None
        if not on:
            raise ValueError("trust_clip needs trust_ratio: there is no ratio to clamp")
        c = float(clip)
        if not (c > 0.0) or math.isinf(c) or c > 3.4028234663852886e38 or _f32(c) == 0.0:
            raise ValueError(f"trust_clip must be a finite number > 0 (as fp32), not {clip!r}")
        return on, _f32(c)

    @staticmethod
    def trust_ratio_of(w_norm: float, u_norm: float, clip: Optional[float] = None) -> float:
        """The host's copy of the rule kk_opt_lamb_ratio applies to an adapted parameter: ||w|| / ||u|| formed in double and rounded once
        to fp32; 1 where either norm is 0 or not finite; min(ratio, fp32(clip)) with a clamp."""
        w, u = float(w_norm), float(u_norm)
        if not (w > 0.0 and u > 0.0 and math.isfinite(w) and math.isfinite(u)):
            return 1.0
        q = w / u
        if clip is not None and q > _f32(float(clip)):
            q = _f32(float(clip))
        return float(torch.tensor(q, dtype=torch.float64).to(torch.float32))

    def _trust_limit_values(self):
        """one float per parameter as avmoe_opt_lamb_step reads it: < 0 not adapted, 0 adapted, > 0 adapted and clamped to it"""
        return [(-1.0 if not a else (0.0 if self.trust_clip is None else self.trust_clip)) for a in self.adapted]

    def _save_trust(self, extra):
        extra.update(trust_ratio=True, trust_clip=self.trust_clip)               # constants only: norms and ratios are rewritten by every step

    def _check_saved_trust(self, extra):
        """load_state_dict(): -> the saved (True, trust_clip), or None where the constructor's clamp stays"""
        if self.trust_ratio and extra.get("trust_ratio") is True:
            return self._check_trust(True, extra.get("trust_clip"))
        return None

    def _apply_saved_trust(self, consts):
        if consts is not None:
            self.trust_clip = consts[1]
            self._trust_limits.copy_(torch.tensor(self._trust_limit_values(), dtype=torch.float32))

    def _build_trust(self):
        """the limits, the workspace of two doubles per table block and the report (header, then w_norm, u_norm, ratio) with its views"""
        L, n = self._lib_with("avmoe_opt_lamb_step", "the layer-wise trust ratios"), len(self._recs)
        lay = cm.OptLambLayout()
        if L.avmoe_opt_lamb_bytes(n, self._n_blocks, C.byref(lay)) == 0:
            capi.check(-1, "avmoe_opt_lamb_bytes")
        self._trust_limits = torch.tensor(self._trust_limit_values(), dtype=torch.float32).to(self._dev)
        self._trust_ws = torch.zeros(int(lay.workspace_bytes), dtype=torch.uint8, device=self._dev)
        self._trust_report = torch.zeros(int(lay.report_bytes), dtype=torch.uint8, device=self._dev)
        hdr = C.sizeof(cm.OptLambHeader)
        w, u, r = (self._trust_report[hdr + 4 * n * k:hdr + 4 * n * (k + 1)].view(torch.float32) for k in range(3))
        r.fill_(1.0)                                     # until the first step: every ratio 1
        self._trust_views = {"w_norm": w, "u_norm": u, "ratio": r}

    @property
    def adapted(self) -> List[bool]:
        """host state, in `params` order: whether the parameter's step takes its trust ratio (the others take exactly 1)"""
        return [r.adapted for r in self._recs]

    @property
    def last_trust_ratios(self) -> torch.Tensor:
        """fp32 DEVICE tensor of len(params), in `params` order: the trust ratio of every parameter at the last applied step() -- exactly 1
        for a parameter that is not adapted or whose weights or update had norm 0.  A view of the trust report, rewritten by every
        applied step and by every replay of a captured one (a skipped step leaves it): reading it is the caller's synchronisation.  Only with `trust_ratio`."""
        self._need(self.trust_ratio, "last_trust_ratios", "trust_ratio")
        return self._trust_views["ratio"]

    @property
    def last_param_norms(self) -> torch.Tensor:
        """fp32 DEVICE tensor of len(params): ||w|| of every parameter BEFORE the last applied step(), summed in double.  As `last_trust_ratios`."""
        self._need(self.trust_ratio, "last_param_norms", "trust_ratio")
        return self._trust_views["w_norm"]

    @property
    def last_update_norms(self) -> torch.Tensor:
        """fp32 DEVICE tensor of len(params): ||u|| of every parameter's update direction at the last applied step() (decoupled: the decay
        term included), summed in double.  As `last_trust_ratios`."""
        self._need(self.trust_ratio, "last_update_norms", "trust_ratio")
        return self._trust_views["u_norm"]

    # ---- Prodigy learning-rate estimation ---------------------------------------------------------------------------
    @staticmethod
    def _check_prodigy(on, d0, d_coef, growth, safeguard):
        """-> (prodigy, d0, d_coef, growth or None, safeguard_warmup) with the numbers as the fp32 values the device gets"""
        if not isinstance(on, bool):
            raise ValueError(f"prodigy must be True or False, not {on!r}")
        if not isinstance(safeguard, bool):
            raise ValueError(f"prodigy_safeguard_warmup must be True or False, not {safeguard!r}")
        big = 3.4028234663852886e38
        a, c = float(d0), float(d_coef)
        if not (a > 0.0) or a > big or _f32(a) == 0.0:
            raise ValueError(f"prodigy_d0 must be a finite number > 0 (as fp32), not {d0!r}")
        if not (c > 0.0) or c > big or _f32(c) == 0.0:
            raise ValueError(f"prodigy_d_coef must be a finite number > 0 (as fp32), not {d_coef!r}")
        g = None
        if growth is not None:
            g = float(growth)
            if not (g >= 1.0) or g > big:
                raise ValueError(f"prodigy_growth must be a finite number >= 1 or None, not {growth!r}")
            g = _f32(g)
        if not on and (_f32(a) != _f32(1e-6) or c != 1.0 or g is not None or safeguard):
            raise ValueError("prodigy_d0 / prodigy_d_coef / prodigy_growth / prodigy_safeguard_warmup need prodigy: there is no estimate to shape")
        return on, _f32(a), _f32(c), g, safeguard

    @staticmethod
    def prodigy_d_next(d: float, d_max: float, d_hat: float, num: float, sum_dot: float, sum_abs: float, beta2: float,
                       d_coef: float = 1.0, growth: Optional[float] = None) -> dict:
        """The host's copy of the rule kk_opt_prodigy_finalize applies after an applied step: from the block's words before the step
        (d, d_max, d_hat as fp32 values, num) and the step's two sums -> {"d", "d_max", "d_hat", "num", "den"} as the block holds them
        after it.  num = beta3 num + sum_dot and den = sum_abs in double with beta3 = fp32(sqrt(beta2)); d_hat = fp32(d_coef num / den),
        left where den is not > 0 or a term is not a finite fp32; d_max = max(d_max, d_hat); d = min(d_max, fp32(d * growth)),
        without `growth` d_max."""
        beta3 = _f32(math.sqrt(float(beta2)))
        num1, den = beta3 * float(num) + float(sum_dot), float(sum_abs)
        if den > 0.0 and math.isfinite(num1) and math.isfinite(den):
            q = _f32(float(d_coef)) * num1 / den
            if abs(q) <= 3.4028234663852886e38:
                d_hat = _f32(q)
        d_max = max(float(d_max), float(d_hat))
        d1 = d_max if growth is None else min(d_max, _f32(float(d) * _f32(float(growth))))
        return {"d": d1, "d_max": d_max, "d_hat": float(d_hat), "num": num1, "den": den}

    def _build_prodigy(self):
        """the device arrays of one x0 and one s pointer per range, beside the shadows', the 32-byte block (d = d_max = d0), the
        workspace of two doubles per table block and the constants step() hands over"""
        L = self._lib_with("avmoe_opt_prodigy_step", "Prodigy learning-rate estimation")
        lay = cm.OptProdigyLayout()
        if L.avmoe_opt_prodigy_bytes(self._n_blocks, C.byref(lay)) == 0:
            capi.check(-1, "avmoe_opt_prodigy_bytes")
        self._prodigy_x0_views, self._prodigy_x0_ptrs = self._side_views("x0", "an x0 / s")
        self._prodigy_s_views, self._prodigy_s_ptrs = self._side_views("s", "an x0 / s")
        self._prodigy_ws = torch.zeros(int(lay.workspace_bytes), dtype=torch.uint8, device=self._dev)
        self._prodigy_block = torch.zeros(int(lay.block_bytes), dtype=torch.uint8, device=self._dev)
        self._prodigy_views = {k: self._prodigy_block[o:o + (8 if dt == "float64" else 4)].view(getattr(torch, dt))[0]
                               for k, (o, dt) in cm.OPT_PRODIGY_FIELDS.items()}
        self._set_prodigy(self.prodigy_d0, self.prodigy_d_coef, self.prodigy_growth, self.prodigy_safeguard_warmup)
        self._seed_prodigy()

    def _set_prodigy(self, d0, d_coef, growth, safeguard):
        self.prodigy_d0, self.prodigy_d_coef, self.prodigy_growth, self.prodigy_safeguard_warmup = d0, d_coef, growth, safeguard
        self._prodigy_c = cm.OptProdigy(d0=d0, d_coef=d_coef, growth=0.0 if growth is None else growth, safeguard_warmup=int(safeguard))

    def _save_prodigy(self, extra):
        """state_dict(): the constants, the block and the two per-element buffers"""
        blk = {k: v.item() for k, v in self._prodigy_views.items()}
        extra.update(prodigy=True, prodigy_d0=self.prodigy_d0, prodigy_d_coef=self.prodigy_d_coef, prodigy_growth=self.prodigy_growth,
                     prodigy_safeguard_warmup=self.prodigy_safeguard_warmup, prodigy_d=blk["d"], prodigy_d_max=blk["d_max"],
                     prodigy_d_hat=blk["d_hat"], prodigy_num=blk["num"], prodigy_den=blk["den"],
                     prodigy_x0=[x.detach().cpu().clone() for x in self._prodigy_x0_views],
                     prodigy_s=[x.detach().cpu().clone() for x in self._prodigy_s_views])

    def _check_saved_prodigy(self, extra):
        """load_state_dict(): -> (constants, {"prodigy_x0": tensors, "prodigy_s": tensors}, the block's words), or None where the
        estimate is re-seeded"""
        if extra.get("prodigy") is True and not self.prodigy:
            raise ValueError("the state dict was saved with prodigy (its rates are multipliers of the estimate d), which this optimizer "
                             "was built without: build it with prodigy=True")
        if not (self.prodigy and extra.get("prodigy") is True):
            return None
        consts = self._check_prodigy(True, extra.get("prodigy_d0", self.prodigy_d0), extra.get("prodigy_d_coef", self.prodigy_d_coef),
                                     extra.get("prodigy_growth"), extra.get("prodigy_safeguard_warmup", False))[1:]
        lists = {}
        for key in ("prodigy_x0", "prodigy_s"):
            lst = extra.get(key)
            if lst is None or len(lst) != len(self._recs):
                raise ValueError(f"state dict has {0 if lst is None else len(lst)} tensors under {key!r}, this optimizer {len(self._recs)} parameters")
            for i, (x, r) in enumerate(zip(lst, self._recs)):
                if tuple(x.shape) != tuple(r.p.shape):
                    raise ValueError(f"parameter index {i}: {key} has shape {tuple(x.shape)}, the parameter {tuple(r.p.shape)}")
            lists[key] = lst
        d, d_max = float(extra["prodigy_d"]), float(extra.get("prodigy_d_max", extra["prodigy_d"]))
        if not (d > 0.0 and d_max >= d and math.isfinite(d_max)):
            raise ValueError(f"the state dict's prodigy_d / prodigy_d_max must be finite with 0 < d <= d_max, not {d!r} / {d_max!r}")
        return consts, lists, {"d": d, "d_max": d_max, "d_hat": float(extra.get("prodigy_d_hat", 0.0)),
                               "num": float(extra.get("prodigy_num", 0.0)), "den": float(extra.get("prodigy_den", 0.0))}

    def _apply_saved_prodigy(self, payload):
        if payload is None:                              # nothing saved: the run starts here, from the parameters as they are now
            return self._seed_prodigy()
        consts, lists, blk = payload
        self._set_prodigy(*consts)
        for views, key in ((self._prodigy_x0_views, "prodigy_x0"), (self._prodigy_s_views, "prodigy_s")):
            for view, x in zip(views, lists[key]):
                view.copy_(x.to(torch.float32))
        for k, val in blk.items():
            self._prodigy_views[k].fill_(val)

    def _seed_prodigy(self):
        """the start of a run: x0 = the parameters as they are now, s = 0, the block {d0, d0, 0, 0, 0.0, 0.0}"""
        for s in self.state:
            s["x0"].copy_(s["p"])
            s["s"].zero_()
        self._prodigy_block.zero_()
        self._prodigy_views["d"].fill_(self.prodigy_d0)
        self._prodigy_views["d_max"].fill_(self.prodigy_d0)

    @property
    def prodigy_d(self) -> torch.Tensor:
        """fp32 DEVICE scalar: the estimate d the NEXT applied step uses (d0 until the first one).  A view of the 32-byte Prodigy block,
        rewritten by every applied step and by every replay of a captured one (a skipped step leaves it): `.item()` is the caller's
        synchronisation.  Only with `prodigy`."""
        self._need(self.prodigy, "prodigy_d", "prodigy")
        return self._prodigy_views["d"]

    @property
    def prodigy_d_hat(self) -> torch.Tensor:
        """fp32 DEVICE scalar: d_coef * num / den of the last applied step, which may lie below d or be negative.  As `prodigy_d`."""
        self._need(self.prodigy, "prodigy_d_hat", "prodigy")
        return self._prodigy_views["d_hat"]

    @property
    def prodigy_block(self) -> Dict[str, torch.Tensor]:
        """every word of the Prodigy block as DEVICE scalars: d, d_max, d_hat (fp32), num, den (fp64).  As `prodigy_d`."""
        self._need(self.prodigy, "prodigy_block", "prodigy")
        return dict(self._prodigy_views)

    @property
    def prodigy_x0(self) -> List[torch.Tensor]:
        """DEVICE views in `params` order: the parameters as they were when the optimizer was built or its state loaded"""
        self._need(self.prodigy, "prodigy_x0", "prodigy")
        return list(self._prodigy_x0_views)

    @property
    def prodigy_s(self) -> List[torch.Tensor]:
        """DEVICE views in `params` order: the running gradient sum s of every parameter"""
        self._need(self.prodigy, "prodigy_s", "prodigy")
        return list(self._prodigy_s_views)

    # ---- schedule-free AdamW --------------------------------------------------------------------------------------
    @staticmethod
    def _check_sf(on, r, lr_power):
        """-> (schedule_free, sf_r, sf_lr_power) with the numbers as the fp32 values the device gets"""
        if not isinstance(on, bool):
            raise ValueError(f"schedule_free must be True or False, not {on!r}")
        out = []
        for name, v in (("sf_r", r), ("sf_lr_power", lr_power)):
            if isinstance(v, bool) or not isinstance(v, (int, float)):
                raise ValueError(f"{name} (schedule_free) must be a finite number >= 0, not {v!r}")
            x = float(v)
            if not (x >= 0.0) or x > 3.4028234663852886e38:
                raise ValueError(f"{name} (schedule_free) must be a finite number >= 0 (as fp32), not {v!r}")
            out.append(_f32(x))
        if not on and (out[0] != 0.0 or out[1] != 2.0):
            raise ValueError("sf_r / sf_lr_power need schedule_free: there is no average to weight")
        return on, out[0], out[1]

    @staticmethod
    def sf_weights_next(weight_sum: float, f_max: float, n: int, f: float, r: float = 0.0, lr_power: float = 2.0) -> tuple:
        """The host's copy of the rule kk_opt_sf_weights applies on an applied step, in its operation order: from the block's words before
        the step (weight_sum, f_max as an fp32 value), n = applied_steps after the step (the first has n = 1) and the step's schedule
        factor f (1 without a schedule) -> (weight_sum, f_max, c, d) as the block holds them after it.  In double from the fp32
        constants: f_max = max(f_max, f); w = n^r * f_max^lr_power (pow(., 0) = 1); weight_sum += w; c = w / weight_sum, 0 where
        weight_sum is not > 0; d = 1 - c; c and d each rounded once to fp32."""
        f, f_max = _f32(float(f)), _f32(float(f_max))
        f_max = f if f > f_max else f_max
        w = math.pow(float(int(n)), _f32(float(r))) * math.pow(f_max, _f32(float(lr_power)))
        total = float(weight_sum) + w
        c = w / total if total > 0.0 else 0.0
        return total, f_max, _f32(c), _f32(1.0 - c)

    def _seed_sf(self):
        """the start of a run: z (exp_avg) = x (the shadow) = the parameters as they are now (padding zero)"""
        for s in self.state:
            s["m"].copy_(s["p"])
            s["e"].copy_(s["p"])

    def _build_sf(self):
        """the 32-byte block on the device (all zero), its views, the views of z and the constants step() hands over"""
        self._lib_with("avmoe_opt_sf_step", "schedule-free AdamW")
        self._sf_block = torch.zeros(C.sizeof(cm.OptSfState), dtype=torch.uint8, device=self._dev)
        self._sf_views = {k: self._sf_block[o:o + (8 if dt == "float64" else 4)].view(getattr(torch, dt))[0]
                          for k, (o, dt) in cm.OPT_SF_FIELDS.items()}
        self._sf_z_views = [r.view("m") for r in self._recs]
        self._set_sf(self.sf_r, self.sf_lr_power)

    def _set_sf(self, r, lr_power):
        self.sf_r, self.sf_lr_power = r, lr_power
        self._sf_c = cm.OptSf(r=r, lr_power=lr_power)

    def _save_sf(self, extra):
        """state_dict(): the constants and the block (z is "exp_avg", x the "ema" list _save_average writes)"""
        blk = {k: v.item() for k, v in self._sf_views.items()}
        extra.update(schedule_free=True, sf_r=self.sf_r, sf_lr_power=self.sf_lr_power, sf_weight_sum=blk["weight_sum"],
                     sf_lr_max=blk["f_max"], sf_c=blk["c"], sf_d=blk["d"])

    def _check_saved_sf(self, extra):
        """load_state_dict(): -> (constants, the block's words), or None where z, x and the block are re-seeded"""
        if extra.get("schedule_free") is True and not self.schedule_free:
            raise ValueError("the state dict was saved with schedule_free (its exp_avg is the base sequence z, not a momentum), which this "
                             "optimizer was built without: build it with schedule_free=True")
        if not (self.schedule_free and extra.get("schedule_free") is True):
            return None
        if extra.get("ema") is None:
            raise ValueError("the state dict was saved with schedule_free but carries no average (\"ema\")")
        consts = self._check_sf(True, extra.get("sf_r", self.sf_r), extra.get("sf_lr_power", self.sf_lr_power))[1:]
        ws, fm, c = float(extra.get("sf_weight_sum", 0.0)), float(extra.get("sf_lr_max", 0.0)), float(extra.get("sf_c", 0.0))
        if not (math.isfinite(ws) and ws >= 0.0 and math.isfinite(fm) and fm >= 0.0 and 0.0 <= c <= 1.0):
            raise ValueError(f"the state dict's sf_weight_sum / sf_lr_max / sf_c must be finite and >= 0 with sf_c <= 1, not {ws!r} / {fm!r} / {c!r}")
        d = float(extra.get("sf_d", _f32(1.0 - c) if ws > 0.0 else 0.0))      # informative: every applied step writes d before it reads it
        if not (0.0 <= d <= 1.0):
            raise ValueError(f"the state dict's sf_d must be in [0, 1], not {d!r}")
        return consts, {"weight_sum": ws, "f_max": fm, "c": c, "d": d}

    def _apply_saved_sf(self, payload):
        self._sf_block.zero_()
        if payload is None:                              # nothing saved: the run starts here, from the parameters as they are now
            self._views["ema_decay"].fill_(0.0)
            return self._seed_sf()
        consts, blk = payload
        self._set_sf(*consts)
        for k, val in blk.items():
            self._sf_views[k].fill_(val)
        self._views["ema_decay"].fill_(blk["d"])

    @property
    def sf_c(self) -> torch.Tensor:
        """fp32 DEVICE scalar: the weight c = w / weight_sum the last applied step's z entered the average x with (1 at the first one;
        `last_ema_decay` is d = 1 - c).  A view of the 32-byte schedule-free block, rewritten by every applied step and by every replay
        of a captured one (a skipped step leaves it): `.item()` is the caller's synchronisation.  Only with `schedule_free`."""
        self._need(self.schedule_free, "sf_c", "schedule_free")
        return self._sf_views["c"]

    @property
    def sf_weight_sum(self) -> torch.Tensor:
        """fp64 DEVICE scalar: the sum of the steps' averaging weights so far.  As `sf_c`."""
        self._need(self.schedule_free, "sf_weight_sum", "schedule_free")
        return self._sf_views["weight_sum"]

    @property
    def sf_lr_max(self) -> torch.Tensor:
        """fp32 DEVICE scalar: the largest schedule factor an applied step has seen (1 without a schedule).  As `sf_c`."""
        self._need(self.schedule_free, "sf_lr_max", "schedule_free")
        return self._sf_views["f_max"]

    @property
    def sf_block(self) -> Dict[str, torch.Tensor]:
        """every word of the schedule-free block as DEVICE scalars: weight_sum (fp64), f_max, c, d (fp32).  As `sf_c`."""
        self._need(self.schedule_free, "sf_block", "schedule_free")
        return dict(self._sf_views)

    @property
    def sf_z(self) -> List[torch.Tensor]:
        """DEVICE views in `params` order: the base sequence z of every parameter (it lives in exp_avg)"""
        self._need(self.schedule_free, "sf_z", "schedule_free")
        return list(self._sf_z_views)

    # ---- orthogonalised momentum (Muon) ---------------------------------------------------------------------------
    MUON_MAX_DIM = 128                                   # AVMOE_MUON_MAX_DIM: the short side one workgroup's LDS holds the Gram matrix of
    MUON_LARGE_MAX_DIM = 2048                            # AVMOE_MUON_LARGE_MAX_DIM: the short side the engine path takes (muon_large)
    MUON_SCALES = ("match_rms_adamw", "original")        # AVMOE_MUON_SCALE_*

    @staticmethod
    def _check_muon(on, momentum, nesterov, ns_steps, scale, max_numel):
        """-> (muon, momentum as the fp32 value the device gets, nesterov, ns_steps, scale, max_numel)"""
        if not isinstance(on, bool):
            raise ValueError(f"muon must be True or False, not {on!r}")
        if not isinstance(nesterov, bool):
            raise ValueError(f"muon_nesterov must be True or False, not {nesterov!r}")
        mu = float(momentum)
        if not (0.0 <= mu < 1.0) or _f32(mu) >= 1.0:
            raise ValueError(f"muon_momentum must be in [0, 1) (as fp32), not {momentum!r}")
        if isinstance(ns_steps, bool) or not isinstance(ns_steps, int) or not (1 <= ns_steps <= 16):
            raise ValueError(f"muon_ns_steps must be an integer in 1..16, not {ns_steps!r}")
        if scale not in FlatAdam.MUON_SCALES:
            raise ValueError(f"muon_scale must be one of {FlatAdam.MUON_SCALES}, not {scale!r}")
        if isinstance(max_numel, bool) or not isinstance(max_numel, int) or max_numel < 1:
            raise ValueError(f"muon_max_numel must be an integer >= 1, not {max_numel!r}")
        if not on and (_f32(mu) != _f32(0.95) or nesterov is not True or ns_steps != 5 or scale != "match_rms_adamw" or max_numel != 262144):
            raise ValueError("muon_momentum / muon_nesterov / muon_ns_steps / muon_scale / muon_max_numel need muon: there is no matrix to orthogonalise")
        return on, _f32(mu), nesterov, ns_steps, scale, max_numel

    @staticmethod
    def muon_shape_of(p, max_numel: int = 262144):
        """(rows, cols) as which a parameter is orthogonalised -- rows = shape[0], cols = numel // rows, a conv weight flattened as
        torch.optim.Muon's users do -- or None where it does not fit: dim() < 2, no elements, min(rows, cols) > 128 or numel > max_numel."""
        if p.dim() < 2 or p.numel() == 0:
            return None
        rows = int(p.shape[0])
        cols = p.numel() // rows
        if min(rows, cols) > FlatAdam.MUON_MAX_DIM or p.numel() > max_numel:
            return None
        return rows, cols

    @staticmethod
    def muon_select(params, param_groups=None, muon_max_numel: int = 262144) -> list:
        """The selection rule of `muon=True`, in `params` order: (rows, cols) for a parameter that is orthogonalised, None for one that
        takes Adam / AdamW.  Default: `muon_shape_of`; a group's "muon": False switches its parameters off, True insists -- ValueError
        naming the parameter where it does not fit, and for a "muon" that is not a bool."""
        override = {}
        for gi, grp in enumerate(param_groups or []):
            if "muon" not in grp:
                continue
            if not isinstance(grp["muon"], bool):
                raise ValueError(f"a parameter group's \"muon\" must be True or False, not {grp['muon']!r}")
            ps = grp["params"]
            for k, p in enumerate([ps] if isinstance(ps, torch.Tensor) else ps):
                if grp["muon"] and FlatAdam.muon_shape_of(p, muon_max_numel) is None:
                    raise ValueError(f"parameter group {gi} asks for muon on its parameter {k} of shape {tuple(p.shape)}, which does not fit: it "
                                     f"needs dim() >= 2, a short side <= {FlatAdam.MUON_MAX_DIM} and numel <= muon_max_numel = {muon_max_numel}")
                override[id(p)] = grp["muon"]
        return [FlatAdam.muon_shape_of(p, muon_max_numel) if override.get(id(p), True) else None for p in params]

    @staticmethod
    def _check_muon_large(on, max_numel, muon):
        """-> (muon_large, muon_large_max_numel)"""
        if not isinstance(on, bool):
            raise ValueError(f"muon_large must be True or False, not {on!r}")
        if isinstance(max_numel, bool) or not isinstance(max_numel, int) or max_numel < 1:
            raise ValueError(f"muon_large_max_numel must be an integer >= 1, not {max_numel!r}")
        if on and not muon:
            raise ValueError("muon_large needs muon: it widens muon's selection to the large matrices")
        if not on and max_numel != 1 << 23:
            raise ValueError("muon_large_max_numel needs muon_large: there is no large matrix to orthogonalise")
        return on, max_numel

    @staticmethod
    def muon_large_shape_of(p, max_numel: int = 1 << 23):
        """(rows, cols) as which the engine path of `muon_large` orthogonalises a parameter -- rows = shape[0], cols = numel // rows -- or
        None where it does not fit: dim() < 2, no elements, min(rows, cols) > 2048 or numel > max_numel.  The rule of the large path
        alone: `muon_select_paths` asks the small rule first."""
        if p.dim() < 2 or p.numel() == 0:
            return None
        rows = int(p.shape[0])
        cols = p.numel() // rows
        if min(rows, cols) > FlatAdam.MUON_LARGE_MAX_DIM or p.numel() > max_numel:
            return None
        return rows, cols

    @staticmethod
    def muon_select_paths(params, param_groups=None, muon_max_numel: int = 262144, muon_large: bool = False,
                          muon_large_max_numel: int = 1 << 23) -> list:
        """The selection of `muon=True, muon_large=...`, in `params` order: ("small", (rows, cols)) for a parameter the one-workgroup
        kernel orthogonalises, ("large", (rows, cols)) for one the engine path does, None for one that takes Adam / AdamW.  The small
        rule (`muon_shape_of`) comes first and keeps what it takes; with `muon_large` a parameter it declines -- for its short side or
        for its numel -- goes to the large path where `muon_large_shape_of` fits.  A group's "muon": False switches its parameters
        off, True insists: ValueError naming the parameter where neither rule fits.  Without `muon_large` this is `muon_select`."""
        if not muon_large:
            return [None if s is None else ("small", s) for s in FlatAdam.muon_select(params, param_groups, muon_max_numel)]

        def path_of(p):
            s = FlatAdam.muon_shape_of(p, muon_max_numel)
            if s is not None:
                return "small", s
            s = FlatAdam.muon_large_shape_of(p, muon_large_max_numel)
            return None if s is None else ("large", s)
        override = {}
        for gi, grp in enumerate(param_groups or []):
            if "muon" not in grp:
                continue
            if not isinstance(grp["muon"], bool):
                raise ValueError(f"a parameter group's \"muon\" must be True or False, not {grp['muon']!r}")
            ps = grp["params"]
            for k, p in enumerate([ps] if isinstance(ps, torch.Tensor) else ps):
                if grp["muon"] and path_of(p) is None:
                    raise ValueError(f"parameter group {gi} asks for muon on its parameter {k} of shape {tuple(p.shape)}, which does not fit: it "
                                     f"needs dim() >= 2, a short side <= {FlatAdam.MUON_LARGE_MAX_DIM} and numel <= muon_large_max_numel = "
                                     f"{muon_large_max_numel}")
                override[id(p)] = grp["muon"]
        return [path_of(p) if override.get(id(p), True) else None for p in params]

    def _muon_paths_of(self, params, param_groups):
        return self.muon_select_paths(params, param_groups, self.muon_max_numel, self.muon_large, self.muon_large_max_numel)

    @staticmethod
    def muon_scale_of(rows: int, cols: int, scale: str = "match_rms_adamw") -> float:
        """the factor s on an orthogonalised parameter's rate, as the fp32 value kk_opt_muon_ns forms: 0.2 sqrt(max(rows, cols))
        ("match_rms_adamw": an Adam learning rate keeps its meaning) or sqrt(max(1, rows / cols)) ("original")"""
        if scale == "original":
            return _f32(math.sqrt(max(1.0, rows / cols)))
        return _f32(0.2 * math.sqrt(float(max(rows, cols))))

    def _set_muon(self, momentum, nesterov, ns_steps, scale):
        self.muon_momentum, self.muon_nesterov, self.muon_ns_steps, self.muon_scale = momentum, nesterov, ns_steps, scale
        self._muon_c = cm.OptMuon(momentum=momentum, nesterov=int(nesterov), ns_steps=ns_steps, scale=self.MUON_SCALES.index(scale))

    def _save_muon(self, extra):
        """state_dict(): constants only -- exp_avg IS the momentum, O and the norms are rewritten by every step"""
        extra.update(muon=True, muon_momentum=self.muon_momentum, muon_nesterov=self.muon_nesterov, muon_ns_steps=self.muon_ns_steps,
                     muon_scale=self.muon_scale, muon_max_numel=self.muon_max_numel)
        if self.muon_large:
            extra.update(muon_large=True, muon_large_max_numel=self.muon_large_max_numel)

    def _check_saved_muon(self, extra):
        """load_state_dict(): -> the saved (momentum, nesterov, ns_steps, scale), or None where the constructor's stay"""
        if extra.get("muon") is True and not self.muon:
            raise ValueError("the state dict was saved with muon (exp_avg of its matrices is a momentum with no second moment beside it), which "
                             "this optimizer was built without: build it with muon=True")
        if extra.get("muon_large") is True and not self.muon_large:
            raise ValueError("the state dict was saved with muon_large (exp_avg of its large matrices is a momentum with no second moment beside "
                             "it), which this optimizer was built without: build it with muon=True, muon_large=True")
        if not (self.muon and extra.get("muon") is True):
            return None
        return self._check_muon(True, extra.get("muon_momentum", self.muon_momentum), extra.get("muon_nesterov", self.muon_nesterov),
                                extra.get("muon_ns_steps", self.muon_ns_steps), extra.get("muon_scale", self.muon_scale),
                                self.muon_max_numel)[1:5]

    def _apply_saved_muon(self, consts):
        if consts is not None:
            self._set_muon(*consts)

    def _build_muon(self):
        """the matrix list (longest first, so that the long ones start first), its image on the device, one work pointer per range,
        the workspace of one double per table block and the report (header, then ||u||_F per matrix)"""
        L, n = self._lib_with("avmoe_opt_muon_step", "orthogonalised momentum"), len(self._recs)
        order = [i for i, r in enumerate(self._recs) if r.muon_path == "small"]
        order.sort(key=lambda i: -self._recs[i].p.numel())            # (stable: equal sizes keep the parameters' order)
        self._muon_order = order
        mats = (cm.OptMuonMat * max(1, len(order)))()
        for m, i in zip(mats, order):
            m.range, (m.rows, m.cols) = i, self._recs[i].muon_shape
        lay = cm.OptMuonLayout()
        if L.avmoe_opt_muon_bytes(n, self._n_blocks, len(order), C.byref(lay)) == 0:
            capi.check(-1, "avmoe_opt_muon_bytes")
        img = torch.zeros(int(lay.table_bytes), dtype=torch.uint8)
        capi.check(L.avmoe_opt_muon_table_build(self._opt_ranges(), n, mats, len(order), img.data_ptr(), int(lay.table_bytes)),
                   "avmoe_opt_muon_table_build")
        self._muon_image = img.to(self._dev)
        views, self._muon_work_ptrs = self._side_views("o", "a work")
        self._muon_views = [None if r.muon_shape is None else v for r, v in zip(self._recs, views)]
        self._muon_ws = torch.zeros(int(lay.workspace_bytes), dtype=torch.uint8, device=self._dev)
        self._muon_report = torch.zeros(int(lay.report_bytes), dtype=torch.uint8, device=self._dev)
        self._muon_norms = self._muon_report[16:16 + 4 * len(order)].view(torch.float32)       # in the list's order
        self._muon_index = torch.tensor(order, dtype=torch.int64).to(self._dev)
        self._set_muon(self.muon_momentum, self.muon_nesterov, self.muon_ns_steps, self.muon_scale)
        self._muon_large_order = []
        if self.muon_large:
            self._build_muon_large(mats, len(order))

    def _build_muon_large(self, small, n_small):
        """the large matrices (longest first), their image on the host and on the device (the step call shapes the engine's launches
        from the host copy), the staging workspace and the report (header, then ||u||_F per large matrix)"""
        L, n = self._lib_with("avmoe_opt_muon_step_large", "orthogonalised momentum for the large matrices"), len(self._recs)
        order = [i for i, r in enumerate(self._recs) if r.muon_path == "large"]
        order.sort(key=lambda i: -self._recs[i].p.numel())
        if not order:
            return
        mats = (cm.OptMuonMat * len(order))()
        for m, i in zip(mats, order):
            m.range, (m.rows, m.cols) = i, self._recs[i].muon_shape
        lay = cm.OptMuonLargeLayout()
        if L.avmoe_opt_muon_large_bytes(n, mats, len(order), C.byref(lay)) == 0:
            capi.check(-1, "avmoe_opt_muon_large_bytes")
        img = torch.zeros(int(lay.table_bytes), dtype=torch.uint8)
        capi.check(L.avmoe_opt_muon_large_table_build(self._opt_ranges(), n, mats, len(order), small, n_small, img.data_ptr(),
                                                      int(lay.table_bytes)), "avmoe_opt_muon_large_table_build")
        self._muon_large_host, self._muon_large_image = img, img.to(self._dev)
        self._muon_large_ws = torch.zeros(int(lay.workspace_bytes), dtype=torch.uint8, device=self._dev)
        self._muon_large_report = torch.zeros(int(lay.report_bytes), dtype=torch.uint8, device=self._dev)
        self._muon_large_norms = self._muon_large_report[16:16 + 4 * len(order)].view(torch.float32)
        self._muon_large_index = torch.tensor(order, dtype=torch.int64).to(self._dev)
        self._muon_large_classes = int(lay.n_classes)
        self._muon_large_order = order

    @property
    def muon_paths(self) -> list:
        """host state, in `params` order: "small" for a parameter the one-workgroup kernel orthogonalises, "large" for one the engine
        path does (`muon_large`), None for one that takes Adam / AdamW"""
        return [r.muon_path for r in self._recs]

    @property
    def orthogonalized(self) -> List[bool]:
        """host state, in `params` order: whether the parameter steps along its orthogonalised momentum (the others take Adam / AdamW)"""
        return [r.muon_shape is not None for r in self._recs]

    @property
    def muon_scales(self) -> List[float]:
        """host floats, in `params` order: the factor s on every orthogonalised parameter's rate (`muon_scale_of`); 0 for the others"""
        return [0.0 if r.muon_shape is None else self.muon_scale_of(*r.muon_shape, self.muon_scale) for r in self._recs]

    @property
    def last_muon_updates(self) -> list:
        """in `params` order: DEVICE views, shaped like the parameter, of the orthogonalised direction O the last applied step() moved
        it along (w = w - lr s O); None for a parameter that is not orthogonalised.  Views of the work buffers, rewritten by every
        applied step and every replay of a captured one (a skipped step leaves them).  Only with `muon`."""
        self._need(self.muon, "last_muon_updates", "muon")
        return list(self._muon_views)

    @property
    def last_muon_norms(self) -> torch.Tensor:
        """fp32 DEVICE tensor of len(params), in `params` order: ||u||_F of every orthogonalised parameter's direction before the
        iteration at the last applied step(), summed in double; 0 for the others.  Gathered from the report on the current stream at
        every call (no synchronisation).  Only with `muon`."""
        self._need(self.muon, "last_muon_norms", "muon")
        out = torch.zeros(len(self._recs), dtype=torch.float32, device=self._dev)
        if self._muon_order:
            out.index_copy_(0, self._muon_index, self._muon_norms)
        if self._muon_large_order:
            out.index_copy_(0, self._muon_large_index, self._muon_large_norms)
        return out

    # ---- the device path ------------------------------------------------------------------------------------------
    def _opt_ranges(self):
        """one avmoe_opt_range per parameter (its own elements only: the norm must not see alignment padding)"""
        arr = (cm.OptRange * len(self._recs))()
        for r, rec in zip(arr, self._recs):
            r.param, r.grad, r.exp_avg, r.exp_avg_sq = (rec.ptr(k) for k in ("p", "g", "m", "v"))
            r.n, r.lr, r.weight_decay = rec.p.numel(), rec.lr0 * self.decay, rec.wd
        return arr

    def _build_device_state(self):
        L = self._lib_with("avmoe_opt_swap_ema", "the device-side optimizer", "avmoe_opt_*")
        # step() makes its one norm call to the entry point that knows every flag: a library without it cannot run this device path at all
        self._lib_with("avmoe_opt_grad_norm_swa", "the norm entry point every device step calls")
        devs = {s["p"].device for s in self.state}
        if len(devs) != 1:
            raise capi.AvmoeError("FlatAdam's device path needs every bucket on one GPU")
        self._dev = devs.pop()
        lay = cm.OptLayout()
        total = L.avmoe_opt_workspace_bytes(self._opt_ranges(), len(self._recs), C.byref(lay))
        if total == 0:
            capi.check(-1, "avmoe_opt_workspace_bytes")
        self._n_blocks, self._table_bytes = int(lay.n_blocks), int(lay.table_bytes)
        self._ws = torch.zeros(total, dtype=torch.uint8, device=self._dev)          # [state block | table | partial sums]
        sb = int(lay.state_bytes)
        self._state_ptr, self._table_ptr = self._ws.data_ptr(), self._ws.data_ptr() + sb
        self._partials_ptr = self._table_ptr + self._table_bytes
        self._views = {k: self._ws[o:o + (8 if dt == "int64" else 4)].view(getattr(torch, dt))[0]
                       for k, (o, dt) in cm.OPT_STATE_FIELDS.items()}
        self._flags = (cm.OPT_CLIP if self.max_grad_norm is not None else 0) | (cm.OPT_SKIP_NONFINITE if self.skip_nonfinite else 0) \
            | (cm.OPT_DECOUPLED_DECAY if self.decoupled_weight_decay else 0)
        self._swa_c = cm.OptSwa()                        # both halves of avmoe_opt_swa; a half that is off is not read
        self._set_schedule(self.lr_schedule)
        self._upload_table()
        if self._averaging:
            self._build_shadows()
        if self._ebufs:
            self._build_buffer_table()
        if self.report_grad_norms:
            self._build_report()
        if self.sam_rho is not None:
            self._build_sam()
        if self.trust_ratio:
            self._build_trust()
        if self.prodigy:
            self._build_prodigy()
        if self.muon:
            self._build_muon()
        if self.schedule_free:
            self._build_sf()

    def _build_report(self):
        """the report buffer (header, then one float per parameter) and the two views the properties hand out"""
        L, n = self._lib_with("avmoe_opt_grad_norm_report", "the per-range gradient norms"), len(self._recs)
        nbytes = L.avmoe_opt_report_bytes(n)
        if nbytes == 0:
            capi.check(-1, "avmoe_opt_report_bytes")
        self._report = torch.zeros(nbytes, dtype=torch.uint8, device=self._dev)
        self._report[:4].view(torch.int32).fill_(-1)      # until the first step: no parameter
        hdr = C.sizeof(cm.OptReportHeader)
        self._report_views = (self._report[hdr:hdr + 4 * n].view(torch.float32), self._report[:4].view(torch.int32)[0])
        self._flags |= cm.OPT_REPORT

    def _build_shadows(self):
        """the views `ema_params` hands out and the device array of one shadow pointer per range, beside the range table"""
        self._ema_views, self._shadow_ptrs = self._side_views("e", "a shadow")
        if self.schedule_free:                           # no flag: the norm call writes no decay, avmoe_opt_sf_step does
            return
        if self.swa_start is not None:
            self._set_swa(self.swa_start, self.swa_freq)
        else:
            self._set_ema(self.ema_decay, self.ema_warmup)

    def _set_ema(self, decay, warmup):
        self.ema_decay, self.ema_warmup = decay, warmup
        self._ema_c = cm.OptEma(decay=decay, warmup=warmup)
        self._flags |= cm.OPT_EMA

    def _set_swa(self, start, freq):
        self.swa_start, self.swa_freq = start, freq
        self._swa_c.start, self._swa_c.freq = start, freq
        self._flags |= cm.OPT_SWA

    def _set_schedule(self, sched: Optional[LRSchedule]):
        """the schedule as the struct step() hands over, and its flag; with its SWA part the other half of avmoe_opt_swa and that flag"""
        self.lr_schedule = sched
        self._sched_c = None if sched is None else sched.c_struct()
        self._flags = (self._flags & ~(cm.OPT_LR_SCHEDULE | cm.OPT_SWA_LR)) | (cm.OPT_LR_SCHEDULE if sched is not None else 0)
        if sched is not None and sched.fill_swa(self._swa_c):
            self._flags |= cm.OPT_SWA_LR

    def _save_schedule(self, extra):
        extra["lr_schedule"] = dataclasses.asdict(self.lr_schedule)

    def _check_saved_schedule(self, extra):
        """load_state_dict(): -> the saved LRSchedule, or None where the constructor's stays"""
        saved = extra.get("lr_schedule")
        if saved is None:
            return None
        if not self._device:
            raise ValueError("the state dict carries a per-step lr_schedule, which needs FlatAdam's device path: build the optimizer "
                             "with lr_schedule (or max_grad_norm / decoupled_weight_decay / skip_nonfinite)")
        return saved if isinstance(saved, LRSchedule) else LRSchedule(**saved)

    def _apply_saved_schedule(self, sched):
        if sched is not None:
            self._set_schedule(sched)

    def _upload_table(self):
        """(re)build the range table with the learning rates of the current epoch and send it with ONE asynchronous copy"""
        img = torch.empty(self._table_bytes, dtype=torch.uint8, pin_memory=True)
        capi.check(capi.lib().avmoe_opt_table_build(self._opt_ranges(), len(self._recs), img.data_ptr(), self._table_bytes),
                   "avmoe_opt_table_build")
        sb = cm.OPT_STATE_BYTES
        self._ws[sb:sb + self._table_bytes].copy_(img, non_blocking=True)
        self._table_decay = self.decay

    def _state_view(self, name):
        if not self._device:
            raise capi.AvmoeError(f"FlatAdam.{name} lives in the device state block: set max_grad_norm, decoupled_weight_decay or "
                                  "skip_nonfinite")
        return self._views[name]

    @property
    def last_grad_norm(self) -> torch.Tensor:
        """fp32 DEVICE scalar: the global norm of (gradient * grad_scale) the last step() saw, before clipping (0 when neither clipping
        nor skipping is on).  A view of the state block: `.item()` is the caller's synchronisation."""
        return self._state_view("total_norm")

    @property
    def applied_steps(self) -> torch.Tensor:
        """int64 DEVICE scalar: steps that updated the parameters (what the bias correction counts); `self.t` counts step() calls."""
        return self._state_view("applied_steps")

    @property
    def skipped_steps(self) -> torch.Tensor:
        """int64 DEVICE scalar: steps held back because the gradient norm was not finite."""
        return self._state_view("skipped_steps")

    @property
    def last_lr_factor(self) -> torch.Tensor:
        """fp32 DEVICE scalar: the schedule's factor f(n) the last applied step used (a skipped step leaves it).  A view of the state
        block, like `last_grad_norm`; only with `lr_schedule`."""
        self._need(self.lr_schedule is not None, "last_lr_factor", "lr_schedule")
        return self._state_view("lr_factor")

    @property
    def last_param_grad_norms(self) -> torch.Tensor:
        """fp32 DEVICE tensor of len(params): the norm of (gradient * grad_scale) of every parameter at the last step(), before clipping,
        in `params` order (`param_names(model)` names them).  A view of the report buffer, rewritten by every step, a skipped one
        included: reading it is the caller's synchronisation.  Only with `report_grad_norms`."""
        self._need(self.report_grad_norms, "last_param_grad_norms", "report_grad_norms")
        return self._report_views[0]

    @property
    def first_nonfinite_param(self) -> torch.Tensor:
        """int32 DEVICE scalar: the lowest index into `params` of a parameter whose gradient norm at the last step() was Inf or NaN, -1 when
        all were finite.  A view of the report buffer, like `last_param_grad_norms`; only with `report_grad_norms`."""
        self._need(self.report_grad_norms, "first_nonfinite_param", "report_grad_norms")
        return self._report_views[1]

    def param_names(self, model: torch.nn.Module) -> List[Optional[str]]:
        """the names of `params`, in that order, from model.named_parameters() by identity; None for a parameter the model does not own"""
        names = {id(p): k for k, p in model.named_parameters()}
        return [names.get(id(r.p)) for r in self._recs]

    @property
    def state_block(self) -> Dict[str, torch.Tensor]:
        """every field of the device state block (avmoe_opt_state) as a DEVICE scalar view: total_norm, clip_coef, bc1, bc2_sqrt,
        applied_steps, skipped_steps, skip, lr_factor (written only with `lr_schedule`)"""
        self._state_view("total_norm")
        return dict(self._views)

    @property
    def params(self) -> List[torch.nn.Parameter]:
        """the parameters in the reducer's order -- the index order of state_dict()"""
        return [r.p for r in self._recs]

    @property
    def _plist(self) -> tuple:
        """for readers written before the records: (parameter, index into self.state, offset, lr0) per parameter, from `_recs`.  A TUPLE,
        and a property without a setter: the old way of setting a rate (`opt._plist[i] = ...`, `opt._plist = ...`) raises instead of
        writing into a copy -- set `_recs[i].lr0`"""
        return tuple((r.p, r.bucket, r.off, r.lr0) for r in self._recs)

    @property
    def _wds(self) -> tuple:
        """beside `_plist`, likewise a tuple: each parameter's weight decay (set `_recs[i].wd`)"""
        return tuple(r.wd for r in self._recs)

    def _keyed_groups(self):
        """[((lr0, weight_decay), [indices into self.params])]: one group per distinct pair, in order of first appearance"""
        out = {}
        for i, r in enumerate(self._recs):
            out.setdefault((r.lr0, r.wd), []).append(i)
        return list(out.items())

    def _groups(self):
        """[(lr0, [indices into self.params])] of the groups above; `_group_decays()` is the list of their weight decays"""
        return [(k[0], idx) for k, idx in self._keyed_groups()]

    def _group_decays(self):
        return [k[1] for k, _ in self._keyed_groups()]

    def torch_param_groups(self) -> List[dict]:
        """param groups for torch.optim.Adam / AdamW over the same parameters, in the grouping and order state_dict() uses, each with its
        learning rate of the current epoch and its weight decay"""
        ps = self.params
        return [{"params": [ps[i] for i in idx], "lr": lr0 * self.decay, "weight_decay": wd} for (lr0, wd), idx in self._keyed_groups()]

    @property
    def decay(self) -> float:
        """StepLR factor of the current epoch (AVE/main_trans_v3.py:323)."""
        return self.gamma ** (self.epoch // self.step_size) if self.step_size else 1.0

    @property
    def lr(self) -> float:
        return self.lr0 * self.decay

    def step(self):
        L = capi.lib()
        self._not_swapped("step()")
        self.t += 1
        # 1 / world of a sum-reducing AdapterGradReducer(average="optimizer") rides in the kernel's gradient scale: no division pass
        scale = self.grad_scale * float(getattr(self.reducer, "grad_scale", 1.0))
        if self._device:                                 # every bucket at once, scalars from the device state block
            stream = torch.cuda.current_stream(self._dev).cuda_stream
            n, flags = len(self._recs), self._flags
            # the entry point that knows every flag: an option that is off is a flag not set and a NULL argument, and the flags choose
            # the kernels (finalize also writes f(applied_steps) and d_n, the update also averages -- the same three launches; with the
            # report, one more behind finalize).  The avmoe_opt_swa struct holds the uniform average's rule and the SWA rate.
            capi.check(L.avmoe_opt_grad_norm_swa(self._table_ptr, n, self._n_blocks, self._partials_ptr, self._state_ptr, scale,
                                                 self.max_grad_norm or 0.0, flags, self.betas[0], self.betas[1], stream,
                                                 None if self._sched_c is None else C.byref(self._sched_c),
                                                 None if self.ema_decay is None else C.byref(self._ema_c),
                                                 self._report.data_ptr() if self.report_grad_norms else None,
                                                 C.byref(self._swa_c) if flags & _SWA_FLAGS else None), "avmoe_opt_grad_norm_swa")
            # the update and the buffers' launch are those of the schedule and the exponential average, so the update gets THEIR flags
            # (AVMOE_OPT_LR_SCHEDULE for AVMOE_OPT_SWA_LR, AVMOE_OPT_EMA for AVMOE_OPT_SWA) and not the report's
            step_flags = flags & ~_NORM_ONLY_FLAGS
            if flags & _SWA_FLAGS:
                step_flags |= (cm.OPT_EMA if flags & cm.OPT_SWA else 0) | (cm.OPT_LR_SCHEDULE if flags & cm.OPT_SWA_LR else 0)
            self._update(L, stream, n, scale, step_flags, self._shadow_ptrs.data_ptr() if flags & _AVERAGE_FLAGS else None)
            if self._ebufs:                              # one launch more: the buffers' averages, with the d_n and skip flag finalize has left
                capi.check(L.avmoe_opt_ema_buffers(*self._ebuf_args, self._state_ptr, stream), "avmoe_opt_ema_buffers")
            return
        for s in self.state:
            for (o, e, r, wd) in s["ranges"]:
                st = L.avmoe_adam_step(s["p"].data_ptr() + 4 * o, s["g"].data_ptr() + 4 * o, s["m"].data_ptr() + 4 * o,
                                       s["v"].data_ptr() + 4 * o, C.c_int64(e - o), C.c_float(r * self.decay),
                                       C.c_float(self.betas[0]), C.c_float(self.betas[1]), C.c_float(self.eps),
                                       C.c_float(wd), C.c_int64(self.t), C.c_float(scale),
                                       torch.cuda.current_stream(s["p"].device).cuda_stream)
                capi.check(st, "avmoe_adam_step")

    def epoch_end(self):
        self.epoch += 1
        if self._device and self.decay != self._table_decay:      # the learning rates live in the table: one async copy, stream-ordered
            self._upload_table()

    # ---- resume ---------------------------------------------------------------------------------------------------
    def state_dict(self) -> dict:
        """torch.optim.Adam's format (class docstring).  A parameter's `step` is `self.t` on the plain path and `applied_steps` on the
        device path -- reading it makes state_dict() a synchronisation point, as the copies of the moments to the CPU are anyway."""
        self._not_swapped("state_dict()")
        self._not_perturbed("state_dict()")
        applied = int(self.applied_steps.item()) if self._device else self.t
        skipped = int(self.skipped_steps.item()) if self._device else 0
        state = {i: {"step": torch.tensor(float(applied)), "exp_avg": r.view("m").detach().cpu().clone(),
                     "exp_avg_sq": r.view("v").detach().cpu().clone()} for i, r in enumerate(self._recs)}
        f = self.lr_schedule.factor(applied) if self.lr_schedule is not None else None      # the rate of the next step
        groups = [{"lr": lr0 * self.decay if f is None else lr0 * self.decay * f, "initial_lr": lr0, "betas": tuple(self.betas), "eps": self.eps,
                   "weight_decay": wd, "params": list(idx)} for (lr0, wd), idx in self._keyed_groups()]
        extra = {"t": self.t, "epoch": self.epoch, "applied_steps": applied, "skipped_steps": skipped,
                 "max_grad_norm": self.max_grad_norm, "decoupled_weight_decay": self.decoupled_weight_decay,
                 "skip_nonfinite": self.skip_nonfinite, "step_size": self.step_size, "gamma": self.gamma}
        for on, save in ((self.lr_schedule is not None, self._save_schedule), (self._averaging, self._save_average),
                         (self._ebufs, self._save_buffers), (self.sam_rho is not None, self._save_sam), (self.trust_ratio, self._save_trust),
                         (self.prodigy, self._save_prodigy), (self.muon, self._save_muon), (self.schedule_free, self._save_sf)):
            if on:
                save(extra)
        if self.report_grad_norms:                       # informative, like the other path options; absent when off
            extra["report_grad_norms"] = True
        return {"state": state, "param_groups": groups, "flat_adam": extra}

    def load_state_dict(self, sd: dict):
        """Writes the moments into the flat buffers, the counters into the state block, and restores t, epoch, each group's lr and
        weight_decay (matched by position) and betas / eps (the first group's: they are per optimizer).  A saved per-step schedule replaces the one the constructor was given (device path only: on the plain path it
        raises); with the saved `applied_steps` the run continues it.  Saved parameters are matched to `self.params` by position across the groups, as torch.optim does; the three
        path options stay what the constructor was given (the saved ones are informative), unknown keys are ignored.  A count or shape
        mismatch raises ValueError naming the parameter index.  With `ema_decay`: saved averages ("ema", with "ema_decay" / "ema_warmup",
        which replace the constructor's) are restored; a dict without them re-seeds the averages from the CURRENT parameters, so load the
        model first.  Without `ema_decay` saved averages are ignored.  With `ema_buffers`: saved buffer averages ("ema_buffers", matched by
        position, "ema_buffer_names" informative) are restored -- a count or shape mismatch raises ValueError naming the buffer -- and a
        dict without them re-seeds the shadows from the CURRENT buffers; without the option saved ones are ignored.  With `sam_rho`: saved
        "sam_rho" / "sam_adaptive" replace the constructor's (ValueError for a bad value); a dict without them leaves them, and
        without the option saved ones are ignored.  With `trust_ratio`: a saved "trust_clip" (beside "trust_ratio": True) replaces the
        constructor's, likewise; which parameters are adapted stays what the constructor's groups say.  With `prodigy`: the saved constants,
        block ("prodigy_d", "prodigy_d_max", "prodigy_d_hat", "prodigy_num", "prodigy_den"), "prodigy_x0" and "prodigy_s" are restored
        (a count or shape mismatch raises ValueError naming the parameter); a dict without "prodigy" re-seeds: x0 = the CURRENT
        parameters, s = 0, d = d0, so load the model first.  Without the option a dict that carries "prodigy" raises ValueError: its
        rates are multipliers of d, not learning rates.  With `muon`: the saved constants ("muon_momentum", "muon_nesterov", "muon_ns_steps",
        "muon_scale") replace the constructor's; which parameters are orthogonalised stays what the constructor says; a dict without
        "muon" loads as before.  Without the option a dict that carries "muon" raises ValueError.  With `schedule_free`: the saved
        constants, block words ("sf_weight_sum", "sf_lr_max", "sf_c") and x ("ema") are restored, exp_avg is z; a dict without
        "schedule_free" keeps exp_avg_sq and the counters and re-seeds z = x = the CURRENT parameters with a zeroed block, so load the
        model first.  Without the option a dict that carries "schedule_free" raises ValueError: its exp_avg is no momentum."""
        self._not_swapped("load_state_dict()")
        self._not_perturbed("load_state_dict()")
        # 1. the groups and the moments
        saved_groups, own_groups = sd["param_groups"], self._groups()
        if len(saved_groups) != len(own_groups):
            raise ValueError(f"state dict has {len(saved_groups)} parameter groups, this optimizer {len(own_groups)}")
        for gi, (sg, (_lr0, idx)) in enumerate(zip(saved_groups, own_groups)):
            if len(sg["params"]) != len(idx):
                raise ValueError(f"parameter group {gi}: state dict lists {len(sg['params'])} parameters, this optimizer {len(idx)} "
                                 f"(first own parameter index {idx[0]})")
        id_map = dict(zip(chain.from_iterable(g["params"] for g in saved_groups), chain.from_iterable(idx for _, idx in own_groups)))
        todo, steps = [], set()
        for k, st in sd["state"].items():
            if k not in id_map:
                raise ValueError(f"state dict has state for parameter index {k}, which no parameter group lists")
            i = id_map[k]
            p = self._recs[i].p
            for name in ("exp_avg", "exp_avg_sq"):
                if name not in st or tuple(st[name].shape) != tuple(p.shape):
                    got = tuple(st[name].shape) if name in st else None
                    raise ValueError(f"parameter index {i}: {name} has shape {got}, the parameter {tuple(p.shape)}")
            steps.add(int(float(st["step"])))
            todo.append((i, st))
        if todo and len(todo) != len(self._recs):
            missing = sorted(set(range(len(self._recs))) - {i for i, _ in todo})
            raise ValueError(f"state dict has no state for parameter index {missing[0]} ({len(missing)} missing; FlatAdam steps all its "
                             "parameters together)")
        if len(steps) > 1:
            raise ValueError(f"parameters carry different step counts {sorted(steps)}: FlatAdam keeps one count for all")
        extra = sd.get("flat_adam", {})
        applied = int(extra.get("applied_steps", steps.pop() if steps else 0))
        # 2. every option's saved keys, validated; nothing is written yet
        sched = self._check_saved_schedule(extra)
        average = self._check_saved_average(extra)
        sam = self._check_saved_sam(extra)
        trust = self._check_saved_trust(extra)
        prodigy = self._check_saved_prodigy(extra)
        muon = self._check_saved_muon(extra)
        sf = self._check_saved_sf(extra)
        buffers = self._check_saved_buffers(extra)
        with torch.no_grad():
            # 3. moments, groups and rates
            if not todo:
                for s in self.state:
                    s["m"].zero_(); s["v"].zero_()
            for i, st in todo:
                self._recs[i].view("m").copy_(st["exp_avg"].to(torch.float32))
                self._recs[i].view("v").copy_(st["exp_avg_sq"].to(torch.float32))
            self.epoch = int(extra.get("epoch", self.epoch))
            self.step_size, self.gamma = extra.get("step_size", self.step_size), extra.get("gamma", self.gamma)
            g0 = saved_groups[0]
            self.betas, self.eps = tuple(g0.get("betas", self.betas)), g0.get("eps", self.eps)
            wds = [sg.get("weight_decay", wd) for sg, wd in zip(saved_groups, self._group_decays())]
            for (_lr_old, idx), wd in zip(own_groups, wds):
                for i in idx:
                    self._recs[i].wd = wd
            if len(set(wds)) == 1:                        # one decay for all: the optimizer's own, as the constructor's argument is
                self.wd = wds[0]
            self._apply_saved_schedule(sched)
            # a dict without initial_lr comes from a torch optimizer that never had a scheduler: its lr is a base rate, whatever the
            # schedule here says (every dict FlatAdam or a torch scheduler wrote carries initial_lr)
            lr0s = [float(sg["initial_lr"]) if "initial_lr" in sg else float(sg["lr"]) / self.decay for sg in saved_groups]
            for (_lr_old, idx), lr_new in zip(own_groups, lr0s):
                for i in idx:
                    self._recs[i].lr0 = lr_new
            if len(own_groups) == 1:
                self.lr0 = lr0s[0]
            self._rebuild_plain_ranges()
            # 4. every option's payload, then the range table
            self._apply_saved_sam(sam)
            self._apply_saved_trust(trust)
            if not self._device:
                self.t = applied                          # the plain path's bias correction counts self.t
                return
            self.t = int(extra.get("t", applied + int(extra.get("skipped_steps", 0))))
            self._views["applied_steps"].fill_(applied)
            self._views["skipped_steps"].fill_(int(extra.get("skipped_steps", 0)))
            if self.lr_schedule is not None:               # what the last applied step used; the next applied step writes its own
                self._views["lr_factor"].fill_(self.lr_schedule.factor(applied - 1) if applied > 0 else 0.0)
            if self._averaging:
                self._apply_saved_average(average, applied)
            if self._ebufs:
                self._apply_saved_buffers(buffers)
            self._apply_saved_muon(muon)
            if self.prodigy:
                self._apply_saved_prodigy(prodigy)
            if self.schedule_free:
                self._apply_saved_sf(sf)
            self._upload_table()

    def _rebuild_plain_ranges(self):
        """the plain path's merged [begin, end, lr0, weight_decay] ranges per bucket from the per-parameter learning rates and decays:
        neighbouring parameters with the same rate and the same decay share one kernel launch, alignment padding rides with its left
        neighbour"""
        for si, s in enumerate(self.state):
            spans = sorted((r.off, r.off + r.p.numel(), r.lr0, r.wd) for r in self._recs if r.bucket == si)
            ranges = []
            for i, (o, e, r, wd) in enumerate(spans):
                end = spans[i + 1][0] if i + 1 < len(spans) else s["g"].numel()
                if ranges and ranges[-1][2:] == [r, wd]:
                    ranges[-1][1] = end
                else:
                    ranges.append([o if ranges else 0, end, r, wd])
            s["ranges"] = ranges

