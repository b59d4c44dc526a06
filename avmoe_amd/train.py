"""The steps either side of the adapter path on the reference's training loop, MI355X-side:

  * `select_trainable`      -- the parameter-freezing / LR-group rule of AVE/main_trans_v3.py:264-315
  * `FlatAdam`, `LRSchedule` -- the flat-bucket optimizer and its per-step schedule live in avmoe_amd/flat_adam.py and are imported here,
                               so `from avmoe_amd.train import FlatAdam, LRSchedule` keeps working; replaces optimizer.step() at
                               main_trans_v3.py:136-138,322-323
  * `hold_bn_stats`         -- a context in which training-mode forward passes leave the BatchNorm running statistics alone (SAM's
                               second pass)
  * `reestimate_bn`         -- BatchNorm statistics re-estimated with forward passes (momentum=None, torch's update_bn), for the
                               raw weights or, with `ema=opt`, for FlatAdam's averaged weights
  * `expert_choice_mask`    -- expert-choice gating as a function: which frames each expert takes from an (S, E) matrix, on the device
  * `sinkhorn_scale` / `sinkhorn_topk` -- Sinkhorn-balanced top-k routing as functions: the column scale of an (S, E) matrix and the
                               selection it gives, on the device
  * `CapacityMeter`         -- the demand and the kept frames of sites with an expert capacity, accumulated on the device
  * `top_p_mask`            -- top-p routing as a function: which experts each frame of an (S, E) matrix takes, on the device
  * `TopPMeter`             -- how many experts the frames of top-p sites take, accumulated on the device
  * `RouterBiasBalancer`    -- aux-loss-free expert balancing of top-k sites: a bias on the selection, updated on the device after
                               every optimizer step
  * `ExpertActivationCounter` -- per-layer expert-activation tables accumulated on the device (no idx.tolist() sync per
                               site), main_trans_v3.py:155-226
  * `save_adapters` / `load_adapters` / `strip_prefix` -- adapter-only checkpoints with the reference's state_dict keys
                               (strict=False load of released checkpoints, main_trans_v3.py:254; HTS-AT key strip,
                               net_trans_v3.py:560-563)

Everything here is host logic around a few small C-ABI entry points (avmoe_expert_histogram, avmoe_router_topk; the optimizer's are
named in avmoe_amd/flat_adam.py); nothing falls back to the CPU for GPU tensors."""
from __future__ import annotations

import contextlib
import ctypes as C
from itertools import chain
from typing import Dict, Iterable, List, Optional

import torch

from . import _capi as capi
from .flat_adam import FlatAdam, LRSchedule  # noqa: F401  (their home: avmoe_amd/flat_adam.py)


# ---------------------------------------------------------------------------------------------------------------------
def select_trainable(model: torch.nn.Module, lr: float, lr_mlp: float, is_vit_ln: bool = False,
                     trainable_substrings=("adapter_blocks", "CMBS", "mlp_class", "temporal_attn"),
                     frozen_substrings=("htsat",), backbone_substrings=("ViT", "swin")) -> List[dict]:
    """Sets requires_grad exactly like the reference launcher and returns its Adam parameter groups: every parameter gets
    its own group, lr_mlp for names containing 'mlp_class', lr otherwise (AVE/main_trans_v3.py:264-315)."""
    groups = []
    for name, p in model.named_parameters():
        p.requires_grad = False
        if any(s in name for s in backbone_substrings):
            p.requires_grad = bool(is_vit_ln) and "norm" in name
        elif any(s in name for s in frozen_substrings):
            p.requires_grad = False
        elif any(s in name for s in trainable_substrings):
            p.requires_grad = True
        groups.append({"params": p, "lr": lr_mlp if "mlp_class" in name else lr, "name": name})
    return groups


# ---------------------------------------------------------------------------------------------------------------------
class ExpertActivationCounter:
    """counts[table][layer][expert] accumulated on the device from the `idx` tensors the sites return; `.numpy()` at the end
    of the evaluation is the only host sync (the reference calls idx.squeeze().tolist() after every site)."""

    def __init__(self, tables: Iterable[str], num_layers: int, num_experts: int, device):
        self.names = list(tables)
        self.L, self.E = num_layers, num_experts
        self.counts = torch.zeros(len(self.names), num_layers, num_experts, dtype=torch.int64, device=device)

    def update(self, table: str, layer: int, idx: torch.Tensor):
        if not idx.is_cuda or idx.dtype != torch.int64:
            raise capi.AvmoeError("expert indices must be an int64 GPU tensor (as returned by MoEAdapter.forward)")
        idx = idx.reshape(-1).contiguous()
        row = self.counts[self.names.index(table), layer]
        st = capi.lib().avmoe_expert_histogram(idx.data_ptr(), C.c_int64(idx.numel()), C.c_int32(self.E), row.data_ptr(),
                                               torch.cuda.current_stream(idx.device).cuda_stream)
        capi.check(st, "avmoe_expert_histogram")

    def numpy(self) -> Dict[str, "object"]:
        c = self.counts.cpu().numpy()
        return {n: c[i] for i, n in enumerate(self.names)}


class CapacityMeter:
    """How much an expert capacity drops (`site.router_capacity_factor`; include/avmoe.h at avmoe_moe_forward_capacity): `demand` and
    `kept_count` of every TRAINING forward of `sites`, accumulated per site into (E_i,) int64 tensors on the reports' device -- two adds on
    the forward's own stream, no host synchronisation (the companion of `ExpertActivationCounter`).  The sites tell their meters
    themselves, so the two sites of an `AdapterPair` and captured steps are counted like any other call.  `overflow()` gives the dropped
    share per site and expert and synchronises; `reset()` clears the totals; `close()` detaches the meter from the sites."""

    def __init__(self, sites):
        self.sites = list(sites)
        if not self.sites:
            raise ValueError("CapacityMeter: no sites")
        self.demand = [None] * len(self.sites)
        self.kept = [None] * len(self.sites)
        self.calls = [0] * len(self.sites)
        for s in self.sites:
            s.__dict__.setdefault("_capacity_meters", []).append(self)

    def update(self, site, report):
        """Add one call's CapacityReport of `site` (a site of this meter, or its index) to the totals."""
        i = site if isinstance(site, int) else next(j for j, s in enumerate(self.sites) if s is site)
        d, k = report.demand.to(torch.int64), report.kept_count.to(torch.int64)
        if self.demand[i] is None or self.demand[i].device != d.device:
            self.demand[i], self.kept[i] = torch.zeros_like(d), torch.zeros_like(k)
        self.demand[i] += d
        self.kept[i] += k
        self.calls[i] += 1

    def overflow(self) -> List[torch.Tensor]:
        """Per site, the share of the token-expert pairs each expert dropped since the last reset(): (E_i,) float64 CPU tensors,
        (demand - kept) / demand, 0 where nothing selected the expert; None for a site that has not reported.  Synchronises."""
        out = []
        for d, k in zip(self.demand, self.kept):
            if d is None:
                out.append(None)
                continue
            d, k = d.cpu().to(torch.float64), k.cpu().to(torch.float64)
            out.append(torch.where(d > 0, (d - k) / d.clamp_min(1.0), torch.zeros_like(d)))
        return out

    def reset(self):
        for t in self.demand + self.kept:
            if t is not None:
                t.zero_()
        self.calls = [0] * len(self.sites)

    def close(self):
        for s in self.sites:
            m = s.__dict__.get("_capacity_meters", [])
            if self in m:
                m.remove(self)


def top_p_mask(probs: torch.Tensor, p: float, k_min: int = 1, k_max: Optional[int] = None) -> torch.Tensor:
    """(S, E) bool: row s is True on the fewest ranked experts of probs[s] whose running mass reaches `p` (higher probability first, equal
    ones in expert order), at least `k_min` and at most `k_max` (default E) of them -- include/avmoe.h at avmoe_router_top_p.  The sites'
    own kernel (`site.router_top_p`) on a caller's matrix."""
    L = capi.lib()
    if not getattr(L, "avmoe_site_top_p", False):
        raise capi.AvmoeError("this libavmoe_hip.so predates avmoe_moe_forward_top_p / avmoe_router_top_p: it serves no top-p routing")
    if not probs.is_cuda:
        raise capi.AvmoeError("top_p_mask runs on the GPU (no CPU fallback)")
    q = probs.reshape(-1, probs.shape[-1]).to(torch.float32).contiguous()
    S, E = q.shape
    bits = torch.empty(S, dtype=torch.int32, device=q.device)
    st = L.avmoe_router_top_p(q.data_ptr(), S, E, float(p), int(k_min), int(E if k_max is None else k_max), 0, None, None, bits.data_ptr(),
                              None, None, torch.cuda.current_stream(q.device).cuda_stream)
    capi.check(st, "avmoe_router_top_p")
    return (bits[:, None] >> torch.arange(E, device=q.device, dtype=torch.int32)[None, :]) & 1 != 0


class TopPMeter:
    """How many experts the frames of top-p sites take (`site.router_top_p`; include/avmoe.h at avmoe_moe_forward_top_p): `khist` and
    `count` of every forward of `sites`, accumulated per site into (E_i + 1,) and (E_i,) int64 tensors on the reports' device -- two adds on
    the forward's own stream, no host synchronisation (the companion of `CapacityMeter`).  The sites tell their meters themselves, so the
    two sites of an `AdapterPair` and captured steps are counted like any other call.  `mean_experts()` gives the mean number of experts
    per frame and site and synchronises; `reset()` clears the totals; `close()` detaches the meter from the sites."""

    def __init__(self, sites):
        self.sites = list(sites)
        if not self.sites:
            raise ValueError("TopPMeter: no sites")
        self.khist = [None] * len(self.sites)
        self.count = [None] * len(self.sites)
        self.calls = [0] * len(self.sites)
        for s in self.sites:
            s.__dict__.setdefault("_top_p_meters", []).append(self)

    def update(self, site, report):
        """Add one call's TopPReport of `site` (a site of this meter, or its index) to the totals."""
        i = site if isinstance(site, int) else next(j for j, s in enumerate(self.sites) if s is site)
        h, c = report.khist.to(torch.int64), report.count.to(torch.int64)
        if self.khist[i] is None or self.khist[i].device != h.device:
            self.khist[i], self.count[i] = torch.zeros_like(h), torch.zeros_like(c)
        self.khist[i] += h
        self.count[i] += c
        self.calls[i] += 1

    def mean_experts(self) -> List[Optional[float]]:
        """Per site, the mean number of experts a frame took since the last reset(): sum_j j khist[j] / sum_j khist[j]; None for a site
        that has not reported.  Synchronises."""
        out = []
        for h in self.khist:
            if h is None or int(h.sum()) == 0:
                out.append(None)
                continue
            h = h.cpu().to(torch.float64)
            out.append(float((h * torch.arange(h.numel(), dtype=torch.float64)).sum() / h.sum()))
        return out

    def reset(self):
        for t in self.khist + self.count:
            if t is not None:
                t.zero_()
        self.calls = [0] * len(self.sites)

    def close(self):
        for s in self.sites:
            m = s.__dict__.get("_top_p_meters", [])
            if self in m:
                m.remove(self)


def topk_experts(probs: torch.Tensor, k: int) -> torch.Tensor:
    """(S, k) int64: the k most probable experts per frame, most probable first, ties in expert order (column 0 == the `idx`
    the sites return).  Extension for statistics (BASELINE config 3); the mixture stays dense as in the reference."""
    if not probs.is_cuda:
        raise capi.AvmoeError("topk_experts runs on the GPU (no CPU fallback)")
    p = probs.reshape(-1, probs.shape[-1]).to(torch.float32).contiguous()
    out = torch.empty(p.shape[0], k, dtype=torch.int64, device=p.device)
    st = capi.lib().avmoe_router_topk(p.data_ptr(), C.c_int64(p.shape[0]), C.c_int32(p.shape[1]), C.c_int32(k), out.data_ptr(),
                                      torch.cuda.current_stream(p.device).cuda_stream)
    capi.check(st, "avmoe_router_topk")
    return out


def expert_choice_mask(probs: torch.Tensor, capacity: int) -> torch.Tensor:
    """(S, E) bool: expert-choice gating as a function (include/avmoe.h at avmoe_expert_choice) -- column e is True on the `capacity`
    frames with the highest probs[:, e], higher probability first, equal probabilities in frame order.  The sites' own selection
    (`site.router_expert_choice`) on a caller's matrix."""
    L = capi.lib()
    if not getattr(L, "avmoe_site_choice", False):
        raise capi.AvmoeError("this libavmoe_hip.so predates avmoe_moe_forward_choice / avmoe_expert_choice: it serves no expert-choice gating")
    if not probs.is_cuda:
        raise capi.AvmoeError("expert_choice_mask runs on the GPU (no CPU fallback)")
    p = probs.reshape(-1, probs.shape[-1]).to(torch.float32).contiguous()
    S, E = p.shape
    bits = torch.empty(S, dtype=torch.int32, device=p.device)
    st = L.avmoe_expert_choice(p.data_ptr(), S, E, int(capacity), 0, None, None, bits.data_ptr(), None, None,
                               torch.cuda.current_stream(p.device).cuda_stream)
    capi.check(st, "avmoe_expert_choice")
    return (bits[:, None] >> torch.arange(E, device=p.device, dtype=torch.int32)[None, :]) & 1 != 0


def _sinkhorn(probs, k, iters, want_mask):
    L = capi.lib()
    if not getattr(L, "avmoe_site_sinkhorn", False):
        raise capi.AvmoeError("this libavmoe_hip.so predates avmoe_moe_forward_sinkhorn / avmoe_router_sinkhorn: it serves no Sinkhorn routing")
    if not probs.is_cuda:
        raise capi.AvmoeError("sinkhorn_scale / sinkhorn_topk run on the GPU (no CPU fallback)")
    p = probs.reshape(-1, probs.shape[-1]).to(torch.float32).contiguous()
    S, E = p.shape
    v = torch.empty(E, dtype=torch.float32, device=p.device)
    bits = torch.empty(S, dtype=torch.int32, device=p.device) if want_mask else None
    st = L.avmoe_router_sinkhorn(p.data_ptr(), S, E, int(k), 0, int(iters), None, None, bits.data_ptr() if want_mask else None, None,
                                 v.data_ptr(), torch.cuda.current_stream(p.device).cuda_stream)
    capi.check(st, "avmoe_router_sinkhorn")
    return v, bits, E


def sinkhorn_scale(probs: torch.Tensor, iters: int) -> torch.Tensor:
    """(E,) float32: the column scale v of Sinkhorn-balanced routing (include/avmoe.h at avmoe_router_sinkhorn) after `iters` rounds of
    row / column normalisation of the (S, E) matrix `probs`.  The sites' own kernel (`site.router_sinkhorn`) on a caller's matrix."""
    return _sinkhorn(probs, 1, iters, False)[0]


def sinkhorn_topk(probs: torch.Tensor, k: int, iters: int) -> torch.Tensor:
    """(S, E) bool: row s is True on the k experts with the largest probs[s, e] * v[e], v = sinkhorn_scale(probs, iters); equal products
    in expert order.  Exactly k experts per frame."""
    _v, bits, E = _sinkhorn(probs, k, iters, True)
    return (bits[:, None] >> torch.arange(E, device=bits.device, dtype=torch.int32)[None, :]) & 1 != 0


# ---------------------------------------------------------------------------------------------------------------------
def router_aux_total(sites, z_weight: float = 0.0, balance_weight: float = 0.0) -> torch.Tensor:
    """sum over `sites` of z_weight * z_loss + balance_weight * balance_loss of their last forward (`site.last_router_aux`: sites with
    `router_aux` on) as one differentiable scalar -- the term to add to the task loss.  Differentiated alone, it takes the sites'
    router-only backward.  Raises if a listed site has no results (setting off, or no forward yet)."""
    terms = []
    for i, site in enumerate(sites):
        aux = getattr(site, "last_router_aux", None)
        if aux is None:
            raise ValueError(f"router_aux_total: site {i} ({type(site).__name__}) has no router auxiliary losses: set site.router_aux = True "
                             "before its forward")
        terms.append(z_weight * aux.z_loss + balance_weight * aux.balance_loss)
    if not terms:
        raise ValueError("router_aux_total: no sites")
    return torch.stack(terms).sum()


class RouterBiasBalancer:
    """Aux-loss-free expert balancing of top-k sites (Wang et al. 2024; include/avmoe.h at avmoe_moe_forward_bias): every site gets a
    per-expert bias that enters its top-k SELECTION only, every training forward adds its selection counts to the site's row of
    `counts`, and `step()` -- once per optimizer step, after `opt.step()` -- lowers the bias of the experts that were selected more often
    than the mean by `rate`, raises the others' and clears the counts: ONE launch for all sites (avmoe_router_bias_update), no gradient,
    no loss term.  bias and counts are flat (n_sites, 16) fp32 tensors on the sites' device, the sites hold views of their rows
    (`site.router_select_bias`, `site.router_select_count`: plain attributes, no state_dict key).  The sites must run with
    `router_top_k` in [1, E).  With `group` of more than one rank, step() first sums the counts over the ranks, so every rank makes the
    same update."""

    ROW = 16                                             # AVMOE_MAX_EXPERTS: the row length of bias / counts

    def __init__(self, sites, rate: float = 1e-3, group=None):
        self.sites = list(sites)
        if not self.sites:
            raise ValueError("RouterBiasBalancer: no sites")
        self.rate = self._rate(rate)
        self.group = group
        self.E = [int(s.num_multimodal_experts + s.num_singlemodal_experts) for s in self.sites]
        for i, e in enumerate(self.E):
            if not 1 <= e <= self.ROW:
                raise ValueError(f"RouterBiasBalancer: site {i} has {e} experts, outside [1, {self.ROW}]")
        devs = {next(s.parameters()).device for s in self.sites}
        if len(devs) != 1:
            raise ValueError(f"RouterBiasBalancer: the sites live on several devices ({sorted(map(str, devs))})")
        self.device = devs.pop()
        n = len(self.sites)
        self.bias = torch.zeros(n, self.ROW, dtype=torch.float32, device=self.device)
        self.counts = torch.zeros(n, self.ROW, dtype=torch.float32, device=self.device)
        self.E_table = torch.tensor(self.E, dtype=torch.int32, device=self.device)
        for i, (s, e) in enumerate(zip(self.sites, self.E)):      # each site its own row: the two sites of a pair never share one
            s.router_select_bias, s.router_select_count = self.bias[i, :e], self.counts[i, :e]

    @staticmethod
    def _rate(rate):
        import math
        if isinstance(rate, bool) or not isinstance(rate, (int, float)) or not math.isfinite(rate) or rate < 0:
            raise ValueError(f"RouterBiasBalancer: rate must be a finite number >= 0, got {rate!r}")
        return float(rate)

    def step(self):
        """The update after an optimizer step: (the counts summed over `group`,) one avmoe_router_bias_update launch on the current stream."""
        L = capi.lib()
        if not getattr(L, "avmoe_site_bias", False):
            raise capi.AvmoeError("this libavmoe_hip.so predates avmoe_moe_forward_bias / avmoe_router_bias_update: it serves no router selection bias")
        if not self.bias.is_cuda:
            raise capi.AvmoeError("RouterBiasBalancer.step runs on the GPU (no CPU fallback)")
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized() and dist.get_world_size(self.group) > 1:
            dist.all_reduce(self.counts, op=dist.ReduceOp.SUM, group=self.group)      # integers in fp32: exact, the same on every rank
        st = L.avmoe_router_bias_update(self.bias.data_ptr(), self.counts.data_ptr(), self.E_table.data_ptr(), len(self.sites),
                                        self.rate, torch.cuda.current_stream(self.device).cuda_stream)
        capi.check(st, "avmoe_router_bias_update")

    def loads(self) -> List[torch.Tensor]:
        """Per site, the share of the selections each expert received since the last step() ((E_i,) tensors that sum to 1; zeros when
        nothing was counted).  The counts are not cleared."""
        out = []
        for i, e in enumerate(self.E):
            c = self.counts[i, :e]
            out.append(c / c.sum().clamp_min(1.0))
        return out

    def state_dict(self) -> dict:
        return {"bias": self.bias.detach().cpu().clone(), "counts": self.counts.detach().cpu().clone(), "E": list(self.E), "rate": self.rate}

    def load_state_dict(self, state: dict):
        if list(state["E"]) != self.E:
            raise ValueError(f"RouterBiasBalancer.load_state_dict: the state is for sites with {list(state['E'])} experts, these have {self.E}")
        for name in ("bias", "counts"):
            t = torch.as_tensor(state[name], dtype=torch.float32)
            if tuple(t.shape) != (len(self.sites), self.ROW):
                raise ValueError(f"RouterBiasBalancer.load_state_dict: {name} has shape {tuple(t.shape)}, expected {(len(self.sites), self.ROW)}")
            getattr(self, name).copy_(t)                 # in place: the sites keep their views
        self.rate = self._rate(state["rate"])

    def detach(self):
        """Gives the sites back their None: they run unbiased again, and count nothing."""
        for s in self.sites:
            s.router_select_bias = s.router_select_count = None


@contextlib.contextmanager
def hold_bn_stats(model: torch.nn.Module):
    """`with hold_bn_stats(model): loss_fn(model(batch)).backward()` -- inside, every `torch.nn.modules.batchnorm._BatchNorm` of `model`
    has `momentum = 0.0`: a training-mode forward pass normalises with the batch statistics as ever and leaves `running_mean` /
    `running_var` as they are (running = (1 - 0) * running + 0 * batch).  The second pass of a sharpness-aware step (FlatAdam,
    "Sharpness-aware minimization") runs on perturbed weights and must not move the statistics a second time.  The adapter sites read
    `momentum` on every call (MoEAdapter._bn_momentum), torch's own BatchNorm modules likewise.  The momenta are restored on exit, also
    when the body raises.  `num_batches_tracked` still advances inside, as torch's does with momentum 0: the counter only matters to
    momentum=None, which this context refuses.  A batch statistic that is Inf or NaN still reaches the running one (0 * Inf is NaN).
    ValueError, before anything is touched, when a BatchNorm has `momentum=None`: a cumulative average has no factor to hold it with."""
    bns = [(k, m) for k, m in model.named_modules() if isinstance(m, torch.nn.modules.batchnorm._BatchNorm)]
    for k, m in bns:
        if m.momentum is None:
            raise ValueError(f"hold_bn_stats: BatchNorm {k!r} has momentum=None (the cumulative average), which cannot be held")
    momenta = [m.momentum for _k, m in bns]
    try:
        for _k, m in bns:
            m.momentum = 0.0
        yield model
    finally:
        for (_k, m), mom in zip(bns, momenta):
            m.momentum = mom


def reestimate_bn(model: torch.nn.Module, batches: Iterable, forward=None, ema: Optional[FlatAdam] = None) -> int:
    """Re-estimates the running statistics of every BatchNorm in `model` with training-mode forward passes over `batches` -- the last
    step of weight averaging (torch.optim.swa_utils.update_bn): every `torch.nn.modules.batchnorm._BatchNorm` (the adapter sites' own
    and any other) is reset in place, switched to `momentum=None` (torch's cumulative average: the sites form 1 / num_batches_tracked
    on the device, include/avmoe.h at avmoe_moe_desc.bn_momentum) and the batches are run under `torch.no_grad()`.  Returns the number
    of batches run; every `momentum` and every module's `training` flag is restored, also when a batch raises.

    forward(model, batch) runs one batch; default `model(*batch)` for a tuple or list, else `model(batch)` (update_bn itself passes
    `batch[0]`, which cannot drive a model that takes two modalities).

    ema=None: update_bn's behaviour -- the model's own statistics are the re-estimated ones and the counters are left at the number of
    batches.  ema=opt (a FlatAdam with `ema_decay`, `swa_start` or `schedule_free`, and `ema_buffers`): everything runs inside `opt.ema_weights()`, so the forward
    passes see the AVERAGED weights and write the buffers that hold the averaged statistics meanwhile; after the swap back
    `opt.ema_buffers` are the re-estimated statistics, the model's raw weights and raw statistics are bit for bit what they were, and
    the counters (integer buffers, outside the optimizer's table: not swapped) are copied back in place.  ValueError, before anything
    is touched, when `opt` has no `ema_buffers` or a float buffer of a statistics-tracking BatchNorm of `model` is not among them (by
    address: its raw statistics would be overwritten); RuntimeError while the averages are already swapped in.  When a batch raises,
    the swap back, the momenta, the flags and the counters are still restored, but `opt.ema_buffers` are left partly re-estimated.

    Empty `batches`: returns 0 and leaves everything as it was.

    Training-mode side effects of the model are the caller's: the AVS "v1" attention dropout draws from the global RNG, and the AVS
    `is_training` noise flag is set inside `forward`.  Later `opt.step()` calls keep averaging into the re-estimated shadows, so call
    this right before an evaluation or a checkpoint (`save_adapters(model, path, ema=opt)` then writes the re-estimated statistics)."""
    bns = [(k, m) for k, m in model.named_modules() if isinstance(m, torch.nn.modules.batchnorm._BatchNorm)]
    if ema is not None:
        if not getattr(ema, "_ebufs", None):
            raise ValueError("reestimate_bn: ema has no ema_buffers (FlatAdam(ema_decay=..., ema_buffers=model)): the re-estimated statistics "
                             "would overwrite the raw ones")
        have = {t.data_ptr() for _name, t in ema._ebufs}
        for k, m in bns:
            for attr in ("running_mean", "running_var"):
                t = m._buffers.get(attr)
                if t is not None and t.data_ptr() not in have:
                    raise ValueError(f"reestimate_bn: buffer {k + '.' if k else ''}{attr} is not among ema's ema_buffers: its raw statistics "
                                     "would be overwritten")
        ema._not_swapped("reestimate_bn()")
    it = iter(batches)
    try:
        first = next(it)
    except StopIteration:
        return 0
    if forward is None:
        forward = lambda mod, batch: mod(*batch) if isinstance(batch, (tuple, list)) else mod(batch)
    momenta = [m.momentum for _k, m in bns]
    flags = [(m, m.training) for m in model.modules()]
    counts = [(m.num_batches_tracked, m.num_batches_tracked.clone()) for _k, m in bns if m.num_batches_tracked is not None]
    n = 0
    with (ema.ema_weights() if ema is not None else contextlib.nullcontext()):
        try:
            for _k, m in bns:
                m.reset_running_stats()                  # in place: the sites and FlatAdam's buffer table keep the addresses
                m.momentum = None
            model.train()
            with torch.no_grad():
                for batch in chain((first,), it):
                    forward(model, batch)
                    n += 1
        finally:
            for (_k, m), mom in zip(bns, momenta):
                m.momentum = mom
            for m, flag in flags:
                m.training = flag
            if ema is not None:
                with torch.no_grad():
                    for t, old in counts:
                        t.copy_(old)
    return n


def adapter_state_dict(model: torch.nn.Module, substrings=("adapter",), ema: Optional[FlatAdam] = None) -> Dict[str, torch.Tensor]:
    """The adapter / router entries of model.state_dict() (keys containing 'adapter': `*_adapter_blocks_p{1,2}.*`).
    ema: a FlatAdam built with `ema_decay`, `swa_start` or `schedule_free` -- every parameter it holds is written with its AVERAGED value (`opt.ema_params`), and with
    `ema_buffers` every buffer it holds (BatchNorm running statistics) with its averaged value too (`opt.ema_buffers`); everything else
    (other buffers, parameters outside the optimizer) as it is.  The model is not modified, and the result loads with `load_adapters`
    like any other.  RuntimeError while `ema` holds perturbed weights (sam_perturb)."""
    src, bsrc = {}, {}
    if ema is not None:
        ema._not_perturbed("adapter_state_dict(ema=...)")
        if not ema._swapped:                             # inside ema_weights() the parameters and buffers ARE the averages already
            src = {id(p): e for p, e in zip(ema.params, ema.ema_params)}
            if ema._ebufs:                               # by address and shape: state_dict() hands out the buffer tensors themselves
                bsrc = {(t.data_ptr(), tuple(t.shape)): e for (_name, t), e in zip(ema._ebufs, ema.ema_buffers)}
        else:
            ema.ema_params                               # (raises without ema_decay)

    def pick(v):
        if id(v) in src:
            return src[id(v)]
        return bsrc.get((v.data_ptr(), tuple(v.shape)), v) if bsrc and v.dtype == torch.float32 else v
    return {k: pick(v).detach().cpu().clone() for k, v in model.state_dict(keep_vars=True).items() if any(s in k for s in substrings)}


def save_adapters(model: torch.nn.Module, path: str, substrings=("adapter",), ema: Optional[FlatAdam] = None):
    """torch.save of `adapter_state_dict(model, substrings, ema)`"""
    torch.save(adapter_state_dict(model, substrings, ema), path)


def load_adapters(model: torch.nn.Module, path_or_state, strict_adapters: bool = True):
    """Loads a full released checkpoint or an adapter-only file with strict=False (the reference's own call,
    AVE/main_trans_v3.py:254) and reports what did not match.  strict_adapters: every adapter key of the MODEL must have been
    found (raises otherwise) -- backbone / head keys may be missing."""
    sd = torch.load(path_or_state, map_location="cpu") if isinstance(path_or_state, str) else path_or_state
    res = model.load_state_dict(sd, strict=False)
    if strict_adapters:
        missing = [k for k in res.missing_keys if "adapter" in k]
        if missing:
            raise KeyError(f"checkpoint lacks adapter entries: {missing[:5]}{' ...' if len(missing) > 5 else ''}")
    return res


def strip_prefix(state_dict: Dict[str, torch.Tensor], n: int = 10) -> Dict[str, torch.Tensor]:
    """k[n:] for every key -- how the reference loads the HTS-AT checkpoint whose keys carry a 10-character module prefix
    (net_trans_v3.py:560-563)."""
    return {k[n:]: v for k, v in state_dict.items()}
