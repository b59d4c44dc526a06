"""Host-side mirror of the reference's adapter modules, running on the HIP path.

`MoEAdapter` / `ExpertAdapter` keep the reference's constructor arguments, `forward` signatures, return
tuples and `state_dict` key names for each of its five task copies, so the task models (AVE / AVQA /
AVVP / AVS) can import them instead of their own classes and load released checkpoints unchanged:

    AVE   AVMOE/AVE/nets/net_trans_v3.py:296-487           -> avmoe_amd.adapters.MoEAdapter (= ave)
    AVQA  AVMOE/AVQA/net_grd_avst/net_avst_v2.py:215-399   -> avmoe_amd.adapters.MoEAdapterAVQA
    AVVP  AVMOE/AVVP/nets/mgn.py:39-224                    -> avmoe_amd.adapters.MoEAdapterAVVP
    AVS   AVMOE/AVS/avs_scripts/avs_{s4,ms3}/model/PVT_AVSModel_v2.py:90-318 -> avmoe_amd.adapters.MoEAdapterAVS

The submodules (`conv_adapter`, `fc`, `router`, `multimodal_experts.{j}.bn1`, ...) are real torch modules
used ONLY as parameter containers (same names, shapes and default initialisation as the reference); their
own `forward` is never called.  All arithmetic happens in avmoe_amd/lib/libavmoe_hip.so through
`AdapterFunction` (a `torch.autograd.Function` over the C ABI).  There is no eager / CPU fallback: a
missing library or a non-GPU tensor raises.
"""
from __future__ import annotations

import ctypes as C
import itertools
import math
from collections import namedtuple
from fractions import Fraction
from typing import Dict

import numbers
import os
import torch
import torch.nn as nn

from . import _capi as capi
from . import _capi_moe as cm

_SCRATCH: Dict[tuple, torch.Tensor] = {}
_MIX_SITES = itertools.count()       # construction order of the sites of this process: the per-site index behind the default `mix_seed`
_SIDE_STREAMS: Dict[int, "torch.cuda.Stream"] = {}


def side_stream(dev: torch.device) -> "torch.cuda.Stream":
    """THE side stream of a device: every AdapterPair shares it (pairs run one after another, so one second stream -- and one
    second scratch workspace -- is all the concurrency there is to have)."""
    key = dev.index if dev.index is not None else torch.cuda.current_device()
    st = _SIDE_STREAMS.get(key)
    if st is None:
        st = _SIDE_STREAMS[key] = torch.cuda.Stream(device=dev)
    return st


def release_workspaces():
    """Drops the cached transient workspaces (one per device and stream) -- e.g. after the largest site shape of a run has
    changed.  Synchronises first: kernels still in flight may be using them."""
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    _SCRATCH.clear()


def _scratch(dev: torch.device, nbytes: int, slot: int = 0, stream: int = None) -> torch.Tensor:
    """Transient workspace per (device, stream), grown on demand and reused (its users are ordered by that stream).
    slot: a second workspace on the same stream (AdapterPair.same_stream interleaves the sections of two sites on ONE stream).
    stream: the handle of the stream the caller is on, when it has it at hand (a torch.cuda.current_stream() lookup costs ~3 us; at the
    reference's batch of 2 clips a pair-step made 20 of them)."""
    key = (dev.index if dev.index is not None else torch.cuda.current_device(),
           stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream, slot)
    buf = _SCRATCH.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        _SCRATCH[key] = buf
    return buf


_FUSED_DX = os.environ.get("AVMOE_NO_FUSED_DX") is None      # development A/B: the token gradients as two kernels each (dX overwrites, the other site's dY adds)
_warned_side_stream = False
_SHARED_GPU = None          # process-wide override of avmoe_moe_desc.shared_gpu: None = decide per call (below), True / False = always / never


def set_shared_gpu(mode):
    """avmoe_moe_desc.shared_gpu for every site call of this process: True = always ask for the protected launches (another stream's
    kernels may be on the GPU: a second adapter site, a backbone GEMM), False = never (the caller asserts that nothing else runs
    on the GPU while adapter calls do), None (default) = per call: protected whenever the call is issued on a stream other than the
    device's default stream, and always in AdapterPair's two-stream mode.  A module attribute `shared_gpu` (True / False) overrides
    this for one site.  include/avmoe.h says which kernel families the flag protects and what it costs."""
    global _SHARED_GPU
    if mode not in (None, True, False):
        raise ValueError("set_shared_gpu: None, True or False")
    _SHARED_GPU = mode


def _shared_gpu_of(module, dev, asked):
    """The shared_gpu flag of one call: AdapterPair's explicit request, else the site's attribute, else the process-wide mode,
    else 'is this call on a side stream?' (a caller that left the default stream did so to overlap something)."""
    if asked:
        return True
    own = module.__dict__.get("shared_gpu", None)
    if own is not None:
        return bool(own)
    if _SHARED_GPU is not None:
        return _SHARED_GPU
    side = torch.cuda.current_stream(dev).cuda_stream != torch.cuda.default_stream(dev).cuda_stream
    global _warned_side_stream
    if side and not _warned_side_stream:      # said once: the protected launches change the BatchNorm summation order of some kernel families and cost residency
        _warned_side_stream = True
        import warnings
        warnings.warn("avmoe_amd: adapter call on a non-default stream -> avmoe_moe_desc.shared_gpu = 1 (CU-exclusive launches of the generalised "
                      "bottleneck-space kernels, include/avmoe.h); avmoe_amd.adapters.set_shared_gpu(False) if nothing else runs on the GPU", stacklevel=3)
    return side


RouterAux = namedtuple("RouterAux", ["z_loss", "balance_loss", "load"])
RouterAux.__doc__ = """The router auxiliary losses of one site call (`site.last_router_aux`; include/avmoe.h at avmoe_moe_forward_aux):
z_loss = mean_s logsumexp(logits_s)^2 and balance_loss = E sum_e load_e P_e, 0-d fp32 tensors with a grad_fn; load (E,), the share of
the routing slots each expert received, without gradient."""


def _publish_aux(module, aux, load):
    """site.last_router_aux of the call that just ran: the two losses as views of the autograd output `aux` (their gradients come back
    as its gradient), or None when the site ran without them."""
    if aux is None:
        module.__dict__["_last_router_aux"] = None
    else:
        z, b = aux.unbind(0)
        module.__dict__["_last_router_aux"] = RouterAux(z, b, load)


def _ws_sizes(module, L, desc):
    """(saved_bytes, scratch_bytes) of a call shape, kept on the module (two plan evaluations otherwise).  THE key of that cache: anything
    else that comes to decide a workspace size joins it here, for the forward and the backward alike.  The test hooks do: the frames per
    chunk of the N x N block size three of the plan's buffers."""
    key = (desc.S, desc.N, desc.M, desc.dtype, desc.training, desc.shared_gpu, *capi._hooks)
    cache = module.__dict__.setdefault("_ws_sizes", {})
    sizes = cache.get(key)
    if sizes is None:
        sizes = (L.avmoe_moe_saved_bytes(C.byref(desc)), L.avmoe_moe_scratch_bytes(C.byref(desc)))
        if sizes[0] == 0:
            raise capi.AvmoeError(L.avmoe_last_error().decode())
        cache[key] = sizes
    return sizes


def _mode_offset(module, L, desc):
    """Byte offset of the `mode` words in the saved workspace of a call shape (the named-buffer table, walked once per shape and kept on the
    module under _ws_sizes' key): where a Sinkhorn forward leaves its column scale."""
    key = (desc.S, desc.N, desc.M, desc.dtype, desc.training, desc.shared_gpu, *capi._hooks)
    cache = module.__dict__.setdefault("_mode_off", {})
    off = cache.get(key)
    if off is None:
        off = cache[key] = next(o for n, _r, o, _b in cm.buffer_table(L, desc) if n == "mode")
    return off


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _rate(name, v):
    """a drop rate of the mixture regularisers: a real number in [0, 1)"""
    if isinstance(v, bool) or not isinstance(v, numbers.Real) or not 0.0 <= float(v) < 1.0:
        raise ValueError(f"{name} must be a number in [0, 1), got {v!r}")
    return float(v)


# `site.last_sinkhorn`: the column scale v (E) fp32 the last Sinkhorn forward ranked with, the number of frames that took each expert (E) int32,
# and the (S) int32 bitmask of the selection (bit e: expert e took the frame) -- device tensors
SinkhornReport = namedtuple("SinkhornReport", ["scale", "count", "choice"])


def expert_choice_capacity(k, S, E):
    """c = min(S, max(1, ceil(k S / E))) of expert-choice gating with a mean of k experts per frame, evaluated exactly (Fraction(k))."""
    return min(S, max(1, math.ceil(Fraction(k) * S / E)))


# `site.last_capacity`: the capacity c of the last forward with an expert capacity (a host int), the (S) int32 bitmask of the kept pairs (bit e:
# expert e kept the frame), and per expert the number of frames that selected it and the number it kept, (E) int32 each -- device tensors
CapacityReport = namedtuple("CapacityReport", ["capacity", "kept", "demand", "kept_count"])


def router_capacity(f, k, S, E):
    """c = min(S, max(1, ceil(f k S / E))) of an expert capacity with capacity factor f behind top-k routing (GShard, Switch), evaluated
    exactly (Fraction(f), Fraction(k)): the budget of frames per expert and call."""
    return min(S, max(1, math.ceil(Fraction(f) * Fraction(k) * S / E)))


_CAPACITY_POLICIES = {"order": 0, "priority": 1}


# `site.last_top_p`: of the last top-p forward, the (S) int32 bitmask of the selection (bit e: frame s took expert e), the number of frames that
# took each expert (E) int32, and the number of frames served by j experts (E + 1) int32 -- device tensors
TopPReport = namedtuple("TopPReport", ["choice", "count", "khist"])


def _draw_mix(module, L, S, E, p, q, dev, stream):
    """The (S, E) multiplier of one training-mode call, drawn on `stream` by avmoe_mix_drop_draw into the site's cached tensor.  The site
    owns the generator's state block {seed, calls} on the device: nothing the host writes changes between two calls, so a captured
    forward draws afresh on every replay.  The block is made on the first call (a host-to-device copy: before any graph capture) and
    made anew -- calls = 0 -- when `mix_seed` is assigned or the site has moved to another device."""
    d = module.__dict__
    state = d.get("_mix_state")
    if state is None or state.device != dev:
        seed = module.mix_seed
        state = d["_mix_state"] = torch.tensor([seed - (1 << 64) if seed >= (1 << 63) else seed, 0], dtype=torch.int64, device=dev)
    buf = d.get("_mix_buf")
    if buf is None or buf.shape != (S, E) or buf.device != dev:
        buf = d["_mix_buf"] = torch.empty(S, E, dtype=torch.float32, device=dev)
    capi.check(L.avmoe_mix_drop_draw(state.data_ptr(), S, E, p, q, buf.data_ptr(), stream), "avmoe_mix_drop_draw")
    d["_mix_draws"] = d.get("_mix_draws", 0) + 1        # which draw the cached tensor holds: a backward checks that it is still its forward's
    return buf


_Routing = namedtuple("_Routing", ["choice_k", "sk_iters", "cap_f", "top_p"])      # what one call does about each selection stage; None: off


def _routing_of(module):
    """The selection stage of the call `module` is about to make, from the site's settings alone (a contradiction in them does not depend on
    the call: reported first, in eval mode too), the eval-mode rules resolved: without `router_sinkhorn_eval` an eval call routes greedily
    (S-BASE: the plain top-k call), and `router_capacity_eval_factor` stands in for the factor (None: an evaluation drops nothing, it
    should not depend on the batch).  Top-p is per frame: the same call in training and eval mode."""
    E = module.num_multimodal_experts + module.num_singlemodal_experts
    top_k, biased = module.router_top_k, module.router_select_bias is not None or module.router_select_count is not None
    choice_k, sk_iters, cap_f = module.router_expert_choice, module.router_sinkhorn, module.router_capacity_factor
    if choice_k is not None:
        if (top_k is not None and top_k < E) or biased:
            raise ValueError("router_expert_choice selects per expert: it combines with neither router_top_k in [1, E) nor router_select_bias / "
                             "router_select_count (a RouterBiasBalancer)")
        if not getattr(capi.lib(), "avmoe_site_choice", False):
            raise capi.AvmoeError("this libavmoe_hip.so predates avmoe_moe_forward_choice / avmoe_expert_choice: it serves no expert-choice gating")
    if sk_iters is not None:
        if top_k is None or not 1 <= top_k < E:
            raise ValueError(f"router_sinkhorn balances a top-k selection: it needs router_top_k in [1, {E}), got {top_k!r}")
        if choice_k is not None or biased:
            raise ValueError("router_sinkhorn balances within the call: it combines with neither router_select_bias / router_select_count "
                             "(a RouterBiasBalancer) nor router_expert_choice")
        if not getattr(capi.lib(), "avmoe_site_sinkhorn", False):
            raise capi.AvmoeError("this libavmoe_hip.so predates avmoe_moe_forward_sinkhorn / avmoe_router_sinkhorn: it serves no Sinkhorn routing")
    if cap_f is not None:
        if top_k is None or not 1 <= top_k < E:
            raise ValueError(f"router_capacity_factor bounds the frames of a top-k selection: it needs router_top_k in [1, {E}), "
                             f"got {top_k!r}")
        if choice_k is not None:
            raise ValueError("router_capacity_factor does not combine with router_expert_choice: expert choice already gives every expert "
                             "exactly its share of the frames")
        if sk_iters is not None:
            raise ValueError("router_capacity_factor does not combine with router_sinkhorn: a capacity acts on the plain (or biased) top-k "
                             "selection, not on one balanced within the call")
        if not getattr(capi.lib(), "avmoe_site_capacity", False):
            raise capi.AvmoeError("this libavmoe_hip.so predates avmoe_moe_forward_capacity / avmoe_router_capacity: it serves no expert capacity")
    top_p = module.router_top_p
    if top_p is not None:
        if choice_k is not None:
            raise ValueError("router_top_p does not combine with router_expert_choice: there each expert picks its frames, here each frame "
                             "picks as many experts as reach the mass p")
        if sk_iters is not None:
            raise ValueError("router_top_p does not combine with router_sinkhorn: Sinkhorn balances a selection of exactly k experts per frame, "
                             "top-p lets the number of experts vary")
        if cap_f is not None:
            raise ValueError("router_top_p does not combine with router_capacity_factor: the budget c = ceil(f k S / E) needs a fixed number "
                             "of experts per frame")
        if biased:
            raise ValueError("router_top_p does not combine with router_select_bias / router_select_count (a RouterBiasBalancer): a bias on "
                             "the ranking would change which probabilities the running mass adds up")
        if not 1 <= module.router_top_p_min_k <= (top_k if (top_k is not None and 1 <= top_k < E) else E):
            raise ValueError(f"router_top_p_min_k {module.router_top_p_min_k} must lie in [1, k_max], k_max = router_top_k in [1, {E}) or else {E}")
        if E < 2:
            raise ValueError("router_top_p needs at least two experts")
        if not getattr(capi.lib(), "avmoe_site_top_p", False):
            raise capi.AvmoeError("this libavmoe_hip.so predates avmoe_moe_forward_top_p / avmoe_router_top_p: it serves no top-p routing")
    if not module.training:
        sk_iters = sk_iters if module.router_sinkhorn_eval else None
        cap_f = module.router_capacity_eval_factor if cap_f is not None else None
    return _Routing(choice_k, sk_iters, cap_f, top_p)


def _site_forward(module, X, Y, noise, names, params, add_to=None, shared_gpu=None, stream=None):
    """One avmoe_moe_forward_aux call: every site goes through it, with top_k = 0 for a dense one and aux = NULL without the auxiliary
    losses -- or, in training mode with `drop_path` / `expert_dropout` on, the draw of the multiplier and one avmoe_moe_forward_reg call;
    or, with `router_select_bias` / `router_select_count` set, one avmoe_moe_forward_bias call (which takes the multiplier too);
    or, with `router_expert_choice` set, one avmoe_moe_forward_choice call (which takes the multiplier too), in training and eval mode alike;
    or, with `router_sinkhorn` set, one avmoe_moe_forward_sinkhorn call (which takes the multiplier too);
    or, with `router_capacity_factor` set, one avmoe_moe_forward_capacity call (which takes the multiplier, the selection bias and the
    counts too) -- the last two in eval mode by the rules of _routing_of, else the call the site makes without them;
    or, with `router_top_p` set, one avmoe_moe_forward_top_p call (which takes the multiplier too), in training and eval mode alike.
    Returns (out, probs, idx, lb, state, aux) with state = what the backward needs and aux = None or ((2,) [z, balance], load (E,)):
    the router auxiliary losses of a site with `router_aux` on.
    add_to: a contiguous tensor like X that receives `+= adapter(X, Y)` in place (avmoe_moe_desc.accumulate_out) and is
    returned as `out`.  shared_gpu: True = another stream's kernels may run beside this call (AdapterPair); None = _shared_gpu_of.
    stream: the handle (int) of the CURRENT stream when the caller already has it (AdapterPair), else looked up."""
    choice_k, sk_iters, cap_f, top_p = _routing_of(module)
    if not (X.is_cuda and Y.is_cuda):
        raise capi.AvmoeError("avmoe_amd runs on MI355X only: tensors must live on a GPU (no CPU fallback)")
    if stream is None:
        stream = torch.cuda.current_stream(X.device).cuda_stream
    if X.dtype != Y.dtype or X.dtype not in (torch.float32, torch.bfloat16):
        raise capi.AvmoeError(f"activations must both be float32 or bfloat16, got {X.dtype} / {Y.dtype}")
    L = capi.lib()
    X = X.contiguous()
    Y = Y.contiguous()
    S, N, Cc = X.shape
    desc = module._desc(S, N, Y.shape[1], X.dtype == torch.bfloat16)
    shared_gpu = _shared_gpu_of(module, X.device, shared_gpu)
    desc.shared_gpu = int(shared_gpu)                     # (include/avmoe.h: kernels of another stream may be on the GPU during this call and its backward)
    keep = module._attention_keep(S, N, X.device)
    ptrs = module._fill_ptrs(params, keep, names=names, device=X.device)
    E = module.num_multimodal_experts + module.num_singlemodal_experts
    top_k = module.router_top_k
    k = top_k if (top_k is not None and top_k < E) else 0      # 0: the dense mixture (k >= E is the dense mixture too)
    renorm = int(module.router_top_k_renorm) if k else 1       # (a dense site records renorm = 1 in `saved`, as avmoe_moe_forward does)
    if not L.avmoe_site_aux and (k or module.router_aux):
        raise capi.AvmoeError("this libavmoe_hip.so predates avmoe_moe_forward_aux: it serves neither top-k gating nor the router auxiliary losses")
    drop_p, drop_q = module.drop_path, module.expert_dropout
    reg = bool(module.training and (drop_p > 0.0 or drop_q > 0.0))      # (eval mode ignores both settings)
    if reg and not getattr(L, "avmoe_site_reg", False):
        raise capi.AvmoeError("this libavmoe_hip.so predates avmoe_moe_forward_reg / avmoe_mix_drop_draw: it serves neither drop_path nor expert_dropout")
    # aux-loss-free balancing (avmoe_amd.train.RouterBiasBalancer; include/avmoe.h at avmoe_moe_forward_bias): the bias on the selection,
    # and -- in training mode only -- the tensor the selection counts are added to.  Eval mode applies the bias and counts nothing.
    sel_bias = module.router_select_bias
    sel_count = module.router_select_count if module.training else None
    if sel_bias is not None and not k:
        raise ValueError("router_select_bias needs top-k gating (router_top_k in [1, E)): a dense mixture has no selection")
    for what, t_ in (("router_select_bias", sel_bias), ("router_select_count", sel_count)):
        if t_ is not None and not (torch.is_tensor(t_) and t_.dtype == torch.float32 and t_.device == X.device and t_.numel() == E and t_.is_contiguous()):
            raise ValueError(f"{what} must be a contiguous float32 tensor of {E} elements on the tokens' device")
    biased = sel_bias is not None or sel_count is not None
    if biased and not getattr(L, "avmoe_site_bias", False):
        raise capi.AvmoeError("this libavmoe_hip.so predates avmoe_moe_forward_bias / avmoe_router_bias_update: it serves no router selection bias")
    # expert-choice gating (include/avmoe.h at avmoe_moe_forward_choice): each expert takes its c frames, c from the mean number of
    # experts per frame -- exactly, in rationals --; a function of S alone, so a captured call keeps its capacity
    capacity, choice = 0, None
    if choice_k is not None:
        capacity = expert_choice_capacity(choice_k, S, E)
        choice = torch.empty(S, device=X.device, dtype=torch.int32)
    module.__dict__["_last_expert_choice"] = choice
    # Sinkhorn-balanced top-k (include/avmoe.h at avmoe_moe_forward_sinkhorn): the reports of the call's actual selection
    sk_choice = sk_count = None
    if sk_iters is not None:
        sk_choice = torch.empty(S, device=X.device, dtype=torch.int32)
        sk_count = torch.empty(E, device=X.device, dtype=torch.int32)
    module.__dict__["_last_sinkhorn"] = None
    # expert capacity (include/avmoe.h at avmoe_moe_forward_capacity): c from the factor -- exactly, in rationals; a function of S alone, so a
    # captured call keeps its capacity --, the multiplier for the backward (this call's own tensor) and the reports
    cap_c, cap_scale, cap_rep = 0, None, None
    if cap_f is not None:
        cap_c = router_capacity(cap_f, k, S, E)
        cap_scale = torch.empty(S, E, device=X.device, dtype=torch.float32)
        cap_rep = CapacityReport(cap_c, torch.empty(S, device=X.device, dtype=torch.int32), torch.empty(E, device=X.device, dtype=torch.int32),
                                 torch.empty(E, device=X.device, dtype=torch.int32))
    module.__dict__["_last_capacity"] = cap_rep
    # top-p routing (include/avmoe.h at avmoe_moe_forward_top_p): k_max is the site's top_k, the reports are this call's own tensors
    tp_rep = None
    if top_p is not None:
        tp_rep = TopPReport(torch.empty(S, device=X.device, dtype=torch.int32), torch.empty(E, device=X.device, dtype=torch.int32),
                            torch.empty(E + 1, device=X.device, dtype=torch.int32))
    module.__dict__["_last_top_p"] = tp_rep
    sizes = _ws_sizes(module, L, desc)
    saved = torch.empty(sizes[0], dtype=torch.uint8, device=X.device)
    scratch = _scratch(X.device, sizes[1], stream=stream)
    if add_to is not None:
        if add_to.shape != X.shape or add_to.dtype != X.dtype or not add_to.is_contiguous() or add_to.device != X.device:
            raise capi.AvmoeError("add_to must be a contiguous tensor with the shape, dtype and device of the tokens")
        out, desc.accumulate_out = add_to, 1
    else:
        out = torch.empty_like(X)
    probs = torch.empty(S, E, device=X.device, dtype=torch.float32)
    idx = torch.empty(S, device=X.device, dtype=torch.int64)
    lb = torch.empty((), device=X.device, dtype=torch.float32)      # always written by the router's kernels (0 without the LB loss)
    if noise is not None:
        noise = noise.to(torch.float32).contiguous()
    aux = None
    if module.router_aux:                                # the router auxiliary losses beside the forward (dense or top-k)
        aux = (torch.empty(2, device=X.device, dtype=torch.float32), torch.empty(E, device=X.device, dtype=torch.float32))
    mix = _draw_mix(module, L, S, E, drop_p, drop_q, X.device, stream) if reg else None
    module.__dict__["_mix_last"] = mix
    head = (C.byref(desc), X.data_ptr(), Y.data_ptr(), C.byref(ptrs), _ptr(noise))
    outs = (out.data_ptr(), probs.data_ptr(), idx.data_ptr(), lb.data_ptr(), aux[0].data_ptr() if aux else None, aux[1].data_ptr() if aux else None)
    ws = (saved.data_ptr(), scratch.data_ptr(), stream)
    if choice is not None:                               # expert choice (and the multiplier, when one was drawn)
        fn, args = "avmoe_moe_forward_choice", (capacity, int(module.router_expert_choice_renorm), _ptr(mix), *outs, choice.data_ptr())
    elif sk_iters is not None:                           # Sinkhorn-balanced top-k (and the multiplier, when one was drawn)
        fn, args = "avmoe_moe_forward_sinkhorn", (k, renorm, sk_iters, _ptr(mix), *outs, sk_choice.data_ptr(), sk_count.data_ptr())
    elif cap_f is not None:                              # expert capacity behind top-k (and the multiplier, the bias, the counts)
        fn, args = "avmoe_moe_forward_capacity", (k, renorm, _ptr(mix), _ptr(sel_bias), _ptr(sel_count), cap_c,
                                                  _CAPACITY_POLICIES[module.router_capacity_policy], cap_scale.data_ptr(), cap_rep.kept.data_ptr(),
                                                  cap_rep.demand.data_ptr(), cap_rep.kept_count.data_ptr(), *outs)
    elif top_p is not None:                              # top-p: k_max = the site's k, or E (and the multiplier, when one was drawn)
        fn, args = "avmoe_moe_forward_top_p", (top_p, module.router_top_p_min_k, k if k else E, int(module.router_top_k_renorm), _ptr(mix), *outs,
                                               tp_rep.choice.data_ptr(), tp_rep.count.data_ptr(), tp_rep.khist.data_ptr())
    elif biased:                                         # the selection bias / counts (and the multiplier, when one was drawn)
        fn, args = "avmoe_moe_forward_bias", (k, renorm, _ptr(mix), _ptr(sel_bias), _ptr(sel_count), *outs)
    elif mix is not None:                                # the multiplier on the mixture weights, drawn just above on the same stream
        fn, args = "avmoe_moe_forward_reg", (k, renorm, mix.data_ptr(), *outs)
    elif L.avmoe_site_aux:
        fn, args = "avmoe_moe_forward_aux", (k, renorm, *outs)
    else:                                                # a library from before the _aux entry points (AVMOE_LIB): the plain site, the one second path
        fn, args = "avmoe_moe_forward", outs[:4]
    st = getattr(L, fn)(*head, *args, *ws)
    desc.accumulate_out = 0
    capi.check(st, fn)
    if sk_iters is not None:                              # the scale the call used: a copy of its E words in `saved` (no sync; `saved` is not kept alive)
        off = _mode_offset(module, L, desc) + 4 * 16      # (csrc/kernels.h: MODE_SELECT_WORDS = 16, the bits of the column scale)
        module.__dict__["_last_sinkhorn"] = SinkhornReport(saved[off:off + 4 * E].view(torch.float32).clone(), sk_count, sk_choice)
    if cap_rep is not None and module.training:           # avmoe_amd.train.CapacityMeter: two adds on this stream, no sync
        for meter in module.__dict__.get("_capacity_meters", ()):
            meter.update(module, cap_rep)
    if tp_rep is not None:                                # avmoe_amd.train.TopPMeter: two adds on this stream, no sync
        for meter in module.__dict__.get("_top_p_meters", ()):
            meter.update(module, tp_rep)
    if module.__dict__.get("_keep_saved"):                # avmoe_amd.debug.keep_saved: checker-side view of the last call's workspace
        module.__dict__["_last_saved"] = (desc, saved)
    if cap_scale is not None:                            # the backward's multiplier is this call's own cap_scale (it holds the draw too): no draw number
        mix = (cap_scale, None)
    else:
        mix = (mix, module.__dict__["_mix_draws"]) if mix is not None else None      # (the tensor is the site's cached one: with its draw number)
    return out, probs, idx, lb, ((desc, keep, ptrs, mix), saved, X, Y), aux


class _SiteBackward:
    """One site's backward through the C ABI, writing (or, with acc_*, adding) the token gradients into dX / dY.
    run(0) = the whole of it; run(mask) = the sections of avmoe_moe_backward_aux / _part (1: touches neither dX nor dY, 2: every
    writer of dX, 4: every writer of dY), in this order.  finish() returns the parameter gradients in `names` order (None where not needed,
    or for all of them when a gradient sink took them)."""

    def __init__(self, module, state, names, params, needs, d_out, d_lb, dX, dY, acc_dx=False, acc_dy=False, scratch_slot=0, stream=None,
                 d_probs=None, d_aux=None):
        self.L = capi.lib()
        (desc, keep, fwd_ptrs, mix), self.saved, self.X, self.Y = state
        self.mix = None                                  # the forward's multiplier on the mixture weights (drop_path / expert_dropout), given again
        if mix is not None:
            if mix[1] is not None and module.__dict__.get("_mix_draws") != mix[1]:
                raise capi.AvmoeError("drop_path / expert_dropout: the site ran another training forward before this one's backward, and the "
                                      "site's one multiplier tensor now holds that call's draw (run each forward's backward before the next forward)")
            self.mix = mix[0]
        self.desc, self.names, self.module = desc, names, module
        self.stream = stream if stream is not None else torch.cuda.current_stream(self.X.device).cuda_stream      # (the stream this object is built AND run on)
        tensors = dict(zip(names, params))
        # the forward's pointer struct, as long as it was built from these very parameters (autograd's saved-tensor version checks -- or, with an
        # anchor parameter, the pair's own stamp -- refuse a backward on anything else); "v1" sites rebuild (their struct carries dropout draws)
        self.ptrs = fwd_ptrs if (fwd_ptrs is not None and not keep) else module._fill_ptrs(params, keep)
        # Parameter gradients.  With a gradient sink attached (avmoe_amd.dp.AdapterGradReducer(sites=...)) the kernels
        # write straight into the reducer's flat bucket -- `param.grad` are views of it -- and autograd gets None: no
        # per-parameter accumulation kernels.  Otherwise: fresh tensors, accumulated by autograd as usual.
        sink = self.sink = getattr(module, "_grad_sink", None)
        self.use_sink = sink is not None and all(needs) and sink.matches(names, tensors)
        filler = module._site_cache()["fill_p"]
        if self.use_sink:
            # zeros, not empty: on accumulation micro-steps the alignment padding is added to the bucket as well
            self.flat = sink.flat if sink.fresh else torch.zeros_like(sink.flat)
            self.grads = None                            # the kernels write at flat + offset: no per-parameter views needed
            hit = module.__dict__.get("_gptrs_cache")     # the struct of the last call, as long as the sink's memory is the same
            if hit is not None and hit[0] == (self.flat.data_ptr(), id(sink)):
                self.gptrs = hit[1]
            else:
                self.gptrs = filler.fill(cm.MoePtrs(), None, base_ptr=self.flat.data_ptr(), offsets=sink.offsets)
                module.__dict__["_gptrs_cache"] = ((self.flat.data_ptr(), id(sink)), self.gptrs)
        else:
            self.gptrs = cm.MoePtrs()
            self.grads = {k: (torch.empty_like(v) if needs[i] else None) for i, (k, v) in enumerate(tensors.items())}
            filler.fill(self.gptrs, [self.grads[k] for k in names])
        # d_out None: out got no gradient -> the router-only backward (dOut = NULL, whole: run(0) only)
        self.d_out = d_out.to(self.X.dtype).contiguous() if d_out is not None else None
        self.dprobs = d_probs.to(torch.float32).reshape(desc.S, -1).contiguous() if d_probs is not None else None
        self.lbg = d_lb.to(torch.float32).reshape(1).contiguous() if (d_lb is not None and desc.lb_loss) else None
        self.daux = d_aux.to(torch.float32).reshape(2).contiguous() if d_aux is not None else None      # [g_z, g_balance]
        if not self.L.avmoe_site_aux and (self.d_out is None or self.dprobs is not None or self.daux is not None):
            raise capi.AvmoeError("this libavmoe_hip.so predates avmoe_moe_backward_aux: it serves neither a gradient for probs or the router "
                                  "auxiliary losses nor a backward without a gradient for out")
        self.scratch = _scratch(self.X.device, _ws_sizes(module, self.L, desc)[1], scratch_slot, stream=self.stream)
        self.dX, self.dY, self.acc = dX, dY, (int(acc_dx), int(acc_dy))

    def run(self, parts=0):
        d = self.desc
        d.accumulate_dx, d.accumulate_dy = self.acc
        if self.mix is not None:
            fn = "avmoe_moe_backward_reg"
            st = self.L.avmoe_moe_backward_reg(C.byref(d), self.X.data_ptr(), self.Y.data_ptr(), C.byref(self.ptrs), _ptr(self.d_out),
                                               _ptr(self.dprobs), _ptr(self.lbg), _ptr(self.daux), self.mix.data_ptr(), self.saved.data_ptr(),
                                               self.scratch.data_ptr(), self.dX.data_ptr(), self.dY.data_ptr(), C.byref(self.gptrs),
                                               int(parts), self.stream)
        elif self.L.avmoe_site_aux:                            # NULL for each upstream gradient that is absent
            fn = "avmoe_moe_backward_aux"
            st = self.L.avmoe_moe_backward_aux(C.byref(d), self.X.data_ptr(), self.Y.data_ptr(), C.byref(self.ptrs), _ptr(self.d_out),
                                               _ptr(self.dprobs), _ptr(self.lbg), _ptr(self.daux), self.saved.data_ptr(),
                                               self.scratch.data_ptr(), self.dX.data_ptr(), self.dY.data_ptr(), C.byref(self.gptrs),
                                               int(parts), self.stream)
        else:                                                  # (a library from before the _aux entry points: __init__ has refused what it cannot serve)
            fn = "avmoe_moe_backward_part"
            st = self.L.avmoe_moe_backward_part(C.byref(d), self.X.data_ptr(), self.Y.data_ptr(), C.byref(self.ptrs), self.d_out.data_ptr(),
                                                _ptr(self.lbg), self.saved.data_ptr(), self.scratch.data_ptr(), self.dX.data_ptr(),
                                                self.dY.data_ptr(), C.byref(self.gptrs), int(parts), self.stream)
        d.accumulate_dx = d.accumulate_dy = 0
        capi.check(st, fn)
        return self

    def fused_ok(self, other):
        """Does the library serve `token gradient = this site's dX + the other site's dY` as ONE kernel (avmoe_moe_backward_dx_dy)?
        (asked once per pair of call shapes and test-hook state: the answer is a function of the two plans)"""
        da, db = self.desc, other.desc
        key = (id(other.module), da.S, da.N, da.M, da.dtype, da.training, db.S, db.N, db.M, db.dtype, db.training, *capi._hooks)
        cache = self.module.__dict__.setdefault("_fused_ok", {})
        ok = cache.get(key)
        if ok is None:
            # (a library older than ABI 10 loaded through AVMOE_LIB lacks the entry point: the two-kernel hand-over then)
            ok = cache[key] = hasattr(self.L, "avmoe_moe_backward_dx_dy") and \
                self.L.avmoe_moe_backward_dx_dy(C.byref(da), None, None, None, C.byref(db), None, None, None, None) == 0
        return ok

    def run_fused(self, other):
        """dX (this site) + dY (the other site) written once into self.dX: after sections 1 + 32 + 8 of both sites, in place of this
        site's section 64 and the other site's section 16; the current stream must be ordered behind the other site's section 8."""
        st = self.L.avmoe_moe_backward_dx_dy(C.byref(self.desc), self.X.data_ptr(), self.saved.data_ptr(), self.scratch.data_ptr(),
                                             C.byref(other.desc), other.saved.data_ptr(), other.scratch.data_ptr(), self.dX.data_ptr(), self.stream)
        capi.check(st, "avmoe_moe_backward_dx_dy")
        return self

    def finish_needs_stream(self):
        """does finish() issue a torch op (which runs on the CURRENT stream)?"""
        return self.sink is not None and ((self.use_sink and not self.sink.fresh) or (not self.use_sink and self.sink.stale))

    def finish(self):
        sink = self.sink
        if self.use_sink:
            if not sink.fresh:
                sink.flat.add_(self.flat)                # accumulation micro-step: one fused add for the whole site
            sink.done()
            return (None,) * len(self.names)
        if sink is not None:
            # a sink is attached but this backward did not go through it (a parameter frozen after the reducer was built, a layout
            # mismatch): autograd ADDS the tensors returned below into param.grad -- views of the sink's slice.  After a lazy zero_grad
            # the slice still holds the previous step's values: zero it first, and take it out of the `stale` state so that the
            # reducer's finish() does not wipe what autograd is about to add
            if sink.stale:
                sink.flat.zero_()
            sink.stale = False
            sink.fresh = False
            sink.calls -= 1
        return tuple(self.grads[k] for k in self.names)


def _site_backward(module, state, names, params, needs, d_out, d_lb, dX, dY, acc_dx=False, acc_dy=False, d_probs=None, d_aux=None):
    """The whole backward of one site in one call (see _SiteBackward)."""
    return _SiteBackward(module, state, names, params, needs, d_out, d_lb, dX, dY, acc_dx, acc_dy, d_probs=d_probs, d_aux=d_aux).run(0).finish()


class AdapterFunction(torch.autograd.Function):
    """out, probs, idx, lb, aux, load = f(X, Y, noise, *params) on token-major X:(S,N,C), Y:(S,M,Cy); aux = [z, balance] and load: the
    router auxiliary losses of a site with `router_aux` on, else None."""

    @staticmethod
    def forward(ctx, module, X, Y, noise, names, *params):
        out, probs, idx, lb, state, aux = _site_forward(module, X, Y, noise, names, params)
        aux, load = aux if aux is not None else (None, None)
        ctx.set_materialize_grads(False)                 # no zero tensors (= fill kernels) for the gradients of probs / idx / lb nobody sent
        ctx.module, ctx.names, ctx.state = module, names, state[:2]
        sink = getattr(module, "_grad_sink", None)
        if sink is not None and any(ctx.needs_input_grad[5:]):
            sink.calls += 1                              # the site's bucket is complete after as many backward calls
        ctx.save_for_backward(state[2], state[3], *params)
        ctx.mark_non_differentiable(idx)                 # probs is differentiable, as in the reference (F.softmax of the router logits)
        if load is not None:
            ctx.mark_non_differentiable(load)
        return out, probs, idx, lb, aux, load

    @staticmethod
    def backward(ctx, d_out, d_probs, _d_idx, d_lb, d_aux=None, _d_load=None):
        X, Y, *params = ctx.saved_tensors
        # d_out None (only probs, the load-balancing loss and / or the router auxiliary losses were differentiated): the router-only backward
        dX, dY = torch.empty_like(X), torch.empty_like(Y)
        pg = _site_backward(ctx.module, (*ctx.state, X, Y), ctx.names, params, ctx.needs_input_grad[5:], d_out, d_lb, dX, dY,
                            d_probs=d_probs, d_aux=d_aux)
        return (None, dX, dY, None, None) + pg


class _PairFunction(torch.autograd.Function):
    """Both adapter sites of one backbone layer (net_trans_v3.py:695-698): site A adapts the tokens Xa with Xb as the other
    modality, site B adapts Xb with Xa.  Each token tensor therefore receives two gradients (as X of one site and as Y of
    the other); the second one is ADDED inside the GEMM epilogues (avmoe_moe_desc.accumulate_*), so no separate
    accumulation pass over the token gradients runs."""

    @staticmethod
    def forward(ctx, site_a, site_b, side, Xa, Xb, base_a, base_b, names_a, names_b, noises, *params):
        """side: the second HIP stream (two-stream mode) or None (both sites on the caller's stream).
        base_a / base_b: None, or the residual streams that take `+= adapter output` in place (returned as the outputs).
        noises: (noise_a, noise_b) -- the AVS logit noise of the two sites, (S, E) already scaled, or None each.
        params: every parameter of the two sites -- or, with gradient sinks on both (`lean`, AdapterPair.forward), ONE anchor
        parameter: the sinks take the gradients, autograd only has to know that the outputs depend on something trainable."""
        na = len(names_a)
        ctx.lean = len(params) == 1 and na > 1
        if ctx.lean:
            pa, pb = tuple(site_a._param_tensors().values()), tuple(site_b._param_tensors().values())
            # autograd's saved-tensor checks see the anchor only: remember which memory and which version every other parameter
            # had, the backward re-fetches them by name and refuses to run on anything else
            ctx.pstamp = tuple((t.data_ptr(), t._version) for t in pa + pb)
        else:
            pa, pb = params[:na], params[na:]
        Xa, Xb = Xa.contiguous(), Xb.contiguous()
        main = torch.cuda.current_stream(Xa.device)
        side, ctx.events = (side[0], side[1:]) if isinstance(side, tuple) else (side, None)
        # fork / join through the pair's OWN events, made once and re-recorded every step (Stream.wait_stream makes and destroys an
        # event per call, and destroying an event that is still pending blocks the host until the GPU reaches it: the host then never
        # runs ahead of the GPU across a step boundary -- measured: 167 us of GPU idle time per cfg-2 step)
        def fork(ev):
            ev.record(main); side.wait_event(ev)
        def join(ev):
            ev.record(side); main.wait_event(ev)
        if side is not None:                           # site B on the side stream, concurrently with site A
            ctx_ev = ctx.events if ctx.events else tuple(torch.cuda.Event() for _ in range(6))
            fork(ctx_ev[2])
            two = side.cuda_stream != main.cuda_stream      # (same_stream: the schedule of the two-stream mode on one stream -- nothing overlaps)
            with torch.cuda.stream(side):
                out_b, pr_b, idx_b, lb_b, st_b, ax_b = _site_forward(site_b, Xb, Xa, noises[1], names_b, pb, add_to=base_b, shared_gpu=two, stream=side.cuda_stream)
            out_a, pr_a, idx_a, lb_a, st_a, ax_a = _site_forward(site_a, Xa, Xb, noises[0], names_a, pa, add_to=base_a, shared_gpu=two, stream=main.cuda_stream)
            join(ctx_ev[3])
            for t_ in (out_b, idx_b, pr_b, lb_b, st_b[1]) + (ax_b if ax_b is not None else ()):
                t_.record_stream(main)
            if site_b.last_expert_choice is not None:    # (made on the side stream like the outputs above)
                site_b.last_expert_choice.record_stream(main)
            if site_b.last_sinkhorn is not None:
                for t_ in site_b.last_sinkhorn:
                    t_.record_stream(main)
            if site_b.last_top_p is not None:
                for t_ in site_b.last_top_p:
                    t_.record_stream(main)
            if site_b.last_capacity is not None:         # (and the backward's multiplier of such a call)
                for t_ in site_b.last_capacity[1:] + (st_b[0][3][0],):
                    t_.record_stream(main)
        else:
            out_a, pr_a, idx_a, lb_a, st_a, ax_a = _site_forward(site_a, Xa, Xb, noises[0], names_a, pa, add_to=base_a, stream=main.cuda_stream)
            out_b, pr_b, idx_b, lb_b, st_b, ax_b = _site_forward(site_b, st_a[3], st_a[2], noises[1], names_b, pb, add_to=base_b, stream=main.cuda_stream)
        (ax_a, ld_a), (ax_b, ld_b) = (ax_a if ax_a is not None else (None, None)), (ax_b if ax_b is not None else (None, None))
        dirty = [t for t in (base_a, base_b) if t is not None]
        if dirty:
            ctx.mark_dirty(*dirty)
        ctx.has_base = (base_a is not None, base_b is not None)
        ctx.set_materialize_grads(False)                 # no zero tensors (= fill kernels) for the gradients of the index outputs
        ctx.side = side
        ctx.sites, ctx.names, ctx.states = (site_a, site_b), (names_a, names_b), (st_a[:2], st_b[:2])
        needs_ab = ((True,), (True,)) if ctx.lean else (ctx.needs_input_grad[10:10 + na], ctx.needs_input_grad[10 + na:])
        for site, needs in ((site_a, needs_ab[0]), (site_b, needs_ab[1])):
            sink = getattr(site, "_grad_sink", None)
            if sink is not None and any(needs) and (not ctx.lean or ctx.needs_input_grad[10]):
                sink.calls += 1
        ctx.save_for_backward(st_a[2], st_a[3], *params)
        ctx.mark_non_differentiable(idx_a, idx_b, *(t_ for t_ in (ld_a, ld_b) if t_ is not None))       # the probabilities are differentiable, as in the reference
        return out_a, out_b, idx_a, idx_b, pr_a, pr_b, lb_a, lb_b, ax_a, ax_b, ld_a, ld_b

    @staticmethod
    def backward(ctx, d_a, d_b, _ia, _ib, dp_a, dp_b, d_lba, d_lbb, dx_a=None, dx_b=None, _dla=None, _dlb=None):
        Xa, Xb, *params = ctx.saved_tensors
        router_only = d_a is None and d_b is None        # neither output got a gradient: the router-only backward for both sites
        if not router_only:                              # (one output without: zeros for it -- the sections and the fused dX + dY path
            d_a = torch.zeros_like(Xa) if d_a is None else d_a      # assume a full backward of both sites)
            d_b = torch.zeros_like(Xb) if d_b is None else d_b
        (site_a, site_b), (names_a, names_b) = ctx.sites, ctx.names
        na = len(names_a)
        gXa, gXb = torch.empty_like(Xa), torch.empty_like(Xb)
        if ctx.lean:                                       # the sinks take every parameter gradient; autograd gets None for the anchor
            if getattr(site_a, "_grad_sink", None) is None or getattr(site_b, "_grad_sink", None) is None:
                raise capi.AvmoeError("AdapterPair: the gradient sink of a site was detached between its forward and its backward")
            params = tuple(site_a._param_tensors().values()) + tuple(site_b._param_tensors().values())
            if tuple((t.data_ptr(), t._version) for t in params) != ctx.pstamp:
                raise capi.AvmoeError("AdapterPair: a parameter of the pair was replaced or modified in place between the forward and "
                                      "its backward (optimizer step / load_state_dict between micro-steps, or a retained graph)")
            needs_a, needs_b = (True,) * na, (True,) * len(names_b)
        else:
            needs_a, needs_b = ctx.needs_input_grad[10:10 + na], ctx.needs_input_grad[10 + na:]
        gba = d_a if ctx.has_base[0] else None            # out = base + adapter(...): the residual stream passes the gradient on
        gbb = d_b if ctx.has_base[1] else None
        if router_only:                                   # both sites on the caller's stream, one after the other: A overwrites, B adds
            pga = _site_backward(site_a, (*ctx.states[0], Xa, Xb), names_a, params[:na], needs_a, None, d_lba, gXa, gXb, d_probs=dp_a, d_aux=dx_a)
            pgb = _site_backward(site_b, (*ctx.states[1], Xb, Xa), names_b, params[na:], needs_b, None, d_lbb, gXb, gXa, acc_dx=True,
                                 acc_dy=True, d_probs=dp_b, d_aux=dx_b)
            return (None, None, None, gXa, gXb, gba, gbb, None, None, None) + ((None,) if ctx.lean else pga + pgb)
        if ctx.side is not None:
            # Two streams, cross-ordered hand-over: ONE buffer per token tensor, no add kernel.  Each site OVERWRITES its own token
            # gradient with its dX (section 2) and ADDS its dY to the other tensor's buffer (section 16) once the other site's dX is
            # there -- both sites run sections 1, 2 and 8 (everything but the GEMM that writes dY) without waiting for each other; only
            # the two dY GEMMs are ordered behind the events.  (Measured on MI355X at cfg-2, round 2: 5.79 ms per step against 5.97 for
            # two buffers + a fused add and 6.04 / 6.06 for the variants that serialise one site's tail behind the other -- dropped.)
            side, main = ctx.side, torch.cuda.current_stream(Xa.device)
            ev_a, ev_b, ev_fork, ev_join, ev_a6, ev_b6 = ctx.events if ctx.events else tuple(torch.cuda.Event() for _ in range(6))
            ev_fork.record(main); side.wait_event(ev_fork)
            slot_b = 1 if side.cuda_stream == main.cuda_stream else 0      # (same_stream: the two sites' sections interleave on ONE stream)
            with torch.cuda.stream(side):
                cbk = _SiteBackward(site_b, (*ctx.states[1], Xb, Xa), names_b, params[na:], needs_b, d_b, d_lbb, gXb, gXa, acc_dx=False, acc_dy=True,
                                    scratch_slot=slot_b, stream=side.cuda_stream, d_probs=dp_b, d_aux=dx_b)
            cak = _SiteBackward(site_a, (*ctx.states[0], Xa, Xb), names_a, params[:na], needs_a, d_a, d_lba, gXa, gXb, acc_dx=False, acc_dy=True,
                                stream=main.cuda_stream, d_probs=dp_a, d_aux=dx_a)
            # Round 5: where the library serves it (avmoe_moe_backward_dx_dy: the tuned bf16 shapes), a token gradient is written ONCE -- the
            # dX product of its own site with the other site's dY product folded in as two more contraction segments -- instead of
            # overwritten by one site and read back + added by the other.  That product moves to the END of its site's backward (it
            # needs the other site's hop-1 chain, section 8); decided per tensor.
            fuse_a = _FUSED_DX and cak.fused_ok(cbk)     # gXa = A's dX + B's dY
            fuse_b = _FUSED_DX and cbk.fused_ok(cak)     # gXb = B's dX + A's dY
            # (the backward objects carry their stream's handle: their C calls need no stream context around them)
            cbk.run(1 | 32 if fuse_b else 3)
            if not fuse_b:
                ev_b.record(side)                        # gXb holds site B's dX
            cbk.run(8)                                   # the hop-1 chain up to (not including) the GEMM that writes dY
            ev_b6.record(side)
            cak.run(1 | 32 if fuse_a else 3)
            if not fuse_a:
                ev_a.record(main)                        # gXa holds site A's dX
            cak.run(8)
            ev_a6.record(main)
            if fuse_b:
                side.wait_event(ev_a6)
                cbk.run_fused(cak)                       # gXb complete
            if not fuse_a:
                side.wait_event(ev_a)                    # gXa holds site A's dX
                cbk.run(16)                              # += site B's dY
            if cbk.finish_needs_stream():
                with torch.cuda.stream(side):            # (an accumulation micro-step adds its bucket with a torch op: on the site's stream)
                    pgb = cbk.finish()
            else:
                pgb = cbk.finish()
            if fuse_a:
                main.wait_event(ev_b6)
                cak.run_fused(cbk)                       # gXa complete
            if not fuse_b:
                main.wait_event(ev_b)                    # gXb holds site B's dX
                cak.run(16)
            pga = cak.finish()
            ev_join.record(side); main.wait_event(ev_join)
            for t_ in tuple(g_ for g_ in pgb if g_ is not None) + (cbk.d_out,) + tuple(g_ for g_ in (cbk.dprobs, cbk.daux) if g_ is not None):
                t_.record_stream(main)
            gXa.record_stream(side); gXb.record_stream(side)
            return (None, None, None, gXa, gXb, gba, gbb, None, None, None) + ((None,) if ctx.lean else pga + pgb)
        # One stream: both sites add into both token gradients; the second one to run re-reads them in its GEMM epilogues.  The
        # larger tensor is re-read more cheaply by the dX kernel (fewer stationary fragments per wave), so the site whose X is the
        # larger tensor runs second
        first_b = Xa.numel() >= Xb.numel()
        def run_a(acc):
            return _site_backward(site_a, (*ctx.states[0], Xa, Xb), names_a, params[:na], needs_a, d_a,
                                  d_lba, gXa, gXb, acc_dx=acc, acc_dy=acc, d_probs=dp_a, d_aux=dx_a)   # dX -> gXa, dY -> gXb
        def run_b(acc):
            return _site_backward(site_b, (*ctx.states[1], Xb, Xa), names_b, params[na:], needs_b, d_b,
                                  d_lbb, gXb, gXa, acc_dx=acc, acc_dy=acc, d_probs=dp_b, d_aux=dx_b)   # dX -> gXb, dY -> gXa
        if first_b:
            pgb = run_b(False); pga = run_a(True)
        else:
            pga = run_a(False); pgb = run_b(True)
        return (None, None, None, gXa, gXb, gba, gbb, None, None, None) + ((None,) if ctx.lean else pga + pgb)


class ExpertAdapter(nn.Module):
    """Parameter container with the reference's ExpertAdapter state (net_trans_v3.py:296-374).  It only
    runs as part of a MoEAdapter (the experts of one site are evaluated together on the GPU)."""

    def __init__(self, input_dim, output_dim, adapter_kind, reduction_factor=16, opt=None, use_bn=True,
                 use_gate=True, num_tk=87, is_multimodal=True, variant="ave"):
        super().__init__()
        if adapter_kind != "bottleneck":
            # "basic" exists in the reference (net_trans_v3.py:365-371) but is never instantiated
            raise NotImplementedError(f"adapter_kind={adapter_kind!r}")
        self.adapter_kind, self.use_bn, self.is_multimodal, self.opt, self.num_tk = \
            adapter_kind, bool(use_bn), is_multimodal, opt, num_tk
        g = opt.num_conv_group
        self.gate = nn.Parameter(torch.zeros(1)) if use_gate else None
        self.down_sample_size = input_dim // reduction_factor
        if is_multimodal:
            self.my_tokens = nn.Parameter(torch.rand((num_tk, input_dim)))
            self.gate_av = nn.Parameter(torch.zeros(1))
        elif variant == "avvp":
            self.gate_av = nn.Parameter(torch.zeros(1))                       # mgn.py:83
        elif variant == "avs" and getattr(opt, "is_self_attention", 0) and \
                getattr(opt, "self_attention_version", "v1") == "v2":         # PVT_AVSModel_v2.py:143-145
            self.my_tokens = nn.Parameter(torch.rand((num_tk, input_dim)))
            self.gate_self = nn.Parameter(torch.zeros(1))
        elif getattr(opt, "is_self_attention", 0):
            # AVS self_attention_version "v1" (its default, PVT_AVSModel_v2.py:141-142) and the AVE / AVQA is_self_attention
            # switch (net_trans_v3.py:342-343): the unimodal expert's input is replaced by MultiheadAttention(x, x, x) over the
            # FRAMES.  Parameter container only (in_proj_weight, in_proj_bias, out_proj.*); csrc/mha_frames.hip does the work.
            self.num_head, self.head_dropout = 4, 0.2
            self.self_attention = nn.MultiheadAttention(input_dim, num_heads=self.num_head, dropout=self.head_dropout)
        self.down_sampler = nn.Conv2d(input_dim, self.down_sample_size, 1, groups=g, bias=False)
        self.up_sampler = nn.Conv2d(self.down_sample_size, output_dim, 1, groups=g, bias=False)
        if use_bn:
            self.bn1 = nn.BatchNorm2d(self.down_sample_size)
            self.bn2 = nn.BatchNorm2d(output_dim)
        if opt.is_before_layernorm:
            self.ln_before = nn.LayerNorm(output_dim)
        if opt.is_post_layernorm:
            self.ln_post = nn.LayerNorm(output_dim)

    def forward(self, x, vis_token=None):
        raise capi.AvmoeError("ExpertAdapter runs inside MoEAdapter.forward on the HIP path; it has no standalone forward")


class MoEAdapter(nn.Module):
    """AVE signature (net_trans_v3.py:438-487).  forward(x, vis_token) -> (out (S,C,N,1), expert_indices (S,1))."""

    variant = "ave"

    def __init__(self, input_dim, output_dim, adapter_kind, dim_list, layer_idx, reduction_factor=16, opt=None,
                 use_bn=True, use_gate=True, num_tk=87, conv_dim_in=0, conv_dim_out=0, linear_in=0, linear_out=0):
        super().__init__()
        if input_dim != output_dim or linear_out != input_dim:
            raise ValueError("the adapter sites have input_dim == output_dim == linear_out (net_trans_v3.py:599-637)")
        self.opt, self.use_bn, self.use_gate, self.num_tk = opt, bool(use_bn), bool(use_gate), num_tk
        self.input_dim, self.reduction_factor = input_dim, reduction_factor
        self.conv_adapter = nn.Conv2d(conv_dim_in, conv_dim_out, kernel_size=1)
        self.fc = nn.Linear(linear_in, linear_out)
        self.num_multimodal_experts = opt.num_multimodal_experts
        self.num_singlemodal_experts = opt.num_singlemodal_experts
        mk = lambda mm: ExpertAdapter(input_dim, output_dim, adapter_kind, reduction_factor, opt, use_bn, use_gate,
                                      num_tk, is_multimodal=mm, variant=self.variant)
        self.multimodal_experts = nn.ModuleList([mk(True) for _ in range(self.num_multimodal_experts)])
        self.singlemodal_experts = nn.ModuleList([mk(False) for _ in range(self.num_singlemodal_experts)])
        E = self.num_multimodal_experts + self.num_singlemodal_experts
        self.router = nn.Sequential(nn.Linear(input_dim + linear_out, 128), nn.ReLU(), nn.Linear(128, 32), nn.ReLU(),
                                    nn.Linear(32, E))
        # top-k gating of the mixture (an extension: the reference mixes densely, net_trans_v3.py:482-486; include/avmoe.h at
        # avmoe_moe_forward_topk).  Plain attributes, not state: reassigning them switches the mode of the next call.
        self.router_top_k = getattr(opt, "router_top_k", None)
        self.router_top_k_renorm = getattr(opt, "router_top_k_renorm", True)
        # the router auxiliary losses (z-loss, Switch balance loss: include/avmoe.h at avmoe_moe_forward_aux) beside every forward; a
        # plain attribute like the two above.  Off: the entry points and launches of a site without them.
        self.router_aux = getattr(opt, "router_aux", False)
        # expert-choice gating (include/avmoe.h at avmoe_moe_forward_choice): each expert takes its share of the frames.  Plain attributes too.
        self.router_expert_choice = getattr(opt, "router_expert_choice", None)
        self.router_expert_choice_renorm = getattr(opt, "router_expert_choice_renorm", False)
        # Sinkhorn-balanced top-k (include/avmoe.h at avmoe_moe_forward_sinkhorn): the top-k selection balanced within each call.  Plain attributes too.
        self.router_sinkhorn = getattr(opt, "router_sinkhorn", None)
        self.router_sinkhorn_eval = getattr(opt, "router_sinkhorn_eval", False)
        # expert capacity behind top-k (include/avmoe.h at avmoe_moe_forward_capacity): overflow pairs dropped within each call.  Plain attributes too.
        self.router_capacity_factor = getattr(opt, "router_capacity_factor", None)
        # top-p routing (include/avmoe.h at avmoe_moe_forward_top_p): each frame takes the fewest experts that reach the mass p.  Plain attributes too.
        self.router_top_p = getattr(opt, "router_top_p", None)
        self.router_top_p_min_k = getattr(opt, "router_top_p_min_k", 1)
        self.router_capacity_policy = getattr(opt, "router_capacity_policy", "order")
        self.router_capacity_eval_factor = getattr(opt, "router_capacity_eval_factor", None)
        # the regularisers of the mixture (include/avmoe.h at avmoe_moe_forward_reg): stochastic depth on the adapter branch and expert
        # dropout, training mode only.  Plain attributes like the ones above, not state: no state_dict key, no buffer.
        self.__dict__["_mix_index"] = next(_MIX_SITES)
        self.drop_path = getattr(opt, "adapter_drop_path", 0.0)
        self.expert_dropout = getattr(opt, "adapter_expert_dropout", 0.0)

    @property
    def drop_path(self):
        """p in [0, 1): in training mode every frame's whole adapter output is dropped with probability p (with `add_to`, nothing is
        added) and the kept frames are scaled by 1 / (1 - p).  Eval mode ignores it."""
        return self.__dict__.get("_drop_path", 0.0)       # (.get: a module pickled before the setting existed has none)

    @drop_path.setter
    def drop_path(self, v):
        self.__dict__["_drop_path"] = _rate("drop_path", v)

    @property
    def expert_dropout(self):
        """q in [0, 1): in training mode every (frame, expert) pair of the mixture is dropped independently with probability q and the
        kept ones are scaled by 1 / (1 - q); no renormalisation, no rescue of a frame that loses every expert.  Eval mode ignores it."""
        return self.__dict__.get("_expert_dropout", 0.0)

    @expert_dropout.setter
    def expert_dropout(self, v):
        self.__dict__["_expert_dropout"] = _rate("expert_dropout", v)

    @property
    def mix_seed(self):
        """The 64-bit seed of the site's generator.  Unless assigned: derived from torch.initial_seed() and the site's index in this process's
        construction order, so that two sites do not share their draws.  Assigning it restarts the site's generator (mix_calls = 0).  The
        generator's state is no buffer and is not saved: a resumed run starts it again from its seed."""
        s = self.__dict__.get("_mix_seed")
        if s is None:
            s = (torch.initial_seed() * 0x9E3779B97F4A7C15 + (self.__dict__.get("_mix_index", 0) + 1) * 0xD1B54A32D192ED03) & ((1 << 64) - 1)
        return s

    @mix_seed.setter
    def mix_seed(self, s):
        if s is not None:
            if isinstance(s, bool) or not isinstance(s, numbers.Integral) or not 0 <= int(s) < (1 << 64):
                raise ValueError(f"mix_seed must be None or an integer in [0, 2^64), got {s!r}")
            s = int(s)
        self.__dict__["_mix_seed"] = s
        for k in ("_mix_state", "_mix_last"):
            self.__dict__.pop(k, None)

    @property
    def last_mix_scale(self):
        """The (S, E) multiplier on the mixture weights the last forward drew (a view of the site's own tensor, which the next training
        forward overwrites: read it, do not write it), or None when that forward ran without one (both rates 0, or eval mode)."""
        t = self.__dict__.get("_mix_last")
        return t.detach() if t is not None else None

    @property
    def mix_calls(self):
        """How many multipliers the site's generator has drawn since it was (re)started, read from the device (synchronises)."""
        st = self.__dict__.get("_mix_state")
        return int(st[1].item()) if st is not None else 0

    @property
    def router_select_bias(self):
        """None, or a device tensor (view) of E floats: the bias on the top-k SELECTION of aux-loss-free balancing (the mixture weights do not
        see it).  A plain attribute -- no parameter, no buffer, no state_dict key; avmoe_amd.train.RouterBiasBalancer owns and sets it."""
        return self.__dict__.get("_router_select_bias")   # (.get: a module pickled before the setting existed has none)

    @router_select_bias.setter
    def router_select_bias(self, t):
        self.__dict__["_router_select_bias"] = t

    @property
    def router_select_count(self):
        """None, or a device tensor (view) of E floats that every TRAINING forward adds its selection counts to (eval forwards do not)."""
        return self.__dict__.get("_router_select_count")

    @router_select_count.setter
    def router_select_count(self, t):
        self.__dict__["_router_select_count"] = t

    @property
    def router_aux(self):
        """True: every forward also forms the router z-loss and balance loss and leaves them in `last_router_aux`."""
        return self.__dict__.get("_router_aux", False)     # (.get: a module pickled before the setting existed has none)

    @router_aux.setter
    def router_aux(self, v):
        if not isinstance(v, bool):
            raise ValueError(f"router_aux must be True or False, got {v!r}")
        self.__dict__["_router_aux"] = v

    @property
    def last_router_aux(self):
        """RouterAux(z_loss, balance_loss, load) of the last forward, or None when it ran with `router_aux` off (or none ran yet)."""
        return self.__dict__.get("_last_router_aux")

    @property
    def router_top_k(self):
        """k of the top-k gating, or None: the dense mixture (also what k == E computes)."""
        return self.__dict__.get("_router_top_k")          # (.get: a module pickled before the setting existed stays dense)

    @router_top_k.setter
    def router_top_k(self, k):
        E = self.num_multimodal_experts + self.num_singlemodal_experts
        if k is not None:
            if isinstance(k, bool) or not isinstance(k, numbers.Integral) or not 1 <= int(k) <= E:
                raise ValueError(f"router_top_k must be None or an integer in [1, {E}], got {k!r}")
            k = int(k)
        self.__dict__["_router_top_k"] = k

    @property
    def router_expert_choice(self):
        """None (off), or k in (0, E]: expert-choice gating with a mean of k experts per frame -- each expert takes the
        c = min(S, max(1, ceil(k S / E))) frames of the call on which the router scores it highest; a frame may get no expert (its output is 0)
        or several.  It applies in training and eval mode alike, so an evaluation depends on the batch.  It combines with neither
        `router_top_k` in [1, E) nor a selection bias (checked when the site runs)."""
        return self.__dict__.get("_router_expert_choice")  # (.get: a module pickled before the setting existed has none)

    @router_expert_choice.setter
    def router_expert_choice(self, k):
        E = self.num_multimodal_experts + self.num_singlemodal_experts
        if k is not None:
            if isinstance(k, bool) or not isinstance(k, (numbers.Real, Fraction)) or not (math.isfinite(k) and 0 < k <= E):
                raise ValueError(f"router_expert_choice must be None or a number in (0, {E}], got {k!r}")
        self.__dict__["_router_expert_choice"] = k

    @property
    def router_expert_choice_renorm(self):
        """False (the default, as in Zhou et al. 2022): a frame's weights are the probabilities of the experts that took it; True: divided
        by their sum (a frame no expert took keeps weights of 0)."""
        return self.__dict__.get("_router_expert_choice_renorm", False)

    @router_expert_choice_renorm.setter
    def router_expert_choice_renorm(self, v):
        self.__dict__["_router_expert_choice_renorm"] = bool(v)

    @property
    def last_expert_choice(self):
        """The (S,) int32 bitmask of the last forward -- bit e set where expert e took the frame --, detached; None when it ran without
        `router_expert_choice` (or none ran yet)."""
        return self.__dict__.get("_last_expert_choice")

    @property
    def router_sinkhorn(self):
        """None (off), or n in [1, 64]: Sinkhorn-balanced top-k routing -- n rounds of row / column normalisation of the call's softmax give a
        scale v per expert, and every frame takes the `router_top_k` experts with the largest p v; the weights stay those of the unscaled p.
        It balances within each call (under data parallel: each rank over its own frames), keeps exactly k experts per frame, and has no
        loss term, no rate and no state.  It needs `router_top_k` in [1, E) and combines with neither a selection bias nor
        `router_expert_choice` (checked when the site runs).  Training mode only unless `router_sinkhorn_eval`."""
        return self.__dict__.get("_router_sinkhorn")      # (.get: a module pickled before the setting existed has none)

    @router_sinkhorn.setter
    def router_sinkhorn(self, n):
        if n is not None:
            if isinstance(n, bool) or not isinstance(n, numbers.Integral) or not 1 <= int(n) <= 64:
                raise ValueError(f"router_sinkhorn must be None or an integer in [1, 64], got {n!r}")
            n = int(n)
        self.__dict__["_router_sinkhorn"] = n

    @property
    def router_sinkhorn_eval(self):
        """False (the default, as S-BASE routes at inference): in eval mode the site runs plain top-k, since a balanced assignment depends on
        the rest of the batch; True: Sinkhorn stays on in eval mode."""
        return self.__dict__.get("_router_sinkhorn_eval", False)

    @router_sinkhorn_eval.setter
    def router_sinkhorn_eval(self, v):
        self.__dict__["_router_sinkhorn_eval"] = bool(v)

    @property
    def last_sinkhorn(self):
        """SinkhornReport(scale (E) fp32, count (E) int32, choice (S) int32) of the last forward, device tensors -- the column scale it ranked
        with, the frames each expert took and the bitmask of the selection --; None when it ran without Sinkhorn (or none ran yet)."""
        return self.__dict__.get("_last_sinkhorn")

    @property
    def router_top_p(self):
        """None (off), or a real number P in (0, 1]: top-p ("dynamic-k") routing -- every frame takes the fewest of its ranked experts whose
        probability mass reaches P, at least `router_top_p_min_k` and at most `router_top_k` of them (E when that is unset or not in
        [1, E)); `router_top_k_renorm` says whether the kept weights are renormalised.  Per frame and independent of the batch: training and
        eval mode alike, no parameter, no loss weight, no state.  It combines with none of `router_expert_choice`, `router_sinkhorn`,
        `router_capacity_factor`, `router_select_bias` / `router_select_count` (checked when the site runs)."""
        return self.__dict__.get("_router_top_p")         # (.get: a module pickled before the setting existed has none)

    @router_top_p.setter
    def router_top_p(self, p):
        if p is not None:
            if isinstance(p, bool) or not isinstance(p, numbers.Real) or not 0.0 < float(p) <= 1.0:
                raise ValueError(f"router_top_p must be None or a number in (0, 1], got {p!r}")
            p = float(p)
            if not 0.0 < C.c_float(p).value <= 1.0:       # (the call takes it in fp32)
                raise ValueError(f"router_top_p must lie in (0, 1] as an fp32 number, got {p!r}")
        self.__dict__["_router_top_p"] = p

    @property
    def router_top_p_min_k(self):
        """The fewest experts a frame takes under `router_top_p` (default 1); at most k_max, checked when the site runs."""
        return self.__dict__.get("_router_top_p_min_k", 1)

    @router_top_p_min_k.setter
    def router_top_p_min_k(self, k):
        if isinstance(k, bool) or not isinstance(k, numbers.Integral) or int(k) < 1:
            raise ValueError(f"router_top_p_min_k must be an integer >= 1, got {k!r}")
        self.__dict__["_router_top_p_min_k"] = int(k)

    @property
    def last_top_p(self):
        """TopPReport(choice (S) int32, count (E) int32, khist (E + 1) int32) of the last forward, device tensors -- the bitmask of the
        selection, the frames each expert took and the number of frames served by j experts --; None when it ran without top-p (or none
        ran yet)."""
        return self.__dict__.get("_last_top_p")

    @staticmethod
    def _capacity_factor(name, f):
        if f is not None:
            if isinstance(f, bool) or not isinstance(f, numbers.Real) or not math.isfinite(f) or not f > 0:
                raise ValueError(f"{name} must be None or a finite number > 0, got {f!r}")
        return f

    @property
    def router_capacity_factor(self):
        """None (off), or a finite number f > 0: an expert capacity behind top-k routing (GShard, Switch, V-MoE) -- every expert serves at
        most c = router_capacity(f, router_top_k, S, E) = ceil(f k S / E) of the call's frames; the token-expert pairs beyond that budget
        are dropped (weight exactly 0, nothing renormalised afterwards), and a frame that lost every pair passes through the residual.
        It needs `router_top_k` in [1, E) and combines with neither `router_expert_choice` nor `router_sinkhorn` (checked when the site
        runs); it does combine with a selection bias and its counts (which keep counting demand), `drop_path` / `expert_dropout` and
        `router_aux`.  Training mode only unless `router_capacity_eval_factor`."""
        return self.__dict__.get("_router_capacity_factor")      # (.get: a module pickled before the setting existed has none)

    @router_capacity_factor.setter
    def router_capacity_factor(self, f):
        self.__dict__["_router_capacity_factor"] = self._capacity_factor("router_capacity_factor", f)

    @property
    def router_capacity_policy(self):
        """"order" (the default; GShard / Switch): an expert keeps the first c frames, in frame order, that selected it; "priority"
        (batch-prioritised routing, V-MoE): the c selecting frames on which the router scores it highest, equal scores in frame order."""
        return self.__dict__.get("_router_capacity_policy", "order")

    @router_capacity_policy.setter
    def router_capacity_policy(self, v):
        if v not in _CAPACITY_POLICIES:
            raise ValueError(f"router_capacity_policy must be 'order' or 'priority', got {v!r}")
        self.__dict__["_router_capacity_policy"] = v

    @property
    def router_capacity_eval_factor(self):
        """None (the default): in eval mode the site drops nothing -- the call it makes without a capacity --, since what a capacity drops
        depends on the rest of the batch; a finite number > 0: the capacity factor of eval mode (Switch's eval_capacity_factor)."""
        return self.__dict__.get("_router_capacity_eval_factor")

    @router_capacity_eval_factor.setter
    def router_capacity_eval_factor(self, f):
        self.__dict__["_router_capacity_eval_factor"] = self._capacity_factor("router_capacity_eval_factor", f)

    @property
    def last_capacity(self):
        """CapacityReport(capacity, kept (S) int32, demand (E) int32, kept_count (E) int32) of the last forward -- the budget c (a host int),
        the bitmask of the kept pairs, the frames that selected each expert and the frames it kept; device tensors, nothing synchronised --;
        None when it ran without a capacity (or none ran yet)."""
        return self.__dict__.get("_last_capacity")

    @property
    def router_top_k_renorm(self):
        """True: the kept probabilities are renormalised to sum 1 (a softmax over the kept logits); False: taken as they are (Switch)."""
        return self.__dict__.get("_router_top_k_renorm", True)

    @router_top_k_renorm.setter
    def router_top_k_renorm(self, v):
        self.__dict__["_router_top_k_renorm"] = bool(v)

    # ---- plumbing ---------------------------------------------------------------------------------
    def _self_attn(self):
        if self.variant == "avvp":
            return "nxn"
        if self.variant == "avs" and getattr(self.opt, "is_self_attention", 0) and \
                getattr(self.opt, "self_attention_version", "v1") == "v2":
            return "v2"
        if getattr(self.opt, "is_self_attention", 0) and self.num_singlemodal_experts > 0:
            return "v1"
        return "none"

    def _attention_keep(self, S, N, device):
        """{key: (N * heads, S, S) f32} dropout multipliers (0 or 1 / (1 - p)) of the "v1" experts' attention weights for one
        training-mode call -- the draw nn.MultiheadAttention makes with the global RNG (one per unimodal expert, in expert
        order); {} in eval mode.  `self.attention_keep` (same keys) overrides the draw: tests replay a recorded one."""
        if self._self_attn() != "v1" or not self.training:
            return {}
        forced = getattr(self, "attention_keep", None)
        out = {}
        for j, ex in enumerate(self.singlemodal_experts):
            key = f"singlemodal_experts.{j}.{cm.SA_KEEP}"
            p = ex.self_attention.dropout
            if forced is not None:
                out[key] = forced[key].to(device=device, dtype=torch.float32).contiguous()
            elif p > 0.0:
                out[key] = (torch.rand(N * ex.self_attention.num_heads, S, S, device=device) >= p).float().mul_(1.0 / (1.0 - p))
        return out

    def _desc(self, S, N, M, bf16):
        d = cm.MoeDesc()
        d.S, d.N, d.C, d.M, d.Cy = S, N, self.input_dim, M, self.fc.in_features
        if N != self.conv_adapter.out_channels or M != self.conv_adapter.in_channels:
            raise capi.AvmoeError(f"token counts ({N}, {M}) do not match conv_adapter "
                                  f"({self.conv_adapter.out_channels}, {self.conv_adapter.in_channels})")
        d.E_m, d.E_s = self.num_multimodal_experts, self.num_singlemodal_experts
        d.d, d.groups, d.K = self.input_dim // self.reduction_factor, self.opt.num_conv_group, self.num_tk
        d.use_bn, d.use_gate = int(self.use_bn), int(self.use_gate)
        d.ln_before, d.ln_post = int(bool(self.opt.is_before_layernorm)), int(bool(self.opt.is_post_layernorm))
        d.variant, d.self_attn = cm.VARIANT[self.variant], cm.SELF_ATTN[self._self_attn()]
        d.lb_loss = int(self.variant in ("avvp", "avs") and getattr(self.opt, "use_load_balacing_loss", 0) == 1)
        d.dtype, d.training = (capi.BF16 if bf16 else capi.F32), int(self.training)
        bn = self.multimodal_experts[0].bn1 if (self.use_bn and self.num_multimodal_experts) else \
            (self.singlemodal_experts[0].bn1 if self.use_bn else None)
        d.bn_eps = bn.eps if bn is not None else 1e-5
        d.bn_momentum = self._bn_momentum() if bn is not None else 0.1
        experts = list(self.multimodal_experts) + list(self.singlemodal_experts)
        d.ln_eps = experts[0].ln_before.eps if self.opt.is_before_layernorm else 1e-5
        return d

    def _bn_momentum(self):
        """avmoe_moe_desc.bn_momentum of a site with BatchNorm, read from the modules on every call (torch.optim.swa_utils.update_bn and
        avmoe_amd.train.reestimate_bn set and restore `momentum` between calls): the first BatchNorm's value when all are numbers; -1.0,
        the cumulative average of include/avmoe.h, when all are None (torch's momentum=None); a mix within one site is refused."""
        bns = self._site_cache()["bns"]
        none = [k for k, m in bns if m.momentum is None]
        if not none:
            return bns[0][1].momentum
        if len(none) != len(bns):
            other = next(k for k, m in bns if m.momentum is not None)
            raise capi.AvmoeError(f"BatchNorm momentum must be None on every BatchNorm of a site or on none: {none[0]} has momentum=None, "
                                  f"{other} has momentum={dict(bns)[other].momentum}")
        for k, m in bns:
            if m._buffers.get("num_batches_tracked") is None:
                raise capi.AvmoeError(f"{k} has momentum=None (cumulative average) but no num_batches_tracked: the update factor is "
                                      "1 / (num_batches_tracked + 1)")
        if not capi.lib().avmoe_bn_cumulative:
            raise capi.AvmoeError("this libavmoe_hip.so predates avmoe_bn_cumulative_supported: it takes BatchNorm momentum=None "
                                  "(cumulative average) as a number")
        return -1.0

    def _site_cache(self):
        """Per-module bookkeeping that does not change from call to call (walking named_parameters / named_buffers and resolving
        state_dict keys costs ~0.25 ms per call otherwise -- at the reference's batch of 2 clips that is most of a site's step):
        parameter NAMES and where each parameter / float buffer lives (owner module, attribute), the key -> ABI-field resolution,
        the BatchNorm counters.  The tensors themselves are fetched from their owners' `_parameters` / `_buffers` on every call, so
        a Parameter that was REPLACED (`load_state_dict(assign=True)`, `m.gate = nn.Parameter(..)`, swap-on-convert `.to()`) is
        picked up; `refresh()` drops the cache (call after ADDING / REMOVING parameters or submodules)."""
        c = self.__dict__.get("_avmoe_cache")
        if c is None:
            owners, names = [], []                                     # (owner module, attribute) per parameter, named_parameters order
            seen = set()
            for mod_name, mod in self.named_modules():
                for attr, p in mod._parameters.items():
                    if p is not None and id(p) not in seen:
                        seen.add(id(p))
                        names.append((mod_name + "." if mod_name else "") + attr)
                        owners.append((mod, attr))
            if tuple(names) != tuple(k for k, _ in self.named_parameters()):
                raise capi.AvmoeError("MoEAdapter: parameter registry does not match named_parameters() (parametrized module?)")
            bufs, nbts = [], []                                        # (key, owner module, attribute): float buffers / int64 counters
            for mod_name, mod in self.named_modules():
                for attr, b in mod._buffers.items():
                    if b is not None and b.is_floating_point():
                        bufs.append(((mod_name + "." if mod_name else "") + attr, mod, attr))
                    elif b is not None and attr == "num_batches_tracked" and isinstance(mod, nn.BatchNorm2d):
                        nbts.append(((mod_name + "." if mod_name else "") + attr, mod, attr))
            E_m, E_s = self.num_multimodal_experts, self.num_singlemodal_experts
            bns = [(f"{pre}.{n}", getattr(ex, n)) for pre, ex in zip(cm.expert_prefixes(E_m, E_s), list(self.multimodal_experts) +
                   list(self.singlemodal_experts)) for n in ("bn1", "bn2")] if self.use_bn else []      # every BatchNorm of the site (_bn_momentum)
            c = dict(names=tuple(names), owners=owners, bufs=bufs, nbts=nbts, bns=bns, fill_p=cm.PtrFiller(names, E_m, E_s),
                     fill_b=cm.PtrFiller([k for k, _, _ in bufs], E_m, E_s), fill_n=cm.PtrFiller([k for k, _, _ in nbts], E_m, E_s))
            self.__dict__["_avmoe_cache"] = c
        return c

    def refresh(self):
        for k in ("_avmoe_cache", "_ptrs_cache", "_gptrs_cache", "_ws_sizes"):
            self.__dict__.pop(k, None)

    def __getstate__(self):
        st = self.__dict__.copy()                                      # per-process bookkeeping does not travel (deepcopy / pickle)
        for k in ("_avmoe_cache", "_last_saved", "_ptrs_cache", "_gptrs_cache", "_ws_sizes", "_last_router_aux", "_mix_state", "_mix_buf",
                  "_mix_last", "_mix_draws", "_last_expert_choice", "_last_sinkhorn", "_mode_off",
                  "_last_capacity", "_capacity_meters", "_last_top_p", "_top_p_meters"):
            st.pop(k, None)
        return st

    def _param_tensors(self):
        """{state_dict key: the Parameter CURRENTLY registered under it} (fetched from the owning modules on every call)."""
        c = self._site_cache()
        out = {k: m._parameters.get(a) for k, (m, a) in zip(c["names"], c["owners"])}
        if any(v is None for v in out.values()):                       # a parameter was removed / set to None: rebuild the registry once
            self.refresh()
            c = self._site_cache()
            out = {k: m._parameters[a] for k, (m, a) in zip(c["names"], c["owners"])}
        return out

    def _fill_ptrs(self, params, keep=None, names=None, device=None):
        """MoePtrs of this site's parameters (in _site_cache order), float buffers, BatchNorm counters and -- for the "v1" experts --
        dropout draws.  The filled struct is kept and handed out again while every pointer is the one it was built from (a call
        costs ~60 data_ptr() reads instead of ~60 validations + ctypes stores: at the reference's batch of 2 clips the host side of
        a site step is what bounds it); `names` / `device`: validate dtype / layout / placement when the struct is (re)built."""
        c = self._site_cache()
        bufs = [m._buffers[a] for _, m, a in c["bufs"]]
        bump = bool(self.training and self.use_bn and c["nbts"])
        cnts = [m._buffers[a] for _, m, a in c["nbts"]] if bump else []
        key = (bump, tuple(t.data_ptr() for t in params), tuple(t.data_ptr() for t in bufs), tuple(t.data_ptr() for t in cnts))
        hit = self.__dict__.get("_ptrs_cache")
        if not keep and hit is not None and hit[0] == key:
            return hit[1]
        if names is not None:
            for k, v in zip(names, params):
                if v.dtype != torch.float32 or not v.is_contiguous() or v.device != device:
                    raise capi.AvmoeError(f"parameter {k} must be a contiguous float32 tensor on {device}")
        P = cm.MoePtrs()
        c["fill_p"].fill(P, params)
        for b in bufs:
            if b.dtype != torch.float32 or not b.is_contiguous():
                raise capi.AvmoeError("BatchNorm running statistics must be contiguous float32 tensors")
        c["fill_b"].fill(P, bufs)
        if bump:                                                      # num_batches_tracked += 1 happens inside the forward's kernels (ABI 6)
            for t in cnts:
                if t.dtype != torch.int64 or (bufs and t.device != bufs[0].device):
                    raise capi.AvmoeError("BatchNorm num_batches_tracked must be int64 tensors on the module's device")
            c["fill_n"].fill(P, cnts)
        if keep:
            P2 = cm.make_ptrs(keep, self.num_multimodal_experts, self.num_singlemodal_experts)
            for j in range(self.num_multimodal_experts + self.num_singlemodal_experts):
                if P2.e[j].sa_keep:
                    P.e[j].sa_keep = P2.e[j].sa_keep
        elif names is not None:
            self.__dict__["_ptrs_cache"] = (key, P)                   # (only structs built WITH validation are kept)
        return P

    def grad_layout(self, align: int = 64):
        """(names, offsets, total) of this site's parameter gradients inside one flat fp32 buffer (offsets in elements,
        aligned) -- the layout a gradient sink must use (avmoe_amd.dp)."""
        names, offs, off = [], [], 0
        for k, v in self.named_parameters():
            names.append(k); offs.append(off)
            off += -(-v.numel() // align) * align
        return tuple(names), tuple(offs), off

    def _buffer_tensors(self):
        return {k: v for k, v in self.named_buffers() if v.is_floating_point()}

    def _run(self, x, vis_token, noise=None):
        # the reference hands (S, C, N, 1) permuted views of token-major memory (net_trans_v3.py:695-698)
        X = x.squeeze(-1).permute(0, 2, 1)
        Y = vis_token.squeeze(-1).permute(0, 2, 1)
        P = self._param_tensors()
        names = tuple(P.keys())
        out, probs, idx, lb, aux, load = AdapterFunction.apply(self, X, Y, noise, names, *P.values())
        _publish_aux(self, aux, load)
        return out.permute(0, 2, 1).unsqueeze(-1), probs, idx, lb

    def forward(self, x, vis_token=None):
        out, _probs, idx, _lb = self._run(x, vis_token)
        return out, idx.unsqueeze(-1)                                         # net_trans_v3.py:487


class MoEAdapterAVQA(MoEAdapter):
    """AVQA signature: no num_tk argument, K comes from opt.num_tokens (net_avst_v2.py:233,350-351)."""

    variant = "avqa"

    def __init__(self, input_dim, output_dim, adapter_kind, dim_list, layer_idx, reduction_factor=16, opt=None,
                 use_bn=True, use_gate=True, conv_dim_in=0, conv_dim_out=0, linear_in=0, linear_out=0):
        super().__init__(input_dim, output_dim, adapter_kind, dim_list, layer_idx, reduction_factor, opt, use_bn,
                         use_gate, opt.num_tokens, conv_dim_in, conv_dim_out, linear_in, linear_out)


class MoEAdapterAVVP(MoEAdapter):
    """AVVP signature (mgn.py:161-217): r / bn / gate / K come from `opt`; forward -> (out, load_balancing_loss)."""

    variant = "avvp"

    def __init__(self, input_dim, output_dim, adapter_kind, dim_list, layer_idx, opt=None, conv_dim_in=0,
                 conv_dim_out=0, linear_in=0, linear_out=0):
        super().__init__(input_dim, output_dim, adapter_kind, dim_list, layer_idx, opt.Adapter_downsample, opt,
                         bool(opt.is_bn), bool(opt.is_gate), opt.num_tokens, conv_dim_in, conv_dim_out, linear_in,
                         linear_out)

    def forward(self, x, vis_token=None):
        out, _probs, _idx, lb = self._run(x, vis_token)
        return out, (lb if self.opt.use_load_balacing_loss == 1 else 0.)       # mgn.py:212-217


class MoEAdapterAVS(MoEAdapter):
    """AVS signature (PVT_AVSModel_v2.py:253-312): forward(x, vis_token, is_training=True) ->
    (out, expert_indices (S,1), gating_probs (S,1,E), load_balancing_loss)."""

    variant = "avs"

    def forward(self, x, vis_token=None, is_training=True):
        noise = None
        if is_training:                                                        # PVT_AVSModel_v2.py:294-296
            E = self.num_multimodal_experts + self.num_singlemodal_experts
            noise = torch.randn(x.shape[0], E, device=x.device, dtype=torch.float32) * 0.01
        out, probs, idx, lb = self._run(x, vis_token, noise)
        return out, idx.unsqueeze(-1), probs.unsqueeze(1), (lb if self.opt.use_load_balacing_loss == 1 else 0.)


def _storage_range(t: torch.Tensor):
    lo = t.untyped_storage().data_ptr()
    return lo, lo + t.untyped_storage().nbytes()


def _safe_inplace(base: torch.Tensor, others) -> bool:
    """May `base` be overwritten in place?  It has to own its storage (not a view of something else somebody may read)
    and that storage must not overlap any of `others`."""
    if base._base is not None or base.untyped_storage().nbytes() != base.numel() * base.element_size():
        return False
    lo, hi = _storage_range(base)
    for o in others:
        olo, ohi = _storage_range(o)
        if lo < ohi and olo < hi:
            return False
    return True


class AdapterPair(nn.Module):
    """The two adapter sites of one backbone layer run as one autograd node:

        pair = AdapterPair(audio_site, visual_site)            # two MoEAdapter* modules of one variant (shared, not copied)
        out_a, idx_a, out_v, idx_v = pair(f_a, f_v)            # AVE / AVQA: == audio_site(f_a, f_v) + visual_site(f_v, f_a)
        out_a, lb_a, out_v, lb_v = pair(f_a, f_v)              # AVVP  (mgn.py:212-217)
        out_a, idx_a, probs_a, lb_a, out_v, idx_v, probs_v, lb_v = pair(f_a, f_v, is_training=True)      # AVS (PVT_AVSModel_v2.py:294-312)

    Numerically identical to calling the two sites one after the other; in the backward the gradient each token tensor
    receives from its second use is added inside the GEMM epilogues instead of by a separate accumulation kernel."""

    def __init__(self, site_a: MoEAdapter, site_b: MoEAdapter, concurrent: bool = True):
        """concurrent=True runs the two sites on two HIP streams (their kernels overlap; each token tensor collects its two gradients
        in ONE buffer: a site overwrites its own tokens' gradient with its dX and, behind an event, adds its dY to the other tensor in
        the GEMM epilogue -- nobody waits before the last section); False runs them back to back on the caller's stream.  Sites with
        latent self attention on their own tokens (AVS "v2") write dX in their last section too, so their backward cannot be split:
        such a pair always runs back to back."""
        super().__init__()
        if site_a.variant != site_b.variant:
            raise ValueError(f"AdapterPair: the two sites have different signatures ({site_a.variant} / {site_b.variant})")
        splittable = all(m._self_attn() != "v2" for m in (site_a, site_b))
        self.concurrent, self._side, self._events = bool(concurrent) and splittable, None, None
        # same_stream (measurement aid, bench.py's per-launch profiling pass): the two-stream SCHEDULE -- every kernel in the variant
        # the concurrent mode launches (dX overwrites, dY adds behind the other site's dX) -- issued on the caller's stream alone,
        # so that an event bracket around a launch measures that launch and not the other stream's kernels
        self.same_stream = False
        self.variant = site_a.variant
        self.site_a, self.site_b = site_a, site_b

    def forward(self, x_a, x_b, add_to=(None, None), is_training=True):
        """add_to = (base_a, base_b): token-major (S, N, C) residual streams (or None) that receive `+= adapter output` IN PLACE
        inside the output GEMM and are returned (in the (S, C, N, 1) view) instead of the bare adapter outputs -- the
        `f = f + f_res` of net_trans_v3.py:709,712 without a separate pass.  Only hand in tensors nobody else needs at their
        old value (e.g. the fresh result of `x + attention(x)`).
        is_training: the AVS sites' flag (logit noise, drawn for site A first -- the order of two separate calls)."""
        Xa = x_a.squeeze(-1).permute(0, 2, 1)
        Xb = x_b.squeeze(-1).permute(0, 2, 1)
        Pa, Pb = self.site_a._param_tensors(), self.site_b._param_tensors()
        if self.concurrent and self._side is None:
            self._side = side_stream(x_a.device)
            self._events = tuple(torch.cuda.Event() for _ in range(6))      # backward hand-over (2), fork, join, hop-1 chains done (2)
        for base, X in zip(add_to, (Xa, Xb)):
            if base is not None and not _safe_inplace(base, (Xa, Xb)):
                raise capi.AvmoeError("add_to must own its storage (no view) and must not overlap the token tensors")
        noises = (None, None)
        if self.variant == "avs" and is_training:                             # PVT_AVSModel_v2.py:294-296
            noises = tuple(torch.randn(x.shape[0], m.num_multimodal_experts + m.num_singlemodal_experts, device=x.device,
                                       dtype=torch.float32) * 0.01 for m, x in ((self.site_a, x_a), (self.site_b, x_b)))
        side = ((torch.cuda.current_stream(x_a.device) if self.same_stream else self._side,) + self._events) if self.concurrent else None
        # With a gradient sink on both sites (avmoe_amd.dp.AdapterGradReducer(sites=...)) and every parameter trainable, the backward
        # writes the parameter gradients into the reducer's buckets and autograd gets None for them anyway: ONE anchor parameter
        # then stands in for the ~120 of the pair (unwrapping, saving and returning a gradient slot for each of them is a third of
        # the host time of a step at the reference's batch of 2 clips -- tests/dev/host_split.py).
        lean = torch.is_grad_enabled() and all(
            getattr(m, "_grad_sink", None) is not None and m._grad_sink.flat is not None and all(p.requires_grad for p in P.values())
            and m._grad_sink.matches(tuple(P.keys()), P) for m, P in ((self.site_a, Pa), (self.site_b, Pb)))
        plist = (next(iter(Pa.values())),) if lean and len(Pa) > 1 else (*Pa.values(), *Pb.values())
        out_a, out_b, idx_a, idx_b, pr_a, pr_b, lb_a, lb_b, ax_a, ax_b, ld_a, ld_b = _PairFunction.apply(
            self.site_a, self.site_b, side, Xa, Xb, add_to[0], add_to[1], tuple(Pa.keys()), tuple(Pb.keys()), noises, *plist)
        _publish_aux(self.site_a, ax_a, ld_a)               # (each site's own `router_aux` setting decided: read in _site_forward)
        _publish_aux(self.site_b, ax_b, ld_b)
        out_a, out_b = out_a.permute(0, 2, 1).unsqueeze(-1), out_b.permute(0, 2, 1).unsqueeze(-1)
        if self.variant in ("ave", "avqa"):
            return out_a, idx_a.unsqueeze(-1), out_b, idx_b.unsqueeze(-1)
        use_lb = (self.site_a.opt.use_load_balacing_loss == 1, self.site_b.opt.use_load_balacing_loss == 1)
        lb_a, lb_b = (lb_a if use_lb[0] else 0.), (lb_b if use_lb[1] else 0.)
        if self.variant == "avvp":
            return out_a, lb_a, out_b, lb_b
        return (out_a, idx_a.unsqueeze(-1), pr_a.unsqueeze(1), lb_a, out_b, idx_b.unsqueeze(-1), pr_b.unsqueeze(1), lb_b)
