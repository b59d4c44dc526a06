"""ctypes declarations + thin helpers for the MoE-adapter section of include/avmoe.h."""
from __future__ import annotations

import ctypes as C
from typing import Dict, List

MAX_EXPERTS = 16
OPT_CLIP, OPT_SKIP_NONFINITE, OPT_DECOUPLED_DECAY, OPT_LR_SCHEDULE = 1, 2, 4, 8      # flags of avmoe_opt_grad_norm[_sched] / avmoe_opt_adam_step
OPT_EMA = 16                                                        # ... of avmoe_opt_grad_norm_ema / avmoe_opt_adam_step_ema only
OPT_REPORT = 32                                                     # ... of avmoe_opt_grad_norm_report only
OPT_SWA, OPT_SWA_LR = 64, 128                                       # ... of avmoe_opt_grad_norm_swa only
SWA_ANNEAL_KINDS = {"cos": 0, "linear": 1}                          # AVMOE_SWA_ANNEAL_*
SCHED_KINDS = {"none": 0, "cosine": 1, "linear": 2, "step": 3}      # AVMOE_SCHED_*
VARIANT = {"ave": 0, "avqa": 0, "avvp": 1, "avs": 2}
SELF_ATTN = {"none": 0, "v2": 1, "nxn": 2, "v1": 3}


class MoeDesc(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("S", "N", "C", "M", "Cy", "E_m", "E_s", "d", "groups", "K", "use_bn",
                                         "use_gate", "ln_before", "ln_post", "variant", "self_attn", "lb_loss",
                                         "dtype", "training")] + \
               [(n, C.c_float) for n in ("bn_eps", "ln_eps", "bn_momentum")] + \
               [(n, C.c_int32) for n in ("accumulate_dx", "accumulate_dy", "accumulate_out", "shared_gpu")]


class OptRange(C.Structure):
    """avmoe_opt_range: one flat (param, grad, exp_avg, exp_avg_sq) range of the optimizer with its learning rate and decay"""
    _fields_ = [(n, C.c_void_p) for n in ("param", "grad", "exp_avg", "exp_avg_sq")] + [("n", C.c_int64), ("lr", C.c_float),
                                                                                       ("weight_decay", C.c_float)]


class OptLayout(C.Structure):
    _fields_ = [("state_bytes", C.c_size_t), ("table_bytes", C.c_size_t), ("partial_bytes", C.c_size_t), ("n_blocks", C.c_int64)]


class OptSchedule(C.Structure):
    """avmoe_opt_schedule: the host constants of a per-step learning-rate schedule"""
    _fields_ = [("warmup_steps", C.c_int64), ("warmup_start", C.c_float), ("decay_kind", C.c_int32), ("total_steps", C.c_int64),
                ("min_factor", C.c_float), ("gamma", C.c_float), ("step_size", C.c_int64)]


class OptEma(C.Structure):
    """avmoe_opt_ema: the host constants of the weight average, d_n = min(decay, (1 + n) / (warmup + n))"""
    _fields_ = [("decay", C.c_float), ("warmup", C.c_float)]


class OptSwa(C.Structure):
    """avmoe_opt_swa: the host constants of stochastic weight averaging -- the uniform average (start, freq) and the annealed rate"""
    _fields_ = [("start", C.c_int64), ("lr_start", C.c_int64), ("freq", C.c_int32), ("anneal_steps", C.c_int32), ("lr_factor", C.c_float),
                ("anneal_kind", C.c_int32)]


class OptBuffer(C.Structure):
    """avmoe_opt_buffer: one averaged buffer (BatchNorm running statistics) with its shadow; a record of the buffer table"""
    _fields_ = [("buffer", C.c_void_p), ("shadow", C.c_void_p), ("n", C.c_int64)]


class OptSamState(C.Structure):
    """avmoe_opt_sam_state: what avmoe_opt_sam_perturb's finalize launch leaves on the device"""
    _fields_ = [("norm", C.c_float), ("scale", C.c_float), ("nonfinite", C.c_int32), ("reserved", C.c_int32)]


class OptReportHeader(C.Structure):
    """avmoe_opt_report_header: what precedes the per-range norms in a report buffer"""
    _fields_ = [("first_nonfinite", C.c_int32), ("n_ranges", C.c_int32), ("reserved", C.c_int32 * 2)]


class OptLambHeader(C.Structure):
    """avmoe_opt_lamb_header: what precedes w_norm[n], u_norm[n], ratio[n] in a trust report buffer"""
    _fields_ = [("n_ranges", C.c_int32), ("reserved", C.c_int32 * 3)]


class OptLambLayout(C.Structure):
    """avmoe_opt_lamb_layout: the bytes of avmoe_opt_lamb_step's workspace and report"""
    _fields_ = [("workspace_bytes", C.c_size_t), ("report_bytes", C.c_size_t)]


class OptProdigy(C.Structure):
    """avmoe_opt_prodigy: the host constants of Prodigy learning-rate estimation (growth 0: no limit)"""
    _fields_ = [("d0", C.c_float), ("d_coef", C.c_float), ("growth", C.c_float), ("safeguard_warmup", C.c_int32)]


class OptProdigyState(C.Structure):
    """avmoe_opt_prodigy_state: the 32-byte block avmoe_opt_prodigy_step's finalize launch keeps on the device"""
    _fields_ = [("d", C.c_float), ("d_max", C.c_float), ("d_hat", C.c_float), ("reserved", C.c_int32), ("num", C.c_double), ("den", C.c_double)]


class OptSf(C.Structure):
    """avmoe_opt_sf: the host constants of schedule-free AdamW (the averaging weight of step n is n^r * f_max^lr_power)"""
    _fields_ = [("r", C.c_float), ("lr_power", C.c_float)]


class OptSfState(C.Structure):
    """avmoe_opt_sf_state: the 32-byte block avmoe_opt_sf_step's weights launch keeps on the device (all zero at the start)"""
    _fields_ = [("weight_sum", C.c_double), ("f_max", C.c_float), ("c", C.c_float), ("d", C.c_float), ("reserved", C.c_int32 * 3)]


class OptProdigyLayout(C.Structure):
    """avmoe_opt_prodigy_layout: the bytes of avmoe_opt_prodigy_step's workspace and block"""
    _fields_ = [("workspace_bytes", C.c_size_t), ("block_bytes", C.c_size_t)]


class OptMuonMat(C.Structure):
    """avmoe_opt_muon_mat: one orthogonalised matrix: the range it is, read as row-major rows x cols"""
    _fields_ = [("range", C.c_int32), ("rows", C.c_int32), ("cols", C.c_int32), ("reserved", C.c_int32)]


class OptMuon(C.Structure):
    """avmoe_opt_muon: the host constants of orthogonalised momentum (scale: 0 match_rms_adamw, 1 original)"""
    _fields_ = [("momentum", C.c_float), ("nesterov", C.c_int32), ("ns_steps", C.c_int32), ("scale", C.c_int32)]


class OptMuonLayout(C.Structure):
    """avmoe_opt_muon_layout: the bytes of the matrix image, avmoe_opt_muon_step's workspace and its report"""
    _fields_ = [("table_bytes", C.c_size_t), ("workspace_bytes", C.c_size_t), ("report_bytes", C.c_size_t)]


class OptMuonLargeLayout(C.Structure):
    """avmoe_opt_muon_large_layout: the bytes of the large-matrix image, the staging workspace and the report; the class count"""
    _fields_ = [("table_bytes", C.c_size_t), ("workspace_bytes", C.c_size_t), ("report_bytes", C.c_size_t), ("n_classes", C.c_int32),
                ("reserved", C.c_int32)]


class OptMuonClass(C.Structure):
    """avmoe_opt_muon_class: one class of equal-shaped large matrices after orientation (d = the short side)"""
    _fields_ = [("d", C.c_int32), ("L", C.c_int32), ("count", C.c_int32), ("ksplit", C.c_int32)]


# avmoe_opt_prodigy_state: field -> (byte offset, torch dtype name); 32 bytes
OPT_PRODIGY_FIELDS = {"d": (0, "float32"), "d_max": (4, "float32"), "d_hat": (8, "float32"), "num": (16, "float64"), "den": (24, "float64")}

# avmoe_opt_sf_state: field -> (byte offset, torch dtype name); 32 bytes
OPT_SF_FIELDS = {"weight_sum": (0, "float64"), "f_max": (8, "float32"), "c": (12, "float32"), "d": (16, "float32")}

# avmoe_opt_state: field -> (byte offset, torch dtype name); 64 bytes
OPT_STATE_BYTES = 64
OPT_STATE_FIELDS = {"total_norm": (0, "float32"), "clip_coef": (4, "float32"), "bc1": (8, "float32"), "bc2_sqrt": (12, "float32"),
                    "applied_steps": (16, "int64"), "skipped_steps": (24, "int64"), "skip": (32, "int32"), "lr_factor": (36, "float32"),
                    "ema_decay": (40, "float32")}


_EXPERT_FIELDS = ("gate", "my_tokens", "gate_lat", "down_w", "up_w", "bn1_w", "bn1_b", "bn2_w", "bn2_b",
                  "lnb_w", "lnb_b", "lnp_w", "lnp_b", "bn1_rm", "bn1_rv", "bn2_rm", "bn2_rv",
                  "sa_in_w", "sa_in_b", "sa_out_w", "sa_out_b", "sa_keep", "bn1_nbt", "bn2_nbt")
_TOP_FIELDS = ("conv_w", "conv_b", "fc_w", "fc_b", "r0_w", "r0_b", "r2_w", "r2_b", "r4_w", "r4_b")


class ExpertPtrs(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in _EXPERT_FIELDS]


class MoePtrs(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in _TOP_FIELDS] + [("e", ExpertPtrs * MAX_EXPERTS)]


SA_KEEP = "self_attention.__keep__"

# state_dict leaf (relative to the expert prefix) -> ExpertPtrs field
EXPERT_KEY_TO_FIELD = {
    "gate": "gate", "my_tokens": "my_tokens", "gate_av": "gate_lat", "gate_self": "gate_lat",
    "down_sampler.weight": "down_w", "up_sampler.weight": "up_w",
    "bn1.weight": "bn1_w", "bn1.bias": "bn1_b", "bn2.weight": "bn2_w", "bn2.bias": "bn2_b",
    "ln_before.weight": "lnb_w", "ln_before.bias": "lnb_b", "ln_post.weight": "lnp_w", "ln_post.bias": "lnp_b",
    "bn1.running_mean": "bn1_rm", "bn1.running_var": "bn1_rv", "bn2.running_mean": "bn2_rm", "bn2.running_var": "bn2_rv",
    "self_attention.in_proj_weight": "sa_in_w", "self_attention.in_proj_bias": "sa_in_b",
    "self_attention.out_proj.weight": "sa_out_w", "self_attention.out_proj.bias": "sa_out_b",
    SA_KEEP: "sa_keep",            # not a state_dict entry: the dropout multiplier of one call (include/avmoe.h)
    "bn1.num_batches_tracked": "bn1_nbt", "bn2.num_batches_tracked": "bn2_nbt",      # int64 counters, bumped inside the forward (ABI 6)
}
INT64_FIELDS = ("bn1_nbt", "bn2_nbt")
TOP_KEY_TO_FIELD = {
    "conv_adapter.weight": "conv_w", "conv_adapter.bias": "conv_b", "fc.weight": "fc_w", "fc.bias": "fc_b",
    "router.0.weight": "r0_w", "router.0.bias": "r0_b", "router.2.weight": "r2_w", "router.2.bias": "r2_b",
    "router.4.weight": "r4_w", "router.4.bias": "r4_b",
}


# include/avmoe.h: AVMOE_NXN_* (avmoe_nxn_strip)
NXN_OP = {"STATS": 0, "ATT": 1, "ATT_FROM_LSE": 2, "XR": 3, "Y": 4, "DXQ": 5, "DXK": 6, "ATT_BWD": 7}


def declare(L):
    L.avmoe_adam_step.restype = C.c_int
    L.avmoe_adam_step.argtypes = [C.c_void_p] * 4 + [C.c_int64] + [C.c_float] * 5 + [C.c_int64, C.c_float, C.c_void_p]
    L.avmoe_add2.restype = C.c_int
    L.avmoe_add2.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p]
    L.avmoe_router_topk.restype = C.c_int
    L.avmoe_router_topk.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
    L.avmoe_expert_histogram.restype = C.c_int
    L.avmoe_expert_histogram.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p]
    L.avmoe_router_forward.restype = C.c_int
    L.avmoe_router_forward.argtypes = [C.POINTER(MoeDesc), C.c_void_p, C.POINTER(MoePtrs)] + [C.c_void_p] * 7
    for fn in (L.avmoe_expert_forward_cross, L.avmoe_expert_forward_uni):      # sub-ops (ABI 7): one expert's output alone
        fn.restype = C.c_int
        fn.argtypes = [C.POINTER(MoeDesc), C.c_void_p, C.c_void_p, C.POINTER(MoePtrs), C.c_int32] + [C.c_void_p] * 4
    L.avmoe_remap_forward.restype = C.c_int                                    # the remap materialised
    L.avmoe_remap_forward.argtypes = [C.POINTER(MoeDesc), C.c_void_p, C.POINTER(MoePtrs)] + [C.c_void_p] * 5
    L.avmoe_moe_saved_bytes.restype = C.c_size_t
    L.avmoe_moe_saved_bytes.argtypes = [C.POINTER(MoeDesc)]
    L.avmoe_moe_scratch_bytes.restype = C.c_size_t
    L.avmoe_moe_scratch_bytes.argtypes = [C.POINTER(MoeDesc)]
    L.avmoe_moe_forward.restype = C.c_int
    L.avmoe_moe_forward.argtypes = [C.POINTER(MoeDesc), C.c_void_p, C.c_void_p, C.POINTER(MoePtrs), C.c_void_p,
                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.avmoe_moe_backward.restype = C.c_int
    L.avmoe_moe_backward.argtypes = [C.POINTER(MoeDesc), C.c_void_p, C.c_void_p, C.POINTER(MoePtrs), C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(MoePtrs),
                                     C.c_void_p]
    L.avmoe_moe_backward_part.restype = C.c_int
    L.avmoe_moe_backward_part.argtypes = [C.POINTER(MoeDesc), C.c_void_p, C.c_void_p, C.POINTER(MoePtrs), C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(MoePtrs),
                                          C.c_int32, C.c_void_p]
    # the site entry points found by symbol (added under ABI 11: dprobs and dOut == NULL, top-k gating, the router auxiliary losses), keyed on the
    # newest one; avmoe_site_aux: what the facade asks once (a development A/B may load an older library through AVMOE_LIB)
    L.avmoe_site_aux = hasattr(L, "avmoe_moe_backward_aux")
    # avmoe_moe_desc.bn_momentum < 0 = torch's momentum=None (found by symbol, ABI 11: an older library would take -1.0 as a number)
    L.avmoe_bn_cumulative = hasattr(L, "avmoe_bn_cumulative_supported")
    if L.avmoe_bn_cumulative:
        L.avmoe_bn_cumulative_supported.restype = C.c_int
        L.avmoe_bn_cumulative = bool(L.avmoe_bn_cumulative_supported())
    if L.avmoe_site_aux:
        head = [C.POINTER(MoeDesc), C.c_void_p, C.c_void_p, C.POINTER(MoePtrs), C.c_void_p]
        L.avmoe_moe_forward_topk.restype, L.avmoe_moe_forward_topk.argtypes = C.c_int, head + [C.c_int32, C.c_int32] + [C.c_void_p] * 7
        L.avmoe_moe_forward_aux.restype, L.avmoe_moe_forward_aux.argtypes = C.c_int, head + [C.c_int32, C.c_int32] + [C.c_void_p] * 9
        L.avmoe_moe_backward_ex.restype = L.avmoe_moe_backward_aux.restype = C.c_int
        L.avmoe_moe_backward_ex.argtypes = head + [C.c_void_p] * 6 + [C.POINTER(MoePtrs), C.c_int32, C.c_void_p]
        L.avmoe_moe_backward_aux.argtypes = head + [C.c_void_p] * 7 + [C.POINTER(MoePtrs), C.c_int32, C.c_void_p]
    # the mixture regularisers (found by symbol: a multiplier on the mixture weights, and its draw on the device)
    L.avmoe_site_reg = L.avmoe_site_aux and hasattr(L, "avmoe_moe_forward_reg") and hasattr(L, "avmoe_mix_drop_draw")
    if L.avmoe_site_reg:
        L.avmoe_moe_forward_reg.restype, L.avmoe_moe_forward_reg.argtypes = C.c_int, head + [C.c_int32, C.c_int32] + [C.c_void_p] * 10
        L.avmoe_moe_backward_reg.restype = C.c_int
        L.avmoe_moe_backward_reg.argtypes = head + [C.c_void_p] * 8 + [C.POINTER(MoePtrs), C.c_int32, C.c_void_p]
        L.avmoe_mix_drop_draw.restype = C.c_int
        L.avmoe_mix_drop_draw.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_float, C.c_float, C.c_void_p, C.c_void_p]
    # aux-loss-free balancing (found by symbol: a bias on the top-k selection, the selection counts, and the update of the bias)
    L.avmoe_site_bias = L.avmoe_site_reg and hasattr(L, "avmoe_moe_forward_bias") and hasattr(L, "avmoe_router_bias_update")
    if L.avmoe_site_bias:
        L.avmoe_moe_forward_bias.restype, L.avmoe_moe_forward_bias.argtypes = C.c_int, head + [C.c_int32, C.c_int32] + [C.c_void_p] * 12
        L.avmoe_router_bias_update.restype = C.c_int
        L.avmoe_router_bias_update.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_float, C.c_void_p]
    # expert-choice gating (found by symbol: the site forward with a per-expert selection of frames, and the selection as a sub-op)
    L.avmoe_site_choice = L.avmoe_site_reg and hasattr(L, "avmoe_moe_forward_choice") and hasattr(L, "avmoe_expert_choice")
    if L.avmoe_site_choice:
        L.avmoe_moe_forward_choice.restype, L.avmoe_moe_forward_choice.argtypes = C.c_int, head + [C.c_int32, C.c_int32] + [C.c_void_p] * 11
        L.avmoe_expert_choice.restype = C.c_int
        L.avmoe_expert_choice.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32] + [C.c_void_p] * 6
    # Sinkhorn-balanced top-k (found by symbol: the site forward with the selection balanced within the call, and the two kernels as a sub-op)
    L.avmoe_site_sinkhorn = L.avmoe_site_reg and hasattr(L, "avmoe_moe_forward_sinkhorn") and hasattr(L, "avmoe_router_sinkhorn")
    if L.avmoe_site_sinkhorn:
        L.avmoe_moe_forward_sinkhorn.restype, L.avmoe_moe_forward_sinkhorn.argtypes = C.c_int, head + [C.c_int32] * 3 + [C.c_void_p] * 12
        L.avmoe_router_sinkhorn.restype = C.c_int
        L.avmoe_router_sinkhorn.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32] + [C.c_void_p] * 6
    # expert capacity behind top-k (found by symbol: the site forward that drops the pairs beyond each expert's budget, and the kernels as a sub-op)
    L.avmoe_site_capacity = bool(L.avmoe_site_bias and hasattr(L, "avmoe_moe_forward_capacity") and hasattr(L, "avmoe_router_capacity"))
    if L.avmoe_site_capacity:
        L.avmoe_moe_forward_capacity.restype = C.c_int
        L.avmoe_moe_forward_capacity.argtypes = head + [C.c_int32, C.c_int32] + [C.c_void_p] * 3 + [C.c_int32, C.c_int32] + [C.c_void_p] * 13
        L.avmoe_router_capacity.restype = C.c_int
        L.avmoe_router_capacity.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_int32] + [C.c_void_p] * 9
    # top-p routing (found by symbol: the site forward where each frame takes the fewest experts reaching the mass P, and the kernels as a sub-op)
    L.avmoe_site_top_p = bool(L.avmoe_site_reg and hasattr(L, "avmoe_moe_forward_top_p") and hasattr(L, "avmoe_router_top_p"))
    if L.avmoe_site_top_p:
        L.avmoe_moe_forward_top_p.restype = C.c_int
        L.avmoe_moe_forward_top_p.argtypes = head + [C.c_float] + [C.c_int32] * 3 + [C.c_void_p] * 13
        L.avmoe_router_top_p.restype = C.c_int
        L.avmoe_router_top_p.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_float, C.c_int32, C.c_int32, C.c_int32] + [C.c_void_p] * 6
    if hasattr(L, "avmoe_moe_backward_dx_dy"):       # (ABI 10; a development A/B may load an older library through AVMOE_LIB, with AVMOE_NO_FUSED_DX=1)
        L.avmoe_moe_backward_dx_dy.restype = C.c_int
        L.avmoe_moe_backward_dx_dy.argtypes = [C.POINTER(MoeDesc), C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(MoeDesc), C.c_void_p, C.c_void_p,
                                               C.c_void_p, C.c_void_p]
    if hasattr(L, "avmoe_opt_swap_ema"):             # (found by its newest symbol: the optimizer with device-side state, one tree builds all of it)
        step_args = [C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.c_float, C.c_float, C.c_float, C.c_float, C.c_int32, C.c_void_p]
        norm_args = [C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_int32, C.c_float, C.c_float, C.c_void_p]
        L.avmoe_opt_workspace_bytes.restype = C.c_size_t
        L.avmoe_opt_workspace_bytes.argtypes = [C.POINTER(OptRange), C.c_int32, C.POINTER(OptLayout)]
        for name, args in (("table_build", [C.POINTER(OptRange), C.c_int32, C.c_void_p, C.c_size_t]),
                           ("grad_norm", norm_args), ("grad_norm_sched", norm_args + [C.POINTER(OptSchedule)]),
                           ("grad_norm_ema", norm_args + [C.POINTER(OptSchedule), C.POINTER(OptEma)]),
                           ("adam_step", step_args), ("adam_step_ema", step_args + [C.c_void_p]),
                           ("swap_ema", [C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p])):
            fn = getattr(L, "avmoe_opt_" + name)
            fn.restype, fn.argtypes = C.c_int, args
        if hasattr(L, "avmoe_opt_grad_norm_report"):  # (found by symbol: the per-range gradient norms)
            L.avmoe_opt_report_bytes.restype, L.avmoe_opt_report_bytes.argtypes = C.c_size_t, [C.c_int32]
            L.avmoe_opt_grad_norm_report.restype = C.c_int
            L.avmoe_opt_grad_norm_report.argtypes = norm_args + [C.POINTER(OptSchedule), C.POINTER(OptEma), C.c_void_p]
        if hasattr(L, "avmoe_opt_grad_norm_swa"):     # (found by symbol: stochastic weight averaging)
            L.avmoe_opt_grad_norm_swa.restype = C.c_int
            L.avmoe_opt_grad_norm_swa.argtypes = norm_args + [C.POINTER(OptSchedule), C.POINTER(OptEma), C.c_void_p, C.POINTER(OptSwa)]
        if hasattr(L, "avmoe_opt_adam_step_sam"):     # (found by symbol: sharpness-aware minimization)
            L.avmoe_opt_sam_perturb.restype = L.avmoe_opt_adam_step_sam.restype = C.c_int
            L.avmoe_opt_sam_perturb.argtypes = [C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_int32, C.c_void_p,
                                                C.c_void_p]
            L.avmoe_opt_adam_step_sam.argtypes = step_args + [C.c_void_p, C.c_void_p]
        if hasattr(L, "avmoe_opt_lamb_step"):         # (found by symbol: layer-wise trust ratios)
            L.avmoe_opt_lamb_bytes.restype, L.avmoe_opt_lamb_bytes.argtypes = C.c_size_t, [C.c_int32, C.c_int64, C.POINTER(OptLambLayout)]
            L.avmoe_opt_lamb_step.restype = C.c_int
            L.avmoe_opt_lamb_step.argtypes = step_args + [C.c_void_p] * 5       # shadows, hold, limits, workspace, report
        if hasattr(L, "avmoe_opt_prodigy_step"):      # (found by symbol: Prodigy learning-rate estimation)
            L.avmoe_opt_prodigy_bytes.restype, L.avmoe_opt_prodigy_bytes.argtypes = C.c_size_t, [C.c_int64, C.POINTER(OptProdigyLayout)]
            L.avmoe_opt_prodigy_step.restype = C.c_int
            # shadows, hold, x0, s, consts (HOST), block, workspace
            L.avmoe_opt_prodigy_step.argtypes = step_args + [C.c_void_p] * 4 + [C.POINTER(OptProdigy), C.c_void_p, C.c_void_p]
        if hasattr(L, "avmoe_opt_sf_step"):           # (found by symbol: schedule-free AdamW)
            L.avmoe_opt_sf_step.restype = C.c_int
            L.avmoe_opt_sf_step.argtypes = step_args + [C.c_void_p, C.c_void_p, C.POINTER(OptSf), C.c_void_p]      # x, hold, consts (HOST), block
        if hasattr(L, "avmoe_opt_muon_step"):         # (found by symbol: orthogonalised momentum)
            L.avmoe_opt_muon_bytes.restype = C.c_size_t
            L.avmoe_opt_muon_bytes.argtypes = [C.c_int32, C.c_int64, C.c_int32, C.POINTER(OptMuonLayout)]
            L.avmoe_opt_muon_table_build.restype = C.c_int
            L.avmoe_opt_muon_table_build.argtypes = [C.POINTER(OptRange), C.c_int32, C.POINTER(OptMuonMat), C.c_int32, C.c_void_p, C.c_size_t]
            L.avmoe_opt_muon_step.restype = C.c_int
            # shadows, hold, mats (the DEVICE image), n_mats, work, consts (HOST), workspace, report
            L.avmoe_opt_muon_step.argtypes = step_args + [C.c_void_p] * 3 + [C.c_int32, C.c_void_p, C.POINTER(OptMuon), C.c_void_p, C.c_void_p]
            L.avmoe_opt_muon_ns.restype = C.c_int
            L.avmoe_opt_muon_ns.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]
        if hasattr(L, "avmoe_opt_muon_step_large"):   # (found by symbol: orthogonalised momentum for the large matrices)
            L.avmoe_opt_muon_large_bytes.restype = C.c_size_t
            L.avmoe_opt_muon_large_bytes.argtypes = [C.c_int32, C.POINTER(OptMuonMat), C.c_int32, C.POINTER(OptMuonLargeLayout)]
            L.avmoe_opt_muon_large_table_build.restype = C.c_int
            L.avmoe_opt_muon_large_table_build.argtypes = [C.POINTER(OptRange), C.c_int32, C.POINTER(OptMuonMat), C.c_int32, C.POINTER(OptMuonMat),
                                                           C.c_int32, C.c_void_p, C.c_size_t]
            L.avmoe_opt_muon_large_classes.restype = C.c_int
            L.avmoe_opt_muon_large_classes.argtypes = [C.c_void_p, C.POINTER(OptMuonClass), C.c_int32, C.POINTER(C.c_int32)]
            L.avmoe_opt_muon_step_large.restype = C.c_int
            # ... avmoe_opt_muon_step's, then the large image (DEVICE, HOST), n_large, the large workspace and report
            L.avmoe_opt_muon_step_large.argtypes = L.avmoe_opt_muon_step.argtypes + [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
            L.avmoe_opt_muon_ns_large.restype = C.c_int
            L.avmoe_opt_muon_ns_large.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    if hasattr(L, "avmoe_opt_swap_buffers"):         # (found by symbol: the averaged buffers)
        L.avmoe_opt_buffer_table_bytes.restype = C.c_size_t
        L.avmoe_opt_buffer_table_bytes.argtypes = [C.POINTER(OptBuffer), C.c_int32, C.POINTER(C.c_int64)]
        for name, args in (("buffer_table_build", [C.POINTER(OptBuffer), C.c_int32, C.c_void_p, C.c_size_t]),
                           ("ema_buffers", [C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p]),
                           ("swap_buffers", [C.c_void_p, C.c_int32, C.c_int64, C.c_void_p])):
            fn = getattr(L, "avmoe_opt_" + name)
            fn.restype, fn.argtypes = C.c_int, args
    if hasattr(L, "avmoe_nxn_strip"):                # (found by symbol: one strip kernel of the N x N block on raw operands, tests only)
        L.avmoe_nxn_strip.restype = C.c_int
        L.avmoe_nxn_strip.argtypes = [C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32] + [C.c_void_p] * 5
    L.avmoe_moe_buffer_info.restype = C.c_int
    L.avmoe_moe_buffer_info.argtypes = [C.POINTER(MoeDesc), C.c_int32, C.POINTER(C.c_char_p), C.POINTER(C.c_int32),
                                        C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]


def expert_prefixes(E_m: int, E_s: int) -> List[str]:
    return [f"multimodal_experts.{j}" for j in range(E_m)] + [f"singlemodal_experts.{j}" for j in range(E_s)]


def make_ptrs(tensors: Dict[str, "object"], E_m: int, E_s: int) -> MoePtrs:
    """Fill a MoePtrs from {state_dict key: CUDA fp32 tensor}.  Missing keys stay NULL.  The caller keeps
    the tensors alive for the duration of the call."""
    import torch
    P = MoePtrs()
    for k, f in TOP_KEY_TO_FIELD.items():
        t = tensors.get(k)
        if t is not None:
            assert t.dtype == torch.float32 and t.is_contiguous(), k
            setattr(P, f, t.data_ptr())
    for j, pre in enumerate(expert_prefixes(E_m, E_s)):
        for leaf, f in EXPERT_KEY_TO_FIELD.items():
            t = tensors.get(f"{pre}.{leaf}")
            if t is not None:
                assert t.dtype == (torch.int64 if f in INT64_FIELDS else torch.float32) and t.is_contiguous(), (pre, leaf)
                setattr(P.e[j], f, t.data_ptr())
    return P


class PtrFiller:
    """Fills MoePtrs structs for a FIXED list of state_dict keys: the key -> (expert, field) resolution is done once, a call then
    only writes one data_ptr per tensor (the per-call cost of the facade matters at small batches: 48 sites per AVE step)."""

    def __init__(self, keys, E_m: int, E_s: int):
        pre = expert_prefixes(E_m, E_s)
        self.slots = []                                   # (expert index or -1, field name) per key; None for keys the ABI does not take
        for k in keys:
            slot = None
            if k in TOP_KEY_TO_FIELD:
                slot = (-1, TOP_KEY_TO_FIELD[k])
            else:
                for j, pr in enumerate(pre):
                    if k.startswith(pr + "."):
                        f = EXPERT_KEY_TO_FIELD.get(k[len(pr) + 1:])
                        if f is not None:
                            slot = (j, f)
                        break
            self.slots.append(slot)

    def fill(self, P: MoePtrs, tensors, base_ptr: int = 0, offsets=None):
        """tensors: in key order (None entries are skipped; the caller vouches for contiguous fp32); with `offsets` (elements of
        fp32) the pointers are base_ptr + 4 * offset."""
        ex = {}                                           # P.e[j] builds a new ctypes view on every access: fetch each once
        for i, slot in enumerate(self.slots):
            if slot is None:
                continue
            if offsets is not None:
                ptr = base_ptr + 4 * offsets[i]
            else:
                t = tensors[i]
                if t is None:
                    continue
                ptr = t.data_ptr()
            j = slot[0]
            if j < 0:
                setattr(P, slot[1], ptr)
            else:
                e = ex.get(j)
                if e is None:
                    e = ex[j] = P.e[j]
                setattr(e, slot[1], ptr)
        return P


def buffer_table(L, desc: MoeDesc):
    """[(name, region, offset, bytes)] of the workspace layout for `desc`."""
    out = []
    i = 0
    while True:
        name, region, off, nb = C.c_char_p(), C.c_int32(), C.c_size_t(), C.c_size_t()
        st = L.avmoe_moe_buffer_info(C.byref(desc), i, C.byref(name), C.byref(region), C.byref(off), C.byref(nb))
        if st != 0:
            break
        out.append((name.value.decode(), region.value, off.value, nb.value))
        i += 1
    return out
