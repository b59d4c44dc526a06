#!/usr/bin/env python3
"""bench.py -- clip-pairs/sec of the AVMoE adapter hot path (fwd+bwd) on MI355X.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--config cfg2|cfg1|cfg3|cfg4|cfg5] [--dtype bf16|f32] [--dump-outputs DIR] [--full] ...
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N --steps K --warmup W
    (python bench.py --gpus N without a launcher starts that launcher itself, before any GPU call, and relays rank 0's line)

A plain run does only what the headline needs: it sets up, runs W warm-up steps, times K steps, writes --dump-outputs if asked,
and prints the line (`value`, `ms_per_step`, the configuration and the path-level roofline fraction, which costs no run of its own).
Everything else the line can carry -- the repetitions of the K steps, the profiling pass, the fp32 re-run, the B = 2 leg, the CPU
baseline, the parity legs, the other configurations and the exposed all-reduce time -- runs with --full only (the --no-* options
then leave single legs out); without it those members are null.

Default workload (BASELINE.json configs[1], "cfg-2"): synthetic token tensors f_a:(S=B*T, N_a=1024, C=768),
f_v:(S, N_v=196, C=768) with B=32 clips x T=10 frames PER GPU, one adapter site = the audio-side MoEAdapter
(x=f_a, vis_token=f_v) + the visual-side MoEAdapter (x=f_v, vis_token=f_a)  [AVE net_trans_v3.py:695-698],
4 experts (2 cross-modal + 2 unimodal), bottleneck 64 (reduction 12), 2 conv groups, 32 latent tokens,
BatchNorm (training mode) + both LayerNorms on, gates = 0.5, bf16 activations with fp32 accumulation and
fp32 parameters.  One step = forward of both adapters + backward to both token tensors and every adapter /
router parameter (+ the RCCL all-reduce of those parameter gradients when N > 1).  Inputs are resident in
HBM before the timed region.  value = clips processed by all ranks / max-over-ranks time.
--config cfg1|cfg3|cfg4|cfg5: the multi-site workloads of SURVEY 8(d) (every adapter site pair of the backbone table,
positions p1 and p2; clip-pairs/s = clips through ALL of them per second).

The JSON line carries
  roofline      PATH level: algorithmic bytes per clip-pair x clip-pairs/s vs the 8 TB/s HBM peak (`frac`), the
                reference-formulation FLOPs vs the dense MFMA peak beside it (`mfma`), and with --full the dominant kernel family of a
                HIP-event profiling pass over the same step with every launch alone on the GPU (`dominant_kernel`)
and with --full also
  parity        max errors of this very build against oracle/avmoe_oracle.py at the benchmarked shapes with B = 2 clips, run the
                way the timed region runs it (AdapterPair in the same --pair mode): fp32 outputs / gradients / router indices,
                bf16 the same against the oracle on bf16-rounded inputs.  Gradients are compared KINK-AWARE: the oracle is
                re-run with the ReLU mask the HIP path actually used (avmoe_amd.debug.relu_masks), so units whose
                pre-activation lies within rounding of zero sit on the same side in both; the plain comparison is reported too
  other_configs (N = 1) 3 timed steps each of cfg-1 (the reference's own operating point: B = 2, fp32, 24 site pairs), cfg-4 and cfg-5, 2 of cfg-3,
                after the cfg-2 region, with their own ms_per_step, path-level roofline fraction and kink-aware parity
  value_f32     the same step in fp32 (the configuration held to the 1e-3 bar)
  cpu_baseline  oracle/avmoe_oracle.py (eager PyTorch, fp32) timed on this box's host cores on a bounded
                sample of the same workload (same shapes, B=2 clips), rank 0 at N=1 only

--dump-outputs DIR writes what the last timed step computed as DIR/<name>.npy (dump_outputs); the inputs and parameters are seeded, so
two builds run with the same arguments can be compared output for output.
"""
from __future__ import annotations

import argparse
import gc
import json
import os
import statistics
import subprocess
import sys
import time
from types import SimpleNamespace as NS

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0            # MI355X_MICROARCH.md: HBM3E 8 TB/s (spec)
MFMA_PEAK_TF = {"bf16": 2500.0, "f32": 157.3}
ROUND = "r06"                    # profiles/<ROUND>_pmc_traffic.json is the PMC pass that belongs to this build

# ---- workloads --------------------------------------------------------------------------------
# a site pair: (C_a, N_a, C_v, N_v, count) -- `count` identical pairs (block pairs of the stage x positions p1, p2)
HTSAT = [(96, 4096), (192, 1024), (384, 256), (768, 64)]
SWIN_B = [(128, 2304), (256, 576), (512, 144), (1024, 36)]
SWIN_L = [(192, 2304), (384, 576), (768, 144), (1536, 36)]
PVT_B5 = [(64, 3136), (128, 784), (320, 196), (512, 49)]
DEPTH_PAIRS = (2, 2, 6, 2)       # adapted block pairs per stage (net_trans_v3.py:675-680)


def _table(vis, stages, positions=2):
    return [(HTSAT[i][0], HTSAT[i][1], vis[i][0], vis[i][1], DEPTH_PAIRS[i] * positions) for i in stages]


CONFIGS = {
    # BASELINE.json configs[1]: THE metric's configuration
    "cfg2": dict(B=32, T=10, dtype="bf16", variant="ave", E_m=2, E_s=2, reduction=12, groups=2, K=32,
                 pairs=[(768, 1024, 768, 196, 1)], what="one AVMoE adapter site (audio-side + visual-side MoEAdapter)"),
    # configs[0]: AVE, batch 2, Swin-B x HTS-AT, all 12 block pairs x {p1, p2}, r = 8, fp32
    "cfg1": dict(B=2, T=10, dtype="f32", variant="ave", E_m=2, E_s=2, reduction=8, groups=2, K=32,
                 pairs=_table(SWIN_B, (0, 1, 2, 3)), what="AVE: Swin-B x HTS-AT, 12 block pairs x {p1,p2} = 24 site pairs"),
    # configs[2]: AVVP (N x N unimodal attention, LB loss), batch 64, Swin-L x HTS-AT
    "cfg3": dict(B=64, T=10, dtype="bf16", variant="avvp", E_m=2, E_s=2, reduction=8, groups=2, K=32,
                 pairs=_table(SWIN_L, (0, 1, 2, 3)), what="AVVP: Swin-L x HTS-AT, 24 site pairs, N x N unimodal attention"),
    # configs[3]: AVQA, 32 clips per GPU (256 over 8), Swin-L, 1 + 2 experts, 2 latent tokens, 4 groups
    "cfg4": dict(B=32, T=10, dtype="bf16", variant="avqa", E_m=1, E_s=2, reduction=8, groups=4, K=2,
                 pairs=_table(SWIN_L, (0, 1, 2, 3)), what="AVQA: Swin-L x HTS-AT, 24 site pairs, 1+2 experts, K=2, 4 groups"),
    # configs[4]: AVS S4, PVT-v2-b5 x HTS-AT, 4 + 4 experts, bottleneck 128 at the C=512 stage (r = 4), T = 5, K = 87 (the AVS default)
    "cfg5": dict(B=8, T=5, dtype="bf16", variant="avs", E_m=4, E_s=4, reduction=4, groups=2, K=87,
                 pairs=[(HTSAT[i][0], HTSAT[i][1], PVT_B5[i][0], PVT_B5[i][1], 2) for i in range(4)],
                 what="AVS S4: PVT-v2-b5 x HTS-AT, 8 site pairs, 4+4 experts, r=4 (bottleneck 128 at C=512), 87 latent tokens"),
}


def make_opt(c):
    return NS(num_conv_group=c["groups"], is_before_layernorm=1, is_post_layernorm=1, is_self_attention=0,
              self_attention_version="v1", num_multimodal_experts=c["E_m"], num_singlemodal_experts=c["E_s"],
              use_load_balacing_loss=1 if c["variant"] in ("avvp", "avs") else 0,
              Adapter_downsample=c["reduction"], is_bn=1, is_gate=1, num_tokens=c["K"])


def new_site(c, Cx, Nx, Cy, Ny):
    """One MoEAdapter of the configuration's task variant, built the way that task's model builds it."""
    from avmoe_amd import adapters as A
    common = dict(input_dim=Cx, output_dim=Cx, adapter_kind="bottleneck", dim_list=None, layer_idx=0, opt=make_opt(c),
                  conv_dim_in=Ny, conv_dim_out=Nx, linear_in=Cy, linear_out=Cx)
    if c["variant"] == "avvp":
        return A.MoEAdapterAVVP(**common)
    if c["variant"] == "avqa":
        return A.MoEAdapterAVQA(reduction_factor=c["reduction"], use_bn=True, use_gate=True, **common)
    cls = A.MoEAdapterAVS if c["variant"] == "avs" else A.MoEAdapter
    return cls(reduction_factor=c["reduction"], use_bn=True, use_gate=True, num_tk=c["K"], **common)


def build_pair(c, shape, device, seed=0):
    """The two MoEAdapters of one site pair, reference default init (seed), then gates <- 0.5."""
    import torch
    C_a, N_a, C_v, N_v = shape
    torch.manual_seed(seed)
    audio, visual = new_site(c, C_a, N_a, C_v, N_v), new_site(c, C_v, N_v, C_a, N_a)
    for m in (audio, visual):
        with torch.no_grad():
            for k, p in m.named_parameters():
                if k.endswith(("gate", "gate_av", "gate_self")):
                    p.fill_(0.5)
        m.to(device).train()
    return audio, visual


def algorithmic_bytes_per_clip_pair(c, esz):
    """ideal fusion reads f_a,f_v (fwd) + writes 2 residuals + reads 2 upstream grads + re-reads
    f_a,f_v (bwd) + writes 2 input grads = 5 passes over both token tensors, per site pair."""
    return sum(5.0 * c["T"] * (Na * Ca + Nv * Cv) * esz * cnt for Ca, Na, Cv, Nv, cnt in c["pairs"])


def reference_flops_forward(Cx, Nx, Cy, Ny, S, E_m, E_s, d, g, K, nxn=False):
    """Algorithmic FLOPs of one MoEAdapter forward in the reference's formulation (multiply-add = 2): token
    remap + fc, router, the four latent-attention products per cross-modal expert, grouped down + up, mixture
    (+ the N x N block of the AVVP unimodal experts)."""
    E = E_m + E_s
    f = 2.0 * S * Nx * Ny * Cy + 2.0 * S * Nx * Cy * Cx
    f += 2.0 * S * (2 * Cx * 128 + 128 * 32 + 32 * E)
    f += E_m * 8.0 * S * K * Cx * Nx
    f += E * 4.0 * S * Nx * Cx * d / g
    f += 2.0 * S * E * Cx * Nx
    if nxn:
        f += E_s * 4.0 * S * Nx * Nx * Cx
    return f


def reference_flops_per_clip_pair(c):
    tot = 0.0
    for Ca, Na, Cv, Nv, cnt in c["pairs"]:
        kw = dict(S=c["T"], E_m=c["E_m"], E_s=c["E_s"], g=c["groups"], K=c["K"], nxn=c["variant"] == "avvp")
        tot += cnt * 3.0 * (reference_flops_forward(Ca, Na, Cv, Nv, d=Ca // c["reduction"], **kw) +
                            reference_flops_forward(Cv, Nv, Ca, Na, d=Cv // c["reduction"], **kw))
    return tot


# ---- CPU legs (rank 0, N = 1): the oracle as timed baseline AND as parity checker ------------------------------------
def _oracle_cfgs(c, shape):
    from oracle import avmoe_oracle as O
    Ca, Na, Cv, Nv = shape
    kw = dict(E_m=c["E_m"], E_s=c["E_s"], reduction=c["reduction"], groups=c["groups"], K=c["K"],
              variant=c["variant"], lb_loss=c["variant"] in ("avvp", "avs"))
    return O.AdapterConfig(Cx=Ca, Nx=Na, Cy=Cv, Ny=Nv, **kw), O.AdapterConfig(Cx=Cv, Nx=Nv, Cy=Ca, Ny=Na, **kw)


def cpu_baseline(c, budget_s=15.0, min_timed=3):
    """Eager-PyTorch fp32 oracle on the host cores, same shapes at B=2: 1 warm-up, then timed steps until ~budget_s of
    CPU work (min_timed .. 8 of them); the median is reported.  Returns (json object, the inputs / parameters / results of the last
    step: parity_check compares the HIP path with them)."""
    import torch
    from oracle import avmoe_oracle as O
    # eager PyTorch on many tiny bmm/softmax ops gets SLOWER past a few dozen threads (measured on the 256-thread
    # GPU host: 132 s/step with 256 threads); use at most 32 and report the number actually used
    cores = min(os.cpu_count() or 1, 32)
    torch.set_num_threads(cores)
    Bc = 2
    S = Bc * c["T"]
    work = []
    g = torch.Generator().manual_seed(1234)
    for i, (Ca, Na, Cv, Nv, cnt) in enumerate(c["pairs"]):
        ca, cv = _oracle_cfgs(c, (Ca, Na, Cv, Nv))
        Pa, Ba = O.init_params(ca, seed=2 * i)
        Pv, Bv = O.init_params(cv, seed=2 * i + 1)
        fa = 0.3 * torch.randn(S, Na, Ca, generator=g)
        fv = 0.3 * torch.randn(S, Nv, Cv, generator=g)
        ga, gv = torch.randn(fa.shape, generator=g), torch.randn(fv.shape, generator=g)
        work.append(dict(ca=ca, cv=cv, Pa=Pa, Ba=Ba, Pv=Pv, Bv=Bv, fa=fa, fv=fv, ga=ga, gv=gv, cnt=cnt))
    lbw = 0.01 if c["variant"] in ("avvp", "avs") else 0.0
    times = []
    t_start = time.time()
    for it in range(9):
        for w in work:      # the `cnt` site pairs of a stage have the same shapes: time one, scale
            t0 = time.time()
            w["ra"] = O.moe_forward_backward(w["Pa"], w["Ba"], w["fa"], w["fv"], w["ca"], w["ga"], training=True, lb_weight=lbw)
            w["rv"] = O.moe_forward_backward(w["Pv"], w["Bv"], w["fv"], w["fa"], w["cv"], w["gv"], training=True, lb_weight=lbw)
            w["dt"] = time.time() - t0
        dt = sum(w["dt"] * w["cnt"] for w in work)
        if it > 0:
            times.append(dt)
        if time.time() - t_start > budget_s and len(times) >= min_timed:
            break
    med = statistics.median(times)
    obj = dict(value=Bc / med, unit="clip-pairs/s", cores=cores, host_cores=os.cpu_count(), kind="port", dtype="f32", clips=Bc,
               sample=f"oracle/avmoe_oracle.py eager PyTorch fp32, {c['name']} shapes at B={Bc} clips (S={S} frames), "
                      f"{len(times)} timed fwd+bwd steps after 1 warm-up, median {med:.2f} s/step "
                      f"(one site pair per distinct shape timed, x its multiplicity), {torch.get_num_threads()} of {os.cpu_count()} host threads; "
                      f"the GPU value is {c['dtype']} at B={c['B']} clips")
    return obj, (work, lbw)


def parity_check(c, material, device, pair_mode="concurrent"):
    """parity_check_ with the library's size thresholds lifted (avmoe_test_hooks): the
    B = 2 shapes then run through the SAME streaming kernels (dpost_pair, tok_pair2) the timed region's full batch takes."""
    from avmoe_amd import _capi
    with _capi.test_hooks(_capi.HOOK_ALL_FORCE):
        res = parity_check_(c, material, device, pair_mode)
    res["kernels"] = "the timed region's: size thresholds of dpost_pair / tok_pair2 / hop1_stream / tile_stream lifted for the B = 2 shapes (avmoe_test_hooks)"
    return res


def parity_check_(c, material, device, pair_mode="concurrent"):
    """This build against the oracle at the benchmarked shapes, B = 2 clips, through the C ABI behind the module API -- the two
    sites of a pair run the way the timed region runs them (AdapterPair in `pair_mode`; two module calls with --pair off), so each token tensor's gradient is the sum of its dX from one site and its dY from the other.
    fp32: outputs max-abs relative to the tensor's max, indices bit-exact, gradients norm-wise per tensor (+ token rows of the
    audio gradient one by one).  bf16: against the oracle evaluated on the bf16-rounded inputs.
    Kink-aware: at these sizes (10^5 .. 10^6 ReLU units per cross-modal expert) a few pre-activations lie within rounding of zero
    in ANY draw; there the mask -- and with it that token's gradient row and ~1/sqrt(tokens) of every sum over tokens -- is decided
    by rounding, in the oracle as much as here.  The HIP path's own mask is read back (avmoe_amd.debug.relu_masks), the oracle is
    re-run with `relu(z)` replaced by `z * mask` (identical wherever mask == z > 0) and the gradients are compared with THAT run:
    `grad_rel_f32` / `grad_relnorm_bf16_same_mask`.  `relu_units_flipped` counts the units where the two masks differ and
    `flipped_preact_max_rel` is the largest |pre-activation| among them relative to the rms pre-activation (rounding-sized, or
    there is a bug); the comparison against the oracle's own mask stays in the line as `grad_rel_f32_own_mask` / `grad_relnorm_bf16`."""
    import torch
    from oracle import avmoe_oracle as O
    from avmoe_amd.adapters import AdapterPair
    from avmoe_amd import debug as dbg
    work, lbw = material
    can_pair = pair_mode != "off"
    res = dict(clips=2, path=(f"AdapterPair(--pair {pair_mode})" if can_pair else "two module calls"), idx_equal=True,
               out_rel_f32=0.0, grad_rel_f32=0.0, worst_f32=None, grad_rel_f32_own_mask=0.0, worst_f32_own_mask=None,
               relu_units=0, relu_units_flipped=0, flipped_preact_max_rel=0.0,
               out_rel_bf16=None, grad_relnorm_bf16=None, worst_bf16=None, grad_relnorm_bf16_same_mask=None, worst_bf16_same_mask=None,
               grad_relnorm_bf16_major=None, worst_bf16_major=None, grad_relnorm_bf16_tiny_joint=None, grad_eps_bf16_single_sums=None, worst_bf16_single_sums=None, grad_relnorm_bf16_vectors=None, worst_bf16_vectors=None,
               dx_rows=0, **{"dx_rows_above_1e-3": 0}, dx_row_maxabs_f32=0.0,
               measures="out_*: max-abs / max ; grad_*: norm-wise per tensor, worst tensor (floor 1e-3 of the largest gradient norm) ; "
                        "grad_rel_f32, *_same_mask, dx_rows*: against the oracle run with the HIP path's ReLU mask (kink-aware) ; "
                        "*_own_mask, grad_relnorm_bf16: against the oracle's own mask ; dx_rows_above_1e-3: token rows of the audio-token "
                        "gradient (fp32) whose max-abs error exceeds 1e-3 of its max")
    detail = [] if os.environ.get("AVMOE_PARITY_DETAIL") else None          # dev: per-tensor errors to stderr

    def hip(w, bf16, Ga, Gv):
        """both sites of the pair on the HIP path -> (out_a, out_v, idx_a, idx_v, grads_a, grads_v, token grads, masks_a, masks_v)"""
        ca, cv = w["ca"], w["cv"]
        ma, mv = new_site(c, ca.Cx, ca.Nx, ca.Cy, ca.Ny), new_site(c, cv.Cx, cv.Nx, cv.Cy, cv.Ny)
        ma.load_state_dict({**w["Pa"], **w["Ba"]}); mv.load_state_dict({**w["Pv"], **w["Bv"]})
        for m in (ma, mv):
            m.to(device).train()
            dbg.keep_saved(m)
        tdt = torch.bfloat16 if bf16 else torch.float32
        fa, fv = w["fa"].to(device, tdt).requires_grad_(True), w["fv"].to(device, tdt).requires_grad_(True)
        xa, xv = fa.permute(0, 2, 1).unsqueeze(-1), fv.permute(0, 2, 1).unsqueeze(-1)
        lbs, idx_a, idx_v = [], None, None
        pair = AdapterPair(ma, mv, concurrent=(pair_mode != "serial")) if can_pair else None
        if pair is not None and pair_mode == "same":
            pair.same_stream = True
        if can_pair and c["variant"] == "avs":
            out_a, idx_a, _p, lb_a, out_v, idx_v, _q, lb_v = pair(xa, xv, is_training=False)
            lbs = [lb_a, lb_v]
        elif can_pair and c["variant"] == "avvp":
            out_a, lb_a, out_v, lb_v = pair(xa, xv)
            lbs = [lb_a, lb_v]
        elif can_pair:
            out_a, idx_a, out_v, idx_v = pair(xa, xv)
        elif c["variant"] == "avs":
            out_a, idx_a, _p, lb_a = ma(xa, xv, is_training=False)
            out_v, idx_v, _p, lb_v = mv(xv, xa, is_training=False)
            lbs = [lb_a, lb_v]
        elif c["variant"] == "avvp":
            (out_a, lb_a), (out_v, lb_v) = ma(xa, xv), mv(xv, xa)
            lbs = [lb_a, lb_v]
        else:
            (out_a, idx_a), (out_v, idx_v) = ma(xa, xv), mv(xv, xa)
        ota, otv = out_a.squeeze(-1).permute(0, 2, 1), out_v.squeeze(-1).permute(0, 2, 1)
        loss = (ota.float() * Ga.to(device)).sum() + (otv.float() * Gv.to(device)).sum()
        for lb in lbs:
            if torch.is_tensor(lb) and lbw:
                loss = loss + lbw * lb
        loss.backward()
        torch.cuda.synchronize()
        ga = {k: p.grad.float().cpu() for k, p in ma.named_parameters()}
        gv = {k: p.grad.float().cpu() for k, p in mv.named_parameters()}
        tok = dict(fa=fa.grad.float().cpu(), fv=fv.grad.float().cpu())
        flat = lambda i: i.reshape(-1).cpu() if i is not None else None
        return (ota.detach().float().cpu(), otv.detach().float().cpu(), flat(idx_a), flat(idx_v), ga, gv, tok, dbg.relu_masks(ma), dbg.relu_masks(mv))

    def oracle(w, fa, fv, Ga, Gv, masks=(None, None), recs=(None, None)):
        ra = O.moe_forward_backward(w["Pa"], w["Ba"], fa, fv, w["ca"], Ga, training=True, lb_weight=lbw, relu_masks=masks[0], record=recs[0])
        rv = O.moe_forward_backward(w["Pv"], w["Bv"], fv, fa, w["cv"], Gv, training=True, lb_weight=lbw, relu_masks=masks[1], record=recs[1])
        return ra, rv

    def grad_items(got, ra, rv):
        """(tag, key, HIP tensor, oracle tensor) over both sites' parameters and the two (summed) token gradients"""
        ga, gv, tok = got
        items = [("a", k, ga[k], v) for k, v in ra[1].items() if k not in ("X", "Y")]
        items += [("v", k, gv[k], v) for k, v in rv[1].items() if k not in ("X", "Y")]
        items += [("tok", "f_a", tok["fa"], ra[1]["X"] + rv[1]["Y"]), ("tok", "f_v", tok["fv"], rv[1]["X"] + ra[1]["Y"])]
        return items

    def worst(items, floor_rel=1e-3, skip_small=False, min_numel=0, log=True):
        nmax = max(float(v.norm()) for _t, _k, _g, v in items)
        e_w, k_w = 0.0, None
        for tag, k, g, v in items:
            if (skip_small and float(v.norm()) < floor_rel * nmax) or v.numel() < min_numel:
                continue
            e = float((g - v).norm()) / max(float(v.norm()), floor_rel * nmax)
            if detail is not None and log:
                detail.append((tag, k, e))
            if e > e_w:
                e_w, k_w = e, f"{k} ({tag})"
        return e_w, k_w

    def split_view(items):
        """the same comparison the way the -m gpu tests bar it (tests/golden_util.py::bf16_budget_violations): the tensors of <= 16
        elements (scalar gates, the router's last bias: single sums of both signs over every token, each of which can cancel to a
        small fraction of its terms) as ONE vector; the tensors that carry >= 1 % of the largest gradient norm one by one; every
        other tensor (more than 16 elements, below 1 % of the largest norm: fc.bias, router.0.bias, ...) as one vector again; the
        structurally zero ones (a bias in front of a train-mode BatchNorm: < 1e-6 of the largest norm) by their absolute error relative
        to the largest norm (pure rounding noise of sums that cancel exactly: eager autocast leaves 0.3 - 2 % there)"""
        nmax = max(float(v.norm()) for _t, _k, _g, v in items)
        tiny = [(g, v) for _t, _k, g, v in items if v.numel() <= 16]
        tj = None
        if tiny:
            gt, vt = torch.cat([g.reshape(-1) for g, _ in tiny]), torch.cat([v.reshape(-1) for _, v in tiny])
            tj = float((gt - vt).norm() / vt.norm().clamp_min(1e-30))
        e_w, k_w = 0.0, None
        rest = []                                # > 16 elements and < 1 % of the largest norm: barred as ONE vector too -- no tensor is in neither view
        sz = 0.0                                 # ... except the STRUCTURALLY ZERO ones (below 1e-6 of the largest norm: a bias in front of a train-mode
        for tag, k, g, v in items:               # BatchNorm -- exactly zero in real arithmetic), barred in absolute terms: ||g - v|| / largest norm
            if v.numel() <= 16:
                continue
            if float(v.norm()) < 1e-6 * nmax:
                sz = max(sz, float((g - v).norm()) / nmax)
                continue
            if float(v.norm()) < 1e-2 * nmax:
                rest.append((g, v))
                continue
            e = float((g - v).norm() / v.norm())
            if e > e_w:
                e_w, k_w = e, f"{k} ({tag})"
        rj = None
        if rest:
            gr, vr = torch.cat([g.reshape(-1) for g, _ in rest]), torch.cat([v.reshape(-1) for _, v in rest])
            rj = float((gr - vr).norm() / vr.norm().clamp_min(1e-30))
        return tj, e_w, k_w, rj, sz

    def upd(key_e, key_w, e, k):
        if e > (res[key_e] or 0.0):
            res[key_e], res[key_w] = e, k

    for w in work:
        shape_tag = f"C_a={w['ca'].Cx},N_a={w['ca'].Nx}"
        for bf16 in ([False, True] if c["dtype"] == "bf16" else [False]):
            if bf16:
                fa, fv, Ga, Gv = (t.bfloat16().float() for t in (w["fa"], w["fv"], w["ga"], w["gv"]))
                ra, rv = oracle(w, fa, fv, Ga, Gv)
            else:
                fa, fv, Ga, Gv = w["fa"], w["fv"], w["ga"], w["gv"]
                ra, rv = w["ra"], w["rv"]                       # the CPU-baseline leg's last step: the oracle on its own mask
            oa, ov, ia, iv, ga, gv, tok, mka, mkv = hip(w, bf16, Ga, Gv)
            for i_h, r in ((ia, ra), (iv, rv)):
                if i_h is not None:
                    res["idx_equal"] = res["idx_equal"] and bool(torch.equal(i_h, r[0]["idx"]))
            e_out = max(float((oa - ra[0]["out"]).abs().max() / ra[0]["out"].abs().max()), float((ov - rv[0]["out"]).abs().max() / rv[0]["out"].abs().max()))
            reca, recv = {}, {}
            sa, sv = oracle(w, fa, fv, Ga, Gv, masks=(mka, mkv), recs=(reca, recv))      # the oracle on the HIP path's mask
            e_own, k_own = worst(grad_items((ga, gv, tok), ra, rv), skip_small=bf16)
            e_same, k_same = worst(grad_items((ga, gv, tok), sa, sv), skip_small=bf16)
            if not bf16:
                res["out_rel_f32"] = max(res["out_rel_f32"], e_out)
                upd("grad_rel_f32", "worst_f32", e_same, f"{k_same} [{shape_tag}]")
                upd("grad_rel_f32_own_mask", "worst_f32_own_mask", e_own, f"{k_own} [{shape_tag}]")
                for rec, mk in ((reca, mka), (recv, mkv)):
                    for pre, z in rec.items():
                        flip = mk[pre] != (z > 0)
                        res["relu_units"] += z.numel()
                        res["relu_units_flipped"] += int(flip.sum())
                        if bool(flip.any()):
                            res["flipped_preact_max_rel"] = max(res["flipped_preact_max_rel"], float(z[flip].abs().max() / z.pow(2).mean().sqrt()))
                ref_fa = sa[1]["X"] + sv[1]["Y"]
                row_err = (tok["fa"] - ref_fa).abs().amax(-1) / ref_fa.abs().max()
                res["dx_rows"] += row_err.numel()
                res["dx_rows_above_1e-3"] += int((row_err > 1e-3).sum())
                res["dx_row_maxabs_f32"] = max(res["dx_row_maxabs_f32"], float(row_err.max()))
            else:
                res["out_rel_bf16"] = max(res["out_rel_bf16"] or 0.0, e_out)
                upd("grad_relnorm_bf16", "worst_bf16", e_own, f"{k_own} [{shape_tag}]")
                upd("grad_relnorm_bf16_same_mask", "worst_bf16_same_mask", e_same, f"{k_same} [{shape_tag}]")
                tj, e_major, k_major, rj, sz = split_view(grad_items((ga, gv, tok), sa, sv))
                res["grad_abs_bf16_structural_zero"] = max(res.get("grad_abs_bf16_structural_zero") or 0.0, sz)
                upd("grad_relnorm_bf16_major", "worst_bf16_major", e_major, f"{k_major} [{shape_tag}]")
                if tj is not None:
                    res["grad_relnorm_bf16_tiny_joint"] = max(res.get("grad_relnorm_bf16_tiny_joint") or 0.0, tj)
                if rj is not None:
                    res["grad_relnorm_bf16_rest"] = max(res.get("grad_relnorm_bf16_rest") or 0.0, rj)
                # ---- every tensor ONE BY ONE, anchored on the reference formulation's own bf16 error ----
                # (a) tensors of more than 16 elements (>= 1e-3 of the largest gradient norm; the structurally zero ones have their own view above):
                #     norm-wise error on this draw, next to the error of the reference formulation run eagerly under torch.autocast(bfloat16) on the
                #     same inputs (own mask).  Listed when above 5 % AND above that eager error.
                # (b) single-sum tensors (<= 16 elements: the scalar gates, the router's last bias) over SEVERAL draws of the upstream gradient with
                #     the forward fixed.  <G, y> for a random G: value and rounding error are both zero-mean sums over the same ~1e6 terms, so the
                #     relative error of ONE draw is a ratio of two normals -- heavy-tailed; 10 - 50 x outliers on a few of ~100 scalars are chance
                #     (profiles/r06_gate_grad_draws.txt: the eager-autocast run shows the same tail).  The estimate without that tail is
                #     eps = rms_k(hip_k - oracle_k) / rms_k(oracle_k) over the draws k.  Listed when above 5 % AND above the eager eps.
                if SINGLE_SUM_DRAWS > 1:
                  try:          # (a checker-side view: whatever goes wrong in it must not cost the line -- it then carries the message instead)
                    def eager_run(P, B, X, Y, cfg, Gl, keys):
                        """the oracle's formulation eagerly on the GPU under bf16 autocast: (all gradients of the first draw, `keys` for the others)"""
                        Pd, Bd = {k: v.to(device) for k, v in P.items()}, {k: v.to(device) for k, v in B.items()}
                        with torch.autocast("cuda", dtype=torch.bfloat16):
                            full = O.moe_forward_backward(Pd, Bd, X.to(device), Y.to(device), cfg, Gl[0].to(device), training=True, lb_weight=lbw)[1]
                            rest = O.moe_grads_over_draws(Pd, Bd, X.to(device), Y.to(device), cfg, [g_.to(device) for g_ in Gl[1:]], keys, training=True, lb_weight=lbw)
                        return {k: v.float().cpu() for k, v in full.items()}, [{k: v.float().cpu() for k, v in r_.items()} for r_ in rest]
                    keys_a = [k for k, v in sa[1].items() if k not in ("X", "Y") and v.numel() <= 16]
                    keys_v = [k for k, v in sv[1].items() if k not in ("X", "Y") and v.numel() <= 16]
                    gd = torch.Generator().manual_seed(4321)
                    draws = [(torch.randn(fa.shape, generator=gd).bfloat16().float(), torch.randn(fv.shape, generator=gd).bfloat16().float())
                             for _ in range(SINGLE_SUM_DRAWS - 1)]
                    refs_a = O.moe_grads_over_draws(w["Pa"], w["Ba"], fa, fv, w["ca"], [d_[0] for d_ in draws], keys_a, lb_weight=lbw, relu_masks=mka)
                    refs_v = O.moe_grads_over_draws(w["Pv"], w["Bv"], fv, fa, w["cv"], [d_[1] for d_ in draws], keys_v, lb_weight=lbw, relu_masks=mkv)
                    ea, ea_d = eager_run(w["Pa"], w["Ba"], fa, fv, w["ca"], [Ga] + [d_[0] for d_ in draws], keys_a)
                    ev, ev_d = eager_run(w["Pv"], w["Bv"], fv, fa, w["cv"], [Gv] + [d_[1] for d_ in draws], keys_v)
                    tok_e = dict(fa=ea["X"] + ev["Y"], fv=ev["X"] + ea["Y"])
                    items_h, items_e = grad_items((ga, gv, tok), sa, sv), grad_items((ea, ev, tok_e), sa, sv)
                    nmax = max(float(v.norm()) for _t, _k, _g, v in items_h)
                    above = res.setdefault("bf16_tensors_above_5pct_and_eager", [])
                    for (tag, k, g_h, v), (_t2, _k2, g_e, _v2) in zip(items_h, items_e):
                        if v.numel() <= 16 or float(v.norm()) < 1e-3 * nmax:
                            continue
                        e_h, e_e = float((g_h - v).norm() / v.norm()), float((g_e - v).norm() / v.norm())
                        upd("grad_relnorm_bf16_vectors", "worst_bf16_vectors", e_h, f"{k} ({tag}) [{shape_tag}] (eager {e_e:.3f})")
                        res["bf16_tensors_compared"] = res.get("bf16_tensors_compared", 0) + 1
                        if e_h > 5e-2 and e_h > e_e:
                            above.append(f"{k} ({tag}) [{shape_tag}] {e_h:.3f} (eager {e_e:.3f})")
                    acc = {}
                    def add(tag, k, g, g_e, v):
                        s_ = acc.setdefault(f"{k} ({tag})", [0.0, 0.0, 0.0])
                        s_[0] += float((g - v).pow(2).sum()); s_[1] += float((g_e - v).pow(2).sum()); s_[2] += float(v.pow(2).sum())
                    for k in keys_a: add("a", k, ga[k], ea[k], sa[1][k])
                    for k in keys_v: add("v", k, gv[k], ev[k], sv[1][k])
                    for (Ga_k, Gv_k), r_a, r_v, e_a, e_v in zip(draws, refs_a, refs_v, ea_d, ev_d):
                        _oa, _ov, _ia, _iv, ga_k, gv_k, _tok, mka_k, mkv_k = hip(w, True, Ga_k, Gv_k)
                        if not (all(torch.equal(mka_k[p_], mka[p_]) for p_ in mka) and all(torch.equal(mkv_k[p_], mkv[p_]) for p_ in mkv)):
                            res["single_sum_view_error"] = "the ReLU mask of a repeated forward differs (the forward does not depend on the upstream gradient)"
                        for k in keys_a: add("a", k, ga_k[k], e_a[k], r_a[k])
                        for k in keys_v: add("v", k, gv_k[k], e_v[k], r_v[k])
                    for name, (se, see, sr) in acc.items():
                        rms = (sr / SINGLE_SUM_DRAWS) ** 0.5
                        if rms < 1e-3 * nmax:          # below 1e-3 of the largest gradient norm (incl. the structurally zero ones: a bias in front of a train-mode BatchNorm)
                            continue
                        e_h, e_e = (se / sr) ** 0.5, (see / sr) ** 0.5
                        upd("grad_eps_bf16_single_sums", "worst_bf16_single_sums", e_h, f"{name} [{shape_tag}] (eager {e_e:.3f})")
                        res["bf16_tensors_compared"] = res.get("bf16_tensors_compared", 0) + 1
                        if e_h > 5e-2 and e_h > e_e:
                            above.append(f"{name} [{shape_tag}] eps {e_h:.3f} (eager {e_e:.3f})")
                    res["single_sum_draws"] = SINGLE_SUM_DRAWS
                  except Exception as e:
                    res["single_sum_view_error"] = f"{type(e).__name__}: {e}"
                    res.pop("bf16_tensors_above_5pct_and_eager", None)          # (not measured: ok_bf16_grads falls back to the single-draw criterion)
    for k in ("out_rel_f32", "grad_rel_f32", "grad_rel_f32_own_mask", "flipped_preact_max_rel", "out_rel_bf16", "grad_relnorm_bf16",
              "grad_relnorm_bf16_same_mask", "grad_eps_bf16_single_sums", "grad_relnorm_bf16_vectors", "grad_relnorm_bf16_major", "grad_relnorm_bf16_tiny_joint", "grad_relnorm_bf16_rest", "grad_abs_bf16_structural_zero", "dx_row_maxabs_f32"):
        if res.get(k) is not None:
            res[k] = float(f"{res[k]:.3e}")
    if detail:
        for row in sorted(detail, key=lambda r: -r[2])[:25]:
            print("parity %-4s %-46s err %.3e" % row[:3], file=sys.stderr)
    res["checked_against"] = "oracle/avmoe_oracle.py (pinned on the reference's vectors: tests/test_oracle_golden.py)"
    return parity_verdict(res)


# The bars of the parity leg (the same numbers the -m gpu tests assert).  HARD ones fail the run (non-zero exit AFTER the line is
# printed): the fp32 path is the one held to north_star's 1e-3, indices are bit-exact, and a bf16 output off by more than the test
# bound is a bug (round 3: a run-to-run blip of the cfg-3 forward went unnoticed because this leg only printed numbers).  The bf16
# gradient bar is reported as `ok_bf16_grads` (SOFT: bf16 activations have an error budget of their own).
SINGLE_SUM_DRAWS = 6          # upstream-gradient draws of the bf16 parity leg's single-sum view (1 = off)
PARITY_BARS = dict(out_rel_f32=1e-3, grad_rel_f32=1e-3, out_rel_bf16=1e-2, grad_relnorm_bf16_same_mask=5e-2, grad_relnorm_bf16_major=5e-2,
                   grad_relnorm_bf16_tiny_joint=5e-2, grad_relnorm_bf16_rest=5e-2, grad_abs_bf16_structural_zero=1e-2)
# members that are the same in every parity object: the headline `parity` carries them, the other configurations' objects leave them out
PARITY_CONSTANT_KEYS = ("measures", "bars", "kernels", "checked_against")


def parity_verdict(res):
    """adds ok / ok_bf16_grads / failed (list of the keys above their bar) to a parity object"""
    failed = [] if res.get("idx_equal", True) else ["idx_equal"]
    for k in ("out_rel_f32", "grad_rel_f32", "out_rel_bf16"):
        if res.get(k) is not None and not (res[k] <= PARITY_BARS[k]):
            failed.append(k)
    soft = res.get("grad_relnorm_bf16_same_mask")
    res["ok"] = not failed
    res["ok_bf16_grads_single_draw"] = None if soft is None else bool(soft <= PARITY_BARS["grad_relnorm_bf16_same_mask"])      # rounds 2 - 5's `ok_bf16_grads`: every tensor >= 1e-3 of the largest norm one by one on ONE draw of the upstream gradient, 5 % flat (for a single sum: a ratio of two normals)
    above = res.get("bf16_tensors_above_5pct_and_eager")
    # every tensor >= 1e-3 of the largest norm one by one (vectors on the one draw, single sums as rms error / rms value over `single_sum_draws` draws):
    # none above 5 % AND above the error of the reference formulation itself under bf16 autocast on the same inputs
    res["ok_bf16_grads"] = res["ok_bf16_grads_single_draw"] if above is None else bool(len(above) == 0)
    mj, tj, rj = res.get("grad_relnorm_bf16_major"), res.get("grad_relnorm_bf16_tiny_joint"), res.get("grad_relnorm_bf16_rest")
    res["ok_bf16_grads_as_tested"] = None if mj is None else bool(mj <= PARITY_BARS["grad_relnorm_bf16_major"] and (tj is None or tj <= PARITY_BARS["grad_relnorm_bf16_tiny_joint"])
                                                                  and (rj is None or rj <= PARITY_BARS["grad_relnorm_bf16_rest"])
                                                                  and (res.get("grad_abs_bf16_structural_zero") or 0.0) <= PARITY_BARS["grad_abs_bf16_structural_zero"])      # four views that cover every tensor
    res["failed"] = failed
    res["bars"] = PARITY_BARS
    return res


# ---- launcher ------------------------------------------------------------------------------------------------------
def self_launch(args, argv):
    """--gpus N > 1 without a launcher environment: start `torch.distributed.run` with N ranks as a CHILD process -- before
    this process has touched the GPU -- and relay its output (rank 0 prints the JSON line)."""
    port = int(os.environ.get("MASTER_PORT", 29500 + os.getpid() % 2000))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + argv
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    proc = subprocess.run(cmd, env=env)
    raise SystemExit(proc.returncode)


class Workload:
    """Modules + resident inputs + the step function of one configuration on this rank's GPU."""

    def __init__(self, c, tdt, device, rank, world, pair_mode):
        import torch
        from avmoe_amd.dp import AdapterGradReducer
        from avmoe_amd.adapters import AdapterPair
        self.c, self.world, self.device = c, world, device
        self.can_pair = True
        self.pair_mode = pair_mode
        S = c["B"] * c["T"]
        self.lbw = 0.01 if c["variant"] in ("avvp", "avs") else 0.0
        g = torch.Generator(device="cpu").manual_seed(1234 + rank)
        self.work, sites = [], []
        for i, (Ca, Na, Cv, Nv, cnt) in enumerate(c["pairs"]):      # the `cnt` pairs of a shape share the inputs, not the modules
            f_a = (0.3 * torch.randn(S, Na, Ca, generator=g)).to(device, tdt).requires_grad_(True)
            f_v = (0.3 * torch.randn(S, Nv, Cv, generator=g)).to(device, tdt).requires_grad_(True)
            g_a = torch.randn(S, Na, Ca, generator=g).to(device, tdt)
            g_v = torch.randn(S, Nv, Cv, generator=g).to(device, tdt)
            mods = []
            for j in range(cnt):
                a, v = build_pair(c, (Ca, Na, Cv, Nv), device, seed=100 * i + j)
                pr = AdapterPair(a, v, concurrent=(self.pair_mode != "serial")) if self.can_pair else None
                if pr is not None and self.pair_mode == "same":
                    pr.same_stream = True
                mods.append((a, v, pr))
                sites += [a, v]
            self.work.append(dict(f_a=f_a, f_v=f_v, ga4=g_a.permute(0, 2, 1).unsqueeze(-1), gv4=g_v.permute(0, 2, 1).unsqueeze(-1), mods=mods))
        params = [p for m in sites for p in m.parameters()]
        self.reducer = AdapterGradReducer(params, bucket_mb=64.0, sites=sites)

    def set_same_stream(self, on):
        """every AdapterPair of the workload keeps its mode's SCHEDULE (two-stream mode: dX overwrites, dY adds behind the other
        site's dX -- the kernel variants of the timed region) but issues it on the caller's stream alone (AdapterPair.same_stream):
        an event bracket around a launch then measures that launch, not the other stream's kernels.  Returns the previous setting."""
        prev = False
        for w in self.work:
            for _a, _v, pr in w["mods"]:
                if pr is not None:
                    prev = prev or pr.same_stream
                    pr.same_stream = bool(on)
        return prev

    def step(self, sync=True, keep=None, outs=None):
        """keep: a list that receives clones of every gradient of the step (token gradients per pair, then the flat parameter-gradient
        buckets) -- the two-stream / one-stream comparison after the timed region.
        outs: a list that receives (name, tensor) for what the step hands its caller, per pair: the two sites' returns (outputs, router
        indices / probabilities / load-balancing losses where the variant returns them) and the two token gradients -- references, no
        copies (the parameter gradients stay readable after the step: param_grads)"""
        import torch
        c, reducer = self.c, self.reducer
        reducer.begin(sync=sync)
        for i, w in enumerate(self.work):
            xa, xv = w["f_a"].permute(0, 2, 1).unsqueeze(-1), w["f_v"].permute(0, 2, 1).unsqueeze(-1)   # the reference's (S,C,N,1) views
            for j, (a, v, pr) in enumerate(w["mods"]):
                extra = []
                idx_a = idx_v = probs_a = probs_v = lb_a = lb_v = None
                paired = self.pair_mode != "off" and pr is not None
                if paired and c["variant"] == "avs":
                    out_a, idx_a, probs_a, lb_a, out_v, idx_v, probs_v, lb_v = pr(xa, xv, is_training=True)
                    extra = [self.lbw * (lb_a + lb_v)]
                elif paired and c["variant"] == "avvp":
                    out_a, lb_a, out_v, lb_v = pr(xa, xv)
                    extra = [lb_a + lb_v]
                elif paired:
                    out_a, idx_a, out_v, idx_v = pr(xa, xv)          # net_trans_v3.py:695-698 as one autograd node (AdapterPair)
                elif c["variant"] == "avs":
                    out_a, idx_a, probs_a, lb_a = a(xa, xv, is_training=True)
                    out_v, idx_v, probs_v, lb_v = v(xv, xa, is_training=True)
                    extra = [self.lbw * (lb_a + lb_v)]
                elif c["variant"] == "avvp":
                    out_a, lb_a = a(xa, xv)
                    out_v, lb_v = v(xv, xa)
                    extra = [lb_a + lb_v]
                else:
                    out_a, idx_a = a(xa, xv)                   # net_trans_v3.py:695
                    out_v, idx_v = v(xv, xa)                   # net_trans_v3.py:697
                torch.autograd.backward([out_a, out_v] + extra, [w["ga4"], w["gv4"]] + [None] * len(extra))
                if outs is not None:
                    got = dict(out_a=out_a, idx_a=idx_a, probs_a=probs_a, lb_a=lb_a, out_v=out_v, idx_v=idx_v, probs_v=probs_v, lb_v=lb_v,
                               grad_f_a=w["f_a"].grad, grad_f_v=w["f_v"].grad)
                    outs += [(f"pair{i}_{j}_{k}", t.detach()) for k, t in got.items() if torch.is_tensor(t)]
                # the pairs of a shape share the synthetic inputs, not the modules: every pair's input gradients are its own (in the
                # model they flow into different layers), so they are dropped here instead of being summed over the pairs
                if keep is not None:
                    keep += [w["f_a"].grad.detach().clone(), w["f_v"].grad.detach().clone()]
                w["f_a"].grad = None
                w["f_v"].grad = None
        reducer.finish()
        if keep is not None:
            torch.cuda.synchronize()
            keep += [b.flat.detach().clone() for b in reducer.buckets if b.flat is not None]
        reducer.zero_grad(lazy=True)           # site slices are overwritten by the next backward: no fill launch (dp.py)

    def two_stream_bit_equal(self):
        """One step in the mode of the timed region (two streams per pair) and one with the same schedule issued on ONE stream, on the
        same inputs and parameters: every gradient equal bit for bit?  (The kernels, their launch shapes and summation orders are the
        same; what differs is that another stream's kernels share the GPU -- DESIGN section 5, the compute-unit co-residency effect.)"""
        import torch
        a, b = [], []
        self.step(sync=False, keep=a)
        prev = self.set_same_stream(True)
        self.step(sync=False, keep=b)
        self.set_same_stream(prev)
        torch.cuda.synchronize()
        return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))

    def param_grads(self):
        """(name, tensor) per site: the gradients of all its parameters (what the last step left in `.grad`), flattened and concatenated
        in parameters() order"""
        import torch
        res = []
        for i, w in enumerate(self.work):
            for j, (a, v, _pr) in enumerate(w["mods"]):
                for tag, m in (("a", a), ("v", v)):
                    gs = [(p.grad if p.grad is not None else torch.zeros_like(p)).detach().reshape(-1) for p in m.parameters()]
                    res.append((f"pair{i}_{j}_param_grads_{tag}", torch.cat(gs)))
        return res

    def timed(self, steps, warmup, outs=None):
        """W untimed warm-up steps, then exactly K steps bracketed by barrier + synchronize; MAX over the ranks.  outs: receives what
        the LAST timed step hands its caller (step)."""
        import torch
        import torch.distributed as dist

        def barrier():
            if self.world > 1:
                dist.barrier()
            torch.cuda.synchronize()
        for _ in range(warmup):
            self.step()
        barrier()
        t0 = time.perf_counter()
        for k in range(steps):
            self.step(outs=outs if k == steps - 1 else None)
        barrier()
        dt = time.perf_counter() - t0
        if self.world > 1:
            tt = torch.tensor([dt], device=self.device, dtype=torch.float64)
            dist.all_reduce(tt, op=dist.ReduceOp.MAX)
            dt = float(tt.item())
        return dt

    def release(self):
        import torch
        from avmoe_amd.adapters import release_workspaces
        self.work, self.reducer = None, None
        gc.collect()
        release_workspaces()
        torch.cuda.empty_cache()


def path_roofline(c, esz, dtype, value, world):
    abytes, rflops = algorithmic_bytes_per_clip_pair(c, esz), reference_flops_per_clip_pair(c)
    path_gbs = abytes * value / world / 1e9
    path_tfs = rflops * value / world / 1e12
    return dict(bound="hbm", achieved=round(path_gbs, 1), peak=HBM_PEAK_GBS, unit="GB/s", frac=round(path_gbs / HBM_PEAK_GBS, 4), traffic=None,
                level="path (SURVEY 8d): algorithmic bytes per clip-pair x clip-pairs/s per GPU",
                algorithmic_bytes_per_clip_pair=round(abytes), algorithmic_bytes_per_step=round(abytes * c["B"]),
                mfma_frac=round(path_tfs / MFMA_PEAK_TF[dtype], 4), mfma_tflops=round(path_tfs, 1),
                mfma_detail=dict(achieved=round(path_tfs, 1), peak=MFMA_PEAK_TF[dtype], unit="TFLOP/s", frac=round(path_tfs / MFMA_PEAK_TF[dtype], 4),
                          reference_flops_per_clip_pair=round(rflops),
                          note="FLOPs of the reference's formulation (SURVEY 8d); the factorised path executes fewer"))


def other_config_line(name, device, pair_mode, steps=3, warmup=2):
    """One of the multi-site configurations on the driver's line: `steps` timed steps (bf16, the configuration's own batch), the
    path-level roofline fraction, and the kink-aware parity of its site shapes against the oracle at B = 2."""
    import torch
    c = dict(CONFIGS[name], name=name)
    wl = Workload(c, torch.bfloat16 if c["dtype"] == "bf16" else torch.float32, device, 0, 1, pair_mode)
    dt = wl.timed(steps, warmup)
    wl.release()
    value = c["B"] / (dt / steps)
    esz = 2 if c["dtype"] == "bf16" else 4
    rl = path_roofline(c, esz, c["dtype"], value, 1)
    cpu, material = cpu_baseline(c, budget_s=0.0, min_timed=1)
    parity = {k: v for k, v in parity_check(c, material, device, pair_mode).items() if k not in PARITY_CONSTANT_KEYS}
    # the descriptive strings (roofline level, CPU sample, the parity constants) are the headline's: the line stays short enough to be read whole
    return dict(workload=f"{name}: {c['what']}", value=round(value, 2), unit="clip-pairs/s", ms_per_step=round(1e3 * dt / steps, 3), steps=steps,
                warmup=warmup, dtype=c["dtype"], clips_per_gpu=c["B"], site_pairs=sum(p[4] for p in c["pairs"]),
                roofline=dict(bound="hbm", frac=rl["frac"], achieved=rl["achieved"], peak=rl["peak"], unit="GB/s",
                              algorithmic_bytes_per_step=rl["algorithmic_bytes_per_step"]),
                parity=parity, cpu_baseline=dict(value=cpu["value"], unit=cpu["unit"], cores=cpu["cores"], kind=cpu["kind"]))


DUMP_BYTES = 60_000_000          # --dump-outputs: the .npy files together stay below this (the documented limit is 64 MB)


def dump_outputs(out_dir, arrays, budget=DUMP_BYTES):
    """--dump-outputs: every (name, tensor) as out_dir/<name>.npy in float32.  Water-filling over the budget: the smallest arrays whole
    (in their own shape), the larger ones an equal number of elements each, flat in the tensor's logical order, at sorted positions drawn
    from a generator seeded with the array's name -- the same positions in every run and every build.  Returns (files, bytes)."""
    import zlib
    import numpy as np
    import torch
    os.makedirs(out_dir, exist_ok=True)
    room = (budget - 128 * len(arrays)) // 4           # float32 elements after the .npy headers (128 bytes each)
    sizes = sorted(t.numel() for _n, t in arrays)
    cap = None
    for i, n in enumerate(sizes):
        share = room // (len(sizes) - i)
        if n > share:
            cap = share
            break
        room -= n
    nbytes = 0
    for name, t in arrays:
        if cap is not None and t.numel() > cap:
            g = torch.Generator().manual_seed(zlib.crc32(name.encode()))
            pos = torch.randint(t.numel(), (cap,), generator=g).sort().values.to(t.device)
            t = t[torch.unravel_index(pos, t.shape)]
        path = os.path.join(out_dir, f"{name}.npy")
        np.save(path, t.float().cpu().numpy())
        nbytes += os.path.getsize(path)
    return len(arrays), nbytes


def lib_stamp():
    """digest of the sources the loaded library was built from (avmoe_amd/build.py)"""
    try:
        with open(os.path.join(ROOT, "avmoe_amd", "lib", "libavmoe_hip.stamp")) as fh:
            return fh.read().strip()
    except OSError:
        return None


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--config", default="cfg2", choices=sorted(CONFIGS))
    ap.add_argument("--dtype", default=None, choices=["bf16", "f32"], help="default: the configuration's own (cfg1: f32, else bf16)")
    ap.add_argument("--batch", type=int, default=None, help="clips per GPU (default: the configuration's)")
    ap.add_argument("--full", action="store_true",
                    help="after the headline, every other leg of the line: repetitions, profiling pass, fp32 re-run, B = 2 leg, CPU baseline, "
                         "parity, the other configurations, the exposed all-reduce time (default: the headline alone)")
    ap.add_argument("--reps", type=int, default=None, help="timed repetitions of the K steps (value = the first; the others give the spread); "
                                                           "default 3 with --full, else 1")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full: skips the CPU legs (cpu_baseline, parity, other configurations)")
    ap.add_argument("--no-roofline", action="store_true", help="no roofline object; --full: also skips the profiling pass and the B = 2 leg")
    ap.add_argument("--no-f32", action="store_true", help="--full: skips the fp32 re-run (value_f32)")
    ap.add_argument("--no-other-configs", action="store_true", help="--full: skips the cfg-1 / cfg-3 / cfg-4 / cfg-5 legs of the default (cfg-2, N = 1) run")
    ap.add_argument("--pair", default="concurrent", choices=["concurrent", "same", "serial", "off"],
                    help="how the two sites of a layer are run: AdapterPair on two streams / the two-stream schedule and kernel variants issued on "
                         "ONE stream (profiling: every launch alone on the GPU) / back to back on one stream / two separate calls")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last of them computed (per site pair: outputs, router indices / probabilities / "
                         "losses, token gradients, parameter gradients) as DIR/<name>.npy in float32, under 64 MB in all (a seeded sample of "
                         "the large arrays); rank 0")
    args = ap.parse_args(argv)
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if args.reps is None:
        args.reps = 3 if args.full else 1
    return args


def main():
    args = parse_args()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        self_launch(args, sys.argv[1:])

    import torch
    import torch.distributed as dist
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: the adapter path has no CPU fallback")
    if os.environ.get("AVMOE_BENCH_BACKEND", "nccl") != "nccl":      # development: several ranks share the GPUs that exist
        local_rank %= torch.cuda.device_count()
    torch.cuda.set_device(local_rank)
    device = torch.device("cuda", local_rank)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        backend = os.environ.get("AVMOE_BENCH_BACKEND", "nccl")      # "gloo": development only (several ranks on one GPU)
        if backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=device)
        else:
            dist.init_process_group(backend, rank=rank, world_size=world)
    if args.gpus != world:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")

    from avmoe_amd import _capi as capi
    os.environ.setdefault("AVMOE_PROF_SHAPES", "1")     # profiler families per kernel and launch shape (read at first launch)
    capi.lib()
    c = dict(CONFIGS[args.config], name=args.config)
    if args.batch:
        c["B"] = args.batch
    dtype = args.dtype or c["dtype"]
    c["dtype"] = dtype
    tdt = torch.bfloat16 if dtype == "bf16" else torch.float32
    esz = 2 if dtype == "bf16" else 4

    wl = Workload(c, tdt, device, rank, world, args.pair)
    pair_mode = wl.pair_mode
    msg_bytes = wl.reducer.message_bytes()
    last = [] if args.dump_outputs and rank == 0 else None
    dt = wl.timed(args.steps, args.warmup, outs=last)          # THE timed region: W warm-up steps, then exactly K steps
    if last is not None:                                       # what the last of the K steps computed (before the repetitions below)
        n, nbytes = dump_outputs(args.dump_outputs, last + wl.param_grads())
        last = None
        print(f"bench.py: --dump-outputs: {n} arrays, {nbytes} bytes in {args.dump_outputs}", file=sys.stderr, flush=True)
    ms_per_step = 1e3 * dt / args.steps
    value = c["B"] * world / (dt / args.steps)
    rep_ms = [ms_per_step] + [1e3 * wl.timed(args.steps, 0) / args.steps for _ in range(max(0, args.reps - 1))]
    rccl = None
    if world > 1 and args.full:       # the exchange, outside the timed region: bytes / messages per step and what the backward does not hide of it
        wl.reducer.time_exposed = True
        for _ in range(5):
            wl.step()
        ex = wl.reducer.exposed_ms()
        wl.reducer.time_exposed = False
        rccl = dict(rccl_ranks=world, backend=dist.get_backend(), grad_allreduce_bytes=msg_bytes, buckets=len(wl.reducer.messages()),
                    bucket_bytes=wl.reducer.messages(), reduce_op="avg (ncclAvg)" if wl.reducer._avg_op else "sum",
                    exposed_allreduce_ms=round(statistics.median(ex), 4) if ex else None,
                    exposed_note="median over 5 extra steps of the HIP-event time between the end of the enqueued backward and the last "
                                 "bucket's all-reduce on the compute stream (AdapterGradReducer.exposed_ms)")

    roofline = None
    if not args.no_roofline:
        roofline = path_roofline(c, esz, dtype, value, world)
        if rank == 0 and args.full:
            # Profiling pass: HIP events around every launch (one family per kernel AND launch shape).  The pair keeps the SCHEDULE of
            # the timed region -- in two-stream mode every kernel in the variant that mode launches: dX overwrites, dY adds behind
            # the other site's dX -- but issues it on ONE stream (AdapterPair.same_stream; the helper streams INSIDE a site are off
            # while the profiler is on: side.cpp): an event bracket on a stream that shares the GPU with another stream also measures
            # the time a launch WAITS for compute units behind the other stream's kernels (a 10 us split-K reduction reads 100 us),
            # which is neither the kernel's duration nor what rocprofv3 reports for it.  Rank 0 only: its steps must not enter a
            # collective (sync=False = an accumulation micro-step).
            L = capi.lib()
            flipped = wl.set_same_stream(True)
            for _ in range(2):
                wl.step(sync=False)
            torch.cuda.synchronize()
            L.avmoe_prof_reset()
            L.avmoe_prof_enable(1)
            nprof = 3
            for _ in range(nprof):
                wl.step(sync=False)
            torch.cuda.synchronize()
            L.avmoe_prof_enable(0)
            wl.set_same_stream(flipped)
            rep = capi.prof_report()
            L.avmoe_prof_reset()
            if os.environ.get("AVMOE_FAMILIES_OUT"):      # dev: every family of the profiling pass
                with open(os.environ["AVMOE_FAMILIES_OUT"], "w") as fh:
                    json.dump(sorted(rep, key=lambda r: -r["total_ms"]), fh, indent=0)
            tot_ms = sum(r["total_ms"] for r in rep)
            dom = max(rep, key=lambda r: r["total_ms"])
            avg_ms = dom["total_ms"] / dom["calls"]
            gbs = dom["alg_bytes"] / dom["calls"] / (avg_ms * 1e-3) / 1e9
            tfs = dom["flops"] / dom["calls"] / (avg_ms * 1e-3) / 1e12
            dk = dict(kernel=dom["name"], bound="hbm", achieved=round(gbs, 1), peak=HBM_PEAK_GBS, unit="GB/s", frac=round(gbs / HBM_PEAK_GBS, 4),
                      traffic=None, launches_per_step=dom["calls"] // nprof, avg_launch_us=round(avg_ms * 1e3, 2),
                      share_of_gpu_time=round(dom["total_ms"] / tot_ms, 3), kernel_tflops=round(tfs, 1),
                      measured="HIP events on the launch stream, every launch alone on the GPU (profiling pass of 3 steps after the timed "
                               f"region: the schedule and kernel variants of --pair {pair_mode}"
                               + (" -- dX overwrites (non-accumulating), dY accumulates --" if pair_mode == "concurrent" else "") +
                               " issued on one stream, helper streams off); the largest (kernel, launch shape) family by time per step")
            tj = os.path.join(ROOT, "profiles", f"{ROUND}_pmc_traffic.json")
            if os.path.isfile(tj) and args.config == "cfg2" and not args.batch and dtype == "bf16":
                with open(tj) as fh:       # HBM bytes from THIS round's rocprofv3 --pmc passes (scripts/make_profiles.sh)
                    tjd = json.load(fh)
                if tjd.get("__lib_stamp__") and tjd["__lib_stamp__"] == lib_stamp():
                    t = tjd.get(dom["name"].split(" NT")[0].split(" M")[0])
                    if t:      # the dominant launch is the largest one of its family
                        dk["traffic"] = t["read_bytes_largest_launch"] + t["write_bytes_largest_launch"]
                        dk["traffic_source"] = f"profiles/{ROUND}_pmc_traffic.json"
                    if tjd.get("__total_bytes_per_step__"):
                        roofline["traffic"] = tjd["__total_bytes_per_step__"]
                        roofline["traffic_source"] = f"profiles/{ROUND}_pmc_traffic.json: FETCH_SIZE + WRITE_SIZE over every kernel of one step (PMC pass of this very build: library stamps equal)"
                else:
                    roofline["traffic_note"] = (f"profiles/{ROUND}_pmc_traffic.json was collected on a different build of the library "
                                                "(stamp mismatch): not reported")
            # scalars first (the driver's record keeps the scalar members of `roofline`), the full objects beside them
            roofline["dominant_kernel"] = dk["kernel"]
            roofline["dominant_frac"] = dk["frac"]
            roofline["dominant_us"] = dk["avg_launch_us"]
            roofline["dominant_gbs"] = dk["achieved"]
            roofline["dominant_traffic"] = dk["traffic"]
            roofline["dominant_variant"] = f"as launched by --pair {pair_mode}" + (": dX non-accumulating" if pair_mode == "concurrent" else "")
            roofline["dominant_detail"] = dk
            roofline["gpu_time_ms_per_step"] = round(tot_ms / nprof, 3)
            roofline["launches_per_step"] = sum(r["calls"] for r in rep) // nprof
            roofline["kernel_families"] = len(rep)
            roofline["families"] = sorted([dict(name=r["name"], calls=r["calls"] // nprof, ms_per_step=round(r["total_ms"] / nprof, 4),
                                                gbs=round(r["alg_bytes"] / max(r["total_ms"], 1e-9) / 1e6, 1))
                                           for r in rep], key=lambda r: -r["ms_per_step"])[:12]

    if isinstance(roofline, dict) and rank == 0 and pair_mode == "concurrent" and args.full:
        reps = [wl.two_stream_bit_equal() for _ in range(3)]
        roofline["two_stream_bit_equal"] = all(reps)
        roofline["two_stream_note"] = ("3 x (one step on two streams, one with the same schedule on one stream; same inputs): every token and parameter "
                                       "gradient bit-identical -- the co-residency guard of include/avmoe.h (shared_gpu) on the timed configuration")
    wl.release()
    value_f32 = None
    if args.full and dtype == "bf16" and not args.no_f32 and world == 1:
        wl = Workload(c, torch.float32, device, rank, world, args.pair)
        k32 = max(3, args.steps // 2)
        dt32 = wl.timed(k32, 2)
        value_f32 = dict(value=round(c["B"] * world / (dt32 / k32), 2), unit="clip-pairs/s", ms_per_step=round(1e3 * dt32 / k32, 4), steps=k32,
                         dtype="f32", note="fp32 activations on the bf16 matrix pipe: three bf16 planes per value (six plane products of order <= 2, 5.8e-9 relative per product, fp32 accumulation; csrc/moe_run.h: AVMOE_FWD_SPLIT3) for the forward and every product of the backward a cancelling sum is formed from, two planes (three products, 1.5e-5 per product) for its leaf gradients dWt / dWf / dWcK / dX / dY (AVMOE_LEAF2): the configuration held to the 1e-3 parity bar")
        wl.release()

    # the reference's own batch (AVE/train.sh:33: 2 clips): the same step at B = 2, where the launch rate binds -- step time and launches per step
    b2 = None
    if args.full and args.config == "cfg2" and not args.batch and not args.dtype and world == 1 and not args.no_roofline:
        wl = Workload(dict(c, B=2), tdt, device, rank, world, args.pair)
        k2 = max(20, args.steps)
        t2 = [1e3 * wl.timed(k2, 5 if i == 0 else 0) / k2 for i in range(3)]
        L = capi.lib()
        flipped = wl.set_same_stream(True)
        wl.step(sync=False)
        torch.cuda.synchronize()
        L.avmoe_prof_reset(); L.avmoe_prof_enable(1)
        wl.step(sync=False)
        torch.cuda.synchronize()
        L.avmoe_prof_enable(0)
        wl.set_same_stream(flipped)
        rep2 = capi.prof_report()
        L.avmoe_prof_reset()
        b2 = dict(ms_per_step=round(min(t2), 4), repeat_ms_per_step=[round(x, 4) for x in t2], launches_per_step=sum(r["calls"] for r in rep2),
                  gpu_time_ms_per_step=round(sum(r["total_ms"] for r in rep2), 4), clips=2, steps=k2,
                  note="cfg-2 shapes at B = 2 clips (the reference's batch): best of 3 repetitions of the timed steps; launches = timed scopes of the library in one step")
        wl.release()

    cpu = parity = others = None
    exit_code = 0
    if args.full and not args.no_cpu_baseline and rank == 0 and world == 1:
        cpu, material = cpu_baseline(c)
        try:
            parity = parity_check(c, material, device, pair_mode)
        except Exception as e:      # the line must not be lost to its checker leg: it then says so (and the run exits non-zero after printing it)
            parity = dict(ok=False, error=f"{type(e).__name__}: {e}", failed=["parity leg raised"])
        del material
        if args.config == "cfg2" and not args.batch and not args.dtype and not args.no_other_configs:
            others = {}
            for name in ("cfg1", "cfg4", "cfg5", "cfg3"):
                try:       # (cfg-3: 0.7 s per step -- two timed steps)
                    others[name] = other_config_line(name, device, args.pair, **(dict(steps=2, warmup=1) if name == "cfg3" else {}))
                except Exception as e:      # the headline line must not be lost to a side leg
                    others[name] = dict(error=f"{type(e).__name__}: {e}")
                gc.collect()
                torch.cuda.empty_cache()

    if rank == 0:
        shapes = [dict(C_a=Ca, N_a=Na, C_v=Cv, N_v=Nv, site_pairs=cnt, bottleneck_a=Ca // c["reduction"], bottleneck_v=Cv // c["reduction"])
                  for Ca, Na, Cv, Nv, cnt in c["pairs"]]
        line = {
            "metric": "clip-pairs/sec (adapter fwd+bwd, AVE-shape synthetic)", "value": round(value, 2),
            "unit": "clip-pairs/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(ms_per_step, 4), "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": dtype, "data": "synthetic",
            "config": {"workload": f"{args.config}: {c['what']}, fwd+bwd incl. input and parameter grads", "variant": c["variant"],
                       "clips_per_gpu": c["B"], "frames_per_clip": c["T"], "site_pairs": sum(p[4] for p in c["pairs"]), "shapes": shapes,
                       "experts": f"{c['E_m']} cross-modal + {c['E_s']} unimodal", "reduction": c["reduction"], "latent_tokens": c["K"],
                       "groups": c["groups"], "pair_mode": pair_mode, "parallelism": f"dp{world}",
                       "grad_allreduce_bytes": msg_bytes if world > 1 else 0},
            "repeat_ms_per_step": [round(x, 4) for x in rep_ms],
            "spread_rel": round((max(rep_ms) - min(rep_ms)) / statistics.median(rep_ms), 4),
            "roofline": roofline, "parity": parity,
            # top-level scalars (the driver's record keeps scalars): the fp32 configuration and the other configurations' steps
            "value_f32": value_f32["value"] if value_f32 else None, "ms_per_step_f32": value_f32["ms_per_step"] if value_f32 else None,
            "f32_detail": value_f32, "cpu_baseline": cpu, "other_configs": others,
        }
        if others:
            for name, o in others.items():
                line[f"{name}_ms_per_step"] = o.get("ms_per_step")
                line[f"{name}_parity_ok"] = (o.get("parity") or {}).get("ok")
        if parity is not None:
            line["parity_ok"] = parity["ok"]
        if b2:
            line["b2"] = b2
            line["b2_ms_per_step"] = b2["ms_per_step"]
        if isinstance(roofline, dict) and args.full:
            # scalar copies INSIDE `roofline` (the driver's record keeps the scalar members of roofline / config / cpu_baseline only)
            roofline["f32_value"] = value_f32["value"] if value_f32 else None
            roofline["f32_ms_per_step"] = value_f32["ms_per_step"] if value_f32 else None
            for name in ("cfg1", "cfg3", "cfg4", "cfg5"):
                o = (others or {}).get(name) or {}
                roofline[f"{name}_ms_per_step"] = o.get("ms_per_step")
                roofline[f"{name}_parity_ok"] = (o.get("parity") or {}).get("ok")
            for k in ("out_rel_f32", "grad_rel_f32", "out_rel_bf16", "grad_relnorm_bf16_major", "grad_relnorm_bf16_rest", "grad_relnorm_bf16_tiny_joint",
                      "grad_abs_bf16_structural_zero"):
                roofline[k] = (parity or {}).get(k)
            roofline["parity_ok"] = parity["ok"] if parity else None
            roofline["ok_bf16_grads"] = (parity or {}).get("ok_bf16_grads")
            roofline["b2_ms_per_step"] = b2["ms_per_step"] if b2 else None
            roofline["launches_per_step_b2"] = b2["launches_per_step"] if b2 else None
            # the scalars a reader wants first come first (a record that keeps only the leading scalar members keeps these); long strings,
            # per-config parity flags and the list-valued members go last
            lead = ("bound", "achieved", "peak", "unit", "frac", "traffic", "f32_value", "f32_ms_per_step", "parity_ok", "ok_bf16_grads",
                    "cfg1_ms_per_step", "cfg3_ms_per_step", "cfg4_ms_per_step", "cfg5_ms_per_step", "b2_ms_per_step", "launches_per_step",
                    "dominant_kernel", "dominant_frac", "dominant_us", "dominant_traffic", "two_stream_bit_equal", "gpu_time_ms_per_step",
                    "launches_per_step_b2", "dominant_gbs", "mfma_frac", "mfma_tflops")
            tail = ("level", "traffic_source", "traffic_note", "dominant_variant", "dominant_detail", "families")
            ordered = {k: roofline[k] for k in lead if k in roofline}
            ordered.update({k: v for k, v in roofline.items() if k not in lead and k not in tail})
            ordered.update({k: roofline[k] for k in tail if k in roofline})
            roofline = line["roofline"] = ordered
        if rccl:
            line.update(rccl_ranks=rccl["rccl_ranks"], grad_allreduce_bytes=rccl["grad_allreduce_bytes"], allreduce_buckets=rccl["buckets"],
                        exposed_allreduce_ms=rccl["exposed_allreduce_ms"], rccl=rccl)
        print(json.dumps(line), flush=True)
        bad = [("cfg2" if args.config == "cfg2" else args.config, parity["failed"])] if (parity and not parity["ok"]) else []
        bad += [(n, o["parity"]["failed"]) for n, o in (others or {}).items() if o.get("parity") and not o["parity"]["ok"]]
        if bad:
            print(f"bench.py: PARITY FAILED (bars {PARITY_BARS}): {bad}", file=sys.stderr, flush=True)
            exit_code = 1
    if world > 1:
        dist.barrier()                       # the other ranks wait for rank 0's extra passes: clean teardown of the communicator
        dist.destroy_process_group()
    if exit_code:
        raise SystemExit(exit_code)


if __name__ == "__main__":
    main()
