"""Driver for a kernel trace of the optimizer step (DESIGN_CURRENT.md section 4b):

    rocprofv3 --kernel-trace --stats -d OUT -o NAME -- python scripts/flat_adam_step_profile.py --model eight_site --mode device

--mode device      FlatAdam(max_grad_norm=..., skip_nonfinite=True).step(): three launches whatever the model
--mode clip_plain  torch.nn.utils.clip_grad_norm_ over the bucket views + the plain FlatAdam.step() (one avmoe_adam_step per merged range)
--schedule         (device mode) a per-step LRSchedule -- warm-up + cosine across the measured steps -- evaluated on the device: still three launches
--schedule-upload  (device mode) the same schedule WITHOUT the device-side factor: the rates are rewritten into the range table and the
                   table is re-sent before every step (FlatAdam._upload_table()), the only way to a per-step schedule before --schedule
--ema              (device mode) FlatAdam(ema_decay=0.999): the update launch also advances the weight average -- still three launches
--ema-foreach      (device mode) the same average kept OUTSIDE the optimizer: the step without it, then torch._foreach_lerp_ over the
                   parameter views with the decay computed on the host (FlatAdam.ema_decay_at), what a user had to write before --ema
--ema-buffers      (with --ema) FlatAdam(ema_buffers=model): the model's BatchNorm running statistics are averaged too -- one launch more
                   (`kk_opt_ema_buffers`), whatever the number of buffers
--ema-buffers-foreach  (with --ema) the same buffer average kept OUTSIDE the optimizer: the --ema step, then torch._foreach_lerp_ over the
                   model's fp32 buffers with the decay computed on the host, what a user had to write before --ema-buffers
--swa              (device mode, in place of --ema) FlatAdam(swa_start=total // 4, swa_freq=5): the uniform average of stochastic weight
                   averaging -- the launches of --ema, the decay by another rule in the finalize launch; with --schedule the schedule
                   also anneals to a constant SWA rate from step total // 2 on (LRSchedule(swa_start=...)); goes with --ema-buffers too
--sam              (device mode) FlatAdam(sam_rho=0.05): every iteration is sam_perturb() -- three launches: the norm pass of the first
                   gradient, a one-block finalize, hold = w ; w += e -- and then step(), whose update launch reads the weights from the
                   hold buffers; --adaptive with it: the ASAM perturbation.  Combines with --ema, --swa, --schedule, --report
--sam-foreach      (device mode) the same perturbation done OUTSIDE the optimizer with torch._foreach_* ops over the parameter views
                   (norm, scale, clone, add), then the weights copied back and the step without SAM: what a user had to write before --sam
--per-step-events  an event pair around every step() (and, with --sam / --sam-foreach, around every perturbation): `step_seg_us` and
                   `perturb_us` are the means of those segments -- the way to time the step of a --sam iteration alone, and the
                   counterpart without --sam measured the same way
--report           (device mode) FlatAdam(report_grad_norms=True): one more launch behind finalize writes every parameter's gradient norm
--lamb             (device mode) FlatAdam(trust_ratio=True, trust_clip=10.0): layer-wise trust ratios -- three launches (moments and block
                   sums, a wave per parameter for norms and ratio, the update) in place of the one update launch: 5 per step.
                   Combines with --schedule, --ema, --swa, --report, --sam
--prodigy          (device mode) FlatAdam(lr=1.0, prodigy=True): Prodigy learning-rate estimation -- two launches (the update with both block
                   sums, a one-block finalize that writes d) in place of the one update launch: 4 per step.  The alternative to --lamb;
                   combines with --schedule, --ema, --swa, --report, --sam
--adamw            (device mode) decoupled weight decay (torch.optim.AdamW's rule): the baseline of --muon
--muon             (device mode) FlatAdam(muon=True, decoupled_weight_decay=True): orthogonalised momentum for the hidden matrices -- two
                   launches (the table walk with m, u and block sums; a workgroup per matrix for the Newton-Schulz iteration and the
                   update) in place of the one update launch: 4 per step.  The alternative to --lamb / --prodigy; combines with
                   --schedule, --ema, --swa, --report, --sam.  Time it with --per-step-events: `step_seg_median_us` is the median of the
                   event pairs around every step()
--muon-large       (with --muon) FlatAdam(muon=True, muon_large=True): the matrices the small rule declines go through the tiled engine --
                   2 + 1 + 3 * ns_steps * classes (+ split-K reduces) + 1 launches in place of the one update launch
--sched-free       (device mode) FlatAdam(schedule_free=True, decoupled_weight_decay=True): schedule-free AdamW -- two launches (one thread
                   for the averaging weight, the table walk over y, the gradient, z, v and x) in place of the one update launch: the norm
                   call's + 2 per step.  The alternative to --ema / --swa / --lamb / --prodigy / --muon; combines with --schedule (a
                   warm-up without a decay there), --ema-buffers, --report, --sam
--model two_bucket the model of tests/test_flat_adam_device_gpu.py ; eight_site the model of tests/test_training_loop_gpu.py ;
        wide_site  one AVE MoEAdapter at Swin-L / HTS-AT widths (C = 768, 196 x 1024 tokens, a 768-wide other modality), parameters as
                   plain ranges: conv_adapter is 196 x 1024 and fc 768 x 768, the matrices only --muon-large orthogonalises

The gradients are random values written into the buckets once (no backward: the trace holds the optimizer's launches only).  Prints one
JSON line: launches per step are the trace's calls / steps; `step_us` is the event-timed mean of --steps steps enqueued back to back,
`step_wall_us` the host time to enqueue one step (the launch-bound side).  With --sam / --sam-foreach a "step" of both is a whole
iteration, perturbation included; `perturb_us` and `step_seg_us` are its two parts."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def build(model_name, dev):
    from avmoe_amd.adapters import MoEAdapter
    if model_name == "wide_site":
        from tests.golden_util import load_golden
        from tests.test_adapters_api import _opt
        _, cfg, _ = load_golden("ave_train")
        torch.manual_seed(11)
        m = MoEAdapter(input_dim=768, output_dim=768, adapter_kind="bottleneck", dim_list=None, layer_idx=0, opt=_opt(cfg), conv_dim_in=1024,
                       conv_dim_out=196, linear_in=768, linear_out=768, reduction_factor=8, use_bn=True, use_gate=True, num_tk=87).to(dev)
        return [p for p in m.parameters() if p.requires_grad], None, m
    if model_name == "two_bucket":
        from tests.test_flat_adam_device_gpu import make_model
        m = make_model(dev)
        return m.all_params(), [m.site], m
    from tests.test_training_loop_gpu import TinyModel
    from avmoe_amd.train import select_trainable
    torch.manual_seed(11)
    m = TinyModel(64, 100, 48, 160).to(dev)
    groups = select_trainable(m, lr=5e-3, lr_mlp=5e-3)
    return [g["params"] for g in groups if g["params"].requires_grad], [s for s in m.modules() if isinstance(s, MoEAdapter)], m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", choices=["two_bucket", "eight_site", "wide_site"], default="eight_site")
    ap.add_argument("--mode", choices=["device", "clip_plain"], default="device")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--schedule", action="store_true")
    ap.add_argument("--schedule-upload", action="store_true")
    ap.add_argument("--ema", action="store_true")
    ap.add_argument("--ema-foreach", action="store_true")
    ap.add_argument("--ema-buffers", action="store_true")
    ap.add_argument("--ema-buffers-foreach", action="store_true")
    ap.add_argument("--report", action="store_true")
    ap.add_argument("--swa", action="store_true")
    ap.add_argument("--sam", action="store_true")
    ap.add_argument("--adaptive", action="store_true")
    ap.add_argument("--sam-foreach", action="store_true")
    ap.add_argument("--per-step-events", action="store_true")
    ap.add_argument("--lamb", action="store_true")
    ap.add_argument("--prodigy", action="store_true")
    ap.add_argument("--adamw", action="store_true")
    ap.add_argument("--muon", action="store_true")
    ap.add_argument("--muon-large", action="store_true")
    ap.add_argument("--sched-free", action="store_true")
    a = ap.parse_args()
    if (a.schedule or a.schedule_upload) and a.mode != "device":
        ap.error("--schedule / --schedule-upload go with --mode device")
    if a.schedule and a.schedule_upload:
        ap.error("--schedule and --schedule-upload are the two sides of one comparison")
    if (a.ema or a.ema_foreach) and a.mode != "device":
        ap.error("--ema / --ema-foreach go with --mode device")
    if a.report and a.mode != "device":
        ap.error("--report goes with --mode device")
    if a.ema and a.ema_foreach:
        ap.error("--ema and --ema-foreach are the two sides of one comparison")
    if a.swa and (a.mode != "device" or a.ema or a.ema_foreach or a.schedule_upload or a.ema_buffers_foreach):
        ap.error("--swa goes with --mode device and is the alternative to --ema; it combines with --schedule, --ema-buffers and --report")
    if a.sched_free and (a.mode != "device" or a.ema or a.ema_foreach or a.swa or a.lamb or a.prodigy or a.muon or a.schedule_upload):
        ap.error("--sched-free goes with --mode device and is the alternative to --ema / --swa / --lamb / --prodigy / --muon")
    if a.ema_buffers and not (a.ema or a.swa or a.sched_free):
        ap.error("--ema-buffers goes with --ema, --swa or --sched-free")
    if a.ema_buffers_foreach and not a.ema:
        ap.error("--ema-buffers-foreach goes with --ema")
    if a.ema_buffers and a.ema_buffers_foreach:
        ap.error("--ema-buffers and --ema-buffers-foreach are the two sides of one comparison")
    if (a.sam or a.sam_foreach) and a.mode != "device":
        ap.error("--sam / --sam-foreach go with --mode device")
    if a.sam and a.sam_foreach:
        ap.error("--sam and --sam-foreach are the two sides of one comparison")
    if a.adaptive and not a.sam:
        ap.error("--adaptive goes with --sam")
    if a.lamb and a.mode != "device":
        ap.error("--lamb goes with --mode device")
    if a.prodigy and (a.mode != "device" or a.lamb):
        ap.error("--prodigy goes with --mode device and is the alternative to --lamb")
    if a.muon and (a.mode != "device" or a.lamb or a.prodigy):
        ap.error("--muon goes with --mode device and is the alternative to --lamb / --prodigy")
    if a.muon_large and not a.muon:
        ap.error("--muon-large goes with --muon")
    if a.adamw and a.mode != "device":
        ap.error("--adamw goes with --mode device")
    from avmoe_amd.dp import AdapterGradReducer
    from avmoe_amd.train import FlatAdam, LRSchedule
    dev = torch.device("cuda:0")
    params, sites, model = build(a.model, dev)
    red = AdapterGradReducer(params, sites=sites) if sites is not None else AdapterGradReducer(params)
    kw = dict(max_grad_norm=1.0, skip_nonfinite=True) if a.mode == "device" else {}
    total = a.warmup + a.steps
    sched = None
    if a.schedule or a.schedule_upload:
        swa_lr = dict(swa_start=total // 2, swa_factor=0.2, swa_anneal_steps=max(1, total // 8)) if a.swa else {}
        sched = LRSchedule(warmup_steps=total // 4, warmup_start=0.1, decay_kind="cosine", total_steps=max(total, total // 4 + 1), min_factor=0.05,
                           **swa_lr)
        if a.sched_free:                                 # the recipe: a warm-up and no decay
            sched = LRSchedule(warmup_steps=total // 4, warmup_start=0.1)
    if a.schedule:
        kw["lr_schedule"] = sched
    ema_decay, ema_warmup = 0.999, 10.0
    if a.ema:
        kw.update(ema_decay=ema_decay, ema_warmup=ema_warmup)
    swa_start, swa_freq = max(1, total // 4), 5
    if a.swa:
        kw.update(swa_start=swa_start, swa_freq=swa_freq)
    if a.report:
        kw["report_grad_norms"] = True
    if a.ema_buffers:
        kw["ema_buffers"] = model
    sam_rho = 0.05
    if a.sam:
        kw.update(sam_rho=sam_rho, sam_adaptive=a.adaptive)
    if a.lamb:
        kw.update(trust_ratio=True, trust_clip=10.0)
    buffers = [b for _, b in model.named_buffers() if b.dtype == torch.float32 and b.numel() > 0]
    buffer_shadows = [b.detach().clone() for b in buffers] if a.ema_buffers_foreach else None
    if a.prodigy:
        kw.update(prodigy=True)
    if a.adamw or a.muon:
        kw.update(decoupled_weight_decay=True)
    if a.muon:
        kw.update(muon=True)
    if a.muon_large:
        kw.update(muon_large=True)
    if a.sched_free:
        kw.update(schedule_free=True, decoupled_weight_decay=True)
    opt = FlatAdam(red, lr=1.0 if a.prodigy else 1e-3, weight_decay=1e-2, **kw)
    shadows = [p.detach().clone() for p in opt.params] if a.ema_foreach else None
    views = [p.data for p in opt.params]
    base_lr = [r.lr0 for r in opt._recs]
    g = torch.Generator().manual_seed(0)
    for b in red.buckets:
        b.flat.copy_(torch.randn(b.flat.numel(), generator=g))
    grads = [p for p in params]
    grads_of = [p.grad for p in opt.params]

    split = a.per_step_events or a.sam or a.sam_foreach
    marks = []                                           # four events per measured iteration: around the perturbation, around the step

    def perturb():
        if a.sam:
            opt.sam_perturb()
            return None
        # the host's way: a norm per tensor and the norm of those, the scale kept on the device (no synchronisation), a clone of every
        # parameter, e = scale * g per tensor and the sum in place
        norm = torch.linalg.vector_norm(torch.stack(torch._foreach_norm(grads_of)))
        held = [v.clone() for v in views]
        torch._foreach_add_(views, torch._foreach_mul(grads_of, sam_rho / (norm + 1e-12)))
        return held

    def iteration(measured):
        if not split:
            return step()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)] if measured else None
        if ev:
            ev[0].record()
        held = perturb() if (a.sam or a.sam_foreach) else None
        if ev:
            ev[1].record()
        if held is not None:
            torch._foreach_copy_(views, held)            # the weights back, outside both timed segments
        if ev:
            ev[2].record()
        step()
        if ev:
            ev[3].record()
            marks.append(ev)

    def step():
        if a.mode == "clip_plain":
            torch.nn.utils.clip_grad_norm_(grads, 1.0)
        if a.schedule_upload:                            # the host drives the schedule: new rates into the table, the table to the device
            f = sched.factor(opt.t)                      # opt.t == applied_steps here: the fixed finite gradients never skip a step
            for r, lr0 in zip(opt._recs, base_lr):
                r.lr0 = lr0 * f
            opt._upload_table()
        opt.step()
        if a.ema_foreach:                                # ema += (1 - d) * (p - ema), d of this step from the host's count of steps
            torch._foreach_lerp_(shadows, views, 1.0 - FlatAdam.ema_decay_at(opt.t, ema_decay, ema_warmup))
        if a.ema_buffers_foreach:
            torch._foreach_lerp_(buffer_shadows, buffers, 1.0 - FlatAdam.ema_decay_at(opt.t, ema_decay, ema_warmup))

    for _ in range(a.warmup):
        iteration(False)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    for _ in range(a.steps):
        iteration(True)
    e1.record()
    wall = time.perf_counter() - t0
    torch.cuda.synchronize()
    extra = {"schedule": "device"} if a.schedule else {"schedule": "table upload per step"} if a.schedule_upload else {}
    if a.ema or a.ema_foreach:
        extra["ema"] = "device" if a.ema else "torch._foreach_lerp_ per step"
        avg = opt.ema_params if a.ema else shadows
        extra["ema_minus_param_max"] = max(float((e - p).abs().max()) for e, p in zip(avg, views))
    if a.ema:
        extra["last_ema_decay"] = float(opt.last_ema_decay.item())
        extra["want_ema_decay"] = FlatAdam.ema_decay_at(total, ema_decay, ema_warmup)
    if a.swa:
        extra["swa"] = "device"
        extra["swa_models_averaged"] = FlatAdam.swa_n_averaged_at(total, swa_start, swa_freq)
        extra["ema_minus_param_max"] = max(float((e - p).abs().max()) for e, p in zip(opt.ema_params, views))
        extra["last_ema_decay"] = float(opt.last_ema_decay.item())
        extra["want_ema_decay"] = FlatAdam.swa_decay_at(total, swa_start, swa_freq)
    if a.ema_buffers or a.ema_buffers_foreach:
        extra["ema_buffers"] = "device" if a.ema_buffers else "torch._foreach_lerp_ per step"
        avg = opt.ema_buffers if a.ema_buffers else buffer_shadows
        extra["buffers"], extra["buffer_elements"] = len(avg), sum(b.numel() for b in avg)
        extra["buffer_blocks"] = sum((b.numel() + 1023) // 1024 for b in avg)
    if split:
        segs = sorted(e[2].elapsed_time(e[3]) for e in marks)
        extra["step_seg_us"] = round(1e3 * sum(segs) / len(segs), 2)
        extra["step_seg_median_us"] = round(1e3 * segs[len(segs) // 2], 2)
        extra["step_seg_min_us"], extra["step_seg_max_us"] = round(1e3 * segs[0], 2), round(1e3 * segs[-1], 2)
    if a.sam or a.sam_foreach:
        extra["sam"] = ("device, adaptive" if a.adaptive else "device") if a.sam else "torch._foreach_* per step"
        extra["perturb_us"] = round(1e3 * sum(e[0].elapsed_time(e[1]) for e in marks) / len(marks), 2)
    if a.sam:
        extra["last_sam_norm"], extra["last_sam_scale"] = float(opt.last_sam_norm.item()), float(opt.last_sam_scale.item())
        extra["sam_nonfinite"], extra["perturbed"] = int(opt.sam_nonfinite.item()), opt.perturbed
    if a.lamb:
        r = opt.last_trust_ratios
        extra["lamb"] = "device"
        extra["adapted"], extra["ratio_min"], extra["ratio_max"] = sum(opt.adapted), float(r.min().item()), float(r.max().item())
        extra["ratios_not_one"] = int((r != 1.0).sum().item())
    if a.prodigy:
        extra["prodigy"] = "device"
        extra["d0"], extra["d"], extra["d_hat"] = opt.prodigy_d0, float(opt.prodigy_d.item()), float(opt.prodigy_d_hat.item())
    if a.muon:
        shapes = [r.muon_shape for r in opt._recs if r.muon_shape is not None]
        extra["muon"] = "device"
        extra["matrices"], extra["matrix_elements"] = len(shapes), sum(r * c for r, c in shapes)
        extra["largest_matrix"] = list(max(shapes, key=lambda sh: sh[0] * sh[1]))
        extra["widest_short_side"] = max(min(sh) for sh in shapes)
        extra["muon_norm_min"] = float(opt.last_muon_norms[opt._muon_index].min().item())
    if a.muon_large:
        extra["large_matrices"] = [list(r.muon_shape) for r in opt._recs if r.muon_path == "large"]
        extra["large_classes"] = getattr(opt, "_muon_large_classes", 0)
    if a.sched_free:
        extra["sched_free"] = "device"
        extra["sf_c"], extra["sf_weight_sum"], extra["sf_lr_max"] = float(opt.sf_c.item()), float(opt.sf_weight_sum.item()), float(opt.sf_lr_max.item())
        extra["last_ema_decay"] = float(opt.last_ema_decay.item())
        extra["x_minus_y_max"] = max(float((e - p).abs().max()) for e, p in zip(opt.ema_params, views))
    if a.adamw or a.muon or a.sched_free:
        extra["decay"] = "decoupled"
    if a.report:
        extra["report"] = "device"
        extra["first_nonfinite_param"] = int(opt.first_nonfinite_param.item())
        extra["param_norms_vs_total"] = float(opt.last_param_grad_norms.double().pow(2).sum().sqrt().item()) / float(opt.last_grad_norm.item())
    if a.schedule:
        extra["last_lr_factor"] = float(opt.last_lr_factor.item())
        extra["want_lr_factor"] = sched.factor(total - 1)
    print(json.dumps({"model": a.model, "mode": a.mode, **extra, "steps": a.steps, "warmup": a.warmup, "buckets": len(red.buckets),
                      "parameters": len(params), "elements": sum(p.numel() for p in params),
                      "plain_launches_per_step": sum(len(s["ranges"]) for s in opt.state),
                      "step_us": round(1e3 * e0.elapsed_time(e1) / a.steps, 2), "step_wall_us": round(1e6 * wall / a.steps, 2)}))


if __name__ == "__main__":
    main()
