"""FlatAdam's per-group weight decay (both paths) and the per-parameter gradient norms of its device path (avmoe_amd.train.FlatAdam:
param_groups with "weight_decay", report_grad_norms; include/avmoe.h: avmoe_opt_grad_norm_report) on the two-bucket model of
tests/test_flat_adam_device_gpu.py, against PyTorch on the same GPU, and at the C ABI on ranges cut from one flat tensor.

Tolerances.  Adam arithmetic against torch: the bar of tests/test_flat_adam_device_gpu.py, 1e-6 * max|p| + 2e-3 * lr per parameter and step
with the parameters re-synchronised after each step.  A range's norm against the fp64 norm of its own gradient: 2^-22 relative -- the
kernel adds doubles (each block sum and their sum are exact to double rounding, far below fp32), takes a double square root and rounds
ONCE to fp32, which alone is 2^-24.  sqrt(sum norms^2) against total_norm: 2^-21 -- one fp32 rounding on either side and the fp32
roundings of the terms.  Everything that is the same kernels on the same bits is held to bit-equality."""
import copy
import ctypes as C
import io
import math

import pytest
import torch

from tests.test_flat_adam_device_gpu import (LR, LR_X, WD, assert_flats_equal, bits, fixed_grads, flats, make_model, make_opt, set_grads, tol)

pytestmark = pytest.mark.gpu

NORM_TOL, TOTAL_TOL = 2.0 ** -22, 2.0 ** -21


# ---- per-group weight decay --------------------------------------------------------------------------------------------
def decay_groups(model, wd0=0.0, wd_rest=None):
    """two decay groups crossed with make_model's two learning rates: biases and every 1-D parameter at `wd0`, the rest at `wd_rest`
    (None: no key, the constructor's decay); the plain parameters of the second bucket are all 1-D"""
    site = list(model.site.parameters())
    rest = {"params": [p for p in site if p.dim() > 1], "lr": LR}
    if wd_rest is not None:
        rest["weight_decay"] = wd_rest
    return [rest, {"params": [p for p in site if p.dim() <= 1], "lr": LR, "weight_decay": wd0},
            {"params": list(model.extra), "lr": LR_X, "weight_decay": wd0}]


def make_group_opt(model, groups, **kw):
    from avmoe_amd.dp import AdapterGradReducer
    from avmoe_amd.train import FlatAdam
    red = AdapterGradReducer(model.all_params(), sites=[model.site])
    kw.setdefault("lr", LR)
    return red, FlatAdam(red, param_groups=groups, **kw)


def rate_of(opt, i):
    return opt._recs[i].lr0 * opt.decay


@pytest.mark.parametrize("path,decoupled", [("device", False), ("device", True), ("plain", False)])
def test_per_group_decay_matches_torch(path, decoupled):
    dev = torch.device("cuda:0")
    ref = make_model(dev)
    fused = copy.deepcopy(ref)
    assert any(p.dim() <= 1 for p in ref.site.parameters()) and any(p.dim() > 1 for p in ref.site.parameters())
    grads = fixed_grads(ref, 6, dev)
    kw = dict(weight_decay=WD)
    if path == "device":
        kw.update(decoupled_weight_decay=decoupled, skip_nonfinite=True)
    _, fopt = make_group_opt(fused, decay_groups(fused), **kw)
    assert fopt._device == (path == "device")
    groups = fopt.torch_param_groups()
    assert sorted((g["lr"], g["weight_decay"]) for g in groups) == sorted([(LR, WD), (LR, 0.0), (LR_X, 0.0)])
    ref_of = {id(q): p for p, q in zip(ref.all_params(), fused.all_params())}
    topt = (torch.optim.AdamW if decoupled else torch.optim.Adam)(
        [{"params": [ref_of[id(q)] for q in g["params"]], "lr": g["lr"], "weight_decay": g["weight_decay"]} for g in groups], lr=LR)
    order = [ref_of[id(q)] for q in fopt.params]
    for k in range(6):
        for p, gr in zip(ref.all_params(), grads[k]):
            p.grad = gr.clone()
        set_grads(fused, grads[k])
        topt.step(); fopt.step()
        worst = 0.0
        with torch.no_grad():
            for i, (p, q) in enumerate(zip(order, fopt.params)):
                err, bound = float((p - q).abs().max()), tol(p, rate_of(fopt, i))
                worst = max(worst, err / bound)
                assert err <= bound, (path, decoupled, k, i, err, bound)
                q.copy_(p)
        print(f"{path}, decoupled={decoupled}, step {k + 1}: worst error / bound = {worst:.3f}")


def test_a_parameter_of_the_zero_decay_group_is_not_decayed():
    dev = torch.device("cuda:0")
    model = make_model(dev)
    _, opt = make_group_opt(model, decay_groups(model), weight_decay=WD, decoupled_weight_decay=True)
    zero = [torch.zeros_like(p) for p in model.all_params()]
    before = [bits(p) for p in opt.params]
    for _ in range(3):
        set_grads(model, zero)
        opt.step()
    kept = changed = 0
    for p, old, wd in zip(opt.params, before, (r.wd for r in opt._recs)):
        same = torch.equal(bits(p), old)
        assert same or wd != 0.0, (tuple(p.shape), wd)      # (a decayed parameter that is all zeros stays as it is, too)
        kept, changed = kept + (wd == 0.0), changed + (not same)
    assert kept > len(model.extra) and changed > 0          # the 1-D parameters of the site too, and its matrices did decay


def assert_dicts_equal(a, b):
    assert a["param_groups"] == b["param_groups"] and a["flat_adam"] == b["flat_adam"] and a["state"].keys() == b["state"].keys()
    for i in a["state"]:
        assert a["state"][i].keys() == b["state"][i].keys()
        for k in a["state"][i]:
            assert torch.equal(a["state"][i][k], b["state"][i][k]), (i, k)


@pytest.mark.parametrize("path", ["device", "plain"])
def test_without_a_group_decay_everything_is_what_it_was(path):
    """no group names a decay: the groups are those of the learning rates alone, each with the constructor's decay, and naming that same
    decay in every group changes neither the dict nor a bit"""
    dev = torch.device("cuda:0")
    a = make_model(dev)
    b = copy.deepcopy(a)
    grads = fixed_grads(a, 4, dev)
    kw = dict(weight_decay=WD, **(dict(max_grad_norm=20.0, skip_nonfinite=True) if path == "device" else {}))
    _, oa = make_opt(a, **kw)                                # {"params": extra, "lr": LR_X}: no key anywhere
    _, ob = make_group_opt(b, decay_groups(b, wd0=WD, wd_rest=WD), **kw)
    for k in range(4):
        set_grads(a, grads[k]); oa.step()
        set_grads(b, grads[k]); ob.step()
    assert_flats_equal(flats(oa), flats(ob), "group decay equal to the optimizer's")
    sa, sb = oa.state_dict(), ob.state_dict()
    assert_dicts_equal(sa, sb)
    assert "report_grad_norms" not in sa["flat_adam"]
    assert [(g["lr"], g["initial_lr"], g["weight_decay"]) for g in sa["param_groups"]] == [(lr0, lr0, WD) for lr0, _ in oa._groups()]
    assert [lr0 for lr0, _ in oa._groups()] in ([LR, LR_X], [LR_X, LR]) and oa._group_decays() == [WD, WD]
    assert all(set(g) == {"lr", "initial_lr", "betas", "eps", "weight_decay", "params"} for g in sa["param_groups"])
    assert sorted(i for g in sa["param_groups"] for i in g["params"]) == list(range(len(oa.params)))
    ta, tb = oa.torch_param_groups(), ob.torch_param_groups()
    assert [(g["lr"], g["weight_decay"], [id(p) for p in g["params"]]) for g in ta] == \
        [(lr0, WD, [id(oa.params[i]) for i in idx]) for lr0, idx in oa._groups()]
    assert [(g["lr"], g["weight_decay"], len(g["params"])) for g in ta] == [(g["lr"], g["weight_decay"], len(g["params"])) for g in tb]


GROUP_KW = dict(weight_decay=WD, step_size=2, gamma=0.5, max_grad_norm=20.0, decoupled_weight_decay=True, skip_nonfinite=True)


def test_resume_restores_each_groups_decay_and_interchanges_with_torch():
    dev = torch.device("cuda:0")
    a = make_model(dev)
    b = copy.deepcopy(a)
    grads = fixed_grads(a, 7, dev)
    _, oa = make_group_opt(a, decay_groups(a), **GROUP_KW)
    for k in range(6):
        set_grads(a, grads[k]); oa.step(); oa.epoch_end()
    _, ob = make_group_opt(b, decay_groups(b), **GROUP_KW)
    for k in range(3):
        set_grads(b, grads[k]); ob.step(); ob.epoch_end()
    sd = ob.state_dict()
    saved = [g["weight_decay"] for g in sd["param_groups"]]
    assert saved == ob._group_decays() and sorted(saved) == [0.0, 0.0, WD]
    buf = io.BytesIO()
    torch.save(sd, buf)
    buf.seek(0)
    sd2 = torch.load(buf)
    # a fresh optimizer with the same grouping but other decays everywhere: the dict's must win, group by group
    _, oc = make_group_opt(b, decay_groups(b, wd0=0.25, wd_rest=0.5), **{**GROUP_KW, "weight_decay": 0.125})
    assert oc._group_decays() != saved
    oc.load_state_dict(sd2)
    assert oc._group_decays() == saved and [lr0 for lr0, _ in oc._groups()] == [lr0 for lr0, _ in ob._groups()]
    for k in range(3, 6):
        set_grads(b, grads[k]); oc.step(); oc.epoch_end()
    assert_flats_equal(flats(oa), flats(oc), "resumed run with group decays")
    assert int(oc.applied_steps.item()) == 6
    # torch.optim.AdamW over the same groups loads the dict ...
    topt = torch.optim.AdamW(oc.torch_param_groups(), lr=LR, weight_decay=0.125)
    topt.load_state_dict(oc.state_dict())
    assert [g["weight_decay"] for g in topt.param_groups] == saved
    # ... and the dict that optimizer writes loads back, decays included
    tsd = topt.state_dict()
    for g, wd in zip(tsd["param_groups"], (0.03, 0.0, 0.07)):
        g["weight_decay"] = wd
    _, od = make_group_opt(b, decay_groups(b), **GROUP_KW)
    od.load_state_dict(tsd)
    assert od._group_decays() == [0.03, 0.0, 0.07] and int(od.applied_steps.item()) == 6
    assert [g["weight_decay"] for g in od.state_dict()["param_groups"]] == [0.03, 0.0, 0.07]


# ---- range norms at the C ABI ------------------------------------------------------------------------------------------
PATH_LENGTHS = (0, 1, 3, 4, 1023, 1024, 1025, 4100, 300001)     # empty; scalar tails; one block, its edges; several; > 256 blocks in one range
MANY_LENGTHS = tuple(1 + (7 * i) % 9 for i in range(300))       # > 256 ranges and > 64 per round of a block's waves, 1 .. 9 elements each


class AbiRanges:
    """ranges of the given lengths cut from one flat tensor per stream (param, grad, exp_avg, exp_avg_sq), every start 16-byte aligned,
    with the workspace, the uploaded table and a report buffer: what a caller of the C ABI holds"""

    def __init__(self, lengths, dev, seed=11, scale=0.5):
        from avmoe_amd import _capi, _capi_moe as cm
        self.cm, self.L, self.scale, self.n = cm, _capi.lib(), scale, len(lengths)
        self.spans, off = [], 0
        for n in lengths:
            self.spans.append((off, off + n))
            off += (n + 3) // 4 * 4
        total = off + 4
        g = torch.Generator().manual_seed(seed)
        self.g = torch.randn(total, generator=g).to(dev)
        self.p = torch.randn(total, generator=g).to(dev)
        self.m, self.v = torch.zeros_like(self.p), torch.zeros_like(self.p)
        arr = (cm.OptRange * self.n)()
        for r, (o, e) in zip(arr, self.spans):
            r.param, r.grad, r.exp_avg, r.exp_avg_sq = (t.data_ptr() + 4 * o for t in (self.p, self.g, self.m, self.v))
            r.n, r.lr, r.weight_decay = e - o, 1e-3, 0.0
            assert r.grad % 16 == 0
        lay = cm.OptLayout()
        nbytes = self.L.avmoe_opt_workspace_bytes(arr, self.n, C.byref(lay))
        assert nbytes > 0 and lay.n_blocks == sum((n + 1023) // 1024 for n in lengths)
        self.n_blocks = int(lay.n_blocks)
        self.ws = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
        img = torch.empty(int(lay.table_bytes), dtype=torch.uint8)
        assert self.L.avmoe_opt_table_build(arr, self.n, img.data_ptr(), int(lay.table_bytes)) == 0
        sb = int(lay.state_bytes)
        self.ws[sb:sb + int(lay.table_bytes)].copy_(img)
        self.state_ptr, self.table_ptr = self.ws.data_ptr(), self.ws.data_ptr() + sb
        self.partials_ptr = self.table_ptr + int(lay.table_bytes)
        rb = self.L.avmoe_opt_report_bytes(self.n)
        assert rb == 16 + (4 * self.n + 15) // 16 * 16
        self.report = torch.full((rb,), 0x5a, dtype=torch.uint8, device=dev)      # needs no initialisation: garbage before the first call
        assert self.report.data_ptr() % 16 == 0 and self.ws.data_ptr() % 16 == 0
        torch.cuda.synchronize()

    def norm(self, flags=0):
        cm = self.cm
        st = self.L.avmoe_opt_grad_norm_report(self.table_ptr, self.n, self.n_blocks, self.partials_ptr, self.state_ptr, self.scale, 0.0,
                                               flags | cm.OPT_REPORT, 0.9, 0.999, torch.cuda.current_stream().cuda_stream, None, None,
                                               self.report.data_ptr())
        assert st == 0, self.L.avmoe_last_error()
        torch.cuda.synchronize()
        hdr = self.report[:16].view(torch.int32).cpu().tolist()
        assert hdr[1] == self.n and hdr[2:] == [0, 0]
        return self.report[16:16 + 4 * self.n].view(torch.float32).clone(), hdr[0]

    def update(self, flags=0):
        st = self.L.avmoe_opt_adam_step_ema(self.table_ptr, self.n, self.n_blocks, self.state_ptr, 0.9, 0.999, 1e-8, self.scale, flags,
                                            torch.cuda.current_stream().cuda_stream, None)
        assert st == 0, self.L.avmoe_last_error()
        torch.cuda.synchronize()

    def state(self, name):
        o, dt = self.cm.OPT_STATE_FIELDS[name]
        return self.ws[o:o + (8 if dt == "int64" else 4)].view(getattr(torch, dt))[0].item()

    def reference(self):
        """fp64 norms of (gradient * scale) per range, and the fp64 norm of all of them"""
        ref = [float(torch.linalg.vector_norm(self.g[o:e].double() * self.scale)) for o, e in self.spans]
        return ref, math.sqrt(sum(x * x for x in ref))


def check_norms(h, norms, ref, skip=()):
    got, worst = norms.cpu().double().tolist(), 0.0
    for r, (x, want, (o, e)) in enumerate(zip(got, ref, h.spans)):
        if r in skip:
            continue
        if e == o:
            assert x == 0.0 and want == 0.0, r                # a range without elements reports exactly 0
            continue
        worst = max(worst, abs(x - want) / want)
        assert want > 0 and abs(x - want) <= NORM_TOL * want, (r, e - o, x, want)
    return got, worst


@pytest.fixture(scope="module")
def path_ranges():
    h = AbiRanges(PATH_LENGTHS, torch.device("cuda:0"))
    return h, h.reference()


@pytest.mark.parametrize("which", ["paths", "many"])
def test_range_norms_at_the_c_abi(which, path_ranges):
    if which == "paths":
        h, (ref, ref_total) = path_ranges
    else:
        h = AbiRanges(MANY_LENGTHS, torch.device("cuda:0"), seed=12)
        ref, ref_total = h.reference()
        assert h.n == 300 and set(MANY_LENGTHS) == set(range(1, 10))
    norms, first = h.norm()
    got, worst = check_norms(h, norms, ref)
    total = float(h.state("total_norm"))
    mine = math.sqrt(sum(x * x for x in got))
    print(f"{which}: {h.n} ranges, {h.n_blocks} blocks: worst relative error of a range norm {worst:.3e} (bound {NORM_TOL:.3e}); total_norm {total!r}, "
          f"from the range norms {mine!r}, fp64 {ref_total!r}")
    assert abs(mine - total) <= TOTAL_TOL * total
    assert abs(total - ref_total) <= TOTAL_TOL * ref_total       # without clipping and skipping the flag alone makes it the true norm
    assert first == -1 and h.state("clip_coef") == 1.0 and h.state("skip") == 0
    again, first2 = h.norm()
    assert torch.equal(bits(norms), bits(again)) and first2 == -1          # same input, same bits


def test_first_nonfinite_range_is_located_and_the_step_is_skipped(path_ranges):
    shared, (ref, _) = path_ranges
    h = AbiRanges(PATH_LENGTHS, torch.device("cuda:0"))     # its own buffers with the same gradients: the shared ones stay as they are
    assert torch.equal(h.g, shared.g)
    cm = h.cm
    (o6, e6), (o3, e3) = h.spans[6], h.spans[3]
    good6, good3 = h.g[o6 + 1000].clone(), h.g[o3 + 2].clone()
    h.g[o6 + 1000] = float("nan")
    h.g[o3 + 2] = float("inf")
    before = [t.clone() for t in (h.p, h.m, h.v)]
    norms, first = h.norm(cm.OPT_SKIP_NONFINITE)
    assert first == 3
    got, _ = check_norms(h, norms, ref, skip=(3, 6))
    assert got[3] == float("inf") and math.isnan(got[6])
    assert h.state("skip") == 1 and h.state("skipped_steps") == 1 and h.state("applied_steps") == 0
    h.update(cm.OPT_SKIP_NONFINITE)
    for t, old in zip((h.p, h.m, h.v), before):
        assert torch.equal(bits(t), bits(old))
    h.g[o3 + 2] = good3                                      # the Inf gone, the NaN further back is now the first
    _, first = h.norm(cm.OPT_SKIP_NONFINITE)
    assert first == 6 and h.state("skip") == 1
    h.g[o6 + 1000] = good6
    norms, first = h.norm(cm.OPT_SKIP_NONFINITE)
    assert first == -1 and h.state("skip") == 0 and h.state("applied_steps") == 1
    check_norms(h, norms, ref)
    h.update(cm.OPT_SKIP_NONFINITE)
    assert not torch.equal(bits(h.p), bits(before[0]))       # and this step is applied


# ---- the facade --------------------------------------------------------------------------------------------------------
def all_flats(opt):
    return [tuple(s[k].clone() for k in ("p", "m", "v", "e") if k in s) for s in opt.state]


def assert_all_equal(a, b, what):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert len(x) == len(y)
        for j, (u, w) in enumerate(zip(x, y)):
            assert torch.equal(bits(u), bits(w)), (what, i, j)


def test_the_report_changes_nothing_else():
    from avmoe_amd.train import LRSchedule
    dev = torch.device("cuda:0")
    a = make_model(dev)
    grads = fixed_grads(a, 5, dev)
    full = dict(weight_decay=WD, max_grad_norm=20.0, skip_nonfinite=True, ema_decay=0.9,
                lr_schedule=LRSchedule(warmup_steps=2, warmup_start=0.1, decay_kind="cosine", total_steps=9, min_factor=0.05))
    for kw in (full, dict(weight_decay=WD, decoupled_weight_decay=True)):
        ma, mb = copy.deepcopy(a), copy.deepcopy(a)
        _, on = make_opt(ma, report_grad_norms=True, **kw)
        _, off = make_opt(mb, **kw)
        for k in range(5):
            set_grads(ma, grads[k]); on.step()
            set_grads(mb, grads[k]); off.step()
        assert_all_equal(all_flats(on), all_flats(off), "report on / off")
        words_on, words_off = on._ws[:64].view(torch.int32).cpu().tolist(), off._ws[:64].view(torch.int32).cpu().tolist()
        assert float(on.state_block["clip_coef"].item()) < 1.0 if "max_grad_norm" in kw else float(on.state_block["clip_coef"].item()) == 1.0
        if "max_grad_norm" in kw:
            assert words_on == words_off                     # every word of the state block
        else:                                                # neither clipping nor skipping: the norm is now the true one, 0 without the option
            assert words_on[1:] == words_off[1:] and float(off.last_grad_norm.item()) == 0.0
            want = math.sqrt(sum(float(p.grad.double().pow(2).sum()) for p in on.params))
            assert abs(float(on.last_grad_norm.item()) - want) <= NORM_TOL * want
        assert int(on.first_nonfinite_param.item()) == -1
        assert "report_grad_norms" not in off.state_dict()["flat_adam"] and on.state_dict()["flat_adam"]["report_grad_norms"] is True


def test_facade_reports_every_parameters_norm_by_name():
    from avmoe_amd._capi import AvmoeError
    dev = torch.device("cuda:0")
    model = make_model(dev)
    _, opt = make_opt(model, report_grad_norms=True)         # the option alone selects the device path
    assert opt._device
    set_grads(model, fixed_grads(model, 1, dev)[0])
    opt.step()
    norms, first = opt.last_param_grad_norms, opt.first_nonfinite_param
    assert norms.is_cuda and norms.dtype == torch.float32 and tuple(norms.shape) == (len(opt.params),)
    assert first.is_cuda and first.dtype == torch.int32 and first.dim() == 0 and int(first.item()) == -1
    for i, (x, p) in enumerate(zip(norms.cpu().double().tolist(), opt.params)):
        want = float(p.grad.double().norm())
        assert want > 0 and abs(x - want) <= NORM_TOL * want, (i, x, want)
    names, named = opt.param_names(model), dict(model.named_parameters())
    assert len(names) == len(opt.params) and all(named[k] is p for k, p in zip(names, opt.params))
    partial = opt.param_names(model.site)                    # a parameter the module does not own has no name
    assert [k is None for k in partial] == [any(p is e for e in model.extra) for p in opt.params] and None in partial
    # which parameter made the step skip
    victim = 5
    opt.params[victim].grad.view(-1)[0] = float("nan")
    opt.step()
    assert int(opt.first_nonfinite_param.item()) == victim and names[victim] is not None
    assert math.isnan(float(opt.last_param_grad_norms[victim].item()))
    _, plain = make_opt(make_model(dev), skip_nonfinite=True)
    for name in ("last_param_grad_norms", "first_nonfinite_param"):
        with pytest.raises(AvmoeError, match="report_grad_norms"):
            getattr(plain, name)
    assert plain.param_names(model) == [None] * len(plain.params)


def test_a_captured_step_rewrites_the_report_on_replay():
    dev = torch.device("cuda:0")
    a = make_model(dev)
    b = copy.deepcopy(a)
    grads = fixed_grads(a, 3, dev)
    kw = dict(weight_decay=WD, max_grad_norm=20.0, skip_nonfinite=True, report_grad_norms=True)
    _, oa = make_opt(a, **kw)
    _, ob = make_opt(b, **kw)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    eager = []
    with torch.cuda.stream(s):                               # three eager steps (they also load the kernels before the capture)
        for k in range(3):
            set_grads(a, grads[k]); oa.step()
            eager.append(oa._report.clone())
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        ob.step()
    torch.cuda.synchronize()
    assert int(ob.applied_steps.item()) == 0                 # capturing runs nothing
    for k in range(3):
        set_grads(b, grads[k])
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(ob._report, eager[k]), k          # header and norms, bit for bit
    assert not torch.equal(eager[0], eager[1])
    assert_flats_equal(flats(oa), flats(ob), "graph replay with the report")
