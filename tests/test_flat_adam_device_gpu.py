"""FlatAdam's device path (avmoe_amd.train, include/avmoe.h: avmoe_opt_*): global-norm clipping, AdamW, skipping of non-finite steps,
resume and graph capture -- against PyTorch itself on the same GPU (torch.optim.Adam / AdamW + torch.nn.utils.clip_grad_norm_) fed
bit-identical gradients.  The model everywhere: one real adapter site (its gradients arrive through the reducer's gradient sink) and a
second bucket of plain parameters of 1, 2, 7 and 130 elements, with two learning-rate groups.

Tolerances.  Norm: 2^-23 relative to the fp64 norm rounded to fp32 -- the kernel's sums are exact to double rounding, so its result is
one fp32 rounding of the sum plus one of the square root away.  Adam arithmetic: the project's own bound of
tests/test_adapters_gpu.py::test_flat_adam_matches_torch_adam_and_histogram_matches_bincount, 1e-6 * max|p| + 2e-3 * lr per parameter and
step with the parameters re-synchronised after each step.  Everything that is the same kernels on the same bits is held to bit-equality."""
import copy
import io
import math

import numpy as np
import pytest
import torch

from oracle import avmoe_oracle as O
from tests.test_adapters_api import build_module

pytestmark = pytest.mark.gpu

CFG = O.AdapterConfig(Cx=64, Nx=50, Cy=48, Ny=20, reduction=4, groups=2, K=6)
LR, LR_X, WD = 3e-3, 1e-2, 1e-2
EXTRA_SIZES = (1, 2, 7, 130)                 # not multiples of 4 or 64: scalar tails and padding in the second bucket


class Model(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.site = build_module("ave", CFG)
        g = torch.Generator().manual_seed(9)
        self.extra = torch.nn.ParameterList([torch.nn.Parameter(torch.randn(n, generator=g)) for n in EXTRA_SIZES])
        with torch.no_grad():
            for k, p in self.site.named_parameters():
                if k.endswith(("gate", "gate_av")):
                    p.fill_(0.4)

    def all_params(self):
        return list(self.site.parameters()) + list(self.extra)


def make_model(dev, seed=0):
    torch.manual_seed(seed)
    return Model().to(dev).train()


def make_opt(model, **kw):
    from avmoe_amd.dp import AdapterGradReducer
    from avmoe_amd.train import FlatAdam
    red = AdapterGradReducer(model.all_params(), sites=[model.site], average=kw.pop("average", "auto"))
    kw.setdefault("lr", LR)
    opt = FlatAdam(red, param_groups=[{"params": list(model.extra), "lr": LR_X}], **kw)
    return red, opt


def batch(g, dev, S=4):
    X = torch.randn(S, CFG.Cx, CFG.Nx, 1, generator=g).to(dev)
    Y = torch.randn(S, CFG.Cy, CFG.Ny, 1, generator=g).to(dev)
    G = torch.randn(S, CFG.Cx, CFG.Nx, 1, generator=g).to(dev)
    W = [torch.randn(n, generator=g).to(dev) for n in EXTRA_SIZES]
    return X, Y, G, W


def backward(model, b):
    """a real backward: the site through its gradient sink (when a reducer holds it), the plain parameters through autograd"""
    X, Y, G, W = b
    out = model.site(X, Y)[0]
    ((out * G).sum() + sum((e * w).sum() for e, w in zip(model.extra, W))).backward()


def copy_grads(src, dst):
    with torch.no_grad():
        for p, q in zip(src.all_params(), dst.all_params()):
            q.grad.copy_(p.grad)


def norm64(params, scale=1.0):
    return math.sqrt(sum(float((p.grad.double() * scale).pow(2).sum()) for p in params))


def bits(t):
    return t.detach().clone().view(torch.int32)


def tol(p, lr):
    return 1e-6 * float(p.abs().max()) + 2e-3 * lr


def lr_of(model, p, decay):
    return (LR_X if any(p is e for e in model.extra) else LR) * decay


def host_bias_corrections(betas, step):
    """what avmoe_adam_step computes on the host: double pow of the fp32 betas, rounded to fp32"""
    b1, b2 = float(np.float32(betas[0])), float(np.float32(betas[1]))
    return np.float32(1.0 - b1 ** step), np.float32(math.sqrt(1.0 - b2 ** step))


def ulps(a, b):
    return abs(int(np.float32(a).view(np.int32)) - int(np.float32(b).view(np.int32)))


def flats(opt):
    return [(s["p"].clone(), s["m"].clone(), s["v"].clone()) for s in opt.state]


def assert_flats_equal(a, b, what=""):
    for i, (x, y) in enumerate(zip(a, b)):
        for name, u, w in zip("pmv", x, y):
            assert torch.equal(bits(u), bits(w)), (what, i, name)


# ---------------------------------------------------------------------------------------------------------------------
def test_grad_norm_is_exact_to_fp32_rounding_covers_parameters_only_and_repeats():
    dev = torch.device("cuda:0")
    model = make_model(dev)
    red, opt = make_opt(model, skip_nonfinite=True)
    assert len(red.buckets) == 2 and len(red.sinks) == 1
    red.begin(sync=True)
    backward(model, batch(torch.Generator().manual_seed(1), dev))
    red.finish()
    for b in red.buckets:                                   # alignment padding belongs to no range: whatever it holds must not count
        pad = torch.ones(b.flat.numel(), dtype=torch.bool, device=dev)
        for p, o in zip(b.params, b.offsets):
            pad[o:o + p.numel()] = False
        assert int(pad.sum()) > 0
        assert float(b.flat[pad].abs().max()) == 0.0        # (and the real backward left it zero)
        b.flat[pad] = 1000.0
    params = opt.params
    assert len(params) == len(model.all_params()) and {id(p) for p in params} == {id(p) for p in model.all_params()}
    got = []
    for scale in (1.0, 1.0, 0.125):
        opt.grad_scale = scale
        opt.step()
        want = norm64(params, scale)
        n = float(opt.last_grad_norm.item())
        print(f"grad norm: scale {scale} kernel {n!r} fp64 {want!r} rel {abs(n - float(np.float32(want))) / want:.3e}")
        assert want > 0 and abs(n - float(np.float32(want))) <= 2.0 ** -23 * want, (scale, n, want)
        got.append(int(bits(opt.last_grad_norm).item()))
    assert got[0] == got[1]                                 # same input, same bits
    assert int(opt.applied_steps.item()) == 3 and int(opt.skipped_steps.item()) == 0 and opt.t == 3


@pytest.mark.parametrize("decoupled", [False, True])
@pytest.mark.parametrize("clip", ["above", "below"])
def test_clipping_and_adamw_match_torch_and_factor_one_is_bit_equal_to_the_plain_path(clip, decoupled):
    dev = torch.device("cuda:0")
    ref = make_model(dev)
    fused, plain = copy.deepcopy(ref), copy.deepcopy(ref)
    g = torch.Generator().manual_seed(2)
    batches = [batch(g, dev) for _ in range(3)]
    ref.zero_grad()
    backward(ref, batches[0])
    first = norm64(ref.all_params())
    max_norm = 1e6 if clip == "above" else 0.05 * first     # above: the factor is exactly 1 ; below: a factor of about 0.05
    betas = (0.9, 0.999)
    groups = [{"params": list(ref.site.parameters()), "lr": LR}, {"params": list(ref.extra), "lr": LR_X}]
    topt = (torch.optim.AdamW if decoupled else torch.optim.Adam)(groups, lr=LR, betas=betas, weight_decay=WD)
    sched = torch.optim.lr_scheduler.StepLR(topt, step_size=1, gamma=0.5)
    red, fopt = make_opt(fused, weight_decay=WD, step_size=1, gamma=0.5, max_grad_norm=max_norm, decoupled_weight_decay=decoupled)
    check_plain = clip == "above" and not decoupled
    if check_plain:
        pred, popt = make_opt(plain, weight_decay=WD, step_size=1, gamma=0.5)
    for step in range(3):
        decay = 0.5 ** step
        topt.zero_grad()
        backward(ref, batches[step])
        red.begin(sync=True)
        backward(fused, batches[step])                      # fills the buckets through the gradient sink and the hooks
        red.finish()
        copy_grads(ref, fused)                              # bit-identical gradients: the comparison is about the optimizer only
        if check_plain:
            copy_grads(ref, plain)
        before = [b.flat.clone() for b in red.buckets]
        total = torch.nn.utils.clip_grad_norm_(ref.all_params(), max_norm)
        topt.step(); sched.step()
        fopt.step()
        for b, old in zip(red.buckets, before):             # the factor is applied in the update: the buckets are not rescaled
            assert torch.equal(bits(b.flat), bits(old))
        n, coef = float(fopt.last_grad_norm.item()), float(fopt.state_block["clip_coef"].item())
        assert abs(n - float(total)) <= 1e-5 * float(total)
        assert coef == 1.0 if clip == "above" else abs(coef - max_norm / n) <= 1e-5 * coef
        bc = (float(fopt.state_block["bc1"].item()), float(fopt.state_block["bc2_sqrt"].item()))
        hbc = host_bias_corrections(betas, step + 1)
        assert ulps(bc[0], hbc[0]) <= 1 and ulps(bc[1], hbc[1]) <= 1, (step, bc, hbc)
        if check_plain:
            popt.step()
            same_bc = ulps(bc[0], hbc[0]) == 0 and ulps(bc[1], hbc[1]) == 0
            assert same_bc or step > 0                      # beta^1 is exact on host and device alike
            print(f"step {step + 1}: device bias corrections {bc}, host {hbc}, bit-equal {same_bc}")
            for p, q in zip(plain.all_params(), fused.all_params()):
                if same_bc:
                    assert torch.equal(bits(p), bits(q)), step
                else:
                    assert float((p - q).abs().max()) <= tol(p, lr_of(plain, p, decay)), step
            for sp, sf in zip(popt.state, fopt.state):      # the moments do not depend on the bias corrections
                assert torch.equal(bits(sp["m"]), bits(sf["m"])) and torch.equal(bits(sp["v"]), bits(sf["v"])), step
            popt.epoch_end(); pred.zero_grad()
        fopt.epoch_end(); red.zero_grad()
        with torch.no_grad():
            worst = 0.0
            for (k, p), q in zip([(k, p) for k, p in ref.named_parameters()], [q for _, q in fused.named_parameters()]):
                err = float((p - q).abs().max())
                worst = max(worst, err / tol(p, lr_of(ref, p, decay)))
                assert err <= tol(p, lr_of(ref, p, decay)), (step, k, err)
                q.copy_(p)
            if check_plain:
                for p, q in zip(ref.all_params(), plain.all_params()):
                    q.copy_(p)
            print(f"step {step + 1} ({clip}, decoupled={decoupled}): worst error / bound = {worst:.3f}, norm {n:.4f}, factor {coef:.4f}")
    assert int(fopt.applied_steps.item()) == 3


@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
def test_nonfinite_step_is_skipped_without_touching_anything(bad):
    dev = torch.device("cuda:0")
    ref = make_model(dev)
    fused = copy.deepcopy(ref)
    g = torch.Generator().manual_seed(3)
    topt = torch.optim.Adam([{"params": list(ref.site.parameters()), "lr": LR}, {"params": list(ref.extra), "lr": LR_X}], lr=LR,
                            weight_decay=WD)
    red, fopt = make_opt(fused, weight_decay=WD, skip_nonfinite=True, max_grad_norm=1e6)
    for step, poison in enumerate([False, True, False]):
        b = batch(g, dev)
        topt.zero_grad()
        backward(ref, b)
        red.begin(sync=True)
        backward(fused, b)
        red.finish()
        copy_grads(ref, fused)
        if poison:
            victim = fused.all_params()[3]
            victim.grad.view(-1)[victim.numel() // 2] = bad          # a value in a tensor, written on the device
            before = flats(fopt)
            fopt.step()
            assert_flats_equal(before, flats(fopt), "skipped step")
            assert int(fopt.skipped_steps.item()) == 1 and int(fopt.applied_steps.item()) == 1 and fopt.t == 2
            assert not math.isfinite(float(fopt.last_grad_norm.item()))
        else:                                               # the torch optimizer simply does not step on the poisoned gradient
            topt.step()
            fopt.step()
            applied = 1 if step == 0 else 2
            assert int(fopt.applied_steps.item()) == applied
            hbc = host_bias_corrections((0.9, 0.999), applied)       # the step after the skip uses the bias correction of step 2, not 3
            assert ulps(float(fopt.state_block["bc1"].item()), hbc[0]) <= 1 and ulps(float(fopt.state_block["bc2_sqrt"].item()), hbc[1]) <= 1
            with torch.no_grad():
                for (k, p), q in zip(list(ref.named_parameters()), [q for _, q in fused.named_parameters()]):
                    assert float((p - q).abs().max()) <= tol(p, lr_of(ref, p, 1.0)), (step, k)
                    q.copy_(p)
        red.zero_grad()
    assert int(fopt.skipped_steps.item()) == 1 and int(fopt.applied_steps.item()) == 2 and fopt.t == 3


def test_without_skip_nonfinite_nothing_is_held_back():
    dev = torch.device("cuda:0")
    ref = make_model(dev)
    fused = copy.deepcopy(ref)
    topt = torch.optim.Adam(ref.all_params(), lr=LR)
    red, fopt = make_opt(fused, max_grad_norm=1.0)
    b = batch(torch.Generator().manual_seed(4), dev)
    backward(ref, b)
    red.begin(sync=True)
    backward(fused, b)
    red.finish()
    copy_grads(ref, fused)
    for m in (ref, fused):
        v = m.all_params()[3]
        v.grad.view(-1)[0] = float("inf")
    torch.nn.utils.clip_grad_norm_(ref.all_params(), 1.0)
    topt.step()
    fopt.step()
    assert not bool(torch.isfinite(ref.all_params()[3]).all())      # torch lets it through ...
    assert not bool(torch.isfinite(fused.all_params()[3]).all())    # ... and so does FlatAdam
    assert int(fopt.applied_steps.item()) == 1 and int(fopt.skipped_steps.item()) == 0


# ---------------------------------------------------------------------------------------------------------------------
def fixed_grads(model, n_steps, dev, seed=5):
    g = torch.Generator().manual_seed(seed)
    return [[torch.randn(p.shape, generator=g).to(dev) for p in model.all_params()] for _ in range(n_steps)]


def set_grads(model, grads):
    with torch.no_grad():
        for p, gr in zip(model.all_params(), grads):
            p.grad.copy_(gr)


RESUME_KW = dict(weight_decay=WD, step_size=2, gamma=0.5, max_grad_norm=20.0, decoupled_weight_decay=True, skip_nonfinite=True)


def test_resume_is_bit_equal_to_an_uninterrupted_run():
    dev = torch.device("cuda:0")
    a = make_model(dev)
    b = copy.deepcopy(a)
    grads = fixed_grads(a, 4, dev)
    _, oa = make_opt(a, **RESUME_KW)
    for k in range(4):
        set_grads(a, grads[k]); oa.step(); oa.epoch_end()
    _, ob = make_opt(b, **RESUME_KW)
    for k in range(2):
        set_grads(b, grads[k]); ob.step(); ob.epoch_end()
    sd = ob.state_dict()
    buf = io.BytesIO()
    torch.save(sd, buf)                                     # the dict survives torch.save / torch.load
    buf.seek(0)
    sd2 = torch.load(buf)
    assert sd2["flat_adam"] == sd["flat_adam"] and sd2["param_groups"] == sd["param_groups"]
    assert all(torch.equal(sd2["state"][i][k], sd["state"][i][k]) for i in sd["state"] for k in ("step", "exp_avg", "exp_avg_sq"))
    assert sd["flat_adam"]["t"] == 2 and sd["flat_adam"]["epoch"] == 2 and float(sd["state"][0]["step"]) == 2.0
    assert all(v["exp_avg"].device.type == "cpu" and v["exp_avg"].shape == p.shape for v, p in zip(sd["state"].values(), ob.params))
    _, oc = make_opt(b, **RESUME_KW)                         # a fresh optimizer over the parameters as the interrupted run left them
    oc.load_state_dict(sd2)
    assert oc.t == 2 and oc.epoch == 2 and int(oc.applied_steps.item()) == 2
    for k in range(2, 4):
        set_grads(b, grads[k]); oc.step(); oc.epoch_end()
    assert_flats_equal(flats(oa), flats(oc), "resumed run")
    assert int(oc.applied_steps.item()) == 4 and torch.equal(bits(oa.last_grad_norm), bits(oc.last_grad_norm))


def test_state_dict_interchanges_with_torch_adamw():
    dev = torch.device("cuda:0")
    ref = make_model(dev)
    fused = copy.deepcopy(ref)
    grads = fixed_grads(ref, 6, dev)
    kw = dict(weight_decay=WD, decoupled_weight_decay=True)
    _, fopt = make_opt(fused, **kw)
    ref_of = {id(q): p for p, q in zip(ref.all_params(), fused.all_params())}

    def torch_opt(fo):                                      # AdamW over the same parameters in FlatAdam's order and grouping
        return torch.optim.AdamW([{"params": [ref_of[id(q)] for q in g_["params"]], "lr": g_["lr"]} for g_ in fo.torch_param_groups()],
                                 lr=LR, weight_decay=WD)

    def compare_and_sync(what):
        with torch.no_grad():
            for p, q in zip(ref.all_params(), fused.all_params()):
                assert float((p - q).abs().max()) <= tol(p, lr_of(ref, p, 1.0)), what
                q.copy_(p)

    # FlatAdam -> torch: two steps here, then both continue from the same state
    for k in range(2):
        set_grads(fused, grads[k]); fopt.step()
    with torch.no_grad():
        for p, q in zip(ref.all_params(), fused.all_params()):
            p.copy_(q)
    topt = torch_opt(fopt)
    topt.load_state_dict(fopt.state_dict())
    for p, gr in zip(ref.all_params(), grads[2]):
        p.grad = gr.clone()
    set_grads(fused, grads[2])
    topt.step(); fopt.step()
    compare_and_sync("FlatAdam -> AdamW")
    # torch -> FlatAdam: torch goes on for two steps, a fresh FlatAdam takes its state over
    for k in (3, 4):
        for p, gr in zip(ref.all_params(), grads[k]):
            p.grad = gr.clone()
        topt.step()
    with torch.no_grad():
        for p, q in zip(ref.all_params(), fused.all_params()):
            q.copy_(p)
    _, fopt2 = make_opt(fused, **kw)
    sd = topt.state_dict()
    sd["somebody_elses_key"] = 1                            # unknown keys are ignored
    fopt2.load_state_dict(sd)
    assert int(fopt2.applied_steps.item()) == 5 and fopt2.t == 5
    for p, gr in zip(ref.all_params(), grads[5]):
        p.grad = gr.clone()
    set_grads(fused, grads[5])
    topt.step(); fopt2.step()
    compare_and_sync("AdamW -> FlatAdam")


def test_load_state_dict_names_the_mismatching_parameter():
    dev = torch.device("cuda:0")
    model = make_model(dev)
    _, opt = make_opt(model, skip_nonfinite=True)
    sd = opt.state_dict()
    bad = copy.deepcopy(sd)
    bad["state"][5]["exp_avg"] = torch.zeros(3, 3)
    with pytest.raises(ValueError, match="parameter index 5"):
        opt.load_state_dict(bad)
    bad = copy.deepcopy(sd)
    del bad["state"][7]
    with pytest.raises(ValueError, match="parameter index 7"):
        opt.load_state_dict(bad)
    bad = copy.deepcopy(sd)
    bad["param_groups"][0]["params"] = bad["param_groups"][0]["params"][:-1]
    with pytest.raises(ValueError, match="parameter group 0"):
        opt.load_state_dict(bad)
    bad = copy.deepcopy(sd)
    bad["param_groups"] = bad["param_groups"][:1]
    with pytest.raises(ValueError, match="parameter groups"):
        opt.load_state_dict(bad)
    opt.load_state_dict(sd)                                 # and the untouched dict still loads


def test_plain_path_state_dict_resumes_too():
    """the plain path counts step() calls (self.t): its state dict carries them as `step` and a reloaded optimizer continues bit for bit"""
    dev = torch.device("cuda:0")
    a = make_model(dev)
    b = copy.deepcopy(a)
    grads = fixed_grads(a, 3, dev)
    _, oa = make_opt(a, weight_decay=WD)
    for k in range(3):
        set_grads(a, grads[k]); oa.step()
    _, ob = make_opt(b, weight_decay=WD)
    for k in range(2):
        set_grads(b, grads[k]); ob.step()
    sd = ob.state_dict()
    assert float(sd["state"][0]["step"]) == 2.0
    _, oc = make_opt(b, weight_decay=WD)
    oc.load_state_dict(sd)
    set_grads(b, grads[2]); oc.step()
    assert_flats_equal(flats(oa), flats(oc), "plain resume")
    with pytest.raises(Exception):
        oa.applied_steps                                    # device tensors exist on the device path only


# ---------------------------------------------------------------------------------------------------------------------
def test_step_is_capturable_and_replays_with_new_gradients():
    dev = torch.device("cuda:0")
    a = make_model(dev)
    b = copy.deepcopy(a)
    grads = fixed_grads(a, 3, dev)
    kw = dict(weight_decay=WD, max_grad_norm=20.0, skip_nonfinite=True)
    _, oa = make_opt(a, **kw)
    _, ob = make_opt(b, **kw)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                               # three eager steps (they also load the kernels before the capture)
        for k in range(3):
            set_grads(a, grads[k]); oa.step()
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
    assert int(ob.applied_steps.item()) == 3 and int(ob.skipped_steps.item()) == 0
    assert_flats_equal(flats(oa), flats(ob), "graph replay")
    assert torch.equal(bits(oa.last_grad_norm), bits(ob.last_grad_norm))
    assert float(oa.state_block["clip_coef"].item()) < 1.0        # the captured step did clip
