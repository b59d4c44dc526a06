"""FlatAdam's later options -- per-parameter gradient norms, stochastic weight averaging, averaged buffers, SAM / ASAM, layer-wise trust
ratios, Prodigy, Muon, per-group settings -- and its resume path held to bit-equality with the library as it was before the optimizer
moved into its own module (avmoe_amd/flat_adam.py).  tests/test_flat_adam_flag_matrix_gpu.py does the same for the 32 combinations of the
five first options and no resume; this file is a NAMED LIST of combinations, not a power set: each option once with clipping, and the
compositions whose branches of step(), _update(), state_dict() and load_state_dict() differ.

The model is the flag matrix's -- plain parameters of 1, 3, 4, 5, 1023, 1024, 1025 and 2049 elements in two buckets -- with the last two
shaped as matrices, (205, 5) and (3, 683): rows > cols and rows < cols, each across a 1024-element block boundary, so that Muon and LAMB
see more than (2, 2) and (32, 32).  Two BatchNorm-like fp32 buffers of 5 and 64 elements serve `ema_buffers`; they are rewritten before
every step.  Parameters, gradients (SAM: both of a step) and buffers come from one closed-form integer formula of (step, element
index), exact in fp32: no random generator.  The Prodigy combinations add a part that stays from step to step (`gradients`), so that the
estimate d grows: the fixture names d0, the saved d and the last d of each.  Four steps; with skip_nonfinite the third one carries one inf and is skipped.

After step 2 `state_dict()` is taken and a second optimizer over a copy of the model (parameters and buffers as they are then) loads
it; steps 3 and 4 run on both.  The two must agree with each other and with the fixture: that pins load_state_dict().

tests/golden/flat_adam_option_matrix.json holds, per combination, the SHA-256 of
  * each bucket's p, m, v and, where the combination has them, e, x0, s -- alignment padding included -- after the last step,
  * the device words the options hand out (the Prodigy block, the buffers' shadows, and the per-parameter gradient norms, trust ratios,
    Muon norms and the SAM norm and scale, where on),
  * a canonical serialisation of the state dict of step 2 (tensor bytes and repr of everything else, in key order),
and the 64-byte state block as hex, for the first optimizer ("run") and for the resumed one ("resumed").  It was recorded TWICE, in two
processes, with this file's main on the commit the fixture names, and the two recordings agree in every combination ("left_out", the
place for one that would not, is empty):

    PYTHONPATH=<a built checkout of that commit> python tests/test_flat_adam_option_matrix_gpu.py --record PATH --commit HASH

which uses FlatAdam's public interface only and so runs unchanged on that commit."""
import hashlib
import json
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

SIZES = (1, 3, 4, 5, 1023, 1024, 1025, 2049)
SHAPES = {4: (2, 2), 1024: (32, 32), 1025: (205, 5), 2049: (3, 683)}
BUFFER_SIZES = (5, 64)
LR, LR_X, WD, GRAD_SCALE = 3e-3, 1e-2, 1e-2, 0.5
BUCKET_MB = 17200 / (1 << 20)                    # 4300 elements: 2049 + 1025 + 1024 (padded to 64s: 4224) fill the first bucket
STEPS, SAVE_STEP, INF_STEP, INF_PARAM = 4, 2, 3, 6
MAX_NORM, RHO = 1.0, 0.05
SAM_OFFSET, BUFFER_OFFSET = 16, 32               # the `step` of a SAM step's first gradient and of the buffers, beside the step's own
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "flat_adam_option_matrix.json")
_golden = None


def _sched(**swa):
    from avmoe_amd.train import LRSchedule
    return LRSchedule(warmup_steps=2, decay_kind="cosine", total_steps=6, **swa)


def _x_group(params):
    return [{"params": params[:4], "lr": LR_X}]


CLIP = dict(max_grad_norm=MAX_NORM)
# name -> (FlatAdam keywords beside lr / weight_decay / grad_scale, parameter groups of the eight parameters).  Read: "sam" in the name
# runs sam_perturb() before every step, "skip" poisons step 3, "bufs" hands the two buffers over, "sched" builds a fresh LRSchedule.
COMBOS = {
    "report": (dict(CLIP, report_grad_norms=True), _x_group),
    "swa": (dict(CLIP, swa_start=2, swa_freq=2), _x_group),
    "swa+sched_swa_lr+bufs": (dict(CLIP, swa_start=2, swa_freq=2,
                                   lr_schedule=dict(swa_start=2, swa_factor=0.5, swa_anneal_steps=2, swa_anneal="linear")), _x_group),
    "ema+bufs+skip": (dict(CLIP, ema_decay=0.9, ema_warmup=2.0, skip_nonfinite=True), _x_group),
    "sam": (dict(CLIP, sam_rho=RHO), _x_group),
    "asam+skip": (dict(CLIP, sam_rho=RHO, sam_adaptive=True, skip_nonfinite=True), _x_group),
    "lamb+adamw+trust_clip": (dict(CLIP, trust_ratio=True, trust_clip=2.0, decoupled_weight_decay=True), _x_group),
    "lamb+sam+report": (dict(CLIP, trust_ratio=True, sam_rho=RHO, report_grad_norms=True), _x_group),
    "prodigy": (dict(CLIP, prodigy=True, prodigy_d0=1e-3), _x_group),
    "prodigy+growth+safeguard+sched+ema": (dict(CLIP, prodigy=True, prodigy_d0=1e-3, prodigy_growth=1.5, prodigy_safeguard_warmup=True,
                                                lr_schedule={}, ema_decay=0.9, ema_warmup=2.0), _x_group),
    "prodigy+sam+skip": (dict(CLIP, prodigy=True, prodigy_d0=1e-3, sam_rho=RHO, skip_nonfinite=True), _x_group),
    "muon+adamw": (dict(CLIP, muon=True, decoupled_weight_decay=True), _x_group),
    "muon_plain_momentum+original+group_off": (dict(CLIP, muon=True, muon_nesterov=False, muon_scale="original"),
                                               lambda ps: _x_group(ps) + [{"params": [ps[5]], "muon": False}]),
    "muon+sam+swa+skip": (dict(CLIP, muon=True, sam_rho=RHO, swa_start=2, swa_freq=2, skip_nonfinite=True), _x_group),
    "lamb+groups": (dict(CLIP, trust_ratio=True),
                    lambda ps: [{"params": ps[:4], "lr": LR_X, "weight_decay": 0.0},
                                {"params": [ps[6]], "lr": 2e-3, "weight_decay": 0.05, "trust_ratio": False}]),
    "plain+two_groups": (dict(), lambda ps: _x_group(ps) + [{"params": ps[6:], "lr": 2e-3, "weight_decay": 0.0}]),
}
SINGLE_OPTION = ("report", "swa", "sam", "prodigy")          # (and the plain path) may never be left out of the fixture


def _closed_form(step, sizes, k0, shapes):
    """one tensor per size: ((a k + b step) / 128 mod 2048 - 1024) / 256 over the running element index k, multiples of 2^-8 in [-4, 4)"""
    out = []
    for n in sizes:
        k = torch.arange(k0 + 1, k0 + n + 1, dtype=torch.int64)
        h = (k * 2654435761 + (step + 2) * 40503) // 128 % 2048 - 1024
        out.append((h.to(torch.float32) / 256.0).reshape(shapes.get(n, (n,))))
        k0 += n
    return out


def values(step):
    return _closed_form(step, SIZES, 0, SHAPES)


def gradients(name, step):
    """the gradients of `step`.  Prodigy's estimate grows only where successive gradients agree (num sums g . (x0 - w)), so its
    combinations get a part that stays, values(0), and a quarter of the part that changes: still multiples of 2^-10, exact in fp32"""
    if "prodigy" in name:
        return [g0 + 0.25 * g for g0, g in zip(values(0), values(step))]
    return values(step)


def buffer_values(step):
    """the two buffers before `step`: in [0, 2), as a running variance may be"""
    return [0.25 * v + 1.0 for v in _closed_form(step + BUFFER_OFFSET, BUFFER_SIZES, sum(SIZES), {})]


def digest(t):
    return hashlib.sha256(t.detach().contiguous().reshape(-1).view(torch.uint8).cpu().numpy().tobytes()).hexdigest()


def _feed(h, obj):
    if isinstance(obj, torch.Tensor):
        h.update(f"T{obj.dtype}{tuple(obj.shape)}".encode())
        h.update(obj.detach().contiguous().cpu().reshape(-1).view(torch.uint8).numpy().tobytes())
    elif isinstance(obj, dict):
        h.update(b"{")
        for k in sorted(obj, key=repr):
            h.update(repr(k).encode() + b":")
            _feed(h, obj[k])
        h.update(b"}")
    elif isinstance(obj, (list, tuple)):
        h.update(b"[")
        for x in obj:
            _feed(h, x)
            h.update(b",")
        h.update(b"]")
    else:
        h.update(repr(obj).encode())


def digest_state_dict(sd):
    h = hashlib.sha256()
    _feed(h, sd)
    return h.hexdigest()


class Side:
    """one model (eight parameters, two buffers) with its reducer and optimizer"""

    def __init__(self, name, dev, param_values, buffer_tensors):
        from avmoe_amd.dp import AdapterGradReducer
        from avmoe_amd.train import FlatAdam
        kw, groups = COMBOS[name]
        kw = dict(kw)
        if "lr_schedule" in kw:
            kw["lr_schedule"] = _sched(**kw["lr_schedule"])
        self.name, self.dev = name, dev
        self.params = [torch.nn.Parameter(v.detach().clone().to(dev)) for v in param_values]
        self.buffers = [b.detach().clone().to(dev) for b in buffer_tensors]
        if "bufs" in name:
            kw["ema_buffers"] = [(f"bn.{i}", b) for i, b in enumerate(self.buffers)]
        red = AdapterGradReducer(self.params, bucket_mb=BUCKET_MB)
        assert len(red.buckets) == 2 and sorted(p.numel() for b in red.buckets for p in b.params) == sorted(SIZES)
        self.opt = FlatAdam(red, lr=1.0 if "prodigy" in name else LR, weight_decay=WD, grad_scale=GRAD_SCALE,
                            param_groups=groups(self.params), **kw)

    def set_grads(self, gs):
        with torch.no_grad():
            for p, g in zip(self.params, gs):
                p.grad.copy_(g)

    def step(self, step):
        with torch.no_grad():
            for b, v in zip(self.buffers, buffer_values(step)):
                b.copy_(v)
        if "sam" in self.name:                              # the first gradient of the step is always finite
            self.set_grads(gradients(self.name, step + SAM_OFFSET))
            self.opt.sam_perturb()
        gs = gradients(self.name, step)
        if "skip" in self.name and step == INF_STEP:
            gs[INF_PARAM].view(-1)[SIZES[INF_PARAM] // 2] = float("inf")
        self.set_grads(gs)
        self.opt.step()

    def digests(self):
        """-> {"arrays": {name: sha256}, "state": 128 hex digits, None on the plain path}"""
        opt, name = self.opt, self.name
        arrays = {f"bucket{i}.{k}": digest(s[k]) for i, s in enumerate(opt.state) for k in ("p", "m", "v", "e", "x0", "s") if k in s}
        if "prodigy" in name:
            blk = opt.prodigy_block
            arrays.update({f"prodigy_block.{k}": digest(blk[k]) for k in sorted(blk)})
        if "bufs" in name:
            arrays.update({f"buffer_shadow{i}": digest(v) for i, v in enumerate(opt.ema_buffers)})
        if "report" in name:
            arrays["param_grad_norms"], arrays["first_nonfinite_param"] = digest(opt.last_param_grad_norms), digest(opt.first_nonfinite_param)
        if "lamb" in name:
            arrays["trust_ratios"] = digest(opt.last_trust_ratios)
        if "muon" in name:
            arrays["muon_norms"] = digest(opt.last_muon_norms)
        if "sam" in name:
            arrays["sam_norm"], arrays["sam_scale"] = digest(opt.last_sam_norm), digest(opt.last_sam_scale)
        state = None
        if not name.startswith("plain"):                    # the device path: the state block is the first 64 bytes under its views
            first = opt.state_block["total_norm"]
            block = torch.empty(0, dtype=torch.uint8, device=self.dev).set_(first.untyped_storage(), first.storage_offset() * 4, (64,))
            state = block.cpu().numpy().tobytes().hex()
            applied = STEPS - 1 if "skip" in name else STEPS
            assert int(opt.applied_steps.item()) == applied and int(opt.skipped_steps.item()) == STEPS - applied
            assert "sam" not in name or not opt.perturbed
        return {"arrays": arrays, "state": state}


def run(name, dev):
    """-> {"state_dict": sha256 of the dict after step 2, "run": digests after step 4, "resumed": those of the optimizer that loaded it};
    with Prodigy also "prodigy_d": [d0, the saved d, d after step 4] as floats"""
    a = Side(name, dev, [0.25 * v for v in values(-1)], buffer_values(0))
    for step in range(1, SAVE_STEP + 1):
        a.step(step)
    sd = a.opt.state_dict()
    b = Side(name, dev, [p.data for p in a.params], a.buffers)
    b.opt.load_state_dict(sd)
    for step in range(SAVE_STEP + 1, STEPS + 1):
        a.step(step)
        b.step(step)
    out = {"state_dict": digest_state_dict(sd), "run": a.digests(), "resumed": b.digests()}
    if "prodigy" in name:
        out["prodigy_d"] = [a.opt.prodigy_d0, float(sd["flat_adam"]["prodigy_d"]), float(a.opt.prodigy_d.item())]
    return out


def golden():
    global _golden
    if _golden is None:
        with open(FIXTURE) as fh:
            _golden = json.load(fh)
    return _golden


def _assert_digests_equal(got, want, what):
    assert set(got["arrays"]) == set(want["arrays"]), (what, sorted(got["arrays"]), sorted(want["arrays"]))
    for array, sha in got["arrays"].items():
        assert sha == want["arrays"][array], f"{what}: {array} differs"
    assert got["state"] == want["state"], f"{what}: the state block differs: {got['state']} != {want['state']}"


@pytest.mark.parametrize("name", list(COMBOS))
def test_option_combination_is_bit_equal_to_the_recorded_library(name):
    want = golden()["combinations"].get(name)
    assert want is not None, f"the fixture has no combination {name!r} (left out: {golden()['left_out'].get(name)})"
    got = run(name, torch.device("cuda:0"))
    _assert_digests_equal(got["resumed"], got["run"], f"{name}: the resumed optimizer against the one that went on")
    _assert_digests_equal(got["run"], want["run"], f"{name}: against the recorded bytes")
    _assert_digests_equal(got["resumed"], want["resumed"], f"{name}: the resumed optimizer against the recorded bytes")
    assert got["state_dict"] == want["state_dict"], f"{name}: state_dict() after step {SAVE_STEP} differs from the recorded one"
    assert got.get("prodigy_d") == want.get("prodigy_d"), name


def test_the_fixture_holds_exactly_the_named_combinations():
    g = golden()
    assert g["commit"] and g["hipcc"] and g["recordings"] == 2
    assert sorted(list(g["combinations"]) + list(g["left_out"])) == sorted(COMBOS)
    assert len(g["left_out"]) <= 2 and not any(n in g["left_out"] for n in SINGLE_OPTION + ("plain+two_groups",))
    for name, c in g["combinations"].items():
        assert (c["run"]["state"] is None) == name.startswith("plain") and c["run"]["state"] == c["resumed"]["state"]
        assert c["run"]["arrays"] == c["resumed"]["arrays"], name
        want = {"p", "m", "v"} | ({"e"} if ("ema" in name or "swa" in name) else set()) | ({"x0", "s"} if "prodigy" in name else set())
        assert {k.split(".")[1] for k in c["run"]["arrays"] if k.startswith("bucket")} == want, name
        if "prodigy" in name:                               # the estimate did grow: the finalize rule's d_max / growth branch is pinned,
            d0, d_saved, d_last = c["prodigy_d"]            # and (but where the warm-up holds step 1 back) the resume restores a grown d
            assert d_last > d_saved >= d0 and (d_saved > d0 or "sched" in name), (name, c["prodigy_d"])
            assert c["run"]["arrays"]["prodigy_block.d"] != c["run"]["arrays"]["prodigy_block.d_max"] or "growth" not in name, name


def main(argv):
    import argparse
    import subprocess
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--record", required=True, metavar="PATH")
    ap.add_argument("--commit", required=True, help="the commit of the tree that is recorded")
    a = ap.parse_args(argv)
    import avmoe_amd
    hipcc = subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--version"], stdout=subprocess.PIPE, text=True, check=True).stdout
    dev = torch.device("cuda:0")
    out = {"commit": a.commit, "hipcc": hipcc.strip().splitlines(), "recordings": 1, "left_out": {},
           "combinations": {name: run(name, dev) for name in COMBOS}}
    with open(a.record, "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(f"recorded {len(COMBOS)} combinations of {avmoe_amd.__file__} into {a.record}")


if __name__ == "__main__":
    main(sys.argv[1:])
