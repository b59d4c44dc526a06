"""Every instantiation of FlatAdam's device kernels (kk_opt_finalize<SCHED, EMA>, kk_opt_adam<DECOUPLED, SCHED, EMA>; csrc/opt_kernels.hip)
held to bit-equality with the library as it was before the kernels were folded into one body each.

The model is the two-bucket model of tests/test_flat_adam_ema_gpu.py -- plain parameters of 1, 3, 4, 5, 1023, 1024, 1025 and 2049 elements,
the tail and block-boundary cases of the 1024-element block -- in two parameter groups with different rates, weight_decay 0.01 and
grad_scale 0.5.  All 32 combinations of max_grad_norm, skip_nonfinite, decoupled_weight_decay, lr_schedule and ema_decay take four steps;
the combination with everything off is the plain path (avmoe_adam_step).  Parameters and gradients come from a closed-form integer formula
of (step, element index), exact in fp32, so the fixture depends on no random generator.  With skip_nonfinite the third step carries one
inf and is skipped; without it every gradient is finite, so no NaN payload is ever compared.

tests/golden/flat_adam_flag_matrix.json holds, per combination, the SHA-256 of the raw bytes of each bucket's parameters, both moments and
(where on) averages after the last step, alignment padding included, and the 64-byte state block as hex.  It was recorded with this file's
main on the commit the fixture names:

    PYTHONPATH=<a built checkout of that commit> python tests/test_flat_adam_flag_matrix_gpu.py --record PATH --commit HASH

which uses FlatAdam's public interface only and so runs unchanged on that commit."""
import hashlib
import itertools
import json
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

SIZES = (1, 3, 4, 5, 1023, 1024, 1025, 2049)
SHAPES = {4: (2, 2), 1024: (32, 32)}
LR, LR_X, WD, GRAD_SCALE = 3e-3, 1e-2, 1e-2, 0.5
BUCKET_MB = 17200 / (1 << 20)                    # 4300 elements: 2049 + 1025 + 1024 (padded to 64s: 4224) fill the first bucket
STEPS, INF_STEP, INF_PARAM = 4, 3, 6
MAX_NORM = 1.0                                   # the scaled gradients' norm is above 50 at every step (asserted): every step clips
OPTIONS = ("clip", "skip", "adamw", "sched", "ema")
COMBOS = ["".join(c) for c in itertools.product("01", repeat=len(OPTIONS))]          # "10010": clip and sched on
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "flat_adam_flag_matrix.json")
_golden = None


def values(step):
    """one tensor per parameter: ((a k + b step) / 128 mod 2048 - 1024) / 256 over the running element index k, multiples of 2^-8 in [-4, 4)"""
    out, k0 = [], 0
    for n in SIZES:
        k = torch.arange(k0 + 1, k0 + n + 1, dtype=torch.int64)
        h = (k * 2654435761 + (step + 2) * 40503) // 128 % 2048 - 1024
        out.append((h.to(torch.float32) / 256.0).reshape(SHAPES.get(n, (n,))))
        k0 += n
    return out


def options(combo):
    from avmoe_amd.train import LRSchedule
    on = {name: bit == "1" for name, bit in zip(OPTIONS, combo)}
    kw = dict(lr=LR, weight_decay=WD, grad_scale=GRAD_SCALE)
    if on["clip"]:
        kw["max_grad_norm"] = MAX_NORM
    if on["skip"]:
        kw["skip_nonfinite"] = True
    if on["adamw"]:
        kw["decoupled_weight_decay"] = True
    if on["sched"]:
        kw["lr_schedule"] = LRSchedule(warmup_steps=2, decay_kind="cosine", total_steps=6)
    if on["ema"]:
        kw.update(ema_decay=0.9, ema_warmup=2.0)
    return on, kw


def digest(t):
    return hashlib.sha256(t.detach().contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()


def run(combo, dev):
    """-> {"arrays": {"bucket0.p": sha256, ...}, "state": 128 hex digits or None} after STEPS steps"""
    from avmoe_amd.dp import AdapterGradReducer
    from avmoe_amd.train import FlatAdam
    on, kw = options(combo)
    params = [torch.nn.Parameter((0.25 * v).to(dev)) for v in values(-1)]
    red = AdapterGradReducer(params, bucket_mb=BUCKET_MB)
    assert len(red.buckets) == 2 and sorted(p.numel() for b in red.buckets for p in b.params) == sorted(SIZES)
    opt = FlatAdam(red, param_groups=[{"params": params[:4], "lr": LR_X}], **kw)
    for step in range(1, STEPS + 1):
        gs = values(step)
        assert GRAD_SCALE * float(torch.cat([g.reshape(-1) for g in gs]).double().norm()) > 50.0 * MAX_NORM
        if on["skip"] and step == INF_STEP:
            gs[INF_PARAM].view(-1)[SIZES[INF_PARAM] // 2] = float("inf")
        with torch.no_grad():
            for p, g in zip(params, gs):
                p.grad.copy_(g)
        opt.step()
    arrays = {f"bucket{i}.{k}": digest(s[k]) for i, s in enumerate(opt.state) for k in "pmve" if k in s}
    state = None
    if any(on.values()):                                     # the device path: the state block is the first 64 bytes under its views
        first = opt.state_block["total_norm"]
        block = torch.empty(0, dtype=torch.uint8, device=dev).set_(first.untyped_storage(), first.storage_offset() * 4, (64,))
        state = block.cpu().numpy().tobytes().hex()
        applied = STEPS - 1 if on["skip"] else STEPS
        assert int(opt.applied_steps.item()) == applied and int(opt.skipped_steps.item()) == STEPS - applied
    return {"arrays": arrays, "state": state}


def golden():
    global _golden
    if _golden is None:
        with open(FIXTURE) as fh:
            _golden = json.load(fh)
    return _golden


@pytest.mark.parametrize("combo", COMBOS)
def test_flag_combination_is_bit_equal_to_the_recorded_library(combo):
    name = ", ".join(f"{o}={b}" for o, b in zip(OPTIONS, combo))
    want = golden()["combinations"].get(combo)
    assert want is not None, f"the fixture has no combination {combo} ({name})"
    got = run(combo, torch.device("cuda:0"))
    assert set(got["arrays"]) == set(want["arrays"]), (name, sorted(got["arrays"]), sorted(want["arrays"]))
    assert len(got["arrays"]) == 2 * (4 if combo[OPTIONS.index("ema")] == "1" else 3), name
    for array, sha in got["arrays"].items():
        assert sha == want["arrays"][array], f"{name}: {array} differs from the recorded bytes"
    assert got["state"] == want["state"], f"{name}: the state block differs: {got['state']} != {want['state']}"


def test_the_fixture_holds_exactly_the_32_combinations():
    g = golden()
    assert sorted(g["combinations"]) == sorted(COMBOS) and len(COMBOS) == 32
    assert g["commit"] and g["hipcc"]
    assert g["combinations"]["0" * len(OPTIONS)]["state"] is None        # the plain path has no state block
    assert all(len(c["state"]) == 128 for k, c in g["combinations"].items() if "1" in k)


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
    out = {"commit": a.commit, "hipcc": hipcc.strip().splitlines(), "options": list(OPTIONS), "combinations": {c: run(c, dev) for c in COMBOS}}
    with open(a.record, "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(f"recorded {len(COMBOS)} combinations of {avmoe_amd.__file__} into {a.record}")


if __name__ == "__main__":
    main(sys.argv[1:])
