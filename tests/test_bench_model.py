"""bench.py's work model on the CPU (no GPU, no kernels): the per-clip-pair byte / FLOP figures are SURVEY 8(d)'s, every
configuration BASELINE.json names is defined, and a bare `--gpus N` builds the launcher command the driver would use."""
import sys
import types

import pytest

import bench


def test_cfg2_work_model_matches_survey_8d():
    c = bench.CONFIGS["cfg2"]
    assert bench.algorithmic_bytes_per_clip_pair(c, 2) == pytest.approx(93.7e6, rel=2e-3)          # 93.7 MB per clip-pair
    assert bench.reference_flops_per_clip_pair(c) == pytest.approx(90.70e9, rel=2e-3)              # 90.70 GFLOP fwd+bwd
    assert bench.algorithmic_bytes_per_clip_pair(c, 2) * c["B"] == pytest.approx(3.00e9, rel=2e-3)


def test_every_baseline_configuration_is_defined():
    assert set(bench.CONFIGS) == {"cfg1", "cfg2", "cfg3", "cfg4", "cfg5"}
    c1 = bench.CONFIGS["cfg1"]
    assert sum(p[4] for p in c1["pairs"]) == 24 and c1["dtype"] == "f32" and c1["B"] == 2            # 12 block pairs x {p1, p2}
    assert (96, 4096, 128, 2304, 4) in c1["pairs"] and (768, 64, 1024, 36, 4) in c1["pairs"]
    c4 = bench.CONFIGS["cfg4"]
    assert (c4["E_m"], c4["E_s"], c4["K"], c4["groups"]) == (1, 2, 2, 4)
    assert bench.CONFIGS["cfg5"]["K"] == 87 and bench.CONFIGS["cfg3"]["variant"] == "avvp"


def test_self_launch_builds_the_torchrun_command(monkeypatch):
    seen = {}

    def fake_run(cmd, env=None):
        seen["cmd"], seen["env"] = cmd, env
        return types.SimpleNamespace(returncode=0)
    monkeypatch.setattr(bench.subprocess, "run", fake_run)
    with pytest.raises(SystemExit) as e:
        bench.self_launch(types.SimpleNamespace(gpus=4), ["--gpus", "4", "--steps", "3"])
    assert e.value.code == 0
    cmd = seen["cmd"]
    assert cmd[:3] == [sys.executable, "-m", "torch.distributed.run"] and "--nproc-per-node=4" in cmd and "127.0.0.1" in cmd
    assert cmd[-4:] == ["--gpus", "4", "--steps", "3"] and seen["env"]["HSA_ENABLE_IPC_MODE_LEGACY"] == "0"


def test_parity_verdict_of_the_bf16_gradient_views():
    """bench.parity_verdict: `ok` is about the hard bars (fp32 1e-3, bf16 output, indices); `ok_bf16_grads` is `no tensor above 5 % AND above the
    eager-autocast error` (vectors on the one draw, single sums over several draws of the upstream gradient) where that list was measured, and falls
    back to the single-draw criterion of rounds 2 - 5 -- which stays on the line under its own name -- where it was not."""
    import bench
    base = dict(idx_equal=True, out_rel_f32=2e-6, grad_rel_f32=1e-4, out_rel_bf16=5e-3, grad_relnorm_bf16_same_mask=0.08, grad_relnorm_bf16_major=0.01,
                grad_relnorm_bf16_tiny_joint=0.01, grad_relnorm_bf16_rest=0.01, grad_abs_bf16_structural_zero=1e-4)
    r = bench.parity_verdict(dict(base, bf16_tensors_above_5pct_and_eager=[]))
    assert r["ok"] and r["ok_bf16_grads"] is True and r["ok_bf16_grads_single_draw"] is False and r["ok_bf16_grads_as_tested"] is True
    r = bench.parity_verdict(dict(base, bf16_tensors_above_5pct_and_eager=["router.0.weight (v) 0.064 (eager 0.059)"]))
    assert r["ok"] and r["ok_bf16_grads"] is False
    r = bench.parity_verdict(dict(base))                                  # the multi-draw view not measured: the single-draw criterion decides
    assert r["ok_bf16_grads"] is False
    r = bench.parity_verdict(dict(base, grad_relnorm_bf16_same_mask=0.03))
    assert r["ok_bf16_grads"] is True and r["ok_bf16_grads_single_draw"] is True
    r = bench.parity_verdict(dict(base, grad_rel_f32=2e-3, bf16_tensors_above_5pct_and_eager=[]))      # a hard bar
    assert not r["ok"] and "grad_rel_f32" in r["failed"]
    r = bench.parity_verdict(dict(idx_equal=True, out_rel_f32=2e-6, grad_rel_f32=1e-4))                # an fp32 configuration: no bf16 leg
    assert r["ok"] and r["ok_bf16_grads"] is None


def test_dump_outputs_whole_or_seeded_sample_within_the_budget(tmp_path):
    """bench.dump_outputs (--dump-outputs): float32 .npy files under the byte budget; arrays that fit are written whole in their own shape,
    the larger ones as the same seeded positions every time, taken in the tensor's logical order (a permuted view is sampled as its values)."""
    import numpy as np
    import torch
    big = torch.arange(6 * 500 * 40, dtype=torch.float32).reshape(6, 500, 40)
    view = big.permute(0, 2, 1).unsqueeze(-1)                                   # the (S, C, N, 1) view a site returns
    arrays = [("pair0_0_out_a", view), ("pair0_0_idx_a", torch.tensor([[1], [3]])), ("pair0_0_lb_a", torch.tensor(0.25, dtype=torch.bfloat16))]
    budget = 4 * 30_000
    n, nbytes = bench.dump_outputs(str(tmp_path / "a"), arrays, budget=budget)
    assert n == 3 and nbytes <= budget
    assert sum(f.stat().st_size for f in (tmp_path / "a").iterdir()) == nbytes
    out = np.load(tmp_path / "a" / "pair0_0_out_a.npy")
    idx = np.load(tmp_path / "a" / "pair0_0_idx_a.npy")
    lb = np.load(tmp_path / "a" / "pair0_0_lb_a.npy")
    assert out.dtype == idx.dtype == lb.dtype == np.float32
    assert idx.shape == (2, 1) and idx.ravel().tolist() == [1.0, 3.0] and lb.shape == () and float(lb) == 0.25
    assert out.ndim == 1 and 20_000 < out.size < view.numel()
    where = np.argsort(view.reshape(-1).numpy())[out.astype(np.int64)]         # logical position of every sampled (distinct) value
    assert np.all(np.diff(where) >= 0) and where[0] < view.numel() // 100 and where[-1] > view.numel() * 99 // 100
    bench.dump_outputs(str(tmp_path / "b"), arrays, budget=budget)
    assert np.array_equal(out, np.load(tmp_path / "b" / "pair0_0_out_a.npy"))                # same positions run to run
    n, nbytes = bench.dump_outputs(str(tmp_path / "c"), arrays)                              # the default budget: everything whole
    whole = np.load(tmp_path / "c" / "pair0_0_out_a.npy")
    assert whole.shape == (6, 40, 500, 1) and np.array_equal(whole, view.numpy()) and nbytes <= bench.DUMP_BYTES <= 64 << 20


def test_a_plain_run_is_the_headline_alone():
    """bench.parse_args: without --full one repetition of the K steps (the headline's own) and no other leg; --full brings back the three
    repetitions and every leg the --no-* options do not leave out; an explicit --reps holds either way."""
    a = bench.parse_args(["--gpus", "1", "--steps", "20", "--warmup", "5"])
    assert not a.full and a.reps == 1 and (a.steps, a.warmup, a.gpus) == (20, 5, 1)
    a = bench.parse_args(["--gpus", "1", "--steps", "20", "--warmup", "5", "--full"])
    assert a.full and a.reps == 3 and not (a.no_cpu_baseline or a.no_roofline or a.no_f32 or a.no_other_configs)
    assert bench.parse_args(["--reps", "2"]).reps == 2 and bench.parse_args(["--full", "--reps", "1"]).reps == 1
