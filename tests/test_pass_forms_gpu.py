"""Which form of every bottleneck-space pass runs (csrc/pass.h: one form chain per pass -- kfs_* streamed, kf_* register-resident, kg_*
generalised, kt_* / kk_mid any shape), at the smallest shapes where the choice can go wrong.

The forms decide for themselves at launch, so the only outside view of the choice is the profiler: every pass opens one scope, named
"... (stream)" when its streamed form ran.  EXPECTED below is NOT derived from the code under test: it is the record of
tests/dev/pass_forms_record.py taken on commit 05f121e ("Streamed products: one form chain (try_forms), one switch table"), the last
commit whose k_* wrappers spelled the choice by hand (profiles/r15_pass_forms_record_parent.txt)."""
import hashlib

import pytest
import torch

from oracle import avmoe_oracle as O

pytestmark = pytest.mark.gpu

# scopes of the bottleneck-space passes (prefix match: AVMOE_PROF_SHAPES appends a token count), and the Gram pass that follows
# post_small_bwd unless its streamed form left dGq itself
PASS_SCOPES = ("k_pre_small", "k_mid", "k_post_small", "k_pre_bwd", "k_pre_lat_bwd", "k_gram64")


def _tuned(N, M, E_m, E_s, variant="ave"):          # tests/test_round6_kernels_gpu.py::_cfg
    return O.AdapterConfig(Cx=768, Nx=N, Cy=768, Ny=M, reduction=12, groups=2, K=32, E_m=E_m, E_s=E_s, variant=variant)


def _family(name):
    from tests.topk_families import family_config
    return family_config(name)


# case -> (config, frames, bf16, hook names)
CASES = {
    "short_frame_20": (lambda: (_tuned(20, 32, 2, 2), 40, True), ()),                       # 800 tokens: below the 2048-token line
    "short_frame_20_force": (lambda: (_tuned(20, 32, 2, 2), 40, True), ("HOOK_KFS_FORCE",)),
    "ragged_196": (lambda: (_tuned(196, 64, 2, 2), 20, True), ()),                          # 3920 tokens: streamed without a hook
    "ragged_196_off": (lambda: (_tuned(196, 64, 2, 2), 20, True), ("HOOK_KFS_OFF",)),
    "three_experts_force": (lambda: (_tuned(180, 64, 1, 2), 16, True), ("HOOK_KFS_FORCE",)),    # no gram64: post_small_bwd steps aside
    "one_frame_force": (lambda: (_tuned(256, 64, 2, 2), 1, True), ("HOOK_KFS_FORCE",)),     # no fused hop-2 logits: pre_small steps aside
    "avvp_force": (lambda: (_tuned(64, 32, 2, 2, "avvp"), 8, True), ("HOOK_KFS_FORCE",)),   # N x N experts: pre_small / pre_bwd step aside
    "tile_fast_f32": (lambda: _family("tile_fast"), ()),
    "tile_fast_f32_force": (lambda: _family("tile_fast"), ("HOOK_KFS_FORCE",)),             # fp32 never streams
    "tile_gen": (lambda: _family("tile_gen"), ()),
    "tile_kernels": (lambda: _family("tile_kernels"), ()),
}

# name -> calls of one forward + backward, recorded on commit 05f121e (see the module docstring)
EXPECTED = {
    "short_frame_20": {"k_gram64": 2, "k_mid_bwd": 1, "k_post_small": 1, "k_post_small_bwd": 1, "k_pre_bwd_finalize": 1, "k_pre_lat_bwd": 1, "k_pre_small": 1, "k_pre_small_bwd": 1},
    "short_frame_20_force": {"k_gram64": 1, "k_mid_bwd (stream)": 1, "k_post_small (stream)": 1, "k_post_small_bwd (stream)": 1, "k_pre_bwd (stream)": 1, "k_pre_bwd_finalize": 1, "k_pre_small": 1},
    "ragged_196": {"k_gram64": 1, "k_mid_bwd (stream)": 1, "k_post_small (stream)": 1, "k_post_small_bwd (stream)": 1, "k_pre_bwd (stream)": 1, "k_pre_bwd_finalize": 1, "k_pre_small (stream)": 1},
    "ragged_196_off": {"k_gram64": 2, "k_mid_bwd": 1, "k_post_small": 1, "k_post_small_bwd": 1, "k_pre_bwd_finalize": 1, "k_pre_lat_bwd": 1, "k_pre_small": 1, "k_pre_small_bwd": 1},
    "three_experts_force": {"k_mid": 1, "k_mid_bwd (stream)": 1, "k_post_small (stream)": 1, "k_post_small_bwd": 1, "k_pre_bwd (stream)": 1, "k_pre_bwd_finalize": 1, "k_pre_small": 1},
    "one_frame_force": {"k_gram64": 1, "k_mid_bwd (stream)": 1, "k_post_small (stream)": 1, "k_post_small_bwd (stream)": 1, "k_pre_bwd (stream)": 1, "k_pre_bwd_finalize": 1, "k_pre_small": 1},
    "avvp_force": {"k_gram64": 1, "k_mid_bwd (stream)": 1, "k_post_small (stream)": 1, "k_post_small_bwd (stream)": 1, "k_pre_bwd_finalize": 1, "k_pre_lat_bwd": 1, "k_pre_small": 1, "k_pre_small_bwd": 1},
    "tile_fast_f32": {"k_mid": 1, "k_mid_bwd": 1, "k_post_small": 1, "k_post_small_bwd": 1, "k_pre_bwd_finalize": 1, "k_pre_lat_bwd": 1, "k_pre_small": 1, "k_pre_small_bwd": 1},
    "tile_fast_f32_force": {"k_mid": 1, "k_mid_bwd": 1, "k_post_small": 1, "k_post_small_bwd": 1, "k_pre_bwd_finalize": 1, "k_pre_lat_bwd": 1, "k_pre_small": 1, "k_pre_small_bwd": 1},
    "tile_gen": {"k_mid": 1, "k_mid_bwd": 1, "k_post_small": 1, "k_post_small_bwd": 1, "k_pre_small": 1, "k_pre_small_bwd": 1},
    "tile_kernels": {"k_mid": 1, "k_mid_bwd": 1, "k_post_small": 1, "k_post_small_bwd": 1, "k_pre_small": 1, "k_pre_small_bwd": 1},
}


def run_case(name, seed=11):
    """One forward + backward of the case with the profiler on: ({scope name: (calls, algorithmic bytes)}, guards intact,
    {tensor name: CPU tensor})."""
    from tests.moe_gpu_util import MoeRun
    from avmoe_amd import _capi
    make, hooks = CASES[name]
    cfg, S, bf16 = make()
    P, B = O.init_params(cfg, seed=seed)
    g = torch.Generator().manual_seed(seed + 100)
    X = 0.3 * torch.randn(S, cfg.Nx, cfg.Cx, generator=g)
    Y = 0.3 * torch.randn(S, cfg.Ny, cfg.Cy, generator=g)
    G = torch.randn(S, cfg.Nx, cfg.Cx, generator=g)
    mask = 0
    for h in hooks:
        mask |= getattr(_capi, h)
    L = _capi.lib()
    with _capi.test_hooks(mask):
        L.avmoe_prof_reset(); L.avmoe_prof_enable(1)
        try:
            run = MoeRun(cfg, P, B, X, Y, bf16=bf16, training=True).forward()
            grads = run.backward(G)
            torch.cuda.synchronize()
            ran = {f["name"]: (f["calls"], f["alg_bytes"]) for f in _capi.prof_report()}
        finally:
            L.avmoe_prof_enable(0); L.avmoe_prof_reset()
    tensors = {"out": run.out.cpu(), "probs": run.probs.cpu(), "idx": run.idx.cpu()}
    tensors.update({"d " + k: v for k, v in grads.items()})
    return ran, run.guards_intact(), tensors


def pass_scopes(ran):
    """{scope name: calls} of the bottleneck-space passes"""
    return {n: c for n, (c, _b) in ran.items() if n.startswith(PASS_SCOPES)}


def digest(t):
    return hashlib.sha256(t.contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()


@pytest.mark.parametrize("case", list(CASES))
def test_each_pass_runs_the_form_the_parent_ran(case):
    ran, guards, tensors = run_case(case)
    print(case, sorted(pass_scopes(ran).items()))
    assert pass_scopes(ran) == EXPECTED[case], sorted(ran)
    assert guards, "a kernel wrote past its workspace"
    for k, v in tensors.items():
        if v.is_floating_point():
            assert torch.isfinite(v).all(), k
