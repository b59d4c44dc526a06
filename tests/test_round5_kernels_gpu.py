"""Round-5 kernels against the paths they replace, on shapes with ragged tiles and edge counts (bf16, C = Cy = 768, bottleneck 64 in 2 groups:
the shapes csrc/hop1_stream.hip and csrc/dx_stream3.hip are built for).  Both sides run bf16 operands with fp32 accumulation, so they
agree far more tightly than either agrees with the fp32 oracle: a wrong row of a ragged tile or a mis-counted wait shows up as an O(1)
error here where the bf16-vs-oracle budget (1e-2) could hide it.

  * hop-1 products against Y (R, V, dBm, dQ): streaming kernels (test hook avmoe_test_hooks lifts their size threshold) == tiled engine
  * token gradients: avmoe_moe_backward_dx_dy (one kernel per tensor) == dX overwriting + the other site's dY adding behind an event
"""
import pytest
import torch

from oracle import avmoe_oracle as O

pytestmark = pytest.mark.gpu

# (frames, tokens of X, tokens of Y, cross-modal experts, unimodal experts): token counts that are / are not multiples of the 32-token tiles,
# a frame shorter than one tile, one and two cross-modal experts (32 / 64 latent rows), a single frame
SHAPES = {
    "ragged_both": (12, 180, 76, 2, 2),
    "short_y_frame": (40, 100, 20, 2, 2),
    "one_cross_expert": (12, 196, 132, 1, 3),
    "three_cross_experts_engine": (6, 96, 64, 3, 1),       # 96 latent rows: beyond the streaming kernels, the engine keeps the site
    "single_frame": (1, 2304, 1024, 2, 2),
    "y_not_multiple_of_4": (10, 128, 50, 2, 2),            # kk_hop1_yk steps aside (M % 4), the token contractions do not
}


def _cfg(N, M, E_m, E_s):
    return O.AdapterConfig(Cx=768, Nx=N, Cy=768, Ny=M, reduction=12, groups=2, K=32, E_m=E_m, E_s=E_s, variant="ave")


def _run_site(cfg, S, seed):
    from tests.moe_gpu_util import MoeRun
    P, B = O.init_params(cfg, seed=seed)
    g = torch.Generator().manual_seed(seed + 100)
    X = 0.3 * torch.randn(S, cfg.Nx, cfg.Cx, generator=g)
    Y = 0.3 * torch.randn(S, cfg.Ny, cfg.Cy, generator=g)
    G = torch.randn(S, cfg.Nx, cfg.Cx, generator=g)
    run = MoeRun(cfg, P, B, X, Y, bf16=True, training=True).forward()
    got = run.backward(G)
    assert run.guards_intact(), "a kernel wrote past its workspace"
    return run.out.float().cpu(), run.idx.cpu(), {k: v.float().cpu() for k, v in got.items()}


@pytest.mark.parametrize("shape", list(SHAPES))
def test_hop1_streaming_kernels_equal_the_engine(shape, monkeypatch):
    S, N, M, E_m, E_s = SHAPES[shape]
    cfg = _cfg(N, M, E_m, E_s)
    from avmoe_amd import _capi
    with _capi.test_hooks(0):
        out_e, idx_e, g_e = _run_site(cfg, S, 3)                    # below the size threshold: the tiled engine
    with _capi.test_hooks(_capi.HOOK_HOP1S_FORCE):
        out_s, idx_s, g_s = _run_site(cfg, S, 3)                    # the streaming kernels wherever they serve the shape
    assert torch.equal(idx_e, idx_s)
    assert all(torch.isfinite(v).all() for v in g_s.values()) and torch.isfinite(out_s).all()
    # R / V are stored in bf16 by both paths but summed in another order: a last-bit difference there passes through two unscaled softmaxes
    # (measured: up to 2.5e-3 of the largest output on single elements, 1e-3 norm-wise); a wrong tile row would be O(1)
    assert float((out_s - out_e).abs().max()) <= 8e-3 * float(out_e.abs().max())
    assert float((out_s - out_e).norm() / out_e.norm()) <= 3e-3
    gmax = max(float(v.norm()) for v in g_e.values())
    for k, v in g_e.items():
        err = float((g_s[k] - v).norm()) / max(float(v.norm()), 1e-3 * gmax)
        # (summation order and one bf16 rounding of R / V / dBm / dQ apart; the tensors below 1 % of the largest norm -- fc.bias, the
        # gates, router.0: sums that cancel -- move by 1 - 3 % between ANY two bf16 evaluations, profiles/r05_bf16_tensor_table.txt)
        assert err <= (1e-2 if float(v.norm()) >= 1e-2 * gmax else 6e-2), (k, err)


# (frames, tokens of X, tokens of Y): ragged last tiles of a frame (the dZx / dL2 fragments are masked there), a frame shorter than one tile,
# more frames than blocks (130 > 128 per group: tile ranges that begin and end inside a frame, the leading parts through the slab)
TP2_SHAPES = {"ragged_180": (12, 180, 64), "ragged_196": (5, 196, 64), "short_frame_20": (40, 20, 64), "whole_tiles_128": (10, 128, 64),
              "frames_split_over_blocks": (130, 64, 32), "ragged_and_split": (131, 40, 32)}


@pytest.mark.parametrize("shape", list(TP2_SHAPES))
def test_token_contractions_streaming_equal_the_tiled_engine(shape, monkeypatch):
    """dWt = dZx^T X and dT[s] = dL2[s]^T X[s] (csrc/tok_pair2.hip, forced onto small sites) against gemm_tokpair: same bf16 operands, fp32
    accumulation in another order -- every parameter gradient within 1e-3 norm-wise (2 % for the tensors below 1 % of the largest)."""
    S, N, M = TP2_SHAPES[shape]
    cfg = _cfg(N, M, 2, 2)
    from avmoe_amd import _capi
    with _capi.test_hooks(0):
        out_e, idx_e, g_e = _run_site(cfg, S, 5)
    L = _capi.lib()
    L.avmoe_prof_reset(); L.avmoe_prof_enable(1)
    try:
        with _capi.test_hooks(_capi.HOOK_TOKPAIR2_FORCE):
            out_s, idx_s, g_s = _run_site(cfg, S, 5)
        ran = [f["name"] for f in _capi.prof_report()]
    finally:
        L.avmoe_prof_enable(0); L.avmoe_prof_reset()
    assert any(n.startswith("k_tok_pair2") for n in ran), ran      # (the hook did switch the kernel; with one frame per block the sums can even agree bit for bit)
    assert torch.equal(out_e, out_s) and torch.equal(idx_e, idx_s)          # (the forward does not change)
    gmax = max(float(v.norm()) for v in g_e.values())
    for k, v in g_e.items():
        assert torch.isfinite(g_s[k]).all(), k
        err = float((g_s[k] - v).norm()) / max(float(v.norm()), 1e-3 * gmax)
        assert err <= (1e-3 if float(v.norm()) >= 1e-2 * gmax else 2e-2), (k, err)


def _pair_step(ca, cv, S, fused, monkeypatch):
    import avmoe_amd.adapters as A
    from tests.test_adapters_api import build_module
    monkeypatch.setattr(A, "_FUSED_DX", fused)
    dev = torch.device("cuda:0")
    Pa, Ba = O.init_params(ca, seed=0)
    Pv, Bv = O.init_params(cv, seed=1)
    ma, mv = build_module("ave", ca).to(dev).train(), build_module("ave", cv).to(dev).train()
    ma.load_state_dict({**Pa, **Ba}); mv.load_state_dict({**Pv, **Bv})
    pair = A.AdapterPair(ma, mv, concurrent=True)
    g = torch.Generator().manual_seed(77)
    fa, fv = 0.3 * torch.randn(S, ca.Nx, ca.Cx, generator=g), 0.3 * torch.randn(S, cv.Nx, cv.Cx, generator=g)
    ga, gv = torch.randn(fa.shape, generator=g).bfloat16(), torch.randn(fv.shape, generator=g).bfloat16()
    xa = fa.to(dev, torch.bfloat16).requires_grad_(True)
    xv = fv.to(dev, torch.bfloat16).requires_grad_(True)
    out_a, _ia, out_v, _iv = pair(xa.permute(0, 2, 1).unsqueeze(-1), xv.permute(0, 2, 1).unsqueeze(-1))
    torch.autograd.backward([out_a, out_v], [ga.to(dev).permute(0, 2, 1).unsqueeze(-1), gv.to(dev).permute(0, 2, 1).unsqueeze(-1)])
    torch.cuda.synchronize()
    res = {"d_fa": xa.grad.float().cpu(), "d_fv": xv.grad.float().cpu()}
    for tag, m in (("a", ma), ("v", mv)):
        res.update({f"{tag}.{k}": p.grad.float().cpu() for k, p in m.named_parameters()})
    return res


@pytest.mark.parametrize("shape", ["ragged_both", "short_y_frame", "one_cross_expert", "single_frame"])
def test_token_gradient_written_once_equals_the_two_kernel_handover(shape, monkeypatch):
    """AdapterPair two-stream step: dT = dX_A + dY_B from avmoe_moe_backward_dx_dy against dX overwriting and dY adding.  The parameter
    gradients do not pass through either and must be bit-identical; the token gradients differ by one bf16 rounding of the sum."""
    S, N, M, E_m, E_s = SHAPES[shape]
    S = max(S, -(-2048 // min(N, M)))                               # the fused kernel wants >= 2048 tokens per tensor
    ca, cv = _cfg(N, M, E_m, E_s), _cfg(M, N, E_m, E_s)
    two = _pair_step(ca, cv, S, False, monkeypatch)
    one = _pair_step(ca, cv, S, True, monkeypatch)
    for k in two:
        assert torch.isfinite(one[k]).all(), k
        if k in ("d_fa", "d_fv"):
            # two kernels: bf16(bf16(dX) + dY) ; one kernel: bf16(dX + dY) -- within two bf16 roundings of each other, row by row
            ref = two[k]
            tol = 2.0 ** -7 * ref.abs().amax(-1, keepdim=True).clamp_min(1e-6)
            assert bool(((one[k] - ref).abs() <= tol).all()), (k, float(((one[k] - ref).abs() / tol).max()))
            assert float((one[k] - ref).norm() / ref.norm()) <= 4e-3, k
        else:
            assert torch.equal(one[k], two[k]), k


def test_form_chain_follows_the_hooks_inside_one_process():
    """One site, one set of workspaces, forward + backward twice: with every size threshold lifted (the streaming forms of the hop-1
    products and of the token contractions serve it), then with the hooks at 0 (every chain ends in the engine).  The forms a product goes
    through are chosen per call; the two runs agree within the bounds of test_hop1_streaming_kernels_equal_the_engine above."""
    from avmoe_amd import _capi
    from tests.moe_gpu_util import MoeRun
    S, N, M = TP2_SHAPES["ragged_196"]                     # the smallest site of this file that the streaming forms serve
    cfg = _cfg(N, M, 2, 2)
    P, B = O.init_params(cfg, seed=7)
    g = torch.Generator().manual_seed(107)
    X, Y, G = (0.3 * torch.randn(S, cfg.Nx, cfg.Cx, generator=g), 0.3 * torch.randn(S, cfg.Ny, cfg.Cy, generator=g),
               torch.randn(S, cfg.Nx, cfg.Cx, generator=g))
    run = MoeRun(cfg, P, B, X, Y, bf16=True, training=True)
    L = _capi.lib()

    def step(mask):
        L.avmoe_prof_reset(); L.avmoe_prof_enable(1)
        try:
            with _capi.test_hooks(mask):
                got = run.forward().backward(G)
            ran = {f["name"] for f in _capi.prof_report()}
        finally:
            L.avmoe_prof_enable(0); L.avmoe_prof_reset()
        assert run.guards_intact(), "a kernel wrote past its workspace"
        return run.out.float().cpu(), run.idx.cpu(), {k: v.float().cpu() for k, v in got.items()}, ran

    streamed = {"k_hop1_yk", "k_hop1_yt_frames", "k_hop1_yt_sum", "k_tok_pair2"}
    out_s, idx_s, g_s, ran_s = step(_capi.HOOK_ALL_FORCE)
    out_e, idx_e, g_e, ran_e = step(0)
    assert streamed <= ran_s, sorted(ran_s)
    assert not (streamed & ran_e), sorted(ran_e)
    assert torch.equal(idx_e, idx_s)
    assert all(torch.isfinite(v).all() for v in g_s.values()) and torch.isfinite(out_s).all()
    assert float((out_s - out_e).abs().max()) <= 8e-3 * float(out_e.abs().max())
    assert float((out_s - out_e).norm() / out_e.norm()) <= 3e-3
    gmax = max(float(v.norm()) for v in g_e.values())
    for k, v in g_e.items():
        err = float((g_s[k] - v).norm()) / max(float(v.norm()), 1e-3 * gmax)
        assert err <= (1e-2 if float(v.norm()) >= 1e-2 * gmax else 6e-2), (k, err)
