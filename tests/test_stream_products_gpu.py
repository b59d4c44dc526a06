"""Every bf16 streaming product of one adapter site (the benchmarked shape: C = Cy = 768 in 2 groups, bottleneck 64, K = 32, four experts)
recomputed in fp64 from the operands EXACTLY AS THE KERNEL READ THEM and compared element by element with a derived bound
(tests/stream_product_ref.py; tests/test_stream_product_checker.py shows what such a check catches).

The workspace names every intermediate (avmoe_moe_buffer_info), no two named buffers share memory (moe_plan.cpp::make_plan gives each its own
offset) and avmoe_moe_backward_part stops the backward at its section boundaries: the test runs the forward, then sections 1, 32, 64, 8, 16, and
reads operands and results back after each.  Both operands are read as stored (bf16 and fp32 are exact in fp64), so nothing upstream adds error:
the bound is ~2^-8 per ELEMENT where the end-to-end tests allow 1e-2 per TENSOR -- one wrong row of a ragged tile, one dropped token, one frame
boundary off by one shows.  The profiler is on and each product is only counted when the kernel family it is meant to exercise ran
(asserted by name); where a shape legitimately steps aside (documented launcher conditions) the test asserts that it did.

Survival of operands and results to the section boundary (moe_forward.cpp / moe_backward.cpp; every reader below takes them as const):
  F1 sx, rin[:, :C]   written by k_xstats_fin, read by pre_small / the router.                      F2 L2: written once by kfs_pre_small (lg[] = sum of
  the group partials L2g, tile_stream.hip:913,989).     F4 Rext[:, :Kcy, :M], F5 V, F6 out: written once.
  F3  Z holds Zx only until kfs_pre_small overwrites it IN PLACE with z: checked through z's defining map (below), with the map's roundings named.
  B1  dAp / dApx / dBp: read-only for post_small_bwd (tile_stream.hip:451,1530) and post_prep_bwd (weight_kernels.hip:376).
  B2  dWt, dT after section 32 hold MORE than tok_pair2's product: dWt += dTW^T Text (moe_backward.cpp:287), dT += dTW Wt (:313) + 2 dTT T (:329);
      all of those operands are stored too (dTW, dTT in bf16), so the reference is the whole sum.  k_finish_dT and k_down_bwd read them as const.
  B3  Zw (= dZx), dL2x, rs2x are last written by pre_small_bwd in section 1; section 32 only reads them (asserted: snapshots compared).
  B4  dV, dRT, dBm: dBm is read-only for k_prep_dBm (bwd_kernels.hip:911); the streaming dQ is stored in bf16 as dQT (moe_backward.cpp:412).
  B5 / B6  dY / dT are outputs of the call.

On the row scale of B3 / B6: dx_stream2.hip:170 and dx_stream3.hip:351 take rs2x as an fp32 scalar (`a + rs * x` in fp32), NOT as bf16 planes --
no 2^-16 term there, two more fp32 roundings instead.  The two-plane form occurs in F3's latent term (tile_stream.hip:794 mm_lds_finish).
"""
import ctypes as C

import pytest
import torch

from oracle import avmoe_oracle as O
from tests.stream_product_ref import check_bound, check_product, check_untouched, product_bound, product_ref, EPS_BF16

pytestmark = pytest.mark.gpu

PRODUCTS = {
    "F1": "gemm_stream k384_n128 + stats: sx, rin[:, :C] from X",
    "F2": "... + x64: L2 from X, Text",
    "F3": "... main product: z through its defining map from X Wt^T",
    "F4": "kk_hop1_yk: Rext[..., :M] from Qx, Y",
    "F5": "kk_hop1_yt<frames>: V from BmX, Y",
    "F6": "gemm_stream k160_n384: out from Apost, Bpost",
    "B1": "k_dpost_pair + reduce: dAp (+ dApx), dBp from dOut, Bpost, Apost",
    "B2": "k_tok_pair2 (+ finish): dWt, dT from Zw, dL2x, X",
    "B3": "k_dx_stream2: dX",
    "B4": "kk_hop1_yk, kk_hop1_yt<sum> + kk_hop1_sum: dBm, dQ from dV, dRT, Y",
    "B5": "gemm_stream k64+96mn_*: dY from dRT, Qx, BmX, dV",
    "B6": "k_dx_stream3: dT = dX_A + dY_B",
}
RAGGED = {"ragged_196_76", "ragged_180_one_cross", "short_frame_20", "pair_ragged_180_76", "pair_short_20"}
CHECKED = {}      # product -> {shape: (kernel family seen, worst err / bound)}

# (frames, N, M, E_m, E_s).  k_dpost_pair wants >= 4096 tokens in whole 64-token tiles even when forced: the frame counts make S * N such a number.
SHAPES = {
    "ragged_196_76": (32, 196, 76, 2, 2),              # ragged on both sides
    "ragged_180_one_cross": (32, 180, 76, 1, 3),       # one cross-modal expert: 32 latent rows
    "short_frame_20": (208, 20, 64, 2, 2),             # a frame shorter than one 32-token tile
    "whole_tiles": (16, 256, 64, 2, 2),
    "many_frames_64": (132, 64, 32, 2, 2),             # more frames than blocks per group: tile ranges begin and end inside a frame, slab paths
    "one_long_frame": (1, 2304, 1024, 2, 2),
}
PAIR_SHAPES = {"pair_ragged_180_76": (12, 180, 76, 2, 2), "pair_short_20": (128, 20, 64, 2, 2), "pair_whole": (8, 256, 64, 2, 2),
               "pair_one_cross": (12, 196, 132, 1, 3)}


def _cfg(N, M, E_m, E_s):
    return O.AdapterConfig(Cx=768, Nx=N, Cy=768, Ny=M, reduction=12, groups=2, K=32, E_m=E_m, E_s=E_s, variant="ave")


def draw_inputs(cfg, S, seed, X=None, Y=None):
    """X, Y and dOut of a site, drawn from the seed on the CPU (a given X or Y is kept and not drawn)"""
    g = torch.Generator().manual_seed(seed + 100)
    X = 0.3 * torch.randn(S, cfg.Nx, cfg.Cx, generator=g) if X is None else X
    Y = 0.3 * torch.randn(S, cfg.Ny, cfg.Cy, generator=g) if Y is None else Y
    return X, Y, torch.randn(S, cfg.Nx, cfg.Cx, generator=g)


class Site:
    """One site on cuda:0 (bf16 and training mode unless told otherwise) with its workspaces (tests/moe_gpu_util.py::MoeRun: NaN-poisoned,
    guard bands), the backward in sections, and every named buffer as a device view.  self.B: the BatchNorm buffers as uploaded."""

    def __init__(self, cfg, S, seed, X=None, Y=None, training=True):
        self.make_run(cfg, S, seed, X, Y, training=training)
        r = self.run
        self.E, self.g, self.Cg, self.N, self.M, self.Cc, self.Cy = cfg.E, cfg.groups, cfg.Cx // cfg.groups, cfg.Nx, cfg.Ny, cfg.Cx, cfg.Cy
        self.NT = S * self.N
        E, g = self.E, self.g
        self.dgp = r.table["wsum"][2] // 4 // (E * g)
        self.El = cfg.E_m
        self.Kp = 32
        self.KL = self.El * self.Kp
        self.KLT = self.KL + 2
        self.KLp = -(-self.KLT // 8) * 8
        self.Kcy, self.Kcyb, self.Kcyp = self.KL, self.KL + 1, -(-max(self.KL, 1) // 8) * 8
        self.KP = E * self.dgp + 3 * E
        self.KPp = -(-self.KP // 8) * 8
        self.XW = -(-(self.KPp - E * self.dgp) // 16) * 16
        self.Mk, self.Mb = -(-(self.M + 2) // 8) * 8, -(-(self.M + 1) // 8) * 8
        assert self.dgp == 32 and r.table["Text"][2] == S * self.KLT * self.Cc * 2 and r.table["Z"][2] == self.NT * E * g * self.dgp * 2       # (the tuned layout)

    def make_run(self, cfg, S, seed, X=None, Y=None, training=True, bf16=True, counters=False):
        """parameters, buffers and inputs from the seed, and the MoeRun: the part of a site that no layout enters (the subclasses for
        other layouts and element types start here).  counters: upload num_batches_tracked too"""
        from tests.moe_gpu_util import MoeRun
        P, B = O.init_params(cfg, seed=seed)
        X, Y, self.G = draw_inputs(cfg, S, seed, X, Y)
        self.P, self.B, self.cfg, self.S, self.training, self.bf16 = P, B, cfg, S, training, bf16
        self.T = torch.bfloat16 if bf16 else torch.float32
        self.run = MoeRun(cfg, P, B, X, Y, bf16=bf16, training=training, counters=counters)

    def dev(self, name, dtype, shape):
        region, off, nbytes = self.run.table[name]
        raw = (self.run.saved if region == 0 else self.run.scratch)[off:off + nbytes]
        n = 1
        for k in shape:
            n *= k
        return raw.view(dtype)[:n].reshape(shape)

    def bf(self, name, shape):
        return self.dev(name, torch.bfloat16, shape)

    def f32(self, name, shape):
        return self.dev(name, torch.float32, shape)

    def begin_backward(self):
        r = self.run
        from avmoe_amd import _capi_moe as cm
        r.dOut = self.G.to(r.dev, r.tdt).contiguous()
        r.dX = torch.full_like(r.X, float("nan"))
        r.dY = torch.full_like(r.Y, float("nan"))
        r.grads = {k: torch.full_like(v, float("nan")) for k, v in r.params.items()}
        r.gptrs = cm.make_ptrs(r.grads, self.cfg.E_m, self.cfg.E_s)
        r.lbw = torch.zeros(1, device=r.dev, dtype=torch.float32)

    def part(self, parts):
        from avmoe_amd import _capi as capi
        r = self.run
        st = r.L.avmoe_moe_backward_part(C.byref(r.desc), r.X.data_ptr(), r.Y.data_ptr(), C.byref(r.ptrs), r.dOut.data_ptr(), r.lbw.data_ptr(),
                                         r.saved.data_ptr(), r.scratch.data_ptr(), r.dX.data_ptr(), r.dY.data_ptr(), C.byref(r.gptrs), int(parts),
                                         torch.cuda.current_stream().cuda_stream)
        capi.check(st, f"avmoe_moe_backward_part({parts})")
        torch.cuda.synchronize()


@pytest.fixture(autouse=True)
def _release_device_memory():
    """The sites here hold workspaces of up to a few hundred MB, NaN-poisoned: hand them back to the device after every test, so that the
    modules that run after this one allocate as they did before it existed."""
    yield
    import gc
    gc.collect()
    if torch.cuda.is_available():
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


class Profiled:
    def __enter__(self):
        from avmoe_amd import _capi
        self.capi, self.L = _capi, _capi.lib()
        self.hooks = _capi.test_hooks(_capi.HOOK_ALL_FORCE)
        self.hooks.__enter__()
        self.L.avmoe_prof_reset(); self.L.avmoe_prof_enable(1)
        return self

    def names(self):
        """the kernel families launched since the last call"""
        torch.cuda.synchronize()
        ran = {f["name"] for f in self.capi.prof_report()}
        self.L.avmoe_prof_reset()
        return ran

    def __exit__(self, *exc):
        self.L.avmoe_prof_enable(0); self.L.avmoe_prof_reset()
        self.hooks.__exit__(*exc)
        return False


class Recorder:
    """Collects the failures of one shape (every product is tried; the test fails at the end with all of them) and the margins."""

    def __init__(self, shape):
        self.shape, self.fail = shape, []

    def product(self, tag, kernel, fn):
        """fn() -> worst err / bound (raises AssertionError on a mismatch); counted for the coverage test under the kernel family seen"""
        try:
            ratio = fn()
        except AssertionError as e:
            self.fail.append(f"{tag} [{kernel}]: {e}")
            return
        prev = CHECKED.setdefault(tag, {}).get(self.shape)
        CHECKED[tag][self.shape] = (kernel, max(ratio, prev[1] if prev else 0.0))
        print(f"MARGIN {tag} {self.shape} {kernel} worst_err_over_bound {ratio:.4f}")

    def stepped_aside(self, tag, kernel, why):
        print(f"ASIDE  {tag} {self.shape} {kernel} not launched: {why}")

    def finish(self):
        assert not self.fail, "\n".join(self.fail)


def _forward_products(s, ran, rec):
    r = s.run
    S, N, M, Cc, Cy, g, Cg, E, dgp, NT = s.S, s.N, s.M, s.Cc, s.Cy, s.g, s.Cg, s.E, s.dgp, s.NT
    X, Y = r.X, r.Y
    Text = s.bf("Text", (S, s.KLT, Cc))
    stats = sorted(n for n in ran if n.startswith("gemm_stream_k384_n128+stats"))
    assert len(stats) <= 1 and (stats or "gemm_stream_k384_n128" in ran), ran      # the down projection always streams at these shapes
    down = stats[0] if stats else "gemm_stream_k384_n128"
    # ---- F1: fused statistics -----------------------------------------------------------------------------------------------------
    if N >= 64:                                                            # gemm_stream_stats_ok: M >= 64 rows per frame
        assert stats, ran
        sx = s.f32("sx", (2, NT))
        X2 = X.reshape(NT, Cc)
        rec.product("F1", stats[0], lambda: max(
            check_product(sx[0].reshape(NT, 1), X2, torch.ones(Cc, 1, device=X.device), out_bf16=False, k_terms=Cc, name="F1 sx row sums"),
            check_product(sx[1].reshape(NT, 1, 1), X2.reshape(NT, 1, Cc), X2.reshape(NT, Cc, 1), out_bf16=False, k_terms=Cc, name="F1 sx row sums of squares"),
            # rin = (sum of the 32-row column partials) * fl32(1 / N): fwd_kernels.hip:510, scale = 1.f / (float)d.N at moe_forward.cpp:71 --
            # the rounding of 1 / N and of the product are two more terms of 2^-24 |ref| each
            check_product(s.f32("rin", (S, 2 * Cc))[:, :Cc].reshape(S, 1, Cc), torch.full((S, 1, N), 1.0 / N, dtype=torch.float64, device=X.device), X,
                          out_bf16=False, k_terms=N + 2, name="F1 rin[:, :C]")))
    else:
        assert not stats, ran
        rec.stepped_aside("F1", "gemm_stream_k384_n128+stats", "N < 64 (gemm_stream_stats_ok)")
    # ---- F2: hop-2 logits out of the same pass ----------------------------------------------------------------------------------------
    x64 = "gemm_stream_k384_n128+stats+x64"
    if N >= 64 and S >= 2:                                                 # moe_plan.cpp: fuse_l2 needs the fused statistics and >= 2 frames
        assert x64 in ran, ran
        L2 = s.f32("L2", (S, N, s.KL))
        rec.product("F2", x64, lambda: check_product(L2, X, Text[:, :s.KL].transpose(1, 2), out_bf16=False, k_terms=Cc, name="F2 L2"))
    else:
        assert x64 not in ran, ran
        rec.stepped_aside("F2", x64, "N < 64 or a single frame (moe_plan.cpp: fuse_l2)")
    # ---- F3: the main product through z ------------------------------------------------------------------------------------------------
    # kfs_pre_small (tile_stream.hip:967-992), per token, expert e, group i, entry j:
    #     zr = Zx + gv * pw          Zx: the bf16 the GEMM stored (unpack_seg) ; pw = a . TW, latent experts only (mm_lds_finish: TW in two planes)
    #     z  = bf16( rr * (zr - mu * wsum) + dconst )        rr, mu as stored in rmu ; wsum, dconst fp32
    # so  |z - z_ref| <= |rr| * (eZx + |gv| * ePW)  +  6 * 2^-24 * (|rr| (|Zx| + |gv pw| + |mu wsum|) + |dconst|)   (six fp32 operations, each rounding a
    # value no larger than that sum)  +  2^-8 * (|z_ref| + all of the former)   (the store)
    # with eZx = Cg 2^-23 magZx + 2^-8 |Zx| (fp32 accumulation + the GEMM's bf16 store) and ePW = (Kp 2^-23 + 2^-16) magPW.
    def f3():
        Wt = s.bf("Wt", (g, E * dgp, Cg))
        Zx, magZ = product_ref(X.reshape(S, N, g, Cg).permute(0, 2, 1, 3), Wt.transpose(1, 2))                 # (S, g, N, E * dgp)
        Zx, magZ = Zx.reshape(S, g, N, E, dgp), magZ.reshape(S, g, N, E, dgp)
        eZ = product_bound(Zx, magZ, out_bf16=True, k_terms=Cg)
        rmu = s.f32("rmu", (2, E, S, N)).double()
        rr, mu = rmu[0].permute(1, 2, 0)[:, None, :, :, None], rmu[1].permute(1, 2, 0)[:, None, :, :, None]      # (S, 1, N, E, 1)
        ws, dc = s.f32("wsum", (g, E, dgp)).double()[None, :, None], s.f32("dconst", (g, E, dgp)).double()[None, :, None]
        pw, ePW = torch.zeros_like(Zx), torch.zeros_like(Zx)
        if s.El:
            a = s.bf("a", (s.El, S, N, s.Kp))
            TW = s.f32("TW", (S, s.KLT, g, E, dgp))
            for l in range(s.El):                                          # (latent experts come first: expert l owns slot l)
                gv = float(s.P[f"multimodal_experts.{l}.gate_av"])
                p, m = product_ref(a[l][:, None], TW[:, l * s.Kp:(l + 1) * s.Kp, :, l].permute(0, 2, 1, 3))      # (S, g, N, dgp)
                pw[:, :, :, l] = gv * p
                ePW[:, :, :, l] = abs(gv) * product_bound(p, m, out_bf16=False, k_terms=s.Kp, split_planes=True)
        zref = rr * (Zx + pw - mu * ws) + dc
        pre = rr.abs() * (eZ + ePW) + 6 * 2.0 ** -24 * (rr.abs() * (Zx.abs() + pw.abs() + (mu * ws).abs()) + dc.abs())
        bound = pre + EPS_BF16 * (zref.abs() + pre)
        z = s.bf("Z", (S, N, g, E, dgp)).permute(0, 2, 1, 3, 4)
        return check_bound(z, zref, bound, "F3 z = LN-folded X Wt^T")
    rec.product("F3", down, f3)
    # ---- F4 / F5: hop 1 against Y ---------------------------------------------------------------------------------------------------------
    Qx = s.bf("Qx", (s.Kcy, Cy))
    assert "k_hop1_yk" in ran and "k_hop1_yt_frames" in ran, ran            # (M % 4 == 0 and 17 <= Kcyb <= 80 at every shape here)
    rec.product("F4", "k_hop1_yk", lambda: check_product(s.bf("Rext", (S, s.Kcyb, s.Mk))[:, :s.Kcy, :M], Qx, Y.transpose(1, 2), out_bf16=True, k_terms=Cy, name="F4 Rext[..., :M]"))
    BmX = s.bf("BmX", (S, s.Kcyb, s.Mb))
    rec.product("F5", "k_hop1_yt_frames", lambda: check_product(s.bf("V", (S, s.Kcyb, Cy)), BmX[:, :, :M], Y, out_bf16=True, k_terms=M, name="F5 V"))
    # ---- F6: the output product -------------------------------------------------------------------------------------------------------------
    assert "gemm_stream_k160_n384" in ran, ran
    Ap = s.bf("Apost", (NT, g, s.KPp))
    Bp = s.bf("Bpost", (g, Cg, s.KPp))
    rec.product("F6", "gemm_stream_k160_n384", lambda: check_product(
        r.out.reshape(NT, g, Cg).permute(1, 0, 2), Ap[:, :, :s.KP].permute(1, 0, 2), Bp[:, :, :s.KP].transpose(1, 2), out_bf16=True, k_terms=s.KP, name="F6 out"))


def _section1(s, ran, rec):
    r = s.run
    NT, g, Cg, E, dgp = s.NT, s.g, s.Cg, s.E, s.dgp
    dO = r.dOut.reshape(NT, g, Cg)
    if NT >= 4096:                                                         # (and NT % 64 == 0: the shapes are chosen so)
        assert "k_dpost_pair" in ran and "k_dpair_reduce" in ran, ran
        Ap = s.bf("Apost", (NT, g, s.KPp))
        Bp = s.bf("Bpost", (g, Cg, s.KPp))
        nm = E * dgp

        def b1():
            ref, mag = product_ref(dO.permute(1, 0, 2), Bp[:, :, :s.KP])                                       # (g, NT, KP)
            a = check_bound(s.bf("dAp", (NT, g, nm)).permute(1, 0, 2), ref[:, :, :nm], product_bound(ref[:, :, :nm], mag[:, :, :nm], out_bf16=True, k_terms=Cg), "B1 dAp")
            b = check_bound(s.f32("dApx", (NT, g, s.XW))[:, :, :s.KP - nm].permute(1, 0, 2), ref[:, :, nm:],
                            product_bound(ref[:, :, nm:], mag[:, :, nm:], out_bf16=False, k_terms=Cg), "B1 dApx")
            dBp = s.f32("dBp", (g, Cg, s.KPp))
            c = check_product(dBp[:, :, :s.KP], dO.permute(1, 2, 0), Ap[:, :, :s.KP].permute(1, 0, 2), out_bf16=False, k_terms=NT, name="B1 dBp")
            # kk_dpair / kk_dpair_reduce store columns < KP only (dpost_pair.hip:217,227): the padding columns keep the workspace poison
            check_untouched(s.dev("dBp", torch.int32, (g, Cg, s.KPp))[:, :, s.KP:], -1, "B1 dBp padding columns")
            return max(a, b, c)
        rec.product("B1", "k_dpost_pair", b1)
    else:
        assert "k_dpost_pair" not in ran, ran
        rec.stepped_aside("B1", "k_dpost_pair", "fewer than 4096 tokens (dpost_pair.hip:258)")


def _dx_operands(s):
    """A = [dZx | dL2x[:, :KLT]], B = [Wt ; Text] per (frame, group), extra = rs2x * X: the three segments of the dX product"""
    S, N, g, Cg, E, dgp, Cc = s.S, s.N, s.g, s.Cg, s.E, s.dgp, s.Cc
    Zw = s.bf("Zw", (S, N, g, E * dgp)).permute(0, 2, 1, 3)                                                     # (S, g, N, 128)
    dL2 = s.bf("dL2x", (S, N, s.KLp))[:, None, :, :s.KLT].expand(S, g, N, s.KLT)
    Wt = s.bf("Wt", (g, E * dgp, Cg))[None].expand(S, g, E * dgp, Cg)
    Tx = s.bf("Text", (S, s.KLT, g, Cg)).permute(0, 2, 1, 3)
    rs = s.f32("rs2x", (S, N)).double()[:, None, :, None]
    Xg = s.run.X.reshape(S, N, g, Cg).permute(0, 2, 1, 3).double()
    return torch.cat([Zw, dL2], 3).double(), torch.cat([Wt, Tx], 2).double(), rs * Xg


def _dy_operands(s):
    """A = [BmX[:, :, :M]^T | dRT[:, :, :Kcy]], B = [dV ; Qx] per frame: the two segments of the dY product"""
    S, M, Cy = s.S, s.M, s.Cy
    BmT = s.bf("BmX", (S, s.Kcyb, s.Mb))[:, :, :M].transpose(1, 2)
    dRT = s.bf("dRT", (S, M, s.Kcyp))[:, :, :s.Kcy]
    dV = s.bf("dV", (S, s.Kcyb, Cy))
    Qx = s.bf("Qx", (s.Kcy, Cy))[None].expand(S, s.Kcy, Cy)
    return torch.cat([BmT, dRT], 2).double(), torch.cat([dV, Qx], 1).double()


def _section32(s, ran, rec, snap):
    r = s.run
    S, N, g, Cg, E, dgp, Cc, NT = s.S, s.N, s.g, s.Cg, s.E, s.dgp, s.Cc, s.NT
    for k, v in snap.items():                                              # the operands of B2 / B3 as section 1 left them
        assert torch.equal(v, s.dev(k, torch.uint8, (v.numel(),))), f"section 32 changed {k}"
    if s.KLp < 72:                                                         # tok_pair2.hip:317: dL2x rows at least 72 wide (two cross-modal experts)
        assert "k_tok_pair2" not in ran and "gemm_tokpair" in ran, ran
        rec.stepped_aside("B2", "k_tok_pair2", "dL2x rows narrower than 72 (tok_pair2.hip:317): gemm_tokpair ran")
        return
    assert "k_tok_pair2" in ran and "k_tp2_finish" in ran, ran             # (N >= 16, KL <= 64 at every shape here)
    nm = E * dgp
    Zw = s.bf("Zw", (NT, g, nm))
    X = r.X
    dTW = s.bf("dTW", (S, s.KLT, g, nm))
    Text = s.bf("Text", (S, s.KLT, g, Cg))
    Wt = s.bf("Wt", (g, nm, Cg))

    def b2():
        # dWt[i] = dZx[:, i]^T X[:, i] (tok_pair2) + dTW[:, :, i]^T Text[:, :, i] (engine, accumulating: moe_backward.cpp:287): one fp32 sum of
        # NT + S * KLT products, the accumulating epilogue's add is one more rounding of a partial sum
        A = torch.cat([Zw.permute(1, 2, 0), dTW.reshape(S * s.KLT, g, nm).permute(1, 2, 0)], 2)
        B = torch.cat([X.reshape(NT, g, Cg).permute(1, 0, 2), Text.reshape(S * s.KLT, g, Cg).permute(1, 0, 2)], 1)
        a = check_product(s.f32("dWt", (g, nm, Cg)), A, B, out_bf16=False, k_terms=NT + S * s.KLT + 1, name="B2 dWt")
        # dT[s] = dL2[s]^T X[s] (tok_pair2) + dTW[s] Wt (:313) + 2 dTT[s] T[s] (:329, alpha = 2 is exact); the slots are 32 rows each
        dL2 = s.bf("dL2x", (S, N, s.KLp))[:, :, :s.KL]
        dTT = s.bf("dTT", (S, s.El, 32, s.Kp))
        A2 = torch.zeros(S, g, s.KL, N + nm + s.KL, dtype=torch.float64, device=X.device)
        A2[:, :, :, :N] = dL2.transpose(1, 2)[:, None].double()
        A2[:, :, :, N:N + nm] = dTW[:, :s.KL].permute(0, 2, 1, 3).double()
        for l in range(s.El):
            A2[:, :, l * 32:(l + 1) * 32, N + nm + l * 32:N + nm + (l + 1) * 32] = 2.0 * dTT[:, l][:, None].double()
        B2 = torch.cat([X.reshape(S, N, g, Cg).permute(0, 2, 1, 3), Wt[None].expand(S, g, nm, Cg), Text[:, :s.KL].permute(0, 2, 1, 3)], 2)
        b = check_product(s.f32("dT", (S, s.KL, g, Cg)).permute(0, 2, 1, 3), A2, B2, out_bf16=False, k_terms=N + nm + s.Kp + 2, name="B2 dT")
        return max(a, b)
    rec.product("B2", "k_tok_pair2", b2)


def _section64(s, ran, rec):
    S, N, g, Cg = s.S, s.N, s.g, s.Cg
    if N >= 64 and s.KLp >= 72:                                            # dx_stream2.hip:184 (and S * N >= 2048: every shape here)
        assert "k_dx_stream2" in ran, ran
        A, B, extra = _dx_operands(s)
        # + 2: the fp32 multiply and add of the row-scale term (dx_stream2.hip:170)
        rec.product("B3", "k_dx_stream2", lambda: check_product(s.run.dX.reshape(S, N, g, Cg).permute(0, 2, 1, 3), A, B, extra=extra, out_bf16=True,
                                                                k_terms=A.shape[-1] + 2, name="B3 dX"))
    else:
        assert "k_dx_stream2" not in ran, ran
        rec.stepped_aside("B3", "k_dx_stream2", "N < 64 or dL2x rows narrower than 72 (dx_stream2.hip:184)")


def _section8(s, ran, rec):
    S, M, Cy = s.S, s.M, s.Cy
    Y = s.run.Y
    assert "k_hop1_yk" in ran, ran                                        # (M % 4 == 0, Kcyb <= 80 at every shape here)
    dV = s.bf("dV", (S, s.Kcyb, Cy))

    def b4():
        a = check_product(s.f32("dBm", (S, s.Kcyb, s.Mb))[:, :, :M], dV, Y.transpose(1, 2), out_bf16=False, k_terms=Cy, name="B4 dBm")
        if s.Kcyp < 64:
            return a
        dRT = s.bf("dRT", (S * M, s.Kcyp))[:, :s.Kcy]
        return max(a, check_product(s.bf("dQT", (s.Kcy, Cy)), dRT.transpose(0, 1), Y.reshape(S * M, Cy), out_bf16=True, k_terms=S * M, name="B4 dQ (stored as dQT)"))
    if s.Kcyp >= 64:                                                       # hop1_stream.hip:462: rows of dRT at least 64 wide (two cross-modal experts)
        assert "k_hop1_yt_sum" in ran and "k_hop1_sum" in ran, ran
        rec.product("B4", "k_hop1_yk+k_hop1_yt_sum", b4)
    else:
        assert "k_hop1_yt_sum" not in ran, ran
        rec.stepped_aside("B4", "k_hop1_yt_sum", "dRT rows narrower than 64 (hop1_stream.hip:462); dBm checked below")
        rec.product("B4", "k_hop1_yk", b4)


def _section16(s, ran, rec):
    S, M, Cy = s.S, s.M, s.Cy
    dyk = [n for n in ran if n.startswith("gemm_stream_k64+96mn")]
    if M >= 64 or S == 1:                                                  # gemm_stream.hip:602: several frames need >= 64 rows each
        assert dyk, ran
        A, B = _dy_operands(s)
        rec.product("B5", dyk[0], lambda: check_product(s.run.dY, A, B, out_bf16=True, k_terms=A.shape[-1], name="B5 dY"))
    else:
        assert not dyk, ran
        rec.stepped_aside("B5", "gemm_stream_k64+96mn", "fewer than 64 tokens of Y per frame (gemm_stream.hip:602)")


@pytest.mark.parametrize("shape", list(SHAPES))
def test_products_of_one_site(shape):
    S, N, M, E_m, E_s = SHAPES[shape]
    rec = Recorder(shape)
    with Profiled() as prof:
        s = Site(_cfg(N, M, E_m, E_s), S, seed=21)
        s.run.forward()
        _forward_products(s, prof.names(), rec)
        s.begin_backward()
        s.part(1)
        ran = prof.names()
        _section1(s, ran, rec)
        snap = {k: s.dev(k, torch.uint8, (s.run.table[k][2],)).clone() for k in ("Zw", "dL2x", "rs2x")}
        s.part(32)
        _section32(s, prof.names(), rec, snap)
        s.part(64)
        _section64(s, prof.names(), rec)
        s.part(8)
        _section8(s, prof.names(), rec)
        s.part(16)
        _section16(s, prof.names(), rec)
        assert s.run.guards_intact(), "a kernel wrote past its workspace"
        assert torch.isfinite(s.run.out.float()).all() and torch.isfinite(s.run.dX.float()).all() and torch.isfinite(s.run.dY.float()).all()
    rec.finish()


@pytest.mark.parametrize("shape", list(PAIR_SHAPES))
def test_token_gradient_of_a_site_pair(shape):
    """B6: dT = dX_A + dY_B from ONE kernel (avmoe_moe_backward_dx_dy after sections 1 + 32 + 8 of both sites): the three segments of site A's dX
    product and the two of site B's dY product, read from the two sites' workspaces."""
    S, Na, Nb, E_m, E_s = PAIR_SHAPES[shape]
    S = max(S, -(-2048 // Na))                                             # dx_stream3.hip:370: >= 2048 tokens
    rec = Recorder(shape)
    with Profiled() as prof:
        g = torch.Generator().manual_seed(77)
        Ta, Tb = 0.3 * torch.randn(S, Na, 768, generator=g), 0.3 * torch.randn(S, Nb, 768, generator=g)
        a = Site(_cfg(Na, Nb, E_m, E_s), S, seed=31, X=Ta, Y=Tb)
        b = Site(_cfg(Nb, Na, E_m, E_s), S, seed=32, X=Tb, Y=Ta)
        for s in (a, b):
            s.run.forward()
            s.begin_backward()
            for p in (1, 32, 8):
                s.part(p)
        dT = torch.full_like(a.run.X, float("nan"))
        st = a.run.L.avmoe_moe_backward_dx_dy(C.byref(a.run.desc), a.run.X.data_ptr(), a.run.saved.data_ptr(), a.run.scratch.data_ptr(),
                                              C.byref(b.run.desc), b.run.saved.data_ptr(), b.run.scratch.data_ptr(), dT.data_ptr(),
                                              torch.cuda.current_stream().cuda_stream)
        ran = prof.names()
        if a.KLp < 72:                                                     # moe_backward.cpp:502: site A's dL2x rows at least 72 wide
            assert st == 1 and "k_dx_stream3" not in ran, (st, ran)
            rec.stepped_aside("B6", "k_dx_stream3", "site A has one cross-modal expert: dL2x rows narrower than 72 (moe_backward.cpp:502)")
            return
        assert st == 0, (st, a.run.L.avmoe_last_error())
        assert "k_dx_stream3" in ran, ran
        Ax, Bx, extra = _dx_operands(a)                                    # (S, g, Na, .), (S, g, ., Cg)
        Ay, By = _dy_operands(b)                                           # (S, Na, .), (S, ., 768)
        gq, Cg = a.g, a.Cg
        A = torch.cat([Ax, Ay[:, None].expand(S, gq, Na, Ay.shape[-1])], 3)
        B = torch.cat([Bx, By.reshape(S, By.shape[1], gq, Cg).permute(0, 2, 1, 3)], 2)
        # + 2: the fp32 multiply and add of the row-scale term (dx_stream3.hip:351)
        rec.product("B6", "k_dx_stream3", lambda: check_product(dT.reshape(S, Na, gq, Cg).permute(0, 2, 1, 3), A, B, extra=extra, out_bf16=True,
                                                                k_terms=A.shape[-1] + 2, name="B6 dT = dX_A + dY_B"))
        assert a.run.guards_intact() and b.run.guards_intact(), "a kernel wrote past its workspace"
        assert torch.isfinite(dT.float()).all()
    rec.finish()


@pytest.mark.parametrize("S,N", [(20, 196), (16, 256), (40, 76), (3, 1000)])
def test_fused_statistics_are_exact_on_small_integers(S, N):
    """X drawn from the integers -3 .. 3: every product and partial sum of the fused statistics is an integer far below 2^24, so there is no
    tolerance at all -- sx equals the integer row sums / sums of squares bit for bit, rin[:, :C] equals fl32(column sum * fl32(1 / N)), the ONE
    rounding of kk_xstats_fin's `* scale`.  Pins the ragged last tile of a frame and the 32-row column-partial chunks."""
    cfg = _cfg(N, 64, 2, 2)
    g = torch.Generator().manual_seed(S * 1000 + N)
    X = torch.randint(-3, 4, (S, N, 768), generator=g).float()
    with Profiled() as prof:
        s = Site(cfg, S, seed=5, X=X)
        s.run.forward()
        ran = prof.names()
        assert any(n.startswith("gemm_stream_k384_n128+stats") for n in ran), ran
        sx = s.f32("sx", (2, S * N)).cpu()
        rin = s.f32("rin", (S, 2 * 768))[:, :768].cpu()
        assert s.run.guards_intact()
    X2 = X.reshape(S * N, 768)
    assert torch.equal(sx[0], X2.sum(1)), int((sx[0] != X2.sum(1)).sum())
    assert torch.equal(sx[1], (X2 * X2).sum(1)), int((sx[1] != (X2 * X2).sum(1)).sum())
    want = X.double().sum(1).float() * torch.tensor(1.0, dtype=torch.float32).div(float(N))
    assert torch.equal(rin, want), (int((rin != want).sum()), float((rin - want).abs().max()))
    CHECKED.setdefault("F1 exact", {})[f"{S}x{N}"] = ("gemm_stream_k384_n128+stats", 0.0)


def test_every_streaming_product_was_checked():
    """Closes the module: each of the twelve products was checked against fp64, with its kernel family seen by the profiler, in at least two
    shapes, one of them ragged.  (Runs after the tests above: it fails when they did not run or a product was skipped.)"""
    missing = {}
    for tag in PRODUCTS:
        got = CHECKED.get(tag, {})
        if len(got) < 2 or not (set(got) & RAGGED):
            missing[tag] = (PRODUCTS[tag], sorted(got))
    for tag, shapes in sorted(CHECKED.items()):
        for sh, (kernel, ratio) in sorted(shapes.items()):
            print(f"COVERED {tag} {sh} {kernel} {ratio:.4f}")
    assert not missing, f"products not checked in two shapes (one ragged): {missing}"
