"""The per-token bottleneck-space passes of the tuned site (C = 768 in 2 groups, bottleneck 64, 32 latent tokens) checked ELEMENT BY ELEMENT
against fp64 recomputed from the operands exactly as each kernel read them, with the derived bounds of tests/pass_ref.py
(tests/test_pass_checker.py shows what such a check catches: one token row from the neighbouring tile, a frame boundary off by one, two
experts or the two groups swapped, one element two bf16 ulps off).  Three forms of the same arithmetic: kfs_* (csrc/tile_stream.hip,
HOOK_KFS_FORCE), kf_*<bf16> (csrc/tile_fast.hip, HOOK_KFS_OFF) and kf_*<float> (an fp32 site of the same shape).  The profiler is on and
the scope names (csrc/pass.h: "... (stream)" when the streamed form ran, as tests/test_pass_forms_gpu.py reads them) assert which form ran.

Checked here (the tags of the closing coverage test):
  P1  pre_small: a = the softmax over each latent slot of the stored L2, rmu = (rr, mu) from sx, L2, a AS STORED, TT and Tsum
      (tile_fast.hip:572-637, tile_stream.hip:896-955).
  P1z z through its defining map rnd_T(rr (Zx + gv a . TW - mu wsum) + dconst) (tile_fast.hip:651-652), Zx recomputed from X and Wt with the
      down projection's own bound (Z held Zx only until the pass overwrote it in place), rr / mu as stored: F3 of
      test_stream_products_gpu.py, here in all three forms.
  P2  bn1 = (mean, rstd, scale, shift) from the stored Z: fp32 column sums over all NT tokens, finalized in double (fwd_kernels.hip:988-1004).
  P3  mz, Szz: in gram64 mode from z' as gram.hip forms it (act(BN1(z)) rounded to bf16, :94-99; only elements within the fp32 evaluation's
      error of a bf16 rounding tie carry an operand error); otherwise Szz as the engine's contraction of the stored Zp and mz as its column
      means (fwd_kernels.hip:1140).
  P4  post_small: rpmup, the main columns of Apost, the 3 E scalar columns from rp / mup AS STORED (tile_fast.hip:321-339), the padding
      columns KP..KPp.  No kernel writes the padding (kf_post_small stores 32 columns per expert at e * 32 and 3 E scalars at E * 32:
      tile_fast.hip:308,329; tile_stream.hip:712,735) and the output product contracts over K = KP columns only (moe_forward.cpp:273): the
      contract is "untouched", asserted against the workspace poison as test_stream_products_gpu.py does for dBp.
  P5  dSooT, gram64 mode, register-resident bf16 form only (tile_fast.hip:497; the streamed form keeps dSoo in registers for its fused
      Gram product: tile_stream.hip:333, and three experts / fp32 sites have no gram64 mode: moe_plan.cpp:176).
  P6  the final dzp = post_small_bwd followed by mid_bwd, as ONE map from dAp / dApx (kf_mid_bwd rewrites dzp in place,
      tile_fast.hip:161, so what the first pass stored does not survive section 1; its store is one named rounding in the bound).
  P7  dGq in its three forms: from dSooT as stored with gram.hip's operand rounding reproduced exactly (register-resident form, gram64
      mode); from the reference's dSoo with its bound and the operand's bf16 rounding as a named term (the fused streamed form, mirror
      tile included); on the engine path (three experts, fp32) Zw = rnd_T(dSoo z') from the reference's dSoo in the same way against the
      stored Zp (tile_fast.hip:502-504, moe_backward.cpp:131-136).
  P8  dsm[3], dsm[4] = the token means of dy and dy * zh from the final dzp as stored (bwd_kernels.hip:72-73).
  P9  pre_small_bwd: Zw (= dZx), dslat (register-resident forms: the streamed form hands the sums over in registers, tile_stream.hip:1202),
      dL2x[:, KL], dL2x[:, KL + 1] == 1 exactly, rs2x.
  P10 dL2x[:, :KL] from a, L2, TT, TW, Tsum, the gate and dzraw / the LayerNorm sums: read back as stored (Zw, dslat) in the register-resident
      forms; in the streamed form they never leave the registers, so the reference carries pre_small_bwd's values and bounds forward.
      Columns KLT..KLp: written by nobody, read by nobody (every reader contracts K = KLT: moe_backward.cpp:37, :263, :300): untouched.

Survival of operands and results to the end of section 1 (moe_backward.cpp:86-150): Z, bn1, Gq, uvh, probs, rpmup, rmu, wsum, dconst are
forward state, read as const by every backward kernel; dAp / dApx are written by phase 1 (:119) and only read afterwards; sdSzz and
dsm[0..2] are written by k_post_prep_bwd (:140) before mid_bwd reads them, dsm[3, 4] by mid_bwd's finalizer before pre_small_bwd reads them
(tile_fast.hip:711), and nothing later in section 1 rewrites any of them; dzp is last written by mid_bwd, Zw / dL2x / rs2x / dslat by
pre_small_bwd (Zw held dSoo z' before, in the non-Gram path only: that operand of the engine's dGq is gone by then, Zp is not).  dApost
arrives split (bf16 columns + fp32 dApx) or whole (one fp32 array, moe_backward.cpp:113); which one is read off the workspace: the poison
survives in dApx exactly when the whole form ran.

Every site here runs in training mode with BatchNorm, both LayerNorms and the gate on.  The run-time branches of the same kernels for
ln_before, ln_post, use_gate or use_bn off and for eval mode are held per token by tests/test_pass_variants_fp64_gpu.py (at ragged_196,
short_frame_20 and three_experts of this module's shapes).  NOT checked in either: the XR instantiations (N x N and frame-attention experts)."""
import pytest
import torch

from oracle import avmoe_oracle as O
from tests import pass_ref as R
from tests.stream_product_ref import check_bound, check_untouched, product_bound, product_ref
from tests.test_round6_kernels_gpu import _cfg
from tests.test_stream_products_gpu import Profiled, Recorder, Site, _release_device_memory  # noqa: F401  (the fixture: autouse here too)

pytestmark = pytest.mark.gpu

TAGS = {"P1": "pre_small: a, rmu", "P1z": "pre_small: z through its defining map",
        "P2": "pre_small column sums + k_bn1_finalize: bn1 mean / rstd / scale / shift",
        "P8": "mid_bwd column sums + finalizer: dsm[3], dsm[4]",
        "P3": "mz and Szz from z' as the Gram kernel forms it (gram64 mode); from the stored Zp otherwise",
        "P7": "dGq in the fused streamed form, from gram.hip and on the engine path",
        "P4": "post_small: rpmup, Apost main / scalar / padding columns", "P5": "post_small_bwd: dSooT",
        "P6": "post_small_bwd + mid_bwd: final dzp", "P9": "pre_small_bwd: Zw, dslat, dL2x[:, KL:KL + 2], rs2x",
        "P10": "pre_lat_bwd / the fused pass: dL2x[:, :KL]"}
# (frames, N, M, E_m, E_s): the smallest shapes at which these kernels can go wrong
SHAPES = {
    "ragged_196": (20, 196, 64, 2, 2),                 # streams unforced; ragged last tile
    "short_frame_20": (40, 20, 32, 2, 2),              # a frame shorter than two 16-token tiles
    "many_frames": (300, 48, 32, 2, 2),                # persistent blocks walk several frames; more virtual blocks than CUs
    "one_frame": (1, 1024, 64, 2, 2),
    "ragged_100": (30, 100, 32, 2, 2),                 # a second shape at which pre_small streams (four experts, >= 2 frames of >= 64 tokens)
    "three_experts": (16, 180, 64, 1, 2),              # no gram64 mode
    "two_experts": (16, 180, 64, 1, 1),
}
RAGGED = {"ragged_196", "ragged_100", "short_frame_20", "three_experts", "two_experts"}      # (196, 20 and 180 are no multiples of 16)
FORMS = {"stream": ("HOOK_KFS_FORCE", True), "fast": ("HOOK_KFS_OFF", True), "f32": (None, False)}
CASES = [(f, sh) for f in FORMS for sh in SHAPES if f != "f32" or sh in ("ragged_196", "short_frame_20", "three_experts")]
CHECKED = {}      # (tag, form) -> {shape: worst err / bound}
ASIDE = {}        # (tag, form) -> {shape: why}


class PassSite(Site):
    """tests/test_stream_products_gpu.py::Site in either element type (that class is bf16 only)"""

    def __init__(self, cfg, S, seed, bf16):
        from tests.moe_gpu_util import MoeRun
        P, B = O.init_params(cfg, seed=seed)
        g = torch.Generator().manual_seed(seed + 100)
        X = 0.3 * torch.randn(S, cfg.Nx, cfg.Cx, generator=g)
        Y = 0.3 * torch.randn(S, cfg.Ny, cfg.Cy, generator=g)
        self.G = torch.randn(S, cfg.Nx, cfg.Cx, generator=g)
        self.P, self.cfg, self.S, self.bf16 = P, cfg, S, bf16
        self.T = torch.bfloat16 if bf16 else torch.float32
        self.run = MoeRun(cfg, P, B, X, Y, bf16=bf16, training=True)
        self.E, self.g, self.N, self.El = cfg.E, cfg.groups, cfg.Nx, cfg.E_m
        self.NT = S * self.N
        self.dgp = self.run.table["wsum"][2] // 4 // (self.E * self.g)
        self.KL = self.El * 32
        self.KLp = -(-(self.KL + 2) // 8) * 8
        self.KP = self.E * 32 + 3 * self.E
        self.KPp = -(-self.KP // 8) * 8
        self.XW = -(-(self.KPp - self.E * 32) // 16) * 16
        esz = 2 if bf16 else 4
        assert self.dgp == 32 and self.g == 2 and self.run.table["Z"][2] == self.NT * self.E * 2 * 32 * esz        # (the tuned layout)
        self.relu = torch.tensor([e < cfg.E_m for e in range(cfg.E)])      # (the cross-modal experts come first and carry the ReLU: net_trans_v3.py:398)

    def z(self, name):
        """a Z-space tensor (Z, dzp, Zw) as (NT, g, E, 32): rows are [group][expert][32] (tile_fast.hip:99 col = g * E * 32 + e * 32 + c)"""
        return self.dev(name, self.T, (self.NT, self.g, self.E, 32))

    def tokE(self, name):
        """[r | mu][expert][token] -> two (NT, E) tensors"""
        v = self.f32(name, (2, self.E, self.NT))
        return v[0].t(), v[1].t()


class PassRecorder(Recorder):
    """Recorder that files a margin under (tag, form) for this module's coverage test"""

    def __init__(self, shape, form):
        super().__init__(shape)
        self.form = form

    def product(self, tag, kernel, fn):
        try:
            ratio = fn()
        except AssertionError as e:
            self.fail.append(f"{tag} [{self.form}: {kernel}]: {e}")
            return
        CHECKED.setdefault((tag, self.form), {})[self.shape] = ratio
        print(f"MARGIN {tag} {self.shape} {self.form} {kernel} worst_err_over_bound {ratio:.4f}")


def _aside(rec, tag, kernel, why):
    rec.stepped_aside(tag, kernel, why)
    ASIDE.setdefault((tag, rec.form), {})[rec.shape] = why


def _forward(s, form, ran, rec):
    NT, g, E, S, N = s.NT, s.g, s.E, s.S, s.N
    bf16 = s.bf16
    DZ = g * E * 32
    # ---- P2: BatchNorm-1 statistics, column sums over all NT tokens of the z that pre_small stored ---------------------------------------
    pre_streams = "k_pre_small (stream)" in ran
    assert ("k_pre_small" in ran) == (not pre_streams), ran
    # the streamed pre_small wants the fused hop-2 logits, Dims::fuse_l2 (moe_plan.cpp:181): E * dgp == 128, >= 2 frames, the fused statistics
    # (>= 64 tokens per frame): at two_experts and three_experts the register-resident pre_small runs under HOOK_KFS_FORCE too.
    assert pre_streams == (form == "stream" and E == 4 and S >= 2 and N >= 64), ran
    pre_checked = form != "stream" or pre_streams      # (under "stream" the register-resident kernel is NOT filed: the "fast" case of the same shape checks it)
    if not pre_checked:
        why = "one frame" if S < 2 else "fewer than 64 tokens per frame" if N < 64 else "E * dgp != 128 (fewer than four experts)"
        for tag in ("P1", "P1z", "P2"):
            _aside(rec, tag, "k_pre_small (stream)", f"no fused hop-2 logits ({why}): the register-resident pre_small ran")
    pfx = s.cfg.expert_prefixes()
    pre_name = "k_pre_small (stream)" if pre_streams else "k_pre_small"
    # ---- P1: the softmax over each latent slot of the stored L2; (rr, mu) from sx, L2, a as stored, TT, Tsum ------------------------------
    El, KLT = s.El, s.KL + 2
    L2 = s.f32("L2", (NT, El, 32))                                         # [token][slot][32] (tile_fast.hip:580; written by the pass itself when the logits are fused, :662)
    a = s.dev("a", s.T, (El, NT, 32)).permute(1, 0, 2)                     # planes per slot (tile_fast.hip:661)
    Tsum = s.f32("Tsum", (2, S, KLT))[0][:, :s.KL].reshape(S, El, 32).repeat_interleave(N, 0)          # the row sums of Text (moe_plan.h:102)
    gv = torch.tensor([float(s.P[f"{p}.gate_av"]) if e < El else 0.0 for e, p in enumerate(pfx)])

    def p1():
        x = check_bound(a, *R.softmax_ref(L2, out_bf16=bf16), "P1 a (token, latent slot, latent token)")
        ref = R.rmu_ref(s.f32("sx", (2, NT)), L2, a, s.f32("TT", (S, El, 32, 32)), Tsum, gv, s.cfg.Cx, s.cfg.ln_eps, planes=bf16)
        rr, mu = s.tokE("rmu")
        return max(x, check_bound(rr, *ref["rr"], "P1 rmu[0] = rr (token, expert)"), check_bound(mu, *ref["mu"], "P1 rmu[1] = mu (token, expert)"))
    if pre_checked:
        rec.product("P1", pre_name, p1)
    # ---- P1z: z through its defining map from the down projection recomputed (Z held Zx until the pass overwrote it in place) -----------------
    Cg = s.cfg.Cx // g
    X = s.run.X.reshape(NT, g, Cg).permute(1, 0, 2)                        # (g, NT, Cg)
    Wt = s.dev("Wt", s.T, (g, E * 32, Cg))                                 # [group][expert][32][c] (moe_plan.h:88)
    eng = 0.0 if bf16 else 2.0 ** -27                                      # fp32 operands as three bf16 planes, six plane products (DESIGN_CURRENT 3c)

    def p1z():
        Zx, magZ = product_ref(X, Wt.transpose(1, 2))                      # (g, NT, E * 32): the GEMM's own fp32 sum over Cg terms and its store
        eZ = product_bound(Zx, magZ, out_bf16=bf16, k_terms=Cg) + eng * magZ
        Zx, eZ = (v.reshape(g, NT, E, 32).permute(1, 0, 2, 3) for v in (Zx, eZ))
        pw, epw = torch.zeros_like(Zx), torch.zeros_like(Zx)
        TWall = s.f32("TW", (S, KLT, g, E, 32))
        af = a.reshape(S, N, El, 32)
        for l in range(El):                                                # gv * (a . TW): 32 terms, two planes in the bf16 forms (tile_fast.hip:642), then the product with gv
            T = TWall[:, l * 32:(l + 1) * 32, :, l]                         # (S, 32, g, 32)
            p, m = (torch.einsum("snk,skic->snic", u, v).reshape(NT, g, 32) for u, v in ((af[:, :, l].double(), T.double()), (af[:, :, l].double().abs(), T.double().abs())))
            pw[:, :, l] = float(gv[l]) * p
            epw[:, :, l] = abs(float(gv[l])) * (32 * R.EPS_ACC + (R.EPS_PLANES if bf16 else 0.0)) * m
        rr, mu = s.tokE("rmu")
        ref, bound = R.z_map_ref(Zx, eZ, pw, epw, rr, mu, s.f32("wsum", (g, E, 32)), s.f32("dconst", (g, E, 32)), out_bf16=bf16)
        return check_bound(s.z("Z"), ref, bound, "P1z z = LN-folded X Wt^T (token, group, expert, entry)")
    if pre_checked:
        rec.product("P1z", pre_name, p1z)
    wb = [torch.stack([s.P[f"{p}.bn1.{k}"].reshape(g, 32) for p in pfx], 1).to(s.run.dev) for k in ("weight", "bias")]      # (g, E, 32)

    def p2():
        ref, bound = R.bn1_ref(s.z("Z"), wb[0], wb[1], s.cfg.bn_eps)
        return check_bound(s.f32("bn1", (4, g, E, 32)), ref, bound, "P2 bn1 ([mean, rstd, scale, shift], group, expert, entry)")
    if pre_checked:
        rec.product("P2", pre_name + " + k_bn1_finalize", p2)
    # ---- P3: BatchNorm-2 moments of z' -----------------------------------------------------------------------------------------------
    if bf16 and E in (2, 4):                                               # gram64 mode (moe_plan.cpp:176): z' formed on the fly in bf16, one pass (moe_forward.cpp:257)
        assert "k_gram64" in ran and "k_mid" not in ran, ran

        def p3():
            ref = R.gram_ref(s.z("Z"), s.f32("bn1", (4, g, E, 32)), s.relu)
            return max(check_bound(s.f32("mz", (g, E, 32)), *ref["mz"], "P3 mz (group, expert, entry)"),
                       check_bound(s.f32("Szz", (g, E, 32, 32)), *ref["Szz"], "P3 Szz (group, expert, row, column)"))
        rec.product("P3", "k_gram64", p3)
    else:                                                                  # kf_mid stores z' (Zp), the engine contracts it over the tokens (moe_forward.cpp:259-266)
        assert "k_mid" in ran and "k_gram64" not in ran, ran

        def p3e():
            Zp = s.z("Zp").double()
            ref = torch.einsum("tgej,tgel->gejl", Zp, Zp) / NT
            mag = torch.einsum("tgej,tgel->gejl", Zp.abs(), Zp.abs()) / NT
            # fp32 operands go to the matrix pipe as three bf16 planes, six plane products: 2^-27 per product (DESIGN_CURRENT 3c); alpha = 1 / NT
            x = check_bound(s.f32("Szz", (g, E, 32, 32)), ref, ((NT + 2) * R.EPS_ACC + eng) * mag, "P3 Szz = Zp^T Zp / NT (group, expert, row, column)")
            return max(x, check_bound(s.f32("mz", (g, E, 32)), *R.colsum_ref(Zp, 1.0 / NT), "P3 mz = column means of the stored Zp (fwd_kernels.hip:1140)"))
        rec.product("P3", "k_mid + engine", p3e)
    # ---- P4 ---------------------------------------------------------------------------------------------------------------------------
    name = "k_post_small (stream)" if form == "stream" else "k_post_small"
    assert name in ran and ("k_post_small (stream)" in ran) == (form == "stream"), ran
    uvh = s.f32("uvh", (2 * DZ + 2 * g * E,))
    us, vh = uvh[:DZ].reshape(g, E, 32), uvh[DZ:2 * DZ].reshape(g, E, 32)
    H1p, H2p = uvh[2 * DZ:2 * DZ + g * E].reshape(g, E), uvh[2 * DZ + g * E:].reshape(g, E)        # (tile_fast.hip:256)
    probs = s.f32("probs", (S, E))
    # the gate lives in weight space (moe_plan.cpp:35 gate_w; tile_fast.hip:1132 use_gate = 0): qv = probs.  Checked, not trusted: the
    # third scalar column of Apost is q itself
    qv = probs.repeat_interleave(N, 0)
    rp, mup = s.tokE("rpmup")
    Ap = s.dev("Apost", s.T, (NT, g, s.KPp))
    cfg = s.cfg

    def p4():
        ref = R.post_small_ref(s.z("Z"), s.f32("bn1", (4, g, E, 32)), s.f32("Gq", (g, E, 32, 32)), us, vh, H1p, H2p, qv, s.relu, cfg.Cx, cfg.ln_eps,
                               planes=bf16, out_bf16=bf16)
        a = check_bound(rp, *ref["rp"], "P4 rpmup[0] = rp (token, expert)")
        b = check_bound(mup, *ref["mup"], "P4 rpmup[1] = mup (token, expert)")
        c = check_bound(Ap[:, :, :E * 32].reshape(NT, g, E, 32), *ref["Apost"], "P4 Apost main columns (token, group, expert, entry)")
        cr, cb = R.scalar_cols_ref(qv, rp, mup, out_bf16=bf16)
        sc = Ap[:, :, E * 32:s.KP].reshape(NT, g, E, 3)
        d = check_bound(sc, cr[:, None].expand(NT, g, E, 3), cb[:, None].expand(NT, g, E, 3), "P4 Apost scalar columns (token, group, expert, [q rp, -q rp mup, q])")
        if s.KPp > s.KP:
            isz = torch.int16 if bf16 else torch.int32
            check_untouched(s.dev("Apost", isz, (NT, g, s.KPp))[:, :, s.KP:], -1, "P4 Apost padding columns KP..KPp")
        return max(a, b, c, d)
    rec.product("P4", name, p4)


def _backward(s, form, ran, rec):
    NT, g, E, S, N = s.NT, s.g, s.E, s.S, s.N
    bf16, cfg = s.bf16, s.cfg
    stream = form == "stream"
    gram64 = bf16 and E in (2, 4)                                          # moe_plan.cpp:176
    # ---- which forms ran ------------------------------------------------------------------------------------------------------------
    if stream:
        assert "k_mid_bwd (stream)" in ran and "k_pre_bwd (stream)" in ran and "k_pre_small_bwd" not in ran, ran
        psb_streams = "k_post_small_bwd (stream)" in ran
        assert ("k_post_small_bwd" in ran) == (not psb_streams), ran
        if E == 3:                                                         # no Gram-fused mode: the streamed post_small_bwd steps aside (tile_stream.hip:148)
            assert not psb_streams, ran
            rec.stepped_aside("P6", "k_post_small_bwd (stream)", "three experts: no gram64 mode; the register-resident first half ran, mid_bwd streamed")
        else:                                                              # two and four experts: the Gram-fused streamed form
            assert psb_streams, ran
        psb = "k_post_small_bwd (stream)" if psb_streams else "k_post_small_bwd"
        mdb, prb = "k_mid_bwd (stream)", "k_pre_bwd (stream)"
    else:
        assert not any(n.endswith("(stream)") for n in ran), ran
        assert all(n in ran for n in ("k_post_small_bwd", "k_mid_bwd", "k_pre_small_bwd")), ran
        psb, mdb, prb, psb_streams = "k_post_small_bwd", "k_mid_bwd", "k_pre_small_bwd", False
    # ---- operands as stored -----------------------------------------------------------------------------------------------------------
    DZ = g * E * 32
    Z, bn1 = s.z("Z"), s.f32("bn1", (4, g, E, 32))
    uvh = s.f32("uvh", (2 * DZ + 2 * g * E,))
    us, vh = uvh[:DZ].reshape(g, E, 32), uvh[DZ:2 * DZ].reshape(g, E, 32)
    qv = s.f32("probs", (S, E)).repeat_interleave(N, 0)
    rp, mup = s.tokE("rpmup")
    dsm = s.f32("dsm", (8, g, E, 32))                                      # dusum, dvh, dmz / NT, mdy, mdyz, .. (moe_plan.h:182)
    split = bf16 and not bool(torch.isnan(s.f32("dApx", (NT, g, s.XW))[:, :, :3 * E]).any())
    if split:                                                              # bf16 columns (rows E * 32 wide) + fp32 dApx (moe_backward.cpp:108-109)
        dAp = s.dev("dAp", torch.bfloat16, (NT, g, E, 32))
        dApx = s.f32("dApx", (NT, g, s.XW))[:, :, :3 * E].reshape(NT, g, E, 3)
    else:                                                                  # one fp32 array (NT, g, KPp)
        whole = s.f32("dAp", (NT, g, s.KPp))
        dAp, dApx = whole[:, :, :E * 32].reshape(NT, g, E, 32), whole[:, :, E * 32:s.KP].reshape(NT, g, E, 3)
    if psb_streams:
        assert split, "the streamed post_small_bwd reads the split dApost"
    print(f"DAPOST {rec.shape} {form}: {'split (bf16 + dApx)' if split else 'whole (fp32)'}")
    dzp = s.z("dzp")
    ref = R.post_mid_bwd_ref(dAp, dApx, Z, bn1, s.f32("Gq", (g, E, 32, 32)), us, vh, qv, rp, mup, dsm[2], s.f32("sdSzz", (g, E, 32, 32)), s.relu, cfg.Cx,
                             planes=bf16, out_bf16=bf16)
    # ---- P5 -------------------------------------------------------------------------------------------------------------------------
    if gram64 and not psb_streams:
        rec.product("P5", psb, lambda: check_bound(s.f32("dSooT", (E, NT)).t(), *ref["dSoo"], "P5 dSooT (token, expert)"))
    else:
        _aside(rec, "P5", psb, "dSoo stays in registers (streamed: fused Gram product)" if psb_streams else "no gram64 mode (three experts / fp32): dSooT is not written")
    # ---- P7: dGq = sum_t dSoo z' z'^T --------------------------------------------------------------------------------------------------
    if gram64:
        assert ("k_gram64" in ran) == (not psb_streams), ran               # (the streamed post_small_bwd leaves dGq itself: moe_backward.cpp:126)
        dSoo_st = None if psb_streams else s.f32("dSooT", (E, NT)).t()

        def p7():
            w, ew = (ref["dSoo"][0], ref["dSoo"][1]) if psb_streams else (dSoo_st, None)
            G, e = R.dgq_ref(Z, bn1, s.relu, w, ew, mirrored=psb_streams)
            return check_bound(s.f32("dGq", (g, E, 32, 32)), G, e, "P7 dGq (group, expert, row, column)")
        rec.product("P7", psb + " (fused Gram)" if psb_streams else "k_gram64 (weighted)", p7)
    else:
        assert "k_gram64" not in ran and not psb_streams, ran              # the engine path: Zw = rnd_T(dSoo z') against the stored Zp (moe_backward.cpp:131-136)

        def p7e():
            G, e = R.dgq_engine_ref(Z, bn1, s.relu, s.z("Zp"), ref["dSoo"][0], ref["dSoo"][1], out_bf16=bf16, prod_eps=0.0 if bf16 else 2.0 ** -27)
            return check_bound(s.f32("dGq", (g, E, 32, 32)), G, e, "P7 dGq, engine path (group, expert, row, column)")
        rec.product("P7", psb + " + engine", p7e)
    # ---- P6 -------------------------------------------------------------------------------------------------------------------------
    rec.product("P6", psb + " + " + mdb, lambda: R.check_masked(dzp, *ref["dzp"], f"P6 {rec.shape} {form} final dzp (token, group, expert, entry)"))
    # ---- P8 -------------------------------------------------------------------------------------------------------------------------
    def p8():
        (m3, b3), (m4, b4) = R.dsm34_ref(dzp, Z, bn1)
        return max(check_bound(dsm[3], m3, b3, "P8 dsm[3] = mean dy (group, expert, entry)"), check_bound(dsm[4], m4, b4, "P8 dsm[4] = mean dy zh (group, expert, entry)"))
    rec.product("P8", mdb + " + finalizer", p8)
    # ---- P9 -------------------------------------------------------------------------------------------------------------------------
    rr, mu = s.tokE("rmu")
    dL2x = s.dev("dL2x", s.T, (NT, s.KLp))

    r9 = R.pre_small_bwd_ref(dzp, Z, bn1, dsm[3], dsm[4], rr, mu, s.f32("wsum", (g, E, 32)), s.f32("dconst", (g, E, 32)), cfg.Cx, out_bf16=bf16)

    def p9():
        out = [check_bound(s.z("Zw"), *r9["Zw"], "P9 Zw = dZx (token, group, expert, entry)"),
               check_bound(dL2x[:, s.KL], *r9["dL2x_KL"], "P9 dL2x[:, KL] (token)"),
               check_bound(s.f32("rs2x", (NT,)), *r9["rs2x"], "P9 rs2x (token)")]
        ones = dL2x[:, s.KL + 1].float()
        assert bool((ones == 1.0).all()), f"P9 dL2x[:, KL + 1] != 1 at token {int((ones != 1.0).nonzero()[0])}"
        if not stream:                                                     # tile_fast.hip:817: this expert's own sums, for pre_lat_bwd
            dsl = s.f32("dslat", (s.El, 2, NT))
            out.append(check_bound(dsl[:, 0].t(), r9["dSx"][0][:, :s.El], r9["dSx"][1][:, :s.El], "P9 dslat dSx (token, cross-modal expert)"))
            out.append(check_bound(dsl[:, 1].t(), r9["dSxx"][0][:, :s.El], r9["dSxx"][1][:, :s.El], "P9 dslat dSxx (token, cross-modal expert)"))
        return max(out)
    rec.product("P9", prb, p9)
    # ---- P10: dL2x[:, :KL], the hop-2 block ---------------------------------------------------------------------------------------------
    El = s.El
    TWall = s.f32("TW", (S, s.KL + 2, g, E, 32))
    TW = torch.stack([TWall[:, l * 32:(l + 1) * 32, :, l] for l in range(El)], 1)                    # (S, El, 32, g, 32): slot l's rows, expert l's columns (tile_fast.hip:879)
    Tsum = s.f32("Tsum", (2, S, s.KL + 2))[0][:, :s.KL].reshape(S, El, 32).repeat_interleave(N, 0)
    gv = torch.tensor([float(s.P[f"{p}.gate_av"]) for p in cfg.expert_prefixes()[:El]])
    assert stream or "k_pre_lat_bwd" in ran, ran

    def p10():
        if stream:                                                         # dzraw and the sums stay in fp32 registers (tile_stream.hip:1189, :1202)
            dzr, edzr = r9["dzr"][0][:, :, :El], r9["dzr"][1][:, :, :El]
            (dSx, edSx), (dSxx, edSxx) = ((v[:, :El] for v in r9[k]) for k in ("dSx", "dSxx"))
        else:                                                              # read back as stored: Zw and dslat (tile_fast.hip:903, :907)
            dzr = s.z("Zw")[:, :, :El].double()
            dsl = s.f32("dslat", (El, 2, NT)).double()
            dSx, dSxx = dsl[:, 0].t(), dsl[:, 1].t()
            edzr, edSx, edSxx = torch.zeros_like(dzr), torch.zeros_like(dSx), torch.zeros_like(dSxx)
        ref, bound = R.pre_lat_bwd_ref(s.dev("a", s.T, (El, NT, 32)).permute(1, 0, 2), s.f32("L2", (NT, El, 32)), s.f32("TT", (S, El, 32, 32)), TW, Tsum, gv,
                                       dzr, edzr, dSx, edSx, dSxx, edSxx, cfg.Cx, planes=bf16, out_bf16=bf16)
        # columns KLT..KLp: nobody writes them (the kernels store the El * 32 slot columns and the pair at KL: tile_fast.hip:836-837, :973) and
        # every reader contracts K = KLT columns of rows KLp wide (moe_backward.cpp:37, :263, :300): the contract is "untouched"
        check_untouched(s.dev("dL2x", torch.int16 if bf16 else torch.int32, (NT, s.KLp))[:, s.KL + 2:], -1, "P10 dL2x padding columns KLT..KLp")
        return check_bound(dL2x[:, :s.KL].reshape(NT, El, 32), ref, bound, "P10 dL2x[:, :KL] (token, latent slot, latent token)")
    rec.product("P10", prb if stream else "k_pre_lat_bwd", p10)
    if stream:
        rec.stepped_aside("P9 dslat", prb, "the fused pass keeps the experts' LayerNorm sums in registers (tile_stream.hip:1202)")


@pytest.mark.parametrize("form,shape", CASES)
def test_passes_of_one_site(form, shape):
    from avmoe_amd import _capi
    S, N, M, E_m, E_s = SHAPES[shape]
    hook, bf16 = FORMS[form]
    rec = PassRecorder(shape, form)
    # (Profiled sets HOOK_ALL_FORCE; the nested test_hooks REPLACES the whole mask, so the other force bits -- tok_pair2, dpost_pair, hop-1 --
    # are off in here: none of them chooses a form of these passes, and dApost's form is read off the workspace)
    with Profiled() as prof, _capi.test_hooks(getattr(_capi, hook) if hook else 0):
        s = PassSite(_cfg(N, M, E_m, E_s), S, seed=21, bf16=bf16)
        s.run.forward()
        _forward(s, form, prof.names(), rec)
        s.begin_backward()
        s.part(1)
        _backward(s, form, prof.names(), rec)
        assert s.run.guards_intact(), "a kernel wrote past its workspace"
        assert torch.isfinite(s.run.out.float()).all() and torch.isfinite(s.z("dzp").float()).all() and torch.isfinite(s.z("Zw").float()).all()
    rec.finish()


def test_every_pass_was_checked_in_every_form():
    """Closes the module: each tag was checked against fp64 in each of the three forms, in at least two shapes, one of them ragged -- or
    its step-aside was asserted at every shape of that form where it was not checked.  (Runs after the tests above: it fails when they did not run.)"""
    missing = {}
    for tag in TAGS:
        for form in FORMS:
            got, aside = CHECKED.get((tag, form), {}), ASIDE.get((tag, form), {})
            for sh, ratio in sorted(got.items()):
                print(f"COVERED {tag} {form} {sh} {ratio:.4f}")
            shapes_of_form = [sh for f, sh in CASES if f == form]
            if aside and set(got) | set(aside) == set(shapes_of_form):      # the exception: wherever it was not checked, its step-aside was asserted
                print(f"COVERED {tag} {form} stepped aside at {sorted(aside)}: {sorted(set(aside.values()))}")
                continue
            if len(got) < 2 or not (set(got) & RAGGED):
                missing[(tag, form)] = (TAGS[tag], sorted(got), sorted(aside))
    assert not missing, f"passes not checked in two shapes (one ragged): {missing}"
