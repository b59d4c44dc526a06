"""The per-token bottleneck-space passes in the other two links of every pass's form chain (csrc/pass.h) -- the generalised register-resident
kernels kg_* (csrc/tile_gen.inc: 13 (groups, chunks per group) instances x 3 latent-slot widths, fp32 and bf16) and the any-shape kernels
kt_* / kk_mid (csrc/tile_kernels.hip, fwd_kernels.hip) -- checked ELEMENT BY ELEMENT against fp64 recomputed from the operands exactly as each
kernel read them, with the derived bounds of tests/pass_ref.py, by the method of tests/test_passes_fp64_gpu.py (which does this for the tuned
shape): the forward, then section 1 of the backward (avmoe_moe_backward_part; the whole backward at the site with latent self attention,
which the library does not split), every operand and result read from the named workspace buffers as stored.
tests/test_gen_pass_checker.py shows on the CPU what these checks catch (a padded latent slot left in the softmax, TT read with stride Kp, a
stale round's constants, an idle wave's write, exchanged groups, the odd chunk from the neighbouring expert, a non-zero padding entry, one
tile's mat-vec off by 1 %, one bf16 ulp) and asserts the table of tests/gen_pass_cases.py: which instance and which rounds of resident
experts each case exercises.

Which form ran: the profiler is on; a generalised or any-shape pass opens ONE scope per pass, never named "... (stream)", and neither
k_pre_lat_bwd nor k_pre_bwd_finalize nor k_gram64 (the tuned family's scopes; tests/test_pass_forms_gpu.py).  The two are told apart by
the layout the plan gave the site (tests/gen_pass_cases.py::Layout: entries per group padded to 16 and latent slots to 16 / 32 / 96 with
Z in the site's type, against both padded to 8 with Z in fp32), and every case asserts family and (NG, NCG, KC).  No development switch
is named: the product library has none, and the test hooks are all off.

Checked (the tags, with the meaning they have in tests/test_passes_fp64_gpu.py):
  P1  a = the softmax over the K real latent tokens of each slot of the stored L2; the slots K..Kp EXACTLY 0; the real slots sum to 1 within
      the sum of their bounds; rmu = (rr, mu) from sx, L2, a as stored, TT (indexed with the true K) and Tsum (indexed with Kp).
  P1z z through its defining map, Zx recomputed from X and Wt (block-diagonal where the plan merged the groups).
  P2  bn1 from the stored Z; the padding entries dg..dgp of all four rows exactly 0 (fwd_kernels.hip:988-1019 leaves them 0).
  P3  Zp element-wise = rnd_T(act(z scale + shift)) with the kink mask (kg_mid tile_gen.inc:173-176, kk_mid fwd_kernels.hip:1081-1084), then mz /
      Szz from the stored Zp on the engine path.
  P4  rpmup, Apost's main columns, its 3 E scalar columns from rp / mup as stored, its padding columns KP..KPp untouched (tile_gen.inc:354-358
      and tile_kernels.hip:501-509 store E * dgp + 3 E columns).
  P6  the final dzp = post_small_bwd followed by mid_bwd as one map.
  P7  dGq on the engine path (the only one these forms have).
  P8  dsm[3, 4].
  P9  Zw, dL2x[:, KL], dL2x[:, KL + 1] == 1, rs2x; dslat in the generalised form (the any-shape kernel keeps the sums in registers).
  P10 dL2x[:, :KL]: from Zw and dslat as stored in the generalised form (kg_pre_lat_bwd), from the reference's dzraw and sums with their bounds
      in the any-shape form (one kernel, the values stay in LDS / registers).  The columns of the padding slots K..Kp are WRITTEN, as zero:
      tile_gen.inc:931 leaves d = 0 there, a is exactly 0, so :948 stores du2 * 0 + 0 * (0 - sada); tile_kernels.hip:1002-1007 stores a
      literal 0.  Columns KLT..KLp: written by nobody (untouched).
P5 and gram64 mode do not exist in these forms.  Padding entries dg..dgp of z, Zp, Apost, dzp, Zw: exactly 0 -- z because the padding rows of
Wt and the padding entries of wsum, dconst and TW are 0 (rr (0 + gv 0 - mu 0) + 0), the others because bn1's scale and shift are 0 there
and a ReLU expert masks z' <= 0.  The references compute them from the operands as stored (reference 0, bound 0: exact), and they are
asserted once more by themselves so that the message names the padding.

Each case runs twice and must leave the same bytes in every checked buffer; the guard bands behind both workspaces stay intact.

ReLU kinks: pass_ref.KINK and KINK_CAP = 1e-5 as they are; a tensor may leave out floor(cap x elements) elements, 0 at every case but
many_blocks (16.5 M elements of dzp: 165).  The seeds were chosen on the CPU (tests/test_gen_pass_checker.py keeps the criterion): the
oracle's own fp32 z has no ReLU pre-activation within 16 x the kink window at any case but many_blocks, whose 9.4 M pre-activations put
several into that window at any seed; its seed, the best of 880, keeps the nearest one 6.7 windows away.

NOT covered here: the XR instantiations (N x N and frame-attention experts: sxr, ZR, dZR, dsr); the streaming products around the passes
(tests/test_stream_products_gpu.py).  Every site here runs in training mode with BatchNorm, both LayerNorms and the gate on: the run-time
branches for ln_before, ln_post, use_gate or use_bn off and for eval mode are held per token by tests/test_pass_variants_fp64_gpu.py (at
g2c3_k32_e6, merged_k2 and kt_three_groups_50 of this module's cases).
"""
import time

import pytest
import torch

from oracle import avmoe_oracle as O
from tests import pass_ref as R
from tests.gen_pass_cases import BF16_CASES, CASES, RAGGED, Layout, case_config
from tests.stream_product_ref import ProductMismatch, check_bound, check_untouched, product_bound, product_ref
from tests.test_stream_products_gpu import Profiled, Recorder, Site, _release_device_memory  # noqa: F401  (the fixture: autouse here too)

pytestmark = pytest.mark.gpu

TAGS = {"P1": "pre_small: a (padding slots 0, real slots sum to 1), rmu", "P1z": "pre_small: z through its defining map",
        "P2": "pre_small column sums + k_bn1_finalize: bn1", "P3": "mid: Zp element-wise; mz and Szz from the stored Zp",
        "P4": "post_small: rpmup, Apost main / scalar / padding columns", "P6": "post_small_bwd + mid_bwd: final dzp",
        "P7": "dGq on the engine path", "P8": "mid_bwd column sums + finalizer: dsm[3], dsm[4]",
        "P9": "pre_small_bwd: Zw, dslat, dL2x[:, KL:KL + 2], rs2x", "P10": "pre_lat_bwd / the fused any-shape pass: dL2x[:, :KL]"}
RUNS = [(c, "f32") for c in CASES] + [(c, "bf16") for c in BF16_CASES]
CHECKED = {}      # (tag, dtype) -> {case: worst err / bound}
ASIDE = {}        # (tag, dtype) -> {case: why}
TIMES = {}        # (case, dtype) -> seconds
RAN = {}          # (case, dtype) -> "family (NG, NCG, KC)"
# what the two runs of a case must agree on, byte for byte, at the end of the backward sections that ran
REPEAT = ("Z", "a", "rmu", "bn1", "mz", "Szz", "Apost", "rpmup", "Zp", "dzp", "dsm", "dGq", "Zw", "dL2x", "rs2x")


class GenSite(Site):
    """tests/test_stream_products_gpu.py::Site for any layout, in either element type: every width read off the workspace layout"""

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
        lay = self.lay = Layout(cfg, S, bf16, {n: b for n, (_r, _o, b) in self.run.table.items()})
        self.E, self.N, self.NT = cfg.E, cfg.Nx, S * cfg.Nx
        self.g, self.dg, self.dgp, self.lat, self.El, self.K, self.Kp = lay.g, lay.dg, lay.dgp, lay.lat, lay.El, lay.K, lay.Kp
        self.KL, self.KLT, self.KLp, self.KP, self.KPp, self.XW = lay.KL, lay.KLT, lay.KLp, lay.KP, lay.KPp, lay.XW
        self.zbf = lay.zsz == 2                                            # Z / dzp: the site's type in the generalised form, fp32 in the any-shape form
        self.ZT = torch.bfloat16 if self.zbf else torch.float32
        self.planes = bf16 and lay.family == "tile_gen"                    # mmT_split; kg_*<float> and kt_* run the exact-fp32 pipe
        self.relu = torch.tensor([e < cfg.E_m for e in range(cfg.E)])      # (the cross-modal experts come first and carry the ReLU: net_trans_v3.py:398)
        pfx = cfg.expert_prefixes()
        gname = lambda e: "gate_av" if e < cfg.E_m else "gate_self"        # (latent self attention: PVT_AVSModel_v2.py:144-145)
        self.gv = torch.tensor([float(P[f"{pfx[e]}.{gname(e)}"]) if e in lay.lat else 0.0 for e in range(cfg.E)])

    def z(self, name):
        """a Z-space tensor in the Z type (Z, dzp) as (NT, g, E, dgp): rows are [group][expert][dgp]"""
        return self.dev(name, self.ZT, (self.NT, self.g, self.E, self.dgp))

    def zT(self, name):
        """a Z-space tensor in the site's type (Zp, Zw)"""
        return self.dev(name, self.T, (self.NT, self.g, self.E, self.dgp))

    def tokE(self, name):
        """[r | mu][expert][token] -> two (NT, E) tensors"""
        v = self.f32(name, (2, self.E, self.NT))
        return v[0].t(), v[1].t()

    def latent(self):
        """L2, a (NT, El, Kp); TT (S, El, K, K); TW (S, El, Kp, g, dgp): slot l's rows in its expert's columns; Tsum (NT, El, Kp)"""
        S, N, NT, El, Kp, K = self.S, self.N, self.NT, self.El, self.Kp, self.K
        L2 = self.f32("L2", (NT, El, Kp))                                  # [token][slot][Kp] (tile_gen.inc:586)
        a = self.dev("a", self.T, (El, NT, Kp)).permute(1, 0, 2)           # planes per slot (tile_gen.inc:620)
        TT = self.f32("TT", (S, El, K, K))                                 # the TRUE K (tile_gen.inc:527)
        TWall = self.f32("TW", (S, self.KLT, self.g, self.E, self.dgp))
        TW = torch.stack([TWall[:, l * Kp:(l + 1) * Kp, :, e] for l, e in enumerate(self.lat)], 1)
        Tsum = self.f32("Tsum", (2, S, self.KLT))[0][:, :self.KL].reshape(S, El, Kp).repeat_interleave(N, 0)
        return L2, a, TT, TW, Tsum


class GenRecorder(Recorder):
    """Recorder that files a margin under (tag, dtype) for this module's coverage test"""

    def __init__(self, case, dtype, form):
        super().__init__(case)
        self.dtype, self.form = dtype, form

    def product(self, tag, kernel, fn):
        try:
            ratio = fn()
        except AssertionError as e:
            self.fail.append(f"{tag} [{self.form} {self.dtype}: {kernel}]: {e}")
            return
        CHECKED.setdefault((tag, self.dtype), {})[self.shape] = ratio
        print(f"MARGIN {tag} {self.shape} {self.form} {self.dtype} {kernel} worst_err_over_bound {ratio:.4f}")

    def aside(self, tag, kernel, why):
        self.stepped_aside(tag, kernel, why)
        ASIDE.setdefault((tag, self.dtype), {})[self.shape] = why


def _zero(x, name):
    """padding the kernel text says holds 0 (either sign) holds it"""
    bad = x != 0                                                           # (NaN != 0: the workspace poison shows too)
    if bool(bad.any()):
        raise ProductMismatch(f"{name}: {int(bad.sum())} of {x.numel()} padding elements are not 0, first at {tuple(int(i) for i in bad.nonzero()[0])}")


def _forward(s, ran, rec):
    NT, g, E, S, N, dg, dgp, El, K, Kp = s.NT, s.g, s.E, s.S, s.N, s.dg, s.dgp, s.El, s.K, s.Kp
    bf16, zbf, cfg = s.bf16, s.zbf, s.cfg
    DZ = g * E * dgp
    assert {"k_pre_small", "k_mid", "k_post_small"} <= ran and "k_gram64" not in ran and not any(n.endswith("(stream)") for n in ran), ran
    L2, a, TT, TW, Tsum = s.latent()

    # ---- P1 ----------------------------------------------------------------------------------------------------------------------------
    def p1():
        ref, bound = R.softmax_ref(L2, out_bf16=bf16, K=K)
        _zero(a[..., K:], "P1 a, slots K..Kp (token, latent slot, slot - K)")
        out = [check_bound(a, ref, bound, "P1 a (token, latent slot, latent token)")]
        out.append(check_bound(a[..., :K].double().sum(-1), torch.ones(NT, El, dtype=torch.float64, device=a.device), bound[..., :K].sum(-1),
                               "P1 the real slots of a sum to 1 (token, latent slot)"))
        r = R.rmu_ref(s.f32("sx", (2, NT)), L2, a, TT, Tsum, s.gv, cfg.Cx, cfg.ln_eps, planes=s.planes)
        rr, mu = s.tokE("rmu")
        out += [check_bound(rr, *r["rr"], "P1 rmu[0] = rr (token, expert)"), check_bound(mu, *r["mu"], "P1 rmu[1] = mu (token, expert)")]
        return max(out)
    rec.product("P1", "k_pre_small", p1)
    # ---- P1z ---------------------------------------------------------------------------------------------------------------------------
    Cg = cfg.Cx // g
    X = s.run.X.reshape(NT, g, Cg).permute(1, 0, 2)                        # (g, NT, Cg)
    Wt = s.dev("Wt", s.T, (g, E * dgp, Cg))                                # [group][expert][dgp][c]; one group of block-diagonal rows where merged
    eng = 0.0 if bf16 else 2.0 ** -27                                      # fp32 operands as three bf16 planes, six plane products (DESIGN_CURRENT 3c)

    def p1z():
        Zx, magZ = product_ref(X, Wt.transpose(1, 2))                      # (g, NT, E * dgp): the GEMM's own fp32 sum over Cg terms and its store
        eZ = product_bound(Zx, magZ, out_bf16=zbf, k_terms=Cg) + eng * magZ
        Zx, eZ = (v.reshape(g, NT, E, dgp).permute(1, 0, 2, 3) for v in (Zx, eZ))
        pw, epw = torch.zeros_like(Zx), torch.zeros_like(Zx)
        af = a.reshape(S, N, El, Kp).double()
        for l, e in enumerate(s.lat):                                      # gv * (a . TW): Kp terms (the padding slots are 0 x 0), two planes in kg_*<bf16>
            T = TW[:, l].double()                                          # (S, Kp, g, dgp)
            p, m = (torch.einsum("snk,skic->snic", u, v).reshape(NT, g, dgp) for u, v in ((af[:, :, l], T), (af[:, :, l].abs(), T.abs())))
            pw[:, :, e] = float(s.gv[e]) * p
            epw[:, :, e] = abs(float(s.gv[e])) * (Kp * R.EPS_ACC + (R.EPS_PLANES if s.planes else 0.0)) * m
        rr, mu = s.tokE("rmu")
        ref, bound = R.z_map_ref(Zx, eZ, pw, epw, rr, mu, s.f32("wsum", (g, E, dgp)), s.f32("dconst", (g, E, dgp)), out_bf16=zbf)
        _zero(s.z("Z")[..., dg:], "P1z z, padding entries dg..dgp (token, group, expert, entry - dg)")
        return check_bound(s.z("Z"), ref, bound, "P1z z = LN-folded X Wt^T (token, group, expert, entry)")
    rec.product("P1z", "k_pre_small", p1z)
    # ---- P2 ----------------------------------------------------------------------------------------------------------------------------
    pfx = cfg.expert_prefixes()
    wb = [torch.stack([s.P[f"{p}.bn1.{k}"].reshape(g, dg) for p in pfx], 1).to(s.run.dev) for k in ("weight", "bias")]      # (g, E, dg)
    bn1 = s.f32("bn1", (4, g, E, dgp))

    def p2():
        ref, bound = R.bn1_ref(s.z("Z")[..., :dg], wb[0], wb[1], cfg.bn_eps)
        _zero(bn1[..., dg:], "P2 bn1, padding entries dg..dgp ([mean, rstd, scale, shift], group, expert, entry - dg)")
        return check_bound(bn1[..., :dg], ref, bound, "P2 bn1 ([mean, rstd, scale, shift], group, expert, entry)")
    rec.product("P2", "k_pre_small + k_bn1_finalize", p2)
    # ---- P3 ----------------------------------------------------------------------------------------------------------------------------
    def p3():
        Zp = s.zT("Zp")
        _zp, ezp, y, _ym, kink = R.zprime(s.z("Z"), bn1, s.relu)
        r = s.relu.to(y.device).view(1, 1, -1, 1)
        mask = (~r | (y > 0)).expand_as(y)
        bound = R._store(y, ezp, bf16)
        _zero(Zp[..., dg:], "P3 Zp, padding entries dg..dgp (token, group, expert, entry - dg)")
        out = [R.check_masked(Zp[..., :dg], y[..., :dg], bound[..., :dg], mask[..., :dg], kink.expand_as(y)[..., :dg],
                              f"P3 {rec.shape} {rec.dtype} Zp = rnd_T(act(z scale + shift)) (token, group, expert, entry)")]
        Zd = Zp.double()
        ref = torch.einsum("tgej,tgel->gejl", Zd, Zd) / NT
        mag = torch.einsum("tgej,tgel->gejl", Zd.abs(), Zd.abs()) / NT
        out.append(check_bound(s.f32("Szz", (g, E, dgp, dgp)), ref, ((NT + 2) * R.EPS_ACC + eng) * mag, "P3 Szz = Zp^T Zp / NT (group, expert, row, column)"))
        out.append(check_bound(s.f32("mz", (g, E, dgp)), *R.colsum_ref(Zp, 1.0 / NT), "P3 mz = column means of the stored Zp"))
        return max(out)
    rec.product("P3", "k_mid + engine", p3)
    # ---- P4 ----------------------------------------------------------------------------------------------------------------------------
    uvh = s.f32("uvh", (2 * DZ + 2 * g * E,))
    us, vh = uvh[:DZ].reshape(g, E, dgp), uvh[DZ:2 * DZ].reshape(g, E, dgp)
    H1p, H2p = uvh[2 * DZ:2 * DZ + g * E].reshape(g, E), uvh[2 * DZ + g * E:].reshape(g, E)        # (tile_gen.inc:301)
    qv = s.f32("probs", (S, E)).repeat_interleave(N, 0)                    # the gate lives in weight space; checked, not trusted: the third scalar column is q itself
    rp, mup = s.tokE("rpmup")
    Ap = s.dev("Apost", s.T, (NT, g, s.KPp))

    def p4():
        ref = R.post_small_ref(s.z("Z"), bn1, s.f32("Gq", (g, E, dgp, dgp)), us, vh, H1p, H2p, qv, s.relu, cfg.Cx, cfg.ln_eps, planes=s.planes, out_bf16=bf16)
        main = Ap[:, :, :E * dgp].reshape(NT, g, E, dgp)
        _zero(main[..., dg:], "P4 Apost main columns, padding entries dg..dgp (token, group, expert, entry - dg)")
        out = [check_bound(rp, *ref["rp"], "P4 rpmup[0] = rp (token, expert)"), check_bound(mup, *ref["mup"], "P4 rpmup[1] = mup (token, expert)"),
               check_bound(main, *ref["Apost"], "P4 Apost main columns (token, group, expert, entry)")]
        cr, cb = R.scalar_cols_ref(qv, rp, mup, out_bf16=bf16)
        sc = Ap[:, :, E * dgp:s.KP].reshape(NT, g, E, 3)
        out.append(check_bound(sc, cr[:, None].expand(NT, g, E, 3), cb[:, None].expand(NT, g, E, 3), "P4 Apost scalar columns (token, group, expert, [q rp, -q rp mup, q])"))
        if s.KPp > s.KP:
            check_untouched(s.dev("Apost", torch.int16 if bf16 else torch.int32, (NT, g, s.KPp))[:, :, s.KP:], -1, "P4 Apost padding columns KP..KPp")
        return max(out)
    rec.product("P4", "k_post_small", p4)


def _backward(s, ran, rec):
    NT, g, E, S, N, dg, dgp, El, K, Kp = s.NT, s.g, s.E, s.S, s.N, s.dg, s.dgp, s.El, s.K, s.Kp
    bf16, zbf, cfg = s.bf16, s.zbf, s.cfg
    gen = s.lay.family == "tile_gen"
    assert {"k_post_small_bwd", "k_mid_bwd", "k_pre_small_bwd"} <= ran, ran
    assert not any(n.endswith("(stream)") for n in ran) and not ({"k_pre_lat_bwd", "k_pre_bwd_finalize", "k_gram64"} & ran), ran
    DZ = g * E * dgp
    Z, bn1 = s.z("Z"), s.f32("bn1", (4, g, E, dgp))
    uvh = s.f32("uvh", (2 * DZ + 2 * g * E,))
    us, vh = uvh[:DZ].reshape(g, E, dgp), uvh[DZ:2 * DZ].reshape(g, E, dgp)
    qv = s.f32("probs", (S, E)).repeat_interleave(N, 0)
    rp, mup = s.tokE("rpmup")
    dsm = s.f32("dsm", (8, g, E, dgp))                                     # dusum, dvh, dmz / NT, mdy, mdyz, .. (moe_plan.h:182)
    split = bf16 and gen and not bool(torch.isnan(s.f32("dApx", (NT, g, s.XW))[:, :, :3 * E]).any())
    if split:                                                              # T columns (rows E * dgp wide: tile_gen.inc:394) + fp32 dApx
        dAp = s.dev("dAp", torch.bfloat16, (NT, g, E, dgp))
        dApx = s.f32("dApx", (NT, g, s.XW))[:, :, :3 * E].reshape(NT, g, E, 3)
    else:                                                                  # one fp32 array (NT, g, KPp)
        whole = s.f32("dAp", (NT, g, s.KPp))
        dAp, dApx = whole[:, :, :E * dgp].reshape(NT, g, E, dgp), whole[:, :, E * dgp:s.KP].reshape(NT, g, E, 3)
    print(f"DAPOST {rec.shape} {rec.dtype}: {'split (bf16 + dApx)' if split else 'whole (fp32)'}")
    dzp = s.z("dzp")
    ref = R.post_mid_bwd_ref(dAp, dApx, Z, bn1, s.f32("Gq", (g, E, dgp, dgp)), us, vh, qv, rp, mup, dsm[2], s.f32("sdSzz", (g, E, dgp, dgp)), s.relu, cfg.Cx,
                             planes=s.planes, out_bf16=zbf)

    # ---- P7: the engine contracts Zw = rnd_T(dSoo z') with the stored Zp over the tokens (moe_backward.cpp:131-136) -----------------------
    def p7():
        G, e = R.dgq_engine_ref(Z, bn1, s.relu, s.zT("Zp"), ref["dSoo"][0], ref["dSoo"][1], out_bf16=bf16, prod_eps=0.0 if bf16 else 2.0 ** -27)
        return check_bound(s.f32("dGq", (g, E, dgp, dgp)), G, e, "P7 dGq, engine path (group, expert, row, column)")
    rec.product("P7", "k_post_small_bwd + engine", p7)

    # ---- P6 ----------------------------------------------------------------------------------------------------------------------------
    def p6():
        d2, bound, mask, kink = ref["dzp"]
        _zero(dzp[..., dg:], "P6 dzp, padding entries dg..dgp (token, group, expert, entry - dg)")
        return R.check_masked(dzp[..., :dg], d2[..., :dg], bound[..., :dg], mask.expand_as(d2)[..., :dg], kink.expand_as(d2)[..., :dg],
                              f"P6 {rec.shape} {rec.dtype} final dzp (token, group, expert, entry)")
    rec.product("P6", "k_post_small_bwd + k_mid_bwd", p6)

    # ---- P8 ----------------------------------------------------------------------------------------------------------------------------
    def p8():
        (m3, b3), (m4, b4) = R.dsm34_ref(dzp, Z, bn1)
        return max(check_bound(dsm[3], m3, b3, "P8 dsm[3] = mean dy (group, expert, entry)"), check_bound(dsm[4], m4, b4, "P8 dsm[4] = mean dy zh (group, expert, entry)"))
    rec.product("P8", "k_mid_bwd + finalizer", p8)
    # ---- P9 ----------------------------------------------------------------------------------------------------------------------------
    rr, mu = s.tokE("rmu")
    dL2x = s.dev("dL2x", s.T, (NT, s.KLp))
    r9 = R.pre_small_bwd_ref(dzp, Z, bn1, dsm[3], dsm[4], rr, mu, s.f32("wsum", (g, E, dgp)), s.f32("dconst", (g, E, dgp)), cfg.Cx, out_bf16=bf16)

    def p9():
        Zw = s.zT("Zw")
        _zero(Zw[..., dg:], "P9 Zw, padding entries dg..dgp (token, group, expert, entry - dg)")
        out = [check_bound(Zw, *r9["Zw"], "P9 Zw = dZx (token, group, expert, entry)"),
               check_bound(dL2x[:, s.KL], *r9["dL2x_KL"], "P9 dL2x[:, KL] (token)"),
               check_bound(s.f32("rs2x", (NT,)), *r9["rs2x"], "P9 rs2x (token)")]
        ones = dL2x[:, s.KL + 1].float()
        assert bool((ones == 1.0).all()), f"P9 dL2x[:, KL + 1] != 1 at token {int((ones != 1.0).nonzero()[0])}"
        if gen:                                                            # tile_gen.inc:802: the experts with a latent slot leave their own sums for kg_pre_lat_bwd
            dsl = s.f32("dslat", (El, 2, NT))
            out.append(check_bound(dsl[:, 0].t(), r9["dSx"][0][:, s.lat], r9["dSx"][1][:, s.lat], "P9 dslat dSx (token, latent slot)"))
            out.append(check_bound(dsl[:, 1].t(), r9["dSxx"][0][:, s.lat], r9["dSxx"][1][:, s.lat], "P9 dslat dSxx (token, latent slot)"))
        return max(out)
    rec.product("P9", "k_pre_small_bwd", p9)
    if not gen:
        rec.stepped_aside("P9 dslat", "k_pre_small_bwd", "the any-shape kernel keeps the experts' LayerNorm sums in registers (tile_kernels.hip:915-931)")
    # ---- P10 ---------------------------------------------------------------------------------------------------------------------------
    L2, a, TT, TW, Tsum = s.latent()
    gvl = s.gv[s.lat]

    def p10():
        if gen:                                                            # kg_pre_lat_bwd reads them back as stored: Zw and dslat (tile_gen.inc:886, :893)
            dzr = s.zT("Zw")[:, :, s.lat].double()
            dsl = s.f32("dslat", (El, 2, NT)).double()
            dSx, dSxx = dsl[:, 0].t(), dsl[:, 1].t()
            edzr, edSx, edSxx = torch.zeros_like(dzr), torch.zeros_like(dSx), torch.zeros_like(dSxx)
        else:                                                              # one kernel: dzraw in the wave's LDS tile, the sums in registers (tile_kernels.hip:909, :967)
            dzr, edzr = r9["dzr"][0][:, :, s.lat], r9["dzr"][1][:, :, s.lat]
            (dSx, edSx), (dSxx, edSxx) = ((v[:, s.lat] for v in r9[k]) for k in ("dSx", "dSxx"))
        ref10, bound10 = R.pre_lat_bwd_ref(a, L2, TT, TW, Tsum, gvl, dzr, edzr, dSx, edSx, dSxx, edSxx, cfg.Cx, planes=s.planes, out_bf16=bf16)
        got = dL2x[:, :s.KL].reshape(NT, El, Kp)
        _zero(got[..., K:], "P10 dL2x[:, :KL], columns of the padding slots K..Kp (token, latent slot, slot - K)")
        if s.KLp > s.KLT:
            check_untouched(s.dev("dL2x", torch.int16 if bf16 else torch.int32, (NT, s.KLp))[:, s.KLT:], -1, "P10 dL2x padding columns KLT..KLp")
        return check_bound(got, ref10, bound10, "P10 dL2x[:, :KL] (token, latent slot, latent token)")
    rec.product("P10", "k_pre_small_bwd (kg_pre_lat_bwd)" if gen else "k_pre_small_bwd", p10)


def _run(case, bf16):
    cfg, S, seed, _family, _inst = case_config(case)
    s = GenSite(cfg, S, seed=seed, bf16=bf16)
    s.run.forward()
    return s


@pytest.mark.parametrize("case,dtype", RUNS)
def test_passes_of_one_site(case, dtype):
    from avmoe_amd import _capi
    t0 = time.time()
    bf16 = dtype == "bf16"
    cfg, _S, _seed, family, inst = case_config(case)
    # Section 1 alone, except with latent self attention: such a site accumulates into dX to the end and the library serves its backward whole
    # only (moe_backward.cpp:59).  What is read here survives the later sections: they read Zw, dL2x and rs2x as operands (moe_backward.cpp:32-37,
    # :152, :263, :299) and touch none of the other buffers, and no two buffers of the workspace share bytes (asserted below).
    parts = 7 if cfg.self_attn == "v2" else 1
    # (Profiled sets the force bits of the streamed products; the nested test_hooks REPLACES the whole mask with 0: every choice is the product's own)
    with Profiled() as prof, _capi.test_hooks(0):
        s = _run(case, bf16)
        assert (s.lay.family, s.lay.instance) == (family, inst), f"{case}: the plan chose {s.lay.family} {s.lay.instance}, the case is meant for {family} {inst}"
        form = family if inst is None else f"{family} {inst}"
        RAN[(case, dtype)] = form
        print(f"\nINSTANCE {case} {dtype}: {form}, g {s.g} (merged {s.lay.merged}), dgp {s.dgp} (dg {s.dg}), Kp {s.Kp} (K {s.K}), {s.lay.blocks} blocks of {s.lay.per} tokens")
        rec = GenRecorder(case, dtype, form)
        _forward(s, prof.names(), rec)
        if parts != 1:
            for region in (0, 1):
                iv = sorted((o, o + b, n) for n, (r, o, b) in s.run.table.items() if r == region and b > 0)
                assert all(x[1] <= y[0] for x, y in zip(iv, iv[1:])), f"workspace buffers overlap: {[(x[2], y[2]) for x, y in zip(iv, iv[1:]) if x[1] > y[0]]}"
        s.begin_backward()
        s.part(parts)
        _backward(s, prof.names(), rec)
        assert s.run.guards_intact(), "a kernel wrote past its workspace"
        assert torch.isfinite(s.run.out.float()).all() and torch.isfinite(s.z("dzp").float()).all() and torch.isfinite(s.zT("Zw").float()).all()
        # ---- the same bytes twice ----
        again = _run(case, bf16)
        again.begin_backward()
        again.part(parts)
        for name in REPEAT + (("dslat",) if family == "tile_gen" else ()):
            _r, _o, nb = s.run.table[name]
            x, y = s.dev(name, torch.uint8, (nb,)), again.dev(name, torch.uint8, (nb,))
            assert torch.equal(x, y), f"{name}: {int((x != y).sum())} of {nb} bytes differ between two runs of the same site"
        assert again.run.guards_intact(), "a kernel wrote past its workspace (second run)"
    TIMES[(case, dtype)] = time.time() - t0
    print(f"TIME   {case} {dtype} {TIMES[(case, dtype)]:.2f} s")
    rec.finish()


def test_every_pass_was_checked_at_every_case():
    """Closes the module: every tag x dtype x case was checked against fp64, or its step-aside was recorded with a reason.  (Runs after the
    tests above: it fails when they did not run.)"""
    missing = []
    for tag in TAGS:
        for case, dtype in RUNS:
            if case in CHECKED.get((tag, dtype), {}):
                print(f"COVERED {tag} {dtype} {case} {RAN.get((case, dtype))} {CHECKED[(tag, dtype)][case]:.4f}")
            elif case in ASIDE.get((tag, dtype), {}):
                print(f"COVERED {tag} {dtype} {case} stepped aside: {ASIDE[(tag, dtype)][case]}")
            else:
                missing.append((tag, dtype, case))
    for (case, dtype), t in TIMES.items():
        print(f"TIME   {case} {dtype} {t:.2f} s")
    print(f"TIME   module {sum(TIMES.values()):.2f} s over {len(TIMES)} cases")
    assert not missing, f"not checked and no reason recorded: {missing}"
    assert RAGGED & {c for c, _d in RUNS}
