"""The per-token bottleneck-space passes with a switch OFF or in EVAL mode, checked ELEMENT BY ELEMENT against fp64 recomputed from the operands
exactly as each kernel read them, by the method and with the helpers of tests/test_passes_fp64_gpu.py and tests/test_gen_passes_fp64_gpu.py
(which hold every site in training mode with BatchNorm, both LayerNorms and the gate on).  ln_before, ln_post, use_gate, use_bn and training
are RUN-TIME branches inside every form of every pass; tests/pass_ref.py carries one argument per branch, its roundings counted from the
kernel text, and tests/test_pass_checker.py shows on the CPU what these checks catch (the eval backward keeping the batch-mean terms, eval
bn1 from the batch statistics or without eps, scale = w without BatchNorm, a stale rr, rp from a LayerNorm that is off, a gate applied with
the gate off or twice, a non-zero rs2x, a neighbouring expert's running mean, one bf16 ulp, a running statistic changed by an eval forward).

Seven variants (tests/pass_variant_cases.py) at ten sites, all four forms of every pass: kfs_* (csrc/tile_stream.hip), kf_*<bf16> and
kf_*<float> (tile_fast.hip), kg_* (tile_gen.inc, fp32 and bf16), kt_* / kk_mid (tile_kernels.hip, fwd_kernels.hip).  The forward, then section 1
of the backward (avmoe_moe_backward_part), every operand and result read from the named workspace buffers as stored; one Recorder per
site, so a run reports every failing tag.  The profiler is on and the scope names assert which form ran; family and instance are asserted
from the layout the plan gave the site (no switch reaches the plan: moe_plan.cpp:126-130, :175-182).

What each switch does to the STORED buffers, as read from the kernels and the host code and asserted here (the tags have the meaning they
have in the two train-mode modules):
  P1  a: unchanged by every switch.  rmu: ALL FOUR forms store it unconditionally (tile_fast.hip:667, tile_stream.hip:977, tile_gen.inc:670,
      tile_kernels.hip:373); with ln_before off it is exactly (1, 0).
  P1z z = rnd_T(Zx + gv a . TW) with ln_before off (the `: zr` arm): two fp32 operations, no wsum / dconst term.
  P2  bn1: eval = (running_mean, rsqrtf(running_var + eps), w rstd, b - mean scale) from the buffers AS UPLOADED; no BatchNorm = exactly
      (0, 1, 1, 0); the padding entries dg..dgp exactly 0 in every mode (fwd_kernels.hip:1041-1075).
  P3  Zp = rnd_T(act(z scale + shift)) wherever k_mid runs (every site outside gram64 mode: moe_forward.cpp:250), mz = its column means
      (fwd_kernels.hip:1206: in every mode).  Szz is written only in train mode with BatchNorm (moe_forward.cpp:251, :256): otherwise
      UNTOUCHED -- and in gram64 mode (the tuned bf16 shape with 2 or 4 experts; the plan's choice reads neither switch, moe_plan.cpp:176)
      neither k_mid nor k_gram64 runs then, so mz is untouched too and no Zp exists: no value to compare, so those sites file P3 as a
      step-aside whose contract (both buffers still hold the poison) is asserted, and the other forms check it.
  P4  rpmup = (1, 0) exactly and Apost = rnd_T(q z') with ln_post off; the scalar columns [q, -0, q]: the middle one is a NEGATIVE zero in
      both element types ((-q * 1) * 0), asserted as a bit pattern.  The gate: every site's plan folds it into Bpost (Dims::gate_w,
      moe_plan.cpp:35; the launchers pass use_gate && !gate_w), so q = probs with the gate on AND off, and the third scalar column -- q
      itself -- shows which arm ran: it is compared with probs as stored (bound: the store alone).  The token-space arm of the kernels
      (a.use_gate: q = probs * gate) runs only under the development switch that clears gate_w (sw.gate_token), which the product
      library never sets and no test hook reaches: it stays UNEXERCISED here.  What is held is that no variant takes it.
  P5  dSooT (register-resident bf16 form in gram64 mode only): dSoo, or exactly 0 with ln_post off (tile_fast.hip:459, :497).
  P6  the final dzp: without moments (a.moments = use_bn && training) mid_bwd adds two literal zeros; with ln_post off dz' = q dAp.
  P7  dGq: with ln_post on it arrives by the path the plan's gram64 flag chooses, in every mode (moe_backward.cpp:123-133: fused into the
      streamed post_small_bwd, k_gram64 from dSooT, or the engine on Zw x Zp); with ln_post off none of the three runs: UNTOUCHED in
      every form -- that contract is all there is to check, and it is filed as the check.
  P8  dsm[3, 4]: every form accumulates the two column sums and the finalizer stores them in EVERY mode (tile_fast.hip:156,
      tile_stream.hip:552, bwd_kernels.hip:72-73) with zh from bn1 as stored -- only pre_small_bwd stops READING them (bn_train).
  P9  Zw = rnd_T(scale dy) in eval, rnd_T(dy) without BatchNorm, no product with rr when ln_before is off; then dL2x[:, KL] == 0,
      dL2x[:, KL + 1] == 1, rs2x == 0 exactly.  dslat: the register-resident forms (kf_*, kg_*) store it for the experts with a latent
      slot -- exact zeros with ln_before off (tile_fast.hip:798-817, tile_gen.inc:791-802); the streamed and the any-shape form never write
      it (tile_stream.hip:1202, tile_kernels.hip:929: the sums stay in LDS / registers): UNTOUCHED there, asserted against the poison.
  P10 dL2x[:, :KL] from the same operands (with ln_before off the LayerNorm sums it reads are the zeros above).

Which kernel ran, from the profiler scopes: no k_gram64 scope in a forward without train-mode BatchNorm; k_mid exactly outside gram64
mode.  The streamed post_small_bwd needs Dims::gram64 and the split dApost (tile_stream.hip:1467), NOT train-mode BatchNorm: gram64 is a
property of shape and type, so at the two streamed sites it carries "(stream)" in every variant, eval included, and with ln_post on its
fused Gram product leaves dGq (moe_backward.cpp:123); the register-resident bf16 site takes k_gram64 from dSooT (:125) and three experts /
fp32 / the other families the engine (:128) -- in eval and without BatchNorm as in training.  pre_small streams only with the fused hop-2
logits (Dims::fuse_l2: four experts, >= 2 frames of >= 64 tokens): at stream_short_20 the register-resident kernel runs under
HOOK_KFS_FORCE and the step-aside is recorded.

State: after an eval forward, and in train mode without BatchNorm, every BatchNorm running mean, running variance and
num_batches_tracked of the site is bit-identical to what was uploaded.  Each site runs twice and leaves the same bytes in every checked
buffer; the guard bands stay intact.

ReLU kinks: pass_ref.KINK and KINK_CAP = 1e-5 as they are; the largest checked tensor has 1 003 520 elements, so no element may be left out.

NOT covered here: the XR instantiations (N x N and frame-attention experts); the weight-space kernels (read only as stored operands);
cumulative BatchNorm (tests/test_bn_cumulative_gpu.py)."""
import time
from types import SimpleNamespace

import pytest
import torch

from oracle import avmoe_oracle as O
from tests import pass_ref as R
from tests.gen_pass_cases import Layout
from tests.pass_variant_cases import RAGGED, SITES, VARIANTS, site_config
from tests.stream_product_ref import ProductMismatch, check_bound, check_untouched, product_bound, product_ref
from tests.test_stream_products_gpu import Profiled, Recorder, Site, _release_device_memory  # noqa: F401  (the fixture: autouse here too)

pytestmark = pytest.mark.gpu

TAGS = {"P1": "pre_small: a, rmu", "P1z": "pre_small: z through its defining map", "P2": "k_bn1_finalize: bn1 in the variant's BatchNorm mode",
        "P3": "mid: Zp, mz; Szz written or untouched", "P4": "post_small: rpmup, Apost main / scalar / padding columns",
        "P5": "post_small_bwd: dSooT", "P6": "post_small_bwd + mid_bwd: final dzp", "P7": "dGq: its path, or untouched",
        "P8": "mid_bwd column sums + finalizer: dsm[3], dsm[4]", "P9": "pre_small_bwd: Zw, dslat, dL2x[:, KL:KL + 2], rs2x",
        "P10": "pre_lat_bwd / the fused passes: dL2x[:, :KL]"}
RUNS = [(site, variant) for site in SITES for variant in VARIANTS]
CHECKED = {}      # (tag, variant) -> {site: worst err / bound}
ASIDE = {}        # (tag, variant) -> {site: why}
TIMES = {}        # (site, variant) -> seconds


def _ru(x, m):
    return -(-x // m) * m


class VarSite(Site):
    """tests/test_stream_products_gpu.py::Site for any layout, element type and mode: every width read off the workspace layout, the
    BatchNorm buffers kept (self.B, as uploaded) and the int64 counters uploaded too"""

    def __init__(self, site, variant):
        self.form, _what, bf16, _hook = SITES[site]
        cfg, S, seed, training, family, inst = site_config(site, variant)
        self.make_run(cfg, S, seed, training=training, bf16=bf16, counters=True)
        r, P = self.run, self.P
        nbytes = {n: b for n, (_r, _o, b) in r.table.items()}
        E, NT = cfg.E, S * cfg.Nx
        if family == "tuned":                                              # bottleneck 64 in 2 groups, 32 latent tokens: tile_fast.hip / tile_stream.hip
            esz = 2 if bf16 else 4
            lay = SimpleNamespace(family="tuned", instance=None, merged=False, g=2, dg=32, dgp=nbytes["wsum"] // 4 // (E * 2), lat=list(range(cfg.E_m)),
                                  El=cfg.E_m, K=32, Kp=nbytes["a"] // (cfg.E_m * NT * esz), zsz=nbytes["Z"] // (NT * E * 2 * 32))
            assert (lay.dgp, lay.Kp, lay.zsz) == (32, 32, esz), f"{site} {variant}: not the tuned layout ({lay.dgp}, {lay.Kp}, {lay.zsz})"
            lay.KL = lay.El * lay.Kp
            lay.KLT, lay.KLp, lay.KP = lay.KL + 2, _ru(lay.KL + 2, 8), E * 32 + 3 * E
            lay.KPp = _ru(lay.KP, 8)
            lay.XW = _ru(lay.KPp - E * 32, 16)
        else:
            lay = Layout(cfg, S, bf16, nbytes)
            assert (lay.family, lay.instance) == (family, inst), f"{site} {variant}: the plan chose {lay.family} {lay.instance}, the site is meant for {family} {inst}"
        self.lay = lay
        self.E, self.N, self.NT = E, cfg.Nx, NT
        self.g, self.dg, self.dgp, self.lat, self.El, self.K, self.Kp = lay.g, lay.dg, lay.dgp, lay.lat, lay.El, lay.K, lay.Kp
        self.KL, self.KLT, self.KLp, self.KP, self.KPp, self.XW = lay.KL, lay.KLT, lay.KLp, lay.KP, lay.KPp, lay.XW
        self.zbf = lay.zsz == 2                                            # Z / dzp: the site's type in the register-resident forms, fp32 in the any-shape form
        self.ZT = torch.bfloat16 if self.zbf else torch.float32
        self.planes = bf16 and lay.family != "tile_kernels"                # mmT_split / mm_presplit; kf_*<float>, kg_*<float> and kt_* run the exact-fp32 pipe
        self.gram64 = lay.family == "tuned" and bf16 and E in (2, 4)       # moe_plan.cpp:176
        self.relu = torch.tensor([e < cfg.E_m for e in range(E)])          # (the cross-modal experts come first and carry the ReLU)
        pfx = cfg.expert_prefixes()
        gname = lambda e: "gate_av" if e < cfg.E_m else "gate_self"
        self.gv = torch.tensor([float(P[f"{pfx[e]}.{gname(e)}"]) if e in lay.lat else 0.0 for e in range(E)])
        self.v = SimpleNamespace(ln_before=cfg.ln_before, ln_post=cfg.ln_post, use_gate=cfg.use_gate, use_bn=cfg.use_bn, training=training,
                                 moments=cfg.use_bn and training, bn="off" if not cfg.use_bn else ("train" if training else "eval"))

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
        L2 = self.f32("L2", (NT, El, Kp))
        a = self.dev("a", self.T, (El, NT, Kp)).permute(1, 0, 2)
        TT = self.f32("TT", (S, El, K, K))
        TWall = self.f32("TW", (S, self.KLT, self.g, self.E, self.dgp))
        TW = torch.stack([TWall[:, l * Kp:(l + 1) * Kp, :, e] for l, e in enumerate(self.lat)], 1)
        Tsum = self.f32("Tsum", (2, S, self.KLT))[0][:, :self.KL].reshape(S, El, Kp).repeat_interleave(N, 0)
        return L2, a, TT, TW, Tsum

    def raw(self, name):
        """every byte of a buffer"""
        _r, _o, nb = self.run.table[name]
        return self.dev(name, torch.uint8, (nb,))

    def poisoned(self, name, what):
        """no kernel wrote the buffer: every byte still holds the workspace poison"""
        check_untouched(self.raw(name).view(torch.int8), -1, what)

    def bn_stat(self, leaf):
        """a BatchNorm-1 buffer of every expert AS UPLOADED, (g, E, dg)"""
        return torch.stack([self.B[f"{p}.bn1.{leaf}"].reshape(self.g, self.dg) for p in self.cfg.expert_prefixes()], 1).to(self.run.dev)


class VarRecorder(Recorder):
    """Recorder that files a margin under (tag, variant) for this module's coverage test"""

    def __init__(self, site, variant, form):
        super().__init__(site)
        self.variant, self.form = variant, form

    def product(self, tag, kernel, fn):
        try:
            ratio = fn()
        except AssertionError as e:
            self.fail.append(f"{tag} [{self.variant} {self.form}: {kernel}]: {e}")
            return
        CHECKED.setdefault((tag, self.variant), {})[self.shape] = ratio
        print(f"MARGIN {tag} {self.variant} {self.form} {self.shape} {kernel} worst_err_over_bound {ratio:.4f}")

    def aside(self, tag, kernel, why):
        self.stepped_aside(f"{tag} {self.variant}", kernel, why)
        ASIDE.setdefault((tag, self.variant), {})[self.shape] = why

    def check(self, what, ok, msg=""):
        """a condition on which kernel ran or on a buffer's contract: recorded like a mismatch, so the other tags of the site are still tried"""
        if not ok:
            self.fail.append(f"{what} [{self.variant} {self.form}]: {msg}")


def _zero(x, name):
    """padding the kernel text says holds 0 (either sign) holds it"""
    bad = x != 0                                                           # (NaN != 0: the workspace poison shows too)
    if bool(bad.any()):
        raise ProductMismatch(f"{name}: {int(bad.sum())} of {x.numel()} elements are not 0, first at {tuple(int(i) for i in bad.nonzero()[0])}")


def _exact(x, value, name):
    bad = x != value
    if bool(bad.any()):
        i = tuple(int(k) for k in bad.nonzero()[0])
        raise ProductMismatch(f"{name}: {int(bad.sum())} of {x.numel()} elements are not {value}, first {float(x[i])!r} at {i}")


def _forward(s, ran, rec):
    NT, g, E, S, N, dg, dgp, El, K, Kp = s.NT, s.g, s.E, s.S, s.N, s.dg, s.dgp, s.El, s.K, s.Kp
    bf16, zbf, cfg, v, form = s.bf16, s.zbf, s.cfg, s.v, s.form
    tuned = s.lay.family == "tuned"
    DZ = g * E * dgp
    # ---- which kernels ran ----------------------------------------------------------------------------------------------------------------
    rec.check("forward scopes", ("k_gram64" in ran) == (s.gram64 and v.moments),
              f"k_gram64 runs exactly in gram64 mode with train-mode BatchNorm (moe_forward.cpp:251): {sorted(ran)}")
    rec.check("forward scopes", ("k_mid" in ran) == (not s.gram64), f"k_mid runs exactly outside gram64 mode (moe_forward.cpp:250): {sorted(ran)}")
    pre_streams = "k_pre_small (stream)" in ran
    rec.check("forward scopes", ("k_pre_small" in ran) == (not pre_streams), f"{sorted(ran)}")
    if form == "stream":
        rec.check("forward scopes", "k_post_small (stream)" in ran and "k_post_small" not in ran, f"post_small did not stream: {sorted(ran)}")
        # the streamed pre_small wants the fused hop-2 logits, Dims::fuse_l2 (moe_plan.cpp:181): E * dgp == 128, >= 2 frames, >= 64 tokens per frame
        rec.check("forward scopes", pre_streams == (E == 4 and S >= 2 and N >= 64), f"{sorted(ran)}")
    else:
        rec.check("forward scopes", not any(n.endswith("(stream)") for n in ran) and "k_post_small" in ran, f"{sorted(ran)}")
    pre_checked = form != "stream" or pre_streams      # (under "stream" the register-resident pre_small is NOT filed: the "fast" site checks it)
    if not pre_checked:
        for tag in ("P1", "P1z", "P2"):
            rec.aside(tag, "k_pre_small (stream)", "no fused hop-2 logits (fewer than 64 tokens per frame): the register-resident pre_small ran")
    pre_name = "k_pre_small (stream)" if pre_streams else "k_pre_small"
    L2, a, TT, TW, Tsum = s.latent()

    # ---- P1 ----------------------------------------------------------------------------------------------------------------------------
    def p1():
        ref, bound = R.softmax_ref(L2, out_bf16=bf16, K=K)
        _zero(a[..., K:], "P1 a, slots K..Kp (token, latent slot, slot - K)")
        out = [check_bound(a, ref, bound, "P1 a (token, latent slot, latent token)")]
        r = R.rmu_ref(s.f32("sx", (2, NT)), L2, a, TT, Tsum, s.gv, cfg.Cx, cfg.ln_eps, planes=s.planes, ln_before=v.ln_before)
        rr, mu = s.tokE("rmu")
        out += [check_bound(rr, *r["rr"], "P1 rmu[0] = rr (token, expert)"), check_bound(mu, *r["mu"], "P1 rmu[1] = mu (token, expert)")]
        return max(out)
    if pre_checked:
        rec.product("P1", pre_name, p1)
    # ---- P1z ---------------------------------------------------------------------------------------------------------------------------
    Cg = cfg.Cx // g
    X = s.run.X.reshape(NT, g, Cg).permute(1, 0, 2)                        # (g, NT, Cg)
    Wt = s.dev("Wt", s.T, (g, E * dgp, Cg))                                # [group][expert][dgp][c]; one group of block-diagonal rows where merged
    eng = 0.0 if bf16 else 2.0 ** -27                                      # fp32 operands as three bf16 planes, six plane products (DESIGN_CURRENT 3c)

    def p1z():
        Zx, magZ = product_ref(X, Wt.transpose(1, 2))                      # (g, NT, E * dgp): the GEMM's own fp32 sum over Cg terms and its store
        eZ = product_bound(Zx, magZ, out_bf16=zbf, k_terms=Cg) + eng * magZ
        Zx, eZ = (t.reshape(g, NT, E, dgp).permute(1, 0, 2, 3) for t in (Zx, eZ))
        pw, epw = torch.zeros_like(Zx), torch.zeros_like(Zx)
        af = a.reshape(S, N, El, Kp).double()
        for l, e in enumerate(s.lat):                                      # gv * (a . TW): Kp terms, two planes in the bf16 register-resident and streamed forms
            T = TW[:, l].double()                                          # (S, Kp, g, dgp)
            p, m = (torch.einsum("snk,skic->snic", u, w).reshape(NT, g, dgp) for u, w in ((af[:, :, l], T), (af[:, :, l].abs(), T.abs())))
            pw[:, :, e] = float(s.gv[e]) * p
            epw[:, :, e] = abs(float(s.gv[e])) * (Kp * R.EPS_ACC + (R.EPS_PLANES if s.planes else 0.0)) * m
        rr, mu = s.tokE("rmu")
        ref, bound = R.z_map_ref(Zx, eZ, pw, epw, rr, mu, s.f32("wsum", (g, E, dgp)), s.f32("dconst", (g, E, dgp)), out_bf16=zbf, ln_before=v.ln_before)
        _zero(s.z("Z")[..., dg:], "P1z z, padding entries dg..dgp (token, group, expert, entry - dg)")
        return check_bound(s.z("Z"), ref, bound, "P1z z through its defining map (token, group, expert, entry)")
    if pre_checked:
        rec.product("P1z", pre_name, p1z)
    # ---- P2 ----------------------------------------------------------------------------------------------------------------------------
    pfx = cfg.expert_prefixes()
    if v.use_bn:
        wb = [torch.stack([s.P[f"{p}.bn1.{k}"].reshape(g, dg) for p in pfx], 1).to(s.run.dev) for k in ("weight", "bias")]      # (g, E, dg)
    else:                                                                  # (a site without BatchNorm has no such parameters: only their shape is read)
        wb = [torch.zeros(g, E, dg, device=s.run.dev)] * 2
    bn1 = s.f32("bn1", (4, g, E, dgp))

    def p2():
        rm, rv = (s.bn_stat("running_mean"), s.bn_stat("running_var")) if v.bn == "eval" else (None, None)
        ref, bound = R.bn1_ref(s.z("Z")[..., :dg], wb[0], wb[1], cfg.bn_eps, mode=v.bn, rm=rm, rv=rv)
        _zero(bn1[..., dg:], "P2 bn1, padding entries dg..dgp ([mean, rstd, scale, shift], group, expert, entry - dg)")
        return check_bound(bn1[..., :dg], ref, bound, f"P2 bn1, BatchNorm mode '{v.bn}' ([mean, rstd, scale, shift], group, expert, entry)")
    if pre_checked:
        rec.product("P2", pre_name + " + k_bn1_finalize", p2)
    # ---- state: a forward that does not train BatchNorm leaves every running statistic and counter as uploaded ------------------------------
    if not v.moments:
        r = s.run
        for k, up in s.B.items():
            try:
                R.state_unchanged(r.buffers[k] if up.is_floating_point() else r.nbt[k], up, f"state {k} (BatchNorm mode '{v.bn}')")
            except AssertionError as e:
                rec.fail.append(f"state [{rec.variant} {form}]: {e}")
    # ---- P3 ----------------------------------------------------------------------------------------------------------------------------
    if s.gram64 and v.moments:                                             # z' formed on the fly in bf16, one pass (moe_forward.cpp:254)
        def p3g():
            ref = R.gram_ref(s.z("Z"), bn1, s.relu)
            return max(check_bound(s.f32("mz", (g, E, 32)), *ref["mz"], "P3 mz (group, expert, entry)"),
                       check_bound(s.f32("Szz", (g, E, 32, 32)), *ref["Szz"], "P3 Szz (group, expert, row, column)"))
        rec.product("P3", "k_gram64", p3g)
    elif s.gram64:                                                         # neither k_mid nor k_gram64: no Zp, mz and Szz as the workspace arrived
        try:                                                               # a step-aside, asserted: no value exists to compare (the other forms check P3)
            s.poisoned("mz", "P3 mz (gram64 mode without train-mode BatchNorm: nobody writes it)")
            s.poisoned("Szz", "P3 Szz (gram64 mode without train-mode BatchNorm: nobody writes it)")
            rec.aside("P3", "k_gram64", "gram64 mode without train-mode BatchNorm: neither k_mid nor k_gram64 runs (moe_forward.cpp:250-251); mz and Szz untouched")
        except AssertionError as e:
            rec.fail.append(f"P3 [{rec.variant} {form}]: {e}")
    else:
        def p3():
            Zp = s.zT("Zp")
            _zp, ezp, y, _ym, kink = R.zprime(s.z("Z"), bn1, s.relu)
            r = s.relu.to(y.device).view(1, 1, -1, 1)
            mask = (~r | (y > 0)).expand_as(y)
            bound = R._store(y, ezp, bf16)
            _zero(Zp[..., dg:], "P3 Zp, padding entries dg..dgp (token, group, expert, entry - dg)")
            out = [R.check_masked(Zp[..., :dg], y[..., :dg], bound[..., :dg], mask[..., :dg], kink.expand_as(y)[..., :dg],
                                  f"P3 {rec.shape} {rec.variant} Zp = rnd_T(act(z scale + shift)) (token, group, expert, entry)")]
            out.append(check_bound(s.f32("mz", (g, E, dgp)), *R.colsum_ref(Zp, 1.0 / NT), "P3 mz = column means of the stored Zp"))
            if v.moments:
                Zd = Zp.double()
                ref = torch.einsum("tgej,tgel->gejl", Zd, Zd) / NT
                mag = torch.einsum("tgej,tgel->gejl", Zd.abs(), Zd.abs()) / NT
                out.append(check_bound(s.f32("Szz", (g, E, dgp, dgp)), ref, ((NT + 2) * R.EPS_ACC + eng) * mag, "P3 Szz = Zp^T Zp / NT (group, expert, row, column)"))
            else:
                s.poisoned("Szz", "P3 Szz (no train-mode BatchNorm: moe_forward.cpp:256 does not launch the product)")
            return max(out)
        rec.product("P3", "k_mid" + (" + engine" if v.moments else ""), p3)
    # ---- P4 ----------------------------------------------------------------------------------------------------------------------------
    uvh = s.f32("uvh", (2 * DZ + 2 * g * E,))
    us, vh = uvh[:DZ].reshape(g, E, dgp), uvh[DZ:2 * DZ].reshape(g, E, dgp)
    H1p, H2p = uvh[2 * DZ:2 * DZ + g * E].reshape(g, E), uvh[2 * DZ + g * E:].reshape(g, E)
    qv = s.f32("probs", (S, E)).repeat_interleave(N, 0)                    # gate_w: the gate lives in weight space, on or off (checked: the third scalar column is q itself)
    rp, mup = s.tokE("rpmup")
    Ap = s.dev("Apost", s.T, (NT, g, s.KPp))

    def p4():
        ref = R.post_small_ref(s.z("Z"), bn1, s.f32("Gq", (g, E, dgp, dgp)), us, vh, H1p, H2p, qv, s.relu, cfg.Cx, cfg.ln_eps, planes=s.planes, out_bf16=bf16,
                               ln_post=v.ln_post)
        main = Ap[:, :, :E * dgp].reshape(NT, g, E, dgp)
        _zero(main[..., dg:], "P4 Apost main columns, padding entries dg..dgp (token, group, expert, entry - dg)")
        out = [check_bound(rp, *ref["rp"], "P4 rpmup[0] = rp (token, expert)"), check_bound(mup, *ref["mup"], "P4 rpmup[1] = mup (token, expert)"),
               check_bound(main, *ref["Apost"], "P4 Apost main columns (token, group, expert, entry)")]
        cr, cb = R.scalar_cols_ref(qv, rp, mup, out_bf16=bf16, ln_post=v.ln_post)
        sc = Ap[:, :, E * dgp:s.KP].reshape(NT, g, E, 3)
        out.append(check_bound(sc, cr[:, None].expand(NT, g, E, 3), cb[:, None].expand(NT, g, E, 3), "P4 Apost scalar columns (token, group, expert, [q rp, -q rp mup, q])"))
        if not v.ln_post:
            R.neg_zero(sc[..., 1].float(), "P4 Apost middle scalar column without LayerNorm-post (token, group, expert)")
        if s.KPp > s.KP:
            check_untouched(s.dev("Apost", torch.int16 if bf16 else torch.int32, (NT, g, s.KPp))[:, :, s.KP:], -1, "P4 Apost padding columns KP..KPp")
        return max(out)
    rec.product("P4", "k_post_small (stream)" if form == "stream" else "k_post_small", p4)


def _backward(s, ran, rec):
    NT, g, E, S, N, dg, dgp, El, K, Kp = s.NT, s.g, s.E, s.S, s.N, s.dg, s.dgp, s.El, s.K, s.Kp
    bf16, zbf, cfg, v, form = s.bf16, s.zbf, s.cfg, s.v, s.form
    tuned, gen = s.lay.family == "tuned", s.lay.family == "tile_gen"
    stream = form == "stream"
    # ---- which forms ran ------------------------------------------------------------------------------------------------------------------
    psb_streams = "k_post_small_bwd (stream)" in ran
    rec.check("backward scopes", ("k_post_small_bwd" in ran) == (not psb_streams), f"{sorted(ran)}")
    if stream:
        rec.check("backward scopes", "k_mid_bwd (stream)" in ran and "k_pre_bwd (stream)" in ran and "k_pre_small_bwd" not in ran, f"mid_bwd / pre_small_bwd did not stream: {sorted(ran)}")
        # the streamed post_small_bwd wants Dims::gram64 (two or four experts in bf16; no switch enters: moe_plan.cpp:176) and the split dApost
        rec.check("backward scopes", psb_streams == s.gram64, f"{sorted(ran)}")
        mdb, prb = "k_mid_bwd (stream)", "k_pre_bwd (stream)"
    else:
        rec.check("backward scopes", not any(n.endswith("(stream)") for n in ran) and {"k_post_small_bwd", "k_mid_bwd", "k_pre_small_bwd"} <= ran, f"{sorted(ran)}")
        rec.check("backward scopes", ("k_pre_lat_bwd" in ran) == (tuned and El > 0), f"{sorted(ran)}")
        mdb, prb = "k_mid_bwd", "k_pre_small_bwd"
    psb = "k_post_small_bwd (stream)" if psb_streams else "k_post_small_bwd"
    # dGq: the path is the plan's, in every BatchNorm mode (moe_backward.cpp:123-133); without LayerNorm-post none of the three runs
    gram_bwd = "k_gram64" in ran
    rec.check("backward scopes", gram_bwd == (v.ln_post and s.gram64 and not psb_streams), f"k_gram64 (weighted) runs exactly for ln_post in gram64 mode behind a register-resident post_small_bwd: {sorted(ran)}")
    # ---- operands as stored ---------------------------------------------------------------------------------------------------------------
    DZ = g * E * dgp
    Z, bn1 = s.z("Z"), s.f32("bn1", (4, g, E, dgp))
    uvh = s.f32("uvh", (2 * DZ + 2 * g * E,))
    us, vh = uvh[:DZ].reshape(g, E, dgp), uvh[DZ:2 * DZ].reshape(g, E, dgp)
    qv = s.f32("probs", (S, E)).repeat_interleave(N, 0)
    rp, mup = s.tokE("rpmup")
    dsm = s.f32("dsm", (8, g, E, dgp))
    split = bf16 and zbf and not bool(torch.isnan(s.f32("dApx", (NT, g, s.XW))[:, :, :3 * E]).any())
    if split:                                                              # T columns (rows E * dgp wide) + fp32 dApx (moe_backward.cpp:101-109)
        dAp = s.dev("dAp", torch.bfloat16, (NT, g, E, dgp))
        dApx = s.f32("dApx", (NT, g, s.XW))[:, :, :3 * E].reshape(NT, g, E, 3)
    else:                                                                  # one fp32 array (NT, g, KPp)
        whole = s.f32("dAp", (NT, g, s.KPp))
        dAp, dApx = whole[:, :, :E * dgp].reshape(NT, g, E, dgp), whole[:, :, E * dgp:s.KP].reshape(NT, g, E, 3)
    if psb_streams:
        rec.check("backward scopes", split, "the streamed post_small_bwd reads the split dApost")
    print(f"DAPOST {rec.shape} {rec.variant}: {'split (bf16 + dApx)' if split else 'whole (fp32)'}")
    dzp = s.z("dzp")
    ref = R.post_mid_bwd_ref(dAp, dApx, Z, bn1, s.f32("Gq", (g, E, dgp, dgp)), us, vh, qv, rp, mup, dsm[2] if v.moments else None,
                             s.f32("sdSzz", (g, E, dgp, dgp)) if v.moments else None, s.relu, cfg.Cx, planes=s.planes, out_bf16=zbf,
                             ln_post=v.ln_post, moments=v.moments)
    # ---- P5 ----------------------------------------------------------------------------------------------------------------------------
    if s.gram64 and not psb_streams:                                       # kf_post_small_bwd stores dSoo for gram.hip (tile_fast.hip:497), 0.f with ln_post off (:459)
        def p5():
            got = s.f32("dSooT", (E, NT)).t()
            if not v.ln_post:
                _exact(got, 0.0, "P5 dSooT without LayerNorm-post (token, expert)")
            return check_bound(got, *ref["dSoo"], "P5 dSooT (token, expert)")
        rec.product("P5", psb, p5)
    else:
        try:                                                               # the step-aside, asserted: the buffer is as the workspace arrived
            s.poisoned("dSooT", "P5 dSooT (nobody writes it: the streamed form keeps dSoo in registers, the other sites have no gram64 mode)")
            rec.aside("P5", psb, "dSoo stays in registers (streamed: fused Gram product)" if psb_streams else "no gram64 mode: dSooT is not written")
        except AssertionError as e:
            rec.fail.append(f"P5 [{rec.variant} {form}]: {e}")
    # ---- P7 ----------------------------------------------------------------------------------------------------------------------------
    if not v.ln_post:
        def p7u():
            s.poisoned("dGq", "P7 dGq without LayerNorm-post (moe_backward.cpp:123-133: no path runs; tile_stream.hip:438 skips the slab sum)")
            return 0.0
        rec.product("P7", "untouched", p7u)
    elif s.gram64:
        dSoo_st = None if psb_streams else s.f32("dSooT", (E, NT)).t()

        def p7():
            w, ew = (ref["dSoo"][0], ref["dSoo"][1]) if psb_streams else (dSoo_st, None)
            G, e = R.dgq_ref(Z, bn1, s.relu, w, ew, mirrored=psb_streams)
            return check_bound(s.f32("dGq", (g, E, 32, 32)), G, e, "P7 dGq (group, expert, row, column)")
        rec.product("P7", psb + " (fused Gram)" if psb_streams else "k_gram64 (weighted)", p7)
    else:
        def p7e():
            G, e = R.dgq_engine_ref(Z, bn1, s.relu, s.zT("Zp"), ref["dSoo"][0], ref["dSoo"][1], out_bf16=bf16, prod_eps=0.0 if bf16 else 2.0 ** -27)
            return check_bound(s.f32("dGq", (g, E, dgp, dgp)), G, e, "P7 dGq, engine path (group, expert, row, column)")
        rec.product("P7", psb + " + engine", p7e)

    # ---- P6 ----------------------------------------------------------------------------------------------------------------------------
    def p6():
        d2, bound, mask, kink = ref["dzp"]
        _zero(dzp[..., dg:], "P6 dzp, padding entries dg..dgp (token, group, expert, entry - dg)")
        return R.check_masked(dzp[..., :dg], d2[..., :dg], bound[..., :dg], mask.expand_as(d2)[..., :dg], kink.expand_as(d2)[..., :dg],
                              f"P6 {rec.shape} {rec.variant} final dzp (token, group, expert, entry)")
    rec.product("P6", psb + " + " + mdb, p6)

    # ---- P8: formed and stored in every mode (bwd_kernels.hip:72-73), zh from bn1 as stored --------------------------------------------------
    def p8():
        (m3, b3), (m4, b4) = R.dsm34_ref(dzp, Z, bn1)
        return max(check_bound(dsm[3], m3, b3, "P8 dsm[3] = mean dy (group, expert, entry)"), check_bound(dsm[4], m4, b4, "P8 dsm[4] = mean dy zh (group, expert, entry)"))
    rec.product("P8", mdb + " + finalizer", p8)
    # ---- P9 ----------------------------------------------------------------------------------------------------------------------------
    rr, mu = s.tokE("rmu")
    dL2x = s.dev("dL2x", s.T, (NT, s.KLp))
    train = v.bn == "train"
    r9 = R.pre_small_bwd_ref(dzp, Z, bn1, dsm[3] if train else None, dsm[4] if train else None, rr, mu, s.f32("wsum", (g, E, dgp)), s.f32("dconst", (g, E, dgp)),
                             cfg.Cx, out_bf16=bf16, bn=v.bn, ln_before=v.ln_before)
    has_dslat = (tuned and not stream) or gen                              # tile_fast.hip:817, tile_gen.inc:802; not tile_stream.hip:1202 / tile_kernels.hip:929

    def p9():
        Zw = s.zT("Zw")
        _zero(Zw[..., dg:], "P9 Zw, padding entries dg..dgp (token, group, expert, entry - dg)")
        out = [check_bound(Zw, *r9["Zw"], "P9 Zw = dZx (token, group, expert, entry)"),
               check_bound(dL2x[:, s.KL], *r9["dL2x_KL"], "P9 dL2x[:, KL] (token)"),
               check_bound(s.f32("rs2x", (NT,)), *r9["rs2x"], "P9 rs2x (token)")]
        _exact(dL2x[:, s.KL + 1].float(), 1.0, "P9 dL2x[:, KL + 1] (token)")
        if not v.ln_before:
            _exact(dL2x[:, s.KL].float(), 0.0, "P9 dL2x[:, KL] without LayerNorm-before (token)")
            _exact(s.f32("rs2x", (NT,)), 0.0, "P9 rs2x without LayerNorm-before (token)")
        if has_dslat:
            dsl = s.f32("dslat", (El, 2, NT))
            out.append(check_bound(dsl[:, 0].t(), r9["dSx"][0][:, s.lat], r9["dSx"][1][:, s.lat], "P9 dslat dSx (token, latent slot)"))
            out.append(check_bound(dsl[:, 1].t(), r9["dSxx"][0][:, s.lat], r9["dSxx"][1][:, s.lat], "P9 dslat dSxx (token, latent slot)"))
        else:
            s.poisoned("dslat", "P9 dslat (the streamed and the any-shape pass keep the LayerNorm sums in registers / LDS: nobody writes it)")
        return max(out)
    rec.product("P9", prb, p9)
    # ---- P10 ---------------------------------------------------------------------------------------------------------------------------
    L2, a, TT, TW, Tsum = s.latent()
    gvl = s.gv[s.lat]

    def p10():
        if has_dslat:                                                      # pre_lat_bwd reads them back as stored: Zw and dslat
            dzr = s.zT("Zw")[:, :, s.lat].double()
            dsl = s.f32("dslat", (El, 2, NT)).double()
            dSx, dSxx = dsl[:, 0].t(), dsl[:, 1].t()
            edzr, edSx, edSxx = torch.zeros_like(dzr), torch.zeros_like(dSx), torch.zeros_like(dSxx)
        else:                                                              # one kernel: dzraw and the sums never leave the chip
            dzr, edzr = r9["dzr"][0][:, :, s.lat], r9["dzr"][1][:, :, s.lat]
            (dSx, edSx), (dSxx, edSxx) = ((t[:, s.lat] for t in r9[k]) for k in ("dSx", "dSxx"))
        ref10, bound10 = R.pre_lat_bwd_ref(a, L2, TT, TW, Tsum, gvl, dzr, edzr, dSx, edSx, dSxx, edSxx, cfg.Cx, planes=s.planes, out_bf16=bf16)
        got = dL2x[:, :s.KL].reshape(NT, El, Kp)
        _zero(got[..., K:], "P10 dL2x[:, :KL], columns of the padding slots K..Kp (token, latent slot, slot - K)")
        if s.KLp > s.KLT:
            check_untouched(s.dev("dL2x", torch.int16 if bf16 else torch.int32, (NT, s.KLp))[:, s.KLT:], -1, "P10 dL2x padding columns KLT..KLp")
        return check_bound(got, ref10, bound10, "P10 dL2x[:, :KL] (token, latent slot, latent token)")
    rec.product("P10", prb if (stream or not (tuned or gen)) else ("k_pre_lat_bwd" if tuned else "k_pre_small_bwd (kg_pre_lat_bwd)"), p10)


def _run(site, variant):
    s = VarSite(site, variant)
    s.run.forward()
    return s


# what the two runs of a site must agree on, byte for byte, at the end of section 1 (a buffer nobody wrote holds the poison both times)
REPEAT = ("Z", "a", "rmu", "bn1", "mz", "Szz", "Apost", "rpmup", "dzp", "dsm", "dGq", "dSooT", "Zw", "dL2x", "rs2x", "dslat")


@pytest.mark.parametrize("site,variant", RUNS)
def test_passes_of_one_site(site, variant):
    from avmoe_amd import _capi
    t0 = time.time()
    form, _what, _bf16, hook = SITES[site]
    rec = VarRecorder(site, variant, form)
    # (Profiled sets HOOK_ALL_FORCE; the nested test_hooks REPLACES the whole mask: only the named bit, or none, is on in here)
    with Profiled() as prof, _capi.test_hooks(getattr(_capi, hook) if hook else 0):
        s = _run(site, variant)
        print(f"\nSITE   {site} {variant}: {s.lay.family} {s.lay.instance}, g {s.g}, dgp {s.dgp} (dg {s.dg}), Kp {s.Kp} (K {s.K}), {s.NT} tokens, BatchNorm '{s.v.bn}'")
        _forward(s, prof.names(), rec)
        s.begin_backward()
        s.part(1)
        _backward(s, prof.names(), rec)
        rec.check("guards", s.run.guards_intact(), "a kernel wrote past its workspace")
        rec.check("finite", bool(torch.isfinite(s.run.out.float()).all() and torch.isfinite(s.z("dzp").float()).all() and torch.isfinite(s.zT("Zw").float()).all()),
                  "out, dzp or Zw holds a non-finite value")
        # ---- the same bytes twice ----
        again = _run(site, variant)
        again.begin_backward()
        again.part(1)
        for name in REPEAT + (() if s.gram64 else ("Zp",)):
            x, y = s.raw(name), again.raw(name)
            rec.check("repeat", torch.equal(x, y), f"{name}: {int((x != y).sum())} of {x.numel()} bytes differ between two runs of the same site")
        rec.check("guards", again.run.guards_intact(), "a kernel wrote past its workspace (second run)")
    TIMES[(site, variant)] = time.time() - t0
    print(f"TIME   {site} {variant} {TIMES[(site, variant)]:.2f} s")
    rec.finish()


def test_every_pass_was_checked_in_every_variant():
    """Closes the module: each (tag, variant) pair was checked against fp64 in the streamed form -- or its step-aside was asserted at every
    streamed site -- AND in at least one other form at a ragged shape.  (Runs after the tests above: it fails when they did not run.)"""
    missing = {}
    streamed = [s for s in SITES if SITES[s][0] == "stream"]
    for tag in TAGS:
        for variant in VARIANTS:
            got, aside = CHECKED.get((tag, variant), {}), ASIDE.get((tag, variant), {})
            for site, ratio in sorted(got.items()):
                print(f"COVERED {tag} {variant} {SITES[site][0]} {site} {ratio:.4f}")
            for site, why in sorted(aside.items()):
                print(f"COVERED {tag} {variant} {SITES[site][0]} {site} stepped aside: {why}")
            in_stream = any(s in got for s in streamed) or all(s in got or s in aside for s in streamed)
            others = [s for s in got if SITES[s][0] != "stream"]
            if not in_stream or not others or not (set(others) & RAGGED):
                missing[(tag, variant)] = (TAGS[tag], sorted(got), sorted(aside))
    for (site, variant), t in TIMES.items():
        print(f"TIME   {site} {variant} {t:.2f} s")
    print(f"TIME   module {sum(TIMES.values()):.2f} s over {len(TIMES)} cases")
    assert not missing, f"not checked in the streamed form (or its step-aside asserted) and in one other form at a ragged shape: {missing}"
