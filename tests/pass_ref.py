"""fp64 references and per-element bounds for the per-token bottleneck-space passes of the tuned shape (bottleneck 64 in 2 groups, 32 latent
tokens): post_small, the post_small_bwd + mid_bwd composite and pre_small_bwd, in their three forms (csrc/tile_stream.hip kfs_*,
csrc/tile_fast.hip kf_*<bf16>, kf_*<float>), which share one arithmetic.  In the style of tests/stream_product_ref.py, whose check_bound /
EPS_* this module reuses: every function takes the operands AS STORED (bf16 and fp32 are exact in fp64) and returns (ref, bound) per output,

    ref   = the formula of oracle/algebra_ref.py (forward :182-265, POST_SMALL backward :305-325, phase 3 :353-364, phase 4 :365-382)
    bound = sum over the kernel's roundings of  eps_i * (magnitude of what that rounding rounds),  propagated to first order,

the roundings counted from the kernel text (tile_fast.hip line numbers in the comments below; the streamed kernels repeat the same
expressions: tile_stream.hip:676-700 / :296-370 / :530-550 / :1150-1199).  Unit roundoffs:

    U32        2^-24   one fp32 operation (round to nearest); an fp32 division: hipcc compiles HIP device code with
                       -fhip-fp32-correctly-rounded-divide-sqrt on by default (clang command-line reference), so `x / C` and `1.f / x` are
                       correctly rounded
    EPS_ACC    2^-23   per term of an fp32 sum of k terms in any order (stream_product_ref.py)
    EPS_BF16   2^-8    a bf16 store
    EPS_PLANES 2^-16   a two-plane mat-vec, bf16 forms only (tile_lane.h:113 mmT_split, tile_stream.hip:165 mm_presplit)
    EPS_RSQRT  2^-22   rsqrtf: __clang_hip_math.h:671 maps it to __ocml_rsqrt_f32, which the ROCm device libraries build to the OpenCL C
                       accuracy table (rsqrt: <= 2 ulp; an ulp of fp32 is 2^-23 relative)

Nothing is fitted to a measured error.  Layouts here are token-major: Z-space tensors (NT, g, E, GD), per-token scalars (NT, E), per-column
constants (g, E, GD), d x d matrices (g, E, GD, GD) indexed [k][c] as the kernels read them (W[c] = sum_k P[k] M[k][c], tile_lane.h:82).
Works on CPU and GPU tensors alike.

Every width comes from the operands: GD entries per group (the last axis of a Z-space tensor), g groups (1 when the plan merged them), Kp
latent slots per expert (the last axis of a / L2) of which the first K are real (the side of TT), and the contraction lengths in the EPS_ACC
terms (`_nsum`).  At the tuned shape (g = 2, GD = Kp = K = 32) every count below is the number it was when this module spelled 32.

The same functions serve the other two links of every pass's form chain, the generalised register-resident kernels kg_* (csrc/tile_gen.inc,
fp32 and bf16) and the any-shape kernels kt_* (csrc/tile_kernels.hip, Z-space tensors always fp32).  They were read against tile_fast.hip
expression by expression; where they round differently the difference is named here, with its line, and is either inside a count the
bound already carries or an argument of the function:
    planes=False       kg_*<float> (tile_lane.h:143-147 mmT<.., false>) and every kt_* (tile_kernels.hip:40-47 tile_mm) run their mat-vecs on
                       the exact-fp32 matrix pipe: no plane term.  kg_*<bf16>: mmT_split (tile_lane.h:113-128), an odd last chunk padded with
                       zeros, EPS_PLANES as in the tuned forms.
    order of the sums  tile_gen.inc:335-343 adds a lane's products over ALL groups and chunks before the fold over the four lanes (tile_fast
                       folds per group); tile_kernels.hip:483-490 adds per column tile and folds over sixteen lanes.  The bounds count
                       terms in ANY order (EPS_ACC per term), so neither needs a term of its own.
    softmax            tile_gen.inc:603-614: padding slots contribute an exact 0 to the sum, `inv = 1.f / sum` then `ex * inv`, as tile_fast
                       (two roundings, counted); tile_kernels.hip:304-314 evaluates __expf twice with the same argument (same value).
                       The sum has K non-zero terms; Kp + 2 are counted.
    1 / rr             tile_gen.inc:742,768 multiplies by irr = 1.f / rr (two roundings, as tile_fast); tile_kernels.hip:901 divides (one):
                       three are counted for zc either way.
    token sums         flush_cols (tile_gen.inc:93-99) folds the tile slots of an expert in LDS, flush_colacc (tile_kernels.hip:97-107) the
                       waves of the block, before the block partial is written: a sum of NT terms has NT - 1 additions however it is
                       bracketed, so the extra fold is inside colsum_ref's (NT + 2) EPS_ACC.  expert_scalar (tile_gen.inc:103-111) only
                       feeds blkscal, which no per-token output reads.
    rounds of experts  dL2x[:, KL] / rs2x add the experts round by round through dsxs (tile_gen.inc:822-831; tile_kernels.hip:929-930 expert by
                       expert): still E terms in expert order, an fp32 partial in between (no extra rounding).

The switches.  ln_before, ln_post, use_gate, use_bn and training are run-time branches inside every form of every pass (F_LN_BEFORE ..
F_USE_GATE in tile_fast.hip; a.ln_before, a.use_bn, a.bn_train, a.ln_post, a.use_gate, a.moments in the other three files); every function
whose map they change takes them as keyword arguments that default to the training-mode site with everything on:
    ln_before=False    rmu_ref / rmu_off_ref (exactly (1, 0), stored by all four forms), z_map_ref (two operations), pre_small_bwd_ref (Zw = dz,
                       dSx = dSxx = dL2x[:, KL] = rs2x = 0 exactly)
    ln_post=False      post_small_ref (rp = 1, mup = 0, Apost = rnd_T(q z')), scalar_cols_ref ([q, -0, q]; neg_zero), post_mid_bwd_ref (no dSoo)
    bn / mode          bn1_ref mode "eval" / "off", pre_small_bwd_ref bn "eval" (dz = scale dy) / "off" (dz = dy); post_mid_bwd_ref
                       moments=False (use_bn && training is false: mid_bwd adds literal zeros).  zprime and dsm34_ref read bn1 AS STORED and
                       need no switch: their counts of two and three roundings cover the exact products with scale = 1, shift = 0.
    use_gate           no argument: every launcher passes use_gate && !gate_w and the plan folds the gate into Bpost (Dims::gate_w,
                       moe_plan.cpp:35), so qv = probs whether the gate is on or off -- the callers pass probs and the third scalar column of
                       Apost, q itself, shows which arm ran.  The kernels' token-space arm (q = probs * gate) runs only under the
                       development switch that clears gate_w (sw.gate_token): no test reaches it, it stays unexercised.
In a branch where the kernel's value is exact the bound is 0 and check_bound demands equality."""
import torch

from tests.stream_product_ref import EPS_ACC, EPS_BF16, EPS_PLANES, ProductMismatch, check_bound

U32 = 2.0 ** -24
EPS_RSQRT = 2.0 ** -22
KINK = 2.0 ** -22          # |y_ref| <= KINK * (|z * scale| + |shift|): the ReLU may fall on either side
KINK_CAP = 1e-5            # at most this share of a tensor's elements (expected ~1e-7: z is continuous at O(1))

def _nsum(g, gd):
    """terms of an fp32 sum over one token's g * gd bottleneck entries of an expert (in-lane partials, then the fold over the lanes that
    hold the token): 2 * 32 at the tuned shape"""
    return g * gd


def _store(ref, pre, out_bf16):
    """bound behind a store of element type T: the arithmetic error `pre`, plus the bf16 rounding of (ref + that error)"""
    return pre + EPS_BF16 * (ref.abs() + pre) if out_bf16 else pre


def zprime(Z, bn1, relu):
    """z' = act(z * scale + shift) as every pass forms it from the stored z (tile_fast.hip:138-139, 278-279, 441-442): two fp32 roundings
    (or one, fused).  -> (zp, ezp, y, ymag, kink); relu: (E,) bool"""
    z, sc, sh = Z.double(), bn1[2].double(), bn1[3].double()
    y = z * sc + sh
    ymag = (z * sc).abs() + sh.abs()
    r = relu.to(z.device).view(1, 1, -1, 1)
    zp = torch.where(r, y.clamp_min(0.0), y)
    return zp, 2 * U32 * ymag, y, ymag, r & (y.abs() <= KINK * ymag)


def matvec(zp, ezp, M, planes):
    """w[t, g, e, c] = sum_k zp[t, g, e, k] M[g, e, k, c] on the matrix pipe: GD terms in fp32 (32 at the tuned shape), two bf16 planes in
    the bf16 register-resident forms -> (w, mag, err)"""
    M = M.double()
    w = torch.einsum("tgek,gekc->tgec", zp, M)
    mag = torch.einsum("tgek,gekc->tgec", zp.abs(), M.abs())
    err = torch.einsum("tgek,gekc->tgec", ezp, M.abs()) + (M.shape[-2] * EPS_ACC + (EPS_PLANES if planes else 0.0)) * mag
    return w, mag, err


def _first_order(r, evar, what):
    """|d rsqrt(v)| = 0.5 r^3 |dv| is honest only while r^2 |dv| is small: an input where it is not is a wrong test input"""
    worst = float((r * r * evar).max())
    assert worst <= 0.125, f"{what}: r^2 * bound(var) = {worst:.3g} > 1/8 at token {int((r * r * evar).reshape(r.shape[0], -1).max(1).values.argmax())}"


def post_small_ref(Z, bn1, Gq, us, vh, H1p, H2p, qv, relu, C, ln_eps, *, planes, out_bf16, ln_post=True):
    """tile_fast.hip:274-311 (tile_gen.inc:300-361, tile_kernels.hip:457-516).  Z (NT, g, E, GD); Gq (g, E, GD, GD); us, vh (g, E, GD);
    H1p, H2p (g, E): the per-group parts the kernel adds (:256; tile_gen.inc:301); qv (NT, E) = probs * gate -- probs alone when the
    site has no gate, and also when the plan folded the gate into Bpost (Dims::gate_w, moe_plan.cpp:35: every launcher passes
    use_gate && !gate_w, tile_fast.hip:1132, tile_stream.hip:1419, tile_gen.inc:1147, tile_kernels.hip:526).
    ln_post=False: every form initialises rp = 1, mup = 0 and skips the statistics (tile_fast.hip:282-283, tile_stream.hip:679-680,
    tile_gen.inc:327, tile_kernels.hip:472-473), stores that pair, and forms Apost = rnd_T((qv * 1) * z'): the product with 1 is exact,
    ONE fp32 rounding is left.
    -> {"rp", "mup": (NT, E); "Apost": (NT, g, E, GD)}, each (ref, bound)"""
    zp, ezp, _y, _ym, _k = zprime(Z, bn1, relu)
    us, vh, qv = us.double(), vh.double(), qv.double()
    if not ln_post:
        one, zero = torch.ones_like(qv), torch.zeros_like(qv)
        A = qv[:, None, :, None] * zp
        pre = qv.abs()[:, None, :, None] * ezp + U32 * A.abs()
        return {"rp": (one, zero), "mup": (zero, zero.clone()), "Apost": (A, _store(A, pre, out_bf16))}
    w, wmag, ew = matvec(zp, ezp, Gq, planes)                                  # :288
    H1, H2 = H1p.double().sum(0), H2p.double().sum(0)
    H1m, H2m = H1p.double().abs().sum(0), H2p.double().abs().sum(0)
    g = Z.shape[1]
    k = _nsum(g, Z.shape[3]) + 1 + g                                         # the products (64 at the tuned shape), the fold of the lanes' partials, H (g parts)
    So = (zp * us).sum((1, 3)) + H1                                          # :293, :297
    So_mag = (zp.abs() * us.abs()).sum((1, 3)) + H1m
    eSo = (ezp * us.abs()).sum((1, 3)) + k * EPS_ACC * So_mag
    t = w + 2 * vh                                                           # :294: one rounding for the sum, then the product
    tmag = wmag + 2 * vh.abs()
    Soo = (zp * t).sum((1, 3)) + H2
    Soo_mag = (zp.abs() * tmag).sum((1, 3)) + H2m
    eSoo = (ezp * tmag + zp.abs() * (ew + U32 * tmag)).sum((1, 3)) + k * EPS_ACC * Soo_mag
    mup = So / C                                                             # :298
    emup = eSo / C + U32 * So_mag / C
    var = (Soo / C - mup * mup).clamp_min(0.0) + ln_eps                      # :299: /, *, -, + : four roundings of values no larger than vmag
    vmag = Soo_mag / C + (So_mag / C) ** 2 + ln_eps
    evar = eSoo / C + 2 * mup.abs() * emup + 4 * U32 * vmag
    rp = torch.rsqrt(var)
    _first_order(rp, evar, "post_small rp")
    erp = 0.5 * rp ** 3 * evar + EPS_RSQRT * rp
    scl = (qv * rp)[:, None, :, None]                                        # :303, :306: two products
    A = scl * zp
    pre = (qv.abs() * erp)[:, None, :, None] * zp.abs() + scl.abs() * ezp + 2 * U32 * A.abs()
    return {"rp": (rp, erp), "mup": (mup, emup), "Apost": (A, _store(A, pre, out_bf16))}


def scalar_cols_ref(qv, rp, mup, *, out_bf16, ln_post=True):
    """[q rp, -q rp mup, q] from rp / mup AS STORED (tile_fast.hip:321-339, tile_stream.hip:723-738, tile_gen.inc:358,
    tile_kernels.hip:509): two fp32 products and a store.
    ln_post=False: the stored pair is (1, 0), so the columns are [q * 1, (-q * 1) * 0, q] = [q, -0, q]: both products exact (arithmetic
    bound 0), the middle column a NEGATIVE zero in either type (q >= 0: a probability; -q * 1 = -q, and (-q) * (+0) = -0 also when
    q = 0) -- neg_zero() asserts that bit pattern, which a comparison of values cannot see.
    -> (ref, bound), (NT, E, 3)"""
    qv, rp, mup = qv.double(), rp.double(), mup.double()
    ref = torch.stack([qv * rp, -qv * rp * mup, qv], -1)
    if not ln_post:
        return ref, _store(ref, torch.zeros_like(ref), out_bf16)
    pre = torch.stack([U32 * (qv * rp).abs(), 2 * U32 * (qv * rp * mup).abs(), torch.zeros_like(qv)], -1)
    return ref, _store(ref, pre, out_bf16)


def neg_zero(x, name):
    """every element of x is -0 (sign bit set, magnitude 0): the middle scalar column of Apost without LayerNorm-post"""
    bad = ~((x == 0) & torch.signbit(x))
    if bool(bad.any()):
        i = tuple(int(k) for k in bad.nonzero()[0])
        raise ProductMismatch(f"{name}: {int(bad.sum())} of {x.numel()} elements are not -0, first {float(x[i])!r} at {i}")


def post_mid_bwd_ref(dAp, dApx, Z, bn1, Gq, us, vh, qv, rp, mup, dm, sdSzz, relu, C, *, planes, out_bf16, ln_post=True, moments=True):
    """post_small_bwd (tile_fast.hip:434-506) followed by mid_bwd (:133-161) as ONE map to the final dzp; the first pass's store of dz' is one
    named rounding of the intermediate.  dAp (NT, g, E, GD); dApx (NT, g, E, 3); rp, mup (NT, E) as stored; dm = dsm[2] (g, E, GD).
    The generalised kernels spell the same expressions (tile_gen.inc:451-458, :483-485, :254-255), the any-shape ones too
    (tile_kernels.hip:663-670, :686-688, :781-782) but keep dz' in fp32 whatever the site's type (out_bf16=False there).
    ln_post=False: dSo = dSoo = 0 exactly, no Gq mat-vec, dz' = (qv rp) dAp with rp = 1 as stored -- the product qv * 1 is exact, ONE
    rounding (tile_fast.hip:459-485, tile_stream.hip:312-326, tile_gen.inc:452-484, tile_kernels.hip:664-687).
    moments=False (a.moments = use_bn && training, tile_fast.hip:1169: eval mode or no BatchNorm): mid_bwd reads neither sdSzz nor
    dsm[2] and adds two literal zeros, d = dz' + 0.f + 0.f (tile_fast.hip:102, :146, :153; tile_stream.hip:473, :543; tile_gen.inc:216-218,
    :247; tile_kernels.hip:743, :770): exact, so the only roundings behind the first store are that store read back and the final one.
    dm / sdSzz are then not read here either (pass None: the buffers hold whatever the workspace held).
    -> {"dSoo": (ref, bound) (NT, E); "dzp": (unmasked ref, bound, mask, kink) (NT, g, E, GD)}"""
    zp, ezp, y, _ym, kink = zprime(Z, bn1, relu)
    r = relu.to(zp.device).view(1, 1, -1, 1)
    mask = ~r | (y > 0)                                                      # :154: relu && z' <= 0 -> 0
    d, us, vh, qv, rp, mup = dAp.double(), us.double(), vh.double(), qv.double(), rp.double(), mup.double()
    if ln_post:
        dz1, dz1m, e1, dSoo, edSoo, ew = _post_bwd_ln(d, dApx, zp, ezp, Gq, us, vh, qv, rp, mup, C, Z.shape[1], Z.shape[3], planes)
    else:
        k1 = (qv * rp)[:, None, :, None]                                     # :472 (rp is 1: exact), :483
        dz1 = k1 * d
        dz1m, e1 = dz1.abs(), U32 * dz1.abs()
        dSoo = torch.zeros_like(qv)
        edSoo = torch.zeros_like(qv)
    e1 = _store(dz1, e1, out_bf16)                                           # :496 st_row<T>: the intermediate dz' as mid_bwd reads it back
    if moments:
        dm = dm.double()
        w2, w2mag, ew2 = matvec(zp, ezp, sdSzz, planes)                      # :146
        d2 = dz1 + dm + w2                                                   # :153: two adds
        pre = e1 + ew2 + 2 * U32 * (dz1m + dm.abs() + w2mag)
    else:                                                                    # :153 with dm = 0.f and w = 0.f: exact, and :154 rounds a value
        return {"dSoo": (dSoo, edSoo), "dzp": (dz1, e1, mask, kink)}         # that the first store already rounded to T: exact too
    return {"dSoo": (dSoo, edSoo), "dzp": (d2, _store(d2, pre, out_bf16), mask, kink)}     # :154 rndT<T>


def _post_bwd_ln(d, dApx, zp, ezp, Gq, us, vh, qv, rp, mup, C, g, GD, planes):
    """the LayerNorm-post arm of post_small_bwd (tile_fast.hip:449-485) -> dz' before its store, its magnitude and arithmetic bound,
    dSoo with its bound"""
    da = dApx.double().sum(1)                                                # :423 / :449: group 0 + group 1, one rounding (tile_gen.inc:444: g - 1 of them)
    dam = dApx.double().abs().sum(1)
    eda = (g - 1) * U32 * dam
    zz = (d * zp).sum((1, 3))                                                # :457-458
    zzm = (d.abs() * zp.abs()).sum((1, 3))
    ezz = (d.abs() * ezp).sum((1, 3)) + (_nsum(g, GD) + 2) * EPS_ACC * zzm
    drp = qv * (zz + da[..., 0] - mup * da[..., 1])                          # :463: four products, two sums
    drpm = qv.abs() * (zzm + dam[..., 0] + mup.abs() * dam[..., 1])
    edrp = qv.abs() * (ezz + eda[..., 0] + mup.abs() * eda[..., 1]) + 6 * U32 * drpm
    dmup = -qv * rp * da[..., 1]                                             # :464
    dmupm = (qv * rp).abs() * dam[..., 1]
    edmup = (qv * rp).abs() * eda[..., 1] + 2 * U32 * dmupm
    h = 0.5 * rp ** 3
    dvarp, dvm = -h * drp, h * drpm                                          # :465: three roundings (the factor -0.5 is exact)
    edv = h * edrp + 3 * U32 * dvm
    dSoo, dSoom = dvarp / C, dvm / C                                         # :466
    edSoo = edv / C + U32 * dSoom
    dmup2 = dmup - 2 * mup * dvarp                                           # :467: a product and a difference
    dmup2m = dmupm + 2 * mup.abs() * dvm
    edmup2 = edmup + 2 * mup.abs() * edv + 2 * U32 * dmup2m
    dSo, dSom = dmup2 / C, dmup2m / C                                        # :468
    edSo = edmup2 / C + U32 * dSom
    w, wmag, ew = matvec(zp, ezp, Gq, planes)                                  # :477
    k1 = (qv * rp)[:, None, :, None]                                         # :472
    x = lambda v: v[:, None, :, None]
    tt, ttm = 2 * w + 2 * vh, 2 * wmag + 2 * vh.abs()
    dz1 = k1 * d + x(dSo) * us + x(dSoo) * tt                                # :483-485: k1, k1 d, dSo us, the sum in brackets, dSoo (..), two adds
    dz1m = (k1 * d).abs() + x(dSom) * us.abs() + x(dSoom) * ttm
    e1 = x(edSo) * us.abs() + x(edSoo) * ttm + x(dSoom) * 2 * ew + 7 * U32 * dz1m
    return dz1, dz1m, e1, dSoo, edSoo, ew


def pre_small_bwd_ref(dy, Z, bn1, mdy, mdyz, rr, mu, wsum, dconst, C, *, out_bf16, bn="train", ln_before=True):
    """tile_fast.hip:753-838, tile_gen.inc:740-831, tile_kernels.hip:876-931, :1012-1020 (training-mode BatchNorm-1, folded LayerNorm).
    dy: the final dzp as stored (NT, g, E, GD); mdy, mdyz = dsm[3], dsm[4] (g, E, GD); rr, mu (NT, E) as stored; `zraw - mu wsum` is (z - dconst) / rr from the STORED z, as in the kernel (:770).
    bn: "train" as above; "eval" (use_bn && !training): dz = scale * dy, ONE rounding, dsm[3, 4] not read (tile_fast.hip:711, :767;
    tile_stream.hip:1073, :1168; tile_gen.inc:725, :765; tile_kernels.hip:866, :898); "off" (!use_bn): dz = dy exactly (:765).
    mdy / mdyz may be None unless bn == "train".
    ln_before=False: the kernels take rr = 1, mu = 0 WITHOUT reading rmu (tile_fast.hip:727-733, tile_stream.hip:1150, tile_gen.inc:740-741,
    tile_kernels.hip:878-879), Zw = rnd_T(dz) (:774 / :905: no product), and dSx = dSxx = 0 (:798-806), so the sum over the experts
    dL2x[:, KL] is 0 and rs2x = 2 * 0 = 0, all exact (bound 0).
    -> {"Zw": (NT, g, E, GD), "dzr": the same before its store (what the fused streamed pass hands to its hop-2 block); "dSx", "dSxx": (NT, E) (dslat holds the cross-modal experts' pair); "dL2x_KL", "rs2x": (NT,)}"""
    dy, z = dy.double(), Z.double()
    mean, rstd, sc = bn1[0].double(), bn1[1].double(), bn1[2].double()
    ws, dc = wsum.double(), dconst.double()
    rr_, mu_ = rr.double(), mu.double()
    rr, mu = rr_[:, None, :, None], mu_[:, None, :, None]
    if bn == "train":
        mdy, mdyz = mdy.double(), mdyz.double()
        zh3 = (z - mean) * rstd * mdyz                                       # :766: -, *, *, then -, -, * : six roundings
        dz = sc * (dy - mdy - zh3)
        dzm = sc.abs() * (dy.abs() + mdy.abs() + zh3.abs())
        edz = 6 * U32 * dzm
    elif bn == "eval":
        dz = sc * dy                                                         # :767
        dzm = dz.abs()
        edz = U32 * dzm
    else:
        assert bn == "off", bn
        dz, dzm, edz = dy, dy.abs(), torch.zeros_like(dy)                    # :764
    if not ln_before:
        zt, zn = torch.zeros_like(rr_), torch.zeros(dy.shape[0], dtype=torch.float64, device=dy.device)
        return {"Zw": (dz, _store(dz, edz, out_bf16)), "dzr": (dz, edz), "dSx": (zt, zt.clone()), "dSxx": (zt.clone(), zt.clone()),
                "dL2x_KL": (zn, zn.clone()), "rs2x": (zn.clone(), zn.clone())}
    zc = (z - dc) / rr                                                       # :747, :770: 1 / rr, the difference, the product
    ezc = 3 * U32 * zc.abs()
    k = _nsum(Z.shape[1], Z.shape[3]) + 2
    sdr = (dz * zc).sum((1, 3))                                              # :772, :800
    sdrm = (dzm * zc.abs()).sum((1, 3))
    esdr = (edz * zc.abs() + dzm * ezc).sum((1, 3)) + k * EPS_ACC * sdrm
    sdm = (dz * ws).sum((1, 3))
    sdmm = (dzm * ws.abs()).sum((1, 3))
    esdm = (edz * ws.abs()).sum((1, 3)) + k * EPS_ACC * sdmm
    v = rr * dz                                                              # :773
    ev = rr.abs() * edz + U32 * (rr.abs() * dzm)
    Zw = (v, _store(v, ev, out_bf16))                                        # :816
    dmu, dmum = -rr_ * sdm, rr_.abs() * sdmm                                 # :801
    edmu = rr_.abs() * esdm + U32 * dmum
    h = 0.5 * rr_.abs() ** 3
    dvar, dvm = -0.5 * rr_ ** 3 * sdr, h * sdrm                              # :802
    edv = h * esdr + 3 * U32 * dvm
    dSxx, dSxxm = dvar / C, dvm / C                                          # :803
    edSxx = edv / C + U32 * dSxxm
    dmu2, dmu2m = dmu - 2 * mu_ * dvar, dmum + 2 * mu_.abs() * dvm           # :804
    edmu2 = edmu + 2 * mu_.abs() * edv + 2 * U32 * dmu2m
    dSx, dSxm = dmu2 / C, dmu2m / C                                          # :805
    edSx = edmu2 / C + U32 * dSxm
    E = dSx.shape[1]
    ax, axm = dSx.sum(1), dSxm.sum(1)                                        # :835-836: E terms in expert order, stored as T
    eax = edSx.sum(1) + E * EPS_ACC * axm
    axx, axxm = 2 * dSxx.sum(1), 2 * dSxxm.sum(1)                            # :838 (the factor 2 is exact)
    eaxx = 2 * edSxx.sum(1) + E * EPS_ACC * axxm
    return {"Zw": Zw, "dzr": (v, ev), "dSx": (dSx, edSx), "dSxx": (dSxx, edSxx), "dL2x_KL": (ax, _store(ax, eax, out_bf16)), "rs2x": (axx, eaxx)}


def state_unchanged(now, uploaded, name):
    """a BatchNorm buffer (running mean, running variance, num_batches_tracked) after a forward that does not train BatchNorm -- eval mode,
    or no BatchNorm at all (bn1_finalize_col writes rm / rv / nbt only under use_bn && training, fwd_kernels.hip:1054-1067) -- is
    bit-identical to what was uploaded"""
    now, uploaded = now.detach().cpu(), uploaded.detach().cpu().to(now.dtype)
    if now.shape != uploaded.shape:
        raise ProductMismatch(f"{name}: shape {tuple(now.shape)} against {tuple(uploaded.shape)} uploaded")
    same = now.reshape(-1).contiguous().view(torch.uint8) == uploaded.reshape(-1).contiguous().view(torch.uint8)
    if not bool(same.all()):
        raise ProductMismatch(f"{name}: changed by a forward that does not train BatchNorm ({int((~same).sum())} bytes differ)")


def check_masked(got, ref, bound, mask, kink, name):
    """got == mask * ref within bound, where an element at the ReLU kink (zprime's `kink`) may sit on either branch: exactly 0, or the
    unmasked value within its bound.  The one exclusion there is; capped at KINK_CAP of the tensor, count printed.  -> worst err / bound"""
    nk = int(kink.sum())
    print(f"KINK   {name}: {nk} of {kink.numel()} elements within 2^-22 of the ReLU kink")
    if nk > KINK_CAP * kink.numel():
        raise ProductMismatch(f"{name}: {nk} of {kink.numel()} elements at the ReLU kink, more than {KINK_CAP:g} of the tensor")
    kink = kink.expand_as(ref)
    g = got.double()
    on = torch.where(kink, g != 0, mask.expand_as(ref))                      # at the kink: the branch the result took
    return check_bound(got, torch.where(on, ref, torch.zeros_like(ref)), torch.where(on, bound, torch.zeros_like(bound)), name)


def colsum_ref(x, scale, *, extra_terms=0):
    """scale * sum over tokens of x (NT, ...): an fp32 sum of NT terms in any order (per-lane accumulators, block partials, the finalizer),
    each term possibly the product of fp32 factors (`extra_terms` more roundings), times an fp32 scale.  -> (ref, bound)"""
    # (What this bound can see: NT * 2^-23 * sum |x| is about 1.5 typical |x| at NT = 3 920 and about 25 at NT = 14 400 -- one MISSING token
    # shows only in columns where that token is large, and not at all at the largest shape; a wrong block partial, a column shifted by
    # one, a wrong scale do show.  The term count is the issue's, any order; the per-lane / per-block partials are not bounded separately.)
    x = x.double()
    nt = x.shape[0]
    return x.sum(0) * scale, (nt + 2 + extra_terms) * EPS_ACC * x.abs().sum(0) * abs(scale)


def bn1_ref(Z, w, b, bn_eps, *, mode="train", rm=None, rv=None):
    """BatchNorm-1 (training mode) from the stored z: the two fp32 column sums over NT tokens (tile_fast.hip:654 per-lane accumulators ->
    colsum_fin.h block partials), then fwd_kernels.hip:988-1004 in double up to the casts: mean = fl32(s0 / NT), var = fl32(s1 / NT - m^2),
    rstd = rsqrtf(var + eps), scale = w * rstd, shift = b - mean * scale.  Z (NT, g, E, 32); w, b (g, E, 32).  -> (ref, bound), (4, g, E, 32)
    mode="eval" (bn1_finalize_col, fwd_kernels.hip:1068-1071: use_bn && !training): mean = running_mean and var = running_var AS
    UPLOADED (rm, rv (g, E, 32): exact), then the same fp32 tail: the sum var + eps (one rounding), rsqrtf (EPS_RSQRT), scale = w * rstd
    (one), shift = b - mean * scale (two).  Z is not read.
    mode="off" (:1051, !use_bn): exactly (0, 1, 1, 0), bound 0.
    The padding entries dg..dgp of all four rows are 0 in every mode (:1043, :1049, :1074); the callers pass the real entries and assert
    the padding by itself."""
    if mode == "off":
        one, zero = torch.ones_like(w, dtype=torch.float64), torch.zeros_like(w, dtype=torch.float64)
        return torch.stack([zero, one, one, zero]), torch.zeros(4, *w.shape, dtype=torch.float64, device=w.device)
    if mode == "eval":
        w, b, mean, var = w.double(), b.double(), rm.double(), rv.double()
        rstd = torch.rsqrt(var + bn_eps)
        evar = U32 * (var + bn_eps)
        _first_order(rstd[None], evar[None], "bn1 rstd (eval)")
        erstd = 0.5 * rstd ** 3 * evar + EPS_RSQRT * rstd
        sc = w * rstd
        esc = w.abs() * erstd + U32 * sc.abs()
        sh = b - mean * sc
        esh = mean.abs() * esc + 2 * U32 * (b.abs() + (mean * sc).abs())
        return torch.stack([mean, rstd, sc, sh]), torch.stack([torch.zeros_like(mean), erstd, esc, esh])
    assert mode == "train", mode
    z, w, b = Z.double(), w.double(), b.double()
    nt = z.shape[0]
    k = (nt + 2) * EPS_ACC                                                   # NT terms (each z * z product rounded once) + the partials' folds
    mean, m2 = z.mean(0), (z * z).mean(0)
    emean = k * z.abs().mean(0) + U32 * mean.abs()
    var = (m2 - mean * mean).clamp_min(0.0)
    evar = k * m2 + 2 * mean.abs() * k * z.abs().mean(0) + 2 * U32 * (m2 + mean * mean + bn_eps)      # the cast of var, the sum var + eps
    rstd = torch.rsqrt(var + bn_eps)
    _first_order(rstd[None], evar[None], "bn1 rstd")
    erstd = 0.5 * rstd ** 3 * evar + EPS_RSQRT * rstd
    sc = w * rstd
    esc = w.abs() * erstd + U32 * sc.abs()
    sh = b - mean * sc
    esh = mean.abs() * esc + sc.abs() * emean + 2 * U32 * (b.abs() + (mean * sc).abs())
    return torch.stack([mean, rstd, sc, sh]), torch.stack([emean, erstd, esc, esh])


def dsm34_ref(dy, Z, bn1):
    """dsm[3], dsm[4] = the token means of dy and dy * zh (tile_fast.hip:152-156 per-lane sums of the STORED dy, bwd_kernels.hip:72-73),
    zh = (z - mean) * rstd in fp32: three more roundings per term.  -> ((mdy, bound), (mdyz, bound)), each (g, E, 32)"""
    dy, z = dy.double(), Z.double()
    nt = dy.shape[0]
    zh = (z - bn1[0].double()) * bn1[1].double()
    return colsum_ref(dy, 1.0 / nt, extra_terms=1), colsum_ref(dy * zh, 1.0 / nt, extra_terms=4)


EPS_EXP = 2.0 ** -23       # __expf(x) = __builtin_amdgcn_exp2f(log2e * x) (__clang_hip_math.h:200-203: the mapping is all the header states).  No file
                           # under the ROCm installation documents the accuracy of that hardware exponential; 1 ulp is the figure of AMD's public
                           # instruction-set guide for V_EXP_F32.  The rounding of x and of log2e * x moves the result by 3 * U32 * |x| relative
TINY = 2.0 ** -126         # ... and it flushes a denormal result to zero


def softmax_ref(L2, *, out_bf16, K=None):
    """a = softmax over each latent slot's logits as stored (tile_fast.hip:592-613): max, __expf(l - max), the fp32 sum of Kp terms (32 at
    the tuned shape), inv = 1 / sum, a = rnd_T(ex * inv).  L2 (NT, El, Kp).  K: the real latent tokens of a slot (default: all Kp); the
    generalised kernels keep slots K..Kp out of the maximum and give them ex = 0 (tile_gen.inc:594, :603; tile_kernels.hip:301-317 never
    visits them and stores 0, :318-320), so a is EXACTLY 0 there (bound 0) whatever the logits buffer holds.  -> (ref, bound)"""
    Kp = L2.shape[-1]
    lg = L2.double() if K is None or K == Kp else L2[..., :K].double()
    x = lg - lg.max(-1, keepdim=True).values
    ex = torch.exp(x)
    rel = 3 * U32 * x.abs() + EPS_EXP
    eex = ex * rel + TINY
    sm = ex.sum(-1, keepdim=True)
    esm = eex.sum(-1, keepdim=True) + (Kp + 2) * EPS_ACC * sm
    a = ex / sm
    pre = a * (rel + esm / sm + 2 * U32) + TINY / sm                         # 1 / sum and the product: two roundings
    bound = _store(a, pre, out_bf16)
    if lg.shape[-1] < Kp:
        pad = torch.zeros(*a.shape[:-1], Kp - a.shape[-1], dtype=a.dtype, device=a.device)
        a, bound = torch.cat([a, pad], -1), torch.cat([bound, pad], -1)
    return a, bound


def rmu_off_ref(NT, E, device):
    """rmu without LayerNorm-before: every form initialises mu = 0, rr = 1 (tile_fast.hip:634, tile_stream.hip:952, tile_gen.inc:638,
    tile_kernels.hip:341), skips the statistics and STORES the pair unconditionally (tile_fast.hip:667, tile_stream.hip:977,
    tile_gen.inc:670, tile_kernels.hip:373): exactly (1, 0) in all four forms, bound 0.  -> {"rr", "mu": (ref, bound)}"""
    one, zero = torch.ones(NT, E, dtype=torch.float64, device=device), torch.zeros(NT, E, dtype=torch.float64, device=device)
    return {"rr": (one, zero), "mu": (zero.clone(), zero.clone())}


def rmu_ref(sx, L2, a, TT, Tsum, gv, C, ln_eps, *, planes, ln_before=True):
    """rmu = (rr, mu) of every expert (tile_fast.hip:572-637) from the stored row sums of X, the logits and a AS STORED (the kernel forms
    u1, u2, u3 from the rounded a, :612-614).  sx (2, NT); L2, a (NT, El, Kp); TT (NT, El, K, K) -- the token's frame's -- or per frame
    (S, El, K, K), K <= Kp the real latent tokens of a slot; Tsum (NT, El, Kp); gv (E,): the latent gate (gate_av / gate_self) of the experts
    that own a latent slot, 0 for the others (the first El experts own the slots).  The generalised kernels index TT with the true K and
    everything else with Kp (tile_gen.inc:527-535 stage_latent; tile_kernels.hip:269-278); slots K..Kp enter no sum (u2 is masked,
    tile_gen.inc:617; tb and TT are staged as 0 there and a is exactly 0: softmax_ref), so the sums here run over the K real slots while
    the term counts stay those of the Kp-wide loops.  ln_before=False: rmu_off_ref.  -> {"rr", "mu": (ref, bound)}, each (NT, E)"""
    if not ln_before:
        return rmu_off_ref(a.shape[0], gv.shape[0], a.device)
    s0, s1, lg, a, TT, gv = sx[0].double(), sx[1].double(), L2.double(), a.double(), TT.double(), gv.double().to(sx.device)
    NT, El, Kp, K = a.shape[0], a.shape[1], a.shape[2], TT.shape[-1]
    E = gv.shape[0]
    tb = Tsum.double() / C                                                   # :549: one rounding
    if K < Kp:
        a, lg, tb = a[..., :K], lg[..., :K], tb[..., :K]
    k = (Kp + 2) * EPS_ACC
    u1, u1m = (a * tb).sum(-1), (a * tb).abs().sum(-1)                       # :614
    eu1 = (k + U32) * u1m
    u2, u2m = (a * lg).sum(-1), (a * lg).abs().sum(-1)
    eu2 = k * u2m
    if TT.shape[0] == NT:                                                    # :621
        w, wm = torch.einsum("tlk,tlkn->tln", a, TT), torch.einsum("tlk,tlkn->tln", a.abs(), TT.abs())
    else:                                                                    # per frame (S, El, K, K): tokens are frame-major
        af = a.reshape(TT.shape[0], -1, El, K)
        w, wm = torch.einsum("snlk,slkm->snlm", af, TT).reshape(NT, El, K), torch.einsum("snlk,slkm->snlm", af.abs(), TT.abs()).reshape(NT, El, K)
    ew = (Kp * EPS_ACC + (EPS_PLANES if planes else 0.0)) * wm
    u3, u3m = (w * a).sum(-1), (wm * a.abs()).sum(-1)                        # :623
    eu3 = (a.abs() * ew).sum(-1) + k * u3m
    z = torch.zeros(NT, E - El, dtype=torch.float64, device=a.device)
    pad = lambda v: torch.cat([v, z], 1)
    u1, u1m, eu1, u2, u2m, eu2, u3, u3m, eu3 = (pad(v) for v in (u1, u1m, eu1, u2, u2m, eu2, u3, u3m, eu3))
    g = gv[None]
    Sx = s0[:, None] + g * C * u1                                            # :626: gv * C, * u1, the sum
    Sxm = s0.abs()[:, None] + g.abs() * C * u1m
    eSx = g.abs() * C * eu1 + 3 * U32 * Sxm
    Sxx = s1[:, None] + 2 * g * u2 + g * g * u3                              # :627: six roundings
    Sxxm = s1.abs()[:, None] + 2 * g.abs() * u2m + g * g * u3m
    eSxx = 2 * g.abs() * eu2 + g * g * eu3 + 6 * U32 * Sxxm
    mu = Sx / C                                                              # :636
    emu = eSx / C + U32 * Sxm / C
    var = (Sxx / C - mu * mu).clamp_min(0.0) + ln_eps                        # :637
    evar = eSxx / C + 2 * mu.abs() * emu + 4 * U32 * (Sxxm / C + (Sxm / C) ** 2 + ln_eps)
    rr = torch.rsqrt(var)
    _first_order(rr, evar, "pre_small rr")
    return {"rr": (rr, 0.5 * rr ** 3 * evar + EPS_RSQRT * rr), "mu": (mu, emu)}


def pre_lat_bwd_ref(a, L2, TT, TW, Tsum, gv, dzr, edzr, dSx, edSx, dSxx, edSxx, C, *, planes, out_bf16):
    """dL2x[:, :KL], the hop-2 block of the experts with a latent slot (tile_fast.hip:924-974, tile_stream.hip:1219-1294, tile_gen.inc:886-950,
    tile_kernels.hip:945-1010).  a, L2 (NT, El, Kp) as stored; TT (S, El, K, K), TW (S, El, Kp, g, GD): slot l's rows of TW in its expert's
    columns, [k][group][entry]; Tsum (NT, El, Kp); gv (El,); dzr (NT, g, El, GD) and dSx, dSxx (NT, El) with their error bounds: the
    register-resident forms read them back as stored (Zw, dslat: errors 0), the streamed and the any-shape form keep them in fp32 (registers /
    the wave's LDS tile: pre_small_bwd_ref's values and bounds, Zw's without its store).  The padding slots K..Kp: every kernel writes them,
    as zero (tile_gen.inc:931 leaves d = 0 and a is exactly 0 there, so :948 stores du2 * 0 + 0 * (0 - sada); tile_kernels.hip:1002-1007
    stores a literal 0): reference 0, bound 0.  -> (ref, bound), (NT, El, Kp)"""
    a, lg, TT, TW, dzr = a.double(), L2.double(), TT.double(), TW.double(), dzr.double()
    NT, El, Kp, K, GD = a.shape[0], a.shape[1], a.shape[2], TT.shape[-1], dzr.shape[-1]
    S = TT.shape[0]
    g = gv.double().to(a.device)[None]
    tb = Tsum.double() / C                                                   # :881 (:1222): one rounding
    if K < Kp:
        a, lg, tb, TW = a[..., :K], lg[..., :K], tb[..., :K], TW[:, :, :K]
    pl = EPS_PLANES if planes else 0.0
    af = a.reshape(S, -1, El, K)
    ta = torch.einsum("snlk,slkm->snlm", af, TT).reshape(NT, El, K)         # :946
    tam = torch.einsum("snlk,slkm->snlm", af.abs(), TT.abs()).reshape(NT, El, K)
    eta = (Kp * EPS_ACC + pl) * tam
    df = dzr.reshape(S, -1, dzr.shape[1], El, GD)
    twd = torch.einsum("slkic,snilc->snlk", TW, df).reshape(NT, El, K)      # :947: g * GD terms (64 at the tuned shape)
    twdm = torch.einsum("slkic,snilc->snlk", TW.abs(), df.abs()).reshape(NT, El, K)
    etwd = torch.einsum("slkic,snilc->snlk", TW.abs(), edzr.reshape(df.shape)).reshape(NT, El, K) + (_nsum(dzr.shape[1], GD) * EPS_ACC + pl) * twdm
    du1, du2, du3 = dSx * g * C, 2 * g * dSxx, g * g * dSxx                  # :941
    edu1 = edSx * g.abs() * C + 2 * U32 * du1.abs()
    edu2 = 2 * g.abs() * edSxx + U32 * du2.abs()
    edu3 = g * g * edSxx + 2 * U32 * du3.abs()
    x = lambda v: v[..., None]
    d = x(g) * twd + x(du1) * tb + x(du2) * lg + 2 * x(du3) * ta             # :954: eight roundings
    dm = x(g.abs()) * twdm + (x(du1) * tb).abs() + (x(du2) * lg).abs() + 2 * x(du3.abs()) * tam
    ed = x(g.abs()) * etwd + x(edu1) * tb.abs() + U32 * (x(du1) * tb).abs() + x(edu2) * lg.abs() + 2 * x(edu3) * tam + 2 * x(du3.abs()) * eta + 8 * U32 * dm
    sada = (a * d).sum(-1, keepdim=True)                                     # :955, :961
    sadam = (a.abs() * dm).sum(-1, keepdim=True)
    esada = (a.abs() * ed).sum(-1, keepdim=True) + (Kp + 2) * EPS_ACC * sadam
    v0 = x(du2) * a + a * (d - sada)                                         # :971: four roundings
    v0m = (x(du2) * a).abs() + a.abs() * (dm + sadam)
    pre = x(edu2) * a.abs() + a.abs() * (ed + esada) + 4 * U32 * v0m
    bound = _store(v0, pre, out_bf16)
    if K < Kp:
        pad = torch.zeros(NT, El, Kp - K, dtype=v0.dtype, device=v0.device)
        v0, bound = torch.cat([v0, pad], -1), torch.cat([bound, pad], -1)
    return v0, bound


def zprime_bf16(Z, bn1, relu):
    """z' as the Gram kernel forms it on the fly (gram.hip:94-99): act(scale * z + shift) in fp32, rounded to bf16.  The fp64 value rounds
    to the same bf16 number unless it lies within the fp32 evaluation's error of a rounding tie: only THOSE elements carry an error,
    one bf16 spacing.  -> (zb, ezb)"""
    zp, ezp, _y, _ym, _k = zprime(Z, bn1, relu)
    zb = zp.float().bfloat16().double()
    _m, ex = torch.frexp(zp)
    ulp = torch.ldexp(torch.ones_like(zp), ex - 8)                           # the bf16 spacing in zp's binade (8 significant bits)
    frac = zp.abs() / ulp
    tie = ((frac - torch.floor(frac)) - 0.5).abs() * ulp                     # distance to the nearest tie
    amb = tie <= ezp + U32 * zp.abs()                                        # (+ the detour of this reference through fp32)
    return zb, torch.where(amb, ulp, torch.zeros_like(ulp)) + torch.where(zp.abs() <= ezp, ezp, torch.zeros_like(ezp))


def gram_ref(Z, bn1, relu):
    """mz = mean_t z', Szz[g, e] = z'^T z' / NT with z' in bf16 (gram.hip:98 column sums of the rounded values, :140 bf16 x bf16 products --
    exact in fp32 -- accumulated in fp32 over NT tokens; the block partials summed and scaled by 1 / NT, :218).  -> {"mz", "Szz"}"""
    zb, ezb = zprime_bf16(Z, bn1, relu)
    nt = zb.shape[0]
    k = (nt + 2) * EPS_ACC
    mz = zb.mean(0)
    emz = k * zb.abs().mean(0) + ezb.mean(0)
    Szz = torch.einsum("tgej,tgel->gejl", zb, zb) / nt
    mag = torch.einsum("tgej,tgel->gejl", zb.abs(), zb.abs()) / nt
    e = (torch.einsum("tgej,tgel->gejl", ezb, zb.abs()) + torch.einsum("tgej,tgel->gejl", zb.abs(), ezb)) / nt
    return {"mz": (mz, emz), "Szz": (Szz, k * mag + e)}


def dgq_ref(Z, bn1, relu, w, ew, *, mirrored):
    """dGq[g, e][j][l] = sum_t bf16(w[t, e] z'[t, j]) z'[t, l] with z' in bf16: gram.hip:133 (the A fragment scaled by dSoo as STORED in
    dSooT, ew = None: the fp32 product and its bf16 rounding are reproduced exactly) or tile_stream.hip:351-360 (dSoo in registers: w is
    post_mid_bwd_ref's value with its bound ew, so the operand's bf16 rounding is one more named term).  mirrored: the streamed form
    computes the off-diagonal 16 x 16 tile once and stores its transpose below the diagonal (tile_stream.hip:419).  -> (ref, bound)"""
    zb, ezb = zprime_bf16(Z, bn1, relu)
    nt = zb.shape[0]
    wx = w.double()[:, None, :, None]
    if ew is None:
        fa = (zb.float() * wx.float()).bfloat16().double()
        efa = torch.where(ezb > 0, wx.abs() * ezb * (1 + 2 * EPS_BF16), torch.zeros_like(ezb))
    else:
        fa = zb * wx
        efa = ew[:, None, :, None] * zb.abs() + wx.abs() * ezb + (U32 + EPS_BF16) * fa.abs()
        efa = efa + EPS_BF16 * efa
    G = torch.einsum("tgej,tgel->gejl", fa, zb)
    mag = torch.einsum("tgej,tgel->gejl", fa.abs(), zb.abs())
    e = torch.einsum("tgej,tgel->gejl", efa, zb.abs()) + torch.einsum("tgej,tgel->gejl", fa.abs(), ezb) + (nt + 2) * EPS_ACC * mag
    if mirrored:
        G, e = G.clone(), e.clone()
        G[..., 16:, :16] = G[..., :16, 16:].transpose(-1, -2)
        e[..., 16:, :16] = e[..., :16, 16:].transpose(-1, -2)
    return G, e


def dgq_engine_ref(Z, bn1, relu, Zp, dSoo, edSoo, *, out_bf16, prod_eps=0.0):
    """dGq outside gram64 mode: post_small_bwd stores Zp = rnd_T(z') and Zw = rnd_T(dSoo z') (tile_fast.hip:502-504) and the engine contracts
    them over the tokens, dGq[g, e][j][l] = sum_t Zw[t, j] Zp[t, l] (moe_backward.cpp:131-136).  Zp is read AS STORED; Zw does not survive
    section 1 (pre_small_bwd rewrites the buffer), so it is the reference's dSoo (post_mid_bwd_ref, with its bound) times z', one fp32
    product and the store as named roundings.  prod_eps: the engine's error per product (fp32 operands as bf16 planes).  -> (ref, bound)"""
    zp, ezp, _y, _ym, _k = zprime(Z, bn1, relu)
    Zp = Zp.double()
    nt = Zp.shape[0]
    wx = dSoo.double()[:, None, :, None]
    zw = wx * zp
    ezw = _store(zw, edSoo[:, None, :, None] * zp.abs() + wx.abs() * ezp + U32 * zw.abs(), out_bf16)
    G = torch.einsum("tgej,tgel->gejl", zw, Zp)
    mag = torch.einsum("tgej,tgel->gejl", zw.abs(), Zp.abs())
    return G, torch.einsum("tgej,tgel->gejl", ezw, Zp.abs()) + ((nt + 2) * EPS_ACC + prod_eps) * mag


def z_map_ref(Zx, eZx, pw, epw, rr, mu, wsum, dconst, *, out_bf16, ln_before=True):
    """z = rnd_T(rr (Zx + gv pw - mu wsum) + dconst) (tile_fast.hip:651-652, tile_stream.hip:962-963) with rr, mu AS STORED (NT, E).  Z holds Zx
    only until the pass overwrites it in place, so Zx (NT, g, E, 32) is the down projection recomputed with its own bound eZx, and pw the
    latent term gv * (a . TW) with its bound (zero for the unimodal experts).  Six fp32 operations, each rounding a value no larger than
    |rr| (|Zx| + |pw| + |mu wsum|) + |dconst|.
    ln_before=False: z = rnd_T(Zx + gv pw) (the `: zr` arm of tile_fast.hip:652, tile_stream.hip:963, tile_gen.inc:662, tile_kernels.hip:361):
    the product with gv and the sum, TWO fp32 operations, no wsum / dconst term; rr, mu, wsum, dconst are not read.  -> (ref, bound)"""
    if not ln_before:
        z = Zx + pw
        return z, _store(z, eZx + epw + 2 * U32 * (Zx.abs() + pw.abs()), out_bf16)
    rr, mu = rr.double()[:, None, :, None], mu.double()[:, None, :, None]
    ws, dc = wsum.double(), dconst.double()
    z = rr * (Zx + pw - mu * ws) + dc
    pre = rr.abs() * (eZx + epw) + 6 * U32 * (rr.abs() * (Zx.abs() + pw.abs() + (mu * ws).abs()) + dc.abs())
    return z, _store(z, pre, out_bf16)
