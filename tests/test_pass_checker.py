"""tests/pass_ref.py on the CPU: an honest emulation of each per-token bottleneck-space pass stays inside its bound with room to spare, and
each of the mistakes such a kernel makes fails, naming the output and the token.  These are the conditions that make
tests/test_passes_fp64_gpu.py mean something (the model: tests/test_stream_product_checker.py).

The emulation is written HERE, from the formulas of oracle/algebra_ref.py, not taken from the library: fp32 arithmetic one operation at a
time, every sum accumulated one term at a time in a SHUFFLED order, the d x d mat-vecs with both operands as two bf16 planes and lo x lo
dropped (csrc/tile_lane.h::mmT_split), bf16 stores round-to-nearest-even.  Without stores (`out_bf16=False`: the arithmetic part of the
bound alone) it must stay below HALF of the bound (the scalar columns excepted: see the test); behind a bf16 store the whole ratio reaches 1 and no more (a correct store gets
arbitrarily close to its unit roundoff: test_stream_product_checker.py's docstring)."""
import pytest
import torch

from tests import pass_ref as R
from tests.stream_product_ref import ProductMismatch, check_bound

S, N, G, E, D, C = 4, 20, 2, 4, 32, 768          # four frames of 20 tokens: a frame is shorter than two 16-token tiles
NT = S * N
RELU = torch.tensor([True, True, False, False])  # (the cross-modal experts come first and carry the ReLU)
EPS = 1e-5
F32 = torch.float32


def _bf(x):
    return x.bfloat16().float()


def _ssum(terms, seed):
    """fp32 sum over the LAST axis, one term at a time, in a shuffled order"""
    g = torch.Generator().manual_seed(seed)
    acc = torch.zeros(terms.shape[:-1], dtype=F32)
    for k in torch.randperm(terms.shape[-1], generator=g).tolist():
        acc = acc + terms[..., k]
    return acc


def _tok(x):
    """(NT, g, E, 32) -> (NT, E, 64): a token's 64 entries of one expert as the last axis"""
    return x.permute(0, 2, 1, 3).reshape(x.shape[0], x.shape[2], -1)


def _mv(zp, M, planes, seed):
    """w[t, g, e, c] = sum_k zp[t, g, e, k] M[g, e, k, c]; planes: hi.hi + hi.lo + lo.hi of the two-plane operands, fp32 accumulation"""
    if planes:
        zh, Mh = _bf(zp), _bf(M)
        zl, Ml = _bf(zp - zh), _bf(M - Mh)
        terms = torch.cat([zh[..., :, None] * Mh, zh[..., :, None] * Ml, zl[..., :, None] * Mh], -2)      # (NT, g, E, 96, 32): exact products
    else:
        terms = zp[..., :, None] * M
    return _ssum(terms.transpose(-1, -2), seed)


def _operands(seed=0):
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s, k=1.0: k * torch.randn(*s, generator=g)
    o = dict(
        Z=_bf(rn(NT, G, E, D)), bn1=torch.stack([rn(G, E, D, k=0.1), 1.0 + 0.2 * torch.rand(G, E, D, generator=g), 1.0 + rn(G, E, D, k=0.1), rn(G, E, D, k=0.3)]),
        us=rn(G, E, D, k=0.5), vh=rn(G, E, D, k=0.3), H1p=rn(G, E), H2p=40.0 + rn(G, E).abs(), probs=torch.softmax(rn(S, E), -1),
        dAp=_bf(rn(NT, G, E, D)), dApx=rn(NT, G, E, 3), dm=rn(G, E, D, k=0.2), mdy=rn(G, E, D, k=0.05), mdyz=rn(G, E, D, k=0.05),
        wsum=rn(G, E, D, k=0.5), dconst=rn(G, E, D, k=0.1), rr=0.5 + torch.rand(NT, E, generator=g), mu=rn(NT, E, k=0.1))
    B = rn(G, E, 48, D, k=0.3)
    o["Gq"] = B.transpose(-1, -2) @ B                # symmetric positive semi-definite, as Wh^T Wh is
    o["sdSzz"] = rn(G, E, D, D, k=0.02)
    o["qv"] = o["probs"].repeat_interleave(N, 0)      # (NT, E): a frame's probabilities for each of its tokens
    return o


def _zp(o):
    y = o["Z"] * o["bn1"][2] + o["bn1"][3]
    return torch.where(RELU.view(1, 1, E, 1), y.clamp_min(0.0), y), y


def emu_post_small(o, planes, out_bf16, seed, qv=None, vh_factor=2.0, ln_post=True):
    st = _bf if out_bf16 else (lambda x: x)
    qv = o["qv"] if qv is None else qv
    zp, _ = _zp(o)
    if not ln_post:                                      # rp = 1, mup = 0, no statistics
        rp, mup = torch.ones_like(qv), torch.zeros_like(qv)
        return dict(rp=rp, mup=mup, Apost=st((qv * rp)[:, None, :, None] * zp))
    w = _mv(zp, o["Gq"], planes, seed)
    So = _ssum(_tok(zp * o["us"]), seed + 1) + (o["H1p"][0] + o["H1p"][1])
    Soo = _ssum(_tok(zp * (w + vh_factor * o["vh"])), seed + 2) + (o["H2p"][0] + o["H2p"][1])
    mup = So / C
    rp = torch.rsqrt((Soo / C - mup * mup).clamp_min(0.0) + EPS)
    return dict(rp=rp, mup=mup, Apost=st((qv * rp)[:, None, :, None] * zp))


def emu_scalar_cols(qv, rp, mup, out_bf16):
    st = _bf if out_bf16 else (lambda x: x)
    return st(torch.stack([qv * rp, -qv * rp * mup, qv], -1))


def emu_post_mid_bwd(o, rp, mup, planes, out_bf16, seed, qv=None, with_dm=True, ln_post=True, moments=True):
    st = _bf if out_bf16 else (lambda x: x)
    qv = o["qv"] if qv is None else qv
    zp, y = _zp(o)
    x = lambda v: v[:, None, :, None]
    if ln_post:
        da = o["dApx"][:, 0] + o["dApx"][:, 1]
        zz = _ssum(_tok(o["dAp"] * zp), seed)
        drp = qv * zz + qv * da[..., 0] - qv * mup * da[..., 1]
        dmup = -qv * rp * da[..., 1]
        dvarp = drp * (-0.5) * rp * rp * rp
        dSoo = dvarp / C
        dmup = dmup - 2.0 * mup * dvarp
        dSo = dmup / C
        w = _mv(zp, o["Gq"], planes, seed + 1)
        dz1 = st(x(qv * rp) * o["dAp"] + x(dSo) * o["us"] + x(dSoo) * (2.0 * w + 2.0 * o["vh"]))
    else:
        dSoo = torch.zeros_like(qv)
        dz1 = st(x(qv * rp) * o["dAp"])
    if moments:
        w2 = _mv(zp, o["sdSzz"], planes, seed + 2)
        d2 = dz1 + o["dm"] + w2 if with_dm else dz1 + w2
    else:
        d2 = dz1 + 0.0 + 0.0                             # dm = 0.f, w = 0.f
    return dict(dSoo=dSoo, dzp=torch.where(RELU.view(1, 1, E, 1) & (zp <= 0), torch.zeros_like(d2), st(d2)))


def emu_pre_small_bwd(o, dy, out_bf16, seed, experts=range(E), bn="train", ln_before=True):
    st = _bf if out_bf16 else (lambda x: x)
    mean, rstd, sc = o["bn1"][0], o["bn1"][1], o["bn1"][2]
    rr, mu = o["rr"][:, None, :, None], o["mu"][:, None, :, None]
    if bn == "train":
        dz = sc * (dy - o["mdy"] - (o["Z"] - mean) * rstd * o["mdyz"])
    else:
        dz = sc * dy if bn == "eval" else dy
    if not ln_before:                                    # rr = 1, mu = 0 without reading rmu; no sums
        zero = torch.zeros(NT)
        return dict(Zw=st(dz), dSx=torch.zeros(NT, E), dSxx=torch.zeros(NT, E), dL2x_KL=st(zero), rs2x=2.0 * zero)
    zc = (o["Z"] - o["dconst"]) * (1.0 / rr)
    sdr, sdm = _ssum(_tok(dz * zc), seed), _ssum(_tok(dz * o["wsum"]), seed + 1)
    dmu = -o["rr"] * sdm
    dvar = sdr * (-0.5) * o["rr"] * o["rr"] * o["rr"]
    dSxx = dvar / C
    dmu = dmu - 2.0 * o["mu"] * dvar
    dSx = dmu / C
    accx, accxx = torch.zeros(NT), torch.zeros(NT)
    for e in experts:
        accx, accxx = accx + dSx[:, e], accxx + dSxx[:, e]
    return dict(Zw=st(rr * dz), dSx=dSx, dSxx=dSxx, dL2x_KL=st(accx), rs2x=2.0 * accxx)


def ref_post_small(o, planes, out_bf16):
    return R.post_small_ref(o["Z"], o["bn1"], o["Gq"], o["us"], o["vh"], o["H1p"], o["H2p"], o["qv"], RELU, C, EPS, planes=planes, out_bf16=out_bf16)


def ref_post_mid_bwd(o, rp, mup, planes, out_bf16):
    return R.post_mid_bwd_ref(o["dAp"], o["dApx"], o["Z"], o["bn1"], o["Gq"], o["us"], o["vh"], o["qv"], rp, mup, o["dm"], o["sdSzz"], RELU, C,
                              planes=planes, out_bf16=out_bf16)


def ref_pre_small_bwd(o, dy, out_bf16):
    return R.pre_small_bwd_ref(dy, o["Z"], o["bn1"], o["mdy"], o["mdyz"], o["rr"], o["mu"], o["wsum"], o["dconst"], C, out_bf16=out_bf16)


def check_all(got, ref, tag):
    """every output of one pass against its (ref, bound); -> {name: worst err / bound}"""
    out = {}
    for k, v in ref.items():
        if k not in got:
            continue
        out[k] = R.check_masked(got[k], *v, f"{tag} {k}") if len(v) == 4 else check_bound(got[k], v[0], v[1], f"{tag} {k}")
    return out


@pytest.fixture(scope="module")
def ops():
    o = _operands()
    fwd = emu_post_small(o, True, True, seed=10)
    bwd = emu_post_mid_bwd(o, fwd["rp"], fwd["mup"], True, True, seed=20)
    return o, fwd, bwd


# ---- the honest emulation ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("planes", [False, True])
def test_honest_emulation_of_every_pass_passes_with_room(ops, planes):
    o, fwd, bwd = ops
    # the arithmetic alone (no stores): below half of the bound
    f32 = emu_post_small(o, planes, False, seed=1)
    r = check_all(f32, ref_post_small(o, planes, False), "post_small")
    b32 = emu_post_mid_bwd(o, f32["rp"], f32["mup"], planes, False, seed=2)
    r.update(check_all(b32, ref_post_mid_bwd(o, f32["rp"], f32["mup"], planes, False), "post_small_bwd + mid_bwd"))
    r.update(check_all(emu_pre_small_bwd(o, b32["dzp"], False, seed=3), ref_pre_small_bwd(o, b32["dzp"], False), "pre_small_bwd"))
    r["cols"] = check_bound(emu_scalar_cols(o["qv"], f32["rp"], f32["mup"], False), *R.scalar_cols_ref(o["qv"], f32["rp"], f32["mup"], out_bf16=False), "scalar columns")
    print(sorted(r.items()))
    # (the scalar columns are ONE or TWO correctly rounded products and nothing else: like a store, a single rounding reaches its unit
    # roundoff, so their arithmetic ratio is bounded by 1, not by a half; every output with a sum in it has the factor 2 of EPS_ACC to spare)
    assert r.pop("cols") <= 1.0
    assert max(r.values()) < 0.5, r
    # behind bf16 stores: at or below 1
    f16 = emu_post_small(o, planes, True, seed=4)
    r = check_all(f16, ref_post_small(o, planes, True), "post_small")
    b16 = emu_post_mid_bwd(o, f16["rp"], f16["mup"], planes, True, seed=5)
    r.update(check_all(b16, ref_post_mid_bwd(o, f16["rp"], f16["mup"], planes, True), "post_small_bwd + mid_bwd"))
    r.update(check_all(emu_pre_small_bwd(o, b16["dzp"], True, seed=6), ref_pre_small_bwd(o, b16["dzp"], True), "pre_small_bwd"))
    r["cols"] = check_bound(emu_scalar_cols(o["qv"], f16["rp"], f16["mup"], True), *R.scalar_cols_ref(o["qv"], f16["rp"], f16["mup"], out_bf16=True), "scalar columns")
    assert max(r.values()) <= 1.0, r


def test_one_plane_alone_fails(ops):
    """the 2^-16 term is that of TWO planes: the hi plane alone is 2^-9 and shows in rp"""
    o, _, _ = ops
    one = dict(o, Gq=_bf(o["Gq"]), Z=o["Z"])
    got = emu_post_small(one, False, True, seed=1)
    with pytest.raises(ProductMismatch, match="post_small rp"):
        check_all(got, ref_post_small(o, True, True), "post_small")


# ---- planted faults ---------------------------------------------------------------------------------------------------------------------
def _outputs(ops, out_bf16=True):
    """{output name: (honest result, check(result))} of the three per-token outputs"""
    o, fwd, bwd = ops
    rf, rb = ref_post_small(o, True, out_bf16), ref_post_mid_bwd(o, fwd["rp"], fwd["mup"], True, out_bf16)
    pre = emu_pre_small_bwd(o, bwd["dzp"], out_bf16, seed=30)
    rp_ = ref_pre_small_bwd(o, bwd["dzp"], out_bf16)
    return {"Apost": (fwd["Apost"], lambda x: check_bound(x, *rf["Apost"], "post_small Apost")),
            "dzp": (bwd["dzp"], lambda x: R.check_masked(x, *rb["dzp"], "post_small_bwd + mid_bwd dzp")),
            "Zw": (pre["Zw"], lambda x: check_bound(x, *rp_["Zw"], "pre_small_bwd Zw"))}


@pytest.mark.parametrize("out", ["Apost", "dzp", "Zw"])
def test_token_row_from_the_next_tile_fails(ops, out):
    """a stale ring slot: token 21's row holds token 37's (the same row of the next 16-token tile)"""
    good, check = _outputs(ops)[out]
    assert check(good) <= 1.0
    bad = good.clone()
    bad[21] = good[37]
    with pytest.raises(ProductMismatch) as e:
        check(bad)
    assert out in str(e.value) and "= (21," in str(e.value), str(e.value)


def test_last_token_of_a_frame_with_the_next_frames_probabilities_fails(ops):
    o, fwd, _ = ops
    qv = o["qv"].clone()
    t = 2 * N - 1                                        # the last token of frame 1 ...
    qv[t] = o["probs"][2]                                # ... with frame 2's router probabilities
    bad = emu_post_small(o, True, True, seed=10, qv=qv)
    with pytest.raises(ProductMismatch) as e:
        check_bound(bad["Apost"], *ref_post_small(o, True, True)["Apost"], "post_small Apost")
    assert f"= ({t}," in str(e.value), str(e.value)
    with pytest.raises(ProductMismatch) as e:
        check_bound(emu_scalar_cols(qv, fwd["rp"], fwd["mup"], True), *R.scalar_cols_ref(o["qv"], fwd["rp"], fwd["mup"], out_bf16=True), "Apost scalar columns")
    assert f"= ({t}," in str(e.value) and "scalar columns" in str(e.value)
    badb = emu_post_mid_bwd(o, fwd["rp"], fwd["mup"], True, True, seed=20, qv=qv)
    rb = ref_post_mid_bwd(o, fwd["rp"], fwd["mup"], True, True)
    with pytest.raises(ProductMismatch) as e:
        R.check_masked(badb["dzp"], *rb["dzp"], "dzp")
    assert f"= ({t}," in str(e.value)
    with pytest.raises(ProductMismatch) as e:
        check_bound(badb["dSoo"], *rb["dSoo"], "dSoo")
    assert f"= ({t}," in str(e.value) and "dSoo" in str(e.value)


@pytest.mark.parametrize("out", ["Apost", "dzp", "Zw"])
def test_two_experts_slots_swapped_fails(ops, out):
    good, check = _outputs(ops)[out]
    bad = good.clone()
    bad[50, :, 2], bad[50, :, 3] = good[50, :, 3], good[50, :, 2]
    with pytest.raises(ProductMismatch) as e:
        check(bad)
    assert out in str(e.value) and "= (50," in str(e.value)


@pytest.mark.parametrize("out", ["Apost", "dzp", "Zw"])
def test_the_two_groups_swapped_fails(ops, out):
    good, check = _outputs(ops)[out]
    bad = good.clone()
    bad[7, 0], bad[7, 1] = good[7, 1], good[7, 0]
    with pytest.raises(ProductMismatch) as e:
        check(bad)
    assert out in str(e.value) and "= (7," in str(e.value)


def test_one_token_missing_from_a_column_sum_over_3920_tokens_fails():
    """BatchNorm statistics / dsm-like: the token mean of 3 920 rows of 256 columns; token 2077 never added"""
    nt = 3920
    g = torch.Generator().manual_seed(3)
    x = _bf(torch.randn(nt, 256, generator=g))
    scale = torch.tensor(1.0, dtype=F32).div(float(nt))

    def emu(skip=()):
        order = [t for t in torch.randperm(nt, generator=torch.Generator().manual_seed(9)).tolist() if t not in skip]
        parts = []
        for s in range(16):                              # sixteen block partials, then the finalizer
            acc = torch.zeros(256)
            for t in order[s * 245:(s + 1) * 245]:
                acc = acc + x[t]
            parts.append(acc)
        acc = parts[0]
        for p in parts[1:]:
            acc = acc + p
        return acc * scale
    ref, bound = R.colsum_ref(x, 1.0 / nt)
    assert check_bound(emu(), ref, bound, "column means") < 0.5
    with pytest.raises(ProductMismatch, match="column means without token 2077"):
        check_bound(emu(skip=(2077,)), ref, bound, "column means without token 2077")


def test_vh_in_place_of_2_vh_in_Soo_fails(ops):
    o, _, _ = ops
    bad = emu_post_small(o, True, True, seed=10, vh_factor=1.0)
    with pytest.raises(ProductMismatch, match="post_small rp"):
        check_all(bad, ref_post_small(o, True, True), "post_small")


def test_dsm2_term_missing_from_mid_bwd_fails(ops):
    o, fwd, _ = ops
    bad = emu_post_mid_bwd(o, fwd["rp"], fwd["mup"], True, True, seed=20, with_dm=False)
    with pytest.raises(ProductMismatch, match="dzp"):
        R.check_masked(bad["dzp"], *ref_post_mid_bwd(o, fwd["rp"], fwd["mup"], True, True)["dzp"], "post_small_bwd + mid_bwd dzp")


def test_statistics_column_summed_over_the_latent_experts_only_fails(ops):
    o, _, bwd = ops
    ref = ref_pre_small_bwd(o, bwd["dzp"], True)
    good = emu_pre_small_bwd(o, bwd["dzp"], True, seed=30)
    assert check_bound(good["dL2x_KL"], *ref["dL2x_KL"], "pre_small_bwd dL2x[:, KL]") <= 1.0
    bad = emu_pre_small_bwd(o, bwd["dzp"], True, seed=30, experts=range(2))
    with pytest.raises(ProductMismatch, match=r"dL2x\[:, KL\]"):
        check_bound(bad["dL2x_KL"], *ref["dL2x_KL"], "pre_small_bwd dL2x[:, KL]")
    with pytest.raises(ProductMismatch, match="rs2x"):
        check_bound(bad["rs2x"], *ref["rs2x"], "pre_small_bwd rs2x")


@pytest.mark.parametrize("out", ["Apost", "dzp", "Zw"])
def test_one_element_two_bf16_ulps_off_fails(ops, out):
    good, check = _outputs(ops)[out]
    idx = (33, 1, 3, 5)                                  # (an expert without the ReLU: the element is not masked)
    assert float(good[idx]) != 0.0
    bits = good.contiguous().view(torch.int32).clone()
    bits[idx] += 2 << 16
    with pytest.raises(ProductMismatch, match="1 of") as e:
        check(bits.view(F32))
    assert "= (33, 1, 3, 5)" in str(e.value)


# ---- the ReLU kink ----------------------------------------------------------------------------------------------------------------------
def test_kink_elements_may_take_either_branch_and_are_capped(ops):
    o, fwd, bwd = ops
    rep = lambda v: v.repeat(8, *([1] * (v.dim() - 1)))                 # 640 tokens: one kink element is below the cap of 1e-5 of the tensor
    o = dict(o, **{k: rep(o[k]) for k in ("Z", "dAp", "dApx", "qv")})
    fwd = {k: rep(v) for k, v in fwd.items()}
    o2 = dict(o, Z=o["Z"].clone(), bn1=o["bn1"].clone())
    o2["bn1"][3, 0, 0, 4] = 0.0
    o2["Z"][11, 0, 0, 4] = 0.0                           # y = 0 exactly: z' = 0 whichever way the comparison falls
    ref = ref_post_mid_bwd(o2, fwd["rp"], fwd["mup"], True, True)["dzp"]
    assert int(ref[3].sum()) == 1 and bool(ref[3][11, 0, 0, 4])
    got = emu_post_mid_bwd(o2, fwd["rp"], fwd["mup"], True, True, seed=20)["dzp"]
    assert float(got[11, 0, 0, 4]) == 0.0                # (the emulation masks at y <= 0, the reference keeps y > 0: they agree here)
    assert R.check_masked(got, *ref, "dzp") <= 1.0
    other = got.clone()
    other[11, 0, 0, 4] = _bf(ref[0][11, 0, 0, 4].float())          # the other branch: the unmasked value
    assert R.check_masked(other, *ref, "dzp") <= 1.0
    other[11, 0, 0, 4] = 0.5 * other[11, 0, 0, 4] + 1e-3           # neither branch
    with pytest.raises(ProductMismatch):
        R.check_masked(other, *ref, "dzp")
    # away from the kink a wrongly masked element fails
    wrong = got.clone()
    t = int((~ref[2][:, 0, 0, 7].reshape(-1)).nonzero()[0])        # a token that the ReLU masks at (group 0, expert 0, entry 7)
    wrong[t, 0, 0, 7] = _bf(ref[0][t, 0, 0, 7].float())
    with pytest.raises(ProductMismatch):
        R.check_masked(wrong, *ref, "dzp")
    # more kink elements than the cap allows: a wrong test input
    many = torch.zeros_like(ref[3])
    many[:2] = True
    with pytest.raises(ProductMismatch, match="kink"):
        R.check_masked(got, ref[0], ref[1], ref[2], many, "dzp")


def test_cancelling_variance_is_refused_as_a_test_input(ops):
    """first order is asserted honest: an input whose LayerNorm-post variance cancels to rounding level is a wrong input, not an exclusion"""
    o, _, _ = ops
    bad = dict(o, H2p=o["H2p"] * 0.0 - 1e6, H1p=o["H1p"] * 0.0)          # Soo / C - mup^2 far below zero: clamped, var = eps against magnitudes of 1e6 / C
    with pytest.raises(AssertionError, match="1/8"):
        ref_post_small(bad, True, True)


# ---- pre_small: the softmax over a latent slot, the folded-LayerNorm statistics -----------------------------------------------------------
EL = 2


def _pre_operands(seed=40):
    g = torch.Generator().manual_seed(seed)
    T = 0.2 * torch.randn(S, EL, D, 48, generator=g)
    return dict(L2=3.0 * torch.randn(NT, EL, D, generator=g), sx=torch.stack([2.0 * torch.randn(NT, generator=g), 60.0 + 5.0 * torch.rand(NT, generator=g)]),
                TT=T @ T.transpose(-1, -2), Tsum=torch.randn(S, EL, D, generator=g), gv=torch.tensor([0.4, -0.3, 0.0, 0.0]))


def _per_token(v):
    return v.repeat_interleave(N, 0)                 # a frame's constants for each of its tokens


def emu_softmax(L2, out_bf16, seed):
    st = _bf if out_bf16 else (lambda x: x)
    ex = torch.exp2(torch.tensor(1.4426950408889634, dtype=F32) * (L2 - L2.max(-1, keepdim=True).values))
    return st(ex * (1.0 / _ssum(ex, seed))[..., None])


def emu_rmu(p, a, TT, Tsum, planes, seed):
    tb = Tsum / C
    u1, u2 = _ssum(a * tb, seed), _ssum(a * p["L2"], seed + 1)
    if planes:
        ah, Th = _bf(a), _bf(TT)
        al, Tl = _bf(a - ah), _bf(TT - Th)
        terms = torch.cat([ah[..., :, None] * Th, ah[..., :, None] * Tl, al[..., :, None] * Th], -2)
    else:
        terms = a[..., :, None] * TT
    u3 = _ssum(_ssum(terms.transpose(-1, -2), seed + 2) * a, seed + 3)
    z = torch.zeros(NT, E - EL)
    u1, u2, u3 = (torch.cat([v, z], 1) for v in (u1, u2, u3))
    gv = p["gv"][None]
    Sx = p["sx"][0][:, None] + gv * C * u1
    Sxx = p["sx"][1][:, None] + 2.0 * gv * u2 + gv * gv * u3
    mu = Sx / C
    return dict(rr=torch.rsqrt((Sxx / C - mu * mu).clamp_min(0.0) + EPS), mu=mu)


@pytest.mark.parametrize("planes", [False, True])
def test_honest_emulation_of_pre_small_passes_with_room(planes):
    p = _pre_operands()
    a32 = emu_softmax(p["L2"], False, seed=1)
    assert check_bound(a32, *R.softmax_ref(p["L2"], out_bf16=False), "pre_small a") < 0.5
    a16 = emu_softmax(p["L2"], True, seed=1)
    assert check_bound(a16, *R.softmax_ref(p["L2"], out_bf16=True), "pre_small a") <= 1.0
    TT, Ts = _per_token(p["TT"]), _per_token(p["Tsum"])
    got = emu_rmu(p, a16, TT, Ts, planes, seed=5)
    r = check_all(got, R.rmu_ref(p["sx"], p["L2"], a16, TT, Ts, p["gv"], C, EPS, planes=planes), "pre_small")
    assert max(r.values()) < 0.5, r


def test_last_token_of_a_frame_with_the_next_frames_latent_constants_fails():
    p = _pre_operands()
    a = emu_softmax(p["L2"], True, seed=1)
    TT, Ts = _per_token(p["TT"]), _per_token(p["Tsum"])
    ref = R.rmu_ref(p["sx"], p["L2"], a, TT, Ts, p["gv"], C, EPS, planes=True)
    t = 3 * N - 1                                    # the last token of frame 2 with frame 3's TT / Tsum
    for which in ("TT", "Tsum"):
        TTb, Tsb = TT.clone(), Ts.clone()
        if which == "TT":
            TTb[t] = p["TT"][3]
        else:
            Tsb[t] = p["Tsum"][3]
        got = emu_rmu(p, a, TTb, Tsb, True, seed=5)
        with pytest.raises(ProductMismatch) as e:
            check_all(got, ref, "pre_small")
        assert f"= ({t}," in str(e.value) and "pre_small" in str(e.value), (which, str(e.value))


def test_softmax_row_from_the_next_tile_and_two_ulps_fail():
    p = _pre_operands()
    a = emu_softmax(p["L2"], True, seed=1)
    ref = R.softmax_ref(p["L2"], out_bf16=True)
    bad = a.clone()
    bad[5] = a[21]
    with pytest.raises(ProductMismatch) as e:
        check_bound(bad, *ref, "pre_small a")
    assert "= (5," in str(e.value)
    bad = a.clone()
    bad[:, 0], bad[:, 1] = a[:, 1], a[:, 0]          # the two latent slots swapped
    with pytest.raises(ProductMismatch, match="pre_small a"):
        check_bound(bad, *ref, "pre_small a")
    idx = tuple(int(i) for i in (a > 0.05).nonzero()[0])
    bits = a.contiguous().view(torch.int32).clone()
    bits[idx] += 2 << 16
    with pytest.raises(ProductMismatch, match="1 of"):
        check_bound(bits.view(F32), *ref, "pre_small a")


def test_bn1_statistics_and_one_token_missing():
    """bn1 (mean, rstd, scale, shift) from fp32 column sums over 3 920 tokens; one token never added shows in the mean"""
    nt = 3920
    g = torch.Generator().manual_seed(8)
    Z = _bf(0.2 + torch.randn(nt, G, 2, D, generator=g))
    w, b = 1.0 + 0.1 * torch.randn(G, 2, D, generator=g), 0.1 * torch.randn(G, 2, D, generator=g)

    def emu(skip=()):
        keep = [t for t in torch.randperm(nt, generator=torch.Generator().manual_seed(2)).tolist() if t not in skip]
        s0, s1 = torch.zeros(G, 2, D), torch.zeros(G, 2, D)
        for t in keep:
            s0, s1 = s0 + Z[t], s1 + Z[t] * Z[t]
        m = s0.double() / nt
        v = (s1.double() / nt - m * m).clamp_min(0.0)
        mean, var = m.float(), v.float()
        rstd = torch.rsqrt(var + 1e-5)
        sc = w * rstd
        return torch.stack([mean, rstd, sc, b - mean * sc])
    ref, bound = R.bn1_ref(Z, w, b, 1e-5)
    assert check_bound(emu(), ref, bound, "bn1") < 0.5
    with pytest.raises(ProductMismatch, match="bn1 without token 77"):
        check_bound(emu(skip=(77,)), ref, bound, "bn1 without token 77")


# ---- the hop-2 block of the backward: dL2x[:, :KL] -------------------------------------------------------------------------------------
def _mv_tok(v, M, planes, seed):
    """w[t, l, n] = sum_k v[t, l, k] M[t, l, k, n] with per-token matrices; planes as _mv"""
    if planes:
        vh, Mh = _bf(v), _bf(M)
        vl, Ml = _bf(v - vh), _bf(M - Mh)
        terms = torch.cat([vh[..., :, None] * Mh, vh[..., :, None] * Ml, vl[..., :, None] * Mh], -2)
    else:
        terms = v[..., :, None] * M
    return _ssum(terms.transpose(-1, -2), seed)


def emu_pre_lat(p, a, TT, TW, Ts, dzr, dSx, dSxx, planes, out_bf16, seed):
    """TT (NT, El, 32, 32), TW (NT, El, 32, g, 32) per token; dzr (NT, g, El, 32)"""
    st = _bf if out_bf16 else (lambda x: x)
    gv = p["gv"][:EL][None]
    tb = Ts / C
    ta = _mv_tok(a, TT, planes, seed)
    dflat = dzr.permute(0, 2, 1, 3).reshape(NT, EL, G * D)                               # [group][entry] as the contraction index
    twd = _mv_tok(dflat, TW.reshape(NT, EL, D, G * D).transpose(-1, -2), planes, seed + 1)
    du1, du2, du3 = dSx * gv * C, 2.0 * gv * dSxx, gv * gv * dSxx
    x = lambda v: v[..., None]
    d = x(gv) * twd + x(du1) * tb + x(du2) * p["L2"] + 2.0 * x(du3) * ta
    sada = _ssum(a * d, seed + 2)
    return st(x(du2) * a + a * (d - x(sada)))


def _lat_operands():
    p = _pre_operands()
    g = torch.Generator().manual_seed(41)
    a = emu_softmax(p["L2"], True, seed=1)
    TW = 0.3 * torch.randn(S, EL, D, G, D, generator=g)
    dzr = _bf(0.5 * torch.randn(NT, G, EL, D, generator=g))
    dSx, dSxx = 1e-3 * torch.randn(NT, EL, generator=g), 1e-3 * torch.randn(NT, EL, generator=g)
    return p, a, TW, dzr, dSx, dSxx


def _lat_ref(p, a, TW, dzr, dSx, dSxx, planes, out_bf16):
    zero = torch.zeros(NT, EL, dtype=torch.float64)
    return R.pre_lat_bwd_ref(a, p["L2"], p["TT"], TW, _per_token(p["Tsum"]), p["gv"][:EL], dzr, torch.zeros(NT, G, EL, D, dtype=torch.float64),
                             dSx.double(), zero, dSxx.double(), zero, C, planes=planes, out_bf16=out_bf16)


@pytest.mark.parametrize("planes", [False, True])
def test_honest_emulation_of_the_hop2_block_passes_with_room(planes):
    p, a, TW, dzr, dSx, dSxx = _lat_operands()
    args = (p, a, _per_token(p["TT"]), _per_token(TW), _per_token(p["Tsum"]), dzr, dSx, dSxx, planes)
    assert check_bound(emu_pre_lat(*args, False, seed=3), *_lat_ref(p, a, TW, dzr, dSx, dSxx, planes, False), "pre_lat_bwd dL2x[:, :KL]") < 0.5
    assert check_bound(emu_pre_lat(*args, True, seed=3), *_lat_ref(p, a, TW, dzr, dSx, dSxx, planes, True), "pre_lat_bwd dL2x[:, :KL]") <= 1.0


def test_hop2_block_faults_fail():
    p, a, TW, dzr, dSx, dSxx = _lat_operands()
    ref = _lat_ref(p, a, TW, dzr, dSx, dSxx, True, True)
    TT, TWt, Ts = _per_token(p["TT"]), _per_token(TW), _per_token(p["Tsum"])
    good = emu_pre_lat(p, a, TT, TWt, Ts, dzr, dSx, dSxx, True, True, seed=3)
    t = 2 * N - 1                                    # the last token of frame 1 with frame 2's TW
    TWb = TWt.clone()
    TWb[t] = TW[2]
    with pytest.raises(ProductMismatch) as e:
        check_bound(emu_pre_lat(p, a, TT, TWb, Ts, dzr, dSx, dSxx, True, True, seed=3), *ref, "pre_lat_bwd dL2x[:, :KL]")
    assert f"= ({t}," in str(e.value) and "dL2x" in str(e.value)
    bad = good.clone()
    bad[21] = good[37]                               # a stale ring slot
    with pytest.raises(ProductMismatch) as e:
        check_bound(bad, *ref, "pre_lat_bwd dL2x[:, :KL]")
    assert "= (21," in str(e.value)
    bad = good.clone()
    bad[:, 0], bad[:, 1] = good[:, 1], good[:, 0]    # the two latent slots swapped
    with pytest.raises(ProductMismatch, match="dL2x"):
        check_bound(bad, *ref, "pre_lat_bwd dL2x[:, :KL]")
    idx = tuple(int(i) for i in (good.abs() > 1e-3).nonzero()[0])
    bits = good.contiguous().view(torch.int32).clone()
    bits[idx] += 2 << 16
    with pytest.raises(ProductMismatch, match="1 of"):
        check_bound(bits.view(F32), *ref, "pre_lat_bwd dL2x[:, :KL]")


def test_gram_moments_and_one_token_missing():
    """mz / Szz from z' rounded to bf16 as the Gram kernel forms it: bf16 products are exact in fp32, so the bound is the accumulation's
    alone (+ one bf16 spacing for the rare element at a rounding tie) -- one token of 3 920 never added shows"""
    nt = 3920
    g = torch.Generator().manual_seed(6)
    Z = _bf(torch.randn(nt, G, E, D, generator=g))
    bn1 = torch.stack([torch.zeros(G, E, D), torch.ones(G, E, D), 1.0 + 0.1 * torch.randn(G, E, D, generator=g), 0.3 * torch.randn(G, E, D, generator=g)])
    ref = R.gram_ref(Z, bn1, RELU)
    y = Z * bn1[2] + bn1[3]
    zb = _bf(torch.where(RELU.view(1, 1, E, 1), y.clamp_min(0.0), y))
    acc, s0 = torch.zeros(G, E, D, D), torch.zeros(G, E, D)
    for t in torch.randperm(nt, generator=g).tolist():
        acc, s0 = acc + zb[t][..., :, None] * zb[t][..., None, :], s0 + zb[t]
    inv = torch.tensor(1.0, dtype=F32).div(float(nt))
    assert check_bound(acc * inv, *ref["Szz"], "Szz") < 0.5 and check_bound(s0 * inv, *ref["mz"], "mz") < 0.5
    with pytest.raises(ProductMismatch, match="Szz without token 77"):
        check_bound((acc - zb[77][..., :, None] * zb[77][..., None, :]) * inv, *ref["Szz"], "Szz without token 77")
    zs = zb.clone()                                      # the two groups swapped in every token
    zs[:, 0], zs[:, 1] = zb[:, 1], zb[:, 0]
    with pytest.raises(ProductMismatch, match="mz"):
        check_bound(zs.sum(0) * inv, *ref["mz"], "mz")


def test_weighted_gram_product_and_a_wrong_mirror_tile():
    nt = 640
    g = torch.Generator().manual_seed(12)
    Z = _bf(torch.randn(nt, G, E, D, generator=g))
    bn1 = torch.stack([torch.zeros(G, E, D), torch.ones(G, E, D), 1.0 + 0.1 * torch.randn(G, E, D, generator=g), 0.3 * torch.randn(G, E, D, generator=g)])
    w = 1e-3 * torch.randn(nt, E, generator=g)
    y = Z * bn1[2] + bn1[3]
    zb = _bf(torch.where(RELU.view(1, 1, E, 1), y.clamp_min(0.0), y))
    fa = _bf(zb * w[:, None, :, None])
    acc = torch.zeros(G, E, D, D)
    for t in torch.randperm(nt, generator=g).tolist():
        acc = acc + fa[t][..., :, None] * zb[t][..., None, :]
    ref = R.dgq_ref(Z, bn1, RELU, w, None, mirrored=False)
    assert check_bound(acc, *ref, "dGq") < 0.5
    mir = acc.clone()
    mir[..., 16:, :16] = acc[..., :16, 16:].transpose(-1, -2)
    assert check_bound(mir, *R.dgq_ref(Z, bn1, RELU, w, torch.zeros(nt, E, dtype=torch.float64), mirrored=True), "dGq (streamed)") <= 1.0
    bad = mir.clone()
    bad[..., 16:, :16] = acc[..., :16, 16:]              # the mirror tile stored without its transpose
    with pytest.raises(ProductMismatch, match="dGq"):
        check_bound(bad, *R.dgq_ref(Z, bn1, RELU, w, torch.zeros(nt, E, dtype=torch.float64), mirrored=True), "dGq (streamed)")
    with pytest.raises(ProductMismatch, match="dGq"):
        check_bound(acc - fa[5][..., :, None] * zb[5][..., None, :], *ref, "dGq without token 5")


def test_engine_path_dgq_and_z_map():
    """dGq outside gram64 mode (Zw = rnd(dSoo z') against the stored Zp) and z through its defining map: the honest emulation passes, one
    token missing from the contraction / the dconst term dropped / a token row from the next tile fail"""
    nt = 640
    g = torch.Generator().manual_seed(14)
    Z = _bf(torch.randn(nt, G, E, D, generator=g))
    bn1 = torch.stack([torch.zeros(G, E, D), torch.ones(G, E, D), 1.0 + 0.1 * torch.randn(G, E, D, generator=g), 0.3 * torch.randn(G, E, D, generator=g)])
    w = 1e-3 * torch.randn(nt, E, generator=g)
    y = Z * bn1[2] + bn1[3]
    zp = torch.where(RELU.view(1, 1, E, 1), y.clamp_min(0.0), y)
    Zp, Zw = _bf(zp), _bf(w[:, None, :, None] * zp)
    acc = torch.zeros(G, E, D, D)
    for t in torch.randperm(nt, generator=g).tolist():
        acc = acc + Zw[t][..., :, None] * Zp[t][..., None, :]
    ref = R.dgq_engine_ref(Z, bn1, RELU, Zp, w, torch.zeros(nt, E, dtype=torch.float64), out_bf16=True)
    assert check_bound(acc, *ref, "dGq (engine)") <= 1.0
    with pytest.raises(ProductMismatch, match="dGq"):
        check_bound(acc - 40.0 * Zw[5][..., :, None] * Zp[5][..., None, :], *ref, "dGq (engine) with token 5 off")
    with pytest.raises(ProductMismatch, match="dGq"):
        check_bound(acc.flip(0), *ref, "dGq (engine), groups swapped")
    # z map
    Zx = _bf(torch.randn(nt, G, E, D, generator=g))
    pw = 0.1 * torch.randn(nt, G, E, D, generator=g)
    rr, mu = 0.5 + torch.rand(nt, E, generator=g), 0.1 * torch.randn(nt, E, generator=g)
    ws, dc = 0.5 * torch.randn(G, E, D, generator=g), 0.3 * torch.randn(G, E, D, generator=g)
    x = lambda v: v[:, None, :, None]
    zero = torch.zeros(nt, G, E, D, dtype=torch.float64)
    zref = R.z_map_ref(Zx.double(), zero, pw.double(), zero, rr, mu, ws, dc, out_bf16=True)
    good = _bf(x(rr) * ((Zx + pw) - x(mu) * ws) + dc)
    assert check_bound(good, *zref, "z") <= 1.0
    assert check_bound(x(rr) * ((Zx + pw) - x(mu) * ws) + dc, *R.z_map_ref(Zx.double(), zero, pw.double(), zero, rr, mu, ws, dc, out_bf16=False), "z") < 0.5
    with pytest.raises(ProductMismatch, match="z without dconst"):
        check_bound(_bf(x(rr) * ((Zx + pw) - x(mu) * ws)), *zref, "z without dconst")
    bad = good.clone()
    bad[21] = good[37]
    with pytest.raises(ProductMismatch) as e:
        check_bound(bad, *zref, "z")
    assert "= (21," in str(e.value)


# ---- the switches: ln_before, ln_post, use_gate, use_bn off and eval mode ---------------------------------------------------------------------
# Every switch is a run-time branch inside every form of every pass; tests/pass_ref.py carries one argument per branch and
# tests/test_pass_variants_fp64_gpu.py holds the kernels to them.  Here: the honest emulation of each of that module's seven variants stays
# inside the new bounds in two summation orders, each planted fault fails its tag, and the seeds keep the oracle clear of the ReLU kink.
from tests.pass_variant_cases import SITES, VARIANTS, kink_clearance      # noqa: E402

BN_EPS = 1e-5


def _variant_flags(variant):
    fields, training = VARIANTS[variant]
    use_bn = fields.get("use_bn", True)
    return dict(ln_before=fields.get("ln_before", True), ln_post=fields.get("ln_post", True), use_gate=fields.get("use_gate", True),
                bn="off" if not use_bn else ("train" if training else "eval"), moments=use_bn and training)


def _bn_params(seed=50):
    """BatchNorm-1 weight, bias and running statistics as O.init_params(randomize=True) draws them: means in +-0.2, variances in [0.5, 1.5]"""
    g = torch.Generator().manual_seed(seed)
    return dict(w=1.0 + 0.1 * torch.randn(G, E, D, generator=g), b=0.3 * torch.randn(G, E, D, generator=g),
                rm=0.4 * torch.rand(G, E, D, generator=g) - 0.2, rv=0.5 + torch.rand(G, E, D, generator=g))


def emu_bn1(p, mode, eps=BN_EPS, mean=None, var=None, scale=None):
    """bn1_finalize_col's eval and no-BatchNorm arms (fwd_kernels.hip:1051, :1068-1071) in fp32, one operation at a time; mean / var / scale:
    a planted fault's replacement"""
    if mode == "off":
        z, o = torch.zeros(G, E, D), torch.ones(G, E, D)
        return torch.stack([z, o, o if scale is None else scale, z])
    mean = p["rm"] if mean is None else mean
    var = p["rv"] if var is None else var
    rstd = torch.rsqrt(var + torch.tensor(eps, dtype=F32))
    sc = p["w"] * rstd
    return torch.stack([mean, rstd, sc, p["b"] - mean * sc])


def ref_bn1(p, mode, Z=None):
    return R.bn1_ref(Z, p["w"], p["b"], BN_EPS, mode=mode, rm=p["rm"], rv=p["rv"])


# The operands are the synthetic tuned-width ones of _operands(), not the GPU sites' own, and tests/gen_pass_emu.py is not taught the switches:
# every arm a switch adds is element-wise or exact (a product with scale, a sum with gv * pw, a stored constant, a literal zero).  None
# holds a sum whose term count depends on g, dgp or Kp, none runs a mat-vec, so no new bound has a width in it; the sums and mat-vecs of the
# arms that stay on are the train-mode ones, which tests/test_gen_pass_checker.py already emulates at the generalised widths.
def _variant_operands(variant, seed=0):
    """the operands of _operands() with bn1 as the variant's BatchNorm mode leaves it"""
    f = _variant_flags(variant)
    o = _operands(seed)
    if f["bn"] != "train":
        o["bn1"] = emu_bn1(_bn_params(), f["bn"])
    return o, f


def _run_variant(o, f, planes, out_bf16, seed):
    """forward, post_small_bwd + mid_bwd, pre_small_bwd of one variant -> {output: worst err / bound}"""
    fwd = emu_post_small(o, planes, out_bf16, seed=seed, ln_post=f["ln_post"])
    r = check_all(fwd, R.post_small_ref(o["Z"], o["bn1"], o["Gq"], o["us"], o["vh"], o["H1p"], o["H2p"], o["qv"], RELU, C, EPS, planes=planes, out_bf16=out_bf16,
                                        ln_post=f["ln_post"]), "post_small")
    r["cols"] = check_bound(emu_scalar_cols(o["qv"], fwd["rp"], fwd["mup"], out_bf16), *R.scalar_cols_ref(o["qv"], fwd["rp"], fwd["mup"], out_bf16=out_bf16, ln_post=f["ln_post"]),
                            "Apost scalar columns")
    bwd = emu_post_mid_bwd(o, fwd["rp"], fwd["mup"], planes, out_bf16, seed=seed + 10, ln_post=f["ln_post"], moments=f["moments"])
    rb = R.post_mid_bwd_ref(o["dAp"], o["dApx"], o["Z"], o["bn1"], o["Gq"], o["us"], o["vh"], o["qv"], fwd["rp"], fwd["mup"], o["dm"] if f["moments"] else None,
                            o["sdSzz"] if f["moments"] else None, RELU, C, planes=planes, out_bf16=out_bf16, ln_post=f["ln_post"], moments=f["moments"])
    r.update({"b_" + k: v for k, v in check_all(bwd, rb, "post_small_bwd + mid_bwd").items()})
    train = f["bn"] == "train"
    pre = emu_pre_small_bwd(o, bwd["dzp"], out_bf16, seed=seed + 20, bn=f["bn"], ln_before=f["ln_before"])
    rp_ = R.pre_small_bwd_ref(bwd["dzp"], o["Z"], o["bn1"], o["mdy"] if train else None, o["mdyz"] if train else None, o["rr"], o["mu"], o["wsum"], o["dconst"], C,
                              out_bf16=out_bf16, bn=f["bn"], ln_before=f["ln_before"])
    r.update({"p_" + k: v for k, v in check_all(pre, rp_, "pre_small_bwd").items()})
    return r, fwd, bwd, pre


@pytest.mark.parametrize("planes", [False, True])
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_honest_emulation_of_every_variant_stays_inside_its_bounds_in_two_orders(variant, planes):
    """(an output that is ONE correctly rounded operation, or exact, reaches its bound or has none: the ratio is bounded by 1, not by a half)"""
    o, f = _variant_operands(variant)
    for out_bf16 in (False, True):
        for seed in (1, 101):                            # two summation orders
            r, fwd, _bwd, pre = _run_variant(o, f, planes, out_bf16, seed)
            assert max(r.values()) <= 1.0, (variant, out_bf16, seed, r)
            if not f["ln_post"]:
                assert bool((fwd["rp"] == 1).all() and (fwd["mup"] == 0).all())
                R.neg_zero(emu_scalar_cols(o["qv"], fwd["rp"], fwd["mup"], out_bf16)[..., 1], "Apost middle scalar column")
            if not f["ln_before"]:
                assert bool((pre["rs2x"] == 0).all() and (pre["dL2x_KL"] == 0).all() and (pre["dSx"] == 0).all())


def test_bn1_eval_and_off_references():
    p = _bn_params()
    assert check_bound(emu_bn1(p, "eval"), *ref_bn1(p, "eval"), "bn1 (eval)") <= 1.0
    ref, bound = ref_bn1(p, "off")
    assert float(bound.max()) == 0.0 and check_bound(emu_bn1(p, "off"), ref, bound, "bn1 (off)") == 0.0
    assert torch.equal(ref, torch.stack([torch.zeros(G, E, D), torch.ones(G, E, D), torch.ones(G, E, D), torch.zeros(G, E, D)]).double())
    rr = R.rmu_off_ref(NT, E, "cpu")
    assert bool((rr["rr"][0] == 1).all() and (rr["mu"][0] == 0).all() and (rr["rr"][1] == 0).all() and (rr["mu"][1] == 0).all())


# ---- planted faults, one per branch -------------------------------------------------------------------------------------------------------------
def test_eval_backward_that_keeps_the_batch_mean_terms_fails():
    o, f = _variant_operands("eval")
    _r, _fwd, bwd, _pre = _run_variant(o, f, True, True, 1)
    bad = emu_pre_small_bwd(o, bwd["dzp"], True, seed=21, bn="train")                    # - mdy - zh * mdyz kept
    ref = R.pre_small_bwd_ref(bwd["dzp"], o["Z"], o["bn1"], None, None, o["rr"], o["mu"], o["wsum"], o["dconst"], C, out_bf16=True, bn="eval")
    with pytest.raises(ProductMismatch, match="P9 Zw"):
        check_bound(bad["Zw"], *ref["Zw"], "P9 Zw")


@pytest.mark.parametrize("fault", ["batch statistics", "no eps"])
def test_eval_bn1_from_the_batch_statistics_or_without_eps_fails(fault):
    p = _bn_params()
    o = _operands()
    if fault == "batch statistics":
        z = o["Z"]
        bad = emu_bn1(p, "eval", mean=z.mean(0), var=z.var(0, unbiased=False))
    else:
        bad = emu_bn1(p, "eval", eps=0.0)
    with pytest.raises(ProductMismatch, match="P2 bn1"):
        check_bound(bad, *ref_bn1(p, "eval"), "P2 bn1")


def test_scale_w_without_batchnorm_fails():
    p = _bn_params()
    with pytest.raises(ProductMismatch, match="P2 bn1"):
        check_bound(emu_bn1(p, "off", scale=p["w"]), *ref_bn1(p, "off"), "P2 bn1")


def test_stale_rr_without_layernorm_before_fails():
    o, f = _variant_operands("no_ln_before")
    _r, _fwd, bwd, pre = _run_variant(o, f, True, True, 1)
    ref = R.pre_small_bwd_ref(bwd["dzp"], o["Z"], o["bn1"], o["mdy"], o["mdyz"], o["rr"], o["mu"], o["wsum"], o["dconst"], C, out_bf16=True, ln_before=False)
    assert check_bound(pre["Zw"], *ref["Zw"], "P9 Zw") <= 1.0
    bad = _bf(o["rr"][:, None, :, None] * pre["Zw"])                                     # Zw = rr * dz with the rr some earlier site left in rmu
    with pytest.raises(ProductMismatch, match="P9 Zw"):
        check_bound(bad, *ref["Zw"], "P9 Zw")


def test_nonzero_rs2x_without_layernorm_before_fails():
    o, f = _variant_operands("bare")
    _r, _fwd, bwd, pre = _run_variant(o, f, True, True, 1)
    ref = R.pre_small_bwd_ref(bwd["dzp"], o["Z"], o["bn1"], None, None, o["rr"], o["mu"], o["wsum"], o["dconst"], C, out_bf16=True, bn="off", ln_before=False)
    bad = pre["rs2x"].clone()
    bad[33] = 1e-30
    with pytest.raises(ProductMismatch, match=r"P9 rs2x.*= \(33,\)"):
        check_bound(bad, *ref["rs2x"], "P9 rs2x")


def test_rp_from_a_layernorm_that_is_off_fails():
    o, f = _variant_operands("no_ln_post")
    ref = R.post_small_ref(o["Z"], o["bn1"], o["Gq"], o["us"], o["vh"], o["H1p"], o["H2p"], o["qv"], RELU, C, EPS, planes=True, out_bf16=True, ln_post=False)
    bad = emu_post_small(o, True, True, seed=1, ln_post=True)
    for k in ("rp", "mup", "Apost"):
        with pytest.raises(ProductMismatch, match=f"P4 {k}"):
            check_bound(bad[k], *ref[k], f"P4 {k}")


@pytest.mark.parametrize("variant", ["no_gate", "eval"])
def test_gate_applied_in_token_space_fails(variant):
    """no_gate: the gate applied with use_gate off.  eval (gate on): the plan folds the gate into Bpost (Dims::gate_w), so a kernel that
    multiplies it in as well applies it twice.  Either way q must be probs as stored, and the third scalar column is q itself."""
    o, f = _variant_operands(variant)
    gate = torch.tensor([0.9, 1.1, 0.8, 1.2])
    qbad = o["qv"] * gate
    ref = R.post_small_ref(o["Z"], o["bn1"], o["Gq"], o["us"], o["vh"], o["H1p"], o["H2p"], o["qv"], RELU, C, EPS, planes=True, out_bf16=True, ln_post=f["ln_post"])
    good = emu_post_small(o, True, True, seed=1, ln_post=f["ln_post"])
    bad = emu_post_small(o, True, True, seed=1, qv=qbad, ln_post=f["ln_post"])
    assert check_bound(good["Apost"], *ref["Apost"], "P4 Apost") <= 1.0
    with pytest.raises(ProductMismatch, match="P4 Apost"):
        check_bound(bad["Apost"], *ref["Apost"], "P4 Apost")
    cols = R.scalar_cols_ref(o["qv"], good["rp"], good["mup"], out_bf16=True, ln_post=f["ln_post"])
    with pytest.raises(ProductMismatch, match="scalar columns"):
        check_bound(emu_scalar_cols(qbad, good["rp"], good["mup"], True), *cols, "P4 Apost scalar columns")
    with pytest.raises(ProductMismatch, match="scalar columns"):                        # ... and the third column alone shows it
        check_bound(emu_scalar_cols(qbad, good["rp"], good["mup"], True)[..., 2], cols[0][..., 2], cols[1][..., 2], "P4 Apost scalar columns [q]")


def test_one_token_with_the_neighbouring_experts_running_mean_fails():
    o, f = _variant_operands("eval")
    p = _bn_params()
    ref = R.post_small_ref(o["Z"], o["bn1"], o["Gq"], o["us"], o["vh"], o["H1p"], o["H2p"], o["qv"], RELU, C, EPS, planes=True, out_bf16=True)
    good = emu_post_small(o, True, True, seed=1)
    assert check_bound(good["Apost"], *ref["Apost"], "P4 Apost") <= 1.0
    t, e = 47, 2
    other = emu_bn1(p, "eval", mean=p["rm"].roll(1, 1))                                  # every expert with its neighbour's running mean
    o2 = dict(o, bn1=o["bn1"].clone())
    o2["bn1"][3, :, e] = other[3, :, e]
    wrong = emu_post_small(o2, True, True, seed=1)
    bad = good["Apost"].clone()
    bad[t, :, e] = wrong["Apost"][t, :, e]
    with pytest.raises(ProductMismatch) as x:
        check_bound(bad, *ref["Apost"], "P4 Apost")
    assert f"= ({t}," in str(x.value) and "P4 Apost" in str(x.value), str(x.value)


@pytest.mark.parametrize("variant", ["no_ln_post", "bare"])
def test_one_bf16_ulp_in_apost_fails(variant):
    o, f = _variant_operands(variant)
    ref, bound = R.post_small_ref(o["Z"], o["bn1"], o["Gq"], o["us"], o["vh"], o["H1p"], o["H2p"], o["qv"], RELU, C, EPS, planes=True, out_bf16=True, ln_post=False)["Apost"]
    good = emu_post_small(o, True, True, seed=1, ln_post=False)["Apost"]
    assert check_bound(good, ref, bound, "P4 Apost") <= 1.0
    idx = (33, 1, 3, 5)                                  # (an expert without the ReLU)
    assert float(good[idx]) != 0.0
    bits = good.contiguous().view(torch.int32).clone()
    away = (good[idx].double() >= ref[idx]) == (good[idx] > 0)                           # one ulp AWAY from the reference
    bits[idx] += (1 << 16) if away else -(1 << 16)
    with pytest.raises(ProductMismatch, match="1 of") as x:
        check_bound(bits.view(F32), ref, bound, "P4 Apost")
    assert "= (33, 1, 3, 5)" in str(x.value)


def test_a_running_statistic_changed_by_an_eval_forward_fails():
    p = _bn_params()
    R.state_unchanged(p["rv"].clone(), p["rv"], "bn1.running_var")
    R.state_unchanged(torch.tensor(7), torch.tensor(7), "bn1.num_batches_tracked")
    bits = p["rv"].clone().view(torch.int32)
    bits[1, 2, 3] += 1                                   # one fp32 ulp in one entry
    with pytest.raises(ProductMismatch, match="running_var"):
        R.state_unchanged(bits.view(F32), p["rv"], "bn1.running_var")
    with pytest.raises(ProductMismatch, match="num_batches_tracked"):
        R.state_unchanged(torch.tensor(8), torch.tensor(7), "bn1.num_batches_tracked")


def test_negative_zero_is_told_from_positive_zero():
    R.neg_zero(torch.full((4, 3), -0.0), "middle column")
    R.neg_zero(torch.full((4, 3), -0.0).bfloat16().float(), "middle column")
    with pytest.raises(ProductMismatch, match="middle column"):
        R.neg_zero(torch.zeros(4, 3), "middle column")


# ---- the seeds of the variant sites ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_the_seeds_keep_the_oracles_variants_clear_of_the_relu_kink(variant):
    """the criterion of tests/test_gen_pass_checker.py at every site of tests/test_pass_variants_fp64_gpu.py, in the variant's BatchNorm mode: the
    oracle's own fp32 pre-activation has nothing within 16 kink windows, so the reference alone satisfies KINK_CAP (0 elements at these sizes)"""
    seen = {}
    for site, (_form, what, _bf16, _hook) in SITES.items():
        if what not in seen:
            seen[what] = kink_clearance(site, variant, R.KINK)
            print(f"{variant} {what}: nearest ReLU pre-activation at {seen[what]:.1f} kink windows")
    assert min(seen.values()) > 16.0, seen
