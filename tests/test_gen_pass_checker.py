"""What tests/test_gen_passes_fp64_gpu.py rests on, shown without a GPU.

1. The table of tests/gen_pass_cases.py: the plan puts every case on the kernel family and (NG, NCG, KC) instance it is meant for, with the
   rounds of resident experts, idle waves and dynamic LDS the case names (the layout comes from the library's buffer table; the rounds from
   the transcription of pick_round beside the table).
2. The seeds: the oracle's own fp32 z keeps every ReLU pre-activation 16 kink windows away from 0 at every case but many_blocks, and out
   of the window itself there.
3. tests/pass_ref.py takes its widths from its operands now: at the tuned shape every ref and every bound is BIT-IDENTICAL to the module as
   it stood with 32 spelled out (tests/pass_ref_tuned.py), on the operands of tests/test_pass_checker.py.
4. The GPU module's own checks (`_forward`, `_backward`) run here on tests/gen_pass_emu.py::EmuSite -- a torch fp32 emulation of each map in the
   workspace layout, operands from the oracle's forward and backward -- at four shapes of the table in both types: the honest emulation
   stays inside every bound in two summation orders (two bf16 planes where the form has them), and each fault such a kernel can make
   fails the check of the pass it is in."""
import copy

import pytest
import torch

from tests import pass_ref as R
from tests import pass_ref_tuned as R0
from tests import test_gen_passes_fp64_gpu as G
from tests import test_pass_checker as C0
from tests.gen_pass_cases import BF16_CASES, CASES, case_config, plan_layout, rounds
from tests.gen_pass_emu import EmuSite

FWD, BWD = {"k_pre_small", "k_mid", "k_post_small"}, {"k_post_small_bwd", "k_mid_bwd", "k_pre_small_bwd"}
EMU_CASES = ("g2c1_k8_e5", "g4c2_k87_e8", "merged_k2", "kt_three_groups_50")      # (the ragged one of the two any-shape sites)

# case -> {kernel: (experts resident R, rounds, idle waves in the last round, rounds in grid.z)}: pick_round's answers worked out by hand from
# lds_floats_pre_parts and the launchers (13 KB per wave: pe + pw <= 3328 floats at NS = 1, 2 pe + 4 pw <= 13312 at R = 2)
ROUNDS = {
    "g2c1_k8_e5": {"pre_small": (5, 1, 0, True), "post_small": (5, 1, 0, True), "pre_small_bwd": (5, 1, 0, False), "pre_lat_bwd": (2, 1, 0, True)},
    "g2c3_k32_e6": {"pre_small": (2, 3, 0, True), "post_small": (2, 3, 0, True), "mid_bwd": (2, 3, 0, True), "mid": (6, 1, 0, True), "pre_lat_bwd": (2, 2, 1, True)},
    "g2c3_k20_v2": {"pre_small": (1, 4, 0, True), "pre_lat_bwd": (1, 4, 0, True)},
    "g4c2_k87_e8": {"pre_small": (1, 8, 0, True), "mid": (4, 2, 0, True), "post_small": (2, 4, 0, True), "pre_small_bwd": (4, 2, 0, False)},
    "g2c6_k87": {"pre_small": (1, 8, 0, True), "post_small": (1, 8, 0, True), "pre_small_bwd": (4, 2, 0, False)},
    "pad40_k87": {"post_small": (2, 4, 1, True), "post_small_bwd": (2, 4, 1, True), "mid_bwd": (2, 4, 1, True), "pre_small_bwd": (7, 1, 0, False)},
    "merged_k2": {"pre_small": (3, 1, 0, True), "post_small": (3, 1, 0, True)},
    "short_36": {"pre_small": (1, 3, 0, True), "post_small": (1, 3, 0, True), "pre_small_bwd": (1, 3, 0, False)},
    "tiny_3": {"pre_small": (1, 4, 0, True), "pre_lat_bwd": (1, 2, 0, True)},
    "many_blocks": {"post_small": (2, 4, 1, False), "post_small_bwd": (2, 4, 1, False), "mid_bwd": (2, 4, 1, False), "pre_small": (7, 1, 0, False)},
}


# ---- 1. the table ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(CASES))
def test_the_plan_puts_each_case_on_its_instance(case):
    cfg, S, _seed, family, inst = case_config(case)
    for bf16 in (False, True) if case in BF16_CASES else (False,):
        lay = plan_layout(cfg, S, bf16)
        assert (lay.family, lay.instance) == (family, inst), (bf16, lay.family, lay.instance)
        assert cfg.Cx <= 768 and S * cfg.Nx <= 25000
        if family != "tile_gen":
            assert lay.zsz == 4 and lay.dgp == 8 and lay.Kp == 8           # the any-shape layout: Z in fp32 whatever the site's type
            continue
        got = rounds(lay, cfg.E)
        for k, want in ROUNDS[case].items():
            assert (got[k][0], got[k][2], got[k][3], got[k][5]) == want, (case, k, got[k])
    if case == "g2c6_k87":
        assert got["pre_small"][4] == 120192 and got["pre_lat_bwd"][4] == 115600      # > 64 KB of dynamic LDS
    if case == "merged_k2":
        assert lay.merged and (lay.dg, lay.dgp, lay.K, lay.Kp) == (12, 16, 2, 16)
    if case == "pad40_k87":
        assert (lay.dg, lay.dgp) == (40, 48)
    if case == "short_36":
        assert lay.per < 64
    if case == "tiny_3":
        assert cfg.Nx < 16
    if case == "many_blocks":
        assert lay.blocks >= 384
    if case == "g2c3_k20_v2":
        assert lay.El == cfg.E and (lay.K, lay.Kp) == (20, 32)


# ---- 2. the seeds -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(CASES))
def test_the_seed_keeps_the_oracles_z_clear_of_the_relu_kink(case):
    from oracle import avmoe_oracle as O
    from oracle.algebra_ref import AlgebraRef
    cfg, S, seed, _f, _i = case_config(case)
    P, B = O.init_params(cfg, seed=seed)
    g = torch.Generator().manual_seed(seed + 100)
    X = 0.3 * torch.randn(S, cfg.Nx, cfg.Cx, generator=g)
    Y = 0.3 * torch.randn(S, cfg.Ny, cfg.Cy, generator=g)
    A = AlgebraRef(cfg, P, B)
    A.forward(X, Y, training=True)
    worst = float("inf")
    for ex, e in zip(A.experts, A.sv["E"]):
        if ex.relu:
            sc = e["g1"] * e["r1"]
            sh = P[f"{ex.pre}.bn1.bias"].reshape(sc.shape) - e["z"].mean((0, 1)) * sc
            y, ymag = e["z"] * sc + sh, (e["z"] * sc).abs() + sh.abs()
            worst = min(worst, float((y.abs() / (R.KINK * ymag)).min()))
    print(f"{case}: nearest ReLU pre-activation at {worst:.1f} kink windows")
    # many_blocks: 9.4 M pre-activations; about 40 of them fall within 16 windows at any seed (the best of 880 seeds: 6.7)
    assert worst > (4.0 if case == "many_blocks" else 16.0)


# ---- 3. the tuned shape: bit-identical -----------------------------------------------------------------------------------------------------------
def _flat(v, out, key):
    if isinstance(v, dict):
        for k, x in v.items():
            _flat(x, out, f"{key}.{k}")
    elif isinstance(v, (tuple, list)):
        for i, x in enumerate(v):
            _flat(x, out, f"{key}[{i}]")
    else:
        out[key] = v


def _same(name, fn):
    a, b = {}, {}
    _flat(fn(R), a, name)
    _flat(fn(R0), b, name)
    assert a.keys() == b.keys() and a
    for k in a:
        assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), f"{k} differs from the tuned-shape module"
    return len(a)


def test_tuned_shape_refs_and_bounds_are_bit_identical():
    o = C0._operands()
    fwd = C0.emu_post_small(o, True, True, seed=10)
    bwd = C0.emu_post_mid_bwd(o, fwd["rp"], fwd["mup"], True, True, seed=20)
    n = 0
    for planes in (False, True):
        for ob in (False, True):
            n += _same("post_small", lambda M: M.post_small_ref(o["Z"], o["bn1"], o["Gq"], o["us"], o["vh"], o["H1p"], o["H2p"], o["qv"], C0.RELU, C0.C, C0.EPS, planes=planes, out_bf16=ob))
            n += _same("post_mid_bwd", lambda M: M.post_mid_bwd_ref(o["dAp"], o["dApx"], o["Z"], o["bn1"], o["Gq"], o["us"], o["vh"], o["qv"], fwd["rp"], fwd["mup"], o["dm"],
                                                                    o["sdSzz"], C0.RELU, C0.C, planes=planes, out_bf16=ob))
    p, a, TW, dzr, dSx, dSxx = C0._lat_operands()
    TTt, Tst = C0._per_token(p["TT"]), C0._per_token(p["Tsum"])
    zero, zz = torch.zeros(C0.NT, C0.EL, dtype=torch.float64), torch.zeros(C0.NT, C0.G, C0.EL, C0.D, dtype=torch.float64)
    for ob in (False, True):
        n += _same("scalar_cols", lambda M: M.scalar_cols_ref(o["qv"], fwd["rp"], fwd["mup"], out_bf16=ob))
        n += _same("pre_small_bwd", lambda M: M.pre_small_bwd_ref(bwd["dzp"], o["Z"], o["bn1"], o["mdy"], o["mdyz"], o["rr"], o["mu"], o["wsum"], o["dconst"], C0.C, out_bf16=ob))
        n += _same("softmax", lambda M: M.softmax_ref(p["L2"], out_bf16=ob))
        n += _same("z_map", lambda M: M.z_map_ref(o["Z"].double(), 1e-6 * o["Z"].double().abs(), 0.1 * o["dAp"].double(), 1e-7 * o["dAp"].double().abs(), o["rr"], o["mu"],
                                                   o["wsum"], o["dconst"], out_bf16=ob))
        n += _same("dgq_engine", lambda M: M.dgq_engine_ref(o["Z"], o["bn1"], C0.RELU, o["Z"], fwd["rp"], 1e-6 * fwd["rp"].double().abs(), out_bf16=ob, prod_eps=2.0 ** -27))
        for planes in (False, True):
            n += _same("pre_lat_bwd", lambda M: M.pre_lat_bwd_ref(a, p["L2"], p["TT"], TW, Tst, p["gv"][:C0.EL], dzr, zz, dSx.double(), zero, dSxx.double(), zero, C0.C,
                                                                  planes=planes, out_bf16=ob))
    for planes in (False, True):
        n += _same("rmu per token", lambda M: M.rmu_ref(p["sx"], p["L2"], a, TTt, Tst, p["gv"], C0.C, C0.EPS, planes=planes))
        n += _same("rmu per frame", lambda M: M.rmu_ref(p["sx"], p["L2"], a, p["TT"], Tst, p["gv"], C0.C, C0.EPS, planes=planes))
    w, b = 1.0 + 0.1 * o["us"], 0.1 * o["vh"]
    n += _same("bn1", lambda M: M.bn1_ref(o["Z"], w, b, 1e-5))
    n += _same("dsm34", lambda M: M.dsm34_ref(bwd["dzp"], o["Z"], o["bn1"]))
    n += _same("gram", lambda M: M.gram_ref(o["Z"], o["bn1"], C0.RELU))
    n += _same("dgq", lambda M: M.dgq_ref(o["Z"], o["bn1"], C0.RELU, fwd["rp"], None, mirrored=True))
    n += _same("zprime", lambda M: M.zprime(o["Z"], o["bn1"], C0.RELU))
    for k in ("U32", "EPS_RSQRT", "KINK", "KINK_CAP", "EPS_EXP", "TINY", "EPS_ACC", "EPS_BF16", "EPS_PLANES"):
        assert getattr(R, k) == getattr(R0, k)
    assert R._nsum(2, 32) == 2 * R0.FDG and n > 100


# ---- 4. the GPU module's checks on the emulation ------------------------------------------------------------------------------------------------
class EmuRecorder(G.GenRecorder):
    """keeps its margins to itself: the GPU module's coverage test counts GPU runs only"""

    def __init__(self, case, dtype):
        super().__init__(case, dtype, "emulation")
        self.ratio = {}

    def product(self, tag, kernel, fn):
        try:
            self.ratio[tag] = fn()
        except AssertionError as e:
            self.fail.append(f"{tag} [{kernel}]: {e}")

    def aside(self, tag, kernel, why):
        self.ratio[tag] = None


_SITES = {}


def site(case, dtype, order=0):
    """an honest emulated site (cached: the faults below work on copies)"""
    key = (case, dtype, order)
    if key not in _SITES:
        cfg, S, seed, _f, _i = case_config(case)
        bf16 = dtype == "bf16"
        _SITES[key] = EmuSite(cfg, S, seed, bf16, plan_layout(cfg, S, bf16), order=order)
    return _SITES[key]


def check(s, case, dtype):
    rec = EmuRecorder(case, dtype)
    G._forward(s, FWD, rec)
    G._backward(s, BWD, rec)
    return rec


def faulty(s):
    t = copy.copy(s)
    t.b = {k: v.clone() for k, v in s.b.items()}
    return t


def failed(rec, tag, text=None):
    hit = [f for f in rec.fail if f.startswith(tag + " ") and (text is None or text in f)]
    assert hit, f"expected {tag} ({text}) to fail; failures: {rec.fail}"
    return hit[0]


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("case", EMU_CASES)
def test_honest_emulation_stays_inside_every_bound_in_two_orders(case, dtype):
    for order in (0, 1000):
        rec = check(site(case, dtype, order), case, dtype)
        print(case, dtype, order, sorted((k, None if v is None else round(v, 4)) for k, v in rec.ratio.items()))
        rec.finish()
        assert set(rec.ratio) == set(G.TAGS) and max(v for v in rec.ratio.values() if v is not None) <= 1.0


def _put_pre(t, e, av, rr, mu, z):
    if av is not None:
        t.dev("a", t.T, (t.El, t.NT, t.Kp))[t.lat.index(e)] = av.to(t.T)
    r = t.f32("rmu", (2, t.E, t.NT))
    r[0, e], r[1, e] = rr, mu
    t.z("Z")[:, :, e] = z.to(t.ZT)


def _put_post(t, e, rp, mup, main, scal, rows=slice(None)):
    r = t.f32("rpmup", (2, t.E, t.NT))
    r[0, e, rows], r[1, e, rows] = rp[rows], mup[rows]
    Ap = t.dev("Apost", t.T, (t.NT, t.g, t.KPp))
    Ap[rows, :, e * t.dgp:(e + 1) * t.dgp] = t.st(main)[rows].to(t.T)
    Ap[rows, :, t.E * t.dgp + 3 * e:t.E * t.dgp + 3 * e + 3] = t.st(scal)[rows].to(t.T)


def test_a_padded_latent_slot_left_in_the_softmax_fails():
    case, dtype = "g2c1_k8_e5", "f32"                                       # K = 8 of 16 slots
    t = faulty(site(case, dtype))
    L2 = t.f32("L2", (t.NT, t.El, t.Kp))
    L2[:, :, t.K:] = L2[:, :, :t.K].mean(-1, keepdim=True)                 # whatever the padding of the logits buffer holds: here a plausible logit
    assert not check(t, case, dtype).fail                                  # ... which an honest kernel never looks at
    _put_pre(t, 0, *t.pre_small_expert(0, 0, slots=t.K + 1))
    rec = check(t, case, dtype)
    failed(rec, "P1", "slots K..Kp")


def test_TT_read_with_the_padded_stride_fails():
    case, dtype = "g4c2_k87_e8", "f32"                                      # K = 87 in 96 slots: TT is (S, El, 87, 87)
    t = faulty(site(case, dtype))
    _av, rr, mu, z = t.pre_small_expert(1, 0, tt_stride=t.Kp)
    _put_pre(t, 1, None, rr, mu, z)
    assert "rmu" in failed(check(t, case, dtype), "P1")


def test_a_second_round_expert_on_the_first_rounds_staged_constants_fails():
    case, dtype = "g4c2_k87_e8", "bf16"                                     # post_small: R = 2, expert 2 opens the second round
    t = faulty(site(case, dtype))
    _put_post(t, 2, *t.post_small_expert(2, 0, cst=0))
    msg = failed(check(t, case, dtype), "P4")
    assert "rp" in msg or "Apost" in msg


def test_an_idle_waves_write_to_the_last_experts_row_fails():
    """a round of two over five experts: the idle wave of the last round is clamped to expert E - 1; were its tile loop not cut short
    (tile_gen.inc:306 `act ? n_end : n_beg`) it would write that expert's rows from its own stale LDS slot, expert 3's constants"""
    case, dtype = "g2c1_k8_e5", "bf16"
    t = faulty(site(case, dtype))
    e = t.E - 1
    _put_post(t, e, *t.post_small_expert(e, 0, cst=e - 1), rows=slice(0, 16))
    msg = failed(check(t, case, dtype), "P4")
    tok = int(msg.split("= (")[1].split(",")[0])
    assert tok < 16, msg


def test_two_of_four_groups_exchanged_fails():
    case, dtype = "g4c2_k87_e8", "bf16"
    t = faulty(site(case, dtype))
    Ap = t.dev("Apost", t.T, (t.NT, t.g, t.KPp))
    lo, hi = 3 * t.dgp, 4 * t.dgp
    Ap[:, 1, lo:hi], Ap[:, 2, lo:hi] = Ap[:, 2, lo:hi].clone(), Ap[:, 1, lo:hi].clone()
    assert "Apost main columns" in failed(check(t, case, dtype), "P4")
    t = faulty(site(case, dtype))
    Z = t.z("Z")
    Z[:, 0, 5], Z[:, 3, 5] = Z[:, 3, 5].clone(), Z[:, 0, 5].clone()
    failed(check(t, case, dtype), "P1z")


def test_the_odd_last_chunk_from_the_neighbouring_experts_segment_fails():
    case, dtype = "g2c1_k8_e5", "f32"                                       # NCG = 1: the one chunk of a group IS the odd chunk (ld_one)
    t = faulty(site(case, dtype))
    _put_post(t, 1, *t.post_small_expert(1, 0, odd_from=2))
    failed(check(t, case, dtype), "P4")


@pytest.mark.parametrize("buf,tag", [("Z", "P1z"), ("Zp", "P3"), ("Apost", "P4"), ("dzp", "P6"), ("Zw", "P9"), ("bn1", "P2"), ("a", "P1"), ("dL2x", "P10")])
def test_a_non_zero_padding_entry_fails(buf, tag):
    case, dtype = "merged_k2", "bf16"                                       # 12 entries padded to 16, 2 latent tokens in 16 slots
    t = faulty(site(case, dtype))
    tiny = 2.0 ** -20
    if buf in ("Z", "dzp"):
        t.z(buf)[7, 0, 1, 13] = tiny
    elif buf in ("Zp", "Zw"):
        t.zT(buf)[7, 0, 2, 15] = tiny
    elif buf == "Apost":
        t.dev("Apost", t.T, (t.NT, t.g, t.KPp))[7, 0, 1 * t.dgp + 12] = tiny
    elif buf == "bn1":
        t.f32("bn1", (4, t.g, t.E, t.dgp))[2, 0, 1, 14] = tiny
    elif buf == "a":
        t.dev("a", t.T, (t.El, t.NT, t.Kp))[0, 7, 2] = tiny
    else:
        t.dev("dL2x", t.T, (t.NT, t.KLp))[7, 5] = tiny
    assert "padding" in failed(check(t, case, dtype), tag) or buf in ("a", "dL2x")


def test_one_tiles_matvec_off_by_one_percent_fails():
    """what csrc/tile_lane.h:99 records of the fp32 matrix pipe: one 16-token tile in a thousand, off by about 1 %"""
    for case, dtype in (("kt_three_groups_50", "f32"), ("g4c2_k87_e8", "f32")):
        t = faulty(site(case, dtype))
        ws = torch.ones(t.NT)
        ws[16:32] = 1.01
        _put_post(t, 0, *t.post_small_expert(0, 0, w_scale=ws))
        msg = failed(check(t, case, dtype), "P4")
        assert 16 <= int(msg.split("= (")[1].split(",")[0]) < 32, msg


@pytest.mark.parametrize("buf,tag", [("Apost", "P4"), ("Zw", "P9"), ("dzp", "P6"), ("dL2x", "P10"), ("a", "P1")])
def test_one_bf16_ulp_in_a_bf16_output_fails(buf, tag):
    """one ulp AWAY from the fp64 value (towards it, a correctly rounded result that sat at the far end of its rounding interval may pass)"""
    case, dtype = "g4c2_k87_e8", "bf16"
    s = site(case, dtype)
    view = {"Apost": lambda x: x.dev("Apost", x.T, (x.NT, x.g, x.KPp))[:, :, :x.E * x.dgp], "Zw": lambda x: x.zT("Zw"), "dzp": lambda x: x.z("dzp"),
            "dL2x": lambda x: x.dev("dL2x", x.T, (x.NT, x.KLp))[:, :x.KL], "a": lambda x: x.dev("a", x.T, (x.El, x.NT, x.Kp))}[buf]
    idx = tuple(int(i) for i in (view(s).float().abs() > 0.05 * float(view(s).float().abs().max())).nonzero()[3])
    hits = 0
    for step in (1, -1):
        t = faulty(s)
        v = view(t)
        bits = v.view(torch.int16)
        bits[idx] += step
        rec = check(t, case, dtype)
        hits += any(f.startswith(tag + " ") for f in rec.fail)
    assert hits >= 1, "neither direction failed"
