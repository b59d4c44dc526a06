"""tests/mha_ref.py on the CPU: an emulation of the frame-attention ("v1") expert chain and of the x + xr glue -- the kernels' roundings, fp32
sums in two orders, the plane splits of the fp32 glue products -- stays inside every bound at every case and input family of
tests/test_mha_chain_fp64_gpu.py, and each of the mistakes such a chain makes fails the link it belongs to and no other.  These are the
conditions that make the GPU module mean something: if a bound fails the honest emulation, the bound is wrong.

Emulation: operands in the buffers' own dtypes; products as fp32 matmuls (order 0) or as fp32 partial sums over chunks of 16 of the contraction
added in reverse (order 1); row and column sums as torch's fp32 sum (order 0) or folded from the last lane / chunk (order 1); every store a
round-to-nearest-even cast.  What lies upstream of the chain (Wt, and in the backward dZR, dsr, dZx, dL2x, Text, rs2x) is drawn.

Measured on the fp64 scores of the drawn sites (test_families_hold_on_the_fp64_scores asserts the conditions and prints these):
  S13_C96   flat: max span 0.015    peaked: 0.978 of the rows span > 8 (max 21.7); row maxima 0.333 column 0 / 0.333 column S - 1 / 0.667 last 8-group
  S70_C128  flat: max span 0.021    peaked: 1.000 of the rows span > 8 (max 28.2); row maxima 0.333 column 0 / 0.320 column S - 1 / 0.589 last 8-group
  (the default draw: max span 0.23 / 0.33 -- flat already, which is why the peaked family is there)
"""
import pytest
import torch

from tests import mha_ref as M
from tests.test_hop1_checker import fmm, fsum

SITES, CASES, draw_site = M.SITES, M.CASES, M.draw_site


def dims_of(cfg, S, bf16, training=True):
    from avmoe_amd import _capi
    from avmoe_amd import _capi_moe as cm
    from tests.moe_gpu_util import make_desc
    return M.Dims(cfg, S, bf16, {n: b for (n, _r, _o, b) in cm.buffer_table(_capi.lib(), make_desc(cfg, S, bf16, training))})


def _planes(x, n):
    p0 = x.bfloat16().float()
    r1 = x - p0
    p1 = r1.bfloat16().float()
    return [p0, p1] if n == 2 else [p0, p1, (r1 - p1).bfloat16().float()]


def pmm(A, Bm, order, planes):
    """an fp32 product on the bf16 matrix pipe: the plane products of order < planes, smallest first (gemm.hip:237, :270)"""
    if not planes:
        return fmm(A, Bm, order)
    a, b = _planes(A.float(), planes), _planes(Bm.float(), planes)
    acc = None
    for o in reversed(range(planes)):
        for i in range(o + 1):
            p = fmm(a[i], b[o - i], order)
            acc = p if acc is None else acc + p
    return acc


def colsum(x, order, drop_last=False):
    """km_colsum_part + k_colsum_f32 (mha_frames.hip:64-83)"""
    rows = x.shape[0]
    chunks = max(1, min(256, rows // 64))
    rpc = -(-rows // chunks)
    parts = [fsum(x[c * rpc:(c + 1) * rpc].float(), 0, order) for c in range(chunks - int(drop_last))]
    return torch.stack(parts).double().sum(0).float() if order == 0 else fsum(torch.stack(parts), 0, 1)


def one_ulp(x):
    """every element one bf16 ulp further from zero"""
    return (x.bfloat16().view(torch.int16) + 1).view(torch.bfloat16).to(x.dtype)


def emulate(d, P, X, keep, order=0, fault=None, seed=3):
    """{buffer: tensor} behind one forward + backward (the backward's scratch: the last slot)"""
    S, N, C, Hh, dh, Sp, NT, g, Cg, E, dgp = d.S, d.N, d.C, d.H, d.dh, d.Sp, d.NT, d.g, d.Cg, d.E, d.dgp
    nan = float("nan")
    R = lambda x: x.float().to(d.T)
    f = lambda x: x.float()
    gen = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=gen)
    B = {k: v.float() for k, v in P.items()}
    X = B["X"] = R(X)
    B["keep"] = keep
    X2 = f(X).reshape(NT, C)
    fwd_planes = 0 if d.bf16 else 3
    Wt = B["Wt"] = R(0.2 * rn(g, E * dgp, Cg))
    n = d.nxr
    B["xr"], B["sxr"] = torch.zeros(n, S, N, C, dtype=d.T), torch.zeros(n, 3, NT)
    ZR = M.poison((NT, g, E, dgp), torch.float32)
    if d.v1:
        for k, sh in d.shapes().items():
            if k.startswith("m"):
                B[k] = M.poison(sh[1], torch.float32 if sh[0] == "f" else d.T)
    heads = lambda t: M._heads(d, t)
    unheads = lambda t: t.permute(2, 0, 1, 3).reshape(S, N, C)
    for j, e, pre in d.slots:
        if not d.v1:                                               # AVVP: the N x N block's xr is an operand here
            B["xr"][0] = R(0.3 * rn(S, N, C))
        else:
            par = lambda k: B[f"{pre}.self_attention.{k}"]
            Win, Wout = R(par("in_proj_weight")), R(par("out_proj.weight"))
            B["mWin"][j], B["mWout"][j] = Win, Wout
            Wuse = f(Win)
            if fault == "qkv_exchanged":
                Wuse = torch.cat([Wuse[C:2 * C], Wuse[2 * C:], Wuse[:C]])
            col = torch.arange(3 * C)
            bias = par("in_proj_bias")[col % C if fault == "bias_mod_C" else col]
            QKV = R(f(R(fmm(X2, Wuse.t(), order))) + bias)
            if fault == "ulp_mQKV":
                QKV = one_ulp(QKV)
            B["mQKV"][j] = QKV.reshape(S, N, 3 * C)
            q, k, v = (f(t) for t in M.qkv(d, B["mQKV"][j]))
            qs, ks = q, k
            if fault == "head_plus_1":
                qs = q.roll(-1, 1)
            if fault == "token_plus_1":
                ks = k.roll(-1, 0)
            alpha = {"alpha_missing": 1.0, "alpha_1_over_dh": 1.0 / dh}.get(fault, d.alpha)
            sc = fmm(qs, ks.transpose(-1, -2), order) * torch.tensor(alpha, dtype=torch.float32)
            B["mSc"][..., :S] = sc
            if fault == "softmax_over_Sp":
                sc = torch.cat([sc, torch.zeros(N, Hh, S, Sp - S)], -1)
            mx = sc.max(-1, keepdim=True).values
            ex = torch.exp(sc - mx)
            inv = (1.0 / ex.double().sum(-1, keepdim=True)).float()
            if fault == "neighbour_row_sum":
                inv = inv.roll(1, 2)
            Pm = torch.zeros(N, Hh, S, Sp, dtype=d.T)
            Pm[..., :S] = R(ex * inv)[..., :S]
            if fault == "slot1_reads_slot0_mP" and j == 1:
                Psrc, B["mP"][j] = B["mP"][0], Pm
            else:
                Psrc = B["mP"][j] = Pm
            kp = M.keep_of(d, B, pre)
            if kp is not None:
                kk = kp.float()
                if fault == "keep_stride_Sp":
                    flat = kk.reshape(-1)
                    idx = (torch.arange(N * Hh * S)[:, None] * Sp + torch.arange(S)[None]) % flat.numel()
                    kk = flat[idx].reshape(N, Hh, S, S)
                Pd = torch.zeros(N, Hh, S, Sp, dtype=d.T)
                Pd[..., :S] = R(f(Psrc[..., :S]) * kk)
                if fault == "nan_in_column_S":
                    Pd[..., S] = nan
                B["mPd"][j] = Pd
            else:
                Pd = Psrc
            if fault == "nan_in_column_S":                         # the product reads one 8-group: K = Sp against zero rows of v
                o = fmm(f(Pd), torch.cat([v, torch.zeros(N, Hh, Sp - S, dh)], 2), order)
            else:
                o = fmm(f(Pd[..., :S]), v, order)
            if fault == "heads_reversed":
                o = o.flip(1)
            Om = R(unheads(o))
            if fault == "ulp_mO":
                Om = one_ulp(Om)
            B["mO"][j] = Om
            t = f(R(fmm(f(Om).reshape(NT, C), f(Wout).t(), order)))
            if fault != "bout_missing":
                t = t + par("out_proj.bias")
            if fault != "minus_X_missing":
                t = t - X2
            xr = R(t)
            if fault == "ulp_xr":
                xr = one_ulp(xr)
            B["xr"][j] = xr.reshape(S, N, C)
        xr2 = f(B["xr"][j]).reshape(NT, C)
        xa = xr2 if fault == "x_dot_xr_as_xr_xr" else X2
        B["sxr"][j] = torch.stack([fsum(xr2, -1, order), fsum(xr2 * xr2, -1, order), fsum(xa * xr2, -1, order)])
        xg = xr2.reshape(NT, g, Cg).permute(1, 0, 2)
        if d.v1:
            eu = (e + 1) % E if fault == "zr_other_expert" else e
            ZR[:, :, e] = pmm(xg, f(Wt[:, eu * dgp:(eu + 1) * dgp]).transpose(1, 2), order, fwd_planes).permute(1, 0, 2)
        else:
            ZR = pmm(xg, f(Wt).transpose(1, 2), order, fwd_planes).permute(1, 0, 2).reshape(NT, g, E, dgp)
    B["ZR"] = ZR.reshape(S, N, g, E, dgp)
    if d.v1:
        B["scores"] = B["mSc"].clone()                             # (read behind the forward: the backward overwrites mSc)
    if keep is None and d.v1:
        return B                                                   # eval: forward only
    # ---- backward: the last slot ----
    j, e, pre = d.slots[-1]
    dZR = B["dZR"] = R(0.1 * rn(S, N, g, E, dgp))
    dsr = B["dsr"] = 0.05 * rn(n, 3, NT)
    B["Zw"], B["dL2x"] = R(0.1 * rn(S, N, g, E * dgp)), R(0.1 * rn(S, N, d.KLp))
    B["Text"], B["rs2x"] = R(0.3 * rn(S, d.KLT, C)), 0.05 * rn(S, N)
    xr2 = f(B["xr"][j]).reshape(NT, C)
    grp = lambda t: t.reshape(NT, g, Cg).permute(1, 0, 2)
    ungrp = lambda t: t.permute(1, 0, 2).reshape(NT, C)
    dz = f(dZR).reshape(NT, g, E, dgp).permute(1, 0, 2, 3)
    bwd_planes = 0 if d.bf16 else 3
    if d.v1:
        p = pmm(dz[:, :, e], f(Wt[:, e * dgp:(e + 1) * dgp]), order, bwd_planes)
    else:
        p = pmm(dz.reshape(g, NT, E * dgp), f(Wt), order, bwd_planes)
    d0, d1, d2 = dsr[j][0][:, None], dsr[j][1][:, None], dsr[j][2][:, None]
    dxr0 = f(R(ungrp(p) + d1 * xr2))
    dxr = dxr0 + (d1 if fault == "axpy_dsr2_from_plane_1" else d2) * X2
    if fault != "axpy_without_dsr0":
        dxr = dxr + d0
    dxr = R(dxr)
    B["dxr"] = dxr.reshape(S, N, C)
    if not d.v1:
        return B
    dx2 = f(dxr)
    # dX: the site's product, the axpy, the attention's input gradient
    A = torch.cat([f(B["Zw"]).permute(0, 2, 1, 3), f(B["dL2x"])[:, None, :, :d.KLT].expand(S, g, N, d.KLT)], 3)
    Bm = torch.cat([f(Wt)[None].expand(S, g, E * dgp, Cg), f(B["Text"]).reshape(S, d.KLT, g, Cg).permute(0, 2, 1, 3)], 2)
    sg = lambda t: t.reshape(S, N, g, Cg).permute(0, 2, 1, 3)
    unsg = lambda t: t.permute(0, 2, 1, 3).reshape(NT, C)
    dX = f(R(unsg(pmm(A, Bm, order, 0 if d.bf16 else 2) + B["rs2x"][:, None, :, None] * sg(f(X)))))
    dX = dX + d2 * xr2
    if fault != "axpy_without_minus_dxr":
        dX = dX - dx2
    dX = f(R(dX))
    G = {}
    sa = lambda k: f"{pre}.self_attention.{k}"
    G[sa("out_proj.bias")] = colsum(dx2, order, fault == "dbout_last_chunk_dropped")
    Om, Wout, Win = f(B["mO"][j]).reshape(NT, C), f(B["mWout"][j]), f(B["mWin"][j])
    dWout = fmm(dx2.t(), Om, order)
    G[sa("out_proj.weight")] = dWout.t().contiguous() if fault == "dWout_transposed" else dWout
    dO = R(fmm(dx2, Wout, order))
    B["mdO"] = dO.reshape(S, N, C)
    q, k, v = (f(t) for t in M.qkv(d, B["mQKV"][j]))
    dOh = heads(f(B["mdO"]))
    kp = M.keep_of(d, B, pre).float()
    Pm, Pd = f(B["mP"][j][..., :S]), f(B["mPd"][j][..., :S])
    dP = fmm(dOh, v.transpose(-1, -2), order)
    if fault != "keep_not_applied":
        dP = dP * kp
    B["mSc"][..., :S] = dP
    dv = R(fmm((Pm if fault == "dv_from_P" else Pd).transpose(-1, -2), dOh, order))
    dot = 0.0 if fault == "dS_without_row_dot" else fsum(Pm * dP, -1, order)[..., None]
    dS = torch.zeros(N, Hh, S, Sp, dtype=d.T)
    dS[..., :S] = R(Pm * (dP - dot))
    B["mdS"] = dS
    dSf = f(dS[..., :S])
    al = torch.tensor(d.alpha, dtype=torch.float32)
    dq = R(fmm(dSf, k, order) * (1.0 if fault == "dq_without_alpha" else al))
    dk = R(fmm(dSf if fault == "dk_from_untransposed_dS" else dSf.transpose(-1, -2), q, order) * al)
    dQKV = torch.cat([unheads(f(t)) for t in (dq, dk, dv)], -1).to(d.T)
    if fault == "ulp_mdQKV":
        dQKV = one_ulp(dQKV)
    B["mdQKV"] = dQKV
    dQ2 = f(dQKV).reshape(NT, 3 * C)
    dbin = colsum(dQ2, order)
    if fault == "dbin_first_C_only":
        dbin[C:] = nan                                             # (the caller's NaN prefill)
    G[sa("in_proj_bias")] = dbin
    G[sa("in_proj_weight")] = fmm(dQ2.t(), X2, order)
    Wx = torch.cat([Win[i * C:(i + 1) * C].t() for i in range(3)]) if fault == "dX_through_Win_T" else Win
    B["dX"] = R(dX + fmm(dQ2, Wx, order)).reshape(S, N, C)
    B["grads"] = G
    return B


def run_links(d, B, training=True):
    """{tag (+ slot): worst err / bound, or the AssertionError}: every link the GPU module runs at such a site"""
    out = {}

    def run(tag, fn):
        try:
            out[tag] = fn()
        except AssertionError as ex:
            out[tag] = ex

    last = d.slots[-1][0]
    if not d.v1:
        for tag in M.GLUE:
            run(tag, lambda tag=tag: {**M.FORWARD, **M.BACKWARD}[tag][2](d, B, 0))
        return out
    for j, _e, _pre in d.slots:
        for tag, (_w, _k, fn) in M.FORWARD.items():
            kw = {"stored_scores": j == last} if tag == "softmax" else {}
            run(f"{tag}[{j}]", lambda fn=fn, j=j, kw=kw: fn(d, B, j, **kw))
    run("scores", lambda: M.link_scores(d, B, last))
    run("zr_others", lambda: M.link_zr_others(d, B))
    if training:
        for tag, (_w, _k, fn) in M.BACKWARD.items():
            if tag == "dx" and len(d.slots) > 1:
                continue
            run(tag, lambda fn=fn: fn(d, B, last))
    return out


_SITES = {}


def _site(site, family, dtype):
    key = (site, family, dtype)
    if key not in _SITES:
        _SITES.clear()
        cfg, S, training, P, _Bf, X, _Y, _G, keep = draw_site(site, family)
        _SITES[key] = (dims_of(cfg, S, dtype == "bf16", training), P, X, keep, training)
    return _SITES[key]


@pytest.mark.parametrize("site,family,dtype", CASES)
def test_honest_emulation_stays_inside_every_bound(site, family, dtype):
    d, P, X, keep, training = _site(site, family, dtype)
    for order in (0, 1):
        B = emulate(d, P, X, keep, order)
        res = run_links(d, B, training)
        bad = {k: str(v) for k, v in res.items() if isinstance(v, AssertionError)}
        assert not bad, bad
        assert max(res.values()) <= 1.0, res
        if d.v1:
            M.check_family(d, B["scores"], family)


# fault -> (links that must fail: at least one of them, and nothing outside them; (site, family) it is planted at)
FAULTS = {
    "bias_mod_C": ({"qkv[0]"}, ("S13_C96", "default")),
    "qkv_exchanged": ({"qkv[0]"}, ("S13_C96", "default")),
    "head_plus_1": ({"scores"}, ("S13_C96", "default")),
    "token_plus_1": ({"scores"}, ("S13_C96", "default")),
    "alpha_missing": ({"scores"}, ("S13_C96", "default")),
    "alpha_1_over_dh": ({"scores"}, ("S13_C96", "default")),
    "softmax_over_Sp": ({"softmax[0]"}, ("S13_C96", "default")),
    "neighbour_row_sum": ({"softmax[0]"}, ("S13_C96", "peaked")),
    "keep_stride_Sp": ({"keep[0]"}, ("S13_C96", "default")),
    "heads_reversed": ({"o[0]"}, ("S13_C96", "default")),
    "bout_missing": ({"xr[0]"}, ("S13_C96", "default")),
    "minus_X_missing": ({"xr[0]"}, ("S13_C96", "default")),
    "x_dot_xr_as_xr_xr": ({"sxr[0]"}, ("S13_C96", "default")),
    "zr_other_expert": ({"zr[0]", "zr[1]"}, ("S13_two_slots", "default")),
    "slot1_reads_slot0_mP": ({"keep[1]"}, ("S13_two_slots", "default")),
    "keep_not_applied": ({"dpd"}, ("S13_C96", "default")),
    "dv_from_P": ({"dv"}, ("S13_C96", "default")),
    "dS_without_row_dot": ({"ds"}, ("S13_C96", "peaked")),
    "dq_without_alpha": ({"dq"}, ("S13_C96", "default")),
    "dk_from_untransposed_dS": ({"dk"}, ("S13_C96", "peaked")),
    "dbin_first_C_only": ({"dbin"}, ("S13_C96", "default")),
    "dbout_last_chunk_dropped": ({"dbout"}, ("S13_C96", "default")),
    "dWout_transposed": ({"dwout"}, ("S13_C96", "default")),
    "dX_through_Win_T": ({"dx"}, ("S13_C96", "default")),
    "axpy_without_minus_dxr": ({"dx"}, ("S13_C96", "default")),
    "axpy_without_dsr0": ({"dxr"}, ("S13_C96", "default")),
    "axpy_dsr2_from_plane_1": ({"dxr"}, ("S13_C96", "default")),
    "ulp_mQKV": ({"qkv[0]"}, ("S13_C96", "default")),
    "ulp_mO": ({"o[0]"}, ("S13_C96", "default")),
    "ulp_xr": ({"xr[0]"}, ("S13_C96", "default")),
    "ulp_mdQKV": ({"dq", "dk", "dv"}, ("S13_C96", "default")),
    "nan_in_column_S": ({"keep[0]", "o[0]"}, ("S13_C96", "default")),
}
@pytest.mark.parametrize("fault", list(FAULTS))
def test_planted_fault_fails_its_link(fault):
    want, (site, family) = FAULTS[fault]
    d, P, X, keep, training = _site(site, family, "bf16")
    res = run_links(d, emulate(d, P, X, keep, 0, fault), training)
    failed = {k for k, v in res.items() if isinstance(v, AssertionError)}
    if fault == "nan_in_column_S":
        # the padding check AND the product that read it; the NaN then travels on, and nothing in front of it fails
        assert want <= failed and not failed & {"cast[0]", "qkv[0]", "scores", "softmax[0]"}, failed
    else:
        assert failed and failed <= want, (failed, want, {k: str(res[k])[:200] for k in failed})
    # ... and every link passes without the fault, on the same inputs
    res = run_links(d, emulate(d, P, X, keep, 0), training)
    assert not [k for k, v in res.items() if isinstance(v, AssertionError)]


@pytest.mark.parametrize("site", ["S13_C96", "S70_C128"])
def test_families_hold_on_the_fp64_scores(site):
    """the scalings of mha_ref.apply_family, from fp64 alone: flat -> every score row spans < 0.5; peaked -> >= 90 % of the rows span > 8 and
    the row maxima sit in column 0, in column S - 1 and in the last 8-group"""
    for family in ("flat", "peaked"):
        cfg, S, _tr, P, _Bf, X, _Y, _G, _keep = draw_site(site, family)
        d = dims_of(cfg, S, True)
        pre = d.slots[-1][2]
        Xb = X.bfloat16().double().reshape(d.NT, d.C)
        W = P[f"{pre}.self_attention.in_proj_weight"].bfloat16().double()
        qkv = (Xb @ W.t() + P[f"{pre}.self_attention.in_proj_bias"].double()).reshape(S, cfg.Nx, 3 * d.C)
        q, k, _ = M.qkv(d, qkv)
        got = M.check_family(d, d.alpha * (q @ k.transpose(-1, -2)), family)
        print(f"FAMILY {site} {family} " + ", ".join(f"{a} {b:.3f}" for a, b in got.items()))


def test_a_family_without_its_property_fails():
    cfg, S, _tr, P, _Bf, X, _Y, _G, keep = draw_site("S13_C96", "default")
    d = dims_of(cfg, S, True)
    Sc = emulate(d, P, X, keep, 0)["scores"]
    with pytest.raises(AssertionError):
        M.check_family(d, Sc, "peaked")
    cfg, S, _tr, P, _Bf, X, _Y, _G, keep = draw_site("S13_C96", "peaked")
    with pytest.raises(AssertionError):
        M.check_family(d, emulate(d, P, X, keep, 0)["scores"], "flat")


def test_colsum_bound_is_the_path_not_the_row_count():
    """COLSUM: at NT = 200 (three chunks of 67 rows) the bound is 21 roundings, a ninth of NT * EPS_ACC"""
    assert M.colsum_bound(200, 1.0) == (17 + 2 + 1 + 1) * M.EPS_ACC
    assert M.colsum_bound(200, 1.0) < 200 * M.EPS_ACC / 9
