"""tests/hop1_ref.py on the CPU: an emulation of every link of the hop-1 chain with the kernels' roundings and fp32 sums in two orders stays
inside the bounds at every shape and input family of tests/test_hop1_chain_fp64_gpu.py, and each of the mistakes such a chain makes -- a
softmax over the padded extent, a maximum from the wrong lanes, a neighbouring row's 1 / sum or dot, a padding row that is not zeroed, two
extension columns exchanged, a column off by one, a missing term of the glue, a transposed store left out, a product left out of an
accumulated sum, a gradient row too many, one bf16 ulp in an fp32 result -- fails the link it belongs to.  These are the conditions that make
the GPU module mean something.  The parent code meets the first condition by construction: if a bound fails the emulation, the bound is wrong.

Emulation: operands in the buffers' own dtypes; products as fp32 matmuls (order 0) or as fp32 partial sums over chunks of 16 of the contraction
added in reverse (order 1); wave sums as torch's fp32 sum (order 0) or 64 lane sums folded from the last lane (order 1); the softmax as the
three kernel texts sum it (double / float); every store as a round-to-nearest-even cast.  What lies upstream of the chain in the backward
(dT, dtbar, drin, dZx, a, gate a, du3 a) is drawn."""
import pytest
import torch

from oracle import avmoe_oracle as O
from tests import hop1_ref as H

# the GPU module's shapes (frames, N, M, E_m, E_s) + a site with K = 20 in 32-row slots (padding rows k >= K) at the narrow width of the
# generalised passes
SHAPES = {
    "pad_77_71": (32, 77, 71, 2, 2), "one_cross_66": (33, 196, 66, 1, 3), "long_k_y": (33, 200, 300, 2, 2), "long_k_x": (32, 300, 100, 2, 2),
    "short_20": (34, 20, 65, 2, 2), "rows_1100": (2, 1100, 64, 2, 2), "rows_4100": (2, 4100, 40, 2, 2),
}
FAMILY_SHAPES = ("pad_77_71", "one_cross_66", "rows_1100")
CASES = [(s, "default") for s in SHAPES] + [(s, f) for s in FAMILY_SHAPES for f in ("flat", "peaked")] + [("k20", f) for f in H.FAMILIES] + [("pad_77_71_f32", "default"), ("k20_f32", "peaked")] + [("v2_k20", f) for f in H.FAMILIES] + [("v2_k20_f32", "default")]


def _cfg(shape):
    if shape == "v2_k20":
        from tests.gen_pass_cases import case_config
        cfg, S, _seed, _fam, _inst = case_config("g2c3_k20_v2")
        return cfg, S
    if shape == "k20":
        return O.AdapterConfig(Cx=192, Nx=77, Cy=64, Ny=23, reduction=2, groups=2, K=20, E_m=2, E_s=2, variant="ave"), 4
    S, N, M, E_m, E_s = SHAPES[shape]
    return O.AdapterConfig(Cx=768, Nx=N, Cy=768, Ny=M, reduction=12, groups=2, K=32, E_m=E_m, E_s=E_s, variant="ave"), S


def _dims(cfg, S, bf16=True):
    from avmoe_amd import _capi
    from avmoe_amd import _capi_moe as cm
    from tests.moe_gpu_util import make_desc
    return H.Dims(cfg, S, bf16, {n: b for (n, _r, _o, b) in cm.buffer_table(_capi.lib(), make_desc(cfg, S, bf16, True))})


def fsum(x, dim, order):
    x = x.float()
    if order == 0:
        return x.sum(dim)
    x = x.movedim(dim, -1)
    n = x.shape[-1]
    pad = -n % 64
    if pad:
        x = torch.cat([x, x.new_zeros(*x.shape[:-1], pad)], -1)
    lanes = x.reshape(*x.shape[:-1], -1, 64).sum(-2)
    acc = lanes[..., 63]
    for l in range(62, -1, -1):
        acc = acc + lanes[..., l]
    return acc


def fmm(A, Bm, order):
    A, Bm = A.float(), Bm.float()
    if order == 0:
        return A @ Bm
    K = A.shape[-1]
    acc = None
    for k0 in reversed(range(0, K, 16)):
        p = A[..., k0:k0 + 16] @ Bm[..., k0:k0 + 16, :]
        acc = p if acc is None else acc + p
    return acc


def emulate(d, P, Y, order=0, fault=None, seed=3):
    """{buffer: tensor} of one forward + backward of the chain.  fault: one of FAULTS -- the step it names goes wrong, everything behind it
    continues from what that step stored (as the real chain would)."""
    S, N, M, C, Cy, K, Kp, Kcy, Kcyb, Np, Mk, Mb, El = d.S, d.N, d.M, d.C, d.Cy, d.K, d.Kp, d.Kcy, d.Kcyb, d.Np, d.Mk, d.Mb, d.El
    f32, nan = torch.float32, float("nan")
    R = lambda x: x.float().to(d.T)
    g = torch.Generator().manual_seed(seed)
    B = {k: v.float() for k, v in P.items()}
    Y = R(Y)
    B["Y"] = Y
    X = B["X"] = R(B["X"])
    Kcx = d.Kcx
    Wc, bc, Wf, bf = H._params(d, B)
    # ---- k_prep_all ----
    WcK = torch.zeros(N, Mk); WcK[:, :M], WcK[:, M], WcK[:, M + 1] = Wc, bc, 1.0
    WcT = torch.zeros(M + 1, Np); WcT[:M, :N], WcT[M, :N] = Wc.t(), bc
    B["WcK"], B["WcT"], B["WfT"] = R(WcK), R(WcT), R(Wf)
    rw = fsum(B["WfT"], -1, order)
    wbar = torch.zeros(Mb); wbar[:M] = (fsum(Wc, 0, order).double() / N).float()
    scal = torch.zeros(64); scal[0] = fsum(bc, 0, order) / N; scal[1] = 1.0
    T0 = torch.zeros(El, Kp, C)
    for l, k in enumerate(d.tok_keys):
        T0[l, :K] = B[k]
    B["rw"], B["wbar"], B["scal"], B["T0T"] = rw, wbar, scal, R(T0.reshape(d.KL, C))
    Text = torch.zeros(S, d.KLT, C, dtype=d.T); Text[:, d.KL] = 1.0
    Tsum = torch.zeros(2, S, d.KLT); Tsum[:, :, d.KL] = float(C)
    # ---- Qx, k_qrqb_fill ----
    T0y = B["T0T"][:Kcy].float()
    B["Qx"] = R(fmm(T0y, B["WfT"], order))
    qrqb = torch.stack([fsum(T0y * rw, -1, order), fsum(T0y * bf, -1, order)])
    B["qrqb"] = qrqb
    Rext = torch.zeros(S, Kcyb, Mk, dtype=d.T)
    Rext[:, :Kcy, :M] = R(fmm(B["Qx"], Y.float().transpose(1, 2), order))
    a, b = (1, 0) if fault == "qr_qb_exchanged" else (0, 1)
    Rext[:, :Kcy, M], Rext[:, :Kcy, M + 1] = R(qrqb[a]), R(qrqb[b])
    B["Rext"] = Rext
    BmX = torch.zeros(S, Kcyb, Mb, dtype=d.T)
    if fault != "wbar_missing":
        BmX[:, Kcy] = R(wbar)
    # ---- L1, softmax ----
    L1 = torch.full((S, Kcyb, Np), nan)
    L1[:, :Kcy, :N] = fmm(Rext[:, :Kcy, :M + 2], B["WcK"][:, :M + 2].float().t(), order)
    if fault == "ulp_L1":
        L1[:, :Kcy, :N] = _one_ulp(L1[:, :Kcy, :N])
    B["L1"] = L1
    text = H.softmax_text(N, Np)
    real = H.real_rows(d)
    if fault == "kcy_row_not_zeroed":
        real = real.clone(); real[Kcy] = True
    if fault == "slot_row_not_zeroed":
        assert Kp > K
        real = real.clone(); real[K] = True
    p = torch.nan_to_num(L1[:, real], nan=0.0)                  # (a row that should have been skipped: whatever lies there, zeros here)
    n = Np if fault == "softmax_over_Np" else N
    p = p[..., :n]
    mx = (p[..., :64] if fault == "max_of_first_64" else p).max(-1, keepdim=True).values
    e = torch.exp(p - mx)
    inv = 1.0 / fsum(e, -1, order)[..., None] if text == "plain" else (1.0 / e.double().sum(-1, keepdim=True)).float()
    if fault == "inv_of_neighbour_row":
        inv = inv.roll(1, 1)
    A1 = torch.zeros(S, Kcyb, Np, dtype=d.T)
    A1[:, real, :n] = R(e * inv)
    B["A1y"] = A1
    # ---- [Bm | ab], V, TV, k_finish_T, TT, TW ----
    BmX[:, :Kcy, :M + 1] = R(fmm(A1[:, :Kcy, :N], B["WcT"][:, :N].float().t(), order))
    B["BmX"] = BmX
    B["V"] = R(fmm(BmX[:, :, :M], Y, order))
    TV = fmm(B["V"], B["WfT"].float().t(), order)
    if fault == "ulp_TV":
        TV = _one_ulp(TV)
    B["TV"] = TV
    tok = torch.stack([B[k] for k in d.tok_keys[:d.Ey]])[None]
    ab = BmX[:, :Kcy, M - 1 if fault == "ab_from_M_minus_1" else M].float().reshape(S, d.Ey, Kp)[:, :, :K, None]
    v = tok + TV[:, :Kcy].reshape(S, d.Ey, Kp, C)[:, :, :K]
    v = v + (ab * rw + bf)
    Ty = torch.zeros(S, d.Ey, Kp, C, dtype=d.T); Ty[:, :, :K] = R(v)
    Text[:, :Kcy] = Ty.reshape(S, Kcy, C)
    st = Text[:, :Kcy].double()
    Tsum[0, :, :Kcy], Tsum[1, :, :Kcy] = st.sum(-1).float(), (st * st).sum(-1).float()
    rin = torch.full((S, 2 * C), nan)
    rin[:, C:] = TV[:, Kcy] + (0.0 if fault == "scal_rw_missing" else scal[0] * rw) + bf
    rin[:, :C] = 0.0
    if Kcx:                                                   # latent self attention on X: L1 / TV are overwritten from their start
        T0x = B["T0T"][Kcy:].float()
        L1x = torch.full((S, Kcx, Np), nan)
        L1x[..., :N] = fmm(T0x, X.float().transpose(1, 2), order)
        realx = H.real_rows_x(d)
        if fault == "x_slot_row_not_zeroed":
            realx = realx.clone(); realx[K] = True
        px = torch.nan_to_num(L1x[:, realx, :N], nan=0.0)
        ex = torch.exp(px - px.max(-1, keepdim=True).values)
        invx = 1.0 / fsum(ex, -1, order)[..., None] if text == "plain" else (1.0 / ex.double().sum(-1, keepdim=True)).float()
        A1x = torch.zeros(S, Kcx, Np, dtype=d.T)
        A1x[:, realx, :N] = R(ex * invx)
        B["A1x"] = A1x
        TVx = fmm(A1x[..., :N], X, order)
        tokx = torch.stack([B[k] for k in d.tok_keys[d.Ey:]])[None]
        Tx = torch.zeros(S, d.Ex, Kp, C, dtype=d.T); Tx[:, :, :K] = R(tokx + TVx.reshape(S, d.Ex, Kp, C)[:, :, :K])
        Text[:, Kcy:d.KL] = Tx.reshape(S, Kcx, C)
        st = Text[:, Kcy:d.KL].double()
        Tsum[0, :, Kcy:d.KL], Tsum[1, :, Kcy:d.KL] = st.sum(-1).float(), (st * st).sum(-1).float()
        B["L1"] = L1.clone(); B["L1"].reshape(-1)[:S * Kcx * Np] = L1x.reshape(-1)
        B["TV"] = TV.clone(); B["TV"].reshape(-1)[:S * Kcx * C] = TVx.reshape(-1)
    B["Text"], B["Tsum"], B["rin"] = Text, Tsum, rin
    Tk = Text[:, :d.KL].reshape(S, El, Kp, C)[:, :, :K].float()
    B["TT"] = fmm(Tk, Tk.transpose(2, 3), order)
    Wt = R(0.05 * torch.randn(d.g, d.E * d.dgp, d.Cg, generator=g))
    B["Wt"] = Wt
    B["TW"] = fmm(Text.reshape(S, d.KLT, d.g, d.Cg).permute(0, 2, 1, 3), Wt.float().transpose(1, 2)[None], order).permute(0, 2, 1, 3).contiguous()
    fwd = dict(B)
    # ---- backward: what phase 5 receives ----
    mask = (torch.arange(Kp) < K).float()
    for nm in ("a", "ag", "aw"):
        B[nm] = R(0.3 * torch.randn(El, S, N, Kp, generator=g) * mask)
    B["Zw"] = R(0.2 * torch.randn(S, N, d.g, d.E * d.dgp, generator=g))
    dTW = torch.zeros(S, d.KLT, d.g, d.E * d.dgp, dtype=d.T)
    for l in range(El):
        z = B["Zw"][:, :, :, l * d.dgp:(l + 1) * d.dgp].float().permute(0, 2, 1, 3)
        dTW[:, l * Kp:l * Kp + K, :, l * d.dgp:(l + 1) * d.dgp] = R(fmm(B["ag"][l, :, :, :K].float().transpose(1, 2)[:, None], z, order).permute(0, 2, 1, 3))
    B["dTW"] = dTW
    dTT = torch.zeros(S, El, K, Kp, dtype=d.T)
    dTT[..., :K] = R(fmm(B["aw"][:, :, :, :K].float().permute(1, 0, 3, 2), B["a"][:, :, :, :K].float().permute(1, 0, 2, 3), order))
    B["dTT"] = dTT
    dT, dtbar = 0.1 * torch.randn(S, d.KL, C, generator=g), torch.randn(S, d.KL, generator=g)
    rbw = 0.1 * torch.randn(S * (d.E + 160 + 2 * C), generator=g)
    B["dT"], B["dtbar"], B["rbw"] = dT, dtbar, rbw
    # ---- k_finish_dT ----
    add = torch.zeros_like(dtbar) if fault == "dtbar_dropped" else dtbar / float(C)
    full = dT + add[..., None]
    dTy = torch.zeros(S, Kcyb, C, dtype=d.T)
    dTy[:, :Kcy], dTy[:, Kcy] = R(full[:, :Kcy]), R(H.drin_of(d, B)[:, C:])
    B["dTy"] = dTy
    src = dTy.float()
    if fault == "dabx_from_unrounded_dTy":
        src = torch.cat([full[:, :Kcy], H.drin_of(d, B)[:, None, C:]], 1)
    B["dabx"] = fsum(src * rw, -1, order)
    dT0 = fsum(full, 0, order)
    # ---- phase 6a ----
    B["dV"] = R(fmm(dTy, B["WfT"], order))
    dBm = torch.full((S, Kcyb, Mb), nan); dBm[:, :, :M] = fmm(B["dV"], Y.float().transpose(1, 2), order)
    B["dBm"] = dBm
    dBmT = torch.zeros(S, Kcyb, Mb, dtype=d.T)
    dBmT[:, :Kcy, :M] = R(dBm[:, :Kcy, :M])
    if fault != "dBmT_column_M_zero":
        dBmT[:, :Kcy, M] = R(B["dabx"][:, :Kcy])
    B["dBmT"] = dBmT
    dvec = torch.zeros(2 * C + Mb + 64)
    dvec[2 * C:2 * C + M], dvec[2 * C + Mb] = fsum(dBm[:, Kcy, :M], 0, order), fsum(B["dabx"][:, Kcy], 0, order)
    dA1 = torch.full((S, Kcyb, Np), nan)
    dA1[:, :, :N] = fmm(dBmT[:, :, :M + 1], B["WcK"][:, :M + 1].float().t(), order)
    if fault == "ulp_dA1":
        dA1[:, :, :N] = _one_ulp(dA1[:, :, :N])
    B["L1"] = dA1
    a1, da = A1[:, :, :N].float(), dA1[:, :, :N]
    dot = fsum(a1 * da, -1, order)[..., None]
    if fault == "softmax_bwd_without_dot":
        dot = torch.zeros_like(dot)
    if fault == "softmax_bwd_dot_of_row_above":
        dot = dot.roll(1, 1)
    dL1 = torch.zeros(S, Kcyb, Np, dtype=d.T)
    dL1[:, :, :N] = R(a1 * (da - dot))
    B["dL1"] = dL1
    dR = R(fmm(dL1[:, :Kcy, :N], B["WcT"][:M, :N].float().t(), order))                      # (S, Kcy, M)
    dRT = torch.zeros(S, M, d.Kcyp, dtype=d.T)
    if fault == "dRT_untransposed":
        dRT.reshape(S, -1)[:, :Kcy * M] = dR.reshape(S, Kcy * M)
    else:
        dRT[:, :, :Kcy] = dR.transpose(1, 2)
    B["dRT"] = dRT
    rows = S * Kcyb
    dWcK = torch.zeros(N, Mk)
    dWcK[:, :M + 1] = fmm(A1[:, :, :N].reshape(rows, N).float().t(), dBmT[:, :, :M + 1].reshape(rows, M + 1), order)
    if fault != "dWcK_second_product_missing":
        dWcK[:, :M + 2] += fmm(dL1[:, :, :N].reshape(rows, N).float().t(), Rext[:, :, :M + 2].reshape(rows, M + 2), order)
    if fault == "ulp_dWcK":
        dWcK[:, :M + 2] = _one_ulp(dWcK[:, :M + 2])
    B["dWcK"] = dWcK
    part = torch.stack([fsum(dL1[:, :, :N].float() * bc, -1, order), fsum(dL1[:, :, :N], -1, order)])      # (2, S, Kcyb)
    fin = fsum(part, 1, order)
    B["dqp"] = torch.cat([part.reshape(-1), fin.reshape(-1)])
    B["dQT"] = R(fmm(dRT[:, :, :Kcy].reshape(S * M, Kcy).float().t(), Y.reshape(S * M, Cy), order)) if fault != "dRT_untransposed" else R(torch.zeros(Kcy, Cy))
    dT0[:Kcy] += fmm(B["dQT"], B["WfT"].float().t(), order)
    B["dT0"] = dT0
    B["dWf"] = fmm(dTy.reshape(rows, C).float().t(), B["V"].reshape(rows, Cy), order) + fmm(T0y.t(), B["dQT"], order)
    abx = H._abx(d, B).float()
    dvec[:C] = fsum(dTy.float() * abx[..., None], (0, 1), 0) + fsum(T0y * fin[0, :Kcy, None], 0, order)
    dvec[C:2 * C] = fsum(dTy, (0, 1), 0) + fsum(T0y * fin[1, :Kcy, None], 0, order)
    B["dvec"] = dvec
    if Kcx:                                                   # phase 6b: dA1x into L1, dL1x into dL1 (from their start), the transposed copy
        B["dTx"] = R(full[:, Kcy:])
        dA1x = torch.full((S, Kcx, Np), nan)
        dA1x[..., :N] = fmm(B["dTx"], X.float().transpose(1, 2), order)
        B["L1"] = dA1.clone(); B["L1"].reshape(-1)[:S * Kcx * Np] = dA1x.reshape(-1)
        ax = B["A1x"][..., :N].float()
        dotx = fsum(ax * dA1x[..., :N], -1, order)[..., None]
        if fault == "x_bwd_dot_of_row_above":
            dotx = dotx.roll(1, 1)
        dL1x = torch.zeros(S, Kcx, Np, dtype=d.T)
        dL1x[..., :N] = R(ax * (dA1x[..., :N] - dotx))
        B["dL1"] = dL1.clone(); B["dL1"].reshape(-1)[:S * Kcx * Np] = dL1x.reshape(-1)
        dL1xT = torch.zeros(S, N, d.Kcxp, dtype=d.T)
        if fault == "dL1xT_row_stride_N":                     # (a copy that forgets the frame: every frame lands on frame 0)
            dL1xT[0, :, :Kcx] = dL1x[-1, :, :N].t()
        else:
            dL1xT[:, :, :Kcx] = dL1x[..., :N].transpose(1, 2)
        B["dL1xT"] = dL1xT
        dT0[Kcy:] += fmm(dL1xT[:, :, :Kcx].reshape(S * N, Kcx).float().t(), X.reshape(S * N, C), order)
    # ---- k_hop1_finalize ----
    G = {}
    G["conv_adapter.weight"] = (dWcK[:, :M] + (0.0 if fault == "dwbar_missing_from_conv_w" else dvec[2 * C:2 * C + M] / float(N))).reshape(N, M, 1, 1)
    G["conv_adapter.bias"] = dWcK[:, M] + dvec[2 * C + Mb] / float(N)
    G["fc.weight"] = B["dWf"] + (0.0 if fault == "drw_missing_from_fc_w" else dvec[:C, None])
    G["fc.bias"] = dvec[C:2 * C].clone()
    tails = {}
    for l in range(d.Ey):
        big = torch.full((Kp + 1, C), nan)
        kc = torch.arange(l * Kp, l * Kp + Kp)
        val = dT0[kc] + fin[0][kc][:, None] * rw + fin[1][kc][:, None] * bf
        nrow = K + 1 if fault == "my_tokens_row_K_written" else K
        big[:nrow] = val[:nrow] if nrow <= Kp else torch.cat([val, val[:1]])
        G[d.tok_keys[l]], tails[d.tok_keys[l]] = big[:K], big[K:]
    for l in range(d.Ey, El):
        G[d.tok_keys[l]] = dT0[l * Kp:l * Kp + K].clone()
    B["grads"], B["grads_tail"] = G, tails
    return fwd, B


def _one_ulp(x):
    """one bf16 ulp (2^-8 relative) on the element of every row that is largest in magnitude"""
    x = x.clone()
    i = x.abs().argmax(-1, keepdim=True)
    x.scatter_(-1, i, x.gather(-1, i) * (1 + 2.0 ** -8))
    return x


_SITES = {}


def _site(shape, family):
    if (shape, family) not in _SITES:
        _SITES.clear()                                                    # (one site's buffers at a time)
        cfg, S = _cfg(shape.replace("_f32", ""))
        d = _dims(cfg, S, not shape.endswith("_f32"))
        P, _ = O.init_params(cfg, seed=21)
        P = H.apply_family(P, family, cfg)
        g = torch.Generator().manual_seed(121)
        P["X"] = H.family_X(0.3 * torch.randn(S, cfg.Nx, cfg.Cx, generator=g), family, cfg)      # (the GPU module draws X first)
        Y = 0.3 * torch.randn(S, cfg.Ny, cfg.Cy, generator=g)
        _SITES[(shape, family)] = (d, P, Y)
    return _SITES[(shape, family)]


def _check_all(d, fwd, bwd):
    worst = {}
    for tag, (_w, _f, fn) in H.FORWARD.items():
        if not d.Kcx or tag in H.V2_FORWARD_Y:
            worst[tag] = fn(d, fwd)
    for tag, (_w, _f, fn) in H.BACKWARD.items():
        if not d.Kcx or tag in H.V2_BACKWARD_Y:
            worst[tag] = fn(d, bwd)
    if d.Kcx:
        for tag, (_w, _f, fn) in H.FORWARD_X.items():
            worst[tag] = fn(d, fwd)
        for tag, (_w, _f, fn) in H.BACKWARD_X.items():
            worst[tag] = fn(d, bwd)
    return worst


@pytest.mark.parametrize("shape,family", CASES)
def test_honest_emulation_stays_inside_every_bound(shape, family):
    d, P, Y = _site(shape, family)
    for order in (0, 1):
        fwd, bwd = emulate(d, P, Y, order)
        H.check_family(d, fwd["L1"], family)
        worst = _check_all(d, fwd, bwd)
        assert max(worst.values()) <= 1.0, worst
        # the exact links are exact, and the fp32 results (no bf16 store, whose unit roundoff a correct store reaches) keep room
        for tag in ("L1", "TV", "TT", "TW", "dA1", "dWcK", "dWf", "dT0", "dqrqb", "dvec", "L1x", "TVx", "dA1x", "dT0x"):
            assert worst.get(tag, 0.0) < 0.5, (tag, worst[tag])


# fault -> (the link that must fail, (shape, family) it is planted at)
FAULTS = {
    "softmax_over_Np": ("softmax", ("pad_77_71", "default")),
    "max_of_first_64": ("softmax", ("pad_77_71", "steep")),
    "inv_of_neighbour_row": ("softmax", ("pad_77_71", "peaked")),
    "kcy_row_not_zeroed": ("softmax", ("one_cross_66", "default")),
    "slot_row_not_zeroed": ("softmax", ("k20", "default")),
    "qr_qb_exchanged": ("qrqb", ("pad_77_71", "default")),
    "ab_from_M_minus_1": ("finish_T", ("pad_77_71", "default")),
    "wbar_missing": ("qrqb", ("pad_77_71", "default")),
    "scal_rw_missing": ("finish_T", ("pad_77_71", "default")),
    "dabx_from_unrounded_dTy": ("finish_dT", ("pad_77_71", "default")),
    "dtbar_dropped": ("finish_dT", ("pad_77_71", "default")),
    "dBmT_column_M_zero": ("prep_dBm", ("pad_77_71", "default")),
    "softmax_bwd_without_dot": ("softmax_bwd", ("pad_77_71", "peaked")),
    "softmax_bwd_dot_of_row_above": ("softmax_bwd", ("pad_77_71", "peaked")),
    "dRT_untransposed": ("dRT", ("pad_77_71", "default")),
    "dWcK_second_product_missing": ("dWcK", ("pad_77_71", "default")),
    "dwbar_missing_from_conv_w": ("finalize", ("pad_77_71", "default")),
    "drw_missing_from_fc_w": ("finalize", ("pad_77_71", "default")),
    "my_tokens_row_K_written": ("finalize", ("k20", "default")),
    "x_slot_row_not_zeroed": ("softmax_x", ("v2_k20", "default")),
    "x_bwd_dot_of_row_above": ("softmax_bwd_x", ("v2_k20", "peaked")),
    "dL1xT_row_stride_N": ("softmax_bwd_x", ("v2_k20", "default")),
    "ulp_L1": ("L1", ("pad_77_71", "default")),
    "ulp_TV": ("TV", ("pad_77_71", "default")),
    "ulp_dA1": ("dA1", ("pad_77_71", "default")),
    "ulp_dWcK": ("dWcK", ("pad_77_71", "default")),
}


@pytest.mark.parametrize("fault", list(FAULTS))
def test_planted_fault_fails_its_link(fault):
    tag, (shape, family) = FAULTS[fault]
    if family == "steep":
        # a maximum taken from the first 64 columns is the same softmax in exact arithmetic: it shows once exp overflows, i.e. when a row's
        # maximum beyond column 64 lies more than 88 above the one inside -- the peaked family with the tokens scaled by another 20
        d, P, Y = _site(shape, "peaked")
        P = {k: (v * 20.0 if k.endswith(".my_tokens") else v) for k, v in P.items()}
    else:
        d, P, Y = _site(shape, family)
    fwd, bwd = emulate(d, P, Y, 0, fault)
    fn = H.LINKS[tag][2]
    is_fwd = tag in H.FORWARD or tag in H.FORWARD_X
    with pytest.raises(H.ProductMismatch):
        fn(d, fwd if is_fwd else bwd)
    # ... and the same link passes without the fault, on the same inputs
    fwd, bwd = emulate(d, P, Y, 0, None)
    assert fn(d, fwd if is_fwd else bwd) <= 1.0


def test_a_family_without_its_property_fails():
    """check_family asserts (it never skips): a flat site is not peaked, a peaked one not flat"""
    d, P, Y = _site("pad_77_71", "flat")
    fwd, _ = emulate(d, P, Y, 0)
    with pytest.raises(AssertionError):
        H.check_family(d, fwd["L1"], "peaked")
    d, P, Y = _site("pad_77_71", "peaked")
    fwd, _ = emulate(d, P, Y, 0)
    with pytest.raises(AssertionError):
        H.check_family(d, fwd["L1"], "flat")
