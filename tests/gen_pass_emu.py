"""A torch fp32 emulation of one site's per-token bottleneck-space passes in the WORKSPACE LAYOUT of the generalised (csrc/tile_gen.inc) and
any-shape (csrc/tile_kernels.hip) forms, for tests/test_gen_pass_checker.py: `EmuSite` offers the named buffers the way
tests/test_gen_passes_fp64_gpu.py::GenSite does, so the CPU test runs the GPU module's own checks (`_forward`, `_backward`) on it -- an honest
emulation must pass them, a planted fault must fail them.

Written from the formulas of oracle/algebra_ref.py, not from the library.  The operands upstream of the passes (X, the folded weights, the
latent tokens' TT / TW / Tsum, the logits, Gq / usum / vh / H, the router's probabilities, dOut and everything phase 1 and 2 of the backward
make of it) are the oracle's own fp32 tensors, padded into the plan's layout (entries per group to dgp, latent slots to Kp, the groups merged
where the plan merged them).  The passes themselves: fp32 arithmetic one operation at a time, every sum accumulated one term at a time in an
order shuffled by `seed`, the mat-vecs of the bf16 generalised form with both operands as two bf16 planes and lo x lo dropped
(csrc/tile_lane.h::mmT_split), stores round-to-nearest-even.  The rounds of resident experts do not change the arithmetic; what they can
get wrong is planted by the test."""
from types import SimpleNamespace

import torch

from oracle import avmoe_oracle as O
from oracle.algebra_ref import AlgebraRef

F32 = torch.float32
POISON = float("nan")


def bf(x):
    return x.bfloat16().float()


def ssum(terms, seed):
    """fp32 sum over the LAST axis, one term at a time, in a shuffled order"""
    g = torch.Generator().manual_seed(seed)
    acc = torch.zeros(terms.shape[:-1], dtype=F32)
    for k in torch.randperm(terms.shape[-1], generator=g).tolist():
        acc = acc + terms[..., k]
    return acc


def mv(v, M, planes, seed):
    """w[..., c] = sum_k v[..., k] M[..., k, c]; planes: hi.hi + hi.lo + lo.hi of the two-plane operands, fp32 accumulation"""
    if planes:
        vh, Mh = bf(v), bf(M)
        vl, Ml = bf(v - vh), bf(M - Mh)
        terms = torch.cat([vh[..., :, None] * Mh, vh[..., :, None] * Ml, vl[..., :, None] * Mh], -2)
    else:
        terms = v[..., :, None] * M
    return ssum(terms.transpose(-1, -2), seed)


def _sym(M):
    return M + M.transpose(-1, -2) - torch.diag_embed(torch.diagonal(M, dim1=-2, dim2=-1))


class EmuSite:
    """the buffers of one emulated forward + section 1 of the backward, named and laid out as the workspace"""

    def __init__(self, cfg, S, seed, bf16, lay, order=0):
        self.cfg, self.S, self.bf16, self.lay = cfg, S, bf16, lay
        self.T = torch.bfloat16 if bf16 else F32
        self.E, self.N, self.NT = cfg.E, cfg.Nx, S * cfg.Nx
        self.g, self.dg, self.dgp, self.lat, self.El, self.K, self.Kp = lay.g, lay.dg, lay.dgp, lay.lat, lay.El, lay.K, lay.Kp
        self.KL, self.KLT, self.KLp, self.KP, self.KPp, self.XW = lay.KL, lay.KLT, lay.KLp, lay.KP, lay.KPp, lay.XW
        self.zbf = lay.zsz == 2
        self.ZT = torch.bfloat16 if self.zbf else F32
        self.planes = bf16 and lay.family == "tile_gen"
        self.relu = torch.tensor([e < cfg.E_m for e in range(cfg.E)])
        self.P, B = O.init_params(cfg, seed=seed)
        gen = torch.Generator().manual_seed(seed + 100)
        X = 0.3 * torch.randn(S, cfg.Nx, cfg.Cx, generator=gen)
        Y = 0.3 * torch.randn(S, cfg.Ny, cfg.Cy, generator=gen)
        self.G = torch.randn(S, cfg.Nx, cfg.Cx, generator=gen)
        st = bf if bf16 else (lambda v: v)
        self.st, self.zst = st, (bf if self.zbf else (lambda v: v))
        X, Y, self.G = st(X), st(Y), st(self.G)                            # the site's inputs arrive in its type
        self.run = SimpleNamespace(X=X.to(self.T), dev=torch.device("cpu"), out=torch.zeros(1))
        self.A = AlgebraRef(cfg, self.P, B)
        self.A.forward(X, Y, training=True)
        pfx = cfg.expert_prefixes()
        self.gv = torch.tensor([float(self.A.sv["E"][e]["gv"]) if e in lay.lat else 0.0 for e in range(cfg.E)])
        assert all(float(self.P[f"{pfx[e]}.{'gate_av' if e < cfg.E_m else 'gate_self'}"]) == float(self.gv[e]) for e in lay.lat)
        self.b = {}
        self._operands()
        self.forward(order)
        self.backward(order)

    # ---- access, as GenSite -----------------------------------------------------------------------------------------------------------
    def dev(self, name, dtype, shape):
        t = self.b[name].reshape(-1)
        if t.dtype != dtype:
            t = t.view(dtype)
        n = 1
        for k in shape:
            n *= k
        return t[:n].reshape(shape)

    def f32(self, name, shape):
        return self.dev(name, F32, shape)

    def z(self, name):
        return self.dev(name, self.ZT, (self.NT, self.g, self.E, self.dgp))

    def zT(self, name):
        return self.dev(name, self.T, (self.NT, self.g, self.E, self.dgp))

    def tokE(self, name):
        v = self.f32(name, (2, self.E, self.NT))
        return v[0].t(), v[1].t()

    def latent(self):
        S, N, NT, El, Kp, K = self.S, self.N, self.NT, self.El, self.Kp, self.K
        L2 = self.f32("L2", (NT, El, Kp))
        a = self.dev("a", self.T, (El, NT, Kp)).permute(1, 0, 2)
        TT = self.f32("TT", (S, El, K, K))
        TWall = self.f32("TW", (S, self.KLT, self.g, self.E, self.dgp))
        TW = torch.stack([TWall[:, l * Kp:(l + 1) * Kp, :, e] for l, e in enumerate(self.lat)], 1)
        Tsum = self.f32("Tsum", (2, S, self.KLT))[0][:, :self.KL].reshape(S, El, Kp).repeat_interleave(N, 0)
        return L2, a, TT, TW, Tsum

    def put(self, name, t, dtype=None):
        self.b[name] = t.contiguous().to(dtype or F32)

    # ---- the oracle's tensors in the plan's layout ------------------------------------------------------------------------------------------
    def cols(self, x):
        """(..., g0, dg0) of the oracle -> (..., g, dgp): the groups merged where the plan merged them, entries padded with 0"""
        x = x.reshape(*x.shape[:-2], self.g, self.dg)
        return torch.cat([x, torch.zeros(*x.shape[:-1], self.dgp - self.dg)], -1)

    def mats(self, M):
        """(g0, dg0, dg0) -> (g, dgp, dgp): block-diagonal where merged"""
        if self.lay.merged:
            M = torch.block_diag(*M)[None]
        out = torch.zeros(self.g, self.dgp, self.dgp)
        out[:, :self.dg, :self.dg] = M
        return out

    def _operands(self):
        cfg, sv, S, N, NT, E, g, dg, dgp, K, Kp, El = self.cfg, self.A.sv, self.S, self.N, self.NT, self.E, self.g, self.dg, self.dgp, self.K, self.Kp, self.El
        C, g0 = cfg.Cx, cfg.groups
        Cg0, dg0 = C // g0, cfg.d // g0
        ex = sv["E"]
        X = sv["X"]
        # Wt [group][expert][dgp][c]: one group of block-diagonal rows where merged (fwd_kernels.hip:1096-1105)
        Wt = torch.zeros(g, E, dgp, C // g)
        for e in range(E):
            w = ex[e]["Wt"]                                                # (g0, dg0, Cg0)
            if self.lay.merged:
                for i in range(g0):
                    Wt[0, e, i * dg0:(i + 1) * dg0, i * Cg0:(i + 1) * Cg0] = w[i]
            else:
                Wt[:, e, :dg] = w
        self.put("Wt", self.st(Wt).reshape(g, E * dgp, C // g), self.T)
        self.put("wsum", torch.stack([self.cols(ex[e]["wsum"]) for e in range(E)], 1))
        self.put("dconst", torch.stack([self.cols(ex[e]["dconst"]) for e in range(E)], 1))
        self.put("sx", torch.stack([X.sum(-1).reshape(NT), (X * X).sum(-1).reshape(NT)]))
        L2 = torch.full((NT, El, Kp), 50.0)                                # what the padding slots of the logits hold is nobody's business: large
        TT = torch.zeros(S, El, K, K)
        TW = torch.zeros(S, self.KLT, g, E, dgp)
        Tsum = torch.zeros(2, S, self.KLT)
        for l, e in enumerate(self.lat):
            L2[:, l, :K] = ex[e]["L2"].reshape(NT, K)
            TT[:, l] = ex[e]["TT"]
            TW[:, l * Kp:l * Kp + K, :, e] = self.cols(ex[e]["TW"])
            Tsum[0, :, l * Kp:l * Kp + K] = ex[e]["T"].sum(-1)
        self.put("L2", L2); self.put("TT", TT); self.put("TW", TW); self.put("Tsum", Tsum)
        self.put("probs", sv["p"])
        self.put("Gq", torch.stack([self.mats(ex[e]["G"]) for e in range(E)], 1))
        us = torch.stack([self.cols(ex[e]["usum"]) for e in range(E)], 1)
        vh = torch.stack([self.cols(ex[e]["vh"]) for e in range(E)], 1)
        h2 = [ex[e]["h2"].reshape(g, -1) for e in range(E)]                # (g, Cg): the per-group parts of H1, H2
        H1p = torch.stack([h.sum(-1) for h in h2], 1)
        H2p = torch.stack([(h * h).sum(-1) for h in h2], 1)
        self.put("uvh", torch.cat([us.reshape(-1), vh.reshape(-1), H1p.reshape(-1), H2p.reshape(-1)]))

    # ---- the forward passes ------------------------------------------------------------------------------------------------------------------
    def forward(self, order):
        cfg, S, N, NT, E, g, dg, dgp, K, Kp, El = self.cfg, self.S, self.N, self.NT, self.E, self.g, self.dg, self.dgp, self.K, self.Kp, self.El
        C, st, zst = float(cfg.Cx), self.st, self.zst
        X = self.run.X.float().reshape(NT, g, -1)
        Wt = self.dev("Wt", self.T, (g, E * dgp, cfg.Cx // g)).float()
        self.Zx = zst(torch.einsum("tgc,gjc->tgj", X, Wt)).reshape(NT, g, E, dgp)       # the down projection's own store
        # pre_small
        a = torch.zeros(El, NT, Kp)
        rmu = torch.zeros(2, E, NT)
        Z = torch.zeros(NT, g, E, dgp)
        self.put("a", a, self.T)
        for e in range(E):
            av, rmu[0, e], rmu[1, e], Z[:, :, e] = self.pre_small_expert(e, order)
            if e in self.lat:
                a[self.lat.index(e)] = av
        self.put("a", a, self.T); self.put("rmu", rmu); self.put("Z", Z, self.ZT)
        # BatchNorm-1: column sums over the tokens, finalized in double (fwd_kernels.hip:1000-1016); the padding entries stay 0
        s0, s1 = ssum(Z.permute(1, 2, 3, 0), order + 7), ssum((Z * Z).permute(1, 2, 3, 0), order + 8)
        m = s0.double() / NT
        v = (s1.double() / NT - m * m).clamp_min(0.0)
        mean, var = m.float(), v.float()
        rstd = torch.rsqrt(var + cfg.bn_eps)
        pfx = cfg.expert_prefixes()
        w1 = torch.stack([self.cols(self.P[f"{p}.bn1.weight"].reshape(cfg.groups, -1)) for p in pfx], 1)
        b1 = torch.stack([self.cols(self.P[f"{p}.bn1.bias"].reshape(cfg.groups, -1)) for p in pfx], 1)
        sc = w1 * rstd
        bn1 = torch.stack([mean, rstd, sc, b1 - mean * sc])
        bn1[..., dg:] = 0.0
        self.put("bn1", bn1)
        # mid
        zp = self.zprime()
        Zp = st(zp)
        self.put("Zp", Zp, self.T)
        self.put("mz", ssum(Zp.permute(1, 2, 3, 0), order + 9) / NT)
        self.put("Szz", ssum((Zp[..., :, None] * Zp[..., None, :]).permute(1, 2, 3, 4, 0), order + 10) / NT)
        # post_small
        rpmup = torch.zeros(2, E, NT)
        Ap = torch.full((NT, g, self.KPp), POISON)
        for e in range(E):
            rpmup[0, e], rpmup[1, e], Ap[:, :, e * dgp:(e + 1) * dgp], Ap[:, :, E * dgp + 3 * e:E * dgp + 3 * e + 3] = self.post_small_expert(e, order)
        self.put("rpmup", rpmup)
        self.put("Apost", self.poisoned(st(Ap), Ap), self.T)

    def pre_small_expert(self, e, order, slots=None, tt_stride=None):
        """-> a (NT, Kp) as stored (None without a latent slot), rr, mu (NT,), z (NT, g, dgp) as stored, of expert e.  What a faulty kernel
        would do instead: slots = how many latent slots the softmax takes in (K; K + 1 leaves a padding slot in); tt_stride = the row stride
        TT is read with (K; Kp reads the wrong rows of the K x K matrix, and beyond it)"""
        cfg, S, N, NT, g, E, dgp, K, Kp = self.cfg, self.S, self.N, self.NT, self.g, self.E, self.dgp, self.K, self.Kp
        C, st = float(cfg.Cx), self.st
        L2, _a, TT, TW, Tsum = self.latent()
        wsum, dconst, sx = self.f32("wsum", (g, E, dgp)), self.f32("dconst", (g, E, dgp)), self.f32("sx", (2, NT))
        Sx, Sxx = sx[0].clone(), sx[1].clone()
        gv = self.gv[e]
        p, av = torch.zeros(NT, g, dgp), None
        if e in self.lat:
            l = self.lat.index(e)
            n = K if slots is None else slots
            lg = L2[:, l, :n]
            ex = torch.exp(lg - lg.max(-1, keepdim=True).values)
            ex = torch.cat([ex, torch.zeros(NT, Kp - n)], -1)               # masked slots add an exact 0
            av = st(ex * (1.0 / ssum(ex, order + 1))[:, None])
            tb = Tsum[:, l] / C
            u1, u2 = ssum(av * tb, order + 2), ssum(av[:, :n] * lg, order + 3)
            TTp = torch.zeros(S, Kp, Kp)
            if tt_stride is None:
                TTp[:, :K, :K] = TT[:, l]
            else:                                                          # tt[k1 * stride + k2] inside the flat (S, El, K, K) buffer
                flat = self.f32("TT", (S * self.El * K * K,))
                k1, k2 = torch.meshgrid(torch.arange(K), torch.arange(K), indexing="ij")
                for s_ in range(S):
                    TTp[s_, :K, :K] = flat[((s_ * self.El + l) * K * K + k1 * tt_stride + k2).clamp_max(flat.numel() - 1)]
            w = mv(av, TTp.repeat_interleave(N, 0), self.planes, order + 4)
            u3 = ssum(w * av, order + 5)
            Sx = Sx + gv * C * u1
            Sxx = Sxx + (2.0 * gv * u2 + gv * gv * u3)
            p = mv(av, TW[:, l].reshape(S, Kp, g * dgp).repeat_interleave(N, 0), self.planes, order + 6).reshape(NT, g, dgp)
        mu = Sx / C
        rr = torch.rsqrt((Sxx / C - mu * mu).clamp_min(0.0) + cfg.ln_eps)
        zr = self.Zx[:, :, e] + gv * p
        return av, rr, mu, self.zst(rr[:, None, None] * (zr - mu[:, None, None] * wsum[:, e]) + dconst[:, e])

    def post_small_expert(self, e, order, cst=None, odd_from=None, w_scale=None):
        """-> rp, mup (NT,), the main columns (NT, g, dgp) and the scalar columns (NT, 1, 3) of expert e before their store.  What a faulty kernel
        would do instead: cst = the expert whose STAGED constants (Gq, us, vh, scale, shift) are used; odd_from = the expert whose segment the
        last 16-entry chunk of z is loaded from; w_scale (NT,) = a factor on the mat-vec's result"""
        cfg, S, N, NT, g, E, dgp = self.cfg, self.S, self.N, self.NT, self.g, self.E, self.dgp
        C, c = float(cfg.Cx), (e if cst is None else cst)
        us, vh, H1p, H2p = self.uvh()
        bn1 = self.f32("bn1", (4, g, E, dgp))
        Z = self.z("Z").float()
        z = Z[:, :, e].clone()
        if odd_from is not None:
            z[..., dgp - 16:] = Z[:, :, odd_from, dgp - 16:]
        y = z * bn1[2][:, c] + bn1[3][:, c]
        zp = y.clamp_min(0.0) if bool(self.relu[e]) else y
        w = mv(zp, self.f32("Gq", (g, E, dgp, dgp))[:, c], self.planes, order + 11)
        if w_scale is not None:
            w = w * w_scale[:, None, None]
        qv = self.f32("probs", (S, E)).repeat_interleave(N, 0)[:, e]
        So = ssum((zp * us[:, c]).reshape(NT, -1), order + 12) + ssum(H1p[:, e], order + 13)
        Soo = ssum((zp * (w + 2.0 * vh[:, c])).reshape(NT, -1), order + 14) + ssum(H2p[:, e], order + 15)
        mup = So / C
        rp = torch.rsqrt((Soo / C - mup * mup).clamp_min(0.0) + cfg.ln_eps)
        return rp, mup, (qv * rp)[:, None, None] * zp, torch.stack([qv * rp, -qv * rp * mup, qv], -1)[:, None, :]

    def poisoned(self, stored, raw):
        """the workspace poison (all bits set) wherever `raw` is NaN, in the bit pattern of the site's type"""
        if self.bf16:
            bits = stored.bfloat16().view(torch.int16).clone()
            bits[torch.isnan(raw)] = -1
            return bits.view(torch.bfloat16)
        bits = stored.float().view(torch.int32).clone()
        bits[torch.isnan(raw)] = -1
        return bits.view(F32)

    def uvh(self):
        g, E, dgp = self.g, self.E, self.dgp
        DZ = g * E * dgp
        u = self.f32("uvh", (2 * DZ + 2 * g * E,))
        return u[:DZ].reshape(g, E, dgp), u[DZ:2 * DZ].reshape(g, E, dgp), u[2 * DZ:2 * DZ + g * E].reshape(g, E), u[2 * DZ + g * E:].reshape(g, E)

    def zprime(self):
        bn1 = self.f32("bn1", (4, self.g, self.E, self.dgp))
        y = self.z("Z").float() * bn1[2] + bn1[3]
        return torch.where(self.relu.view(1, 1, -1, 1), y.clamp_min(0.0), y)

    # ---- section 1 of the backward -------------------------------------------------------------------------------------------------------------
    def backward(self, order):
        cfg, sv, S, N, NT, E, g, dg, dgp, K, Kp, El = self.cfg, self.A.sv, self.S, self.N, self.NT, self.E, self.g, self.dg, self.dgp, self.K, self.Kp, self.El
        C, st, zst, ntot = float(cfg.Cx), self.st, self.zst, self.NT
        g0 = cfg.groups
        Cg0 = cfg.Cx // g0
        ex = sv["E"]
        dout = self.G
        doutg = dout.reshape(S, N, g0, Cg0)
        # phase 1 and 2 with the oracle's formulas (algebra_ref.py:295-351): dApost whole (one fp32 array), dm = dmz / NT, sdSzz = sym(dSzz) / NT
        dAp = torch.full((NT, g, self.KPp), POISON)
        dm, sdSzz = torch.zeros(g, E, dgp), torch.zeros(g, E, dgp, dgp)
        for e in range(E):
            x = ex[e]
            dAz = torch.einsum("snic,icj->snij", doutg, x["Bmain"])
            dAp[:, :, e * dgp:(e + 1) * dgp] = self.cols(dAz).reshape(NT, g, dgp)
            Bh, Bg, Bb = (x[k].reshape(g, -1) for k in ("Bh", "Bg", "Bb"))
            dg_ = dout.reshape(NT, g, -1)
            dAp[:, :, E * dgp + 3 * e:E * dgp + 3 * e + 3] = torch.stack([(dg_ * Bh).sum(-1), (dg_ * Bg).sum(-1), (dg_ * Bb).sum(-1)], -1)
            zp, q, rp, mup = x["zp"], x["q"], x["rp"], x["mup"]
            da1, da2 = dout @ x["Bh"], dout @ x["Bg"]
            zz = (dAz * zp).sum((-1, -2))
            drp = q * zz + q * da1 - q * mup * da2
            dvarp = drp * (-0.5) * rp ** 3
            dSoo = dvarp / C
            dSo = (-q * rp * da2 - 2 * mup * dvarp) / C
            dBmain = x["gate"] * torch.einsum("snic,snij->icj", doutg, x["Az"])
            dBh = x["gate"] * torch.einsum("snc,sn->c", dout, x["c1"]).reshape(g0, Cg0)
            Wh, h2, k2, Wu_g, gp = x["Wh"], x["h2"], x["k2"], x["Wu_g"], x["gp"]
            dusum = torch.einsum("sn,snij->ij", dSo, zp)
            dG = torch.einsum("sn,snij,snil->ijl", dSoo, zp, zp)
            dvh = 2 * torch.einsum("sn,snij->ij", dSoo, zp)
            dWh = gp[..., None] * dBmain + torch.einsum("ijl,icl->icj", _sym(dG), Wh) + dusum[:, None, :] + dvh[:, None, :] * h2[..., None]
            dh2 = gp * dBh + torch.einsum("ij,icj->ic", dvh, Wh) + dSo.sum() + 2 * h2 * dSoo.sum()
            dk2 = (dWh * Wu_g).sum(-1) - x["mo"] * dh2
            dv2 = dk2 * x["g2"] * (-0.5) * x["rs2"] ** 3
            dmo = -k2 * dh2 - 2 * x["mo"] * dv2
            dm[:, e] = self.cols(torch.einsum("ic,icj->ij", dmo, Wu_g) / ntot)
            sdSzz[:, e] = self.mats(_sym(torch.einsum("ic,icj,icl->ijl", dv2, Wu_g, Wu_g)) / ntot)
        self.put("dAp", dAp)
        self.put("dApx", torch.full((NT, g, self.XW), POISON))
        dsm = torch.zeros(8, g, E, dgp)
        dsm[2] = dm
        self.put("sdSzz", sdSzz)
        # post_small_bwd
        us, vh, _H1p, _H2p = self.uvh()
        qv = self.f32("probs", (S, E)).repeat_interleave(N, 0)
        rp, mup = self.tokE("rpmup")
        zp = self.zprime()
        y = self.z("Z").float() * self.f32("bn1", (4, g, E, dgp))[2] + self.f32("bn1", (4, g, E, dgp))[3]
        d = torch.nan_to_num(dAp[:, :, :E * dgp]).reshape(NT, g, E, dgp)
        dax = dAp[:, :, E * dgp:self.KP].reshape(NT, g, E, 3)
        da = ssum(dax.permute(0, 2, 3, 1), order + 20)                     # (NT, E, 3): the groups' parts
        tok = lambda x: x.permute(0, 2, 1, 3).reshape(NT, E, g * dgp)
        zz = ssum(tok(d * zp), order + 21)
        drp = qv * zz + qv * da[..., 0] - qv * mup * da[..., 1]
        dmup = -qv * rp * da[..., 1]
        dvarp = drp * (-0.5) * rp * rp * rp
        dSoo = dvarp / C
        dmup = dmup - 2.0 * mup * dvarp
        dSo = dmup / C
        w = mv(zp, self.f32("Gq", (g, E, dgp, dgp)), self.planes, order + 22)
        xx = lambda v: v[:, None, :, None]
        dz1 = zst(xx(qv * rp) * d + (xx(dSo) * us + xx(dSoo) * (2.0 * w + 2.0 * vh)))
        self.put("Zp", st(zp), self.T)
        Zw1 = st(xx(dSoo) * zp)
        self.put("dGq", ssum((Zw1[..., :, None] * st(zp)[..., None, :]).permute(1, 2, 3, 4, 0), order + 23))
        # mid_bwd
        w2 = mv(zp, sdSzz, self.planes, order + 24)
        d2 = dz1 + dm + w2
        dzp = torch.where(self.relu.view(1, 1, -1, 1) & (zp <= 0), torch.zeros_like(d2), zst(d2))
        self.put("dzp", dzp, self.ZT)
        bn1 = self.f32("bn1", (4, g, E, dgp))
        Z = self.z("Z").float()
        zh = (Z - bn1[0]) * bn1[1]
        dsm[3] = ssum(dzp.permute(1, 2, 3, 0), order + 25) / NT
        dsm[4] = ssum((dzp * zh).permute(1, 2, 3, 0), order + 26) / NT
        self.put("dsm", dsm)
        # pre_small_bwd
        rr_, mu_ = self.tokE("rmu")
        rr, mu = rr_[:, None, :, None], mu_[:, None, :, None]
        wsum, dconst = self.f32("wsum", (g, E, dgp)), self.f32("dconst", (g, E, dgp))
        dz = bn1[2] * (dzp - dsm[3] - (Z - bn1[0]) * bn1[1] * dsm[4])
        zc = (Z - dconst) * (1.0 / rr)
        sdr, sdm = ssum(tok(dz * zc), order + 27), ssum(tok(dz * wsum), order + 28)
        dmu = -rr_ * sdm
        dvar = sdr * (-0.5) * rr_ * rr_ * rr_
        dSxx = dvar / C
        dmu = dmu - 2.0 * mu_ * dvar
        dSx = dmu / C
        dzr = rr * dz                                                      # fp32: what the any-shape kernel keeps in its LDS tile
        self.put("Zw", st(dzr), self.T)
        accx, accxx = torch.zeros(NT), torch.zeros(NT)
        for e in range(E):
            accx, accxx = accx + dSx[:, e], accxx + dSxx[:, e]
        dL2x = torch.full((NT, self.KLp), POISON)
        dL2x[:, self.KL], dL2x[:, self.KL + 1] = accx, 1.0
        self.put("rs2x", 2.0 * accxx)
        self.put("dslat", torch.stack([torch.stack([dSx[:, e], dSxx[:, e]]) for e in self.lat]))
        # the hop-2 block: the generalised kernel reads dzraw back as stored, the any-shape kernel keeps it in fp32
        L2, a, TT, TW, Tsum = self.latent()
        a = a.float()
        src = st(dzr) if self.lay.family == "tile_gen" else dzr
        for l, e in enumerate(self.lat):
            gv = self.gv[e]
            tb = Tsum[:, l] / C
            av = a[:, l]
            TTp = torch.zeros(S, Kp, Kp)
            TTp[:, :K, :K] = TT[:, l]
            ta = mv(av, TTp.repeat_interleave(N, 0), self.planes, order + 30)
            twd = mv(src[:, :, e].reshape(NT, g * dgp), TW[:, l].reshape(S, Kp, g * dgp).transpose(1, 2).repeat_interleave(N, 0), self.planes, order + 31)
            du1, du2, du3 = dSx[:, e] * gv * C, 2.0 * gv * dSxx[:, e], gv * gv * dSxx[:, e]
            x1 = lambda v: v[:, None]
            dd = gv * twd + x1(du1) * tb + x1(du2) * torch.nan_to_num(L2[:, l]) + 2.0 * x1(du3) * ta
            dd[:, K:] = 0.0
            sada = ssum(av * dd, order + 32)
            dL2x[:, l * Kp:(l + 1) * Kp] = x1(du2) * av + av * (dd - x1(sada))
        self.put("dL2x", self.poisoned(st(dL2x), dL2x), self.T)
