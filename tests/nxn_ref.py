"""fp64 references and element-wise bounds for the strip kernels of the AVVP N x N block (csrc/nxn_att.hip), one op of avmoe_nxn_strip
(include/avmoe.h) at a time, from the operands exactly as the kernel read them (bf16 and fp32 are exact in fp64).  Same style as
tests/stream_product_ref.py / tests/pass_ref.py; check_bound, check_untouched and EPS_* come from there.

    att[i][j] = exp(X_i . X_j - lse_i)        per frame;  i: the row of the softmax ("query"), j: its column ("key")

Every bound is a sum of terms, each named after the line of nxn_att.hip that causes it.  Nothing is fitted to a measured error.

  SCORES   acc[tm][t] = mfma(kf, qf, acc) over C / 32 steps (:107, :256, :440-448): fp32 accumulation of C products in any order,
           e_s = C * EPS_ACC * (|X| |X|^T)   (EPS_ACC = 2^-23 per term as in stream_product_ref: gamma_k with a factor 2 for an accumulator
           that does not round to nearest).  The same for g = X dxr^T (:441, :448, and kk_nxn_att with Kt = dxr).
  S - LSE  `acc - l` (:139, :267, :275, :470) is one fp32 subtraction: 2^-24 at max(|s|, |lse|, |s - lse|).  Together with e_s this is an
           ABSOLUTE error of the argument of exp, i.e. a RELATIVE error of att.
  EXPF     __expf(x) is the native exponential: exp2 of fl32(x * fl32(log2 e)) by the v_exp_f32 instruction (HIP math API: "__expf: fast
           approximate", ROCm device libs native_exp; the CDNA3 / CDNA4 ISA guides give v_exp_f32 1 ulp).  The rounded constant and the
           rounded product are 2 * 2^-24 relative on the argument = EPS_ACC * |x| absolute, again a relative error of the result; the
           instruction itself EPS_ACC relative.  Results below the smallest normal fp32 may be flushed, and bf16 denormals may be flushed
           by the matrix pipe: TINY = 2^-125 absolute.
  ATT->BF16  pb = (__bf16)acc (:285), rb() (:405, :470), pack2 of the stored att (:139): EPS_BF16 relative, on every path -- the strip
           kernels keep the rounding of the stored softmax they replaced.  A kernel that did NOT round here would sit inside the same
           bound (the term is an allowance, not a requirement): tests/test_nxn_checker.py says so.
  DS       ds = rb(att) * (g - d0), then (__bf16)ds (:470, :475): e_g as SCORES; the subtraction 2^-24 at |g| + |rowdot| (the
           cancellation term); the product 2^-24; the second bf16 rounding EPS_BF16.  kk_nxn_att's backward (:136) multiplies the GIVEN
           att_in, so its att carries no error.
  PRODUCT2 accY = mfma(af, pb, accY) over all N streamed rows (:305, :497): the operand's error against |V|, plus N * EPS_ACC on the
           magnitudes.
  STORE    xr: pack2 (:318), EPS_BF16.  Y / DXQ / DXK: bflo(ol) + y in fp32 (2^-24), then pack2 of the sum (:334, :511), ONE bf16 rounding.
  ROWDOT   dot += X y over the lane's C / 4 entries, two shuffles (:333-338): C fp32 terms on |X| . |y|, plus |X| . e_y of the unrounded y.
  LSE      sweep 0 (:110-124, :146-160).  With M the row maximum, lse = M + log(sum_j exp(s_j - M)).  Term j reaches the sum as
           __expf(s_j - m_k) times the rescales __expf(m_k - m_k') of every later change of the running maximum and of the two shuffle
           merges; the arguments of all these exponentials add up to M - s_j, so term j carries (relative): e_s(j) + (EPS_ACC + 2^-24)
           (M - s_j) (argument scaling, subtractions) + (N / 128 + 3) EPS_ACC (the exponentials themselves: its own, one rescale per tile,
           two merges) + (N / 128 + 2) 2^-24 (the rescale products) + (N / 4 + N / 128 + 2) EPS_ACC (the additions on its way: 32 per tile
           and lane).  These are weighted by exp(s_j - M) / sum.  Then __logf = v_log_f32 * ln 2 (1 ulp + the constant + the product:
           2^-22 |log|, and never better than one ulp of its argument: EPS_ACC) and the final fp32 add, 2^-24 |lse|.

Works on CPU and GPU tensors alike."""
import torch

from tests.stream_product_ref import EPS_ACC, EPS_BF16, check_bound, check_untouched  # noqa: F401  (re-exported for the tests)

U32 = 2.0 ** -24           # one fp32 rounding to nearest
TINY = 2.0 ** -125         # flushed fp32 result of v_exp_f32 / flushed bf16 denormal operand
OPS = ("STATS", "ATT", "ATT_FROM_LSE", "XR", "Y", "DXQ", "DXK", "ATT_BWD")
FAMILIES = ("flat", "peaked", "late_max", "early_max", "frame_scales")
CS = (96, 192)
SHAPES = ((1, 128), (3, 256), (2, 384))      # (frames, N): one tile, no prefetch | two tiles, frame offsets | three tiles, prefetch taken and not taken


def make_inputs(family, frames, N, C, seed=0):
    """(X, dxr) bf16 on the CPU.  flat: 0.1 randn (attention near uniform: every key counts); peaked: 0.3 randn (what the rest of the suite
    draws: attention near the identity); late_max / early_max: flat with three tokens of the last / first key tile scaled by 12 (the running
    maximum is replaced in the last tile / never after the first; most exponentials underflow); frame_scales: frame f drawn at 0.05 (f + 1)."""
    g = torch.Generator().manual_seed(1000 * seed + 10 * N + C + FAMILIES.index(family))
    X = torch.randn(frames, N, C, generator=g)
    if family == "peaked":
        X = 0.3 * X
    elif family == "frame_scales":
        X = X * (0.05 * (torch.arange(frames) + 1.0))[:, None, None]
    else:
        X = 0.1 * X
        if family in ("late_max", "early_max"):
            base = N - 128 if family == "late_max" else 0
            X[:, [base + 5, base + 70, base + 127]] *= 12.0
    dxr = 0.1 * torch.randn(frames, N, C, generator=g)
    return X.bfloat16(), dxr.bfloat16()


def row_noise(frames, N, scale, seed, uniform=True):
    g = torch.Generator().manual_seed(77 + seed)
    return (torch.rand(frames, N, generator=g) * 2 - 1) * scale if uniform else torch.randn(frames, N, generator=g) * scale


class NxnRef:
    """The fp64 side of one (X, dxr): scores and their error terms are formed once and shared by the ops."""

    def __init__(self, X, dxr=None):
        self.X = X.double()
        self.Xa = self.X.abs()
        self.F, self.N, self.C = X.shape
        self.s = self.X @ self.X.transpose(1, 2)
        self.es = self.C * EPS_ACC * (self.Xa @ self.Xa.transpose(1, 2))                       # SCORES
        if dxr is not None:
            self.D = dxr.double()
            self.Da = self.D.abs()
            self.g = self.X @ self.D.transpose(1, 2)                                          # g[i][j] = X_i . dxr_j
            self.eg = self.C * EPS_ACC * (self.Xa @ self.Da.transpose(1, 2))
        self._att = {}

    # ---- lse --------------------------------------------------------------------------------------------------------------------------
    def lse(self):
        s, es, N = self.s, self.es, self.N
        nt = N // 128
        M = s.max(-1, keepdim=True).values
        w = torch.exp(s - M)
        L = w.sum(-1)
        ref = M[..., 0] + L.log()
        dist = (M - s) + 2 * es.max(-1, keepdim=True).values                                  # (the kernel's maximum is that of ITS scores)
        rel = es + (EPS_ACC + U32) * dist + (nt + 3) * EPS_ACC + (nt + 2) * U32 + (N // 4 + nt + 2) * EPS_ACC
        e_sum = (w * torch.expm1(rel)).sum(-1) / L + N * TINY                                 # relative error of the sum (L >= 1)
        bound = -torch.log1p(-e_sum) + 2.0 ** -22 * L.log().abs() + EPS_ACC + U32 * ref.abs()
        return ref, bound

    # ---- att = exp(s - lse_i) and its error before / after the bf16 rounding --------------------------------------------------------------
    def att(self, lse):
        key = id(lse)
        if key not in self._att:
            l = lse.double()[..., None]
            d = self.s - l
            a = torch.exp(d)
            delta = self.es + U32 * torch.maximum(torch.maximum(self.s.abs(), l.abs().expand_as(d)), d.abs()) + EPS_ACC * d.abs()      # S - LSE, EXPF (argument)
            e_att = a * (torch.expm1(delta) + EPS_ACC) + TINY                                                                          # EXPF (instruction, flush)
            e_p = e_att + EPS_BF16 * (a + e_att)                                                                                       # ATT->BF16
            self._att = {key: (lse, a, e_att, e_p)}                                           # (one entry: the tests walk the ops lse by lse)
        return self._att[key][1:]

    @staticmethod
    def _product2(P, eP, V, Va, n_terms):
        """PRODUCT2: (P V, its error before the store); P, eP: (F, rows, streamed), V: (F, streamed, C)"""
        return P @ V, eP @ Va + n_terms * EPS_ACC * ((P.abs() + eP) @ Va)

    @staticmethod
    def _store(ref, pre):
        return ref, pre + EPS_BF16 * (ref.abs() + pre)

    @staticmethod
    def _rmw(out0, term, pre):
        """STORE of Y / DXQ / DXK: fl_bf16(fl32(out0 + term))"""
        ref = out0.double() + term
        pre = pre + U32 * (ref.abs() + pre)
        return ref, pre + EPS_BF16 * (ref.abs() + pre)

    def att_stored(self, lse):
        a, e_att, _ = self.att(lse)
        return self._store(a, e_att)

    def xr(self, lse):
        a, _, e_p = self.att(lse)
        return self._store(*self._product2(a.transpose(1, 2), e_p.transpose(1, 2), self.X, self.Xa, self.N))

    def y(self, lse, out0):
        """{"out": (ref, bound), "rowdot": (ref, bound)}"""
        a, _, e_p = self.att(lse)
        y, ey = self._product2(a, e_p, self.D, self.Da, self.N)
        rd = (self.X * y).sum(-1)
        erd = (self.Xa * ey).sum(-1) + self.C * EPS_ACC * (self.Xa * (y.abs() + ey)).sum(-1)   # ROWDOT
        return {"out": self._rmw(out0, y, ey), "rowdot": (rd, erd)}

    def _ds(self, a, e_a, rowdot):
        """DS: (dS, its error as the bf16 operand of the second product); a, e_a: att and its error as the factor of the product"""
        r = rowdot.double()[..., None]
        t = self.g - r
        et = self.eg + U32 * (self.g.abs() + r.abs())
        ds = a * t
        pre = e_a * t.abs() + (a + e_a) * et
        return ds, pre + (U32 + EPS_BF16) * (ds.abs() + pre) + TINY

    def dx(self, key, lse, rowdot, out0):
        a, _, e_p = self.att(lse)
        ds, eds = self._ds(a, e_p, rowdot)
        if key:
            ds, eds = ds.transpose(1, 2), eds.transpose(1, 2)
        return self._rmw(out0, *self._product2(ds, eds, self.X, self.Xa, self.N))

    def att_bwd(self, rowdot, att_in):
        a = att_in.double()
        r = rowdot.double()[..., None]
        t = self.g - r
        ref = a * t
        pre = a.abs() * (self.eg + U32 * (self.g.abs() + r.abs())) + U32 * ref.abs()
        return self._store(ref, pre)


class Operands:
    """Operands of every op for one (family, frames, N, C), as both test modules draw them: lse = fl32(fp64 lse) + a
    per-row offset from [-0.25, 0.25], rowdot drawn per row at the size of the true one, out prefilled with 0.05 randn."""

    def __init__(self, family, frames, N, C, device="cpu"):
        X, dxr = make_inputs(family, frames, N, C)
        self.X, self.dxr = X.to(device), dxr.to(device)
        self.ref = NxnRef(self.X, self.dxr)
        lse_true = self.ref.lse()[0]
        self.lse = (lse_true.float() + row_noise(frames, N, 0.25, 1).to(device)).contiguous()
        rd_true = self.ref.y(self.lse, torch.zeros_like(self.X))["rowdot"][0]
        self.rowdot = row_noise(frames, N, float(rd_true.std()), 2, uniform=False).float().to(device).contiguous()
        g = torch.Generator().manual_seed(5)
        self.out0 = (0.05 * torch.randn(frames, N, C, generator=g)).bfloat16().to(device)
        self.att_in = None

    def operands(self, op):
        kw = {}
        if op in ("ATT_FROM_LSE", "XR", "Y", "DXQ", "DXK"):
            kw["lse"] = self.lse
        if op in ("DXQ", "DXK", "ATT_BWD"):
            kw["rowdot"] = self.rowdot
        if op in ("Y", "DXQ", "DXK"):
            kw["out0"] = self.out0
        if op == "ATT_BWD":
            if self.att_in is None:
                self.att_in = self.ref.att_stored(self.lse)[0].bfloat16()
            kw["att_in"] = self.att_in
        return kw


def xrstats_ref(X, xr):
    """sxr of k_xrstats_v4 (bwd_kernels.hip:754): per token sum xr, sum xr^2, x . xr -- C fp32 terms each.  X, xr: (rows, C) -> (3, rows)"""
    X, R = X.double(), xr.double()
    C = X.shape[-1]
    ref = torch.stack([R.sum(-1), (R * R).sum(-1), (X * R).sum(-1)])
    mag = torch.stack([R.abs().sum(-1), (R * R).sum(-1), (X * R).abs().sum(-1)])
    return ref, C * EPS_ACC * mag


def check_op(op, got, ref, *, lse=None, rowdot=None, out0=None, att_in=None, name=""):
    """The outputs of one op (`got`: {"lse" / "out" / "rowdot": tensor}) against fp64 from exactly the operands it was given; ref: NxnRef.
    ATT's att is held against the lse the kernel itself stored (got["lse"]): that is the value its second sweep uses in every lane (:156-160).
    Returns the worst err / bound over all outputs."""
    w = []
    if op in ("STATS", "ATT"):
        w.append(check_bound(got["lse"], *ref.lse(), f"{name} {op} lse (frame, row)"))
        if op == "ATT":
            w.append(check_bound(got["out"], *ref.att_stored(got["lse"]), f"{name} ATT att (frame, row, key)"))
    elif op == "ATT_FROM_LSE":
        w.append(check_bound(got["out"], *ref.att_stored(lse), f"{name} ATT_FROM_LSE att (frame, row, key)"))
    elif op == "XR":
        w.append(check_bound(got["out"], *ref.xr(lse), f"{name} XR xr (frame, row, channel)"))
    elif op == "Y":
        r = ref.y(lse, out0)
        w.append(check_bound(got["out"], *r["out"], f"{name} Y out (frame, row, channel)"))
        w.append(check_bound(got["rowdot"], *r["rowdot"], f"{name} Y rowdot (frame, row)"))
    elif op in ("DXQ", "DXK"):
        w.append(check_bound(got["out"], *ref.dx(op == "DXK", lse, rowdot, out0), f"{name} {op} out (frame, row, channel)"))
    elif op == "ATT_BWD":
        w.append(check_bound(got["out"], *ref.att_bwd(rowdot, att_in), f"{name} ATT_BWD dS (frame, row, key)"))
    else:
        raise ValueError(op)
    return max(w)
