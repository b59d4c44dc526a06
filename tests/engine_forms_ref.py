"""fp64 references, element-wise bounds and the test cases for the forms of the tiled engine (csrc/gemm.hip, launch_gemm) that only
avmoe_gemm_form (include/avmoe.h, tests only) reaches on operands of the test's choosing: further K segments, the third batch level, kept
split-K slabs and the softmax epilogues (ROWSTATS + gemm_row_lse, EXP, MULSUB).  Same style as tests/stream_product_ref.py (the product part:
product_ref, product_bound, check_bound, check_untouched come from there) and tests/nxn_ref.py (the softmax terms: U32, TINY, EPS_ACC on the
argument and on the result of __expf, the bf16 store; make_inputs and row_noise draw the A = B = X families).

The cases live here because two modules walk them: tests/test_engine_forms_fp64_gpu.py runs the kernel on them, tests/test_engine_forms_checker.py
shows on the CPU that an honest emulation of the kernel's arithmetic stays inside these bounds on exactly these inputs and that each plausible
fault leaves them.  Nothing is fitted to a measured error.

Terms, each from the text of gemm.hip:

  PRODUCT   fp32 accumulation of all K segments into one accumulator (gemm_kernel: gemm_segment per segment on the same `acc`), then the
            epilogue's `rsv * D` and the accumulate add: k_terms = sum of K over the segments + 1 for the D term + 1 for the accumulate term,
            each EPS_ACC = 2^-23 of mag = |A| |B| + |rs D| + |C0|  (stream_product_ref.product_bound).  alpha is 1 or 0.5 here: exact.
            A bf16 store: EPS_BF16 |ref|.
  PLANES 2  f32s2 (lstore: hb = bf16(x), lb = bf16(x - hb); compute: lo x hi, hi x lo, hi x hi): EPS_PLANES = 2^-16 of mag, as in
            stream_product_ref: the dropped lo x lo, each lo <= 2^-8 of its value.  (With BOTH operands fp32 the second plane's own rounding,
            2^-17 per operand, can add another 2^-16 on a single product whose roundings all point one way; over a contraction they do not,
            and the term stays the one the streaming check uses.  The emulation of tests/test_engine_forms_checker.py keeps inside it.)
  PLANES 3  f32s3 (compute(), is_split branch): p0 = bf16(x), r1 = x - p0 (exact in fp32), p1 = bf16(r1), r2 = r1 - p1 (exact), p2 = bf16(r2).
            bf16 keeps 8 significant bits and rounds to nearest: for 2^e <= |x| < 2^(e+1), |r1| <= 2^(e-8), so |p1| <= 2^-8 |x|.  Unless r1 is
            that power of two (then r2 = 0) it lies in a binade <= e - 9, so |r2| <= 2^(e-17).  r2 is a multiple of the fp32 ulp 2^(e-23): at
            most 7 significant bits, so the third plane takes it whole, p2 = r2, |p2| <= 2^-17 |x|, and it leaves NOTHING of x:
            x = p0 + p1 + p2 exactly.  Of the nine plane products the kernel keeps the six of order <= 2 (p2 q0, p1 q1, p0 q2, p1 q0, p0 q1,
            p0 q0) and drops p1 q2, p2 q1 (2^-8 * 2^-17 = 2^-25 |x y| each) and p2 q2 (2^-34): EPS_PLANES3 = 2^-24 (1 + 2^-9) = 5.97e-8 of mag.
            This DISAGREES with the 5.8e-9 quoted in csrc/gemm.h and include/avmoe.h: that figure is a measured typical error per product, not
            a bound; random operands in [1, 2) reach 4.5e-8 (test_three_plane_term_is_derived_not_quoted).
  EXACT     v_mfma_f32_16x16x4_f32 multiplies fp32 by fp32: no operand term.
  ROWSTATS  per row and 128-column tile: mx = max of the tile's fl32 scores (exact on those), sum = __expf(v - mx) over the thread's 64 columns,
            then one shuffle add of the two threads of the row: 65 additions of non-negative terms.  The sum is checked against fp64
            sum_j exp(s_j - mx) with the kernel's OWN stored mx, so the pair stands for the tile's sum_j exp(s_j) whatever mx it chose; per term
            the argument carries the score's error e_s, the subtraction (U32 at max(|s|, |mx|, |s - mx|)) and __expf's argument scaling
            (EPS_ACC |s - mx|), the result EPS_ACC and the flush TINY -- the S - LSE and EXPF terms of nxn_ref.  The max itself is held to
            max_j e_s of its tile.
  ROW_LSE   kk_row_lse: mx = max_t mx_t; per tile one subtraction (U32 |d_t|), one __expf (EPS_ACC |d_t| on the argument, EPS_ACC on the result,
            a flushed result costs sum_t * TINY), one product (U32), `tiles` additions (EPS_ACC each); one __logf (2^-22 |log| and never better
            than EPS_ACC, as nxn_ref's LSE term) and the final add (U32 |lse|).
  EXP       v = alpha * acc, __expf(v - lse): nxn_ref's S - LSE / EXPF terms; the store in the operand type (bf16: EPS_BF16).
  MULSUB    D * (v - rowdot): the score's error, one subtraction (U32 at |v| + |rowdot|), one product (U32), the store; nxn_ref's att_bwd.

Works on CPU and GPU tensors alike."""
import torch

from tests.nxn_ref import TINY, U32, make_inputs, row_noise
from tests.stream_product_ref import (EPS_ACC, EPS_BF16, EPS_PLANES, ProductMismatch, check_bound, check_untouched,  # noqa: F401  (re-exported)
                                      product_bound, product_ref)

EPS_PLANES3 = 2.0 ** -24 * (1 + 2.0 ** -9)
GEMM_H_QUOTED_PLANES3 = 5.8e-9           # csrc/gemm.h; a typical error, NOT used in any bound (module docstring)
KINDS = {"bf16": (1, 0, 0.0), "f32": (0, 0, 0.0), "f32s3": (0, 1, EPS_PLANES3), "f32s2": (0, 2, EPS_PLANES)}   # kind -> (dtype, fp32_planes, operand term)
TILE = 128                                # column tile of the softmax epilogues


def tdtype(kind):
    return torch.bfloat16 if kind == "bf16" else torch.float32


def _draw(g, shape, scale, kind):
    return (scale * torch.randn(*shape, generator=g)).to(tdtype(kind))


def form_bound(ref, mag, mag_prod, *, kind, out_bf16, k_terms):
    return product_bound(ref, mag, out_bf16=out_bf16, k_terms=k_terms) + KINDS[kind][2] * mag_prod


# ---- K segments ------------------------------------------------------------------------------------------------------------------------------
SEG_K = (40, 34, 65, 33)                  # every segment has a K tail (of 32-, 16- and 8-element steps)
SEG_SCALE = (0.5, 0.7, 0.4, 0.6)          # each segment at a scale of its own, all of one order: none hides under another's rounding
SEG_FORMS = (("KM", 2), ("MM", 2), ("KM", 3), ("KM", 4))      # (layouts of the first segment: A / B, segments)


def seg_layouts(first, nseg):
    """[(A MN-major, B MN-major)] per segment: what launch_layout has instances for"""
    return [(first == "MM", True), (False, True), (True, True), (False, True)][:nseg]


class SegCase:
    """nb1 = 3 frames, nb2 = 2 groups; A_i (3, 2 or 1, M, K_i) -- shared by the groups from the third segment on --, B_i (3, 2, K_i, N),
    row_scale (3, 2, M), D (3, 2, M, N) in the operand type, C0 (3, 2, M, N) in the output type.  alpha = 0.5."""
    nb1, nb2, alpha = 3, 2, 0.5

    def __init__(self, kind, first, nseg, *, big=False, out_bf16=False, acc=False, with_d=False, device="cpu"):
        self.kind, self.first, self.nseg, self.out_bf16, self.acc, self.with_d = kind, first, nseg, out_bf16, acc, with_d
        self.M, self.N = (150, 136) if big else (70, 72)
        g = torch.Generator().manual_seed(4000 + 100 * nseg + (first == "MM") + 10 * list(KINDS).index(kind) + 1000 * big)
        self.A = [_draw(g, (self.nb1, 1 if i >= 2 else self.nb2, self.M, SEG_K[i]), SEG_SCALE[i], kind).to(device) for i in range(nseg)]
        self.B = [_draw(g, (self.nb1, self.nb2, SEG_K[i], self.N), SEG_SCALE[i], kind).to(device) for i in range(nseg)]
        self.rs = (1.0 + 0.5 * torch.randn(self.nb1, self.nb2, self.M, generator=g)).to(device)
        self.D = _draw(g, (self.nb1, self.nb2, self.M, self.N), 0.8, kind).to(device)
        self.C0 = (0.9 * torch.randn(self.nb1, self.nb2, self.M, self.N, generator=g)).to(torch.bfloat16 if out_bf16 else torch.float32).to(device)
        self.name = f"segments {kind} {first}x{nseg} M{self.M} N{self.N} {'bf16' if out_bf16 else 'f32'}-out{' +D' if with_d else ''}{' +C' if acc else ''}"

    def ref(self):
        full = (self.nb1, self.nb2, self.M)
        Ac = torch.cat([a.double().expand(*full, a.shape[-1]) for a in self.A], -1) * self.alpha
        Bc = torch.cat([b.double() for b in self.B], -2)
        ref, mag_prod = product_ref(Ac, Bc)
        mag = mag_prod
        if self.with_d:
            t = self.rs.double()[..., None] * self.D.double()
            ref, mag = ref + t, mag + t.abs()
        if self.acc:
            ref, mag = ref + self.C0.double(), mag + self.C0.double().abs()
        k_terms = sum(SEG_K[:self.nseg]) + int(self.with_d) + int(self.acc)
        return ref, form_bound(ref, mag, mag_prod, kind=self.kind, out_bf16=self.out_bf16, k_terms=k_terms)


def seg_cases(device="cpu", only_kind=None):
    """Every K-segment case of the GPU test: (tile, SegCase).  Types x forms (the exact fp32 pipe has two segments only) x tiles 32 / 64 / 128
    forced and auto; fp32 / bf16 output, accumulate and row_scale * D are walked over them so that each value meets each form, tile and type."""
    out = []
    for ki, kind in enumerate(KINDS):
        if only_kind and kind != only_kind:
            continue
        for fi, (first, nseg) in enumerate(SEG_FORMS):
            if kind == "f32" and nseg > 2:
                continue
            for ti, tile in enumerate((32, 64, 128, 0)):
                out.append((tile, SegCase(kind, first, nseg, big=tile == 128, out_bf16=bool((fi + ti) & 1), acc=bool(((fi + ti) >> 1) & 1),
                                          with_d=bool((ti + fi // 2 + ki) & 1), device=device)))
    return out


# ---- third batch level, kept slabs -----------------------------------------------------------------------------------------------------------
class Nb3Case:
    """the dTW pattern: both operands MN-major, batch (nb1, nb3, nb2) = (3, 2, 2), M = 32, N = 48, K = 70; A (3, 2, 2, M, K), B (3, 2, 2, K, N)"""
    nb1, nb3, nb2, M, N, K = 3, 2, 2, 32, 48, 70

    def __init__(self, kind, out_bf16, device="cpu"):
        self.kind, self.out_bf16 = kind, out_bf16
        g = torch.Generator().manual_seed(5000 + list(KINDS).index(kind))
        self.A = _draw(g, (self.nb1, self.nb3, self.nb2, self.M, self.K), 0.5, kind).to(device)
        self.B = _draw(g, (self.nb1, self.nb3, self.nb2, self.K, self.N), 0.5, kind).to(device)
        self.name = f"nb3 {kind} {'bf16' if out_bf16 else 'f32'}-out"

    def ref(self):
        ref, mag = product_ref(self.A, self.B)
        return ref, form_bound(ref, mag, mag, kind=self.kind, out_bf16=self.out_bf16, k_terms=self.K)


class SlabCase:
    """kept slabs: ksplit = 4, batch 2 x 2, M = 70, N = 40, K = 700; A K-major (2, 2, M, K), B MN-major (2, 2, K, N); the slabs are fp32 and alpha
    is not applied to them"""
    nb1, nb2, M, N, K, ksplit = 2, 2, 70, 40, 700, 4

    def __init__(self, kind, device="cpu"):
        self.kind = kind
        g = torch.Generator().manual_seed(6000 + list(KINDS).index(kind))
        self.A = _draw(g, (self.nb1, self.nb2, self.M, self.K), 0.5, kind).to(device)
        self.B = _draw(g, (self.nb1, self.nb2, self.K, self.N), 0.5, kind).to(device)
        self.name = f"kept slabs {kind}"

    def ref(self):
        ref, mag = product_ref(self.A, self.B)
        return ref, form_bound(ref, mag, mag, kind=self.kind, out_bf16=False, k_terms=self.K)      # (the slabs are added in fp64 by the test)

    def kper(self):
        """K entries per slab, as launch_gemm cuts them: round_up(ceil(K / ksplit), 256 bytes of K)"""
        bk = 128 if self.kind == "bf16" else 64
        return -(-(-(-self.K // self.ksplit)) // bk) * bk


# ---- softmax epilogues -----------------------------------------------------------------------------------------------------------------------
SOFTMAX_KINDS = ("bf16", "f32", "f32s3")
SOFTMAX_FREE = ((3, 150, 200, 96), (2, 128, 130, 100), (1, 40, 64, 192))      # (frames, M, N, K), free rectangular A, B
SOFTMAX_X = (2, 256, 384, 96)                                                  # A = B = X (A: the first 256 tokens)
SOFTMAX_FAMILIES = ("flat", "late_max", "early_max", "frame_scales")


def softmax_ids():
    return [("free", s) for s in SOFTMAX_FREE] + [(f, SOFTMAX_X) for f in SOFTMAX_FAMILIES]


class SoftmaxCase:
    """One (family, shape, type): A (F, M, K), B (F, N, K) K-major, the drawn lse offsets, rowdot and D; refs per alpha (1 and 0.5)"""

    def __init__(self, kind, family, shape, device="cpu"):
        self.kind, self.family, self.shape = kind, family, shape
        F, M, N, K = shape
        g = torch.Generator().manual_seed(7000 + M + K + list(KINDS).index(kind))
        if family == "free":
            A, B = 0.3 * torch.randn(F, M, K, generator=g), 0.3 * torch.randn(F, N, K, generator=g)
            self.shared = False
        else:
            X, dxr = make_inputs(family, F, N, K)
            B = X.float() + (0.0 if kind == "bf16" else 2.0 ** -6) * dxr.float()       # fp32: mantissa bits below the first bf16 plane
            A = B[:, :M]
            self.shared = True
        self.A, self.B = A.to(tdtype(kind)).to(device).contiguous(), B.to(tdtype(kind)).to(device).contiguous()
        self.D = (0.1 * torch.randn(F, M, N, generator=g).abs()).to(tdtype(kind)).to(device)
        self.noise = row_noise(F, M, 0.25, 1).to(device)
        self.rd_unit = row_noise(F, M, 1.0, 2, uniform=False).to(device)
        self.tiles = -(-N // TILE)
        self.name = f"softmax {kind} {family} {F}x{M}x{N}x{K}"
        self._r = {}

    def at(self, alpha):
        if alpha not in self._r:
            self._r[alpha] = SoftmaxRef(self, alpha)
        return self._r[alpha]


class SoftmaxRef:
    def __init__(self, c, alpha):
        A, B = c.A.double(), c.B.double()
        K = A.shape[-1]
        self.c, self.alpha = c, alpha
        self.out_bf16 = c.kind == "bf16"
        self.s = alpha * (A @ B.transpose(1, 2))
        self.es = (K * EPS_ACC + KINDS[c.kind][2]) * alpha * (A.abs() @ B.abs().transpose(1, 2))
        M = self.s.max(-1, keepdim=True).values
        self.lse_true = M[..., 0] + torch.exp(self.s - M).sum(-1).log()
        self.lse_in = (self.lse_true.float() + c.noise).contiguous()                           # EXP's operand: per-row offsets
        self.rowdot = (c.rd_unit * float(self.s.std())).float().contiguous()                    # MULSUB's operand: drawn per row

    def _exp_terms(self, sub):
        """a = exp(s - sub) and its error before a store (sub: (F, M) as the kernel read it)"""
        l = sub.double()[..., None]
        d = self.s - l
        a = torch.exp(d)
        delta = self.es + U32 * torch.maximum(torch.maximum(self.s.abs(), l.abs().expand_as(d)), d.abs()) + EPS_ACC * d.abs()
        return a, a * (torch.expm1(delta) + EPS_ACC) + TINY

    def _store(self, ref, pre):
        return (ref, pre + EPS_BF16 * (ref.abs() + pre)) if self.out_bf16 else (ref, pre)

    def parts(self, mx_got):
        """ROWSTATS: ((max ref, bound), (sum ref, bound)), each (F, M, tiles); the sums against the kernel's own maxima mx_got (F, M, tiles)"""
        N = self.s.shape[-1]
        mr, mb, sr, sb = [], [], [], []
        for t in range(self.c.tiles):
            sl = slice(t * TILE, min(N, (t + 1) * TILE))
            mr.append(self.s[..., sl].max(-1).values)
            mb.append(self.es[..., sl].max(-1).values)
            sub = SoftmaxRef.__new__(SoftmaxRef)
            sub.s, sub.es = self.s[..., sl], self.es[..., sl]
            a, e = sub._exp_terms(mx_got[..., t])
            sr.append(a.sum(-1))
            sb.append(e.sum(-1) + 65 * EPS_ACC * (a + e).sum(-1))
        st = lambda v: torch.stack(v, -1)
        return (st(mr), st(mb)), (st(sr), st(sb))

    def exp(self, lse):
        return self._store(*self._exp_terms(lse))

    def mulsub(self, sub, D):
        r = sub.double()[..., None]
        Dd = D.double()
        ref = Dd * (self.s - r)
        pre = Dd.abs() * (self.es + U32 * (self.s.abs() + r.abs())) + U32 * ref.abs() + TINY
        return self._store(ref, pre)


def row_lse_ref(parts):
    """kk_row_lse on GIVEN parts (..., tiles, 2) -> (ref, bound) (...)"""
    p = parts.double()
    mx_t, sm_t = p[..., 0], p[..., 1]
    tiles = p.shape[-2]
    M = mx_t.max(-1, keepdim=True).values
    d = mx_t - M
    w = sm_t * torch.exp(d)
    L = w.sum(-1)
    ref = M[..., 0] + L.log()
    rel = (U32 + EPS_ACC) * d.abs() + EPS_ACC + U32 + tiles * EPS_ACC
    e_sum = ((w * torch.expm1(rel)).sum(-1) + (sm_t + 1).sum(-1) * TINY) / L
    return ref, -torch.log1p(-e_sum) + 2.0 ** -22 * L.log().abs() + EPS_ACC + U32 * ref.abs()


def lse_from_scores_bound(parts, sum_ref, sum_bound):
    """lse of the kernel's own parts against the fp64 lse of the SCORES: row_lse_ref's bound plus what the parts themselves may be off by --
    each pair stands for its tile's sum_j exp(s_j) up to the relative error of its sum (the max cancels: `parts`' docstring)"""
    rho = (sum_bound / sum_ref).max(-1).values
    return row_lse_ref(parts)[1] + -torch.log1p(-rho)


LSE_ALONE = (("one tile", 257, 1), ("a tile 150 below the maximum", 257, 3), ("one row", 1, 2), ("grid-stride loop", 1048579, 2))


def lse_alone_parts(what, rows, tiles, device="cpu"):
    g = torch.Generator().manual_seed(rows + tiles)
    p = torch.stack([3.0 * torch.randn(rows, tiles, generator=g), 1.0 + 127.0 * torch.rand(rows, tiles, generator=g)], -1)
    if "150" in what:
        p[:, 1, 0] = p[:, :, 0].max(-1).values - 150.0          # its term underflows: exp(-150) < 2^-126
    return p.float().to(device).contiguous()
