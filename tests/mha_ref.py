"""fp64 references and element-wise bounds for the links of the frame-attention ("v1") expert chain -- mha_frames_forward / mha_frames_backward
(csrc/mha_frames.hip) and the x + xr glue around them that the v1 experts share with the AVVP ones (k_xrstats, ZR = xr Wt^T, dxr = dZR Wt +
rs xr, k_nxn_axpy) -- each from its operands EXACTLY AS STORED in the workspace (bf16 and fp32 are exact in fp64: nothing upstream of a link
adds error).  Same method as tests/hop1_ref.py, whose Dims, check_exact / check_zero, dot_bound and softmax terms are reused; the product
terms come from tests/stream_product_ref.py, the softmax terms from tests/nxn_ref.py, the plane terms from tests/engine_forms_ref.py.  Nothing
is fitted to a measured error and no constant is new.

A link is a function  link(d, B, j) -> worst err / bound  (raises ProductMismatch, an AssertionError, naming the element).  d: Dims, B: {buffer:
tensor in the buffer's own dtype and shape (Dims.shapes)} plus "X", "keep" ({expert prefix: (N * H, S, S)} or None), "scores" (mSc as it stood behind the forward), "grads", "dX" and the
parameters under their state-dict names, j: the xr slot.  tests/test_mha_chain_fp64_gpu.py hands device views, tests/test_mha_checker.py an
emulation on the CPU.

Terms (per element), each named after the line that causes it (mha_frames.hip unless another file is named):

  CAST      k_cast (:98-99): stT<T>, ONE round-to-nearest-even rounding; held as equality.
  PRODUCT   a product through launch_gemm -- an instance of the tiled engine or, for the flat (NT-row) products of a bf16 site with NT >= 256,
            the B-stationary streaming kernel (stage_instances below says which; fp32 accumulators either way, K chunks / split K only
            reorder): k * EPS_ACC * (|A| |B|), k the contraction
            length -- C for X Win^T (:102), O Wout^T (:128), dxr Wout (:170); dh for q k^T (:109) and dO v^T (:175); S for Pd v (:122),
            Pd^T dO (:181), dS k (:192), dS^T q (:198); NT for dWout (:165) and dWin (:205); 3 C for dQKV Win (:210).  alpha (:110, :193, :199)
            is one fp32 product of the accumulator: U32 |ref|.  A store in T: EPS_BF16 |ref| (bf16), nothing (fp32).
  PLANES    fp32 sites.  The products of mha_frames.hip leave split3 at 0 (:97, :156): the exact fp32 matrix instruction, NO operand term.  The
            glue's products are built by moe_forward.cpp:54 / moe_backward.cpp:55: three planes (EPS_PLANES3 of |A| |B|) for ZR and dxr; the
            site's dX product is a two-plane leaf (moe_backward.cpp:156, EPS_PLANES).
  RMW       a second kernel that reads the stored T value and stores again: km_add_bias (:32, one fp32 add), km_finish (:59, two),
            kk_nxn_axpy (bwd_kernels.hip:838, :841: a product and two adds each), the accumulating epilogue of dX += dQKV Win (:211).  The value
            read carries the first store's rounding (it is not itself stored any more, so it is an error term, not an operand); r fp32
            operations cost r * U32 of the sum of the |terms|; then the store.
  SOFTMAX   k_softmax_rows at n = S, ld = Sp: Sp % 8 == 0 and S <= 1024 select kk_softmax_rows_reg<T, 4> at EVERY legal v1 site
            (fwd_kernels.hip:671-674; "reg4", also at S = 70 > 64: a lane holds four 4-vectors, a row up to 1024 entries).  hop1_ref.softmax_ref:
            `p - mx` U32 on the argument, __expf EPS_ACC |x| on the argument + EPS_ACC + TINY, the sum in double and 1 / sum rounded once, e * inv,
            the store.  Where the scores are no longer stored (slot 0 of a two-slot site: mSc is scratch) the argument also carries the
            product's own bound es = dh EPS_ACC alpha |q| |k| + U32 |s|.
  KEEP      km_keep (:42): one fp32 product, the store.  km_keep_bwd (:50): one fp32 product in place.
  SOFTMAX'  k_softmax_rows_bwd, "reg4" (bwd_kernels.hip:444-446): hop1_ref.softmax_bwd_ref -- DOT with 16 additions per lane + 7.
  XRSTATS   kk_xrstats_v4 (bwd_kernels.hip:800-812): 16 lanes per row; per 64-column chunk a lane forms four products (one rounding), two
            pair sums and their sum (two on the path) and adds it to its accumulator (one): 4 roundings per chunk on any path, then 4 shuffle
            steps: (4 ceil(C / 64) + 4) * EPS_ACC * sum |terms|.  kk_xrstats (C % 4 != 0) cannot be reached: make_plan asks (C / groups) % 8 == 0
            of EVERY site (moe_plan.cpp:54), AVVP included.
  COLSUM    km_colsum_part + k_colsum_f32 (:64-83, fwd_kernels.hip:38-61): chunks = clamp(rows / 64, 1, 256) row chunks of rpc = ceil(rows /
            chunks) rows; a wave adds every fourth row of its chunk (ceil(rpc / 4) additions), the four waves fold in two steps; k_colsum_f32
            adds the chunks in NS = 4 (chunks < 128) or 64 streams; a stream has n = ceil(chunks / NS) rows, its accumulator a0 takes one per
            round of four (n // 4) and every row of the tail loop (n % 4: fwd_kernels.hip:51); the streams fold in double and round once:
            (ceil(rpc / 4) + 2 + n // 4 + n % 4 + 1) * EPS_ACC * sum |x| -- not rows * EPS_ACC.

What is NOT held here: slot 0's backward scratch at two-slot sites (the scratch holds the last slot); dZR / dsr, which enter as stored operands
(the XR arm of pre_small / pre_small_bwd writes them); the N x N kernels of the AVVP site (tests/test_nxn_strips_fp64_gpu.py); the glue's
share of the down projection's gradient, dWt_e += dZR_e^T xr_e (moe_backward.cpp:266): it accumulates into a dWt whose earlier value is not
kept, so it has no stored operands to be held against (its kernel instance is asserted, stage_instances).
"""
import math

import torch

from oracle import avmoe_oracle as O
from tests import hop1_ref as H
from tests.engine_forms_ref import EPS_PLANES3
from tests.hop1_ref import _ru, _store, castT, check_exact, check_zero, dot_bound  # noqa: F401
from tests.nxn_ref import TINY, U32
from tests.stream_product_ref import EPS_ACC, EPS_BF16, EPS_PLANES, ProductMismatch, check_bound, product_ref  # noqa: F401

HEADS = 4
FAMILIES = ("default", "flat", "peaked")
# input families (chosen on the CPU from the fp64 scores alone, tests/test_mha_checker.py::test_families_hold_on_the_fp64_scores):
#   flat    the q / k rows of in_proj_weight and in_proj_bias times FLAT_SCALE: the scores shrink by its square
#   peaked  the q / k rows of in_proj_weight times PEAK_SCALE, the q bias replaced by PEAK_BIAS * (its direction), and for every token one frame
#           pushed along Wk^T bq by PEAK_PUSH: that frame's key meets the common part of every query, so its column holds the row maxima --
#           frame 0 for n % 3 == 0, frame S - 1 for n % 3 == 1, the first frame of the last 8-group for n % 3 == 2
FLAT_SCALE, PEAK_SCALE, PEAK_BIAS, PEAK_PUSH = 0.25, 4.0, 3.0, 3.0


class Dims(H.Dims):
    """hop1_ref.Dims + the widths of the frame attention (moe_plan.cpp:66-80) and the buffers of moe_plan.h:129-151"""

    def __init__(self, cfg, S, bf16, nbytes):
        self.v1 = cfg.self_attn == "v1"
        self.H, self.dh, self.Sp = HEADS, cfg.Cx // HEADS, _ru(S, 8)
        self.nxr = cfg.E_s if self.v1 else 1
        self.alpha = float(torch.tensor(1.0) / torch.sqrt(torch.tensor(float(self.dh))))        # 1.f / std::sqrt((float)dh) (:110, :155)
        super().__init__(cfg, S, bf16, nbytes)
        self.KLp = _ru(self.KLT, 8)
        self.slots = [(e - cfg.E_m if self.v1 else 0, e, cfg.expert_prefixes()[e]) for e in range(cfg.E_m, cfg.E)]      # (slot, expert, prefix)

    def shapes(self):
        S, N, C, Hh, Sp, n = self.S, self.N, self.C, self.H, self.Sp, self.nxr
        sh = dict(super().shapes())
        sh.update({"xr": ("T", (n, S, N, C)), "sxr": ("f", (n, 3, self.NT)), "ZR": ("f", (S, N, self.g, self.E, self.dgp)),
                   "dZR": ("T", (S, N, self.g, self.E, self.dgp)), "dsr": ("f", (n, 3, self.NT)), "dxr": ("T", (S, N, C)),
                   "dL2x": ("T", (S, N, _ru(self.KLT, 8))), "rs2x": ("f", (S, N))})
        if self.v1:
            sh.update({"mWin": ("T", (n, 3 * C, C)), "mWout": ("T", (n, C, C)), "mQKV": ("T", (n, S, N, 3 * C)), "mP": ("T", (n, N, Hh, S, Sp)),
                       "mPd": ("T", (n, N, Hh, S, Sp)), "mO": ("T", (n, S, N, C)), "mSc": ("f", (N, Hh, S, Sp)), "mdO": ("T", (S, N, C)),
                       "mdS": ("T", (N, Hh, S, Sp)), "mdQKV": ("T", (S, N, 3 * C))})
        return sh


# ---- helpers -----------------------------------------------------------------------------------------------------------------------------
def _heads(d, t):
    """(S, N, C) -> (N, H, S, dh): token n = batch level 1, head h = level 2, frame s = row (site_views.h: per_token, groups)"""
    return t.reshape(d.S, d.N, d.H, d.dh).permute(1, 2, 0, 3)


def qkv(d, t):
    """[s][n][q | k | v] -> three (N, H, S, dh)"""
    return tuple(_heads(d, t[..., i * d.C:(i + 1) * d.C]) for i in range(3))


def keep_of(d, B, pre):
    k = (B.get("keep") or {}).get(pre)
    return None if k is None else k.reshape(d.N, d.H, d.S, d.S).double()


def prod(d, got, A, Bm, k, name, out_T, extra=None, alpha=1.0, planes=0.0):
    """PRODUCT: got == alpha * (A @ Bm) (+ extra, an epilogue term: one more accumulated term)"""
    ref, mag = product_ref(A, Bm)
    ref, mag = alpha * ref, alpha * mag
    magp = mag
    if extra is not None:
        ref, mag = ref + extra.double(), mag + extra.double().abs()
        k = k + 1
    pre = k * EPS_ACC * mag + planes * magp + (U32 * ref.abs() if alpha != 1.0 else 0.0)
    return check_bound(got, ref, _store(d, ref, pre, out_T), name)


def rmw_bound(d, ref, first_ref, first_pre, terms_mag, ops):
    """RMW: the bound of T(fl32(stored + terms)) where `stored` = T(first_ref +- first_pre) is not an operand any more"""
    e1 = _store(d, first_ref, first_pre, True)
    pre = e1 + ops * U32 * (first_ref.abs() + e1 + terms_mag)
    return _store(d, ref, pre, True)


def softmax_ref(d, s, es=None):
    """hop1_ref.softmax_ref ("reg4") with an error es of the argument for scores that are no longer stored"""
    if es is None:
        return H.softmax_ref(d, s, "reg4")
    p = s.double()
    mx = p.max(-1, keepdim=True).values
    x = p - mx
    e = torch.exp(x)
    delta = 2 * es.max(-1, keepdim=True).values + es + U32 * (torch.maximum(torch.maximum(p.abs(), mx.abs().expand_as(p)), x.abs()) + 2 * es) + EPS_ACC * (x.abs() + 2 * es)
    e_e = e * (torch.expm1(delta) + EPS_ACC) + TINY
    sm = e.sum(-1, keepdim=True)
    e_sum = e_e.sum(-1, keepdim=True) / sm + U32
    ref = e / sm
    pre = e_e / sm + ref * (e_sum / (1 - e_sum)) + U32 * ref
    return ref, _store(d, ref, pre, True)


def colsum_bound(rows, mag):
    """COLSUM"""
    chunks = max(1, min(256, rows // 64))
    rpc = -(-rows // chunks)
    n = -(-chunks // (64 if chunks >= 128 else 4))
    return (-(-rpc // 4) + 2 + n // 4 + n % 4 + 1) * EPS_ACC * mag


def _poison(t):
    """the workspace poison (0xFF bytes) is intact in every element"""
    iv = t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)
    return bool((iv == -1).all())


def poison(shape, dtype):
    """a buffer as the tests' workspaces arrive: every byte 0xFF (a NaN in fp32 and in bf16)"""
    return torch.full(tuple(shape), -1, dtype=torch.int32 if dtype == torch.float32 else torch.int16).view(dtype)


def check_poison(t, name, zeroed=False):
    """padding no kernel writes: the NaN poison of the tests' workspaces (or the zero of AVMOE_TEST_ZERO_WS)"""
    if t.numel() == 0:
        return 0.0
    if zeroed:
        return check_zero(t, name)
    if not _poison(t):
        raise ProductMismatch(f"{name}: {int((~torch.isnan(t.float())).sum())} of {t.numel()} elements that no kernel writes lost the workspace poison")
    return 0.0


def _par(B, pre, k):
    return B[f"{pre}.self_attention.{k}"].float()


# ---- forward links, per slot (mha_frames_forward, then moe_forward.cpp:195-200) ------------------------------------------------------------------
def link_cast(d, B, j):
    """mWin / mWout: CAST of in_proj_weight / out_proj.weight (:98-99)"""
    pre = d.slots[j][2]
    return max(check_exact(B["mWin"][j], castT(d, _par(B, pre, "in_proj_weight")), f"slot {j} mWin = T(in_proj_weight) (row, c)"),
               check_exact(B["mWout"][j], castT(d, _par(B, pre, "out_proj.weight")), f"slot {j} mWout = T(out_proj.weight) (row, c)"))


def link_qkv(d, B, j):
    """mQKV = T(T(X Win^T) + bin[i % 3C]) (:102, km_add_bias :32): PRODUCT over C, then RMW with one add"""
    pre = d.slots[j][2]
    p, mag = product_ref(B["X"].reshape(d.NT, d.C), B["mWin"][j].t())
    b = _par(B, pre, "in_proj_bias").double()[None]
    ref = p + b
    return check_bound(B["mQKV"][j].reshape(d.NT, 3 * d.C), ref, rmw_bound(d, ref, p, d.C * EPS_ACC * mag, b.abs(), 1), f"slot {j} mQKV = X Win^T + bin (token, column)")


def scores_ref(d, B, j):
    q, k, _ = qkv(d, B["mQKV"][j])
    ref, mag = product_ref(q, k.transpose(-1, -2))
    ref, mag = d.alpha * ref, d.alpha * mag
    return ref, d.dh * EPS_ACC * mag + U32 * ref.abs()


def link_scores(d, B, j, zeroed=False):
    """mSc = alpha q k^T per (token, head) (:109-110), fp32, read behind the forward; columns S .. Sp: the product stores S columns of the Sp
    wide row, the padding is untouched (the workspace poison)"""
    ref, bnd = scores_ref(d, B, j)
    return max(check_bound(B["scores"][..., :d.S], ref, bnd, f"slot {j} mSc = q k^T / sqrt(dh) (token, head, s, s')"),
               check_poison(B["scores"][..., d.S:], "mSc columns S .. Sp", zeroed))


def link_softmax(d, B, j, stored_scores=True):
    """mP = softmax_rows(mSc) (:113): every row per element, its sum, columns S .. Sp exactly 0 (training and eval alike)"""
    S = d.S
    if stored_scores:
        ref, bnd = softmax_ref(d, B["scores"][..., :S])
    else:
        ref, bnd = softmax_ref(d, *scores_ref(d, B, j))
    P = B["mP"][j]
    return max(check_bound(P[..., :S], ref, bnd, f"slot {j} mP = softmax(mSc) [reg4] (token, head, s, s')"),
               check_bound(P[..., :S].double().sum(-1), torch.ones_like(ref[..., 0]), bnd.sum(-1), f"slot {j} mP row sums (token, head, s)"),
               check_zero(P[..., S:], f"slot {j} mP columns S .. Sp (token, head, s, s' - S)") if d.Sp > S else 0.0)


def link_keep(d, B, j, zeroed=False):
    """mPd = T(P * keep[n * H + h][s][s']) at stride S (km_keep :36-43), padding exactly 0; without sa_keep mPd is untouched"""
    keep = keep_of(d, B, d.slots[j][2])
    if keep is None:
        return check_poison(B["mPd"][j], f"slot {j} mPd without sa_keep", zeroed)
    ref = B["mP"][j][..., :d.S].double() * keep
    Pd = B["mPd"][j]
    return max(check_bound(Pd[..., :d.S], ref, _store(d, ref, U32 * ref.abs(), True), f"slot {j} mPd = P * keep (token, head, s, s')"),
               check_zero(Pd[..., d.S:], f"slot {j} mPd columns S .. Sp (token, head, s, s' - S)") if d.Sp > d.S else 0.0)


def _pd(d, B, j):
    return (B["mP"] if keep_of(d, B, d.slots[j][2]) is None else B["mPd"])[j][..., :d.S]


def link_o(d, B, j):
    """mO = Pd v per (token, head), heads concatenated in head order (:122): PRODUCT over S; P where there is no keep"""
    _, _, v = qkv(d, B["mQKV"][j])
    return prod(d, _heads(d, B["mO"][j]), _pd(d, B, j), v, d.S, f"slot {j} mO = Pd v (token, head, s, dh)", True)


def link_xr(d, B, j):
    """xr = T(T(O Wout^T) + bout - X) (:128, km_finish :59): PRODUCT over C, then RMW with two adds"""
    pre = d.slots[j][2]
    p, mag = product_ref(B["mO"][j].reshape(d.NT, d.C), B["mWout"][j].t())
    b, X = _par(B, pre, "out_proj.bias").double()[None], B["X"].reshape(d.NT, d.C).double()
    ref = p + b - X
    return check_bound(B["xr"][j].reshape(d.NT, d.C), ref, rmw_bound(d, ref, p, d.C * EPS_ACC * mag, b.abs() + X.abs(), 2), f"slot {j} xr = O Wout^T + bout - X (token, c)")


def link_sxr(d, B, j):
    """sxr = (sum xr, sum xr^2, x . xr) per token (kk_xrstats_v4): XRSTATS"""
    X, R = B["X"].reshape(d.NT, d.C).double(), B["xr"][j].reshape(d.NT, d.C).double()
    ref = torch.stack([R.sum(-1), (R * R).sum(-1), (X * R).sum(-1)])
    mag = torch.stack([R.abs().sum(-1), (R * R).sum(-1), (X * R).abs().sum(-1)])
    return check_bound(B["sxr"][j], ref, (4 * -(-d.C // 64) + 4) * EPS_ACC * mag, f"slot {j} sxr (sum, token)")


def _wt(d, B, e=None):
    """Wt (g, E * dgp, Cg); e: the rows of one expert"""
    Wt = B["Wt"]
    return Wt if e is None else Wt[:, e * d.dgp:(e + 1) * d.dgp]


def link_zr(d, B, j):
    """v1: ZR[:, e] = xr_slot Wt_e^T per group (moe_forward.cpp:196-200), fp32, PRODUCT over Cg (+ PLANES 3 at fp32 sites).  AVVP: the whole
    ZR = xr Wt^T (:236)"""
    planes = 0.0 if d.bf16 else EPS_PLANES3
    xr = B["xr"][j].reshape(d.NT, d.g, d.Cg).permute(1, 0, 2)
    ZR = B["ZR"].reshape(d.NT, d.g, d.E, d.dgp).permute(1, 0, 2, 3)
    if not d.v1:
        return prod(d, ZR.reshape(d.g, d.NT, d.E * d.dgp), xr, _wt(d, B).transpose(1, 2), d.Cg, "ZR = xr Wt^T (group, token, column)", False, planes=planes)
    e = d.slots[j][1]
    return prod(d, ZR[:, :, e], xr, _wt(d, B, e).transpose(1, 2), d.Cg, f"slot {j} ZR[:, e] = xr Wt_e^T (group, token, column)", False, planes=planes)


def link_zr_others(d, B, zeroed=False):
    """the ZR columns of the experts without an xr slot (the multimodal ones): no kernel of a v1 site writes them"""
    ZR = B["ZR"].reshape(d.NT, d.g, d.E, d.dgp)
    return check_poison(ZR[:, :, :d.cfg.E_m], "ZR columns of the multimodal experts", zeroed)


# ---- backward links: the LAST slot (the scratch holds nothing else) --------------------------------------------------------------------------------
def link_dxr(d, B, j):
    """dxr = T(T(dZR_e Wt_e + dsr1 * xr) + dsr2 * X + dsr0) (moe_backward.cpp:165-172 | :176-183; kk_nxn_axpy bwd_kernels.hip:838): PRODUCT over
    dgp (v1) or E * dgp (AVVP) with the row-scale term in the epilogue (+ PLANES 3), then RMW with a product and two adds"""
    planes = 0.0 if d.bf16 else EPS_PLANES3
    NT = d.NT
    dsr = B["dsr"][j].double()
    xr = B["xr"][j].reshape(NT, d.g, d.Cg).permute(1, 0, 2).double()
    X = B["X"].reshape(NT, d.g, d.Cg).permute(1, 0, 2).double()
    dZR = B["dZR"].reshape(NT, d.g, d.E, d.dgp).permute(1, 0, 2, 3)
    if d.v1:
        e = d.slots[j][1]
        A, W, k = dZR[:, :, e], _wt(d, B, e), d.dgp
    else:
        A, W, k = dZR.reshape(d.g, NT, d.E * d.dgp), _wt(d, B), d.E * d.dgp
    p, magp = product_ref(A, W)
    t = dsr[1][None, :, None] * xr
    p, mag = p + t, magp + t.abs()
    first_pre = (k + 1) * EPS_ACC * mag + planes * magp
    t2, t0 = dsr[2][None, :, None] * X, dsr[0][None, :, None].expand_as(X)
    ref = p + t2 + t0
    got = B["dxr"].reshape(NT, d.g, d.Cg).permute(1, 0, 2)
    return check_bound(got, ref, rmw_bound(d, ref, p, first_pre, t2.abs() + t0.abs(), 3), f"slot {j} dxr = dZR Wt + dsr1 xr + dsr2 X + dsr0 (group, token, c)")


def link_dbout(d, B, j):
    """dbout = colsum(dxr) (:162): COLSUM over NT rows, delivered to the caller"""
    x = B["dxr"].reshape(d.NT, d.C).double()
    return check_bound(B["grads"][f"{d.slots[j][2]}.self_attention.out_proj.bias"], x.sum(0), colsum_bound(d.NT, x.abs().sum(0)), f"slot {j} dbout = colsum(dxr) (c)")


def link_dwout(d, B, j):
    """dWout = dxr^T O (:165), fp32, split K: PRODUCT over NT"""
    return prod(d, B["grads"][f"{d.slots[j][2]}.self_attention.out_proj.weight"], B["dxr"].reshape(d.NT, d.C).t(), B["mO"][j].reshape(d.NT, d.C), d.NT,
                f"slot {j} dWout = dxr^T O (row, c)", False)


def link_do(d, B, j):
    """mdO = dxr Wout (:170): PRODUCT over C"""
    return prod(d, B["mdO"].reshape(d.NT, d.C), B["dxr"].reshape(d.NT, d.C), B["mWout"][j], d.C, f"slot {j} mdO = dxr Wout (token, c)", True)


def link_dpd(d, B, j, zeroed=False):
    """mSc = (dO v^T) * keep (:175, km_keep_bwd :50): PRODUCT over dh and KEEP as one link, fp32; the padding stays what the forward left"""
    _, _, v = qkv(d, B["mQKV"][j])
    ref, mag = product_ref(_heads(d, B["mdO"]), v.transpose(-1, -2))
    keep = keep_of(d, B, d.slots[j][2])
    pre = d.dh * EPS_ACC * mag
    if keep is not None:
        ref, pre = ref * keep, pre * keep
        pre = pre + U32 * ref.abs()
    return max(check_bound(B["mSc"][..., :d.S], ref, pre, f"slot {j} mSc = (dO v^T) * keep (token, head, s, s')"),
               check_poison(B["mSc"][..., d.S:], "mSc columns S .. Sp behind the backward", zeroed))


def link_dv(d, B, j):
    """dv = Pd^T dO (:181): PRODUCT over S; from Pd with keep, from P without"""
    _, _, dv = qkv(d, B["mdQKV"])
    return prod(d, dv, _pd(d, B, j).transpose(-1, -2), _heads(d, B["mdO"]), d.S, f"slot {j} dv = Pd^T dO (token, head, s', dh)", True)


def link_ds(d, B, j):
    """mdS = P (dP - sum P dP) (:189): SOFTMAX'; columns S .. Sp exactly 0"""
    ref, bnd = H.softmax_bwd_ref(d, B["mP"][j][..., :d.S], B["mSc"][..., :d.S], "reg4")
    return max(check_bound(B["mdS"][..., :d.S], ref, bnd, f"slot {j} mdS = P (dP - dot) [reg4] (token, head, s, s')"),
               check_zero(B["mdS"][..., d.S:], "mdS columns S .. Sp") if d.Sp > d.S else 0.0)


def link_dq(d, B, j):
    """dq = alpha dS k (:192-193): PRODUCT over S"""
    _, k, _ = qkv(d, B["mQKV"][j])
    dq, _, _ = qkv(d, B["mdQKV"])
    return prod(d, dq, B["mdS"][..., :d.S], k, d.S, f"slot {j} dq = alpha dS k (token, head, s, dh)", True, alpha=d.alpha)


def link_dk(d, B, j):
    """dk = alpha dS^T q (:198-199): PRODUCT over S"""
    q, _, _ = qkv(d, B["mQKV"][j])
    _, dk, _ = qkv(d, B["mdQKV"])
    return prod(d, dk, B["mdS"][..., :d.S].transpose(-1, -2), q, d.S, f"slot {j} dk = alpha dS^T q (token, head, s', dh)", True, alpha=d.alpha)


def link_dbin(d, B, j):
    """dbin = colsum(mdQKV), all 3 C columns (:202): COLSUM"""
    x = B["mdQKV"].reshape(d.NT, 3 * d.C).double()
    return check_bound(B["grads"][f"{d.slots[j][2]}.self_attention.in_proj_bias"], x.sum(0), colsum_bound(d.NT, x.abs().sum(0)), f"slot {j} dbin = colsum(dQKV) (column)")


def link_dwin(d, B, j):
    """dWin = dQKV^T X (:205), fp32, split K: PRODUCT over NT"""
    return prod(d, B["grads"][f"{d.slots[j][2]}.self_attention.in_proj_weight"], B["mdQKV"].reshape(d.NT, 3 * d.C).t(), B["X"].reshape(d.NT, d.C), d.NT,
                f"slot {j} dWin = dQKV^T X (row, c)", False)


def link_dx(d, B, j):
    """dX of a single-slot v1 site: the sum of its three read-modify-writes.  (1) the site's dX product [dZx | dL2x] [Wt ; Text] + rs2x X
    (moe_backward.cpp:152-158; operands and terms as tests/test_stream_products_gpu.py B3; two-plane leaf at fp32 sites), stored in T;
    (2) kk_nxn_axpy: + dsr2 * xr - dxr with the STORED dxr (bwd_kernels.hip:841: a product and two adds), stored; (3) += dQKV Win (:210-211:
    PRODUCT over 3 C + the accumulate term), stored."""
    S, N, g, Cg, NT = d.S, d.N, d.g, d.Cg, d.NT
    A = torch.cat([B["Zw"].reshape(S, N, g, d.E * d.dgp).permute(0, 2, 1, 3), B["dL2x"][:, None, :, :d.KLT].expand(S, g, N, d.KLT)], 3)
    Bm = torch.cat([B["Wt"][None].expand(S, g, d.E * d.dgp, Cg), B["Text"].reshape(S, d.KLT, g, Cg).permute(0, 2, 1, 3)], 2)
    grp = lambda t: t.reshape(S, N, g, Cg).permute(0, 2, 1, 3).double()
    p0, magp = product_ref(A, Bm)
    t = B["rs2x"].double()[:, None, :, None] * grp(B["X"])
    p0, mag0 = p0 + t, magp + t.abs()
    e0 = _store(d, p0, (A.shape[-1] + 2) * EPS_ACC * mag0 + (0.0 if d.bf16 else EPS_PLANES) * magp, True)
    t2 = B["dsr"][j][2].double().reshape(S, 1, N, 1) * grp(B["xr"][j])
    gx = grp(B["dxr"])
    p1 = p0 + t2 - gx
    e1 = _store(d, p1, e0 + 3 * U32 * (p0.abs() + e0 + t2.abs() + gx.abs()), True)
    p2, mag2 = product_ref(B["mdQKV"].reshape(NT, 3 * d.C), B["mWin"][j])
    p2, mag2 = grp(p2), grp(mag2)
    ref = p1 + p2
    pre = e1 + (3 * d.C + 1) * EPS_ACC * (mag2 + p1.abs() + e1)
    return check_bound(grp(B["dX"]), ref, _store(d, ref, pre, True), f"slot {j} dX = dX product + dsr2 xr - dxr + dQKV Win (frame, group, n, c)")


FORWARD = {   # tag -> (what, kernel family of the profiler, link)
    "cast": ("mWin, mWout", "k_cast", link_cast), "qkv": ("mQKV", "gemm", link_qkv), "softmax": ("mP", "k_softmax_rows", link_softmax),
    "keep": ("mPd", "km_keep", link_keep), "o": ("mO", "gemm", link_o), "xr": ("xr", "gemm", link_xr), "sxr": ("sxr", "k_xrstats", link_sxr),
    "zr": ("ZR", "gemm", link_zr),
}
BACKWARD = {
    "dxr": ("dxr", "k_nxn_axpy", link_dxr), "dbout": ("dbout", "km_colsum_part", link_dbout), "dwout": ("dWout", "gemm", link_dwout),
    "do": ("mdO", "gemm", link_do), "dpd": ("mSc as dPd", "km_keep_bwd", link_dpd), "dv": ("dv", "gemm", link_dv),
    "ds": ("mdS", "k_softmax_rows_bwd", link_ds), "dq": ("dq", "gemm", link_dq), "dk": ("dk", "gemm", link_dk),
    "dbin": ("dbin", "km_colsum_part", link_dbin), "dwin": ("dWin", "gemm", link_dwin), "dx": ("dX", "gemm", link_dx),
}
GLUE = ("sxr", "zr", "dxr")      # the links an AVVP site shares


# ---- input families ----------------------------------------------------------------------------------------------------------------------------
def last_group(S):
    return 8 * ((S - 1) // 8)


def apply_family(P, X, family, cfg):
    """(P, X) of one family (module head)"""
    assert family in FAMILIES
    if family == "default":
        return P, X
    P, X = dict(P), X.clone()
    C, S, N = cfg.Cx, X.shape[0], cfg.Nx
    for e in range(cfg.E_m, cfg.E):
        pre = cfg.expert_prefixes()[e]
        W, b = P[f"{pre}.self_attention.in_proj_weight"].clone(), P[f"{pre}.self_attention.in_proj_bias"].clone()
        if family == "flat":
            W[:2 * C] *= FLAT_SCALE
            b[:2 * C] *= FLAT_SCALE
        else:
            W[:2 * C] *= PEAK_SCALE
            b[:C] = PEAK_BIAS * b[:C] / b[:C].norm() * math.sqrt(C)
        P[f"{pre}.self_attention.in_proj_weight"], P[f"{pre}.self_attention.in_proj_bias"] = W, b
    if family == "peaked":
        pre = cfg.expert_prefixes()[cfg.E - 1]                       # (the last slot is the one whose scores are stored)
        W, b = P[f"{pre}.self_attention.in_proj_weight"], P[f"{pre}.self_attention.in_proj_bias"]
        w = W[C:2 * C].t() @ b[:C]
        w = PEAK_PUSH * w / w.norm()
        n = torch.arange(N)
        for r, s in ((0, 0), (1, S - 1), (2, last_group(S))):
            X[s, n[n % 3 == r]] += w
    return P, X


def check_family(d, Sc, family):
    """the properties of the scores the family is there for, from the stored mSc (asserted, never skipped); returns the measured shares"""
    p = Sc[..., :d.S].double()
    span = (p.max(-1).values - p.min(-1).values).reshape(-1)
    am = p.argmax(-1).reshape(-1)
    got = {"max span": float(span.max()), "share span > 8": float((span > 8).double().mean()), "max in column 0": float((am == 0).double().mean()),
           "max in column S - 1": float((am == d.S - 1).double().mean()), "max in the last 8-group": float((am >= last_group(d.S)).double().mean())}
    if family == "flat":
        assert got["max span"] < 0.5, f"flat: a score row spans {got['max span']:.3g} >= 0.5"
    elif family == "peaked":
        assert got["share span > 8"] >= 0.9, f"peaked: only {got['share span > 8']:.3f} of the score rows span more than 8"
        for k in ("max in column 0", "max in column S - 1", "max in the last 8-group"):
            assert got[k] >= 0.1, f"peaked: {k}: only {got[k]:.3f} of the rows"
    return got


def draw_keep(cfg, S, seed):
    """{prefix: (N * H, S, S)} in {0, 1 / 0.8} (dropout 0.2), one row of every expert's all zero"""
    g = torch.Generator().manual_seed(seed + 7)
    out = {}
    for e in range(cfg.E_m, cfg.E):
        k = (torch.rand(cfg.Nx * HEADS, S, S, generator=g) >= 0.2).float() / 0.8
        k[min(5, cfg.Nx * HEADS - 1), S // 2] = 0.0
        out[cfg.expert_prefixes()[e]] = k
    return out


# ---- which kernel serves each product of the stage and of the glue ----------------------------------------------------------------------------
def stream_config(ks, tiles):
    """the configuration launch_gemm_stream picks for a one-segment product without accumulate (gemm_stream.hip:721-727, in its order)"""
    if ks <= 2 and tiles <= 12:
        return "k64_n192"
    if tiles <= 4 and ks <= 5:
        return "k160_n64"
    if ks <= 5 and tiles <= 24:
        return "k160_n384"
    if ks <= 12 and tiles <= 8:
        return "k384_n128"
    if ks <= 12 and tiles <= 9:
        return "k384_n144"
    return None


def stream_serves(d, a_kmajor, M, N, K, nb1, accumulate=False):
    """the name of the streaming kernel's record, or None where launch_gemm_stream steps aside (gemm_stream.hip:591-599: bf16, K-major A,
    M * nb1 >= 256, K <= 384, N <= 768 and a multiple of 4, no per-sample B; every stride of these products is a multiple of 16 bytes).  The
    batched products of the stage have a B per (token, head): nb1 > 1 with sB1 != 0.  An accumulating product is taken by k160_n64 /
    k160_n384 only (:722, :725)."""
    if not d.bf16 or not a_kmajor or nb1 > 1 or M < 256 or K > 384 or N > 768 or N % 4:
        return None
    ks, tiles = -(-K // 32), -(-N // 16)
    if accumulate:
        return "gemm_stream_k160_n64" if (tiles <= 4 and ks <= 5) else ("gemm_stream_k160_n384" if (ks <= 5 and tiles <= 24) else None)
    cfg = stream_config(ks, tiles)
    return cfg and "gemm_stream_" + cfg


def engine_tile(M, N, batch):
    """the tile launch_gemm picks (gemm.h:184 gemm_auto_tile; gemm.hip:1176-1180: fewer than GEMM_MIN_BLOCKS = 160 blocks -> the next smaller
    tile).  No product here is split over K (choose_ksplit: K / (4 * 64) < 2 at NT < 512) or folded (nb1 = 1 or nb2 = 4)."""
    cd = lambda a, b: -(-a // b)
    t = 128 if (M > 64 and N > 64) else (32 if (M <= 32 and N <= 32) else 64)
    if t == 128 and cd(M, 128) * cd(N, 128) * batch < 160:
        t = 64
    if t == 64 and cd(M, 64) * cd(N, 64) * batch < 160:
        t = 32
    return t


def instance(d, layout, M, N, K, nb1=1, nb2=1, ty=None, accumulate=False):
    """the profiler name of one product: gemm_stream_<configuration>, or gemm_<layout>_<type>_<tile> of the tiled engine.  gemm_frames never
    serves one of them: it wants nb2 = 1 and nb1 >= 32 frames against one shared B (frame_gemm.hip:340-341)."""
    return stream_serves(d, layout[0] == "K", M, N, K, nb1, accumulate) or f"gemm_{layout}_{ty or ('bf16' if d.bf16 else 'f32')}_{engine_tile(M, N, nb1 * nb2)}"


def stage_instances(d):
    """({name: launches} of the forward, of section 2) that the frame attention and its glue add to the site's profiler report, per site: the
    products of mha_frames.hip in their order, ZR (moe_forward.cpp:196), dxr (moe_backward.cpp:165) and the expert's share of dWt (:266).  fp32 sites: the stage runs the exact
    fp32 instances, the glue three planes.  Not in the report: dWout = dxr^T O, the first scoped launch of mha_frames_backward, which closes
    the record of that name (prof.cpp:39, :58)."""
    S, N, C, NT, dh, Hh = d.S, d.N, d.C, d.NT, d.dh, d.H
    planes = None if d.bf16 else "f32s3"
    fwd = [instance(d, "KK", NT, 3 * C, C),                       # X Win^T
           instance(d, "KK", S, S, dh, N, Hh),                    # q k^T
           instance(d, "KM", S, dh, S, N, Hh),                    # Pd v
           instance(d, "KK", NT, C, C),                           # O Wout^T
           instance(d, "KK", NT, d.dgp, d.Cg, 1, d.g, planes)]    # ZR[:, e] = xr Wt_e^T
    bwd = [instance(d, "KM", NT, d.Cg, d.dgp, 1, d.g, planes),    # dxr = dZR_e Wt_e + dsr1 xr
           instance(d, "KM", NT, C, C),                           # dO = dxr Wout
           instance(d, "KK", S, S, dh, N, Hh),                    # dPd = dO v^T
           instance(d, "MM", S, dh, S, N, Hh),                    # dv = Pd^T dO
           instance(d, "KM", S, dh, S, N, Hh),                    # dq = dS k
           instance(d, "MM", S, dh, S, N, Hh),                    # dk = dS^T q
           instance(d, "MM", 3 * C, C, NT),                       # dWin = dQKV^T X
           instance(d, "KM", NT, C, 3 * C, accumulate=True),      # dX += dQKV Win
           instance(d, "MM", d.dgp, d.Cg, NT, 1, d.g, None if d.bf16 else "f32s2")]      # dWt_e += dZR_e^T xr_e (moe_backward.cpp:266; a two-plane leaf)
    out = []
    for names in (fwd, bwd):
        c = {}
        for n in names:
            c[n] = c.get(n, 0) + len(d.slots)
        out.append(c)
    return tuple(out)


# ---- the sites of both test modules ------------------------------------------------------------------------------------------------------------
# case -> (S, N, C, E_m, E_s, reduction, variant, self_attn, training): the table of the issue.  reduction 4 keeps the two groups apart at
# C >= 96 (g = 2), 8 merges them (g = 1: moe_plan.cpp:95-106)
SITES = {
    "S5_C64": (5, 24, 64, 1, 1, 8, "avs", "v1", True),
    "S8_C32": (8, 25, 32, 1, 1, 8, "avs", "v1", True),
    "S13_C96": (13, 12, 96, 1, 1, 4, "avs", "v1", True),
    "S70_C128": (70, 6, 128, 1, 1, 4, "avs", "v1", True),
    "S13_C320": (13, 9, 320, 1, 1, 4, "avs", "v1", True),
    "S13_two_slots": (13, 24, 64, 2, 2, 8, "avs", "v1", True),
    "S5_eval": (5, 24, 64, 1, 1, 8, "avs", "v1", False),
    "avvp": (6, 40, 96, 2, 2, 4, "avvp", "none", True),
}
CASES = [("S5_C64", "default", "bf16"), ("S5_C64", "default", "fp32"), ("S8_C32", "default", "bf16"), ("S13_C96", "default", "bf16"),
         ("S13_C96", "default", "fp32"), ("S70_C128", "default", "bf16"), ("S13_C320", "default", "bf16"), ("S13_two_slots", "default", "bf16"),
         ("S5_eval", "default", "bf16"), ("avvp", "default", "bf16")] + [(s, f, "bf16") for s in ("S13_C96", "S70_C128") for f in ("flat", "peaked")]
SEED = 21


def site_config(site):
    S, N, C, E_m, E_s, red, variant, sa, training = SITES[site]
    return O.AdapterConfig(Cx=C, Nx=N, Cy=64, Ny=16, reduction=red, groups=2, K=8, E_m=E_m, E_s=E_s, variant=variant, self_attn=sa), S, training


def draw_site(site, family):
    """(cfg, S, training, P, Bf, X, Y, G, keep) as both modules draw them"""
    cfg, S, training = site_config(site)
    P, Bf = O.init_params(cfg, seed=SEED)
    g = torch.Generator().manual_seed(SEED + 100)
    X = 0.3 * torch.randn(S, cfg.Nx, cfg.Cx, generator=g)
    Y = 0.3 * torch.randn(S, cfg.Ny, cfg.Cy, generator=g)
    G = torch.randn(S, cfg.Nx, cfg.Cx, generator=g)
    if cfg.self_attn == "v1":
        P, X = apply_family(P, X, family, cfg)
    keep = draw_keep(cfg, S, SEED) if (training and cfg.self_attn == "v1") else None
    return cfg, S, training, P, Bf, X, Y, G, keep
