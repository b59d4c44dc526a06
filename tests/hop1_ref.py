"""fp64 references and element-wise bounds for the links of the hop-1 chain between its two ends on Y -- the weight-space glue (k_prep_all's
remap part, k_qrqb_fill, k_finish_T, k_finish_dT, k_prep_dBm, k_dqrqb, k_hop1_finalize), the products of its middle (Qx, L1, [Bm | ab], TV, TT,
TW, dTW, dTT, dV, dA1, dR^T, dWcK, dWf, dT0), the row softmax in both directions, and the latent-on-X side of an AVS v2 site (FORWARD_X /
BACKWARD_X) -- each from its operands EXACTLY AS STORED in the workspace (bf16 and fp32 are exact in fp64, so
nothing upstream of a link adds error).  Same style as tests/stream_product_ref.py / tests/nxn_ref.py: check_bound, the product terms and the
softmax terms come from there; nothing here is fitted to a measured error and no constant is new.

A link is a function  link(d, B) -> worst err / bound  (raises ProductMismatch, an AssertionError, naming the element).  d: Dims (every padded
width of the plan), B: {buffer name: tensor in the buffer's own dtype and shape (Dims.shape)} plus "Y" and the parameters under their state-dict
names.  The GPU test hands device views of the workspace, tests/test_hop1_checker.py an emulation on the CPU.

Terms (per element unless said otherwise):

  CAST      stT<T> / st4T<T> = (__bf16)x (device_utils.h:30,57,71): round to nearest even, ONE rounding.  Held as EQUALITY with torch's
            .bfloat16() of the fp32 value the kernel text forms (fwd_kernels.hip:162,166,169,262,563,582; bwd_kernels.hip:564-572).
  PRODUCT   product_bound of stream_product_ref: k * EPS_ACC * (|A| |B|) for an fp32 accumulation of k products in any order (the engine and
            frame_gemm.hip alike: MFMA into fp32 accumulators, K chunks / split K only reorder), + EPS_BF16 |ref| for a bf16 store.
  DOT       a wave's fp32 dot product of k terms (kk_qrqb_fill :550-558, prep_rw :181-189, kk_finish_dT :458-471, kk_dqrqb_part
            bwd_kernels.hip:607-608, the softmax backward's `dot` :360, :393): every lane adds its ceil(k / 64) products one after the other
            (the register-resident softmax backward: its 4 NV entries, whatever n is), wave_sum folds the 64 lanes in 6 steps, and each
            product rounds once: at most ceil(k / 64) + 7 roundings on any path, so (ceil(k / 64) + 7) * EPS_ACC * sum |x y| (dot_bound).
            The order-free k * EPS_ACC of PRODUCT would hide what these links are there for: the rounding of dTy in front of dabx is
            2^-9 sqrt(C) of the sum, below C * 2^-23 of it.
  ELEMENTWISE  r fp32 operations on a sum of terms: r * U32 * (sum of the |terms|)   (each operation rounds a value no larger than that sum).
  SOFTMAX   as nxn_ref: `p - mx` one fp32 subtraction, U32 * max(|p|, |mx|, |p - mx|) ABSOLUTE on the argument; __expf: EPS_ACC * |x| on the
            argument (rounded log2 e, rounded product) and EPS_ACC relative (v_exp_f32), TINY absolute (flushed results).  The sum of the
            exponentials carries their relative errors weighted by exp(x_j) / sum, plus its own additions:
              kk_softmax_rows_reg<NV> (fwd_kernels.hip:652-658)  sums in double and rounds 1 / sum to fp32 once:  U32
              kk_softmax_rows         (:615-618)                  float, n / 64 additions per lane + 6 shuffle steps: (ceil(n / 64) + 6) * EPS_ACC,
                                                                  and `1.f / sm` (one ulp: EPS_ACC)
            then `e * inv` (U32) and the store (EPS_BF16 in bf16; fp32 stores nothing more).  The maximum of fp32 numbers is exact.
  DSUM      a sum the kernel accumulates in double and casts once (k_finish_T's Tsum :741-753, prep_wbar :218-224): U32 * |ref| for the cast
            + 2^-24 of the result for whatever fp32 partial it folds (the issue's statement of the term), i.e. 2 * U32 * |ref|; where fp32
            partials enter first (prep_wbar's eight accumulators per stream) they count as DOT terms.
  PLANES    an fp32 site feeds its fp32 operands to the bf16 matrix pipe in three planes (EPS_PLANES3 of engine_forms_ref) or, for dWf and
            dWcK, two (EPS_PLANES of stream_product_ref), of |A| |B|; its stores are fp32 and every CAST is the identity.
  FSUM      a sum over frames / rows in fp32 (or double partials folded in fp32): (terms) * EPS_ACC * sum |x|.

What a bound on a SUM cannot see: an error that stays below (terms) * 2^-23 * sum |x| -- one dropped frame among hundreds whose term is smaller
than the allowed rounding of the others, or two terms exchanged.  The per-element links around it (every frame's row Kcy of dBm, every dabx)
are what pin those.
"""
import torch

from tests.engine_forms_ref import EPS_PLANES3
from tests.nxn_ref import TINY, U32
from tests.stream_product_ref import (EPS_ACC, EPS_BF16, EPS_PLANES, ProductMismatch, check_bound, check_untouched, product_bound,  # noqa: F401
                                      product_ref)


def _ru(x, m):
    return -(-x // m) * m


class Dims:
    """The widths of one site as moe_plan.cpp lays them out (:135-143, :164-166); Kp and dgp are the plan's choice and are read off the sizes
    of its buffers (nbytes: {name: bytes} from avmoe_moe_buffer_info, which needs no GPU)."""

    def __init__(self, cfg, S, bf16, nbytes):
        self.cfg, self.S, self.bf16 = cfg, S, bf16
        self.esz = 2 if bf16 else 4
        self.T = torch.bfloat16 if bf16 else torch.float32
        self.N, self.M, self.C, self.Cy, self.K, self.E = cfg.Nx, cfg.Ny, cfg.Cx, cfg.Cy, cfg.K, cfg.E
        self.NT = S * self.N
        self.Ey = cfg.E_m
        self.Ex = cfg.E_s if cfg.self_attn == "v2" else 0
        self.El = self.Ey + self.Ex
        self.Kp = nbytes["a"] // (max(self.El, 1) * self.NT * self.esz)
        self.g = 1 if nbytes["mWd"] > 4 else cfg.groups
        self.Cg = self.C // self.g
        self.dgp = nbytes["wsum"] // 4 // (self.E * self.g)
        self.DZ = self.E * self.g * self.dgp
        self.KL = self.El * self.Kp
        self.KLT = self.KL + 2
        self.Kcy, self.Kcx = self.Ey * self.Kp, self.Ex * self.Kp
        self.Kcyb = self.Kcy + 1
        self.Kcyp, self.Kcxp = _ru(max(self.Kcy, 1), 8), _ru(max(self.Kcx, 1), 8)
        self.Np, self.Mk, self.Mb = _ru(self.N, 8), _ru(self.M + 2, 8), _ru(self.M + 1, 8)
        self.tok_keys = [cfg.expert_prefixes()[l] + ".my_tokens" for l in range(self.El)]      # (latent experts come first: expert l owns slot l)
        for k, v in self.shapes().items():                                                     # the table agrees with the plan's sizes
            n = 1
            for x in v[1]:
                n *= x
            assert n * (4 if v[0] == "f" else self.esz) <= nbytes[k], (k, v, nbytes[k])

    def shapes(self):
        """{buffer: ("T" | "f", shape)} -- moe_plan.h::AVMOE_BUFFERS, the hop-1 chain's part"""
        S, N, M, C, Cy, K = self.S, self.N, self.M, self.C, self.Cy, self.K
        rows = max(self.Kcyb, self.Kcx)
        return {
            "WcK": ("T", (N, self.Mk)), "WcT": ("T", (M + 1, self.Np)), "WfT": ("T", (C, Cy)), "rw": ("f", (C,)), "wbar": ("f", (self.Mb,)),
            "scal": ("f", (64,)), "T0T": ("T", (self.KL, C)), "Wt": ("T", (self.g, self.E * self.dgp, self.Cg)),
            "Qx": ("T", (self.Kcy, Cy)), "qrqb": ("f", (2, self.Kcy)), "Rext": ("T", (S, self.Kcyb, self.Mk)),
            "A1y": ("T", (S, self.Kcyb, self.Np)), "BmX": ("T", (S, self.Kcyb, self.Mb)), "V": ("T", (S, self.Kcyb, Cy)),
            "Text": ("T", (S, self.KLT, C)), "Tsum": ("f", (2, S, self.KLT)), "TT": ("f", (S, max(self.El, 1), K, K)),
            "TW": ("f", (S, self.KLT, self.g, self.E * self.dgp)), "rin": ("f", (S, 2 * C)),
            "L1": ("f", (S, rows, self.Np)), "TV": ("f", (S, rows, C)),
            "dT": ("f", (S, self.KL, C)), "dtbar": ("f", (S, self.KL)), "rbw": ("f", (S * (self.E + 32 + 128 + 2 * C),)),
            "dTy": ("T", (S, self.Kcyb, C)), "dTx": ("T", (S, max(self.Kcx, 1), C)), "dabx": ("f", (S, self.Kcyb)),
            "dV": ("T", (S, self.Kcyb, Cy)), "dBm": ("f", (S, self.Kcyb, self.Mb)), "dBmT": ("T", (S, self.Kcyb, self.Mb)),
            "dvec": ("f", (2 * C + self.Mb + 64,)), "dL1": ("T", (S, rows, self.Np)), "dRT": ("T", (S, M, self.Kcyp)),
            "dWcK": ("f", (N, self.Mk)), "dqp": ("f", (2 * S * self.Kcyb + 2 * self.Kcyb,)), "dT0": ("f", (self.KL, C)),
            "dQT": ("T", (self.Kcy, Cy)), "dWf": ("f", (C, Cy)),
            "A1x": ("T", (S, max(self.Kcx, 1), self.Np)), "dL1xT": ("T", (S, N, self.Kcxp)),
            "Zw": ("T", (S, N, self.g, self.E * self.dgp)), "a": ("T", (self.El, S, N, self.Kp)), "ag": ("T", (self.El, S, N, self.Kp)),
            "aw": ("T", (self.El, S, N, self.Kp)), "dTW": ("T", (S, self.KLT, self.g, self.E * self.dgp)), "dTT": ("T", (S, self.El, K, self.Kp)),
        }


# ---- helpers -----------------------------------------------------------------------------------------------------------------------------
def check_exact(got, want, name):
    """bit-for-bit (values compared: +0 == -0), every element finite"""
    return check_bound(got, want.double(), torch.zeros_like(want, dtype=torch.float64), name)


def check_zero(region, name):
    return check_exact(region, torch.zeros_like(region, dtype=torch.float64), name)


def castT(d, x):
    """CAST: what stT<T> stores for the fp32 value x"""
    return x.float().to(d.T)


def _store(d, ref, pre, out_T):
    """a value with absolute error `pre` before its store in T (out_T) or in fp32"""
    return pre + EPS_BF16 * (ref.abs() + pre) if (out_T and d.bf16) else pre


def _params(d, B):
    Wc = B["conv_adapter.weight"].reshape(d.N, d.M).float()
    return Wc, B["conv_adapter.bias"].float(), B["fc.weight"].float(), B["fc.bias"].float()


def dot_bound(k, mag, per_lane=None):
    """DOT: k terms over a wave (per_lane: the additions of one lane where they are not ceil(k / 64))"""
    return ((per_lane if per_lane else -(-k // 64)) + 7) * EPS_ACC * mag


def real_rows(d):
    """mask over the Kcyb rows of a frame: a latent row kc < Kcy whose slot entry k = kc % Kp is a token (k < K)"""
    q = torch.arange(d.Kcyb)
    return (q < d.Kcy) & ((q % d.Kp) < d.K)


# ---- forward links, in the order of moe_forward.cpp:92-180 -------------------------------------------------------------------------------------
def link_prep(d, B):
    """k_prep_all, remap part (fwd_kernels.hip:157-278): WcK = [Wc | bc | 1 | 0..], WcT = [Wc ; bc] with Np padding, WfT (CAST each),
    rw = Wf 1 from the T-rounded weights (DOT, Cy terms), wbar = mean_n Wc (DOT over N + DSUM; padding m >= M exactly 0),
    scal[0] = mean(bc) (DOT over N + the division: U32), T0T (CAST; slot rows k >= K exactly 0), the ones / zero row of Text and their Tsum."""
    Wc, bc, Wf, _ = _params(d, B)
    N, M, C = d.N, d.M, d.C
    dev = Wc.device
    WcK = torch.zeros(N, d.Mk, device=dev)
    WcK[:, :M], WcK[:, M], WcK[:, M + 1] = Wc, bc, 1.0
    WcT = torch.zeros(M + 1, d.Np, device=dev)
    WcT[:M, :N], WcT[M, :N] = Wc.t(), bc
    w = [check_exact(B["WcK"], castT(d, WcK), "prep WcK = T([Wc | bc | 1 | 0]) (n, m)"),
         check_exact(B["WcT"], castT(d, WcT), "prep WcT = T([Wc ; bc]^T, Np padding 0) (m, n)"),
         check_exact(B["WfT"], castT(d, Wf), "prep WfT (c, y)")]
    WfR = castT(d, Wf).double()
    w.append(check_bound(B["rw"], WfR.sum(1), dot_bound(d.Cy, WfR.abs().sum(1)), "prep rw = T(Wf) 1 (c)"))
    ref = torch.zeros(d.Mb, dtype=torch.float64, device=dev)
    ref[:M] = Wc.double().mean(0)
    bnd = torch.zeros_like(ref)
    bnd[:M] = N * EPS_ACC * Wc.double().abs().mean(0) + 2 * U32 * ref[:M].abs()
    w.append(check_bound(B["wbar"], ref, bnd, "prep wbar = mean_n Wc, padding 0 (m)"))
    mb = bc.double().mean()
    w.append(check_bound(B["scal"][:2], torch.stack([mb, torch.ones_like(mb)]),
                         torch.stack([N * EPS_ACC * bc.double().abs().mean() + U32 * mb.abs(), torch.zeros_like(mb)]), "prep scal[0] = mean(bc), scal[1] = 1"))
    T0 = torch.zeros(d.El, d.Kp, C, device=dev)
    for l, k in enumerate(d.tok_keys):
        T0[l, :d.K] = B[k].float()
    w.append(check_exact(B["T0T"], castT(d, T0.reshape(d.KL, C)), "prep T0T = T(my_tokens), slot rows k >= K zero (row, c)"))
    return max(w)


def link_const_rows(d, B):
    """prep_const_rows (fwd_kernels.hip:268-277) as the forward leaves them: ones row of Text exactly 1 with Tsum = C in both planes, the dm1
    row exactly 0 (the backward writes it) with Tsum 0."""
    Text, Tsum = B["Text"], B["Tsum"]
    one = torch.ones_like(Text[:, d.KL], dtype=torch.float64)
    w = [check_exact(Text[:, d.KL], one, "Text ones row (frame, c)"), check_zero(Text[:, d.KL + 1], "Text dm1 row in the forward (frame, c)"),
         check_exact(Tsum[:, :, d.KL], torch.full_like(Tsum[:, :, d.KL], float(d.C), dtype=torch.float64), "Tsum of the ones row = C (plane, frame)"),
         check_zero(Tsum[:, :, d.KL + 1], "Tsum of the dm1 row (plane, frame)")]
    return max(w)


def link_Qx(d, B):
    """Qx = T0 Wf (moe_forward.cpp:94-98): C terms, stored in T"""
    return check_product(B["Qx"], B["T0T"][:d.Kcy], B["WfT"], d, out_T=True, k_terms=d.C, name="Qx = T0 Wf (row, y)")


def planes_term(d, mag, planes=3):
    """PLANES: nothing on a bf16 site; on an fp32 site the operand term of the engine's three-plane (moe_run.h: AVMOE_FWD_SPLIT3 = 1,
    AVMOE_BWD_PLANES = 1) or two-plane form (AVMOE_LEAF2 class 8: dWf, dWcK)"""
    return 0.0 if d.bf16 else (EPS_PLANES3 if planes == 3 else EPS_PLANES) * mag


def check_product(got, A, Bm, d, *, out_T, k_terms, name, extra=None, planes=3):
    ref, mag = product_ref(A, Bm, extra)
    return check_bound(got, ref, product_bound(ref, mag, out_bf16=out_T and d.bf16, k_terms=k_terms) + planes_term(d, mag, planes), name)


def link_qrqb(d, B):
    """k_qrqb_fill (fwd_kernels.hip:541-585): qr = T0 . rw, qb = T0 . bf (DOT, C terms); Rext[s][kc][M] = T(qr), [M + 1] = T(qb): CAST of
    the stored qrqb, the same bits in every frame; columns M + 2 .. Mk exactly 0; row Kcy of Rext exactly 0; row Kcy of BmX = T(wbar)."""
    _, _, _, bf = _params(d, B)
    T0 = B["T0T"][:d.Kcy].double()
    rw = B["rw"].double()
    vec = torch.stack([rw, bf.double()], 1)                                                      # (C, 2)
    ref, mag = T0 @ vec, T0.abs() @ vec.abs()
    w = [check_bound(B["qrqb"].t(), ref, dot_bound(d.C, mag), "qrqb = T0 . [rw | bf] (row, qr / qb)")]
    Rext, M = B["Rext"], d.M
    ext = castT(d, B["qrqb"].t())[None].expand(d.S, d.Kcy, 2)
    w.append(check_exact(Rext[:, :d.Kcy, M:M + 2], ext, "Rext[.., M : M + 2] = T(qr | qb) in every frame (frame, row, qr / qb)"))
    w.append(check_zero(Rext[:, :d.Kcy, M + 2:], "Rext columns M + 2 .. Mk (frame, row, column - M - 2)"))
    w.append(check_zero(Rext[:, d.Kcy], "Rext row Kcy (frame, column)"))
    w.append(check_exact(B["BmX"][:, d.Kcy], castT(d, B["wbar"])[None].expand(d.S, d.Mb), "BmX row Kcy = T(wbar) (frame, m)"))
    return max(w)


def link_L1(d, B):
    """L1[s] = [R | qr | qb][s] [Wc | bc | 1]^T in fp32 (moe_forward.cpp:109-115): M + 2 terms"""
    return check_product(B["L1"][:, :d.Kcy, :d.N], B["Rext"][:, :d.Kcy, :d.M + 2], B["WcK"][:, :d.M + 2].t(), d, out_T=False, k_terms=d.M + 2,
                         name="L1 = [R | qr | qb] [Wc | bc | 1]^T (frame, row, n)")


def softmax_text(n, ld):
    """the kernel text k_softmax_rows launches (fwd_kernels.hip:671-680; ld_in = ld_out = Np % 4 == 0 at every site)"""
    if ld % 4 == 0 and n <= 4096:
        return "reg4" if n <= 1024 else "reg16"
    return "plain"


def softmax_bwd_text(ld):
    """... and k_softmax_rows_bwd (bwd_kernels.hip:419-433; the buffers are 256-byte aligned: moe_plan.cpp)"""
    if ld % 4 == 0 and ld <= 4096:
        return "reg4" if ld <= 1024 else "reg16"
    return "plain"


def softmax_ref(d, L, text):
    """(ref, bound) of T(softmax(L)) per element; L: (.., n) fp32 logits as stored (SOFTMAX above)"""
    p = L.double()
    n = p.shape[-1]
    mx = p.max(-1, keepdim=True).values
    x = p - mx
    e = torch.exp(x)
    delta = U32 * torch.maximum(torch.maximum(p.abs(), mx.abs().expand_as(p)), x.abs()) + EPS_ACC * x.abs()
    e_e = e * (torch.expm1(delta) + EPS_ACC) + TINY
    sm = e.sum(-1, keepdim=True)
    e_sum = e_e.sum(-1, keepdim=True) / sm + (U32 if text != "plain" else ((-(-n // 64) + 6) * EPS_ACC + EPS_ACC))      # relative (sm >= 1)
    ref = e / sm
    pre = e_e / sm + ref * (e_sum / (1 - e_sum)) + U32 * ref
    return ref, _store(d, ref, pre, True)


def link_softmax(d, B, text=None):
    """k_softmax_rows -> A1y (fwd_kernels.hip:602-683): every real row per element against fp64 of the stored L1 row; its sum 1 within the sum of
    the elements' bounds; columns N .. Np exactly 0; row Kcy of every frame and the slot rows k >= K exactly 0 (whatever L1 holds there: the
    workspace poison)."""
    text = text or softmax_text(d.N, d.Np)
    A1, N = B["A1y"], d.N
    real = real_rows(d).to(A1.device)
    ref, bnd = softmax_ref(d, B["L1"][:, :d.Kcyb][:, real, :N], text)
    w = [check_bound(A1[:, real, :N], ref, bnd, f"A1y = softmax(L1) [{text}] (frame, real row, n)"),
         check_bound(A1[:, real, :N].double().sum(-1), torch.ones_like(ref[..., 0]), bnd.sum(-1), f"A1y row sums [{text}] (frame, real row)"),
         check_zero(A1[:, :, N:], "A1y columns N .. Np (frame, row, column - N)"),
         check_zero(A1[:, ~real], "A1y row Kcy and slot rows k >= K (frame, row, column)")]
    return max(w)


def link_BmX(d, B):
    """[Bm | ab][s] = A1[s] [Wc | bc] into BmX[:, :Kcy] (moe_forward.cpp:118-124): N terms, stored in T; ab in column M."""
    return check_product(B["BmX"][:, :d.Kcy, :d.M + 1], B["A1y"][:, :d.Kcy, :d.N], B["WcT"][:, :d.N].t(), d, out_T=True, k_terms=d.N,
                         name="[Bm | ab] = A1 [Wc | bc] (frame, row, m)")


def link_BmX_pad(d, B):
    """the columns of BmX behind ab, M + 1 .. Mb, rows < Kcy: exactly 0"""
    return check_zero(B["BmX"][:, :d.Kcy, d.M + 1:], "BmX columns M + 1 .. Mb (frame, row, column - M - 1)")


def link_TV(d, B):
    """TV = V Wf^T in fp32, all S * Kcyb rows (moe_forward.cpp:133-138): Cy terms"""
    return check_product(B["TV"][:, :d.Kcyb], B["V"], B["WfT"].t(), d, out_T=False, k_terms=d.Cy, name="TV = V Wf^T (frame, row, c)")


def link_finish_T(d, B):
    """k_finish_T, src = 0 (fwd_kernels.hip:694-754): Text[s][slot rows] = T(T0 + TV + ab rw + bf) from the stored TV, BmX[.., M], rw and the
    parameters -- `tk + tv`, `ab * r + b` (two roundings, or one when contracted), `v +=`: ELEMENTWISE with r = 4, then the store;
    Tsum against the sums of the row AS STORED (DSUM); rin[s][C:] = TV[s][Kcy] + scal[0] rw + bf (ELEMENTWISE, r = 3); slot rows k >= K exactly
    0 in Text and Tsum."""
    _, _, _, bf = _params(d, B)
    S, C, K, Kp = d.S, d.C, d.K, d.Kp
    rw, bfd = B["rw"].double(), bf.double()
    w = []
    Text = B["Text"][:, :d.Kcy].reshape(S, d.Ey, Kp, C)
    Tsum = B["Tsum"][:, :, :d.Kcy].reshape(2, S, d.Ey, Kp)
    tok = torch.stack([B[k].double() for k in d.tok_keys[:d.Ey]])[None]                           # (1, Ey, K, C)
    tv = B["TV"][:, :d.Kcy].reshape(S, d.Ey, Kp, C)[:, :, :K].double()
    ab = B["BmX"][:, :d.Kcy, d.M].reshape(S, d.Ey, Kp)[:, :, :K].double()[..., None]
    ref = tok + tv + ab * rw + bfd
    pre = 4 * U32 * (tok.abs() + tv.abs() + (ab * rw).abs() + bfd.abs())
    w.append(check_bound(Text[:, :, :K], ref, _store(d, ref, pre, True), "Text y slots = T(T0 + TV + ab rw + bf) (frame, slot, k, c)"))
    st = Text[:, :, :K].double()
    for pl, (r, nm) in enumerate(((st.sum(-1), "sum"), ((st * st).sum(-1), "sum of squares"))):
        w.append(check_bound(Tsum[pl][:, :, :K], r, 2 * U32 * r.abs(), f"Tsum row {nm} of Text as stored (frame, slot, k)"))
    if Kp > K:
        w.append(check_zero(Text[:, :, K:], "Text slot rows k >= K (frame, slot, k - K, c)"))
        w.append(check_zero(Tsum[:, :, :, K:], "Tsum slot rows k >= K (plane, frame, slot, k - K)"))
    tvb = B["TV"][:, d.Kcy].double()
    s0 = B["scal"][0].double()
    ref = tvb + s0 * rw + bfd
    w.append(check_bound(B["rin"][:, C:], ref, 3 * U32 * (tvb.abs() + (s0 * rw).abs() + bfd.abs()), "rin[:, C:] = TV[Kcy] + scal[0] rw + bf (frame, c)"))
    return max(w)


def link_TT(d, B):
    """TT[s][l] = T T^T per (frame, slot), rows k < K (moe_forward.cpp:165-172): C terms, fp32"""
    T = B["Text"][:, :d.KL].reshape(d.S, d.El, d.Kp, d.C)[:, :, :d.K]
    return check_product(B["TT"], T, T.transpose(2, 3), d, out_T=False, k_terms=d.C, name="TT = T T^T (frame, slot, k, k')")


def link_TW(d, B):
    """TW = Text Wt^T over all KLT rows, per group (moe_forward.cpp:173-180): Cg terms, fp32.  The ones row is a real row; the dm1 row is zero
    in the forward, so its products are exactly 0 (a bound of 0 demands equality)."""
    A = B["Text"].reshape(d.S, d.KLT, d.g, d.Cg).permute(0, 2, 1, 3)                              # (S, g, KLT, Cg)
    return check_product(B["TW"].permute(0, 2, 1, 3), A, B["Wt"].transpose(1, 2)[None], d, out_T=False, k_terms=d.Cg, name="TW = Text Wt^T (frame, group, row, j)")


# ---- backward links, in the order of moe_backward.cpp:330-396 ----------------------------------------------------------------------------------
def drin_of(d, B):
    """drin (S, 2 C) inside rbw: behind the S x 128 block of dh1 (bwd_kernels.hip:318-319, :913)"""
    return B["rbw"][d.S * 128:d.S * 128 + d.S * 2 * d.C].reshape(d.S, 2 * d.C)


def link_finish_dT(d, B):
    """kk_finish_dT (bwd_kernels.hip:443-488): dTy[s][q < Kcy] = Tb(dT + dtbar / C): the division (U32 |add|), the addition (U32), the store;
    row Kcy = Tb(drin[s][C:]) (CAST: add = 0 is exact); dabx = dTy . rw from the ROUNDED dTy as stored (DOT, C terms); dTx likewise where the
    site has latent-on-X slots."""
    S, C, Kcy = d.S, d.C, d.Kcy
    dT, dtb = B["dT"].double(), B["dtbar"].double()
    add = dtb[:, :Kcy, None] / C
    ref = dT[:, :Kcy] + add
    pre = U32 * add.abs() + U32 * ref.abs()
    w = [check_bound(B["dTy"][:, :Kcy], ref, _store(d, ref, pre, True), "dTy = Tb(dT + dtbar / C) (frame, row, c)"),
         check_exact(B["dTy"][:, Kcy], castT(d, drin_of(d, B)[:, C:]), "dTy row Kcy = Tb(drin[:, C:]) (frame, c)")]
    dTy, rw = B["dTy"].double(), B["rw"].double()
    w.append(check_bound(B["dabx"], dTy @ rw, dot_bound(C, dTy.abs() @ rw.abs()), "dabx = dTy(rounded) . rw (frame, row)"))
    if d.Kcx:
        add = dtb[:, Kcy:, None] / C
        ref = dT[:, Kcy:] + add
        pre = U32 * add.abs() + U32 * ref.abs()
        w.append(check_bound(B["dTx"], ref, _store(d, ref, pre, True), "dTx = T(dT + dtbar / C) (frame, row, c)"))
    return max(w)


def link_dV(d, B):
    """dV = dTy Wf (moe_backward.cpp:342-347): C terms, stored in T"""
    return check_product(B["dV"], B["dTy"], B["WfT"], d, out_T=True, k_terms=d.C, name="dV = dTy Wf (frame, row, y)")


def link_prep_dBm(d, B):
    """kk_prep_dBm (bwd_kernels.hip:553-599): dBmT = T([dBm | dabx | 0]) (CAST) with row Kcy exactly 0 -- every column, the 4-vector that
    contains column M among them (it mixes dBm, dabx and zeros when M % 4 != 0); dwbar[m] = sum_s dBm[s][Kcy][m] and dbcbar = sum_s dabx[s][Kcy]
    in dvec (FSUM, S terms)."""
    S, M, Kcy = d.S, d.M, d.Kcy
    want = torch.zeros_like(B["dBm"])
    want[:, :Kcy, :M] = B["dBm"][:, :Kcy, :M]
    want[:, :Kcy, M] = B["dabx"][:, :Kcy]
    v0 = (M // 4) * 4
    w = [check_exact(B["dBmT"][:, :, v0:v0 + 4], castT(d, want[:, :, v0:v0 + 4]), f"dBmT, the vector {v0} .. {v0 + 3} that holds column M = {M} (frame, row, m - {v0})"),
         check_exact(B["dBmT"], castT(d, want), "dBmT = T([dBm | dabx | 0]), row Kcy 0 (frame, row, m)")]
    x = B["dBm"][:, Kcy, :M].double()
    dv = B["dvec"][2 * d.C:]
    w.append(check_bound(dv[:M], x.sum(0), S * EPS_ACC * x.abs().sum(0), "dvec dwbar = sum_s dBm[s][Kcy] (m)"))
    y = B["dabx"][:, Kcy].double()
    w.append(check_bound(dv[d.Mb], y.sum(), S * EPS_ACC * y.abs().sum(), "dvec dbcbar = sum_s dabx[s][Kcy]"))
    if d.Mb > M:
        w.append(check_zero(dv[M:d.Mb], "dvec dwbar padding M .. Mb keeps the cleared zero (m - M)"))
    return max(w)


def link_dA1(d, B):
    """dA1[s] = [dBm | dab][s] [Wc | bc]^T into L1, all Kcyb rows (moe_backward.cpp:365-371): M + 1 terms, fp32; row Kcy is the product of the
    zero row: exactly 0."""
    return check_product(B["L1"][:, :d.Kcyb, :d.N], B["dBmT"][:, :, :d.M + 1], B["WcK"][:, :d.M + 1].t(), d, out_T=False, k_terms=d.M + 1,
                         name="dA1 = [dBm | dab] [Wc | bc]^T (frame, row, n)")


def softmax_bwd_ref(d, a, da, text="plain"):
    """(ref, bound) of T(a (da - sum a da)) per element (bwd_kernels.hip:359-365, :386-405, the three texts share the arithmetic): DOT over n
    terms, `da - dot` (U32 at |da| + |dot|), the product (U32), the store"""
    a, da = a.double(), da.double()
    n = a.shape[-1]
    dot = (a * da).sum(-1, keepdim=True)
    e_dot = dot_bound(n, (a * da).abs().sum(-1, keepdim=True), per_lane={"reg4": 16, "reg16": 64}.get(text))
    ref = a * (da - dot)
    pre = a.abs() * (e_dot + U32 * (da.abs() + dot.abs())) + U32 * ref.abs() + TINY      # (TINY: a flushed denormal product, as nxn_ref's DS)
    return ref, _store(d, ref, pre, True)


def link_softmax_bwd(d, B):
    """k_softmax_rows_bwd -> dL1 = a (da - sum a da) from the stored A1y and dA1 (in L1); columns N .. Np exactly 0; rows with a = 0 (row
    Kcy, slot rows k >= K) exactly 0: their bound is 0."""
    N = d.N
    text = softmax_bwd_text(d.Np)
    ref, bnd = softmax_bwd_ref(d, B["A1y"][:, :, :N], B["L1"][:, :d.Kcyb, :N], text)
    return max(check_bound(B["dL1"][:, :d.Kcyb, :N], ref, bnd, f"dL1 = a (da - dot) [{text}] (frame, row, n)"),
               check_zero(B["dL1"][:, :d.Kcyb, N:], "dL1 columns N .. Np (frame, row, column - N)"))


def link_dRT(d, B):
    """dR[s]^T = (dL1[s] Wc)^T stored [m][kc] with row stride Kcyp (moe_backward.cpp:382-388): N terms, stored in T; the padding kc >= Kcy
    keeps the zero of the backward's one clearing launch."""
    w = check_product(B["dRT"][:, :, :d.Kcy], B["WcT"][:d.M, :d.N], B["dL1"][:, :d.Kcy, :d.N].transpose(1, 2), d, out_T=True, k_terms=d.N,
                      name="dRT = (dL1 Wc)^T (frame, m, row)")
    if d.Kcyp > d.Kcy:
        w = max(w, check_zero(B["dRT"][:, :, d.Kcy:], "dRT padding rows Kcy .. Kcyp (frame, m, row - Kcy)"))
    return w


def link_dWcK(d, B):
    """dWcK = A1^T [dBm | dab] (columns < M + 1) + dL1^T [R | qr | qb] (columns < M + 2), both over all S * Kcyb rows, the second accumulated on
    the first (moe_backward.cpp:372-396): one fp32 sum of 2 S Kcyb products + the accumulating add; columns M + 2 .. Mk keep the cleared 0."""
    S, N, M, R = d.S, d.N, d.M, d.S * d.Kcyb
    A = torch.cat([B["A1y"][:, :, :N].reshape(R, N), B["dL1"][:, :d.Kcyb, :N].reshape(R, N)]).double().t()      # (N, 2 R)
    dB = torch.zeros(R, M + 2, dtype=torch.float64, device=A.device)
    dB[:, :M + 1] = B["dBmT"][:, :, :M + 1].reshape(R, M + 1).double()
    Bm = torch.cat([dB, B["Rext"][:, :, :M + 2].reshape(R, M + 2).double()])
    w = check_product(B["dWcK"][:, :M + 2], A, Bm, d, out_T=False, k_terms=2 * R + 1, name="dWcK = A1^T [dBm | dab] + dL1^T [R | qr | qb] (n, m)", planes=2)
    if d.Mk > M + 2:
        w = max(w, check_zero(B["dWcK"][:, M + 2:], "dWcK columns M + 2 .. Mk (n, m - M - 2)"))
    return w


def link_dTW(d, B):
    """dTW[s][slot l rows k < K][group][own expert's columns] = ag[l]^T dZx (moe_backward.cpp:248-257; the third batch level puts slot l at
    sC3 = Kp * DZ + dgp: rows l Kp .., columns l dgp .. of every group): N terms, stored in T.  Everything else in dTW -- the other experts'
    columns, slot rows k >= K, the ones / dm1 rows -- keeps the zero of the backward's one clearing launch."""
    S, N, K, Kp, dgp = d.S, d.N, d.K, d.Kp, d.dgp
    ref = torch.zeros(S, d.KLT, d.g, d.E * dgp, dtype=torch.float64, device=B["dTW"].device)
    mag = torch.zeros_like(ref)
    Zw = B["Zw"].double()                                                                          # (S, N, g, E dgp)
    for l in range(d.El):                                                                          # (e_of_lat[l] = l: the latent experts come first)
        ag = B["ag"][l, :, :, :K].double().transpose(1, 2)                                         # (S, K, N)
        z = Zw[:, :, :, l * dgp:(l + 1) * dgp].permute(0, 2, 1, 3)                                 # (S, g, N, dgp)
        ref[:, l * Kp:l * Kp + K, :, l * dgp:(l + 1) * dgp] = (ag[:, None] @ z).permute(0, 2, 1, 3)
        mag[:, l * Kp:l * Kp + K, :, l * dgp:(l + 1) * dgp] = (ag.abs()[:, None] @ z.abs()).permute(0, 2, 1, 3)
    return check_bound(B["dTW"], ref, product_bound(ref, mag, out_bf16=d.bf16, k_terms=N) + planes_term(d, mag), "dTW = gate a^T dZx, zero elsewhere (frame, row, group, column)")


def link_dTT(d, B):
    """dTT[s][l] = aw[l]^T a[l], rows and columns k < K, row stride Kp (moe_backward.cpp:313-320): N terms, stored in T"""
    K = d.K
    aw, a = B["aw"][:, :, :, :K].double().permute(1, 0, 3, 2), B["a"][:, :, :, :K].double().permute(1, 0, 2, 3)      # (S, El, K, N), (S, El, N, K)
    ref, mag = aw @ a, aw.abs() @ a.abs()
    return check_bound(B["dTT"][:, :, :, :K], ref, product_bound(ref, mag, out_bf16=d.bf16, k_terms=d.N) + planes_term(d, mag), "dTT = (du3 a)^T a (frame, slot, k, k')")


def link_dqrqb(d, B):
    """k_dqrqb (bwd_kernels.hip:602-611): per (frame, row) dqr = sum_n dL1 bc[n], dqb = sum_n dL1 (DOT, N terms) into dqp; kk_hop1_vec (:619-657)
    adds them over the frames into dqp_fin (double, then four fp32 partials: FSUM, S terms)."""
    _, bc, _, _ = _params(d, B)
    R = d.S * d.Kcyb
    dL1 = B["dL1"][:, :d.Kcyb, :d.N].double()
    vec = torch.stack([bc.double(), torch.ones_like(bc, dtype=torch.float64)], 1)                  # (N, 2)
    part = B["dqp"][:2 * R].reshape(2, d.S, d.Kcyb)
    w = check_bound(part.permute(1, 2, 0), dL1 @ vec, dot_bound(d.N, dL1.abs() @ vec.abs()), "dqp = dL1 . [bc | 1] (frame, row, dqr / dqb)")
    fin = B["dqp"][2 * R:2 * R + 2 * d.Kcyb].reshape(2, d.Kcyb)
    p = part.double()
    return max(w, check_bound(fin, p.sum(1), d.S * EPS_ACC * p.abs().sum(1), "dqp_fin = sum over the frames of dqp (dqr / dqb, row)"))


def _abx(d, B):
    """the factor of drw's rows: ab = BmX[.., M] for the latent rows, scal[0] = mean(bc) for row Kcy (bwd_kernels.hip:543)"""
    abx = B["BmX"][:, :, d.M].double().clone()
    abx[:, d.Kcy] = B["scal"][0].double()
    return abx


def link_dvec(d, B):
    """drw, dbf in dvec after section 8: kk_dT0_dTy's row chunks + k_colsum_f32 (bwd_kernels.hip:525-546, :927), then kk_hop1_vec adds
    sum_kc T0[kc] dqr[kc] / dqb[kc] in place (:658-673): ONE sum of S Kcyb + Kcy terms (FSUM; + 2 for the chunk fold and the in-place add)."""
    C, R = d.C, d.S * d.Kcyb
    dTy = B["dTy"].double().reshape(R, C)
    abx = _abx(d, B).reshape(R)
    T0 = B["T0T"][:d.Kcy].double()
    fin = B["dqp"][2 * R:2 * R + 2 * d.Kcyb].reshape(2, d.Kcyb)[:, :d.Kcy].double()
    k = R + d.Kcy + 2
    ref = torch.stack([abx @ dTy + fin[0] @ T0, dTy.sum(0) + fin[1] @ T0])
    mag = torch.stack([abx.abs() @ dTy.abs() + fin[0].abs() @ T0.abs(), dTy.abs().sum(0) + fin[1].abs() @ T0.abs()])
    return check_bound(B["dvec"][:2 * C].reshape(2, C), ref, k * EPS_ACC * mag, "dvec drw / dbf (drw / dbf, c)")


def link_dT0(d, B):
    """dT0[kc] = sum_s (dT + dtbar / C) (kk_dT0_dTy, bwd_kernels.hip:499-523: double, then eight fp32 partials), y slots += dQ Wf^T
    (moe_backward.cpp:413-419: Cy terms, accumulated): one sum of S + Cy terms (+ 3: the division, the addition, the accumulating add).
    The x slots of an AVS v2 site receive a further product from X and are not held here."""
    Kcy, C = d.Kcy, d.C
    x = B["dT"][:, :Kcy].double()
    add = (B["dtbar"][:, :Kcy].double() / C)[..., None]
    ref0, mag0 = (x + add).sum(0), (x.abs() + add.abs()).sum(0)
    ref1, mag1 = product_ref(B["dQT"], B["WfT"].t())
    return check_bound(B["dT0"][:Kcy], ref0 + ref1, (d.S + d.Cy + 3) * EPS_ACC * (mag0 + mag1) + planes_term(d, mag1), "dT0[y slots] = sum_s (dT + dtbar / C) + dQ Wf^T (row, c)")


def link_dWf(d, B):
    """dWf = dTy^T V, then += T0^T dQ (moe_backward.cpp:348-354, :420-427): the whole sum from the stored operands, S Kcyb + Kcy terms + the
    accumulating add; dQ as stored in bf16 (dQT)."""
    R = d.S * d.Kcyb
    A = torch.cat([B["dTy"].reshape(R, d.C), B["T0T"][:d.Kcy]]).double().t()
    Bm = torch.cat([B["V"].reshape(R, d.Cy), B["dQT"]]).double()
    return check_product(B["dWf"], A, Bm, d, out_T=False, k_terms=R + d.Kcy + 1, name="dWf = dTy^T V + T0^T dQ (c, y)", planes=2)


def link_finalize(d, B):
    """kk_hop1_finalize (bwd_kernels.hip:678-709), the caller's gradients from the stored dWcK, dWf, dvec, dT0, dqp_fin, rw, bf:
    conv_w = dWcK[:, :M] + dwbar / N, conv_b = dWcK[:, M] + dbcbar / N (the division and the addition: U32 each), fc_w = dWf + drw[c] (U32),
    fc_b = dbf (a copy), my_tokens[k < K] = dT0 + dqr rw + dqb bf (ELEMENTWISE, r = 4).  check_bound demands finite values: the NaN prefill
    of the gradients is gone wherever a value belongs.  "grads": {state-dict name: tensor}."""
    _, _, _, bf = _params(d, B)
    G, N, M, C, R = B["grads"], d.N, d.M, d.C, d.S * d.Kcyb
    dv = B["dvec"].double()
    drw, dbf, dwbar, dbcbar = dv[:C], dv[C:2 * C], dv[2 * C:2 * C + M], dv[2 * C + d.Mb]
    dWcK = B["dWcK"].double()
    ref = dWcK[:, :M] + dwbar / N
    w = [check_bound(G["conv_adapter.weight"].reshape(N, M), ref, U32 * (dwbar / N).abs() + U32 * ref.abs(), "conv_adapter.weight gradient (n, m)")]
    ref = dWcK[:, M] + dbcbar / N
    w.append(check_bound(G["conv_adapter.bias"], ref, U32 * (dbcbar / N).abs() + U32 * ref.abs(), "conv_adapter.bias gradient (n)"))
    ref = B["dWf"].double() + drw[:, None]
    w.append(check_bound(G["fc.weight"], ref, U32 * ref.abs(), "fc.weight gradient = dWf + drw[c] (c, y)"))
    w.append(check_exact(G["fc.bias"], B["dvec"][C:2 * C], "fc.bias gradient = dbf (c)"))
    fin = B["dqp"][2 * R:2 * R + 2 * d.Kcyb].reshape(2, d.Kcyb).double()
    rw, bfd = B["rw"].double(), bf.double()
    for l in range(d.Ey):
        kc = torch.arange(l * d.Kp, l * d.Kp + d.K, device=dv.device)
        t0 = B["dT0"][kc].double()
        qr, qb = fin[0][kc][:, None] * rw, fin[1][kc][:, None] * bfd
        ref = t0 + qr + qb
        w.append(check_bound(G[d.tok_keys[l]], ref, 4 * U32 * (t0.abs() + qr.abs() + qb.abs()), f"{d.tok_keys[l]} gradient (k, c)"))
    # my_tokens gradients are written for rows k < K only: the rows a caller's (K, C) tensor does not have.  "grads_tail": {name: the NaN-filled
    # rows that lie directly behind the K rows handed to the library}
    for k, tail in (B.get("grads_tail") or {}).items():
        if not bool(torch.isnan(tail).all()):
            raise ProductMismatch(f"{k} gradient: {int((~torch.isnan(tail)).sum())} entries of the rows k >= K behind the tensor were written")
    return max(w)


# ---- the latent-on-X side of an AVS v2 site (moe_forward.cpp:141-161, moe_backward.cpp:429-463) -----------------------------------------------
# After a whole forward / backward of such a site L1, TV and dL1 hold the x-side values, Kcx rows per frame from the start of the buffer.
def _xview(d, t):
    return t.reshape(-1)[:d.S * d.Kcx * t.shape[-1]].reshape(d.S, d.Kcx, t.shape[-1])


def real_rows_x(d):
    return (torch.arange(d.Kcx) % d.Kp) < d.K


def link_L1x(d, B):
    """L1x[s] = T0x X[s]^T in fp32 (moe_forward.cpp:144-150): C terms"""
    return check_product(_xview(d, B["L1"])[:, :, :d.N], B["T0T"][d.Kcy:], B["X"].transpose(1, 2), d, out_T=False, k_terms=d.C, name="L1x = T0x X^T (frame, row, n)")


def link_softmax_x(d, B):
    """k_softmax_rows -> A1x (grp = valid = Kcx: no ybar row; slot rows k >= K exactly 0, columns N .. Np exactly 0)"""
    text = softmax_text(d.N, d.Np)
    A1, N = B["A1x"], d.N
    real = real_rows_x(d).to(A1.device)
    ref, bnd = softmax_ref(d, _xview(d, B["L1"])[:, real, :N], text)
    w = [check_bound(A1[:, real, :N], ref, bnd, f"A1x = softmax(L1x) [{text}] (frame, real row, n)"),
         check_zero(A1[:, :, N:], "A1x columns N .. Np (frame, row, column - N)")]
    if d.Kp > d.K:
        w.append(check_zero(A1[:, ~real], "A1x slot rows k >= K (frame, row, column)"))
    return max(w)


def link_zero_rows_y(d, B):
    """what survives of k_softmax_rows on the y side once L1 is overwritten: the exact zeros of A1y (columns N .. Np, row Kcy, slot rows
    k >= K).  (The values of the real rows have lost their logits; [Bm | ab] is still held against them.)"""
    A1 = B["A1y"]
    real = real_rows(d).to(A1.device)
    return max(check_zero(A1[:, :, d.N:], "A1y columns N .. Np (frame, row, column - N)"),
               check_zero(A1[:, ~real], "A1y row Kcy and slot rows k >= K (frame, row, column)"))


def link_TVx(d, B):
    """TVx[s] = A1x[s] X[s] in fp32 (moe_forward.cpp:153-159): N terms"""
    return check_product(_xview(d, B["TV"]), B["A1x"][:, :, :d.N], B["X"], d, out_T=False, k_terms=d.N, name="TVx = A1x X (frame, row, c)")


def link_finish_Tx(d, B):
    """k_finish_T, src = 1 (fwd_kernels.hip:718-753): Text x slots = T(T0 + TV) (one addition), Tsum of the rows as stored, slot rows k >= K 0"""
    S, C, K, Kp = d.S, d.C, d.K, d.Kp
    Text = B["Text"][:, d.Kcy:d.KL].reshape(S, d.Ex, Kp, C)
    Tsum = B["Tsum"][:, :, d.Kcy:d.KL].reshape(2, S, d.Ex, Kp)
    tok = torch.stack([B[k].double() for k in d.tok_keys[d.Ey:]])[None]
    tv = _xview(d, B["TV"]).reshape(S, d.Ex, Kp, C)[:, :, :K].double()
    ref = tok + tv
    w = [check_bound(Text[:, :, :K], ref, _store(d, ref, U32 * (tok.abs() + tv.abs()), True), "Text x slots = T(T0 + TVx) (frame, slot, k, c)")]
    st = Text[:, :, :K].double()
    for pl, (r, nm) in enumerate(((st.sum(-1), "sum"), ((st * st).sum(-1), "sum of squares"))):
        w.append(check_bound(Tsum[pl][:, :, :K], r, 2 * U32 * r.abs(), f"Tsum row {nm} of the x slots as stored (frame, slot, k)"))
    if Kp > K:
        w.append(check_zero(Text[:, :, K:], "Text x-slot rows k >= K (frame, slot, k - K, c)"))
        w.append(check_zero(Tsum[:, :, :, K:], "Tsum x-slot rows k >= K (plane, frame, slot, k - K)"))
    return max(w)


def link_dA1x(d, B):
    """dA1x[s] = dTx[s] X[s]^T into L1 (moe_backward.cpp:432-438): C terms, fp32"""
    return check_product(_xview(d, B["L1"])[:, :, :d.N], B["dTx"], B["X"].transpose(1, 2), d, out_T=False, k_terms=d.C, name="dA1x = dTx X^T (frame, row, n)")


def link_softmax_bwd_x(d, B):
    """k_softmax_rows_bwd with the transposed copy (moe_backward.cpp:446-448; the only user of out_t): dL1x per element from the stored A1x
    and dA1x; dL1xT[s n][row] holds the SAME bits as dL1x[s][row][n]; its padding rows Kcx .. Kcxp keep the MEMSET0 in front of the launch."""
    N = d.N
    text = softmax_bwd_text(d.Np)
    ref, bnd = softmax_bwd_ref(d, B["A1x"][:, :, :N], _xview(d, B["L1"])[:, :, :N], text)
    dL1 = _xview(d, B["dL1"])
    w = [check_bound(dL1[:, :, :N], ref, bnd, f"dL1x = a (da - dot) [{text}] (frame, row, n)"),
         check_zero(dL1[:, :, N:], "dL1x columns N .. Np (frame, row, column - N)"),
         check_exact(B["dL1xT"][:, :, :d.Kcx], dL1[:, :, :N].transpose(1, 2), "dL1xT = dL1x transposed, the same bits (frame, n, row)")]
    if d.Kcxp > d.Kcx:
        w.append(check_zero(B["dL1xT"][:, :, d.Kcx:], "dL1xT padding rows Kcx .. Kcxp (frame, n, row - Kcx)"))
    return max(w)


def link_dT0x(d, B):
    """dT0[x slots] = sum_s (dT + dtbar / C) + sum_{s, n} dL1x^T X (bwd_kernels.hip:499-523, moe_backward.cpp:449-455): one sum of S + S N
    terms (+ 3 as link_dT0)"""
    Kcy, C = d.Kcy, d.C
    x = B["dT"][:, Kcy:].double()
    add = (B["dtbar"][:, Kcy:].double() / C)[..., None]
    ref0, mag0 = (x + add).sum(0), (x.abs() + add.abs()).sum(0)
    A = B["dL1xT"][:, :, :d.Kcx].reshape(d.NT, d.Kcx).double().t()
    ref1, mag1 = product_ref(A, B["X"].reshape(d.NT, C))
    return check_bound(B["dT0"][Kcy:], ref0 + ref1, (d.S + d.NT + 3) * EPS_ACC * (mag0 + mag1) + planes_term(d, mag1), "dT0[x slots] (row, c)")


def link_finalize_x(d, B):
    """kk_hop1_finalize on the latent-on-X slots: my_tokens[k < K] = dT0 (a copy, bwd_kernels.hip:703-706), nothing behind row K"""
    w = 0.0
    for l in range(d.Ey, d.El):
        w = max(w, check_exact(B["grads"][d.tok_keys[l]], B["dT0"][l * d.Kp:l * d.Kp + d.K], f"{d.tok_keys[l]} gradient = dT0 rows (k, c)"))
    return w


FORWARD_X = {
    "L1x": ("L1x = T0x X^T", "gemm", link_L1x),
    "softmax_x": ("k_softmax_rows: A1x", "k_softmax_rows", link_softmax_x),
    "A1y_zeros": ("A1y: the exact zeros of its padding columns and rows", "k_softmax_rows", link_zero_rows_y),
    "TVx": ("TVx = A1x X", "gemm", link_TVx),
    "finish_Tx": ("k_finish_T(src = 1): Text x slots, Tsum", "finish_T", link_finish_Tx),
}
BACKWARD_X = {
    "dA1x": ("dA1x = dTx X^T", "gemm", link_dA1x),
    "softmax_bwd_x": ("k_softmax_rows_bwd with the transposed copy: dL1x, dL1xT", "k_softmax_rows_bwd", link_softmax_bwd_x),
    "dT0x": ("dT0[x slots]", "gemm", link_dT0x),
    "finalize_x": ("k_hop1_finalize: my_tokens of the latent-on-X experts", "k_hop1_finalize", link_finalize_x),
}
# the y-side links whose operands survive the whole forward / backward of such a site (the others read L1 / TV / dL1, which hold the x side)
V2_FORWARD_Y = ("prep", "const_rows", "Qx", "qrqb", "BmX", "BmX_pad", "TT", "TW")
V2_BACKWARD_Y = ("dTW", "dTT", "finish_dT", "dV", "prep_dBm", "dvec", "dT0", "dWf", "finalize")


# tag -> (what, the kernel family the profiler must have seen, link)
FORWARD = {
    "prep": ("k_prep_all remap part: WcK, WcT, WfT, rw, wbar, scal, T0T", "k_prep_all", link_prep),
    "const_rows": ("k_prep_all: ones / dm1 row of Text and Tsum", "k_prep_all", link_const_rows),
    "Qx": ("Qx = T0 Wf", "gemm", link_Qx),
    "qrqb": ("k_qrqb_fill: qrqb, Rext extension columns and row Kcy, BmX row Kcy", "k_qrqb_fill", link_qrqb),
    "L1": ("L1 = [R | qr | qb][Wc | bc | 1]^T", "frames", link_L1),
    "softmax": ("k_softmax_rows: A1y", "k_softmax_rows", link_softmax),
    "BmX": ("[Bm | ab] = A1 [Wc | bc]", "frames", link_BmX),
    "BmX_pad": ("BmX columns M + 1 .. Mb", "frames", link_BmX_pad),
    "TV": ("TV = V Wf^T", "gemm", link_TV),
    "finish_T": ("k_finish_T: Text y slots, Tsum, rin[:, C:]", "finish_T", link_finish_T),
    "TT": ("TT = T T^T", "gemm", link_TT),
    "TW": ("TW = Text Wt^T", "gemm", link_TW),
}
BACKWARD = {
    "dTW": ("dTW = gate a^T dZx in the third-batch-level layout", "gemm", link_dTW),
    "dTT": ("dTT = (du3 a)^T a", "gemm", link_dTT),
    "finish_dT": ("k_finish_dT: dTy, dTx, dabx", "finish_dT", link_finish_dT),
    "dV": ("dV = dTy Wf", "gemm", link_dV),
    "prep_dBm": ("k_prep_dBm: dBmT, dwbar, dbcbar", "prep_dBm", link_prep_dBm),
    "dA1": ("dA1 = [dBm | dab][Wc | bc]^T", "frames", link_dA1),
    "softmax_bwd": ("k_softmax_rows_bwd: dL1", "k_softmax_rows_bwd", link_softmax_bwd),
    "dRT": ("dR^T = (dL1 Wc)^T", "frames", link_dRT),
    "dWcK": ("dWcK, both accumulated products", "gemm", link_dWcK),
    "dqrqb": ("k_dqrqb: dqp and dqp_fin", "k_dqrqb", link_dqrqb),
    "dvec": ("drw, dbf through their final values in dvec", "k_hop1_finalize", link_dvec),
    "dT0": ("dT0 = sum_s (dT + dtbar / C), y slots += dQ Wf^T", "gemm", link_dT0),
    "dWf": ("dWf = dTy^T V + T0^T dQ", "gemm", link_dWf),
    "finalize": ("k_hop1_finalize: conv_w, conv_b, fc_w, fc_b, my_tokens gradients", "k_hop1_finalize", link_finalize),
}
LINKS = {**FORWARD, **BACKWARD, **FORWARD_X, **BACKWARD_X}


def _pf_shape(d, link):
    return {"L1": (d.Kcy, d.N, d.M + 2), "BmX": (d.Kcy, d.M + 1, d.N), "dA1": (d.Kcyb, d.N, d.M + 1), "dRT": (d.Kcy, d.M, d.N)}[link]


def stream_serves(d, link):
    """launch_gemm tries the B-stationary streaming kernel BEFORE launch_gemm_frames (gemm.hip:1138), and it takes a per-frame product of the
    chain where its own conditions hold (gemm_stream.hip:591-599: bf16, row-major C, >= 256 rows in all, K <= 384, >= 64 rows per frame,
    an output width that is a multiple of 4; the paddings of the plan satisfy its alignment tests) and one of its one-segment
    configurations fits (:720-726: K steps of 32 and column tiles of 16).  -> the profiler name of that configuration, or None"""
    M_, N_, K_ = _pf_shape(d, link)
    if not d.bf16 or link == "dRT" or M_ * d.S < 256 or K_ > 384 or N_ > 768 or (d.S > 1 and M_ < 64) or N_ % 4:
        return None
    ks, tiles = -(-K_ // 32), -(-N_ // 16)
    for name, kmax, tmax in (("gemm_stream_k64_n192", 2, 12), ("gemm_stream_k160_n64", 5, 4), ("gemm_stream_k160_n384", 5, 24),
                             ("gemm_stream_k384_n128", 12, 8), ("gemm_stream_k384_n144", 12, 9)):
        if ks <= kmax and tiles <= tmax:
            return name
    return None


def frames_serves(d, link):
    """whether launch_gemm_frames takes the product (frame_gemm.hip:336-350: bf16, >= 32 frames, output width >= 64, not both K > 256 and
    N > 224; every other condition holds by the plan's paddings) -> (served, "plain" | "long" | "long T" | "T", why not)"""
    M_, N_, K_ = _pf_shape(d, link)
    tr = link == "dRT"
    why = []
    if stream_serves(d, link):
        why.append(f"{stream_serves(d, link)} takes it first")
    if not d.bf16:
        why.append("an fp32 site")
    if d.S < 32:
        why.append("fewer than 32 frames")
    if N_ < 64:
        why.append(f"output width {N_} < 64")
    if K_ > 256 and N_ > 224:
        why.append(f"K = {K_} > 256 and N = {N_} > 224")
    if M_ > 64 and (tr or link != "dA1"):
        why.append(f"{M_} rows per frame and not one tall matrix")
    form = ("long" if K_ > 256 else "plain") + (" T" if tr else "")
    return not why, form, ", ".join(why)


# ---- input families -------------------------------------------------------------------------------------------------------------------------
FAMILIES = ("default", "flat", "peaked")
TOKEN_SCALE = {"default": 1.0, "flat": 0.02, "peaked": 2.0}
BOOST = 3.0


def boosted_columns(N):
    """the keys whose conv_adapter rows the peaked family scales by BOOST so that row maxima fall there: column 0, the last column, and one
    more inside the last partial 4-vector where N % 4 != 0 (N % 4 == 1: that vector IS the last column)"""
    cols = {0, N - 1}
    if N % 4 >= 2:
        cols.add(N - N % 4)
    return sorted(cols)


def apply_family(P, family, cfg):
    """The default draw (0.3 randn, U(0, 1) tokens) leaves the hop-1 logits nearly flat; L1 is linear in my_tokens, so scaling the tokens
    scales every row's span: flat -> every key counts, peaked -> most of a row's mass on a few keys.  peaked also scales the conv_adapter
    rows (weight and bias) of boosted_columns, which puts row maxima into the first column, the last one and the last partial vector."""
    assert family in FAMILIES
    P = dict(P)
    for k in list(P):
        if k.endswith(".my_tokens"):
            P[k] = P[k] * TOKEN_SCALE[family]
    if family == "peaked":
        cols = boosted_columns(cfg.Nx)
        W, b = P["conv_adapter.weight"].clone(), P["conv_adapter.bias"].clone()
        W[cols] *= BOOST
        b[cols] *= BOOST
        P["conv_adapter.weight"], P["conv_adapter.bias"] = W, b
    return P


def family_X(X, family, cfg):
    """the X of a family: the peaked family scales the tokens boosted_columns of X by BOOST, which does for the logits of the latent self
    attention on X (L1x = T0x X^T) what the conv_adapter rows do for the cross-modal ones; a site without that attention has no use for it"""
    if family == "peaked" and cfg.self_attn == "v2":
        X = X.clone()
        X[:, boosted_columns(cfg.Nx)] *= BOOST
    return X


def check_family(d, L1, family):
    """the properties of the stored L1 the family is there for (asserted, never skipped).  At an AVS v2 site the stored L1 is the x side's."""
    if family == "default":
        return
    if d.Kcx:
        p = _xview(d, L1)[:, real_rows_x(d).to(L1.device), :d.N].double()
    else:
        p = L1[:, :d.Kcyb][:, real_rows(d).to(L1.device), :d.N].double()
    span = p.max(-1).values - p.min(-1).values
    if family == "flat":
        assert float(span.max()) < 0.5, f"flat: a row of L1 spans {float(span.max()):.3g} >= 0.5"
        return
    share = float((span > 8).double().mean())
    assert share >= 0.5, f"peaked: only {share:.2f} of the real rows span more than 8"
    am = p.argmax(-1).reshape(-1)
    assert bool((am == 0).any()) and bool((am == d.N - 1).any()), "peaked: no row maximum in column 0 / in the last column"
    if d.N % 4:
        assert bool((am >= d.N - d.N % 4).any()), "peaked: no row maximum in the last partial 4-vector"
