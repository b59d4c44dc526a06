// Where the tensors of one MoEAdapter site lie, as matrix views (gemm.h: Mat): the stored shape, leading dimension, frame stride and element
// type of every workspace buffer (moe_plan.h: AVMOE_BUFFERS) and caller tensor that is an operand of a product, stated ONCE.  The products of
// moe_forward.cpp / moe_backward.cpp / mha_frames.hip are built from these views and state no stride of their own.
// `sv` / `sc`: base of the region the buffer lives in (saved / scratch); a null base gives a null view (shape-only queries).
// A frame is one sample s of the site (the first batch level of a per-frame product); NT = S * N tokens.
#pragma once
#include "gemm.h"
#include "moe_plan.h"

namespace avmoe {
namespace views {

inline Mat view(const void* base, size_t off, int esz, long rows, long cols, long ld, long s1 = 0, long s2 = 0) {
  Mat m; m.p = base ? (const char*)base + off : nullptr; m.esz = esz; m.rows = (int)rows; m.cols = (int)cols; m.ld = ld; m.s1 = s1; m.s2 = s2;
  return m;
}

// ---- the caller's token tensors (element type T) ----
inline Mat tokens_x(const Dims& d, const void* p) { return view(p, 0, d.esz, d.N, d.C, d.C, (long)d.N * d.C); }          // X, out, dOut, dX: (S, N, C)
inline Mat tokens_y(const Dims& d, const void* p) { return view(p, 0, d.esz, d.M, d.Cy, d.Cy, (long)d.M * d.Cy); }       // Y, dY: (S, M, Cy)

// ---- weights-derived operands ----
inline Mat WcK(const Plan& pl, const char* sv) { const Dims& d = pl.d; return view(sv, pl.o_WcK, d.esz, d.N, d.M + 2, d.Mk); }      // [n][m | bc | 1]
inline Mat WcT(const Plan& pl, const char* sv) { const Dims& d = pl.d; return view(sv, pl.o_WcT, d.esz, d.M + 1, d.N, d.Np); }      // [m | bc-row][n]
inline Mat WfT(const Plan& pl, const char* sv) { const Dims& d = pl.d; return view(sv, pl.o_WfT, d.esz, d.C, d.Cy, d.Cy); }         // fc.weight (C, Cy) in element type T: NOT a transpose
inline Mat T0T(const Plan& pl, const char* sv) { const Dims& d = pl.d; return view(sv, pl.o_T0T, d.esz, d.KL, d.C, d.C); }          // stacked my_tokens (KL, C) in element type T: the y slots, then the x slots
// [i][e][jp][c] = Wd * gamma_b: per group i (second level) the (E * dgp, Cg) rows of all experts
inline Mat Wt(const Plan& pl, const char* sv) { const Dims& d = pl.d; return view(sv, pl.o_Wt, d.esz, d.E * d.dgp, d.Cg, d.Cg, 0, (long)d.E * d.dgp * d.Cg); }
inline Mat dWt(const Plan& pl, const char* sc) { const Dims& d = pl.d; return view(sc, pl.o_dWt, 4, d.E * d.dgp, d.Cg, d.Cg, 0, (long)d.E * d.dgp * d.Cg); }
// ---- hop 1 (Kcyb rows per frame: the Kcy latent rows, then the wbar / ybar row) ----
inline Mat Qx(const Plan& pl, const char* sv) { const Dims& d = pl.d; return view(sv, pl.o_Qx, d.esz, d.Kcy, d.Cy, d.Cy); }          // T0 Wf
inline Mat Rext(const Plan& pl, const char* sv) { const Dims& d = pl.d; return view(sv, pl.o_Rext, d.esz, d.Kcyb, d.M + 2, d.Mk, (long)d.Kcyb * d.Mk); }      // [R | qr | qb] ; last row 0
inline Mat A1y(const Plan& pl, const char* sv) { const Dims& d = pl.d; return view(sv, pl.o_A1y, d.esz, d.Kcyb, d.N, d.Np, (long)d.Kcyb * d.Np); }            // softmax_n ; last row 0
inline Mat BmX(const Plan& pl, const char* sv) { const Dims& d = pl.d; return view(sv, pl.o_BmX, d.esz, d.Kcyb, d.M + 1, d.Mb, (long)d.Kcyb * d.Mb); }        // [A1 Wc | ab] ; last row wbar
inline Mat V(const Plan& pl, const char* sv) { const Dims& d = pl.d; return view(sv, pl.o_V, d.esz, d.Kcyb, d.Cy, d.Cy, (long)d.Kcyb * d.Cy); }
inline Mat A1x(const Plan& pl, const char* sv) { const Dims& d = pl.d; return view(sv, pl.o_A1x, d.esz, d.Kcx, d.N, d.Np, (long)d.Kcx * d.Np); }
// T[s] rows (El slots of Kp rows, K of them used) + ones row + dm1 row
inline Mat Text(const Plan& pl, const char* sv) { const Dims& d = pl.d; return view(sv, pl.o_Text, d.esz, d.KLT, d.C, d.C, (long)d.KLT * d.C); }
inline Mat TT(const Plan& pl, const char* sv) { const Dims& d = pl.d; return view(sv, pl.o_TT, 4, d.El * d.K, d.K, d.K, (long)d.El * d.K * d.K); }           // [s][slot] T T^T, (K, K) each
inline Mat L1(const Plan& pl, const char* sc, int rows) { const Dims& d = pl.d; return view(sc, pl.o_L1, 4, rows, d.N, d.Np, (long)rows * d.Np); }           // L1 ; dA1 in the backward: `rows` (Kcyb | Kcx) per frame
inline Mat TV(const Plan& pl, const char* sc, int rows) { const Dims& d = pl.d; return view(sc, pl.o_TV, 4, rows, d.C, d.C, (long)rows * d.C); }
// ---- per token; the DZ-wide rows are [group][expert][dgp] ----
inline Mat dz_rows(const Dims& d, const char* base, size_t off, int esz, int rows) { return view(base, off, esz, rows, d.DZ, d.DZ, (long)rows * d.DZ); }
inline Mat TW(const Plan& pl, const char* sv) { return dz_rows(pl.d, sv, pl.o_TW, 4, pl.d.KLT); }                       // Text rows through Wt
inline Mat dTW(const Plan& pl, const char* sc) { return dz_rows(pl.d, sc, pl.o_dTW, pl.d.esz, pl.d.KLT); }
inline Mat Z(const Plan& pl, const char* sv) { return dz_rows(pl.d, sv, pl.o_Z, pl.d.zsz, pl.d.N); }                    // Zx then z (in place)
inline Mat ZR(const Plan& pl, const char* sv) { return dz_rows(pl.d, sv, pl.o_ZR, 4, pl.d.N); }                         // xr through Wt
inline Mat dZR(const Plan& pl, const char* sc) { return dz_rows(pl.d, sc, pl.o_dZR, pl.d.esz, pl.d.N); }
inline Mat Zp(const Plan& pl, const char* sc) { return dz_rows(pl.d, sc, pl.o_Zp, pl.d.esz, pl.d.N); }                  // z'
inline Mat Zw(const Plan& pl, const char* sc) { return dz_rows(pl.d, sc, pl.o_Zw, pl.d.esz, pl.d.N); }                  // dSoo z' ; later dZx
inline Mat L2(const Plan& pl, const char* sv) { const Dims& d = pl.d; return view(sv, pl.o_L2, 4, d.N, d.KL, d.KL, (long)d.N * d.KL); }
inline Mat L2g(const Plan& pl, const char* sc) { const Dims& d = pl.d; return view(sc, pl.o_L2g, 4, d.N, d.KL, d.KL, (long)d.N * d.KL, (long)d.NT * d.KL); }  // per-group partial hop-2 logits [group][token][KL]
// a / aw / ag: one plane [token][Kp] per latent slot, Dims::aL apart
inline Mat lat_plane(const Dims& d, const char* base, size_t off) { return view(base, off, d.esz, d.N, d.K, d.Kp, (long)d.N * d.Kp); }
inline Mat a(const Plan& pl, const char* sv) { return lat_plane(pl.d, sv, pl.o_a); }
inline Mat aw(const Plan& pl, const char* sc) { return lat_plane(pl.d, sc, pl.o_aw); }                                  // du3 * a
inline Mat ag(const Plan& pl, const char* sc) { return lat_plane(pl.d, sc, pl.o_ag); }                                  // gate_lat * a
// (g * E) Gram matrices (dgp, dgp), one under the other
inline Mat gram(const Dims& d, const char* base, size_t off) { return view(base, off, 4, (long)d.g * d.E * d.dgp, d.dgp, d.dgp); }
inline Mat Szz(const Plan& pl, const char* sv) { return gram(pl.d, sv, pl.o_Szz); }
inline Mat dGq(const Plan& pl, const char* sc) { return gram(pl.d, sc, pl.o_dGq); }
// post GEMM: per group KPp columns (KP used) of Apost's token rows, per group Cg rows of Bpost
inline Mat Apost(const Plan& pl, const char* sv) { const Dims& d = pl.d; return view(sv, pl.o_Apost, d.esz, d.NT, (long)d.g * d.KPp, (long)d.g * d.KPp); }
inline Mat Bpost(const Plan& pl, const char* sv) { const Dims& d = pl.d; return view(sv, pl.o_Bpost, d.esz, d.C, d.KPp, d.KPp); }
inline Mat dBp(const Plan& pl, const char* sc) { const Dims& d = pl.d; return view(sc, pl.o_dBp, 4, d.C, d.KPp, d.KPp); }
inline Mat dAp(const Plan& pl, const char* sc) { const Dims& d = pl.d; return view(sc, pl.o_dAp, 4, d.NT, (long)d.g * d.KPp, (long)d.g * d.KPp); }
// ... in its split form (sites that keep z in bf16): the buffer holds the E * dgp bottleneck columns per (token, group) in bf16, as rows of
// their own -- not what its table entry sizes -- and dApx the 3 E scalar columns in fp32
inline Mat dAp_split(const Plan& pl, const char* sc) { const Dims& d = pl.d; return view(sc, pl.o_dAp, 2, d.NT, (long)d.g * d.E * d.dgp, (long)d.g * d.E * d.dgp); }
// ---- AVVP N x N block ----
inline Mat att(const Plan& pl, const char* sv) { const Dims& d = pl.d; return view(sv, pl.o_att, d.esz, d.N, d.N, d.Np, (long)d.N * d.Np); }      // softmax_rows(X X^T), nxc frames
inline Mat dSc(const Plan& pl, const char* sc) { const Dims& d = pl.d; return view(sc, pl.o_dSc, d.esz, d.N, d.N, d.Np, (long)d.N * d.Np); }
inline Mat xr(const Plan& pl, const char* sv, int slot) { const Dims& d = pl.d; return tokens_x(d, sv ? sv + pl.o_xr + (size_t)slot * d.NT * d.C * d.esz : nullptr); }   // att^T X | MHA_e(X) - X per slot
inline Mat nyt(const Plan& pl, const char* sc) { const Dims& d = pl.d; return view(sc, pl.o_nyt, 4, d.N, d.C, d.C, (long)d.N * d.C); }            // y = att dxr of a chunk
inline Mat dxr(const Plan& pl, const char* sc) { return tokens_x(pl.d, sc ? sc + pl.o_dxr : nullptr); }
// ---- backward ----
inline Mat dL2x(const Plan& pl, const char* sc) { const Dims& d = pl.d; return view(sc, pl.o_dL2x, d.esz, d.N, d.KLT, d.KLp, (long)d.N * d.KLp); }            // [dL2 | dsx | 1]
inline Mat dTT(const Plan& pl, const char* sc) { const Dims& d = pl.d; return view(sc, pl.o_dTT, d.esz, d.El * d.K, d.K, d.Kp, (long)d.El * d.K * d.Kp); }     // [s][slot] (K, K), rows padded to Kp
inline Mat dT(const Plan& pl, const char* sc) { const Dims& d = pl.d; return view(sc, pl.o_dT, 4, d.KL, d.C, d.C, (long)d.KL * d.C); }
inline Mat dTy(const Plan& pl, const char* sc) { const Dims& d = pl.d; return view(sc, pl.o_dTy, d.esz, d.Kcyb, d.C, d.C, (long)d.Kcyb * d.C); }              // y-slots of dT + dm2 row, in T
inline Mat dTx(const Plan& pl, const char* sc) { const Dims& d = pl.d; return view(sc, pl.o_dTx, d.esz, d.Kcx, d.C, d.C, (long)d.Kcx * d.C); }
inline Mat dT0(const Plan& pl, const char* sc) { const Dims& d = pl.d; return view(sc, pl.o_dT0, 4, d.KL, d.C, d.C); }
inline Mat dV(const Plan& pl, const char* sc) { const Dims& d = pl.d; return view(sc, pl.o_dV, d.esz, d.Kcyb, d.Cy, d.Cy, (long)d.Kcyb * d.Cy); }
inline Mat dBm(const Plan& pl, const char* sc) { const Dims& d = pl.d; return view(sc, pl.o_dBm, 4, d.Kcyb, d.M + 1, d.Mb, (long)d.Kcyb * d.Mb); }
inline Mat dBmT(const Plan& pl, const char* sc) { const Dims& d = pl.d; return view(sc, pl.o_dBmT, d.esz, d.Kcyb, d.M + 1, d.Mb, (long)d.Kcyb * d.Mb); }      // [dBm | dab] in element type T: NOT a transpose
inline Mat dL1(const Plan& pl, const char* sc, int rows) { const Dims& d = pl.d; return view(sc, pl.o_dL1, d.esz, rows, d.N, d.Np, (long)rows * d.Np); }
inline Mat dWcK(const Plan& pl, const char* sc) { const Dims& d = pl.d; return view(sc, pl.o_dWcK, 4, d.N, d.M + 2, d.Mk); }
inline Mat dRT(const Plan& pl, const char* sc) { const Dims& d = pl.d; return view(sc, pl.o_dRT, d.esz, d.M, d.Kcy, d.Kcyp, (long)d.M * d.Kcyp); }            // dR[s] TRANSPOSED: stored [m][kc]
inline Mat dL1xT(const Plan& pl, const char* sc) { const Dims& d = pl.d; return view(sc, pl.o_dL1xT, d.esz, d.N, d.Kcx, d.Kcxp, (long)d.N * d.Kcxp); }        // dL1x[s] TRANSPOSED: stored [token][kc]
inline Mat dQT(const Plan& pl, const char* sc) { const Dims& d = pl.d; return view(sc, pl.o_dQT, d.esz, d.Kcy, d.Cy, d.Cy); }                                  // dQ (Kcy, Cy) in element type T: NOT a transpose
inline Mat dWf(const Plan& pl, const char* sc) { const Dims& d = pl.d; return view(sc, pl.o_dWf, 4, d.C, d.Cy, d.Cy); }
// ---- AVS "v1" MultiheadAttention across the frames; the tensors kept for the backward once per xr slot ----
inline const char* slot_at(const char* base, size_t off, size_t slot_bytes, int slot) { return base ? base + off + slot * slot_bytes : nullptr; }
inline Mat mWin(const Plan& pl, const char* sv, int slot) { const Dims& d = pl.d; return view(slot_at(sv, pl.o_mWin, (size_t)3 * d.C * d.C * d.esz, slot), 0, d.esz, 3 * d.C, d.C, d.C); }      // in_proj_weight (3 C, C) in element type T
inline Mat mWout(const Plan& pl, const char* sv, int slot) { const Dims& d = pl.d; return view(slot_at(sv, pl.o_mWout, (size_t)d.C * d.C * d.esz, slot), 0, d.esz, d.C, d.C, d.C); }           // out_proj.weight (C, C) in element type T
inline Mat qkv_rows(const Dims& d, const char* p) { return view(p, 0, d.esz, d.N, 3 * d.C, 3 * d.C, (long)d.N * 3 * d.C); }                                          // [s][n][q | k | v]
inline Mat mQKV(const Plan& pl, const char* sv, int slot) { return qkv_rows(pl.d, slot_at(sv, pl.o_mQKV, (size_t)pl.d.NT * 3 * pl.d.C * pl.d.esz, slot)); }
inline Mat mdQKV(const Plan& pl, const char* sc) { return qkv_rows(pl.d, slot_at(sc, pl.o_mdQKV, 0, 0)); }
inline Mat mO(const Plan& pl, const char* sv, int slot) { return tokens_x(pl.d, slot_at(sv, pl.o_mO, (size_t)pl.d.NT * pl.d.C * pl.d.esz, slot)); }              // heads concatenated, before out_proj
inline Mat mdO(const Plan& pl, const char* sc) { return tokens_x(pl.d, slot_at(sc, pl.o_mdO, 0, 0)); }
// a (S, N, width) tensor per token n (first level): the (S, width) matrix of its frames -- the heads are its column groups
inline Mat per_token(const Dims& d, const Mat& v) { Mat m = v; m.rows = d.S; m.ld = v.s1; m.s1 = v.ld; return m; }
// [n][h][s][s']: per token the (S, S) matrices of its H heads one under the other, rows padded to Sp
inline Mat head_mats(const Dims& d, const char* base, size_t off, int esz) { return view(base, off, esz, (long)d.H * d.S, d.S, d.Sp, (long)d.H * d.S * d.Sp); }
inline Mat mP(const Plan& pl, const char* sv, int slot) { const Dims& d = pl.d; return head_mats(d, sv, pl.o_mP + slot * (size_t)d.N * d.H * d.S * d.Sp * d.esz, d.esz); }      // softmax
inline Mat mPd(const Plan& pl, const char* sv, int slot) { const Dims& d = pl.d; return head_mats(d, sv, pl.o_mPd + slot * (size_t)d.N * d.H * d.S * d.Sp * d.esz, d.esz); }    // after dropout
inline Mat mSc(const Plan& pl, const char* sc) { return head_mats(pl.d, sc, pl.o_mSc, 4); }                                                                          // scores ; d Pd in the backward
inline Mat mdS(const Plan& pl, const char* sc) { return head_mats(pl.d, sc, pl.o_mdS, pl.d.esz); }

}  // namespace views
}  // namespace avmoe
