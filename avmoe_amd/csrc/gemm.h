// Generic strided / batched MFMA GEMM engine for gfx950 (MI355X).
//
// Every wide contraction of the adapter path -- remap, latent-token attention hops, grouped
// down/up projections, their input- and weight-gradient products -- is expressed as one call of
// this engine (see DESIGN.md "bottleneck-space algebra"), so the full-width token tensors are only
// ever touched by MFMA tiles.
//
//   C[b][i][j] (+)= alpha * sum_k A[b][i][k] * B[b][j][k]   (+ row_scale[b][i] * D[b][i][j])
//
// Operand layouts (per operand):
//   K_MAJOR  : k is the contiguous index  (element (i,k) at  i*ld + k)
//   MN_MAJOR : i is the contiguous index  (element (i,k) at  k*ld + i)   -- read through LDS with
//              ds_read_b64_tr_b16 (bf16) / strided ds_read_b32 (f32)
// C is addressed with explicit (sCi, sCj) strides; one of them must be 1.
//
// Contract for callers (checked in gemm.hip::launch_gemm, of each of the up to four K segments of a product):
//   * base pointers 16-byte aligned, ld * sizeof(T) and batch strides * sizeof(T) multiples of 16
//   * K_MAJOR operands: every row readable (finite) up to roundup(K, 16/sizeof(T)) elements; at
//     least one of the two operands is ZERO in that padding
//   * MN_MAJOR operands: every k-row readable up to roundup(M or N, 16/sizeof(T)) elements
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "common.h"

namespace avmoe {

enum GemmDtype { GEMM_F32 = 0, GEMM_BF16 = 1 };
enum GemmLayout { K_MAJOR = 0, MN_MAJOR = 1 };

inline int gemm_dtype_bytes(int dtype) { return dtype == GEMM_BF16 ? 2 : 4; }

// A tensor as a batch of row-major matrices: where one operand of a product lies.  `rows` x `cols` with leading dimension `ld` is the STORED
// shape of one matrix; `s1` steps from frame to frame (the first batch level of a product), `s2` along its second batch level; `t` = the
// product reads the transpose of what is stored.  Strides and `ld` in elements of `esz` bytes.  The site's tensors are stated once, in
// site_views.h; a call site cuts and regroups them with the methods below and binds them with GemmArgs::product, which derives M / N / K,
// layouts, leading dimensions and strides from them and refuses operands that do not fit each other.
struct Mat {
  const void* p = nullptr;
  int esz = 0;                          // 0: an invalid view (flat() of frames that do not abut) -- every binding refuses it
  int rows = 0, cols = 0;
  long ld = 0, s1 = 0, s2 = 0;
  bool t = false;
  Mat moved(long elements) const { Mat m = *this; if (p) m.p = (const char*)p + elements * esz; return m; }      // (a null base stays null: shape-only queries)
  Mat T() const { Mat m = *this; m.t = !t; return m; }
  Mat rows_at(long r0, int n) const { Mat m = moved(r0 * ld); m.rows = n; return m; }
  Mat cols_at(long c0, int n) const { Mat m = moved(c0); m.cols = n; return m; }
  Mat frames_at(long f0) const { return moved(f0 * s1); }                                                       // frame f0 becomes frame 0
  // `frames` frames as the rows of one matrix
  Mat flat(int frames) const {
    Mat m = *this; m.rows = frames * rows; m.s1 = 0;
    if (s1 != (long)rows * ld) { set_last_error("Mat::flat: frames of %d rows x ld %ld lie %ld elements apart", rows, ld, s1); m.esz = 0; }
    return m;
  }
  Mat groups(int g) const { Mat m = *this; m.cols = cols / g; m.s2 = m.cols; return m; }                        // g equal column groups as the second batch level
  Mat row_blocks(int step, int n) const { Mat m = *this; m.rows = n; m.s2 = step * ld; return m; }              // blocks of n rows, `step` rows apart, as the second batch level
  Mat planes(long stride) const { Mat m = *this; m.s2 = stride; return m; }                                     // whole copies of the tensor, `stride` elements apart, as the second batch level
};

// One K segment of a product:  sum_k A[b][i][k] * B[b][j][k].  The layouts are per segment and always meant: the engine and the streaming
// wrappers refuse a segment whose layouts they have no kernel for.
struct GemmSeg {
  const void* A = nullptr; const void* B = nullptr; int K = 0;
  int a_layout = K_MAJOR, b_layout = K_MAJOR;
  long lda = 0, ldb = 0, sA1 = 0, sA2 = 0, sB1 = 0, sB2 = 0;   // leading dimensions and batch strides, elements
  // The segment of the product A B (A: M x K, B: K x N, as views).  From  C[i][j] = sum_k A[i][k] B[j][k] : an A stored M x K is K_MAJOR, read
  // as the transpose of a stored K x M MN_MAJOR; a B stored K x N is MN_MAJOR, read as the transpose of a stored N x K K_MAJOR.
  // Returns M and N; refuses (ERR_BAD_ARG) when the two disagree on K or on the element type `esz`.
  int bind(const Mat& a, const Mat& b, int esz, int* M, int* N) {
    const int ka = a.t ? a.rows : a.cols, kb = b.t ? b.cols : b.rows;
    if (a.esz != esz || b.esz != esz) { set_last_error("product: operands of %d and %d bytes per element, dtype has %d", a.esz, b.esz, esz); return ERR_BAD_ARG; }
    if (ka != kb) { set_last_error("product: A has K = %d, B has K = %d", ka, kb); return ERR_BAD_ARG; }
    A = a.p; a_layout = a.t ? MN_MAJOR : K_MAJOR; lda = a.ld; sA1 = a.s1; sA2 = a.s2;
    B = b.p; b_layout = b.t ? K_MAJOR : MN_MAJOR; ldb = b.ld; sB1 = b.s1; sB2 = b.s2;
    K = ka; *M = a.t ? a.cols : a.rows; *N = b.t ? b.rows : b.cols;
    return OK;
  }
};

// A product: its first K segment (the base: A, B, K, a_layout .. sB2), up to three further ones (`seg`), the output, the batch levels, optional terms
struct GemmArgs : GemmSeg {
  void* C = nullptr;
  int M = 0, N = 0;
  int nb1 = 1, nb2 = 1;                 // batch = nb1 * nb2 ; b = b1 * nb2 + b2
  int nb3 = 1;                          // optional third batch level (tiled engine only, no D term): batch = nb1 * nb3 * nb2,
  long sA3 = 0, sB3 = 0, sC3 = 0;       // b = (b1 * nb3 + b3) * nb2 + b2 ; strides in elements
  int dtype = GEMM_F32;                 // A, B (and D) element type
  int out_dtype = GEMM_F32;             // C element type
  long sCi = 0, sCj = 1, sC1 = 0, sC2 = 0;   // C strides, elements
  float alpha = 1.f;
  int accumulate = 0;                   // C += ...
  // optional epilogue term  row_scale[b][i] * D[b][i][j]   (D: dtype `dtype`, j contiguous)
  const float* row_scale = nullptr;
  long sRS1 = 0, sRS2 = 0;
  const void* D = nullptr;
  long sDi = 0, sD1 = 0, sD2 = 0;
  // split-K: partial sums go to fp32 slabs [ksplit][batch][M][N] in `slabs`, then a reduce pass
  int ksplit = 1;
  float* slabs = nullptr;
  int keep_slabs = 0;                   // split-K: leave the partial sums in `slabs` (no reduce pass): the caller's consumer adds them
  // fp32 operands only: the product on the bf16 matrix pipe in THREE-PLANE form -- every value as three bf16 planes (x = p0 + p1 + p2 up to
  // 2^-24 |x|), the six plane products of order <= 2, fp32 accumulation: 5.8e-9 relative per product (the fp32 rounding of the sum itself is
  // 2 - 4e-7) at 6 x 16 instead of 8 x 32 matrix-pipe cycles per 16 x 16 x 32 block.  The site's BACKWARD sets it; the forward keeps
  // v_mfma_f32_16x16x4_f32 (same values to the last bit as rounds 1 - 3: which ReLU units sit on which side of zero does not move).
  // Non-finite operands: an Inf splits into (Inf, NaN, NaN) -- the residual planes are Inf - Inf -- so a product that exact fp32 arithmetic
  // would return as Inf comes out NaN; finite inputs only (as everywhere on this path: workspaces are NaN-poisoned in the tests).
  // 2 = TWO planes (split once at the LDS store), the three plane products of order <= 1: 2^-16 relative per product, half the matrix-pipe work --
  // available through avmoe_gemm (fp32_planes = 2) and used by the site backward for the products nothing downstream forms a cancelling sum
  // from (moe_run.h: AVMOE_LEAF2 = 26 -- dWt, the hop-1 weight gradients, the token gradients; AVMOE_BWD_PLANES has why not for all of them).
  int split3 = 0;
  int tile = 0;                         // 0 = auto, 64 or 128 = force block tile
  // optional second, third and fourth K segments (seg[0 .. 2]; present when A is set, each needs the one before it), accumulated into the
  // same tile before the epilogue, each with its own layouts and strides:  C += alpha * sum_i seg[i].A[b][i][k] * seg[i].B[b][j][k]
  // Built on the tiled engine: a second segment (K_MAJOR A, MN_MAJOR B) behind a first one with B MN_MAJOR -- fuses e.g.
  // dX = dZx Wt + [dL2|dsx|1] [T;1;dm1/N] so the (NT, C) result is written once -- and a third (MN_MAJOR A and B) with an optional fourth
  // (K_MAJOR A, MN_MAJOR B) behind a K_MAJOR A / MN_MAJOR B first and a second segment (bf16 or a plane form; A strided by sA1 only) -- the
  // OTHER adapter site's dY = [Bm ; wbar]^T dV + dR^T Q folded into this site's dX product (moe_backward_dx_dy): the token gradient is
  // written once instead of written by one site and read back + added by the other.
  GemmSeg seg[3];
  const GemmSeg& segment(int i) const { return i ? seg[i - 1] : *this; }      // i = 0 .. 3: all four, the first included
  // optional split output (streaming kernel only; launch_gemm_stream returns 1 when it cannot honour it): columns >= nsplit
  // (a multiple of 32) go, in fp32, to Cx[b2][i][j - nsplit] (row stride ldcx, group stride sCx2) instead of C -- lets the
  // wide part of a product be stored in bf16 while a few columns that feed long fp32 sums keep full precision.
  float* Cx = nullptr;
  int nsplit = 0;
  long ldcx = 0, sCx2 = 0;
  // optional statistics of A as a side product (streaming kernel only, K_MAJOR bf16 A, no second segment; launch_gemm_stream returns
  // 1 when it cannot honour them): per row the sum and the sum of squares over THIS group's K columns,
  //   st_rows[(2 b2) * st_ntot + b1 * M + i] = sum_k A ,  st_rows[(2 b2 + 1) * st_ntot + b1 * M + i] = sum_k A^2 ,
  // and per row tile the column sums  st_cols[(b1 * tiles + t) * (nb2 * K) + b2 * K + k] = sum_{i in tile t} A[b1][i][k]
  // (tiles = row tiles per sample, returned through st_tiles) -- the LayerNorm sums and the router's token means of X without a
  // separate pass over X.
  // optional softmax epilogues of the tiled engine (128 x 128 tile, no split-K, row-major C):
  //   epi = GEMM_EPI_ROWSTATS : nothing is stored to C; per row and column tile the running softmax statistics of alpha * (A B^T)
  //         go to row_part[((b * M + i) * tiles + t) * 2 + {0, 1}] = (max, sum of exp(v - max)), tiles = ceil(N / 128)
  //   epi = GEMM_EPI_EXP      : C = exp(alpha * (A B^T) - row_lse[b * M + i])
  //   epi = GEMM_EPI_MULSUB   : C = D * (alpha * (A B^T) - row_lse[b * M + i])      (D without row_scale: the softmax backward
  //         dS = att * (d att - rowdot) with d att = the product, never stored)
  // -- a row softmax without the scores ever leaving the chip (gemm_row_lse combines the parts).
  int epi = 0;
  float* row_part = nullptr;
  const float* row_lse = nullptr;
  float* st_rows = nullptr;
  float* st_cols = nullptr;
  long st_ntot = 0;
  int* st_tiles = nullptr;
  // optional EXTRA output columns against a per-sample matrix, from the same pass over A (streaming kernel with statistics only;
  // launch_gemm_stream returns 1 when it cannot honour them):
  //   xcols.C[b1][b2][i][j] = sum_k A[b1][b2][i][k] * xcols.B[b1][b2][j][k]      j < xcols.N <= 64, B K_MAJOR (ldb), fp32 result (row stride ldc)
  // -- the hop-2 logits of a site, X[s] T[s]^T, as per-group partial sums out of the down projection's pass over X (the caller adds
  // the groups): X is read once instead of twice.
  struct {
    const void* B = nullptr; int N = 0; long ldb = 0, sB1 = 0, sB2 = 0;
    float* C = nullptr; long ldc = 0, sC1 = 0, sC2 = 0;
  } xcols;

  // C = A B from views: the operands through GemmSeg::bind, M and N from them, C's strides from its view (a C that is the transpose of a stored
  // N x M gets sCi = 1, sCj = ld).  Set dtype / out_dtype (and Cx / nsplit) first: C must have out_dtype's element and the product's shape -- with a
  // split output its nsplit columns.  Batch counts, alpha, accumulate, ksplit and the epilogues stay the caller's.
  int product(const Mat& c, const Mat& a, const Mat& b) {
    AVMOE_TRY(bind(a, b, gemm_dtype_bytes(dtype), &M, &N));
    const int ci = c.t ? c.cols : c.rows, cj = c.t ? c.rows : c.cols;
    if (c.esz != gemm_dtype_bytes(out_dtype)) { set_last_error("product: C of %d bytes per element, out_dtype has %d", c.esz, gemm_dtype_bytes(out_dtype)); return ERR_BAD_ARG; }
    if (ci != M || cj != (nsplit ? nsplit : N)) { set_last_error("product: C is %d x %d, A B is %d x %d", ci, cj, M, N); return ERR_BAD_ARG; }
    C = const_cast<void*>(c.p); sCi = c.t ? 1 : c.ld; sCj = c.t ? c.ld : 1; sC1 = c.s1; sC2 = c.s2;
    return OK;
  }
  // + A B as K segment i = 1 .. 3 (seg[i - 1]) of a product already bound: it must have the product's M x N
  int add_segment(int i, const Mat& a, const Mat& b) {
    int m = 0, n = 0;
    AVMOE_TRY(seg[i - 1].bind(a, b, gemm_dtype_bytes(dtype), &m, &n));
    if (m != M || n != N) { set_last_error("product: segment %d is %d x %d, the product %d x %d", i, m, n, M, N); seg[i - 1] = GemmSeg(); return ERR_BAD_ARG; }
    return OK;
  }
  // + row_scale * D (or the D of GEMM_EPI_MULSUB): D stored M x N, in dtype
  int add_term(const Mat& dm) {
    if (dm.esz != gemm_dtype_bytes(dtype) || dm.t || dm.rows != M || dm.cols != N) { set_last_error("product: D is %d x %d of %d bytes, the product %d x %d", dm.rows, dm.cols, dm.esz, M, N); return ERR_BAD_ARG; }
    D = dm.p; sDi = dm.ld; sD1 = dm.s1; sD2 = dm.s2;
    return OK;
  }
};

// The block tile launch_gemm picks by itself for an (M, N) product, before it looks at the block count: what sizes split-K slabs (choose_ksplit)
inline int gemm_auto_tile(int M, int N) { return (M > 64 && N > 64) ? 128 : ((M <= 32 && N <= 32) ? 32 : 64); }

// Returns 0 on success, negative avmoe status otherwise (message through set_last_error).
int launch_gemm(const GemmArgs& args, hipStream_t stream);

// Streaming (B-stationary, persistent) kernel for token-streaming shapes; 0 = launched, 1 = shape not covered, < 0 error.
// launch_gemm tries it first.
enum { GEMM_EPI_NONE = 0, GEMM_EPI_ROWSTATS = 1, GEMM_EPI_EXP = 2, GEMM_EPI_MULSUB = 3 };
// lse[r] = log sum_j exp(v[r][j]) from the (max, sum) parts of GEMM_EPI_ROWSTATS (rows = batch * M, tiles = ceil(N / 128))
int gemm_row_lse(const float* row_part, long rows, int tiles, float* lse, hipStream_t stream);
int launch_gemm_stream(const GemmArgs& args, hipStream_t stream);
// Per-frame products of <= 64 rows against ONE shared K-major matrix (frame_gemm.hip); 0 = launched, 1 = shape not covered, < 0 error.
int launch_gemm_frames(const GemmArgs& args, hipStream_t stream);

// Two token contractions against the same (S, N, g * Cg) bf16 tensor X in ONE pass over it:
//   C1[gi][i][j]  = sum over ALL tokens t   A1[t][gi * sA1g + i] * X[t][gi * Cg + j]      i < M1 <= 128   (split over frame chunks: slabs + reduce)
//   C2[s][i][c]   = sum over the tokens of frame s   A2[t][i] * X[t][c]                   i < M2 <= 128   (one result per frame)
// (the backward's dWt = dZx^T X and dT[s] = dL2[s]^T X[s]).  Both results fp32.  Returns 1 when the shape is not served.
struct TokPairArgs {
  const void* A1 = nullptr; long lda1 = 0; int M1 = 0; long sA1g = 0;
  const void* A2 = nullptr; long lda2 = 0; int M2 = 0;
  const void* X = nullptr; long ldx = 0;
  int S = 0, N = 0, g = 1, Cg = 0;
  float* C1 = nullptr; float* C2 = nullptr;
  float* slabs = nullptr; size_t slab_cap = 0;          // floats
};
int launch_gemm_tokpair(const TokPairArgs& args, hipStream_t stream);

// Streaming kernels tuned for ONE product each of the bf16 cfg-2 site (384 channels per group, 128 bottleneck columns, 768-channel Y).  Like
// launch_gemm_stream they take the engine's descriptor of the product, check everything they assume of it and return 0 = launched,
// 1 = not served (nothing was launched: the caller goes on to the next form, launch_gemm last -- forms.h: try_forms), < 0 error.  launch_gemm does not try them.
int launch_dx_stream2(const GemmArgs& args, hipStream_t stream);     // dX[s] = dZx[s] Wt + dL2x[s] T[s] + rs X[s]: two K segments + row-scale term (dx_stream2.hip)
// ... with the other site's dY as segments three and four (seg[1], seg[2]), written once (dx_stream3.hip); slabs: >= 256 bytes the kernel may scribble on
bool dx_stream3_serves(const GemmArgs& args);                        // the same answer from shape and strides alone (no buffers yet)
int launch_dx_stream3(const GemmArgs& args, hipStream_t stream);
// the hop-1 chain's products against Y (hop1_stream.hip): C[s] = A[(s)] Y[s]^T (K-major A and Y, nb1 frames; slabs: 16 bytes the kernel may
// scribble on), C[s] = A[s] Y[s] (K-major A, MN-major Y, nb1 frames), C = A^T Y over all tokens (MN-major A and Y, one batch; slabs: slab_cap floats)
int launch_hop1_yk(const GemmArgs& args, hipStream_t stream);
int launch_hop1_yt_frames(const GemmArgs& args, hipStream_t stream);
int launch_hop1_yt_sum(const GemmArgs& args, size_t slab_cap, hipStream_t stream);
int launch_tok_pair2(const TokPairArgs& args, hipStream_t stream);   // launch_gemm_tokpair's two contractions with every accumulator in registers (tok_pair2.hip)
// dBpost = dOut^T Apost (`dbpost`) and dApost = dOut Bpost in its split-output form (`dapost`: Cx / nsplit) from one pass over dOut
// (dpost_pair.hip); slab_cap: floats in dbpost.slabs
int launch_dpost_pair(const GemmArgs& dbpost, const GemmArgs& dapost, size_t slab_cap, hipStream_t stream);
// Whether the streaming kernel serves a per-sample bf16 product  (M rows per sample, nb1 samples) x (K per group, lda) -> N columns per group
// WITH the statistics of A (GemmArgs::st_rows / st_cols): what a plan asks before it drops the separate statistics pass.
bool gemm_stream_stats_ok(int M, int nb1, int N, int K, long lda, long ldc);

// Bytes of fp32 slab workspace a split-K launch of `args` needs (0 when ksplit <= 1).
size_t gemm_slab_bytes(const GemmArgs& args);

}  // namespace avmoe
