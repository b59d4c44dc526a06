// Muon for the optimizer with device-side state (include/avmoe.h, avmoe_opt_muon_step): orthogonalised momentum for the ranges that are
// listed as small matrices, the unchanged Adam / AdamW update for every other range.  Two launches in place of kk_opt_adam --
//   kk_opt_muon_update<DECOUPLED, SCHED, EMA, HOLD>   one block per table block (the table walk of opt_table.h).  A range that is not
//                                          listed: adam_quad with kk_opt_adam's arguments, so kk_opt_adam's bits.  A listed range: the
//                                          momentum m (into exp_avg), the direction u into the range's slice of the work buffer, and the
//                                          block's sum of (double)u^2.  Listed: in the image's map, or in the second map that
//                                          avmoe_opt_muon_step_large (opt_muon_large.hip) hands in for the large matrices
//   kk_opt_muon_ns<STEP>                   one workgroup per matrix: ||u||_F from the block sums in a fixed order, then the Newton-Schulz
//                                          iteration in place in the work buffer, then (STEP) decay and update of the parameter
// The first optimizer kernel here whose hot path is matrix-shaped.  With Y the d x L view of a matrix (d = its short side <= 128):
//   A = Y Y^T and B = b A + c A A live in LDS as d_pad x d_pad fp32 (d_pad = d rounded up to 16, the padding rows zero), row stride
//   d_pad + 4 words so that 16-byte reads of 16 rows fall on different banks;
//   Y is streamed in chunks of T columns through the rest of the LDS (a d_pad x T image, row stride T + 4).  Y <- a Y + B Y is local to
//   a chunk, so a chunk is loaded, multiplied (accumulators in registers, at most 4 tiles per wave), overwritten in LDS, stored, and
//   the NEXT iteration's Gram matrix is accumulated from the image just produced: one pass over Y per iteration, plus one before the
//   first for the Gram matrix of Y0.  The two-pass form (Gram in a pass of its own, MUON_GRAM_SECOND_PASS below) measured 10 - 17 %
//   slower at every shape (DESIGN_CURRENT.md section 4b).
//   Products: v_mfma_f32_16x16x4_f32, a tile's 4 k-steps from one 16-byte read of each operand where the operand is contiguous along the
//   contraction index (both operands of a Gram product; the B operand of B Y is read word by word).
//   Tiles are dealt to the eight waves round robin; every accumulator array is indexed by unrolled constants only (no scratch).
// LDS: the launch always asks for the whole 160 KB of a compute unit, whatever d -- a workgroup that issues v_mfma_f32_16x16x4_f32 must
// not share its CU with a foreign dense-MFMA block (include/avmoe.h, avmoe_moe_desc::shared_gpu), and a step may run beside an
// all-reduce or a backbone kernel.  The kernel has no static LDS: the reduction tree uses the head of the dynamic block.
// No floating-point atomics; every sum has a fixed order.
#include "../../include/avmoe.h"
#include "common.h"
#include "adam_elem.h"
#include "opt_table.h"
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

namespace avmoe {

typedef __attribute__((ext_vector_type(4))) float f32x4;

constexpr uint32_t MUON_MAGIC = 0x4d554f4eu;     // "MUON"
constexpr int MUON_LDS_BYTES = 160 * 1024;       // the whole CU
constexpr int MUON_LDS_FLOATS = MUON_LDS_BYTES / 4;
#ifndef MUON_GRAM_SECOND_PASS
#define MUON_GRAM_SECOND_PASS 0                  // development builds (timing only): 1 = the next iteration's Gram matrix is taken in a pass
#endif                                           // of its own over Y instead of from the chunk just produced (scripts/muon_ns_probe.py)
constexpr int MUON_THREADS = 512, MUON_WAVES = 8;   // two waves per SIMD: one hides the other's LDS reads and dependent matrix instructions
constexpr int MUON_GT = 64 / MUON_WAVES;            // Gram tiles per wave at d_pad = 128
constexpr int MUON_UT = 32 / MUON_WAVES;            // output tiles of a chunk per wave, at most
constexpr int MUON_BATCH = 8;                       // independent global loads a thread has in flight when a chunk moves
constexpr float MUON_A = 3.4445f, MUON_B = -4.7750f, MUON_C = 2.0315f;

// the image avmoe_opt_muon_table_build writes: header, n_mats matrices, then n_ranges int32: the matrix of a range, or -1
struct MuonHeader { uint32_t magic; int32_t n_mats, n_ranges, reserved; };
static_assert(sizeof(MuonHeader) == 16 && sizeof(avmoe_opt_muon_mat) == 16 && sizeof(avmoe_opt_muon) == 16, "Muon layout");

static size_t muon_image_bytes(int32_t n_ranges, int32_t n_mats) {
  return round16(sizeof(MuonHeader) + (size_t)n_mats * sizeof(avmoe_opt_muon_mat) + (size_t)n_ranges * sizeof(int32_t));
}

// One element of a listed range (include/avmoe.h): the momentum and the direction, every operation rounded to fp32 in the order written
// (contraction off, so the 16-byte body and the scalar tail round alike).  p is only read.
template <bool DECOUPLED>
__device__ __forceinline__ float muon_elem(float p, float& m, float g, float mu, float wd, float gscale, int nesterov) {
#pragma clang fp contract(off)
  float gr;
  if constexpr (DECOUPLED) gr = g * gscale;
  else gr = __builtin_fmaf(gscale, g, wd * p);
  const float t = (1.f - mu) * gr;
  m = __builtin_fmaf(mu, m, t);
  return nesterov ? __builtin_fmaf(mu, m, t) : m;
}

template <bool DECOUPLED, bool SCHED, bool EMA, bool HOLD>
__global__ void __launch_bounds__(256) kk_opt_muon_update(const void* __restrict__ table, const avmoe_opt_state* __restrict__ state, float b1, float b2,
                                                          float eps, float grad_scale, float* const* __restrict__ shadows,
                                                          float* const* __restrict__ hold, int n_ranges, const void* __restrict__ image, int n_mats,
                                                          float* const* __restrict__ work, float mu, int nesterov, double* __restrict__ sums,
                                                          const void* __restrict__ large, int n_large) {
  const bool skip = state->skip != 0;
  if constexpr (!HOLD) {
    if (skip) return;
  }
  OptWork w;
  w.range = -1; w.n_ranges = -1;
  const bool mine = opt_work(table, w);                   // false for a thread past its range's end, too: the block's range is in w then
  if (w.range < 0 || w.n_ranges != n_ranges) return;      // block-uniform from here on
  const MuonHeader mh = *(const MuonHeader*)image;
  if (mh.magic != MUON_MAGIC || mh.n_mats != n_mats || mh.n_ranges != n_ranges) return;
  int mat = ((const int32_t*)((const avmoe_opt_muon_mat*)((const char*)image + sizeof(MuonHeader)) + n_mats))[w.range];
  if (large) {                                            // avmoe_opt_muon_step_large: a range of the large image's map is listed too
    const int32_t* large_map = muonl_map(large, n_large, n_ranges);
    if (!large_map) return;
    if (mat < 0) mat = large_map[w.range];
  }
  const avmoe_opt_range& r = w.r;
  const float* h = nullptr;
  if constexpr (HOLD) {
    h = opt_shadow(w, hold, n_ranges);
    if (!h) return;
    if (skip) {
      if (mine) restore_quad(r.param, h, w.i0, (long)r.n);
      return;
    }
  }
  float* e = nullptr;
  float d = 0.f;
  if constexpr (EMA) {
    e = opt_shadow(w, shadows, n_ranges);
    if (!e) return;
    d = state->ema_decay;
  }
  const float gscale = grad_scale * state->clip_coef;
  if (mat < 0) {                                          // not listed: kk_opt_adam's call
    float lr = r.lr;
    if constexpr (SCHED) lr *= state->lr_factor;
    if (mine) adam_quad<DECOUPLED, EMA, HOLD>(r.param, r.grad, r.exp_avg, r.exp_avg_sq, w.i0, (long)r.n, lr, b1, b2, eps, r.weight_decay, state->bc1,
                                              state->bc2_sqrt, gscale, e, d, h);
    return;
  }
  float* wk = opt_shadow(w, work, n_ranges);
  if (!wk) return;
  double su = 0.0;
  if (mine) {
    const float* __restrict__ src = r.param;
    if constexpr (HOLD) src = h;
    const long i0 = w.i0, n = r.n;
    const float wd = r.weight_decay;
    if (i0 + 3 < n) {
      const float4 pp = *(const float4*)(src + i0), gg = *(const float4*)(r.grad + i0);
      float4 mm = *(float4*)(r.exp_avg + i0), uu;
      const float* P = (const float*)&pp; const float* G = (const float*)&gg; float* M = (float*)&mm; float* U = (float*)&uu;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        U[k] = muon_elem<DECOUPLED>(P[k], M[k], G[k], mu, wd, gscale, nesterov);
        su += (double)U[k] * (double)U[k];
      }
      *(float4*)(r.exp_avg + i0) = mm; *(float4*)(wk + i0) = uu;
    } else {
      for (long i = i0; i < n; ++i) {
        float mv = r.exp_avg[i];
        const float u = muon_elem<DECOUPLED>(src[i], mv, r.grad[i], mu, wd, gscale, nesterov);
        r.exp_avg[i] = mv; wk[i] = u;
        su += (double)u * (double)u;
      }
    }
  }
  const double t = block_sum_256(su);
  if (threadIdx.x == 0) sums[blockIdx.x] = t;
}

// a scalar the optimiser cannot see through (always 0): added to the wave index where a tile loop starts, so that the sixteen tiles'
// addresses are formed where they are used instead of being hoisted out of every loop into (and spilled from) registers
__device__ __forceinline__ int sopaque0() { int v = 0; asm volatile("" : "+s"(v)); return v; }

// acc[s] += the 16 x 16 tile (ti, tj) of S S^T over K columns (K a multiple of 16) for the wave's tiles t = wv + MUON_WAVES s < nt * nt,
// ti = t / nt, tj = t % nt.  S: LDS, row-major with stride ld (a multiple of 4).  Lane (r = lane & 15, q = lane >> 4) reads S[16 ti + r]
// [k0 + 4 q .. + 3] and S[16 tj + r][the same]: the four k-steps of one 16-byte read pair, the same permutation of k in both operands.
// The tile lands as acc[s][v] = (S S^T)[16 ti + 4 q + v][16 tj + r].
__device__ __forceinline__ void muon_gram(f32x4 (&acc)[MUON_GT], const float* S, int ld, int K, int nt, int wv0, int r, int q) {
  const int wv = wv0 + sopaque0();
#pragma unroll
  for (int s = 0; s < MUON_GT; ++s) {
    const int t = wv + MUON_WAVES * s;
    if (t < nt * nt) {
      const int ti = t / nt, tj = t - ti * nt;
      const float* ap = S + (16 * ti + r) * ld + 4 * q;
      const float* bp = S + (16 * tj + r) * ld + 4 * q;
      f32x4 c = acc[s];
      for (int k0 = 0; k0 < K; k0 += 16) {
        const float4 a = *(const float4*)(ap + k0), b = *(const float4*)(bp + k0);
        c = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b.x, c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b.y, c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b.z, c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b.w, c, 0, 0, 0);
      }
      acc[s] = c;
    }
  }
}

// what the STEP instantiation needs beyond the sub-op's arguments
struct MuonStep {
  const void* table;
  const avmoe_opt_state* state;
  const double* sums;
  float* const* shadows;
  float* const* hold;
  void* report;
  long n_blocks;
  int n_ranges;
  int decoupled, sched, ema, with_hold, scale;
  const void* large;              // avmoe_opt_muon_step_large: the image of n_large large matrices the table walk has checked, else NULL
  int n_large;
};

// One workgroup of 512 threads per matrix (see the head of this file).  STEP: the norm from launch 1's block sums, the report, and in
// the last pass the parameter (and its shadow); otherwise (avmoe_opt_muon_ns) the norm from the elements and nothing but the work buffer.
// A launch that does not match its image (STEP: or its table), or a matrix whose buffers cannot take the accesses, touches nothing.
template <bool STEP>
__global__ void __launch_bounds__(MUON_THREADS) kk_opt_muon_ns(const void* __restrict__ image, int n_mats, float* const* __restrict__ work, int ns_steps,
                                                      MuonStep sa) {
  extern __shared__ __align__(16) float lds[];
  if constexpr (STEP) {
    if (sa.state->skip) return;
    if (sa.large && !muonl_map(sa.large, sa.n_large, sa.n_ranges)) return;      // the table walk has left no u and no sums then
  }
  const MuonHeader mh = *(const MuonHeader*)image;
  if (mh.magic != MUON_MAGIC || mh.n_mats != n_mats || (int)gridDim.x != n_mats) return;
  const avmoe_opt_muon_mat mt = ((const avmoe_opt_muon_mat*)((const char*)image + sizeof(MuonHeader)))[blockIdx.x];
  if (mt.range < 0 || mt.range >= mh.n_ranges || mt.rows < 1 || mt.cols < 1) return;
  const int rows = mt.rows, cols = mt.cols;
  const bool wide = rows <= cols;
  const int d = wide ? rows : cols, L = wide ? cols : rows;
  if (d > AVMOE_MUON_MAX_DIM) return;
  const long n = (long)rows * cols;
  const long si = wide ? cols : 1, sl = wide ? 1 : cols;      // element (i, l) of the d x L view is X[i * si + l * sl]
  float* __restrict__ X = work[mt.range];
  if (!X || ((uintptr_t)X & 15u) != 0) return;
  const int tid = threadIdx.x;

  // STEP: the range, its blocks in the map (the search of kk_opt_range_norms), its side buffers and rates
  float* param = nullptr; const float* src = nullptr; float* ema = nullptr;
  long lo = 0, nb = 0;
  float lr = 0.f, wd = 0.f, step = 0.f, decay = 0.f;
  if constexpr (STEP) {
    const OptHeader h = *(const OptHeader*)sa.table;
    if (h.magic != OPT_MAGIC || h.n_ranges != sa.n_ranges || h.n_blocks != sa.n_blocks || mh.n_ranges != sa.n_ranges) return;
    const avmoe_opt_range* ranges = (const avmoe_opt_range*)((const char*)sa.table + sizeof(OptHeader));
    const OptBlock* map = (const OptBlock*)(ranges + sa.n_ranges);
    const avmoe_opt_range r = ranges[mt.range];
    if (r.n != n) return;
    nb = (n + OPT_BLOCK - 1) / OPT_BLOCK;
    long hi = sa.n_blocks;
    while (lo < hi) {
      const long mid = (lo + hi) >> 1;
      if (map[mid].range < mt.range) lo = mid + 1; else hi = mid;
    }
    if (lo + nb > sa.n_blocks || map[lo].range != mt.range || map[lo + nb - 1].range != mt.range) return;
    param = r.param; src = r.param;
    if (sa.with_hold) {
      src = sa.hold[mt.range];
      if (!src || ((uintptr_t)src & 15u) != 0) return;
    }
    if (sa.ema) {
      ema = sa.shadows[mt.range];
      if (!ema || ((uintptr_t)ema & 15u) != 0) return;
      decay = sa.state->ema_decay;
    }
    lr = r.lr;
    if (sa.sched) lr *= sa.state->lr_factor;
    wd = r.weight_decay;
    const double big = (double)(rows > cols ? rows : cols);
    const float s = sa.scale == AVMOE_MUON_SCALE_ORIGINAL ? (float)sqrt(fmax(1.0, (double)rows / (double)cols)) : (float)(0.2 * sqrt(big));
    step = lr * s;
  }

  // ||u||_F: thread t adds its terms in index order, then a tree over the head of the LDS
  double* red = (double*)lds;
  double acc = 0.0;
  if constexpr (STEP) {
    for (long i = tid; i < nb; i += MUON_THREADS) acc += sa.sums[lo + i];
  } else {
    for (long i = tid; i < n; i += MUON_THREADS) { const double v = (double)X[i]; acc += v * v; }
  }
  red[tid] = acc;
  __syncthreads();
#pragma unroll
  for (int s = MUON_THREADS / 2; s > 0; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  const double nrm = sqrt(red[0]);
  __syncthreads();                                          // the tree's words become A
  const float inv = (float)(1.0 / (nrm + 1e-7));
  if constexpr (STEP) {
    if (tid == 0) {
      if (blockIdx.x == 0) *(int4*)sa.report = make_int4(n_mats, 0, 0, 0);
      ((float*)sa.report)[4 + blockIdx.x] = (float)nrm;
    }
  }

  // the LDS plan
  const int dp = (d + 15) & ~15, nt = dp >> 4, ldA = dp + 4;
  float* As = lds;
  float* Bs = As + dp * ldA;
  float* Ys = Bs + dp * ldA;
  int T = (MUON_LDS_FLOATS - 2 * dp * ldA) / dp - 4;        // the widest chunk the rest of the LDS holds
  const int tcap = 16 * (32 / nt), lpad = (L + 15) & ~15;   // at most 32 output tiles (MUON_UT per wave); no wider than the matrix
  T = T < tcap ? T : tcap;
  T = T < lpad ? T : lpad;
  T = T >= 32 ? (T & ~31) : 16;                             // row stride T + 4 = 4 mod 32 words where the room allows
  const int ldY = T + 4, ntl = T >> 4, nchunk = (L + T - 1) / T;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, r = lane & 15, q = lane >> 4;

  // element e of a chunk image -> (i, l): consecutive threads take consecutive addresses of the work buffer, along l for a wide matrix,
  // along i for a tall one
  const int nel = dp * T;
  auto split = [&](int e, int& i, int& l) {
    if (wide) { i = e / T; l = e - i * T; } else { l = e / dp; i = e - l * dp; }
  };
  // chunk [l0, l0 + T) of the view -> Ys, times sc; rows >= d and columns >= L are zeros.  MUON_BATCH loads per thread are issued before
  // the first store, unconditional at an index clamped into the matrix (a load under a condition is waited for on the spot).
  auto load = [&](int l0, float sc) {
    for (int e0 = tid; e0 < nel; e0 += MUON_BATCH * MUON_THREADS) {
      float v[MUON_BATCH];
      int at[MUON_BATCH];
#pragma unroll
      for (int u = 0; u < MUON_BATCH; ++u) {
        const int e = e0 + u * MUON_THREADS < nel ? e0 + u * MUON_THREADS : nel - 1;
        int i, l;
        split(e, i, l);
        const bool in = i < d && l0 + l < L;
        const int ic = i < d ? i : d - 1, lc = l0 + l < L ? l0 + l : L - 1;
        const float x = X[ic * si + (long)lc * sl];
        v[u] = in ? x * sc : 0.f;
        at[u] = i * ldY + l;
      }
#pragma unroll
      for (int u = 0; u < MUON_BATCH; ++u)
        if (e0 + u * MUON_THREADS < nel) Ys[at[u]] = v[u];
    }
  };

  f32x4 G[MUON_GT];
#pragma unroll
  for (int s = 0; s < MUON_GT; ++s) G[s] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int c = 0; c < nchunk; ++c) {                        // the Gram matrix of Y0
    load(c * T, inv);
    __syncthreads();
    muon_gram(G, Ys, ldY, T, nt, wv, r, q);
    __syncthreads();
  }

  for (int it = 0; it < ns_steps; ++it) {
    const bool last = it == ns_steps - 1;
    // A -> LDS, B = b A + c A A -> LDS (A is symmetric bit for bit: both triangles are the same chain of products)
    const int wa = wv + sopaque0();
#pragma unroll
    for (int s = 0; s < MUON_GT; ++s) {
      const int t = wa + MUON_WAVES * s;
      if (t < nt * nt) {
        const int ti = t / nt, tj = t - ti * nt;
#pragma unroll
        for (int v = 0; v < 4; ++v) As[(16 * ti + 4 * q + v) * ldA + 16 * tj + r] = G[s][v];
      }
      G[s] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    __syncthreads();
    {
      f32x4 P[MUON_GT];
#pragma unroll
      for (int s = 0; s < MUON_GT; ++s) P[s] = f32x4{0.f, 0.f, 0.f, 0.f};
      muon_gram(P, As, ldA, dp, nt, wv, r, q);
#pragma unroll
      for (int s = 0; s < MUON_GT; ++s) {
        const int t = wa + MUON_WAVES * s;
        if (t < nt * nt) {
          const int ti = t / nt, tj = t - ti * nt;
#pragma unroll
          for (int v = 0; v < 4; ++v) {
            const int idx = (16 * ti + 4 * q + v) * ldA + 16 * tj + r;
            Bs[idx] = MUON_B * As[idx] + MUON_C * P[s][v];
          }
        }
      }
    }
    __syncthreads();

    for (int c = 0; c < nchunk; ++c) {
      const int l0 = c * T;
      load(l0, it == 0 ? inv : 1.f);
      __syncthreads();
      // U = B Y for the wave's tiles p = wv + MUON_WAVES s < nt * ntl: rows 16 ti of B, columns 16 tl of the chunk
      const int wc = wv + sopaque0();
      f32x4 U[MUON_UT];
#pragma unroll
      for (int s = 0; s < MUON_UT; ++s) {
        U[s] = f32x4{0.f, 0.f, 0.f, 0.f};
        const int p = wc + MUON_WAVES * s;
        if (p < nt * ntl) {
          const int tl = p / nt, ti = p - tl * nt;
          const float* ap = Bs + (16 * ti + r) * ldA + 4 * q;
          const float* bp = Ys + (4 * q) * ldY + 16 * tl + r;
          f32x4 cc = U[s];
          for (int k0 = 0; k0 < dp; k0 += 16) {
            const float4 a = *(const float4*)(ap + k0);
            const float* b = bp + k0 * ldY;
            cc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b[0], cc, 0, 0, 0);
            cc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b[ldY], cc, 0, 0, 0);
            cc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b[2 * ldY], cc, 0, 0, 0);
            cc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b[3 * ldY], cc, 0, 0, 0);
          }
          U[s] = cc;
        }
      }
      __syncthreads();                                      // every wave has read the old image
#pragma unroll
      for (int s = 0; s < MUON_UT; ++s) {
        const int p = wc + MUON_WAVES * s;
        if (p < nt * ntl) {
          const int tl = p / nt, ti = p - tl * nt;
#pragma unroll
          for (int v = 0; v < 4; ++v) {
            const int idx = (16 * ti + 4 * q + v) * ldY + 16 * tl + r;
            Ys[idx] = MUON_A * Ys[idx] + U[s][v];
          }
        }
      }
      __syncthreads();
      // the new image -> the work buffer; STEP, last pass: and the parameter (its loads batched like the chunk's)
      for (int e0 = tid; e0 < nel; e0 += MUON_BATCH * MUON_THREADS) {
        float o[MUON_BATCH], pv[MUON_BATCH], ev[MUON_BATCH];
        long idx[MUON_BATCH];
        bool in[MUON_BATCH];
#pragma unroll
        for (int u = 0; u < MUON_BATCH; ++u) {
          const int e = e0 + u * MUON_THREADS < nel ? e0 + u * MUON_THREADS : nel - 1;
          int i, l;
          split(e, i, l);
          in[u] = e0 + u * MUON_THREADS < nel && i < d && l0 + l < L;
          const int ic = i < d ? i : d - 1, lc = l0 + l < L ? l0 + l : L - 1;
          idx[u] = ic * si + (long)lc * sl;
          o[u] = Ys[i * ldY + l];
          pv[u] = 0.f; ev[u] = 0.f;
          if constexpr (STEP) {
            if (last) {
              pv[u] = src[idx[u]];
              if (ema) ev[u] = ema[idx[u]];
            }
          }
        }
#pragma unroll
        for (int u = 0; u < MUON_BATCH; ++u) {
          if (in[u]) {
            X[idx[u]] = o[u];
            if constexpr (STEP) {
              if (last) {
                const float pn = muon_next(pv[u], o[u], lr, wd, step, sa.decoupled != 0);
                param[idx[u]] = pn;
                if (ema) ema[idx[u]] = ema_next(ev[u], pn, decay);
              }
            }
          }
        }
      }
#if !MUON_GRAM_SECOND_PASS
      if (!last) muon_gram(G, Ys, ldY, T, nt, wv, r, q);
#endif
      __syncthreads();
    }
#if MUON_GRAM_SECOND_PASS
    if (!last) {
      for (int c = 0; c < nchunk; ++c) {
        load(c * T, 1.f);
        __syncthreads();
        muon_gram(G, Ys, ldY, T, nt, wv, r, q);
        __syncthreads();
      }
    }
#endif
  }
}

using MuonUpdateKernel = decltype(&kk_opt_muon_update<false, false, false, false>);
constexpr MuonUpdateKernel OPT_MUON[16] = {           // [DECOUPLED | SCHED << 1 | EMA << 2 | HOLD << 3]
    kk_opt_muon_update<false, false, false, false>, kk_opt_muon_update<true, false, false, false>,
    kk_opt_muon_update<false, true, false, false>,  kk_opt_muon_update<true, true, false, false>,
    kk_opt_muon_update<false, false, true, false>,  kk_opt_muon_update<true, false, true, false>,
    kk_opt_muon_update<false, true, true, false>,   kk_opt_muon_update<true, true, true, false>,
    kk_opt_muon_update<false, false, false, true>,  kk_opt_muon_update<true, false, false, true>,
    kk_opt_muon_update<false, true, false, true>,   kk_opt_muon_update<true, true, false, true>,
    kk_opt_muon_update<false, false, true, true>,   kk_opt_muon_update<true, false, true, true>,
    kk_opt_muon_update<false, true, true, true>,    kk_opt_muon_update<true, true, true, true>};

// what both launching calls refuse about the image, the work pointers and the iteration count
static int check_muon_args(const char* who, const void* mats, int32_t n_mats, float* const* work, int32_t ns_steps) {
  if (!mats) { set_last_error("%s: the matrix image is NULL", who); return ERR_BAD_ARG; }
  if (!work) { set_last_error("%s: the work pointer array is NULL", who); return ERR_BAD_ARG; }
  if (n_mats < 0) { set_last_error("%s: negative matrix count %d", who, (int)n_mats); return ERR_BAD_ARG; }
  if (ns_steps < 1 || ns_steps > 16) { set_last_error("%s: ns_steps must be in 1..16, not %d", who, (int)ns_steps); return ERR_BAD_ARG; }
  if (((uintptr_t)mats & 15u) != 0) { set_last_error("%s: the matrix image must be 16-byte aligned", who); return ERR_ALIGNMENT; }
  if (((uintptr_t)work & 7u) != 0) { set_last_error("%s: the work pointer array must be 8-byte aligned", who); return ERR_ALIGNMENT; }
  return OK;
}

static LdsAttrOnce g_muon_lds_step, g_muon_lds_ns;

// avmoe_opt_muon_step in two halves (opt_table.h): avmoe_opt_muon_step_large makes its own checks between them
int muon_step_check(const char* who, const void* table, int32_t n_ranges, int64_t n_blocks, const avmoe_opt_state* state, float beta1, float beta2,
                    float eps, float grad_scale, int32_t flags, float* const* shadows, float* const* hold, const void* mats, int32_t n_mats,
                    float* const* work, const avmoe_opt_muon* consts, const double* workspace, const void* report) {
  const bool with_hold = hold != nullptr;
  AVMOE_TRY(check_step_args(who, table, n_ranges, n_blocks, state, beta1, beta2, eps, grad_scale, flags, OPT_STEP_FLAGS, shadows, with_hold, hold));
  if (!consts) { set_last_error("%s: the constants are NULL", who); return ERR_BAD_ARG; }
  if (!workspace) { set_last_error("%s: the workspace is NULL", who); return ERR_BAD_ARG; }
  if (!report) { set_last_error("%s: the report buffer is NULL", who); return ERR_BAD_ARG; }
  AVMOE_TRY(check_muon_args(who, mats, n_mats, work, consts->ns_steps));
  if (!(consts->momentum >= 0.f && consts->momentum < 1.f)) { set_last_error("%s: momentum must be in [0, 1)", who); return ERR_BAD_ARG; }
  if (consts->nesterov != 0 && consts->nesterov != 1) { set_last_error("%s: nesterov must be 0 or 1, not %d", who, (int)consts->nesterov); return ERR_BAD_ARG; }
  if (consts->scale != AVMOE_MUON_SCALE_MATCH_RMS_ADAMW && consts->scale != AVMOE_MUON_SCALE_ORIGINAL) {
    set_last_error("%s: unknown scale %d", who, (int)consts->scale); return ERR_BAD_ARG;
  }
  if (((uintptr_t)workspace & 7u) != 0) { set_last_error("%s: the workspace must be 8-byte aligned", who); return ERR_ALIGNMENT; }
  if (((uintptr_t)report & 15u) != 0) { set_last_error("%s: the report buffer must be 16-byte aligned", who); return ERR_ALIGNMENT; }
  return OK;
}

int muon_step_launch(const char* who, const void* table, int32_t n_ranges, int64_t n_blocks, const avmoe_opt_state* state, float beta1, float beta2,
                     float eps, float grad_scale, int32_t flags, hipStream_t stream, float* const* shadows, float* const* hold, const void* mats,
                     int32_t n_mats, float* const* work, const avmoe_opt_muon* consts, double* workspace, void* report, const void* large,
                     int32_t n_large) {
  const bool with_hold = hold != nullptr;
  const bool dec = (flags & AVMOE_OPT_DECOUPLED_DECAY) != 0, sched = (flags & AVMOE_OPT_LR_SCHEDULE) != 0, ema = (flags & AVMOE_OPT_EMA) != 0;
  if (n_mats > 0) AVMOE_TRY(g_muon_lds_step.ensure((const void*)kk_opt_muon_ns<true>, MUON_LDS_BYTES, who));
  if (n_blocks > 0) {
    hipLaunchKernelGGL(OPT_MUON[(int)dec | (int)sched << 1 | (int)ema << 2 | (int)with_hold << 3], dim3((unsigned)n_blocks), dim3(256), 0,
                       stream, table, state, beta1, beta2, eps, grad_scale, ema ? shadows : nullptr, hold, (int)n_ranges, mats, (int)n_mats,
                       work, consts->momentum, (int)consts->nesterov, workspace, large, (int)n_large);
    AVMOE_CHECK_LAUNCH("opt_muon_update");
  }
  if (n_mats > 0 && n_blocks > 0) {
    MuonStep sa;
    sa.table = table; sa.state = state; sa.sums = workspace; sa.shadows = ema ? shadows : nullptr; sa.hold = hold; sa.report = report;
    sa.n_blocks = (long)n_blocks; sa.n_ranges = (int)n_ranges;
    sa.decoupled = (int)dec; sa.sched = (int)sched; sa.ema = (int)ema; sa.with_hold = (int)with_hold; sa.scale = (int)consts->scale;
    sa.large = large; sa.n_large = (int)n_large;
    hipLaunchKernelGGL(kk_opt_muon_ns<true>, dim3((unsigned)n_mats), dim3(MUON_THREADS), MUON_LDS_BYTES, stream, mats, (int)n_mats, work,
                       (int)consts->ns_steps, sa);
    AVMOE_CHECK_LAUNCH("opt_muon_ns");
  }
  return OK;
}

}  // namespace avmoe

using namespace avmoe;

extern "C" {

size_t avmoe_opt_muon_bytes(int32_t n_ranges, int64_t n_blocks, int32_t n_mats, avmoe_opt_muon_layout* layout) {
  if (n_ranges < 0 || n_mats < 0 || n_mats > n_ranges) {
    set_last_error("avmoe_opt_muon_bytes: bad range / matrix count %d / %d", (int)n_ranges, (int)n_mats); return 0;
  }
  if (n_blocks < 0 || n_blocks > (int64_t)INT32_MAX) { set_last_error("avmoe_opt_muon_bytes: bad block count %lld", (long long)n_blocks); return 0; }
  avmoe_opt_muon_layout l;
  l.table_bytes = muon_image_bytes(n_ranges, n_mats);
  l.workspace_bytes = round16((size_t)(n_blocks > 0 ? n_blocks : 1) * sizeof(double));
  l.report_bytes = 16 + round16((size_t)(n_mats > 0 ? n_mats : 1) * sizeof(float));
  if (layout) *layout = l;
  return l.table_bytes + l.workspace_bytes + l.report_bytes;
}

int avmoe_opt_muon_table_build(const avmoe_opt_range* ranges, int32_t n_ranges, const avmoe_opt_muon_mat* mats, int32_t n_mats, void* image,
                               size_t image_bytes) {
  const char* who = "avmoe_opt_muon_table_build";
  if (n_ranges < 0 || n_mats < 0) { set_last_error("%s: negative range / matrix count", who); return ERR_BAD_ARG; }
  if (n_mats > 0 && !mats) { set_last_error("%s: mats is NULL", who); return ERR_BAD_ARG; }
  if (!image) { set_last_error("%s: image is NULL", who); return ERR_BAD_ARG; }
  std::vector<int32_t> map((size_t)n_ranges, -1);
  for (int32_t j = 0; j < n_mats; ++j) {
    const avmoe_opt_muon_mat& m = mats[j];
    if (m.range < 0 || m.range >= n_ranges) { set_last_error("%s: matrix %d names range %d of %d", who, (int)j, (int)m.range, (int)n_ranges); return ERR_BAD_ARG; }
    if (m.rows < 1 || m.cols < 1) { set_last_error("%s: matrix %d is %d x %d", who, (int)j, (int)m.rows, (int)m.cols); return ERR_BAD_ARG; }
    if ((m.rows < m.cols ? m.rows : m.cols) > AVMOE_MUON_MAX_DIM) {
      set_last_error("%s: matrix %d is %d x %d: its short side is above %d", who, (int)j, (int)m.rows, (int)m.cols, AVMOE_MUON_MAX_DIM); return ERR_BAD_ARG;
    }
    if (ranges && (int64_t)m.rows * m.cols != ranges[m.range].n) {
      set_last_error("%s: matrix %d is %d x %d, its range %d has %lld elements", who, (int)j, (int)m.rows, (int)m.cols, (int)m.range,
                     (long long)ranges[m.range].n);
      return ERR_BAD_ARG;
    }
    if (map[m.range] >= 0) { set_last_error("%s: range %d is named twice (matrices %d and %d)", who, (int)m.range, (int)map[m.range], (int)j); return ERR_BAD_ARG; }
    map[m.range] = j;
  }
  const size_t need = muon_image_bytes(n_ranges, n_mats);
  if (image_bytes < need) { set_last_error("%s: image of %zu bytes, %zu needed", who, image_bytes, need); return ERR_WORKSPACE; }
  char* p = (char*)image;
  memset(p, 0, need);
  const MuonHeader h{MUON_MAGIC, n_mats, n_ranges, 0};
  memcpy(p, &h, sizeof h);
  for (int32_t j = 0; j < n_mats; ++j) {
    const avmoe_opt_muon_mat m{mats[j].range, mats[j].rows, mats[j].cols, 0};
    memcpy(p + sizeof h + (size_t)j * sizeof m, &m, sizeof m);
  }
  if (n_ranges > 0) memcpy(p + sizeof h + (size_t)n_mats * sizeof(avmoe_opt_muon_mat), map.data(), (size_t)n_ranges * sizeof(int32_t));
  return OK;
}

int avmoe_opt_muon_step(const void* table, int32_t n_ranges, int64_t n_blocks, const avmoe_opt_state* state, float beta1, float beta2, float eps,
                        float grad_scale, int32_t flags, void* stream, float* const* shadows, float* const* hold, const void* mats, int32_t n_mats,
                        float* const* work, const avmoe_opt_muon* consts, double* workspace, void* report) {
  const char* who = "avmoe_opt_muon_step";
  AVMOE_TRY(muon_step_check(who, table, n_ranges, n_blocks, state, beta1, beta2, eps, grad_scale, flags, shadows, hold, mats, n_mats, work, consts,
                            workspace, report));
  return muon_step_launch(who, table, n_ranges, n_blocks, state, beta1, beta2, eps, grad_scale, flags, (hipStream_t)stream, shadows, hold, mats,
                          n_mats, work, consts, workspace, report, nullptr, 0);
}

int avmoe_opt_muon_ns(const void* mats, int32_t n_mats, float* const* work, int32_t ns_steps, void* stream) {
  const char* who = "avmoe_opt_muon_ns";
  AVMOE_TRY(check_muon_args(who, mats, n_mats, work, ns_steps));
  if (n_mats == 0) return OK;
  AVMOE_TRY(g_muon_lds_ns.ensure((const void*)kk_opt_muon_ns<false>, MUON_LDS_BYTES, who));
  MuonStep sa{};
  hipLaunchKernelGGL(kk_opt_muon_ns<false>, dim3((unsigned)n_mats), dim3(MUON_THREADS), MUON_LDS_BYTES, (hipStream_t)stream, mats, (int)n_mats, work, (int)ns_steps,
                     sa);
  AVMOE_CHECK_LAUNCH("opt_muon_ns");
  return OK;
}

}  // extern "C"
