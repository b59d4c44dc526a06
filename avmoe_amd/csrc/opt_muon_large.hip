// Muon for the LARGE matrices of the optimizer with device-side state (include/avmoe.h, avmoe_opt_muon_step_large): a short side above
// AVMOE_MUON_MAX_DIM, where a d x d fp32 Gram matrix no longer fits the LDS of a compute unit (2.4 MB at d = 768), so the three products
// of a Newton-Schulz iteration run on the tiled engine (gemm.hip, launch_gemm) instead of inside one workgroup (opt_muon.hip).  The rule
// per element and per matrix is opt_muon.hip's; this file adds what feeds the engine from the flat buckets without the host:
//   kk_opt_muon_large_pack<STEP>      (tiles, matrices) blocks: ||u||_F from the block sums in a fixed order, Y0 = Y * inv into a packed
//                                     staging area (class by class, matrix by matrix, short side first), the padding, the constants
//   launch_gemm x 3 per class and iteration, batched over the class, fp32 operands in three-plane form
//   kk_opt_muon_large_apply<DECOUPLED, SCHED, EMA, HOLD>   (tiles, matrices) blocks: O from staging into work[range], decay, update, shadow
//   kk_opt_muon_large_sumsq / kk_opt_muon_large_unpack     avmoe_opt_muon_ns_large only (tests): the block sums without a table, O alone
// Equal-shaped matrices of different sites lie at unrelated offsets in the buckets; the staging area gives the engine one batch stride
// per class.  Zero rows and columns stay zero through the iteration, so the padding to the engine's 16-byte rows is exact.
// No floating-point atomics; every sum has a fixed order.  No static state: the engine's launches are shaped from the HOST copy of the
// image on every call.
#include "../../include/avmoe.h"
#include "common.h"
#include "adam_elem.h"
#include "gemm.h"
#include "opt_table.h"
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

namespace avmoe {

constexpr int MUONL_TILE = 32;                   // staging moves in 32 x 32 tiles, 256 threads, four rows of a tile per thread
constexpr int MUONL_MAX_GX = 256;                // blocks per matrix at most: each adds the matrix's block sums itself
constexpr float MUONL_A = 3.4445f, MUONL_B = -4.7750f, MUONL_C = 2.0315f;
constexpr size_t MUONL_VEC_BYTES = (size_t)AVMOE_MUON_LARGE_MAX_DIM * sizeof(float);

// the image avmoe_opt_muon_large_table_build writes: header (opt_table.h), n_mats matrices, n_classes classes, then n_ranges int32: the
// matrix of a range, or -1.  Offsets are bytes from the workspace's base, multiples of 16.
struct MuonLargeMat {
  int32_t range, rows, cols, cls;
  int64_t y0, y1;             // the matrix's slot in its class's two staging buffers (d4 x L4 floats)
  int64_t a, b;               // ... in the class's A and B buffers (d x d4 floats)
  int64_t sum0;               // avmoe_opt_muon_ns_large: its first block sum, in doubles from sums_off
  int64_t reserved;
};
struct MuonLargeClass {
  int32_t d, L, count, ksplit;
  int64_t y0, y1, a, b, slabs;    // the class's buffers; slabs: 0 without split-K
  int64_t reserved;
};
static_assert(sizeof(MuonLargeMat) == MUONL_MAT_BYTES && sizeof(MuonLargeClass) == MUONL_CLASS_BYTES, "large Muon layout");

static inline int r4(int x) { return (x + 3) & ~3; }

static size_t muonl_image_bytes(int32_t n_ranges, int32_t n_mats, int32_t n_classes) {
  return round16(sizeof(MuonLargeHeader) + (size_t)n_mats * sizeof(MuonLargeMat) + (size_t)n_classes * sizeof(MuonLargeClass) +
                 (size_t)n_ranges * sizeof(int32_t));
}

// The Gram product of a class splits its contraction index where that index is long and the output tiles are few (128 x 4096: one 128 x 128
// tile per matrix): partial sums in slabs, one reduce launch more.  Fixed by the shape alone, so that the bits do not depend on the call.
static int muonl_ksplit(int d, int L, int count) {
  const long tiles = (long)cdiv(d, 128) * cdiv(d, 128) * count;
  if (L < 2048 || tiles >= 64) return 1;
  const int k = L / 512;
  return k > 8 ? 8 : k;
}

// classes in the order of first appearance, every matrix's class and slot, the workspace's bytes.  The list is assumed checked.
static size_t muonl_plan(const avmoe_opt_muon_mat* mats, int32_t n_mats, std::vector<MuonLargeClass>& classes, std::vector<MuonLargeMat>& out,
                         int64_t& sums_off) {
  classes.clear(); out.assign((size_t)n_mats, MuonLargeMat{});
  std::vector<int> slot((size_t)n_mats, 0);
  int64_t nsum = 0;
  for (int32_t j = 0; j < n_mats; ++j) {
    const int rows = mats[j].rows, cols = mats[j].cols, d = rows < cols ? rows : cols, L = rows < cols ? cols : rows;
    size_t c = 0;
    while (c < classes.size() && !(classes[c].d == d && classes[c].L == L)) ++c;
    if (c == classes.size()) { MuonLargeClass k{}; k.d = d; k.L = L; classes.push_back(k); }
    slot[j] = classes[c].count++;
    out[j].range = mats[j].range; out[j].rows = rows; out[j].cols = cols; out[j].cls = (int32_t)c;
    out[j].sum0 = nsum;
    nsum += ((int64_t)rows * cols + OPT_BLOCK - 1) / OPT_BLOCK;
  }
  size_t at = 2 * MUONL_VEC_BYTES;                           // the constant vectors a and b
  sums_off = (int64_t)at;
  at += round16((size_t)(nsum > 0 ? nsum : 1) * sizeof(double));
  for (MuonLargeClass& k : classes) {
    const size_t ybytes = (size_t)k.count * r4(k.d) * r4(k.L) * sizeof(float), abytes = (size_t)k.count * k.d * r4(k.d) * sizeof(float);
    k.ksplit = muonl_ksplit(k.d, k.L, k.count);
    k.y0 = (int64_t)at; at += ybytes;
    k.y1 = (int64_t)at; at += ybytes;
    k.a = (int64_t)at; at += abytes;
    k.b = (int64_t)at; at += abytes;
    k.slabs = 0;
    if (k.ksplit > 1) { k.slabs = (int64_t)at; at += (size_t)k.ksplit * k.count * k.d * k.d * sizeof(float); }
  }
  for (int32_t j = 0; j < n_mats; ++j) {
    const MuonLargeClass& k = classes[(size_t)out[j].cls];
    const int64_t ys = (int64_t)r4(k.d) * r4(k.L) * sizeof(float), as = (int64_t)k.d * r4(k.d) * sizeof(float);
    out[j].y0 = k.y0 + slot[j] * ys; out[j].y1 = k.y1 + slot[j] * ys;
    out[j].a = k.a + slot[j] * as; out[j].b = k.b + slot[j] * as;
  }
  return round16(at);
}

// what the list must satisfy; `small` (or NULL): the list of the one-workgroup kernel, whose ranges may not be named again
static int muonl_check_list(const char* who, const avmoe_opt_range* ranges, int32_t n_ranges, const avmoe_opt_muon_mat* mats, int32_t n_mats,
                            const avmoe_opt_muon_mat* small, int32_t n_small, std::vector<int32_t>* map_out) {
  if (n_ranges < 0 || n_mats < 0 || n_small < 0) { set_last_error("%s: negative range / matrix count", who); return ERR_BAD_ARG; }
  if (n_mats > 0 && !mats) { set_last_error("%s: mats is NULL", who); return ERR_BAD_ARG; }
  if (n_small > 0 && !small) { set_last_error("%s: the small list is NULL", who); return ERR_BAD_ARG; }
  std::vector<int32_t> map((size_t)n_ranges, -1);
  std::vector<char> in_small((size_t)n_ranges, 0);
  for (int32_t j = 0; j < n_small; ++j)
    if (small[j].range >= 0 && small[j].range < n_ranges) in_small[(size_t)small[j].range] = 1;
  for (int32_t j = 0; j < n_mats; ++j) {
    const avmoe_opt_muon_mat& m = mats[j];
    if (m.range < 0 || m.range >= n_ranges) { set_last_error("%s: matrix %d names range %d of %d", who, (int)j, (int)m.range, (int)n_ranges); return ERR_BAD_ARG; }
    if (m.rows < 1 || m.cols < 1) { set_last_error("%s: matrix %d is %d x %d", who, (int)j, (int)m.rows, (int)m.cols); return ERR_BAD_ARG; }
    if ((m.rows < m.cols ? m.rows : m.cols) > AVMOE_MUON_LARGE_MAX_DIM) {
      set_last_error("%s: matrix %d is %d x %d: its short side is above %d", who, (int)j, (int)m.rows, (int)m.cols, AVMOE_MUON_LARGE_MAX_DIM); return ERR_BAD_ARG;
    }
    if ((int64_t)m.rows * m.cols > (int64_t)INT32_MAX) { set_last_error("%s: matrix %d is %d x %d: too many elements", who, (int)j, (int)m.rows, (int)m.cols); return ERR_BAD_ARG; }
    if (ranges && (int64_t)m.rows * m.cols != ranges[m.range].n) {
      set_last_error("%s: matrix %d is %d x %d, its range %d has %lld elements", who, (int)j, (int)m.rows, (int)m.cols, (int)m.range,
                     (long long)ranges[m.range].n);
      return ERR_BAD_ARG;
    }
    if (map[(size_t)m.range] >= 0) { set_last_error("%s: range %d is named twice (matrices %d and %d)", who, (int)m.range, (int)map[(size_t)m.range], (int)j); return ERR_BAD_ARG; }
    if (in_small[(size_t)m.range]) { set_last_error("%s: range %d is named twice (matrix %d and the small list)", who, (int)m.range, (int)j); return ERR_BAD_ARG; }
    map[(size_t)m.range] = j;
  }
  if (map_out) map_out->swap(map);
  return OK;
}

struct MuonLargeView {            // a checked image, as a kernel sees it
  MuonLargeHeader h;
  const MuonLargeMat* mats;
  const MuonLargeClass* classes;
};

__host__ __device__ inline bool muonl_view(const void* image, int n_mats, MuonLargeView& v) {
  v.h = *(const MuonLargeHeader*)image;
  if (v.h.magic != MUONL_MAGIC || v.h.n_mats != n_mats || v.h.n_classes < 0 || v.h.n_ranges < 0) return false;
  v.mats = (const MuonLargeMat*)((const char*)image + sizeof(MuonLargeHeader));
  v.classes = (const MuonLargeClass*)(v.mats + n_mats);
  return true;
}

// the blocks of range `range` in the table's map (the search of kk_opt_muon_ns): -> false where the table is not this launch's
__device__ __forceinline__ bool muonl_range_blocks(const void* table, int n_ranges, long n_blocks, int range, long n, avmoe_opt_range& r, long& lo, long& nb) {
  const OptHeader h = *(const OptHeader*)table;
  if (h.magic != OPT_MAGIC || h.n_ranges != n_ranges || h.n_blocks != n_blocks || range < 0 || range >= n_ranges) return false;
  const avmoe_opt_range* ranges = (const avmoe_opt_range*)((const char*)table + sizeof(OptHeader));
  const OptBlock* map = (const OptBlock*)(ranges + n_ranges);
  r = ranges[range];
  if (r.n != n) return false;
  nb = (n + OPT_BLOCK - 1) / OPT_BLOCK;
  lo = 0;
  long hi = n_blocks;
  while (lo < hi) {
    const long mid = (lo + hi) >> 1;
    if (map[mid].range < range) lo = mid + 1; else hi = mid;
  }
  return lo + nb <= n_blocks && map[lo].range == range && map[lo + nb - 1].range == range;
}

struct MuonLargeStep {            // what the STEP instantiations need beyond the image
  const void* table;
  const avmoe_opt_state* state;
  const double* sums;             // the table walk's block sums
  float* const* shadows;
  float* const* hold;
  void* report;
  long n_blocks;
  int n_ranges, scale, ns_steps;
};

// avmoe_opt_muon_ns_large: the sums of (double)x^2 over the 1024-element blocks of every matrix, as the table walk leaves them
__global__ void __launch_bounds__(256) kk_opt_muon_large_sumsq(const void* __restrict__ image, int n_mats, float* const* __restrict__ work,
                                                               char* __restrict__ ws) {
  MuonLargeView v;
  if (!muonl_view(image, n_mats, v) || (int)gridDim.y != n_mats) return;
  const MuonLargeMat mt = v.mats[blockIdx.y];
  if (mt.range < 0 || mt.range >= v.h.n_ranges || mt.rows < 1 || mt.cols < 1) return;
  const float* __restrict__ X = work[mt.range];
  if (!X || ((uintptr_t)X & 15u) != 0) return;
  const long n = (long)mt.rows * mt.cols, nb = (n + OPT_BLOCK - 1) / OPT_BLOCK;
  double* sums = (double*)(ws + v.h.sums_off) + mt.sum0;
  for (long blk = blockIdx.x; blk < nb; blk += gridDim.x) {
    const long i0 = (blk * 256 + threadIdx.x) * 4;
    double su = 0.0;
    for (long i = i0; i < i0 + 4 && i < n; ++i) { const double x = (double)X[i]; su += x * x; }
    const double t = block_sum_256(su);
    if (threadIdx.x == 0) sums[blk] = t;
    __syncthreads();                                         // the tree's words are free again
  }
}

// One launch for all large matrices: block (x, y) serves tiles x, x + gridDim.x, ... of matrix y.  Every block of a matrix adds the
// matrix's block sums itself, in one fixed order (thread t: blocks t, t + 256, ..., then a tree), so all of them hold the same inv.
template <bool STEP>
__global__ void __launch_bounds__(256) kk_opt_muon_large_pack(const void* __restrict__ image, int n_mats, float* const* __restrict__ work,
                                                              char* __restrict__ ws, MuonLargeStep sa) {
  __shared__ double red[256];
  __shared__ float tile[MUONL_TILE][MUONL_TILE + 1];
  if constexpr (STEP) {
    if (sa.state->skip) return;
  }
  MuonLargeView v;
  if (!muonl_view(image, n_mats, v) || (int)gridDim.y != n_mats) return;
  const MuonLargeMat mt = v.mats[blockIdx.y];
  if (mt.range < 0 || mt.range >= v.h.n_ranges || mt.rows < 1 || mt.cols < 1 || mt.cls < 0 || mt.cls >= v.h.n_classes) return;
  const int rows = mt.rows, cols = mt.cols;
  const bool wide = rows <= cols;
  const int d = wide ? rows : cols, L = wide ? cols : rows;
  if (d > AVMOE_MUON_LARGE_MAX_DIM) return;
  const int d4 = (d + 3) & ~3, L4 = (L + 3) & ~3;
  const int ti_n = (d4 + MUONL_TILE - 1) / MUONL_TILE, tl_n = (L4 + MUONL_TILE - 1) / MUONL_TILE;
  const long tiles = (long)ti_n * tl_n;
  if ((long)blockIdx.x >= tiles) return;                     // (block 0 of a matrix always has a tile)
  const long n = (long)rows * cols;
  const float* __restrict__ X = work[mt.range];
  if (!X || ((uintptr_t)X & 15u) != 0) return;
  const int tid = threadIdx.x;

  const double* sums;
  long nb = (n + OPT_BLOCK - 1) / OPT_BLOCK;
  if constexpr (STEP) {
    if (v.h.n_ranges != sa.n_ranges) return;
    avmoe_opt_range r;
    long lo;
    if (!muonl_range_blocks(sa.table, sa.n_ranges, sa.n_blocks, mt.range, n, r, lo, nb)) return;
    sums = sa.sums + lo;
  } else {
    sums = (const double*)(ws + v.h.sums_off) + mt.sum0;
  }
  double acc = 0.0;
  for (long i = tid; i < nb; i += 256) acc += sums[i];
  red[tid] = acc;
  __syncthreads();
#pragma unroll
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  const double nrm = sqrt(red[0]);
  const float inv = (float)(1.0 / (nrm + 1e-7));

  float* __restrict__ Y0 = (float*)(ws + mt.y0);
  float* __restrict__ Y1 = (float*)(ws + mt.y1);
  if (blockIdx.x == 0) {
    if constexpr (STEP) {
      if (tid == 0) {
        if (blockIdx.y == 0) *(int4*)sa.report = make_int4(n_mats, 0, 0, 0);
        ((float*)sa.report)[4 + blockIdx.y] = (float)nrm;
      }
    }
    if (d4 > d) {                                            // the padding columns of A and B: the engine writes d columns only
      float* A = (float*)(ws + mt.a); float* B = (float*)(ws + mt.b);
      const int pad = d4 - d;
      for (int e = tid; e < d * pad; e += 256) {
        const int i = e / pad, j = d + e - i * pad;
        A[i * d4 + j] = 0.f; B[i * d4 + j] = 0.f;
      }
    }
    if (blockIdx.y == 0) {                                   // the row_scale vectors of the two epilogues
      float* va = (float*)ws; float* vb = va + AVMOE_MUON_LARGE_MAX_DIM;
      for (int e = tid; e < AVMOE_MUON_LARGE_MAX_DIM; e += 256) { va[e] = MUONL_A; vb[e] = MUONL_B; }
    }
  }

  const int tx = tid & 31, ty = tid >> 5;
  for (long t = blockIdx.x; t < tiles; t += gridDim.x) {
    const int i0 = (int)(t / tl_n) * MUONL_TILE, l0 = (int)(t % tl_n) * MUONL_TILE;
    if (!wide) {                                             // element (i, l) of the view is X[l * cols + i]: consecutive threads along i
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int l = l0 + ty + 8 * k, i = i0 + tx;
        tile[ty + 8 * k][tx] = (i < d && l < L) ? X[(long)l * cols + i] : 0.f;
      }
      __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int i = i0 + ty + 8 * k, l = l0 + tx;
      if (i < d4 && l < L4) {
        const bool in = i < d && l < L;
        float x = 0.f;
        if (in) x = (wide ? X[(long)i * cols + l] : tile[tx][ty + 8 * k]) * inv;
        Y0[(long)i * L4 + l] = x;
        if (!in) Y1[(long)i * L4 + l] = 0.f;                 // the engine writes d rows of L columns only
      }
    }
    if (!wide) __syncthreads();
  }
}

// f(index into the range, O) for every element of the matrix, O read from the d4 x L4 staging image Y; tall matrices go through a
// 32 x 32 LDS tile so that both sides move along their contiguous index
template <typename F>
__device__ __forceinline__ void muonl_unpack(const float* __restrict__ Y, int rows, int cols, float (&tile)[MUONL_TILE][MUONL_TILE + 1], F f) {
  const bool wide = rows <= cols;
  const int d = wide ? rows : cols, L = wide ? cols : rows, L4 = (L + 3) & ~3;
  const int tl_n = (L + MUONL_TILE - 1) / MUONL_TILE;
  const long tiles = (long)((d + MUONL_TILE - 1) / MUONL_TILE) * tl_n;
  const int tid = threadIdx.x, tx = tid & 31, ty = tid >> 5;
  for (long t = blockIdx.x; t < tiles; t += gridDim.x) {
    const int i0 = (int)(t / tl_n) * MUONL_TILE, l0 = (int)(t % tl_n) * MUONL_TILE;
    if (wide) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int i = i0 + ty + 8 * k, l = l0 + tx;
        if (i < d && l < L) f((long)i * cols + l, Y[(long)i * L4 + l]);
      }
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int i = i0 + ty + 8 * k, l = l0 + tx;
        tile[ty + 8 * k][tx] = (i < d && l < L) ? Y[(long)i * L4 + l] : 0.f;
      }
      __syncthreads();
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int l = l0 + ty + 8 * k, i = i0 + tx;
        if (i < d && l < L) f((long)l * cols + i, tile[tx][ty + 8 * k]);
      }
      __syncthreads();
    }
  }
}

// avmoe_opt_muon_ns_large: O from the staging buffer the last iteration wrote into the work buffers, nothing else
__global__ void __launch_bounds__(256) kk_opt_muon_large_unpack(const void* __restrict__ image, int n_mats, float* const* __restrict__ work,
                                                                const char* __restrict__ ws, int ns_steps) {
  __shared__ float tile[MUONL_TILE][MUONL_TILE + 1];
  MuonLargeView v;
  if (!muonl_view(image, n_mats, v) || (int)gridDim.y != n_mats) return;
  const MuonLargeMat mt = v.mats[blockIdx.y];
  if (mt.range < 0 || mt.range >= v.h.n_ranges || mt.rows < 1 || mt.cols < 1) return;
  if ((mt.rows < mt.cols ? mt.rows : mt.cols) > AVMOE_MUON_LARGE_MAX_DIM) return;
  float* __restrict__ X = work[mt.range];
  if (!X || ((uintptr_t)X & 15u) != 0) return;
  const float* Y = (const float*)(ws + ((ns_steps & 1) ? mt.y1 : mt.y0));
  muonl_unpack(Y, mt.rows, mt.cols, tile, [&](long idx, float o) { X[idx] = o; });
}

// One launch for all large matrices, behind the engine: O into work[range], decay and update of the parameter (HOLD: read from the hold
// buffer), the shadow.  lr, s and step as kk_opt_muon_ns forms them.  A skipped step writes nothing here: under HOLD the table walk has
// already written param = hold for every range.
template <bool DECOUPLED, bool SCHED, bool EMA, bool HOLD>
__global__ void __launch_bounds__(256) kk_opt_muon_large_apply(const void* __restrict__ image, int n_mats, float* const* __restrict__ work,
                                                               const char* __restrict__ ws, MuonLargeStep sa) {
  __shared__ float tile[MUONL_TILE][MUONL_TILE + 1];
  if (sa.state->skip) return;
  MuonLargeView v;
  if (!muonl_view(image, n_mats, v) || (int)gridDim.y != n_mats || v.h.n_ranges != sa.n_ranges) return;
  const MuonLargeMat mt = v.mats[blockIdx.y];
  if (mt.range < 0 || mt.range >= v.h.n_ranges || mt.rows < 1 || mt.cols < 1) return;
  const int rows = mt.rows, cols = mt.cols;
  if ((rows < cols ? rows : cols) > AVMOE_MUON_LARGE_MAX_DIM) return;
  avmoe_opt_range r;
  long lo, nb;
  if (!muonl_range_blocks(sa.table, sa.n_ranges, sa.n_blocks, mt.range, (long)rows * cols, r, lo, nb)) return;
  float* __restrict__ X = work[mt.range];
  if (!X || ((uintptr_t)X & 15u) != 0) return;
  float* __restrict__ param = r.param;
  const float* __restrict__ src = r.param;
  if constexpr (HOLD) {
    src = sa.hold[mt.range];
    if (!src || ((uintptr_t)src & 15u) != 0) return;
  }
  float* __restrict__ ema = nullptr;
  float decay = 0.f;
  if constexpr (EMA) {
    ema = sa.shadows[mt.range];
    if (!ema || ((uintptr_t)ema & 15u) != 0) return;
    decay = sa.state->ema_decay;
  }
  float lr = r.lr;
  if constexpr (SCHED) lr *= sa.state->lr_factor;
  const float wd = r.weight_decay;
  const double big = (double)(rows > cols ? rows : cols);
  const float s = sa.scale == AVMOE_MUON_SCALE_ORIGINAL ? (float)sqrt(fmax(1.0, (double)rows / (double)cols)) : (float)(0.2 * sqrt(big));
  const float step = lr * s;
  const float* Y = (const float*)(ws + ((sa.ns_steps & 1) ? mt.y1 : mt.y0));
  muonl_unpack(Y, rows, cols, tile, [&](long idx, float o) {
    X[idx] = o;
    const float pn = muon_next(src[idx], o, lr, wd, step, DECOUPLED);
    param[idx] = pn;
    if constexpr (EMA) ema[idx] = ema_next(ema[idx], pn, decay);
  });
}

using MuonLargeApplyKernel = decltype(&kk_opt_muon_large_apply<false, false, false, false>);
constexpr MuonLargeApplyKernel OPT_MUON_LARGE_APPLY[16] = {           // [DECOUPLED | SCHED << 1 | EMA << 2 | HOLD << 3]
    kk_opt_muon_large_apply<false, false, false, false>, kk_opt_muon_large_apply<true, false, false, false>,
    kk_opt_muon_large_apply<false, true, false, false>,  kk_opt_muon_large_apply<true, true, false, false>,
    kk_opt_muon_large_apply<false, false, true, false>,  kk_opt_muon_large_apply<true, false, true, false>,
    kk_opt_muon_large_apply<false, true, true, false>,   kk_opt_muon_large_apply<true, true, true, false>,
    kk_opt_muon_large_apply<false, false, false, true>,  kk_opt_muon_large_apply<true, false, false, true>,
    kk_opt_muon_large_apply<false, true, false, true>,   kk_opt_muon_large_apply<true, true, false, true>,
    kk_opt_muon_large_apply<false, false, true, true>,   kk_opt_muon_large_apply<true, false, true, true>,
    kk_opt_muon_large_apply<false, true, true, true>,    kk_opt_muon_large_apply<true, true, true, true>};

// what both launching calls refuse about the large image, its host copy and the workspace
static int muonl_check_args(const char* who, const void* large, const void* large_host, int32_t n_large, int32_t n_ranges, const void* ws,
                            MuonLargeView& v) {
  if (!large) { set_last_error("%s: the large image is NULL", who); return ERR_BAD_ARG; }
  if (!large_host) { set_last_error("%s: the host copy of the large image is NULL", who); return ERR_BAD_ARG; }
  if (!ws) { set_last_error("%s: the large workspace is NULL", who); return ERR_BAD_ARG; }
  if (n_large < 0) { set_last_error("%s: negative large matrix count %d", who, (int)n_large); return ERR_BAD_ARG; }
  if (((uintptr_t)large & 15u) != 0 || ((uintptr_t)large_host & 7u) != 0) { set_last_error("%s: the large image must be 16-byte aligned", who); return ERR_ALIGNMENT; }
  if (((uintptr_t)ws & 15u) != 0) { set_last_error("%s: the large workspace must be 16-byte aligned", who); return ERR_ALIGNMENT; }
  if (!muonl_view(large_host, n_large, v) || (n_ranges >= 0 && v.h.n_ranges != n_ranges)) {
    set_last_error("%s: the host copy of the large image is not one of %d matrices and %d ranges", who, (int)n_large, (int)n_ranges); return ERR_BAD_ARG;
  }
  return OK;
}

static unsigned muonl_grid_x(const MuonLargeView& v) {
  long most = 1;
  for (int32_t j = 0; j < v.h.n_mats; ++j) {
    const int d = v.mats[j].rows < v.mats[j].cols ? v.mats[j].rows : v.mats[j].cols, L = v.mats[j].rows < v.mats[j].cols ? v.mats[j].cols : v.mats[j].rows;
    const long t = (long)cdiv(r4(d), MUONL_TILE) * cdiv(r4(L), MUONL_TILE);
    most = t > most ? t : most;
  }
  most = (most + 3) / 4;                                      // about four tiles per block
  return (unsigned)(most > MUONL_MAX_GX ? MUONL_MAX_GX : most);
}

// the engine sequence: per class, ns_steps times  A = Y Y^T ;  B = c (A A^T) + b A ;  Y' = B Y + a Y  (Y and Y' the two staging buffers in turn)
static int muonl_iterate(const MuonLargeView& v, char* ws, int ns_steps, hipStream_t stream) {
  const float* va = (const float*)ws;
  const float* vb = va + AVMOE_MUON_LARGE_MAX_DIM;
  for (int32_t c = 0; c < v.h.n_classes; ++c) {
    const MuonLargeClass& k = v.classes[c];
    const int d = k.d, L = k.L, d4 = r4(d), L4 = r4(L);
    const long ys = (long)d4 * L4, as = (long)d * d4;
    float* Y[2] = {(float*)(ws + k.y0), (float*)(ws + k.y1)};
    float* A = (float*)(ws + k.a);
    float* B = (float*)(ws + k.b);
    for (int it = 0; it < ns_steps; ++it) {
      const float* Yc = Y[it & 1];
      float* Yn = Y[(it + 1) & 1];
      GemmArgs g;                                            // A = Y Y^T
      g.dtype = GEMM_F32; g.split3 = 1; g.nb1 = k.count;
      g.A = Yc; g.B = Yc; g.K = L; g.a_layout = K_MAJOR; g.b_layout = K_MAJOR; g.lda = g.ldb = L4; g.sA1 = g.sB1 = ys;
      g.C = A; g.M = g.N = d; g.sCi = d4; g.sCj = 1; g.sC1 = as;
      if (k.ksplit > 1) { g.ksplit = k.ksplit; g.slabs = (float*)(ws + k.slabs); }
      AVMOE_TRY(launch_gemm(g, stream));
      GemmArgs h;                                            // B = c (A A^T) + b A
      h.dtype = GEMM_F32; h.split3 = 1; h.nb1 = k.count;
      h.A = A; h.B = A; h.K = d; h.a_layout = K_MAJOR; h.b_layout = K_MAJOR; h.lda = h.ldb = d4; h.sA1 = h.sB1 = as;
      h.C = B; h.M = h.N = d; h.sCi = d4; h.sCj = 1; h.sC1 = as;
      h.alpha = MUONL_C; h.row_scale = vb; h.D = A; h.sDi = d4; h.sD1 = as;
      AVMOE_TRY(launch_gemm(h, stream));
      GemmArgs y;                                            // Y' = B Y + a Y
      y.dtype = GEMM_F32; y.split3 = 1; y.nb1 = k.count;
      y.A = B; y.a_layout = K_MAJOR; y.lda = d4; y.sA1 = as;
      y.B = Yc; y.b_layout = MN_MAJOR; y.ldb = L4; y.sB1 = ys; y.K = d;
      y.C = Yn; y.M = d; y.N = L; y.sCi = L4; y.sCj = 1; y.sC1 = ys;
      y.row_scale = va; y.D = Yc; y.sDi = L4; y.sD1 = ys;
      AVMOE_TRY(launch_gemm(y, stream));
    }
  }
  return OK;
}

}  // namespace avmoe

using namespace avmoe;

extern "C" {

size_t avmoe_opt_muon_large_bytes(int32_t n_ranges, const avmoe_opt_muon_mat* mats, int32_t n_mats, avmoe_opt_muon_large_layout* layout) {
  const char* who = "avmoe_opt_muon_large_bytes";
  if (n_mats > n_ranges) { set_last_error("%s: bad range / matrix count %d / %d", who, (int)n_ranges, (int)n_mats); return 0; }
  if (muonl_check_list(who, nullptr, n_ranges, mats, n_mats, nullptr, 0, nullptr) != OK) return 0;
  std::vector<MuonLargeClass> classes;
  std::vector<MuonLargeMat> out;
  int64_t sums_off;
  avmoe_opt_muon_large_layout l;
  l.workspace_bytes = muonl_plan(mats, n_mats, classes, out, sums_off);
  l.table_bytes = muonl_image_bytes(n_ranges, n_mats, (int32_t)classes.size());
  l.report_bytes = 16 + round16((size_t)(n_mats > 0 ? n_mats : 1) * sizeof(float));
  l.n_classes = (int32_t)classes.size(); l.reserved = 0;
  if (layout) *layout = l;
  return l.table_bytes + l.workspace_bytes + l.report_bytes;
}

int avmoe_opt_muon_large_table_build(const avmoe_opt_range* ranges, int32_t n_ranges, const avmoe_opt_muon_mat* mats, int32_t n_mats,
                                     const avmoe_opt_muon_mat* small, int32_t n_small, void* image, size_t image_bytes) {
  const char* who = "avmoe_opt_muon_large_table_build";
  if (!image) { set_last_error("%s: image is NULL", who); return ERR_BAD_ARG; }
  std::vector<int32_t> map;
  AVMOE_TRY(muonl_check_list(who, ranges, n_ranges, mats, n_mats, small, n_small, &map));
  std::vector<MuonLargeClass> classes;
  std::vector<MuonLargeMat> out;
  MuonLargeHeader h{};
  h.ws_bytes = (int64_t)muonl_plan(mats, n_mats, classes, out, h.sums_off);
  h.magic = MUONL_MAGIC; h.n_mats = n_mats; h.n_ranges = n_ranges; h.n_classes = (int32_t)classes.size();
  const size_t need = muonl_image_bytes(n_ranges, n_mats, h.n_classes);
  if (image_bytes < need) { set_last_error("%s: image of %zu bytes, %zu needed", who, image_bytes, need); return ERR_WORKSPACE; }
  char* p = (char*)image;
  memset(p, 0, need);
  memcpy(p, &h, sizeof h); p += sizeof h;
  if (n_mats > 0) memcpy(p, out.data(), (size_t)n_mats * sizeof(MuonLargeMat));
  p += (size_t)n_mats * sizeof(MuonLargeMat);
  if (!classes.empty()) memcpy(p, classes.data(), classes.size() * sizeof(MuonLargeClass));
  p += classes.size() * sizeof(MuonLargeClass);
  if (n_ranges > 0) memcpy(p, map.data(), (size_t)n_ranges * sizeof(int32_t));
  return OK;
}

int avmoe_opt_muon_large_classes(const void* image, avmoe_opt_muon_class* out, int32_t cap, int32_t* cls_of) {
  const char* who = "avmoe_opt_muon_large_classes";
  if (!image) { set_last_error("%s: image is NULL", who); return ERR_BAD_ARG; }
  MuonLargeHeader h;
  memcpy(&h, image, sizeof h);
  MuonLargeView v;
  if (h.magic != MUONL_MAGIC || h.n_mats < 0 || !muonl_view(image, h.n_mats, v)) { set_last_error("%s: not a large matrix image", who); return ERR_BAD_ARG; }
  for (int32_t c = 0; out && c < v.h.n_classes && c < cap; ++c) out[c] = avmoe_opt_muon_class{v.classes[c].d, v.classes[c].L, v.classes[c].count, v.classes[c].ksplit};
  for (int32_t j = 0; cls_of && j < v.h.n_mats; ++j) cls_of[j] = v.mats[j].cls;
  return v.h.n_classes;
}

int avmoe_opt_muon_step_large(const void* table, int32_t n_ranges, int64_t n_blocks, const avmoe_opt_state* state, float beta1, float beta2, float eps,
                              float grad_scale, int32_t flags, void* stream, float* const* shadows, float* const* hold, const void* mats, int32_t n_mats,
                              float* const* work, const avmoe_opt_muon* consts, double* workspace, void* report, const void* large,
                              const void* large_host, int32_t n_large, void* large_workspace, void* large_report) {
  const char* who = "avmoe_opt_muon_step_large";
  AVMOE_TRY(muon_step_check(who, table, n_ranges, n_blocks, state, beta1, beta2, eps, grad_scale, flags, shadows, hold, mats, n_mats, work, consts,
                            workspace, report));
  if (!large_report) { set_last_error("%s: the large report buffer is NULL", who); return ERR_BAD_ARG; }
  MuonLargeView v;
  AVMOE_TRY(muonl_check_args(who, large, large_host, n_large, n_ranges, large_workspace, v));
  if (((uintptr_t)large_report & 15u) != 0) { set_last_error("%s: the large report buffer must be 16-byte aligned", who); return ERR_ALIGNMENT; }
  const hipStream_t st = (hipStream_t)stream;
  AVMOE_TRY(muon_step_launch(who, table, n_ranges, n_blocks, state, beta1, beta2, eps, grad_scale, flags, st, shadows, hold, mats, n_mats, work,
                             consts, workspace, report, n_large > 0 ? large : nullptr, n_large));
  if (n_large == 0 || n_blocks <= 0) return OK;
  const bool dec = (flags & AVMOE_OPT_DECOUPLED_DECAY) != 0, sched = (flags & AVMOE_OPT_LR_SCHEDULE) != 0, ema = (flags & AVMOE_OPT_EMA) != 0;
  MuonLargeStep sa;
  sa.table = table; sa.state = state; sa.sums = workspace; sa.shadows = ema ? shadows : nullptr; sa.hold = hold; sa.report = large_report;
  sa.n_blocks = (long)n_blocks; sa.n_ranges = (int)n_ranges; sa.scale = (int)consts->scale; sa.ns_steps = (int)consts->ns_steps;
  const dim3 grid(muonl_grid_x(v), (unsigned)n_large);
  hipLaunchKernelGGL(kk_opt_muon_large_pack<true>, grid, dim3(256), 0, st, large, (int)n_large, work, (char*)large_workspace, sa);
  AVMOE_CHECK_LAUNCH("opt_muon_large_pack");
  AVMOE_TRY(muonl_iterate(v, (char*)large_workspace, (int)consts->ns_steps, st));
  hipLaunchKernelGGL(OPT_MUON_LARGE_APPLY[(int)dec | (int)sched << 1 | (int)ema << 2 | (int)(hold != nullptr) << 3], grid, dim3(256), 0, st, large,
                     (int)n_large, work, (const char*)large_workspace, sa);
  AVMOE_CHECK_LAUNCH("opt_muon_large_apply");
  return OK;
}

int avmoe_opt_muon_ns_large(const void* large, const void* large_host, int32_t n_large, float* const* work, int32_t ns_steps, void* large_workspace,
                            void* stream) {
  const char* who = "avmoe_opt_muon_ns_large";
  if (!work) { set_last_error("%s: the work pointer array is NULL", who); return ERR_BAD_ARG; }
  if (ns_steps < 1 || ns_steps > 16) { set_last_error("%s: ns_steps must be in 1..16, not %d", who, (int)ns_steps); return ERR_BAD_ARG; }
  MuonLargeView v;
  AVMOE_TRY(muonl_check_args(who, large, large_host, n_large, -1, large_workspace, v));
  if (((uintptr_t)work & 7u) != 0) { set_last_error("%s: the work pointer array must be 8-byte aligned", who); return ERR_ALIGNMENT; }
  if (n_large == 0) return OK;
  const hipStream_t st = (hipStream_t)stream;
  const dim3 grid(muonl_grid_x(v), (unsigned)n_large);
  hipLaunchKernelGGL(kk_opt_muon_large_sumsq, grid, dim3(256), 0, st, large, (int)n_large, work, (char*)large_workspace);
  AVMOE_CHECK_LAUNCH("opt_muon_large_sumsq");
  hipLaunchKernelGGL(kk_opt_muon_large_pack<false>, grid, dim3(256), 0, st, large, (int)n_large, work, (char*)large_workspace, MuonLargeStep{});
  AVMOE_CHECK_LAUNCH("opt_muon_large_pack");
  AVMOE_TRY(muonl_iterate(v, (char*)large_workspace, (int)ns_steps, st));
  hipLaunchKernelGGL(kk_opt_muon_large_unpack, grid, dim3(256), 0, st, large, (int)n_large, work, (const char*)large_workspace, (int)ns_steps);
  AVMOE_CHECK_LAUNCH("opt_muon_large_unpack");
  return OK;
}

}  // extern "C"
