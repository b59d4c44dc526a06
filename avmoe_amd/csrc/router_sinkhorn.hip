// Sinkhorn-balanced top-k routing (avmoe_moe_forward_sinkhorn / avmoe_router_sinkhorn, include/avmoe.h; S-BASE, Clark et al. 2022; BASE
// layers, Lewis et al. 2021): the call's (S, E) softmax p is balanced by n rounds of row / column normalisation,
//   v = 1 ;  n times:  u_s = 1 / sum_e p[s, e] v_e ,  v_e = (S / E) / sum_s p[s, e] u_s ,
// and every frame takes the k experts with the largest q[s, e] = p[s, e] v_e.  u_s does not change a row's ranking, so the E words v are
// all the first launch produces; the second one and the router backward evaluate the selection per frame from them (topk_select_scaled).
//   kk_sk_scale   ONE block of up to 1024 threads, the n rounds in one launch.  Thread t owns the frames t, t + blockDim, ... and takes them
//                 in frame order: the row step is local to a frame (u_s from its E values and v), and the frame's share p[s, e] u_s goes
//                 into E column partials the thread keeps in registers.  A round ends with the block's column sums: a butterfly of
//                 shuffles within the wave, the wave totals through the LDS, added in wave order by one thread per expert.  Every sum has
//                 one fixed order: the same input gives the same bits on every call.  No cooperative launch, no waiting on another
//                 block, no floating-point atomics.
//                 p stays in the LDS between the rounds while its image fits (SK_LDS_CAP of the CU's 160 KB, the reduction scratch
//                 beside it); a larger p -- at most 1.3 MB, L2-resident -- is read again from global memory every round.  A thread reads
//                 back only the rows it wrote itself, with ds_read_b32 at a lane stride of one row: the rows are `ld` = E | 1 floats
//                 apart, an ODD number of banks, so the 32 lanes of a group hit 32 different banks (rows of E = 16 floats put them on
//                 two: 16-way).
//   kk_sk_apply   one thread per frame: q, the mask, kept_s from the UNSCALED p in expert order, the weights (times mix), the bitmask word
//                 and the per-expert counts of the selection: ballot and popcount per wave, wave totals by LDS integer adds, one integer
//                 global add per expert and block into the words kk_sk_scale cleared -- integer counts do not depend on arrival order.
// A column whose sum is 0 (the softmax underflowed in every frame) gets the largest finite fp32: v is never Inf or NaN, and 0 * v = 0
// keeps such a column last.  Every access is guarded by s < S and e < E.
#include "../../include/avmoe.h"
#include "common.h"
#include "device_utils.h"
#include "kernels.h"
#include <hip/hip_runtime.h>
#include <cfloat>
#include <climits>
#include <cstdint>

namespace avmoe {

namespace {

constexpr int SK_WAVES = 16;                               // of a 1024-thread block
constexpr int SK_RED = SK_WAVES * MAX_E + MAX_E;           // floats of reduction scratch: the wave totals [wave][e], then v
constexpr int SK_LDS_CAP = 152 * 1024;                     // bytes: scratch + the image of p, of the CU's 160 KB

// the E values of one frame into registers (0 beyond E).  vec: E == EP, a multiple of 4, and p is 16-byte aligned -- whole 16-byte loads
template <int EP>
__device__ __forceinline__ void sk_load_row(const float* row, int E, bool vec, float (&r)[EP]) {
  if constexpr (EP >= 4) {
    if (vec) {
#pragma unroll
      for (int j = 0; j < EP / 4; ++j) {
        const float4 x = ((const float4*)row)[j];
        r[4 * j] = x.x; r[4 * j + 1] = x.y; r[4 * j + 2] = x.z; r[4 * j + 3] = x.w;
      }
      return;
    }
  }
#pragma unroll
  for (int e = 0; e < EP; ++e) r[e] = e < E ? row[e] : 0.f;
}

// EP: E rounded up to 2, 4, 8 or 16 -- the partials and v are register arrays with compile-time indices.  ld: the row stride of the LDS
// image in floats, 0 = p does not fit and is read from global memory in every round.
template <int EP>
__global__ void __launch_bounds__(1024) kk_sk_scale(const float* p, long S, int E, int iters, int ld, int* v_bits, int* count) {
  extern __shared__ float sk_lds[];
  float* s_red = sk_lds;
  float* s_v = sk_lds + SK_WAVES * MAX_E;
  float* s_p = sk_lds + SK_RED;
  const int t = threadIdx.x, nt = blockDim.x, lane = t & 63, wv = t >> 6, nw = nt >> 6;   // (nt: a multiple of 64)
  const bool vec = EP >= 4 && E == EP && ((uintptr_t)p & 15) == 0;                       // (uniform over the block)
  if (count && t < E) count[t] = 0;                        // kk_sk_apply, behind this launch on the stream, adds into them
  if (ld)
    for (long s = t; s < S; s += nt) {                     // (no barrier behind it: a thread reads back its own rows only)
      float r[EP];
      sk_load_row<EP>(p + s * E, E, vec, r);
#pragma unroll
      for (int e = 0; e < EP; ++e)
        if (e < E) s_p[(int)s * ld + e] = r[e];
    }
  float v[EP];
#pragma unroll
  for (int e = 0; e < EP; ++e) v[e] = e < E ? 1.f : 0.f;
  const float target = (float)S / (float)E;
  for (int it = 0; it < iters; ++it) {
    float acc[EP];
#pragma unroll
    for (int e = 0; e < EP; ++e) acc[e] = 0.f;
    for (long s = t; s < S; s += nt) {                     // the thread's frames, in frame order
      float r[EP];
      if (ld) {
#pragma unroll
        for (int e = 0; e < EP; ++e) r[e] = e < E ? s_p[(int)s * ld + e] : 0.f;
      } else sk_load_row<EP>(p + s * E, E, vec, r);
      float dot = 0.f;
#pragma unroll
      for (int e = 0; e < EP; ++e) dot += r[e] * v[e];     // row step, in expert order
      const float u = 1.f / dot;
#pragma unroll
      for (int e = 0; e < EP; ++e) acc[e] += r[e] * u;     // column step: this frame's share
    }
#pragma unroll
    for (int e = 0; e < EP; ++e) acc[e] = wave_sum(acc[e]);
    if (lane == 0) {
#pragma unroll
      for (int e = 0; e < EP; ++e)
        if (e < E) s_red[wv * MAX_E + e] = acc[e];
    }
    __syncthreads();
    if (t < E) {                                           // the wave totals in wave order; a sum of 0 (or NaN) gives the largest finite fp32
      float sum = 0.f;
      for (int w = 0; w < nw; ++w) sum += s_red[w * MAX_E + t];
      s_v[t] = fminf(target / sum, FLT_MAX);
    }
    __syncthreads();                                       // (s_red is written again behind this barrier, s_v behind the next round's first)
#pragma unroll
    for (int e = 0; e < EP; ++e)
      if (e < E) v[e] = s_v[e];
  }
  if (t < E) v_bits[t] = __float_as_int(s_v[t]);           // (thread t wrote s_v[t] itself)
}

__global__ void __launch_bounds__(256) kk_sk_apply(const float* p, long S, int E, int k, int renorm, const float* mix, const int* v_bits,
                                                   float* w, int32_t* choice, int* count) {
  __shared__ float s_v[MAX_E];
  __shared__ int s_cnt[MAX_E];
  __shared__ float s_pr[256][MAX_E + 1];                   // one frame's probabilities per thread (+ 1: no bank conflicts)
  const int t = threadIdx.x;
  if (t < E) { s_v[t] = __int_as_float(v_bits[t]); s_cnt[t] = 0; }
  __syncthreads();
  const long s = (long)blockIdx.x * 256 + t;
  unsigned m = 0u;
  if (s < S) {
    float* pr = s_pr[t];
    for (int e = 0; e < E; ++e) pr[e] = p[s * E + e];
    float kept;
    m = topk_select_scaled(pr, s_v, E, k, &kept);
    if (choice) choice[s] = (int32_t)m;
    if (w)
      for (int e = 0; e < E; ++e) {
        float x = ((m >> e) & 1u) ? (renorm ? pr[e] / kept : pr[e]) : 0.f;
        if (mix) x *= mix[s * E + e];
        w[s * E + e] = x;
      }
  }
  if (count) {                                             // (uniform over the grid; every lane of the block gets here: m = 0 beyond S)
    for (int e = 0; e < E; ++e) {
      const unsigned long long b = __ballot((m >> e) & 1u);
      if ((t & 63) == 0 && b) atomicAdd(&s_cnt[e], (int)__popcll(b));
    }
    __syncthreads();
    if (t < E && s_cnt[t]) atomicAdd(&count[t], s_cnt[t]);
  }
}

template <int EP>
int sk_scale_launch(const float* p, long S, int E, int iters, int* v_bits, int* count, hipStream_t st) {
  static LdsAttrOnce attr;
  const int nt = (int)std::min<long>(1024, round_up(S, 64));
  const int ld_fit = E | 1;
  const long image = (long)sizeof(float) * (SK_RED + S * ld_fit);
  const int ld = image <= SK_LDS_CAP ? ld_fit : 0;
  const int lds = ld ? (int)image : (int)sizeof(float) * SK_RED;
  if (lds > 65536) AVMOE_TRY(attr.ensure((const void*)kk_sk_scale<EP>, SK_LDS_CAP, "sinkhorn_scale"));
  hipLaunchKernelGGL(kk_sk_scale<EP>, dim3(1), dim3((unsigned)nt), (size_t)lds, st, p, S, E, iters, ld, v_bits, count);
  AVMOE_CHECK_LAUNCH("sinkhorn_scale");
  return OK;
}

}  // namespace

int k_sk_scale(const float* p, long S, int E, int iters, int* v_bits, int* count, hipStream_t st) {
  if (E <= 2) return sk_scale_launch<2>(p, S, E, iters, v_bits, count, st);
  if (E <= 4) return sk_scale_launch<4>(p, S, E, iters, v_bits, count, st);
  if (E <= 8) return sk_scale_launch<8>(p, S, E, iters, v_bits, count, st);
  return sk_scale_launch<16>(p, S, E, iters, v_bits, count, st);
}

int k_sk_apply(const float* p, long S, int E, int top_k, int renorm, const float* mix, const int* v_bits, float* w, int32_t* choice,
               int* count, hipStream_t st) {
  hipLaunchKernelGGL(kk_sk_apply, dim3((unsigned)cdiv(S, 256)), dim3(256), 0, st, p, S, E, top_k, renorm ? 1 : 0, mix, v_bits, w, choice,
                     count);
  AVMOE_CHECK_LAUNCH("sinkhorn_apply");
  return OK;
}

}  // namespace avmoe

extern "C" int avmoe_router_sinkhorn(const float* p, int64_t S, int32_t E, int32_t top_k, int32_t renorm, int32_t iters,
                                     const float* mix_scale, float* w, int32_t* choice, int32_t* count, float* v, void* stream) {
  using namespace avmoe;
  if (!p || !v) { set_last_error("avmoe_router_sinkhorn: null pointer"); return ERR_BAD_ARG; }
  if (E < 2 || E > MAX_E) { set_last_error("avmoe_router_sinkhorn: E %d not in [2, %d]", (int)E, MAX_E); return ERR_BAD_ARG; }
  if (S < 1 || S > (int64_t)INT_MAX) { set_last_error("avmoe_router_sinkhorn: S %lld not in [1, 2^31)", (long long)S); return ERR_BAD_ARG; }
  if (top_k < 1 || top_k >= E) { set_last_error("avmoe_router_sinkhorn: top_k %d not in [1, %d)", (int)top_k, (int)E); return ERR_BAD_ARG; }
  if (iters < 1 || iters > 64) { set_last_error("avmoe_router_sinkhorn: iters %d not in [1, 64]", (int)iters); return ERR_BAD_ARG; }
  if (w) {
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)w, n = (uintptr_t)S * (uintptr_t)E * sizeof(float);
    if (a < b + n && b < a + n) { set_last_error("avmoe_router_sinkhorn: w overlaps p"); return ERR_BAD_ARG; }
  }
  hipStream_t st = (hipStream_t)stream;
  AVMOE_TRY(k_sk_scale(p, (long)S, (int)E, (int)iters, (int*)v, (int*)count, st));
  if (!w && !choice && !count) return OK;
  return k_sk_apply(p, (long)S, (int)E, (int)top_k, renorm, mix_scale, (const int*)v, w, choice, (int*)count, st);
}
