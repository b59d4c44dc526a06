// Top-p routing (avmoe_moe_forward_top_p / avmoe_router_top_p, include/avmoe.h; "dynamic-k" routing, Huang et al. 2024): every frame takes
// the fewest of its ranked experts whose probability mass reaches P, at least k_min and at most k_max of them.  The rule is per frame
// (topp_select, device_utils.h): nothing depends on the rest of the call.
//   kk_top_p_apply   one thread per frame: the mask and kept_s by topp_select, the weights (times mix) and the bitmask word; thread 0 of
//                    block 0 leaves the words the router backward reads (mode not NULL: a site call).
//   kk_top_p_count   ONE block of 256 threads, launched only when count or khist is asked for: thread t takes the frames t, t + 256, ...
//                    and keeps E counts and E + 1 histogram bins in registers; every bin is then one integer block sum (shuffles within
//                    the wave, the four waves in wave order) and ONE store -- the outputs are overwritten, nothing is cleared, and integer
//                    sums have the same bits on every call.  It reads the frames' bitmask words when the apply launch left them in
//                    `choice` (k_s = their popcount), else it runs topp_select on p itself.
// Every access is guarded by s < S and e < E.
#include "../../include/avmoe.h"
#include "common.h"
#include "device_utils.h"
#include "kernels.h"
#include <hip/hip_runtime.h>
#include <climits>
#include <cstdint>

namespace avmoe {

namespace {

__global__ void __launch_bounds__(256) kk_top_p_apply(const float* p, long S, int E, float P, int k_min, int k_max, int renorm,
                                                      const float* mix, float* w, int32_t* choice, int* mode) {
  __shared__ float s_pr[256][MAX_E + 1];                   // one frame's probabilities per thread (+ 1: no bank conflicts)
  const int t = threadIdx.x;
  if (mode && blockIdx.x == 0 && t == 0) {                 // (behind the router's own words on the stream: kk_router_tail left the dense form)
    mode[MODE_K] = k_max; mode[MODE_RENORM] = renorm; mode[MODE_SELECT] = MODE_SELECT_TOP_P;
    mode[MODE_SELECT_WORDS] = __float_as_int(P); mode[MODE_SELECT_WORDS + 1] = k_min;
  }
  const long s = (long)blockIdx.x * 256 + t;
  if (s >= S) return;                                      // (no barrier in this kernel)
  float* pr = s_pr[t];
  for (int e = 0; e < E; ++e) pr[e] = p[s * E + e];
  float kept;
  const unsigned m = topp_select(pr, E, P, k_min, k_max, &kept);
  if (choice) choice[s] = (int32_t)m;
  if (w)
    for (int e = 0; e < E; ++e) {
      float x = ((m >> e) & 1u) ? (renorm ? pr[e] / kept : pr[e]) : 0.f;
      if (mix) x *= mix[s * E + e];
      w[s * E + e] = x;
    }
}

// block (256 threads) integer sum through LDS scratch of 4 words; result valid in every thread
__device__ __forceinline__ int block_sum256_i(int v, int* scratch4) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) scratch4[threadIdx.x >> 6] = v;
  __syncthreads();
  return scratch4[0] + scratch4[1] + scratch4[2] + scratch4[3];
}

__global__ void __launch_bounds__(256) kk_top_p_count(const float* p, const int32_t* choice, long S, int E, float P, int k_min, int k_max,
                                                      int32_t* count, int32_t* khist) {
  __shared__ int red[4];
  __shared__ float s_pr[256][MAX_E + 1];
  int cnt[MAX_E], kh[MAX_E + 1];
#pragma unroll
  for (int e = 0; e < MAX_E; ++e) cnt[e] = 0;
#pragma unroll
  for (int j = 0; j <= MAX_E; ++j) kh[j] = 0;
  float* pr = s_pr[threadIdx.x];
  for (long s = threadIdx.x; s < S; s += 256) {
    unsigned m;
    if (choice) m = (unsigned)choice[s];                   // (uniform over the block) the words the apply launch wrote
    else {
      for (int e = 0; e < E; ++e) pr[e] = p[s * E + e];
      float kept;
      m = topp_select(pr, E, P, k_min, k_max, &kept);
    }
    const int ks = __popc(m);
#pragma unroll
    for (int e = 0; e < MAX_E; ++e) cnt[e] += (int)((m >> e) & 1u);
#pragma unroll
    for (int j = 0; j <= MAX_E; ++j) kh[j] += (int)(ks == j);
  }
#pragma unroll
  for (int e = 0; e < MAX_E; ++e)
    if (count && e < E) {                                  // (uniform over the block)
      const int c = block_sum256_i(cnt[e], red);
      if (threadIdx.x == 0) count[e] = c;
    }
#pragma unroll
  for (int j = 0; j <= MAX_E; ++j)
    if (khist && j <= E) {                                 // (uniform over the block)
      const int c = block_sum256_i(kh[j], red);
      if (threadIdx.x == 0) khist[j] = c;
    }
}

}  // namespace

int k_top_p_apply(const float* p, long S, int E, float top_p, int k_min, int k_max, int renorm, const float* mix, float* w, int32_t* choice,
                  int* mode, hipStream_t st) {
  hipLaunchKernelGGL(kk_top_p_apply, dim3((unsigned)cdiv(S, 256)), dim3(256), 0, st, p, S, E, top_p, k_min, k_max, renorm ? 1 : 0, mix, w,
                     choice, mode);
  AVMOE_CHECK_LAUNCH("top_p_apply");
  return OK;
}

int k_top_p_count(const float* p, const int32_t* choice, long S, int E, float top_p, int k_min, int k_max, int32_t* count, int32_t* khist,
                  hipStream_t st) {
  hipLaunchKernelGGL(kk_top_p_count, dim3(1), dim3(256), 0, st, p, choice, S, E, top_p, k_min, k_max, count, khist);
  AVMOE_CHECK_LAUNCH("top_p_count");
  return OK;
}

// the ranges both entry points share (`fn`: the entry point's name in the error strings); nothing is launched behind a refusal
int top_p_check(const char* fn, int E, float top_p, int k_min, int k_max) {
  if (E < 2 || E > MAX_E) { set_last_error("%s: E %d not in [2, %d]", fn, E, MAX_E); return ERR_BAD_ARG; }
  if (!(top_p > 0.f && top_p <= 1.f)) { set_last_error("%s: top_p %g not in (0, 1]", fn, (double)top_p); return ERR_BAD_ARG; }      // (NaN fails both comparisons)
  if (k_min < 1 || k_min > E) { set_last_error("%s: k_min %d not in [1, %d]", fn, k_min, E); return ERR_BAD_ARG; }
  if (k_max < 1 || k_max > E) { set_last_error("%s: k_max %d not in [1, %d]", fn, k_max, E); return ERR_BAD_ARG; }
  if (k_min > k_max) { set_last_error("%s: k_min %d above k_max %d", fn, k_min, k_max); return ERR_BAD_ARG; }
  return OK;
}

}  // namespace avmoe

extern "C" int avmoe_router_top_p(const float* p, int64_t S, int32_t E, float top_p, int32_t k_min, int32_t k_max, int32_t renorm,
                                  const float* mix_scale, float* w, int32_t* choice, int32_t* count, int32_t* khist, void* stream) {
  using namespace avmoe;
  if (!p) { set_last_error("avmoe_router_top_p: null pointer"); return ERR_BAD_ARG; }
  AVMOE_TRY(top_p_check("avmoe_router_top_p", (int)E, top_p, (int)k_min, (int)k_max));
  if (S < 1 || S > (int64_t)INT_MAX) { set_last_error("avmoe_router_top_p: S %lld not in [1, 2^31)", (long long)S); return ERR_BAD_ARG; }
  if (w) {
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)w, n = (uintptr_t)S * (uintptr_t)E * sizeof(float);
    if (a < b + n && b < a + n) { set_last_error("avmoe_router_top_p: w overlaps p"); return ERR_BAD_ARG; }
  }
  hipStream_t st = (hipStream_t)stream;
  if (w || choice) AVMOE_TRY(k_top_p_apply(p, (long)S, (int)E, top_p, (int)k_min, (int)k_max, renorm, mix_scale, w, choice, nullptr, st));
  if (count || khist) AVMOE_TRY(k_top_p_count(p, choice, (long)S, (int)E, top_p, (int)k_min, (int)k_max, count, khist, st));
  return OK;
}
