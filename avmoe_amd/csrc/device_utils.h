// Small device helpers shared by the bottleneck-space kernels (wave64 reductions, T <-> f32).
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include "stream_isa.h"      // the vector types (f32x4, u32x4, u32x2, ...) and the streaming kernels' inline-ISA helpers

// launch KERN<__bf16> or KERN<float> by the run-time operand type
#define DISPATCH_T(bf16, KERN, grid, block, shmem, st, ...)                                   \
  do {                                                                                        \
    if (bf16) hipLaunchKernelGGL((KERN<__bf16>), grid, block, shmem, st, __VA_ARGS__);        \
    else hipLaunchKernelGGL((KERN<float>), grid, block, shmem, st, __VA_ARGS__);              \
  } while (0)

namespace avmoe {

// blocks of 256 threads for n elements, at most `cap` (grid-stride kernels)
inline unsigned grid1d(long n, int cap = 4096) { return (unsigned)std::max<long>(1, std::min<long>((n + 255) / 256, cap)); }

// Wave-level LDS fence: what this wave wrote to the LDS is visible to its own lanes' reads behind it (release fence, wave barrier, acquire
// fence -- no s_barrier: the other waves of the block are not involved).
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ float bf2f(unsigned short h) {
  return __builtin_bit_cast(float, ((unsigned int)h) << 16);
}
__device__ __forceinline__ unsigned short f2bf(float x) {
  return __builtin_bit_cast(unsigned short, (__bf16)x);
}

// top-k gating of one frame (avmoe_moe_forward_topk) from its E probabilities p: bit e of the result is set when expert e is among the
// k most probable -- higher probability first, equal probabilities in expert order (kk_router_topk) -- and *kept = the sum of the
// kept probabilities, added in expert order.  The forward and the router backward call it on the same p: the same selection.
__device__ __forceinline__ unsigned topk_select(const float* p, int E, int k, float* kept) {
  unsigned m = 0u;
  float s = 0.f;
  for (int e = 0; e < E; ++e) {
    int rank = 0;                                  // experts that come before e
    for (int f = 0; f < E; ++f) rank += (p[f] > p[e]) || (p[f] == p[e] && f < e);
    if (rank < k) { m |= 1u << e; s += p[e]; }
  }
  *kept = s;
  return m;
}

// The same with a selection bias b (avmoe_moe_forward_bias: aux-loss-free balancing): the experts are ranked on the score
// sc_e = p_e + b_e -- ONE fp32 addition, so the selection repeats bit for bit from p and b -- with the same tie rule on the scores,
// and *kept stays the sum of the kept UNBIASED probabilities, added in expert order: the bias enters the selection only.
__device__ __forceinline__ unsigned topk_select_biased(const float* p, const float* b, int E, int k, float* kept) {
  float sc[16];                                    // (AVMOE_MAX_EXPERTS)
  for (int e = 0; e < E; ++e) sc[e] = __fadd_rn(p[e], b[e]);      // (never contracted into a neighbouring product)
  unsigned m = 0u;
  float s = 0.f;
  for (int e = 0; e < E; ++e) {
    int rank = 0;
    for (int f = 0; f < E; ++f) rank += (sc[f] > sc[e]) || (sc[f] == sc[e] && f < e);
    if (rank < k) { m |= 1u << e; s += p[e]; }
  }
  *kept = s;
  return m;
}

// Expert-choice gating (avmoe_moe_forward_choice, expert_choice.hip): the order-preserving 32-bit key of an fp32 value -- a larger value
// has a larger key, -0 and +0 share one, so that for numbers key order IS the order of `>` / `==` -- and the membership test of frame s in
// an expert's selection from its two words: T = the c-th largest value of the column, L = the last frame taken among the values equal to T.
// The forward and the router backward call ec_member on the same p, T, L: the same mask.
__device__ __forceinline__ unsigned ec_key(float v) {
  unsigned u = __float_as_uint(v);
  if (u == 0x80000000u) u = 0u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ec_unkey(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }
__device__ __forceinline__ bool ec_member(float p, float T, int L, long s) {
  const unsigned kp = ec_key(p), kt = ec_key(T);
  return kp > kt || (kp == kt && s <= (long)L);
}

// Sinkhorn-balanced top-k (avmoe_moe_forward_sinkhorn, router_sinkhorn.hip): the experts are ranked on the score q_e = p_e v_e -- ONE fp32
// multiplication, so the selection repeats bit for bit from p and the E words v -- with the tie rule of topk_select on q, and *kept stays
// the sum of the kept UNSCALED probabilities, added in expert order: v enters the selection only.  The ranks are taken on ec_key(q), for
// numbers the order of `>` / `==` and a total order on every bit pattern: exactly k experts are marked whatever p holds.
__device__ __forceinline__ unsigned topk_select_scaled(const float* p, const float* v, int E, int k, float* kept) {
  unsigned q[16];                                  // (AVMOE_MAX_EXPERTS)
  for (int e = 0; e < E; ++e) q[e] = ec_key(__fmul_rn(p[e], v[e]));   // (never contracted into a neighbouring sum)
  unsigned m = 0u;
  float s = 0.f;
  for (int e = 0; e < E; ++e) {
    int rank = 0;
    for (int f = 0; f < E; ++f) rank += (q[f] > q[e]) || (q[f] == q[e] && f < e);
    if (rank < k) { m |= 1u << e; s += p[e]; }
  }
  *kept = s;
  return m;
}

// Top-p routing (avmoe_moe_forward_top_p, router_top_p.hip): the frame takes the shortest prefix of its ranked experts whose mass reaches P,
// at least k_min and at most k_max of them.  The ranks are those of topk_select, taken on ec_key(p) as in topk_select_scaled (a total order
// on every bit pattern: a permutation of 0 .. E - 1, packed four bits per expert); the running mass c_j = c_(j-1) + p_(j) is ONE fp32
// addition per rank, in rank order, and k* = the first j with c_j >= P (E when none does).  *kept = the sum of the kept p in expert order,
// as topk_select forms it: with k_min = k_max = k the bits of plain top-k.  The forward, the auxiliary losses and the router backward call
// it on the same p, P, k_min, k_max: the same selection.
__device__ __forceinline__ unsigned topp_select(const float* p, int E, float P, int k_min, int k_max, float* kept) {
  unsigned long long ranks = 0ull;                 // nibble e: the rank of expert e
  for (int e = 0; e < E; ++e) {
    const unsigned qe = ec_key(p[e]);
    int rank = 0;
    for (int f = 0; f < E; ++f) { const unsigned qf = ec_key(p[f]); rank += (qf > qe) || (qf == qe && f < e); }
    ranks |= (unsigned long long)rank << (4 * e);
  }
  int ks = E;
  float c = 0.f;
  for (int j = 0; j < E; ++j) {                    // the expert of rank j (exactly one)
    float pj = 0.f;
    for (int e = 0; e < E; ++e) if ((int)((ranks >> (4 * e)) & 15ull) == j) pj = p[e];
    c = __fadd_rn(c, pj);                          // (never contracted, never reassociated)
    if (c >= P) { ks = j + 1; break; }
  }
  ks = min(max(ks, k_min), k_max);
  unsigned m = 0u;
  float s = 0.f;
  for (int e = 0; e < E; ++e)
    if ((int)((ranks >> (4 * e)) & 15ull) < ks) { m |= 1u << e; s += p[e]; }
  *kept = s;
  return m;
}

// element access for the activation / operand type T (float or __bf16)
template <typename T> __device__ __forceinline__ float ldT(const T* p, long i);
template <> __device__ __forceinline__ float ldT<float>(const float* p, long i) { return p[i]; }
template <> __device__ __forceinline__ float ldT<__bf16>(const __bf16* p, long i) {
  return bf2f(((const unsigned short*)p)[i]);
}
template <typename T> __device__ __forceinline__ void stT(T* p, long i, float v);
template <> __device__ __forceinline__ void stT<float>(float* p, long i, float v) { p[i] = v; }
template <> __device__ __forceinline__ void stT<__bf16>(__bf16* p, long i, float v) {
  ((unsigned short*)p)[i] = f2bf(v);
}

// four consecutive elements (index i a multiple of 4, base 16-byte aligned): one 16-byte / 8-byte access
template <typename T> __device__ __forceinline__ float4 ld4T(const T* p, long i);
template <> __device__ __forceinline__ float4 ld4T<float>(const float* p, long i) { return *(const float4*)(p + i); }
template <> __device__ __forceinline__ float4 ld4T<__bf16>(const __bf16* p, long i) {
  const u32x2 u = *(const u32x2*)((const unsigned short*)p + i);
  return make_float4(__builtin_bit_cast(float, u[0] << 16), __builtin_bit_cast(float, u[0] & 0xffff0000u),
                     __builtin_bit_cast(float, u[1] << 16), __builtin_bit_cast(float, u[1] & 0xffff0000u));
}
template <typename T> __device__ __forceinline__ void st4T(T* p, long i, const float4& v);
template <> __device__ __forceinline__ void st4T<float>(float* p, long i, const float4& v) { *(float4*)(p + i) = v; }
template <> __device__ __forceinline__ void st4T<__bf16>(__bf16* p, long i, const float4& v) {
  u32x2 u;
  u[0] = (unsigned)f2bf(v.x) | ((unsigned)f2bf(v.y) << 16); u[1] = (unsigned)f2bf(v.z) | ((unsigned)f2bf(v.w) << 16);
  *(u32x2*)((unsigned short*)p + i) = u;
}

// wave64 all-reduce (every lane gets the result)
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// the same for a double per lane (row statistics whose consumer takes a DIFFERENCE of sums: variance, softmax denominators)
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// block (256 threads) sum through LDS scratch of >= 4 floats; result valid in every thread
__device__ __forceinline__ float block_sum256(float v, float* scratch4) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) scratch4[threadIdx.x >> 6] = v;
  __syncthreads();
  return scratch4[0] + scratch4[1] + scratch4[2] + scratch4[3];
}

}  // namespace avmoe
