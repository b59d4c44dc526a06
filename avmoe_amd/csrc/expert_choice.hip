// Expert-choice gating (avmoe_moe_forward_choice / avmoe_expert_choice, include/avmoe.h; Zhou et al. 2022): each expert e takes the c frames
// on which the router's softmax p[s, e] is highest -- higher probability first, equal probabilities in frame order -- and the mixture
// weights become w[s, e] = m[s, e] p[s, e] (/ kept_s with renorm).  The selection of an expert is described by two words,
//   T_e = the c-th largest value of column e ,  L_e = the largest frame taken among the frames equal to T_e ,
//   m[s, e] = (p[s, e] > T_e) || (p[s, e] == T_e && s <= L_e)            (device_utils.h: ec_member)
// and those are all the first launch produces; the second one and the router backward evaluate the mask per frame from them.
//   kk_ec_select  one block per expert.  An exact radix select on the order-preserving key (ec_key) for the c-th largest: most significant
//                 byte first, a 256-bin INTEGER histogram in the LDS per byte (LDS integer atomics: the counts do not depend on the order
//                 the lanes arrive in), a descending scan of the bins narrows the prefix and the remaining rank.  Then ONE ordered pass over
//                 the frames, a chunk of blockDim frames at a time in frame order, with a block-wide prefix count of key == T (ballot and
//                 popcount per wave, wave totals through the LDS): the frame that holds the `need`-th tie is L_e.
//   kk_ec_apply   one thread per frame: the mask from p, T, L, kept_s added in expert order, the weights (times mix) and the bitmask word.
// No floating-point atomics, no tickets, no fences: the same bytes on every call.  Non-finite values have a place in key order like any
// other, so exactly c frames per expert are marked whatever the column holds; every access is guarded by s < S.
#include "../../include/avmoe.h"
#include "common.h"
#include "device_utils.h"
#include "kernels.h"
#include <hip/hip_runtime.h>
#include <climits>

namespace avmoe {

namespace {

__global__ void __launch_bounds__(1024) kk_ec_select(const float* p, long S, int E, int c, int* thr_bits, int* last) {
  __shared__ int s_hist[256];
  __shared__ unsigned s_prefix;
  __shared__ int s_need, s_last;
  __shared__ int s_wc[2][16];
  const int e = blockIdx.x, t = threadIdx.x, nt = blockDim.x, lane = t & 63, wv = t >> 6, nw = nt >> 6;   // (nt: a multiple of 64)
  const float* col = p + e;
  unsigned prefix = 0u, mask = 0u;         // the key bytes fixed so far
  int need = c;                            // rank of the wanted key among the keys that match them, from the top, 1-based
  for (int shift = 24; shift >= 0; shift -= 8) {
    for (int i = t; i < 256; i += nt) s_hist[i] = 0;
    __syncthreads();
    for (long s0 = 0; s0 < S; s0 += nt) {          // (the same trip count in every lane: the ballots see whole waves)
      const long s = s0 + t;
      const bool on = s < S;
      const unsigned key = on ? ec_key(col[s * E]) : 0u;
      const bool hit = on && (key & mask) == prefix;
      const int bin = (int)((key >> shift) & 255u);
      const unsigned long long hb = __ballot(hit);
      if (hb) {                                    // (uniform over the wave) the lanes that share the first hit's bin add ONE count together
        const int lead = __ffsll((long long)hb) - 1;
        const int bin0 = __shfl(bin, lead, 64);
        const unsigned long long same = __ballot(hit && bin == bin0);
        if (lane == lead) atomicAdd(&s_hist[bin0], (int)__popcll(same));
        else if (hit && bin != bin0) atomicAdd(&s_hist[bin], 1);
      }
    }
    __syncthreads();
    if (t < 64) {                                  // descending scan: lane l owns the bins 255 - 4 l ... 252 - 4 l
      int h[4], tot = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) { h[j] = s_hist[255 - 4 * lane - j]; tot += h[j]; }
      int inc = tot;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const int v = __shfl_up(inc, o, 64);
        if (lane >= o) inc += v;
      }
      const int exc = inc - tot;
      if (exc < need && need <= inc) {             // one lane: the matching keys number at least `need`
        int r = need - exc;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (r > 0 && r <= h[j]) { s_prefix = prefix | ((unsigned)(255 - 4 * lane - j) << shift); s_need = r; r = 0; }
          else if (r > 0) r -= h[j];
        }
      }
    }
    __syncthreads();
    prefix = s_prefix; need = s_need; mask |= 0xffu << shift;
  }
  // prefix is the key of T; `need` of the frames that hold it are taken, in frame order
  if (t == 0) s_last = -1;
  int base = 0, par = 0;
  for (long s0 = 0; s0 < S; s0 += nt, par ^= 1) {
    const long s = s0 + t;
    const bool flag = s < S && ec_key(col[s * E]) == prefix;
    const unsigned long long b = __ballot(flag);
    if (lane == 0) s_wc[par][wv] = (int)__popcll(b);
    __syncthreads();                               // (one barrier per chunk: the next chunk writes the other half of s_wc)
    int before = base, total = 0;
    for (int w = 0; w < nw; ++w) { const int v = s_wc[par][w]; if (w < wv) before += v; total += v; }
    const int rank = before + (int)__popcll(b & ((1ull << lane) - 1ull)) + 1;
    if (flag && rank == need) s_last = (int)s;
    base += total;
    if (base >= need) break;                       // (uniform over the block)
  }
  __syncthreads();
  if (t == 0) {
    if (thr_bits) thr_bits[e] = __float_as_int(ec_unkey(prefix));
    if (last) last[e] = s_last;
  }
}

__global__ void __launch_bounds__(256) kk_ec_apply(const float* p, long S, int E, int renorm, const float* mix, const int* thr_bits,
                                                   const int* last, float* w, int32_t* choice) {
  __shared__ float s_T[MAX_E];
  __shared__ int s_L[MAX_E];
  if ((int)threadIdx.x < E) { s_T[threadIdx.x] = __int_as_float(thr_bits[threadIdx.x]); s_L[threadIdx.x] = last[threadIdx.x]; }
  __syncthreads();
  const long s = (long)blockIdx.x * 256 + threadIdx.x;
  if (s >= S) return;
  unsigned m = 0u;
  float kept = 0.f;
  for (int e = 0; e < E; ++e) {
    const float pe = p[s * E + e];
    if (ec_member(pe, s_T[e], s_L[e], s)) { m |= 1u << e; kept += pe; }
  }
  if (choice) choice[s] = (int32_t)m;
  if (!w) return;
  for (int e = 0; e < E; ++e) {                    // (a frame no expert took: every weight 0, nothing divided)
    const float pe = p[s * E + e];
    float v = ((m >> e) & 1u) ? (renorm ? pe / kept : pe) : 0.f;
    if (mix) v *= mix[s * E + e];
    w[s * E + e] = v;
  }
}

}  // namespace

int k_expert_choice(const float* p, long S, int E, int capacity, int renorm, const float* mix, float* w, int32_t* choice, int* thr_bits,
                    int* last, hipStream_t st) {
  const int nt = (int)std::min<long>(1024, round_up(S, 64));
  hipLaunchKernelGGL(kk_ec_select, dim3((unsigned)E), dim3((unsigned)nt), 0, st, p, S, E, capacity, thr_bits, last);
  AVMOE_CHECK_LAUNCH("expert_choice_select");
  if (!w && !choice) return OK;
  hipLaunchKernelGGL(kk_ec_apply, dim3((unsigned)cdiv(S, 256)), dim3(256), 0, st, p, S, E, renorm ? 1 : 0, mix, (const int*)thr_bits,
                     (const int*)last, w, choice);
  AVMOE_CHECK_LAUNCH("expert_choice_apply");
  return OK;
}

}  // namespace avmoe

extern "C" int avmoe_expert_choice(const float* p, int64_t S, int32_t E, int32_t capacity, int32_t renorm, const float* mix_scale, float* w,
                                   int32_t* choice, float* thr, int32_t* last, void* stream) {
  using namespace avmoe;
  if (!p) { set_last_error("avmoe_expert_choice: null pointer"); return ERR_BAD_ARG; }
  if (S < 1 || S > (int64_t)INT_MAX) { set_last_error("avmoe_expert_choice: S %lld not in [1, 2^31)", (long long)S); return ERR_BAD_ARG; }
  if (E < 1 || E > MAX_E) { set_last_error("avmoe_expert_choice: E %d not in [1, %d]", (int)E, MAX_E); return ERR_BAD_ARG; }
  if (capacity < 1 || (int64_t)capacity > S) {
    set_last_error("avmoe_expert_choice: capacity %d not in [1, %lld]", (int)capacity, (long long)S); return ERR_BAD_ARG;
  }
  hipStream_t st = (hipStream_t)stream;
  int* tl = nullptr;                               // the two words per expert the caller did not ask for, when the second launch needs them
  if ((w || choice) && (!thr || !last)) {
    if (hipMallocAsync((void**)&tl, 2 * MAX_E * sizeof(int), st) != hipSuccess) {
      (void)hipGetLastError(); set_last_error("avmoe_expert_choice: no memory for the selection words"); return ERR_WORKSPACE;
    }
  }
  const int status = k_expert_choice(p, (long)S, (int)E, (int)capacity, renorm, mix_scale, w, choice, thr ? (int*)thr : tl,
                                     last ? (int*)last : (tl ? tl + MAX_E : nullptr), st);
  if (tl) (void)hipFreeAsync(tl, st);
  return status;
}
