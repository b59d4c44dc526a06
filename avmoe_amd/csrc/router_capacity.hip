// Expert capacity for top-k routing (avmoe_moe_forward_capacity / avmoe_router_capacity, include/avmoe.h; GShard, Lepikhin et al. 2020;
// Switch, Fedus et al. 2021; batch-prioritised routing, V-MoE, Riquelme et al. 2021): every expert serves at most c of the frames whose own
// top-k selection chose it, and the pairs beyond that budget are dropped -- their mixture weight becomes exactly +0.0f.  With
// m[s, e] = 1[e in S_k(s)] the selection of the top-k form (topk_select / topk_select_biased on the call's dense softmax p):
//   policy 0 "order"     expert e keeps the first c selecting frames in frame order:      keep = m && s <= L_e
//   policy 1 "priority"  expert e keeps the c selecting frames with the largest p[s, e],
//                        equal values in frame order:                                      keep = m && ec_member(p[s, e], T_e, L_e, s)
// An expert's outcome is two words as in expert choice (device_utils.h: ec_member), a threshold T_e and a last frame L_e; with
// demand_e = sum_s m[s, e] <= c everything is kept: T_e = -Inf, L_e = S - 1.  Policy 0 does not use T_e (written as -Inf).
//   kk_cap_mask    one thread per frame: the selection word m[s] (bit e = m[s, e]) recomputed from p and the bias with the forward's own
//                  helpers -- not inferred from the weights, which underflow and carry the multiplier.
//   kk_cap_select  one block per expert.  Policy 1: the exact radix select of kk_ec_select (most significant byte first, a 256-bin INTEGER
//                  histogram in the LDS per byte) over the frames whose word has bit e -- the first byte's histogram also totals the
//                  demand, and a demand within the budget ends the block there --, then ONE ordered pass for the last tied frame taken.
//                  Policy 0: one ordered pass, a chunk of blockDim frames at a time in frame order, with a block-wide prefix count of
//                  bit e (ballot and popcount per wave, wave totals through the LDS): the frame that holds the c-th is L_e, the final
//                  count the demand.  Leaves T_e, L_e, demand_e and kept_e = min(demand_e, c).
//   kk_cap_apply   one thread per frame: keep from m, p, T, L; the dropped entries of w are SET to +0.0f, cap_scale = keep ? mix (or 1) : 0,
//                  and the bitmask of the kept pairs.
// LDS integer atomics only: no floating-point atomics, no tickets, no fences -- the same bytes on every call.  Every access is guarded by
// s < S.
#include "../../include/avmoe.h"
#include "common.h"
#include "device_utils.h"
#include "kernels.h"
#include <hip/hip_runtime.h>
#include <climits>
#include <cstdint>

namespace avmoe {

namespace {

constexpr int CAP_NEG_INF = (int)0xff800000u;      // the bits of -Inf: ec_member holds for every number

__global__ void __launch_bounds__(256) kk_cap_mask(const float* p, long S, int E, int k, const float* bias, int32_t* mask) {
  __shared__ float s_b[MAX_E];
  __shared__ float s_pr[256][MAX_E + 1];                   // one frame's probabilities per thread (+ 1: no bank conflicts)
  const int t = threadIdx.x;
  if (bias && t < E) s_b[t] = bias[t];
  __syncthreads();
  const long s = (long)blockIdx.x * 256 + t;
  if (s >= S) return;
  float* pr = s_pr[t];
  for (int e = 0; e < E; ++e) pr[e] = p[s * E + e];
  float kept;
  mask[s] = (int32_t)(bias ? topk_select_biased(pr, s_b, E, k, &kept) : topk_select(pr, E, k, &kept));
}

__global__ void __launch_bounds__(1024) kk_cap_select(const float* p, const int32_t* mask, long S, int E, int c, int policy, int* thr_bits,
                                                      int* last, int32_t* demand, int32_t* kept_count) {
  __shared__ int s_hist[256];
  __shared__ unsigned s_prefix;
  __shared__ int s_need, s_last, s_total;
  __shared__ int s_wc[2][16];
  const int e = blockIdx.x, t = threadIdx.x, nt = blockDim.x, lane = t & 63, wv = t >> 6, nw = nt >> 6;   // (nt: a multiple of 64)
  const float* col = p + e;
  if (t == 0) s_last = -1;
  if (policy == 0) {                               // ---- order: the c-th selecting frame, and the demand
    int base = 0, par = 0;
    for (long s0 = 0; s0 < S; s0 += nt, par ^= 1) {        // (the same trip count in every lane: the ballots see whole waves)
      const long s = s0 + t;
      const bool flag = s < S && ((mask[s] >> e) & 1);
      const unsigned long long b = __ballot(flag);
      if (lane == 0) s_wc[par][wv] = (int)__popcll(b);
      __syncthreads();                             // (one barrier per chunk: the next chunk writes the other half of s_wc)
      int before = base, total = 0;
      for (int w = 0; w < nw; ++w) { const int v = s_wc[par][w]; if (w < wv) before += v; total += v; }
      const int rank = before + (int)__popcll(b & ((1ull << lane) - 1ull)) + 1;
      if (flag && rank == c) s_last = (int)s;      // (one thread of the block at most)
      base += total;
    }
    __syncthreads();
    if (t == 0) {
      const bool over = base > c;
      thr_bits[e] = CAP_NEG_INF;
      last[e] = over ? s_last : (int)(S - 1);
      if (demand) demand[e] = base;
      if (kept_count) kept_count[e] = over ? c : base;
    }
    return;
  }
  // ---- priority: the c-th largest p[s, e] among the selecting frames
  unsigned prefix = 0u, kmask = 0u;                // the key bytes fixed so far
  int need = c;                                    // rank of the wanted key among the keys that match them, from the top, 1-based
  for (int shift = 24; shift >= 0; shift -= 8) {
    for (int i = t; i < 256; i += nt) s_hist[i] = 0;
    __syncthreads();
    for (long s0 = 0; s0 < S; s0 += nt) {
      const long s = s0 + t;
      const bool on = s < S && ((mask[s] >> e) & 1);
      const unsigned key = on ? ec_key(col[s * E]) : 0u;
      const bool hit = on && (key & kmask) == prefix;
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
      if (lane == 63) s_total = inc;               // the keys that matched: in the first pass, the demand
      const int exc = inc - tot;
      if (exc < need && need <= inc) {             // one lane, when the matching keys number at least `need`
        int r = need - exc;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (r > 0 && r <= h[j]) { s_prefix = prefix | ((unsigned)(255 - 4 * lane - j) << shift); s_need = r; r = 0; }
          else if (r > 0) r -= h[j];
        }
      }
    }
    __syncthreads();
    if (shift == 24) {
      const int dem = s_total;                     // (uniform over the block)
      if (t == 0) {
        if (demand) demand[e] = dem;
        if (kept_count) kept_count[e] = dem > c ? c : dem;
      }
      if (dem <= c) {                              // within the budget: everything kept (s_prefix / s_need were not written)
        if (t == 0) { thr_bits[e] = CAP_NEG_INF; last[e] = (int)(S - 1); }
        return;
      }
    }
    prefix = s_prefix; need = s_need; kmask |= 0xffu << shift;
  }
  // prefix is the key of T; `need` of the selecting frames that hold it are taken, in frame order
  int base = 0, par = 0;
  for (long s0 = 0; s0 < S; s0 += nt, par ^= 1) {
    const long s = s0 + t;
    const bool flag = s < S && ((mask[s] >> e) & 1) && ec_key(col[s * E]) == prefix;
    const unsigned long long b = __ballot(flag);
    if (lane == 0) s_wc[par][wv] = (int)__popcll(b);
    __syncthreads();
    int before = base, total = 0;
    for (int w = 0; w < nw; ++w) { const int v = s_wc[par][w]; if (w < wv) before += v; total += v; }
    const int rank = before + (int)__popcll(b & ((1ull << lane) - 1ull)) + 1;
    if (flag && rank == need) s_last = (int)s;
    base += total;
    if (base >= need) break;                       // (uniform over the block)
  }
  __syncthreads();
  if (t == 0) { thr_bits[e] = __float_as_int(ec_unkey(prefix)); last[e] = s_last; }
}

__global__ void __launch_bounds__(256) kk_cap_apply(const float* p, const int32_t* mask, long S, int E, int policy, const int* thr_bits,
                                                    const int* last, const float* mix, float* w, float* cap_scale, int32_t* kept) {
  __shared__ float s_T[MAX_E];
  __shared__ int s_L[MAX_E];
  if ((int)threadIdx.x < E) { s_T[threadIdx.x] = __int_as_float(thr_bits[threadIdx.x]); s_L[threadIdx.x] = last[threadIdx.x]; }
  __syncthreads();
  const long s = (long)blockIdx.x * 256 + threadIdx.x;
  if (s >= S) return;
  const unsigned m = (unsigned)mask[s];            // (mask and kept may be one buffer: read before the word is written)
  unsigned km = 0u;
  for (int e = 0; e < E; ++e) {
    const bool sel = (m >> e) & 1u;
    const bool keep = sel && (policy ? ec_member(p[s * E + e], s_T[e], s_L[e], s) : s <= (long)s_L[e]);
    if (keep) km |= 1u << e;
    if (cap_scale) cap_scale[s * E + e] = keep ? (mix ? mix[s * E + e] : 1.f) : 0.f;
    if (w && sel && !keep) w[s * E + e] = 0.f;     // set, not multiplied
  }
  if (kept) kept[s] = (int32_t)km;
}

}  // namespace

int k_cap_mask(const float* p, long S, int E, int top_k, const float* bias, int32_t* mask, hipStream_t st) {
  hipLaunchKernelGGL(kk_cap_mask, dim3((unsigned)cdiv(S, 256)), dim3(256), 0, st, p, S, E, top_k, bias, mask);
  AVMOE_CHECK_LAUNCH("capacity_mask");
  return OK;
}

int k_cap_select(const float* p, const int32_t* mask, long S, int E, int capacity, int policy, int* thr_bits, int* last, int32_t* demand,
                 int32_t* kept_count, hipStream_t st) {
  const int nt = (int)std::min<long>(1024, round_up(S, 64));
  hipLaunchKernelGGL(kk_cap_select, dim3((unsigned)E), dim3((unsigned)nt), 0, st, p, mask, S, E, capacity, policy, thr_bits, last, demand,
                     kept_count);
  AVMOE_CHECK_LAUNCH("capacity_select");
  return OK;
}

int k_cap_apply(const float* p, const int32_t* mask, long S, int E, int policy, const int* thr_bits, const int* last, const float* mix,
                float* w, float* cap_scale, int32_t* kept, hipStream_t st) {
  hipLaunchKernelGGL(kk_cap_apply, dim3((unsigned)cdiv(S, 256)), dim3(256), 0, st, p, mask, S, E, policy, thr_bits, last, mix, w, cap_scale,
                     kept);
  AVMOE_CHECK_LAUNCH("capacity_apply");
  return OK;
}

}  // namespace avmoe

extern "C" int avmoe_router_capacity(const float* p, int64_t S, int32_t E, int32_t top_k, const float* select_bias, int32_t capacity,
                                     int32_t policy, const float* mix_scale, float* w, float* cap_scale, int32_t* kept, int32_t* demand,
                                     int32_t* kept_count, float* thr, int32_t* last, void* stream) {
  using namespace avmoe;
  if (!p) { set_last_error("avmoe_router_capacity: null pointer"); return ERR_BAD_ARG; }
  if (E < 2 || E > MAX_E) { set_last_error("avmoe_router_capacity: E %d not in [2, %d]", (int)E, MAX_E); return ERR_BAD_ARG; }
  if (S < 1 || S > (int64_t)INT_MAX) { set_last_error("avmoe_router_capacity: S %lld not in [1, 2^31)", (long long)S); return ERR_BAD_ARG; }
  if (top_k < 1 || top_k >= E) { set_last_error("avmoe_router_capacity: top_k %d not in [1, %d)", (int)top_k, (int)E); return ERR_BAD_ARG; }
  if (capacity < 1 || (int64_t)capacity > S) {
    set_last_error("avmoe_router_capacity: capacity %d not in [1, %lld]", (int)capacity, (long long)S); return ERR_BAD_ARG;
  }
  if (policy != 0 && policy != 1) { set_last_error("avmoe_router_capacity: policy %d not in {0, 1}", (int)policy); return ERR_BAD_ARG; }
  if (w) {
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)w, n = (uintptr_t)S * (uintptr_t)E * sizeof(float);
    if (a < b + n && b < a + n) { set_last_error("avmoe_router_capacity: w overlaps p"); return ERR_BAD_ARG; }
  }
  hipStream_t st = (hipStream_t)stream;
  int* tmp = nullptr;                              // the selection words (S) and the two words per expert the caller did not ask for
  const size_t words = (size_t)S + 2 * MAX_E;
  if (hipMallocAsync((void**)&tmp, words * sizeof(int), st) != hipSuccess) {
    (void)hipGetLastError(); set_last_error("avmoe_router_capacity: no memory for the selection words"); return ERR_WORKSPACE;
  }
  int* T = thr ? (int*)thr : tmp + S;
  int* L = last ? (int*)last : tmp + S + MAX_E;
  int status = k_cap_mask(p, (long)S, (int)E, (int)top_k, select_bias, tmp, st);
  if (status == OK) status = k_cap_select(p, tmp, (long)S, (int)E, (int)capacity, (int)policy, T, L, demand, kept_count, st);
  if (status == OK && (w || cap_scale || kept))
    status = k_cap_apply(p, tmp, (long)S, (int)E, (int)policy, T, L, mix_scale, w, cap_scale, kept, st);
  (void)hipFreeAsync(tmp, st);
  return status;
}
