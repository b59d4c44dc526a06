// Bottleneck-space kernels, register-resident form generalised over the shapes the reference's models have
// (net_trans_v3.py:571-637, net_avst_v2.py, mgn.py, PVT_AVSModel_v2.py): any expert count, 1 / 2 / 4 conv groups, a per-group
// bottleneck of 16 .. 96 entries (padded to a multiple of 16) and 16 / 32 / 96 latent-token slots (2, 32 and 87 tokens padded).
// tile_fast.hip is the tuned instance for bottleneck 64 in 2 groups / 32 tokens / 2-4 experts (BASELINE config 2) and keeps
// that shape; everything else that fits the table below runs here instead of on the LDS-tiled kernels of tile_kernels.hip.
//
// Same data path as tile_fast.hip: a wavefront owns 16 tokens; lane (r = lane & 15, q = lane >> 4) holds, for token r, the
// entries dd = 16 c + 4 q + x (c = chunk, x = 0..3) of the current expert and group -- Z-space tensors go HBM <-> registers with
// 16-byte accesses, per-token mat-vecs run transposed on the fp32 matrix pipe with the small matrix as A operand from LDS
// (mmT), sums over a token's entries are in-lane + two row swaps, sums over tokens (BatchNorm statistics) live in per-lane
// accumulators for a whole expert pass and are folded once with DPP adds (no float atomics: bit-reproducible).
// Template parameters: NG groups, NCG 16-entry chunks per group, KC 16-slot chunks of latent tokens; the expert count, the true
// number of latent tokens (the padding slots are masked out of the softmax) and every stride are run-time values.
// Arithmetic and names: oracle/algebra_ref.py.
#include "pass.h"
#include "device_utils.h"
#include "prof.h"
#include <algorithm>
#include <mutex>
#include <utility>
#include <vector>

namespace avmoe {

#include "tile_lane.h"

namespace {

struct GenDims { int S, N, C, E, K, Kp, El, KL, KLT, KLp, KPp, NT, per, DZ, XW;
                 int R, NS; long aL; };      // experts resident per round, tile slots: a block has 64 * R * NS threads (see "rounds" below)

// ---- one 16-entry chunk of a row, this lane's 4 entries (chunk pairs: ld_seg / st_seg of tile_lane.h) ------------------------------
template <typename T> __device__ __forceinline__ void ld_one(const T* seg, float4& c0, int q);
template <> __device__ __forceinline__ void ld_one<float>(const float* seg, float4& c0, int q) { c0 = *(const float4*)(seg + 4 * q); }
template <> __device__ __forceinline__ void ld_one<__bf16>(const __bf16* seg, float4& c0, int q) {
  const uint2 u = *(const uint2*)(seg + 4 * q);
  c0 = make_float4(__uint_as_float(u.x << 16), __uint_as_float(u.x & 0xffff0000u), __uint_as_float(u.y << 16), __uint_as_float(u.y & 0xffff0000u));
}
template <typename T> __device__ __forceinline__ void st_one(T* seg, const float4& c0, int q);
template <> __device__ __forceinline__ void st_one<float>(float* seg, const float4& c0, int q) { *(float4*)(seg + 4 * q) = c0; }
template <> __device__ __forceinline__ void st_one<__bf16>(__bf16* seg, const float4& c0, int q) {
  *(uint2*)(seg + 4 * q) = make_uint2((unsigned)f2bf(c0.x) | ((unsigned)f2bf(c0.y) << 16), (unsigned)f2bf(c0.z) | ((unsigned)f2bf(c0.w) << 16));
}
// NC consecutive chunks starting at `seg` (chunk pairs as one 16-byte access per lane, an odd last chunk as 8 / 16 bytes)
template <typename T, int NC> __device__ __forceinline__ void ld_chunks(const T* seg, float4 (&v)[NC], int q) {
#pragma unroll
  for (int c = 0; c + 1 < NC; c += 2) ld_seg<T>(seg + 16 * c, v[c], v[c + 1], q);
  if constexpr (NC & 1) ld_one<T>(seg + 16 * (NC - 1), v[NC - 1], q);
}
template <typename T, int NC> __device__ __forceinline__ void st_chunks(T* seg, const float4 (&v)[NC], int q) {
#pragma unroll
  for (int c = 0; c + 1 < NC; c += 2) st_seg<T>(seg + 16 * c, v[c], v[c + 1], q);
  if constexpr (NC & 1) st_one<T>(seg + 16 * (NC - 1), v[NC - 1], q);
}
template <int NC> __device__ __forceinline__ void zero_chunks(float4 (&v)[NC]) {
#pragma unroll
  for (int c = 0; c < NC; ++c) v[c] = zero4();
}

// column of entry jj (0 .. GD) of group gi, expert e inside a Z-space row [group][expert][GD]
__device__ __forceinline__ int zcolg(int gi, int e, int E, int GD) { return (gi * E + e) * GD; }

// ---- rounds of resident experts -------------------------------------------------------------------------------------------------
// The waves of a block take DIFFERENT experts of the SAME 16-token tiles (wave = tile slot * R + resident index; expert = first
// expert of the round + resident index), so that the experts' segments of a Z-space row [group][expert][GD] are requested
// together (one DRAM page, neighbouring sectors) instead of E sweeps over the block's tokens apart -- tile_fast.hip has the
// measurements.  R experts are resident at a time (their per-expert constants in LDS, R chosen on the host from the LDS they
// need); E > R runs as ceil(E / R) rounds.  NS tile slots (R * NS waves per block).
// waves per block an instance is compiled for: the wide instances (bottleneck >= 128, 87 latent tokens) need more than 256 registers
// per wave and keep their four-wave blocks
// (the narrow instances -- <= 32 bottleneck entries, <= 32 latent slots: under 128 registers -- may run sixteen waves: what a block
// that has its CU to itself, Dims::excl, needs to keep the CU busy)
constexpr int gen_max_waves(int ng, int ncg, int kc) { return (ng * ncg >= 8 || kc == 6) ? 4 : ((ng * ncg <= 2 && kc <= 2) ? 16 : 8); }
struct RoundWave { int er, ts; };
__device__ __forceinline__ RoundWave round_wave(const GenDims& t) { const int w = threadIdx.x >> 6; return RoundWave{w % t.R, w / t.R}; }

// fold per-lane token-slot accumulators over the 16 token slots and the tile slots, write colpart[blk][slot][column] of the round's experts
template <int NG, int NCG>
__device__ __forceinline__ void flush_cols(float4 (&acc)[NG][NCG], float* s_col /* [R * NS waves][NG * NCG * 16] */, float* colpart, int blk, int slot,
                                           int e0, const GenDims& t) {
  constexpr int GD = NCG * 16, DD = NG * GD;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane & 15, q = lane >> 4;
#pragma unroll
  for (int gi = 0; gi < NG; ++gi)
#pragma unroll
    for (int c = 0; c < NCG; ++c)
#pragma unroll
      for (int x = 0; x < 4; ++x) {
        const float v = rsum16(at(acc[gi][c], x));
        if (r == 0) s_col[wave * DD + gi * GD + 16 * c + 4 * q + x] = v;
      }
  __syncthreads();
  for (int i = threadIdx.x; i < t.R * DD; i += blockDim.x) {
    const int er = i / DD, dd = i % DD, e = e0 + er;
    if (e >= t.E) continue;
    float v = 0.f;
    for (int u = 0; u < t.NS; ++u) v += s_col[(u * t.R + er) * DD + dd];
    colpart[((long)blk * 4 + slot) * t.DZ + zcolg(dd / GD, e, t.E, GD) + dd % GD] = v;
  }
  __syncthreads();
}
// sum of per-wave values (already wave-uniform) over the tile slots of resident expert er        s_w: [R * NS]
__device__ __forceinline__ float expert_scalar(float v, float* s_w, int er, const GenDims& t) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  __syncthreads();
  if (lane == 0) s_w[wave] = v;
  __syncthreads();
  float o = 0.f;
  for (int u = 0; u < t.NS; ++u) o += s_w[u * t.R + er];
  return o;
}
// per-expert column constants (index dd = gi * GD + jj) from arrays laid out like a Z-space row
template <int NG, int NCG>
__device__ __forceinline__ void stage_cols(float* dst, const float* src, int e, int E) {
  constexpr int GD = NCG * 16, DD = NG * GD;
  for (int dd = threadIdx.x; dd < DD; dd += blockDim.x) dst[dd] = src ? src[zcolg(dd / GD, e, E, GD) + dd % GD] : 0.f;
}
// a (group, expert) block matrix M[j][l] (GD x GD, row-major in global memory) into LDS transposed for mmT: dst[(gi*GD + l) * ld + j]
template <int NG, int NCG>
__device__ __forceinline__ void stage_blocks_T(float* dst, int ld, const float* src, int e, int E) {
  constexpr int GD = NCG * 16;
  tile_fill<8>(NG * GD * GD, blockDim.x,
              [&](int i) { const int gi = i / (GD * GD), rem = i % (GD * GD), j = rem / GD, l = rem % GD; return src[((long)(gi * E + e) * GD + j) * GD + l]; },
              [&](int i, float v) { const int gi = i / (GD * GD), rem = i % (GD * GD), j = rem / GD, l = rem % GD; dst[(gi * GD + l) * ld + j] = v; });
}

#if GEN_PART == 5
// =====================================================================================================
// MID forward: z' = act(BN1(z)) -> Zp (operand of the second-moment GEMM) + column sums of z'   (net_trans_v3.py:397-400)
// =====================================================================================================
struct GMidFArgs { int relu_of_e[MAX_E]; GenDims t; };

template <typename T, int NG, int NCG>
__global__ void __launch_bounds__(gen_max_waves(NG, NCG, 0) * 64) kg_mid(GMidFArgs a, const void* __restrict__ Z_, const float* __restrict__ bn1, void* __restrict__ Zp_, float* __restrict__ colpart) {
  constexpr int GD = NCG * 16, DD = NG * GD;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const T* Z = (const T*)Z_; T* Zp = (T*)Zp_;
  const GenDims& t = a.t;
  const int E = t.E, DZ = t.DZ;
  const int s = blockIdx.y, lane = threadIdx.x & 63, r = lane & 15, q = lane >> 4;
  const RoundWave rw = round_wave(t);
  float* s_c = smem + rw.er * 2 * DD;            // sc, sh  [R][2][DD]
  float* s_col = smem + t.R * 2 * DD;            // [R * NS][DD]
  const int n_beg = blockIdx.x * t.per, n_end = min(t.N, n_beg + t.per);
  const int blk = blockIdx.y * gridDim.x + blockIdx.x;
  for (int e0 = blockIdx.z * t.R; e0 < E; e0 += t.R * gridDim.z) {      // (small sites: one round per block, grid.z rounds)
    const bool act = e0 + rw.er < E;
    const int e = act ? e0 + rw.er : E - 1;
    __syncthreads();
    for (int k = 0; k < t.R && e0 + k < E; ++k) {
      float* c_ = smem + k * 2 * DD;
      stage_cols<NG, NCG>(c_, bn1 + 2 * DZ, e0 + k, E); stage_cols<NG, NCG>(c_ + DD, bn1 + 3 * DZ, e0 + k, E);
    }
    __syncthreads();
    const bool relu = a.relu_of_e[e];
    float4 cs0[NG][NCG];
#pragma unroll
    for (int gi = 0; gi < NG; ++gi) zero_chunks<NCG>(cs0[gi]);
    for (int n0 = n_beg + 16 * rw.ts; n0 < (act ? n_end : n_beg); n0 += 16 * t.NS) {
      const int oz = opaque0();
      const bool ok = n0 + r < t.N;
      const long row = ((long)s * t.N + n0 + r) * DZ;
#pragma unroll
      for (int gi = 0; gi < NG; ++gi) {
        float4 z[NCG], zp[NCG];
        zero_chunks<NCG>(z);
        if (ok) ld_chunks<T, NCG>(Z + row + zcolg(gi, e, E, GD), z, q);
#pragma unroll
        for (int c = 0; c < NCG; ++c) {
          const float4 sc = ld4(s_c + oz + gi * GD + 16 * c + 4 * q), sh = ld4(s_c + oz + DD + gi * GD + 16 * c + 4 * q);
#pragma unroll
          for (int x = 0; x < 4; ++x) {
            float y = at(z[c], x) * at(sc, x) + at(sh, x);
            if (relu) y = fmaxf(y, 0.f);
            y = ok ? rndT<T>(y) : 0.f;
            at(zp[c], x) = y;
            at(cs0[gi][c], x) += y;
          }
        }
        if (ok) st_chunks<T, NCG>(Zp + row + zcolg(gi, e, E, GD), zp, q);
      }
    }
    flush_cols<NG, NCG>(cs0, s_col, colpart, blk, 0, e0, t);
  }
}

// =====================================================================================================
// MID backward      (BN2-moment terms + BN1/ReLU mask; algebra_ref.py MID backward)
// =====================================================================================================
struct GMidArgs { int relu_of_e[MAX_E]; GenDims t; int moments; };

template <typename T, int NG, int NCG>
__global__ void __launch_bounds__(gen_max_waves(NG, NCG, 0) * 64) kg_mid_bwd(GMidArgs a, const void* __restrict__ Z_, const float* __restrict__ bn1, const float* __restrict__ dsm,
                                                  const float* __restrict__ sdSzz, void* __restrict__ dzp_, float* __restrict__ colpart) {
  constexpr int GD = NCG * 16, DD = NG * GD, LDG = GD + 4;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int PE = NG * GD * LDG + 5 * DD;      // per resident expert: [NG * GD][LDG] transposed blocks | mean, rstd, sc, sh, dmz [5][DD]
  const T* Z = (const T*)Z_; T* dzp = (T*)dzp_;
  const GenDims& t = a.t;
  const int E = t.E, DZ = t.DZ;
  const int s = blockIdx.y, lane = threadIdx.x & 63, r = lane & 15, q = lane >> 4;
  const RoundWave rw = round_wave(t);
  float* s_S = smem + rw.er * PE;
  float* s_bn = s_S + NG * GD * LDG;
  float* s_col = smem + t.R * PE;        // [R * NS][DD]
  const int n_beg = blockIdx.x * t.per, n_end = min(t.N, n_beg + t.per);
  const int blk = blockIdx.y * gridDim.x + blockIdx.x;
  for (int e0 = blockIdx.z * t.R; e0 < E; e0 += t.R * gridDim.z) {      // (small sites: one round per block, grid.z rounds)
    const bool act = e0 + rw.er < E;
    const int e = act ? e0 + rw.er : E - 1;
    __syncthreads();
    for (int k = 0; k < t.R && e0 + k < E; ++k) {
      float* S_ = smem + k * PE;
      float* b_ = S_ + NG * GD * LDG;
      const int ek = e0 + k;
      if (a.moments) stage_blocks_T<NG, NCG>(S_, LDG, sdSzz, ek, E);
      stage_cols<NG, NCG>(b_, bn1, ek, E); stage_cols<NG, NCG>(b_ + DD, bn1 + DZ, ek, E); stage_cols<NG, NCG>(b_ + 2 * DD, bn1 + 2 * DZ, ek, E);
      stage_cols<NG, NCG>(b_ + 3 * DD, bn1 + 3 * DZ, ek, E); stage_cols<NG, NCG>(b_ + 4 * DD, a.moments ? dsm + 2 * DZ : nullptr, ek, E);
    }
    __syncthreads();
    const bool relu = a.relu_of_e[e];
    float4 cs0[NG][NCG], cs1[NG][NCG];
#pragma unroll
    for (int gi = 0; gi < NG; ++gi) { zero_chunks<NCG>(cs0[gi]); zero_chunks<NCG>(cs1[gi]); }
    for (int n0 = n_beg + 16 * rw.ts; n0 < (act ? n_end : n_beg); n0 += 16 * t.NS) {
      const int oz = opaque0();
      const bool ok = n0 + r < t.N;
      const long row = ((long)s * t.N + n0 + r) * DZ;
#pragma unroll
      for (int gi = 0; gi < NG; ++gi) {
        float4 z[NCG], dz[NCG], zp[NCG], dyo[NCG];
        zero_chunks<NCG>(z); zero_chunks<NCG>(dz);
        if (ok) { ld_chunks<T, NCG>(Z + row + zcolg(gi, e, E, GD), z, q); ld_chunks<T, NCG>(dzp + row + zcolg(gi, e, E, GD), dz, q); }
        const float* bn = s_bn + oz + gi * GD;
#pragma unroll
        for (int c = 0; c < NCG; ++c) {
          const float4 sc = ld4(bn + 2 * DD + 16 * c + 4 * q), sh = ld4(bn + 3 * DD + 16 * c + 4 * q);
#pragma unroll
          for (int x = 0; x < 4; ++x) {
            const float y = at(z[c], x) * at(sc, x) + at(sh, x);
            at(zp[c], x) = relu ? fmaxf(y, 0.f) : y;
          }
        }
#pragma unroll
        for (int c = 0; c < NCG; ++c) {
          f32x4 w = {0.f, 0.f, 0.f, 0.f};
          if (a.moments) w = mmT<NCG, sizeof(T) == 2>(s_S + oz + gi * GD * LDG, LDG, 16 * c, zp, r, q);
          const float4 mean = ld4(bn + 16 * c + 4 * q), rstd = ld4(bn + DD + 16 * c + 4 * q), dm = ld4(bn + 4 * DD + 16 * c + 4 * q);
          float4 dy;
#pragma unroll
          for (int x = 0; x < 4; ++x) {
            const float zv = at(z[c], x);
            const float zh = (zv - at(mean, x)) * at(rstd, x);
            const float d = at(dz[c], x) + at(dm, x) + w[x];
            const float v = (!ok || (relu && at(zp[c], x) <= 0.f)) ? 0.f : rndT<T>(d);     // as stored: the BN1 sums see the same numbers
            at(dy, x) = v;
            at(cs0[gi][c], x) += v; at(cs1[gi][c], x) += v * zh;
          }
          dyo[c] = dy;
        }
        if (ok) st_chunks<T, NCG>(dzp + row + zcolg(gi, e, E, GD), dyo, q);
      }
    }
    flush_cols<NG, NCG>(cs0, s_col, colpart, blk, 2, e0, t);
    flush_cols<NG, NCG>(cs1, s_col, colpart, blk, 3, e0, t);
  }
}

// =====================================================================================================
// POST_SMALL forward  (net_trans_v3.py:430-434,485-486)
// =====================================================================================================
struct GPostArgs { P16 gate; int relu_of_e[MAX_E]; GenDims t; int ln_post, use_gate; float ln_eps; };

template <typename T, int NG, int NCG>
__global__ void __launch_bounds__(gen_max_waves(NG, NCG, 0) * 64) kg_post_small(GPostArgs a, const void* __restrict__ Z_, const float* __restrict__ bn1, const float* __restrict__ Gq,
                                                     const float* __restrict__ uvh, const float* __restrict__ probs, void* __restrict__ Apost_, float* __restrict__ rpmup) {
  constexpr int GD = NCG * 16, DD = NG * GD, LDG = GD + 4;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int PE = NG * GD * LDG + 4 * DD;      // per resident expert: [NG * GD][LDG] | us, vh, sc, sh  [4][DD]
  T* Apost = (T*)Apost_; const T* Z = (const T*)Z_;
  const GenDims& t = a.t;
  const int E = t.E, DZ = t.DZ;
  const int s = blockIdx.y, lane = threadIdx.x & 63, r = lane & 15, q = lane >> 4;
  const RoundWave rw = round_wave(t);
  float* s_G = smem + rw.er * PE;
  float* s_c = s_G + NG * GD * LDG;
  const int n_beg = blockIdx.x * t.per, n_end = min(t.N, n_beg + t.per);
  for (int e0 = blockIdx.z * t.R; e0 < E; e0 += t.R * gridDim.z) {      // (small sites: one round per block, grid.z rounds)
    const bool act = e0 + rw.er < E;
    const int e = act ? e0 + rw.er : E - 1;
    __syncthreads();
    for (int k = 0; k < t.R && e0 + k < E; ++k) {
      float* G_ = smem + k * PE;
      float* c_ = G_ + NG * GD * LDG;
      const int ek = e0 + k;
      if (a.ln_post) stage_blocks_T<NG, NCG>(G_, LDG, Gq, ek, E);
      stage_cols<NG, NCG>(c_, uvh, ek, E); stage_cols<NG, NCG>(c_ + DD, uvh + DZ, ek, E);
      stage_cols<NG, NCG>(c_ + 2 * DD, bn1 + 2 * DZ, ek, E); stage_cols<NG, NCG>(c_ + 3 * DD, bn1 + 3 * DZ, ek, E);
    }
    float H1 = 0.f, H2 = 0.f;
    for (int gi = 0; gi < NG; ++gi) { H1 += uvh[2 * DZ + gi * E + e]; H2 += uvh[2 * DZ + NG * E + gi * E + e]; }
    __syncthreads();
    const bool relu = a.relu_of_e[e];
    const float gate = a.use_gate ? a.gate.p[e][0] : 1.f;
    const float qv = probs[(long)s * E + e] * gate;
    for (int n0 = n_beg + 16 * rw.ts; n0 < (act ? n_end : n_beg); n0 += 16 * t.NS) {
      const int oz = opaque0();
      const bool ok = n0 + r < t.N;
      const long tok = (long)s * t.N + n0 + r;
      float4 zp[NG][NCG];
      float so = 0.f, soo = 0.f;
#pragma unroll
      for (int gi = 0; gi < NG; ++gi) {
        float4 zraw[NCG];
        zero_chunks<NCG>(zraw);
        if (ok) ld_chunks<T, NCG>(Z + tok * DZ + zcolg(gi, e, E, GD), zraw, q);
        const float* cc = s_c + oz + gi * GD;
#pragma unroll
        for (int c = 0; c < NCG; ++c) {
          const float4 sc = ld4(cc + 2 * DD + 16 * c + 4 * q), sh = ld4(cc + 3 * DD + 16 * c + 4 * q);
#pragma unroll
          for (int x = 0; x < 4; ++x) {
            const float y = at(zraw[c], x) * at(sc, x) + at(sh, x);
            at(zp[gi][c], x) = relu ? fmaxf(y, 0.f) : y;
          }
        }
        if (a.ln_post) {
#pragma unroll
          for (int c = 0; c < NCG; ++c) {
            const f32x4 w = mmT<NCG, sizeof(T) == 2>(s_G + oz + gi * GD * LDG, LDG, 16 * c, zp[gi], r, q);
            const float4 us = ld4(cc + 16 * c + 4 * q), vh = ld4(cc + DD + 16 * c + 4 * q);
#pragma unroll
            for (int x = 0; x < 4; ++x) {
              const float zv = at(zp[gi][c], x);
              so += zv * at(us, x);
              soo += zv * (w[x] + 2.f * at(vh, x));
            }
          }
        }
      }
      float rp = 1.f, mup = 0.f;
      if (a.ln_post) {
        const float So = qsum4(so) + H1, Soo = qsum4(soo) + H2;
        mup = So / (float)t.C;
        rp = rsqrtf(fmaxf(Soo / (float)t.C - mup * mup, 0.f) + a.ln_eps);
      }
      if (ok) {
        const float sc = qv * rp;
#pragma unroll
        for (int gi = 0; gi < NG; ++gi) {
          float4 v[NCG];
#pragma unroll
          for (int c = 0; c < NCG; ++c) v[c] = make_float4(sc * zp[gi][c].x, sc * zp[gi][c].y, sc * zp[gi][c].z, sc * zp[gi][c].w);
          st_chunks<T, NCG>(Apost + (tok * NG + gi) * t.KPp + e * GD, v, q);
        }
        if (q < NG) {          // the three scalar columns ride in every group's row (each group's output GEMM adds its own channels)
          const long base = (tok * NG + q) * t.KPp + E * GD + 3 * e;
          stT<T>(Apost, base + 0, qv * rp); stT<T>(Apost, base + 1, -qv * rp * mup); stT<T>(Apost, base + 2, qv);
        }
        if (q == 3) { rpmup[(long)e * t.NT + tok] = rp; rpmup[(long)t.NT * E + (long)e * t.NT + tok] = mup; }
      }
    }
  }
}

// =====================================================================================================
// POST_SMALL backward
// =====================================================================================================
struct GPostBArgs { P16 gate; int relu_of_e[MAX_E]; GenDims t; int ln_post, use_gate; const float* dApx; float* dSooT; int dapw; };   // dSooT: Gram-fused mode (gram.hip)

// D16: dApost = T columns (row stride KPp per group) + fp32 side array dApx [token][group][16] (the streaming GEMM's split output)
template <typename T, int NG, int NCG, bool D16>
__global__ void __launch_bounds__(gen_max_waves(NG, NCG, 0) * 64) kg_post_small_bwd(GPostBArgs a, const void* __restrict__ Z_, const float* __restrict__ bn1, const float* __restrict__ Gq,
                                                         const float* __restrict__ uvh, const float* __restrict__ probs, const float* __restrict__ rpmup,
                                                         const void* __restrict__ dAp_, void* __restrict__ dzp_, void* __restrict__ Zp_, void* __restrict__ Zw_,
                                                         float* __restrict__ colpart, float* __restrict__ blkscal) {
  constexpr int GD = NCG * 16, DD = NG * GD, LDG = GD + 4;
  constexpr bool KEEP = NG * NCG <= 8;          // dApost chunks stay in registers between the two sweeps over a token's groups
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int PE = NG * GD * LDG + 4 * DD;      // per resident expert: [NG * GD][LDG] | us, vh, sc, sh  [4][DD]
  T* Zp = (T*)Zp_; T* Zw = (T*)Zw_; const T* Z = (const T*)Z_; T* dzp = (T*)dzp_;
  const float* dAp = (const float*)dAp_; const T* dAp16 = (const T*)dAp_;
  const GenDims& t = a.t;
  const int E = t.E, DZ = t.DZ;
  const int s = blockIdx.y, lane = threadIdx.x & 63, r = lane & 15, q = lane >> 4;
  const RoundWave rw = round_wave(t);
  float* s_G = smem + rw.er * PE;
  float* s_c = s_G + NG * GD * LDG;
  float* s_col = smem + t.R * PE;                 // [R * NS][DD]
  float* s_sc = s_col + t.R * t.NS * DD;          // [R * NS]
  const int n_beg = blockIdx.x * t.per, n_end = min(t.N, n_beg + t.per);
  const int blk = blockIdx.y * gridDim.x + blockIdx.x;
  auto load_d = [&](long tok, int gi, int e, float4 (&d)[NCG]) {
    if constexpr (D16) ld_chunks<T, NCG>(dAp16 + (tok * NG + gi) * a.dapw + e * GD, d, q);      // (split form: rows of E * GD T columns)
    else ld_chunks<float, NCG>(dAp + (tok * NG + gi) * t.KPp + e * GD, d, q);
  };
  for (int e0 = blockIdx.z * t.R; e0 < E; e0 += t.R * gridDim.z) {      // (small sites: one round per block, grid.z rounds)
    const bool act = e0 + rw.er < E;
    const int e = act ? e0 + rw.er : E - 1;
    __syncthreads();
    for (int k = 0; k < t.R && e0 + k < E; ++k) {
      float* G_ = smem + k * PE;
      float* c_ = G_ + NG * GD * LDG;
      const int ek = e0 + k;
      if (a.ln_post) stage_blocks_T<NG, NCG>(G_, LDG, Gq, ek, E);
      stage_cols<NG, NCG>(c_, uvh, ek, E); stage_cols<NG, NCG>(c_ + DD, uvh + DZ, ek, E);
      stage_cols<NG, NCG>(c_ + 2 * DD, bn1 + 2 * DZ, ek, E); stage_cols<NG, NCG>(c_ + 3 * DD, bn1 + 3 * DZ, ek, E);
    }
    __syncthreads();
    const bool relu = a.relu_of_e[e];
    const float gate = a.use_gate ? a.gate.p[e][0] : 1.f;
    const float qv = probs[(long)s * E + e] * gate;
    float sdq = 0.f, sdSo = 0.f, sdSoo = 0.f;
    float4 cs0[NG][NCG], cs1[NG][NCG];
#pragma unroll
    for (int gi = 0; gi < NG; ++gi) { zero_chunks<NCG>(cs0[gi]); zero_chunks<NCG>(cs1[gi]); }
    int qsel = 0;      // the lane (of the four that hold a token) that takes this tile's scalar terms: four times as many partial sums
    for (int n0 = n_beg + 16 * rw.ts; n0 < (act ? n_end : n_beg); n0 += 16 * t.NS, qsel = (qsel + 1) & 3) {
      const int oz = opaque0();
      const bool ok = n0 + r < t.N;
      const long tok = (long)s * t.N + n0 + r;
      float4 zp[NG][NCG], dk[KEEP ? NG : 1][NCG];
      float da1 = 0.f, da2 = 0.f, da3 = 0.f, rp = 1.f, mup = 0.f, zz = 0.f;
#pragma unroll
      for (int gi = 0; gi < NG; ++gi) {
        float4 zraw[NCG], d[NCG];
        zero_chunks<NCG>(zraw); zero_chunks<NCG>(d);
        if (ok) { ld_chunks<T, NCG>(Z + tok * DZ + zcolg(gi, e, E, GD), zraw, q); load_d(tok, gi, e, d); }
        const float* cc = s_c + oz + gi * GD;
#pragma unroll
        for (int c = 0; c < NCG; ++c) {
          const float4 sc = ld4(cc + 2 * DD + 16 * c + 4 * q), sh = ld4(cc + 3 * DD + 16 * c + 4 * q);
#pragma unroll
          for (int x = 0; x < 4; ++x) {
            const float y = at(zraw[c], x) * at(sc, x) + at(sh, x);
            const float zv = relu ? fmaxf(y, 0.f) : y;
            at(zp[gi][c], x) = zv;
            zz += at(d[c], x) * zv;
          }
          if constexpr (KEEP) dk[gi][c] = d[c];
        }
        if (ok) {
          const float* p = D16 ? a.dApx + (tok * NG + gi) * t.XW + 3 * e : dAp + (tok * NG + gi) * t.KPp + E * GD + 3 * e;
          da1 += p[0]; da2 += p[1]; da3 += p[2];
        }
      }
      if (ok) { rp = rpmup[(long)e * t.NT + tok]; mup = rpmup[(long)t.NT * E + (long)e * t.NT + tok]; }
      zz = qsum4(zz);
      float dSo = 0.f, dSoo = 0.f;
      if (ok) {
        const float dq = rp * zz + rp * da1 - rp * mup * da2 + da3;
        if (a.ln_post) {
          const float drp = qv * zz + qv * da1 - qv * mup * da2;
          float dmup = -qv * rp * da2;
          const float dvarp = drp * (-0.5f) * rp * rp * rp;
          dSoo = dvarp / (float)t.C;
          dmup -= 2.f * mup * dvarp;
          dSo = dmup / (float)t.C;
        }
        if (q == qsel) { sdq += dq; sdSo += dSo; sdSoo += dSoo; }
      }
      const float k1 = qv * rp;
#pragma unroll
      for (int gi = 0; gi < NG; ++gi) {
        float4 d[NCG], dzo[NCG];
        if constexpr (KEEP) {
#pragma unroll
          for (int c = 0; c < NCG; ++c) d[c] = dk[gi][c];
        } else {
          zero_chunks<NCG>(d);
          if (ok) load_d(tok, gi, e, d);
        }
        const float* cc = s_c + oz + gi * GD;
#pragma unroll
        for (int c = 0; c < NCG; ++c) {
          f32x4 w = {0.f, 0.f, 0.f, 0.f};
          if (a.ln_post) w = mmT<NCG, sizeof(T) == 2>(s_G + oz + gi * GD * LDG, LDG, 16 * c, zp[gi], r, q);
          const float4 us = ld4(cc + 16 * c + 4 * q), vh = ld4(cc + DD + 16 * c + 4 * q);
          float4 o;
#pragma unroll
          for (int x = 0; x < 4; ++x) {
            const float zv = at(zp[gi][c], x);
            float dzv = k1 * at(d[c], x);
            if (a.ln_post) {
              dzv += dSo * at(us, x) + dSoo * (2.f * w[x] + 2.f * at(vh, x));
              at(cs0[gi][c], x) += dSo * zv; at(cs1[gi][c], x) += dSoo * zv;
            }
            at(o, x) = dzv;
          }
          dzo[c] = o;
        }
        if (ok) {
          const long seg = tok * DZ + zcolg(gi, e, E, GD);
          st_chunks<T, NCG>(dzp + seg, dzo, q);
          if (a.dSooT) {                 // the streaming Gram kernel forms z' from z itself and takes dSoo per (expert, token)
            if (gi == 0 && q == 0) a.dSooT[(long)e * t.NT + tok] = dSoo;
          } else {
            float4 zw[NCG];
#pragma unroll
            for (int c = 0; c < NCG; ++c) zw[c] = make_float4(dSoo * zp[gi][c].x, dSoo * zp[gi][c].y, dSoo * zp[gi][c].z, dSoo * zp[gi][c].w);
            st_chunks<T, NCG>(Zp + seg, zp[gi], q);
            st_chunks<T, NCG>(Zw + seg, zw, q);
          }
        }
      }
    }
    flush_cols<NG, NCG>(cs0, s_col, colpart, blk, 0, e0, t);
    flush_cols<NG, NCG>(cs1, s_col, colpart, blk, 1, e0, t);
    const float v0 = expert_scalar(wave_sum(sdq), s_sc, rw.er, t), v1 = expert_scalar(wave_sum(sdSo), s_sc, rw.er, t), v2 = expert_scalar(wave_sum(sdSoo), s_sc, rw.er, t);
    if (act && rw.ts == 0 && lane == 0) { float* o = blkscal + ((long)blk * E + e) * 4; o[0] = v0; o[1] = v1; o[2] = v2; }
  }
}

#endif   // GEN_PART == 5
// =====================================================================================================
// PRE_SMALL forward   (net_trans_v3.py:385-395)
// =====================================================================================================
struct GPreArgs { P16 glat; int lat_of_e[MAX_E]; int nxn_of_e[MAX_E]; long sxr_off[MAX_E]; GenDims t; int ln_before; float ln_eps;
                  const float* ZR; const float* sxr; };

// latent-token matrices of (frame s, latent slot l) into LDS: TT transposed [Kp][LDK] (zero beyond the K real tokens), and the
// expert's TW slice either transposed [DD][LDK] (WT: W[tok][dd] = sum_k a[k] TW[k][dd]) or as stored [Kp][LDD] (W[tok][k] = sum_dd ..)
template <int NG, int NCG, int KC, bool WT>
__device__ __forceinline__ void stage_latent(float* s_TT, float* s_TW, float* s_tb, const float* TT, const float* TW, const float* Tsum,
                                             const GenDims& t, int s, int l, int e) {
  constexpr int GD = NCG * 16, DD = NG * GD, Kp = KC * 16, LDK = Kp + 4, LDD = DD + 4;
  const float* tt = TT + ((long)s * t.El + l) * t.K * t.K;
  const int K = t.K;
  tile_fill<8>(Kp * Kp, blockDim.x,
              [&](int i) { const int k1 = i / Kp, k2 = i % Kp; return tt[min(k1, K - 1) * K + min(k2, K - 1)]; },
              [&](int i, float v) { const int k1 = i / Kp, k2 = i % Kp; s_TT[k2 * LDK + k1] = (k1 < K && k2 < K) ? v : 0.f; });
  tile_fill<8>(Kp * DD, blockDim.x,
              [&](int i) { const int k = i / DD, dd = i % DD; return TW[((long)s * t.KLT + (long)l * t.Kp + min(k, K - 1)) * t.DZ + zcolg(dd / GD, e, t.E, GD) + dd % GD]; },
              [&](int i, float v0) { const int k = i / DD, dd = i % DD; const float v = k < K ? v0 : 0.f; if constexpr (WT) s_TW[dd * LDK + k] = v; else s_TW[k * LDD + dd] = v; });
  for (int k = threadIdx.x; k < Kp; k += blockDim.x) s_tb[k] = k < t.K ? Tsum[(long)s * t.KLT + (long)l * t.Kp + k] / (float)t.C : 0.f;
}

#if GEN_PART == 1 || GEN_PART == 2
template <typename T, int NG, int NCG, int KC, bool XR>
__global__ void __launch_bounds__(gen_max_waves(NG, NCG, KC) * 64) kg_pre_small(GPreArgs a, void* __restrict__ Z_, const float* __restrict__ L2, const float* __restrict__ sxs,
                                                    const float* __restrict__ TT, const float* __restrict__ TW, const float* __restrict__ Tsum,
                                                    const float* __restrict__ wsum, const float* __restrict__ dconst, void* __restrict__ aout_,
                                                    float* __restrict__ rmu, float* __restrict__ colpart) {
  constexpr int GD = NCG * 16, DD = NG * GD, Kp = KC * 16, LDK = Kp + 4;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int PE = Kp * LDK + DD * LDK + Kp + 2 * DD;      // per resident expert: TT^T [Kp][LDK] | TW^T [DD][LDK] | tb [Kp] | wsum, dconst [2][DD]
  T* aout = (T*)aout_; T* Z = (T*)Z_;
  const GenDims& t = a.t;
  const int E = t.E, DZ = t.DZ;
  const int s = blockIdx.y, lane = threadIdx.x & 63, r = lane & 15, q = lane >> 4;
  const RoundWave rw = round_wave(t);
  float* s_TT = smem + rw.er * PE;
  float* s_TWt = s_TT + Kp * LDK;
  float* s_tb = s_TWt + DD * LDK;
  float* s_c = s_tb + Kp;
  float* s_col = smem + t.R * PE;        // [R * NS][DD]
  const int n_beg = blockIdx.x * t.per, n_end = min(t.N, n_beg + t.per);
  const int blk = blockIdx.y * gridDim.x + blockIdx.x;
  for (int e0 = blockIdx.z * t.R; e0 < E; e0 += t.R * gridDim.z) {      // (small sites: one round per block, grid.z rounds)
    const bool act = e0 + rw.er < E;
    const int e = act ? e0 + rw.er : E - 1;
    const int l = a.lat_of_e[e];
    const bool nxn = XR && a.nxn_of_e[e] != 0;
    const float gv = (nxn || l >= 0) ? a.glat.p[e][0] : 0.f;
    __syncthreads();
    for (int k = 0; k < t.R && e0 + k < E; ++k) {
      float* TT_ = smem + k * PE;
      float* TWt_ = TT_ + Kp * LDK;
      float* tb_ = TWt_ + DD * LDK;
      const int ek = e0 + k, lk = a.lat_of_e[ek];
      if (lk >= 0) stage_latent<NG, NCG, KC, true>(TT_, TWt_, tb_, TT, TW, Tsum, t, s, lk, ek);
      stage_cols<NG, NCG>(tb_ + Kp, wsum, ek, E); stage_cols<NG, NCG>(tb_ + Kp + DD, dconst, ek, E);
    }
    __syncthreads();
    float4 cs0[NG][NCG], cs1[NG][NCG];
#pragma unroll
    for (int gi = 0; gi < NG; ++gi) { zero_chunks<NCG>(cs0[gi]); zero_chunks<NCG>(cs1[gi]); }
    for (int n0 = n_beg + 16 * rw.ts; n0 < (act ? n_end : n_beg); n0 += 16 * t.NS) {
      const int oz = opaque0();
      const bool ok = n0 + r < t.N;
      const long tok = (long)s * t.N + n0 + r;
      float Sx = ok ? sxs[tok] : 0.f, Sxx = ok ? sxs[t.NT + tok] : 1.f;
      float4 av[KC];
      zero_chunks<KC>(av);
      if (l >= 0) {
        const long lo = tok * t.KL + (long)l * t.Kp + 4 * q;
        float4 lg[KC];
        float mx = -INFINITY;
#pragma unroll
        for (int j = 0; j < KC; ++j) {
          lg[j] = ok ? ld4(L2 + lo + 16 * j) : zero4();
#pragma unroll
          for (int x = 0; x < 4; ++x)
            if (16 * j + 4 * q + x < t.K) mx = fmaxf(mx, at(lg[j], x));
        }
        mx = qmax4(mx);
        float sum = 0.f;
        float4 ex[KC];
#pragma unroll
        for (int j = 0; j < KC; ++j)
#pragma unroll
          for (int x = 0; x < 4; ++x) {
            const float v = (16 * j + 4 * q + x < t.K) ? __expf(at(lg[j], x) - mx) : 0.f;
            at(ex[j], x) = v; sum += v;
          }
        sum = qsum4(sum);
        const float inv = ok ? 1.f / sum : 0.f;
        float u1 = 0.f, u2 = 0.f;
#pragma unroll
        for (int j = 0; j < KC; ++j) {
          const float4 tb = ld4(s_tb + oz + 16 * j + 4 * q);
#pragma unroll
          for (int x = 0; x < 4; ++x) {
            const float v = rndT<T>(at(ex[j], x) * inv);
            at(av[j], x) = v;
            u1 += v * at(tb, x);
            if (16 * j + 4 * q + x < t.K) u2 += v * at(lg[j], x);
          }
        }
        if (ok) st_chunks<T, KC>(aout + (long)l * t.aL + tok * t.Kp, av, q);
        u1 = qsum4(u1); u2 = qsum4(u2);
        float u3 = 0.f;
#pragma unroll
        for (int ct = 0; ct < KC; ++ct) {
          const f32x4 w = mmT<KC, sizeof(T) == 2>(s_TT + oz, LDK, 16 * ct, av, r, q);
#pragma unroll
          for (int x = 0; x < 4; ++x) u3 += w[x] * at(av[ct], x);
        }
        u3 = qsum4(u3);
        Sx += gv * (float)t.C * u1;
        Sxx += 2.f * gv * u2 + gv * gv * u3;
      }
      if (nxn && ok) {             // x' = x + g xr : sums of x' from the sums of x, xr and x . xr   (mgn.py:132-139)
        const float* sxr = a.sxr + a.sxr_off[e];
        Sx += gv * sxr[tok];
        Sxx += 2.f * gv * sxr[2L * t.NT + tok] + gv * gv * sxr[(long)t.NT + tok];
      }
      float mu = 0.f, rr = 1.f;
      if (a.ln_before) {
        mu = Sx / (float)t.C;
        rr = rsqrtf(fmaxf(Sxx / (float)t.C - mu * mu, 0.f) + a.ln_eps);
      }
#pragma unroll
      for (int gi = 0; gi < NG; ++gi) {
        float4 z[NCG], zo[NCG];
        zero_chunks<NCG>(z);
        const long seg = tok * DZ + zcolg(gi, e, E, GD);
        if (ok) ld_chunks<T, NCG>(Z + seg, z, q);
#pragma unroll
        for (int c = 0; c < NCG; ++c) {
          f32x4 p = {0.f, 0.f, 0.f, 0.f};
          if (l >= 0) p = mmT<KC, sizeof(T) == 2>(s_TWt + oz + gi * GD * LDK, LDK, 16 * c, av, r, q);
          if (nxn && ok) {           // xr through Wt (fp32 rows in the Z layout)
            const float4 zr4 = ld4(a.ZR + seg + 16 * c + 4 * q);
            p = f32x4{zr4.x, zr4.y, zr4.z, zr4.w};
          }
          const float4 ws = ld4(s_c + oz + gi * GD + 16 * c + 4 * q), dc = ld4(s_c + oz + DD + gi * GD + 16 * c + 4 * q);
          float4 o;
#pragma unroll
          for (int x = 0; x < 4; ++x) {
            const float zr = at(z[c], x) + gv * p[x];
            const float zv = rndT<T>(a.ln_before ? rr * (zr - mu * at(ws, x)) + at(dc, x) : zr);   // as stored: BN1 statistics of the stored z
            at(o, x) = zv;
            if (ok) { at(cs0[gi][c], x) += zv; at(cs1[gi][c], x) += zv * zv; }
          }
          zo[c] = o;
        }
        if (ok) st_chunks<T, NCG>(Z + seg, zo, q);
      }
      if (ok && q == 0) { rmu[(long)e * t.NT + tok] = rr; rmu[(long)t.NT * E + (long)e * t.NT + tok] = mu; }
    }
    flush_cols<NG, NCG>(cs0, s_col, colpart, blk, 0, e0, t);
    flush_cols<NG, NCG>(cs1, s_col, colpart, blk, 1, e0, t);
  }
}

#endif   // GEN_PART 1, 2
// =====================================================================================================
// PRE_SMALL backward
// =====================================================================================================
struct GPreBArgs { P16 glat; int lat_of_e[MAX_E]; int nxn_of_e[MAX_E]; int first_of_slot[MAX_E]; long sxr_off[MAX_E]; GenDims t;
                   int ln_before, use_bn, bn_train; const float* ZR; const float* sxr; void* dZR; float* dsr; };

#if GEN_PART == 3 || GEN_PART == 4
// PRE_SMALL backward is two kernels (tile_fast.hip has the measurements): kg_pre_small_bwd -- BN1 input gradient, folded-LayerNorm
// sums and dzraw of every expert, small per-expert constants, so all experts of a round are resident -- and kg_pre_lat_bwd -- the
// hop-2 block of the cross-modal experts (softmax backward over the latent tokens, the mat-vecs against TW / TT) from dzraw as
// stored and the expert's own LayerNorm sums (dslat), with the latent-token matrices in LDS (up to 140 KB per expert).
template <typename T, int NG, int NCG, bool XR>
__global__ void __launch_bounds__(gen_max_waves(NG, NCG, 0) * 64) kg_pre_small_bwd(GPreBArgs a, const void* __restrict__ Z_, const float* __restrict__ wsum,
                                                        const float* __restrict__ dconst, const float* __restrict__ rmu,
                                                        const float* __restrict__ bn1, const float* __restrict__ dsm, const void* __restrict__ dy_in_,
                                                        void* __restrict__ dZx_, void* __restrict__ dL2x_, float* __restrict__ dslat,
                                                        float* __restrict__ dsxs, float* __restrict__ rs2x, float* __restrict__ colpart,
                                                        float* __restrict__ blkscal) {
  constexpr int GD = NCG * 16, DD = NG * GD;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int PE = 7 * DD;      // per resident expert: mean, rstd, sc, mdy, mdyz, wsum, dconst [7][DD]
  const T* Z = (const T*)Z_; const T* dy_in = (const T*)dy_in_;
  T* dZx = (T*)dZx_; T* dL2x = (T*)dL2x_;
  const GenDims& t = a.t;
  const int E = t.E, DZ = t.DZ, NWV = t.R * t.NS;
  const int s = blockIdx.y, wave = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane & 15, q = lane >> 4;
  const RoundWave rw = round_wave(t);
  float* s_bn = smem + rw.er * PE;
  float* s_col = smem + t.R * PE;        // [R * NS][DD]
  float* s_sc = s_col + NWV * DD;        // [R * NS]
  float* s_ln = s_sc + NWV;              // [2][R * NS][16][2]: (dSx, dSxx) of each wave's expert for the step's tokens, two steps deep
  const int n_beg = blockIdx.x * t.per, n_end = min(t.N, n_beg + t.per);
  const int blk = blockIdx.y * gridDim.x + blockIdx.x;
  for (int e0 = 0; e0 < E; e0 += t.R) {
    const bool act = e0 + rw.er < E;
    const int e = act ? e0 + rw.er : E - 1;
    const int l = act ? a.lat_of_e[e] : -1;
    const bool nxn = XR && act && a.nxn_of_e[e] != 0;
    const float gv = nxn ? a.glat.p[e][0] : 0.f;
    // the lowest resident expert of this expert's xr slot adds up the slot's statistics gradients of the round (below)
    bool slot_lead = nxn;
    for (int k = 0; k < rw.er; ++k) if (XR && a.nxn_of_e[e0 + k] && a.sxr_off[e0 + k] == a.sxr_off[e]) slot_lead = false;
    __syncthreads();
    for (int k = 0; k < t.R && e0 + k < E; ++k) {
      float* bn_ = smem + k * PE;
      const int ek = e0 + k;
      stage_cols<NG, NCG>(bn_, bn1, ek, E); stage_cols<NG, NCG>(bn_ + DD, bn1 + DZ, ek, E); stage_cols<NG, NCG>(bn_ + 2 * DD, bn1 + 2 * DZ, ek, E);
      stage_cols<NG, NCG>(bn_ + 3 * DD, a.bn_train ? dsm + 3 * DZ : nullptr, ek, E); stage_cols<NG, NCG>(bn_ + 4 * DD, a.bn_train ? dsm + 4 * DZ : nullptr, ek, E);
      stage_cols<NG, NCG>(bn_ + 5 * DD, wsum, ek, E); stage_cols<NG, NCG>(bn_ + 6 * DD, dconst, ek, E);
    }
    __syncthreads();
    float sdg = 0.f;
    float4 cs0[NG][NCG], cs1[NG][NCG];
#pragma unroll
    for (int gi = 0; gi < NG; ++gi) { zero_chunks<NCG>(cs0[gi]); zero_chunks<NCG>(cs1[gi]); }
    int par = 0;
    int qsel = 0;      // the lane (of the four that hold a token) that takes this tile's scalar terms: four times as many partial sums
    for (int nb = n_beg; nb < n_end; nb += 16 * t.NS, par ^= 1, qsel = (qsel + 1) & 3) {      // (uniform trip count: one barrier per step)
      const int n0 = nb + 16 * rw.ts;
      const int oz = opaque0();
      const bool ok = act && n0 < n_end && n0 + r < t.N;
      const long tok = (long)s * t.N + n0 + r;
      const float rr = (a.ln_before && ok) ? rmu[(long)e * t.NT + tok] : 1.f;
      const float mu = (a.ln_before && ok) ? rmu[(long)t.NT * E + (long)e * t.NT + tok] : 0.f;
      const float irr = 1.f / rr;
      float s_dr = 0.f, s_dmu = 0.f, szr = 0.f;
      // ---- per group: BN1 input gradient, folded-LayerNorm sums, dzraw ----
#pragma unroll
      for (int gi = 0; gi < NG; ++gi) {
        float4 zrow[NCG], dyrow[NCG], dzr[NCG];
        zero_chunks<NCG>(zrow); zero_chunks<NCG>(dyrow);
        const long seg = tok * DZ + zcolg(gi, e, E, GD);
        if (ok) { ld_chunks<T, NCG>(Z + seg, zrow, q); ld_chunks<T, NCG>(dy_in + seg, dyrow, q); }
        const float* bn = s_bn + oz + gi * GD;
#pragma unroll
        for (int c = 0; c < NCG; ++c) {
          const float4 mean = ld4(bn + 16 * c + 4 * q), rstd = ld4(bn + DD + 16 * c + 4 * q), sc = ld4(bn + 2 * DD + 16 * c + 4 * q);
          const float4 mdy = ld4(bn + 3 * DD + 16 * c + 4 * q), mdyz = ld4(bn + 4 * DD + 16 * c + 4 * q);
          const float4 ws = ld4(bn + 5 * DD + 16 * c + 4 * q), dc = ld4(bn + 6 * DD + 16 * c + 4 * q);
#pragma unroll
          for (int x = 0; x < 4; ++x) {
            float v = 0.f;
            if (ok) {
              const float zv = at(zrow[c], x);
              float dz = at(dyrow[c], x);
              if (a.use_bn) {
                if (a.bn_train) dz = at(sc, x) * (dz - at(mdy, x) - (zv - at(mean, x)) * at(rstd, x) * at(mdyz, x));
                else dz = at(sc, x) * dz;
              }
              if (a.ln_before) {
                const float zc = (zv - at(dc, x)) * irr;
                at(cs0[gi][c], x) += dz; at(cs1[gi][c], x) += -rr * mu * dz;
                s_dr += dz * zc; s_dmu += dz * at(ws, x);
                v = rr * dz;
              } else v = dz;
            }
            at(dzr[c], x) = v;
          }
        }
        if (ok) st_chunks<T, NCG>(dZx + seg, dzr, q);
        if (nxn && ok) {             // x' = x + g xr : d(xr Wt^T) = g dzraw, and dzraw . (xr Wt^T) for the gate
          float4 gz[NCG];
#pragma unroll
          for (int c = 0; c < NCG; ++c) {
            const float4 zr4 = ld4(a.ZR + seg + 16 * c + 4 * q);
#pragma unroll
            for (int x = 0; x < 4; ++x) { szr += at(dzr[c], x) * at(zr4, x); at(gz[c], x) = gv * at(dzr[c], x); }
          }
          st_chunks<T, NCG>((T*)a.dZR + seg, gz, q);
        }
      }
      if (nxn) szr = qsum4(szr);
      float dSx = 0.f, dSxx = 0.f;
      if (a.ln_before) {
        const float sdr = qsum4(s_dr), sdm = qsum4(s_dmu);
        float dmu = -rr * sdm;
        const float dvar = sdr * (-0.5f) * rr * rr * rr;
        dSxx = dvar / (float)t.C;
        dmu -= 2.f * mu * dvar;
        dSx = dmu / (float)t.C;
      }
      if (!ok) { dSx = 0.f; dSxx = 0.f; }
      float* ln = s_ln + ((par * NWV + wave) * 16 + r) * 2;
      if (q == 0) { ln[0] = dSx; ln[1] = dSxx; }      // for the sums over the round's experts (behind the barrier below)
      if (ok && q == 0 && l >= 0) { dslat[(2L * l) * t.NT + tok] = dSx; dslat[(2L * l + 1) * t.NT + tok] = dSxx; }      // this expert's own sums: kg_pre_lat_bwd
      if (nxn && ok && q == qsel) {   // the gate's share of the statistics gradients of this expert's xr slot
        const float* sxr = a.sxr + a.sxr_off[e];
        sdg += dSx * sxr[tok] + dSxx * (2.f * sxr[2L * t.NT + tok] + 2.f * gv * sxr[(long)t.NT + tok]) + szr;
      }
      __syncthreads();             // every resident expert's sums of this step are in s_ln[par]
      const float* lnr = s_ln + ((par * NWV + rw.ts * t.R) * 16 + r) * 2;      // resident expert k of this tile slot: lnr[k * 32 + 0 / 1]
      if (XR && slot_lead && ok && q == 0) {
        // statistics gradients to (sum xr, sum xr^2, x . xr) of the xr slot: the resident experts that share it, in expert order,
        // on top of what earlier rounds left
        float v0 = 0.f, v1 = 0.f, v2 = 0.f;
        for (int k = 0; k < t.R && e0 + k < E; ++k)
          if (a.nxn_of_e[e0 + k] && a.sxr_off[e0 + k] == a.sxr_off[e]) {
            const float g = a.glat.p[e0 + k][0], dx = lnr[k * 32], dxx = lnr[k * 32 + 1];
            v0 += g * dx; v1 += 2.f * g * g * dxx; v2 += 2.f * g * dxx;
          }
        float* dsr = a.dsr + a.sxr_off[e];
        if (a.first_of_slot[e]) { dsr[tok] = v0; dsr[(long)t.NT + tok] = v1; dsr[2L * t.NT + tok] = v2; }
        else { dsr[tok] += v0; dsr[(long)t.NT + tok] += v1; dsr[2L * t.NT + tok] += v2; }
      }
      if (rw.er == 0 && ok && q == 0) {      // (resident expert 0 of a round is always a real expert: ok implies act)
        float accx = 0.f, accxx = 0.f;
        for (int k = 0; k < t.R && e0 + k < E; ++k) { accx += lnr[k * 32]; accxx += lnr[k * 32 + 1]; }
        if (e0 != 0) { accx += dsxs[tok]; accxx += dsxs[t.NT + tok]; }
        if (e0 + t.R < E) { dsxs[tok] = accx; dsxs[t.NT + tok] = accxx; }
        else {
          stT<T>(dL2x, tok * t.KLp + t.KL, accx);
          stT<T>(dL2x, tok * t.KLp + t.KL + 1, 1.f);
          rs2x[tok] = 2.f * accxx;
        }
      }
    }
    flush_cols<NG, NCG>(cs0, s_col, colpart, blk, 0, e0, t);
    flush_cols<NG, NCG>(cs1, s_col, colpart, blk, 1, e0, t);
    const float vg = expert_scalar(wave_sum(sdg), s_sc, rw.er, t);
    if (act && rw.ts == 0 && lane == 0) blkscal[((long)blk * E + e) * 4 + 3] = vg;      // (a cross-modal expert's slot is rewritten by kg_pre_lat_bwd)
  }
}

// The hop-2 block.  Rounds over the CROSS-MODAL experts (resident index = latent slot l; t.R / t.NS chosen from the latent-token
// matrices' LDS); small sites run their rounds in different blocks (grid.z).
struct GPreLArgs { P16 glat; int e_of_lat[MAX_E]; GenDims t; };

template <typename T, int NG, int NCG, int KC>
__global__ void __launch_bounds__(gen_max_waves(NG, NCG, KC) * 64) kg_pre_lat_bwd(GPreLArgs a, const float* __restrict__ L2, const float* __restrict__ TT,
                                                      const float* __restrict__ TW, const float* __restrict__ Tsum, const void* __restrict__ ain_,
                                                      const void* __restrict__ dZx_, const float* __restrict__ dslat, void* __restrict__ dL2x_,
                                                      void* __restrict__ aw_, void* __restrict__ ag_, float* __restrict__ blkscal, float* __restrict__ dtbp) {
  constexpr int GD = NCG * 16, DD = NG * GD, Kp = KC * 16, LDK = Kp + 4, LDD = DD + 4;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int PE = Kp * LDK + Kp * LDD + Kp;      // per resident expert: TT^T [Kp][LDK] | TW [Kp][LDD] | tb [Kp]
  const T* ain = (const T*)ain_; const T* dZx = (const T*)dZx_;
  T* dL2x = (T*)dL2x_; T* aw_o = (T*)aw_; T* ag_o = (T*)ag_;
  const GenDims& t = a.t;
  const int E = t.E, El = t.El, DZ = t.DZ, NWV = t.R * t.NS;
  const int s = blockIdx.y, wave = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane & 15, q = lane >> 4;
  const RoundWave rw = round_wave(t);
  float* s_TT = smem + rw.er * PE;
  float* s_TW = s_TT + Kp * LDK;
  float* s_tb = s_TW + Kp * LDD;
  float* s_col = smem + t.R * PE;        // [R * NS][Kp]
  float* s_sc = s_col + NWV * Kp;        // [R * NS]
  const int n_beg = blockIdx.x * t.per, n_end = min(t.N, n_beg + t.per);
  const int blk = blockIdx.y * gridDim.x + blockIdx.x;
  for (int l0 = blockIdx.z * t.R; l0 < El; l0 += t.R * gridDim.z) {
    const bool act = l0 + rw.er < El;
    const int l = act ? l0 + rw.er : El - 1;
    const int e = a.e_of_lat[l];
    const float gv = a.glat.p[e][0];
    __syncthreads();
    for (int k = 0; k < t.R && l0 + k < El; ++k) {
      float* TT_ = smem + k * PE;
      float* TW_ = TT_ + Kp * LDK;
      stage_latent<NG, NCG, KC, false>(TT_, TW_, TW_ + Kp * LDD, TT, TW, Tsum, t, s, l0 + k, a.e_of_lat[l0 + k]);
    }
    __syncthreads();
    float sdg = 0.f;
    float4 ck[KC];
    zero_chunks<KC>(ck);
    int qsel = 0;      // the lane (of the four that hold a token) that takes this tile's scalar terms
    for (int n0 = n_beg + 16 * rw.ts; n0 < (act ? n_end : n_beg); n0 += 16 * t.NS, qsel = (qsel + 1) & 3) {
      const int oz = opaque0();
      const bool ok = n0 + r < t.N;
      const long tok = (long)s * t.N + n0 + r;
      const float dSx = ok ? dslat[(2L * l) * t.NT + tok] : 0.f, dSxx = ok ? dslat[(2L * l + 1) * t.NT + tok] : 0.f;
      float4 twd[KC];                     // sum_dd TW[k][dd] dzraw[dd]  (all groups)
      zero_chunks<KC>(twd);
#pragma unroll
      for (int gi = 0; gi < NG; ++gi) {
        float4 dzr[NCG];
        zero_chunks<NCG>(dzr);
        if (ok) ld_chunks<T, NCG>(dZx + tok * DZ + zcolg(gi, e, E, GD), dzr, q);
#pragma unroll
        for (int ct = 0; ct < KC; ++ct) {
          const f32x4 w = mmT<NCG, sizeof(T) == 2>(s_TW + oz + gi * GD, LDD, 16 * ct, dzr, r, q);
#pragma unroll
          for (int x = 0; x < 4; ++x) at(twd[ct], x) += w[x];
        }
      }
      const long so = tok * t.KLp + (long)l * t.Kp, sa = (long)l * t.aL + tok * t.Kp;      // rows of dL2x ; planes of a / aw / ag
      float4 av[KC], lg[KC];
      zero_chunks<KC>(av);
      if (ok) ld_chunks<T, KC>(ain + sa, av, q);
      float u1 = 0.f, u2 = 0.f, dgr = 0.f;
#pragma unroll
      for (int j = 0; j < KC; ++j) {
        lg[j] = ok ? ld4(L2 + tok * t.KL + (long)l * t.Kp + 16 * j + 4 * q) : zero4();
        const float4 tb = ld4(s_tb + oz + 16 * j + 4 * q);
#pragma unroll
        for (int x = 0; x < 4; ++x) {
          const float ac = at(av[j], x);                           // exactly 0 in the padding slots
          u1 += ac * at(tb, x);
          if (16 * j + 4 * q + x < t.K) u2 += ac * at(lg[j], x);
          dgr += ac * at(twd[j], x);                               // dzraw . (a TW) = a . (TW dzraw)
        }
      }
      u1 = qsum4(u1); u2 = qsum4(u2); dgr = qsum4(dgr);
      const float du1 = dSx * gv * (float)t.C, du2 = 2.f * gv * dSxx, du3 = gv * gv * dSxx;
      float u3 = 0.f, sada = 0.f;
      float4 da[KC];
#pragma unroll
      for (int ct = 0; ct < KC; ++ct) {
        const f32x4 ta = mmT<KC, sizeof(T) == 2>(s_TT + oz, LDK, 16 * ct, av, r, q);
        const float4 tb = ld4(s_tb + oz + 16 * ct + 4 * q);
#pragma unroll
        for (int x = 0; x < 4; ++x) {
          const float ac = at(av[ct], x);
          u3 += ta[x] * ac;
          float d = 0.f;
          if (ok && 16 * ct + 4 * q + x < t.K) {
            d = gv * at(twd[ct], x) + du1 * at(tb, x) + du2 * at(lg[ct], x) + 2.f * du3 * ta[x];
            sada += ac * d;
            at(ck[ct], x) += du1 * ac;
          }
          at(da[ct], x) = d;
        }
      }
      u3 = qsum4(u3); sada = qsum4(sada);
      if (ok && q == qsel) sdg += dSx * (float)t.C * u1 + dSxx * (2.f * u2 + 2.f * gv * u3) + dgr;
      if (ok) {
        float4 v0[KC], v1[KC], v2[KC];
#pragma unroll
        for (int j = 0; j < KC; ++j)
#pragma unroll
          for (int x = 0; x < 4; ++x) {
            const float ac = at(av[j], x);
            at(v0[j], x) = du2 * ac + ac * (at(da[j], x) - sada); at(v1[j], x) = du3 * ac; at(v2[j], x) = gv * ac;
          }
        st_chunks<T, KC>(dL2x + so, v0, q); st_chunks<T, KC>(aw_o + sa, v1, q); st_chunks<T, KC>(ag_o + sa, v2, q);
      }
    }
    const float vg = expert_scalar(wave_sum(sdg), s_sc, rw.er, t);
    if (act && rw.ts == 0 && lane == 0) blkscal[((long)blk * E + e) * 4 + 3] = vg;
#pragma unroll
    for (int j = 0; j < KC; ++j)
#pragma unroll
      for (int x = 0; x < 4; ++x) {
        const float v = rsum16(at(ck[j], x));
        if (r == 0) s_col[wave * Kp + 16 * j + 4 * q + x] = v;
      }
    __syncthreads();
    for (int i = threadIdx.x; i < t.R * Kp; i += blockDim.x) {
      const int k = i / Kp, kk = i % Kp;
      if (l0 + k >= El) continue;
      float v = 0.f;
      for (int u = 0; u < t.NS; ++u) v += s_col[(u * t.R + k) * Kp + kk];
      dtbp[(long)blk * t.KL + (long)(l0 + k) * t.Kp + kk] = v;
    }
    __syncthreads();
  }
}

#endif   // GEN_PART 3, 4
// ---- host side ------------------------------------------------------------------------------------------------------------
GenDims make_gd(const Dims& d, int per) {
  GenDims t;
  t.S = d.S; t.N = d.N; t.C = d.C; t.E = d.E; t.K = d.K; t.Kp = d.Kp; t.El = d.El; t.KL = d.KL; t.KLT = d.KLT; t.KLp = d.KLp; t.KPp = d.KPp;
  t.NT = d.NT; t.per = per; t.DZ = d.DZ; t.XW = d.XW;
  t.R = 1; t.NS = 4;      // (pick_round)
  t.aL = d.aL;
  return t;
}
void gen_grid(const Dims& d, dim3* grid, int* per) {
  const int bps = d.nblk_tok / d.S;
  *per = (int)round_up(cdiv(d.N, bps), 16);
  *grid = dim3((unsigned)bps, (unsigned)d.S);
}
int kc_of(const Dims& d) { return d.El > 0 ? d.Kp / 16 : 1; }

// LDS floats of the largest kernel (pre_small / pre_small_bwd) -- what decides whether a shape is eligible at all
// pe: per resident expert, pw: per wave of the block
void lds_floats_pre_parts(int ng, int ncg, int kc, bool bwd, size_t* pe, size_t* pw) {
  const size_t GD = ncg * 16, DD = ng * GD, Kp = kc * 16;
  if (!bwd) { *pe = Kp * (Kp + 4) + DD * (Kp + 4) + Kp + 2 * DD; *pw = DD; }
  else { *pe = Kp * (Kp + 4) + Kp * (DD + 4) + Kp; *pw = Kp + 1; }      // (the hop-2 kernel of the backward: kg_pre_lat_bwd)
}
size_t lds_floats_pre(int ng, int ncg, int kc, bool bwd) {      // one resident expert, four tile slots (the smallest configuration)
  size_t pe, pw; lds_floats_pre_parts(ng, ncg, kc, bwd, &pe, &pw);
  return pe + 4 * pw;
}
// Experts resident per round and tile slots for a kernel whose constants take `pe` floats of LDS per expert and `pw` per wave: as
// many experts as there are (at most 8 waves; one for blocks of fewer than 64 tokens), as long as a wave's share of the LDS stays within what three waves per SIMD leave
// it (13 KB) -- beyond that the residency lost costs more than the locality gained; at least four waves per block.
void pick_round(int E, size_t pe, size_t pw, int max_waves, int per, int* R, int* NS, size_t* lds_bytes, int excl = 0) {
  // (fewer than four tiles per block: nothing to gain from sharing rows, and four tile slots keep all four waves busy)
  const int top = per < 64 ? 1 : std::min(E, max_waves);
  const int cand[4] = {top, (top + 1) / 2, 2, 1};
  int r = 1;
  for (int c : cand) {
    if (c < 1 || c > E) continue;
    const int ns = std::max(1, 4 / c);
    if (c == 1 || (pe * c + pw * c * ns) * 4 <= (size_t)13 * 1024 * c * ns) { r = c; break; }
  }
  if (const char* ev = switches().gen_r) r = std::max(1, std::min(top, atoi(ev)));      // development: A/B of the round size
  // excl (one block per CU, gen_lds_request): as many waves as the instance is compiled for, so that the CU is not left at four waves
  const int waves = (excl && per >= 128) ? max_waves : 4;
  *R = r; *NS = std::max(1, waves / r);
  *lds_bytes = (pe * r + pw * r * (*NS)) * 4;
}

// Dims::excl (other kernels may share the GPU with this call): every launch of this family asks for 150 KB of dynamic LDS, so that
// a block has its compute unit's LDS to itself and no block of another kernel lands beside it -- a block of these kernels that
// shares a CU with a bf16 GEMM block of the engine (wide LDS reads beside matrix instructions) gets wrong 16-byte LDS reads now and
// then on MI355X / ROCm 7.2 (round 4: two-stream AdapterPair at the tile_gen sites, 15 of 35 steps moved; with the request 0 of 35;
// scripts/mfma_probe.hip shows the same with two stand-alone kernels: 887 674 wrong sums -> 0).  One block per CU costs residency
// where the grid is larger than the chip; alone on the GPU (Dims::excl = 0) nothing changes.
// (development: AVMOE_GEN_HOG=<bytes> forces a request for every launch)
constexpr size_t GEN_EXCL_LDS = 150 * 1024;
static inline size_t gen_lds_request(size_t need, int excl) {
  const long hog = switches().gen_hog;
  if (hog >= 0) return std::max(need, (size_t)hog);
  return excl ? std::max(need, GEN_EXCL_LDS) : need;
}

int set_dyn_lds(const void* fn, size_t bytes, const char* what) {
  if (bytes <= 65536) return OK;
  if (bytes > 160 * 1024) { set_last_error("%s needs %zu B of LDS", what, bytes); return ERR_UNSUPPORTED; }
  // the limit (not this launch's size), once per kernel function and device: with Dims::excl every launch is above 64 KB
  static std::mutex mu;
  static std::vector<std::pair<const void*, int>> done;
  int dev = 0;
  (void)hipGetDevice(&dev);
  {
    std::lock_guard<std::mutex> lk(mu);
    for (const auto& p : done) if (p.first == fn && p.second == dev) return OK;
  }
  hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
  if (e != hipSuccess) { (void)hipGetLastError(); set_last_error("%s: LDS attribute: %s", what, hipGetErrorString(e)); return ERR_LAUNCH; }
  std::lock_guard<std::mutex> lk(mu);
  done.emplace_back(fn, dev);
  return OK;
}

// the (groups, chunks per group, latent chunks) combinations that are built
#define GEN_SHAPES(X)                                                                                                  \
  X(1, 1) X(1, 2) X(1, 3) X(1, 4) X(1, 6) X(2, 1) X(2, 2) X(2, 3) X(2, 4) X(2, 6) X(4, 1) X(4, 2) X(4, 3)
#define GEN_KCS(X, NG, NCG) X(NG, NCG, 1) X(NG, NCG, 2) X(NG, NCG, 6)

}  // namespace

#if GEN_PART == 5
bool tile_gen_ok(const Dims& d) {
  if (d.dgp % 16 || (d.El > 0 && d.Kp % 16)) return false;
  const int ncg = d.dgp / 16, kc = kc_of(d);
  bool shape = false;
#define X(NG, NCG) shape = shape || (d.g == NG && ncg == NCG);
  GEN_SHAPES(X)
#undef X
  if (!shape || !(kc == 1 || kc == 2 || kc == 6)) return false;
  return lds_floats_pre(d.g, ncg, kc, false) * 4 <= 160 * 1024 && lds_floats_pre(d.g, ncg, kc, true) * 4 <= 160 * 1024;
}

#endif   // GEN_PART == 5 (tile_gen_ok)

// Sites with few token blocks (late backbone stages: 36 .. 256 tokens per frame) are bound by the per-expert prologues -- staging a
// frame's matrices -- run one after the other by the same few blocks: there the rounds of a kernel whose experts do not depend on
// each other go to different blocks (grid.z), eight times the blocks at cfg-5 (k_post_small_bwd on 2560 tokens: 309 us before).
static inline void spread_rounds(dim3* grid, const GenDims& t) {
  if ((long)grid->x * grid->y < 384) grid->z = (unsigned)((t.E + t.R - 1) / t.R);
}
// (the block: 64 threads per resident expert and tile slot -- a.t.R, a.t.NS)
#define LAUNCH_ONE(KF, SH, ...)                                                                                         \
  do {                                                                                                                  \
    const size_t sh__ = gen_lds_request(SH, d.excl);                                                                    \
    AVMOE_TRY(set_dyn_lds((const void*)KF, sh__, "tile_gen"));                                                          \
    hipLaunchKernelGGL(KF, grid, dim3(64 * a.t.R * a.t.NS), sh__, st, __VA_ARGS__);                                     \
  } while (0)

#if GEN_PART == 5
int kg_mid(PassCall& c, hipStream_t st) {
  const Plan& pl = c.pl; const Dims& d = pl.d; char* saved = c.saved; char* scratch = c.scratch;
  if (!d.gen) return 1;
  dim3 grid; int per; gen_grid(d, &grid, &per);
  GMidFArgs a;
  put(a.relu_of_e, c.x.relu_of_e);
  a.t = make_gd(d, per);
  size_t sh; pick_round(d.E, 2 * (size_t)d.DD, (size_t)d.DD, gen_max_waves(d.g, d.dgp / 16, 0), per, &a.t.R, &a.t.NS, &sh, d.excl);
  spread_rounds(&grid, a.t);
  const int ncg = d.dgp / 16; bool done = false;
#define X(NG, NCG)                                                                                                      \
  if (!done && d.g == NG && ncg == NCG) {                                                                               \
    done = true;                                                                                                        \
    if (d.bf16) LAUNCH_ONE((kg_mid<__bf16, NG, NCG>), sh, a, (const void*)(saved + pl.o_Z), (const float*)(saved + pl.o_bn1), (void*)(scratch + pl.o_Zp), (float*)(scratch + pl.o_colpart)); \
    else LAUNCH_ONE((kg_mid<float, NG, NCG>), sh, a, (const void*)(saved + pl.o_Z), (const float*)(saved + pl.o_bn1), (void*)(scratch + pl.o_Zp), (float*)(scratch + pl.o_colpart)); \
  }
  GEN_SHAPES(X)
#undef X
  if (!done) { set_last_error("mid: shape not built"); return ERR_UNSUPPORTED; }
  AVMOE_CHECK_LAUNCH("mid (general)");
  c.ran = PASS_GEN;
  return OK;
}

int kg_mid_bwd(PassCall& c, hipStream_t st) {
  const Plan& pl = c.pl; const Dims& d = pl.d; char* saved = c.saved; char* scratch = c.scratch;
  if (!d.gen) return 1;
  dim3 grid; int per; gen_grid(d, &grid, &per);
  GMidArgs a;
  put(a.relu_of_e, c.x.relu_of_e);
  a.t = make_gd(d, per); a.moments = d.use_bn && d.training;
  size_t sh; pick_round(d.E, (size_t)d.DD * (d.dgp + 4) + 5 * d.DD, (size_t)d.DD, gen_max_waves(d.g, d.dgp / 16, 0), per, &a.t.R, &a.t.NS, &sh, d.excl);
  spread_rounds(&grid, a.t);
  const int ncg = d.dgp / 16; bool done = false;
#define MB_ARGS a, (const void*)(saved + pl.o_Z), (const float*)(saved + pl.o_bn1), (const float*)(scratch + pl.o_dsm), (const float*)(scratch + pl.o_sdSzz), \
                (void*)(scratch + pl.o_dzp), (float*)(scratch + pl.o_colpart)
#define X(NG, NCG)                                                                                                      \
  if (!done && d.g == NG && ncg == NCG) {                                                                               \
    done = true;                                                                                                        \
    if (d.bf16) LAUNCH_ONE((kg_mid_bwd<__bf16, NG, NCG>), sh, MB_ARGS); else LAUNCH_ONE((kg_mid_bwd<float, NG, NCG>), sh, MB_ARGS);   \
  }
  GEN_SHAPES(X)
#undef X
#undef MB_ARGS
  if (!done) { set_last_error("mid_bwd: shape not built"); return ERR_UNSUPPORTED; }
  AVMOE_CHECK_LAUNCH("mid_bwd (general)");
  c.ran = PASS_GEN;
  return OK;
}

int kg_post_small(PassCall& c, hipStream_t st) {
  const Plan& pl = c.pl; const Dims& d = pl.d; char* saved = c.saved; char* scratch = c.scratch;
  if (!d.gen) return 1;
  dim3 grid; int per; gen_grid(d, &grid, &per);
  GPostArgs a;
  a.gate = c.x.gate; put(a.relu_of_e, c.x.relu_of_e);
  a.t = make_gd(d, per); a.ln_post = d.ln_post; a.use_gate = d.use_gate && !d.gate_w; a.ln_eps = d.ln_eps;
  size_t sh; pick_round(d.E, (size_t)d.DD * (d.dgp + 4) + 4 * d.DD, 0, gen_max_waves(d.g, d.dgp / 16, 0), per, &a.t.R, &a.t.NS, &sh, d.excl);
  spread_rounds(&grid, a.t);
  const int ncg = d.dgp / 16; bool done = false;
#define PS_ARGS a, (const void*)(saved + pl.o_Z), (const float*)(saved + pl.o_bn1), (const float*)(saved + pl.o_Gq), (const float*)(saved + pl.o_uvh), \
                (const float*)(saved + pl.o_probs), (void*)(saved + pl.o_Apost), (float*)(saved + pl.o_rpmup)
#define X(NG, NCG)                                                                                                      \
  if (!done && d.g == NG && ncg == NCG) {                                                                               \
    done = true;                                                                                                        \
    if (d.bf16) LAUNCH_ONE((kg_post_small<__bf16, NG, NCG>), sh, PS_ARGS); else LAUNCH_ONE((kg_post_small<float, NG, NCG>), sh, PS_ARGS); \
  }
  GEN_SHAPES(X)
#undef X
#undef PS_ARGS
  if (!done) { set_last_error("post_small: shape not built"); return ERR_UNSUPPORTED; }
  AVMOE_CHECK_LAUNCH("post_small (general)");
  c.ran = PASS_GEN;
  return OK;
}

int kg_post_small_bwd(PassCall& c, hipStream_t st) {
  const Plan& pl = c.pl; const Dims& d = pl.d; char* saved = c.saved; char* scratch = c.scratch;
  if (!d.gen) return 1;
  dim3 grid; int per; gen_grid(d, &grid, &per);
  GPostBArgs a;
  a.gate = c.x.gate; put(a.relu_of_e, c.x.relu_of_e);
  a.t = make_gd(d, per); a.ln_post = d.ln_post; a.use_gate = d.use_gate && !d.gate_w;
  a.dApx = (const float*)(scratch + pl.o_dApx); a.dapw = d.E * d.dgp;
  a.dSooT = d.gram64 ? (float*)(scratch + pl.o_dSooT) : nullptr;
  if (c.dap16 && !d.bf16) { set_last_error("post_small_bwd: split dApost is a bf16 form"); return ERR_BAD_ARG; }
  size_t sh; pick_round(d.E, (size_t)d.DD * (d.dgp + 4) + 4 * d.DD, (size_t)d.DD + 1, gen_max_waves(d.g, d.dgp / 16, 0), per, &a.t.R, &a.t.NS, &sh, d.excl);
  spread_rounds(&grid, a.t);
  const int ncg = d.dgp / 16; bool done = false;
#define PB_ARGS a, (const void*)(saved + pl.o_Z), (const float*)(saved + pl.o_bn1), (const float*)(saved + pl.o_Gq), (const float*)(saved + pl.o_uvh), \
                (const float*)(saved + pl.o_probs), (const float*)(saved + pl.o_rpmup), (const void*)(scratch + pl.o_dAp), (void*)(scratch + pl.o_dzp), \
                (void*)(scratch + pl.o_Zp), (void*)(scratch + pl.o_Zw), (float*)(scratch + pl.o_colpart), (float*)(scratch + pl.o_blkscal)
#define X(NG, NCG)                                                                                                      \
  if (!done && d.g == NG && ncg == NCG) {                                                                               \
    done = true;                                                                                                        \
    if (c.dap16) LAUNCH_ONE((kg_post_small_bwd<__bf16, NG, NCG, true>), sh, PB_ARGS);                                     \
    else if (d.bf16) LAUNCH_ONE((kg_post_small_bwd<__bf16, NG, NCG, false>), sh, PB_ARGS);                              \
    else LAUNCH_ONE((kg_post_small_bwd<float, NG, NCG, false>), sh, PB_ARGS);                                           \
  }
  GEN_SHAPES(X)
#undef X
#undef PB_ARGS
  if (!done) { set_last_error("post_small_bwd: shape not built"); return ERR_UNSUPPORTED; }
  AVMOE_CHECK_LAUNCH("post_small_bwd (general)");
  c.ran = PASS_GEN;
  return OK;
}

#endif   // GEN_PART == 5

// pre_small / pre_small_bwd: one translation unit per activation type (tile_gen_pre_{f32,bf16}.hip, tile_gen_preb_{f32,bf16}.hip)
#if GEN_PART >= 1 && GEN_PART <= 4
#if GEN_PART == 1 || GEN_PART == 3
typedef float GenT;
#define GEN_FN(base) base##_f32
#else
typedef __bf16 GenT;
#define GEN_FN(base) base##_bf16
#endif
#endif

#if GEN_PART == 1 || GEN_PART == 2
int GEN_FN(kg_pre_small)(PassCall& c, hipStream_t st) {
  const Plan& pl = c.pl; const Dims& d = pl.d; char* saved = c.saved; char* scratch = c.scratch;
  dim3 grid; int per; gen_grid(d, &grid, &per);
  GPreArgs a;
  a.glat = c.x.glat; put(a.lat_of_e, c.x.lat_of_e); put(a.nxn_of_e, c.x.nxn_of_e); put(a.sxr_off, c.x.sxr_off);
  a.ZR = (const float*)(saved + pl.o_ZR); a.sxr = (const float*)(saved + pl.o_sxr);
  a.t = make_gd(d, per); a.ln_before = d.ln_before; a.ln_eps = d.ln_eps;
  const int ncg = d.dgp / 16, kc = kc_of(d); bool done = false;
  size_t sh, pe, pw; lds_floats_pre_parts(d.g, ncg, kc, false, &pe, &pw);
  pick_round(d.E, pe, pw, gen_max_waves(d.g, ncg, kc), per, &a.t.R, &a.t.NS, &sh, d.excl);
  spread_rounds(&grid, a.t);
#define PR_ARGS a, (void*)(saved + pl.o_Z), (const float*)(saved + pl.o_L2), (const float*)(saved + pl.o_sx), (const float*)(saved + pl.o_TT), \
                (const float*)(saved + pl.o_TW), (const float*)(saved + pl.o_Tsum), (const float*)(saved + pl.o_wsum), (const float*)(saved + pl.o_dconst), \
                (void*)(saved + pl.o_a), (float*)(saved + pl.o_rmu), (float*)(scratch + pl.o_colpart)
#define Y(NG, NCG, KC_)                                                                                                 \
  if (!done && d.g == NG && ncg == NCG && kc == KC_) {                                                                  \
    done = true;                                                                                                        \
    if (d.nxn) LAUNCH_ONE((kg_pre_small<GenT, NG, NCG, KC_, true>), sh, PR_ARGS);                                       \
    else LAUNCH_ONE((kg_pre_small<GenT, NG, NCG, KC_, false>), sh, PR_ARGS);                                            \
  }
#define X(NG, NCG) GEN_KCS(Y, NG, NCG)
  GEN_SHAPES(X)
#undef X
#undef Y
#undef PR_ARGS
  if (!done) { set_last_error("pre_small: shape not built"); return ERR_UNSUPPORTED; }
  AVMOE_CHECK_LAUNCH("pre_small (general)");
  return OK;
}

#endif   // GEN_PART 1, 2

#if GEN_PART == 3 || GEN_PART == 4
int GEN_FN(kg_pre_small_bwd)(PassCall& c, hipStream_t st) {
  const Plan& pl = c.pl; const Dims& d = pl.d; char* saved = c.saved; char* scratch = c.scratch;
  dim3 grid; int per; gen_grid(d, &grid, &per);
  const int ncg = d.dgp / 16, kc = kc_of(d);
  {   // ---- every expert: BN1 / LayerNorm part ----
    GPreBArgs a;
    a.glat = c.x.glat; put(a.lat_of_e, c.x.lat_of_e); put(a.nxn_of_e, c.x.nxn_of_e); put(a.first_of_slot, c.x.first_of_slot); put(a.sxr_off, c.x.sxr_off);
    a.ZR = (const float*)(saved + pl.o_ZR); a.sxr = (const float*)(saved + pl.o_sxr);
    a.dZR = (void*)(scratch + pl.o_dZR); a.dsr = (float*)(scratch + pl.o_dsr);
    a.t = make_gd(d, per); a.ln_before = d.ln_before; a.use_bn = d.use_bn; a.bn_train = d.use_bn && d.training;
    size_t sh; pick_round(d.E, 7 * (size_t)d.DD, (size_t)d.DD + 1 + 64, gen_max_waves(d.g, ncg, 0), per, &a.t.R, &a.t.NS, &sh, d.excl);
    bool done = false;
#define PB_ARGS a, (const void*)(saved + pl.o_Z), (const float*)(saved + pl.o_wsum), (const float*)(saved + pl.o_dconst), (const float*)(saved + pl.o_rmu), \
                (const float*)(saved + pl.o_bn1), (const float*)(scratch + pl.o_dsm), (const void*)(scratch + pl.o_dzp), (void*)(scratch + pl.o_Zw), \
                (void*)(scratch + pl.o_dL2x), (float*)(scratch + pl.o_dslat), (float*)(scratch + pl.o_dsxs), (float*)(scratch + pl.o_rs2x), \
                (float*)(scratch + pl.o_colpart), (float*)(scratch + pl.o_blkscal)
#define X(NG, NCG)                                                                                                      \
    if (!done && d.g == NG && ncg == NCG) {                                                                             \
      done = true;                                                                                                      \
      if (d.nxn) LAUNCH_ONE((kg_pre_small_bwd<GenT, NG, NCG, true>), sh, PB_ARGS);                                      \
      else LAUNCH_ONE((kg_pre_small_bwd<GenT, NG, NCG, false>), sh, PB_ARGS);                                           \
    }
    GEN_SHAPES(X)
#undef X
#undef PB_ARGS
    if (!done) { set_last_error("pre_small_bwd: shape not built"); return ERR_UNSUPPORTED; }
    AVMOE_CHECK_LAUNCH("pre_small_bwd (general)");
  }
  if (d.El > 0) {   // ---- the cross-modal experts' hop-2 block (after the kernel above on the same stream: reads dZx and dslat) ----
    GPreLArgs a;
    a.glat = c.x.glat; put(a.e_of_lat, c.x.e_of_lat);
    a.t = make_gd(d, per);
    const size_t Kp = (size_t)kc * 16;
    size_t sh; pick_round(d.El, Kp * (Kp + 4) + Kp * ((size_t)d.DD + 4) + Kp, Kp + 1, gen_max_waves(d.g, ncg, kc), per, &a.t.R, &a.t.NS, &sh, d.excl);
    if ((long)grid.x * grid.y < 384) grid.z = (unsigned)((d.El + a.t.R - 1) / a.t.R);
    bool done = false;
#define PL_ARGS a, (const float*)(saved + pl.o_L2), (const float*)(saved + pl.o_TT), (const float*)(saved + pl.o_TW), (const float*)(saved + pl.o_Tsum), \
                (const void*)(saved + pl.o_a), (const void*)(scratch + pl.o_Zw), (const float*)(scratch + pl.o_dslat), (void*)(scratch + pl.o_dL2x), \
                (void*)(scratch + pl.o_aw), (void*)(scratch + pl.o_ag), (float*)(scratch + pl.o_blkscal), (float*)(scratch + pl.o_dtbp)
#define Y(NG, NCG, KC_)                                                                                                 \
    if (!done && d.g == NG && ncg == NCG && kc == KC_) {                                                                \
      done = true;                                                                                                      \
      LAUNCH_ONE((kg_pre_lat_bwd<GenT, NG, NCG, KC_>), sh, PL_ARGS);                                                    \
    }
#define X(NG, NCG) GEN_KCS(Y, NG, NCG)
    GEN_SHAPES(X)
#undef X
#undef Y
#undef PL_ARGS
    if (!done) { set_last_error("pre_lat_bwd: shape not built"); return ERR_UNSUPPORTED; }
    AVMOE_CHECK_LAUNCH("pre_lat_bwd (general)");
  }
  return OK;
}
#endif   // GEN_PART 3, 4

#if GEN_PART == 5
int kg_pre_small_f32(PassCall&, hipStream_t);
int kg_pre_small_bf16(PassCall&, hipStream_t);
int kg_pre_small_bwd_f32(PassCall&, hipStream_t);
int kg_pre_small_bwd_bf16(PassCall&, hipStream_t);
int kg_pre_small(PassCall& c, hipStream_t st) {
  if (!c.pl.d.gen) return 1;
  return launched(c, PASS_GEN, c.pl.d.bf16 ? kg_pre_small_bf16(c, st) : kg_pre_small_f32(c, st));
}
int kg_pre_small_bwd(PassCall& c, hipStream_t st) {
  if (!c.pl.d.gen) return 1;
  return launched(c, PASS_GEN, c.pl.d.bf16 ? kg_pre_small_bwd_bf16(c, st) : kg_pre_small_bwd_f32(c, st));
}
#endif

}  // namespace avmoe
