// Device helpers shared by the register-resident bottleneck-space kernels (tile_fast.hip) and their streaming form (tile_stream.hip):
// what belongs to their shape (bottleneck 64 in 2 groups of 32, 32 latent tokens) -- the dimensions, whole-row accesses in unpacked and
// raw form, the wave-per-expert folds of column / scalar accumulators.  The shape-independent lane-layout primitives (reductions,
// packed bf16 segments, the transposed mat-vec, the batched fill) come from tile_lane.h.  Included inside `namespace avmoe`; everything
// lives in an anonymous namespace (one copy per translation unit).
#pragma once
#include "tile_lane.h"

namespace {

constexpr int FDD = 64;     // bottleneck width of one expert (2 groups x 32)
constexpr int FDG = 32;     // per group
constexpr int FK = 32;      // latent tokens
constexpr int LD32 = 36;    // leading dim of LDS matrices with 32 columns   (4*ld = 16 mod 32: conflict-free A-operand reads)
constexpr int LD64 = 68;    // ... with 64 columns

struct FastDims { int S, N, C, El, KL, KLT, KLp, KPp, NT, per; long aL; };      // aL: plane stride of a / aw / ag ([slot][token][32])
// per: the tokens of a frame that one virtual block takes (Dims::nblk_tok blocks over the S frames), in whole 16-token tiles
inline int tok_per_vblock(const Dims& d) { return (int)round_up(cdiv(d.N, d.nblk_tok / d.S), 16); }
inline FastDims make_fd(const Dims& d) {
  FastDims t;
  t.S = d.S; t.N = d.N; t.C = d.C; t.El = d.El; t.KL = d.KL; t.KLT = d.KLT; t.KLp = d.KLp; t.KPp = d.KPp; t.NT = d.NT; t.per = tok_per_vblock(d); t.aL = d.aL;
  return t;
}

// one expert's 64 bottleneck entries of a Z-space row ([group][expert][32], element type T): chunks v[0..3]
template <typename T, int E> __device__ __forceinline__ void ld_row(const T* row, int e, int q, float4 (&v)[4]) {
  ld_seg<T>(row + e * FDG, v[0], v[1], q); ld_seg<T>(row + E * FDG + e * FDG, v[2], v[3], q);
}
template <typename T, int E> __device__ __forceinline__ void st_row(T* row, int e, int q, const float4 (&v)[4]) {
  st_seg<T>(row + e * FDG, v[0], v[1], q); st_seg<T>(row + E * FDG + e * FDG, v[2], v[3], q);
}
// the same row as RAW registers (bf16: 2 x 16 bytes): several tiles' loads are kept in flight in this form and only
// unpacked (quad exchange + widen) when a tile is computed
template <typename T> struct RawRow;
template <> struct RawRow<float> { float4 v[4]; };
template <> struct RawRow<__bf16> { uint4 v[2]; };
template <int E> __device__ __forceinline__ void ldraw_row(const float* row, int e, int q, RawRow<float>& o) {
  o.v[0] = *(const float4*)(row + e * FDG + 4 * q); o.v[1] = *(const float4*)(row + e * FDG + 16 + 4 * q);
  o.v[2] = *(const float4*)(row + E * FDG + e * FDG + 4 * q); o.v[3] = *(const float4*)(row + E * FDG + e * FDG + 16 + 4 * q);
}
template <int E> __device__ __forceinline__ void ldraw_row(const __bf16* row, int e, int q, RawRow<__bf16>& o) {
  o.v[0] = *(const uint4*)(row + e * FDG + seg_off8(q)); o.v[1] = *(const uint4*)(row + E * FDG + e * FDG + seg_off8(q));
}
__device__ __forceinline__ void zero_raw(RawRow<float>& o) { o.v[0] = o.v[1] = o.v[2] = o.v[3] = make_float4(0.f, 0.f, 0.f, 0.f); }
__device__ __forceinline__ void zero_raw(RawRow<__bf16>& o) { o.v[0] = o.v[1] = make_uint4(0u, 0u, 0u, 0u); }
__device__ __forceinline__ void unpack_row(const RawRow<float>& i, float4 (&v)[4]) { v[0] = i.v[0]; v[1] = i.v[1]; v[2] = i.v[2]; v[3] = i.v[3]; }
__device__ __forceinline__ void unpack_seg(const uint4& u, float4& c0, float4& c1) {
  const auto s0 = __builtin_amdgcn_permlane16_swap(u.x, u.z, false, false);
  const auto s1 = __builtin_amdgcn_permlane16_swap(u.y, u.w, false, false);
  c0 = make_float4(__uint_as_float(s0[0] << 16), __uint_as_float(s0[0] & 0xffff0000u), __uint_as_float(s1[0] << 16), __uint_as_float(s1[0] & 0xffff0000u));
  c1 = make_float4(__uint_as_float(s0[1] << 16), __uint_as_float(s0[1] & 0xffff0000u), __uint_as_float(s1[1] << 16), __uint_as_float(s1[1] & 0xffff0000u));
}
__device__ __forceinline__ void unpack_row(const RawRow<__bf16>& i, float4 (&v)[4]) { unpack_seg(i.v[0], v[0], v[1]); unpack_seg(i.v[1], v[2], v[3]); }
// one 32-entry segment in raw form
template <typename T> struct RawSeg;
template <> struct RawSeg<float> { float4 v[2]; };
template <> struct RawSeg<__bf16> { uint4 v; };
__device__ __forceinline__ void zero_raw(RawSeg<float>& o) { o.v[0] = o.v[1] = make_float4(0.f, 0.f, 0.f, 0.f); }
__device__ __forceinline__ void zero_raw(RawSeg<__bf16>& o) { o.v = make_uint4(0u, 0u, 0u, 0u); }
__device__ __forceinline__ void ldraw_seg(const float* seg, int q, RawSeg<float>& o) { o.v[0] = *(const float4*)(seg + 4 * q); o.v[1] = *(const float4*)(seg + 16 + 4 * q); }
__device__ __forceinline__ void ldraw_seg(const __bf16* seg, int q, RawSeg<__bf16>& o) { o.v = *(const uint4*)(seg + seg_off8(q)); }
__device__ __forceinline__ void unpack_rawseg(const RawSeg<float>& i, float4& c0, float4& c1) { c0 = i.v[0]; c1 = i.v[1]; }
__device__ __forceinline__ void unpack_rawseg(const RawSeg<__bf16>& i, float4& c0, float4& c1) { unpack_seg(i.v, c0, c1); }
__device__ __forceinline__ void zero_row(float4 (&v)[4]) { v[0] = v[1] = v[2] = v[3] = make_float4(0.f, 0.f, 0.f, 0.f); }

// column offset of chunk c (dd = 16 c + 4 q ..) of expert e inside a Z-space row [group][expert][32]
template <int E> __device__ __forceinline__ int zcol(int c, int e, int q) { return (c >> 1) * (E * FDG) + e * FDG + (c & 1) * 16 + 4 * q; }

// ---- wave-per-expert form --------------------------------------------------------------------------------------------------
// The waves of a block take DIFFERENT experts of the SAME 16-token tiles (wave = tile slot * E + expert), so the E 64-byte segments
// of a Z-space row [group][expert][32] are requested within the same few hundred cycles -- one DRAM page, neighbouring sectors of
// the same lines -- instead of E sweeps over the block's tokens apart.  Measured on kf_mid_bwd at the cfg-2 audio site (same
// bytes, same occupancy): 183 -> 125 us; with an expert-outer loop the HBM traffic is the same but every sweep touches one
// 64-byte sector in four of each row.
template <int E> struct WE {
  static constexpr int NS = (E == 2) ? 2 : 1;      // tile slots: tiles a block works on at a time
  static constexpr int NW = E * NS, NTHR = 64 * NW;
};
// fold per-lane token-slot accumulators (acc[c][x] for dd = 16 c + 4 q + x of expert e) over the 16 token slots and the tile slots,
// then write colpart[blk][slot][colmap(e, dd)]          s_x: [NW][64]
template <int E>
__device__ __forceinline__ void flush_cols_we(float4 (&acc)[4], float* s_x, float* colpart, int blk, int slot, int e, int ts) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane & 15, q = lane >> 4;
#pragma unroll
  for (int c = 0; c < 4; ++c)
#pragma unroll
    for (int x = 0; x < 4; ++x) {
      const float v = rsum16(at(acc[c], x));
      if (r == 0) s_x[wave * FDD + 16 * c + 4 * q + x] = v;
    }
  __syncthreads();
  if (ts == 0) {
    const int dd = lane;
    float v = 0.f;
#pragma unroll
    for (int u = 0; u < WE<E>::NS; ++u) v += s_x[(u * E + e) * FDD + dd];
    colpart[((long)blk * 4 + slot) * (E * FDD) + (dd >> 5) * (E * FDG) + e * FDG + (dd & 31)] = v;
  }
  __syncthreads();
}
// sum of per-wave values (already wave-uniform) over the tile slots of expert e          s_w: [NW]
template <int E>
__device__ __forceinline__ float expert_scalar(float v, float* s_w, int e) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  __syncthreads();
  if (lane == 0) s_w[wave] = v;
  __syncthreads();
  float o = 0.f;
#pragma unroll
  for (int u = 0; u < WE<E>::NS; ++u) o += s_w[u * E + e];
  return o;
}

}  // namespace
