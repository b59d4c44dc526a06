// Lane-layout helpers of the register-resident bottleneck-space kernels, whatever their shape: the tuned 64 / 32 / 32 instance
// (tile_fast.hip), its streaming form (tile_stream.hip) and the generalised family (tile_gen.inc).  A wavefront owns 16 tokens; lane
// (r = lane & 15, q = lane >> 4) holds, for token r, the entries 16 c + 4 q + x (c = chunk, x = 0..3) of a row.  Here: the reductions
// over a token's four lanes and over a tile's sixteen tokens, packed bf16 segment accesses, the transposed mat-vec on the matrix pipe
// and the batched global -> LDS fill.  Device-only; included inside `namespace avmoe`; everything lives in an anonymous namespace
// (one copy per translation unit).
#pragma once

namespace {

// reductions over the 4 lanes that hold one token (same r, q = 0..3): the gfx950 row swaps v_permlane16_swap (rows 0<->1,
// 2<->3) and v_permlane32_swap (rows 0,1 <-> 2,3) -- plain VALU, no LDS crossbar round trip as with ds_bpermute
__device__ __forceinline__ float qsum4(float v) {
  const unsigned u = __float_as_uint(v);
  const auto a = __builtin_amdgcn_permlane16_swap(u, u, false, false);
  const float w = __uint_as_float(a[0]) + __uint_as_float(a[1]);
  const unsigned x = __float_as_uint(w);
  const auto b = __builtin_amdgcn_permlane32_swap(x, x, false, false);
  return __uint_as_float(b[0]) + __uint_as_float(b[1]);
}
__device__ __forceinline__ float qmax4(float v) {
  const unsigned u = __float_as_uint(v);
  const auto a = __builtin_amdgcn_permlane16_swap(u, u, false, false);
  const float w = fmaxf(__uint_as_float(a[0]), __uint_as_float(a[1]));
  const unsigned x = __float_as_uint(w);
  const auto b = __builtin_amdgcn_permlane32_swap(x, x, false, false);
  return fmaxf(__uint_as_float(b[0]), __uint_as_float(b[1]));
}
// sum over the 16 lanes of a row (all tokens of the tile, fixed q): DPP adds -- quad swaps, then half-row and row mirrors
// (after the quad steps every quad is uniform, so a mirror pairs the right partners)
template <int CTRL> __device__ __forceinline__ float dpp_f(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, true));
}
__device__ __forceinline__ float rsum16(float v) {
  v += dpp_f<0xB1>(v);      // quad_perm [1,0,3,2]
  v += dpp_f<0x4E>(v);      // quad_perm [2,3,0,1]
  v += dpp_f<0x141>(v);     // row_half_mirror
  v += dpp_f<0x140>(v);     // row_mirror
  return v;
}
// an integer the optimiser cannot see through (always 0): added to LDS offsets inside the tile loops so that the per-expert
// constants are re-read from LDS each tile instead of being hoisted into (and spilled from) registers
__device__ __forceinline__ int opaque0() { int v = 0; asm volatile("" : "+v"(v)); return v; }
__device__ __forceinline__ float4 ld4(const float* p) { return *(const float4*)p; }
__device__ __forceinline__ float4 zero4() { return make_float4(0.f, 0.f, 0.f, 0.f); }
__device__ __forceinline__ float& at(float4& v, int x) { return ((float*)&v)[x]; }
__device__ __forceinline__ float at(const float4& v, int x) { return ((const float*)&v)[x]; }
// a value as it reads back from a tensor of element type T
template <typename T> __device__ __forceinline__ float rndT(float v);
template <> __device__ __forceinline__ float rndT<float>(float v) { return v; }
template <> __device__ __forceinline__ float rndT<__bf16>(float v) { return bf2f(f2bf(v)); }

// ---- 32-wide bf16 segments (one expert's 32 bottleneck entries of a group / one latent slot's 32 tokens / a pair of 16-entry chunks)
// as ONE 16-byte access per lane: lanes q and q^1 trade quads with v_permlane16_swap, so that lane q even holds entries 4q .. 4q+7 of
// the first 16-chunk and lane q odd entries 4(q-1) .. 4(q-1)+7 of the second -- the four q lanes cover the 64-byte segment contiguously.
// (fp32 tensors keep their two 16-byte accesses per lane.)  The swap is its own inverse: loads use it the other way round.
__device__ __forceinline__ int seg_off8(int q) { return (q & 1) * 16 + (q >> 1) * 8; }
template <typename T> __device__ __forceinline__ void st_seg(T* seg, const float4& c0, const float4& c1, int q);
template <> __device__ __forceinline__ void st_seg<float>(float* seg, const float4& c0, const float4& c1, int q) {
  *(float4*)(seg + 4 * q) = c0; *(float4*)(seg + 16 + 4 * q) = c1;
}
template <> __device__ __forceinline__ void st_seg<__bf16>(__bf16* seg, const float4& c0, const float4& c1, int q) {
  const unsigned a0 = (unsigned)f2bf(c0.x) | ((unsigned)f2bf(c0.y) << 16), a1 = (unsigned)f2bf(c0.z) | ((unsigned)f2bf(c0.w) << 16);
  const unsigned b0 = (unsigned)f2bf(c1.x) | ((unsigned)f2bf(c1.y) << 16), b1 = (unsigned)f2bf(c1.z) | ((unsigned)f2bf(c1.w) << 16);
  const auto s0 = __builtin_amdgcn_permlane16_swap(a0, b0, false, false);
  const auto s1 = __builtin_amdgcn_permlane16_swap(a1, b1, false, false);
  *(uint4*)(seg + seg_off8(q)) = make_uint4(s0[0], s1[0], s0[1], s1[1]);
}
template <typename T> __device__ __forceinline__ void ld_seg(const T* seg, float4& c0, float4& c1, int q);
template <> __device__ __forceinline__ void ld_seg<float>(const float* seg, float4& c0, float4& c1, int q) {
  c0 = *(const float4*)(seg + 4 * q); c1 = *(const float4*)(seg + 16 + 4 * q);
}
template <> __device__ __forceinline__ void ld_seg<__bf16>(const __bf16* seg, float4& c0, float4& c1, int q) {
  const uint4 u = *(const uint4*)(seg + seg_off8(q));
  const auto s0 = __builtin_amdgcn_permlane16_swap(u.x, u.z, false, false);
  const auto s1 = __builtin_amdgcn_permlane16_swap(u.y, u.w, false, false);
  c0 = make_float4(__uint_as_float(s0[0] << 16), __uint_as_float(s0[0] & 0xffff0000u), __uint_as_float(s1[0] << 16), __uint_as_float(s1[0] & 0xffff0000u));
  c1 = make_float4(__uint_as_float(s0[1] << 16), __uint_as_float(s0[1] & 0xffff0000u), __uint_as_float(s1[1] << 16), __uint_as_float(s1[1] & 0xffff0000u));
}

// ---- the transposed mat-vec ---------------------------------------------------------------------------------------------------
// W[tok r][col0 + 4 q + x] = sum over NJ chunks of  P[r][16 j + 4 q' + x'] * M[16 j + 4 q' + x'][col0 + ...]
// Mt: the matrix TRANSPOSED in LDS, Mt[n][k] (leading dim ld = 4 mod 32 words, so that the 16-byte reads are conflict-free): the A
// operands of the four MFMA steps x' = 0..3 of a chunk are then one 16-byte read  Mt[col0 + r][16 j + 4 q .. + 3].   p[j]: this lane's
// chunk registers.
#ifndef TILE_NO_MFMA
#define TILE_NO_MFMA 0         // development builds (timing only): 1 = the exact-fp32 mat-vecs skip the matrix pipe and the LDS reads.  Set for
#endif                         // the whole build it reaches every family that includes this header, the generalised kernels too.
#ifndef TILE_MMT_BF16
#define TILE_MMT_BF16 1        // the bf16 instantiations run their mat-vecs on the bf16 matrix pipe in split form (mmT_split); 0 (development builds): exact-fp32 MFMA everywhere
#endif
// The same product on the bf16 matrix pipe with fp32-class accuracy: both operands split into two bf16 planes, hi = bf16(v) and
// lo = bf16(v - hi), and  hi.hi + hi.lo + lo.hi  accumulated in fp32 (the dropped lo.lo term is 2^-16 of a product; measured error of
// a mat-vec ~4e-6 relative).  One v_mfma_f32_16x16x32_bf16 covers TWO 16-entry chunks: a lane's eight contraction entries are its
// four of chunk j and its four of chunk j + 1 -- the same permutation of the contraction index for the A operand (two 16-byte LDS
// reads, as before) and the B operand (the lane's own registers), so nothing moves between lanes and the result lands in the
// layout of the fp32 form.  An odd last chunk is padded with zeros.  Three of these instructions per pair of chunks instead of eight
// v_mfma_f32_16x16x4_f32: the cfg-2 step 5.12 -> 5.05 ms (same-box A/B, round 4).
// WHY (round 4): v_mfma_f32_16x16x4_f32 returned wrong sums in these kernels -- one 16-token tile in ~10^3, off by ~1 % -- whenever a
// bf16 GEMM of the engine ran on the same compute units from another stream (AdapterPair's two-stream mode; never alone on the
// GPU, never with the mat-vecs on the vector ALU: tests/dev/race_buffers.py, scripts/mfma_probe.hip).  The bf16
// matrix instructions next to the same neighbours repeat bit for bit.
__device__ __forceinline__ void split8(const float4& v0, const float4& v1, bf16x8& hi, bf16x8& lo) {
  const float f[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const __bf16 h = (__bf16)f[i];
    hi[i] = h;
    lo[i] = (__bf16)(f[i] - (float)h);
  }
}
template <int NJ>
__device__ __forceinline__ f32x4 mmT_split(const float* Mt, int ld, int col0, const float4* p, int r, int q) {
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  const float* mp = Mt + (col0 + r) * ld + 4 * q;
#pragma unroll
  for (int j = 0; j < NJ; j += 2) {
    const float4 a0 = *(const float4*)(mp + 16 * j);
    const float4 a1 = (j + 1 < NJ) ? *(const float4*)(mp + 16 * (j + 1)) : make_float4(0.f, 0.f, 0.f, 0.f);
    const float4 p1 = (j + 1 < NJ) ? p[j + 1 < NJ ? j + 1 : j] : make_float4(0.f, 0.f, 0.f, 0.f);
    bf16x8 ah, al, ph, pl;
    split8(a0, a1, ah, al);
    split8(p[j], p1, ph, pl);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al, ph, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, pl, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, ph, acc, 0, 0, 0);
  }
  return acc;
}
// SPLIT: the bf16 instantiations (sizeof(T) == 2); the fp32 ones keep the exact-fp32 matrix instruction (their neighbours on the
// other stream are fp32 GEMMs: repeatable in every test)
template <int NJ, bool SPLIT>
__device__ __forceinline__ f32x4 mmT(const float* Mt, int ld, int col0, const float4* p, int r, int q) {
#if TILE_MMT_BF16
  if constexpr (SPLIT) return mmT_split<NJ>(Mt, ld, col0, p, r, q);
#endif
#if TILE_NO_MFMA
  return f32x4{p[0].x, p[0].y, p[0].z, p[0].w};
#endif
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  const float* mp = Mt + (col0 + r) * ld + 4 * q;
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const float4 a = *(const float4*)(mp + 16 * j);
#pragma unroll
    for (int x = 0; x < 4; ++x) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(at(a, x), at(p[j], x), acc, 0, 0, 0);
  }
  return acc;
}

// A block's per-frame constants go global -> LDS in BATCHES: U independent loads per thread in flight, then their stores (nthr: the
// block's thread count).  As plain loops (`for (i = tid; i < n; i += threads) lds[f(i)] = g[h(i)]`) the compiler kept them rolled --
// load, s_waitcnt vmcnt(0), store, branch: one memory round trip per element and thread, 24 in a row in kf_pre_lat_bwd's prologue (19 us
// per block, a quarter of the kernel; a timing-only build without the fills: -103 us per cfg-2 step over the six kernels) and 84 in a
// row per block and frame for the latent-token matrices of an 87-token site.  The loads are unconditional (clamped index: a load under
// a condition is waited for on the spot), the stores conditional.  Used for the latent-token matrices (kf_pre_small, kf_pre_lat_bwd:
// 126 -> 101 us and 47 -> 36 us at the two cfg-2 sites) and the staging loops of the generalised kernels; the d x d matrices of
// kf_mid_bwd / kf_post_small / kf_post_small_bwd measured the same either way and keep the plain loops.
template <int U, typename LD, typename ST>
__device__ __forceinline__ void tile_fill(int n, int nthr, LD&& ld, ST&& st) {
  for (int i0 = threadIdx.x; i0 < n; i0 += U * nthr) {
    float v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) v[u] = ld(min(i0 + u * nthr, n - 1));
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (i0 + u * nthr < n) st(i0 + u * nthr, v[u]);
  }
}

}  // namespace
