// Backward of one site when `out` gets no gradient: only a loss on the routing probabilities, the load-balancing loss and / or the
// router auxiliary losses (z-loss, balance loss: avmoe_moe_backward_aux) was differentiated.  Then every expert product, the Gram products and the token-space passes of the full backward would produce exact
// zeros; only the router and the mean / remap chain carry gradient.  Per frame s, with [g1 | g2] = d rin after the router backward
// (g1: the mean of X, g2: the mean of Yf = fc(conv_adapter(Y)); C each):
//   dX[s,n,:]  = g1[s] / N
//   u[s]       = Wf^T g2[s] / N
//   dY[s,m,:]  = N wbar[m] u[s]                          wbar = mean_n Wc (saved by the forward)
//   ybar[s]    = sum_m wbar[m] Y[s,m,:] + mean(bc)
//   dWf        = sum_s g2[s] (x) ybar[s]      dbf = sum_s g2[s]
//   dWc[n,m]   = sum_s <u[s], Y[s,m,:]>       dbc[n] = sum_s sum u[s]     (the same for every n)
// and every expert parameter gradient is 0.  Memory-bound: one pass over Y (read once, dY written in the same pass), one broadcast
// write of dX, small reductions.
// The multiplier on the mixture weights (avmoe_moe_backward_reg: mix_scale) scales the gradient of the mixture weights alone, and this
// path has none (dp is zero-filled below): it does not take the tensor.  After a forward with a multiplier the router backward still
// finds the softmax in psm, because that forward wrote the top-k mode word (fwd_kernels.hip: k_router).
#include "kernels.h"
#include "moe_run.h"
#include "device_utils.h"
#include "prof.h"
#include "gemm.h"
#include <algorithm>

namespace avmoe {

namespace {

constexpr int RO_FR = 8;          // frames per block of the u product

// u[s][k] = (1/N) sum_c g2[s][c] Wf[c][k]: block (64 columns k, RO_FR frames); the four waves take every fourth channel of each
// 256-channel slab of g2 (staged in LDS), their partial sums are added in a fixed order
__global__ void __launch_bounds__(256) kk_ro_u(const float* drin, const float* Wf, float* u, int S, int C, int Cy, float invN) {
  __shared__ float s_g[RO_FR][256];
  __shared__ float s_p[4][RO_FR][64];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int k = blockIdx.x * 64 + lane, s0 = blockIdx.y * RO_FR;
  const long C2 = 2L * C;
  float acc[RO_FR];
#pragma unroll
  for (int f = 0; f < RO_FR; ++f) acc[f] = 0.f;
  for (int c0 = 0; c0 < C; c0 += 256) {
    __syncthreads();
    for (int i = threadIdx.x; i < RO_FR * 256; i += 256) {
      const int f = i >> 8, c = c0 + (i & 255);
      s_g[f][i & 255] = (c < C && s0 + f < S) ? drin[(long)(s0 + f) * C2 + C + c] : 0.f;
    }
    __syncthreads();
    if (k < Cy)
      for (int j = wave; j < 256 && c0 + j < C; j += 4) {
        const float w = Wf[(long)(c0 + j) * Cy + k];
#pragma unroll
        for (int f = 0; f < RO_FR; ++f) acc[f] += s_g[f][j] * w;
      }
  }
#pragma unroll
  for (int f = 0; f < RO_FR; ++f) s_p[wave][f][lane] = acc[f];
  __syncthreads();
  for (int i = threadIdx.x; i < RO_FR * 64; i += 256) {
    const int f = i >> 6, l = i & 63, kk = blockIdx.x * 64 + l;
    if (kk < Cy && s0 + f < S) u[(long)(s0 + f) * Cy + kk] = ((s_p[0][f][l] + s_p[1][f][l]) + (s_p[2][f][l] + s_p[3][f][l])) * invN;
  }
}

template <typename T, bool V4>
__device__ __forceinline__ float4 ro_ld4(const T* p, long row, int k, int Cy) {
  if (V4) return k < Cy ? ld4T<T>(p, row + k) : make_float4(0.f, 0.f, 0.f, 0.f);
  return make_float4(k < Cy ? ldT<T>(p, row + k) : 0.f, k + 1 < Cy ? ldT<T>(p, row + k + 1) : 0.f,
                     k + 2 < Cy ? ldT<T>(p, row + k + 2) : 0.f, k + 3 < Cy ? ldT<T>(p, row + k + 3) : 0.f);
}
template <typename T, bool V4>
__device__ __forceinline__ void ro_st4(T* p, long row, int k, int Cy, const float4& v) {
  if (V4) { if (k < Cy) st4T<T>(p, row + k, v); return; }
  if (k < Cy) stT<T>(p, row + k, v.x);
  if (k + 1 < Cy) stT<T>(p, row + k + 1, v.y);
  if (k + 2 < Cy) stT<T>(p, row + k + 2, v.z);
  if (k + 3 < Cy) stT<T>(p, row + k + 3, v.w);
}

// The pass over Y: block (chunk, s) takes rows [chunk * RO_ROWS, + RO_ROWS) of frame s, each wave every fourth row, each lane four
// channels of a 256-channel tile.  Per row: <u[s], Y[s,m,:]> (-> wcp[s][m]), wbar[m] Y[s,m,:] into the block's ybar partial, and
// dY[s,m,:] = N wbar[m] u[s] (+ dY when accumulating) written in the same pass.
template <typename T, bool V4>
__global__ void __launch_bounds__(256) kk_ro_y(const void* Y_, void* dY_, const float* u, const float* wbar, float* ybp, float* wcp,
                                               float* usum, int M, int Cy, int nch, float fN, int acc) {
  const T* Y = (const T*)Y_;
  T* dY = (T*)dY_;
  __shared__ float s_dot[RO_ROWS];
  __shared__ float4 s_acc[4][64];
  const int ch = blockIdx.x, s = blockIdx.y;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int m0 = ch * RO_ROWS, m1 = min(M, m0 + RO_ROWS);
  if (threadIdx.x < RO_ROWS) s_dot[threadIdx.x] = 0.f;
  __syncthreads();
  const float* us = u + (long)s * Cy;
  float ut = 0.f;                                          // sum of u[s] (chunk 0's wave 0): for dbc
  for (int k0 = 0; k0 < Cy; k0 += 256) {
    const int k = k0 + 4 * lane;
    const float4 uv = make_float4(k < Cy ? us[k] : 0.f, k + 1 < Cy ? us[k + 1] : 0.f, k + 2 < Cy ? us[k + 2] : 0.f, k + 3 < Cy ? us[k + 3] : 0.f);
    if (ch == 0 && wave == 0) ut += wave_sum((uv.x + uv.y) + (uv.z + uv.w));
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int m = m0 + wave; m < m1; m += 4) {
      const long row = ((long)s * M + m) * Cy;
      const float w = wbar[m];
      const float4 y = ro_ld4<T, V4>(Y, row, k, Cy);
      const float p = wave_sum(uv.x * y.x + uv.y * y.y + uv.z * y.z + uv.w * y.w);
      if (lane == 0) s_dot[m - m0] += p;                  // (row m belongs to this wave alone)
      a.x += w * y.x; a.y += w * y.y; a.z += w * y.z; a.w += w * y.w;
      const float f = fN * w;
      float4 o = make_float4(f * uv.x, f * uv.y, f * uv.z, f * uv.w);
      if (acc) {
        const float4 q = ro_ld4<T, V4>(dY, row, k, Cy);
        o.x += q.x; o.y += q.y; o.z += q.z; o.w += q.w;
      }
      ro_st4<T, V4>(dY, row, k, Cy, o);
    }
    s_acc[wave][lane] = a;
    __syncthreads();
    if (wave == 0) {
      const float4 b0 = s_acc[0][lane], b1 = s_acc[1][lane], b2 = s_acc[2][lane], b3 = s_acc[3][lane];
      float* dst = ybp + ((long)s * nch + ch) * Cy;
      const float v[4] = {(b0.x + b1.x) + (b2.x + b3.x), (b0.y + b1.y) + (b2.y + b3.y), (b0.z + b1.z) + (b2.z + b3.z), (b0.w + b1.w) + (b2.w + b3.w)};
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (k + j < Cy) dst[k + j] = v[j];
    }
    __syncthreads();
  }
  if (threadIdx.x < m1 - m0) wcp[(long)s * M + m0 + threadIdx.x] = s_dot[threadIdx.x];
  if (ch == 0 && threadIdx.x == 0) usum[s] = ut;
}

// ybar[s][k] = sum over the chunks of the partials + mean(bc)
__global__ void __launch_bounds__(256) kk_ro_ybar(const float* ybp, const float* scal, float* ybar, int S, int Cy, int nch) {
  const float mbc = scal[0];
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < (long)S * Cy; i += (long)gridDim.x * 256) {
    const long s = i / Cy, k = i % Cy;
    float a = 0.f;
    for (int c = 0; c < nch; ++c) a += ybp[(s * nch + c) * Cy + k];
    ybar[i] = a + mbc;
  }
}

// dbf[c] = sum_s g2[s][c]
__global__ void __launch_bounds__(256) kk_ro_bf(const float* drin, float* gbf, int S, int C) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  float a = 0.f;
  for (int s = 0; s < S; ++s) a += drin[2L * C * s + C + c];
  gbf[c] = a;
}

// dWc[n][m] = sum_s wcp[s][m] for every n: blocks of 64 columns x 64 rows (the column sums formed per block, four frame streams
// combined in a fixed order); the last block: dbc[n] = sum over the frames of usum (sum of u[s]), for every n
__global__ void __launch_bounds__(256) kk_ro_wc(const float* wcp, const float* usum, float* gWc, float* gbc, int S, int N, int M, int nbm, int nbn) {
  __shared__ float red[4][64];
  __shared__ float tot[4];
  const int b = blockIdx.x;
  if (b < nbm * nbn) {
    const int bm = b % nbm, bn = b / nbm;
    const int l = threadIdx.x & 63, q = threadIdx.x >> 6, m = bm * 64 + l;
    float a = 0.f;
    if (m < M)
      for (int s = q; s < S; s += 4) a += wcp[(long)s * M + m];
    red[q][l] = a;
    __syncthreads();
    const float v = (red[0][l] + red[1][l]) + (red[2][l] + red[3][l]);
    if (m < M)
      for (int n = bn * 64 + q; n < min(N, bn * 64 + 64); n += 4) gWc[(long)n * M + m] = v;
    return;
  }
  float a = 0.f;
  for (int i = threadIdx.x; i < S; i += 256) a += usum[i];
  const float t = block_sum256(a, tot);
  for (int n = threadIdx.x; n < N; n += 256) gbc[n] = t;
}

// dX[s,n,:] = g1[s] / N (+ dX when accumulating); C is a multiple of 8
template <typename T>
__global__ void __launch_bounds__(256) kk_ro_dx(const float* drin, void* dX_, int S, int N, int C, float invN, int acc) {
  T* dX = (T*)dX_;
  const long n4 = (long)S * N * C / 4, C2 = 2L * C;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
    const long e = 4 * i, s = e / ((long)N * C), k = e % C;
    const float4 g = *(const float4*)(drin + s * C2 + k);
    float4 o = make_float4(g.x * invN, g.y * invN, g.z * invN, g.w * invN);
    if (acc) {
      const float4 q = ld4T<T>(dX, e);
      o.x += q.x; o.y += q.y; o.z += q.z; o.w += q.w;
    }
    st4T<T>(dX, e, o);
  }
}

// zero-fill of up to RO_ZMAX parameter gradients in one launch: blockIdx.x picks the tensor, blockIdx.y strides over it
constexpr int RO_ZMAX = 64;
struct ZeroList { float* p[RO_ZMAX]; long n[RO_ZMAX]; };
__global__ void __launch_bounds__(256) kk_ro_zero(ZeroList z) {
  float* p = z.p[blockIdx.x];
  const long n = z.n[blockIdx.x];
  for (long i = (long)blockIdx.y * 256 + threadIdx.x; i < n; i += (long)gridDim.y * 256) p[i] = 0.f;
}

}  // namespace

int k_zero_bytes(void* ptr, size_t bytes, hipStream_t st);      // bwd_kernels.hip

int moe_backward_router_only(const Plan& pl, const void* Y, const avmoe_moe_ptrs& prm, const float* dprobs, const float* lb_grad,
                             char* sv, char* sc, void* dX, void* dY, const avmoe_moe_ptrs& grads, hipStream_t st, const float* aux_grad) {
  const Dims& d = pl.d;
  // the mixture's share of d probs is 0: the router backward sees only dprobs, the load-balancing term and the auxiliary losses
  AVMOE_TRY(k_zero_bytes(sc + pl.o_dp, (size_t)d.S * d.E * sizeof(float), st));      // (a kernel, not hipMemsetAsync: moe_backward.cpp has the reason)
  AVMOE_TRY(k_router_bwd(pl, sv, sc, prm, grads, lb_grad, dprobs, st, aux_grad, nullptr));
  const float* drin = (const float*)(sc + pl.o_rbw) + (long)d.S * 128;
  const int nch = ro_chunks(d);
  float* u = (float*)(sc + pl.o_ro);
  float* ybar = u + (long)d.S * d.Cy;
  float* ybp = ybar + (long)d.S * d.Cy;
  float* wcp = ybp + (long)d.S * nch * d.Cy;
  float* usum = wcp + (long)d.S * d.M;
  const float fN = (float)d.N, invN = 1.f / (float)d.N;
  {
    ProfScope ps("k_ro_u", (double)d.C * d.Cy * 4.0, 2.0 * d.S * d.C * (double)d.Cy, st);
    hipLaunchKernelGGL(kk_ro_u, dim3((unsigned)cdiv(d.Cy, 64), (unsigned)cdiv(d.S, RO_FR)), dim3(256), 0, st, drin, (const float*)prm.fc_w, u,
                       d.S, d.C, d.Cy, invN);
  }
  {
    const double ybytes = (double)d.S * d.M * d.Cy * d.esz;
    ProfScope ps("k_ro_y", (long)d.S * d.M, ybytes * (d.acc_dy ? 3.0 : 2.0), 4.0 * d.S * d.M * (double)d.Cy, st);
    const dim3 grid((unsigned)nch, (unsigned)d.S);
    const bool v4 = d.Cy % 4 == 0;
    const float* wb = (const float*)(sv + pl.o_wbar);
    if (d.bf16) {
      if (v4) hipLaunchKernelGGL((kk_ro_y<__bf16, true>), grid, dim3(256), 0, st, Y, dY, u, wb, ybp, wcp, usum, d.M, d.Cy, nch, fN, d.acc_dy);
      else hipLaunchKernelGGL((kk_ro_y<__bf16, false>), grid, dim3(256), 0, st, Y, dY, u, wb, ybp, wcp, usum, d.M, d.Cy, nch, fN, d.acc_dy);
    } else {
      if (v4) hipLaunchKernelGGL((kk_ro_y<float, true>), grid, dim3(256), 0, st, Y, dY, u, wb, ybp, wcp, usum, d.M, d.Cy, nch, fN, d.acc_dy);
      else hipLaunchKernelGGL((kk_ro_y<float, false>), grid, dim3(256), 0, st, Y, dY, u, wb, ybp, wcp, usum, d.M, d.Cy, nch, fN, d.acc_dy);
    }
  }
  {
    ProfScope ps("k_ro_reduce", 0.0, 0.0, st);
    hipLaunchKernelGGL(kk_ro_ybar, dim3(grid1d((long)d.S * d.Cy, 1024)), dim3(256), 0, st, (const float*)ybp, (const float*)(sv + pl.o_scal),
                       ybar, d.S, d.Cy, nch);
    if (grads.fc_b) hipLaunchKernelGGL(kk_ro_bf, dim3((unsigned)cdiv(d.C, 256)), dim3(256), 0, st, drin, grads.fc_b, d.S, d.C);
  }
  if (grads.fc_w) {   // dWf = g2^T ybar  (fp32 engine GEMM over the frames; the split-K slabs are free again after the router backward)
    GemmArgs g;
    g.dtype = GEMM_F32; g.out_dtype = GEMM_F32;
    g.A = drin + d.C; g.B = ybar; g.C = grads.fc_w;
    g.M = d.C; g.N = d.Cy; g.K = d.S; g.a_layout = g.b_layout = MN_MAJOR; g.lda = 2L * d.C; g.ldb = d.Cy; g.sCi = d.Cy;
    g.tile = 64; g.slabs = (float*)(sc + pl.o_slabs); g.ksplit = choose_ksplit(g, slab_floats(d));
    AVMOE_TRY(launch_gemm(g, st));
  }
  {
    ProfScope ps("k_ro_reduce", 0.0, 0.0, st);
    const int nbm = cdiv(d.M, 64), nbn = cdiv(d.N, 64);
    if (grads.conv_w || grads.conv_b) {
      // (a missing pointer of the two only skips its own job)
      const int nb = (grads.conv_w ? nbm * nbn : 0) + (grads.conv_b ? 1 : 0);
      hipLaunchKernelGGL(kk_ro_wc, dim3((unsigned)nb), dim3(256), 0, st, (const float*)wcp, (const float*)usum, grads.conv_w, grads.conv_b, d.S,
                         d.N, d.M, grads.conv_w ? nbm : 0, grads.conv_w ? nbn : 0);
    }
  }
  {
    ProfScope ps("k_ro_dx", (long)d.NT, (double)d.NT * d.C * d.esz * (d.acc_dx ? 2.0 : 1.0), 0.0, st);
    const unsigned g = grid1d((long)d.NT * d.C / 4, 8192);
    if (d.bf16) hipLaunchKernelGGL(kk_ro_dx<__bf16>, dim3(g), dim3(256), 0, st, drin, dX, d.S, d.N, d.C, invN, d.acc_dx);
    else hipLaunchKernelGGL(kk_ro_dx<float>, dim3(g), dim3(256), 0, st, drin, dX, d.S, d.N, d.C, invN, d.acc_dx);
  }
  {   // every expert parameter gradient is exactly 0 (only the parameters the site has: a pointer the full backward would not write is left alone)
    ProfScope ps("k_ro_zero", 0.0, 0.0, st);
    ZeroList z;
    int cnt = 0;
    auto flush = [&]() -> int {
      if (cnt) hipLaunchKernelGGL(kk_ro_zero, dim3((unsigned)cnt, 8), dim3(256), 0, st, z);
      cnt = 0;
      return OK;
    };
    auto add = [&](float* p, long n) { if (!p || n <= 0) return; z.p[cnt] = p; z.n[cnt] = n; if (++cnt == RO_ZMAX) flush(); };
    const long C = d.C;
    const int gr = d.mg ? d.mg : d.g;                      // the parameters' own group count (a merged site runs as one group: moe_plan.cpp)
    for (int e = 0; e < d.E; ++e) {
      const avmoe_expert_ptrs& g = grads.e[e];
      const bool cross = e < d.E_m, v2 = d.self_attn == AVMOE_SELF_ATTN_LATENT_V2, v1 = d.self_attn == AVMOE_SELF_ATTN_MHA_V1;
      if (d.use_gate) add(g.gate, 1);
      if (cross || v2) add(g.my_tokens, (long)d.K * C);
      if (cross || v2 || d.variant == AVMOE_VARIANT_AVVP) add(g.gate_lat, 1);
      add(g.down_w, (long)d.d * (C / gr));
      add(g.up_w, C * (d.d / gr));
      if (d.use_bn) { add(g.bn1_w, d.d); add(g.bn1_b, d.d); add(g.bn2_w, C); add(g.bn2_b, C); }
      if (d.ln_before) { add(g.lnb_w, C); add(g.lnb_b, C); }
      if (d.ln_post) { add(g.lnp_w, C); add(g.lnp_b, C); }
      if (!cross && v1) { add(g.sa_in_w, 3 * C * C); add(g.sa_in_b, 3 * C); add(g.sa_out_w, C * C); add(g.sa_out_b, C); }
    }
    flush();
  }
  AVMOE_CHECK_LAUNCH("router_only_bwd");
  return OK;
}

}  // namespace avmoe
