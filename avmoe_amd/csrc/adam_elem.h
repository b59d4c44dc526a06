// The Adam element update, written ONCE for kk_adam (train_kernels.hip: one flat range per launch, scalars from the host) and kk_opt_adam
// (opt_kernels.hip: every range of the optimizer in one launch, scalars from the device state block; there also the weight average).
// The fused multiply-adds are spelled out and contraction is switched off around them: left to itself the compiler fuses
// `b1 * m + (1 - b1) * g` one way in a 16-byte body and another way in a scalar tail loop, and two kernels that serve the same element
// through different paths (the plain path's merged ranges run over alignment padding, the table's ranges end at the parameter) would
// differ in the last bit.  The form below is the one kk_adam's 16-byte body has always compiled to, so the plain path computes what it
// did, and both paths agree bit for bit on equal inputs (tests/test_flat_adam_device_gpu.py holds them to that).
#pragma once
#include <hip/hip_runtime.h>

namespace avmoe {

// DECOUPLED = false: torch.optim.Adam (weight decay joins the gradient).  true: torch.optim.AdamW (p *= 1 - lr * wd first, no wd term).
template <bool DECOUPLED>
__device__ __forceinline__ void adam_elem(float& p, float& m, float& v, float g, float lr, float b1, float b2, float eps, float wd, float bc1,
                                          float bc2_sqrt, float gscale) {
#pragma clang fp contract(off)
  float gr;
  if constexpr (DECOUPLED) {
    p *= 1.f - lr * wd;
    gr = g * gscale;
  } else {
    gr = __builtin_fmaf(gscale, g, wd * p);
  }
  m = __builtin_fmaf(b1, m, (1.f - b1) * gr);
  v = __builtin_fmaf(b2, v, ((1.f - b2) * gr) * gr);
  p -= ((lr / bc1) * m) / (sqrtf(v) / bc2_sqrt + eps);
}

// One step of an exponential moving average, written ONCE for the parameter averages (ema_elem below, inside kk_opt_adam) and the buffer
// averages (kk_opt_ema_buffers): -> d * avg + (1 - d) * x.  (1 - d) and the product are rounded, then one fused multiply-add; contraction
// is off so that no caller's surroundings decide how it fuses.
__device__ __forceinline__ float ema_next(float avg, float x, float d) {
#pragma clang fp contract(off)
  return __builtin_fmaf(d, avg, (1.f - d) * x);
}

// The weight average of one element (include/avmoe.h, AVMOE_OPT_EMA): ema = d * ema + (1 - d) * p with the parameter's NEW value.  Spelled
// like the moments above, for the same reason: the 16-byte body and the scalar tail must round alike.
__device__ __forceinline__ void ema_elem(float& e, float p, float d) { e = ema_next(e, p, d); }

// Sharpness-aware minimization (include/avmoe.h, avmoe_opt_sam_perturb): the perturbed value p + e of one element, written ONCE for the
// 16-byte body and the scalar tail of kk_opt_sam_perturb.  e = scale * (g * gscale), ADAPTIVE: e = (scale * (p * p)) * (g * gscale) --
// every product rounded to fp32 in this order, contraction off, then one addition: at most four roundings in e and one in the sum.
// e == 0 (a zero gradient, scale == 0) returns p itself, so that a signed zero keeps its bits too.
template <bool ADAPTIVE>
__device__ __forceinline__ float sam_elem(float p, float g, float gscale, float scale) {
#pragma clang fp contract(off)
  const float gr = g * gscale;
  float e;
  if constexpr (ADAPTIVE) e = (scale * (p * p)) * gr;
  else e = scale * gr;
  return e == 0.f ? p : p + e;
}

// Layer-wise trust ratios (include/avmoe.h, avmoe_opt_lamb_step).  The moments of one element, by adam_elem's expressions in adam_elem's
// spelling -- the gradient with grad_scale * clip factor (coupled decay: and wd * p), then the two fused multiply-adds -- so that a run
// with the trust ratio keeps the moments Adam gets from the same gradients, bit for bit.  p is only read.
template <bool DECOUPLED>
__device__ __forceinline__ void lamb_moments(float p, float& m, float& v, float g, float b1, float b2, float wd, float gscale) {
#pragma clang fp contract(off)
  float gr;
  if constexpr (DECOUPLED) gr = g * gscale;
  else gr = __builtin_fmaf(gscale, g, wd * p);
  m = __builtin_fmaf(b1, m, (1.f - b1) * gr);
  v = __builtin_fmaf(b2, v, ((1.f - b2) * gr) * gr);
}

// The update direction u of one element from its STORED moments, written ONCE for the kernel that norms it (kk_opt_lamb_moments) and the
// one that applies it (kk_opt_lamb_apply): both call this on the same fp32 values, so the u that is normed and the u that is applied have
// the same bits.  u = (m / bc1) / (sqrt(v) / bc2_sqrt + eps), DECOUPLED (the paper's LAMB): + wd * p.  Every operation is rounded to
// fp32 in this order, contraction off: five roundings (m / bc1, the root, / bc2_sqrt, + eps, the quotient), seven with the decay term
// and its addition.  This is another order of operations than adam_elem's ((lr / bc1) * m) / (...): the update is NOT Adam's bits.
template <bool DECOUPLED>
__device__ __forceinline__ float lamb_dir(float p, float m, float v, float wd, float bc1, float bc2_sqrt, float eps) {
#pragma clang fp contract(off)
  const float u = (m / bc1) / (sqrtf(v) / bc2_sqrt + eps);
  if constexpr (DECOUPLED) return u + wd * p;
  else return u;
}

// p - step * u with step = (lr * lr_factor) * ratio of the element's range: the product and the difference are rounded, contraction off,
// so the 16-byte body and the scalar tail round alike
__device__ __forceinline__ float lamb_next(float p, float u, float step) {
#pragma clang fp contract(off)
  return p - step * u;
}

// elements [i0, min(i0 + 4, n)) of one range, the applying half of a step with trust ratios: reads p (HOLD: from `hold`), m and v, forms
// u with lamb_dir and writes p; EMA: the same thread advances the shadow from the new p, as adam_quad does.  m and v are only read.
template <bool DECOUPLED, bool EMA, bool HOLD>
__device__ __forceinline__ void lamb_quad(float* __restrict__ p, const float* __restrict__ m, const float* __restrict__ v, long i0, long n, float step,
                                          float eps, float wd, float bc1, float bc2_sqrt, float* __restrict__ ema, float d,
                                          const float* __restrict__ hold) {
  if (i0 + 3 < n) {
    float4 pp;
    const float4 mm = *(const float4*)(m + i0), vv = *(const float4*)(v + i0);
    if constexpr (HOLD) pp = *(const float4*)(hold + i0);
    else pp = *(float4*)(p + i0);
    float* P = (float*)&pp; const float* M = (const float*)&mm; const float* V = (const float*)&vv;
#pragma unroll
    for (int k = 0; k < 4; ++k) P[k] = lamb_next(P[k], lamb_dir<DECOUPLED>(P[k], M[k], V[k], wd, bc1, bc2_sqrt, eps), step);
    *(float4*)(p + i0) = pp;
    if constexpr (EMA) {
      float4 ee = *(float4*)(ema + i0);
      float* E = (float*)&ee;
#pragma unroll
      for (int k = 0; k < 4; ++k) ema_elem(E[k], P[k], d);
      *(float4*)(ema + i0) = ee;
    }
  } else {
    for (long i = i0; i < n; ++i) {
      float pv;
      if constexpr (HOLD) pv = hold[i];
      else pv = p[i];
      pv = lamb_next(pv, lamb_dir<DECOUPLED>(pv, m[i], v[i], wd, bc1, bc2_sqrt, eps), step);
      p[i] = pv;
      if constexpr (EMA) ema_elem(ema[i], pv, d);
    }
  }
}

// Prodigy learning-rate estimation (include/avmoe.h, avmoe_opt_prodigy_step).  What a thread reads once for all its elements: the
// estimate d of this step, step = (lr * lr_factor) * d of its range, c = step * (d / d0) (safeguard_warmup: d * (d / d0)), deps = d * eps,
// every product rounded to fp32 in this order by the kernel, and the constants of the run.
struct ProdigyScal { float d, step, c, deps, b1, b2, beta3, wd, gscale; };

// One element of a step, written ONCE for the 16-byte body and the scalar tail of kk_opt_prodigy_update (prodigy_quad below).  Every
// operation is rounded to fp32 in the order written, contraction off:
//     gr = fma(gscale, g, wd * p)          (DECOUPLED: gr = g * gscale, and p <- p * (1 - step * wd) before the Adam term)
//     dg = d * gr ;  cg = c * gr
//     m  = fma(b1, m, (1 - b1) * dg) ;  v = fma(b2, v, ((1 - b2) * dg) * dg)      -- adam_elem's spelling on d * gr: with d == 1 its bits
//     s  = fma(beta3, s, cg)
//     dot += (double)cg * ((double)x0 - (double)p)   with p as it was BEFORE the step ;   l1 += (double)|s|   with the new s
//     den = sqrt(v) + deps ;  p = p - (step * m) / den
// (d * gr)^2 may underflow fp32: v then takes what IEEE gradual underflow leaves, possibly 0.  Where den is not > 0 -- v == 0 and
// d * eps == 0, or a NaN -- the quotient is not formed and the Adam term of this element is dropped: p keeps its value (DECOUPLED: its
// decayed value), m, v, s and both sums advance as above.
template <bool DECOUPLED>
__device__ __forceinline__ void prodigy_elem(float& p, float& m, float& v, float& s, float g, float x0, const ProdigyScal& k, double& dot, double& l1) {
#pragma clang fp contract(off)
  float gr;
  if constexpr (DECOUPLED) gr = g * k.gscale;
  else gr = __builtin_fmaf(k.gscale, g, k.wd * p);
  const float dg = k.d * gr, cg = k.c * gr;
  dot += (double)cg * ((double)x0 - (double)p);
  if constexpr (DECOUPLED) p *= 1.f - k.step * k.wd;
  m = __builtin_fmaf(k.b1, m, (1.f - k.b1) * dg);
  v = __builtin_fmaf(k.b2, v, ((1.f - k.b2) * dg) * dg);
  s = __builtin_fmaf(k.beta3, s, cg);
  l1 += (double)fabsf(s);
  const float den = sqrtf(v) + k.deps;
  if (den > 0.f) p -= (k.step * m) / den;
}

// elements [i0, min(i0 + 4, n)) of one range (i0 < n): reads p (HOLD: from `hold`), g, m, v, s and x0, writes p, m, v and s and adds the
// elements' terms to `dot` and `l1`; EMA: the same thread advances the shadow from the new p with decay `decay`, as adam_quad does.
// Four elements left: 16-byte loads, all issued before the first store.  At the tail: four loads per stream all the same, unconditional
// at an index clamped into the range and issued before the first store; only the arithmetic and the stores are masked.
template <bool DECOUPLED, bool EMA, bool HOLD>
__device__ __forceinline__ void prodigy_quad(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                             float* __restrict__ s, const float* __restrict__ x0, long i0, long n, const ProdigyScal& k,
                                             float* __restrict__ ema, float decay, const float* __restrict__ hold, double& dot, double& l1) {
  const float* __restrict__ src = p;
  if constexpr (HOLD) src = hold;
  if (i0 + 3 < n) {
    float4 pp = *(const float4*)(src + i0), mm = *(float4*)(m + i0), vv = *(float4*)(v + i0), ss = *(float4*)(s + i0), ee;
    const float4 gg = *(const float4*)(g + i0), xx = *(const float4*)(x0 + i0);
    if constexpr (EMA) ee = *(float4*)(ema + i0);
    float* P = (float*)&pp; float* M = (float*)&mm; float* V = (float*)&vv; float* S = (float*)&ss; float* E = (float*)&ee;
    const float* G = (const float*)&gg; const float* X = (const float*)&xx;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      prodigy_elem<DECOUPLED>(P[j], M[j], V[j], S[j], G[j], X[j], k, dot, l1);
      if constexpr (EMA) ema_elem(E[j], P[j], decay);
    }
    *(float4*)(p + i0) = pp; *(float4*)(m + i0) = mm; *(float4*)(v + i0) = vv; *(float4*)(s + i0) = ss;
    if constexpr (EMA) *(float4*)(ema + i0) = ee;
  } else {
    const long last = n - 1;
    long idx[4];
    float P[4], G[4], M[4], V[4], S[4], X[4], E[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      idx[j] = i0 + j < last ? i0 + j : last;
      P[j] = src[idx[j]]; G[j] = g[idx[j]]; M[j] = m[idx[j]]; V[j] = v[idx[j]]; S[j] = s[idx[j]]; X[j] = x0[idx[j]];
      if constexpr (EMA) E[j] = ema[idx[j]];
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (i0 + j <= last) {
        prodigy_elem<DECOUPLED>(P[j], M[j], V[j], S[j], G[j], X[j], k, dot, l1);
        p[idx[j]] = P[j]; m[idx[j]] = M[j]; v[idx[j]] = V[j]; s[idx[j]] = S[j];
        if constexpr (EMA) { ema_elem(E[j], P[j], decay); ema[idx[j]] = E[j]; }
      }
    }
  }
}

// elements [i0, min(i0 + 4, n)) of one range: 16-byte loads and stores where four elements are left, element by element at the tail.
// EMA: the same thread also advances the shadow value of each element from the parameter value it still holds in a register, with decay d
// (without it `ema` and `d` are not read).
// HOLD: the element's parameter value is READ from `hold` (the unperturbed parameters avmoe_opt_sam_perturb has kept) and the result is
// written to `p`, which is only written (without it `hold` is not read).  The arithmetic is the same calls on the same values.
template <bool DECOUPLED, bool EMA, bool HOLD = false>
__device__ __forceinline__ void adam_quad(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v, long i0,
                                          long n, float lr, float b1, float b2, float eps, float wd, float bc1, float bc2_sqrt, float gscale,
                                          float* __restrict__ ema, float d, const float* __restrict__ hold = nullptr) {
  if (i0 + 3 < n) {
    float4 pp, mm = *(float4*)(m + i0), vv = *(float4*)(v + i0);
    if constexpr (HOLD) pp = *(const float4*)(hold + i0);
    else pp = *(float4*)(p + i0);
    const float4 gg = *(const float4*)(g + i0);
    float* P = (float*)&pp; float* M = (float*)&mm; float* V = (float*)&vv; const float* G = (const float*)&gg;
#pragma unroll
    for (int k = 0; k < 4; ++k) adam_elem<DECOUPLED>(P[k], M[k], V[k], G[k], lr, b1, b2, eps, wd, bc1, bc2_sqrt, gscale);
    *(float4*)(p + i0) = pp; *(float4*)(m + i0) = mm; *(float4*)(v + i0) = vv;
    if constexpr (EMA) {
      float4 ee = *(float4*)(ema + i0);
      float* E = (float*)&ee;
#pragma unroll
      for (int k = 0; k < 4; ++k) ema_elem(E[k], P[k], d);
      *(float4*)(ema + i0) = ee;
    }
  } else {
    for (long i = i0; i < n; ++i) {
      if constexpr (HOLD) {
        float pv = hold[i];
        adam_elem<DECOUPLED>(pv, m[i], v[i], g[i], lr, b1, b2, eps, wd, bc1, bc2_sqrt, gscale);
        p[i] = pv;
        if constexpr (EMA) ema_elem(ema[i], pv, d);
      } else {
        adam_elem<DECOUPLED>(p[i], m[i], v[i], g[i], lr, b1, b2, eps, wd, bc1, bc2_sqrt, gscale);
        if constexpr (EMA) ema_elem(ema[i], p[i], d);
      }
    }
  }
}

// Schedule-free AdamW (include/avmoe.h, avmoe_opt_sf_step).  What a thread reads once for all its elements: step = lr * lr_factor of its
// range, d = 1 - c of this step from the 32-byte block, and the constants of the run.
struct SfScal { float step, d, b1, b2, eps, wd, bc2_sqrt, gscale; };

// One element of a step, written ONCE for the 16-byte body and the scalar tail of kk_opt_sf_update (sf_quad below).  y is the parameter
// as the sites see it (the gradient was taken there), z the base sequence (it lives in exp_avg), x the average (the shadow).  Every
// operation is rounded to fp32 in the order written, contraction off:
//     gr = fma(gscale, g, wd * y)          (DECOUPLED: gr = g * gscale)
//     v  = fma(b2, v, ((1 - b2) * gr) * gr)                                       -- adam_elem's spelling: Adam's bits for v from the same gr
//     u  = gr / (sqrt(v) / bc2_sqrt + eps)                                        (DECOUPLED: u = u + wd * y)
//     z  = z - step * u
//     x  = fma(d, x, (1 - d) * z)                                                 -- ema_next: the average's own expression
//     y  = fma(b1, x, (1 - b1) * z)
// There is no momentum buffer and no first-moment bias correction: b1 is the interpolation.  d == 0 gives x == z and b1 == 0 gives
// y == z, bit for bit.
template <bool DECOUPLED>
__device__ __forceinline__ void sf_elem(float& y, float& z, float& v, float& x, float g, const SfScal& k) {
#pragma clang fp contract(off)
  float gr;
  if constexpr (DECOUPLED) gr = g * k.gscale;
  else gr = __builtin_fmaf(k.gscale, g, k.wd * y);
  v = __builtin_fmaf(k.b2, v, ((1.f - k.b2) * gr) * gr);
  float u = gr / (sqrtf(v) / k.bc2_sqrt + k.eps);
  if constexpr (DECOUPLED) u = u + k.wd * y;
  z = z - k.step * u;
  x = ema_next(x, z, k.d);
  y = __builtin_fmaf(k.b1, x, (1.f - k.b1) * z);
}

// elements [i0, min(i0 + 4, n)) of one range (i0 < n): reads y (HOLD: from `hold`, else from p), g, z, v and x, writes p, z, v and x --
// five streams in, four out.  Four elements left: 16-byte loads, all issued before the first store.  At the tail: element by element.
template <bool DECOUPLED, bool HOLD>
__device__ __forceinline__ void sf_quad(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ z, float* __restrict__ v,
                                        float* __restrict__ x, long i0, long n, const SfScal& k, const float* __restrict__ hold) {
  if (i0 + 3 < n) {
    float4 yy, zz = *(float4*)(z + i0), vv = *(float4*)(v + i0), xx = *(float4*)(x + i0);
    if constexpr (HOLD) yy = *(const float4*)(hold + i0);
    else yy = *(float4*)(p + i0);
    const float4 gg = *(const float4*)(g + i0);
    float* Y = (float*)&yy; float* Z = (float*)&zz; float* V = (float*)&vv; float* X = (float*)&xx; const float* G = (const float*)&gg;
#pragma unroll
    for (int j = 0; j < 4; ++j) sf_elem<DECOUPLED>(Y[j], Z[j], V[j], X[j], G[j], k);
    *(float4*)(p + i0) = yy; *(float4*)(z + i0) = zz; *(float4*)(v + i0) = vv; *(float4*)(x + i0) = xx;
  } else {
    for (long i = i0; i < n; ++i) {
      float yv, zv = z[i], vv = v[i], xv = x[i];
      if constexpr (HOLD) yv = hold[i];
      else yv = p[i];
      sf_elem<DECOUPLED>(yv, zv, vv, xv, g[i], k);
      p[i] = yv; z[i] = zv; v[i] = vv; x[i] = xv;
    }
  }
}

// Orthogonalised momentum (include/avmoe.h, avmoe_opt_muon_step): the parameter's new value from the finished direction O, written ONCE for
// kk_opt_muon_ns (opt_muon.hip) and kk_opt_muon_large_apply (opt_muon_large.hip): decay (decoupled), then p - step * O with step = lr * s; as lamb_next
__device__ __forceinline__ float muon_next(float p, float o, float lr, float wd, float step, bool decoupled) {
#pragma clang fp contract(off)
  if (decoupled) p *= 1.f - lr * wd;
  return p - step * o;
}

}  // namespace avmoe
