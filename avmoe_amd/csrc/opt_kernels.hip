// The optimizer with its state on the device (include/avmoe.h, "optimizer with device-side state"): every (param, grad, exp_avg,
// exp_avg_sq) range the optimizer owns is one entry of a table in device memory, and three launches serve a step whatever the number of
// buckets and ranges --
//   kk_opt_sqsum                           sum of (grad * grad_scale)^2 per 1024-element block, in double, into the partial-sum workspace
//   kk_opt_finalize<SCHED, EMA>            one block adds the partial sums in a fixed order and writes the state block: norm, clip factor,
//                                          skip flag, step counters, bias corrections; SCHED: and the learning-rate factor of a per-step
//                                          schedule; EMA: and the decay of the weight average for this step.  Stochastic weight
//                                          averaging is the same two words by another rule (avmoe_opt_swa: the annealed rate under
//                                          SCHED, the uniform average's decay under EMA), a launch-uniform branch and no kernel more
//   kk_opt_adam<DECOUPLED, SCHED, EMA>     the Adam / AdamW update of every range; reads the state block, writes nothing when the step is
//                                          skipped; EMA: the thread that holds an element's new value also advances its average,
//                                          ema = d ema + (1 - d) p, in a shadow buffer per range -- two more 4-byte streams per element
// one more launch per step under AVMOE_OPT_REPORT --
//   kk_opt_range_norms                     one wave per range adds the range's block partial sums in a fixed order and writes the range's
//                                          norm into the report buffer; a range whose norm is not finite lowers the report's
//                                          first_nonfinite with an integer atomicMin (a minimum does not depend on the order)
// and one launch beside the step --
//   kk_opt_swap                            exchanges every range's parameters with their averages (evaluation with the averaged weights,
//                                          and back)
// and, for tensors that cannot move into the flat buckets (BatchNorm running statistics: buffers at their own addresses, possibly only
// 4-byte aligned), a table of {buffer, shadow, n} records of its own with one launch per step and one beside it --
//   kk_opt_ema_buffers                     behind the update: shadow = d shadow + (1 - d) buffer with the state block's d and skip flag
//   kk_opt_swap_buffers                    exchanges every buffer with its shadow, beside kk_opt_swap
// and, for sharpness-aware minimization (include/avmoe.h, avmoe_opt_sam_perturb), three launches after the FIRST backward pass of a step --
//   kk_opt_sqsum (or kk_opt_sqsum_adaptive: of |p| * grad)   the norm pass of the perturbing gradient, into the same partial-sum workspace
//   kk_opt_sam_finalize                    one block adds the partial sums in finalize's order and writes the 16-byte SAM block: norm,
//                                          scale = rho / (norm + 1e-12), nonfinite
//   kk_opt_sam_perturb<ADAPTIVE>           hold = p ; p = p + e for every element of every range, in a hold buffer per range (as the shadows)
// -- and kk_opt_adam<..., HOLD> for the step behind the second backward pass: it reads every p from hold and writes it to param, so the
// unperturbed parameters come back exactly (a copy, not p + e - e); a skipped step writes param = hold and nothing else
// and, for layer-wise trust ratios (LAMB; include/avmoe.h, avmoe_opt_lamb_step), three launches in place of kk_opt_adam --
//   kk_opt_lamb_moments<DECOUPLED, HOLD>   the moments of every element, by adam_elem's expressions, and per 1024-element block the sums
//                                          of u^2 and p^2 in double, u = lamb_dir (adam_elem.h) of the values just stored
//   kk_opt_lamb_ratio                      one wave per range, the walk of kk_opt_range_norms over both sums: ||p||, ||u|| and
//                                          ratio = ||p|| / ||u|| (formed in double, rounded once; 1 for a range that is not adapted or
//                                          has a zero or non-finite norm; clamped where the range has a limit) into the trust report
//   kk_opt_lamb_apply<DECOUPLED, SCHED, EMA, HOLD>   p = p - (lr * lr_factor * ratio) * u with u recomputed by the same helper from the
//                                          same stored values; EMA and HOLD as in kk_opt_adam
// The update is NOT Adam's bits (u is formed in another order of operations); the moments are.
// and, for Prodigy learning-rate estimation (include/avmoe.h, avmoe_opt_prodigy_step), two launches in place of kk_opt_adam --
//   kk_opt_prodigy_update<DECOUPLED, SCHED, EMA, HOLD>   the step of every element with the estimate d of the 32-byte Prodigy block in
//                                          every rate (prodigy_elem, adam_elem.h), the running gradient sum s beside the moments, and per
//                                          1024-element block the sums of c gr (x0 - p) and |s| in double
//   kk_opt_prodigy_finalize                one block adds both sums in finalize's order and writes num, den, d_hat, d_max and the d of the
//                                          NEXT step into the Prodigy block
// The per-range norms are a kernel of their own, next to finalize, and not a part of it: finalize is ONE block whose additions define the
// bits of total_norm, and a model has thousands of ranges -- a wave per range over many blocks finishes them in the time finalize takes,
// inside finalize they would wait on one block's 256 threads and stretch the serial part of every step.  Finalize only resets the
// report's header (first_nonfinite = -1) before the range kernel runs behind it on the same stream.
// Each body exists once; the host picks an instantiation from a table indexed by the flag bits, and every instantiation of a kernel takes
// the same arguments (those of an option that is off are not read).  Plain bandwidth kernels: 16-byte loads and stores, no matrix pipe,
// LDS only for the block reduction.  No floating-point atomics: the norm repeats bit for bit.
#include "../../include/avmoe.h"
#include "common.h"
#include "adam_elem.h"
#include "opt_table.h"
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>

namespace avmoe {

// sum over the block's elements of ((double)grad * grad_scale)^2 -> partials[blockIdx.x].  A launch whose grid does not match the table
// (a stale or foreign image) touches nothing but its own partial sum.
__global__ void __launch_bounds__(256) kk_opt_sqsum(const void* __restrict__ table, double* __restrict__ partials, float grad_scale) {
  OptWork w;
  double acc = 0.0;
  if (opt_work(table, w)) {
    const avmoe_opt_range& r = w.r;
    const long i0 = w.i0;
    const double gs = (double)grad_scale;
    if (i0 + 3 < r.n) {
      const float4 g = *(const float4*)(r.grad + i0);
      const double a = (double)g.x * gs, c = (double)g.y * gs, d = (double)g.z * gs, e = (double)g.w * gs;
      acc = a * a + c * c + d * d + e * e;
    } else {
      for (long i = i0; i < r.n; ++i) { const double a = (double)r.grad[i] * gs; acc += a * a; }
    }
  }
  const double sum = block_sum_256(acc);
  if (threadIdx.x == 0) partials[blockIdx.x] = sum;
}

// sum over the block's elements of ((double)(|param| * grad) * grad_scale)^2 -> partials[blockIdx.x]: the norm pass of the adaptive
// perturbation (ASAM's T_w g with T_w = |w|).  |p| * g is one fp32 product, as the perturbation kernel forms its factors; the rest is
// kk_opt_sqsum.  The parameters are only read.
__global__ void __launch_bounds__(256) kk_opt_sqsum_adaptive(const void* __restrict__ table, double* __restrict__ partials, float grad_scale) {
  OptWork w;
  double acc = 0.0;
  if (opt_work(table, w)) {
    const avmoe_opt_range& r = w.r;
    const long i0 = w.i0;
    const double gs = (double)grad_scale;
    if (i0 + 3 < r.n) {
      const float4 g = *(const float4*)(r.grad + i0), p = *(const float4*)(r.param + i0);
      const double a = (double)(fabsf(p.x) * g.x) * gs, c = (double)(fabsf(p.y) * g.y) * gs, d = (double)(fabsf(p.z) * g.z) * gs,
                   e = (double)(fabsf(p.w) * g.w) * gs;
      acc = a * a + c * c + d * d + e * e;
    } else {
      for (long i = i0; i < r.n; ++i) { const double a = (double)(fabsf(r.param[i]) * r.grad[i]) * gs; acc += a * a; }
    }
  }
  const double sum = block_sum_256(acc);
  if (threadIdx.x == 0) partials[blockIdx.x] = sum;
}

// One block: the sum of the partial sums.  Thread t adds partials[t], partials[t + 256], ... in that order, the 256 sums go through the
// tree above: a fixed order, written ONCE for kk_opt_finalize and kk_opt_sam_finalize, so both get the same bits from the same partials.
__device__ __forceinline__ double opt_total_256(const double* __restrict__ partials, long n_partials) {
  double acc = 0.0;
  for (long i = threadIdx.x; i < n_partials; i += 256) acc += partials[i];
  return block_sum_256(acc);
}

// the factor of a per-step schedule at n applied steps (include/avmoe.h, avmoe_opt_schedule), in double.  Contraction is off so that the
// expression rounds like the same closed form written on a host (LRSchedule.factor in avmoe_amd/train.py).
__device__ __forceinline__ double sched_factor(const avmoe_opt_schedule& s, int64_t n) {
#pragma clang fp contract(off)
  const int64_t W = s.warmup_steps;
  if (n < W) {
    const double s0 = (double)s.warmup_start;
    return s0 + (1.0 - s0) * (double)n / (double)W;
  }
  const int64_t u = n - W, D = s.total_steps - W, c = u < D ? u : D;
  const double fmin = (double)s.min_factor;
  switch (s.decay_kind) {
    case AVMOE_SCHED_COSINE: return fmin + (1.0 - fmin) * 0.5 * (1.0 + cos(M_PI * (double)c / (double)D));
    case AVMOE_SCHED_LINEAR: return 1.0 - (1.0 - fmin) * (double)c / (double)D;
    case AVMOE_SCHED_STEP: return pow((double)s.gamma, (double)(u / s.step_size));
    default: return 1.0;
  }
}

// the decay of the weight average at n applied steps, this one included (include/avmoe.h, avmoe_opt_ema), in double: contraction off for the
// same reason (FlatAdam.ema_decay_at in avmoe_amd/train.py is the host's copy)
__device__ __forceinline__ double ema_decay(const avmoe_opt_ema& e, int64_t n) {
#pragma clang fp contract(off)
  const double d = (double)e.decay, w = (1.0 + (double)n) / ((double)e.warmup + (double)n);
  return w < d ? w : d;
}

// Stochastic weight averaging (include/avmoe.h, avmoe_opt_swa).  The copy the finalize kernel gets is the caller's with the half that is
// off marked by a value the checks refuse from a caller: start = 0 without AVMOE_OPT_SWA, lr_start = -1 without AVMOE_OPT_SWA_LR.
__device__ __forceinline__ bool swa_averages(const avmoe_opt_swa& w) { return w.start > 0; }
__device__ __forceinline__ bool swa_anneals(const avmoe_opt_swa& w) { return w.lr_start >= 0; }

// the uniform average's decay at n applied steps, this one included, in double (FlatAdam.swa_decay_at is the host's copy): 0 below
// `start` (the shadow follows the parameters), k / (k + 1) at the k-th averaging step after the first (torch's AveragedModel with
// n_averaged = k), 1 between two averaging steps (the shadow keeps its value)
__device__ __forceinline__ double swa_decay(const avmoe_opt_swa& w, int64_t n) {
#pragma clang fp contract(off)
  if (n < w.start) return 0.0;
  const int64_t u = n - w.start;
  const int64_t c = w.freq;
  if (u % c != 0) return 1.0;
  const double k = (double)(u / c);
  return k / (k + 1.0);
}

// the learning-rate factor at n applied steps with the annealing of torch's SWALR from step lr_start on, in closed form and in double
// (LRSchedule.factor is the host's copy, in this operation order); `s` is the base schedule, all zero for base = 1
__device__ __forceinline__ double swa_lr_factor(const avmoe_opt_schedule& s, const avmoe_opt_swa& w, int64_t n) {
#pragma clang fp contract(off)
  if (n < w.lr_start) return sched_factor(s, n);
  const double f0 = sched_factor(s, w.lr_start), to = (double)w.lr_factor;
  double t = 1.0;
  if (w.anneal_steps > 0) {
    t = (double)(n - w.lr_start) / (double)w.anneal_steps;
    t = t < 1.0 ? t : 1.0;
  }
  const double alpha = w.anneal_kind == AVMOE_SWA_ANNEAL_LINEAR ? t : (1.0 - cos(M_PI * t)) / 2.0;
  return f0 + (to - f0) * alpha;
}

// One block.  The partial sums are added by opt_total_256: a fixed order.  n_partials == 0 (neither clipping nor skipping asked for): the
// norm is reported as 0 and only the counters advance.
// SCHED: the step that is applied now is number n = applied_steps before it (the first one has n = 0); its factor goes into the state
// block, rounded once to fp32.  A skipped step leaves the factor alone.
// EMA: the average's decay for this step, from n = applied_steps AFTER it (the first one has n = 1), likewise.
// swa: where its half is on (see above), the factor is the annealed one and the decay that of the uniform average -- the same words of
// the state block by another rule, one branch that every launch takes the same way.
// The schedule and the average's constants ride in the kernel arguments: constants of the run, so a captured launch replays them.
// report != NULL (AVMOE_OPT_REPORT): the header of the report is reset for kk_opt_range_norms, which follows on the same stream.
template <bool SCHED, bool EMA>
__global__ void __launch_bounds__(256) kk_opt_finalize(const double* __restrict__ partials, long n_partials, avmoe_opt_state* __restrict__ state,
                                                       float max_norm, int clip, int skip_nonfinite, float beta1, float beta2,
                                                       avmoe_opt_schedule sched, avmoe_opt_ema ema, avmoe_opt_report_header* __restrict__ report,
                                                       int n_ranges, avmoe_opt_swa swa) {
  const double sum = opt_total_256(partials, n_partials);
  if (threadIdx.x != 0) return;
  if (report) *report = avmoe_opt_report_header{-1, n_ranges, {0, 0}};
  const float total = (float)sqrt(sum);
  float coef = 1.0f;
  if (clip) {                                           // torch.nn.utils.clip_grad_norm_: clamp(max_norm / (total_norm + 1e-6), max = 1); NaN stays NaN
    const float c = max_norm / (total + 1e-6f);
    coef = c < 1.0f ? c : (c != c ? c : 1.0f);
  }
  const int skip = (skip_nonfinite && !isfinite(total)) ? 1 : 0;
  const int64_t before = state->applied_steps, applied = before + (skip ? 0 : 1);
  state->total_norm = total;
  state->clip_coef = coef;
  state->skip = skip;
  state->applied_steps = applied;
  state->skipped_steps += skip;
  const double bc1 = 1.0 - pow((double)beta1, (double)applied), bc2 = 1.0 - pow((double)beta2, (double)applied);
  state->bc1 = (float)bc1;
  state->bc2_sqrt = (float)sqrt(bc2);
  if constexpr (SCHED) {
    if (!skip) state->lr_factor = (float)(swa_anneals(swa) ? swa_lr_factor(sched, swa, before) : sched_factor(sched, before));
  }
  if constexpr (EMA) {
    if (!skip) state->ema_decay = (float)(swa_averages(swa) ? swa_decay(swa, applied) : ema_decay(ema, applied));
  }
}

// AVMOE_OPT_REPORT.  One wave per range, grid-strided over the ranges.  The blocks of a range are neighbours in the block map, which is
// sorted by range: a binary search finds the first, the range's length says how many.  Lane l adds partials l, l + 64, ... of the range
// in that order and a butterfly over the 64 lanes adds the lane sums -- a fixed order, every lane ends with the same bits.  A range
// without elements has no block and reports 0.  A launch that does not match its table (wrong magic, other counts) touches nothing, and
// a range whose blocks are not where the map must have them (a foreign image) is left out.
__global__ void __launch_bounds__(256) kk_opt_range_norms(const void* __restrict__ table, const double* __restrict__ partials, int n_ranges,
                                                          long n_blocks, avmoe_opt_report_header* __restrict__ report) {
  const OptHeader h = *(const OptHeader*)table;
  if (h.magic != OPT_MAGIC || h.n_ranges != n_ranges || h.n_blocks != n_blocks) return;
  const avmoe_opt_range* ranges = (const avmoe_opt_range*)((const char*)table + sizeof(OptHeader));
  const OptBlock* map = (const OptBlock*)(ranges + n_ranges);
  float* norms = (float*)(report + 1);
  const int lane = threadIdx.x & 63, waves = (int)gridDim.x * 4;
  for (int r = (int)blockIdx.x * 4 + ((int)threadIdx.x >> 6); r < n_ranges; r += waves) {
    const long nb = (long)((ranges[r].n + OPT_BLOCK - 1) / OPT_BLOCK);
    long lo = 0, hi = n_blocks;                       // the first block whose range is >= r
    while (lo < hi) {
      const long mid = (lo + hi) >> 1;
      if (map[mid].range < r) lo = mid + 1; else hi = mid;
    }
    if (nb < 0 || lo + nb > n_blocks) continue;
    if (nb > 0 && (map[lo].range != r || map[lo + nb - 1].range != r)) continue;
    double acc = 0.0;
    for (long i = lane; i < nb; i += 64) acc += partials[lo + i];
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) acc += __shfl_xor(acc, s, 64);
    if (lane == 0) {
      const float norm = (float)sqrt(acc);
      norms[r] = norm;
      // -1 is the largest unsigned value: the minimum over the ranges that are not finite, or -1 where there is none
      if (!isfinite(norm)) atomicMin((unsigned int*)&report->first_nonfinite, (unsigned int)r);
    }
  }
}

// SCHED: the range's rate times the state block's lr_factor, for the update and for the decoupled decay term alike
// EMA: shadows[range] is the range's average; the state block's ema_decay is this step's d
// HOLD: hold[range] holds the range's unperturbed parameters (kk_opt_sam_perturb): every p is read from there and written to param; a
// skipped step writes param = hold and nothing else
template <bool DECOUPLED, bool SCHED, bool EMA, bool HOLD>
__global__ void __launch_bounds__(256) kk_opt_adam(const void* __restrict__ table, const avmoe_opt_state* __restrict__ state, float b1, float b2,
                                                   float eps, float grad_scale, float* const* __restrict__ shadows, int n_shadows,
                                                   float* const* __restrict__ hold) {
  if constexpr (!HOLD) {
    if (state->skip) return;                            // a skipped step writes nothing: p, m, v (and the average) stay bit for bit
  }
  OptWork w;
  if (!opt_work(table, w)) return;
  const avmoe_opt_range& r = w.r;
  const float* h = nullptr;
  if constexpr (HOLD) {
    h = opt_shadow(w, hold, n_shadows);
    if (!h) return;
    if (state->skip) { restore_quad(r.param, h, w.i0, (long)r.n); return; }
  }
  float lr = r.lr;
  if constexpr (SCHED) lr *= state->lr_factor;
  float* e = nullptr;
  float d = 0.f;
  if constexpr (EMA) {
    e = opt_shadow(w, shadows, n_shadows);
    if (!e) return;
    d = state->ema_decay;
  }
  // one multiplier for the gradient: grad_scale * clip factor (== grad_scale exactly when the factor is 1)
  adam_quad<DECOUPLED, EMA, HOLD>(r.param, r.grad, r.exp_avg, r.exp_avg_sq, w.i0, (long)r.n, lr, b1, b2, eps, r.weight_decay, state->bc1,
                                  state->bc2_sqrt, grad_scale * state->clip_coef, e, d, h);
}

// ---- layer-wise trust ratios (include/avmoe.h, avmoe_opt_lamb_step) ----
static_assert(sizeof(avmoe_opt_lamb_header) == 16 && sizeof(avmoe_opt_lamb_layout) == 16, "trust report layout");

// The moments of every element and the block's sums for the two norms: sums[2 b] = sum of (double)u^2, sums[2 b + 1] = sum of (double)p^2
// over the elements of table block b, each through block_sum_256 (a fixed order).  p is read from param, under HOLD from hold[range];
// m and v are written, p is not.  u is formed from the m and v that have just been stored (lamb_dir).  A skipped step writes nothing;
// a launch that does not match its table, or whose hold / shadow entry for the range cannot take 16-byte accesses, touches nothing
// (`shadows` is NULL without the average: kk_opt_lamb_apply would refuse such a range, so its moments must stay too).
template <bool DECOUPLED, bool HOLD>
__global__ void __launch_bounds__(256) kk_opt_lamb_moments(const void* __restrict__ table, const avmoe_opt_state* __restrict__ state, float b1, float b2,
                                                           float eps, float grad_scale, float* const* __restrict__ shadows,
                                                           float* const* __restrict__ hold, int n_ranges, double* __restrict__ sums) {
  if (state->skip) return;
  OptWork w;
  bool ok = opt_work(table, w) && w.n_ranges == n_ranges;
  const float* __restrict__ src = nullptr;
  if (ok) {
    src = w.r.param;
    if constexpr (HOLD) { src = opt_shadow(w, hold, n_ranges); ok = src != nullptr; }
    if (ok && shadows) ok = opt_shadow(w, shadows, n_ranges) != nullptr;
  }
  double su = 0.0, sp = 0.0;
  if (ok) {
    const avmoe_opt_range& r = w.r;
    const long i0 = w.i0, n = r.n;
    const float bc1 = state->bc1, bc2_sqrt = state->bc2_sqrt, gscale = grad_scale * state->clip_coef, wd = r.weight_decay;
    if (i0 + 3 < n) {
      const float4 pp = *(const float4*)(src + i0), gg = *(const float4*)(r.grad + i0);
      float4 mm = *(float4*)(r.exp_avg + i0), vv = *(float4*)(r.exp_avg_sq + i0);
      const float* P = (const float*)&pp; const float* G = (const float*)&gg; float* M = (float*)&mm; float* V = (float*)&vv;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        lamb_moments<DECOUPLED>(P[k], M[k], V[k], G[k], b1, b2, wd, gscale);
        const double u = (double)lamb_dir<DECOUPLED>(P[k], M[k], V[k], wd, bc1, bc2_sqrt, eps), q = (double)P[k];
        su += u * u;
        sp += q * q;
      }
      *(float4*)(r.exp_avg + i0) = mm; *(float4*)(r.exp_avg_sq + i0) = vv;
    } else {
      for (long i = i0; i < n; ++i) {
        const float pv = src[i];
        float mv = r.exp_avg[i], vv = r.exp_avg_sq[i];
        lamb_moments<DECOUPLED>(pv, mv, vv, r.grad[i], b1, b2, wd, gscale);
        r.exp_avg[i] = mv; r.exp_avg_sq[i] = vv;
        const double u = (double)lamb_dir<DECOUPLED>(pv, mv, vv, wd, bc1, bc2_sqrt, eps), q = (double)pv;
        su += u * u;
        sp += q * q;
      }
    }
  }
  // thread 0 of a block that has work serves the block's first element, so its `ok` is the block's
  const double tu = block_sum_256(su);
  __syncthreads();                                      // the tree's LDS is used a second time
  const double tp = block_sum_256(sp);
  if (threadIdx.x == 0 && ok) { sums[2 * (long)blockIdx.x] = tu; sums[2 * (long)blockIdx.x + 1] = tp; }
}

// One wave per range, grid-strided over the ranges: the walk of kk_opt_range_norms over the two sums of every block of the range (binary
// search of the block map, lane l adds blocks l, l + 64, ..., a fixed butterfly: no floating-point atomics, the same bits every time).
// The report: the 16-byte header, then w_norm[n_ranges], u_norm[n_ranges], ratio[n_ranges].  The norms are the double square roots rounded
// to fp32; the ratio is formed in double from the double norms and rounded once.  limits[r] < 0 (or NaN): the range is not adapted,
// ratio exactly 1; 0: adapted; > 0: the ratio is clamped to it.  A skipped step leaves the report as it was.
__global__ void __launch_bounds__(256) kk_opt_lamb_ratio(const void* __restrict__ table, const double* __restrict__ sums, int n_ranges, long n_blocks,
                                                         const float* __restrict__ limits, const avmoe_opt_state* __restrict__ state,
                                                         avmoe_opt_lamb_header* __restrict__ report) {
  if (state->skip) return;
  const OptHeader h = *(const OptHeader*)table;
  if (h.magic != OPT_MAGIC || h.n_ranges != n_ranges || h.n_blocks != n_blocks) return;
  const avmoe_opt_range* ranges = (const avmoe_opt_range*)((const char*)table + sizeof(OptHeader));
  const OptBlock* map = (const OptBlock*)(ranges + n_ranges);
  float* w_norm = (float*)(report + 1);
  float* u_norm = w_norm + n_ranges;
  float* ratio = u_norm + n_ranges;
  if (blockIdx.x == 0 && threadIdx.x == 0) *report = avmoe_opt_lamb_header{n_ranges, {0, 0, 0}};
  const int lane = threadIdx.x & 63, waves = (int)gridDim.x * 4;
  for (int r = (int)blockIdx.x * 4 + ((int)threadIdx.x >> 6); r < n_ranges; r += waves) {
    const long nb = (long)((ranges[r].n + OPT_BLOCK - 1) / OPT_BLOCK);
    long lo = 0, hi = n_blocks;                       // the first block whose range is >= r
    while (lo < hi) {
      const long mid = (lo + hi) >> 1;
      if (map[mid].range < r) lo = mid + 1; else hi = mid;
    }
    if (nb < 0 || lo + nb > n_blocks) continue;
    if (nb > 0 && (map[lo].range != r || map[lo + nb - 1].range != r)) continue;
    double au = 0.0, ap = 0.0;
    for (long i = lane; i < nb; i += 64) { au += sums[2 * (lo + i)]; ap += sums[2 * (lo + i) + 1]; }
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) { au += __shfl_xor(au, s, 64); ap += __shfl_xor(ap, s, 64); }
    if (lane == 0) {
      const double wn = sqrt(ap), un = sqrt(au);
      const float lim = limits[r];
      double q = 1.0;
      if (lim >= 0.f && wn > 0.0 && un > 0.0 && isfinite(wn) && isfinite(un)) {
        q = wn / un;
        if (lim > 0.f && q > (double)lim) q = (double)lim;
      }
      w_norm[r] = (float)wn;
      u_norm[r] = (float)un;
      ratio[r] = (float)q;
    }
  }
}

// p = p - ((lr * lr_factor) * ratio) * u for every element of every range, u recomputed by lamb_dir from the m and v kk_opt_lamb_moments
// has stored and the p it read: the bits that were normed.  SCHED, EMA and HOLD as in kk_opt_adam; m, v and the gradients are not
// touched.  A skipped step writes nothing, under HOLD param = hold and nothing else.
template <bool DECOUPLED, bool SCHED, bool EMA, bool HOLD>
__global__ void __launch_bounds__(256) kk_opt_lamb_apply(const void* __restrict__ table, const avmoe_opt_state* __restrict__ state, float eps,
                                                         float* const* __restrict__ shadows, float* const* __restrict__ hold, int n_ranges,
                                                         const avmoe_opt_lamb_header* __restrict__ report) {
  if constexpr (!HOLD) {
    if (state->skip) return;
  }
  OptWork w;
  if (!opt_work(table, w) || w.n_ranges != n_ranges) return;
  const avmoe_opt_range& r = w.r;
  const float* h = nullptr;
  if constexpr (HOLD) {
    h = opt_shadow(w, hold, n_ranges);
    if (!h) return;
    if (state->skip) { restore_quad(r.param, h, w.i0, (long)r.n); return; }
  }
  float lr = r.lr;
  if constexpr (SCHED) lr *= state->lr_factor;
  float* e = nullptr;
  float d = 0.f;
  if constexpr (EMA) {
    e = opt_shadow(w, shadows, n_ranges);
    if (!e) return;
    d = state->ema_decay;
  }
  const float ratio = ((const float*)(report + 1))[2 * (long)n_ranges + w.range];
  lamb_quad<DECOUPLED, EMA, HOLD>(r.param, r.exp_avg, r.exp_avg_sq, w.i0, (long)r.n, lr * ratio, eps, r.weight_decay, state->bc1, state->bc2_sqrt,
                                  e, d, h);
}

// ---- Prodigy learning-rate estimation (include/avmoe.h, avmoe_opt_prodigy_step) ----
static_assert(sizeof(avmoe_opt_prodigy_state) == 32 && sizeof(avmoe_opt_prodigy) == 16 && sizeof(avmoe_opt_prodigy_layout) == 16, "Prodigy layout");

// The step of every element of every range with this step's d, read from the Prodigy block, and the block's two sums:
// sums[2 b] = sum of (double)(c gr) * ((double)x0 - (double)p), sums[2 b + 1] = sum of (double)|s| over the elements of table block b, each
// through block_sum_256 (a fixed order).  SCHED, EMA and HOLD as in kk_opt_adam; x0s[range] and ss[range] are the range's x0 and s, under
// the rules of the shadows.  A skipped step writes nothing, the sums included; under HOLD param = hold and nothing else.  A launch that
// does not match its table, or a range one of whose side buffers cannot take 16-byte accesses, touches nothing but its own two sums,
// which are written as 0: kk_opt_prodigy_finalize adds every block's.
template <bool DECOUPLED, bool SCHED, bool EMA, bool HOLD>
__global__ void __launch_bounds__(256) kk_opt_prodigy_update(const void* __restrict__ table, const avmoe_opt_state* __restrict__ state, float b1, float b2,
                                                             float beta3, float eps, float grad_scale, float* const* __restrict__ shadows,
                                                             float* const* __restrict__ hold, float* const* __restrict__ x0s,
                                                             float* const* __restrict__ ss, int n_ranges, float d0, int safeguard,
                                                             const avmoe_opt_prodigy_state* __restrict__ blk, double* __restrict__ sums) {
  const bool skip = state->skip != 0;
  if constexpr (!HOLD) {
    if (skip) return;
  }
  OptWork w;
  bool ok = opt_work(table, w) && w.n_ranges == n_ranges;
  const float* x0 = nullptr; const float* h = nullptr;
  float* s = nullptr; float* e = nullptr;
  if (ok) {
    x0 = opt_shadow(w, x0s, n_ranges);
    s = opt_shadow(w, ss, n_ranges);
    ok = x0 != nullptr && s != nullptr;
    if constexpr (HOLD) { h = opt_shadow(w, hold, n_ranges); ok = ok && h != nullptr; }
    if constexpr (EMA) { e = opt_shadow(w, shadows, n_ranges); ok = ok && e != nullptr; }
  }
  if constexpr (HOLD) {
    if (skip) {                                          // the whole launch takes this branch: no sum is formed
      if (ok) restore_quad(w.r.param, h, w.i0, (long)w.r.n);
      return;
    }
  }
  double dot = 0.0, l1 = 0.0;
  if (ok) {
#pragma clang fp contract(off)
    const avmoe_opt_range& r = w.r;
    float lr = r.lr;
    if constexpr (SCHED) lr *= state->lr_factor;
    ProdigyScal k;
    k.d = blk->d;
    k.step = lr * k.d;
    const float dd0 = k.d / d0;
    k.c = (safeguard ? k.d : k.step) * dd0;
    k.deps = k.d * eps;
    k.b1 = b1; k.b2 = b2; k.beta3 = beta3; k.wd = r.weight_decay;
    k.gscale = grad_scale * state->clip_coef;
    float decay = 0.f;
    if constexpr (EMA) decay = state->ema_decay;
    prodigy_quad<DECOUPLED, EMA, HOLD>(r.param, r.grad, r.exp_avg, r.exp_avg_sq, s, x0, w.i0, (long)r.n, k, e, decay, h, dot, l1);
  }
  const double td = block_sum_256(dot);
  __syncthreads();                                      // the tree's LDS is used a second time
  const double ta = block_sum_256(l1);
  if (threadIdx.x == 0) { sums[2 * (long)blockIdx.x] = td; sums[2 * (long)blockIdx.x + 1] = ta; }
}

// One block.  Thread t adds sums of blocks t, t + 256, ... in that order, the 256 thread sums go through block_sum_256: opt_total_256's
// order over each of the two interleaved sums.  Then, in double unless stated (FlatAdam.prodigy_d_next in avmoe_amd/train.py is the
// host's copy; contraction off):
//     num = beta3 * num + sum_dot ;  den = sum_abs
//     d_hat = fp32(d_coef * num / den)      left as it is when den is not > 0 or num, den or the quotient is not a finite fp32
//     d_max = max(d_max, d_hat) ;  d = min(d_max, fp32(d * growth))      growth == 0: d = d_max
// A skipped step, or a launch that does not match its table's header, leaves the block as it is.
__global__ void __launch_bounds__(256) kk_opt_prodigy_finalize(const void* __restrict__ table, int n_ranges, long n_blocks,
                                                               const double* __restrict__ sums, const avmoe_opt_state* __restrict__ state,
                                                               avmoe_opt_prodigy_state* __restrict__ blk, float beta3, float d_coef, float growth) {
#pragma clang fp contract(off)
  if (state->skip) return;
  const OptHeader h = *(const OptHeader*)table;
  if (h.magic != OPT_MAGIC || h.n_ranges != n_ranges || h.n_blocks != n_blocks) return;
  double ad = 0.0, aa = 0.0;
  for (long i = threadIdx.x; i < n_blocks; i += 256) { ad += sums[2 * i]; aa += sums[2 * i + 1]; }
  const double sum_dot = block_sum_256(ad);
  __syncthreads();
  const double sum_abs = block_sum_256(aa);
  if (threadIdx.x != 0) return;
  const double num = (double)beta3 * blk->num + sum_dot, den = sum_abs;
  float d_hat = blk->d_hat, d_max = blk->d_max, d = blk->d;
  if (den > 0.0 && isfinite(num) && isfinite(den)) {
    const double q = (double)d_coef * num / den;
    if (fabs(q) <= 3.4028234663852886e38) d_hat = (float)q;
  }
  d_max = d_hat > d_max ? d_hat : d_max;
  if (growth > 0.f) { const float g = d * growth; d = g < d_max ? g : d_max; }
  else d = d_max;
  blk->num = num; blk->den = den;
  blk->d_hat = d_hat; blk->d_max = d_max; blk->d = d;
}

// One block: the SAM block from the partial sums of the perturbing gradient's norm pass.  The sum, the square root and its rounding are
// those of kk_opt_finalize, so `norm` has the bits total_norm gets from the same partial sums.
__global__ void __launch_bounds__(256) kk_opt_sam_finalize(const double* __restrict__ partials, long n_partials, avmoe_opt_sam_state* __restrict__ sam,
                                                           float rho) {
  const double sum = opt_total_256(partials, n_partials);
  if (threadIdx.x != 0) return;
  const float norm = (float)sqrt(sum);
  const bool fin = isfinite(norm);
  *sam = avmoe_opt_sam_state{norm, fin ? (float)((double)rho / ((double)norm + 1e-12)) : 0.f, fin ? 0 : 1, 0};
}

// hold[i] = param[i], then param[i] = param[i] + e (sam_elem, adam_elem.h) for every element of every range; with the block's
// `nonfinite` set only hold is written.  Gradients are only read; alignment padding belongs to no range and is not touched.
template <bool ADAPTIVE>
__global__ void __launch_bounds__(256) kk_opt_sam_perturb(const void* __restrict__ table, const avmoe_opt_sam_state* __restrict__ sam, float grad_scale,
                                                          float* const* __restrict__ hold, int n_hold) {
  OptWork w;
  if (!opt_work(table, w)) return;
  float* __restrict__ h = opt_shadow(w, hold, n_hold);
  if (!h) return;
  const float scale = sam->scale;
  const bool move = sam->nonfinite == 0;
  float* __restrict__ p = w.r.param;
  const float* __restrict__ g = w.r.grad;
  const long i0 = w.i0, n = w.r.n;
  if (i0 + 3 < n) {
    float4 pp = *(const float4*)(p + i0);
    const float4 gg = *(const float4*)(g + i0);
    *(float4*)(h + i0) = pp;
    if (move) {
      float* P = (float*)&pp; const float* G = (const float*)&gg;
#pragma unroll
      for (int k = 0; k < 4; ++k) P[k] = sam_elem<ADAPTIVE>(P[k], G[k], grad_scale, scale);
      *(float4*)(p + i0) = pp;
    }
  } else {
    for (long i = i0; i < n; ++i) {
      const float a = p[i];
      h[i] = a;
      if (move) p[i] = sam_elem<ADAPTIVE>(a, g[i], grad_scale, scale);
    }
  }
}

// param[i] <-> shadow[i] for every element of every range; alignment padding belongs to no range and is not touched
__global__ void __launch_bounds__(256) kk_opt_swap(const void* __restrict__ table, float* const* __restrict__ shadows, int n_shadows) {
  OptWork w;
  if (!opt_work(table, w)) return;
  float* __restrict__ e = opt_shadow(w, shadows, n_shadows);
  if (!e) return;
  float* __restrict__ p = w.r.param;
  const long i0 = w.i0, n = w.r.n;
  if (i0 + 3 < n) {
    const float4 pp = *(const float4*)(p + i0), ee = *(const float4*)(e + i0);
    *(float4*)(p + i0) = ee; *(float4*)(e + i0) = pp;
  } else {
    for (long i = i0; i < n; ++i) { const float a = p[i]; p[i] = e[i]; e[i] = a; }
  }
}

// ---- the buffer table (include/avmoe.h, "averaged buffers"): tensors that stay at their own addresses -- BatchNorm running statistics,
// which the sites' forward kernels write in place -- each with a shadow in one flat allocation of the caller.  A table of its own beside
// the range table: a buffer has no gradient and no moments, and it may be only 4-byte aligned, so the buffer side is accessed element by
// element (a block's 256 threads take consecutive elements, four rounds: every access is a full coalesced line anyway).
constexpr uint32_t OPT_BUF_MAGIC = 0x4f505442u;  // "OPTB"
static_assert(sizeof(avmoe_opt_buffer) == 24, "buffer table layout");

// What a block of a one-block-per-table-block launch serves: elements [i0, i0 + 1024) of record `rec`, clipped to its n.
// -> false where the launch does not match the table (wrong magic, other counts, a block or record index outside it, a record without
// elements): such a launch touches nothing.
__device__ __forceinline__ bool opt_buffer_work(const void* __restrict__ table, int n_buffers, long n_blocks, avmoe_opt_buffer& rec, long& i0) {
  const OptHeader h = *(const OptHeader*)table;
  if (h.magic != OPT_BUF_MAGIC || h.n_ranges != n_buffers || h.n_blocks != n_blocks || (long)blockIdx.x >= h.n_blocks) return false;
  const avmoe_opt_buffer* recs = (const avmoe_opt_buffer*)((const char*)table + sizeof(OptHeader));
  const OptBlock b = ((const OptBlock*)(recs + h.n_ranges))[blockIdx.x];
  if (b.range < 0 || b.range >= h.n_ranges || b.block < 0) return false;
  rec = recs[b.range];
  i0 = (long)b.block * OPT_BLOCK;
  return rec.n > 0 && i0 < rec.n;
}

// shadow = d_n shadow + (1 - d_n) buffer for every element of every record, d_n and the skip flag from the state block the step's
// finalize launch has just written.  The four loads of a thread are unconditional, at an index clamped into the record, and issued
// before the first store; only the stores are masked (DESIGN_CURRENT.md section 3).  The buffers are only read.
__global__ void __launch_bounds__(256) kk_opt_ema_buffers(const void* __restrict__ table, int n_buffers, long n_blocks,
                                                          const avmoe_opt_state* __restrict__ state) {
  if (state->skip) return;                              // a skipped step writes nothing
  avmoe_opt_buffer r;
  long i0;
  if (!opt_buffer_work(table, n_buffers, n_blocks, r, i0)) return;
  const float d = state->ema_decay;
  const float* __restrict__ b = r.buffer;
  float* __restrict__ s = r.shadow;
  const long last = r.n - 1;
  long idx[4];
  float x[4], e[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const long i = i0 + k * 256 + (long)threadIdx.x;
    idx[k] = i < last ? i : last;
    x[k] = b[idx[k]];
    e[k] = s[idx[k]];
  }
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (i0 + k * 256 + (long)threadIdx.x <= last) s[idx[k]] = ema_next(e[k], x[k], d);
}

// buffer[i] <-> shadow[i] for every element of every record; the same walk
__global__ void __launch_bounds__(256) kk_opt_swap_buffers(const void* __restrict__ table, int n_buffers, long n_blocks) {
  avmoe_opt_buffer r;
  long i0;
  if (!opt_buffer_work(table, n_buffers, n_blocks, r, i0)) return;
  float* __restrict__ b = r.buffer;
  float* __restrict__ s = r.shadow;
  const long last = r.n - 1;
  long idx[4];
  float x[4], e[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const long i = i0 + k * 256 + (long)threadIdx.x;
    idx[k] = i < last ? i : last;
    x[k] = b[idx[k]];
    e[k] = s[idx[k]];
  }
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (i0 + k * 256 + (long)threadIdx.x <= last) { b[idx[k]] = e[k]; s[idx[k]] = x[k]; }
}

// the instantiations, indexed by the flag bits: an option more is a template parameter more and an initialiser twice as long
using FinalizeKernel = decltype(&kk_opt_finalize<false, false>);
using AdamKernel = decltype(&kk_opt_adam<false, false, false, false>);
constexpr FinalizeKernel OPT_FINALIZE[4] = {   // [SCHED | EMA << 1]
    kk_opt_finalize<false, false>, kk_opt_finalize<true, false>, kk_opt_finalize<false, true>, kk_opt_finalize<true, true>};
constexpr AdamKernel OPT_ADAM[16] = {          // [DECOUPLED | SCHED << 1 | EMA << 2 | HOLD << 3]
    kk_opt_adam<false, false, false, false>, kk_opt_adam<true, false, false, false>, kk_opt_adam<false, true, false, false>,
    kk_opt_adam<true, true, false, false>,   kk_opt_adam<false, false, true, false>, kk_opt_adam<true, false, true, false>,
    kk_opt_adam<false, true, true, false>,   kk_opt_adam<true, true, true, false>,   kk_opt_adam<false, false, false, true>,
    kk_opt_adam<true, false, false, true>,   kk_opt_adam<false, true, false, true>,  kk_opt_adam<true, true, false, true>,
    kk_opt_adam<false, false, true, true>,   kk_opt_adam<true, false, true, true>,   kk_opt_adam<false, true, true, true>,
    kk_opt_adam<true, true, true, true>};

using LambMomentsKernel = decltype(&kk_opt_lamb_moments<false, false>);
using LambApplyKernel = decltype(&kk_opt_lamb_apply<false, false, false, false>);
constexpr LambMomentsKernel OPT_LAMB_MOMENTS[4] = {   // [DECOUPLED | HOLD << 1]
    kk_opt_lamb_moments<false, false>, kk_opt_lamb_moments<true, false>, kk_opt_lamb_moments<false, true>, kk_opt_lamb_moments<true, true>};
constexpr LambApplyKernel OPT_LAMB_APPLY[16] = {      // [DECOUPLED | SCHED << 1 | EMA << 2 | HOLD << 3]
    kk_opt_lamb_apply<false, false, false, false>, kk_opt_lamb_apply<true, false, false, false>, kk_opt_lamb_apply<false, true, false, false>,
    kk_opt_lamb_apply<true, true, false, false>,   kk_opt_lamb_apply<false, false, true, false>, kk_opt_lamb_apply<true, false, true, false>,
    kk_opt_lamb_apply<false, true, true, false>,   kk_opt_lamb_apply<true, true, true, false>,   kk_opt_lamb_apply<false, false, false, true>,
    kk_opt_lamb_apply<true, false, false, true>,   kk_opt_lamb_apply<false, true, false, true>,  kk_opt_lamb_apply<true, true, false, true>,
    kk_opt_lamb_apply<false, false, true, true>,   kk_opt_lamb_apply<true, false, true, true>,   kk_opt_lamb_apply<false, true, true, true>,
    kk_opt_lamb_apply<true, true, true, true>};

using ProdigyKernel = decltype(&kk_opt_prodigy_update<false, false, false, false>);
constexpr ProdigyKernel OPT_PRODIGY[16] = {           // [DECOUPLED | SCHED << 1 | EMA << 2 | HOLD << 3]
    kk_opt_prodigy_update<false, false, false, false>, kk_opt_prodigy_update<true, false, false, false>,
    kk_opt_prodigy_update<false, true, false, false>,  kk_opt_prodigy_update<true, true, false, false>,
    kk_opt_prodigy_update<false, false, true, false>,  kk_opt_prodigy_update<true, false, true, false>,
    kk_opt_prodigy_update<false, true, true, false>,   kk_opt_prodigy_update<true, true, true, false>,
    kk_opt_prodigy_update<false, false, false, true>,  kk_opt_prodigy_update<true, false, false, true>,
    kk_opt_prodigy_update<false, true, false, true>,   kk_opt_prodigy_update<true, true, false, true>,
    kk_opt_prodigy_update<false, false, true, true>,   kk_opt_prodigy_update<true, false, true, true>,
    kk_opt_prodigy_update<false, true, true, true>,    kk_opt_prodigy_update<true, true, true, true>};

static long range_blocks(int64_t n) { return (long)((n + OPT_BLOCK - 1) / OPT_BLOCK); }

// host-side validation of a range list -> OK and the block count, or the error
static int check_ranges(const char* who, const avmoe_opt_range* ranges, int32_t n_ranges, int64_t* n_blocks) {
  if (n_ranges < 0) { set_last_error("%s: negative range count %d", who, (int)n_ranges); return ERR_BAD_ARG; }
  if (n_ranges > 0 && !ranges) { set_last_error("%s: ranges is NULL", who); return ERR_BAD_ARG; }
  int64_t nb = 0;
  for (int32_t i = 0; i < n_ranges; ++i) {
    const avmoe_opt_range& r = ranges[i];
    if (r.n < 0) { set_last_error("%s: range %d has negative length %lld", who, (int)i, (long long)r.n); return ERR_BAD_ARG; }
    if (!r.param || !r.grad || !r.exp_avg || !r.exp_avg_sq) { set_last_error("%s: range %d has a NULL pointer", who, (int)i); return ERR_BAD_ARG; }
    if (!(r.lr == r.lr) || !(r.weight_decay == r.weight_decay)) { set_last_error("%s: range %d has a NaN lr / weight_decay", who, (int)i); return ERR_BAD_ARG; }
    if ((((uintptr_t)r.param | (uintptr_t)r.grad | (uintptr_t)r.exp_avg | (uintptr_t)r.exp_avg_sq) & 15u) != 0) {
      set_last_error("%s: range %d does not start 16-byte aligned", who, (int)i); return ERR_ALIGNMENT;
    }
    if (r.n > ((int64_t)INT32_MAX - 1) * OPT_BLOCK) { set_last_error("%s: range %d is too long", who, (int)i); return ERR_UNSUPPORTED; }
    nb += range_blocks(r.n);
  }
  if (nb > (int64_t)INT32_MAX) { set_last_error("%s: more than 2^31 blocks", who); return ERR_UNSUPPORTED; }
  *n_blocks = nb;
  return OK;
}

static size_t table_bytes_of(int32_t n_ranges, int64_t n_blocks) {
  return round16(sizeof(OptHeader) + (size_t)n_ranges * sizeof(avmoe_opt_range) + (size_t)n_blocks * sizeof(OptBlock));
}

// the table half of a launch's arguments: all avmoe_opt_swap_ema has
static int check_table_args(const char* who, const void* table, int32_t n_ranges, int64_t n_blocks) {
  if (!table) { set_last_error("%s: NULL table", who); return ERR_BAD_ARG; }
  if (n_ranges < 0 || n_blocks < 0 || n_blocks > (int64_t)INT32_MAX) { set_last_error("%s: bad range / block count", who); return ERR_BAD_ARG; }
  if (((uintptr_t)table & 15u) != 0) { set_last_error("%s: the table must be 16-byte aligned", who); return ERR_ALIGNMENT; }
  return OK;
}

// host-side validation of a buffer list -> OK and the block count, or the error
static int check_buffers(const char* who, const avmoe_opt_buffer* buffers, int32_t n_buffers, int64_t* n_blocks) {
  if (n_buffers < 0) { set_last_error("%s: negative buffer count %d", who, (int)n_buffers); return ERR_BAD_ARG; }
  if (n_buffers > 0 && !buffers) { set_last_error("%s: buffers is NULL", who); return ERR_BAD_ARG; }
  int64_t nb = 0;
  for (int32_t i = 0; i < n_buffers; ++i) {
    const avmoe_opt_buffer& r = buffers[i];
    if (r.n < 0) { set_last_error("%s: buffer %d has negative length %lld", who, (int)i, (long long)r.n); return ERR_BAD_ARG; }
    if (!r.buffer || !r.shadow) { set_last_error("%s: buffer %d has a NULL pointer", who, (int)i); return ERR_BAD_ARG; }
    if (((uintptr_t)r.buffer & 3u) != 0) { set_last_error("%s: buffer %d is not 4-byte aligned", who, (int)i); return ERR_ALIGNMENT; }
    if (((uintptr_t)r.shadow & 15u) != 0) { set_last_error("%s: the shadow of buffer %d is not 16-byte aligned", who, (int)i); return ERR_ALIGNMENT; }
    if (r.n > ((int64_t)INT32_MAX - 1) * OPT_BLOCK) { set_last_error("%s: buffer %d is too long", who, (int)i); return ERR_UNSUPPORTED; }
    nb += range_blocks(r.n);
  }
  if (nb > (int64_t)INT32_MAX) { set_last_error("%s: more than 2^31 blocks", who); return ERR_UNSUPPORTED; }
  *n_blocks = nb;
  return OK;
}

static size_t buffer_table_bytes_of(int32_t n_buffers, int64_t n_blocks) {
  return round16(sizeof(OptHeader) + (size_t)n_buffers * sizeof(avmoe_opt_buffer) + (size_t)n_blocks * sizeof(OptBlock));
}

// the state block first: a misaligned one is a bad argument whatever the table's alignment
static int check_launch_args(const char* who, const void* table, int32_t n_ranges, int64_t n_blocks, const void* state, float beta1, float beta2) {
  if (!state) { set_last_error("%s: NULL state", who); return ERR_BAD_ARG; }
  if (((uintptr_t)state & 15u) != 0) { set_last_error("%s: the state block must be 16-byte aligned", who); return ERR_BAD_ARG; }
  AVMOE_TRY(check_table_args(who, table, n_ranges, n_blocks));
  if (!(beta1 >= 0.f && beta1 < 1.f) || !(beta2 >= 0.f && beta2 < 1.f)) { set_last_error("%s: betas must be in [0, 1)", who); return ERR_BAD_ARG; }
  return OK;
}

// host-side validation of a schedule: everything the finalize kernel divides by or raises to a power
static int check_schedule(const char* who, const avmoe_opt_schedule* s) {
  if (!s) { set_last_error("%s: AVMOE_OPT_LR_SCHEDULE without a schedule", who); return ERR_BAD_ARG; }
  if (s->warmup_steps < 0 || s->total_steps < 0 || s->step_size < 0) { set_last_error("%s: negative warmup_steps / total_steps / step_size", who); return ERR_BAD_ARG; }
  if (!(s->warmup_start >= 0.f && s->warmup_start <= 1.f) || !(s->min_factor >= 0.f && s->min_factor <= 1.f)) {
    set_last_error("%s: warmup_start and min_factor must be in [0, 1]", who); return ERR_BAD_ARG;
  }
  if (!(s->gamma > 0.f && s->gamma <= 1.f)) { set_last_error("%s: gamma must be in (0, 1]", who); return ERR_BAD_ARG; }
  switch (s->decay_kind) {
    case AVMOE_SCHED_NONE: break;
    case AVMOE_SCHED_COSINE: case AVMOE_SCHED_LINEAR:
      if (s->total_steps <= s->warmup_steps) { set_last_error("%s: total_steps must be larger than warmup_steps for a cosine / linear decay", who); return ERR_BAD_ARG; }
      break;
    case AVMOE_SCHED_STEP:
      if (s->step_size <= 0) { set_last_error("%s: step_size must be positive for a step decay", who); return ERR_BAD_ARG; }
      break;
    default: set_last_error("%s: unknown decay_kind %d", who, (int)s->decay_kind); return ERR_BAD_ARG;
  }
  return OK;
}

// host-side validation of the average's constants and of the shadow pointer array (DEVICE memory: its entries are checked by the kernels)
static int check_ema(const char* who, const avmoe_opt_ema* e) {
  if (!e) { set_last_error("%s: AVMOE_OPT_EMA without its constants", who); return ERR_BAD_ARG; }
  if (!(e->decay >= 0.f && e->decay < 1.f)) { set_last_error("%s: the average's decay must be in [0, 1)", who); return ERR_BAD_ARG; }
  if (!(e->warmup >= 1.f) || std::isinf(e->warmup)) { set_last_error("%s: the average's warmup must be >= 1 and finite", who); return ERR_BAD_ARG; }
  return OK;
}
// host-side validation of the halves of avmoe_opt_swa that the flags switch on
static int check_swa(const char* who, const avmoe_opt_swa* w, bool average, bool anneal) {
  if (!w) { set_last_error("%s: AVMOE_OPT_SWA / AVMOE_OPT_SWA_LR without avmoe_opt_swa", who); return ERR_BAD_ARG; }
  if (average) {
    if (w->start < 1) { set_last_error("%s: avmoe_opt_swa.start must be >= 1, not %lld", who, (long long)w->start); return ERR_BAD_ARG; }
    if (w->freq < 1) { set_last_error("%s: avmoe_opt_swa.freq must be >= 1, not %d", who, (int)w->freq); return ERR_BAD_ARG; }
  }
  if (anneal) {
    if (w->lr_start < 0) { set_last_error("%s: avmoe_opt_swa.lr_start must be >= 0, not %lld", who, (long long)w->lr_start); return ERR_BAD_ARG; }
    if (w->anneal_steps < 0) { set_last_error("%s: avmoe_opt_swa.anneal_steps must be >= 0, not %d", who, (int)w->anneal_steps); return ERR_BAD_ARG; }
    if (!(w->lr_factor >= 0.f && w->lr_factor <= 1.f)) { set_last_error("%s: avmoe_opt_swa.lr_factor must be in [0, 1]", who); return ERR_BAD_ARG; }
    if (w->anneal_kind != AVMOE_SWA_ANNEAL_COS && w->anneal_kind != AVMOE_SWA_ANNEAL_LINEAR) {
      set_last_error("%s: unknown avmoe_opt_swa.anneal_kind %d", who, (int)w->anneal_kind); return ERR_BAD_ARG;
    }
  }
  return OK;
}
static int check_shadows(const char* who, float* const* shadows) {
  if (!shadows) { set_last_error("%s: the shadow pointer array is NULL", who); return ERR_BAD_ARG; }
  if (((uintptr_t)shadows & 7u) != 0) { set_last_error("%s: the shadow pointer array must be 8-byte aligned", who); return ERR_ALIGNMENT; }
  return OK;
}

static int check_hold(const char* who, float* const* hold) {
  if (!hold) { set_last_error("%s: the hold pointer array is NULL", who); return ERR_BAD_ARG; }
  if (((uintptr_t)hold & 7u) != 0) { set_last_error("%s: the hold pointer array must be 8-byte aligned", who); return ERR_ALIGNMENT; }
  return OK;
}

constexpr int32_t OPT_FLAGS = AVMOE_OPT_CLIP | AVMOE_OPT_SKIP_NONFINITE | AVMOE_OPT_DECOUPLED_DECAY;
constexpr int OPT_REPORT_MAX_GRID = 1024;        // blocks of 4 waves: more ranges than 4096 take a second round

// avmoe_opt_grad_norm (sched == NULL, ema == NULL), avmoe_opt_grad_norm_sched (ema == NULL), avmoe_opt_grad_norm_ema (report == NULL) and
// avmoe_opt_grad_norm_report (swa == NULL), avmoe_opt_grad_norm_swa: the same checks and the same norm launch, then the finalize kernel the flags
// ask for, then the per-range norms.  AVMOE_OPT_SWA_LR takes the SCHED instantiation and AVMOE_OPT_SWA the EMA one.
static int grad_norm(const char* who, const void* table, int32_t n_ranges, int64_t n_blocks, double* partials, avmoe_opt_state* state, float grad_scale,
                     float max_norm, int32_t flags, int32_t known_flags, float beta1, float beta2, const avmoe_opt_schedule* sched,
                     const avmoe_opt_ema* ema, void* report, const avmoe_opt_swa* swa, void* stream) {
  AVMOE_TRY(check_launch_args(who, table, n_ranges, n_blocks, state, beta1, beta2));
  const bool clip = (flags & AVMOE_OPT_CLIP) != 0, skip = (flags & AVMOE_OPT_SKIP_NONFINITE) != 0;
  const bool with_sched = (flags & AVMOE_OPT_LR_SCHEDULE) != 0, with_ema = (flags & AVMOE_OPT_EMA) != 0;
  const bool with_report = (flags & AVMOE_OPT_REPORT) != 0;
  const bool with_swa = (flags & AVMOE_OPT_SWA) != 0, with_swa_lr = (flags & AVMOE_OPT_SWA_LR) != 0;
  if ((flags & ~known_flags) != 0) { set_last_error("%s: unknown flag", who); return ERR_BAD_ARG; }
  if (clip && !(max_norm >= 0.f)) { set_last_error("%s: max_norm must be >= 0 and not NaN", who); return ERR_BAD_ARG; }
  if (!(grad_scale == grad_scale)) { set_last_error("%s: grad_scale is NaN", who); return ERR_BAD_ARG; }
  if (with_sched) AVMOE_TRY(check_schedule(who, sched));
  if (with_ema) AVMOE_TRY(check_ema(who, ema));
  avmoe_opt_swa w{};                                     // the kernel's copy: the half that is off as swa_averages / swa_anneals read it
  w.lr_start = -1;
  if (with_swa || with_swa_lr) {
    AVMOE_TRY(check_swa(who, swa, with_swa, with_swa_lr));
    if (with_swa && with_ema) { set_last_error("%s: AVMOE_OPT_SWA and AVMOE_OPT_EMA are alternatives: one average, one decay word", who); return ERR_BAD_ARG; }
    if (with_swa) { w.start = swa->start; w.freq = swa->freq; }
    if (with_swa_lr) { w.lr_start = swa->lr_start; w.anneal_steps = swa->anneal_steps; w.lr_factor = swa->lr_factor; w.anneal_kind = swa->anneal_kind; }
  }
  if (with_report) {
    if (!report) { set_last_error("%s: AVMOE_OPT_REPORT without a report buffer", who); return ERR_BAD_ARG; }
    if (((uintptr_t)report & 15u) != 0) { set_last_error("%s: the report buffer must be 16-byte aligned", who); return ERR_ALIGNMENT; }
  }
  avmoe_opt_report_header* rep = with_report ? (avmoe_opt_report_header*)report : nullptr;
  const bool norm = (clip || skip || with_report) && n_blocks > 0;
  if (norm) {
    if (!partials) { set_last_error("%s: partials is NULL", who); return ERR_BAD_ARG; }
    if (((uintptr_t)partials & 7u) != 0) { set_last_error("%s: partials must be 8-byte aligned", who); return ERR_ALIGNMENT; }
    hipLaunchKernelGGL(kk_opt_sqsum, dim3((unsigned)n_blocks), dim3(256), 0, (hipStream_t)stream, table, partials, grad_scale);
    AVMOE_CHECK_LAUNCH("opt_sqsum");
  }
  hipLaunchKernelGGL(OPT_FINALIZE[(int)(with_sched || with_swa_lr) | (int)(with_ema || with_swa) << 1], dim3(1), dim3(256), 0, (hipStream_t)stream, (const double*)partials,
                     norm ? (long)n_blocks : 0L, state, max_norm, (int)clip, (int)skip, beta1, beta2, with_sched ? *sched : avmoe_opt_schedule{},
                     with_ema ? *ema : avmoe_opt_ema{}, rep, (int)n_ranges, w);
  AVMOE_CHECK_LAUNCH("opt_finalize");
  if (rep && n_ranges > 0) {
    const int grid = (int)std::min<int64_t>(((int64_t)n_ranges + 3) / 4, OPT_REPORT_MAX_GRID);
    hipLaunchKernelGGL(kk_opt_range_norms, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, table, (const double*)partials, (int)n_ranges,
                       (long)n_blocks, rep);
    AVMOE_CHECK_LAUNCH("opt_range_norms");
  }
  return OK;
}

// what every update entry point refuses, in one order: adam_step below, avmoe_opt_lamb_step, avmoe_opt_prodigy_step and (opt_muon.hip)
// avmoe_opt_muon_step
int check_step_args(const char* who, const void* table, int32_t n_ranges, int64_t n_blocks, const avmoe_opt_state* state, float beta1,
                           float beta2, float eps, float grad_scale, int32_t flags, int32_t known_flags, float* const* shadows, bool with_hold,
                           float* const* hold) {
  AVMOE_TRY(check_launch_args(who, table, n_ranges, n_blocks, state, beta1, beta2));
  if ((flags & ~known_flags) != 0) { set_last_error("%s: unknown flag", who); return ERR_BAD_ARG; }
  if (!(eps >= 0.f) || !(grad_scale == grad_scale)) { set_last_error("%s: eps must be >= 0, grad_scale not NaN", who); return ERR_BAD_ARG; }
  if ((flags & AVMOE_OPT_EMA) != 0) AVMOE_TRY(check_shadows(who, shadows));
  if (with_hold) AVMOE_TRY(check_hold(who, hold));
  return OK;
}

// avmoe_opt_adam_step (shadows == NULL, the flag unknown), avmoe_opt_adam_step_ema and avmoe_opt_adam_step_sam (with_hold: the HOLD
// instantiations): the same checks, then the update kernel the flags ask for
static int adam_step(const char* who, const void* table, int32_t n_ranges, int64_t n_blocks, const avmoe_opt_state* state, float beta1, float beta2,
                     float eps, float grad_scale, int32_t flags, int32_t known_flags, float* const* shadows, bool with_hold, float* const* hold,
                     void* stream) {
  AVMOE_TRY(check_step_args(who, table, n_ranges, n_blocks, state, beta1, beta2, eps, grad_scale, flags, known_flags, shadows, with_hold, hold));
  const bool dec = (flags & AVMOE_OPT_DECOUPLED_DECAY) != 0, sched = (flags & AVMOE_OPT_LR_SCHEDULE) != 0, ema = (flags & AVMOE_OPT_EMA) != 0;
  if (n_blocks == 0) return OK;
  hipLaunchKernelGGL(OPT_ADAM[(int)dec | (int)sched << 1 | (int)ema << 2 | (int)with_hold << 3], dim3((unsigned)n_blocks), dim3(256), 0,
                     (hipStream_t)stream, table, state, beta1, beta2, eps, grad_scale, shadows, (int)n_ranges, with_hold ? hold : nullptr);
  AVMOE_CHECK_LAUNCH("opt_adam");
  return OK;
}

}  // namespace avmoe

using namespace avmoe;

extern "C" {

size_t avmoe_opt_workspace_bytes(const avmoe_opt_range* ranges, int32_t n_ranges, avmoe_opt_layout* layout) {
  int64_t nb = 0;
  if (check_ranges("avmoe_opt_workspace_bytes", ranges, n_ranges, &nb) != OK) return 0;
  avmoe_opt_layout l;
  l.state_bytes = sizeof(avmoe_opt_state);
  l.table_bytes = table_bytes_of(n_ranges, nb);
  l.partial_bytes = round16((size_t)(nb > 0 ? nb : 1) * sizeof(double));
  l.n_blocks = nb;
  if (layout) *layout = l;
  return l.state_bytes + l.table_bytes + l.partial_bytes;
}

int avmoe_opt_table_build(const avmoe_opt_range* ranges, int32_t n_ranges, void* image, size_t image_bytes) {
  int64_t nb = 0;
  AVMOE_TRY(check_ranges("avmoe_opt_table_build", ranges, n_ranges, &nb));
  if (!image) { set_last_error("avmoe_opt_table_build: image is NULL"); return ERR_BAD_ARG; }
  const size_t need = table_bytes_of(n_ranges, nb);
  if (image_bytes < need) { set_last_error("avmoe_opt_table_build: image of %zu bytes, %zu needed", image_bytes, need); return ERR_WORKSPACE; }
  char* p = (char*)image;
  memset(p, 0, need);
  OptHeader h{OPT_MAGIC, n_ranges, nb};
  memcpy(p, &h, sizeof h);
  if (n_ranges > 0) memcpy(p + sizeof h, ranges, (size_t)n_ranges * sizeof(avmoe_opt_range));
  OptBlock* bm = (OptBlock*)(p + sizeof h + (size_t)n_ranges * sizeof(avmoe_opt_range));
  for (int32_t i = 0; i < n_ranges; ++i)
    for (long b = 0, e = range_blocks(ranges[i].n); b < e; ++b) *bm++ = OptBlock{i, (int32_t)b};
  return OK;
}

int avmoe_opt_grad_norm(const void* table, int32_t n_ranges, int64_t n_blocks, double* partials, avmoe_opt_state* state, float grad_scale,
                        float max_norm, int32_t flags, float beta1, float beta2, void* stream) {
  return grad_norm("avmoe_opt_grad_norm", table, n_ranges, n_blocks, partials, state, grad_scale, max_norm, flags, OPT_FLAGS, beta1, beta2, nullptr, nullptr,
                   nullptr, nullptr, stream);
}

int avmoe_opt_grad_norm_sched(const void* table, int32_t n_ranges, int64_t n_blocks, double* partials, avmoe_opt_state* state, float grad_scale,
                              float max_norm, int32_t flags, float beta1, float beta2, void* stream, const avmoe_opt_schedule* sched) {
  return grad_norm("avmoe_opt_grad_norm_sched", table, n_ranges, n_blocks, partials, state, grad_scale, max_norm, flags, OPT_FLAGS | AVMOE_OPT_LR_SCHEDULE,
                   beta1, beta2, sched, nullptr, nullptr, nullptr, stream);
}

int avmoe_opt_adam_step(const void* table, int32_t n_ranges, int64_t n_blocks, const avmoe_opt_state* state, float beta1, float beta2, float eps,
                        float grad_scale, int32_t flags, void* stream) {
  return adam_step("avmoe_opt_adam_step", table, n_ranges, n_blocks, state, beta1, beta2, eps, grad_scale, flags, OPT_FLAGS | AVMOE_OPT_LR_SCHEDULE, nullptr,
                   false, nullptr, stream);
}

int avmoe_opt_grad_norm_ema(const void* table, int32_t n_ranges, int64_t n_blocks, double* partials, avmoe_opt_state* state, float grad_scale,
                            float max_norm, int32_t flags, float beta1, float beta2, void* stream, const avmoe_opt_schedule* sched,
                            const avmoe_opt_ema* ema) {
  return grad_norm("avmoe_opt_grad_norm_ema", table, n_ranges, n_blocks, partials, state, grad_scale, max_norm, flags,
                   OPT_FLAGS | AVMOE_OPT_LR_SCHEDULE | AVMOE_OPT_EMA, beta1, beta2, sched, ema, nullptr, nullptr, stream);
}

size_t avmoe_opt_report_bytes(int32_t n_ranges) {
  if (n_ranges < 0) { set_last_error("avmoe_opt_report_bytes: negative range count %d", (int)n_ranges); return 0; }
  return sizeof(avmoe_opt_report_header) + round16((size_t)n_ranges * sizeof(float));
}

int avmoe_opt_grad_norm_report(const void* table, int32_t n_ranges, int64_t n_blocks, double* partials, avmoe_opt_state* state, float grad_scale,
                               float max_norm, int32_t flags, float beta1, float beta2, void* stream, const avmoe_opt_schedule* sched,
                               const avmoe_opt_ema* ema, void* report) {
  return grad_norm("avmoe_opt_grad_norm_report", table, n_ranges, n_blocks, partials, state, grad_scale, max_norm, flags,
                   OPT_FLAGS | AVMOE_OPT_LR_SCHEDULE | AVMOE_OPT_EMA | AVMOE_OPT_REPORT, beta1, beta2, sched, ema, report, nullptr, stream);
}

int avmoe_opt_grad_norm_swa(const void* table, int32_t n_ranges, int64_t n_blocks, double* partials, avmoe_opt_state* state, float grad_scale,
                            float max_norm, int32_t flags, float beta1, float beta2, void* stream, const avmoe_opt_schedule* sched,
                            const avmoe_opt_ema* ema, void* report, const avmoe_opt_swa* swa) {
  return grad_norm("avmoe_opt_grad_norm_swa", table, n_ranges, n_blocks, partials, state, grad_scale, max_norm, flags,
                   OPT_FLAGS | AVMOE_OPT_LR_SCHEDULE | AVMOE_OPT_EMA | AVMOE_OPT_REPORT | AVMOE_OPT_SWA | AVMOE_OPT_SWA_LR, beta1, beta2, sched, ema, report,
                   swa, stream);
}

int avmoe_opt_adam_step_ema(const void* table, int32_t n_ranges, int64_t n_blocks, const avmoe_opt_state* state, float beta1, float beta2, float eps,
                            float grad_scale, int32_t flags, void* stream, float* const* shadows) {
  return adam_step("avmoe_opt_adam_step_ema", table, n_ranges, n_blocks, state, beta1, beta2, eps, grad_scale, flags,
                   OPT_FLAGS | AVMOE_OPT_LR_SCHEDULE | AVMOE_OPT_EMA, shadows, false, nullptr, stream);
}

int avmoe_opt_sam_perturb(const void* table, int32_t n_ranges, int64_t n_blocks, double* partials, avmoe_opt_sam_state* sam, float grad_scale, float rho,
                          int32_t adaptive, float* const* hold, void* stream) {
  const char* who = "avmoe_opt_sam_perturb";
  if (!sam) { set_last_error("%s: NULL sam block", who); return ERR_BAD_ARG; }
  if (((uintptr_t)sam & 15u) != 0) { set_last_error("%s: the sam block must be 16-byte aligned", who); return ERR_BAD_ARG; }
  AVMOE_TRY(check_table_args(who, table, n_ranges, n_blocks));
  if (!(rho >= 0.f) || std::isinf(rho)) { set_last_error("%s: rho must be >= 0 and finite", who); return ERR_BAD_ARG; }
  if (!(grad_scale == grad_scale)) { set_last_error("%s: grad_scale is NaN", who); return ERR_BAD_ARG; }
  if (adaptive != 0 && adaptive != 1) { set_last_error("%s: adaptive must be 0 or 1, not %d", who, (int)adaptive); return ERR_BAD_ARG; }
  AVMOE_TRY(check_hold(who, hold));
  if (n_blocks > 0) {
    if (!partials) { set_last_error("%s: partials is NULL", who); return ERR_BAD_ARG; }
    if (((uintptr_t)partials & 7u) != 0) { set_last_error("%s: partials must be 8-byte aligned", who); return ERR_ALIGNMENT; }
    hipLaunchKernelGGL(adaptive ? kk_opt_sqsum_adaptive : kk_opt_sqsum, dim3((unsigned)n_blocks), dim3(256), 0, (hipStream_t)stream, table, partials,
                       grad_scale);
    AVMOE_CHECK_LAUNCH("opt_sqsum");
  }
  hipLaunchKernelGGL(kk_opt_sam_finalize, dim3(1), dim3(256), 0, (hipStream_t)stream, (const double*)partials, (long)n_blocks, sam, rho);
  AVMOE_CHECK_LAUNCH("opt_sam_finalize");
  if (n_blocks == 0) return OK;
  hipLaunchKernelGGL(adaptive ? kk_opt_sam_perturb<true> : kk_opt_sam_perturb<false>, dim3((unsigned)n_blocks), dim3(256), 0, (hipStream_t)stream, table,
                     (const avmoe_opt_sam_state*)sam, grad_scale, hold, (int)n_ranges);
  AVMOE_CHECK_LAUNCH("opt_sam_perturb");
  return OK;
}

int avmoe_opt_adam_step_sam(const void* table, int32_t n_ranges, int64_t n_blocks, const avmoe_opt_state* state, float beta1, float beta2, float eps,
                            float grad_scale, int32_t flags, void* stream, float* const* shadows, float* const* hold) {
  return adam_step("avmoe_opt_adam_step_sam", table, n_ranges, n_blocks, state, beta1, beta2, eps, grad_scale, flags,
                   OPT_FLAGS | AVMOE_OPT_LR_SCHEDULE | AVMOE_OPT_EMA, shadows, true, hold, stream);
}

size_t avmoe_opt_lamb_bytes(int32_t n_ranges, int64_t n_blocks, avmoe_opt_lamb_layout* layout) {
  if (n_ranges < 0) { set_last_error("avmoe_opt_lamb_bytes: negative range count %d", (int)n_ranges); return 0; }
  if (n_blocks < 0 || n_blocks > (int64_t)INT32_MAX) { set_last_error("avmoe_opt_lamb_bytes: bad block count %lld", (long long)n_blocks); return 0; }
  avmoe_opt_lamb_layout l;
  l.workspace_bytes = round16((size_t)(n_blocks > 0 ? n_blocks : 1) * 2 * sizeof(double));
  l.report_bytes = sizeof(avmoe_opt_lamb_header) + round16((size_t)n_ranges * 3 * sizeof(float));
  if (layout) *layout = l;
  return l.workspace_bytes + l.report_bytes;
}

int avmoe_opt_lamb_step(const void* table, int32_t n_ranges, int64_t n_blocks, const avmoe_opt_state* state, float beta1, float beta2, float eps,
                        float grad_scale, int32_t flags, void* stream, float* const* shadows, float* const* hold, const float* limits,
                        double* workspace, void* report) {
  const char* who = "avmoe_opt_lamb_step";
  const bool with_hold = hold != nullptr;
  AVMOE_TRY(check_step_args(who, table, n_ranges, n_blocks, state, beta1, beta2, eps, grad_scale, flags, OPT_FLAGS | AVMOE_OPT_LR_SCHEDULE | AVMOE_OPT_EMA,
                            shadows, with_hold, hold));
  if (!limits) { set_last_error("%s: the limits array is NULL", who); return ERR_BAD_ARG; }
  if (!workspace) { set_last_error("%s: the workspace is NULL", who); return ERR_BAD_ARG; }
  if (!report) { set_last_error("%s: the trust report buffer is NULL", who); return ERR_BAD_ARG; }
  if (((uintptr_t)limits & 3u) != 0) { set_last_error("%s: the limits array must be 4-byte aligned", who); return ERR_ALIGNMENT; }
  if (((uintptr_t)workspace & 7u) != 0) { set_last_error("%s: the workspace must be 8-byte aligned", who); return ERR_ALIGNMENT; }
  if (((uintptr_t)report & 15u) != 0) { set_last_error("%s: the trust report buffer must be 16-byte aligned", who); return ERR_ALIGNMENT; }
  const bool dec = (flags & AVMOE_OPT_DECOUPLED_DECAY) != 0, sched = (flags & AVMOE_OPT_LR_SCHEDULE) != 0, ema = (flags & AVMOE_OPT_EMA) != 0;
  avmoe_opt_lamb_header* rep = (avmoe_opt_lamb_header*)report;
  if (n_blocks > 0) {
    hipLaunchKernelGGL(OPT_LAMB_MOMENTS[(int)dec | (int)with_hold << 1], dim3((unsigned)n_blocks), dim3(256), 0, (hipStream_t)stream, table, state,
                       beta1, beta2, eps, grad_scale, ema ? shadows : nullptr, hold, (int)n_ranges, workspace);
    AVMOE_CHECK_LAUNCH("opt_lamb_moments");
  }
  if (n_ranges > 0) {
    const int grid = (int)std::min<int64_t>(((int64_t)n_ranges + 3) / 4, OPT_REPORT_MAX_GRID);
    hipLaunchKernelGGL(kk_opt_lamb_ratio, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, table, (const double*)workspace, (int)n_ranges,
                       (long)n_blocks, limits, state, rep);
    AVMOE_CHECK_LAUNCH("opt_lamb_ratio");
  }
  if (n_blocks > 0) {
    hipLaunchKernelGGL(OPT_LAMB_APPLY[(int)dec | (int)sched << 1 | (int)ema << 2 | (int)with_hold << 3], dim3((unsigned)n_blocks), dim3(256), 0,
                       (hipStream_t)stream, table, state, eps, ema ? shadows : nullptr, hold, (int)n_ranges, (const avmoe_opt_lamb_header*)rep);
    AVMOE_CHECK_LAUNCH("opt_lamb_apply");
  }
  return OK;
}

size_t avmoe_opt_prodigy_bytes(int64_t n_blocks, avmoe_opt_prodigy_layout* layout) {
  if (n_blocks < 0 || n_blocks > (int64_t)INT32_MAX) { set_last_error("avmoe_opt_prodigy_bytes: bad block count %lld", (long long)n_blocks); return 0; }
  avmoe_opt_prodigy_layout l;
  l.workspace_bytes = round16((size_t)(n_blocks > 0 ? n_blocks : 1) * 2 * sizeof(double));
  l.block_bytes = sizeof(avmoe_opt_prodigy_state);
  if (layout) *layout = l;
  return l.workspace_bytes + l.block_bytes;
}

int avmoe_opt_prodigy_step(const void* table, int32_t n_ranges, int64_t n_blocks, const avmoe_opt_state* state, float beta1, float beta2, float eps,
                           float grad_scale, int32_t flags, void* stream, float* const* shadows, float* const* hold, float* const* x0,
                           float* const* s, const avmoe_opt_prodigy* consts, avmoe_opt_prodigy_state* block, double* workspace) {
  const char* who = "avmoe_opt_prodigy_step";
  const bool with_hold = hold != nullptr;
  AVMOE_TRY(check_step_args(who, table, n_ranges, n_blocks, state, beta1, beta2, eps, grad_scale, flags, OPT_FLAGS | AVMOE_OPT_LR_SCHEDULE | AVMOE_OPT_EMA,
                            shadows, with_hold, hold));
  if (!x0 || !s) { set_last_error("%s: the x0 / s pointer array is NULL", who); return ERR_BAD_ARG; }
  if (!consts) { set_last_error("%s: the constants are NULL", who); return ERR_BAD_ARG; }
  if (!block) { set_last_error("%s: the Prodigy block is NULL", who); return ERR_BAD_ARG; }
  if (!workspace) { set_last_error("%s: the workspace is NULL", who); return ERR_BAD_ARG; }
  if (!(consts->d0 > 0.f) || std::isinf(consts->d0)) { set_last_error("%s: d0 must be a finite number > 0", who); return ERR_BAD_ARG; }
  if (!(consts->d_coef > 0.f) || std::isinf(consts->d_coef)) { set_last_error("%s: d_coef must be a finite number > 0", who); return ERR_BAD_ARG; }
  if (!(consts->growth == 0.f || consts->growth >= 1.f) || std::isinf(consts->growth)) {
    set_last_error("%s: growth must be 0 (none) or a finite number >= 1", who); return ERR_BAD_ARG;
  }
  if (consts->safeguard_warmup != 0 && consts->safeguard_warmup != 1) {
    set_last_error("%s: safeguard_warmup must be 0 or 1, not %d", who, (int)consts->safeguard_warmup); return ERR_BAD_ARG;
  }
  if ((((uintptr_t)x0 | (uintptr_t)s) & 7u) != 0) { set_last_error("%s: the x0 / s pointer arrays must be 8-byte aligned", who); return ERR_ALIGNMENT; }
  if (((uintptr_t)block & 15u) != 0) { set_last_error("%s: the Prodigy block must be 16-byte aligned", who); return ERR_ALIGNMENT; }
  if (((uintptr_t)workspace & 7u) != 0) { set_last_error("%s: the workspace must be 8-byte aligned", who); return ERR_ALIGNMENT; }
  const bool dec = (flags & AVMOE_OPT_DECOUPLED_DECAY) != 0, sched = (flags & AVMOE_OPT_LR_SCHEDULE) != 0, ema = (flags & AVMOE_OPT_EMA) != 0;
  const float beta3 = (float)sqrt((double)beta2);
  if (n_blocks > 0) {
    hipLaunchKernelGGL(OPT_PRODIGY[(int)dec | (int)sched << 1 | (int)ema << 2 | (int)with_hold << 3], dim3((unsigned)n_blocks), dim3(256), 0,
                       (hipStream_t)stream, table, state, beta1, beta2, beta3, eps, grad_scale, ema ? shadows : nullptr, hold, x0, s, (int)n_ranges,
                       consts->d0, (int)consts->safeguard_warmup, (const avmoe_opt_prodigy_state*)block, workspace);
    AVMOE_CHECK_LAUNCH("opt_prodigy_update");
  }
  hipLaunchKernelGGL(kk_opt_prodigy_finalize, dim3(1), dim3(256), 0, (hipStream_t)stream, table, (int)n_ranges, (long)n_blocks,
                     (const double*)workspace, state, block, beta3, consts->d_coef, consts->growth);
  AVMOE_CHECK_LAUNCH("opt_prodigy_finalize");
  return OK;
}

int avmoe_opt_swap_ema(const void* table, int32_t n_ranges, int64_t n_blocks, float* const* shadows, void* stream) {
  const char* who = "avmoe_opt_swap_ema";
  AVMOE_TRY(check_table_args(who, table, n_ranges, n_blocks));
  AVMOE_TRY(check_shadows(who, shadows));
  if (n_blocks == 0) return OK;
  hipLaunchKernelGGL(kk_opt_swap, dim3((unsigned)n_blocks), dim3(256), 0, (hipStream_t)stream, table, shadows, (int)n_ranges);
  AVMOE_CHECK_LAUNCH("opt_swap");
  return OK;
}

size_t avmoe_opt_buffer_table_bytes(const avmoe_opt_buffer* buffers, int32_t n_buffers, int64_t* n_blocks) {
  int64_t nb = 0;
  if (check_buffers("avmoe_opt_buffer_table_bytes", buffers, n_buffers, &nb) != OK) return 0;
  if (n_blocks) *n_blocks = nb;
  return buffer_table_bytes_of(n_buffers, nb);
}

int avmoe_opt_buffer_table_build(const avmoe_opt_buffer* buffers, int32_t n_buffers, void* image, size_t image_bytes) {
  int64_t nb = 0;
  AVMOE_TRY(check_buffers("avmoe_opt_buffer_table_build", buffers, n_buffers, &nb));
  if (!image) { set_last_error("avmoe_opt_buffer_table_build: image is NULL"); return ERR_BAD_ARG; }
  const size_t need = buffer_table_bytes_of(n_buffers, nb);
  if (image_bytes < need) { set_last_error("avmoe_opt_buffer_table_build: image of %zu bytes, %zu needed", image_bytes, need); return ERR_WORKSPACE; }
  char* p = (char*)image;
  memset(p, 0, need);
  OptHeader h{OPT_BUF_MAGIC, n_buffers, nb};
  memcpy(p, &h, sizeof h);
  if (n_buffers > 0) memcpy(p + sizeof h, buffers, (size_t)n_buffers * sizeof(avmoe_opt_buffer));
  char* bm = p + sizeof h + (size_t)n_buffers * sizeof(avmoe_opt_buffer);     // memcpy: the caller's image need not be aligned
  for (int32_t i = 0; i < n_buffers; ++i)
    for (long b = 0, e = range_blocks(buffers[i].n); b < e; ++b, bm += sizeof(OptBlock)) {
      const OptBlock ob{i, (int32_t)b};
      memcpy(bm, &ob, sizeof ob);
    }
  return OK;
}

int avmoe_opt_ema_buffers(const void* table, int32_t n_buffers, int64_t n_blocks, const avmoe_opt_state* state, void* stream) {
  const char* who = "avmoe_opt_ema_buffers";
  if (!state) { set_last_error("%s: NULL state", who); return ERR_BAD_ARG; }
  if (((uintptr_t)state & 15u) != 0) { set_last_error("%s: the state block must be 16-byte aligned", who); return ERR_BAD_ARG; }
  AVMOE_TRY(check_table_args(who, table, n_buffers, n_blocks));
  if (n_blocks == 0) return OK;
  hipLaunchKernelGGL(kk_opt_ema_buffers, dim3((unsigned)n_blocks), dim3(256), 0, (hipStream_t)stream, table, (int)n_buffers, (long)n_blocks, state);
  AVMOE_CHECK_LAUNCH("opt_ema_buffers");
  return OK;
}

int avmoe_opt_swap_buffers(const void* table, int32_t n_buffers, int64_t n_blocks, void* stream) {
  const char* who = "avmoe_opt_swap_buffers";
  AVMOE_TRY(check_table_args(who, table, n_buffers, n_blocks));
  if (n_blocks == 0) return OK;
  hipLaunchKernelGGL(kk_opt_swap_buffers, dim3((unsigned)n_blocks), dim3(256), 0, (hipStream_t)stream, table, (int)n_buffers, (long)n_blocks);
  AVMOE_CHECK_LAUNCH("opt_swap_buffers");
  return OK;
}

}  // extern "C"
