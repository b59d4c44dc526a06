// Schedule-free AdamW on the optimizer's range table (include/avmoe.h, avmoe_opt_sf_step): two launches in place of kk_opt_adam, behind
// the unchanged norm call of a step --
//   kk_opt_sf_weights                      one block, one thread: this step's weight c = w / weight_sum in the running average from the
//                                          counters the finalize launch has just left in the state block, into the 32-byte
//                                          avmoe_opt_sf_state; d = 1 - c also into state->ema_decay, for avmoe_opt_ema_buffers behind it
//   kk_opt_sf_update<DECOUPLED, SCHED, HOLD>   the table walk of kk_opt_adam (opt_work, opt_shadow, restore_quad) with sf_quad
//                                          (adam_elem.h): y = param, z = exp_avg, v = exp_avg_sq, x = the shadow -- five 4-byte streams
//                                          read (y, grad, z, v, x) and four written per element
// Plain bandwidth kernels: 16-byte loads and stores, no matrix pipe, no LDS, no floating-point atomics; a skipped step writes nothing
// (HOLD: param = hold and nothing else), and a launch that does not match its table's header touches nothing.
#include "../../include/avmoe.h"
#include "common.h"
#include "adam_elem.h"
#include "opt_table.h"
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>

namespace avmoe {

static_assert(sizeof(avmoe_opt_sf_state) == 32 && sizeof(avmoe_opt_sf) == 8, "schedule-free layout");

// One block; thread 0 alone works.  In double unless stated, contraction off (FlatAdam.sf_weights_next in avmoe_amd/flat_adam.py is the
// host's copy, in this operation order):
//     f_max = max(f_max, f) ;  w = pow(n, r) * pow(f_max, lr_power) ;  weight_sum += w
//     c = w / weight_sum   (0 where weight_sum is not > 0) ;  d = 1 - c ;  c and d each rounded once to fp32
// with n = applied_steps AFTER this step (the finalize launch has advanced it) and f = the state block's lr_factor under `sched`, else
// 1.  d is also copied into state->ema_decay.  A skipped step, or a launch that does not match its table's header, writes nothing.
__global__ void __launch_bounds__(64) kk_opt_sf_weights(const void* __restrict__ table, int n_ranges, long n_blocks, avmoe_opt_state* __restrict__ state,
                                                        avmoe_opt_sf_state* __restrict__ blk, float r, float lr_power, int sched) {
#pragma clang fp contract(off)
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  if (state->skip) return;
  const OptHeader h = *(const OptHeader*)table;
  if (h.magic != OPT_MAGIC || h.n_ranges != n_ranges || h.n_blocks != n_blocks) return;
  const double n = (double)state->applied_steps;
  const float f = sched ? state->lr_factor : 1.f;
  const float f_old = blk->f_max, f_max = f > f_old ? f : f_old;
  const double w = pow(n, (double)r) * pow((double)f_max, (double)lr_power);
  const double sum = blk->weight_sum + w;
  const double c = sum > 0.0 ? w / sum : 0.0;
  const float d = (float)(1.0 - c);
  blk->weight_sum = sum;
  blk->f_max = f_max;
  blk->c = (float)c;
  blk->d = d;
  state->ema_decay = d;
}

// SCHED: the range's rate times the state block's lr_factor.  xs[range] is the range's average x, hold[range] (HOLD) its unperturbed
// parameters under the rules of kk_opt_adam: every y is read from there and written to param; a skipped step writes param = hold and
// nothing else.  d is this step's, which kk_opt_sf_weights has just left in the block.
template <bool DECOUPLED, bool SCHED, bool HOLD>
__global__ void __launch_bounds__(256) kk_opt_sf_update(const void* __restrict__ table, const avmoe_opt_state* __restrict__ state, float b1, float b2,
                                                        float eps, float grad_scale, float* const* __restrict__ xs,
                                                        float* const* __restrict__ hold, int n_ranges,
                                                        const avmoe_opt_sf_state* __restrict__ blk) {
  const bool skip = state->skip != 0;
  if constexpr (!HOLD) {
    if (skip) return;                                     // a skipped step writes nothing
  }
  OptWork w;
  if (!opt_work(table, w) || w.n_ranges != n_ranges) return;
  float* x = opt_shadow(w, xs, n_ranges);
  if (!x) return;
  const avmoe_opt_range& r = w.r;
  const float* h = nullptr;
  if constexpr (HOLD) {
    h = opt_shadow(w, hold, n_ranges);
    if (!h) return;
    if (skip) { restore_quad(r.param, h, w.i0, (long)r.n); return; }
  }
  SfScal k;
  k.step = r.lr;
  if constexpr (SCHED) k.step *= state->lr_factor;
  k.d = blk->d;
  k.b1 = b1; k.b2 = b2; k.eps = eps; k.wd = r.weight_decay;
  k.bc2_sqrt = state->bc2_sqrt;
  k.gscale = grad_scale * state->clip_coef;               // one multiplier for the gradient, as in kk_opt_adam
  sf_quad<DECOUPLED, HOLD>(r.param, r.grad, r.exp_avg, r.exp_avg_sq, x, w.i0, (long)r.n, k, h);
}

using SfKernel = decltype(&kk_opt_sf_update<false, false, false>);
constexpr SfKernel OPT_SF[8] = {                          // [DECOUPLED | SCHED << 1 | HOLD << 2]
    kk_opt_sf_update<false, false, false>, kk_opt_sf_update<true, false, false>, kk_opt_sf_update<false, true, false>,
    kk_opt_sf_update<true, true, false>,   kk_opt_sf_update<false, false, true>, kk_opt_sf_update<true, false, true>,
    kk_opt_sf_update<false, true, true>,   kk_opt_sf_update<true, true, true>};

constexpr int32_t OPT_SF_FLAGS = AVMOE_OPT_CLIP | AVMOE_OPT_SKIP_NONFINITE | AVMOE_OPT_DECOUPLED_DECAY | AVMOE_OPT_LR_SCHEDULE;

}  // namespace avmoe

using namespace avmoe;

extern "C" {

int avmoe_opt_sf_step(const void* table, int32_t n_ranges, int64_t n_blocks, avmoe_opt_state* state, float beta1, float beta2, float eps,
                      float grad_scale, int32_t flags, void* stream, float* const* x, float* const* hold, const avmoe_opt_sf* consts,
                      avmoe_opt_sf_state* block) {
  const char* who = "avmoe_opt_sf_step";
  const bool with_hold = hold != nullptr;
  AVMOE_TRY(check_step_args(who, table, n_ranges, n_blocks, state, beta1, beta2, eps, grad_scale, flags, OPT_SF_FLAGS, nullptr, with_hold, hold));
  if (!x) { set_last_error("%s: the x pointer array is NULL", who); return ERR_BAD_ARG; }
  if (!consts) { set_last_error("%s: the constants are NULL", who); return ERR_BAD_ARG; }
  if (!block) { set_last_error("%s: the schedule-free block is NULL", who); return ERR_BAD_ARG; }
  if (!(consts->r >= 0.f) || std::isinf(consts->r)) { set_last_error("%s: r must be a finite number >= 0", who); return ERR_BAD_ARG; }
  if (!(consts->lr_power >= 0.f) || std::isinf(consts->lr_power)) { set_last_error("%s: lr_power must be a finite number >= 0", who); return ERR_BAD_ARG; }
  if (((uintptr_t)x & 7u) != 0) { set_last_error("%s: the x pointer array must be 8-byte aligned", who); return ERR_ALIGNMENT; }
  if (((uintptr_t)block & 15u) != 0) { set_last_error("%s: the schedule-free block must be 16-byte aligned", who); return ERR_ALIGNMENT; }
  const bool dec = (flags & AVMOE_OPT_DECOUPLED_DECAY) != 0, sched = (flags & AVMOE_OPT_LR_SCHEDULE) != 0;
  hipLaunchKernelGGL(kk_opt_sf_weights, dim3(1), dim3(64), 0, (hipStream_t)stream, table, (int)n_ranges, (long)n_blocks, state, block, consts->r,
                     consts->lr_power, (int)sched);
  AVMOE_CHECK_LAUNCH("opt_sf_weights");
  if (n_blocks == 0) return OK;
  hipLaunchKernelGGL(OPT_SF[(int)dec | (int)sched << 1 | (int)with_hold << 2], dim3((unsigned)n_blocks), dim3(256), 0, (hipStream_t)stream, table,
                     (const avmoe_opt_state*)state, beta1, beta2, eps, grad_scale, x, hold, (int)n_ranges, (const avmoe_opt_sf_state*)block);
  AVMOE_CHECK_LAUNCH("opt_sf_update");
  return OK;
}

}  // extern "C"
