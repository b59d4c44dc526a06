// The update of the selection bias of aux-loss-free expert balancing (avmoe_router_bias_update, include/avmoe.h; Wang et al. 2024): after
// every optimizer step an expert that received more than its share of the routing slots has its bias lowered by a fixed rate, one that
// received less has it raised.  The bias enters the top-k SELECTION of the site calls only (avmoe_moe_forward_bias), which also add up
// the counts this kernel consumes.  No gradient, no loss term.
//   tot  = sum_e counts[i][e]                    (added in expert order)
//   d_e  = tot - E_i counts[i][e]                (> 0: expert e is below the mean count tot / E_i)
//   bias[i][e] += +rate (d_e > 0), -rate (d_e < 0), nothing (d_e == 0) ;  counts[i][e] = 0        -- a row with tot == 0 is left alone
// counts are sums of integers kept in fp32: tot and E_i counts[i][e] are exact below 2^24, i.e. up to 2^24 / 16 = 1 048 576 routing slots
// per site between two updates at E = 16; beyond that the SIGN of d_e can be wrong for near-balanced experts (the values stay finite).
// ONE launch for all sites of a model: one block (one wave) per site, lane e < E_i serves expert e; every lane parks its count in the LDS,
// a barrier, then each lane adds the row up in expert order itself -- no shuffle tree, no atomics, the same bits on every call.  Columns
// e >= E_i of both arrays are neither read nor written.  E comes from a device table and no host scalar changes between two calls: the
// launch is capturable.
#include "../../include/avmoe.h"
#include "common.h"
#include <hip/hip_runtime.h>
#include <cmath>

namespace avmoe {

namespace {

constexpr int ROW = AVMOE_MAX_EXPERTS;       // row length of bias / counts

__global__ void __launch_bounds__(64) kk_router_bias_update(float* bias, float* counts, const int* E_of, int n_sites, float rate) {
  __shared__ float s_c[ROW];
  const int i = blockIdx.x, e = threadIdx.x;
  if (i >= n_sites) return;                  // (uniform over the block)
  const int E = E_of[i];
  if (E < 1 || E > ROW) return;              // (uniform over the block) not a row of this table: skipped
  const bool on = e < E;
  const long at = (long)i * ROW + e;
  const float c = on ? counts[at] : 0.f;
  if (on) s_c[e] = c;
  __syncthreads();
  float tot = 0.f;
  for (int f = 0; f < E; ++f) tot += s_c[f];
  if (!on || tot == 0.f) return;
  const float d = tot - (float)E * c;        // integers: exact below 2^24 (a fused multiply-add is exact too)
  if (d > 0.f) bias[at] = bias[at] + rate;
  else if (d < 0.f) bias[at] = bias[at] - rate;
  counts[at] = 0.f;
}

}  // namespace

}  // namespace avmoe

extern "C" int avmoe_router_bias_update(float* bias, float* counts, const int32_t* E, int32_t n_sites, float rate, void* stream) {
  using namespace avmoe;
  if (!bias || !counts || !E) { set_last_error("avmoe_router_bias_update: null pointer"); return ERR_BAD_ARG; }
  if (n_sites < 1) { set_last_error("avmoe_router_bias_update: n_sites %d < 1", (int)n_sites); return ERR_BAD_ARG; }
  if (!(rate >= 0.f) || !std::isfinite(rate)) { set_last_error("avmoe_router_bias_update: rate %g is negative or not finite", (double)rate); return ERR_BAD_ARG; }
  hipLaunchKernelGGL(kk_router_bias_update, dim3((unsigned)n_sites), dim3(64), 0, (hipStream_t)stream, bias, counts, (const int*)E, (int)n_sites, rate);
  AVMOE_CHECK_LAUNCH("router_bias_update");
  return OK;
}
