// The draw of the mixture regularisers (avmoe_mix_drop_draw, include/avmoe.h): stochastic depth per frame and expert dropout per
// (frame, expert), as ONE (S, E) fp32 multiplier on the mixture weights that the site call consumes (avmoe_moe_forward_reg / _backward_reg:
// mix_scale).  The site body never draws, as with `noise` and `sa_keep`.
//   m[s, e] = a[s] b[s, e]      a[s] = 0 with probability p, else 1 / (1 - p)      b[s, e] = 0 with probability q, else 1 / (1 - q)
// Generator: Philox-4x32-10 (Salmon et al. 2011), key = the two halves of state.seed, counter = (calls low, calls high, s, e / 4); lane
// e % 4 of the result serves expert e.  The frame's own draw has counter word 3 = 0xFFFFFFFF (no expert group reaches it: E <= 16) and
// uses lane 0.  A uniform is (x >> 8) * 2^-24, exact in fp32; the pair / frame is dropped when u < q / u < p.
// The two kept scales are formed on the host, once, by IEEE fp32 division, and multiplied on the device: a kept value is exactly
// fl(fl(1 / (1 - p)) fl(1 / (1 - q))).
//
// The counter lives in the state block {uint64 seed, uint64 calls} on the device and the kernel advances it itself: no host scalar
// changes between two calls, so a captured launch draws a fresh multiplier on every replay.
// ONE block: every thread reads `calls` into a register first, a block barrier follows, and only then one thread stores calls + 1 (a plain
// C++ store from one lane).  Within one block the barrier orders every read before the store; a grid of several blocks would need a second
// launch for the increment (a block scheduled late could read the new value), and there is no work here to spread: S E / 4 generator calls
// of ~70 integer instructions each -- 256 work items at S = 64, E = 16 -- finish inside the launch latency of a second kernel.
// No loads depend on the lane: the state block is read at one uniform address, the rest is arithmetic, and the stores are masked by e < E.
#include "../../include/avmoe.h"
#include "common.h"
#include <hip/hip_runtime.h>

namespace avmoe {

namespace {

struct U4 { unsigned x, y, z, w; };

__device__ __forceinline__ U4 philox4x32_10(U4 c, unsigned k0, unsigned k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned hi0 = __umulhi(0xD2511F53u, c.x), lo0 = 0xD2511F53u * c.x;
    const unsigned hi1 = __umulhi(0xCD9E8D57u, c.z), lo1 = 0xCD9E8D57u * c.z;
    c = U4{hi1 ^ c.y ^ k0, lo1, hi0 ^ c.w ^ k1, lo0};
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  return c;
}
__device__ __forceinline__ float uniform24(unsigned x) { return (float)(x >> 8) * (1.f / 16777216.f); }

__global__ void __launch_bounds__(256) kk_mix_drop_draw(unsigned long long* state, int S, int E, float p, float q, float keep_a, float keep_b,
                                                        float* mix) {
  const unsigned long long seed = state[0], calls = state[1];      // read by every thread before the barrier below
  const unsigned k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32);
  const unsigned c0 = (unsigned)calls, c1 = (unsigned)(calls >> 32);
  const int G = (E + 3) / 4;
  const long items = (long)S * G;
  for (long i = threadIdx.x; i < items; i += 256) {
    const unsigned s = (unsigned)(i / G), g = (unsigned)(i % G);
    const U4 rb = philox4x32_10(U4{c0, c1, s, g}, k0, k1);
    const U4 ra = philox4x32_10(U4{c0, c1, s, 0xFFFFFFFFu}, k0, k1);
    const float a = uniform24(ra.x) < p ? 0.f : keep_a;
    const unsigned r[4] = {rb.x, rb.y, rb.z, rb.w};
    float* row = mix + (long)s * E;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int e = (int)g * 4 + j;
      const float b = uniform24(r[j]) < q ? 0.f : keep_b;
      if (e < E) row[e] = a * b;
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) state[1] = calls + 1;
}

}  // namespace

}  // namespace avmoe

extern "C" int avmoe_mix_drop_draw(void* state, int64_t S, int32_t E, float p, float q, float* mix_scale, void* stream) {
  using namespace avmoe;
  if (!state || !mix_scale) { set_last_error("avmoe_mix_drop_draw: null pointer"); return ERR_BAD_ARG; }
  if (S < 1 || S > 0x7fffffffLL || E < 1 || E > 16) { set_last_error("avmoe_mix_drop_draw: S %lld / E %d not served (S >= 1, 1 <= E <= 16)", (long long)S, (int)E); return ERR_BAD_ARG; }
  if (!(p >= 0.f && p < 1.f) || !(q >= 0.f && q < 1.f)) { set_last_error("avmoe_mix_drop_draw: p %g / q %g not in [0, 1)", (double)p, (double)q); return ERR_BAD_ARG; }
  const float keep_a = 1.f / (1.f - p), keep_b = 1.f / (1.f - q);
  hipLaunchKernelGGL(kk_mix_drop_draw, dim3(1), dim3(256), 0, (hipStream_t)stream, (unsigned long long*)state, (int)S, (int)E, p, q, keep_a, keep_b,
                     mix_scale);
  AVMOE_CHECK_LAUNCH("mix_drop_draw");
  return OK;
}
