// Development: prints the per-expert tables of the bottleneck-space passes (csrc/pass.h: PassExperts) for a handful of descriptors, from the
// parameter pointers a pass receives (unit gates and merged-group copies applied, as moe_forward / moe_backward do).  The check of
// pass_experts(): every family's kernels get their tables from it, so what it prints is what reaches them.
//
//   hipcc -std=c++17 -O1 tests/dev/pass_experts_dump.cpp -Lavmoe_amd/lib -lavmoe_hip -Wl,-rpath,$PWD/avmoe_amd/lib -o pass_experts_dump
//   (+ -fsanitize=address,undefined for the sanitizer run: the program and pass.h are instrumented, the library is not)
//
// No GPU: make_plan and the two pointer rewrites are host code, nothing is launched.  Pointers are made up and printed as offsets from
// their bases (prm + .., saved + ..).
#include <cstdio>
#include "../../avmoe_amd/csrc/pass.h"

namespace avmoe { avmoe_moe_ptrs with_unit_gates(const Plan& pl, const avmoe_moe_ptrs& prm, char* sv); }   // moe_forward.cpp
using namespace avmoe;

static char* const PRM = (char*)0x1000000;
static char* const SAVED = (char*)0x10000000;

static avmoe_moe_desc desc(int variant, int self_attn, int S, int N, int C, int M, int Cy, int E_m, int E_s, int d, int groups, int K, int bf16) {
  avmoe_moe_desc q = {};
  q.S = S; q.N = N; q.C = C; q.M = M; q.Cy = Cy; q.E_m = E_m; q.E_s = E_s; q.d = d; q.groups = groups; q.K = K;
  q.use_bn = q.use_gate = q.ln_before = q.ln_post = 1; q.variant = variant; q.self_attn = self_attn;
  q.dtype = bf16 ? AVMOE_BF16 : AVMOE_F32; q.training = 1; q.bn_eps = 1e-5f; q.ln_eps = 1e-5f; q.bn_momentum = 0.1f;
  return q;
}

static void ptr(const float* p) {
  const char* c = (const char*)p;
  if (!c) printf(" null");
  else if (c >= SAVED) printf(" saved+%ld", (long)(c - SAVED));
  else printf(" prm+%ld", (long)(c - PRM));
}

static int dump(const char* name, const avmoe_moe_desc& q) {
  Plan pl;
  if (make_plan(&q, &pl) != OK) { printf("%s: make_plan: %s\n", name, last_error()); return 1; }
  const Dims& d = pl.d;
  avmoe_moe_ptrs in = {};
  for (int e = 0; e < d.E; ++e) {                          // (entries beyond d.E stay NULL, as the facade leaves them)
    in.e[e].gate = (float*)(PRM + 256 * e); in.e[e].gate_lat = (float*)(PRM + 256 * e + 64);
    in.e[e].down_w = (float*)(PRM + 256 * e + 128); in.e[e].up_w = (float*)(PRM + 256 * e + 192);
  }
  avmoe_moe_ptrs prm = with_unit_gates(pl, in, SAVED);
  if (d.mg) prm = merged_params(pl, prm, SAVED);
  const PassCall c(pl, SAVED, nullptr, prm);
  const PassExperts& x = c.x;
  printf("%s: E=%d El=%d g=%d dgp=%d Kp=%d gen=%d mg=%d nxn=%d mha=%d nxr=%d NT=%d\n", name, d.E, d.El, d.g, d.dgp, d.Kp, d.gen, d.mg, d.nxn, d.mha, d.nxr, d.NT);
  for (int e = 0; e < d.E; ++e) {
    printf("  e=%2d relu=%d lat=%2d nxn=%d first_of_slot=%d sxr_off=%ld e_of_lat=%d gate", e, x.relu_of_e[e], x.lat_of_e[e], x.nxn_of_e[e], x.first_of_slot[e],
           x.sxr_off[e], x.e_of_lat[e]);
    ptr(x.gate.p[e]); printf(" glat"); ptr(x.glat.p[e]); printf("\n");
  }
  bool rest = true;                                        // what no kernel reads: zeros, as Dims has them beyond d.E
  for (int e = d.E; e < MAX_E; ++e)
    rest = rest && !x.relu_of_e[e] && !x.lat_of_e[e] && !x.nxn_of_e[e] && !x.first_of_slot[e] && !x.sxr_off[e] && !x.e_of_lat[e] && !x.gate.p[e] && !x.glat.p[e];
  printf("  e=%d..%d: %s\n", d.E, MAX_E - 1, rest ? "all zero / null" : "NOT all zero");
  if (!rest) return 1;
  return 0;
}

int main() {
  int bad = 0;
  bad |= dump("AVE 2 + 2, tuned shape, bf16", desc(AVMOE_VARIANT_AVE, AVMOE_SELF_ATTN_NONE, 20, 196, 768, 64, 768, 2, 2, 64, 2, 32, 1));
  bad |= dump("AVE 1 + 2 (three experts), bf16", desc(AVMOE_VARIANT_AVE, AVMOE_SELF_ATTN_NONE, 16, 180, 768, 64, 768, 1, 2, 64, 2, 32, 1));
  bad |= dump("AVVP 2 + 2 (the N x N experts share xr slot 0), bf16", desc(AVMOE_VARIANT_AVVP, AVMOE_SELF_ATTN_NONE, 8, 64, 768, 32, 768, 2, 2, 64, 2, 32, 1));
  bad |= dump("AVS v1 2 + 2 (one xr slot per unimodal expert, unit gates), fp32", desc(AVMOE_VARIANT_AVS, AVMOE_SELF_ATTN_MHA_V1, 5, 40, 128, 33, 128, 2, 2, 64, 2, 32, 0));
  bad |= dump("AVS v2 2 + 2 (every expert has latent tokens), fp32", desc(AVMOE_VARIANT_AVS, AVMOE_SELF_ATTN_LATENT_V2, 3, 40, 96, 33, 64, 2, 2, 32, 2, 8, 0));
  bad |= dump("AVS 4 + 4, K = 87, four groups (generalised kernels), fp32", desc(AVMOE_VARIANT_AVS, AVMOE_SELF_ATTN_NONE, 3, 49, 512, 64, 768, 4, 4, 128, 4, 87, 0));
  bad |= dump("AVE 2 + 2, four groups of 3 merged into one, fp32", desc(AVMOE_VARIANT_AVE, AVMOE_SELF_ATTN_NONE, 3, 50, 192, 40, 96, 2, 2, 12, 4, 9, 0));
  bad |= dump("AVS 2 + 2, three groups of 8 (any-shape kernels), fp32", desc(AVMOE_VARIANT_AVS, AVMOE_SELF_ATTN_NONE, 3, 64, 480, 40, 64, 2, 2, 24, 3, 8, 0));
  return bad;
}
