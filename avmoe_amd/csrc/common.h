// Shared host-side helpers: status codes and the thread-local error message behind avmoe_last_error().
#pragma once
#include <hip/hip_runtime.h>
#include <atomic>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>

// Cache policy of the streaming kernels' direct global -> LDS loads: the `aux` argument of __builtin_amdgcn_global_load_lds (gfx950: 1 = sc0,
// 2 = nt, 16 = sc1).  2, the non-temporal hint: a tile that is read once is not kept in the L2 / Infinity Cache in place of lines somebody
// will come back to.  Measured on the tile loop of kk_hop1_yk rebuilt without its kernel (scripts/lds_stream_probe.hip, MI355X): with the
// loop's one small store per wave and tile (32-byte runs: the partly written lines now survive until their other parts arrive) 4.58 -> 5.08
// TB/s, without the store no difference (5.9 TB/s); sc0 alone: none.  Applied per kernel where the two-stream STEP gains (hop1_stream.hip: the
// Y streams, -1.1 %); the X-side kernels (tok_pair2 / dpost_pair / dx_stream3) measured neutral to +1 % with it and keep 0.
#ifndef AVMOE_LDS_AUX
#define AVMOE_LDS_AUX 2
#endif

namespace avmoe {

enum Status : int {
  OK = 0,
  ERR_BAD_ARG = -1,        // null pointer / inconsistent descriptor
  ERR_UNSUPPORTED = -2,    // valid request the library does not implement
  ERR_ALIGNMENT = -3,      // pointer / stride alignment contract violated
  ERR_WORKSPACE = -4,      // workspace too small
  ERR_LAUNCH = -5,         // HIP launch failure
};

void set_last_error(const char* fmt, ...);
const char* last_error();

#define AVMOE_CHECK_LAUNCH(what)                                                         \
  do {                                                                                   \
    hipError_t e__ = hipGetLastError();                                                  \
    if (e__ != hipSuccess) {                                                             \
      ::avmoe::set_last_error("%s: %s", what, hipGetErrorString(e__));                   \
      return ::avmoe::ERR_LAUNCH;                                                        \
    }                                                                                    \
  } while (0)

#define AVMOE_TRY(expr)                 \
  do {                                  \
    int s__ = (expr);                   \
    if (s__ != 0) return s__;           \
  } while (0)

// ---- the switch table: every form switch and development override of the library, in one struct, filled once per process (common.cpp) ----
// Test hooks: process state set through avmoe_test_hooks (include/avmoe.h) -- size thresholds of the streaming kernels lifted, frames per
// chunk of the AVVP N x N block; the environment variables AVMOE_TOKPAIR2_FORCE / AVMOE_DPAIR_FORCE / AVMOE_HOP1S_FORCE / AVMOE_KFS_FORCE /
// AVMOE_KFS_OFF / AVMOE_NXN_CHUNK seed them when the table is first asked for.
enum { HOOK_TOKPAIR2_FORCE = 1, HOOK_DPAIR_FORCE = 2, HOOK_HOP1S_FORCE = 4, HOOK_KFS_FORCE = 8, HOOK_KFS_OFF = 16 };
// Development switches (A/B toggles, sweep overrides) exist only in builds made with -DAVMOE_DEV (AVMOE_DEV_BUILD=1 python -m
// avmoe_amd.build): there each is read from the environment variable AVMOE_<NAME> ONCE, when the table is first asked for; in the
// product library each is a compile-time constant (its default), so every branch on one folds away.  Four environment variables are part
// of the product and read with plain getenv, once per process: AVMOE_PROF_SHAPES (profiler families per launch shape, prof.cpp),
// AVMOE_NO_SIDE / AVMOE_SIDE_MIN (helper streams inside a call: off / smallest site in token elements that forks, side.cpp, moe_plan.h),
// AVMOE_LIB (Python side).  No kernel choice depends on the environment at call time.
#ifndef AVMOE_LEAF2
#define AVMOE_LEAF2 26                   // (moe_run.h has the classes and the measurement)
#endif
// flags: set = the variable is present.  X(field, "AVMOE_<NAME>")
#define AVMOE_DEV_FLAGS(X)                                                                                                             \
  X(gemm_nostream, "AVMOE_GEMM_NOSTREAM")        /* launch_gemm: the tiled engine only, neither streaming form (A/B) */                \
  X(gemm_nofold, "AVMOE_GEMM_NOFOLD")            /* launch_gemm: no batch fold */                                                      \
  X(no_frame_gemm, "AVMOE_NO_FRAME_GEMM")        /* launch_gemm_frames serves nothing */                                               \
  X(no_tokpair, "AVMOE_NO_TOKPAIR")              /* launch_gemm_tokpair serves nothing: dWt and dT as two engine GEMMs */              \
  X(no_tokpair2, "AVMOE_NO_TOKPAIR2")            /* launch_tok_pair2 serves nothing */                                                 \
  X(no_hop1s, "AVMOE_NO_HOP1S")                  /* the three hop1_stream.hip forms serve nothing */                                   \
  X(no_dpair, "AVMOE_NO_DPAIR")                  /* launch_dpost_pair serves nothing */                                                \
  X(no_dx2, "AVMOE_NO_DX2")                      /* launch_dx_stream2 serves nothing */                                                \
  X(dap_f32, "AVMOE_DAP_F32")                    /* backward: dApost in one fp32 array (the engine), not the split bf16 + fp32 form */ \
  X(stream_pf2, "AVMOE_STREAM_PF2")              /* streaming GEMM: two row tiles of loads in flight */                                \
  X(stream_dy_whole, "AVMOE_STREAM_DY_WHOLE")    /* streaming GEMM: dY in one 768-column block instead of two halves */                \
  X(pick_waves_pow2, "AVMOE_PICK_WAVES_POW2")    /* tile_kernels.hip: the largest of 4, 2, 1 waves per block that fits */              \
  X(gate_token, "AVMOE_GATE_TOKEN")              /* plan: the output gates in token space, not in weight space */                      \
  X(no_gen, "AVMOE_NO_GEN")                      /* plan: without the generalised register-resident kernels */                         \
  X(no_merge, "AVMOE_NO_MERGE")                  /* plan: no merged groups */                                                          \
  X(no_pad32, "AVMOE_NO_PAD32")                  /* plan: per-group bottlenecks below 32 are not padded to the tuned shape */           \
  X(no_fast, "AVMOE_NO_FAST")                    /* plan: the generalised kernels at the tuned shape too (A/B) */                      \
  X(nxn_old_bwd, "AVMOE_NXN_OLD_BWD")            /* plan: the N x N block without the strip kernels */                                 \
  X(no_gram64, "AVMOE_NO_GRAM64")                /* plan: the Gram products on the engine */                                           \
  X(no_fuse_xstats, "AVMOE_NO_FUSE_XSTATS")      /* plan: a separate statistics pass over X */                                         \
  X(no_fuse_l2, "AVMOE_NO_FUSE_L2")              /* plan: the hop-2 logits as a product of their own */
// numbers: the value when the variable is present (nonempty = 1: and not empty), else the default.  X(type, field, "AVMOE_<NAME>", default, nonempty)
#define AVMOE_DEV_NUMS(X)                                                                                                              \
  X(long, ks_target, "AVMOE_KS_TARGET", 512, 0)          /* choose_ksplit: workgroups wanted */                                        \
  X(int, tokpair_tk, "AVMOE_TOKPAIR_TK", 256, 1)         /* launch_gemm_tokpair: tokens per K step (multiple of 64) */                 \
  X(int, leaf2, "AVMOE_LEAF2", AVMOE_LEAF2, 0)           /* backward, fp32 sites: classes of products in two-plane form (moe_run.h) */ \
  X(int, bwd_stop, "AVMOE_BWD_STOP", 0, 0)               /* backward: return after the n-th step of section 1 (moe_backward.cpp) */    \
  X(int, side_mask, "AVMOE_SIDE_MASK", 7, 1)             /* the forks: 1 forward, 2 backward section 1, 4 backward section 2 */        \
  X(long, gen_hog, "AVMOE_GEN_HOG", -1, 0)               /* generalised kernels: bytes of dynamic LDS every launch asks for */
// texts: the variable's value, parsed where it is used; nullptr = not set.  X(field, "AVMOE_<NAME>")
#define AVMOE_DEV_TEXTS(X)                                                                                                             \
  X(gen_r, "AVMOE_GEN_R")                        /* generalised kernels: experts resident per round */                                 \
  X(bps, "AVMOE_BPS")                            /* plan: "<blocks per sample for N >= 512>,<for N < 512>" of the per-token kernels */  \
  X(nxn_budget_mb, "AVMOE_NXN_BUDGET_MB")        /* plan: chunk workspace of the N x N block, MiB */                                   \
  X(stream_cfg, "AVMOE_STREAM_CFG")              /* streaming GEMM: forced configuration (gemm_stream.hip) */                          \
  X(stream_contig, "AVMOE_STREAM_CONTIG")        /* streaming GEMM: forced tile-to-block assignment */
#ifdef AVMOE_DEV
#define AVMOE_SWITCH(type, name, dflt) type name = dflt;
#else
#define AVMOE_SWITCH(type, name, dflt) static constexpr type name = dflt;
#endif
struct Switches {
  std::atomic<unsigned> hook_mask{0};          // HOOK_* bits
  std::atomic<int> nxn_chunk{0};               // frames per chunk of the N x N block; 0 = the library's own choice
  bool hook(unsigned bit) const { return (hook_mask.load(std::memory_order_relaxed) & bit) != 0; }
#define X(name, env) AVMOE_SWITCH(bool, name, false)
  AVMOE_DEV_FLAGS(X)
#undef X
#define X(type, name, env, dflt, nonempty) AVMOE_SWITCH(type, name, dflt)
  AVMOE_DEV_NUMS(X)
#undef X
#define X(name, env) AVMOE_SWITCH(const char*, name, nullptr)
  AVMOE_DEV_TEXTS(X)
#undef X
};
#undef AVMOE_SWITCH
const Switches& switches();
void set_test_hooks(unsigned mask, int nxn_chunk);

// hipFuncAttributeMaxDynamicSharedMemorySize is a per-DEVICE property of a kernel function: one flag per (kernel instantiation,
// device), so a second GPU in the same process gets its attribute too (a process-wide `static bool` set it on the first one only).
struct LdsAttrOnce {
  bool done[64] = {};
  int ensure(const void* fn, int bytes, const char* what);      // OK / ERR_LAUNCH ; no-op for <= 64 KiB and after the first call per device
};

// compute units of the current device (cached per device; <= 0 on a failed query)
int cu_count();

static inline long round_up(long x, long m) { return (x + m - 1) / m * m; }
static inline int cdiv(long a, long b) { return (int)((a + b - 1) / b); }

}  // namespace avmoe
