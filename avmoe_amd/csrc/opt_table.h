// The table walk of the optimizer with device-side state, shared by opt_kernels.hip and opt_muon.hip: the table image's layout, what a
// thread of a one-block-per-table-block launch serves, the block reduction in a fixed order, the rules of the per-range side buffers
// (shadows, hold, ...), and the host-side checks every update entry point makes.  Device code lives in headers once; each translation
// unit gets its own copy.
#pragma once
#include "../../include/avmoe.h"
#include "common.h"
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

namespace avmoe {

constexpr int OPT_BLOCK = 1024;                  // elements per block: 256 threads x 4, as kk_adam
constexpr uint32_t OPT_MAGIC = 0x4f50544du;      // "OPTM"

// the table image: header, the ranges, then one (range, block inside the range) pair per 1024-element block
struct OptHeader { uint32_t magic; int32_t n_ranges; int64_t n_blocks; };
struct OptBlock { int32_t range, block; };
static_assert(sizeof(OptHeader) == 16 && sizeof(avmoe_opt_range) == 48 && sizeof(avmoe_opt_state) == 64, "table / state layout");
static_assert(sizeof(avmoe_opt_report_header) == 16, "report layout");
static_assert(sizeof(avmoe_opt_sam_state) == 16, "SAM block layout");
static_assert(sizeof(avmoe_opt_swa) == 32 && sizeof(avmoe_opt_schedule) == 40 && sizeof(avmoe_opt_ema) == 8, "constants of a run");

// What a thread of a one-block-per-table-block launch serves: elements [i0, min(i0 + 4, r.n)) of range `range`.
struct OptWork { int32_t n_ranges, range; avmoe_opt_range r; long i0; };

// -> false where the thread has nothing to touch: a launch whose grid does not match the table (a stale or foreign image: wrong magic, a
// block past n_blocks, a range index outside the table), or a thread past the end of its range.
__device__ __forceinline__ bool opt_work(const void* __restrict__ table, OptWork& w) {
  const OptHeader h = *(const OptHeader*)table;
  if (h.magic != OPT_MAGIC || (long)blockIdx.x >= h.n_blocks) return false;
  const char* ranges = (const char*)table + sizeof(OptHeader);
  const OptBlock b = ((const OptBlock*)(ranges + (size_t)h.n_ranges * sizeof(avmoe_opt_range)))[blockIdx.x];
  if (b.range < 0 || b.range >= h.n_ranges) return false;
  w.n_ranges = h.n_ranges;
  w.range = b.range;
  w.r = ((const avmoe_opt_range*)ranges)[b.range];
  w.i0 = ((long)b.block * 256 + threadIdx.x) * 4;
  return w.i0 < w.r.n;
}

// one value per thread of a 256-thread block -> their sum, by a tree over LDS: a fixed order of additions
__device__ __forceinline__ double block_sum_256(double acc) {
  __shared__ double red[256];
  red[threadIdx.x] = acc;
  __syncthreads();
#pragma unroll
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  return red[0];
}

// the shadow buffer of range `range`, or NULL where the pointer array was not made for this table (another range count) or the entry
// cannot take 16-byte accesses: such a launch touches nothing
__device__ __forceinline__ float* opt_shadow(const OptWork& w, float* const* __restrict__ shadows, int n_shadows) {
  if (w.n_ranges != n_shadows) return nullptr;
  float* e = shadows[w.range];
  return ((uintptr_t)e & 15u) == 0 ? e : nullptr;
}

// param[i] = hold[i] for elements [i0, min(i0 + 4, n)) of one range: what a skipped step under HOLD does
__device__ __forceinline__ void restore_quad(float* __restrict__ p, const float* __restrict__ h, long i0, long n) {
  if (i0 + 3 < n) {
    *(float4*)(p + i0) = *(const float4*)(h + i0);
  } else {
    for (long i = i0; i < n; ++i) p[i] = h[i];
  }
}

constexpr int32_t OPT_STEP_FLAGS = AVMOE_OPT_CLIP | AVMOE_OPT_SKIP_NONFINITE | AVMOE_OPT_DECOUPLED_DECAY | AVMOE_OPT_LR_SCHEDULE | AVMOE_OPT_EMA;

inline size_t round16(size_t b) { return (b + 15) & ~(size_t)15; }

// what every update entry point refuses, in one order (opt_kernels.hip)
int check_step_args(const char* who, const void* table, int32_t n_ranges, int64_t n_blocks, const avmoe_opt_state* state, float beta1,
                    float beta2, float eps, float grad_scale, int32_t flags, int32_t known_flags, float* const* shadows, bool with_hold,
                    float* const* hold);

// The head of the image avmoe_opt_muon_large_table_build writes (opt_muon_large.hip: header, n_mats matrices of 64 bytes, n_classes classes
// of 64 bytes, then n_ranges int32: the large matrix of a range, or -1), here because the table walk of opt_muon.hip reads that map too.
constexpr uint32_t MUONL_MAGIC = 0x4d554c47u;    // "MULG"
constexpr size_t MUONL_MAT_BYTES = 64, MUONL_CLASS_BYTES = 64;
struct MuonLargeHeader { uint32_t magic; int32_t n_mats, n_ranges, n_classes; int64_t sums_off, ws_bytes; };
static_assert(sizeof(MuonLargeHeader) == 32, "large Muon image header");

// the range -> matrix map of a large image, or NULL where the image is not one of n_mats matrices and n_ranges ranges
__host__ __device__ inline const int32_t* muonl_map(const void* image, int n_mats, int n_ranges) {
  const MuonLargeHeader h = *(const MuonLargeHeader*)image;
  if (h.magic != MUONL_MAGIC || h.n_mats != n_mats || h.n_ranges != n_ranges || h.n_classes < 0) return nullptr;
  return (const int32_t*)((const char*)image + sizeof(MuonLargeHeader) + (size_t)n_mats * MUONL_MAT_BYTES + (size_t)h.n_classes * MUONL_CLASS_BYTES);
}

// avmoe_opt_muon_step in two halves (opt_muon.hip), so that avmoe_opt_muon_step_large (opt_muon_large.hip) makes every check before its
// first launch: what the call refuses, then the table walk and the one-workgroup-per-matrix kernel.  large (DEVICE, or NULL): the image
// of n_large large matrices; the table walk treats the ranges of its map as listed too, and touches nothing where the image is not this
// launch's.
int muon_step_check(const char* who, const void* table, int32_t n_ranges, int64_t n_blocks, const avmoe_opt_state* state, float beta1, float beta2,
                    float eps, float grad_scale, int32_t flags, float* const* shadows, float* const* hold, const void* mats, int32_t n_mats,
                    float* const* work, const avmoe_opt_muon* consts, const double* workspace, const void* report);
int muon_step_launch(const char* who, const void* table, int32_t n_ranges, int64_t n_blocks, const avmoe_opt_state* state, float beta1, float beta2,
                     float eps, float grad_scale, int32_t flags, hipStream_t stream, float* const* shadows, float* const* hold, const void* mats,
                     int32_t n_mats, float* const* work, const avmoe_opt_muon* consts, double* workspace, void* report, const void* large,
                     int32_t n_large);

}  // namespace avmoe
