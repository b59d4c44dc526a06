// The inline-ISA primitives of the streaming kernels (DESIGN_CURRENT.md section 3 / 3b), each defined once: direct global -> LDS loads,
// counted vector-memory waits in front of a bare barrier, LDS reads issued and waited for by hand, bf16 pack / unpack by bit tricks.
// Device-only; include after <hip/hip_runtime.h>.  What each one is for and what the compiler does otherwise stands beside it: these
// details (a memory clobber, the registers a wait names, a clamp) decide whether such a kernel is correct and fast.  Ring geometry, piece
// dealing, buffer counts and the wait arithmetic are each kernel's own.
#pragma once

namespace avmoe {

// ---- vector and address-space types --------------------------------------------------------------------------------------------------
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;         // one MFMA operand of v_mfma_f32_16x16x32_bf16
typedef __attribute__((ext_vector_type(4))) float f32x4;           // one 16 x 16 accumulator tile per lane
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;
typedef __attribute__((ext_vector_type(2))) unsigned int u32x2;
typedef __attribute__((ext_vector_type(4))) short s16x4;           // what the ds_read_tr16_b64 intrinsic returns
typedef __attribute__((ext_vector_type(8))) short s16x8;
typedef __attribute__((address_space(1))) const void* gptr_t;      // global source / LDS destination of a direct load
typedef __attribute__((address_space(3))) void* lptr_t;
typedef __attribute__((address_space(3))) s16x4* lds_s16x4;        // operand of the transposing-read intrinsic

// ---- bf16 by bit tricks ---------------------------------------------------------------------------------------------------------------
// round-to-nearest-even bf16 in the low half of a dword, ready to be or-ed into a pair (device_utils.h::f2bf returns the bare 16 bits)
__device__ __forceinline__ unsigned int f2bf_u(float x) { return (unsigned int)__builtin_bit_cast(unsigned short, (__bf16)x); }
__device__ __forceinline__ unsigned int pack2(float a, float b) { return f2bf_u(a) | (f2bf_u(b) << 16); }
// the two bf16 of a dword as floats: a shift / a mask, no conversion instruction
__device__ __forceinline__ float bflo(unsigned int u) { return __builtin_bit_cast(float, u << 16); }
__device__ __forceinline__ float bfhi(unsigned int u) { return __builtin_bit_cast(float, u & 0xffff0000u); }

// ---- direct global -> LDS loads ---------------------------------------------------------------------------------------------------------
// the 32-bit LDS address of a pointer into shared memory (the operand of the hand-issued reads below)
__device__ __forceinline__ unsigned lds_off(const void* p) { return (unsigned)(size_t)(lptr_t)p; }
// One wave instruction moves 64 x BYTES (16 or 4) from per-lane global addresses to CONSECUTIVE LDS addresses from `l` (wave-uniform): no
// staging registers.  AUX is the cache policy (0 plain, 2 non-temporal: common.h::AVMOE_LDS_AUX); every kernel passes its own *_AUX macro.
// The load counts on vmcnt like any vector-memory instruction, and the compiler puts s_waitcnt vmcnt(0) in front of every LDS access IT
// can see after one -- which is why the kernels wait by count (wait_vm) and read the LDS through the asm statements below.
template <int BYTES, int AUX>
__device__ __forceinline__ void glds(const void* g, const void* l) {
  static_assert(BYTES == 16 || BYTES == 4, "dwordx4 or dword");
  if constexpr (BYTES == 16) __builtin_amdgcn_global_load_lds((gptr_t)g, (lptr_t)l, 16, 0, AUX);      // (the builtin wants the size as a literal)
  else __builtin_amdgcn_global_load_lds((gptr_t)g, (lptr_t)l, 4, 0, AUX);
}

// ---- vector-memory waits ----------------------------------------------------------------------------------------------------------------
// until at most N vector-memory operations of this wave are pending (loads and stores complete in issue order as far as this counter
// goes).  The memory clobber keeps the compiler's own memory accesses on their side.  The counter holds 6 bits: N is clamped at its
// ceiling, which waits for more than asked, never for less.
template <int N> __device__ __forceinline__ void wait_vm() { asm volatile("s_waitcnt vmcnt(%0)" :: "n"(N < 63 ? N : 63) : "memory"); }
// ... for a run-time (wave-uniform) n: the immediate has to be a constant
__device__ __forceinline__ void wait_vm_n(int n) {
  switch (n) {
#define W1(k) case k: wait_vm<k>(); break;
#define W8(k) W1(k) W1(k + 1) W1(k + 2) W1(k + 3) W1(k + 4) W1(k + 5) W1(k + 6) W1(k + 7)
    W8(0) W8(8) W8(16) W8(24) W8(32) W8(40) W8(48) W1(56) W1(57) W1(58) W1(59) W1(60) W1(61) W1(62)
#undef W8
#undef W1
    default: wait_vm<63>(); break;
  }
}

// ---- LDS accesses issued by hand -------------------------------------------------------------------------------------------------------
// For the intrinsics and for plain C++ loads the compiler first drains EVERY direct load in flight (it cannot tell that they go to another
// buffer) and then waits lgkmcnt(0) in front of the first use: no load overlaps the arithmetic and the matrix pipe idles for one LDS
// latency per read.  As asm statements the reads are issued where they are written and waited for by count (wait_lgkm below).  Two
// flavours:
//   plain   with a memory clobber: the compiler moves none of its own memory accesses across the read.  Needed wherever the same LDS is
//           also written or read from C++ between two barriers (a wave-private tile, a fold buffer, stores to a dump word in flight).
//   _ro     without: the tile is READ-ONLY between two barriers and every access to it in that span is one of these statements or a
//           C++ load, so the compiler's own loads may move across (volatile asm statements keep their order among themselves).
template <int OFF> __device__ __forceinline__ void tr_issue(u32x2& d, unsigned addr) { asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(d) : "v"(addr), "n"(OFF) : "memory"); }
template <int OFF> __device__ __forceinline__ void tr_issue_ro(u32x2& d, unsigned addr) { asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(d) : "v"(addr), "n"(OFF)); }
template <int OFF, typename V> __device__ __forceinline__ void lds_rd128(V& d, unsigned addr) { asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(d) : "v"(addr), "n"(OFF) : "memory"); }
template <int OFF> __device__ __forceinline__ void lds_rd128_ro(u32x4& d, unsigned addr) { asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(d) : "v"(addr), "n"(OFF)); }
__device__ __forceinline__ void lds_rd32(float& v, unsigned addr) { asm volatile("ds_read_b32 %0, %1" : "=v"(v) : "v"(addr) : "memory"); }
// (one value needed at once: read and wait in one statement)
__device__ __forceinline__ float lds_rd32_wait(unsigned addr) { float v; asm volatile("ds_read_b32 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(v) : "v"(addr) : "memory"); return v; }
__device__ __forceinline__ void lds_wr128(unsigned addr, const f32x4& v) { asm volatile("ds_write_b128 %0, %1" :: "v"(addr), "v"(v) : "memory"); }
__device__ __forceinline__ void lds_wr64(unsigned addr, const u32x2& v) { asm volatile("ds_write_b64 %0, %1" :: "v"(addr), "v"(v) : "memory"); }
__device__ __forceinline__ void lds_wr32(unsigned addr, float v) { asm volatile("ds_write_b32 %0, %1" :: "v"(addr), "v"(v) : "memory"); }

// until at most N LDS operations are pending (the LDS answers in order).  The registers named are those the reads to be waited for
// filled: they pass THROUGH the statement, so their users stay behind the wait -- without them the compiler may use a register before
// its read has landed.  The forms on single registers belong to the _ro reads (no clobber), the forms on fragment sets to tr_issue.
template <int N> __device__ __forceinline__ void wait_lgkm(u32x4& a) { asm volatile("s_waitcnt lgkmcnt(%1)" : "+v"(a) : "n"(N)); }
template <int N> __device__ __forceinline__ void wait_lgkm(u32x4& a, u32x4& b) { asm volatile("s_waitcnt lgkmcnt(%2)" : "+v"(a), "+v"(b) : "n"(N)); }
template <int N> __device__ __forceinline__ void wait_lgkm(u32x2& a, u32x2& b) { asm volatile("s_waitcnt lgkmcnt(%2)" : "+v"(a), "+v"(b) : "n"(N)); }
template <int N> __device__ __forceinline__ void wait_lgkm(u32x2 (&x)[3][2]) {
  asm volatile("s_waitcnt lgkmcnt(%6)" : "+v"(x[0][0]), "+v"(x[0][1]), "+v"(x[1][0]), "+v"(x[1][1]), "+v"(x[2][0]), "+v"(x[2][1]) : "n"(N) : "memory");
}
template <int N> __device__ __forceinline__ void wait_lgkm(u32x2 (&x)[3][2], u32x2 (&y)[3][2]) {
  asm volatile("s_waitcnt lgkmcnt(%12)" : "+v"(x[0][0]), "+v"(x[0][1]), "+v"(x[1][0]), "+v"(x[1][1]), "+v"(x[2][0]), "+v"(x[2][1]),
               "+v"(y[0][0]), "+v"(y[0][1]), "+v"(y[1][0]), "+v"(y[1][1]), "+v"(y[2][0]), "+v"(y[2][1]) : "n"(N) : "memory");
}

// ---- transposed MFMA fragments ----------------------------------------------------------------------------------------------------------
// One 16-column fragment of a token-major tile whose contraction index is the token: rows 8 q .. 8 q + 7 as two transposing reads (`base`
// already holds the lane's row 8 q + (r >> 2) and column group 4 (r & 3)), OFF = byte offset of the column tile, ROWB = LDS row pitch.
template <int OFF, int ROWB>
__device__ __forceinline__ void tr_frag2(u32x2 (&f)[2], unsigned base) { tr_issue<OFF>(f[0], base); tr_issue<OFF + 4 * ROWB>(f[1], base); }
__device__ __forceinline__ bf16x8 tr_pack(const u32x2 (&f)[2]) { return __builtin_bit_cast(bf16x8, u32x4{f[0][0], f[0][1], f[1][0], f[1][1]}); }
// ... with the entries of the tokens beyond a ragged tile's end zeroed (mk: 0xffffffff / 0x0000ffff / 0 per pair of tokens)
__device__ __forceinline__ bf16x8 tr_pack_masked(const u32x2 (&f)[2], const u32x4& mk) { return __builtin_bit_cast(bf16x8, u32x4{f[0][0], f[0][1], f[1][0], f[1][1]} & mk); }

}  // namespace avmoe
