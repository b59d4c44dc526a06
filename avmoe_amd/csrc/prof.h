// Optional per-launch timing (HIP events on the launch stream), off by default.  bench.py switches it on for
// a separate profiling pass to find the dominant kernel and its average duration / algorithmic bytes; the
// numbers must agree with `rocprofv3 --kernel-trace --stats` of the same command (profiles/).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

namespace avmoe {

bool prof_enabled();
void prof_enable(bool on);
void prof_reset();
// call right before / after a launch; `name` must be a string literal or otherwise outlive the report
void prof_begin(const char* name, double alg_bytes, double flops, hipStream_t st);
void prof_end(hipStream_t st);
// JSON array of {"name","calls","total_ms","alg_bytes","flops"}; returns bytes written (excluding NUL)
size_t prof_report(char* buf, size_t cap);

// AVMOE_PROF_SHAPES=1: one family per distinct launch shape (the GEMM engine appends M/N/K, the bottleneck-space scopes
// their token count) instead of one per kernel name
bool prof_shapes();
void prof_begin_tagged(const char* name, long tag, double alg_bytes, double flops, hipStream_t st);
// the open record under another name (tag < 0: untagged) and with other bytes
void prof_relabel(const char* name, long tag, double alg_bytes);

struct ProfScope {
  hipStream_t st; bool on; long tag = -1;
  ProfScope(const char* name, double bytes, double flops, hipStream_t s) : st(s), on(prof_enabled()) {
    if (on) prof_begin(name, bytes, flops, s);
  }
  ProfScope(const char* name, long tokens, double bytes, double flops, hipStream_t s) : st(s), on(prof_enabled()), tag(tokens) {
    if (on) prof_begin_tagged(name, tokens, bytes, flops, s);
  }
  ~ProfScope() { if (on) prof_end(st); }
  // A wrapper whose forms differ in what the profiler shows (pass.h): the form that ran is known after the chain.
  void relabel(const char* name, double bytes) { if (on) prof_relabel(name, tag, bytes); }
  // ends the record here and opens the next one on the same stream (tagged with this scope's token count, or not)
  void next(const char* name, bool tagged, double bytes) {
    if (!on) return;
    prof_end(st);
    if (tagged) prof_begin_tagged(name, tag, bytes, 0.0, st); else prof_begin(name, bytes, 0.0, st);
  }
};

}  // namespace avmoe
