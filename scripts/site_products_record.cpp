// Stand-alone record of every product descriptor that moe_forward / moe_backward / moe_backward_dx_dy hand to the engine and to the streaming
// forms: the check of a refactor of the call sites that must not move one field.  No GPU and no device code: the five host files of the site path are
// linked against stubs of everything they call -- the kernel wrappers (k_*) only note their name, the launch_* stubs print every field of the
// descriptor they are handed (all four K segments, xcols, TokPairArgs; pointers as region + offset from fake region bases) and answer
// "launched" or "not served" by a switch, so that both arms of every form chain are recorded.  The site descriptions are those of the fixtures
// under tests/golden and of cfg-2 (bench.py: CONFIGS), between them every branch of the two files.
// Build and run from the repository root; for another tree (the parent's csrc from `git archive`) name that tree's csrc in -I and in the five files:
//   g++ -std=c++17 -O1 -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -Iavmoe_amd/csrc scripts/site_products_record.cpp
//       avmoe_amd/csrc/{moe_forward,moe_backward,moe_plan,common,side}.cpp -o site_products_record
//   ./site_products_record > record.txt            one line per case: the plan's flags, the number of descriptors, a digest of their text
//   ./site_products_record --full > full.txt       every field of every descriptor (about 1 MB)
// Two trees that describe the same products give the same output, in either form.  Exit status 0 and a last line "descriptors: N": every case ran to the end.
#include "pass.h"
#include "moe_run.h"
#include "side.h"
#include <cstdint>
#include <cstdio>
#include <cstdarg>
#include <cstring>
#include <map>
#include <string>

// ---- the HIP runtime calls of side.cpp / common.cpp: no device here ----
static int g_fake_handle[4];
extern "C" {
hipError_t hipGetDevice(int* dev) { *dev = 0; return hipSuccess; }
hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned) { *s = (hipStream_t)&g_fake_handle[0]; return hipSuccess; }
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned) { *e = (hipEvent_t)&g_fake_handle[1]; return hipSuccess; }
hipError_t hipEventRecord(hipEvent_t, hipStream_t) { return hipSuccess; }
hipError_t hipStreamWaitEvent(hipStream_t, hipEvent_t, unsigned) { return hipSuccess; }
hipError_t hipGetLastError(void) { return hipSuccess; }
const char* hipGetErrorString(hipError_t) { return "stub"; }
hipError_t hipMemsetAsync(void*, int, size_t, hipStream_t) { return hipSuccess; }
hipError_t hipFuncSetAttribute(const void*, hipFuncAttribute, int) { return hipSuccess; }
hipError_t hipGetDevicePropertiesR0600(hipDeviceProp_tR0600* p, int) { std::memset(p, 0, sizeof(*p)); p->multiProcessorCount = 256; return hipSuccess; }
}

namespace avmoe {

static bool g_serve = false;      // what the forms answer: launched (0) or not served (1)
static bool g_gen = true;         // whether tile_gen_ok serves the shapes it is asked about
static long g_count = 0;

// fake region bases: region r starts at r << 40
enum { R_SV = 1, R_SC, R_X, R_Y, R_OUT, R_DOUT, R_DX, R_DY, R_SVB, R_SCB, R_PROBS };
static char* base(int r) { return (char*)((uintptr_t)r << 40); }
// what a stub prints goes through `say`: into the text of the descriptor being printed (g_text), else into the digest of the case (FNV-1a, 64 bits)
// and, with --full, to the output
static std::string* g_text = nullptr;
static bool g_full = false;
static uint64_t g_digest = 0;
static void mix(const char* s) { for (; *s; ++s) { g_digest ^= (unsigned char)*s; g_digest *= 1099511628211ull; } }
static void say(const char* fmt, ...) {
  char line[1024];
  va_list ap; va_start(ap, fmt); std::vsnprintf(line, sizeof line, fmt, ap); va_end(ap);
  if (g_text) { *g_text += line; return; }
  mix(line);
  if (g_full) std::fputs(line, stdout);
}
static void ptr(const char* name, const void* p) {
  const uintptr_t v = (uintptr_t)p;
  if (!p) say(" %s=null", name);
  else if ((v >> 40) >= 1 && (v >> 40) <= R_PROBS) say(" %s=r%d+%llu", name, (int)(v >> 40), (unsigned long long)(v & (((uintptr_t)1 << 40) - 1)));
  else say(" %s=set", name);                              // (the address of a local of the caller)
}
static const char* on(hipStream_t st) { return st ? "side" : "main"; }
static int note(const char* name) { say("  %s\n", name); return 0; }

static void print_seg(const char* tag, const GemmSeg& s) {
  say("    %s:", tag);
  ptr("A", s.A); ptr("B", s.B);
  say(" K=%d a_layout=%d b_layout=%d lda=%ld ldb=%ld sA1=%ld sA2=%ld sB1=%ld sB2=%ld\n", s.K, s.a_layout, s.b_layout, s.lda, s.ldb, s.sA1, s.sA2, s.sB1, s.sB2);
}
// Every field of the descriptor; a segment behind the first and the xcols line are left out when they are all default.  The whole text goes into
// the digest of the case; --full prints each distinct text once, as "D<n>", where it first occurs, and a launch line names it.
static std::map<std::string, int> g_seen;
static void print_args(const char* who, const GemmArgs& g, hipStream_t st) {
  ++g_count;
  std::string text;
  g_text = &text;
  for (int i = 0; i < 4; ++i) {
    const GemmSeg& sg = g.segment(i);
    if (i && !sg.A && !sg.B && !sg.K && sg.a_layout == K_MAJOR && sg.b_layout == K_MAJOR && !sg.lda && !sg.ldb && !sg.sA1 && !sg.sA2 && !sg.sB1 && !sg.sB2) continue;
    char tag[8]; std::snprintf(tag, sizeof tag, "seg%d", i); print_seg(tag, sg);
  }
  say("    out:");
  ptr("C", g.C);
  say(" M=%d N=%d nb1=%d nb2=%d nb3=%d sA3=%ld sB3=%ld sC3=%ld dtype=%d out_dtype=%d sCi=%ld sCj=%ld sC1=%ld sC2=%ld alpha=%.9g accumulate=%d\n", g.M, g.N, g.nb1,
              g.nb2, g.nb3, g.sA3, g.sB3, g.sC3, g.dtype, g.out_dtype, g.sCi, g.sCj, g.sC1, g.sC2, (double)g.alpha, g.accumulate);
  say("    terms:");
  ptr("row_scale", g.row_scale); ptr("D", g.D);
  say(" sRS1=%ld sRS2=%ld sDi=%ld sD1=%ld sD2=%ld ksplit=%d", g.sRS1, g.sRS2, g.sDi, g.sD1, g.sD2, g.ksplit);
  ptr("slabs", g.slabs);
  say(" keep_slabs=%d split3=%d tile=%d", g.keep_slabs, g.split3, g.tile);
  ptr("Cx", g.Cx);
  say(" nsplit=%d ldcx=%ld sCx2=%ld epi=%d", g.nsplit, g.ldcx, g.sCx2, g.epi);
  ptr("row_part", g.row_part); ptr("row_lse", g.row_lse); ptr("st_rows", g.st_rows); ptr("st_cols", g.st_cols);
  say(" st_ntot=%ld", g.st_ntot);
  ptr("st_tiles", g.st_tiles);
  say("\n");
  const auto& x = g.xcols;
  if (x.B || x.C || x.N || x.ldb || x.sB1 || x.sB2 || x.ldc || x.sC1 || x.sC2) {
    say("    xcols:");
    ptr("B", x.B);
    say(" N=%d ldb=%ld sB1=%ld sB2=%ld", x.N, x.ldb, x.sB1, x.sB2);
    ptr("C", x.C);
    say(" ldc=%ld sC1=%ld sC2=%ld\n", x.ldc, x.sC1, x.sC2);
  }
  g_text = nullptr;
  auto it = g_seen.find(text);
  const bool first = it == g_seen.end();
  if (first) it = g_seen.emplace(text, (int)g_seen.size() + 1).first;
  char head[96]; std::snprintf(head, sizeof head, "  %s [%s]", who, on(st));
  mix(head); mix(text.c_str());
  if (g_full) std::printf("%s D%d\n%s", head, it->second, first ? text.c_str() : "");
}
static int form(const char* who, const GemmArgs& g, hipStream_t st) {
  print_args(who, g, st);
  say("    -> %s\n", g_serve ? "launched" : "not served");
  return g_serve ? 0 : 1;
}
static int pair_form(const char* who, const TokPairArgs& t, hipStream_t st) {
  ++g_count;
  say("  %s [%s]\n    pair:", who, on(st));
  ptr("A1", t.A1); say(" lda1=%ld M1=%d sA1g=%ld", t.lda1, t.M1, t.sA1g);
  ptr("A2", t.A2); say(" lda2=%ld M2=%d", t.lda2, t.M2);
  ptr("X", t.X); say(" ldx=%ld S=%d N=%d g=%d Cg=%d", t.ldx, t.S, t.N, t.g, t.Cg);
  ptr("C1", t.C1); ptr("C2", t.C2); ptr("slabs", t.slabs);
  say(" slab_cap=%zu\n    -> %s\n", t.slab_cap, g_serve ? "launched" : "not served");
  return g_serve ? 0 : 1;
}

// ---- the engine and the forms ----
int launch_gemm(const GemmArgs& g, hipStream_t st) { print_args("launch_gemm", g, st); return 0; }
int launch_gemm_stream(const GemmArgs& g, hipStream_t st) {
  if (!g.st_tiles) return form("launch_gemm_stream", g, st);
  print_args("launch_gemm_stream (statistics)", g, st);   // the one form with nothing behind it: always launched
  *g.st_tiles = cdiv(g.M, 32);
  return 0;
}
int launch_gemm_frames(const GemmArgs& g, hipStream_t st) { return form("launch_gemm_frames", g, st); }
int launch_dx_stream2(const GemmArgs& g, hipStream_t st) { return form("launch_dx_stream2", g, st); }
bool dx_stream3_serves(const GemmArgs& g) { say("  dx_stream3_serves -> %d\n", (int)g_serve); return g_serve; }
int launch_dx_stream3(const GemmArgs& g, hipStream_t st) { print_args("launch_dx_stream3", g, st); return 0; }
int launch_hop1_yk(const GemmArgs& g, hipStream_t st) { return form("launch_hop1_yk", g, st); }
int launch_hop1_yt_frames(const GemmArgs& g, hipStream_t st) { return form("launch_hop1_yt_frames", g, st); }
int launch_hop1_yt_sum(const GemmArgs& g, size_t cap, hipStream_t st) { say("  (slab_cap=%zu)\n", cap); return form("launch_hop1_yt_sum", g, st); }
int launch_dpost_pair(const GemmArgs& b, const GemmArgs& a, size_t cap, hipStream_t st) {
  say("  (slab_cap=%zu)\n", cap);
  print_args("launch_dpost_pair: dbpost", b, st);
  return form("launch_dpost_pair: dapost", a, st);
}
int launch_gemm_tokpair(const TokPairArgs& t, hipStream_t st) { return pair_form("launch_gemm_tokpair", t, st); }
int launch_tok_pair2(const TokPairArgs& t, hipStream_t st) { return pair_form("launch_tok_pair2", t, st); }
int gemm_row_lse(const float* part, long rows, int tiles, float* lse, hipStream_t) {
  say("  gemm_row_lse:"); ptr("part", part); ptr("lse", lse); say(" rows=%ld tiles=%d\n", rows, tiles);
  return 0;
}

// ---- what the plan asks of the kernel files (the conditions of gemm_stream.hip, nxn_att.hip and tile_fast.hip; tile_gen_ok by a switch) ----
bool gemm_stream_stats_ok(int M, int nb1, int N, int K, long lda, long ldc) {
  const int ks = cdiv(K, 32), tiles = cdiv(N, 16);
  if (M < 64 || (long)M * nb1 < 256 || K > 384 || K % 8 || lda % 8 || ldc % 8 || N % 8) return false;
  return (ks <= 2 && tiles <= 12) || (ks <= 5 && tiles <= 24) || tiles <= 8;
}
bool nxn_att_ok(int bf16, int N, int C, int Np) { return bf16 && (C == 96 || C == 192) && N % 128 == 0 && N >= 128 && Np % 8 == 0; }
bool tile_fast_shape(const Dims& d) { return d.DD == 64 && d.dgp == 32 && d.g == 2 && d.K == 32 && d.Kp == 32 && d.E >= 2 && d.E <= 4; }
bool tile_fast_ok(const Dims& d) { return tile_fast_shape(d) && !d.gen; }
bool tile_gen_ok(const Dims& d) { return g_gen && d.dgp % 16 == 0 && (d.El == 0 || d.Kp % 16 == 0); }
bool prof_enabled() { return false; }
avmoe_moe_ptrs merged_params(const Plan&, const avmoe_moe_ptrs& p, char*) { note("merged_params"); return p; }
avmoe_moe_ptrs merged_grads(const Plan&, const avmoe_moe_ptrs& p, char*) { note("merged_grads"); return p; }
int mha_frames_forward(const Plan&, const void* X, const avmoe_expert_ptrs&, int slot, char*, char*, hipStream_t) {
  say("  mha_frames_forward slot=%d", slot); ptr("X", X); say("\n"); return 0;
}
int mha_frames_backward(const Plan&, const void* X, const avmoe_expert_ptrs&, const avmoe_expert_ptrs&, int slot, const void* dxr, char*, char*, float* slabs, size_t cap, void* dX, hipStream_t) {
  say("  mha_frames_backward slot=%d cap=%zu", slot, cap); ptr("X", X); ptr("dxr", dxr); ptr("slabs", slabs); ptr("dX", dX); say("\n"); return 0;
}

// ---- the kernel wrappers: their name; the N x N strip kernels with the chunk pointers they are handed ----
int k_post_small_bwd(PassCall& c, avmoe_moe_ptrs const&, hipStream_t) {
  say("  k_post_small_bwd dap16=%d\n", c.dap16);
  if (g_serve && c.dap16 && c.pl.d.gram64) c.ran = PASS_STREAM;      // (the streamed form leaves dGq itself)
  return 0;
}
int k_nxn_att(void const* X, int frames, int, int, int, float* lse, void* att, int have, hipStream_t) {
  say("  k_nxn_att frames=%d have_lse=%d", frames, have); ptr("X", X); ptr("lse", lse); ptr("att", att); say("\n"); return 0;
}
int k_nxn_att_bwd(void const* X, void const* dxr, int frames, int, int, int, float const* rd, void const* att, void* dS, hipStream_t) {
  say("  k_nxn_att_bwd frames=%d", frames); ptr("X", X); ptr("dxr", dxr); ptr("rowdot", rd); ptr("att", att); ptr("dS", dS); say("\n"); return 0;
}
int k_nxn_axpy(Plan const&, void const* X, char*, char*, void* dX, int slot, int repl, hipStream_t) {
  say("  k_nxn_axpy slot=%d replaced=%d", slot, repl); ptr("X", X); ptr("dX", dX); say("\n"); return 0;
}
int k_nxn_dx(int key, void const* X, void const* dxr, int frames, int, int, int, float const* lse, float const* rd, void* dX, hipStream_t) {
  say("  k_nxn_dx key=%d frames=%d", key, frames); ptr("X", X); ptr("dxr", dxr); ptr("lse", lse); ptr("rowdot", rd); ptr("dX", dX); say("\n"); return 0;
}
int k_nxn_rowdot(int, void const* X, float const* y, long rows, int, void* dX, float* rd, hipStream_t) {
  say("  k_nxn_rowdot rows=%ld", rows); ptr("X", X); ptr("y", y); ptr("dX", dX); ptr("rowdot", rd); say("\n"); return 0;
}
int k_nxn_xr(void const* X, int frames, int, int, int, float const* lse, void* xr, hipStream_t) {
  say("  k_nxn_xr frames=%d", frames); ptr("X", X); ptr("lse", lse); ptr("xr", xr); say("\n"); return 0;
}
int k_nxn_y(void const* X, void const* dxr, int frames, int, int, int, float const* lse, float* rd, void* dX, hipStream_t) {
  say("  k_nxn_y frames=%d", frames); ptr("X", X); ptr("dxr", dxr); ptr("lse", lse); ptr("rowdot", rd); ptr("dX", dX); say("\n"); return 0;
}
int k_add_bias(bool, void*, long, int, int, float const*, float const*, hipStream_t) { return note("k_add_bias"); }
int k_bn1_finalize(Plan const&, char*, char*, avmoe_moe_ptrs const&, hipStream_t) { return note("k_bn1_finalize"); }
int k_bn_count(Plan const&, avmoe_moe_ptrs const&, hipStream_t) { return note("k_bn_count"); }
int k_colsum_f32(float const*, long, int, long, int, long, float*, long, float, hipStream_t) { return note("k_colsum_f32"); }
int k_down_bwd(Plan const&, char*, avmoe_moe_ptrs const&, avmoe_moe_ptrs const&, hipStream_t) { return note("k_down_bwd"); }
int k_dqrqb(Plan const&, char*, float const*, hipStream_t) { return note("k_dqrqb"); }
int k_finish_T(Plan const&, char*, char*, avmoe_moe_ptrs const&, int, hipStream_t) { return note("k_finish_T"); }
int k_finish_dT(Plan const&, char*, char*, hipStream_t) { return note("k_finish_dT"); }
int k_gram64(Plan const&, void const*, float const*, float, float*, float*, hipStream_t, float const*, float*, float*) { return note("k_gram64"); }
int k_hop1_finalize(Plan const&, char*, char*, avmoe_moe_ptrs const&, avmoe_moe_ptrs const&, hipStream_t) { return note("k_hop1_finalize"); }
int k_merge_expand(Plan const&, char*, avmoe_moe_ptrs const&, hipStream_t) { return note("k_merge_expand"); }
int k_merge_gather(Plan const&, char*, avmoe_moe_ptrs const&, hipStream_t) { return note("k_merge_gather"); }
int k_mid(PassCall&, hipStream_t) { return note("k_mid"); }
int k_mid_bwd(PassCall&, avmoe_moe_ptrs const&, hipStream_t) { return note("k_mid_bwd"); }
int k_onehot_noise(float*, int, int, int, float, hipStream_t) { return note("k_onehot_noise"); }
int k_post_prep(Plan const&, char*, char*, avmoe_moe_ptrs const&, hipStream_t) { return note("k_post_prep"); }
int k_post_prep_bwd(Plan const&, char*, char*, avmoe_moe_ptrs const&, avmoe_moe_ptrs const&, hipStream_t) { return note("k_post_prep_bwd"); }
int k_post_small(PassCall&, hipStream_t) { return note("k_post_small"); }
int k_pre_small(PassCall&, hipStream_t) { return note("k_pre_small"); }
int k_pre_small_bwd(PassCall&, avmoe_moe_ptrs const&, hipStream_t) { return note("k_pre_small_bwd"); }
int k_prep_all(Plan const&, char*, avmoe_moe_ptrs const&, hipStream_t) { return note("k_prep_all"); }
int k_prep_dBm(Plan const&, char*, hipStream_t) { return note("k_prep_dBm"); }
int k_qrqb_fill(Plan const&, char*, float const*, hipStream_t) { return note("k_qrqb_fill"); }
int k_router(Plan const&, char*, char*, avmoe_moe_ptrs const&, float const*, float*, int64_t*, float*, hipStream_t, int, int, float*, float*, float const*, float const*, float*, RouterChoice const*, RouterSinkhorn const*) { return note("k_router"); }
int k_router_bwd(Plan const&, char*, char*, avmoe_moe_ptrs const&, avmoe_moe_ptrs const&, float const*, float const*, hipStream_t, float const*, float const*) { return note("k_router_bwd"); }
int k_softmax_rows(int, float const*, long, int, int, void*, int, int, int, int, int, hipStream_t) { return note("k_softmax_rows"); }
int k_softmax_rows_bwd(int, void const*, float const*, long, int, int, void*, void*, int, int, hipStream_t) { return note("k_softmax_rows_bwd"); }
int k_sum_parts(float const*, int, long, float*, hipStream_t) { return note("k_sum_parts"); }
int k_xrstats(Plan const&, void const*, char*, int, hipStream_t) { return note("k_xrstats"); }
int k_xstats(Plan const&, void const*, char*, char*, hipStream_t) { return note("k_xstats"); }
int k_xstats_fin(float const*, int, long, float*, float const*, int, int, int, float*, long, float, hipStream_t) { return note("k_xstats_fin"); }
int k_zero_bytes(void*, size_t, hipStream_t) { return note("k_zero_bytes"); }

}  // namespace avmoe

using namespace avmoe;

// ---- the sites ----
struct Site { const char* name; int S, N, C, M, Cy, E_m, E_s, red, groups, K, use_bn, ln, variant, self_attn, bf16, training; };
static avmoe_moe_desc desc_of(const Site& s) {
  avmoe_moe_desc d;
  std::memset(&d, 0, sizeof d);
  d.S = s.S; d.N = s.N; d.C = s.C; d.M = s.M; d.Cy = s.Cy; d.E_m = s.E_m; d.E_s = s.E_s; d.d = s.C / s.red; d.groups = s.groups; d.K = s.K;
  d.use_bn = s.use_bn; d.use_gate = 1; d.ln_before = s.ln; d.ln_post = s.ln; d.variant = s.variant; d.self_attn = s.self_attn;
  d.lb_loss = s.variant != 0; d.dtype = s.bf16 ? AVMOE_BF16 : AVMOE_F32; d.training = s.training;
  d.bn_eps = 1e-5f; d.ln_eps = 1e-5f; d.bn_momentum = 0.1f;
  return d;
}
static avmoe_moe_ptrs g_prm, g_grads;      // all null: no stub reads a parameter (self_attention.* checks live in mha_frames.hip, stubbed)
static long g_cases = 0;

static bool plan_of(const Site& s, Plan* pl, int acc = 0) {
  avmoe_moe_desc d = desc_of(s);
  d.accumulate_dx = d.accumulate_dy = d.accumulate_out = acc;
  const int rc = make_plan(&d, pl);
  if (rc != OK) std::printf("  make_plan: %d (%s)\n", rc, last_error());
  return rc == OK;
}
static void begin(const char* what, const Site& s, const Plan& pl) {
  const Dims& d = pl.d;
  ++g_cases;
  g_digest = 14695981039346656037ull;
  char head[400];
  std::snprintf(head, sizeof head, "== %s: %s serve=%d gen_ok=%d | g=%d mg=%d gen=%d dgp=%d zsz=%d gram64=%d fuse_xs=%d fuse_l2=%d El=%d Kcy=%d Kcx=%d KP=%d KPp=%d nxn=%d mha=%d nxc=%d nflash=%d", what, s.name,
              (int)g_serve, (int)g_gen, d.g, d.mg, d.gen, d.dgp, d.zsz, d.gram64, d.fuse_xs, d.fuse_l2, d.El, d.Kcy, d.Kcx, d.KP, d.KPp, d.nxn, d.mha, d.nxc, d.nflash);
  mix(head);
  std::printf(g_full ? "%s\n" : "%s", head);
}
static void end(int rc, long before) {
  if (rc != OK) say("  rc=%d (%s)\n", rc, last_error());
  if (g_full) std::printf("  descriptors of the case: %ld\n", g_count - before);
  else std::printf(" | descriptors=%ld digest=%016llx\n", g_count - before, (unsigned long long)g_digest);
}

static void forward(const Site& s) {
  Plan pl;
  if (!plan_of(s, &pl)) return;
  begin("forward", s, pl);
  const long c0 = g_count;
  end(moe_forward(pl, base(R_X), base(R_Y), g_prm, nullptr, base(R_OUT), (float*)base(R_PROBS), nullptr, nullptr, base(R_SV), base(R_SC), nullptr, 0, 1, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr), c0);
}
static void backward(const Site& s, int parts, int acc = 0) {
  Plan pl;
  if (!plan_of(s, &pl, acc)) return;
  char what[32]; std::snprintf(what, sizeof what, "backward parts=%d acc=%d", parts, acc);
  begin(what, s, pl);
  const long c0 = g_count;
  end(moe_backward(pl, base(R_X), base(R_Y), g_prm, base(R_DOUT), nullptr, base(R_SV), base(R_SC), base(R_DX), base(R_DY), g_grads, nullptr, parts, nullptr, nullptr, nullptr), c0);
}
static void pair(const Site& a, const Site& b, bool launch) {
  Plan pa, pb;
  if (!plan_of(a, &pa) || !plan_of(b, &pb)) return;
  begin(launch ? "dx_dy launch, site A" : "dx_dy query, site A", a, pa);
  const long c0 = g_count;
  const int rc = launch ? moe_backward_dx_dy(pa, base(R_X), base(R_SV), base(R_SC), pb, base(R_SVB), base(R_SCB), base(R_DX), true, nullptr)
                        : moe_backward_dx_dy(pa, nullptr, nullptr, nullptr, pb, nullptr, nullptr, nullptr, false, nullptr);
  say("  dx_dy -> %d\n", rc);
  end(rc < 0 ? rc : OK, c0);
}

int main(int argc, char** argv) {
  g_full = argc > 1 && !std::strcmp(argv[1], "--full");
  //                 name                 S    N     C    M    Cy  Em Es red g  K  bn ln var sa bf16 train
  const Site cfg2a_bf16{"cfg2 audio bf16", 320, 1024, 768, 196, 768, 2, 2, 12, 2, 32, 1, 1, 0, 0, 1, 1};      // bench.py: CONFIGS["cfg2"], B * T frames
  const Site cfg2v_bf16{"cfg2 visual bf16", 320, 196, 768, 1024, 768, 2, 2, 12, 2, 32, 1, 1, 0, 0, 1, 1};
  const Site cfg2a_f32{"cfg2 audio f32", 320, 1024, 768, 196, 768, 2, 2, 12, 2, 32, 1, 1, 0, 0, 0, 1};
  const Site cfg2v_f32{"cfg2 visual f32", 320, 196, 768, 1024, 768, 2, 2, 12, 2, 32, 1, 1, 0, 0, 0, 1};
  const Site cfg2_b2{"cfg2 audio bf16 B=2", 20, 1024, 768, 196, 768, 2, 2, 12, 2, 32, 1, 1, 0, 0, 1, 1};      // below the helper-stream threshold
  const Site ave_train{"ave_train", 6, 40, 96, 56, 64, 2, 2, 8, 2, 8, 1, 1, 0, 0, 0, 1};
  const Site ave_swap{"ave_swap_train", 6, 56, 64, 40, 96, 2, 2, 8, 2, 8, 1, 1, 0, 0, 0, 1};                // ave_train's partner: its X is ave_train's Y
  const Site ave_bf16{"ave_train bf16", 6, 40, 96, 56, 64, 2, 2, 8, 2, 8, 1, 1, 0, 0, 1, 1};
  const Site ave_eval{"ave_eval", 6, 40, 96, 56, 64, 2, 2, 8, 2, 8, 1, 1, 0, 0, 0, 0};
  const Site ave_nobn{"ave_nobn", 6, 40, 96, 56, 64, 2, 2, 8, 2, 8, 0, 1, 0, 0, 0, 1};
  const Site ave_noln{"ave_noln_nogate", 6, 40, 96, 56, 64, 2, 2, 8, 2, 8, 1, 0, 0, 0, 0, 1};
  const Site ave_e1p1{"ave_e1p1_train", 6, 40, 96, 56, 64, 1, 1, 8, 2, 8, 1, 1, 0, 0, 0, 1};               // 2 experts: KP % 4 != 0
  const Site ave_cross{"ave_only_cross", 6, 40, 96, 56, 64, 1, 0, 8, 2, 8, 1, 1, 0, 0, 0, 1};
  const Site ave_single{"ave single-modal only", 6, 40, 96, 56, 64, 0, 2, 8, 2, 8, 1, 1, 0, 0, 0, 1};      // El = 0, Kcy = 0
  const Site ave_wide{"ave_wide_train bf16", 2, 64, 768, 49, 192, 2, 2, 12, 2, 32, 1, 1, 0, 0, 1, 1};
  const Site avqa{"avqa_train", 6, 40, 96, 56, 64, 1, 2, 8, 4, 2, 1, 1, 0, 0, 0, 1};                       // merged groups, 3 experts
  const Site avqa_bf16{"avqa_train bf16", 6, 40, 96, 56, 64, 1, 2, 8, 4, 2, 1, 1, 0, 0, 1, 1};
  const Site avs_k87{"avs_k87_train", 3, 40, 96, 56, 64, 2, 2, 8, 2, 87, 1, 1, 2, 0, 0, 1};
  const Site avs_v2{"avs_v2_train", 6, 40, 96, 56, 64, 2, 2, 8, 2, 8, 1, 1, 2, 1, 0, 1};                   // latent self attention on X: Kcx > 0
  const Site avs_v2_bf16{"avs_v2_train bf16", 6, 40, 96, 56, 64, 2, 2, 8, 2, 8, 1, 1, 2, 1, 1, 1};
  const Site avs_v1{"avs_v1_train", 5, 24, 64, 40, 48, 2, 2, 4, 2, 8, 1, 1, 2, 3, 0, 1};
  const Site avs_v1_fast{"avs_v1_fast_train bf16", 4, 40, 128, 24, 64, 2, 2, 2, 2, 32, 1, 1, 2, 3, 1, 1};
  const Site avvp{"avvp_train", 6, 40, 96, 56, 64, 2, 2, 8, 2, 8, 1, 1, 1, 2, 0, 1};
  const Site avvp_bf16{"avvp_train bf16", 6, 40, 96, 56, 64, 2, 2, 8, 2, 8, 1, 1, 1, 2, 1, 1};
  const Site avvp_eval{"avvp_eval", 6, 40, 96, 56, 64, 2, 2, 8, 2, 8, 1, 1, 1, 2, 0, 0};
  const Site avvp_fast{"avvp_fast_train bf16", 4, 40, 128, 24, 64, 1, 1, 2, 2, 32, 1, 1, 1, 2, 1, 1};
  const Site avvp_flash{"avvp N=128 bf16", 6, 128, 96, 56, 64, 2, 2, 8, 2, 8, 1, 1, 1, 2, 1, 1};            // the strip kernels (nflash)
  const Site* all[] = {&cfg2a_bf16, &cfg2v_bf16, &cfg2a_f32, &cfg2v_f32, &cfg2_b2, &ave_train, &ave_swap, &ave_bf16, &ave_eval, &ave_nobn, &ave_noln, &ave_e1p1, &ave_cross,
                       &ave_single, &ave_wide, &avqa, &avqa_bf16, &avs_k87, &avs_v2, &avs_v2_bf16, &avs_v1, &avs_v1_fast, &avvp, &avvp_bf16, &avvp_eval, &avvp_fast, &avvp_flash};
  for (int serve = 0; serve < 2; ++serve)
    for (int gen = 1; gen >= 0; --gen) {
      g_serve = serve; g_gen = gen;
      for (const Site* s : all) {
        if (!gen && s->C == 768 && s->K == 32) continue;      // (the plans of the register-resident shape do not ask tile_gen_ok: the same record twice)
        forward(*s);
        backward(*s, 0);
      }
      if (!gen) continue;
      // the split backward, section by section, and with accumulation into dX / dY / out
      for (const Site* s : {&cfg2a_bf16, &ave_train, &ave_cross}) {
        for (int parts : {1, 32, 64, 8, 16}) backward(*s, parts);
        backward(*s, 2 | 4, 1);
      }
      // the frame loop of the N x N block in chunks
      set_test_hooks(0, 4);
      for (const Site* s : {&avvp, &avvp_bf16, &avvp_flash}) { forward(*s); backward(*s, 0); }
      set_test_hooks(0, 0);
      // one token gradient for site A's dX and site B's dY
      pair(cfg2a_bf16, cfg2v_bf16, false); pair(cfg2a_bf16, cfg2v_bf16, true);
      pair(cfg2a_f32, cfg2v_f32, true);
      pair(ave_swap, ave_train, true); pair(ave_bf16, ave_swap, true);      // fp32 on the engine ; mismatched element types: not served
      pair(ave_swap, ave_cross, true);
    }
  std::printf("cases: %ld\ndistinct descriptors: %zu\ndescriptors: %ld\n", g_cases, g_seen.size(), g_count);
  return 0;
}
