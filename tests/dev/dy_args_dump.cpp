// Development: prints every field of the GemmArgs that describe a site's dY product -- the in-site one (with and without a cross-modal
// expert) and the two segments moe_backward_dx_dy hangs behind the other site's dX product -- for fixed descriptors, fp32 and bf16.
// The check of a change to those descriptors (moe_backward.cpp: fill_dy_args): build against two revisions and diff the two outputs.
//
//   hipcc -std=c++17 -O1 -rdynamic tests/dev/dy_args_dump.cpp -Lavmoe_amd/lib -lavmoe_hip -Wl,-rpath,$PWD/avmoe_amd/lib -o dy_args_dump
//
// No GPU: the program defines the three launchers the products go to (an executable's definition comes before the library's), runs section
// 16 of moe_backward alone and moe_backward_dx_dy on made-up base addresses, and nothing is launched.  The pointers are printed as given.
#include <cstdio>
#include "../../avmoe_amd/csrc/moe_run.h"

namespace avmoe {

static void dump_seg(const char* tag, const GemmSeg& s) {
  printf("  %s A=%p B=%p K=%d a_layout=%d b_layout=%d lda=%ld ldb=%ld sA1=%ld sA2=%ld sB1=%ld sB2=%ld\n", tag, s.A, s.B, s.K, s.a_layout, s.b_layout,
         s.lda, s.ldb, s.sA1, s.sA2, s.sB1, s.sB2);
}
static int dump(const char* how, const GemmArgs& g) {
  printf(" %s\n", how);
  for (int i = 0; i < 4; ++i) { char t[8]; snprintf(t, sizeof t, "seg%d", i); dump_seg(t, g.segment(i)); }
  printf("  C=%p M=%d N=%d nb1=%d nb2=%d nb3=%d sA3=%ld sB3=%ld sC3=%ld dtype=%d out_dtype=%d sCi=%ld sCj=%ld sC1=%ld sC2=%ld alpha=%g accumulate=%d\n",
         g.C, g.M, g.N, g.nb1, g.nb2, g.nb3, g.sA3, g.sB3, g.sC3, g.dtype, g.out_dtype, g.sCi, g.sCj, g.sC1, g.sC2, (double)g.alpha, g.accumulate);
  printf("  row_scale=%p sRS1=%ld sRS2=%ld D=%p sDi=%ld sD1=%ld sD2=%ld ksplit=%d slabs=%p keep_slabs=%d split3=%d tile=%d\n", (const void*)g.row_scale,
         g.sRS1, g.sRS2, g.D, g.sDi, g.sD1, g.sD2, g.ksplit, (void*)g.slabs, g.keep_slabs, g.split3, g.tile);
  printf("  Cx=%p nsplit=%d ldcx=%ld sCx2=%ld epi=%d row_part=%p row_lse=%p st_rows=%p st_cols=%p st_ntot=%ld st_tiles=%p xcols.B=%p xcols.N=%d xcols.C=%p\n",
         (void*)g.Cx, g.nsplit, g.ldcx, g.sCx2, g.epi, (void*)g.row_part, (const void*)g.row_lse, (void*)g.st_rows, (void*)g.st_cols, g.st_ntot,
         (void*)g.st_tiles, g.xcols.B, g.xcols.N, (void*)g.xcols.C);
  return OK;
}

static bool g_stream3 = false;
int launch_gemm(const GemmArgs& g, hipStream_t) { return dump("launch_gemm", g); }
bool dx_stream3_serves(const GemmArgs&) { return g_stream3; }
int launch_dx_stream3(const GemmArgs& g, hipStream_t) { return dump("launch_dx_stream3", g); }

}  // namespace avmoe

using namespace avmoe;

static avmoe_moe_desc desc(int S, int N, int C, int M, int Cy, int E_m, int E_s, int bf16, int acc_dy) {
  avmoe_moe_desc d = {};
  d.S = S; d.N = N; d.C = C; d.M = M; d.Cy = Cy; d.E_m = E_m; d.E_s = E_s; d.d = 32; d.groups = 2; d.K = 8;
  d.use_bn = d.use_gate = d.ln_before = d.ln_post = 1; d.variant = AVMOE_VARIANT_AVE; d.self_attn = AVMOE_SELF_ATTN_NONE;
  d.dtype = bf16 ? AVMOE_BF16 : AVMOE_F32; d.training = 1; d.bn_eps = 1e-5f; d.ln_eps = 1e-5f; d.bn_momentum = 0.1f; d.accumulate_dy = acc_dy;
  return d;
}

int main() {
  char* const X = (char*)0x1000000, * const Y = (char*)0x2000000, * const dO = (char*)0x3000000, * const dX = (char*)0x4000000, * const dY = (char*)0x5000000;
  char* const sva = (char*)0x10000000, * const sca = (char*)0x20000000, * const svb = (char*)0x30000000, * const scb = (char*)0x40000000;
  avmoe_moe_ptrs prm = {}, grads = {};
  for (int bf16 = 0; bf16 < 2; ++bf16) {
    for (int E_m = 0; E_m <= 2; E_m += 2) {
      for (int acc = 0; acc < 2; ++acc) {                  // the in-site product: section 16 alone
        const avmoe_moe_desc q = desc(6, 40, 96, 56, 64, E_m, 2, bf16, acc);
        Plan pl;
        if (make_plan(&q, &pl) != OK) { printf("make_plan: %s\n", last_error()); return 1; }
        printf("in-site bf16=%d E_m=%d accumulate_dy=%d\n", bf16, E_m, acc);
        const int rc = moe_backward(pl, X, Y, prm, dO, nullptr, sva, sca, dX, dY, grads, nullptr, 16, nullptr, nullptr);
        if (rc != OK) { printf("moe_backward: %d %s\n", rc, last_error()); return 1; }
      }
      for (int s3 = 0; s3 < 2; ++s3) {                     // site A's dX product with site B's dY behind it, on either launcher
        const avmoe_moe_desc qa = desc(6, 40, 96, 56, 96, 2, 2, bf16, 0), qb = desc(6, 56, 96, 40, 96, E_m, 2, bf16, 0);
        Plan pa, pb;
        if (make_plan(&qa, &pa) != OK || make_plan(&qb, &pb) != OK) { printf("make_plan: %s\n", last_error()); return 1; }
        g_stream3 = s3 != 0;
        printf("dx_dy bf16=%d E_m(B)=%d streaming=%d\n", bf16, E_m, s3);
        const int rc = moe_backward_dx_dy(pa, X, sva, sca, pb, svb, scb, dX, true, nullptr);
        printf(" rc=%d\n", rc);
        if (rc < 0) { printf("moe_backward_dx_dy: %s\n", last_error()); return 1; }
      }
    }
  }
  return 0;
}
