// Stand-alone check of the matrix views of csrc/gemm.h (Mat, GemmArgs::product / add_segment / add_term): every view operation builds a product
// that is compared, field by field, with the descriptor written out by hand, and every refusal is provoked once.  Host code only, nothing is
// launched.  Built and run by tests/test_product_views_host.py:
//   g++ -std=c++17 -D__HIP_PLATFORM_AMD__ -I<rocm>/include tests/product_views_check.cpp -o product_views_check
// Prints one line per check; exit status 0 and "ok" on the last line when all hold.
#include "../avmoe_amd/csrc/gemm.h"
#include <cstdarg>
#include <cstdio>
#include <cstring>

namespace avmoe {
static char g_err[512];
void set_last_error(const char* fmt, ...) { va_list ap; va_start(ap, fmt); std::vsnprintf(g_err, sizeof g_err, fmt, ap); va_end(ap); }
const char* last_error() { return g_err; }
}  // namespace avmoe
using namespace avmoe;

static int g_bad = 0;
static void report(const char* what, bool ok) { std::printf("%-28s %s\n", what, ok ? "ok" : "MISMATCH"); g_bad += !ok; }

static bool same_seg(const GemmSeg& a, const GemmSeg& b) {
  return a.A == b.A && a.B == b.B && a.K == b.K && a.a_layout == b.a_layout && a.b_layout == b.b_layout && a.lda == b.lda && a.ldb == b.ldb && a.sA1 == b.sA1 &&
         a.sA2 == b.sA2 && a.sB1 == b.sB1 && a.sB2 == b.sB2;
}
// every field the binding sets (the rest of the two descriptors is default-constructed on both sides)
static bool same(const GemmArgs& a, const GemmArgs& b) {
  bool ok = a.C == b.C && a.M == b.M && a.N == b.N && a.sCi == b.sCi && a.sCj == b.sCj && a.sC1 == b.sC1 && a.sC2 == b.sC2 && a.D == b.D && a.sDi == b.sDi &&
            a.sD1 == b.sD1 && a.sD2 == b.sD2;
  for (int i = 0; i < 4; ++i) ok = ok && same_seg(a.segment(i), b.segment(i));
  return ok;
}
static Mat mat(const void* p, int esz, int rows, int cols, long ld, long s1 = 0) { Mat m; m.p = p; m.esz = esz; m.rows = rows; m.cols = cols; m.ld = ld; m.s1 = s1; return m; }
static GemmArgs typed(int dtype, int out_dtype) { GemmArgs g; g.dtype = dtype; g.out_dtype = out_dtype; return g; }
static bool refused(int rc) { const bool r = rc == ERR_BAD_ARG && g_err[0]; g_err[0] = 0; return r; }

int main() {
  // 2 frames; fp32 tensors X (5 x 12, ld 16), W (7 x 12, ld 16), P (5 x 7, ld 8), Q (12 x 7, ld 8) ; bf16 tensors H (24 x 6, ld 8), U (6 x 3, ld 8)
  static float X[2 * 5 * 16], W[7 * 16], P[2 * 5 * 8], Q[2 * 12 * 8], R[2 * 24 * 24];
  static unsigned short H[2 * 24 * 8], U[6 * 8], O[2 * 24 * 8];
  const Mat Xv = mat(X, 4, 5, 12, 16, 5 * 16), Wv = mat(W, 4, 7, 12, 16), Pv = mat(P, 4, 5, 7, 8, 5 * 8), Qv = mat(Q, 4, 12, 7, 8, 12 * 8);
  const Mat Hv = mat(H, 2, 24, 6, 8, 24 * 8), Uv = mat(U, 2, 6, 3, 8), Ov = mat(O, 2, 24, 3, 8, 24 * 8);

  {   // T(): P[s] = X[s] W^T  -- B as the transpose of a stored N x K
    GemmArgs g = typed(GEMM_F32, GEMM_F32), h = g;
    const int rc = g.product(Pv, Xv, Wv.T());
    h.A = X; h.B = W; h.C = P; h.M = 5; h.N = 7; h.K = 12; h.lda = 16; h.ldb = 16; h.sA1 = 80; h.sCi = 8; h.sC1 = 40;
    report("T() of B", rc == OK && same(g, h));
  }
  {   // T() of A and a stored K x N B: Q[s] = X[s]^T P[s]
    GemmArgs g = typed(GEMM_F32, GEMM_F32), h = g;
    const int rc = g.product(Qv, Xv.T(), Pv);
    h.A = X; h.B = P; h.C = Q; h.M = 12; h.N = 7; h.K = 5; h.a_layout = h.b_layout = MN_MAJOR; h.lda = 16; h.ldb = 8; h.sA1 = 80; h.sB1 = 40; h.sCi = 8; h.sC1 = 96;
    report("T() of A", rc == OK && same(g, h));
  }
  {   // rows_at / cols_at: rows 1..3 of X[s] against columns 4..11 of rows 2..6 of W; the pointer moves by the view's own element bytes
    GemmArgs g = typed(GEMM_F32, GEMM_F32), h = g;
    const int rc = g.product(Pv.rows_at(1, 3).cols_at(2, 5), Xv.rows_at(1, 3).cols_at(4, 8), Wv.rows_at(2, 5).cols_at(4, 8).T());
    h.A = X + 16 + 4; h.B = W + 2 * 16 + 4; h.C = P + 8 + 2; h.M = 3; h.N = 5; h.K = 8; h.lda = 16; h.ldb = 16; h.sA1 = 80; h.sCi = 8; h.sC1 = 40;
    report("rows_at / cols_at (fp32)", rc == OK && same(g, h));
    GemmArgs g2 = typed(GEMM_BF16, GEMM_BF16), h2 = g2;
    const int rc2 = g2.product(Ov.rows_at(3, 4), Hv.rows_at(3, 4).cols_at(1, 5), Uv.rows_at(1, 5));
    h2.A = H + 3 * 8 + 1; h2.B = U + 8; h2.C = O + 3 * 8; h2.M = 4; h2.N = 3; h2.K = 5; h2.b_layout = MN_MAJOR; h2.lda = 8; h2.ldb = 8; h2.sA1 = 192; h2.sCi = 8; h2.sC1 = 192;
    report("rows_at / cols_at (bf16)", rc2 == OK && same(g2, h2));
  }
  {   // flat(): both frames of H as one 48-row matrix: O = H U
    GemmArgs g = typed(GEMM_BF16, GEMM_BF16), h = g;
    const int rc = g.product(Ov.flat(2), Hv.flat(2), Uv);
    h.A = H; h.B = U; h.C = O; h.M = 48; h.N = 3; h.K = 6; h.b_layout = MN_MAJOR; h.lda = 8; h.ldb = 8; h.sCi = 8;
    report("flat()", rc == OK && same(g, h));
  }
  {   // groups(): the 12 columns of X and of W in 2 groups of 6 as the second batch level; frames of a matrix view
    GemmArgs g = typed(GEMM_F32, GEMM_F32), h = g;
    const Mat Rg = mat(R, 4, 5, 14, 24, 5 * 24).groups(2), Wg = Wv.groups(2);
    const int rc = g.product(Rg, Xv.groups(2), Wg.T());
    h.A = X; h.B = W; h.C = R; h.M = 5; h.N = 7; h.K = 6; h.lda = 16; h.ldb = 16; h.sA1 = 80; h.sA2 = 6; h.sB2 = 6; h.sCi = 24; h.sC1 = 120; h.sC2 = 7;
    report("groups()", rc == OK && same(g, h));
  }
  {   // row blocks: H[s] as 3 slots of 8 rows of which 6 are used: G[s][slot] = H_slot H_slot^T, stacked 6-row blocks of a 24-wide fp32... in bf16 here
    GemmArgs g = typed(GEMM_BF16, GEMM_F32), h = g;
    const Mat Hb = Hv.row_blocks(8, 6), Gv = mat(R, 4, 18, 6, 8, 18 * 8).row_blocks(6, 6);
    const int rc = g.product(Gv, Hb, Hb.T());
    h.A = H; h.B = H; h.C = R; h.M = 6; h.N = 6; h.K = 6; h.lda = 8; h.ldb = 8; h.sA1 = h.sB1 = 192; h.sA2 = h.sB2 = 64; h.sCi = 8; h.sC1 = 144; h.sC2 = 48;
    report("row_blocks()", rc == OK && same(g, h));
  }
  {   // planes: whole copies of H, 2 * 24 * 8 elements apart, as the second batch level: G[s][plane] = H^T H
    GemmArgs g = typed(GEMM_BF16, GEMM_F32), h = g;
    const Mat Hp = Hv.planes(384), Gv = mat(R, 4, 12, 6, 8, 12 * 8).row_blocks(6, 6);
    const int rc = g.product(Gv, Hp.T(), Hp);
    h.A = H; h.B = H; h.C = R; h.M = 6; h.N = 6; h.K = 24; h.a_layout = h.b_layout = MN_MAJOR; h.lda = 8; h.ldb = 8; h.sA1 = h.sB1 = 192; h.sA2 = h.sB2 = 384;
    h.sCi = 8; h.sC1 = 96; h.sC2 = 48;
    report("planes()", rc == OK && same(g, h));
  }
  {   // frames_at(): from frame 1 on
    GemmArgs g = typed(GEMM_F32, GEMM_F32), h = g;
    const int rc = g.product(Pv.frames_at(1), Xv.frames_at(1), Wv.T());
    h.A = X + 80; h.B = W; h.C = P + 40; h.M = 5; h.N = 7; h.K = 12; h.lda = 16; h.ldb = 16; h.sA1 = 80; h.sCi = 8; h.sC1 = 40;
    report("frames_at()", rc == OK && same(g, h));
  }
  {   // a transposed C: (X[s] W^T)^T stored 7 x 5 with ld 8
    GemmArgs g = typed(GEMM_F32, GEMM_F32), h = g;
    const Mat Ct = mat(R, 4, 7, 5, 8, 7 * 8);
    const int rc = g.product(Ct.T(), Xv, Wv.T());
    h.A = X; h.B = W; h.C = R; h.M = 5; h.N = 7; h.K = 12; h.lda = 16; h.ldb = 16; h.sA1 = 80; h.sCi = 1; h.sCj = 8; h.sC1 = 56;
    report("transposed C", rc == OK && same(g, h));
  }
  {   // a second segment and a D term: P[s] = X[s] W^T + Q[s]^T ... as  X[s] (5 x 12) W^T (12 x 7)  +  X[s] (5 x 12) Q[s] (12 x 7)  + rs P'[s]
    GemmArgs g = typed(GEMM_F32, GEMM_F32), h = g;
    const Mat Dv = mat(R, 4, 5, 7, 24, 5 * 24);
    int rc = g.product(Pv, Xv, Wv.T());
    if (rc == OK) rc = g.add_segment(1, Xv, Qv);
    if (rc == OK) rc = g.add_term(Dv);
    h.A = X; h.B = W; h.C = P; h.M = 5; h.N = 7; h.K = 12; h.lda = 16; h.ldb = 16; h.sA1 = 80; h.sCi = 8; h.sC1 = 40;
    h.seg[0].A = X; h.seg[0].B = Q; h.seg[0].K = 12; h.seg[0].b_layout = MN_MAJOR; h.seg[0].lda = 16; h.seg[0].ldb = 8; h.seg[0].sA1 = 80; h.seg[0].sB1 = 96;
    h.D = R; h.sDi = 24; h.sD1 = 120;
    report("second segment + D term", rc == OK && same(g, h));
    // ---- the refusals ----
    report("refuses: segment shape", refused(g.add_segment(2, Xv.rows_at(0, 4), Qv)) && !g.seg[1].A);
    report("refuses: segment K", refused(g.add_segment(2, Xv, Qv.rows_at(0, 11))));
    report("refuses: D shape", refused(g.add_term(Dv.cols_at(0, 6))));
    report("refuses: D element bytes", refused(g.add_term(Ov)));
  }
  {
    GemmArgs g = typed(GEMM_F32, GEMM_F32);
    report("refuses: K mismatch", refused(g.product(Pv, Xv, Wv.cols_at(0, 11).T())));
    report("refuses: C shape (rows)", refused(g.product(Pv.rows_at(0, 4), Xv, Wv.T())));
    report("refuses: C shape (columns)", refused(g.product(Pv.cols_at(0, 6), Xv, Wv.T())));
    report("refuses: C not transposed", refused(g.product(mat(R, 4, 7, 5, 8), Xv, Wv.T())));
    report("refuses: A bytes vs dtype", refused(g.product(Ov, Hv, Uv)));
    GemmArgs b = typed(GEMM_BF16, GEMM_F32);
    report("refuses: C bytes vs out", refused(b.product(Ov, Hv, Uv)));
    // flat() of frames that do not abut: X's frames are 80 elements apart, a 4-row block of them is 64
    const Mat bad = Xv.rows_at(0, 4).flat(2);
    report("refuses: flat() apart", bad.esz == 0 && g_err[0] != 0 && refused(g.product(Pv.rows_at(0, 4).flat(2), bad, Wv.T())));
  }
  std::printf(g_bad ? "FAILED: %d\n" : "ok\n", g_bad);
  return g_bad ? 1 : 0;
}
