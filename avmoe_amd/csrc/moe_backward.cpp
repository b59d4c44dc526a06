// Backward orchestration of one MoEAdapter site.  Mirrors oracle/algebra_ref.py::AlgebraRef.backward:
// phase 1 the two GEMMs against dOut, phases 2-4 bottleneck / weight space, phase 5 GEMMs against X,
// phase 6 the hop-1 (latent token) chain back to Y and the remap parameters.  Stream-ordered, no
// allocation, no host sync.
#include <functional>
#include "pass.h"
#include "moe_run.h"
#include "side.h"
#include "site_views.h"

namespace avmoe {

// Zero fill of a workspace range by a kernel of the library (bwd_kernels.hip), not hipMemsetAsync: in a captured graph the runtime's memset
// node cleared the range on the first replay only -- from the second replay on the accumulators started from garbage
// (tests/test_mix_drop_gpu.py replays a captured step three times; a kernel node replays like every other launch of the call).
#define MEMSET0(ptr, bytes) AVMOE_TRY(k_zero_bytes((ptr), (bytes), st))

avmoe_moe_ptrs with_unit_gates(const Plan& pl, const avmoe_moe_ptrs& prm, char* sv);   // moe_forward.cpp
int k_zero_bytes(void* ptr, size_t bytes, hipStream_t st);                                // bwd_kernels.hip
static const char* at(const char* base, size_t off) { return base ? base + off : nullptr; }      // (the query of moe_backward_dx_dy has no buffers)

// parts: bit mask of the sections to run, 0 = 7 = the whole backward:
//   1  phases 1-4: the GEMMs against dOut and the bottleneck / weight space (touches neither dX nor dY)
//   2  phase 5: the GEMMs against X -- every writer of dX ;  in two steps (plain sites only): 32 = phase 5 without the dX product
//      (touches neither dX nor dY), 64 = the dX product alone -- or moe_backward_dx_dy below in its place
//   4  phase 6: the hop-1 chain back to Y and the remap parameters -- every writer of dY;  in two steps: 8 = phase 6 without the
//      GEMM(s) that write dY (touches neither dX nor dY), 16 = those GEMMs alone (after 8)
// Sections are stream-ordered through `scratch`: a caller may put event records / waits between them (AdapterPair orders the
// two sites' accumulations into the shared token gradients this way) but nothing that touches the workspaces.
// the operands of  dX[s] = dZx[s] Wt + [dL2 | dsx | 1][s] [T ; 1 ; dm1/N][s] + 2 dSxx X[s]  (phase 5; moe_backward_dx_dy adds the other site's dY to it)
static int dx_product(GemmArgs& g, const Plan& pl, const void* X, const char* sv, const char* sc, void* dX) {
  const Dims& d = pl.d;
  g.out_dtype = d.bf16 ? GEMM_BF16 : GEMM_F32;
  AVMOE_TRY(g.product(views::tokens_x(d, dX).groups(d.g), views::Zw(pl, sc).groups(d.g), views::Wt(pl, sv)));
  AVMOE_TRY(g.add_segment(1, views::dL2x(pl, sc), views::Text(pl, sv).groups(d.g)));
  AVMOE_TRY(g.add_term(views::tokens_x(d, X).groups(d.g)));
  g.nb1 = d.S; g.nb2 = d.g; g.row_scale = (const float*)at(sc, pl.o_rs2x); g.sRS1 = d.N;
  return OK;
}

int moe_backward(const Plan& pl, const void* X, const void* Y, const avmoe_moe_ptrs& prm_in, const void* dOut, const float* lb_grad,
                 char* sv, char* sc, void* dX, void* dY, const avmoe_moe_ptrs& grads_in, hipStream_t st, int parts, const float* dprobs,
                 const float* aux_grad, const float* mix_scale) {
  const Dims& d = pl.d;
  if (parts == 0) parts = 7;
  if ((parts & (32 | 64)) && (d.Kcx > 0 || d.mha || d.nxn)) { set_last_error("split backward: sections 32 / 64 serve plain sites only (this one goes on accumulating into dX)"); return ERR_UNSUPPORTED; }
  if ((parts & 2) && (parts & (32 | 64))) { set_last_error("split backward: section 2 IS sections 32 + 64"); return ERR_BAD_ARG; }
  if ((parts & 7) != 7 && d.Kcx > 0) { set_last_error("split backward: sites with latent self attention write dX in the last section"); return ERR_UNSUPPORTED; }
  avmoe_moe_ptrs prm = with_unit_gates(pl, prm_in, sv);
  avmoe_moe_ptrs grads = grads_in;
  if (d.mg) { prm = merged_params(pl, prm, sv); grads = merged_grads(pl, grads_in, sc); }     // the forward left the dense copies in `saved`
  const int dt = d.bf16 ? GEMM_BF16 : GEMM_F32;
  float* slabs = (float*)(sc + pl.o_slabs);
  const size_t slab_cap = slab_floats(d);
  auto base = [&](int out_dt = GEMM_F32) { GemmArgs g; g.dtype = dt; g.out_dtype = out_dt; g.slabs = slabs; g.split3 = AVMOE_BWD_PLANES; return g; };      // (split3: fp32 sites only, gemm.h; moe_run.h: two planes in the backward)
  auto run_on = [&](GemmArgs& g, bool split, hipStream_t on) {
    if (split) g.ksplit = choose_ksplit(g, slab_cap);
    return launch_gemm(g, on);
  };
  auto run = [&](GemmArgs& g, bool split) { return run_on(g, split, st); };
  auto engine = [&](bool split) { return [&run_on, split](GemmArgs& g, hipStream_t on) { return run_on(g, split, on); }; };      // ... as the last form of a chain (forms.h)
  // fp32 sites: products whose result is a parameter gradient or a token gradient (nothing downstream forms a cancelling sum from it) in the
  // TWO-plane form (gemm.hip: f32s2; moe_run.h: AVMOE_LEAF2 has the classes and the measurement).  bf16 sites ignore split3.
  const Switches& sw = switches();
  auto leaf = [&](GemmArgs& g, int cls) { if (sw.leaf2 & cls) g.split3 = 2; };
  // Independent branches run on a helper stream (side.h) and are joined before their first consumer and before the section ends:
  //   section 1: dBpost = dOut^T Apost (+ its split-K reduce; the only user of the slabs until the join) beside dApost -> post_small_bwd -> Gram
  //   section 2: the dX GEMM (nothing in this call reads dX) beside the dWt / dT chain
  Side* side = side_worth(d) ? side_acquire(st) : nullptr;
  SideScope fk1(side, st), fk2(side, st);                  // joined on every way out (error returns included)
  const size_t esz = d.esz;
  // the site's tensors (site_views.h); `f`: all frames as one matrix, `g`: the channel groups as the second batch level
  namespace vw = views;
  const Mat Xs = vw::tokens_x(d, X), Ys = vw::tokens_y(d, Y), dXs = vw::tokens_x(d, dX), Xfg = Xs.flat(d.S).groups(d.g), dOfg = vw::tokens_x(d, dOut).flat(d.S).groups(d.g);
  const Mat Wt = vw::Wt(pl, sv), Text = vw::Text(pl, sv), WfT = vw::WfT(pl, sv), T0 = vw::T0T(pl, sv), WcK = vw::WcK(pl, sv), Qx = vw::Qx(pl, sv), BmX = vw::BmX(pl, sv);
  const Mat Zw = vw::Zw(pl, sc), Zwfg = Zw.flat(d.S).groups(d.g), dZRfg = vw::dZR(pl, sc).flat(d.S).groups(d.g), dxr = vw::dxr(pl, sc), dxrfg = dxr.flat(d.S).groups(d.g);
  const Mat dWt = vw::dWt(pl, sc), dTW = vw::dTW(pl, sc), dT = vw::dT(pl, sc), dTT = vw::dTT(pl, sc), dL2x = vw::dL2x(pl, sc), dT0 = vw::dT0(pl, sc);
  const Mat dTy = vw::dTy(pl, sc), dV = vw::dV(pl, sc), dBmT = vw::dBmT(pl, sc), dWcK = vw::dWcK(pl, sc), dRT = vw::dRT(pl, sc), dQT = vw::dQT(pl, sc), dWf = vw::dWf(pl, sc);
  // development builds: AVMOE_BWD_STOP=n returns after the n-th step of section 1 (1 the two GEMMs against dOut, 2 post_small_bwd, 3 the
  // Gram products, 4 post_prep_bwd, 5 mid_bwd, 6 router_bwd) -- workspaces as that step left them (tests/dev/race_buffers.py)
#define BWD_STOP(n) do { if (sw.bwd_stop == (n)) return OK; } while (0)
  if (parts & 1) {   // =============================== section 1: phases 1 - 4 ===============================
  // the accumulators that start from zero (dtbp, dTW, dWcK, dqp, dRT) are adjacent in the plan: one memset instead of five
  MEMSET0(sc + pl.o_dtbp, (pl.o_dRT - pl.o_dtbp) + (size_t)d.S * d.M * d.Kcyp * esz);

  // ---- phase 1: dApost = dOut Bpost ; dBpost = dOut^T Apost -------------------------------------
  // (the engine's Gram path splits K itself: it needs the slabs; sites on the generalised kernels keep post_small_bwd off the GPU while
  // a GEMM of the helper stream runs -- tile_gen.inc::gen_lds_request has the reason)
  const bool fork1 = side && (sw.side_mask & 2) && (d.gram64 || !d.ln_post) && !d.gen;
  int dap16 = 1;     // dApost stored as [E x 32 bottleneck columns in T | 3 E scalar columns in fp32 (dApx)]: the register-resident bf16 path
  const int npost = (d.KP % 4 == 0) ? d.KP : d.KPp;      // dApost's columns: KP, or the padded KPp when KP is not a multiple of 4 (2 or 3 experts): Bpost's
                                                         // padding columns are zero, the streaming kernel wants whole 4-column vectors, and nobody reads the padding of dAp
  const Mat Bpg = vw::Bpost(pl, sv).row_blocks(d.Cg, d.Cg).cols_at(0, npost);
  GemmArgs gb = base();                                    // dBpost = dOut^T Apost
  AVMOE_TRY(gb.product(vw::dBp(pl, sc).row_blocks(d.Cg, d.Cg).cols_at(0, d.KP), dOfg.T(), vw::Apost(pl, sv).groups(d.g).cols_at(0, d.KP)));
  gb.nb2 = d.g;
  leaf(gb, 1);
  GemmArgs ga = base();                                    // dApost = dOut Bpost
  AVMOE_TRY(ga.product(vw::dAp(pl, sc).groups(d.g).cols_at(0, npost), dOfg, Bpg));
  ga.nb2 = d.g;
  // ... as bf16 main columns + fp32 scalar columns (sites that keep z in bf16): 640 instead of 1152 bytes per token, written and re-read;
  // the T columns as rows of their own (E * dgp wide: whole 128-byte lines), not inside KPp-wide rows
  GemmArgs h = base(GEMM_BF16);
  h.Cx = (float*)(sc + pl.o_dApx); h.nsplit = d.E * d.dgp; h.ldcx = (long)d.g * d.XW; h.sCx2 = d.XW;
  AVMOE_TRY(h.product(vw::dAp_split(pl, sc).groups(d.g), dOfg, Bpg));
  h.nb2 = d.g;
  // The forms, in order: both products from one pass over dOut (dpost_pair.hip: the tuned bf16 shape); else dBpost on the engine (forked beside) and
  // dApost in its split form from the streaming GEMM; else dApost in one fp32 array from the engine (dap16 = 0)
  const bool split = d.zsz == 2;                           // (sites that keep z in bf16: a property of the plan, which no descriptor carries)
  auto dap_whole = [&](const GemmArgs&, hipStream_t on) { dap16 = 0; return launch_gemm(ga, on); };
  auto one_by_one = [&](const GemmArgs&, hipStream_t on) -> int {
    if (fork1) AVMOE_TRY(fk1.fork());
    AVMOE_TRY(run_on(gb, true, fork1 ? side->s : on));
    return split && !sw.dap_f32 ? try_forms(h, on, launch_gemm_stream, dap_whole) : dap_whole(ga, on);
  };
  AVMOE_TRY(split ? try_forms(gb, st, with(launch_dpost_pair, std::cref(h), slab_cap), one_by_one) : one_by_one(gb, st));
  BWD_STOP(1);
  // ---- phase 2: bottleneck space (LayerNorm-post statistics), then weight space ------------------
  PassCall pass(pl, sv, sc, prm);                          // (pass.h: each pass tries its forms in order)
  pass.dap16 = dap16;
  AVMOE_TRY(k_post_small_bwd(pass, grads, st));
  BWD_STOP(2);
  if (d.ln_post && d.gram64 && pass.streamed()) {
    // (dGq came out of post_small_bwd's own pass: tile_stream.hip)
  } else if (d.ln_post && d.gram64) {                      // dG[i][e] = sum_t dSoo z' z'^T : one streaming pass over z (z' formed on the fly)
    AVMOE_TRY(k_gram64(pl, sv + pl.o_Z, (const float*)(sc + pl.o_dSooT), 1.f, (float*)(sc + pl.o_gpartT), (float*)(sc + pl.o_dGq), st,
                       (const float*)(sv + pl.o_bn1)));
  } else if (d.ln_post) {                                  // ... as batched engine GEMMs on Zw = dSoo z'
    GemmArgs g = base();
    AVMOE_TRY(g.product(vw::dGq(pl, sc).row_blocks(d.dgp, d.dgp), Zw.flat(d.S).groups(d.g * d.E).T(), vw::Zp(pl, sc).flat(d.S).groups(d.g * d.E)));
    g.nb2 = d.g * d.E;
    AVMOE_TRY(run(g, true));
  }
  if (fk1.open) AVMOE_TRY(fk1.join());                     // (forked only when dpost_pair did not serve)
  BWD_STOP(3);
  AVMOE_TRY(k_post_prep_bwd(pl, sv, sc, prm, grads, st));
  BWD_STOP(4);
  // ---- phase 3: ReLU / BN1 ; router --------------------------------------------------------------
  AVMOE_TRY(k_mid_bwd(pass, grads, st));
  BWD_STOP(5);
  AVMOE_TRY(k_router_bwd(pl, sv, sc, prm, grads, lb_grad, dprobs, st, aux_grad, mix_scale));
  BWD_STOP(6);
  // ---- phase 4: folded LayerNorm / hop-2 softmax ---------------------------------------------------
  if (d.nxn) MEMSET0(sc + pl.o_dZR, (size_t)d.NT * d.DZ * esz);
  AVMOE_TRY(k_pre_small_bwd(pass, grads, st));
  }
  if (parts & (2 | 32 | 64)) {   // =============================== section 2: phase 5 ====================================
  const bool do_dx = (parts & (2 | 64)) != 0, do_rest = (parts & (2 | 32)) != 0;
  const bool fork2 = side && (sw.side_mask & 4) && !d.mha && !d.nxn && (parts & 2);             // (those variants go on accumulating into dX below)

  // ---- phase 5: GEMMs against X --------------------------------------------------------------------
  if (do_dx) {   // dX[s] = dZx[s] Wt + [dL2 | dsx | 1][s] [T ; 1 ; dm1/N][s] + 2 dSxx X[s]   -- one pass: two K segments + row-scale epilogue
    GemmArgs g = base();
    AVMOE_TRY(dx_product(g, pl, X, sv, sc, dX));
    g.accumulate = d.acc_dx;
    leaf(g, 16);
    if (fork2) AVMOE_TRY(fk2.fork());
    AVMOE_TRY(try_forms(g, fork2 ? side->s : st, launch_dx_stream2, engine(false)));      // (dx_stream2.hip: the eight-wave direct-load form of the tuned bf16 shape)
  }
  if (do_rest) {
  if (d.mha) {   // ---- AVS "v1": per expert back through ZR = xr Wt_e^T, the row sums and xr = MHA_e(X) - X -------------------
    for (int e = 0; e < d.E; ++e) {
      if (!d.nxn_of_e[e]) continue;
      const int slot = d.xr_of_e[e];
      {                                                    // dxr = dZR[:, expert e] Wt_e + (2 dSxx) xr
        GemmArgs g = base(dt);
        AVMOE_TRY(g.product(dxrfg, dZRfg.cols_at(e * d.dgp, d.dgp), Wt.rows_at(e * d.dgp, d.dgp)));
        AVMOE_TRY(g.add_term(vw::xr(pl, sv, slot).flat(d.S).groups(d.g)));
        g.nb2 = d.g; g.row_scale = (const float*)(sc + pl.o_dsr) + (size_t)slot * 3 * d.NT + d.NT;
        AVMOE_TRY(run(g, false));
      }
      AVMOE_TRY(k_nxn_axpy(pl, X, sv, sc, dX, slot, 1, st));   // dxr += dsr2 X + dsr0 ; dX += dsr2 xr - dxr (input replaced)
      AVMOE_TRY(mha_frames_backward(pl, X, prm.e[e], grads.e[e], slot, sc + pl.o_dxr, sv, sc, slabs, slab_cap, dX, st));
    }
  } else if (d.nxn) {   // ---- AVVP N x N block: back through ZR = xr Wt^T, the three row sums and xr = att^T X --------------------
    {                                                      // dxr = dZR Wt + (2 g^2 dSxx) xr
      GemmArgs g = base(dt);
      AVMOE_TRY(g.product(dxrfg, dZRfg, Wt));
      AVMOE_TRY(g.add_term(vw::xr(pl, sv, 0).flat(d.S).groups(d.g)));
      g.nb2 = d.g; g.row_scale = (const float*)(sc + pl.o_dsr) + d.NT;
      AVMOE_TRY(run(g, false));
    }
    AVMOE_TRY(k_nxn_axpy(pl, X, sv, sc, dX, 0, 0, st));      // dxr += dsr2 X + dsr0 ; dX += dsr2 xr
    for (int s0 = 0; s0 < d.S; s0 += d.nxc) {              // d.nxc frames at a time (all of them when the forward kept att: moe_plan.cpp)
      const int ns = std::min(d.nxc, d.S - s0);
      const Mat Xm = Xs.frames_at(s0), dxm = dxr.frames_at(s0), dXm = dXs.frames_at(s0), att = vw::att(pl, sv), dSc = vw::dSc(pl, sc);
      const void* Xc = Xm.p; const void* dxc = dxm.p; void* dXc = (void*)dXm.p;
      const int Np = (int)att.ld;                          // (row stride of att / dSc: what the strip kernels take)
      if (d.nflash) {
        // the strip kernels re-form att from the kept row log-sum-exp in their accumulators: neither the softmax nor y = att dxr exists in memory
        const float* lse = (const float*)(sv + pl.o_nlse) + (size_t)s0 * d.N;
        AVMOE_TRY(k_nxn_y(Xc, dxc, ns, d.N, d.C, Np, lse, (float*)(sc + pl.o_nrd), dXc, st));           // rowdot = X . (att dxr) ; dX += att dxr
        // dX += dS X + dS^T X, dS = att * (X dxr^T - rowdot) formed in the accumulators of both kernels
        AVMOE_TRY(k_nxn_dx(0, Xc, dxc, ns, d.N, d.C, Np, lse, (const float*)(sc + pl.o_nrd), dXc, st));
        AVMOE_TRY(k_nxn_dx(1, Xc, dxc, ns, d.N, d.C, Np, lse, (const float*)(sc + pl.o_nrd), dXc, st));
        continue;
      } else {
        if (d.nxc < d.S && nxn_att_ok(d.bf16, d.N, d.C, Np)) {
          AVMOE_TRY(k_nxn_att(Xc, ns, d.N, d.C, Np, (float*)(sv + pl.o_nlse) + (size_t)s0 * d.N, sv + pl.o_att, 1, st));
        } else if (d.nxc < d.S) {                            // the forward ran in chunks too: att of these frames again, from the kept row log-sum-exp
          GemmArgs g = base(dt);
          AVMOE_TRY(g.product(att, Xm, Xm.T()));
          g.nb1 = ns;
          g.epi = GEMM_EPI_EXP; g.row_lse = (const float*)(sv + pl.o_nlse) + (size_t)s0 * d.N;
          g.split3 = AVMOE_FWD_SPLIT3;                       // (the forward's arithmetic: the chunked site must re-form the very att the unchunked one kept)
          AVMOE_TRY(run(g, false));
        }
        {                                                    // y[s] = att[s] dxr[s]   (fp32): the direct term of dX and the softmax's row term
          GemmArgs g = base();
          AVMOE_TRY(g.product(vw::nyt(pl, sc), att, dxm));
          g.nb1 = ns;
          AVMOE_TRY(run(g, true));
        }
        // dX[s] += y[s] ; rowdot_i = X_i . y_i  ( = sum_j att_ij d att_ij, with d att_ij = X_i . dxr_j )
        AVMOE_TRY(k_nxn_rowdot(d.bf16, Xc, (const float*)(sc + pl.o_nyt), (long)ns * d.N, d.C, dXc, (float*)(sc + pl.o_nrd), st));
        if (nxn_att_ok(d.bf16, d.N, d.C, Np)) {            // dSc[s] = att[s] * (X[s] dxr[s]^T - rowdot): d att never leaves the chip
          AVMOE_TRY(k_nxn_att_bwd(Xc, dxc, ns, d.N, d.C, Np, (const float*)(sc + pl.o_nrd), sv + pl.o_att, sc + pl.o_dSc, st));
        } else {
          GemmArgs g = base(dt);
          AVMOE_TRY(g.product(dSc, Xm, dxm.T()));
          AVMOE_TRY(g.add_term(att));
          g.nb1 = ns; g.epi = GEMM_EPI_MULSUB; g.row_lse = (const float*)(sc + pl.o_nrd);
          AVMOE_TRY(run(g, false));
        }
      }
      for (int tr = 0; tr < 2; ++tr) {                     // dX[s] += dSc[s] X[s]  and  dSc[s]^T X[s]
        GemmArgs g = base(dt);
        AVMOE_TRY(g.product(dXm, tr ? dSc.T() : dSc, Xm));
        g.nb1 = ns; g.accumulate = 1;
        AVMOE_TRY(run(g, true));
      }
    }
  }
  if (d.El > 0) {                                          // dTW[s][slot l] = gate * a^T dzraw  (own expert's columns), all slots in one launch
    const int e0 = d.e_of_lat[0];                          // (latent experts are consecutive: the multimodal ones come first, AVS v2 makes all of them latent)
    GemmArgs g = base(dt);
    AVMOE_TRY(g.product(dTW.rows_at(0, d.K).groups(d.g).cols_at(e0 * d.dgp, d.dgp), vw::ag(pl, sc).T(), Zw.groups(d.g).cols_at(e0 * d.dgp, d.dgp)));
    g.nb1 = d.S; g.nb2 = d.g; g.nb3 = d.El;               // third level: the latent slots -- ag's planes, the experts' columns, dTW's Kp-row slots
    g.sA3 = d.aL; g.sB3 = d.dgp; g.sC3 = (long)d.Kp * d.DZ + d.dgp;
    AVMOE_TRY(run(g, false));
  }
  bool pair_done = d.bf16 && d.El > 0;                     // dWt = dZx^T X and dT[s] = dL2[s]^T X[s] in ONE pass over X (bf16 sites with latent tokens: TokPairArgs has no dtype)
  if (pair_done) {
    const Mat l2 = dL2x.cols_at(0, d.KL);
    TokPairArgs t{Zwfg.p, Zwfg.ld, Zwfg.cols, Zwfg.s2, l2.p, l2.ld, l2.cols, Xs.p, Xs.ld, d.S, d.N, d.g, d.Cg, (float*)dWt.p, (float*)dT.p, slabs, slab_cap};
    // as one streaming pass with every accumulator in registers (tok_pair2.hip: the tuned shape), or in the tiled form, or as the two engine products below
    auto two_products = [&](const TokPairArgs&, hipStream_t) { pair_done = false; return (int)OK; };
    AVMOE_TRY(try_forms(t, st, launch_tok_pair2, launch_gemm_tokpair, two_products));
  }
  {                                                        // dWt = dZx^T X  + dTW^T Text
    GemmArgs g = base();
    AVMOE_TRY(g.product(dWt, Zwfg.T(), Xfg));
    g.nb2 = d.g;
    leaf(g, 2);
    if (!pair_done) AVMOE_TRY(run(g, true));
    if (d.El > 0) {
      GemmArgs h = g;
      AVMOE_TRY(h.product(dWt, dTW.flat(d.S).groups(d.g).T(), Text.flat(d.S).groups(d.g)));
      h.accumulate = 1; h.ksplit = 1;
      AVMOE_TRY(run(h, true));
    }
    if (d.mha) {                                           // + dZR[:, expert e]^T xr_e
      for (int e = 0; e < d.E; ++e) {
        if (!d.nxn_of_e[e]) continue;
        GemmArgs h = g;
        AVMOE_TRY(h.product(dWt.rows_at(e * d.dgp, d.dgp), dZRfg.cols_at(e * d.dgp, d.dgp).T(), vw::xr(pl, sv, d.xr_of_e[e]).flat(d.S).groups(d.g)));
        h.accumulate = 1; h.ksplit = 1;
        AVMOE_TRY(run(h, true));
      }
    } else if (d.nxn) {                                    // + dZR^T xr
      GemmArgs h = g;
      AVMOE_TRY(h.product(dWt, dZRfg.T(), vw::xr(pl, sv, 0).flat(d.S).groups(d.g)));
      h.accumulate = 1; h.ksplit = 1;
      AVMOE_TRY(run(h, true));
    }
  }
  if (d.El > 0) {
    if (!pair_done) {                                      // dT[s] = dL2[s]^T X[s]
      GemmArgs g = base();
      AVMOE_TRY(g.product(dT, dL2x.cols_at(0, d.KL).T(), Xs));
      g.nb1 = d.S;
      leaf(g, 4);
      AVMOE_TRY(run(g, false));
    }
    {                                                      // dT += dTW Wt
      GemmArgs g = base();
      AVMOE_TRY(g.product(dT.groups(d.g), dTW.rows_at(0, d.KL).groups(d.g), Wt));
      g.nb1 = d.S; g.nb2 = d.g; g.accumulate = 1;
      AVMOE_TRY(run(g, false));
    }
    {                                                      // dTT[s][l] = sum_t du3 a a^T   (symmetric)
      GemmArgs g = base(dt);
      AVMOE_TRY(g.product(dTT.row_blocks(d.K, d.K), vw::aw(pl, sc).planes(d.aL).T(), vw::a(pl, sv).planes(d.aL)));      // (aw, a: per-slot planes)
      g.nb1 = d.S; g.nb2 = d.El;
      AVMOE_TRY(run(g, false));
    }
    {                                                      // dT += 2 dTT T
      GemmArgs g = base();
      AVMOE_TRY(g.product(dT.row_blocks(d.Kp, d.K), dTT.row_blocks(d.K, d.K), Text.row_blocks(d.Kp, d.K)));
      g.nb1 = d.S; g.nb2 = d.El; g.alpha = 2.f; g.accumulate = 1;
      AVMOE_TRY(run(g, false));
    }
  }
  AVMOE_TRY(k_finish_dT(pl, sv, sc, st));                  // + dtbar / C ; dTy (T, with the dm2 row) ; dTx ; dT0 ; drw, dbf
  AVMOE_TRY(k_down_bwd(pl, sc, prm, grads, st));
  if (d.mg) AVMOE_TRY(k_merge_gather(pl, sc, grads_in, st));   // diagonal blocks of the dense weight gradients -> the caller's grouped ones
  }
  if (fork2) AVMOE_TRY(fk2.join());
  }
  // ======================= section 3: phase 6 (4 = all of it; 8 = everything but the writers of dY; 16 = the writers of dY) ==========
  const bool do6a = (parts & (4 | 8)) != 0, do6b = (parts & (4 | 16)) != 0;
  if (!do6a && !do6b) return OK;

  if (do6a) {
  // ---- phase 6a: cross-modal hop-1 chain back to Y and the remap parameters -------------------------
  {                                                        // dV = dTy Wf   (row Kcy: d ybar)
    GemmArgs g = base(dt);
    AVMOE_TRY(g.product(dV.flat(d.S), dTy.flat(d.S), WfT));
    AVMOE_TRY(run(g, false));
  }
  {                                                        // dWf = dTy^T V
    GemmArgs g = base();
    AVMOE_TRY(g.product(dWf, dTy.flat(d.S).T(), vw::V(pl, sv).flat(d.S)));
    leaf(g, 8);
    AVMOE_TRY(run(g, true));
  }
  {                                                        // dBm[s] = dV[s] Y[s]^T
    GemmArgs g = base();
    AVMOE_TRY(g.product(vw::dBm(pl, sc).cols_at(0, d.M), dV, Ys.T()));
    g.nb1 = d.S;
    AVMOE_TRY(try_forms(g, st, launch_hop1_yk, engine(false)));      // (hop1_stream.hip: dV[s] stationary per frame)
  }
  AVMOE_TRY(k_prep_dBm(pl, sc, st));
  }
  if (d.Kcy > 0 && do6a) {
    {                                                      // dA1[s] = [dBm | dab][s] [Wc | bc]^T
      GemmArgs g = base();
      AVMOE_TRY(g.product(vw::L1(pl, sc, d.Kcyb), dBmT, WcK.cols_at(0, d.M + 1).T()));
      g.nb1 = d.S;
      AVMOE_TRY(run(g, false));
    }
    {                                                      // dWcK[:, :M+1] += A1^T [dBm | dab]
      GemmArgs g = base();
      AVMOE_TRY(g.product(dWcK.cols_at(0, d.M + 1), vw::A1y(pl, sv).flat(d.S).T(), dBmT.flat(d.S)));
      g.accumulate = 1;
      leaf(g, 8);
      AVMOE_TRY(run(g, true));
    }
    AVMOE_TRY(k_softmax_rows_bwd(d.bf16, sv + pl.o_A1y, (const float*)(sc + pl.o_L1), (long)d.S * d.Kcyb, d.N, (int)vw::A1y(pl, sv).ld,
                                 sc + pl.o_dL1, nullptr, 1, 1, st));
    {                                                      // dR[s]^T = (dL1[s] Wc)^T   stored [m][kc]
      GemmArgs g = base(dt);
      AVMOE_TRY(g.product(dRT.T(), vw::dL1(pl, sc, d.Kcyb).rows_at(0, d.Kcy), vw::WcT(pl, sv).rows_at(0, d.M).T()));
      g.nb1 = d.S;
      AVMOE_TRY(run(g, false));
    }
    {                                                      // dWcK[:, :M+2] += dL1^T [R | qr | qb]
      GemmArgs g = base();
      AVMOE_TRY(g.product(dWcK, vw::dL1(pl, sc, d.Kcyb).flat(d.S).T(), vw::Rext(pl, sv).flat(d.S)));
      g.accumulate = 1;
      leaf(g, 8);
      AVMOE_TRY(run(g, true));
    }
    AVMOE_TRY(k_dqrqb(pl, sc, prm.conv_b, st));
    {                                                      // dQ = sum_s dR[s] Y[s]
      GemmArgs g = base(dt);                               // (straight in the operand dtype of its two consumers)
      AVMOE_TRY(g.product(dQT, dRT.flat(d.S).T(), Ys.flat(d.S)));
      AVMOE_TRY(try_forms(g, st, with(launch_hop1_yt_sum, slab_cap), engine(true)));      // (hop1_stream.hip: one pass over Y with every accumulator in registers + a slab sum)
    }
  }
  if (do6b) {   // dY[s] = [Bm ; wbar][s]^T dV[s] + dR[s]^T Q   -- one pass over dY (two K segments; no cross-modal expert: wbar (x) d ybar[s] alone)
    GemmArgs g = base(dt);
    AVMOE_TRY(g.product(vw::tokens_y(d, dY), BmX.cols_at(0, d.M).T(), dV));
    if (d.Kcy > 0) AVMOE_TRY(g.add_segment(1, dRT, Qx));
    g.nb1 = d.S; g.accumulate = d.acc_dy;
    if (d.Kcy > 0) leaf(g, 16);                            // (the one-segment product has always stayed on AVMOE_BWD_PLANES)
    AVMOE_TRY(run(g, false));
  }
  if (d.Kcy > 0 && do6a) {
    {                                                      // dT0[y slots] += dQ Wf^T
      GemmArgs g = base();
      AVMOE_TRY(g.product(dT0.rows_at(0, d.Kcy), dQT, WfT.T()));
      g.accumulate = 1;
      AVMOE_TRY(run(g, false));
    }
    {                                                      // dWf += T0^T dQ
      GemmArgs g = base();
      AVMOE_TRY(g.product(dWf, T0.rows_at(0, d.Kcy).T(), dQT));
      g.accumulate = 1;
      leaf(g, 8);
      AVMOE_TRY(run(g, false));
    }
  }
  // ---- phase 6b: latent self attention on X (AVS v2) ----------------------------------------------
  if (d.Kcx > 0) {
    const Mat dTx = vw::dTx(pl, sc), A1x = vw::A1x(pl, sv), dL1xT = vw::dL1xT(pl, sc);
    {                                                      // dA1x[s] = dTx[s] X[s]^T
      GemmArgs g = base();
      AVMOE_TRY(g.product(vw::L1(pl, sc, d.Kcx), dTx, Xs.T()));
      g.nb1 = d.S;
      AVMOE_TRY(run(g, false));
    }
    {                                                      // dX[s] += A1x[s]^T dTx[s]
      GemmArgs g = base(dt);
      AVMOE_TRY(g.product(dXs, A1x.T(), dTx));
      g.nb1 = d.S; g.accumulate = 1;
      AVMOE_TRY(run(g, false));
    }
    MEMSET0(sc + pl.o_dL1xT, (size_t)d.NT * d.Kcxp * esz);
    AVMOE_TRY(k_softmax_rows_bwd(d.bf16, A1x.p, (const float*)(sc + pl.o_L1), (long)d.S * d.Kcx, d.N, (int)A1x.ld,
                                 sc + pl.o_dL1, (void*)dL1xT.p, d.Kcx, (int)dL1xT.ld, st));
    {                                                      // dT0[x slots] += sum_{s,n} dL1x^T X
      GemmArgs g = base();
      AVMOE_TRY(g.product(dT0.rows_at(d.Kcy, d.Kcx), dL1xT.flat(d.S).T(), Xs.flat(d.S)));
      g.accumulate = 1;
      AVMOE_TRY(run(g, true));
    }
    {                                                      // dX += dL1x^T T0x
      GemmArgs g = base(dt);
      AVMOE_TRY(g.product(dXs.flat(d.S), dL1xT.flat(d.S), T0.rows_at(d.Kcy, d.Kcx)));
      g.accumulate = 1;
      AVMOE_TRY(run(g, false));
    }
  }
  if (do6a) AVMOE_TRY(k_hop1_finalize(pl, sv, sc, prm, grads, st));
  return OK;
}

// The gradient of a token tensor that is X of site A and Y of site B (the two sites of one backbone layer), written once: site A's dX
// product with site B's dY product as two more K segments (dx_stream3.hip).  After sections 1 + 32 + 8 of BOTH sites; replaces section 64 of
// A and section 16 of B.  launch = false: only says whether the shapes are served.  0 = served (launched), 1 = not served, < 0 error.
int moe_backward_dx_dy(const Plan& pa, const void* X, char* sva, char* sca, const Plan& pb, char* svb, char* scb, void* dX, bool launch, hipStream_t st) {
  const Dims& a = pa.d;
  const Dims& b = pb.d;
  if (a.bf16 != b.bf16 || a.mha || a.nxn || a.Kcx > 0 || b.M != a.N || b.Cy != a.C || b.S != a.S || b.Kcx > 0) return 1;
  // site A's dX product with site B's  dY[s] = [Bm ; wbar][s]^T dV[s] + dR[s]^T Q  as a third and a fourth K segment (gemm.h: GemmArgs::seg)
  GemmArgs g; g.dtype = a.bf16 ? GEMM_BF16 : GEMM_F32; g.split3 = (AVMOE_LEAF2 & 16) ? 2 : AVMOE_BWD_PLANES;
  g.slabs = (float*)at(sca, pa.o_slabs);                   // (the streaming form's dump word)
  AVMOE_TRY(dx_product(g, pa, X, sva, sca, dX));
  AVMOE_TRY(g.add_segment(2, views::BmX(pb, svb).cols_at(0, b.M).T(), views::dV(pb, scb).groups(a.g)));
  if (b.Kcy > 0) AVMOE_TRY(g.add_segment(3, views::dRT(pb, scb), views::Qx(pb, svb).groups(a.g)));
  // The streaming form (dx_stream3.hip: the tuned bf16 shape), or, round 6, the same sum on the tiled engine: the token gradient is written
  // once instead of written by site A and read back + added by site B.  fp32 sites only (AVMOE_DXDY_GEN = 1; 3 = bf16 sites of the
  // generalised shapes too: measured, moe_run.h).
  const bool stream = !a.mg && !b.mg && dx_stream3_serves(g);
  if (!stream && !(AVMOE_DXDY_GEN & (a.bf16 ? 2 : 1))) return 1;
  if (!launch) return OK;
  return stream ? launch_dx_stream3(g, st) : launch_gemm(g, st);
}

}  // namespace avmoe
