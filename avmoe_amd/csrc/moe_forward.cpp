// Forward orchestration of one MoEAdapter site: a fixed sequence of engine GEMMs and bottleneck-space
// kernels on the caller's stream (no allocation, no host sync: capturable in a hipGraph).
// Stage names follow oracle/algebra_ref.py::AlgebraRef.forward.
#include "pass.h"
#include "moe_run.h"
#include "prof.h"
#include "side.h"
#include "site_views.h"

namespace avmoe {

int choose_ksplit(const GemmArgs& g, size_t slab_floats_cap) {
  const int tile = g.tile ? g.tile : gemm_auto_tile(g.M, g.N);
  const long nb = (long)g.nb1 * g.nb2 * (g.nb3 > 0 ? g.nb3 : 1);          // (every batch level has its own slabs: gemm_slab_bytes)
  const long tiles = (long)cdiv(g.M, tile) * cdiv(g.N, tile) * nb;
  const int bk = g.dtype == GEMM_BF16 ? 64 : 32;
  long ks = std::max<long>(1, switches().ks_target / std::max<long>(tiles, 1));      // (512 workgroups wanted)
  ks = std::min<long>(ks, std::max<long>(1, g.K / (4 * bk)));
  ks = std::min<long>(ks, 64);
  const size_t per = (size_t)nb * g.M * g.N;
  while (ks > 1 && per * ks > slab_floats_cap) --ks;
  return (int)ks;
}

// The "v1" experts run through the x + gate * xr code of the AVVP ones with gate 1: a device constant stands in for gate_av.
avmoe_moe_ptrs with_unit_gates(const Plan& pl, const avmoe_moe_ptrs& prm, char* sv) {
  avmoe_moe_ptrs p = prm;
  if (pl.d.mha)
    for (int e = 0; e < pl.d.E; ++e)
      if (pl.d.nxn_of_e[e]) p.e[e].gate_lat = (float*)(sv + pl.o_scal) + 1;
  return p;
}

int moe_forward(const Plan& pl, const void* X, const void* Y, const avmoe_moe_ptrs& prm_in, void* out, const RouteCall& route, char* sv, char* sc,
                hipStream_t st) {
  const Dims& d = pl.d;
  // Cumulative BatchNorm average (bn_momentum < 0): the statistic kernels form 1 / (counter + 1) on the device, so every counter must be there
  const bool cumul = d.use_bn && d.training && d.bn_momentum < 0.f;
  if (cumul)
    for (int e = 0; e < d.E; ++e)
      if (!prm_in.e[e].bn1_nbt || !prm_in.e[e].bn2_nbt) {
        set_last_error("moe_forward: bn_momentum < 0 (cumulative average) needs expert %d's %s (%s.num_batches_tracked)", e,
                       prm_in.e[e].bn1_nbt ? "bn2_nbt" : "bn1_nbt", prm_in.e[e].bn1_nbt ? "bn2" : "bn1");
        return ERR_BAD_ARG;
      }
  avmoe_moe_ptrs prm = with_unit_gates(pl, prm_in, sv);
  if (d.mg) {                                              // merged groups: run on block-diagonal dense copies of the grouped weights
    AVMOE_TRY(k_merge_expand(pl, sv, prm_in, st));
    prm = merged_params(pl, prm, sv);
  }
  const int dt = d.bf16 ? GEMM_BF16 : GEMM_F32;
  float* slabs = (float*)(sc + pl.o_slabs);
  const size_t slab_cap = slab_floats(d);
  auto base = [&](int out_dt = GEMM_F32) { GemmArgs g; g.dtype = dt; g.out_dtype = out_dt; g.slabs = slabs; g.split3 = AVMOE_FWD_SPLIT3; return g; };      // (split3: fp32 sites only, gemm.h)
  // the site's tensors (site_views.h); the token tensors all frames as one matrix too
  namespace vw = views;
  const Mat Xs = vw::tokens_x(d, X), Ys = vw::tokens_y(d, Y), Wt = vw::Wt(pl, sv), Text = vw::Text(pl, sv), WfT = vw::WfT(pl, sv), T0 = vw::T0T(pl, sv);
  const Mat Qx = vw::Qx(pl, sv), Rext = vw::Rext(pl, sv), A1y = vw::A1y(pl, sv), BmX = vw::BmX(pl, sv), V = vw::V(pl, sv), Z = vw::Z(pl, sv);

  // ---- weights-derived operands --------------------------------------------------------------
  AVMOE_TRY(k_prep_all(pl, sv, prm, st));                  // (also scal[1] = 1: the unit gate of with_unit_gates)
  // ---- token statistics of X: row sums (LayerNorm), column means (router) ---------------------
  if (!d.fuse_xs) AVMOE_TRY(k_xstats(pl, X, sv, sc, st));          // (fused: they come out of the down projection below)
  // Zx = X Wt^T per frame, with the row sums / column sums of X as side products (fused statistics).  It depends on X and the
  // weights only, the hop-1 chain below on Y and the weights only: the two run on two streams and meet at the router.
  auto fused_down = [&](hipStream_t xs) -> int {
    GemmArgs g = base(GEMM_BF16);
    int tiles = 0;
    AVMOE_TRY(g.product(Z.groups(d.g), Xs.groups(d.g), Wt.T()));
    g.nb1 = d.S; g.nb2 = d.g;
    g.st_rows = (float*)(sc + pl.o_sxp); g.st_cols = (float*)(sc + pl.o_xpart); g.st_ntot = d.NT; g.st_tiles = &tiles;
    if (d.fuse_l2) {                                       // + L2g[gi][s] = X[s][:, group gi] T[s][:, group gi]^T : the hop-2 logits, per group
      const Mat T = Text.groups(d.g), L = vw::L2g(pl, sc);
      g.xcols = {T.p, d.KL, T.ld, T.s1, T.s2, (float*)L.p, L.ld, L.s1, L.s2};
    }
    const int rc = launch_gemm_stream(g, xs);              // (the one form that leaves the statistics: no chain, no engine behind it)
    if (rc != OK) {
      if (rc == 1) set_last_error("moe_forward: the streaming down projection with statistics does not serve this shape (plan / kernel mismatch)");
      return rc == 1 ? ERR_UNSUPPORTED : rc;
    }
    if ((2L * d.NT) % 4 == 0)      // the two finishing sums (row sums over the groups, column means over the tiles) in one launch
      return k_xstats_fin((const float*)(sc + pl.o_sxp), d.g, 2L * d.NT, (float*)(sv + pl.o_sx), (const float*)(sc + pl.o_xpart), tiles, d.C, d.S,
                          (float*)(sv + pl.o_rin), 2L * d.C, 1.f / (float)d.N, xs);
    AVMOE_TRY(k_sum_parts((const float*)(sc + pl.o_sxp), d.g, 2L * d.NT, (float*)(sv + pl.o_sx), xs));
    return k_colsum_f32((const float*)(sc + pl.o_xpart), tiles, d.C, d.C, d.S, (long)tiles * d.C, (float*)(sv + pl.o_rin), 2L * d.C,
                        1.f / (float)d.N, xs);
  };
  // (with the logits fused in, the pass needs the latent tokens T: it runs behind the hop-1 chain, on the caller's stream)
  Side* side = (d.fuse_xs && !d.fuse_l2 && (switches().side_mask & 1) && side_worth(d)) ? side_acquire(st) : nullptr;
  SideScope fk(side, st);
  if (side) {
    AVMOE_TRY(fk.fork());
    AVMOE_TRY(fused_down(side->s));
  }

  // ---- hop 1, cross-modal experts: latent tokens read the (never materialised) remapped Y -----
  if (d.Kcy > 0) {
    GemmArgs g = base(dt);                                 // Q = T0 Wf
    AVMOE_TRY(g.product(Qx, T0.rows_at(0, d.Kcy), WfT));
    AVMOE_TRY(launch_gemm(g, st));
  }
  AVMOE_TRY(k_qrqb_fill(pl, sv, prm.fc_b, st));
  if (d.Kcy > 0) {
    {                                                      // R[s] = Q Y[s]^T
      GemmArgs g = base(dt);
      AVMOE_TRY(g.product(Rext.rows_at(0, d.Kcy).cols_at(0, d.M), Qx, Ys.T()));
      g.nb1 = d.S;
      AVMOE_TRY(try_forms(g, st, launch_hop1_yk, launch_gemm));      // (hop1_stream.hip: Q stationary, Y streamed in whole token rows)
    }
    {                                                      // L1[s] = [R | qr | qb] [Wc | bc | 1]^T
      GemmArgs g = base();
      AVMOE_TRY(g.product(vw::L1(pl, sc, d.Kcyb).rows_at(0, d.Kcy), Rext.rows_at(0, d.Kcy), vw::WcK(pl, sv).T()));
      g.nb1 = d.S;
      AVMOE_TRY(launch_gemm(g, st));
    }
    AVMOE_TRY(k_softmax_rows(d.bf16, (const float*)(sc + pl.o_L1), (long)d.S * d.Kcyb, d.N, vw::L1(pl, sc, d.Kcyb).ld, (void*)A1y.p, A1y.ld,
                             d.Kcyb, d.Kcy, d.Kp, d.K, st));
    {                                                      // [Bm | ab][s] = A1[s] [Wc | bc]
      GemmArgs g = base(dt);
      AVMOE_TRY(g.product(BmX.rows_at(0, d.Kcy), A1y.rows_at(0, d.Kcy), vw::WcT(pl, sv).T()));
      g.nb1 = d.S;
      AVMOE_TRY(launch_gemm(g, st));
    }
  }
  {                                                        // V[s] = [Bm ; wbar][s] Y[s]   (token contraction)
    GemmArgs g = base(dt);
    AVMOE_TRY(g.product(V, BmX.cols_at(0, d.M), Ys));
    g.nb1 = d.S;
    AVMOE_TRY(try_forms(g, st, launch_hop1_yt_frames, launch_gemm));      // (hop1_stream.hip)
  }
  {                                                        // TV = V Wf^T
    GemmArgs g = base();
    AVMOE_TRY(g.product(vw::TV(pl, sc, d.Kcyb).flat(d.S), V.flat(d.S), WfT.T()));
    AVMOE_TRY(launch_gemm(g, st));
  }
  AVMOE_TRY(k_finish_T(pl, sv, sc, prm, 0, st));

  // ---- hop 1, latent self attention on X (AVS v2) ----------------------------------------------
  if (d.Kcx > 0) {
    {                                                      // L1x[s] = T0x X[s]^T
      GemmArgs g = base();
      AVMOE_TRY(g.product(vw::L1(pl, sc, d.Kcx), T0.rows_at(d.Kcy, d.Kcx), Xs.T()));
      g.nb1 = d.S;
      AVMOE_TRY(launch_gemm(g, st));
    }
    AVMOE_TRY(k_softmax_rows(d.bf16, (const float*)(sc + pl.o_L1), (long)d.S * d.Kcx, d.N, vw::L1(pl, sc, d.Kcx).ld, (void*)vw::A1x(pl, sv).p, vw::A1x(pl, sv).ld,
                             d.Kcx, d.Kcx, d.Kp, d.K, st));
    {                                                      // TVx[s] = A1x[s] X[s]
      GemmArgs g = base();
      AVMOE_TRY(g.product(vw::TV(pl, sc, d.Kcx), vw::A1x(pl, sv), Xs));
      g.nb1 = d.S;
      AVMOE_TRY(launch_gemm(g, st));
    }
    AVMOE_TRY(k_finish_T(pl, sv, sc, prm, 1, st));
  }

  // ---- per-sample K-space matrices of the latent tokens ------------------------------------------
  // (row sums of Text: k_finish_T writes them with the rows, k_prep_all those of the constant rows)
  if (d.El > 0) {                                          // TT[s][l] = T T^T
    GemmArgs g = base();
    const Mat T = Text.row_blocks(d.Kp, d.K);              // (the K used rows of every latent slot)
    AVMOE_TRY(g.product(vw::TT(pl, sv).row_blocks(d.K, d.K), T, T.T()));
    g.nb1 = d.S; g.nb2 = d.El;
    AVMOE_TRY(launch_gemm(g, st));
  }
  auto down_gemm = [&](const Mat& rows, const Mat& dst) {    // rows (nrows, C) -> (nrows, DZ) through Wt
    GemmArgs g = base(dst.esz == 2 ? GEMM_BF16 : GEMM_F32);
    AVMOE_TRY(g.product(dst.groups(d.g), rows.groups(d.g), Wt.T()));
    g.nb2 = d.g;
    return launch_gemm(g, st);
  };
  AVMOE_TRY(down_gemm(Text.flat(d.S), vw::TW(pl, sv).flat(d.S)));          // TW (all latent rows x all experts)
  // ---- the X-side GEMMs ------------------------------------------------------------------------
  if (d.fuse_xs) {
    if (side) AVMOE_TRY(fk.join());
    else AVMOE_TRY(fused_down(st));
  } else {
    AVMOE_TRY(down_gemm(Xs.flat(d.S), Z.flat(d.S)));                        // Zx = X Wt^T
  }
  // ---- router (its input: the token means of X -- after the statistics above) ----------------------
  AVMOE_TRY(k_router(pl, sv, sc, prm, route, st));        // (and the selection stage behind it, when the call has one)
  if (d.KL > 0 && !d.fuse_l2) {                            // L2[s] = X[s] T[s]^T   (fused: per-group partial sums came out of the down projection; pre_small adds them into L2)
    GemmArgs g = base();
    AVMOE_TRY(g.product(vw::L2(pl, sv), Xs, Text.rows_at(0, d.KL).T()));
    g.nb1 = d.S;
    AVMOE_TRY(launch_gemm(g, st));
  }
  // ---- AVVP unimodal N x N block (mgn.py:132-139): xr = softmax_rows(X X^T)^T X, shared by the unimodal experts;
  //      their input x + gate_av * xr enters the LN-folded projection through ZR = xr Wt^T and three row sums ----
  if (d.mha) {                                             // AVS "v1": one xr = MHA_e(X) - X per unimodal expert, through that expert's Wt rows
    for (int e = 0; e < d.E; ++e) {
      if (!d.nxn_of_e[e]) continue;
      const int slot = d.xr_of_e[e];
      AVMOE_TRY(mha_frames_forward(pl, X, prm.e[e], slot, sv, sc, st));
      AVMOE_TRY(k_xrstats(pl, X, sv, slot, st));
      GemmArgs g = base();                                 // ZR[:, expert e] = xr Wt_e^T
      AVMOE_TRY(g.product(vw::ZR(pl, sv).flat(d.S).groups(d.g).cols_at(e * d.dgp, d.dgp), vw::xr(pl, sv, slot).flat(d.S).groups(d.g),
                          Wt.rows_at(e * d.dgp, d.dgp).T()));
      g.nb2 = d.g;
      AVMOE_TRY(launch_gemm(g, st));
    }
  } else if (d.nxn) {
    for (int s0 = 0; s0 < d.S; s0 += d.nxc) {              // d.nxc frames at a time through one workspace (all of them when they fit: moe_plan.cpp)
      const int ns = std::min(d.nxc, d.S - s0);
      const Mat Xm = Xs.frames_at(s0), xrm = vw::xr(pl, sv, 0).frames_at(s0), att = vw::att(pl, sv);
      const void* Xc = Xm.p;
      // att[s] = softmax_rows(X[s] X[s]^T) without the scores leaving the chip: the product runs twice with softmax epilogues -- (max, sum exp)
      // per row and column tile, then exp(score - lse) straight to att; the row log-sum-exp is kept for the backward
      float* lse = (float*)(sv + pl.o_nlse) + (size_t)s0 * d.N;
      if (d.nflash) {     // the large-N sites: row statistics, then xr = att^T X with att re-formed in the accumulators (nxn_att.hip)
        AVMOE_TRY(k_nxn_att(Xc, ns, d.N, d.C, (int)att.ld, lse, nullptr, 0, st));
        AVMOE_TRY(k_nxn_xr(Xc, ns, d.N, d.C, (int)att.ld, lse, (void*)xrm.p, st));
        continue;
      }
      if (nxn_att_ok(d.bf16, d.N, d.C, (int)att.ld)) {                 // ... as one kernel for the large-N sites (nxn_att.hip)
        AVMOE_TRY(k_nxn_att(Xc, ns, d.N, d.C, (int)att.ld, lse, (void*)att.p, 0, st));
      } else
      for (int pass = 0; pass < 2; ++pass) {
        GemmArgs g = base(dt);
        AVMOE_TRY(g.product(att, Xm, Xm.T()));
        g.nb1 = ns;
        if (pass == 0) { g.epi = GEMM_EPI_ROWSTATS; g.row_part = (float*)(sc + pl.o_npart); }
        else { g.epi = GEMM_EPI_EXP; g.row_lse = lse; }
        AVMOE_TRY(launch_gemm(g, st));
        if (pass == 0) AVMOE_TRY(gemm_row_lse((const float*)(sc + pl.o_npart), (long)ns * d.N, cdiv(d.N, 128), lse, st));
      }
      {                                                    // xr[s] = att[s]^T X[s]
        GemmArgs g = base(dt);
        AVMOE_TRY(g.product(xrm, att.T(), Xm));
        g.nb1 = ns;
        g.ksplit = choose_ksplit(g, slab_cap);             // few frames x few column tiles: split the token contraction to fill the chip
        AVMOE_TRY(launch_gemm(g, st));
      }
    }
    AVMOE_TRY(k_xrstats(pl, X, sv, 0, st));
    AVMOE_TRY(down_gemm(vw::xr(pl, sv, 0).flat(d.S), vw::ZR(pl, sv).flat(d.S)));
  }
  // ---- bottleneck space --------------------------------------------------------------------------
  PassCall pass(pl, sv, sc, prm);                          // (pass.h: each pass tries its forms in order)
  AVMOE_TRY(k_pre_small(pass, st));
  AVMOE_TRY(k_bn1_finalize(pl, sv, sc, prm, st));
  if (!d.gram64) AVMOE_TRY(k_mid(pass, st));
  if (d.use_bn && d.training && d.gram64) {
    // No MID pass and no stored z' on this path: ONE streaming pass over z forms z' = act(BN1(z)) on the way into LDS and leaves
    // both BatchNorm-2 moments -- Szz[i][e] = z'^T z' / NT and the column means mz (every later kernel recomputes z' from z anyway)
    AVMOE_TRY(k_gram64(pl, sv + pl.o_Z, nullptr, 1.f / (float)d.NT, (float*)(sc + pl.o_gpartT), (float*)(sv + pl.o_Szz), st,
                       (const float*)(sv + pl.o_bn1), (float*)(sc + pl.o_gcolT), (float*)(sv + pl.o_mz)));
  } else if (d.use_bn && d.training) {                     // ... as 8 batched token contractions of the engine
    GemmArgs g = base();
    const Mat Zp = vw::Zp(pl, sc).flat(d.S).groups(d.g * d.E);      // Szz[i][e] = z'^T z' / NT
    AVMOE_TRY(g.product(vw::Szz(pl, sv).row_blocks(d.dgp, d.dgp), Zp.T(), Zp));
    g.nb2 = d.g * d.E;
    g.alpha = 1.f / (float)d.NT;
    g.ksplit = choose_ksplit(g, slab_cap);
    AVMOE_TRY(launch_gemm(g, st));
  }
  AVMOE_TRY(k_post_prep(pl, sv, sc, prm, st));
  AVMOE_TRY(k_post_small(pass, st));
  {                                                        // out = Apost Bpost^T  (mixture, gates, BN2, LN-post folded in)
    GemmArgs g = base(dt);
    AVMOE_TRY(g.product(vw::tokens_x(d, out).flat(d.S).groups(d.g), vw::Apost(pl, sv).groups(d.g).cols_at(0, d.KP),
                        vw::Bpost(pl, sv).row_blocks(d.Cg, d.Cg).cols_at(0, d.KP).T()));
    g.nb2 = d.g;
    g.accumulate = d.acc_out;
    AVMOE_TRY(launch_gemm(g, st));
  }
  if (cumul) AVMOE_TRY(k_bn_count(pl, prm_in, st));          // behind k_bn1_finalize / k_post_prep, which only read the counters in this mode
  return OK;
}

// ---- sub-ops of the C ABI (for tests / partial adoption; the product path never calls them) -------------------------
// What ExpertAdapter.forward of expert e returns -- gate * LN_post(BN2(up(act(BN1(down(LN_before(x'))))))), net_trans_v3.py:377-435 --
// as the site forward with the router pushed to an exact one-hot on that expert: a logit offset of 3e4 makes softmax return 1.0 for it
// and 0.0 for the others (exp underflows to zero), so out = 1 * out_e + 0 * out_others.  Same kernels and workspaces as
// avmoe_moe_forward.  A NON-FINITE value in another expert's output still propagates (0 * Inf = NaN), exactly as it does in the
// reference's own mixture (net_trans_v3.py:485-486) -- compare modules on finite parameters.
int expert_forward(const Plan& pl, const void* X, const void* Y, const avmoe_moe_ptrs& prm, int e, void* out, char* sv, char* sc, hipStream_t st) {
  const Dims& d = pl.d;
  if (e < 0 || e >= d.E) { set_last_error("expert_forward: expert %d of %d", e, d.E); return ERR_BAD_ARG; }
  float* noise = (float*)(sc + pl.o_dp);                   // (S, E) floats of a backward-only buffer
  AVMOE_TRY(k_onehot_noise(noise, d.S, d.E, e, 3.0e4f, st));
  // Training mode: only the SELECTED expert's BatchNorm running statistics and counters advance (what ExpertAdapter.forward of that
  // one module does).  The other experts still run -- their outputs enter the mixture with weight exactly 0 -- but their
  // running_mean / running_var / num_batches_tracked updates go to a write-only dump in a backward-only scratch buffer (training
  // mode never READS running statistics), so comparing a site module by module does not advance every module E times.
  avmoe_moe_ptrs q = prm;
  if (d.training && d.use_bn) {
    float* dump = (float*)(sc + pl.o_dWf);               // C x Cy floats >= max(C, d) ; 256-byte aligned
    // (cumulative average, bn_momentum < 0: the kernels READ a counter per expert -- the others get a zeroed one in another backward-only buffer)
    int64_t* dump_n = nullptr;
    if (d.bn_momentum < 0.f) {
      dump_n = (int64_t*)(sc + pl.o_dsm);
      if (hipMemsetAsync(dump_n, 0, sizeof(int64_t), st) != hipSuccess) { set_last_error("expert_forward: memset of the dump counter failed"); return ERR_LAUNCH; }
    }
    for (int o = 0; o < d.E; ++o) {
      if (o == e) continue;
      q.e[o].bn1_rm = q.e[o].bn1_rv = q.e[o].bn2_rm = q.e[o].bn2_rv = dump;
      q.e[o].bn1_nbt = q.e[o].bn2_nbt = dump_n;
    }
  }
  RouteCall route; route.noise = noise;                    // the dense mixture on the one-hot softmax, nothing reported
  return moe_forward(pl, X, Y, q, out, route, sv, sc, st);
}

// The remap MATERIALISED (the product path folds it away): Yt = conv_adapter(Y) (S, N, Cy), then
// Yf = fc(Yt) (S, N, C) -- `vis_token` of net_trans_v3.py:469-471, token-major.  Two engine GEMMs on the T-typed weight copies of
// k_prep_all + the two biases.
int remap_forward(const Plan& pl, const void* Y, const avmoe_moe_ptrs& prm, void* Yt, void* Yf, char* sv, char* sc, hipStream_t st) {
  const Dims& d = pl.d;
  if (!prm.fc_b) { set_last_error("remap_forward: fc.bias missing"); return ERR_BAD_ARG; }
  const int dt = d.bf16 ? GEMM_BF16 : GEMM_F32;
  const Mat Yts = views::view(Yt, 0, d.esz, d.N, d.Cy, d.Cy, (long)d.N * d.Cy);      // the remapped Y: (S, N, Cy)
  // k_prep_all also prepares the experts' operands, by the plan's group layout: a merged-groups site (Dims::mg) must hand it the dense
  // block-diagonal copies, as moe_forward does -- with the grouped down_sampler it would read g times the tensor's length
  avmoe_moe_ptrs p = prm;
  if (d.mg) {
    AVMOE_TRY(k_merge_expand(pl, sv, prm, st));
    p = merged_params(pl, prm, sv);
  }
  AVMOE_TRY(k_prep_all(pl, sv, p, st));
  {                                                        // Yt[s] = Wc Y[s]
    GemmArgs g; g.dtype = dt; g.out_dtype = dt; g.slabs = (float*)(sc + pl.o_slabs);
    AVMOE_TRY(g.product(Yts, views::WcK(pl, sv).cols_at(0, d.M), views::tokens_y(d, Y)));
    g.nb1 = d.S;
    AVMOE_TRY(launch_gemm(g, st));
  }
  AVMOE_TRY(k_add_bias(d.bf16, Yt, (long)d.S * d.N, d.Cy, d.N, prm.conv_b, nullptr, st));
  {                                                        // Yf = Yt Wf^T
    GemmArgs g; g.dtype = dt; g.out_dtype = dt; g.slabs = (float*)(sc + pl.o_slabs);
    AVMOE_TRY(g.product(views::tokens_x(d, Yf).flat(d.S), Yts.flat(d.S), views::WfT(pl, sv).T()));
    AVMOE_TRY(launch_gemm(g, st));
  }
  return k_add_bias(d.bf16, Yf, (long)d.S * d.N, d.C, 1, nullptr, prm.fc_b, st);
}

}  // namespace avmoe
