// The bottleneck-space passes of a site call (pre_small, mid, post_small and their backward passes) under the form protocol of forms.h.
// A call site describes the pass once (PassCall); each k_* wrapper lists the forms that may run it, in order: the streamed form
// (kfs_*, tile_stream.hip), the register-resident one (kf_*, tile_fast.hip), the generalised one (kg_*, tile_gen.inc) and the any-shape
// one (kt_* / kk_mid, tile_kernels.hip / fwd_kernels.hip), which serves every site and so ends every chain.  A form takes (PassCall&,
// stream) and answers 0 = launched, 1 = not served (nothing was launched), < 0 = error; whether it serves is its own business.  A new
// pass form starts here: declare it below, list it in its wrapper's chain.
#pragma once
#include "forms.h"
#include "kernels.h"

namespace avmoe {

// The per-expert tables every family hands to its kernels, from the plan and the parameter pointers the pass receives (unit gates and
// merged-group copies already applied: moe_forward / moe_backward).  Every family copies what its argument struct has.
struct PassExperts {
  P16 gate, glat;                                  // output gate ; gate_av / gate_self (hop-2 block, x + g xr input)
  int relu_of_e[MAX_E], lat_of_e[MAX_E], nxn_of_e[MAX_E];
  long sxr_off[MAX_E];                             // offset of the expert's xr slot in sxr / dsr ([slot][3][token])
  int first_of_slot[MAX_E];                        // the first expert of its xr slot (AVVP: all share slot 0; "v1": a slot each)
  int e_of_lat[MAX_E];
};
// Entries beyond d.E: make_plan zeroes Dims, so relu_of_e / nxn_of_e / lat_of_e are 0 there (lat_of_e is -1 only for the unimodal experts
// below d.E) -- what the copies that guarded with e < d.E and those that did not both handed over.  No kernel reads them.
inline PassExperts pass_experts(const Dims& d, const avmoe_moe_ptrs& prm) {
  PassExperts x = {};
  bool seen[MAX_E] = {};
  for (int e = 0; e < MAX_E; ++e) {
    x.gate.p[e] = prm.e[e].gate; x.glat.p[e] = prm.e[e].gate_lat;
    x.relu_of_e[e] = d.relu_of_e[e]; x.lat_of_e[e] = d.lat_of_e[e];
    if (e < d.E && d.nxn_of_e[e]) {
      const int slot = d.xr_of_e[e];
      x.nxn_of_e[e] = 1; x.sxr_off[e] = (long)slot * 3 * d.NT;
      x.first_of_slot[e] = !seen[slot]; seen[slot] = true;
    }
    if (e < d.E && d.lat_of_e[e] >= 0) x.e_of_lat[d.lat_of_e[e]] = e;
  }
  return x;
}
template <class V, int N> inline void put(V (&dst)[N], const V (&src)[N]) { for (int i = 0; i < N; ++i) dst[i] = src[i]; }

enum PassForm { PASS_NONE = 0, PASS_STREAM, PASS_FAST, PASS_GEN, PASS_TILE };

// One pass call.  A site call makes one and hands it to its passes in turn.
struct PassCall {
  const Plan& pl; char* saved; char* scratch; const avmoe_moe_ptrs& prm;
  PassExperts x;
  int dap16 = 0;             // post_small_bwd: dApost = [T columns | fp32 dApx] (moe_backward.cpp)
  PassForm ran = PASS_NONE;  // out: the form that launched sets it (the wrapper clears it); PASS_STREAM names the profiler scope
                             // "... (stream)" and tells moe_backward.cpp that post_small_bwd left dGq itself
  PassCall(const Plan& pl_, char* sv, char* sc, const avmoe_moe_ptrs& prm_) : pl(pl_), saved(sv), scratch(sc), prm(prm_), x(pass_experts(pl_.d, prm_)) {}
  bool streamed() const { return ran == PASS_STREAM; }
};
// what a form returns after its launch: rc, with the out-field set when the launch went out
inline int launched(PassCall& c, PassForm f, int rc) { if (rc == OK) c.ran = f; return rc; }

// ---- the forms -----------------------------------------------------------------------------------------------------------------
// tile_stream.hip: the tuned shape in bf16 from 2048 tokens on (one persistent block per CU, wave-private LDS rings filled by direct loads)
int kfs_pre_small(PassCall& c, hipStream_t st);
int kfs_post_small(PassCall& c, hipStream_t st);
int kfs_post_small_bwd(PassCall& c, hipStream_t st);      // split dApost with the Gram products: leaves dGq as well
int kfs_mid_bwd(PassCall& c, hipStream_t st);
int kfs_pre_bwd(PassCall& c, hipStream_t st);             // pre_small_bwd + pre_lat_bwd in one pass
// tile_fast.hip: register-resident, bottleneck 64 in 2 groups / 32 latent tokens / 2 - 4 experts (tile_fast_ok)
int kf_pre_small(PassCall& c, hipStream_t st);
int kf_mid(PassCall& c, hipStream_t st);
int kf_post_small(PassCall& c, hipStream_t st);
int kf_post_small_bwd(PassCall& c, hipStream_t st);
int kf_mid_bwd(PassCall& c, hipStream_t st);
int kf_pre_small_bwd(PassCall& c, hipStream_t st);
int kf_pre_lat_bwd(PassCall& c, hipStream_t st);          // the hop-2 block of the cross-modal experts, after kf_pre_small_bwd
// tile_gen.inc: register-resident, generalised over groups (1 / 2 / 4), per-group bottleneck (16 .. 96) and latent slots (Dims::gen)
int kg_pre_small(PassCall& c, hipStream_t st);
int kg_mid(PassCall& c, hipStream_t st);
int kg_post_small(PassCall& c, hipStream_t st);
int kg_post_small_bwd(PassCall& c, hipStream_t st);
int kg_mid_bwd(PassCall& c, hipStream_t st);
int kg_pre_small_bwd(PassCall& c, hipStream_t st);        // both kernels
// (the any-shape forms kt_* / kk_mid are local to their wrappers' files)

// ---- algorithmic bytes of the passes ---------------------------------------------------------------------------------------------
// Every element a pass has to read or write, once (zsz / esz: element sizes of the Z-space and T-typed tensors): the numerators of
// their HBM rooflines and what the profiler scopes report.
inline double lat_bytes(const Dims& d, int planes) { return d.KL ? (double)d.KL * (4 + planes * d.esz) : 0.0; }      // logits + a (aw, ag, dL2) per token
inline double bytes_pre_small(const Dims& d) { return (double)d.NT * (2.0 * d.DZ * d.zsz + lat_bytes(d, 1) + 8.0 + 8.0 * d.E); }
inline double bytes_mid(const Dims& d) { return (double)d.NT * d.DZ * (double)(d.zsz + d.esz); }
inline double bytes_post_small(const Dims& d) { return (double)d.NT * ((double)d.DZ * d.zsz + (double)d.g * d.KPp * d.esz + 8.0 * d.E); }
inline double bytes_post_small_bwd(const Dims& d, int dap16) {
  const double zspace = d.gram64 ? (double)d.DZ * (d.esz + d.zsz) + 4.0 * d.E       // read the saved z', write dz' and dSoo
                                 : (double)d.DZ * (2.0 * d.zsz + 2.0 * d.esz);      // read Z, write dz', z', dSoo z'
  const double split = dap16 ? (double)d.NT * d.g * (d.E * d.dgp * 2.0 + (d.KPp - 16) * 4.0 - d.E * d.dgp * 2.0) : 0.0;
  return (double)d.NT * (zspace + (double)d.g * d.KPp * 4.0 + 8.0 * d.E) - split;
}
inline double bytes_mid_bwd(const Dims& d) { return (double)d.NT * (3.0 * d.DZ * d.zsz); }
inline double bytes_pre_small_bwd(const Dims& d) {
  return (double)d.NT * ((double)d.DZ * (2.0 * d.zsz + d.esz) + lat_bytes(d, 4) + 8.0 * d.E + 12.0);
}
// ... of its forms that the profiler shows under scopes of their own: the streamed pass, and the two kernels of tile_fast.hip
inline double bytes_pre_bwd_stream(const Dims& d) {
  return (double)d.NT * ((double)d.DZ * (2.0 * d.zsz + d.esz) + 8.0 * d.E + 4.0 + (d.KL ? lat_bytes(d, 4) + d.KLp * d.esz - d.KL * d.esz : 0.0));
}
inline double bytes_pre_small_bwd_fast(const Dims& d) { return (double)d.NT * ((double)d.DZ * (2.0 * d.zsz + d.esz) + 8.0 * d.E + 8.0 * d.El + 12.0); }
inline double bytes_pre_lat_bwd_fast(const Dims& d) { return (double)d.NT * ((double)d.El * d.DD * d.esz + lat_bytes(d, 4) + 8.0 * d.El); }

}  // namespace avmoe
