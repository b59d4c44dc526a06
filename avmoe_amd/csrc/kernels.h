// Launch wrappers of the bottleneck-space kernels (everything that is not a GEMM).
// Naming follows oracle/algebra_ref.py; buffer layouts are documented in moe_plan.h.
#pragma once
#include "moe_plan.h"
#include <hip/hip_runtime.h>
#include <variant>

namespace avmoe {

struct P16 { const float* p[MAX_E]; };
struct W16 { float* p[MAX_E]; };
struct N16 { int64_t* p[MAX_E]; };       // num_batches_tracked counters (avmoe_expert_ptrs::bn1_nbt / bn2_nbt), NULL = none

// All wrappers return 0 or a negative status; `bf16` selects the operand type T.
// ---- forward: weight preparation -------------------------------------------------------------
// remap operands, folded expert weights, stacked latent tokens, the constant rows of Text: one launch
int k_prep_all(const Plan& pl, char* saved, const avmoe_moe_ptrs& prm, hipStream_t st);
// merged groups (Dims::mg): block-diagonal dense copies of the grouped down_sampler / up_sampler weights, and the way back for
// their gradients (only the diagonal blocks are parameters)
int k_merge_expand(const Plan& pl, char* saved, const avmoe_moe_ptrs& prm, hipStream_t st);
int k_merge_gather(const Plan& pl, char* scratch, const avmoe_moe_ptrs& grads, hipStream_t st);
avmoe_moe_ptrs merged_params(const Plan& pl, const avmoe_moe_ptrs& prm, char* saved);
avmoe_moe_ptrs merged_grads(const Plan& pl, const avmoe_moe_ptrs& grads, char* scratch);
// ---- forward: token statistics ---------------------------------------------------------------
int k_rowstats(int bf16, const void* X, long rows, int C, float* out_sum_sq /* [2][rows] */, hipStream_t st);
int k_xstats(const Plan& pl, const void* X, char* saved, char* scratch, hipStream_t st);   // row sums + column means of X
int k_sum_parts(const float* parts, int nparts, long n, float* out, hipStream_t st);       // out[i] = sum_p parts[p * n + i]
// ... and, in the same launch, rin[s][c] = scale * sum over the `tiles` column partials xpart[s][tile][c] (fused X statistics)
int k_xstats_fin(const float* parts, int nparts, long n, float* out, const float* xpart, int tiles, int C, int S, float* rin, long rin_ld,
                 float scale, hipStream_t st);
int k_colmean(int bf16, const void* X, int S, int N, int C, float* out, long out_ld, hipStream_t st);
// ---- forward: hop 1 ---------------------------------------------------------------------------
// qr / qb (after Q = T0 Wf) into qrqb and the extension columns of Rext ; the ybar rows of Rext / BmX
int k_qrqb_fill(const Plan& pl, char* saved, const float* fc_b, hipStream_t st);
int k_softmax_rows(int bf16_out, const float* in, long rows, int n, int ld_in, void* out, int ld_out, int grp, int valid,
                   int slot, int kvalid, hipStream_t st);
int k_finish_T(const Plan& pl, char* saved, char* scratch, const avmoe_moe_ptrs& prm, int src /*0 y, 1 x*/,
               hipStream_t st);
// ---- forward: router --------------------------------------------------------------------------
// The words of `saved + o_mode` (moe_plan.h: 64 ints).  Block 0 of every router forward writes the first six, the selection stage behind it
// the words per expert; the router backward reads them -- it takes the forward's selection from here, never from live tensors.
constexpr int MODE_K = 0, MODE_RENORM = 1;                  // the k of the mixture weights in `probs` (0: dense, `psm` unused; E: dense behind a multiplier or a stage), their renorm
constexpr int MODE_SELECT = 2;                              // what the experts were ranked on: 0 = p, or
constexpr int MODE_SELECT_BIASED = 1, MODE_SELECT_SINKHORN = 2;   // p + b (avmoe_moe_forward_bias) ; p v (avmoe_moe_forward_sinkhorn) -- the bits of b / v in MODE_SELECT_WORDS
constexpr int MODE_SELECT_TOP_P = 3;                        // p, the smallest ranked prefix reaching P (avmoe_moe_forward_top_p): MODE_K = k_max, the bits of P in MODE_SELECT_WORDS, k_min in the word behind it
constexpr int MODE_CHOICE_C = 3, MODE_CHOICE_RENORM = 4;    // expert choice: the capacity (0: off), its renorm
constexpr int MODE_SK_ITERS = 5;                            // Sinkhorn: the rounds (0: off)
constexpr int MODE_SELECT_WORDS = 16;                       // [16, 16 + E): the bits of the selection bias, or of the Sinkhorn column scale, the forward used; top-p: [16] = the bits of P, [17] = k_min
constexpr int MODE_CHOICE_THR = 32, MODE_CHOICE_LAST = 48;  // [32, 32 + E) / [48, 48 + E): expert choice, the bits of the thresholds T_e / the last frames taken L_e

struct RouterChoice { int capacity, renorm; int32_t* choice; };     // avmoe_moe_forward_choice: c in [1, S], renorm, (S) bitmask out or NULL
struct RouterSinkhorn { int iters; int32_t* choice; int32_t* count; };   // avmoe_moe_forward_sinkhorn: n in [1, 64], (S) bitmask out or NULL, (E) counts out or NULL
struct RouterCapacity { int capacity, policy; float* cap_scale; int32_t* kept; int32_t* demand; int32_t* kept_count; };   // avmoe_moe_forward_capacity: c in [1, S], 0 "order" / 1 "priority", (S, E) multiplier out, (S) bitmask / (E) / (E) counts out or NULL
struct RouterTopP { float p; int k_min, k_max; int32_t *choice, *count, *khist; };   // avmoe_moe_forward_top_p: P in (0, 1], 1 <= k_min <= k_max <= E, (S) bitmask / (E) frames per expert / (E + 1) frames per number of experts out or NULL
// How one call routes: every field's default means "off", a call site names what it sets.  route_check (capi.cpp) holds the ranges.
struct RouteCall {
  const float* noise = nullptr;           // (S, E) added to the router's logits
  int top_k = 0;                          // > 0 (< E): top-k gating of the mixture (avmoe_moe_forward_topk); 0 = the dense mixture
  int renorm = 1;                         // the kept weights renormalised (k = 0: it only lands in the mode word of `saved`, unread -- a dense site records 1)
  float* probs_out = nullptr; int64_t* idx_out = nullptr; float* lb_out = nullptr;      // (S, E) the dense softmax, (S) its argmax, the load-balancing loss (0 for a site without it)
  float *aux_out = nullptr, *load_out = nullptr;      // [z, balance], the router auxiliary losses (avmoe_moe_forward_aux), (E) the share of the routing slots per expert (read with aux_out only)
  const float* mix_scale = nullptr;       // (S, E) multiplier on the mixture weights behind top-k (avmoe_moe_forward_reg / _backward_reg: stochastic depth, expert dropout)
  const float* select_bias = nullptr; float* select_count = nullptr;      // (E) bias on the top-k selection alone, (E) selection counts added to (avmoe_moe_forward_bias: aux-loss-free balancing)
  // The stage behind the router, a variant (two at once cannot be written down) -- none; expert choice: each expert takes its `capacity` frames (top_k 0,
  // no selection bias); Sinkhorn-balanced top-k: the experts are ranked on p v, v from `iters` rounds on the call's softmax (top_k in [1, E), no selection bias);
  // expert capacity: every expert keeps at most `capacity` of the frames that selected it (top_k in [1, E); the router runs as without it, the dropped weights are zeroed);
  // top-p: each frame takes the fewest ranked experts whose mass reaches p, between k_min and k_max of them (top_k 0, no selection bias; renorm is the call's)
  std::variant<std::monostate, RouterChoice, RouterSinkhorn, RouterCapacity, RouterTopP> stage;
};
int k_onehot_noise(float* noise, int S, int E, int hot, float value, hipStream_t st);      // sub-ops of the C ABI (fwd_kernels.hip)
int k_add_bias(bool bf16, void* Z, long rows, int cols, int period, const float* rowb, const float* colb, hipStream_t st);
// the router, then the call's selection stage (k_expert_choice ; k_sk_scale, k_sk_apply ; k_cap_mask, k_cap_select, k_cap_apply ; k_top_p_apply, k_top_p_count) on the same stream
int k_router(const Plan& pl, char* saved, char* scratch, const avmoe_moe_ptrs& prm, const RouteCall& r, hipStream_t st);
// expert-choice gating (expert_choice.hip): per column e of p (S, E) the threshold T_e = its c-th largest value and L_e = the last frame taken
// among the ties (one block per expert), then per frame the mask, the weights w (times mix) and the bitmask word.  thr_bits / last: E words
// each, written by the first launch and read by the second; w / choice: NULL = not written.  Two launches, no host scalar that changes.
int k_expert_choice(const float* p, long S, int E, int capacity, int renorm, const float* mix, float* w, int32_t* choice, int* thr_bits,
                    int* last, hipStream_t st);
// Sinkhorn-balanced top-k (router_sinkhorn.hip): k_sk_scale, ONE block, runs the `iters` rounds of row / column normalisation on p (S, E),
// leaves the bits of the column scale v in v_bits (E words) and clears count (E words, or NULL); k_sk_apply, one thread per frame, ranks
// on p v and writes the weights w (times mix), the bitmask word and the counts of the selection (added into count).  w / choice / count:
// NULL = not written.  No host scalar that changes.
int k_sk_scale(const float* p, long S, int E, int iters, int* v_bits, int* count, hipStream_t st);
int k_sk_apply(const float* p, long S, int E, int top_k, int renorm, const float* mix, const int* v_bits, float* w, int32_t* choice,
               int* count, hipStream_t st);
// Expert capacity for top-k routing (router_capacity.hip), behind a k_router call in the top-k form: k_cap_mask, one thread per frame, leaves
// the selection word of every frame (topk_select / topk_select_biased on p); k_cap_select, one block per expert, the two words per expert
// (policy 0 "order": the c-th selecting frame; policy 1 "priority": the c-th largest p among the selecting frames and the last tied frame
// taken), demand and kept_count (E words each, or NULL); k_cap_apply, one thread per frame, sets the dropped entries of w to +0.0f and writes
// cap_scale (S, E) = keep ? mix (or 1) : 0 and the bitmask of the kept pairs (w / cap_scale / kept: NULL = not written; kept may be mask).
int k_cap_mask(const float* p, long S, int E, int top_k, const float* bias, int32_t* mask, hipStream_t st);
int k_cap_select(const float* p, const int32_t* mask, long S, int E, int capacity, int policy, int* thr_bits, int* last, int32_t* demand,
                 int32_t* kept_count, hipStream_t st);
int k_cap_apply(const float* p, const int32_t* mask, long S, int E, int policy, const int* thr_bits, const int* last, const float* mix,
                float* w, float* cap_scale, int32_t* kept, hipStream_t st);
// Top-p routing (router_top_p.hip): k_top_p_apply, one thread per frame, runs topp_select on p (S, E) and writes the weights w (times mix),
// the bitmask word and -- mode not NULL -- the mode words of the router backward (MODE_K = k_max, MODE_RENORM, MODE_SELECT = MODE_SELECT_TOP_P,
// the bits of P and k_min in MODE_SELECT_WORDS); k_top_p_count, ONE block, overwrites count (E) and khist (E + 1) with integer sums in a fixed
// order, from the bitmask words when `choice` holds them, else from its own topp_select on p.  w / choice / count / khist: NULL = not written.
// No host scalar that changes, no clear.
int k_top_p_apply(const float* p, long S, int E, float top_p, int k_min, int k_max, int renorm, const float* mix, float* w, int32_t* choice,
                  int* mode, hipStream_t st);
int k_top_p_count(const float* p, const int32_t* choice, long S, int E, float top_p, int k_min, int k_max, int32_t* count, int32_t* khist,
                  hipStream_t st);
int top_p_check(const char* fn, int E, float top_p, int k_min, int k_max);      // the ranges of both entry points: 0, or AVMOE_ERR_BAD_ARG with the message set
// ---- forward: per token -----------------------------------------------------------------------
struct PassCall;       // pass.h: the description of a bottleneck-space pass call, the forms of every pass and their protocol
int k_pre_small(PassCall& c, hipStream_t st);
int k_bn1_finalize(const Plan& pl, char* saved, char* scratch, const avmoe_moe_ptrs& prm, hipStream_t st);
int k_bn_count(const Plan& pl, const avmoe_moe_ptrs& prm, hipStream_t st);      // cumulative average only: +1 on every BatchNorm counter of the site
int k_mid(PassCall& c, hipStream_t st);
int k_post_prep(const Plan& pl, char* saved, char* scratch, const avmoe_moe_ptrs& prm, hipStream_t st);
int k_post_small(PassCall& c, hipStream_t st);

// ---- backward ---------------------------------------------------------------------------------
int k_post_small_bwd(PassCall& c, const avmoe_moe_ptrs& grads, hipStream_t st);       // (each backward pass + its finalize)
int k_post_prep_bwd(const Plan& pl, char* saved, char* scratch, const avmoe_moe_ptrs& prm,
                    const avmoe_moe_ptrs& grads, hipStream_t st);
int k_mid_bwd(PassCall& c, const avmoe_moe_ptrs& grads, hipStream_t st);
int k_pre_small_bwd(PassCall& c, const avmoe_moe_ptrs& grads, hipStream_t st);
int k_post_small_bwd_finalize(const Plan& pl, char* saved, char* scratch, const avmoe_moe_ptrs& prm,
                              const avmoe_moe_ptrs& grads, hipStream_t st);
int k_mid_bwd_finalize(const Plan& pl, char* saved, char* scratch, const avmoe_moe_ptrs& prm, const avmoe_moe_ptrs& grads,
                       hipStream_t st);
int k_pre_small_bwd_finalize(const Plan& pl, char* saved, char* scratch, const avmoe_moe_ptrs& prm,
                             const avmoe_moe_ptrs& grads, hipStream_t st);
int k_router_bwd(const Plan& pl, char* saved, char* scratch, const avmoe_moe_ptrs& prm, const avmoe_moe_ptrs& grads,
                 const float* lb_grad, const float* dprobs, hipStream_t st, const float* aux_grad, const float* mix_scale);
int k_softmax_rows_bwd(int bf16, const void* a, const float* da, long rows, int n, int ld, void* out_dl, void* out_t, int grp,
                       int ldT, hipStream_t st);
int k_finish_dT(const Plan& pl, char* saved, char* scratch, hipStream_t st);
int k_prep_dBm(const Plan& pl, char* scratch, hipStream_t st);
int k_dqrqb(const Plan& pl, char* scratch, const float* conv_b, hipStream_t st);
int k_hop1_finalize(const Plan& pl, char* saved, char* scratch, const avmoe_moe_ptrs& prm, const avmoe_moe_ptrs& grads,
                    hipStream_t st);
int k_down_bwd(const Plan& pl, char* scratch, const avmoe_moe_ptrs& prm, const avmoe_moe_ptrs& grads, hipStream_t st);

int k_xrstats(const Plan& pl, const void* X, char* saved, int slot, hipStream_t st);
int k_nxn_axpy(const Plan& pl, const void* X, char* saved, char* scratch, void* dX, int slot, int replaces, hipStream_t st);
// att = softmax_rows(X X^T) of `frames` frames in one kernel (nxn_att.hip); have_lse: the row log-sum-exp is given (only the exp sweep runs)
bool nxn_att_ok(int bf16, int N, int C, int Np);
int k_nxn_att(const void* X, int frames, int N, int C, int Np, float* lse, void* att, int have_lse, hipStream_t st);
int k_nxn_att_bwd(const void* X, const void* dxr, int frames, int N, int C, int Np, const float* rowdot, const void* att, void* dS, hipStream_t st);
// the same backward without the softmax in memory (nxn_att.hip, round 4): att re-formed from the kept row log-sum-exp in the accumulators
int k_nxn_y(const void* X, const void* dxr, int frames, int N, int C, int Np, const float* lse, float* rowdot, void* dX, hipStream_t st);   // rowdot = X . (att dxr) ; dX += att dxr
int k_nxn_xr(const void* X, int frames, int N, int C, int Np, const float* lse, void* xr, hipStream_t st);      // forward: xr = att^T X (lse from k_nxn_att with att == nullptr)
int k_nxn_dx(int key, const void* X, const void* dxr, int frames, int N, int C, int Np, const float* lse, const float* rowdot, void* dX, hipStream_t st);   // dX += dS X (key = 0) / dS^T X (key = 1), dS in the accumulators
int k_nxn_rowdot(int bf16, const void* X, const float* y, long rows, int C, void* dX, float* rowdot, hipStream_t st);   // dX += y ; rowdot = sum_c X y
// the shapes the register-resident kernel families serve (tile_fast.hip, tile_gen.inc); their forms are declared in pass.h
bool tile_fast_ok(const Dims& d);
bool tile_fast_shape(const Dims& d);      // the shape alone (the Gram-fused mode of gram.hip serves it on either kernel family)
bool tile_gen_ok(const Dims& d);
// streaming Gram of z' for the register-resident shape in bf16 (gram.hip): out[g*E][dgp][dgp] = scale * sum_t w[e][t] z' z'^T
int k_gram64(const Plan& pl, const void* Zp, const float* w, float scale, float* part, float* out, hipStream_t st, const float* bn1 = nullptr,
             float* colpart = nullptr, float* mz = nullptr);   // bn1: the input is z, z' = act(BN1(z)) on the fly; mz: column means of z' as well
// generic helpers
int k_colsum_f32(const float* in, long R, int ncol, long row_stride, int nslot, long slot_in, float* out, long slot_out,
                 float scale, hipStream_t st);
// two independent column sums (one slot each) in one launch when they are of the same row-count class; bit-identical to two launches
int k_colsum2_f32(const float* in0, long R0, int ncol0, long rs0, float* out0, float scale0,
                  const float* in1, long R1, int ncol1, long rs1, float* out1, float scale1, hipStream_t st);
int k_reduce_colpart(const Plan& pl, char* scratch, int slot0, int nslots, hipStream_t st);   // colpart -> colsum
int k_fill_f32(float* p, long n, float v, hipStream_t st);
int k_cast(int bf16_out, const float* src, long rows, int cols, long ld_src, void* dst, long ld_dst, hipStream_t st);

}  // namespace avmoe
