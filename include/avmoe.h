/* avmoe.h -- C ABI of the MI355X-native AVMoE adapter hot path (libavmoe_hip.so).
 *
 * The reference (yingchengy/AVMOE) has no FFI: its boundary for this path is the Python nn.Module API
 * of MoEAdapter / ExpertAdapter (AVMOE/AVE/nets/net_trans_v3.py:296-487 and the four task copies).
 * This header is what a binding for that path binds instead: plain pointers, sizes, strides and a
 * hipStream_t (passed as void*), int status returns, no exceptions, no torch types.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless said otherwise; the library never allocates or frees
 *     caller memory; scratch comes from a caller-provided workspace
 *   - all entry points are asynchronous on `stream`, re-entrant across streams, and keep no global
 *     mutable state besides a thread-local error string, the optional profiler (avmoe_prof_*) and the
 *     test hooks (avmoe_test_hooks); the environment is read ONCE per process, never per call
 *   - return 0 on success, negative on error (avmoe_last_error() has the message)
 */
#ifndef AVMOE_H_
#define AVMOE_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AVMOE_ABI_VERSION 11

enum { AVMOE_OK = 0, AVMOE_ERR_BAD_ARG = -1, AVMOE_ERR_UNSUPPORTED = -2, AVMOE_ERR_ALIGNMENT = -3,
       AVMOE_ERR_WORKSPACE = -4, AVMOE_ERR_LAUNCH = -5 };
enum { AVMOE_F32 = 0, AVMOE_BF16 = 1 };
enum { AVMOE_K_MAJOR = 0, AVMOE_MN_MAJOR = 1 };

int avmoe_abi_version(void);
int avmoe_bn_cumulative_supported(void); /* 1: avmoe_moe_desc::bn_momentum < 0 selects the cumulative average (a library without the symbol takes it as a number) */
const char* avmoe_last_error(void);      /* thread-local, valid until the next failing call */

/* ---- sub-op: the strided / batched MFMA GEMM every wide contraction of the path runs on --------
 * C[b][i][j] (+)= alpha * sum_k A[b][i][k] * B[b][j][k]  (+ row_scale[b][i] * D[b][i][j])
 * Replaces the reference's conv2d(1x1) / linear / bmm calls (net_trans_v3.py:380-388,395,401,469-470).
 * Layout / alignment contract: avmoe_amd/csrc/gemm.h. */
typedef struct avmoe_gemm_desc {
  int32_t M, N, K;
  int32_t nb1, nb2;                 /* batch = nb1 * nb2 */
  int32_t dtype, out_dtype;         /* AVMOE_F32 | AVMOE_BF16 */
  int32_t a_layout, b_layout;       /* AVMOE_K_MAJOR | AVMOE_MN_MAJOR */
  int32_t accumulate, ksplit, tile;
  int32_t fp32_planes;              /* ABI 9, fp32 operands: 0 = products on v_mfma_f32_16x16x4_f32, 1 = on the bf16 matrix pipe with every value as three
                                       bf16 planes (six plane products of order <= 2: 5.8e-9 relative per product, fp32 accumulation) -- what most of the
                                       site calls use; 2 (ABI 11) = two planes, the three plane products of order <= 1: 1.5e-5 relative per product at half the
                                       matrix-pipe work (the site backward uses it for its leaf products: csrc/moe_run.h, AVMOE_LEAF2); avmoe_amd/csrc/gemm.h::GemmArgs::split3 */
  float alpha;
  int64_t lda, ldb, sA1, sA2, sB1, sB2;
  int64_t sCi, sCj, sC1, sC2;
  int64_t sRS1, sRS2, sDi, sD1, sD2;
} avmoe_gemm_desc;

size_t avmoe_gemm_workspace_bytes(const avmoe_gemm_desc* desc);
int avmoe_gemm(const avmoe_gemm_desc* desc, const void* A, const void* B, void* C,
               const float* row_scale, const void* D, void* workspace, void* stream);


/* ---- the adapter site: MoEAdapter.forward / backward -------------------------------------------
 * Replaces  MoEAdapter.forward(x, vis_token[, is_training])  (AVE net_trans_v3.py:468-487,
 * AVQA net_avst_v2.py:381-399, AVVP mgn.py:185-217, AVS PVT_AVSModel_v2.py:283-312) and its autograd.
 *
 * Tensors are TOKEN-MAJOR and contiguous: X (S, N, C), Y (S, M, Cy), out / dOut / dX (S, N, C),
 * dY (S, M, Cy), element type desc.dtype (AVMOE_F32 | AVMOE_BF16).  [The reference hands the module
 * (S, C, N, 1) permuted VIEWS of exactly this memory -- net_trans_v3.py:695.]
 * Parameters / buffers / their gradients are fp32, one pointer per reference state_dict entry.      */
#define AVMOE_MAX_EXPERTS 16
enum { AVMOE_VARIANT_AVE = 0, AVMOE_VARIANT_AVVP = 1, AVMOE_VARIANT_AVS = 2 };   /* AVQA == AVE math */
enum { AVMOE_SELF_ATTN_NONE = 0, AVMOE_SELF_ATTN_LATENT_V2 = 1, AVMOE_SELF_ATTN_NXN = 2,
       AVMOE_SELF_ATTN_MHA_V1 = 3 };   /* AVS self_attention_version "v1": nn.MultiheadAttention(C, 4) across the FRAMES (ABI 3) */

typedef struct avmoe_moe_desc {
  int32_t S, N, C;          /* this modality: frames, tokens, channels  (C = input_dim = linear_out) */
  int32_t M, Cy;            /* other modality: tokens (conv_dim_in), channels (linear_in)            */
  int32_t E_m, E_s;         /* opt.num_multimodal_experts, opt.num_singlemodal_experts               */
  int32_t d, groups, K;     /* bottleneck = C // reduction_factor, opt.num_conv_group, num_tk         */
  int32_t use_bn, use_gate, ln_before, ln_post;
  int32_t variant, self_attn, lb_loss;
  int32_t dtype;            /* activations */
  int32_t training;         /* 1: BatchNorm batch statistics + running-stat update ; 0: running stats */
  float bn_eps, ln_eps, bn_momentum;
  /* bn_momentum >= 0: torch's fixed momentum, r <- (1 - m) r + m x.
   * bn_momentum < 0 (the facade passes -1.0f; added under ABI 11, AVMOE_ABI_VERSION unchanged: avmoe_bn_cumulative_supported): torch's
   * momentum=None, the CUMULATIVE average.  In a training-mode forward with BatchNorm, with n the value of a BatchNorm's own
   * num_batches_tracked BEFORE this call, every element of its running mean / variance becomes (1 - f) r + f x with
   * f = 1.0f / (float)(n + 1) and x the batch mean / the unbiased batch variance, and the counter becomes n + 1; bn1 and bn2 of an
   * expert each use their own counter (avmoe_expert_ptrs::bn1_nbt / bn2_nbt).  f is formed on the device -- no host read of the
   * counter, the forward stays capturable.  The statistic kernels only READ the counters in this mode; one small launch behind them,
   * on the same stream, adds 1 to every counter of the site, so f never depends on which thread got to a counter first.  Such a call
   * with use_bn && training and an expert's bn1_nbt or bn2_nbt NULL is refused (AVMOE_ERR_BAD_ARG, avmoe_last_error names the
   * counter) before anything is launched.  Eval mode and use_bn == 0 ignore the field. */
  /* backward only: add dX / dY to what the output buffers already hold instead of overwriting them -- lets a caller whose
   * token tensor feeds several sites (the audio tokens are X of the audio site and Y of the visual site,
   * net_trans_v3.py:695-698) collect the gradient in one buffer without a separate accumulation pass (ABI 2) */
  int32_t accumulate_dx, accumulate_dy;
  /* forward only (ABI 3): out += adapter(X, Y) instead of out = ... -- the caller's residual stream (x + attention(x), then
   * "+ adapter residual", net_trans_v3.py:706-709) takes the adapter's contribution inside the output GEMM's epilogue */
  int32_t accumulate_out;
  /* ABI 8: 1 = kernels of OTHER streams may be on the GPU while this call runs (a caller that overlaps two sites on two streams:
   * AdapterPair's two-stream mode; a backbone GEMM on another stream).  0 = the call is alone on the GPU (its own helper stream
   * never runs beside the kernels below).
   * Why: on MI355X / ROCm 7.2 a workgroup that shares a COMPUTE UNIT with a workgroup of another kernel that keeps the matrix pipe busy
   * (v_mfma_f32_32x32x16_bf16 chains, a GEMM tile's 16 independent v_mfma_f32_16x16x32_bf16 chains) occasionally gets wrong results in
   * its own upper lanes: v_mfma_f32_16x16x4_f32 sums (lanes 48 - 51) and per-block column sums.  scripts/mfma_probe.hip shows it with two
   * stand-alone kernels; every mode and mitigation of it, run on an MI355X, is kept in profiles/r05_mfma_probe.txt (+ _part2): 0
   * mismatches alone or beside LDS-only / sparse-MFMA aggressors, 10^5 - 10^6 per run beside a dense-MFMA aggressor whatever the
   * victim's LDS read width (ds_read_b128 or two ds_read_b64) and whatever wait states follow its MFMAs, and 0 again once the
   * victim's blocks take a whole CU's LDS each (no other block fits beside them; requests with which 2 or 4 of them fill a CU do not
   * suffice: a block can land beside foreign blocks that are already there).
   * Round 6 (profiles/r06_mfma_probe.txt): the same victim with its mat-vecs in the split-bf16 form of the tuned kernels (two bf16 planes,
   * v_mfma_f32_16x16x32_bf16) is corrupted just the same beside an aggressor that issues v_mfma_f32_32x32x16_bf16 (7 x 10^7 mismatches in 200
   * repetitions; 4 x 10^5 .. 1.5 x 10^6 beside sixteen independent chains of 16x16x32; 0 alone, 0 beside an aggressor of its own instruction
   * shape) -- no form of these kernels is immune by construction, only placement protects them.
   * What the flag does: every bottleneck-space kernel that uses the matrix pipe keeps other kernels' blocks off its compute units --
   *   - the generalised family (csrc/tile_gen.inc) and the any-shape fallback (csrc/tile_kernels.hip) launch with 150 KB of dynamic LDS, one
   *     block per CU; the backward does not fork its dBpost product beside them;
   *   - the tuned instance at LARGE bf16 sites (csrc/tile_stream.hip: pre_small, post_small, post_small_bwd, mid_bwd -- one persistent block
   *     per CU by design) asks for the whole 160 KB;
   *   - the tuned instance elsewhere (csrc/tile_fast.hip: every small site; pre_small_bwd / pre_lat_bwd of large sites) asks for 150 KB per
   *     block where the grid has at most one block per CU (nothing is lost) and for 80 KB where it is larger (two blocks fill a CU; a foreign
   *     block can only land beside the first or the last block of a CU); the streaming Gram kernel (csrc/gram.hip) asks for 80 KB likewise.
   * The streaming GEMM kernels and the tiled engine are not touched: their products have not moved in any two-stream repetition (they issue
   * long independent chains; what goes wrong in the probe is a short dependent chain whose result the VALU consumes at once).
   * bench.py reports `roofline.two_stream_bit_equal` (three steps on two streams against the same schedule on one stream, every gradient bit for
   * bit) on every default run; tests/test_two_stream_repeat_gpu.py is the longer guard.
   * Cost: residency of those kernels where the grid exceeds the chip (BASELINE config 4: 80 -> 90 ms per step).  The flag changes their
   * block shape, i.e. the summation order of the per-block BatchNorm column sums: results agree to fp32 rounding of those sums, and
   * repeat bit for bit for a given flag.
   * The Python wrappers set it in AdapterPair's two-stream mode and, by default (warned once), for every call issued on a stream other than
   * the device's default stream (avmoe_amd.adapters.set_shared_gpu). */
  int32_t shared_gpu;
} avmoe_moe_desc;

typedef struct avmoe_expert_ptrs {        /* <list>.{j}.*  ; unused entries NULL                     */
  float *gate, *my_tokens, *gate_lat;     /* gate ; my_tokens ; gate_av | gate_self                   */
  float *down_w, *up_w;                   /* down_sampler.weight (d, C/g) ; up_sampler.weight (C, d/g)*/
  float *bn1_w, *bn1_b, *bn2_w, *bn2_b;
  float *lnb_w, *lnb_b, *lnp_w, *lnp_b;   /* ln_before.* ; ln_post.*                                  */
  float *bn1_rm, *bn1_rv, *bn2_rm, *bn2_rv; /* running_mean / running_var (updated in place in training) */
  /* ABI 3 -- AVS unimodal expert with self_attention_version "v1" (PVT_AVSModel_v2.py:141-142,210-214):
   * self_attention.{in_proj_weight (3C, C), in_proj_bias (3C), out_proj.weight (C, C), out_proj.bias (C)} and, in `params`
   * only, sa_keep: the dropout multiplier of the attention weights, (N * 4, S, S) f32 holding 0 or 1 / (1 - p), or NULL for
   * no dropout (eval).  The caller draws it (the reference uses the global RNG) and keeps it alive until the backward.  */
  float *sa_in_w, *sa_in_b, *sa_out_w, *sa_out_b, *sa_keep;
  /* ABI 6 -- bn1.num_batches_tracked / bn2.num_batches_tracked (one int64 each), or NULL: a training-mode forward with BatchNorm
   * adds 1 to each inside its own kernels (torch.nn.BatchNorm2d semantics), so the caller needs no extra launch for the counters.
   * With avmoe_moe_desc::bn_momentum < 0 they are required: the update factor is 1 / (counter + 1). */
  int64_t *bn1_nbt, *bn2_nbt;
} avmoe_expert_ptrs;

typedef struct avmoe_moe_ptrs {
  float *conv_w, *conv_b, *fc_w, *fc_b;   /* conv_adapter.{weight (N, M), bias} ; fc.{weight (C, Cy), bias} */
  float *r0_w, *r0_b, *r2_w, *r2_b, *r4_w, *r4_b;   /* router.{0,2,4}.*                               */
  avmoe_expert_ptrs e[AVMOE_MAX_EXPERTS]; /* multimodal experts first, then singlemodal               */
} avmoe_moe_ptrs;

size_t avmoe_moe_saved_bytes(const avmoe_moe_desc* desc);     /* 0 + error string on a bad descriptor */
size_t avmoe_moe_scratch_bytes(const avmoe_moe_desc* desc);

/* out (S,N,C) ; probs (S,E) f32 ; idx (S) int64 = first-max argmax of probs ; lb: 1 float (0 if !lb_loss).
 * noise: optional (S,E) f32 already scaled by 0.01 (AVS logit noise), or NULL.                       */
int avmoe_moe_forward(const avmoe_moe_desc* desc, const void* X, const void* Y, const avmoe_moe_ptrs* params,
                      const float* noise, void* out, float* probs, int64_t* idx, float* lb,
                      void* saved, void* scratch, void* stream);

/* avmoe_moe_forward_topk (added under ABI 11; AVMOE_ABI_VERSION unchanged, a binding finds it by symbol) -- top-k gating of the
 * mixture (Shazeer et al. 2017, Switch, Mixtral; BASELINE config 3 "router top-k=2"; the reference mixes densely,
 * net_trans_v3.py:482-486).  With p = softmax(router logits) of frame s and S_k(s) its k most probable experts (higher probability
 * first, equal probabilities in expert order: the order of avmoe_router_topk), m_e = 1[e in S_k(s)]:
 *     renorm != 0:  w_e = m_e p_e / sum_j m_j p_j      (= a softmax over the kept logits)
 *     renorm == 0:  w_e = m_e p_e                      (Switch style)
 *     out = sum_e w_e expert_e(x)
 * Only the mixture weights change: every expert still runs on every frame (no speed-up), so BatchNorm batch statistics and
 * running-statistic updates are those of the dense site.  probs stays the dense softmax (bit-equal to avmoe_moe_forward), idx its
 * first-max argmax, lb the load-balancing loss on the dense softmax.  top_k must be in [1, E] (AVMOE_ERR_BAD_ARG otherwise); top_k == E
 * is avmoe_moe_forward, whatever renorm says.
 * The backward entry points (avmoe_moe_backward, _part, _ex with its router-only path; avmoe_moe_backward_dx_dy has no router term)
 * read the mode from `saved`, where every forward writes it, and keep their signatures.  They give the gradients of <out, dOut> + <probs, dprobs> + (*lb_grad) * lb: the mixture's
 * gradient dw of the weights is mapped to the softmax --  renorm: dp_e = m_e (dw_e - sum_j w_j dw_j) / sum_j m_j p_j ; otherwise
 * dp_e = m_e dw_e --, dprobs and the load-balancing term are added, then the softmax Jacobian.  The selection has no gradient.  With
 * k = 1 and renorm, w is one-hot and the mixture sends no gradient to the router (only dprobs and lb do): renorm = 0 is the setting that
 * trains the router through the mixture at k = 1.
 * The sub-ops avmoe_router_forward and avmoe_expert_forward_* stay dense.                                                              */
int avmoe_moe_forward_topk(const avmoe_moe_desc* desc, const void* X, const void* Y, const avmoe_moe_ptrs* params,
                           const float* noise, int32_t top_k, int32_t renorm, void* out, float* probs, int64_t* idx, float* lb,
                           void* saved, void* scratch, void* stream);

/* Gradients of  <out, dOut> + (*lb_grad) * lb .  Every pointer in `grads` that is non-NULL is OVERWRITTEN
 * with the gradient of the matching parameter; dX / dY are overwritten.  `saved` must be the buffer the
 * matching forward filled.  lb_grad: DEVICE pointer to the upstream gradient of the load-balancing loss
 * (one float; read on the stream, so no host sync), or NULL for 0.                                    */
int avmoe_moe_backward(const avmoe_moe_desc* desc, const void* X, const void* Y, const avmoe_moe_ptrs* params,
                       const void* dOut, const float* lb_grad, void* saved, void* scratch,
                       void* dX, void* dY, const avmoe_moe_ptrs* grads, void* stream);

/* ABI 4 -- the same backward in stream-ordered sections.  `parts` is a bit mask: 1 = the GEMMs against dOut and the bottleneck /
 * weight space (touches neither dX nor dY), 2 = the GEMMs against X (every writer of dX), 4 = the chain back to Y and the remap
 * parameters (every writer of dY); 0 or 7 = all of it (== avmoe_moe_backward).  ABI 5: section 4 in two steps -- 8 = the chain
 * without the GEMM(s) that write dY (touches neither dX nor dY), 16 = those GEMMs alone.  Sections must be run in this order with the
 * same arguments; between calls the caller may record / wait events on the stream but must leave `saved` and `scratch` alone.
 * Purpose: a token tensor that feeds two sites (the audio tokens are X of the audio site and Y of the visual site,
 * net_trans_v3.py:695-698) collects both gradients in ONE buffer while the two sites run on two streams -- the smaller site
 * runs through and overwrites (its dY / dX), an event orders the larger site's sections 2 and 4 behind it, and that site adds
 * its dX / dY in the GEMM epilogues (accumulate_dx / accumulate_dy); or, cross-wise: each site overwrites its own tokens' gradient
 * (sections 1, 2, 8), then adds its dY to the other tensor (16) once the other site's section 2 is done.
 * Not available (AVMOE_ERR_UNSUPPORTED) for sites with latent self attention (AVS v2), whose last section writes dX too.
 * ABI 10: section 2 in two steps (plain sites: no N x N / frame / latent self attention) -- 32 = the GEMMs against X without the dX
 * product (touches neither dX nor dY), 64 = the dX product alone (after 1; independent of 32 and 8).                              */
int avmoe_moe_backward_part(const avmoe_moe_desc* desc, const void* X, const void* Y, const avmoe_moe_ptrs* params,
                            const void* dOut, const float* lb_grad, void* saved, void* scratch,
                            void* dX, void* dY, const avmoe_moe_ptrs* grads, int32_t parts, void* stream);

/* avmoe_moe_backward_ex (added under ABI 11; AVMOE_ABI_VERSION unchanged, a binding finds it by symbol) -- the backward with two more
 * upstream gradients: the gradients of  <out, dOut> + <probs, dprobs> + (*lb_grad) * lb.  The reference returns the gating probabilities
 * as an ordinary autograd tensor (PVT_AVSModel_v2.py:298,312), so a loss built on them (router entropy, a balance term,
 * distillation of the routing; NOT the router z-loss, which needs the logits: avmoe_moe_forward_aux) reaches the router, the remap parameters, X and Y.
 *   dprobs: DEVICE pointer to (S, E) f32, or NULL for 0 (then the launched kernels and every result bit are those of
 *           avmoe_moe_backward_part with the same `parts`).  The term enters the router backward in section 1.
 *   dOut:   NULL = out gets no gradient.  Then only the router and the mean / remap chain carry gradient and no expert, Gram or
 *           token-space product runs: the router backward, one pass over Y that also writes dY, one broadcast write of dX and small
 *           reductions (csrc/router_only_bwd.hip); every expert parameter gradient is written as 0.  Only parts 0 / 7 are served
 *           (AVMOE_ERR_UNSUPPORTED otherwise).  accumulate_dx / accumulate_dy are honoured.
 *   parts, lb_grad and everything else: as avmoe_moe_backward_part.  avmoe_moe_backward(_part) == _ex with dprobs = NULL.         */
int avmoe_moe_backward_ex(const avmoe_moe_desc* desc, const void* X, const void* Y, const avmoe_moe_ptrs* params,
                          const void* dOut /* NULL: out gets no gradient */, const float* dprobs /* (S,E) f32 or NULL */,
                          const float* lb_grad, void* saved, void* scratch, void* dX, void* dY,
                          const avmoe_moe_ptrs* grads, int32_t parts, void* stream);

/* avmoe_moe_forward_aux / avmoe_moe_backward_aux (added under ABI 11; AVMOE_ABI_VERSION unchanged, a binding finds them by symbol) --
 * the router auxiliary losses that go with top-k routing (an extension: ST-MoE's router z-loss, Switch's balance loss).  With l the
 * router logits of a site call (the AVS noise included), p = softmax(l), S frames, E experts:
 *     lse_s   = logsumexp_e l_se                          z = (1 / S) sum_s lse_s^2
 *     k'      = top_k when 0 < top_k < E, else 1
 *     S_k'(s) = the k' most probable experts of frame s (higher probability first, equal probabilities in expert order: the rule of
 *               avmoe_router_topk and of the top-k mixture), taken on the dense softmax
 *     load_e  = (1 / (S k')) sum_s 1[e in S_k'(s)]        (sums to 1)          P_e = (1 / S) sum_s p_se
 *     balance = E sum_e load_e P_e                        (1 at a uniform router)
 * avmoe_moe_forward_aux is avmoe_moe_forward (top_k == 0 or E) / avmoe_moe_forward_topk (0 < top_k < E) with two more outputs:
 *   aux:  DEVICE pointer to 2 floats [z, balance], or NULL: then exactly those entry points, launch for launch.
 *   load: DEVICE pointer to E floats, or NULL (ignored when aux is NULL).
 * out, probs, idx and lb have the bits of the call without aux.  The losses come out of one small one-block launch after the router
 * (fixed summation order: the results repeat bit for bit); on a site with lb_loss that launch forms lb too, in place of its own.
 * avmoe_moe_backward_aux is avmoe_moe_backward_ex with one more upstream gradient:
 *   aux_grad: DEVICE pointer to 2 floats [g_z, g_balance], or NULL (then avmoe_moe_backward_ex, bit for bit).  It must follow a
 *             forward that had aux != NULL (`saved` carries lse and load).  The gradients are those of
 *             <out, dOut> + <probs, dprobs> + (*lb_grad) * lb + g_z * z + g_balance * balance:
 *             d balance / d p_se = E load_e / S joins the gradient of p before the softmax Jacobian (the selection carries no gradient,
 *             as in the mixture), d z / d l_se = (2 / S) lse_s p_se is added to the gradient of the logits after it.  No launch is
 *             added.  dOut == NULL takes the router-only path as in avmoe_moe_backward_ex.
 * The library has one forward and one backward body (csrc/capi.cpp): since the mixture regularisers they are reached in full through
 * avmoe_moe_forward_reg / avmoe_moe_backward_reg below, which are these two plus mix_scale.  The Python facade (avmoe_amd.adapters) calls
 * the _aux entry points, with top_k = 0 for a dense site and NULL for every option that is off, and the _reg ones for a site call with a
 * multiplier.  avmoe_moe_forward, _forward_topk, _forward_aux, avmoe_moe_backward, _backward_part, _backward_ex and _backward_aux remain as
 * the same bodies with fewer arguments -- they differ only in what they refuse (_topk: top_k == 0; _backward, _part: dOut == NULL) and have no behaviour of
 * their own.                                                                                                                          */
int avmoe_moe_forward_aux(const avmoe_moe_desc* desc, const void* X, const void* Y, const avmoe_moe_ptrs* params,
                          const float* noise, int32_t top_k /* 0: dense */, int32_t renorm, void* out, float* probs, int64_t* idx,
                          float* lb, float* aux /* [z, balance] or NULL */, float* load /* (E) or NULL */, void* saved, void* scratch,
                          void* stream);
int avmoe_moe_backward_aux(const avmoe_moe_desc* desc, const void* X, const void* Y, const avmoe_moe_ptrs* params,
                           const void* dOut, const float* dprobs, const float* lb_grad, const float* aux_grad /* [g_z, g_balance] or NULL */,
                           void* saved, void* scratch, void* dX, void* dY, const avmoe_moe_ptrs* grads, int32_t parts, void* stream);

/* avmoe_moe_forward_reg / avmoe_moe_backward_reg (ABI 12 in the project's count of boundary revisions; like every addition since 11 they
 * are found by symbol and AVMOE_ABI_VERSION stays 11) -- the regularisers of the mixture: stochastic depth (drop_path) on the adapter
 * branch and expert dropout.  Both are one per-(frame, expert) multiplier on the mixture weights, applied behind top-k:
 *     out[s] = sum_e mix_scale[s, e] w[s, e] expert_e(x)[s]          w: the dense softmax, or the top-k weights
 *   mix_scale: DEVICE pointer to (S, E) f32, or NULL.  The site call consumes the tensor and does not draw (the convention of `noise` and
 *              sa_keep); avmoe_mix_drop_draw below fills it.  Any finite values are served.  NULL: avmoe_moe_forward_aux /
 *              avmoe_moe_backward_aux, launch for launch and instruction for instruction (one uniform branch on the pointer in two router
 *              kernels, not taken).  A tensor of ones gives the bits of NULL in every output.
 * Only the weights the experts' outputs are mixed with change.  Every expert still runs on every frame, and BatchNorm batch and running
 * statistics, probs, idx, lb, aux and load are those of the call without the multiplier, bit for bit.  A frame whose multipliers are all 0
 * gets out[s] = 0 exactly (with accumulation into a residual stream at the caller, nothing is added).  A dense site (top_k 0 or E) with
 * a multiplier is run as top-k with k = E without renormalisation -- w = p exactly -- so that `saved` keeps the softmax beside the
 * multiplied weights; the mode word of `saved` then reads [E, 0].
 * avmoe_moe_backward_reg takes the SAME tensor again (it is not kept in `saved`): the gradient of the mixture with respect to the weights
 * is multiplied by mix_scale before it joins what avmoe_moe_backward_aux does (the top-k map, dprobs, lb, the auxiliary losses, the
 * softmax Jacobian).  mix_scale itself has no gradient.  A frame whose multipliers are all 0 has dOut[s] multiplied by exactly 0 on its way
 * into the experts; the router-side terms are untouched.  Without train-mode BatchNorm such a frame's dX / dY are therefore the router's
 * term alone.  With it the frame's tokens still enter the batch statistics (the statistics stay dense), and the kept frames' gradients
 * reach them through those: that part of dX / dY is not zero, and it is the derivative.  dOut == NULL (the router-only path) forms no gradient of the weights and
 * does not read mix_scale.  A backward that follows a forward with a multiplier must be given it; every older backward entry point passes NULL. */
int avmoe_moe_forward_reg(const avmoe_moe_desc* desc, const void* X, const void* Y, const avmoe_moe_ptrs* params,
                          const float* noise, int32_t top_k /* 0: dense */, int32_t renorm, const float* mix_scale /* (S,E) f32 or NULL */,
                          void* out, float* probs, int64_t* idx, float* lb, float* aux /* [z, balance] or NULL */,
                          float* load /* (E) or NULL */, void* saved, void* scratch, void* stream);
int avmoe_moe_backward_reg(const avmoe_moe_desc* desc, const void* X, const void* Y, const avmoe_moe_ptrs* params,
                           const void* dOut, const float* dprobs, const float* lb_grad, const float* aux_grad,
                           const float* mix_scale /* the forward's, or NULL */, void* saved, void* scratch, void* dX, void* dY,
                           const avmoe_moe_ptrs* grads, int32_t parts, void* stream);

/* avmoe_mix_drop_draw (found by symbol, as above) -- draws mix_scale on the device, ONE launch (csrc/mix_drop.hip):
 *     mix_scale[s, e] = a[s] b[s, e]     a[s] = 0 with probability p, else 1 / (1 - p)     b[s, e] = 0 with probability q, else 1 / (1 - q)
 * (p: drop_path, per frame; q: expert dropout, per pair, independent, no renormalisation and no rescue of a frame that loses every
 * expert.)  state: DEVICE pointer to 16 bytes {uint64 seed, uint64 calls}, owned by the caller, 8-byte aligned.  Generator:
 * Philox-4x32-10, key = (seed low, seed high), counter = (calls low, calls high, s, e / 4), lane e % 4 serves expert e; the frame's draw
 * uses counter word 3 = 0xFFFFFFFF, lane 0.  A uniform is (x >> 8) * 2^-24; dropped when u < q / u < p.  Kept values are exactly
 * fl(fl(1 / (1 - p)) * fl(1 / (1 - q))) in fp32.  The kernel reads `calls` and stores calls + 1 itself: no host scalar changes between
 * two calls, so a captured launch draws a fresh multiplier on every replay.  Calls on one state block must be ordered (one stream, or events).
 * AVMOE_ERR_BAD_ARG, with nothing launched and nothing written: a NULL pointer, p or q outside [0, 1), S < 1, E outside [1, 16].       */
int avmoe_mix_drop_draw(void* state, int64_t S, int32_t E, float p, float q, float* mix_scale, void* stream);

/* avmoe_moe_forward_bias / avmoe_router_bias_update (found by symbol, as above; AVMOE_ABI_VERSION stays 11) -- aux-loss-free expert
 * balancing of the top-k gating (Wang et al. 2024, DeepSeek-V3): a per-expert bias b that enters the SELECTION only.  With p the dense
 * softmax of a frame and 0 < k < E:
 *     sc_e   = p_e + b_e                     ONE fp32 addition
 *     S_k(s) = the k experts with the highest score (higher score first, equal scores in expert order: the tie rule of the top-k mixture)
 *     kept   = sum of the kept p_e           unbiased, added in expert order
 *     w_e    = m_e p_e / kept (renorm) or m_e p_e ,  then times mix_scale          -- the weights never see b
 * avmoe_moe_forward_bias is avmoe_moe_forward_reg plus
 *   select_bias:  DEVICE pointer to E floats, or NULL.  Read by the call, never written.  It has no gradient.
 *   select_count: DEVICE pointer to E floats, or NULL.  ADDED to, not overwritten: select_count[e] += the number of frames of this call
 *                 that selected expert e (the actual, biased selection; without a bias the plain one; a dense site counts every frame's
 *                 first-max expert, as `load` does).  Integers kept in fp32, exact below 2^24; one thread of one block adds them in.
 * Both NULL: avmoe_moe_forward_reg, launch for launch and bit for bit.  With a bias, probs, idx, lb, the z-loss, the BatchNorm statistics
 * and every saved tensor but the weights are those of the call without it, bit for bit, and a bias of zeros gives the bits of NULL in
 * every output.  `load` (and the balance loss formed from it) is the share of the ACTUAL selection.  select_count with aux comes out of
 * the auxiliary-loss launch; without aux it costs one more one-block launch.
 * select_bias != NULL with top_k == 0 or top_k == E: AVMOE_ERR_BAD_ARG before anything is launched (a dense mixture has no selection).
 * `saved`: word [2] of the `mode` buffer (64 four-byte words; [0] = k, [1] = renorm) is 1 when the forward used a bias and 0 otherwise
 * -- every router forward writes it --, and words [16, 16 + E) hold the bits of the bias values it USED.  No buffer is added and
 * avmoe_moe_saved_bytes does not change.  There is no new backward entry point: every existing one recomputes the selection from the
 * saved softmax and THOSE words, so a bias updated between a forward and its backward does not change the backward's selection.
 *
 * avmoe_router_bias_update -- the update after an optimizer step, ONE launch for all sites of a model (csrc/router_bias.hip).  bias and
 * counts: DEVICE (n_sites, 16) f32, row i belongs to site i, E: DEVICE (n_sites) int32.  For every site i with E_i in [1, 16]:
 *     tot = sum_e counts[i][e]  (expert order) ;  tot == 0: the row is left alone ;  otherwise  d_e = tot - E_i counts[i][e]  and
 *     bias[i][e] += +rate (d_e > 0: below the mean count), -rate (d_e < 0), nothing (d_e == 0) ;  then counts[i][e] = 0.
 * The sign test is exact while tot and E_i counts[i][e] stay below 2^24 (1 048 576 routing slots per site between two updates at E = 16).
 * Columns e >= E_i are neither read nor written; a row whose E_i is outside [1, 16] is skipped.  No host scalar changes between two
 * calls: the launch is capturable.  AVMOE_ERR_BAD_ARG, with nothing launched: a NULL pointer, n_sites < 1, rate negative or not finite. */
int avmoe_moe_forward_bias(const avmoe_moe_desc* desc, const void* X, const void* Y, const avmoe_moe_ptrs* params,
                           const float* noise, int32_t top_k /* 0: dense */, int32_t renorm, const float* mix_scale /* (S,E) f32 or NULL */,
                           const float* select_bias /* (E) f32 or NULL */, float* select_count /* (E) f32, added to, or NULL */,
                           void* out, float* probs, int64_t* idx, float* lb, float* aux /* [z, balance] or NULL */,
                           float* load /* (E) or NULL */, void* saved, void* scratch, void* stream);
int avmoe_router_bias_update(float* bias /* DEVICE (n_sites, 16) */, float* counts /* DEVICE (n_sites, 16) */,
                             const int32_t* E /* DEVICE (n_sites) */, int32_t n_sites, float rate, void* stream);

/* avmoe_moe_forward_choice / avmoe_expert_choice (found by symbol, as above; AVMOE_ABI_VERSION stays 11) -- expert-choice gating (Zhou et
 * al. 2022; csrc/expert_choice.hip): each EXPERT takes the `capacity` frames on which the router scores it highest, so the load is balanced
 * by construction -- no loss weight, no update rate -- and a frame may be served by no, one or several experts.  With p the dense softmax
 * of the call, (S, E) fp32, AVS noise included, and capacity = c in [1, S]:
 *     C_e     = the c frames with the highest p[s, e]: higher probability first, equal probabilities in frame order (lower s first)
 *     m[s, e] = 1[s in C_e] ,   n_s = sum_e m[s, e] ,   kept_s = sum_e m[s, e] p[s, e]       added in expert order
 *     w[s, e] = m[s, e] p[s, e]                         renorm == 0
 *     w[s, e] = m[s, e] p[s, e] / kept_s                renorm != 0 ;  w[s, :] = 0 where n_s == 0
 *     w is then multiplied by mix_scale[s, e] if one is given, and out[s] = sum_e w[s, e] expert_e(x)[s]  (out[s] = 0 exactly where n_s == 0).
 * Only the weights change: every expert still runs on every frame, and the BatchNorm batch and running statistics, probs (the dense
 * softmax), idx (its first-max argmax), lb, aux and load are those of the dense call, bit for bit -- the auxiliary losses keep the dense
 * site's rule k' = 1 (the load of the actual selection is 1 / E by construction and carries no information).  The selection has no gradient.
 * The selection of expert e is fully described by two words: T_e, the c-th largest value of column e, and L_e, the largest frame index
 * taken among the frames equal to T_e;  m[s, e] = (p[s, e] > T_e) || (p[s, e] == T_e && s <= L_e)  exactly.
 * Backward, with g = dL/d(mix w) arriving as today and dw_e = mix_e g_e:  dp_e = m_e dw_e (renorm == 0) ;
 * dp_e = m_e (dw_e - sum_j (mix w)_j g_j) / kept_s (renorm != 0), dp = 0 where n_s == 0 ;  then dprobs, lb, the auxiliary terms and the
 * softmax Jacobian as ever.  It evaluates the mask per frame from the saved softmax and the words below and never runs the selection again.
 * There is no new backward entry point and no further backward launch: every existing one serves a choice forward (avmoe_moe_backward_reg
 * when a multiplier was used; dOut == NULL takes the router-only path; avmoe_moe_backward_dx_dy is untouched).
 * `saved`, `mode` buffer:  [3] = c (0: expert choice off -- every router forward writes it), [4] = renorm of the choice,
 * [32 + e] = the bits of T_e, [48 + e] = L_e.  A choice forward leaves [0] = E, [1] = 0, the "dense with a multiplier" form, so the saved
 * softmax is kept; [2] and [16, 32) are as without it.  No buffer is added and avmoe_moe_saved_bytes does not change.
 * Non-finite probabilities give an unspecified selection; every access stays in bounds and exactly c frames per expert are marked.
 *
 * avmoe_moe_forward_choice is avmoe_moe_forward_reg with top_k = 0, plus the choice: choice[s] (DEVICE (S) int32, or NULL) has bit e set
 * iff s in C_e.  There is no selection bias and no selection count in this mode.  It adds two launches to the forward (one block per
 * expert for T and L; one thread per frame for the weights and the bitmask); no host scalar changes between calls, so it is capturable.
 * capacity outside [1, S]: AVMOE_ERR_BAD_ARG with nothing launched.  capacity == S without renorm and without a multiplier gives
 * avmoe_moe_forward's bits in every output.
 *
 * avmoe_expert_choice -- the same kernels on a caller's DEVICE (S, E) fp32 matrix p.  w (S, E), choice (S), thr (E: T_e) and last (E: L_e)
 * may each be NULL; w must not overlap p.  With w or choice asked for but thr or last NULL, the call takes the 128 bytes for the missing
 * words from the stream's memory pool (hipMallocAsync / hipFreeAsync): it allocates, and capturing that form needs a runtime that captures
 * pool allocations -- pass thr and last to avoid it (the site call never allocates: its words live in `saved`).
 * AVMOE_ERR_BAD_ARG, with nothing launched: p NULL, S outside [1, 2^31 - 1] (L_e is an int32), E outside [1, 16], capacity outside [1, S]. */
int avmoe_moe_forward_choice(const avmoe_moe_desc* desc, const void* X, const void* Y, const avmoe_moe_ptrs* params,
                             const float* noise, int32_t capacity, int32_t renorm, const float* mix_scale /* (S,E) f32 or NULL */,
                             void* out, float* probs, int64_t* idx, float* lb, float* aux /* [z, balance] or NULL */,
                             float* load /* (E) or NULL */, int32_t* choice /* (S) or NULL */, void* saved, void* scratch, void* stream);
int avmoe_expert_choice(const float* p, int64_t S, int32_t E, int32_t capacity, int32_t renorm, const float* mix_scale /* (S,E) or NULL */,
                        float* w /* (S,E) or NULL */, int32_t* choice /* (S) or NULL */, float* thr /* (E) or NULL */,
                        int32_t* last /* (E) or NULL */, void* stream);

/* avmoe_moe_forward_sinkhorn / avmoe_router_sinkhorn (found by symbol, as above; AVMOE_ABI_VERSION stays 11) -- Sinkhorn-balanced top-k
 * routing (S-BASE, Clark et al. 2022; BASE layers, Lewis et al. 2021; csrc/router_sinkhorn.hip): the selection is balanced within the call,
 * and every frame is still served by exactly k experts.  No loss weight, no update rate, no persistent state.  With p the dense softmax of
 * the call, (S, E) fp32, AVS noise included, n = iters in [1, 64] and k = top_k in [1, E):
 *     v_e = 1 ;  n times:  u_s = 1 / sum_e p[s, e] v_e        (row step)
 *                          v_e = (S / E) / sum_s p[s, e] u_s   (column step)
 *     q[s, e] = p[s, e] * v_e                                  ONE fp32 multiplication: the selection repeats from p and v
 *     m[s, :] = the k experts with the largest q[s, :], equal q in expert order          (the tie rule of top-k gating, on q)
 *     kept_s  = sum_e m[s, e] p[s, e]                          the UNSCALED p, added in expert order
 *     w[s, e] = m[s, e] p[s, e] / kept_s  (renorm != 0)  |  m[s, e] p[s, e]  (renorm == 0) ;  then multiplied by mix_scale[s, e] if given.
 * u_s does not change a row's ranking, so the E words v describe the selection of the whole call; v enters the selection only, the weights
 * come from the unscaled p (as with a selection bias).  v has no gradient (a stop-gradient, as in S-BASE), and neither has the selection.
 * A column whose sum is 0 gets the largest finite fp32: v is never Inf or NaN.  Every sum of the iteration has one fixed order (one block:
 * frames per thread in frame order, shuffles within a wave, the waves in wave order), so the same input gives the same bits on every call.
 * Only the weights change: every expert still runs on every frame, and the BatchNorm batch and running statistics, probs (the dense
 * softmax), idx, lb, aux and load are those of avmoe_moe_forward_reg with the same top_k, renorm and mix_scale, bit for bit -- the losses
 * keep describing the router's own preference, not the balanced selection, which is reported through choice and count.
 * Backward:  dp_e is the top-k formula (at avmoe_moe_forward_topk / _reg) with m from the scaled selection; dprobs, lb, the auxiliary terms
 * and the softmax Jacobian follow unchanged.  The mask is recomputed per frame from the saved softmax and the words of v the forward USED.
 * There is no new backward entry point and no further backward launch: every existing one serves a Sinkhorn forward (avmoe_moe_backward_reg
 * when a multiplier was used; dOut == NULL takes the router-only path).
 * `saved`, `mode` buffer:  [0] = k, [1] = renorm, [2] = 2 ("ranked on p v"; 1 is the selection bias, 0 neither -- every router forward
 * writes it, so a later plain forward on the same workspace switches the mode off), [5] = n, [16 + e] = the bits of v_e.  No buffer is
 * added and avmoe_moe_saved_bytes does not change.
 * Non-finite probabilities give an unspecified selection; every access stays in bounds and exactly k experts are marked per frame.
 *
 * avmoe_moe_forward_sinkhorn is avmoe_moe_forward_reg plus iters and the two reports: choice[s] (DEVICE (S) int32, or NULL) has bit e set
 * iff frame s took expert e; count[e] (DEVICE (E) int32, or NULL; overwritten) is the number of frames that took expert e -- integer adds,
 * the same on every call.  There is no selection bias and no expert choice in this mode.  It adds two launches to the forward (one block
 * for v; one thread per frame for the weights, the bitmask and the counts); no host scalar changes between calls, so it is capturable.
 * top_k outside [1, E) or iters outside [1, 64]: AVMOE_ERR_BAD_ARG with nothing launched.
 *
 * avmoe_router_sinkhorn -- the same kernels on a caller's DEVICE (S, E) fp32 matrix p.  w (S, E), choice (S) and count (E) may each be NULL;
 * v (E) is required, so the call never allocates.  AVMOE_ERR_BAD_ARG, with nothing launched: p or v NULL, E outside [2, 16], S outside
 * [1, 2^31 - 1], top_k outside [1, E), iters outside [1, 64], w overlapping p. */
int avmoe_moe_forward_sinkhorn(const avmoe_moe_desc* desc, const void* X, const void* Y, const avmoe_moe_ptrs* params,
                               const float* noise, int32_t top_k, int32_t renorm, int32_t iters, const float* mix_scale /* (S,E) f32 or NULL */,
                               void* out, float* probs, int64_t* idx, float* lb, float* aux /* [z, balance] or NULL */,
                               float* load /* (E) or NULL */, int32_t* choice /* (S) int32 or NULL */, int32_t* count /* (E) int32 or NULL */,
                               void* saved, void* scratch, void* stream);
int avmoe_router_sinkhorn(const float* p, int64_t S, int32_t E, int32_t top_k, int32_t renorm, int32_t iters,
                          const float* mix_scale /* (S,E) or NULL */, float* w /* (S,E) or NULL */, int32_t* choice /* (S) or NULL */,
                          int32_t* count /* (E) or NULL */, float* v /* (E) */, void* stream);

/* avmoe_moe_forward_capacity / avmoe_router_capacity (found by symbol, as above; AVMOE_ABI_VERSION stays 11) -- an expert capacity behind
 * top-k routing (GShard, Lepikhin et al. 2020; Switch, Fedus et al. 2021; batch-prioritised routing: V-MoE, Riquelme et al. 2021;
 * csrc/router_capacity.hip): every expert serves at most c = capacity frames of the call, the token-expert pairs beyond that budget are
 * dropped, and a frame that lost every pair passes through the residual.  With p the dense softmax of the call, (S, E) fp32, AVS noise
 * included, k = top_k in [1, E), c in [1, S] and
 *     m[s, e]  = 1[e in S_k(s)]          the selection the top-k form makes: on p, or on p + select_bias when a bias is given
 *     demand_e = sum_s m[s, e]
 *   policy 0, "order" (GShard / Switch):  expert e keeps the first c frames, in frame order, that selected it;
 *   policy 1, "priority" (V-MoE):         expert e keeps the c selecting frames with the largest p[s, e] -- the unbiased, unscaled p; equal
 *                                         values in frame order.  For k = 1 this is V-MoE's rule; for k > 1 the priority is PER PAIR
 *                                         (a frame's second choice competes with its own p[s, e], not with the frame's best score).
 *   demand_e <= c: everything is kept.     keep[s, e] = m[s, e] and "kept by expert e";  kept_e = min(demand_e, c).
 *     w[s, e]         = keep[s, e] * w_topk[s, e] * mix_scale[s, e]
 *     cap_scale[s, e] = keep[s, e] ? (mix_scale ? mix_scale[s, e] : 1.0f) : 0.0f
 * w_topk is exactly what the top-k form writes: with renorm it is normalised over the FULL top-k set (as GShard normalises before it
 * drops), and nothing is renormalised after dropping.  A dropped pair's weight is exactly +0.0f: set, not multiplied.  A frame that lost
 * every pair has output 0 (with accumulate_out: nothing is added).  Each expert's outcome is two words as in expert choice, a threshold T_e
 * and a last frame L_e: keep = m && s <= L_e (policy 0; T_e = -Inf), keep = m && (p > T_e || (p == T_e && s <= L_e)) (policy 1);
 * within the budget T_e = -Inf, L_e = S - 1.
 * Only the weights change: every expert still runs on every frame, and probs (the dense softmax), idx, lb, aux, load, the saved softmax and
 * log-sum-exp, the mode words, the BatchNorm batch and running statistics and select_count are those of avmoe_moe_forward_bias with the same
 * arguments, bit for bit -- select_count means DEMAND, which is what a balancer should see.
 * Backward:  the keep mask is a {0, 1} factor on the mixture weights behind top-k, which is what mix_scale means: the backward of such a
 * forward is avmoe_moe_backward_reg with mix_scale = cap_scale, and the whole call equals avmoe_moe_forward_bias with mix_scale = cap_scale
 * bit for bit.  Nothing else is recorded: no new backward entry point, no backward launch, no mode word, no buffer;
 * avmoe_moe_saved_bytes and avmoe_moe_scratch_bytes do not change.
 * Non-finite probabilities give an unspecified selection; every access stays in bounds.
 *
 * avmoe_moe_forward_capacity is avmoe_moe_forward_bias plus capacity, policy, cap_scale (DEVICE (S, E) fp32, required) and three optional
 * reports: kept[s] (DEVICE (S) int32) has bit e set iff the pair (s, e) was kept, demand[e] and kept_count[e] (DEVICE (E) int32 each) are
 * demand_e and kept_e -- integer counts, the same bytes on every call.  It adds three launches to the forward behind the router (one thread
 * per frame for the selection words, one block per expert for its two words, one thread per frame for the weights); no host scalar changes
 * between calls, so it is capturable.  AVMOE_ERR_BAD_ARG with nothing launched: top_k outside [1, E), capacity outside [1, S], policy
 * outside {0, 1}, cap_scale NULL.
 *
 * avmoe_router_capacity -- the same kernels on a caller's DEVICE (S, E) fp32 matrix p.  w (S, E), or NULL, is in and out: it holds the top-k
 * weights (times the multiplier) and gets its dropped entries set to +0.0f.  cap_scale (S, E), kept (S), demand (E), kept_count (E),
 * thr (E, T_e) and last (E, L_e) may each be NULL.  The call takes S + 32 words from the stream's memory pool for the selection words.
 * AVMOE_ERR_BAD_ARG, with nothing launched: p NULL, E outside [2, 16], S outside [1, 2^31 - 1], top_k outside [1, E), capacity outside
 * [1, S], policy outside {0, 1}, w overlapping p. */
int avmoe_moe_forward_capacity(const avmoe_moe_desc* desc, const void* X, const void* Y, const avmoe_moe_ptrs* params,
                               const float* noise, int32_t top_k, int32_t renorm, const float* mix_scale /* (S,E) f32 or NULL */,
                               const float* select_bias /* (E) or NULL */, float* select_count /* (E) or NULL */, int32_t capacity,
                               int32_t policy, float* cap_scale /* (S,E) f32 */, int32_t* kept /* (S) int32 or NULL */,
                               int32_t* demand /* (E) int32 or NULL */, int32_t* kept_count /* (E) int32 or NULL */, void* out, float* probs,
                               int64_t* idx, float* lb, float* aux /* [z, balance] or NULL */, float* load /* (E) or NULL */, void* saved,
                               void* scratch, void* stream);
int avmoe_router_capacity(const float* p, int64_t S, int32_t E, int32_t top_k, const float* select_bias /* (E) or NULL */, int32_t capacity,
                          int32_t policy, const float* mix_scale /* (S,E) or NULL */, float* w /* (S,E) in/out or NULL */,
                          float* cap_scale /* (S,E) or NULL */, int32_t* kept /* (S) or NULL */, int32_t* demand /* (E) or NULL */,
                          int32_t* kept_count /* (E) or NULL */, float* thr /* (E) or NULL */, int32_t* last /* (E) or NULL */, void* stream);

/* avmoe_moe_forward_top_p / avmoe_router_top_p (found by symbol, as above; AVMOE_ABI_VERSION stays 11) -- top-p routing ("dynamic-k"
 * routing: Huang et al. 2024, "Harder tasks need more experts"; csrc/router_top_p.hip): the router decides how many experts a frame needs.
 * A frame whose softmax is peaked is served by one expert, an ambiguous one by as many as it takes to cover the probability mass P.  The
 * rule is per frame and independent of the batch: the same in eval mode and under data parallel.  No parameter, no loss weight, no state.
 * With p the dense softmax of the call, (S, E) fp32, AVS noise included, P = top_p fp32 in (0, 1], 1 <= k_min <= k_max <= E and
 * 2 <= E <= 16, per frame s:
 *     rank     the experts as top-k gating does: higher p first, equal p in expert order (on the order-preserving key of p: a total order
 *              on every bit pattern)
 *     c_0 = 0 ;  c_j = c_(j-1) + p_(j)  for j = 1 .. E         the running mass in rank order, ONE fp32 addition per step
 *     k*       = the smallest j with c_j >= P  (an fp32 comparison) ;  E when no j reaches P (P = 1 and an fp32 row sum that falls short)
 *     k_s      = min(max(k*, k_min), k_max)
 *     m[s, e]  = 1 iff rank(e) < k_s
 *     kept_s   = sum_e m[s, e] p[s, e]                          added in expert order: with k_min = k_max = k the bits of plain top-k
 *     w[s, e]  = m[s, e] p[s, e] / kept_s  (renorm != 0)  |  m[s, e] p[s, e]  (renorm == 0) ;  then multiplied by mix_scale[s, e] if given.
 * The selection carries no gradient.  Only the weights change: every expert still runs on every frame, and the BatchNorm batch and running
 * statistics, probs (the dense softmax), idx and lb are those of avmoe_moe_forward_reg on the same inputs, bit for bit.
 * Backward:  dp_e is the top-k formula (at avmoe_moe_forward_topk / _reg) with this mask; dprobs, lb, the auxiliary terms and the softmax
 * Jacobian follow unchanged.  The mask is recomputed per frame from the saved softmax and the words the forward left in `mode`.  There is
 * no new backward entry point and no further backward launch: every existing one serves a top-p forward (avmoe_moe_backward_reg when a
 * multiplier was used; dOut == NULL takes the router-only path).
 * Auxiliary losses (aux, load):  load_e = count_e / sum_e count_e, the share of the routing slots actually handed out, and
 * balance = E sum_e load_e P_e; z is unchanged, and the backward's balance term keeps using the saved load.
 * `saved`, `mode` buffer:  [0] = k_max, [1] = renorm, [2] = 3 ("smallest ranked prefix reaching P"; 2 is Sinkhorn, 1 the selection bias,
 * 0 neither -- every router forward writes it, so a later plain forward on the same workspace switches the mode off), [16] = the bits of
 * P, [17] = k_min; [3], [4], [5] as a plain forward writes them.  No buffer is added and avmoe_moe_saved_bytes does not change.
 * Non-finite probabilities give an unspecified selection; every access stays in bounds and between k_min and k_max experts are marked per
 * frame.
 *
 * avmoe_moe_forward_top_p is avmoe_moe_forward_reg with top_p, k_min, k_max in place of top_k, plus three reports, each DEVICE int32 or
 * NULL and each OVERWRITTEN with the same bits on every call: choice[s] (S) has bit e set iff frame s took expert e; count[e] (E) is the
 * number of frames that took expert e; khist[j] (E + 1) is the number of frames with k_s = j.  There is no selection bias, no Sinkhorn, no
 * capacity and no expert choice in this mode.  It adds one launch to the forward (one thread per frame: the weights, the bitmask, the mode
 * words) and, only when count or khist is asked for, a second one (one block: integer sums in a fixed order, nothing cleared); nothing is
 * allocated and no host scalar changes between calls, so it is capturable.  AVMOE_ERR_BAD_ARG with nothing launched: top_p not in (0, 1]
 * or NaN, k_min or k_max outside [1, E], k_min > k_max, E outside [2, 16].
 *
 * avmoe_router_top_p -- the same kernels on a caller's DEVICE (S, E) fp32 matrix p.  w (S, E), choice (S), count (E) and khist (E + 1) may
 * each be NULL.  AVMOE_ERR_BAD_ARG, with nothing launched: the refusals above, p NULL, S outside [1, 2^31 - 1], w overlapping p. */
int avmoe_moe_forward_top_p(const avmoe_moe_desc* desc, const void* X, const void* Y, const avmoe_moe_ptrs* params,
                            const float* noise, float top_p, int32_t k_min, int32_t k_max, int32_t renorm,
                            const float* mix_scale /* (S,E) f32 or NULL */, void* out, float* probs, int64_t* idx, float* lb,
                            float* aux /* [z, balance] or NULL */, float* load /* (E) or NULL */, int32_t* choice /* (S) int32 or NULL */,
                            int32_t* count /* (E) int32 or NULL */, int32_t* khist /* (E + 1) int32 or NULL */, void* saved, void* scratch,
                            void* stream);
int avmoe_router_top_p(const float* p, int64_t S, int32_t E, float top_p, int32_t k_min, int32_t k_max, int32_t renorm,
                       const float* mix_scale /* (S,E) or NULL */, float* w /* (S,E) or NULL */, int32_t* choice /* (S) or NULL */,
                       int32_t* count /* (E) or NULL */, int32_t* khist /* (E + 1) or NULL */, void* stream);

/* ABI 10 -- the gradient of a token tensor T that is X of site A and Y of site B (the two adapter sites of one backbone layer:
 * the audio tokens are X of the audio site and Y of the visual site, net_trans_v3.py:695-698), written ONCE:
 *     dT = dX_A + dY_B
 * with site B's dY product ([Bm ; wbar]^T dV + dR^T Q) as two more contraction segments of site A's dX pass, instead of one kernel that
 * overwrites dT and a second one that reads it back and adds (1 GB of HBM traffic less at BASELINE config 2's audio tokens).
 * Call after sections 1 + 32 + 8 of BOTH sites (their `saved` / `scratch` as those calls left them; B's workspaces are only read), in
 * place of section 64 of A and section 16 of B; the stream must be ordered behind both sites' section 8.  dT is overwritten.
 * Returns 0 = launched, 1 = these shapes are not served (nothing launched: run section 64 of A, then section 16 of B with
 * accumulate_dy), < 0 = error.  dT == NULL: nothing is launched, the return value only says whether the shapes are served.
 * Served: bf16 pairs of the tuned shape (one streaming kernel, csrc/dx_stream3.hip) and -- round 6 -- fp32 pairs of ANY shape without the AVVP N x N /
 * frame-attention / latent-self-attention variants on site A (the tiled engine with site B's product as a third and fourth K segment). */
int avmoe_moe_backward_dx_dy(const avmoe_moe_desc* desc_a, const void* X_a, void* saved_a, void* scratch_a,
                             const avmoe_moe_desc* desc_b, void* saved_b, void* scratch_b, void* dT, void* stream);

/* Sub-op (tests / partial adoption): the router alone -- Sequential(Linear(2C,128), ReLU, Linear(128,32), ReLU,
 * Linear(32,E)) + optional logit noise + softmax + first-max argmax  (net_trans_v3.py:460-466,477-479).
 * rin (S, 2C) f32 = [mean over tokens of x | mean over tokens of the remapped other modality]; same workspaces as the
 * site calls (rin is copied into `saved`; a following avmoe_moe_backward on it is not meaningful).  probs (S,E) f32,
 * idx (S) int64, lb (1 float, written only when desc.lb_loss) may each be NULL.                                    */
int avmoe_router_forward(const avmoe_moe_desc* desc, const float* rin, const avmoe_moe_ptrs* params, const float* noise,
                         float* probs, int64_t* idx, float* lb, void* saved, void* scratch, void* stream);

/* ABI 7 -- sub-ops (tests / partial adoption), same workspaces as the site calls; a following avmoe_moe_backward on them is not
 * meaningful.  The product path never materialises either; these exist so that a maintainer can compare the
 * library with the reference one module at a time.
 * avmoe_expert_forward_cross / _uni: what ExpertAdapter.forward returns for multimodal_experts[j] / singlemodal_experts[j]
 * (gate * LN_post(BN2(up(act(BN1(down(LN_before(x'))))))), net_trans_v3.py:377-435 ; mgn.py:132-139 and PVT_AVSModel_v2.py:210-227
 * for the unimodal variants) into out (S, N, C): the site forward with the router pushed to an exact one-hot on that expert.  In
 * training mode only THAT expert's BatchNorm running statistics and counters advance (the others' updates are discarded); a
 * non-finite value in another expert's output propagates (0 * Inf), as in the reference's mixture.
 * avmoe_remap_forward: the remapped other modality, materialised -- Yt = conv_adapter(Y) (S, N, Cy) and Yf = fc(Yt) (S, N, C), the
 * `vis_token` every expert and the router read (net_trans_v3.py:469-471); both in desc.dtype, both written.                      */
int avmoe_expert_forward_cross(const avmoe_moe_desc* desc, const void* X, const void* Y, const avmoe_moe_ptrs* params, int32_t j,
                               void* out, void* saved, void* scratch, void* stream);
int avmoe_expert_forward_uni(const avmoe_moe_desc* desc, const void* X, const void* Y, const avmoe_moe_ptrs* params, int32_t j,
                             void* out, void* saved, void* scratch, void* stream);
int avmoe_remap_forward(const avmoe_moe_desc* desc, const void* Y, const avmoe_moe_ptrs* params, void* Yt, void* Yf, void* saved,
                        void* scratch, void* stream);

/* Workspace introspection for tests: buffer `index` -> name / region (0 saved, 1 scratch) / offset / bytes.
 * Returns 0, or AVMOE_ERR_BAD_ARG when index is past the last buffer.                                 */
int avmoe_moe_buffer_info(const avmoe_moe_desc* desc, int32_t index, const char** name, int32_t* region,
                          size_t* offset, size_t* bytes);


/* ---- either side of the path on the training loop ---------------------------------------
 * avmoe_adam_step: one torch.optim.Adam step (no amsgrad; L2 weight_decay added to the gradient) over a FLAT fp32
 * parameter bucket -- replaces optimizer.step() over the adapter parameters (AVE/main_trans_v3.py:322).  `step` is the
 * 1-based step count (bias correction), grad_scale multiplies the gradient first (1/accum_itr, 1/world ...).
 * avmoe_expert_histogram: counts[e] += #{s : idx[s] == e} on the device (int64 counts, exact) -- replaces the host loop
 * over idx.tolist() that fills the expert-activation tables (AVE/main_trans_v3.py:183-207).                          */
int avmoe_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float lr, float beta1,
                    float beta2, float eps, float weight_decay, int64_t step, float grad_scale, void* stream);
int avmoe_expert_histogram(const int64_t* idx, int64_t S, int32_t E, int64_t* counts, void* stream);
/* ABI 4 -- dst1 += src1 and dst2 += src2 (n1 / n2 elements of `dtype`, 16-byte aligned) in ONE launch: how the two token tensors of a
 * site pair (net_trans_v3.py:695-698) collect their second gradient when the two sites' backward passes ran on two streams.   */
int avmoe_add2(void* dst1, const void* src1, int64_t n1, void* dst2, const void* src2, int64_t n2, int32_t dtype, void* stream);
/* Extension (no reference counterpart; BASELINE config 3 "router top-k=2"): idx (S, k) int64 = the k most probable experts of
 * every frame from probs (S, E) f32, most probable first, equal probabilities in expert order -- column 0 is the forward's
 * first-max argmax.  It only reports the selection; a top-k MIXTURE is avmoe_moe_forward_topk.                           */
int avmoe_router_topk(const float* probs, int64_t S, int32_t E, int32_t k, int64_t* idx, void* stream);

/* ---- optimizer with device-side state (added under ABI 11; AVMOE_ABI_VERSION unchanged, a binding finds these by symbol) ----------
 * Global-norm gradient clipping, Adam / AdamW, skipping of a step whose gradient is not finite, and a step count that lives on the
 * device -- over EVERY flat range the optimizer owns in three launches per step whatever the number of buckets and ranges (two when
 * neither clipping nor skipping is asked for), without a host synchronisation and without a host scalar that changes from step to
 * step, so a step can be captured into a graph and replayed.  avmoe_adam_step above is unchanged and stays the plain path.
 *
 * The range table.  One avmoe_opt_range per flat range: four DEVICE pointers to n fp32 elements each (16-byte aligned: AVMOE_ERR_ALIGNMENT
 * otherwise), the range's learning rate and weight decay.  A norm counts exactly the n elements of every range: alignment padding
 * between the parameters of a bucket belongs to no range.  avmoe_opt_table_build writes the table IMAGE (the ranges and a block -> range
 * map, one block per 1024 elements) into HOST memory of the caller, who copies it to the device -- once, and again when a learning rate
 * changes (the library never allocates and never copies).  avmoe_opt_workspace_bytes returns the device bytes of state block + table +
 * partial sums (each a multiple of 16; 0 and an error string on a bad range list) and fills `layout` (may be NULL).
 *
 * The state block (device, 16-byte aligned, zeroed by the caller before the first step) is written by avmoe_opt_grad_norm and read by
 * avmoe_opt_adam_step; a caller may read it back for logging or write the counters to resume a run.                                     */
typedef struct avmoe_opt_range {
  float* param; const float* grad; float* exp_avg; float* exp_avg_sq;
  int64_t n;
  float lr, weight_decay;
} avmoe_opt_range;

typedef struct avmoe_opt_state {
  float total_norm;           /* sqrt(sum (grad * grad_scale)^2) over every element of every range; 0 when no norm was asked for
                                 (none of AVMOE_OPT_CLIP, AVMOE_OPT_SKIP_NONFINITE, AVMOE_OPT_REPORT) */
  float clip_coef;            /* min(1, max_norm / (total_norm + 1e-6)) -- torch.nn.utils.clip_grad_norm_; exactly 1 when clipping is off */
  float bc1, bc2_sqrt;        /* 1 - beta1^applied_steps ; sqrt(1 - beta2^applied_steps): computed in double, rounded to fp32 */
  int64_t applied_steps;      /* steps that updated the parameters */
  int64_t skipped_steps;      /* steps held back because the norm was not finite */
  int32_t skip;               /* this step is held back */
  float lr_factor;            /* AVMOE_OPT_LR_SCHEDULE / AVMOE_OPT_SWA_LR: the factor of the last applied step (below); never written without one of them */
  float ema_decay;            /* AVMOE_OPT_EMA / AVMOE_OPT_SWA: the weight average's decay d of the last applied step (below); never written without one of them
                                 -- except by avmoe_opt_sf_step, the ONE step entry point that writes the state block: it leaves its d = 1 - c here */
  int32_t reserved[5];
} avmoe_opt_state;

typedef struct avmoe_opt_layout { size_t state_bytes, table_bytes, partial_bytes; int64_t n_blocks; } avmoe_opt_layout;

enum { AVMOE_OPT_CLIP = 1, AVMOE_OPT_SKIP_NONFINITE = 2, AVMOE_OPT_DECOUPLED_DECAY = 4, AVMOE_OPT_LR_SCHEDULE = 8, AVMOE_OPT_EMA = 16 };

size_t avmoe_opt_workspace_bytes(const avmoe_opt_range* ranges /* HOST */, int32_t n_ranges, avmoe_opt_layout* layout /* HOST, or NULL */);
int avmoe_opt_table_build(const avmoe_opt_range* ranges /* HOST */, int32_t n_ranges, void* image /* HOST, layout.table_bytes */,
                          size_t image_bytes);

/* The norm pass and its finalize step.  One launch over all ranges squares every element as a double ((double)grad * grad_scale) and
 * leaves one double per block in `partials` (layout.partial_bytes); one more launch of a single block adds them in a fixed order -- no
 * floating-point atomics, the same input gives the same bits -- and its last thread writes the state block:
 *     total_norm, clip_coef (AVMOE_OPT_CLIP; max_norm >= 0), skip = AVMOE_OPT_SKIP_NONFINITE && !isfinite(total_norm),
 *     applied_steps += !skip, skipped_steps += skip, bc1, bc2_sqrt for the new applied_steps
 * (and lr_factor under AVMOE_OPT_LR_SCHEDULE: avmoe_opt_grad_norm_sched below).
 * With neither flag the norm launch is left out (total_norm = 0) and only the counters and bias corrections advance.  The sum is exact
 * to double rounding, so total_norm is the true norm to two fp32 roundings.  `table`, n_ranges, n_blocks: the image on the device and
 * what it was built for (a kernel whose grid does not match its table's header does nothing).
 *
 * The update.  One launch walks the table; per element g = grad * (grad_scale * clip_coef), then
 *     coupled decay (default): exactly avmoe_adam_step's arithmetic (g += weight_decay * p ; exp_avg, exp_avg_sq, p) -- bit-equal to it
 *                              where clip_coef is 1 and the bias corrections agree;
 *     AVMOE_OPT_DECOUPLED_DECAY: p *= 1 - lr * weight_decay first, then the update without the decay term (torch.optim.AdamW).
 * When `skip` is set nothing is written.  The GRADIENT buffers are never written: unlike torch.nn.utils.clip_grad_norm_, which rescales
 * the gradients in place, the factor is applied inside the update, and a caller that reads the gradients afterwards sees them unclipped.
 * Call avmoe_opt_grad_norm before avmoe_opt_adam_step on the same stream, with the same grad_scale and betas, every step.
 * Errors (before any launch): AVMOE_ERR_BAD_ARG for NULL pointers, a negative range count / length, max_norm negative or NaN, betas
 * outside [0, 1), a state block that is not 16-byte aligned; AVMOE_ERR_ALIGNMENT for a table entry or table that is not.               */
int avmoe_opt_grad_norm(const void* table, int32_t n_ranges, int64_t n_blocks, double* partials, avmoe_opt_state* state, float grad_scale,
                        float max_norm, int32_t flags, float beta1, float beta2, void* stream);
int avmoe_opt_adam_step(const void* table, int32_t n_ranges, int64_t n_blocks, const avmoe_opt_state* state, float beta1, float beta2,
                        float eps, float grad_scale, int32_t flags, void* stream);

/* A per-step learning-rate schedule evaluated on the device (added under ABI 11 like the block above; found by symbol).  The schedule is
 * a function of applied_steps alone, so it costs no launch and no host scalar that changes from step to step: a scheduled step stays 3
 * launches (2 without a norm) and replays from a captured graph, and a step that is skipped holds the schedule back by itself.
 * avmoe_opt_schedule holds HOST constants that are fixed for a run.  With n = applied_steps before this update (the first applied step
 * has n = 0), W = warmup_steps, s0 = warmup_start, fmin = min_factor:
 *     n <  W:  f = s0 + (1 - s0) * n / W
 *     n >= W:  u = n - W, D = total_steps - W, c = min(u, D)
 *              AVMOE_SCHED_COSINE  f = fmin + (1 - fmin) * 0.5 * (1 + cos(pi * c / D))
 *              AVMOE_SCHED_LINEAR  f = 1 - (1 - fmin) * c / D
 *              AVMOE_SCHED_STEP    f = gamma ^ (u / step_size), integer division
 *              AVMOE_SCHED_NONE    f = 1
 * avmoe_opt_grad_norm_sched is avmoe_opt_grad_norm with one more argument; with AVMOE_OPT_LR_SCHEDULE in `flags` its finalize step
 * evaluates f in double from the fp32 constants, rounds it once to fp32 and writes state->lr_factor (a skipped step leaves it as it
 * was); without the flag `sched` is not read and the call is avmoe_opt_grad_norm.  avmoe_opt_adam_step with the flag then uses
 * lr * lr_factor in place of each range's lr, in the update and in the decoupled decay term alike; f = 1 gives the bits of the
 * unscheduled step.  Pass the flag to both calls of a step.  avmoe_opt_grad_norm itself refuses the flag (it has no schedule), and
 * without the flag both entry points launch what they did before and write the same bits.
 * Errors (AVMOE_ERR_BAD_ARG, before any launch): the flag with sched == NULL, a negative warmup_steps / total_steps / step_size,
 * warmup_start or min_factor outside [0, 1] or NaN, gamma outside (0, 1] or NaN, total_steps <= warmup_steps for COSINE / LINEAR,
 * step_size <= 0 for STEP, an unknown decay_kind.  The fields are ordered so that the struct packs into 40 bytes without padding
 * (gamma ahead of step_size).                                                                                     */
enum { AVMOE_SCHED_NONE = 0, AVMOE_SCHED_COSINE = 1, AVMOE_SCHED_LINEAR = 2, AVMOE_SCHED_STEP = 3 };

typedef struct avmoe_opt_schedule {
  int64_t warmup_steps;       /* W: steps of linear warm-up from warmup_start to 1 (0: none) */
  float warmup_start;         /* s0 in [0, 1] */
  int32_t decay_kind;         /* AVMOE_SCHED_* */
  int64_t total_steps;        /* the end of the decay, counted from step 0 (COSINE / LINEAR); the factor stays at min_factor from there on */
  float min_factor;           /* fmin in [0, 1] */
  float gamma;                /* STEP: in (0, 1] */
  int64_t step_size;          /* STEP: > 0 */
} avmoe_opt_schedule;

int avmoe_opt_grad_norm_sched(const void* table, int32_t n_ranges, int64_t n_blocks, double* partials, avmoe_opt_state* state, float grad_scale,
                              float max_norm, int32_t flags, float beta1, float beta2, void* stream, const avmoe_opt_schedule* sched /* HOST */);

/* An exponential moving average of the parameters kept on the device (added under ABI 11 like the two blocks above; found by symbol): the
 * weights a fine-tuning run evaluates and checkpoints in place of the raw ones.  Every range has a SHADOW buffer of n fp32 elements
 * (device, 16-byte aligned, initialised by the caller -- usually to the parameters).  The shadow pointers do not ride in avmoe_opt_range:
 * `shadows` is a DEVICE array of n_ranges float*, entry i belonging to range i of the table (8-byte aligned; NULL gives
 * AVMOE_ERR_BAD_ARG, a misaligned array AVMOE_ERR_ALIGNMENT; the library cannot read the entries, so a kernel that finds an entry that
 * is not 16-byte aligned, or an n_ranges that is not its table's, touches nothing).  avmoe_opt_ema holds HOST constants that are fixed
 * for a run.  With n = applied_steps AFTER this update (the first applied step has n = 1), W = warmup:
 *     d_n = min(decay, (1 + n) / (W + n))
 * W = 1 is a constant decay; W = 10 is the usual warm-up that lets the average follow the first steps closely (d_1 = 2 / 11).
 * avmoe_opt_grad_norm_ema is avmoe_opt_grad_norm_sched with one more argument; with AVMOE_OPT_EMA in `flags` its finalize step evaluates
 * d_n in double from the fp32 constants, rounds it once to fp32 and writes state->ema_decay (a skipped step leaves it as it was);
 * AVMOE_OPT_LR_SCHEDULE may be set in the same call.  avmoe_opt_adam_step_ema with the flag then computes, in the thread that has just
 * produced the element's new value p,
 *     shadow = fma(d, shadow, (1 - d) * p)            (fp32; (1 - d) and the product rounded, then one fused multiply-add)
 * so the update and the average are ONE launch: a step stays 3 launches (2 without a norm) and reads and writes two more 4-byte streams
 * per element.  A skipped step writes nothing, the shadows included.  p, exp_avg and exp_avg_sq get the bits they get without the flag.
 * Pass the flag to both calls of a step; without it neither entry point reads its last argument and both launch what
 * avmoe_opt_grad_norm_sched / avmoe_opt_adam_step launch.  Those older entry points refuse the flag.
 * avmoe_opt_swap_ema exchanges param[i] and shadow[i] for every element of every range in one launch (alignment padding belongs to no
 * range and is not touched): call it once to evaluate with the averaged weights and once more to go on training.
 * Errors (before any launch): AVMOE_ERR_BAD_ARG for the flag with ema == NULL, decay outside [0, 1) or NaN, warmup < 1, NaN or
 * infinite, shadows == NULL; AVMOE_ERR_ALIGNMENT for a shadow array that is not 8-byte aligned; and everything the older entry points
 * refuse.  Tensors that are no range of the table: BatchNorm running statistics are averaged by avmoe_opt_ema_buffers below; parameters
 * the optimizer does not hold are not covered.                                                                                        */
typedef struct avmoe_opt_ema {
  float decay;                /* in [0, 1): the decay the average settles at */
  float warmup;               /* W >= 1 */
} avmoe_opt_ema;

int avmoe_opt_grad_norm_ema(const void* table, int32_t n_ranges, int64_t n_blocks, double* partials, avmoe_opt_state* state, float grad_scale,
                            float max_norm, int32_t flags, float beta1, float beta2, void* stream, const avmoe_opt_schedule* sched /* HOST, or NULL */,
                            const avmoe_opt_ema* ema /* HOST */);
int avmoe_opt_adam_step_ema(const void* table, int32_t n_ranges, int64_t n_blocks, const avmoe_opt_state* state, float beta1, float beta2,
                            float eps, float grad_scale, int32_t flags, void* stream, float* const* shadows /* DEVICE */);
int avmoe_opt_swap_ema(const void* table, int32_t n_ranges, int64_t n_blocks, float* const* shadows /* DEVICE */, void* stream);

/* Averaged buffers (added under ABI 11 like the blocks above; found by symbol): the floating-point state of a model that is no parameter
 * -- BatchNorm running mean and variance -- averaged and swapped together with the weights, so that an evaluation with the averaged
 * weights runs on statistics that belong to them.  Such a tensor stays where it is (the site kernels write it in place through cached
 * addresses) and may be only 4-byte aligned, so it cannot be a range of the range table: the BUFFER TABLE is a second table, one
 * avmoe_opt_buffer per tensor -- the buffer (DEVICE, n fp32, 4-byte aligned), its shadow (DEVICE, n fp32, 16-byte aligned; the caller
 * keeps all shadows in one flat allocation and initialises them, usually to the buffers) and n -- followed by a block -> record map, one
 * block per 1024 elements of one buffer.  avmoe_opt_buffer_table_bytes returns the bytes of the image (a multiple of 16; 0 and an error
 * string on a bad list) and the block count; avmoe_opt_buffer_table_build writes the image into HOST memory of the caller, who copies
 * it to the device (16-byte aligned) once.  Image layout: {uint32 magic; int32 n_buffers; int64 n_blocks}, the records, then n_blocks
 * pairs {int32 record; int32 block inside the record}, sorted by record.
 * avmoe_opt_ema_buffers is ONE launch over all buffers, to be called behind avmoe_opt_adam_step_ema of a step with AVMOE_OPT_EMA, on the
 * same stream: it reads `skip` and `ema_decay` from the state block that step's finalize launch has written and computes
 *     shadow = fma(d, shadow, (1 - d) * buffer)       (fp32; the expression of the parameter average, one helper in csrc/adam_elem.h)
 * for every element; a skipped step writes nothing, and the buffers themselves are only read.  avmoe_opt_swap_buffers exchanges
 * buffer[i] and shadow[i] for every element in one launch, in place: call it beside avmoe_opt_swap_ema.  No host scalar changes from
 * step to step, so both replay from a captured graph.  A launch whose n_buffers / n_blocks are not its table's touches nothing.
 * Errors (before any launch): AVMOE_ERR_BAD_ARG for a NULL table or state, a negative count, a state block that is not 16-byte aligned,
 * (table functions) a NULL pointer or negative length in a record; AVMOE_ERR_ALIGNMENT for a table that is not 16-byte aligned,
 * (table functions) a buffer that is not 4-byte or a shadow that is not 16-byte aligned; AVMOE_ERR_WORKSPACE for an image too small.  */
typedef struct avmoe_opt_buffer {
  float* buffer;              /* DEVICE: the tensor itself, read by the average, exchanged by the swap */
  float* shadow;              /* DEVICE: its average */
  int64_t n;                  /* elements */
} avmoe_opt_buffer;

size_t avmoe_opt_buffer_table_bytes(const avmoe_opt_buffer* buffers /* HOST */, int32_t n_buffers, int64_t* n_blocks /* HOST, or NULL */);
int avmoe_opt_buffer_table_build(const avmoe_opt_buffer* buffers /* HOST */, int32_t n_buffers, void* image /* HOST */, size_t image_bytes);
int avmoe_opt_ema_buffers(const void* table, int32_t n_buffers, int64_t n_blocks, const avmoe_opt_state* state, void* stream);
int avmoe_opt_swap_buffers(const void* table, int32_t n_buffers, int64_t n_blocks, void* stream);

/* The gradient norm of every range and the first range whose norm is not finite (added under ABI 11 like the blocks above; found by
 * symbol): which parameter made a step skip, or whose gradient is out of line with its neighbours', without a .norm() per tensor.  The
 * norm pass already leaves one double per 1024-element block and every block belongs to one range, so the per-range norms are a
 * segmented sum of numbers the step has computed anyway.
 * The report buffer (DEVICE, 16-byte aligned, avmoe_opt_report_bytes(n_ranges) bytes: the 16-byte header, then n_ranges floats, rounded
 * up to 16; 0 and an error string on a negative count) needs no initialisation.
 * avmoe_opt_grad_norm_report is avmoe_opt_grad_norm_ema with one more argument and knows every flag.  With AVMOE_OPT_REPORT in `flags`:
 *   - the norm launch runs whether or not clipping or skipping is on, and total_norm is the true norm also with neither (it is 0 there
 *     without the flag -- the one difference; clip_coef stays exactly 1);
 *   - the finalize launch resets the header, and ONE more launch (a step is 4 launches then) gives a wave to every range: lane l adds the
 *     range's block sums l, l + 64, ... in order, a fixed butterfly adds the 64 lane sums, and
 *         norms[r] = (float)sqrt(sum of range r's block sums, in double)          (a range of length 0 reports 0)
 *     No floating-point atomics: the same input gives the same bits.  first_nonfinite = the lowest r whose norms[r] is Inf or NaN, or -1
 *     (an integer minimum, which does not depend on the order).  Both are rewritten every step, a skipped step included;
 *   - every word of the state block but total_norm in the case above, and with it parameters, moments and averages, gets the bits it
 *     gets without the flag: the global sum keeps its own order of additions and is not rebuilt from the per-range sums.
 * The norms are those of grad * grad_scale, before clipping.  No host synchronisation, no allocation, no host scalar that changes from
 * step to step: a captured step rewrites the report on replay.  Without the flag `report` is not read and the call is
 * avmoe_opt_grad_norm_ema; avmoe_opt_adam_step_ema does not know the flag and needs no change (pass it the flags without it).
 * Errors (before any launch): AVMOE_ERR_BAD_ARG for the flag with report == NULL, AVMOE_ERR_ALIGNMENT for a report that is not 16-byte
 * aligned, and everything avmoe_opt_grad_norm_ema refuses.  The older entry points refuse the flag ("unknown flag").                  */
enum { AVMOE_OPT_REPORT = 32 };

typedef struct avmoe_opt_report_header {
  int32_t first_nonfinite;    /* the lowest range index whose norm is not finite, or -1 */
  int32_t n_ranges;           /* the floats that follow the header */
  int32_t reserved[2];
} avmoe_opt_report_header;

size_t avmoe_opt_report_bytes(int32_t n_ranges);
int avmoe_opt_grad_norm_report(const void* table, int32_t n_ranges, int64_t n_blocks, double* partials, avmoe_opt_state* state, float grad_scale,
                               float max_norm, int32_t flags, float beta1, float beta2, void* stream, const avmoe_opt_schedule* sched /* HOST, or NULL */,
                               const avmoe_opt_ema* ema /* HOST, or NULL */, void* report /* DEVICE, 16-byte aligned */);

/* Stochastic weight averaging (added under ABI 11 like the blocks above; found by symbol): torch.optim.swa_utils on the device -- the
 * UNIFORM average of the weights over the tail of a run (AveragedModel), and the learning rate annealed to a constant for that tail
 * (SWALR).  Both are functions of applied_steps alone, evaluated by the finalize launch into the two words of the state block the
 * schedule and the exponential average already use, so neither costs a launch, a counter or a host scalar that changes from step to
 * step: the state block stays 64 bytes, a step stays 3 launches (4 with averaged buffers), replays from a captured graph, and a skipped
 * step advances nothing.  avmoe_opt_swa holds HOST constants that are fixed for a run.
 * AVMOE_OPT_SWA, the average.  With n = applied_steps AFTER this update (the first applied step has n = 1), N = start, c = freq:
 *     n <  N:                     d = 0            the shadow follows the parameters
 *     n >= N, (n - N) % c == 0:   k = (n - N) / c, d = k / (k + 1)   -- AveragedModel.update_parameters with n_averaged = k; the first
 *                                                  averaged step copies the parameters
 *     otherwise:                  d = 1            the shadow keeps its value
 * d is formed in double, rounded once to fp32 and written to state->ema_decay; the number of models averaged so far is
 * (n - N) / c + 1 for n >= N, so no counter is kept.  The update is that of AVMOE_OPT_EMA, shadow = fma(d, shadow, (1 - d) * p), by the
 * same kernels: pass AVMOE_OPT_EMA (not AVMOE_OPT_SWA) to avmoe_opt_adam_step_ema, and call avmoe_opt_ema_buffers / avmoe_opt_swap_ema /
 * avmoe_opt_swap_buffers as for the exponential average.  AVMOE_OPT_SWA and AVMOE_OPT_EMA in one call are refused.
 * AVMOE_OPT_SWA_LR, the learning rate.  With n = applied_steps BEFORE this update (the schedule's convention), N' = lr_start,
 * A = anneal_steps, s = lr_factor, base(n) = the factor of `sched` under AVMOE_OPT_LR_SCHEDULE and 1 without that flag (`sched` is then
 * not read and may be NULL):
 *     n <  N':  f = base(n)
 *     n >= N':  f0 = base(N'), t = A == 0 ? 1 : min(1, (n - N') / A),
 *               alpha = t (AVMOE_SWA_ANNEAL_LINEAR) or (1 - cos(pi t)) / 2 (AVMOE_SWA_ANNEAL_COS), f = f0 + (s - f0) * alpha
 * -- SWALR(swa_lr = s * lr0, anneal_epochs = A) constructed when step N' is due and stepped once per applied step, in closed form.  f
 * is evaluated in double, rounded once to fp32 and written to state->lr_factor: pass AVMOE_OPT_LR_SCHEDULE (not AVMOE_OPT_SWA_LR) to
 * avmoe_opt_adam_step_ema.  Either flag may be used without the other; the fields of the one that is off are not read.
 * avmoe_opt_grad_norm_swa is avmoe_opt_grad_norm_report with one more argument and knows every flag; without the two flags `swa` is not
 * read and the call is avmoe_opt_grad_norm_report: the same kernels are launched and every written bit is the same.  The older entry
 * points, avmoe_opt_grad_norm_report included, refuse both flags ("unknown flag").
 * Errors (AVMOE_ERR_BAD_ARG, before any launch): either flag with swa == NULL; AVMOE_OPT_SWA with start < 1 or freq < 1, or together with
 * AVMOE_OPT_EMA; AVMOE_OPT_SWA_LR with lr_start < 0, anneal_steps < 0, lr_factor outside [0, 1] or NaN, an unknown anneal_kind; and
 * everything avmoe_opt_grad_norm_report refuses.  32 bytes without padding (the two periods are 32-bit).                                                          */
enum { AVMOE_OPT_SWA = 64, AVMOE_OPT_SWA_LR = 128 };
enum { AVMOE_SWA_ANNEAL_COS = 0, AVMOE_SWA_ANNEAL_LINEAR = 1 };

typedef struct avmoe_opt_swa {
  int64_t start;              /* N >= 1: the first applied step (counted from 1) that enters the average */
  int64_t lr_start;           /* N' >= 0: the first step (counted from 0) of the annealed learning rate */
  int32_t freq;               /* c >= 1: every c-th applied step from `start` on enters the average */
  int32_t anneal_steps;       /* A >= 0: steps from base(N') to lr_factor (0: at once) */
  float lr_factor;            /* s in [0, 1]: the factor the learning rate settles at */
  int32_t anneal_kind;        /* AVMOE_SWA_ANNEAL_* */
} avmoe_opt_swa;

int avmoe_opt_grad_norm_swa(const void* table, int32_t n_ranges, int64_t n_blocks, double* partials, avmoe_opt_state* state, float grad_scale,
                            float max_norm, int32_t flags, float beta1, float beta2, void* stream, const avmoe_opt_schedule* sched /* HOST, or NULL */,
                            const avmoe_opt_ema* ema /* HOST, or NULL */, void* report /* DEVICE, 16-byte aligned, or NULL */,
                            const avmoe_opt_swa* swa /* HOST */);

/* Sharpness-aware minimization, SAM and its adaptive form ASAM (added under ABI 11 like the blocks above; found by symbol): a step takes
 * the gradient at w + e, the point in the ball of radius rho around the weights w where a first gradient g says the loss is highest, and
 * applies it to w itself.  Two calls serve it, beside the calls of a step: avmoe_opt_sam_perturb after the first backward pass moves the
 * parameters to w + e and keeps w, avmoe_opt_adam_step_sam after the second one updates w.  Every range has a HOLD buffer of n fp32
 * elements (device, 16-byte aligned, needs no initialisation); `hold` is a DEVICE array of n_ranges float*, entry i belonging to range i
 * of the table, under the rules of `shadows` above.  No flag: the norm pass of the second gradient is avmoe_opt_grad_norm_swa (or an
 * older one) unchanged, and every entry point above keeps refusing the flags it refuses.
 * avmoe_opt_sam_perturb is THREE launches on `stream`, whatever the number of ranges, without a host synchronisation and without a host
 * scalar that changes from step to step (rho, grad_scale and `adaptive` are constants of a run), so it replays from a captured graph:
 *   1. the norm pass: one double per 1024-element block in `partials`, the sum of ((double)grad * grad_scale)^2 -- the very kernel of
 *      avmoe_opt_grad_norm -- or, adaptive, of ((double)(|p| * grad) * grad_scale)^2 with |p| * grad rounded to fp32;
 *   2. one block adds the partial sums in the order of avmoe_opt_grad_norm's finalize launch (the same helper) and writes *sam:
 *          norm = (float)sqrt(sum), scale = (float)(rho / ((double)norm + 1e-12)), nonfinite = 0
 *      or, when norm is Inf or NaN, scale = 0 and nonfinite = 1.  Not adaptive, `norm` has the bits state->total_norm gets from the same
 *      gradient and grad_scale under AVMOE_OPT_REPORT;
 *   3. per element of every range, in fp32 with every product rounded (one helper in csrc/adam_elem.h):
 *          hold = p ;  e = scale * (grad * grad_scale)   or, adaptive,   e = (scale * (p * p)) * (grad * grad_scale) ;  p = p + e
 *      With `nonfinite` set hold is still written and p is not; e == 0 (a zero gradient) leaves p's bits as they are.
 * Gradients and moments are only read, the optimizer's state block is not touched, alignment padding belongs to no range and is not
 * touched.  `partials` is the workspace of the norm pass (layout.partial_bytes): the step's own norm pass overwrites it later.
 * avmoe_opt_adam_step_sam is avmoe_opt_adam_step_ema in which every element's p is READ from hold and the result is written to param:
 * still one launch, the flags of avmoe_opt_adam_step_ema, and param, exp_avg, exp_avg_sq and the shadows get exactly the bits
 * avmoe_opt_adam_step_ema gives from the unperturbed parameters with the same gradient -- the restoration is a copy, not p + e - e.
 * When state->skip is set it writes param = hold and NOTHING else: a skipped step still undoes the perturbation.  A step without a
 * perturbation before it is avmoe_opt_adam_step_ema.  avmoe_opt_swap_ema with `hold` in place of `shadows` abandons a perturbation (param
 * gets the kept values back; hold gets the perturbed ones, which nobody reads).
 * Errors (before any launch).  avmoe_opt_sam_perturb: AVMOE_ERR_BAD_ARG for a NULL table, partials (with n_blocks > 0), sam or hold, a
 * negative count, rho negative, NaN or infinite, grad_scale NaN, `adaptive` not 0 or 1, a sam block that is not 16-byte aligned;
 * AVMOE_ERR_ALIGNMENT for a hold array or partials that are not 8-byte aligned or a table that is not 16-byte aligned.
 * avmoe_opt_adam_step_sam: AVMOE_ERR_BAD_ARG for hold == NULL, AVMOE_ERR_ALIGNMENT for a hold array that is not 8-byte aligned, and
 * everything avmoe_opt_adam_step_ema refuses.                                                                                        */
typedef struct avmoe_opt_sam_state {   /* DEVICE, 16 bytes, 16-byte aligned, needs no initialisation */
  float norm;                 /* ||g * grad_scale||  (adaptive: |||p| * g * grad_scale||) of the perturbing gradient */
  float scale;                /* rho / (norm + 1e-12) formed in double, rounded once to fp32; 0 when norm is Inf / NaN */
  int32_t nonfinite;          /* 1: the norm was not finite and the parameters were left as they are */
  int32_t reserved;
} avmoe_opt_sam_state;

int avmoe_opt_sam_perturb(const void* table, int32_t n_ranges, int64_t n_blocks, double* partials, avmoe_opt_sam_state* sam, float grad_scale,
                          float rho, int32_t adaptive, float* const* hold /* DEVICE array of n_ranges float*, as `shadows` */, void* stream);
int avmoe_opt_adam_step_sam(const void* table, int32_t n_ranges, int64_t n_blocks, const avmoe_opt_state* state, float beta1, float beta2,
                            float eps, float grad_scale, int32_t flags, void* stream, float* const* shadows /* DEVICE, or NULL without AVMOE_OPT_EMA */,
                            float* const* hold /* DEVICE */);

/* Layer-wise trust ratios, LAMB (You et al. 2020; added under ABI 11 like the blocks above; found by symbol): every range's step is
 * rescaled by ||p|| / ||u||, the norm of the range's parameters over the norm of its update direction, which keeps the relative change of
 * every tensor near lr whatever the batch size has done to the gradient's scale.  No flag and no new word in the state block:
 * avmoe_opt_lamb_step is called IN PLACE of avmoe_opt_adam_step_ema / avmoe_opt_adam_step_sam, behind the unchanged norm call of a step
 * (avmoe_opt_grad_norm_report / avmoe_opt_grad_norm_swa), on the same stream with the same grad_scale and betas, and every entry point
 * above keeps refusing the flags it refuses.  With g' = grad * (grad_scale * clip_coef), per element of range r, every operation rounded to
 * fp32 in the order written (csrc/adam_elem.h: lamb_moments, lamb_dir, lamb_next; contraction off):
 *     coupled decay:                                gr = fma(gscale, grad, wd * p) ;  m, v from gr as avmoe_opt_adam_step forms them ;
 *                                                   u = (m / bc1) / (sqrt(v) / bc2_sqrt + eps)
 *     AVMOE_OPT_DECOUPLED_DECAY (the paper's LAMB):  gr = grad * gscale ;  m, v from gr ;  u = (m / bc1) / (sqrt(v) / bc2_sqrt + eps) + wd * p
 *     ratio_r = ||p_r|| / ||u_r||, both norms summed in double and the quotient formed in double, rounded once to fp32 ;
 *               1 where either norm is 0 or not finite, and for a range that is not adapted ; min(ratio, limit) where the range has one
 *     p = p - ((lr_r * lr_factor) * ratio_r) * u                     (lr_factor under AVMOE_OPT_LR_SCHEDULE)
 * p is the value before the step, for the norm too -- with hold != NULL (the step behind avmoe_opt_sam_perturb) the held value.  Bias
 * correction stays, as in the paper.  exp_avg and exp_avg_sq get the bits avmoe_opt_adam_step_ema gives them from the same p, gradient
 * and state block; the parameters do NOT (u is formed in another order than Adam's ((lr / bc1) * m) / (...)).
 * `limits` is a DEVICE array of n_ranges floats: < 0 the range is not adapted (ratio exactly 1.0f, through the same kernels), 0 adapted
 * without a clamp, > 0 the ratio is clamped to it.  `workspace` (DEVICE, 8-byte aligned) takes two doubles per table block; `report`
 * (DEVICE, 16-byte aligned) is the 16-byte avmoe_opt_lamb_header, then three arrays of n_ranges floats: w_norm, u_norm (the double square
 * roots rounded to fp32) and ratio.  Neither needs initialisation.  avmoe_opt_lamb_bytes returns both sizes (each a multiple of 16; 0 and
 * an error string on a negative count or more than 2^31 - 1 blocks) and their sum.
 * avmoe_opt_lamb_step is THREE launches on `stream` whatever the number of ranges, without a host synchronisation and without a host
 * scalar that changes from step to step, so it replays from a captured graph:
 *   1. one block per table block: the moments, and the block's sums of (double)u^2 and (double)p^2 into the workspace, u formed from the
 *      moments just stored;
 *   2. one wave per range adds the range's block sums in a fixed order (the walk of AVMOE_OPT_REPORT's launch; no floating-point atomics)
 *      and writes w_norm, u_norm and ratio into the report;
 *   3. one block per table block: u again, by the same helper from the same stored values, and the update; with AVMOE_OPT_EMA the shadow
 *      advances from the new p as in avmoe_opt_adam_step_ema.
 * When state->skip is set nothing is written, the report included -- with hold != NULL param = hold and nothing else.  Gradients are only
 * read; alignment padding belongs to no range and is not touched.  A launch that does not match its table's header, a shadow / hold entry
 * that is not 16-byte aligned or a pointer array made for another range count touches nothing, as in the kernels above.
 * `flags` are those of avmoe_opt_adam_step_ema; `shadows` may be NULL without AVMOE_OPT_EMA; hold == NULL is the step without a
 * perturbation before it.
 * Errors (before any launch): everything avmoe_opt_adam_step_sam refuses (hold != NULL) or avmoe_opt_adam_step_ema refuses (hold == NULL);
 * AVMOE_ERR_BAD_ARG for NULL limits, workspace or report; AVMOE_ERR_ALIGNMENT for limits that are not 4-byte, a workspace that is not
 * 8-byte or a report that is not 16-byte aligned.                                                                                     */
typedef struct avmoe_opt_lamb_header {
  int32_t n_ranges;           /* the floats in each of the three arrays that follow the header */
  int32_t reserved[3];
} avmoe_opt_lamb_header;

typedef struct avmoe_opt_lamb_layout { size_t workspace_bytes, report_bytes; } avmoe_opt_lamb_layout;

size_t avmoe_opt_lamb_bytes(int32_t n_ranges, int64_t n_blocks, avmoe_opt_lamb_layout* layout /* HOST, or NULL */);
int avmoe_opt_lamb_step(const void* table, int32_t n_ranges, int64_t n_blocks, const avmoe_opt_state* state, float beta1, float beta2,
                        float eps, float grad_scale, int32_t flags, void* stream, float* const* shadows /* DEVICE, or NULL without AVMOE_OPT_EMA */,
                        float* const* hold /* DEVICE, or NULL */, const float* limits /* DEVICE, n_ranges floats */,
                        double* workspace /* DEVICE */, void* report /* DEVICE, 16-byte aligned */);

/* Prodigy learning-rate estimation (Mishchenko & Defazio, "Prodigy: An Expeditiously Adaptive Parameter-Free Learner"; added under ABI 11
 * like the blocks above; found by symbol): the step size is lr_r * d with an estimate d of the distance to the solution that the step
 * itself maintains, from two global sums per step.  No flag and no new word in the state block: avmoe_opt_prodigy_step is called IN PLACE
 * of avmoe_opt_adam_step_ema / avmoe_opt_adam_step_sam, behind the unchanged norm call of a step, on the same stream with the same
 * grad_scale and betas, and every entry point above keeps refusing what it refuses.
 * State beyond Adam's: per element x0 (the parameter where the run started) and s (a running gradient sum, zero at the start), in flat
 * side buffers addressed by DEVICE arrays of n_ranges float* under the rules of `shadows`; and the 32-byte avmoe_opt_prodigy_state on the
 * device, which starts as {d0, d0, 0, 0, 0.0, 0.0}.  Constants of a run (avmoe_opt_prodigy, HOST): d0 > 0, d_coef > 0, growth >= 1 or
 * 0 for none, safeguard_warmup 0 / 1; and beta3 = fp32(sqrt((double)beta2)).
 * An applied step reads d from the block.  With gscale = grad_scale * clip_coef, per range r
 *     step_r = (lr_r * lr_factor) * d          (lr_factor under AVMOE_OPT_LR_SCHEDULE)
 *     c_r    = step_r * (d / d0)               (safeguard_warmup: c_r = d * (d / d0))
 * and per element, every operation rounded to fp32 in the order written (csrc/adam_elem.h: prodigy_elem; contraction off):
 *     coupled decay:              gr = fma(gscale, grad, wd * p)
 *     AVMOE_OPT_DECOUPLED_DECAY:  gr = grad * gscale ;  p <- p * (1 - step_r * wd) before the Adam term
 *     dg = d * gr ;  cg = c_r * gr
 *     m  = fma(b1, m, (1 - b1) * dg) ;  v = fma(b2, v, ((1 - b2) * dg) * dg) ;  s = fma(beta3, s, cg)
 *     p  = p - (step_r * m) / (sqrt(v) + d * eps)
 * and, in double, per 1024-element table block:  sum of (double)cg * ((double)x0 - (double)p) with p BEFORE the step (with hold != NULL
 * the held value), and sum of (double)|s| with the new s.  There is no bias correction, as in the paper.  With d == 1 the moments are
 * the bits avmoe_opt_adam_step forms from the same gradient.
 * Underflow: (d * gr)^2 may underflow fp32 (a small d0 times a small gradient); v then holds what gradual underflow leaves, possibly 0.
 * Where sqrt(v) + d * eps is not > 0 (v == 0 with d * eps == 0, or a NaN) the quotient is not formed and the element's Adam term is
 * dropped: p keeps its (decayed) value while m, v, s and the sums advance.
 * Then ONE block adds the block sums in a fixed order (thread t blocks t, t + 256, ..., then a tree; no floating-point atomics) and
 * writes the block, in double unless stated:
 *     num   = beta3 * num + sum_dot ;  den = sum_abs
 *     d_hat = fp32(d_coef * num / den)         left as it is when den is not > 0, or num, den or the quotient is not a finite fp32
 *     d_max = max(d_max, d_hat)
 *     d     = min(d_max, fp32(d * growth))     growth == 0: d = d_max
 * so d never falls; the update of step k uses d_k, and step k + 1 reads d_{k+1}.
 * avmoe_opt_prodigy_step is TWO launches on `stream` whatever the number of ranges (kk_opt_prodigy_update<DECOUPLED, SCHED, EMA, HOLD>,
 * kk_opt_prodigy_finalize), without a host synchronisation and without a host scalar that changes from step to step, so it replays
 * from a captured graph.  `workspace` (DEVICE, 8-byte aligned) takes two doubles per table block and needs no initialisation;
 * avmoe_opt_prodigy_bytes returns its size and the block's (each a multiple of 16; 0 and an error string on a negative count or more
 * than 2^31 - 1 blocks) and their sum.
 * When state->skip is set nothing is written: d, num, den, s, x0, moments, parameters and the workspace keep their values -- with
 * hold != NULL param = hold and nothing else.  Gradients and x0 are only read; alignment padding belongs to no range and is not touched.
 * A launch that does not match its table's header touches nothing but the workspace; a range whose shadow / hold / x0 / s entry is not
 * 16-byte aligned, or pointer arrays made for another range count, are left out likewise (their block sums count as 0).
 * `flags` are those of avmoe_opt_adam_step_ema; `shadows` may be NULL without AVMOE_OPT_EMA; hold == NULL is the step without a
 * perturbation before it.
 * Errors (before any launch): everything avmoe_opt_adam_step_sam refuses (hold != NULL) or avmoe_opt_adam_step_ema refuses (hold == NULL);
 * AVMOE_ERR_BAD_ARG for NULL x0, s, consts, block or workspace, for a d0 or d_coef that is not a finite number > 0 (NaN included), a
 * growth that is neither 0 nor a finite number >= 1, a safeguard_warmup that is neither 0 nor 1; AVMOE_ERR_ALIGNMENT for pointer arrays
 * or a workspace that are not 8-byte or a block that is not 16-byte aligned.                                                          */
typedef struct avmoe_opt_prodigy_state {
  float d;                    /* the estimate the NEXT applied step uses */
  float d_max;                /* the largest d_hat so far (at least d0) */
  float d_hat;                /* the last estimate, which may be below d or negative */
  int32_t reserved;
  double num;                 /* the decayed sum of <c g, x0 - x> */
  double den;                 /* sum of |s| at the last applied step */
} avmoe_opt_prodigy_state;

typedef struct avmoe_opt_prodigy {
  float d0;                   /* > 0 */
  float d_coef;               /* > 0 */
  float growth;               /* >= 1: d grows by at most this factor per step; 0: no limit */
  int32_t safeguard_warmup;   /* 1: the weight of a step in s and num leaves the learning rate out (for use with a warm-up) */
} avmoe_opt_prodigy;

typedef struct avmoe_opt_prodigy_layout { size_t workspace_bytes, block_bytes; } avmoe_opt_prodigy_layout;

size_t avmoe_opt_prodigy_bytes(int64_t n_blocks, avmoe_opt_prodigy_layout* layout /* HOST, or NULL */);
int avmoe_opt_prodigy_step(const void* table, int32_t n_ranges, int64_t n_blocks, const avmoe_opt_state* state, float beta1, float beta2,
                           float eps, float grad_scale, int32_t flags, void* stream, float* const* shadows /* DEVICE, or NULL without AVMOE_OPT_EMA */,
                           float* const* hold /* DEVICE, or NULL */, float* const* x0 /* DEVICE */, float* const* s /* DEVICE */,
                           const avmoe_opt_prodigy* consts /* HOST */, avmoe_opt_prodigy_state* block /* DEVICE, 16-byte aligned */,
                           double* workspace /* DEVICE */);

/* Schedule-free AdamW (Defazio et al. 2024, "The Road Less Scheduled"; added under ABI 11 like the blocks above; found by symbol): a
 * constant rate after a warm-up, the gradient taken at an interpolation y of a base sequence z and a running average x, and x -- the
 * weights one evaluates -- as good as a tuned decay at whatever step the run stops.  No flag and no new word in the state block:
 * avmoe_opt_sf_step is called IN PLACE of avmoe_opt_adam_step_ema / avmoe_opt_adam_step_sam, behind the unchanged norm call of a step
 * (made WITHOUT AVMOE_OPT_EMA / AVMOE_OPT_SWA), on the same stream with the same grad_scale and betas.
 * State: y is the range's `param`, z lives in its `exp_avg`, v in `exp_avg_sq`, x in a flat side buffer per range addressed by a DEVICE
 * array of n_ranges float* under the rules of `shadows` (it IS the shadow: avmoe_opt_swap_ema exchanges y and x); z and x start as
 * copies of the parameters; and the 32-byte avmoe_opt_sf_state on the device, which starts all zero.  Constants of a run (avmoe_opt_sf,
 * HOST): r >= 0 and lr_power >= 0, both finite.
 * An applied step, with n = applied_steps after it (the first has n = 1) and f = lr_factor under AVMOE_OPT_LR_SCHEDULE, else 1.  First
 * ONE thread advances the block, in double, contraction off (the same for every range: a range's constant rate cancels in the ratio):
 *     f_max      = max(f_max, f)
 *     w          = pow(n, r) * pow(f_max, lr_power)          (pow(., 0) = 1)
 *     weight_sum = weight_sum + w
 *     c          = w / weight_sum                            (0 where weight_sum is not > 0: a warm-up that starts at factor 0)
 *     d          = fp32(1 - c)                               (c and d each rounded once to fp32)
 * and copies d into state->ema_decay, so that avmoe_opt_ema_buffers behind it averages the buffers with the same weight: the one place
 * a step entry point writes the state block.  Then per element, with gscale = grad_scale * clip_coef and y the parameter (with
 * hold != NULL the held value), every operation rounded to fp32 in the order written (csrc/adam_elem.h: sf_elem; contraction off):
 *     coupled decay:              gr = fma(gscale, grad, wd * y)
 *     AVMOE_OPT_DECOUPLED_DECAY:  gr = grad * gscale
 *     v = fma(b2, v, ((1 - b2) * gr) * gr)                   (Adam's bits for v from the same gr)
 *     u = gr / (sqrt(v) / bc2_sqrt + eps)                    (AVMOE_OPT_DECOUPLED_DECAY: u = u + wd * y)
 *     z = z - (lr_r * f) * u
 *     x = fma(d, x, (1 - d) * z)
 *     y = fma(b1, x, (1 - b1) * z)                           -> param
 * There is no momentum buffer and no first-moment bias correction: beta1 is the interpolation.  The first applied step has c = 1,
 * d = 0 and x = z exactly; beta1 = 0 gives y = z exactly.
 * avmoe_opt_sf_step is TWO launches on `stream` whatever the number of ranges (kk_opt_sf_weights: one block; kk_opt_sf_update<DECOUPLED,
 * SCHED, HOLD>: the table walk, five 4-byte streams read and four written per element), without a host synchronisation and without a
 * host scalar that changes from step to step, so it replays from a captured graph.  No floating-point atomics.
 * When state->skip is set nothing is written -- the block and state->ema_decay included; with hold != NULL param = hold and nothing
 * else.  Gradients are only read; alignment padding belongs to no range and is not touched.  A launch that does not match its table's
 * header touches nothing; a range whose x / hold entry is not 16-byte aligned, or pointer arrays made for another range count, are left
 * out likewise.
 * `flags`: AVMOE_OPT_CLIP, AVMOE_OPT_SKIP_NONFINITE, AVMOE_OPT_DECOUPLED_DECAY, AVMOE_OPT_LR_SCHEDULE (the averaging is implied: any
 * other flag is unknown).  hold == NULL is the step without a perturbation before it.
 * Errors (before any launch): everything avmoe_opt_adam_step_sam refuses (hold != NULL) or avmoe_opt_adam_step_ema refuses (hold == NULL);
 * AVMOE_ERR_BAD_ARG for NULL x, consts or block and for an r or lr_power that is not a finite number >= 0 (NaN included);
 * AVMOE_ERR_ALIGNMENT for a block that is not 16-byte or a pointer array that is not 8-byte aligned.                                  */
typedef struct avmoe_opt_sf_state {
  double weight_sum;          /* the sum of the steps' averaging weights w so far */
  float f_max;                /* the largest lr_factor so far (1 after the first applied step without a schedule) */
  float c;                    /* the last applied step's weight in the average, w / weight_sum */
  float d;                    /* 1 - c: the decay the average took (also state->ema_decay) */
  int32_t reserved[3];
} avmoe_opt_sf_state;

typedef struct avmoe_opt_sf {
  float r;                    /* >= 0: a step's weight grows like n^r (0: none) */
  float lr_power;             /* >= 0: ... and like f_max^lr_power (2: the paper's; 0: none) */
} avmoe_opt_sf;

int avmoe_opt_sf_step(const void* table, int32_t n_ranges, int64_t n_blocks, avmoe_opt_state* state, float beta1, float beta2, float eps,
                      float grad_scale, int32_t flags, void* stream, float* const* x /* DEVICE: the shadows, required */,
                      float* const* hold /* DEVICE, or NULL */, const avmoe_opt_sf* consts /* HOST */,
                      avmoe_opt_sf_state* block /* DEVICE, 16-byte aligned */);

/* Muon: orthogonalised momentum for small hidden matrices (Jordan et al. 2024; torch.optim.Muon's rule with the iteration in fp32; added
 * under ABI 11 like the blocks above; found by symbol).  A range that is listed as a matrix steps along the nearest semi-orthogonal
 * matrix of its momentum, found by Newton-Schulz iterations; every other range takes the unchanged Adam / AdamW update.  No flag and
 * no new word in the state block: avmoe_opt_muon_step is called IN PLACE of avmoe_opt_adam_step_ema / avmoe_opt_adam_step_sam, behind
 * the unchanged norm call of a step, on the same stream with the same grad_scale and betas.
 * The matrices are described once, on the host: avmoe_opt_muon_table_build checks a list of avmoe_opt_muon_mat {range, rows, cols} --
 * the range's elements read as a row-major rows x cols matrix -- and writes an image (header, the matrices in the caller's order, a
 * range -> matrix map) that the caller copies to DEVICE memory; that image is the `mats` of the two calls below.  The checks need the
 * host's copy, which is why they are made there and not by the calls that launch: a call that launches reads no device memory on the
 * host.  Callers sort the list by rows * cols descending, so that the long matrices start first.
 * With gscale = grad_scale * clip_coef, mu = momentum, lr = lr_r * lr_factor (under AVMOE_OPT_LR_SCHEDULE), w the parameter before the
 * step (with hold != NULL the held value), per element of a listed range, every operation rounded to fp32 in the order written,
 * contraction off:
 *     gr = fma(gscale, grad, wd * w)          AVMOE_OPT_DECOUPLED_DECAY: gr = grad * gscale
 *     m  = fma(mu, m, (1 - mu) * gr)          m is exp_avg; exp_avg_sq is neither read nor written; there is no bias correction
 *     u  = fma(mu, m, (1 - mu) * gr)          nesterov == 0: u = m
 * and per matrix, with d = min(rows, cols), Y the d x L view of u (Y = u for rows <= cols, Y = u^T otherwise):
 *     Y0 = Y * fp32(1 / (||u||_F + 1e-7))     ||u||_F: the sum of (double)u^2 in a fixed order, its double square root
 *     ns_steps times:  A = Y Y^T ;  B = b A + c (A A) ;  Y = a Y + B Y        (a, b, c) = (3.4445, -4.7750, 2.0315)
 *     O  = the rows x cols view of Y ;  s = fp32(0.2 * sqrt((double)max(rows, cols)))     (AVMOE_MUON_SCALE_MATCH_RMS_ADAMW)
 *                                       s = fp32(sqrt(max(1.0, (double)rows / cols)))     (AVMOE_MUON_SCALE_ORIGINAL)
 *     w  = w * (1 - lr * wd)                  (AVMOE_OPT_DECOUPLED_DECAY only)
 *     w  = w - (lr * s) * O                   under AVMOE_OPT_EMA then shadow = d shadow + (1 - d) w as avmoe_opt_adam_step_ema does
 * The products run on v_mfma_f32_16x16x4_f32 (exact fp32, fp32 accumulation in chains along the contraction index).  A zero u gives O = 0.
 * avmoe_opt_muon_step is TWO launches on `stream` whatever the number of ranges, without a host synchronisation and without a host
 * scalar that changes from step to step, so it replays from a captured graph:
 *   kk_opt_muon_update<DECOUPLED, SCHED, EMA, HOLD>   one block per table block.  A range that is not listed gets exactly the update of
 *       avmoe_opt_adam_step_ema / _sam (the same helpers of csrc/adam_elem.h, the same bits, the shadow included).  A listed range gets
 *       m, and u into work[range] -- one flat fp32 buffer per bucket in the bucket's layout, addressed by a DEVICE array of n_ranges
 *       float* under the rules of `shadows`; entries of ranges that are not listed are not read -- and the block's sum of (double)u^2
 *       into `workspace` (one double per table block, no initialisation needed).
 *   kk_opt_muon_ns<STEP>   one workgroup of 512 threads per matrix.  It adds its range's block sums in a fixed order (thread t blocks
 *       t, t + 512, ..., then a tree; no floating-point atomics: the same input gives the same bits), runs the iteration in place in
 *       the work buffer, and in the last pass applies decay and update to the parameter.  O stays in the work buffer.  A and B stay in
 *       LDS as d_pad x d_pad fp32 (d padded to a multiple of 16 by zero rows); Y is streamed from global memory in chunks along its
 *       long side, each chunk updated in place in LDS and the next iteration's Gram matrix accumulated from the chunk just produced
 *       (one pass over Y per iteration).  The launch ALWAYS asks for 160 KB of dynamic LDS, whatever d: a workgroup that issues
 *       v_mfma_f32_16x16x4_f32 must have its compute unit to itself (avmoe_moe_desc::shared_gpu above), and an all-reduce or a backbone
 *       kernel may be on the GPU during a step.
 * `report` (DEVICE, 16-byte aligned): a 16-byte header {n_mats, 0, 0, 0}, then ||u||_F of every matrix as fp32, in the list's order.
 * avmoe_opt_muon_bytes returns the bytes of the image, the workspace and the report (each a multiple of 16; 0 and an error string on a
 * negative count or more than 2^31 - 1 blocks) and their sum.
 * When state->skip is set nothing is written: moments, parameters, work buffers, workspace and report keep their values -- with
 * hold != NULL param = hold (every range, listed or not) and nothing else.  Gradients are only read; alignment padding belongs to no
 * range and is not touched, in the work buffers neither.  A launch that does not match its table's or its image's header touches
 * nothing; a listed range whose work / shadow / hold entry is not 16-byte aligned is left out by both launches.
 * avmoe_opt_muon_ns is the second launch alone, for tests: on matrices already in the work buffers it computes ||u||_F itself (thread t
 * elements t, t + 512, ..., then the tree), normalises and iterates; no table, no parameter, no report.
 * Errors of avmoe_opt_muon_table_build: AVMOE_ERR_BAD_ARG for NULL mats (with n_mats > 0) or image, negative counts, a range index
 * outside [0, n_ranges), rows or cols < 1, min(rows, cols) > 128, rows * cols != n of the range (where `ranges` is given), a range
 * named twice; AVMOE_ERR_WORKSPACE for an image that is too small.
 * Errors of the two calls (before any launch): everything avmoe_opt_adam_step_sam refuses (hold != NULL) or avmoe_opt_adam_step_ema
 * refuses (hold == NULL); AVMOE_ERR_BAD_ARG for NULL mats, work, consts, workspace or report, a negative n_mats, a momentum outside
 * [0, 1), nesterov not 0 / 1, ns_steps outside 1..16, an unknown scale; AVMOE_ERR_ALIGNMENT for an image or report that is not 16-byte
 * or a work pointer array or workspace that is not 8-byte aligned.
 * NOT covered by these calls: min(rows, cols) > 128 (avmoe_opt_muon_step_large below serves it), a matrix split across workgroups, an
 * iteration in bf16.                                                                                                                    */
#define AVMOE_MUON_MAX_DIM 128
#define AVMOE_MUON_SCALE_MATCH_RMS_ADAMW 0
#define AVMOE_MUON_SCALE_ORIGINAL 1

typedef struct avmoe_opt_muon_mat {
  int32_t range;              /* index into the optimizer's table */
  int32_t rows, cols;         /* rows * cols == n of the range */
  int32_t reserved;           /* 0 */
} avmoe_opt_muon_mat;

typedef struct avmoe_opt_muon {
  float momentum;             /* mu, in [0, 1) */
  int32_t nesterov;           /* 0 / 1 */
  int32_t ns_steps;           /* 1 .. 16 */
  int32_t scale;              /* AVMOE_MUON_SCALE_* */
} avmoe_opt_muon;

typedef struct avmoe_opt_muon_layout { size_t table_bytes, workspace_bytes, report_bytes; } avmoe_opt_muon_layout;

size_t avmoe_opt_muon_bytes(int32_t n_ranges, int64_t n_blocks, int32_t n_mats, avmoe_opt_muon_layout* layout /* HOST, or NULL */);
int avmoe_opt_muon_table_build(const avmoe_opt_range* ranges /* HOST, or NULL */, int32_t n_ranges, const avmoe_opt_muon_mat* mats /* HOST */,
                               int32_t n_mats, void* image /* HOST */, size_t image_bytes);
int avmoe_opt_muon_step(const void* table, int32_t n_ranges, int64_t n_blocks, const avmoe_opt_state* state, float beta1, float beta2,
                        float eps, float grad_scale, int32_t flags, void* stream, float* const* shadows /* DEVICE, or NULL without AVMOE_OPT_EMA */,
                        float* const* hold /* DEVICE, or NULL */, const void* mats /* DEVICE: the image */, int32_t n_mats,
                        float* const* work /* DEVICE */, const avmoe_opt_muon* consts /* HOST */, double* workspace /* DEVICE */,
                        void* report /* DEVICE, 16-byte aligned */);
int avmoe_opt_muon_ns(const void* mats /* DEVICE: the image */, int32_t n_mats, float* const* work /* DEVICE */, int32_t ns_steps, void* stream);

/* Muon for the LARGE matrices: a short side above AVMOE_MUON_MAX_DIM (or a numel the caller keeps from the one-workgroup kernel), up to
 * AVMOE_MUON_LARGE_MAX_DIM (added under ABI 11; found by symbol; csrc/opt_muon_large.hip).  The rule is EXACTLY the one stated above for
 * a listed range -- gr, m, u per element, ||u||_F from the block sums in double in a fixed order, Y0, the iteration, the scale with
 * max(rows, cols), decay, update, shadow -- only the arithmetic of the three products differs: they run on the tiled engine
 * (csrc/gemm.hip, launch_gemm) with fp32 operands in THREE-PLANE form (avmoe_gemm's fp32_planes = 3: every value as three bf16 planes,
 * 5.8e-9 relative per product, fp32 accumulation).  That form and not v_mfma_f32_16x16x4_f32 because the engine's exact-fp32 tiles
 * would need their compute unit to themselves (avmoe_moe_desc::shared_gpu) and the engine makes no whole-CU LDS request; its error
 * is a fortieth of the fp32 rounding of the sums themselves.  A d x d Gram matrix at d = 768 is 2.4 MB: nothing of this path is
 * LDS-resident.
 * avmoe_opt_muon_large_table_build (HOST) checks the list -- range index, rows, cols >= 1, min(rows, cols) <= 2048, rows * cols == n of
 * the range (where `ranges` is given), no range named twice, in this list or in `small` (the list the caller gave
 * avmoe_opt_muon_table_build, or NULL) -- orients every matrix short side first (d = min(rows, cols), L = the other side) and groups
 * the matrices into CLASSES of equal (d, L), in the order of first appearance.  The image: header, the matrices in the caller's order
 * (with their class and slot), the classes (with their offsets into the workspace), a range -> matrix map.  The caller keeps the HOST
 * image and copies it to DEVICE memory: the calls below take both, because the engine's launches are shaped on the host from the
 * classes and a call that launches reads no device memory on the host.  avmoe_opt_muon_large_bytes returns image, workspace and
 * report bytes (each a multiple of 16) and the class count; the workspace depends on the shapes, so the query takes the list.
 * The workspace (DEVICE, 16-byte aligned, no initialisation needed) holds two constant vectors (a and b, 2048 floats each), the block
 * sums of avmoe_opt_muon_ns_large, and per class two staging buffers Y (count x d4 x L4 floats: d4, L4 = d, L rounded up to 4, the
 * padding rows and columns zero, which the iteration keeps zero, so the padding is exact), A and B (count x d x d4) and the slabs of a
 * split-K Gram product.  Equal-shaped matrices of different sites lie at unrelated offsets in the flat buckets: the staging area is
 * what gives the engine a uniform batch stride.
 * avmoe_opt_muon_step_large is avmoe_opt_muon_step (same arguments, same checks, same bits for every range that is not large) plus:
 *   1  kk_opt_muon_update, which treats the ranges of the large map as listed too (m, u into work[range], the block's sum of u^2)
 *   2  kk_opt_muon_ns<STEP> over the small matrices (when n_mats > 0)
 *   3  kk_opt_muon_large_pack<STEP>: one launch for all large matrices.  Every workgroup of a matrix adds the matrix's block sums in
 *      the same fixed order (thread t blocks t, t + 256, ..., then a tree; no floating-point atomics), forms inv = fp32(1 / (||u||_F +
 *      1e-7)), writes the norm to the report and Y0 = Y * inv into the first staging buffer (32 x 32 tiles through LDS, transposed on
 *      the way for rows > cols), zeroes the padding of both staging buffers and of A and B, and writes the constant vectors
 *   4  per class and iteration THREE engine launches, batched over the class:  A = Y Y^T (both operands K-major, M = N = d, K = L;
 *      split-K with slabs from the workspace where L is long and the tiles are few: one reduce launch more);  B = c (A A^T) + b A
 *      (A is symmetric; the b A term is the engine's row_scale * D epilogue with the constant vector b);  Y' = B Y + a Y into the
 *      other staging buffer (Y the MN-major operand and D, row_scale the constant vector a)
 *   5  kk_opt_muon_large_apply<DECOUPLED, SCHED, EMA, HOLD>: one launch for all large matrices.  It reads O from staging (transposing
 *      back), writes O into work[range], decay and update on the parameter (read from hold[range] with hold != NULL) with muon_next of
 *      csrc/adam_elem.h, and the shadow with ema_next
 * -- 2 + 1 + 3 * ns_steps * classes (+ the engine's split-K reduces) + 1 launches (one less without small matrices), without an
 * allocation, a host synchronisation or a host scalar that changes per step: it replays from a captured graph.  When state->skip is
 * set launches 3 and 5 write nothing (launch 1 has written param = hold under hold != NULL, for every range); the engine launches of
 * a skipped step run on the staging buffers and are harmless.  `large_report`: {n_large, 0, 0, 0}, then ||u||_F per large matrix as
 * fp32, in the list's order.  A launch that does not match its image or table, or a matrix whose work / hold / shadow entry is not
 * 16-byte aligned, touches nothing of that matrix.
 * avmoe_opt_muon_ns_large is the iteration alone, for tests: on matrices already in the work buffers it takes the block sums itself
 * (one launch more, sums in the workspace), packs, iterates and writes O back into the work buffers; no table, no parameter, no report.
 * Errors of avmoe_opt_muon_large_table_build: AVMOE_ERR_BAD_ARG for NULL mats (with n_mats > 0) or image, negative counts, a range
 * index outside [0, n_ranges), rows or cols < 1, min(rows, cols) > 2048, rows * cols != n of the range, a range named twice (either
 * list); AVMOE_ERR_WORKSPACE for an image that is too small.  avmoe_opt_muon_table_build keeps refusing a short side above 128.
 * Errors of the two launching calls (before any launch): everything avmoe_opt_muon_step refuses; AVMOE_ERR_BAD_ARG for a NULL large
 * image (either copy), workspace or report, a negative n_large, a HOST image whose header does not say n_large matrices and n_ranges
 * ranges; AVMOE_ERR_ALIGNMENT for a large image, workspace or report that is not 16-byte aligned; the engine's own status where it
 * refuses a product.
 * NOT covered: min(rows, cols) > 2048, an iteration in bf16.                                                                            */
#define AVMOE_MUON_LARGE_MAX_DIM 2048

typedef struct avmoe_opt_muon_large_layout { size_t table_bytes, workspace_bytes, report_bytes; int32_t n_classes, reserved; } avmoe_opt_muon_large_layout;

/* one class of an image, as avmoe_opt_muon_large_classes reports it (tests, tools) */
typedef struct avmoe_opt_muon_class { int32_t d, L, count, ksplit; } avmoe_opt_muon_class;

size_t avmoe_opt_muon_large_bytes(int32_t n_ranges, const avmoe_opt_muon_mat* mats /* HOST */, int32_t n_mats,
                                  avmoe_opt_muon_large_layout* layout /* HOST, or NULL */);
int avmoe_opt_muon_large_table_build(const avmoe_opt_range* ranges /* HOST, or NULL */, int32_t n_ranges, const avmoe_opt_muon_mat* mats /* HOST */,
                                     int32_t n_mats, const avmoe_opt_muon_mat* small /* HOST, or NULL */, int32_t n_small, void* image /* HOST */,
                                     size_t image_bytes);
/* the classes of a HOST image into out[0 .. cap) and the class of every matrix into cls_of[0 .. n_mats) (either may be NULL); returns
 * the class count, or a negative status for an image that is not one */
int avmoe_opt_muon_large_classes(const void* image /* HOST */, avmoe_opt_muon_class* out, int32_t cap, int32_t* cls_of);
int avmoe_opt_muon_step_large(const void* table, int32_t n_ranges, int64_t n_blocks, const avmoe_opt_state* state, float beta1, float beta2,
                              float eps, float grad_scale, int32_t flags, void* stream, float* const* shadows /* DEVICE, or NULL without AVMOE_OPT_EMA */,
                              float* const* hold /* DEVICE, or NULL */, const void* mats /* DEVICE: the small image */, int32_t n_mats,
                              float* const* work /* DEVICE */, const avmoe_opt_muon* consts /* HOST */, double* workspace /* DEVICE */,
                              void* report /* DEVICE, 16-byte aligned */, const void* large /* DEVICE: the large image */,
                              const void* large_host /* HOST: the same image */, int32_t n_large, void* large_workspace /* DEVICE, 16-byte aligned */,
                              void* large_report /* DEVICE, 16-byte aligned */);
int avmoe_opt_muon_ns_large(const void* large /* DEVICE: the large image */, const void* large_host /* HOST: the same image */, int32_t n_large,
                            float* const* work /* DEVICE */, int32_t ns_steps, void* large_workspace /* DEVICE, 16-byte aligned */, void* stream);

/* ---- test hooks (ABI 11; process-wide; tests and bench.py's parity leg only) ---------------------------
 * The streaming kernels (csrc/dpost_pair.hip, tok_pair2.hip, hop1_stream.hip) serve sites from 32 768 tokens on; below that the
 * tiled engine is faster.  force_mask lifts those thresholds so that a test can run the benchmarked kernels on shapes its oracle
 * finishes in seconds: bit 1 = tok_pair2, 2 = dpost_pair (from 4096 tokens), 4 = the hop-1 products against Y, 8 = the streaming form of the
 * bottleneck-space kernels (csrc/tile_stream.hip); bit 16 switches that form OFF (the A/B against csrc/tile_fast.hip).  nxn_chunk > 0:
 * frames per chunk of the AVVP N x N block (0 = the library's own choice).  Returns the previous force_mask.  The initial values
 * come from the environment variables AVMOE_TOKPAIR2_FORCE / AVMOE_DPAIR_FORCE / AVMOE_HOP1S_FORCE / AVMOE_KFS_FORCE / AVMOE_KFS_OFF / AVMOE_NXN_CHUNK, read once
 * when the library is first asked -- no kernel choice depends on the environment at call time.                                  */
enum { AVMOE_HOOK_TOKPAIR2_FORCE = 1, AVMOE_HOOK_DPAIR_FORCE = 2, AVMOE_HOOK_HOP1S_FORCE = 4, AVMOE_HOOK_KFS_FORCE = 8, AVMOE_HOOK_KFS_OFF = 16 };
uint32_t avmoe_test_hooks(uint32_t force_mask, int32_t nxn_chunk);

/* avmoe_nxn_strip (added under ABI 11; AVMOE_ABI_VERSION unchanged, a binding finds it by symbol; tests only) -- ONE strip kernel of the
 * AVVP N x N block (csrc/nxn_att.hip) on raw operands, so that each can be checked alone (tests/test_nxn_strips_fp64_gpu.py).  bf16
 * operands, att[i][j] = exp(X_i . X_j - lse_i) per frame, rows of att / dS are N wide.  No site call goes through it.
 *   X, dxr, out (XR / Y / DXQ / DXK): (frames, N, C) bf16;  lse, rowdot: (frames, N) fp32;  att_in, out (ATT / ATT_FROM_LSE / ATT_BWD): (frames, N, N) bf16
 *   STATS         lse = row log-sum-exp of X X^T                              (writes lse)
 *   ATT           the same, then out = att                                    (writes lse, out)
 *   ATT_FROM_LSE  out = att from the given lse                                (reads lse)
 *   XR            out = att^T X                                               (reads lse)
 *   Y             y = att dxr: rowdot = X . y, out += y                       (reads lse, writes rowdot, read-modify-writes out)
 *   DXQ / DXK     out += dS X / dS^T X, dS = att * (X dxr^T - rowdot)         (reads lse, rowdot, read-modify-writes out)
 *   ATT_BWD       out = dS = att_in * (X dxr^T - rowdot)                      (reads rowdot, att_in)
 * It adds no arithmetic: AVMOE_ERR_BAD_ARG for an unknown op or a NULL pointer among those the op uses (unused ones may be NULL), then the
 * kernel's own wrapper and its status -- AVMOE_ERR_UNSUPPORTED unless C is 96 or 192 and N a positive multiple of 128; frames <= 0 is
 * AVMOE_OK without a launch.                                                                                                    */
enum { AVMOE_NXN_STATS = 0, AVMOE_NXN_ATT = 1, AVMOE_NXN_ATT_FROM_LSE = 2, AVMOE_NXN_XR = 3, AVMOE_NXN_Y = 4, AVMOE_NXN_DXQ = 5,
       AVMOE_NXN_DXK = 6, AVMOE_NXN_ATT_BWD = 7 };
int avmoe_nxn_strip(int32_t op, const void* X, const void* dxr, int32_t frames, int32_t N, int32_t C, float* lse, float* rowdot, void* out,
                    const void* att_in, void* stream);

/* avmoe_gemm_form / avmoe_gemm_row_lse (added under ABI 11; AVMOE_ABI_VERSION unchanged, a binding finds them by symbol; tests only) -- the
 * forms of the tiled engine (csrc/gemm.hip, launch_gemm) that avmoe_gemm_desc has no field for, on raw operands, so that each can be checked
 * alone against fp64 of its own operands (tests/test_engine_forms_fp64_gpu.py).  No site call goes through either.  They add no arithmetic:
 * avmoe_gemm_form fills the engine's descriptor (csrc/gemm.h: GemmArgs) and calls launch_gemm, whose refusals and status codes come back
 * unchanged (AVMOE_ERR_BAD_ARG of its own only for a NULL desc / A / B array).
 *   base            the first K segment and everything avmoe_gemm takes (A[0], B[0] are its operands)
 *   seg[0 .. 2]     the second, third and fourth K segment: K, both layouts, leading dimensions and the two batch strides of each; segment
 *                   i + 1 is present when A[i + 1] / B[i + 1] are set (NULL otherwise), and the engine wants the one before it present
 *   nb3, sA3 .. sC3 the third batch level: batch = nb1 * nb3 * nb2, b = (b1 * nb3 + b3) * nb2 + b2 (plain products only)
 *   epi             AVMOE_GEMM_EPI_*: ROWSTATS writes row_part[((b * M + i) * tiles + t) * 2 + {0, 1}] = (max, sum of exp(v - max)) of column tile t
 *                   (tiles = ceil(N / 128)) of v = alpha * (A B^T) and leaves C alone; EXP stores exp(v - row_lse[b * M + i]); MULSUB stores
 *                   D * (v - row_lse[b * M + i]) (D without row_scale)
 *   keep_slabs      split-K (base.ksplit > 1) whose fp32 partial sums stay in `workspace` as [ksplit][batch][M][N]; C is not written
 * avmoe_gemm_row_lse: lse[r] = log sum_j exp(v[r][j]) from the (max, sum) parts of ROWSTATS, rows = batch * M (gemm_row_lse; rows <= 0:
 * AVMOE_OK without a launch; AVMOE_ERR_BAD_ARG for a NULL pointer or tiles <= 0).                                                         */
enum { AVMOE_GEMM_EPI_NONE = 0, AVMOE_GEMM_EPI_ROWSTATS = 1, AVMOE_GEMM_EPI_EXP = 2, AVMOE_GEMM_EPI_MULSUB = 3 };
typedef struct avmoe_gemm_form_seg {
  int32_t K, a_layout, b_layout, reserved;
  int64_t lda, ldb, sA1, sA2, sB1, sB2;
} avmoe_gemm_form_seg;
typedef struct avmoe_gemm_form_desc {
  avmoe_gemm_desc base;
  int32_t nb3, epi, keep_slabs, reserved;
  int64_t sA3, sB3, sC3;
  avmoe_gemm_form_seg seg[3];
} avmoe_gemm_form_desc;
int avmoe_gemm_form(const avmoe_gemm_form_desc* desc, const void* const* A /* [4] */, const void* const* B /* [4] */, void* C,
                    const float* row_scale, const void* D, void* workspace, float* row_part, const float* row_lse, void* stream);
int avmoe_gemm_row_lse(const float* row_part, int64_t rows, int32_t tiles, float* lse, void* stream);

/* ---- optional per-launch timing (HIP events on the launch stream; off by default; process-wide) --------
 * avmoe_prof_report writes a JSON array of {"name","calls","total_ms","alg_bytes","flops"} per kernel family
 * into buf (NUL-terminated, truncated to cap) and returns the full length.  Used by bench.py for the roofline. */
void avmoe_prof_enable(int on);
void avmoe_prof_reset(void);
size_t avmoe_prof_report(char* buf, size_t cap);

#ifdef __cplusplus
}
#endif
#endif /* AVMOE_H_ */
