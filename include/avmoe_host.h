/* avmoe_host.h -- the adapter-site ABI of avmoe.h evaluated on the HOST (CPU, fp32, host pointers).
 *
 * "a host (CPU, C++) implementation of the same ABI is the restatement used for CPU timing and no-GPU CI".  Same
 * descriptor (avmoe_moe_desc), same parameter structs (avmoe_moe_ptrs: one pointer per reference state_dict entry), same token-major
 * tensors and the same results as avmoe_moe_forward / avmoe_moe_backward -- but the reference's formulation evaluated directly
 * (net_trans_v3.py:377-487 op by op, hand-written reverse pass), no workspaces, no streams.  Library: avmoe_amd/lib/libavmoe_host.so
 * (avmoe_amd/csrc/host_moe.cpp, built with g++ by avmoe_amd.build.build_host()).  TEST / CI infrastructure: the product path
 * (libavmoe_hip.so) never loads it and has no CPU fallback.
 *
 * Served: AVE / AVQA / AVVP (N x N block) / AVS (self_attention_version "v2" and, since round 6, "v1": MultiheadAttention across the frames with
 * the caller's dropout multipliers, avmoe_expert_ptrs::sa_keep), training and eval BatchNorm, every flag, logit noise, load-balancing loss.
 * AVMOE_ERR_UNSUPPORTED: dtype != AVMOE_F32.                                                                                             */
#ifndef AVMOE_HOST_H
#define AVMOE_HOST_H
#include "avmoe.h"

#ifdef __cplusplus
extern "C" {
#endif

const char* avmoe_host_last_error(void);
size_t avmoe_host_moe_saved_bytes(const avmoe_moe_desc* desc);       /* the backward recomputes the forward: `saved` may be NULL */

/* as avmoe_moe_forward: out (S, N, C), probs (S, E) or NULL, idx (S) int64 or NULL, lb (1 float) or NULL; in training mode the
 * BatchNorm running statistics / num_batches_tracked in `params` advance.  bn_momentum < 0: the cumulative average of avmoe.h, factor
 * 1.0f / (float)(counter + 1) read before the counter's own bump; a NULL bn1_nbt / bn2_nbt is then AVMOE_ERR_BAD_ARG, named in
 * avmoe_host_last_error, before anything is written.                                                                                  */
int avmoe_host_moe_forward(const avmoe_moe_desc* desc, const float* X, const float* Y, const avmoe_moe_ptrs* params, const float* noise,
                           float* out, float* probs, int64_t* idx, float* lb, void* saved);

/* as avmoe_moe_backward: gradients of <out, dOut> + (*lb_grad) * lb; every non-NULL pointer in `grads` is overwritten, dX / dY are
 * overwritten.  `noise`: the same logit noise the forward saw (the forward is recomputed; running statistics do not advance again).
 * lb_grad: HOST pointer or NULL.                                                                                                       */
int avmoe_host_moe_backward(const avmoe_moe_desc* desc, const float* X, const float* Y, const avmoe_moe_ptrs* params, const float* noise,
                            const float* dOut, const float* lb_grad, void* saved, float* dX, float* dY, const avmoe_moe_ptrs* grads);

/* as avmoe_moe_backward_ex: gradients of <out, dOut> + <probs, dprobs> + (*lb_grad) * lb.  dOut == NULL means dOut = 0 (the checker
 * evaluates the whole reverse pass; it has no router-only path), dprobs: (S, E) HOST pointer or NULL.                                  */
int avmoe_host_moe_backward_ex(const avmoe_moe_desc* desc, const float* X, const float* Y, const avmoe_moe_ptrs* params, const float* noise,
                               const float* dOut, const float* dprobs, const float* lb_grad, void* saved, float* dX, float* dY,
                               const avmoe_moe_ptrs* grads);

/* as avmoe_moe_forward_topk: top-k gating of the mixture (top_k in [1, E]; top_k == E is the dense site).                         */
int avmoe_host_moe_forward_topk(const avmoe_moe_desc* desc, const float* X, const float* Y, const avmoe_moe_ptrs* params, const float* noise,
                                int32_t top_k, int32_t renorm, float* out, float* probs, int64_t* idx, float* lb, void* saved);

/* avmoe_host_moe_backward_ex of a top-k forward: the same top_k / renorm as the forward (it is recomputed).                          */
int avmoe_host_moe_backward_topk(const avmoe_moe_desc* desc, const float* X, const float* Y, const avmoe_moe_ptrs* params, const float* noise,
                                 const float* dOut, const float* dprobs, const float* lb_grad, void* saved, float* dX, float* dY,
                                 const avmoe_moe_ptrs* grads, int32_t top_k, int32_t renorm);

/* as avmoe_moe_forward_aux: the router auxiliary losses aux = [z, balance] and load (E) beside the forward's outputs (top_k 0: dense;
 * aux NULL: avmoe_host_moe_forward / _forward_topk).                                                                              */
int avmoe_host_moe_forward_aux(const avmoe_moe_desc* desc, const float* X, const float* Y, const avmoe_moe_ptrs* params, const float* noise,
                               int32_t top_k, int32_t renorm, float* out, float* probs, int64_t* idx, float* lb, float* aux, float* load,
                               void* saved);

/* as avmoe_moe_backward_aux: avmoe_host_moe_backward_ex / _topk (top_k 0: dense) plus aux_grad = [g_z, g_balance] or NULL.           */
int avmoe_host_moe_backward_aux(const avmoe_moe_desc* desc, const float* X, const float* Y, const avmoe_moe_ptrs* params, const float* noise,
                                const float* dOut, const float* dprobs, const float* lb_grad, const float* aux_grad, void* saved,
                                float* dX, float* dY, const avmoe_moe_ptrs* grads, int32_t top_k, int32_t renorm);

/* as avmoe_moe_forward_reg: avmoe_host_moe_forward_aux plus mix_scale, the (S, E) multiplier on the mixture weights behind top-k
 * (stochastic depth / expert dropout), HOST pointer or NULL (= avmoe_host_moe_forward_aux).  The multiplier is an input: the host
 * side has no generator.  probs / idx / lb / aux / load and the BatchNorm statistics do not depend on it.                           */
int avmoe_host_moe_forward_reg(const avmoe_moe_desc* desc, const float* X, const float* Y, const avmoe_moe_ptrs* params, const float* noise,
                               int32_t top_k, int32_t renorm, const float* mix_scale, float* out, float* probs, int64_t* idx, float* lb,
                               float* aux, float* load, void* saved);

/* as avmoe_moe_backward_reg: avmoe_host_moe_backward_aux with the forward's mix_scale (it carries no gradient).                     */
int avmoe_host_moe_backward_reg(const avmoe_moe_desc* desc, const float* X, const float* Y, const avmoe_moe_ptrs* params, const float* noise,
                                const float* dOut, const float* dprobs, const float* lb_grad, const float* aux_grad, const float* mix_scale,
                                void* saved, float* dX, float* dY, const avmoe_moe_ptrs* grads, int32_t top_k, int32_t renorm);

/* as avmoe_moe_forward_bias: avmoe_host_moe_forward_reg plus the selection bias of aux-loss-free balancing.  select_bias: (E) HOST
 * pointer or NULL; the k experts are chosen on p + b (one fp32 addition, the tie rule of the top-k mixture), the weights are formed
 * from the unbiased p, and load / balance are the actual selection's.  select_count: (E) HOST pointer or NULL, ADDED to: the number of
 * frames that selected each expert.  select_bias with top_k == 0 or E: AVMOE_ERR_BAD_ARG.  Both NULL: avmoe_host_moe_forward_reg.     */
int avmoe_host_moe_forward_bias(const avmoe_moe_desc* desc, const float* X, const float* Y, const avmoe_moe_ptrs* params, const float* noise,
                                int32_t top_k, int32_t renorm, const float* mix_scale, const float* select_bias, float* select_count,
                                float* out, float* probs, int64_t* idx, float* lb, float* aux, float* load, void* saved);

/* avmoe_host_moe_backward_reg of such a forward.  The host backward recomputes the forward, so it takes the bias the forward saw as an
 * argument (the device library reads it from `saved`); the bias and the selection carry no gradient.                                 */
int avmoe_host_moe_backward_bias(const avmoe_moe_desc* desc, const float* X, const float* Y, const avmoe_moe_ptrs* params, const float* noise,
                                 const float* dOut, const float* dprobs, const float* lb_grad, const float* aux_grad, const float* mix_scale,
                                 const float* select_bias, void* saved, float* dX, float* dY, const avmoe_moe_ptrs* grads, int32_t top_k,
                                 int32_t renorm);

#ifdef __cplusplus
}
#endif
#endif
