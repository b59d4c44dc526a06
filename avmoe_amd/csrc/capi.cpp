// C ABI (include/avmoe.h) -> internal C++ entry points.  No exceptions cross this boundary.
#include "../../include/avmoe.h"
#include "common.h"
#include "gemm.h"
#include "moe_run.h"
#include "prof.h"

using namespace avmoe;

static GemmArgs to_args(const avmoe_gemm_desc* d) {
  GemmArgs a;
  a.M = d->M; a.N = d->N; a.K = d->K; a.nb1 = d->nb1; a.nb2 = d->nb2;
  a.dtype = d->dtype; a.out_dtype = d->out_dtype; a.a_layout = d->a_layout; a.b_layout = d->b_layout;
  a.accumulate = d->accumulate; a.ksplit = d->ksplit; a.tile = d->tile; a.split3 = d->dtype == AVMOE_F32 ? (d->fp32_planes == 2 ? 2 : (d->fp32_planes != 0 ? 1 : 0)) : 0; a.alpha = d->alpha;
  a.lda = d->lda; a.ldb = d->ldb; a.sA1 = d->sA1; a.sA2 = d->sA2; a.sB1 = d->sB1; a.sB2 = d->sB2;
  a.sCi = d->sCi; a.sCj = d->sCj; a.sC1 = d->sC1; a.sC2 = d->sC2;
  a.sRS1 = d->sRS1; a.sRS2 = d->sRS2; a.sDi = d->sDi; a.sD1 = d->sD1; a.sD2 = d->sD2;
  return a;
}

extern "C" {

int avmoe_abi_version(void) { return AVMOE_ABI_VERSION; }
int avmoe_bn_cumulative_supported(void) { return 1; }
const char* avmoe_last_error(void) { return last_error(); }

size_t avmoe_gemm_workspace_bytes(const avmoe_gemm_desc* desc) {
  if (!desc) return 0;
  return gemm_slab_bytes(to_args(desc));
}

int avmoe_gemm(const avmoe_gemm_desc* desc, const void* A, const void* B, void* C, const float* row_scale,
               const void* D, void* workspace, void* stream) {
  if (!desc) { set_last_error("avmoe_gemm: null desc"); return ERR_BAD_ARG; }
  GemmArgs a = to_args(desc);
  a.A = A; a.B = B; a.C = C; a.row_scale = row_scale; a.D = D; a.slabs = (float*)workspace;
  return launch_gemm(a, (hipStream_t)stream);
}


size_t avmoe_moe_saved_bytes(const avmoe_moe_desc* desc) {
  Plan pl;
  return make_plan(desc, &pl) == OK ? pl.saved_bytes : 0;
}
size_t avmoe_moe_scratch_bytes(const avmoe_moe_desc* desc) {
  Plan pl;
  return make_plan(desc, &pl) == OK ? pl.scratch_bytes : 0;
}

}  // extern "C"

// The ranges of a site call's routing, checked once before anything is launched (`fn`: the entry point's name in the error strings; k_min: the smallest top_k it takes)
static int route_check(const char* fn, int k_min, const Dims& d, const RouteCall& r) {
  const int k = r.top_k;
  if (k < k_min || k > d.E) { set_last_error("%s: top_k %d not in [%d, %d]", fn, k, k_min, d.E); return ERR_BAD_ARG; }
  if (r.select_bias && (k == 0 || k == d.E)) {           // a dense mixture has no selection
    set_last_error("%s: select_bias needs top-k gating, 0 < top_k < E (top_k %d, E %d)", fn, k, d.E); return ERR_BAD_ARG;
  }
  const auto *ch = std::get_if<RouterChoice>(&r.stage); const auto *sk = std::get_if<RouterSinkhorn>(&r.stage);
  const auto *cap = std::get_if<RouterCapacity>(&r.stage);
  if ((sk || cap) && (k < 1 || k >= d.E)) { set_last_error("%s: top_k %d not in [1, %d)", fn, k, d.E); return ERR_BAD_ARG; }      // (both act on a top-k selection; E >= 2 follows)
  const int c = ch ? ch->capacity : cap ? cap->capacity : 1;      // (no stage with a capacity: nothing to refuse)
  if (c < 1 || c > d.S) { set_last_error("%s: capacity %d not in [1, %d]", fn, c, d.S); return ERR_BAD_ARG; }
  if (sk && (sk->iters < 1 || sk->iters > 64)) { set_last_error("%s: iters %d not in [1, 64]", fn, sk->iters); return ERR_BAD_ARG; }
  if (cap && cap->policy != 0 && cap->policy != 1) { set_last_error("%s: policy %d not in {0, 1}", fn, cap->policy); return ERR_BAD_ARG; }
  if (cap && !cap->cap_scale) { set_last_error("%s: cap_scale is NULL (the backward's multiplier is required)", fn); return ERR_BAD_ARG; }
  if (const auto* tp = std::get_if<RouterTopP>(&r.stage)) AVMOE_TRY(top_p_check(fn, d.E, tp->p, tp->k_min, tp->k_max));      // (E >= 2, P in (0, 1], 1 <= k_min <= k_max <= E)
  return OK;
}

// The one forward behind avmoe_moe_forward / _topk / _aux / _reg / _bias / _choice / _sinkhorn / _capacity / _top_p
static int site_forward(const char* fn, int k_min, const avmoe_moe_desc* desc, const void* X, const void* Y, const avmoe_moe_ptrs* params, void* out,
                        const RouteCall& route, void* saved, void* scratch, void* stream) {
  Plan pl;
  AVMOE_TRY(make_plan(desc, &pl));
  if (!X || !Y || !params || !out || !saved || !scratch) { set_last_error("%s: null pointer", fn); return ERR_BAD_ARG; }
  AVMOE_TRY(route_check(fn, k_min, pl.d, route));
  RouteCall r = route;
  if (r.top_k == pl.d.E) r.top_k = 0;                    // 0 and E: the dense mixture, whatever renorm says (the load then counts every frame's first expert)
  return moe_forward(pl, X, Y, *params, out, r, (char*)saved, (char*)scratch, (hipStream_t)stream);
}

// The one backward behind avmoe_moe_backward / _part / _ex / _aux / _reg (null_dout: dOut == NULL asks for the router-only backward, else it is refused)
static int site_backward(const char* fn, bool null_dout, const avmoe_moe_desc* desc, const void* X, const void* Y, const avmoe_moe_ptrs* params,
                         const void* dOut, const float* dprobs, const float* lb_grad, const float* aux_grad, const float* mix_scale, void* saved, void* scratch,
                         void* dX, void* dY, const avmoe_moe_ptrs* grads, int32_t parts, void* stream) {
  Plan pl;
  AVMOE_TRY(make_plan(desc, &pl));
  if (!X || !Y || !params || (!dOut && !null_dout) || !saved || !scratch || !dX || !dY || !grads || parts < 0 || parts > 127) {
    set_last_error("%s: null pointer or parts not in 0..127", fn); return ERR_BAD_ARG;
  }
  if ((parts & 4) && (parts & 24)) {        // 4 IS sections 8 + 16: asking for both would run the hop-1 chain twice into the same accumulators
    set_last_error("%s: parts %d combines section 4 with its halves 8 / 16", fn, parts); return ERR_BAD_ARG;
  }
  if (!dOut) {                              // out gets no gradient: the router-only backward, whole (it has no sections)
    if (parts != 0 && parts != 7) { set_last_error("%s: dOut == NULL serves parts 0 / 7 only, not %d", fn, parts); return ERR_UNSUPPORTED; }
    return moe_backward_router_only(pl, Y, *params, dprobs, lb_grad, (char*)saved, (char*)scratch, dX, dY, *grads, (hipStream_t)stream, aux_grad);
  }
  return moe_backward(pl, X, Y, *params, dOut, lb_grad, (char*)saved, (char*)scratch, dX, dY, *grads, (hipStream_t)stream, parts, dprobs,
                      aux_grad, mix_scale);
}

// the routing fields every site entry point has
static RouteCall route_of(const float* noise, int32_t top_k, int32_t renorm, float* probs, int64_t* idx, float* lb) {
  RouteCall r;
  r.noise = noise; r.top_k = top_k; r.renorm = renorm != 0; r.probs_out = probs; r.idx_out = idx; r.lb_out = lb;
  return r;
}

extern "C" {

int avmoe_moe_forward(const avmoe_moe_desc* desc, const void* X, const void* Y, const avmoe_moe_ptrs* params,
                      const float* noise, void* out, float* probs, int64_t* idx, float* lb, void* saved, void* scratch,
                      void* stream) {
  return site_forward("avmoe_moe_forward", 0, desc, X, Y, params, out, route_of(noise, 0, 1, probs, idx, lb), saved, scratch, stream);
}

int avmoe_moe_forward_topk(const avmoe_moe_desc* desc, const void* X, const void* Y, const avmoe_moe_ptrs* params, const float* noise,
                           int32_t top_k, int32_t renorm, void* out, float* probs, int64_t* idx, float* lb, void* saved, void* scratch,
                           void* stream) {
  return site_forward("avmoe_moe_forward_topk", 1, desc, X, Y, params, out, route_of(noise, top_k, renorm, probs, idx, lb), saved, scratch, stream);
}

int avmoe_moe_forward_aux(const avmoe_moe_desc* desc, const void* X, const void* Y, const avmoe_moe_ptrs* params, const float* noise,
                          int32_t top_k, int32_t renorm, void* out, float* probs, int64_t* idx, float* lb, float* aux, float* load,
                          void* saved, void* scratch, void* stream) {
  RouteCall r = route_of(noise, top_k, renorm, probs, idx, lb); r.aux_out = aux; r.load_out = load;
  return site_forward("avmoe_moe_forward_aux", 0, desc, X, Y, params, out, r, saved, scratch, stream);
}

int avmoe_moe_forward_reg(const avmoe_moe_desc* desc, const void* X, const void* Y, const avmoe_moe_ptrs* params, const float* noise,
                          int32_t top_k, int32_t renorm, const float* mix_scale, void* out, float* probs, int64_t* idx, float* lb,
                          float* aux, float* load, void* saved, void* scratch, void* stream) {
  RouteCall r = route_of(noise, top_k, renorm, probs, idx, lb); r.aux_out = aux; r.load_out = load; r.mix_scale = mix_scale;
  return site_forward("avmoe_moe_forward_reg", 0, desc, X, Y, params, out, r, saved, scratch, stream);
}

int avmoe_moe_forward_bias(const avmoe_moe_desc* desc, const void* X, const void* Y, const avmoe_moe_ptrs* params, const float* noise,
                           int32_t top_k, int32_t renorm, const float* mix_scale, const float* select_bias, float* select_count, void* out,
                           float* probs, int64_t* idx, float* lb, float* aux, float* load, void* saved, void* scratch, void* stream) {
  RouteCall r = route_of(noise, top_k, renorm, probs, idx, lb);
  r.aux_out = aux; r.load_out = load; r.mix_scale = mix_scale; r.select_bias = select_bias; r.select_count = select_count;
  return site_forward("avmoe_moe_forward_bias", 0, desc, X, Y, params, out, r, saved, scratch, stream);
}

int avmoe_moe_forward_choice(const avmoe_moe_desc* desc, const void* X, const void* Y, const avmoe_moe_ptrs* params, const float* noise,
                             int32_t capacity, int32_t renorm, const float* mix_scale, void* out, float* probs, int64_t* idx, float* lb,
                             float* aux, float* load, int32_t* choice, void* saved, void* scratch, void* stream) {
  RouteCall r = route_of(noise, 0, 0, probs, idx, lb); r.aux_out = aux; r.load_out = load; r.mix_scale = mix_scale;
  r.stage = RouterChoice{capacity, renorm != 0, choice};
  return site_forward("avmoe_moe_forward_choice", 0, desc, X, Y, params, out, r, saved, scratch, stream);
}

int avmoe_moe_forward_sinkhorn(const avmoe_moe_desc* desc, const void* X, const void* Y, const avmoe_moe_ptrs* params, const float* noise,
                               int32_t top_k, int32_t renorm, int32_t iters, const float* mix_scale, void* out, float* probs, int64_t* idx,
                               float* lb, float* aux, float* load, int32_t* choice, int32_t* count, void* saved, void* scratch,
                               void* stream) {
  RouteCall r = route_of(noise, top_k, renorm, probs, idx, lb); r.aux_out = aux; r.load_out = load; r.mix_scale = mix_scale;
  r.stage = RouterSinkhorn{iters, choice, count};
  return site_forward("avmoe_moe_forward_sinkhorn", 1, desc, X, Y, params, out, r, saved, scratch, stream);
}

int avmoe_moe_forward_capacity(const avmoe_moe_desc* desc, const void* X, const void* Y, const avmoe_moe_ptrs* params, const float* noise,
                               int32_t top_k, int32_t renorm, const float* mix_scale, const float* select_bias, float* select_count,
                               int32_t capacity, int32_t policy, float* cap_scale, int32_t* kept, int32_t* demand, int32_t* kept_count,
                               void* out, float* probs, int64_t* idx, float* lb, float* aux, float* load, void* saved, void* scratch,
                               void* stream) {
  RouteCall r = route_of(noise, top_k, renorm, probs, idx, lb);
  r.aux_out = aux; r.load_out = load; r.mix_scale = mix_scale; r.select_bias = select_bias; r.select_count = select_count;
  r.stage = RouterCapacity{capacity, policy, cap_scale, kept, demand, kept_count};
  return site_forward("avmoe_moe_forward_capacity", 1, desc, X, Y, params, out, r, saved, scratch, stream);
}

int avmoe_moe_forward_top_p(const avmoe_moe_desc* desc, const void* X, const void* Y, const avmoe_moe_ptrs* params, const float* noise,
                            float top_p, int32_t k_min, int32_t k_max, int32_t renorm, const float* mix_scale, void* out, float* probs,
                            int64_t* idx, float* lb, float* aux, float* load, int32_t* choice, int32_t* count, int32_t* khist, void* saved,
                            void* scratch, void* stream) {
  RouteCall r = route_of(noise, 0, renorm, probs, idx, lb); r.aux_out = aux; r.load_out = load; r.mix_scale = mix_scale;
  r.stage = RouterTopP{top_p, k_min, k_max, choice, count, khist};
  return site_forward("avmoe_moe_forward_top_p", 0, desc, X, Y, params, out, r, saved, scratch, stream);
}

int avmoe_moe_backward(const avmoe_moe_desc* desc, const void* X, const void* Y, const avmoe_moe_ptrs* params,
                       const void* dOut, const float* lb_grad, void* saved, void* scratch, void* dX, void* dY,
                       const avmoe_moe_ptrs* grads, void* stream) {
  return site_backward("avmoe_moe_backward", false, desc, X, Y, params, dOut, nullptr, lb_grad, nullptr, nullptr, saved, scratch, dX, dY, grads, 0, stream);
}

int avmoe_moe_backward_part(const avmoe_moe_desc* desc, const void* X, const void* Y, const avmoe_moe_ptrs* params,
                            const void* dOut, const float* lb_grad, void* saved, void* scratch, void* dX, void* dY,
                            const avmoe_moe_ptrs* grads, int32_t parts, void* stream) {
  return site_backward("avmoe_moe_backward_part", false, desc, X, Y, params, dOut, nullptr, lb_grad, nullptr, nullptr, saved, scratch, dX, dY, grads, parts, stream);
}

int avmoe_moe_backward_ex(const avmoe_moe_desc* desc, const void* X, const void* Y, const avmoe_moe_ptrs* params, const void* dOut,
                          const float* dprobs, const float* lb_grad, void* saved, void* scratch, void* dX, void* dY,
                          const avmoe_moe_ptrs* grads, int32_t parts, void* stream) {
  return site_backward("avmoe_moe_backward_ex", true, desc, X, Y, params, dOut, dprobs, lb_grad, nullptr, nullptr, saved, scratch, dX, dY, grads, parts, stream);
}

int avmoe_moe_backward_aux(const avmoe_moe_desc* desc, const void* X, const void* Y, const avmoe_moe_ptrs* params, const void* dOut,
                           const float* dprobs, const float* lb_grad, const float* aux_grad, void* saved, void* scratch, void* dX,
                           void* dY, const avmoe_moe_ptrs* grads, int32_t parts, void* stream) {
  return site_backward("avmoe_moe_backward_aux", true, desc, X, Y, params, dOut, dprobs, lb_grad, aux_grad, nullptr, saved, scratch, dX, dY, grads, parts, stream);
}

int avmoe_moe_backward_reg(const avmoe_moe_desc* desc, const void* X, const void* Y, const avmoe_moe_ptrs* params, const void* dOut,
                           const float* dprobs, const float* lb_grad, const float* aux_grad, const float* mix_scale, void* saved,
                           void* scratch, void* dX, void* dY, const avmoe_moe_ptrs* grads, int32_t parts, void* stream) {
  return site_backward("avmoe_moe_backward_reg", true, desc, X, Y, params, dOut, dprobs, lb_grad, aux_grad, mix_scale, saved, scratch, dX, dY, grads, parts, stream);
}

int avmoe_moe_backward_dx_dy(const avmoe_moe_desc* desc_a, const void* X_a, void* saved_a, void* scratch_a,
                             const avmoe_moe_desc* desc_b, void* saved_b, void* scratch_b, void* dT, void* stream) {
  Plan pa, pb;
  AVMOE_TRY(make_plan(desc_a, &pa));
  AVMOE_TRY(make_plan(desc_b, &pb));
  if (dT && (!X_a || !saved_a || !scratch_a || !saved_b || !scratch_b)) { set_last_error("avmoe_moe_backward_dx_dy: null pointer"); return ERR_BAD_ARG; }
  return moe_backward_dx_dy(pa, X_a, (char*)saved_a, (char*)scratch_a, pb, (char*)saved_b, (char*)scratch_b, dT, dT != nullptr, (hipStream_t)stream);
}

int avmoe_router_forward(const avmoe_moe_desc* desc, const float* rin, const avmoe_moe_ptrs* params, const float* noise,
                         float* probs, int64_t* idx, float* lb, void* saved, void* scratch, void* stream) {
  Plan pl;
  AVMOE_TRY(make_plan(desc, &pl));
  if (!rin || !params || !saved || !scratch) { set_last_error("avmoe_router_forward: null pointer"); return ERR_BAD_ARG; }
  const size_t bytes = (size_t)pl.d.S * 2 * pl.d.C * sizeof(float);
  if (hipMemcpyAsync((char*)saved + pl.o_rin, rin, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream) != hipSuccess) {
    set_last_error("avmoe_router_forward: copy of rin failed"); return ERR_LAUNCH;
  }
  return k_router(pl, (char*)saved, (char*)scratch, *params, route_of(noise, 0, 1, probs, idx, lb), (hipStream_t)stream);
}

int avmoe_expert_forward_cross(const avmoe_moe_desc* desc, const void* X, const void* Y, const avmoe_moe_ptrs* params, int32_t j,
                               void* out, void* saved, void* scratch, void* stream) {
  Plan pl;
  AVMOE_TRY(make_plan(desc, &pl));
  if (!X || !Y || !params || !out || !saved || !scratch) { set_last_error("avmoe_expert_forward_cross: null pointer"); return ERR_BAD_ARG; }
  if (j < 0 || j >= desc->E_m) { set_last_error("avmoe_expert_forward_cross: expert %d of %d cross-modal experts", j, desc->E_m); return ERR_BAD_ARG; }
  return expert_forward(pl, X, Y, *params, j, out, (char*)saved, (char*)scratch, (hipStream_t)stream);
}

int avmoe_expert_forward_uni(const avmoe_moe_desc* desc, const void* X, const void* Y, const avmoe_moe_ptrs* params, int32_t j,
                             void* out, void* saved, void* scratch, void* stream) {
  Plan pl;
  AVMOE_TRY(make_plan(desc, &pl));
  if (!X || !Y || !params || !out || !saved || !scratch) { set_last_error("avmoe_expert_forward_uni: null pointer"); return ERR_BAD_ARG; }
  if (j < 0 || j >= desc->E_s) { set_last_error("avmoe_expert_forward_uni: expert %d of %d unimodal experts", j, desc->E_s); return ERR_BAD_ARG; }
  return expert_forward(pl, X, Y, *params, desc->E_m + j, out, (char*)saved, (char*)scratch, (hipStream_t)stream);
}

int avmoe_remap_forward(const avmoe_moe_desc* desc, const void* Y, const avmoe_moe_ptrs* params, void* Yt, void* Yf, void* saved,
                        void* scratch, void* stream) {
  Plan pl;
  AVMOE_TRY(make_plan(desc, &pl));
  if (!Y || !params || !Yt || !Yf || !saved || !scratch) { set_last_error("avmoe_remap_forward: null pointer"); return ERR_BAD_ARG; }
  return remap_forward(pl, Y, *params, Yt, Yf, (char*)saved, (char*)scratch, (hipStream_t)stream);
}

int avmoe_moe_buffer_info(const avmoe_moe_desc* desc, int32_t index, const char** name, int32_t* region, size_t* offset,
                          size_t* bytes) {
  Plan pl;
  AVMOE_TRY(make_plan(desc, &pl));
  if (index < 0 || index >= pl.nbuf) { set_last_error("buffer index %d out of range", index); return ERR_BAD_ARG; }
  if (name) *name = pl.info[index].name;
  if (region) *region = pl.info[index].region;
  if (offset) *offset = pl.info[index].offset;
  if (bytes) *bytes = pl.info[index].bytes;
  return OK;
}


uint32_t avmoe_test_hooks(uint32_t force_mask, int32_t nxn_chunk) {
  const unsigned prev = switches().hook_mask.load();
  set_test_hooks(force_mask, nxn_chunk);
  return prev;
}

// One strip kernel of the AVVP N x N block (nxn_att.hip) on raw operands, Np = N: no arithmetic of its own -- the pointers the op needs,
// then the wrapper and its status (shapes the kernels do not serve: ERR_UNSUPPORTED from the wrappers' own check).
int avmoe_nxn_strip(int32_t op, const void* X, const void* dxr, int32_t frames, int32_t N, int32_t C, float* lse, float* rowdot, void* out,
                    const void* att_in, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  bool ok = X != nullptr;
  switch (op) {
    case AVMOE_NXN_STATS:        ok = ok && lse; break;
    case AVMOE_NXN_ATT:
    case AVMOE_NXN_ATT_FROM_LSE:
    case AVMOE_NXN_XR:           ok = ok && lse && out; break;
    case AVMOE_NXN_Y:
    case AVMOE_NXN_DXQ:
    case AVMOE_NXN_DXK:          ok = ok && dxr && lse && rowdot && out; break;
    case AVMOE_NXN_ATT_BWD:      ok = ok && dxr && rowdot && out && att_in; break;
    default: set_last_error("avmoe_nxn_strip: unknown op %d", op); return ERR_BAD_ARG;
  }
  if (!ok) { set_last_error("avmoe_nxn_strip: op %d: null pointer", op); return ERR_BAD_ARG; }
  switch (op) {
    case AVMOE_NXN_STATS:        return k_nxn_att(X, frames, N, C, N, lse, nullptr, 0, st);
    case AVMOE_NXN_ATT:          return k_nxn_att(X, frames, N, C, N, lse, out, 0, st);
    case AVMOE_NXN_ATT_FROM_LSE: return k_nxn_att(X, frames, N, C, N, lse, out, 1, st);
    case AVMOE_NXN_XR:           return k_nxn_xr(X, frames, N, C, N, lse, out, st);
    case AVMOE_NXN_Y:            return k_nxn_y(X, dxr, frames, N, C, N, lse, rowdot, out, st);
    case AVMOE_NXN_DXQ:          return k_nxn_dx(0, X, dxr, frames, N, C, N, lse, rowdot, out, st);
    case AVMOE_NXN_DXK:          return k_nxn_dx(1, X, dxr, frames, N, C, N, lse, rowdot, out, st);
    default:                     return k_nxn_att_bwd(X, dxr, frames, N, C, N, rowdot, att_in, out, st);
  }
}

// The tiled engine's further forms on raw operands (tests only): fills a GemmArgs from the descriptor and calls launch_gemm -- no arithmetic and
// no check of its own beyond the NULL descriptor / pointer arrays; every refusal and status is the engine's.
int avmoe_gemm_form(const avmoe_gemm_form_desc* desc, const void* const* A, const void* const* B, void* C, const float* row_scale, const void* D,
                    void* workspace, float* row_part, const float* row_lse, void* stream) {
  if (!desc || !A || !B) { set_last_error("avmoe_gemm_form: null desc or pointer array"); return ERR_BAD_ARG; }
  GemmArgs a = to_args(&desc->base);
  a.A = A[0]; a.B = B[0]; a.C = C; a.row_scale = row_scale; a.D = D; a.slabs = (float*)workspace;
  a.nb3 = desc->nb3; a.sA3 = desc->sA3; a.sB3 = desc->sB3; a.sC3 = desc->sC3;
  a.epi = desc->epi; a.keep_slabs = desc->keep_slabs; a.row_part = row_part; a.row_lse = row_lse;
  for (int i = 0; i < 3; ++i) {
    const avmoe_gemm_form_seg& s = desc->seg[i];
    GemmSeg& g = a.seg[i];
    g.A = A[i + 1]; g.B = B[i + 1]; g.K = s.K; g.a_layout = s.a_layout; g.b_layout = s.b_layout;
    g.lda = s.lda; g.ldb = s.ldb; g.sA1 = s.sA1; g.sA2 = s.sA2; g.sB1 = s.sB1; g.sB2 = s.sB2;
  }
  return launch_gemm(a, (hipStream_t)stream);
}

int avmoe_gemm_row_lse(const float* row_part, int64_t rows, int32_t tiles, float* lse, void* stream) {
  if (rows > 0 && (!row_part || !lse || tiles <= 0)) { set_last_error("avmoe_gemm_row_lse: null pointer or tiles <= 0"); return ERR_BAD_ARG; }
  return gemm_row_lse(row_part, (long)rows, tiles, lse, (hipStream_t)stream);
}

void avmoe_prof_enable(int on) { prof_enable(on != 0); }
void avmoe_prof_reset(void) { prof_reset(); }
size_t avmoe_prof_report(char* buf, size_t cap) { return prof_report(buf, cap); }

}  // extern "C"
