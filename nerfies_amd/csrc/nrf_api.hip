// C-ABI entry points of the MI355X nerfies hot path (include/nerfies_amd.h is the contract): handle life cycle, validation, the
// per-op and debug entry points.  The plan lives in nrf_plan.hip, the launch sequences in nrf_run.hip (nrf_handle.h).
#include "nrf_handle.h"

using namespace nrf;
using namespace nrf::api;

thread_local char nrf::api::g_err[256] = "ok";

const Knobs& nrf::knobs() {
  static const Knobs k = [] {
    Knobs v;
    v.trace_regions = getenv("NRF_TRACE_REGIONS") != nullptr;
#ifdef NRF_EXPERIMENT
    v.debug_occ = getenv("NRF_DEBUG_OCC") != nullptr;
    v.timeline = getenv("NRF_TIMELINE") != nullptr;
    v.dynamic_tiles = getenv("NRF_DYNAMIC_TILES") != nullptr;
    if (const char* e = getenv("NRF_GRID_MUL")) v.grid_mul = atoi(e) < 1 ? 1 : atoi(e);
    if (const char* e = getenv("NRF_WARP_GRID_MUL")) v.warp_grid_mul = atoi(e);
    if (const char* e = getenv("NRF_OLD_SHARE")) v.old_share = atof(e);
#endif
    return v;
  }();
  return k;
}

extern "C" {

int nrf_version(void) { return NRF_VERSION; }
const char* nrf_last_error(void) { return g_err; }

int nrf_create(const nrf_model_desc* desc, nrf_handle* out) {
  if (!desc || !out) return fail(NRF_E_NULL, "desc / out is null");
  const nrf_model_desc& d = *desc;
  // The chains run 8 trunk layers with ONE layer that reads [h, posenc] (modules.py:41-62 concatenates the inputs in front of layer i
  // for i in skips).  The caller's trunk (depth xd <= 8, skip xs) is laid out on them:
  //   * no skip reached (nerf_skips = () or xs >= xd): layers 0..xd-1, zero posenc rows in layer 4, identity layers behind;
  //   * xs <= 4 and xd - xs <= 4: layers 0..xs-1, IDENTITY layers xs..3 (relu(h . I) = h for h >= 0: exact, also on the bf16 chain),
  //     the caller's skip layer at 4, the rest behind it -- the kernels' own layout, every mode;
  //   * any other xs in 1..7: layers in place, the skip GEMM moves to layer xs (float32 chains only: a run-time layer index there,
  //     a compile-time position in the bf16 stream).
  const bool skip_reached = d.nerf_skip_layer >= 0 && d.nerf_skip_layer < d.nerf_trunk_depth;
  if (d.nerf_trunk_depth < 1 || d.nerf_trunk_depth > TRUNK_DEPTH)
    return fail(NRF_E_UNSUPPORTED, "nerf_trunk_depth must be in [1,8]");
  if (skip_reached && d.nerf_skip_layer == 0)   // layer 0 would read [posenc, posenc]: two blocks of one leaf on the same rows
    return fail(NRF_E_UNSUPPORTED, "nerf_skips = (0,) (the first layer reading its input twice) is not built");
  if (d.nerf_trunk_width < 1 || d.nerf_trunk_width > TRUNK_W)   // narrower trunks run zero-padded (test_vrig.gin: 128)
    return fail(NRF_E_UNSUPPORTED, "nerf_trunk_width must be in [1,256]");
  // rgb branch (modules.py:129-134): 1..4 layers; layer 0 reads [bottleneck, condition], layers 1.. are (width, width) and run
  // under a run-time count in the float32 64-row chains.  Depth 0 (the logits straight on [bottleneck, condition]) is not built.
  if (d.nerf_rgb_branch_depth < 1 || d.nerf_rgb_branch_depth > RGB_MAX_DEPTH)
    return fail(NRF_E_UNSUPPORTED, "nerf_rgb_branch_depth must be in [1,4]");
  if (d.nerf_rgb_branch_width < 1 || d.nerf_rgb_branch_width > RGB_W)
    return fail(NRF_E_UNSUPPORTED, "nerf_rgb_branch_width must be in [1,128]");
  if (d.use_trunk_condition)   // models.py:203-204: never forwarded by construct_nerf, no preset; a silent no-op would change the layout
    return fail(NRF_E_UNSUPPORTED, "use_trunk_condition (trunk conditioning) is not built");
  if (d.use_alpha_condition && d.use_appearance_metadata && (d.num_appearance_features < 1 || d.num_appearance_features > 16))
    return fail(NRF_E_SHAPE, "num_appearance_features must be in [1,16]");
  if (!(d.noise_std >= 0.f)) return fail(NRF_E_SHAPE, "noise_std must be >= 0");
  if (d.use_warp && d.warp_metadata_encoder_type != NRF_META_GLO && d.warp_metadata_encoder_type != NRF_META_TIME)
    return fail(NRF_E_UNSUPPORTED, "warp_metadata_encoder_type must be glo or time ('blend' exists only for the TranslationField, no preset)");
  if (d.use_warp && d.warp_metadata_encoder_type == NRF_META_TIME && (d.num_time_encoder_freqs < 0 || d.num_time_encoder_freqs > 8))
    return fail(NRF_E_SHAPE, "num_time_encoder_freqs must be in [0,8]");
  if (d.use_warp) {
    if (d.warp_field_type != NRF_WARP_SE3 && d.warp_field_type != NRF_WARP_TRANSLATION) return fail(NRF_E_UNSUPPORTED, "warp_field_type");
    if (d.num_warp_freqs < 0 || d.num_warp_freqs > 8) return fail(NRF_E_SHAPE, "num_warp_freqs must be in [0,8]");
    if (d.num_warp_features < 1 || d.num_warp_features > 8) return fail(NRF_E_SHAPE, "num_warp_features must be in [1,8]");
    if (d.num_warp_embeddings < 1 && d.warp_metadata_encoder_type != NRF_META_TIME) return fail(NRF_E_SHAPE, "num_warp_embeddings must be positive");
    if (d.warp_trunk_depth < 0 || d.warp_trunk_depth > WARP_DEPTH) return fail(NRF_E_UNSUPPORTED, "warp_trunk_depth must be in [1,6] (0 = 6)");
    if (d.warp_trunk_width < 0 || d.warp_trunk_width > WARP_W) return fail(NRF_E_UNSUPPORTED, "warp_trunk_width must be in [1,128] (0 = 128)");
  }
  if (d.num_coarse_samples < 3 || d.num_coarse_samples > 256) return fail(NRF_E_SHAPE, "num_coarse_samples must be in [3,256]");
  if (d.num_fine_samples < 0 || d.num_coarse_samples + d.num_fine_samples > 512)
    return fail(NRF_E_SHAPE, "num_coarse_samples + num_fine_samples must be <= 512");
  if (d.num_nerf_point_freqs < 1 || d.num_nerf_point_freqs > 10) return fail(NRF_E_SHAPE, "num_nerf_point_freqs must be in [1,10]");
  if (d.num_nerf_viewdir_freqs < 0 || d.num_nerf_viewdir_freqs > 8) return fail(NRF_E_SHAPE, "num_nerf_viewdir_freqs must be in [0,8]");
  if (d.sigma_activation != NRF_ACT_RELU && d.sigma_activation != NRF_ACT_SOFTPLUS) return fail(NRF_E_UNSUPPORTED, "sigma_activation");
  nrf_handle h = new nrf_handle_s();
  h->d = d;
  {
    const int xd = d.nerf_trunk_depth, xs = skip_reached ? d.nerf_skip_layer : -1;
    h->xdepth = xd; h->xskip = xs;                                              // what the caller's tree holds
    int imap[TRUNK_DEPTH], K = SKIP_LAYER;
    for (int i = 0; i < TRUNK_DEPTH; ++i) imap[i] = i;
    if (xs >= 0 && xs <= SKIP_LAYER && xd - xs <= TRUNK_DEPTH - SKIP_LAYER) {
      for (int i = xs; i < xd; ++i) imap[i] = SKIP_LAYER + (i - xs);
    } else if (xs >= 0) {
      K = xs;
    }
    for (int i = 0; i < TRUNK_DEPTH; ++i) h->emap[i] = -1;
    for (int i = 0; i < xd; ++i) h->emap[imap[i]] = i;
    h->d.nerf_trunk_depth = TRUNK_DEPTH; h->d.nerf_skip_layer = K;                // what the kernels run
  }
  h->nlevels = d.num_fine_samples > 0 ? 2 : 1;
  h->P = 3 + 6 * d.num_nerf_point_freqs;
  h->PK = (h->P + 15) / 16 * 16;                  // K of the posenc GEMMs: whole 16-k quads of the MFMA loop
  h->V = d.use_viewdirs ? 3 + 6 * d.num_nerf_viewdir_freqs : 0;
  h->app_in_cond = (d.use_appearance_metadata && d.use_alpha_condition) ? 1 : 0;   // models.py:206
  h->A = h->app_in_cond ? d.num_appearance_features : 0;                              // models.py:204-205
  h->warp = d.use_warp != 0;
  if (h->warp) {
    h->time_enc = d.warp_metadata_encoder_type == NRF_META_TIME;
    h->Ft = d.num_time_encoder_freqs; h->Tin = 1 + 2 * h->Ft;   // AnnealedSinusoidalEncoder of the scalar time stamp
    h->Fw = d.num_warp_freqs; h->G = d.num_warp_features;
    h->wxdepth = d.warp_trunk_depth ? d.warp_trunk_depth : WARP_DEPTH;
    h->wxwidth = d.warp_trunk_width ? d.warp_trunk_width : WARP_W;
    h->Win = 3 + 6 * h->Fw + h->G;                 // [annealed posenc, GLO code] (warping.py:326-327)
    h->PKw = (h->Win + 15) / 16 * 16;
  }
  h->R = h->V + (h->app_in_cond ? d.num_appearance_features : 0) + (d.use_camera_metadata ? d.num_camera_features : 0);
  if (h->R > 64) { delete h; return fail(NRF_E_SHAPE, "rgb condition wider than 64"); }
  build_layout(h);
  build_pack_offsets(h);
  *out = h;
  return NRF_OK;
}

int nrf_destroy(nrf_handle h) {
  delete h;
  return NRF_OK;
}

int nrf_param_count(nrf_handle h, int64_t* n) {
  if (!h || !n) return fail(NRF_E_NULL, "null");
  *n = h->xnparams;
  return NRF_OK;
}

int nrf_param_layout(nrf_handle h, nrf_tensor_info* out, int32_t* n) {
  if (!h || !n) return fail(NRF_E_NULL, "null");
  if (out) {
    if (*n < (int32_t)h->xlayout.size()) return fail(NRF_E_SHAPE, "layout array too small");
    memcpy(out, h->xlayout.data(), h->xlayout.size() * sizeof(nrf_tensor_info));
  }
  *n = (int32_t)h->xlayout.size();
  return NRF_OK;
}

// The flag word of nrf_forward / nrf_workspace_bytes*: unknown bits and contradictory combinations are refused up front
// (they used to pass through: NRF_FLAG_WARP_F32 without NRF_FLAG_BF16 was silently ignored, and TRAIN | WARP_JACOBIAN sized a
// workspace for a plan no call can run).
static int check_flags(const nrf_handle_s* h, uint32_t flags) {
  const uint32_t known = NRF_FLAG_TRAIN | NRF_FLAG_NO_WARP | NRF_FLAG_BF16 | NRF_FLAG_WARP_JACOBIAN | NRF_FLAG_WARP_F32 | NRF_FLAG_BF16X3 |
                         NRF_FLAG_RAY_GRADS | NRF_FLAG_FROZEN;
  if (flags & ~known) return fail(NRF_E_UNSUPPORTED, "unknown bits in flags");
  if (flags & NRF_FLAG_FROZEN) {   // one valid word: TRAIN | RAY_GRADS | FROZEN (float32 mode)
    if (!(flags & NRF_FLAG_TRAIN) || !(flags & NRF_FLAG_RAY_GRADS))
      return fail(NRF_E_UNSUPPORTED, "NRF_FLAG_FROZEN narrows the stash of NRF_FLAG_TRAIN | NRF_FLAG_RAY_GRADS to what nrf_backward_rays reads: "
                                     "only together with both");
    if (flags & (NRF_FLAG_BF16 | NRF_FLAG_BF16X3 | NRF_FLAG_WARP_JACOBIAN))
      return fail(NRF_E_UNSUPPORTED, "NRF_FLAG_FROZEN is built for the float32 mode: not with NRF_FLAG_BF16 / NRF_FLAG_BF16X3 / "
                                     "NRF_FLAG_WARP_JACOBIAN");
  }
  if ((flags & NRF_FLAG_RAY_GRADS) && (flags & (NRF_FLAG_BF16 | NRF_FLAG_BF16X3)))
    return fail(NRF_E_UNSUPPORTED, "NRF_FLAG_RAY_GRADS is built for the float32 mode: not with NRF_FLAG_BF16 / NRF_FLAG_BF16X3");
  if ((flags & NRF_FLAG_RAY_GRADS) && !(flags & NRF_FLAG_TRAIN))
    return fail(NRF_E_UNSUPPORTED, "NRF_FLAG_RAY_GRADS keeps what nrf_backward_rays reads of a stashed forward: only together with NRF_FLAG_TRAIN");
  if ((flags & NRF_FLAG_BF16X3) && (flags & (NRF_FLAG_TRAIN | NRF_FLAG_BF16)))
    return fail(NRF_E_UNSUPPORTED, "NRF_FLAG_BF16X3 is an inference mode of its own: not with NRF_FLAG_TRAIN (the training chains stash float32 or "
                                   "bfloat16 activations) and not with NRF_FLAG_BF16");
  if ((flags & NRF_FLAG_WARP_F32) && !(flags & (NRF_FLAG_BF16 | NRF_FLAG_BF16X3)))
    return fail(NRF_E_UNSUPPORTED, "NRF_FLAG_WARP_F32 only qualifies NRF_FLAG_BF16 / NRF_FLAG_BF16X3 (the float32 mode runs the warp trunk in float32 anyway)");
  if ((flags & NRF_FLAG_TRAIN) && (flags & NRF_FLAG_WARP_JACOBIAN))
    return fail(NRF_E_UNSUPPORTED, "NRF_FLAG_WARP_JACOBIAN is an inference output (training consumes the Jacobian through nrf_elastic)");
  if ((flags & NRF_FLAG_TRAIN) && (flags & NRF_FLAG_NO_WARP))
    return fail(NRF_E_UNSUPPORTED, "NRF_FLAG_NO_WARP cannot be combined with NRF_FLAG_TRAIN");
  if ((flags & (NRF_FLAG_BF16 | NRF_FLAG_BF16X3)) && h->d.nerf_skip_layer != SKIP_LAYER)
    return fail(NRF_E_UNSUPPORTED, "NRF_FLAG_BF16: the bfloat16 chains run the skip at trunk layer 4; this model's nerf_skips cannot be laid out "
                                   "around it (needs skip <= 4 and depth - skip <= 4): use the float32 mode");
  if ((flags & (NRF_FLAG_BF16 | NRF_FLAG_BF16X3)) && h->d.nerf_rgb_branch_depth > 1)
    return fail(NRF_E_UNSUPPORTED, "NRF_FLAG_BF16 / NRF_FLAG_BF16X3: the bfloat16 chains run an rgb branch of one layer; this model's "
                                   "nerf_rgb_branch_depth > 1 (rgb branch layers 1..) exists in the float32 chains only: use the float32 mode");
  return NRF_OK;
}

int nrf_workspace_bytes(nrf_handle h, int32_t num_rays, uint32_t flags, size_t* bytes) {
  if (!h || !bytes) return fail(NRF_E_NULL, "null");
  if (num_rays <= 0) return fail(NRF_E_SHAPE, "num_rays must be positive");
  CK(check_flags(h, flags));
  query_device(h);
  build_plan(h, num_rays, flags);
  *bytes = h->plan.total_floats * sizeof(float);
  return NRF_OK;
}

int nrf_forward(nrf_handle h, const float* params, const nrf_rays* rays, const nrf_step_scalars* scalars,
                const nrf_rand* rnd, const nrf_outputs* out, uint32_t flags, void* workspace, size_t workspace_bytes,
                void* stream) {
  if (!h) return fail(NRF_E_NULL, "handle is null");
  CK(check_flags(h, flags));
  return forward_impl(h, params, rays, scalars, rnd, out, flags, (float*)workspace, workspace_bytes, (hipStream_t)stream);
}

// nrf_backward / nrf_backward_ex: the state checks, the zero stand-in of a missing d_rgb, the reverse pass
static int backward_checked(nrf_handle h, const float* params, const nrf_rays* rays, nrf_output_grads g, float* grad_params,
                            void* workspace, size_t workspace_bytes, void* stream, const nrf_ray_grads* rg = nullptr) {
  if (!h || !params || !rays || !workspace) return fail(NRF_E_NULL, "null argument");
  // a frozen stash (NRF_FLAG_FROZEN) is the one case without a parameter gradient: nrf_backward_rays with grad_params NULL
  const bool frozen = h->stashed_ws == workspace && h->stashed_modes.frozen;
  if (!grad_params && !frozen) return fail(NRF_E_NULL, "null argument");
  if (h->stashed_ws != workspace || h->stashed_B != rays->num_rays)
    return fail(NRF_E_STATE, rg ? "nrf_backward_rays needs a preceding nrf_forward(NRF_FLAG_TRAIN | NRF_FLAG_RAY_GRADS) on this workspace"
                                : "nrf_backward needs a preceding nrf_forward(NRF_FLAG_TRAIN) on this workspace");
  if (rg && !h->stashed_modes.ray_grads)
    return fail(NRF_E_STATE, "nrf_backward_rays: the stashed nrf_forward ran without NRF_FLAG_RAY_GRADS (nothing of the rays' "
                             "gradient was kept); run nrf_forward(NRF_FLAG_TRAIN | NRF_FLAG_RAY_GRADS)");
  if (rg && rg->d_viewdirs && (!h->d.use_viewdirs || !rays->viewdirs || h->V > 64))
    return fail(NRF_E_UNSUPPORTED, "nrf_ray_grads.d_viewdirs needs a model with use_viewdirs (at most 64 encoded columns) and rays->viewdirs "
                                   "(without them the condition does not read a view direction of its own)");
  if (h->stashed_plan != h->plan.serial)   // another call re-planned the handle (other num_rays / flags) since the stashed forward
    return fail(NRF_E_STATE, "nrf_backward: the workspace layout changed since the stashed nrf_forward (an intervening call with "
                             "another num_rays / flags); run nrf_forward(NRF_FLAG_TRAIN) again");
  if (workspace_bytes < h->plan.total_floats * sizeof(float)) return fail(NRF_E_WORKSPACE, "workspace too small");
  if (frozen && !rg)
    return fail(NRF_E_STATE, "nrf_backward: the stashed nrf_forward ran under NRF_FLAG_FROZEN (nothing of the parameter gradient was "
                             "kept); call nrf_backward_rays with grad_params NULL, or run nrf_forward without the flag");
  if (frozen && grad_params)
    return fail(NRF_E_STATE, "nrf_backward_rays: the stashed nrf_forward ran under NRF_FLAG_FROZEN (nothing of the parameter gradient "
                             "was kept): grad_params must be NULL");
  if (h->nlevels < 2) g.fine = nrf_level_grads{};   // no fine level: nothing to read
  if ((g.coarse.d_warped_points || g.fine.d_warped_points) && !h->stashed_modes.warp_on)
    return fail(NRF_E_STATE, "nrf_backward_ex: d_warped_points given, but the stashed nrf_forward ran without the warp field "
                             "(there are no warped points to carry a gradient)");
  float* ws = (float*)workspace;
  hipStream_t st = (hipStream_t)stream;
  const float* zero = ws + h->plan.zero_rgb;
  if (!g.coarse.d_rgb || (h->nlevels > 1 && !g.fine.d_rgb)) {
    hipError_t e = hipMemsetAsync(ws + h->plan.zero_rgb, 0, (size_t)rays->num_rays * 3 * sizeof(float), st);
    if (e != hipSuccess) return fail_hip(e, "zero d_rgb");
  }
  if (!g.coarse.d_rgb) g.coarse.d_rgb = zero;
  if (!g.fine.d_rgb) g.fine.d_rgb = zero;
  if (frozen) return backward_rays_frozen_impl(h, params, rays, &g, nullptr, rg, nullptr, ws, st);
  return backward_impl(h, params, rays, &g, nullptr, grad_params, nullptr, ws, st, nullptr, nullptr, nullptr, nullptr, false, rg);
}

int nrf_backward(nrf_handle h, const float* params, const nrf_rays* rays, const float* d_rgb_coarse,
                 const float* d_rgb_fine, float* grad_params, void* workspace, size_t workspace_bytes, void* stream) {
  nrf_output_grads g{};
  g.coarse.d_rgb = d_rgb_coarse; g.fine.d_rgb = d_rgb_fine;
  return backward_checked(h, params, rays, g, grad_params, workspace, workspace_bytes, stream);
}

int nrf_backward_ex(nrf_handle h, const float* params, const nrf_rays* rays, const nrf_output_grads* g, float* grad_params,
                    void* workspace, size_t workspace_bytes, void* stream) {
  if (!g) return fail(NRF_E_NULL, "nrf_output_grads is null (pass a zeroed struct for a zero gradient)");
  return backward_checked(h, params, rays, *g, grad_params, workspace, workspace_bytes, stream);
}

int nrf_backward_rays(nrf_handle h, const float* params, const nrf_rays* rays, const nrf_output_grads* g, const nrf_ray_grads* rg,
                      float* grad_params, void* workspace, size_t workspace_bytes, void* stream) {
  if (!g) return fail(NRF_E_NULL, "nrf_output_grads is null (pass a zeroed struct for a zero gradient)");
  if (!rg) return fail(NRF_E_NULL, "nrf_ray_grads is null (pass a struct of NULL pointers for no ray gradient)");
  return backward_checked(h, params, rays, *g, grad_params, workspace, workspace_bytes, stream, rg);
}

int nrf_train_step_loss_grad(nrf_handle h, const float* params, const nrf_rays* rays, const float* target_rgb,
                             const nrf_step_scalars* scalars, const nrf_rand* rnd, float* grad_params, float* stats,
                             void* workspace, size_t workspace_bytes, void* stream) {
  if (!h || !target_rgb || !grad_params) return fail(NRF_E_NULL, "null argument");
  CK(forward_impl(h, params, rays, scalars, rnd, nullptr, NRF_FLAG_TRAIN, (float*)workspace, workspace_bytes,
                  (hipStream_t)stream));
  return backward_impl(h, params, rays, nullptr, target_rgb, grad_params, stats, (float*)workspace, (hipStream_t)stream);
}

// nrf_train_step_loss_grad_ex / _rays behind their own flag checks: the regularisers' validation, forward, reverse.  `flags`: the
// forward's whole word; rg: the ray gradients to write, or nullptr
static int train_step_ex(nrf_handle h, const float* params, const nrf_rays* rays, const float* target_rgb,
                         const nrf_step_scalars* scalars, const nrf_rand* rnd, const nrf_background* bg, const nrf_elastic* el,
                         const nrf_warp_reg* wr, uint32_t flags, const nrf_ray_grads* rg, float* grad_params, float* stats,
                         void* workspace, size_t workspace_bytes, void* stream) {
  int bgN = 0;
  if (el) {
    if (!h->warp) return fail(NRF_E_UNSUPPORTED, "the elastic regulariser needs the warp field");
    if (el->reduce_method != NRF_ELASTIC_WEIGHT && el->reduce_method != NRF_ELASTIC_MEDIAN)
      return fail(NRF_E_UNSUPPORTED, "unknown elastic reduce_method");
    if (el->loss_type < NRF_ELASTIC_LOG_SVALS || el->loss_type > NRF_ELASTIC_LOG_DET)
      return fail(NRF_E_UNSUPPORTED, "unknown elastic loss_type ('nr' is not built: the reference marks it as producing NaNs)");
    if (!scalars) return fail(NRF_E_NULL, "nrf_step_scalars required");
  }
  if (wr && !h->warp) return fail(NRF_E_UNSUPPORTED, "the warp_reg loss needs the warp field");
  if (bg && bg->num_points > 0) {
    if (!h->warp) return fail(NRF_E_UNSUPPORTED, "the background regulariser needs the warp field");
    if (h->time_enc) return fail(NRF_E_UNSUPPORTED, "the background regulariser draws warp IDS (training.py:121-123): not defined for the time encoder");
    if (!bg->points) return fail(NRF_E_NULL, "background points is null");
    if (!bg->warp_ids && (!bg->id_choices || bg->num_choices <= 0))
      return fail(NRF_E_NULL, "background: give warp_ids (points already noised) or id_choices (the library draws ids and noise)");
    if (!scalars) return fail(NRF_E_NULL, "nrf_step_scalars required");
    bgN = bg->num_points;
  }
  CK(forward_impl(h, params, rays, scalars, rnd, nullptr, flags, (float*)workspace, workspace_bytes, (hipStream_t)stream, bgN,
                  el ? 1 : 0, bgN > 0 ? bg : nullptr));
  return backward_impl(h, params, rays, nullptr, target_rgb, grad_params, stats, (float*)workspace, (hipStream_t)stream,
                       bgN > 0 ? bg : nullptr, scalars, el, wr, /*bg_forward_done=*/bgN > 0, rg);
}

int nrf_train_step_loss_grad_ex(nrf_handle h, const float* params, const nrf_rays* rays, const float* target_rgb,
                                const nrf_step_scalars* scalars, const nrf_rand* rnd, const nrf_background* bg,
                                const nrf_elastic* el, const nrf_warp_reg* wr, uint32_t flags, float* grad_params, float* stats,
                                void* workspace, size_t workspace_bytes, void* stream) {
  if (!h || !target_rgb || !grad_params) return fail(NRF_E_NULL, "null argument");
  if (flags & NRF_FLAG_RAY_GRADS)
    return fail(NRF_E_UNSUPPORTED, "NRF_FLAG_RAY_GRADS: nrf_train_step_loss_grad_ex has no ray gradient; use nrf_train_step_loss_grad_rays "
                                   "(or nrf_forward + nrf_backward_rays)");
  if (flags & ~(uint32_t)(NRF_FLAG_BF16 | NRF_FLAG_WARP_F32)) return fail(NRF_E_UNSUPPORTED, "nrf_train_step_loss_grad_ex flags: 0, NRF_FLAG_BF16 [| NRF_FLAG_WARP_F32]");
  CK(check_flags(h, NRF_FLAG_TRAIN | flags));   // the same word nrf_workspace_bytes_ex validated (WARP_F32 without BF16 is refused here too)
  return train_step_ex(h, params, rays, target_rgb, scalars, rnd, bg, el, wr, NRF_FLAG_TRAIN | flags, nullptr, grad_params, stats,
                       workspace, workspace_bytes, stream);
}

int nrf_train_step_loss_grad_rays(nrf_handle h, const float* params, const nrf_rays* rays, const float* target_rgb,
                                  const nrf_step_scalars* scalars, const nrf_rand* rnd, const nrf_background* bg,
                                  const nrf_elastic* el, const nrf_warp_reg* wr, uint32_t flags, const nrf_ray_grads* ray_grads,
                                  float* grad_params, float* stats, void* workspace, size_t workspace_bytes, void* stream) {
  if (!h || !target_rgb || !grad_params) return fail(NRF_E_NULL, "null argument");
  if (!ray_grads) return fail(NRF_E_NULL, "nrf_ray_grads is null (nrf_train_step_loss_grad_ex is the step without ray gradients)");
  if (flags)
    return fail(NRF_E_UNSUPPORTED, "nrf_train_step_loss_grad_rays flags: 0 (the float32 mode only: no NRF_FLAG_BF16, NRF_FLAG_BF16X3 or "
                                   "NRF_FLAG_WARP_F32; NRF_FLAG_TRAIN | NRF_FLAG_RAY_GRADS are implied)");
  if (ray_grads->d_viewdirs && rays && (!h->d.use_viewdirs || !rays->viewdirs || h->V > 64))
    return fail(NRF_E_UNSUPPORTED, "nrf_ray_grads.d_viewdirs needs a model with use_viewdirs (at most 64 encoded columns) and rays->viewdirs "
                                   "(without them the view term is part of d_directions)");
  CK(check_flags(h, NRF_FLAG_TRAIN | NRF_FLAG_RAY_GRADS));
  return train_step_ex(h, params, rays, target_rgb, scalars, rnd, bg, el, wr, NRF_FLAG_TRAIN | NRF_FLAG_RAY_GRADS, ray_grads,
                       grad_params, stats, workspace, workspace_bytes, stream);
}

int nrf_loss_grad_rays(nrf_handle h, const float* params, const nrf_rays* rays, const float* target_rgb, const nrf_step_scalars* scalars,
                       const nrf_rand* rnd, const nrf_ray_grads* ray_grads, float* stats, void* workspace, size_t workspace_bytes,
                       void* stream) {
  if (!h || !target_rgb) return fail(NRF_E_NULL, "null argument");
  if (!ray_grads) return fail(NRF_E_NULL, "nrf_ray_grads is null (the frozen step returns nothing else)");
  if (ray_grads->d_viewdirs && rays && (!h->d.use_viewdirs || !rays->viewdirs || h->V > 64))
    return fail(NRF_E_UNSUPPORTED, "nrf_ray_grads.d_viewdirs needs a model with use_viewdirs (at most 64 encoded columns) and rays->viewdirs "
                                   "(without them the view term is part of d_directions)");
  const uint32_t flags = NRF_FLAG_TRAIN | NRF_FLAG_RAY_GRADS | NRF_FLAG_FROZEN;
  CK(check_flags(h, flags));
  CK(forward_impl(h, params, rays, scalars, rnd, nullptr, flags, (float*)workspace, workspace_bytes, (hipStream_t)stream));
  return backward_rays_frozen_impl(h, params, rays, nullptr, target_rgb, ray_grads, stats, (float*)workspace, (hipStream_t)stream, scalars);
}

int nrf_workspace_bytes_ex(nrf_handle h, int32_t num_rays, uint32_t flags, int32_t num_background_points,
                           int32_t use_elastic_loss, size_t* bytes) {
  if (!h || !bytes) return fail(NRF_E_NULL, "null");
  if (num_rays <= 0 || num_background_points < 0) return fail(NRF_E_SHAPE, "bad sizes");
  if ((num_background_points > 0 || use_elastic_loss) && !h->warp)
    return fail(NRF_E_UNSUPPORTED, "the background / elastic regularisers need the warp field");
  CK(check_flags(h, flags));
  if ((flags & NRF_FLAG_FROZEN) && (num_background_points > 0 || use_elastic_loss))
    return fail(NRF_E_UNSUPPORTED, "NRF_FLAG_FROZEN: the frozen step applies no regulariser (no background points, no elastic loss)");
  query_device(h);
  const bool tr = flags & NRF_FLAG_TRAIN;
  build_plan(h, num_rays, flags, tr ? num_background_points : 0, tr && use_elastic_loss ? 1 : 0);
  *bytes = h->plan.total_floats * sizeof(float);
  return NRF_OK;
}

// Stand-alone SE3 field on arbitrary points (create_warp_field(num_batch_dims=1), models.py:165-184; the
// field training.compute_background_loss applies, training.py:127-130).  Mini workspace:
// [pack descriptors | packed trunk weights | padded output].
namespace {
struct WarpPointsPlan { size_t desc_f, wpk_f, out_f, ctr_f, emb_f, ip_f, total_f; int ntiles; };
WarpPointsPlan warp_points_plan(nrf_handle h, int n) {
  WarpPointsPlan q;
  q.ntiles = (n + TILE_ROWS - 1) / TILE_ROWS;
  size_t o = 0;
  auto take = [&](size_t f) { size_t r = o; o = align_up(o + f, ALIGN_F); return r; };
  q.desc_f = take(16 * sizeof(PackDesc) / 4);
  q.wpk_f = take(h->wpk.total);
  q.out_f = take((size_t)q.ntiles * TILE_ROWS * 3);
  q.ctr_f = take(16);
  q.emb_f = q.ip_f = 0;
  if (h->d.warp_field_type == NRF_WARP_TRANSLATION || h->wxdepth != WARP_DEPTH || h->wxwidth != WARP_W) {
    // no rotation head in the caller's tree, or a trunk shallower / narrower than the kernels': run on the padded image
    q.emb_f = take((h->emb.size() + 1) * sizeof(EmbedDesc) / 4);
    q.ip_f = take((size_t)h->nparams);
  }
  q.total_f = o;
  return q;
}
}  // namespace

int nrf_warp_points_workspace_bytes(nrf_handle h, int32_t num_points, size_t* bytes) {
  if (!h || !bytes) return fail(NRF_E_NULL, "null");
  if (!h->warp) return fail(NRF_E_UNSUPPORTED, "model has no warp field");
  if (num_points <= 0) return fail(NRF_E_SHAPE, "num_points must be positive");
  *bytes = warp_points_plan(h, num_points).total_f * sizeof(float);
  return NRF_OK;
}

int nrf_warp_points(nrf_handle h, const float* params, const float* points, const int32_t* warp_ids, int32_t num_points,
                    const nrf_step_scalars* scalars, float* warped, void* workspace, size_t workspace_bytes, void* stream) {
  if (!h || !params || !points || !warp_ids || !scalars || !warped || !workspace) return fail(NRF_E_NULL, "null argument");
  if (!h->warp) return fail(NRF_E_UNSUPPORTED, "model has no warp field");
  if (h->time_enc) return fail(NRF_E_UNSUPPORTED, "nrf_warp_points takes warp ids: not built for the time encoder");
  if (num_points <= 0) return fail(NRF_E_SHAPE, "num_points must be positive");
  query_device(h);
  const WarpPointsPlan q = warp_points_plan(h, num_points);
  if (workspace_bytes < q.total_f * sizeof(float)) return fail(NRF_E_WORKSPACE, "workspace too small (nrf_warp_points_workspace_bytes)");
  float* ws = (float*)workspace;
  hipStream_t st = (hipStream_t)stream;
  const bool padded = q.ip_f != 0;
  if (padded) {
    hipError_t e0 = hipMemcpyAsync(ws + q.emb_f, h->emb.data(), h->emb.size() * sizeof(EmbedDesc), hipMemcpyHostToDevice, st);
    if (e0 != hipSuccess) return fail_hip(e0, "upload embed table");
    e0 = hipMemsetAsync(ws + q.ip_f, 0, (size_t)h->nparams * sizeof(float), st);
    if (e0 != hipSuccess) return fail_hip(e0, "zero padded params");
    launch_embed(reinterpret_cast<const EmbedDesc*>(ws + q.emb_f), (int)h->emb.size(), params, ws + q.ip_f, true, st);
    params = ws + q.ip_f;
  }
  const WarpParamOffsets& wo = padded ? h->wpo : h->xwpo;   // else the caller's buffer: external offsets
  if (h->wp_pack.empty() || h->wp_pack_base != (int64_t)q.wpk_f) {
    h->wp_pack.clear();
    warp_pack_descs(h, wo, (int64_t)q.wpk_f, false, h->wp_pack);
    h->wp_pack_base = (int64_t)q.wpk_f;
  }
  hipError_t e = hipMemcpyAsync(ws + q.desc_f, h->wp_pack.data(), h->wp_pack.size() * sizeof(PackDesc), hipMemcpyHostToDevice, st);
  if (e != hipSuccess) return fail_hip(e, "upload warp pack table");
  launch_pack(reinterpret_cast<const PackDesc*>(ws + q.desc_f), (int)h->wp_pack.size(), params, ws, st);
  WarpFwdArgs a = warp_points_args(h, params, wo, ws + q.wpk_f, scalars, points, warp_ids, num_points, ws + q.out_f);
  e = hipMemsetAsync(ws + q.ctr_f, 0, 16 * sizeof(int), st);
  if (e != hipSuccess) return fail_hip(e, "zero tile counter");
  a.tile_counter = tile_counter_or_null(ws + q.ctr_f, 0);
  launch_warp_fwd(a, nullptr, false, tile_grid(a.ntiles, 2, h->num_cus), st);
  e = hipMemcpyAsync(warped, ws + q.out_f, (size_t)num_points * 3 * sizeof(float), hipMemcpyDeviceToDevice, st);
  if (e != hipSuccess) return fail_hip(e, "copy warped points");
  return check_launch("nrf_warp_points");
}

// ---- Field queries (nrf_query_points / nrf_query_grid): render_samples up to the activations (models.py:230-277) at the
// caller's points.  A plan of their own in the style of warp_points_plan: h->plan is neither read nor written, so a ray plan's
// digest and a pending nrf_backward are as they were.  The one exception: a query handed the very memory a ray plan's tables or
// stash live in overwrites them, so it forgets that upload / stash (h->uploaded_ws, h->stashed_ws) instead of leaving them stale.
// Workspace:
// [pack descriptors | embed table | padded params | forward image of one MLP | SE3 trunk image | tile counters |
//  cond, condterm, alpha_ct of G groups | grid points | per-point code rows | warped points | out4]
namespace {
struct QueryPlan { size_t desc_f, emb_f, ip_f, wpk_f, wwpk_f, ctr_f, cond_f, condterm_f, alpha_ct_f, points_f, ids_f, wpoints_f, out4_f, total_f; int N, ntiles; };
constexpr int QUERY_MAX_DESCS = 32;   // 11 + rgb branch layers 1..3 + 7 of the SE3 trunk
QueryPlan query_plan(const nrf_handle_s* h, int G, int S) {
  QueryPlan q;
  q.N = G * S;
  q.ntiles = (q.N + TILE_ROWS - 1) / TILE_ROWS;
  const size_t rows_pad = (size_t)q.ntiles * TILE_ROWS;
  size_t o = 0;
  auto take = [&](size_t f) { size_t r = o; o = align_up(o + f, ALIGN_F); return r; };
  q.desc_f = take(QUERY_MAX_DESCS * sizeof(PackDesc) / 4);
  q.emb_f = q.ip_f = 0;
  if (h->embed) {   // a model narrower than the kernels runs on its zero-padded image
    q.emb_f = take((h->emb.size() + 1) * sizeof(EmbedDesc) / 4);
    q.ip_f = take((size_t)h->nparams);
  }
  q.wpk_f = take(h->pk.total);
  q.wwpk_f = h->warp ? take(h->wpk.total) : 0;
  q.ctr_f = take(16);
  q.cond_f = take((size_t)G * (h->R > 0 ? h->R : 1));
  q.condterm_f = take((size_t)G * RGB_W);
  q.alpha_ct_f = take((size_t)G);
  q.points_f = take(rows_pad * 3);   // nrf_query_grid forms its points here
  q.ids_f = q.wpoints_f = 0;
  if (h->warp) {
    q.ids_f = take(rows_pad);
    q.wpoints_f = take(rows_pad * 3);
  }
  q.out4_f = take(rows_pad * 4);
  q.total_f = o;
  return q;
}

// the flag word of a query: 0 or NRF_FLAG_NO_WARP; every other bit by its name
int query_flags(uint32_t flags) {
  static const struct { uint32_t bit; const char* name; } named[] = {
      {NRF_FLAG_TRAIN, "NRF_FLAG_TRAIN"}, {NRF_FLAG_BF16, "NRF_FLAG_BF16"}, {NRF_FLAG_WARP_JACOBIAN, "NRF_FLAG_WARP_JACOBIAN"},
      {NRF_FLAG_WARP_F32, "NRF_FLAG_WARP_F32"}, {NRF_FLAG_BF16X3, "NRF_FLAG_BF16X3"}, {NRF_FLAG_RAY_GRADS, "NRF_FLAG_RAY_GRADS"},
      {NRF_FLAG_FROZEN, "NRF_FLAG_FROZEN"}};
  for (const auto& f : named)
    if (flags & f.bit) {
      snprintf(g_err, sizeof(g_err), "%s: a field query runs in the float32 mode without a stash; flags: 0 or NRF_FLAG_NO_WARP", f.name);
      return NRF_E_UNSUPPORTED;
    }
  if (flags & ~(uint32_t)NRF_FLAG_NO_WARP) {
    snprintf(g_err, sizeof(g_err), "unknown bits 0x%x in flags; a field query takes 0 or NRF_FLAG_NO_WARP", flags & ~(uint32_t)NRF_FLAG_NO_WARP);
    return NRF_E_UNSUPPORTED;
  }
  return NRF_OK;
}

int query_shape(int G, int S) {
  if (G <= 0) return fail(NRF_E_SHAPE, "num_groups (groups->num_rays) must be positive");
  if (S <= 0) return fail(NRF_E_SHAPE, "points_per_group / count must be positive");
  if ((int64_t)G * S > NRF_QUERY_MAX_POINTS) return fail(NRF_E_SHAPE, "a field query takes at most 1 << 24 points per call (NRF_QUERY_MAX_POINTS)");
  return NRF_OK;
}

// both entries behind their own argument checks; points == nullptr: the grid's, already formed at q.points_f
int query_impl(nrf_handle h, const float* params_x, const nrf_rays* groups, const float* points, int S, int level,
               const nrf_step_scalars* sc, uint32_t flags, const nrf_field_out* out, float* ws, const QueryPlan& q, hipStream_t st) {
  const nrf_model_desc& d = h->d;
  const int G = groups->num_rays, N = q.N;
  const bool warp_on = h->warp && !(flags & NRF_FLAG_NO_WARP);
  const bool full = out->rgb != nullptr;
  Prof& pf = h->prof;
  query_device(h);
  // the caller may hand over memory a ray plan lived in: that plan's tables and stash are gone with this call
  if (h->uploaded_ws == (void*)ws) h->uploaded_ws = nullptr;
  if (h->stashed_ws == (void*)ws) h->stashed_ws = nullptr;
  if (!points) points = ws + q.points_f;
  const float* params = params_x;
  hipError_t e;
  if (h->embed) {
    e = hipMemcpyAsync(ws + q.emb_f, h->emb.data(), h->emb.size() * sizeof(EmbedDesc), hipMemcpyHostToDevice, st);
    if (e != hipSuccess) return fail_hip(e, "upload embed table");
    e = hipMemsetAsync(ws + q.ip_f, 0, (size_t)h->nparams * sizeof(float), st);
    if (e != hipSuccess) return fail_hip(e, "zero padded params");
    launch_embed(reinterpret_cast<const EmbedDesc*>(ws + q.emb_f), (int)h->emb.size(), params_x, ws + q.ip_f, true, st);
    params = ws + q.ip_f;
  }
  // forward image of the asked level at the handle's PackOffsets (the transposed images' room stays unwritten and unread), and the
  // SE3 trunk's.  The offsets do not depend on the number of points: the table is rebuilt when the level changes
  const MlpParamOffsets& po = h->po[level];
  if (h->q_pack_level != level) {
    std::vector<PackDesc>& v = h->q_pack;
    v.clear();
    const PackOffsets& pk = h->pk;
    auto add = [&](int64_t src, int dst, int ld, int row0, int kvalid, int K, int ncb) {
      PackDesc p;
      p.src_off = src; p.dst_off = (int64_t)q.wpk_f + dst; p.src_ld = ld; p.src_row0 = row0; p.kvalid = kvalid; p.K = K; p.ncb = ncb;
      p.transposed = 0; p.nwaves = 4; p.nvalid = 1 << 30;
      v.push_back(p);
    };
    add(po.trunk_k[0], pk.fwd_L[0], 256, 0, h->P, h->PK, 2);
    for (int l = 1; l < TRUNK_DEPTH; ++l) add(po.trunk_k[l], pk.fwd_L[l], 256, 0, 256, 256, 2);
    add(po.trunk_k[d.nerf_skip_layer], pk.fwd_L4b, 256, 256, h->P, h->PK, 2);
    add(po.bn_k, pk.fwd_bn, 256, 0, 256, 256, 2);
    add(po.rgbh_k, pk.fwd_rgbh, 128, 0, 256, 256, 1);
    for (int x = 0; x < d.nerf_rgb_branch_depth - 1; ++x) add(po.rgbx_k[x], pk.fwd_rgbx + x * RGB_W * RGB_W, 128, 0, 128, 128, 1);
    if (h->warp) warp_pack_descs(h, h->wpo, (int64_t)q.wwpk_f, false, v);
    h->q_pack_level = level;
  }
  if ((int)h->q_pack.size() > QUERY_MAX_DESCS) return fail(NRF_E_STATE, "field query: pack table larger than its workspace region");
  e = hipMemcpyAsync(ws + q.desc_f, h->q_pack.data(), h->q_pack.size() * sizeof(PackDesc), hipMemcpyHostToDevice, st);
  if (e != hipSuccess) return fail_hip(e, "upload query pack table");
  if (tile_counter_or_null(ws + q.ctr_f, 0)) {   // NRF_DYNAMIC_TILES experiment only
    e = hipMemsetAsync(ws + q.ctr_f, 0, 16 * sizeof(int), st);
    if (e != hipSuccess) return fail_hip(e, "zero tile counters");
  }
  pf.begin("query_prep", 0, st);   // no return between a begin and its end
  launch_pack(reinterpret_cast<const PackDesc*>(ws + q.desc_f), (int)h->q_pack.size(), params, ws, st);
  // per-group terms (models.py:186-228): the full query's condition term; the density-only query of a use_alpha_condition model
  // needs the appearance code's term of the alpha head alone, so ray_prep runs on the appearance columns only (same kernel, same
  // fmaf chain: the same alpha_ct bits) and no view direction or camera code is read
  if (full || h->A > 0) {
    RayPrepArgs ra;
    memset(&ra, 0, sizeof(ra));
    ra.params = params; ra.cond = ws + q.cond_f; ra.viewdirs = groups->viewdirs;
    ra.app_ids = groups->appearance_codes ? nullptr : groups->appearance_ids; ra.app_codes = groups->appearance_codes;
    ra.B = G; ra.app_feat = h->A; ra.app_off = h->app_off; ra.R = h->A;
    if (full) {
      ra.cam_ids = groups->camera_codes ? nullptr : groups->camera_ids; ra.cam_codes = groups->camera_codes;
      ra.Fv = d.num_nerf_viewdir_freqs; ra.use_viewdirs = d.use_viewdirs;
      ra.cam_feat = d.use_camera_metadata ? d.num_camera_features : 0; ra.cam_off = h->cam_off; ra.R = h->R;
    }
    ra.rgbh_k[0] = po.rgbh_k; ra.rgbh_b[0] = po.rgbh_b; ra.alpha_k[0] = po.alpha_k;
    ra.condterm[0] = ws + q.condterm_f; ra.alpha_ct[0] = h->A > 0 ? ws + q.alpha_ct_f : nullptr;
    launch_ray_prep(ra, st);
  }
  pf.end(st);
  if (warp_on) {
    // per-point rows of the code table: group g's id, or row g of the caller's codes (metadata_encoded).  The SE3 kernel has two
    // prologues: `row / S` ids together with x = o + z d formed from rays, or explicit points together with ONE ID PER POINT
    // (warp_chain.hip: points_in -> point_ids[r]); explicit points with per-group ids is neither, and giving the kernel a third
    // would change a kernel every plan runs.  So the ids are written out: 4 bytes per row next to a trunk of 1.6e5 MACs, below
    // the resolution of the 128^3 measurement (profiles/field_query.md)
    int32_t* ids = reinterpret_cast<int32_t*>(ws + q.ids_f);
    launch_field_ids(groups->warp_codes ? nullptr : groups->warp_ids, N, S, ids, st);
    WarpFwdArgs wa = warp_points_args(h, params, h->wpo, ws + q.wwpk_f, sc, points, ids, N, ws + q.wpoints_f);
    if (groups->warp_codes) wa.embed_table = groups->warp_codes;
    wa.tile_counter = tile_counter_or_null(ws + q.ctr_f, 0);
    const double Wi = h->Win;
    pf.begin("query_warp", 2.0 * (Wi * 128 + 3 * 16384.0 + (128 + Wi) * 128 + 16384.0 + 128 * 6) * N, st);
    launch_warp_fwd(wa, nullptr, false, tile_grid(wa.ntiles, warp_grid_mul(), h->num_cus), st);
    pf.end(st);
    points = ws + q.wpoints_f;
  }
  ChainFwdArgs a;
  memset(&a, 0, sizeof(a));
  a.params = params; a.po = po; a.wpk = ws + q.wpk_f; a.pk = h->pk;
  a.condterm = ws + q.condterm_f; a.points = points; a.out4 = reinterpret_cast<float4*>(ws + q.out4_f);
  a.S = S; a.B = G; a.rows = N; a.ntiles = q.ntiles;
  a.F = d.num_nerf_point_freqs; a.P = h->P; a.PK = h->PK; a.sigma_act = d.sigma_activation; a.skip = d.nerf_skip_layer;
  a.tile_counter = tile_counter_or_null(ws + q.ctr_f, 1);
  a.alpha_ct = h->A > 0 ? ws + q.alpha_ct_f : nullptr;
  a.nx = d.nerf_rgb_branch_depth - 1;
  // the full query picks its tiling as a forward launch of this many tiles does (nrf_run.hip Forward::mlp); the density chain is
  // built on 64-row tiles only (chain_query.hip)
  const bool c32 = full && chain32_for(h, q.ntiles);
  const int grid = c32 ? tile_grid(2 * q.ntiles, 4, h->num_cus) : tile_grid(q.ntiles, knobs().grid_mul, h->num_cus);
  a.k_old = k_old_for(q.ntiles, grid, h->num_cus, 0.0);
  const double P = h->P, trunk = P * 256 + 6 * 65536.0 + (256 + P) * 256 + 256;   // MACs per row: trunk + alpha head
  if (full) {
    pf.begin("query_mlp", 2.0 * (trunk + 65536.0 + (256.0 + h->R) * 128 + 128 * 3 + 16384.0 * a.nx) * N, st);
    if (c32) launch_chain_fwd32(a, false, grid, st);
    else launch_chain_fwd(a, false, grid, st);
    pf.end(st);
    pf.begin("query_unpack", 0, st);
    launch_field_unpack(a.out4, N, out->sigma, out->rgb, st);
    pf.end(st);
  } else if (out->sigma) {
    pf.begin("query_density", 2.0 * (trunk + (h->A > 0 ? 65536.0 : 0.0)) * N, st);
    launch_chain_density(a, out->sigma, grid, st);
    pf.end(st);
  }
  if (out->warped_points) {
    e = hipMemcpyAsync(out->warped_points, ws + q.wpoints_f, (size_t)N * 3 * sizeof(float), hipMemcpyDeviceToDevice, st);
    if (e != hipSuccess) return fail_hip(e, "copy warped points");
  }
  return check_launch("nrf_query_points");
}

// what both entries check of everything but the points
int query_args(nrf_handle h, const float* params, const nrf_rays* groups, int S, int level, const nrf_step_scalars* sc, uint32_t flags,
               const nrf_field_out* out, const void* workspace) {
  if (!h) return fail(NRF_E_NULL, "handle is null");
  if (!params) return fail(NRF_E_NULL, "params is null");
  if (!groups) return fail(NRF_E_NULL, "groups is null");
  if (!sc) return fail(NRF_E_NULL, "scalars (nrf_step_scalars) is null");
  if (!out) return fail(NRF_E_NULL, "out (nrf_field_out) is null");
  if (!workspace) return fail(NRF_E_NULL, "workspace is null");
  CK(query_flags(flags));
  CK(query_shape(groups->num_rays, S));
  if (level != 0 && level != 1) return fail(NRF_E_SHAPE, "level must be 0 (coarse) or 1 (fine)");
  if (level >= h->nlevels) return fail(NRF_E_SHAPE, "level = 1: the model has no fine level (num_fine_samples == 0)");
  const bool warp_on = h->warp && !(flags & NRF_FLAG_NO_WARP);
  if (out->warped_points && !warp_on)
    return fail(NRF_E_UNSUPPORTED, "the warped_points output needs the warp field (a model with use_warp, no NRF_FLAG_NO_WARP)");
  if (warp_on && h->time_enc)
    return fail(NRF_E_UNSUPPORTED, "a field query takes warp ids or codes: not built for the time encoder with the warp on (NRF_FLAG_NO_WARP runs)");
  if (out->rgb && h->d.use_viewdirs && !groups->viewdirs)
    return fail(NRF_E_UNSUPPORTED, "out->rgb on a use_viewdirs model needs groups->viewdirs (a point has no direction to fall back on)");
  if (out->rgb && h->d.use_camera_metadata && !groups->camera_ids && !groups->camera_codes)
    return fail(NRF_E_NULL, "camera_ids (or camera_codes) required (use_camera_metadata)");
  if ((out->rgb || out->sigma) && h->app_in_cond && !groups->appearance_ids && !groups->appearance_codes)
    return fail(NRF_E_NULL, "appearance_ids (or appearance_codes) required");
  if (warp_on && !groups->warp_ids && !groups->warp_codes) return fail(NRF_E_NULL, "warp_ids (or warp_codes) required (use_warp)");
  return NRF_OK;
}
}  // namespace

int nrf_query_workspace_bytes(nrf_handle h, int32_t num_groups, int32_t points_per_group, uint32_t flags, size_t* bytes) {
  if (!h || !bytes) return fail(NRF_E_NULL, "handle / bytes is null");
  CK(query_flags(flags));
  CK(query_shape(num_groups, points_per_group));
  *bytes = query_plan(h, num_groups, points_per_group).total_f * sizeof(float);
  return NRF_OK;
}

int nrf_query_points(nrf_handle h, const float* params, const nrf_rays* groups, const float* points, int32_t points_per_group,
                     int32_t level, const nrf_step_scalars* scalars, uint32_t flags, const nrf_field_out* out, void* workspace,
                     size_t workspace_bytes, void* stream) {
  if (h && !points) return fail(NRF_E_NULL, "points is null");
  CK(query_args(h, params, groups, points_per_group, level, scalars, flags, out, workspace));
  const QueryPlan q = query_plan(h, groups->num_rays, points_per_group);
  if (workspace_bytes < q.total_f * sizeof(float)) return fail(NRF_E_WORKSPACE, "workspace too small (see nrf_query_workspace_bytes)");
  return query_impl(h, params, groups, points, points_per_group, level, scalars, flags, out, (float*)workspace, q, (hipStream_t)stream);
}

int nrf_query_grid(nrf_handle h, const float* params, const nrf_rays* group, const nrf_grid* grid, int64_t first, int32_t count,
                   int32_t level, const nrf_step_scalars* scalars, uint32_t flags, const nrf_field_out* out, void* workspace,
                   size_t workspace_bytes, void* stream) {
  if (h && !grid) return fail(NRF_E_NULL, "grid is null");
  CK(query_args(h, params, group, count, level, scalars, flags, out, workspace));
  if (group->num_rays != 1) return fail(NRF_E_SHAPE, "nrf_query_grid: group->num_rays must be 1 (one condition for the whole grid)");
  if (grid->dims[0] <= 0 || grid->dims[1] <= 0 || grid->dims[2] <= 0) return fail(NRF_E_SHAPE, "grid dims must be positive");
  // at most 2^40 points in a grid: the product of three int32 extents cannot wrap int64 behind this
  const int64_t plane = (int64_t)grid->dims[0] * grid->dims[1];
  if (plane > NRF_GRID_MAX_POINTS || plane * grid->dims[2] > NRF_GRID_MAX_POINTS)
    return fail(NRF_E_SHAPE, "grid dims: more than NRF_GRID_MAX_POINTS (1 << 40) points in dims[0] * dims[1] * dims[2]");
  const int64_t total = plane * grid->dims[2];
  if (first < 0 || first + count > total) return fail(NRF_E_SHAPE, "first + count runs beyond the grid (dims[0] * dims[1] * dims[2] points)");
  const QueryPlan q = query_plan(h, 1, count);
  if (workspace_bytes < q.total_f * sizeof(float)) return fail(NRF_E_WORKSPACE, "workspace too small (see nrf_query_workspace_bytes)");
  query_device(h);
  launch_grid_points(*grid, first, count, (float*)workspace + q.points_f, (hipStream_t)stream);
  return query_impl(h, params, group, nullptr, count, level, scalars, flags, out, (float*)workspace, q, (hipStream_t)stream);
}

int nrf_set_option(nrf_handle h, int32_t option, int64_t value) {
  if (!h) return fail(NRF_E_NULL, "handle is null");
  if (option == NRF_OPT_CHAIN_TILE_ROWS) {
    if (value != 0 && value != 32 && value != 64) return fail(NRF_E_UNSUPPORTED, "NRF_OPT_CHAIN_TILE_ROWS: 0 (automatic), 32 or 64");
    if (value == 32 && h->d.nerf_rgb_branch_depth > 1)
      return fail(NRF_E_UNSUPPORTED, "NRF_OPT_CHAIN_TILE_ROWS = 32: the 32-row chains run an rgb branch of one layer; a model with "
                                     "nerf_rgb_branch_depth > 1 keeps the 64-row kernels at every launch size");
    if (h->chain_rows_opt != (int)value) {
      h->chain_rows_opt = (int)value;
      h->stashed_ws = nullptr;   // a stash written under the old plan is not differentiated under the new one
    }
    return NRF_OK;
  }
  if (option == NRF_OPT_BF16_WGRAD_MERGE) {
    if (value != 0 && value != 1) return fail(NRF_E_UNSUPPORTED, "NRF_OPT_BF16_WGRAD_MERGE: 0 or 1");
    if (h->bf16_wgrad_merge != (int)value) {
      h->bf16_wgrad_merge = (int)value;
      h->stashed_ws = nullptr;
    }
    return NRF_OK;
  }
  return fail(NRF_E_UNSUPPORTED, "unknown option");
}

int nrf_profile_enable(nrf_handle h, int32_t on) {
  if (!h) return fail(NRF_E_NULL, "handle is null");
  h->prof.drain();
  h->prof.acc.clear();
  h->prof.on = on != 0;
  return NRF_OK;
}

int nrf_profile_read(nrf_handle h, nrf_profile_entry* out, int32_t* n) {
  if (!h || !n) return fail(NRF_E_NULL, "null");
  h->prof.drain();
  const int32_t cnt = (int32_t)h->prof.acc.size();
  if (out) {
    if (*n < cnt) return fail(NRF_E_SHAPE, "profile array too small");
    for (int32_t i = 0; i < cnt; ++i) {
      memset(&out[i], 0, sizeof(out[i]));
      snprintf(out[i].name, sizeof(out[i].name), "%s", h->prof.acc[i].name.c_str());
      out[i].ms = h->prof.acc[i].ms; out[i].launches = h->prof.acc[i].launches; out[i].flops_per_launch = h->prof.acc[i].flops;
    }
    h->prof.acc.clear();
  }
  *n = cnt;
  return NRF_OK;
}

int nrf_debug_ws_offset(nrf_handle h, const char* name, int32_t level, int64_t* float_offset) {
  if (!h || !name || !float_offset) return fail(NRF_E_NULL, "null");
  if (level < 0 || level > 3 || h->plan.key.B < 0) return fail(NRF_E_STATE, "no workspace plan yet / bad level");
  const LevelWs& L = h->plan.L[level];
  const struct { const char* n; size_t v; } tab[] = {
      {"st_pe", L.st_pe}, {"st_h", L.st_h}, {"st_bn", L.st_bn}, {"st_rgbh", L.st_rgbh}, {"dy_trunk", L.dy_trunk},
      {"dy_bn", L.dy_bn}, {"dy_rgbh", L.dy_rgbh}, {"d_raw4", L.d_raw4}, {"z", L.z}, {"out4", L.out4},
      {"wpoints", L.wpoints}, {"d_points", L.d_points}, {"w_st_win", L.w_st_win}, {"w_st_h", L.w_st_h},
      {"w_st_wv", L.w_st_wv}, {"w_dy", L.w_dy}, {"w_dw4", L.w_dw4}, {"w_dv4", L.w_dv4},
      {"w_bits", L.w_bits}, {"bits_trunk", L.bits_trunk}, {"bits_rgbh", L.bits_rgbh},
      {"st_rgbx", L.st_rgbx}, {"bits_rgbx", L.bits_rgbx}, {"dy_rgbx", L.dy_rgbx},   // rgb branch layers 1..D-1, [D-1][ntiles]...
      {"b_pe", L.b_pe}, {"b_h", L.b_h}, {"b_bn", L.b_bn}, {"b_rgbh", L.b_rgbh}, {"b_bits", L.b_bits}, {"b_dy", L.b_dy},
      {"b_dbn", L.b_dbn}, {"b_drgbh", L.b_drgbh}, {"b_dsmall", L.b_dsmall},
      {"bw_in", L.bw_in}, {"bw_h", L.bw_h}, {"bw_bits", L.bw_bits}, {"bw_dy", L.bw_dy}, {"bw_dhead", L.bw_dhead},
      {"points_raw", L.points_raw},
      {"bg_points", h->plan.bg_points}, {"bg_ids", h->plan.bg_ids},
      {"timeline", h->plan.timeline + (size_t)(level & 1) * TIMELINE_LEVEL_F}};
  for (const auto& t : tab)
    if (!strcmp(t.n, name)) { *float_offset = (int64_t)t.v; return NRF_OK; }
  return fail(NRF_E_SHAPE, "unknown workspace buffer name");
}

// FNV-1a over everything of the plan that reaches the device or a launch, field by field (LevelWs has padding; serial and the
// host-side bf_stream_ok guard stay out)
int nrf_debug_plan_digest(nrf_handle h, uint64_t* digest) {
  if (!h || !digest) return fail(NRF_E_NULL, "null");
  const WsPlan& p = h->plan;
  if (p.key.B < 0) return fail(NRF_E_STATE, "no workspace plan yet");
  uint64_t x = 0xcbf29ce484222325ull;
  auto bytes = [&](const void* v, size_t n) {
    for (size_t i = 0; i < n; ++i) x = (x ^ static_cast<const unsigned char*>(v)[i]) * 0x100000001b3ull;
  };
  auto put = [&](auto v) { bytes(&v, sizeof(v)); };
  auto vec = [&](const auto& v) { put((uint64_t)v.size()); bytes(v.data(), v.size() * sizeof(v[0])); };
  put(p.key.B); put(p.key.flags); put(p.key.bgN); put(p.key.elastic); put(p.key.chain_rows_opt); put(p.key.bf16_wgrad_merge);
  put(p.total_floats);
  for (int i = 0; i < 4; ++i) { put(p.S[i]); put(p.rows[i]); put(p.ntiles[i]); }
  put(p.bwd32); put(p.bfw); put(p.tg_tiles_per); put(p.wgrad_nwg); put(p.bwgrad_nwg);
  for (int i = 0; i < 4; ++i) put(p.nreduce_pass[i]);
  for (size_t v : {p.tables, p.bf_desc, p.bfw_wpk, p.bfw_wpkT, p.iparams, p.igrad, p.cond, p.mse, p.zero_rgb, p.warp_wpk, p.bg_loss,
                   p.bg_points, p.bg_ids, p.el_sums, p.el_coef, p.wr_sums, p.t_codes, p.t_dcodes, p.t_in, p.t_h, p.t_dpre, p.counters,
                   p.timeline, p.seg_clock})
    put(v);
  for (const LevelWs& L : p.L) {
    for (size_t v : {L.wpk, L.z, L.out4, L.rgb, L.depth, L.med, L.acc, L.weights, L.condterm, L.alpha_ct, L.dsig_ray, L.bf_wpk,
                     L.bf_wpkT, L.b_pe, L.b_h, L.b_bn, L.b_rgbh, L.b_bits, L.b_dy, L.b_dbn, L.b_drgbh, L.b_dsmall})
      put(v);
    put(L.b_ngroups);
    for (size_t v : {L.bw_in, L.bw_h, L.bw_bits, L.bw_dy, L.bw_dhead}) put(v);
    put(L.bw_ngroups);
    for (size_t v : {L.st_pe, L.st_h, L.st_bn, L.st_rgbh, L.bits_trunk, L.bits_rgbh, L.d_raw4, L.dy_trunk, L.dy_bn, L.dy_rgbh, L.dray,
                     L.small_part, L.cond_grad, L.wpoints, L.points_raw, L.d_points, L.el_dw4, L.el_dv4, L.w_st_win, L.w_st_h,
                     L.w_st_wv, L.w_bits, L.w_dy, L.w_dw4, L.w_dv4, L.w_small_part})
      put(v);
  }
  for (size_t v : {p.pack_off_b, p.groups_off_b, p.reduce_off_b, p.segs_off_b, p.segbegin_off_b, p.emb_off_b, p.bgroups_off_b,
                   p.bsegs_off_b, p.bsegbegin_off_b})
    put(v);
  vec(p.pack); vec(p.bfpack); vec(p.groups); vec(p.bgroups); vec(p.segs); vec(p.seg_begin); vec(p.bsegs); vec(p.bseg_begin);
  vec(p.reduce);
  *digest = x;
  return NRF_OK;
}

int nrf_debug_wgrad_segments(nrf_handle h, const void* workspace, double* out, int32_t* n) {
  if (!h || !n) return fail(NRF_E_NULL, "null");
  const WsPlan& p = h->plan;
  const int32_t cnt = (int32_t)p.segs.size();
  if (out) {
    if (*n < cnt || !workspace) return fail(NRF_E_SHAPE, "segment array too small / workspace null");
    std::vector<unsigned long long> clk(cnt);
    hipError_t e = hipMemcpy(clk.data(), (const float*)workspace + p.seg_clock, cnt * sizeof(unsigned long long), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail_hip(e, "read segment clocks");
    int wg = 0;
    for (int32_t i = 0; i < cnt; ++i) {
      while (wg + 1 < (int)p.seg_begin.size() && p.seg_begin[wg + 1] <= i) ++wg;
      const WgradGroup& g = p.groups[p.segs[i].group];
      out[6 * i + 0] = wg; out[6 * i + 1] = p.segs[i].group; out[6 * i + 2] = g.Kb; out[6 * i + 3] = g.Nb;
      out[6 * i + 4] = p.segs[i].tile_end - p.segs[i].tile_begin; out[6 * i + 5] = (double)clk[i];
    }
  }
  *n = cnt;
  return NRF_OK;
}

int nrf_adam_step(float* params, float* m, float* v, const float* grad, int64_t n, double lr, double beta1, double beta2,
                  double eps, int64_t step, double grad_scale, void* stream) {
  if (!params || !m || !v || !grad) return fail(NRF_E_NULL, "null argument");
  if (n <= 0) return fail(NRF_E_SHAPE, "n must be positive");
  launch_adam(params, m, v, grad, n, lr, beta1, beta2, eps, step, grad_scale, (hipStream_t)stream);
  return check_launch("nrf_adam_step");
}

int nrf_dynamic_scalars_write(nrf_dynamic_scalars* device_dst, const nrf_dynamic_scalars* host_values, void* stream) {
  if (!device_dst || !host_values) return fail(NRF_E_NULL, "null argument");
  launch_dynamic_write(device_dst, *host_values, (hipStream_t)stream);
  return check_launch("nrf_dynamic_scalars_write");
}

int nrf_adam_step_dynamic(float* params, float* m, float* v, const float* grad, int64_t n, double beta1, double beta2, double eps,
                          const nrf_dynamic_scalars* dynamic, void* stream) {
  if (!params || !m || !v || !grad || !dynamic) return fail(NRF_E_NULL, "null argument");
  if (n <= 0) return fail(NRF_E_SHAPE, "n must be positive");
  launch_adam_dynamic(params, m, v, grad, n, beta1, beta2, eps, dynamic, (hipStream_t)stream);
  return check_launch("nrf_adam_step_dynamic");
}

int nrf_sample_along_rays(const float* origins, const float* directions, int32_t num_rays, int32_t num_samples,
                          float near_plane, float far_plane, int32_t stratified, int32_t linear_disparity,
                          const float* t_rand, uint64_t seed, uint64_t offset, float* z_vals, void* stream) {
  (void)origins; (void)directions;   // z_vals do not depend on the ray; points are formed inside the MLP kernel
  if (!z_vals) return fail(NRF_E_NULL, "z_vals is null");
  if (num_rays <= 0 || num_samples < 2) return fail(NRF_E_SHAPE, "bad shape");
  launch_sample_coarse(t_rand, num_rays, num_samples, near_plane, far_plane, stratified, linear_disparity, seed, offset,
                       nullptr, z_vals, (hipStream_t)stream);
  return check_launch("nrf_sample_along_rays");
}

int nrf_volumetric_rendering(const float* rgb_sigma, const float* z_vals, const float* directions, int32_t num_rays,
                             int32_t num_samples, int32_t white_background, int32_t sample_at_infinity,
                             const nrf_level_out* out, void* stream) {
  if (!rgb_sigma || !z_vals || !directions || !out) return fail(NRF_E_NULL, "null argument");
  if (num_rays <= 0 || num_samples < 1 || num_samples > 512) return fail(NRF_E_SHAPE, "num_samples must be in [1,512]");
  launch_composite_fwd(reinterpret_cast<const float4*>(rgb_sigma), z_vals, directions, num_rays, num_samples,
                       white_background, sample_at_infinity, out->rgb, out->depth, out->med_depth, out->acc, out->weights,
                       (hipStream_t)stream);
  return check_launch("nrf_volumetric_rendering");
}

int nrf_sample_pdf(const float* z_coarse, const float* weights_coarse, int32_t num_rays, int32_t num_coarse,
                   int32_t num_fine, int32_t stratified, const float* u, uint64_t seed, uint64_t offset, float* z_out,
                   void* stream) {
  if (!z_coarse || !weights_coarse || !z_out) return fail(NRF_E_NULL, "null argument");
  if (num_rays <= 0 || num_coarse < 3 || num_coarse > 256 || num_fine < 1 || num_coarse + num_fine > 512)
    return fail(NRF_E_SHAPE, "need 3 <= num_coarse <= 256 and num_coarse + num_fine <= 512");
  launch_sample_fine(z_coarse, weights_coarse, num_rays, num_coarse, num_fine, stratified, u, seed, offset, nullptr, z_out,
                     (hipStream_t)stream);
  return check_launch("nrf_sample_pdf");
}

namespace {
int camera_args(const nrf_camera* cam, CameraArgs* c) {
  if (!cam) return fail(NRF_E_NULL, "camera is null");
  if (!(cam->focal_length > 0.f) || !(cam->pixel_aspect_ratio > 0.f))
    return fail(NRF_E_SHAPE, "focal_length and pixel_aspect_ratio must be positive");
  if (cam->image_size[0] <= 0 || cam->image_size[1] <= 0) return fail(NRF_E_SHAPE, "image_size must be positive");
  for (int i = 0; i < 9; ++i) c->R[i] = cam->orientation[i];
  for (int i = 0; i < 3; ++i) c->pos[i] = cam->position[i];
  c->focal = cam->focal_length;
  c->cx = cam->principal_point[0];
  c->cy = cam->principal_point[1];
  c->skew = cam->skew;
  c->aspect = cam->pixel_aspect_ratio;
  c->k1 = cam->radial_distortion[0];
  c->k2 = cam->radial_distortion[1];
  c->k3 = cam->radial_distortion[2];
  c->p1 = cam->tangential_distortion[0];
  c->p2 = cam->tangential_distortion[1];
  c->width = cam->image_size[0];
  c->height = cam->image_size[1];
  // has_radial_distortion or has_tangential_distortion (camera.py:232): the solver is skipped, not run to a no-op
  c->distorted = (c->k1 != 0.f || c->k2 != 0.f || c->k3 != 0.f || c->p1 != 0.f || c->p2 != 0.f) ? 1 : 0;
  return NRF_OK;
}
bool aligned8(const void* p) { return ((uintptr_t)p & 7u) == 0; }
}  // namespace

int nrf_camera_pixels_to_rays(const nrf_camera* camera, const float* pixels, int64_t n, float* origins,
                              float* directions, float* pixels_out, void* stream) {
  CameraArgs c;
  CK(camera_args(camera, &c));
  if (!directions) return fail(NRF_E_NULL, "directions is null");
  if (n <= 0) return fail(NRF_E_SHAPE, "n must be positive");
  if (!pixels && n != (int64_t)c.width * c.height)
    return fail(NRF_E_SHAPE, "pixels == NULL renders the pixel centres: n must equal width*height");
  if (!aligned8(pixels) || !aligned8(pixels_out)) return fail(NRF_E_SHAPE, "pixel buffers must be 8-byte aligned");
  launch_camera_rays(c, pixels, nullptr, (long)n, origins, directions, pixels_out, (hipStream_t)stream);
  return check_launch("nrf_camera_pixels_to_rays");
}

int nrf_camera_pixels_to_points(const nrf_camera* camera, const float* pixels, const float* depth, int64_t n,
                                float* points, void* stream) {
  CameraArgs c;
  CK(camera_args(camera, &c));
  if (!pixels || !depth || !points) return fail(NRF_E_NULL, "pixels / depth / points is null");
  if (n <= 0) return fail(NRF_E_SHAPE, "n must be positive");
  if (!aligned8(pixels)) return fail(NRF_E_SHAPE, "pixel buffers must be 8-byte aligned");
  launch_camera_rays(c, pixels, depth, (long)n, nullptr, points, nullptr, (hipStream_t)stream);
  return check_launch("nrf_camera_pixels_to_points");
}

int nrf_camera_project(const nrf_camera* camera, const float* points, int64_t n, float* pixels, void* stream) {
  CameraArgs c;
  CK(camera_args(camera, &c));
  if (!points || !pixels) return fail(NRF_E_NULL, "points / pixels is null");
  if (n <= 0) return fail(NRF_E_SHAPE, "n must be positive");
  if (!aligned8(pixels)) return fail(NRF_E_SHAPE, "pixel buffers must be 8-byte aligned");
  launch_camera_project(c, points, (long)n, pixels, (hipStream_t)stream);
  return check_launch("nrf_camera_project");
}

namespace {
bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }
// what every camera-table entry point checks before any HIP call
int table_args(const float* cameras, int32_t num_cameras, int64_t n) {
  if (!cameras) return fail(NRF_E_NULL, "cameras is null");
  if (num_cameras <= 0) return fail(NRF_E_SHAPE, "num_cameras must be positive");
  if (n < 0 || n > INT32_MAX) return fail(NRF_E_SHAPE, "n must be in [0, INT32_MAX]");
  if (!aligned16(cameras)) return fail(NRF_E_SHAPE, "the camera table must be 16-byte aligned");
  return NRF_OK;
}
int table_workspace_args(int64_t n, const void* workspace, size_t workspace_bytes) {
  if (!workspace) return fail(NRF_E_NULL, "workspace is null");
  if (!aligned16(workspace)) return fail(NRF_E_SHAPE, "workspace must be 16-byte aligned");
  if (workspace_bytes < camera_table_workspace_bytes((long)n))
    return fail(NRF_E_WORKSPACE, "workspace too small (see nrf_camera_table_workspace_bytes)");
  return NRF_OK;
}
}  // namespace

int nrf_camera_table_workspace_bytes(int64_t n, int32_t num_cameras, size_t* bytes) {
  if (!bytes) return fail(NRF_E_NULL, "bytes is null");
  if (num_cameras <= 0) return fail(NRF_E_SHAPE, "num_cameras must be positive");
  if (n < 0 || n > INT32_MAX) return fail(NRF_E_SHAPE, "n must be in [0, INT32_MAX]");
  *bytes = camera_table_workspace_bytes((long)n);
  return NRF_OK;
}

int nrf_camera_table_rays(const float* cameras, int32_t num_cameras, const int32_t* camera_index, const float* pixels, int64_t n,
                          float* origins, float* directions, void* stream) {
  CK(table_args(cameras, num_cameras, n));
  if (n == 0) return NRF_OK;   // nothing to do: the per-ray buffers of an empty batch may be NULL
  if (!pixels || !directions) return fail(NRF_E_NULL, "pixels / directions is null");
  if (!aligned8(pixels)) return fail(NRF_E_SHAPE, "pixel buffers must be 8-byte aligned");
  launch_camera_table_rays(cameras, num_cameras, camera_index, pixels, (long)n, origins, directions, (hipStream_t)stream);
  return check_launch("nrf_camera_table_rays");
}

int nrf_camera_table_project(const float* cameras, int32_t num_cameras, const int32_t* camera_index, const float* points, int64_t n,
                             float* pixels, void* stream) {
  CK(table_args(cameras, num_cameras, n));
  if (n == 0) return NRF_OK;
  if (!points || !pixels) return fail(NRF_E_NULL, "points / pixels is null");
  if (!aligned8(pixels)) return fail(NRF_E_SHAPE, "pixel buffers must be 8-byte aligned");
  launch_camera_table_project(cameras, num_cameras, camera_index, points, (long)n, pixels, (hipStream_t)stream);
  return check_launch("nrf_camera_table_project");
}

int nrf_camera_table_rays_backward(const float* cameras, int32_t num_cameras, const int32_t* camera_index, const float* pixels,
                                   int64_t n, const float* d_origins, const float* d_directions, float* d_cameras, float* d_pixels,
                                   void* workspace, size_t workspace_bytes, void* stream) {
  CK(table_args(cameras, num_cameras, n));
  if ((!pixels && n > 0) || !d_cameras) return fail(NRF_E_NULL, "pixels / d_cameras is null");
  if (!aligned8(pixels) || !aligned8(d_pixels)) return fail(NRF_E_SHAPE, "pixel buffers must be 8-byte aligned");
  CK(table_workspace_args(n, workspace, workspace_bytes));
  launch_camera_table_rays_backward(cameras, num_cameras, camera_index, pixels, (long)n, d_origins, d_directions, d_cameras, d_pixels,
                                    workspace, (hipStream_t)stream);
  return check_launch("nrf_camera_table_rays_backward");
}

int nrf_camera_table_project_backward(const float* cameras, int32_t num_cameras, const int32_t* camera_index, const float* points,
                                      int64_t n, const float* d_pixels, float* d_cameras, float* d_points, void* workspace,
                                      size_t workspace_bytes, void* stream) {
  CK(table_args(cameras, num_cameras, n));
  if (((!points || !d_pixels) && n > 0) || !d_cameras) return fail(NRF_E_NULL, "points / d_pixels / d_cameras is null");
  if (!aligned8(d_pixels)) return fail(NRF_E_SHAPE, "pixel buffers must be 8-byte aligned");
  CK(table_workspace_args(n, workspace, workspace_bytes));
  launch_camera_table_project_backward(cameras, num_cameras, camera_index, points, (long)n, d_pixels, d_cameras, d_points, workspace,
                                       (hipStream_t)stream);
  return check_launch("nrf_camera_table_project_backward");
}

int nrf_camera_table_compose(const float* cameras, const float* deltas, int32_t num_cameras, float* out, void* stream) {
  CK(table_args(cameras, num_cameras, 0));
  if (!deltas || !out) return fail(NRF_E_NULL, "deltas / out is null");
  if (!aligned16(deltas) || !aligned16(out)) return fail(NRF_E_SHAPE, "the delta table and the output table must be 16-byte aligned");
  if (out == cameras) return fail(NRF_E_SHAPE, "out may not alias cameras");
  launch_camera_compose(cameras, deltas, num_cameras, out, (hipStream_t)stream);
  return check_launch("nrf_camera_table_compose");
}

int nrf_camera_table_compose_backward(const float* cameras, const float* deltas, int32_t num_cameras, const float* d_cameras,
                                      float* d_deltas, void* stream) {
  CK(table_args(cameras, num_cameras, 0));
  if (!deltas || !d_cameras || !d_deltas) return fail(NRF_E_NULL, "deltas / d_cameras / d_deltas is null");
  if (!aligned16(deltas) || !aligned16(d_cameras) || !aligned16(d_deltas))
    return fail(NRF_E_SHAPE, "the delta table and the gradient tables must be 16-byte aligned");
  launch_camera_compose_backward(cameras, deltas, num_cameras, d_cameras, d_deltas, (hipStream_t)stream);
  return check_launch("nrf_camera_table_compose_backward");
}

}  // extern "C"
