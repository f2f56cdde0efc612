// Launch sequences of the C-ABI layer: forward_impl stands in for NerfModel.apply (models.py:289-375), backward_impl for the gradient
// half of training.train_step (training.py:168-265) incl. the regularisers; both run on the plan nrf_plan.hip built, as a list of
// stages (Forward / Backward below, the pattern of nrf_plan.hip's Planner) over one call's context (Run).  The argument builders in
// front of them also serve the stand-alone field entries (nrf_field.hip).  See nrf_handle.h.
#include "nrf_handle.h"

using namespace nrf;
using namespace nrf::api;

namespace nrf {
namespace api {

int check_launch(const char* where) {
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? NRF_OK : fail_hip(e, where);
}

// what every SE3 forward launch reads of the field itself, whatever points it runs on
static WarpFwdArgs warp_field_args(nrf_handle h, const float* params, const WarpParamOffsets& po, const float* wpk, const nrf_step_scalars* sc) {
  WarpFwdArgs a;
  memset(&a, 0, sizeof(a));
  a.params = params; a.po = po; a.wpk = wpk; a.pk = h->wpk;
  a.F = h->Fw; a.G = h->G; a.Win = h->Win; a.PKw = h->PKw; a.alpha = sc->warp_alpha; a.dyn = sc->dynamic;
  return a;
}

WarpFwdArgs warp_points_args(nrf_handle h, const float* params, const WarpParamOffsets& po, const float* wpk, const nrf_step_scalars* sc,
                             const float* points, const int32_t* ids, int n, float* out) {
  WarpFwdArgs a = warp_field_args(h, params, po, wpk, sc);
  a.points_in = points; a.point_ids = ids; a.points_out = out; a.embed_table = params + po.embed;
  a.S = 1; a.B = n; a.rows = n; a.ntiles = (n + TILE_ROWS - 1) / TILE_ROWS;
  return a;
}

int require_ids_or_codes(const nrf_handle_s* h, const nrf_rays* r, bool camera, bool appearance, bool warp) {
  if (camera && h->d.use_camera_metadata && !r->camera_ids && !r->camera_codes) return fail(NRF_E_NULL, "camera_ids (or camera_codes) required (use_camera_metadata)");
  if (appearance && h->app_in_cond && !r->appearance_ids && !r->appearance_codes) return fail(NRF_E_NULL, "appearance_ids (or appearance_codes) required");
  if (warp && !r->warp_ids && !r->warp_codes) return fail(NRF_E_NULL, "warp_ids (or warp_codes) required (use_warp)");
  return NRF_OK;
}

const float* embed_params(nrf_handle h, const float* params_x, const EmbedDesc* table, float* image, bool zero_by_kernel, hipStream_t stream) {
  if (zero_by_kernel) {
    // the frozen step is made to be captured and replayed many times (one alignment step per replay): its image is cleared by a
    // kernel, not by a memset node.  Observed on an MI355X: from the SECOND replay of a captured step on, the image behind the
    // replayed memset node is no longer the eager one and the step returns NaN once the host has allocated in between, on the
    // non-frozen plans as well; with a full-width model (no padded image, no memset) every replay is exact.  The other callers
    // keep hipMemsetAsync as they were.
    ZeroArgs z;
    memset(&z, 0, sizeof(z));
    z.add(image, h->nparams);
    launch_zero_ranges(z, stream);
  } else if (hipMemsetAsync(image, 0, (size_t)h->nparams * sizeof(float), stream) != hipSuccess) {
    fail(NRF_E_HIP, "zero padded params");
    return nullptr;
  }
  launch_embed(table, (int)h->emb.size(), params_x, image, true, stream);
  return image;
}

RayPrepArgs ray_prep_args(const nrf_handle_s* h, const float* params, const nrf_rays* r, const float* viewdirs, float* cond,
                          const RayPrepLevel* lv, int nlv, bool app_only) {
  RayPrepArgs ra;
  memset(&ra, 0, sizeof(ra));
  ra.params = params; ra.cond = cond; ra.viewdirs = viewdirs; ra.B = r->num_rays;
  ra.app_ids = r->appearance_codes ? nullptr : r->appearance_ids; ra.app_codes = r->appearance_codes;
  ra.app_feat = h->A; ra.app_off = h->app_off; ra.R = h->A;
  if (!app_only) {
    ra.cam_ids = r->camera_codes ? nullptr : r->camera_ids; ra.cam_codes = r->camera_codes;
    ra.Fv = h->d.num_nerf_viewdir_freqs; ra.use_viewdirs = h->d.use_viewdirs;
    ra.cam_feat = h->d.use_camera_metadata ? h->d.num_camera_features : 0; ra.cam_off = h->cam_off; ra.R = h->R;
  }
  for (int i = 0; i < nlv; ++i) {
    const MlpParamOffsets& po = h->po[lv[i].level];
    ra.rgbh_k[i] = po.rgbh_k; ra.rgbh_b[i] = po.rgbh_b; ra.alpha_k[i] = po.alpha_k;
    ra.condterm[i] = lv[i].condterm; ra.alpha_ct[i] = h->A > 0 ? lv[i].alpha_ct : nullptr;
  }
  return ra;
}

ChainFwdArgs chain_model_args(const nrf_handle_s* h, const float* params, int level, const float* alpha_ct) {
  ChainFwdArgs a;
  memset(&a, 0, sizeof(a));
  a.params = params; a.po = h->po[level]; a.pk = h->pk; a.alpha_ct = h->A > 0 ? alpha_ct : nullptr; a.nx = h->d.nerf_rgb_branch_depth - 1;
  a.F = h->d.num_nerf_point_freqs; a.P = h->P; a.PK = h->PK; a.sigma_act = h->d.sigma_activation; a.skip = h->d.nerf_skip_layer;
  return a;
}

// algorithmic flops per MLP row (2 flop / MAC, dense layers only, unpadded)
static double rgbx_flops_row(const nrf_handle_s* h) { return 2.0 * 16384.0 * (h->d.nerf_rgb_branch_depth - 1); }   // rgb branch layers 1..
static double trunk_macs_row(const nrf_handle_s* h) { return h->P * 256 + 6 * 65536.0 + (256 + h->P) * 256 + 256; }   // 8 layers + alpha head
double density_flops_row(const nrf_handle_s* h) { return 2.0 * (trunk_macs_row(h) + (h->A > 0 ? 65536.0 : 0.0)); }   // (+ bottleneck)
double density_bwd_flops_row(const nrf_handle_s* h) { return 2.0 * (256 + (h->A > 0 ? 65536.0 : 0.0) + 7 * 65536.0 + 2.0 * 256 * h->P); }
double fwd_flops_row(const nrf_handle_s* h) { return 2.0 * (trunk_macs_row(h) + 65536.0 + (256.0 + h->R) * 128 + 128 * 3) + rgbx_flops_row(h); }
// SE3 field per row: trunk + heads
double warp_fwd_flops_row(const nrf_handle_s* h) { return 2.0 * (h->Win * 128 + 3 * 16384.0 + (128 + h->Win) * 128 + 16384.0 + 128 * 6); }

namespace {

int validate_rays(nrf_handle h, const nrf_rays* rays) {
  if (!rays || !rays->origins || !rays->directions) return fail(NRF_E_NULL, "rays / origins / directions is null");
  if (rays->num_rays <= 0) return fail(NRF_E_SHAPE, "num_rays must be positive");
  CK(require_ids_or_codes(h, rays, true, true, h->warp && !h->time_enc));
  if (h->warp && h->time_enc && !rays->time && !rays->warp_codes) return fail(NRF_E_NULL, "time (or warp_codes) required (warp_metadata_encoder_type 'time')");
  return NRF_OK;
}

int copy_out(float* dst, const float* src, size_t n, hipStream_t stream) {
  if (!dst) return NRF_OK;
  hipError_t e = hipMemcpyAsync(dst, src, n * sizeof(float), hipMemcpyDeviceToDevice, stream);
  return e == hipSuccess ? NRF_OK : fail_hip(e, "copy output");
}

double dgrad_flops_row(nrf_handle h, bool warp_on) {
  const double base = 2.0 * (128 * 3 + 256 * 128 + 65536.0 + 256 + 7 * 65536.0) + rgbx_flops_row(h);
  return warp_on ? base + 2.0 * (2.0 * 256 * h->P) : base;   // + d posenc through layer 0 and the skip rows
}
double warp_dgrad_flops_row(nrf_handle h) { return 2.0 * (128 * 6 + 5 * 16384.0 + 2.0 * h->G * 128); }
double warp_fwd_flops_row_or0(nrf_handle h) { return h->warp ? warp_fwd_flops_row(h) : 0.0; }
double wgrad_flops_row(nrf_handle h) {
  const double P = h->P, R = h->R;
  return 2.0 * (2 * P * 256 + 7 * 65536.0 + 65536.0 + (256 + R) * 128 + 256 + 128 * 3) + rgbx_flops_row(h);
}

// The modes of a forward call on the plan build_plan just made for `flags`
Modes forward_modes(const nrf_handle_s* h, uint32_t flags) {
  Modes m;
  m.train = flags & NRF_FLAG_TRAIN;
  m.warp_on = h->warp && !(flags & NRF_FLAG_NO_WARP);
  m.bf16 = flags & NRF_FLAG_BF16; m.x3 = flags & NRF_FLAG_BF16X3;   // x3: inference only (check_flags)
  m.jac = flags & NRF_FLAG_WARP_JACOBIAN;
  m.ray_grads = m.train && (flags & NRF_FLAG_RAY_GRADS);
  m.frozen = m.ray_grads && (flags & NRF_FLAG_FROZEN);
  // the SE3 trunk follows the MLPs into bf16 / split-bf16 unless the caller opts out (NRF_FLAG_WARP_F32) or asks for the Jacobian
  // output (inference tangent pass: fp32 kernels, their input stash); a training plan has decided already (its stash layout depends on it)
  const bool follows = m.train ? h->plan.bfw : !(flags & NRF_FLAG_WARP_F32) && !m.jac;
  if (m.warp_on && follows) m.trunk = m.x3 ? WarpTrunk::X3 : m.bf16 ? WarpTrunk::BF16 : WarpTrunk::F32;
  return m;
}

// One call's context and the argument builders both directions share.  `params` is the INTERNAL parameter image: the caller's
// buffer, or for a narrower model its zero-padded image in the workspace (nrf_internal.h EmbedDesc).
struct Run {
  nrf_handle h;  const WsPlan& p;  const nrf_model_desc& d;  Prof& pf;  const Modes m;
  float* ws;  hipStream_t stream;
  const nrf_rays* rays;  const nrf_step_scalars* sc;  const nrf_background* bg;
  const int B;  const bool bg_on;   // bg_on: the fused train step's background batch (the only caller that passes `bg`)
  const char* tables;   // descriptor tables (upload_tables)
  const float* params = nullptr;
  Run(nrf_handle h_, const Modes& m_, float* ws_, hipStream_t st, const nrf_rays* r, const nrf_step_scalars* s, const nrf_background* b)
      : h(h_), p(h_->plan), d(h_->d), pf(h_->prof), m(m_), ws(ws_), stream(st), rays(r), sc(s), bg(b), B(h_->plan.key.B),
        bg_on(b && h_->plan.key.bgN > 0), tables(reinterpret_cast<const char*>(ws_ + h_->plan.tables)) {}
  const nrf_dynamic_scalars* dyn() const { return sc ? sc->dynamic : nullptr; }
  bool bf16_trunk() const { return m.trunk == WarpTrunk::BF16; }
  int rows_pad(int lv) const { return p.ntiles[lv] * TILE_ROWS; }
  int pks() const { return (h->PKw + 31) / 32 * 32; }
  template <class T> const T* table(size_t off_b) const { return reinterpret_cast<const T*>(tables + off_b); }
  uint32_t* u32(size_t off) const { return reinterpret_cast<uint32_t*>(ws + off); }
  float4* f4(size_t off) const { return reinterpret_cast<float4*>(ws + off); }
  BfStash bf_stash(int lv) const {
    const LevelWs& L = p.L[lv];
    BfStash b;
    b.pe = u32(L.b_pe); b.h = u32(L.b_h); b.bn = u32(L.b_bn); b.rgbh = u32(L.b_rgbh); b.bits = u32(L.b_bits);
    b.dy = u32(L.b_dy); b.dbn = u32(L.b_dbn); b.drgbh = u32(L.b_drgbh); b.dsmall = u32(L.b_dsmall); b.ngroups = L.b_ngroups;
    return b;
  }
  BfWarpStash bfw_stash(int lv) const {
    const LevelWs& L = p.L[lv];
    BfWarpStash b;
    b.win = u32(L.bw_in); b.h = u32(L.bw_h); b.bits = u32(L.bw_bits); b.dy = u32(L.bw_dy); b.dhead = u32(L.bw_dhead); b.ngroups = L.bw_ngroups;
    return b;
  }
  // the points / ids the background level runs on: the caller's (already noised, ids given) or the library's own draw
  const float* bg_points() const { return bg->warp_ids ? bg->points : ws + p.bg_points; }
  const int32_t* bg_ids() const { return bg->warp_ids ? bg->warp_ids : reinterpret_cast<const int32_t*>(ws + p.bg_ids); }
  // modules.TimeEncoder once per ray (warping.py:311-313, models.py:252-254), forward or reverse
  TimeEncArgs time_enc_args(bool reverse) const {
    TimeEncArgs a;
    memset(&a, 0, sizeof(a));
    a.params = params; a.po = h->tpo; a.time = rays->time; a.B = B; a.F = h->Ft; a.Tin = h->Tin; a.G = h->G;
    if (m.train && !m.frozen) { a.st_in = ws + p.t_in; a.st_h = ws + p.t_h; }
    if (reverse) { a.d_codes = ws + p.t_dcodes; a.st_dpre = ws + p.t_dpre; }
    else { a.alpha = sc->time_alpha; a.dyn = dyn(); a.codes = ws + p.t_codes; }
    return a;
  }
  // The bf16 (or split-bf16) trunk's additions to the forward or reverse arguments of a pass over level `lv`: its weight stream,
  // the pass's stash, the rows of the per-row fp32 buffers.  prim >= 0: the tangent pass (lv = TG) of primal level `prim` --
  // tangent groups = 3 x the primal groups, masks = the primal pass's bits.  The float32 kernels read none of it.
  template <class A> void add_bf16_trunk(A& a, size_t stream_off, int lv, bool stash, int prim = -1) const {
    if (m.trunk == WarpTrunk::F32) return;
    a.bwpk = ws + stream_off;
    a.rows_pad = rows_pad(prim >= 0 ? prim : lv);
    if (stash) a.bst = bfw_stash(lv);
    if (prim < 0) return;
    a.rows = p.rows[prim];
    a.bprim_bits = u32(p.L[prim].bw_bits); a.bng_prim = p.L[prim].bw_ngroups;
  }
};

struct Forward : Run {
  const nrf_rand* rnd;  const nrf_outputs* out;
  Forward(const Run& r, const nrf_rand* rnd_, const nrf_outputs* out_) : Run(r), rnd(rnd_), out(out_) {}
  int checks(size_t ws_bytes) const {
    if (ws_bytes < p.total_floats * sizeof(float)) return fail(NRF_E_WORKSPACE, "workspace too small (see nrf_workspace_bytes)");
    // the bf16 / x3 chains' streams (launch_bf16_pack below)
    if ((m.bf16 || m.x3) && !p.bf_stream_ok) return fail(NRF_E_STATE, "bf16 weight stream tables do not match the kernels' chunk sequence");
    if (m.warp_on && !sc) return fail(NRF_E_NULL, "nrf_step_scalars (warp_alpha) required with the warp field");
    if (h->warp && !m.warp_on && m.train) return fail(NRF_E_UNSUPPORTED, "NRF_FLAG_NO_WARP cannot be combined with NRF_FLAG_TRAIN");
    if (d.use_stratified_sampling && !rnd) return fail(NRF_E_NULL, "nrf_rand required with stratified sampling");
    const bool encoded = rays->warp_codes || rays->appearance_codes || rays->camera_codes;
    if (encoded && m.train) return fail(NRF_E_UNSUPPORTED, "pre-encoded metadata (metadata_encoded) is an inference input: no gradient flows to the codes");
    if (m.jac && (!m.warp_on || m.train)) return fail(NRF_E_UNSUPPORTED, "NRF_FLAG_WARP_JACOBIAN needs the warp field and an inference call (training consumes the Jacobian through nrf_elastic)");
    if (!m.jac && out && (out->coarse.warp_jacobian || out->fine.warp_jacobian)) return fail(NRF_E_STATE, "warp_jacobian outputs need NRF_FLAG_WARP_JACOBIAN");
    return NRF_OK;
  }
  // tables, the padded parameter image, weight packs, per-ray terms, coarse samples, the background draw, the time encoder
  int prepare(const float* params_x) {
    CK(upload_tables(h, ws, stream));
    if (tile_counter_or_null(ws + p.counters, 0) &&   // NRF_DYNAMIC_TILES experiment only
        hipMemsetAsync(ws + p.counters, 0, 64 * sizeof(int), stream) != hipSuccess) return fail(NRF_E_HIP, "zero tile counters");
    params = params_x;
    // narrower model: run on its zero-padded image (the table went up with upload_tables)
    if (h->embed && !(params = embed_params(h, params_x, table<EmbedDesc>(p.emb_off_b), ws + p.iparams, m.frozen, stream))) return NRF_E_HIP;
    pf.begin("pack_prep_sample", 0, stream);
    if (!p.pack.empty()) launch_pack(table<PackDesc>(p.pack_off_b), (int)p.pack.size(), params, ws, stream);
    if (m.bf16 || m.x3) launch_bf16_pack(reinterpret_cast<const RcPackDesc*>(ws + p.bf_desc), (int)p.bfpack.size(), params, ws, stream);
    ray_prep();
    launch_sample_coarse(rnd ? rnd->t_rand : nullptr, B, p.S[0], d.near_plane, d.far_plane, d.use_stratified_sampling,
                         d.use_linear_disparity, rnd ? rnd->seed : 0, rnd ? rnd->offset : 0, dyn(), ws + p.L[0].z, stream);
    // nrf_background.warp_ids == NULL: training.py:121-126 on the device (ids from id_choices, noise added), into the workspace
    if (m.train && bg_on && m.warp_on && !bg->warp_ids)
      launch_background_draw(bg->points, p.key.bgN, bg->id_choices, bg->num_choices, bg->noise_std, rnd ? rnd->seed : 0, rnd ? rnd->offset : 0,
                             dyn(), ws + p.bg_points, reinterpret_cast<int32_t*>(ws + p.bg_ids), stream);
    pf.end(stream);
    if (m.warp_on && h->time_enc && !rays->warp_codes) launch_time_encoder_fwd(time_enc_args(false), stream);
    return NRF_OK;
  }

  void ray_prep() const {
    RayPrepLevel lv[2];
    for (int i = 0; i < h->nlevels; ++i) lv[i] = {i, ws + p.L[i].condterm, ws + p.L[i].alpha_ct};
    const float* viewdirs = rays->viewdirs ? rays->viewdirs : rays->directions;   // models.py:326-329
    launch_ray_prep(ray_prep_args(h, params, rays, viewdirs, ws + p.cond, lv, h->nlevels, false), stream);
  }

  void sample_fine() {
    pf.begin("sample_pdf", 0, stream);
    launch_sample_fine(ws + p.L[0].z, ws + p.L[0].weights, B, d.num_coarse_samples, d.num_fine_samples, d.use_stratified_sampling,
                       rnd ? rnd->u : nullptr, rnd ? rnd->seed : 0, rnd ? rnd->offset : 0, dyn(), ws + p.L[1].z, stream);
    pf.end(stream);
  }
  // the fp32 stash of a pass over level L (a training plan, or an inference plan that returns the Jacobian)
  void keep_warp_stash(WarpFwdArgs& a, const LevelWs& L) const {
    a.st_win = ws + L.w_st_win; a.st_h = m.frozen ? nullptr : ws + L.w_st_h; a.st_wv = f4(L.w_st_wv); a.bits = u32(L.w_bits);
  }

  WarpFwdArgs warp_fwd_args(int lv) const {
    const LevelWs& L = p.L[lv];
    WarpFwdArgs a = warp_field_args(h, params, h->wpo, ws + p.warp_wpk, sc);
    a.zvals = ws + L.z; a.origins = rays->origins; a.directions = rays->directions;
    // metadata_encoded (warping.py:378-381): the caller's per-ray codes stand in for the table, row = ray
    // the same for the TimeEncoder's per-ray output
    const bool per_ray = rays->warp_codes || h->time_enc;
    a.warp_ids = per_ray ? nullptr : rays->warp_ids;
    a.embed_table = rays->warp_codes ? rays->warp_codes : h->time_enc ? ws + p.t_codes : params + h->wpo.embed;
    a.points_out = ws + L.wpoints; a.points_raw = ws + L.points_raw;
    a.S = p.S[lv]; a.B = B; a.rows = p.rows[lv]; a.ntiles = p.ntiles[lv];
    a.tile_counter = tile_counter_or_null(ws + p.counters, CT_WARP_FWD + lv);
    if (m.train || m.jac) keep_warp_stash(a, L);
    return a;
  }
  // SE3 field on level lv's samples; the background-point batch of the fused train step rides in the coarse launch (its 256
  // tiles under-fill the chip)
  void warp(int lv) {
    const bool with_bg = lv == 0 && m.train && bg_on;
    const bool stash = m.train || m.jac;
    WarpFwdArgs wa = warp_fwd_args(lv), bga;
    if (with_bg) {
      bga = warp_points_args(h, params, h->wpo, ws + p.warp_wpk, sc, bg_points(), bg_ids(), p.key.bgN, ws + p.L[BG].wpoints);
      keep_warp_stash(bga, p.L[BG]);
    }
    add_bf16_trunk(wa, p.bfw_wpk, lv, stash);
    if (with_bg) add_bf16_trunk(bga, p.bfw_wpk, BG, true);
    const WarpFwdArgs* bgp = with_bg ? &bga : nullptr;
    pf.begin(lv == 0 ? "warp_fwd_coarse" : "warp_fwd_fine", warp_fwd_flops_row(h) * (p.rows[lv] + (with_bg ? p.key.bgN : 0)), stream);
    if (m.trunk == WarpTrunk::X3) launch_warp_fwd_x3(wa, h->num_cus, stream);   // split-bf16 arithmetic (warp_bf16x3.hip)
    else if (bf16_trunk()) launch_warp_fwd_bf16(wa, bgp, stash, h->num_cus, stream);   // one workgroup per CU, 256 rows per iteration
    else launch_warp_fwd(wa, bgp, stash, tile_grid(p.ntiles[lv] + (with_bg ? p.ntiles[BG] : 0), warp_grid_mul(), h->num_cus), stream, m.frozen);
    pf.end(stream);
  }
  // forward-mode pass of the warp Jacobian of level lv (warping.py:385-387): 3 tangent tiles per primal tile
  // the stash a tangent pass of level lv writes: TG, or -- ray gradients next to the elastic regulariser, whose reverse pass and
  // wgrad groups keep reading the coarse tangents in TG -- the fine level's scratch (Planner::ray_grad_buffers)
  const LevelWs& tangent_level(int lv) const { return m.ray_grads && p.key.elastic && lv > 0 ? p.rg_tan_fine : p.L[TG]; }
  void tangent_fwd(int lv) {
    const LevelWs &L = p.L[lv], &T = tangent_level(lv);
    WarpFwdArgs ta = warp_fwd_args(lv);
    ta.nt_prim = p.ntiles[lv]; ta.prim_win = ws + L.w_st_win; ta.prim_bits = u32(L.w_bits);
    ta.ntiles = 3 * p.ntiles[lv]; ta.rows = ta.ntiles * TILE_ROWS;
    keep_warp_stash(ta, T);
    ta.bits = nullptr; ta.points_out = ws + T.wpoints; ta.points_raw = nullptr;
    if (m.frozen) { ta.st_win = nullptr; ta.points_out = nullptr; }   // a frozen plan's tangent level is its (dw, dv) rows alone
    ta.tile_counter = tile_counter_or_null(ws + p.counters, CT_TAN_FWD);
    add_bf16_trunk(ta, p.bfw_wpk, TG, true, lv);
    pf.begin("warp_tangent_fwd", 3.0 * warp_fwd_flops_row(h) * p.rows[lv], stream);
    if (bf16_trunk()) launch_warp_fwd_bf16(ta, nullptr, true, h->num_cus, stream);
    else launch_warp_fwd(ta, nullptr, true, tile_grid(ta.ntiles, warp_grid_mul(), h->num_cus), stream, m.frozen);
    pf.end(stream);
  }
  // forward-mode Jacobian of the warp: on the coarse samples for the elastic regulariser (models.py:345), per level
  // as an output (return_warp_jacobian, models.py:345-346, 367-368)
  // ... and per level into the workspace for nrf_backward_rays (NRF_FLAG_RAY_GRADS: the tangent pass runs in the forward, right
  // behind the primal pass whose (alpha, codes) it shares; the levels take turns on the one tangent stash, except next to the
  // elastic regulariser: tangent_level)
  void jacobian(int lv) {
    float* jout = !out ? nullptr : lv == 0 ? out->coarse.warp_jacobian : out->fine.warp_jacobian;
    if (m.ray_grads) jout = ws + p.L[lv].rg_jac;
    if ((lv == 0 && m.train && p.key.elastic) || (m.jac && jout) || m.ray_grads) tangent_fwd(lv);
    if (!(m.jac || m.ray_grads) || !jout) return;
    JacobianArgs ja;
    memset(&ja, 0, sizeof(ja));   // x_rows = nullptr: the points come from the fp32 input stash
    ja.prim_win = ws + p.L[lv].w_st_win; ja.prim_wv = f4(p.L[lv].w_st_wv); ja.tan_wv = f4(tangent_level(lv).w_st_wv); ja.out = jout;
    ja.rows = p.rows[lv]; ja.rows_pad = rows_pad(lv); ja.PKS = pks();
    launch_jacobian(ja, stream);
  }

  ChainFwdArgs chain_fwd_args(int lv) const {
    const LevelWs& L = p.L[lv];
    ChainFwdArgs a = chain_model_args(h, params, lv, ws + L.alpha_ct);
    a.wpk = ws + L.wpk; a.condterm = ws + L.condterm; a.zvals = ws + L.z; a.origins = rays->origins; a.directions = rays->directions;
    a.points = m.warp_on ? ws + L.wpoints : nullptr; a.out4 = f4(L.out4);
    a.S = p.S[lv]; a.B = B; a.rows = p.rows[lv]; a.ntiles = p.ntiles[lv];
    a.tile_counter = tile_counter_or_null(ws + p.counters, CT_MLP_FWD + lv);
    a.timeline = knobs().timeline ? reinterpret_cast<unsigned long long*>(ws + p.timeline + lv * TIMELINE_LEVEL_F) : nullptr;
    if (d.noise_std > 0.f && d.use_stratified_sampling) {   // model_utils.noise_regularize (model_utils.py:266-282)
      a.noise_std = d.noise_std;
      a.noise = rnd ? (lv == 0 ? rnd->noise_coarse : rnd->noise_fine) : nullptr;
      a.noise_seed = rnd ? rnd->seed : 0; a.noise_offset = rnd ? rnd->offset : 0; a.noise_stream = 2u + (unsigned)lv;
      a.dyn = dyn();
    }
    if (m.train && m.bf16) {
      a.bst = bf_stash(lv);
    } else if (m.frozen) {   // posenc stash and sign words only (nerf_chain.h STASH_BITS)
      a.st_pe = ws + L.st_pe; a.bits_trunk = u32(L.bits_trunk); a.bits_rgbh = u32(L.bits_rgbh); a.bits_rgbx = u32(L.bits_rgbx);
    } else if (m.train) {
      a.st_pe = ws + L.st_pe; a.st_h = ws + L.st_h; a.st_bn = ws + L.st_bn; a.st_rgbh = ws + L.st_rgbh;
      a.bits_trunk = u32(L.bits_trunk); a.bits_rgbh = u32(L.bits_rgbh); a.st_rgbx = ws + L.st_rgbx; a.bits_rgbx = u32(L.bits_rgbx);
    }
    return a;
  }

  void mlp(int lv) {
    ChainFwdArgs a = chain_fwd_args(lv);
    const ChainTiling t = chain_fwd_tiling(h, p.ntiles[lv], !m.bf16 && !m.x3);
    a.k_old = t.k_old;
    pf.begin(lv == 0 ? "mlp_fwd_coarse" : "mlp_fwd_fine", fwd_flops_row(h) * p.rows[lv], stream);
    if (m.bf16 || m.x3) a.wpk = ws + p.L[lv].bf_wpk;
    if (m.bf16) launch_chain_fwd_bf16(a, h->num_cus, stream);   // one workgroup per CU (90 KiB of weight staging), 256 samples per workgroup iteration
    else if (m.x3) launch_chain_fwd_x3(a, h->num_cus, stream);   // one four-wave workgroup per CU (150 KiB ring), 128 samples per workgroup iteration
    else if (m.frozen) launch_chain_fwd_frozen(a, t.c32, t.grid, stream);
    else if (t.c32) launch_chain_fwd32(a, m.train, t.grid, stream);
    else launch_chain_fwd(a, m.train, t.grid, stream);
    pf.end(stream);
  }

  void composite(int lv) {
    const LevelWs& L = p.L[lv];
    pf.begin("composite_fwd", 0, stream);
    launch_composite_fwd(f4(L.out4), ws + L.z, rays->directions, B, p.S[lv], d.use_white_background, d.use_sample_at_infinity,
                         ws + L.rgb, ws + L.depth, ws + L.med, ws + L.acc, ws + L.weights, stream);
    pf.end(stream);
  }

  int outputs(int lv) const {
    if (!out) return NRF_OK;
    const LevelWs& L = p.L[lv];
    const nrf_level_out& lo = lv == 0 ? out->coarse : out->fine;
    const size_t nb = B, nr = p.rows[lv];
    const struct { float* dst; size_t src, n; } plain[] = {{lo.rgb, L.rgb, 3 * nb}, {lo.depth, L.depth, nb}, {lo.med_depth, L.med, nb},
                                                            {lo.acc, L.acc, nb}, {lo.weights, L.weights, nr}, {lo.z_vals, L.z, nr}};
    for (const auto& c : plain) CK(copy_out(c.dst, ws + c.src, c.n, stream));
    if (lo.warped_points && !m.warp_on) return fail(NRF_E_UNSUPPORTED, "the warped_points output needs the warp field (models.py:266-267)");
    if (lo.points && !m.warp_on)   // models.py:247-248: `points` is returned whether or not the model warps
      launch_sample_points(rays->origins, rays->directions, ws + L.z, B, p.S[lv], lo.points, stream);
    else if (lo.points || lo.warped_points) {
      CK(copy_out(lo.points, ws + L.points_raw, 3 * nr, stream));
      CK(copy_out(lo.warped_points, ws + L.wpoints, 3 * nr, stream));
    }
    return NRF_OK;
  }
};

struct Backward : Run {
  const nrf_elastic* el;  const nrf_warp_reg* wr;  const bool el_on, wr_on;
  const nrf_ray_grads* rg = nullptr;   // nrf_backward_rays: the ray gradients to write (the stash was kept under NRF_FLAG_RAY_GRADS)
  bool fold_viewdirs = false;          // nrf_train_step_loss_grad_rays: rays->viewdirs == NULL adds the view term to d_directions
  const nrf_output_grads* og;   // the caller's cotangents (nrf_backward[_ex]) or nullptr (fused step: the MSE loss against `target`)
  float* grad = nullptr;   // INTERNAL layout, as params
  double mlp_rows = 0;     // samples of all levels
  Backward(const Run& r, const nrf_elastic* el_, const nrf_warp_reg* wr_, const nrf_output_grads* og_)
      : Run(r), el(el_), wr(wr_), el_on(el_ && p.key.elastic && m.warp_on), wr_on(wr_ && m.warp_on), og(og_) {
    for (int lv = 0; lv < h->nlevels; ++lv) mlp_rows += p.rows[lv];
  }
  int zero() const {   // everything that is accumulated into, zeroed by one launch
    ZeroArgs z;
    memset(&z, 0, sizeof(z));
    if (!m.frozen) z.add(grad, h->nparams);   // a frozen stash has no parameter gradient: dray is all its reverse pass adds into
    if (m.warp_on && h->time_enc && !m.frozen) z.add(ws + p.t_dcodes, (long long)B * h->G);
    if (wr_on) z.add(ws + p.wr_sums, 64);
    if (bg_on) z.add(ws + p.bg_loss, 64);
    for (int lv = 0; lv < h->nlevels; ++lv) z.add(ws + p.L[lv].dray, (long long)B * RGB_W);
    if (p.bwd32)   // the 32-row reverse chain ADDS its bias column sums into the workgroups' slices
      for (int lv = 0; lv < h->nlevels; ++lv) z.add(ws + p.L[lv].small_part, (long long)p.grid_mlp_bwd * SMALL_PART);
    if (z.overflow) return fail(NRF_E_STATE, "zero_ranges table full: an accumulator would stay unzeroed");
    launch_zero_ranges(z, stream);
    return NRF_OK;
  }

  const nrf_level_grads* level_grads(int lv) const { return !og ? nullptr : lv == 0 ? &og->coarse : &og->fine; }

  void composite_bwd(const float* target) {
    CompositeBwdArgs ca[2];
    for (int lv = 0; lv < h->nlevels; ++lv) {
      const LevelWs& L = p.L[lv];
      CompositeBwdArgs& c = ca[lv];
      memset(&c, 0, sizeof(c));
      c.out4 = f4(L.out4); c.z = ws + L.z; c.dirs = rays->directions; c.sigma_act = d.sigma_activation;
      c.B = B; c.S = p.S[lv]; c.white_bkgd = d.use_white_background; c.sample_at_inf = d.use_sample_at_infinity;
      c.rgb_out = ws + L.rgb; c.target = target;
      if (const nrf_level_grads* g = level_grads(lv)) { c.d_rgb = g->d_rgb; c.d_depth = g->d_depth; c.d_acc = g->d_acc; c.d_w = g->d_weights; }
      c.loss_scale = 2.0f / (3.0f * (float)B);   // d/d rgb of mean over (B,3) (training.py:172)
      c.d_raw4 = f4(L.d_raw4); c.rows_pad = rows_pad(lv);
      c.mse_ray = ws + p.mse + (size_t)lv * B; c.dsig_ray = h->A > 0 ? ws + L.dsig_ray : nullptr;
      if (rg && rg->d_directions) c.sdsig_ray = ws + L.rg_sdsig;
    }
    pf.begin("composite_bwd", 0, stream);
    launch_composite_bwd(ca[0], h->nlevels > 1 ? &ca[1] : nullptr, stream);
    pf.end(stream);
  }

  ChainBwdArgs chain_bwd_args(int lv) const {
    const LevelWs& L = p.L[lv];
    ChainBwdArgs a;
    memset(&a, 0, sizeof(a));
    a.params = params; a.po = h->po[lv]; a.wpk = ws + L.wpk; a.pk = h->pk;
    a.S = p.S[lv]; a.B = B; a.rows = p.rows[lv]; a.ntiles = p.ntiles[lv];
    a.d_raw4 = f4(L.d_raw4); a.bits_trunk = u32(L.bits_trunk); a.bits_rgbh = u32(L.bits_rgbh);
    a.dy_trunk = ws + L.dy_trunk; a.dy_bn = ws + L.dy_bn; a.dy_rgbh = ws + L.dy_rgbh; a.dray = ws + L.dray; a.small_part = ws + L.small_part;
    if (m.frozen) a.dy_trunk = a.dy_bn = a.dy_rgbh = a.small_part = nullptr;   // not in the plan, not written (bwd_tile<., ., false>)
    if (m.warp_on) { a.d_points = ws + L.d_points; a.st_pe = ws + L.st_pe; }
    else if (rg && (rg->d_origins || rg->d_directions)) {   // no warp field: d points only for the ray stage, W^T images of their own
      a.d_points = ws + L.d_points; a.st_pe = ws + L.st_pe;
    }
    if (m.ray_grads && !h->warp) { a.wpk = ws + L.rg_wpkT; a.pk.bwd_L0T = p.rg_L0T; a.pk.bwd_L4bT = p.rg_L4bT; }
    a.F = d.num_nerf_point_freqs; a.P = h->P; a.PK = h->PK; a.skip = d.nerf_skip_layer;
    a.alpha_on_bn = h->A > 0 ? 1 : 0;
    a.nx = d.nerf_rgb_branch_depth - 1; a.bits_rgbx = u32(L.bits_rgbx); a.dy_rgbx = m.frozen ? nullptr : ws + L.dy_rgbx;
    return a;
  }
  // ONE NeRF-MLP dgrad launch over the tiles of both levels, on the grid the plan's reduce table was built for
  void mlp_dgrad() {
    // the d-points section runs whenever chain_bwd_args hands d_points over
    const double flops = dgrad_flops_row(h, m.warp_on || (rg && (rg->d_origins || rg->d_directions))) * mlp_rows;
    if (!m.bf16) {
      ChainBwdArgs ca[2];
      for (int lv = 0; lv < h->nlevels; ++lv) ca[lv] = chain_bwd_args(lv);
      pf.begin("mlp_dgrad", flops, stream);
      if (m.frozen) launch_chain_bwd_frozen(ca[0], h->nlevels > 1 ? &ca[1] : nullptr, p.grid_mlp_bwd, stream);   // 64-row tiles always
      else (p.bwd32 ? launch_chain_bwd32 : launch_chain_bwd)(ca[0], h->nlevels > 1 ? &ca[1] : nullptr, p.grid_mlp_bwd, stream);
      pf.end(stream);
      return;
    }
    // bf16 chains: dpre of every layer into the bf16 dY stash, then the per-ray condition sums
    ChainBwdBf16Args ba[2];
    for (int lv = 0; lv < h->nlevels; ++lv) {
      const LevelWs& L = p.L[lv];
      ChainBwdBf16Args& b = ba[lv];
      memset(&b, 0, sizeof(b));
      b.wpk = ws + L.bf_wpkT; b.d_raw4 = f4(L.d_raw4);
      b.S = p.S[lv]; b.B = B; b.rows = p.rows[lv]; b.st = bf_stash(lv);
      if (m.warp_on) {
        b.points = ws + L.wpoints; b.d_points = ws + L.d_points; b.rows_pad = rows_pad(lv);
        b.F = d.num_nerf_point_freqs; b.P = h->P;
      }
    }
    pf.begin("mlp_dgrad", flops, stream);
    launch_chain_bwd_bf16(ba[0], h->nlevels > 1 ? &ba[1] : nullptr, h->num_cus, stream);
    pf.end(stream);
    for (int lv = 0; lv < h->nlevels; ++lv) launch_dray_bf16(ba[lv].st.drgbh, B, p.S[lv], ws + p.L[lv].dray, stream);
  }

  void elastic() const {   // training.compute_elastic_loss on the coarse samples
    const LevelWs &L = p.L[0], &T = p.L[TG];
    ElasticArgs ea;
    memset(&ea, 0, sizeof(ea));
    ea.prim_win = ws + L.w_st_win; ea.prim_wv = f4(L.w_st_wv);
    if (bf16_trunk()) ea.x_rows = ws + L.points_raw;   // bf16 trunk: no fp32 input stash
    ea.tan_wv = f4(T.w_st_wv); ea.coef = ws + L.weights;
    if (el->reduce_method == NRF_ELASTIC_MEDIAN) {   // training.py:182-188
      launch_median_coef(ws + L.weights, B, p.S[0], ws + p.el_coef, stream);
      ea.coef = ws + p.el_coef; ea.res_selected = 1;
    }
    ea.tan_dw4 = f4(T.w_dw4); ea.tan_dv4 = f4(T.w_dv4);
    ea.prim_dw4 = f4(L.el_dw4); ea.prim_dv4 = f4(L.el_dv4);
    ea.part = ws + p.el_sums; ea.rows = p.rows[0]; ea.rows_pad = rows_pad(0); ea.PKS = pks();
    ea.eps = el->eps; ea.alpha = el->loss_alpha; ea.scale = el->loss_scale; ea.gscale = el->loss_weight / (float)B;
    ea.inv_rays = 1.0f / (float)B; ea.dyn = dyn(); ea.loss_type = el->loss_type;
    pf.begin("elastic", 0, stream);
    launch_elastic(ea, stream);
    pf.end(stream);
  }
  // The caller's and the regularisers' gradients w.r.t. the warped points, added into d_points ahead of the SE3 dgrad, in two
  // parts around the ray stage: the caller's cotangent reaches the rays, the regularisers' terms do not (they regularise the field;
  // nrf_train_step_loss_grad_rays treats their dependence on the sample positions as stop-gradient)
  void point_cotangents() {
    for (int lv = 0; lv < h->nlevels && m.warp_on; ++lv)   // nrf_backward_ex: the caller's own d loss / d warped point
      if (const nrf_level_grads* g = level_grads(lv))
        if (g->d_warped_points) launch_add_point_cotangent(g->d_warped_points, p.rows[lv], ws + p.L[lv].d_points, stream);
  }
  void point_regularisers() {
    if (el_on) elastic();
    if (wr_on)   // use_warp_reg_loss (training.py:199-212): + d loss / d warped point at the median-depth sample of each ray
      for (int lv = 0; lv < h->nlevels; ++lv) {
        const LevelWs& L = p.L[lv];
        launch_warp_reg(ws + L.weights, ws + L.points_raw, ws + L.wpoints, B, p.S[lv], wr->loss_alpha, wr->loss_scale,
                        wr->loss_weight / (float)B, ws + L.d_points, ws + p.wr_sums + 2 * lv, stream);
      }
    // background regulariser (training.compute_background_loss, training.py:117-135): the SE3 field on the (already noised)
    // background points with one warp id per point; general loss of |x' - x|^2
    if (bg_on)
      launch_background_loss(bg_points(), ws + p.L[BG].wpoints, p.key.bgN, rows_pad(BG), bg->loss_alpha, bg->loss_scale,
                             bg->loss_weight, ws + p.L[BG].d_points, ws + p.bg_loss, stream);
  }
  // nrf_backward_rays: d_points (+ the caller's warped-point cotangent) -> the three per-ray gradients, both levels in one launch
  void ray_grads() {
    RayGradArgs a;
    memset(&a, 0, sizeof(a));
    for (int lv = 0; lv < h->nlevels; ++lv) {
      const LevelWs& L = p.L[lv];
      a.d_points[lv] = ws + L.d_points; a.z[lv] = ws + L.z; a.jac[lv] = m.warp_on ? ws + L.rg_jac : nullptr;
      a.dray[lv] = ws + L.dray; a.sdsig[lv] = ws + L.rg_sdsig; a.rgbh_k[lv] = h->po[lv].rgbh_k; a.S[lv] = p.S[lv];
    }
    a.params = params; a.dirs = rays->directions; a.viewdirs = rays->viewdirs;
    a.fold_viewdirs = fold_viewdirs && d.use_viewdirs && !rays->viewdirs;
    a.B = B; a.nlevels = h->nlevels; a.V = h->V; a.Fv = d.num_nerf_viewdir_freqs;
    a.d_origins = rg->d_origins; a.d_directions = rg->d_directions; a.d_viewdirs = rg->d_viewdirs;
    pf.begin("ray_grads", 0, stream);
    launch_ray_grad(a, stream);
    pf.end(stream);
  }
  // reverse arguments of the pass over level lv (BG: S = 1 from Planner::shapes), at the fp32 rows `x_rows` (bf16 trunk only)
  WarpBwdArgs warp_bwd_args(int lv, const float* x_rows) const {
    const LevelWs& L = p.L[lv];
    WarpBwdArgs w;
    memset(&w, 0, sizeof(w));
    w.params = params; w.po = h->wpo; w.wpk = ws + p.warp_wpk; w.pk = h->wpk;
    w.S = p.S[lv]; w.rows = p.rows[lv]; w.ntiles = p.ntiles[lv]; w.nt_prim = p.ntiles[lv];
    w.d_points = ws + L.d_points; w.st_win = ws + L.w_st_win; w.st_wv = f4(L.w_st_wv); w.bits = u32(L.w_bits);
    w.F = h->Fw; w.G = h->G; w.Win = h->Win; w.PKw = h->PKw;
    w.dy = ws + L.w_dy; w.d_w4 = f4(L.w_dw4); w.d_v4 = f4(L.w_dv4);
    w.small_part = ws + p.L[0].w_small_part;   // one set of bias partials for the whole launch
    add_bf16_trunk(w, p.bfw_wpkT, lv, true);
    if (bf16_trunk()) w.x_rows = x_rows;
    return w;
  }
  // ONE SE3 dgrad launch (coarse + fine + background tiles) on the plan's grid, then the reverse of the tangent pass
  void warp_dgrad() {
    WarpBwdArgs wa[3];
    int nlev = 0;
    double rows_all = mlp_rows;
    for (int lv = 0; lv < h->nlevels; ++lv) {
      WarpBwdArgs& w = wa[nlev++] = warp_bwd_args(lv, ws + p.L[lv].points_raw);
      w.B = B;
      w.warp_ids = h->time_enc ? nullptr : rays->warp_ids;   // TimeEncoder: the code gradient is per ray
      w.grad_embed = h->time_enc ? ws + p.t_dcodes : grad + h->wpo.embed;
      if (el_on && lv == 0) { w.extra_dw4 = f4(p.L[0].el_dw4); w.extra_dv4 = f4(p.L[0].el_dv4); }
    }
    if (bg_on) {
      WarpBwdArgs& w = wa[nlev++] = warp_bwd_args(BG, bg_points());
      w.B = p.key.bgN; w.point_ids = bg_ids(); w.grad_embed = grad + h->wpo.embed;
      rows_all += p.rows[BG];
    }
    const WarpBwdArgs *w1 = nlev > 1 ? &wa[1] : nullptr, *w2 = nlev > 2 ? &wa[2] : nullptr;
    pf.begin("warp_dgrad", warp_dgrad_flops_row(h) * rows_all, stream);
    if (bf16_trunk()) launch_warp_bwd_bf16(wa[0], w1, w2, h->num_cus, stream);
    else launch_warp_bwd(wa[0], w1, w2, p.grid_warp_bwd, stream);
    pf.end(stream);
    if (!el_on) return;
    const LevelWs& T = p.L[TG];
    WarpBwdArgs ta = wa[0];
    ta.tangent = 1; ta.nt_prim = p.ntiles[0]; ta.ntiles = p.ntiles[TG]; ta.rows = p.rows[TG];
    ta.extra_dw4 = ta.extra_dv4 = nullptr;
    ta.d_points = nullptr; ta.st_win = nullptr; ta.st_wv = nullptr; ta.small_part = nullptr;
    ta.dy = ws + T.w_dy; ta.d_w4 = f4(T.w_dw4); ta.d_v4 = f4(T.w_dv4);
    add_bf16_trunk(ta, p.bfw_wpkT, TG, true, 0);
    pf.begin("warp_tangent_dgrad", 3.0 * warp_dgrad_flops_row(h) * p.rows[0], stream);
    if (bf16_trunk()) launch_warp_bwd_bf16(ta, nullptr, nullptr, h->num_cus, stream);
    else launch_warp_bwd(ta, nullptr, nullptr, tile_grid(p.ntiles[TG], warp_grid_mul(), h->num_cus), stream);
    pf.end(stream);
  }

  void cond_grads() {
    const float* dray1 = h->nlevels > 1 ? ws + p.L[1].dray : nullptr;
    pf.begin("cond_wgrad", 0, stream);
    launch_cond_wgrad(ws + p.cond, ws + p.L[0].dray, dray1, B, h->R, ws + p.L[0].cond_grad, h->nlevels > 1 ? ws + p.L[1].cond_grad : nullptr, stream);
    launch_cond_embed_grad(params, ws + p.L[0].dray, dray1, rays->appearance_ids, rays->camera_ids, B, h->V,
                           h->app_in_cond ? d.num_appearance_features : 0, h->app_off, d.use_camera_metadata ? d.num_camera_features : 0,
                           h->cam_off, h->po[0].rgbh_k, h->po[h->nlevels > 1 ? 1 : 0].rgbh_k, grad, stream);
    for (int lv = 0; lv < h->nlevels && h->A > 0; ++lv)   // appearance-code rows of the alpha head, the codes' gradient through it (modules.py:152-157)
      launch_alpha_cond_grad(params, ws + p.cond, ws + p.L[lv].dsig_ray, rays->appearance_ids, B, h->R, h->V, h->A, h->app_off,
                             h->po[lv].alpha_k, grad, stream);
    pf.end(stream);
  }

  void wgrad() {
    // the SE3 groups also run over the background rows and, with the elastic regulariser, over the three tangent rows per
    // coarse sample (warping.py:385-387 jacfwd): algorithmic work of the step, counted
    const double warp_rows = m.warp_on ? mlp_rows + (bg_on ? p.key.bgN : 0) + (el_on ? 3.0 * p.rows[0] : 0.0) : 0.0;
    if (!p.segs.empty()) {
      pf.begin("wgrad", (m.bf16 ? 0.0 : wgrad_flops_row(h)) * mlp_rows + warp_fwd_flops_row_or0(h) * warp_rows, stream);
      launch_wgrad(table<WgradGroup>(p.groups_off_b), table<WgradSegment>(p.segs_off_b), table<int>(p.segbegin_off_b), p.wgrad_nwg, ws,
                   reinterpret_cast<unsigned long long*>(ws + p.seg_clock), stream);
      pf.end(stream);
    }
    if (!p.bsegs.empty()) {
      pf.begin("wgrad_bf16", wgrad_flops_row(h) * mlp_rows + (bf16_trunk() ? warp_fwd_flops_row_or0(h) * warp_rows : 0.0), stream);
      launch_wgrad_bf16(table<WgradGroup>(p.bgroups_off_b), table<WgradSegment>(p.bsegs_off_b), table<int>(p.bsegbegin_off_b),
                        p.bwgrad_nwg, ws, stream);
      pf.end(stream);
    }
  }
  // reduce into the gradient, its copy-out for a narrower model, the step's statistics
  int reduce_and_finish(float* grad_x, float* stats) {
    pf.begin("grad_reduce", 0, stream);
    const ReduceDesc* rd = table<ReduceDesc>(p.reduce_off_b);
    // one launch: the grid's columns are the chain heads, the later passes into shared leaves (SE3 field) hang behind them (nrf_plan.hip)
    if (p.nreduce_pass[0] > 0) launch_reduce(rd, 0, p.nreduce_pass[0], ws, grad, stream);
    if (p.nreduce_pass[2] > 0) launch_reduce(rd, p.nreduce_pass[0] + p.nreduce_pass[1], p.nreduce_pass[2], ws, grad, stream);
    if (h->embed) {
      hipError_t e = hipMemsetAsync(grad_x, 0, (size_t)h->xnparams * sizeof(float), stream);
      if (e != hipSuccess) return fail_hip(e, "zero grad");
      launch_embed(table<EmbedDesc>(p.emb_off_b), (int)h->emb.size(), grad, grad_x, false, stream);
    }
    if (stats) finish_stats(stats);
    pf.end(stream);
    return NRF_OK;
  }
  void finish_stats(float* stats) {   // the step's statistics from the per-ray / per-workgroup sums the reverse kernels left
    StatsArgs sa;
    memset(&sa, 0, sizeof(sa));
    sa.mse_ray = ws + p.mse; sa.B = B; sa.nlevels = h->nlevels;
    if (bg_on) { sa.bg_sum = ws + p.bg_loss; sa.bgN = p.key.bgN; sa.bg_weight = bg->loss_weight; }
    if (el_on) {
      sa.el_part = ws + p.el_sums; sa.el_nwg = (rows_pad(0) + 255) / 256; sa.el_jac_rows = p.rows[0]; sa.el_weight = el->loss_weight;
      sa.el_rows = el->reduce_method == NRF_ELASTIC_MEDIAN ? B : p.rows[0];
    }
    if (wr_on) { sa.wr_sums = ws + p.wr_sums; sa.wr_weight = wr->loss_weight; }
    sa.stats = stats; sa.dyn = dyn();
    launch_finish_stats(sa, stream);
  }
};

}  // namespace

int forward_impl(nrf_handle h, const float* params_x, const nrf_rays* rays, const nrf_step_scalars* scalars, const nrf_rand* rnd,
                 const nrf_outputs* out, uint32_t flags, float* ws, size_t ws_bytes, hipStream_t stream, int bgN,
                 int elastic, const nrf_background* bg) {
  CK(validate_rays(h, rays));
  if (!params_x || !ws) return fail(NRF_E_NULL, "params / workspace is null");
  query_device(h);
  build_plan(h, rays->num_rays, flags, bgN, elastic);
  Forward f(Run(h, forward_modes(h, flags), ws, stream, rays, scalars, bg), rnd, out);
  CK(f.checks(ws_bytes));
  CK(f.prepare(params_x));
  for (int lv = 0; lv < h->nlevels; ++lv) {
    if (lv == 1) f.sample_fine();
    if (f.m.warp_on) { f.warp(lv); f.jacobian(lv); }
    f.mlp(lv);
    f.composite(lv);
    CK(f.outputs(lv));
  }
  CK(check_launch("nrf_forward"));
  h->stashed_ws = f.m.train ? (void*)ws : nullptr;
  h->stashed_plan = f.m.train ? h->plan.serial : 0;
  h->stashed_B = f.m.train ? rays->num_rays : -1;
  h->stashed_modes = f.m;
  return NRF_OK;
}

// og != nullptr: upstream gradient mode, the cotangents of the rendered outputs (nrf_backward[_ex]; d_rgb of every level set by the
// caller); else MSE-loss mode against `target` (the fused train step).
// Launch order (round 3): the reverse passes of the two levels are independent, so every kernel type runs ONCE
// over the tiles of all levels -- composite_bwd x levels, ONE NeRF-MLP dgrad launch (coarse + fine tiles), the regularisers'
// point gradients, ONE SE3 dgrad launch (coarse + fine + background tiles), the tangent pass, then wgrad / reduce.
int backward_impl(nrf_handle h, const float* params_x, const nrf_rays* rays, const nrf_output_grads* og, const float* target,
                  float* grad_x, float* stats, float* ws, hipStream_t stream, const nrf_background* bg,
                  const nrf_step_scalars* scalars, const nrf_elastic* el, const nrf_warp_reg* wr, bool bg_forward_done,
                  const nrf_ray_grads* rg) {
  Backward b(Run(h, h->stashed_modes, ws, stream, rays, scalars, bg), el, wr, og);
  // nothing asked for: the stage (and its inputs) are skipped
  if (rg && (rg->d_origins || rg->d_directions || rg->d_viewdirs)) b.rg = rg;
  // the fused step's ray gradients: with rays->viewdirs NULL the view term is folded into d_directions
  b.fold_viewdirs = og == nullptr && rg != nullptr;
  // the gradient buffer is zero-filled and accumulated into with 16-byte accesses (zero_ranges_kernel, reduce passes)
  if ((reinterpret_cast<uintptr_t>(grad_x) & 15u) != 0) return fail(NRF_E_SHAPE, "grad_params must be 16-byte aligned");
  // p.bwd32 alone selects the 32-row reverse path (zeroed slices and launch); that kernel has no d-points output
  if (b.p.bwd32 && b.m.warp_on) return fail(NRF_E_STATE, "plan built for the 32-row reverse chain but the stashed forward ran the warp field");
  if (b.p.bwd32 && b.rg) return fail(NRF_E_STATE, "plan built for the 32-row reverse chain but ray gradients (NRF_FLAG_RAY_GRADS) are asked for");
  // the background batch's warp forward ran inside the coarse warp launch of the fused train step
  if (b.bg_on && !bg_forward_done) return fail(NRF_E_STATE, "background regulariser without its forward pass");
  // narrower model: the stashed forward left the padded parameter image in the workspace; gradients are formed
  // in the padded layout and copied out at the end
  b.params = h->embed ? ws + b.p.iparams : params_x;
  b.grad = h->embed ? ws + b.p.igrad : grad_x;
  CK(b.zero());
  b.composite_bwd(target);
  b.mlp_dgrad();
  b.point_cotangents();
  if (b.rg) b.ray_grads();
  b.point_regularisers();   // behind the ray stage: launch_warp_reg adds into d_points
  if (b.m.warp_on) b.warp_dgrad();
  b.cond_grads();
  if (b.m.warp_on && h->time_enc) {   // reverse of the TimeEncoder: d codes -> its six layers' weight gradients
    launch_time_encoder_bwd(b.time_enc_args(true), stream);
    launch_time_encoder_wgrad(b.time_enc_args(true), b.grad, stream);
  }
  b.wgrad();
  CK(b.reduce_and_finish(grad_x, stats));
  return check_launch("nrf_backward");
}

// The reverse pass of a frozen stash (NRF_FLAG_FROZEN), which keeps what the rays' gradient reads and nothing else: composite_bwd,
// ONE 64-row NeRF data-gradient launch without dY images or bias partials, the caller's warped-point cotangent, the ray stage.  No SE3
// dgrad (the warp Jacobians were formed in the forward), no condition / GLO / time-encoder gradients, no wgrad, no reduce pass.
int backward_rays_frozen_impl(nrf_handle h, const float* params_x, const nrf_rays* rays, const nrf_output_grads* og, const float* target,
                              const nrf_ray_grads* rg, float* stats, float* ws, hipStream_t stream, const nrf_step_scalars* scalars) {
  Backward b(Run(h, h->stashed_modes, ws, stream, rays, scalars, nullptr), nullptr, nullptr, og);
  if (!b.m.frozen || b.p.bwd32) return fail(NRF_E_STATE, "the stashed forward did not run under NRF_FLAG_FROZEN");
  if (rg->d_origins || rg->d_directions || rg->d_viewdirs) b.rg = rg;
  b.fold_viewdirs = og == nullptr;   // the fused step: rays->viewdirs == NULL adds the view term to d_directions
  b.params = h->embed ? ws + b.p.iparams : params_x;   // narrower model: the forward left its padded image in the workspace
  CK(b.zero());
  b.composite_bwd(target);
  b.mlp_dgrad();
  b.point_cotangents();
  if (b.rg) b.ray_grads();
  if (stats) b.finish_stats(stats);
  return check_launch("nrf_backward_rays (frozen)");
}

}  // namespace api
}  // namespace nrf
