// Stand-alone field entries of the C-ABI layer: parts of the field run outside the ray plan, on the ray path's own builders
// (nrf_handle.h).  Each carves a small plan of its own: h->plan is neither read nor written, so a ray plan's digest and a pending
// nrf_backward are as they were -- unless the entry is handed the very memory that plan's tables or stash live in (forget_workspace).
#include "nrf_handle.h"

using namespace nrf;
using namespace nrf::api;

namespace {
// an entry writes over what a ray plan keeps in `ws`: its tables and stash are forgotten instead of left stale
void forget_workspace(nrf_handle h, const void* ws) {
  if (h->uploaded_ws == ws) h->uploaded_ws = nullptr;   // a following nrf_forward uploads its tables again
  if (h->stashed_ws == ws) h->stashed_ws = nullptr;     // a following nrf_backward is refused (NRF_E_STATE)
}
// a model narrower than the kernels runs on its zero-padded image: the embed table to ws + emb_f, the image at ws + ip_f (as
// embed_params).  Every side plan derives from this; which models need the image is the plan's own condition
struct PaddedImage {
  size_t emb_f = 0, ip_f = 0;
  void carve(Carve& c, const nrf_handle_s* h) {
    emb_f = c.take((h->emb.size() + 1) * sizeof(EmbedDesc) / 4);
    ip_f = c.take((size_t)h->nparams);
  }
};
const float* embed_side(nrf_handle h, const float* params_x, float* ws, const PaddedImage& p, hipStream_t st) {
  const hipError_t e = hipMemcpyAsync(ws + p.emb_f, h->emb.data(), h->emb.size() * sizeof(EmbedDesc), hipMemcpyHostToDevice, st);
  if (e != hipSuccess) { fail_hip(e, "upload embed table"); return nullptr; }
  return embed_params(h, params_x, reinterpret_cast<const EmbedDesc*>(ws + p.emb_f), ws + p.ip_f, false, st);
}
// the entry's pack table, rebuilt when what it was built for changes
template <class Build> void refresh(SidePack& c, int64_t key, Build build) {
  if (c.key == key) return;
  c.descs.clear();
  build(c.descs);
  c.key = key;
}
int upload_pack_table(const SidePack& pack, float* dst, const char* what, hipStream_t st) {
  const hipError_t e = hipMemcpyAsync(dst, pack.descs.data(), pack.descs.size() * sizeof(PackDesc), hipMemcpyHostToDevice, st);
  return e == hipSuccess ? NRF_OK : fail_hip(e, what);
}
// how every entry ends: the warped points (where asked for) out of the workspace's padded rows, then the launches' verdict
int finish_entry(const char* entry, float* warped_points, const float* ws_rows, int n, hipStream_t st) {
  if (warped_points) {
    const hipError_t e = hipMemcpyAsync(warped_points, ws_rows, (size_t)n * 3 * sizeof(float), hipMemcpyDeviceToDevice, st);
    if (e != hipSuccess) return fail_hip(e, "copy warped points");
  }
  return check_launch(entry);
}

// ---- Stand-alone SE3 field on arbitrary points (create_warp_field(num_batch_dims=1), models.py:165-184; the field
// training.compute_background_loss applies, training.py:127-130).  Workspace:
// [pack descriptors | packed trunk weights | padded output | tile counter | embed table, padded params (narrow trunks)]
struct WarpPointsPlan : PaddedImage { size_t desc_f, wpk_f, out_f, ctr_f, total_f; int ntiles; };
WarpPointsPlan warp_points_plan(nrf_handle h, int n) {
  WarpPointsPlan q;
  q.ntiles = (n + TILE_ROWS - 1) / TILE_ROWS;
  Carve c;
  q.desc_f = c.take(16 * sizeof(PackDesc) / 4);
  q.wpk_f = c.take(h->wpk.total);
  q.out_f = c.take((size_t)q.ntiles * TILE_ROWS * 3);
  q.ctr_f = c.take(16);
  // no rotation head in the caller's tree, or a trunk shallower / narrower than the kernels': run on the padded image
  if (h->d.warp_field_type == NRF_WARP_TRANSLATION || h->wxdepth != WARP_DEPTH || h->wxwidth != WARP_W) q.carve(c, h);
  q.total_f = c.o;
  return q;
}

// ---- The field inverted (nrf_unwarp_points): Newton's iteration on W(x; id) = y around the SE3 trunk's primal and tangent passes,
// the launches of a gradient query's warp part.  Workspace, every per-row buffer of ntiles * 64 rows:
// [pack descriptors | packed trunk | x | trunk-input stash | sign words | (w, v) | tangent (dw, dv) | warped | per-row state ||
//  embed table, padded params (narrow / translation trunks)]
// The caller's ids are read where they are (one per point: the kernel's own prologue), and the SE3 kernels hand their tiles out
// statically: the plan holds no copy of the ids and no tile counter.
struct UnwarpPlan : PaddedImage {
  size_t desc_f, wpk_f, x_f, win_f, bits_f, wv_f, twv_f, warped_f, state_f, total_f;
  int ntiles;
  size_t rows_pad() const { return (size_t)ntiles * TILE_ROWS; }
};
UnwarpPlan unwarp_plan(const nrf_handle_s* h, int n) {
  UnwarpPlan q;
  q.ntiles = (n + TILE_ROWS - 1) / TILE_ROWS;
  const size_t rows_pad = q.rows_pad();
  const int PKSw = (h->PKw + 31) / 32 * 32;
  Carve c;
  q.desc_f = c.take(16 * sizeof(PackDesc) / 4);
  q.wpk_f = c.take(h->wpk.total);
  q.x_f = c.take(rows_pad * 3);
  q.win_f = c.take((size_t)q.ntiles * PKSw * TILE_ROWS);
  q.bits_f = c.take((size_t)WARP_DEPTH * q.ntiles * 4 * 64);
  q.wv_f = c.take(rows_pad * 8);
  q.twv_f = c.take(3 * rows_pad * 8);   // 3 tangent tiles per primal tile
  q.warped_f = c.take(rows_pad * 3);
  q.state_f = c.take(rows_pad);
  if (h->d.warp_field_type == NRF_WARP_TRANSLATION || h->wxdepth != WARP_DEPTH || h->wxwidth != WARP_W) q.carve(c, h);   // as WarpPointsPlan
  q.total_f = c.o;
  return q;
}

// what both unwarp entries check of the handle and the count
int unwarp_model(const char* entry, const nrf_handle_s* h, int n) {
  const auto refuse = [&](int code, const char* rule) {
    snprintf(g_err, sizeof(g_err), "%s: %s", entry, rule);
    return code;
  };
  if (!h->warp) return refuse(NRF_E_UNSUPPORTED, "the model has no warp field");
  if (h->time_enc) return refuse(NRF_E_UNSUPPORTED, "takes warp ids or codes: not built for the time encoder");
  if (n <= 0 || n > NRF_UNWARP_MAX_POINTS) return refuse(NRF_E_SHAPE, "num_points must be in 1..NRF_UNWARP_MAX_POINTS (1 << 20); callers chunk");
  return NRF_OK;
}

// ---- Field queries, value (nrf_query_points / nrf_query_grid) and gradient (nrf_query_points_grad / nrf_query_grid_grad): what both
// plans hold, in this order, before their own tails:
// [pack descriptors | embed table | padded params | images of one MLP | SE3 trunk image | tile counters |
//  cond, condterm, alpha_ct of G groups | points of a grid || warp: per-point code rows | warped points]
// Every per-row buffer holds ntiles * 64 rows.
struct QueryBase : PaddedImage {
  size_t desc_f, wpk_f, wwpk_f, ctr_f, cond_f, condterm_f, alpha_ct_f, points_f, ids_f = 0, wpoints_f = 0, total_f;
  int N, ntiles;
  size_t rows_pad() const { return (size_t)ntiles * TILE_ROWS; }
};
// carves the shared regions (mlp_image_f: the floats of the plan's MLP image) and hands the carver on for the plan's tail
Carve query_base(QueryBase& q, const nrf_handle_s* h, int G, int S, int max_descs, size_t mlp_image_f) {
  q.N = G * S;
  q.ntiles = (q.N + TILE_ROWS - 1) / TILE_ROWS;
  Carve c;
  q.desc_f = c.take(max_descs * sizeof(PackDesc) / 4);
  if (h->embed) q.carve(c, h);
  q.wpk_f = c.take(mlp_image_f);
  q.wwpk_f = h->warp ? c.take(h->wpk.total) : 0;
  q.ctr_f = c.take(16);
  q.cond_f = c.take((size_t)G * (h->R > 0 ? h->R : 1));
  q.condterm_f = c.take((size_t)G * RGB_W);
  q.alpha_ct_f = c.take((size_t)G);
  q.points_f = c.take(q.rows_pad() * 3);   // a grid entry forms its points here
  if (h->warp) {
    q.ids_f = c.take(q.rows_pad());
    q.wpoints_f = c.take(q.rows_pad() * 3);
  }
  return c;
}

// what the two kinds of query say differently around the shared steps
struct QueryKind { int max_descs; const char *prep, *too_large, *upload, *too_small; };
// 11 + rgb branch layers 1..3 + 7 of the SE3 trunk
constexpr QueryKind VALUE_QUERY = {32, "query_prep", "field query: pack table larger than its workspace region", "upload query pack table",
                                   "workspace too small (see nrf_query_workspace_bytes)"};
// 11 + 9 transposed + 2 d-posenc + 3 x 2 rgb branch layers + 7 of the SE3 trunk
constexpr QueryKind GRAD_QUERY = {48, "qgrad_prep", "gradient query: pack table larger than its workspace region",
                                  "upload gradient query pack table", "workspace too small (see nrf_query_grad_workspace_bytes)"};

// The value query: render_samples up to the activations (models.py:230-277) at the caller's points.  Tail: [out4]
struct QueryPlan : QueryBase { size_t out4_f; };
QueryPlan query_plan(const nrf_handle_s* h, int G, int S) {
  QueryPlan q;
  Carve c = query_base(q, h, G, S, VALUE_QUERY.max_descs, h->pk.total);
  q.out4_f = c.take(q.rows_pad() * 4);
  q.total_f = c.o;
  return q;
}

// The gradient query: the density chain keeping its sign words and posenc stash, the reverse chain from the density to the point, the
// warp Jacobian of the row.  The MLP image holds the forward and transposed images, W0^T / skip rows^T behind them on a model without
// a warp field.  Tail:
// [sign words | posenc stash | sigma'(raw) | d points || warp: trunk input | sign words | (w, v) | tangent (dw, dv) | Jacobian]
// The reverse chain writes d_points for whole tiles and the stashes are indexed by tile.
struct QueryGradPlan : QueryBase {
  size_t bits_f, pe_f, dsig_f, dpoints_f, w_win_f = 0, w_bits_f = 0, w_wv_f = 0, t_wv_f = 0, jac_f = 0;
  int L0T, L4bT;   // PackOffsets::bwd_L0T / bwd_L4bT inside the image at wpk_f
};
QueryGradPlan query_grad_plan(const nrf_handle_s* h, int G, int S) {
  QueryGradPlan q;
  // a warp model's PackOffsets hold the two d-posenc images; without a warp field they follow the level's own images and their
  // prefetch slack (as a ray-gradient plan places them, nrf_plan.hip rg_wpkT)
  q.L0T = h->warp ? h->pk.bwd_L0T : h->pk.total;
  q.L4bT = h->warp ? h->pk.bwd_L4bT : h->pk.total + 256 * 64;
  Carve c = query_base(q, h, G, S, GRAD_QUERY.max_descs, h->warp ? (size_t)h->pk.total : (size_t)q.L4bT + 256 * 64 + 4096);
  const size_t rows_pad = q.rows_pad();
  const int PKS = (h->PK + 31) / 32 * 32;
  q.bits_f = c.take((size_t)TRUNK_DEPTH * q.ntiles * 4 * 128);      // 8 layers x tile x 4 waves x 128 words: 256 B per row
  q.pe_f = c.take((size_t)q.ntiles * PKS * TILE_ROWS);              // [PKS][64] per tile: 4 PKS B per row
  q.dsig_f = c.take(rows_pad);
  q.dpoints_f = c.take(rows_pad * 3);
  if (h->warp) {
    const int PKSw = (h->PKw + 31) / 32 * 32;
    q.w_win_f = c.take((size_t)q.ntiles * PKSw * TILE_ROWS);
    q.w_bits_f = c.take((size_t)WARP_DEPTH * q.ntiles * 4 * 64);
    q.w_wv_f = c.take(rows_pad * 8);
    q.t_wv_f = c.take(3 * rows_pad * 8);                            // 3 tangent tiles per primal tile
    q.jac_f = c.take(rows_pad * 9);
  }
  q.total_f = c.o;
  return q;
}

// the flag word of a query: 0 or NRF_FLAG_NO_WARP; every other bit by its name
int query_flags(uint32_t flags) {
  for (const FlagName& f : FLAG_NAMES)
    if (flags & f.bit & ~(uint32_t)NRF_FLAG_NO_WARP) {
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

int query_grad_shape(int G, int S) {
  CK(query_shape(G, S));
  if ((int64_t)G * S > NRF_QUERY_GRAD_MAX_POINTS)
    return fail(NRF_E_SHAPE, "a gradient query takes at most 1 << 20 points per call (NRF_QUERY_GRAD_MAX_POINTS)");
  return NRF_OK;
}

// what the value entries check of everything but the points
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
  return require_ids_or_codes(h, groups, out->rgb != nullptr, out->rgb || out->sigma, warp_on);
}

// ... and the gradient entries: a density-only query's rules and the smaller point cap
int query_grad_args(nrf_handle h, const float* params, const nrf_rays* groups, int S, int level, const nrf_step_scalars* sc, uint32_t flags,
                    const nrf_field_grad_out* out, const void* workspace) {
  if (h && params && groups && sc && !out) return fail(NRF_E_NULL, "out (nrf_field_grad_out) is null");
  float always = 0.f;   // the density is computed whatever the caller asks for: the ids it needs are required
  const nrf_field_out as_density = {&always, nullptr, out ? out->warped_points : nullptr};
  CK(query_args(h, params, groups, S, level, sc, flags, &as_density, workspace));
  return query_grad_shape(groups->num_rays, S);
}

// what the grid entries check of the grid and the range inside it
int grid_range(const char* entry, const nrf_rays* group, const nrf_grid* grid, int64_t first, int count) {
  if (group->num_rays != 1) {
    snprintf(g_err, sizeof(g_err), "%s: group->num_rays must be 1 (one condition for the whole grid)", entry);
    return NRF_E_SHAPE;
  }
  if (grid->dims[0] <= 0 || grid->dims[1] <= 0 || grid->dims[2] <= 0) return fail(NRF_E_SHAPE, "grid dims must be positive");
  // at most 2^40 points in a grid: the product of three int32 extents cannot wrap int64 behind this
  const int64_t plane = (int64_t)grid->dims[0] * grid->dims[1];
  if (plane > NRF_GRID_MAX_POINTS || plane * grid->dims[2] > NRF_GRID_MAX_POINTS)
    return fail(NRF_E_SHAPE, "grid dims: more than NRF_GRID_MAX_POINTS (1 << 40) points in dims[0] * dims[1] * dims[2]");
  const int64_t total = plane * grid->dims[2];
  if (first < 0 || first + count > total) return fail(NRF_E_SHAPE, "first + count runs beyond the grid (dims[0] * dims[1] * dims[2] points)");
  return NRF_OK;
}

// How both kinds of query begin: the padded image, the pack table of `level` (rebuilt by `build` when the level changes: the offsets do
// not depend on the number of points), the counters, and the kind's prep region -- the pack kernel and the per-group terms
// (models.py:186-228).  `full`: the condition term of a query with colour; otherwise only a use_alpha_condition model has a term, the
// appearance code's of the alpha head, so ray_prep runs on the appearance columns alone (same kernel, same fmaf chain: the same
// alpha_ct bits) and no view direction or camera code is read.  *params: what the launches behind read
template <class Build>
int query_prologue(nrf_handle h, const QueryKind& k, SidePack& pack, Build build, const float* params_x, const nrf_rays* groups, int level,
                   bool full, float* ws, const QueryBase& q, hipStream_t st, const float** params) {
  query_device(h);
  forget_workspace(h, ws);
  *params = params_x;
  if (h->embed && !(*params = embed_side(h, params_x, ws, q, st))) return NRF_E_HIP;
  refresh(pack, level, build);
  if ((int)pack.descs.size() > k.max_descs) return fail(NRF_E_STATE, k.too_large);
  CK(upload_pack_table(pack, ws + q.desc_f, k.upload, st));
  if (tile_counter_or_null(ws + q.ctr_f, 0)) {   // NRF_DYNAMIC_TILES experiment only
    const hipError_t e = hipMemsetAsync(ws + q.ctr_f, 0, 16 * sizeof(int), st);
    if (e != hipSuccess) return fail_hip(e, "zero tile counters");
  }
  h->prof.begin(k.prep, 0, st);   // no return between a begin and its end
  launch_pack(reinterpret_cast<const PackDesc*>(ws + q.desc_f), (int)pack.descs.size(), *params, ws, st);
  if (full || h->A > 0) {
    const RayPrepLevel lv{level, ws + q.condterm_f, ws + q.alpha_ct_f};
    launch_ray_prep(ray_prep_args(h, *params, groups, groups->viewdirs, ws + q.cond_f, &lv, 1, !full), st);
  }
  h->prof.end(st);
  return NRF_OK;
}

// The primal SE3 launch of a query, its per-point rows of the code table written: group g's id, or row g of the caller's codes
// (metadata_encoded).  The SE3 kernel has two prologues: `row / S` ids together with x = o + z d formed from rays, or explicit points
// together with ONE ID PER POINT (warp_chain.hip: points_in -> point_ids[r]); explicit points with per-group ids is neither, and giving
// the kernel a third would change a kernel every plan runs.  So the ids are written out: 4 bytes per row next to a trunk of 1.6e5
// MACs, below the resolution of the 128^3 measurement (profiles/field_query.md)
WarpFwdArgs query_warp_args(nrf_handle h, const float* params, const nrf_rays* groups, const float* points, int S,
                            const nrf_step_scalars* sc, float* ws, const QueryBase& q, hipStream_t st) {
  int32_t* ids = reinterpret_cast<int32_t*>(ws + q.ids_f);
  launch_field_ids(groups->warp_codes ? nullptr : groups->warp_ids, q.N, S, ids, st);
  WarpFwdArgs wa = warp_points_args(h, params, h->wpo, ws + q.wwpk_f, sc, points, ids, q.N, ws + q.wpoints_f);
  if (groups->warp_codes) wa.embed_table = groups->warp_codes;
  wa.tile_counter = tile_counter_or_null(ws + q.ctr_f, 0);
  return wa;
}

// a value query behind its entry's checks
int query_impl(const char* entry, nrf_handle h, const float* params_x, const nrf_rays* groups, const float* points, int S, int level,
               const nrf_step_scalars* sc, uint32_t flags, const nrf_field_out* out, float* ws, const QueryPlan& q, hipStream_t st) {
  const int G = groups->num_rays, N = q.N;
  const bool warp_on = h->warp && !(flags & NRF_FLAG_NO_WARP);
  const bool full = out->rgb != nullptr;
  Prof& pf = h->prof;
  // forward image of the asked level at the handle's PackOffsets (the transposed images' room stays unwritten and unread), and the
  // SE3 trunk's
  const auto build = [&](std::vector<PackDesc>& v) {
    mlp_pack_descs(h, level, (int64_t)q.wpk_f, false, v);
    if (h->warp) warp_pack_descs(h, h->wpo, (int64_t)q.wwpk_f, false, v);
  };
  const float* params;
  CK(query_prologue(h, VALUE_QUERY, h->q_pack, build, params_x, groups, level, full, ws, q, st, &params));
  if (warp_on) {
    const WarpFwdArgs wa = query_warp_args(h, params, groups, points, S, sc, ws, q, st);
    pf.begin("query_warp", warp_fwd_flops_row(h) * N, st);
    launch_warp_fwd(wa, nullptr, false, tile_grid(wa.ntiles, warp_grid_mul(), h->num_cus), st);
    pf.end(st);
    points = ws + q.wpoints_f;
  }
  ChainFwdArgs a = chain_model_args(h, params, level, ws + q.alpha_ct_f);
  a.wpk = ws + q.wpk_f; a.condterm = ws + q.condterm_f; a.points = points; a.out4 = reinterpret_cast<float4*>(ws + q.out4_f);
  a.S = S; a.B = G; a.rows = N; a.ntiles = q.ntiles;
  a.tile_counter = tile_counter_or_null(ws + q.ctr_f, 1);
  const ChainTiling t = chain_fwd_tiling(h, q.ntiles, full);   // the density chain is built on 64-row tiles only (chain_query.hip)
  a.k_old = t.k_old;
  if (full) {
    pf.begin("query_mlp", fwd_flops_row(h) * N, st);
    if (t.c32) launch_chain_fwd32(a, false, t.grid, st);
    else launch_chain_fwd(a, false, t.grid, st);
    pf.end(st);
    pf.begin("query_unpack", 0, st);
    launch_field_unpack(a.out4, N, out->sigma, out->rgb, st);
    pf.end(st);
  } else if (out->sigma) {
    pf.begin("query_density", density_flops_row(h) * N, st);
    launch_chain_density(a, out->sigma, t.grid, st);
    pf.end(st);
  }
  return finish_entry(entry, out->warped_points, ws + q.wpoints_f, N, st);
}

// a gradient query behind its entry's checks
int query_grad_impl(const char* entry, nrf_handle h, const float* params_x, const nrf_rays* groups, const float* points, int S, int level,
                    const nrf_step_scalars* sc, uint32_t flags, const nrf_field_grad_out* out, float* ws, const QueryGradPlan& q,
                    hipStream_t st) {
  const int G = groups->num_rays, N = q.N;
  const bool warp_on = h->warp && !(flags & NRF_FLAG_NO_WARP);
  Prof& pf = h->prof;
  // forward and transposed images of the asked level, the two d-posenc images, the SE3 trunk's forward image
  const auto build = [&](std::vector<PackDesc>& v) {
    mlp_pack_descs(h, level, (int64_t)q.wpk_f, true, v);
    if (!h->warp) {   // mlp_pack_descs adds them for a warp model, at its PackOffsets
      const MlpParamOffsets& po = h->po[level];
      v.push_back(PackDesc{po.trunk_k[0], (int64_t)q.wpk_f + q.L0T, 256, 0, 256, 256, 2, 1, 1, h->P});
      v.push_back(PackDesc{po.trunk_k[h->d.nerf_skip_layer], (int64_t)q.wpk_f + q.L4bT, 256, 256, 256, 256, 2, 1, 1, h->P});
    }
    if (h->warp) warp_pack_descs(h, h->wpo, (int64_t)q.wwpk_f, false, v);
  };
  const float* params;
  CK(query_prologue(h, GRAD_QUERY, h->qg_pack, build, params_x, groups, level, false, ws, q, st, &params));
  if (warp_on) {
    // the primal SE3 forward keeping what a frozen ray plan keeps (trunk input, sign words, (w, v)); its tangent pass, three tangent
    // tiles per primal tile; the Jacobian of every row
    const int PKSw = (h->PKw + 31) / 32 * 32;
    WarpFwdArgs wa = query_warp_args(h, params, groups, points, S, sc, ws, q, st);
    wa.st_win = ws + q.w_win_f; wa.st_wv = reinterpret_cast<float4*>(ws + q.w_wv_f); wa.bits = reinterpret_cast<uint32_t*>(ws + q.w_bits_f);
    pf.begin("qgrad_warp", warp_fwd_flops_row(h) * N, st);
    launch_warp_fwd(wa, nullptr, true, tile_grid(wa.ntiles, warp_grid_mul(), h->num_cus), st, true);
    pf.end(st);
    WarpFwdArgs ta = wa;
    ta.nt_prim = q.ntiles; ta.prim_win = wa.st_win; ta.prim_bits = wa.bits;
    ta.ntiles = 3 * q.ntiles; ta.rows = ta.ntiles * TILE_ROWS;
    ta.st_win = nullptr; ta.bits = nullptr; ta.points_out = nullptr; ta.st_wv = reinterpret_cast<float4*>(ws + q.t_wv_f);
    ta.tile_counter = tile_counter_or_null(ws + q.ctr_f, 2);
    pf.begin("qgrad_tangent", 3.0 * warp_fwd_flops_row(h) * N, st);
    launch_warp_fwd(ta, nullptr, true, tile_grid(ta.ntiles, warp_grid_mul(), h->num_cus), st, true);
    pf.end(st);
    JacobianArgs ja;
    memset(&ja, 0, sizeof(ja));   // x_rows = nullptr: the points come from the trunk-input stash
    ja.prim_win = wa.st_win; ja.prim_wv = wa.st_wv; ja.tan_wv = ta.st_wv; ja.out = ws + q.jac_f;
    ja.rows = N; ja.rows_pad = q.ntiles * TILE_ROWS; ja.PKS = PKSw;
    pf.begin("qgrad_jacobian", 0, st);
    launch_jacobian(ja, st);
    pf.end(st);
    points = ws + q.wpoints_f;
  }
  ChainFwdArgs a = chain_model_args(h, params, level, ws + q.alpha_ct_f);
  a.wpk = ws + q.wpk_f; a.points = points; a.S = S; a.B = G; a.rows = N; a.ntiles = q.ntiles;
  a.st_pe = ws + q.pe_f; a.bits_trunk = reinterpret_cast<uint32_t*>(ws + q.bits_f);
  a.tile_counter = tile_counter_or_null(ws + q.ctr_f, 1);
  const ChainTiling t = chain_fwd_tiling(h, q.ntiles, false);   // 64-row tiles only (chain_query_grad.hip)
  a.k_old = t.k_old;
  pf.begin("qgrad_fwd", density_flops_row(h) * N, st);
  launch_chain_density_stash(a, out->sigma, ws + q.dsig_f, t.grid, st);
  pf.end(st);
  ChainBwdArgs b;
  memset(&b, 0, sizeof(b));
  b.params = params; b.po = a.po; b.wpk = a.wpk; b.pk = a.pk; b.pk.bwd_L0T = q.L0T; b.pk.bwd_L4bT = q.L4bT;
  b.S = S; b.B = G; b.rows = N; b.ntiles = q.ntiles;
  b.bits_trunk = a.bits_trunk; b.st_pe = a.st_pe; b.d_points = ws + q.dpoints_f;
  b.F = a.F; b.P = a.P; b.PK = a.PK; b.skip = a.skip; b.alpha_on_bn = h->A > 0;
  pf.begin("qgrad_bwd", density_bwd_flops_row(h) * N, st);
  launch_chain_density_bwd(b, ws + q.dsig_f, t.grid, st);
  pf.end(st);
  if (out->grad_sigma || out->normals) {
    pf.begin("qgrad_finish", 0, st);
    launch_field_grad_finish(ws + q.dpoints_f, warp_on ? ws + q.jac_f : nullptr, N, out->grad_sigma, out->normals, st);
    pf.end(st);
  }
  return finish_entry(entry, out->warped_points, ws + q.wpoints_f, N, st);
}

// The four query entries, each kind made of its argument checks, its plan and its launches: at the caller's `points`, or (on_grid) at
// points [first, first + S) of `grid`, formed on the device in the plan's own region
template <const QueryKind& K, auto Args, auto Plan, auto Impl, class Out>
int query_entry(const char* entry, bool on_grid, nrf_handle h, const float* params, const nrf_rays* groups, const float* points,
                const nrf_grid* grid, int64_t first, int S, int level, const nrf_step_scalars* sc, uint32_t flags, const Out* out,
                void* workspace, size_t workspace_bytes, void* stream) {
  if (h && !(on_grid ? (const void*)grid : points)) return fail(NRF_E_NULL, on_grid ? "grid is null" : "points is null");
  CK(Args(h, params, groups, S, level, sc, flags, out, workspace));
  if (on_grid) CK(grid_range(entry, groups, grid, first, S));
  const auto q = Plan(h, groups->num_rays, S);
  if (workspace_bytes < q.total_f * sizeof(float)) return fail(NRF_E_WORKSPACE, K.too_small);
  float* ws = (float*)workspace;
  hipStream_t st = (hipStream_t)stream;
  if (on_grid) {
    launch_grid_points(*grid, first, S, ws + q.points_f, st);
    points = ws + q.points_f;
  }
  return Impl(entry, h, params, groups, points, S, level, sc, flags, out, ws, q, st);
}
constexpr auto value_query = query_entry<VALUE_QUERY, query_args, query_plan, query_impl, nrf_field_out>;
constexpr auto grad_query = query_entry<GRAD_QUERY, query_grad_args, query_grad_plan, query_grad_impl, nrf_field_grad_out>;
}  // namespace

extern "C" {

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
  forget_workspace(h, ws);
  const bool padded = q.ip_f != 0;
  if (padded && !(params = embed_side(h, params, ws, q, st))) return NRF_E_HIP;
  const WarpParamOffsets& wo = padded ? h->wpo : h->xwpo;   // else the caller's buffer: external offsets
  SidePack& pack = h->wp_pack;
  refresh(pack, (int64_t)q.wpk_f, [&](std::vector<PackDesc>& v) { warp_pack_descs(h, wo, (int64_t)q.wpk_f, false, v); });
  CK(upload_pack_table(pack, ws + q.desc_f, "upload warp pack table", st));
  launch_pack(reinterpret_cast<const PackDesc*>(ws + q.desc_f), (int)pack.descs.size(), params, ws, st);
  WarpFwdArgs a = warp_points_args(h, params, wo, ws + q.wpk_f, scalars, points, warp_ids, num_points, ws + q.out_f);
  const hipError_t e = hipMemsetAsync(ws + q.ctr_f, 0, 16 * sizeof(int), st);
  if (e != hipSuccess) return fail_hip(e, "zero tile counter");
  a.tile_counter = tile_counter_or_null(ws + q.ctr_f, 0);
  launch_warp_fwd(a, nullptr, false, tile_grid(a.ntiles, 2, h->num_cus), st);
  return finish_entry("nrf_warp_points", warped, ws + q.out_f, num_points, st);
}

int nrf_unwarp_workspace_bytes(nrf_handle h, int32_t num_points, size_t* bytes) {
  if (!h) return fail(NRF_E_NULL, "nrf_unwarp_workspace_bytes: handle is null");
  if (!bytes) return fail(NRF_E_NULL, "nrf_unwarp_workspace_bytes: bytes is null");
  CK(unwarp_model("nrf_unwarp_workspace_bytes", h, num_points));
  *bytes = unwarp_plan(h, num_points).total_f * sizeof(float);
  return NRF_OK;
}

int nrf_unwarp_points(nrf_handle h, const float* params, const float* targets, const int32_t* warp_ids, const float* warp_codes,
                      int32_t num_codes, const float* guess, int32_t num_points, const nrf_step_scalars* scalars, int32_t num_steps,
                      float tolerance, float max_step, const nrf_unwarp_out* out, void* workspace, size_t workspace_bytes, void* stream) {
  const char* null_arg = !h ? "handle" : !params ? "params" : !targets ? "targets" : !warp_ids ? "warp_ids" : !scalars ? "scalars (nrf_step_scalars)"
                         : !out ? "out (nrf_unwarp_out)" : !workspace ? "workspace" : nullptr;
  if (null_arg) {
    snprintf(g_err, sizeof(g_err), "nrf_unwarp_points: %s is null", null_arg);
    return NRF_E_NULL;
  }
  CK(unwarp_model("nrf_unwarp_points", h, num_points));
  if (num_steps < 0 || num_steps > NRF_UNWARP_MAX_STEPS) return fail(NRF_E_SHAPE, "nrf_unwarp_points: num_steps must be in 0..NRF_UNWARP_MAX_STEPS (32)");
  if (!(tolerance >= 0.f)) return fail(NRF_E_SHAPE, "nrf_unwarp_points: tolerance must be >= 0 (and not NaN)");
  if (!(max_step > 0.f)) return fail(NRF_E_SHAPE, "nrf_unwarp_points: max_step must be positive (INFINITY: no limit)");
  if (warp_codes && num_codes <= 0) return fail(NRF_E_SHAPE, "nrf_unwarp_points: num_codes must be positive with warp_codes");
  const UnwarpPlan q = unwarp_plan(h, num_points);
  if (workspace_bytes < q.total_f * sizeof(float)) return fail(NRF_E_WORKSPACE, "nrf_unwarp_points: workspace too small (see nrf_unwarp_workspace_bytes)");
  query_device(h);
  float* ws = (float*)workspace;
  hipStream_t st = (hipStream_t)stream;
  forget_workspace(h, ws);
  const bool padded = q.ip_f != 0;
  if (padded && !(params = embed_side(h, params, ws, q, st))) return NRF_E_HIP;
  const WarpParamOffsets& wo = padded ? h->wpo : h->xwpo;   // as nrf_warp_points
  SidePack& pack = h->un_pack;
  refresh(pack, (int64_t)q.wpk_f, [&](std::vector<PackDesc>& v) { warp_pack_descs(h, wo, (int64_t)q.wpk_f, false, v); });
  CK(upload_pack_table(pack, ws + q.desc_f, "upload unwarp pack table", st));
  launch_pack(reinterpret_cast<const PackDesc*>(ws + q.desc_f), (int)pack.descs.size(), params, ws, st);
  float* x = ws + q.x_f;
  int32_t* state = reinterpret_cast<int32_t*>(ws + q.state_f);
  launch_unwarp_init(guess ? guess : targets, num_points, x, state, st);
  // the primal pass at x keeping what a frozen ray plan keeps, and its tangent pass: a gradient query's two SE3 launches
  WarpFwdArgs wa = warp_points_args(h, params, wo, ws + q.wpk_f, scalars, x, warp_ids, num_points, ws + q.warped_f);
  if (warp_codes) wa.embed_table = warp_codes;
  wa.st_win = ws + q.win_f; wa.st_wv = reinterpret_cast<float4*>(ws + q.wv_f); wa.bits = reinterpret_cast<uint32_t*>(ws + q.bits_f);
  WarpFwdArgs ta = wa;
  ta.nt_prim = q.ntiles; ta.prim_win = wa.st_win; ta.prim_bits = wa.bits;
  ta.ntiles = 3 * q.ntiles; ta.rows = ta.ntiles * TILE_ROWS;
  ta.st_win = nullptr; ta.bits = nullptr; ta.points_out = nullptr; ta.st_wv = reinterpret_cast<float4*>(ws + q.twv_f);
  UnwarpArgs ua;
  memset(&ua, 0, sizeof(ua));
  ua.prim_win = wa.st_win; ua.prim_wv = wa.st_wv; ua.tan_wv = ta.st_wv; ua.warped = wa.points_out; ua.targets = targets;
  ua.x = x; ua.state = state;
  ua.rows = num_points; ua.rows_pad = (int)q.rows_pad(); ua.PKS = (h->PKw + 31) / 32 * 32;
  ua.tolerance = tolerance; ua.max_step = max_step;
  const int grid = tile_grid(wa.ntiles, warp_grid_mul(), h->num_cus), tgrid = tile_grid(ta.ntiles, warp_grid_mul(), h->num_cus);
  const double flops = warp_fwd_flops_row(h) * num_points;
  Prof& pf = h->prof;
  for (int k = 0; k <= num_steps; ++k) {   // the closing pass is the rounds' own launch: the same bits at the same x
    pf.begin("unwarp_warp", flops, st);
    launch_warp_fwd(wa, nullptr, true, grid, st, true);
    pf.end(st);
    if (k == num_steps) break;
    pf.begin("unwarp_tangent", 3.0 * flops, st);
    launch_warp_fwd(ta, nullptr, true, tgrid, st, true);
    pf.end(st);
    pf.begin("unwarp_step", 0, st);
    launch_unwarp_step(ua, st);
    pf.end(st);
  }
  pf.begin("unwarp_step", 0, st);   // the closing kernel: residual and status at the returned x
  launch_unwarp_finish(ua, out->points, out->residual, out->status, st);
  pf.end(st);
  return check_launch("nrf_unwarp_points");
}

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
  return value_query("nrf_query_points", false, h, params, groups, points, nullptr, 0, points_per_group, level, scalars, flags, out,
                     workspace, workspace_bytes, stream);
}

int nrf_query_grid(nrf_handle h, const float* params, const nrf_rays* group, const nrf_grid* grid, int64_t first, int32_t count,
                   int32_t level, const nrf_step_scalars* scalars, uint32_t flags, const nrf_field_out* out, void* workspace,
                   size_t workspace_bytes, void* stream) {
  return value_query("nrf_query_grid", true, h, params, group, nullptr, grid, first, count, level, scalars, flags, out, workspace,
                     workspace_bytes, stream);
}

int nrf_query_grad_workspace_bytes(nrf_handle h, int32_t num_groups, int32_t points_per_group, uint32_t flags, size_t* bytes) {
  if (!h || !bytes) return fail(NRF_E_NULL, "handle / bytes is null");
  CK(query_flags(flags));
  CK(query_grad_shape(num_groups, points_per_group));
  *bytes = query_grad_plan(h, num_groups, points_per_group).total_f * sizeof(float);
  return NRF_OK;
}

int nrf_query_points_grad(nrf_handle h, const float* params, const nrf_rays* groups, const float* points, int32_t points_per_group,
                          int32_t level, const nrf_step_scalars* scalars, uint32_t flags, const nrf_field_grad_out* out, void* workspace,
                          size_t workspace_bytes, void* stream) {
  return grad_query("nrf_query_points_grad", false, h, params, groups, points, nullptr, 0, points_per_group, level, scalars, flags, out,
                    workspace, workspace_bytes, stream);
}

int nrf_query_grid_grad(nrf_handle h, const float* params, const nrf_rays* group, const nrf_grid* grid, int64_t first, int32_t count,
                        int32_t level, const nrf_step_scalars* scalars, uint32_t flags, const nrf_field_grad_out* out, void* workspace,
                        size_t workspace_bytes, void* stream) {
  return grad_query("nrf_query_grid_grad", true, h, params, group, nullptr, grid, first, count, level, scalars, flags, out, workspace,
                    workspace_bytes, stream);
}

}  // extern "C"
