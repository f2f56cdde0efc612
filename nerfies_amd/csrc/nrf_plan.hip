// Plan side of the C-ABI layer: the flat-parameter layout a handle owns (external = the caller's flax tree, internal = what the kernels
// index), the weight-pack tables, and the workspace plan of one (model, num_rays, flags): sub-buffer offsets, the stream-K partitions of
// both wgrad kernels, the reduce / pack / embed descriptor tables and their upload.  See nrf_handle.h.
#include "nrf_handle.h"

using namespace nrf;
using namespace nrf::api;

namespace nrf {
namespace api {

// Appends a leaf to the internal layout (rows x cols = what the kernels index) and to the external one
// (xrows x xcols = what the model owns; defaults to the same).  External rows >= split sit `shift` rows lower inside.
// xname: the leaf's path in the caller's tree when it differs from the internal one; "" = internal only (no external
// leaf: stays zero in the padded image, its gradient is dropped).
static void add_leaf(nrf_handle h, const std::string& name, int rows, int cols, int64_t* off_out, int xrows = -1, int xcols = -1,
              int split = -1, int64_t* xoff_out = nullptr, const char* xname = nullptr) {
  if (xrows < 0) xrows = rows;
  if (xcols < 0) xcols = cols;
  nrf_tensor_info t;
  memset(&t, 0, sizeof(t));
  snprintf(t.name, sizeof(t.name), "%s", name.c_str());
  t.offset = h->nparams;
  t.rows = rows;
  t.cols = cols;
  if (off_out) *off_out = t.offset;
  h->nparams += (int64_t)rows * cols;
  h->nparams = (int64_t)align_up((size_t)h->nparams, 4);   // keep every leaf 16-byte aligned
  h->layout.push_back(t);
  if (xname && !*xname) { h->embed = true; return; }
  nrf_tensor_info x = t;
  if (xname) { snprintf(x.name, sizeof(x.name), "%s", xname); h->embed = true; }
  x.offset = h->xnparams;
  x.rows = xrows;
  x.cols = xcols;
  if (xoff_out) *xoff_out = x.offset;
  h->xnparams += (int64_t)xrows * xcols;
  h->xnparams = (int64_t)align_up((size_t)h->xnparams, 4);
  h->xlayout.push_back(x);
  EmbedDesc e;
  e.ext_off = x.offset; e.int_off = t.offset; e.rows = xrows; e.ext_cols = xcols; e.int_cols = cols;
  e.split = split < 0 ? xrows : split; e.shift = rows - xrows; e.pad_ = 0;
  h->emb.push_back(e);
  if (xrows != rows || xcols != cols) h->embed = true;
}

void build_layout(nrf_handle h) {
  const nrf_model_desc& d = h->d;
  const int W = TRUNK_W, RW = RGB_W;                               // what the kernels index
  const int XW = d.nerf_trunk_width, XRW = d.nerf_rgb_branch_width;   // what the model owns (<= W, RW)
  for (int lv = 0; lv < h->nlevels; ++lv) {
    const std::string base = lv == 0 ? "nerf_mlps_coarse" : "nerf_mlps_fine";
    MlpParamOffsets& po = h->po[lv];
    for (int i = 0; i < TRUNK_DEPTH; ++i) {
      const int hid = i == 0 ? 0 : 1;                 // rows of the running activation, then (layer 0 / skip) the posenc rows
      const int e = h->emap[i];                       // the caller's layer that runs here, or -1: an identity layer
      const int pe = (i == 0 || i == d.nerf_skip_layer) ? h->P : 0;
      const int xpe = (e == 0 || (e >= 0 && e == h->xskip)) ? h->P : 0;   // a skip the caller's trunk never reaches: zero posenc rows inside
      const std::string kn = base + "/MLP_0/hidden_" + std::to_string(i) + "/kernel", bn = base + "/MLP_0/hidden_" + std::to_string(i) + "/bias";
      if (e >= 0) {
        const std::string xkn = base + "/MLP_0/hidden_" + std::to_string(e) + "/kernel", xbn = base + "/MLP_0/hidden_" + std::to_string(e) + "/bias";
        add_leaf(h, kn, hid * W + pe, W, &po.trunk_k[i], hid * XW + xpe, XW, hid * XW, nullptr, e != i ? xkn.c_str() : nullptr);
        add_leaf(h, bn, 1, W, &po.trunk_b[i], 1, XW, -1, nullptr, e != i ? xbn.c_str() : nullptr);
      } else {   // between / behind the caller's layers: internal-only identity (relu(h . I) = h for h >= 0; its gradient is dropped)
        add_leaf(h, kn, hid * W + pe, W, &po.trunk_k[i], -1, -1, -1, nullptr, "");
        add_leaf(h, bn, 1, W, &po.trunk_b[i], -1, -1, -1, nullptr, "");
        EmbedDesc e2;
        e2.ext_off = -1; e2.int_off = po.trunk_k[i]; e2.rows = XW; e2.ext_cols = 1; e2.int_cols = W; e2.split = XW; e2.shift = 0; e2.pad_ = 0;
        h->emb.push_back(e2);
      }
      if (xpe != pe) h->embed = true;
    }
    if (h->R == 0 && h->A == 0) {
      // no condition at all (use_viewdirs = False, no camera / appearance code): NerfMLP has NO bottleneck layer and the rgb branch
      // reads the trunk output (modules.py:149-164).  The kernels keep their layer list: the bottleneck becomes an internal-only
      // IDENTITY (x . I + 0 is exact in float32, and exact on the bf16 chain, whose h8 is already bf16), its gradient is dropped
      add_leaf(h, base + "/bottleneck/kernel", W, W, &po.bn_k, -1, -1, -1, nullptr, "");
      add_leaf(h, base + "/bottleneck/bias", 1, W, &po.bn_b, -1, -1, -1, nullptr, "");
      EmbedDesc e;
      e.ext_off = -1; e.int_off = po.bn_k; e.rows = XW; e.ext_cols = 1; e.int_cols = W; e.split = XW; e.shift = 0; e.pad_ = 0;
      h->emb.push_back(e);
    } else {
      add_leaf(h, base + "/bottleneck/kernel", W, W, &po.bn_k, XW, XW);
      add_leaf(h, base + "/bottleneck/bias", 1, W, &po.bn_b, 1, XW);
    }
    add_leaf(h, base + "/MLP_1/hidden_0/kernel", W + h->R, RW, &po.rgbh_k, XW + h->R, XRW, XW);
    add_leaf(h, base + "/MLP_1/hidden_0/bias", 1, RW, &po.rgbh_b, 1, XRW);
    for (int i = 1; i < d.nerf_rgb_branch_depth; ++i) {   // modules.py:41-50: layers 1.. of the branch read the layer before, (w, w)
      const std::string hn = base + "/MLP_1/hidden_" + std::to_string(i);
      add_leaf(h, hn + "/kernel", RW, RW, &po.rgbx_k[i - 1], XRW, XRW);
      add_leaf(h, hn + "/bias", 1, RW, &po.rgbx_b[i - 1], 1, XRW);
    }
    add_leaf(h, base + "/MLP_1/logit/kernel", RW, 3, &po.logit_k, XRW, 3);
    add_leaf(h, base + "/MLP_1/logit/bias", 1, 3, &po.logit_b);
    add_leaf(h, base + "/MLP_2/logit/kernel", W + h->A, 1, &po.alpha_k, XW + h->A, 1, XW);   // [bottleneck | appearance code] (modules.py:152-157)
    add_leaf(h, base + "/MLP_2/logit/bias", 1, 1, &po.alpha_b);
  }
  if (h->warp) {   // warping.SE3Field (warping.py:202-320); flax names per SURVEY.md A.2
    WarpParamOffsets& w = h->wpo;
    WarpParamOffsets& x = h->xwpo;
    if (h->time_enc) {   // modules.TimeEncoder (modules.py:297-322): self.mlp = MLP(depth 6, width 64, skips (4,), output G)
      w.embed = x.embed = -1;
      for (int i = 0; i < TIME_DEPTH; ++i) {
        const int fin = i == 0 ? h->Tin : i == TIME_SKIP ? TIME_W + h->Tin : TIME_W;
        add_leaf(h, "warp_field/metadata_encoder/mlp/hidden_" + std::to_string(i) + "/kernel", fin, TIME_W, &h->tpo.k[i]);
        add_leaf(h, "warp_field/metadata_encoder/mlp/hidden_" + std::to_string(i) + "/bias", 1, TIME_W, &h->tpo.b[i]);
      }
      add_leaf(h, "warp_field/metadata_encoder/mlp/logit/kernel", TIME_W, d.num_warp_features, &h->tpo.lk);
      add_leaf(h, "warp_field/metadata_encoder/mlp/logit/bias", 1, d.num_warp_features, &h->tpo.lb);
    } else {
      add_leaf(h, "warp_field/metadata_encoder/embed/embedding", d.num_warp_embeddings, d.num_warp_features, &w.embed, -1, -1, -1,
               &x.embed);
    }
    // TranslationField (warping.py:62-199) = the same 6x128 trunk with ONE 3-channel output layer and x' = x + t:
    // exactly the SE3 field with a zero rotation head (theta = 0: R = I, p = v; the closed forms are series in
    // theta^2 there).  Its leaves 'warp_field/mlp/hidden_i' / 'mlp/logit' map onto trunk / branches_v; branches_w
    // exists only internally and stays zero.
    const bool tr = d.warp_field_type == NRF_WARP_TRANSLATION;
    // warp_kwargs trunk_depth / trunk_width (warping.py:225-227): a shallower / narrower trunk runs on the 6 x 128 kernels --
    // identity layers behind the caller's last one (every trunk layer ends in a ReLU: modules.py:41-50), zero padding to 128
    // columns, zero input rows in the skip layer when the caller's trunk (<= 4 layers) never reaches it
    const int XD = h->wxdepth, XWw = h->wxwidth;
    for (int i = 0; i < WARP_DEPTH; ++i) {
      const int hid = i == 0 ? 0 : 1;
      const int pe = (i == 0 || i == WARP_SKIP) ? h->Win : 0;
      const std::string nk = "warp_field/trunk/hidden_" + std::to_string(i) + "/kernel", nb = "warp_field/trunk/hidden_" + std::to_string(i) + "/bias";
      const std::string xk = "warp_field/mlp/hidden_" + std::to_string(i) + "/kernel", xb = "warp_field/mlp/hidden_" + std::to_string(i) + "/bias";
      if (i < XD) {
        add_leaf(h, nk, hid * WARP_W + pe, WARP_W, &w.trunk_k[i], hid * XWw + pe, XWw, hid * XWw, &x.trunk_k[i], tr ? xk.c_str() : nullptr);
        add_leaf(h, nb, 1, WARP_W, &w.trunk_b[i], 1, XWw, -1, &x.trunk_b[i], tr ? xb.c_str() : nullptr);
      } else {
        add_leaf(h, nk, hid * WARP_W + pe, WARP_W, &w.trunk_k[i], -1, -1, -1, nullptr, "");
        add_leaf(h, nb, 1, WARP_W, &w.trunk_b[i], -1, -1, -1, nullptr, "");
        EmbedDesc e;
        e.ext_off = -1; e.int_off = w.trunk_k[i]; e.rows = XWw; e.ext_cols = 1; e.int_cols = WARP_W; e.split = XWw; e.shift = 0; e.pad_ = 0;
        h->emb.push_back(e);
      }
    }
    add_leaf(h, "warp_field/branches_w/logit/kernel", WARP_W, 3, &w.w_k, XWw, 3, -1, &x.w_k, tr ? "" : nullptr);
    add_leaf(h, "warp_field/branches_w/logit/bias", 1, 3, &w.w_b, -1, -1, -1, &x.w_b, tr ? "" : nullptr);
    add_leaf(h, "warp_field/branches_v/logit/kernel", WARP_W, 3, &w.v_k, XWw, 3, -1, &x.v_k, tr ? "warp_field/mlp/logit/kernel" : nullptr);
    add_leaf(h, "warp_field/branches_v/logit/bias", 1, 3, &w.v_b, -1, -1, -1, &x.v_b, tr ? "warp_field/mlp/logit/bias" : nullptr);
  }
  if (d.use_appearance_metadata)
    add_leaf(h, "appearance_encoder/embed/embedding", d.num_appearance_embeddings, d.num_appearance_features, &h->app_off);
  if (d.use_camera_metadata)
    add_leaf(h, "camera_encoder/embed/embedding", d.num_camera_embeddings, d.num_camera_features, &h->cam_off);
}

void build_pack_offsets(nrf_handle h) {
  PackOffsets& pk = h->pk;
  int o = 0;
  auto take = [&](int n) { int r = o; o += n; return r; };
  pk.fwd_L[0] = take(h->PK * 256);
  for (int l = 1; l < TRUNK_DEPTH; ++l) pk.fwd_L[l] = take(256 * 256);
  pk.fwd_L4b = take(h->PK * 256);
  pk.fwd_bn = take(256 * 256);
  pk.fwd_rgbh = take(256 * 128);
  pk.bwd_rgbhT = take(128 * 256);
  pk.bwd_bnT = take(256 * 256);
  pk.bwd_LT[0] = 0;
  for (int l = 1; l < TRUNK_DEPTH; ++l) pk.bwd_LT[l] = take(256 * 256);
  pk.bwd_L0T = pk.bwd_L4bT = 0;
  if (h->warp) { pk.bwd_L0T = take(256 * 64); pk.bwd_L4bT = take(256 * 64); }
  pk.fwd_rgbx = pk.bwd_rgbxT = 0;
  if (const int nx = h->d.nerf_rgb_branch_depth - 1) {   // rgb branch layers 1..nx, behind everything a depth-1 model packs
    pk.fwd_rgbx = take(nx * RGB_W * RGB_W);
    pk.bwd_rgbxT = take(nx * RGB_W * RGB_W);
  }
  pk.total = o + 4096;   // slack: the K loop prefetches two quads past a layer's last weights
  if (h->warp) {
    WarpPackOffsets& w = h->wpk;
    int ow = 0;
    auto takew = [&](int n) { int r = ow; ow += n; return r; };
    w.fwd_L[0] = takew(h->PKw * WARP_W);
    for (int l = 1; l < WARP_DEPTH; ++l) w.fwd_L[l] = takew(WARP_W * WARP_W);
    w.fwd_L4b = takew(h->PKw * WARP_W);
    w.bwd_LT[0] = 0;
    for (int l = 1; l < WARP_DEPTH; ++l) w.bwd_LT[l] = takew(WARP_W * WARP_W);
    w.total = ow + 4096;
  }
}

// Measured (r01): pulling tiles from a global counter is 4-6 % SLOWER than the static round-robin split for the
// chain kernels (fine forward 1.99 vs 1.87 ms) although it removes the tail where the younger workgroup of a CU
// runs alone -- so static is the default and NRF_DYNAMIC_TILES=1 keeps the other path testable.
// Uneven static tile split of the NeRF chain kernels (chain_common.h tile_iter): tiles the older workgroup of a CU takes out
// of the K = ceil(ntiles / CUs) of its CU, when the launch is exactly two workgroups per CU and K >= 4.  NRF_OLD_SHARE
// overrides the share (0 = even split).
static int k_old_for(int ntiles, int grid, int num_cus, double dflt_share) {
  if (grid != 2 * num_cus) return 0;
  const int K = (ntiles + num_cus - 1) / num_cus;
  if (K < 4) return 0;
  const double share = knobs().old_share >= 0.0 ? knobs().old_share : dflt_share;
  if (share <= 0.0) return 0;
  int k = (int)floor(K * share + 0.5);
  return k < 1 ? 1 : (k > K - 1 ? K - 1 : k);
}

// workgroups per CU of the SE3 chain kernels' launches
int warp_grid_mul() {
  const int m = knobs().warp_grid_mul;
  return m < 1 ? 1 : (m > 4 ? 4 : m);
}

int* tile_counter_or_null(float* base, int idx) {
  return knobs().dynamic_tiles ? reinterpret_cast<int*>(base) + idx : nullptr;
}
// automatic choice of the forward chain's tiling (chain32_for): 32-row tiles when the launch has fewer than this many 64-row
// tiles per CU (the 64-row grid of two workgroups per CU is then not filled)
constexpr int AUTO32_FWD_BELOW_TILES_PER_CU = 2;

// the flags a workspace layout depends on: TRAIN, WARP_JACOBIAN, and BF16 together with TRAIN (bf16 stash instead of fp32)
static uint32_t plan_flags(uint32_t flags) {
  uint32_t f = flags & (NRF_FLAG_TRAIN | NRF_FLAG_WARP_JACOBIAN);
  if ((flags & NRF_FLAG_TRAIN) && (flags & NRF_FLAG_BF16)) f |= NRF_FLAG_BF16 | (flags & NRF_FLAG_WARP_F32);
  if (!(flags & NRF_FLAG_TRAIN) && (flags & NRF_FLAG_BF16X3)) f |= NRF_FLAG_BF16X3;   // its own (tripled) weight streams
  if ((flags & NRF_FLAG_TRAIN) && (flags & NRF_FLAG_RAY_GRADS)) f |= NRF_FLAG_RAY_GRADS;   // float32 training only (check_flags)
  if ((f & NRF_FLAG_RAY_GRADS) && (flags & NRF_FLAG_FROZEN)) f |= NRF_FLAG_FROZEN;         // ... with both of them only (check_flags)
  return f;
}

// Rows per workgroup tile of the float32 NeRF chain kernels for a launch over `ntiles` 64-row tiles: true = 32-row half tiles,
// four workgroups per CU (mlp_chain32.hip; nerf_chain.h Tile32).  NRF_OPT_CHAIN_TILE_ROWS forces either.  Automatic = what the
// round-5 A/B measured (profiles/r05_chain32_ab.md): in steady state the 64-row kernels win by 3-5 % (forward 130 vs 123.5 TF, reverse 129 vs 125,
// eval forward 137 vs 132: every B operand float feeds one MFMA instead of two), but a launch that cannot fill the 64-row grid
// twice over -- fewer than two tiles per workgroup slot, e.g. one GPU's 128-ray share of a 1024-ray batch: 128 + 384 tiles for
// 512 slots -- runs 12-34 % faster on half tiles (coarse forward 0.160 -> 0.106 ms, fine 0.301 -> 0.264 ms).  The reverse
// chain never won (0.303 -> 0.327 ms at 512 tiles): its automatic choice stays 64.
// An rgb branch deeper than one layer is compiled into the 64-row kernels only (nerf_chain.h Tile64::FULL): such a handle
// never takes half tiles (nrf_set_option refuses 32 for it), whatever the launch size.
static bool chain32_for(const nrf_handle_s* h, int ntiles, bool reverse = false) {
  if (h->d.nerf_rgb_branch_depth > 1) return false;
  if (h->chain_rows_opt == 32) return true;
  if (h->chain_rows_opt == 64) return false;
  return !reverse && ntiles < AUTO32_FWD_BELOW_TILES_PER_CU * h->num_cus;
}
// 32-row half tiles, four workgroups per CU; else 64-row, two
ChainTiling chain_fwd_tiling(const nrf_handle_s* h, int ntiles, bool allow32) {
  const bool c32 = allow32 && chain32_for(h, ntiles);
  const int grid = c32 ? tile_grid(2 * ntiles, 4, h->num_cus) : tile_grid(ntiles, knobs().grid_mul, h->num_cus);
  return {c32, grid, k_old_for(ntiles, grid, h->num_cus, 0.0)};
}

// fp32 fragment images of the SE3 trunk (warp_chain.hip), packed from the leaves at `w` to base + h->wpk: the forward layers and,
// with `transposed`, the reverse chain's W^T of layers 1..5
void warp_pack_descs(const nrf_handle_s* h, const WarpParamOffsets& w, int64_t base, bool transposed, std::vector<PackDesc>& out) {
  const WarpPackOffsets& wk = h->wpk;
  auto add = [&](int64_t src, int dst, int row0, int kvalid, int K, int tr) {   // PackDesc: ..., ncb, transposed, nwaves, nvalid
    out.push_back(PackDesc{src, base + dst, WARP_W, row0, kvalid, K, 1, tr, 4, 1 << 30});
  };
  add(w.trunk_k[0], wk.fwd_L[0], 0, h->Win, h->PKw, 0);
  for (int l = 1; l < WARP_DEPTH; ++l) add(w.trunk_k[l], wk.fwd_L[l], 0, WARP_W, WARP_W, 0);
  add(w.trunk_k[WARP_SKIP], wk.fwd_L4b, WARP_W, h->Win, h->PKw, 0);
  for (int l = 1; l < WARP_DEPTH && transposed; ++l) add(w.trunk_k[l], wk.bwd_LT[l], 0, WARP_W, WARP_W, 1);
}

// fp32 fragment images of level `lv`'s NeRF MLP (nerf_chain.h), packed from its leaves to base + h->pk: the forward layers and, with
// `transposed`, the reverse chain's W^T images in between, in the order every ray plan's table has (nrf_debug_plan_digest hashes it)
void mlp_pack_descs(const nrf_handle_s* h, int lv, int64_t base, bool transposed, std::vector<PackDesc>& out) {
  const MlpParamOffsets& po = h->po[lv];
  const PackOffsets& pk = h->pk;
  auto add = [&](int64_t src, int dst, int ld, int row0, int kvalid, int K, int ncb, int tr, int nwaves = 4, int nvalid = 1 << 30) {
    if (!tr || transposed) out.push_back(PackDesc{src, base + dst, ld, row0, kvalid, K, ncb, tr, nwaves, nvalid});
  };
  add(po.trunk_k[0], pk.fwd_L[0], 256, 0, h->P, h->PK, 2, 0);
  for (int l = 1; l < TRUNK_DEPTH; ++l) add(po.trunk_k[l], pk.fwd_L[l], 256, 0, 256, 256, 2, 0);
  add(po.trunk_k[h->d.nerf_skip_layer], pk.fwd_L4b, 256, 256, h->P, h->PK, 2, 0);
  add(po.bn_k, pk.fwd_bn, 256, 0, 256, 256, 2, 0);
  add(po.rgbh_k, pk.fwd_rgbh, 128, 0, 256, 256, 1, 0);
  add(po.rgbh_k, pk.bwd_rgbhT, 128, 0, 128, 128, 2, 1);
  for (int x = 0; x < h->d.nerf_rgb_branch_depth - 1; ++x) {   // 128 x 128, one 32-column block per wave, as is and transposed
    add(po.rgbx_k[x], pk.fwd_rgbx + x * RGB_W * RGB_W, 128, 0, 128, 128, 1, 0);
    add(po.rgbx_k[x], pk.bwd_rgbxT + x * RGB_W * RGB_W, 128, 0, 128, 128, 1, 1);
  }
  add(po.bn_k, pk.bwd_bnT, 256, 0, 256, 256, 2, 1);
  for (int l = 1; l < TRUNK_DEPTH; ++l) add(po.trunk_k[l], pk.bwd_LT[l], 256, 0, 256, 256, 2, 1);
  if (h->warp) {   // d posenc streams: B[k][n] = W[row0 + n][k], n < P, one 64-column group
    add(po.trunk_k[0], pk.bwd_L0T, 256, 0, 256, 256, 2, 1, 1, h->P);
    add(po.trunk_k[h->d.nerf_skip_layer], pk.bwd_L4bT, 256, 256, 256, 256, 2, 1, 1, h->P);
  }
}

namespace {

// calibration overrides of the wgrad cost models (scripts/wgrad_calib.py, scripts/r6/cost_sweep.py): experiment builds only
double env_cost(const char* name, double dflt) {
#ifdef NRF_EXPERIMENT
  if (const char* e = getenv(name)) return atof(e);
#endif
  (void)name;
  return dflt;
}

// An operand of an fp32 wgrad group (wgrad.hip): a stash of the level at *off + add (read once the layout is known), SRC_*
// layout, 32-feature blocks and floats per 64-row tile.  {} = none: the vector-column groups have no dY.
struct Operand { int kind; size_t* off; size_t add; int blocks, stride; };
Operand frag256(size_t* off, size_t add = 0) { return {SRC_FRAG256, off, add, 8, FRAG_TILE_256}; }
Operand frag128(size_t* off, size_t add = 0) { return {SRC_FRAG128, off, add, 4, FRAG_TILE_128}; }
Operand plain(size_t* off, int K) { return {SRC_PLAIN, off, 0, (K + 31) / 32, (K + 31) / 32 * 32 * TILE_ROWS}; }   // whole 32-feature blocks

// fp32 wgrad group: leaf [kvalid][cols] (+)= X^T dY over the tiles of level lv, or -- vec > 0, the narrow heads on the VALU --
// X^T v, v = .w (vec 1) / .xyz (vec 3) of the vec4 rows at vecoff (nullptr: the level's d_raw4); vecoff2 / dst2: a second
// vector column set against the same X
struct GroupSpec {
  int lv, accumulate;
  Operand x, dy;
  int kvalid, cols, vec;
  int64_t dst;
  size_t* vecoff;
  size_t* vecoff2;
  int64_t dst2;
};

// Cost of one 64-row tile of an fp32 group, in units of a full 256x256 layer tile; the narrow groups are staging/latency bound,
// so they are charged more than their MFMA share.
// measured with scripts/wgrad_calib.py / wgrad_calib_vrig.py (per-segment wall clocks, least squares), relative to a
// 256x256 tile; round 3 (asm LDS-DMA + 160 KiB ring: the narrow groups are no longer latency-bound): 8x8 = 14.8 us; round 6 (SGPR piece
// tables, refill behind the MFMAs): re-fitted on config A and the vrig shape (gpurun_out/r6h: every narrow type ~6 % cheaper relative
// to 8x8, a segment 0.4-0.5 tiles; the two-vector SE3 heads 0.155: the fit's Kb = 4, Nb = 0 row mixes them with the rgb logits)
double tile_cost(const GroupSpec& sp) {
  const double c_vec256 = env_cost("NRF_COST_VEC256", 0.106), c_vec128 = env_cost("NRF_COST_VEC128", 0.094),
               c_vec128x2 = env_cost("NRF_COST_VEC128X2", 0.155),   // SE3 heads: two vectors against one pass over h6
               c_pe = env_cost("NRF_COST_PE", 0.270),               // 2 x 8 blocks: posenc rows of the NeRF trunk
               c_rgbh = env_cost("NRF_COST_RGBH", 0.516),           // 8 x 4
               c_44 = env_cost("NRF_COST_44", 0.266),               // 4 x 4: SE3 trunk layers
               c_pe128 = env_cost("NRF_COST_PE128", 0.141);         // 2 x 4: SE3 trunk input rows
  const int Kb = sp.x.blocks, Nb = sp.dy.blocks;
  if (Nb == 0) return Kb == 8 ? c_vec256 : sp.vecoff2 ? c_vec128x2 : c_vec128;   // vector columns only (VALU + HBM stream)
  if (Nb == 8) return Kb >= 5 ? 1.0 : c_pe;
  return Kb >= 5 ? c_rgbh : Kb >= 3 ? c_44 : c_pe128;
}

// A source of a bf16 wgrad operand (wgrad_bf16.hip): a bf16 stash at *off + add dwords, `blocks` blocks of it per 32-sample group.
// A second source (BSpec x2 / dy2) supplies the operand's last blocks out of a buffer of `stride` blocks per group.
struct BfSrc { size_t* off; size_t add; int blocks; int stride = 0; };
// A leaf out of a group's slab: leaf [rows][cols] <- slab[0:rows][col0:col0 + cols]; a bias leaf: column sums [col0:col0 + cols] of dY
struct Leaf { int64_t off; int cols, col0; };

// bf16 wgrad group over the 32-sample groups of level lv (ngroups: 0 = the MLP level's), added in reduce pass `accu`
struct BSpec {
  int lv, accu, ngroups;
  BfSrc x, dy, x2, dy2;   // X = [x | x2], dY = [dy | dy2]
  int rows;               // valid rows of X
  Leaf w[2], b[2];        // weight and bias leaves, off < 0: none
};

// Cost of one 32-sample group of a bf16 group: HBM-bound, cost = blocks streamed.
// A chunk costs (Kb + Nb) + a fixed term, in block units (2 KiB streamed).  Round 2 measured + 12 on config A (the per-chunk
// barrier and HBM latency worth 24 KiB of streaming: wgrad 0.87 ms with a pure byte model, 0.61 ms with that one).  Round 6,
// after the copies moved to per-segment SGPR tables (wgrad_bf16.hip): ALONE every shape streams 5.6-6.4 TB/s, i.e. cost ~ bytes
// (scripts/micro/wgrad_bf16_bench.hip), but IN the mixed launch a byte-proportional model is 3-10 % slower than + 12, and the
// narrow shapes (Kb + Nb <= 8: the SE3 trunk's 16 / 12 KiB chunks) are best charged + 8: swept on config D / vrig / A (bf16) at
// narrow = 12 / 8 / 5 / 2: 1.19 / 1.13 / 1.18 / 1.38 ms, 0.92 / 0.84 / 0.90 / 1.03 ms, 0.456 / 0.460 / 0.495 / 0.618 ms
// (profiles/r06_experiments.md section 3)
double bcost(const BSpec& sp) {
  const double bc_chunk = env_cost("NRF_BCOST_CHUNK", 12.0);   // per-chunk fixed cost (barrier + issue), in block units
  // the two merged shapes (10 x 8, 8 x 9: ten accumulator blocks per wave, five copies per wave and chunk) cost more per chunk
  // than their bytes: with a byte-proportional cost the kernel was 10 % SLOWER although it fetched 10 % less (the workgroups
  // inside the merged groups ran ~1.35 x their quota); swept on the GPU at +0 / 6 / 10 / 16 / 24 / 32 units: 0.555 / 0.508 /
  // 0.500 / 0.520 / 0.527 / 0.543 ms
  const double bc_merged = env_cost("NRF_BCOST_MERGED", 10.0);
  const double bc_chunk_narrow = env_cost("NRF_BCOST_CHUNK_NARROW", 8.0);   // ... of the 4 x 4 / 2 x 4 shapes (SE3 trunk: 16 / 12 KiB chunks)
  const double bc_quad = env_cost("NRF_BCOST_QUAD", 0.0);   // per accumulator block (Kb x Nb): the MFMA / operand-read side of a chunk
  const int Kb = sp.x.blocks + sp.x2.blocks, Nb = sp.dy.blocks + sp.dy2.blocks;   // the second sources' blocks included
  return (double)(Kb + Nb) + (Kb + Nb <= 8 ? bc_chunk_narrow : bc_chunk) + bc_quad * Kb * Nb + ((sp.x2.blocks || sp.dy2.blocks) ? bc_merged : 0.0);
}

// Stream-K partition of the wgrad work: equal cost per workgroup, one workgroup per CU.  Group gi is ntiles[gi] tiles of cost[gi];
// every workgroup and every group boundary opens a segment, at cost `seg`.  Fills segs / seg_begin (workgroup w runs segments
// [seg_begin[w], seg_begin[w + 1])) and returns the number of segments (slab partials) of each group.
std::vector<int> stream_k(const std::vector<double>& cost, const std::vector<int>& ntiles, double seg, int nwg,
                          std::vector<WgradSegment>& segs, std::vector<int>& seg_begin) {
  std::vector<int> nsplit(cost.size(), 0);
  double total = 0;
  for (size_t gi = 0; gi < cost.size(); ++gi) total += cost[gi] * ntiles[gi];
  total += seg * (nwg + (double)cost.size());
  const double quota = total / nwg;
  seg_begin.assign(1, 0);
  int w = 0;
  double room = quota;
  for (size_t gi = 0; gi < cost.size(); ++gi) {
    const double c = cost[gi];
    const int nt = ntiles[gi];
    for (int t0 = 0; t0 < nt;) {
      int take_n = (int)floor((room - seg) / c + 1e-9);
      if (take_n <= 0 && w < nwg - 1) {   // this workgroup is full: move on
        seg_begin.push_back((int)segs.size());
        ++w; room += quota;
        continue;
      }
      if (take_n <= 0 || w == nwg - 1 || take_n > nt - t0) take_n = nt - t0;   // the last workgroup absorbs rounding leftovers
      segs.push_back({(int)gi, t0, t0 + take_n, nsplit[gi]++});
      t0 += take_n;
      room -= seg + take_n * c;
    }
  }
  while ((int)seg_begin.size() < nwg + 1) seg_begin.push_back((int)segs.size());
  return nsplit;
}

// The chunk table of one bf16 weight stream (mlp_bf16.hip / warp_bf16.hip; x3: mlp_bf16x3.hip / warp_bf16x3.hip) from float offset
// `base`.  One GEMM = nblocks / pb panels; a panel (chunk) = [row][block of the panel][lane] x 16 B, rows = [bias row,] then the
// k-step rows of each input part.  x3: the same GEMM sequence with every k-step row of a forward stream doubled (W_hi, W_lo); the
// kernel cuts a panel's rows into chunks itself.
struct Stream {
  size_t base, at;   // stream base, floats emitted so far
  int tr;            // 1: a reverse (dgrad) stream, A = W as stored, [m = the layer's input feature][k = its output feature]
  bool x3;
  std::vector<RcPackDesc>& out;
  // an input part: leaf, ld, first row, valid K, input blocks; leaf2 / split: the second of two leaves side by side (SE3 heads w | v)
  struct Part { int64_t leaf; int ld, row0, krows, nin; int64_t leaf2 = -1; int split = 0; };
  // bias: the bias row's leaf, -1 none, -2 a zero row where the kernel runs a bias-style k-step this model does not use;
  // bias2 / bsplit: as leaf2 / split
  void gemm(int pb, int nblocks, int ncols, int64_t bias, std::initializer_list<Part> parts, int64_t bias2 = -1, int bsplit = 0) {
    for (int pn = 0; pn < nblocks / pb; ++pn) {
      int row = 0;
      auto emit = [&](int kind, int64_t src, int64_t src2, int split, int ld, int row0, int krows, int nrows) {
        RcPackDesc e;
        memset(&e, 0, sizeof(e));
        e.src_off = src; e.dst_off = (long long)(base + at + (size_t)row * pb * 256); e.kind = kind; e.src_ld = ld; e.row0 = row0;
        e.krows = krows; e.ncols = ncols; e.ngroups = nrows; e.nout = pb; e.nout_panel = pb; e.o0 = 0; e.transposed = tr;
        e.oblk0 = pn * pb; e.src_off2 = src2 >= 0 ? src2 : 0; e.split = src2 >= 0 ? split : 0; e.x3 = x3 && !tr;
        out.push_back(e);
        row += nrows;
      };
      if (bias >= 0) emit(1, bias, bias2, bsplit, 0, 0, 0, 1);
      else if (bias == -2) emit(2, 0, -1, 0, 0, 0, 0, 1);
      for (const Part& q : parts) emit(0, q.leaf, q.leaf2, q.split, q.ld, q.row0, q.krows, (x3 && !tr ? 2 : 1) * 2 * q.nin);
      at += (size_t)row * pb * 256;
    }
  }
};

ReduceDesc reduce_desc(int64_t dst, int dst_ld, int rows, int cols, int64_t src, int src_ld, int64_t part_stride, int nparts,
                       int accumulate = 0) {
  ReduceDesc r;
  memset(&r, 0, sizeof(r));
  r.dst_off = dst; r.dst_ld = dst_ld; r.rows = rows; r.cols = cols; r.accumulate = accumulate;
  r.src_off = src; r.src_ld = src_ld; r.part_stride = part_stride; r.nparts = nparts;
  return r;
}

// The descriptor tables at ws + plan.tables in layout order, each sized from what was built (round 2 reserved 64 pack / 192
// reduce descriptors without a check) plus its slack: one spare element, or 256 bytes (wgrad groups and segments).  The embed
// table is the handle's, uploaded only for a model that runs on its padded image.
struct Table {
  size_t* off_b;
  const void* data;
  size_t bytes, slack;
  const char* what;
  bool upload;
};
template <class T> Table table(size_t* off_b, const std::vector<T>& v, bool spare, const char* what, bool upload = true) {
  return {off_b, v.data(), v.size() * sizeof(T), spare ? sizeof(T) : 256, what, upload};
}
std::vector<Table> tables_of(nrf_handle h) {
  WsPlan& p = h->plan;
  return {table(&p.pack_off_b, p.pack, true, "upload pack table"), table(&p.groups_off_b, p.groups, false, "upload wgrad table"),
          table(&p.reduce_off_b, p.reduce, true, "upload reduce table"), table(&p.segs_off_b, p.segs, false, "upload wgrad segments"),
          table(&p.segbegin_off_b, p.seg_begin, true, "upload wgrad segment index"),
          table(&p.emb_off_b, h->emb, true, "upload embed table", h->embed),
          table(&p.bgroups_off_b, p.bgroups, false, "upload bf16 wgrad table"),
          table(&p.bsegs_off_b, p.bsegs, false, "upload bf16 wgrad segments"),
          table(&p.bsegbegin_off_b, p.bseg_begin, true, "upload bf16 wgrad segment index")};
}

// build_plan's stages and what they hand on
struct Planner : Carve {
  nrf_handle h;
  WsPlan& p;
  const nrf_model_desc& d;
  const bool train;
  const bool bft;      // bf16 training: the NeRF MLPs stash / differentiate in bfloat16
  const bool x3;       // split-bf16 inference chains (mlp_bf16x3.hip)
  const bool jac;      // tangent pass in an inference plan
  const bool bfw;      // ... and so does the SE3 trunk (warp_bf16.hip)
  const bool wstash;   // the fp32 warp kernels keep their input / sign-bit stash
  const bool rg;       // NRF_FLAG_RAY_GRADS: what nrf_backward_rays reads stays alive
  const bool frozen;   // NRF_FLAG_FROZEN: ... and nothing else of the reverse pass: no activation stash, dY, wgrad slab or reduce entry
  std::vector<size_t> rg_packT[2];      // ... a model without a warp field: the level's pack descriptors that write into rg_wpkT
  const int G;
  std::vector<GroupSpec> specs;         // fp32 wgrad groups
  std::vector<BSpec> bspecs;            // bf16 wgrad groups
  std::vector<int> nsplit, bnsplit;     // segments of each group
  std::vector<ReduceDesc> by_pass[4];   // reduce descriptors by pass (ReduceDesc::accumulate)

  Planner(nrf_handle h_, uint32_t flags)
      : h(h_), p(h_->plan), d(h_->d), train(flags & NRF_FLAG_TRAIN), bft(train && (flags & NRF_FLAG_BF16)),
        x3(!train && (flags & NRF_FLAG_BF16X3)), jac((flags & NRF_FLAG_WARP_JACOBIAN) && h_->warp),
        bfw(bft && h_->warp && !(flags & NRF_FLAG_WARP_F32)), wstash((train && !bfw) || jac), rg(train && (flags & NRF_FLAG_RAY_GRADS)),
        frozen(rg && (flags & NRF_FLAG_FROZEN)), G(h_->num_cus) {}
  void add_reduce(const ReduceDesc& r) { by_pass[r.accumulate].push_back(r); }
  // fp32 groups: leaf [kvalid][cols] <- X^T dY; the narrow heads: leaf [kvalid][vec] <- X^T v
  void gemm(int lv, int accu, Operand x, int kvalid, Operand dy, int64_t dst, int cols) {
    specs.push_back({lv, accu, x, dy, kvalid, cols, 0, dst, nullptr, nullptr, -1});
  }
  void heads(int lv, int accu, Operand x, int kvalid, int vec, int64_t dst, size_t* vecoff = nullptr, size_t* vecoff2 = nullptr,
             int64_t dst2 = -1) {
    specs.push_back({lv, accu, x, Operand{}, kvalid, vec, vec, dst, vecoff, vecoff2, dst2});
  }
  // bf16 groups: leaf [rows][cols] <- (X^T dY)[:, col0:], bias leaf (-1: none) <- column sums of dY
  BSpec& bgemm(int lv, BfSrc x, BfSrc dy, int64_t leaf, int rows, int cols, int64_t bias, int col0 = 0) {
    bspecs.push_back({lv, 0, 0, x, dy, {}, {}, rows, {{leaf, cols, col0}, {-1, 0, 0}}, {{bias, cols, 0}, {-1, 0, 0}}});
    return bspecs.back();
  }

  void shapes();
  void wgrad_specs();
  void fp32_specs(int lv);
  void warp_specs(int lv, int accu);
  void bf16_specs(int lv);
  void bf16_warp_specs(int lv, int accu, bool tangent);
  void cut_wgrad();
  void weight_streams();
  void buffers();
  void take_warp_stash(LevelWs& L, size_t nt);
  void alloc_warp(LevelWs& L, size_t nt);
  void ray_grad_buffers();
  void pack_descs();
  void fp32_groups();
  void bf16_groups();
  void bias_reduces();
  void chain_reduces();
  void tables();
};

void Planner::shapes() {
  const PlanKey& k = p.key;
  p.bfw = bfw;
  p.S[0] = d.num_coarse_samples;
  p.S[1] = d.num_coarse_samples + d.num_fine_samples;
  p.S[BG] = 1;
  p.S[TG] = 1;
  for (int lv = 0; lv < 3; ++lv) {
    p.rows[lv] = lv == BG ? k.bgN : k.B * p.S[lv];
    p.ntiles[lv] = (p.rows[lv] + TILE_ROWS - 1) / TILE_ROWS;
  }
  // the reverse chains' tiling and grids are part of the plan (the reduce table sums one bias partial per workgroup of those
  // launches); the 32-row reverse kernel has no d-points path: models with a warp field keep the 64-row one
  int nt_mlp = 0;
  for (int q = 0; q < h->nlevels; ++q) nt_mlp += p.ntiles[q];
  // ... and so does a ray-gradient plan (its d-points buffer is what nrf_backward_rays reduces)
  p.bwd32 = train && !bft && !h->warp && !rg && chain32_for(h, nt_mlp, true);   // (false for an rgb branch deeper than one layer)
  // ONE dgrad launch over the tiles of all levels: two workgroups per CU on 64-row tiles, four on 32-row half tiles
  p.grid_mlp_bwd = p.bwd32 ? tile_grid(2 * nt_mlp, 4, G) : tile_grid(nt_mlp, 2, G);
  p.grid_warp_bwd = tile_grid(nt_mlp + p.ntiles[BG], warp_grid_mul(), G);   // ONE SE3 dgrad launch: + the background tiles (0 without that batch)
  // Jacobian output / ray gradients: levels run one after the other.  Ray gradients next to the elastic regulariser: TG stays the
  // COARSE tangent level (the regulariser's reverse pass and the TG wgrad groups read it after the forward), the fine level's
  // Jacobian pass gets a scratch of its own (ray_grad_buffers)
  p.tg_tiles_per = rg && h->warp && k.elastic ? p.ntiles[0]
                   : jac || (rg && h->warp)   ? p.ntiles[h->nlevels - 1]
                   : k.elastic                ? p.ntiles[0]
                                              : 0;
  p.ntiles[TG] = 3 * p.tg_tiles_per;
  p.rows[TG] = p.ntiles[TG] * TILE_ROWS;
}

// ---- wgrad groups (training): what each multiplies, which leaves it feeds ----
void Planner::wgrad_specs() {
  if (!train || frozen) return;   // a frozen plan has no weight gradient: no group, segment or slab
  for (int lv = 0; lv < h->nlevels; ++lv) {
    if (bft) bf16_specs(lv);
    else fp32_specs(lv);
    if (h->warp && !bfw) warp_specs(lv, lv > 0 ? 1 : 0);   // the field is shared by both passes: level 1 accumulates
  }
  if (h->warp && !bfw && p.key.bgN > 0) warp_specs(BG, 2);
  if (h->warp && !bfw && p.key.elastic) warp_specs(TG, 3);   // tangent activations x tangent adjoints, same leaves
  // bf16 SE3 trunk: every pass through the field (coarse / fine samples, background points, the 3 tangents per coarse sample)
  // leaves its own X / dY stash; all of them add into the same leaves (reduce passes 0..3).  The tangent pass carries no bias.
  if (bfw) {
    for (int lv = 0; lv < h->nlevels; ++lv) bf16_warp_specs(lv, lv > 0 ? 1 : 0, false);
    if (p.key.bgN > 0) bf16_warp_specs(BG, 2, false);
    if (p.key.elastic) bf16_warp_specs(TG, 3, true);
  }
}

void Planner::fp32_specs(int lv) {
  LevelWs& L = p.L[lv];
  const MlpParamOffsets& po = h->po[lv];
  const size_t layer = (size_t)p.ntiles[lv] * FRAG_TILE_256;
  for (int l = 0; l < TRUNK_DEPTH; ++l) {
    const Operand dy = frag256(&L.dy_trunk, (size_t)l * layer);
    if (l > 0) gemm(lv, 0, frag256(&L.st_h, (size_t)(l - 1) * layer), 256, dy, po.trunk_k[l], 256);
    if (l == 0 || l == d.nerf_skip_layer) gemm(lv, 0, plain(&L.st_pe, h->PK), h->P, dy, po.trunk_k[l] + (l > 0 ? 256 * 256 : 0), 256);
  }
  gemm(lv, 0, frag256(&L.st_h, (size_t)7 * layer), 256, frag256(&L.dy_bn), po.bn_k, 256);
  gemm(lv, 0, frag256(&L.st_bn), 256, frag128(&L.dy_rgbh), po.rgbh_k, 128);
  // rgb branch layers 1..nx: the stash of the layer before x its adjoint (the 128 x 128 shape of the SE3 trunk's groups)
  const int nx = d.nerf_rgb_branch_depth - 1;
  const size_t xlayer = (size_t)p.ntiles[lv] * FRAG_TILE_128;
  for (int x = 0; x < nx; ++x)
    gemm(lv, 0, x ? frag128(&L.st_rgbx, (size_t)(x - 1) * xlayer) : frag128(&L.st_rgbh), 128, frag128(&L.dy_rgbx, (size_t)x * xlayer),
         po.rgbx_k[x], 128);
  // narrow heads on the VALU: alpha (X = h8, or the bottleneck under use_alpha_condition; vec.w) and rgb logits (X = the last
  // rgb hidden layer, vec.xyz)
  heads(lv, 0, h->A > 0 ? frag256(&L.st_bn) : frag256(&L.st_h, (size_t)7 * layer), 256, 1, po.alpha_k);
  heads(lv, 0, nx ? frag128(&L.st_rgbx, (size_t)(nx - 1) * xlayer) : frag128(&L.st_rgbh), 128, 3, po.logit_k);
}

// SE3 trunk + heads of level `lv` (coarse / fine samples, or the background-point batch, or the tangents)
void Planner::warp_specs(int lv, int accu) {
  LevelWs& L = p.L[lv];
  const WarpParamOffsets& w = h->wpo;
  const size_t wl = (size_t)p.ntiles[lv] * FRAG_TILE_128;
  for (int l = 0; l < WARP_DEPTH; ++l) {
    const Operand dy = frag128(&L.w_dy, (size_t)l * wl);
    if (l > 0) gemm(lv, accu, frag128(&L.w_st_h, (size_t)(l - 1) * wl), WARP_W, dy, w.trunk_k[l], WARP_W);
    if (l == 0 || l == WARP_SKIP)
      gemm(lv, accu, plain(&L.w_st_win, h->PKw), h->Win, dy, w.trunk_k[l] + (l > 0 ? (int64_t)WARP_W * WARP_W : 0), WARP_W);
  }
  // both heads read h6: one pass over its stash
  heads(lv, accu, frag128(&L.w_st_h, (size_t)(WARP_DEPTH - 1) * wl), WARP_W, 3, w.w_k, &L.w_dw4, &L.w_dv4, w.v_k);
}

// bf16 training: the NeRF MLP groups go to the bf16 wgrad kernel (X / dY = bf16 stash buffers of Kb / Nb blocks per 32-sample
// group); a group may also own bias gradients (column sums of its dY)
void Planner::bf16_specs(int lv) {
  LevelWs& L = p.L[lv];
  const MlpParamOffsets& po = h->po[lv];
  L.b_ngroups = (p.rows[lv] + 255) / 256 * 8;
  const size_t layer = (size_t)L.b_ngroups * 8 * BF_BLOCK_DW;
  for (int l = 0; l < TRUNK_DEPTH; ++l) {
    const BfSrc dy{&L.b_dy, (size_t)l * layer, 8};
    if (l == 0) {
      bgemm(lv, {&L.b_pe, 0, 2}, dy, po.trunk_k[0], h->P, 256, po.trunk_b[0]);
    } else if (l == d.nerf_skip_layer && h->bf16_wgrad_merge) {
      // (NRF_OPT_BF16_WGRAD_MERGE) the skip layer's kernel is [256 + P, 256]: rows 0..255 multiply h4, rows 256.. the posenc (modules.py:47-48).  ONE group,
      // X = [h4 (8 blocks) | posenc (2 blocks)] against dpre_4, so dpre_4 is streamed once (rounds 2-4: two groups, twice)
      bgemm(lv, {&L.b_h, (size_t)(l - 1) * layer, 8}, dy, po.trunk_k[l], 256 + h->P, 256, po.trunk_b[l]).x2 = {&L.b_pe, 0, 2, 2};
    } else {
      bgemm(lv, {&L.b_h, (size_t)(l - 1) * layer, 8}, dy, po.trunk_k[l], 256, 256, po.trunk_b[l]);
      if (l == d.nerf_skip_layer)   // merge off: the posenc rows of the skip layer as a group of their own (dpre_4 read twice)
        bgemm(lv, {&L.b_pe, 0, 2}, dy, po.trunk_k[l] + 256 * 256, h->P, 256, -1);
    }
  }
  const BfSrc h8{&L.b_h, (size_t)7 * layer, 8}, dsmall{&L.b_dsmall, 0, 2};
  const bool merge_alpha = h->bf16_wgrad_merge && h->A == 0;
  BSpec& bn = bgemm(lv, h8, {&L.b_dbn, 0, 8}, po.bn_k, 256, 256, po.bn_b);
  if (merge_alpha) {
    // the bottleneck AND the alpha head read h8 (modules.py:149-157): ONE group, dY = [d bottleneck (8 blocks) | d raw (block 0 of
    // the small stash)], h8 streamed once; slab column 256 + 3 (d raw sigma) is the alpha kernel's gradient
    bn.dy2 = {&L.b_dsmall, 0, 1, 2};
    bn.w[1] = {po.alpha_k, 1, 256 + 3};
  }
  bgemm(lv, {&L.b_bn, 0, 8}, {&L.b_drgbh, 0, 4}, po.rgbh_k, 256, 128, po.rgbh_b);
  // narrow heads against the "small" dY block: columns 0..2 = d rgb logits (X = rgb hidden), column 3 = d raw sigma (X = h8)
  bgemm(lv, {&L.b_rgbh, 0, 4}, dsmall, po.logit_k, 128, 3, po.logit_b).b[1] = {po.alpha_b, 1, 3};
  if (h->A > 0) bgemm(lv, {&L.b_bn, 0, 8}, dsmall, po.alpha_k, 256, 1, -1, 3);   // use_alpha_condition: X = the bottleneck
  else if (!merge_alpha) bgemm(lv, h8, dsmall, po.alpha_k, 256, 1, -1, 3);
  // (merged: the alpha head rides in the bottleneck's group above)
}

void Planner::bf16_warp_specs(int lv, int accu, bool tangent) {
  LevelWs& L = p.L[lv];
  const WarpParamOffsets& w = h->wpo;
  const int rows = tangent ? p.rows[0] : p.rows[lv];
  L.bw_ngroups = (tangent ? 3 : 1) * ((rows + 255) / 256 * 8);
  const size_t layer = (size_t)L.bw_ngroups * 4 * BF_BLOCK_DW;
  const size_t first = bspecs.size();
  auto bias = [&](int64_t b) { return tangent ? -1 : b; };
  for (int l = 0; l < WARP_DEPTH; ++l) {
    const BfSrc dy{&L.bw_dy, (size_t)l * layer, 4};
    if (l == 0) {
      bgemm(lv, {&L.bw_in, 0, 2}, dy, w.trunk_k[0], h->Win, WARP_W, bias(w.trunk_b[0]));
    } else {
      bgemm(lv, {&L.bw_h, (size_t)(l - 1) * layer, 4}, dy, w.trunk_k[l], WARP_W, WARP_W, bias(w.trunk_b[l]));
      if (l == WARP_SKIP) bgemm(lv, {&L.bw_in, 0, 2}, dy, w.trunk_k[l] + (int64_t)WARP_W * WARP_W, h->Win, WARP_W, -1);
    }
  }
  // both heads read h6 against the "small" dY block: columns 0..2 = dL/dw, 3..5 = dL/dv
  BSpec& hd = bgemm(lv, {&L.bw_h, (size_t)(WARP_DEPTH - 1) * layer, 4}, {&L.bw_dhead, 0, 2}, w.w_k, WARP_W, 3, bias(w.w_b));
  hd.w[1] = {w.v_k, 3, 3};
  hd.b[1] = {bias(w.v_b), 3, 3};
  for (size_t i = first; i < bspecs.size(); ++i) { bspecs[i].accu = accu; bspecs[i].ngroups = L.bw_ngroups; }
}

// ---- stream-K cut of both wgrad kernels' work ----
void Planner::cut_wgrad() {
  if (!specs.empty()) {
    std::vector<double> cost;
    std::vector<int> nt;
    for (const GroupSpec& s : specs) { cost.push_back(tile_cost(s)); nt.push_back(p.ntiles[s.lv]); }
    // fixed cost of opening a segment (pipeline fill + slab flush), in tiles
    nsplit = stream_k(cost, nt, env_cost("NRF_COST_SEG", 0.5), G, p.segs, p.seg_begin);
    p.wgrad_nwg = G;
  }
  if (!bspecs.empty()) {   // "tile" = 32-sample group
    std::vector<double> cost;
    std::vector<int> nt;
    for (const BSpec& s : bspecs) { cost.push_back(bcost(s)); nt.push_back(s.ngroups ? s.ngroups : p.L[s.lv].b_ngroups); }
    // opening a segment (pipeline fill + 256 KiB slab flush), in block units
    bnsplit = stream_k(cost, nt, env_cost("NRF_BCOST_SEG", 16.0), G, p.bsegs, p.bseg_begin);
    p.bwgrad_nwg = G;
  }
}

// ---- weight streams of the bf16 / x3 chains: chunks (panels) in execution order ----
void Planner::weight_streams() {
  // the bf16 chains run the skip at a compile-time layer: a model whose skip moved has no bf16 stream (check_flags refuses it)
  const int skip = SKIP_LAYER;
  p.bf_stream_ok = d.nerf_skip_layer == skip;
  for (int lv = 0; lv < h->nlevels; ++lv) {
    const MlpParamOffsets& po = h->po[lv];
    const size_t fwd_kb = x3 ? BF_X3_STREAM_KB : BF_FWD_STREAM_KB;
    p.L[lv].bf_wpk = take(fwd_kb * 256);   // KiB -> floats
    Stream f{p.L[lv].bf_wpk, 0, 0, x3, p.bfpack};
    f.gemm(2, 8, TRUNK_W, po.trunk_b[0], {{po.trunk_k[0], TRUNK_W, 0, h->P, 2}});
    for (int l = 1; l < TRUNK_DEPTH; ++l) {
      if (l == skip) f.gemm(2, 8, TRUNK_W, po.trunk_b[l], {{po.trunk_k[l], TRUNK_W, 0, TRUNK_W, 8}, {po.trunk_k[l], TRUNK_W, TRUNK_W, h->P, 2}});
      else f.gemm(2, 8, TRUNK_W, po.trunk_b[l], {{po.trunk_k[l], TRUNK_W, 0, TRUNK_W, 8}});
    }
    f.gemm(2, 8, TRUNK_W, po.bn_b, {{po.bn_k, TRUNK_W, 0, TRUNK_W, 8}});        // bottleneck
    f.gemm(1, 1, 1, po.alpha_b, {{po.alpha_k, 1, 0, TRUNK_W, 8}});               // alpha head: one block, column 0
    f.gemm(2, 4, RGB_W, -1, {{po.rgbh_k, RGB_W, 0, TRUNK_W, 8}});                // rgb hidden (bias: the fp32 per-ray term)
    f.gemm(1, 1, 3, po.logit_b, {{po.logit_k, 3, 0, RGB_W, 4}});                 // rgb logits: one block, columns 0..2
    p.bf_stream_ok = p.bf_stream_ok && f.at == fwd_kb * 256;
    if (!bft) continue;
    // dgrad stream (nerf_mlp_bwd_bf16_kernel): ncols = valid M, Part.krows = valid K
    const size_t bwd_kb = h->warp ? BF_BWD_STREAM_DPTS_KB : BF_BWD_STREAM_KB;
    p.L[lv].bf_wpkT = take(bwd_kb * 256);
    Stream b{p.L[lv].bf_wpkT, 0, 1, x3, p.bfpack};
    b.gemm(4, 4, RGB_W, -1, {{po.logit_k, 3, 0, 3, 1}});                       // G1: one k-step (3 valid) + a zero one, 4 blocks
    // the alpha head's transpose is ONE bias-style row (w_alpha[0:256], B = d sigma) in the GEMM that produces the gradient of
    // its input: the trunk output (G3), or -- use_alpha_condition, modules.py:152-157 -- the bottleneck (G2); zeros in the other
    const int64_t arow = po.alpha_k;
    b.gemm(2, 8, TRUNK_W, h->A > 0 ? arow : -2, {{po.rgbh_k, RGB_W, 0, RGB_W, 4}});             // G2: rows 0..255 of [256+R, 128]
    b.gemm(2, 8, TRUNK_W, h->A > 0 ? -2 : arow, {{po.bn_k, TRUNK_W, 0, TRUNK_W, 8}});           // G3
    for (int l = TRUNK_DEPTH - 1; l >= 1; --l) b.gemm(2, 8, TRUNK_W, -1, {{po.trunk_k[l], TRUNK_W, 0, TRUNK_W, 8}});
    if (h->warp) {   // d posenc: W0 and the skip layer's posenc rows as A [m = posenc feature (P valid)][k = output feature]
      b.gemm(2, 2, h->P, -1, {{po.trunk_k[0], TRUNK_W, 0, TRUNK_W, 8}});
      b.gemm(2, 2, h->P, -1, {{po.trunk_k[skip], TRUNK_W, TRUNK_W, TRUNK_W, 8}});
    }
    p.bf_stream_ok = p.bf_stream_ok && b.at == bwd_kb * 256;
  }
  if (h->warp) {   // bf16 SE3 trunk (warp_bf16.hip): forward stream (also for bf16 inference), reverse stream (training); x3: its doubled rows (warp_bf16x3.hip)
    const WarpParamOffsets& w = h->wpo;
    const size_t wfwd_kb = x3 ? BFW_X3_STREAM_KB : BFW_FWD_STREAM_KB;
    p.bfw_wpk = take(wfwd_kb * 256);
    Stream f{p.bfw_wpk, 0, 0, x3, p.bfpack};
    f.gemm(2, 4, WARP_W, w.trunk_b[0], {{w.trunk_k[0], WARP_W, 0, h->Win, 2}});
    for (int l = 1; l < WARP_DEPTH; ++l) {
      if (l == WARP_SKIP) f.gemm(2, 4, WARP_W, w.trunk_b[l], {{w.trunk_k[l], WARP_W, 0, WARP_W, 4}, {w.trunk_k[l], WARP_W, WARP_W, h->Win, 2}});
      else f.gemm(2, 4, WARP_W, w.trunk_b[l], {{w.trunk_k[l], WARP_W, 0, WARP_W, 4}});
    }
    f.gemm(1, 1, 6, w.w_b, {{w.w_k, 3, 0, WARP_W, 4, w.v_k, 3}}, w.v_b, 3);     // heads: columns 0..2 = w, 3..5 = v
    p.bf_stream_ok = p.bf_stream_ok && f.at == wfwd_kb * 256;
    if (bfw) {
      p.bfw_wpkT = take((size_t)BFW_BWD_STREAM_KB * 256);
      Stream b{p.bfw_wpkT, 0, 1, x3, p.bfpack};
      b.gemm(4, 4, WARP_W, -1, {{w.w_k, 3, 0, 6, 1, w.v_k, 3}});         // heads^T: K = (w0..2, v0..2) of one k-step + a zero one
      for (int l = WARP_DEPTH - 1; l >= 1; --l) b.gemm(2, 4, WARP_W, -1, {{w.trunk_k[l], WARP_W, 0, WARP_W, 4}});
      b.gemm(2, 2, h->Win, -1, {{w.trunk_k[0], WARP_W, 0, WARP_W, 4}});                  // C0: d input through layer 0
      b.gemm(2, 2, h->Win, -1, {{w.trunk_k[WARP_SKIP], WARP_W, WARP_W, WARP_W, 4}});     // C4: ... through the skip rows
      p.bf_stream_ok = p.bf_stream_ok && b.at == (size_t)BFW_BWD_STREAM_KB * 256;
    }
  }
  p.bf_desc = take(p.bfpack.size() * sizeof(RcPackDesc) / 4 + 16);
}

// the fp32 warp kernels' input / activation / (w, v) stash of nt tiles (a tangent pass keeps these three and no sign bits)
void Planner::take_warp_stash(LevelWs& L, size_t nt) {
  L.w_st_win = take(nt * ((h->PKw + 31) / 32 * 32) * TILE_ROWS);
  L.w_st_h = take(nt * FRAG_TILE_128 * WARP_DEPTH);
  L.w_st_wv = take(nt * TILE_ROWS * 8);
}

void Planner::alloc_warp(LevelWs& L, size_t nt) {
  L.wpoints = take(nt * TILE_ROWS * 3);
  L.points_raw = take(nt * TILE_ROWS * 3);
  if (frozen) {   // the tangent pass and jacobian_kernel read the trunk input, the sign words and (w, v); the ray stage reads d_points
    L.w_st_win = take(nt * ((h->PKw + 31) / 32 * 32) * TILE_ROWS);
    L.w_st_wv = take(nt * TILE_ROWS * 8);
    L.w_bits = take(nt * 4 * 64 * WARP_DEPTH);
    L.d_points = take(nt * TILE_ROWS * 3);
    return;
  }
  if (wstash) {
    take_warp_stash(L, nt);
    L.w_bits = take(nt * 4 * 64 * WARP_DEPTH);
  }
  if (train && !bfw) {
    L.d_points = take(nt * TILE_ROWS * 3);
    L.w_dy = take(nt * FRAG_TILE_128 * WARP_DEPTH);
    L.w_dw4 = take(nt * TILE_ROWS * 4);
    L.w_dv4 = take(nt * TILE_ROWS * 4);
    L.w_small_part = take((size_t)4 * G * WARP_SMALL_PART);
  }
  if (bfw) {   // bf16 trunk: fp32 rows only for what exp_se3 / the elastic kernel read and write; the rest is the bf16 stash
    const size_t ng = L.bw_ngroups;
    L.w_st_wv = take(nt * TILE_ROWS * 8);
    L.d_points = take(nt * TILE_ROWS * 3);
    L.w_dw4 = take(nt * TILE_ROWS * 4);
    L.w_dv4 = take(nt * TILE_ROWS * 4);
    L.bw_in = take(ng * 2 * BF_BLOCK_DW);
    L.bw_h = take(ng * 4 * BF_BLOCK_DW * WARP_DEPTH);
    L.bw_bits = take(ng * 64 * 2 * WARP_DEPTH);
    L.bw_dy = take(ng * 4 * BF_BLOCK_DW * WARP_DEPTH);
    L.bw_dhead = take(ng * 2 * BF_BLOCK_DW);
  }
}

// ---- per-level and shared buffers ----
void Planner::buffers() {
  const int B = p.key.B, bgN = p.key.bgN;
  p.cond = take((size_t)B * (h->R > 0 ? h->R : 1));
  p.mse = take((size_t)2 * B);   // [level][ray] squared error
  p.zero_rgb = take((size_t)B * 3);
  for (int lv = 0; lv < h->nlevels; ++lv) {
    LevelWs& L = p.L[lv];
    const size_t nt = p.ntiles[lv];
    L.wpk = take(h->pk.total);
    L.z = take((size_t)p.rows[lv]);
    L.out4 = take(nt * TILE_ROWS * 4);
    L.rgb = take((size_t)B * 3);
    L.depth = take(B);
    L.med = take(B);
    L.acc = take(B);
    L.weights = take((size_t)p.rows[lv]);
    L.condterm = take((size_t)B * RGB_W);
    if (h->A > 0) { L.alpha_ct = take(B); L.dsig_ray = take(B); }
    if (bft) {   // bf16 stashes (nrf_internal.h BfStash), dwords
      const size_t ng = L.b_ngroups;
      L.b_pe = take(ng * 2 * BF_BLOCK_DW);
      L.b_h = take(ng * 8 * BF_BLOCK_DW * TRUNK_DEPTH);
      L.b_bn = take(ng * 8 * BF_BLOCK_DW);
      L.b_rgbh = take(ng * 4 * BF_BLOCK_DW);
      L.b_bits = take(ng * 64 * 4 * (TRUNK_DEPTH + 1));
      L.b_dy = take(ng * 8 * BF_BLOCK_DW * TRUNK_DEPTH);
      L.b_dbn = take(ng * 8 * BF_BLOCK_DW);
      L.b_drgbh = take(ng * 4 * BF_BLOCK_DW);
      L.b_dsmall = take(ng * 2 * BF_BLOCK_DW);
      L.d_raw4 = take(nt * TILE_ROWS * 4);
    } else if (frozen) {   // the data-gradient chain reads the sign words and the posenc stash, not the activations
      L.st_pe = take(nt * ((h->PK + 31) / 32 * 32) * TILE_ROWS);
      L.bits_trunk = take(nt * 4 * 128 * TRUNK_DEPTH);
      L.bits_rgbh = take(nt * 4 * 64);
      L.d_raw4 = take(nt * TILE_ROWS * 4);
      if (const size_t nx = d.nerf_rgb_branch_depth - 1) L.bits_rgbx = take(nx * nt * 4 * 64);
    } else if (train) {
      L.st_pe = take(nt * ((h->PK + 31) / 32 * 32) * TILE_ROWS);
      L.st_h = take(nt * FRAG_TILE_256 * TRUNK_DEPTH);
      L.st_bn = take(nt * FRAG_TILE_256);
      L.st_rgbh = take(nt * FRAG_TILE_128);
      L.bits_trunk = take(nt * 4 * 128 * TRUNK_DEPTH);
      L.bits_rgbh = take(nt * 4 * 64);
      L.d_raw4 = take(nt * TILE_ROWS * 4);
      L.dy_trunk = take(nt * FRAG_TILE_256 * TRUNK_DEPTH);
      L.dy_bn = take(nt * FRAG_TILE_256);
      L.dy_rgbh = take(nt * FRAG_TILE_128);
      if (const size_t nx = d.nerf_rgb_branch_depth - 1) {   // rgb branch layers 1..nx: stash, sign bits, adjoints
        L.st_rgbx = take(nx * nt * FRAG_TILE_128);
        L.bits_rgbx = take(nx * nt * 4 * 64);
        L.dy_rgbx = take(nx * nt * FRAG_TILE_128);
      }
    }
    if (frozen) {
      L.dray = take((size_t)B * RGB_W);
    } else if (train) {
      L.dray = take((size_t)B * RGB_W);
      L.small_part = take((size_t)4 * G * SMALL_PART);   // up to four workgroups per CU (32-row reverse chain)
      L.cond_grad = take((size_t)(h->R > 0 ? h->R : 1) * RGB_W);
    }
    if (h->warp) alloc_warp(L, nt);
  }
  if (h->warp && bgN > 0) {
    alloc_warp(p.L[BG], p.ntiles[BG]);
    p.bg_loss = take(64);
    p.bg_points = take((size_t)bgN * 3);   // the library's own draw (nrf_background.warp_ids == NULL): noised points, ids
    p.bg_ids = take((size_t)bgN);
  }
  if (h->time_enc) {
    p.t_codes = take((size_t)B * h->G);
    if (train && !frozen) {
      p.t_dcodes = take((size_t)B * h->G);
      p.t_in = take((size_t)B * TIME_MAX_IN);
      p.t_h = take((size_t)B * TIME_DEPTH * TIME_W);
      p.t_dpre = take((size_t)B * TIME_DEPTH * TIME_W);
    }
  }
  if (jac && !train) alloc_warp(p.L[TG], p.ntiles[TG]);
  if (h->warp && train && !frozen) p.wr_sums = take(64);
  if (h->warp && p.key.elastic && train) {
    alloc_warp(p.L[TG], p.ntiles[TG]);
    p.L[0].el_dw4 = take((size_t)p.ntiles[0] * TILE_ROWS * 4);
    p.L[0].el_dv4 = take((size_t)p.ntiles[0] * TILE_ROWS * 4);
    p.el_sums = take((size_t)5 * (p.ntiles[0] * TILE_ROWS / 256 + 1));
    p.el_coef = take((size_t)p.rows[0]);
  }
  if (h->warp) p.warp_wpk = take(h->wpk.total);
  p.seg_clock = take(2 * (p.segs.size() + 1));
  p.counters = take(64);
  p.timeline = take(2 * TIMELINE_LEVEL_F);
}

// ---- NRF_FLAG_RAY_GRADS: everything the flag adds, behind every offset a plan without it has ----
void Planner::ray_grad_buffers() {
  if (!rg) return;
  for (int lv = 0; lv < h->nlevels; ++lv) {
    LevelWs& L = p.L[lv];
    const size_t nt = p.ntiles[lv];
    L.rg_sdsig = take(p.key.B);
    if (h->warp) {
      L.rg_jac = take(nt * TILE_ROWS * 9);
    } else {
      L.d_points = take(nt * TILE_ROWS * 3);
      // a whole second image: the reverse chain takes ONE wpk base and PackOffsets relative to it, so the transposed layers keep
      // their slots (the forward layers' slots stay unused), W0^T / skip rows^T and the prefetch slack behind them
      L.rg_wpkT = take((size_t)p.rg_L4bT + 256 * 64 + 4096);
      for (size_t i : rg_packT[lv]) p.pack[i].dst_off += (int64_t)L.rg_wpkT;   // built relative to it by pack_descs
    }
  }
  if (!h->warp) return;
  if (p.key.elastic) {   // TG is the elastic regulariser's (buffers()) and serves the coarse Jacobian; the fine pass runs beside it
    if (h->nlevels < 2) return;
    LevelWs& F = p.rg_tan_fine;
    const size_t nt = (size_t)3 * p.ntiles[1];
    F.wpoints = take(nt * TILE_ROWS * 3);
    take_warp_stash(F, nt);
    return;
  }
  // the tangent pass of one level at a time (as the inference Jacobian plan): its input / activation / (w, v) stash
  LevelWs& T = p.L[TG];
  const size_t nt = p.ntiles[TG];
  if (frozen) {   // jacobian_kernel reads the tangent (dw, dv) rows; nothing reads the tangent inputs or activations
    T.w_st_wv = take(nt * TILE_ROWS * 8);
    return;
  }
  T.wpoints = take(nt * TILE_ROWS * 3);
  take_warp_stash(T, nt);
}

// ---- pack descriptors (both levels, forward and transposed streams); a bf16 TRAINING plan reads only the bf16 images of the
//      NeRF MLPs (bfpack), so their fp32 fragment images are not rebuilt every step ----
void Planner::pack_descs() {
  for (int lv = 0; lv < (bft ? 0 : h->nlevels); ++lv) {
    const size_t first = p.pack.size();
    const int64_t base = (int64_t)p.L[lv].wpk;
    mlp_pack_descs(h, lv, base, true, p.pack);
    if (!rg || h->warp) continue;
    // ray gradients without a warp field: the reverse chain reads its transposed images (and the two d-posenc ones) from rg_wpkT,
    // taken behind everything else: those descriptors are made relative to it here and moved onto it by ray_grad_buffers
    p.rg_L0T = h->pk.total; p.rg_L4bT = p.rg_L0T + 256 * 64;   // behind the level's own images and their prefetch slack
    const MlpParamOffsets& po = h->po[lv];
    p.pack.push_back(PackDesc{po.trunk_k[0], base + p.rg_L0T, 256, 0, 256, 256, 2, 1, 1, h->P});
    p.pack.push_back(PackDesc{po.trunk_k[d.nerf_skip_layer], base + p.rg_L4bT, 256, 256, 256, 256, 2, 1, 1, h->P});
    for (size_t i = first; i < p.pack.size(); ++i)
      if (p.pack[i].transposed) { p.pack[i].dst_off -= base; rg_packT[lv].push_back(i); }
  }
  // fp32 fragment images of the SE3 trunk (a bf16-trunk training plan reads only its bf16 streams)
  if (h->warp && !bfw) warp_pack_descs(h, h->wpo, (int64_t)p.warp_wpk, !frozen, p.pack);   // frozen: no SE3 reverse chain, no W^T images
}

// ---- fp32 wgrad groups: slabs (taken in group order) + reduce descriptors ----
void Planner::fp32_groups() {
  int first = 0;
  for (size_t i = 0; i < specs.size(); ++i) {
    const GroupSpec& s = specs[i];
    WgradGroup g;
    memset(&g, 0, sizeof(g));
    g.x_off = (int64_t)(*s.x.off + s.x.add); g.x_kind = s.x.kind; g.x_tile_stride = s.x.stride; g.x_kvalid = s.kvalid; g.Kb = s.x.blocks;
    g.dy_off = s.dy.off ? (int64_t)(*s.dy.off + s.dy.add) : 0; g.dy_kind = s.dy.kind; g.dy_tile_stride = s.dy.stride; g.Nb = s.dy.blocks;
    g.ntiles = p.ntiles[s.lv];
    g.nsplit = nsplit[i];
    g.first_task = first;
    first += g.nsplit;
    g.vec_off = g.vec2_off = -1;
    if (s.vec) {   // two vec4 partial rows per segment
      const int64_t part = (int64_t)g.Kb * 32 * 4;
      g.vec_off = (int64_t)(s.vecoff ? *s.vecoff : p.L[s.lv].d_raw4);
      g.vslab_off = (int64_t)take((size_t)g.nsplit * 2 * g.Kb * 32 * 4);
      if (s.vecoff2) {
        g.vec2_off = (int64_t)*s.vecoff2;
        g.vslab2_off = (int64_t)take((size_t)g.nsplit * 2 * g.Kb * 32 * 4);
        add_reduce(reduce_desc(s.dst2, s.cols, s.kvalid, s.cols, g.vslab2_off, 4, part, 2 * g.nsplit, s.accumulate));
      }
      add_reduce(reduce_desc(s.dst, s.cols, s.kvalid, s.cols, g.vslab_off + (s.vec == 1 ? 3 : 0), 4, part, 2 * g.nsplit, s.accumulate));
    } else {
      g.slab_off = (int64_t)take((size_t)g.nsplit * g.Kb * 32 * g.Nb * 32);
      add_reduce(reduce_desc(s.dst, s.cols, s.kvalid, s.cols, g.slab_off, g.Nb * 32, (int64_t)g.Kb * 32 * g.Nb * 32, g.nsplit,
                             s.accumulate));
    }
    p.groups.push_back(g);
  }
}

// ---- bf16 wgrad groups: slab [Kb*32][Nb*32] per segment (+ a bias slab [Nb*32]); each leaf takes a column window of it ----
void Planner::bf16_groups() {
  for (size_t i = 0; i < bspecs.size(); ++i) {
    const BSpec& s = bspecs[i];
    const int Kb = s.x.blocks + s.x2.blocks, Nb = s.dy.blocks + s.dy2.blocks;
    WgradGroup g;
    memset(&g, 0, sizeof(g));
    g.x_off = (int64_t)(*s.x.off + s.x.add); g.x_tile_stride = s.x.blocks * BF_BLOCK_DW; g.Kb = Kb; g.x_kvalid = s.rows; g.Kb1 = s.x.blocks;
    g.dy_off = (int64_t)(*s.dy.off + s.dy.add); g.dy_tile_stride = s.dy.blocks * BF_BLOCK_DW; g.Nb = Nb; g.Nb1 = s.dy.blocks;
    g.x2_off = s.x2.off ? (int64_t)*s.x2.off : g.x_off; g.x2_tile_stride = s.x2.stride * BF_BLOCK_DW;
    g.dy2_off = s.dy2.off ? (int64_t)*s.dy2.off : g.dy_off; g.dy2_tile_stride = s.dy2.stride * BF_BLOCK_DW;
    g.ntiles = s.ngroups ? s.ngroups : p.L[s.lv].b_ngroups; g.nsplit = bnsplit[i]; g.vec_off = -1; g.vec2_off = -1;
    g.slab_off = (int64_t)take((size_t)g.nsplit * Kb * 32 * Nb * 32);
    g.vslab_off = s.b[0].off >= 0 ? (int64_t)take((size_t)g.nsplit * Nb * 32) : -1;
    p.bgroups.push_back(g);
    for (const Leaf& l : s.w)
      if (l.off >= 0)
        add_reduce(reduce_desc(l.off, l.cols, s.rows, l.cols, g.slab_off + l.col0, Nb * 32, (int64_t)Kb * 32 * Nb * 32, g.nsplit, s.accu));
    for (const Leaf& b : s.b)
      if (b.off >= 0) add_reduce(reduce_desc(b.off, b.cols, 1, b.cols, g.vslab_off + b.col0, Nb * 32, Nb * 32, g.nsplit, s.accu));
  }
}

// ---- bias gradients of the fp32 dgrad launches (per-workgroup partials) and the per-ray condition rows ----
void Planner::bias_reduces() {
  for (int lv = 0; lv < h->nlevels; ++lv) {
    const MlpParamOffsets& po = h->po[lv];
    const LevelWs& L = p.L[lv];
    auto small = [&](int64_t dst, int cols, int sp_off) {
      if (bft) return;   // the bf16 wgrad kernel sums the bias columns itself
      add_reduce(reduce_desc(dst, cols, 1, cols, (int64_t)L.small_part + sp_off, cols, SMALL_PART, p.grid_mlp_bwd));
    };
    for (int l = 0; l < TRUNK_DEPTH; ++l) small(po.trunk_b[l], TRUNK_W, SP_DB_TRUNK + l * TRUNK_W);
    small(po.bn_b, TRUNK_W, SP_DB_BN);
    small(po.rgbh_b, RGB_W, SP_DB_RGBH);
    small(po.logit_b, 3, SP_DB_LOGIT);
    small(po.alpha_b, 1, SP_DB_ALPHA);
    for (int x = 0; x < d.nerf_rgb_branch_depth - 1; ++x) small(po.rgbx_b[x], RGB_W, SP_DB_RGBX + x * RGB_W);
    if (h->R > 0) add_reduce(reduce_desc(po.rgbh_k + 256 * 128, 128, h->R, 128, (int64_t)L.cond_grad, 128, 0, 1));
    if (h->warp && !bfw && lv == 0) {   // the SE3 dgrad launch writes one set of bias partials for all its levels
      const WarpParamOffsets& w = h->wpo;
      auto wsmall = [&](int64_t dst, int cols, int sp_off) {
        add_reduce(reduce_desc(dst, cols, 1, cols, (int64_t)L.w_small_part + sp_off, cols, WARP_SMALL_PART, p.grid_warp_bwd));
      };
      for (int l = 0; l < WARP_DEPTH; ++l) wsmall(w.trunk_b[l], WARP_W, WSP_DB_TRUNK + l * WARP_W);
      wsmall(w.w_b, 3, WSP_DB_W);
      wsmall(w.v_b, 3, WSP_DB_V);
    }
  }
}

// Every pass of a destination in ONE launch: the descriptors that add into a leaf (the SE3 field's: fine level, tangent pass,
// background batch) are chained behind the pass-0 descriptor of the same destination window; a workgroup column of reduce_kernel
// walks the chain with one element -> thread mapping.  Heads first (the launch's grid), chained descriptors behind them.
void Planner::chain_reduces() {
  std::vector<ReduceDesc> all;
  for (const std::vector<ReduceDesc>& pass : by_pass) all.insert(all.end(), pass.begin(), pass.end());
  auto wide_ok = [](const ReduceDesc& d) {
    return ((d.cols | d.src_ld | d.dst_ld) & 3) == 0 && (d.part_stride & 3) == 0 && (d.src_off & 3) == 0 && (d.dst_off & 3) == 0;
  };
  const int n = (int)all.size();
  std::vector<int> prev(n, -1), nxt(n, -1);
  for (int i = 0; i < n; ++i) {
    if (all[i].accumulate == 0) continue;
    for (int j = i - 1; j >= 0; --j)   // the latest earlier descriptor of the same destination window that is still a chain's tail
      if (nxt[j] < 0 && all[j].dst_off == all[i].dst_off && all[j].rows == all[i].rows && all[j].cols == all[i].cols &&
          all[j].dst_ld == all[i].dst_ld && all[j].accumulate < all[i].accumulate) { prev[i] = j; nxt[j] = i; break; }
  }
  std::vector<int> order, pos(n, -1);
  for (int i = 0; i < n; ++i) if (prev[i] < 0 && all[i].accumulate == 0) order.push_back(i);          // heads of pass 0
  const int nheads0 = (int)order.size();
  for (int i = 0; i < n; ++i) if (prev[i] >= 0) order.push_back(i);                                    // chained
  const int nchained_end = (int)order.size();
  for (int i = 0; i < n; ++i) if (prev[i] < 0 && all[i].accumulate != 0) order.push_back(i);          // no pass-0 partner: a second launch
  for (int k = 0; k < (int)order.size(); ++k) pos[order[k]] = k;
  p.reduce.clear();
  for (int k = 0; k < (int)order.size(); ++k) {
    ReduceDesc d = all[order[k]];
    d.next = nxt[order[k]] >= 0 ? pos[nxt[order[k]]] : -1;
    p.reduce.push_back(d);
  }
  for (int k = 0; k < (int)p.reduce.size(); ++k) {   // one mapping per chain, chosen at its head
    if (k >= nheads0 && k < nchained_end) continue;
    bool tall = p.reduce[k].rows == 1, wide = true, big = false;
    for (int q = k; q >= 0; q = p.reduce[q].next) { wide = wide && wide_ok(p.reduce[q]); big = big || p.reduce[q].nparts >= 64; }
    const int path = (tall && big) ? 2 : wide ? 1 : 0;
    for (int q = k; q >= 0; q = p.reduce[q].next) p.reduce[q].path = path;
  }
  p.nreduce_pass[0] = nheads0;
  p.nreduce_pass[1] = nchained_end - nheads0;            // reached through `next`, not launched
  p.nreduce_pass[2] = (int)order.size() - nchained_end;  // launched second (empty in every configuration built so far)
  p.nreduce_pass[3] = 0;
}

// ---- descriptor tables (bytes) ----
void Planner::tables() {
  size_t bytes = 0;
  for (const Table& t : tables_of(h)) {
    *t.off_b = bytes;
    bytes += align_up(t.bytes + t.slack, 256);
  }
  p.tables = take(bytes / 4);
}

}  // namespace

// Lays out the workspace for B rays and (re)builds the descriptor tables.  The order of the take() calls is the layout: padded
// parameter image, bf16 weight streams, per-level buffers (counters and timeline last), wgrad slabs, descriptor tables.
void build_plan(nrf_handle h, int B, uint32_t flags, int bgN, int elastic) {
  const PlanKey key{B, plan_flags(flags), bgN, elastic, h->chain_rows_opt, h->bf16_wgrad_merge};
  if (h->plan.key == key) return;
  static std::atomic<uint64_t> next_serial{1};   // handles may be planned from several host threads
  h->plan = WsPlan();
  h->plan.key = key;
  h->plan.serial = next_serial++;
  Planner s(h, key.flags);
  s.shapes();
  s.wgrad_specs();
  s.cut_wgrad();
  if (h->embed) {
    h->plan.iparams = s.take((size_t)h->nparams);
    if (s.train && !s.frozen) h->plan.igrad = s.take((size_t)h->nparams);
  }
  // The bf16 / x3 chains have their layer list compiled in: a handle with a deeper rgb branch builds none of their stream
  // descriptors (check_flags refuses those modes for it)
  if (h->d.nerf_rgb_branch_depth > 1) h->plan.bf_stream_ok = false;
  else if (!s.train || s.bft) s.weight_streams();
  s.buffers();
  s.pack_descs();
  if (s.train && !s.frozen) {
    s.fp32_groups();
    s.bf16_groups();
    s.bias_reduces();
  }
  s.chain_reduces();
  s.tables();
  s.ray_grad_buffers();   // the flag's buffers lie behind everything a plan without it has

  h->plan.total_floats = s.o;
}

int upload_tables(nrf_handle h, float* ws, hipStream_t stream) {
  WsPlan& p = h->plan;
  if (h->uploaded_ws == (void*)ws && h->uploaded_key == p.key) return NRF_OK;
  char* base = reinterpret_cast<char*>(ws + p.tables);
  for (const Table& t : tables_of(h)) {
    if (!t.upload || !t.bytes) continue;
    const hipError_t e = hipMemcpyAsync(base + *t.off_b, t.data, t.bytes, hipMemcpyHostToDevice, stream);
    if (e != hipSuccess) return fail_hip(e, t.what);
  }
  if (!p.bfpack.empty()) {   // the bf16 pack table has a region of its own
    const hipError_t e = hipMemcpyAsync(ws + p.bf_desc, p.bfpack.data(), p.bfpack.size() * sizeof(RcPackDesc), hipMemcpyHostToDevice, stream);
    if (e != hipSuccess) return fail_hip(e, "upload bf16 pack table");
  }
  h->uploaded_ws = ws;
  h->uploaded_key = p.key;
  return NRF_OK;
}

void query_device(nrf_handle h) {
  if (h->cu_queried) return;
  int dev = 0, cus = 0;
  if (hipGetDevice(&dev) == hipSuccess &&
      hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && cus > 0)
    h->num_cus = cus;
  h->cu_queried = true;
}

}  // namespace api
}  // namespace nrf
