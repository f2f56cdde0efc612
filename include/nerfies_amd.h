/* nerfies_amd.h -- C-ABI of the MI355X-native nerfies hot path.
 *
 * The reference (google/nerfies) is pure Python on JAX and has NO FFI / plugin
 * boundary: the seam this library replaces is the Python call
 *   NerfModel.apply            nerfies/models.py:289-375
 * together with its two callers
 *   training.train_step        nerfies/training.py:138-271
 *   evaluation.render_image    nerfies/evaluation.py:28-101
 * Each entry point below cites the reference function it stands in for.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no C++/torch types.
 *   - every pointer is a DEVICE pointer (HBM) unless the name ends in _host.
 *   - the caller owns every buffer, including the workspace; the library never
 *     allocates, frees or synchronises per call (hipGraph-capture safe).
 *   - all work is enqueued on the caller's hipStream_t (passed as void*).
 *   - every entry returns 0 on success or a negative NRF_E_* code; nothing
 *     throws or aborts.  nrf_last_error() returns the message of the last failing
 *     call MADE BY THE CALLING THREAD (thread-local storage; valid until that thread's
 *     next failing call).  Handles carry no error state, so the errors of several threads never mix.
 *   - a handle caches ONE workspace plan -- the layout for the (num_rays, flags, regularisers) of its most recent call -- and
 *     the descriptor tables it uploads into a workspace belong to that plan.  Calls on one handle must therefore be SERIALISED
 *     by the caller (one host thread at a time, launches of different (num_rays, flags) on different streams ordered by the
 *     caller); changing the batch size or the flags between calls is fine (the plan is rebuilt, the tables re-uploaded), and
 *     nrf_backward refuses a workspace whose forward was stashed under another plan (NRF_E_STATE).  For concurrent streams
 *     or threads create one handle per stream: nrf_create is host-only and cheap.
 *   - grad_params must be 16-byte aligned (it is cleared and accumulated into with 128-bit accesses; NRF_E_SHAPE otherwise).
 *   - fp32 everywhere (the reference computes in fp32); ids are int32.
 */
#ifndef NERFIES_AMD_H_
#define NERFIES_AMD_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NRF_VERSION 660 /* 0.6.6: NRF_FLAG_FROZEN + nrf_loss_grad_rays: ray gradients with the field's parameters fixed (aligning a camera
                           against a trained field).  A frozen stash keeps what nrf_backward_rays reads and nothing of the parameter
                           gradient; nrf_backward_rays accepts grad_params == NULL on such a stash.  Plans without the flag, and every
                           entry point that existed, are unchanged.
                           0.6.5: nrf_train_step_loss_grad_rays (the fused train step with ray gradients; nrf_workspace_bytes_ex accepts
                           NRF_FLAG_TRAIN | NRF_FLAG_RAY_GRADS together with the regularisers) and camera delta tables
                           (NRF_CAMERA_DELTA_ROW): nrf_camera_table_compose / _compose_backward.  Plans without the flag, and plans
                           with the flag but without regularisers, are unchanged.
                           0.6.4: camera tables (NRF_CAMERA_ROW): nrf_camera_table_rays / _project and their reverse passes into the camera
                           parameters (nrf_camera_table_rays_backward / _project_backward, nrf_camera_table_workspace_bytes).  Nothing
                           that existed changes.
                           0.6.3: NRF_FLAG_RAY_GRADS + nrf_backward_rays (nrf_ray_grads): gradients w.r.t. the ray origins, directions and
                           viewdirs (float32 training mode).  nrf_backward / nrf_backward_ex and every plan without the flag are unchanged.
                           0.6.2: nrf_backward_ex (nrf_output_grads): cotangents for depth, acc, weights and warped_points next to
                           rgb.  nrf_backward is unchanged.
                           0.6.1: nerf_rgb_branch_depth accepts 1..4 (float32 mode, 64-row chains; the bfloat16 / split-bf16 modes and
                           NRF_OPT_CHAIN_TILE_ROWS = 32 are refused for a handle with depth > 1); the parameter layout then holds
                           MLP_1/hidden_1.. of both levels.  Nothing changes for depth 1.
                           0.6.0: nrf_model_desc grows warp_trunk_depth / warp_trunk_width (SE3Field / TranslationField trunk_depth <= 6,
                           trunk_width <= 128 of ModelConfig.warp_kwargs); nerf_skip_layer accepts any single index 1..7 (float32
                           mode; the bfloat16 mode where the trunk can be laid out around the chains' layer 4); NRF_FLAG_BF16X3 (split-bf16,
                           float32-emulating inference chains).  Behaviour change
                           since 0.5.0: the flag word is validated on every entry point -- NRF_FLAG_TRAIN | NRF_FLAG_NO_WARP is refused
                           also for models without a warp field (it used to be a no-op there), NRF_FLAG_WARP_F32 without NRF_FLAG_BF16
                           is refused by nrf_train_step_loss_grad_ex as well.
                           0.5.0: nrf_set_option (NRF_OPT_CHAIN_TILE_ROWS: 32-row tiling of the fp32 chains).
                           0.4.0: NRF_FLAG_BF16 also runs the SE3 trunk in bfloat16 (NRF_FLAG_WARP_F32 opts out).
                           0.3.0: device-resident per-step scalars (a whole train step replays from one hipGraph), background ids /
                           noise drawn by the library, `points` output without the warp field.
                           0.2.0: alpha condition, pre-encoded metadata, warp Jacobian output, noise_std, warp_reg loss,
                           elastic loss types, time metadata encoder, stats[16], bf16 training */

enum {
  NRF_OK = 0,
  NRF_E_NULL = -1,        /* null pointer */
  NRF_E_SHAPE = -2,       /* bad size / shape */
  NRF_E_UNSUPPORTED = -3, /* configuration outside what the kernels cover */
  NRF_E_HIP = -4,         /* HIP runtime error (see nrf_last_error) */
  NRF_E_WORKSPACE = -5,   /* workspace too small */
  NRF_E_STATE = -6        /* call order (backward without a stashed forward) */
};

enum { NRF_ACT_RELU = 0, NRF_ACT_SOFTPLUS = 1 };
enum { NRF_WARP_SE3 = 0, NRF_WARP_TRANSLATION = 1 };   /* ModelConfig.warp_field_type (configs.py:99-100) */
enum { NRF_META_GLO = 0, NRF_META_TIME = 1 };           /* ModelConfig.warp_metadata_encoder_type (configs.py:101) */

/* Every NerfModel attribute that reaches the hot path (models.py:75-119), as
 * POD.  Defaults are those of configs.ModelConfig (configs.py:35-105). */
typedef struct nrf_model_desc {
  int32_t num_coarse_samples;      /* models.py:75  */
  int32_t num_fine_samples;        /* models.py:76  (0 = coarse only) */
  int32_t use_viewdirs;            /* models.py:77  */
  float near_plane;                /* models.py:78  */
  float far_plane;                 /* models.py:79  */
  int32_t nerf_trunk_depth;        /* 1..8; the kernels run 8 layers, a shallower trunk gets internal identity layers behind it */
  int32_t nerf_trunk_width;        /* <= 256; the kernels are 256 wide, narrower trunks run zero-padded (test_vrig.gin: 128) */
  int32_t nerf_rgb_branch_depth;   /* 1..4 (modules.py:129-134): layer 0 reads [bottleneck, condition], layers 1.. are (width, width), leaves
                                      MLP_1/hidden_1.. in flax order.  Depth > 1 runs the float32 64-row chains only: NRF_FLAG_BF16 /
                                      NRF_FLAG_BF16X3 and NRF_OPT_CHAIN_TILE_ROWS = 32 -> NRF_E_UNSUPPORTED.  0 (the logits straight on
                                      [bottleneck, condition]) and > 4 are refused by nrf_create */
  int32_t nerf_rgb_branch_width;   /* <= 128 (same) */
  int32_t nerf_skip_layer;         /* nerf_skips = (s,) -> s in 1..7 (modules.py:47-48: layer s reads [h, posenc]); -1 = none (or any index
                                      >= nerf_trunk_depth: never reached).  s <= 4 with nerf_trunk_depth - s <= 4 is laid out around the chains'
                                      own skip at layer 4 (identity layers in between: exact) and runs in every mode; any other s runs
                                      the float32 chains with the skip GEMM at layer s (NRF_FLAG_BF16 -> NRF_E_UNSUPPORTED) */
  int32_t use_stratified_sampling; /* models.py:88; eval.py:239 forces 0 */
  int32_t num_nerf_point_freqs;    /* models.py:89  */
  int32_t num_nerf_viewdir_freqs;  /* models.py:90  */
  int32_t sigma_activation;        /* NRF_ACT_*  (defaults.gin:66 softplus) */
  int32_t use_white_background;
  int32_t use_linear_disparity;
  int32_t use_sample_at_infinity;
  /* metadata / conditions (models.py:186-228) */
  int32_t use_appearance_metadata;
  int32_t num_appearance_embeddings; /* max(appearance_ids)+1, models.py:121 */
  int32_t num_appearance_features;
  int32_t use_camera_metadata;
  int32_t num_camera_embeddings;
  int32_t num_camera_features;
  int32_t use_alpha_condition; /* also gates appearance->rgb (models.py:206) */
  int32_t use_rgb_condition;   /* accepted, unused -- as in the reference */
  int32_t use_trunk_condition; /* never forwarded by construct_nerf */
  /* warp field (warping.py:202-389, SE3Field) */
  int32_t use_warp;
  int32_t num_warp_freqs;
  int32_t num_warp_embeddings;
  int32_t num_warp_features;
  int32_t warp_field_type;         /* NRF_WARP_SE3 (warping.py:202-389, every preset) or NRF_WARP_TRANSLATION
                                      (warping.py:62-199, the dataclass default): leaves warp_field/mlp/... */
  float noise_std;                 /* models.py:80, model_utils.noise_regularize (model_utils.py:266-282): N(0, noise_std) added to
                                      the raw density when > 0 and use_stratified_sampling; 0 = off (every preset) */
  int32_t warp_metadata_encoder_type; /* NRF_META_GLO (every preset) or NRF_META_TIME: modules.TimeEncoder on
                                      metadata['time'] (modules.py:297-322, warping.py:256-259, models.py:252-254) */
  int32_t num_time_encoder_freqs;  /* metadata_encoder_num_freqs (warping.py:234): 1 */
  /* ModelConfig.warp_kwargs (configs.py:105) that reach the trunk of SE3Field / TranslationField (warping.py:225-227, 80-82):
   * 0 = the field's default.  A shallower / narrower trunk runs on the 6 x 128 kernels with identity layers behind its last one and
   * zero padding (exact); `skips` stays (4,) -- a trunk of <= 4 layers never reaches it.  The other warp_kwargs (rotation /
   * pivot / translation branch depths, use_pivot, use_translation, activation, min / max_freq_log2) are not built: the Python
   * host refuses them unless they equal the field's defaults. */
  int32_t warp_trunk_depth;        /* 1..6, 0 -> 6   */
  int32_t warp_trunk_width;        /* 1..128, 0 -> 128 */
} nrf_model_desc;

typedef struct nrf_handle_s* nrf_handle;

/* One leaf of the parameter tree inside the single flat fp32 buffer.  `name`
 * is the flax path below params['model'], e.g.
 * "nerf_mlps_coarse/MLP_0/hidden_4/kernel" -- kernels are [in,out] row-major
 * exactly as flax nn.Dense stores them. */
typedef struct nrf_tensor_info {
  char name[96];
  int64_t offset; /* in floats from the start of the flat buffer */
  int32_t rows;   /* in  (embedding: num_embeddings) ; bias: 1 */
  int32_t cols;   /* out (embedding: features) */
} nrf_tensor_info;

/* rays_dict of NerfModel.__call__ (models.py:300-329). */
typedef struct nrf_rays {
  int32_t num_rays;
  const float* origins;          /* (B,3) */
  const float* directions;       /* (B,3) */
  const float* viewdirs;         /* (B,3) or NULL -> directions (models.py:326-329) */
  const int32_t* warp_ids;       /* (B,) metadata['warp'] or NULL */
  const int32_t* appearance_ids; /* (B,) or NULL */
  const int32_t* camera_ids;     /* (B,) or NULL */
  /* metadata_encoded=True (models.py:198-199, 210-211, 251; warping.py:378-381): the per-ray codes themselves instead
   * of ids into the embedding tables.  A non-NULL *_codes pointer replaces the matching *_ids.  Inference only. */
  const float* warp_codes;       /* (B, num_warp_features) */
  const float* appearance_codes; /* (B, num_appearance_features) */
  const float* camera_codes;     /* (B, num_camera_features) */
  const float* time;             /* (B,) metadata['time'] in [-1,1] (datasets/core.py:272-274); NRF_META_TIME only */
} nrf_rays;

/* The scalars that change from one optimisation step to the next (train.py:280-285 recomputes them from the schedules; the
 * rng key advances), in DEVICE memory.  A launch sequence captured into a hipGraph bakes every by-value argument in; with
 * nrf_step_scalars.dynamic set, the kernels read these values from the device instead, so the caller rewrites this struct
 * (one 64-byte host-to-device copy ahead of the replay) and replays the SAME graph for every step.  adam_c1 / adam_c2 are
 * the bias corrections 1 - beta^(step+1), formed in double on the host exactly as nrf_adam_step forms them. */
typedef struct nrf_dynamic_scalars {
  float warp_alpha;           /* replaces nrf_step_scalars.warp_alpha */
  float time_alpha;           /* replaces nrf_step_scalars.time_alpha */
  float elastic_loss_weight;  /* replaces nrf_elastic.loss_weight */
  float learning_rate;        /* nrf_adam_step_dynamic */
  float adam_c1;              /* nrf_adam_step_dynamic: 1 - beta1^(step+1) */
  float adam_c2;              /* nrf_adam_step_dynamic: 1 - beta2^(step+1) */
  float grad_scale;           /* nrf_adam_step_dynamic: 1 / world_size */
  float reserved0;
  uint64_t rng_seed;          /* replaces nrf_rand.seed (sampling streams, noise, the background draw) */
  uint64_t rng_offset;        /* replaces nrf_rand.offset */
  uint64_t reserved1[2];
} nrf_dynamic_scalars;        /* 64 bytes */

/* Writes *host_values into the device struct with a one-thread kernel on `stream` (the values travel as kernel arguments:
 * no host buffer has to outlive the call, nothing synchronises).  Call it ahead of every graph replay. */
int nrf_dynamic_scalars_write(nrf_dynamic_scalars* device_dst, const nrf_dynamic_scalars* host_values, void* stream);

/* warp_extra + the per-step scalars of training.ScalarParams (training.py:35-43). */
typedef struct nrf_step_scalars {
  float warp_alpha; /* warp_extra['alpha'] */
  float time_alpha; /* warp_extra['time_alpha']: annealing of the TimeEncoder's posenc (NRF_META_TIME) */
  const nrf_dynamic_scalars* dynamic; /* DEVICE pointer or NULL: when set, it overrides warp_alpha / time_alpha above,
                                         nrf_rand.seed / offset and nrf_elastic.loss_weight (graph-replayable step) */
} nrf_step_scalars;

/* Stand-in for the flax RNG streams 'coarse' / 'fine' (models.py:333,355).
 * Either explicit uniforms (parity runs) or an on-device Philox4x32-10 keyed by
 * (seed, offset) (throughput runs).  Ignored when use_stratified_sampling=0. */
typedef struct nrf_rand {
  const float* t_rand; /* (B,N_c) in [0,1) or NULL */
  const float* u;      /* (B,N_f) in [0,1) or NULL */
  uint64_t seed;
  uint64_t offset;
  /* noise_std > 0: explicit standard normals for model_utils.noise_regularize, (B,N_c) and (B,N_c+N_f), or NULL ->
   * Philox (streams 2, 3) + Box-Muller */
  const float* noise_coarse;
  const float* noise_fine;
} nrf_rand;

/* One level of the NerfModel output dict (models.py:278-287). Any pointer may
 * be NULL to skip that output. */
typedef struct nrf_level_out {
  float* rgb;       /* (B,3) */
  float* depth;     /* (B,)  */
  float* med_depth; /* (B,)  */
  float* acc;       /* (B,)  */
  float* weights;   /* (B,S) */
  float* z_vals;    /* (B,S)  (extra: the sample depths of this level) */
  float* points;        /* (B,S,3) sample points before the warp (return_points, models.py:247-248: with or without the warp) */
  float* warped_points; /* (B,S,3) after SE3Field (models.py:266-267); needs the warp field */
  float* warp_jacobian; /* (B,S,3,3) jax.jacfwd(SE3Field.warp) per sample, row-major d x'_i / d x_j (warping.py:385-387,
                           models.py:264-265); needs NRF_FLAG_WARP_JACOBIAN in flags and in nrf_workspace_bytes */
} nrf_level_out;

typedef struct nrf_outputs {
  nrf_level_out coarse;
  nrf_level_out fine;
} nrf_outputs;

/* flags for nrf_forward / nrf_workspace_bytes */
#define NRF_FLAG_TRAIN 1u   /* keep the activation stash nrf_backward needs */
#define NRF_FLAG_NO_WARP 2u /* NerfModel.__call__(use_warp=False) (models.py:296) */
#define NRF_FLAG_BF16 4u    /* NeRF-MLP operands in bfloat16 (fp32 accumulate, fp32 master weights / posenc / warp / composite /
                               loss / Adam); an opt-in mode with no reference counterpart (BASELINE config D) -- ~1e-2 on
                               rendered colour */
#define NRF_FLAG_WARP_JACOBIAN 8u /* return_warp_jacobian (models.py:297): forward-mode tangent pass of the warp per level */
#define NRF_FLAG_WARP_F32 16u     /* with NRF_FLAG_BF16 (or NRF_FLAG_BF16X3): keep SE3Field's 6 x 128 trunk on float32 operands (since 0.4.0 NRF_FLAG_BF16
                                     runs it on bfloat16 operands as well: annealed posenc, exp_se3, (w, v), the Jacobian algebra and
                                     the GLO table stay float32); a call that returns the warp Jacobian uses the float32 trunk anyway */
#define NRF_FLAG_BF16X3 32u       /* since 0.6.0, nrf_forward / nrf_workspace_bytes[_ex] only (inference): the NeRF MLPs
                                     (modules.py:26-62, 95-169) and SE3Field's trunk (warping.py:264-288) in split-bfloat16 arithmetic --
                                     every float32 operand as a bf16 pair hi + lo, a product as hi.hi + hi.lo + lo.hi on the bf16 matrix
                                     pipe, float32 accumulate: float32-EMULATING (an operand carries 16 mantissa bits; rendered colour
                                     within ~1e-6 of the float32 chains without the warp, ~1e-5 with it -- a warped point moves by ~1e-5
                                     and meets the 2^(F-1) posenc band --, far inside the 1e-3 parity gate), not bit-comparable with them.
                                     Posenc, exp_se3, sampling and compositing stay float32.  NRF_FLAG_WARP_F32 keeps the SE3 trunk on
                                     the float32 kernels (bit-identical warped points; a call that returns the warp Jacobian uses them
                                     anyway).  Not with NRF_FLAG_TRAIN or NRF_FLAG_BF16; same model limits as NRF_FLAG_BF16 */

#define NRF_FLAG_RAY_GRADS 64u     /* since 0.6.3, with NRF_FLAG_TRAIN on nrf_forward / nrf_workspace_bytes[_ex]: keep what nrf_backward_rays needs
                                     to differentiate the stashed call w.r.t. the rays -- a d-points buffer and the transposed layer-0 / skip-row
                                     weight images for a model without a warp field (it then runs the 64-row reverse chain), the warp Jacobian
                                     of every sample ([rows][9] per level, one forward-mode tangent pass per level behind the primal pass) for
                                     a model with one.  Float32 mode only: refused (NRF_E_UNSUPPORTED) without NRF_FLAG_TRAIN, with NRF_FLAG_BF16 /
                                     NRF_FLAG_BF16X3 and by the fused nrf_train_step_loss_grad[_ex].  NRF_OPT_CHAIN_TILE_ROWS = 32 is NOT refused:
                                     under the flag it is followed by the forward chain only, as on a model with a warp field (the 32-row
                                     reverse chain has no d-points section, so the reverse pass runs on 64-row tiles over the same stash) */

#define NRF_FLAG_FROZEN 128u       /* since 0.6.6, only as NRF_FLAG_TRAIN | NRF_FLAG_RAY_GRADS | NRF_FLAG_FROZEN (float32 mode) on nrf_forward /
                                     nrf_workspace_bytes[_ex]: the field's parameters are constants of this call, its stash serves
                                     nrf_backward_rays ONLY.  The plan keeps what the forward itself uses, the rendered outputs, the ReLU
                                     sign words and the posenc stash of the NeRF chains, d raw / d points / the per-ray sums, the transposed
                                     weight images of the d-points section, and -- with a warp field -- the primal trunk input, sign words
                                     and (w, v) rows, the tangent (dw, dv) rows and the warp Jacobians.  It holds NO activation stash, dY
                                     image, SE3 reverse stash, wgrad slab / group / segment, reduce table or padded gradient image, and the
                                     chains store none of them.  Any other word that carries the flag -- without NRF_FLAG_TRAIN or
                                     NRF_FLAG_RAY_GRADS, with NRF_FLAG_BF16 / NRF_FLAG_BF16X3 / NRF_FLAG_WARP_JACOBIAN -- and nrf_workspace_bytes_ex
                                     with background points or the elastic switch: NRF_E_UNSUPPORTED.  On a frozen stash nrf_backward /
                                     nrf_backward_ex return NRF_E_STATE; nrf_backward_rays takes grad_params == NULL (see there).
                                     NRF_OPT_CHAIN_TILE_ROWS is followed by the forward chain only, as under NRF_FLAG_RAY_GRADS */

int nrf_version(void);
const char* nrf_last_error(void);

/* models.construct_nerf (models.py:378-489) minus parameter init: validates the
 * configuration and fixes the parameter layout. */
int nrf_create(const nrf_model_desc* desc, nrf_handle* out);
int nrf_destroy(nrf_handle h);

int nrf_param_count(nrf_handle h, int64_t* n_floats);
/* out may be NULL to query *n only. */
int nrf_param_layout(nrf_handle h, nrf_tensor_info* out, int32_t* n);

int nrf_workspace_bytes(nrf_handle h, int32_t num_rays, uint32_t flags, size_t* bytes);

/* NerfModel.apply (models.py:289-375): sampling, [warp,] posenc, NeRF MLPs,
 * compositing, hierarchical resampling, fine pass. */
int nrf_forward(nrf_handle h, const float* params, const nrf_rays* rays,
                const nrf_step_scalars* scalars, const nrf_rand* rnd,
                const nrf_outputs* out, uint32_t flags, void* workspace,
                size_t workspace_bytes, void* stream);

/* Reverse pass of the nrf_forward(NRF_FLAG_TRAIN) call that last used this
 * workspace: the VJP jax.value_and_grad builds at training.py:264-265.
 * d_rgb_coarse / d_rgb_fine are dL/d(out[level]['rgb']) (B,3); either may be
 * NULL.  grad_params (flat, same layout as params) is OVERWRITTEN. */
int nrf_backward(nrf_handle h, const float* params, const nrf_rays* rays,
                 const float* d_rgb_coarse, const float* d_rgb_fine,
                 float* grad_params, void* workspace, size_t workspace_bytes,
                 void* stream);

/* The cotangents of one level of the NerfModel output dict (models.py:278-287), the counterpart of nrf_level_out.  Any pointer
 * may be NULL, which means zero. */
typedef struct nrf_level_grads {
  const float* d_rgb;           /* (B,3) */
  const float* d_depth;         /* (B,)   depth = sum_i w_i z_i; the sample depths carry no gradient (the coarse ones do not
                                   depend on the parameters, the fine ones sit behind stop_gradient, model_utils.py:187) */
  const float* d_acc;           /* (B,)   acc = sum_i w_i, without the last sample under use_sample_at_infinity (model_utils.py:125-126) */
  const float* d_weights;       /* (B,S) */
  const float* d_warped_points; /* (B,S,3) needs a stashed forward that ran the warp field (NRF_E_STATE otherwise) */
} nrf_level_grads;

typedef struct nrf_output_grads {
  nrf_level_grads coarse;
  nrf_level_grads fine;
} nrf_output_grads;

/* Since 0.6.2: nrf_backward with a cotangent for every differentiable output of the stashed nrf_forward(NRF_FLAG_TRAIN) -- the
 * VJP of NerfModel.apply proper (depth supervision, a mask term on acc, distortion / entropy terms on weights, a regulariser on
 * the warped points).  Same state checks as nrf_backward (stashed workspace, ray count, plan); float32 and NRF_FLAG_BF16
 * training stashes alike; no allocation, no synchronisation; grad_params is OVERWRITTEN.  All pointers NULL: a zero gradient.
 * med_depth is piecewise constant in the parameters: it has no cotangent.  Out of scope: a cotangent of warp_jacobian (its
 * adjoint exists only inside the elastic regulariser of nrf_train_step_loss_grad_ex), and extra cotangents through the fused
 * nrf_train_step_loss_grad[_ex], whose loss is fixed.  nrf_backward(.., c, f, ..) == nrf_backward_ex with only d_rgb set. */
int nrf_backward_ex(nrf_handle h, const float* params, const nrf_rays* rays,
                    const nrf_output_grads* g, float* grad_params,
                    void* workspace, size_t workspace_bytes, void* stream);

/* Since 0.6.3: the gradients of the stashed call w.r.t. its rays, each (B,3); any pointer may be NULL, which skips that part. */
typedef struct nrf_ray_grads {
  float* d_origins;    /* sum over levels and samples of J_s^T g_s: g_s = dL/d(warped point s), J_s = the warp Jacobian (I without the field) */
  float* d_directions; /* sum z_s J_s^T g_s, plus the term of the compositing distances (z_{i+1} - z_i) |d| (model_utils.py:104-110).  The
                          sample depths are constants (the coarse ones do not depend on the ray, the fine ones sit behind stop_gradient) */
  float* d_viewdirs;   /* through the rgb condition's posenc(viewdirs); needs use_viewdirs and rays->viewdirs (the normalisation
                          viewdirs = d / |d| is the caller's: differentiate it there) */
} nrf_ray_grads;

/* nrf_backward_ex plus the ray stage: grad_params exactly as nrf_backward_ex writes it, and the three ray gradients (OVERWRITTEN).  The
 * stashed forward must have run with NRF_FLAG_TRAIN | NRF_FLAG_RAY_GRADS (NRF_E_STATE otherwise); ray_grads NULL -> NRF_E_NULL; d_viewdirs for
 * a model without viewdirs, or with rays->viewdirs NULL -> NRF_E_UNSUPPORTED: all decided before any launch.  One wave per ray, no atomics:
 * d_origins / d_directions of two calls on one stash agree bit for bit (d_viewdirs reads the per-ray sums the reverse chain accumulates).
 * A cotangent on warped_points reaches the rays through g_s; `points` carries none (rebuild o + z d from z_vals in the caller).
 *
 * Since 0.6.6, on a stash written under NRF_FLAG_FROZEN: grad_params must be NULL (a non-NULL pointer: NRF_E_STATE -- nothing of the
 * parameter gradient was kept).  The call then runs composite_bwd, ONE 64-row NeRF data-gradient launch that writes d points and the
 * per-ray sums and no dY image, the warped-point cotangent add and the ray stage -- no SE3 reverse chain (the warp Jacobians come from
 * the forward's tangent passes), no condition / GLO / time-encoder gradient, no wgrad, no reduce pass.  grad_params == NULL on a stash
 * that is not frozen stays NRF_E_NULL. */
int nrf_backward_rays(nrf_handle h, const float* params, const nrf_rays* rays, const nrf_output_grads* grads,
                      const nrf_ray_grads* ray_grads, float* grad_params, void* workspace, size_t workspace_bytes, void* stream);

/* training.train_step up to (excluding) pmean + Adam (training.py:168-265):
 * forward, loss = MSE_coarse + MSE_fine (training.py:172,261), backward.
 * target_rgb (B,3).  stats[NRF_NUM_STATS] (device): {mse_coarse, mse_fine, psnr_coarse,
 * psnr_fine, loss_total, 0...}.  grad_params is OVERWRITTEN. */
#define NRF_NUM_STATS 16
int nrf_train_step_loss_grad(nrf_handle h, const float* params, const nrf_rays* rays,
                             const float* target_rgb, const nrf_step_scalars* scalars,
                             const nrf_rand* rnd, float* grad_params, float* stats,
                             void* workspace, size_t workspace_bytes, void* stream);

/* Background-point regulariser of training.compute_background_loss (training.py:117-135, 248-259).  The
 * caller draws the warp id per point (random.choice over model.warp_ids) and adds the N(0, noise_std)
 * noise; the library warps the points with the shared SE3 field (create_warp_field(num_batch_dims=1),
 * models.py:165-184), evaluates  weight * mean(general_loss_with_squared_residual(|x'-x|^2, alpha, scale))
 * (utils.py:264-331) and ADDS its parameter gradient to grad_params. */
typedef struct nrf_background {
  int32_t num_points;
  const float* points;      /* (N,3) points: already noised when warp_ids is given, raw when the library draws */
  const int32_t* warp_ids;  /* (N,) or NULL: the library draws id = id_choices[floor(U * num_choices)] (random.choice over
                               model.warp_ids, training.py:121-123) and adds noise_std * N(0,1) to the points (:124-126) with
                               its Philox streams 4 and 5 of (nrf_rand.seed, offset) -- nothing left for the host to launch */
  float loss_weight;        /* scalar_params.background_loss_weight */
  float loss_alpha;         /* -2 (training.py:119) */
  float loss_scale;         /* 0.001 */
  const int32_t* id_choices;/* (num_choices,) model.warp_ids; used when warp_ids == NULL */
  int32_t num_choices;
  float noise_std;          /* scalar_params.background_noise_std; used when warp_ids == NULL */
} nrf_background;

/* Elastic regulariser of training.compute_elastic_loss (training.py:71-114, 177-197) on the COARSE samples
 * (models.py:345): J = jax.jacfwd(SE3Field.warp) per sample (warping.py:385-387), loss_type 'log_svals':
 * sum_k log(max(s_k(J), eps))^2 -> general_loss(alpha, scale) -> sum over samples with the stop-gradient
 * compositing weights (elastic_reduce_method 'weight'; 'median' instead keeps only the sample at
 * model_utils.compute_depth_index) -> mean over rays, times loss_weight.  The gradient
 * (reverse over the forward-mode Jacobian, incl. exp_se3's second derivatives) is added to grad_params. */
enum { NRF_ELASTIC_WEIGHT = 0, NRF_ELASTIC_MEDIAN = 1 };
/* elastic_loss_type (training.py:86-109): sq_residual = sum log(max(s,eps))^2 | sum (s-1)^2 | sum((J J^T - I)^2)/4 |
 * div(J)^2 | (det J - 1)^2 | log(max(det J, eps))^2.  'nr' (nearest rotation) is not built: the reference marks it as
 * producing NaNs (training.py:58). */
enum { NRF_ELASTIC_LOG_SVALS = 0, NRF_ELASTIC_SVALS = 1, NRF_ELASTIC_JTJ = 2, NRF_ELASTIC_DIV = 3, NRF_ELASTIC_DET = 4,
       NRF_ELASTIC_LOG_DET = 5 };
typedef struct nrf_elastic {
  float loss_weight;      /* scalar_params.elastic_loss_weight */
  int32_t reduce_method;  /* NRF_ELASTIC_WEIGHT / NRF_ELASTIC_MEDIAN */
  float eps;              /* 1e-6 */
  float loss_alpha;       /* -2 (training.py:112-113) */
  float loss_scale;       /* 0.03 */
  int32_t loss_type;      /* NRF_ELASTIC_LOG_SVALS ... */
} nrf_elastic;

/* use_warp_reg_loss (training.py:199-212), both levels: general_loss(|points - warped_points|^2 at the sample of
 * model_utils.compute_depth_index(stop_gradient(weights)), alpha, scale), mean over rays, times loss_weight. */
typedef struct nrf_warp_reg {
  float loss_weight;      /* scalar_params.warp_reg_loss_weight */
  float loss_alpha;       /* scalar_params.warp_reg_loss_alpha (-2) */
  float loss_scale;       /* scalar_params.warp_reg_loss_scale (0.001) */
} nrf_warp_reg;

/* nrf_train_step_loss_grad + the regularisers (bg, el, wr may each be NULL).  stats[5] = mean background loss
 * (unweighted, training.py:259), stats[6] = elastic loss (unweighted, training.py:195), stats[7] = mean elastic
 * residual (training.py:196), stats[8], stats[9] = warp_reg loss coarse / fine (training.py:210), stats[10], stats[11] =
 * mean warp_reg residual coarse / fine (:211), stats[12..14] = mean det / div / |curl| of the coarse warp Jacobian
 * (training.py:214-222, with el); stats[4] includes the weighted terms.  The workspace must come from
 * nrf_workspace_bytes_ex with the same num_background_points / use_elastic_loss.  flags: 0 or NRF_FLAG_BF16. */
int nrf_train_step_loss_grad_ex(nrf_handle h, const float* params, const nrf_rays* rays, const float* target_rgb,
                                const nrf_step_scalars* scalars, const nrf_rand* rnd, const nrf_background* bg,
                                const nrf_elastic* el, const nrf_warp_reg* wr, uint32_t flags, float* grad_params,
                                float* stats, void* workspace, size_t workspace_bytes, void* stream);
int nrf_workspace_bytes_ex(nrf_handle h, int32_t num_rays, uint32_t flags, int32_t num_background_points,
                           int32_t use_elastic_loss, size_t* bytes);

/* Since 0.6.5: nrf_train_step_loss_grad_ex (flags = 0) that also returns the gradients of the loss w.r.t. the rays -- what refining
 * cameras next to the field needs.  One call: the forward under NRF_FLAG_TRAIN | NRF_FLAG_RAY_GRADS, the fixed loss, the reverse
 * pass.  grad_params and stats exactly as nrf_train_step_loss_grad_ex writes them; ray_grads->d_origins / d_directions (B,3) are
 * OVERWRITTEN (either may be NULL, which skips it).  The workspace comes from nrf_workspace_bytes_ex(NRF_FLAG_TRAIN |
 * NRF_FLAG_RAY_GRADS, num_background_points, use_elastic_loss).  Float32 only: NRF_FLAG_BF16* in flags -> NRF_E_UNSUPPORTED;
 * ray_grads NULL -> NRF_E_NULL; both decided before any launch.  nrf_train_step_loss_grad_ex itself keeps refusing the flag.
 *
 * Photometric terms only: the ray gradients are those of MSE_coarse + MSE_fine.  The background, elastic and warp_reg terms
 * regularise the field; their dependence on the sample positions is treated as stop-gradient and they add nothing to the rays
 * (the ray stage runs before warp_reg adds into the warped points' gradient).
 *
 * rays->viewdirs == NULL on a use_viewdirs model (the condition then reads the directions, models.py:326-329): d_directions
 * includes the view-dependence term, i.e. what nrf_backward_rays would return as d_directions + d_viewdirs when called with
 * viewdirs = directions.  One wave owns a ray, so the order of that sum is fixed (no atomics).  d_viewdirs non-NULL in that case
 * stays NRF_E_UNSUPPORTED (as in nrf_backward_rays, which is unchanged).
 *
 * With the elastic regulariser the coarse tangent pass serves both the regulariser and the coarse warp Jacobian of the ray
 * stage; the fine level's Jacobian pass runs into a scratch level of its own. */
int nrf_train_step_loss_grad_rays(nrf_handle h, const float* params, const nrf_rays* rays, const float* target_rgb,
                                  const nrf_step_scalars* scalars, const nrf_rand* rnd, const nrf_background* bg,
                                  const nrf_elastic* el, const nrf_warp_reg* wr, uint32_t flags, const nrf_ray_grads* ray_grads,
                                  float* grad_params, float* stats, void* workspace, size_t workspace_bytes, void* stream);

/* Since 0.6.6: the fused FROZEN step -- the gradients of MSE_coarse + MSE_fine (training.py:172, 261) w.r.t. the rays with the field's
 * parameters fixed: what aligning a camera against a trained field needs (test-time pose alignment of a held-out frame).  One call:
 * nrf_forward under NRF_FLAG_TRAIN | NRF_FLAG_RAY_GRADS | NRF_FLAG_FROZEN, the fixed loss, then the reverse pass nrf_backward_rays runs on
 * a frozen stash.  ray_grads->d_origins / d_directions / d_viewdirs (B,3) are OVERWRITTEN (any may be NULL, which skips it; ray_grads NULL
 * -> NRF_E_NULL).  stats[NRF_NUM_STATS] (device, may be NULL): {mse_coarse, mse_fine, psnr_coarse, psnr_fine, loss_total, 0...} -- no
 * regulariser is applied (they act on the field and never reach the rays), their entries are 0.  rays->viewdirs == NULL on a
 * use_viewdirs model: the view term is folded into d_directions exactly as in nrf_train_step_loss_grad_rays (d_viewdirs then stays
 * NRF_E_UNSUPPORTED).  The workspace comes from nrf_workspace_bytes(NRF_FLAG_TRAIN | NRF_FLAG_RAY_GRADS | NRF_FLAG_FROZEN).  No
 * allocation, no synchronisation, every launch on `stream`: capturable into a hipGraph.  The ray gradients agree with those of
 * nrf_train_step_loss_grad_rays to the order of the float atomics behind dray and the rounding of d_rgb. */
int nrf_loss_grad_rays(nrf_handle h, const float* params, const nrf_rays* rays, const float* target_rgb,
                       const nrf_step_scalars* scalars, const nrf_rand* rnd, const nrf_ray_grads* ray_grads, float* stats,
                       void* workspace, size_t workspace_bytes, void* stream);

/* warping.SE3Field on arbitrary points with one warp id per point: model.create_warp_field(num_batch_dims=1)
 * .apply(points, metadata, warp_extra, False, False) (models.py:165-184, warping.py:355-389). */
int nrf_warp_points_workspace_bytes(nrf_handle h, int32_t num_points, size_t* bytes);
int nrf_warp_points(nrf_handle h, const float* params, const float* points, const int32_t* warp_ids, int32_t num_points,
                    const nrf_step_scalars* scalars, float* warped, void* workspace, size_t workspace_bytes, void* stream);

/* ---- Field queries: the NeRF field at arbitrary points (float32 mode) ----
 * render_samples up to the activations (models.py:230-277): condition inputs, SE3Field warp (unless NRF_FLAG_NO_WARP), posenc,
 * the NerfMLP of `level`, sigmoid(rgb), sigma_activation(raw) -- no noise term, no compositing.  What a flax user gets from
 * apply(method=...): a density grid for a mesh or a point cloud, the canonical volume next to a frame's, the SfM points of a
 * capture against the learnt density.  The entries keep a plan of their own: the handle's ray plan, its stash and the digests
 * of nrf_debug_plan_digest do not move -- unless a query (or nrf_warp_points) is handed the very workspace a ray plan's tables or
 * stash live in: it writes over them, so the handle forgets that upload and stash (the next nrf_forward uploads its tables again,
 * nrf_backward returns NRF_E_STATE until then).  Announced by NRF_HAS_FIELD_QUERY (NRF_VERSION is unchanged). */
#define NRF_HAS_FIELD_QUERY 1
#define NRF_QUERY_MAX_POINTS (1 << 24) /* points of one call; more is NRF_E_SHAPE (the caller loops over chunks) */
#define NRF_GRID_MAX_POINTS (1LL << 40) /* points of a whole nrf_grid (dims[0] * dims[1] * dims[2]); more is NRF_E_SHAPE */

/* Device outputs of a query, N = num_groups * points_per_group rows each; any may be NULL.  rgb == NULL is the density-only
 * query: a kernel of its own that stops behind the alpha head (same sigma bits as the full query). */
typedef struct nrf_field_out {
  float* sigma;         /* (N,)   activated density: what the renderer composites (out4.w) */
  float* rgb;           /* (N,3)  sigmoid(rgb logits) */
  float* warped_points; /* (N,3)  the canonical points the MLP saw; needs the warp field on, else NRF_E_UNSUPPORTED */
} nrf_field_out;

/* A regular grid: point n has i = n % dims[0], j = (n / dims[0]) % dims[1], k = n / (dims[0] * dims[1]) and coordinate
 * c = origin[c] + (float)idx_c * step[c] (one float32 product, then one float32 sum). */
typedef struct nrf_grid {
  float origin[3];
  float step[3];
  int32_t dims[3];
  int32_t reserved;
} nrf_grid;

/* Workspace of a query of num_groups x points_per_group points; one answer whatever the outputs asked for.  Needs no GPU.
 * flags: 0 or NRF_FLAG_NO_WARP, as the query itself. */
int nrf_query_workspace_bytes(nrf_handle h, int32_t num_groups, int32_t points_per_group, uint32_t flags, size_t* bytes);

/* The field at `points` (G,S,3), G = groups->num_rays groups of S = points_per_group points.  The points of group g share
 * row g of groups->viewdirs, *_ids and *_codes (codes replace ids as in nrf_forward); groups->origins / directions are ignored
 * and may be NULL.  viewdirs == NULL is NRF_E_UNSUPPORTED when out->rgb is asked for on a use_viewdirs model (a point has no
 * direction to fall back on).  level: 0 coarse MLP, 1 fine MLP.  flags: 0 or NRF_FLAG_NO_WARP (the points are then canonical
 * points); every other bit is refused.  A time-encoder model is refused with the warp on, as in nrf_warp_points.  Asynchronous
 * on `stream`, no allocation; the workspace may be reused by the next query once this one has run. */
int nrf_query_points(nrf_handle h, const float* params, const nrf_rays* groups, const float* points, int32_t points_per_group,
                     int32_t level, const nrf_step_scalars* scalars, uint32_t flags, const nrf_field_out* out, void* workspace,
                     size_t workspace_bytes, void* stream);

/* The same at points [first, first + count) of `grid`, formed on the device (no host or framework work per point);
 * group->num_rays must be 1.  Workspace: nrf_query_workspace_bytes(h, 1, count, flags); a caller walks a large grid in chunks
 * through one workspace. */
int nrf_query_grid(nrf_handle h, const float* params, const nrf_rays* group, const nrf_grid* grid, int64_t first, int32_t count,
                   int32_t level, const nrf_step_scalars* scalars, uint32_t flags, const nrf_field_out* out, void* workspace,
                   size_t workspace_bytes, void* stream);

/* ---- Gradient queries: the density's slope at arbitrary points (float32 mode) ----
 * d sigma / d x of the field queried above, with respect to the CALLER's point -- through the warp field when it is on -- and the
 * surface normal it gives: what shading a density export, orienting an iso-surface or an Eikonal term needs, in one call where
 * central differences take six density queries.  Forward: the density chain keeping the posenc stash, the trunk's ReLU sign words
 * and sigma'(raw) (about 0.5 KB per row; about 1 KB with the warp field's stash and Jacobian).  Reverse: the data-gradient chain
 * started at the density -- no rgb branch, no per-group sum, no atomic: a row's result does not depend on the launch it ran in.
 * Warp on: the SE3 field's primal and forward-mode tangent passes give J = d x' / d x per row and grad_x = J^T grad_x'.
 * Entries of their own with a plan of their own: nrf_query_points / nrf_query_grid, nrf_field_out and what
 * nrf_query_workspace_bytes returns are as they were.  Announced by NRF_HAS_FIELD_GRADIENT (NRF_VERSION is unchanged). */
#define NRF_HAS_FIELD_GRADIENT 1
#define NRF_QUERY_GRAD_MAX_POINTS (1 << 20) /* points of one call (the stash is ~1 KB per row; callers chunk); more is NRF_E_SHAPE */

/* Device outputs of a gradient query, N rows each; any may be NULL. */
typedef struct nrf_field_grad_out {
  float* sigma;         /* (N,)   activated density: the same bits as nrf_query_points' density-only sigma */
  float* grad_sigma;    /* (N,3)  d sigma / d x at the caller's point (through the warp when it is on) */
  float* normals;       /* (N,3)  -g / |g| of g = grad_sigma, formed in float32 as
                         *          s = fmaf(g.z, g.z, fmaf(g.y, g.y, g.x * g.x)), inv = 1 / sqrtf(s), n_c = -(g_c * inv)
                         *        (one rounding per step, division and square root correctly rounded); exactly 0 where s is 0 or
                         *        not finite */
  float* warped_points; /* (N,3)  as nrf_field_out; needs the warp field on, else NRF_E_UNSUPPORTED */
} nrf_field_grad_out;

/* Workspace of a gradient query of num_groups x points_per_group points; one answer whatever the outputs asked for and for both
 * values of flags (0 or NRF_FLAG_NO_WARP).  Needs no GPU. */
int nrf_query_grad_workspace_bytes(nrf_handle h, int32_t num_groups, int32_t points_per_group, uint32_t flags, size_t* bytes);

/* nrf_query_points' arguments and rules (groups, level, flags: 0 or NRF_FLAG_NO_WARP and every other bit refused by its name, the
 * time encoder refused with the warp on, warped_points refused without it), at most NRF_QUERY_GRAD_MAX_POINTS points.  Density
 * only: no view direction or camera code is read; a use_alpha_condition model needs its appearance ids (or codes).  Every refusal
 * is decided before any HIP call.  Asynchronous on `stream`, no allocation, capturable into a hipGraph; handed the workspace of a
 * ray plan it makes the handle forget that plan's upload and stash, as the queries above. */
int nrf_query_points_grad(nrf_handle h, const float* params, const nrf_rays* groups, const float* points, int32_t points_per_group,
                          int32_t level, const nrf_step_scalars* scalars, uint32_t flags, const nrf_field_grad_out* out, void* workspace,
                          size_t workspace_bytes, void* stream);

/* The same at points [first, first + count) of `grid` (nrf_query_grid's rules; group->num_rays must be 1).  Workspace:
 * nrf_query_grad_workspace_bytes(h, 1, count, flags). */
int nrf_query_grid_grad(nrf_handle h, const float* params, const nrf_rays* group, const nrf_grid* grid, int64_t first, int32_t count,
                        int32_t level, const nrf_step_scalars* scalars, uint32_t flags, const nrf_field_grad_out* out, void* workspace,
                        size_t workspace_bytes, void* stream);

/* ---- The warp field inverted: canonical points into a frame (float32 mode) ----
 * x with W(x; id) = y for canonical targets y: what carries one template surface (a canonical mesh, tracked points) into every
 * frame with its topology and vertex identity intact.  The field has no closed-form inverse; this is Newton's iteration around
 * the launches of a gradient query's warp part, on the device, with no host round trip.  Announced by NRF_HAS_UNWARP (NRF_VERSION
 * is unchanged).
 *
 * The algorithm.  x starts at `guess` (NULL: at the target).  Each of num_steps rounds runs the SE3 trunk's primal pass at the
 * current x keeping its stash (explicit points, one id per point), its forward-mode tangent pass, and one kernel with one thread
 * per row:
 *   r = W(x) - y, res = |r|_2 (float32);
 *   a row that has stopped does nothing;
 *   res <= tolerance: the row stops as converged;
 *   else E = J - I from (w, v), their tangents and x (the Dual evaluation of exp_se3 the warp Jacobian output uses), and
 *     (I + E) dx = r solved in closed form (adjugate over determinant, float32); the Jacobian never goes to memory;
 *   the determinant 0 or not finite, a component of dx not finite, or x - dx not finite: the row stops (status 2) at its current x;
 *   else dx is shortened to length max_step if it is longer, and x -= dx.
 * After the last round one more primal pass -- the same kernel as the rounds', so the bits agree -- gives `residual` and decides
 * status 0 or 1 at the returned x.  num_steps == 0 returns the guess (or the target) with its residual.  Stopped rows still ride
 * through the trunk in later rounds: no compaction, a fixed launch sequence whatever the data.  A row's result depends only on its
 * own target, id (or code row), guess and the scalars -- not on its position or on the other rows.  Where the field folds (a
 * singular value of J near 0) the iteration may land on another preimage or run out of steps: the status and the residual say so.
 *
 * warp_codes == NULL: warp_ids index the model's embedding table.  Else warp_codes is a DEVICE (num_codes, num_warp_features)
 * table and warp_ids index ITS rows: the field at interpolated, in-between-frame codes.
 *
 * Refused before any HIP call, nrf_last_error naming the entry and the rule: a NULL handle, params, targets, warp_ids, scalars, out
 * or workspace (NRF_E_NULL); a model without a warp field, the time encoder (NRF_E_UNSUPPORTED, as nrf_warp_points); num_points
 * outside 1..NRF_UNWARP_MAX_POINTS, num_steps outside 0..NRF_UNWARP_MAX_STEPS, tolerance negative or NaN, max_step not positive
 * (INFINITY: no limit), num_codes <= 0 with warp_codes (NRF_E_SHAPE); a short workspace (NRF_E_WORKSPACE).  Asynchronous on
 * `stream`, no allocation, no synchronisation, capturable into a hipGraph; a plan of its own (the other plans and the digests of
 * nrf_debug_plan_digest do not move); handed the workspace of a ray plan it makes the handle forget that plan's upload and stash,
 * as the queries above. */
#define NRF_HAS_UNWARP 1
#define NRF_UNWARP_MAX_POINTS (1 << 20) /* points of one call (the stash is ~0.5 KB per row; callers chunk); more is NRF_E_SHAPE */
#define NRF_UNWARP_MAX_STEPS 32

/* Device outputs, N = num_points rows each; any may be NULL. */
typedef struct nrf_unwarp_out {
  float* points;    /* (N,3) x with W(x; id) ~= target */
  float* residual;  /* (N,)  |W(x) - target|_2 at the RETURNED x, float32 */
  int32_t* status;  /* (N,)  0 ran out of steps, 1 converged (residual <= tolerance), 2 stopped: singular or non-finite step */
} nrf_unwarp_out;

/* Workspace of a call of num_points points.  Needs no GPU. */
int nrf_unwarp_workspace_bytes(nrf_handle h, int32_t num_points, size_t* bytes);
/* targets (N,3), warp_ids (N,), guess (N,3) or NULL: device arrays. */
int nrf_unwarp_points(nrf_handle h, const float* params, const float* targets, const int32_t* warp_ids, const float* warp_codes,
                      int32_t num_codes, const float* guess, int32_t num_points, const nrf_step_scalars* scalars, int32_t num_steps,
                      float tolerance, float max_step, const nrf_unwarp_out* out, void* workspace, size_t workspace_bytes, void* stream);

/* ---- Mesh extraction: a triangle mesh of the level set sigma = threshold of a device density grid (surface nets) ----
 * Handle-free, like the camera tables: the grid may come from nrf_query_grid or from anywhere.  An indexed mesh with shared
 * vertices, the same bits on every run (no atomic, no claimed slot: every output position is a rank in the order below).
 * Announced by NRF_HAS_MESH (NRF_VERSION is unchanged).
 *
 * sigma: float32 DEVICE array laid out as `grid` lays it out: sample n has i = n % X, j = (n / X) % Y, k = n / (X Y)
 * (X, Y, Z = grid->dims) and sits at origin + idx * step.
 * Inside: a sample is inside iff sigma > threshold (strict: a NaN sample is outside).
 * Cells: cell (i, j, k), 0 <= i < X-1 (likewise j, k), has the corners (i+di, j+dj, k+dk), corner bit b = di + 2 dj + 4 dk; it is
 *   ACTIVE iff its 8 corners are neither all inside nor all outside.  Its linear index is i + (X-1) (j + (Y-1) k).
 * Vertices: one per active cell; the vertex index is the cell's rank among the active cells in linear order.
 * Position, in float32, one rounding per operation, nothing contracted:
 *   walk the 12 cell edges in the order corner a ascending, axis ascending; an edge runs from a to b = a | (1 << axis); take it where
 *   bit `axis` of a is 0 and the two ends differ in insideness.  t = (threshold - s_a) / (s_b - s_a), 0.5 if that is not finite,
 *   else clamped to [0, 1].  The crossing in cell-local coordinates is corner a's offset (di, dj, dk) with t added on `axis`.
 *   local = (the sum of the crossings, added in that order, per axis) / (float)(their count), and
 *   vertex_c = ((float)idx_c + local_c) * step_c + origin_c: one sum, one product, one sum.
 * Faces: for a cell c and an axis ax in the order x, y, z, with u = (ax+1) % 3 and v = (ax+2) % 3: if c[u] >= 1, c[v] >= 1 and the
 *   samples at c and at c + e_ax differ in insideness, the quad of the vertices of the cells c - e_u - e_v, c - e_v, c, c - e_u, in
 *   that order, reversed when the sample at c is outside, split as (q0, q1, q2), (q0, q2, q3).  Faces are ordered by the owner cell's
 *   linear index, then by axis.  Normals (counter-clockwise faces) point from high density to low; a surface that leaves the grid's
 *   box stays open there.  An all-outside (or all-inside) grid is no error: 0 vertices, 0 triangles.
 *
 * Every refusal is decided before any HIP call and names the entry and the rule in nrf_last_error: a NULL pointer (NRF_E_NULL), a
 * dimension below 2, more than NRF_MESH_MAX_CELLS cells, a non-finite threshold, a negative capacity or count (NRF_E_SHAPE), a
 * workspace that is short (NRF_E_WORKSPACE) or not 16-byte aligned.  Asynchronous on `stream`, nothing allocated or synchronised. */
#define NRF_HAS_MESH 1
/* Cells of a grid, (X-1)(Y-1)(Z-1).  Sized by the largest index the entries form in int32: a cell owns at most 3 quads = 6
 * triangles, so triangle indices stay below 6 * 2^28 < 2^31 (and samples, X Y Z <= 8 cells, at or below 2^31 - 1 as well). */
#define NRF_MESH_MAX_CELLS (1 << 28)

/* The first 16 bytes of a mesh workspace after nrf_mesh_count / nrf_mesh_emit ran (DEVICE memory; the caller may copy them). */
typedef struct nrf_mesh_status {
  int32_t num_vertices;       /* what nrf_mesh_count found (also in its `counts`) */
  int32_t num_triangles;
  int32_t emitted_vertices;   /* what the last nrf_mesh_emit wrote: the two totals, or 0 and 0 when a capacity was short */
  int32_t emitted_triangles;
} nrf_mesh_status;

/* Bytes of workspace for a grid of these dims (about 5 bytes per cell: a corner mask and the cell-to-vertex map).  Needs no GPU. */
int nrf_mesh_workspace_bytes(const nrf_grid* grid, size_t* bytes);

/* Classifies the cells and scans the totals: counts[0] = vertices, counts[1] = triangles (two DEVICE int32).  The caller reads them
 * and allocates; the library allocates nothing.  The workspace then serves nrf_mesh_emit for the same sigma, grid and threshold. */
int nrf_mesh_count(const float* sigma, const nrf_grid* grid, float threshold, int32_t* counts, void* workspace, size_t workspace_bytes,
                   void* stream);

/* vertices (V,3) float32, vertex_cell (V,) int32 (each vertex's linear cell index), triangles (F,3) int32, from the workspace
 * nrf_mesh_count filled for the same sigma, grid and threshold.  The capacities (in vertices / triangles) are held against the
 * scanned totals ON THE DEVICE: when either is short, nothing at all is written to the three buffers and
 * nrf_mesh_status.emitted_* become 0; otherwise they become the totals.  No write ever lands at or past a capacity.  A buffer
 * may be NULL where its capacity is 0.  The cell-to-vertex map (int32 per cell, -1 if inactive) is left in the workspace. */
int nrf_mesh_emit(const float* sigma, const nrf_grid* grid, float threshold, int32_t max_vertices, int32_t max_triangles, float* vertices,
                  int32_t* vertex_cell, int32_t* triangles, void* workspace, size_t workspace_bytes, void* stream);

/* One Newton step of every vertex onto the level set, in place, from the field's own density sigma_at (V,) and gradient grad_at
 * (V,3) at the vertices (nrf_query_points_grad):
 *   s = fmaf(g.z, g.z, fmaf(g.y, g.y, g.x * g.x)),  q = (sigma - threshold) / s,  x_c = fmaf(-q, g_c, x_c),
 * then each coordinate is clamped to its own cell's box [origin_c + (float)i_c * step_c, origin_c + (float)(i_c + 1) * step_c]
 * (i = the cell of vertex_cell; a NaN coordinate lands on the lower end): the mesh keeps its topology and cannot fold across
 * cells.  The vertex is unchanged where s is 0 or not finite, or where sigma is not finite.  num_vertices == 0 is a no-op. */
int nrf_mesh_snap(float* vertices, const int32_t* vertex_cell, const float* sigma_at, const float* grad_at, const nrf_grid* grid,
                  float threshold, int32_t num_vertices, void* stream);

/* ---- Mesh clean-up: connected components of an indexed triangle mesh, their table, and the compaction to a submesh ----
 * Handle-free and for any mesh, whatever made it and in whatever vertex and triangle order: triangles (F,3) int32, vertices (V,3)
 * float32, DEVICE arrays.  Every output position is a rank, the same bits on every run.  Announced by NRF_HAS_MESH_COMPONENTS
 * (NRF_VERSION is unchanged).
 *
 * Components.  The graph has the vertices 0 .. V-1.  A triangle is VALID iff its three indices are all in [0, V).  A valid triangle
 *   (a, b, c) joins a-b and b-c; a repeated index is allowed.  An invalid triangle joins nothing and belongs to no component
 *   (triangle indices cannot be validated without a synchronisation and are not: the camera tables' rule for an index outside the
 *   table).  A vertex no valid triangle names is a component of its own.  Component ids are dense, 0 .. C-1, in increasing order of
 *   each component's smallest vertex index.
 * Table.  Per component: its vertices, its valid triangles (a triangle counts for the component of its FIRST index), and the box of
 *   its vertices.  The counts are integer adds; the box is integer min / max on the monotone key of a float32 with the bits u,
 *     key(u) = (u & 0x80000000) ? ~u : (u | 0x80000000)   compared as uint32,
 *   whose order is the floats' order with -0 below +0.  A NaN coordinate is skipped; a component whose coordinates are all NaN gets
 *   (+inf, -inf).  No float is ever summed atomically, so the table too has the same bits on every run.
 * Submesh.  keep (V,) uint8, nonzero = kept.  vertex_map[v] is v's rank among the kept vertices, or -1.  A triangle is kept iff it is
 *   valid and all three of its vertices are kept; kept triangles keep their relative order and are written with mapped indices.
 *   General: the mask may select components, the rows whose animate status is 1, a box, a density cut.
 *
 * Every refusal is decided before any HIP call and names the entry and the rule in nrf_last_error: a NULL pointer where one is
 * required (NRF_E_NULL), a negative count or capacity, a row width below 1 (NRF_E_SHAPE), a workspace that is short or not 16-byte
 * aligned (NRF_E_WORKSPACE).  A buffer may be NULL where its count or capacity is 0.  Capacities are held against the scanned totals
 * ON THE DEVICE: when one is short nothing at all is written and the status words say 0; no write ever lands at or past a capacity.
 * Zero vertices and / or zero triangles is no error (C = 0, or C = V).  Asynchronous on `stream`, nothing allocated or synchronised. */
#define NRF_HAS_MESH_COMPONENTS 1

/* The first 16 bytes of a components workspace (DEVICE memory; the caller may copy them). */
typedef struct nrf_mesh_components_status {
  int32_t num_components;     /* what nrf_mesh_components found (also in its `counts`) */
  int32_t table_components;   /* what the last nrf_mesh_component_table wrote: C rows, or 0 when max_components was short */
  int32_t error;              /* 0, or nonzero when a labelling loop ran into its hard cap (V steps; cannot happen for parent[v] <= v) */
  int32_t reserved;
} nrf_mesh_components_status;
/* The first 16 bytes of a submesh workspace are an nrf_mesh_status: the kept totals, and what the last nrf_mesh_submesh_emit wrote
 * (the totals, or 0 and 0 when a capacity was short).  The submesh kernels have no loop to cap. */

/* Bytes of workspace (about 4 bytes per vertex and a total per 1024 vertices).  Needs no GPU. */
int nrf_mesh_components_workspace_bytes(int32_t num_vertices, int32_t num_triangles, size_t* bytes);

/* vertex_component (V,) int32; counts: DEVICE int32[1] = C.  The workspace then serves nrf_mesh_component_table. */
int nrf_mesh_components(const int32_t* triangles, int32_t num_triangles, int32_t num_vertices, int32_t* vertex_component,
                        int32_t* counts, void* workspace, size_t workspace_bytes, void* stream);

/* comp_counts (C,2) int32 = [vertices, valid triangles] (a triangle counts for the component of its first index);
 * comp_bbox (C,6) float32 = min x y z, max x y z over the component's vertices, or NULL together with `vertices`.
 * max_components is held against C on the device.  A vertex_component entry outside [0, C) is counted nowhere. */
int nrf_mesh_component_table(const int32_t* triangles, int32_t num_triangles, const float* vertices, int32_t num_vertices,
                             const int32_t* vertex_component, int32_t max_components, int32_t* comp_counts, float* comp_bbox,
                             void* workspace, size_t workspace_bytes, void* stream);

/* Bytes of workspace (a total per 1024 vertices and per 1024 triangles).  Needs no GPU. */
int nrf_mesh_submesh_workspace_bytes(int32_t num_vertices, int32_t num_triangles, size_t* bytes);
/* counts: DEVICE int32[2] = kept vertices, kept triangles.  The workspace then serves nrf_mesh_submesh_emit for the same mesh and keep. */
int nrf_mesh_submesh_count(const uint8_t* keep, int32_t num_vertices, const int32_t* triangles, int32_t num_triangles, int32_t* counts,
                           void* workspace, size_t workspace_bytes, void* stream);
/* vertex_map (V,) int32 and triangles_out (kept triangles, 3) int32; both capacities are held against the kept totals. */
int nrf_mesh_submesh_emit(const uint8_t* keep, int32_t num_vertices, const int32_t* triangles, int32_t num_triangles,
                          int32_t max_vertices, int32_t max_triangles, int32_t* vertex_map, int32_t* triangles_out, void* workspace,
                          size_t workspace_bytes, void* stream);
/* dst[vertex_map[v]] = src[v] for every v with 0 <= vertex_map[v] < max_rows: rows of `width` 4-byte words, copied byte for byte. */
int nrf_mesh_gather_rows(const void* src, int32_t width, const int32_t* vertex_map, int32_t num_vertices, void* dst, int32_t max_rows,
                         void* stream);

/* ---- Mesh rasteriser: which triangle every pixel of a camera sees, its depth and barycentrics ----
 * Handle-free: screen (V,3) float32 rows (px, py, z) from anywhere (nrf_camera_table_project_depth, or an orthographic view formed
 * by the caller), triangles (F,3) int32, DEVICE arrays; one camera per call.  Integer coverage, one rounding per float operation in
 * the order written below, and an order-free 64-bit integer min per pixel: the image has the same bits on every run and for every
 * order of the triangles.  Announced by NRF_HAS_MESH_RASTER (NRF_VERSION is unchanged).
 *
 * Usable vertex.  z > near, |px| <= 1048576 and |py| <= 1048576; all three comparisons are false for NaN.  near must be >= 0 and
 *   finite (NRF_E_SHAPE otherwise).
 * Snap.  X = (int64) rintf(px * 256.0f), Y likewise: eight sub-pixel bits.  Pixel (i, j), column i, row j, has its centre at
 *   (Px, Py) = (256 i + 128, 256 j + 128).
 * Skipped triangle.  An index outside [0, V); a vertex that is not usable -- there is NO clipping: a triangle that crosses the near
 *   plane is dropped whole; the area A = (X1-X0)(Y2-Y0) - (Y1-Y0)(X2-X0) (int64; with the bound above every product is below 2^62)
 *   is 0; or its pixel box is empty.  The pixel box is the set of pixels whose centre lies in [min X, max X] x [min Y, max Y],
 *   clamped to the image: columns max(0, ceil((min X - 128) / 256)) .. min(W - 1, floor((max X - 128) / 256)), rows likewise.  Both
 *   orientations are drawn: there is no back-face culling.
 * Coverage.  s = sign(A).  For edge k from vertex a to vertex b, (a, b) = (1,2), (2,0), (0,1): dx = s (Xb - Xa), dy = s (Yb - Ya),
 *   E_k = dx (Py - Ya) - dy (Px - Xa), all int64.  The pixel is covered iff for every k: E_k > 0, or E_k == 0 and the edge is
 *   top-left, i.e. dy < 0, or dy == 0 and dx > 0.  A pixel centre on an edge two triangles share belongs to exactly one of them.
 * Depth and barycentrics, float32: l_k = (float) E_k / (float)(s A) (int64 -> float32 rounds to nearest; IEEE division),
 *   q_k = l_k / z_k, w = (q0 + q1) + q2, depth = 1.0f / w, b_k = q_k / w: perspective-correct.  With a distorted camera the edges are
 *   straight in DISTORTED pixel space: exact at the vertices, second order in the triangle's size between them.
 * Ownership.  The pixel goes to the covering triangle with the smallest key ((uint64) float_bits(depth) << 32) | face_index; depth is
 *   positive, so its bits order as the floats do, and equal depth bits go to the lower face index.  One integer atomic min per
 *   covered pixel: the result does not depend on the order of arrival.
 * Outputs.  face_id (H,W) int32, depth (H,W), bary (H,W,3) or NULL.  Where no triangle covers the pixel: -1, 0, (0, 0, 0); else depth
 *   and bary are recomputed for the owner by the device function the draw pass used.
 * Interpolate.  out[p, c] = (b0 * a0[c] + b1 * a1[c]) + b2 * a2[c] over the owner's corners in the triangle's order; the `background`
 *   row (NULL = zeros) where face_id[p] < 0 (or face_id[p] >= F, or a corner outside [0, V): nothing is read out of bounds).
 * Visibility.  visible[v] = 1 iff v is a corner of a face that owns at least one pixel, else 0; the entry clears the array first.
 *
 * Launches of nrf_mesh_raster_draw, grids fixed by F, W, H; nothing on the host reads a device value, so the call can be captured:
 *   clear (keys all ones, status 0); faces (a thread per triangle: one whose pixel box has at most 256 pixels is drawn by its
 *   thread, a larger one is ranked by ballot into its workgroup's part of a list); scan (the workgroups' totals, one workgroup);
 *   large (a fixed grid striding over the list by the device-side count, a workgroup of 256 per triangle, its threads striding over
 *   the pixel box); resolve (a thread per pixel).  Every loop is bounded by a clamped pixel box or by F; no thread waits on another.
 *   The image does not depend on the 256-pixel constant.
 *
 * Every refusal is decided before any HIP call and names the entry and the argument in nrf_last_error: a NULL pointer where one is
 * required (NRF_E_NULL; a buffer may be NULL where its count is 0); a negative count, a width or height below 1, width * height >
 * NRF_MESH_RASTER_MAX_PIXELS, a bad near, width_a < 1 (NRF_E_SHAPE); a workspace that is short or not 16-byte aligned
 * (NRF_E_WORKSPACE).  F == 0 is no error: an empty image.  Asynchronous on `stream`, nothing allocated or synchronised. */
#define NRF_HAS_MESH_RASTER 1
#define NRF_MESH_RASTER_MAX_PIXELS (1 << 26)

/* The first 16 bytes of a raster workspace (DEVICE memory; the caller may copy them) after nrf_mesh_raster_draw. */
typedef struct nrf_mesh_raster_status {
  int32_t drawn_triangles;     /* triangles that passed every skip rule above */
  int32_t large_triangles;     /* of those, the ones that took the workgroup-per-triangle path */
  int32_t covered_pixels;      /* pixels with face_id >= 0 */
  int32_t reserved;
} nrf_mesh_raster_status;

/* Bytes of workspace (8 per pixel, about 4 per triangle).  Needs no GPU. */
int nrf_mesh_raster_workspace_bytes(int32_t num_triangles, int32_t width, int32_t height, size_t* bytes);
int nrf_mesh_raster_draw(const float* screen, int32_t num_vertices, const int32_t* triangles, int32_t num_triangles, int32_t width,
                         int32_t height, float near, int32_t* face_id, float* depth, float* bary, void* workspace,
                         size_t workspace_bytes, void* stream);
/* attributes (V, width_a) float32 -> out (num_pixels, width_a); bary is required. */
int nrf_mesh_raster_interpolate(const int32_t* face_id, const float* bary, int64_t num_pixels, const int32_t* triangles,
                                int32_t num_triangles, const float* attributes, int32_t num_vertices, int32_t width_a,
                                const float* background, float* out, void* stream);
/* visible (V,) uint8. */
int nrf_mesh_raster_visibility(const int32_t* face_id, int64_t num_pixels, const int32_t* triangles, int32_t num_triangles,
                               int32_t num_vertices, uint8_t* visible, void* stream);

/* flax.optim.Adam.apply_gradient (training.py:268-269; flax 0.3.4 optim/adam.py):
 * g = grad*grad_scale (grad_scale = 1/world_size folds lax.pmean, training.py:266),
 * m,v updated in place, step = number of updates already applied.  Hyper-parameters are doubles
 * (flax keeps them as Python floats: 1-beta2 is formed in double, then rounded to fp32). */
int nrf_adam_step(float* params, float* m, float* v, const float* grad, int64_t n,
                  double lr, double beta1, double beta2, double eps, int64_t step,
                  double grad_scale, void* stream);
/* The same update with lr, the bias corrections and grad_scale read from DEVICE memory (nrf_dynamic_scalars): the launch
 * can sit in a captured graph and still follow the learning-rate schedule and the step count. */
int nrf_adam_step_dynamic(float* params, float* m, float* v, const float* grad, int64_t n, double beta1, double beta2,
                          double eps, const nrf_dynamic_scalars* dynamic, void* stream);

/* ---- measurement: per-kernel wall time from HIP events recorded on the launch stream ----
 * (the reference only has utils.TimeTracker host timers, utils.py:418-465, around an
 * asynchronously dispatched step; these are device-side).  Off by default; when on, entry points
 * are no longer hipGraph-capturable. */
typedef struct nrf_profile_entry {
  char name[32];           /* e.g. "mlp_fwd_fine", "wgrad" */
  double ms;               /* accumulated since the last read */
  int32_t launches;
  int32_t pad_;
  double flops_per_launch; /* ALGORITHMIC flops (2/MAC, dense layers, unpadded) */
} nrf_profile_entry;
int nrf_profile_enable(nrf_handle h, int32_t on);
/* Waits for the recorded events, returns and resets the accumulators.  out may be NULL to query *n. */
int nrf_profile_read(nrf_handle h, nrf_profile_entry* out, int32_t* n);

/* Calibration aid for the wgrad stream-K partition: for each segment of the last
 * nrf_backward / nrf_train_step_loss_grad on `workspace`, 6 doubles {workgroup, group, Kb, Nb,
 * tiles, wall-clock ticks (100 MHz)}.  Synchronous (hipMemcpy); out may be NULL to query *n. */
int nrf_debug_wgrad_segments(nrf_handle h, const void* workspace, double* out, int32_t* n);

/* Test aid: float offset inside the workspace of an internal buffer of `level` (0 coarse, 1 fine, 2 background
 * points, 3 Jacobian tangents) for the last planned (num_rays, flags): "st_pe", "st_h", "st_bn", "st_rgbh",
 * "dy_trunk", "dy_bn", "dy_rgbh", "d_raw4", "z", "out4", "wpoints", "d_points", "w_st_win", "w_st_h", "w_st_wv",
 * "w_dy", "w_dw4", "w_dv4", "bits_trunk", "bits_rgbh", "w_bits", "points_raw" (the unwarped sample points, [rows][3]),
 * "weights" (the per-sample compositing weights, [rows]), "el_dw4", "el_dv4" (level 0 under the elastic regulariser: its
 * gradient w.r.t. the primal SE3 head outputs, [rows] float4; the gradient w.r.t. the head tangents is "w_dw4" / "w_dv4" of
 * level 3, row c * padded_rows + r for d/dx_c); with nerf_rgb_branch_depth = D > 1 also "st_rgbx", "bits_rgbx",
 * "dy_rgbx": the rgb branch layers 1..D-1 as [D-1][tiles] images of the "st_rgbh" / "bits_rgbh" / "dy_rgbh" kind (those keep meaning layer 0).
 * Stash tiles are [features][64 rows] in fragment order (csrc/chain_common.h frag_index); the ReLU sign bits are one
 * uint32 per (tile, wave, lane, column block): nibble q, bit e <-> tile row 4 * ((q&1) + 2*(lane>>5) + 4*(q>>1)) + e of
 * feature wave * 32 * NCB + 32 * cb + (lane & 31)  (NCB = 2 for the 256-wide trunk, 1 otherwise). */
int nrf_debug_ws_offset(nrf_handle h, const char* name, int32_t level, int64_t* float_offset);

/* Test aid: 64-bit FNV-1a digest of the last planned workspace layout -- every sub-buffer offset, the descriptor tables
 * (pack, bf16 pack, wgrad groups and stream-K segments of both wgrad kernels, reduce) and their byte offsets, the tile
 * counts and the launch sizes the plan decides.  Equal digests = the same plan.  Runs without a GPU (nrf_workspace_bytes*
 * plans with the handle's default CU count then).  NRF_E_STATE before the handle's first plan. */
int nrf_debug_plan_digest(nrf_handle h, uint64_t* digest);

/* Tuning options of a handle (no reference counterpart: XLA picks its own tilings).  Must be set before the first
 * nrf_workspace_bytes / nrf_forward call that uses the handle with a given batch size, or between steps (the next call
 * re-plans; a stashed forward cannot be differentiated across a change: NRF_E_STATE).  Unknown option / value:
 * NRF_E_UNSUPPORTED.
 *   NRF_OPT_CHAIN_TILE_ROWS  rows per workgroup tile of the float32 NeRF-MLP chain kernels (modules.py:95-169):
 *                            64 = two workgroups per CU (csrc/mlp_chain.hip), 32 = four per CU (csrc/mlp_chain32.hip): one tile
 *                            body, csrc/nerf_chain.h, instantiated on two tile geometries,
 *                            0 = automatic (default: half tiles for forward launches that under-fill the 64-row grid).  The
 *                            forward results (and the stashes) are bit-identical under both tilings -- a ray's result does not
 *                            depend on the launch it rides in --, gradients agree to the order of float atomics; the workspace
 *                            layout does not depend on it.  A handle with nerf_rgb_branch_depth > 1 keeps the 64-row kernels at
 *                            every launch size (automatic never picks half tiles for it) and refuses the value 32. */
#define NRF_OPT_CHAIN_TILE_ROWS 1
/*   NRF_OPT_BF16_WGRAD_MERGE bf16 training mode: 1 (default) = the weight-gradient GEMMs of the skip layer (X = [h4 | posenc]) and of
 *                            the bottleneck + alpha head (dY = [d bottleneck | d raw]) run as ONE group each, so dpre_4 and h8 are
 *                            streamed once (HBM fetch of the kernel 1.16 x -> 1.03 x its algorithmic bytes; same-box A/B: the step
 *                            1-2 % faster, profiles/r05_wgrad_bf16_merge_ab.md); 0 = one group per weight matrix (rounds 2-4).  Same
 *                            results to float32 summation order; changes the workspace size (query nrf_workspace_bytes* after
 *                            setting it). */
#define NRF_OPT_BF16_WGRAD_MERGE 2
int nrf_set_option(nrf_handle h, int32_t option, int64_t value);

/* ---- individual operators (same device code the fused path runs), exposed so
 * parity tests can check each reference function in isolation. ---- */

/* model_utils.sample_along_rays (model_utils.py:36-73) -> z_vals (B,N). */
int nrf_sample_along_rays(const float* origins, const float* directions, int32_t num_rays,
                          int32_t num_samples, float near_plane, float far_plane,
                          int32_t stratified, int32_t linear_disparity,
                          const float* t_rand, uint64_t seed, uint64_t offset,
                          float* z_vals, void* stream);

/* model_utils.volumetric_rendering (+ compute_depth_map) (model_utils.py:76-136,
 * 218-263).  rgb_sigma is (B,S,4) = (r,g,b,sigma) post-activation. */
int nrf_volumetric_rendering(const float* rgb_sigma, const float* z_vals, const float* directions,
                             int32_t num_rays, int32_t num_samples, int32_t white_background,
                             int32_t sample_at_infinity, const nrf_level_out* out, void* stream);

/* model_utils.sample_pdf (model_utils.py:139-215) applied as models.py:353-357:
 * bins = midpoints of z_coarse, weights = weights_coarse[:,1:-1]; returns the
 * sorted union (B, N_c+N_f). */
int nrf_sample_pdf(const float* z_coarse, const float* weights_coarse, int32_t num_rays,
                   int32_t num_coarse, int32_t num_fine, int32_t stratified, const float* u,
                   uint64_t seed, uint64_t offset, float* z_out, void* stream);

/* ---- camera geometry (the eval / dataset side of the path) ----
 * nerfies/camera.py Camera: orientation is the world-to-camera rotation (row-major),
 * position the camera centre in world space; intrinsics as camera.py:110-140. */
typedef struct nrf_camera {
  float orientation[9];
  float position[3];
  float focal_length;
  float principal_point[2];
  float skew;
  float pixel_aspect_ratio;
  float radial_distortion[3];      /* k1 k2 k3 */
  float tangential_distortion[2];  /* p1 p2 */
  int32_t image_size[2];           /* width, height */
} nrf_camera;

/* Camera.pixels_to_rays (camera.py:244-269) incl. the fixed 10-iteration Newton
 * undistort (camera.py:26-105).  pixels: device [n,2] fp32, or NULL for the pixel
 * centres of the whole image in row-major [H,W] order (get_pixel_centers,
 * camera.py:317-321; then n must equal width*height) -- which makes this
 * datasets/core.py:50-75 camera_to_rays in one launch: directions [n,3], and,
 * when non-NULL, origins [n,3] (the tiled camera position) and pixels_out [n,2]. */
int nrf_camera_pixels_to_rays(const nrf_camera* camera, const float* pixels, int64_t n, float* origins,
                              float* directions, float* pixels_out, void* stream);

/* Camera.pixels_to_points (camera.py:271-277): points [n,3] at `depth` [n] measured
 * along the optical axis. */
int nrf_camera_pixels_to_points(const nrf_camera* camera, const float* pixels, const float* depth, int64_t n,
                                float* points, void* stream);

/* Camera.project (camera.py:283-315): world points [n,3] -> distorted pixel positions [n,2]. */
int nrf_camera_project(const nrf_camera* camera, const float* points, int64_t n, float* pixels, void* stream);

/* ---- camera tables: differentiable cameras (since 0.6.4) ----
 * A camera table is a DEVICE array (num_cameras, NRF_CAMERA_ROW) fp32, 16-byte aligned.  Row c holds the NRF_CAMERA_NPARAMS
 * differentiable fields of nrf_camera in its field order -- orientation[9], position[3], focal_length, principal_point[2], skew,
 * pixel_aspect_ratio, radial_distortion[3], tangential_distortion[2] -- and two pad floats, which are never read and always
 * receive gradient 0.  image_size is not part of a row: these entry points always take explicit pixels.
 *
 * camera_index (n,) int32 names each ray's row; NULL = every ray uses row 0.  The table lives on the device, so its VALUES (and the
 * indices) cannot be validated without a synchronisation and are not: a row with focal_length or pixel_aspect_ratio 0 gives inf / nan
 * as the arithmetic does.  The kernels never read or write outside the table: a ray whose index lies outside [0, num_cameras) gets
 * zero outputs, zero d_pixels / d_points, and contributes no gradient.
 *
 * As everywhere: device pointers plus sizes, nothing allocated or synchronised, every launch on `stream` (graph-capturable); the
 * arguments are validated on the host before any HIP call (NRF_E_NULL / NRF_E_SHAPE / NRF_E_WORKSPACE).  n == 0 is a successful
 * no-op, except that the reverse passes still zero d_cameras; the per-ray buffers of an empty batch may be NULL.  n <= INT32_MAX.  pixels / d_pixels are 8-byte aligned, the
 * workspace 16-byte aligned.
 *
 * Forward, per ray exactly Camera.pixels_to_rays / Camera.project of its row; "distorted" (whether the Newton undistort runs) is
 * decided per row on the device as on the host: any of the five coefficients non-zero. */
#define NRF_CAMERA_ROW 24
#define NRF_CAMERA_NPARAMS 22

/* pixels (n,2) -> directions (n,3) and, when non-NULL, origins (n,3) = the row's position. */
int nrf_camera_table_rays(const float* cameras, int32_t num_cameras, const int32_t* camera_index, const float* pixels, int64_t n,
                          float* origins, float* directions, void* stream);

/* points (n,3) -> pixels (n,2). */
int nrf_camera_table_project(const float* cameras, int32_t num_cameras, const int32_t* camera_index, const float* points, int64_t n,
                             float* pixels, void* stream);

/* points (n,3) -> screen (n,3) = (px, py, z): (px, py) are the bits nrf_camera_table_project writes for the same inputs, z is the
 * point's coordinate along the row's optical axis, orientation[6..8] . (point - position), the number the projection divides by.
 * Validation, the camera_index rule (an index outside the table gives a row of zeros) and n == 0 are those of the entries above.
 * There is NO reverse pass: the entry feeds nrf_mesh_raster_draw, which is not differentiable either. */
int nrf_camera_table_project_depth(const float* cameras, int32_t num_cameras, const int32_t* camera_index, const float* points, int64_t n,
                                   float* screen, void* stream);

/* Bytes of workspace the two reverse passes below need for n rays (num_cameras is validated; today the size depends on n alone). */
int nrf_camera_table_workspace_bytes(int64_t n, int32_t num_cameras, size_t* bytes);

/* Reverse pass of nrf_camera_table_rays: d_origins, d_directions (n,3), either may be NULL (= zeros) -> d_cameras
 * (num_cameras, NRF_CAMERA_ROW), OVERWRITTEN (rows without a ray and the pads become 0), and, when non-NULL, d_pixels (n,2).
 * The undistort is differentiated by the implicit-function theorem at the forward's result, the second normalisation
 * w / |w| is differentiated too (orientation is nine free parameters), and the distortion coefficients of a row whose coefficients
 * are all zero receive the same formula's gradient (J = I there): a lens correction can be learned from zero.  DESIGN.md section 1.
 * The sums over rays use no atomics: two calls on the same inputs give the same bits.  The workspace needs no clearing. */
int nrf_camera_table_rays_backward(const float* cameras, int32_t num_cameras, const int32_t* camera_index, const float* pixels,
                                   int64_t n, const float* d_origins, const float* d_directions, float* d_cameras, float* d_pixels,
                                   void* workspace, size_t workspace_bytes, void* stream);

/* Reverse pass of nrf_camera_table_project: d_pixels (n,2) -> d_cameras as above and, when non-NULL, d_points (n,3). */
int nrf_camera_table_project_backward(const float* cameras, int32_t num_cameras, const int32_t* camera_index, const float* points,
                                      int64_t n, const float* d_pixels, float* d_cameras, float* d_points, void* workspace,
                                      size_t workspace_bytes, void* stream);

/* ---- camera delta tables: refining a camera table (since 0.6.5) ----
 * A delta table is a DEVICE array (num_cameras, NRF_CAMERA_DELTA_ROW) fp32, 16-byte aligned.  Row c changes row c of a base table:
 *   [0:3]   omega            R = exp(hat omega) R0.  orientation is world-to-camera, so this turns the camera in its own frame
 *   [3:6]   t                position = p0 + t
 *   [6]     s                focal_length = f0 exp(s)
 *   [7:9]   principal point  added
 *   [9:12]  radial           added
 *   [12:14] tangential       added
 *   [14:16] pads             never read; their gradient is 0
 * skew and pixel_aspect_ratio are copied through, the output row's pads are 0.  The rotation uses the closed forms and the
 * theta^2 series of the SE3 field (exact value and gradient at omega = 0, where every refinement starts).  One thread per camera;
 * validation, streams and graph capture as for the camera tables above.  `out` may not alias `cameras`. */
#define NRF_CAMERA_DELTA_ROW 16
int nrf_camera_table_compose(const float* cameras, const float* deltas, int32_t num_cameras, float* out, void* stream);
/* d_cameras (num_cameras, NRF_CAMERA_ROW) -> d_deltas (num_cameras, NRF_CAMERA_DELTA_ROW), OVERWRITTEN. */
int nrf_camera_table_compose_backward(const float* cameras, const float* deltas, int32_t num_cameras, const float* d_cameras,
                                      float* d_deltas, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NERFIES_AMD_H_ */
