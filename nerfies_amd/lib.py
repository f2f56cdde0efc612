"""ctypes binding of include/nerfies_amd.h.  Fails loudly when the HIP extension is absent:
there is no CPU or PyTorch fallback for the hot path."""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, '_lib', 'libnerfies_amd.so')

NRF_FLAG_TRAIN = 1
NRF_FLAG_NO_WARP = 2
NRF_FLAG_BF16 = 4
NRF_FLAG_WARP_JACOBIAN = 8
NRF_FLAG_WARP_F32 = 16
NRF_FLAG_BF16X3 = 32
NRF_FLAG_RAY_GRADS = 64
NRF_FLAG_FROZEN = 128      # with TRAIN | RAY_GRADS: the stash serves nrf_backward_rays only (no parameter gradient)
NRF_VERSION = 660          # of include/nerfies_amd.h; tests hold it against the header and the library
NRF_NUM_STATS = 16
NRF_CAMERA_ROW = 24       # floats per row of a camera table
NRF_CAMERA_NPARAMS = 22   # of which differentiable parameters (the rest: pads)
NRF_CAMERA_DELTA_ROW = 16 # floats per row of a camera delta table (nrf_camera_table_compose)
ACT = {'relu': 0, 'softplus': 1}
WARP_FIELD = {'se3': 0, 'translation': 1}
META_ENCODER = {'glo': 0, 'time': 1}
ELASTIC_REDUCE = {'weight': 0, 'median': 1}
ELASTIC_TYPE = {'log_svals': 0, 'svals': 1, 'jtj': 2, 'div': 3, 'det': 4, 'log_det': 5}


class NrfError(RuntimeError):
  pass


class ModelDesc(C.Structure):
  _fields_ = [
      ('num_coarse_samples', C.c_int32), ('num_fine_samples', C.c_int32), ('use_viewdirs', C.c_int32),
      ('near_plane', C.c_float), ('far_plane', C.c_float),
      ('nerf_trunk_depth', C.c_int32), ('nerf_trunk_width', C.c_int32),
      ('nerf_rgb_branch_depth', C.c_int32), ('nerf_rgb_branch_width', C.c_int32), ('nerf_skip_layer', C.c_int32),
      ('use_stratified_sampling', C.c_int32), ('num_nerf_point_freqs', C.c_int32),
      ('num_nerf_viewdir_freqs', C.c_int32), ('sigma_activation', C.c_int32),
      ('use_white_background', C.c_int32), ('use_linear_disparity', C.c_int32), ('use_sample_at_infinity', C.c_int32),
      ('use_appearance_metadata', C.c_int32), ('num_appearance_embeddings', C.c_int32),
      ('num_appearance_features', C.c_int32), ('use_camera_metadata', C.c_int32),
      ('num_camera_embeddings', C.c_int32), ('num_camera_features', C.c_int32),
      ('use_alpha_condition', C.c_int32), ('use_rgb_condition', C.c_int32), ('use_trunk_condition', C.c_int32),
      ('use_warp', C.c_int32), ('num_warp_freqs', C.c_int32), ('num_warp_embeddings', C.c_int32),
      ('num_warp_features', C.c_int32), ('warp_field_type', C.c_int32),
      ('noise_std', C.c_float), ('warp_metadata_encoder_type', C.c_int32), ('num_time_encoder_freqs', C.c_int32),
      ('warp_trunk_depth', C.c_int32), ('warp_trunk_width', C.c_int32),
  ]


class TensorInfo(C.Structure):
  _fields_ = [('name', C.c_char * 96), ('offset', C.c_int64), ('rows', C.c_int32), ('cols', C.c_int32)]


class Rays(C.Structure):
  _fields_ = [('num_rays', C.c_int32), ('origins', C.c_void_p), ('directions', C.c_void_p), ('viewdirs', C.c_void_p),
              ('warp_ids', C.c_void_p), ('appearance_ids', C.c_void_p), ('camera_ids', C.c_void_p),
              ('warp_codes', C.c_void_p), ('appearance_codes', C.c_void_p), ('camera_codes', C.c_void_p),
              ('time', C.c_void_p)]


class DynamicScalars(C.Structure):
  """nrf_dynamic_scalars: the per-step scalars in DEVICE memory (64 bytes) of a graph-replayed train step."""
  _fields_ = [('warp_alpha', C.c_float), ('time_alpha', C.c_float), ('elastic_loss_weight', C.c_float), ('learning_rate', C.c_float),
              ('adam_c1', C.c_float), ('adam_c2', C.c_float), ('grad_scale', C.c_float), ('reserved0', C.c_float),
              ('rng_seed', C.c_uint64), ('rng_offset', C.c_uint64), ('reserved1', C.c_uint64 * 2)]


class StepScalars(C.Structure):
  _fields_ = [('warp_alpha', C.c_float), ('time_alpha', C.c_float), ('dynamic', C.c_void_p)]


class Rand(C.Structure):
  _fields_ = [('t_rand', C.c_void_p), ('u', C.c_void_p), ('seed', C.c_uint64), ('offset', C.c_uint64),
              ('noise_coarse', C.c_void_p), ('noise_fine', C.c_void_p)]


class LevelOut(C.Structure):
  _fields_ = [('rgb', C.c_void_p), ('depth', C.c_void_p), ('med_depth', C.c_void_p), ('acc', C.c_void_p),
              ('weights', C.c_void_p), ('z_vals', C.c_void_p), ('points', C.c_void_p), ('warped_points', C.c_void_p),
              ('warp_jacobian', C.c_void_p)]


class Outputs(C.Structure):
  _fields_ = [('coarse', LevelOut), ('fine', LevelOut)]


class LevelGrads(C.Structure):
  """nrf_level_grads: the cotangents of one level's outputs (nrf_backward_ex); a NULL pointer means zero."""
  _fields_ = [('d_rgb', C.c_void_p), ('d_depth', C.c_void_p), ('d_acc', C.c_void_p), ('d_weights', C.c_void_p),
              ('d_warped_points', C.c_void_p)]


class OutputGrads(C.Structure):
  _fields_ = [('coarse', LevelGrads), ('fine', LevelGrads)]


class RayGrads(C.Structure):
  """nrf_ray_grads: the gradients w.r.t. the rays (nrf_backward_rays), each (B,3); a NULL pointer skips that part."""
  _fields_ = [('d_origins', C.c_void_p), ('d_directions', C.c_void_p), ('d_viewdirs', C.c_void_p)]


class Background(C.Structure):
  _fields_ = [('num_points', C.c_int32), ('points', C.c_void_p), ('warp_ids', C.c_void_p), ('loss_weight', C.c_float),
              ('loss_alpha', C.c_float), ('loss_scale', C.c_float), ('id_choices', C.c_void_p), ('num_choices', C.c_int32),
              ('noise_std', C.c_float)]


class Elastic(C.Structure):
  _fields_ = [('loss_weight', C.c_float), ('reduce_method', C.c_int32), ('eps', C.c_float), ('loss_alpha', C.c_float),
              ('loss_scale', C.c_float), ('loss_type', C.c_int32)]


class WarpReg(C.Structure):
  _fields_ = [('loss_weight', C.c_float), ('loss_alpha', C.c_float), ('loss_scale', C.c_float)]


class CameraDesc(C.Structure):
  _fields_ = [('orientation', C.c_float * 9), ('position', C.c_float * 3), ('focal_length', C.c_float),
              ('principal_point', C.c_float * 2), ('skew', C.c_float), ('pixel_aspect_ratio', C.c_float),
              ('radial_distortion', C.c_float * 3), ('tangential_distortion', C.c_float * 2),
              ('image_size', C.c_int32 * 2)]


class ProfileEntry(C.Structure):
  _fields_ = [('name', C.c_char * 32), ('ms', C.c_double), ('launches', C.c_int32), ('pad_', C.c_int32),
              ('flops_per_launch', C.c_double)]


class FieldOut(C.Structure):
  """nrf_field_out: the device outputs of a field query, N rows each; a NULL pointer skips that output (rgb NULL: density only)."""
  _fields_ = [('sigma', C.c_void_p), ('rgb', C.c_void_p), ('warped_points', C.c_void_p)]


class Grid(C.Structure):
  """nrf_grid: point n = (i, j, k) with x fastest, coordinate c = origin[c] + idx_c * step[c]."""
  _fields_ = [('origin', C.c_float * 3), ('step', C.c_float * 3), ('dims', C.c_int32 * 3), ('reserved', C.c_int32)]


def grid(origin, step, dims) -> Grid:
  """The nrf_grid of `dims` points per axis from `origin`, `step` apart."""
  return Grid((C.c_float * 3)(*[float(v) for v in origin]), (C.c_float * 3)(*[float(v) for v in step]),
              (C.c_int32 * 3)(*[int(v) for v in dims]), 0)


class FieldGradOut(C.Structure):
  """nrf_field_grad_out: the device outputs of a gradient query, N rows each; a NULL pointer skips that output."""
  _fields_ = [('sigma', C.c_void_p), ('grad_sigma', C.c_void_p), ('normals', C.c_void_p), ('warped_points', C.c_void_p)]


class UnwarpOut(C.Structure):
  """nrf_unwarp_out: the device outputs of nrf_unwarp_points, N rows each; a NULL pointer skips that output."""
  _fields_ = [('points', C.c_void_p), ('residual', C.c_void_p), ('status', C.c_void_p)]


class MeshStatus(C.Structure):
  """nrf_mesh_status: the first 16 bytes of a mesh workspace (device memory) after nrf_mesh_count / nrf_mesh_emit."""
  _fields_ = [('num_vertices', C.c_int32), ('num_triangles', C.c_int32), ('emitted_vertices', C.c_int32), ('emitted_triangles', C.c_int32)]


class MeshComponentsStatus(C.Structure):
  """nrf_mesh_components_status: the first 16 bytes of a components workspace (device memory)."""
  _fields_ = [('num_components', C.c_int32), ('table_components', C.c_int32), ('error', C.c_int32), ('reserved', C.c_int32)]


class MeshRasterStatus(C.Structure):
  """nrf_mesh_raster_status: the first 16 bytes of a raster workspace (device memory) after nrf_mesh_raster_draw."""
  _fields_ = [('drawn_triangles', C.c_int32), ('large_triangles', C.c_int32), ('covered_pixels', C.c_int32), ('reserved', C.c_int32)]


NRF_QUERY_MAX_POINTS = 1 << 24   # points of one nrf_query_points / nrf_query_grid call
NRF_QUERY_GRAD_MAX_POINTS = 1 << 20   # points of one nrf_query_points_grad / nrf_query_grid_grad call
NRF_GRID_MAX_POINTS = 1 << 40    # points of a whole nrf_grid
NRF_HAS_UNWARP = 1
NRF_UNWARP_MAX_POINTS = 1 << 20  # points of one nrf_unwarp_points call
NRF_UNWARP_MAX_STEPS = 32        # Newton rounds of one nrf_unwarp_points call
NRF_MESH_MAX_CELLS = 1 << 28     # cells of a grid handed to nrf_mesh_count / nrf_mesh_emit (triangle indices stay in int32)
NRF_HAS_MESH_RASTER = 1
NRF_MESH_RASTER_MAX_PIXELS = 1 << 26   # pixels of one nrf_mesh_raster_draw image
NRF_OPT_CHAIN_TILE_ROWS = 1
NRF_OPT_BF16_WGRAD_MERGE = 2

EXPORTS = [
    'nrf_version', 'nrf_last_error', 'nrf_create', 'nrf_destroy', 'nrf_param_count', 'nrf_param_layout',
    'nrf_workspace_bytes', 'nrf_forward', 'nrf_backward', 'nrf_train_step_loss_grad', 'nrf_adam_step',
    'nrf_sample_along_rays', 'nrf_volumetric_rendering', 'nrf_sample_pdf', 'nrf_profile_enable', 'nrf_profile_read',
    'nrf_debug_wgrad_segments', 'nrf_debug_ws_offset', 'nrf_train_step_loss_grad_ex', 'nrf_workspace_bytes_ex',
    'nrf_warp_points_workspace_bytes', 'nrf_warp_points',
    'nrf_camera_pixels_to_rays', 'nrf_camera_pixels_to_points', 'nrf_camera_project',
    'nrf_dynamic_scalars_write', 'nrf_adam_step_dynamic', 'nrf_set_option', 'nrf_debug_plan_digest', 'nrf_backward_ex',
    'nrf_backward_rays',
    'nrf_camera_table_rays', 'nrf_camera_table_project', 'nrf_camera_table_workspace_bytes', 'nrf_camera_table_rays_backward',
    'nrf_camera_table_project_backward', 'nrf_camera_table_project_depth',
    'nrf_train_step_loss_grad_rays', 'nrf_camera_table_compose', 'nrf_camera_table_compose_backward',
    'nrf_loss_grad_rays',
    'nrf_query_workspace_bytes', 'nrf_query_points', 'nrf_query_grid',
    'nrf_query_grad_workspace_bytes', 'nrf_query_points_grad', 'nrf_query_grid_grad',
    'nrf_unwarp_workspace_bytes', 'nrf_unwarp_points',
    'nrf_mesh_workspace_bytes', 'nrf_mesh_count', 'nrf_mesh_emit', 'nrf_mesh_snap',
    'nrf_mesh_components_workspace_bytes', 'nrf_mesh_components', 'nrf_mesh_component_table',
    'nrf_mesh_submesh_workspace_bytes', 'nrf_mesh_submesh_count', 'nrf_mesh_submesh_emit', 'nrf_mesh_gather_rows',
    'nrf_mesh_raster_workspace_bytes', 'nrf_mesh_raster_draw', 'nrf_mesh_raster_interpolate', 'nrf_mesh_raster_visibility',
]

_lib = None


def load_library(path=None):
  """Loads libnerfies_amd.so (built by nerfies_amd.build / __graft_entry__.build())."""
  global _lib
  if _lib is not None and path is None:
    return _lib
  # torch first: its wheel carries its own HIP runtime; loading ours before it would put two runtimes in one
  # process (device pointers of one are "no ROCm-capable device" errors in the other)
  import torch  # noqa: F401
  path = path or os.environ.get('NRF_LIB_PATH') or LIB_PATH   # NRF_LIB_PATH: experiment builds of the same ABI
  if not os.path.exists(path):
    raise NrfError(
        f'HIP extension not built: {path} is missing. Run `python -c "import __graft_entry__ as g; g.build()"` '
        '(needs hipcc). There is no CPU fallback for the hot path.')
  lib = C.CDLL(path)
  vp, i32, i64, u32, u64, f32, f64 = C.c_void_p, C.c_int32, C.c_int64, C.c_uint32, C.c_uint64, C.c_float, C.c_double
  lib.nrf_version.restype = C.c_int
  lib.nrf_last_error.restype = C.c_char_p
  sigs = {
      'nrf_create': [C.POINTER(ModelDesc), C.POINTER(vp)],
      'nrf_destroy': [vp],
      'nrf_param_count': [vp, C.POINTER(i64)],
      'nrf_param_layout': [vp, C.POINTER(TensorInfo), C.POINTER(i32)],
      'nrf_workspace_bytes': [vp, i32, u32, C.POINTER(C.c_size_t)],
      'nrf_forward': [vp, vp, C.POINTER(Rays), C.POINTER(StepScalars), C.POINTER(Rand), C.POINTER(Outputs), u32, vp,
                      C.c_size_t, vp],
      'nrf_backward': [vp, vp, C.POINTER(Rays), vp, vp, vp, vp, C.c_size_t, vp],
      'nrf_backward_ex': [vp, vp, C.POINTER(Rays), C.POINTER(OutputGrads), vp, vp, C.c_size_t, vp],
      'nrf_backward_rays': [vp, vp, C.POINTER(Rays), C.POINTER(OutputGrads), C.POINTER(RayGrads), vp, vp, C.c_size_t, vp],
      'nrf_train_step_loss_grad': [vp, vp, C.POINTER(Rays), vp, C.POINTER(StepScalars), C.POINTER(Rand), vp, vp, vp,
                                   C.c_size_t, vp],
      'nrf_adam_step': [vp, vp, vp, vp, i64, f64, f64, f64, f64, i64, f64, vp],
      'nrf_adam_step_dynamic': [vp, vp, vp, vp, i64, f64, f64, f64, vp, vp],
      'nrf_dynamic_scalars_write': [vp, C.POINTER(DynamicScalars), vp],
      'nrf_sample_along_rays': [vp, vp, i32, i32, f32, f32, i32, i32, vp, u64, u64, vp, vp],
      'nrf_volumetric_rendering': [vp, vp, vp, i32, i32, i32, i32, C.POINTER(LevelOut), vp],
      'nrf_sample_pdf': [vp, vp, i32, i32, i32, i32, vp, u64, u64, vp, vp],
      'nrf_profile_enable': [vp, i32],
      'nrf_profile_read': [vp, C.POINTER(ProfileEntry), C.POINTER(i32)],
      'nrf_debug_wgrad_segments': [vp, vp, C.POINTER(C.c_double), C.POINTER(i32)],
      'nrf_debug_ws_offset': [vp, C.c_char_p, i32, C.POINTER(i64)],
      'nrf_debug_plan_digest': [vp, C.POINTER(u64)],
      'nrf_set_option': [vp, i32, i64],
      'nrf_train_step_loss_grad_ex': [vp, vp, C.POINTER(Rays), vp, C.POINTER(StepScalars), C.POINTER(Rand),
                                      C.POINTER(Background), C.POINTER(Elastic), C.POINTER(WarpReg), u32, vp, vp, vp,
                                      C.c_size_t, vp],
      'nrf_train_step_loss_grad_rays': [vp, vp, C.POINTER(Rays), vp, C.POINTER(StepScalars), C.POINTER(Rand),
                                        C.POINTER(Background), C.POINTER(Elastic), C.POINTER(WarpReg), u32, C.POINTER(RayGrads),
                                        vp, vp, vp, C.c_size_t, vp],
      'nrf_loss_grad_rays': [vp, vp, C.POINTER(Rays), vp, C.POINTER(StepScalars), C.POINTER(Rand), C.POINTER(RayGrads), vp, vp,
                             C.c_size_t, vp],
      'nrf_workspace_bytes_ex': [vp, i32, u32, i32, i32, C.POINTER(C.c_size_t)],
      'nrf_warp_points_workspace_bytes': [vp, i32, C.POINTER(C.c_size_t)],
      'nrf_warp_points': [vp, vp, vp, vp, i32, C.POINTER(StepScalars), vp, vp, C.c_size_t, vp],
      'nrf_query_workspace_bytes': [vp, i32, i32, u32, C.POINTER(C.c_size_t)],
      'nrf_query_points': [vp, vp, C.POINTER(Rays), vp, i32, i32, C.POINTER(StepScalars), u32, C.POINTER(FieldOut), vp, C.c_size_t, vp],
      'nrf_query_grid': [vp, vp, C.POINTER(Rays), C.POINTER(Grid), i64, i32, i32, C.POINTER(StepScalars), u32, C.POINTER(FieldOut), vp,
                         C.c_size_t, vp],
      'nrf_query_grad_workspace_bytes': [vp, i32, i32, u32, C.POINTER(C.c_size_t)],
      'nrf_query_points_grad': [vp, vp, C.POINTER(Rays), vp, i32, i32, C.POINTER(StepScalars), u32, C.POINTER(FieldGradOut), vp,
                                C.c_size_t, vp],
      'nrf_query_grid_grad': [vp, vp, C.POINTER(Rays), C.POINTER(Grid), i64, i32, i32, C.POINTER(StepScalars), u32,
                              C.POINTER(FieldGradOut), vp, C.c_size_t, vp],
      'nrf_unwarp_workspace_bytes': [vp, i32, C.POINTER(C.c_size_t)],
      'nrf_unwarp_points': [vp, vp, vp, vp, vp, i32, vp, i32, C.POINTER(StepScalars), i32, f32, f32, C.POINTER(UnwarpOut), vp, C.c_size_t, vp],
      'nrf_mesh_workspace_bytes': [C.POINTER(Grid), C.POINTER(C.c_size_t)],
      'nrf_mesh_count': [vp, C.POINTER(Grid), f32, vp, vp, C.c_size_t, vp],
      'nrf_mesh_emit': [vp, C.POINTER(Grid), f32, i32, i32, vp, vp, vp, vp, C.c_size_t, vp],
      'nrf_mesh_snap': [vp, vp, vp, vp, C.POINTER(Grid), f32, i32, vp],
      'nrf_mesh_components_workspace_bytes': [i32, i32, C.POINTER(C.c_size_t)],
      'nrf_mesh_components': [vp, i32, i32, vp, vp, vp, C.c_size_t, vp],
      'nrf_mesh_component_table': [vp, i32, vp, i32, vp, i32, vp, vp, vp, C.c_size_t, vp],
      'nrf_mesh_submesh_workspace_bytes': [i32, i32, C.POINTER(C.c_size_t)],
      'nrf_mesh_submesh_count': [vp, i32, vp, i32, vp, vp, C.c_size_t, vp],
      'nrf_mesh_submesh_emit': [vp, i32, vp, i32, i32, i32, vp, vp, vp, C.c_size_t, vp],
      'nrf_mesh_gather_rows': [vp, i32, vp, i32, vp, i32, vp],
      'nrf_mesh_raster_workspace_bytes': [i32, i32, i32, C.POINTER(C.c_size_t)],
      'nrf_mesh_raster_draw': [vp, i32, vp, i32, i32, i32, f32, vp, vp, vp, vp, C.c_size_t, vp],
      'nrf_mesh_raster_interpolate': [vp, vp, i64, vp, i32, vp, i32, i32, vp, vp, vp],
      'nrf_mesh_raster_visibility': [vp, i64, vp, i32, i32, vp, vp],
      'nrf_camera_pixels_to_rays': [C.POINTER(CameraDesc), vp, i64, vp, vp, vp, vp],
      'nrf_camera_pixels_to_points': [C.POINTER(CameraDesc), vp, vp, i64, vp, vp],
      'nrf_camera_project': [C.POINTER(CameraDesc), vp, i64, vp, vp],
      'nrf_camera_table_rays': [vp, i32, vp, vp, i64, vp, vp, vp],
      'nrf_camera_table_project': [vp, i32, vp, vp, i64, vp, vp],
      'nrf_camera_table_project_depth': [vp, i32, vp, vp, i64, vp, vp],
      'nrf_camera_table_workspace_bytes': [i64, i32, C.POINTER(C.c_size_t)],
      'nrf_camera_table_rays_backward': [vp, i32, vp, vp, i64, vp, vp, vp, vp, vp, C.c_size_t, vp],
      'nrf_camera_table_project_backward': [vp, i32, vp, vp, i64, vp, vp, vp, vp, C.c_size_t, vp],
      'nrf_camera_table_compose': [vp, vp, i32, vp, vp],
      'nrf_camera_table_compose_backward': [vp, vp, i32, vp, vp, vp],
  }
  for name, argtypes in sigs.items():
    fn = getattr(lib, name)
    fn.argtypes = argtypes
    fn.restype = C.c_int
  _lib = lib
  return lib


def check(rc, lib=None):
  if rc != 0:
    lib = lib or load_library()
    raise NrfError(f'nerfies_amd error {rc}: {lib.nrf_last_error().decode()}')
