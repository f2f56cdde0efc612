"""Host-side mirror of nerfies.models (reference: nerfies/models.py:31-489).

`NerfModel.apply` keeps the reference signature (models.py:289-299); the work is done by the HIP
library through the C-ABI (include/nerfies_amd.h).  Differences forced by the missing JAX runtime:
  * `rngs={'coarse': k0, 'fine': k1}`: a key is either an int seed (on-device Philox) or a float
    tensor of explicit uniforms, (B,N_c) for 'coarse' and (B,N_f) for 'fine' (parity runs);
  * arrays are torch tensors on the GPU; params are a `FlatParams` (fast path) or a flax-style
    nested dict (copied into a flat buffer per call).
"""
import ctypes as C
import os
import dataclasses
from typing import Any, Dict, Mapping, NamedTuple, Optional, Sequence, Tuple

import torch

from nerfies_amd import lib as L
from nerfies_amd import params as P


def _ptr(t: Optional[torch.Tensor]):
  return None if t is None else C.c_void_p(t.data_ptr())


def _ref(struct):
  return None if struct is None else C.byref(struct)


def _stream(device):
  """The current stream of `device`, as the `stream` argument of a library call."""
  return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _stream_arg(device):
  """The `stream` argument of a library call on tensors of `device`, where no device rule stands in front of the call."""
  # a device other than the GPU is reached only under a recording stand-in for the library (the host tests drive the chunking on CPU
  # tensors): the library itself follows these pointers on the GPU alone
  return _stream(device) if device.type == 'cuda' else None


def _gpu_reader(what, t):
  """The device rule: (device, `stream` argument) of `t`, a tensor the library will read; `what` names it in the refusal.  Everything
  behind it takes the pair as it comes, so a host test that installs a recording stand-in for the library lifts the rule by
  replacing this one function."""
  device = torch.as_tensor(t).device
  if device.type != 'cuda':
    raise L.NrfError(f'{what} must live on the GPU: the hot path has no CPU fallback')
  return device, _stream(device)


def _ws_tail(ws, stream):
  """The last three arguments of every entry that runs in a workspace."""
  return _ptr(ws), ws.numel() * 4, stream


def _f32(t, device):
  return torch.as_tensor(t, device=device).to(torch.float32).contiguous()


def _ids(t, device):
  if t is None:
    return None
  t = torch.as_tensor(t, device=device)
  if t.dim() == 2 and t.shape[-1] == 1:   # glo.py:50-51 squeezes the trailing 1
    t = t[..., 0]
  return t.to(torch.int32).contiguous()


def _scalars(warp_extra, dynamic: Optional[torch.Tensor] = None) -> 'L.StepScalars':
  """nrf_step_scalars of warp_extra; `dynamic`: the device buffer of a training.DynamicScalars (graph-replayable step)."""
  we = warp_extra or {}
  return L.StepScalars(float(we.get('alpha', 0.0)), float(we.get('time_alpha', 0.0)), None if dynamic is None else dynamic.data_ptr())


def rng_seed_of(coarse_key: int, fine_key: int) -> int:
  """The Philox seed NerfModel._rand_struct derives from integer 'coarse' / 'fine' keys (what a device-resident
  nrf_dynamic_scalars.rng_seed must hold to reproduce the eager call)."""
  seed = 0
  for k in (coarse_key, fine_key):
    seed = (seed * 0x9E3779B97F4A7C15 + int(k)) & 0xFFFFFFFFFFFFFFFF
  return seed


class CallRecord(NamedTuple):
  """One library call's mode and memory: what `NerfModel.stash` holds for `backward`, and what a captured graph keeps so that the
  workspace its launches point into lives as long as the graph."""
  num_rays: int      # first, then the workspace: a record still indexes like the (B, ws) pair the stash used to be
  ws: torch.Tensor   # the workspace the call ran in
  flags: int         # the NRF_FLAG_* word of the call
  generation: int    # NerfModel.generation at the call: it moves when a workspace option replaces the plans


def grid_chunks(total: int, chunk: int):
  """(first, count) pieces that cover [0, total) exactly once, in order, `chunk` points at most each."""
  return [(first, min(chunk, total - first)) for first in range(0, total, chunk)]


def _select_outputs(outputs, allowed):
  """`outputs` as a tuple: a non-empty selection of `allowed`."""
  outputs = tuple(outputs)
  if not outputs or set(outputs) - set(allowed):
    raise L.NrfError(f'outputs must be a non-empty selection of {allowed}, got {outputs}')
  return outputs


def _out_struct(out_type, allowed, tensors):
  """The library's `out_type` over `tensors` ({name: tensor or slice of one}): the fields in the order of `allowed`, a NULL pointer
  (that output is skipped) for a name that is absent."""
  return out_type(*(_ptr(tensors.get(k)) for k in allowed))


def _require_out(where, name, t, shape, dtype=torch.float32):
  """`t` is what the library writes a caller-supplied output `name` of `where` into: contiguous, of `dtype` and `shape`."""
  if tuple(t.shape) != tuple(shape) or t.dtype != dtype or not t.is_contiguous():
    raise L.NrfError(f'{where}: {name} must be a contiguous {dtype} tensor of shape {tuple(shape)}')


RAY_GRADS = ('origins', 'directions', 'viewdirs')   # the rays' differentiable entries, in the order of lib.RayGrads


def _ray_grads_out(where, names, given, num_rays, device, allowed=RAY_GRADS,
                   what="the rays' differentiable entries are 'origins', 'directions', 'viewdirs'"):
  """The ray gradients `names` (out of `allowed`, or an NrfError that ends in `what`) of the method `where`: -> ({name: (B, 3) tensor,
  taken from `given` = the caller's ray_grads_out or allocated}, the lib.RayGrads over them)."""
  names = tuple(names)
  if set(names) - set(allowed):
    raise L.NrfError(f"{where}(ray_grads=...): {sorted(names)} -- {what}")
  out = {}
  for k in names:
    out[k] = (given or {}).get(k)
    if out[k] is None:
      out[k] = torch.empty(num_rays, 3, device=device)
    else:
      _require_out(f'{where}(ray_grads_out=...)', repr(k), out[k], (num_rays, 3))
  return out, _out_struct(L.RayGrads, RAY_GRADS, out)


def _background_struct(background, device):
  """-> (lib.Background or None, its point count, the tensors it points into)."""
  if background is None:
    return None, 0, []
  pts = _f32(background['points'], device).reshape(-1, 3)
  head = (float(background.get('weight', 1.0)), float(background.get('alpha', -2.0)), float(background.get('scale', 0.001)))
  if background.get('warp_ids') is not None:   # the caller drew ids and noise (parity runs)
    ids = _ids(background['warp_ids'], device).reshape(-1)
    return L.Background(pts.shape[0], _ptr(pts), _ptr(ids), *head, None, 0, 0.0), pts.shape[0], [pts, ids]
  choices = _ids(background['id_choices'], device).reshape(-1)   # the library draws them (training.py:121-126)
  bg = L.Background(pts.shape[0], _ptr(pts), None, *head, _ptr(choices), choices.numel(), float(background.get('noise_std', 0.001)))
  return bg, pts.shape[0], [pts, choices]


def _elastic_struct(elastic):
  if elastic is None:
    return None
  method = elastic.get('reduce_method', 'weight')
  if method not in L.ELASTIC_REDUCE:
    raise L.NrfError(f'unknown elastic_reduce_method {method!r}')
  ltype = elastic.get('loss_type', 'log_svals')
  if ltype not in L.ELASTIC_TYPE:
    raise L.NrfError(f"elastic_loss_type {ltype!r} is not built (one of {sorted(L.ELASTIC_TYPE)}; 'nr' produces NaNs in "
                     'the reference itself, training.py:58)')
  return L.Elastic(float(elastic.get('weight', 0.0)), L.ELASTIC_REDUCE[method], float(elastic.get('eps', 1e-6)),
                   float(elastic.get('alpha', -2.0)), float(elastic.get('scale', 0.03)), L.ELASTIC_TYPE[ltype])


def _warp_reg_struct(warp_reg):
  if warp_reg is None:
    return None
  return L.WarpReg(float(warp_reg.get('weight', 0.0)), float(warp_reg.get('alpha', -2.0)), float(warp_reg.get('scale', 0.001)))


def _act_name(a):
  if isinstance(a, str):
    return a
  name = getattr(a, '__name__', str(a))
  for k in ('softplus', 'relu'):
    if k in name:
      return k
  raise ValueError(f'unsupported activation {a!r}')


@dataclasses.dataclass
class NerfModel:
  """Attributes mirror nerfies.models.NerfModel (models.py:75-119)."""
  num_coarse_samples: int
  num_fine_samples: int
  use_viewdirs: bool
  near: float
  far: float
  noise_std: Optional[float]
  nerf_trunk_depth: int
  nerf_trunk_width: int
  nerf_rgb_branch_depth: int
  nerf_rgb_branch_width: int
  nerf_skips: Tuple[int, ...]
  alpha_channels: int
  rgb_channels: int
  use_stratified_sampling: bool
  num_nerf_point_freqs: int
  num_nerf_viewdir_freqs: int
  appearance_ids: Sequence[int]
  camera_ids: Sequence[int]
  warp_ids: Sequence[int]
  num_appearance_features: int
  num_camera_features: int
  num_warp_features: int
  num_warp_freqs: int
  activation: Any = 'relu'
  sigma_activation: Any = 'relu'
  use_white_background: bool = False
  use_linear_disparity: bool = False
  use_sample_at_infinity: bool = True
  warp_field_type: str = 'se3'
  warp_metadata_encoder_type: str = 'glo'
  use_appearance_metadata: bool = False
  use_camera_metadata: bool = False
  use_warp: bool = False
  use_warp_jacobian: bool = False
  use_weights: bool = False
  use_trunk_condition: bool = False
  use_alpha_condition: bool = False
  use_rgb_condition: bool = False
  warp_kwargs: Mapping[str, Any] = dataclasses.field(default_factory=dict)
  metadata_encoded: bool = False

  def __post_init__(self):
    self._handle = None
    self._layout = None
    self._ws = {}
    self._lib = None
    self.stash = None      # the CallRecord of the last training forward / fused step: what `backward` differentiates
    self.last_call = None  # the CallRecord of the last apply / loss_and_grad, training or not (what a graph capture keeps)
    self.generation = 0    # bumped by every workspace option: records of an older generation describe plans that no longer exist

  # models.py:121-131
  @property
  def num_appearance_embeddings(self):
    return max(self.appearance_ids) + 1

  @property
  def num_warp_embeddings(self):
    return max(self.warp_ids) + 1

  @property
  def num_camera_embeddings(self):
    return max(self.camera_ids) + 1

  # ---- C-ABI plumbing -------------------------------------------------------------------
  def desc(self) -> L.ModelDesc:
    if _act_name(self.activation) != 'relu':
      raise L.NrfError('only relu trunk activation is built')
    if self.alpha_channels != 1 or self.rgb_channels != 3:
      raise L.NrfError('alpha_channels/rgb_channels must be 1/3')
    skips = tuple(self.nerf_skips)
    if len(skips) > 1:
      raise L.NrfError('at most one skip layer')
    d = L.ModelDesc()
    d.num_coarse_samples = self.num_coarse_samples
    d.num_fine_samples = self.num_fine_samples
    d.use_viewdirs = int(self.use_viewdirs)
    d.near_plane = float(self.near)
    d.far_plane = float(self.far)
    d.nerf_trunk_depth = self.nerf_trunk_depth
    d.nerf_trunk_width = self.nerf_trunk_width
    d.nerf_rgb_branch_depth = self.nerf_rgb_branch_depth
    d.nerf_rgb_branch_width = self.nerf_rgb_branch_width
    d.nerf_skip_layer = skips[0] if skips else -1
    d.use_stratified_sampling = int(self.use_stratified_sampling)
    d.num_nerf_point_freqs = self.num_nerf_point_freqs
    d.num_nerf_viewdir_freqs = self.num_nerf_viewdir_freqs
    d.sigma_activation = L.ACT[_act_name(self.sigma_activation)]
    d.use_white_background = int(self.use_white_background)
    d.use_linear_disparity = int(self.use_linear_disparity)
    d.use_sample_at_infinity = int(self.use_sample_at_infinity)
    d.use_appearance_metadata = int(self.use_appearance_metadata)
    d.num_appearance_embeddings = self.num_appearance_embeddings if self.use_appearance_metadata else 0
    d.num_appearance_features = self.num_appearance_features
    d.use_camera_metadata = int(self.use_camera_metadata)
    d.num_camera_embeddings = self.num_camera_embeddings if self.use_camera_metadata else 0
    d.num_camera_features = self.num_camera_features
    d.use_alpha_condition = int(self.use_alpha_condition)
    d.use_rgb_condition = int(self.use_rgb_condition)
    d.use_trunk_condition = int(self.use_trunk_condition)
    if self.use_warp and self.warp_field_type not in L.WARP_FIELD:
      raise L.NrfError(f"warp_field_type must be one of {sorted(L.WARP_FIELD)} (warping.py:36-44)")
    wdepth, wwidth = self._warp_trunk_shape()
    if self.use_warp and self.warp_metadata_encoder_type not in L.META_ENCODER:
      raise L.NrfError(f"warp_metadata_encoder_type must be one of {sorted(L.META_ENCODER)} ('blend' exists only in the "
                       'TranslationField, warping.py:142-146, and no preset selects it)')
    d.use_warp = int(self.use_warp)
    d.num_warp_freqs = self.num_warp_freqs
    d.num_warp_embeddings = self.num_warp_embeddings if self.use_warp else 0
    d.num_warp_features = self.num_warp_features
    d.warp_field_type = L.WARP_FIELD[self.warp_field_type] if self.use_warp else 0
    d.noise_std = float(self.noise_std or 0.0)
    d.warp_metadata_encoder_type = L.META_ENCODER[self.warp_metadata_encoder_type] if self.use_warp else 0
    d.num_time_encoder_freqs = 1   # metadata_encoder_num_freqs (warping.py:234): the field's default (_warp_trunk_shape refuses others)
    d.warp_trunk_depth, d.warp_trunk_width = (wdepth, wwidth) if self.use_warp else (0, 0)
    return d

  # ModelConfig.warp_kwargs (configs.py:105) are passed through create_warp_field to the field's constructor
  # (models.py:165-184, warping.py:29-59).  Built: the trunk's depth (<= 6) and width (<= 128) -- SE3Field trunk_depth / trunk_width
  # (warping.py:225-226), TranslationField depth / hidden_channels (warping.py:90-91).  Every other attribute must keep the field's
  # default: the kernels have the branches as bare 3-channel output layers (rotation / pivot / translation depth 0), no pivot or
  # translation branch, relu, skips (4,), frequencies 2^0 .. 2^(F-1) with the identity map.
  _WARP_KW_DEFAULTS = {
      'se3': dict(skips=(4,), rotation_depth=0, pivot_depth=0, translation_depth=0, use_pivot=False, use_translation=False,
                  min_freq_log2=0, max_freq_log2=None, use_identity_map=True, metadata_encoder_num_freqs=1),
      'translation': dict(skips=(4,), min_freq_log2=0, max_freq_log2=None, use_identity_map=True, metadata_encoder_num_freqs=1),
  }
  _WARP_KW_TRUNK = {'se3': ('trunk_depth', 'trunk_width'), 'translation': ('depth', 'hidden_channels')}

  def _warp_trunk_shape(self):
    kw = dict(self.warp_kwargs or {})
    if not self.use_warp or not kw:
      return 0, 0
    ft = self.warp_field_type
    dk, wk = self._WARP_KW_TRUNK.get(ft, (None, None))
    depth, width = int(kw.pop(dk, 6)), int(kw.pop(wk, 128))
    if not (1 <= depth <= 6 and 1 <= width <= 128):
      raise L.NrfError(f'warp_kwargs: {dk} must be in [1, 6] and {wk} in [1, 128] (the warp kernels are 6 x 128; got {depth} x {width})')
    # widths of branches that do not exist at depth 0 are inert (modules.MLP builds no hidden layer), as is the activation name relu
    for inert in ('rotation_width', 'pivot_width', 'translation_width'):
      kw.pop(inert, None)
    if 'activation' in kw and _act_name(kw['activation']) == 'relu':
      kw.pop('activation')
    if 'metadata_encoder_type' in kw and kw['metadata_encoder_type'] == self.warp_metadata_encoder_type:
      kw.pop('metadata_encoder_type')
    for k, dflt in self._WARP_KW_DEFAULTS.get(ft, {}).items():
      if k in kw and (tuple(kw[k]) if k == 'skips' else kw[k]) == dflt:
        kw.pop(k)
    if kw:
      raise L.NrfError(f'warp_kwargs {kw} are not supported: built are {dk} <= 6 and {wk} <= 128; every other attribute of the '
                       f'{ft} field must keep its default (warping.py:216-243)')
    return depth, width


  @property
  def lib(self):
    if self._lib is None:
      self._lib = L.load_library()
    return self._lib

  @property
  def handle(self):
    if self._handle is None:
      h = C.c_void_p()
      d = self.desc()
      L.check(self.lib.nrf_create(C.byref(d), C.byref(h)), self.lib)
      self._handle = h
      rows = os.environ.get('NRF_CHAIN_TILE_ROWS')   # experiments / the A-B tests: 32 or 64 for every model of the process
      if rows:
        self.set_chain_tile_rows(int(rows))
      if os.environ.get('NRF_BF16_WGRAD_MERGE'):   # experiments / the A-B record: merged bf16 wgrad groups (nerfies_amd.h)
        L.check(self.lib.nrf_set_option(h, L.NRF_OPT_BF16_WGRAD_MERGE, int(os.environ['NRF_BF16_WGRAD_MERGE'])), self.lib)
    return self._handle

  def set_chain_tile_rows(self, rows: int):
    """NRF_OPT_CHAIN_TILE_ROWS: rows per workgroup tile of the float32 NeRF chain kernels -- 64 (two workgroups per CU), 32
    (four per CU) or 0 = automatic (the default).  A tuning knob without a reference counterpart; forward results are bit-identical
    under both tilings, gradients agree to the order of float atomics."""
    L.check(self.lib.nrf_set_option(self.handle, L.NRF_OPT_CHAIN_TILE_ROWS, int(rows)), self.lib)
    self._drop_workspaces()

  def set_bf16_wgrad_merge(self, on: bool):
    """NRF_OPT_BF16_WGRAD_MERGE: merged weight-gradient groups of the bf16 training mode (default on).  The option changes the
    training workspace's SIZE and layout, so the cached workspaces (and the stash a pending `backward` would read) are dropped:
    a live model picks the option up at its next step instead of running the new plan in a buffer sized for the old one."""
    L.check(self.lib.nrf_set_option(self.handle, L.NRF_OPT_BF16_WGRAD_MERGE, int(bool(on))), self.lib)
    self._drop_workspaces()

  def _drop_workspaces(self):
    self.generation += 1
    self._ws = {}
    self.stash = self.last_call = None

  @property
  def layout(self) -> P.ParamLayout:
    if self._layout is None:
      n = C.c_int32(0)
      L.check(self.lib.nrf_param_layout(self.handle, None, C.byref(n)), self.lib)
      infos = (L.TensorInfo * n.value)()
      L.check(self.lib.nrf_param_layout(self.handle, infos, C.byref(n)), self.lib)
      total = C.c_int64(0)
      L.check(self.lib.nrf_param_count(self.handle, C.byref(total)), self.lib)
      self._layout = P.layout_from_infos(infos, total.value)
    return self._layout

  @staticmethod
  def bf16_flags(bf16) -> int:
    """bf16=True: NRF_FLAG_BF16 (NeRF MLPs AND the SE3 trunk on bfloat16 operands); bf16='mlp': the NeRF MLPs only
    (NRF_FLAG_WARP_F32: the round-3 behaviour); bf16='x3' (inference only): NRF_FLAG_BF16X3, the NeRF MLPs and the SE3 trunk in split-bf16
    (float32-emulating) arithmetic ('x3mlp': the trunk stays float32); False: float32."""
    if not bf16:
      return 0
    if bf16 == 'x3':
      return L.NRF_FLAG_BF16X3
    if bf16 == 'x3mlp':   # split-bf16 NeRF MLPs, float32 SE3 trunk (bit-identical warped points)
      return L.NRF_FLAG_BF16X3 | L.NRF_FLAG_WARP_F32
    if bf16 == 'mlp':
      return L.NRF_FLAG_BF16 | L.NRF_FLAG_WARP_F32
    return L.NRF_FLAG_BF16

  def flags(self, train=False, bf16=False, no_warp=False, jacobian=False, ray_grads=False, frozen=False) -> int:
    """The NRF_FLAG_* word of a call: the one place where a mode becomes bits."""
    return (L.NRF_FLAG_TRAIN if train else 0) | self.bf16_flags(bf16) | (L.NRF_FLAG_NO_WARP if no_warp else 0) | \
        (L.NRF_FLAG_WARP_JACOBIAN if jacobian else 0) | (L.NRF_FLAG_RAY_GRADS if ray_grads else 0) | \
        (L.NRF_FLAG_FROZEN if frozen else 0)

  def check_mode(self, bf16, train: bool = False):
    """Raises NrfError with the library's own message when this model cannot run in the `bf16` mode (a moved skip or an rgb
    branch deeper than one layer exist in the float32 chains only): what the drivers ask before they load data or capture a graph."""
    nbytes = C.c_size_t(0)
    L.check(self.lib.nrf_workspace_bytes(self.handle, 1, self.flags(train, bf16), C.byref(nbytes)), self.lib)

  def workspace(self, num_rays: int, train: bool, device, num_background_points: int = 0, elastic: bool = False,
                jacobian: bool = False, bf16=False, ray_grads: bool = False) -> torch.Tensor:
    return self._record(num_rays, self.flags(train, bf16, jacobian=jacobian, ray_grads=ray_grads), device, num_background_points,
                        elastic).ws

  def _record(self, num_rays, flags, device, num_background_points=0, elastic=False) -> CallRecord:
    """The CallRecord of a call under `flags`, its workspace taken from the cache.  The cache is keyed by the word the workspace is
    sized for: the call's, less the bits that change no layout -- adding a flag needs no second edit here unless it is one of those."""
    plan = flags & ~L.NRF_FLAG_NO_WARP   # a call that skips the warp field runs in the workspace of one that does not
    if plan & L.NRF_FLAG_BF16X3:   # an 'x3' inference plan has its own weight streams, with or without the float32 trunk
      plan &= ~L.NRF_FLAG_WARP_F32
    elif not plan & L.NRF_FLAG_TRAIN:   # only the TRAINING layout depends on bf16 (bf16 stashes instead of the fp32 ones)
      plan &= ~(L.NRF_FLAG_BF16 | L.NRF_FLAG_WARP_F32)
    key = (plan, int(num_rays), str(device), int(num_background_points), bool(elastic))
    ws = self._workspace(key, device, self.lib.nrf_workspace_bytes_ex, num_rays, plan, int(num_background_points), int(bool(elastic)))
    return CallRecord(int(num_rays), ws, flags, self.generation)

  def _workspace(self, key, device, sizer, *args) -> torch.Tensor:
    """The workspace `sizer(handle, *args, &bytes)` asks for, as float32 words on `device`: the one cached under `key`, made at the
    first call and kept until a workspace option drops the cache -- or, with key=None, a new one that is not kept."""
    ws = self._ws.get(key)
    if ws is None:
      nbytes = C.c_size_t(0)
      L.check(sizer(self.handle, *args, C.byref(nbytes)), self.lib)
      ws = torch.empty((nbytes.value + 3) // 4, dtype=torch.float32, device=device)
      if key is not None:
        self._ws[key] = ws
    return ws

  def flat_params(self, variables, device) -> P.FlatParams:
    params = variables['params'] if isinstance(variables, dict) and 'params' in variables else variables
    if isinstance(params, P.FlatParams):
      return params
    if isinstance(params, dict) and 'model' in params and 'nerf_mlps_coarse' not in params:
      params = params['model']
    return P.FlatParams(P.flat_from_tree(params, self.layout, device), self.layout)

  def _rays_struct(self, rays_dict, device, metadata_encoded=False):
    origins = _f32(rays_dict['origins'], device)
    directions = _f32(rays_dict['directions'], device)
    viewdirs = _f32(rays_dict['viewdirs'], device) if 'viewdirs' in rays_dict else None
    md = rays_dict.get('metadata', {}) or {}
    keep = [origins, directions, viewdirs]
    r = L.Rays()
    r.num_rays = origins.shape[0]
    r.origins, r.directions, r.viewdirs = _ptr(origins), _ptr(directions), _ptr(viewdirs)
    self._metadata_into(r, md, device, metadata_encoded, keep)
    return r, keep

  def _metadata_into(self, r, md, device, metadata_encoded, keep):
    """The ids / codes / time stamps of `md`, one row per ray (or per group of a field query), into the lib.Rays `r`."""
    time_enc = self.use_warp and self.warp_metadata_encoder_type == 'time'
    for field, cfield, key, width in (('warp_ids', 'warp_codes', 'warp', self.num_warp_features),
                                      ('appearance_ids', 'appearance_codes', 'appearance', self.num_appearance_features),
                                      ('camera_ids', 'camera_codes', 'camera', self.num_camera_features)):
      src = md.get('time' if (key == 'warp' and time_enc) else key)   # models.py:252-254
      if src is None:
        continue
      if metadata_encoded:   # the codes themselves, (B, features) (models.py:198-199, 210-211, 251)
        t = _f32(src, device).reshape(r.num_rays, -1)
        if t.shape[1] != width:
          raise L.NrfError(f"metadata_encoded: metadata[{key!r}] must have {width} features, got {t.shape[1]}")
        setattr(r, cfield, _ptr(t))
      elif key == 'warp' and time_enc:   # float timestamps for the TimeEncoder (datasets/core.py:272-274)
        t = _f32(src, device).reshape(-1)
        r.time = _ptr(t)
      else:
        t = _ids(src, device)
        setattr(r, field, _ptr(t))
      keep.append(t)

  def _rand_struct(self, rngs, num_rays, device):
    rnd = L.Rand()
    keep = []
    rngs = rngs or {}
    for field, key, n in (('noise_coarse', 'noise_coarse', self.num_coarse_samples),
                          ('noise_fine', 'noise_fine', self.num_coarse_samples + self.num_fine_samples)):
      k = rngs.get(key)   # explicit standard normals for noise_regularize (parity runs)
      if k is not None:
        t = _f32(k, device)
        if tuple(t.shape) != (num_rays, n):
          raise L.NrfError(f"rngs[{key!r}] normals must have shape {(num_rays, n)}")
        keep.append(t)
        setattr(rnd, field, _ptr(t))
    for field, key, n in (('t_rand', 'coarse', self.num_coarse_samples), ('u', 'fine', self.num_fine_samples)):
      k = rngs.get(key)
      if isinstance(k, torch.Tensor) and k.is_floating_point() and k.dim() == 2:
        if tuple(k.shape) != (num_rays, n):
          raise L.NrfError(f"rngs[{key!r}] uniforms must have shape {(num_rays, n)}")
        t = _f32(k, device)
        keep.append(t)
        setattr(rnd, field, _ptr(t))
      elif k is not None:
        seed = int(k.item()) if isinstance(k, torch.Tensor) else int(k)
        rnd.seed = (rnd.seed * 0x9E3779B97F4A7C15 + seed) & 0xFFFFFFFFFFFFFFFF
    return rnd, keep

  # ---- NerfModel.__call__ (models.py:289-375) ---------------------------------------------
  def apply(self, variables, rays_dict: Dict[str, Any], warp_extra: Dict[str, Any] = None, metadata_encoded=False,
            use_warp=True, return_points=False, return_weights=False, return_warp_jacobian=False,
            deterministic=False, rngs=None, *, train=False, return_z_vals=False, out=None, bf16=False,
            ray_grads=False, frozen=False):
    """Returns {'coarse': {...}, 'fine': {...}} like the reference.  `train=True` keeps the
    activation stash so `backward` can follow (used by training.train_step / autograd).  `out`: a dict
    returned by an earlier call with the same shapes/flags, to be overwritten in place (fixed output
    addresses: what a captured hipGraph replay needs).  `bf16=True` (inference only, no reference counterpart): the NeRF
    MLPs take bfloat16 operands (NRF_FLAG_BF16), everything else stays fp32.  `ray_grads=True` (with train=True, float32 mode):
    NRF_FLAG_RAY_GRADS, the stash also keeps what `backward(..., ray_grads=True)` needs for the gradients w.r.t. the rays.
    `frozen=True` (with train=True, ray_grads=True): NRF_FLAG_FROZEN, the parameters are constants of the call -- the stash keeps ONLY
    what the rays' gradient reads (no activation stash), and `backward(..., ray_grads=...)` returns (None, {name: grad})."""
    del deterministic   # accepted and unused, as in the reference (models.py:298)
    warp_on = bool(self.use_warp and use_warp)
    # models.py:345-346, 367-368: the coarse level carries the Jacobian when the model was built with use_warp_jacobian
    # or the call asks for it, the fine level only when the call asks for it
    jac_levels = set()
    if warp_on and not train:
      if return_warp_jacobian or self.use_warp_jacobian:
        jac_levels.add('coarse')
      if return_warp_jacobian:
        jac_levels.add('fine')
    if train and metadata_encoded:
      raise L.NrfError('metadata_encoded=True is an inference input (the reference never trains with it)')
    device, stream = _gpu_reader('rays', rays_dict['origins'])
    fp = self.flat_params(variables, device)
    rays, keep = self._rays_struct(rays_dict, device, metadata_encoded)
    B = rays.num_rays
    rnd, keep2 = self._rand_struct(rngs, B, device)
    return_weights = self.use_weights or return_weights
    S = (self.num_coarse_samples, self.num_coarse_samples + self.num_fine_samples)
    reuse = out
    out = L.Outputs()
    ret = {}
    levels = [('coarse', out.coarse, S[0])] + ([('fine', out.fine, S[1])] if self.num_fine_samples > 0 else [])
    for name, lo, s in levels:
      if reuse is not None:
        d = reuse[name]
      else:
        d = {'rgb': torch.empty(B, 3, device=device), 'depth': torch.empty(B, device=device),
             'med_depth': torch.empty(B, device=device), 'acc': torch.empty(B, device=device)}
        if return_weights:
          d['weights'] = torch.empty(B, s, device=device)
        if return_z_vals:   # extra (not in the reference dict): the sample depths of this level
          d['z_vals'] = torch.empty(B, s, device=device)
        if return_points:   # models.py:247-248 (always), 266-267 (only behind the warp field)
          d['points'] = torch.empty(B, s, 3, device=device)
          if warp_on:
            d['warped_points'] = torch.empty(B, s, 3, device=device)
        if name in jac_levels:   # models.py:264-265
          d['warp_jacobian'] = torch.empty(B, s, 3, 3, device=device)
      for k, t in d.items():
        setattr(lo, k, _ptr(t))
      ret[name] = d
    scal = _scalars(warp_extra)
    flags = self.flags(train, bf16, no_warp=self.use_warp and not warp_on, jacobian=bool(jac_levels), ray_grads=ray_grads, frozen=frozen)
    rec = self.last_call = self._record(B, flags, device)
    if train:
      self.stash = rec   # what `backward` differentiates (fp32 or bf16 layout), and the batch size it is for
    L.check(self.lib.nrf_forward(self.handle, _ptr(fp.flat), C.byref(rays), C.byref(scal), C.byref(rnd), C.byref(out), flags,
                                 *_ws_tail(rec.ws, stream)), self.lib)
    del keep, keep2
    return ret

  # ---- field queries: render_samples up to the activations (models.py:230-277) at the caller's points; gradient queries: the
  # density's slope and the surface normal there.  Two kinds, each with a plan, a workspace-cache key and an out struct of its own ----
  QUERY_OUTPUTS = ('sigma', 'rgb', 'warped_points')
  GRADIENT_OUTPUTS = ('sigma', 'grad_sigma', 'normals', 'warped_points')

  def _query_workspace(self, kind, num_groups, points_per_group, flags, device) -> torch.Tensor:
    """The workspace of a field query of `kind` ('query' / 'query_grad') from the cache of `_record` (keys of its own: a query has a
    plan of its own), sized by nrf_<kind>_workspace_bytes."""
    return self._workspace((kind, int(num_groups), int(points_per_group), str(device)), device,
                           getattr(self.lib, f'nrf_{kind}_workspace_bytes'), int(num_groups), int(points_per_group), flags)

  @staticmethod
  def _point_groups(points, device):
    """`points` (..., S, 3) -> (float32 contiguous points, the leading dimensions, their product G, S)."""
    pts = _f32(points, device)
    if pts.dim() < 2 or pts.shape[-1] != 3:
      raise L.NrfError(f'points must be (..., S, 3), got {tuple(pts.shape)}')
    lead, S = tuple(pts.shape[:-2]), pts.shape[-2]
    G = 1
    for n in lead:
      G *= n
    return pts, lead, G, S

  def _query_setup(self, variables, num_groups, metadata, warp_extra, level, use_warp, outputs, allowed, device):
    """What a query decides before its groups are known as a lib.Rays: (flat params, `metadata` as one row per group, scalars, flags,
    the level's index, the outputs as a tuple out of `allowed`)."""
    if level not in ('coarse', 'fine'):
      raise L.NrfError(f"level must be 'coarse' or 'fine', got {level!r}")
    outputs = _select_outputs(outputs, allowed)
    fp = self.flat_params(variables, device)
    rows = {}
    for k, v in (metadata or {}).items():   # one row per group, whatever leading dimensions the caller's points had
      v = torch.as_tensor(v, device=device)
      if v.numel() % num_groups or v.numel() == 0:
        raise L.NrfError(f'metadata[{k!r}] must have one row per group ({num_groups}), got shape {tuple(v.shape)}')
      rows[k] = v.reshape(num_groups, -1)
    return fp, rows, _scalars(warp_extra), self.flags(no_warp=self.use_warp and not use_warp), 1 if level == 'fine' else 0, outputs

  def _group_rays(self, num_groups, viewdirs, rows, metadata_encoded, device):
    """The lib.Rays of `num_groups` groups: a row of `viewdirs` and of every entry of `rows` (as `_query_setup` returns them, or a
    slice of whole groups) each; and the tensors it points into."""
    groups, keep = L.Rays(), []
    groups.num_rays = int(num_groups)
    if viewdirs is not None:
      vd = _f32(viewdirs, device).reshape(-1, 3)
      if vd.shape[0] != num_groups:
        raise L.NrfError(f'viewdirs must have one row per group ({num_groups}), got {vd.shape[0]}')
      groups.viewdirs = _ptr(vd)
      keep.append(vd)
    self._metadata_into(groups, rows, device, metadata_encoded, keep)
    return groups, keep

  def _grid_call(self, name, kind, entry, out_type, allowed, variables, origin, step, dims, first, count, out, viewdirs, metadata,
                 warp_extra, level, use_warp, metadata_encoded, workspace_points):
    """The public method `name`: points [first, first + count) of a grid through `entry`, into the tensors of `out`."""
    device = next(iter(out.values())).device
    fp, rows, scal, flags, lv, outputs = self._query_setup(variables, 1, metadata, warp_extra, level, use_warp, out, allowed, device)
    groups, keep = self._group_rays(1, viewdirs, rows, metadata_encoded, device)
    for k in outputs:   # what a grid call writes `count` points into
      _require_out(name, f'out[{k!r}]', out[k], (count,) if k == 'sigma' else (count, 3))
    fo = _out_struct(out_type, allowed, out)
    ws = self._query_workspace(kind, 1, max(int(workspace_points or 0), int(count)), flags, device)
    L.check(getattr(self.lib, entry)(self.handle, _ptr(fp.flat), C.byref(groups), C.byref(L.grid(origin, step, dims)), int(first),
                                     int(count), lv, C.byref(scal), flags, C.byref(fo), *_ws_tail(ws, _stream_arg(device))), self.lib)
    del keep
    return out

  def query_points(self, variables, points, viewdirs=None, metadata=None, warp_extra=None, level='fine', use_warp=True,
                   metadata_encoded=False, outputs=('sigma', 'rgb')):
    """The field at arbitrary points (nrf_query_points): condition inputs, the warp (unless use_warp=False: the points are then
    canonical points), posenc, the NeRF MLP of `level`, sigmoid(rgb), sigma_activation -- no noise, no compositing.
    `points`: (..., S, 3); the leading dimensions are flattened into G groups (an (N, 3) input is one group) whose S points share a
    row of `viewdirs` (G, 3) and of every `metadata` entry ((G, 1) ids, or (G, features) codes with metadata_encoded).  `outputs`
    selects among 'sigma' (activated density), 'rgb' and 'warped_points'; without 'rgb' the density-only kernel runs.  Returns a
    dict of device tensors shaped like points[..., 0] (with a trailing 3 for 'rgb' / 'warped_points')."""
    device, stream = _gpu_reader('points', points)
    pts, lead, G, S = self._point_groups(points, device)
    fp, rows, scal, flags, lv, outputs = self._query_setup(variables, G, metadata, warp_extra, level, use_warp, outputs,
                                                           self.QUERY_OUTPUTS, device)
    groups, keep = self._group_rays(G, viewdirs, rows, metadata_encoded, device)
    ret = {k: torch.empty(*lead, S, *(() if k == 'sigma' else (3,)), dtype=torch.float32, device=device) for k in outputs}
    fo = _out_struct(L.FieldOut, self.QUERY_OUTPUTS, ret)
    ws = self._query_workspace('query', G, S, flags, device)
    L.check(self.lib.nrf_query_points(self.handle, _ptr(fp.flat), C.byref(groups), _ptr(pts), S, lv, C.byref(scal), flags, C.byref(fo),
                                      *_ws_tail(ws, stream)), self.lib)
    del keep
    return ret

  def query_grid(self, variables, origin, step, dims, first, count, out, viewdirs=None, metadata=None, warp_extra=None, level='fine',
                 use_warp=True, metadata_encoded=False, workspace_points=None):
    """Points [first, first + count) of a regular grid (nrf_query_grid: point n = (i, j, k) with x fastest, coordinate
    origin + idx * step, formed on the device) into the preallocated tensors of `out` ({'sigma': (count,), 'rgb': (count, 3), ...}).
    One condition for the whole grid: `viewdirs` (3,) and the metadata rows of ONE group.  `workspace_points`: size the workspace
    for this many points (a caller that walks a grid in chunks passes its chunk size: one workspace serves every chunk)."""
    return self._grid_call('query_grid', 'query', 'nrf_query_grid', L.FieldOut, self.QUERY_OUTPUTS, variables, origin, step, dims, first,
                           count, out, viewdirs, metadata, warp_extra, level, use_warp, metadata_encoded, workspace_points)

  def query_gradient(self, variables, points, metadata=None, warp_extra=None, level='fine', use_warp=True, metadata_encoded=False,
                     outputs=('sigma', 'grad_sigma', 'normals')):
    """The density, its gradient with respect to `points` (through the warp field unless use_warp=False) and the surface normal
    -grad / |grad| (exactly 0 where the gradient vanishes) at arbitrary points: nrf_query_points_grad.  `points` (..., S, 3) is
    grouped as in `query_points`; no view direction is read.  `outputs` selects among 'sigma', 'grad_sigma', 'normals' and
    'warped_points'.  More than NRF_QUERY_GRAD_MAX_POINTS points run as chunks of whole groups (or, one group, of points) through
    one cached workspace.  Returns a dict of device tensors shaped like points[..., 0] (a trailing 3 for all but 'sigma')."""
    device, stream = _gpu_reader('points', points)
    pts, lead, G, S = self._point_groups(points, device)
    fp, rows, scal, flags, lv, outputs = self._query_setup(variables, G, metadata, warp_extra, level, use_warp, outputs,
                                                           self.GRADIENT_OUTPUTS, device)
    pts = pts.reshape(G, S, 3)
    ret = {k: torch.empty(G, S, *(() if k == 'sigma' else (3,)), dtype=torch.float32, device=device) for k in outputs}
    cap = L.NRF_QUERY_GRAD_MAX_POINTS
    if S <= cap:   # chunks of whole groups
      pieces = [(g0, ng, 0, S) for g0, ng in grid_chunks(G, cap // S)]
    elif G == 1:   # one long group: chunks of its points
      pieces = [(0, 1, s0, ns) for s0, ns in grid_chunks(S, cap)]
    else:
      raise L.NrfError(f'query_gradient: groups of more than NRF_QUERY_GRAD_MAX_POINTS = {cap} points are chunked only when there is one group')
    ws = self._query_workspace('query_grad', pieces[0][1], pieces[0][3], flags, device)   # the first piece is the largest
    for g0, ng, s0, ns in pieces:   # every slice below is contiguous: whole groups, or a run of the one group's points
      groups, keep = self._group_rays(ng, None, {k: v[g0:g0 + ng] for k, v in rows.items()}, metadata_encoded, device)
      fo = _out_struct(L.FieldGradOut, self.GRADIENT_OUTPUTS, {k: v[g0:g0 + ng, s0:s0 + ns] for k, v in ret.items()})
      L.check(self.lib.nrf_query_points_grad(self.handle, _ptr(fp.flat), C.byref(groups), _ptr(pts[g0:g0 + ng, s0:s0 + ns]), ns, lv,
                                             C.byref(scal), flags, C.byref(fo), *_ws_tail(ws, stream)), self.lib)
      del keep
    return {k: v.reshape(*lead, S, *v.shape[2:]) for k, v in ret.items()}

  def query_grid_gradient(self, variables, origin, step, dims, first, count, out, metadata=None, warp_extra=None, level='fine',
                          use_warp=True, metadata_encoded=False, workspace_points=None):
    """Points [first, first + count) of a regular grid (nrf_query_grid_grad; the grid of `query_grid`) into the preallocated tensors
    of `out` ({'sigma': (count,), 'grad_sigma': (count, 3), 'normals': (count, 3), ...}); count <= NRF_QUERY_GRAD_MAX_POINTS."""
    return self._grid_call('query_grid_gradient', 'query_grad', 'nrf_query_grid_grad', L.FieldGradOut, self.GRADIENT_OUTPUTS, variables,
                           origin, step, dims, first, count, out, None, metadata, warp_extra, level, use_warp, metadata_encoded,
                           workspace_points)

  def backward(self, variables, rays_dict, d_rgb_coarse=None, d_rgb_fine=None, grad_out: torch.Tensor = None, d_out=None,
               ray_grads=False):
    """VJP of the last `apply(..., train=True)` on the same rays: returns the flat parameter gradient.
    `d_out` = {'coarse': {...}, 'fine': {...}} carries a cotangent for any of 'rgb' (B,3), 'depth' (B,), 'acc' (B,),
    'weights' (B,S) and 'warped_points' (B,S,3) per level (nrf_backward_ex); what is absent (or None) counts as zero.
    'med_depth' is piecewise constant and has none.  `d_rgb_coarse` / `d_rgb_fine` are the 'rgb' entries, positionally.
    `ray_grads`: True, or an iterable of 'origins' / 'directions' / 'viewdirs' -- after `apply(..., train=True, ray_grads=True)`;
    returns (grad, {name: (B,3) gradient w.r.t. rays_dict[name]}) through nrf_backward_rays.  True asks for 'viewdirs' only where
    the model and the rays have them.  On a frozen stash (`apply(..., frozen=True)`) there is no parameter gradient: the call returns
    (None, {name: grad}) and `ray_grads` is required (the library refuses nrf_backward_ex with NRF_E_STATE)."""
    stash = self.stash
    if stash is None:
      raise L.NrfError('backward() needs a preceding apply(..., train=True)')
    device = torch.as_tensor(rays_dict['origins']).device
    fp = self.flat_params(variables, device)
    rays, keep = self._rays_struct(rays_dict, device)
    B = rays.num_rays
    if stash.num_rays != B:
      raise L.NrfError(f'backward(): the stashed forward was run on {stash.num_rays} rays, not {B}')
    ws = stash.ws   # the library also refuses a stash whose workspace plan was replaced by another call (NRF_E_STATE)
    frozen = bool(stash.flags & L.NRF_FLAG_FROZEN)   # no parameter gradient: NULL (a grad_out is the library's to refuse, NRF_E_STATE)
    grad = grad_out if grad_out is not None or frozen else torch.empty_like(fp.flat)
    og, keep2 = self._output_grads(d_out or {}, {'coarse': d_rgb_coarse, 'fine': d_rgb_fine}, B, device)
    tail = (_ptr(grad), *_ws_tail(ws, _stream(device)))
    if ray_grads:
      if ray_grads is True:
        ray_grads = ('origins', 'directions') + (('viewdirs',) if self.use_viewdirs and 'viewdirs' in rays_dict else ())
      rg_out, rg = _ray_grads_out('backward', ray_grads, None, B, device)
      L.check(self.lib.nrf_backward_rays(self.handle, _ptr(fp.flat), C.byref(rays), C.byref(og), C.byref(rg), *tail), self.lib)
    else:
      L.check(self.lib.nrf_backward_ex(self.handle, _ptr(fp.flat), C.byref(rays), C.byref(og), *tail), self.lib)
    del keep, keep2
    return (grad, rg_out) if ray_grads else grad

  def _output_grads(self, d_out, d_rgb, B, device):
    """lib.OutputGrads of a `backward(d_out=...)` dict.  Every buffer is read by the kernels at its full size, so the shapes are
    checked here."""
    S = {'coarse': self.num_coarse_samples, 'fine': self.num_coarse_samples + self.num_fine_samples}
    og, keep = L.OutputGrads(), []
    unknown = set(d_out) - set(S)
    if unknown or ('fine' in d_out and d_out['fine'] and self.num_fine_samples <= 0):
      raise L.NrfError(f"backward(d_out=...): levels {sorted(unknown) or ['fine']} do not exist in this model")
    for name, lg in (('coarse', og.coarse), ('fine', og.fine)):
      level = dict(d_out.get(name) or {})
      if d_rgb[name] is not None:
        if level.get('rgb') is not None:
          raise L.NrfError(f"backward(): the rgb cotangent of level {name!r} was given twice (positionally and in d_out)")
        level['rgb'] = d_rgb[name]
      shapes = {'rgb': (B, 3), 'depth': (B,), 'acc': (B,), 'weights': (B, S[name]), 'warped_points': (B, S[name], 3)}
      for key, t in level.items():
        if key not in shapes:
          raise L.NrfError(f"backward(d_out=...): {name}/{key} has no cotangent (differentiable outputs: {sorted(shapes)})")
        if t is None:
          continue
        t = _f32(t, device)
        if tuple(t.shape) != shapes[key]:
          raise L.NrfError(f"backward(d_out=...): {name}/{key} must have shape {shapes[key]}, got {tuple(t.shape)}")
        keep.append(t)
        setattr(lg, 'd_' + key, _ptr(t))
    return og, keep

  def loss_and_grad(self, fp: P.FlatParams, batch, warp_extra=None, rngs=None, grad_out=None, stats_out=None,
                    background=None, elastic=None, warp_reg=None, bf16=False, dynamic=None, ray_grads=None, ray_grads_out=None):
    """forward + MSE_coarse + MSE_fine [+ background regulariser] + backward in one library call
    (training.py:168-265).  `background` = dict(points (N,3) already noised, warp_ids (N,), weight, alpha=-2,
    scale=1e-3) adds weight * mean(general_loss(|warp(x) - x|^2)) (training.py:117-135, 248-259).
    Instead of 'warp_ids' the dict may carry `id_choices` (the model's warp ids) and `noise_std`: the library then draws the id
    per point and adds the noise itself (training.py:121-126), `points` being the raw points.  `dynamic`: the device buffer
    of a training.DynamicScalars -- warp_alpha / time_alpha / the rng key / the elastic weight are read from it on the device
    (a captured launch sequence stays valid when they change).
    `elastic` = dict(weight, reduce_method='weight', eps=1e-6, alpha=-2, scale=0.03) adds the elastic regulariser
    on the coarse samples (training.py:71-114, 177-197); `loss_type` in lib.ELASTIC_TYPE.  `warp_reg` = dict(weight,
    alpha=-2, scale=1e-3): training.py:199-212 on both levels.  `bf16`: bfloat16 MLP operands (NRF_FLAG_BF16).
    stats (lib.NRF_NUM_STATS floats) = [mse_c, mse_f, psnr_c, psnr_f, total, background_loss, loss/elastic,
    residual/elastic, warp_reg_c, warp_reg_f, warp_reg residual c, f, jacobian det, div, curl, 0].
    `ray_grads`: an iterable of 'origins' / 'directions' -- the call goes through nrf_train_step_loss_grad_rays (float32 mode
    only) and returns (grad, stats, {name: (B,3) gradient of MSE_coarse + MSE_fine w.r.t. batch[name]}); the regularisers
    add nothing to the rays.  A batch without 'viewdirs' on a use_viewdirs model: the view term is part of 'directions'.
    `ray_grads_out`: {name: (B,3) float32 tensor} to write into instead of fresh tensors."""
    if ray_grads is not None and bf16:
      raise L.NrfError('loss_and_grad(ray_grads=...): ray gradients are built for the float32 mode, not with bf16')
    device = fp.flat.device
    rays, keep = self._rays_struct(batch, device)
    rnd, keep2 = self._rand_struct(rngs, rays.num_rays, device)
    target = _f32(batch['rgb'], device)[..., :3].contiguous()
    grad = grad_out if grad_out is not None else torch.empty_like(fp.flat)
    stats = stats_out if stats_out is not None else torch.empty(L.NRF_NUM_STATS, device=device)
    scal = _scalars(warp_extra, dynamic)
    bg, nbg, keep3 = _background_struct(background, device)
    el, wr = _elastic_struct(elastic), _warp_reg_struct(warp_reg)
    flags = self.flags(True, bf16, ray_grads=ray_grads is not None)
    rec = self.stash = self.last_call = self._record(rays.num_rays, flags, device, nbg, el is not None)
    # each entry takes the word without the bits its ABI implies: _ex the bf16 bits, _rays (float32 only) none
    if ray_grads is None:
      entry, mid = self.lib.nrf_train_step_loss_grad_ex, (flags & ~L.NRF_FLAG_TRAIN,)
    else:
      rg_out, rg = _ray_grads_out('loss_and_grad', ray_grads, ray_grads_out, rays.num_rays, device, RAY_GRADS[:2],
                                  "the fused step returns 'origins' and 'directions'")
      entry, mid = self.lib.nrf_train_step_loss_grad_rays, (flags & ~(L.NRF_FLAG_TRAIN | L.NRF_FLAG_RAY_GRADS), C.byref(rg))
    L.check(entry(self.handle, _ptr(fp.flat), C.byref(rays), _ptr(target), C.byref(scal), C.byref(rnd), _ref(bg), _ref(el), _ref(wr), *mid,
                  _ptr(grad), _ptr(stats), *_ws_tail(rec.ws, _stream(device))), self.lib)
    del keep, keep2, keep3
    return (grad, stats) if ray_grads is None else (grad, stats, rg_out)

  def loss_and_ray_grads(self, fp: P.FlatParams, batch, warp_extra=None, rngs=None, ray_grads=('origins', 'directions'),
                         ray_grads_out=None, stats_out=None, dynamic=None):
    """The fused FROZEN step (nrf_loss_grad_rays): forward + MSE_coarse + MSE_fine + the reverse pass down to the rays, with the
    parameters fixed -- no parameter gradient, no regulariser, no activation stash.  Returns (stats, {name: (B,3) gradient w.r.t.
    batch[name]}) for the names in `ray_grads` ('origins', 'directions', 'viewdirs'); stats as `loss_and_grad` with the regulariser
    entries 0.  A batch without 'viewdirs' on a use_viewdirs model: the view term is part of 'directions'.  `ray_grads_out` /
    `stats_out`: tensors to write into (fixed addresses for a captured graph); `dynamic`: as `loss_and_grad`.  Float32 only."""
    device = fp.flat.device
    rays, keep = self._rays_struct(batch, device)
    rnd, keep2 = self._rand_struct(rngs, rays.num_rays, device)
    target = _f32(batch['rgb'], device)[..., :3].contiguous()
    stats = stats_out if stats_out is not None else torch.empty(L.NRF_NUM_STATS, device=device)
    scal = _scalars(warp_extra, dynamic)
    rg_out, rg = _ray_grads_out('loss_and_ray_grads', ray_grads, ray_grads_out, rays.num_rays, device)
    rec = self.stash = self.last_call = self._record(rays.num_rays, self.flags(True, ray_grads=True, frozen=True), device)
    L.check(self.lib.nrf_loss_grad_rays(self.handle, _ptr(fp.flat), C.byref(rays), _ptr(target), C.byref(scal), C.byref(rnd), C.byref(rg),
                                        _ptr(stats), *_ws_tail(rec.ws, _stream(device))), self.lib)
    del keep, keep2
    return stats, rg_out

  def warp_points(self, variables, points, warp_ids, warp_extra):
    """model.create_warp_field(model, num_batch_dims=1).apply(points, ids, warp_extra, False, False)
    ['warped_points'] (models.py:165-184, warping.py:355-389): (N,3) points, one warp id per point."""
    device = torch.as_tensor(points).device
    fp = self.flat_params(variables, device)
    pts = _f32(points, device).reshape(-1, 3)
    ids = _ids(warp_ids, device).reshape(-1)
    n = pts.shape[0]
    # no cache key: callers pass arbitrary point counts, and a workspace kept per count would only pile up
    ws = self._workspace(None, device, self.lib.nrf_warp_points_workspace_bytes, n)
    out = torch.empty(n, 3, device=device)
    scal = _scalars(warp_extra)
    L.check(self.lib.nrf_warp_points(self.handle, _ptr(fp.flat), _ptr(pts), _ptr(ids), n, C.byref(scal), _ptr(out),
                                     *_ws_tail(ws, _stream(device))), self.lib)
    return out.reshape(torch.as_tensor(points).shape)

  UNWARP_OUTPUTS = ('points', 'residual', 'status')

  def unwarp_points(self, variables, points, warp_ids, warp_extra, guess=None, steps=8, tolerance=0.0, max_step=float('inf'),
                    warp_codes=None, outputs=('points', 'residual', 'status')):
    """The warp field inverted (nrf_unwarp_points): x with warp_points(x, id) = `points`, canonical points (..., 3) with one warp id
    each, by `steps` Newton rounds on the device from `guess` (None: from the points themselves).  A row stops once its residual
    |W(x) - point| is <= `tolerance`; a step longer than `max_step` is shortened to it.  `warp_codes` (num_codes, features): the ids
    index ITS rows instead of the model's embedding table (in-between-frame codes).  `outputs` selects among 'points', 'residual'
    (at the returned x) and 'status' (int32: 0 ran out of steps, 1 converged, 2 stopped at a singular or non-finite step).  More
    than NRF_UNWARP_MAX_POINTS points run as chunks through one cached workspace.  Returns a dict of device tensors shaped like
    points[..., 0] (a trailing 3 for 'points')."""
    device, stream = _gpu_reader('points', points)
    outputs = _select_outputs(outputs, self.UNWARP_OUTPUTS)
    y = _f32(points, device)
    if y.dim() < 1 or y.shape[-1] != 3:
      raise L.NrfError(f'points must be (..., 3), got {tuple(y.shape)}')
    lead = tuple(y.shape[:-1])
    y = y.reshape(-1, 3)
    n = y.shape[0]
    ids = _ids(warp_ids, device).reshape(-1)
    if ids.numel() != n:
      raise L.NrfError(f'warp_ids must hold one id per point ({n}), got {ids.numel()}')
    x0 = None
    if guess is not None:
      x0 = _f32(guess, device).reshape(-1, 3)
      if x0.shape[0] != n:
        raise L.NrfError(f'guess must be shaped like points ({n} rows), got {x0.shape[0]}')
    codes = None if warp_codes is None else _f32(warp_codes, device).reshape(-1, self.num_warp_features)
    fp = self.flat_params(variables, device)
    scal = _scalars(warp_extra)
    ret = {k: torch.empty(n, *((3,) if k == 'points' else ()), dtype=torch.int32 if k == 'status' else torch.float32, device=device)
           for k in outputs}
    first = min(n, L.NRF_UNWARP_MAX_POINTS)   # the first chunk is the largest
    ws = self._workspace(('unwarp', first, str(device)), device, self.lib.nrf_unwarp_workspace_bytes, first)
    for r0, nr in grid_chunks(n, L.NRF_UNWARP_MAX_POINTS):
      r1 = r0 + nr
      uo = _out_struct(L.UnwarpOut, self.UNWARP_OUTPUTS, {k: v[r0:r1] for k, v in ret.items()})
      L.check(self.lib.nrf_unwarp_points(self.handle, _ptr(fp.flat), _ptr(y[r0:r1]), _ptr(ids[r0:r1]), _ptr(codes),
                                         0 if codes is None else codes.shape[0], None if x0 is None else _ptr(x0[r0:r1]), nr,
                                         C.byref(scal), int(steps), float(tolerance), float(max_step), C.byref(uo),
                                         *_ws_tail(ws, stream)), self.lib)
    return {k: v.reshape(*lead, *v.shape[1:]) for k, v in ret.items()}

  def profile_enable(self, on=True):
    L.check(self.lib.nrf_profile_enable(self.handle, int(bool(on))), self.lib)

  def profile_read(self):
    """[{name, ms, launches, flops_per_launch}] accumulated since the last read (device-side HIP events)."""
    n = C.c_int32(0)
    L.check(self.lib.nrf_profile_read(self.handle, None, C.byref(n)), self.lib)
    arr = (L.ProfileEntry * max(n.value, 1))()
    L.check(self.lib.nrf_profile_read(self.handle, arr, C.byref(n)), self.lib)
    return [dict(name=arr[i].name.decode(), ms=arr[i].ms, launches=arr[i].launches,
                 flops_per_launch=arr[i].flops_per_launch) for i in range(n.value)]

  def __del__(self):
    try:
      if self._handle is not None and self._lib is not None:
        self._lib.nrf_destroy(self._handle)
    except Exception:   # interpreter shutdown
      pass


def construct_nerf(key, config, batch_size: int, appearance_ids: Sequence[int], camera_ids: Sequence[int],
                   warp_ids: Sequence[int], near: float, far: float, use_warp_jacobian: bool = False,
                   use_weights: bool = False, device='cuda'):
  """models.construct_nerf (models.py:378-489): builds the model and reference-initialised params.

  `key` is an int seed.  `config` is any object with the ModelConfig attributes (configs.py:35-105).
  `batch_size` is accepted for signature parity (shape inference is not needed here)."""
  del batch_size
  g = lambda name, default=None: getattr(config, name, default)
  model = NerfModel(
      num_coarse_samples=g('num_coarse_samples', 64), num_fine_samples=g('num_fine_samples', 128),
      use_viewdirs=g('use_viewdirs', True), near=near, far=far, noise_std=g('noise_std'),
      nerf_trunk_depth=g('nerf_trunk_depth', 8), nerf_trunk_width=g('nerf_trunk_width', 256),
      nerf_rgb_branch_depth=g('nerf_rgb_branch_depth', 1), nerf_rgb_branch_width=g('nerf_rgb_branch_width', 128),
      nerf_skips=tuple(g('nerf_skips', (4,))), alpha_channels=g('alpha_channels', 1), rgb_channels=g('rgb_channels', 3),
      use_stratified_sampling=g('use_stratified_sampling', True), num_nerf_point_freqs=g('num_nerf_point_freqs', 10),
      num_nerf_viewdir_freqs=g('num_nerf_viewdir_freqs', 4), appearance_ids=appearance_ids, camera_ids=camera_ids,
      warp_ids=warp_ids, num_appearance_features=g('appearance_metadata_dims', 8),
      num_camera_features=g('camera_metadata_dims', 2), num_warp_features=g('num_warp_features', 8),
      num_warp_freqs=g('num_warp_freqs', 8), activation=g('activation', 'relu'),
      sigma_activation=g('sigma_activation', 'relu'), use_white_background=g('use_white_background', False),
      use_linear_disparity=g('use_linear_disparity', False), use_sample_at_infinity=g('use_sample_at_infinity', True),
      warp_field_type=g('warp_field_type', 'translation'),
      warp_metadata_encoder_type=g('warp_metadata_encoder_type', 'glo'),
      use_appearance_metadata=g('use_appearance_metadata', False), use_camera_metadata=g('use_camera_metadata', False),
      use_warp=g('use_warp', False), use_warp_jacobian=use_warp_jacobian, use_weights=use_weights,
      use_trunk_condition=g('use_trunk_condition', False),
      use_alpha_condition=g('use_alpha_condition', False), use_rgb_condition=g('use_rgb_condition', False),
      warp_kwargs=dict(g('warp_kwargs', {}) or {}))
  flat = P.init_flat(model.layout, int(key), device)
  return model, P.FlatParams(flat, model.layout)
