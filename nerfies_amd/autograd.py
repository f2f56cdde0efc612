"""NerfModel.apply as a differentiable PyTorch function of the flat parameter buffer.

`render_differentiable` runs `NerfModel.apply(train=True)` and returns the level dicts as tensors that carry a grad_fn: any
PyTorch loss built from 'rgb', 'depth', 'acc', 'weights' or 'warped_points' (depth supervision, a mask term on acc, distortion /
entropy terms on the weights, a regulariser on the warped points) back-propagates into the parameters through ONE
nrf_backward_ex call (include/nerfies_amd.h).  'med_depth', 'points' and 'z_vals' are returned without a gradient: the median
depth is piecewise constant, the sample points and depths do not depend on the parameters (the fine depths sit behind
stop_gradient, model_utils.py:187).  Out of scope: a cotangent of 'warp_jacobian' (its adjoint exists only inside the elastic
regulariser of the fused train step) and extra cotangents through the fused `loss_and_grad`, whose loss is fixed.

Rays: when rays['origins'], rays['directions'] or rays['viewdirs'] requires grad (camera pose / intrinsics refinement, per-frame pose
deltas, a learned lens correction), they enter `RenderFunction` as inputs of their own: the forward sets NRF_FLAG_RAY_GRADS and the
backward is ONE nrf_backward_rays call that returns the parameter gradient and the three (B,3) ray gradients (float32 mode only).
viewdirs = d / |d| is the caller's own torch expression, so autograd carries d_viewdirs on to the directions.  The 'points' output
stays non-differentiable: rebuild o + z d from 'z_vals' in torch; a cotangent on 'warped_points' does reach the rays.  With no
requires_grad ray the call is the one above: same flag word, same launches.  When a ray requires grad and `flat_params` does not
(test-time pose alignment against a trained field), the forward runs under NRF_FLAG_FROZEN: no activation stash is written and the
backward stops at the rays (training.align_step / align_cameras are the fused form of that loop).

Cameras: the rays themselves come differentiably from a camera table (nerfies_amd.camera.pack_cameras, (C, 24) on the device) through
`CameraRaysFunction` (nrf_camera_table_rays / _rays_backward), world points go to pixels through `CameraProjectFunction`.  The
whole chain of a pose / intrinsics / lens refinement:

    table = pack_cameras(cameras).requires_grad_()
    origins, directions = rays_from_table(table, pixels, item_index)       # HIP, one table row per ray
    viewdirs = directions / directions.norm(dim=-1, keepdim=True)          # torch
    out = render_differentiable(model, flat, dict(batch, origins=origins, directions=directions, viewdirs=viewdirs))
    loss(out).backward()                                                   # nrf_backward_rays, then nrf_camera_table_rays_backward
    table.grad                                                             # (C, 24); the two pads of a row stay 0

The distortion coefficients of a camera whose coefficients are all zero receive a gradient as well, so a lens
correction can be learned from zero.  `CameraComposeFunction` (nerfies_amd.camera.compose_cameras) maps a per-camera delta table
(rotation vector, translation, log focal, principal point, distortion) onto a camera table, differentiably in the deltas; the fused
train step with ray gradients is `NerfModel.loss_and_grad(..., ray_grads=...)` / `training.train_step(cameras=...)`.  Out of scope: a
table form of pixels_to_points, the bf16 modes (ray gradients are float32 only)."""
import torch
from torch.autograd.function import once_differentiable

from nerfies_amd import lib as L
from nerfies_amd import params as P

DIFFERENTIABLE = ('rgb', 'depth', 'acc', 'weights', 'warped_points')   # the rest: med_depth, points, z_vals


RAY_KEYS = ('origins', 'directions', 'viewdirs')


class RenderFunction(torch.autograd.Function):
  """forward: the rendered outputs of every level, flattened in the order of `ctx.keys`; backward: one nrf_backward_ex call on the
  stash the forward left, with whatever cotangents autograd delivers.  `origins` / `directions` / `viewdirs` are the rays as
  differentiable inputs, or None for what `rays` holds: when one of them needs a gradient the forward runs under NRF_FLAG_RAY_GRADS
  and the backward is one nrf_backward_rays call instead; when `flat` needs none, under NRF_FLAG_FROZEN as well."""

  @staticmethod
  def forward(ctx, flat, origins, directions, viewdirs, model, rays, warp_extra, rngs, opts, keys):
    fp = P.FlatParams(flat.detach(), model.layout)
    rays = dict(rays, **{k: t.detach() for k, t in zip(RAY_KEYS, (origins, directions, viewdirs)) if t is not None})
    ray_grads = any(ctx.needs_input_grad[1:4])
    # a ray needs a gradient and the parameters do not (aligning a camera against a trained field): the forward runs frozen
    # (NRF_FLAG_FROZEN, no activation stash) and the backward asks for no parameter gradient
    out = model.apply({'params': fp}, rays, warp_extra, rngs=rngs, train=True, ray_grads=ray_grads,
                      frozen=ray_grads and not ctx.needs_input_grad[0], **opts)
    ctx.model, ctx.rays, ctx.fp = model, rays, fp
    ctx.stash = model.stash   # the stash this node differentiates: a later apply(train=True) replaces it
    ctx.set_materialize_grads(False)   # an output the loss does not read stays NULL for the library, not a buffer of zeros
    keys.extend((lv, k) for lv, d in out.items() for k in d)   # handed back to the caller: the order of the returned tuple
    ctx.keys = list(keys)
    tensors = tuple(out[lv][k] for lv, k in ctx.keys)
    ctx.mark_non_differentiable(*(t for (lv, k), t in zip(ctx.keys, tensors) if k not in DIFFERENTIABLE))
    return tensors

  @staticmethod
  @once_differentiable
  def backward(ctx, *grads):
    model = ctx.model
    if model.stash is not ctx.stash:
      raise L.NrfError('render_differentiable: another apply(train=True) / training step ran on this model since the forward; '
                       'its activation stash is gone -- call backward() before the next training forward')
    d_out = {}
    for (lv, k), g in zip(ctx.keys, grads):
      if g is not None and k in DIFFERENTIABLE:
        d_out.setdefault(lv, {})[k] = g
    # inputs 1..3 = origins, directions, viewdirs: only what autograd needs is asked of the library
    want = [k for i, k in enumerate(RAY_KEYS) if ctx.needs_input_grad[1 + i]]
    rg = {}
    if 'viewdirs' in want and not model.use_viewdirs:   # a model without viewdirs never reads them
      want.remove('viewdirs')
      rg['viewdirs'] = torch.zeros_like(ctx.rays['viewdirs'])
    grad = model.backward({'params': ctx.fp}, ctx.rays, d_out=d_out, ray_grads=want)
    if want:
      grad, got = grad
      rg.update(got)
    return (grad if ctx.needs_input_grad[0] else None,) + tuple(rg.get(k) for k in RAY_KEYS) + (None,) * 6


def _requires_grad(t):
  return isinstance(t, torch.Tensor) and t.requires_grad


def render_differentiable(model, flat_params, rays, warp_extra=None, rngs=None, *, return_weights=False, return_points=False,
                          return_z_vals=False, bf16=False):
  """{'coarse': {...}, 'fine': {...}} of `model.apply(train=True)` as differentiable tensors of `flat_params` (a float32 tensor
  of model.layout.total elements on the GPU, usually requires_grad; a params.FlatParams is taken by its `.flat`).
  `bf16`: False, True or 'mlp' -- the training modes of the library; 'x3' is inference-only and refused.
  One pending backward per model: the activation stash belongs to the model's last training forward."""
  if bf16 in ('x3', 'x3mlp'):
    raise L.NrfError(f"render_differentiable(bf16={bf16!r}): the split-bf16 mode is inference-only (no activation stash); "
                     "use False, True or 'mlp'")
  flat = flat_params.flat if isinstance(flat_params, P.FlatParams) else flat_params
  opts = dict(return_weights=return_weights, return_points=return_points, return_z_vals=return_z_vals, bf16=bf16)
  keys = []
  ray_inputs = (None, None, None)
  if any(_requires_grad(rays.get(k)) for k in RAY_KEYS):
    if bf16:
      raise L.NrfError(f"render_differentiable(bf16={bf16!r}): gradients w.r.t. the rays (NRF_FLAG_RAY_GRADS) exist in the float32 mode only")
    if model.use_viewdirs and rays.get('viewdirs') is None:
      # models.py:326-329: the condition then reads the directions themselves; named as the viewdirs input, their gradient
      # through the condition joins the one through the sample points in autograd's own sum
      rays = dict(rays, viewdirs=rays['directions'])
    ray_inputs = tuple(rays.get(k) for k in RAY_KEYS)
  tensors = RenderFunction.apply(flat, *ray_inputs, model, rays, warp_extra, rngs, opts, keys)
  out = {}
  for (lv, k), t in zip(keys, tensors):
    out.setdefault(lv, {})[k] = t
  return out


_camera_ws = {}   # device -> the cached workspace of the camera-table reverse passes


def _camera_workspace(lib, n, num_cameras, device):
  import ctypes as C
  need = C.c_size_t(0)
  L.check(lib.nrf_camera_table_workspace_bytes(n, num_cameras, C.byref(need)), lib)
  ws = _camera_ws.get(device)
  if ws is None or ws.numel() < need.value:
    ws = _camera_ws[device] = torch.empty(need.value, dtype=torch.uint8, device=device)
  return ws


def _ptr(t):
  return t.data_ptr() if t is not None else None


def _table_args(table, x, last, camera_index):
  """-> (table, x flattened to [n, last], index flattened to [n] or None, batch shape), validated."""
  if table.dim() != 2 or table.shape[1] != L.NRF_CAMERA_ROW or table.dtype != torch.float32 or not table.is_cuda:
    raise ValueError(f'a camera table is a float32 CUDA tensor (C, {L.NRF_CAMERA_ROW}) (see pack_cameras)')
  if x.shape[-1] != last or x.dtype != torch.float32 or x.device != table.device:
    raise ValueError(f'expected a float32 [..., {last}] tensor on the device of the table')
  batch = tuple(x.shape[:-1])
  n = 1
  for b in batch:
    n *= b
  if camera_index is not None:
    if camera_index.dtype != torch.int32 or camera_index.device != table.device or camera_index.numel() != n:
      raise ValueError('camera_index must be an int32 tensor on the device of the table with one entry per ray')
    camera_index = camera_index.reshape(-1).contiguous()
  return table, x.reshape(-1, last), camera_index, batch


class CameraRaysFunction(torch.autograd.Function):
  """(table (C,24), pixels (n,2), camera_index (n,) or None) -> (origins, directions): nrf_camera_table_rays; backward: one
  nrf_camera_table_rays_backward call."""

  @staticmethod
  def forward(ctx, table, pixels, camera_index):
    lib = L.load_library()
    table, pixels = table.detach().contiguous(), pixels.detach().contiguous()
    n = pixels.shape[0]
    origins = torch.empty((n, 3), dtype=torch.float32, device=table.device)
    directions = torch.empty((n, 3), dtype=torch.float32, device=table.device)
    with torch.cuda.device(table.device):
      L.check(lib.nrf_camera_table_rays(table.data_ptr(), table.shape[0], _ptr(camera_index), pixels.data_ptr(), n,
                                        origins.data_ptr(), directions.data_ptr(), torch.cuda.current_stream().cuda_stream), lib)
    ctx.save_for_backward(table, pixels, camera_index)
    ctx.set_materialize_grads(False)   # an unused d_origins reaches the library as NULL
    return origins, directions

  @staticmethod
  @once_differentiable
  def backward(ctx, d_origins, d_directions):
    table, pixels, camera_index = ctx.saved_tensors
    lib = L.load_library()
    n = pixels.shape[0]
    d_origins = d_origins.contiguous().float() if d_origins is not None else None
    d_directions = d_directions.contiguous().float() if d_directions is not None else None
    d_table = torch.empty_like(table)
    d_pixels = torch.empty_like(pixels) if ctx.needs_input_grad[1] else None
    with torch.cuda.device(table.device):
      ws = _camera_workspace(lib, n, table.shape[0], table.device)
      L.check(lib.nrf_camera_table_rays_backward(table.data_ptr(), table.shape[0], _ptr(camera_index), pixels.data_ptr(), n,
                                                 _ptr(d_origins), _ptr(d_directions), d_table.data_ptr(), _ptr(d_pixels),
                                                 ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream), lib)
    return (d_table if ctx.needs_input_grad[0] else None), d_pixels, None


class CameraProjectFunction(torch.autograd.Function):
  """(table (C,24), points (n,3), camera_index (n,) or None) -> pixels (n,2): nrf_camera_table_project; backward: one
  nrf_camera_table_project_backward call."""

  @staticmethod
  def forward(ctx, table, points, camera_index):
    lib = L.load_library()
    table, points = table.detach().contiguous(), points.detach().contiguous()
    n = points.shape[0]
    pixels = torch.empty((n, 2), dtype=torch.float32, device=table.device)
    with torch.cuda.device(table.device):
      L.check(lib.nrf_camera_table_project(table.data_ptr(), table.shape[0], _ptr(camera_index), points.data_ptr(), n,
                                           pixels.data_ptr(), torch.cuda.current_stream().cuda_stream), lib)
    ctx.save_for_backward(table, points, camera_index)
    ctx.set_materialize_grads(False)
    return pixels

  @staticmethod
  @once_differentiable
  def backward(ctx, d_pixels):
    table, points, camera_index = ctx.saved_tensors
    if d_pixels is None:
      return None, None, None
    lib = L.load_library()
    n = points.shape[0]
    d_pixels = d_pixels.contiguous().float()
    d_table = torch.empty_like(table)
    d_points = torch.empty_like(points) if ctx.needs_input_grad[1] else None
    with torch.cuda.device(table.device):
      ws = _camera_workspace(lib, n, table.shape[0], table.device)
      L.check(lib.nrf_camera_table_project_backward(table.data_ptr(), table.shape[0], _ptr(camera_index), points.data_ptr(), n,
                                                    d_pixels.data_ptr(), d_table.data_ptr(), _ptr(d_points), ws.data_ptr(),
                                                    ws.numel(), torch.cuda.current_stream().cuda_stream), lib)
    return (d_table if ctx.needs_input_grad[0] else None), d_points, None


def camera_rays(table, pixels, camera_index=None):
  """nerfies_amd.camera.rays_from_table."""
  table, px, idx, batch = _table_args(table, pixels, 2, camera_index)
  origins, directions = CameraRaysFunction.apply(table, px, idx)
  return origins.reshape(batch + (3,)), directions.reshape(batch + (3,))


def camera_project(table, points, camera_index=None):
  """nerfies_amd.camera.project_from_table."""
  table, pts, idx, batch = _table_args(table, points, 3, camera_index)
  return CameraProjectFunction.apply(table, pts, idx).reshape(batch + (2,))


def camera_project_depth(table, points, camera_index=None):
  """nerfies_amd.camera.project_depth_from_table: nrf_camera_table_project_depth, which has no reverse pass."""
  table, pts, idx, batch = _table_args(table, points, 3, camera_index)
  lib = L.load_library()
  table, pts = table.detach().contiguous(), pts.detach().contiguous()
  n = pts.shape[0]
  screen = torch.empty((n, 3), dtype=torch.float32, device=table.device)
  with torch.cuda.device(table.device):
    L.check(lib.nrf_camera_table_project_depth(table.data_ptr(), table.shape[0], _ptr(idx), pts.data_ptr(), n, screen.data_ptr(),
                                               torch.cuda.current_stream().cuda_stream), lib)
  return screen.reshape(batch + (3,))


class CameraComposeFunction(torch.autograd.Function):
  """(table (C,24), deltas (C,16)) -> the composed table (C,24): nrf_camera_table_compose; backward: one
  nrf_camera_table_compose_backward call into the deltas (the base table carries no gradient)."""

  @staticmethod
  def forward(ctx, table, deltas):
    lib = L.load_library()
    table, deltas = table.detach().contiguous(), deltas.detach().contiguous()
    out = torch.empty_like(table)
    with torch.cuda.device(table.device):
      L.check(lib.nrf_camera_table_compose(table.data_ptr(), deltas.data_ptr(), table.shape[0], out.data_ptr(),
                                           torch.cuda.current_stream().cuda_stream), lib)
    ctx.save_for_backward(table, deltas)
    return out

  @staticmethod
  @once_differentiable
  def backward(ctx, d_out):
    table, deltas = ctx.saved_tensors
    lib = L.load_library()
    d_out = d_out.contiguous().float()
    d_deltas = torch.empty_like(deltas)
    with torch.cuda.device(table.device):
      L.check(lib.nrf_camera_table_compose_backward(table.data_ptr(), deltas.data_ptr(), table.shape[0], d_out.data_ptr(),
                                                    d_deltas.data_ptr(), torch.cuda.current_stream().cuda_stream), lib)
    return None, d_deltas


def camera_compose(table, deltas):
  """nerfies_amd.camera.compose_cameras."""
  if table.dim() != 2 or table.shape[1] != L.NRF_CAMERA_ROW or table.dtype != torch.float32 or not table.is_cuda:
    raise ValueError(f'a camera table is a float32 CUDA tensor (C, {L.NRF_CAMERA_ROW}) (see pack_cameras)')
  if tuple(deltas.shape) != (table.shape[0], L.NRF_CAMERA_DELTA_ROW) or deltas.dtype != torch.float32 or deltas.device != table.device:
    raise ValueError(f'a delta table is a float32 tensor ({table.shape[0]}, {L.NRF_CAMERA_DELTA_ROW}) on the device of the camera table')
  return CameraComposeFunction.apply(table, deltas)
