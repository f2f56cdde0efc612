"""NerfModel.apply as a differentiable PyTorch function of the flat parameter buffer.

`render_differentiable` runs `NerfModel.apply(train=True)` and returns the level dicts as tensors that carry a grad_fn: any
PyTorch loss built from 'rgb', 'depth', 'acc', 'weights' or 'warped_points' (depth supervision, a mask term on acc, distortion /
entropy terms on the weights, a regulariser on the warped points) back-propagates into the parameters through ONE
nrf_backward_ex call (include/nerfies_amd.h).  'med_depth', 'points' and 'z_vals' are returned without a gradient: the median
depth is piecewise constant, the sample points and depths do not depend on the parameters (the fine depths sit behind
stop_gradient, model_utils.py:187).  Out of scope: a cotangent of 'warp_jacobian' (its adjoint exists only inside the elastic
regulariser of the fused train step) and extra cotangents through the fused `loss_and_grad`, whose loss is fixed.

Rays: when rays['origins'], rays['directions'] or rays['viewdirs'] requires grad (camera pose / intrinsics refinement, per-frame pose
deltas, a learned lens correction), the call goes through `RayRenderFunction` instead: the forward sets NRF_FLAG_RAY_GRADS and the
backward is ONE nrf_backward_rays call that returns the parameter gradient and the three (B,3) ray gradients (float32 mode only).
viewdirs = d / |d| is the caller's own torch expression, so autograd carries d_viewdirs on to the directions.  The 'points' output
stays non-differentiable: rebuild o + z d from 'z_vals' in torch; a cotangent on 'warped_points' does reach the rays.  With no
requires_grad ray the call is the one above: same flag word, same launches."""
import torch
from torch.autograd.function import once_differentiable

from nerfies_amd import lib as L
from nerfies_amd import params as P

DIFFERENTIABLE = ('rgb', 'depth', 'acc', 'weights', 'warped_points')   # the rest: med_depth, points, z_vals


class RenderFunction(torch.autograd.Function):
  """forward: the rendered outputs of every level, flattened in the order of `ctx.keys`; backward: one nrf_backward_ex call on the
  stash the forward left, with whatever cotangents autograd delivers."""

  @staticmethod
  def forward(ctx, flat, model, rays, warp_extra, rngs, opts, keys):
    fp = P.FlatParams(flat.detach(), model.layout)
    out = model.apply({'params': fp}, rays, warp_extra, rngs=rngs, train=True, **opts)
    ctx.model, ctx.rays, ctx.fp = model, rays, fp
    ctx.stash = model._train_ws   # the stash this node differentiates: a later apply(train=True) replaces it
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
    if model._train_ws is not ctx.stash:
      raise L.NrfError('render_differentiable: another apply(train=True) / training step ran on this model since the forward; '
                       'its activation stash is gone -- call backward() before the next training forward')
    d_out = {}
    for (lv, k), g in zip(ctx.keys, grads):
      if g is not None and k in DIFFERENTIABLE:
        d_out.setdefault(lv, {})[k] = g
    grad = model.backward({'params': ctx.fp}, ctx.rays, d_out=d_out)
    return grad, None, None, None, None, None, None


RAY_KEYS = ('origins', 'directions', 'viewdirs')


class RayRenderFunction(torch.autograd.Function):
  """RenderFunction with the rays as differentiable inputs: forward under NRF_FLAG_RAY_GRADS, backward one nrf_backward_rays call."""

  @staticmethod
  def forward(ctx, flat, origins, directions, viewdirs, model, rays, warp_extra, rngs, opts, keys):
    fp = P.FlatParams(flat.detach(), model.layout)
    rays = dict(rays, origins=origins.detach(), directions=directions.detach())
    if viewdirs is not None:
      rays['viewdirs'] = viewdirs.detach()
    out = model.apply({'params': fp}, rays, warp_extra, rngs=rngs, train=True, ray_grads=True, **opts)
    ctx.model, ctx.rays, ctx.fp = model, rays, fp
    ctx.stash = model._train_ws
    ctx.set_materialize_grads(False)
    keys.extend((lv, k) for lv, d in out.items() for k in d)
    ctx.keys = list(keys)
    tensors = tuple(out[lv][k] for lv, k in ctx.keys)
    ctx.mark_non_differentiable(*(t for (lv, k), t in zip(ctx.keys, tensors) if k not in DIFFERENTIABLE))
    return tensors

  @staticmethod
  @once_differentiable
  def backward(ctx, *grads):
    model = ctx.model
    if model._train_ws is not ctx.stash:
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
    if want:
      grad, got = model.backward({'params': ctx.fp}, ctx.rays, d_out=d_out, ray_grads=want)
      rg.update(got)
    else:
      grad = model.backward({'params': ctx.fp}, ctx.rays, d_out=d_out)
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
  if any(_requires_grad(rays.get(k)) for k in RAY_KEYS):
    if bf16:
      raise L.NrfError(f"render_differentiable(bf16={bf16!r}): gradients w.r.t. the rays (NRF_FLAG_RAY_GRADS) exist in the float32 mode only")
    if model.use_viewdirs and rays.get('viewdirs') is None:
      # models.py:326-329: the condition then reads the directions themselves; named as the viewdirs input, their gradient
      # through the condition joins the one through the sample points in autograd's own sum
      rays = dict(rays, viewdirs=rays['directions'])
    tensors = RayRenderFunction.apply(flat, rays['origins'], rays['directions'], rays.get('viewdirs'), model, rays, warp_extra, rngs,
                                      opts, keys)
  else:
    tensors = RenderFunction.apply(flat, model, rays, warp_extra, rngs, opts, keys)
  out = {}
  for (lv, k), t in zip(keys, tensors):
    out.setdefault(lv, {})[k] = t
  return out

