"""nrf_backward_rays / NerfModel.backward(ray_grads=...) / nerfies_amd.autograd with requires_grad rays: the gradients of the rendered
outputs w.r.t. the ray origins, directions and viewdirs (NRF_FLAG_RAY_GRADS, float32 mode).

The float64 reference is torch.autograd over oracle.nerf_model_apply with requires_grad rays, on the HIP path's own ReLU pattern and
fine depths (the masks are read from the stash of the ray-gradient forward itself, model.stash).  Each of the three tensors has to
lie within helpers.grad_tol of its oracle max-abs.  The directions are 1.7 x a unit vector while the viewdirs stay unit, so the |d|
factor of the compositing distances (model_utils.py:104-110) cannot go missing; shapes as tests/test_gpu_backward_ex.py: B = 7 leaves
a 4-rays-per-block remainder, 80 fine samples are two 64-lane chunks per ray, 16 + 16 samples with the warp keep the tangent pass small."""
import functools
import itertools

import numpy as np
import pytest
import torch

import helpers as H
from oracle import nerfies_oracle as O

pytestmark = pytest.mark.gpu

NRF_E_UNSUPPORTED, NRF_E_STATE = -3, -6   # include/nerfies_amd.h
B = 7
SHAPE = dict(num_coarse_samples=24, num_fine_samples=56, nerf_trunk_width=64, num_nerf_point_freqs=4, use_stratified_sampling=False)
WARP_SHAPE = dict(num_coarse_samples=16, num_fine_samples=16, nerf_trunk_width=64, num_nerf_point_freqs=4, use_stratified_sampling=False,
                  use_warp=True, num_warp_freqs=4)
OUTPUTS = ('rgb', 'depth', 'acc', 'weights')
RAYS = ('origins', 'directions', 'viewdirs')


def _batch(nrays, seed, dtype):
  b = O.synthetic_batch(nrays, seed=seed, dtype=dtype)
  b['viewdirs'] = b['directions'].clone()   # unit
  b['directions'] = b['directions'] * 1.7
  return b


def _cotangents(spec, nrays, keys, seed):
  g = torch.Generator().manual_seed(seed)
  S = {'coarse': spec.num_coarse_samples, 'fine': spec.num_coarse_samples + spec.num_fine_samples}
  shape = lambda lv: {'rgb': (nrays, 3), 'depth': (nrays,), 'acc': (nrays,), 'weights': (nrays, S[lv]), 'warped_points': (nrays, S[lv], 3)}
  return {lv: {k: torch.randn(*shape(lv)[k], generator=g, dtype=torch.float64) for k in keys} for lv in ('coarse', 'fine')}


def _to_gpu(cot):
  return {lv: {k: t.float().to(H.DEV) for k, t in d.items()} for lv, d in cot.items()}


def _stash_masks(model, spec, num_rays):
  """helpers.gpu_relu_masks on the stash of the last training forward, whatever flags it ran under (that helper looks the workspace
  up by the key of a plain training call)."""
  ws = model.stash.ws
  torch.cuda.synchronize()
  masks = {}
  for name, lv, rows in (('coarse', 0, num_rays * spec.num_coarse_samples),
                         ('fine', 1, num_rays * (spec.num_coarse_samples + spec.num_fine_samples))):
    nt = (rows + 63) // 64
    m = H._decode_bits(H._ws_words(model, ws, 'bits_trunk', lv, nt * 4 * 128 * 8), 8, nt, 2, rows)
    masks[f'{name}/MLP_0'] = [m[l][:, :spec.nerf_trunk_width] for l in H.trunk_layer_map(spec)]
    m = H._decode_bits(H._ws_words(model, ws, 'bits_rgbh', lv, nt * 4 * 64), 1, nt, 1, rows)
    masks[f'{name}/MLP_1'] = [m[0][:, :spec.nerf_rgb_branch_width]]
    if nx := spec.nerf_rgb_branch_depth - 1:   # rgb layers 1.. (as tests/test_gpu_rgb_branch_depth.py decodes them)
      m = H._decode_bits(H._ws_words(model, ws, 'bits_rgbx', lv, nx * nt * 4 * 64), nx, nt, 1, rows)
      masks[f'{name}/MLP_1'] += [m[i][:, :spec.nerf_rgb_branch_width] for i in range(nx)]
    if spec.use_warp:
      m = H._decode_bits(H._ws_words(model, ws, 'w_bits', lv, nt * 4 * 64 * 6), 6, nt, 1, rows)
      masks[f'{name}/warp'] = [m[l][:, :getattr(spec, 'warp_trunk_width', 128)] for l in range(6)]
  return masks


class PinnedRays:
  """One stashed ray-gradient forward on the GPU and the float64 oracle pinned to its ReLU pattern and fine depths, the rays as
  requires_grad leaves next to the parameters."""

  def __init__(self, spec, nrays, seed, alpha=0.0, time_alpha=0.0, tile_rows=0, params=None, batch=None):
    self.spec, self.nrays = spec, nrays
    self.warp_extra = {'alpha': alpha, 'time_alpha': time_alpha}
    self.p64 = params if params is not None else O.init_params(spec, seed=seed, trained_like=True, dtype=torch.float64)
    self.b64 = batch if batch is not None else _batch(nrays, seed + 1, torch.float64)
    self.model, self.fp = H.gpu_model(spec, self.p64, nrays)
    if tile_rows:
      self.model.set_chain_tile_rows(tile_rows)
    self.gb = H.gpu_batch(self.b64)
    out = self.model.apply({'params': self.fp}, self.gb, self.warp_extra, train=True, ray_grads=True, return_weights=True,
                           return_z_vals=True)
    torch.cuda.synchronize()
    self.hook = H.PinnedRelu(_stash_masks(self.model, spec, nrays))
    z_fine = out['fine']['z_vals'].cpu().double()
    self.req = {k: self.b64[k].clone().requires_grad_(True) for k in RAYS}
    with O.relu_hook(self.hook):
      self.ret = O.nerf_model_apply(self.p64, spec, dict(self.b64, **self.req), warp_alpha=alpha, time_alpha=time_alpha,
                                    fixed_fine_z=z_fine, return_points=spec.use_warp)
    for lv in ('coarse', 'fine'):   # the two forwards agree, so the pinned comparison is of one function
      for k in OUTPUTS:
        np.testing.assert_allclose(out[lv][k].cpu().numpy(), self.ret[lv][k].detach().numpy(), atol=1e-4, err_msg=f'{lv}/{k}')
    assert self.hook.flips <= H.FLIP_FRACTION * self.hook.total, (self.hook.flips, self.hook.total)

  def oracle(self, cot, names=RAYS):
    loss = sum((self.ret[lv][k] * t).sum() for lv, d in cot.items() for k, t in d.items())
    grads = torch.autograd.grad(loss, [self.req[k] for k in names], allow_unused=True, retain_graph=True)
    return {k: (g if g is not None else torch.zeros_like(self.req[k])) for k, g in zip(names, grads)}

  def gpu(self, cot, names=True):
    return self.model.backward({'params': self.fp}, self.gb, d_out=_to_gpu(cot), ray_grads=names)

  def compare(self, cot, label, names=RAYS, nonzero=RAYS):
    want = self.oracle(cot, names)
    _, got = self.gpu(cot, names)
    tol = H.grad_tol(self.spec)
    for k in names:
      scale = want[k].abs().max().item()
      err = (got[k].cpu().double() - want[k]).abs().max().item() / max(scale, 1e-30)
      print(f'[{label}] d {k}: oracle max-abs {scale:.3e}, error / max-abs {err:.2e} (tolerance {tol:.0e})')
      if k in nonzero:
        assert scale > 0, (label, k)
      assert err < tol, (label, k, err, scale)
    return want, got


@functools.lru_cache(maxsize=None)
def _case(white, inf, act):
  return PinnedRays(O.ModelSpec(use_white_background=white, use_sample_at_infinity=inf, sigma_activation=act, **SHAPE), B, seed=31)


@pytest.mark.parametrize('white,inf,act', list(itertools.product((False, True), (False, True), ('relu', 'softplus'))))
def test_oracle_parity_without_the_warp(white, inf, act):
  r = _case(white, inf, act)
  cot = _cotangents(r.spec, B, OUTPUTS, seed=5)
  r.compare(cot, f'white={white} inf={inf} {act}: rgb + depth + acc + weights')
  r.compare({lv: {'rgb': d['rgb']} for lv, d in cot.items()}, f'white={white} inf={inf} {act}: rgb alone')


@functools.lru_cache(maxsize=None)
def _warp_case(field, encoder='glo'):
  spec = O.ModelSpec(warp_field_type=field, warp_metadata_encoder_type=encoder, **WARP_SHAPE)
  return PinnedRays(spec, 5, seed=41, alpha=2.5, time_alpha=1.5 if encoder == 'time' else 0.0)


@pytest.mark.parametrize('field,encoder', [('se3', 'glo'), ('translation', 'glo'), ('se3', 'time')])
def test_oracle_parity_with_the_warp_field(field, encoder):
  """g_s = the NeRF MLP's d points + the caller's warped_points cotangent, carried to the rays through the stored warp Jacobians."""
  r = _warp_case(field, encoder)
  # neither cotangent reads the colour, so d viewdirs is zero on both sides
  r.compare(_cotangents(r.spec, 5, ('warped_points', 'depth'), seed=6), f'{field} / {encoder}: warped_points + depth',
            nonzero=('origins', 'directions'))
  # ... and with the colour too: d viewdirs of a plan with the warp field
  r.compare(_cotangents(r.spec, 5, ('warped_points', 'depth', 'rgb'), seed=6), f'{field} / {encoder}: warped_points + depth + rgb')


def test_chain_tile_rows_32_is_followed_in_the_forward_only():
  """NRF_OPT_CHAIN_TILE_ROWS = 32 with the flag on a model without a warp field is not refused: the forward stashes on 32-row half
  tiles, the reverse pass runs the 64-row chain (the one with the d-points section) over that stash -- what a model with a warp field
  does under the option.  B = 7 x (24 | 80) samples = 3 and 9 tiles, the last one partly filled."""
  spec = O.ModelSpec(use_white_background=True, **SHAPE)
  r = PinnedRays(spec, B, seed=31, tile_rows=32)
  r.compare(_cotangents(spec, B, OUTPUTS, seed=5), 'tile rows 32: rgb + depth + acc + weights')
  # the same model under the option without the flag still plans the 32-row reverse chain, and its parameter gradient agrees
  cot = _to_gpu(_cotangents(spec, B, OUTPUTS, seed=5))
  g_rays, _ = r.gpu(_cotangents(spec, B, OUTPUTS, seed=5))
  g_rays = g_rays.clone()
  r.model.apply({'params': r.fp}, r.gb, r.warp_extra, train=True)
  g_plain = r.model.backward({'params': r.fp}, r.gb, d_out=cot)
  scale = g_plain.abs().max().item()
  assert scale > 0 and (g_rays - g_plain).abs().max().item() <= 2e-5 * scale   # two tilings: equal to the order of the float sums


def test_deep_rgb_branch_carries_d_viewdirs():
  """nerf_rgb_branch_depth = 2: dray is still the adjoint of the FIRST rgb layer's pre-activation (the reverse chain walks layers
  nx..1 before it forms the per-ray sums), which is what the viewdir rows of that layer's kernel multiply."""
  spec = O.ModelSpec(nerf_rgb_branch_depth=2, use_white_background=True, **SHAPE)
  r = PinnedRays(spec, B, seed=71)
  r.compare(_cotangents(spec, B, OUTPUTS, seed=8), 'rgb branch depth 2: rgb + depth + acc + weights')


def test_model_without_viewdirs():
  spec = O.ModelSpec(use_viewdirs=False, use_white_background=True, **SHAPE)
  r = PinnedRays(spec, B, seed=51)
  cot = _cotangents(spec, B, OUTPUTS, seed=5)
  from nerfies_amd import lib as L
  with pytest.raises(L.NrfError, match=f'error {NRF_E_UNSUPPORTED}: .*d_viewdirs'):
    r.gpu(cot, RAYS)
  r.compare(cot, 'use_viewdirs=False', names=('origins', 'directions'), nonzero=('origins', 'directions'))   # the refusal left the stash usable
  _, got = r.gpu(cot, True)   # True asks for what the model has
  assert sorted(got) == ['directions', 'origins']


def _nocond():
  """As tests/test_gpu_backward_ex.py::_nocond: without a per-ray condition no float atomic feeds a gradient, so bit identity is sound."""
  spec = O.ModelSpec(use_viewdirs=False, use_white_background=True, **SHAPE)
  p32 = O.init_params(spec, seed=51, trained_like=True, dtype=torch.float32)
  model, fp = H.gpu_model(spec, p32, B)
  return spec, model, fp, H.gpu_batch(_batch(B, 52, torch.float32))


def test_parameter_gradient_is_nrf_backward_ex_and_calls_repeat_bit_for_bit():
  from nerfies_amd import lib as L
  spec, model, fp, gb = _nocond()
  cot = _to_gpu(_cotangents(spec, B, OUTPUTS, seed=7))
  model.apply({'params': fp}, gb, {}, train=True, ray_grads=True)
  ex = model.backward({'params': fp}, gb, d_out=cot).clone()   # nrf_backward_ex on the ray-gradient stash
  g1, r1 = model.backward({'params': fp}, gb, d_out=cot, ray_grads=True)
  g1, r1 = g1.clone(), {k: t.clone() for k, t in r1.items()}
  g2, r2 = model.backward({'params': fp}, gb, d_out=cot, ray_grads=True)
  assert ex.abs().max().item() > 0 and torch.equal(g1, ex) and torch.equal(g2, ex)
  for k in ('origins', 'directions'):
    assert r1[k].abs().max().item() > 0 and torch.equal(r1[k], r2[k]), k
  # ... and the same parameter gradient as a stash kept without the flag gives
  model.apply({'params': fp}, gb, {}, train=True)
  assert torch.equal(model.backward({'params': fp}, gb, d_out=cot), ex)
  with pytest.raises(L.NrfError, match=f'error {NRF_E_STATE}: .*NRF_FLAG_RAY_GRADS'):   # that stash holds nothing of the rays' gradient
    model.backward({'params': fp}, gb, d_out=cot, ray_grads=True)


def test_autograd_routes_gradients_to_the_rays(monkeypatch):
  from nerfies_amd import autograd, lib as L
  r = _case(True, True, 'softplus')
  model, fp = r.model, r.fp
  flat = fp.flat.clone().requires_grad_(True)
  rays = dict(r.gb, origins=r.gb['origins'].clone().requires_grad_(True))
  target = torch.linspace(0.1, 0.7, B, device=H.DEV)
  out = autograd.render_differentiable(model, flat, rays, {}, return_z_vals=True)
  assert not out['fine']['z_vals'].requires_grad and out['fine']['depth'].requires_grad
  ((out['fine']['depth'] - target) ** 2).sum().backward()
  with torch.no_grad():
    d_out = {'fine': {'depth': 2.0 * (out['fine']['depth'] - target)}}
  grad, rg = model.backward({'params': fp}, r.gb, d_out=d_out, ray_grads=('origins',))   # the wrapper's stash is still the model's last
  assert rays['origins'].grad.abs().max().item() > 0 and torch.equal(rays['origins'].grad, rg['origins'])
  np.testing.assert_allclose(flat.grad.cpu().numpy(), grad.cpu().numpy(), rtol=0, atol=2e-5 * grad.abs().max().item())
  # directions -> viewdirs = d / |d| in torch: autograd adds the two paths
  d = r.gb['directions'].clone().requires_grad_(True)
  out = autograd.render_differentiable(model, flat, dict(r.gb, directions=d, viewdirs=d / d.norm(dim=-1, keepdim=True)), {})
  out['fine']['rgb'].sum().backward()
  assert d.grad is not None and torch.isfinite(d.grad).all() and d.grad.abs().max().item() > 0
  # no requires_grad ray: the parent's flag word
  seen = []
  real = model.lib.nrf_forward

  def spy(*a):   # (handle, params, rays, scalars, rand, outputs, flags, ...)
    seen.append(int(a[6]))
    return real(*a)
  monkeypatch.setattr(model.lib, 'nrf_forward', spy)
  autograd.render_differentiable(model, flat, r.gb, {})
  autograd.render_differentiable(model, flat, rays, {})
  assert seen == [L.NRF_FLAG_TRAIN, L.NRF_FLAG_TRAIN | L.NRF_FLAG_RAY_GRADS], seen


def test_graph_replay_equals_eager():
  """One forward + nrf_backward_rays captured into a hipGraph and replayed (no allocation, no synchronisation in either)."""
  spec = O.ModelSpec(use_white_background=True, **SHAPE)
  p32 = O.init_params(spec, seed=61, trained_like=True, dtype=torch.float32)
  model, fp = H.gpu_model(spec, p32, B)
  gb = H.gpu_batch(_batch(B, 62, torch.float32))
  cot = _to_gpu(_cotangents(spec, B, OUTPUTS, seed=10))
  grad = torch.zeros_like(fp.flat)

  def step(out=None):
    out = model.apply({'params': fp}, gb, {}, train=True, ray_grads=True, return_weights=True, out=out)
    _, rg = model.backward({'params': fp}, gb, grad_out=grad, d_out=cot, ray_grads=True)
    return out, rg

  s = torch.cuda.Stream()
  s.wait_stream(torch.cuda.current_stream())
  with torch.cuda.stream(s):
    out, rg = step()
  torch.cuda.current_stream().wait_stream(s)
  torch.cuda.synchronize()
  eager = {k: t.clone() for k, t in rg.items()}
  eager_grad = grad.clone()
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph):
    _, rg = step(out)
  for t in rg.values():
    t.zero_()
  grad.zero_()
  graph.replay()
  torch.cuda.synchronize()
  assert sorted(rg) == sorted(RAYS)
  for k, y in eager.items():
    scale = y.abs().max().item()
    assert scale > 0 and (rg[k] - y).abs().max().item() <= 2e-5 * scale, (k, (rg[k] - y).abs().max().item(), scale)
  scale = eager_grad.abs().max().item()   # the parameter gradient written in the same capture
  assert scale > 0 and (grad - eager_grad).abs().max().item() <= 2e-5 * scale, ((grad - eager_grad).abs().max().item(), scale)
