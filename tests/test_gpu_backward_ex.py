"""nrf_backward_ex / NerfModel.backward(d_out=...) / nerfies_amd.autograd: the VJP of NerfModel.apply (models.py:289-375) with a
cotangent for every differentiable output -- rgb, depth, acc, weights (model_utils.py:116-126) and warped_points
(models.py:266-267) -- instead of rgb alone.

Shapes are the smallest that still cross the compositing kernel's seams: B = 7 leaves a 4-rays-per-block remainder, 24 + 56 = 80
fine samples make two 64-sample chunks per ray (the reverse recurrence and the d_weights load cross the chunk boundary), and
the cases run both background and both infinity switches under both sigma activations.  The float64 reference is
torch.autograd over oracle.nerf_model_apply, evaluated on the HIP path's own ReLU pattern and fine depths (tests/helpers.py;
tests/test_gpu_pinned.py has the rationale), within helpers.grad_tol of every leaf's max-abs."""
import functools
import itertools

import numpy as np
import pytest
import torch

import helpers as H
from oracle import nerfies_oracle as O

pytestmark = pytest.mark.gpu

NRF_E_STATE = -6   # include/nerfies_amd.h
B = 7
SHAPE = dict(num_coarse_samples=24, num_fine_samples=56, nerf_trunk_width=64, num_nerf_point_freqs=4, use_stratified_sampling=False)
OUTPUTS = ('rgb', 'depth', 'acc', 'weights')


def _cotangents(spec, nrays, keys, seed):
  """{level: {key: float64 tensor}}: seeded normals in the shapes of NerfModel.apply's outputs."""
  g = torch.Generator().manual_seed(seed)
  S = {'coarse': spec.num_coarse_samples, 'fine': spec.num_coarse_samples + spec.num_fine_samples}
  shape = lambda lv: {'rgb': (nrays, 3), 'depth': (nrays,), 'acc': (nrays,), 'weights': (nrays, S[lv]), 'warped_points': (nrays, S[lv], 3)}
  return {lv: {k: torch.randn(*shape(lv)[k], generator=g, dtype=torch.float64) for k in keys} for lv in ('coarse', 'fine')}


def _to_gpu(cot):
  return {lv: {k: t.float().to(H.DEV) for k, t in d.items()} for lv, d in cot.items()}


Pinned = H.Pinned   # shared with tests/test_gpu_density_regimes.py


@functools.lru_cache(maxsize=None)
def _case(white, inf, act, tile_rows=0):
  spec = O.ModelSpec(use_white_background=white, use_sample_at_infinity=inf, sigma_activation=act, **SHAPE)
  return Pinned(spec, B, seed=31, tile_rows=tile_rows)


@pytest.mark.parametrize('white,inf,act', list(itertools.product((False, True), (False, True), ('relu', 'softplus'))))
def test_oracle_parity_without_the_warp(white, inf, act):
  """loss = sum_l <a_l, rgb_l> + <b_l, depth_l> + <c_l, acc_l> + <D_l, weights_l>, then every cotangent alone: a wrong mask on the
  last sample for acc or a missing white-background term cannot hide behind the other terms."""
  r = _case(white, inf, act)
  cot = _cotangents(r.spec, B, OUTPUTS, seed=5)
  r.compare(cot, f'white={white} inf={inf} {act}: all')
  for k in OUTPUTS:
    want, _ = r.compare({lv: {k: d[k]} for lv, d in cot.items()}, f'white={white} inf={inf} {act}: {k} alone')
    assert max(g.abs().max().item() for g in want.values()) > 0


def test_oracle_parity_on_the_32_row_reverse_chain():
  """NRF_OPT_CHAIN_TILE_ROWS = 32: the 32-row reverse chain reads the same d raw rows the compositing reverse wrote."""
  r = _case(True, True, 'softplus', tile_rows=32)
  r.compare(_cotangents(r.spec, B, OUTPUTS, seed=5), 'white=True inf=True softplus, 32-row tiles: all')


def test_oracle_parity_with_the_warp_field():
  """SE3 field: a cotangent on warped_points at both levels plus one on depth.  d x' joins the NeRF MLP's own d points ahead of the
  SE3 dgrad, so the warp-field leaves and the GLO table see both."""
  nrays = 5
  spec = O.ModelSpec(num_coarse_samples=16, num_fine_samples=16, nerf_trunk_width=64, num_nerf_point_freqs=4, use_stratified_sampling=False,
                     use_warp=True, warp_field_type='se3', num_warp_freqs=4)
  r = Pinned(spec, nrays, seed=41, alpha=2.5, points=True)
  cot = _cotangents(spec, nrays, ('warped_points', 'depth'), seed=6)
  want, got = r.compare(cot, 'warp: warped_points + depth')
  warp_leaves = [p for p in want if p.startswith('warp_field/')]
  assert any('embed' in p for p in warp_leaves) and len(warp_leaves) > 4, warp_leaves
  for p in warp_leaves:
    assert want[p].abs().max().item() > 0 and H.leaf(got, p).abs().max().item() > 0, p
  r.compare({lv: {'warped_points': d['warped_points']} for lv, d in cot.items()}, 'warp: warped_points alone')


def _nocond():
  """A warp-off model without a per-ray condition (use_viewdirs = False): the only float atomics of its reverse pass, the per-ray
  condition sums, feed no gradient, so two calls on the same inputs agree bit for bit and bit identity is a sound criterion."""
  spec = O.ModelSpec(use_viewdirs=False, use_white_background=True, **SHAPE)
  p32 = O.init_params(spec, seed=51, trained_like=True, dtype=torch.float32)
  model, fp = H.gpu_model(spec, p32, B)
  gb = H.gpu_batch(O.synthetic_batch(B, seed=52, dtype=torch.float32))
  return spec, model, fp, gb


def test_rgb_only_is_bit_identical_with_nrf_backward():
  import ctypes as C
  from nerfies_amd import lib as L
  spec, model, fp, gb = _nocond()
  model.apply({'params': fp}, gb, {}, train=True)
  cot = _to_gpu(_cotangents(spec, B, ('rgb',), seed=7))
  dc, df = cot['coarse']['rgb'], cot['fine']['rgb']

  def nrf_backward():
    """The rgb-only export, which NerfModel.backward no longer goes through: a direct call on the model's stash."""
    rays, keep = model._rays_struct(gb, H.DEV)
    grad, ws = torch.empty_like(fp.flat), model.stash.ws
    L.check(model.lib.nrf_backward(model.handle, fp.flat.data_ptr(), C.byref(rays), dc.data_ptr(), df.data_ptr(), grad.data_ptr(),
                                   ws.data_ptr(), ws.numel() * 4, torch.cuda.current_stream().cuda_stream), model.lib)
    torch.cuda.synchronize()   # `keep` holds the rays' buffers until the launches are through
    return grad

  old = nrf_backward()
  assert old.abs().max().item() > 0
  assert torch.equal(model.backward({'params': fp}, gb, d_out=cot), old)
  assert torch.equal(model.backward({'params': fp}, gb, dc, d_out={'fine': {'rgb': df}}), old)   # positional and dict mixed
  # zero-filled depth / acc / weights buffers select the kernel that reads them: the same bits again
  zeros = {lv: dict(d, **{k: torch.zeros_like(t) for k, t in _to_gpu(_cotangents(spec, B, ('depth', 'acc', 'weights'), seed=8))[lv].items()})
           for lv, d in cot.items()}
  assert torch.equal(model.backward({'params': fp}, gb, d_out=zeros), old)
  # no cotangent at all: a zero gradient
  assert model.backward({'params': fp}, gb, d_out={}).abs().max().item() == 0.0
  assert torch.equal(model.backward({'params': fp}, gb, dc, df), old)   # the positional form is the same call
  assert torch.equal(nrf_backward(), old)   # ... and the old entry is what it was, after all of it


def test_bf16_training_mode_follows_the_float32_gradient():
  """NRF_FLAG_BF16 stashes: compositing is the same float32 kernel, so the general VJP holds there as well.  Per-leaf cosine >= 0.98
  against the float32 result, the bar of the bf16 training tests."""
  spec = O.ModelSpec(use_white_background=True, **SHAPE)
  p32 = O.init_params(spec, seed=31, trained_like=True, dtype=torch.float32)
  model, fp = H.gpu_model(spec, p32, B)
  gb = H.gpu_batch(O.synthetic_batch(B, seed=32, dtype=torch.float32))
  cot = _to_gpu(_cotangents(spec, B, OUTPUTS, seed=5))
  model.apply({'params': fp}, gb, {}, train=True, bf16=True)
  g16 = model.backward({'params': fp}, gb, d_out=cot).clone()
  model.apply({'params': fp}, gb, {}, train=True)
  g32 = model.backward({'params': fp}, gb, d_out=cot)
  assert torch.isfinite(g16).all()
  worst = ('', 1.0)
  for name, off, shape in model.layout.entries:
    n = int(np.prod(shape))
    a, b = g16[off:off + n].double(), g32[off:off + n].double()
    assert b.norm().item() > 0, name
    cos = (a @ b).item() / max(a.norm().item() * b.norm().item(), 1e-300)
    if cos < worst[1]:
      worst = (name, cos)
  print(f'[bf16 vs float32, all cotangents] worst leaf {worst[0]} cosine {worst[1]:.4f}')
  assert worst[1] >= 0.98, worst


def test_autograd_wrapper_equals_the_explicit_call():
  from nerfies_amd import autograd, lib as L
  spec, model, fp, gb = _nocond()
  flat = fp.flat.clone().requires_grad_(True)
  out = autograd.render_differentiable(model, flat, gb, {}, return_weights=True, return_z_vals=True)
  for lv in ('coarse', 'fine'):
    assert not out[lv]['med_depth'].requires_grad and not out[lv]['z_vals'].requires_grad
    assert all(out[lv][k].requires_grad for k in OUTPUTS)
  cot = _to_gpu(_cotangents(spec, B, ('rgb', 'weights'), seed=9))
  target = torch.linspace(0.1, 0.7, B, device=H.DEV)
  loss = (out['fine']['rgb'] * cot['fine']['rgb']).sum() + ((out['fine']['acc'] - 1.0) ** 2).sum() \
      + ((out['coarse']['depth'] - target) ** 2).sum() + (out['fine']['weights'] * cot['fine']['weights']).sum()
  loss.backward()
  assert flat.grad is not None and flat.grad.abs().max().item() > 0
  with torch.no_grad():
    d_out = {'fine': {'rgb': cot['fine']['rgb'], 'acc': 2.0 * (out['fine']['acc'] - 1.0), 'weights': cot['fine']['weights']},
             'coarse': {'depth': 2.0 * (out['coarse']['depth'] - target)}}
  explicit = model.backward({'params': fp}, gb, d_out=d_out)   # the stash of the wrapper's forward is still the model's last
  assert torch.equal(flat.grad, explicit)
  with pytest.raises(L.NrfError, match='inference-only'):
    autograd.render_differentiable(model, flat, gb, {}, bf16='x3')
  # bf16=True is a training mode and goes through
  out16 = autograd.render_differentiable(model, flat, gb, {}, bf16=True)
  flat.grad = None
  out16['fine']['depth'].sum().backward()
  assert torch.isfinite(flat.grad).all() and flat.grad.abs().max().item() > 0


def test_refusals():
  from nerfies_amd import lib as L
  spec, model, fp, gb = _nocond()
  S0 = spec.num_coarse_samples
  model.apply({'params': fp}, gb, {}, train=True)
  with pytest.raises(L.NrfError, match=f'error {NRF_E_STATE}: .*d_warped_points'):   # the stashed forward ran without a warp field
    model.backward({'params': fp}, gb, d_out={'coarse': {'warped_points': torch.zeros(B, S0, 3, device=H.DEV)}})
  model.backward({'params': fp}, gb, d_out={'coarse': {'acc': torch.ones(B, device=H.DEV)}})   # the refusal left the stash usable
  model.apply({'params': fp}, gb, {})   # an inference forward: nothing stashed any more
  with pytest.raises(L.NrfError, match=f'error {NRF_E_STATE}: '):
    model.backward({'params': fp}, gb, d_out={'coarse': {'acc': torch.ones(B, device=H.DEV)}})


def test_graph_replay_equals_eager():
  """One forward + nrf_backward_ex captured into a hipGraph (no allocation, no synchronisation in either) and replayed; agreement
  as in tests/test_gpu_graph_step.py: every leaf within 2e-5 of its max-abs (float32 summation order of the atomics)."""
  spec = O.ModelSpec(use_white_background=True, **SHAPE)
  p32 = O.init_params(spec, seed=61, trained_like=True, dtype=torch.float32)
  model, fp = H.gpu_model(spec, p32, B)
  gb = H.gpu_batch(O.synthetic_batch(B, seed=62, dtype=torch.float32))
  cot = _to_gpu(_cotangents(spec, B, OUTPUTS, seed=10))
  grad = torch.zeros_like(fp.flat)

  def step(out=None):
    out = model.apply({'params': fp}, gb, {}, train=True, return_weights=True, out=out)
    model.backward({'params': fp}, gb, grad_out=grad, d_out=cot)
    return out

  s = torch.cuda.Stream()   # one eager step on a side stream: uploads the tables, sizes the workspace, allocates the outputs
  s.wait_stream(torch.cuda.current_stream())
  with torch.cuda.stream(s):
    out = step()
  torch.cuda.current_stream().wait_stream(s)
  torch.cuda.synchronize()
  eager = grad.clone()
  assert eager.abs().max().item() > 0
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph):
    step(out)
  grad.zero_()
  graph.replay()
  torch.cuda.synchronize()
  for name, off, shape in model.layout.entries:
    n = int(np.prod(shape))
    x, y = grad[off:off + n], eager[off:off + n]
    scale = y.abs().max().item()
    assert (x - y).abs().max().item() <= 2e-5 * scale, (name, (x - y).abs().max().item(), scale)
