"""The compositing reverse pass (csrc/ray_kernels.hip composite_bwd_kernel) and what it feeds, at the densities of a trained scene:
empty space (sigma 1e-13 .. 1e-3), surfaces (sigma in the hundreds next to sigma ~ 0, the transmittance gone within a few samples),
opaque rays (float32 transmittance exactly 0) and saturated colours -- tests/helpers.py density_regime; the conditions and the
float32 floor behind the tolerances are in tests/test_density_regimes_host.py, the figures in profiles/density_regimes.md.

(a) The kernel against its own inputs: out4 (activated colour and sigma), z and d_raw4 are read from the workspace, and d_raw4 is
compared with the float64 VJP of compositing + sigmoid + the sigma activation formed from those out4 and z alone.  Nothing else of the
model enters, so a rounding fault of the kernel cannot hide behind the MLPs' own float32 error.
(b) What it feeds: parameter gradients per leaf, ray gradients and the fused step's statistics against the pinned float64 oracle, at
the suite's unchanged tolerances.

Shapes: B = 7 rays of 24 + 56 samples (a 4-rays-per-block remainder, two 64-sample chunks at the fine level); one case B = 5 of
64 + 128 (three chunks: the carried Qin / Tc cross two seams)."""
import numpy as np
import pytest
import torch

import helpers as H
from oracle import nerfies_oracle as O

pytestmark = pytest.mark.gpu

IDS = [c[0] for c in H.D_RAW_CASES]


def _level_buffers(model, ws, spec, B):
  """{level: (out4 (B,S,4), z (B,S), d_raw4 (rows_pad,4))} of the workspace `ws`, on the host."""
  out = {}
  for lv, name in enumerate(H.LEVELS):
    S = spec.num_coarse_samples + (spec.num_fine_samples if lv else 0)
    rows, pad = B * S, (B * S + 63) // 64 * 64   # csrc/nrf_internal.h TILE_ROWS
    f = lambda n, k: torch.from_numpy(H._ws_words(model, ws, n, lv, k).view('float32').copy())
    out[name] = (f('out4', rows * 4).reshape(B, S, 4), f('z', rows).reshape(B, S), f('d_raw4', pad * 4).reshape(pad, 4))
  return out


def _run(kw, mode):
  spec, B, tree, b64, _ = H.regime_case(**kw)
  model, fp = H.gpu_model(spec, tree, B)
  gb = H.gpu_batch(b64)
  cot = H.case_cotangents(spec, B, mode)
  gc = H.cotangents_to_gpu(cot)
  fwd = stats = None
  if mode == 'loss':
    _, stats = model.loss_and_grad(fp, gb)
    ws = model.workspace(B, True, H.DEV)
  else:
    fwd = model.apply({'params': fp}, gb, {}, train=True, return_weights=True, bf16=mode == 'bf16', ray_grads=mode.startswith('rays'))
    ws = model.stash.ws
    if mode == 'plain':
      model.backward({'params': fp}, gb, gc['coarse']['rgb'], gc['fine']['rgb'])
    else:
      model.backward({'params': fp}, gb, d_out=gc, ray_grads=mode.startswith('rays'))
  torch.cuda.synchronize()
  return spec, B, b64, cot, fwd, stats, _level_buffers(model, ws, spec, B)


@pytest.mark.parametrize('cid,kw,mode', H.D_RAW_CASES, ids=IDS)
def test_d_raw_against_the_kernels_own_inputs(cid, kw, mode):
  spec, B, b64, cot, fwd, stats, bufs = _run(kw, mode)
  d32 = b64['directions'].float()
  for lv in H.LEVELS:
    out4, z, d_raw4 = bufs[lv]
    S = z.shape[1]
    outs, ref = H.composite_vjp(spec, out4, z, d32, cot[lv], target=b64['rgb'].float() if mode == 'loss' else None)
    if fwd is not None:   # the forward outputs, at the tolerance of tests/test_gpu_parity.py::test_volumetric_rendering
      for k in H.OUTPUTS:
        np.testing.assert_allclose(fwd[lv][k].cpu().numpy(), outs[k].numpy(), rtol=0, atol=2e-5, err_msg=f'{cid} {lv}/{k}')
    else:                 # the fused step's loss/rgb of this level from the same out4
      mse = ((outs['rgb'] - b64['rgb']) ** 2).mean().item()
      assert abs(stats[H.LEVELS.index(lv)].item() - mse) <= 1e-5 + 3e-4 * mse, (cid, lv, stats[:2], mse)
    if d_raw4.shape[0] > B * S:   # the tile padding rows
      assert d_raw4[B * S:].abs().max().item() == 0.0, (cid, lv)
    H.assert_d_raw(d_raw4[:B * S].reshape(B, S, 4), ref, kw['regime'], f'{cid} {lv}', spec.use_sample_at_infinity)
    assert ref[..., 3].abs().max().item() > 0 and d_raw4[:B * S, 3].abs().max().item() > 0, (cid, lv)   # a density path at both levels


# ---------------------------------------------------------------------------------------------------------------------------
# (b) what the kernel feeds
# ---------------------------------------------------------------------------------------------------------------------------
FINE_DENSITY_HEAD = 'nerf_mlps_fine/MLP_2/logit/kernel'


def _assert_fine_density_path(want, got, label):
  """What the relu cases of tests/test_gpu_backward_ex.py and tests/test_gpu_ray_grads.py lack: a gradient through the fine level's
  density head, on the oracle side and on the GPU side."""
  assert want.abs().max().item() > 0 and got.abs().max().item() > 0, (label, FINE_DENSITY_HEAD)


PARAM_CASES = [('empty', 'softplus'), ('surface', 'softplus'), ('surface', 'relu'), ('opaque', 'softplus'), ('opaque', 'relu')]


@pytest.mark.parametrize('regime,act', PARAM_CASES, ids=[f'{r}-{a}' for r, a in PARAM_CASES])
def test_parameter_gradients_against_the_pinned_oracle(regime, act):
  """nrf_backward_ex with every cotangent: each leaf within helpers.grad_tol of its max-abs."""
  spec, B, tree, b64, _ = H.regime_case(regime, act=act)
  r = H.Pinned(spec, B, seed=H.REGIME_SEED, params=tree, batch=b64)
  want, got = r.compare(H.cotangents(spec, B, H.OUTPUTS, seed=5), f'{regime} {act}: rgb + depth + acc + weights')
  _assert_fine_density_path(want[FINE_DENSITY_HEAD], H.leaf(got, FINE_DENSITY_HEAD), f'{regime} {act}')


@pytest.mark.parametrize('regime,act', PARAM_CASES, ids=[f'{r}-{a}' for r, a in PARAM_CASES])
def test_fused_step_against_the_pinned_oracle(regime, act):
  """nrf_train_step_loss_grad: the gradient of MSE_coarse + MSE_fine per leaf, the total, and loss/rgb and metric/psnr of both
  levels (finish_stats_kernel) at the tolerance tests/test_gpu_reference_onehop.py holds them to."""
  spec, B, tree, b64, _ = H.regime_case(regime, act=act)
  r = H.run_pinned(spec, B, 0.0, params=tree, batch=b64, check_fine_z=False)
  H.assert_pinned(r, f'fused step, {regime} {act}')
  for i, lv in enumerate(H.LEVELS):
    for slot, key in ((i, 'loss/rgb'), (2 + i, 'metric/psnr')):
      want = r['ostats'][lv][key].item()
      assert abs(r['stats'][slot].item() - want) <= 1e-5 + 3e-4 * abs(want), (regime, act, lv, key, r['stats'][slot].item(), want)
  got = H.leaf(r['got'], FINE_DENSITY_HEAD)
  scale = r['errs'][FINE_DENSITY_HEAD][1]
  assert scale > 1e-30 and got.abs().max().item() > 0, (regime, act, scale)


def test_alpha_condition_model_on_surfaces():
  """use_alpha_condition: dsig_ray = the ray's sum of d raw density reaches the alpha head's condition rows and the appearance
  embedding (alpha_cond_grad_kernel), here with a density that is neither flat nor zero."""
  spec, B, tree, b64, _ = H.regime_case('surface', alpha_cond=True)
  r = H.run_pinned(spec, B, 0.0, params=tree, batch=b64, check_fine_z=False)
  H.assert_pinned(r, 'fused step, surface, use_alpha_condition')
  W = spec.nerf_trunk_width
  for lv in H.LEVELS:
    k = H.leaf(r['got'], f'nerf_mlps_{lv}/MLP_2/logit/kernel')
    assert k.shape[0] == W + spec.num_appearance_features and k[W:].abs().max().item() > 0, lv   # the condition rows
  assert H.leaf(r['got'], 'appearance_encoder/embed/embedding').abs().max().item() > 0
  assert r['errs'][FINE_DENSITY_HEAD][1] > 1e-30 and H.leaf(r['got'], FINE_DENSITY_HEAD).abs().max().item() > 0


@pytest.mark.parametrize('regime,act', [('surface', 'softplus'), ('surface', 'relu'), ('opaque', 'softplus')])
def test_ray_gradients_against_the_pinned_oracle(regime, act):
  """nrf_backward_rays: d origins, d directions (the |d| term sum sigma dL/dsigma is large exactly here) and d viewdirs at the
  tolerances of tests/test_gpu_ray_grads.py."""
  from test_gpu_ray_grads import PinnedRays
  spec, B, tree, b64, _ = H.regime_case(regime, act=act)
  r = PinnedRays(spec, B, seed=H.REGIME_SEED, params=tree, batch=b64)
  cot = H.cotangents(spec, B, H.OUTPUTS, seed=5)
  r.compare(cot, f'{regime} {act}: rgb + depth + acc + weights')
  r.compare({lv: {'rgb': d['rgb']} for lv, d in cot.items()}, f'{regime} {act}: rgb alone')
  from nerfies_amd import params as P   # the parameter gradient of the same call (its oracle side: the parameter test of this regime)
  grad, _ = r.gpu(cot)
  assert H.leaf(P.tree_from_flat(grad.cpu(), r.model.layout), FINE_DENSITY_HEAD).abs().max().item() > 0
