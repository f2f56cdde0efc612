"""Frozen-field ray gradients on the GPU: NRF_FLAG_FROZEN / nrf_loss_grad_rays against the non-frozen path that
tests/test_gpu_ray_grads.py pins to the float64 oracle and tests/test_gpu_camera_refine.py holds the fused step against.

The frozen plan keeps no activation stash and no dY image and runs kernels of its own (csrc/chain_frozen.hip, the frozen SE3
instantiations); what it computes must be what the non-frozen path computes.  Gate: GATE_STEP = 2e-5 of the reference tensor's max-abs,
the constant of tests/test_gpu_camera_refine.py for two calls that differ in where d_rgb is rounded and in the order of dray's float
atomics; every comparison also asserts a non-zero reference.  Shapes as in those files: B = 7 with 24 + 56 samples and a 64-wide trunk
without the warp (a remainder in the 4-rays-per-block ray stage, two 64-lane chunks per fine ray, nine 64-row tiles), B = 5 with
16 + 16 samples with the SE3 warp at alpha 2.5, one case with nerf_rgb_branch_depth = 2 (bits_rgbx kept, st_rgbx / dy_rgbx dropped)."""
import functools
import os
import sys
import tempfile
import types

import numpy as np
import pytest
import torch

import helpers as H
from oracle import nerfies_oracle as O
from test_gpu_camera_refine import (DEMO_POSITION_RATIO, DEMO_ROTATION_RATIO, GATE_STEP, SHAPE, Case, _capture, _case, _close, _field, _rows,
                                    _tie_levels)

pytestmark = pytest.mark.gpu

NRF_E_STATE = -6   # include/nerfies_amd.h
OUTPUTS = ('rgb', 'depth', 'acc', 'weights')


class DeepCase(Case):
  """The no-warp case with a two-layer rgb branch."""

  def __init__(self, seed):
    self.spec = O.ModelSpec(use_white_background=True, sigma_activation='softplus', nerf_rgb_branch_depth=2, **SHAPE)
    self.B = 7
    p32 = O.init_params(self.spec, seed=seed, trained_like=True, dtype=torch.float32)
    self.model, self.fp = H.gpu_model(self.spec, p32, self.B)
    b = O.synthetic_batch(self.B, seed=seed + 1, dtype=torch.float32)
    b['viewdirs'] = b['directions'].clone()
    b['directions'] = b['directions'] * 1.7
    self.gb = H.gpu_batch(b)
    g = torch.Generator().manual_seed(seed + 2)
    self.rngs = {'coarse': torch.rand(self.B, self.spec.num_coarse_samples, generator=g).to(H.DEV),
                 'fine': torch.rand(self.B, self.spec.num_fine_samples, generator=g).to(H.DEV)}
    self.we = {'alpha': 0.0, 'time_alpha': 0.0}


@functools.lru_cache(maxsize=None)
def _named(kind):
  return DeepCase(seed=71) if kind == 'rgb-depth-2' else _case(kind == 'warp')


def _cotangents(c, keys, seed):
  g = torch.Generator().manual_seed(seed)
  S = {'coarse': c.spec.num_coarse_samples, 'fine': c.spec.num_coarse_samples + c.spec.num_fine_samples}
  shape = lambda lv: {'rgb': (c.B, 3), 'depth': (c.B,), 'acc': (c.B,), 'weights': (c.B, S[lv]), 'warped_points': (c.B, S[lv], 3)}
  return {lv: {k: torch.randn(*shape(lv)[k], generator=g).to(H.DEV) for k in keys} for lv in ('coarse', 'fine')}


def _apply(c, frozen):
  return c.model.apply({'params': c.fp}, c.gb, c.we, train=True, ray_grads=True, frozen=frozen, rngs=c.rngs, return_weights=True,
                       return_points=bool(c.spec.use_warp))


@pytest.mark.parametrize('kind', ['no-warp', 'warp', 'rgb-depth-2'])
def test_three_call_path_equals_the_non_frozen_one(kind):
  c = _named(kind)
  keys = OUTPUTS + (('warped_points',) if c.spec.use_warp else ())
  cot = _cotangents(c, keys, seed=5)
  out = _apply(c, frozen=False)
  want_out = {lv: {k: out[lv][k].clone() for k in keys} for lv in out}
  grad, want = c.model.backward({'params': c.fp}, c.gb, d_out=cot, ray_grads=True)
  assert grad is not None and sorted(want) == ['directions', 'origins', 'viewdirs']
  want = {k: t.clone() for k, t in want.items()}
  out = _apply(c, frozen=True)
  for lv in out:
    for k in keys:
      _close(out[lv][k], want_out[lv][k], GATE_STEP, f'{kind}: forward {lv}/{k}')
  grad, got = c.model.backward({'params': c.fp}, c.gb, d_out=cot, ray_grads=True)
  assert grad is None   # nothing of the parameter gradient was kept
  for k in ('origins', 'directions', 'viewdirs'):
    _close(got[k], want[k], GATE_STEP, f'{kind}: d {k}')
  # a subset of the names: the others are skipped, not written
  _, got = c.model.backward({'params': c.fp}, c.gb, d_out=cot, ray_grads=('origins',))
  assert sorted(got) == ['origins']
  _close(got['origins'], want['origins'], GATE_STEP, f'{kind}: d origins alone')


def _stats_close(got, want, what):
  for i, name in enumerate(('mse_coarse', 'mse_fine', 'psnr_coarse', 'psnr_fine', 'loss')):
    a, b = got[i].item(), want[i].item()
    print(f'[{what}] stats {name}: {a:.7g} against {b:.7g}')
    assert b != 0 and abs(a - b) <= GATE_STEP * abs(b), (what, name, a, b)
  assert not got[5:].any()   # no regulariser in the frozen step


@pytest.mark.parametrize('warp', [False, True])
def test_fused_step_equals_loss_and_grad(warp):
  c = _case(warp)
  _, want_stats, want = c.fused(c.gb)
  before = c.fp.flat.clone()
  stats, rg = c.model.loss_and_ray_grads(c.fp, c.gb, warp_extra=c.we, rngs=c.rngs)
  torch.cuda.synchronize()
  assert sorted(rg) == ['directions', 'origins']
  for k in ('origins', 'directions'):
    _close(rg[k], want[k], GATE_STEP, f'warp={warp} fused d {k}')
  _stats_close(stats, want_stats, f'warp={warp}')
  assert torch.equal(c.fp.flat, before)
  # with rays->viewdirs the fused frozen step also returns d viewdirs: that of the three-call path on the MSE's cotangent
  _, want3 = c.three_calls(c.gb, ('origins', 'directions', 'viewdirs'))
  _, rg = c.model.loss_and_ray_grads(c.fp, c.gb, warp_extra=c.we, rngs=c.rngs, ray_grads=('origins', 'directions', 'viewdirs'))
  for k in ('origins', 'directions', 'viewdirs'):
    _close(rg[k], want3[k], GATE_STEP, f'warp={warp} fused d {k} against the three-call path')


def test_fused_step_folds_null_viewdirs_into_d_directions():
  c = _case(False)
  no_vd = {k: v for k, v in c.gb.items() if k != 'viewdirs'}
  _, want_stats, want = c.fused(no_vd)
  _, with_vd = c.three_calls(dict(no_vd, viewdirs=c.gb['directions']), ('directions', 'viewdirs'))
  assert with_vd['viewdirs'].abs().max().item() > 0   # the term that has to arrive in d_directions
  stats, rg = c.model.loss_and_ray_grads(c.fp, no_vd, warp_extra=c.we, rngs=c.rngs)
  for k in ('origins', 'directions'):
    _close(rg[k], want[k], GATE_STEP, f'fold: d {k}')
  _close(rg['directions'], with_vd['directions'] + with_vd['viewdirs'], GATE_STEP, 'fold: d directions + d viewdirs')
  _stats_close(stats, want_stats, 'fold')
  from nerfies_amd import lib as L
  with pytest.raises(L.NrfError, match='d_viewdirs'):
    c.model.loss_and_ray_grads(c.fp, no_vd, warp_extra=c.we, rngs=c.rngs, ray_grads=('viewdirs',))


def test_state_errors():
  from nerfies_amd import lib as L
  c = _case(False)
  cot = _cotangents(c, OUTPUTS, seed=6)
  _apply(c, frozen=True)
  with pytest.raises(L.NrfError, match=f'error {NRF_E_STATE}: .*NRF_FLAG_FROZEN'):   # nrf_backward_ex
    c.model.backward({'params': c.fp}, c.gb, d_out=cot)
  with pytest.raises(L.NrfError, match=f'error {NRF_E_STATE}: .*NRF_FLAG_FROZEN'):   # ... with the rgb cotangents given positionally
    c.model.backward({'params': c.fp}, c.gb, cot['coarse']['rgb'], cot['fine']['rgb'])
  with pytest.raises(L.NrfError, match=f'error {NRF_E_STATE}: .*NRF_FLAG_FROZEN.*grad_params must be NULL'):
    c.model.backward({'params': c.fp}, c.gb, d_out=cot, ray_grads=True, grad_out=torch.zeros_like(c.fp.flat))
  import ctypes as C
  rays, keep = c.model._rays_struct(c.gb, H.DEV)   # nrf_backward itself, which the Python host never calls
  ws, g = c.model.stash.ws, torch.zeros_like(c.fp.flat)
  rc = c.model.lib.nrf_backward(c.model.handle, c.fp.flat.data_ptr(), C.byref(rays), cot['coarse']['rgb'].data_ptr(),
                                cot['fine']['rgb'].data_ptr(), g.data_ptr(), ws.data_ptr(), ws.numel() * 4, None)
  assert rc == NRF_E_STATE and b'NRF_FLAG_FROZEN' in c.model.lib.nrf_last_error()
  del keep
  _, rg = c.model.backward({'params': c.fp}, c.gb, d_out=cot, ray_grads=True)   # the refusals left the stash usable
  assert rg['origins'].abs().max().item() > 0
  # the stash of the fused frozen step is frozen too
  c.model.loss_and_ray_grads(c.fp, c.gb, warp_extra=c.we, rngs=c.rngs)
  with pytest.raises(L.NrfError, match=f'error {NRF_E_STATE}: .*NRF_FLAG_FROZEN'):
    c.model.backward({'params': c.fp}, c.gb, d_out=cot)
  # a following non-frozen forward: backward works as before
  c.model.apply({'params': c.fp}, c.gb, c.we, train=True, rngs=c.rngs)
  plain = c.model.backward({'params': c.fp}, c.gb, d_out=cot).clone()
  c.model.apply({'params': c.fp}, c.gb, c.we, train=True, ray_grads=True, rngs=c.rngs)
  grad, _ = c.model.backward({'params': c.fp}, c.gb, d_out=cot, ray_grads=True)
  _close(grad, plain, GATE_STEP, 'parameter gradient after a frozen call')


def test_graph_replay_equals_eager():
  """One loss_and_ray_grads call captured into a hipGraph on a side stream and replayed twice (no allocation, no synchronisation)."""
  c = Case(False, seed=61)
  rg_out = {k: torch.zeros(c.B, 3, device=H.DEV) for k in ('origins', 'directions', 'viewdirs')}
  stats = torch.zeros(16, device=H.DEV)

  def step():
    c.model.loss_and_ray_grads(c.fp, c.gb, warp_extra=c.we, rngs=c.rngs, ray_grads=tuple(rg_out), ray_grads_out=rg_out, stats_out=stats)

  s = torch.cuda.Stream()
  s.wait_stream(torch.cuda.current_stream())
  with torch.cuda.stream(s):
    step()
  torch.cuda.current_stream().wait_stream(s)
  torch.cuda.synchronize()
  eager = {k: t.clone() for k, t in rg_out.items()}
  eager_stats = stats.clone()
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph):
    step()
  for _ in range(2):
    for t in rg_out.values():
      t.zero_()
    stats.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for k, y in eager.items():
      scale = y.abs().max().item()
      assert scale > 0 and (rg_out[k] - y).abs().max().item() <= 2e-5 * scale, (k, (rg_out[k] - y).abs().max().item(), scale)
    assert eager_stats[4].item() > 0 and (stats - eager_stats).abs().max().item() <= 2e-5 * eager_stats.abs().max().item()


def test_autograd_runs_frozen_when_only_a_ray_needs_a_gradient(monkeypatch):
  from nerfies_amd import autograd, lib as L
  c = _case(False)
  model = c.model
  T, R, F = L.NRF_FLAG_TRAIN, L.NRF_FLAG_RAY_GRADS, L.NRF_FLAG_FROZEN
  seen = []
  real = model.lib.nrf_forward

  def spy(*a):   # (handle, params, rays, scalars, rand, outputs, flags, ...)
    seen.append(int(a[6]))
    return real(*a)
  monkeypatch.setattr(model.lib, 'nrf_forward', spy)
  target = torch.linspace(0.1, 0.7, c.B, device=H.DEV)

  def origins_grad(flat):
    rays = dict(c.gb, origins=c.gb['origins'].clone().requires_grad_(True))
    out = autograd.render_differentiable(model, flat, rays, c.we, c.rngs)
    (((out['fine']['depth'] - target) ** 2).sum() + out['coarse']['rgb'].sum()).backward()
    return rays['origins'].grad.clone()

  flat = c.fp.flat.clone()
  got = origins_grad(flat)   # flat needs no gradient: frozen
  flat.requires_grad_(True)
  want = origins_grad(flat)
  assert seen == [T | R | F, T | R], seen
  assert flat.grad is not None and flat.grad.abs().max().item() > 0
  _close(got, want, GATE_STEP, 'autograd: origins.grad frozen against non-frozen')


def test_align_step_leaves_train_steps_d_deltas_and_no_change_in_the_field():
  from nerfies_amd import training
  table0, col, near, far = _capture()
  batch = _rows(col, (4, 3, 0))
  model, fp = _field(near, far)
  model_b, fp_b = _field(near, far)
  assert torch.equal(fp.flat, fp_b.flat)
  before = fp.flat.clone()
  refiner, refiner_b = training.CameraRefiner(table0, groups='all'), training.CameraRefiner(table0, groups='all')
  stats, key = training.align_step(model, fp, batch, refiner, {}, 0, learning_rate=2e-3)
  state_b = training.TrainState(optimizer=training.Optimizer(fp_b))
  _, stats_b, key_b = training.train_step(model_b, 0, state_b, batch, training.ScalarParams(learning_rate=0.0), cameras=refiner_b,
                                          camera_learning_rate=2e-3)
  torch.cuda.synchronize()
  assert key == key_b and torch.equal(fp.flat, before)   # bit for bit
  _close(refiner.d_deltas, refiner_b.d_deltas, GATE_STEP, 'align_step d_deltas against train_step(cameras=..., learning_rate=0)')
  assert refiner.step == 1 and refiner.deltas[:2, :14].abs().max().item() > 0 and not refiner.deltas[2].any()   # frame 2 has no ray
  assert stats[4].item() > 0 and not stats[5:].any()


def test_align_cameras_recovers_a_perturbed_pose():
  """The setting of tests/test_gpu_camera_refine.py::test_recovers_a_perturbed_pose through training.align_cameras: tied levels, the
  768 rays of frame 0 every step, 200 steps, pose only, Adam at 2e-3; the gate is twice the parent-measured ratios of the existing torch
  path (that module's DEMO_*_RATIO), and both errors must shrink."""
  from nerfies_amd import camera, datasets, models, training
  with tempfile.TemporaryDirectory() as d:
    datasets.write_synthetic_scene(d, num_frames=4, size=(32, 24))
    src = datasets.NerfiesDataSource(d, image_scale=1)
    ids = src.train_ids
    table0 = src.camera_table(ids, H.DEV)
    col = src.create_ray_table(ids, H.DEV, shuffle=True, keep_item_index=True).columns
    near, far = src.near, src.far
  cfg = types.SimpleNamespace(num_coarse_samples=32, num_fine_samples=32, num_nerf_point_freqs=6, nerf_trunk_width=128,
                              use_stratified_sampling=False, sigma_activation='softplus')
  model, fp = models.construct_nerf(0, cfg, 0, [0], [0], [0], near, far)
  _tie_levels(model, fp)
  sel = (col['item_index'][:, 0] == 0).nonzero()[:, 0]
  batch = {k: col[k][sel].contiguous() for k in ('pixels', 'item_index', 'origins', 'directions')}
  batch['metadata'] = {}
  assert batch['pixels'].shape[0] == 768
  o, dd = camera.rays_from_table(table0, batch['pixels'], batch['item_index'])
  out = model.apply({'params': fp}, {'origins': o, 'directions': dd, 'metadata': {}}, {})
  batch['rgb'] = out['fine']['rgb'].clone()   # the rendering from the true camera
  off = torch.zeros(table0.shape[0], 16, device=H.DEV)
  off[0, :6] = torch.tensor([0.02, -0.015, 0.01, 0.010, -0.008, 0.006])
  start = camera.compose_cameras(table0, off)
  SL = camera.CAMERA_PARAM_SLICES
  R0, p0 = table0[0, SL['orientation']].reshape(3, 3), table0[0, SL['position']]

  def errors(table):   # the angle from |R - R0|_F = 2 sqrt(2) sin(angle / 2), in float64
    R = table[0, SL['orientation']].reshape(3, 3).double()
    half = ((R - R0.double()).norm() / (2 * 2 ** 0.5)).clamp(max=1.0)
    return (table[0, SL['position']] - p0).norm().item(), 2 * torch.asin(half).item()

  pos0, rot0 = errors(start)
  before = fp.flat.clone()
  refiner = training.align_cameras(model, fp, start, batch, groups='pose', steps=200, learning_rate=2e-3, rays_per_step=768, seed=0)
  pos, rot = errors(refiner.compose())
  print(f'[frozen recovery] position error {pos0:.6f} -> {pos:.3e} ({pos / pos0:.3e}), rotation error {rot0:.6f} -> {rot:.3e} '
        f'({rot / rot0:.3e}); existing torch path: {DEMO_POSITION_RATIO}, {DEMO_ROTATION_RATIO}')
  assert torch.equal(fp.flat, before) and refiner.step == 200
  assert pos < pos0 and rot < rot0
  assert pos / pos0 <= 2 * DEMO_POSITION_RATIO and rot / rot0 <= 2 * DEMO_ROTATION_RATIO
  # seeded subsets: two runs draw the same rays and a shorter run moves the camera less far
  sub = [training.align_cameras(model, fp, start, batch, groups='pose', steps=3, rays_per_step=64, seed=7).deltas.clone() for _ in range(2)]
  assert sub[0][0, :6].abs().max().item() > 0 and (sub[0] - sub[1]).abs().max().item() <= 1e-3 * sub[0].abs().max().item()
  assert not sub[0][1:].any() and not sub[0][:, 6:].any()


def test_eval_driver_aligns_val_cameras_and_renders_refined_train_views(tmp_path, monkeypatch):
  """The shipped test_local preset on a 4-frame 24 x 16 synthetic capture: 20 steps of train.py --refine_cameras pose, then
  eval.py --align_cameras pose --align_steps 10 --align_rays 64 --refined_cameras, once."""
  import json
  from nerfies_amd import camera, datasets, evaluation
  root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
  sys.path.insert(0, root)
  import eval as eval_driver
  import train as train_driver
  from nerfies_amd import gin_lite as gin
  cap, exp = str(tmp_path / 'cap'), str(tmp_path / 'exp')
  ids = datasets.write_synthetic_scene(cap, num_frames=4, size=(24, 16), image_scale=4)   # the preset reads rgb/4x; the last frame is val
  train_ids, val_id = ids[:-1], ids[-1]
  args = ['--base_folder', exp, '--data_dir', cap, '--gin_configs', os.path.join(root, 'configs', 'test_local.gin')]
  for b in ('TrainConfig.batch_size = 64', 'TrainConfig.print_every = 10', 'TrainConfig.log_every = 10', 'TrainConfig.save_every = 20',
            'EvalConfig.eval_once = True'):
    args += ['--gin_bindings', b]
  steps, lr = 10, 2e-3
  align = ['--align_cameras', 'pose', '--align_steps', str(steps), '--align_rays', '64', '--refined_cameras']
  gin.clear_config()
  with pytest.raises(SystemExit, match='--align_cameras.*--bf16'):
    eval_driver.main(args + ['--align_cameras', 'pose', '--bf16'])
  gin.clear_config()
  train_driver.main(args + ['--refine_cameras', 'pose', '--max_steps', '20'])
  refined_dir = os.path.join(exp, 'camera_refined')
  assert sorted(os.listdir(refined_dir)) == sorted(f'{i}.json' for i in train_ids)
  gin.clear_config()
  seen = []
  real = evaluation.rays_from_camera

  def spy(cam, metadata=None, device='cuda'):
    seen.append(cam)
    return real(cam, metadata, device)
  monkeypatch.setattr(evaluation, 'rays_from_camera', spy)
  res = eval_driver.main(args + align)
  gin.clear_config()
  assert set(res) >= {'val', 'train'}
  for k in ('mse', 'psnr', 'mse_aligned', 'psnr_aligned'):   # both metric sets for the held-out frame (24 x 16: too small for ms-ssim)
    assert np.isfinite(res['val'][k]), (k, res['val'])
  assert 'psnr_aligned' not in res['train'] and np.isfinite(res['train']['psnr'])
  scal = [json.loads(l) for l in open(os.path.join(exp, 'summaries', 'eval', 'scalars.jsonl'))]
  assert {'metrics-eval/psnr/val', 'metrics-eval/psnr_aligned/val'} <= {r.get('tag') for r in scal}
  # the aligned camera, written as the capture stores its own
  assert os.listdir(os.path.join(exp, 'camera_aligned')) == [f'{val_id}.json']
  aligned = camera.Camera.from_json(os.path.join(exp, 'camera_aligned', f'{val_id}.json'))
  given = camera.Camera.from_json(os.path.join(cap, 'camera', f'{val_id}.json'))
  np.testing.assert_allclose(aligned.orientation @ aligned.orientation.T, np.eye(3), atol=1e-5)
  assert aligned.focal_length == pytest.approx(given.focal_length, rel=1e-5) and tuple(aligned.image_size) == tuple(given.image_size)
  moved = np.abs(aligned.position - given.position).max()
  assert 0 < moved < 10.0 * steps * lr * 3   # steps of lr 2e-3 in the normalised frame, scene_scale 0.1 (the bound of the train driver's test)
  # the train views were rendered from camera_refined/: a camera equal to the refined file's, unequal to the capture's
  src = datasets.NerfiesDataSource(cap, image_scale=4)
  for item in train_ids:
    want = src.load_camera(os.path.join(refined_dir, f'{item}.json'))
    own = src.load_camera(item)
    assert np.abs(want.position - own.position).max() > 0
    assert any(np.array_equal(c.position, want.position) and np.array_equal(c.orientation, want.orientation) for c in seen), item
    assert not any(np.array_equal(c.position, own.position) and np.array_equal(c.orientation, own.orientation) for c in seen), item
