"""Camera refinement on the GPU: nrf_train_step_loss_grad_rays (the fused train step with ray gradients) against the three-call path
nrf_forward + nrf_backward_rays that tests/test_gpu_ray_grads.py pins to the float64 oracle, the camera delta table
(nrf_camera_table_compose / _compose_backward) against a float64 restatement, and training.CameraRefiner / train_step(cameras=...)
against autograd through compose_cameras -> rays_from_table -> render_differentiable -> MSE.

Shapes as tests/test_gpu_ray_grads.py: B = 7 with 24 + 56 samples and a 64-wide trunk without the warp (a 4-rays-per-block
remainder, two 64-lane chunks per fine ray), B = 5 with 16 + 16 samples with it (a small tangent pass).  Every call gets explicit
uniforms, so two calls sample alike."""
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

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))   # the spawned ranks import this module and helpers

pytestmark = pytest.mark.gpu

GATE_STEP = 2e-5   # fused step against the three-call path: where d_rgb is rounded, atomic order (test_autograd_routes_gradients_to_the_rays)
GATE = 2e-4        # per delta group against float64 autograd (the gate of tests/test_gpu_camera_grads.py)
SHAPE = dict(num_coarse_samples=24, num_fine_samples=56, nerf_trunk_width=64, num_nerf_point_freqs=4, use_stratified_sampling=False)
WARP_SHAPE = dict(num_coarse_samples=16, num_fine_samples=16, nerf_trunk_width=64, num_nerf_point_freqs=4, use_stratified_sampling=False,
                  use_warp=True, num_warp_freqs=4)


def _close(got, want, gate, what):
  scale = want.abs().max().item()
  err = (got - want).abs().max().item()
  print(f'[{what}] max-abs {scale:.3e}, error / max-abs {err / max(scale, 1e-30):.2e} (gate {gate:.0e})')
  assert scale > 0 and err <= gate * scale, (what, err, scale)


class Case:
  """A model, a batch whose directions are 1.7 x a unit vector (the |d| factor of the compositing distances cannot go missing) and
  fixed uniforms."""

  def __init__(self, warp, seed):
    self.spec = O.ModelSpec(use_white_background=True, sigma_activation='softplus', **(WARP_SHAPE if warp else SHAPE))
    self.B = 5 if warp else 7
    p32 = O.init_params(self.spec, seed=seed, trained_like=True, dtype=torch.float32)
    self.model, self.fp = H.gpu_model(self.spec, p32, self.B)
    b = O.synthetic_batch(self.B, seed=seed + 1, dtype=torch.float32)
    b['viewdirs'] = b['directions'].clone()
    b['directions'] = b['directions'] * 1.7
    self.gb = H.gpu_batch(b)
    g = torch.Generator().manual_seed(seed + 2)
    self.rngs = {'coarse': torch.rand(self.B, self.spec.num_coarse_samples, generator=g).to(H.DEV),
                 'fine': torch.rand(self.B, self.spec.num_fine_samples, generator=g).to(H.DEV)}
    self.we = {'alpha': 2.5 if warp else 0.0, 'time_alpha': 0.0}

  def three_calls(self, batch, names):
    """apply(train, ray_grads) + backward(d_out = the MSE's d_rgb per level, ray_grads=names) -> (grad, {name: gradient})."""
    out = self.model.apply({'params': self.fp}, batch, self.we, train=True, ray_grads=True, rngs=self.rngs)
    d_out = {lv: {'rgb': 2.0 * (out[lv]['rgb'] - batch['rgb']) / (3.0 * self.B)} for lv in ('coarse', 'fine')}
    grad, rg = self.model.backward({'params': self.fp}, batch, d_out=d_out, ray_grads=names)
    return grad.clone(), {k: t.clone() for k, t in rg.items()}

  def fused(self, batch, rays=True, **reg):
    res = self.model.loss_and_grad(self.fp, batch, warp_extra=self.we, rngs=self.rngs,
                                   ray_grads=('origins', 'directions') if rays else None, **reg)
    torch.cuda.synchronize()
    return tuple(t.clone() if torch.is_tensor(t) else {k: v.clone() for k, v in t.items()} for t in res)


@functools.lru_cache(maxsize=None)
def _case(warp):
  return Case(warp, seed=41 if warp else 31)


@pytest.mark.parametrize('warp', [False, True])
def test_fused_step_equals_forward_plus_backward_rays(warp):
  c = _case(warp)
  want_grad, want = c.three_calls(c.gb, ('origins', 'directions'))
  grad, stats, rg = c.fused(c.gb)
  for k in ('origins', 'directions'):
    _close(rg[k], want[k], GATE_STEP, f'warp={warp} d {k}')
  _close(grad, want_grad, GATE_STEP, f'warp={warp} parameter gradient')
  _, stats_ex = c.fused(c.gb, rays=False)
  print(f'[warp={warp}] stats[0..4] {stats[:5].tolist()}')
  assert torch.equal(stats[:5], stats_ex[:5]) and stats[4].item() > 0


def test_null_viewdirs_fold_into_d_directions():
  """A batch without 'viewdirs' on a use_viewdirs model: the condition reads the directions, and the fused d_directions is
  d_directions + d_viewdirs of nrf_backward_rays called with viewdirs = directions."""
  c = _case(False)
  no_vd = {k: v for k, v in c.gb.items() if k != 'viewdirs'}
  _, want = c.three_calls(dict(no_vd, viewdirs=c.gb['directions']), ('origins', 'directions', 'viewdirs'))
  assert want['viewdirs'].abs().max().item() > 0
  _, _, rg = c.fused(no_vd)
  _close(rg['directions'], want['directions'] + want['viewdirs'], GATE_STEP, 'd directions + d viewdirs')
  _close(rg['origins'], want['origins'], GATE_STEP, 'd origins')
  print(f"[fold] |d viewdirs| / |d directions| = {want['viewdirs'].abs().max().item() / want['directions'].abs().max().item():.3e}")
  from nerfies_amd import lib as L
  with pytest.raises(L.NrfError, match="'origins' and 'directions'"):
    c.model.loss_and_grad(c.fp, no_vd, warp_extra=c.we, rngs=c.rngs, ray_grads=('viewdirs',))


def test_regularisers_do_not_reach_the_rays_and_are_not_broken_by_them():
  c = _case(True)
  g = torch.Generator().manual_seed(7)
  reg = dict(elastic={'weight': 1.0, 'reduce_method': 'weight'}, warp_reg={'weight': 1.0},
             background={'points': (torch.rand(16, 3, generator=g) - 0.5).to(H.DEV),
                         'warp_ids': torch.randint(0, 4, (16,), generator=g, dtype=torch.int32).to(H.DEV), 'weight': 1.0})
  grad0, _, rg0 = c.fused(c.gb)
  grad, stats, rg = c.fused(c.gb, **reg)
  moved = (grad - grad0).abs().max().item() / grad0.abs().max().item()
  print(f'[regularisers] parameter gradient moved by {moved:.3e} of its max-abs')
  assert moved > 1e-2
  for k in ('origins', 'directions'):
    _close(rg[k], rg0[k], GATE_STEP, f'd {k} with / without regularisers')
    print(f'[regularisers] d {k} bit-equal to the regulariser-free step: {torch.equal(rg[k], rg0[k])}')
  # the coarse tangent stash survives the fine Jacobian pass: the regularisers' gradient and statistics are those of the step
  # without ray gradients
  grad_ex, stats_ex = c.fused(c.gb, rays=False, **reg)
  _close(grad, grad_ex, GATE_STEP, 'parameter gradient with regularisers, with / without ray gradients')
  _close(stats[5:15], stats_ex[5:15], GATE_STEP, 'stats[5..14]')
  assert stats[6].item() != 0 and stats[5].item() != 0 and stats[8].item() != 0
  _, _, rg2 = c.fused(c.gb, **reg)
  for k in ('origins', 'directions'):
    assert torch.equal(rg[k], rg2[k]), k


# ---------------------------------------------------------------------------------------------------------------- compose
def _hat(w):
  z = torch.zeros((), dtype=w.dtype)
  return torch.stack([torch.stack([z, -w[2], w[1]]), torch.stack([w[2], z, -w[0]]), torch.stack([-w[1], w[0], z])])


def _compose64(table, deltas):
  """The float64 restatement of nrf_camera_table_compose (include/nerfies_amd.h)."""
  rows = []
  for b, d in zip(table, deltas):
    R = torch.matrix_exp(_hat(d[0:3])) @ b[0:9].reshape(3, 3)
    rows.append(torch.cat([R.reshape(9), b[9:12] + d[3:6], b[12:13] * torch.exp(d[6:7]), b[13:15] + d[7:9], b[15:17],
                           b[17:20] + d[9:12], b[20:22] + d[12:14], torch.zeros(2, dtype=b.dtype)]))
  return torch.stack(rows)


def test_compose_against_float64():
  """Five cameras, |omega| in {0, 1e-7, 1e-3, 0.3, 2.5} (the series and the closed forms of se3_math.h, which switches at
  |omega|^2 = 4; tests/test_gpu_se3_regimes.py holds both sides of it to the float32 floor).  The intrinsics are of unit magnitude (normalised image coordinates): the forward tolerance is absolute, and
  float32 itself is 3e-5 apart at a focal length of 500 pixels."""
  from nerfies_amd import camera, lib as L
  g = torch.Generator().manual_seed(11)
  C = 5
  table = torch.zeros(C, L.NRF_CAMERA_ROW, dtype=torch.float64)
  for c in range(C):
    table[c, 0:9] = torch.matrix_exp(_hat(torch.randn(3, generator=g, dtype=torch.float64))).reshape(9)
  table[:, 9:12] = 0.3 * torch.randn(C, 3, generator=g, dtype=torch.float64)
  table[:, 12] = 1.0 + 0.4 * torch.rand(C, generator=g, dtype=torch.float64)
  table[:, 13:15] = 0.5 + 0.05 * torch.randn(C, 2, generator=g, dtype=torch.float64)
  table[:, 15] = 0.01
  table[:, 16] = 1.02
  table[:, 17:22] = 0.05 * torch.randn(C, 5, generator=g, dtype=torch.float64)
  deltas = 0.1 * torch.randn(C, L.NRF_CAMERA_DELTA_ROW, generator=g, dtype=torch.float64)
  deltas[:, 14:] = 7.0   # pads: never read
  for c, norm in enumerate((0.0, 1e-7, 1e-3, 0.3, 2.5)):
    axis = torch.randn(3, generator=g, dtype=torch.float64)
    deltas[c, 0:3] = norm * axis / axis.norm()
  t32, d32 = table.float().to(H.DEV), deltas.float().to(H.DEV).requires_grad_(True)
  t64, d64 = t32.detach().cpu().double(), d32.detach().cpu().double().requires_grad_(True)
  out = camera.compose_cameras(t32, d32)
  want = _compose64(t64, d64)
  err = (out.detach().cpu().double() - want.detach()).abs().max().item()
  print(f'[compose] forward: max abs error {err:.2e} (atol 2e-6)')
  assert err <= 2e-6
  assert torch.equal(out[0].detach(), torch.cat([t32[0, :9], out[0, 9:].detach()]))   # omega = 0: R = R0 exactly
  d_cam = torch.randn(C, L.NRF_CAMERA_ROW, generator=g, dtype=torch.float64)
  (out * d_cam.float().to(H.DEV)).sum().backward()
  (want * d_cam.float().double()).sum().backward()
  got, ref = d32.grad.cpu().double(), d64.grad
  for c in range(C):
    for name, sl in camera.CAMERA_DELTA_SLICES.items():
      scale = ref[c, sl].abs().max().item()
      e = (got[c, sl] - ref[c, sl]).abs().max().item()
      print(f'[compose] camera {c} d {name}: max-abs {scale:.3e}, error / max-abs {e / max(scale, 1e-30):.2e}')
      assert scale > 0 and e <= GATE * scale, (c, name, e, scale)
  assert torch.equal(d32.grad[:, 14:], torch.zeros(C, 2, device=H.DEV))
  assert torch.isfinite(d32.grad[0, :3]).all() and d32.grad[0, :3].abs().max().item() > 0


# ---------------------------------------------------------------------------------------------------------------- the chain
@functools.lru_cache(maxsize=None)
def _capture():
  """A 3-frame synthetic capture (32 x 24): its camera table, its ray table with 'item_index', the scene bounds."""
  from nerfies_amd import datasets
  with tempfile.TemporaryDirectory() as d:
    datasets.write_synthetic_scene(d, num_frames=4, size=(32, 24))   # the last frame goes to val_ids
    src = datasets.NerfiesDataSource(d, image_scale=1)
    ids = list(src.train_ids)[:3]
    return src.camera_table(ids, H.DEV), src.create_ray_table(ids, H.DEV, shuffle=True, keep_item_index=True).columns, src.near, src.far


def _field(near, far, seed=0):
  from nerfies_amd import models
  cfg = types.SimpleNamespace(sigma_activation='softplus', **SHAPE)
  return models.construct_nerf(seed, cfg, 0, [0], [0], [0], near, far)


def _rows(col, counts):
  """counts[k] rays of frame k, in the table's permuted order, as one batch."""
  idx = torch.cat([(col['item_index'][:, 0] == k).nonzero()[:n, 0] for k, n in enumerate(counts)])
  batch = {k: v[idx].contiguous() for k, v in col.items() if not k.startswith('metadata/')}
  batch['metadata'] = {}
  return batch


def test_whole_chain_one_step():
  from nerfies_amd import autograd, camera, training
  table0, col, near, far = _capture()
  batch = _rows(col, (4, 3, 0))   # frames 0 and 1 mixed, frame 2 absent
  B = 7
  model, fp = _field(near, far)
  g = torch.Generator().manual_seed(3)
  rngs = {'coarse': torch.rand(B, SHAPE['num_coarse_samples'], generator=g).to(H.DEV),
          'fine': torch.rand(B, SHAPE['num_fine_samples'], generator=g).to(H.DEV)}
  # autograd through the three library stages; viewdirs = directions is what the condition reads without 'viewdirs'
  deltas = torch.zeros(3, 16, device=H.DEV, requires_grad=True)
  o, d = camera.rays_from_table(camera.compose_cameras(table0, deltas), batch['pixels'], batch['item_index'])
  out = autograd.render_differentiable(model, fp.flat, {'origins': o, 'directions': d, 'viewdirs': d, 'metadata': {}}, {}, rngs)
  sum(((out[lv]['rgb'] - batch['rgb']) ** 2).mean() for lv in ('coarse', 'fine')).backward()
  want = deltas.grad.clone()
  # the same rays through a step without cameras, from the same parameters
  model_b, fp_b = _field(near, far)
  state_b = training.TrainState(optimizer=training.Optimizer(fp_b))
  sp = training.ScalarParams(learning_rate=1e-3)
  training.train_step(model_b, 0, state_b, dict(batch, origins=o.detach(), directions=d.detach()), sp, rngs=rngs)
  init = fp.flat.clone()
  refiner = training.CameraRefiner(table0, groups='all')
  state = training.TrainState(optimizer=training.Optimizer(fp))
  training.train_step(model, 0, state, batch, sp, rngs=rngs, cameras=refiner, camera_learning_rate=2e-3)
  torch.cuda.synchronize()
  got = refiner.d_deltas
  for c in range(3):
    for name, sl in camera.CAMERA_DELTA_SLICES.items():
      scale = want[c, sl].abs().max().item()
      e = (got[c, sl] - want[c, sl]).abs().max().item()
      print(f'[chain] camera {c} d {name}: max-abs {scale:.3e}, error / max-abs {e / max(scale, 1e-30):.2e}')
      assert (scale > 0) == (c < 2) and e <= GATE * scale, (c, name, e, scale)
  assert all(refiner.deltas[c, sl].abs().max().item() > 0 for c in (0, 1) for sl in camera.CAMERA_DELTA_SLICES.values())
  assert torch.equal(refiner.deltas[2], torch.zeros(16, device=H.DEV)) and torch.equal(refiner.deltas[:, 14:], torch.zeros(3, 2, device=H.DEV))
  travel = (fp_b.flat - init).norm().item()
  diff = (fp.flat - fp_b.flat).norm().item()
  print(f'[chain] field parameters: |dp| {diff:.3e} over a travel of {travel:.3e}; max entry {(fp.flat - fp_b.flat).abs().max().item():.2e}')
  # the bounds of tests/test_gpu_distributed.py for two float32 summation orders under Adam
  assert travel > 0 and diff < 3e-2 * travel and (fp.flat - fp_b.flat).abs().max().item() < 1e-3
  # groups='pose': the other columns receive no gradient and stay exactly zero
  pose = training.CameraRefiner(table0, groups='pose')
  training.train_step(model, 1, state, batch, sp, rngs=rngs, cameras=pose)
  assert pose.deltas[:2, :6].abs().min(dim=1).values.max().item() > 0 and torch.equal(pose.deltas[:, 6:], torch.zeros(3, 10, device=H.DEV))


# ---------------------------------------------------------------------------------------------------------------- the driver
def test_train_driver_refines_checkpoints_and_writes_cameras(tmp_path, capsys):
  """train.py --refine_cameras pose on the shipped test_local preset (SE3 warp + elastic loss: the fused step with ray gradients next
  to the regulariser), 20 steps, then resumed to 30."""
  import json
  import os
  import sys
  from nerfies_amd import camera, checkpoints, datasets
  root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
  sys.path.insert(0, root)
  import train as train_driver
  from nerfies_amd import gin_lite as gin
  cap, exp = str(tmp_path / 'cap'), str(tmp_path / 'exp')
  ids = datasets.write_synthetic_scene(cap, num_frames=4, size=(24, 16), image_scale=4)[:-1]   # the preset reads rgb/4x
  args = ['--base_folder', exp, '--data_dir', cap, '--gin_configs', os.path.join(root, 'configs', 'test_local.gin')]
  for b in ('TrainConfig.batch_size = 64', 'TrainConfig.print_every = 10', 'TrainConfig.log_every = 10', 'TrainConfig.save_every = 20'):
    args += ['--gin_bindings', b]
  for refused in ('--graph', '--bf16'):
    gin.clear_config()
    with pytest.raises(SystemExit, match='--refine_cameras'):
      train_driver.main(args + ['--refine_cameras', 'pose', refused])
  gin.clear_config()
  state = train_driver.main(args + ['--refine_cameras', 'pose', '--max_steps', '20'])
  ckpt = os.path.join(exp, 'checkpoints')
  assert state.optimizer.step == 20 and os.path.exists(os.path.join(ckpt, 'checkpoint_20'))
  at20 = checkpoints.restore_checkpoint(os.path.join(ckpt, 'cameras_20'), None)
  assert at20['step'] == 20 and at20['deltas'].shape == (3, 16) and np.abs(at20['deltas'][:, :6]).max() > 0
  assert not at20['deltas'][:, 6:].any()   # pose only
  gin.clear_config()
  state = train_driver.main(args + ['--refine_cameras', 'pose', '--max_steps', '30'])
  assert state.optimizer.step == 30 and 'Starting training at step 21' in capsys.readouterr().out
  at30 = checkpoints.restore_checkpoint(os.path.join(ckpt, 'cameras_30'), None)
  # continued, not restarted: Adam's step count and moments carry on, and ten more steps of lr 2e-3 stay within reach of step 20
  assert at30['step'] == 30 and np.abs(at30['m']).max() > 0
  assert 0 < np.abs(at30['deltas'] - at20['deltas']).max() <= 10 * 2e-3 * 3
  out_dir = os.path.join(exp, 'camera_refined')
  assert sorted(os.listdir(out_dir)) == [f'{i}.json' for i in ids]
  for k, item in enumerate(ids):
    refined = camera.Camera.from_json(os.path.join(out_dir, f'{item}.json'))
    given = camera.Camera.from_json(os.path.join(cap, 'camera', f'{item}.json'))
    assert np.abs(refined.position - given.position).max() > 0 and np.abs(refined.orientation - given.orientation).max() > 0
    np.testing.assert_allclose(refined.orientation @ refined.orientation.T, np.eye(3), atol=1e-5)
    # pose only, and written in the capture's own frame and resolution: a drop-in for camera/<item>.json
    assert refined.focal_length == pytest.approx(given.focal_length, rel=1e-5) and tuple(refined.image_size) == tuple(given.image_size)
    assert np.abs(refined.position - given.position).max() < 10.0 * 30 * 2e-3 * 3   # 30 steps of lr 2e-3, scene_scale 0.1
  gin.clear_config()


# ---------------------------------------------------------------------------------------------------------------- two ranks
WORLD, RANK_STEPS = 2, 3


def _two_rank_worker(rank, port, tmp):
  import os
  import torch.distributed as dist
  from nerfies_amd import training
  os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
  torch.cuda.set_device(0)
  dist.init_process_group('gloo', rank=rank, world_size=WORLD)
  table0, col, near, far = _capture()
  batch = _rows(col, (3, 3, 2))
  per = 4
  shard = {k: (v[rank * per:(rank + 1) * per].contiguous() if torch.is_tensor(v) else v) for k, v in batch.items()}
  model, fp = _field(near, far)
  refiner = training.CameraRefiner(table0, groups='pose+focal')
  state = training.TrainState(optimizer=training.Optimizer(fp))
  sp = training.ScalarParams(learning_rate=1e-3)
  g = torch.Generator().manual_seed(5)
  for step in range(RANK_STEPS):
    rngs = {'coarse': torch.rand(8, SHAPE['num_coarse_samples'], generator=g)[rank * per:(rank + 1) * per].to(H.DEV),
            'fine': torch.rand(8, SHAPE['num_fine_samples'], generator=g)[rank * per:(rank + 1) * per].to(H.DEV)}
    training.train_step(model, step, state, shard, sp, rngs=rngs, cameras=refiner)
    both = [torch.empty_like(refiner.deltas) for _ in range(WORLD)]
    dist.all_gather(both, refiner.deltas)
    assert torch.equal(both[0], both[1]) and both[0][:, :7].abs().max().item() > 0, step
  if rank == 0:
    torch.save({'deltas': refiner.deltas.cpu(), 'steps': refiner.step}, tmp)
  dist.barrier()
  dist.destroy_process_group()


def test_two_ranks_keep_the_delta_tables_identical(tmp_path):
  """train_step(cameras=...) on two ranks (the launcher of tests/test_gpu_distributed.py: two processes share cuda:0 over gloo), each on
  its half of a batch that mixes the frames: d_deltas is all-reduced, so the replicas' delta tables agree bit for bit after every step."""
  import socket
  import torch.multiprocessing as mp
  with socket.socket() as s:
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
  tmp = str(tmp_path / 'deltas.pt')
  mp.spawn(_two_rank_worker, args=(port, tmp), nprocs=WORLD, join=True)
  got = torch.load(tmp, weights_only=False)
  assert got['steps'] == RANK_STEPS and got['deltas'][:, :7].abs().max().item() > 0 and not got['deltas'][:, 7:].any()


# ---------------------------------------------------------------------------------------------------------------- recovery
DEMO_POSITION_RATIO, DEMO_ROTATION_RATIO = 6.714e-3, 2.038e-3   # final / initial error of the existing path, measured (docstring below)


def _tie_levels(model, fp):
  """The fine MLP's parameters := the coarse MLP's, so one target serves MSE_coarse + MSE_fine (the fused step's fixed loss)."""
  off = {name: (o, int(np.prod(shape))) for name, o, shape in model.layout.entries}
  for name, (o, n) in off.items():
    if name.startswith('nerf_mlps_fine'):
      oc, nc = off[name.replace('nerf_mlps_fine', 'nerf_mlps_coarse')]
      assert n == nc
      fp.flat[o:o + n] = fp.flat[oc:oc + nc]


def test_recovers_a_perturbed_pose():
  """The setting of scripts/refine_camera_demo.py: a frozen, freshly initialised field (32 + 32 samples, 128-wide trunk), the 768 rays
  of frame 0, that camera turned by (0.02, -0.015, 0.01) rad and moved by (0.010, -0.008, 0.006), groups='pose', Adam at 2e-3, 200
  steps of train_step(cameras=...) with the field's learning rate 0.

  One departure from the demo, on both paths: the fused step's loss is MSE_coarse + MSE_fine against ONE target, so the fine MLP's
  parameters are set to the coarse MLP's (_tie_levels) and the target is the fine rendering from the true camera.  Both terms then have
  their minimum at the true pose.  With independently initialised levels the coarse term's minimum lies elsewhere and the pose error
  grows under this loss on the existing path as well (profiles/camera_refine.md).

  The gate is twice the ratio final / initial error of the EXISTING path in this same tied setting and with this same loss, measured on
  an MI355X with the parent commit's library: render_differentiable (viewdirs = d / |d|) for both levels, the rotation as
  torch.matrix_exp(hat w) @ R_start, torch.optim.Adam(lr=2e-3) on (w, t), 200 steps.  scripts/recovery_existing_path.py is that measurement.  The rotation error is the angle of R R0^T, taken
  from |R - R0|_F in float64.

      existing path:  position 1.4142e-2 -> 9.50e-5 (ratio 6.714e-3), rotation 2.6926e-2 -> 5.487e-5 rad (ratio 2.038e-3)
      this path:      position 1.4142e-2 -> 9.50e-5 (ratio 6.715e-3), rotation 2.6926e-2 -> 5.487e-5 rad (ratio 2.038e-3)

  Both stall at a loss of 2.7e-9 from step 120 on: the target is rendered by NerfModel.apply and is not bit-equal to either path's
  rendering at the true pose, which leaves the same small residual pose for both."""
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
  o, dd = camera.rays_from_table(table0, batch['pixels'], batch['item_index'])
  out = model.apply({'params': fp}, {'origins': o, 'directions': dd, 'metadata': {}}, {})
  batch['rgb'] = out['fine']['rgb'].clone()   # the rendering from the true camera
  off = torch.zeros(table0.shape[0], 16, device=H.DEV)
  off[0, :6] = torch.tensor([0.02, -0.015, 0.01, 0.010, -0.008, 0.006])
  start = camera.compose_cameras(table0, off)
  SL = camera.CAMERA_PARAM_SLICES
  R0, p0 = table0[0, SL['orientation']].reshape(3, 3), table0[0, SL['position']]

  def errors(table):   # the angle from |R - R0|_F = 2 sqrt(2) sin(angle / 2), in float64: acos of the trace resolves nothing below 3.5e-4 rad
    R = table[0, SL['orientation']].reshape(3, 3).double()
    half = ((R - R0.double()).norm() / (2 * 2 ** 0.5)).clamp(max=1.0)
    return (table[0, SL['position']] - p0).norm().item(), 2 * torch.asin(half).item()

  pos0, rot0 = errors(start)
  refiner = training.CameraRefiner(start, groups='pose')
  state = training.TrainState(optimizer=training.Optimizer(fp))
  sp = training.ScalarParams(learning_rate=0.0)   # frozen field
  before = fp.flat.clone()
  key = 0
  for _ in range(200):
    state, _, key = training.train_step(model, key, state, batch, sp, cameras=refiner, camera_learning_rate=2e-3)
  pos, rot = errors(refiner.compose())
  print(f'[recovery] position error {pos0:.6f} -> {pos:.3e} ({pos / pos0:.3e}), rotation error {rot0:.6f} -> {rot:.3e} ({rot / rot0:.3e}); '
        f'existing demo path: {DEMO_POSITION_RATIO}, {DEMO_ROTATION_RATIO}')
  assert torch.equal(fp.flat, before)
  assert pos < pos0 and rot < rot0
  assert pos / pos0 <= 2 * DEMO_POSITION_RATIO and rot / rot0 <= 2 * DEMO_ROTATION_RATIO
