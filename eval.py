"""Evaluation driver: the command-line surface of google/nerfies' eval.py (eval.py:43-58 flags, :65-420) on the
MI355X path: restores the latest checkpoint, renders strided subsets of the train / val items and the test camera
path in chunks (hipGraph-captured forward, rays generated on the GPU), writes rgb / depth PNGs and mse / psnr.

  python eval.py --base_folder EXP --data_dir CAPTURE --gin_configs EXP/config.gin [--gin_bindings "EvalConfig.eval_once = True"]

Opt-in (no reference counterpart; defaults unchanged):
  --refined_cameras          train views are rendered from EXP/camera_refined/<item_id>.json (written by train.py --refine_cameras)
                             where that file exists
  --align_cameras GROUPS     test-time pose alignment of every val frame: a one-row camera table is optimised against the frame's own
                             pixels with the field FROZEN (training.align_cameras, nrf_loss_grad_rays), the frame is rendered again
                             from the aligned camera and both metric sets are reported (psnr and psnr_aligned, ...); the aligned
                             cameras go to EXP/camera_aligned/<item_id>.json.  The aligned numbers have used the held-out image for
                             the camera's six (or more) numbers, as that protocol does.  float32 only.

Multiscale SSIM is reported for frames of at least 176 px per side (five scales), from a restatement of
tf.image.ssim_multiscale's published algorithm (nerfies_amd/evaluation.py)."""
import argparse
import functools
import json
import os
import shutil
import sys
import time

import numpy as np
import torch

from nerfies_amd import camera, checkpoints, configs, evaluation, models, training, utils, visualization as viz
from nerfies_amd import gin_lite as gin
import train as train_driver


def process_batch(*, batch, rng, state, tag, item_id, step, writer, render_fn, save_dir, datasource):
  """Renders one frame, writes its images, returns its metrics (eval.py:65-152)."""
  item_id = item_id.replace('/', '_')
  render = render_fn(state, batch, rng=rng)
  rgb = render['rgb'].cpu().numpy()
  depth_exp, depth_med = render['depth'].cpu().numpy(), render['med_depth'].cpu().numpy()
  if save_dir:
    os.makedirs(save_dir, exist_ok=True)
    colorize_depth = functools.partial(viz.colorize, cmin=datasource.near, cmax=datasource.far, invert=True)
    viz.save_image(os.path.join(save_dir, f'rgb_{item_id}.png'), viz.image_to_uint8(rgb))
    viz.save_image(os.path.join(save_dir, f'depth_expected_viz_{item_id}.png'), viz.image_to_uint8(colorize_depth(depth_exp)))
    viz.save_depth(os.path.join(save_dir, f'depth_expected_{item_id}.png'), depth_exp)
    viz.save_image(os.path.join(save_dir, f'depth_median_viz_{item_id}.png'), viz.image_to_uint8(colorize_depth(depth_med)))
    viz.save_depth(os.path.join(save_dir, f'depth_median_{item_id}.png'), depth_med)
  out = {}
  if 'rgb' in batch:
    m = evaluation.image_metrics(render['rgb'], batch['rgb'])
    out = {k: float(v) for k, v in m.items()}
    if _rank() == 0:
      print(f'\t[{tag}] {item_id}: ' + ', '.join(f'{k}={v:.04f}' for k, v in out.items()), flush=True)
  return out


def _rank():
  import torch.distributed as dist
  return dist.get_rank() if dist.is_available() and dist.is_initialized() else 0


def parse_flags(argv=None):
  """train.py's flags (shared, as in the reference) plus the evaluation-only camera options."""
  p = argparse.ArgumentParser(add_help=False)
  p.add_argument('--align_cameras', default=None, choices=['pose', 'pose+focal', 'all'],
                 help='align every val frame\'s camera against its own pixels with the field frozen, and report both metric sets')
  p.add_argument('--align_steps', type=int, default=100, help='alignment steps per frame')
  p.add_argument('--align_rays', type=int, default=1024, help='rays per alignment step (a seeded random subset of the frame)')
  p.add_argument('--align_lr', type=float, default=2e-3, help='Adam learning rate of the alignment (the value of --camera_lr; untuned)')
  p.add_argument('--refined_cameras', action='store_true',
                 help='render train views from <exp>/camera_refined/<item_id>.json where train.py --refine_cameras wrote one')
  own, rest = p.parse_known_args(argv)
  flags = train_driver.parse_flags(rest)
  for k, v in vars(own).items():
    setattr(flags, k, v)
  return flags


def frame_from_camera(datasource, item_id, cam, device):
  """datasource.item_rays(item_id) seen from `cam` instead of the capture's own camera."""
  item = datasource.get_item(item_id)
  rays = evaluation.rays_from_camera(cam, item['metadata'], device)
  if item['rgb'].shape[:2] != rays['origins'].shape[:2]:
    raise ValueError(f'item {item_id}: image is {item["rgb"].shape[:2]} but the camera says {rays["origins"].shape[:2]}')
  rays['rgb'] = torch.from_numpy(item['rgb']).to(rays['origins'].device)
  return rays


def refined_frames(datasource, item_ids, camera_dir, device):
  """The frames of `item_ids`, from camera_dir/<item_id>.json (the capture's format and frame) where it exists."""
  for item_id in item_ids:
    path = os.path.join(camera_dir, f'{item_id}.json')
    if os.path.exists(path):
      yield frame_from_camera(datasource, item_id, datasource.load_camera(path), device)
    else:
      yield datasource.item_rays(item_id, device)


def write_camera(datasource, cam, path):
  """A camera of the normalised scene frame as the capture stores its own: full resolution, the capture's frame (train.py writes
  camera_refined/ the same way)."""
  cam = cam.copy()
  center, scale = getattr(datasource, 'scene_center', None), getattr(datasource, 'scene_scale', None)
  image_scale = getattr(datasource, 'image_scale', 1)
  if scale is not None:
    cam.position = cam.position / scale
  if center is not None:
    cam.position = cam.position + center
  if image_scale != 1:
    cam = cam.scale(image_scale)
  os.makedirs(os.path.dirname(path), exist_ok=True)
  with open(path, 'w') as f:
    json.dump(cam.to_json(), f, indent=2)


def align_frame(*, model, flags, datasource, out_dir, item_id, batch, rng, state, step, render_fn, device):
  """Test-time pose alignment of one held-out frame: its one-row camera table against its own pixels, the field frozen; then the
  frame rendered from the aligned camera -> its metrics under <name>_aligned."""
  import torch.distributed as dist
  given = datasource.load_camera(item_id)
  n = batch['pixels'].shape[0] * batch['pixels'].shape[1]
  pool = {'pixels': batch['pixels'].reshape(n, 2).contiguous(), 'item_index': torch.zeros(n, 1, dtype=torch.int32, device=device),
          'rgb': batch['rgb'].reshape(n, -1)[:, :3].contiguous(),
          'metadata': {k: v.reshape(n, -1) for k, v in (batch.get('metadata') or {}).items()}}
  refiner = training.align_cameras(model, state.optimizer.target, camera.pack_cameras([given], device), pool, groups=flags.align_cameras,
                                   steps=flags.align_steps, learning_rate=flags.align_lr, rays_per_step=flags.align_rays, seed=step,
                                   warp_extra=state.warp_extra)
  if dist.is_available() and dist.is_initialized():   # dray is accumulated with float atomics: the ranks may differ in the last bit
    dist.broadcast(refiner.deltas, src=0)
  aligned = camera.unpack_camera(refiner.compose()[0], given.image_size)
  if _rank() == 0:
    write_camera(datasource, aligned, os.path.join(out_dir, f'{item_id}.json'))
  render = render_fn(state, frame_from_camera(datasource, item_id, aligned, device), rng=rng)
  out = {f'{k}_aligned': float(v) for k, v in evaluation.image_metrics(render['rgb'], batch['rgb']).items()}
  if _rank() == 0:
    print(f'\t[val] {item_id}: ' + ', '.join(f'{k}={v:.04f}' for k, v in out.items()), flush=True)
  return out


def process_iterator(tag, item_ids, iterator, rng, state, step, render_fn, writer, save_dir, datasource, extra_fn=None):
  """eval.py:155-217.  extra_fn(item_id, batch) -> further metrics of the frame (the aligned set of --align_cameras)."""
  save_dir = os.path.join(save_dir, f'{step:08d}', tag) if save_dir else None
  meters = {}
  for i, (item_id, batch) in enumerate(zip(item_ids, iterator)):
    if tag == 'test':      # a test camera has no metadata of its own: one id per table, drawn from the step (eval.py:171-199)
      g = np.random.RandomState(step)
      md = {}
      for name, ids in (('appearance', datasource.appearance_ids), ('warp', datasource.warp_ids), ('camera', datasource.camera_ids)):
        if ids:
          # a raw id VALUE, as random.choice(datasource.*_ids) gives (the embedding row: tables have max(ids)+1 rows,
          # models.py:121-131) -- the same convention training.train_step's background ids follow
          md[name] = torch.full(batch['origins'][..., :1].shape, int(ids[g.randint(len(ids))]), dtype=torch.int32,
                                device=batch['origins'].device)
      if getattr(datasource, 'use_time', False):
        # eval.py:189-194: timestamp ~ U[0, 1) from the step's key, then jnp.full(shape, timestamp, dtype=uint32) -- the
        # reference's integer cast truncates it to 0; kept (drop-in behaviour), as a float32 tensor the TimeEncoder takes
        timestamp = float(np.uint32(g.uniform(0.0, 1.0)))
        md['time'] = torch.full(batch['origins'][..., :1].shape, timestamp, dtype=torch.float32, device=batch['origins'].device)
      batch['metadata'] = md
    stats = process_batch(batch=batch, rng=rng, state=state, tag=tag, item_id=item_id, step=step, writer=writer,
                          render_fn=render_fn, save_dir=save_dir, datasource=datasource)
    if extra_fn is not None:
      stats.update(extra_fn(item_id, batch))
    for k, v in stats.items():
      meters.setdefault(k, utils.ValueMeter()).update(v)
  for k, m in meters.items():
    writer.scalar(f'metrics-eval/{k}/{tag}', m.reduce('mean'), step)
  return {k: m.reduce('mean') for k, m in meters.items()}


def delete_old_renders(render_dir, max_renders):
  for path in sorted(os.listdir(render_dir))[:-max_renders]:
    shutil.rmtree(os.path.join(render_dir, path))


def main(argv=None):
  flags = parse_flags(argv)
  if flags.align_cameras and flags.bf16:
    raise SystemExit('--align_cameras: not with --bf16 (the frozen ray gradients are built for the float32 mode)')
  gin.parse_config_files_and_bindings(config_files=flags.gin_configs, bindings=flags.gin_bindings, skip_unknown=True)
  exp_config = configs.ExperimentConfig()
  model_config = configs.ModelConfig(use_stratified_sampling=False)        # eval.py:239: explicit kwarg beats the binding
  train_config, eval_config = configs.TrainConfig(), configs.EvalConfig()
  rank, world, device = train_driver.init_distributed()
  exp_dir = flags.base_folder if not exp_config.subname else os.path.join(flags.base_folder, exp_config.subname)
  summary_dir, renders_dir = os.path.join(exp_dir, 'summaries', 'eval'), os.path.join(exp_dir, 'renders')
  checkpoint_dir = os.path.join(exp_dir, 'checkpoints')
  os.makedirs(renders_dir, exist_ok=True)
  datasource = train_driver.make_datasource(flags, exp_config, model_config)

  train_eval_ids = utils.strided_subset(datasource.train_ids, eval_config.num_train_eval)
  val_eval_ids = utils.strided_subset(datasource.val_ids, eval_config.num_val_eval)
  test_cameras = datasource.load_test_cameras(count=eval_config.num_test_eval)

  model, params = models.construct_nerf(
      20200823, model_config, batch_size=eval_config.chunk, appearance_ids=datasource.appearance_ids,
      camera_ids=datasource.camera_ids, warp_ids=datasource.warp_ids, near=datasource.near, far=datasource.far,
      use_warp_jacobian=False, use_weights=False, device=device)
  if flags.bf16:   # as train.py: a model shape the bfloat16 / split-bf16 chains do not run is refused with the library's reason
    try:
      model.check_mode(flags.bf16)
    except models.L.NrfError as e:
      raise SystemExit(f'--bf16: {e}')
  init_state = training.TrainState(optimizer=training.Optimizer(params))
  renderer = evaluation.GraphedChunkRenderer(model, bf16=flags.bf16)   # hipGraph replay per chunk
  render_fn = functools.partial(evaluation.render_image, model_fn=renderer, device_count=world, chunk=eval_config.chunk)
  writer = utils.ScalarLog(summary_dir, enabled=rank == 0)   # summaries, meters and prints on process 0 only
  last_step, results = 0, {}
  while True:
    if checkpoints.latest_checkpoint(checkpoint_dir) is None:
      if eval_config.eval_once:
        raise FileNotFoundError(f'no checkpoint under {checkpoint_dir}')
      time.sleep(10)
      continue
    state = checkpoints.restore_checkpoint(checkpoint_dir, init_state)
    step = state.optimizer.step
    if step <= last_step:
      time.sleep(10)
      continue
    save_dir = renders_dir if eval_config.save_output and rank == 0 else None
    common = dict(rng=0, state=state, step=step, render_fn=render_fn, writer=writer, save_dir=save_dir, datasource=datasource)
    align = None
    if flags.align_cameras:
      align = lambda item_id, batch: align_frame(model=model, flags=flags, datasource=datasource, item_id=item_id, batch=batch, rng=0,
                                                 out_dir=os.path.join(exp_dir, 'camera_aligned'), state=state, step=step,
                                                 render_fn=render_fn, device=device)
    results['val'] = process_iterator('val', val_eval_ids, datasource.create_iterator(val_eval_ids, batch_size=0, repeat=False, device=device),
                                      extra_fn=align, **common)
    train_frames = refined_frames(datasource, train_eval_ids, os.path.join(exp_dir, 'camera_refined'), device) if flags.refined_cameras else \
        datasource.create_iterator(train_eval_ids, batch_size=0, repeat=False, device=device)
    results['train'] = process_iterator('train', train_eval_ids, train_frames, **common)
    if test_cameras:
      frames = (evaluation.rays_from_camera(c, None, device) for c in test_cameras)
      results['test'] = process_iterator('test', [f'{i:03d}' for i in range(len(test_cameras))], frames, **common)
    if save_dir:
      delete_old_renders(renders_dir, eval_config.max_render_checkpoints)
    if eval_config.eval_once or step >= train_config.max_steps:
      break
    last_step = step
  return results


if __name__ == '__main__':
  main(sys.argv[1:])
