#!/usr/bin/env python
"""HIP-event times of training.train_step with camera refinement on and off, float32, at configuration A (1024 rays x (64 + 128)
samples, no warp) and at the gpu_vrig_paper shape (768 rays x (128 + 128), SE3 warp + elastic + background), as markdown:
    python scripts/bench_camera_refine.py --root PARENT_CHECKOUT --json parent.json     # the parent commit, built, on the same box
    python scripts/bench_camera_refine.py --parent parent.json >> profiles/camera_refine.md
Each figure: 10 warm-up steps, then the median over 50 events-bracketed steps on the current stream, learning rates 0 (bench.BENCH_LR).
--root: the checkout whose package is measured (default: this one).  A checkout without training.CameraRefiner (the parent commit) is
measured with refinement off only, on the same rays.  --json: also write the figures to a file.  --parent: such a file, written by
this script for the parent commit in the same session on the same box; its csrc_sha16 and refinement-off medians are printed beside
the new ones.  The parent's figures are never typed in by hand."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if '--root' in sys.argv:   # before the package is imported
  ROOT = os.path.abspath(sys.argv[sys.argv.index('--root') + 1])
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (kernel_source_sha, the workloads' configurations)
from nerfies_amd import models, training  # noqa: E402
from nerfies_amd.camera import Camera, pack_cameras, rays_from_table  # noqa: E402

HAVE_REFINER = hasattr(training, 'CameraRefiner')

WARMUP, REPS, CAMERAS = 10, 50, 256


def median_ms(fn):
  for _ in range(WARMUP):
    fn()
  torch.cuda.synchronize()
  ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(REPS)]
  for a, b in ev:
    a.record()
    fn()
    b.record()
  torch.cuda.synchronize()
  t = sorted(a.elapsed_time(b) for a, b in ev)
  return t[len(t) // 2], t[len(t) // 10], t[-len(t) // 10]


def workload(name, dev):
  M = bench.TRAIN_MODES[name]
  rays = 1024 if name == 'train' else M['rays']
  frames = list(range(CAMERAS))
  model, fp = models.construct_nerf(0, M['cfg'], rays, frames, [0, 1], frames, 0.0206, 0.826, device=dev)
  state = training.TrainState(optimizer=training.Optimizer(fp), warp_alpha=M['alpha'])
  g = torch.Generator().manual_seed(0)
  rng = np.random.default_rng(0)
  cams = []
  for _ in range(CAMERAS):   # cameras on a shell around the scene, looking at it
    pos = rng.normal(size=3)
    pos *= 0.6 / np.linalg.norm(pos)
    cams.append(Camera(orientation=np.eye(3), position=np.zeros(3), focal_length=800.0, principal_point=[480.0, 270.0], image_size=[960, 540],
                       radial_distortion=[0.01, 0.0, 0.0]).look_at(pos, np.zeros(3), np.array([0.0, 1.0, 0.0])))
  table = pack_cameras(cams, dev)
  batch = {'rgb': torch.rand(rays, 3, generator=g).to(dev),
           'pixels': (torch.rand(rays, 2, generator=g) * torch.tensor([960.0, 540.0])).to(dev).contiguous(),
           'item_index': torch.randint(0, CAMERAS, (rays, 1), generator=g, dtype=torch.int32).to(dev)}
  refiner = training.CameraRefiner(table, groups='pose') if HAVE_REFINER else None
  with torch.no_grad():   # refinement off: the same rays (the deltas are zero), precomputed
    o, d = rays_from_table(table, batch['pixels'], batch['item_index'])
  batch['origins'], batch['directions'] = o.clone(), d.clone()
  kw = {}
  if M['reg']:
    sp = training.ScalarParams(learning_rate=bench.BENCH_LR, background_loss_weight=1.0, elastic_loss_weight=M['elastic_w'])
    batch['metadata'] = {'warp': batch['item_index'].long(), 'camera': torch.randint(0, 2, (rays, 1), generator=g).to(dev)}
    batch['background_points'] = ((torch.rand(16384, 3, generator=g) - 0.5) * 0.8).to(dev)
    kw = dict(use_elastic_loss=True, elastic_reduce_method='weight', use_background_loss=True)
  else:
    sp = training.ScalarParams(learning_rate=bench.BENCH_LR)
  box = {'key': 1}

  def step(cameras):
    ckw = dict(cameras=cameras, camera_learning_rate=0.0) if cameras is not None else {}
    _, _, box['key'] = training.train_step(model, box['key'], state, batch, sp, **ckw, **kw)
  return rays, (lambda: step(None)), ((lambda: step(refiner)) if HAVE_REFINER else None)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--root', default=ROOT, help='the checkout to measure (default: the one this script lies in)')
  ap.add_argument('--json', default=None, help='write the figures to this file as well')
  ap.add_argument('--parent', default=None, help="the --json file this script wrote for the parent commit's checkout on this box")
  args = ap.parse_args()
  dev = torch.device('cuda:0')
  device_name = torch.cuda.get_device_name(0)
  parent = None
  if args.parent:
    with open(args.parent) as f:
      parent = json.load(f)
    if parent['device'] != device_name:
      raise SystemExit(f"--parent was measured on {parent['device']!r}, this is {device_name!r}")
  record = {'csrc_sha16': bench.kernel_source_sha(), 'device': device_name, 'warmup': WARMUP, 'reps': REPS, 'off_ms': {}, 'on_ms': {}}
  print(f'\n## Step times ({device_name}, csrc_sha16 {record["csrc_sha16"]}' +
        (f'; parent csrc_sha16 {parent["csrc_sha16"]}' if parent else '') + ')\n')
  print(f'HIP events around training.train_step (float32, one GPU, learning rates 0), {WARMUP} warm-up steps, median of {REPS} '
        f'(10th .. 90th percentile); {CAMERAS} cameras, refinement of the pose.'
        + (' The parent column: this script on the parent commit\'s checkout, same box, same session.' if parent else '') + '\n')
  print('| workload | rays | refinement off ms | parent, off ms | refinement on ms | overhead |')
  print('|---|---|---|---|---|---|')
  fmt = lambda m: f'{m[0]:.3f} ({m[1]:.3f} .. {m[2]:.3f})' if m else '-'
  for name, label in (('train', 'A: (64+128) samples, no warp'), ('vrig', 'gpu_vrig_paper shape: (128+128), SE3 warp + elastic + background')):
    rays, off, on = workload(name, dev)
    m_off = median_ms(off)
    m_on = median_ms(on) if on else None
    record['off_ms'][name], record['on_ms'][name] = m_off, m_on
    over = f'+{100.0 * (m_on[0] / m_off[0] - 1.0):.1f} %' if m_on else '-'
    print(f'| {label} | {rays} | {fmt(m_off)} | {fmt(parent["off_ms"][name]) if parent else "-"} | {fmt(m_on)} | {over} |', flush=True)
  if args.json:
    with open(args.json, 'w') as f:
      json.dump(record, f, indent=1)


if __name__ == '__main__':
  main()
