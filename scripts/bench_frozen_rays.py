#!/usr/bin/env python
"""HIP-event times of the frozen alignment step (training.align_step: nrf_loss_grad_rays + the camera reverse pass) against the only
equivalent the parent commit has -- training.train_step(cameras=..., learning_rate=0) -- and of train_step with refinement off on
both checkouts, float32, at configuration A (1024 rays x (64 + 128) samples, no warp) and at the gpu_vrig_paper shape (768 rays x
(128 + 128), SE3 warp; no regulariser on either side: the frozen step has none), as markdown:
    python scripts/bench_frozen_rays.py --root PARENT_CHECKOUT --json parent.json     # the parent commit, built, on the same box
    python scripts/bench_frozen_rays.py --parent parent.json >> profiles/frozen_rays.md
Each figure: 10 warm-up steps, then the median over 50 events-bracketed steps on the current stream (10th .. 90th percentile), learning
rates 0.  --root: the checkout whose package is measured (default: this one); a checkout without training.align_step (the parent) is
measured on the other two columns only.  --parent: the --json file this script wrote for the parent's checkout in the same session on
the same box; its csrc_sha16 and medians are printed beside the new ones, never typed in by hand.  Below the table: one per-stage
line from nrf_profile_read for the frozen step, and the workspace sizes of the three plans."""
import argparse
import ctypes as C
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
from nerfies_amd import lib as L, models, training  # noqa: E402
from nerfies_amd.camera import Camera, pack_cameras, rays_from_table  # noqa: E402

HAVE_FROZEN = hasattr(training, 'align_step')
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
  with torch.no_grad():   # refinement off: the same rays (the deltas are zero), precomputed
    o, d = rays_from_table(table, batch['pixels'], batch['item_index'])
  batch['origins'], batch['directions'] = o.clone(), d.clone()
  if M['reg']:   # the warp field's ids; the regularisers stay off: alignment has none
    batch['metadata'] = {'warp': batch['item_index'].long(), 'camera': torch.randint(0, 2, (rays, 1), generator=g).to(dev)}
  sp = training.ScalarParams(learning_rate=bench.BENCH_LR)
  refiner = training.CameraRefiner(table, groups='pose')
  aligner = training.CameraRefiner(table, groups='pose')
  box = {'key': 1}

  def step(cameras):
    ckw = dict(cameras=cameras, camera_learning_rate=0.0) if cameras is not None else {}
    _, _, box['key'] = training.train_step(model, box['key'], state, batch, sp, **ckw)

  def align():
    _, box['key'] = training.align_step(model, fp, batch, aligner, state.warp_extra, box['key'], learning_rate=0.0)
  return model, rays, (lambda: step(None)), (lambda: step(refiner)), (align if HAVE_FROZEN else None)


def plan_bytes(model, rays):
  T, R, F = L.NRF_FLAG_TRAIN, L.NRF_FLAG_RAY_GRADS, getattr(L, 'NRF_FLAG_FROZEN', 0)
  out = {}
  for label, flags in (('TRAIN', T), ('TRAIN|RAY_GRADS', T | R)) + ((('TRAIN|RAY_GRADS|FROZEN', T | R | F),) if F else ()):
    n = C.c_size_t(0)
    L.check(model.lib.nrf_workspace_bytes(model.handle, rays, flags, C.byref(n)), model.lib)
    out[label] = n.value
  return out


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
  record = {'csrc_sha16': bench.kernel_source_sha(), 'device': device_name, 'warmup': WARMUP, 'reps': REPS, 'off_ms': {}, 'on_ms': {},
            'align_ms': {}, 'bytes': {}}
  print(f'\n## Step times ({device_name}, csrc_sha16 {record["csrc_sha16"]}' +
        (f'; parent csrc_sha16 {parent["csrc_sha16"]}' if parent else '') + ')\n')
  print(f'HIP events around one step (float32, one GPU, learning rates 0, no regulariser), {WARMUP} warm-up steps, median of {REPS} '
        f'(10th .. 90th percentile); {CAMERAS} cameras, pose deltas.'
        + (' The parent columns: this script on the parent commit\'s checkout, same box, same session.' if parent else '') + '\n')
  print('| workload | rays | train_step ms | parent train_step ms | train_step(cameras, lr 0) ms | parent train_step(cameras, lr 0) ms | align_step ms '
        '| align_step / parent equivalent |')
  print('|---|---|---|---|---|---|---|---|')
  fmt = lambda m: f'{m[0]:.3f} ({m[1]:.3f} .. {m[2]:.3f})' if m else '-'
  stages = []
  for name, label in (('train', 'A: (64+128) samples, no warp'), ('vrig', 'gpu_vrig_paper shape: (128+128), SE3 warp')):
    model, rays, off, on, align = workload(name, dev)
    m_off, m_on = median_ms(off), median_ms(on)
    m_al = median_ms(align) if align else None
    record['off_ms'][name], record['on_ms'][name], record['align_ms'][name] = m_off, m_on, m_al
    record['bytes'][name] = plan_bytes(model, rays)
    base = parent['on_ms'][name] if parent else m_on
    ratio = f'{m_al[0] / base[0]:.3f}' if m_al else '-'
    print(f'| {label} | {rays} | {fmt(m_off)} | {fmt(parent["off_ms"][name]) if parent else "-"} | {fmt(m_on)} | '
          f'{fmt(parent["on_ms"][name]) if parent else "-"} | {fmt(m_al)} | {ratio} |', flush=True)
    if align:   # per-stage device times of the frozen step, REPS steps
      model.profile_enable(True)
      for _ in range(REPS):
        align()
      torch.cuda.synchronize()
      prof = model.profile_read()
      model.profile_enable(False)
      stages.append(f'- {label}: ' + ', '.join(f"{p['name']} {p['ms'] / max(p['launches'], 1) * (p['launches'] / REPS):.3f}" for p in prof)
                    + ' ms per step')
  if stages:
    print('\nPer-stage device time of the frozen step (nrf_profile_read, events around each stage; the camera kernels and Adam are outside):\n')
    print('\n'.join(stages))
  print('\nWorkspace bytes of the plans at these shapes:\n')
  for name, b in record['bytes'].items():
    print(f'- {name}: ' + ', '.join(f'{k} {v}' for k, v in b.items()))
  if args.json:
    with open(args.json, 'w') as f:
      json.dump(record, f, indent=1)


if __name__ == '__main__':
  main()
