#!/usr/bin/env python
"""Camera refinement through the whole differentiable chain, on a synthetic capture:

    pose deltas (C, 16) -> compose_cameras (HIP) -> rays_from_table (HIP) -> viewdirs = d / |d| (torch)
      -> render_differentiable (HIP, nrf_backward_rays) -> photometric + depth loss -> backward -> torch Adam

The NeRF parameters are fixed (a freshly initialised field); the target is its own rendering from the true camera of frame 0.  That
camera's position and orientation are then perturbed and recovered.  A demonstration, not a test:
    python scripts/refine_camera_demo.py [--steps 300]"""
import argparse
import os
import sys
import tempfile
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nerfies_amd import autograd, datasets, models  # noqa: E402
from nerfies_amd.camera import CAMERA_DELTA_SLICES as DL, CAMERA_PARAM_SLICES as SL, compose_cameras, rays_from_table  # noqa: E402


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--steps', type=int, default=300)
  ap.add_argument('--lr', type=float, default=2e-3)
  ap.add_argument('--frozen', action='store_true',
                  help='the same recovery through training.align_cameras: the fused frozen step (nrf_loss_grad_rays) instead of autograd '
                       'over render_differentiable.  Its loss is MSE_coarse + MSE_fine against one target, so the fine MLP is set to the '
                       'coarse one (both terms then have their minimum at the true pose)')
  args = ap.parse_args()
  dev = torch.device('cuda:0')
  with tempfile.TemporaryDirectory() as d:
    datasets.write_synthetic_scene(d, num_frames=4, size=(32, 24))
    src = datasets.NerfiesDataSource(d, image_scale=1)
    ids = src.train_ids
    table0 = src.camera_table(ids, dev)
    rays = src.create_ray_table(ids, dev, shuffle=True, keep_item_index=True)
    near, far = src.near, src.far
  cfg = types.SimpleNamespace(num_coarse_samples=32, num_fine_samples=32, num_nerf_point_freqs=6, nerf_trunk_width=128,
                              use_stratified_sampling=False, sigma_activation='softplus')
  model, fp = models.construct_nerf(0, cfg, 0, [0], [0], [0], near, far)
  col = rays.columns
  sel = (col['item_index'][:, 0] == 0).nonzero()[:, 0]   # the rays of frame 0, in the table's permuted order
  pixels, index = col['pixels'][sel].contiguous(), col['item_index'][sel].contiguous()

  def render(table):
    origins, directions = rays_from_table(table, pixels, index)
    viewdirs = directions / directions.norm(dim=-1, keepdim=True)
    out = autograd.render_differentiable(model, fp.flat, {'origins': origins, 'directions': directions, 'viewdirs': viewdirs,
                                                          'metadata': {}})
    return out['fine']['rgb'], out['fine']['depth']

  with torch.no_grad():
    rgb_t, depth_t = (t.clone() for t in render(table0))
  R0, p0 = table0[0, SL['orientation']].reshape(3, 3).clone(), table0[0, SL['position']].clone()
  w_off = torch.tensor([0.02, -0.015, 0.01], device=dev)     # radians
  p_off = torch.tensor([0.010, -0.008, 0.006], device=dev)   # scene units (the scene spans about 0.3)
  offset = torch.zeros(table0.shape[0], 16, device=dev)
  offset[0, DL['rotation']], offset[0, DL['translation']] = w_off, p_off
  with torch.no_grad():
    start = compose_cameras(table0, offset)   # frame 0 turned by exp(hat w_off) and moved by p_off
  if args.frozen:
    frozen_demo(model, fp, table0, start, pixels, index, args)
    return
  pose = torch.zeros(6, device=dev, requires_grad=True)   # frame 0's (rotation, translation) delta; the other columns stay 0
  opt = torch.optim.Adam([pose], lr=args.lr)
  print(f'frame 0 of {len(ids)}: {pixels.shape[0]} rays; start: position error {p_off.norm().item():.5f}, rotation error '
        f'{w_off.norm().item():.5f} rad')
  for step in range(args.steps + 1):
    deltas = torch.zeros_like(offset)
    deltas[0, :6] = pose
    table = compose_cameras(start, deltas)   # R = exp(hat w) R_start, position + t: differentiable in the deltas
    rgb, depth = render(table)
    loss = ((rgb - rgb_t) ** 2).mean() + ((depth - depth_t) ** 2).mean()
    if step % 10 == 0:
      with torch.no_grad():
        R = table[0, SL['orientation']].reshape(3, 3)
        cosang = ((R @ R0.T).diagonal().sum() - 1) / 2
        print(f'step {step:4d}  loss {loss.item():.3e}  position error {(table[0, SL["position"]] - p0).norm().item():.5f}  rotation error '
              f'{torch.acos(cosang.clamp(-1, 1)).item():.5f} rad')
    if step == args.steps:
      break
    opt.zero_grad()
    loss.backward()
    opt.step()


def frozen_demo(model, fp, table0, start, pixels, index, args):
  from nerfies_amd import training
  off = {name: (o, int(np.prod(shape))) for name, o, shape in model.layout.entries}
  for name, (o, n) in off.items():   # fine MLP := coarse MLP
    if name.startswith('nerf_mlps_fine'):
      oc, _ = off[name.replace('nerf_mlps_fine', 'nerf_mlps_coarse')]
      fp.flat[o:o + n] = fp.flat[oc:oc + n]
  with torch.no_grad():
    o, d = rays_from_table(table0, pixels, index)
    target = model.apply({'params': fp}, {'origins': o, 'directions': d, 'metadata': {}}, {})['fine']['rgb'].clone()
  batch = {'pixels': pixels, 'item_index': index, 'rgb': target, 'metadata': {}}
  R0, p0 = table0[0, SL['orientation']].reshape(3, 3).double(), table0[0, SL['position']]

  def errors(table):   # the angle from |R - R0|_F = 2 sqrt(2) sin(angle / 2), in float64
    half = ((table[0, SL['orientation']].reshape(3, 3).double() - R0).norm() / (2 * 2 ** 0.5)).clamp(max=1.0)
    return (table[0, SL['position']] - p0).norm().item(), 2 * torch.asin(half).item()

  pos0, rot0 = errors(start)
  refiner = training.align_cameras(model, fp, start, batch, groups='pose', steps=args.steps, learning_rate=args.lr)
  pos, rot = errors(refiner.compose())
  print(f'frozen alignment, {pixels.shape[0]} rays, {args.steps} steps: position error {pos0:.5f} -> {pos:.3e}, rotation error '
        f'{rot0:.5f} -> {rot:.3e} rad')


if __name__ == '__main__':
  main()
