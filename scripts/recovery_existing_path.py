#!/usr/bin/env python
"""The reference figures of tests/test_gpu_camera_refine.py::test_recovers_a_perturbed_pose: final / initial pose error of the EXISTING
refinement path -- render_differentiable for both levels (viewdirs = d / |d|), the rotation as torch.matrix_exp(hat w) @ R_start,
torch.optim.Adam on (w, t) -- in that test's setting: frozen field with the fine MLP tied to the coarse one, loss MSE_coarse + MSE_fine
against the fine rendering from the true camera, frame 0 perturbed by the demo's offsets, 200 steps at 2e-3.
    python scripts/recovery_existing_path.py [--root PARENT_CHECKOUT]
--root: the checkout whose package is imported (default: this one); the test's constants were measured on the parent commit's.  The last
line holds the two ratios that go into DEMO_POSITION_RATIO / DEMO_ROTATION_RATIO and profiles/camera_refine.md."""
import os
import sys
import tempfile
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if '--root' in sys.argv:   # before the package is imported
  ROOT = os.path.abspath(sys.argv[sys.argv.index('--root') + 1])
sys.path.insert(0, ROOT)
from nerfies_amd import autograd, datasets, models  # noqa: E402
from nerfies_amd.camera import CAMERA_PARAM_SLICES as SL, rays_from_table  # noqa: E402
import nerfies_amd  # noqa: E402
print('package', nerfies_amd.__file__)

STEPS, LR = 200, 2e-3


def hat(w):
  z = torch.zeros((), device=w.device, dtype=w.dtype)
  return torch.stack([torch.stack([z, -w[2], w[1]]), torch.stack([w[2], z, -w[0]]), torch.stack([-w[1], w[0], z])])


def tie_levels(model, fp):
  off = {name: (o, int(np.prod(shape))) for name, o, shape in model.layout.entries}
  for name, (o, n) in off.items():
    if name.startswith('nerf_mlps_fine'):
      oc, nc = off[name.replace('nerf_mlps_fine', 'nerf_mlps_coarse')]
      assert n == nc
      fp.flat[o:o + n] = fp.flat[oc:oc + nc]


def main():
  dev = torch.device('cuda:0')
  with tempfile.TemporaryDirectory() as d:
    datasets.write_synthetic_scene(d, num_frames=4, size=(32, 24))
    src = datasets.NerfiesDataSource(d, image_scale=1)
    ids = src.train_ids
    table0 = src.camera_table(ids, dev)
    col = src.create_ray_table(ids, dev, shuffle=True, keep_item_index=True).columns
    near, far = src.near, src.far
  cfg = types.SimpleNamespace(num_coarse_samples=32, num_fine_samples=32, num_nerf_point_freqs=6, nerf_trunk_width=128,
                              use_stratified_sampling=False, sigma_activation='softplus')
  model, fp = models.construct_nerf(0, cfg, 0, [0], [0], [0], near, far)
  tie_levels(model, fp)
  sel = (col['item_index'][:, 0] == 0).nonzero()[:, 0]
  pixels, index = col['pixels'][sel].contiguous(), col['item_index'][sel].contiguous()
  with torch.no_grad():
    o, dd = rays_from_table(table0, pixels, index)
    target = model.apply({'params': fp}, {'origins': o, 'directions': dd, 'metadata': {}}, {})['fine']['rgb'].clone()

  def render(table):
    origins, directions = rays_from_table(table, pixels, index)
    viewdirs = directions / directions.norm(dim=-1, keepdim=True)
    out = autograd.render_differentiable(model, fp.flat, {'origins': origins, 'directions': directions, 'viewdirs': viewdirs,
                                                          'metadata': {}})
    return out['coarse']['rgb'], out['fine']['rgb']

  R0, p0 = table0[0, SL['orientation']].reshape(3, 3).clone(), table0[0, SL['position']].clone()
  w_off = torch.tensor([0.02, -0.015, 0.01], device=dev)
  p_off = torch.tensor([0.010, -0.008, 0.006], device=dev)
  R_start = (torch.matrix_exp(hat(w_off.double())) @ R0.double()).float()

  def errors(R, p):
    half = ((R.double() - R0.double()).norm() / (2 * 2 ** 0.5)).clamp(max=1.0)
    return (p - p0).norm().item(), 2 * torch.asin(half).item()

  pos0, rot0 = errors(R_start, p0 + p_off)
  w = torch.zeros(3, device=dev, requires_grad=True)
  t = torch.zeros(3, device=dev, requires_grad=True)
  opt = torch.optim.Adam([w, t], lr=LR)
  for step in range(STEPS + 1):
    R = torch.matrix_exp(hat(w)) @ R_start
    row = torch.cat([R.reshape(9), p0 + p_off + t, table0[0, 12:]])
    table = torch.cat([row[None], table0[1:]], 0)
    rgb_c, rgb_f = render(table)
    loss = ((rgb_c - target) ** 2).mean() + ((rgb_f - target) ** 2).mean()
    if step % 20 == 0 or step == STEPS:
      with torch.no_grad():
        pos, rot = errors(R, p0 + p_off + t)
      print(f'step {step:4d} loss {loss.item():.3e} position error {pos:.6f} ({pos / pos0:.3e}) rotation error {rot:.3e} ({rot / rot0:.3e})',
            flush=True)
    if step == STEPS:
      break
    opt.zero_grad()
    loss.backward()
    opt.step()
  print(f'[existing path] position {pos0:.6f} -> {pos:.6f} ratio {pos / pos0:.4e}; rotation {rot0:.6f} -> {rot:.4e} ratio {rot / rot0:.4e}')


if __name__ == '__main__':
  main()
