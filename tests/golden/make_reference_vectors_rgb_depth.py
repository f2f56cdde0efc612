#!/usr/bin/env python
"""Golden vectors for ModelConfig.nerf_rgb_branch_depth > 1 (configs.py:55, models.py:83,167,178, modules.py:129-134) from the REAL
reference sources, in the manner of make_reference_vectors.py::nerf_model_r6: NerfModel.apply by the unmodified reference on NumPy
float64 through oracle/_shim, on 3 rays with seeded `trained_like` parameters and explicit uniforms.

make_reference_vectors.build_ref_model hard-codes a one-layer rgb branch of width 128 on a 256-wide trunk, so this file builds
ref_models.NerfModel itself with the depth / widths of the spec.  Runs only where the reference lies (the build container); writes
tests/golden/ref_nerf_rgbdepth*.npz, which tests/test_rgb_branch_depth_host.py replays against oracle/nerfies_oracle.py and
tests/test_gpu_rgb_branch_depth.py against the HIP library.  No reference source is copied.

  python tests/golden/make_reference_vectors_rgb_depth.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import make_reference_vectors as M  # noqa: E402  (import-safe: sets up the shim and the reference on sys.path)

O = M.O

COMMON = dict(num_coarse_samples=8, num_fine_samples=6, num_nerf_point_freqs=4, use_stratified_sampling=True)
RGB_DEPTH_CASES = {   # name -> (ModelSpec keywords on top of COMMON, warp alpha)
    'rgbdepth2': (dict(nerf_rgb_branch_depth=2, use_camera_metadata=True), 0.0),
    'rgbdepth3_w72x40': (dict(nerf_rgb_branch_depth=3, nerf_trunk_width=72, nerf_rgb_branch_width=40), 0.0),
    'rgbdepth2_nocond': (dict(nerf_rgb_branch_depth=2, use_viewdirs=False), 0.0),
    'rgbdepth2_warp_alphacond': (dict(nerf_rgb_branch_depth=2, use_warp=True, num_warp_freqs=4, use_appearance_metadata=True,
                                      use_alpha_condition=True), 2.5),
}


def build_ref_model(spec):
  return M.ref_models.NerfModel(
      num_coarse_samples=spec.num_coarse_samples, num_fine_samples=spec.num_fine_samples, use_viewdirs=spec.use_viewdirs,
      near=spec.near, far=spec.far, noise_std=spec.noise_std, nerf_trunk_depth=spec.nerf_trunk_depth,
      nerf_trunk_width=spec.nerf_trunk_width, nerf_rgb_branch_depth=spec.nerf_rgb_branch_depth,
      nerf_rgb_branch_width=spec.nerf_rgb_branch_width, nerf_skips=tuple(spec.nerf_skips), alpha_channels=1, rgb_channels=3,
      use_stratified_sampling=spec.use_stratified_sampling, num_nerf_point_freqs=spec.num_nerf_point_freqs,
      num_nerf_viewdir_freqs=spec.num_nerf_viewdir_freqs, appearance_ids=tuple(range(spec.num_appearance_embeddings)),
      camera_ids=tuple(range(spec.num_camera_embeddings)), warp_ids=tuple(range(spec.num_warp_embeddings)),
      num_appearance_features=spec.num_appearance_features, num_camera_features=spec.num_camera_features,
      num_warp_features=spec.num_warp_features, num_warp_freqs=spec.num_warp_freqs, sigma_activation=M.nn.softplus,
      use_camera_metadata=spec.use_camera_metadata, use_warp=spec.use_warp, warp_field_type=spec.warp_field_type,
      use_appearance_metadata=spec.use_appearance_metadata, use_alpha_condition=spec.use_alpha_condition)


def nerf_model_rgb_depth():
  for name, (kw, alpha) in RGB_DEPTH_CASES.items():
    spec = O.ModelSpec(**COMMON, **kw)
    seed = sum(ord(c) for c in name)
    params = O.init_params(spec, seed=seed, trained_like=True)
    batch = O.synthetic_batch(3, seed=seed + 1)
    rng = np.random.default_rng(seed + 2)
    t_rand = rng.uniform(0, 1, (3, spec.num_coarse_samples)); u = rng.uniform(0, 1, (3, spec.num_fine_samples))
    model = build_ref_model(spec)
    rays = {'origins': batch['origins'].numpy(), 'directions': batch['directions'].numpy(),
            'metadata': {k: v.numpy() for k, v in batch['metadata'].items()}}
    ret = model.apply({'params': M.tree_np(params)}, rays, {'alpha': alpha, 'time_alpha': 0.0}, return_points=spec.use_warp,
                      return_weights=True, rngs={'coarse': M.jrandom.Key(uniform=t_rand), 'fine': M.jrandom.Key(uniform=u)})
    out = dict(t_rand=t_rand, u=u, alpha=alpha, seed=seed)
    for lv, d in ret.items():
      for k, v in d.items():
        out[f'{lv}/{k}'] = v
    M.save('nerf_' + name, **out)


if __name__ == '__main__':
  nerf_model_rgb_depth()
