#!/usr/bin/env python
"""tests/golden/plan_digests.json: the workspace plan of every configuration `cases()` lists -- its nrf_debug_plan_digest and
its nrf_workspace_bytes_ex --, or "refused" where the flag check rejects the combination.  The record pins the planner
(csrc/nrf_plan.hip): moving a buffer, a descriptor or a stream-K cut changes a digest.  tests/test_plan_digest.py compares a
fresh build against it.  Planning runs on the host; the plan depends on the CU count, and the record assumes 256 (the handle's
default when no device is visible, and the MI355X's count).

  python tests/golden/make_plan_digests.py
"""
import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from nerfies_amd import lib as L  # noqa: E402

OUT = os.path.join(HERE, 'plan_digests.json')
NRF_E_UNSUPPORTED = -3   # include/nerfies_amd.h

_WARP = dict(use_warp=1, num_warp_freqs=8, num_warp_embeddings=4, num_warp_features=8)
MODELS = {
    'A': {},                                                                       # no warp, 64 + 128 samples
    'se3_vrig': dict(_WARP, use_appearance_metadata=1, num_appearance_embeddings=4, num_appearance_features=8,
                     use_camera_metadata=1, num_camera_embeddings=2, num_camera_features=2),
    'time_warp': dict(_WARP, warp_metadata_encoder_type=L.META_ENCODER['time'], num_time_encoder_freqs=1),
    'translation': dict(_WARP, warp_field_type=L.WARP_FIELD['translation']),
    'alpha_cond': dict(use_appearance_metadata=1, num_appearance_embeddings=4, num_appearance_features=8, use_alpha_condition=1),
    'no_cond': dict(use_viewdirs=0),                                               # R = 0, A = 0
    'narrow': dict(nerf_trunk_width=128, nerf_rgb_branch_width=64),                # the padded (embed) path
    'skip5': dict(nerf_skip_layer=5),                                              # the moved skip: float32 modes only
    'depth3': dict(nerf_trunk_depth=3),
    'one_level': dict(num_fine_samples=0),
    'warp_trunk4x64': dict(_WARP, warp_trunk_depth=4, warp_trunk_width=64),
}
_T, _BF, _WF, _X3 = L.NRF_FLAG_TRAIN, L.NRF_FLAG_BF16, L.NRF_FLAG_WARP_F32, L.NRF_FLAG_BF16X3
FLAGS = {'0': 0, 'NO_WARP': L.NRF_FLAG_NO_WARP, 'WARP_JACOBIAN': L.NRF_FLAG_WARP_JACOBIAN, 'BF16': _BF, 'BF16|WARP_F32': _BF | _WF,
         'BF16X3': _X3, 'BF16X3|WARP_F32': _X3 | _WF, 'TRAIN': _T, 'TRAIN|BF16': _T | _BF, 'TRAIN|BF16|WARP_F32': _T | _BF | _WF}
RAYS = (1024, 128, 37)   # 128: the automatic 32-row forward tiling; 37: a ragged last tile


def desc(**kw):
  d = L.ModelDesc(num_coarse_samples=64, num_fine_samples=128, use_viewdirs=1, near_plane=0.02, far_plane=0.8,
                  nerf_trunk_depth=8, nerf_trunk_width=256, nerf_rgb_branch_depth=1, nerf_rgb_branch_width=128,
                  nerf_skip_layer=4, use_stratified_sampling=1, num_nerf_point_freqs=8, num_nerf_viewdir_freqs=4,
                  sigma_activation=1, use_sample_at_infinity=1)
  for k, v in kw.items():
    setattr(d, k, v)
  return d


def cases(model):
  """(name, flags, num_rays, num_background_points, use_elastic_loss, chain_tile_rows, bf16_wgrad_merge) of one model: training
  plans under every option, warp models with and without the background / elastic buffers."""
  warp = MODELS[model].get('use_warp', 0)
  for fname, flags in FLAGS.items():
    train = bool(flags & _T)
    extras = [(bg, el) for bg in (0, 256) for el in (0, 1)] if train and warp else [(0, 0)]
    options = [(rows, merge) for rows in (0, 32, 64) for merge in (0, 1)] if train else [(0, 1)]
    for rays in RAYS:
      for bg, el in extras:
        for rows, merge in options:
          yield f'{model}/{fname}/rays={rays}/bg={bg}/elastic={el}/rows={rows}/merge={merge}', flags, rays, bg, el, rows, merge


def plans(lib):
  """{case: {'digest', 'workspace_bytes'} or 'refused'} over every model."""
  out = {}
  for model, kw in MODELS.items():
    h = C.c_void_p()
    d = desc(**kw)
    L.check(lib.nrf_create(C.byref(d), C.byref(h)), lib)
    try:
      for name, flags, rays, bg, el, rows, merge in cases(model):
        L.check(lib.nrf_set_option(h, L.NRF_OPT_CHAIN_TILE_ROWS, rows), lib)
        L.check(lib.nrf_set_option(h, L.NRF_OPT_BF16_WGRAD_MERGE, merge), lib)
        n = C.c_size_t(0)
        rc = lib.nrf_workspace_bytes_ex(h, rays, flags, bg, el, C.byref(n))
        if rc == NRF_E_UNSUPPORTED:
          out[name] = 'refused'
          continue
        L.check(rc, lib)
        dg = C.c_uint64(0)
        L.check(lib.nrf_debug_plan_digest(h, C.byref(dg)), lib)
        out[name] = {'digest': '%016x' % dg.value, 'workspace_bytes': n.value}
    finally:
      lib.nrf_destroy(h)
  return out


def main():
  from nerfies_amd import build
  build.build()
  rec = plans(L.load_library())
  with open(OUT, 'w') as fp:
    json.dump({'num_cus': 256, 'plans': rec}, fp, indent=0, sort_keys=True)
    fp.write('\n')
  print('wrote', len(rec), 'plans')


if __name__ == '__main__':
  main()
