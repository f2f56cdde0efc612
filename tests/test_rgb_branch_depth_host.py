"""ModelConfig.nerf_rgb_branch_depth > 1 (configs.py:55, modules.py:129-134) on the host: the oracle against arrays the unmodified
reference produced with a deeper colour branch (tests/golden/make_reference_vectors_rgb_depth.py), and what the C-ABI accepts,
lays out and plans for such a model.  No GPU: nrf_create / nrf_param_layout / nrf_workspace_bytes_ex run on the host."""
import ctypes as C
import importlib.util
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import nerfies_oracle as O  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
NRF_E_UNSUPPORTED = -3   # include/nerfies_amd.h

COMMON = dict(num_coarse_samples=8, num_fine_samples=6, num_nerf_point_freqs=4, use_stratified_sampling=True)
RGB_DEPTH_CASES = {   # tests/golden/make_reference_vectors_rgb_depth.py::RGB_DEPTH_CASES
    'rgbdepth2': (dict(nerf_rgb_branch_depth=2, use_camera_metadata=True), 0.0),
    'rgbdepth3_w72x40': (dict(nerf_rgb_branch_depth=3, nerf_trunk_width=72, nerf_rgb_branch_width=40), 0.0),
    'rgbdepth2_nocond': (dict(nerf_rgb_branch_depth=2, use_viewdirs=False), 0.0),
    'rgbdepth2_warp_alphacond': (dict(nerf_rgb_branch_depth=2, use_warp=True, num_warp_freqs=4, use_appearance_metadata=True,
                                      use_alpha_condition=True), 2.5),
}


def _ref(name):
  return dict(np.load(os.path.join(GOLDEN, f'ref_{name}.npz'), allow_pickle=False))


def _close(got, want, tol, msg):
  got = got.detach().numpy() if torch.is_tensor(got) else np.asarray(got)
  err = float(np.abs(got - np.asarray(want).reshape(got.shape)).max())
  assert err <= tol, (msg, err)
  return err


@pytest.mark.parametrize('name', sorted(RGB_DEPTH_CASES))
def test_oracle_against_the_reference_run_with_a_deeper_rgb_branch(name):
  """NerfModel.apply by the unmodified reference at nerf_rgb_branch_depth 2 and 3 -- with a camera code, on a 72-wide trunk with a
  40-wide branch, without any condition, with the SE3 warp and use_alpha_condition -- against the oracle on the same rays,
  parameters and uniforms.  Tolerances of test_reference_vectors.py::test_nerf_model_with_moved_skips_and_warp_kwargs."""
  kw, alpha = RGB_DEPTH_CASES[name]
  r = _ref('nerf_' + name)
  spec = O.ModelSpec(**COMMON, **kw)
  seed = int(r['seed'])
  assert seed == sum(ord(c) for c in name) and float(r['alpha']) == alpha
  params = O.init_params(spec, seed=seed, trained_like=True)
  D, w = spec.nerf_rgb_branch_depth, spec.nerf_rgb_branch_width
  for lv in ('nerf_mlps_coarse', 'nerf_mlps_fine'):   # hidden_0 (W + R, w), hidden_1.. (w, w), logit (w, 3): modules.py:41-50
    rgb = params[lv]['MLP_1']
    assert sorted(rgb) == sorted([f'hidden_{i}' for i in range(D)] + ['logit'])
    assert tuple(rgb['hidden_0']['kernel'].shape) == (spec.nerf_trunk_width + spec.rgb_cond_width, w)
    assert all(tuple(rgb[f'hidden_{i}']['kernel'].shape) == (w, w) for i in range(1, D))
    assert tuple(rgb['logit']['kernel'].shape) == (w, 3)
  batch = O.synthetic_batch(3, seed=seed + 1)
  T = lambda a: torch.tensor(a, dtype=torch.float64)
  ret = O.nerf_model_apply(params, spec, batch, alpha, return_points=spec.use_warp, t_rand=T(r['t_rand']), u=T(r['u']))
  worst = 0.0
  for lv in ('coarse', 'fine'):
    for k in ('rgb', 'depth', 'med_depth', 'acc', 'weights'):
      worst = max(worst, _close(ret[lv][k], r[f'{lv}/{k}'], 1e-8, f'{name} {lv}/{k}'))
    if spec.use_warp:
      worst = max(worst, _close(ret[lv]['warped_points'], r[f'{lv}/warped_points'], 1e-9, f'{name} {lv}/warped_points'))
  print(f'{name}: max |oracle - reference| {worst:.2e}')


# ---- the C-ABI on the host ----
def _maker():
  spec = importlib.util.spec_from_file_location('make_plan_digests', os.path.join(GOLDEN, 'make_plan_digests.py'))
  mod = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(mod)
  return mod


@pytest.fixture(scope='module')
def lib():
  from nerfies_amd import build, lib as L
  build.build()          # hipcc cross-compiles gfx950 without a GPU; no-op when up to date
  return L.load_library()


def _create(lib, **kw):
  h = C.c_void_p()
  d = _maker().desc(**kw)
  rc = lib.nrf_create(C.byref(d), C.byref(h))
  return rc, h


def test_nrf_create_accepts_rgb_branch_depth_1_to_4(lib):
  for depth in (1, 2, 3, 4):
    rc, h = _create(lib, nerf_rgb_branch_depth=depth)
    assert rc == 0, (depth, lib.nrf_last_error().decode())
    assert lib.nrf_destroy(h) == 0
  for depth in (0, 5):
    rc, _ = _create(lib, nerf_rgb_branch_depth=depth)
    msg = lib.nrf_last_error().decode()
    assert rc == NRF_E_UNSUPPORTED, (depth, rc)
    assert 'nerf_rgb_branch_depth' in msg and '[1,4]' in msg, msg


def test_param_layout_at_depth_3_is_the_flax_tree(lib):
  """Names, order and shapes of nrf_param_layout = the leaves of the oracle's (= the reference's) tree; 72-wide trunk, 40-wide branch."""
  from nerfies_amd import lib as L
  spec = O.ModelSpec(nerf_rgb_branch_depth=3, nerf_trunk_width=72, nerf_rgb_branch_width=40)
  rc, h = _create(lib, nerf_rgb_branch_depth=3, nerf_trunk_width=72, nerf_rgb_branch_width=40)
  assert rc == 0, lib.nrf_last_error().decode()
  n = C.c_int32(0)
  assert lib.nrf_param_layout(h, None, C.byref(n)) == 0
  infos = (L.TensorInfo * n.value)()
  assert lib.nrf_param_layout(h, infos, C.byref(n)) == 0
  got = [(t.name.decode(), (t.cols,) if t.name.decode().endswith('/bias') else (t.rows, t.cols)) for t in infos]
  want = [(path, tuple(leaf.shape)) for path, leaf in O.tree_leaves_with_path(O.init_params(spec))]
  assert got == want
  assert ('nerf_mlps_fine/MLP_1/hidden_2/kernel', (40, 40)) in got and ('nerf_mlps_coarse/MLP_1/hidden_1/bias', (40,)) in got
  total = C.c_int64(0)
  assert lib.nrf_param_count(h, C.byref(total)) == 0
  # the flat buffer holds exactly the tree's elements, every leaf 16-byte aligned (the 3- and 1-element logit biases are followed
  # by padding): leaf after leaf at the running offset, the count = the end of the last one
  off = 0
  for t, (path, shape) in zip(infos, want):
    assert t.offset == off, path
    off += (math.prod(shape) + 3) // 4 * 4
  assert total.value == off
  assert sum(math.prod(s) for _, s in want) <= off < sum(math.prod(s) for _, s in want) + 4 * len(want)
  assert lib.nrf_destroy(h) == 0


def test_workspace_plans_and_refused_modes_at_depth_2(lib):
  from nerfies_amd import lib as L
  B = 1024
  rc, h = _create(lib, nerf_rgb_branch_depth=2)
  assert rc == 0
  rc, h1 = _create(lib, nerf_rgb_branch_depth=1)
  assert rc == 0
  size = {}
  for hh, key in ((h, 2), (h1, 1)):
    for flags in (0, L.NRF_FLAG_TRAIN):
      n = C.c_size_t(0)
      assert lib.nrf_workspace_bytes_ex(hh, B, flags, 0, 0, C.byref(n)) == 0, lib.nrf_last_error().decode()
      assert n.value > 0
      size[key, flags] = n.value
  for flags in (L.NRF_FLAG_BF16, L.NRF_FLAG_BF16X3, L.NRF_FLAG_TRAIN | L.NRF_FLAG_BF16):
    n = C.c_size_t(0)
    assert lib.nrf_workspace_bytes_ex(h, B, flags, 0, 0, C.byref(n)) == NRF_E_UNSUPPORTED, flags
    msg = lib.nrf_last_error().decode()
    assert 'rgb branch' in msg and 'nerf_rgb_branch_depth' in msg and 'use the float32 mode' in msg, msg
    assert lib.nrf_workspace_bytes_ex(h1, B, flags, 0, 0, C.byref(n)) == 0   # the one-layer branch keeps every mode
  # the extra layer's activation stash and adjoint: 2 x [ntiles][128][64] floats per level (64 + 192 samples per ray)
  ntiles = B * 64 // 64 + B * 192 // 64
  assert size[2, L.NRF_FLAG_TRAIN] - size[1, L.NRF_FLAG_TRAIN] >= 2 * ntiles * 128 * 64 * 4
  # (the inference plan may be SMALLER than the one-layer model's: it holds the two packed 128 x 128 images per level, but none of the
  # bfloat16 / split-bf16 weight streams, which are not built for a handle that cannot run them)
  assert lib.nrf_destroy(h) == 0 and lib.nrf_destroy(h1) == 0


def test_the_32_row_tiling_is_refused_at_depth_2(lib):
  """A deeper rgb branch exists in the 64-row chains only: the plan keeps them at every launch size and the option says so."""
  from nerfies_amd import lib as L
  rc, h = _create(lib, nerf_rgb_branch_depth=2)
  assert rc == 0
  assert lib.nrf_set_option(h, L.NRF_OPT_CHAIN_TILE_ROWS, 32) == NRF_E_UNSUPPORTED
  msg = lib.nrf_last_error().decode()
  assert 'nerf_rgb_branch_depth' in msg and '64-row' in msg, msg
  assert lib.nrf_set_option(h, L.NRF_OPT_CHAIN_TILE_ROWS, 64) == 0
  assert lib.nrf_set_option(h, L.NRF_OPT_CHAIN_TILE_ROWS, 0) == 0
  assert lib.nrf_destroy(h) == 0
  rc, h1 = _create(lib, nerf_rgb_branch_depth=1)
  assert rc == 0 and lib.nrf_set_option(h1, L.NRF_OPT_CHAIN_TILE_ROWS, 32) == 0
  assert lib.nrf_destroy(h1) == 0
