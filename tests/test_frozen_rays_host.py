"""Frozen-field ray gradients on the host (no GPU): NRF_FLAG_FROZEN and nrf_loss_grad_rays against the compiled header, every refused
flag word, the frozen plan's size against the ray-gradient plan it narrows (both test shapes, config A, config D; the byte counts are
recorded in profiles/frozen_rays.md), what the frozen plan drops -- read off the plan, not off machine code -- and the Python names."""
import ctypes as C
import os
import shutil
import subprocess
import types

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'nerfies_amd.h')
NRF_E_NULL, NRF_E_UNSUPPORTED, NRF_E_STATE = -1, -3, -6   # include/nerfies_amd.h

# the shapes of tests/test_gpu_frozen_rays.py, config A (1024 rays x (64 + 128), no warp), the gpu_vrig_paper shape (768 x (128 + 128),
# SE3 warp) and config D (4096 rays x (128 + 128), SE3 warp)
NOWARP = dict(num_coarse_samples=24, num_fine_samples=56, nerf_trunk_width=64, num_nerf_point_freqs=4)
WARP = dict(num_coarse_samples=16, num_fine_samples=16, nerf_trunk_width=64, num_nerf_point_freqs=4, use_warp=True, num_warp_freqs=4,
            warp_field_type='se3')
CONFIG_A = dict(num_coarse_samples=64, num_fine_samples=128, num_nerf_point_freqs=8)
VRIG = dict(num_coarse_samples=128, num_fine_samples=128, num_nerf_point_freqs=8, use_warp=True, num_warp_freqs=8, warp_field_type='se3')
SHAPES = {'test no-warp (7 rays)': (NOWARP, 7), 'test warp (5 rays)': (WARP, 5), 'config A (1024 rays)': (CONFIG_A, 1024),
          'vrig (768 rays, warp)': (VRIG, 768), 'config D (4096 rays, warp)': (VRIG, 4096)}


@pytest.fixture(scope='module')
def lib():
  from nerfies_amd import build, lib as L
  build.build()
  return L.load_library()


def _model(**kw):
  from nerfies_amd import models
  kw.setdefault('use_stratified_sampling', False)
  model, _ = models.construct_nerf(0, types.SimpleNamespace(**kw), 4, [0], [0], [0, 1], 0.1, 1.0, device='cpu')
  return model


def _bytes(lib, model, num_rays, flags):
  n = C.c_size_t(0)
  assert lib.nrf_workspace_bytes(model.handle, num_rays, flags, C.byref(n)) == 0, lib.nrf_last_error()
  return n.value


def test_header_ctypes_and_version_agree(tmp_path, lib):
  from nerfies_amd import lib as L
  cc = shutil.which('gcc') or shutil.which('cc')
  if cc is None:
    pytest.skip('no C compiler')
  proto = ('nrf_handle h, const float* p, const nrf_rays* r, const float* t, const nrf_step_scalars* s, const nrf_rand* q, '
           'const nrf_ray_grads* g, float* st, void* w, size_t n, void* stream')
  lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"',
           f'int nrf_loss_grad_rays({proto}) {{ (void)h; (void)p; (void)r; (void)t; (void)s; (void)q; (void)g; (void)st; (void)w; (void)n; '
           '(void)stream; return 0; }',   # a definition with the mirrored prototype: a mismatch with the header's does not compile
           'int main(void) {', '  printf("NRF_FLAG_FROZEN %u\\n", NRF_FLAG_FROZEN);', '  printf("NRF_VERSION %d\\n", NRF_VERSION);',
           '  printf("NRF_NUM_STATS %d\\n", NRF_NUM_STATS);', '  return 0;', '}']
  src = tmp_path / 'abi.c'
  src.write_text('\n'.join(lines))
  exe = tmp_path / 'abi'
  subprocess.run([cc, '-std=c99', '-Wall', '-Werror', str(src), '-o', str(exe)], check=True)
  got = dict((k, int(v)) for k, v in (line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True,
                                                                                text=True).stdout.splitlines()))
  assert got['NRF_FLAG_FROZEN'] == L.NRF_FLAG_FROZEN == 128
  assert got['NRF_VERSION'] == L.NRF_VERSION == lib.nrf_version() == 660
  assert got['NRF_NUM_STATS'] == L.NRF_NUM_STATS
  assert 'nrf_loss_grad_rays' in L.EXPORTS and len(lib.nrf_loss_grad_rays.argtypes) == 11   # the eleven arguments of the prototype above


def test_every_other_word_with_the_flag_is_refused(lib):
  from nerfies_amd import lib as L
  T, R, F = L.NRF_FLAG_TRAIN, L.NRF_FLAG_RAY_GRADS, L.NRF_FLAG_FROZEN
  model, warp = _model(**NOWARP), _model(**WARP)
  n = C.c_size_t(0)
  refused = (F, T | F, R | F, T | R | F | L.NRF_FLAG_BF16, T | R | F | L.NRF_FLAG_BF16 | L.NRF_FLAG_WARP_F32, T | R | F | L.NRF_FLAG_BF16X3,
             R | F | L.NRF_FLAG_BF16X3, T | R | F | L.NRF_FLAG_WARP_JACOBIAN, F | L.NRF_FLAG_WARP_JACOBIAN)
  for m in (model, warp):
    for flags in refused:
      assert lib.nrf_workspace_bytes(m.handle, 4, flags, C.byref(n)) == NRF_E_UNSUPPORTED, flags
      assert b'NRF_FLAG_FROZEN' in lib.nrf_last_error(), (flags, lib.nrf_last_error())
      assert lib.nrf_workspace_bytes_ex(m.handle, 4, flags, 0, 0, C.byref(n)) == NRF_E_UNSUPPORTED, flags
      assert b'NRF_FLAG_FROZEN' in lib.nrf_last_error(), (flags, lib.nrf_last_error())
    assert lib.nrf_workspace_bytes(m.handle, 4, T | R | F, C.byref(n)) == 0 and n.value > 0
    assert lib.nrf_workspace_bytes_ex(m.handle, 4, T | R | F, 0, 0, C.byref(n)) == 0 and n.value > 0
  # no regulariser in a frozen plan
  for bg, el in ((16, 0), (0, 1), (16, 1)):
    assert lib.nrf_workspace_bytes_ex(warp.handle, 4, T | R | F, bg, el, C.byref(n)) == NRF_E_UNSUPPORTED, (bg, el)
    assert b'NRF_FLAG_FROZEN' in lib.nrf_last_error()
  # nrf_forward refuses the same words before it looks at anything else; the fused train steps take no such word
  rays = L.Rays(num_rays=4)
  buf = (C.c_float * 64)()
  p = C.cast(buf, C.c_void_p)
  assert lib.nrf_forward(model.handle, p, C.byref(rays), None, None, None, T | F, p, 256, None) == NRF_E_UNSUPPORTED
  assert b'NRF_FLAG_FROZEN' in lib.nrf_last_error()
  assert lib.nrf_train_step_loss_grad_ex(model.handle, p, C.byref(rays), p, None, None, None, None, None, F, p, p, p, 256, None) == NRF_E_UNSUPPORTED
  rg = L.RayGrads()
  assert lib.nrf_train_step_loss_grad_rays(model.handle, p, C.byref(rays), p, None, None, None, None, None, F, C.byref(rg), p, p, p, 256,
                                           None) == NRF_E_UNSUPPORTED
  # the existing refusals are what they were
  assert lib.nrf_workspace_bytes(model.handle, 4, R, C.byref(n)) == NRF_E_UNSUPPORTED and b'NRF_FLAG_RAY_GRADS' in lib.nrf_last_error()
  assert lib.nrf_workspace_bytes(model.handle, 4, T | R | L.NRF_FLAG_BF16, C.byref(n)) == NRF_E_UNSUPPORTED
  assert b'NRF_FLAG_RAY_GRADS' in lib.nrf_last_error()
  # nrf_loss_grad_rays: NULL ray_grads, and a d_viewdirs the rays cannot carry, before any launch
  assert lib.nrf_loss_grad_rays(model.handle, p, C.byref(rays), p, None, None, None, p, p, 256, None) == NRF_E_NULL
  rg.d_viewdirs = C.cast(buf, C.c_void_p).value
  assert lib.nrf_loss_grad_rays(model.handle, p, C.byref(rays), p, None, None, C.byref(rg), p, p, 256, None) == NRF_E_UNSUPPORTED
  assert b'd_viewdirs' in lib.nrf_last_error()


@pytest.mark.parametrize('name', list(SHAPES))
def test_frozen_plan_is_smaller_and_has_no_wgrad_segments(lib, name):
  from nerfies_amd import lib as L
  T, R, F = L.NRF_FLAG_TRAIN, L.NRF_FLAG_RAY_GRADS, L.NRF_FLAG_FROZEN
  kw, num_rays = SHAPES[name]
  model = _model(**kw)
  h = model.handle
  train, full = _bytes(lib, model, num_rays, T), _bytes(lib, model, num_rays, T | R)
  nseg = C.c_int32(-1)
  assert lib.nrf_debug_wgrad_segments(h, None, None, C.byref(nseg)) == 0 and nseg.value > 0   # the ray-gradient plan cuts its wgrad work
  frozen = _bytes(lib, model, num_rays, T | R | F)
  assert lib.nrf_debug_wgrad_segments(h, None, None, C.byref(nseg)) == 0 and nseg.value == 0
  print(f'[frozen plan] {name}: TRAIN {train}, TRAIN|RAY_GRADS {full}, TRAIN|RAY_GRADS|FROZEN {frozen} bytes '
        f'({frozen / full:.3f} of the ray-gradient plan)')
  assert 0 < frozen < full
  # what the plan keeps has an offset of its own inside the workspace; what it drops was never laid out (offset 0)
  off = C.c_int64(-1)

  def offset(buf, level):
    assert lib.nrf_debug_ws_offset(h, buf.encode(), level, C.byref(off)) == 0, buf
    return off.value
  warp = bool(kw.get('use_warp'))
  for lv in (0, 1):
    for buf in ('st_pe', 'bits_trunk', 'bits_rgbh', 'd_raw4', 'out4', 'z', 'd_points') + (('w_st_win', 'w_st_wv', 'w_bits', 'wpoints') if warp else ()):
      assert 0 < offset(buf, lv) < frozen // 4, (buf, lv)
    for buf in ('st_h', 'st_bn', 'st_rgbh', 'st_rgbx', 'dy_trunk', 'dy_bn', 'dy_rgbh', 'dy_rgbx', 'w_st_h', 'w_dy', 'w_dw4', 'w_dv4'):
      assert offset(buf, lv) == 0, (buf, lv)
  if warp:   # the tangent level keeps its (dw, dv) rows alone
    assert 0 < offset('w_st_wv', 3) < frozen // 4 and offset('w_st_win', 3) == 0 and offset('w_st_h', 3) == 0
  # ... and the plans without the flag are what they were, in either order
  assert _bytes(lib, model, num_rays, T | R) == full and _bytes(lib, model, num_rays, T) == train


def test_deep_rgb_branch_keeps_its_sign_words_only(lib):
  from nerfies_amd import lib as L
  model = _model(nerf_rgb_branch_depth=2, **NOWARP)
  _bytes(lib, model, 7, L.NRF_FLAG_TRAIN | L.NRF_FLAG_RAY_GRADS | L.NRF_FLAG_FROZEN)
  off = C.c_int64(-1)
  for lv in (0, 1):
    assert lib.nrf_debug_ws_offset(model.handle, b'bits_rgbx', lv, C.byref(off)) == 0 and off.value > 0
    for buf in (b'st_rgbx', b'dy_rgbx'):
      assert lib.nrf_debug_ws_offset(model.handle, buf, lv, C.byref(off)) == 0 and off.value == 0, buf


def test_backward_entries_without_a_stash(lib):
  """Nothing was stashed: nrf_backward_rays with grad_params NULL stays the NULL-argument error it was (only a frozen stash takes it)."""
  from nerfies_amd import lib as L
  model = _model(**NOWARP)
  rays = L.Rays(num_rays=4)
  og, rg = L.OutputGrads(), L.RayGrads()
  buf = (C.c_float * 64)()
  p = C.cast(buf, C.c_void_p)
  assert lib.nrf_backward_rays(model.handle, p, C.byref(rays), C.byref(og), C.byref(rg), None, p, 256, None) == NRF_E_NULL
  assert lib.nrf_backward_ex(model.handle, p, C.byref(rays), C.byref(og), None, p, 256, None) == NRF_E_NULL
  assert lib.nrf_backward_rays(model.handle, p, C.byref(rays), C.byref(og), C.byref(rg), p, p, 256, None) == NRF_E_STATE


def test_python_flag_word_and_workspace_cache():
  from nerfies_amd import lib as L
  model = _model(**NOWARP)
  T, R, F = L.NRF_FLAG_TRAIN, L.NRF_FLAG_RAY_GRADS, L.NRF_FLAG_FROZEN
  assert model.flags(True, ray_grads=True, frozen=True) == T | R | F
  assert model.flags(True, False, False, False, True) == T | R   # the positional calls of before
  assert model.flags(True, ray_grads=True) == T | R and model.flags() == 0
  a = model._record(7, T | R | F, 'cpu')
  b = model._record(7, T | R, 'cpu')
  assert a.flags == T | R | F and b.flags == T | R
  assert a.ws.data_ptr() != b.ws.data_ptr() and a.ws.numel() < b.ws.numel()   # a tensor of its own, sized for the frozen plan
  assert model._record(7, T | R | F, 'cpu').ws.data_ptr() == a.ws.data_ptr()   # ... handed out again for the same word
  with pytest.raises(L.NrfError, match='NRF_FLAG_FROZEN'):
    model._record(7, T | F, 'cpu')
  import inspect
  from nerfies_amd import training
  assert list(inspect.signature(model.loss_and_ray_grads).parameters) == ['fp', 'batch', 'warp_extra', 'rngs', 'ray_grads', 'ray_grads_out',
                                                                          'stats_out', 'dynamic']
  assert list(inspect.signature(training.align_step).parameters)[:7] == ['model', 'params', 'batch', 'refiner', 'warp_extra', 'rng_key',
                                                                         'learning_rate']
  assert inspect.signature(training.align_cameras).parameters['learning_rate'].default == 2e-3
