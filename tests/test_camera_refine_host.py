"""Camera refinement on the host (no GPU): the header against the ctypes mirrors (NRF_CAMERA_DELTA_ROW, NRF_VERSION, the three new
exports), the workspace sizes of the fused train step with ray gradients next to the regularisers, and the refusals that
nrf_train_step_loss_grad_rays / nrf_camera_table_compose[_backward] decide before any HIP call."""
import ctypes as C
import importlib.util
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'nerfies_amd.h')
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
NRF_E_NULL, NRF_E_SHAPE, NRF_E_UNSUPPORTED = -1, -2, -3   # include/nerfies_amd.h
NEW = ('nrf_train_step_loss_grad_rays', 'nrf_camera_table_compose', 'nrf_camera_table_compose_backward')


@pytest.fixture(scope='module')
def lib():
  from nerfies_amd import build, lib as L
  build.build()
  return L.load_library()


def _maker():
  spec = importlib.util.spec_from_file_location('make_plan_digests', os.path.join(GOLDEN, 'make_plan_digests.py'))
  mod = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(mod)
  return mod


@pytest.fixture()
def warp_handle(lib):
  mk = _maker()
  h = C.c_void_p()
  d = mk.desc(**mk.MODELS['se3_vrig'])
  assert lib.nrf_create(C.byref(d), C.byref(h)) == 0
  yield h
  lib.nrf_destroy(h)


def test_header_and_mirrors_agree(tmp_path, lib):
  from nerfies_amd import lib as L
  cc = shutil.which('gcc') or shutil.which('cc')
  if cc is None:
    pytest.skip('no C compiler')
  lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', 'int main(void) {',
           '  printf("NRF_CAMERA_DELTA_ROW %d\\n", NRF_CAMERA_DELTA_ROW);', '  printf("NRF_VERSION %d\\n", NRF_VERSION);',
           # the exports' prototypes, as the header declares them
           '  int (*f)(nrf_handle, const float*, const nrf_rays*, const float*, const nrf_step_scalars*, const nrf_rand*,'
           ' const nrf_background*, const nrf_elastic*, const nrf_warp_reg*, uint32_t, const nrf_ray_grads*, float*, float*, void*,'
           ' size_t, void*) = nrf_train_step_loss_grad_rays;',
           '  int (*g)(const float*, const float*, int32_t, float*, void*) = nrf_camera_table_compose;',
           '  int (*k)(const float*, const float*, int32_t, const float*, float*, void*) = nrf_camera_table_compose_backward;',
           '  printf("fn %d\\n", f != 0 && g != 0 && k != 0);', '  return 0;', '}',
           'int nrf_train_step_loss_grad_rays(nrf_handle h, const float* p, const nrf_rays* r, const float* t, const nrf_step_scalars* s,'
           ' const nrf_rand* n, const nrf_background* b, const nrf_elastic* e, const nrf_warp_reg* w, uint32_t f, const nrf_ray_grads* q,'
           ' float* gp, float* st, void* ws, size_t wb, void* sm) { (void)h; (void)p; (void)r; (void)t; (void)s; (void)n; (void)b; (void)e;'
           ' (void)w; (void)f; (void)q; (void)gp; (void)st; (void)ws; (void)wb; (void)sm; return 0; }',
           'int nrf_camera_table_compose(const float* c, const float* d, int32_t n, float* o, void* s)'
           ' { (void)c; (void)d; (void)n; (void)o; (void)s; return 0; }',
           'int nrf_camera_table_compose_backward(const float* c, const float* d, int32_t n, const float* g, float* o, void* s)'
           ' { (void)c; (void)d; (void)n; (void)g; (void)o; (void)s; return 0; }']
  src = tmp_path / 'abi.c'
  src.write_text('\n'.join(lines))
  exe = tmp_path / 'abi'
  subprocess.run([cc, '-std=c99', '-Wall', '-Werror', str(src), '-o', str(exe)], check=True)
  got = {}
  for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines():
    k, v = line.split()
    got[k] = int(v)
  assert got['NRF_CAMERA_DELTA_ROW'] == L.NRF_CAMERA_DELTA_ROW == 16
  assert got['NRF_VERSION'] >= 650 and got['NRF_VERSION'] == lib.nrf_version()
  for name in NEW:
    assert name in L.EXPORTS and hasattr(lib, name), name
  from nerfies_amd import camera
  cols = sorted((s.start, s.stop) for s in camera.CAMERA_DELTA_SLICES.values())
  assert cols[0][0] == 0 and cols[-1][1] == 14 and all(a[1] == b[0] for a, b in zip(cols, cols[1:]))   # 14, 15: the pads


def test_workspace_with_ray_grads_and_regularisers(lib, warp_handle):
  from nerfies_amd import lib as L
  T, R = L.NRF_FLAG_TRAIN, L.NRF_FLAG_RAY_GRADS
  size = {}
  for flags, bg, el in ((T | R, 256, 1), (T | R, 0, 1), (T | R, 256, 0), (T | R, 0, 0), (T, 256, 1), (T, 0, 1)):
    n = C.c_size_t(0)
    assert lib.nrf_workspace_bytes_ex(warp_handle, 37, flags, bg, el, C.byref(n)) == 0, (flags, bg, el, lib.nrf_last_error())
    size[flags, bg, el] = n.value
  assert size[T | R, 256, 1] > size[T | R, 0, 0] and size[T | R, 256, 1] > size[T, 256, 1]
  assert size[T | R, 0, 1] > size[T | R, 0, 0] and size[T | R, 0, 1] > size[T, 0, 1]
  assert size[T | R, 256, 0] > size[T | R, 0, 0]
  # without the flag: the sizes recorded before this change (tests/golden/plan_digests.json, which tests/test_plan_digest.py pins)
  with open(os.path.join(GOLDEN, 'plan_digests.json')) as fp:
    rec = json.load(fp)['plans']
  for bg, el in ((256, 1), (0, 1)):
    assert size[T, bg, el] == rec[f'se3_vrig/TRAIN/rays=37/bg={bg}/elastic={el}/rows=0/merge=1']['workspace_bytes'], (bg, el)
  # the bfloat16 modes have no ray gradient, with or without regularisers
  n = C.c_size_t(0)
  assert lib.nrf_workspace_bytes_ex(warp_handle, 37, T | R | L.NRF_FLAG_BF16, 256, 1, C.byref(n)) == NRF_E_UNSUPPORTED


def test_train_step_rays_refusals_decided_on_the_host(lib, warp_handle):
  from nerfies_amd import lib as L
  rays = L.Rays(num_rays=4)
  rg = L.RayGrads()
  buf = (C.c_float * 64)()   # stands in for params / target / grad / workspace: none is touched before the refusal
  p = C.cast(buf, C.c_void_p)
  call = lambda flags, q: lib.nrf_train_step_loss_grad_rays(warp_handle, p, C.byref(rays), p, None, None, None, None, None, flags, q,
                                                            p, p, p, 256, None)
  for flags in (L.NRF_FLAG_BF16, L.NRF_FLAG_BF16 | L.NRF_FLAG_WARP_F32, L.NRF_FLAG_BF16X3):
    assert call(flags, C.byref(rg)) == NRF_E_UNSUPPORTED, flags
    assert b'NRF_FLAG_BF16' in lib.nrf_last_error()
  assert call(L.NRF_FLAG_TRAIN, C.byref(rg)) == NRF_E_UNSUPPORTED   # flags = 0 is the only word
  assert call(0, None) == NRF_E_NULL
  assert b'nrf_ray_grads' in lib.nrf_last_error()
  assert lib.nrf_train_step_loss_grad_rays(None, p, C.byref(rays), p, None, None, None, None, None, 0, C.byref(rg), p, p, p, 256,
                                           None) == NRF_E_NULL
  # d_viewdirs without rays->viewdirs: the view term is part of d_directions
  rg.d_viewdirs = p
  assert call(0, C.byref(rg)) == NRF_E_UNSUPPORTED
  assert b'd_viewdirs' in lib.nrf_last_error()


def test_compose_refusals_decided_on_the_host(lib):
  buf = (C.c_float * 128)()
  base = C.addressof(buf)
  base += (-base) % 16
  a, b, c, d = (C.c_void_p(base + 96 * i) for i in range(4))   # 16-byte aligned stand-ins, never dereferenced
  odd = C.c_void_p(base + 4)
  fwd, bwd = lib.nrf_camera_table_compose, lib.nrf_camera_table_compose_backward
  assert fwd(None, b, 1, c, None) == NRF_E_NULL and fwd(a, None, 1, c, None) == NRF_E_NULL and fwd(a, b, 1, None, None) == NRF_E_NULL
  assert bwd(None, b, 1, c, d, None) == NRF_E_NULL and bwd(a, None, 1, c, d, None) == NRF_E_NULL
  assert bwd(a, b, 1, None, d, None) == NRF_E_NULL and bwd(a, b, 1, c, None, None) == NRF_E_NULL
  for n in (0, -3):
    assert fwd(a, b, n, c, None) == NRF_E_SHAPE and bwd(a, b, n, c, d, None) == NRF_E_SHAPE, n
  for args in ((odd, b, 1, c), (a, odd, 1, c), (a, b, 1, odd)):
    assert fwd(*args, None) == NRF_E_SHAPE, args
    assert b'16-byte' in lib.nrf_last_error()
  for args in ((odd, b, 1, c, d), (a, odd, 1, c, d), (a, b, 1, odd, d), (a, b, 1, c, odd)):
    assert bwd(*args, None) == NRF_E_SHAPE, args
  assert fwd(a, b, 1, a, None) == NRF_E_SHAPE   # out may not alias the base table
