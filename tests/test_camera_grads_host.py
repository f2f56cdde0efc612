"""Camera tables on the host (no GPU): the nrf_camera_table_* entry points are exported and bound, size their workspace, refuse bad
arguments before any HIP call, and the Python packing follows the header's field order (include/nerfies_amd.h, NRF_CAMERA_ROW)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'nerfies_amd.h')
NEW = ('nrf_camera_table_rays', 'nrf_camera_table_rays_backward', 'nrf_camera_table_project', 'nrf_camera_table_project_backward',
       'nrf_camera_table_workspace_bytes')
NRF_E_NULL, NRF_E_SHAPE, NRF_E_WORKSPACE = -1, -2, -5


@pytest.fixture(scope='module')
def lib():
  from nerfies_amd import build, lib as L
  build.build()
  return L.load_library()


def _ws_bytes(lib, n, c):
  b = C.c_size_t(0)
  assert lib.nrf_camera_table_workspace_bytes(n, c, C.byref(b)) == 0, lib.nrf_last_error()
  return b.value


def test_new_symbols_are_exported_and_bound(lib):
  from nerfies_amd import lib as L
  raw = C.CDLL(lib._name)
  src = open(HEADER).read()
  for name in NEW:
    assert hasattr(raw, name) and name in L.EXPORTS, name
    assert getattr(lib, name).argtypes is not None and getattr(lib, name).restype is C.c_int, name
    assert re.search(r'\bint %s\(' % name, src), name
  assert '#define NRF_CAMERA_ROW %d' % L.NRF_CAMERA_ROW in src and '#define NRF_CAMERA_NPARAMS %d' % L.NRF_CAMERA_NPARAMS in src
  assert lib.nrf_version() >= 640


def test_workspace_bytes_is_positive_and_monotone(lib):
  sizes = [[_ws_bytes(lib, n, c) for n in (0, 1, 255, 256, 257, 6144, 49152, 518400)] for c in (1, 3, 64, 512)]
  for row in sizes:
    assert all(v > 0 for v in row) and all(a <= b for a, b in zip(row, row[1:])), row
  for lo, hi in zip(sizes, sizes[1:]):
    assert all(a <= b for a, b in zip(lo, hi))
  b = C.c_size_t(0)
  assert lib.nrf_camera_table_workspace_bytes(-1, 1, C.byref(b)) == NRF_E_SHAPE
  assert lib.nrf_camera_table_workspace_bytes(4, 0, C.byref(b)) == NRF_E_SHAPE
  assert lib.nrf_camera_table_workspace_bytes(4, 1, None) == NRF_E_NULL


# host memory stands in for the device buffers: every case below has to return before any HIP call looks at a pointer
class _Args:
  def __init__(self, lib, n=8, c=2):
    self.lib, self.n, self.c = lib, n, c
    self.nbytes = _ws_bytes(lib, n, c)
    self.keep = {k: (C.c_char * (sz + 16))() for k, sz in (('cameras', c * 96), ('in', n * 12), ('g', n * 12), ('out', n * 12),
                                                           ('out2', n * 12), ('d_cameras', c * 96), ('ws', self.nbytes))}
    self.p = {k: (C.addressof(v) + 15) & ~15 for k, v in self.keep.items()}

  def call(self, name, **over):
    a = dict(self.p, n=self.n, c=self.c, nbytes=self.nbytes, index=None)
    a.update(over)
    f = getattr(self.lib, name)
    if name == 'nrf_camera_table_rays':
      return f(a['cameras'], a['c'], a['index'], a['in'], a['n'], a['out'], a['out2'], None)
    if name == 'nrf_camera_table_project':
      return f(a['cameras'], a['c'], a['index'], a['in'], a['n'], a['out'], None)
    if name == 'nrf_camera_table_rays_backward':
      return f(a['cameras'], a['c'], a['index'], a['in'], a['n'], a['g'], a['g'], a['d_cameras'], a['out'], a['ws'], a['nbytes'], None)
    return f(a['cameras'], a['c'], a['index'], a['in'], a['n'], a['g'], a['d_cameras'], a['out'], a['ws'], a['nbytes'], None)


CASES = [(name, over, code) for name in NEW[:4] for over, code in (
    (dict(cameras=None), NRF_E_NULL), (dict(**{'in': None}), NRF_E_NULL), (dict(n=-1), NRF_E_SHAPE), (dict(c=0), NRF_E_SHAPE),
    (dict(c=-3), NRF_E_SHAPE))]
CASES += [('nrf_camera_table_rays', dict(out2=None), NRF_E_NULL),              # directions
          ('nrf_camera_table_project', dict(out=None), NRF_E_NULL),            # pixels
          ('nrf_camera_table_project_backward', dict(g=None), NRF_E_NULL)]     # d_pixels
for _name in ('nrf_camera_table_rays_backward', 'nrf_camera_table_project_backward'):
  CASES += [(_name, dict(d_cameras=None), NRF_E_NULL), (_name, dict(ws=None), NRF_E_NULL), (_name, dict(nbytes=15), NRF_E_WORKSPACE),
            (_name, dict(nbytes=0), NRF_E_WORKSPACE)]


@pytest.mark.parametrize('name,over,code', CASES, ids=[f'{n[17:]}-{"-".join(f"{k}={v}" for k, v in o.items())}' for n, o, _ in CASES])
def test_bad_arguments_are_refused_on_the_host(lib, name, over, code):
  a = _Args(lib)
  if 'nbytes' in over and over['nbytes']:
    over = dict(over, nbytes=a.nbytes - 1)
  assert a.call(name, **over) == code
  msg = lib.nrf_last_error()
  assert msg and msg != b'ok'


def test_workspace_sized_for_fewer_rays_is_refused(lib):
  a = _Args(lib, n=8)
  small = _ws_bytes(lib, 8, 2)
  assert _ws_bytes(lib, 4096, 2) > small
  for name in ('nrf_camera_table_rays_backward', 'nrf_camera_table_project_backward'):
    assert a.call(name, n=4096, nbytes=small) == NRF_E_WORKSPACE and b'workspace' in lib.nrf_last_error()


def test_forward_with_no_rays_succeeds_without_a_device(lib):
  """n == 0: the forward calls launch nothing, so they succeed on a machine without a GPU.  (The reverse passes still launch the
  kernel that zeroes d_cameras: tests/test_gpu_camera_grads.py.)"""
  a = _Args(lib)
  assert a.call('nrf_camera_table_rays', n=0) == 0, lib.nrf_last_error()
  assert a.call('nrf_camera_table_project', n=0) == 0, lib.nrf_last_error()
  assert a.call('nrf_camera_table_rays', n=0, out=None) == 0      # origins are optional
  # an empty batch has no per-ray buffer to look at: NULL (what an empty torch tensor's data_ptr() is) passes
  assert a.call('nrf_camera_table_rays', n=0, out=None, out2=None, **{'in': None}) == 0, lib.nrf_last_error()
  assert a.call('nrf_camera_table_project', n=0, out=None, **{'in': None}) == 0, lib.nrf_last_error()
  assert a.call('nrf_camera_table_rays', n=0, cameras=None) == -1 and a.call('nrf_camera_table_rays', n=0, c=0) == -2


def _header_fields():
  src = open(HEADER).read()
  body = re.search(r'typedef struct nrf_camera \{(.*?)\} nrf_camera;', src, flags=re.S).group(1)
  body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
  return [(t, name, int(cnt or 1)) for t, name, cnt in re.findall(r'\b(int32_t|float)\s+([a-z_0-9]+)(?:\[(\d+)\])?;', body)]


def test_param_slices_follow_the_header():
  from nerfies_amd import lib as L
  from nerfies_amd.camera import CAMERA_PARAM_SLICES
  floats = [(name, cnt) for t, name, cnt in _header_fields() if t == 'float']
  assert [name for t, name, _ in _header_fields() if t != 'float'] == ['image_size']     # the one field a row does not hold
  assert list(CAMERA_PARAM_SLICES) == [name for name, _ in floats]
  at = 0
  for name, cnt in floats:
    sl = CAMERA_PARAM_SLICES[name]
    assert (sl.start, sl.stop, sl.step) == (at, at + cnt, None), name
    at += cnt
  assert at == L.NRF_CAMERA_NPARAMS == 22 and L.NRF_CAMERA_ROW == 24
  covered = sorted(i for sl in CAMERA_PARAM_SLICES.values() for i in range(sl.start, sl.stop))
  assert covered == list(range(22))
  # the ctypes mirror of nrf_camera has the same float fields at the same float offsets
  for name, _ in floats:
    assert getattr(L.CameraDesc, name).offset == 4 * CAMERA_PARAM_SLICES[name].start, name


def test_pack_unpack_round_trip():
  from nerfies_amd.camera import CAMERA_PARAM_SLICES, Camera, pack_cameras, unpack_camera
  rng = np.random.default_rng(0)
  cams = []
  for k in range(3):
    R, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    cams.append(Camera(orientation=R, position=rng.normal(size=3), focal_length=400.0 + k, principal_point=[160.2 + k, 119.7],
                       image_size=[320, 240 + k], skew=0.3 * k, pixel_aspect_ratio=1.0 + 0.01 * k,
                       radial_distortion=[0.05 * k, -0.02, 0.004], tangential_distortion=[0.001, -0.002 * k]))
  table = pack_cameras(cams, device='cpu')
  assert tuple(table.shape) == (3, 24) and table.dtype.is_floating_point and table.element_size() == 4
  assert not table[:, 22:].any()
  for k, cam in enumerate(cams):
    row = table[k].numpy()
    for name, sl in CAMERA_PARAM_SLICES.items():
      np.testing.assert_array_equal(row[sl], np.asarray(getattr(cam, name), np.float32).reshape(-1), err_msg=name)
    back = unpack_camera(table[k], cam.image_size)
    for name, value in cam.get_parameters().items():
      got = getattr(back, name)
      assert got.shape == value.shape and got.dtype == value.dtype, name
      np.testing.assert_array_equal(got, value, err_msg=name)
    np.testing.assert_array_equal(pack_cameras([back], device='cpu')[0].numpy(), row)
