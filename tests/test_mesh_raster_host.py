"""Mesh rasteriser on the host (no GPU): NRF_HAS_MESH_RASTER next to an unchanged NRF_VERSION, the exports, the status struct, every
refusal the entries decide before any HIP call (by entry and argument name in nrf_last_error; stand-in pointers, nothing is touched),
the workspace size, and the NumPy restatement of the definition (tests/mesh_raster_reference.py) against itself: on three inputs
every pixel of the union is owned exactly once and the covered set is what the polygon says, and the sphere of the GPU test has at
most 1 % tie pixels (the share the GPU test's permutation check may leave out)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import mesh_raster_reference as R
import mesh_reference as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'nerfies_amd.h')
NRF_E_NULL, NRF_E_SHAPE, NRF_E_WORKSPACE = -1, -2, -5   # include/nerfies_amd.h
ENTRIES = ('nrf_camera_table_project_depth', 'nrf_mesh_raster_workspace_bytes', 'nrf_mesh_raster_draw', 'nrf_mesh_raster_interpolate',
           'nrf_mesh_raster_visibility')
MAX_PIXELS = 1 << 26


@pytest.fixture(scope='module')
def lib():
  from nerfies_amd import build, lib as L
  build.build()
  return L.load_library()


def test_macro_status_and_exports(tmp_path, lib):
  from nerfies_amd import lib as L
  cc = shutil.which('gcc') or shutil.which('cc')
  assert cc is not None, 'no C compiler'
  lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', 'int main(void) {',
           '  printf("size %zu\\n", sizeof(nrf_mesh_raster_status));']
  for fname, _ in L.MeshRasterStatus._fields_:
    lines.append(f'  printf("{fname} %zu\\n", offsetof(nrf_mesh_raster_status, {fname}));')
  lines += ['  printf("NRF_HAS_MESH_RASTER %d\\n", NRF_HAS_MESH_RASTER);', '  printf("NRF_MESH_RASTER_MAX_PIXELS %d\\n", NRF_MESH_RASTER_MAX_PIXELS);',
            '  printf("NRF_VERSION %d\\n", NRF_VERSION);', '  return 0;', '}']
  src = tmp_path / 'abi.c'
  src.write_text('\n'.join(lines))
  exe = tmp_path / 'abi'
  subprocess.run([cc, '-std=c99', '-Wall', '-Werror', str(src), '-o', str(exe)], check=True)
  got = {}
  for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines():
    k, v = line.split()
    got[k] = int(v)
  assert got['NRF_HAS_MESH_RASTER'] == 1 == L.NRF_HAS_MESH_RASTER
  assert got['NRF_MESH_RASTER_MAX_PIXELS'] == MAX_PIXELS == L.NRF_MESH_RASTER_MAX_PIXELS
  assert got['NRF_VERSION'] == 660 == lib.nrf_version() == L.NRF_VERSION
  assert got['size'] == C.sizeof(L.MeshRasterStatus) == 16
  assert [f for f, _ in L.MeshRasterStatus._fields_] == ['drawn_triangles', 'large_triangles', 'covered_pixels', 'reserved']
  for fname, _ in L.MeshRasterStatus._fields_:
    assert got[fname] == getattr(L.MeshRasterStatus, fname).offset, fname
  for name in ENTRIES:
    assert name in L.EXPORTS and hasattr(lib, name), name


class _Call:
  """The entries with stand-in buffers: nothing is touched before a refusal."""

  def __init__(self, lib):
    self.lib = lib
    self.buf = (C.c_float * 64)()
    self.p = C.cast(self.buf, C.c_void_p)
    self.aligned = C.c_void_p((self.p.value + 15) // 16 * 16)

  def pick(self, v):
    return self.aligned if v == 'p' else (C.c_void_p(self.aligned.value + 4) if v == 'odd' else v)

  def size(self, F=9, W=32, H=24, out='n'):
    n = C.c_size_t(0)
    rc = self.lib.nrf_mesh_raster_workspace_bytes(F, W, H, C.byref(n) if out == 'n' else None)
    return rc, n.value

  def draw(self, screen='p', V=7, tris='p', F=9, W=32, H=24, near=0.0, face_id='p', depth='p', bary='p', ws='p', nbytes=1 << 40):
    return self.lib.nrf_mesh_raster_draw(self.pick(screen), V, self.pick(tris), F, W, H, near, self.pick(face_id), self.pick(depth),
                                         self.pick(bary), self.pick(ws), nbytes, None)

  def interpolate(self, face_id='p', bary='p', P=5, tris='p', F=9, attrs='p', V=7, A=3, bg='p', out='p'):
    return self.lib.nrf_mesh_raster_interpolate(self.pick(face_id), self.pick(bary), P, self.pick(tris), F, self.pick(attrs), V, A,
                                                self.pick(bg), self.pick(out), None)

  def visibility(self, face_id='p', P=5, tris='p', F=9, V=7, visible='p'):
    return self.lib.nrf_mesh_raster_visibility(self.pick(face_id), P, self.pick(tris), F, V, self.pick(visible), None)

  def project(self, cameras='p', C_=1, index=None, points='p', n=4, screen='p'):
    return self.lib.nrf_camera_table_project_depth(self.pick(cameras), C_, self.pick(index), self.pick(points), n, self.pick(screen), None)

  def err(self):
    return self.lib.nrf_last_error()


def test_null_arguments(lib):
  c = _Call(lib)
  assert c.size(out=None)[0] == NRF_E_NULL and b'nrf_mesh_raster_workspace_bytes: bytes' in c.err()
  for arg, name in (('screen', b'screen'), ('tris', b'triangles'), ('face_id', b'face_id'), ('depth', b'depth'), ('ws', b'workspace')):
    assert c.draw(**{arg: None}) == NRF_E_NULL and b'nrf_mesh_raster_draw: ' + name in c.err(), arg
  for arg, name in (('face_id', b'face_id'), ('bary', b'bary'), ('tris', b'triangles'), ('attrs', b'attributes'), ('out', b'out')):
    assert c.interpolate(**{arg: None}) == NRF_E_NULL and b'nrf_mesh_raster_interpolate: ' + name in c.err(), arg
  for arg, name in (('face_id', b'face_id'), ('tris', b'triangles'), ('visible', b'visible')):
    assert c.visibility(**{arg: None}) == NRF_E_NULL and b'nrf_mesh_raster_visibility: ' + name in c.err(), arg
  assert c.project(cameras=None) == NRF_E_NULL
  assert c.project(points=None) == NRF_E_NULL and c.project(screen=None) == NRF_E_NULL
  # a buffer whose count is 0 may be NULL: the workspace rule is the next one met; bary and the background are optional where stated
  assert c.draw(screen=None, V=0, tris=None, F=0, nbytes=0) == NRF_E_WORKSPACE
  assert c.draw(bary=None, nbytes=0) == NRF_E_WORKSPACE
  assert c.interpolate(face_id=None, bary=None, out=None, P=0) == 0
  assert c.visibility(face_id=None, P=0, tris=None, F=0, visible=None, V=0) == 0
  assert c.project(points=None, screen=None, n=0) == 0                    # n == 0: a successful no-op, as for the camera-table entries


def test_shape_refusals(lib):
  c = _Call(lib)
  name = b'nrf_mesh_raster_workspace_bytes:'
  assert c.size(F=-1)[0] == NRF_E_SHAPE and name in c.err() and b'num_triangles' in c.err()
  assert c.size(W=0)[0] == NRF_E_SHAPE and name in c.err() and b'width' in c.err()
  assert c.size(H=0)[0] == NRF_E_SHAPE and name in c.err() and b'height' in c.err()
  assert c.size(W=8193, H=8192)[0] == NRF_E_SHAPE and name in c.err() and b'NRF_MESH_RASTER_MAX_PIXELS' in c.err()
  assert c.size(W=8192, H=8192)[0] == 0 and c.size(W=MAX_PIXELS, H=1)[0] == 0
  name = b'nrf_mesh_raster_draw:'
  assert c.draw(V=-1) == NRF_E_SHAPE and name in c.err() and b'num_vertices' in c.err()
  assert c.draw(F=-1) == NRF_E_SHAPE and name in c.err() and b'num_triangles' in c.err()
  assert c.draw(W=0) == NRF_E_SHAPE and name in c.err() and b'width' in c.err()
  assert c.draw(H=-2) == NRF_E_SHAPE and name in c.err() and b'height' in c.err()
  assert c.draw(W=1 << 14, H=(1 << 12) + 1) == NRF_E_SHAPE and name in c.err() and b'NRF_MESH_RASTER_MAX_PIXELS' in c.err()
  for near in (-1e-6, float('nan'), float('inf'), -float('inf')):
    assert c.draw(near=near) == NRF_E_SHAPE and name in c.err() and b'near' in c.err(), near
  name = b'nrf_mesh_raster_interpolate:'
  for arg, word in (('P', b'num_pixels'), ('F', b'num_triangles'), ('V', b'num_vertices')):
    assert c.interpolate(**{arg: -1}) == NRF_E_SHAPE and name in c.err() and word in c.err(), arg
  for A in (0, -4):
    assert c.interpolate(A=A) == NRF_E_SHAPE and name in c.err() and b'width_a' in c.err()
  name = b'nrf_mesh_raster_visibility:'
  for arg, word in (('P', b'num_pixels'), ('F', b'num_triangles'), ('V', b'num_vertices')):
    assert c.visibility(**{arg: -1}) == NRF_E_SHAPE and name in c.err() and word in c.err(), arg
  assert c.project(C_=0) == NRF_E_SHAPE and c.project(n=-1) == NRF_E_SHAPE and c.project(cameras='odd') == NRF_E_SHAPE


def test_workspace_rules_and_sizes(lib):
  c = _Call(lib)
  rc, need = c.size()
  assert rc == 0 and need >= 16 + 8 * 32 * 24
  assert c.draw(nbytes=need - 1) == NRF_E_WORKSPACE and b'nrf_mesh_raster_draw:' in c.err() and b'nrf_mesh_raster_workspace_bytes' in c.err()
  assert c.draw(ws='odd') == NRF_E_WORKSPACE and b'nrf_mesh_raster_draw:' in c.err() and b'16-byte aligned' in c.err()
  assert c.size(F=0, W=1, H=1)[1] >= 16 + 8
  last = 0
  for F in (0, 1, 255, 256, 257, 1025, 10 ** 6, (1 << 31) - 1):       # grows with F ...
    rc, size = c.size(F=F)
    assert rc == 0 and size >= last, F
    last = size
  assert c.size(F=10 ** 6)[1] > c.size(F=1000)[1] > c.size(F=0)[1]
  last = 0
  for W, H in ((1, 1), (32, 24), (64, 48), (960, 540), (8192, 8192)):   # ... and with W H
    rc, size = c.size(F=1000, W=W, H=H)
    assert rc == 0 and size > last and size >= 8 * W * H, (W, H)
    last = size
  # 8 bytes per pixel, about 4 per triangle
  F, W, H = 2_000_000, 960, 540
  assert 8 * W * H + 4 * F <= c.size(F=F, W=W, H=H)[1] <= 8 * W * H + 4.1 * F + 4096


@pytest.mark.parametrize('name', sorted(R.exactly_once_cases()))
def test_reference_owns_every_pixel_of_the_union_exactly_once(name):
  screen, faces, W, H, polygon = R.exactly_once_cases()[name]
  count = R.coverage_count(screen, faces, W, H)
  inside, boundary = R.polygon_sides(polygon, W, H)
  assert count.max() == 1                                              # no pixel twice, on a shared edge or at the shared vertex
  assert (count[inside] == 1).all() and (count[~inside & ~boundary] == 0).all()
  face_id, depth, bary, status = R.draw(screen, faces, W, H)
  assert np.array_equal(face_id >= 0, count == 1) and status[0] == len(faces) and status[2] == int(count.sum())
  # what the polygon's area says: Pick's theorem on the lattice of pixel centres, I = A - B / 2 + 1
  P = np.asarray(polygon, np.int64)
  nxt = np.roll(P, -1, 0)
  area = abs(int((P[:, 0] * nxt[:, 1] - nxt[:, 0] * P[:, 1]).sum())) / 2 / 256 ** 2
  if name.startswith('quad_split'):                                    # corners on pixel corners: no centre on the boundary
    assert not boundary.any() and count.sum() == area == W * H
  else:                                                                # corners on pixel centres
    B = sum(int(np.gcd(abs(d[0]) // 256, abs(d[1]) // 256)) for d in nxt - P)
    assert boundary.sum() == B and inside.sum() == area - B / 2 + 1
    owned = count[boundary].sum()
    assert 0 < owned < B                                               # top and left borders in, bottom and right ones out
  if name == 'centre_quad':
    want = np.zeros((H, W), bool)
    want[2:7, 2:9] = True                                              # rows 2..6, columns 2..8: 35 = the area
    assert np.array_equal(count == 1, want) and area == 35
  # barycentrics sum to one within rounding and the depth lies between the corners' z
  cov = face_id >= 0
  assert np.abs(bary[cov].sum(-1) - 1).max() < 1e-6
  assert (depth[cov] >= screen[:, 2].min() * (1 - 1e-6)).all() and (depth[cov] <= screen[:, 2].max() * (1 + 1e-6)).all()
  assert (depth[~cov] == 0).all() and (bary[~cov] == 0).all()


def sphere_screen_oracle():
  """The sphere case's screen array from the float64 camera oracle, rounded to float32, and its faces."""
  from oracle import camera_oracle as CO
  vertices, _, faces = M.surface_nets(R.sphere_sigma(), R.SPHERE_ORIGIN, R.SPHERE_STEP, 0.0)
  cam = CO.make_camera(**R.sphere_camera())
  px = CO.project(cam, vertices.astype(np.float64)).reshape(-1, 2)
  z = (vertices.astype(np.float64) - cam['position']) @ cam['orientation'][2]
  return np.concatenate([px, z[:, None]], 1).astype(np.float32), faces, vertices


def test_sphere_case_has_at_most_one_percent_tie_pixels():
  screen, faces, vertices = sphere_screen_oracle()
  W, H = R.SPHERE_IMAGE
  assert len(faces) > 300 and M.edge_report(faces)[0]                  # a closed surface
  face_id, depth, bary, status = R.draw(screen, faces, W, H)
  covered = face_id >= 0
  assert 0.25 * W * H < covered.sum() < 0.9 * W * H                    # the sphere fills the image without leaving it
  assert not covered[0].any() and not covered[-1].any() and not covered[:, 0].any() and not covered[:, -1].any()
  ties = R.tie_pixels(screen, faces, W, H)
  assert ties.sum() <= 0.01 * W * H, int(ties.sum())
  # the front half owns the image: every owner faces the camera's side
  assert status[0] <= len(faces) and status[1] == 0
  count = R.coverage_count(screen, faces, W, H)
  assert (count[covered] >= 2).mean() > 0.8                            # front and back: the depth test decides almost everywhere


def test_reference_by_hand():
  """A right triangle over pixel centres with z = 1, 2, 4: depth is the harmonic interpolation, the first vertex's pixel is its own."""
  screen = np.array([[0.5, 0.5, 1.0], [4.5, 0.5, 2.0], [0.5, 4.5, 4.0]], np.float32)
  faces = np.array([[0, 1, 2]], np.int32)
  face_id, depth, bary, status = R.draw(screen, faces, 6, 6)
  assert face_id[0, 0] == 0 and depth[0, 0] == 1.0 and bary[0, 0].tolist() == [1.0, 0.0, 0.0]
  assert face_id[0, 4] == -1 and face_id[4, 0] == -1                   # the hypotenuse's ends lie on a bottom-right edge
  assert face_id[0, 2] == 0 and np.isclose(depth[0, 2], 1 / (0.5 / 1 + 0.5 / 2))
  assert np.allclose(bary[0, 2], [(0.5 / 1) / 0.75, (0.5 / 2) / 0.75, 0.0])
  assert status == [1, 0, int((face_id >= 0).sum()), 0]
  flipped = R.draw(screen, faces[:, ::-1].copy(), 6, 6)
  assert np.array_equal(flipped[0], face_id)                           # no culling; w is summed in the other order: not bits
  assert np.allclose(flipped[1], depth, rtol=1e-6, atol=0) and np.allclose(flipped[2][..., ::-1], bary, rtol=1e-6, atol=1e-7)
  out = R.interpolate(face_id, bary, faces, np.array([[1.0], [3.0], [5.0]], np.float32), [9.0])
  assert out[0, 0] == 1.0 and out[5 * 6 + 5, 0] == 9.0
  assert R.visibility(face_id, faces, 4).tolist() == [1, 1, 1, 0]
