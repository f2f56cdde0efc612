"""Mesh rasteriser on the GPU (nrf_camera_table_project_depth, nrf_mesh_raster_draw / _interpolate / _visibility,
evaluation.rasterize_mesh / mesh_visibility, export_density --render_mesh).

Draw, interpolate and visibility are held against tests/mesh_raster_reference.py (the header's definition restated in NumPy) bit
for bit: face ids and status counts as integers, depth, barycentrics and interpolated rows as bits.  The only tolerances are the
projection's z against the float64 oracle and the sphere's geometric bounds, each derived where it is used."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

import helpers as H
import mesh_raster_reference as R
from oracle import camera_oracle as CO

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAD = 64
CANARY_I, CANARY_F = -77777, -12345.5


def _dev(a):
  return torch.from_numpy(np.ascontiguousarray(a)).to(H.DEV)


def _bits(a):
  return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


class _Raw:
  """The entries themselves on device tensors, with PAD canary elements behind every output."""

  def __init__(self):
    from nerfies_amd import lib as L
    self.L, self.lib = L, L.load_library()
    self.stream = torch.cuda.current_stream(torch.device(H.DEV)).cuda_stream

  def draw(self, screen, faces, W, H_, near=0.0, with_bary=True):
    screen, faces = np.asarray(screen, np.float32).reshape(-1, 3), np.asarray(faces, np.int32).reshape(-1, 3)
    V, F, P = len(screen), len(faces), W * H_
    ds, df = _dev(screen), _dev(faces)
    n = C.c_size_t(0)
    self.L.check(self.lib.nrf_mesh_raster_workspace_bytes(F, W, H_, C.byref(n)), self.lib)
    ws = torch.full(((n.value + 3) // 4 + PAD,), CANARY_I, dtype=torch.int32, device=H.DEV)
    face_id = torch.full((P + PAD,), CANARY_I, dtype=torch.int32, device=H.DEV)
    depth = torch.full((P + PAD,), CANARY_F, dtype=torch.float32, device=H.DEV)
    bary = torch.full((3 * P + PAD,), CANARY_F, dtype=torch.float32, device=H.DEV)
    ptr = lambda t: t.data_ptr() if t.numel() else None
    self.L.check(self.lib.nrf_mesh_raster_draw(ptr(ds), V, ptr(df), F, W, H_, near, face_id.data_ptr(), depth.data_ptr(),
                                               bary.data_ptr() if with_bary else None, ws.data_ptr(), n.value, self.stream), self.lib)
    assert bool((face_id[P:] == CANARY_I).all()) and bool((depth[P:] == CANARY_F).all())
    assert bool((bary[3 * P if with_bary else 0:] == CANARY_F).all()) and bool((ws[(n.value + 3) // 4:] == CANARY_I).all())
    return (face_id[:P].reshape(H_, W).cpu().numpy(), depth[:P].reshape(H_, W).cpu().numpy(),
            bary[:3 * P].reshape(H_, W, 3).cpu().numpy(), ws[:4].tolist())

  def interpolate(self, face_id, bary, faces, attributes, background):
    fid, b, f, a = _dev(np.asarray(face_id, np.int32).reshape(-1)), _dev(_f32(bary).reshape(-1, 3)), _dev(faces), _dev(_f32(attributes))
    P, A = fid.numel(), a.shape[1]
    bg = _dev(_f32(background)) if background is not None else None
    out = torch.full((P * A + PAD,), CANARY_F, dtype=torch.float32, device=H.DEV)
    self.L.check(self.lib.nrf_mesh_raster_interpolate(fid.data_ptr(), b.data_ptr(), P, f.data_ptr() if f.numel() else None, f.shape[0], a.data_ptr(),
                                                      a.shape[0], A, bg.data_ptr() if bg is not None else None, out.data_ptr(), self.stream),
                 self.lib)
    assert bool((out[P * A:] == CANARY_F).all())
    return out[:P * A].reshape(P, A).cpu().numpy()

  def visibility(self, face_id, faces, V):
    fid, f = _dev(np.asarray(face_id, np.int32).reshape(-1)), _dev(faces)
    vis = torch.full((V + PAD,), 77, dtype=torch.uint8, device=H.DEV)
    self.L.check(self.lib.nrf_mesh_raster_visibility(fid.data_ptr(), fid.numel(), f.data_ptr() if f.numel() else None, f.shape[0], V,
                                                     vis.data_ptr(), self.stream), self.lib)
    assert bool((vis[V:] == 77).all())
    return vis[:V].cpu().numpy()


def _f32(a):
  return np.ascontiguousarray(a, dtype=np.float32)


def _tri(*rows):
  return np.array(rows, np.float32)


def _whole_image_with_small():
  """One triangle over the whole 64 x 48 image at z = 2 (the workgroup path) and small ones in front of it and behind it (the
  thread path): both paths meet in one key buffer."""
  rs = np.random.RandomState(5)
  screen, faces = [[-10.0, -10.0, 2.0], [200.0, -10.0, 2.0], [-10.0, 150.0, 2.0]], [[0, 1, 2]]
  for k in range(24):
    c = rs.uniform([2, 2], [60, 44])
    z = 1.0 + 0.01 * k if k % 2 == 0 else 3.0 + 0.01 * k
    base = len(screen)
    for d in rs.uniform(-4, 4, (3, 2)):
      screen.append([c[0] + d[0], c[1] + d[1], z])
    faces.append([base, base + 1, base + 2])
  order = rs.permutation(len(faces))                                   # the large one is not the first
  return np.array(screen, np.float32), np.array(faces, np.int32)[order], 64, 48, 0.0


LARGE_AT = (0, 1, 63, 64, 65, 255, 256, 300, 599)   # first lanes, the sides of a wave and of a workgroup, a third workgroup's last lane


def _many_large():
  """600 triangles (three workgroups of the faces kernel) on 64 x 48: those at LARGE_AT have pixel boxes of more than 256 pixels, the
  others of at most 16; every triangle has its own constant depth, so no pixel is a tie and the picture has one owner per pixel
  whatever the order."""
  rs = np.random.RandomState(12)
  screen, faces = [], []
  for t in range(600):
    if t in LARGE_AT:
      a = rs.uniform([1, 1], [20, 15])
      corners = [a, a + [rs.uniform(30, 40), rs.uniform(0, 5)], a + [rs.uniform(0, 5), rs.uniform(25, 30)]]
      z = 2.0 + 0.05 * LARGE_AT.index(t)
    else:
      c = rs.uniform([3, 3], [61, 45])
      corners = [c + d for d in rs.uniform(-1.5, 1.5, (3, 2))]
      z = (1.0 if t % 2 == 0 else 3.0) + 0.001 * t                     # in front of the large ones, and behind them
    if rs.rand() < 0.5:
      corners = corners[::-1]                                          # either orientation
    faces.append([len(screen), len(screen) + 1, len(screen) + 2])
    screen += [[p[0], p[1], z] for p in corners]
  return np.array(screen, np.float32), np.array(faces, np.int32), 64, 48, 0.0


def _cases():
  nan, inf = np.nan, np.inf
  front = _tri([4.2, 3.1, 1.0], [25.7, 5.3, 1.5], [9.4, 20.8, 2.0])
  cases = {name: (s, f, W, H_, 0.0) for name, (s, f, W, H_, _) in R.exactly_once_cases().items()}
  cases.update({
      'overlap_depths': (np.concatenate([front, front + np.float32([3.0, 2.0, 0.25])]), [[0, 1, 2], [5, 4, 3]], 32, 24, 0.0),
      # the same triangle three times, under two sets of vertex indices with the same coordinates: equal depth bits
      'overlap_equal_bits': (np.concatenate([front, front]), [[3, 4, 5], [0, 1, 2], [0, 1, 2]], 32, 24, 0.0),
      'behind_near': (np.concatenate([front, _tri([2, 2, 0.5], [20, 3, 1.0], [5, 18, 1.0]), _tri([3, 3, 0.25], [28, 8, 0.7], [8, 21, 0.7])]),
                      [[0, 1, 2], [3, 4, 5], [6, 7, 8]], 32, 24, 0.5),
      'nonfinite': (np.concatenate([front, _tri([nan, 2, 1], [inf, 3, 1], [4, -inf, 1], [5, 5, nan], [1048576.125, 2, 1], [-1048576.0, 30, 0.5],
                                                [6, -1048577.0, 1], [7, 7, inf])]),
                    [[0, 1, 3], [0, 4, 2], [5, 1, 2], [0, 1, 6], [0, 7, 2], [8, 1, 2], [0, 9, 2], [0, 1, 10], [0, 1, 2]], 32, 24, 0.0),
      'bad_index': (front, [[0, 1, 3], [-1, 1, 2], [0, 2 ** 31 - 1, 2], [-2 ** 31, 0, 1], [2, 1, 0]], 32, 24, 0.0),
      'zero_area': (np.concatenate([front, _tri([2.0, 2.0, 1.0], [6.0, 4.0, 1.0], [10.0, 6.0, 1.0])]),
                    [[3, 4, 5], [0, 0, 1], [1, 1, 1], [0, 1, 2]], 32, 24, 0.0),
      'sliver': (_tri([2.25, 2.0, 1.0], [10.25, 10.0, 1.0], [10.25, 10.03, 1.0], [3.1, 3.1, 1.0], [12.4, 3.3, 1.0], [3.1, 3.2, 1.0]),
                 [[0, 1, 2], [3, 4, 5]], 32, 24, 0.0),
      'partly_off': (_tri([-9.3, -4.2, 1.0], [40.6, 8.1, 2.0], [11.2, 31.7, 1.5]), [[0, 1, 2]], 32, 24, 0.0),
      'wholly_off': (_tri([-20.0, 3.0, 1.0], [-2.0, 5.0, 1.0], [-9.0, 20.0, 1.0], [33.0, 2.0, 1.0], [60.0, 4.0, 1.0], [40.0, 30.0, 1.0],
                          [3.0, 24.6, 1.0], [20.0, 25.0, 1.0], [9.0, 90.0, 1.0]), [[0, 1, 2], [3, 4, 5], [6, 7, 8]], 32, 24, 0.0),
      # clamped pixel boxes of 16 x 16 = 256 (columns 0..15, rows 2..17) and 17 x 16 = 272 pixels: the two sides of the split
      'split_256': (_tri([-5.5, 2.5, 1.0], [15.5, 2.5, 1.0], [-5.5, 17.5, 1.0], [-5.5, 2.5, 2.0], [16.5, 2.5, 2.0], [-5.5, 17.5, 2.0]),
                    [[0, 1, 2], [3, 4, 5]], 32, 24, 0.0),
      'whole_image_with_small': _whole_image_with_small(),
      'many_large': _many_large(),
      'no_faces': (front, np.zeros((0, 3), np.int32), 32, 24, 0.0),
      'no_vertices': (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), 32, 24, 0.0),
  })
  return cases


CASES = _cases()
_REF = {}


def reference(name):
  """The reference's (face_id, depth, bary, status) of a case: CPU only, computed once, never changed."""
  if name not in _REF:
    s, f, W, H_, near = CASES[name]
    _REF[name] = R.draw(s, f, W, H_, near)
  return _REF[name]


@pytest.mark.parametrize('name', sorted(CASES))
def test_draw_is_the_reference_bit_for_bit(name):
  s, f, W, H_, near = CASES[name]
  want_id, want_depth, want_bary, want_status = reference(name)
  face_id, depth, bary, status = _Raw().draw(s, f, W, H_, near)
  assert status == want_status, (status, want_status)
  assert np.array_equal(face_id, want_id)
  assert np.array_equal(_bits(depth), _bits(want_depth)) and np.array_equal(_bits(bary), _bits(want_bary))
  print(f'[raster {name}] F {len(f)}: drawn {status[0]}, large {status[1]}, covered {status[2]} of {W * H_}')
  # what each case is there for
  covered = want_id >= 0
  if name in R.exactly_once_cases():
    assert status[0] == len(f) and status[2] == int(R.coverage_count(s, f, W, H_).sum())
  elif name == 'overlap_depths':
    assert set(np.unique(want_id)) == {-1, 0, 1} and status[0] == 2
  elif name == 'overlap_equal_bits':
    assert status[0] == 3 and set(np.unique(want_id)) == {-1, 0}         # three candidates with the same bits: the lowest index wins
    assert R.tie_pixels(s, f, W, H_)[covered].all()
  elif name == 'behind_near':
    assert status[0] == 1 and set(np.unique(want_id)) == {-1, 0}         # z == near and z < near both drop the whole triangle
  elif name == 'nonfinite':
    assert status[0] == 3 and {-1, 5} <= set(np.unique(want_id)) <= {-1, 5, 7, 8}   # |px| == 2^20, z == inf: usable; the rest is not
  elif name == 'bad_index':
    assert status[0] == 1 and set(np.unique(want_id)) == {-1, 4}
  elif name == 'zero_area':
    assert status[0] == 1 and set(np.unique(want_id)) == {-1, 3}
  elif name == 'sliver':
    assert status == [1, 0, 0, 0]                                        # one has an empty pixel box, the other covers no centre
  elif name == 'partly_off':
    assert status[0] == 1 and covered[0].any() and covered[:, -1].any() and not covered.all()
  elif name in ('wholly_off', 'no_faces', 'no_vertices'):
    assert status == [0, 0, 0, 0] and not covered.any() and not depth.any() and not bary.any()
  elif name == 'split_256':
    assert status[:2] == [2, 1] and set(np.unique(want_id)) == {-1, 0, 1}
  elif name == 'whole_image_with_small':
    assert status[0] >= 20 and status[1] == 1 and covered.all() and len(np.unique(want_id)) > 10
    large = int(np.nonzero((np.asarray(f) == 0).any(1))[0][0])
    assert (want_id == large).sum() > 0.5 * W * H_ and (want_id != large).sum() > 20
  elif name == 'many_large':
    assert _large_faces(s, f, W, H_) == list(LARGE_AT) and status[1] == 9 == want_status[1] and status[0] > 500
    assert not R.tie_pixels(s, f, W, H_).any()
    assert set(LARGE_AT) <= set(np.unique(want_id)) and len(np.unique(want_id)) > 100   # every large one and many small ones own pixels


def _large_faces(s, f, W, H_):
  """The faces the reference counts as large, from its own pixel boxes."""
  return [t for t, _, _, _, _, _, i0, i1, j0, j1 in R.triangles(s, f, W, H_) if (i1 - i0 + 1) * (j1 - j0 + 1) > R.SMALL_BOX]


def test_many_large_triangles_in_another_order():
  """The large triangles land on other lanes, waves and workgroups of the faces kernel; the picture is the reference's for that order,
  and the same picture as before under the permutation (no pixel of this case is a tie)."""
  s, f, W, H_, near = CASES['many_large']
  perm = np.random.RandomState(13).permutation(len(f))
  want_id, want_depth, want_bary, want_status = R.draw(s, f[perm], W, H_, near)
  assert want_status[1] == 9 and sorted(perm[_large_faces(s, f[perm], W, H_)]) == list(LARGE_AT)
  face_id, depth, bary, status = _Raw().draw(s, f[perm], W, H_, near)
  assert status == want_status and status[1] == 9
  assert np.array_equal(face_id, want_id)
  assert np.array_equal(_bits(depth), _bits(want_depth)) and np.array_equal(_bits(bary), _bits(want_bary))
  first_id, first_depth = reference('many_large')[:2]
  assert np.array_equal(np.where(face_id >= 0, perm[np.maximum(face_id, 0)], -1), first_id)
  assert np.array_equal(_bits(depth), _bits(first_depth))


def test_draw_without_barycentrics_and_with_any_workspace_contents():
  s, f, W, H_, near = CASES['whole_image_with_small']
  want_id, want_depth, _, want_status = reference('whole_image_with_small')
  raw = _Raw()
  for _ in range(2):                                                     # the workspace comes filled with canaries: draw clears it
    face_id, depth, _, status = raw.draw(s, f, W, H_, near, with_bary=False)
    assert status == want_status and np.array_equal(face_id, want_id) and np.array_equal(_bits(depth), _bits(want_depth))


# ---- projection ----

def _cameras():
  """(table rows as float32, the float64 oracle cameras built from the ROUNDED rows): one distorted, one pinhole."""
  from nerfies_amd import camera as camera_lib
  rs = np.random.RandomState(2)
  cams = []
  for distorted in (True, False):
    q, _ = np.linalg.qr(rs.randn(3, 3))
    q *= np.sign(np.linalg.det(q))
    cams.append(camera_lib.Camera(orientation=q, position=rs.uniform(-0.2, 0.2, 3), focal_length=180.0 + 20 * distorted, principal_point=(31.0, 23.5),
                                  image_size=(64, 48), skew=0.1 * distorted, pixel_aspect_ratio=1.0 + 0.03 * distorted,
                                  radial_distortion=(0.05, -0.02, 0.004) if distorted else (0.0, 0.0, 0.0),
                                  tangential_distortion=(0.002, -0.001) if distorted else (0.0, 0.0)))
  table = camera_lib.pack_cameras(cams, H.DEV)
  rows = table.cpu().numpy().astype(np.float64)
  oracle = [CO.make_camera(orientation=r[0:9], position=r[9:12], focal_length=r[12], principal_point=r[13:15], image_size=(64, 48), skew=r[15],
                           pixel_aspect_ratio=r[16], radial_distortion=r[17:20], tangential_distortion=r[20:22]) for r in rows]
  return table, oracle


def test_project_depth_pixels_are_project_s_bits_and_z_is_the_oracle_s():
  from nerfies_amd import camera as camera_lib
  table, oracle = _cameras()
  rs = np.random.RandomState(4)
  for row, cam in enumerate(oracle):
    local = np.stack([rs.uniform(-0.3, 0.3, 64), rs.uniform(-0.3, 0.3, 64), rs.uniform(0.8, 2.5, 64)], 1)   # in front of the camera
    points = (local @ cam['orientation'] + cam['position']).astype(np.float32)
    index = torch.full((64,), row, dtype=torch.int32, device=H.DEV)
    screen = camera_lib.project_depth_from_table(table, _dev(points), index)
    pixels = camera_lib.project_from_table(table, _dev(points), index)
    assert screen.shape == (64, 3) and not screen.requires_grad
    assert torch.equal(screen[:, :2].contiguous().view(torch.int32), pixels.contiguous().view(torch.int32))
    t = points.astype(np.float64) - cam['position']
    want = t @ cam['orientation'][2]
    # at most four float32 roundings per term (the subtraction, the product, two sums), and a factor of two of margin
    bound = 8 * 2.0 ** -24 * (np.abs(t) @ np.abs(cam['orientation'][2]))
    err = np.abs(screen[:, 2].cpu().numpy().astype(np.float64) - want)
    print(f'[project_depth row {row}] max |z - oracle| / bound = {(err / bound).max():.3f}')
    assert (err <= bound).all() and (want > 0.5).all()
    if row == 0:                                                         # camera_index None = row 0 for every point
      again = camera_lib.project_depth_from_table(table, _dev(points))
      assert torch.equal(again.view(torch.int32), screen.view(torch.int32))


def test_project_depth_camera_index_rule_and_empty_batch():
  from nerfies_amd import camera as camera_lib
  table, oracle = _cameras()
  rs = np.random.RandomState(6)
  points = _dev((rs.uniform(-0.2, 0.2, (300, 3)) + 1.5 * oracle[0]['orientation'][2]).astype(np.float32))   # more than one workgroup
  index_np = rs.randint(-2, 4, 300).astype(np.int32)                     # -2, -1, 2, 3 lie outside the table
  index_np[:4] = [0, 1, -1, 2]
  screen = camera_lib.project_depth_from_table(table, points, _dev(index_np))
  outside = (index_np < 0) | (index_np >= 2)
  assert outside.any() and (~outside).any()
  assert bool((screen[_dev(outside)] == 0).all())
  for row in (0, 1):
    sel = _dev(index_np == row)
    alone = camera_lib.project_depth_from_table(table, points[sel], torch.full((int(sel.sum()),), row, dtype=torch.int32, device=H.DEV))
    assert torch.equal(screen[sel].contiguous().view(torch.int32), alone.view(torch.int32))
    assert bool((alone[:, 2] != 0).all())
  empty = camera_lib.project_depth_from_table(table, torch.zeros(0, 3, device=H.DEV))
  assert empty.shape == (0, 3)


# ---- the sphere through a camera ----

_SPHERE = {}


def sphere():
  """The sphere case, computed once: the device mesh, the table, rasterize_mesh's outputs, the reference on the GPU's own screen."""
  if not _SPHERE:
    from nerfies_amd import camera as camera_lib, evaluation
    mesh = evaluation.extract_mesh_from_grid(_dev(R.sphere_sigma()), R.SPHERE_ORIGIN, R.SPHERE_STEP, 0.0)
    spec = R.sphere_camera()
    cam = camera_lib.Camera(**{k: (np.asarray(v) if not np.isscalar(v) else v) for k, v in spec.items()})
    table = camera_lib.pack_cameras([cam, cam], H.DEV)
    table[0, :] = 0                                                      # row 1 is the camera: camera_row is honoured
    V = mesh['vertices'].shape[0]
    rs = np.random.RandomState(8)
    attrs = {'points': mesh['vertices'], 'one': _dev(rs.randn(V, 1).astype(np.float32)), 'five': _dev(rs.randn(V, 5).astype(np.float32))}
    bg = {'points': 0.0, 'one': 7.5, 'five': [1.0, -2.0, 3.0, -4.0, 5.0]}
    W, H_ = R.SPHERE_IMAGE
    run = lambda faces: evaluation.rasterize_mesh(mesh['vertices'], faces, table, (W, H_), camera_row=1, attributes=attrs, background=bg)
    out = run(mesh['faces'])
    screen, faces = out['screen'].cpu().numpy(), mesh['faces'].cpu().numpy()
    _SPHERE.update(mesh=mesh, table=table, attrs=attrs, bg=bg, run=run, out=out, screen=screen, faces=faces, ref=R.draw(screen, faces, W, H_),
                   ties=R.tie_pixels(screen, faces, W, H_))
  return _SPHERE


def test_sphere_is_the_reference_on_the_gpu_s_own_screen():
  S = sphere()
  out, (want_id, want_depth, want_bary, want_status) = S['out'], S['ref']
  W, H_ = R.SPHERE_IMAGE
  assert len(S['faces']) > 300 and out['face_id'].shape == (H_, W) and out['bary'].shape == (H_, W, 3)
  assert out['status'].tolist() == want_status and want_status[2] > 0.25 * W * H_
  assert np.array_equal(out['face_id'].cpu().numpy(), want_id)
  assert np.array_equal(_bits(out['depth'].cpu().numpy()), _bits(want_depth))
  assert np.array_equal(_bits(out['bary'].cpu().numpy()), _bits(want_bary))
  assert np.array_equal(out['mask'].cpu().numpy(), want_id >= 0) and out['mask'].dtype == torch.bool
  for name, rows in S['attrs'].items():
    want = R.interpolate(want_id, want_bary, S['faces'], rows.cpu().numpy(), np.broadcast_to(np.float32(S['bg'][name]), rows.shape[1:]))
    got = out[name].cpu().numpy()
    assert got.shape == (H_, W, rows.shape[1]) and np.array_equal(_bits(got).reshape(want.shape), _bits(want)), name
  # the screen the GPU made is the oracle's within float32: the host test's tie cap speaks of the same picture
  from test_mesh_raster_host import sphere_screen_oracle
  oracle_screen = sphere_screen_oracle()[0]
  assert np.abs(S['screen'] - oracle_screen).max() < 1e-3


def test_sphere_twice_and_permuted():
  S = sphere()
  W, H_ = R.SPHERE_IMAGE
  out = S['out']
  again = S['run'](S['mesh']['faces'])
  for key in ('face_id', 'depth', 'bary', 'points', 'one', 'five', 'status'):
    assert torch.equal(again[key].view(torch.int32), out[key].view(torch.int32)), key
  perm = np.random.RandomState(9).permutation(len(S['faces']))
  permuted = S['run'](S['mesh']['faces'][_dev(perm)])
  assert torch.equal(permuted['depth'].view(torch.int32), out['depth'].view(torch.int32))   # the depth bits do not depend on the order
  got = permuted['face_id'].cpu().numpy()
  back = np.where(got >= 0, perm[np.maximum(got, 0)], -1)               # a permuted index names the original face perm[index]
  want = out['face_id'].cpu().numpy()
  ties = S['ties']
  assert ties.sum() <= 0.01 * W * H_                                      # the cap the host test holds the oracle's picture to
  assert np.array_equal(back[~ties], want[~ties])
  assert np.array_equal(back >= 0, want >= 0)
  print(f'[sphere permuted] {int(ties.sum())} tie pixels of {W * H_}, {int((back != want).sum())} of them changed owner')


def test_sphere_interpolated_points_lie_in_the_shell():
  S = sphere()
  mask = S['out']['mask'].cpu().numpy()
  p = np.linalg.norm(S['out']['points'].cpu().numpy().astype(np.float64), axis=-1)[mask]
  h, r0 = R.SPHERE_STEP[0], R.SPHERE_R0
  rho = r0 - np.sqrt(3) * h
  lower, upper = np.sqrt(rho ** 2 - 4 * h ** 2), r0 + np.sqrt(3) * h
  # a vertex lies in a cell the sphere crosses (upper), three such vertices are pairwise at most 2 sqrt(3) h apart (lower).  Slack: the
  # interpolation is five float32 operations on barycentrics that sum to one within three roundings: 8 ulp of the upper bound
  slack = 8 * 2.0 ** -23 * upper
  print(f'[sphere shell] |p| in [{p.min():.6f}, {p.max():.6f}], bounds [{lower:.6f}, {upper:.6f}]')
  assert mask.sum() > 500 and p.min() >= lower - slack and p.max() <= upper + slack


# ---- interpolate and visibility ----

@pytest.mark.parametrize('A', [1, 3, 5])
def test_interpolate_is_the_reference_bit_for_bit(A):
  s, f, W, H_, near = CASES['whole_image_with_small']
  face_id, _, bary, _ = reference('whole_image_with_small')
  s2, f2, W2, H2, _ = CASES['overlap_depths']                            # with uncovered pixels: the background row
  face_id2, _, bary2, _ = reference('overlap_depths')
  rs = np.random.RandomState(A)
  raw = _Raw()
  for fid, b, faces, V in ((face_id, bary, f, len(s)), (face_id2, bary2, f2, len(s2))):
    attrs, bg = rs.randn(V, A).astype(np.float32), (rs.randn(A) + 3).astype(np.float32)
    got = raw.interpolate(fid, b, np.asarray(faces, np.int32), attrs, bg)
    assert np.array_equal(_bits(got), _bits(R.interpolate(fid, b, faces, attrs, bg)))
    zeros = raw.interpolate(fid, b, np.asarray(faces, np.int32), attrs, None)   # background NULL = zeros
    assert np.array_equal(_bits(zeros), _bits(R.interpolate(fid, b, faces, attrs, None)))
  assert (face_id2 < 0).any() and np.array_equal(got[(face_id2 < 0).reshape(-1)], np.broadcast_to(bg, (int((face_id2 < 0).sum()), A)))
  # a face id or a corner outside the mesh reads nothing: the background row
  odd = np.array([0, 1, 7, -1, -5, 2 ** 31 - 1], np.int32)
  faces = np.array([[0, 1, 2], [0, 1, 9]], np.int32)
  b = rs.rand(6, 3).astype(np.float32)
  attrs = rs.randn(3, A).astype(np.float32)
  got = raw.interpolate(odd, b, faces, attrs, bg)
  assert np.array_equal(_bits(got), _bits(R.interpolate(odd, b, faces, attrs, bg))) and np.array_equal(got[1:], np.broadcast_to(bg, (5, A)))


def test_visibility_is_the_reference_s_set():
  raw = _Raw()
  for name in ('whole_image_with_small', 'overlap_depths', 'fan', 'no_faces', 'bad_index'):
    s, f, W, H_, near = CASES[name]
    face_id = reference(name)[0]
    V = len(s) + 3                                                       # vertices no face names stay invisible
    got = raw.visibility(face_id, np.asarray(f, np.int32).reshape(-1, 3), V)
    assert np.array_equal(got, R.visibility(face_id, f, V)), name
  assert raw.visibility(np.array([5, -1, 2 ** 31 - 1], np.int32), np.array([[0, 1, 2]], np.int32), 4).tolist() == [0, 0, 0, 0]


def test_the_far_side_of_a_closed_mesh_is_invisible():
  from nerfies_amd import evaluation
  S = sphere()
  V = S['mesh']['vertices'].shape[0]
  visible = evaluation.mesh_visibility(S['out'], S['mesh']['faces'], V)
  assert visible.dtype == torch.bool and visible.shape == (V,)
  assert np.array_equal(visible.cpu().numpy(), R.visibility(S['ref'][0], S['faces'], V).astype(bool))
  position = np.asarray(R.sphere_camera()['position'])
  vertices = S['mesh']['vertices'].cpu().numpy().astype(np.float64)
  facing = -(vertices @ position) / (np.linalg.norm(vertices, axis=1) * np.linalg.norm(position))   # cosine between -x and the view
  vis = visible.cpu().numpy()
  assert 0.2 * V < vis.sum() < 0.8 * V
  assert not vis[facing > 0.5].any()                                     # the far side: hidden behind the near side
  assert vis[facing < -0.6].all()                                        # well inside the near side: every vertex owns a pixel's face


def test_export_density_renders_the_mesh_end_to_end(tmp_path, capsys):
  sys.path.insert(0, ROOT)
  sys.path.insert(0, os.path.join(ROOT, 'scripts'))
  import train as train_driver
  import export_density
  from test_gpu_field_query import GIN
  from nerfies_amd import datasets, gin_lite as gin
  cap, exp = str(tmp_path / 'cap'), str(tmp_path / 'exp')
  datasets.write_synthetic_scene(cap, num_frames=8, size=(24, 16))
  cfg = tmp_path / 'run.gin'
  cfg.write_text(GIN)
  args = ['--base_folder', exp, '--data_dir', cap, '--gin_configs', str(cfg)]
  gin.clear_config()
  train_driver.main(args)
  common = args + ['--canonical', '--resolution', '8']
  gin.clear_config()
  plain = export_density.main(common + ['--threshold', '1e30'])
  grid = np.load(plain['npy'])
  thr = repr(float(np.sort(grid.ravel())[grid.size // 2]))
  gin.clear_config()
  capsys.readouterr()
  item = sorted(os.path.splitext(n)[0] for n in os.listdir(os.path.join(cap, 'camera')))[0]
  res = export_density.main(common + ['--threshold', thr, '--mesh', '--mesh_refine', '1', '--render_mesh', item, '--render_shading', 'normals'])
  printed = capsys.readouterr().out
  gin.clear_config()
  got = res['rendered'][item]
  from PIL import Image
  image = np.asarray(Image.open(got['png']))
  depth = np.load(got['depth_npy'])
  assert image.shape == (16, 24, 3) and image.dtype == np.uint8 and depth.shape == (16, 24) and depth.dtype == np.float32
  assert os.path.basename(got['png']) == f'mesh_render_{item}.png' and os.path.basename(got['depth_npy']) == f'mesh_depth_{item}.npy'
  assert 0.0 <= got['covered'] <= 1.0 and np.isclose(got['covered'], (depth > 0).mean())
  assert (image[depth == 0] == 255).all()                                # the white background where nothing is covered
  line = [l for l in printed.splitlines() if l.startswith(f'mesh_render_{item}:')]
  assert len(line) == 1 and 'of the pixels covered' in line[0] and 'median |mesh ray distance - NeRF depth|' in line[0]
  print(line[0])
  if got['covered'] > 0:
    assert np.isfinite(got['median_abs_depth_difference']) and (depth[depth > 0] > 0).all()
