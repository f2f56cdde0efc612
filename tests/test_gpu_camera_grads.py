"""Camera tables on the GPU (nrf_camera_table_*, csrc/camera.hip; nerfies_amd.camera.rays_from_table / project_from_table): the forward
against the by-value kernels and the oracle, the reverse passes into the camera parameters against central differences of
oracle/camera_oracle.py in float64.

Reference of every camera gradient: per camera and per parameter p, (L(p + h) - L(p - h)) / 2h of the float64 oracle with
h = 1e-6 max(1, |p|), L = sum d_o . o + d_d . d (rays) or sum d_px . px (projection).  Gate, per camera and per parameter group
(GROUPS below): max |err| <= GATE = 2e-4 of the reference's max-abs over that group.  The finite difference itself is within 2e-5 of the
exact float64 gradient (worst: skew, whose gradient is tiny) and a float32 restatement of the formulas errs by <= 6e-6, so the gate is
10 x the reference's own noise.  d_pixels / d_points: the same gate, per camera over its rays, against float64 torch autograd of the
restatement below, which is itself checked against the oracle's values.  Every comparison prints its worst ratio
(profiles/camera_grads.md keeps a copy)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import helpers as H
from nerfies_amd import lib as L
from nerfies_amd.camera import CAMERA_PARAM_SLICES as SL, pack_cameras, project_from_table, rays_from_table
from oracle import camera_oracle as CO
from test_gpu_camera import _pair

pytestmark = pytest.mark.gpu

GATE = 2e-4
GROUPS = {'orientation': SL['orientation'], 'position': SL['position'], 'focal': SL['focal_length'], 'principal point': SL['principal_point'],
          'skew': SL['skew'], 'aspect': SL['pixel_aspect_ratio'], 'radial': SL['radial_distortion'], 'tangential': SL['tangential_distortion']}
SIZE = (320, 240)


# ---- inputs ----
def _cameras(num, seed, undistorted=(), **kw):
  """`num` cameras as tests/test_gpu_camera.py::_pair builds them -> (Cameras, float64 rows (num, 22) of their float32 values)."""
  cams = [_pair(seed + 17 * c, distorted=c not in undistorted, **kw)[0] for c in range(num)]
  rows = np.stack([np.concatenate([np.asarray(getattr(cam, k), np.float64).reshape(-1) for k in SL]) for cam in cams])
  return cams, rows


def _ocam(row, size=SIZE):
  return CO.make_camera(row[SL['orientation']], row[SL['position']], row[12], row[SL['principal_point']], size, row[15], row[16],
                        row[SL['radial_distortion']], row[SL['tangential_distortion']])


def _index(pattern, n, rng):
  """-> (number of cameras, int32 index or None, undistorted cameras)."""
  if pattern == 'null':
    return 1, None, ()
  if pattern == 'random3':
    return 3, rng.integers(0, 3, n).astype(np.int32), (1,)
  if pattern in ('random4', 'random5'):
    num = int(pattern[-1])
    return num, rng.integers(0, num, n).astype(np.int32), (2,)
  assert pattern == 'sorted5'   # runs that cross workgroup boundaries; camera 3 owns no ray
  return 5, np.sort(rng.choice(np.array([0, 1, 2, 4], np.int32), n)), ()


def _fd(rows, idx, loss_of_camera):
  """Central differences per camera and parameter: loss_of_camera(c, oracle camera, rays of c) -> float."""
  out = np.zeros((rows.shape[0], 22))
  for c in range(rows.shape[0]):
    sel = np.nonzero(idx == c)[0]
    if sel.size == 0:
      continue
    for p in range(22):
      h = 1e-6 * max(1.0, abs(rows[c, p]))
      hi, lo = rows[c].copy(), rows[c].copy()
      hi[p] += h
      lo[p] -= h
      out[c, p] = (loss_of_camera(_ocam(hi), sel) - loss_of_camera(_ocam(lo), sel)) / (2 * h)
  return out


def _gate(got, want, label, zero=()):
  """The gate of the module docstring on a (C, 24) gradient against a (C, 22) reference; pads and empty cameras exactly 0, and so are
  the groups named in `zero` (on both sides)."""
  got = got.detach().cpu().double().numpy()
  assert not got[:, 22:].any(), f'{label}: pad gradients'
  worst = 0.0
  for c in range(want.shape[0]):
    if not want[c].any():
      assert not got[c].any(), f'{label}: camera {c} owns no ray'
      continue
    for name, sl in GROUPS.items():
      scale = np.abs(want[c, sl]).max()
      if name in zero:
        assert scale == 0 and not got[c, sl].any(), (label, c, name)
        continue
      assert scale > 0, (label, c, name)
      ratio = np.abs(got[c, sl] - want[c, sl]).max() / scale
      worst = max(worst, ratio)
      assert ratio <= GATE, f'{label}: camera {c} {name}: error / max-abs {ratio:.2e} > {GATE:.0e}'
  print(f'[{label}] worst group error / max-abs {worst:.2e} (gate {GATE:.0e})')
  return worst


def _gate_rays(got, want, idx, label):
  got = got.detach().cpu().double().numpy()
  worst = 0.0
  for c in np.unique(idx):
    sel = idx == c
    scale = np.abs(want[sel]).max()
    ratio = np.abs(got[sel] - want[sel]).max() / scale
    worst = max(worst, ratio)
    assert ratio <= GATE, f'{label}: camera {c}: error / max-abs {ratio:.2e} > {GATE:.0e}'
  print(f'[{label}] worst per-camera error / max-abs {worst:.2e} (gate {GATE:.0e})')


# ---- float64 torch restatement (for d_pixels / d_points only; values pinned to the oracle where it is used) ----
def _t_distort(x, y, k, p):
  r2 = x * x + y * y
  d = 1.0 + r2 * (k[:, 0] + r2 * (k[:, 1] + k[:, 2] * r2))
  return (x * d + 2.0 * p[:, 0] * x * y + p[:, 1] * (r2 + 2.0 * x * x), y * d + 2.0 * p[:, 1] * x * y + p[:, 0] * (r2 + 2.0 * y * y))


def _t_rays(rows, px):
  """rows (n, 22) float64 per ray, px (n, 2) -> directions (n, 3); ten Newton steps differentiated as they are."""
  R, f, cx, cy, s, a = rows[:, :9].reshape(-1, 3, 3), rows[:, 12], rows[:, 13], rows[:, 14], rows[:, 15], rows[:, 16]
  k, p = rows[:, 17:20], rows[:, 20:22]
  yd = (px[:, 1] - cy) / (f * a)
  xd = (px[:, 0] - cx - yd * s) / f
  x, y = xd, yd
  for _ in range(10):
    r2 = x * x + y * y
    d = 1.0 + r2 * (k[:, 0] + r2 * (k[:, 1] + k[:, 2] * r2))
    gx, gy = _t_distort(x, y, k, p)
    fx, fy = gx - xd, gy - yd
    dd = k[:, 0] + r2 * (2.0 * k[:, 1] + 3.0 * k[:, 2] * r2)
    A = d + 2.0 * x * x * dd + 2.0 * p[:, 0] * y + 6.0 * p[:, 1] * x
    B = 2.0 * x * y * dd + 2.0 * p[:, 0] * x + 2.0 * p[:, 1] * y
    Cc = 2.0 * x * y * dd + 2.0 * p[:, 1] * y + 2.0 * p[:, 0] * x
    E = d + 2.0 * y * y * dd + 2.0 * p[:, 1] * x + 6.0 * p[:, 0] * y
    det = Cc * B - A * E
    x, y = x + (fx * E - fy * B) / det, y + (fy * A - fx * Cc) / det
  local = torch.stack([x, y, torch.ones_like(x)], -1)
  local = local / local.norm(dim=-1, keepdim=True)
  world = torch.einsum('ni,nij->nj', local, R)
  return world / world.norm(dim=-1, keepdim=True)


def _t_project(rows, pts):
  R, pos, f, cx, cy, s, a = rows[:, :9].reshape(-1, 3, 3), rows[:, 9:12], rows[:, 12], rows[:, 13], rows[:, 14], rows[:, 15], rows[:, 16]
  local = torch.einsum('nij,nj->ni', R, pts - pos)
  x, y = _t_distort(local[:, 0] / local[:, 2], local[:, 1] / local[:, 2], rows[:, 17:20], rows[:, 20:22])
  return torch.stack([f * x + s * y + cx, f * a * y + cy], -1)


# ---- one case: inputs, oracle values, references (computed once, shared, never modified) ----
class Case:
  def __init__(self, pattern, n, seed=0):
    rng = np.random.default_rng(1000 * seed + n)
    self.n = n
    self.C, self.idx, und = _index(pattern, n, rng)
    self.cams, self.rows = _cameras(self.C, seed + 3, und)
    self.idx0 = self.idx if self.idx is not None else np.zeros(n, np.int32)
    self.px = rng.uniform(0, SIZE, size=(n, 2)).astype(np.float32)
    self.d_o = rng.normal(size=(n, 3)).astype(np.float32)
    self.d_d = rng.normal(size=(n, 3)).astype(np.float32)
    self.d_px = rng.normal(size=(n, 2)).astype(np.float32)
    depth = rng.uniform(0.5, 3.0, n)
    self.pts = np.zeros((n, 3), np.float32)
    for c in range(self.C):
      sel = self.idx0 == c
      self.pts[sel] = CO.pixels_to_points(_ocam(self.rows[c]), self.px[sel], depth[sel])
    self.table = pack_cameras(self.cams, H.DEV)
    self.gidx = torch.from_numpy(self.idx).to(H.DEV) if self.idx is not None else None
    g = lambda a: torch.from_numpy(a).to(H.DEV)
    self.gpx, self.gpts, self.gd_o, self.gd_d, self.gd_px = g(self.px), g(self.pts), g(self.d_o), g(self.d_d), g(self.d_px)

  @functools.cached_property
  def fd_directions(self):
    return _fd(self.rows, self.idx0, lambda oc, sel: float((self.d_d[sel] * CO.pixels_to_rays(oc, self.px[sel])).sum()))

  @functools.cached_property
  def fd_origins(self):
    return _fd(self.rows, self.idx0, lambda oc, sel: float((self.d_o[sel].astype(np.float64) * oc['position']).sum()))

  @functools.cached_property
  def fd_project(self):
    return _fd(self.rows, self.idx0, lambda oc, sel: float((self.d_px[sel] * CO.project(oc, self.pts[sel])).sum()))

  def oracle_rays(self):
    out = np.zeros((self.n, 3))
    for c in range(self.C):
      out[self.idx0 == c] = CO.pixels_to_rays(_ocam(self.rows[c]), self.px[self.idx0 == c])
    return out

  def oracle_project(self):
    out = np.zeros((self.n, 2))
    for c in range(self.C):
      out[self.idx0 == c] = CO.project(_ocam(self.rows[c]), self.pts[self.idx0 == c])
    return out

  @functools.cached_property
  def autograd_d_pixels(self):
    rows = torch.from_numpy(self.rows)[torch.from_numpy(self.idx0).long()]
    px = torch.from_numpy(self.px).double().requires_grad_(True)
    d = _t_rays(rows, px)
    np.testing.assert_allclose(d.detach().numpy(), self.oracle_rays(), rtol=0, atol=1e-12)
    return torch.autograd.grad((d * torch.from_numpy(self.d_d).double()).sum(), px)[0].numpy()

  @functools.cached_property
  def autograd_d_points(self):
    rows = torch.from_numpy(self.rows)[torch.from_numpy(self.idx0).long()]
    pts = torch.from_numpy(self.pts).double().requires_grad_(True)
    px = _t_project(rows, pts)
    np.testing.assert_allclose(px.detach().numpy(), self.oracle_project(), rtol=0, atol=1e-9)
    return torch.autograd.grad((px * torch.from_numpy(self.d_px).double()).sum(), pts)[0].numpy()


@functools.lru_cache(maxsize=None)
def _case(pattern, n):
  return Case(pattern, n)


def _workspace(n, num_cameras, fill=None):
  lib = L.load_library()
  b = C.c_size_t(0)
  L.check(lib.nrf_camera_table_workspace_bytes(n, num_cameras, C.byref(b)), lib)
  ws = torch.empty(b.value // 4, dtype=torch.float32, device=H.DEV)
  if fill is not None:
    ws.fill_(fill)
  return ws


def _rays_backward(case, d_o, d_d, fill=None, want_d_pixels=True):
  """nrf_camera_table_rays_backward called directly -> (d_cameras, d_pixels)."""
  lib = L.load_library()
  ws = _workspace(case.n, case.C, fill)
  d_cam = torch.full((case.C, 24), float('nan') if fill is None else fill, device=H.DEV)
  d_px = torch.full((case.n, 2), float('nan'), device=H.DEV) if want_d_pixels else None
  p = lambda t: t.data_ptr() if t is not None else None
  L.check(lib.nrf_camera_table_rays_backward(case.table.data_ptr(), case.C, p(case.gidx), case.gpx.data_ptr(), case.n, p(d_o), p(d_d),
                                             d_cam.data_ptr(), p(d_px), ws.data_ptr(), ws.numel() * 4,
                                             torch.cuda.current_stream().cuda_stream), lib)
  torch.cuda.synchronize()
  return d_cam, d_px


# ---- 1. forward ----
def test_forward_equals_the_by_value_kernels_and_the_oracle():
  rng = np.random.default_rng(5)
  n, C3 = 1000, 3
  cams, rows = _cameras(C3, 11, undistorted=(1,))
  idx = rng.integers(0, C3, n).astype(np.int32)
  px = rng.uniform(0, SIZE, size=(n, 2)).astype(np.float32)
  table = pack_cameras(cams, H.DEV)
  gpx, gidx = torch.from_numpy(px).to(H.DEV), torch.from_numpy(idx).to(H.DEV)
  origins, directions = rays_from_table(table, gpx, gidx)
  assert origins.shape == directions.shape == (n, 3) and not directions.requires_grad
  depth = rng.uniform(0.5, 3.0, n)
  pts = np.zeros((n, 3), np.float32)
  for c, cam in enumerate(cams):
    pts[idx == c] = CO.pixels_to_points(_ocam(rows[c]), px[idx == c], depth[idx == c])
  gpts = torch.from_numpy(pts).to(H.DEV)
  pixels = project_from_table(table, gpts, gidx)
  assert pixels.shape == (n, 2)
  for c, cam in enumerate(cams):
    sel = torch.from_numpy(idx == c).to(H.DEV)
    assert int(sel.sum()) > 0
    by_value = cam.pixels_to_rays(gpx[sel])
    err = (directions[sel] - by_value).abs().max().item()
    print(f'camera {c}: rays table vs by-value max |diff| {err:.2e} (bit-identical: {torch.equal(directions[sel], by_value)})')
    assert err <= 2.4e-7
    np.testing.assert_allclose(directions[sel].cpu().numpy(), CO.pixels_to_rays(_ocam(rows[c]), px[idx == c]), rtol=0, atol=2e-6)
    assert torch.equal(origins[sel], torch.from_numpy(cam.position).to(H.DEV).expand(int(sel.sum()), 3))
    by_value = cam.project(gpts[sel])
    err = (pixels[sel] - by_value).abs().max().item()
    print(f'camera {c}: project table vs by-value max |diff| {err:.2e} px (bit-identical: {torch.equal(pixels[sel], by_value)})')
    assert err <= 2e-3
    np.testing.assert_allclose(pixels[sel].cpu().numpy(), CO.project(_ocam(rows[c]), pts[idx == c]), rtol=0, atol=2e-3)
  # NULL index = row 0; batch shape kept; [..., 1] index accepted
  o0, d0 = rays_from_table(table, gpx.reshape(10, 100, 2))
  assert d0.shape == (10, 100, 3) and (d0.reshape(n, 3) - cams[0].pixels_to_rays(gpx)).abs().max().item() <= 2.4e-7
  assert torch.equal(o0.reshape(n, 3), torch.from_numpy(cams[0].position).to(H.DEV).expand(n, 3))
  o1, d1 = rays_from_table(table, gpx, gidx.reshape(n, 1))
  assert torch.equal(d1, directions) and torch.equal(o1, origins)


# ---- 2. rays VJP ----
@pytest.mark.parametrize('pattern', ['null', 'random3', 'sorted5'])
@pytest.mark.parametrize('n', [1, 63, 64, 65, 255, 256, 257, 1000, 4097])
def test_rays_vjp_against_the_oracle(n, pattern):
  case = _case(pattern, n)
  label = f'rays n={n} {pattern}'
  table = case.table.clone().requires_grad_(True)
  px = case.gpx.clone().requires_grad_(True)
  origins, directions = rays_from_table(table, px, case.gidx)
  ((origins * case.gd_o).sum() + (directions * case.gd_d).sum()).backward()
  _gate(table.grad, case.fd_origins + case.fd_directions, label + ' d_origins + d_directions')
  _gate_rays(px.grad, case.autograd_d_pixels, case.idx0, label + ' d_pixels')
  # the library call itself: either cotangent alone, and none
  both, d_px = _rays_backward(case, case.gd_o, case.gd_d)
  assert torch.equal(both, table.grad) and torch.equal(d_px, px.grad)
  only_o, _ = _rays_backward(case, case.gd_o, None)
  _gate(only_o, case.fd_origins, label + ' d_origins only', zero=[g for g in GROUPS if g != 'position'])   # origin = position
  only_d, _ = _rays_backward(case, None, case.gd_d)
  _gate(only_d, case.fd_directions, label + ' d_directions only', zero=['position'])
  none, d_px0 = _rays_backward(case, None, None)
  assert not none.any() and not d_px0.any()


# ---- 3. a camera without distortion still learns its coefficients ----
def test_undistorted_camera_gets_coefficient_gradients():
  """k = p = 0: the forward skips the undistort, the reverse pass differentiates it at J = I.  The oracle turns its undistort on at
  +-h, so its central difference is the limit the formula gives."""
  case = _case('random3', 1000)
  assert not case.rows[1, 17:22].any() and case.rows[0, 17:22].all()
  d_cam, _ = _rays_backward(case, None, case.gd_d, want_d_pixels=False)
  want = case.fd_directions
  assert np.abs(want[1, 17:20]).max() > 0 and np.abs(want[1, 20:22]).max() > 0
  _gate(d_cam, want, 'undistorted camera 1 of 3', zero=['position'])
  # ... and of the projection
  lib = L.load_library()
  ws = _workspace(case.n, case.C)
  d_cam = torch.empty((case.C, 24), device=H.DEV)
  L.check(lib.nrf_camera_table_project_backward(case.table.data_ptr(), case.C, case.gidx.data_ptr(), case.gpts.data_ptr(), case.n,
                                                case.gd_px.data_ptr(), d_cam.data_ptr(), None, ws.data_ptr(), ws.numel() * 4,
                                                torch.cuda.current_stream().cuda_stream), lib)
  _gate(d_cam, case.fd_project, 'projection, undistorted camera 1 of 3')


# ---- 4. projection VJP ----
@pytest.mark.parametrize('n', [1, 257, 1000])
def test_project_vjp_against_the_oracle(n):
  case = _case('random4', n)
  label = f'project n={n} C=4'
  table = case.table.clone().requires_grad_(True)
  pts = case.gpts.clone().requires_grad_(True)
  pixels = project_from_table(table, pts, case.gidx)
  np.testing.assert_allclose(pixels.detach().cpu().numpy(), case.oracle_project(), rtol=0, atol=2e-3)
  (pixels * case.gd_px).sum().backward()
  _gate(table.grad, case.fd_project, label + ' d_cameras')
  _gate_rays(pts.grad, case.autograd_d_points, case.idx0, label + ' d_points')
  # without a requires_grad on the points the library gets d_points = NULL and the same table gradient
  table2 = case.table.clone().requires_grad_(True)
  (project_from_table(table2, case.gpts, case.gidx) * case.gd_px).sum().backward()
  assert torch.equal(table2.grad, table.grad)


# ---- 5. determinism ----
@pytest.mark.parametrize('pattern,n', [('random5', 4097), ('null', 12288)])
def test_reverse_pass_repeats_bit_for_bit(pattern, n):
  case = _case(pattern, n)
  first, px1 = _rays_backward(case, case.gd_o, case.gd_d, fill=0.0)
  again, px2 = _rays_backward(case, case.gd_o, case.gd_d, fill=0.0)
  poisoned, px3 = _rays_backward(case, case.gd_o, case.gd_d, fill=float('nan'))
  assert first.abs().max().item() > 0 and torch.isfinite(first).all()
  assert torch.equal(first, again) and torch.equal(first, poisoned)
  assert torch.equal(px1, px2) and torch.equal(px1, px3)


def test_no_rays_still_zeroes_the_gradient():
  lib = L.load_library()
  table = _case('random3', 63).table
  ws = _workspace(0, 3, float('nan'))
  for name, extra in (('nrf_camera_table_rays_backward', (None, None)), ('nrf_camera_table_project_backward', (table.data_ptr(),))):
    d_cam = torch.full((3, 24), float('nan'), device=H.DEV)
    L.check(getattr(lib, name)(table.data_ptr(), 3, None, table.data_ptr(), 0, *extra, d_cam.data_ptr(), None, ws.data_ptr(),
                               ws.numel() * 4, torch.cuda.current_stream().cuda_stream), lib)
    assert not d_cam.any(), name
  o, d = rays_from_table(table, torch.zeros((0, 2), device=H.DEV))
  assert o.shape == d.shape == (0, 3)


# ---- 6. graph capture ----
def test_graph_replay_equals_eager():
  """Forward + reverse pass captured on one stream (no allocation, no synchronisation in either) replay to the eager bits."""
  lib = L.load_library()
  case = _case('random5', 4097)
  n = case.n
  ws = _workspace(n, case.C)
  origins, directions = torch.empty((n, 3), device=H.DEV), torch.empty((n, 3), device=H.DEV)
  d_cam, d_px = torch.empty((case.C, 24), device=H.DEV), torch.empty((n, 2), device=H.DEV)

  def step():
    st = torch.cuda.current_stream().cuda_stream
    L.check(lib.nrf_camera_table_rays(case.table.data_ptr(), case.C, case.gidx.data_ptr(), case.gpx.data_ptr(), n, origins.data_ptr(),
                                      directions.data_ptr(), st), lib)
    L.check(lib.nrf_camera_table_rays_backward(case.table.data_ptr(), case.C, case.gidx.data_ptr(), case.gpx.data_ptr(), n,
                                               case.gd_o.data_ptr(), case.gd_d.data_ptr(), d_cam.data_ptr(), d_px.data_ptr(),
                                               ws.data_ptr(), ws.numel() * 4, st), lib)

  s = torch.cuda.Stream()
  s.wait_stream(torch.cuda.current_stream())
  with torch.cuda.stream(s):
    step()
  torch.cuda.current_stream().wait_stream(s)
  torch.cuda.synchronize()
  eager = [t.clone() for t in (origins, directions, d_cam, d_px)]
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph):
    step()
  for t in (origins, directions, d_cam, d_px, ws):
    t.fill_(float('nan'))
  graph.replay()
  torch.cuda.synchronize()
  for want, got in zip(eager, (origins, directions, d_cam, d_px)):
    assert want.abs().max().item() > 0 and torch.equal(want, got)


# ---- 7. the chain through the renderer ----
def _chain():
  from oracle import nerfies_oracle as O
  spec = O.ModelSpec(num_coarse_samples=16, num_fine_samples=16, num_nerf_point_freqs=4, use_stratified_sampling=False,
                     use_warp=False, use_camera_metadata=True)
  model, fp = H.gpu_model(spec, O.init_params(spec, seed=3, trained_like=True))
  cams = []
  for c in range(2):
    cam = _pair(9 + c, size=(12, 9), focal=15.0, skew=0.0, par=1.0)[0]
    cam.position[:] = [0.05 - 0.03 * c, -0.02, 0.1 + 0.02 * c]
    cams.append(cam)
  rows = np.stack([np.concatenate([np.asarray(getattr(cam, k), np.float64).reshape(-1) for k in SL]) for cam in cams])
  px = np.concatenate([cam.get_pixel_centers().reshape(-1, 2) for cam in cams]).astype(np.float32)
  n = px.shape[0]
  g = torch.Generator().manual_seed(12)
  perm = torch.randperm(n, generator=g)   # as the ray table's global permutation mixes the frames
  item_index = torch.arange(2, dtype=torch.int32).repeat_interleave(12 * 9)[perm].reshape(n, 1)
  px = px[perm.numpy()]
  meta = {k: torch.full((n, 1), v, dtype=torch.int32, device=H.DEV) for k, v in (('warp', 2), ('camera', 1), ('appearance', 0))}
  cot = {'rgb': torch.randn(n, 3, generator=g).to(H.DEV), 'depth': torch.randn(n, generator=g).to(H.DEV)}
  return model, fp, cams, rows, torch.from_numpy(px).to(H.DEV), item_index.to(H.DEV), meta, cot


def test_chain_through_the_renderer(monkeypatch):
  from nerfies_amd import autograd
  model, fp, cams, rows, px, item_index, meta, cot = _chain()
  n = px.shape[0]
  table = pack_cameras(cams, H.DEV).requires_grad_(True)
  origins, directions = rays_from_table(table, px, item_index)
  origins.retain_grad()
  directions.retain_grad()
  rays = {'origins': origins, 'directions': directions, 'viewdirs': directions, 'metadata': meta}
  out = autograd.render_differentiable(model, fp.flat, rays, {})
  ((out['fine']['rgb'] * cot['rgb']).sum() + (out['fine']['depth'] * cot['depth']).sum()).backward()
  assert table.grad is not None and table.grad.abs().max().item() > 0
  assert origins.grad.abs().max().item() > 0 and directions.grad.abs().max().item() > 0
  # (a) table.grad is the library's reverse pass of the retained ray gradients
  lib = L.load_library()
  ws = _workspace(n, 2)
  direct = torch.empty((2, 24), device=H.DEV)
  idx = item_index.reshape(-1).contiguous()
  L.check(lib.nrf_camera_table_rays_backward(table.data_ptr(), 2, idx.data_ptr(), px.data_ptr(), n, origins.grad.data_ptr(),
                                             directions.grad.data_ptr(), direct.data_ptr(), None, ws.data_ptr(), ws.numel() * 4,
                                             torch.cuda.current_stream().cuda_stream), lib)
  assert torch.equal(direct, table.grad)
  # (b) <table.grad, v> = sum d_o . delta o + d_d . delta d, delta = central differences of the oracle cameras along v
  d_o, d_d = origins.grad.cpu().double().numpy(), directions.grad.cpu().double().numpy()
  grad = table.grad.cpu().double().numpy()[:, :22]
  idx_h, px_h = idx.cpu().numpy(), px.cpu().numpy()

  def rays_of(r):
    o, d = np.zeros((n, 3)), np.zeros((n, 3))
    for c in range(2):
      oc = _ocam(r[c], (12, 9))
      o[idx_h == c] = oc['position']
      d[idx_h == c] = CO.pixels_to_rays(oc, px_h[idx_h == c])
    return o, d

  rng = np.random.default_rng(21)
  for trial in range(3):
    v = np.zeros_like(rows)
    for name, sl in GROUPS.items():   # each group moves by its own magnitude (1e-2 where the parameter is 0, as the skew here)
      mag = np.abs(rows[:, sl]).max()
      v[:, sl] = rng.normal(size=v[:, sl].shape) * (mag if mag > 0 else 1e-2)
    h = 1e-6
    (o_hi, d_hi), (o_lo, d_lo) = rays_of(rows + h * v), rays_of(rows - h * v)
    delta_o, delta_d = (o_hi - o_lo) / (2 * h), (d_hi - d_lo) / (2 * h)
    want = (d_o * delta_o).sum() + (d_d * delta_d).sum()
    scale = (np.abs(d_o) * np.abs(delta_o)).sum() + (np.abs(d_d) * np.abs(delta_d)).sum()
    got = (grad * v).sum()
    print(f'[chain direction {trial}] <grad, v> {got:.6e}, oracle {want:.6e}, |diff| / sum |d||delta| {abs(got - want) / scale:.2e} (gate {GATE:.0e})')
    assert scale > 0 and abs(got - want) <= GATE * scale
  # (c) no requires_grad on the table: the rays carry no grad_fn and the renderer takes the path and flag word it took before
  seen = []
  real = model.lib.nrf_forward

  def spy(*a):
    seen.append(int(a[6]))
    return real(*a)
  monkeypatch.setattr(model.lib, 'nrf_forward', spy)
  o2, d2 = rays_from_table(table.detach(), px, item_index)
  assert not o2.requires_grad and not d2.requires_grad and torch.equal(d2, directions.detach())
  autograd.render_differentiable(model, fp.flat, {'origins': o2, 'directions': d2, 'viewdirs': d2, 'metadata': meta}, {})
  assert seen == [L.NRF_FLAG_TRAIN], seen


# ---- 8. datasets ----
def test_ray_table_item_index_reproduces_the_rays(tmp_path):
  from nerfies_amd import datasets
  datasets.write_synthetic_scene(str(tmp_path), num_frames=4, size=(16, 12))
  src = datasets.NerfiesDataSource(str(tmp_path), image_scale=1, use_warp_id=True, use_appearance_id=True, use_camera_id=True)
  ids = src.train_ids
  plain = src.create_ray_table(ids, H.DEV)
  kept = src.create_ray_table(ids, H.DEV, keep_item_index=True)
  assert sorted(kept.columns) == sorted(list(plain.columns) + ['item_index'])
  for k, v in plain.columns.items():
    assert torch.equal(v, kept.columns[k]), k
  ii = kept.columns['item_index']
  n = 3 * 16 * 12
  assert ii.shape == (n, 1) and ii.dtype == torch.int32 and sorted(ii.unique().tolist()) == [0, 1, 2]
  assert 'item_index' in kept.batch(0, 8) and 'item_index' not in kept.batch(0, 8).get('metadata', {})
  table = src.camera_table(ids, H.DEV)
  assert table.shape == (3, 24)
  origins, directions = rays_from_table(table, kept.columns['pixels'], ii)
  assert (directions - kept.columns['directions']).abs().max().item() <= 2.4e-7
  assert (origins - kept.columns['origins']).abs().max().item() <= 2.4e-7
