"""Field queries on the host (no GPU): the header's two structs against their ctypes mirrors, NRF_HAS_FIELD_QUERY next to an unchanged
NRF_VERSION, every refusal nrf_query_points / nrf_query_grid decide before any HIP call (one assertion per rule, the offending name
in nrf_last_error), the workspace size (and the recorded sizes of every side plan), the ray plans' digests behind a query plan, and the chunking of
evaluation.density_grid."""
import ctypes as C
import importlib.util
import json
import os
import shutil
import subprocess

import pytest

import helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'nerfies_amd.h')
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
NRF_E_NULL, NRF_E_SHAPE, NRF_E_UNSUPPORTED, NRF_E_WORKSPACE = -1, -2, -3, -5   # include/nerfies_amd.h


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


@pytest.fixture(scope='module')
def handles(lib):
  """One handle per model of tests/golden/make_plan_digests.py that a rule needs."""
  mk = _maker()
  hs = {}
  for name in ('A', 'se3_vrig', 'time_warp', 'one_level', 'alpha_cond'):
    h = C.c_void_p()
    d = mk.desc(**mk.MODELS[name])
    assert lib.nrf_create(C.byref(d), C.byref(h)) == 0, lib.nrf_last_error()
    hs[name] = h
  yield hs
  for h in hs.values():
    lib.nrf_destroy(h)


def test_structs_and_macros_match_the_compiled_header(tmp_path, lib):
  from nerfies_amd import lib as L
  cc = shutil.which('gcc') or shutil.which('cc')
  assert cc is not None, 'no C compiler'
  pairs = [('nrf_field_out', L.FieldOut), ('nrf_grid', L.Grid)]
  lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', 'int main(void) {']
  for cname, ct in pairs:
    lines.append(f'  printf("{cname} size %zu\\n", sizeof({cname}));')
    for fname, _ in ct._fields_:
      lines.append(f'  printf("{cname} {fname} %zu\\n", offsetof({cname}, {fname}));')
  lines += ['  printf("NRF_HAS_FIELD_QUERY %d\\n", NRF_HAS_FIELD_QUERY);', '  printf("NRF_VERSION %d\\n", NRF_VERSION);',
            '  printf("NRF_QUERY_MAX_POINTS %d\\n", NRF_QUERY_MAX_POINTS);', '  return 0;', '}']
  src = tmp_path / 'abi.c'
  src.write_text('\n'.join(lines))
  exe = tmp_path / 'abi'
  subprocess.run([cc, '-std=c99', '-Wall', '-Werror', str(src), '-o', str(exe)], check=True)
  got = {}
  for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines():
    *k, v = line.split()
    got[' '.join(k)] = int(v)
  for cname, ct in pairs:
    assert got[f'{cname} size'] == C.sizeof(ct), (cname, got[f'{cname} size'], C.sizeof(ct))
    for fname, _ in ct._fields_:
      assert got[f'{cname} {fname}'] == getattr(ct, fname).offset, (cname, fname)
  assert got['NRF_HAS_FIELD_QUERY'] == 1
  assert got['NRF_VERSION'] == 660 == lib.nrf_version() == L.NRF_VERSION
  assert got['NRF_QUERY_MAX_POINTS'] == L.NRF_QUERY_MAX_POINTS == 1 << 24
  for name in ('nrf_query_workspace_bytes', 'nrf_query_points', 'nrf_query_grid'):
    assert name in L.EXPORTS and hasattr(lib, name), name


class _Call:
  """nrf_query_points / nrf_query_grid with stand-in buffers: nothing is touched before a refusal."""

  def __init__(self, lib, h):
    from nerfies_amd import lib as L
    self.L, self.lib, self.h = L, lib, h
    self.buf = (C.c_float * 64)()
    self.p = C.cast(self.buf, C.c_void_p)
    self.sc = L.StepScalars()

  def groups(self, n=2, **kw):
    r = self.L.Rays(num_rays=n)
    for k in kw:
      setattr(r, k, self.p)
    return r

  def points(self, h='h', params='p', groups=None, points='p', S=3, level=0, scalars='sc', flags=0, out=None, ws='p', nbytes=1 << 40):
    L = self.L
    g = groups if groups is not None else self.groups(viewdirs=1, warp_ids=1, appearance_ids=1, camera_ids=1)
    o = out if out is not None else L.FieldOut(sigma=self.p)
    pick = lambda v: self.p if v == 'p' else v
    return self.lib.nrf_query_points(self.h if h == 'h' else h, pick(params), None if g is False else C.byref(g), pick(points), S, level,
                                     C.byref(self.sc) if scalars == 'sc' else scalars, flags, None if o is False else C.byref(o), pick(ws),
                                     nbytes, None)

  def grid(self, dims=(5, 3, 7), first=0, count=105, groups=None, grid='g', level=0, flags=0, out=None, nbytes=1 << 40):
    L = self.L
    g = groups if groups is not None else self.groups(1, viewdirs=1, warp_ids=1, appearance_ids=1, camera_ids=1)
    o = out if out is not None else L.FieldOut(sigma=self.p)
    gr = L.Grid((C.c_float * 3)(0, 0, 0), (C.c_float * 3)(1, 1, 1), (C.c_int32 * 3)(*dims), 0)
    return self.lib.nrf_query_grid(self.h, self.p, C.byref(g), C.byref(gr) if grid == 'g' else grid, first, count, level,
                                   C.byref(self.sc), flags, C.byref(o), self.p, nbytes, None)

  def err(self):
    return self.lib.nrf_last_error()


def test_null_arguments(lib, handles):
  c = _Call(lib, handles['se3_vrig'])
  assert c.points(h=None) == NRF_E_NULL and b'handle' in c.err()
  assert c.points(params=None) == NRF_E_NULL and b'params' in c.err()
  assert c.points(points=None) == NRF_E_NULL and b'points' in c.err()
  assert c.points(scalars=None) == NRF_E_NULL and b'scalars' in c.err()
  assert c.points(out=False) == NRF_E_NULL and b'out' in c.err()
  assert c.points(groups=False) == NRF_E_NULL and b'groups' in c.err()
  assert c.points(ws=None) == NRF_E_NULL and b'workspace' in c.err()
  assert c.grid(grid=None) == NRF_E_NULL and b'grid' in c.err()
  # ids a model needs and the groups lack
  assert c.points(groups=c.groups(viewdirs=1, appearance_ids=1, camera_ids=1)) == NRF_E_NULL and b'warp_ids' in c.err()
  full = c.L.FieldOut(sigma=c.p, rgb=c.p)
  assert c.points(groups=c.groups(viewdirs=1, warp_ids=1), out=full) == NRF_E_NULL and b'camera_ids' in c.err()
  a = _Call(lib, handles['alpha_cond'])
  assert a.points(groups=a.groups(viewdirs=1)) == NRF_E_NULL and b'appearance_ids' in a.err()
  n = C.c_size_t(0)
  assert lib.nrf_query_workspace_bytes(None, 1, 1, 0, C.byref(n)) == NRF_E_NULL
  assert lib.nrf_query_workspace_bytes(handles['A'], 1, 1, 0, None) == NRF_E_NULL


def test_shape_rules(lib, handles):
  c = _Call(lib, handles['se3_vrig'])
  assert c.points(groups=c.groups(0, viewdirs=1, warp_ids=1)) == NRF_E_SHAPE and b'num_groups' in c.err()
  assert c.points(groups=c.groups(-3, viewdirs=1, warp_ids=1)) == NRF_E_SHAPE and b'num_groups' in c.err()
  assert c.points(S=0) == NRF_E_SHAPE and b'points_per_group' in c.err()
  assert c.points(S=-1) == NRF_E_SHAPE and b'points_per_group' in c.err()
  assert c.grid(count=0) == NRF_E_SHAPE and b'count' in c.err()
  assert c.grid(count=-5) == NRF_E_SHAPE and b'count' in c.err()
  assert c.points(level=2) == NRF_E_SHAPE and b'level' in c.err()
  assert c.points(level=-1) == NRF_E_SHAPE and b'level' in c.err()
  one = _Call(lib, handles['one_level'])
  assert one.points(level=1) == NRF_E_SHAPE and b'fine' in one.err()
  assert one.points(level=0, nbytes=0) == NRF_E_WORKSPACE   # level 0 of the same model passes every rule but the workspace's
  # 2^24 points pass the count rule (the workspace one refuses them here); one more does not
  g = c.groups((1 << 12) + 1, viewdirs=1, warp_ids=1)
  assert c.points(groups=g, S=1 << 12) == NRF_E_SHAPE and b'1 << 24' in c.err()
  assert c.points(groups=c.groups(1 << 12, viewdirs=1, warp_ids=1), S=1 << 12, nbytes=0) == NRF_E_WORKSPACE
  assert c.grid(dims=(1 << 10, 1 << 10, 1 << 5), count=(1 << 24) + 1) == NRF_E_SHAPE and b'1 << 24' in c.err()
  n = C.c_size_t(0)
  assert lib.nrf_query_workspace_bytes(handles['A'], (1 << 12) + 1, 1 << 12, 0, C.byref(n)) == NRF_E_SHAPE
  # first + count beyond the grid, a negative first, a group of more than one row, an empty axis
  assert c.grid(first=64, count=42) == NRF_E_SHAPE and b'first + count' in c.err()
  assert c.grid(first=-1, count=5) == NRF_E_SHAPE and b'first + count' in c.err()
  assert c.grid(first=64, count=41, nbytes=0) == NRF_E_WORKSPACE   # the last point of the grid is inside
  assert c.grid(groups=c.groups(2, viewdirs=1, warp_ids=1)) == NRF_E_SHAPE and b'num_rays must be 1' in c.err()
  assert c.grid(dims=(5, 0, 7), count=1) == NRF_E_SHAPE and b'dims' in c.err()
  # extents whose product would wrap int64 (and with it the first + count check) are refused as such
  big = (1 << 31) - 1
  assert c.grid(dims=(big, big, big), count=1) == NRF_E_SHAPE and b'NRF_GRID_MAX_POINTS' in c.err()
  assert c.grid(dims=(1 << 20, 1 << 20, 2), count=1) == NRF_E_SHAPE and b'NRF_GRID_MAX_POINTS' in c.err()
  assert c.grid(dims=(1 << 20, 1 << 20, 1), first=(1 << 40) - 1, count=1, nbytes=0) == NRF_E_WORKSPACE


def test_flag_rules(lib, handles):
  from nerfies_amd import lib as L
  c = _Call(lib, handles['se3_vrig'])
  for name in ('NRF_FLAG_TRAIN', 'NRF_FLAG_BF16', 'NRF_FLAG_BF16X3', 'NRF_FLAG_WARP_JACOBIAN', 'NRF_FLAG_RAY_GRADS', 'NRF_FLAG_WARP_F32',
               'NRF_FLAG_FROZEN'):
    bit = getattr(L, name)
    assert c.points(flags=bit) == NRF_E_UNSUPPORTED and name.encode() in c.err(), name
    assert c.points(flags=bit | L.NRF_FLAG_NO_WARP) == NRF_E_UNSUPPORTED and name.encode() in c.err(), name
    assert c.grid(flags=bit) == NRF_E_UNSUPPORTED and name.encode() in c.err(), name
    n = C.c_size_t(0)
    assert lib.nrf_query_workspace_bytes(handles['se3_vrig'], 2, 3, bit, C.byref(n)) == NRF_E_UNSUPPORTED and name.encode() in c.err()
  assert c.points(flags=1 << 20) == NRF_E_UNSUPPORTED and b'unknown bits 0x100000' in c.err()
  assert c.points(flags=0, nbytes=0) == NRF_E_WORKSPACE and c.points(flags=L.NRF_FLAG_NO_WARP, nbytes=0) == NRF_E_WORKSPACE


def test_unsupported_outputs_and_models(lib, handles):
  from nerfies_amd import lib as L
  c = _Call(lib, handles['se3_vrig'])
  wp = L.FieldOut(sigma=c.p, warped_points=c.p)
  assert c.points(out=wp, nbytes=0) == NRF_E_WORKSPACE                       # the warp is on: the output exists
  assert c.points(out=wp, flags=L.NRF_FLAG_NO_WARP) == NRF_E_UNSUPPORTED and b'warped_points' in c.err()
  a = _Call(lib, handles['A'])                                               # a model without a warp field
  assert a.points(out=L.FieldOut(sigma=a.p, warped_points=a.p)) == NRF_E_UNSUPPORTED and b'warped_points' in a.err()
  t = _Call(lib, handles['time_warp'])
  tg = t.groups(viewdirs=1, time=1)
  assert t.points(groups=tg) == NRF_E_UNSUPPORTED and b'time encoder' in t.err()
  assert t.points(groups=tg, flags=L.NRF_FLAG_NO_WARP, nbytes=0) == NRF_E_WORKSPACE   # with the warp off the model runs
  # rgb on a use_viewdirs model without view directions; the density alone needs none
  full = L.FieldOut(sigma=a.p, rgb=a.p)
  assert a.points(groups=a.groups(), out=full) == NRF_E_UNSUPPORTED and b'viewdirs' in a.err()
  assert a.points(groups=a.groups(viewdirs=1), out=full, nbytes=0) == NRF_E_WORKSPACE
  assert a.points(groups=a.groups(), nbytes=0) == NRF_E_WORKSPACE


def test_workspace_size(lib, handles):
  from nerfies_amd import lib as L
  for name in ('A', 'se3_vrig', 'alpha_cond'):
    h = handles[name]
    size = {}
    for G, S in ((1, 1), (3, 37), (70, 1), (2, 64), (1, 1 << 16), (1 << 8, 1 << 8), (1, 1 << 21)):
      n = C.c_size_t(0)
      assert lib.nrf_query_workspace_bytes(h, G, S, 0, C.byref(n)) == 0, lib.nrf_last_error()
      size[G, S] = n.value
      m = C.c_size_t(0)
      assert lib.nrf_query_workspace_bytes(h, G, S, L.NRF_FLAG_NO_WARP, C.byref(m)) == 0 and m.value == n.value   # one answer
    assert size[1, 1] <= size[3, 37] <= size[1, 1 << 16] < size[1, 1 << 21]
    assert size[1, 1 << 16] <= size[1 << 8, 1 << 8]                      # the same points in more groups: the per-group terms grow
    rows = (1 << 21) - (1 << 16)
    per_row = (size[1, 1 << 21] - size[1, 1 << 16]) / rows
    assert 16 <= per_row <= 48, per_row                                  # out4 (16 B), grid points (12), warped points (12), code rows (4)
    # a short workspace is refused before anything runs, by either entry
    c = _Call(lib, h)
    n = C.c_size_t(0)
    assert lib.nrf_query_workspace_bytes(h, 2, 3, 0, C.byref(n)) == 0
    assert c.points(nbytes=n.value - 1) == NRF_E_WORKSPACE and b'nrf_query_workspace_bytes' in c.err()
    assert lib.nrf_query_workspace_bytes(h, 1, 105, 0, C.byref(n)) == 0
    assert c.grid(nbytes=n.value - 1) == NRF_E_WORKSPACE


def test_ray_plans_keep_their_digests_behind_a_query_plan(lib, handles):
  """A query sizes a plan of its own: the handle's ray plan, before and after, is the committed one."""
  with open(os.path.join(GOLDEN, 'plan_digests.json')) as fp:
    rec = json.load(fp)['plans']
  for model in ('A', 'se3_vrig', 'alpha_cond'):
    h = handles[model]
    for rays in (37, 128):
      want = rec[f'{model}/0/rays={rays}/bg=0/elastic=0/rows=0/merge=1']
      n, q, dg = C.c_size_t(0), C.c_size_t(0), C.c_uint64(0)
      assert lib.nrf_query_workspace_bytes(h, rays, 64, 0, C.byref(q)) == 0
      assert lib.nrf_workspace_bytes_ex(h, rays, 0, 0, 0, C.byref(n)) == 0 and n.value == want['workspace_bytes']
      assert lib.nrf_debug_plan_digest(h, C.byref(dg)) == 0 and '%016x' % dg.value == want['digest'], (model, rays)
      assert lib.nrf_query_workspace_bytes(h, 5, 7, 0, C.byref(q)) == 0      # ... and a query plan leaves the ray plan in place
      assert lib.nrf_debug_plan_digest(h, C.byref(dg)) == 0 and '%016x' % dg.value == want['digest'], (model, rays)
      c = _Call(lib, h)
      assert c.points(nbytes=0) == NRF_E_WORKSPACE
      assert lib.nrf_debug_plan_digest(h, C.byref(dg)) == 0 and '%016x' % dg.value == want['digest'], (model, rays)


def test_side_plan_sizes_match_the_record(lib):
  """tests/golden/side_plan_sizes.json: the workspace of every stand-alone field entry, byte for byte (a refusal: its error code)."""
  spec = importlib.util.spec_from_file_location('make_side_plan_sizes', os.path.join(GOLDEN, 'make_side_plan_sizes.py'))
  mod = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(mod)
  with open(os.path.join(GOLDEN, 'side_plan_sizes.json')) as fp:
    want = json.load(fp)['sizes']
  got = mod.sizes(lib)
  assert sorted(got) == sorted(want)
  wrong = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
  assert not wrong, wrong
  warp_models = [m for m, kw in mod.MODELS.items() if kw.get('use_warp', 0)]
  assert len(want) == (len(mod.MODELS) * (len(mod.QUERY_SHAPES) + len(mod.QUERY_GRAD_SHAPES)) * len(mod.QUERY_FLAGS)
                       + len(warp_models) * len(mod.WARP_POINTS))
  assert (1, 1 << 20) in mod.QUERY_GRAD_SHAPES and (256, 256) not in mod.QUERY_GRAD_SHAPES
  assert all(v > 0 for v in want.values())                    # no entry refuses a listed case


def test_density_grid_chunks_cover_the_grid_once(lib):
  import torch
  from nerfies_amd import evaluation, lib as L
  rec = H.RecordingLib(lib, ['nrf_query_grid'])
  model, fp = H.cpu_field_model(rec)
  res, chunk = (5, 3, 7), 32                                   # 105 points: 32 + 32 + 32 + 9
  assert evaluation.grid_chunks(105, 32) == [(0, 32), (32, 32), (64, 32), (96, 9)]
  out = evaluation.density_grid(model, fp, (-1.0, 0.0, 1.0), (1.0, 3.0, 2.0), res, level='coarse', warp_id=2, chunk=chunk)
  assert tuple(out.shape) == res and out.stride() == (1, 5, 15) and out.dtype == torch.float32   # x fastest in memory
  seen = torch.zeros(105, dtype=torch.int32)
  base = out.permute(2, 1, 0).reshape(-1).data_ptr()
  for c in rec.calls:
    seen[c['first']:c['first'] + c['count']] += 1
    assert c['sigma'] == base + 4 * c['first'] and c['rgb'] is None and c['warped'] is None   # density only, each chunk at its offset
    assert c['dims'] == res and c['level'] == 0 and c['flags'] == 0 and c['num_rays'] == 1 and c['warp_ids']
    assert c['step'] == pytest.approx((0.4, 1.0, 1.0 / 7)) and c['origin'] == pytest.approx((-0.8, 0.5, 1.0 + 0.5 / 7))   # voxel centres
  assert [(c['first'], c['count']) for c in rec.calls] == evaluation.grid_chunks(105, chunk)
  assert bool((seen == 1).all())
  assert len({c['nbytes'] for c in rec.calls}) == 1              # one workspace serves every chunk
  n = C.c_size_t(0)                                              # ... of the size the library asks for one whole chunk
  assert lib.nrf_query_workspace_bytes(model.handle, 1, chunk, 0, C.byref(n)) == 0 and rec.calls[0]['nbytes'] == H.ws_bytes(n.value)
  # the canonical volume: no warp id, NRF_FLAG_NO_WARP; a chunk larger than the grid is one call
  rec.calls.clear()
  evaluation.density_grid(model, fp, (0, 0, 0), (1, 1, 1), 4, chunk=1 << 21)
  assert [(c['first'], c['count'], c['flags'], c['level']) for c in rec.calls] == [(0, 64, L.NRF_FLAG_NO_WARP, 1)]
  for total, ch in ((1, 1), (7, 3), (64, 64), (65, 64), (1000, 7)):
    pieces = evaluation.grid_chunks(total, ch)
    assert pieces[0][0] == 0 and sum(n for _, n in pieces) == total and all(0 < n <= ch for _, n in pieces)
    assert all(a + n == b for (a, n), (b, _) in zip(pieces, pieces[1:]))


def test_query_points_runs_in_the_librarys_workspace(lib, monkeypatch):
  """NerfModel.query_points behind its device rule (CPU points raise before anything else): one call, in a cached workspace of the
  size the library asks for its groups."""
  import torch
  from nerfies_amd import lib as L
  rec = H.RecordingLib(lib, ['nrf_query_points'])
  model, fp = H.cpu_field_model(rec)
  pts, view, ids = torch.zeros(3, 5, 3), torch.zeros(3, 3), torch.arange(3, dtype=torch.int32).reshape(3, 1)
  with pytest.raises(L.NrfError, match='GPU'):
    model.query_points(fp, pts, viewdirs=view, metadata={'warp': ids})
  assert rec.calls == []
  H.lift_device_rule(monkeypatch)
  run = lambda: model.query_points(fp, pts, viewdirs=view, metadata={'warp': ids})
  out = run()
  (c,) = rec.calls
  assert (c['num_rays'], c['S'], c['level'], c['flags']) == (3, 5, 1, 0) and c['points'] == pts.data_ptr()
  assert c['sigma'] == out['sigma'].data_ptr() and c['rgb'] == out['rgb'].data_ptr() and c['warped'] is None
  n = C.c_size_t(0)
  assert lib.nrf_query_workspace_bytes(model.handle, 3, 5, 0, C.byref(n)) == 0 and c['nbytes'] == H.ws_bytes(n.value)
  run()
  assert rec.calls[1]['ws'] == c['ws'] == model._ws['query', 3, 5, 'cpu'].data_ptr()   # the cached one, handed out again


@pytest.mark.parametrize('bad', ['shape', 'dtype', 'stride'])
def test_query_grid_refuses_an_output_it_cannot_write(lib, bad):
  import torch
  from nerfies_amd import lib as L
  rec = H.RecordingLib(lib, ['nrf_query_grid'])
  model, fp = H.cpu_field_model(rec)
  rgb = {'shape': torch.zeros(9, 3), 'dtype': torch.zeros(8, 3, dtype=torch.float64), 'stride': torch.zeros(3, 8).t()}[bad]
  with pytest.raises(L.NrfError, match=r"query_grid: out\['rgb'\].*\(8, 3\)"):
    model.query_grid(fp, (0, 0, 0), (1, 1, 1), (2, 2, 2), 0, 8, {'sigma': torch.zeros(8), 'rgb': rgb}, viewdirs=torch.zeros(3), use_warp=False)
  assert rec.calls == []
