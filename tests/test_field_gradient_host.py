"""Gradient queries on the host (no GPU): nrf_field_grad_out against its ctypes mirror, NRF_HAS_FIELD_GRADIENT next to an unchanged
NRF_VERSION, every refusal nrf_query_points_grad / nrf_query_grid_grad decide before any HIP call (one assertion per rule, the
offending name in nrf_last_error), the workspace size, the other plans behind a gradient plan, and the chunking of
NerfModel.query_gradient and evaluation.normal_grid."""
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


def test_struct_and_macros_match_the_compiled_header(tmp_path, lib):
  from nerfies_amd import lib as L
  cc = shutil.which('gcc') or shutil.which('cc')
  assert cc is not None, 'no C compiler'
  cname, ct = 'nrf_field_grad_out', L.FieldGradOut
  lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', 'int main(void) {',
           f'  printf("size %zu\\n", sizeof({cname}));']
  for fname, _ in ct._fields_:
    lines.append(f'  printf("{fname} %zu\\n", offsetof({cname}, {fname}));')
  lines += ['  printf("NRF_HAS_FIELD_GRADIENT %d\\n", NRF_HAS_FIELD_GRADIENT);', '  printf("NRF_VERSION %d\\n", NRF_VERSION);',
            '  printf("NRF_QUERY_GRAD_MAX_POINTS %d\\n", NRF_QUERY_GRAD_MAX_POINTS);',
            '  printf("field_out %zu\\n", sizeof(nrf_field_out));', '  return 0;', '}']
  src = tmp_path / 'abi.c'
  src.write_text('\n'.join(lines))
  exe = tmp_path / 'abi'
  subprocess.run([cc, '-std=c99', '-Wall', '-Werror', str(src), '-o', str(exe)], check=True)
  got = {}
  for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines():
    k, v = line.split()
    got[k] = int(v)
  assert [f for f, _ in ct._fields_] == ['sigma', 'grad_sigma', 'normals', 'warped_points']
  assert got['size'] == C.sizeof(ct) == 32
  for fname, _ in ct._fields_:
    assert got[fname] == getattr(ct, fname).offset, fname
  assert got['NRF_HAS_FIELD_GRADIENT'] == 1
  assert got['NRF_VERSION'] == 660 == lib.nrf_version() == L.NRF_VERSION
  assert got['NRF_QUERY_GRAD_MAX_POINTS'] == L.NRF_QUERY_GRAD_MAX_POINTS == 1 << 20
  assert got['field_out'] == C.sizeof(L.FieldOut) == 24                     # nrf_field_out is as it was
  for name in ('nrf_query_grad_workspace_bytes', 'nrf_query_points_grad', 'nrf_query_grid_grad'):
    assert name in L.EXPORTS and hasattr(lib, name), name


class _Call:
  """nrf_query_points_grad / nrf_query_grid_grad with stand-in buffers: nothing is touched before a refusal."""

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
    g = groups if groups is not None else self.groups(warp_ids=1, appearance_ids=1)
    o = out if out is not None else L.FieldGradOut(sigma=self.p, grad_sigma=self.p, normals=self.p)
    pick = lambda v: self.p if v == 'p' else v
    return self.lib.nrf_query_points_grad(self.h if h == 'h' else h, pick(params), None if g is False else C.byref(g), pick(points), S, level,
                                          C.byref(self.sc) if scalars == 'sc' else scalars, flags, None if o is False else C.byref(o),
                                          pick(ws), nbytes, None)

  def grid(self, dims=(5, 3, 7), first=0, count=105, groups=None, grid='g', level=0, flags=0, out=None, nbytes=1 << 40):
    L = self.L
    g = groups if groups is not None else self.groups(1, warp_ids=1, appearance_ids=1)
    o = out if out is not None else L.FieldGradOut(grad_sigma=self.p)
    gr = L.Grid((C.c_float * 3)(0, 0, 0), (C.c_float * 3)(1, 1, 1), (C.c_int32 * 3)(*dims), 0)
    return self.lib.nrf_query_grid_grad(self.h, self.p, C.byref(g), C.byref(gr) if grid == 'g' else grid, first, count, level,
                                        C.byref(self.sc), flags, C.byref(o), self.p, nbytes, None)

  def err(self):
    return self.lib.nrf_last_error()


def test_null_arguments(lib, handles):
  c = _Call(lib, handles['se3_vrig'])
  assert c.points(h=None) == NRF_E_NULL and b'handle' in c.err()
  assert c.points(params=None) == NRF_E_NULL and b'params' in c.err()
  assert c.points(points=None) == NRF_E_NULL and b'points' in c.err()
  assert c.points(scalars=None) == NRF_E_NULL and b'scalars' in c.err()
  assert c.points(out=False) == NRF_E_NULL and b'nrf_field_grad_out' in c.err()
  assert c.points(groups=False) == NRF_E_NULL and b'groups' in c.err()
  assert c.points(ws=None) == NRF_E_NULL and b'workspace' in c.err()
  assert c.grid(grid=None) == NRF_E_NULL and b'grid' in c.err()
  # ids a model needs and the groups lack; no view direction or camera code is ever needed
  assert c.points(groups=c.groups()) == NRF_E_NULL and b'warp_ids' in c.err()
  assert c.points(groups=c.groups(warp_ids=1), nbytes=0) == NRF_E_WORKSPACE
  a = _Call(lib, handles['alpha_cond'])
  assert a.points(groups=a.groups()) == NRF_E_NULL and b'appearance_ids' in a.err()
  assert a.points(groups=a.groups(appearance_ids=1), nbytes=0) == NRF_E_WORKSPACE
  n = C.c_size_t(0)
  assert lib.nrf_query_grad_workspace_bytes(None, 1, 1, 0, C.byref(n)) == NRF_E_NULL
  assert lib.nrf_query_grad_workspace_bytes(handles['A'], 1, 1, 0, None) == NRF_E_NULL


def test_shape_rules(lib, handles):
  c = _Call(lib, handles['se3_vrig'])
  assert c.points(groups=c.groups(0, warp_ids=1)) == NRF_E_SHAPE and b'num_groups' in c.err()
  assert c.points(groups=c.groups(-3, warp_ids=1)) == NRF_E_SHAPE and b'num_groups' in c.err()
  assert c.points(S=0) == NRF_E_SHAPE and b'points_per_group' in c.err()
  assert c.points(S=-1) == NRF_E_SHAPE and b'points_per_group' in c.err()
  assert c.grid(count=0) == NRF_E_SHAPE and b'count' in c.err()
  assert c.grid(count=-5) == NRF_E_SHAPE and b'count' in c.err()
  assert c.points(level=2) == NRF_E_SHAPE and b'level' in c.err()
  assert c.points(level=-1) == NRF_E_SHAPE and b'level' in c.err()
  one = _Call(lib, handles['one_level'])
  assert one.points(level=1) == NRF_E_SHAPE and b'fine' in one.err()
  assert one.points(level=0, nbytes=0) == NRF_E_WORKSPACE
  # 2^20 points pass the count rule (the workspace one refuses them here); one more does not
  assert c.points(groups=c.groups((1 << 10) + 1, warp_ids=1), S=1 << 10) == NRF_E_SHAPE and b'NRF_QUERY_GRAD_MAX_POINTS' in c.err()
  assert c.points(groups=c.groups(1 << 10, warp_ids=1), S=1 << 10, nbytes=0) == NRF_E_WORKSPACE
  assert c.points(groups=c.groups(1, warp_ids=1), S=(1 << 20) + 1) == NRF_E_SHAPE and b'1 << 20' in c.err()
  assert c.grid(dims=(1 << 10, 1 << 10, 1 << 5), count=(1 << 20) + 1) == NRF_E_SHAPE and b'1 << 20' in c.err()
  assert c.grid(dims=(1 << 10, 1 << 10, 1 << 5), count=1 << 20, nbytes=0) == NRF_E_WORKSPACE
  n = C.c_size_t(0)
  assert lib.nrf_query_grad_workspace_bytes(handles['A'], (1 << 10) + 1, 1 << 10, 0, C.byref(n)) == NRF_E_SHAPE
  assert lib.nrf_query_grad_workspace_bytes(handles['A'], 1 << 10, 1 << 10, 0, C.byref(n)) == 0
  # the grid's own rules
  assert c.grid(first=64, count=42) == NRF_E_SHAPE and b'first + count' in c.err()
  assert c.grid(first=-1, count=5) == NRF_E_SHAPE and b'first + count' in c.err()
  assert c.grid(first=64, count=41, nbytes=0) == NRF_E_WORKSPACE
  assert c.grid(groups=c.groups(2, warp_ids=1)) == NRF_E_SHAPE and b'nrf_query_grid_grad: group->num_rays must be 1' in c.err()
  assert c.grid(dims=(5, 0, 7), count=1) == NRF_E_SHAPE and b'dims' in c.err()
  assert c.grid(dims=(1 << 20, 1 << 20, 2), count=1) == NRF_E_SHAPE and b'NRF_GRID_MAX_POINTS' in c.err()


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
    assert lib.nrf_query_grad_workspace_bytes(handles['se3_vrig'], 2, 3, bit, C.byref(n)) == NRF_E_UNSUPPORTED and name.encode() in c.err()
  assert c.points(flags=1 << 20) == NRF_E_UNSUPPORTED and b'unknown bits 0x100000' in c.err()
  assert c.points(flags=0, nbytes=0) == NRF_E_WORKSPACE and c.points(flags=L.NRF_FLAG_NO_WARP, nbytes=0) == NRF_E_WORKSPACE


def test_unsupported_outputs_and_models(lib, handles):
  from nerfies_amd import lib as L
  c = _Call(lib, handles['se3_vrig'])
  wp = L.FieldGradOut(grad_sigma=c.p, warped_points=c.p)
  assert c.points(out=wp, nbytes=0) == NRF_E_WORKSPACE                       # the warp is on: the output exists
  assert c.points(out=wp, flags=L.NRF_FLAG_NO_WARP) == NRF_E_UNSUPPORTED and b'warped_points' in c.err()
  a = _Call(lib, handles['A'])                                               # a model without a warp field
  assert a.points(groups=a.groups(), out=L.FieldGradOut(sigma=a.p, warped_points=a.p)) == NRF_E_UNSUPPORTED and b'warped_points' in a.err()
  assert a.points(groups=a.groups(), nbytes=0) == NRF_E_WORKSPACE            # no ids, no view direction: the density needs none
  t = _Call(lib, handles['time_warp'])
  tg = t.groups(time=1)
  assert t.points(groups=tg) == NRF_E_UNSUPPORTED and b'time encoder' in t.err()
  assert t.points(groups=tg, flags=L.NRF_FLAG_NO_WARP, nbytes=0) == NRF_E_WORKSPACE   # with the warp off the model runs


def _carve(n):
  """nrf_handle.h Carve::take: every region is rounded up to 64 floats."""
  return (n + 63) // 64 * 64


def test_workspace_size(lib, handles):
  from nerfies_amd import lib as L
  mk = _maker()
  for name in ('A', 'se3_vrig', 'alpha_cond'):
    h = handles[name]
    kw = mk.MODELS[name]
    size = {}
    for G, S in ((1, 1), (3, 37), (70, 1), (2, 64), (1, 1 << 12), (1 << 6, 1 << 6), (1, 1 << 20)):
      n = C.c_size_t(0)
      assert lib.nrf_query_grad_workspace_bytes(h, G, S, 0, C.byref(n)) == 0, lib.nrf_last_error()
      size[G, S] = n.value
      m = C.c_size_t(0)
      assert lib.nrf_query_grad_workspace_bytes(h, G, S, L.NRF_FLAG_NO_WARP, C.byref(m)) == 0 and m.value == n.value   # one answer
      q = C.c_size_t(0)
      assert lib.nrf_query_workspace_bytes(h, G, S, 0, C.byref(q)) == 0 and q.value < n.value   # the stash comes on top of a query's rows
    assert size[1, 1] <= size[3, 37] <= size[1, 1 << 12] < size[1, 1 << 20]
    assert size[1, 1 << 12] <= size[1 << 6, 1 << 6]                        # the same points in more groups: the per-group terms grow
    rows = (1 << 20) - (1 << 12)                                           # whole tiles at both ends: the carve's rounding cancels
    per_row = (size[1, 1 << 20] - size[1, 1 << 12]) / rows
    # Bytes per added row, from the carve (nrf_field.hip QueryGradPlan).  Every model: grid points 12, sign words 8 layers x 4 B per
    # 32 rows... = 8 x 512 words per 64-row tile = 256, posenc stash 4 PKS with PKS = 3 + 6 F rounded up to 32 (F <= 10: 32 or 64),
    # sigma' 4, d points 12.  A warp model adds: code rows 4, warped points 12, trunk input 4 PKSw (PKSw 32 or 64), sign words
    # 6 x 256 words per tile = 96, (w, v) 32, tangent (dw, dv) 96, Jacobian 36.
    F = kw.get('num_nerf_point_freqs', 8)
    pks = (3 + 6 * F + 31) // 32 * 32
    base = 12 + 256 + 4 * pks + 4 + 12
    lo = base + (0 if not kw.get('use_warp', 0) else 4 + 12 + 4 * 32 + 96 + 32 + 96 + 36)
    hi = base + (0 if not kw.get('use_warp', 0) else 4 + 12 + 4 * 64 + 96 + 32 + 96 + 36)
    assert lo <= per_row <= hi, (name, per_row, lo, hi)
    assert per_row <= 1100                                                 # "~1 KB per row": what NRF_QUERY_GRAD_MAX_POINTS is sized by
    # a short workspace is refused before anything runs, by either entry
    c = _Call(lib, h)
    n = C.c_size_t(0)
    assert lib.nrf_query_grad_workspace_bytes(h, 2, 3, 0, C.byref(n)) == 0
    assert c.points(nbytes=n.value - 1) == NRF_E_WORKSPACE and b'nrf_query_grad_workspace_bytes' in c.err()
    assert lib.nrf_query_grad_workspace_bytes(h, 1, 105, 0, C.byref(n)) == 0
    assert c.grid(nbytes=n.value - 1) == NRF_E_WORKSPACE and b'nrf_query_grad_workspace_bytes' in c.err()


def test_other_plans_stay_behind_a_gradient_plan(lib, handles):
  """A gradient query sizes a plan of its own: the query plan's size and the ray plan's digest, before and after, are the committed ones."""
  with open(os.path.join(GOLDEN, 'plan_digests.json')) as fp:
    rec = json.load(fp)['plans']
  for model in ('A', 'se3_vrig', 'alpha_cond'):
    h = handles[model]
    for rays in (37, 128):
      want = rec[f'{model}/0/rays={rays}/bg=0/elastic=0/rows=0/merge=1']
      n, q0, q1, g, dg = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0), C.c_size_t(0), C.c_uint64(0)
      assert lib.nrf_query_workspace_bytes(h, rays, 64, 0, C.byref(q0)) == 0
      assert lib.nrf_workspace_bytes_ex(h, rays, 0, 0, 0, C.byref(n)) == 0 and n.value == want['workspace_bytes']
      assert lib.nrf_debug_plan_digest(h, C.byref(dg)) == 0 and '%016x' % dg.value == want['digest'], (model, rays)
      assert lib.nrf_query_grad_workspace_bytes(h, rays, 64, 0, C.byref(g)) == 0 and g.value > q0.value
      assert lib.nrf_debug_plan_digest(h, C.byref(dg)) == 0 and '%016x' % dg.value == want['digest'], (model, rays)
      assert lib.nrf_query_workspace_bytes(h, rays, 64, 0, C.byref(q1)) == 0 and q1.value == q0.value
      c = _Call(lib, h)
      assert c.points(nbytes=0) == NRF_E_WORKSPACE and c.grid(nbytes=0) == NRF_E_WORKSPACE
      assert lib.nrf_debug_plan_digest(h, C.byref(dg)) == 0 and '%016x' % dg.value == want['digest'], (model, rays)
  # ... and the recorded size of every existing side plan still holds with gradient plans sized on the same handles in between
  spec = importlib.util.spec_from_file_location('make_side_plan_sizes', os.path.join(GOLDEN, 'make_side_plan_sizes.py'))
  mod = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(mod)
  with open(os.path.join(GOLDEN, 'side_plan_sizes.json')) as fp:
    assert mod.sizes(lib) == json.load(fp)['sizes']


def test_normal_grid_chunks_cover_the_grid_once(lib):
  import torch
  from nerfies_amd import evaluation, lib as L
  rec = H.RecordingLib(lib, ['nrf_query_grid_grad', 'nrf_query_points_grad'])
  model, fp = H.cpu_field_model(rec)
  res, chunk = (5, 3, 7), 32                                   # 105 points: 32 + 32 + 32 + 9
  sigma, normals = evaluation.normal_grid(model, fp, (-1.0, 0.0, 1.0), (1.0, 3.0, 2.0), res, level='coarse', warp_id=2, chunk=chunk)
  assert tuple(sigma.shape) == res and sigma.stride() == (1, 5, 15) and sigma.dtype == torch.float32   # x fastest in memory, as density_grid
  assert tuple(normals.shape) == res + (3,) and normals.stride() == (3, 15, 45, 1) and normals.dtype == torch.float32
  seen = torch.zeros(105, dtype=torch.int32)
  sbase = sigma.permute(2, 1, 0).reshape(-1).data_ptr()
  nbase = normals.permute(2, 1, 0, 3).reshape(-1).data_ptr()
  for c in rec.calls:
    seen[c['first']:c['first'] + c['count']] += 1
    assert c['sigma'] == sbase + 4 * c['first'] and c['normals'] == nbase + 12 * c['first'] and c['grad'] is None and c['warped'] is None
    assert c['dims'] == res and c['level'] == 0 and c['flags'] == 0 and c['num_rays'] == 1 and c['warp_ids']
    assert c['step'] == pytest.approx((0.4, 1.0, 1.0 / 7)) and c['origin'] == pytest.approx((-0.8, 0.5, 1.0 + 0.5 / 7))   # voxel centres
  assert [(c['first'], c['count']) for c in rec.calls] == evaluation.grid_chunks(105, chunk)
  assert bool((seen == 1).all())
  assert len({c['nbytes'] for c in rec.calls}) == 1              # one workspace serves every chunk
  n = C.c_size_t(0)                                              # ... of the size the library asks for one whole chunk
  assert lib.nrf_query_grad_workspace_bytes(model.handle, 1, chunk, 0, C.byref(n)) == 0 and rec.calls[0]['nbytes'] == H.ws_bytes(n.value)
  # the canonical volume: no warp id, NRF_FLAG_NO_WARP; a chunk larger than the cap is cut down to it
  rec.calls.clear()
  evaluation.normal_grid(model, fp, (0, 0, 0), (1, 1, 1), 4, chunk=1 << 30)
  assert [(c['first'], c['count'], c['flags'], c['level']) for c in rec.calls] == [(0, 64, L.NRF_FLAG_NO_WARP, 1)]
  rec.calls.clear()
  evaluation.normal_grid(model, fp, (0, 0, 0), (1, 1, 1), (128, 128, 65), chunk=1 << 30)
  assert [(c['first'], c['count']) for c in rec.calls] == [(0, 1 << 20), (1 << 20, 128 * 128)]


def test_query_gradient_chunks_cover_the_points_once(lib, monkeypatch):
  """NerfModel.query_gradient behind its device rule (CPU points raise before anything else): the recorder never follows a pointer,
  so the chunking runs on CPU tensors."""
  import torch
  from nerfies_amd import lib as L
  rec = H.RecordingLib(lib, ['nrf_query_grid_grad', 'nrf_query_points_grad'])
  model, fp = H.cpu_field_model(rec)
  with pytest.raises(L.NrfError, match='GPU'):
    model.query_gradient(fp, torch.zeros(4, 3))
  assert rec.calls == []
  monkeypatch.setattr(L, 'NRF_QUERY_GRAD_MAX_POINTS', 100)     # the Python side's chunk size; the library's own cap is tested above
  H.lift_device_rule(monkeypatch)
  run = lambda pts, md, use_warp, outputs: model.query_gradient(fp, pts, metadata=md, use_warp=use_warp, outputs=outputs)
  G, S = 7, 37                                                 # 2 groups per call: 2 + 2 + 2 + 1
  ids = torch.arange(G, dtype=torch.int32).reshape(G, 1) % 3
  out = run(torch.zeros(G, S, 3), {'warp': ids}, True, ('sigma', 'grad_sigma'))
  assert tuple(out['sigma'].shape) == (G, S) and tuple(out['grad_sigma'].shape) == (G, S, 3)
  assert [c['num_rays'] for c in rec.calls] == [2, 2, 2, 1] and all(c['S'] == S for c in rec.calls)
  g0 = 0
  for c in rec.calls:
    assert c['sigma'] == out['sigma'].data_ptr() + 4 * g0 * S and c['grad'] == out['grad_sigma'].data_ptr() + 12 * g0 * S
    assert c['normals'] is None and c['warped'] is None and c['warp_ids'] and c['flags'] == 0 and c['level'] == 1
    g0 += c['num_rays']
  assert g0 == G
  assert len({(c['ws'], c['nbytes']) for c in rec.calls}) == 1  # one cached workspace, sized for the largest piece
  n = C.c_size_t(0)                                            # ... by the library itself: two groups of 37 points
  assert lib.nrf_query_grad_workspace_bytes(model.handle, 2, S, 0, C.byref(n)) == 0 and rec.calls[0]['nbytes'] == H.ws_bytes(n.value)
  # leading dimensions are flattened into groups and restored
  rec.calls.clear()
  out = run(torch.zeros(2, 3, 5, 3), {'warp': ids[:6].reshape(2, 3, 1)}, True, ('normals',))
  assert tuple(out['normals'].shape) == (2, 3, 5, 3) and [(c['num_rays'], c['S']) for c in rec.calls] == [(6, 5)]
  # one long group is cut along its points
  rec.calls.clear()
  out = run(torch.zeros(250, 3), {}, False, ('normals',))
  assert tuple(out['normals'].shape) == (250, 3)
  assert [(c['num_rays'], c['S'], c['normals'] - out['normals'].data_ptr()) for c in rec.calls] == [(1, 100, 0), (1, 100, 1200), (1, 50, 2400)]
  assert all(c['flags'] == L.NRF_FLAG_NO_WARP and c['warp_ids'] is None for c in rec.calls)
  assert lib.nrf_query_grad_workspace_bytes(model.handle, 1, 100, L.NRF_FLAG_NO_WARP, C.byref(n)) == 0
  assert {c['nbytes'] for c in rec.calls} == {H.ws_bytes(n.value)}  # one group's first 100 points
  with pytest.raises(L.NrfError, match='outputs'):
    run(torch.zeros(4, 3), {}, False, ('rgb',))
