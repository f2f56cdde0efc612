"""The inverse warp on the host (no GPU): nrf_unwarp_out and the three macros against the compiled header, every refusal
nrf_unwarp_points decides before any HIP call (one assertion per rule: the code, and the entry and the rule in nrf_last_error), the
workspace size, the other plans behind an unwarp plan, the chunking of NerfModel.unwarp_points and the --animate argument rules of
scripts/export_density.py."""
import ctypes as C
import importlib.util
import json
import math
import os
import shutil
import subprocess
import sys

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
  mk = _maker()
  hs = {}
  for name in ('A', 'se3_vrig', 'time_warp', 'translation', 'warp_trunk4x64'):
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
  cname, ct = 'nrf_unwarp_out', L.UnwarpOut
  lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', 'int main(void) {',
           f'  printf("size %zu\\n", sizeof({cname}));']
  for fname, _ in ct._fields_:
    lines.append(f'  printf("{fname} %zu\\n", offsetof({cname}, {fname}));')
  for macro in ('NRF_HAS_UNWARP', 'NRF_UNWARP_MAX_POINTS', 'NRF_UNWARP_MAX_STEPS', 'NRF_VERSION'):
    lines.append(f'  printf("{macro} %d\\n", {macro});')
  lines += ['  return 0;', '}']
  src = tmp_path / 'abi.c'
  src.write_text('\n'.join(lines))
  exe = tmp_path / 'abi'
  subprocess.run([cc, '-std=c99', '-Wall', '-Werror', str(src), '-o', str(exe)], check=True)
  got = {}
  for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines():
    k, v = line.split()
    got[k] = int(v)
  assert [f for f, _ in ct._fields_] == ['points', 'residual', 'status']
  assert got['size'] == C.sizeof(ct) == 24
  for fname, _ in ct._fields_:
    assert got[fname] == getattr(ct, fname).offset, fname
  assert got['NRF_HAS_UNWARP'] == L.NRF_HAS_UNWARP == 1
  assert got['NRF_UNWARP_MAX_POINTS'] == L.NRF_UNWARP_MAX_POINTS == 1 << 20
  assert got['NRF_UNWARP_MAX_STEPS'] == L.NRF_UNWARP_MAX_STEPS == 32
  assert got['NRF_VERSION'] == 660 == lib.nrf_version() == L.NRF_VERSION
  for name in ('nrf_unwarp_workspace_bytes', 'nrf_unwarp_points'):
    assert name in L.EXPORTS and hasattr(lib, name), name


class _Call:
  """nrf_unwarp_points with stand-in buffers: nothing is touched before a refusal."""

  def __init__(self, lib, h):
    from nerfies_amd import lib as L
    self.L, self.lib, self.h = L, lib, h
    self.buf = (C.c_float * 64)()
    self.p = C.cast(self.buf, C.c_void_p)
    self.sc = L.StepScalars()

  def __call__(self, h='h', params='p', targets='p', ids='p', codes=None, num_codes=0, guess=None, n=5, scalars='sc', steps=8, tolerance=0.0,
               max_step=math.inf, out=None, ws='p', nbytes=1 << 40):
    L = self.L
    o = out if out is not None else L.UnwarpOut(points=self.p, residual=self.p, status=self.p)
    pick = lambda v: self.p if v == 'p' else v
    return self.lib.nrf_unwarp_points(self.h if h == 'h' else h, pick(params), pick(targets), pick(ids), pick(codes), num_codes, pick(guess), n,
                                      C.byref(self.sc) if scalars == 'sc' else scalars, steps, tolerance, max_step,
                                      None if o is False else C.byref(o), pick(ws), nbytes, None)

  def refused(self, code, *words, **kw):
    """the call is refused with `code`, and nrf_last_error names the entry and every one of `words`"""
    rc = self(**kw)
    err = self.lib.nrf_last_error()
    assert rc == code, (kw, rc, err)
    for w in (b'nrf_unwarp_points',) + words:
      assert w in err, (kw, w, err)
    return True


def test_null_arguments(lib, handles):
  c = _Call(lib, handles['se3_vrig'])
  assert c.refused(NRF_E_NULL, b'handle', h=None)
  assert c.refused(NRF_E_NULL, b'params', params=None)
  assert c.refused(NRF_E_NULL, b'targets', targets=None)
  assert c.refused(NRF_E_NULL, b'warp_ids', ids=None)
  assert c.refused(NRF_E_NULL, b'warp_ids', ids=None, codes='p', num_codes=3)   # the ids index the code table's rows: still needed
  assert c.refused(NRF_E_NULL, b'scalars', scalars=None)
  assert c.refused(NRF_E_NULL, b'nrf_unwarp_out', out=False)
  assert c.refused(NRF_E_NULL, b'workspace', ws=None)
  # what may be NULL: the guess, the codes, any of the outputs -- the call gets as far as the workspace rule
  assert c.refused(NRF_E_WORKSPACE, guess=None, codes=None, out=c.L.UnwarpOut(), nbytes=0)
  assert c.refused(NRF_E_WORKSPACE, guess='p', codes='p', num_codes=2, nbytes=0)
  n = C.c_size_t(0)
  assert lib.nrf_unwarp_workspace_bytes(None, 1, C.byref(n)) == NRF_E_NULL and b'nrf_unwarp_workspace_bytes' in lib.nrf_last_error()
  assert lib.nrf_unwarp_workspace_bytes(handles['se3_vrig'], 1, None) == NRF_E_NULL and b'bytes' in lib.nrf_last_error()


def test_model_rules(lib, handles):
  assert _Call(lib, handles['A']).refused(NRF_E_UNSUPPORTED, b'no warp field')
  assert _Call(lib, handles['time_warp']).refused(NRF_E_UNSUPPORTED, b'time encoder')
  n = C.c_size_t(0)
  assert lib.nrf_unwarp_workspace_bytes(handles['A'], 5, C.byref(n)) == NRF_E_UNSUPPORTED and b'no warp field' in lib.nrf_last_error()
  assert lib.nrf_unwarp_workspace_bytes(handles['time_warp'], 5, C.byref(n)) == NRF_E_UNSUPPORTED and b'time encoder' in lib.nrf_last_error()
  for name in ('se3_vrig', 'translation', 'warp_trunk4x64'):   # every other warp model runs: the call gets as far as the workspace rule
    assert _Call(lib, handles[name]).refused(NRF_E_WORKSPACE, nbytes=0), name


def test_shape_rules(lib, handles):
  c = _Call(lib, handles['se3_vrig'])
  for n in (0, -1, (1 << 20) + 1):
    assert c.refused(NRF_E_SHAPE, b'num_points', b'NRF_UNWARP_MAX_POINTS', n=n)
  assert c.refused(NRF_E_WORKSPACE, n=1 << 20, nbytes=0) and c.refused(NRF_E_WORKSPACE, n=1, nbytes=0)
  for k in (-1, 33):
    assert c.refused(NRF_E_SHAPE, b'num_steps', b'NRF_UNWARP_MAX_STEPS', steps=k)
  assert c.refused(NRF_E_WORKSPACE, steps=0, nbytes=0) and c.refused(NRF_E_WORKSPACE, steps=32, nbytes=0)
  for t in (-1e-9, -math.inf, math.nan):
    assert c.refused(NRF_E_SHAPE, b'tolerance', tolerance=t)
  assert c.refused(NRF_E_WORKSPACE, tolerance=0.0, nbytes=0) and c.refused(NRF_E_WORKSPACE, tolerance=math.inf, nbytes=0)
  for m in (0.0, -0.5, math.nan):
    assert c.refused(NRF_E_SHAPE, b'max_step', max_step=m)
  assert c.refused(NRF_E_WORKSPACE, max_step=1e-30, nbytes=0) and c.refused(NRF_E_WORKSPACE, max_step=math.inf, nbytes=0)
  for k in (0, -2):
    assert c.refused(NRF_E_SHAPE, b'num_codes', codes='p', num_codes=k)
  assert c.refused(NRF_E_WORKSPACE, codes=None, num_codes=-2, nbytes=0)   # without codes the count is not read
  n = C.c_size_t(0)
  for bad in (0, -1, (1 << 20) + 1):
    assert lib.nrf_unwarp_workspace_bytes(handles['se3_vrig'], bad, C.byref(n)) == NRF_E_SHAPE and b'NRF_UNWARP_MAX_POINTS' in lib.nrf_last_error()


def test_workspace_size(lib, handles):
  mk = _maker()
  for name in ('se3_vrig', 'translation', 'warp_trunk4x64'):
    h = handles[name]
    size = {}
    for pts in (1, 63, 64, 65, 70, 128, 1 << 12, 1 << 20):
      n = C.c_size_t(0)
      assert lib.nrf_unwarp_workspace_bytes(h, pts, C.byref(n)) == 0, lib.nrf_last_error()   # no GPU on this machine's side of the suite
      size[pts] = n.value
    order = sorted(size)
    assert all(size[a] <= size[b] for a, b in zip(order, order[1:])), (name, size)
    assert size[1] == size[63] == size[64] < size[65] == size[70] == size[128]                   # whole 64-row tiles
    # Bytes per added row, from the carve (nrf_field.hip UnwarpPlan): x 12, trunk input 4 PKSw (PKSw = 3 + 6 F + G rounded up to 32:
    # 32..96), sign words 6 x 256 words per 64-row tile = 96, (w, v) 32, tangent (dw, dv) 96, warped 12, state 4
    F, G = mk.MODELS[name].get('num_warp_freqs', 8), mk.MODELS[name].get('num_warp_features', 8)
    pks = (3 + 6 * F + G + 31) // 32 * 32
    per_row = (size[1 << 20] - size[1 << 12]) / ((1 << 20) - (1 << 12))
    assert per_row == 12 + 4 * pks + 96 + 32 + 96 + 12 + 4, (name, per_row, pks)
    assert per_row <= 640                                                                       # "~0.5 KB per row"
    g = C.c_size_t(0)
    assert lib.nrf_query_grad_workspace_bytes(h, 1, 1 << 12, 0, C.byref(g)) == 0 and size[1 << 12] < g.value   # no NeRF chain, no Jacobian
    c = _Call(lib, h)
    assert c.refused(NRF_E_WORKSPACE, b'nrf_unwarp_workspace_bytes', n=70, nbytes=size[70] - 1)
    assert c.refused(NRF_E_WORKSPACE, b'nrf_unwarp_workspace_bytes', n=65, nbytes=size[64])


def test_other_plans_stay_behind_an_unwarp_plan(lib, handles):
  """A value-query, gradient-query or ray plan made before an unwarp plan keeps its size and its digest."""
  with open(os.path.join(GOLDEN, 'plan_digests.json')) as fp:
    rec = json.load(fp)['plans']
  h = handles['se3_vrig']
  for rays in (37, 128):
    want = rec[f'se3_vrig/0/rays={rays}/bg=0/elastic=0/rows=0/merge=1']
    n, q0, q1, g0, g1, u = (C.c_size_t(0) for _ in range(6))
    dg = C.c_uint64(0)
    assert lib.nrf_query_workspace_bytes(h, rays, 64, 0, C.byref(q0)) == 0
    assert lib.nrf_query_grad_workspace_bytes(h, rays, 64, 0, C.byref(g0)) == 0
    assert lib.nrf_workspace_bytes_ex(h, rays, 0, 0, 0, C.byref(n)) == 0 and n.value == want['workspace_bytes']
    assert lib.nrf_debug_plan_digest(h, C.byref(dg)) == 0 and '%016x' % dg.value == want['digest'], rays
    assert lib.nrf_unwarp_workspace_bytes(h, rays * 64, C.byref(u)) == 0 and u.value > 0
    assert _Call(lib, h).refused(NRF_E_WORKSPACE, n=rays * 64, nbytes=0)
    assert lib.nrf_debug_plan_digest(h, C.byref(dg)) == 0 and '%016x' % dg.value == want['digest'], rays
    assert lib.nrf_query_workspace_bytes(h, rays, 64, 0, C.byref(q1)) == 0 and q1.value == q0.value
    assert lib.nrf_query_grad_workspace_bytes(h, rays, 64, 0, C.byref(g1)) == 0 and g1.value == g0.value
  spec = importlib.util.spec_from_file_location('make_side_plan_sizes', os.path.join(GOLDEN, 'make_side_plan_sizes.py'))
  mod = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(mod)
  with open(os.path.join(GOLDEN, 'side_plan_sizes.json')) as fp:
    assert mod.sizes(lib) == json.load(fp)['sizes']


def test_unwarp_chunks_cover_the_points_once(lib, monkeypatch):
  """NerfModel.unwarp_points behind its device rule (CPU points raise before anything else): the recorder never follows a pointer, so
  the chunking runs on CPU tensors."""
  import torch
  from nerfies_amd import lib as L
  rec = H.RecordingLib(lib, ['nrf_unwarp_points'])
  model, fp = H.cpu_field_model(rec)
  with pytest.raises(L.NrfError, match='GPU'):
    model.unwarp_points(fp, torch.zeros(4, 3), torch.zeros(4, dtype=torch.int32), {'alpha': 1.0})
  assert rec.calls == []
  monkeypatch.setattr(L, 'NRF_UNWARP_MAX_POINTS', 100)        # the Python side's chunk size; the library's own cap is tested above
  H.lift_device_rule(monkeypatch)
  run = lambda pts, ids, guess=None, codes=None, outputs=('points', 'residual', 'status'), **kw: model.unwarp_points(
      fp, pts, ids, {'alpha': 2.5}, guess=guess, warp_codes=codes, outputs=outputs, **kw)
  n = 250                                                      # 100 + 100 + 50
  pts, ids, guess = torch.zeros(n, 3), torch.arange(n, dtype=torch.int32) % 3, torch.ones(n, 3)
  out = run(pts, ids, guess, steps=5, tolerance=1e-6, max_step=0.5)
  assert tuple(out['points'].shape) == (n, 3) and out['points'].dtype == torch.float32
  assert tuple(out['residual'].shape) == (n,) and out['residual'].dtype == torch.float32
  assert tuple(out['status'].shape) == (n,) and out['status'].dtype == torch.int32
  assert [c['n'] for c in rec.calls] == [100, 100, 50]
  seen, r0 = torch.zeros(n, dtype=torch.int32), 0
  for c in rec.calls:
    seen[r0:r0 + c['n']] += 1
    assert c['points'] == out['points'].data_ptr() + 12 * r0 and c['residual'] == out['residual'].data_ptr() + 4 * r0
    assert c['status'] == out['status'].data_ptr() + 4 * r0
    assert c['steps'] == 5 and c['tolerance'] == pytest.approx(1e-6) and c['max_step'] == 0.5 and c['alpha'] == 2.5
    assert c['codes'] is None and c['num_codes'] == 0 and c['guess'] is not None and c['targets'] is not None and c['ids'] is not None
    r0 += c['n']
  assert bool((seen == 1).all())
  # targets, ids and guess advance together, 12 / 4 / 12 bytes per row
  for key, per in (('targets', 12), ('ids', 4), ('guess', 12)):
    assert [c[key] - rec.calls[0][key] for c in rec.calls] == [0, 100 * per, 200 * per], key
  assert len({(c['ws'], c['nbytes']) for c in rec.calls}) == 1   # one cached workspace, sized for the largest chunk
  nb = C.c_size_t(0)                                             # ... by the library itself: 100 points
  assert lib.nrf_unwarp_workspace_bytes(model.handle, 100, C.byref(nb)) == 0 and rec.calls[0]['nbytes'] == H.ws_bytes(nb.value)
  # leading dimensions are kept; no guess, a code table, a selection of the outputs
  rec.calls.clear()
  codes = torch.zeros(7, model.num_warp_features)
  out = run(torch.zeros(2, 3, 5, 3), torch.zeros(2, 3, 5, 1, dtype=torch.int64), codes=codes, outputs=('residual',))
  assert set(out) == {'residual'} and tuple(out['residual'].shape) == (2, 3, 5)
  (c,) = rec.calls
  assert c['n'] == 30 and c['guess'] is None and c['codes'] == codes.data_ptr() and c['num_codes'] == 7
  assert c['points'] is None and c['status'] is None and c['max_step'] == math.inf and c['tolerance'] == 0.0
  with pytest.raises(L.NrfError, match='outputs'):
    run(pts, ids, outputs=('jacobian',))
  with pytest.raises(L.NrfError, match='one id per point'):
    run(pts, ids[:7])
  with pytest.raises(L.NrfError, match='guess'):
    run(pts, ids, guess[:7])
  with pytest.raises(L.NrfError, match=r'\(\.\.\., 3\)'):
    run(torch.zeros(5, 2), ids[:5])


def test_animate_argument_errors(capsys):
  sys.path.insert(0, ROOT)
  sys.path.insert(0, os.path.join(ROOT, 'scripts'))
  import export_density
  base = ['--base_folder', 'x', '--data_dir', 'y']
  for argv in (['--canonical', '--animate', '000001'],                       # no --mesh
               ['--mesh', '--frame', '000002', '--animate', '000001'],       # a frame's mesh, not the template's
               ['--mesh', '--canonical', '--animate']):                      # no item id
    with pytest.raises(SystemExit) as e:
      export_density.parse_flags(base + argv)
    assert e.value.code == 2, argv
    assert '--animate' in capsys.readouterr().err, argv
  ok = export_density.parse_flags(base + ['--mesh', '--canonical', '--animate', '000001', '000003', '--animate_steps', '4'])
  assert ok.animate == ['000001', '000003'] and ok.animate_steps == 4 and ok.mesh and ok.canonical
  assert export_density.parse_flags(base + ['--mesh', '--canonical']).animate is None
