"""nrf_backward_ex on the host (no GPU): the ctypes mirrors of nrf_level_grads / nrf_output_grads against the compiled header, the
refusals that are decided before anything is enqueued, and the shape checks of NerfModel.backward(d_out=...) -- every cotangent
buffer is read by the kernels at its full size, so a wrong shape has to stop in Python."""
import ctypes as C
import os
import shutil
import subprocess
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'nerfies_amd.h')
NRF_E_NULL, NRF_E_STATE = -1, -6   # include/nerfies_amd.h


@pytest.fixture(scope='module')
def lib():
  from nerfies_amd import build, lib as L
  build.build()
  return L.load_library()


def _model(**kw):
  from nerfies_amd import models
  cfg = types.SimpleNamespace(num_coarse_samples=8, num_fine_samples=6, num_nerf_point_freqs=4, use_stratified_sampling=False, **kw)
  model, _ = models.construct_nerf(0, cfg, 4, [0], [0], [0, 1], 0.1, 1.0, device='cpu')
  return model


def test_mirrors_match_the_compiled_header(tmp_path):
  from nerfies_amd import lib as L
  cc = shutil.which('gcc') or shutil.which('cc')
  if cc is None:
    pytest.skip('no C compiler')
  pairs = [('nrf_level_grads', L.LevelGrads), ('nrf_output_grads', L.OutputGrads)]
  lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', 'int main(void) {']
  for cname, ct in pairs:
    lines.append(f'  printf("{cname} size %zu\\n", sizeof({cname}));')
    for fname, _ in ct._fields_:
      lines.append(f'  printf("{cname} {fname} %zu\\n", offsetof({cname}, {fname}));')
  lines += ['  printf("NRF_VERSION %d\\n", NRF_VERSION);', '  return 0;', '}']
  src = tmp_path / 'abi.c'
  src.write_text('\n'.join(lines))
  exe = tmp_path / 'abi'
  subprocess.run([cc, '-std=c99', '-Wall', '-Werror', str(src), '-o', str(exe)], check=True)
  got = {}
  for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines():
    *k, v = line.split()
    got[' '.join(k)] = int(v)
  for cname, ct in pairs:
    assert got[f'{cname} size'] == C.sizeof(ct)
    for fname, _ in ct._fields_:
      assert got[f'{cname} {fname}'] == getattr(ct, fname).offset, (cname, fname)
  assert [f for f, _ in L.LevelGrads._fields_] == ['d_rgb', 'd_depth', 'd_acc', 'd_weights', 'd_warped_points']
  assert got['NRF_VERSION'] >= 620 and got['NRF_VERSION'] == L.load_library().nrf_version()


def test_refusals_decided_on_the_host(lib):
  from nerfies_amd import lib as L
  model = _model()
  h = model.handle
  rays = L.Rays(num_rays=4)
  og = L.OutputGrads()
  buf = (C.c_float * 64)()   # stands in for params / grad / workspace: none of them is touched before the refusal
  p = C.cast(buf, C.c_void_p)
  assert lib.nrf_backward_ex(None, p, C.byref(rays), C.byref(og), p, p, 256, None) == NRF_E_NULL
  assert lib.nrf_backward_ex(h, p, C.byref(rays), None, p, p, 256, None) == NRF_E_NULL
  assert b'nrf_output_grads' in lib.nrf_last_error()
  assert lib.nrf_backward_ex(h, p, C.byref(rays), C.byref(og), None, p, 256, None) == NRF_E_NULL
  # no stashed forward on this workspace: the same answer as nrf_backward's
  assert lib.nrf_backward_ex(h, p, C.byref(rays), C.byref(og), p, p, 256, None) == NRF_E_STATE
  msg = lib.nrf_last_error()
  assert lib.nrf_backward(h, p, C.byref(rays), None, None, p, p, 256, None) == NRF_E_STATE
  assert lib.nrf_last_error() == msg and b'nrf_forward(NRF_FLAG_TRAIN)' in msg


def test_d_out_is_validated_before_the_library_reads_it():
  from nerfies_amd import lib as L
  model = _model()
  none = {'coarse': None, 'fine': None}
  og, keep = model._output_grads({'coarse': {'depth': torch.ones(4), 'weights': torch.ones(4, 8)}, 'fine': {'acc': torch.ones(4), 'rgb': None}},
                                 {'coarse': torch.ones(4, 3), 'fine': None}, 4, 'cpu')
  assert og.coarse.d_rgb and og.coarse.d_depth and og.coarse.d_weights and not og.coarse.d_acc and not og.coarse.d_warped_points
  assert og.fine.d_acc and not og.fine.d_rgb and not og.fine.d_weights and len(keep) == 4
  for bad in ({'coarse': {'weights': torch.ones(4, 14)}},          # the fine level's sample count
              {'fine': {'weights': torch.ones(4, 8)}},
              {'coarse': {'depth': torch.ones(4, 1)}},
              {'coarse': {'acc': torch.ones(5)}},
              {'fine': {'warped_points': torch.ones(4, 14)}},
              {'coarse': {'med_depth': torch.ones(4)}},            # piecewise constant: no cotangent
              {'coarse': {'warp_jacobian': torch.ones(4, 8, 3, 3)}},
              {'medium': {'rgb': torch.ones(4, 3)}}):
    with pytest.raises(L.NrfError):
      model._output_grads(bad, none, 4, 'cpu')
  with pytest.raises(L.NrfError, match='twice'):
    model._output_grads({'coarse': {'rgb': torch.ones(4, 3)}}, {'coarse': torch.ones(4, 3), 'fine': None}, 4, 'cpu')
  with pytest.raises(L.NrfError):   # a model without a fine level has no fine cotangents
    _model_single()._output_grads({'fine': {'acc': torch.ones(4)}}, none, 4, 'cpu')


def _model_single():
  from nerfies_amd import models
  cfg = types.SimpleNamespace(num_coarse_samples=8, num_fine_samples=0, num_nerf_point_freqs=4, use_stratified_sampling=False)
  return models.construct_nerf(0, cfg, 4, [0], [0], [0, 1], 0.1, 1.0, device='cpu')[0]


def test_autograd_wrapper_refuses_the_inference_only_mode():
  from nerfies_amd import autograd, lib as L
  for mode in ('x3', 'x3mlp'):
    with pytest.raises(L.NrfError, match='inference-only'):
      autograd.render_differentiable(_model(), torch.zeros(1), {}, bf16=mode)
