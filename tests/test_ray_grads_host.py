"""Gradients w.r.t. the rays on the host (no GPU): the ctypes mirror of nrf_ray_grads, NRF_FLAG_RAY_GRADS and nrf_backward_rays
against the compiled header, the refusals that are decided before anything is enqueued, the workspace sizes with and without the
flag, and the yardstick of tests/test_gpu_ray_grads.py itself -- torch.autograd over oracle.nerf_model_apply w.r.t. origins,
directions and viewdirs -- against float64 central differences."""
import ctypes as C
import os
import shutil
import subprocess
import types

import pytest
import torch

from oracle import nerfies_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'nerfies_amd.h')
NRF_E_NULL, NRF_E_UNSUPPORTED, NRF_E_STATE = -1, -3, -6   # include/nerfies_amd.h


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


def test_mirror_flag_and_export_match_the_compiled_header(tmp_path, lib):
  from nerfies_amd import lib as L
  cc = shutil.which('gcc') or shutil.which('cc')
  if cc is None:
    pytest.skip('no C compiler')
  lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', 'int main(void) {',
           '  printf("size %zu\\n", sizeof(nrf_ray_grads));']
  for fname, _ in L.RayGrads._fields_:
    lines.append(f'  printf("{fname} %zu\\n", offsetof(nrf_ray_grads, {fname}));')
  lines += ['  printf("NRF_FLAG_RAY_GRADS %u\\n", NRF_FLAG_RAY_GRADS);', '  printf("NRF_VERSION %d\\n", NRF_VERSION);',
            # the export's prototype, as the header declares it
            '  int (*f)(nrf_handle, const float*, const nrf_rays*, const nrf_output_grads*, const nrf_ray_grads*, float*, void*, size_t, void*)'
            ' = nrf_backward_rays;', '  printf("fn %d\\n", f != 0);', '  return 0;', '}',
            'int nrf_backward_rays(nrf_handle h, const float* p, const nrf_rays* r, const nrf_output_grads* g, const nrf_ray_grads* q,'
            ' float* o, void* w, size_t n, void* s) { (void)h; (void)p; (void)r; (void)g; (void)q; (void)o; (void)w; (void)n; (void)s; return 0; }']
  src = tmp_path / 'abi.c'
  src.write_text('\n'.join(lines))
  exe = tmp_path / 'abi'
  subprocess.run([cc, '-std=c99', '-Wall', '-Werror', str(src), '-o', str(exe)], check=True)
  got = {}
  for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines():
    k, v = line.split()
    got[k] = int(v)
  assert [f for f, _ in L.RayGrads._fields_] == ['d_origins', 'd_directions', 'd_viewdirs']
  assert got['size'] == C.sizeof(L.RayGrads) == 24
  for fname, _ in L.RayGrads._fields_:
    assert got[fname] == getattr(L.RayGrads, fname).offset, fname
  assert got['NRF_FLAG_RAY_GRADS'] == L.NRF_FLAG_RAY_GRADS == 64
  assert got['NRF_VERSION'] >= 630 and got['NRF_VERSION'] == lib.nrf_version()
  assert 'nrf_backward_rays' in L.EXPORTS and hasattr(lib, 'nrf_backward_rays')


def test_refusals_decided_on_the_host(lib):
  from nerfies_amd import lib as L
  model = _model()
  h = model.handle
  n = C.c_size_t(0)
  T, R = L.NRF_FLAG_TRAIN, L.NRF_FLAG_RAY_GRADS
  for flags in (R, T | R | L.NRF_FLAG_BF16, T | R | L.NRF_FLAG_BF16 | L.NRF_FLAG_WARP_F32, R | L.NRF_FLAG_BF16X3, T | R | L.NRF_FLAG_BF16X3):
    assert lib.nrf_workspace_bytes(h, 4, flags, C.byref(n)) == NRF_E_UNSUPPORTED, flags
    assert b'NRF_FLAG_RAY_GRADS' in lib.nrf_last_error(), flags
    assert lib.nrf_workspace_bytes_ex(h, 4, flags, 0, 0, C.byref(n)) == NRF_E_UNSUPPORTED, flags
  assert lib.nrf_workspace_bytes(h, 4, T | R, C.byref(n)) == 0 and n.value > 0
  rays = L.Rays(num_rays=4)
  og, rg = L.OutputGrads(), L.RayGrads()
  buf = (C.c_float * 64)()   # stands in for params / grad / workspace: none of them is touched before the refusal
  p = C.cast(buf, C.c_void_p)
  # nrf_forward refuses the same words before it looks at anything else
  assert lib.nrf_forward(h, p, C.byref(rays), None, None, None, R, p, 256, None) == NRF_E_UNSUPPORTED
  assert b'NRF_FLAG_RAY_GRADS' in lib.nrf_last_error()
  # the fused train step has no ray gradient
  assert lib.nrf_train_step_loss_grad_ex(h, p, C.byref(rays), p, None, None, None, None, None, R, p, p, p, 256, None) == NRF_E_UNSUPPORTED
  assert b'NRF_FLAG_RAY_GRADS' in lib.nrf_last_error()
  assert lib.nrf_backward_rays(h, p, C.byref(rays), C.byref(og), None, p, p, 256, None) == NRF_E_NULL
  assert b'nrf_ray_grads' in lib.nrf_last_error()
  assert lib.nrf_backward_rays(h, p, C.byref(rays), None, C.byref(rg), p, p, 256, None) == NRF_E_NULL
  assert lib.nrf_backward_rays(None, p, C.byref(rays), C.byref(og), C.byref(rg), p, p, 256, None) == NRF_E_NULL
  # nothing at all was stashed on this workspace: the message says which forward is missing.  (A stash kept by a forward WITHOUT the
  # flag needs a forward, hence a GPU: tests/test_gpu_ray_grads.py::test_parameter_gradient_is_nrf_backward_ex_and_calls_repeat_bit_for_bit)
  assert lib.nrf_backward_rays(h, p, C.byref(rays), C.byref(og), C.byref(rg), p, p, 256, None) == NRF_E_STATE
  assert b'NRF_FLAG_RAY_GRADS' in lib.nrf_last_error()


def test_chain_tile_rows_32_is_not_refused_and_plans_the_64_row_reverse_chain(lib):
  """NRF_OPT_CHAIN_TILE_ROWS = 32 on a model without a warp field: with the flag the plan is built (the option is followed in the
  forward only, as on a model with a warp field); it is the plan of the 64-row reverse chain plus the flag's buffers, so it is
  larger than the 64-row plan without the flag, and the plans without the flag are what they were."""
  from nerfies_amd import lib as L
  model = _model()
  T, R = L.NRF_FLAG_TRAIN, L.NRF_FLAG_RAY_GRADS
  size = {}
  for rows in (64, 32):
    assert lib.nrf_set_option(model.handle, L.NRF_OPT_CHAIN_TILE_ROWS, rows) == 0
    for flags in (T, T | R):
      n = C.c_size_t(0)
      assert lib.nrf_workspace_bytes(model.handle, 37, flags, C.byref(n)) == 0, (rows, flags, lib.nrf_last_error())
      size[rows, flags] = n.value
  assert size[32, T | R] == size[64, T | R] > size[64, T]   # the tiling changes no buffer of the 64-row reverse plan


# nrf_workspace_bytes of the commit before the flag existed, for _model() / _model(use_warp...) at 37 rays.  The sizes depend on the
# compute-unit count the handle plans for (per-workgroup partial buffers): these are for 256, what a handle assumes until it has
# seen a device and what the MI355X reports.  To regenerate: build the parent commit and print nrf_workspace_bytes(handle, 37, flags)
# for flags 0 and NRF_FLAG_TRAIN on both models.
PARENT_BYTES = {('nowarp', 0): 11866880, ('nowarp', 1): 82749696, ('warp', 0): 13105664, ('warp', 1): 94125568}


@pytest.mark.parametrize('kind', ['nowarp', 'warp'])
def test_workspace_sizes(lib, kind):
  """With the flag at least as large; without it exactly the parent's (tests/test_plan_digest.py's claim, restated for sizes)."""
  from nerfies_amd import lib as L
  model = _model(**({'use_warp': True, 'num_warp_freqs': 4, 'warp_field_type': 'se3'} if kind == 'warp' else {}))
  n, m = C.c_size_t(0), C.c_size_t(0)
  for train in (0, 1):
    assert lib.nrf_workspace_bytes(model.handle, 37, train * L.NRF_FLAG_TRAIN, C.byref(n)) == 0
    assert n.value == PARENT_BYTES[kind, train], (kind, train, n.value)
  assert lib.nrf_workspace_bytes(model.handle, 37, L.NRF_FLAG_TRAIN | L.NRF_FLAG_RAY_GRADS, C.byref(m)) == 0
  assert m.value > n.value   # the d-points buffers and W^T images / the Jacobians and the tangent stash
  assert lib.nrf_workspace_bytes(model.handle, 37, L.NRF_FLAG_TRAIN, C.byref(m)) == 0 and m.value == n.value   # ... and back


def _fd_case(use_warp):
  kw = dict(use_warp=True, warp_field_type='se3', num_warp_freqs=3) if use_warp else {}
  spec = O.ModelSpec(num_coarse_samples=6, num_fine_samples=6, nerf_trunk_width=16, nerf_rgb_branch_width=16, num_nerf_point_freqs=3,
                     num_nerf_viewdir_freqs=2, use_stratified_sampling=False, sigma_activation='softplus', use_white_background=True, **kw)
  params = O.init_params(spec, seed=3, trained_like=True, dtype=torch.float64)
  batch = O.synthetic_batch(2, seed=4, dtype=torch.float64)
  batch['viewdirs'] = batch['directions'].clone()
  batch['directions'] = batch['directions'] * 1.7   # non-unit: the compositing distances carry |d|
  return spec, params, batch


@pytest.mark.parametrize('use_warp', [False, True])
def test_oracle_ray_gradients_match_central_differences(use_warp):
  """The yardstick of the GPU test: d loss / d (origins, directions, viewdirs) by torch.autograd over the oracle, with the fine depths
  fixed (they sit behind stop_gradient), against float64 central differences -- 1e-6 of each tensor's max-abs."""
  spec, params, batch = _fd_case(use_warp)
  alpha = 2.5 if use_warp else 0.0
  with torch.no_grad():
    z_fine = O.nerf_model_apply(params, spec, batch, warp_alpha=alpha)['fine']['z_vals'].clone()
  g = torch.Generator().manual_seed(5)
  keys = ('rgb', 'depth', 'acc', 'weights') + (('warped_points',) if use_warp else ())

  def loss_of(rays):
    out = O.nerf_model_apply(params, spec, dict(batch, **rays), warp_alpha=alpha, fixed_fine_z=z_fine, return_points=use_warp)
    if not hasattr(loss_of, 'cot'):
      loss_of.cot = {lv: {k: torch.randn(out[lv][k].shape, generator=g, dtype=torch.float64) for k in keys} for lv in ('coarse', 'fine')}
    return sum((out[lv][k] * t).sum() for lv, d in loss_of.cot.items() for k, t in d.items())

  names = ('origins', 'directions', 'viewdirs')
  req = {k: batch[k].clone().requires_grad_(True) for k in names}
  grads = dict(zip(names, torch.autograd.grad(loss_of(req), [req[k] for k in names])))
  eps = 1e-6
  for k in names:
    fd = torch.zeros_like(batch[k])
    for i in range(batch[k].numel()):
      e = torch.zeros_like(batch[k]).reshape(-1)
      e[i] = eps
      e = e.reshape(batch[k].shape)
      with torch.no_grad():
        fd.reshape(-1)[i] = (loss_of({k: batch[k] + e}) - loss_of({k: batch[k] - e})) / (2 * eps)
    scale = grads[k].abs().max().item()
    assert scale > 0, k
    err = (fd - grads[k]).abs().max().item() / scale
    print(f'[warp={use_warp}] {k}: max-abs {scale:.3e}, central-difference error {err:.2e}')
    assert err < 1e-6, (k, err)
