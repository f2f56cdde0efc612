"""The workspace planner (csrc/nrf_plan.hip) against tests/golden/plan_digests.json: every configuration of
tests/golden/make_plan_digests.py plans the same sub-buffer offsets, descriptor tables and stream-K cuts (nrf_debug_plan_digest)
and the same workspace size as when the record was taken, or is refused as then.  Host only: planning needs no GPU.

The plan depends on the CU count -- the per-workgroup bias partials and the stream-K cut of both wgrad kernels are sized by
it.  The record assumes 256: the handle's default when no device is visible, and the MI355X's count."""
import ctypes as C
import importlib.util
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def _maker():
  spec = importlib.util.spec_from_file_location('make_plan_digests', os.path.join(GOLDEN, 'make_plan_digests.py'))
  mod = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(mod)
  return mod


@pytest.fixture(scope='module')
def lib():
  from nerfies_amd import build, lib as L
  build.build()          # hipcc cross-compiles gfx950 without a GPU; no-op when up to date
  return L.load_library()


def test_digest_needs_a_plan(lib):
  h = C.c_void_p()
  d = _maker().desc()
  assert lib.nrf_create(C.byref(d), C.byref(h)) == 0
  dg = C.c_uint64(0)
  assert lib.nrf_debug_plan_digest(h, C.byref(dg)) == -6   # NRF_E_STATE
  n = C.c_size_t(0)
  assert lib.nrf_workspace_bytes(h, 1024, 0, C.byref(n)) == 0
  assert lib.nrf_debug_plan_digest(h, C.byref(dg)) == 0 and dg.value != 0
  assert lib.nrf_destroy(h) == 0


def test_plans_match_the_record(lib):
  with open(os.path.join(GOLDEN, 'plan_digests.json')) as fp:
    rec = json.load(fp)
  assert rec['num_cus'] == 256
  got = _maker().plans(lib)
  assert sorted(got) == sorted(rec['plans'])
  changed = [k for k in sorted(got) if got[k] != rec['plans'][k]]
  assert not changed, f'{len(changed)} of {len(got)} plans changed, e.g. ' + ', '.join(changed[:6])
