"""nerfies_amd/csrc/se3_math.h itself, compiled unchanged for the host, against a float64 reference across rotation angles.

The header's closed forms sit on the forward and reverse pass of every warp kernel and of the camera-refinement kernels.  Here it
is compiled by the host C++ compiler behind a stand-in for <hip/hip_runtime.h> (which defines __device__ / __forceinline__ away)
and called through ctypes on float arrays: each coefficient over 4096 log-spaced t2 = |w|^2 in [1e-14, 400], t2 = 0, and the 16
float32 neighbours on each side of 0.04 (the switch of the first version of the header), of pi^2, of 4 pi^2 and of every switch
the header has now; then se3_apply, se3_vjp and the Dual Jacobian column / Hessian-vector products over the same sweep.

Gates (tests/se3_reference.py has the reference, the envelope and the floor):
  * a coefficient's error is counted in float32 ulps of max(|exact|, envelope);
  * below the header's lowest switch (everything is a series in t2): 8 ulps;
  * above it: the rounding of the exact value to float32 plus 64 ulps for A, B, C, Ab and plus 256 ulps for Bb, Cb, dAb, dBb, dCb
    (operation order, not digit loss: a coefficient with no correct digit is ~1e7 ulps);
  * vector level: the error of each quantity relative to its max-abs over the sweep bucket is at most 4 x F, F being the same figure
    for a float32 torch evaluation with exact coefficients.
The host's sincosf differs from the device's by an ulp or so, far below what these gates look for."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from oracle import nerfies_oracle as O

import se3_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'nerfies_amd', 'csrc')

STANDIN = '''#pragma once
#define __device__
#define __host__
#define __forceinline__ inline
#include <math.h>
'''

WRAPPER = r'''
#include "se3_math.h"
using namespace nrf;
static V3 ld(const float* p, int i) { return v3(p[3 * i], p[3 * i + 1], p[3 * i + 2]); }
static void st(float* p, int i, V3 a) { p[3 * i] = a.x; p[3 * i + 1] = a.y; p[3 * i + 2] = a.z; }
static V3T<Dual> ldd(const float* p, const float* d, int i) {
  return v3t<Dual>(Dual(p[3 * i], d[3 * i]), Dual(p[3 * i + 1], d[3 * i + 1]), Dual(p[3 * i + 2], d[3 * i + 2]));
}
extern "C" {
#ifdef SE3_NAMED_SWITCHES
int h_se3_switches(float* out) { out[0] = SE3_SERIES_T2; out[1] = SE3_SERIES_DCB_T2; return 2; }   // what the compiled code branches on
#endif
void h_se3_coef(int n, const float* t2, float* out) {          // n x 6: A B C Ab Bb Cb
  for (int i = 0; i < n; ++i) {
    const Se3Coef<float> c = se3_coef<float>(t2[i]);
    float* o = out + 6 * i;
    o[0] = c.A; o[1] = c.B; o[2] = c.C; o[3] = c.Ab; o[4] = c.Bb; o[5] = c.Cb;
  }
}
void h_se3_coef_d(int n, const float* t2, float* out) {        // n x 9: A B C Ab Bb Cb dAb dBb dCb
  for (int i = 0; i < n; ++i) {
    const Se3CoefD k = se3_coef_d(t2[i]);
    float* o = out + 9 * i;
    o[0] = k.c.A; o[1] = k.c.B; o[2] = k.c.C; o[3] = k.c.Ab; o[4] = k.c.Bb; o[5] = k.c.Cb; o[6] = k.dAb; o[7] = k.dBb; o[8] = k.dCb;
  }
}
void h_se3_apply(int n, const float* w, const float* v, const float* x, float* out) {
  for (int i = 0; i < n; ++i) st(out, i, se3_apply(ld(w, i), ld(v, i), ld(x, i)));
}
void h_se3_vjp(int n, const float* w, const float* v, const float* x, const float* g, float* dw, float* dv) {
  for (int i = 0; i < n; ++i) {
    V3 a, b;
    se3_vjp<float>(ld(w, i), ld(v, i), ld(x, i), ld(g, i), a, b);
    st(dw, i, a); st(dv, i, b);
  }
}
// the Dual evaluation of warp_chain.hip's elastic / Jacobian kernels along ONE direction (wd, vd, xd): the tangent of se3_delta (a
// column of J - I) and the tangents of the VJP (the Hessian-vector products), coefficients from se3_coef_d + se3_coef_along
void h_se3_dual(int n, const float* w, const float* v, const float* x, const float* g, const float* wd, const float* vd, const float* xd,
                float* jcol, float* hdw, float* hdv) {
  for (int i = 0; i < n; ++i) {
    const V3 wi = ld(w, i), wdi = ld(wd, i);
    const Se3CoefD kc = se3_coef_d(dot(wi, wi));
    const Se3Coef<Dual> k = se3_coef_along(kc, 2.f * dot(wi, wdi));
    const V3T<Dual> W = ldd(w, wd, i), Vv = ldd(v, vd, i), X = ldd(x, xd, i);
    const V3T<Dual> dl = se3_delta_c<Dual>(k, W, Vv, X);
    st(jcol, i, v3(dl.x.d, dl.y.d, dl.z.d));
    const V3 gi = ld(g, i);
    V3T<Dual> a, b;
    se3_vjp_c<Dual>(k, W, Vv, X, v3t<Dual>(Dual(gi.x), Dual(gi.y), Dual(gi.z)), a, b);
    st(hdw, i, v3(a.x.d, a.y.d, a.z.d)); st(hdv, i, v3(b.x.d, b.y.d, b.z.d));
  }
}
}
'''


def build_host(tmp, csrc=CSRC):
  """The header at `csrc`, compiled for the host into a shared object; a ctypes handle."""
  cxx = shutil.which('g++') or shutil.which('c++') or shutil.which('clang++')
  if cxx is None:
    pytest.skip('no host C++ compiler')
  os.makedirs(os.path.join(tmp, 'hip'), exist_ok=True)
  with open(os.path.join(tmp, 'hip', 'hip_runtime.h'), 'w') as f:
    f.write(STANDIN)
  src, so = os.path.join(tmp, 'se3_host.cpp'), os.path.join(tmp, 'se3_host.so')
  with open(src, 'w') as f:
    f.write(WRAPPER)
  named = ['-DSE3_NAMED_SWITCHES'] if 'SE3_SERIES_DCB_T2' in open(os.path.join(csrc, 'se3_math.h')).read() else []
  subprocess.run([cxx, '-std=c++17', '-O2', '-shared', '-fPIC', *named, '-I', str(tmp), '-I', csrc, src, '-o', so], check=True)
  return C.CDLL(so)


@pytest.fixture(scope='module')
def host(tmp_path_factory):
  return build_host(str(tmp_path_factory.mktemp('se3_host')))


def _p(a):
  return a.ctypes.data_as(C.POINTER(C.c_float))


def _f32(a):
  return np.ascontiguousarray(a, np.float32)


def header_switches(path=os.path.join(CSRC, 'se3_math.h')):
  """Every t2 threshold the header's text compares with: `t2 < 0.04f`, `val(t2) < NAME` with `constexpr float NAME = 4.f;`.  The sweep
  is laid out from these before anything is compiled; test_switches_read_from_the_source_are_the_compiled_ones holds them to the
  constants of the compiled object, so a rewritten condition cannot move the series gate unnoticed."""
  src = re.sub(r'//.*', '', open(path).read())
  named = {k: float(v) for k, v in re.findall(r'constexpr\s+float\s+(\w+)\s*=\s*([0-9.eE+-]+)f\s*;', src)}
  found = re.findall(r't2\)?\s*<\s*([A-Za-z_]\w*|[0-9.eE+-]+f)', src)
  return sorted({named[m] if m in named else float(m[:-1]) for m in found})


def neighbours(x, n=16):
  x = np.float32(x)
  lo, hi = [x], [x]
  for _ in range(n):
    lo.append(np.nextafter(lo[-1], np.float32(-np.inf)))
    hi.append(np.nextafter(hi[-1], np.float32(np.inf)))
  return np.array(lo[::-1] + hi[1:], np.float32)


def sweep_t2():
  parts = [np.logspace(-14, np.log10(400.0), 4096).astype(np.float32), np.zeros(1, np.float32)]
  for x in [0.04, np.pi ** 2, 4 * np.pi ** 2] + header_switches():
    parts.append(neighbours(x))
  return np.unique(np.concatenate(parts))


EDGES = (0.0, 1e-8, 1e-4, 0.01, 0.0256, 0.04, 0.0625, 0.25, 1.0, 4.0, 9.0, 39.0, 401.0)


def _bucket_rows(t2):
  for lo, hi in zip(EDGES[:-1], EDGES[1:]):
    m = (t2 >= np.float32(lo)) & (t2 < np.float32(hi))
    if m.any():
      yield f'[{lo:g}, {hi:g})', m


def test_reference_series_and_closed_forms_agree():
  """The two halves of the reference, each on the other's ground.  In plain float64, 1e-12 relative on [3, 6], around t2 = 4 where
  coef_ref hands over from the series to the closed forms (the series is still converged at 6, the closed forms' numerators have lost
  three digits at 3).  And 1e-12 on [0.5, 2]: there the numerator of dCb is 3e-5 of its largest term, which costs float64 1e-11, so
  on that interval the closed forms are evaluated in extended precision (x87 long double) -- coef_ref never uses them there."""
  t2 = np.linspace(3.0, 6.0, 301)
  a, b = R.coef_series(t2), R.coef_closed(t2)
  rel = np.abs(a - b) / np.maximum(np.abs(a), R.envelope(t2))
  print('series vs closed forms on [3, 6], float64, max relative difference:', dict(zip(R.NAMES, rel.max(1))))
  assert rel.max() <= 1e-12, dict(zip(R.NAMES, rel.max(1)))
  t2 = np.linspace(0.5, 2.0, 301)
  a, b = R.coef_series(t2), R.coef_closed(t2, np.longdouble).astype(np.float64)
  rel = np.abs(a - b) / np.abs(a)
  print('series vs closed forms on [0.5, 2], max relative difference:', dict(zip(R.NAMES, rel.max(1))))
  assert rel.max() <= 1e-12, dict(zip(R.NAMES, rel.max(1)))


def test_reference_algebra_matches_oracle_autograd():
  """se3_reference's algebra in float64 (what everything below is compared with) against torch autograd of the oracle's exp_se3, at
  angles where the oracle's normalised-axis form is well conditioned."""
  g = torch.Generator().manual_seed(5)
  n = 64
  th = torch.logspace(-1.3, 0.85, n, dtype=torch.float64)
  w = torch.nn.functional.normalize(torch.randn(n, 3, generator=g, dtype=torch.float64), dim=-1) * th[:, None]
  v, x, gg, wd, vd, xd = (torch.randn(n, 3, generator=g, dtype=torch.float64) for _ in range(6))

  def warp(w, v, x):
    theta = torch.linalg.norm(w, dim=-1)
    T = O.exp_se3(torch.cat([w, v], -1) / theta[:, None], theta)
    return O.from_homogenous((T @ O.to_homogenous(x)[..., None])[..., 0])

  def grads(w, v, x):
    return torch.autograd.grad((warp(w, v, x) * gg).sum(), (w, v), create_graph=True)
  w_, v_ = w.clone().requires_grad_(), v.clone().requires_grad_()
  ref = {'delta': warp(w, v, x) - x}
  ref['dw'], ref['dv'] = (t.detach() for t in grads(w_, v_, x))
  ref['jcol'] = torch.autograd.functional.jvp(warp, (w, v, x), (wd, vd, xd))[1] - xd
  ref['hdw'], ref['hdv'] = torch.autograd.functional.jvp(grads, (w, v, x), (wd, vd, xd))[1]
  got = R.eval_all(w, v, x, gg, wd, vd, xd, torch.float64)
  for k, r in ref.items():
    err = (got[k] - r).abs().max().item() / r.abs().max().item()
    assert err < 1e-10, (k, err)


def test_switches_read_from_the_source_are_the_compiled_ones(host):
  out = np.zeros(4, np.float32)
  n = host.h_se3_switches(_p(out))
  assert sorted(out[:n].tolist()) == header_switches()


def coefficient_errors(host, t2):
  """(9, n) error of se3_coef_d in float32 ulps of max(|exact|, envelope), the same for the exact value rounded to float32, and the
  (6, n) error of se3_coef (which must return what se3_coef_d does)."""
  n = t2.size
  out9, out6 = np.empty((n, 9), np.float32), np.empty((n, 6), np.float32)
  host.h_se3_coef_d(n, _p(t2), _p(out9))
  host.h_se3_coef(n, _p(t2), _p(out6))
  exact = R.coef_ref(t2.astype(np.float64))
  unit = R.ulp32(np.maximum(np.abs(exact), R.envelope(t2.astype(np.float64))))
  err = np.abs(out9.T.astype(np.float64) - exact) / unit
  rounded = np.abs(exact.astype(np.float32).astype(np.float64) - exact) / unit
  return err, rounded, out9, out6


def print_table(title, t2, err):
  print('\n' + title)
  print('| t2 | ' + ' | '.join(R.NAMES) + ' |')
  print('|---|' + '---|' * len(R.NAMES))
  for label, m in _bucket_rows(t2):
    print(f'| {label} | ' + ' | '.join(f'{err[i, m].max():.3g}' for i in range(len(R.NAMES))) + ' |')


def test_coefficient_sweep(host):
  t2 = sweep_t2()
  sw = header_switches()
  assert sw, 'no t2 threshold found in se3_math.h: say in header_switches() how the header now chooses its branch'
  err, rounded, out9, out6 = coefficient_errors(host, t2)
  print_table(f'se3_coef_d, error in float32 ulps of max(|exact|, envelope); switches at t2 = {sw}', t2, err)
  assert np.isfinite(out9).all() and np.isfinite(out6).all()
  assert np.array_equal(out9[:, :6], out6), 'se3_coef and se3_coef_d disagree on the shared coefficients'
  series = t2 < np.float32(sw[0])
  bad = {}
  for i, name in enumerate(R.NAMES):
    gate = np.where(series, 8.0, rounded[i] + (64.0 if i < 4 else 256.0))
    over = err[i] > gate
    if over.any():
      j = np.argmax(np.where(over, err[i] / gate, 0))
      bad[name] = f'{over.sum()} of {t2.size} points; worst t2 = {t2[j]:.9g}: {err[i, j]:.3g} ulps against {gate[j]:.3g}'
  assert not bad, bad


def test_branches_agree_across_every_switch(host):
  """Across each switch the coefficients are continuous to within the gates: the float32 neighbours just below and just above differ by
  no more than the exact function does plus both sides' allowance."""
  for s in header_switches():
    t2 = neighbours(s, 1)[[0, 1]]   # the last value below the switch, the switch itself
    err, rounded, _, _ = coefficient_errors(host, t2)
    for i, name in enumerate(R.NAMES):
      allow = 64.0 if i < 4 else 256.0
      assert err[i].max() <= rounded[i].max() + allow, (s, name, err[i])


def vector_inputs(vnorm, seed):
  t2 = sweep_t2()
  g = torch.Generator().manual_seed(seed)
  n = t2.size

  def rnd():
    return torch.randn(n, 3, generator=g, dtype=torch.float64)
  w = torch.nn.functional.normalize(rnd(), dim=-1) * torch.from_numpy(np.sqrt(t2.astype(np.float64)))[:, None]
  v = torch.nn.functional.normalize(rnd(), dim=-1) * vnorm
  x = torch.nn.functional.normalize(rnd(), dim=-1) * torch.rand(n, 1, generator=g, dtype=torch.float64)
  gg, wd, vd, xd = rnd(), rnd(), rnd(), rnd()
  return [t.float() for t in (w, v, x, gg, wd, vd, xd)]   # the float32 values are the inputs; the reference sees the same numbers


@pytest.mark.parametrize('vnorm', [0.0, 0.05, 1.0])
def test_vector_sweep(host, vnorm):
  ins = vector_inputs(vnorm, 11)
  n = ins[0].shape[0]
  arr = [_f32(t.numpy()) for t in ins]
  w, v, x, gg, wd, vd, xd = arr
  got = {k: np.empty((n, 3), np.float32) for k in ('delta', 'dw', 'dv', 'jcol', 'hdw', 'hdv')}
  xw = np.empty((n, 3), np.float32)
  host.h_se3_apply(n, _p(w), _p(v), _p(x), _p(xw))
  got['delta'] = (xw.astype(np.float64) - x.astype(np.float64))
  host.h_se3_vjp(n, _p(w), _p(v), _p(x), _p(gg), _p(got['dw']), _p(got['dv']))
  host.h_se3_dual(n, _p(w), _p(v), _p(x), _p(gg), _p(wd), _p(vd), _p(xd), _p(got['jcol']), _p(got['hdw']), _p(got['hdv']))
  ref = {k: t.numpy() for k, t in R.eval_all(*ins, torch.float64).items()}
  f32 = {k: t.double().numpy() for k, t in R.eval_all(*ins, torch.float32).items()}
  # se3_apply returns x + delta: the floor of the displacement read back from it carries the rounding of that sum
  f32['delta'] = ((ins[2] + R.eval_all(*ins, torch.float32)['delta']).double() - ins[2].double()).numpy()
  t2 = (w.astype(np.float32) ** 2).sum(1)
  print(f'\n|v| = {vnorm}: max error / max |reference| per bucket, header (floor F)')
  print('| t2 | ' + ' | '.join(got) + ' |')
  print('|---|' + '---|' * len(got))
  bad = []
  for label, m in _bucket_rows(t2):
    cells = []
    for k in got:
      scale = np.abs(ref[k][m]).max()
      if scale == 0:
        assert np.abs(got[k][m]).max() == 0, (label, k)
        cells.append('0 (0)')
        continue
      e = np.abs(got[k][m].astype(np.float64) - ref[k][m]).max() / scale
      F = np.abs(f32[k][m] - ref[k][m]).max() / scale
      cells.append(f'{e:.2e} ({F:.2e})')
      if not e <= 4 * F:
        bad.append((label, k, e, F))
    print(f'| {label} | ' + ' | '.join(cells) + ' |')
  assert not bad, bad
