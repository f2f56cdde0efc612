"""Float64 reference of the SE(3) algebra in nerfies_amd/csrc/se3_math.h, and the float32 floor its tests are gated on.

Coefficients of exp_se3 applied to a point, as functions of t2 = |w|^2, with phi_k = sum_n (-t2)^n / (2n + k)!:
  A = phi_1 = sin t / t,  B = phi_2 = (1 - cos t) / t^2,  C = phi_3 = (t - sin t) / t^3,
  Ab = 2 dA/dt2,  Bb = 2 dB/dt2,  Cb = 2 dC/dt2   (dX/dw = Xb w),  dAb = dAb/dt2,  dBb = dBb/dt2,  dCb = dCb/dt2.
Below t2 = 4 they are 20-term series in t2 (converged to 1e-16 there; partial sums stay below 1), above it closed forms in
sin / cos / t written over ONE denominator, so that no coefficient is a difference of two others divided by t2.

The vector-level algebra (se3_delta, se3_vjp, one Jacobian column on Duals) is written once on torch tensors of any dtype: in
float64 with float64 coefficients it is the reference; in float32 with those coefficients rounded to float32 it is the floor F --
the error a float32 evaluation has when its coefficients are exact, a property of the arithmetic and not of the header."""
import math

import numpy as np
import torch

NAMES = ('A', 'B', 'C', 'Ab', 'Bb', 'Cb', 'dAb', 'dBb', 'dCb')
NTERMS = 20
SERIES_T2 = 4.0   # the series below, the closed forms from here on (the 21st term at t2 = 4 is 4^20 / 41! = 3e-38)


def _series():
  def phi(k, n):
    return [(-1.0) ** i / math.factorial(2 * i + k) for i in range(n)]

  def der(p):
    return [(i + 1) * p[i + 1] for i in range(len(p) - 1)]
  out = {}
  for name, k in (('A', 1), ('B', 2), ('C', 3)):
    p = phi(k, NTERMS + 2)
    b = [2.0 * c for c in der(p)]
    out[name], out[name + 'b'], out['d' + name + 'b'] = p[:NTERMS], b[:NTERMS], der(b)[:NTERMS]
  return out


SERIES = _series()


def coef_series(t2, xp=np.float64):
  t2 = np.asarray(t2, xp)
  out = []
  for name in NAMES:
    acc = np.zeros_like(t2)
    for c in reversed(SERIES[name]):
      acc = acc * t2 + xp(c)
    out.append(acc)
  return np.stack(out)


def coef_closed(t2, xp=np.float64):
  t2 = np.asarray(t2, xp)
  t = np.sqrt(t2)
  s, c = np.sin(t), np.cos(t)
  omc = 2 * np.sin(t / 2) ** 2
  A = s / t
  B = omc / t2
  C = (t - s) / (t2 * t)
  Ab = (t * c - s) / (t2 * t)
  Bb = (t * s - 2 * omc) / t2 ** 2
  Cb = (3 * s - 2 * t - t * c) / (t2 ** 2 * t)
  dAb = (Cb - Bb) / 2
  dBb = (t2 * c - 5 * t * s + 8 * omc) / (2 * t2 ** 3)
  dCb = (t2 * s + 7 * t * c + 8 * t - 15 * s) / (2 * t2 ** 3 * t)
  return np.stack([A, B, C, Ab, Bb, Cb, dAb, dBb, dCb])


def coef_ref(t2):
  """(9, n) float64: NAMES at t2 (any shape flattened)."""
  t2 = np.asarray(t2, np.float64).reshape(-1)
  small = t2 < SERIES_T2
  out = np.empty((len(NAMES), t2.size))
  out[:, small] = coef_series(t2[small])
  out[:, ~small] = coef_closed(t2[~small])
  return out


def envelope(t2):
  """(9, n): each coefficient's local size.  Near 0 it is |X(0)|; for large t every coefficient is (polynomial in t, sin t, cos t)
  over a power of t and oscillates through zero, and its size is the amplitude of that oscillation: the leading power of t with sin and
  cos replaced by 1.  The smaller of the two, so that the envelope never exceeds what the coefficient reaches."""
  t = np.sqrt(np.maximum(np.asarray(t2, np.float64).reshape(-1), 1e-60))   # 1 / t^5 stays finite; the minimum below picks |X(0)| there
  at0 = np.array([1.0, 1 / 2, 1 / 6, 1 / 3, 1 / 12, 1 / 60, 1 / 30, 1 / 180, 1 / 1260])[:, None]
  amp = np.stack([1 / t, 2 / t ** 2, 1 / t ** 2, 1 / t ** 2, 1 / t ** 3, 3 / t ** 4, 0.5 / t ** 3, 0.5 / t ** 4, 0.5 / t ** 5])
  return np.minimum(at0, amp)


def ulp32(x):
  return np.spacing(np.abs(np.asarray(x)).astype(np.float32)).astype(np.float64)


# ------------------------------------------------------------------ the vector-level algebra, on any dtype and on Duals
class Dual:
  """value + one forward-mode tangent, on torch tensors."""

  def __init__(self, v, d=None):
    self.v, self.d = v, (torch.zeros_like(v) if torch.is_tensor(v) else 0.0) if d is None else d

  @staticmethod
  def lift(a):
    return a if isinstance(a, Dual) else Dual(a)

  def __add__(self, o):
    o = Dual.lift(o)
    return Dual(self.v + o.v, self.d + o.d)

  def __sub__(self, o):
    o = Dual.lift(o)
    return Dual(self.v - o.v, self.d - o.d)

  def __mul__(self, o):
    o = Dual.lift(o)
    return Dual(self.v * o.v, self.v * o.d + self.d * o.v)
  __radd__, __rmul__ = __add__, __mul__


def cross(a, b):
  return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def dot(a, b):
  return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _add(*vs):
  return tuple(sum(c[1:], c[0]) for c in zip(*vs))


def _scale(s, a):
  return tuple(s * c for c in a)


def delta(k, w, v, x):
  """x' - x = A w*x + B w*(w*x) + v + B w*v + C w*(w*v);  k = dict of coefficients, w / v / x = 3-tuples."""
  wx, wv = cross(w, x), cross(w, v)
  return _add(_scale(k['A'], wx), _scale(k['B'], cross(w, wx)), v, _scale(k['B'], wv), _scale(k['C'], cross(w, wv)))


def vjp(k, w, v, x, g):
  """(dw, dv) of g . (exp_se3(w, v) x)."""
  gw, wgw = cross(g, w), cross(w, cross(w, g))
  dv = _add(g, _scale(k['B'], gw), _scale(k['C'], wgw))
  wx, wv = cross(w, x), cross(w, v)
  wwx, wwv = cross(w, wx), cross(w, wv)
  wg = dot(w, g)

  def D(y):
    return _add(_scale(wg, y), _scale(dot(w, y), g), _scale(-2.0 * dot(y, g), w))
  sa = k['Ab'] * dot(g, wx) + k['Bb'] * (dot(g, wwx) + dot(g, wv)) + k['Cb'] * dot(g, wwv)
  dw = _add(_scale(k['A'], cross(x, g)), _scale(k['B'], _add(D(x), cross(v, g))), _scale(k['C'], D(v)), _scale(sa, w))
  return dw, dv


def coef_tensors(t2, dtype):
  """{name: tensor of dtype}: the exact coefficients at t2 (a tensor), rounded once to dtype."""
  c = coef_ref(t2.detach().double().numpy())
  return {n: torch.from_numpy(c[i]).reshape(t2.shape).to(dtype) for i, n in enumerate(NAMES)}


def coef_along(k, t2d):
  """Dual coefficients along a direction whose t2 tangent is t2d: X(Dual(t2, d)) = Dual(X, X'(t2) d)."""
  return {'A': Dual(k['A'], 0.5 * k['Ab'] * t2d), 'B': Dual(k['B'], 0.5 * k['Bb'] * t2d), 'C': Dual(k['C'], 0.5 * k['Cb'] * t2d),
          'Ab': Dual(k['Ab'], k['dAb'] * t2d), 'Bb': Dual(k['Bb'], k['dBb'] * t2d), 'Cb': Dual(k['Cb'], k['dCb'] * t2d)}


def _cols(a):
  return tuple(a[..., i] for i in range(3))


def _duals(a, ad):
  return tuple(Dual(p, q) for p, q in zip(_cols(a), _cols(ad)))


def eval_all(w, v, x, g, wd, vd, xd, dtype):
  """dict(delta, dw, dv, jcol, hdw, hdv), each (..., 3) of dtype: the algebra on inputs cast to dtype, with t2 = w . w formed in
  dtype and the exact coefficients AT THAT t2 rounded to dtype.  jcol is the tangent of delta along (wd, vd, xd) (one column of
  J - I when the tangents are the Jacobians of w, v, x with respect to one coordinate); hdw / hdv are the tangents of the VJP along the
  same direction (the Hessian-vector products of the elastic loss's reverse pass)."""
  w, v, x, g, wd, vd, xd = (a.to(dtype) for a in (w, v, x, g, wd, vd, xd))
  W, V, X, G = _cols(w), _cols(v), _cols(x), _cols(g)
  t2 = dot(W, W)
  k = coef_tensors(t2, dtype)
  out = {'delta': torch.stack(delta(k, W, V, X), -1)}
  dw, dv = vjp(k, W, V, X, G)
  out['dw'], out['dv'] = torch.stack(dw, -1), torch.stack(dv, -1)
  kd = coef_along(k, 2.0 * dot(W, _cols(wd)))
  Wd, Vd, Xd = _duals(w, wd), _duals(v, vd), _duals(x, xd)
  out['jcol'] = torch.stack([c.d for c in delta(kd, Wd, Vd, Xd)], -1)
  hdw, hdv = vjp(kd, Wd, Vd, Xd, tuple(Dual(c) for c in G))
  out['hdw'], out['hdv'] = torch.stack([c.d for c in hdw], -1), torch.stack([c.d for c in hdv], -1)
  return out
