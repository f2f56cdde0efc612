"""Shared test plumbing: oracle ModelSpec -> nerfies_amd model on the GPU with identical parameters."""
import ctypes as C
import functools
import os
import types

import numpy as np
import torch

from oracle import nerfies_oracle as O

DEV = 'cuda:0'


def config_from_spec(spec):
  """An object with the configs.ModelConfig attribute names construct_nerf reads (configs.py:35-105)."""
  return types.SimpleNamespace(
      num_coarse_samples=spec.num_coarse_samples, num_fine_samples=spec.num_fine_samples,
      use_viewdirs=spec.use_viewdirs, nerf_trunk_depth=spec.nerf_trunk_depth, nerf_trunk_width=spec.nerf_trunk_width,
      nerf_rgb_branch_depth=spec.nerf_rgb_branch_depth, nerf_rgb_branch_width=spec.nerf_rgb_branch_width,
      nerf_skips=tuple(spec.nerf_skips), use_stratified_sampling=spec.use_stratified_sampling,
      num_nerf_point_freqs=spec.num_nerf_point_freqs, num_nerf_viewdir_freqs=spec.num_nerf_viewdir_freqs,
      sigma_activation=spec.sigma_activation, use_white_background=spec.use_white_background,
      use_linear_disparity=spec.use_linear_disparity, use_sample_at_infinity=spec.use_sample_at_infinity,
      use_appearance_metadata=spec.use_appearance_metadata, use_camera_metadata=spec.use_camera_metadata,
      appearance_metadata_dims=spec.num_appearance_features, camera_metadata_dims=spec.num_camera_features,
      use_warp=spec.use_warp, num_warp_freqs=spec.num_warp_freqs, num_warp_features=spec.num_warp_features,
      warp_field_type=spec.warp_field_type, use_alpha_condition=spec.use_alpha_condition, use_rgb_condition=spec.use_rgb_condition,
      noise_std=spec.noise_std, warp_metadata_encoder_type=spec.warp_metadata_encoder_type, warp_kwargs=warp_kwargs_from_spec(spec))


def warp_kwargs_from_spec(spec):
  """ModelConfig.warp_kwargs (configs.py:105) as a Gin file would bind them: the trunk's depth / width under the field's own attribute
  names (SE3Field trunk_depth / trunk_width, warping.py:225-226; TranslationField depth / hidden_channels, warping.py:90-91)."""
  d, w = getattr(spec, 'warp_trunk_depth', 6), getattr(spec, 'warp_trunk_width', 128)
  if not spec.use_warp or (d, w) == (6, 128):
    return {}
  dk, wk = ('depth', 'hidden_channels') if spec.warp_field_type == 'translation' else ('trunk_depth', 'trunk_width')
  return {dk: d, wk: w}


def gpu_model(spec, oparams, batch_size=0):
  """(model, FlatParams on DEV) holding exactly the oracle parameter tree `oparams`."""
  from nerfies_amd import models, params as P
  model, fp = models.construct_nerf(
      0, config_from_spec(spec), batch_size, list(range(spec.num_appearance_embeddings)),
      list(range(spec.num_camera_embeddings)), list(range(spec.num_warp_embeddings)), spec.near, spec.far)
  P.flat_from_tree(O.tree_map(lambda t: t.float(), oparams), model.layout, DEV, out=fp.flat)
  return model, fp


# ---------------------------------------------------------------------------------------------
# The Python host without a GPU: a model on CPU tensors whose library records the entries that would follow device pointers
# ---------------------------------------------------------------------------------------------
_ENTRY_ARGS = {   # entry -> (its `fn` in a record, the names of its arguments in the header's order)
    'nrf_query_points': ('points', 'h params groups points S level scalars flags out ws nbytes stream'),
    'nrf_query_points_grad': ('grad', 'h params groups points S level scalars flags out ws nbytes stream'),
    'nrf_query_grid': ('grid', 'h params groups grid first count level scalars flags out ws nbytes stream'),
    'nrf_query_grid_grad': ('grid_grad', 'h params groups grid first count level scalars flags out ws nbytes stream'),
    'nrf_unwarp_points': ('unwarp', 'h params targets ids codes num_codes guess n scalars steps tolerance max_step out ws nbytes stream'),
    'nrf_mesh_count': ('count', 'sigma grid thr counts ws nbytes stream'),
    'nrf_mesh_emit': ('emit', 'sigma grid thr mv mt vertices cell tris ws nbytes stream'),
    'nrf_mesh_snap': ('snap', 'vertices cell sigma_at grad_at grid thr n stream'),
}
_FIELD_NAMES = {'grad_sigma': 'grad', 'warped_points': 'warped', 'warp_alpha': 'alpha'}   # struct fields under the records' shorter names


class RecordingLib:
  """The library with the entries `names` replaced by recorders that return 0; every other entry (handle, layout, workspace sizes)
  is the real one.  A record is a dict: `fn`, every scalar argument and pointer value under the argument's name, and the fields
  of every struct argument (lib.Rays, lib.Grid, the out struct, lib.StepScalars) under their own (_FIELD_NAMES).  No recorder
  follows a pointer, so the host code runs on CPU tensors; the one of nrf_mesh_count reports `found` = (vertices, triangles)
  through its counts pointer (host memory then).  `peek(record)` sees a record while the call's tensors are still alive."""

  def __init__(self, real, names, found=(0, 0), peek=None):
    self._real, self._names, self.found, self.peek = real, tuple(names), found, peek
    self.calls = []

  def __getattr__(self, name):
    return functools.partial(self._record, name) if name in self._names else getattr(self._real, name)

  def _record(self, name, *args):
    fn, argnames = _ENTRY_ARGS.get(name, (name, ''))
    call = dict(fn=fn) if argnames else dict(fn=fn, args=args)
    for k, v in zip(argnames.split(), args):
      v = getattr(v, '_obj', v)   # ctypes.byref(struct)
      if isinstance(v, C.Structure):
        for f, _ in v._fields_:
          x = getattr(v, f)
          call[_FIELD_NAMES.get(f, f)] = tuple(x) if isinstance(x, C.Array) else x
      else:
        call[k] = v.value if isinstance(v, C.c_void_p) else v
    if name == 'nrf_mesh_count':
      out = C.cast(call['counts'], C.POINTER(C.c_int32))
      out[0], out[1] = self.found
    if self.peek is not None:
      self.peek(call)
    self.calls.append(call)
    return 0


def cpu_field_model(lib, **cfg):
  """(model, FlatParams) on the CPU for the host tests of the field entries: a small SE3 model with three warp ids and two appearance
  and camera ids, its library `lib` (a RecordingLib)."""
  from nerfies_amd import models
  cfg = types.SimpleNamespace(**dict(dict(use_warp=True, warp_field_type='se3', num_warp_freqs=4, num_nerf_point_freqs=6,
                                          sigma_activation='softplus', use_stratified_sampling=False), **cfg))
  model, fp = models.construct_nerf(0, cfg, 0, [0, 1], [0, 1], [0, 1, 2], 0.1, 1.0, device='cpu')
  model._lib = lib
  return model, fp


def lift_device_rule(monkeypatch):
  """NerfModel's device rule (models._gpu_reader) lifted for a test: a tensor of any device passes, and the call gets no stream.  For
  a model whose library is a RecordingLib: the public methods then run on CPU tensors."""
  from nerfies_amd import models
  monkeypatch.setattr(models, '_gpu_reader', lambda what, t: (torch.as_tensor(t).device, None))


def ws_bytes(nbytes):
  """The bytes of the float32 workspace NerfModel allocates for a sizer's answer `nbytes` (rounded up to whole floats)."""
  return 4 * ((nbytes + 3) // 4)


def gpu_batch(batch):
  out = {k: v.to(DEV).float() for k, v in batch.items() if torch.is_tensor(v)}
  out['metadata'] = {k: (v.to(DEV).float() if v.is_floating_point() else v.to(DEV)) for k, v in batch.get('metadata', {}).items()}
  return out


def flat_grad_from_tree(grads, layout):
  from nerfies_amd import params as P
  return P.flat_from_tree(O.tree_map(lambda t: t.float(), grads), layout, 'cpu')


# ---------------------------------------------------------------------------------------------
# ReLU sign bits of the last stashed forward (training workspace), decoded to boolean masks the
# oracle can be pinned to (oracle.relu_hook).  Layout: include/nerfies_amd.h nrf_debug_ws_offset.
# ---------------------------------------------------------------------------------------------
def _ws_words(model, ws, name, level, nwords):
  import ctypes as C
  from nerfies_amd import lib as L
  off = C.c_int64(0)
  L.check(model.lib.nrf_debug_ws_offset(model.handle, name.encode(), level, C.byref(off)), model.lib)
  return ws[off.value:off.value + nwords].view(torch.int32).cpu().numpy().view('uint32')


def _decode_bits(words, nlayers, ntiles, ncb, rows):
  """words: uint32 [nlayers][ntiles][4 waves][64 lanes][ncb] -> bool [nlayers][rows][4 * 32 * ncb]."""
  import numpy as np
  w = words.reshape(nlayers, ntiles, 4, 64, ncb)
  q, e = np.arange(8), np.arange(4)
  bits = ((w[..., None, None] >> (4 * q[:, None] + e[None, :]).astype('uint32')) & 1).astype(bool)   # [L][t][wave][lane][cb][q][e]
  lane = np.arange(64)
  j, h = lane & 31, lane >> 5
  g = (q[None, :] & 1) + 2 * h[:, None] + 4 * (q[None, :] >> 1)          # [lane][q]
  p = 4 * g[:, :, None] + e[None, None, :]                               # [lane][q][e] tile row
  wave, cb = np.arange(4), np.arange(ncb)
  n = wave[:, None, None] * 32 * ncb + 32 * cb[None, None, :] + j[None, :, None]   # [wave][lane][cb] feature
  out = np.zeros((nlayers, ntiles * 64, 4 * 32 * ncb), bool)
  t = np.arange(ntiles)
  rows_idx = (t[:, None, None, None, None, None] * 64 + p[None, None, :, None, :, :])          # [t][1][lane][1][q][e]
  rows_idx = np.broadcast_to(rows_idx, (ntiles, 4, 64, ncb, 8, 4))
  cols_idx = np.broadcast_to(n[None, :, :, :, None, None], (ntiles, 4, 64, ncb, 8, 4))
  for l in range(nlayers):
    out[l][rows_idx, cols_idx] = bits[l]
  return torch.from_numpy(out[:, :rows])


def trunk_layer_map(spec):
  """The chain layer (0..7) each of the caller's trunk layers runs on (csrc/nrf_api.hip nrf_create): in place, unless the trunk's skip
  s <= 4 with depth - s <= 4 is laid out around the kernels' own skip layer 4 (identity layers s..3 in between); the layers behind
  the caller's last one are identities as well and appear in no oracle hook."""
  xd = spec.nerf_trunk_depth
  xs = spec.nerf_skips[0] if (len(spec.nerf_skips) and spec.nerf_skips[0] < xd) else -1
  imap = list(range(8))
  if 0 <= xs <= 4 and xd - xs <= 4:
    for i in range(xs, xd):
      imap[i] = 4 + (i - xs)
  return imap[:xd] + [l for l in range(8) if l not in imap[:xd]]


def gpu_relu_masks(model, spec, num_rays, nbg=0, elastic=False):
  """{oracle hook name: [bool (rows, width) per layer]} read back from the training workspace of the last
  loss_and_grad / apply(train=True) call with these sizes."""
  ws = model.workspace(num_rays, True, DEV, nbg, elastic)
  torch.cuda.synchronize()
  masks = {}
  WW = getattr(spec, 'warp_trunk_width', 128)
  levels = [('coarse', 0, num_rays * spec.num_coarse_samples)]
  if spec.num_fine_samples > 0:
    levels.append(('fine', 1, num_rays * (spec.num_coarse_samples + spec.num_fine_samples)))
  for name, lv, rows in levels:
    nt = (rows + 63) // 64
    m = _decode_bits(_ws_words(model, ws, 'bits_trunk', lv, nt * 4 * 128 * 8), 8, nt, 2, rows)
    masks[f'{name}/MLP_0'] = [m[l][:, :spec.nerf_trunk_width] for l in trunk_layer_map(spec)]
    m = _decode_bits(_ws_words(model, ws, 'bits_rgbh', lv, nt * 4 * 64), 1, nt, 1, rows)
    masks[f'{name}/MLP_1'] = [m[0][:, :spec.nerf_rgb_branch_width]]
    if spec.use_warp:
      m = _decode_bits(_ws_words(model, ws, 'w_bits', lv, nt * 4 * 64 * 6), 6, nt, 1, rows)
      masks[f'{name}/warp'] = [m[l][:, :WW] for l in range(6)]
  if spec.use_warp and nbg > 0:
    nt = (nbg + 63) // 64
    m = _decode_bits(_ws_words(model, ws, 'w_bits', 2, nt * 4 * 64 * 6), 6, nt, 1, nbg)
    masks['background/warp'] = [m[l][:, :WW] for l in range(6)]
  return masks


class PinnedRelu:
  """oracle.relu_hook callable: activation = pre * mask with the HIP path's masks.  Records where the oracle's own sign
  disagrees: `flips` / `total` units and, per disagreeing unit, |pre| relative to its layer's rms (`mags`)."""

  def __init__(self, masks):
    self.masks = masks
    self.flips, self.total, self.mags = 0, 0, []

  def __call__(self, name, layer, pre):
    m = self.masks[name][layer].reshape(pre.shape)
    with torch.no_grad():
      bad = (pre.detach() > 0) != m
      nb = int(bad.sum())
      self.flips += nb
      self.total += m.numel()
      if nb:
        rms = float(pre.detach().pow(2).mean().sqrt())
        self.mags.append(pre.detach()[bad].abs().double() / max(rms, 1e-30))
    return pre * m.to(pre.dtype)

  @property
  def worst(self):
    return float(torch.cat(self.mags).max()) if self.mags else 0.0

  def quantile(self, q):
    return float(torch.cat(self.mags).quantile(q)) if self.mags else 0.0


# ---------------------------------------------------------------------------------------------
# Pinned-branch gradient parity (see tests/test_gpu_pinned.py for the rationale)
# ---------------------------------------------------------------------------------------------
FLIP_FRACTION = 2e-3     # units whose fp64 sign differs from the HIP path's
FLIP_PRE = 5e-3          # ... and the 95th percentile of their |pre| relative to the layer rms (rounding-level ties only)


def grad_tol(spec):
  """Per-leaf gradient tolerance, relative to the leaf's max-abs entry: 2e-3, and 4e-3 with the warp on at F_p = 9, 10.
  With the warp on, float32 rounding of the warped point (3e-8 absolute) is a phase error of 2^(F_p-1) * 3e-8 in the top
  posenc band; the per-sample dL/dx' (dominated by the top bands, magnitude ~2^F_p) cancels across samples into a much
  smaller parameter gradient, so the RELATIVE error of the warp leaves grows like 2^F_p in ANY float32 evaluation: the
  oracle's own float32 restatement, with identical branches and samples, is 4e-4 from float64 at F_p = 8 and 1-2e-3 at
  F_p = 10 (tests/test_pinned_host.py::test_float32_floor_of_the_warp_gradients)."""
  return 4e-3 if (spec.use_warp and spec.num_nerf_point_freqs > 8) else 2e-3


def host_threads(n):
  class _T:
    def __enter__(self):
      self.prev = torch.get_num_threads()
      torch.set_num_threads(max(1, min(n, os.cpu_count() or 1)))

    def __exit__(self, *a):
      torch.set_num_threads(self.prev)
  return _T()


def leaf(tree, path):
  node = tree
  for k in path.split('/'):
    node = node[k]
  return node


def run_pinned(spec, B, alpha, seed=3, strat=True, elastic=None, background=None, params=None, batch=None, t_rand=None, u=None,
               warp_reg=None, time_alpha=None, check_fine_z=True):
  """GPU loss_and_grad, masks read back, fp64 oracle pinned to them.  Returns a dict of everything compared."""
  from nerfies_amd import params as P
  p64 = params if params is not None else O.init_params(spec, seed=seed, trained_like=True, dtype=torch.float64)
  b64 = batch if batch is not None else O.synthetic_batch(B, seed=seed + 1, dtype=torch.float64)
  model, fp = gpu_model(spec, p64, B)
  gb = gpu_batch(b64)
  rngs = None
  if spec.use_stratified_sampling and t_rand is None:
    g = torch.Generator().manual_seed(seed)
    t_rand = torch.rand(B, spec.num_coarse_samples, generator=g).double()
    u = torch.rand(B, spec.num_fine_samples, generator=g).double()
  if t_rand is not None:
    rngs = {'coarse': t_rand.float().to(DEV), 'fine': u.float().to(DEV)}
  gkw, okw, nbg = {}, {}, 0
  if background is not None:   # dict(points, warp_ids, noise, weight)
    nbg = background['points'].shape[0]
    gkw['background'] = {'points': (background['points'] + background['noise']).float().to(DEV),
                         'warp_ids': background['warp_ids'].to(DEV), 'weight': background['weight']}
    okw.update(use_background_loss=True, background_loss_weight=background['weight'],
               background={k: background[k] for k in ('points', 'warp_ids', 'noise')})
  if elastic is not None:      # dict(weight, reduce_method[, loss_type])
    gkw['elastic'] = dict(elastic)
    okw.update(use_elastic_loss=True, elastic_loss_weight=elastic['weight'], elastic_reduce_method=elastic.get('reduce_method', 'weight'),
               elastic_loss_type=elastic.get('loss_type', 'log_svals'))
  if warp_reg is not None:     # dict(weight[, alpha, scale])
    gkw['warp_reg'] = dict(warp_reg)
    okw.update(use_warp_reg_loss=True, warp_reg_loss_weight=warp_reg['weight'], warp_reg_loss_alpha=warp_reg.get('alpha', -2.0),
               warp_reg_loss_scale=warp_reg.get('scale', 0.001))
  if spec.noise_std and spec.use_stratified_sampling:   # explicit normals for model_utils.noise_regularize
    g2 = torch.Generator().manual_seed(seed + 77)
    nz_c = torch.randn(B, spec.num_coarse_samples, generator=g2).double()
    nz_f = torch.randn(B, spec.num_coarse_samples + spec.num_fine_samples, generator=g2).double()
    rngs = dict(rngs or {}, noise_coarse=nz_c.float().to(DEV), noise_fine=nz_f.float().to(DEV))
    okw.update(noise_coarse=nz_c, noise_fine=nz_f)
  if time_alpha is not None:   # warp_extra['time_alpha'] (TimeEncoder window, models.py:252-254)
    okw['time_alpha'] = time_alpha
  grad, stats = model.loss_and_grad(fp, gb, warp_extra={'alpha': alpha, 'time_alpha': time_alpha or 0.0}, rngs=rngs, **gkw)
  torch.cuda.synchronize()
  masks = gpu_relu_masks(model, spec, B, nbg, elastic is not None)
  hook = PinnedRelu(masks)
  # the fine samples are a stop_gradient input of the fine pass (model_utils.py:187): the oracle takes the HIP path's own
  # (they agree with its natural ones to ~1e-5, asserted below; through the 2^(F_p-1) posenc that difference alone
  # would move the gradients by more than the kernels' own error)
  z_fine = None
  if spec.num_fine_samples > 0:
    ws = model.workspace(B, True, DEV, nbg, elastic is not None)
    S1 = spec.num_coarse_samples + spec.num_fine_samples
    z_fine = _ws_words(model, ws, 'z', 1, B * S1).view('float32').reshape(B, S1)
    z_fine = torch.from_numpy(z_fine.copy()).double()
  with O.relu_hook(hook):
    loss, ostats, ograds, ret = O.loss_and_grad(p64, spec, b64, warp_alpha=alpha, t_rand=t_rand, u=u, fixed_fine_z=z_fine, **okw)
  if z_fine is not None:   # ... and its own resampling lands on the same depths
    with torch.no_grad():
      z_nat = O.sample_pdf(.5 * (ret['coarse']['z_vals'][..., 1:] + ret['coarse']['z_vals'][..., :-1]), ret['coarse']['weights'][..., 1:-1],
                           b64['origins'], b64['directions'], ret['coarse']['z_vals'], spec.num_fine_samples,
                           spec.use_stratified_sampling, u)[0]
    # check_fine_z=False (tests/test_gpu_density_regimes.py): where the coarse weights are 1e-9 or a step, the inverse CDF of
    # model_utils.py:139-215 is flat or vertical and moves single samples by whole bins under float32 rounding of the weights in ANY
    # float32 evaluation; the oracle is given the HIP path's depths either way, and the resampling has its own forward tests
    if check_fine_z:
      assert (z_nat - z_fine).abs().max().item() < 2e-4 * (spec.far - spec.near), (z_nat - z_fine).abs().max().item()
      assert (z_nat - z_fine).abs().mean().item() < 2e-6 * (spec.far - spec.near)
    else:
      print(f'[fine depths, HIP path vs the oracle\'s own resampling] max {(z_nat - z_fine).abs().max().item():.2e} mean {(z_nat - z_fine).abs().mean().item():.2e}')
  got = P.tree_from_flat(grad.cpu(), model.layout)
  errs = {}
  for path, og in O.tree_leaves_with_path(ograds):
    scale = max(og.abs().max().item(), 1e-30)
    errs[path] = ((leaf(got, path).double() - og).abs().max().item() / scale, scale)
  return dict(model=model, fp=fp, gb=gb, rngs=rngs, stats=stats.cpu(), loss=loss.item(), ostats=ostats, ret=ret, errs=errs, hook=hook,
              alpha=alpha, time_alpha=time_alpha, tol=grad_tol(spec), spec=spec, p64=p64, b64=b64, t_rand=t_rand, u=u, okw=okw, got=got)


def assert_unpinned(r, label, factor=3.0):
  """The UNPINNED full-shape statistic: the same HIP gradient against the FREE-RUNNING float64 oracle -- its own
  ReLU branches, its own fine samples, nothing taken from the HIP path -- as per-leaf relative L2 distance, next to the distance of
  the oracle's own float32 evaluation from that float64 run.  float32 ties flip whole ReLU columns in ANY float32 evaluation
  order, so element-wise agreement is not a property a float32 path can have (that is what the pinned comparison removes); what
  can be asserted without conditioning on the HIP path's outputs is that it sits no further from float64 than `factor` x the
  reference arithmetic restated in float32 does."""
  spec, p64, b64 = r['spec'], r['p64'], r['b64']
  to32 = lambda t: t.float() if torch.is_tensor(t) and t.is_floating_point() else t
  _, _, g64, _ = O.loss_and_grad(p64, spec, b64, warp_alpha=r['alpha'], t_rand=r['t_rand'], u=r['u'], **r['okw'])
  p32 = O.tree_map(to32, p64)
  b32 = {k: (O.tree_map(to32, v) if isinstance(v, dict) else to32(v)) for k, v in b64.items()}
  okw32 = {k: (O.tree_map(to32, v) if isinstance(v, dict) else to32(v)) for k, v in r['okw'].items()}
  _, _, g32, _ = O.loss_and_grad(p32, spec, b32, warp_alpha=r['alpha'], t_rand=to32(r['t_rand']) if r['t_rand'] is not None else None,
                                 u=to32(r['u']) if r['u'] is not None else None, **okw32)
  worst = ('', 0.0, 0.0)
  rows = []
  for (path, want), (_, f32) in zip(O.tree_leaves_with_path(g64), O.tree_leaves_with_path(g32)):
    nrm = max(want.norm().item(), 1e-30)
    l2_gpu = (leaf(r['got'], path).double() - want).norm().item() / nrm
    l2_f32 = (f32.double() - want).norm().item() / nrm
    rows.append((path, l2_gpu, l2_f32))
    if l2_gpu > worst[1]:
      worst = (path, l2_gpu, l2_f32)
  med_gpu = sorted(x[1] for x in rows)[len(rows) // 2]
  med_f32 = sorted(x[2] for x in rows)[len(rows) // 2]
  print(f'[{label}, UNPINNED vs the free-running float64 oracle] per-leaf relative L2: worst {worst[0]} hip {worst[1]:.2e} '
        f'(float32 oracle {worst[2]:.2e}); median hip {med_gpu:.2e} / float32 oracle {med_f32:.2e}')
  for path, l2_gpu, l2_f32 in rows:
    assert l2_gpu <= factor * l2_f32 + 1e-5, (label, path, l2_gpu, l2_f32)


def assert_pinned(r, label, loss_tol=1e-5):
  assert abs(r['stats'][4].item() - r['loss']) < loss_tol, (label, r['stats'][4].item(), r['loss'])
  worst = max(r['errs'].items(), key=lambda kv: kv[1][0])
  print(f'[{label}] loss gpu {r["stats"][4].item():.7f} oracle {r["loss"]:.7f}; worst leaf {worst[0]} rel err {worst[1][0]:.2e}; '
        f'ReLU ties {r["hook"].flips}/{r["hook"].total} (|pre|/rms: 95 % below {r["hook"].quantile(0.95):.1e}, max {r["hook"].worst:.1e})')
  for path, (err, scale) in r['errs'].items():
    assert err < r['tol'], (label, path, err, scale)
  h = r['hook']
  assert h.flips <= FLIP_FRACTION * h.total, (label, h.flips, h.total)
  assert h.quantile(0.95) < FLIP_PRE, (label, h.quantile(0.95), h.worst)


def assert_forward(r, spec, atol=1e-4):
  """The rendered outputs of a (non-training) forward on the same rays against the pinned oracle's."""
  out = r['model'].apply({'params': r['fp']}, r['gb'], {'alpha': r['alpha'], 'time_alpha': r.get('time_alpha') or 0.0}, rngs=r['rngs'],
                         return_weights=True)
  for lv in out:
    for k in ('rgb', 'depth', 'acc', 'weights'):
      np.testing.assert_allclose(out[lv][k].cpu().numpy(), r['ret'][lv][k].detach().numpy(), atol=atol, err_msg=f'{lv}/{k}')


# ---------------------------------------------------------------------------------------------
# One stashed training forward + the float64 oracle pinned to it (moved here from tests/test_gpu_backward_ex.py so that
# tests/test_gpu_density_regimes.py shares it; `params` / `batch` let a caller bring its own tree instead of the seeded one)
# ---------------------------------------------------------------------------------------------
OUTPUTS = ('rgb', 'depth', 'acc', 'weights')


def cotangents_to_gpu(cot):
  return {lv: {k: t.float().to(DEV) for k, t in d.items()} for lv, d in cot.items()}


class Pinned:
  """One stashed training forward on the GPU and the float64 oracle pinned to its ReLU pattern and fine depths; `compare(cot)`
  back-propagates the cotangents `cot` through both and returns the worst per-leaf error relative to the leaf's max-abs."""

  def __init__(self, spec, nrays, seed, alpha=0.0, tile_rows=0, points=False, params=None, batch=None):
    self.spec, self.alpha = spec, alpha
    self.p64 = params if params is not None else O.init_params(spec, seed=seed, trained_like=True, dtype=torch.float64)
    self.b64 = batch if batch is not None else O.synthetic_batch(nrays, seed=seed + 1, dtype=torch.float64)
    self.model, self.fp = gpu_model(spec, self.p64, nrays)
    if tile_rows:
      self.model.set_chain_tile_rows(tile_rows)
    self.gb = gpu_batch(self.b64)
    out = self.model.apply({'params': self.fp}, self.gb, {'alpha': alpha}, train=True, return_weights=True, return_z_vals=True)
    torch.cuda.synchronize()
    masks = gpu_relu_masks(self.model, spec, nrays)
    z_fine = out['fine']['z_vals'].cpu().double()
    leaves = list(O.tree_leaves_with_path(self.p64))
    self.paths = [p for p, _ in leaves]
    self.req = [t.detach().clone().requires_grad_(True) for _, t in leaves]
    it = iter(self.req)
    params_r = O.tree_map(lambda _: next(it), self.p64)
    self.hook = PinnedRelu(masks)
    with O.relu_hook(self.hook):
      self.ret = O.nerf_model_apply(params_r, spec, self.b64, warp_alpha=alpha, fixed_fine_z=z_fine, return_points=points)
    for lv in ('coarse', 'fine'):   # the two forwards agree, so the pinned comparison is of one function
      for k in OUTPUTS:
        np.testing.assert_allclose(out[lv][k].cpu().numpy(), self.ret[lv][k].detach().numpy(), atol=1e-4, err_msg=f'{lv}/{k}')
    assert self.hook.flips <= FLIP_FRACTION * self.hook.total, (self.hook.flips, self.hook.total)

  def oracle_grads(self, cot):
    loss = sum((self.ret[lv][k] * t).sum() for lv, d in cot.items() for k, t in d.items())
    grads = torch.autograd.grad(loss, self.req, allow_unused=True, retain_graph=True)
    return {p: (g if g is not None else torch.zeros_like(t)) for p, g, t in zip(self.paths, grads, self.req)}

  def gpu_grads(self, cot, **kw):
    from nerfies_amd import params as P
    grad = self.model.backward({'params': self.fp}, self.gb, d_out=cotangents_to_gpu(cot), **kw)
    return P.tree_from_flat(grad.cpu(), self.model.layout)

  def compare(self, cot, label):
    want, got = self.oracle_grads(cot), self.gpu_grads(cot)
    errs = {}
    for path, og in want.items():
      scale = max(og.abs().max().item(), 1e-30)
      errs[path] = ((leaf(got, path).double() - og).abs().max().item() / scale, scale)
    worst = max(errs.items(), key=lambda kv: kv[1][0])
    print(f'[{label}] worst leaf {worst[0]} rel err {worst[1][0]:.2e} (max-abs {worst[1][1]:.2e}); tolerance {grad_tol(self.spec):.0e}')
    for path, (err, scale) in errs.items():
      assert err < grad_tol(self.spec), (label, path, err, scale)
    return want, got


# ---------------------------------------------------------------------------------------------
# bf16 training stash (csrc/nrf_internal.h BfStash) decoded to [rows, features] float64 matrices
# ---------------------------------------------------------------------------------------------
def bf16_stash(model, ws, name, level, nlayers, nblocks, rows, as_float32=False, ngroups=None):
  """Buffer `name` ("b_pe", "b_h", "b_bn", "b_rgbh", "b_dy", "b_dbn", "b_drgbh", "b_dsmall") of `level`: [nlayers] matrices
  (rows, 32 * nblocks).  Layout per 32-sample group: [block b][jp][lane = n + 32 h][8 bf16], the 8 = features
  32 b + 8 (2 jp + jj) + 4 h + i in (jj, i) order."""
  ng = ngroups if ngroups is not None else (rows + 255) // 256 * 8
  words = _ws_words(model, ws, name, level, nlayers * ng * nblocks * 512)
  a = words.view('uint16').reshape(nlayers, ng, nblocks, 2, 2, 32, 2, 4)        # [L][g][b][jp][h][n][jj][i]
  a = a.transpose(0, 1, 5, 2, 3, 6, 4, 7).reshape(nlayers, ng * 32, nblocks * 32)  # [L][g, n][b, jp, jj, h, i]
  f = (a.astype('uint32') << 16).view('float32')
  if not as_float32:   # float32 holds a bfloat16 exactly: the full-shape tests keep it to halve the host memory
    f = f.astype('float64')
  return [torch.from_numpy(f[l, :rows].copy()) for l in range(nlayers)]


def bf16_round(t):
  return t.float().to(torch.bfloat16).double()


# ---------------------------------------------------------------------------------------------
# tests/golden/make_reference_vectors.py::loss_directional -- the seeded parameter directions and the cases, shared by the CPU
# (oracle autograd vs the reference's finite difference) and the GPU test (HIP gradient vs the same numbers)
# ---------------------------------------------------------------------------------------------
LOSS_DIR_CASES = {
    'nowarp': dict(spec=dict(num_coarse_samples=64, num_fine_samples=128, num_nerf_point_freqs=8, use_stratified_sampling=True),
                   B=12, alpha=0.0, bg=0),
    'warp_bg': dict(spec=dict(num_coarse_samples=24, num_fine_samples=24, num_nerf_point_freqs=6, use_stratified_sampling=True, use_warp=True,
                              num_warp_freqs=5, num_warp_features=8, use_camera_metadata=True), B=8, alpha=3.25, bg=9),
}


def loss_directions(params, seed, ndir):
  """[{path tuple: float64 array}] exactly as make_reference_vectors.loss_directions draws them: leaves in sorted path order,
  standard normals scaled by the leaf's rms + 1e-3."""
  leaves = []

  def walk(t, path):
    for k in sorted(t):
      if isinstance(t[k], dict):
        walk(t[k], path + (k,))
      else:
        leaves.append((path + (k,), np.asarray(t[k].detach().double().numpy() if torch.is_tensor(t[k]) else t[k], dtype=np.float64)))
  walk(params, ())
  rng = np.random.default_rng(seed)
  dirs = []
  for _ in range(ndir):
    dirs.append({path: rng.standard_normal(a.shape) * (np.sqrt(np.mean(a * a)) + 1e-3) for path, a in leaves})
  return dirs


def tree_dot(grads, direction, path=()):
  """<grad tree, direction> in float64."""
  tot = 0.0
  for k, v in grads.items():
    if isinstance(v, dict):
      tot += tree_dot(v, direction, path + (k,))
    else:
      g = v.detach().double().cpu().numpy() if torch.is_tensor(v) else np.asarray(v, dtype=np.float64)
      tot += float((g * direction[path + (k,)]).sum())
  return tot



# ---------------------------------------------------------------------------------------------
# Density regimes (tests/test_density_regimes_host.py, tests/test_gpu_density_regimes.py, profiles/density_regimes.md)
#
# oracle.init_params(trained_like=True) keeps every softplus density within (0.4, 0.8) and the fine relu density at 0.  A regime
# rewrites each level's density head (MLP_2/logit: kernel x K, a new bias) so that chosen quantiles of the level's own raw density
# land at chosen values, measured on the float64 oracle; the optional colour option scales the rgb head (MLP_1/logit) the same way.
# ---------------------------------------------------------------------------------------------
REGIMES = ('empty', 'surface', 'opaque')
LEVELS = ('coarse', 'fine')


def _heads(params, spec, batch):
  """One float64 oracle evaluation: {level: dict(raw (B,S) raw density, rgb (B,S,3) raw colour, z (B,S))}."""
  seen = {}
  key = {}
  for lv in LEVELS:
    key[id(params[f'nerf_mlps_{lv}']['MLP_2']['logit'])] = (lv, 'raw')
    key[id(params[f'nerf_mlps_{lv}']['MLP_1']['logit'])] = (lv, 'rgb')

  def hook(p, x):
    y = x @ p['kernel'] + p['bias']
    if id(p) in key:
      seen[key[id(p)]] = y.detach()
    return y
  with torch.no_grad(), O.dense_hook(hook):
    ret = O.nerf_model_apply(params, spec, batch)
  out = {}
  for lv in LEVELS:
    z = ret[lv]['z_vals']
    out[lv] = dict(raw=seen[(lv, 'raw')].reshape(z.shape), rgb=seen[(lv, 'rgb')].reshape(*z.shape, 3), z=z)
  return out


def _dists(spec, z, directions):
  last = 1e10 if spec.use_sample_at_infinity else 1e-19
  d = torch.cat([z[..., 1:] - z[..., :-1], torch.full_like(z[..., :1], last)], -1)
  return d * torch.linalg.norm(directions, dim=-1, keepdim=True)


def regime_stats(spec, head, directions):
  """What the regime conditions are stated on, from one level's float64 raw density / colour / depths."""
  raw, z = head['raw'], head['z']
  sigma = O._sigma_act(spec.sigma_activation, raw)
  dist = _dists(spec, z, directions)
  alpha = 1.0 - torch.exp(-sigma * dist)
  T = torch.cat([torch.ones_like(alpha[..., :1]), torch.cumprod(1.0 - alpha[..., :-1] + 1e-10, -1)], -1)
  a32 = 1.0 - torch.exp(-sigma.float() * dist.float())
  T32 = torch.cumprod(1.0 - a32 + 1e-10, -1)   # float32, inclusive: what the transmittance ends at
  rgb = torch.sigmoid(head['rgb'])
  n = float(sigma.numel())
  return dict(
      raw_min=raw.min().item(), raw_max=raw.max().item(), sigma_min=sigma.min().item(), sigma_max=sigma.max().item(),
      sigma_zero=(sigma == 0).sum().item() / n, sigma_lt_1e6=(sigma < 1e-6).sum().item() / n, sigma_lt_1e4=(sigma < 1e-4).sum().item() / n,
      tau_gt_5=(sigma * dist > 5).sum().item() / n, alpha_gt_099=(alpha > 0.99).sum().item() / n,
      rays_T_lt_1e3=(T[..., -1] < 1e-3).sum().item() / T.shape[0], rays_T_gt_half=(T.min(-1).values > 0.5).sum().item(),
      rays_T32_zero=(T32[..., -1] == 0).sum().item() / T.shape[0], T_min=T.min().item(),
      rgb_saturated=((rgb < 1e-3) | (rgb > 1 - 1e-3)).sum().item() / float(rgb.numel()))


def _quantile(x, q):
  return torch.quantile(x.reshape(-1), q).item()


def _density_head(spec, regime, head, bias, directions):
  """(K, new bias) of one level's density head: with u = raw - bias the head's bias-free output, the new raw density is K u + b."""
  u = head['raw'] - bias
  dist = _dists(spec, head['z'], directions)
  finite = torch.ones_like(u, dtype=torch.bool)
  finite[..., -1] = False   # the last distance (1e10 |d| or 1e-19 |d|) says nothing about the ray's extent
  relu = spec.sigma_activation == 'relu'
  if regime == 'empty':      # median at -15 (sigma 3e-7), everything inside [-29, -6.5]
    lo, med, hi = u.min().item(), _quantile(u, 0.5), u.max().item()
    K = min(8.5 / max(hi - med, 1e-30), 14.0 / max(med - lo, 1e-30))
    return K, -15.0 - K * med
  if regime == 'surface':
    # anchor: the larger of the emptiest ray's largest value (the last sample apart: at infinity any density is opaque, and the
    # transmittance never sees it) and the 32 % quantile goes to -17.5 (softplus: sigma 2.5e-8, where 1 - expf(-sigma) is exactly 0; relu: -0.5, sigma 0),
    # so one whole ray and a third of the samples stay empty; K puts the 85 % quantile of (u - anchor) dist at an optical depth of 8
    # and the optical depth of the median ray (the sum of its positive (u - anchor) dist) at 16 or more (T = 1e-7)
    anchor, low = max(u[..., :-1].max(-1).values.min().item(), _quantile(u, 0.32)), -0.5 if relu else -17.5
    tau = (u - anchor) * dist * finite
    ray = tau.clamp(min=0).sum(-1).sort(descending=True).values[(u.shape[0] + 1) // 2 - 1].item()
    K = max(8.0 / max(_quantile(tau[finite], 0.85), 1e-30), 16.0 / max(ray, 1e-30))
    return K, low - K * anchor
  if regime == 'opaque':
    # the 25 % quantile at raw 0; the 40 % quantile of (u - anchor) dist at an optical depth of 6 (alpha 0.9975), and every ray's
    # optical depth (the sum of its positive (u - anchor) dist) at 120 or more: exp(-120) is below float32's smallest denormal
    anchor = _quantile(u, 0.25)
    tau = (u - anchor) * dist * finite
    K = max(6.0 / max(_quantile(tau[finite], 0.40), 1e-30), 120.0 / max(tau.clamp(min=0).sum(-1).min().item(), 1e-30))
    return K, -K * anchor
  raise ValueError(regime)


def density_regime(params, spec, batch, regime, saturated_rgb=False):
  """(tree, stats): `params` (a float64 oracle tree, left untouched) with both levels' density heads rewritten into `regime`, and
  {level: regime_stats} of the result.  The coarse head goes first: the fine depths follow the coarse weights, so the fine head is
  placed on the raw density it has at the depths the rewritten coarse level sends it.  No random numbers are drawn."""
  tree = O.tree_map(lambda t: t.clone(), params)
  d = batch['directions']
  for lv in LEVELS:
    head = _heads(tree, spec, batch)[lv]
    lg = tree[f'nerf_mlps_{lv}']['MLP_2']['logit']
    K, b = _density_head(spec, regime, head, lg['bias'], d)
    lg['kernel'], lg['bias'] = lg['kernel'] * K, torch.full_like(lg['bias'], b)
    if saturated_rgb:   # the 85 % quantile of |raw colour| at 7 (sigmoid within 9e-4 of 0 or 1)
      cg = tree[f'nerf_mlps_{lv}']['MLP_1']['logit']
      k = 7.0 / _quantile(head['rgb'].abs(), 0.85)
      cg['kernel'], cg['bias'] = cg['kernel'] * k, cg['bias'] * k
  heads = _heads(tree, spec, batch)
  stats = {lv: regime_stats(spec, heads[lv], d) for lv in LEVELS}
  assert_regime(spec, regime, stats, saturated_rgb)
  return tree, stats


def assert_regime(spec, regime, stats, saturated_rgb=False):
  """The regime's defining conditions, on the float64 oracle's values."""
  relu = spec.sigma_activation == 'relu'
  for lv in LEVELS:
    s = stats[lv]
    if regime == 'empty':
      assert not relu and -30 <= s['raw_min'] and s['raw_max'] <= -6 and s['sigma_lt_1e6'] >= 0.5, (lv, s)
      assert 9e-14 <= s['sigma_min'] and s['sigma_max'] <= 2.5e-3, (lv, s)
    elif regime == 'surface':
      assert (s['sigma_zero'] if relu else s['sigma_lt_1e4']) >= 0.30 and s['tau_gt_5'] >= 0.10, (lv, s)
      assert s['rays_T_lt_1e3'] >= 0.5 and s['rays_T_gt_half'] >= 1, (lv, s)
    elif regime == 'opaque':
      if lv == 'coarse':
        assert s['alpha_gt_099'] > 0.5, (lv, s)
      assert s['rays_T32_zero'] == 1.0, (lv, s)
    if saturated_rgb:
      assert s['rgb_saturated'] >= 0.10, (lv, s)


def cotangents(spec, nrays, keys, seed):
  """{level: {key: float64 tensor}}: seeded normals in the shapes of NerfModel.apply's outputs."""
  g = torch.Generator().manual_seed(seed)
  S = {'coarse': spec.num_coarse_samples, 'fine': spec.num_coarse_samples + spec.num_fine_samples}
  shape = lambda lv: {'rgb': (nrays, 3), 'depth': (nrays,), 'acc': (nrays,), 'weights': (nrays, S[lv])}
  return {lv: {k: torch.randn(*shape(lv)[k], generator=g, dtype=torch.float64) for k in keys} for lv in LEVELS}


def render_raw(spec, raw4, z, directions):
  """model_utils.py:104-126 behind models.py:276-277 in the dtype of `raw4` (B,S,4) = raw colour, raw density, restated in plain torch
  operations for torch.autograd: softplus differentiates as sigmoid(x); the exclusive cumprod of :112-115 is written as the running
  product it is, so that its reverse pass is the division-free recurrence and not torch.cumprod's own backward formula."""
  rgb, sigma = torch.sigmoid(raw4[..., :3]), O._sigma_act(spec.sigma_activation, raw4[..., 3])
  last = 1e10 if spec.use_sample_at_infinity else 1e-19
  dists = torch.cat([z[..., 1:] - z[..., :-1], torch.full_like(z[..., :1], last)], -1) * torch.linalg.norm(directions[..., None, :], dim=-1)
  alpha = 1.0 - torch.exp(-sigma * dists)
  t = 1.0 - alpha + 1e-10
  T = [torch.ones_like(alpha[..., 0])]
  for i in range(alpha.shape[-1] - 1):
    T.append(T[-1] * t[..., i])
  weights = alpha * torch.stack(T, -1)
  out_rgb = (weights[..., None] * rgb).sum(-2)
  acc = weights.sum(-1)
  if spec.use_white_background:
    out_rgb = out_rgb + (1. - acc[..., None])
  if spec.use_sample_at_infinity:
    acc = weights[..., :-1].sum(-1)
  return {'rgb': out_rgb, 'depth': (weights * z).sum(-1), 'acc': acc, 'weights': weights}


def d_raw_autograd(spec, raw4, z, directions, cot):
  """d <cot, outputs> / d raw4 by torch.autograd over render_raw, in raw4's dtype."""
  x = raw4.detach().clone().requires_grad_(True)
  out = render_raw(spec, x, z.to(x.dtype), directions.to(x.dtype))
  return torch.autograd.grad(sum((out[k] * t.to(x.dtype)).sum() for k, t in cot.items()), x)[0], out


def composite_vjp(spec, out4, z, directions, cot, target=None):
  """float64 compositing of ACTIVATED values out4 (B,S,4) = sigmoid colour, sigma, and its VJP carried to the raw heads through
  derivatives that are functions of the activated values alone: sigmoid' = c (1 - c), softplus' = -expm1(-sigma), relu' =
  [sigma > 0].  `target` (B,3): the rgb cotangent is that of mean((rgb - target)^2).  Returns (outputs, d_raw4)."""
  a = out4.double().detach().clone().requires_grad_(True)
  out = O.volumetric_rendering(a[..., :3], a[..., 3], z.double(), directions.double(), spec.use_white_background,
                               spec.use_sample_at_infinity)
  cot = dict(cot)
  if target is not None:
    cot['rgb'] = 2.0 * (out['rgb'].detach() - target.double()) / target.numel()
  g = torch.autograd.grad(sum((out[k] * t.double()).sum() for k, t in cot.items()), a)[0]
  c, sigma = a.detach()[..., :3], a.detach()[..., 3]
  dact = -torch.expm1(-sigma) if spec.sigma_activation == 'softplus' else (sigma > 0).double()
  return {k: v.detach() for k, v in out.items()}, torch.cat([g[..., :3] * c * (1 - c), (g[..., 3] * dact)[..., None]], -1)


# Behind a hard surface a whole ray's density gradient is a product of exp(-optical depth) factors that float64 still holds (1e-60,
# 1e-150) and no float32 evaluation can (normal floats end at 1.2e-38): with cotangents of order 1, a ray whose largest reference entry
# is below RAY_FLOOR counts as having RAY_FLOOR for its largest entry, which holds the kernel to an absolute 1e-30 there.
RAY_FLOOR = 1e-30
# alpha = 1 - exp(-sigma dist) is a multiple of 2^-24 in float32 (model_utils.py:110 as written), so every weight carries an absolute
# error of up to 2^-24 in any float32 evaluation, the reference's own included, and a colour entry w_i g_k c (1 - c) one of up to
# 2^-24 |g| / 4 <= 2^-24 for cotangents below 4: that much of a colour entry's error is not counted (on a ray through empty space
# without the sample at infinity every weight is below 2^-24 and the whole ray would otherwise be its own rounding error).
COLOUR_ATOL = 2.0 ** -24
EXCLUDE_BELOW = 1e-5   # a density-component element may leave the elementwise criterion only with an error below this x the ray's largest
EXCLUDE_SHARE = 0.02   # ... and at most this share of a case's elements may


def d_raw_errors(got, ref, last_at_infinity=True):
  """got, ref (B,S,4).  Density component: elementwise |delta| / (|ref| + 1e-6 ray max) and the mask of the elements whose error is
  below EXCLUDE_BELOW x the ray's largest density entry; colour components: (|delta| - COLOUR_ATOL)+ over the ray's largest colour
  entry (the reference's own 1 - exp(-sigma dist) has no relative precision, so the weights w_i that scale them have none either).
  `last_at_infinity` (use_sample_at_infinity): dL/dsigma of the last sample carries its distance of 1e10 |d| and would be every ray's
  largest entry by ten orders of magnitude, so the ray max of the other samples is taken without it, and the last sample is held
  against the larger of that and its own magnitude."""
  got, ref = got.double(), ref.double()
  dw, rw = (got[..., 3] - ref[..., 3]).abs(), ref[..., 3].abs()
  wmax = (rw[..., :-1] if last_at_infinity else rw).max(-1, keepdim=True).values.clamp(min=RAY_FLOOR).expand_as(rw).clone()
  wmax[..., -1] = torch.maximum(wmax[..., -1], rw[..., -1])
  w_rel = torch.where(dw == 0, torch.zeros_like(dw), dw / (rw + 1e-6 * wmax))
  dc = ((got[..., :3] - ref[..., :3]).abs().flatten(1).max(-1).values - COLOUR_ATOL).clamp(min=0)
  cmax = ref[..., :3].abs().flatten(1).max(-1).values
  c_ray = torch.where(dc == 0, torch.zeros_like(dc), dc / cmax.clamp(min=1e-300))
  return dict(w_rel=w_rel, w_small=dw < EXCLUDE_BELOW * wmax, w_ray=(dw / wmax).max().item(), c_ray=c_ray.max().item())


def d_raw_summary(got, ref, w_tol, last_at_infinity=True):
  """(worst elementwise density error among the elements held to the criterion, share of excluded elements, worst density error /
  ray max, worst colour error / ray max) -- an element is excluded when it misses `w_tol` with an error below EXCLUDE_BELOW x ray max."""
  e = d_raw_errors(got, ref, last_at_infinity)
  excluded = (e['w_rel'] > w_tol) & e['w_small']
  held = e['w_rel'][~excluded]
  return held.max().item() if held.numel() else 0.0, excluded.sum().item() / float(e['w_rel'].numel()), e['w_ray'], e['c_ray']


# ---- the cases of tests/test_gpu_density_regimes.py, shared with the host test that measures their float32 floor -------------
REGIME_SHAPE = dict(num_coarse_samples=24, num_fine_samples=56, nerf_trunk_width=64, num_nerf_point_freqs=4, use_stratified_sampling=False)
REGIME_SHAPE_3 = dict(REGIME_SHAPE, num_coarse_samples=64, num_fine_samples=128)   # three 64-sample chunks at the fine level
REGIME_SEED = 31
_REGIME_CACHE = {}


def regime_batch(nrays, seed=REGIME_SEED + 1):
  """oracle.synthetic_batch with unit viewdirs and directions of length 1.7: the |d| factor of the distances cannot go missing."""
  b = O.synthetic_batch(nrays, seed=seed, dtype=torch.float64)
  b['viewdirs'] = b['directions'].clone()
  b['directions'] = b['directions'] * 1.7
  return b


def regime_case(regime, act='softplus', white=False, inf=True, sat=False, three=False, alpha_cond=False):
  """(spec, B, float64 tree in `regime`, float64 batch, {level: regime_stats}); B = 7 rays of 24 + 56 samples, or 5 of 64 + 128."""
  key = (regime, act, white, inf, sat, three, alpha_cond)
  if key not in _REGIME_CACHE:
    extra = dict(use_appearance_metadata=True, use_alpha_condition=True) if alpha_cond else {}
    spec = O.ModelSpec(sigma_activation=act, use_white_background=white, use_sample_at_infinity=inf,
                       **(REGIME_SHAPE_3 if three else REGIME_SHAPE), **extra)
    B = 5 if three else 7
    p64 = O.init_params(spec, seed=REGIME_SEED, trained_like=True, dtype=torch.float64)
    b64 = regime_batch(B)
    if regime == 'stock':
      heads = _heads(p64, spec, b64)
      tree, stats = p64, {lv: regime_stats(spec, heads[lv], b64['directions']) for lv in LEVELS}
    else:
      tree, stats = density_regime(p64, spec, b64, regime, saturated_rgb=sat)
    _REGIME_CACHE[key] = (spec, B, tree, b64, stats)
  return _REGIME_CACHE[key]


# (id, regime_case arguments, mode).  Modes: 'plain' nrf_backward with rgb cotangents (composite_bwd_kernel<false, false>), 'extra'
# nrf_backward_ex with rgb, depth, acc and weights cotangents (<true, false>), 'rays' / 'rays_extra' nrf_backward_rays (<false, true> /
# <true, true>), 'loss' nrf_train_step_loss_grad (d_rgb == NULL, the target from the batch), 'bf16' the extra case under NRF_FLAG_BF16.
D_RAW_CASES = [
    ('empty-softplus-plain', dict(regime='empty'), 'plain'),
    ('empty-softplus-extra', dict(regime='empty'), 'extra'),
    ('empty-softplus-loss', dict(regime='empty'), 'loss'),
    ('surface-softplus-plain', dict(regime='surface'), 'plain'),
    ('surface-softplus-extra', dict(regime='surface'), 'extra'),
    ('surface-softplus-white', dict(regime='surface', white=True), 'extra'),
    ('surface-softplus-noinf', dict(regime='surface', inf=False), 'extra'),
    ('surface-softplus-white-noinf', dict(regime='surface', white=True, inf=False), 'extra'),
    ('surface-softplus-saturated', dict(regime='surface', sat=True), 'extra'),
    ('surface-softplus-rays-extra', dict(regime='surface'), 'rays_extra'),
    ('surface-softplus-loss', dict(regime='surface'), 'loss'),
    ('surface-softplus-bf16', dict(regime='surface'), 'bf16'),
    ('surface-softplus-three-chunks', dict(regime='surface', three=True), 'extra'),
    ('surface-relu-extra', dict(regime='surface', act='relu'), 'extra'),
    ('surface-relu-white-noinf', dict(regime='surface', act='relu', white=True, inf=False), 'extra'),
    ('opaque-softplus-extra', dict(regime='opaque'), 'extra'),
    ('opaque-relu-extra', dict(regime='opaque', act='relu'), 'extra'),
    ('opaque-relu-saturated-plain', dict(regime='opaque', act='relu', sat=True), 'plain'),
    ('opaque-relu-rays', dict(regime='opaque', act='relu'), 'rays'),
]


def case_cotangents(spec, B, mode):
  return cotangents(spec, B, ('rgb',) if mode in ('plain', 'rays', 'loss') else OUTPUTS, seed=5)


# The float32 floor of d raw per regime: the worst figures of tests/test_density_regimes_host.py::test_float32_floor_of_d_raw over the
# regime's cases and both levels (the colour floor: over all regimes; plain float32 torch autograd of compositing + activations against the same in float64; the
# figures per case are in profiles/density_regimes.md), rounded up.  w_rel: density component, elementwise |delta| / (|ref| + 1e-6 ray
# max); w_ray / c_ray: density / colour error over the ray's largest entry.  The GPU tolerances are 4 x the floor: a different but
# equally valid order of the float32 sums and products, as for grad_tol.
D_RAW_FLOOR = {
    'empty': dict(w_rel=7.7e-3, w_ray=1.4e-4, c_ray=4.0e-7),
    # behind a sample with sigma dist in (16.6, 23) alpha rounds to 1 and t = 1 - alpha + 1e-10 is 1e-10 instead of up to 6e-8 (the
    # reference's own float32 formula), so everything further along the ray is off by that factor: elementwise the density floor is
    # 0.3 and says little there; the error over the ray's largest entry is what holds the kernel in this regime
    'surface': dict(w_rel=0.31, w_ray=6.3e-4, c_ray=4.0e-7),
    'opaque': dict(w_rel=9.1e-2, w_ray=6.8e-4, c_ray=4.0e-7),
}
D_RAW_TOL = {r: {k: 4.0 * v for k, v in f.items()} for r, f in D_RAW_FLOOR.items()}


def assert_d_raw(got, ref, regime, label, last_at_infinity=True):
  """d raw (B,S,4) of the HIP path against the float64 VJP `ref` at D_RAW_TOL[regime]; returns the figures."""
  tol = D_RAW_TOL[regime]
  held, share, w_ray, c_ray = d_raw_summary(got, ref, tol['w_rel'], last_at_infinity)
  worst = d_raw_errors(got, ref, last_at_infinity)['w_rel'].max().item()
  print(f'[{label}] density: elementwise worst {worst:.2e} (held to the criterion: {held:.2e}, tolerance {tol["w_rel"]:.1e}; excluded '
        f'{share:.4f}), / ray max {w_ray:.2e} (tolerance {tol["w_ray"]:.1e}); colour / ray max {c_ray:.2e} (tolerance {tol["c_ray"]:.1e})')
  assert torch.isfinite(got).all(), label
  assert held <= tol['w_rel'] and share <= EXCLUDE_SHARE, (label, held, share)
  assert w_ray <= tol['w_ray'], (label, w_ray)
  assert c_ray <= tol['c_ray'], (label, c_ray)
  return dict(w_rel=worst, held=held, excluded=share, w_ray=w_ray, c_ray=c_ray)


# ---------------------------------------------------------------------------------------------
# Rotation regimes (tests/test_se3_regimes_host.py, tests/test_gpu_se3_regimes.py, profiles/se3_regimes.md)
#
# oracle.init_params(trained_like=True) draws the SE3 heads from U[0, 0.3): one unexamined distribution of the rotation angle
# theta = |w|.  A regime rewrites warp_field/branches_w/logit (kernel x K, a new bias) so that chosen statistics of theta, measured on
# the float64 oracle over the batch's sample points (both levels), land at chosen values, and scales branches_v so that the median |v|
# is 0.05 (a capture's deformations, tests/test_gpu_bf16_warp.py).  With u the head's bias-free output minus its mean over the rows and
# m the direction of that mean, the new head is w = K u + beta m: beta places theta, K spreads it.
# ---------------------------------------------------------------------------------------------
ROTATION_REGIMES = ('init', 'tiny', 'seam', 'trained', 'large')
ROTATION_SHAPE = dict(REGIME_SHAPE, use_warp=True, num_warp_freqs=4, num_warp_features=8)
ROTATION_SHAPE_3 = dict(REGIME_SHAPE_3, use_warp=True, num_warp_freqs=4, num_warp_features=8)
ROTATION_ALPHA = 2.5
V_MEDIAN = 0.05
_ROTATION_CACHE = {}


def _warp_heads(params, spec, batch, alpha=ROTATION_ALPHA):
  """One float64 oracle evaluation: {level: dict(w (rows,3), v (rows,3))}, the SE3 heads' outputs at the level's sample points."""
  wf = params['warp_field']
  key = {id(wf['branches_w']['logit']): 'w', id(wf['branches_v']['logit']): 'v'}
  seen = {'w': [], 'v': []}

  def hook(p, x):
    y = x @ p['kernel'] + p['bias']
    if id(p) in key:
      seen[key[id(p)]].append(y.detach().reshape(-1, 3))
    return y
  with torch.no_grad(), O.dense_hook(hook):
    O.nerf_model_apply(params, spec, batch, warp_alpha=alpha)
  assert len(seen['w']) == 2 and len(seen['v']) == 2   # the coarse pass, then the fine pass
  return {lv: dict(w=seen['w'][i], v=seen['v'][i]) for i, lv in enumerate(LEVELS)}


def rotation_stats(heads):
  """What the regime conditions are stated on: per level, quantiles and shares of theta = |w| over ALL of the level's rows."""
  out = {}
  for lv, h in heads.items():
    th = torch.linalg.norm(h['w'], dim=-1)
    t2 = th * th
    n = float(th.numel())
    share = lambda m: m.sum().item() / n
    out[lv] = dict(
        rows=int(n), min=th.min().item(), q10=_quantile(th, 0.10), median=_quantile(th, 0.5), q90=_quantile(th, 0.90), max=th.max().item(),
        v_median=_quantile(torch.linalg.norm(h['v'], dim=-1), 0.5),
        init_band=share((th > 1e-6) & (th < 1e-2)), below_015=share(th < 0.15),
        seam_below=share((t2 >= 0.0256) & (t2 < 0.04)), seam_above=share((t2 >= 0.04) & (t2 <= 0.0625)),
        seam_rest_ok=share(((t2 >= 0.0256) & (t2 <= 0.0625)) | ((t2 >= 0.01) & (t2 <= 0.09))),
        below_pi=share(th < np.pi), above_pi=share(th > np.pi))
  return out


# (location statistic, its target, spread statistic, its target) of theta per regime
_ROTATION_TARGETS = {
    'tiny': (lambda t: _quantile(t, 0.5), 0.03, lambda t: _quantile(t, 0.95) - _quantile(t, 0.5), 0.06),
    'seam': (lambda t: _quantile(t, 0.5), 0.2, lambda t: (t - _quantile(t, 0.5)).abs().max().item(), 0.035),
    'trained': (lambda t: _quantile(t, 0.5), 0.6, lambda t: _quantile(t, 0.9) - _quantile(t, 0.1), 0.7),
    'large': (lambda t: _quantile(t, 0.5), np.pi, lambda t: t.max().item() - _quantile(t, 0.5), 7.1 - np.pi),
}


def rotation_regime(params, spec, batch, regime):
  """(tree, stats): `params` (a float64 oracle tree, left untouched) with the SE3 heads rewritten into `regime`, and rotation_stats of
  the result.  'init' takes the tree as it is (the caller passes the reference initialisation).  No random numbers are drawn."""
  tree = O.tree_map(lambda t: t.clone(), params)
  if regime != 'init':
    loc, t_loc, spread, t_spread = _ROTATION_TARGETS[regime]
    for _ in range(2):   # the fine depths follow the coarse weights, which follow the warp: place, re-measure, place again
      wl, vl = tree['warp_field']['branches_w']['logit'], tree['warp_field']['branches_v']['logit']
      heads = _warp_heads(tree, spec, batch)
      w = torch.cat([heads[lv]['w'] for lv in LEVELS]) - wl['bias']
      mean = w.mean(0)
      m, u = mean / mean.norm(), w - mean
      K, beta = t_spread / max(spread(u @ m), 1e-30), t_loc
      for _ in range(50):
        th = torch.linalg.norm(K * u + beta * m, dim=-1)
        K, beta = K * t_spread / max(spread(th), 1e-30), beta + t_loc - loc(th)
      # w = K (kernel^T h - mean) + beta m
      wl['kernel'], wl['bias'] = wl['kernel'] * K, beta * m - K * mean
      kv = V_MEDIAN / _quantile(torch.linalg.norm(torch.cat([heads[lv]['v'] for lv in LEVELS]), dim=-1), 0.5)
      vl['kernel'], vl['bias'] = vl['kernel'] * kv, vl['bias'] * kv
  stats = rotation_stats(_warp_heads(tree, spec, batch))
  assert_rotation_regime(regime, stats)
  return tree, stats


def assert_rotation_regime(regime, stats):
  """The regime's defining conditions on theta, per level, over all of the level's rows (none excluded)."""
  for lv in LEVELS:
    s = stats[lv]
    if regime == 'init':
      assert s['init_band'] >= 0.90, (lv, s)
    elif regime == 'tiny':
      assert 0.01 <= s['median'] <= 0.05 and s['below_015'] >= 0.95, (lv, s)
    elif regime == 'seam':
      assert s['seam_below'] >= 0.30 and s['seam_above'] >= 0.30 and s['seam_rest_ok'] == 1.0, (lv, s)
    elif regime == 'trained':
      assert 0.2 <= s['q10'] and s['q90'] <= 1.2, (lv, s)
    elif regime == 'large':
      assert s['below_pi'] >= 0.20 and s['above_pi'] >= 0.20 and 2 * np.pi <= max(stats[l]['max'] for l in LEVELS) <= 8.0, (lv, s)
      assert s['max'] <= 8.0, (lv, s)
    else:
      raise ValueError(regime)
    if regime != 'init':
      assert 0.03 <= s['v_median'] <= 0.08, (lv, s)


def rotation_case(regime, three=False):
  """(spec, B, float64 tree in `regime`, float64 batch, {level: rotation_stats}); B = 7 rays of 24 + 56 samples, or 5 of 64 + 128."""
  key = (regime, three)
  if key not in _ROTATION_CACHE:
    spec = O.ModelSpec(sigma_activation='softplus', **(ROTATION_SHAPE_3 if three else ROTATION_SHAPE))
    B = 5 if three else 7
    p64 = O.init_params(spec, seed=REGIME_SEED, trained_like=regime != 'init', dtype=torch.float64)
    b64 = regime_batch(B)
    tree, stats = rotation_regime(p64, spec, b64, regime)
    _ROTATION_CACHE[key] = (spec, B, tree, b64, stats)
  return _ROTATION_CACHE[key]
