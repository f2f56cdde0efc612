"""Host-side mirror of nerfies.evaluation.render_image (reference: nerfies/evaluation.py:28-101)."""
import ctypes as C
import math
from typing import Any, Callable, Dict, Optional

import torch
import torch.distributed as dist

from nerfies_amd import lib as L
from nerfies_amd.models import _stream_arg, grid_chunks  # noqa: F401 (grid_chunks is public here as well)


def _tree_map(fn, tree):
  if isinstance(tree, dict):
    return {k: _tree_map(fn, v) for k, v in tree.items()}
  return fn(tree)


class GraphedChunkRenderer:
  """One fixed-size chunk of NerfModel.apply captured in a hipGraph (torch.cuda.CUDAGraph over the
  library's launches on the capture stream) and replayed per chunk: the eval forward is ~20 kernel
  launches of a few hundred microseconds at 8k rays, so launch gaps matter (BASELINE config E).

  model_fn-compatible: `renderer(key_0, key_1, params, rays_dict, warp_extra)`; rays are copied into
  static buffers, the graph is replayed and copies of the static outputs are returned.
  One graph per (chunk size, parameter buffer, warp_alpha, time_alpha, metadata keys) is kept -- the two step scalars are
  by-value kernel arguments baked into the captured launches -- so a frame whose last chunk is
  shorter replays two graphs instead of re-capturing twice per frame; render_image additionally edge-pads the tail to
  the full chunk when the renderer asks for it (`wants_fixed_chunks`), so that one graph serves the whole frame."""
  wants_fixed_chunks = True
  MAX_GRAPHS = 8
  # what NerfModel.apply reads of a ray tree (models.py:289-375).  Dataset items also carry 'rgb' / 'pixels' / 'depth'
  # (datasets.item_rays) while camera-path frames do not (rays_from_camera): only the consumed keys are captured and copied, so
  # one renderer serves both kinds of frame (eval.py renders val / train items and then test cameras through the same one)
  CONSUMED = ('origins', 'directions', 'viewdirs', 'metadata')

  def __init__(self, model, use_warp=True, bf16=False):
    self.model = model
    self.use_warp = use_warp
    self.bf16 = bf16   # NRF_FLAG_BF16 inference mode (bfloat16 MLP operands)
    # key -> (graph, static inputs, static outputs, the call's CallRecord: its workspace lives as long as the graph that points into it)
    self._slots = {}   # insertion-ordered, oldest evicted
    self._generation = model.generation   # the model's workspace generation the slots were captured under
    self.captures = 0

  def _capture(self, fp, rays, warp_extra):
    model = self.model
    ins = _tree_map(lambda x: x.clone(), rays)
    call = lambda out=None: model.apply({'params': fp}, ins, warp_extra, use_warp=self.use_warp, out=out, bf16=self.bf16)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
      outs = call()               # warm-up: uploads the descriptor tables (not capturable), sizes the workspace
      call(outs)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
      call(outs)
    self.captures += 1
    return graph, ins, outs, model.last_call

  def __call__(self, key_0, key_1, params, rays, warp_extra):
    # the static buffers are overwritten by the next replay: a plain model_fn caller gets copies
    return _tree_map(lambda x: x.clone(), self.call_static(key_0, key_1, params, rays, warp_extra))

  def call_static(self, key_0, key_1, params, rays, warp_extra):
    """As __call__, but returns the graph's own output buffers (valid until the next replay): render_image copies each chunk
    straight into the frame at its offset, so a chunk's outputs are moved once instead of cloned and then concatenated."""
    del key_0, key_1               # eval is deterministic (eval.py:239 forces use_stratified_sampling off)
    rays = {k: rays[k] for k in self.CONSUMED if rays.get(k) is not None}
    n = rays['origins'].shape[0]
    # every scalar of lib.StepScalars is part of the key: a replay would otherwise render with the captured value
    scalars = tuple(float((warp_extra or {}).get(k, 0.0)) for k in ('alpha', 'time_alpha'))
    key = (n, params.flat.data_ptr(), scalars, 'viewdirs' in rays, tuple(sorted((rays.get('metadata') or {}).keys())))
    if self._generation != self.model.generation:   # a workspace option replaced the plans: every captured one is stale
      self._slots.clear()
      self._generation = self.model.generation
    slot = self._slots.get(key)
    if slot is None:
      # every chunk size has its own workspace (descriptor tables included), so graphs of different sizes coexist
      while len(self._slots) >= self.MAX_GRAPHS:
        del self._slots[next(iter(self._slots))]
      slot = self._slots[key] = self._capture(params, rays, warp_extra)
    else:
      def cp(dst, src):
        if isinstance(dst, dict):
          for k in dst:
            cp(dst[k], src[k])
        else:
          dst.copy_(src)
      _check_same_tree(slot[1], rays)   # same keys / shapes / dtypes as the captured chunk, or a clear NrfError
      cp(slot[1], rays)
    slot[0].replay()
    return slot[2]


def _check_same_tree(dst, src, path='rays'):
  """The replay path copies new rays into the captured static buffers: same keys, same shapes, same dtypes -- or a clear error
  (a missing sub-dict used to surface as a TypeError on None)."""
  if isinstance(dst, dict):
    if not isinstance(src, dict) or set(dst) != set(src):
      have = sorted(src) if isinstance(src, dict) else type(src).__name__
      raise L.NrfError(f'GraphedChunkRenderer: {path} has keys {have}, the captured chunk had {sorted(dst)}; render with the same '
                       'ray tree or use a new renderer')
    for k in dst:
      _check_same_tree(dst[k], src[k], f'{path}/{k}')
  elif tuple(dst.shape) != tuple(src.shape) or dst.dtype != src.dtype:
    raise L.NrfError(f'GraphedChunkRenderer: {path} is {tuple(src.shape)} {src.dtype}, the captured chunk had {tuple(dst.shape)} {dst.dtype}')


def _all_gather_rows(gathered, packed):
  """dist.all_gather_into_tensor of a rank's packed rows.  RCCL (backend 'nccl') is a stream operation and takes the device
  buffers as they are.  gloo -- the transport of the tests that put several ranks on ONE GPU -- is a host collective: staged
  through host tensors explicitly (the device-to-host copy is the synchronisation point), so that it never reads a device buffer
  the stream has not finished writing."""
  if packed.is_cuda and dist.get_backend() != 'nccl':
    host = torch.empty(gathered.shape, dtype=gathered.dtype)
    dist.all_gather_into_tensor(host, packed.cpu())
    gathered.copy_(host)
  else:
    dist.all_gather_into_tensor(gathered, packed)


def _pack(ret, rows):
  """Every output key of a rendered chunk side by side in one (rows, sum of widths) float32 buffer: one collective carries all."""
  keys = list(ret.keys())
  cols = [ret[k].reshape(rows, -1).to(torch.float32) for k in keys]
  return keys, cols, [c.shape[1] for c in cols]


def render_image(state, rays_dict: Dict[str, Any], model_fn: Callable, device_count: int = 1, rng=0,
                 chunk: int = 8192, default_ret_key: Optional[str] = None, tile_parallel: str = 'band'):
  """Renders all pixels of an (H,W) ray image in chunks (evaluation.py:62-99).

  model_fn(key_0, key_1, params, chunk_rays_dict, warp_extra) -> {'coarse': {...}, 'fine': {...}}.
  With torch.distributed initialised the frame is split over the ranks (image tiles are disjoint: no reduction, the
  reference all_gathers and keeps replica 0, eval.py:339, evaluation.py:92):
    tile_parallel='band' (default): every rank renders a contiguous BAND of whole chunks -- full-size launches, the shape the
      kernels are tuned for -- into a band buffer, and ONE all_gather per frame assembles it (BASELINE configs[4]: "8-GPU
      image-tile parallel");
    tile_parallel='chunk': the reference's own order -- every chunk is cut `world` ways (evaluation.py:61-92), one packed
      all_gather per chunk (64 latency-bound collectives and 1/world-size launches for a 960x540 frame on 8 GPUs).
  Both give the single-rank frame bit for bit (rows are rendered independently of their position in a launch).  The last
  chunk is edge-padded (evaluation.py:71-78): to the full chunk for a graph-replaying renderer, to a multiple of the world
  size in 'chunk' mode."""
  if tile_parallel not in ('band', 'chunk'):
    raise ValueError("tile_parallel must be 'band' or 'chunk'")
  h, w = rays_dict['origins'].shape[:2]
  flat = _tree_map(lambda x: x.reshape(h * w, -1), rays_dict)
  num_rays = h * w
  dist_on = dist.is_available() and dist.is_initialized()   # a one-rank communicator still runs the gather (RCCL on the GPU)
  world = dist.get_world_size() if dist_on else 1
  rank = dist.get_rank() if world > 1 else 0
  del device_count
  call = getattr(model_fn, 'call_static', model_fn)   # a graph renderer hands out its static output buffers (no per-chunk clone)
  num_chunks = int(math.ceil(num_rays / chunk))
  # a graph-replaying renderer wants ONE chunk size per frame: the tail is edge-padded to the full chunk (rendered and
  # dropped) instead of being a second shape; otherwise it is padded to a multiple of the world size only
  fixed = bool(getattr(model_fn, 'wants_fixed_chunks', False)) and num_chunks > 1

  def padded_chunk(batch_idx, multiple):
    i0 = batch_idx * chunk
    rays = _tree_map(lambda x: x[i0:i0 + chunk], flat)
    n = rays['origins'].shape[0]
    full = -(-chunk // multiple) * multiple if fixed else n
    pad = max(full - n, 0) + (multiple - max(full, n) % multiple) % multiple
    if pad:
      rays = _tree_map(lambda x: torch.cat([x, x[-1:].expand(pad, *x.shape[1:])], 0), rays)
    return i0, n, n + pad, rays

  if dist_on and tile_parallel == 'band':
    # balanced bands: rank r renders base (+ 1 for the first `rem` ranks) whole chunks starting at r * base + min(r, rem) --
    # 9 chunks on 8 ranks are 2 + 1 x 7, not 2 x 4 + 1 + 0 x 3.  all_gather wants equal pieces, so every band buffer holds
    # cmax chunks and the frame is assembled from each rank's leading rows
    base, rem = divmod(num_chunks, world)
    cmax = base + (1 if rem else 0)
    first = lambda r: r * base + min(r, rem)
    count = lambda r: base + (1 if r < rem else 0)
    band_rows = cmax * chunk
    band, meta = None, None
    for c in range(first(rank), first(rank) + count(rank)):
      i0, n, _, rays = padded_chunk(c, 1)
      out = call(rng, rng + 1, state.optimizer.target, rays, state.warp_extra)
      ret = out[default_ret_key or ('fine' if 'fine' in out else 'coarse')]
      keys, cols, widths = _pack(ret, rays['origins'].shape[0])
      if band is None:
        band = torch.zeros(band_rows, sum(widths), dtype=torch.float32, device=cols[0].device)
        meta = (keys, widths, [tuple(ret[k].shape[1:]) for k in keys], [ret[k].dtype for k in keys])
      at, col = i0 - first(rank) * chunk, 0
      for cdata, wd in zip(cols, widths):
        band[at:at + n, col:col + wd].copy_(cdata[:n])
        col += wd
    # only when there are more ranks than chunks does a rank own none; it then learns the output layout from rank 0 (every rank
    # sees base == 0 locally, so all of them join this broadcast or none does).  Otherwise: ONE collective per frame.
    if world > 1 and base == 0:
      lay = [meta]
      dist.broadcast_object_list(lay, src=0)
      meta = lay[0]
    keys, widths, shapes, dtypes = meta
    if band is None:
      band = torch.zeros(band_rows, sum(widths), dtype=torch.float32, device=flat['origins'].device)
    gathered = torch.empty(world * band_rows, band.shape[1], dtype=band.dtype, device=band.device)
    _all_gather_rows(gathered, band)     # ONE collective per frame
    if rem:   # bands of unequal length: keep each rank's leading count(r) chunks
      gathered = torch.cat([gathered[r * band_rows:r * band_rows + count(r) * chunk] for r in range(world) if count(r)], 0)
    split = torch.split(gathered[:num_rays], widths, 1)
    return {k: split[i].reshape(h, w, *shapes[i]).to(dtypes[i]) for i, k in enumerate(keys)}

  frame = None          # output key -> (num_rays, ...) buffer, filled chunk by chunk at the chunk's offset
  for batch_idx in range(num_chunks):
    i0, n, total, chunk_rays = padded_chunk(batch_idx, world)
    per = total // world
    mine = _tree_map(lambda x: x[rank * per:(rank + 1) * per], chunk_rays) if world > 1 else chunk_rays
    out = call(rng, rng + 1, state.optimizer.target, mine, state.warp_extra)
    ret_key = default_ret_key or ('fine' if 'fine' in out else 'coarse')
    ret = out[ret_key]
    if dist_on:   # ONE all_gather per chunk: every output key packed side by side into a (per, sum of widths) buffer
      keys, cols, widths = _pack(ret, per)
      packed = torch.cat(cols, 1).contiguous()
      gathered = torch.empty(world * per, packed.shape[1], dtype=packed.dtype, device=packed.device)
      _all_gather_rows(gathered, packed)
      split = torch.split(gathered, widths, 1)
      ret = {k: split[i].reshape(world * per, *ret[k].shape[1:]).to(ret[k].dtype) for i, k in enumerate(keys)}
    if frame is None:
      frame = {k: torch.empty(num_rays, *v.shape[1:], dtype=v.dtype, device=v.device) for k, v in ret.items()}
    for k, v in ret.items():
      frame[k][i0:i0 + n].copy_(v[:n])     # drops the padding; the only copy a chunk's outputs see
  return {k: v.reshape(h, w, *v.shape[1:]) for k, v in frame.items()}


def rays_from_camera(camera, metadata: Optional[Dict[str, int]] = None, device='cuda'):
  """One dataset item for a camera, built on the GPU: what datasets/core.py:163-190 (_camera_to_rays_fn +
  _tf_broadcast_metadata_fn) assembles on the host -- origins / directions / pixels [H, W, .] and every metadata id
  ('warp', 'appearance', 'camera') broadcast to [H, W, 1] int32."""
  rays = camera.to_rays(device)
  h, w = rays['origins'].shape[:2]
  if metadata:   # ids are int32 table rows; 'time' is the float stamp of the TimeEncoder (core.py:508-509, 602-603)
    dev = rays['origins'].device
    rays['metadata'] = {k: (torch.full((h, w, 1), float(v), dtype=torch.float32, device=dev) if k == 'time' else
                            torch.full((h, w, 1), int(v), dtype=torch.int32, device=dev)) for k, v in metadata.items()}
  return rays


def _box_grid(bbox_min, bbox_max, resolution):
  """(res, origin, step): `resolution` voxels per axis (an int, or (X, Y, Z)) over the box, sampled at the voxel centres."""
  res = (int(resolution),) * 3 if isinstance(resolution, int) else tuple(int(r) for r in resolution)
  if len(res) != 3 or min(res) <= 0:
    raise ValueError(f'resolution must be a positive int or (X, Y, Z), got {resolution!r}')
  lo = [float(v) for v in bbox_min]
  hi = [float(v) for v in bbox_max]
  step = [(h - l) / r for l, h, r in zip(lo, hi, res)]
  origin = [l + 0.5 * s for l, s in zip(lo, step)]
  return res, origin, step


def _one_group_metadata(warp_id, appearance_id, camera_id, device):
  """The metadata of ONE group (one condition for a whole grid, or for every vertex of a mesh): a (1, 1) id row per id given."""
  ids = dict(warp=warp_id, appearance=appearance_id, camera=camera_id)
  return {k: torch.tensor([[int(v)]], dtype=torch.int32, device=device) for k, v in ids.items() if v is not None}


def _walk_grid(query, widths, cap, params, bbox_min, bbox_max, resolution, level, warp_id, appearance_id, warp_extra, chunk, device):
  """The grid entry `query` (NerfModel.query_grid or .query_grid_gradient) over the voxel centres of the box, `chunk` (at most `cap`)
  points per call through one workspace: {name: (X, Y, Z, *widths[name]) float32 device tensor, x fastest in memory}."""
  res, origin, step = _box_grid(bbox_min, bbox_max, resolution)
  if device is None:
    device = params.flat.device if hasattr(params, 'flat') else 'cuda'
  metadata = _one_group_metadata(warp_id, appearance_id, None, device)
  total = res[0] * res[1] * res[2]
  chunk = max(1, min(int(chunk), total, cap))
  flat = {k: torch.empty(total, *w, dtype=torch.float32, device=device) for k, w in widths.items()}
  for first, count in grid_chunks(total, chunk):
    query(params, origin, step, res, first, count, {k: v[first:first + count] for k, v in flat.items()}, metadata=metadata,
          warp_extra=warp_extra, level=level, use_warp=warp_id is not None, workspace_points=chunk)
  return {k: flat[k].view(res[2], res[1], res[0], *w).permute(2, 1, 0, *range(3, 3 + len(w))) for k, w in widths.items()}


def density_grid(model, params, bbox_min, bbox_max, resolution, level='fine', warp_id=None, appearance_id=None, warp_extra=None,
                 chunk=1 << 21, device=None):
  """Activated density of the field on a regular grid over the box [bbox_min, bbox_max]: an (X, Y, Z) float32 device tensor, `x`
  fastest in memory, sampled at the voxel centres.  `resolution`: voxels per axis (an int, or (X, Y, Z)).  `warp_id=None` queries the
  canonical (template) volume (NRF_FLAG_NO_WARP); an id queries that frame's observation volume through the warp field.
  `appearance_id`: the appearance code of a use_alpha_condition model (its density depends on it).  The points are formed on the
  device by nrf_query_grid, `chunk` of them per call through one workspace; the density-only kernel runs (no colour is computed)."""
  return _walk_grid(model.query_grid, {'sigma': ()}, 1 << 24, params, bbox_min, bbox_max, resolution, level, warp_id, appearance_id,
                    warp_extra, chunk, device)['sigma']


def normal_grid(model, params, bbox_min, bbox_max, resolution, level='fine', warp_id=None, appearance_id=None, warp_extra=None,
                chunk=1 << 20, device=None):
  """Density and surface normals -grad sigma / |grad sigma| on the grid of `density_grid` (same box, voxel centres, memory order and
  arguments): (sigma (X, Y, Z), normals (X, Y, Z, 3)), float32 device tensors.  A normal is exactly 0 where the gradient vanishes.
  With a `warp_id` the gradient is taken with respect to the observation-space point, through the warp field.  The points are formed
  on the device by nrf_query_grid_grad, `chunk` (at most NRF_QUERY_GRAD_MAX_POINTS) of them per call through one workspace."""
  out = _walk_grid(model.query_grid_gradient, {'sigma': (), 'normals': (3,)}, L.NRF_QUERY_GRAD_MAX_POINTS, params, bbox_min, bbox_max,
                   resolution, level, warp_id, appearance_id, warp_extra, chunk, device)
  return out['sigma'], out['normals']


MESH_VIEW_DIRECTION = (0.0, 0.0, 1.0)   # the direction every exported colour is queried along


def _mesh_grid(sigma, origin, step):
  """(the x-fastest flat view of an (X, Y, Z) density tensor, its nrf_grid)."""
  if sigma.dim() != 3 or sigma.dtype != torch.float32:
    raise ValueError(f'sigma must be a float32 (X, Y, Z) tensor, got {sigma.dtype} {tuple(sigma.shape)}')
  flat = sigma.permute(2, 1, 0).contiguous().reshape(-1)   # no copy for a tensor laid out as density_grid returns it
  return flat, L.grid(origin, step, sigma.shape)


def extract_mesh_from_grid(sigma, origin, step, threshold, lib=None):
  """Surface nets of a density grid from anywhere (nrf_mesh_count, then nrf_mesh_emit; the definition is in
  include/nerfies_amd.h): `sigma` is a float32 (X, Y, Z) device tensor whose sample (i, j, k) sits at origin + idx * step (the
  memory order of `density_grid` is used as it is; any other is copied once).  A sample is inside iff sigma > threshold.  Returns
  device tensors {'vertices' (V, 3) float32, 'vertex_cell' (V,) int32, 'faces' (F, 3) int32}: one vertex per active cell, shared by
  its faces, counter-clockwise faces whose normals point from high density to low, the same bits on every run.  The two counts are
  read back once, to size the outputs; an empty mesh is (0, 3) tensors."""
  lib = lib or L.load_library()
  flat, grid = _mesh_grid(sigma, origin, step)
  device = flat.device
  stream = _stream_arg(device)
  nbytes = C.c_size_t(0)
  L.check(lib.nrf_mesh_workspace_bytes(C.byref(grid), C.byref(nbytes)), lib)
  ws = torch.empty((nbytes.value + 3) // 4, dtype=torch.int32, device=device)
  counts = torch.zeros(2, dtype=torch.int32, device=device)
  L.check(lib.nrf_mesh_count(flat.data_ptr(), C.byref(grid), float(threshold), counts.data_ptr(), ws.data_ptr(), ws.numel() * 4, stream), lib)
  nv, nt = (int(v) for v in counts.tolist())
  vertices = torch.empty(nv, 3, dtype=torch.float32, device=device)
  vertex_cell = torch.empty(nv, dtype=torch.int32, device=device)
  faces = torch.empty(nt, 3, dtype=torch.int32, device=device)
  ptr = lambda t: t.data_ptr() if t.numel() else None
  L.check(lib.nrf_mesh_emit(flat.data_ptr(), C.byref(grid), float(threshold), nv, nt, ptr(vertices), ptr(vertex_cell), ptr(faces),
                            ws.data_ptr(), ws.numel() * 4, stream), lib)
  return {'vertices': vertices, 'vertex_cell': vertex_cell, 'faces': faces}


def _mesh_workspace(lib, sizer, num_vertices, num_triangles, device):
  nbytes = C.c_size_t(0)
  L.check(sizer(num_vertices, num_triangles, C.byref(nbytes)), lib)
  return torch.empty((nbytes.value + 3) // 4, dtype=torch.int32, device=device)


def _faces_arg(faces):
  faces = torch.as_tensor(faces)
  if faces.dtype != torch.int32 or faces.dim() != 2 or faces.shape[1] != 3:
    raise ValueError(f'faces must be an (F, 3) int32 tensor, got {faces.dtype} {tuple(faces.shape)}')
  return faces.contiguous()


def mesh_components(vertices, faces, lib=None, num_vertices=None):
  """Connected components of an indexed triangle mesh on the device (nrf_mesh_components, then nrf_mesh_component_table; the
  definitions are in include/nerfies_amd.h): `faces` (F, 3) int32 of any mesh in any order, `vertices` (V, 3) float32, or None to
  skip the boxes (then V is `num_vertices`, or by default one more than the largest index of `faces`).  A triangle with an index
  outside [0, V) joins nothing; a vertex no triangle names is a component of its own; ids are dense in increasing order of each
  component's smallest vertex.  Returns device tensors {'labels' (V,) int32, 'num_vertices' (C,) int32, 'num_triangles' (C,) int32
  (a triangle counts for its first index's component), and with vertices 'bbox_min' (C, 3), 'bbox_max' (C, 3) float32}, the same
  bits on every run.  C is read back once, to size the table."""
  lib = lib or L.load_library()
  faces = _faces_arg(faces)
  device = faces.device
  if vertices is not None:
    vertices = torch.as_tensor(vertices)
    if vertices.dtype != torch.float32 or vertices.dim() != 2 or vertices.shape[1] != 3:
      raise ValueError(f'vertices must be a (V, 3) float32 tensor, got {vertices.dtype} {tuple(vertices.shape)}')
    vertices = vertices.contiguous()
    if num_vertices is not None and int(num_vertices) != vertices.shape[0]:
      raise ValueError(f'num_vertices = {num_vertices} but vertices has {vertices.shape[0]} rows')
    V = vertices.shape[0]
  elif num_vertices is not None:
    V = int(num_vertices)
  else:
    V = int(faces.max()) + 1 if faces.numel() else 0
  F = faces.shape[0]
  stream = _stream_arg(device)
  ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None
  ws = _mesh_workspace(lib, lib.nrf_mesh_components_workspace_bytes, V, F, device)
  labels = torch.empty(V, dtype=torch.int32, device=device)
  count = torch.zeros(1, dtype=torch.int32, device=device)
  L.check(lib.nrf_mesh_components(ptr(faces), F, V, ptr(labels), count.data_ptr(), ws.data_ptr(), ws.numel() * 4, stream), lib)
  nc = int(count.item())
  comp_counts = torch.empty(nc, 2, dtype=torch.int32, device=device)
  bbox = torch.empty(nc, 6, dtype=torch.float32, device=device) if vertices is not None else None
  L.check(lib.nrf_mesh_component_table(ptr(faces), F, vertices.data_ptr() if vertices is not None else None, V, ptr(labels), nc,
                                       ptr(comp_counts), bbox.data_ptr() if bbox is not None else None, ws.data_ptr(), ws.numel() * 4,
                                       stream), lib)
  out = {'labels': labels, 'num_vertices': comp_counts[:, 0].contiguous(), 'num_triangles': comp_counts[:, 1].contiguous()}
  if bbox is not None:
    out.update(bbox_min=bbox[:, :3].contiguous(), bbox_max=bbox[:, 3:].contiguous())
  return out


def _gather_rows(lib, src, vertex_map, kept, stream):
  """src (V, ...) -> (kept, ...): the rows whose vertex_map is not -1, in order (nrf_mesh_gather_rows)."""
  src = src.contiguous()
  V = src.shape[0]
  row_bytes = (src.numel() // V) * src.element_size() if V else 0
  dst = torch.empty((kept,) + tuple(src.shape[1:]), dtype=src.dtype, device=src.device)
  if V == 0 or kept == 0 or row_bytes == 0:
    return dst
  if row_bytes % 4:
    raise ValueError(f'submesh gathers rows of 4-byte words; a row of {src.dtype} {tuple(src.shape[1:])} has {row_bytes} bytes')
  L.check(lib.nrf_mesh_gather_rows(src.data_ptr(), row_bytes // 4, vertex_map.data_ptr(), V, dst.data_ptr(), kept, stream), lib)
  return dst


def submesh(mesh, keep_vertices, lib=None):
  """The mesh restricted to the vertices a mask keeps (nrf_mesh_submesh_count / _emit, nrf_mesh_gather_rows): `mesh` is a dict as
  extract_mesh / extract_mesh_from_grid return it, or any dict with 'faces' (F, 3) int32; `keep_vertices` a (V,) bool or uint8
  device tensor.  A triangle is kept iff all three of its vertices are (and its indices are in [0, V)); kept vertices and triangles
  keep their order.  Every tensor of the dict whose first dimension is V is gathered -- 'vertices', 'vertex_cell', 'normals',
  'sigma', 'rgb', anything the caller added -- and a (K, V, ...) tensor (an animate_mesh result) along its second; 'faces' is
  re-indexed; everything else is passed on as it is.  Adds 'vertex_map' (V,) int32: each old vertex's new index, or -1.  The mask
  may come from anywhere: components (clean_mesh), animate_mesh's status == 1, a box, a density cut."""
  lib = lib or L.load_library()
  faces = _faces_arg(mesh['faces'])
  device = faces.device
  keep = torch.as_tensor(keep_vertices)
  if keep.dim() != 1 or keep.dtype not in (torch.bool, torch.uint8):
    raise ValueError(f'keep_vertices must be a (V,) bool or uint8 tensor, got {keep.dtype} {tuple(keep.shape)}')
  keep = keep.to(device=device, dtype=torch.uint8).contiguous()
  V, F = keep.shape[0], faces.shape[0]
  stream = _stream_arg(device)
  ptr = lambda t: t.data_ptr() if t.numel() else None
  ws = _mesh_workspace(lib, lib.nrf_mesh_submesh_workspace_bytes, V, F, device)
  counts = torch.zeros(2, dtype=torch.int32, device=device)
  L.check(lib.nrf_mesh_submesh_count(ptr(keep), V, ptr(faces), F, counts.data_ptr(), ws.data_ptr(), ws.numel() * 4, stream), lib)
  nv, nt = (int(v) for v in counts.tolist())
  vertex_map = torch.empty(V, dtype=torch.int32, device=device)
  faces_out = torch.empty(nt, 3, dtype=torch.int32, device=device)
  L.check(lib.nrf_mesh_submesh_emit(ptr(keep), V, ptr(faces), F, nv, nt, ptr(vertex_map), ptr(faces_out), ws.data_ptr(), ws.numel() * 4,
                                    stream), lib)
  out = {}
  for key, value in mesh.items():
    if key == 'faces':
      out[key] = faces_out
    elif not torch.is_tensor(value) or value.dim() == 0 or key == 'vertex_map':
      out[key] = value
    elif value.shape[0] == V:
      out[key] = _gather_rows(lib, value, vertex_map, nv, stream)
    elif value.dim() >= 2 and value.shape[1] == V:
      out[key] = torch.stack([_gather_rows(lib, value[k], vertex_map, nv, stream) for k in range(value.shape[0])], 0) if value.shape[0] \
          else value.new_empty((0, nv) + tuple(value.shape[2:]))
    else:
      out[key] = value
  out['vertex_map'] = vertex_map
  return out


def select_components(num_triangles, keep='largest', min_triangles=1):
  """The component ids clean_mesh keeps, from the (C,) triangle counts as a list: those with at least `min_triangles` triangles, and of
  them all (`keep='all'`), the one (`'largest'`) or the `keep` = K >= 1 with the most triangles, ties going to the smaller id."""
  if keep == 'largest':
    keep = 1
  if keep != 'all' and (isinstance(keep, bool) or not isinstance(keep, int) or keep < 1):
    raise ValueError(f"keep must be 'all', 'largest' or an int >= 1, got {keep!r}")
  ids = [c for c, n in enumerate(num_triangles) if n >= int(min_triangles)]
  if keep != 'all':
    ids = sorted(sorted(ids, key=lambda c: (-num_triangles[c], c))[:keep])
  return ids


def clean_mesh(mesh, keep='largest', min_triangles=1, lib=None):
  """Drops the floaters of a mesh dict (mesh_components, then submesh): components with fewer than `min_triangles` triangles go first
  (the default drops the vertices no triangle names), then `keep` = 'all', 'largest' or an int K >= 1 keeps the K components with the
  most triangles, ties going to the smaller component id.  The selection runs on the (C,) table, read back once.  Returns submesh's
  dict, with 'components': the table of the mesh as it came in (mesh_components' dict, labels included) and its 'kept' ids."""
  lib = lib or L.load_library()
  vertices = mesh.get('vertices')
  faces = _faces_arg(mesh['faces'])
  if torch.is_tensor(vertices) and vertices.dim() == 2 and vertices.dtype == torch.float32:
    comps = mesh_components(vertices, faces, lib=lib)
  else:   # e.g. an animate_mesh result: no single set of positions to box
    comps = mesh_components(None, faces, lib=lib, num_vertices=vertices.shape[1] if torch.is_tensor(vertices) else None)
  ids = select_components(comps['num_triangles'].tolist(), keep, min_triangles)
  keep_component = torch.zeros(comps['num_triangles'].shape[0], dtype=torch.bool, device=faces.device)
  if ids:
    keep_component[torch.tensor(ids, dtype=torch.int64, device=faces.device)] = True
  out = submesh(mesh, keep_component[comps['labels'].long()], lib=lib)
  out['components'] = dict(comps, kept=ids)
  return out


def _raster_rows(t, width, what):
  t = torch.as_tensor(t)
  if t.dtype != torch.float32 or t.dim() != 2 or (width is not None and t.shape[1] != width) or t.shape[1] < 1:
    raise ValueError(f'{what} must be a float32 (V, {width or "A"}) tensor, got {t.dtype} {tuple(t.shape)}')
  return t.contiguous()


def rasterize_screen(screen, faces, image_size, near=0.0, attributes=None, background=0.0, lib=None):
  """nrf_mesh_raster_draw on a (V, 3) float32 device tensor of (px, py, z) rows from anywhere, then one nrf_mesh_raster_interpolate
  per entry of `attributes`: what rasterize_mesh runs after its projection (an orthographic view is screen = (x, y, z) scaled by the
  caller).  image_size is (width, height).  Returns rasterize_mesh's dict, with 'status': the (4,) int32 device tensor of the
  workspace's nrf_mesh_raster_status (drawn triangles, large triangles, covered pixels, 0)."""
  lib = lib or L.load_library()
  screen = _raster_rows(screen, 3, 'screen')
  faces = _faces_arg(faces).to(screen.device)
  device = screen.device
  W, H = int(image_size[0]), int(image_size[1])
  V, F = screen.shape[0], faces.shape[0]
  stream = _stream_arg(device)
  ptr = lambda t: t.data_ptr() if t.numel() else None
  ws = _mesh_workspace(lib, lambda nv, nt, out: lib.nrf_mesh_raster_workspace_bytes(nt, W, H, out), V, F, device)
  face_id = torch.empty(H, W, dtype=torch.int32, device=device)
  depth = torch.empty(H, W, dtype=torch.float32, device=device)
  bary = torch.empty(H, W, 3, dtype=torch.float32, device=device)
  L.check(lib.nrf_mesh_raster_draw(ptr(screen), V, ptr(faces), F, W, H, float(near), face_id.data_ptr(), depth.data_ptr(), bary.data_ptr(),
                                   ws.data_ptr(), ws.numel() * 4, stream), lib)
  out = {'face_id': face_id, 'depth': depth, 'mask': face_id >= 0, 'bary': bary, 'status': ws[:4].clone()}
  for name, rows in (attributes or {}).items():
    if name in out or name == 'screen':
      raise ValueError(f'attribute name {name!r} is one of the raster outputs')
    rows = _raster_rows(rows, None, f'attributes[{name!r}]').to(device)
    if rows.shape[0] != V:
      raise ValueError(f'attributes[{name!r}] has {rows.shape[0]} rows for {V} vertices')
    A = rows.shape[1]
    bg = torch.as_tensor(background[name] if isinstance(background, dict) else background, dtype=torch.float32).to(device)
    bg = bg.expand(A).contiguous() if bg.dim() <= 1 else bg
    if tuple(bg.shape) != (A,):
      raise ValueError(f'background of {name!r} must be a scalar or ({A},), got {tuple(bg.shape)}')
    value = torch.empty(H, W, A, dtype=torch.float32, device=device)
    L.check(lib.nrf_mesh_raster_interpolate(face_id.data_ptr(), bary.data_ptr(), H * W, ptr(faces), F, ptr(rows), V, A, bg.data_ptr(),
                                            value.data_ptr(), stream), lib)
    out[name] = value
  return out


def rasterize_mesh(vertices, faces, table, image_size, camera_row=0, near=0.0, attributes=None, background=0.0, lib=None):
  """One frame's mesh seen by one camera, all on the device (nrf_camera_table_project_depth, nrf_mesh_raster_draw, then one
  nrf_mesh_raster_interpolate per attribute; the definition is in include/nerfies_amd.h): `vertices` (V, 3) float32, `faces` (F, 3)
  int32, `table` a pack_cameras table of which row `camera_row` is used, image_size (width, height), `near` the plane behind which a
  vertex drops its triangles whole (no clipping).  `attributes` is a dict name -> (V, A) float32, e.g. {'rgb': ..., 'normals': ...,
  'points': vertices}; `background` a scalar, an (A,) row, or a dict of those by name.  Returns device tensors {'face_id' (H, W) int32
  (-1: no triangle), 'depth' (H, W) along the optical axis (0 where empty), 'mask' (H, W) bool, 'bary' (H, W, 3), 'screen' (V, 3),
  'status' (4,) int32 and one (H, W, A) tensor per attribute}, the same bits on every run and for every order of the faces."""
  from nerfies_amd import camera as camera_lib
  lib = lib or L.load_library()
  vertices = _raster_rows(vertices, 3, 'vertices')
  row = int(camera_row)
  if not 0 <= row < table.shape[0]:
    raise ValueError(f'camera_row = {row} is outside the table of {table.shape[0]} rows')
  index = torch.full((vertices.shape[0],), row, dtype=torch.int32, device=vertices.device) if row else None
  screen = camera_lib.project_depth_from_table(table, vertices, index)
  out = rasterize_screen(screen, faces, image_size, near=near, attributes=attributes, background=background, lib=lib)
  out['screen'] = screen
  return out


def mesh_visibility(raster, faces, num_vertices, lib=None):
  """(V,) bool: the vertices that are a corner of a face owning at least one pixel of `raster` (a rasterize_mesh result, or its
  'face_id' tensor): nrf_mesh_raster_visibility."""
  lib = lib or L.load_library()
  face_id = (raster['face_id'] if isinstance(raster, dict) else raster).contiguous()
  if face_id.dtype != torch.int32:
    raise ValueError(f'face_id must be int32, got {face_id.dtype}')
  faces = _faces_arg(faces).to(face_id.device)
  V = int(num_vertices)
  visible = torch.empty(V, dtype=torch.uint8, device=face_id.device)
  ptr = lambda t: t.data_ptr() if t.numel() else None
  L.check(lib.nrf_mesh_raster_visibility(ptr(face_id), face_id.numel(), ptr(faces), faces.shape[0], V, ptr(visible),
                                         _stream_arg(face_id.device)), lib)
  return visible.bool()


def extract_mesh(model, params, bbox_min, bbox_max, resolution, threshold, level='fine', warp_id=None, appearance_id=None, camera_id=None,
                 warp_extra=None, refine_steps=2, colors=True, chunk=1 << 21, clean=None):
  """A triangle mesh of the field's level set sigma = threshold over the box [bbox_min, bbox_max], all on the device: `density_grid`
  (same arguments; its voxel centres are the mesh's samples, so `resolution` R gives R - 1 cells per axis), surface nets
  (`extract_mesh_from_grid`), then `refine_steps` rounds of the field's own density and gradient at the vertices
  (NerfModel.query_gradient) and one Newton step onto the level set each (nrf_mesh_snap: every vertex stays inside its cell, the
  faces do not change).  `warp_id=None` meshes the canonical (template) volume, an id that frame's observation volume.
  `appearance_id` / `camera_id`: the codes the colour is queried with (and, for a use_alpha_condition model, the density).
  Returns device tensors {'vertices' (V, 3), 'faces' (F, 3) int32, 'normals' (V, 3) = -grad sigma / |grad sigma| at the final
  vertices, 'sigma' (V,) there, and with `colors` 'rgb' (V, 3) along MESH_VIEW_DIRECTION}.
  `clean`: None, or the keyword set of `clean_mesh` as a dict (keep=, min_triangles=), applied right after surface nets and before the
  refinement, the normals and the colours, so a dropped vertex costs no query; the dict then also has clean_mesh's 'vertex_map' (over
  the uncleaned vertices) and 'components'.  Every kept row has the bits it has without `clean`: a query's row does not depend on the
  launch it ran in."""
  res, origin, step = _box_grid(bbox_min, bbox_max, resolution)
  alpha_app = appearance_id if getattr(model, 'use_alpha_condition', False) else None
  sigma = density_grid(model, params, bbox_min, bbox_max, res, level=level, warp_id=warp_id, appearance_id=alpha_app,
                       warp_extra=warp_extra, chunk=chunk)
  lib = model.lib
  mesh = extract_mesh_from_grid(sigma, origin, step, threshold, lib=lib)
  if clean is not None:
    mesh = clean_mesh(mesh, lib=lib, **clean)
  vertices, vertex_cell = mesh['vertices'], mesh['vertex_cell']
  device = vertices.device
  nv = vertices.shape[0]
  out = {'vertices': vertices, 'faces': mesh['faces']}
  if clean is not None:
    out.update(vertex_map=mesh['vertex_map'], components=mesh['components'])
  if nv == 0:
    out.update(normals=torch.zeros(0, 3, device=device), sigma=torch.zeros(0, device=device))
    if colors:
      out['rgb'] = torch.zeros(0, 3, device=device)
    return out
  use_warp = warp_id is not None
  md = _one_group_metadata(warp_id, alpha_app, None, device)
  _, grid = _mesh_grid(sigma, origin, step)
  kw = dict(metadata=md, warp_extra=warp_extra, level=level, use_warp=use_warp)
  for _ in range(int(refine_steps)):
    q = model.query_gradient(params, vertices, outputs=('sigma', 'grad_sigma'), **kw)
    L.check(lib.nrf_mesh_snap(vertices.data_ptr(), vertex_cell.data_ptr(), q['sigma'].data_ptr(), q['grad_sigma'].data_ptr(), C.byref(grid),
                              float(threshold), nv, _stream_arg(device)), lib)
  q = model.query_gradient(params, vertices, outputs=('sigma', 'normals'), **kw)
  out.update(normals=q['normals'], sigma=q['sigma'])
  if colors:
    cmd = _one_group_metadata(warp_id, appearance_id, camera_id, device)
    view = torch.tensor([MESH_VIEW_DIRECTION], dtype=torch.float32, device=device)
    per = max(1, min(int(chunk), L.NRF_QUERY_MAX_POINTS))
    parts = [model.query_points(params, vertices[first:first + count], viewdirs=view, metadata=cmd, warp_extra=warp_extra, level=level,
                                use_warp=use_warp, outputs=('rgb',))['rgb'] for first, count in grid_chunks(nv, per)]
    out['rgb'] = torch.cat(parts, 0)
  return out


def animate_mesh(model, params, vertices, warp_ids, warp_extra=None, steps=8, tolerance=1e-6, warm_start=True):
  """A canonical (template) surface carried into frames: for each of the K `warp_ids`, in order, the observation-space points x_k
  with warp_points(x_k, id_k) = `vertices` (V, 3), e.g. those of extract_mesh(warp_id=None) -- NerfModel.unwarp_points, `steps`
  Newton rounds per frame.  The faces are the template's: every frame keeps its topology and vertex order.  With `warm_start` frame
  k + 1 starts from frame k's solution (adjacent frames are close), frame 0 from the template itself.  `tolerance`: the residual
  |W(x) - vertex| at which a vertex counts as converged; the default is about four times the float32 forward's own error at scene
  scale.  Returns device tensors {'vertices' (K, V, 3), 'residual' (K, V), 'status' (K, V) int32: 1 converged, 0 ran out of
  steps, 2 stopped where the field is singular}; a vertex with another status than 1 is returned as it is, for the caller to see."""
  vertices = torch.as_tensor(vertices)
  device = vertices.device
  ids = [int(i) for i in warp_ids]
  V = vertices.shape[0]
  out = {'vertices': torch.empty(len(ids), V, 3, dtype=torch.float32, device=device),
         'residual': torch.empty(len(ids), V, dtype=torch.float32, device=device),
         'status': torch.empty(len(ids), V, dtype=torch.int32, device=device)}
  guess = None
  for k, wid in enumerate(ids):
    if V == 0:
      break
    got = model.unwarp_points(params, vertices, torch.full((V,), wid, dtype=torch.int32, device=device), warp_extra, guess=guess,
                              steps=steps, tolerance=tolerance)
    out['vertices'][k], out['residual'][k], out['status'][k] = got['points'], got['residual'], got['status']
    if warm_start:
      guess = got['points']
  return out


def compute_psnr(mse):
  """utils.compute_psnr (utils.py:283-293): -10 log10(mse)."""
  return -10.0 * torch.log10(torch.as_tensor(mse))


_MSSSIM_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)


def compute_multiscale_ssim(image1: torch.Tensor, image2: torch.Tensor, max_val: float = 1.0, filter_size: int = 11,
                            filter_sigma: float = 1.5, k1: float = 0.01, k2: float = 0.03) -> torch.Tensor:
  """MS-SSIM of two [H, W, C] images (eval.py:60-62 calls tf.image.ssim_multiscale(image1, image2, max_val=1.0)).

  TensorFlow is a third-party dependency that is absent here, so its published algorithm (Wang, Simoncelli & Bovik 2003,
  with TF's defaults) is restated and is UNPINNED against TF itself: per channel, 5 scales; at each scale an
  11x11 sigma-1.5 Gaussian window (VALID) gives the local means / variances / covariance, the contrast-structure term
  cs = (2 s12 + c2) / (s1 + s2 + c2) and the full ssim = cs * (2 m1 m2 + c1) / (m1^2 + m2^2 + c1) are averaged over
  the window positions; images are halved by 2x2 average pooling between scales (odd sizes padded symmetrically);
  result = prod_i relu(cs_i)^w_i over the first 4 scales times relu(ssim_5)^w_5, averaged over channels.  Needs
  H, W >= 11 * 2^4 = 176."""
  x = image1.to(torch.float32).permute(2, 0, 1)[None]
  y = image2.to(x.device, torch.float32).permute(2, 0, 1)[None]
  c = x.shape[1]
  if min(x.shape[-2:]) < filter_size * 2 ** (len(_MSSSIM_WEIGHTS) - 1):
    raise ValueError(f'MS-SSIM needs images of at least {filter_size * 2 ** (len(_MSSSIM_WEIGHTS) - 1)} px per side')
  r = torch.arange(filter_size, dtype=torch.float32, device=x.device) - (filter_size - 1) / 2
  g = torch.exp(-0.5 * (r / filter_sigma) ** 2)
  g = g / g.sum()
  win = (g[:, None] * g[None, :])[None, None].repeat(c, 1, 1, 1)
  blur = lambda t: torch.nn.functional.conv2d(t, win, groups=c)
  c1, c2 = (k1 * max_val) ** 2, (k2 * max_val) ** 2
  terms = []
  for i, w in enumerate(_MSSSIM_WEIGHTS):
    if i:
      ph, pw = x.shape[-2] % 2, x.shape[-1] % 2
      if ph or pw:
        x = torch.nn.functional.pad(x, (0, pw, 0, ph), mode='replicate')     # symmetric padding of one pixel
        y = torch.nn.functional.pad(y, (0, pw, 0, ph), mode='replicate')
      x = torch.nn.functional.avg_pool2d(x, 2)
      y = torch.nn.functional.avg_pool2d(y, 2)
    m1, m2 = blur(x), blur(y)
    num0, den0 = m1 * m2 * 2.0, m1 * m1 + m2 * m2
    cs = (blur(x * y) * 2.0 - num0 + c2) / (blur(x * x + y * y) - den0 + c2)
    if i + 1 < len(_MSSSIM_WEIGHTS):
      terms.append(torch.relu(cs.mean(dim=(-2, -1))) ** w)
    else:
      terms.append(torch.relu((cs * (num0 + c1) / (den0 + c1)).mean(dim=(-2, -1))) ** w)
  return torch.stack(terms, 0).prod(0).mean()


def image_metrics(rgb: torch.Tensor, target: torch.Tensor) -> Dict[str, torch.Tensor]:
  """mse / psnr (/ multiscale ssim when the frame is large enough for 5 scales) of a rendered frame against its
  target (eval.py:121-128)."""
  target = target.to(rgb.device)
  mse = ((rgb - target) ** 2).mean()
  out = {'mse': mse, 'psnr': compute_psnr(mse)}
  if min(rgb.shape[:2]) >= 176:
    out['ssim'] = compute_multiscale_ssim(target, rgb)
  return out
