#!/usr/bin/env python
"""Density grid of a trained field: loads the experiment's latest checkpoint, takes the box of the capture's scene points
(points.npy, in the normalised scene frame) and queries the activated density on a regular grid through the library's field
query (evaluation.density_grid -> nrf_query_grid: the points are formed on the device, the density-only kernel runs).

  python scripts/export_density.py --base_folder EXP --data_dir CAPTURE --gin_configs EXP/config.gin \\
      --resolution 128 --frame 000012            # the observation volume of frame 000012 (through the warp field)
  python scripts/export_density.py ... --canonical   # the canonical (template) volume: the warp field is skipped

Writes, next to the checkpoints' experiment directory:
  density_<name>.npy   float32 (X, Y, Z) sigma at the voxel centres (<name> = the frame id, or 'canonical'), and
  density_<name>.ply   ASCII point cloud of the voxel centres with sigma > --threshold, coloured by a full query along a fixed
                       view direction.
With --normals (evaluation.normal_grid -> nrf_query_grid_grad: the density's gradient from the reverse chain, no finite differences):
  normals_<name>.npy   float32 (X, Y, Z, 3) unit normals -grad sigma / |grad sigma| at the voxel centres (0 where the gradient
                       vanishes), and the PLY's vertices gain the properties nx ny nz.
With --mesh (evaluation.extract_mesh -> nrf_mesh_count / nrf_mesh_emit / nrf_mesh_snap: surface nets on the device grid, the vertices
pulled onto the level set sigma = --threshold by --mesh_refine Newton steps along the field's own gradient):
  mesh_<name>.ply      binary little-endian triangle mesh: vertices x y z nx ny nz red green blue, faces as vertex_indices lists.
The .npy grid and the point cloud stay what they were; the mesh is the iso-surface they stopped short of.
With --mesh_keep largest | K and / or --mesh_min_triangles M (evaluation.clean_mesh -> nrf_mesh_components / nrf_mesh_submesh_*: connected
components on the device) the floaters are dropped right after surface nets, before any vertex is refined or coloured; the component
table's head is printed either way, and --animate carries the cleaned template.
With --mesh --canonical --animate ITEM_ID [ITEM_ID ...] (evaluation.animate_mesh -> nrf_unwarp_points: the warp field inverted at the
template's vertices, Newton's iteration on the device, each frame started from the one before):
  mesh_canonical_at_<item_id>.ply   the template carried into that frame: the same vertex_indices and colours, the vertices x with
                       warp(x, frame) = template vertex, the normals of the field there.  Vertices that did not converge are counted
                       in the printed summary and written as they are.
With --mesh --render_mesh ITEM_ID [ITEM_ID ...] (evaluation.rasterize_mesh -> nrf_camera_table_project_depth / nrf_mesh_raster_draw /
nrf_mesh_raster_interpolate: the mesh rasterised on the device into that item's own camera, at the capture's image size and near plane;
an item named by --animate is drawn with the mesh carried into it, any other with the mesh as extracted):
  mesh_render_<item_id>.png   the mesh over a white background, coloured by its vertices' rgb or, with --render_shading normals, by
                       its normals (n / 2 + 1 / 2),
  mesh_depth_<item_id>.npy    float32 (H, W): the distance from the camera's position to the mesh along each pixel's ray, 0 where no
                       triangle covers the pixel,
and prints the covered share of pixels and the median of |mesh ray distance - NeRF depth| over the covered pixels, the NeRF depth
being that of evaluation.render_image for the same camera."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import train as train_driver   # noqa: E402
from nerfies_amd import camera as camera_lib, checkpoints, configs, evaluation, models, training   # noqa: E402
from nerfies_amd import visualization as viz   # noqa: E402
from nerfies_amd import gin_lite as gin   # noqa: E402

VIEW_DIRECTION = (0.0, 0.0, 1.0)   # the direction every exported colour is queried along


def parse_flags(argv=None):
  """The drivers' flags (train.py) plus the export's own."""
  p = argparse.ArgumentParser(add_help=False)
  p.add_argument('--resolution', type=int, nargs='+', default=[64], help='voxels per axis: one number, or X Y Z')
  which = p.add_mutually_exclusive_group(required=True)
  which.add_argument('--frame', default=None, metavar='ITEM_ID', help="query that frame's observation volume (its warp / appearance / camera ids)")
  which.add_argument('--canonical', action='store_true', help='query the canonical volume (NRF_FLAG_NO_WARP)')
  p.add_argument('--threshold', type=float, default=10.0, help='voxels with sigma above it go into the PLY')
  p.add_argument('--level', default='fine', choices=['coarse', 'fine'])
  p.add_argument('--normals', action='store_true', help='also export the surface normals -grad sigma / |grad sigma| (npy, and nx ny nz in the PLY)')
  p.add_argument('--mesh', action='store_true', help='also extract the triangle mesh of the level set sigma = --threshold (mesh_<name>.ply)')
  p.add_argument('--mesh_refine', type=int, default=2, metavar='K', help='Newton steps of the mesh vertices onto the level set')
  p.add_argument('--mesh_keep', default='all', metavar='{all,largest,K}',
                 help='with --mesh: the connected components to keep: all, the largest, or the K with the most triangles')
  p.add_argument('--mesh_min_triangles', type=int, default=0, metavar='M', help='with --mesh: drop components with fewer triangles first')
  p.add_argument('--animate', nargs='+', default=None, metavar='ITEM_ID',
                 help='with --mesh --canonical: carry the template mesh into these frames (mesh_canonical_at_<item_id>.ply each)')
  p.add_argument('--animate_steps', type=int, default=8, metavar='K', help='Newton rounds per frame of --animate')
  p.add_argument('--render_mesh', nargs='+', default=None, metavar='ITEM_ID',
                 help="with --mesh: rasterise the mesh into these items' cameras (mesh_render_<item_id>.png, mesh_depth_<item_id>.npy) and "
                      "compare it with the NeRF's depth there.  The NeRF's `depth` is a distance along unit rays, not the coordinate z along "
                      "the optical axis the rasteriser orders by: the mesh side is converted, to |interpolated surface point - camera "
                      "position|, and that distance is what the .npy holds")
  p.add_argument('--render_shading', default='rgb', choices=['rgb', 'normals'], help='with --render_mesh: what colours the PNG')
  p.add_argument('--margin', type=float, default=0.0, help="grow the scene points' box by this fraction of its size on every side")
  own, rest = p.parse_known_args(argv)
  if len(own.resolution) not in (1, 3):
    p.error('--resolution takes one number or three')
  if own.mesh_keep not in ('all', 'largest'):
    if not own.mesh_keep.isdigit() or int(own.mesh_keep) < 1:
      p.error("--mesh_keep takes 'all', 'largest' or a number K >= 1")
    own.mesh_keep = int(own.mesh_keep)
  if own.mesh_min_triangles < 0:
    p.error('--mesh_min_triangles must not be negative')
  if own.animate is not None and not (own.mesh and own.canonical):
    p.error('--animate carries the canonical mesh into frames: it needs --mesh --canonical')
  if own.render_mesh is not None and not own.mesh:
    p.error('--render_mesh rasterises the mesh: it needs --mesh')
  flags = train_driver.parse_flags(rest)
  for k, v in vars(own).items():
    setattr(flags, k, v)
  return flags


def write_ply(path, xyz, rgb, normals=None):
  """ASCII PLY of points (N, 3) with colours (N, 3) in [0, 1] and, when given, normals (N, 3) as nx ny nz."""
  rgb8 = np.clip(np.rint(rgb * 255.0), 0, 255).astype(np.uint8)
  with open(path, 'w') as f:
    f.write('ply\nformat ascii 1.0\n')
    f.write(f'element vertex {len(xyz)}\n')
    f.write('property float x\nproperty float y\nproperty float z\n')
    if normals is not None:
      f.write('property float nx\nproperty float ny\nproperty float nz\n')
    f.write('property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n')
    if normals is None:
      for (x, y, z), (r, g, b) in zip(xyz, rgb8):
        f.write(f'{x:.6f} {y:.6f} {z:.6f} {r} {g} {b}\n')
    else:
      for (x, y, z), (nx, ny, nz), (r, g, b) in zip(xyz, normals, rgb8):
        f.write(f'{x:.6f} {y:.6f} {z:.6f} {nx:.6f} {ny:.6f} {nz:.6f} {r} {g} {b}\n')


def write_mesh_ply(path, vertices, normals, rgb, faces):
  """Binary little-endian PLY of an indexed triangle mesh: vertices (V, 3), normals (V, 3), colours (V, 3) in [0, 1], faces (F, 3)."""
  vert = np.zeros(len(vertices), dtype=[('xyz', '<f4', 3), ('n', '<f4', 3), ('rgb', 'u1', 3)])
  vert['xyz'], vert['n'] = vertices, normals
  vert['rgb'] = np.clip(np.rint(np.asarray(rgb) * 255.0), 0, 255).astype(np.uint8)
  face = np.zeros(len(faces), dtype=[('n', 'u1'), ('idx', '<i4', 3)])
  face['n'], face['idx'] = 3, faces
  head = ('ply\nformat binary_little_endian 1.0\n'
          f'element vertex {len(vert)}\n'
          'property float x\nproperty float y\nproperty float z\nproperty float nx\nproperty float ny\nproperty float nz\n'
          'property uchar red\nproperty uchar green\nproperty uchar blue\n'
          f'element face {len(face)}\nproperty list uchar int vertex_indices\nend_header\n')
  with open(path, 'wb') as f:
    f.write(head.encode('ascii'))
    f.write(vert.tobytes())
    f.write(face.tobytes())


def print_component_table(name, comps, head=8):
  """The first `head` rows of evaluation.mesh_components' table, largest first; returns the number of components."""
  nv, nt = comps['num_vertices'].tolist(), comps['num_triangles'].tolist()
  lo, hi = comps['bbox_min'].cpu().numpy().astype(np.float64), comps['bbox_max'].cpu().numpy().astype(np.float64)
  kept = comps.get('kept')
  order = sorted(range(len(nt)), key=lambda c: (-nt[c], c))
  print(f'mesh_{name}: {len(nt)} connected components' + ('' if kept is None else f', {len(kept)} kept'), flush=True)
  for c in order[:head]:
    mark = '' if kept is None else (' kept' if c in kept else ' dropped')
    print(f'  component {c}: {nv[c]} vertices, {nt[c]} triangles, box {lo[c].round(4).tolist()} .. {hi[c].round(4).tolist()}{mark}', flush=True)
  if len(order) > head:
    print(f'  ... and {len(order) - head} smaller', flush=True)
  return len(nt)


def animate(flags, model, target, warp_extra, datasource, mesh, alpha_app, exp_dir, carried=None):
  """--animate: the template `mesh` carried into every frame of flags.animate; {item id: its PLY}.  `carried`, when given, receives
  {item id: (vertices, normals)} on the device."""
  if not model.use_warp or model.warp_metadata_encoder_type == 'time':
    raise SystemExit('--animate: needs a model with a warp field driven by warp ids (not the time encoder)')
  known = list(datasource.train_ids) + list(datasource.val_ids)
  for item in flags.animate:
    if item not in known:
      raise SystemExit(f'--animate {item}: not an item of the capture')
  ids = [datasource.get_warp_id(item) for item in flags.animate]
  frames = evaluation.animate_mesh(model, target, mesh['vertices'], ids, warp_extra=warp_extra, steps=flags.animate_steps)
  faces, rgb = mesh['faces'].cpu().numpy(), mesh['rgb'].cpu().numpy()
  nv, written = mesh['vertices'].shape[0], {}
  for k, (item, wid) in enumerate(zip(flags.animate, ids)):
    verts = frames['vertices'][k]
    normals = torch.zeros(0, 3)
    if nv:   # the field's normals where the vertices now are, through that frame's warp
      md = evaluation._one_group_metadata(wid, alpha_app, None, verts.device)
      normals = model.query_gradient(target, verts, metadata=md, warp_extra=warp_extra, level=flags.level, outputs=('normals',))['normals']
    path = os.path.join(exp_dir, f'mesh_canonical_at_{item}.ply')
    write_mesh_ply(path, verts.cpu().numpy(), normals.cpu().numpy(), rgb, faces)
    status = frames['status'][k]
    left, stopped = int((status == 0).sum()), int((status == 2).sum())
    worst = float(frames['residual'][k].max()) if nv else 0.0
    print(f'mesh_canonical_at_{item}: {nv} vertices, {nv - left - stopped} converged, {left} out of steps, {stopped} stopped at a singular '
          f'step, largest residual {worst:.3g} -> {path}', flush=True)
    written[item] = path
    if carried is not None:
      carried[item] = (verts, normals)
  return written


def render_mesh(flags, model, state, datasource, mesh, carried, exp_dir):
  """--render_mesh: the mesh rasterised into each item's camera and held against the field's own depth there;
  {item id: {'png', 'depth_npy', 'covered', 'median_abs_depth_difference'}}."""
  known = list(datasource.train_ids) + list(datasource.val_ids)
  device = mesh['faces'].device
  model_fn = lambda key_0, key_1, params, rays, warp_extra: model.apply({'params': params}, rays, warp_extra)
  out = {}
  for item in flags.render_mesh:
    if item not in known:
      raise SystemExit(f'--render_mesh {item}: not an item of the capture')
    vertices, normals = carried.get(item, (mesh['vertices'], mesh['normals']))
    cam = datasource.load_camera(item)
    W, H = int(cam.image_size[0]), int(cam.image_size[1])
    table = camera_lib.pack_cameras([cam], device)
    shade = mesh['rgb'] if flags.render_shading == 'rgb' else normals * 0.5 + 0.5
    raster = evaluation.rasterize_mesh(vertices, mesh['faces'], table, (W, H), near=datasource.near,
                                       attributes={'shade': shade.float().contiguous(), 'points': vertices}, background={'shade': 1.0, 'points': 0.0},
                                       lib=model.lib)
    mask = raster['mask']
    position = table[0, 9:12]
    distance = torch.where(mask, (raster['points'] - position).norm(dim=-1), torch.zeros((), device=device))
    png = os.path.join(exp_dir, f'mesh_render_{item}.png')
    viz.save_image(png, viz.image_to_uint8(raster['shade'].cpu().numpy()))
    depth_npy = os.path.join(exp_dir, f'mesh_depth_{item}.npy')
    np.save(depth_npy, distance.cpu().numpy())
    rays = datasource.item_rays(item, device)
    rays = {k: rays[k] for k in ('origins', 'directions', 'viewdirs', 'metadata') if k in rays}
    field = evaluation.render_image(state, rays, model_fn, chunk=8192)['depth'].reshape(H, W)
    covered = float(mask.float().mean())
    median = float((distance - field).abs()[mask].median()) if bool(mask.any()) else float('nan')
    print(f'mesh_render_{item}: {W} x {H}, {covered:.2%} of the pixels covered, median |mesh ray distance - NeRF depth| {median:.4g} over '
          f'them -> {png}, {depth_npy}', flush=True)
    out[item] = {'png': png, 'depth_npy': depth_npy, 'covered': covered, 'median_abs_depth_difference': median}
  return out


def main(argv=None):
  flags = parse_flags(argv)
  if flags.bf16:
    raise SystemExit('--bf16: a field query runs in the float32 mode')
  gin.parse_config_files_and_bindings(config_files=flags.gin_configs, bindings=flags.gin_bindings, skip_unknown=True)
  exp_config = configs.ExperimentConfig()
  model_config = configs.ModelConfig(use_stratified_sampling=False)
  _, _, device = train_driver.init_distributed()
  exp_dir = flags.base_folder if not exp_config.subname else os.path.join(flags.base_folder, exp_config.subname)
  checkpoint_dir = os.path.join(exp_dir, 'checkpoints')
  datasource = train_driver.make_datasource(flags, exp_config, model_config)
  model, params = models.construct_nerf(
      20200823, model_config, batch_size=0, appearance_ids=datasource.appearance_ids, camera_ids=datasource.camera_ids,
      warp_ids=datasource.warp_ids, near=datasource.near, far=datasource.far, device=device)
  if checkpoints.latest_checkpoint(checkpoint_dir) is None:
    raise FileNotFoundError(f'no checkpoint under {checkpoint_dir}')
  state = checkpoints.restore_checkpoint(checkpoint_dir, training.TrainState(optimizer=training.Optimizer(params)))
  target = state.optimizer.target

  # the ids of the queried frame; the canonical volume borrows the first training frame's appearance / camera ids (its density
  # does not depend on them unless the model conditions the alpha head, its colour does)
  item = flags.frame if flags.frame is not None else datasource.train_ids[0]
  if flags.frame is not None and flags.frame not in list(datasource.train_ids) + list(datasource.val_ids):
    raise SystemExit(f'--frame {flags.frame}: not an item of the capture')
  use_warp = bool(model.use_warp) and not flags.canonical
  if use_warp and model.warp_metadata_encoder_type == 'time':
    raise SystemExit('--frame: a field query takes warp ids, not the time encoder (use --canonical)')
  warp_id = datasource.get_warp_id(item) if use_warp else None
  app_id = datasource.get_appearance_id(item) if model.use_appearance_metadata else None
  cam_id = datasource.get_camera_id(item) if model.use_camera_metadata else None
  name = flags.frame if flags.frame is not None else 'canonical'

  points = datasource.load_points()
  lo, hi = points.min(0).astype(np.float64), points.max(0).astype(np.float64)
  pad = flags.margin * (hi - lo)
  lo, hi = lo - pad, hi + pad
  res = tuple(flags.resolution * 3 if len(flags.resolution) == 1 else flags.resolution)
  alpha_app = app_id if model.use_alpha_condition else None
  normals, normals_npy = None, None
  if flags.normals:   # the same sigma bits as density_grid, and the normals of the same voxels
    sigma, normals = evaluation.normal_grid(model, target, lo, hi, res, level=flags.level, warp_id=warp_id, appearance_id=alpha_app,
                                            warp_extra=state.warp_extra)
    normals_npy = os.path.join(exp_dir, f'normals_{name}.npy')
    np.save(normals_npy, np.ascontiguousarray(normals.cpu().numpy()))
  else:
    sigma = evaluation.density_grid(model, target, lo, hi, res, level=flags.level, warp_id=warp_id, appearance_id=alpha_app,
                                    warp_extra=state.warp_extra)
  grid = sigma.cpu().numpy()
  npy = os.path.join(exp_dir, f'density_{name}.npy')
  np.save(npy, np.ascontiguousarray(grid))

  # voxel centres over the threshold, coloured by a full query along one view direction
  idx = torch.nonzero(sigma > flags.threshold)                       # (M, 3) voxel indices (i, j, k)
  step = torch.tensor([(h - l) / r for l, h, r in zip(lo, hi, res)], dtype=torch.float64, device=sigma.device)
  centres = (torch.tensor(lo, dtype=torch.float64, device=sigma.device) + (idx.double() + 0.5) * step).float()
  rgb = torch.zeros(0, 3, device=sigma.device)
  if idx.shape[0] > 0:
    metadata = {}
    for key, val in (('warp', warp_id), ('appearance', app_id), ('camera', cam_id)):
      if val is not None:
        metadata[key] = torch.tensor([[int(val)]], dtype=torch.int32, device=sigma.device)
    view = torch.tensor([VIEW_DIRECTION], dtype=torch.float32, device=sigma.device)
    parts = []
    for first in range(0, centres.shape[0], 1 << 21):
      out = model.query_points(target, centres[first:first + (1 << 21)], viewdirs=view, metadata=metadata, warp_extra=state.warp_extra,
                               level=flags.level, use_warp=use_warp, outputs=('rgb',))
      parts.append(out['rgb'])
    rgb = torch.cat(parts, 0)
  ply = os.path.join(exp_dir, f'density_{name}.ply')
  write_ply(ply, centres.cpu().numpy(), rgb.cpu().numpy(),
            None if normals is None else normals[idx[:, 0], idx[:, 1], idx[:, 2]].cpu().numpy())
  print(f'density_{name}: {res[0]} x {res[1]} x {res[2]} voxels over [{lo.round(4).tolist()}, {hi.round(4).tolist()}], sigma in '
        f'[{grid.min():.4g}, {grid.max():.4g}], {idx.shape[0]} voxels over {flags.threshold:g} -> {npy}, {ply}', flush=True)
  ret = {'npy': npy, 'ply': ply, 'resolution': res, 'num_vertices': int(idx.shape[0]), 'bbox': (lo, hi)}
  if normals_npy is not None:
    ret['normals_npy'] = normals_npy
  if flags.mesh:
    clean = None   # --mesh_keep all without a triangle floor: the mesh as it always was
    if flags.mesh_keep != 'all' or flags.mesh_min_triangles > 0:
      clean = dict(keep=flags.mesh_keep, min_triangles=flags.mesh_min_triangles)
    mesh = evaluation.extract_mesh(model, target, lo, hi, res, flags.threshold, level=flags.level, warp_id=warp_id, appearance_id=app_id,
                                   camera_id=cam_id, warp_extra=state.warp_extra, refine_steps=flags.mesh_refine, clean=clean)
    comps = mesh['components'] if clean is not None else evaluation.mesh_components(mesh['vertices'], mesh['faces'], lib=model.lib)
    ret['num_mesh_components'] = print_component_table(name, comps)
    mesh_ply = os.path.join(exp_dir, f'mesh_{name}.ply')
    write_mesh_ply(mesh_ply, *(mesh[k].cpu().numpy() for k in ('vertices', 'normals', 'rgb', 'faces')))
    print(f'mesh_{name}: {mesh["vertices"].shape[0]} vertices, {mesh["faces"].shape[0]} faces at sigma = {flags.threshold:g}, '
          f'{flags.mesh_refine} refine steps -> {mesh_ply}', flush=True)
    ret.update(mesh_ply=mesh_ply, num_mesh_vertices=int(mesh['vertices'].shape[0]), num_mesh_faces=int(mesh['faces'].shape[0]))
    carried = {}
    if flags.animate is not None:
      ret['animated'] = animate(flags, model, target, state.warp_extra, datasource, mesh, alpha_app, exp_dir, carried)
    if flags.render_mesh is not None:
      ret['rendered'] = render_mesh(flags, model, state, datasource, mesh, carried, exp_dir)
  return ret


if __name__ == '__main__':
  main(sys.argv[1:])
