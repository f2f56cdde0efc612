#!/usr/bin/env python
"""Headline benchmark: train rays/s on synthetic 1024-ray x (64+128)-sample batches.

Workload (BASELINE.json configs[1]): configs/gpu_quarterhd.gin shape as measured -- 1024 rays per
GPU, N_c=64 + N_f=128 samples (256 MLP rows per ray), F_p=8, fp32, warp off, stratified sampling,
softplus sigma.  One step = forward + MSE loss + backward (C-ABI nrf_train_step_loss_grad) +
gradient all-reduce over RCCL (N>1) + fused Adam -- i.e. everything training.train_step times.
Inputs (rays, target colours, parameters) are resident in HBM before the timed region.

  python bench.py --gpus N --steps K --warmup W
N>1: one rank per GPU over RCCL.  Under torch.distributed.run (WORLD_SIZE set) the process is a rank; WITHOUT it
`python bench.py --gpus N` re-launches itself under `python -m torch.distributed.run --nnodes=1 --nproc-per-node N
--master-addr 127.0.0.1` (train.py:254-262: jax.pmap over the local devices).  The top-level line is weak scaling (1024 rays
per GPU); with N>1 it also carries a nested `strong_scaling` record -- the north star's 1024-ray GLOBAL batch, 1024/N rays
per GPU, eager and replayed from one hipGraph -- so ONE run yields both curves.  The line checks itself: `rccl_ranks == N`,
`replica_param_checksums_agree`, `grad_allreduce_us` and the exposed (non-overlapped) share of the collective.
A box with fewer devices than ranks (the one-GPU lease the tests run on) still runs the N-rank code path: ranks share
devices and the transport is gloo (RCCL refuses two ranks on one device); the line then says `oversubscribed` and its value is
NOT a scaling measurement.  Rank 0 prints ONE JSON line.

Secondary lines (never the default): --mode train_bf16 | vrig | fullhd | eval, --bf16 (or BENCH_BF16=1) for the bfloat16
NeRF-MLP mode of vrig / fullhd / eval, --rays-per-gpu N (e.g. 128 = one GPU's share of the north star's 1024-ray global batch
on 8 GPUs: the strong-scaling point), --graph (the whole step replayed from one hipGraph).

A plain run does only what the headline figure needs: set-up, burn-in, W warm-up steps, K timed steps, the result line.
--full adds everything else the line used to carry: clock / power sampling, the per-kernel HIP-event profile and roofline, the
replica checks and all-reduce timings of N>1, the strong-scaling record, the CPU baseline and, on the default one-GPU line, the
sustained run, the config-E parity record and the secondary lines.  --dump-outputs DIR writes what the last timed step returned
(train: parameters, Adam moments, gradient, step statistics; eval: the rendered chunk) as DIR/<name>.npy.  The train steps run
at learning rate 0 (BENCH_LR) and start from the same Adam state and key whatever the burn-in did, so every run gives the last
step the same inputs and its outputs agree to rounding: two builds can be compared output for output.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
  sys.path.insert(0, ROOT)

import torch
import torch.distributed as dist

RAYS_PER_GPU = 1024
CPU_MICROBATCH = 128               # rays per microbatch of cpu_baseline's gradient-accumulation candidates
N_COARSE, N_FINE, POINT_FREQS = 64, 128, 8
PEAK_FP32_MFMA_TFLOPS = 157.3   # MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32, dense
PEAK_BF16_MFMA_TFLOPS = 2500.0  # dense bf16 MFMA (the opt-in bf16 modes)
PEAK_HBM_GBS = 8000.0           # HBM3E spec (~6300 achievable)
PEAK_CLOCK_MHZ = 2400.0         # the boost clock the MFMA peaks are quoted at
# profile name -> kernel symbol in profiles/hbm_traffic.json (PMC FETCH_SIZE/WRITE_SIZE of the committed rocprofv3 run).
# Only names that are ONE launch per step are listed (a per-kernel PMC average over two different launches is not a
# per-launch figure): the merged dgrad launches of round 3 qualify, the per-level forward launches do not.
TRAFFIC_KERNEL = {'wgrad': 'nrf::wgrad_kernel', 'wgrad_bf16': 'nrf::wgrad_bf16_kernel', 'mlp_dgrad': 'nrf::nerf_mlp_bwd_kernel',
                  'warp_dgrad': 'nrf::se3_warp_bwd_kernel<false>'}


def kernel_source_sha():
  """sha256[:16] over the HIP sources: profiles/hbm_traffic.json carries the value it was measured at."""
  import hashlib
  h = hashlib.sha256()
  csrc = os.path.join(ROOT, 'nerfies_amd', 'csrc')
  for f in sorted(os.listdir(csrc)):
    if f.endswith(('.hip', '.h')):
      h.update(open(os.path.join(csrc, f), 'rb').read())
  return h.hexdigest()[:16]


def hbm_traffic(profile_name, mode='train'):
  """(HBM bytes per launch of the dominant kernel, provenance) from the committed PMC pass of THIS workload
  (profiles/hbm_traffic.json: {'modes': {mode: {'source', 'kernels': {symbol: {fetch_bytes, write_bytes}}}}}, written by
  scripts/make_hbm_traffic.py: FETCH_SIZE x2 per the gfx950 correction + WRITE_SIZE).  The file records the hash of the
  kernel sources it was measured at; when the sources have changed since, the figure is stale and (None, reason) is
  returned instead."""
  path = os.path.join(ROOT, 'profiles', 'hbm_traffic.json')
  sym = TRAFFIC_KERNEL.get(profile_name)
  if sym is None or not os.path.exists(path):
    return None, 'no PMC pass committed for this kernel'
  rec = json.load(open(path))
  modes = rec.get('modes') or {'train': {'kernels': rec.get('kernels', {}), 'source': rec.get('source')}}
  m = modes.get(mode)
  if m is None:
    return None, f'no PMC pass committed for the {mode} workload'
  k = m.get('kernels', {}).get(sym)
  if k is None:
    return None, 'kernel not in profiles/hbm_traffic.json'
  if rec.get('csrc_sha16') != kernel_source_sha():
    return None, f"stale: measured at csrc {rec.get('csrc_sha16')}, sources are now {kernel_source_sha()}"
  return k['fetch_bytes'] + k['write_bytes'], m.get('source') or rec.get('source', 'profiles/hbm_traffic.json')


class ClockSampler:
  """Shader clock / board power of the bench GPU, sampled from sysfs (amdgpu hwmon: freq1_input Hz, power1_average or
  power1_input uW) on a background thread, so a sub-second timed window can be shown to sit in a steady state."""

  def __init__(self, index=0, period=0.05):
    import glob
    self.files = {}
    cards = sorted(glob.glob('/sys/class/drm/card[0-9]*/device/hwmon/hwmon*'))
    self.card = None
    try:   # the card whose PCI address is the bench device's (a box exposes many cards, one of them visible to HIP)
      pr = torch.cuda.get_device_properties(index)
      want = f'{pr.pci_domain_id:04x}:{pr.pci_bus_id:02x}:{pr.pci_device_id:02x}'
      match = [c for c in cards if want in os.path.realpath(os.path.join(c, '..', '..'))]
      cards = match or cards
      self.card = want if match else None
    except (AttributeError, RuntimeError):
      pass
    if cards:
      hw = cards[0] if self.card else cards[min(index, len(cards) - 1)]
      for key, names in (('sclk_mhz', ['freq1_input']), ('power_w', ['power1_average', 'power1_input'])):
        for n in names:
          if os.path.exists(os.path.join(hw, n)):
            self.files[key] = os.path.join(hw, n)
            break
    self.period, self.samples, self._stop, self._thread = period, {k: [] for k in self.files}, False, None

  def _read(self):
    for k, f in self.files.items():
      try:
        v = float(open(f).read().strip())
        self.samples[k].append(v / 1e6)
      except (OSError, ValueError):
        pass

  def start(self):
    import threading
    self.samples = {k: [] for k in self.files}
    self._stop = False

    def loop():
      while not self._stop:
        self._read()
        time.sleep(self.period)
    self._thread = threading.Thread(target=loop, daemon=True)
    self._thread.start()

  def stop(self):
    self._stop = True
    if self._thread is not None:
      self._thread.join()
    out = {}
    for k, v in self.samples.items():
      if v:
        out[k] = {'min': min(v), 'mean': sum(v) / len(v), 'max': max(v), 'n': len(v)}
    if out:
      out['pci'] = self.card or 'unmatched (first hwmon card)'
    return out or None


def burn_in(step, seconds, world=1, device=None):
  """Untimed steps of the same workload for >= `seconds` (clocks / power settle), in rounds of 16 steps.  A step contains
  the gradient all-reduce, so with world > 1 every rank must run the SAME number of rounds: the decision to go on is itself
  all-reduced (MAX of the ranks' elapsed times)."""
  t0, n = time.perf_counter(), 0
  while True:
    for _ in range(16):
      step()
    torch.cuda.synchronize()
    n += 16
    elapsed = time.perf_counter() - t0
    if world > 1:
      t = torch.tensor([elapsed], device=device, dtype=torch.float64)
      dist.all_reduce(t, op=dist.ReduceOp.MAX)
      elapsed = t.item()
    if elapsed >= seconds:
      return n


class Cfg:
  num_coarse_samples = N_COARSE
  num_fine_samples = N_FINE
  num_nerf_point_freqs = POINT_FREQS
  num_nerf_viewdir_freqs = 4
  sigma_activation = 'softplus'
  use_stratified_sampling = True
  use_viewdirs = True


class CfgVrig(Cfg):   # configs/gpu_vrig_paper.gin: 128+128, F_p=8, SE3 F_w=6 G=8, camera code, elastic + background
  num_coarse_samples, num_fine_samples = 128, 128
  use_warp, num_warp_freqs, num_warp_features, use_camera_metadata = True, 6, 8, True
  warp_field_type = 'se3'


class CfgFullHD(Cfg):   # configs/gpu_fullhd.gin:24-40 + warp_defaults.gin: 256+256, F_p=10, SE3 F_w=8 G=8, appearance ids
  num_coarse_samples, num_fine_samples, num_nerf_point_freqs = 256, 256, 10
  use_warp, num_warp_freqs, num_warp_features, use_appearance_metadata = True, 8, 8, True
  warp_field_type = 'se3'


class CfgEval(Cfg):
  num_coarse_samples, num_fine_samples, use_stratified_sampling = 128, 128, False


class CfgEvalWarp(CfgEval):   # BASELINE.md config E as nerfies renders it (eval.py:330-339): SE3 warp F_w=8, G=8, forward only
  use_warp, num_warp_freqs, num_warp_features, warp_field_type = True, 8, 8, 'se3'


# Learning rate of the benchmarked train steps.  0: every step starts from the same seeded parameters, so what a step computes is
# the same from run to run up to rounding.  With a positive rate it is not: the fine level's float atomics sum in a different order
# on every run, and Adam's normalised update turns those rounding differences into lr-sized parameter moves that grow step after
# step.  The cost of a step does not depend on the rate: Adam still reads and writes every parameter and both moments.
BENCH_LR = 0.0

# training workloads: rays per GPU, model config, regularisers, warp alpha, the gin shape they stand for
NUM_FRAMES = int(os.environ.get('BENCH_FRAMES', 256))   # frames of the synthetic capture: warp / appearance ids per frame

TRAIN_MODES = {
    'train': dict(rays=RAYS_PER_GPU, cfg=Cfg, reg=False, alpha=0.0, metric='train rays/sec (192 samples/ray)',
                  workload='gpu_quarterhd.gin shape: {rays} rays/GPU x (64+128) samples, F_p=8, warp off, stratified, '
                           'fwd+MSE+bwd+grad all-reduce+Adam'),
    'vrig': dict(rays=768, cfg=CfgVrig, reg=True, alpha=6.0, elastic_w=0.001,
                 metric='train rays/sec (256 samples/ray, SE3 warp + elastic + background regularisers)',
                 workload="gpu_vrig_paper.gin shape: {rays} rays/GPU x (128+128) samples, SE3 warp F_w=6 + camera code, elastic "
                          "loss (reduce 'weight', w=0.001) on the coarse samples, 16384 background points per GPU (w=1), stratified"),
    'fullhd': dict(rays=512, cfg=CfgFullHD, reg=True, alpha=8.0, elastic_w=0.01,
                   metric='train rays/sec (512 samples/ray, SE3 warp + elastic + background regularisers)',
                   workload="gpu_fullhd.gin shape: {rays} rays/GPU (4096 global on 8) x (256+256) samples, F_p=10, SE3 warp F_w=8, "
                            "appearance + warp ids, elastic loss (reduce 'weight', w=0.01) on the coarse samples, 16384 background "
                            'points per GPU (w=1), stratified'),
}
TRAIN_MODES['train_bf16'] = dict(TRAIN_MODES['train'], force_bf16=True)
BF16_NOTE_MLP = (' [opt-in bf16 mode, NeRF MLPs only: bfloat16 NeRF-MLP operands and activation / dY stash; fp32 master weights, posenc, '
                 'SE3 warp field and its regularisers, compositing, loss, all-reduce, Adam]')
BF16_NOTE_ALL = (' [opt-in bf16 mode: bfloat16 operands and activation / dY stash of the NeRF MLPs and of the SE3 trunk; fp32 master '
                 'weights, posenc, exp_se3 / Jacobian algebra / regularisers, GLO tables, compositing, loss, all-reduce, Adam]')


DUMP_LIMIT_BYTES = 64 << 20


def _leaves(tree, prefix=''):
  """(dotted name, tensor) of every tensor in a nested dict; '/' in a key (the stats' 'loss/rgb') becomes '_'."""
  for k, v in tree.items():
    name = prefix + str(k).replace('/', '_')
    if isinstance(v, dict):
      yield from _leaves(v, name + '.')
    elif torch.is_tensor(v):
      yield name, v


def dump_outputs(path, arrays, limit=DUMP_LIMIT_BYTES):
  """--dump-outputs: every {name: tensor} as <path>/<name>.npy, float64 kept, everything else as float32.  If the arrays
  together exceed `limit` bytes, each array above an even share of it is replaced by a fixed sample of its flattened elements
  (positions drawn by a generator seeded from the name, sorted, written as <name>.index.npy), so two runs write the same
  positions.  Returns {name: number of elements written}."""
  import zlib
  import numpy as np
  os.makedirs(path, exist_ok=True)
  arrs = {}
  for name, t in arrays.items():
    a = t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    arrs[name] = a.astype(np.float64 if a.dtype == np.float64 else np.float32)
  share = limit // max(len(arrs), 1)
  sampled = sum(a.nbytes for a in arrs.values()) > limit
  written = {}
  for name, a in arrs.items():
    if sampled and a.nbytes > share:
      k = share // (a.itemsize + 8)   # the float64 index costs 8 bytes per element
      idx = np.sort(np.random.default_rng(zlib.crc32(name.encode())).choice(a.size, k, replace=False))
      np.save(os.path.join(path, name + '.index.npy'), idx.astype(np.float64))
      a = a.reshape(-1)[idx]
    np.save(os.path.join(path, name + '.npy'), a)
    written[name] = int(a.size)
  return written


def synthetic_batch(n, seed, device):
  g = torch.Generator(device='cpu').manual_seed(seed)
  o = torch.rand(n, 3, generator=g) - 0.5
  d = torch.randn(n, 3, generator=g)
  d = d / d.norm(dim=-1, keepdim=True)
  rgb = torch.rand(n, 3, generator=g)
  return {'origins': o.to(device), 'directions': d.to(device), 'rgb': rgb.to(device), 'metadata': {}}


_CPU_W = {}


def _cpu_worker_init(threads):
  """Worker of cpu_baseline's process-parallel candidate: its own copy of the oracle model and of the (seeded) batch."""
  from oracle import nerfies_oracle as O
  torch.set_num_threads(threads)
  spec = O.ModelSpec(num_coarse_samples=N_COARSE, num_fine_samples=N_FINE, num_nerf_point_freqs=POINT_FREQS,
                     use_stratified_sampling=True)
  n = RAYS_PER_GPU
  g = torch.Generator().manual_seed(0)
  _CPU_W.update(O=O, spec=spec, params=O.init_params(spec, seed=0, dtype=torch.float32),
                batch=O.synthetic_batch(n, seed=0, dtype=torch.float32), t_rand=torch.rand(n, N_COARSE, generator=g),
                u=torch.rand(n, N_FINE, generator=g))


def _cpu_worker_grads(job):
  i0, i1, values = job
  O, W = _CPU_W['O'], _CPU_W
  for (_, t), val in zip(O.tree_leaves_with_path(W['params']), values):
    t.copy_(val)
  cut = lambda t: t[i0:i1] if torch.is_tensor(t) else {k: cut(x) for k, x in t.items()}
  _, _, grads, _ = O.loss_and_grad(W['params'], W['spec'], cut(W['batch']), t_rand=W['t_rand'][i0:i1], u=W['u'][i0:i1])
  return [gt for _, gt in O.tree_leaves_with_path(grads)]


def cpu_baseline(seconds_budget=24.0):
  """The oracle's torch-CPU fp32 restatement of the same train step ("reference restated on CPU": JAX is not installable here,
  BASELINE.md plan B) on the SAME batch as the GPU line: 1024 rays x (64+128), fwd + bwd + Adam (training.py:138-271).

  Three ways to run that one step are timed and the fastest is the reported value (round 5 timed only the first and understated
  the CPU by 2.3x or more):
    full       one autograd graph over all 1024 rays (peak memory ~20 GB; torch's intra-op pool scales poorly on it);
    microbatch 8 x 128 rays (CPU_MICROBATCH) with gradient ACCUMULATION -- the loss is a mean over rays (training.py:172), so the sum of the
               microbatch gradients / 8 is the full-batch gradient: the same optimizer step, cache-sized graphs;
    processes  the same 8 microbatches dealt to P worker processes of T threads each (P x T <= the host's cores): what a host
               with more cores than torch's intra-op pool can use gives; skipped on hosts with < 2 x T cores.
  Thread counts are probed on the microbatch shape (0.2-0.5 s a probe) and the best is used for both; `cores` = the threads
  used, `cores_available` = os.cpu_count().  Bounded: ~25 s of CPU work on a 64+-core host."""
  from oracle import nerfies_oracle as O
  spec = O.ModelSpec(num_coarse_samples=N_COARSE, num_fine_samples=N_FINE, num_nerf_point_freqs=POINT_FREQS,
                     use_stratified_sampling=True)
  params = O.init_params(spec, seed=0, dtype=torch.float32)
  leaves = [t for _, t in O.tree_leaves_with_path(params)]
  m = [torch.zeros_like(t) for t in leaves]
  v = [torch.zeros_like(t) for t in leaves]
  counter = [0]
  n, mb = RAYS_PER_GPU, CPU_MICROBATCH
  batch = O.synthetic_batch(n, seed=0, dtype=torch.float32)
  g = torch.Generator().manual_seed(0)
  t_rand = torch.rand(n, N_COARSE, generator=g)
  u = torch.rand(n, N_FINE, generator=g)

  def shard(i0, i1):
    cut = lambda t: t[i0:i1] if torch.is_tensor(t) else {k: cut(x) for k, x in t.items()}
    return cut(batch), t_rand[i0:i1], u[i0:i1]

  def grads_of(i0, i1):
    b, tr, uu = shard(i0, i1)
    _, _, grads, _ = O.loss_and_grad(params, spec, b, t_rand=tr, u=uu)
    return [gt for _, gt in O.tree_leaves_with_path(grads)]

  def adam(gs, scale=1.0):
    for j, gt in enumerate(gs):
      p, m[j], v[j] = O.adam_update(leaves[j], m[j], v[j], gt * scale if scale != 1.0 else gt, counter[0], 1e-3)
      leaves[j].copy_(p)
    counter[0] += 1

  def step_full():
    t0 = time.perf_counter()
    adam(grads_of(0, n))
    return time.perf_counter() - t0

  def step_micro():
    t0 = time.perf_counter()
    acc = None
    for i0 in range(0, n, mb):
      gs = grads_of(i0, i0 + mb)
      acc = gs if acc is None else [a.add_(b) for a, b in zip(acc, gs)]
    adam(acc, mb / n)
    return time.perf_counter() - t0

  def probe():
    t0 = time.perf_counter()
    grads_of(0, mb)
    return time.perf_counter() - t0

  ncpu = os.cpu_count() or 1
  best_t, best_threads, probed = None, 1, {}
  for th in sorted({c for c in (4, 8, 16, 32, 64, ncpu) if c <= ncpu}):
    torch.set_num_threads(th)
    probe()                       # warm-up at this thread count
    t = min(probe(), probe())
    probed[th] = round(mb / t, 1)
    if best_t is None or t < best_t:
      best_t, best_threads = t, th
    if t > 3 * best_t:            # clearly past the scaling knee
      break
  if os.environ.get('BENCH_CPU_THREADS'):   # tests: pin the per-process thread count (exercises the worker-process candidate)
    best_threads = int(os.environ['BENCH_CPU_THREADS'])
  torch.set_num_threads(best_threads)

  def timed(fn, budget, at_least, at_most):
    fn()                          # warm-up at this shape (allocator, thread pool)
    ts, t0 = [], time.perf_counter()
    while len(ts) < at_least or (time.perf_counter() - t0 < budget and len(ts) < at_most):
      ts.append(fn())
    ts.sort()
    return ts[len(ts) // 2], len(ts)
  t_micro, n_micro = timed(step_micro, 0.45 * seconds_budget, 2, 12)
  t_full, n_full = timed(step_full, 0.35 * seconds_budget, 1, 6)
  cands = {'microbatch_grad_accumulation': {'microbatches': f'{n // mb} x {mb} rays', 'rays_per_s': n / t_micro, 'steps_timed': n_micro, 'cores_used': best_threads},
           'full_batch_one_graph': {'rays_per_s': n / t_full, 'steps_timed': n_full, 'cores_used': best_threads}}
  # ---- candidate 3: the microbatches in parallel worker processes ----
  nproc = min(n // mb, ncpu // best_threads)
  if nproc >= 2 and not os.environ.get('BENCH_CPU_NO_PROCS'):
    pool = None
    try:
      import concurrent.futures as cf
      import multiprocessing as mp
      # spawn: fork is not an option in a process that holds a HIP context.  ProcessPoolExecutor (not mp.Pool, which respawns a
      # worker whose initializer fails for ever) + a deadline on every result: a host that cannot run workers costs seconds
      pool = cf.ProcessPoolExecutor(nproc, mp_context=mp.get_context('spawn'), initializer=_cpu_worker_init, initargs=(best_threads,))
      deadline = 60.0 + 4.0 * t_micro

      def step_procs():
        t0 = time.perf_counter()
        futs = [pool.submit(_cpu_worker_grads, (i0, i0 + mb, [t.clone() for t in leaves])) for i0 in range(0, n, mb)]
        acc = None
        for f in futs:
          gs = f.result(timeout=deadline)
          acc = gs if acc is None else [a.add_(b) for a, b in zip(acc, gs)]
        adam(acc, mb / n)
        return time.perf_counter() - t0
      t_procs, n_procs = timed(step_procs, 0.2 * seconds_budget, 2, 12)
      cands[f'microbatch_in_{nproc}_processes'] = {'rays_per_s': n / t_procs, 'steps_timed': n_procs,
                                                         'cores_used': nproc * best_threads}
    except Exception as e:   # noqa: BLE001  (a host that cannot spawn workers still reports the in-process candidates)
      cands['microbatch_in_processes'] = {'error': f'{type(e).__name__}: {e}'[:200], 'rays_per_s': 0.0, 'cores_used': 0}
    finally:
      if pool is not None:
        procs = list(getattr(pool, '_processes', {}).values())
        pool.shutdown(wait=False, cancel_futures=True)
        for pr in procs:   # the exact worker processes this pool started
          if pr.is_alive():
            pr.terminate()
  variant = max(cands, key=lambda k: cands[k]['rays_per_s'])
  best_threads = cands[variant]['cores_used']
  return {'value': cands[variant]['rays_per_s'], 'unit': 'rays/s', 'cores': best_threads, 'cores_used': best_threads,
          'cores_available': ncpu, 'kind': 'port', 'variant': variant, 'candidates': cands,
          'thread_probe_rays_per_s_on_128_rays': probed,
          'sample': f'{n} rays x ({N_COARSE}+{N_FINE}) samples (the full GPU batch), fwd+bwd+Adam, fp32 torch-CPU oracle; '
                    f'reported = the fastest of {sorted(cands)} (median step of each), {best_threads} of {ncpu} host threads '
                    f'(thread count per process: best of a probe on 128 rays)'}


def eval_parity(dev, num_rays=256, threads=32):
  """The parity half of BASELINE's metric ("...; eval PSNR vs reference") in the driver-run line: `num_rays` deterministic rays of
  config E (the video-render shape as eval.py renders it: 128+128 samples, SE3 warp F_w=8 G=8, deterministic sampling,
  eval.py:239) rendered by the HIP path in float32 and by the float64 oracle (the checker leg the contract allows the oracle in)
  from the same trained-like parameters.  max-abs differences of rgb / depth / acc at both levels and the PSNR of the HIP frame
  against the oracle's (north star: rgb / depth within 1e-3).  Outside every timed region."""
  from oracle import nerfies_oracle as O
  from nerfies_amd import models, params as P
  import types
  t0 = time.perf_counter()
  spec = O.ModelSpec(num_coarse_samples=128, num_fine_samples=128, num_nerf_point_freqs=8, use_stratified_sampling=False,
                     use_warp=True, num_warp_freqs=8, num_warp_features=8, num_warp_embeddings=4)
  p64 = O.init_params(spec, seed=51, trained_like=True, dtype=torch.float64)
  b64 = O.synthetic_batch(num_rays, seed=52, dtype=torch.float64)
  cfg = types.SimpleNamespace(num_coarse_samples=128, num_fine_samples=128, num_nerf_point_freqs=8, num_nerf_viewdir_freqs=4,
                              sigma_activation='softplus', use_stratified_sampling=False, use_viewdirs=True, use_warp=True,
                              num_warp_freqs=8, num_warp_features=8, warp_field_type='se3')
  ids = list(range(spec.num_warp_embeddings))
  model, fp = models.construct_nerf(0, cfg, num_rays, ids, [0, 1], ids, spec.near, spec.far, device=dev)
  P.flat_from_tree(O.tree_map(lambda t: t.float(), p64), model.layout, dev, out=fp.flat)
  rays = {'origins': b64['origins'].to(dev).float(), 'directions': b64['directions'].to(dev).float(),
          'metadata': {'warp': b64['metadata']['warp'].to(dev)}}
  alpha = 8.0
  out = model.apply({'params': fp}, rays, {'alpha': alpha})
  out_x3 = model.apply({'params': fp}, rays, {'alpha': alpha}, bf16='x3')   # the split-bf16 (float32-emulating) chains on the same rays
  torch.cuda.synchronize()
  prev = torch.get_num_threads()
  torch.set_num_threads(max(1, min(threads, os.cpu_count() or 1)))
  try:
    with torch.no_grad():
      ref = O.nerf_model_apply(p64, spec, {'origins': b64['origins'], 'directions': b64['directions'],
                                           'metadata': {'warp': b64['metadata']['warp']}}, warp_alpha=alpha)
  finally:
    torch.set_num_threads(prev)
  err = {lv: {k: float((out[lv][k].cpu().double() - ref[lv][k]).abs().max()) for k in ('rgb', 'depth', 'acc')}
         for lv in ('coarse', 'fine')}
  mse = float(((out['fine']['rgb'].cpu().double() - ref['fine']['rgb']) ** 2).mean())
  import math
  worst = max(max(v.values()) for v in err.values())
  err3 = {lv: {k: float((out_x3[lv][k].cpu().double() - ref[lv][k]).abs().max()) for k in ('rgb', 'depth', 'acc')} for lv in ('coarse', 'fine')}
  mse3 = float(((out_x3['fine']['rgb'].cpu().double() - ref['fine']['rgb']) ** 2).mean())
  x3 = {'mode': 'NRF_FLAG_BF16X3: split-bf16 NeRF chains and SE3 trunk', 'max_abs_rgb': err3['fine']['rgb'], 'max_abs_depth': err3['fine']['depth'],
        'max_abs_acc': err3['fine']['acc'], 'max_abs_coarse': err3['coarse'], 'psnr_vs_oracle_db': (-10.0 * math.log10(mse3)) if mse3 > 0 else float('inf'),
        'max_abs_rgb_vs_f32_path': float((out_x3['fine']['rgb'] - out['fine']['rgb']).abs().max()),
        'pass': bool(max(max(v.values()) for v in err3.values()) <= 1e-3)}
  return {'rays': num_rays, 'bf16x3': x3, 'workload': 'config E (eval.py render): 128+128 samples, SE3 warp F_w=8 G=8 alpha=8, deterministic, fp32',
          'against': 'float64 oracle (oracle/nerfies_oracle.py, pinned to the reference-run vectors tests/golden/ref_*.npz)',
          'max_abs_rgb': err['fine']['rgb'], 'max_abs_depth': err['fine']['depth'], 'max_abs_acc': err['fine']['acc'],
          'max_abs_coarse': err['coarse'], 'psnr_vs_oracle_db': (-10.0 * math.log10(mse)) if mse > 0 else float('inf'),
          'tolerance': 1e-3, 'pass': bool(worst <= 1e-3), 'seconds': time.perf_counter() - t0}


def secondary_lines(args, ctx):
  """The other BASELINE configs on the same box, in the same driver-run line (round 5: only the builder's own runs had them):
  vrig fp32 (configs[2] shape), fullhd bf16 (configs[3], the precision BASELINE names for it), eval with the SE3 warp fp32
  (configs[4]): a short burn-in, 10 timed steps each, the dominant kernel's roofline.  Outside the headline's timed region."""
  out = []
  sa = argparse.Namespace(**dict(vars(args), burn_in_s=0.5, steps=10, warmup=3))
  for mode, bf16 in (('vrig', False), ('fullhd', True)):
    t0 = time.perf_counter()
    try:
      M = TRAIN_MODES[mode]
      r = train_workload(sa, M, M['cfg'], M['rays'], bf16, False, ctx)
      roof, _ = roofline_of(r['prof'], bf16, mode + ('_bf16' if bf16 else ''), M['rays'], M['cfg'])
      at_clock(roof, r['clocks'])
      step_flops = sum(e['flops_per_launch'] * e['launches'] for e in r['prof']) / r['prof_steps']
      out.append({'mode': mode, 'dtype': 'bf16' if bf16 else 'f32', 'value': r['value'], 'unit': 'rays/s', 'ms_per_step': r['ms_per_step'],
                  'steps': sa.steps, 'rays_per_gpu': M['rays'], 'step_tflops': step_flops / (r['ms_per_step'] * 1e-3) / 1e12,
                  'roofline': {k: roof.get(k) for k in ('bound', 'kernel', 'achieved', 'peak', 'unit', 'frac', 'kernel_ms', 'frac_at_clock')},
                  'kernels_ms': {k: round(v['ms'] * v['launches_per_step'], 4) for k, v in kernel_table(r['prof'], r['prof_steps']).items()},
                  'final_loss_fine': r['loss'], 'seconds': time.perf_counter() - t0})
    except Exception as e:   # noqa: BLE001  (a secondary line must never take the headline down)
      out.append({'mode': mode, 'dtype': 'bf16' if bf16 else 'f32', 'error': f'{type(e).__name__}: {e}'[:300]})
    torch.cuda.empty_cache()
  # eval (configs[4]): with the SE3 warp in float32 (what eval.py renders), and the split-bf16 (float32-emulating) mode without and
  # with the warp (NRF_FLAG_BF16X3: NeRF chains and SE3 trunk)
  for mode, warp, prec, dtype in (('eval_warp', True, False, 'f32'), ('eval_x3', False, 'x3', 'bf16x3 (fp32-emulating)'),
                                  ('eval_warp_x3', True, 'x3', 'bf16x3 (fp32-emulating)')):
    t0 = time.perf_counter()
    try:
      ea = argparse.Namespace(**dict(vars(args), burn_in_s=0.5, steps=10, warmup=2, warp=warp, frame=False))
      line = eval_mode(ea, ctx['world'], ctx['rank'], ctx['dev'], prec, emit=False)
      out.append({'mode': mode, 'dtype': dtype, 'value': line['value'], 'unit': 'rays/s', 'ms_per_step': line['ms_per_step'],
                  'steps': ea.steps, 'rays_per_gpu': 8192, 'step_tflops': line['step_tflops'],
                  'roofline': {k: line['roofline'].get(k) for k in ('bound', 'kernel', 'achieved', 'peak', 'unit', 'frac', 'kernel_ms', 'frac_at_clock')},
                  'seconds': time.perf_counter() - t0})
    except Exception as e:   # noqa: BLE001
      out.append({'mode': mode, 'dtype': dtype, 'error': f'{type(e).__name__}: {e}'[:300]})
    torch.cuda.empty_cache()
  torch.cuda.empty_cache()
  return out


def rccl_preflight_begin(rank):
  """Before init_process_group('nccl'): have RCCL write its INIT / GRAPH log of this rank to a file, so the bench line can say
  what the communicator actually uses (xGMI P2P vs SHM vs NET), next to `rccl_ranks`.  Leaves an explicit NCCL_DEBUG alone."""
  import tempfile
  if os.environ.get('NCCL_DEBUG') and not os.environ.get('NCCL_DEBUG_FILE'):
    return None   # the user wants the log on the console
  d = tempfile.mkdtemp(prefix='bench_rccl_')
  os.environ.setdefault('NCCL_DEBUG', 'INFO')
  os.environ.setdefault('NCCL_DEBUG_SUBSYS', 'INIT,GRAPH,ENV')
  os.environ.setdefault('NCCL_DEBUG_FILE', os.path.join(d, f'rank{rank}.log'))
  return os.environ['NCCL_DEBUG_FILE']


def rccl_preflight_summary(path):
  """What RCCL logged while the communicator came up (parsed, bounded): transports of the channel connections, channel
  count, rank count, the warnings.  None when no log was captured."""
  import re
  if not path:
    return None
  if not os.path.exists(path):   # say what is there instead (RCCL appends nothing to the name unless it holds %h / %p)
    d = os.path.dirname(path)
    return {'log_lines': 0, 'missing': path, 'dir': sorted(os.listdir(d))[:8] if os.path.isdir(d) else None,
            'NCCL_DEBUG': os.environ.get('NCCL_DEBUG'), 'NCCL_DEBUG_FILE': os.environ.get('NCCL_DEBUG_FILE')}
  try:
    text = open(path, errors='replace').read()
  except OSError as e:
    return {'log_lines': 0, 'error': str(e)[:200]}
  lines = text.splitlines()
  via = {}
  for m in re.finditer(r'\bvia\s+([A-Za-z0-9_/\-]+)', text):
    via[m.group(1)] = via.get(m.group(1), 0) + 1
  chan = re.findall(r'(\d+) coll channels', text)
  nranks = re.findall(r'nranks (\d+)', text)
  xgmi = len(re.findall(r'XGMI', text, flags=re.I))
  warns = [l.split('NCCL WARN', 1)[1].strip()[:160] for l in lines if 'NCCL WARN' in l][:5]
  envs = sorted({m.group(1) for m in re.finditer(r'NCCL INFO (NCCL_[A-Z0-9_]+|RCCL_[A-Z0-9_]+) set', text)})[:12]
  ver = re.search(r'(RCCL version[^\n]*|NCCL version[^\n]*)', text)
  return {'log_lines': len(lines), 'version_line': ver.group(1).strip()[:120] if ver else None,
          'nranks_seen': sorted(set(int(x) for x in nranks)), 'coll_channels': sorted(set(int(c) for c in chan)),
          'connections_via': via, 'xgmi_mentions': xgmi, 'warnings': warns, 'env_overrides': envs,
          'init_complete': bool(re.search(r'Init COMPLETE|init complete', text, flags=re.I))}


def kernel_table(prof, nsteps):
  return {e['name']: {'ms': e['ms'] / max(e['launches'], 1), 'launches_per_step': e['launches'] / nsteps,
                      'tflops': (e['flops_per_launch'] / (e['ms'] / max(e['launches'], 1) * 1e-3) / 1e12)
                      if e['flops_per_launch'] > 0 and e['ms'] > 0 else None} for e in prof}


def roofline_of(prof, bf16, mode_key, rays_per_gpu, cfg):
  """Roofline entry of the dominant kernel (largest accumulated time among the kernels that carry algorithmic flops)."""
  mf = [e for e in prof if e['flops_per_launch'] > 0]
  dom = max(mf, key=lambda e: e['ms'])
  dom_ms = dom['ms'] / dom['launches']
  achieved = dom['flops_per_launch'] / (dom_ms * 1e-3) / 1e12
  traffic, traffic_src = hbm_traffic(dom['name'], mode_key)
  # the NeRF-MLP kernels run on bf16 MFMA in the bf16 modes, and so does the SE3 trunk unless --warp-f32 keeps it in float32
  # (bf16 == 'mlp'); the fp32 wgrad kernel never does
  on_bf16 = bool(bf16) and (dom['name'].startswith('mlp_') or (bf16 not in ('mlp', 'x3mlp') and dom['name'].startswith('warp_')))
  peak_tf = PEAK_BF16_MFMA_TFLOPS if on_bf16 else PEAK_FP32_MFMA_TFLOPS
  if on_bf16 and bf16 in ('x3', 'x3mlp'):
    # split-bf16: the ALGORITHMIC flops of the layer (what `achieved` counts) cost three bf16 MFMAs each (hi.hi + lo.hi + hi.lo)
    peak_tf = PEAK_BF16_MFMA_TFLOPS / 3.0
  r = {'bound': 'mfma', 'kernel': dom['name'], 'achieved': achieved, 'peak': peak_tf, 'unit': 'TFLOP/s', 'frac': achieved / peak_tf,
       'traffic': traffic, 'traffic_source': traffic_src, 'kernel_ms': dom_ms, 'flops_per_launch': dom['flops_per_launch']}
  if dom['name'] == 'wgrad_bf16':
    # HBM-bound: the kernel's algorithmic traffic is both bf16 stashes read once -- per MLP row X = posenc 64 + h1..h8 8x256 +
    # bottleneck 256 + rgb hidden 128 features, dY = dpre0..7 8x256 + d bottleneck 256 + d rgb hidden 128 + d raw 4, 2 B each
    rows = rays_per_gpu * (2 * cfg.num_coarse_samples + cfg.num_fine_samples)
    alg_bytes = rows * 2 * ((64 + 8 * 256 + 256 + 128) + (8 * 256 + 256 + 128 + 4))
    if getattr(cfg, 'use_warp', False) and bf16 != 'mlp':
      # + the SE3 trunk's stashes of every pass through the field: coarse + fine samples, 16384 background points, 3 tangents per
      # coarse sample; per row X = trunk input (3 + 6 F_w + G) + h1..h6 6x128, dY = dpre0..5 6x128 + (dw, dv) 6
      win = 3 + 6 * cfg.num_warp_freqs + cfg.num_warp_features
      wrows = rows + 16384 + 3 * rays_per_gpu * cfg.num_coarse_samples
      alg_bytes += wrows * 2 * ((win + 6 * 128) + (6 * 128 + 6))
    gbs = alg_bytes / (dom_ms * 1e-3) / 1e9
    r = {'bound': 'hbm', 'kernel': dom['name'], 'achieved': gbs, 'peak': PEAK_HBM_GBS, 'unit': 'GB/s', 'frac': gbs / PEAK_HBM_GBS,
         'traffic': traffic, 'traffic_source': traffic_src, 'kernel_ms': dom_ms, 'bytes_per_launch': alg_bytes}
  return r, peak_tf


def at_clock(roofline, clocks):
  """The MFMA peak of the guide is quoted at the 2.4 GHz boost clock.  The bf16 chain kernels pull the board to its 1.4 kW
  limit and the shader clock drops (1.9-2.0 GHz measured), so `frac` (against the guide's peak, as the contract asks) understates
  how busy the matrix pipe is; `frac_at_clock` = achieved / (peak x measured clock / 2400 MHz) says that.  Extra keys only."""
  mhz = ((clocks or {}).get('sclk_mhz') or {}).get('mean')
  if roofline.get('bound') == 'mfma' and mhz:
    roofline['sclk_mhz'] = mhz
    roofline['frac_at_clock'] = roofline['achieved'] / (roofline['peak'] * mhz / PEAK_CLOCK_MHZ)


def rccl_version():
  try:
    v = torch.cuda.nccl.version()
    return '.'.join(str(x) for x in v) if isinstance(v, (tuple, list)) else str(v)
  except Exception as e:   # noqa: BLE001
    return f'unavailable ({type(e).__name__})'


def eval_mode(args, world, rank, dev, bf16, emit=True, dump=None):
  """BASELINE configs[4]: the video-render forward, 8192-ray chunks x (128+128), hipGraph replay.  --warp: with the SE3 field
  (the path eval.py actually renders, models.py:251-267: 526.1 MFLOP/ray); --frame: additionally times evaluation.render_image
  on a whole 960x540 frame (chunk scheduling, tail padding, the copy of every chunk into the frame buffer included).
  `dump`: directory for the rendered chunk of the last timed replay (rank 0)."""
  from nerfies_amd import evaluation, models, training
  n = 8192
  cfg = CfgEvalWarp if args.warp else CfgEval
  model, fp = models.construct_nerf(0, cfg, n, list(range(NUM_FRAMES)), [0, 1], list(range(NUM_FRAMES)), 0.0206, 0.826, device=dev)
  rays = {k: v for k, v in synthetic_batch(n, 100 + rank, dev).items() if k != 'rgb'}
  extra = {}
  if args.warp:
    # a rendered frame is ONE camera at one time stamp: every ray of a chunk carries the same warp id
    rays['metadata'] = {'warp': torch.full((n, 1), 3 + rank, dtype=torch.int32, device=dev)}
    extra = {'alpha': 8.0}
  fn = evaluation.GraphedChunkRenderer(model, bf16=bf16)
  box = {}

  def step():
    box['out'] = fn.call_static(0, 1, fp, rays, extra)
  prof_step = lambda: model.apply({'params': fp}, rays, extra, bf16=bf16)   # HIP events cannot be recorded inside a graph replay

  def barrier():
    if world > 1:
      dist.barrier()
    torch.cuda.synchronize()
  if args.burn_in_s > 0:
    burn_in(step, args.burn_in_s, world, dev)
  for _ in range(args.warmup):
    step()
  barrier()
  sampler = ClockSampler((dev.index or 0) if world > 1 else 0) if args.full else None
  if sampler:
    sampler.start()
  t0 = time.perf_counter()
  for _ in range(args.steps):
    step()
  barrier()
  elapsed = time.perf_counter() - t0
  clocks = sampler.stop() if sampler else None
  if world > 1:
    t = torch.tensor([elapsed], device=dev, dtype=torch.float64)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    elapsed = t.item()
  dumped = dump_outputs(dump, dict(_leaves(box['out']))) if dump and rank == 0 else None
  frame = None
  if args.frame:
    # one 960 x 540 frame (the quarter-HD capture of the README) through render_image: 64 chunks of 8192 rays, the last one
    # edge-padded (518400 = 63 x 8192 + 2304); each rank renders its slice of every chunk, one packed all_gather per chunk
    h, w = 540, 960
    fr = {k: v for k, v in synthetic_batch(h * w, 7, dev).items() if k != 'rgb'}
    fr = {k: v.reshape(h, w, 3) for k, v in fr.items() if k != 'metadata'}
    if args.warp:
      fr['metadata'] = {'warp': torch.full((h, w, 1), 3, dtype=torch.int32, device=dev)}
    state = training.TrainState(optimizer=training.Optimizer(fp), warp_alpha=extra.get('alpha', 0.0))
    render = lambda: evaluation.render_image(state, fr, fn, chunk=n)
    render()
    barrier()
    t1 = time.perf_counter()
    for _ in range(3):
      render()
    barrier()
    frame_ms = 1e3 * (time.perf_counter() - t1) / 3
    nchunks = -(-h * w // n)
    chunk_ms = 1e3 * elapsed / args.steps * (1.0 / world if world > 1 else 1.0)
    frame = {'size': [w, h], 'chunks': nchunks, 'frame_ms': frame_ms, 'sum_of_chunk_replays_ms': nchunks * chunk_ms,
             'overhead_frac': frame_ms / (nchunks * chunk_ms) - 1.0 if world == 1 else None,
             'frames_per_s': 1e3 / frame_ms}
  prof = None
  if args.full:
    model.profile_enable(True)
    for _ in range(5):
      prof_step()
    torch.cuda.synchronize()
    prof = model.profile_read()
    model.profile_enable(False)
  if rank == 0:
    ms = 1e3 * elapsed / args.steps
    warp_txt = 'SE3 warp F_w=8 G=8 (one warp id per chunk)' if args.warp else 'warp off'
    line = {
        'metric': 'eval rays/sec (128+128 samples/ray, forward only, hipGraph replay)' + (' [SE3 warp on]' if args.warp else '') +
                  (' [split-bf16 (bf16x3) arithmetic: NeRF MLPs' + (' + SE3 trunk]' if (args.warp and bf16 == 'x3') else ']') if bf16 in ('x3', 'x3mlp') else ' [bf16 MLP operands]' if bf16 else ''),
        'value': world * n * args.steps / elapsed, 'unit': 'rays/s', 'n_gpus': world, 'steps': args.steps, 'warmup': args.warmup,
        'ms_per_step': ms, 'higher_is_better': True, 'scaling': 'weak', 'vs_baseline': None,
        'dtype': ('bf16x3 (fp32-emulating) NeRF MLPs + f32 warp field' if (args.warp and bf16 == 'x3mlp') else 'bf16x3 (fp32-emulating)') if bf16 in ('x3', 'x3mlp') else
                 ('bf16 NeRF MLPs + f32 warp field' if (args.warp and bf16 == 'mlp') else 'bf16') if bf16 else 'f32', 'data': 'synthetic',
        'config': {'workload': f'gpu eval/video shape: 8192-ray chunk x (128+128) samples, F_p=8, {warp_txt}, deterministic, forward only',
                   'rays_per_gpu': n, 'parallelism': f'ray-shard dp{world}'}}
    if prof is not None:
      roofline, peak = roofline_of(prof, bf16, ('eval_warp' if args.warp else 'eval') + ('_x3' if bf16 in ('x3', 'x3mlp') else '_bf16' if bf16 else ''), n, cfg)
      if bf16 in ('x3', 'x3mlp'):
        roofline['peak_note'] = ('dense bf16 MFMA peak / 3: every algorithmic multiply-add is three bf16 MFMAs (hi.hi + lo.hi + hi.lo, fp32 accumulate); '
                                 'the float32 chains it emulates are priced against 157.3 TFLOP/s')
      at_clock(roofline, clocks)
      step_flops = sum(e['flops_per_launch'] * e['launches'] for e in prof) / 5
      line.update({'roofline': roofline, 'step_tflops': step_flops / (ms * 1e-3) / 1e12, 'kernels': kernel_table(prof, 5)})
    line.update({'frame': frame, 'steady_state': {'burn_in_s': args.burn_in_s, 'timed_window_s': elapsed, 'during_timed_window': clocks},
                 'csrc_sha16': kernel_source_sha(), 'full': bool(args.full), 'dumped_outputs': dumped})
    if emit:
      print(json.dumps(line))
    return line
  return None


def free_port():
  import socket
  with socket.socket() as s:
    s.bind(('127.0.0.1', 0))
    return s.getsockname()[1]


def launch_plan(n, argv, ndev, environ=None):
  """(command, environment) that runs THIS script as N ranks on one node: what `python bench.py --gpus N` execs when it was not
  started by torch.distributed.run itself (the reference's jax.pmap over local devices, train.py:254-262, needs no launcher;
  one process per GPU does).  With fewer visible devices than ranks the ranks share devices and the collective transport is
  gloo (RCCL refuses two ranks on one device): the N-rank code path of a one-GPU box, flagged in the line as `oversubscribed`."""
  env = dict(os.environ if environ is None else environ)
  env.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')   # dmabuf IPC: RCCL's P2P setup fails without it on this driver
  env.setdefault('OMP_NUM_THREADS', '4')
  if ndev < n:
    env['BENCH_SAME_DEVICE'] = '1'
    env.setdefault('BENCH_DIST_BACKEND', 'gloo')
    env['BENCH_OVERSUBSCRIBED'] = f'{n} ranks on {ndev} visible device(s)'
  cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', f'--nproc-per-node={n}', '--master-addr', '127.0.0.1',
         '--master-port', str(free_port()), os.path.abspath(__file__)] + list(argv)
  return cmd, env


def self_launch(args, argv):
  import subprocess
  ndev = torch.cuda.device_count()
  if ndev == 0:
    raise SystemExit('bench.py needs a GPU (torch.cuda.device_count() == 0)')
  cmd, env = launch_plan(args.gpus, argv, ndev)
  print('bench.py: not under torch.distributed.run -> ' + ' '.join(cmd[1:8]) + ' ...', file=sys.stderr, flush=True)
  return subprocess.run(cmd, env=env).returncode


def train_workload(args, M, cfg, rays_per_gpu, bf16, graph, ctx, profile=True, dump=None):
  """One training workload measured as the contract says: burn-in, W warm-up steps, K timed steps between barrier +
  synchronize, MAX over ranks; with --full then the self-checks (replica checksums, the collective on its own, the step without
  the collective) and the per-kernel HIP-event profile.  `dump`: directory for what the last timed step returned (rank 0).
  Returns a dict of measurements (every rank; rank 0 prints)."""
  from nerfies_amd import models, training
  world, rank, dev, dist_on = ctx['world'], ctx['rank'], ctx['dev'], ctx['dist_on']
  # metadata ids as a capture has them: one warp / appearance id per FRAME (a vrig capture has a few hundred frames and a batch
  # draws rays uniformly over all of them), two camera ids (left / right rig camera).  Rounds 1-2 drew the ids from 4 frames,
  # which turns the embedding-table gradient into ~800 same-address atomics per table row and step -- an artefact of the
  # synthetic batch, not of the workload.
  frames = list(range(NUM_FRAMES))
  model, fp = models.construct_nerf(0, cfg, rays_per_gpu, frames, [0, 1], frames, 0.0206, 0.826, device=dev)
  state = training.TrainState(optimizer=training.Optimizer(fp), warp_alpha=M['alpha'])
  batch = synthetic_batch(rays_per_gpu, seed=100 + rank, device=dev)   # each rank: its own ray shard
  kw = {}
  if M['reg']:
    sp = training.ScalarParams(learning_rate=BENCH_LR, background_loss_weight=1.0, elastic_loss_weight=M['elastic_w'])
    g = torch.Generator().manual_seed(rank)
    md = {'warp': torch.randint(0, NUM_FRAMES, (rays_per_gpu, 1), generator=g).to(dev)}
    if getattr(cfg, 'use_camera_metadata', False):
      md['camera'] = torch.randint(0, 2, (rays_per_gpu, 1), generator=g).to(dev)
    if getattr(cfg, 'use_appearance_metadata', False):
      md['appearance'] = torch.randint(0, NUM_FRAMES, (rays_per_gpu, 1), generator=g).to(dev)
    batch['metadata'] = md
    # train.py:186-197: min(len(points), n_dev * 16384) points per step, sharded -> 16384 per device
    batch['background_points'] = ((torch.rand(16384, 3, generator=g) - 0.5) * 0.8).to(dev)
    kw = dict(use_elastic_loss=True, elastic_reduce_method='weight', use_background_loss=True)
  else:
    sp = training.ScalarParams(learning_rate=BENCH_LR)
  key = 12345 + rank

  def barrier():
    if dist_on:
      dist.barrier()
    torch.cuda.synchronize()

  box = {'state': state, 'key': key, 'stats': None}
  if graph:
    gstep = training.GraphedTrainStep(model, state, batch, sp, bf16=bf16, **kw)

    def step():
      box['stats'] = gstep(box['key'])
      box['key'] += 1
  else:
    def step():
      box['state'], box['stats'], box['key'] = training.train_step(model, box['key'], box['state'], batch, sp, bf16=bf16, **kw)

  def timed(nsteps):
    barrier()
    t0 = time.perf_counter()
    for _ in range(nsteps):
      step()
    barrier()
    el = time.perf_counter() - t0
    if world > 1:
      t = torch.tensor([el], device=dev, dtype=torch.float64)
      dist.all_reduce(t, op=dist.ReduceOp.MAX)
      el = t.item()
    return el

  # untimed burn-in at the same workload (>= --burn-in-s seconds) so the short timed window below sits at steady-state
  # clocks and power; the sampler keeps running through the timed region
  sampler = ClockSampler(ctx['local_rank'] if world > 1 else 0) if args.full else None
  burn_steps = burn_in(step, args.burn_in_s, world, dev) if args.burn_in_s > 0 else 0
  if burn_steps:
    # the burn-in runs for a time, not for a number of steps: the warm-up and timed steps start again from the initial Adam
    # state and key (the parameters stay the seeded ones at BENCH_LR = 0), so what the last timed step is given does not depend
    # on how many burn-in steps ran
    opt = state.optimizer
    opt.m.zero_()
    opt.v.zero_()
    opt.step = 0
    box['key'] = key
  for _ in range(args.warmup):
    step()
  barrier()
  if sampler:
    sampler.start()
  elapsed = timed(args.steps)
  clocks = sampler.stop() if sampler else None
  state, stats, key = box['state'], box['stats'], box['key']
  dumped = None
  if dump and rank == 0:
    opt = state.optimizer
    dumped = dump_outputs(dump, dict([('params', opt.target.flat), ('adam_m', opt.m), ('adam_v', opt.v), ('grad', opt.grad)] +
                                     [('stats.' + k, v) for k, v in _leaves(stats)]))
  loss = stats['fine']['loss/rgb'].item()
  # every rank applied the same all-reduced gradient to the same initial parameters: the replicas must be BIT-identical.
  # Checked on a checksum of the bits of the parameters and of Adam's first moment, which every step's gradient enters also at
  # BENCH_LR = 0 (the per-rank losses are reported too: the step's statistics are pmean'ed over the ranks, training.py:267, so
  # they agree as well)
  per_rank_loss, replicas_agree = [loss], True
  if dist_on and args.full:
    flat = torch.cat([state.optimizer.target.flat, state.optimizer.m])
    mine = torch.stack([flat.view(torch.int32).to(torch.int64).sum(), (flat.view(torch.int32).to(torch.int64) * 31 % 1000003).sum()])
    both = torch.cat([mine.to(torch.float64), torch.tensor([loss], device=dev, dtype=torch.float64)])
    allr = [torch.empty_like(both) for _ in range(dist.get_world_size())]
    dist.all_gather(allr, both)
    per_rank_loss = [float(a[2]) for a in allr]
    replicas_agree = all(bool((a[:2] == allr[0][:2]).all()) for a in allr)
    if not replicas_agree:
      raise SystemExit(f'rank {rank}: parameter replicas diverged across ranks: checksums {[a[:2].tolist() for a in allr]}')

  # ---- the gradient all-reduce on its own (outside the timed region): the fused [grad | stats] buffer, 20 calls ----
  allreduce_us = exposed_us = None
  if dist_on and args.full:
    buf = torch.zeros_like(state.optimizer._gs)
    for _ in range(5):
      dist.all_reduce(buf)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    barrier()
    e0.record()
    for _ in range(20):
      dist.all_reduce(buf)
    e1.record()
    torch.cuda.synchronize()
    allreduce_us = e0.elapsed_time(e1) * 1e3 / 20
    if not graph:
      # the exposed share of the collective: the same K steps with the all-reduce taken out (each rank then applies its OWN
      # gradient: the replicas diverge from here on, which is why this runs after the checksum check and nothing below compares
      # ranks).  exposed = t(step) - t(step without the collective); the rest of grad_allreduce_us hides under kernels.
      keep = training.psum_gradients
      training.psum_gradients = lambda grad, st, fused=None: (grad, st.clone(), world)
      try:
        for _ in range(args.warmup):
          step()
        nocomm = timed(args.steps)
      finally:
        training.psum_gradients = keep
      exposed_us = 1e6 * (elapsed - nocomm) / args.steps

  prof, prof_steps = None, 0
  if profile and args.full:
    # per-kernel timing of the SAME step with HIP events on the launch stream (eager: events cannot be recorded inside a
    # graph replay)
    model.profile_enable(True)
    prof_steps = max(5, min(args.steps, 20))
    for _ in range(prof_steps):
      state, stats, key = training.train_step(model, key, state, batch, sp, bf16=bf16, **kw)
    torch.cuda.synchronize()
    prof = model.profile_read()
    model.profile_enable(False)
  return {'elapsed': elapsed, 'ms_per_step': 1e3 * elapsed / args.steps, 'value': world * rays_per_gpu * args.steps / elapsed,
          'loss': loss, 'per_rank_loss': per_rank_loss, 'replicas_agree': replicas_agree, 'allreduce_us': allreduce_us,
          'allreduce_exposed_us': exposed_us, 'allreduce_bytes': 4 * state.optimizer._gs.numel(), 'burn_steps': burn_steps,
          'clocks': clocks, 'prof': prof, 'prof_steps': prof_steps, 'dumped': dumped}


def main(argv=None):
  argv = list(sys.argv[1:] if argv is None else argv)
  ap = argparse.ArgumentParser()
  ap.add_argument('--gpus', type=int, default=1)
  ap.add_argument('--steps', type=int, default=30)
  ap.add_argument('--warmup', type=int, default=5)
  ap.add_argument('--full', action='store_true',
                  help='measure and check everything beyond the headline figure: clock / power sampling, per-kernel profile and '
                       'roofline, replica checks, all-reduce timings and strong scaling (N>1), the CPU baseline and, on the default '
                       'one-GPU line, the sustained run, eval_parity and the secondary lines')
  ap.add_argument('--dump-outputs', metavar='DIR', default=None,
                  help='write what the last timed step returned as DIR/<name>.npy (float32 / float64, at most 64 MB in all)')
  ap.add_argument('--no-cpu-baseline', action='store_true', help='--full: skip the CPU baseline')
  ap.add_argument('--no-extras', action='store_true',
                  help='--full, headline line only: skip eval_parity (config-E HIP vs float64 oracle), the secondary lines (vrig fp32, '
                       'fullhd bf16, eval with the warp) and the sustained run that the default one-GPU line carries')
  ap.add_argument('--sustained-s', type=float, default=5.0, help='seconds of the sustained headline run of the default line')
  ap.add_argument('--burn-in-s', type=float, default=3.0,
                  help='seconds of untimed steps of the same workload before the warm-up + timed steps (steady-state clocks)')
  ap.add_argument('--mode', default='train', choices=['train', 'train_bf16', 'eval', 'vrig', 'fullhd'],
                  help='train: BASELINE configs[1] (default, the headline); eval: configs[4] video-render forward '
                       '(8192-ray chunks x (128+128), hipGraph replay); vrig: configs[2] shape (768 rays/GPU x (128+128), '
                       'SE3 warp F_w=6 + camera code + elastic + background regularisers); fullhd: configs[3] shape (512 rays/GPU x '
                       '(256+256), F_p=10, SE3 warp F_w=8, appearance ids, elastic + background; --bf16 = the precision BASELINE '
                       'names for it); train_bf16: the headline workload with bfloat16 MLP operands and stash (opt-in mode, '
                       'never the default line)')
  ap.add_argument('--bf16', action='store_true', help='vrig / fullhd / eval: NeRF MLPs in the bf16 mode (same as BENCH_BF16=1)')
  ap.add_argument('--rays-per-gpu', type=int, default=0,
                  help='rays per GPU of the training modes (default: the mode\'s own, 1024 for the headline); 128 = one GPU\'s share '
                       'of a 1024-ray global batch on 8 GPUs (the north star\'s strong-scaling point)')
  ap.add_argument('--graph', action='store_true', help='replay the whole train step (loss+grad, all-reduce, Adam) from one hipGraph')
  ap.add_argument('--no-strong', action='store_true', help='N>1: skip the nested strong-scaling record (1024-ray global batch)')
  ap.add_argument('--warp', action='store_true', help='eval mode: render with the SE3 warp field (the path eval.py takes)')
  ap.add_argument('--split-bf16', action='store_true',
                  help='--mode eval: the NeRF MLPs and the SE3 trunk (--warp-f32: the MLPs only) in split-bf16 arithmetic (NRF_FLAG_BF16X3: every float32 operand as a bf16 pair, three bf16 '
                       'MFMAs per product, float32 accumulate -- float32-emulating, ~1e-6 of the float32 chains on rendered colour); the '
                       "line says dtype 'bf16x3 (fp32-emulating)', never 'f32'")
  ap.add_argument('--warp-f32', action='store_true', help='bf16 modes: keep the SE3 trunk in float32 (NRF_FLAG_WARP_F32; the round-3 behaviour)')
  ap.add_argument('--chain-rows', type=int, default=0, choices=[0, 32, 64],
                  help='rows per workgroup tile of the fp32 NeRF chain kernels (NRF_OPT_CHAIN_TILE_ROWS): 0 = the library\'s automatic choice')
  ap.add_argument('--bf16-wgrad-merge', type=int, default=None, choices=[0, 1],
                  help='bf16 training modes: NRF_OPT_BF16_WGRAD_MERGE (1, the library default: skip-layer and bottleneck+alpha weight-gradient '
                       'groups merged, operands streamed once; 0: one group per weight matrix, as rounds 2-4)')
  ap.add_argument('--frame', action='store_true', help='eval mode: also time evaluation.render_image on a whole 960x540 frame')
  args = ap.parse_args(argv)

  if args.bf16_wgrad_merge is not None:
    os.environ['NRF_BF16_WGRAD_MERGE'] = str(args.bf16_wgrad_merge)
  if args.chain_rows:
    os.environ['NRF_CHAIN_TILE_ROWS'] = str(args.chain_rows)   # read by models.NerfModel when it creates its handle
  if args.gpus > 1 and 'WORLD_SIZE' not in os.environ:
    # `python bench.py --gpus N` as the driver types it: become the launcher of N ranks (one per GPU) and return their exit code
    raise SystemExit(self_launch(args, argv))
  world = int(os.environ.get('WORLD_SIZE', '1'))
  rank = int(os.environ.get('RANK', '0'))
  local_rank = int(os.environ.get('LOCAL_RANK', '0'))
  if world != max(args.gpus, 1):
    raise SystemExit(f'--gpus {args.gpus} but the launcher started WORLD_SIZE={world} ranks')
  # Hooks for exercising the N>1 code path on a ONE-GPU box (set by launch_plan when ranks outnumber devices, never by the
  # driver): BENCH_DIST_BACKEND=gloo swaps RCCL for gloo, BENCH_SAME_DEVICE=1 places the ranks round-robin on the visible
  # devices (RCCL refuses two ranks on one device), BENCH_FORCE_DIST=1 creates the RCCL communicator even with ONE rank, so
  # that the step's fused [grad | stats] all-reduce really goes through librccl on the one GPU a box has.
  backend = os.environ.get('BENCH_DIST_BACKEND', 'nccl')
  force_dist = bool(os.environ.get('BENCH_FORCE_DIST')) and world == 1
  if os.environ.get('BENCH_SAME_DEVICE'):
    local_rank = local_rank % max(torch.cuda.device_count(), 1)
  if world > 1 or force_dist:
    os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
    os.environ.setdefault('MASTER_PORT', '29531')
    torch.cuda.set_device(local_rank)
    kw = {'rank': rank, 'world_size': world} if force_dist else {}
    import datetime
    kw['timeout'] = datetime.timedelta(minutes=5)   # a rank that falls out of a collective fails the run in minutes, not in the default 10+
    # pre-flight of the first real N-GPU run: RCCL must be the transport whenever every rank has its own device, and the line
    # records what the communicator came up with
    if torch.cuda.device_count() >= world and not os.environ.get('BENCH_SAME_DEVICE') and backend != 'nccl':
      raise SystemExit(f'{torch.cuda.device_count()} devices for {world} ranks but BENCH_DIST_BACKEND={backend}: the scaling run must '
                       'use nccl (RCCL)')
    rccl_log = rccl_preflight_begin(rank) if backend == 'nccl' and args.full else None
    if backend == 'nccl':
      dist.init_process_group('nccl', device_id=torch.device('cuda', local_rank), **kw)
    else:
      dist.init_process_group(backend, **kw)
  else:
    rccl_log = None
  dev = torch.device('cuda', local_rank if world > 1 else 0)
  torch.cuda.set_device(dev)
  dist_on = world > 1 or force_dist
  ctx = {'world': world, 'rank': rank, 'local_rank': local_rank, 'dev': dev, 'dist_on': dist_on}

  bf16 = args.bf16 or bool(os.environ.get('BENCH_BF16'))
  if bf16 and args.warp_f32:
    bf16 = 'mlp'
  if args.split_bf16:
    if args.mode != 'eval' or args.bf16 or os.environ.get('BENCH_BF16'):
      raise SystemExit('--split-bf16 is an inference mode (--mode eval) of its own, not combined with --bf16')
    bf16 = 'x3mlp' if args.warp_f32 else 'x3'   # --warp-f32: the SE3 trunk stays on the float32 kernels
  if args.mode == 'eval':
    eval_mode(args, world, rank, dev, bf16, dump=args.dump_outputs)
    if dist_on:
      dist.destroy_process_group()
    return

  M = TRAIN_MODES[args.mode]
  bf16 = bf16 or bool(M.get('force_bf16'))
  BF16_NOTE = BF16_NOTE_MLP if bf16 == 'mlp' else BF16_NOTE_ALL
  cfg = M['cfg']
  rays_per_gpu = args.rays_per_gpu or M['rays']
  r = train_workload(args, M, cfg, rays_per_gpu, bf16, args.graph, ctx, dump=args.dump_outputs)

  # ---- N>1: the north star's other curve in the same run.  "1024-ray batches at 1, 2, 4, 8": the GLOBAL batch stays 1024
  #      rays, every GPU gets 1024/N of them (training.py:266 pmean over the same global batch) -- eager, and with the whole
  #      step replayed from one hipGraph (what a ~1 ms step needs) ----
  strong = None
  if world > 1 and args.full and not args.no_strong and not args.rays_per_gpu and RAYS_PER_GPU % world == 0:
    per = RAYS_PER_GPU // world
    strong = {'global_batch': RAYS_PER_GPU, 'rays_per_gpu': per, 'scaling': 'strong', 'unit': 'rays/s'}
    sargs = argparse.Namespace(**dict(vars(args), burn_in_s=min(args.burn_in_s, 1.0)))
    # BENCH_STRONG_GRAPH=0 leaves the hipGraph variant out (the RCCL all-reduce inside a captured graph has only ever run on a
    # one-rank communicator: tests/test_gpu_rccl.py); a variant that raises is reported as its error text, the line still prints
    variants = (('eager', False),) + ((('graph', True),) if os.environ.get('BENCH_STRONG_GRAPH', '1') != '0' else ())
    for name, g in variants:
      try:
        s = train_workload(sargs, M, cfg, per, bf16, g, ctx, profile=False)
        strong[name] = {'value': s['value'], 'ms_per_step': s['ms_per_step'], 'replica_param_checksums_agree': s['replicas_agree'],
                        'allreduce_exposed_us': s['allreduce_exposed_us'], 'final_loss_fine': s['loss']}
      except Exception as e:   # noqa: BLE001  (SystemExit of a replica mismatch is NOT caught: that must fail the run)
        strong[name] = {'error': f'{type(e).__name__}: {e}'[:300]}

  if rank == 0:
    prof, prof_steps, elapsed, clocks = r['prof'], r['prof_steps'], r['elapsed'], r['clocks']
    ms_per_step = r['ms_per_step']
    mixed = bf16 == 'mlp' and getattr(cfg, 'use_warp', False)   # bf16 NeRF MLPs next to a float32 SE3 trunk
    profiled = {}
    if prof is not None:
      step_flops = sum(e['flops_per_launch'] * e['launches'] for e in prof) / prof_steps
      mode_key = args.mode + ('_bf16' if bf16 and not M.get('force_bf16') else '')
      roofline, peak_tf = roofline_of(prof, bf16, mode_key, rays_per_gpu, cfg)
      at_clock(roofline, clocks)
      kernels = kernel_table(prof, prof_steps)
      ksum_ms = sum(v['ms'] * v['launches_per_step'] for v in kernels.values())
      # the step's flops are priced against the bf16 peak only when every MFMA kernel of it runs in bf16 (warp off)
      step_peak = PEAK_BF16_MFMA_TFLOPS if (bf16 and not mixed) else PEAK_FP32_MFMA_TFLOPS
      profiled = {
          'roofline': roofline,
          'step_tflops': step_flops / (ms_per_step * 1e-3) / 1e12,
          ('step_frac_of_bf16_mfma_peak' if step_peak == PEAK_BF16_MFMA_TFLOPS else 'step_frac_of_fp32_mfma_peak'):
              None if mixed else step_flops / (ms_per_step * 1e-3) / 1e12 / step_peak,
          'kernels': kernels, 'sum_of_kernels_ms': ksum_ms, 'step_over_sum_of_kernels': ms_per_step / ksum_ms if ksum_ms else None}
    checked = {}
    if args.full:
      checked = {'per_rank_final_loss_fine': r['per_rank_loss'], 'replica_param_checksums_agree': r['replicas_agree']}
    over = os.environ.get('BENCH_OVERSUBSCRIBED')
    out = {
        'metric': M['metric'], 'value': r['value'], 'unit': 'rays/s', 'n_gpus': world,
        'steps': args.steps, 'warmup': args.warmup, 'ms_per_step': ms_per_step, 'higher_is_better': True,
        'scaling': 'weak', 'vs_baseline': None,
        'dtype': ('bf16 NeRF MLPs + f32 warp field' if mixed else 'bf16') if bf16 else 'f32', 'data': 'synthetic',
        'config': {'workload': M['workload'].format(rays=rays_per_gpu) + (BF16_NOTE if bf16 else '') +
                               (' [whole step replayed from one hipGraph]' if args.graph else ''),
                   'rays_per_gpu': rays_per_gpu, 'global_batch': world * rays_per_gpu, 'parallelism': f'ray-shard dp{world}',
                   'metadata_frames': NUM_FRAMES if M['reg'] else None, 'learning_rate': BENCH_LR},
        **profiled,
        'final_loss_fine': r['loss'], **checked,
        'steady_state': {'burn_in_steps': r['burn_steps'], 'burn_in_s': args.burn_in_s, 'timed_window_s': elapsed,
                         'during_timed_window': clocks},
        'graph_replay': bool(args.graph),
        'rccl_ranks': dist.get_world_size() if dist_on else 1, 'dist_backend': backend if dist_on else None,
        'rccl_version': rccl_version() if dist_on and backend == 'nccl' and args.full else None,
        'rccl_preflight': rccl_preflight_summary(rccl_log) if dist_on and backend == 'nccl' and args.full else None,
        'grad_allreduce_us': r['allreduce_us'], 'grad_allreduce_bytes': r['allreduce_bytes'],
        'grad_allreduce_exposed_us': r['allreduce_exposed_us'],
        'grad_allreduce_exposed_frac': (r['allreduce_exposed_us'] / (1e3 * ms_per_step)) if r['allreduce_exposed_us'] is not None else None,
        'strong_scaling': strong,
        'oversubscribed': over,
        'chain_tile_rows': args.chain_rows or 'auto', 'bf16_wgrad_merge': 'default (1)' if args.bf16_wgrad_merge is None else args.bf16_wgrad_merge,
        'csrc_sha16': kernel_source_sha(), 'full': bool(args.full), 'dumped_outputs': r['dumped'],
    }
    if over:
      out['config']['workload'] += f' [OVERSUBSCRIBED: {over}, transport {backend} -- code-path check, not a scaling measurement]'
    default_line = (args.full and world == 1 and args.mode == 'train' and not force_dist and not args.graph and not args.rays_per_gpu and
                    not bf16 and not args.no_extras)
    if default_line:
      # ---- what makes the ONE driver-run line certify more than the headline's 0.14 s window (all outside the timed region):
      #      (c) a sustained run of the same workload, (a) config-E parity against the oracle, (b) the other BASELINE configs ----
      try:
        sargs = argparse.Namespace(**dict(vars(args), burn_in_s=0.0, warmup=2, steps=max(20, int(1.05 * args.sustained_s / (ms_per_step * 1e-3)) + 2)))   # + 5 %: the sustained steps may run faster than the headline's
        sr = train_workload(sargs, M, cfg, rays_per_gpu, bf16, False, ctx, profile=False)
        out['sustained'] = {'seconds': sr['elapsed'], 'steps': sargs.steps, 'value': sr['value'], 'unit': 'rays/s',
                            'ms_per_step': sr['ms_per_step'], 'vs_headline': sr['value'] / r['value'], 'clocks': sr['clocks']}
      except Exception as e:   # noqa: BLE001
        out['sustained'] = {'error': f'{type(e).__name__}: {e}'[:300]}
      torch.cuda.empty_cache()
      try:
        out['eval_parity'] = eval_parity(dev)
      except Exception as e:   # noqa: BLE001
        out['eval_parity'] = {'error': f'{type(e).__name__}: {e}'[:300]}
      out['secondary'] = secondary_lines(args, ctx)
      # the driver's record keeps `config`, `roofline` and `cpu_baseline` whole and only the NAMES of other keys: a compact copy
      # of the three certificates rides in `config` (it still names the workload; the full objects are top-level keys)
      ep, sec, sus = out['eval_parity'], out['secondary'], out['sustained']
      out['config']['certified_in_this_run'] = {
          'eval_parity': dict({k: ep.get(k) for k in ('rays', 'max_abs_rgb', 'max_abs_depth', 'psnr_vs_oracle_db', 'pass', 'error') if k in ep},
                              **({'bf16x3': {k: ep['bf16x3'].get(k) for k in ('max_abs_rgb', 'max_abs_depth', 'psnr_vs_oracle_db', 'max_abs_rgb_vs_f32_path', 'pass')}}
                                 if isinstance(ep.get('bf16x3'), dict) else {})),
          'secondary': [{k: (x.get('roofline') or {}).get('frac') if k == 'roofline_frac' else x.get(k)
                         for k in ('mode', 'dtype', 'value', 'ms_per_step', 'roofline_frac', 'error') if k == 'roofline_frac' or k in x}
                        for x in sec],
          'sustained': {k: sus.get(k) for k in ('seconds', 'value', 'error') if k in sus}}
    if args.full and world == 1 and args.mode == 'train' and not args.no_cpu_baseline and not force_dist:
      out['cpu_baseline'] = cpu_baseline()
    # the per-kernel table is the longest object of the line: it goes LAST but for the certificates, which a tail-only reader
    # of the line (the driver keeps the last ~2 KB of stdout) must still see
    for k in ('kernels', 'eval_parity', 'secondary', 'sustained'):
      if k in out:
        out[k] = out.pop(k)
    print(json.dumps(out), flush=True)
  if dist_on:
    dist.barrier()
    dist.destroy_process_group()


if __name__ == '__main__':
  main()
