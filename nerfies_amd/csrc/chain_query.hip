// Kernels of a field query (nrf_query_points / nrf_query_grid, include/nerfies_amd.h): the NeRF field at arbitrary points.
//   density chain (64-row tiles): the density-only query -- a 512^3 grid is 1.3e8 rows, none of which needs a colour.
//       The tile runs the chain's prologue, the eight trunk layers and the alpha head and stores ONE float per row: no
//       bottleneck, rgb branch, logits, sigmoid or condition term.  A use_alpha_condition model keeps the bottleneck layer (its
//       alpha head reads it) and the per-group code term, and drops the rgb branch alone.
//   field_ids / field_unpack / grid_points: the per-point code rows of the SE3 forward, out4 -> (sigma, rgb), a grid's points.
// density_tile is nerf_chain.h fwd_tile up to the alpha head, spelled from the same pieces (G::k_loop, fwd_epilogue, the head's
// four partial sums in one order): every rounding a row's sigma goes through is that of the full chain, so the two queries give
// the same bits.  It is a function of its own in a translation unit of its own: fwd_tile and every kernel instantiated from it
// are compiled from unchanged text (profiles/field_query.md has the resource table before / after).  64-row tiles only: the 32-row
// K loop sits at its 128-register bound with 28 bytes of scratch in every kernel built on it, and no new kernel may spill; both
// tilings give a row the same bits, so a small density-only query loses nothing but occupancy.
#include "nerf_chain.h"

namespace nrf {

struct DensityArgs1 { ChainFwdArgs a[1]; float* sigma; };   // a[]: read through a run-time index (nerf_chain.h ChainFwdArgs1)

template <class G>
__device__ __forceinline__ void density_tile(const ChainFwdArgs& A, float* __restrict__ sigma, const int tile, const int T, float* smem,
                                             const int tid0, const int wave) {
  constexpr int ROWS = G::ROWS;
  float* act = smem;                  // [256][ROWS] swizzled
  float* pe = smem + TRUNK_W * ROWS;  // [max(PK, G::SCRATCH_ROWS)][ROWS]; reused as scratch after the skip layer
  const float* __restrict__ prm = A.params;
  const int PK = A.PK;
  const int nq_pe = PK / 16;
  int tid = tid0;
  asm volatile("" : "+v"(tid));   // per-tile lane constants (nerf_chain.h fwd_tile)
  const int lane = tid & 63;
  const int h = lane >> 5;
  const int p = G::prow(lane);
  const int part = G::part(wave, h);
  const int row0 = G::row0(tile, T);
  // ---- prologue: the point + SinusoidalEncoder (modules.py:213-228) ----
  {
    int r = row0 + p;
    r = r < A.rows ? r : A.rows - 1;
    const float x[3] = {A.points[3 * r], A.points[3 * r + 1], A.points[3 * r + 2]};
    auto put = [&](int k, float v) { pe[k * ROWS + p] = v; };
    if (part == 0) {
#pragma unroll
      for (int c = 0; c < 3; ++c) put(c, x[c]);
    } else if (part == 1) {
      for (int k = A.P; k < PK; ++k) put(k, 0.f);
    }
    const float half_pi = 1.57079632679489661923f;   // fp32(pi/2), modules.py:222
    for (int f = part; f < A.F; f += G::PARTS) {
      const float fr = (float)(1 << f);
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float a = __fmul_rn(x[c], fr);
        put(3 + (2 * f) * 3 + c, sinf(a));
        put(3 + (2 * f + 1) * 3 + c, sinf(__fadd_rn(a, half_pi)));
      }
    }
  }
  __syncthreads();

  f32x16 acc[G::RB][2];
  const float4* wpk4 = reinterpret_cast<const float4*>(A.wpk);
  const __amdgpu_buffer_rsrc_t no_stash = make_rsrc(nullptr, FRAG_TILE_256 * 4);
  // ---- trunk: 8 x Dense(256)+ReLU, skip concat [h, posenc] at layer A.skip (modules.py:41-50) ----
  const float4* wL0 = wpk4 + (A.pk.fwd_L[0] / 4) + wave * (PK / 4) * 64;
  WQuad<2> wnext = prefetch_quad<2>(wL0, lane);
  BiasRegs<2> bnext = bias_load<2>(prm + A.po.trunk_b[0], wave * 64, lane);
#pragma unroll 1
  for (int l = 0; l < TRUNK_DEPTH; ++l) {
    bias_set<2>(acc, bnext);
    if (l == 0) {
      G::template k_loop<2, false>(acc, pe, nq_pe, wL0, lane, wnext);
    } else {
      G::template k_loop<2, true>(acc, act, 16, wpk4 + (A.pk.fwd_L[l] / 4) + wave * 64 * 64, lane, wnext);
      if (l == A.skip) {
        const float4* w4b = wpk4 + (A.pk.fwd_L4b / 4) + wave * (PK / 4) * 64;
        G::template k_loop<2, false>(acc, pe, nq_pe, w4b, lane, prefetch_quad<2>(w4b, lane));
      }
    }
    // behind the last layer: the bottleneck's first weights and bias (read by a use_alpha_condition model only; the image is
    // there for every model)
    wnext = prefetch_quad<2>(wpk4 + ((l + 1 < TRUNK_DEPTH ? A.pk.fwd_L[l + 1] : A.pk.fwd_bn) / 4) + wave * 64 * 64, lane);
    bnext = bias_load<2>(prm + (l + 1 < TRUNK_DEPTH ? A.po.trunk_b[l + 1] : A.po.bn_b), wave * 64, lane);
    __builtin_amdgcn_sched_barrier(0);
    fwd_epilogue<2, EPI_RELU, STASH_NONE, G>(acc, wave * 64, act, no_stash, 0, nullptr, lane, T);
  }
  // ---- use_alpha_condition: the head reads the bottleneck, Dense(256), no activation (modules.py:149-157) ----
  if (A.alpha_ct) {
    bias_set<2>(acc, bnext);
    G::template k_loop<2, true>(acc, act, 16, wpk4 + (A.pk.fwd_bn / 4) + wave * 64 * 64, lane, wnext);
    __builtin_amdgcn_sched_barrier(0);
    fwd_epilogue<2, EPI_LINEAR, STASH_NONE, G>(acc, wave * 64, act, no_stash, 0, nullptr, lane, T);
  }
  // ---- alpha head: four partial sums (wave w: the fmaf chain over k = 64 w .. 64 w + 63), combined in one order ----
  {
    const float4* __restrict__ wa4 = reinterpret_cast<const float4*>(prm + A.po.alpha_k) + wave * 16;
    float s = 0.f;
    const int k0 = wave * 64;
#pragma unroll 1
    for (int kc = 0; kc < 4; ++kc) {
      float4 w4[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) w4[i] = wa4[4 * kc + i];
      float a[16];
#pragma unroll
      for (int i = 0; i < 16; ++i) a[i] = act[G::elem(k0 + 16 * kc + i, p)];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        s = fmaf(a[4 * i], w4[i].x, s); s = fmaf(a[4 * i + 1], w4[i].y, s);
        s = fmaf(a[4 * i + 2], w4[i].z, s); s = fmaf(a[4 * i + 3], w4[i].w, s);
      }
    }
    if (G::part_writer(h)) pe[wave * ROWS + p] = s;   // scratch (the posenc is no longer needed for this tile)
    __syncthreads();
    if (part == 0) {
      float sigma_raw = (pe[p] + pe[ROWS + p]) + (pe[2 * ROWS + p] + pe[3 * ROWS + p]) + prm[A.po.alpha_b];
      if (A.alpha_ct) sigma_raw += A.alpha_ct[min((row0 + p) / A.S, A.B - 1)];
      if (row0 + p < A.rows) sigma[(size_t)row0 + p] = sigma_activation(sigma_raw, A.sigma_act);
    }
    __syncthreads();   // scratch (aliases pe) is free again for the next tile's prologue
  }
}

__global__ __launch_bounds__(256, Tile64::WG_PER_CU) void nerf_density_kernel(const DensityArgs1 P) {
  const ChainFwdArgs& A = P.a[blockIdx.x >> 24];
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int tid0 = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid0 >> 6);
  int* tslot = reinterpret_cast<int*>(smem + ACT_FLOATS);   // posenc / scratch rows: free between tiles
  const TileIter ti = tile_iter(A.ntiles, A.k_old);
  for (int tile = A.tile_counter ? next_tile(A.tile_counter, tslot) : ti.first; tile < (A.tile_counter ? A.ntiles : ti.end);
       tile = A.tile_counter ? next_tile(A.tile_counter, tslot, tile) : tile + ti.step)
    density_tile<Tile64>(A, P.sigma, tile, 0, smem, tid0, wave);
}

void launch_chain_density(const ChainFwdArgs& a, float* sigma, int grid, hipStream_t stream) {
  DensityArgs1 p;
  p.a[0] = a; p.sigma = sigma;
  const size_t lds = chain_fwd_lds_bytes<Tile64>(a.PK);
  (void)hipFuncSetAttribute((const void*)nerf_density_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL(nerf_density_kernel, dim3(grid), dim3(256), lds, stream, p);
}

__global__ void field_ids_kernel(const int32_t* __restrict__ group_ids, int rows, int S, int32_t* __restrict__ ids) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= rows) return;
  const int g = r / S;
  ids[r] = group_ids ? group_ids[g] : g;
}

void launch_field_ids(const int32_t* group_ids, int rows, int S, int32_t* ids, hipStream_t stream) {
  hipLaunchKernelGGL(field_ids_kernel, dim3((rows + 255) / 256), dim3(256), 0, stream, group_ids, rows, S, ids);
}

__global__ void field_unpack_kernel(const float4* __restrict__ out4, int rows, float* __restrict__ sigma, float* __restrict__ rgb) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= rows) return;
  const float4 o = out4[r];
  if (sigma) sigma[r] = o.w;
  if (rgb) { rgb[3 * (size_t)r] = o.x; rgb[3 * (size_t)r + 1] = o.y; rgb[3 * (size_t)r + 2] = o.z; }
}

void launch_field_unpack(const float4* out4, int rows, float* sigma, float* rgb, hipStream_t stream) {
  hipLaunchKernelGGL(field_unpack_kernel, dim3((rows + 255) / 256), dim3(256), 0, stream, out4, rows, sigma, rgb);
}

__global__ void grid_points_kernel(const nrf_grid g, long long first, int count, float* __restrict__ out) {
  // product, then sum: two float32 roundings, as the header states them.  hipcc defines __fmul_rn / __fadd_rn as the plain operators
  // and would contract the pair into one fused multiply-add
#pragma clang fp contract(off)
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= count) return;
  const long long n = first + t;
  const long long nx = g.dims[0], nxy = nx * g.dims[1];
  const int idx[3] = {(int)(n % nx), (int)((n / nx) % g.dims[1]), (int)(n / nxy)};
#pragma unroll
  for (int c = 0; c < 3; ++c) {   // plain operators: the pragma above governs them, not the bodies of __fmul_rn / __fadd_rn
    const float prod = (float)idx[c] * g.step[c];
    out[3 * (size_t)t + c] = g.origin[c] + prod;
  }
}

void launch_grid_points(const nrf_grid& g, long long first, int count, float* out, hipStream_t stream) {
  hipLaunchKernelGGL(grid_points_kernel, dim3((count + 255) / 256), dim3(256), 0, stream, g, first, count, out);
}

}  // namespace nrf
