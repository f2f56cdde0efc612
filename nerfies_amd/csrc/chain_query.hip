// Kernels of a field query (nrf_query_points / nrf_query_grid, include/nerfies_amd.h): the NeRF field at arbitrary points.
//   density chain (64-row tiles): the density-only query -- a 512^3 grid is 1.3e8 rows, none of which needs a colour.
//       The tile runs the chain's prologue, the eight trunk layers and the alpha head and stores ONE float per row: no
//       bottleneck, rgb branch, logits, sigmoid or condition term.  A use_alpha_condition model keeps the bottleneck layer (its
//       alpha head reads it) and the per-group code term, and drops the rgb branch alone.
//   field_ids / field_unpack / grid_points: the per-point code rows of the SE3 forward, out4 -> (sigma, rgb), a grid's points.
// The density tile is nerf_chain.h fwd_tile in its density mode (fwd_tile<Tile64, STASH_NONE, true>): the chain's own text up to the
// alpha head, so every rounding a row's sigma goes through is that of the full chain and the two queries give the same bits.  The
// mode is compile time and off by default: every other kernel instantiated from fwd_tile compiles to the assembly it had before the
// mode existed (profiles/field_query.md has the comparison and the resource table).  64-row tiles only: the 32-row K loop sits at its
// 128-register bound with 28 bytes of scratch in every kernel built on it, and no density kernel may spill; both tilings give a row
// the same bits, so a small density-only query loses nothing but occupancy.
#include "nerf_chain.h"

namespace nrf {

struct DensityArgs1 { ChainFwdArgs a[1]; float* sigma; };   // a[]: read through a run-time index (nerf_chain.h ChainFwdArgs1)

__global__ __launch_bounds__(256, Tile64::WG_PER_CU) void nerf_density_kernel(const DensityArgs1 P) {
  const ChainFwdArgs& A = P.a[blockIdx.x >> 24];
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int tid0 = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid0 >> 6);
  auto no_stamp = []() {};
  int* tslot = reinterpret_cast<int*>(smem + ACT_FLOATS);   // posenc / scratch rows: free between tiles
  const TileIter ti = tile_iter(A.ntiles, A.k_old);
  for (int tile = A.tile_counter ? next_tile(A.tile_counter, tslot) : ti.first; tile < (A.tile_counter ? A.ntiles : ti.end);
       tile = A.tile_counter ? next_tile(A.tile_counter, tslot, tile) : tile + ti.step)
    fwd_tile<Tile64, STASH_NONE, true>(A, tile, 0, smem, tid0, wave, no_stamp, P.sigma);
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
