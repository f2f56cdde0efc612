// Kernels of a gradient query (nrf_query_points_grad / nrf_query_grid_grad, include/nerfies_amd.h): the density, its gradient with
// respect to the caller's point and the surface normal -grad / |grad|.
//   forward  (64-row tiles): the density tile of chain_query.hip keeping what the reverse needs -- nerf_chain.h
//       fwd_tile<Tile64, STASH_BITS, true>: the posenc stash, the trunk's ReLU sign words (256 + 4 PKS bytes per row) and sigma'(raw),
//       one float per row.  The same function as the density-only query's tile: the same sigma bits.
//   reverse  (64-row tiles): nerf_chain.h bwd_tile started at the density, bwd_tile<Tile64, NoBwdAcc, false, true>.  ds = sigma'(raw)
//       enters at the alpha head -- dpre_7 = mask_7(ds (x) w_alpha) needs no GEMM; a use_alpha_condition model: d bn = ds (x)
//       w_alpha[0:256], then the W_bn^T step -- and runs down the trunk with bwd_tile's own d-posenc section and chain rule.  No rgb
//       logit^T, rgb branch, per-ray sums, dY image or bias sum: nothing is accumulated across rows, so there is no atomic and a
//       row's gradient does not depend on the launch it ran in.
//   finish   (one thread per row): grad = J^T grad' through the warp Jacobian of the row (the existing primal + tangent + Jacobian
//       kernels of warp_chain.hip, launched as they are), and the normal.
// Both modes are compile time and off by default: every other chain kernel compiles to the assembly it had before they existed
// (profiles/field_gradient.md has the comparison and the resource table).  64-row tiles only, for the reason chain_query.hip gives.
#include "nerf_chain.h"

namespace nrf {

struct DensityGradFwdArgs1 { ChainFwdArgs a[1]; float* sigma; float* dsig; };   // a[]: read through a run-time index (nerf_chain.h ChainFwdArgs1)
struct DensityGradBwdArgs1 { ChainBwdArgs a[1]; const float* dsig; };

__global__ __launch_bounds__(256, Tile64::WG_PER_CU) void nerf_density_stash_kernel(const DensityGradFwdArgs1 P) {
  const ChainFwdArgs& A = P.a[blockIdx.x >> 24];
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int tid0 = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid0 >> 6);
  auto no_stamp = []() {};
  int* tslot = reinterpret_cast<int*>(smem + ACT_FLOATS);   // posenc / scratch rows: free between tiles
  const TileIter ti = tile_iter(A.ntiles, A.k_old);
  for (int tile = A.tile_counter ? next_tile(A.tile_counter, tslot) : ti.first; tile < (A.tile_counter ? A.ntiles : ti.end);
       tile = A.tile_counter ? next_tile(A.tile_counter, tslot, tile) : tile + ti.step)
    fwd_tile<Tile64, STASH_BITS, true>(A, tile, 0, smem, tid0, wave, no_stamp, P.sigma, P.dsig);
}

void launch_chain_density_stash(const ChainFwdArgs& a, float* sigma, float* dsig, int grid, hipStream_t stream) {
  DensityGradFwdArgs1 p;
  p.a[0] = a; p.sigma = sigma; p.dsig = dsig;
  const size_t lds = chain_fwd_lds_bytes<Tile64>(a.PK);
  (void)hipFuncSetAttribute((const void*)nerf_density_stash_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL(nerf_density_stash_kernel, dim3(grid), dim3(256), lds, stream, p);
}

__global__ __launch_bounds__(256, Tile64::WG_PER_CU) void nerf_density_bwd_kernel(const DensityGradBwdArgs1 P) {
  const ChainBwdArgs& A = P.a[blockIdx.x >> 24];
  extern __shared__ __attribute__((aligned(16))) float smem[];
  NoBwdAcc C;
#pragma unroll 1
  for (int tile = blockIdx.x; tile < A.ntiles; tile += gridDim.x) bwd_tile<Tile64, NoBwdAcc, false, true>(A, tile, 0, smem, C, P.dsig);
}

void launch_chain_density_bwd(const ChainBwdArgs& a, const float* dsig, int grid, hipStream_t stream) {
  DensityGradBwdArgs1 p;
  p.a[0] = a; p.dsig = dsig;
  const size_t lds = chain_lds_bytes<Tile64>(a.PK);
  (void)hipFuncSetAttribute((const void*)nerf_density_bwd_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL(nerf_density_bwd_kernel, dim3(grid), dim3(256), lds, stream, p);
}

// grad = J^T grad' (jac: the warp Jacobian d x'_i / d x_j, row-major [rows][9]; nullptr: the identity) and the normal
//   s = fmaf(g.z, g.z, fmaf(g.y, g.y, g.x * g.x));  n = -(g * (1 / sqrtf(s)))  -- exactly 0 where s is 0 or not finite
// (include/nerfies_amd.h nrf_field_grad_out).  Either output may be nullptr.
__global__ void field_grad_finish_kernel(const float* __restrict__ d_points, const float* __restrict__ jac, int rows, float* __restrict__ grad,
                                         float* __restrict__ normals) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= rows) return;
  const float* dp = d_points + 3 * (size_t)r;
  float g[3] = {dp[0], dp[1], dp[2]};
  if (jac) {
    const float* J = jac + 9 * (size_t)r;
    const float gp[3] = {g[0], g[1], g[2]};
#pragma unroll
    for (int c = 0; c < 3; ++c) g[c] = fmaf(J[6 + c], gp[2], fmaf(J[3 + c], gp[1], __fmul_rn(J[c], gp[0])));
  }
  if (grad) {
#pragma unroll
    for (int c = 0; c < 3; ++c) grad[3 * (size_t)r + c] = g[c];
  }
  if (normals) {
    const float s = fmaf(g[2], g[2], fmaf(g[1], g[1], __fmul_rn(g[0], g[0])));
    const bool ok = s > 0.f && s < __builtin_inff();
    const float inv = ok ? 1.f / sqrtf(s) : 0.f;
#pragma unroll
    for (int c = 0; c < 3; ++c) normals[3 * (size_t)r + c] = ok ? -__fmul_rn(g[c], inv) : 0.f;
  }
}

void launch_field_grad_finish(const float* d_points, const float* jac, int rows, float* grad, float* normals, hipStream_t stream) {
  hipLaunchKernelGGL(field_grad_finish_kernel, dim3((rows + 255) / 256), dim3(256), 0, stream, d_points, jac, rows, grad, normals);
}

}  // namespace nrf
