// The float32 NeRF-MLP chain kernels of a frozen-field plan (NRF_FLAG_FROZEN, include/nerfies_amd.h): the field's parameters are
// constants of the call and the reverse pass stops at the rays, so nothing the weight gradient reads is written.
//   forward  (64- and 32-row tiles): the posenc stash and the ReLU sign words, no activation stash (nerf_chain.h fwd_tile<., STASH_BITS>);
//   reverse  (64-row tiles):         d_points and dray, no dY image, no bias column sums -- none of the 23 cross-tile accumulators
//                                    of BwdAcc, nothing to flush, small_part untouched (nerf_chain.h bwd_tile<., ., false>).
// The tile bodies are those of mlp_chain.hip / mlp_chain32.hip (nerf_chain.h), instantiated on compile-time modes, as are the density
// kernels of chain_query.hip / chain_query_grad.hip (fwd_tile's DENSITY, bwd_tile's DENS); the kernels of one kind of plan share a
// translation unit.
#include "nerf_chain.h"

namespace nrf {

__global__ __launch_bounds__(256, Tile64::WG_PER_CU) void nerf_mlp_fwd_bits_kernel(const ChainFwdArgs1 P) {
  const ChainFwdArgs& A = P.a[blockIdx.x >> 24];
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int tid0 = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid0 >> 6);
  auto no_stamp = []() {};
  int* tslot = reinterpret_cast<int*>(smem + ACT_FLOATS);   // posenc / scratch rows: free between tiles
  const TileIter ti = tile_iter(A.ntiles, A.k_old);
  for (int tile = A.tile_counter ? next_tile(A.tile_counter, tslot) : ti.first; tile < (A.tile_counter ? A.ntiles : ti.end);
       tile = A.tile_counter ? next_tile(A.tile_counter, tslot, tile) : tile + ti.step)
    fwd_tile<Tile64, STASH_BITS>(A, tile, 0, smem, tid0, wave, no_stamp);
}

__global__ __launch_bounds__(256, Tile32::WG_PER_CU) void nerf_mlp_fwd32_bits_kernel(const ChainFwdArgs1 P) {
  const ChainFwdArgs& A = P.a[blockIdx.x >> 24];
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int tid0 = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid0 >> 6);
  const int nhalf = 2 * A.ntiles;
  auto no_stamp = []() {};
#pragma unroll 1
  for (int ht = blockIdx.x; ht < nhalf; ht += gridDim.x) fwd_tile<Tile32, STASH_BITS>(A, ht >> 1, ht & 1, smem, tid0, wave, no_stamp);
}

void launch_chain_fwd_frozen(const ChainFwdArgs& a, bool tile32, int grid, hipStream_t stream) {
  ChainFwdArgs1 p;
  p.a[0] = a;
  if (tile32) {
    const size_t lds = chain_fwd_lds_bytes<Tile32>(a.PK);
    (void)hipFuncSetAttribute((const void*)nerf_mlp_fwd32_bits_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(nerf_mlp_fwd32_bits_kernel, dim3(grid), dim3(256), lds, stream, p);
  } else {
    const size_t lds = chain_fwd_lds_bytes<Tile64>(a.PK);
    (void)hipFuncSetAttribute((const void*)nerf_mlp_fwd_bits_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(nerf_mlp_fwd_bits_kernel, dim3(grid), dim3(256), lds, stream, p);
  }
}

// Both levels in one launch, tiles dealt round-robin (nerf_chain.h ChainBwdArgs2), as nerf_mlp_bwd_kernel without its flushes.
__global__ __launch_bounds__(256, Tile64::WG_PER_CU) void nerf_mlp_bwd_rays_kernel(const ChainBwdArgs2 P) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int nt0 = P.nt0, ntot = P.ntot;
  NoBwdAcc C;
#pragma unroll 1
  for (int g = blockIdx.x; g < ntot; g += gridDim.x) {
    const int lv = g >= nt0 ? 1 : 0;
    bwd_tile<Tile64, NoBwdAcc, false>(P.a[lv], g - (lv ? nt0 : 0), 0, smem, C);
  }
}

void launch_chain_bwd_frozen(const ChainBwdArgs& a0, const ChainBwdArgs* a1, int grid, hipStream_t stream) {
  const size_t lds = chain_lds_bytes<Tile64>(a0.d_points ? a0.PK : 4);
  (void)hipFuncSetAttribute((const void*)nerf_mlp_bwd_rays_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  ChainBwdArgs2 p;
  p.a[0] = a0; p.a[1] = a1 ? *a1 : a0;
  p.nt0 = a0.ntiles; p.ntot = p.nt0 + (a1 ? a1->ntiles : 0);
  hipLaunchKernelGGL(nerf_mlp_bwd_rays_kernel, dim3(grid), dim3(256), lds, stream, p);
}

}  // namespace nrf
