// The fused NeRF-MLP chain on 32-ROW tiles, FOUR workgroups per CU (round 5): the kernels that instantiate the shared tile bodies
// of nerf_chain.h (fwd_tile / bwd_tile) on the Tile32 geometry defined there.  Same math, same packed weights, same HBM images
// as the 64-row kernels of mlp_chain.hip, so the two tilings can be mixed launch by launch (forward 32 / reverse 64 and so on);
// nerf_chain.h says why the second tiling exists and how its rows map onto the 64-row images.
#include <stdio.h>
#include <stdlib.h>

#include "nerf_chain.h"

namespace nrf {

template <bool STASH>
__global__ __launch_bounds__(256, Tile32::WG_PER_CU) void nerf_mlp_fwd32_kernel(const ChainFwdArgs1 P) {
  const ChainFwdArgs& A = P.a[blockIdx.x >> 24];
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int tid0 = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid0 >> 6);
  const int nhalf = 2 * A.ntiles;
  auto no_stamp = []() {};
#pragma unroll 1
  for (int ht = blockIdx.x; ht < nhalf; ht += gridDim.x) fwd_tile<Tile32, STASH>(A, ht >> 1, ht & 1, smem, tid0, wave, no_stamp);
}

void launch_chain_fwd32(const ChainFwdArgs& a, bool stash, int grid, hipStream_t stream) {
  const size_t lds = chain_fwd_lds_bytes<Tile32>(a.PK);
  ChainFwdArgs1 p;
  p.a[0] = a;
  if (stash) {
    (void)hipFuncSetAttribute((const void*)nerf_mlp_fwd32_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(nerf_mlp_fwd32_kernel<true>, dim3(grid), dim3(256), lds, stream, p);
  } else {
    (void)hipFuncSetAttribute((const void*)nerf_mlp_fwd32_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(nerf_mlp_fwd32_kernel<false>, dim3(grid), dim3(256), lds, stream, p);
  }
}

// Both levels in one launch, as nerf_mlp_bwd_kernel: global half tiles [0, nt0) are level 0, [nt0, ntot) level 1, dealt
// round-robin.  Nothing to flush: every half tile adds its bias partials to small_part itself (nerf_chain.h bias32_add).
__global__ __launch_bounds__(256, Tile32::WG_PER_CU) void nerf_mlp_bwd32_kernel(const ChainBwdArgs2 P) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int nt0 = P.nt0, ntot = P.ntot;
  NoBwdAcc C;
#pragma unroll 1
  for (int g = blockIdx.x; g < ntot; g += gridDim.x) {
    const int lv = g >= nt0 ? 1 : 0;
    const int ht = g - (lv ? nt0 : 0);
    bwd_tile<Tile32>(P.a[lv], ht >> 1, ht & 1, smem, C);
  }
}

void launch_chain_bwd32(const ChainBwdArgs& a0, const ChainBwdArgs* a1, int grid, hipStream_t stream) {
  const size_t lds = chain_lds_bytes<Tile32>(4);
  (void)hipFuncSetAttribute((const void*)nerf_mlp_bwd32_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  ChainBwdArgs2 p;
  p.a[0] = a0; p.a[1] = a1 ? *a1 : a0;
  p.nt0 = 2 * a0.ntiles; p.ntot = p.nt0 + (a1 ? 2 * a1->ntiles : 0);
  hipLaunchKernelGGL(nerf_mlp_bwd32_kernel, dim3(grid), dim3(256), lds, stream, p);
}

}  // namespace nrf
