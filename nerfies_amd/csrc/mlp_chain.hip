// Fused NeRF-MLP chain for gfx950 on 64-ROW tiles: posenc -> 8x256 trunk (skip at 4) -> alpha head / bottleneck -> rgb branch,
// forward and data-gradient passes.  The tile bodies are nerf_chain.h fwd_tile / bwd_tile, shared with the 32-row kernels of
// mlp_chain32.hip; this file holds the 64-row kernels (tile hand-out, timeline, bias-gradient registers) and the weight packing.
//
// Design (one workgroup = 4 waves = one 64-row tile, persistent over tiles, TWO
// workgroups resident per CU so one's epilogues hide under the other's MFMAs):
//   * activations of the tile live in LDS, feature-major  act[k][64 rows]
//     (XOR-swizzled 16-byte granules so the MFMA epilogue's ds_write_b128 is
//     bank-conflict free; the A-operand ds_read_b64 covers a whole row);
//   * every layer is  acc[64 x 64 per wave] += A(LDS) x B(weights), with
//     v_mfma_f32_32x32x2_f32 (exact fp32 == an fmaf chain).  Rows are
//     interleaved so that MFMA row-block rb holds tile rows p = 2*i + rb: one
//     ds_read_b64 then feeds the A operand of both row blocks;
//   * weights are pre-packed per layer in B-fragment order, so each lane
//     streams its B operands with one coalesced global_load_dwordx4 per 16
//     MFMAs straight from L2 -- no LDS traffic for weights;
//   * the training stash is written straight from the accumulator registers in
//     "fragment-native" order (coalesced 1 KiB per wave store); the dgrad pass
//     and the wgrad GEMM read it back in the same order.
#include <stdio.h>
#include <stdlib.h>

#include "nerf_chain.h"

namespace nrf {

template <bool STASH>
__global__ __launch_bounds__(256, Tile64::WG_PER_CU) void nerf_mlp_fwd_kernel(const ChainFwdArgs1 P) {
  const ChainFwdArgs& A = P.a[blockIdx.x >> 24];
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int tid0 = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid0 >> 6);
  // in-kernel timeline (scripts/timeline_mlp.py): compiled in only with -DNRF_TIMELINE_BUILD -- its counters and clock values
  // are live across the whole kernel, in a kernel that is out of registers
#ifdef NRF_TIMELINE_BUILD
  int stamp_i = 0;
  auto STAMP = [&]() {
    if (A.timeline && blockIdx.x == 0 && (tid0 & 63) == 0 && stamp_i < 64) A.timeline[wave * 64 + stamp_i] = clock64();
    ++stamp_i;
  };
  unsigned long long wg_t0 = 0, wg_w0 = 0;
  if (A.timeline && tid0 == 0) { wg_t0 = clock64(); wg_w0 = wall_clock64(); }
#else
  auto STAMP = [&]() {};
#endif
  int* tslot = reinterpret_cast<int*>(smem + ACT_FLOATS);   // posenc / scratch rows: free between tiles
  const TileIter ti = tile_iter(A.ntiles, A.k_old);
  for (int tile = A.tile_counter ? next_tile(A.tile_counter, tslot) : ti.first; tile < (A.tile_counter ? A.ntiles : ti.end);
       tile = A.tile_counter ? next_tile(A.tile_counter, tslot, tile) : tile + ti.step) {
    STAMP();   // tile start
    fwd_tile<Tile64, STASH>(A, tile, 0, smem, tid0, wave, STAMP);
  }
#ifdef NRF_TIMELINE_BUILD
  if (A.timeline && tid0 == 0) {   // per-workgroup residency record: start, end (shader clock), HW_ID, XCC_ID
    unsigned long long* rec = A.timeline + 1024 + 4 * (size_t)blockIdx.x;
    rec[0] = wg_t0; rec[1] = clock64();
    rec[2] = __builtin_amdgcn_s_getreg((4) | (0 << 6) | (31 << 11));    // HW_REG_HW_ID
    rec[3] = (__builtin_amdgcn_s_getreg((20) | (0 << 6) | (31 << 11)) & 0xf)   // HW_REG_XCC_ID
             | ((wall_clock64() - wg_w0) << 8);                               // residency in 100 MHz ticks
  }
#endif
}

void launch_chain_fwd(const ChainFwdArgs& a, bool stash, int grid, hipStream_t stream) {
  const size_t lds = chain_fwd_lds_bytes<Tile64>(a.PK);
  ChainFwdArgs1 p;
  p.a[0] = a;
  if (knobs().debug_occ) {
    int nb = -1;
    (void)hipFuncSetAttribute((const void*)nerf_mlp_fwd_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, (const void*)nerf_mlp_fwd_kernel<true>, 256, lds);
    hipFuncAttributes fa;
    (void)hipFuncGetAttributes(&fa, (const void*)nerf_mlp_fwd_kernel<true>);
    fprintf(stderr, "[nrf] fwd<true>: lds %zu B, occupancy %d blocks/CU (err %d), regs %d, static lds %zu, scratch %zu\n", lds, nb, (int)e,
            fa.numRegs, fa.sharedSizeBytes, fa.localSizeBytes);
  }
  if (stash) {
    (void)hipFuncSetAttribute((const void*)nerf_mlp_fwd_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(nerf_mlp_fwd_kernel<true>, dim3(grid), dim3(256), lds, stream, p);
  } else {
    (void)hipFuncSetAttribute((const void*)nerf_mlp_fwd_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(nerf_mlp_fwd_kernel<false>, dim3(grid), dim3(256), lds, stream, p);
  }
}

// ---------------------------------------------------------------------------------------------
// backward: the bias-gradient registers (nerf_chain.h BwdAcc) of a workgroup, zeroed and flushed per level
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ void bwd_acc_zero(BwdAcc& c) {
#pragma unroll
  for (int l = 0; l < TRUNK_DEPTH; ++l) c.db_trunk[l][0] = c.db_trunk[l][1] = 0.f;
  c.db_bn[0] = c.db_bn[1] = 0.f;
  c.db_rgbh = 0.f;
  c.dsum[0] = c.dsum[1] = c.dsum[2] = c.dsum[3] = 0.f;
}

__device__ __forceinline__ void rgbx_bias_zero(const ChainBwdArgs& A) {
  const int lane = threadIdx.x & 63;
  if (lane < 32)   // the threads rgbx_bias_add writes from: feature n = wave * 32 + lane
    for (int x = 0; x < A.nx; ++x) A.small_part[(size_t)blockIdx.x * SMALL_PART + SP_DB_RGBX + x * RGB_W + (threadIdx.x >> 6) * 32 + lane] = 0.f;
}

// the per-workgroup partials of level A -> small_part[blockIdx.x]
__device__ __forceinline__ void bwd_flush(const ChainBwdArgs& A, float* smem, const BwdAcc& C) {
  float* dr = smem + ACT_FLOATS;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int j = lane & 31, h = lane >> 5;
  const float (&db_trunk)[TRUNK_DEPTH][2] = C.db_trunk;
  const float (&db_bn)[2] = C.db_bn;
  const float db_rgbh = C.db_rgbh;
  const float (&dsum)[4] = C.dsum;
  __syncthreads();   // dr may still be read by the tile just finished
  // ---- flush the per-workgroup partials ----
  float* sp = A.small_part + (size_t)blockIdx.x * SMALL_PART;
#pragma unroll
  for (int cb = 0; cb < 2; ++cb) {
    const int n = wave * 64 + 32 * cb + j;
#pragma unroll
    for (int l = 0; l < TRUNK_DEPTH; ++l) {
      const float v = db_trunk[l][cb] + __shfl_xor(db_trunk[l][cb], 32);
      if (h == 0) sp[SP_DB_TRUNK + l * TRUNK_W + n] = v;
    }
    const float vb = db_bn[cb] + __shfl_xor(db_bn[cb], 32);
    if (h == 0) sp[SP_DB_BN + n] = vb;
  }
  {
    const int n = wave * 32 + j;
    const float vr = db_rgbh + __shfl_xor(db_rgbh, 32);
    if (h == 0) sp[SP_DB_RGBH + n] = vr;
  }
  __syncthreads();
  if (tid < TILE_ROWS) {
#pragma unroll
    for (int c = 0; c < 4; ++c) dr[c * TILE_ROWS + tid] = dsum[c];
  }
  __syncthreads();
  if (tid < 4) {
    float s = 0.f;
    for (int q = 0; q < TILE_ROWS; ++q) s += dr[tid * TILE_ROWS + q];
    sp[tid < 3 ? SP_DB_LOGIT + tid : SP_DB_ALPHA] = s;
  }
  __syncthreads();
}

// Both levels in one launch (nerf_chain.h ChainBwdArgs2); the bias partials are flushed per level.
__global__ __launch_bounds__(256, Tile64::WG_PER_CU) void nerf_mlp_bwd_kernel(const ChainBwdArgs2 P) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  BwdAcc C;
  bwd_acc_zero(C);
  const int nt0 = P.nt0, ntot = P.ntot;
  int cur = -1;
  if (P.a[0].nx > 0) {
    rgbx_bias_zero(P.a[0]);
    if (ntot > nt0) rgbx_bias_zero(P.a[1]);
  }
  if ((int)blockIdx.x >= nt0 && nt0 > 0) bwd_flush(P.a[0], smem, C);   // no coarse tile for this workgroup: its partial is zero
#pragma unroll 1
  for (int g = blockIdx.x; g < ntot; g += gridDim.x) {
    const int lv = g >= nt0 ? 1 : 0;
    if (lv != cur) {
      if (cur == 0) { bwd_flush(P.a[0], smem, C); bwd_acc_zero(C); }
      cur = lv;
    }
    bwd_tile<Tile64>(P.a[lv], g - (lv ? nt0 : 0), 0, smem, C);
  }
  if (cur == 0) {
    bwd_flush(P.a[0], smem, C);
    if (ntot > nt0) { bwd_acc_zero(C); bwd_flush(P.a[1], smem, C); }
  } else if (cur == 1) {
    bwd_flush(P.a[1], smem, C);
  }
}

void launch_chain_bwd(const ChainBwdArgs& a0, const ChainBwdArgs* a1, int grid, hipStream_t stream) {
  const size_t lds = chain_lds_bytes<Tile64>(a0.d_points ? a0.PK : 4);
  (void)hipFuncSetAttribute((const void*)nerf_mlp_bwd_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  ChainBwdArgs2 p;
  p.a[0] = a0; p.a[1] = a1 ? *a1 : a0;
  p.nt0 = a0.ntiles; p.ntot = p.nt0 + (a1 ? a1->ntiles : 0);
  hipLaunchKernelGGL(nerf_mlp_bwd_kernel, dim3(grid), dim3(256), lds, stream, p);
}

// ---------------------------------------------------------------------------------------------
// weight packing: canonical [in,out] kernels -> per-wave B-fragment streams
// ---------------------------------------------------------------------------------------------
__global__ void pack_weights_kernel(const PackDesc* __restrict__ descs, const float* __restrict__ params,
                                    float* __restrict__ ws) {
  const PackDesc d = descs[blockIdx.y];
  const float* __restrict__ src = params + d.src_off;
  float* __restrict__ dst = ws + d.dst_off;
  const int ncols_wave = d.ncb == 2 ? 64 : 32;
  const int total = d.K * ncols_wave * d.nwaves;
  for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += gridDim.x * blockDim.x) {
    const int e = idx & 3, lane = (idx >> 2) & 63;
    const int per_it = 256;                       // floats per (wave, it)
    const int nit = d.ncb == 2 ? d.K / 4 : d.K / 8;
    const int it = (idx / per_it) % nit, w = idx / (per_it * nit);
    int k, n;
    if (d.ncb == 2) { k = 4 * it + 2 * (e >> 1) + (lane >> 5); n = 64 * w + 32 * (e & 1) + (lane & 31); }
    else            { k = 8 * it + 2 * e + (lane >> 5);        n = 32 * w + (lane & 31); }
    float v = 0.f;
    if (k < d.kvalid && n < d.nvalid)
      v = d.transposed ? src[(size_t)(d.src_row0 + n) * d.src_ld + k] : src[(size_t)(d.src_row0 + k) * d.src_ld + n];
    dst[idx] = v;
  }
}

void launch_pack(const PackDesc* d_descs, int ndesc, const float* params, float* ws, hipStream_t stream) {
  hipLaunchKernelGGL(pack_weights_kernel, dim3(64, ndesc), dim3(256), 0, stream, d_descs, params, ws);
}

}  // namespace nrf
