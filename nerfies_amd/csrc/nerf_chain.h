// The fused fp32 NeRF-MLP chain, written ONCE for both tilings: posenc -> 8x256 trunk (skip at 4) -> alpha head / bottleneck ->
// rgb branch, forward (fwd_tile) and data-gradient (bwd_tile) passes of one workgroup tile.  mlp_chain.hip instantiates them
// on 64-row tiles (Tile64, chain_common.h: two workgroups per CU), mlp_chain32.hip on 32-row tiles (Tile32 below: four per CU).
// The library picks the tiling per launch, so both must give a row the same bits: every per-element rounding sequence lives
// here, in one place, and the geometry only says where an element sits.
//
// Replaces (reference, /root/reference/nerfies):
//   modules.SinusoidalEncoder   modules.py:172-228  (fused into the tile prologue)
//   modules.MLP / NerfMLP       modules.py:26-62, 65-169
//   nn.sigmoid / sigma_activation  models.py:276-277
#pragma once
#include "chain_common.h"
#include "philox.h"

namespace nrf {

// ---------------------------------------------------------------------------------------------
// 32-row tiling.  Same math, same packed weights, same HBM images (fragment-order stash, ReLU sign bits, d raw / out4 rows)
// as the 64-row tiling -- a 32-row workgroup owns one HALF (T = 0 / 1) of a 64-row stash tile, so wgrad, the reduce passes and
// every reader of the workspace are untouched and the two tilings can be mixed launch by launch.
//
// Why a second tiling.  The 64-row kernel keeps 128 accumulators + two weight sets per wave (256 VGPRs): two waves per SIMD.
// A single wave issues one fp32 MFMA per 68.8 clocks (64 is the pipe rate) and ~12 % of a tile is outside K loops (prologue,
// VALU heads, epilogues); with two waves per SIMD a pair of tiles co-runs at 88 % of the MFMA rate.  Here a wave owns 32 rows
// x 64 columns: 32 accumulators, two 16-register weight sets, 8 A registers -> <= 128 VGPRs, FOUR waves per SIMD (4 x 40 KiB
// of LDS per CU), so every non-MFMA phase has three other waves' MFMA streams to hide under, tiles are half as long (launch
// tail / quantisation) and a 128-ray batch -- one GPU's share of the north star's 1024-ray batch on 8 GPUs: 128 + 384
// 64-row tiles for 512 workgroup slots -- becomes 256 + 768 half tiles for 1024 slots.  Cost: every B operand float feeds
// ONE MFMA instead of two, i.e. the packed weights stream from L2 at twice the rate (16 B/clk per CU, ~9.8 TB/s aggregate),
// and the A operand is read with ds_read_b32 (one row block) instead of ds_read_b64.
//
// Tile-row mapping: MFMA row i = half-tile row i (the 64-row kernel interleaves two row blocks: row 2i + rb).  Accumulator
// registers 4t..4t+3 of lane (j, h) are rows 8t + 4h .. +3 of column j: granule g' = 2t + h of the half tile = granule
// 8T + 2t + h of the 64-row tile.  In the 64-row fragment order that is float4 slot q = 4T + 2(t>>1) + h,
// lane' = j + 32 (t & 1) (chain_common.h frag_index), so a wave's store instruction writes two 512-byte runs.
// ---------------------------------------------------------------------------------------------
constexpr int HT_ROWS = 32;   // rows per half tile

// LDS address (floats) of granule (k, g): rows 4g..4g+3 of feature k, g = 0..7.  Swizzle with (k >> 1) & 7: the epilogue's
// ds_write_b128 (16 lanes = 16 consecutive features, one granule: 128 (k & 1) + 16 (g ^ ((k >> 1) & 7)) bytes mod 256) and
// the A operand's ds_read_b32 (32 rows of an even + 32 rows of an odd feature = 256 distinct bytes) are conflict free, and
// (k >> 1) & 7 is the k-step index inside a 16-k quad, so the per-lane read offsets are the same for every quad.
__device__ __forceinline__ int act32_addr(int k, int g) { return k * HT_ROWS + 4 * (g ^ ((k >> 1) & 7)); }
__device__ __forceinline__ int act32_elem(int k, int p) { return act32_addr(k, p >> 2) + (p & 3); }

// K loops: acc[cb] (32 rows x 32 columns each) += A[32 x K] * B[K x 64] for this wave.  Weight streams as in
// chain_common.h (NCB = 2: float4 = {ks0 cb0, ks0 cb1, ks1 cb0, ks1 cb1}, 4 k per float4; quad = 16 k = 4 float4).
template <int S0>
__device__ __forceinline__ void mfma32_half(f32x16 (&acc)[2], const float (&a)[4], const WQuad<2>& w) {
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const int ks = S0 + s;
    const float4 b = w.b[ks >> 1];
    acc[0] = mfma32(a[s], (ks & 1) ? b.z : b.x, acc[0]);
    acc[1] = mfma32(a[s], (ks & 1) ? b.w : b.y, acc[1]);
  }
}

template <bool SWZ>
__device__ __forceinline__ void k_loop32(f32x16 (&acc)[2], const float* lds_in, int nquads, const float4* __restrict__ wp, int lane,
                                         const WQuad<2>& first) {
  constexpr int QUAD_FLOATS = 16 * HT_ROWS;
  asm volatile("" : "+v"(lane));   // the offsets below are recomputed per call, not kept live across the layer loop
  const int i = lane & 31, kk = lane >> 5;
  int off[8];   // per-lane float offsets of the quad's 8 A reads (k = 2t + kk)
#pragma unroll
  for (int t = 0; t < 8; ++t) {
    const int k = 2 * t + kk;
    off[t] = SWZ ? act32_elem(k, i) : (k * HT_ROWS + i);
  }
  const float* ap = lds_in;
  const float4* bp = wp + lane;
  WQuad<2> bc = first;
  float a0[4], a1[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) a0[s] = ap[off[s]];
  auto quad = [&]() {
    WQuad<2> bn;   // weights run up to one quad past the end of the layer (the pack buffer is padded)
#pragma unroll
    for (int t = 0; t < 4; ++t) bn.b[t] = bp[(4 + t) * 64];
#pragma unroll
    for (int s = 0; s < 4; ++s) a1[s] = ap[off[4 + s]];
    mfma32_half<0>(acc, a0, bc);
#pragma unroll
    for (int s = 0; s < 4; ++s) a0[s] = ap[QUAD_FLOATS + off[s]];
    mfma32_half<4>(acc, a1, bc);
    __builtin_amdgcn_sched_group_barrier(0x020, 4, 0);   // VMEM read: next quad's weights
    __builtin_amdgcn_sched_group_barrier(0x100, 4, 0);   // DS read: second half of this quad
    __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);   // MFMA
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);   // DS read (next quad)
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);   // MFMA
    }
    __builtin_amdgcn_sched_group_barrier(0x008, 8, 0);
    bc = bn;
    ap += QUAD_FLOATS;
    bp += 4 * 64;
  };
  if (nquads > 0) quad();   // peeled: an exact vmcnt behind the previous epilogue's stash stores (chain_common.h mfma_k_loop)
#pragma unroll 2
  for (int q = 1; q < nquads; ++q) quad();
}

// 32 columns per wave (NCB = 1 stream: float4 = ks0..ks3, 8 k per float4; quad = 2 float4).  ONE accumulator, k-steps in order:
// the same fmaf chain per output element as the 64-row kernel, so the two tilings agree bit for bit (a sub-batch of rays, which
// may run on the other tiling, reproduces its rows exactly: tests/test_gpu_fullsize.py).  The chain of dependent MFMAs costs a
// lone wave some issue slots; this layer is 5 % of a tile and the other waves of the SIMD fill them.
template <bool SWZ>
__device__ __forceinline__ void k_loop32_n1(f32x16& acc, const float* lds_in, int nquads, const float4* __restrict__ wp, int lane,
                                            const WQuad<1>& first) {
  constexpr int QUAD_FLOATS = 16 * HT_ROWS;
  asm volatile("" : "+v"(lane));
  const int i = lane & 31, kk = lane >> 5;
  int off[8];
#pragma unroll
  for (int t = 0; t < 8; ++t) {
    const int k = 2 * t + kk;
    off[t] = SWZ ? act32_elem(k, i) : (k * HT_ROWS + i);
  }
  const float* ap = lds_in;
  const float4* bp = wp + lane;
  WQuad<1> bc = first;
#pragma unroll 2
  for (int q = 0; q < nquads; ++q) {
    WQuad<1> bn;
    bn.b[0] = bp[2 * 64];
    bn.b[1] = bp[3 * 64];
    float a[8];
#pragma unroll
    for (int s = 0; s < 8; ++s) a[s] = ap[off[s]];
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) {
      const float4 b = bc.b[ks >> 2];
      const float bv = (ks & 3) == 0 ? b.x : (ks & 3) == 1 ? b.y : (ks & 3) == 2 ? b.z : b.w;
      acc = mfma32(a[ks], bv, acc);
    }
    bc = bn;
    ap += QUAD_FLOATS;
    bp += 2 * 64;
  }
}

struct Tile32 {
  static constexpr int ROWS = HT_ROWS;
  static constexpr int RB = 1;
  static constexpr int NPIECE = 4;
  static constexpr int PARTS = 8;          // per-row (VALU) phases: 8 threads per row, part = 2 wave + h, row = lane & 31
  static constexpr int WG_PER_CU = 4;
  static constexpr int SCRATCH_ROWS = 12;  // the VALU heads need 4 x 3 logit partials behind the activation tile
  static constexpr bool FULL = false;      // one-layer rgb branch, no d points: chain32_for refuses the rest
  static constexpr bool BIAS_IN_REGS = false;   // no room for BwdAcc at 128 VGPRs: bias32_add
  __device__ static __forceinline__ int row0(int tile, int T) { return tile * TILE_ROWS + HT_ROWS * T; }
  __device__ static __forceinline__ int part(int wave, int h) { return 2 * wave + h; }
  __device__ static __forceinline__ int prow(int lane) { return lane & 31; }
  __device__ static __forceinline__ bool part_writer(int h) { return h == 0; }   // both lane halves run a row's chain; half 0 keeps it
  __device__ static __forceinline__ int epilogue_lane(int lane) {
    asm volatile("" : "+v"(lane));   // epilogue-local lane constants: not live across the K loops
    return lane;
  }
  __device__ static __forceinline__ int addr(int k, int g) { return act32_addr(k, g); }
  __device__ static __forceinline__ int elem(int k, int p) { return act32_elem(k, p); }
  __device__ static __forceinline__ int granule(int t, int h) { return 2 * t + h; }
  template <int NCB>
  __device__ static __forceinline__ float4 piece(const f32x16 (&acc)[1][NCB], int cb, int t) {
    const f32x16& a = acc[0][cb];
    return make_float4(a[4 * t], a[4 * t + 1], a[4 * t + 2], a[4 * t + 3]);
  }
  // byte offset of piece t of lane (j, h) inside one 8 KiB feature block of a 64-row fragment tile, half T
  __device__ static __forceinline__ int frag_voff(int lane, int t) { return ((lane & 31) + 32 * (t & 1)) * 16 + (lane >> 5) * 1024; }
  __device__ static __forceinline__ int frag_slot(int T, int t) { return (4 * T + 2 * (t >> 1)) * 1024; }
  template <int NCB, bool SWZ>
  __device__ static __forceinline__ void k_loop(f32x16 (&acc)[1][NCB], const float* lds_in, int nquads, const float4* __restrict__ wp, int lane,
                                                const WQuad<NCB>& first) {
    if constexpr (NCB == 2) k_loop32<SWZ>(acc[0], lds_in, nquads, wp, lane, first);
    else k_loop32_n1<SWZ>(acc[0][0], lds_in, nquads, wp, lane, first);
  }
  // Sign nibbles of a lane's four pieces (nibble t at bits 4t of nib[cb]) -> the 64-row kernel's bit image.  There, the word of
  // lane (j, ho) and column block cb holds nibble q = granule (q & 1) + 2 ho + 4 (q >> 1); piece t of lane (j, h) here is granule
  // 8T + 2t + h, i.e. nibble 4T + 2 (t >> 1) + h of the word of lane (j, t & 1): half T of every word belongs to this workgroup,
  // and the two lanes (j, 0) / (j, 1) swap two nibbles per column block so that each writes its own lane's 16-bit half.  One
  // exchange serves all column blocks: it runs when the last one is complete.
  template <int NCB>
  __device__ static __forceinline__ void bits_store(const uint32_t (&nib)[NCB], int cb_done, uint32_t* words_wave, int lane, int T) {
    if (cb_done != NCB - 1) return;
    asm volatile("" : "+v"(lane));
    const int h = lane >> 5;
    uint32_t send = 0;
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb) {
      const uint32_t n0 = nib[cb] & 15u, n1 = (nib[cb] >> 4) & 15u, n2 = (nib[cb] >> 8) & 15u, n3 = (nib[cb] >> 12) & 15u;
      send |= (h ? (n0 | (n2 << 4)) : (n1 | (n3 << 4))) << (8 * cb);
    }
    const uint32_t recv = (uint32_t)__shfl_xor((int)send, 32);
    uint16_t* out = reinterpret_cast<uint16_t*>(words_wave);
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb) {
      const uint32_t n0 = nib[cb] & 15u, n1 = (nib[cb] >> 4) & 15u, n2 = (nib[cb] >> 8) & 15u, n3 = (nib[cb] >> 12) & 15u;
      const uint32_t rc = (recv >> (8 * cb)) & 255u;
      const uint32_t half = h ? ((rc & 15u) | (n1 << 4) | ((rc >> 4) << 8) | (n3 << 12)) : (n0 | ((rc & 15u) << 4) | (n2 << 8) | ((rc >> 4) << 12));
      out[(lane * NCB + cb) * 2 + T] = (uint16_t)half;
    }
  }
  // the mask of piece t of lane (., h) comes from the two words (lane halves 0 / 1) of its column
  template <int NCB> struct Mask { uint32_t w[2][NCB]; };
  template <int NCB>
  __device__ static __forceinline__ Mask<NCB> mask_load(const uint32_t* words_wave, int lane) {
    const int j = lane & 31;
    Mask<NCB> m;
    if constexpr (NCB == 2) {
      const uint2 mq0 = *reinterpret_cast<const uint2*>(words_wave + j * 2);
      const uint2 mq1 = *reinterpret_cast<const uint2*>(words_wave + (j + 32) * 2);
      m.w[0][0] = mq0.x; m.w[0][1] = mq0.y; m.w[1][0] = mq1.x; m.w[1][1] = mq1.y;
    } else {
      m.w[0][0] = words_wave[j]; m.w[1][0] = words_wave[j + 32];
    }
    return m;
  }
  template <int NCB>
  __device__ static __forceinline__ uint32_t mask_nibble(const Mask<NCB>& m, int cb, int T, int t, int h) {
    return (m.w[t & 1][cb] >> (16 * T + 4 * (2 * (t >> 1) + h))) & 15u;
  }
  // posenc tile [k][32 rows] in LDS -> this half of its 64-row fragment-order stash tile (chain_common.h stash_tile_from_lds)
  __device__ static __forceinline__ void stash_posenc(const float* tile_lds, int kvalid, int nblocks, float* stash_tile, int T, int wave, int lane) {
    const __amdgpu_buffer_rsrc_t r = make_rsrc(stash_tile, nblocks * 32 * TILE_ROWS * 4);
    const int j = lane & 31, kk = lane >> 5;
    for (int pp = wave; pp < nblocks * 4; pp += 4) {
      const int blk = pp >> 2, qq = pp & 3;
      const int k = blk * 32 + j, g = (qq & 1) + 2 * kk + 4 * (qq >> 1);
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (k < kvalid) v = *reinterpret_cast<const float4*>(tile_lds + k * HT_ROWS + 4 * g);
      buf_store4(v, r, lane * 16, (blk * 8 + 4 * T + qq) * 1024);
    }
  }
};

// dynamic LDS of a chain kernel: the activation tile [256][ROWS] and `rows` scratch rows behind it
template <class G>
inline size_t chain_lds_bytes(int rows) { return (size_t)(TRUNK_W + rows) * G::ROWS * sizeof(float); }
template <class G>
inline size_t chain_fwd_lds_bytes(int pk) { return chain_lds_bytes<G>(pk > G::SCRATCH_ROWS ? pk : G::SCRATCH_ROWS); }

// ---------------------------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ float sigma_activation(float x, int kind) {
  if (kind == 1) {  // softplus, computed as jax.nn.softplus = logaddexp(x, 0)
    return fmaxf(x, 0.f) + log1pf(expf(-fabsf(x)));
  }
  return relu(x);
}

// The arguments are read through a run-time index into the kernarg segment (always 0: gridDim.x < 2^24): hipcc then fetches
// each field with a scalar load where it is used instead of keeping the whole 700-byte struct in SGPRs for the lifetime of the
// kernel (round 2: 116 spilled SGPRs, parked in VGPR lanes of a kernel that is out of VGPRs).
struct ChainFwdArgs1 { ChainFwdArgs a[1]; };

// One tile of the forward chain: 64-row tile `tile`, or its half T on 32-row tiles.  STAMP() marks a phase boundary for the
// in-kernel timeline of the 64-row kernel (a no-op otherwise).  STASH (chain_common.h): STASH_BITS keeps the posenc stash and the
// sign words and stores no activation.
// DENSITY (field queries, chain_query.hip / chain_query_grad.hip; 64-row tiles): the tile ends at the alpha head.  It runs the prologue,
// the posenc stash (if STASH), the eight trunk layers and the head -- a use_alpha_condition model also the bottleneck layer its head
// reads, unstashed, and the per-group code term -- and stores sigma[rows] = sigma_activation(raw) (may be nullptr) and, if STASH,
// dsig[ntiles * 64] = sigma'(raw), the start of bwd_tile<., ., false, true>.  No rgb branch, logits or noise term; every rounding of
// a row's sigma is the full chain's, so the two give the same bits.  A density launch reads params / po / wpk / pk / points / rows /
// ntiles / F / P / PK / skip / sigma_act / alpha_ct, S and B with alpha_ct, st_pe and bits_trunk with STASH.
template <class G, int STASH, bool DENSITY = false, class Stamp>
__device__ __forceinline__ void fwd_tile(const ChainFwdArgs& A, const int tile, const int T, float* smem, const int tid0, const int wave,
                                         Stamp& STAMP, float* __restrict__ sigma = nullptr, float* __restrict__ dsig = nullptr) {
  static_assert(G::FULL || !DENSITY, "density mode: 64-row tiles only (the 32-row K loop spills, profiles/field_query.md)");
  constexpr int ROWS = G::ROWS;
  float* act = smem;                  // [256][ROWS] swizzled
  float* pe = smem + TRUNK_W * ROWS;  // [max(PK, G::SCRATCH_ROWS)][ROWS]; reused as scratch after the skip layer
  const float* __restrict__ prm = A.params;
  const int PK = A.PK;
  const int PKS = (PK + 31) / 32 * 32;   // features per posenc stash tile (whole 32-feature blocks)
  const int nq_pe = PK / 16;
  // the lane index is made opaque once per tile: everything derived from it (fragment addresses, row indices, mask shifts)
  // is then recomputed per tile instead of being hoisted out of the tile loop into registers that live -- i.e. spill -- across
  // the whole kernel (hipcc hoists ~50 such per-lane constants otherwise)
  int tid = tid0;
  asm volatile("" : "+v"(tid));
  const int lane = tid & 63;
  const int j = lane & 31, h = lane >> 5;
  const int p = G::prow(lane);          // tile row handled in the per-row (VALU) phases ...
  const int part = G::part(wave, h);    // ... by PARTS threads, this one's share of the work
  const int row0 = G::row0(tile, T);
  // ---- prologue: sample point + SinusoidalEncoder (modules.py:213-228) ----
  {
    int r = row0 + p;
    r = r < A.rows ? r : A.rows - 1;
    float x[3];
    if (DENSITY || A.points) {   // a density launch always has points
      x[0] = A.points[3 * r]; x[1] = A.points[3 * r + 1]; x[2] = A.points[3 * r + 2];
    } else {
      const int ray = r / A.S;
      const float z = A.zvals[r];
#pragma unroll
      for (int c = 0; c < 3; ++c)   // origins + z_vals * directions  (model_utils.py:72-73)
        x[c] = __fadd_rn(A.origins[3 * ray + c], __fmul_rn(z, A.directions[3 * ray + c]));
    }
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
  if (STASH) G::stash_posenc(pe, PK, PKS / 32, A.st_pe + (size_t)tile * PKS * TILE_ROWS, T, wave, lane);   // posenc stash, coalesced

  STAMP();   // prologue done
  f32x16 acc[G::RB][2];
  const float4* wpk4 = reinterpret_cast<const float4*>(A.wpk);
  const size_t st_h_layer = (size_t)A.ntiles * FRAG_TILE_256;       // floats
  const int wv_soff = wave * 2 * 8 * 1024;                           // bytes: this wave's slice of a tile

  // ---- trunk: 8 x Dense(256)+ReLU, skip concat [h, posenc] at layer 4 (modules.py:41-50) ----
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
    // the next layer's first weights go out before this layer's stash stores
    wnext = prefetch_quad<2>(wpk4 + ((l + 1 < TRUNK_DEPTH ? A.pk.fwd_L[l + 1] : A.pk.fwd_bn) / 4) + wave * 64 * 64, lane);
    bnext = bias_load<2>(prm + (l + 1 < TRUNK_DEPTH ? A.po.trunk_b[l + 1] : A.po.bn_b), wave * 64, lane);   // ... and its bias (chain_common.h)
    __builtin_amdgcn_sched_barrier(0);
    STAMP();   // k loop of layer l issued
    fwd_epilogue<2, EPI_RELU, STASH, G>(
        acc, wave * 64, act,
        make_rsrc(STASH == STASH_FULL ? A.st_h + l * st_h_layer + (size_t)tile * FRAG_TILE_256 : nullptr, FRAG_TILE_256 * 4), wv_soff,
        STASH ? A.bits_trunk + (((size_t)l * A.ntiles + tile) * 4 + wave) * 128 : nullptr, lane, T);
    STAMP();   // epilogue of layer l done
  }

  // ---- alpha head: Dense(256->1) on the trunk output, or -- use_alpha_condition -- Dense(256+A->1) on
  //      [bottleneck, appearance code] with the per-ray code term from ray_prep (modules.py:152-157).  Four partial sums in
  //      every tiling (wave w: the fmaf chain over k = 64 w .. 64 w + 63), combined in one order ----
  float sigma_raw = 0.f;
  auto alpha_head = [&]() {
    // weights in chunks of 16 (wave-uniform -> one s_load_dwordx16 per chunk instead of a scalar load and a
    // wait per k), activations as 16 independent LDS reads
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
    if (G::part_writer(h)) pe[wave * ROWS + p] = s;   // scratch (posenc no longer needed for this tile)
    __syncthreads();
    if (part == 0)
      sigma_raw = (pe[p] + pe[ROWS + p]) + (pe[2 * ROWS + p] + pe[3 * ROWS + p]) + prm[A.po.alpha_b];
  };
  if (!A.alpha_ct) alpha_head();

  STAMP();   // alpha head done
  // ---- density mode: the tile ends here.  Only a use_alpha_condition model's head reads the bottleneck; nothing is kept of it ----
  if constexpr (DENSITY) {
    if (A.alpha_ct) {
      bias_set<2>(acc, bnext);
      G::template k_loop<2, true>(acc, act, 16, wpk4 + (A.pk.fwd_bn / 4) + wave * 64 * 64, lane, wnext);
      __builtin_amdgcn_sched_barrier(0);
      fwd_epilogue<2, EPI_LINEAR, STASH_NONE, G>(acc, wave * 64, act, make_rsrc(nullptr, FRAG_TILE_256 * 4), 0, nullptr, lane, T);
      alpha_head();
      if (part == 0) sigma_raw += A.alpha_ct[min((row0 + p) / A.S, A.B - 1)];
    }
    if (part == 0) {
      const float sg = sigma_activation(sigma_raw, A.sigma_act);
      if (sigma != nullptr && row0 + p < A.rows) sigma[(size_t)row0 + p] = sg;
      // sigma'(raw): softplus' = sigmoid(raw) = 1 - exp(-sigma) from the activated value (ray_kernels.hip composite_bwd), relu'
      if constexpr (STASH != STASH_NONE) dsig[(size_t)row0 + p] = A.sigma_act == 1 ? -expm1f(-sg) : (sg > 0.f ? 1.f : 0.f);
    }
    __syncthreads();   // scratch (aliases pe) is free again for the next tile's prologue
    return;
  }
  // ---- bottleneck: Dense(256), no activation (modules.py:149-150) ----
  bias_set<2>(acc, bnext);
  G::template k_loop<2, true>(acc, act, 16, wpk4 + (A.pk.fwd_bn / 4) + wave * 64 * 64, lane, wnext);
  const float4* wrgb = wpk4 + (A.pk.fwd_rgbh / 4) + wave * 32 * 64;
  const WQuad<1> wrgb0 = prefetch_quad<1>(wrgb, lane);
  __builtin_amdgcn_sched_barrier(0);
  fwd_epilogue<2, EPI_LINEAR, STASH == STASH_FULL ? STASH_FULL : STASH_NONE, G>(
      acc, wave * 64, act,
      make_rsrc(STASH == STASH_FULL ? A.st_bn + (size_t)tile * FRAG_TILE_256 : nullptr, FRAG_TILE_256 * 4), wv_soff, nullptr, lane, T);
  if (A.alpha_ct) {
    alpha_head();   // the scratch is next written by the rgb logits, two barriers further on
    if (part == 0) sigma_raw += A.alpha_ct[min((row0 + p) / A.S, A.B - 1)];
  }

  STAMP();   // bottleneck done
  // ---- rgb branch hidden: Dense(256+R -> 128)+ReLU; the R per-ray condition columns are
  //      folded into condterm[ray][n] (= cond . W[256:] + bias) by ray_prep ----
  {
    f32x16 acc1[G::RB][1];
    zero_acc<1>(acc1);
    const int n = wave * 32 + j;
    // rows visited by this lane increase with q: walk the ray boundaries instead of dividing.  The first
    // condition term is fetched before the K loop so that its latency hides under the MFMAs.
    int ray = row0 / A.S;
    int nextb = (ray + 1) * A.S - row0;   // first tile row of the next ray
    float ct = A.condterm[(size_t)min(ray, A.B - 1) * RGB_W + n];
    G::template k_loop<1, true>(acc1, act, 16, wrgb, lane, wrgb0);
    const __amdgpu_buffer_rsrc_t st = make_rsrc(STASH == STASH_FULL ? A.st_rgbh + (size_t)tile * FRAG_TILE_128 : nullptr, FRAG_TILE_128 * 4);
    __syncthreads();
    uint32_t mb[1] = {0u};
#pragma unroll
    for (int q = 0; q < G::NPIECE; ++q) {
      const int g = G::granule(q, h);
      const float4 a4 = G::template piece<1>(acc1, 0, q);
      const float av[4] = {a4.x, a4.y, a4.z, a4.w};
      float v[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int pr = 4 * g + e;
        while (pr >= nextb) { ++ray; nextb += A.S; ct = A.condterm[(size_t)min(ray, A.B - 1) * RGB_W + n]; }
        v[e] = av[e] + ct;
      }
      float4 v4 = make_float4(v[0], v[1], v[2], v[3]);
      if (STASH) mb[0] |= sign_nibble(v4) << (4 * q);
      v4.x = relu(v4.x); v4.y = relu(v4.y); v4.z = relu(v4.z); v4.w = relu(v4.w);
      *reinterpret_cast<float4*>(act + G::addr(n, g)) = v4;
      if (STASH == STASH_FULL) buf_store4(v4, st, G::frag_voff(lane, q), wave * 8 * 1024 + G::frag_slot(T, q));
    }
    if (STASH) G::template bits_store<1>(mb, 0, A.bits_rgbh + ((size_t)tile * 4 + wave) * 64, lane, T);
    __syncthreads();
  }

  // ---- rgb branch layers 1..nx (nerf_rgb_branch_depth = nx + 1, modules.py:41-50): Dense(128 -> 128)+ReLU on the LDS image of
  //      the layer before; nx = 0 for every depth-1 model, which runs none of this.  64-row tiles only ----
  if constexpr (G::FULL) {
#pragma unroll 1
    for (int x = 0; x < A.nx; ++x) {
      f32x16 acc1[G::RB][1];
      zero_acc<1>(acc1);
      const int n = wave * 32 + j;
      const float4* wx = wpk4 + ((A.pk.fwd_rgbx + x * RGB_W * RGB_W) / 4) + wave * 16 * 64;
      const float bx = prm[A.po.rgbx_b[x] + n];
      G::template k_loop<1, true>(acc1, act, 8, wx, lane, prefetch_quad<1>(wx, lane));
      const __amdgpu_buffer_rsrc_t st =
          make_rsrc(STASH == STASH_FULL ? A.st_rgbx + ((size_t)x * A.ntiles + tile) * FRAG_TILE_128 : nullptr, FRAG_TILE_128 * 4);
      __syncthreads();
      uint32_t mb[1] = {0u};
#pragma unroll
      for (int q = 0; q < G::NPIECE; ++q) {
        const int g = G::granule(q, h);
        float4 v4 = G::template piece<1>(acc1, 0, q);
        v4.x += bx; v4.y += bx; v4.z += bx; v4.w += bx;
        if (STASH) mb[0] |= sign_nibble(v4) << (4 * q);
        v4.x = relu(v4.x); v4.y = relu(v4.y); v4.z = relu(v4.z); v4.w = relu(v4.w);
        *reinterpret_cast<float4*>(act + G::addr(n, g)) = v4;
        if (STASH == STASH_FULL) buf_store4(v4, st, G::frag_voff(lane, q), wave * 8 * 1024 + G::frag_slot(T, q));
      }
      if (STASH) G::template bits_store<1>(mb, 0, A.bits_rgbx + (((size_t)x * A.ntiles + tile) * 4 + wave) * 64, lane, T);
      __syncthreads();
    }
  }

  STAMP();   // rgb hidden done
  // ---- rgb logits Dense(128->3), sigmoid; sigma activation (models.py:276-277).  As the alpha head: four partial sums
  //      (wave w: k = 32 w .. 32 w + 31 in order), combined in one order ----
  {
    // [128][3] row-major: this wave's 32 k = 96 consecutive floats, read as 6 chunks of 16
    const float4* __restrict__ wl4 = reinterpret_cast<const float4*>(prm + A.po.logit_k) + wave * 24;
    float sc[3] = {0.f, 0.f, 0.f};
    const int k0 = wave * 32;
#pragma unroll 1
    for (int kc = 0; kc < 2; ++kc) {   // 16 k = 48 weights per trip
      float4 w4[12];
#pragma unroll
      for (int i = 0; i < 12; ++i) w4[i] = wl4[12 * kc + i];
      const float* wf = reinterpret_cast<const float*>(w4);
      float a[16];
#pragma unroll
      for (int i = 0; i < 16; ++i) a[i] = act[G::elem(k0 + 16 * kc + i, p)];
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        sc[0] = fmaf(a[i], wf[3 * i], sc[0]); sc[1] = fmaf(a[i], wf[3 * i + 1], sc[1]); sc[2] = fmaf(a[i], wf[3 * i + 2], sc[2]);
      }
    }
    if (G::part_writer(h)) {
#pragma unroll
      for (int c = 0; c < 3; ++c) pe[(3 * wave + c) * ROWS + p] = sc[c];
    }
    __syncthreads();
    if (part == 0) {
      float t[3];
#pragma unroll
      for (int c = 0; c < 3; ++c)
        t[c] = (pe[c * ROWS + p] + pe[(3 + c) * ROWS + p]) + (pe[(6 + c) * ROWS + p] + pe[(9 + c) * ROWS + p]) +
               prm[A.po.logit_b + c];
      float4 o;
      o.x = 1.f / (1.f + expf(-t[0])); o.y = 1.f / (1.f + expf(-t[1])); o.z = 1.f / (1.f + expf(-t[2]));
      if (A.noise_std > 0.f) {   // model_utils.noise_regularize (model_utils.py:266-282)
        const int row = row0 + p;
        const float nz = A.noise ? A.noise[min(row, A.rows - 1)]
                                 : philox_normal(A.dyn ? A.dyn->rng_seed : A.noise_seed, A.dyn ? A.dyn->rng_offset : A.noise_offset, A.noise_stream, (uint32_t)row);
        sigma_raw = __fadd_rn(sigma_raw, __fmul_rn(nz, A.noise_std));
      }
      o.w = sigma_activation(sigma_raw, A.sigma_act);
      A.out4[(size_t)row0 + p] = o;
    }
    __syncthreads();   // scratch (aliases pe) is free again for the next tile's prologue
  }
}

// ---------------------------------------------------------------------------------------------
// backward (data gradients; bias gradients accumulated per workgroup)
// ---------------------------------------------------------------------------------------------
// (small_part layout: nrf_internal.h SP_DB_*)

// Where a tile's column sums (bias gradients) go is the one thing the tilings do differently.
// 64-row tiles: per-lane accumulators of one workgroup, carried across its tiles of one level and flushed once
// (mlp_chain.hip bwd_flush).
struct BwdAcc {
  float db_trunk[TRUNK_DEPTH][2];
  float db_bn[2];
  float db_rgbh;
  float dsum[4];   // threads < 64: column sums of d_raw (logit / alpha bias grads)
};
struct NoBwdAcc {};
// 32-row tiles: at 128 VGPRs there is no room for them next to 32 accumulators + two weight sets, so every half tile adds its
// column sums (lane halves combined by one shuffle) straight into the workgroup's OWN slice of small_part with fire-and-forget
// float atomics -- no contention (the slice is private), ~2.4 k atomics per half tile next to 330 KB of dY stores.  The host
// zeroes small_part before the launch; the reduce pass sums the slices as before.
__device__ __forceinline__ void bias32_add(float* sp, float v, int h) {
  v += __shfl_xor(v, 32);
  if (h == 0) atomicAdd(sp, v);
}
// Bias gradients of the rgb branch layers 1..nx (64-row tiles).  The reverse kernel has no register to spare for more per-lane
// accumulators (it sits at the 256-register bound), so these partials live in the workgroup's own small_part row: zeroed by the
// workgroup when the kernel starts, added to once per tile by the one thread that owns feature n (lane half 0) -- no atomics, a
// fixed order.
__device__ __forceinline__ void rgbx_bias_add(const ChainBwdArgs& A, int x, int n, int h, float bsum) {
  const float v = bsum + __shfl_xor(bsum, 32);
  if (h == 0) {
    float* o = A.small_part + (size_t)blockIdx.x * SMALL_PART + SP_DB_RGBX + x * RGB_W + n;
    *o += v;
  }
}

// Reverse epilogue of one column block of a lane: piece q = src(q, g) [+ ds (x) wa, the alpha head's d sigma_raw term]
// [* ReLU mask] -> LDS tile (the next step's A operand) and (DY) the dY image; returns bsum + the column sum of what was written.
template <class G, bool DY, class Src, class Msk>
__device__ __forceinline__ float bwd_epilogue(Src src, bool add_ds, const float* ds_row, float wa, Msk mask, float bsum, int n, float* act,
                                              __amdgpu_buffer_rsrc_t dy, int soff, int lane, int T) {
  const int h = lane >> 5;
#pragma unroll
  for (int q = 0; q < G::NPIECE; ++q) {
    const int g = G::granule(q, h);
    float4 v = src(q, g);
    if (add_ds) {
      const float4 ds = *reinterpret_cast<const float4*>(ds_row + 4 * g);
      v.x = fmaf(ds.x, wa, v.x); v.y = fmaf(ds.y, wa, v.y); v.z = fmaf(ds.z, wa, v.z); v.w = fmaf(ds.w, wa, v.w);
    }
    v = mask(v, q);
    bsum += (v.x + v.y) + (v.z + v.w);
    *reinterpret_cast<float4*>(act + G::addr(n, g)) = v;
    if constexpr (DY) buf_store4(v, dy, G::frag_voff(lane, q), soff + G::frag_slot(T, q));
  }
  return bsum;
}

// One tile of level A (tile = index inside the level; T = its half on 32-row tiles).  C: BwdAcc on 64-row tiles.
// DY = false (frozen-field plans, NRF_FLAG_FROZEN: the reverse pass stops at the rays): the chain still forms every dpre tile in
// LDS, accumulates dray and writes d_points, but stores no dY image and keeps no bias column sum (C: NoBwdAcc; small_part unused).
// DENS (gradient queries, chain_query_grad.hip; 64-row tiles, DY = false): the reverse starts at the density.  dsig [ntiles * 64] =
// sigma'(raw) (fwd_tile<., STASH_BITS, true>) takes the place of d sigma_raw and there is no d rgb: no logit^T, rgb branch, per-ray
// sums or d-bottleneck GEMM.  ds enters at the alpha head -- dpre_7 = mask_7(ds (x) w_alpha) needs no GEMM; a use_alpha_condition
// model: d bn = ds (x) w_alpha[0:256], then the W_bn^T step -- and runs down the trunk and through the d-posenc section as it stands.
// Nothing is accumulated across rows, so there is no atomic and a row's gradient does not depend on the launch it ran in.  A density
// launch reads params / po / wpk / pk / rows / ntiles / bits_trunk / d_points (always set) / st_pe / F / P / PK / skip / alpha_on_bn.
template <class G, class Acc, bool DY = true, bool DENS = false>
__device__ __forceinline__ void bwd_tile(const ChainBwdArgs& A, const int tile, const int T, float* smem, Acc& C,
                                         const float* __restrict__ dsig = nullptr) {
  static_assert(!DENS || (G::FULL && !DY), "density start: 64-row tiles (the d-points section), no dY image, no bias sums");
  constexpr int ROWS = G::ROWS;
  constexpr bool REGS = G::BIAS_IN_REGS && DY;    // bias column sums in the workgroup's registers ...
  constexpr bool ATOM = !G::BIAS_IN_REGS && DY;   // ... or added to its small_part slice
  float* act = smem;                    // [256][ROWS] swizzled: current dpre tile
  float* dr = smem + TRUNK_W * ROWS;    // [4][ROWS]: d raw rgb (3) and d raw sigma of the tile rows
  int tid = threadIdx.x;
  asm volatile("" : "+v"(tid));
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int row0 = G::row0(tile, T);
  const float* __restrict__ prm = A.params;
  const float4* wpk4 = reinterpret_cast<const float4*>(A.wpk);
  const size_t layer_fl = (size_t)A.ntiles * FRAG_TILE_256;   // floats per trunk layer
  const int wv = wave * 2 * 8 * 1024;                           // bytes: this wave's slice of a tile
  [[maybe_unused]] float* sp = A.small_part + (size_t)blockIdx.x * SMALL_PART;
  const auto no_mask = [](const float4& v, int) { return v; };
  if constexpr (DENS) {
    // ---- density start: sigma'(raw) of the tile rows -> the d sigma_raw row (read behind the next barrier) ----
    if (tid < ROWS) dr[3 * ROWS + tid] = dsig[(size_t)row0 + tid];
  } else {
    // ---- d raw of the tile rows -> LDS; its column sums are the logit / alpha bias gradients ----
    if (tid < ROWS) {
      const float4 d = A.d_raw4[(size_t)row0 + tid];
      dr[tid] = d.x; dr[ROWS + tid] = d.y; dr[2 * ROWS + tid] = d.z; dr[3 * ROWS + tid] = d.w;
      if constexpr (REGS) { C.dsum[0] += d.x; C.dsum[1] += d.y; C.dsum[2] += d.z; C.dsum[3] += d.w; }
    } else if (ATOM && tid >= 64 && tid < 64 + ROWS) {   // wave 1, lanes 0..31 sum the columns
      const float4 d = A.d_raw4[(size_t)row0 + tid - 64];
      float s0 = d.x, s1 = d.y, s2 = d.z, s3 = d.w;
  #pragma unroll
      for (int o = 16; o > 0; o >>= 1) { s0 += __shfl_xor(s0, o); s1 += __shfl_xor(s1, o); s2 += __shfl_xor(s2, o); s3 += __shfl_xor(s3, o); }
      if (tid == 64) {
        atomicAdd(sp + SP_DB_LOGIT, s0); atomicAdd(sp + SP_DB_LOGIT + 1, s1); atomicAdd(sp + SP_DB_LOGIT + 2, s2);
        atomicAdd(sp + SP_DB_ALPHA, s3);
      }
    }
    __syncthreads();

    // ---- rgb logit^T (3 -> 128) on the VALU, ReLU mask of the rgb hidden layer ----
    {
      int ln = lane;
      asm volatile("" : "+v"(ln));   // section-local lane constants (see the d posenc section)
      const int lane = ln, j = ln & 31, h = ln >> 5;
      const int n = wave * 32 + j;
      const float w0 = prm[A.po.logit_k + 3 * n], w1 = prm[A.po.logit_k + 3 * n + 1], w2 = prm[A.po.logit_k + 3 * n + 2];
      // the logits read the LAST rgb layer: layer nx's mask, dY image and bias partial when the branch is deeper than one layer
      const int nx = G::FULL ? A.nx : 0;
      const size_t xt = nx ? (size_t)(nx - 1) * A.ntiles + tile : 0;
      const auto mb = G::template mask_load<1>(nx ? A.bits_rgbx + (xt * 4 + wave) * 64 : A.bits_rgbh + ((size_t)tile * 4 + wave) * 64, lane);
      const __amdgpu_buffer_rsrc_t dy =
          make_rsrc(nx ? A.dy_rgbx + xt * FRAG_TILE_128 : A.dy_rgbh + (size_t)tile * FRAG_TILE_128, FRAG_TILE_128 * 4);
      float bsum = 0.f;
      if constexpr (REGS) bsum = nx ? 0.f : C.db_rgbh;
      bsum = bwd_epilogue<G, DY>(
          [&](int, int g) {
            const float4 d0 = *reinterpret_cast<const float4*>(dr + 4 * g);
            const float4 d1 = *reinterpret_cast<const float4*>(dr + ROWS + 4 * g);
            const float4 d2 = *reinterpret_cast<const float4*>(dr + 2 * ROWS + 4 * g);
            // d0 w0 + d1 w1 + d2 w2 with the rounding steps spelled out (one product, two fused multiply-adds): left to the
            // compiler's contraction, the grouping depends on the code around it, and every tiling must produce the same bits
            auto dot3 = [&](float a0, float a1, float a2) { return fmaf(a2, w2, fmaf(a0, w0, __fmul_rn(a1, w1))); };
            return make_float4(dot3(d0.x, d1.x, d2.x), dot3(d0.y, d1.y, d2.y), dot3(d0.z, d1.z, d2.z), dot3(d0.w, d1.w, d2.w));
          },
          false, nullptr, 0.f, [&](const float4& v, int q) { return mask4(v, G::template mask_nibble<1>(mb, 0, T, q, h)); }, bsum, n, act, dy,
          wave * 8 * 1024, lane, T);
      if constexpr (REGS) {
        if (nx) rgbx_bias_add(A, nx - 1, n, h, bsum);
        else C.db_rgbh = bsum;
      } else if constexpr (ATOM) {
        bias32_add(sp + SP_DB_RGBH + n, bsum, h);
      }
    }
    __syncthreads();
    // ---- rgb branch layers nx..1 (none for a depth-1 branch):  dpre_{x-1} = (dpre_x . W_x^T) * mask_{x-1}; dpre_0 lands where the
    //      depth-1 chain leaves it (LDS tile, dy_rgbh, db_rgbh), so everything below is the same for every depth.  64-row tiles only ----
    if constexpr (G::FULL) {
  #pragma unroll 1
      for (int x = A.nx; x >= 1; --x) {
        f32x16 acc1[G::RB][1];
        zero_acc<1>(acc1);
        {
          const float4* wx = wpk4 + ((A.pk.bwd_rgbxT + (x - 1) * RGB_W * RGB_W) / 4) + wave * 16 * 64;
          G::template k_loop<1, true>(acc1, act, 8, wx, lane, prefetch_quad<1>(wx, lane));
        }
        __builtin_amdgcn_sched_barrier(0);
        const size_t xt = x > 1 ? (size_t)(x - 2) * A.ntiles + tile : 0;
        const __amdgpu_buffer_rsrc_t dy =
            make_rsrc(x > 1 ? A.dy_rgbx + xt * FRAG_TILE_128 : A.dy_rgbh + (size_t)tile * FRAG_TILE_128, FRAG_TILE_128 * 4);
        __syncthreads();   // every wave has read dpre_x
        int le = tid;
        asm volatile("" : "+v"(le));   // epilogue-local lane constants
        const int lane = le & 63, j = lane & 31, h = lane >> 5;
        const int n = wave * 32 + j;
        const auto mb = G::template mask_load<1>(x > 1 ? A.bits_rgbx + (xt * 4 + wave) * 64 : A.bits_rgbh + ((size_t)tile * 4 + wave) * 64, lane);
        [[maybe_unused]] const float bsum = bwd_epilogue<G, DY>(
            [&](int q, int) { return G::template piece<1>(acc1, 0, q); }, false, nullptr, 0.f,
            [&](const float4& v, int q) { return mask4(v, G::template mask_nibble<1>(mb, 0, T, q, h)); }, 0.f, n, act, dy, wave * 8 * 1024, lane, T);
        if constexpr (REGS) {
          if (x > 1) rgbx_bias_add(A, x - 2, n, h, bsum);
          else C.db_rgbh += bsum;
        }
        __syncthreads();
      }
    }
    // ---- per-ray sums of dpre_rgbh (gradient of the per-ray condition columns of the rgb branch):
    //      thread (n, half) walks ROWS / 2 tile rows of feature n in LDS and flushes at ray boundaries ----
    {
      int t2 = tid;
      asm volatile("" : "+v"(t2));
      const int n = t2 & 127, hf = t2 >> 7;
      const int r0 = ROWS / 2 * hf;
      int ray = (row0 + r0) / A.S;
      int nextb = (ray + 1) * A.S - row0;   // first tile row of the next ray
      const int nvalid = A.rows - row0;      // tile rows >= nvalid are padding
      float ray_sum = 0.f;
  #pragma unroll 1
      for (int g = r0 / 4; g < r0 / 4 + ROWS / 8; ++g) {
        const float4 v4 = *reinterpret_cast<const float4*>(act + G::addr(n, g));
        const float v[4] = {v4.x, v4.y, v4.z, v4.w};
  #pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int pr = 4 * g + e;
          while (pr >= nextb) {
            if (ray < A.B && ray_sum != 0.f) atomicAdd(A.dray + (size_t)ray * RGB_W + n, ray_sum);
            ray_sum = 0.f; ++ray; nextb += A.S;
          }
          if (pr < nvalid) ray_sum += v[e];
        }
      }
      if (ray < A.B && ray_sum != 0.f) atomicAdd(A.dray + (size_t)ray * RGB_W + n, ray_sum);
    }
  }

  f32x16 acc[G::RB][2];
  // ---- d bottleneck = dpre_rgbh . W_rgbh[0:256]^T   (K=128 -> N=256), linear.  Density start: there is no d rgb, so d bn is the
  //      alpha head's term alone (use_alpha_condition: zero accumulators + ds (x) w_alpha[0:256]) or not formed at all ----
  zero_acc<2>(acc);
  if constexpr (!DENS) {
    const float4* w0 = wpk4 + (A.pk.bwd_rgbhT / 4) + wave * 32 * 64;
    G::template k_loop<2, true>(acc, act, 8, w0, lane, prefetch_quad<2>(w0, lane));
  }
  // the next GEMM's first weights: W_bn^T, or (density start, the head on the trunk) W_7^T
  WQuad<2> wnext = prefetch_quad<2>(wpk4 + ((DENS && !A.alpha_on_bn ? A.pk.bwd_LT[TRUNK_DEPTH - 1] : A.pk.bwd_bnT) / 4) + wave * 64 * 64, lane);
  __builtin_amdgcn_sched_barrier(0);
  if (!DENS || A.alpha_on_bn) {
    const __amdgpu_buffer_rsrc_t dy = make_rsrc(A.dy_bn + (size_t)tile * FRAG_TILE_256, FRAG_TILE_256 * 4);
    __syncthreads();
    int le = tid;
    asm volatile("" : "+v"(le));   // epilogue-local lane constants: not live across the K loops
    const int lane = le & 63, j = lane & 31, h = lane >> 5;
#pragma unroll
    for (int cb = 0; cb < 2; ++cb) {
      const int n = wave * 64 + 32 * cb + j;
      const float wab = A.alpha_on_bn ? prm[A.po.alpha_k + n] : 0.f;   // use_alpha_condition: the alpha head reads the bottleneck
      [[maybe_unused]] const float bsum = bwd_epilogue<G, DY>([&](int q, int) { return G::template piece<2>(acc, cb, q); }, A.alpha_on_bn, dr + 3 * ROWS, wab,
                                         no_mask, 0.f, n, act, dy, wv + cb * 8 * 1024, lane, T);
      if constexpr (REGS) C.db_bn[cb] += bsum;
      else if constexpr (ATOM) bias32_add(sp + SP_DB_BN + n, bsum, h);
    }
    __syncthreads();
  }

  // ---- d h8 = dbn . W_bn^T + d sigma_raw (x) w_alpha ; mask h8 > 0 -> dpre_7 ----
  // ---- then l = 7..1:  d h_l = dpre_l . W_l[0:256]^T ; mask h_l > 0 -> dpre_{l-1} ----
#pragma unroll 1
  for (int l = TRUNK_DEPTH; l >= 1; --l) {
    // the output of this step is dpre_{l-1}; its mask is sign(pre_{l-1}) = bits_trunk[l-1]
    const auto mb = G::template mask_load<2>(A.bits_trunk + (((size_t)(l - 1) * A.ntiles + tile) * 4 + wave) * 128, lane);
    zero_acc<2>(acc);
    const int woff = (l == TRUNK_DEPTH) ? A.pk.bwd_bnT : A.pk.bwd_LT[l];
    // density start, the head on the trunk: the l = 8 step is the head's own term, ds (x) w_alpha on zero accumulators -- nothing to multiply
    if (!DENS || l < TRUNK_DEPTH || A.alpha_on_bn)
      G::template k_loop<2, true>(acc, act, 16, wpk4 + (woff / 4) + wave * 64 * 64, lane, wnext);
    wnext = prefetch_quad<2>(wpk4 + (A.pk.bwd_LT[l > 1 ? l - 1 : 1] / 4) + wave * 64 * 64, lane);
    __builtin_amdgcn_sched_barrier(0);
    const __amdgpu_buffer_rsrc_t dy =
        make_rsrc(A.dy_trunk + (size_t)(l - 1) * layer_fl + (size_t)tile * FRAG_TILE_256, FRAG_TILE_256 * 4);
    __syncthreads();
    int le = tid;
    asm volatile("" : "+v"(le));   // epilogue-local lane constants: not live across the K loop
    const int lane = le & 63, j = lane & 31, h = lane >> 5;
    float bs[2];
#pragma unroll
    for (int cb = 0; cb < 2; ++cb) {
      const int n = wave * 64 + 32 * cb + j;
      const float wa = (l == TRUNK_DEPTH && !A.alpha_on_bn) ? prm[A.po.alpha_k + n] : 0.f;
      bs[cb] = bwd_epilogue<G, DY>([&](int q, int) { return G::template piece<2>(acc, cb, q); }, l == TRUNK_DEPTH, dr + 3 * ROWS, wa,
                               [&](const float4& v, int q) { return mask4(v, G::template mask_nibble<2>(mb, cb, T, q, h)); }, 0.f, n, act, dy,
                               wv + cb * 8 * 1024, lane, T);
      if constexpr (ATOM) bias32_add(sp + SP_DB_TRUNK + (l - 1) * TRUNK_W + n, bs[cb], h);
    }
    if constexpr (REGS) {
      // runtime layer index -> static register: add into the matching accumulator
#pragma unroll
      for (int q = 0; q < TRUNK_DEPTH; ++q)
        if (q == l - 1) { C.db_trunk[q][0] += bs[0]; C.db_trunk[q][1] += bs[1]; }
    }
    __syncthreads();

    // ---- warp on: d posenc = dpre_4 . W4[256:]^T + dpre_0 . W0^T  (256 -> PK columns).  Wave w owns
    //      MFMA row block w&1 (tile rows 2i + rb) x column block w>>1; the result goes to the dpe tile
    //      in LDS (aliases dr, dead since the l = 8 step), element (n, row) at n*64 + (row ^ (n & 31)).  64-row tiles only ----
    if constexpr (G::FULL) {
      if (A.d_points && (l - 1 == A.skip || l == 1)) {
        float* dpe = dr;
        const bool first = (l - 1 == A.skip);
        int ln = lane;
        asm volatile("" : "+v"(ln));   // opaque: the per-lane constants of this section are recomputed here, not hoisted out of
                                       // the tile loop into registers that live (= spill) across the trunk layers
        const float4* wq = wpk4 + ((first ? A.pk.bwd_L4bT : A.pk.bwd_L0T) / 4) + ln;
        const int rb = wave & 1, cb = wave >> 1;
        f32x16 a2;
#pragma unroll
        for (int r = 0; r < 16; ++r) a2[r] = 0.f;
        const int j = ln & 31, h = ln >> 5;
        const int i = j, kk = h;
        const int aoff = 2 * (i & 1) + rb;
        const int PKS = (A.PK + 31) / 32 * 32;
        const int npw = PKS / 32 * 2;   // pieces per wave: 2 or 4
        // B from L2 in batches of 4 float4, the next batch in flight under the current one's MFMAs
        auto load_b = [&](float4 (&b)[4], int bt) {
#pragma unroll
          for (int u = 0; u < 4; ++u) b[u] = wq[(bt * 4 + u) * 64];
        };
        auto mma_b = [&](const float4 (&b)[4], int bt) {
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const int k0 = 4 * (bt * 4 + u) + kk;
            const float a0 = act[act_addr(k0, i >> 1) + aoff];
            const float a1 = act[act_addr(k0 + 2, i >> 1) + aoff];
            a2 = mfma32(a0, cb ? b[u].y : b[u].x, a2);
            a2 = mfma32(a1, cb ? b[u].w : b[u].z, a2);
          }
        };
        float4 b0[4], b1[4];
        load_b(b0, 0);
#pragma unroll 1
        for (int bt = 0; bt < 16; bt += 2) {
          load_b(b1, bt + 1);
          mma_b(b0, bt);
          if (bt + 2 < 16) load_b(b0, bt + 2);
          mma_b(b1, bt + 1);
        }
        const int n = 32 * cb + j;
        if (n < A.PK) {
#pragma unroll
          for (int reg = 0; reg < 16; ++reg) {
            const int row = 2 * c_row(reg, h) + rb;
            float* o = dpe + n * TILE_ROWS + (row ^ (n & 31));
            *o = first ? a2[reg] : *o + a2[reg];
          }
        }
        __syncthreads();
        if (!first) {
          // chain rule through SinusoidalEncoder: d sin(f x) = f cos(f x), d sin(f x + pi/2) = -f sin(f x),
          // with sin / cos taken from the forward posenc stash.  Every thread holds 4 rows of one feature per piece:
          // feature k's term  -+ 2^f * pe[k] * dpe[partner(k)]  goes to the contrib tile (act is dead), element (k, row)
          // at k*64 + (row ^ (k & 31)); 192 threads then sum their (row, c) over the 2F features in a fixed order.
          float* contrib = act;
          const int nfeat = 3 + 6 * A.F;
          float4 pv[4];
          {
            const float4* pe4 = reinterpret_cast<const float4*>(A.st_pe + (size_t)tile * PKS * TILE_ROWS) + ln;
#pragma unroll
            for (int u = 0; u < 4; ++u)
              if (u < npw) pv[u] = pe4[(wave + 4 * u) * 64];
          }
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            if (u < npw) {
              const int pid = wave + 4 * u, q = pid & 7;
              const int k = (pid >> 3) * 32 + j, g = (q & 1) + 2 * h + 4 * (q >> 1);
              if (k >= 3 && k < nfeat) {
                const int f = (k - 3) / 6, r = (k - 3) - 6 * f;
                const int partner = r < 3 ? k + 3 : k - 3;
                const float sgn = r < 3 ? -(float)(1 << f) : (float)(1 << f);
                const float* dp = dpe + partner * TILE_ROWS;
                float* co = contrib + k * TILE_ROWS;
                const float pvv[4] = {pv[u].x, pv[u].y, pv[u].z, pv[u].w};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                  const int row = 4 * g + e;
                  co[row ^ (k & 31)] = sgn * pvv[e] * dp[row ^ (partner & 31)];
                }
              }
            }
          }
          __syncthreads();
          if (tid < 3 * TILE_ROWS) {
            const int row = tid / 3, c = tid - 3 * row;
            float dx = dpe[c * TILE_ROWS + (row ^ c)];
            for (int f = 0; f < A.F; ++f) {
              const int ns = 3 + 6 * f + c, nc = ns + 3;
              dx += contrib[ns * TILE_ROWS + (row ^ (ns & 31))] + contrib[nc * TILE_ROWS + (row ^ (nc & 31))];
            }
            A.d_points[(size_t)tile * TILE_ROWS * 3 + tid] = dx;
          }
        }
        if (!first) __syncthreads();   // dr (aliased) is rewritten by the next tile
      }
    }
  }
}

// ONE launch for the coarse and the fine MLP (the two backward passes are independent: no gradient flows from the fine
// pass into the coarse MLP): global tiles [0, nt0) are level 0, [nt0, ntot) level 1, dealt round-robin, so a
// workgroup runs its 2 coarse tiles and goes straight on with its 6 fine ones (config A) instead of ramping up and draining
// twice.  The level's arguments are indexed in the kernarg segment (scalar loads, one copy of the tile code).
struct ChainBwdArgs2 { ChainBwdArgs a[2]; int nt0, ntot; };

}  // namespace nrf
