// The one placement rule of the mesh entries (mesh.hip, mesh_components.hip, mesh_raster.hip).  A workgroup of MESH_THREADS threads
// owns BLOCK consecutive elements as ROUNDS rounds of MESH_THREADS, and every output slot is a rank:
//     scanned workgroup total  +  the totals of the (round, wave) pairs before this wave  +  the popcount of the wave's ballot below this lane.
// No atomic, no flag another workgroup waits on: a counting kernel stores per-workgroup totals (vote, block_total), a one-workgroup
// kernel scans them (mesh_scan.h), the emitting kernels vote again and read the scan (walk).  The kernels keep what is theirs: what is
// voted on, and what is written at the slot.
#pragma once

#include "mesh_scan.h"

namespace nrf {

constexpr int MESH_THREADS = 256;   // of every mesh kernel but the scans
constexpr int MESH_WAVES = MESH_THREADS / 64;

__device__ __forceinline__ unsigned long long lanes_below() { return (1ull << (threadIdx.x & 63)) - 1ull; }

template <int ROUNDS>
struct MeshRank {
  static constexpr int BLOCK = MESH_THREADS * ROUNDS;   // elements of one workgroup
  static constexpr int SLOTS = ROUNDS * MESH_WAVES;     // its (round, wave) pairs, in element order: the ints of LDS a kernel declares

  // the element this thread owns in round r; 64-bit, since the last workgroup's may pass 2^31
  static __device__ __forceinline__ long long owned(const int r) { return (long long)blockIdx.x * BLOCK + r * MESH_THREADS + threadIdx.x; }

  // The wave's vote of round r on the low BITS bits of `flags`: the set bits before this lane's own, counted in lane order, then bit
  // order; lane 0 stores the wave's total.  Uniform over the workgroup; a __syncthreads() separates it from block_total and walk.
  template <int BITS = 1>
  static __device__ __forceinline__ int vote(int* __restrict__ s, const int r, const unsigned flags) {
    int rank = 0, total = 0;
#pragma unroll
    for (int b = 0; b < BITS; ++b) {
      const unsigned long long ballot = __ballot(((flags >> b) & 1u) != 0u);
      rank += __popcll(ballot & lanes_below());
      total += __popcll(ballot);
    }
    if ((threadIdx.x & 63) == 0) s[r * MESH_WAVES + (threadIdx.x >> 6)] = total;
    return rank;
  }

  static __device__ __forceinline__ int block_total(const int* __restrict__ s) {
    int total = 0;
#pragma unroll
    for (int e = 0; e < SLOTS; ++e) total += s[e];
    return total;
  }

  // fn(r, before) once per round, `before` = first + the totals of the (round, wave) pairs before this wave's: uniform over the wave
  template <class Fn>
  static __device__ __forceinline__ void walk(const int* __restrict__ s, int before, Fn&& fn) {
    const int wave = threadIdx.x >> 6;
#pragma unroll
    for (int r = 0; r < ROUNDS; ++r) {
#pragma unroll
      for (int w = 0; w < MESH_WAVES; ++w) {
        if (w == wave) fn(r, before);
        before += s[r * MESH_WAVES + w];
      }
    }
  }
};

}  // namespace nrf
