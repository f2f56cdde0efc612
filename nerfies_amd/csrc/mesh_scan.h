// The scan of the mesh entries' placement rule (mesh_rank.h; mesh.hip, mesh_components.hip, mesh_raster.hip): exclusive scans of two
// arrays of per-workgroup totals, in place, by ONE workgroup of SCAN_THREADS threads, each thread a contiguous run.  No workgroup ever
// waits on another's flag, so nothing can stall: the kernels before it store the totals, the kernels after it read the scan.  Each
// entry wraps it in a kernel of its own that writes that entry's status words.
#pragma once

#include <hip/hip_runtime.h>

namespace nrf {

constexpr int SCAN_THREADS = 1024;

// a[0 .. na) and b[0 .. nb) become their exclusive prefix sums; every thread returns with the two totals.  `b` may be null with nb = 0.
__device__ __forceinline__ void mesh_scan_totals(int* __restrict__ a, const int na, int* __restrict__ b, const int nb, int& total_a,
                                                 int& total_b) {
  __shared__ int ta[SCAN_THREADS], tb[SCAN_THREADS];
  const int t = threadIdx.x;
  const int pa = (na + SCAN_THREADS - 1) / SCAN_THREADS, pb = (nb + SCAN_THREADS - 1) / SCAN_THREADS;
  const long long fa = (long long)t * pa, fb = (long long)t * pb;
  const int a0 = fa < na ? (int)fa : na, b0 = fb < nb ? (int)fb : nb;
  const int a1 = a0 + pa < na ? a0 + pa : na, b1 = b0 + pb < nb ? b0 + pb : nb;
  int ma = 0, mb = 0;
  for (int i = a0; i < a1; ++i) ma += a[i];
  for (int i = b0; i < b1; ++i) mb += b[i];
  ta[t] = ma;
  tb[t] = mb;
  __syncthreads();
  for (int off = 1; off < SCAN_THREADS; off <<= 1) {
    const int xa = t >= off ? ta[t - off] : 0, xb = t >= off ? tb[t - off] : 0;
    __syncthreads();
    ta[t] += xa;
    tb[t] += xb;
    __syncthreads();
  }
  int ra = ta[t] - ma, rb = tb[t] - mb;
  for (int i = a0; i < a1; ++i) {
    const int v = a[i];
    a[i] = ra;
    ra += v;
  }
  for (int i = b0; i < b1; ++i) {
    const int v = b[i];
    b[i] = rb;
    rb += v;
  }
  total_a = ta[SCAN_THREADS - 1];
  total_b = tb[SCAN_THREADS - 1];
}

}  // namespace nrf
