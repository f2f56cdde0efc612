// Mesh rasteriser on the device (nrf_mesh_raster_draw / _interpolate / _visibility; the definition is whole in include/nerfies_amd.h
// and restated in NumPy in tests/mesh_raster_reference.py): which triangle every pixel of one camera sees, its depth and its
// perspective-correct barycentrics.  Handle-free: any (V,3) screen array, any triangles, in any order.
//
// Coverage is integer arithmetic on coordinates snapped to 1/256 pixel; depth and barycentrics are float32 with one rounding per
// operation in the order the header gives (the file is compiled with contraction off, as mesh.hip is).  A pixel's owner is the minimum
// of the 64-bit keys (depth bits << 32 | face index) of the triangles that cover it, taken with an integer atomicMin on a uint64 in
// ordinary device memory: a minimum does not depend on the order its operands arrive in, so the image has the same bits on every run
// and for every order of the triangles.  The resolve pass recomputes the owner's depth and barycentrics with the device function the
// draw pass used (raster_shade).
//
// No thread waits on another.  A triangle whose pixel box has more than RASTER_SMALL pixels is not drawn by its thread: it is ranked
// within its workgroup (the rule of mesh_rank.h, one round) into the workgroup's Faces::BLOCK slots of a list, the workgroups' totals
// are scanned, and a fixed grid of workgroups strides over the ranks 0 .. total-1, finding each rank's workgroup by bisection of the
// scan.  Every loop is bounded by a clamped pixel box, by F, or by log2 of the number of workgroups.  The host half is built from
// mesh_host.h.
#include "mesh_host.h"
#include "mesh_rank.h"

#include <cmath>

#pragma clang fp contract(off)

using namespace nrf;
using namespace nrf::api;

namespace {

using Faces = MeshRank<1>;                   // one triangle per thread of the faces kernel
constexpr int RASTER_SMALL = 256;            // pixels of a pixel box a single thread still draws
constexpr int RASTER_LARGE_BLOCKS = 1024;    // at most this many workgroups stride over the list of large triangles
constexpr unsigned long long KEY_EMPTY = ~0ull;

// byte offsets of the workspace
struct RasterPlan {
  size_t keys, block_large, list, total;
  int nbt;
};

RasterPlan raster_plan(int F, int W, int H) {
  RasterPlan p;
  MeshCarve c;
  p.nbt = (int)blocks_of(F, Faces::BLOCK);
  p.keys = c.take(sizeof(unsigned long long) * (size_t)W * (size_t)H);
  p.block_large = c.take(sizeof(int) * (size_t)p.nbt);
  p.list = c.take(sizeof(int) * (size_t)p.nbt * Faces::BLOCK);
  p.total = c.total;
  return p;
}

// A triangle that passed every skip rule: snapped corners, their z, s and s A > 0, and the clamped pixel box.
struct RasterTri {
  long long X[3], Y[3];
  float z[3];
  long long area;   // s A
  long long s;
  int i0, i1, j0, j1;
};

__device__ __forceinline__ bool raster_setup(const float* __restrict__ screen, const int V, const int* __restrict__ triangles,
                                             const long long t, const int W, const int H, const float near, RasterTri& T) {
  long long lo_x = 0, hi_x = 0, lo_y = 0, hi_y = 0;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int v = triangles[3 * (size_t)t + k];
    if (v < 0 || v >= V) return false;
    const float px = screen[3 * (size_t)v + 0], py = screen[3 * (size_t)v + 1], z = screen[3 * (size_t)v + 2];
    if (!(z > near && fabsf(px) <= 1048576.0f && fabsf(py) <= 1048576.0f)) return false;   // false for NaN
    T.X[k] = (long long)rintf(px * 256.0f);
    T.Y[k] = (long long)rintf(py * 256.0f);
    T.z[k] = z;
    lo_x = k == 0 || T.X[k] < lo_x ? T.X[k] : lo_x;
    hi_x = k == 0 || T.X[k] > hi_x ? T.X[k] : hi_x;
    lo_y = k == 0 || T.Y[k] < lo_y ? T.Y[k] : lo_y;
    hi_y = k == 0 || T.Y[k] > hi_y ? T.Y[k] : hi_y;
  }
  const long long A = (T.X[1] - T.X[0]) * (T.Y[2] - T.Y[0]) - (T.Y[1] - T.Y[0]) * (T.X[2] - T.X[0]);
  if (A == 0) return false;
  T.s = A > 0 ? 1 : -1;
  T.area = T.s * A;
  // pixels whose centre 256 i + 128 lies in [lo, hi]; >> 8 on a signed value is the floor of the division by 256
  const long long i0 = (lo_x - 128 + 255) >> 8, i1 = (hi_x - 128) >> 8, j0 = (lo_y - 128 + 255) >> 8, j1 = (hi_y - 128) >> 8;
  T.i0 = (int)(i0 > 0 ? i0 : 0);
  T.i1 = (int)(i1 < W - 1 ? i1 : W - 1);
  T.j0 = (int)(j0 > 0 ? j0 : 0);
  T.j1 = (int)(j1 < H - 1 ? j1 : H - 1);
  return T.i0 <= T.i1 && T.j0 <= T.j1;
}

// Coverage of pixel (i, j) inside T's pixel box, and where covered its depth and barycentrics: the header's formulas, in their order.
__device__ __forceinline__ bool raster_shade(const RasterTri& T, const int i, const int j, float& depth, float* b) {
  const long long Px = 256ll * i + 128, Py = 256ll * j + 128;
  float q[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int va = (k + 1) % 3, vb = (k + 2) % 3;
    const long long dx = T.s * (T.X[vb] - T.X[va]), dy = T.s * (T.Y[vb] - T.Y[va]);
    const long long E = dx * (Py - T.Y[va]) - dy * (Px - T.X[va]);
    const bool top_left = dy < 0 || (dy == 0 && dx > 0);
    if (!(E > 0 || (E == 0 && top_left))) return false;
    const float l = (float)E / (float)T.area;
    q[k] = l / T.z[k];
  }
  const float w = (q[0] + q[1]) + q[2];
  depth = 1.0f / w;
  b[0] = q[0] / w;
  b[1] = q[1] / w;
  b[2] = q[2] / w;
  return true;
}

// the pixel's key against the triangle's: a stale read can only be too large, and then the atomic decides
__device__ __forceinline__ void raster_offer(unsigned long long* __restrict__ keys, const size_t pixel, const float depth, const unsigned face) {
  const unsigned long long key = ((unsigned long long)__float_as_uint(depth) << 32) | face;
  if (key < __hip_atomic_load(keys + pixel, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(keys + pixel, key);
}

__global__ __launch_bounds__(MESH_THREADS) void raster_clear_kernel(unsigned long long* __restrict__ keys, const long long pixels,
                                                                    int* __restrict__ status) {
  const long long p = (long long)blockIdx.x * MESH_THREADS + threadIdx.x;
  if (p < pixels) keys[p] = KEY_EMPTY;
  if (p < 4) status[p] = 0;
}

// One thread per triangle: small ones are drawn here, large ones are ranked into list[blockIdx.x * Faces::BLOCK ..].
__global__ __launch_bounds__(MESH_THREADS) void raster_faces_kernel(const float* __restrict__ screen, const int V,
                                                                    const int* __restrict__ triangles, const int F, const int W, const int H,
                                                                    const float near, unsigned long long* __restrict__ keys,
                                                                    int* __restrict__ block_large, int* __restrict__ list,
                                                                    int* __restrict__ status) {
  __shared__ int wave_large[Faces::SLOTS];
  const long long t = Faces::owned(0);
  RasterTri T;
  const bool drawn = t < F && raster_setup(screen, V, triangles, t, W, H, near, T);
  bool large = false;
  if (drawn) {
    const int bw = T.i1 - T.i0 + 1, bh = T.j1 - T.j0 + 1;
    large = (long long)bw * bh > RASTER_SMALL;
    if (!large) {
      for (int j = T.j0; j <= T.j1; ++j) {
        for (int i = T.i0; i <= T.i1; ++i) {
          float depth, b[3];
          if (raster_shade(T, i, j, depth, b)) raster_offer(keys, (size_t)j * W + i, depth, (unsigned)t);
        }
      }
    }
  }
  const unsigned long long bd = __ballot(drawn);
  if ((threadIdx.x & 63) == 0 && bd != 0ull) atomicAdd(status + 0, __popcll(bd));   // a count, not a rank: an integer add per wave
  const int rank = Faces::vote(wave_large, 0, large);
  __syncthreads();
  Faces::walk(wave_large, 0, [&](const int, const int before) {
    if (large) list[(size_t)blockIdx.x * Faces::BLOCK + before + rank] = (int)t;
  });
  if (threadIdx.x == 0) block_large[blockIdx.x] = Faces::block_total(wave_large);
}

__global__ __launch_bounds__(SCAN_THREADS) void raster_scan_kernel(int* __restrict__ block_large, const int nblocks, int* __restrict__ status) {
  int total, unused;
  mesh_scan_totals(block_large, nblocks, nullptr, 0, total, unused);
  if (threadIdx.x == SCAN_THREADS - 1) status[1] = total;
}

// Rank r of the large triangles belongs to the faces workgroup g with block_large[g] <= r < block_large[g + 1] (the scan is
// exclusive); one workgroup draws it, its threads striding over the pixel box.
__global__ __launch_bounds__(MESH_THREADS) void raster_large_kernel(const float* __restrict__ screen, const int V,
                                                                    const int* __restrict__ triangles, const int F, const int W, const int H,
                                                                    const float near, unsigned long long* __restrict__ keys,
                                                                    const int* __restrict__ block_large, const int nblocks,
                                                                    const int* __restrict__ list, const int* __restrict__ status) {
  int total = status[1];
  total = total < F ? total : F;
  for (int r = blockIdx.x; r < total; r += gridDim.x) {   // uniform over the workgroup
    int lo = 0, hi = nblocks - 1;   // the last g with block_large[g] <= r
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (block_large[mid] <= r) lo = mid; else hi = mid - 1;
    }
    const int local = r - block_large[lo];
    if (local < 0 || local >= Faces::BLOCK) continue;
    const int t = list[(size_t)lo * Faces::BLOCK + local];
    if (t < 0 || t >= F) continue;
    RasterTri T;
    if (!raster_setup(screen, V, triangles, t, W, H, near, T)) continue;
    const int bw = T.i1 - T.i0 + 1;
    const long long n = (long long)bw * (T.j1 - T.j0 + 1);
    for (long long p = threadIdx.x; p < n; p += MESH_THREADS) {
      const int row = (int)(p / bw);
      const int i = T.i0 + (int)(p - (long long)row * bw), j = T.j0 + row;
      float depth, b[3];
      if (raster_shade(T, i, j, depth, b)) raster_offer(keys, (size_t)j * W + i, depth, (unsigned)t);
    }
  }
}

__global__ __launch_bounds__(MESH_THREADS) void raster_resolve_kernel(const float* __restrict__ screen, const int V,
                                                                      const int* __restrict__ triangles, const int F, const int W, const int H,
                                                                      const float near, const unsigned long long* __restrict__ keys,
                                                                      int* __restrict__ face_id, float* __restrict__ depth_out,
                                                                      float* __restrict__ bary, int* __restrict__ status) {
  const long long pixels = (long long)W * H;
  const long long p = (long long)blockIdx.x * MESH_THREADS + threadIdx.x;
  bool covered = false;
  if (p < pixels) {
    const unsigned long long key = keys[p];
    int face = -1;
    float depth = 0.0f, b[3] = {0.0f, 0.0f, 0.0f};
    const unsigned t = (unsigned)(key & 0xffffffffull);
    if (key != KEY_EMPTY && t < (unsigned)F) {
      const int j = (int)(p / W), i = (int)(p - (long long)j * W);
      RasterTri T;
      if (raster_setup(screen, V, triangles, t, W, H, near, T) && i >= T.i0 && i <= T.i1 && j >= T.j0 && j <= T.j1 &&
          raster_shade(T, i, j, depth, b)) {
        face = (int)t;
        covered = true;
      } else {   // cannot happen for a key the draw passes wrote
        depth = 0.0f;
        b[0] = b[1] = b[2] = 0.0f;
      }
    }
    face_id[p] = face;
    depth_out[p] = depth;
    if (bary) {
      bary[3 * (size_t)p + 0] = b[0];
      bary[3 * (size_t)p + 1] = b[1];
      bary[3 * (size_t)p + 2] = b[2];
    }
  }
  const unsigned long long bc = __ballot(covered);
  if ((threadIdx.x & 63) == 0 && bc != 0ull) atomicAdd(status + 2, __popcll(bc));
}

// one thread per output element
__global__ __launch_bounds__(MESH_THREADS) void raster_interpolate_kernel(const int* __restrict__ face_id, const float* __restrict__ bary,
                                                                          const long long elements, const int* __restrict__ triangles,
                                                                          const int F, const float* __restrict__ attributes, const int V,
                                                                          const int A, const float* __restrict__ background,
                                                                          float* __restrict__ out) {
  const long long e = (long long)blockIdx.x * MESH_THREADS + threadIdx.x;
  if (e >= elements) return;
  const long long p = e / A;
  const int c = (int)(e - p * A);
  float r = background ? background[c] : 0.0f;
  const int f = face_id[p];
  if (f >= 0 && f < F) {
    const int v0 = triangles[3 * (size_t)f + 0], v1 = triangles[3 * (size_t)f + 1], v2 = triangles[3 * (size_t)f + 2];
    if (v0 >= 0 && v0 < V && v1 >= 0 && v1 < V && v2 >= 0 && v2 < V) {
      const float b0 = bary[3 * (size_t)p + 0], b1 = bary[3 * (size_t)p + 1], b2 = bary[3 * (size_t)p + 2];
      r = (b0 * attributes[(size_t)v0 * A + c] + b1 * attributes[(size_t)v1 * A + c]) + b2 * attributes[(size_t)v2 * A + c];
    }
  }
  out[e] = r;
}

__global__ __launch_bounds__(MESH_THREADS) void raster_visibility_clear_kernel(unsigned char* __restrict__ visible, const int V) {
  const long long v = (long long)blockIdx.x * MESH_THREADS + threadIdx.x;
  if (v < V) visible[v] = 0;
}

// every store writes the same byte value: the order plays no part
__global__ __launch_bounds__(MESH_THREADS) void raster_visibility_kernel(const int* __restrict__ face_id, const long long pixels,
                                                                         const int* __restrict__ triangles, const int F, const int V,
                                                                         unsigned char* __restrict__ visible) {
  const long long p = (long long)blockIdx.x * MESH_THREADS + threadIdx.x;
  if (p >= pixels) return;
  const int f = face_id[p];
  if (f < 0 || f >= F) return;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int v = triangles[3 * (size_t)f + k];
    if (v >= 0 && v < V) visible[v] = 1;
  }
}

int rs_image(const char* entry, int32_t num_triangles, int32_t width, int32_t height) {
  if (num_triangles < 0) return mesh_shape(entry, "num_triangles must not be negative");
  if (width < 1) return mesh_shape(entry, "width must be at least 1");
  if (height < 1) return mesh_shape(entry, "height must be at least 1");
  if ((long long)width * height > (long long)NRF_MESH_RASTER_MAX_PIXELS)
    return mesh_shape(entry, "width * height is more than NRF_MESH_RASTER_MAX_PIXELS");
  return NRF_OK;
}

// the pixels and the mesh interpolate and visibility are handed
int rs_pixels_mesh(const char* entry, const int32_t* face_id, int64_t num_pixels, const int32_t* triangles, int32_t num_triangles,
                   int32_t num_vertices) {
  if (num_pixels < 0) return mesh_shape(entry, "num_pixels must not be negative");
  if (num_triangles < 0) return mesh_shape(entry, "num_triangles must not be negative");
  if (num_vertices < 0) return mesh_shape(entry, "num_vertices must not be negative");
  if (num_pixels > 0 && !face_id) return mesh_null(entry, "face_id");
  if (num_triangles > 0 && !triangles) return mesh_null(entry, "triangles");
  return NRF_OK;
}

}  // namespace

extern "C" {

int nrf_mesh_raster_workspace_bytes(int32_t num_triangles, int32_t width, int32_t height, size_t* bytes) {
  const char* entry = "nrf_mesh_raster_workspace_bytes";
  CK(rs_image(entry, num_triangles, width, height));
  if (!bytes) return mesh_null(entry, "bytes");
  *bytes = raster_plan(num_triangles, width, height).total;
  return NRF_OK;
}

int nrf_mesh_raster_draw(const float* screen, int32_t num_vertices, const int32_t* triangles, int32_t num_triangles, int32_t width,
                         int32_t height, float near, int32_t* face_id, float* depth, float* bary, void* workspace,
                         size_t workspace_bytes, void* stream) {
  const char* entry = "nrf_mesh_raster_draw";
  if (num_vertices < 0) return mesh_shape(entry, "num_vertices must not be negative");
  CK(rs_image(entry, num_triangles, width, height));
  if (!(near >= 0.0f) || !std::isfinite(near)) return mesh_shape(entry, "near must be finite and not negative");
  if (num_vertices > 0 && !screen) return mesh_null(entry, "screen");
  if (num_triangles > 0 && !triangles) return mesh_null(entry, "triangles");
  if (!face_id) return mesh_null(entry, "face_id");
  if (!depth) return mesh_null(entry, "depth");
  const int V = num_vertices, F = num_triangles, W = width, H = height;
  const RasterPlan p = raster_plan(F, W, H);
  CK(mesh_workspace(entry, "nrf_mesh_raster_workspace_bytes", NRF_E_WORKSPACE, p.total, workspace, workspace_bytes));
  char* ws = (char*)workspace;
  int* status = (int*)ws;
  unsigned long long* keys = (unsigned long long*)(ws + p.keys);
  int* block_large = (int*)(ws + p.block_large);
  int* list = (int*)(ws + p.list);
  const long long pixels = (long long)W * H;
  const long long pblocks = blocks_of(pixels, MESH_THREADS);
  MESH_LAUNCH(raster_clear_kernel, pblocks, MESH_THREADS, keys, pixels, status);
  if (F > 0) {
    MESH_LAUNCH(raster_faces_kernel, p.nbt, MESH_THREADS, screen, V, triangles, F, W, H, near, keys, block_large, list, status);
    MESH_LAUNCH(raster_scan_kernel, 1, SCAN_THREADS, block_large, p.nbt, status);
    MESH_LAUNCH(raster_large_kernel, F < RASTER_LARGE_BLOCKS ? F : RASTER_LARGE_BLOCKS, MESH_THREADS, screen, V, triangles, F, W, H, near, keys,
              (const int*)block_large, p.nbt, (const int*)list, (const int*)status);
  }
  MESH_LAUNCH(raster_resolve_kernel, pblocks, MESH_THREADS, screen, V, triangles, F, W, H, near, (const unsigned long long*)keys, face_id, depth,
            bary, status);
  return check_launch(entry);
}

int nrf_mesh_raster_interpolate(const int32_t* face_id, const float* bary, int64_t num_pixels, const int32_t* triangles,
                                int32_t num_triangles, const float* attributes, int32_t num_vertices, int32_t width_a,
                                const float* background, float* out, void* stream) {
  const char* entry = "nrf_mesh_raster_interpolate";
  CK(rs_pixels_mesh(entry, face_id, num_pixels, triangles, num_triangles, num_vertices));
  if (width_a < 1) return mesh_shape(entry, "width_a must be at least 1");
  if (num_pixels > 0x7fffffffll * MESH_THREADS / width_a)
    return mesh_shape(entry, "num_pixels * width_a is more than 2^31 - 1 workgroups of 256 elements");
  if (num_pixels > 0 && !bary) return mesh_null(entry, "bary");
  if (num_vertices > 0 && !attributes) return mesh_null(entry, "attributes");
  if (num_pixels > 0 && !out) return mesh_null(entry, "out");
  if (num_pixels == 0) return NRF_OK;
  const long long elements = (long long)num_pixels * width_a;
  MESH_LAUNCH(raster_interpolate_kernel, blocks_of(elements, MESH_THREADS), MESH_THREADS, face_id, bary, elements, triangles, num_triangles,
            attributes, num_vertices, width_a, background, out);
  return check_launch(entry);
}

int nrf_mesh_raster_visibility(const int32_t* face_id, int64_t num_pixels, const int32_t* triangles, int32_t num_triangles,
                               int32_t num_vertices, uint8_t* visible, void* stream) {
  const char* entry = "nrf_mesh_raster_visibility";
  CK(rs_pixels_mesh(entry, face_id, num_pixels, triangles, num_triangles, num_vertices));
  if (num_pixels > 0x7fffffffll * MESH_THREADS) return mesh_shape(entry, "num_pixels is more than 2^31 - 1 workgroups of 256 pixels");
  if (num_vertices > 0 && !visible) return mesh_null(entry, "visible");
  if (num_vertices == 0) return NRF_OK;
  MESH_LAUNCH(raster_visibility_clear_kernel, blocks_of(num_vertices, MESH_THREADS), MESH_THREADS, visible, num_vertices);
  if (num_pixels > 0 && num_triangles > 0)
    MESH_LAUNCH(raster_visibility_kernel, blocks_of(num_pixels, MESH_THREADS), MESH_THREADS, face_id, (long long)num_pixels, triangles,
              num_triangles, num_vertices, visible);
  return check_launch(entry);
}

}  // extern "C"
