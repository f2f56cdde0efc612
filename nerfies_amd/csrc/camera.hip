// Camera geometry on the GPU: pixel -> world ray (with the 10-step Newton undistort), world point -> pixel.
//
// Reference behaviour: nerfies/camera.py:225-269 (pixel_to_local_rays, pixels_to_rays), :26-105 (undistort),
// :283-315 (project), :317-321 (get_pixel_centers), nerfies/datasets/core.py:50-75 (camera_to_rays).
// One thread per pixel; every output is an HBM-bound stream (12 B in / 32 B out per pixel), so the [n,3]
// outputs are transposed through LDS and written as one contiguous run per workgroup.
//
// Camera table (nrf_camera_table_*): the same per-ray arithmetic with the camera read from a device-resident
// (C, NRF_CAMERA_ROW) table by a per-ray index, and the reverse passes into the table.  A reverse pass is two launches: one thread
// per ray forms the 22 partials, a workgroup whose rays share a camera reduces them to one record, any other workgroup leaves one
// record per ray; then one workgroup per camera sums its records in a fixed order (no float atomics: repeatable bit for bit).
#include <hip/hip_runtime.h>

#include "nrf_internal.h"
#include "se3_math.h"

namespace nrf {
namespace {

constexpr int CAM_THREADS = 256;

// Newton on (fx, fy) = distort(x, y) - (xd, yd); the update is skipped where |det J| <= 1e-9 and the iteration
// count is fixed at 10 (camera.py:76-105) so the result does not depend on a convergence test.
__device__ __forceinline__ void undistort(const CameraArgs& c, float xd, float yd, float& xo, float& yo) {
  float x = xd, y = yd;
#pragma unroll 1
  for (int it = 0; it < 10; ++it) {
    const float r = x * x + y * y;
    const float d = 1.0f + r * (c.k1 + r * (c.k2 + c.k3 * r));
    const float fx = d * x + 2.0f * c.p1 * x * y + c.p2 * (r + 2.0f * x * x) - xd;
    const float fy = d * y + 2.0f * c.p2 * x * y + c.p1 * (r + 2.0f * y * y) - yd;
    const float d_r = c.k1 + r * (2.0f * c.k2 + 3.0f * c.k3 * r);
    const float d_x = 2.0f * x * d_r, d_y = 2.0f * y * d_r;
    const float fx_x = d + d_x * x + 2.0f * c.p1 * y + 6.0f * c.p2 * x;
    const float fx_y = d_y * x + 2.0f * c.p1 * x + 2.0f * c.p2 * y;
    const float fy_x = d_x * y + 2.0f * c.p2 * y + 2.0f * c.p1 * x;
    const float fy_y = d + d_y * y + 2.0f * c.p2 * x + 6.0f * c.p1 * y;
    const float den = fy_x * fx_y - fx_x * fy_y;
    const bool ok = fabsf(den) > 1e-9f;
    x += ok ? (fx * fy_y - fy * fx_y) / den : 0.0f;
    y += ok ? (fy * fx_x - fx * fy_x) / den : 0.0f;
  }
  xo = x;
  yo = y;
}

// pixel -> unit world direction (camera.py:225-269): normalised image coordinates, the undistort, orientation^T and the second
// normalisation.  Shared by the by-value kernels and the table kernels, so both give the same bits.
__device__ __forceinline__ void ray_direction(const CameraArgs& c, float2 px, float& wx, float& wy, float& wz) {
  float y = (px.y - c.cy) / (c.focal * c.aspect);
  float x = (px.x - c.cx - y * c.skew) / c.focal;
  if (c.distorted) undistort(c, x, y, x, y);
  const float inv = 1.0f / sqrtf(x * x + y * y + 1.0f);
  const float lx = x * inv, ly = y * inv, lz = inv;
  // world = orientation^T * local, renormalised (camera.py:262-267)
  wx = c.R[0] * lx + c.R[3] * ly + c.R[6] * lz;
  wy = c.R[1] * lx + c.R[4] * ly + c.R[7] * lz;
  wz = c.R[2] * lx + c.R[5] * ly + c.R[8] * lz;
  const float inv2 = 1.0f / sqrtf(wx * wx + wy * wy + wz * wz);
  wx *= inv2; wy *= inv2; wz *= inv2;
}

// (point - position) -> distorted pixel (camera.py:283-315); lz_out, when given, receives the coordinate along the optical axis
__device__ __forceinline__ float2 project_local(const CameraArgs& c, float tx, float ty, float tz, float* lz_out = nullptr) {
  const float lx = c.R[0] * tx + c.R[1] * ty + c.R[2] * tz;
  const float ly = c.R[3] * tx + c.R[4] * ty + c.R[5] * tz;
  const float lz = c.R[6] * tx + c.R[7] * ty + c.R[8] * tz;
  if (lz_out) *lz_out = lz;
  float x = lx / lz, y = ly / lz;
  const float r2 = x * x + y * y;
  const float dist = 1.0f + r2 * (c.k1 + r2 * (c.k2 + c.k3 * r2));
  const float xy = x * y;
  const float xd = x * dist + 2.0f * c.p1 * xy + c.p2 * (r2 + 2.0f * x * x);
  const float yd = y * dist + 2.0f * c.p2 * xy + c.p1 * (r2 + 2.0f * y * y);
  return make_float2(c.focal * xd + c.skew * yd + c.cx, c.focal * c.aspect * yd + c.cy);
}

// MODE 0: unit ray directions.  MODE 1: points at a given depth along the optical axis (pixels_to_points).
template <int MODE>
__global__ __launch_bounds__(CAM_THREADS) void camera_rays_kernel(CameraArgs c, const float2* __restrict__ pixels,
                                                                  const float* __restrict__ depth, long n,
                                                                  float* __restrict__ origins,
                                                                  float* __restrict__ directions,
                                                                  float2* __restrict__ pixels_out) {
  __shared__ float tile[3 * CAM_THREADS];
  const long base = (long)blockIdx.x * CAM_THREADS;
  const long i = base + threadIdx.x;
  float o[3] = {0.f, 0.f, 0.f};
  if (i < n) {
    float2 px;
    if (pixels) {
      px = pixels[i];
    } else {   // pixel centres of the [H, W] image in row-major order (camera.py:317-321)
      const long row = i / c.width;
      px = make_float2((float)(i - row * c.width) + 0.5f, (float)row + 0.5f);
    }
    if (pixels_out) pixels_out[i] = px;
    float wx, wy, wz;
    ray_direction(c, px, wx, wy, wz);
    if (MODE == 1) {   // rays * depth / cos(angle to the optical axis) + position (camera.py:271-277)
      const float s = depth[i] / (wx * c.R[6] + wy * c.R[7] + wz * c.R[8]);
      wx = wx * s + c.pos[0]; wy = wy * s + c.pos[1]; wz = wz * s + c.pos[2];
    }
    o[0] = wx; o[1] = wy; o[2] = wz;
  }
  tile[3 * threadIdx.x + 0] = o[0];
  tile[3 * threadIdx.x + 1] = o[1];
  tile[3 * threadIdx.x + 2] = o[2];
  __syncthreads();
  const long lim = min((long)3 * CAM_THREADS, 3 * (n - base));
#pragma unroll
  for (int e = 0; e < 3; ++e) {
    const int j = e * CAM_THREADS + threadIdx.x;
    if (j < lim) {
      directions[3 * base + j] = tile[j];
      if (origins) origins[3 * base + j] = c.pos[j % 3];   // 3*base is a multiple of 3
    }
  }
}

__global__ __launch_bounds__(CAM_THREADS) void camera_project_kernel(CameraArgs c, const float* __restrict__ points, long n,
                                                                     float2* __restrict__ pixels) {
  __shared__ float tile[3 * CAM_THREADS];
  const long base = (long)blockIdx.x * CAM_THREADS;
  const long lim = min((long)3 * CAM_THREADS, 3 * (n - base));
#pragma unroll
  for (int e = 0; e < 3; ++e) {
    const int j = e * CAM_THREADS + threadIdx.x;
    if (j < lim) tile[j] = points[3 * base + j] - c.pos[j % 3];
  }
  __syncthreads();
  const long i = base + threadIdx.x;
  if (i >= n) return;
  const float tx = tile[3 * threadIdx.x], ty = tile[3 * threadIdx.x + 1], tz = tile[3 * threadIdx.x + 2];
  pixels[i] = project_local(c, tx, ty, tz);
}


// ---- camera table ----

constexpr int NP = NRF_CAMERA_NPARAMS;   // 22 differentiable floats of a row; floats 22, 23 are pads: never read, gradient 0
constexpr int KEY_NONE = -1;             // block key: no ray of the workgroup has a camera
constexpr int KEY_MIXED = -2;            // block key: the workgroup's rays are of several cameras, one record per ray

// Row `row` of the table as the by-value kernels' argument block.  "Distorted" is the host's rule (camera.py:232) per row.
__device__ __forceinline__ CameraArgs load_camera_row(const float* __restrict__ cameras, int row) {
  const float* p = cameras + (long)row * NRF_CAMERA_ROW;   // 96 B rows of a 16-byte aligned table
  const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4),
               d = *reinterpret_cast<const float4*>(p + 8), e = *reinterpret_cast<const float4*>(p + 12),
               f = *reinterpret_cast<const float4*>(p + 16);
  const float2 g = *reinterpret_cast<const float2*>(p + 20);
  CameraArgs c;
  c.R[0] = a.x; c.R[1] = a.y; c.R[2] = a.z; c.R[3] = a.w; c.R[4] = b.x; c.R[5] = b.y; c.R[6] = b.z; c.R[7] = b.w; c.R[8] = d.x;
  c.pos[0] = d.y; c.pos[1] = d.z; c.pos[2] = d.w;
  c.focal = e.x; c.cx = e.y; c.cy = e.z; c.skew = e.w;
  c.aspect = f.x; c.k1 = f.y; c.k2 = f.z; c.k3 = f.w;
  c.p1 = g.x; c.p2 = g.y;
  c.width = c.height = 0;
  c.distorted = (c.k1 != 0.f || c.k2 != 0.f || c.k3 != 0.f || c.p1 != 0.f || c.p2 != 0.f) ? 1 : 0;
  return c;
}

// The ray's table row, or -1 for an index outside [0, C): such a ray reads no row, gets zero outputs and leaves no gradient.
__device__ __forceinline__ int camera_row_of(const int* __restrict__ camera_index, long i, int num_cameras) {
  const int k = camera_index ? camera_index[i] : 0;
  return (k >= 0 && k < num_cameras) ? k : -1;
}

__global__ __launch_bounds__(CAM_THREADS) void camera_table_rays_kernel(const float* __restrict__ cameras, int num_cameras,
                                                                        const int* __restrict__ camera_index,
                                                                        const float2* __restrict__ pixels, long n,
                                                                        float* __restrict__ origins, float* __restrict__ directions) {
  __shared__ float tile[3 * CAM_THREADS];
  __shared__ float otile[3 * CAM_THREADS];
  const long base = (long)blockIdx.x * CAM_THREADS;
  const long i = base + threadIdx.x;
  float w[3] = {0.f, 0.f, 0.f}, o[3] = {0.f, 0.f, 0.f};
  if (i < n) {
    const int row = camera_row_of(camera_index, i, num_cameras);
    if (row >= 0) {
      const CameraArgs c = load_camera_row(cameras, row);
      ray_direction(c, pixels[i], w[0], w[1], w[2]);
      o[0] = c.pos[0]; o[1] = c.pos[1]; o[2] = c.pos[2];
    }
  }
#pragma unroll
  for (int e = 0; e < 3; ++e) {
    tile[3 * threadIdx.x + e] = w[e];
    otile[3 * threadIdx.x + e] = o[e];
  }
  __syncthreads();
  const long lim = min((long)3 * CAM_THREADS, 3 * (n - base));
#pragma unroll
  for (int e = 0; e < 3; ++e) {
    const int j = e * CAM_THREADS + threadIdx.x;
    if (j < lim) {
      directions[3 * base + j] = tile[j];
      if (origins) origins[3 * base + j] = otile[j];
    }
  }
}

// One kernel for nrf_camera_table_project (pixels (n,2), screen NULL) and nrf_camera_table_project_depth (screen (n,3) = pixel and
// local z, pixels NULL): the arithmetic is the same instructions for both, so the pixel has the same bits.  No reverse pass takes z.
__global__ __launch_bounds__(CAM_THREADS) void camera_table_project_kernel(const float* __restrict__ cameras, int num_cameras,
                                                                           const int* __restrict__ camera_index,
                                                                           const float* __restrict__ points, long n,
                                                                           float2* __restrict__ pixels, float* __restrict__ screen) {
  __shared__ float tile[3 * CAM_THREADS];
  const long base = (long)blockIdx.x * CAM_THREADS;
  const long lim = min((long)3 * CAM_THREADS, 3 * (n - base));
#pragma unroll
  for (int e = 0; e < 3; ++e) {
    const int j = e * CAM_THREADS + threadIdx.x;
    if (j < lim) tile[j] = points[3 * base + j];
  }
  __syncthreads();
  const long i = base + threadIdx.x;
  if (i >= n) return;
  const int row = camera_row_of(camera_index, i, num_cameras);
  float2 px = make_float2(0.f, 0.f);
  float z = 0.f;
  if (row >= 0) {
    const CameraArgs c = load_camera_row(cameras, row);
    px = project_local(c, tile[3 * threadIdx.x] - c.pos[0], tile[3 * threadIdx.x + 1] - c.pos[1], tile[3 * threadIdx.x + 2] - c.pos[2], &z);
  }
  if (screen) {
    screen[3 * i + 0] = px.x;
    screen[3 * i + 1] = px.y;
    screen[3 * i + 2] = z;
  } else {
    pixels[i] = px;
  }
}

// d distort / d (x, y) at (x, y), the matrix the forward's Newton step inverts.
struct DistortJac {
  float r, xx, xy, yx, yy;   // r = x^2 + y^2; xx = d xd/dx, xy = d xd/dy, yx = d yd/dx, yy = d yd/dy
};
__device__ __forceinline__ DistortJac distort_jacobian(const CameraArgs& c, float x, float y) {
  DistortJac j;
  j.r = x * x + y * y;
  const float d = 1.0f + j.r * (c.k1 + j.r * (c.k2 + c.k3 * j.r));
  const float d_r = c.k1 + j.r * (2.0f * c.k2 + 3.0f * c.k3 * j.r);
  const float d_x = 2.0f * x * d_r, d_y = 2.0f * y * d_r;
  j.xx = d + d_x * x + 2.0f * c.p1 * y + 6.0f * c.p2 * x;
  j.xy = d_y * x + 2.0f * c.p1 * x + 2.0f * c.p2 * y;
  j.yx = d_x * y + 2.0f * c.p2 * y + 2.0f * c.p1 * x;
  j.yy = d + d_y * y + 2.0f * c.p2 * x + 6.0f * c.p1 * y;
  return j;
}

// g[17..21] += (a, b) . d distort / d (k1, k2, k3, p1, p2) at (x, y)
__device__ __forceinline__ void distort_coefficient_grads(float x, float y, float r, float a, float b, float* g) {
  const float s = a * x + b * y;
  g[17] = s * r;
  g[18] = s * r * r;
  g[19] = s * r * r * r;
  g[20] = a * (2.0f * x * y) + b * (r + 2.0f * y * y);
  g[21] = a * (r + 2.0f * x * x) + b * (2.0f * x * y);
}

// Reverse of ray_direction (and of origin = position) for one ray: g[0..21] in table order, dpx = d loss / d pixel.
// The undistort is differentiated by the implicit-function theorem at the forward's result: J^T lambda = g,
// d/d(xd, yd) = lambda, d/dk = -lambda . d distort/dk -- for a camera with zero coefficients too (J = I there).
__device__ __forceinline__ void rays_vjp(const CameraArgs& c, float2 px, const float* go, const float* gd, float* g, float2& dpx) {
  const float fa = c.focal * c.aspect;
  const float y0 = (px.y - c.cy) / fa;
  const float x0 = (px.x - c.cx - y0 * c.skew) / c.focal;
  float x = x0, y = y0;
  if (c.distorted) undistort(c, x0, y0, x, y);
  const float inv = 1.0f / sqrtf(x * x + y * y + 1.0f);
  const float l[3] = {x * inv, y * inv, inv};
  float w[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) w[j] = c.R[j] * l[0] + c.R[3 + j] * l[1] + c.R[6 + j] * l[2];
  const float inv2 = 1.0f / sqrtf(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
  // d = w / |w|: orientation is nine free parameters, so this normalisation has a derivative although it keeps the value
  const float dg = (w[0] * gd[0] + w[1] * gd[1] + w[2] * gd[2]) * inv2;
  float gw[3], gl[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) gw[j] = inv2 * (gd[j] - w[j] * inv2 * dg);
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) g[3 * i + j] = l[i] * gw[j];
    gl[i] = c.R[3 * i] * gw[0] + c.R[3 * i + 1] * gw[1] + c.R[3 * i + 2] * gw[2];
    g[9 + i] = go[i];
  }
  const float lg = l[0] * gl[0] + l[1] * gl[1] + l[2] * gl[2];
  const float gx = inv * (gl[0] - l[0] * lg), gy = inv * (gl[1] - l[1] * lg);
  const DistortJac J = distort_jacobian(c, x, y);
  const float det = J.xx * J.yy - J.xy * J.yx;
  const bool ok = fabsf(det) > 1e-9f;   // where the forward skips its update: lambda = g, no coefficient gradient
  const float lx = ok ? (J.yy * gx - J.yx * gy) / det : gx;
  const float ly = ok ? (J.xx * gy - J.xy * gx) / det : gy;
  distort_coefficient_grads(x, y, J.r, ok ? -lx : 0.0f, ok ? -ly : 0.0f, g);
  const float t = lx / c.focal;          // d / d (px - cx - y0 skew)
  const float gy0 = ly - t * c.skew;
  const float u = gy0 / fa;              // d / d (py - cy)
  dpx = make_float2(t, u);
  g[12] = -(t * x0) - u * c.aspect * y0;
  g[13] = -t;
  g[14] = -u;
  g[15] = -(t * y0);
  g[16] = -(u * c.focal * y0);
}

// Reverse of project_local(point - position): g[0..21] in table order, dpt = d loss / d point.
__device__ __forceinline__ void project_vjp(const CameraArgs& c, const float* pt, float2 gp, float* g, float* dpt) {
  const float t[3] = {pt[0] - c.pos[0], pt[1] - c.pos[1], pt[2] - c.pos[2]};
  float l[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) l[i] = c.R[3 * i] * t[0] + c.R[3 * i + 1] * t[1] + c.R[3 * i + 2] * t[2];
  const float x = l[0] / l[2], y = l[1] / l[2];
  const DistortJac J = distort_jacobian(c, x, y);
  const float dist = 1.0f + J.r * (c.k1 + J.r * (c.k2 + c.k3 * J.r));
  const float xd = x * dist + 2.0f * c.p1 * x * y + c.p2 * (J.r + 2.0f * x * x);
  const float yd = y * dist + 2.0f * c.p2 * x * y + c.p1 * (J.r + 2.0f * y * y);
  // px = focal xd + skew yd + cx, py = focal aspect yd + cy
  g[12] = gp.x * xd + gp.y * c.aspect * yd;
  g[13] = gp.x;
  g[14] = gp.y;
  g[15] = gp.x * yd;
  g[16] = gp.y * c.focal * yd;
  const float gxd = gp.x * c.focal, gyd = gp.x * c.skew + gp.y * c.focal * c.aspect;
  distort_coefficient_grads(x, y, J.r, gxd, gyd, g);
  const float gx = gxd * J.xx + gyd * J.yx, gy = gxd * J.xy + gyd * J.yy;
  const float gl[3] = {gx / l[2], gy / l[2], -(gx * x + gy * y) / l[2]};
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) g[3 * i + j] = gl[i] * t[j];
  }
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    dpt[j] = c.R[j] * gl[0] + c.R[3 + j] * gl[1] + c.R[6 + j] * gl[2];
    g[9 + j] = -dpt[j];
  }
}

// Sum of v over the workgroup in a fixed order: xor butterflies inside each wave (every lane ends with the same bits), then the four
// waves' partials in wave order.  NP values at once; the result is returned to threads 0..NP-1.
__device__ __forceinline__ float block_sum_params(const float* g, float (*part)[NRF_CAMERA_ROW]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    float v = g[p];
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    if (lane == 0) part[wave][p] = v;
  }
  __syncthreads();
  float r = 0.f;
  if (threadIdx.x < NP) r = ((part[0][threadIdx.x] + part[1][threadIdx.x]) + part[2][threadIdx.x]) + part[3][threadIdx.x];
  return r;
}

// Workspace of a reverse pass, nb = ceil(n / 256) workgroups: ray keys [nb*256] int32, ray values [NP][nb*256], block keys [nb]
// int32, block values [NP][nb] (SoA, so a wave's stores are contiguous).  Stage 1 writes every block key, and the ray keys of a
// MIXED block only; stage 2 reads nothing else, so the workspace needs no clearing.
struct TableWorkspace {
  int* ray_keys;
  float* ray_vals;
  int* block_keys;
  float* block_vals;
  long nb, np;
};
__host__ __device__ inline TableWorkspace table_workspace(void* ws, long n) {
  TableWorkspace t;
  t.nb = (n + CAM_THREADS - 1) / CAM_THREADS;
  t.np = t.nb * CAM_THREADS;
  t.ray_keys = reinterpret_cast<int*>(ws);
  t.ray_vals = reinterpret_cast<float*>(t.ray_keys + t.np);
  t.block_keys = reinterpret_cast<int*>(t.ray_vals + NP * t.np);
  t.block_vals = reinterpret_cast<float*>(t.block_keys + t.nb);
  return t;
}

// Stage 1 of a reverse pass.  MODE 0: rays (in = pixels [n,2], ga = d_origins, gb = d_directions, d_in = d_pixels [n,2]);
// MODE 1: projection (in = points [n,3], ga = d_pixels [n,2], d_in = d_points [n,3]).  NULL cotangents are zeros.
template <int MODE>
__global__ __launch_bounds__(CAM_THREADS) void camera_table_vjp_kernel(const float* __restrict__ cameras, int num_cameras,
                                                                       const int* __restrict__ camera_index,
                                                                       const float* __restrict__ in, const float* __restrict__ ga,
                                                                       const float* __restrict__ gb, long n, TableWorkspace ws,
                                                                       float* __restrict__ d_in) {
  __shared__ float part[4][NRF_CAMERA_ROW];
  __shared__ int key0;
  const long base = (long)blockIdx.x * CAM_THREADS;
  const long i = base + threadIdx.x;
  float g[NP];
#pragma unroll
  for (int p = 0; p < NP; ++p) g[p] = 0.f;
  int key = KEY_NONE;
  if (i < n) {
    key = camera_row_of(camera_index, i, num_cameras);
    float din[3] = {0.f, 0.f, 0.f};
    if (key >= 0) {
      const CameraArgs c = load_camera_row(cameras, key);
      if (MODE == 0) {
        float go[3], gd[3];
#pragma unroll
        for (int e = 0; e < 3; ++e) {
          go[e] = ga ? ga[3 * i + e] : 0.f;
          gd[e] = gb ? gb[3 * i + e] : 0.f;
        }
        float2 dpx;
        rays_vjp(c, reinterpret_cast<const float2*>(in)[i], go, gd, g, dpx);
        din[0] = dpx.x; din[1] = dpx.y;
      } else {
        const float pt[3] = {in[3 * i], in[3 * i + 1], in[3 * i + 2]};
        project_vjp(c, pt, reinterpret_cast<const float2*>(ga)[i], g, din);
      }
    }
    if (d_in) {
      if (MODE == 0) {
        reinterpret_cast<float2*>(d_in)[i] = make_float2(din[0], din[1]);
      } else {
#pragma unroll
        for (int e = 0; e < 3; ++e) d_in[3 * i + e] = din[e];
      }
    }
  }
  if (threadIdx.x == 0) key0 = key;   // ray `base` exists in every launched workgroup
  __syncthreads();
  const int k0 = key0;
  const bool shared_camera = __syncthreads_and(i >= n || key == k0) && k0 >= 0;
  if (shared_camera) {   // one record for the workgroup (rays past n hold zeros)
    const float r = block_sum_params(g, part);
    if (threadIdx.x < NP) ws.block_vals[threadIdx.x * ws.nb + blockIdx.x] = r;
    if (threadIdx.x == 0) ws.block_keys[blockIdx.x] = k0;
    return;
  }
  const bool any = __syncthreads_or(key >= 0);
  if (threadIdx.x == 0) ws.block_keys[blockIdx.x] = any ? KEY_MIXED : KEY_NONE;
  if (!any) return;
  ws.ray_keys[i] = key;   // i < np
  if (key >= 0) {
#pragma unroll
    for (int p = 0; p < NP; ++p) ws.ray_vals[p * ws.np + i] = g[p];
  }
}

// Stage 2: workgroup c sums camera c's records.  Thread t takes the block records b = t (mod 256) and, of every MIXED block, ray
// t, both in increasing b, 256 blocks at a time; the 256 partial sums then go through block_sum_params.  The block keys decide
// which ray keys are read at all: a whole frame of one camera costs nb block keys, a permuted batch n keys per camera.
__global__ __launch_bounds__(CAM_THREADS) void camera_table_reduce_kernel(TableWorkspace ws, float* __restrict__ d_cameras) {
  __shared__ float part[4][NRF_CAMERA_ROW];
  __shared__ unsigned long long mixed[4];
  const int cam = blockIdx.x;
  float acc[NP];
#pragma unroll
  for (int p = 0; p < NP; ++p) acc[p] = 0.f;
  for (long cb = 0; cb < ws.nb; cb += CAM_THREADS) {
    const long b = cb + threadIdx.x;
    const int kb = b < ws.nb ? ws.block_keys[b] : KEY_NONE;
    if (kb == cam) {
#pragma unroll
      for (int p = 0; p < NP; ++p) acc[p] += ws.block_vals[p * ws.nb + b];
    }
    const unsigned long long m = __ballot(kb == KEY_MIXED);
    if ((threadIdx.x & 63) == 0) mixed[threadIdx.x >> 6] = m;
    __syncthreads();
    for (int j = 0; j < CAM_THREADS; j += 8) {   // eight blocks' keys in flight at once
      const unsigned bits = __builtin_amdgcn_readfirstlane((unsigned)(mixed[j >> 6] >> (j & 63)) & 0xffu);
      if (bits == 0) continue;
      int k[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) k[u] = (bits >> u & 1u) ? ws.ray_keys[(cb + j + u) * CAM_THREADS + threadIdx.x] : KEY_NONE;
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        if (k[u] == cam) {
          const long slot = (cb + j + u) * CAM_THREADS + threadIdx.x;
#pragma unroll
          for (int p = 0; p < NP; ++p) acc[p] += ws.ray_vals[p * ws.np + slot];
        }
      }
    }
    __syncthreads();   // mixed[] is rewritten by the next 256 blocks
  }
  const float r = block_sum_params(acc, part);
  if (threadIdx.x < NRF_CAMERA_ROW) d_cameras[(long)cam * NRF_CAMERA_ROW + threadIdx.x] = threadIdx.x < NP ? r : 0.f;
}

// ---- camera delta tables (nrf_camera_table_compose*): one thread per camera.  The rotation is the SE3 field's closed form with
// v = 0 on the columns of R0 (se3_math.h: the theta^2 series below |omega|^2 = 4), so value and VJP are exact at omega = 0.
constexpr int ND = NRF_CAMERA_DELTA_ROW;

__global__ __launch_bounds__(CAM_THREADS) void camera_compose_kernel(const float* __restrict__ cameras, const float* __restrict__ deltas,
                                                                     int num_cameras, float* __restrict__ out) {
  const int cam = blockIdx.x * CAM_THREADS + threadIdx.x;
  if (cam >= num_cameras) return;
  const float* __restrict__ b = cameras + (long)cam * NRF_CAMERA_ROW;
  const float* __restrict__ d = deltas + (long)cam * ND;
  float* __restrict__ o = out + (long)cam * NRF_CAMERA_ROW;
  const V3 w = v3(d[0], d[1], d[2]), zero = v3(0.f, 0.f, 0.f);
  const Se3Coef<float> k = se3_coef<float>(dot(w, w));
  for (int j = 0; j < 3; ++j) {   // column j of R0 (row-major orientation[3 i + j])
    const V3 c = v3(b[j], b[3 + j], b[6 + j]);
    const V3 r = c + se3_delta_c<float>(k, w, zero, c);
    o[j] = r.x; o[3 + j] = r.y; o[6 + j] = r.z;
  }
  for (int i = 0; i < 3; ++i) o[9 + i] = b[9 + i] + d[3 + i];
  o[12] = b[12] * expf(d[6]);
  o[13] = b[13] + d[7]; o[14] = b[14] + d[8];
  o[15] = b[15]; o[16] = b[16];
  for (int i = 0; i < 5; ++i) o[17 + i] = b[17 + i] + d[9 + i];   // radial [3], tangential [2]
  o[22] = 0.f; o[23] = 0.f;
}

__global__ __launch_bounds__(CAM_THREADS) void camera_compose_bwd_kernel(const float* __restrict__ cameras, const float* __restrict__ deltas,
                                                                         int num_cameras, const float* __restrict__ d_cameras,
                                                                         float* __restrict__ d_deltas) {
  const int cam = blockIdx.x * CAM_THREADS + threadIdx.x;
  if (cam >= num_cameras) return;
  const float* __restrict__ b = cameras + (long)cam * NRF_CAMERA_ROW;
  const float* __restrict__ d = deltas + (long)cam * ND;
  const float* __restrict__ g = d_cameras + (long)cam * NRF_CAMERA_ROW;
  float* __restrict__ o = d_deltas + (long)cam * ND;
  const V3 w = v3(d[0], d[1], d[2]), zero = v3(0.f, 0.f, 0.f);
  const Se3Coef<float> k = se3_coef<float>(dot(w, w));
  V3 dw = zero;
  for (int j = 0; j < 3; ++j) {
    V3 dwj, dvj;
    se3_vjp_c<float>(k, w, zero, v3(b[j], b[3 + j], b[6 + j]), v3(g[j], g[3 + j], g[6 + j]), dwj, dvj);
    dw = dw + dwj;
  }
  o[0] = dw.x; o[1] = dw.y; o[2] = dw.z;
  for (int i = 0; i < 3; ++i) o[3 + i] = g[9 + i];
  o[6] = g[12] * b[12] * expf(d[6]);
  o[7] = g[13]; o[8] = g[14];
  for (int i = 0; i < 5; ++i) o[9 + i] = g[17 + i];
  o[14] = 0.f; o[15] = 0.f;
}

}  // namespace

void launch_camera_compose(const float* cameras, const float* deltas, int num_cameras, float* out, hipStream_t stream) {
  camera_compose_kernel<<<(unsigned)((num_cameras + CAM_THREADS - 1) / CAM_THREADS), CAM_THREADS, 0, stream>>>(cameras, deltas,
                                                                                                              num_cameras, out);
}

void launch_camera_compose_backward(const float* cameras, const float* deltas, int num_cameras, const float* d_cameras, float* d_deltas,
                                    hipStream_t stream) {
  camera_compose_bwd_kernel<<<(unsigned)((num_cameras + CAM_THREADS - 1) / CAM_THREADS), CAM_THREADS, 0, stream>>>(
      cameras, deltas, num_cameras, d_cameras, d_deltas);
}

void launch_camera_rays(const CameraArgs& c, const float* pixels, const float* depth, long n, float* origins,
                        float* directions, float* pixels_out, hipStream_t stream) {
  const unsigned blocks = (unsigned)((n + CAM_THREADS - 1) / CAM_THREADS);
  if (depth)
    camera_rays_kernel<1><<<blocks, CAM_THREADS, 0, stream>>>(c, (const float2*)pixels, depth, n, nullptr, directions,
                                                             (float2*)pixels_out);
  else
    camera_rays_kernel<0><<<blocks, CAM_THREADS, 0, stream>>>(c, (const float2*)pixels, nullptr, n, origins, directions,
                                                             (float2*)pixels_out);
}

void launch_camera_project(const CameraArgs& c, const float* points, long n, float* pixels, hipStream_t stream) {
  const unsigned blocks = (unsigned)((n + CAM_THREADS - 1) / CAM_THREADS);
  camera_project_kernel<<<blocks, CAM_THREADS, 0, stream>>>(c, points, n, (float2*)pixels);
}

size_t camera_table_workspace_bytes(long n) {
  const long nb = (n + CAM_THREADS - 1) / CAM_THREADS > 0 ? (n + CAM_THREADS - 1) / CAM_THREADS : 1;
  return (size_t)nb * (CAM_THREADS + 1) * (NP + 1) * sizeof(float);
}

void launch_camera_table_rays(const float* cameras, int num_cameras, const int* camera_index, const float* pixels, long n,
                              float* origins, float* directions, hipStream_t stream) {
  const unsigned blocks = (unsigned)((n + CAM_THREADS - 1) / CAM_THREADS);
  camera_table_rays_kernel<<<blocks, CAM_THREADS, 0, stream>>>(cameras, num_cameras, camera_index, (const float2*)pixels, n, origins,
                                                               directions);
}

void launch_camera_table_project(const float* cameras, int num_cameras, const int* camera_index, const float* points, long n,
                                 float* pixels, hipStream_t stream) {
  const unsigned blocks = (unsigned)((n + CAM_THREADS - 1) / CAM_THREADS);
  camera_table_project_kernel<<<blocks, CAM_THREADS, 0, stream>>>(cameras, num_cameras, camera_index, points, n, (float2*)pixels, nullptr);
}

void launch_camera_table_project_depth(const float* cameras, int num_cameras, const int* camera_index, const float* points, long n,
                                       float* screen, hipStream_t stream) {
  const unsigned blocks = (unsigned)((n + CAM_THREADS - 1) / CAM_THREADS);
  camera_table_project_kernel<<<blocks, CAM_THREADS, 0, stream>>>(cameras, num_cameras, camera_index, points, n, nullptr, screen);
}

void launch_camera_table_rays_backward(const float* cameras, int num_cameras, const int* camera_index, const float* pixels, long n,
                                       const float* d_origins, const float* d_directions, float* d_cameras, float* d_pixels,
                                       void* workspace, hipStream_t stream) {
  const TableWorkspace ws = table_workspace(workspace, n);
  if (ws.nb)
    camera_table_vjp_kernel<0><<<(unsigned)ws.nb, CAM_THREADS, 0, stream>>>(cameras, num_cameras, camera_index, pixels, d_origins,
                                                                           d_directions, n, ws, d_pixels);
  camera_table_reduce_kernel<<<num_cameras, CAM_THREADS, 0, stream>>>(ws, d_cameras);
}

void launch_camera_table_project_backward(const float* cameras, int num_cameras, const int* camera_index, const float* points, long n,
                                          const float* d_pixels, float* d_cameras, float* d_points, void* workspace,
                                          hipStream_t stream) {
  const TableWorkspace ws = table_workspace(workspace, n);
  if (ws.nb)
    camera_table_vjp_kernel<1><<<(unsigned)ws.nb, CAM_THREADS, 0, stream>>>(cameras, num_cameras, camera_index, points, d_pixels,
                                                                           nullptr, n, ws, d_points);
  camera_table_reduce_kernel<<<num_cameras, CAM_THREADS, 0, stream>>>(ws, d_cameras);
}

}  // namespace nrf
