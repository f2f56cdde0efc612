// Surface nets on a device density grid (nrf_mesh_count / nrf_mesh_emit / nrf_mesh_snap; the definition is in
// include/nerfies_amd.h): an indexed, deterministic triangle mesh of the level set sigma = threshold.
//
// Cells are walked in their linear order, i fastest: a workgroup of 256 threads owns Cells::BLOCK = 1024 consecutive cells as four
// rounds of 256, so the 64 lanes of a wave read consecutive x (the eight corner reads of a wave are eight runs of 65 floats, but for
// the rows that end inside the wave) and the neighbours' re-reads hit the cache.  Every output slot is a rank, by the rule of
// mesh_rank.h: the number of active cells (quads) before this one in that order.  The kernels here say what is voted on (a cell is
// active; the up to three quads it owns) and what is written at the slot; the host half is built from mesh_host.h.
//
// Every float operation below is a single rounding in the order the header states: contraction is off for the whole file.
#include "mesh_host.h"
#include "mesh_rank.h"

#include <cmath>

#pragma clang fp contract(off)

using namespace nrf;
using namespace nrf::api;

namespace {

constexpr int ROUNDS = 4;
using Cells = MeshRank<ROUNDS>;

struct MeshDims {
  int X, Y, Z;      // samples
  int cx, cy, cz;   // cells
  int ncells;
  int nblocks;      // workgroups of Cells::BLOCK cells
};

// byte offsets of the workspace's regions
struct MeshPlan {
  size_t block_v, block_q, mask, map, total;
};

MeshDims mesh_dims(const nrf_grid* g) {
  MeshDims d;
  d.X = g->dims[0]; d.Y = g->dims[1]; d.Z = g->dims[2];
  d.cx = d.X - 1; d.cy = d.Y - 1; d.cz = d.Z - 1;
  d.ncells = d.cx * d.cy * d.cz;
  d.nblocks = (int)blocks_of(d.ncells, Cells::BLOCK);
  return d;
}

MeshPlan mesh_plan(const MeshDims& d) {
  MeshPlan p;
  MeshCarve c;
  p.block_v = c.take(sizeof(int) * (size_t)d.nblocks);
  p.block_q = c.take(sizeof(int) * (size_t)d.nblocks);
  p.mask = c.take((size_t)d.ncells);
  p.map = c.take(sizeof(int) * (size_t)d.ncells);
  p.total = c.total;
  return p;
}

__device__ __forceinline__ void cell_coords(int cell, const MeshDims& d, int& i, int& j, int& k) {
  i = cell % d.cx;
  const int r = cell / d.cx;
  j = r % d.cy;
  k = r / d.cy;
}

// a thread's cell of round r: an int, as everything derived from it is (at most NRF_MESH_MAX_CELLS cells, rounded up to a workgroup)
__device__ __forceinline__ int owned_cell(const int r) { return (int)Cells::owned(r); }

// the three quads a cell may own, from its corner mask and its position: bit ax set iff the samples at c and c + e_ax differ in
// insideness and c[u] >= 1, c[v] >= 1 (u = ax + 1, v = ax + 2 mod 3)
__device__ __forceinline__ unsigned owned_quads(unsigned m, int i, int j, int k) {
  const unsigned c0 = m & 1u;
  unsigned q = 0;
  if ((((m >> 1) & 1u) != c0) && j >= 1 && k >= 1) q |= 1u;
  if ((((m >> 2) & 1u) != c0) && k >= 1 && i >= 1) q |= 2u;
  if ((((m >> 4) & 1u) != c0) && i >= 1 && j >= 1) q |= 4u;
  return q;
}

// Stage 1: corner mask per cell, per-workgroup totals of active cells and owned quads.
__global__ __launch_bounds__(MESH_THREADS) void mesh_classify_kernel(const float* __restrict__ sigma, const MeshDims d, const float thr,
                                                                     unsigned char* __restrict__ mask, int* __restrict__ block_v,
                                                                     int* __restrict__ block_q) {
  __shared__ int sv[Cells::SLOTS], sq[Cells::SLOTS];
  const size_t sy = (size_t)d.X, sz = (size_t)d.X * (size_t)d.Y;
#pragma unroll
  for (int r = 0; r < ROUNDS; ++r) {
    const int cell = owned_cell(r);
    bool active = false;
    unsigned q = 0;
    if (cell < d.ncells) {
      int i, j, k;
      cell_coords(cell, d, i, j, k);
      const float* s = sigma + ((size_t)i + sy * (size_t)j + sz * (size_t)k);
      unsigned m = 0;
#pragma unroll
      for (int b = 0; b < 8; ++b) {
        const float v = s[(size_t)(b & 1) + sy * (size_t)((b >> 1) & 1) + sz * (size_t)(b >> 2)];
        m |= (v > thr ? 1u : 0u) << b;   // strict: a NaN sample is outside
      }
      mask[cell] = (unsigned char)m;
      active = m != 0u && m != 255u;
      q = owned_quads(m, i, j, k);
    }
    Cells::vote(sv, r, active);
    Cells::vote<3>(sq, r, q);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    block_v[blockIdx.x] = Cells::block_total(sv);
    block_q[blockIdx.x] = Cells::block_total(sq);
  }
}

// Stage 2: exclusive scans of the workgroup totals, in place, by ONE workgroup (mesh_scan.h); the totals go to the workspace's status
// words and to the caller's counts.
__global__ __launch_bounds__(SCAN_THREADS) void mesh_scan_kernel(int* __restrict__ block_v, int* __restrict__ block_q, const int nblocks,
                                                                 int* __restrict__ status, int* __restrict__ counts) {
  int nv, nq;
  mesh_scan_totals(block_v, nblocks, block_q, nblocks, nv, nq);
  if (threadIdx.x == SCAN_THREADS - 1) {
    const int nt = 2 * nq;
    status[0] = nv;
    status[1] = nt;
    status[2] = 0;
    status[3] = 0;
    counts[0] = nv;
    counts[1] = nt;
  }
}

// the vertex of an active cell: the mean of its edge crossings in cell-local coordinates, then (idx + local) * step + origin
__device__ __forceinline__ void cell_vertex(const float* __restrict__ s, const size_t sy, const size_t sz, const unsigned m, const float thr,
                                            const int i, const int j, const int k, const nrf_grid& g, float out[3]) {
  float v[8];
#pragma unroll
  for (int b = 0; b < 8; ++b) v[b] = s[(size_t)(b & 1) + sy * (size_t)((b >> 1) & 1) + sz * (size_t)(b >> 2)];
  float ax = 0.f, ay = 0.f, az = 0.f;
  int count = 0;
#pragma unroll
  for (int a = 0; a < 8; ++a) {
#pragma unroll
    for (int axis = 0; axis < 3; ++axis) {
      if ((a >> axis) & 1) continue;
      const int b = a | (1 << axis);
      if ((((m >> a) ^ (m >> b)) & 1u) == 0u) continue;
      float t = (thr - v[a]) / (v[b] - v[a]);
      if (!isfinite(t)) t = 0.5f;
      else if (t < 0.f) t = 0.f;
      else if (t > 1.f) t = 1.f;
      float px = (float)(a & 1), py = (float)((a >> 1) & 1), pz = (float)(a >> 2);
      if (axis == 0) px = px + t;
      if (axis == 1) py = py + t;
      if (axis == 2) pz = pz + t;
      ax = ax + px;
      ay = ay + py;
      az = az + pz;
      ++count;
    }
  }
  const float n = (float)count;
  const float lx = ax / n, ly = ay / n, lz = az / n;
  const float hx = (float)i + lx, hy = (float)j + ly, hz = (float)k + lz;
  const float mx = hx * g.step[0], my = hy * g.step[1], mz = hz * g.step[2];
  out[0] = mx + g.origin[0];
  out[1] = my + g.origin[1];
  out[2] = mz + g.origin[2];
}

// Stage 3a: the cell-to-vertex map (always), and, when both capacities hold the scanned totals, the vertices and their cells.
__global__ __launch_bounds__(MESH_THREADS) void mesh_vertices_kernel(const float* __restrict__ sigma, const MeshDims d, const nrf_grid g,
                                                                     const float thr, const unsigned char* __restrict__ mask,
                                                                     const int* __restrict__ block_v, int* __restrict__ status,
                                                                     const int max_vertices, const int max_triangles,
                                                                     float* __restrict__ vertices, int* __restrict__ vertex_cell,
                                                                     int* __restrict__ map) {
  __shared__ int sv[Cells::SLOTS];
  const bool fits = status[0] <= max_vertices && status[1] <= max_triangles;
  int rank[ROUNDS];
  unsigned ms[ROUNDS];
#pragma unroll
  for (int r = 0; r < ROUNDS; ++r) {
    const int cell = owned_cell(r);
    ms[r] = cell < d.ncells ? (unsigned)mask[cell] : 0u;
    rank[r] = Cells::vote(sv, r, ms[r] != 0u && ms[r] != 255u);
  }
  __syncthreads();
  if (blockIdx.x == 0 && threadIdx.x == 0) {   // what the caller reads back: all of the mesh, or none of it
    status[2] = fits ? status[0] : 0;
    status[3] = fits ? status[1] : 0;
  }
  const size_t sy = (size_t)d.X, sz = (size_t)d.X * (size_t)d.Y;
  Cells::walk(sv, block_v[blockIdx.x], [&](const int r, const int before) {
    const int cell = owned_cell(r);
    const unsigned m = ms[r];
    if (cell >= d.ncells) return;
    const bool active = m != 0u && m != 255u;
    const int vid = before + rank[r];
    map[cell] = active ? vid : -1;
    if (active && fits && vid < max_vertices) {
      int i, j, k;
      cell_coords(cell, d, i, j, k);
      float p[3];
      cell_vertex(sigma + ((size_t)i + sy * (size_t)j + sz * (size_t)k), sy, sz, m, thr, i, j, k, g, p);
      vertices[3 * (size_t)vid + 0] = p[0];
      vertices[3 * (size_t)vid + 1] = p[1];
      vertices[3 * (size_t)vid + 2] = p[2];
      vertex_cell[vid] = cell;
    }
  });
}

// Stage 3b: two triangles per owned quad, from the map.
__global__ __launch_bounds__(MESH_THREADS) void mesh_faces_kernel(const MeshDims d, const unsigned char* __restrict__ mask,
                                                                  const int* __restrict__ map, const int* __restrict__ block_q,
                                                                  const int* __restrict__ status, const int max_vertices,
                                                                  const int max_triangles, int* __restrict__ triangles) {
  __shared__ int sq[Cells::SLOTS];
  if (!(status[0] <= max_vertices && status[1] <= max_triangles)) return;   // uniform over the grid
  int rank[ROUNDS];
  unsigned qs[ROUNDS];
#pragma unroll
  for (int r = 0; r < ROUNDS; ++r) {
    const int cell = owned_cell(r);
    unsigned q = 0;
    if (cell < d.ncells) {
      int i, j, k;
      cell_coords(cell, d, i, j, k);
      const unsigned m = (unsigned)mask[cell];
      q = owned_quads(m, i, j, k) | ((m & 1u) << 3);   // bit 3: the sample at c is inside
    }
    qs[r] = q;
    rank[r] = Cells::vote<3>(sq, r, q);   // a lane's quads are consecutive, in axis order
  }
  __syncthreads();
  const int ey = d.cx, ez = d.cx * d.cy;   // cell strides
  Cells::walk(sq, block_q[blockIdx.x], [&](const int r, const int before) {
    if ((qs[r] & 7u) == 0u) return;
    const int cell = owned_cell(r);
    const bool inside = (qs[r] & 8u) != 0u;
    int quad = before + rank[r];
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
      if (((qs[r] >> ax) & 1u) == 0u) continue;
      const int eu = ax == 0 ? ey : (ax == 1 ? ez : 1), ev = ax == 0 ? ez : (ax == 1 ? 1 : ey);
      int q0 = map[cell - eu - ev], q1 = map[cell - ev], q2 = map[cell], q3 = map[cell - eu];
      if (!inside) {
        int t = q0; q0 = q3; q3 = t;
        t = q1; q1 = q2; q2 = t;
      }
      const long long tri = 2ll * quad;
      if (tri + 1 < (long long)max_triangles) {
        int* o = triangles + 3 * (size_t)tri;
        o[0] = q0; o[1] = q1; o[2] = q2;
        o[3] = q0; o[4] = q2; o[5] = q3;
      }
      ++quad;
    }
  });
}

// One Newton step onto the level set per vertex, then the clamp to the vertex's own cell.
__global__ __launch_bounds__(MESH_THREADS) void mesh_snap_kernel(float* __restrict__ vertices, const int* __restrict__ vertex_cell,
                                                                 const float* __restrict__ sigma_at, const float* __restrict__ grad_at,
                                                                 const nrf_grid g, const MeshDims d, const float thr, const int n) {
  const int v = blockIdx.x * MESH_THREADS + threadIdx.x;
  if (v >= n) return;
  const float gx = grad_at[3 * (size_t)v + 0], gy = grad_at[3 * (size_t)v + 1], gz = grad_at[3 * (size_t)v + 2];
  const float sg = sigma_at[v];
  const float s = fmaf(gz, gz, fmaf(gy, gy, gx * gx));
  if (!(s > 0.f) || !isfinite(s) || !isfinite(sg)) return;
  const int cell = vertex_cell[v];
  if (cell < 0 || cell >= d.ncells) return;   // not a vertex of this grid: nothing to clamp to
  int idx[3];
  cell_coords(cell, d, idx[0], idx[1], idx[2]);
  const float q = (sg - thr) / s;
  const float gr[3] = {gx, gy, gz};
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    float x = fmaf(-q, gr[c], vertices[3 * (size_t)v + c]);
    const float p0 = (float)idx[c] * g.step[c], p1 = (float)(idx[c] + 1) * g.step[c];
    const float e0 = g.origin[c] + p0, e1 = g.origin[c] + p1;
    const float lo = e0 < e1 ? e0 : e1, hi = e0 < e1 ? e1 : e0;
    if (!(x >= lo)) x = lo;   // a NaN (an infinite step times a zero slope) lands on lo
    else if (x > hi) x = hi;
    vertices[3 * (size_t)v + c] = x;
  }
}

// what every entry checks of its grid and threshold before any HIP call
int mesh_args(const char* entry, const nrf_grid* grid, float threshold, bool with_threshold) {
  if (!grid) return mesh_null(entry, "grid");
  long long cells = 1;
  for (int c = 0; c < 3; ++c) {
    if (grid->dims[c] < 2) {
      char msg[200];
      snprintf(msg, sizeof(msg), "%s: grid->dims[%d] = %d: a mesh needs at least 2 samples per axis", entry, c, grid->dims[c]);
      return fail(NRF_E_SHAPE, msg);
    }
    cells *= (long long)(grid->dims[c] - 1);
    if (cells > NRF_MESH_MAX_CELLS) return mesh_shape(entry, "more than NRF_MESH_MAX_CELLS = 1 << 28 cells");
  }
  if (with_threshold && !std::isfinite(threshold)) return mesh_shape(entry, "threshold must be finite");
  return NRF_OK;
}

// the workspace rule of count and emit; a misaligned pointer is NRF_E_SHAPE to these two (mesh_host.h)
int grid_workspace(const char* entry, const MeshPlan& p, const void* workspace, size_t bytes) {
  return mesh_workspace(entry, "nrf_mesh_workspace_bytes", NRF_E_SHAPE, p.total, workspace, bytes);
}

}  // namespace

extern "C" {

int nrf_mesh_workspace_bytes(const nrf_grid* grid, size_t* bytes) {
  CK(mesh_args("nrf_mesh_workspace_bytes", grid, 0.f, false));
  if (!bytes) return mesh_null("nrf_mesh_workspace_bytes", "bytes");
  *bytes = mesh_plan(mesh_dims(grid)).total;
  return NRF_OK;
}

int nrf_mesh_count(const float* sigma, const nrf_grid* grid, float threshold, int32_t* counts, void* workspace, size_t workspace_bytes,
                   void* stream) {
  const char* entry = "nrf_mesh_count";
  if (!sigma) return mesh_null(entry, "sigma");
  CK(mesh_args(entry, grid, threshold, true));
  if (!counts) return mesh_null(entry, "counts");
  const MeshDims d = mesh_dims(grid);
  const MeshPlan p = mesh_plan(d);
  CK(grid_workspace(entry, p, workspace, workspace_bytes));
  char* ws = (char*)workspace;
  MESH_LAUNCH(mesh_classify_kernel, d.nblocks, MESH_THREADS, sigma, d, threshold, (unsigned char*)(ws + p.mask), (int*)(ws + p.block_v),
              (int*)(ws + p.block_q));
  MESH_LAUNCH(mesh_scan_kernel, 1, SCAN_THREADS, (int*)(ws + p.block_v), (int*)(ws + p.block_q), d.nblocks, (int*)ws, counts);
  return check_launch(entry);
}

int nrf_mesh_emit(const float* sigma, const nrf_grid* grid, float threshold, int32_t max_vertices, int32_t max_triangles, float* vertices,
                  int32_t* vertex_cell, int32_t* triangles, void* workspace, size_t workspace_bytes, void* stream) {
  const char* entry = "nrf_mesh_emit";
  if (!sigma) return mesh_null(entry, "sigma");
  CK(mesh_args(entry, grid, threshold, true));
  if (max_vertices < 0) return mesh_shape(entry, "max_vertices must not be negative");
  if (max_triangles < 0) return mesh_shape(entry, "max_triangles must not be negative");
  if (max_vertices > 0 && !vertices) return mesh_null(entry, "vertices");
  if (max_vertices > 0 && !vertex_cell) return mesh_null(entry, "vertex_cell");
  if (max_triangles > 0 && !triangles) return mesh_null(entry, "triangles");
  const MeshDims d = mesh_dims(grid);
  const MeshPlan p = mesh_plan(d);
  CK(grid_workspace(entry, p, workspace, workspace_bytes));
  char* ws = (char*)workspace;
  MESH_LAUNCH(mesh_vertices_kernel, d.nblocks, MESH_THREADS, sigma, d, *grid, threshold, (const unsigned char*)(ws + p.mask),
              (const int*)(ws + p.block_v), (int*)ws, max_vertices, max_triangles, vertices, vertex_cell, (int*)(ws + p.map));
  MESH_LAUNCH(mesh_faces_kernel, d.nblocks, MESH_THREADS, d, (const unsigned char*)(ws + p.mask), (const int*)(ws + p.map),
              (const int*)(ws + p.block_q), (const int*)ws, max_vertices, max_triangles, triangles);
  return check_launch(entry);
}

int nrf_mesh_snap(float* vertices, const int32_t* vertex_cell, const float* sigma_at, const float* grad_at, const nrf_grid* grid,
                  float threshold, int32_t num_vertices, void* stream) {
  const char* entry = "nrf_mesh_snap";
  CK(mesh_args(entry, grid, threshold, true));
  if (num_vertices < 0) return mesh_shape(entry, "num_vertices must not be negative");
  if (num_vertices == 0) return NRF_OK;   // an empty mesh: the buffers may be NULL
  if (!vertices) return mesh_null(entry, "vertices");
  if (!vertex_cell) return mesh_null(entry, "vertex_cell");
  if (!sigma_at) return mesh_null(entry, "sigma_at");
  if (!grad_at) return mesh_null(entry, "grad_at");
  const MeshDims d = mesh_dims(grid);
  MESH_LAUNCH(mesh_snap_kernel, blocks_of(num_vertices, MESH_THREADS), MESH_THREADS, vertices, vertex_cell, sigma_at, grad_at, *grid, d,
              threshold, num_vertices);
  return check_launch(entry);
}

}  // extern "C"
