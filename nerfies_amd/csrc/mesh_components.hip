// Mesh clean-up on the device (nrf_mesh_components / nrf_mesh_component_table / nrf_mesh_submesh_* / nrf_mesh_gather_rows; the
// definitions are in include/nerfies_amd.h): connected components of an indexed triangle mesh, their table, and the compaction of a
// mesh to the vertices a mask keeps.  Handle-free: any mesh, in any vertex and triangle order.
//
// Labelling is a union-find over `parent`, with the invariant parent[v] <= v and entries that only ever decrease: a root is the
// smallest vertex of its tree, so when the hooks are done the roots ARE the components' smallest vertices, and a component's id is
// its root's rank among the roots in vertex order.  Every walk strictly descends in index, so it ends within V steps whatever
// another workgroup does meanwhile; a failed compare-and-swap means the entry got smaller, and the retry continues from the value it
// returned with a strictly smaller pair of vertices.  No thread waits for another: every loop is bounded by V, holds a hard cap on
// top of that, and on overrun sets the status block's error word and leaves.
//
// Every output slot is a rank, by the rule of mesh_rank.h; the ranking kernels here say what is voted on (a vertex is a root, a vertex
// or triangle is kept) and what is written at the slot.  The only atomics on outputs are the table's integer adds and integer min /
// max, which do not depend on the order they arrive in.  The host half is built from mesh_host.h.
#include "mesh_host.h"
#include "mesh_rank.h"

using namespace nrf;
using namespace nrf::api;

namespace {

constexpr int ROUNDS = 4;
using Elems = MeshRank<ROUNDS>;   // the vertices (triangles) of the ranking kernels

// byte offsets of the components workspace
struct ComponentsPlan {
  size_t parent, block_roots, total;
  int nbv;
};

ComponentsPlan components_plan(int V) {
  ComponentsPlan p;
  MeshCarve c;
  p.nbv = (int)blocks_of(V, Elems::BLOCK);
  p.parent = c.take(sizeof(int) * (size_t)V);
  p.block_roots = c.take(sizeof(int) * (size_t)p.nbv);
  p.total = c.total;
  return p;
}

struct SubmeshPlan {
  size_t block_v, block_t, total;
  int nbv, nbt;
};

SubmeshPlan submesh_plan(int V, int F) {
  SubmeshPlan p;
  MeshCarve c;
  p.nbv = (int)blocks_of(V, Elems::BLOCK);
  p.nbt = (int)blocks_of(F, Elems::BLOCK);
  p.block_v = c.take(sizeof(int) * (size_t)p.nbv);
  p.block_t = c.take(sizeof(int) * (size_t)p.nbt);
  p.total = c.total;
  return p;
}

// an entry of `parent` another workgroup may have rewritten: served by L2, never by this CU's L1
__device__ __forceinline__ int load_parent(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ bool valid_triangle(const int a, const int b, const int c, const int V) {
  return a >= 0 && a < V && b >= 0 && b < V && c >= 0 && c < V;
}

// The root above x, halving the path on the way (an entry is only ever lowered, to an ancestor).  -1, and the error word, if the walk
// took more than `cap` steps: it descends strictly, so V steps cannot be passed.
__device__ int find_root(int* __restrict__ parent, int x, const int cap, int* __restrict__ status) {
  int p = load_parent(parent + x);
  for (int n = 0; p != x; ++n) {
    if (n >= cap) {
      atomicOr(status + 2, 1);
      return -1;
    }
    const int g = load_parent(parent + p);
    if (g != p) atomicMin(parent + x, g);
    x = p;
    p = g;
  }
  return x;
}

// joins the trees of a and b: the larger root is hooked under the smaller.  A retry's pair lies strictly below the root it lost.
__device__ void join(int* __restrict__ parent, int a, int b, const int cap, int* __restrict__ status) {
  for (int n = 0;; ++n) {
    if (n > cap) {
      atomicOr(status + 2, 2);
      return;
    }
    a = find_root(parent, a, cap, status);
    if (a < 0) return;
    b = find_root(parent, b, cap, status);
    if (b < 0 || a == b) return;
    const int hi = a > b ? a : b, lo = a > b ? b : a;
    const int old = atomicCAS(parent + hi, hi, lo);
    if (old == hi) return;
    a = old;   // hi was hooked meanwhile, under old < hi
    b = lo;
  }
}

__global__ __launch_bounds__(MESH_THREADS) void cc_init_kernel(int* __restrict__ parent, const int V, int* __restrict__ status) {
  const long long v = (long long)blockIdx.x * MESH_THREADS + threadIdx.x;
  if (v < V) parent[v] = (int)v;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    status[2] = 0;
    status[3] = 0;
  }
}

__global__ __launch_bounds__(MESH_THREADS) void cc_hook_kernel(const int* __restrict__ triangles, const int F, const int V,
                                                               int* __restrict__ parent, int* __restrict__ status) {
  const long long t = (long long)blockIdx.x * MESH_THREADS + threadIdx.x;
  if (t >= F) return;
  const int a = triangles[3 * (size_t)t + 0], b = triangles[3 * (size_t)t + 1], c = triangles[3 * (size_t)t + 2];
  if (!valid_triangle(a, b, c, V)) return;
  join(parent, a, b, V, status);
  join(parent, b, c, V, status);
}

// every vertex points at its root; per-workgroup totals of the roots
__global__ __launch_bounds__(MESH_THREADS) void cc_flatten_kernel(int* __restrict__ parent, const int V, int* __restrict__ block_roots,
                                                                  int* __restrict__ status) {
  __shared__ int sr[Elems::SLOTS];
#pragma unroll
  for (int r = 0; r < ROUNDS; ++r) {
    const long long v = Elems::owned(r);
    bool root = false;
    if (v < V) {
      const int top = find_root(parent, (int)v, V, status);
      root = top == (int)v;
      if (top >= 0 && !root) __hip_atomic_store(parent + v, top, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    Elems::vote(sr, r, root);
  }
  __syncthreads();
  if (threadIdx.x == 0) block_roots[blockIdx.x] = Elems::block_total(sr);
}

__global__ __launch_bounds__(SCAN_THREADS) void cc_scan_kernel(int* __restrict__ block_roots, const int nblocks, int* __restrict__ status,
                                                               int* __restrict__ counts) {
  int nc, unused;
  mesh_scan_totals(block_roots, nblocks, nullptr, 0, nc, unused);
  if (threadIdx.x == SCAN_THREADS - 1) {
    status[0] = nc;
    status[1] = 0;
    counts[0] = nc;
  }
}

// a root's id is its rank among the roots
__global__ __launch_bounds__(MESH_THREADS) void cc_label_roots_kernel(const int* __restrict__ parent, const int V,
                                                                      const int* __restrict__ block_roots, int* __restrict__ vertex_component) {
  __shared__ int sr[Elems::SLOTS];
  int rank[ROUNDS];
  bool roots[ROUNDS];
#pragma unroll
  for (int r = 0; r < ROUNDS; ++r) {
    const long long v = Elems::owned(r);
    roots[r] = v < V && parent[v] == (int)v;
    rank[r] = Elems::vote(sr, r, roots[r]);
  }
  __syncthreads();
  Elems::walk(sr, block_roots[blockIdx.x], [&](const int r, const int before) {
    if (roots[r]) vertex_component[Elems::owned(r)] = before + rank[r];
  });
}

__global__ __launch_bounds__(MESH_THREADS) void cc_label_rest_kernel(const int* __restrict__ parent, const int V, int* vertex_component) {
  const long long v = (long long)blockIdx.x * MESH_THREADS + threadIdx.x;
  if (v >= V) return;
  const int top = parent[v];
  if (top != (int)v && top >= 0 && top < V) vertex_component[v] = vertex_component[top];   // a root's entry is not written here
}

// The monotone key of a float: unsigned order of the keys = numeric order of the floats, with -0 below +0.
__device__ __forceinline__ unsigned float_key(const float x) {
  const unsigned u = __float_as_uint(x);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key_float(const unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k); }

constexpr unsigned KEY_PLUS_INF = 0xff800000u;    // float_key(+inf)
constexpr unsigned KEY_MINUS_INF = 0x007fffffu;   // float_key(-inf)

// zeroes the table's rows and seeds the boxes with (+inf, -inf) as keys; says what this table call writes
__global__ __launch_bounds__(MESH_THREADS) void table_init_kernel(int* __restrict__ status, const int max_components, int* __restrict__ comp_counts,
                                                                  unsigned* __restrict__ comp_bbox) {
  const int C = status[0];
  const bool fits = C <= max_components;
  const long long c = (long long)blockIdx.x * MESH_THREADS + threadIdx.x;
  if (fits && c < C) {
    comp_counts[2 * c + 0] = 0;
    comp_counts[2 * c + 1] = 0;
    if (comp_bbox) {
#pragma unroll
      for (int e = 0; e < 3; ++e) {
        comp_bbox[6 * c + e] = KEY_PLUS_INF;
        comp_bbox[6 * c + 3 + e] = KEY_MINUS_INF;
      }
    }
  }
  if (c == 0) status[1] = fits ? C : 0;
}

constexpr int TABLE_MAX_BLOCKS = 1024;   // of the accumulate kernel: bounds the atomics that meet on one component's row
constexpr int TABLE_PEEL = 4;            // distinct labels among a wave's 64 elements that are reduced in the wave; the rest go lane by lane

// a component's partial row; the wave that holds one holds it in every lane
struct RowAcc {
  int lab, nv, nt;
  unsigned lo[3], hi[3];   // keys; 0xffffffff and 0 are neutral (what a NaN coordinate contributes)
};

__device__ __forceinline__ void row_clear(RowAcc& a, const int lab) {
  a.lab = lab;
  a.nv = 0;
  a.nt = 0;
#pragma unroll
  for (int e = 0; e < 3; ++e) {
    a.lo[e] = 0xffffffffu;
    a.hi[e] = 0u;
  }
}

__device__ __forceinline__ void row_add(RowAcc& a, const RowAcc& b) {
  a.nv += b.nv;
  a.nt += b.nt;
#pragma unroll
  for (int e = 0; e < 3; ++e) {
    a.lo[e] = b.lo[e] < a.lo[e] ? b.lo[e] : a.lo[e];
    a.hi[e] = b.hi[e] > a.hi[e] ? b.hi[e] : a.hi[e];
  }
}

// ONE lane's atomics for a partial row: integer adds, integer min / max -- the order they arrive in plays no part
__device__ __forceinline__ void row_flush(const RowAcc& a, int* __restrict__ comp_counts, unsigned* __restrict__ comp_bbox) {
  if (a.lab < 0) return;
  if (a.nv != 0) atomicAdd(comp_counts + 2 * (size_t)a.lab, a.nv);
  if (a.nt != 0) atomicAdd(comp_counts + 2 * (size_t)a.lab + 1, a.nt);
  if (comp_bbox && a.nv != 0) {
#pragma unroll
    for (int e = 0; e < 3; ++e) {
      atomicMin(comp_bbox + 6 * (size_t)a.lab + e, a.lo[e]);
      atomicMax(comp_bbox + 6 * (size_t)a.lab + 3 + e, a.hi[e]);
    }
  }
}

// a wave's partial row of `members` elements into the row the wave holds.  Another component's part replaces the held row (which is
// flushed) only when it is the majority of the wave's elements; a minority goes straight to the table and the held row stays.
__device__ __forceinline__ void row_merge(RowAcc& held, const RowAcc& part, const int members, const int lane,
                                          int* __restrict__ comp_counts, unsigned* __restrict__ comp_bbox) {
  if (part.lab != held.lab) {
    if (held.lab >= 0 && members < 32) {
      if (lane == 0) row_flush(part, comp_counts, comp_bbox);
      return;
    }
    if (lane == 0) row_flush(held, comp_counts, comp_bbox);
    row_clear(held, part.lab);
  }
  row_add(held, part);
}

// Vertices into their component's vertex count and box, triangles into the triangle count of their first index's component.  A wave
// walks groups of 64 consecutive elements; in a group the lanes of one component are reduced in the wave (the first TABLE_PEEL
// components of the group; a mesh in surface-nets order has one or two), and the component the wave mostly sees is held in registers
// across groups, then merged over the workgroup: a large component costs a handful of atomics per workgroup, not one per vertex.
__global__ __launch_bounds__(MESH_THREADS) void table_accumulate_kernel(const int* __restrict__ triangles, const int F,
                                                                        const float* __restrict__ vertices, const int V,
                                                                        const int* __restrict__ vertex_component, const int* __restrict__ status,
                                                                        const int max_components, int* __restrict__ comp_counts,
                                                                        unsigned* __restrict__ comp_bbox) {
  __shared__ RowAcc shared[MESH_WAVES];
  const int C = status[0];
  if (C > max_components) return;   // uniform over the grid
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long n = V > F ? V : F;
  const long long stride = (long long)gridDim.x * MESH_THREADS;
  RowAcc held;
  row_clear(held, -1);
  for (long long base = (long long)blockIdx.x * MESH_THREADS + wave * 64; base < n; base += stride) {   // uniform over the wave
    const long long i = base + lane;
    RowAcc own;
    row_clear(own, -1);
    if (i < V) {
      const int lab = vertex_component[i];
      if (lab >= 0 && lab < C) {   // else not a label of this mesh: counted nowhere
        own.lab = lab;
        if (comp_bbox) {
#pragma unroll
          for (int e = 0; e < 3; ++e) {
            const float x = vertices[3 * (size_t)i + e];
            if (x == x) own.lo[e] = own.hi[e] = float_key(x);
          }
        }
      }
    }
    unsigned long long rest = __ballot(own.lab >= 0);
    for (int peel = 0; peel < TABLE_PEEL && rest != 0ull; ++peel) {
      RowAcc part;
      row_clear(part, __shfl(own.lab, __ffsll((long long)rest) - 1));
      const bool member = own.lab == part.lab;
      const unsigned long long members = __ballot(member);
      part.nv = __popcll(members);
      if (comp_bbox) {
#pragma unroll
        for (int e = 0; e < 3; ++e) {
          part.lo[e] = member ? own.lo[e] : 0xffffffffu;
          part.hi[e] = member ? own.hi[e] : 0u;
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
#pragma unroll
          for (int e = 0; e < 3; ++e) {
            const unsigned ol = (unsigned)__shfl_xor((int)part.lo[e], off), oh = (unsigned)__shfl_xor((int)part.hi[e], off);
            part.lo[e] = ol < part.lo[e] ? ol : part.lo[e];
            part.hi[e] = oh > part.hi[e] ? oh : part.hi[e];
          }
        }
      }
      row_merge(held, part, part.nv, lane, comp_counts, comp_bbox);
      rest &= ~members;
    }
    if ((rest >> lane) & 1ull) {   // a group with more components than are peeled: the remaining lanes one by one
      own.nv = 1;
      row_flush(own, comp_counts, comp_bbox);
    }
    int tlab = -1;
    if (i < F) {
      const int a = triangles[3 * (size_t)i + 0], b = triangles[3 * (size_t)i + 1], c = triangles[3 * (size_t)i + 2];
      if (valid_triangle(a, b, c, V)) {
        tlab = vertex_component[a];
        if (tlab < 0 || tlab >= C) tlab = -1;
      }
    }
    rest = __ballot(tlab >= 0);
    for (int peel = 0; peel < TABLE_PEEL && rest != 0ull; ++peel) {
      RowAcc part;
      row_clear(part, __shfl(tlab, __ffsll((long long)rest) - 1));
      const unsigned long long members = __ballot(tlab == part.lab);
      part.nt = __popcll(members);
      row_merge(held, part, part.nt, lane, comp_counts, comp_bbox);
      rest &= ~members;
    }
    if ((rest >> lane) & 1ull) atomicAdd(comp_counts + 2 * (size_t)tlab + 1, 1);
  }
  if (lane == 0) shared[wave] = held;
  __syncthreads();
  if (threadIdx.x == 0) {   // the waves' held rows, merged where they are one component's
    RowAcc run = shared[0];
    for (int w = 1; w < MESH_WAVES; ++w) {
      const RowAcc next = shared[w];
      if (next.lab == run.lab) {
        row_add(run, next);
      } else {
        row_flush(run, comp_counts, comp_bbox);
        run = next;
      }
    }
    row_flush(run, comp_counts, comp_bbox);
  }
}

// the boxes' keys back to floats, in place
__global__ __launch_bounds__(MESH_THREADS) void table_decode_kernel(const int* __restrict__ status, const int max_components,
                                                                    unsigned* __restrict__ comp_bbox) {
  const int C = status[0];
  const long long w = (long long)blockIdx.x * MESH_THREADS + threadIdx.x;
  if (C > max_components || w >= 6ll * C) return;
  comp_bbox[w] = __float_as_uint(key_float(comp_bbox[w]));
}

__global__ __launch_bounds__(MESH_THREADS) void submesh_count_vertices_kernel(const unsigned char* __restrict__ keep, const int V,
                                                                              int* __restrict__ block_v) {
  __shared__ int s[Elems::SLOTS];
#pragma unroll
  for (int r = 0; r < ROUNDS; ++r) {
    const long long v = Elems::owned(r);
    Elems::vote(s, r, v < V && keep[v] != 0);
  }
  __syncthreads();
  if (threadIdx.x == 0) block_v[blockIdx.x] = Elems::block_total(s);
}

__device__ __forceinline__ bool kept_triangle(const unsigned char* __restrict__ keep, const int* __restrict__ triangles, const long long t,
                                              const int F, const int V) {
  if (t >= F) return false;
  const int a = triangles[3 * (size_t)t + 0], b = triangles[3 * (size_t)t + 1], c = triangles[3 * (size_t)t + 2];
  return valid_triangle(a, b, c, V) && keep[a] != 0 && keep[b] != 0 && keep[c] != 0;
}

__global__ __launch_bounds__(MESH_THREADS) void submesh_count_triangles_kernel(const unsigned char* __restrict__ keep, const int V,
                                                                               const int* __restrict__ triangles, const int F,
                                                                               int* __restrict__ block_t) {
  __shared__ int s[Elems::SLOTS];
#pragma unroll
  for (int r = 0; r < ROUNDS; ++r) Elems::vote(s, r, kept_triangle(keep, triangles, Elems::owned(r), F, V));
  __syncthreads();
  if (threadIdx.x == 0) block_t[blockIdx.x] = Elems::block_total(s);
}

__global__ __launch_bounds__(SCAN_THREADS) void submesh_scan_kernel(int* __restrict__ block_v, const int nbv, int* __restrict__ block_t,
                                                                    const int nbt, int* __restrict__ status, int* __restrict__ counts) {
  int nv, nt;
  mesh_scan_totals(block_v, nbv, block_t, nbt, nv, nt);
  if (threadIdx.x == SCAN_THREADS - 1) {
    status[0] = nv;
    status[1] = nt;
    status[2] = 0;
    status[3] = 0;
    counts[0] = nv;
    counts[1] = nt;
  }
}

// vertex_map, when both capacities hold the scanned totals
__global__ __launch_bounds__(MESH_THREADS) void submesh_map_kernel(const unsigned char* __restrict__ keep, const int V,
                                                                   const int* __restrict__ block_v, int* __restrict__ status,
                                                                   const int max_vertices, const int max_triangles, int* __restrict__ vertex_map) {
  __shared__ int s[Elems::SLOTS];
  const bool fits = status[0] <= max_vertices && status[1] <= max_triangles;
  int rank[ROUNDS];
  bool kept[ROUNDS];
#pragma unroll
  for (int r = 0; r < ROUNDS; ++r) {
    const long long v = Elems::owned(r);
    kept[r] = v < V && keep[v] != 0;
    rank[r] = Elems::vote(s, r, kept[r]);
  }
  __syncthreads();
  if (blockIdx.x == 0 && threadIdx.x == 0) {   // what the caller reads back: all of the submesh, or none of it
    status[2] = fits ? status[0] : 0;
    status[3] = fits ? status[1] : 0;
  }
  if (!fits || V == 0) return;
  Elems::walk(s, block_v[blockIdx.x], [&](const int r, const int before) {
    const long long v = Elems::owned(r);
    if (v < V) vertex_map[v] = kept[r] ? before + rank[r] : -1;
  });
}

// the kept triangles, in their order, with mapped indices
__global__ __launch_bounds__(MESH_THREADS) void submesh_triangles_kernel(const unsigned char* __restrict__ keep, const int V,
                                                                         const int* __restrict__ triangles, const int F,
                                                                         const int* __restrict__ block_t, const int* __restrict__ status,
                                                                         const int max_vertices, const int max_triangles,
                                                                         const int* __restrict__ vertex_map, int* __restrict__ triangles_out) {
  __shared__ int s[Elems::SLOTS];
  if (!(status[0] <= max_vertices && status[1] <= max_triangles)) return;   // uniform over the grid
  int rank[ROUNDS];
  bool kept[ROUNDS];
#pragma unroll
  for (int r = 0; r < ROUNDS; ++r) {
    kept[r] = kept_triangle(keep, triangles, Elems::owned(r), F, V);
    rank[r] = Elems::vote(s, r, kept[r]);
  }
  __syncthreads();
  Elems::walk(s, block_t[blockIdx.x], [&](const int r, const int before) {
    const int slot = before + rank[r];
    if (!kept[r] || slot >= max_triangles) return;
    const int* in = triangles + 3 * (size_t)Elems::owned(r);
    int* o = triangles_out + 3 * (size_t)slot;
    o[0] = vertex_map[in[0]];
    o[1] = vertex_map[in[1]];
    o[2] = vertex_map[in[2]];
  });
}

// one thread per 4-byte word of src
__global__ __launch_bounds__(MESH_THREADS) void gather_rows_kernel(const unsigned* __restrict__ src, const int width,
                                                                   const int* __restrict__ vertex_map, const long long words,
                                                                   unsigned* __restrict__ dst, const int max_rows) {
  const long long i = (long long)blockIdx.x * MESH_THREADS + threadIdx.x;
  if (i >= words) return;
  const long long v = i / width;
  const int m = vertex_map[v];
  if (m >= 0 && m < max_rows) dst[(size_t)m * width + (size_t)(i - v * width)] = src[i];
}

// the mesh every entry is handed: counts and the pointers they make necessary
int mc_mesh(const char* entry, const int32_t* triangles, int32_t num_triangles, int32_t num_vertices) {
  if (num_vertices < 0) return mesh_shape(entry, "num_vertices must not be negative");
  if (num_triangles < 0) return mesh_shape(entry, "num_triangles must not be negative");
  if (num_triangles > 0 && !triangles) return mesh_null(entry, "triangles");
  return NRF_OK;
}

}  // namespace

extern "C" {

int nrf_mesh_components_workspace_bytes(int32_t num_vertices, int32_t num_triangles, size_t* bytes) {
  const char* entry = "nrf_mesh_components_workspace_bytes";
  if (num_vertices < 0) return mesh_shape(entry, "num_vertices must not be negative");
  if (num_triangles < 0) return mesh_shape(entry, "num_triangles must not be negative");
  if (!bytes) return mesh_null(entry, "bytes");
  *bytes = components_plan(num_vertices).total;
  return NRF_OK;
}

int nrf_mesh_components(const int32_t* triangles, int32_t num_triangles, int32_t num_vertices, int32_t* vertex_component, int32_t* counts,
                        void* workspace, size_t workspace_bytes, void* stream) {
  const char* entry = "nrf_mesh_components";
  CK(mc_mesh(entry, triangles, num_triangles, num_vertices));
  if (num_vertices > 0 && !vertex_component) return mesh_null(entry, "vertex_component");
  if (!counts) return mesh_null(entry, "counts");
  const int V = num_vertices, F = num_triangles;
  const ComponentsPlan p = components_plan(V);
  CK(mesh_workspace(entry, "nrf_mesh_components_workspace_bytes", NRF_E_WORKSPACE, p.total, workspace, workspace_bytes));
  char* ws = (char*)workspace;
  int* status = (int*)ws;
  int* parent = (int*)(ws + p.parent);
  int* block_roots = (int*)(ws + p.block_roots);
  const int per_thread = (int)blocks_of(V, MESH_THREADS);
  MESH_LAUNCH(cc_init_kernel, per_thread > 0 ? per_thread : 1, MESH_THREADS, parent, V, status);
  if (V > 0 && F > 0) MESH_LAUNCH(cc_hook_kernel, blocks_of(F, MESH_THREADS), MESH_THREADS, triangles, F, V, parent, status);
  if (V > 0) MESH_LAUNCH(cc_flatten_kernel, p.nbv, MESH_THREADS, parent, V, block_roots, status);
  MESH_LAUNCH(cc_scan_kernel, 1, SCAN_THREADS, block_roots, p.nbv, status, counts);
  if (V > 0) {
    MESH_LAUNCH(cc_label_roots_kernel, p.nbv, MESH_THREADS, (const int*)parent, V, (const int*)block_roots, vertex_component);
    MESH_LAUNCH(cc_label_rest_kernel, per_thread, MESH_THREADS, (const int*)parent, V, vertex_component);
  }
  return check_launch(entry);
}

int nrf_mesh_component_table(const int32_t* triangles, int32_t num_triangles, const float* vertices, int32_t num_vertices,
                             const int32_t* vertex_component, int32_t max_components, int32_t* comp_counts, float* comp_bbox,
                             void* workspace, size_t workspace_bytes, void* stream) {
  const char* entry = "nrf_mesh_component_table";
  CK(mc_mesh(entry, triangles, num_triangles, num_vertices));
  if (max_components < 0) return mesh_shape(entry, "max_components must not be negative");
  if (num_vertices > 0 && !vertex_component) return mesh_null(entry, "vertex_component");
  if (max_components > 0 && !comp_counts) return mesh_null(entry, "comp_counts");
  if (comp_bbox && num_vertices > 0 && !vertices) return mesh_null(entry, "vertices (comp_bbox is given)");
  if (vertices && max_components > 0 && !comp_bbox) return mesh_null(entry, "comp_bbox (vertices are given)");
  const int V = num_vertices, F = num_triangles;
  const ComponentsPlan p = components_plan(V);
  CK(mesh_workspace(entry, "nrf_mesh_components_workspace_bytes", NRF_E_WORKSPACE, p.total, workspace, workspace_bytes));
  int* status = (int*)workspace;
  unsigned* box = vertices ? (unsigned*)comp_bbox : nullptr;
  const int cblocks = (int)blocks_of(max_components, MESH_THREADS);
  MESH_LAUNCH(table_init_kernel, cblocks > 0 ? cblocks : 1, MESH_THREADS, status, max_components, comp_counts, box);
  const long long nblocks = blocks_of(V > F ? V : F, MESH_THREADS);
  if (nblocks > 0 && max_components > 0)
    MESH_LAUNCH(table_accumulate_kernel, nblocks < TABLE_MAX_BLOCKS ? nblocks : TABLE_MAX_BLOCKS, MESH_THREADS, triangles, F, vertices, V,
                vertex_component, (const int*)status, max_components, comp_counts, box);
  if (box && max_components > 0)
    MESH_LAUNCH(table_decode_kernel, blocks_of(6ll * max_components, MESH_THREADS), MESH_THREADS, (const int*)status, max_components, box);
  return check_launch(entry);
}

int nrf_mesh_submesh_workspace_bytes(int32_t num_vertices, int32_t num_triangles, size_t* bytes) {
  const char* entry = "nrf_mesh_submesh_workspace_bytes";
  if (num_vertices < 0) return mesh_shape(entry, "num_vertices must not be negative");
  if (num_triangles < 0) return mesh_shape(entry, "num_triangles must not be negative");
  if (!bytes) return mesh_null(entry, "bytes");
  *bytes = submesh_plan(num_vertices, num_triangles).total;
  return NRF_OK;
}

int nrf_mesh_submesh_count(const uint8_t* keep, int32_t num_vertices, const int32_t* triangles, int32_t num_triangles, int32_t* counts,
                           void* workspace, size_t workspace_bytes, void* stream) {
  const char* entry = "nrf_mesh_submesh_count";
  CK(mc_mesh(entry, triangles, num_triangles, num_vertices));
  if (num_vertices > 0 && !keep) return mesh_null(entry, "keep");
  if (!counts) return mesh_null(entry, "counts");
  const int V = num_vertices, F = num_triangles;
  const SubmeshPlan p = submesh_plan(V, F);
  CK(mesh_workspace(entry, "nrf_mesh_submesh_workspace_bytes", NRF_E_WORKSPACE, p.total, workspace, workspace_bytes));
  char* ws = (char*)workspace;
  int* block_v = (int*)(ws + p.block_v);
  int* block_t = (int*)(ws + p.block_t);
  if (V > 0) MESH_LAUNCH(submesh_count_vertices_kernel, p.nbv, MESH_THREADS, keep, V, block_v);
  if (F > 0) MESH_LAUNCH(submesh_count_triangles_kernel, p.nbt, MESH_THREADS, keep, V, triangles, F, block_t);
  MESH_LAUNCH(submesh_scan_kernel, 1, SCAN_THREADS, block_v, p.nbv, block_t, p.nbt, (int*)ws, counts);
  return check_launch(entry);
}

int nrf_mesh_submesh_emit(const uint8_t* keep, int32_t num_vertices, const int32_t* triangles, int32_t num_triangles, int32_t max_vertices,
                          int32_t max_triangles, int32_t* vertex_map, int32_t* triangles_out, void* workspace, size_t workspace_bytes,
                          void* stream) {
  const char* entry = "nrf_mesh_submesh_emit";
  CK(mc_mesh(entry, triangles, num_triangles, num_vertices));
  if (max_vertices < 0) return mesh_shape(entry, "max_vertices must not be negative");
  if (max_triangles < 0) return mesh_shape(entry, "max_triangles must not be negative");
  if (num_vertices > 0 && !keep) return mesh_null(entry, "keep");
  if (num_vertices > 0 && !vertex_map) return mesh_null(entry, "vertex_map");
  if (max_triangles > 0 && !triangles_out) return mesh_null(entry, "triangles_out");
  const int V = num_vertices, F = num_triangles;
  const SubmeshPlan p = submesh_plan(V, F);
  CK(mesh_workspace(entry, "nrf_mesh_submesh_workspace_bytes", NRF_E_WORKSPACE, p.total, workspace, workspace_bytes));
  char* ws = (char*)workspace;
  MESH_LAUNCH(submesh_map_kernel, p.nbv > 0 ? p.nbv : 1, MESH_THREADS, keep, V, (const int*)(ws + p.block_v), (int*)ws, max_vertices,
            max_triangles, vertex_map);
  if (F > 0 && V > 0 && max_triangles > 0)
    MESH_LAUNCH(submesh_triangles_kernel, p.nbt, MESH_THREADS, keep, V, triangles, F, (const int*)(ws + p.block_t), (const int*)ws, max_vertices,
              max_triangles, (const int*)vertex_map, triangles_out);
  return check_launch(entry);
}

int nrf_mesh_gather_rows(const void* src, int32_t width, const int32_t* vertex_map, int32_t num_vertices, void* dst, int32_t max_rows,
                         void* stream) {
  const char* entry = "nrf_mesh_gather_rows";
  char msg[200];
  if (num_vertices < 0) return mesh_shape(entry, "num_vertices must not be negative");
  if (max_rows < 0) return mesh_shape(entry, "max_rows must not be negative");
  if (width < 1) {
    snprintf(msg, sizeof(msg), "%s: width = %d: a row has at least one 4-byte word", entry, width);
    return fail(NRF_E_SHAPE, msg);
  }
  const long long words = (long long)num_vertices * width;
  const long long blocks = blocks_of(words, MESH_THREADS);
  if (blocks > 0x7fffffffll) {
    snprintf(msg, sizeof(msg), "%s: num_vertices * width is more than 2^31 - 1 workgroups of %d words", entry, MESH_THREADS);
    return fail(NRF_E_SHAPE, msg);
  }
  if (num_vertices == 0 || max_rows == 0) return NRF_OK;   // nothing to copy: the buffers may be NULL
  if (!src) return mesh_null(entry, "src");
  if (!vertex_map) return mesh_null(entry, "vertex_map");
  if (!dst) return mesh_null(entry, "dst");
  MESH_LAUNCH(gather_rows_kernel, blocks, MESH_THREADS, (const unsigned*)src, width, vertex_map, words, (unsigned*)dst, max_rows);
  return check_launch(entry);
}

}  // extern "C"
