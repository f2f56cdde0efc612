// What the host halves of the mesh entries share (mesh.hip, mesh_components.hip, mesh_raster.hip): the refusals every entry words
// the same way, the workspace rule, the carving of a workspace behind its status header, and the launch.
#pragma once

#include "nrf_handle.h"

namespace nrf {
namespace api {

constexpr size_t MESH_HEADER_BYTES = 256;   // the status block of a workspace, padded
constexpr size_t MESH_ALIGN = 256;          // of every region behind it

inline int mesh_null(const char* entry, const char* name) {
  char msg[200];
  snprintf(msg, sizeof(msg), "%s: %s is null", entry, name);
  return fail(NRF_E_NULL, msg);
}

inline int mesh_shape(const char* entry, const char* what) {
  char msg[200];
  snprintf(msg, sizeof(msg), "%s: %s", entry, what);
  return fail(NRF_E_SHAPE, msg);
}

// workgroups of `per` elements that cover n.  Where n came in as an int32 count the quotient fits an int, and the plans narrow it.
inline long long blocks_of(long long n, int per) { return (n + per - 1) / per; }

// byte offsets of a workspace's regions, in the order they are taken
struct MeshCarve {
  size_t total = MESH_HEADER_BYTES;
  size_t take(size_t bytes) {
    const size_t at = total;
    total = align_up(total + bytes, MESH_ALIGN);
    return at;
  }
};

// The workspace an entry is handed, against the `need` bytes of its plan; `sizer` is the entry that reports them.  A misaligned
// pointer is NRF_E_SHAPE to the surface-net entries and NRF_E_WORKSPACE to the components and raster entries: both are in the ABI,
// so the caller says which.
inline int mesh_workspace(const char* entry, const char* sizer, int misaligned, size_t need, const void* workspace, size_t bytes) {
  char msg[200];
  if (!workspace) return mesh_null(entry, "workspace");
  if (((uintptr_t)workspace & 15u) != 0) {
    snprintf(msg, sizeof(msg), "%s: workspace must be 16-byte aligned", entry);
    return fail(misaligned, msg);
  }
  if (bytes < need) {
    snprintf(msg, sizeof(msg), "%s: workspace too small (see %s)", entry, sizer);
    return fail(NRF_E_WORKSPACE, msg);
  }
  return NRF_OK;
}

// on the `stream` the entry was handed
#define MESH_LAUNCH(kernel, blocks, threads, ...) \
  hipLaunchKernelGGL(kernel, dim3((unsigned)(blocks)), dim3(threads), 0, (hipStream_t)stream, __VA_ARGS__)

}  // namespace api
}  // namespace nrf
