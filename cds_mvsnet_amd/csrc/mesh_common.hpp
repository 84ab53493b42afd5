// What the mesh kernels share (mesh_clean.hip, mesh_simplify.hip, mesh_smooth.hip, mesh_sample.hip, raster.hip, mesh_texture.hip;
// DESIGN §1.10-1.15, §1.17): the launch shape, the size and finiteness tests, the face loader, the rasteriser's rule 1, and the one
// compaction behind cds_mesh_cc_gather and cds_mesh_simplify_gather.
#pragma once
#include "cds_common.hpp"

namespace cds_mesh {

constexpr int kThreads = 256;                                            // the workgroup of every mesh kernel
constexpr double kHuge = 1.7976931348623157e308;

inline unsigned blocks_for(long long n) { return (unsigned)((n + kThreads - 1) / kThreads); }

// Two counts that an int32 index can address.
inline bool sizes_ok(long long n_a, long long n_b) { return n_a >= 0 && n_a <= 0x7fffffffLL && n_b >= 0 && n_b <= 0x7fffffffLL; }

__host__ __device__ __forceinline__ bool finite_pos(double x) { return x > 0.0 && x <= kHuge; }      // false for a NaN
__device__ __forceinline__ bool is_finite(double x) { return fabs(x) <= kHuge; }                      // false for a NaN

// The three indices of a face; false for a face with an index outside the vertices, which every kernel skips.
__device__ __forceinline__ bool load_face(const int* __restrict__ faces, long long face, long long n_vertices, int idx[3]) {
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    idx[k] = faces[3 * face + k];
    ok = ok && (unsigned long long)(long long)idx[k] < (unsigned long long)n_vertices;
  }
  return ok;
}

// Rule 1 of the rasteriser (include/cds_mvsnet_hip.h, "Rendering a triangle mesh"), stated once for raster.hip and
// mesh_texture.hip.  c: the CDS_RASTER_CAM doubles of one view; X: a world point.  -> the camera-space point and the pixel
// coordinates, bracketed as the rule writes them.
struct ViewPoint {
  double xc0, xc1, z, u, v;
};

__device__ __forceinline__ ViewPoint view_point(const double* __restrict__ c, double X0, double X1, double X2) {
  ViewPoint p;
  p.xc0 = ((c[0] * X0 + c[1] * X1) + c[2] * X2) + c[9];
  p.xc1 = ((c[3] * X0 + c[4] * X1) + c[5] * X2) + c[10];
  p.z = ((c[6] * X0 + c[7] * X1) + c[8] * X2) + c[11];
  p.u = ((c[12] * p.xc0 + c[13] * p.xc1) + c[14] * p.z) / p.z;
  p.v = (c[15] * p.xc1 + c[16] * p.z) / p.z;
  return p;
}

constexpr int kUnusable = INT_MIN;                                       // X and Y of a vertex that rule 1 rejects
constexpr long long kSnapLimit = 1ll << 28;

// The snapped coordinates of rule 1; false, and both kUnusable, for a vertex that is not usable.
__device__ __forceinline__ bool snap_point(const ViewPoint& p, int& X, int& Y) {
  const double sx = floor(p.u * 256.0 + 0.5), sy = floor(p.v * 256.0 + 0.5);
  // an infinite or NaN u fails |X| < 2^28 as well: u 256 + 0.5 keeps it
  const bool usable = p.z > 0.0 && fabs(p.u) <= kHuge && fabs(p.v) <= kHuge && fabs(sx) < (double)kSnapLimit &&
                      fabs(sy) < (double)kSnapLimit;
  X = usable ? (int)sx : kUnusable;
  Y = usable ? (int)sy : kUnusable;
  return usable;
}

}  // namespace cds_mesh

// mesh_clean.hip: the kept vertex rows at vertex_new, the bits and not the value, and the kept faces at face_new, renumbered
// through vertex_new; a face with an index outside the vertices is skipped.  *_new: the exclusive prefix sums of the keep flags.
// colors: three bytes per row, or with `packed` the words of cds_voxel_merge_f32 (r | g << 8 | b << 16); may be null.  The
// argument checks of the two entry points are here: CDS_EINVAL, and 0 before any pointer is looked at when out_vertices == 0.
int cds_mesh_compact_dispatch(const float* vertices, const void* colors, bool packed, const int* faces, long long n_vertices,
                              long long n_faces, const unsigned char* vertex_keep, const int* vertex_new,
                              const unsigned char* face_keep, const int* face_new, long long out_vertices, long long out_faces,
                              float* vertices_out, unsigned char* colors_out, int* faces_out, void* stream);
