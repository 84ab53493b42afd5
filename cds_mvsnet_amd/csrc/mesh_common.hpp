// What the mesh kernels share (mesh_clean.hip, mesh_simplify.hip, mesh_smooth.hip, mesh_sample.hip, raster.hip, mesh_texture.hip,
// photo.hip): the launch shape, the size and finiteness tests, the face loader, the rasteriser's
// rules 1, 4 and 6 for one point, and the one compaction behind cds_mesh_cc_gather and cds_mesh_simplify_gather.
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

// Rules 4 and 6 of the rasteriser, stated once for raster.hip and photo.hip: the plane of a face in camera space, the depth of a
// pixel's ray on it and the weights of the three corners at that point.
struct FacePlane {
  double n[3], d;
};

__device__ __forceinline__ void load_point(const double* __restrict__ xc, int v, double p[3]) {
  p[0] = xc[3 * (long long)v]; p[1] = xc[3 * (long long)v + 1]; p[2] = xc[3 * (long long)v + 2];
}

__device__ __forceinline__ FacePlane face_plane(const double a[3], const double b[3], const double c[3]) {
  const double e1[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]}, e2[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
  FacePlane f;
  f.n[0] = e1[1] * e2[2] - e1[2] * e2[1];
  f.n[1] = e1[2] * e2[0] - e1[0] * e2[2];
  f.n[2] = e1[0] * e2[1] - e1[1] * e2[0];
  f.d = (f.n[0] * a[0] + f.n[1] * a[1]) + f.n[2] * a[2];
  return f;
}

// Rule 4 for one pixel: the ray (rx, ry, 1) and the depth along it.  The fragment exists iff the result is finite and > 0.
__device__ __forceinline__ double fragment_depth(const FacePlane& f, const double* __restrict__ cam, int px, int py, double& rx,
                                                 double& ry) {
  ry = (((double)py + 0.5) - cam[16]) / cam[15];
  rx = ((((double)px + 0.5) - cam[14]) - cam[13] * ry) / cam[12];
  const double den = (f.n[0] * rx + f.n[1] * ry) + f.n[2];
  return f.d / den;
}

__device__ __forceinline__ bool fragment_exists(double zf) { return zf > 0.0 && zf <= kHuge; }

// Rule 6: the weights of the corners a, b, c (camera space) at the surface point zf (rx, ry, 1).
__device__ __forceinline__ void surface_weights(const FacePlane& f, const double a[3], const double b[3], const double c[3],
                                                double zf, double rx, double ry, double wt[3]) {
  const double P[3] = {zf * rx, zf * ry, zf};
  const double pa[3] = {a[0] - P[0], a[1] - P[1], a[2] - P[2]}, pb[3] = {b[0] - P[0], b[1] - P[1], b[2] - P[2]},
               pc[3] = {c[0] - P[0], c[1] - P[1], c[2] - P[2]};
  const double nn = (f.n[0] * f.n[0] + f.n[1] * f.n[1]) + f.n[2] * f.n[2];
  const double* q[4] = {pb, pc, pa, pb};                               // w_a from (b, c), w_b from (c, a), w_c from (a, b)
  for (int k = 0; k < 3; ++k) {
    const double* s = q[k];
    const double* t = q[k + 1];
    const double c0 = s[1] * t[2] - s[2] * t[1], c1 = s[2] * t[0] - s[0] * t[2], c2 = s[0] * t[1] - s[1] * t[0];
    wt[k] = ((f.n[0] * c0 + f.n[1] * c1) + f.n[2] * c2) / nn;
  }
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
