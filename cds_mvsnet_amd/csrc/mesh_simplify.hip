// Vertex clustering with quadric placement (the rule is stated in include/cds_mvsnet_hip.h): the vertices of a cell
// of side `cell` (the cells of --merge_voxel: pointcloud.voxel_groups) become one vertex, the faces are rewritten to the clusters,
// and the faces that collapse or repeat are dropped.  The cells, the sorts and the prefix sums are the caller's (torch); the mean
// position and the colour of a cluster come from cds_voxel_merge_f32 (cloud.hip).
//
//   cds_mesh_simplify_faces        one thread per face: its three clusters, the collapsed flag, the identity (the triple rotated so
//                                  that the smallest cluster comes first)
//   cds_mesh_simplify_quadric_f32  one thread per cluster: the fp64 mean of its members, the nine sums of rule 3 over its incidences
//                                  in ascending (face, corner) order, the regularised solve of rule 4
//   cds_mesh_simplify_mark         one thread per face: the keep flag of the three clusters of a surviving face
//   cds_mesh_simplify_gather       one thread per cluster and per face: the kept clusters' rows and the renumbered faces; it is
//                                  the compaction of cds_mesh_cc_gather (cds_mesh_compact_dispatch, mesh_common.hpp) with the
//                                  clusters as vertices and packed colours, and has no kernel here
//
// Nothing here depends on an order the hardware chooses: the sums of a cluster are one thread's serial chain in the order the
// rule gives, mark stores the same byte from every writer, and the other kernels write each word once.  No float atomics.
// The library is built with -ffp-contract=off, so every fp64 product and sum below is rounded as written.
#include "mesh_common.hpp"

namespace {

using namespace cds_mesh;

// A face outside the vertices, or one whose vertex has a cluster outside [0, n_clusters), is written as collapsed with the
// clusters -1: nothing later reads a row through it.
__global__ __launch_bounds__(kThreads) void faces_kernel(const int* __restrict__ faces, long long n_faces, long long n_vertices,
                                                         const int* __restrict__ cluster, long long n_clusters,
                                                         int* __restrict__ face_clusters, unsigned char* __restrict__ collapsed,
                                                         int* __restrict__ identity) {
  const long long face = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (face >= n_faces) return;
  int idx[3], c[3] = {-1, -1, -1};
  bool ok = load_face(faces, face, n_vertices, idx);
  if (ok) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      c[k] = cluster[idx[k]];
      ok = ok && (unsigned long long)(long long)c[k] < (unsigned long long)n_clusters;
    }
  }
  if (!ok) c[0] = c[1] = c[2] = -1;
  const bool gone = !ok || c[0] == c[1] || c[1] == c[2] || c[0] == c[2];
  int first = 0;                                                         // the corner of the smallest cluster
  if (c[1] < c[first]) first = 1;
  if (c[2] < c[first]) first = 2;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    face_clusters[3 * face + k] = c[k];
    identity[3 * face + k] = c[(first + k) % 3];
  }
  collapsed[face] = gone ? 1 : 0;
}

// Cluster c holds the vertices perm[start[c] .. start[c + 1]) and the corners inc[inc_start[c] .. inc_start[c + 1]), a corner
// being 3 face + j.  The mean repeats the loop, guards and fp64 expressions of voxel_merge_kernel (cloud.hip), so fp32(m) is that
// kernel's position bit for bit.
__global__ __launch_bounds__(kThreads) void quadric_kernel(const float* __restrict__ vertices, long long n_vertices,
                                                           const int* __restrict__ faces, long long n_faces,
                                                           const long long* __restrict__ perm, const int* __restrict__ start,
                                                           const long long* __restrict__ inc, const int* __restrict__ inc_start,
                                                           long long n_clusters, double cell, float* __restrict__ out_positions,
                                                           unsigned char* __restrict__ out_fallback) {
  const long long c = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (c >= n_clusters) return;
  double sx = 0.0, sy = 0.0, sz = 0.0;
  int cnt = 0;
  for (int j = start[c], e = start[c + 1]; j < e; ++j) {
    if (j < 0 || j >= n_vertices) continue;                              // offsets outside the permutation: read nothing
    const long long i = perm[j];
    if (i < 0 || i >= n_vertices) continue;
    sx += (double)vertices[3 * i];
    sy += (double)vertices[3 * i + 1];
    sz += (double)vertices[3 * i + 2];
    ++cnt;
  }
  const double k = (double)cnt;
  const double mx = sx / k, my = sy / k, mz = sz / k;

  double a00 = 0.0, a01 = 0.0, a02 = 0.0, a11 = 0.0, a12 = 0.0, a22 = 0.0, b0 = 0.0, b1 = 0.0, b2 = 0.0;
  const long long n_corners = 3 * n_faces;
  for (int j = inc_start[c], e = inc_start[c + 1]; j < e; ++j) {
    if (j < 0 || j >= n_corners) continue;
    const long long corner = inc[j];
    if (corner < 0 || corner >= n_corners) continue;
    int idx[3];
    if (!load_face(faces, corner / 3, n_vertices, idx)) continue;
    const double p0x = (double)vertices[3 * (long long)idx[0]], p0y = (double)vertices[3 * (long long)idx[0] + 1],
                 p0z = (double)vertices[3 * (long long)idx[0] + 2];
    const double e1x = (double)vertices[3 * (long long)idx[1]] - p0x, e1y = (double)vertices[3 * (long long)idx[1] + 1] - p0y,
                 e1z = (double)vertices[3 * (long long)idx[1] + 2] - p0z;
    const double e2x = (double)vertices[3 * (long long)idx[2]] - p0x, e2y = (double)vertices[3 * (long long)idx[2] + 1] - p0y,
                 e2z = (double)vertices[3 * (long long)idx[2] + 2] - p0z;
    const double nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
    const double w2 = (nx * nx + ny * ny) + nz * nz;
    if (!finite_pos(w2)) continue;                                       // zero area, or not finite: contributes nothing
    const double qx = p0x - mx, qy = p0y - my, qz = p0z - mz;
    const double d = (nx * qx + ny * qy) + nz * qz;
    a00 += nx * nx; a01 += nx * ny; a02 += nx * nz; a11 += ny * ny; a12 += ny * nz; a22 += nz * nz;
    b0 += nx * d; b1 += ny * d; b2 += nz * d;
  }

  const double tr = (a00 + a11) + a22;
  const double lam = tr * 0.0009765625;                                  // 2^-10: exact
  const double m00 = a00 + lam, m11 = a11 + lam, m22 = a22 + lam;
  const double c00 = m11 * m22 - a12 * a12, c01 = a02 * a12 - a01 * m22, c02 = a01 * a12 - a02 * m11;
  const double c11 = m00 * m22 - a02 * a02, c12 = a01 * a02 - m00 * a12, c22 = m00 * m11 - a01 * a01;
  const double det = (m00 * c00 + a01 * c01) + a02 * c02;
  const double y0 = ((c00 * b0 + c01 * b1) + c02 * b2) / det;
  const double y1 = ((c01 * b0 + c11 * b1) + c12 * b2) / det;
  const double y2 = ((c02 * b0 + c12 * b1) + c22 * b2) / det;
  const bool solved = finite_pos(tr) && finite_pos(det) && is_finite(y0) && is_finite(y1) && is_finite(y2) &&
                      fmax(fmax(fabs(y0), fabs(y1)), fabs(y2)) <= cell;
  out_positions[3 * c] = (float)(solved ? mx + y0 : mx);
  out_positions[3 * c + 1] = (float)(solved ? my + y1 : my);
  out_positions[3 * c + 2] = (float)(solved ? mz + y2 : mz);
  out_fallback[c] = solved ? 0 : 1;
}

__global__ __launch_bounds__(kThreads) void mark_kernel(const int* __restrict__ face_clusters,
                                                        const unsigned char* __restrict__ face_keep, long long n_faces,
                                                        long long n_clusters, unsigned char* cluster_keep) {
  const long long face = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (face >= n_faces || !face_keep[face]) return;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int c = face_clusters[3 * face + k];
    if ((unsigned long long)(long long)c < (unsigned long long)n_clusters) cluster_keep[c] = 1;   // every writer stores the same byte
  }
}

}  // namespace

extern "C" int cds_mesh_simplify_faces(const int* faces, long long n_faces, long long n_vertices, const int* cluster,
                                       long long n_clusters, int* face_clusters, unsigned char* collapsed, int* identity,
                                       void* stream) {
  if (!sizes_ok(n_vertices, n_faces) || n_clusters < 0 || n_clusters > n_vertices) return CDS_EINVAL;
  if (n_faces == 0) return 0;
  if (!faces || !face_clusters || !collapsed || !identity || (n_vertices > 0 && !cluster)) return CDS_EINVAL;
  hipLaunchKernelGGL(faces_kernel, dim3(blocks_for(n_faces)), dim3(kThreads), 0, (hipStream_t)stream, faces, n_faces, n_vertices,
                     cluster, n_clusters, face_clusters, collapsed, identity);
  return cds_launch_status();
}

extern "C" int cds_mesh_simplify_quadric_f32(const float* vertices, long long n_vertices, const int* faces, long long n_faces,
                                             const long long* perm, const int* start, const long long* inc, const int* inc_start,
                                             long long n_clusters, float cell, float* out_positions,
                                             unsigned char* out_fallback, void* stream) {
  if (!sizes_ok(n_vertices, n_faces) || 3 * n_faces > 0x7fffffffLL || n_clusters < 0 || n_clusters > n_vertices ||
      !(cell > 0.f && cell <= 3.402823466e+38f))
    return CDS_EINVAL;
  if (n_clusters == 0) return 0;
  if (!vertices || !perm || !start || !inc_start || !out_positions || !out_fallback || (n_faces > 0 && (!faces || !inc)))
    return CDS_EINVAL;
  hipLaunchKernelGGL(quadric_kernel, dim3(blocks_for(n_clusters)), dim3(kThreads), 0, (hipStream_t)stream, vertices, n_vertices,
                     faces, n_faces, perm, start, inc, inc_start, n_clusters, (double)cell, out_positions, out_fallback);
  return cds_launch_status();
}

extern "C" int cds_mesh_simplify_mark(const int* face_clusters, const unsigned char* face_keep, long long n_faces,
                                      long long n_clusters, unsigned char* cluster_keep, void* stream) {
  if (!sizes_ok(n_clusters, n_faces)) return CDS_EINVAL;
  if (n_faces == 0 || n_clusters == 0) return 0;
  if (!face_clusters || !face_keep || !cluster_keep) return CDS_EINVAL;
  hipLaunchKernelGGL(mark_kernel, dim3(blocks_for(n_faces)), dim3(kThreads), 0, (hipStream_t)stream, face_clusters, face_keep,
                     n_faces, n_clusters, cluster_keep);
  return cds_launch_status();
}

extern "C" int cds_mesh_simplify_gather(const float* positions, const unsigned* colors, long long n_clusters,
                                        const unsigned char* cluster_keep, const int* cluster_new, const int* face_clusters,
                                        long long n_faces, const unsigned char* face_keep, const int* face_new,
                                        long long out_vertices, long long out_faces, float* vertices_out,
                                        unsigned char* colors_out, int* faces_out, void* stream) {
  return cds_mesh_compact_dispatch(positions, colors, true, face_clusters, n_clusters, n_faces, cluster_keep, cluster_new, face_keep,
                                   face_new, out_vertices, out_faces, vertices_out, colors_out, faces_out, stream);
}
