// Point-cloud registration and preparation kernels of the Tanks and Temples F-score (cds_mvsnet_amd/tt_eval.py).
// They restate what the public evaluation toolbox does with Open3D on the host, over the sparse grid of pointcloud.hip:
//
//   cds_transform_points_f32   p = fp32(T x): a 3x4 float64 transform applied in float64, rounded once
//   cds_nn_index_f32           capped nearest neighbour with the index of the nearest target point (grid_walk with the NearestIndex sink)
//   cds_icp_sums_f64           one registration step: transform, nearest neighbour and the 18 pair sums of the Umeyama update
//   cds_voxel_mean_f32         voxel_down_sample: the mean of the points of each occupied voxel
//   cds_polygon_crop_f32       SelectionPolygonVolume: axis range and even-odd polygon test in float64
//
// 256-thread workgroups; the sums are fp64 in a fixed order (per-workgroup records, reduced by a second pass whose shape depends
// on the point count only), no atomics on floating-point data - bit-reproducible run to run, as in depth_metrics.hip / loss.hip.
#include "feat_common.hpp"
#include "grid_common.hpp"

namespace {

constexpr int ICP_NF = CDS_ICP_SUMS;
constexpr int ICP_MAX_GROUPS = CDS_ICP_MAX_GROUPS;

// row r of the 3x4 transform applied to (x, y, z): each product and each sum rounded separately (the library is built without
// contraction), the result rounded once to fp32
__device__ __forceinline__ float transform_row(const double* __restrict__ T, int r, double x, double y, double z) {
  return (float)(((T[4 * r] * x + T[4 * r + 1] * y) + T[4 * r + 2] * z) + T[4 * r + 3]);
}

__global__ __launch_bounds__(256) void transform_points_kernel(const float* __restrict__ pts, long long n,
                                                               const double* __restrict__ T, float* __restrict__ out) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const double x = (double)pts[3 * i], y = (double)pts[3 * i + 1], z = (double)pts[3 * i + 2];
    out[3 * i] = transform_row(T, 0, x, y, z);
    out[3 * i + 1] = transform_row(T, 1, x, y, z);
    out[3 * i + 2] = transform_row(T, 2, x, y, z);
  }
}

__global__ __launch_bounds__(256) void nn_index_kernel(const float* __restrict__ query, const long long* __restrict__ order,
                                                       long long m, GridView g, float cap, float* __restrict__ dist,
                                                       int* __restrict__ index) {
  const float cap2 = cap * cap;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (long long)gridDim.x * blockDim.x) {
    const long long qi = order ? order[i] : i;
    NearestIndex n{cap2, cap2, 0x7fffffff, -1};
    grid_walk(g, query[3 * qi], query[3 * qi + 1], query[3 * qi + 2], n);
    const bool hit = n.d2 < cap2;
    dist[qi] = hit ? fminf(sqrtf(n.d2), cap) : cap;
    index[qi] = hit ? n.index : -1;
  }
}

// sum of v over the workgroup (256 threads), valid in every thread
__device__ __forceinline__ double icp_block_sum(double v, double* red) {
  v = wave_sum_f64(v);
  __syncthreads();                       // red may still be read from the previous call
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

// Pass 1.  Workgroup g of `groups` strides over the source points and writes record [g][18]: count, sum p (3), sum q (3),
// sum q p^T (9, row-major: q row, p column), sum |p - q|^2, sum |p|^2 (the source variance of the scale estimate needs it),
// over the accepted pairs; p = fp32(T s), q its nearest target point.
__global__ __launch_bounds__(256) void icp_sums_kernel(const float* __restrict__ src, const long long* __restrict__ order,
                                                       long long m, const double* __restrict__ T, GridView g, float cap,
                                                       double* __restrict__ rec, int* __restrict__ index,
                                                       float* __restrict__ dist) {
  __shared__ double red[4];
  const float cap2 = cap * cap;
  double a[ICP_NF];
#pragma unroll
  for (int k = 0; k < ICP_NF; ++k) a[k] = 0.0;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < m; i += (long long)gridDim.x * 256) {
    const long long si = order ? order[i] : i;
    const double x = (double)src[3 * si], y = (double)src[3 * si + 1], z = (double)src[3 * si + 2];
    const float px = transform_row(T, 0, x, y, z), py = transform_row(T, 1, x, y, z), pz = transform_row(T, 2, x, y, z);
    NearestIndex n{cap2, cap2, 0x7fffffff, -1};
    grid_walk(g, px, py, pz, n);
    const bool hit = n.d2 < cap2;
    if (index) index[si] = hit ? n.index : -1;
    if (dist) dist[si] = hit ? fminf(sqrtf(n.d2), cap) : cap;
    if (hit) {
      const float4 t = g.pts[n.pos];
      const double p[3] = {(double)px, (double)py, (double)pz}, q[3] = {(double)t.x, (double)t.y, (double)t.z};
      a[0] += 1.0;
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        a[1 + r] += p[r];
        a[4 + r] += q[r];
#pragma unroll
        for (int c = 0; c < 3; ++c) a[7 + 3 * r + c] += q[r] * p[c];       // exact: a product of two fp32 values
      }
      const double dx = p[0] - q[0], dy = p[1] - q[1], dz = p[2] - q[2];
      a[16] += (dx * dx + dy * dy) + dz * dz;
      a[17] += (p[0] * p[0] + p[1] * p[1]) + p[2] * p[2];
    }
  }
  double* __restrict__ r = rec + (size_t)blockIdx.x * ICP_NF;
#pragma unroll
  for (int k = 0; k < ICP_NF; ++k) {
    const double v = icp_block_sum(a[k], red);
    if (threadIdx.x == 0) r[k] = v;
  }
}

// Pass 2.  One workgroup sums the `groups` records field by field, in a fixed order -> out [18].
__global__ __launch_bounds__(256) void icp_reduce_kernel(const double* __restrict__ rec, int groups, double* __restrict__ out) {
  __shared__ double red[4];
  for (int f = 0; f < ICP_NF; ++f) {
    double s = 0.0;
    for (int i = threadIdx.x; i < groups; i += 256) s += rec[(size_t)i * ICP_NF + f];
    s = icp_block_sum(s, red);
    if (threadIdx.x == 0) out[f] = s;
  }
}

// Voxel v holds the points perm[start[v] .. start[v + 1]) (input indices, ascending inside a voxel: the sort by key is stable).
// Their mean is accumulated in fp64 in that order and rounded once.
__global__ __launch_bounds__(256) void voxel_mean_kernel(const float* __restrict__ pts, long long n,
                                                         const long long* __restrict__ perm, const int* __restrict__ start,
                                                         long long n_voxels, float* __restrict__ out) {
  for (long long v = (long long)blockIdx.x * blockDim.x + threadIdx.x; v < n_voxels; v += (long long)gridDim.x * blockDim.x) {
    const int b = start[v], e = start[v + 1];
    double sx = 0.0, sy = 0.0, sz = 0.0;
    int cnt = 0;
    for (int j = b; j < e; ++j) {
      if (j < 0 || j >= n) continue;                       // offsets outside the permutation: read nothing
      const long long i = perm[j];
      if (i < 0 || i >= n) continue;
      sx += (double)pts[3 * i];
      sy += (double)pts[3 * i + 1];
      sz += (double)pts[3 * i + 2];
      ++cnt;
    }
    const double c = (double)cnt;
    out[3 * v] = (float)(sx / c);
    out[3 * v + 1] = (float)(sy / c);
    out[3 * v + 2] = (float)(sz / c);
  }
}

// keep[i] = axis_min <= p[w] <= axis_max and an odd number of polygon edges crossed by the ray from p towards -u, all in fp64.
// The polygon's (u, v) coordinates are staged in LDS once per workgroup.
__global__ __launch_bounds__(256) void polygon_crop_kernel(const float* __restrict__ pts, long long n,
                                                           const double* __restrict__ poly, int P, int iu, int iv, int iw,
                                                           double axis_min, double axis_max, unsigned char* __restrict__ keep) {
  __shared__ double pu[CDS_CROP_MAX_VERTICES], pv[CDS_CROP_MAX_VERTICES];
  for (int k = threadIdx.x; k < P; k += 256) {
    pu[k] = poly[3 * k + iu];
    pv[k] = poly[3 * k + iv];
  }
  __syncthreads();
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const double u = (double)pts[3 * i + iu], v = (double)pts[3 * i + iv], w = (double)pts[3 * i + iw];
    int crossings = 0;
    if (w >= axis_min && w <= axis_max) {
      double au = pu[P - 1], av = pv[P - 1];               // edge (P - 1, 0) first: the parity does not depend on the order
      for (int k = 0; k < P; ++k) {
        const double bu = pu[k], bv = pv[k];
        if ((v < av) != (v < bv) && au + (v - av) / (bv - av) * (bu - au) < u) ++crossings;
        au = bu; av = bv;
      }
    }
    keep[i] = (unsigned char)(crossings & 1);
  }
}

inline int icp_groups(long long m) {
  const long long want = (m + 255) / 256;
  return (int)(want < 1 ? 1 : want < ICP_MAX_GROUPS ? want : ICP_MAX_GROUPS);
}

}  // namespace

extern "C" int cds_transform_points_f32(const float* points, long long n, const double* T, float* out, void* stream) {
  if (n < 0 || !T || (n > 0 && (!points || !out))) return CDS_EINVAL;
  if (n == 0) return 0;
  hipLaunchKernelGGL(transform_points_kernel, dim3(grid_blocks(n)), dim3(256), 0, (hipStream_t)stream, points, n, T, out);
  return cds_launch_status();
}

extern "C" int cds_nn_index_f32(const float* query, const long long* order, long long m, const float* pts, const int* cell_start,
                                const long long* cell_keys, const int* coarse_start, const long long* table_keys,
                                const int* table_vals, int log2_slots, const float* frame_host, float max_dist, float* dist,
                                int* index, void* stream) {
  GridView g;
  if (m < 0 || !(max_dist >= 0.0f)) return CDS_EINVAL;
  if (m == 0) return 0;
  if (!query || !dist || !index ||
      !grid_view(pts, cell_start, cell_keys, coarse_start, table_keys, table_vals, log2_slots, frame_host, g))
    return CDS_EINVAL;
  hipLaunchKernelGGL(nn_index_kernel, dim3(grid_blocks(m)), dim3(256), 0, (hipStream_t)stream, query, order, m, g, max_dist, dist,
                     index);
  return cds_launch_status();
}

extern "C" int cds_icp_sums_f64(const float* source, const long long* order, long long m, const double* T, const float* pts,
                                const int* cell_start, const long long* cell_keys, const int* coarse_start,
                                const long long* table_keys, const int* table_vals, int log2_slots, const float* frame_host,
                                float max_dist, double* ws, long long ws_doubles, double* out, int* index, float* dist,
                                void* stream) {
  GridView g;
  if (m < 1 || !source || !T || !ws || !out || !(max_dist >= 0.0f) ||
      !grid_view(pts, cell_start, cell_keys, coarse_start, table_keys, table_vals, log2_slots, frame_host, g))
    return CDS_EINVAL;
  const int groups = icp_groups(m);
  if ((long long)groups * ICP_NF > ws_doubles) return CDS_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(icp_sums_kernel, dim3(groups), dim3(256), 0, st, source, order, m, T, g, max_dist, ws, index, dist);
  hipLaunchKernelGGL(icp_reduce_kernel, dim3(1), dim3(256), 0, st, ws, groups, out);
  return cds_launch_status();
}

extern "C" int cds_voxel_mean_f32(const float* points, long long n, const long long* perm, const int* start, long long n_voxels,
                                  float* out, void* stream) {
  if (n < 0 || n_voxels < 0 || n_voxels > n || n > 0x7fffffffLL) return CDS_EINVAL;
  if (n_voxels == 0) return 0;
  if (!points || !perm || !start || !out) return CDS_EINVAL;
  hipLaunchKernelGGL(voxel_mean_kernel, dim3(grid_blocks(n_voxels)), dim3(256), 0, (hipStream_t)stream, points, n, perm, start,
                     n_voxels, out);
  return cds_launch_status();
}

extern "C" int cds_polygon_crop_f32(const float* points, long long n, const double* polygon, int P, int axis, double axis_min,
                                    double axis_max, unsigned char* keep, void* stream) {
  if (n < 0 || !polygon || P < 3 || P > CDS_CROP_MAX_VERTICES || axis < 0 || axis > 2) return CDS_EINVAL;
  if (n == 0) return 0;
  if (!points || !keep) return CDS_EINVAL;
  const int iu = axis == 0 ? 1 : 0, iv = axis == 2 ? 1 : 2;   // (u, v) = (Y, Z), (X, Z), (X, Y) for w = X, Y, Z
  hipLaunchKernelGGL(polygon_crop_kernel, dim3(grid_blocks(n)), dim3(256), 0, (hipStream_t)stream, points, n, polygon, P, iu, iv,
                     axis, axis_min, axis_max, keep);
  return cds_launch_status();
}
