// Outlier removal for fused clouds (cds_mvsnet_amd/pointcloud.py: remove_outliers), over the sparse grid of
// pointcloud.hip / grid_common.hpp:
//
//   cds_knn_mean_f64        per query the mean distance to its k nearest grid points (capped terms), one query per lane in cell
//                           order: grid_walk, the walk of cds_nn_query_f32, with a k-slot candidate list per lane as its sink
//   cds_radius_count_f32    per query the number of grid points within a radius, up to a cap (cell side >= radius)
//   cds_outlier_stats_f64   mean and sample standard deviation of n doubles, summed in one fixed order
//
// The candidate list lives in LDS, laid out [slot][lane]: slot j of lane t is list[j * blockDim.x + t], so whatever slots the
// lanes of a wave touch, they touch 64 different banks.  (A per-lane array indexed at run time would go to scratch.)  The
// current worst d2 and its slot stay in registers; an insert overwrites the worst and rescans the k slots for the new one.
// Inserts are rare once the list is full: the walk visits the nearest cells first.  No workgroup barrier is needed, a lane only
// ever touches its own column, so the workgroup size is free: one wave (cds_knn_mean_wg_f64 takes it as an argument; profiles/cloud_outliers.md).
//
// Every rule is a function of the inputs: the k smallest d2 form a multiset that no visiting order changes, the sums run in a
// stated order, nothing is accumulated with atomics.
#include "grid_common.hpp"

namespace {

constexpr int kStatChunk = 4096;   // elements per chunk of the fixed-order sum: 256 lanes x 16
constexpr int kStatLanes = 256;

// grid_walk's sink for the k nearest: the k smallest d2 below cap2 seen so far; column `col` = &list[lane], stride = lanes per workgroup
struct KnnList {
  float* col;
  int stride, k, count;
  float cap2, worst;
  int worst_at;

  __device__ __forceinline__ float bound() const { return count < k ? cap2 : worst; }

  __device__ __forceinline__ void rescan() {
    worst = col[0];
    worst_at = 0;
    for (int j = 1; j < k; ++j) {
      const float v = col[j * stride];
      if (v > worst) { worst = v; worst_at = j; }
    }
  }

  // a region whose points are all at least bound() away cannot change the list: an equal candidate changes nothing for a multiset
  __device__ __forceinline__ bool skips(float lb2) const { return lb2 >= bound(); }

  __device__ __forceinline__ void add(float d2, const float4&, int) {
    if (!(d2 < bound())) return;          // at or beyond the cap, or no better than the worst of a full list (NaN too)
    if (count < k) {
      col[count * stride] = d2;
      if (++count == k) rescan();
    } else {
      col[worst_at * stride] = d2;
      rescan();
    }
  }
};

// mean[q] = (t_0 + t_1 + ... ) / terms in ascending d2 order, t_j = sqrt((double)d2_j) for the accepted, (double)cap for the rest
__global__ __launch_bounds__(256) void knn_mean_kernel(const float* __restrict__ query, const long long* __restrict__ order,
                                                       long long m, GridView g, int k, float cap, double* __restrict__ mean,
                                                       float* __restrict__ kth) {
  extern __shared__ float list[];
  const float cap2 = cap * cap;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (long long)gridDim.x * blockDim.x) {
    const long long qi = order ? order[i] : i;
    KnnList s{list + threadIdx.x, (int)blockDim.x, k, 0, cap2, cap2, 0};
    grid_walk(g, query[3 * qi], query[3 * qi + 1], query[3 * qi + 2], s);
    // selection sort of the lane's column: ascending d2, summed as it goes
    double sum = 0.0;
    float last = 0.0f;
    for (int a = 0; a < s.count; ++a) {
      float lo = s.col[a * s.stride];
      int at = a;
      for (int j = a + 1; j < s.count; ++j) {
        const float v = s.col[j * s.stride];
        if (v < lo) { lo = v; at = j; }
      }
      if (at != a) s.col[at * s.stride] = s.col[a * s.stride];
      sum += sqrt((double)lo);
      last = lo;
    }
    // an infinite cap accepts every point, the walk ends when the grid is exhausted: min(k, n) terms, none missing
    const int terms = cap == INFINITY ? s.count : k;
    for (int a = s.count; a < terms; ++a) sum += (double)cap;
    mean[qi] = sum / (double)terms;
    if (kth) kth[qi] = s.count == terms && terms > 0 ? sqrtf(last) : cap;
  }
}

__global__ __launch_bounds__(256) void radius_count_kernel(const float* __restrict__ query, const long long* __restrict__ order,
                                                           long long m, GridView g, float radius, int cap,
                                                           int* __restrict__ count) {
  const Frame& f = g.f;
  const float r2 = radius * radius;
  const float reach = radius + 2.0f * f.slop;     // binning error of the point and of the query
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (long long)gridDim.x * blockDim.x) {
    const long long qi = order ? order[i] : i;
    const float qx = query[3 * qi], qy = query[3 * qi + 1], qz = query[3 * qi + 2];
    // h >= radius: the cells that [q - reach, q + reach] touches, three per axis and a fourth next to a cell boundary
    const float ax = cell_of(qx - reach, f.ox, f.h), bx = cell_of(qx + reach, f.ox, f.h);
    const float ay = cell_of(qy - reach, f.oy, f.h), by = cell_of(qy + reach, f.oy, f.h);
    const float az = cell_of(qz - reach, f.oz, f.h), bz = cell_of(qz + reach, f.oz, f.h);
    int c = 0;
    // a query whose range misses the grid on one axis has no neighbour (clamping would fold far cells onto the border)
    const bool hit = bx >= 0.0f && ax < (float)f.nx && by >= 0.0f && ay < (float)f.ny && bz >= 0.0f && az < (float)f.nz;
    if (hit) {
      const int x0 = clamp_cell(ax, f.nx), x1 = clamp_cell(bx, f.nx), y0 = clamp_cell(ay, f.ny), y1 = clamp_cell(by, f.ny),
                z0 = clamp_cell(az, f.nz), z1 = clamp_cell(bz, f.nz);
      for (int z = z0; z <= z1 && c < cap; ++z)
        for (int y = y0; y <= y1 && c < cap; ++y)
          for (int x = x0; x <= x1 && c < cap; ++x) {
            const int cell = find(g.t, fine_key(x, y, z));
            if (cell < 0) continue;
            const int e = g.cell_start[cell + 1];
            for (int j = g.cell_start[cell]; j < e && c < cap; ++j) {
              const float4 p = g.pts[j];
              const float dx = p.x - qx, dy = p.y - qy, dz = p.z - qz;
              if (dx * dx + dy * dy + dz * dz <= r2) ++c;
            }
          }
    }
    count[qi] = c;
  }
}

// ws[c] = the sum of chunk c of the terms (x itself, or (x - mu)^2 with mu = out[0]): lane l adds terms l, l + 256, ... in that
// order to +0.0, terms past n are +0.0, the lanes fold by halves
template <bool DEVIATION>
__global__ __launch_bounds__(kStatLanes) void stat_chunks_kernel(const double* __restrict__ x, long long n, long long chunks,
                                                                 const double* __restrict__ out, double* __restrict__ ws) {
  __shared__ double lane[kStatLanes];
  const int l = threadIdx.x;
  const double mu = DEVIATION ? out[0] : 0.0;
  for (long long c = blockIdx.x; c < chunks; c += gridDim.x) {
    double acc = 0.0;
    for (int r = 0; r < kStatChunk / kStatLanes; ++r) {
      const long long i = c * kStatChunk + r * kStatLanes + l;
      double t = 0.0;
      if (i < n) {
        t = x[i];
        if (DEVIATION) { const double d = t - mu; t = d * d; }
      }
      acc += t;
    }
    __syncthreads();                      // lane[] may still be read from the previous chunk
    lane[l] = acc;
    __syncthreads();
    for (int s = kStatLanes / 2; s >= 1; s >>= 1) {
      if (l < s) lane[l] += lane[l + s];
      __syncthreads();
    }
    if (l == 0) ws[c] = lane[0];
  }
}

// one thread: the chunk sums in ascending order; then mu = S / n, or sigma = sqrt(S / (n - 1)) (0 for n = 1)
template <bool DEVIATION>
__global__ void stat_finish_kernel(const double* __restrict__ ws, long long chunks, long long n, double* __restrict__ out) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  double s = 0.0;
  for (long long c = 0; c < chunks; ++c) s += ws[c];
  if (DEVIATION) out[1] = n > 1 ? sqrt(s / (double)(n - 1)) : 0.0;
  else out[0] = s / (double)n;
}

}  // namespace

extern "C" int cds_knn_mean_wg_f64(const float* query, const long long* order, long long m, const float* pts,
                                   const int* cell_start, const long long* cell_keys, const int* coarse_start,
                                   const long long* table_keys, const int* table_vals, int log2_slots, const float* frame_host,
                                   int k, float max_dist, double* mean, float* kth, int threads, void* stream) {
  GridView g;
  if (m < 0 || k < 1 || k > CDS_KNN_MAX_K || !(max_dist >= 0.0f)) return CDS_EINVAL;
  if (threads != 64 && threads != 128 && threads != 256) return CDS_EINVAL;
  if (!grid_view(pts, cell_start, cell_keys, coarse_start, table_keys, table_vals, log2_slots, frame_host, g)) return CDS_EINVAL;
  if (m == 0) return 0;
  if (!query || !mean) return CDS_EINVAL;
  const long long groups = (m + threads - 1) / threads;
  hipLaunchKernelGGL(knn_mean_kernel, dim3((unsigned)(groups < 32768 ? groups : 32768)), dim3(threads),
                     (size_t)k * threads * sizeof(float), (hipStream_t)stream, query, order, m, g, k, max_dist, mean, kth);
  return cds_launch_status();
}

// measured on a 4 M point surface cloud (profiles/cloud_outliers.md): single waves match or beat 128 and 256 lanes at k = 9, 21, 64;
// at k = 64 the lists of a 256-lane group take 64 KiB, two groups per CU, and single waves fill the LDS to the last list
extern "C" int cds_knn_mean_f64(const float* query, const long long* order, long long m, const float* pts,
                                const int* cell_start, const long long* cell_keys, const int* coarse_start,
                                const long long* table_keys, const int* table_vals, int log2_slots, const float* frame_host, int k,
                                float max_dist, double* mean, float* kth, void* stream) {
  return cds_knn_mean_wg_f64(query, order, m, pts, cell_start, cell_keys, coarse_start, table_keys, table_vals, log2_slots, frame_host,
                             k, max_dist, mean, kth, 64, stream);
}

extern "C" int cds_radius_count_f32(const float* query, const long long* order, long long m, const float* pts,
                                    const int* cell_start, const long long* cell_keys, const int* coarse_start,
                                    const long long* table_keys, const int* table_vals, int log2_slots, const float* frame_host,
                                    float radius, int cap, int* count, void* stream) {
  GridView g;
  if (m < 0 || !(radius >= 0.0f) || radius == INFINITY || cap < 1) return CDS_EINVAL;
  if (!grid_view(pts, cell_start, cell_keys, coarse_start, table_keys, table_vals, log2_slots, frame_host, g)) return CDS_EINVAL;
  if (g.f.h < radius) return CDS_EINVAL;
  if (m == 0) return 0;
  if (!query || !count) return CDS_EINVAL;
  hipLaunchKernelGGL(radius_count_kernel, dim3(grid_blocks(m)), dim3(256), 0, (hipStream_t)stream, query, order, m, g, radius, cap,
                     count);
  return cds_launch_status();
}

extern "C" int cds_outlier_stats_f64(const double* x, long long n, double* ws, long long ws_doubles, double* out, void* stream) {
  if (n < 1 || !x || !ws || !out) return CDS_EINVAL;
  const long long chunks = (n + kStatChunk - 1) / kStatChunk;
  if (ws_doubles < chunks) return CDS_EINVAL;
  const dim3 groups((unsigned)(chunks < 4096 ? chunks : 4096));
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(stat_chunks_kernel<false>, groups, dim3(kStatLanes), 0, st, x, n, chunks, (const double*)out, ws);
  hipLaunchKernelGGL(stat_finish_kernel<false>, dim3(1), dim3(64), 0, st, (const double*)ws, chunks, n, out);
  hipLaunchKernelGGL(stat_chunks_kernel<true>, groups, dim3(kStatLanes), 0, st, x, n, chunks, (const double*)out, ws);
  hipLaunchKernelGGL(stat_finish_kernel<true>, dim3(1), dim3(64), 0, st, (const double*)ws, chunks, n, out);
  return cds_launch_status();
}
