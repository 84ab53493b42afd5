// Gipuma-style depth-map fusion (the fusion step of the reference's `--filter_method gipuma`, gipuma.py:153-195, which
// shells out to fusibile; Galliani et al., ICCV 2015).  cds_mvsnet_amd/gipuma.py drives these kernels; the rule is
// restated in float32 numpy in tests/gipuma_ref.py.
//
//   gipuma_prob_filter_kernel  all views: D'_v(p) = D_v(p) if C_v[0](p) > p1 and C_v[1](p) > p2 and C_v[2](p) > p3, else 0
//                              (gipuma.py:153-175), and the RGB of every pixel packed as r | g << 8 | b << 16 in one word
//   gipuma_fuse_view_kernel    one reference view r, one lane per pixel p = (x, y) of r (integer coordinates, no +0.5),
//                              looping over the other views j in ascending order
//   gipuma_count_kernel /      raster-order compaction of the emitted points over all views (prefix sum over the emit
//   gipuma_scan_kernel /       flags in tiles of 4096: per-tile counts, one workgroup scans the counts, each tile then
//   gipuma_compact_kernel      rescans its flags and writes its points in order; no atomics, so the order is fixed)
//
// The fusion rule for reference view r, per pixel p with d = D'_r(p):
//   skip p if used_r(p) is set or d is not in (depth_min, depth_max);
//   X = Minv_r (d x - p4_r.x, d y - p4_r.y, d - p4_r.z);  S = X;  rgb = I_r(p) (integer sums);  n = 0
//   for j != r ascending:
//     (a, b, z) = P_j (X, 1);  skip if z <= 0;  u = a / z;  v = b / z;  skip unless 0 <= u < w and 0 <= v < h
//     iu = min(floor(u + 0.5), w - 1);  iv = min(floor(v + 0.5), h - 1);  dj = D'_j(iu, iv)
//     skip if dj is not in (depth_min, depth_max);  skip unless |fb_rj / z - fb_rj / dj| < disp_thresh
//     n += 1;  S += Minv_j (dj iu - p4_j.x, dj iv - p4_j.y, dj - p4_j.z);  rgb += I_j(iu, iv)
//   if n >= num_consistent: emit S / (n + 1) with colour rgb / (n + 1) (integer floor) and set used_j(iu, iv) = 1 for
//   every counted (j, iu, iv).  A used pixel still counts as evidence for a later r; it only never starts a point.
// Points where fusibile is not known or not consistent with itself, and which this rule fixes: z <= 0 never counts; a
// sample outside (depth_min, depth_max) never counts; the depth sample, its 3D point and the used mark all use the same
// rounded pixel; fb_rj = K_r[0][0] |c_r - c_j| (f from K, not from decomposing P).
//
// Arithmetic (every step one correctly rounded fp32 operation, -ffp-contract=off, true divisions): a matrix-vector row is
// ((m0 q0 + m1 q1) + m2 q2) (+ m3); q = (d x - p4.x, d y - p4.y, d - p4.z) with d x one product; S.k = S.k + row_k;
// u = a / z, v = b / z, u + 0.5 then floor; the disparity test is fabs(fb / z - fb / dj) < disp_thresh; the point is
// S.k / (float)(n + 1).  tests/gipuma_ref.py performs the same operations in the same order.
//
// Per-view constants views[V][24] (host float64, cast to float32): P_v = K_v E_v[:3] (12, row-major; p4_v is its last
// column), Minv_v = inverse(P_v[:, :3]) (9), 3 unused.  fb[V][V]: fb_rj = K_r[0][0] |c_r - c_j| with c_v = -Minv_v p4_v.
// The loop index j is uniform over the wave, so those rows are read with scalar loads.
//
// The reference views depend on each other through `used`: one launch per r, in order, on one stream.  Inside a launch
// there is no race: it reads used_r only and writes only used_j for j != r, always the value 1.  A lane that emits runs
// the j loop a second time to mark `used`, recomputing the same decisions with the same code (no cap on V).
#include "cds_common.hpp"

namespace {

constexpr int kTile = 4096;                 // emit flags per compaction tile: 256 lanes x 16 flags (one 16-byte load)
constexpr int kViewWords = 24;

__device__ __forceinline__ float row3(const float* m, float q0, float q1, float q2) {
  return (m[0] * q0 + m[1] * q1) + m[2] * q2;
}

__device__ __forceinline__ float row4(const float* m, float q0, float q1, float q2) {
  return ((m[0] * q0 + m[1] * q1) + m[2] * q2) + m[3];
}

// One (pixel, view) decision of the rule: true when view j counts as evidence for the point X; then (iu, iv) is the
// rounded pixel of j and dj its depth.  Both loops of the fusion kernel call this, so they take the same decisions.
__device__ __forceinline__ bool consistent(const float* __restrict__ c, const float* __restrict__ depth_j, float f, int w,
                                           int h, float X0, float X1, float X2, float dmin, float dmax, float disp, int& iu,
                                           int& iv, float& dj) {
  const float a = row4(c, X0, X1, X2);
  const float b = row4(c + 4, X0, X1, X2);
  const float z = row4(c + 8, X0, X1, X2);
  if (!(z > 0.0f)) return false;
  const float u = a / z, v = b / z;
  if (!(u >= 0.0f && u < (float)w && v >= 0.0f && v < (float)h)) return false;
  iu = (int)fminf(floorf(u + 0.5f), (float)(w - 1));
  iv = (int)fminf(floorf(v + 0.5f), (float)(h - 1));
  dj = depth_j[iv * w + iu];
  if (!(dj > dmin && dj < dmax)) return false;
  return fabsf(f / z - f / dj) < disp;
}

__global__ __launch_bounds__(256) void gipuma_prob_filter_kernel(const float* __restrict__ depth,
                                                                 const float* __restrict__ conf,
                                                                 const unsigned char* __restrict__ rgb8, long long n,
                                                                 int hw, float t0, float t1, float t2,
                                                                 float* __restrict__ out, unsigned* __restrict__ rgb) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const long long v = i / hw, p = i - v * hw;
    const float* cv = conf + v * 3 * hw + p;
    out[i] = (cv[0] > t0 && cv[hw] > t1 && cv[2 * hw] > t2) ? depth[i] : 0.0f;
    const unsigned char* c = rgb8 + 3 * i;
    rgb[i] = (unsigned)c[0] | ((unsigned)c[1] << 8) | ((unsigned)c[2] << 16);
  }
}

// rec[r hw + p] = (S / (n + 1) as three float bit patterns, packed colour) for an emitted pixel; emit[r hw + p] = 0 / 1
__global__ __launch_bounds__(256) void gipuma_fuse_view_kernel(const float* __restrict__ depth, const unsigned* __restrict__ rgb,
                                                               const float* __restrict__ views, const float* __restrict__ fb_row,
                                                               int r, int V, int h, int w, float dmin, float dmax, float disp,
                                                               int ncons, unsigned char* used, unsigned char* __restrict__ emit,
                                                               uint4* __restrict__ rec) {
  const int hw = h * w;
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= hw) return;
  const long long base = (long long)r * hw;
  const float d = depth[base + p];
  if (used[base + p] || !(d > dmin && d < dmax)) {
    emit[base + p] = 0;
    return;
  }
  const int y = p / w, x = p - y * w;
  const float* cr = views + r * kViewWords;
  const float q0 = d * (float)x - cr[3], q1 = d * (float)y - cr[7], q2 = d - cr[11];
  const float X0 = row3(cr + 12, q0, q1, q2), X1 = row3(cr + 15, q0, q1, q2), X2 = row3(cr + 18, q0, q1, q2);
  float S0 = X0, S1 = X1, S2 = X2;
  const unsigned c0 = rgb[base + p];
  unsigned sr = c0 & 255u, sg = (c0 >> 8) & 255u, sb = (c0 >> 16) & 255u;
  int n = 0;
  for (int j = 0; j < V; ++j) {
    if (j == r) continue;
    const float* c = views + j * kViewWords;
    const long long bj = (long long)j * hw;
    int iu, iv;
    float dj;
    if (!consistent(c, depth + bj, fb_row[j], w, h, X0, X1, X2, dmin, dmax, disp, iu, iv, dj)) continue;
    const int pj = iv * w + iu;
    const float e0 = dj * (float)iu - c[3], e1 = dj * (float)iv - c[7], e2 = dj - c[11];
    S0 = S0 + row3(c + 12, e0, e1, e2);
    S1 = S1 + row3(c + 15, e0, e1, e2);
    S2 = S2 + row3(c + 18, e0, e1, e2);
    const unsigned cj = rgb[bj + pj];
    sr += cj & 255u;
    sg += (cj >> 8) & 255u;
    sb += (cj >> 16) & 255u;
    ++n;
  }
  const bool ok = n >= ncons;
  emit[base + p] = ok ? 1 : 0;
  if (!ok) return;
  const float k = (float)(n + 1);
  const unsigned m = (unsigned)(n + 1);
  rec[base + p] = make_uint4(__float_as_uint(S0 / k), __float_as_uint(S1 / k), __float_as_uint(S2 / k),
                             (sr / m) | ((sg / m) << 8) | ((sb / m) << 16));
  for (int j = 0; j < V; ++j) {
    if (j == r) continue;
    const long long bj = (long long)j * hw;
    int iu, iv;
    float dj;
    if (consistent(views + j * kViewWords, depth + bj, fb_row[j], w, h, X0, X1, X2, dmin, dmax, disp, iu, iv, dj))
      used[bj + iv * w + iu] = 1;
  }
}

// inclusive scan of one value per lane over a 256-lane workgroup; returns the lane's inclusive sum, total in *total
__device__ __forceinline__ int block_scan_256(int v, int* lds, int* total) {
  const int t = threadIdx.x;
  lds[t] = v;
  __syncthreads();
  for (int off = 1; off < 256; off <<= 1) {
    const int add = t >= off ? lds[t - off] : 0;
    __syncthreads();
    lds[t] += add;
    __syncthreads();
  }
  const int inc = lds[t];
  *total = lds[255];
  __syncthreads();
  return inc;
}

__device__ __forceinline__ int flags16(const uint4 f) {
  // each byte is 0 or 1: the byte sums of the four words
  const unsigned s = f.x + f.y + f.z + f.w;          // at most 4 per byte: no carry between bytes
  return (int)((s & 255u) + ((s >> 8) & 255u) + ((s >> 16) & 255u) + (s >> 24));
}

__global__ __launch_bounds__(256) void gipuma_count_kernel(const uint4* __restrict__ emit, int* __restrict__ tile_count) {
  __shared__ int lds[256];
  int total;
  block_scan_256(flags16(emit[(long long)blockIdx.x * 256 + threadIdx.x]), lds, &total);
  if (threadIdx.x == 0) tile_count[blockIdx.x] = total;
}

// one workgroup: exclusive offsets of the tile counts, in chunks of 256, and the grand total
__global__ __launch_bounds__(256) void gipuma_scan_kernel(const int* __restrict__ tile_count, int tiles,
                                                          int* __restrict__ tile_off, int* __restrict__ total) {
  __shared__ int lds[256];
  int carry = 0;
  for (int b = 0; b < tiles; b += 256) {
    const int i = b + (int)threadIdx.x;
    const int v = i < tiles ? tile_count[i] : 0;
    int sum;
    const int inc = block_scan_256(v, lds, &sum);
    if (i < tiles) tile_off[i] = carry + inc - v;
    carry += sum;
  }
  if (threadIdx.x == 0) *total = carry;
}

__global__ __launch_bounds__(256) void gipuma_compact_kernel(const uint4* __restrict__ emit, const uint4* __restrict__ rec,
                                                             const int* __restrict__ tile_off, int hw,
                                                             float* __restrict__ points, unsigned* __restrict__ colors,
                                                             int* __restrict__ ref_view) {
  __shared__ int lds[256];
  const long long first = (long long)blockIdx.x * kTile + (long long)threadIdx.x * 16;
  const uint4 f = emit[(long long)blockIdx.x * 256 + threadIdx.x];
  const int cnt = flags16(f);
  int total;
  const int inc = block_scan_256(cnt, lds, &total);
  if (cnt == 0) return;
  int o = tile_off[blockIdx.x] + inc - cnt;
  const unsigned words[4] = {f.x, f.y, f.z, f.w};
  for (int k = 0; k < 16; ++k) {
    if (!((words[k >> 2] >> (8 * (k & 3))) & 255u)) continue;
    const long long i = first + k;
    const uint4 q = rec[i];
    points[3ll * o] = __uint_as_float(q.x);
    points[3ll * o + 1] = __uint_as_float(q.y);
    points[3ll * o + 2] = __uint_as_float(q.z);
    colors[o] = q.w;
    ref_view[o] = (int)(i / hw);
    ++o;
  }
}

int grid_blocks(long long n) { return (int)(n < 1 ? 1 : (n + 255) / 256 < 8192 ? (n + 255) / 256 : 8192); }

}  // namespace

extern "C" int cds_gipuma_tiles(long long n) {
  if (n < 0 || n > (long long)INT32_MAX - kTile) return CDS_EINVAL;
  return (int)((n + kTile - 1) / kTile);
}

extern "C" int cds_gipuma_prob_filter_f32(const float* depths, const float* confs, const unsigned char* rgb8, int V, int h,
                                          int w, const float* prob_thresh_host, float* depth_out, unsigned* rgb_out,
                                          void* stream) {
  if (V < 1 || h < 1 || w < 1 || (long long)V * h * w > INT32_MAX || !depths || !confs || !rgb8 || !prob_thresh_host ||
      !depth_out || !rgb_out)
    return CDS_EINVAL;
  const long long n = (long long)V * h * w;
  hipLaunchKernelGGL(gipuma_prob_filter_kernel, dim3(grid_blocks(n)), dim3(256), 0, (hipStream_t)stream, depths, confs, rgb8, n,
                     h * w, prob_thresh_host[0], prob_thresh_host[1], prob_thresh_host[2], depth_out, rgb_out);
  return cds_launch_status();
}

extern "C" int cds_gipuma_fuse_view_f32(const float* depths, const unsigned* rgb, const float* views, const float* fb, int r,
                                        int V, int h, int w, float depth_min, float depth_max, float disp_thresh,
                                        int num_consistent, unsigned char* used, unsigned char* emit, unsigned* records,
                                        void* stream) {
  if (V < 1 || r < 0 || r >= V || h < 1 || w < 1 || (long long)V * h * w > INT32_MAX || !depths || !rgb || !views || !fb ||
      !used || !emit || !records || ((size_t)records & 15))
    return CDS_EINVAL;
  hipLaunchKernelGGL(gipuma_fuse_view_kernel, dim3((h * w + 255) / 256), dim3(256), 0, (hipStream_t)stream, depths, rgb, views,
                     fb + (long long)r * V, r, V, h, w, depth_min, depth_max, disp_thresh, num_consistent, used, emit,
                     (uint4*)records);
  return cds_launch_status();
}

extern "C" int cds_gipuma_scan(const unsigned char* emit, int tiles, int* tile_count, int* tile_off, int* total, void* stream) {
  if (tiles < 1 || !emit || !tile_count || !tile_off || !total || ((size_t)emit & 15)) return CDS_EINVAL;
  hipLaunchKernelGGL(gipuma_count_kernel, dim3(tiles), dim3(256), 0, (hipStream_t)stream, (const uint4*)emit, tile_count);
  hipLaunchKernelGGL(gipuma_scan_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, tile_count, tiles, tile_off, total);
  return cds_launch_status();
}

extern "C" int cds_gipuma_compact_f32(const unsigned char* emit, const unsigned* records, const int* tile_off, int tiles,
                                      int hw, float* points, unsigned* colors, int* ref_view, void* stream) {
  if (tiles < 1 || hw < 1 || !emit || !records || !tile_off || !points || !colors || !ref_view || ((size_t)emit & 15) ||
      ((size_t)records & 15))
    return CDS_EINVAL;
  hipLaunchKernelGGL(gipuma_compact_kernel, dim3(tiles), dim3(256), 0, (hipStream_t)stream, (const uint4*)emit,
                     (const uint4*)records, tile_off, hw, points, colors, ref_view);
  return cds_launch_status();
}
