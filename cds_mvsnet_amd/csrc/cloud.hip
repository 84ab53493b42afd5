// Fused clouds that other tools can use (both rules are stated in include/cds_mvsnet_hip.h):
//
//   cds_depth_normals_f32   one oriented world-frame normal per pixel of a depth map: an inverse-depth plane fit over a
//                           (2r+1)^2 window, closed form, exact on planes, facing the camera by construction
//   cds_voxel_merge_f32     one attributed point per occupied voxel: mean position (bit for bit that of cds_voxel_mean_f32),
//                           rounded mean colour, normalised sum of the normals, point count
//
// Normals: one 256-thread workgroup per 32x8 pixel tile.  The tile plus an r-pixel halo is staged in LDS once as the pair
// (depth, 1/depth), both fp64, read back with one 16-byte LDS load per tap: each reciprocal, the only expensive fp64 operation of
// the rule, is computed once per pixel and not once per window it falls into (up to 81).  A pixel that is not valid (outside the
// image, valid == 0, depth not finite or not > 0) is staged with a NaN depth, so it fails the jump test without a test of its
// own.  The window loop is compiled for each radius (template parameter): trip counts and LDS offsets are constants.  It has no
// branches: a tap that does not enter adds 0 to the integer moments and +-0.0 to the three fp64 sums, which leaves them bit for
// bit what the rule's "sum over the entering pixels in visiting order" gives.  Largest tile: r = 4, 40 x 16 cells x 16 B = 10 KiB.
#include "cds_common.hpp"

namespace {

constexpr int kTileW = 32, kTileH = 8;   // 256 threads: one wave covers two tile rows

struct NormalCam {
  float K[9], R[9];                      // intrinsics and the rotation of E (world -> camera), row-major
};

template <int R>
__global__ __launch_bounds__(256) void depth_normals_kernel(const float* __restrict__ depth,
                                                            const unsigned char* __restrict__ valid, NormalCam cam, int h,
                                                            int w, float jump, int min_pts, float* __restrict__ normals,
                                                            unsigned char* __restrict__ ok) {
  constexpr int LW = kTileW + 2 * R, LH = kTileH + 2 * R;
  __shared__ double2 s_c[LH * LW];       // (depth, 1 / depth); (NaN, 0) where the pixel is not valid
  const int x0 = blockIdx.x * kTileW - R, y0 = blockIdx.y * kTileH - R;
  for (int c = threadIdx.x; c < LH * LW; c += 256) {
    const int yy = y0 + c / LW, xx = x0 + c % LW;
    float d = 0.f;
    if (xx >= 0 && xx < w && yy >= 0 && yy < h) {
      const size_t q = (size_t)yy * w + xx;
      const float dq = depth[q];
      if ((!valid || valid[q] != 0) && dq > 0.f && dq <= 3.402823466e+38f) d = dq;   // NaN fails dq > 0, +inf the second test
    }
    s_c[c] = d > 0.f ? make_double2((double)d, 1.0 / (double)d) : make_double2(__builtin_nan(""), 0.0);
  }
  __syncthreads();
  const int tx = threadIdx.x % kTileW, ty = threadIdx.x / kTileW;
  const int x = blockIdx.x * kTileW + tx, y = blockIdx.y * kTileH + ty;
  if (x >= w || y >= h) return;
  const size_t hw = (size_t)h * w, p = (size_t)y * w + x;
  const int lc = (ty + R) * LW + tx + R;
  const double dc = s_c[lc].x;
  float nx = 0.f, ny = 0.f, nz = 0.f;
  unsigned char good = 0;
  if (dc == dc) {                                              // a valid centre
    const double lim = (double)jump * dc;                      // float x float: exact in fp64
    int n = 0, sx = 0, sy = 0, sxx = 0, sxy = 0, syy = 0;
    double b0 = 0.0, b1 = 0.0, b2 = 0.0;
#pragma unroll
    for (int dy = -R; dy <= R; ++dy) {
#pragma unroll
      for (int dx = -R; dx <= R; ++dx) {
        const double2 c = s_c[lc + dy * LW + dx];
        const bool enter = fabs(c.x - dc) <= lim;              // float - float: exact in fp64; false for a NaN depth
        const int e = enter ? 1 : 0;
        const double iv = enter ? c.y : 0.0;
        n += e;
        sx += dx * e; sy += dy * e; sxx += dx * dx * e; sxy += dx * dy * e; syy += dy * dy * e;
        if (dx != 0) b0 += (double)dx * iv;                    // adding 0 * iv would change nothing
        if (dy != 0) b1 += (double)dy * iv;
        b2 += iv;
      }
    }
    // S = [[sxx, sxy, sx], [sxy, syy, sy], [sx, sy, n]]; its adjugate and determinant in integers (|det| < 2^31 up to r = 4:
    // it is at most sxx syy n = 540 * 540 * 81)
    const long long a00 = (long long)syy * n - (long long)sy * sy, a01 = (long long)sx * sy - (long long)sxy * n,
                    a02 = (long long)sxy * sy - (long long)syy * sx, a11 = (long long)sxx * n - (long long)sx * sx,
                    a12 = (long long)sxy * sx - (long long)sxx * sy, a22 = (long long)sxx * syy - (long long)sxy * sxy;
    const long long det = (long long)sxx * a00 + (long long)sxy * a01 + (long long)sx * a02;
    const double t0 = ((double)a00 * b0 + (double)a01 * b1) + (double)a02 * b2;
    const double t1 = ((double)a01 * b0 + (double)a11 * b1) + (double)a12 * b2;
    const double t2 = ((double)a02 * b0 + (double)a12 * b1) + (double)a22 * b2;
    if (n >= min_pts && det != 0 && t2 > 0.0) {
      const double px = (double)x + 0.5, py = (double)y + 0.5;
      const double g0 = t0, g1 = t1, g2 = (t2 - t0 * px) - t1 * py;
      const double c0 = -(((double)cam.K[0] * g0 + (double)cam.K[3] * g1) + (double)cam.K[6] * g2);
      const double c1 = -(((double)cam.K[1] * g0 + (double)cam.K[4] * g1) + (double)cam.K[7] * g2);
      const double c2 = -(((double)cam.K[2] * g0 + (double)cam.K[5] * g1) + (double)cam.K[8] * g2);
      const double w0 = ((double)cam.R[0] * c0 + (double)cam.R[3] * c1) + (double)cam.R[6] * c2;
      const double w1 = ((double)cam.R[1] * c0 + (double)cam.R[4] * c1) + (double)cam.R[7] * c2;
      const double w2 = ((double)cam.R[2] * c0 + (double)cam.R[5] * c1) + (double)cam.R[8] * c2;
      const double nn = sqrt((w0 * w0 + w1 * w1) + w2 * w2);
      if (nn > 0.0 && nn <= 1.7976931348623157e308) {           // a NaN norm fails the first test
        nx = (float)(w0 / nn);
        ny = (float)(w1 / nn);
        nz = (float)(w2 / nn);
        good = 1;
      }
    }
  }
  normals[p] = nx;
  normals[hw + p] = ny;
  normals[2 * hw + p] = nz;
  ok[p] = good;
}

// Voxel v holds the points perm[start[v] .. start[v + 1]), exactly as in voxel_mean_kernel (registration.hip), whose loop,
// guards and fp64 expressions the position repeats so that the two agree bit for bit.
__global__ __launch_bounds__(256) void voxel_merge_kernel(const float* __restrict__ pts, const unsigned* __restrict__ colors,
                                                          const float* __restrict__ normals, long long n,
                                                          const long long* __restrict__ perm, const int* __restrict__ start,
                                                          long long n_voxels, float* __restrict__ out_pts,
                                                          unsigned* __restrict__ out_colors, float* __restrict__ out_normals,
                                                          int* __restrict__ out_counts) {
  for (long long v = (long long)blockIdx.x * blockDim.x + threadIdx.x; v < n_voxels; v += (long long)gridDim.x * blockDim.x) {
    const int b = start[v], e = start[v + 1];
    double sx = 0.0, sy = 0.0, sz = 0.0, mx = 0.0, my = 0.0, mz = 0.0;
    unsigned long long cr = 0, cg = 0, cb = 0;
    int cnt = 0;
    for (int j = b; j < e; ++j) {
      if (j < 0 || j >= n) continue;                       // offsets outside the permutation: read nothing
      const long long i = perm[j];
      if (i < 0 || i >= n) continue;
      sx += (double)pts[3 * i];
      sy += (double)pts[3 * i + 1];
      sz += (double)pts[3 * i + 2];
      const unsigned c = colors[i];
      cr += c & 255u;
      cg += (c >> 8) & 255u;
      cb += (c >> 16) & 255u;
      if (normals) {
        mx += (double)normals[3 * i];
        my += (double)normals[3 * i + 1];
        mz += (double)normals[3 * i + 2];
      }
      ++cnt;
    }
    const double c = (double)cnt;
    out_pts[3 * v] = (float)(sx / c);
    out_pts[3 * v + 1] = (float)(sy / c);
    out_pts[3 * v + 2] = (float)(sz / c);
    unsigned packed = 0;
    if (cnt > 0) {                                         // round half up: (2 sum + k) / (2 k), at most 255
      const unsigned long long k = (unsigned long long)cnt;
      packed = (unsigned)((2 * cr + k) / (2 * k)) | (unsigned)((2 * cg + k) / (2 * k)) << 8 |
               (unsigned)((2 * cb + k) / (2 * k)) << 16;
    }
    out_colors[v] = packed;
    out_counts[v] = cnt;
    if (normals) {
      const double nn = sqrt((mx * mx + my * my) + mz * mz);
      const bool good = nn > 0.0 && nn <= 1.7976931348623157e308;
      out_normals[3 * v] = good ? (float)(mx / nn) : 0.f;
      out_normals[3 * v + 1] = good ? (float)(my / nn) : 0.f;
      out_normals[3 * v + 2] = good ? (float)(mz / nn) : 0.f;
    }
  }
}

template <int R>
void launch_normals(const float* depth, const unsigned char* valid, const NormalCam& cam, int h, int w, float jump, int min_pts,
                    float* normals, unsigned char* ok, hipStream_t st) {
  hipLaunchKernelGGL(depth_normals_kernel<R>, dim3(cds_ceil_div(w, kTileW), cds_ceil_div(h, kTileH)), dim3(256), 0, st, depth,
                     valid, cam, h, w, jump, min_pts, normals, ok);
}

}  // namespace

extern "C" int cds_depth_normals_f32(const float* depth, const unsigned char* valid, const float* cam_host, int h, int w,
                                     int radius, float jump, int min_pts, float* normals, unsigned char* ok, void* stream) {
  if (!depth || !cam_host || !normals || !ok || h < 1 || w < 1 || (long long)h * w > 0x7fffffffLL || radius < 1 || radius > 4 ||
      !(jump > 0.f) || min_pts < 3 || min_pts > (2 * radius + 1) * (2 * radius + 1) || cds_ceil_div(h, kTileH) > 65535)
    return CDS_EINVAL;
  NormalCam cam;
  for (int i = 0; i < 9; ++i) cam.K[i] = cam_host[i];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) cam.R[3 * r + c] = cam_host[9 + 4 * r + c];
  hipStream_t st = (hipStream_t)stream;
  switch (radius) {
    case 1: launch_normals<1>(depth, valid, cam, h, w, jump, min_pts, normals, ok, st); break;
    case 2: launch_normals<2>(depth, valid, cam, h, w, jump, min_pts, normals, ok, st); break;
    case 3: launch_normals<3>(depth, valid, cam, h, w, jump, min_pts, normals, ok, st); break;
    default: launch_normals<4>(depth, valid, cam, h, w, jump, min_pts, normals, ok, st); break;
  }
  return cds_launch_status();
}

extern "C" int cds_voxel_merge_f32(const float* points, const unsigned* colors, const float* normals, long long n,
                                   const long long* perm, const int* start, long long n_voxels, float* out_points,
                                   unsigned* out_colors, float* out_normals, int* out_counts, void* stream) {
  if (n < 0 || n_voxels < 0 || n_voxels > n || n > 0x7fffffffLL) return CDS_EINVAL;
  if (n_voxels == 0) return 0;
  if (!points || !colors || !perm || !start || !out_points || !out_colors || !out_counts || (normals && !out_normals))
    return CDS_EINVAL;
  const long long blocks = (n_voxels + 255) / 256;
  hipLaunchKernelGGL(voxel_merge_kernel, dim3((unsigned)(blocks < 8192 ? blocks : 8192)), dim3(256), 0, (hipStream_t)stream,
                     points, colors, normals, n, perm, start, n_voxels, out_points, out_colors, out_normals, out_counts);
  return cds_launch_status();
}
