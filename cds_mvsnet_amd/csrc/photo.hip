// A mesh scored against the photographs of its scan (rules S and C are stated in include/cds_mvsnet_hip.h): the
// textured render of the rasteriser's face map, and PSNR / SSIM sums of two images under a mask.
//
//   cds_photo_shade    one thread per pixel: rule S, the surface point of the rasteriser's rule 6 looked up in the face's atlas cell
//   cds_photo_scores   one workgroup per tile of kTile x kTile windows: rule C.  The tile of both images and the mask, with the
//                      10-pixel halo of the 11 x 11 window, is staged in LDS once; per channel the row pass of the five moment
//                      maps goes into LDS and the column pass comes out of it.  A second kernel adds the tiles' records.
//
// Arithmetic is fp64 with the bracketing of the rules (the library is built with -ffp-contract=off); decisions are made on
// integers.  There is no atomic: a tile's sums are a fixed tree over its 256 threads, a view's sums a fixed walk and tree over its
// tiles, so a view's numbers are the same bits run to run.  Every index that comes from data (face, vertex, uv) is tested against
// its range before it is used, and the tile loader never reads outside an image.
#include "mesh_common.hpp"

namespace {

using cds_mesh::blocks_for;
using cds_mesh::kThreads;

constexpr int kCam = CDS_RASTER_CAM;

// ---------------------------------------------------------------------------------------------------------------------- shade
struct ShadeArgs {
  const float* vertices;
  long long n_vertices;
  const int* faces;
  long long n_faces;
  const int* uv;
  const unsigned char* atlas;
  int atlas_h, atlas_w;
  const double* cams;
  const int* face;
  int h, w;
  unsigned char* image;
};

// One coordinate of rule S inside the cell [o, o + c): the two texels and the weight of the upper one.
__device__ __forceinline__ void cell_sample(double t, long long o, long long c, int& lo, int& hi, double& f) {
  const double low = (double)o + 0.5, high = (double)(o + c) - 0.5;
  double tc = t > low ? t : low;                                         // a NaN takes the lower bound
  tc = tc < high ? tc : high;
  const double x = tc - 0.5, xl = floor(x);
  lo = (int)xl;
  hi = lo + 1 < (int)(o + c - 1) ? lo + 1 : (int)(o + c - 1);
  f = x - xl;
}

__global__ __launch_bounds__(kThreads) void photo_shade_kernel(const ShadeArgs a) {
  const long long p = (long long)blockIdx.x * kThreads + threadIdx.x, hw = (long long)a.h * a.w;
  if (p >= hw) return;
  const int view = blockIdx.y;
  const size_t o = (size_t)view * hw + p;
  unsigned char rgb[3] = {0, 0, 0};
  const long long f = a.face[o];
  int idx[3] = {0, 0, 0};
  if (f >= 0 && f < a.n_faces && cds_mesh::load_face(a.faces, f, a.n_vertices, idx)) {
    const int* t = a.uv + 6 * f;
    const long long ua[2] = {t[0], t[1]}, ub[2] = {t[2], t[3]}, uc[2] = {t[4], t[5]};
    const long long x0 = ua[0] - 1, y0 = ua[1] - 1, c = ub[0] - ua[0] + 2;
    if (c >= 4 && x0 >= 0 && y0 >= 0 && x0 + c <= a.atlas_w && y0 + c <= a.atlas_h) {
      const double* cam = a.cams + (long long)view * kCam;
      double X[3][3];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const float* q = a.vertices + 3 * (long long)idx[k];
        const cds_mesh::ViewPoint vp = cds_mesh::view_point(cam, q[0], q[1], q[2]);                  // rule 1
        X[k][0] = vp.xc0; X[k][1] = vp.xc1; X[k][2] = vp.z;
      }
      const cds_mesh::FacePlane pl = cds_mesh::face_plane(X[0], X[1], X[2]);
      double rx, ry, wt[3];
      const double zf = cds_mesh::fragment_depth(pl, cam, (int)(p % a.w), (int)(p / a.w), rx, ry);
      cds_mesh::surface_weights(pl, X[0], X[1], X[2], zf, rx, ry, wt);
      const double tx = (wt[0] * (double)ua[0] + wt[1] * (double)ub[0]) + wt[2] * (double)uc[0];
      const double ty = (wt[0] * (double)ua[1] + wt[1] * (double)ub[1]) + wt[2] * (double)uc[1];
      int xl, xh, yl, yh;
      double fx, fy;
      cell_sample(tx, x0, c, xl, xh, fx);
      cell_sample(ty, y0, c, yl, yh, fy);
      const double gx = 1.0 - fx, gy = 1.0 - fy;
      const double w00 = gx * gy, w10 = fx * gy, w01 = gx * fy, w11 = fx * fy;
      const size_t aw = (size_t)a.atlas_w;
      const unsigned char *p00 = a.atlas + 3 * ((size_t)yl * aw + xl), *p10 = a.atlas + 3 * ((size_t)yl * aw + xh),
                          *p01 = a.atlas + 3 * ((size_t)yh * aw + xl), *p11 = a.atlas + 3 * ((size_t)yh * aw + xh);
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        const double val = ((w00 * (double)p00[ch] + w10 * (double)p10[ch]) + w01 * (double)p01[ch]) + w11 * (double)p11[ch];
        rgb[ch] = (unsigned char)(int)floor(val + 0.5);
      }
    }
  }
  unsigned char* out = a.image + 3 * o;
  out[0] = rgb[0]; out[1] = rgb[1]; out[2] = rgb[2];
}

// -------------------------------------------------------------------------------------------------------------------- compare
constexpr int kTile = CDS_PHOTO_TILE;                                    // windows per tile side: kTile x kTile = kThreads
constexpr int kWin = 11;                                                 // the window side
constexpr int kIn = kTile + kWin - 1;                                    // pixels per side that a tile's windows read
constexpr int kFields = CDS_PHOTO_RECORD;                                // n_px, sse[3], n_win as int64; ssim_sum[3] as fp64 bits
constexpr int kIntFields = 5;
static_assert(kTile * kTile == kThreads, "one thread per window of a tile");

struct Gauss {
  double g[kWin];
};

struct ComparePlanes {
  double r[5][kIn][kTile];                                               // the row pass of one channel's five moments
};

union CompareScratch {
  ComparePlanes planes;
  long long red[kFields][kThreads];                                      // the tile's sums, after the last column pass
};

// The fixed tree over the workgroup's 256 values of every field: ints exact, doubles in this order every run.
__device__ __forceinline__ void tree_sum(long long (*red)[kThreads], int tid) {
  for (int s = kThreads / 2; s >= 1; s >>= 1) {
    __syncthreads();
    if (tid < s) {
#pragma unroll
      for (int f = 0; f < kIntFields; ++f) red[f][tid] += red[f][tid + s];
#pragma unroll
      for (int f = kIntFields; f < kFields; ++f)
        red[f][tid] = __double_as_longlong(__longlong_as_double(red[f][tid]) + __longlong_as_double(red[f][tid + s]));
    }
  }
  __syncthreads();
}

__global__ __launch_bounds__(kThreads) void photo_scores_kernel(const unsigned char* __restrict__ a,
                                                                const unsigned char* __restrict__ b,
                                                                const unsigned char* __restrict__ mask, const Gauss gw, int h, int w,
                                                                int tiles_x, long long* __restrict__ rec,
                                                                double* __restrict__ ssim_map) {
  __shared__ unsigned char sa[3][kIn][kIn], sb[3][kIn][kIn], sm[kIn][kIn], mrow[kIn][kTile];
  __shared__ CompareScratch sc;
  const int tid = threadIdx.x, view = blockIdx.y;
  const int x0 = (int)(blockIdx.x % tiles_x) * kTile, y0 = (int)(blockIdx.x / tiles_x) * kTile;
  const size_t hw = (size_t)h * w;
  const unsigned char* __restrict__ av = a + 3 * (size_t)view * hw;
  const unsigned char* __restrict__ bv = b + 3 * (size_t)view * hw;
  const unsigned char* __restrict__ mv = mask + (size_t)view * hw;

  // the tile and its halo, once: a row of the tile is 3 kIn consecutive bytes of the image; outside the image 0, and mask 0
  for (int i = tid; i < kIn * 3 * kIn; i += kThreads) {
    const int row = i / (3 * kIn), col = i - row * (3 * kIn), px = col / 3, ch = col - 3 * px;
    const int gy = y0 + row, gx = x0 + px;
    unsigned char va = 0, vb = 0;
    if (gy < h && gx < w) {
      const size_t q = 3 * ((size_t)gy * w + gx) + ch;
      va = av[q]; vb = bv[q];
    }
    sa[ch][row][px] = va; sb[ch][row][px] = vb;
  }
  for (int i = tid; i < kIn * kIn; i += kThreads) {
    const int row = i / kIn, px = i - row * kIn;
    const int gy = y0 + row, gx = x0 + px;
    sm[row][px] = (gy < h && gx < w && mv[(size_t)gy * w + gx] != 0) ? 1 : 0;
  }
  __syncthreads();

  const int tx = tid % kTile, ty = tid / kTile;
  const int wx = x0 + tx, wy = y0 + ty;                                  // this thread's pixel, and the top-left of its window
  long long n_px = 0, sse[3] = {0, 0, 0}, n_win = 0;
  double ssim_sum[3] = {0.0, 0.0, 0.0};
  if (sm[ty][tx]) {                                                      // 0 outside the image
    n_px = 1;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const int d = (int)sa[ch][ty][tx] - (int)sb[ch][ty][tx];
      sse[ch] = d * d;
    }
  }
  for (int i = tid; i < kIn * kTile; i += kThreads) {
    const int row = i / kTile, col = i - row * kTile;
    int cnt = 0;
#pragma unroll
    for (int k = 0; k < kWin; ++k) cnt += sm[row][col + k];
    mrow[row][col] = (unsigned char)cnt;
  }
  __syncthreads();
  const bool exists = wx <= w - kWin && wy <= h - kWin;
  int cnt = 0;
#pragma unroll
  for (int k = 0; k < kWin; ++k) cnt += mrow[ty + k][tx];
  const bool counts = exists && cnt == kWin * kWin;
  n_win = counts ? 1 : 0;
  const size_t mw = exists ? (size_t)(w - kWin + 1) : 0, mh = exists ? (size_t)(h - kWin + 1) : 0;

  for (int ch = 0; ch < 3; ++ch) {
    for (int i = tid; i < kIn * kTile; i += kThreads) {
      const int row = i / kTile, col = i - row * kTile;
      double r[5];
#pragma unroll
      for (int k = 0; k < kWin; ++k) {
        const double va = (double)sa[ch][row][col + k], vb = (double)sb[ch][row][col + k];
        const double m[5] = {va, vb, va * va, vb * vb, va * vb};
#pragma unroll
        for (int q = 0; q < 5; ++q) r[q] = k == 0 ? gw.g[0] * m[q] : r[q] + gw.g[k] * m[q];
      }
#pragma unroll
      for (int q = 0; q < 5; ++q) sc.planes.r[q][row][col] = r[q];
    }
    __syncthreads();
    if (exists) {
      double ssim = __longlong_as_double(0x7ff8000000000000ll);          // a window that does not count
      if (counts) {
        double e[5];
#pragma unroll
        for (int k = 0; k < kWin; ++k)
#pragma unroll
          for (int q = 0; q < 5; ++q) {
            const double v = sc.planes.r[q][ty + k][tx];
            e[q] = k == 0 ? gw.g[0] * v : e[q] + gw.g[k] * v;
          }
        const double mua = e[0], mub = e[1];
        const double va = e[2] - mua * mua, vb = e[3] - mub * mub, vab = e[4] - mua * mub;
        const double C1 = 6.5025, C2 = 58.5225;
        const double num = ((2.0 * mua) * mub + C1) * (2.0 * vab + C2);
        const double den = ((mua * mua + mub * mub) + C1) * ((va + vb) + C2);
        ssim = num / den;
        ssim_sum[ch] = ssim;
      }
      if (ssim_map) ssim_map[(((size_t)view * 3 + ch) * mh + wy) * mw + wx] = ssim;
    }
    __syncthreads();                                                     // the planes are written again
  }

  sc.red[0][tid] = n_px;
  sc.red[1][tid] = sse[0]; sc.red[2][tid] = sse[1]; sc.red[3][tid] = sse[2];
  sc.red[4][tid] = n_win;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) sc.red[kIntFields + ch][tid] = __double_as_longlong(ssim_sum[ch]);
  tree_sum(sc.red, tid);
  if (tid < kFields) rec[((size_t)view * gridDim.x + blockIdx.x) * kFields + tid] = sc.red[tid][0];
}

// Workgroup v adds the records of view v's tiles: thread t walks the tiles t, t + 256, ... in that order, then the tree.
__global__ __launch_bounds__(kThreads) void photo_scores_reduce_kernel(const long long* __restrict__ rec, long long tiles,
                                                                       long long* __restrict__ counts,
                                                                       double* __restrict__ ssim_sum) {
  __shared__ long long red[kFields][kThreads];
  const int tid = threadIdx.x;
  const long long* __restrict__ r = rec + (size_t)blockIdx.x * tiles * kFields;
  long long si[kIntFields] = {0, 0, 0, 0, 0};
  double sd[kFields - kIntFields] = {0.0, 0.0, 0.0};
  for (long long i = tid; i < tiles; i += kThreads) {
#pragma unroll
    for (int f = 0; f < kIntFields; ++f) si[f] += r[i * kFields + f];
#pragma unroll
    for (int f = kIntFields; f < kFields; ++f) sd[f - kIntFields] += __longlong_as_double(r[i * kFields + f]);
  }
#pragma unroll
  for (int f = 0; f < kIntFields; ++f) red[f][tid] = si[f];
#pragma unroll
  for (int f = kIntFields; f < kFields; ++f) red[f][tid] = __double_as_longlong(sd[f - kIntFields]);
  tree_sum(red, tid);
  if (tid < kIntFields) counts[(size_t)blockIdx.x * kIntFields + tid] = red[tid][0];
  else if (tid < kFields) ssim_sum[(size_t)blockIdx.x * 3 + (tid - kIntFields)] = __longlong_as_double(red[tid][0]);
}

bool map_ok(int n_views, int h, int w) {
  return n_views >= 1 && n_views <= CDS_RASTER_MAX_CHUNK && h >= 1 && w >= 1 && (long long)h * w <= 0x7fffffffLL;
}

long long tiles_of(int h, int w) { return (long long)((h + kTile - 1) / kTile) * ((w + kTile - 1) / kTile); }

}  // namespace

extern "C" int cds_photo_shade(const float* vertices, long long n_vertices, const int* faces, long long n_faces, const int* uv,
                               const unsigned char* atlas, int atlas_h, int atlas_w, const double* cams, int n_views,
                               const int* face, int h, int w, unsigned char* image, void* stream) {
  bool size_ok = atlas_h == 0 && atlas_w == 0;                           // no atlas: every pixel takes the fall-back
  for (int s = 2; (1 << s) <= CDS_TEXTURE_MAX_SIZE; ++s)
    if ((1 << s) == atlas_w && (atlas_h == atlas_w || 2 * atlas_h == atlas_w)) size_ok = true;
  if (!cds_mesh::sizes_ok(n_vertices, n_faces) || !map_ok(n_views, h, w) || !size_ok) return CDS_EINVAL;
  if (!face || !image || !cams) return CDS_EINVAL;
  const bool empty = n_faces == 0 || atlas_w == 0;
  if (!empty && (!vertices || !faces || !uv || !atlas)) return CDS_EINVAL;
  ShadeArgs a;
  a.vertices = vertices; a.n_vertices = n_vertices; a.faces = faces; a.n_faces = empty ? 0 : n_faces; a.uv = uv; a.atlas = atlas;
  a.atlas_h = atlas_h; a.atlas_w = atlas_w; a.cams = cams; a.face = face; a.h = h; a.w = w; a.image = image;
  hipLaunchKernelGGL(photo_shade_kernel, dim3(blocks_for((long long)h * w), (unsigned)n_views), dim3(kThreads), 0,
                     (hipStream_t)stream, a);
  return cds_launch_status();
}

extern "C" int cds_photo_scores(const unsigned char* a, const unsigned char* b, const unsigned char* mask, const double* g,
                                int n_views, int h, int w, long long* ws, long long ws_words, long long* counts, double* ssim_sum,
                                double* ssim_map, void* stream) {
  if (!map_ok(n_views, h, w) || !a || !b || !mask || !g || !ws || !counts || !ssim_sum) return CDS_EINVAL;
  const long long tiles = tiles_of(h, w);
  if (ws_words < (long long)n_views * tiles * kFields) return CDS_EINVAL;
  Gauss gw;
  for (int k = 0; k < kWin; ++k) gw.g[k] = g[k];
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(photo_scores_kernel, dim3((unsigned)tiles, (unsigned)n_views), dim3(kThreads), 0, st, a, b, mask, gw, h, w,
                     (w + kTile - 1) / kTile, ws, ssim_map);
  hipLaunchKernelGGL(photo_scores_reduce_kernel, dim3((unsigned)n_views), dim3(kThreads), 0, st, ws, tiles, counts, ssim_sum);
  return cds_launch_status();
}
