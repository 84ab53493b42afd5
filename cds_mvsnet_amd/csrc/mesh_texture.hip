// A texture atlas for a mesh from the images of a scan (the rule is stated in include/cds_mvsnet_hip.h): one view
// and one square cell per face, every texel a function of the input alone.
//
//   cds_texture_votes   one thread per (view, pixel) of the rasteriser's face and valid maps: rule 1, integer atomic adds
//   cds_texture_best    one thread per face: folds a chunk's votes into the running key of rule 2
//   cds_texture_cells   one thread per face: the view of rule 2 from the key, the cell size of rule 3
//   cds_texture_place   one thread per face of the sorted order: rules 4 and 5, the cell's origin from its Morton start, the UV
//   cds_texture_fill    one thread per atlas texel, or per 4 x 4 unit: rule 6
//
// Decisions are made in integers or fp64 with the bracketing of the rule (the library is built with -ffp-contract=off).  The only
// atomic is the integer add of the votes: a count does not depend on the order of its additions.  Every loop has its bound fixed
// before it starts, and every index that comes from data (face, view, sorted position, cell origin, pixel) is tested against its
// range before it is used: wrong tables leave texels black, they are never followed outside a buffer.
#include "mesh_common.hpp"

namespace {

using cds_mesh::blocks_for;
using cds_mesh::kThreads;

constexpr int kCam = CDS_RASTER_CAM;

// ---------------------------------------------------------------------------------------------------------------------- votes
// kRuns: neighbouring pixels of a row mostly hold the same face; the first lane of a run of equal faces inside the wave adds the
// run's length.  Without it every counted pixel makes its own add.
template <bool kRuns>
__global__ __launch_bounds__(kThreads) void texture_votes_kernel(const int* __restrict__ face,
                                                                 const unsigned char* __restrict__ valid, long long hw,
                                                                 long long n_faces, int* __restrict__ votes) {
  const long long p = (long long)blockIdx.x * kThreads + threadIdx.x;
  const int view = blockIdx.y;
  int f = -1;
  if (p < hw) {
    const size_t o = (size_t)view * hw + p;
    if (valid[o] != 0) f = face[o];
  }
  if (f < 0 || f >= n_faces) f = -1;                                     // a pixel without a vote
  int* row = votes + (long long)view * n_faces;
  if (!kRuns) {
    if (f >= 0) atomicAdd(row + f, 1);
    return;
  }
  const int lane = threadIdx.x & 63;                                     // every lane of the wave reaches the shuffle
  const int prev = __shfl_up(f, 1);
  const bool head = lane == 0 || prev != f;
  const unsigned long long heads = __ballot(head);
  const unsigned long long after = lane == 63 ? 0ull : heads >> (lane + 1);
  const int len = after ? __ffsll(after) : 64 - lane;                    // up to the next head, or the end of the wave
  if (head && f >= 0) atomicAdd(row + f, len);
}

// ----------------------------------------------------------------------------------------------------------------------- best
__global__ __launch_bounds__(kThreads) void texture_best_kernel(const int* __restrict__ votes, long long n_faces, int n_views,
                                                                int view0, unsigned long long* __restrict__ key) {
  const long long f = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (f >= n_faces) return;
  unsigned long long k = key[f];
  for (int v = 0; v < n_views; ++v) {
    const int cnt = votes[(long long)v * n_faces + f];
    const unsigned long long cand = ((unsigned long long)(unsigned)(cnt > 0 ? cnt : 0) << 32) |
                                    (unsigned long long)(0xffffffffu - (unsigned)(view0 + v));
    k = cand > k ? cand : k;
  }
  key[f] = k;
}

// ---------------------------------------------------------------------------------------------------------------------- cells
__global__ __launch_bounds__(kThreads) void texture_cells_kernel(const float* __restrict__ vertices, long long n_vertices,
                                                                 const int* __restrict__ faces, long long n_faces,
                                                                 const double* __restrict__ cams, int n_views,
                                                                 const unsigned long long* __restrict__ key, long long min_px,
                                                                 double scale, int max_cell, int steps, int* __restrict__ view_out,
                                                                 int* __restrict__ cell) {
  const long long f = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (f >= n_faces) return;
  const unsigned long long k = key[f];
  const long long count = (long long)(k >> 32), view = (long long)(0xffffffffu - (unsigned)(k & 0xffffffffull));
  const bool seen = count >= min_px && view < n_views;
  int c = 4, idx[3];
  if (seen && cds_mesh::load_face(faces, f, n_vertices, idx)) {
    const double* cam = cams + view * kCam;
    long long X[3], Y[3];
    bool usable = true;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const float* q = vertices + 3 * (long long)idx[i];
      int sx, sy;
      usable = cds_mesh::snap_point(cds_mesh::view_point(cam, q[0], q[1], q[2]), sx, sy) && usable;
      X[i] = sx; Y[i] = sy;
    }
    if (usable) {
      long long L2 = 0;                                                  // < 2^59: |X|, |Y| < 2^28
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        const int j = i == 2 ? 0 : i + 1;
        const long long dx = X[j] - X[i], dy = Y[j] - Y[i], e = dx * dx + dy * dy;
        L2 = e > L2 ? e : L2;
      }
      const double t = (scale * scale) * (double)L2;
      // n <= c - 2  iff  (256 (c - 2))^2 >= t: the smallest power of two that holds n + 2, without a square root
      bool found = false;
      for (int s = 0; s < steps; ++s) {                                  // steps = log2(max_cell / 4): the classes below max_cell
        const double m = 256.0 * (double)((4 << s) - 2);
        if (!found && m * m >= t) { c = 4 << s; found = true; }
      }
      if (!found) c = max_cell;
    }
  }
  view_out[f] = seen ? (int)view : -1;
  cell[3 * f] = 0; cell[3 * f + 1] = 0; cell[3 * f + 2] = c;
}

// ---------------------------------------------------------------------------------------------------------------------- place
// The even bits of a Morton index, packed.
__device__ __forceinline__ unsigned even_bits(unsigned long long m) {
  m &= 0x5555555555555555ull;
  m = (m | (m >> 1)) & 0x3333333333333333ull;
  m = (m | (m >> 2)) & 0x0f0f0f0f0f0f0f0full;
  m = (m | (m >> 4)) & 0x00ff00ff00ff00ffull;
  m = (m | (m >> 8)) & 0x0000ffff0000ffffull;
  m = (m | (m >> 16)) & 0x00000000ffffffffull;
  return (unsigned)m;
}

// x to the even bits of a 32-bit index (x < 2^16).
__device__ __forceinline__ unsigned spread_bits(unsigned x) {
  x &= 0xffffu;
  x = (x | (x << 8)) & 0x00ff00ffu;
  x = (x | (x << 4)) & 0x0f0f0f0fu;
  x = (x | (x << 2)) & 0x33333333u;
  x = (x | (x << 1)) & 0x55555555u;
  return x;
}

__device__ __forceinline__ bool cell_size_ok(int c, int max_cell) { return c >= 4 && c <= max_cell && (c & (c - 1)) == 0; }

__global__ __launch_bounds__(kThreads) void texture_place_kernel(const long long* __restrict__ order,
                                                                 const long long* __restrict__ starts, long long n_faces,
                                                                 long long total, int max_cell, int* __restrict__ cell,
                                                                 int* __restrict__ uv) {
  const long long k = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (k >= n_faces) return;
  const long long f = order[k], start = starts[k];
  if (f < 0 || f >= n_faces) return;
  const int c = cell[3 * f + 2];
  if (!cell_size_ok(c, max_cell)) return;
  const long long units = (long long)(c >> 2) * (c >> 2);
  if (start < 0 || start > total - units || (start & (units - 1)) != 0) return;     // not a start of rule 4
  const int x = 4 * (int)even_bits((unsigned long long)start), y = 4 * (int)even_bits((unsigned long long)start >> 1);
  cell[3 * f] = x; cell[3 * f + 1] = y;
  int* t = uv + 6 * f;
  t[0] = x + 1;     t[1] = y + 1;
  t[2] = x + c - 1; t[3] = y + 1;
  t[4] = x + 1;     t[5] = y + c - 1;
}

// ----------------------------------------------------------------------------------------------------------------------- fill
struct FillArgs {
  const float* vertices;
  const unsigned char* colors;
  long long n_vertices;
  const int* faces;
  long long n_faces;
  const double* cams;
  const unsigned char* images;                                           // every view's [h][w][3] bytes, at its offset of views
  long long image_bytes;
  const long long* views;                                                // [n_views][3]: byte offset, h, w
  int n_views;
  const int* view;
  const int* cell;
  const long long* order;
  const long long* starts;
  long long total;
  int max_cell, log2_w, height;
  unsigned char* atlas;
};

// What the texels of one cell share.
struct CellFace {
  int x0, y0, c, view;                                                   // view < 0: the vertex-colour rule
  int h, w;                                                              // the view's image
  const unsigned char* img;
  double P[3][3];                                                        // the corners A, B, C
  int idx[3];
};

// The last sorted position whose start is <= m (mesh_sample.hip's search); starts[0] == 0 <= m is the caller's.
__device__ __forceinline__ long long owner(const long long* __restrict__ starts, long long lo, long long hi, long long m) {
  while (lo < hi) {
    const long long mid = lo + (hi - lo + 1) / 2;
    if (starts[mid] <= m) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// The cell that holds unit (ux, uy); false where the unit belongs to none.
__device__ __forceinline__ bool load_cell(const FillArgs& a, int ux, int uy, CellFace& cf) {
  const long long m = (long long)(spread_bits((unsigned)ux) | (spread_bits((unsigned)uy) << 1));
  if (m >= a.total || a.starts[0] > m) return false;
  const long long k = owner(a.starts, 0, a.n_faces - 1, m);
  const long long f = a.order[k];
  if (f < 0 || f >= a.n_faces) return false;
  cf.x0 = a.cell[3 * f]; cf.y0 = a.cell[3 * f + 1]; cf.c = a.cell[3 * f + 2];
  if (!cell_size_ok(cf.c, a.max_cell)) return false;
  const int i = 4 * ux - cf.x0, j = 4 * uy - cf.y0;
  if (i < 0 || i >= cf.c || j < 0 || j >= cf.c) return false;            // tables that do not belong together
  if (!cds_mesh::load_face(a.faces, f, a.n_vertices, cf.idx)) return false;
  const int v = a.view[f];
  cf.view = -1; cf.h = 1; cf.w = 1; cf.img = a.images;
  if (v >= 0 && v < a.n_views) {
    const long long off = a.views[3 * (long long)v], h = a.views[3 * (long long)v + 1], w = a.views[3 * (long long)v + 2];
    // an image that does not lie inside the buffer is not read: the face keeps its vertex colours
    if (h >= 1 && w >= 1 && h * w <= 0x7fffffffLL && off >= 0 && off <= a.image_bytes - 3 * h * w) {
      cf.view = v; cf.h = (int)h; cf.w = (int)w; cf.img = a.images + off;
    }
  }
#pragma unroll
  for (int q = 0; q < 3; ++q)
#pragma unroll
    for (int d = 0; d < 3; ++d) cf.P[q][d] = a.vertices[3 * (long long)cf.idx[q] + d];
  return true;
}

// Rule 6 for texel (i, j) of the cell.
__device__ __forceinline__ void texel(const FillArgs& a, const CellFace& cf, int i, int j, unsigned char rgb[3]) {
  const double den = (double)(cf.c - 2);
  const double wb = (((double)i + 0.5) - 1.0) / den, wc = (((double)j + 0.5) - 1.0) / den, wa = (1.0 - wb) - wc;
  if (cf.view >= 0) {
    double P[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) P[d] = (wa * cf.P[0][d] + wb * cf.P[1][d]) + wc * cf.P[2][d];
    const cds_mesh::ViewPoint p = cds_mesh::view_point(a.cams + (long long)cf.view * kCam, P[0], P[1], P[2]);
    if (p.z > 0.0 && cds_mesh::is_finite(p.u) && cds_mesh::is_finite(p.v)) {
      const int w = cf.w, h = cf.h;
      const double wmax = (double)w - 0.5, hmax = (double)h - 0.5;
      const double uc = p.u < 0.5 ? 0.5 : (p.u > wmax ? wmax : p.u), vc = p.v < 0.5 ? 0.5 : (p.v > hmax ? hmax : p.v);
      const double x = uc - 0.5, y = vc - 0.5;
      int x0 = (int)floor(x), y0 = (int)floor(y);
      x0 = x0 < 0 ? 0 : (x0 > w - 1 ? w - 1 : x0);                       // already there; the image is never read outside
      y0 = y0 < 0 ? 0 : (y0 > h - 1 ? h - 1 : y0);
      const int x1 = x0 + 1 < w ? x0 + 1 : x0, y1 = y0 + 1 < h ? y0 + 1 : y0;
      const double fx = x - (double)x0, fy = y - (double)y0, gx = 1.0 - fx, gy = 1.0 - fy;
      const double w00 = gx * gy, w10 = fx * gy, w01 = gx * fy, w11 = fx * fy;
      const unsigned char* img = cf.img;
      const unsigned char *p00 = img + 3 * ((size_t)y0 * w + x0), *p10 = img + 3 * ((size_t)y0 * w + x1),
                          *p01 = img + 3 * ((size_t)y1 * w + x0), *p11 = img + 3 * ((size_t)y1 * w + x1);
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        const double val = ((w00 * (double)p00[ch] + w10 * (double)p10[ch]) + w01 * (double)p01[ch]) + w11 * (double)p11[ch];
        rgb[ch] = (unsigned char)(int)floor(val + 0.5);
      }
      return;
    }
  }
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    const double ca = a.colors[3 * (long long)cf.idx[0] + ch], cb = a.colors[3 * (long long)cf.idx[1] + ch],
                 cc = a.colors[3 * (long long)cf.idx[2] + ch];
    const double val = (wa * ca + wb * cb) + wc * cc;
    const double cl = val > 0.0 ? (val < 255.0 ? val : 255.0) : 0.0;     // NaN -> 0
    rgb[ch] = (unsigned char)(int)floor(cl + 0.5);
  }
}

// One thread per texel: a wave writes 192 consecutive bytes of a row.
__global__ __launch_bounds__(kThreads) void texture_fill_texel_kernel(const FillArgs a) {
  const long long t = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (t >= ((long long)a.height << a.log2_w)) return;
  const int x = (int)(t & ((1ll << a.log2_w) - 1)), y = (int)(t >> a.log2_w);
  unsigned char rgb[3] = {0, 0, 0};
  CellFace cf;
  if (load_cell(a, x >> 2, y >> 2, cf)) texel(a, cf, x - cf.x0, y - cf.y0, rgb);
  unsigned char* o = a.atlas + 3 * t;
  o[0] = rgb[0]; o[1] = rgb[1]; o[2] = rgb[2];
}

// One thread per 4 x 4 unit: one search for 16 texels; every row of the unit is 12 bytes, written as three words.
__global__ __launch_bounds__(kThreads) void texture_fill_unit_kernel(const FillArgs a) {
  const long long t = (long long)blockIdx.x * kThreads + threadIdx.x;
  const int log2_uw = a.log2_w - 2;
  if (t >= ((long long)(a.height >> 2) << log2_uw)) return;
  const int ux = (int)(t & ((1ll << log2_uw) - 1)), uy = (int)(t >> log2_uw);
  CellFace cf;
  const bool owned = load_cell(a, ux, uy, cf);
  for (int r = 0; r < 4; ++r) {
    unsigned word[3] = {0u, 0u, 0u};
    if (owned) {
      unsigned char row[12];
#pragma unroll
      for (int q = 0; q < 4; ++q) texel(a, cf, 4 * ux + q - cf.x0, 4 * uy + r - cf.y0, row + 3 * q);
#pragma unroll
      for (int q = 0; q < 3; ++q)
        word[q] = (unsigned)row[4 * q] | ((unsigned)row[4 * q + 1] << 8) | ((unsigned)row[4 * q + 2] << 16) |
                  ((unsigned)row[4 * q + 3] << 24);
    }
    unsigned* o = reinterpret_cast<unsigned*>(a.atlas + 3 * ((((long long)(4 * uy + r)) << a.log2_w) + 4 * ux));
    o[0] = word[0]; o[1] = word[1]; o[2] = word[2];
  }
}

bool map_ok(int n_views, int h, int w) {
  return n_views >= 1 && n_views <= CDS_RASTER_MAX_CHUNK && h >= 1 && w >= 1 && (long long)h * w <= 0x7fffffffLL;
}

// max_cell: a power of two in 4 .. CDS_TEXTURE_MAX_CELL -> log2(max_cell / 4); -1 for another value.
int cell_steps(int max_cell) {
  for (int s = 0; (4 << s) <= CDS_TEXTURE_MAX_CELL; ++s)
    if ((4 << s) == max_cell) return s;
  return -1;
}

}  // namespace

extern "C" int cds_texture_votes(const int* face, const unsigned char* valid, int n_views, int h, int w, long long n_faces,
                                 int* votes, int runs, void* stream) {
  if (!map_ok(n_views, h, w) || !cds_mesh::sizes_ok(n_faces, 0) || (runs != 0 && runs != 1)) return CDS_EINVAL;
  if (n_faces == 0) return 0;
  if (!face || !valid || !votes) return CDS_EINVAL;
  const long long hw = (long long)h * w;
  const dim3 grid(blocks_for(hw), (unsigned)n_views);
  if (runs)
    hipLaunchKernelGGL(texture_votes_kernel<true>, grid, dim3(kThreads), 0, (hipStream_t)stream, face, valid, hw, n_faces, votes);
  else
    hipLaunchKernelGGL(texture_votes_kernel<false>, grid, dim3(kThreads), 0, (hipStream_t)stream, face, valid, hw, n_faces, votes);
  return cds_launch_status();
}

extern "C" int cds_texture_best(const int* votes, long long n_faces, int n_views, int view0, unsigned long long* key, void* stream) {
  if (!cds_mesh::sizes_ok(n_faces, 0) || n_views < 1 || n_views > CDS_RASTER_MAX_CHUNK || view0 < 0 ||
      (long long)view0 + n_views > 0x7fffffffLL)
    return CDS_EINVAL;
  if (n_faces == 0) return 0;
  if (!votes || !key) return CDS_EINVAL;
  hipLaunchKernelGGL(texture_best_kernel, dim3(blocks_for(n_faces)), dim3(kThreads), 0, (hipStream_t)stream, votes, n_faces, n_views,
                     view0, key);
  return cds_launch_status();
}

extern "C" int cds_texture_cells(const float* vertices, long long n_vertices, const int* faces, long long n_faces, const double* cams,
                                 int n_views, const unsigned long long* key, long long min_px, double scale, int max_cell,
                                 int* view, int* cell, void* stream) {
  const int steps = cell_steps(max_cell);
  if (!cds_mesh::sizes_ok(n_vertices, n_faces) || n_views < 1 || min_px < 1 || !cds_mesh::finite_pos(scale) || steps < 0)
    return CDS_EINVAL;
  if (n_faces == 0) return 0;
  if (!vertices || !faces || !cams || !key || !view || !cell) return CDS_EINVAL;
  hipLaunchKernelGGL(texture_cells_kernel, dim3(blocks_for(n_faces)), dim3(kThreads), 0, (hipStream_t)stream, vertices, n_vertices,
                     faces, n_faces, cams, n_views, key, min_px, scale, max_cell, steps, view, cell);
  return cds_launch_status();
}

extern "C" int cds_texture_place(const long long* order, const long long* starts, long long n_faces, long long total, int max_cell,
                                 int* cell, int* uv, void* stream) {
  if (!cds_mesh::sizes_ok(n_faces, 0) || total < 0 || total > CDS_TEXTURE_MAX_UNITS || cell_steps(max_cell) < 0) return CDS_EINVAL;
  if (n_faces == 0) return 0;
  if (!order || !starts || !cell || !uv) return CDS_EINVAL;
  hipLaunchKernelGGL(texture_place_kernel, dim3(blocks_for(n_faces)), dim3(kThreads), 0, (hipStream_t)stream, order, starts, n_faces,
                     total, max_cell, cell, uv);
  return cds_launch_status();
}

extern "C" int cds_texture_fill(const float* vertices, const unsigned char* colors, long long n_vertices, const int* faces,
                                long long n_faces, const double* cams, const unsigned char* images, long long image_bytes,
                                const long long* views, int n_views, const int* view, const int* cell, const long long* order, const long long* starts, long long total,
                                int max_cell, int atlas_h, int atlas_w, unsigned char* atlas, int per_unit, void* stream) {
  int log2_w = -1;
  for (int s = 2; (1 << s) <= CDS_TEXTURE_MAX_SIZE; ++s)
    if ((1 << s) == atlas_w) log2_w = s;
  if (!cds_mesh::sizes_ok(n_vertices, n_faces) || n_views < 1 || image_bytes < 0 || total < 0 ||
      total > CDS_TEXTURE_MAX_UNITS || cell_steps(max_cell) < 0 || log2_w < 0 || (atlas_h != atlas_w && 2 * atlas_h != atlas_w) ||
      total > (long long)(atlas_h >> 2) * (atlas_w >> 2) || (per_unit != 0 && per_unit != 1))
    return CDS_EINVAL;
  if (!atlas || ((size_t)atlas & 3) != 0) return CDS_EINVAL;
  if (n_faces > 0 && (!vertices || !colors || !faces || !cams || !images || !views || !view || !cell || !order || !starts)) return CDS_EINVAL;
  FillArgs a;
  a.vertices = vertices; a.colors = colors; a.n_vertices = n_vertices; a.faces = faces; a.n_faces = n_faces; a.cams = cams;
  a.images = images; a.image_bytes = image_bytes; a.views = views; a.n_views = n_views; a.view = view; a.cell = cell; a.order = order; a.starts = starts;
  a.total = n_faces > 0 ? total : 0; a.max_cell = max_cell; a.log2_w = log2_w; a.height = atlas_h; a.atlas = atlas;
  const long long texels = (long long)atlas_h * atlas_w;
  if (per_unit)
    hipLaunchKernelGGL(texture_fill_unit_kernel, dim3(blocks_for(texels / 16)), dim3(kThreads), 0, (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL(texture_fill_texel_kernel, dim3(blocks_for(texels)), dim3(kThreads), 0, (hipStream_t)stream, a);
  return cds_launch_status();
}
