// A texture atlas for a mesh from the images of a scan (the rule is stated in include/cds_mvsnet_hip.h): one view
// and one square cell per face, every texel a function of the input alone.
//
//   cds_texture_votes   one thread per (view, pixel) of the rasteriser's face and valid maps: rule 1, integer atomic adds
//   cds_texture_best    one thread per face: folds a chunk's votes into the running key of rule 2
//   cds_texture_cells   one thread per face: the view of rule 2 from the key, the cell size of rule 3
//   cds_texture_place   one thread per face of the sorted order: rules 4 and 5, the cell's origin from its Morton start, the UV
//   cds_texture_fill    one thread per atlas texel, or per 4 x 4 unit: rule 6
// and the seam levelling of DESIGN §1.19 (rules L1-L6 of the header):
//   cds_texture_level_samples  one thread per node, a (vertex, view) pair: rule L2, the image branch of rule 6 at the vertex
//   cds_texture_level_pairs    one thread per node: the integer pair table of rule L3
//   cds_texture_level_step     one thread per node: one iteration of rule L5, gathers only
//   cds_texture_fill_level     cds_texture_fill with rule L6: the same load_cell / texel, instantiated with the corrections
//
// Decisions are made in integers or fp64 with the bracketing of the rule (the library is built with -ffp-contract=off).  The only
// atomics are the integer adds of the votes and of the pair table: such a sum does not depend on the order of its additions.
// Every loop has its bound fixed before it starts, and every index that comes from data (face, view, sorted position, cell
// origin, pixel, node, span, corner, table slot) is tested against its range before it is used: wrong tables leave texels black
// or unlevelled, they are never followed outside a buffer.
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
  const int* corner_node;                                                // rule L6 (the levelled fill only): [n_faces][3]
  const double* g;                                                       // [n_nodes][3]
  long long n_nodes;
};

// What the texels of one cell share.
struct CellFace {
  int x0, y0, c, view;                                                   // view < 0: the vertex-colour rule
  int h, w;                                                              // the view's image
  const unsigned char* img;
  double P[3][3];                                                        // the corners A, B, C
  int idx[3];
  bool level;                                                            // rule L6: the three corner nodes are inside [0, N)
  double G[3][3];                                                        // their corrections
};

// The last sorted position whose start is <= m (mesh_sample.hip's search); starts[0] == 0 <= m is the caller's.
__device__ __forceinline__ long long owner(const long long* __restrict__ starts, long long lo, long long hi, long long m) {
  while (lo < hi) {
    const long long mid = lo + (hi - lo + 1) / 2;
    if (starts[mid] <= m) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// The image of view v; false for an entry that does not lie inside the bytes, which is not read.
__device__ __forceinline__ bool view_image(const long long* __restrict__ views, const unsigned char* __restrict__ images,
                                           long long image_bytes, long long v, int& h_out, int& w_out,
                                           const unsigned char*& img) {
  const long long off = views[3 * v], h = views[3 * v + 1], w = views[3 * v + 2];
  if (!(h >= 1 && w >= 1 && h * w <= 0x7fffffffLL && off >= 0 && off <= image_bytes - 3 * h * w)) return false;
  h_out = (int)h; w_out = (int)w; img = images + off;
  return true;
}

// The image branch of rule 6 for the world point P in one view: the unrounded values; false unless z > 0 and u, v are finite.
__device__ __forceinline__ bool image_value(const double* __restrict__ cam, int h, int w, const unsigned char* __restrict__ img,
                                            double P0, double P1, double P2, double val[3]) {
  const cds_mesh::ViewPoint p = cds_mesh::view_point(cam, P0, P1, P2);
  if (!(p.z > 0.0 && cds_mesh::is_finite(p.u) && cds_mesh::is_finite(p.v))) return false;
  const double wmax = (double)w - 0.5, hmax = (double)h - 0.5;
  const double uc = p.u < 0.5 ? 0.5 : (p.u > wmax ? wmax : p.u), vc = p.v < 0.5 ? 0.5 : (p.v > hmax ? hmax : p.v);
  const double x = uc - 0.5, y = vc - 0.5;
  int x0 = (int)floor(x), y0 = (int)floor(y);
  x0 = x0 < 0 ? 0 : (x0 > w - 1 ? w - 1 : x0);                           // already there; the image is never read outside
  y0 = y0 < 0 ? 0 : (y0 > h - 1 ? h - 1 : y0);
  const int x1 = x0 + 1 < w ? x0 + 1 : x0, y1 = y0 + 1 < h ? y0 + 1 : y0;
  const double fx = x - (double)x0, fy = y - (double)y0, gx = 1.0 - fx, gy = 1.0 - fy;
  const double w00 = gx * gy, w10 = fx * gy, w01 = gx * fy, w11 = fx * fy;
  const unsigned char *p00 = img + 3 * ((size_t)y0 * w + x0), *p10 = img + 3 * ((size_t)y0 * w + x1),
                      *p01 = img + 3 * ((size_t)y1 * w + x0), *p11 = img + 3 * ((size_t)y1 * w + x1);
#pragma unroll
  for (int ch = 0; ch < 3; ++ch)
    val[ch] = ((w00 * (double)p00[ch] + w10 * (double)p10[ch]) + w01 * (double)p01[ch]) + w11 * (double)p11[ch];
  return true;
}

// clamp(value, 0, 255) with clamp(NaN) = 0, then the nearest level.
__device__ __forceinline__ unsigned char clamped_level(double val) {
  const double cl = val > 0.0 ? (val < 255.0 ? val : 255.0) : 0.0;
  return (unsigned char)(int)floor(cl + 0.5);
}

// The cell that holds unit (ux, uy); false where the unit belongs to none.  kLevel: the corrections of the face's corner nodes too.
template <bool kLevel>
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
  // an image that does not lie inside the buffer is not read: the face keeps its vertex colours
  if (v >= 0 && v < a.n_views && view_image(a.views, a.images, a.image_bytes, v, cf.h, cf.w, cf.img)) cf.view = v;
  cf.level = false;
  if (kLevel && cf.view >= 0) {
    long long node[3];
    bool inside = true;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      node[q] = a.corner_node[3 * f + q];
      inside = inside && node[q] >= 0 && node[q] < a.n_nodes;
    }
    if (inside) {                                                        // a node outside [0, N) is never followed
      cf.level = true;
#pragma unroll
      for (int q = 0; q < 3; ++q)
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) cf.G[q][ch] = a.g[3 * node[q] + ch];
    }
  }
#pragma unroll
  for (int q = 0; q < 3; ++q)
#pragma unroll
    for (int d = 0; d < 3; ++d) cf.P[q][d] = a.vertices[3 * (long long)cf.idx[q] + d];
  return true;
}

// Rule 6 for texel (i, j) of the cell; with kLevel, rule L6 on its image branch.
template <bool kLevel>
__device__ __forceinline__ void texel(const FillArgs& a, const CellFace& cf, int i, int j, unsigned char rgb[3]) {
  const double den = (double)(cf.c - 2);
  const double wb = (((double)i + 0.5) - 1.0) / den, wc = (((double)j + 0.5) - 1.0) / den, wa = (1.0 - wb) - wc;
  if (cf.view >= 0) {
    double P[3], val[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) P[d] = (wa * cf.P[0][d] + wb * cf.P[1][d]) + wc * cf.P[2][d];
    if (image_value(a.cams + (long long)cf.view * kCam, cf.h, cf.w, cf.img, P[0], P[1], P[2], val)) {
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        if (kLevel && cf.level) {
          const double corr = (wa * cf.G[0][ch] + wb * cf.G[1][ch]) + wc * cf.G[2][ch];
          rgb[ch] = clamped_level(val[ch] + corr);
        } else {
          rgb[ch] = (unsigned char)(int)floor(val[ch] + 0.5);
        }
      }
      return;
    }
  }
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    const double ca = a.colors[3 * (long long)cf.idx[0] + ch], cb = a.colors[3 * (long long)cf.idx[1] + ch],
                 cc = a.colors[3 * (long long)cf.idx[2] + ch];
    rgb[ch] = clamped_level((wa * ca + wb * cb) + wc * cc);              // NaN -> 0
  }
}

// One thread per texel: a wave writes 192 consecutive bytes of a row.
template <bool kLevel>
__global__ __launch_bounds__(kThreads) void texture_fill_texel_kernel(const FillArgs a) {
  const long long t = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (t >= ((long long)a.height << a.log2_w)) return;
  const int x = (int)(t & ((1ll << a.log2_w) - 1)), y = (int)(t >> a.log2_w);
  unsigned char rgb[3] = {0, 0, 0};
  CellFace cf;
  if (load_cell<kLevel>(a, x >> 2, y >> 2, cf)) texel<kLevel>(a, cf, x - cf.x0, y - cf.y0, rgb);
  unsigned char* o = a.atlas + 3 * t;
  o[0] = rgb[0]; o[1] = rgb[1]; o[2] = rgb[2];
}

// One thread per 4 x 4 unit: one search for 16 texels; every row of the unit is 12 bytes, written as three words.
template <bool kLevel>
__global__ __launch_bounds__(kThreads) void texture_fill_unit_kernel(const FillArgs a) {
  const long long t = (long long)blockIdx.x * kThreads + threadIdx.x;
  const int log2_uw = a.log2_w - 2;
  if (t >= ((long long)(a.height >> 2) << log2_uw)) return;
  const int ux = (int)(t & ((1ll << log2_uw) - 1)), uy = (int)(t >> log2_uw);
  CellFace cf;
  const bool owned = load_cell<kLevel>(a, ux, uy, cf);
  for (int r = 0; r < 4; ++r) {
    unsigned word[3] = {0u, 0u, 0u};
    if (owned) {
      unsigned char row[12];
#pragma unroll
      for (int q = 0; q < 4; ++q) texel<kLevel>(a, cf, 4 * ux + q - cf.x0, 4 * uy + r - cf.y0, row + 3 * q);
#pragma unroll
      for (int q = 0; q < 3; ++q)
        word[q] = (unsigned)row[4 * q] | ((unsigned)row[4 * q + 1] << 8) | ((unsigned)row[4 * q + 2] << 16) |
                  ((unsigned)row[4 * q + 3] << 24);
    }
    unsigned* o = reinterpret_cast<unsigned*>(a.atlas + 3 * ((((long long)(4 * uy + r)) << a.log2_w) + 4 * ux));
    o[0] = word[0]; o[1] = word[1]; o[2] = word[2];
  }
}

// --------------------------------------------------------------------------------------------------------------------- level
// Seam levelling (rules L1-L6).  A node is a (vertex, view) pair; node_key = vertex * V + view, ascending, so the
// nodes of one vertex are consecutive: span[n] = (the first node of n's vertex, their number).

// Rule L2: one thread per node.  A node whose key, view entry or projection does not fit is not ok and samples 0.
__global__ __launch_bounds__(kThreads) void level_samples_kernel(const float* __restrict__ vertices, long long n_vertices,
                                                                 const double* __restrict__ cams,
                                                                 const unsigned char* __restrict__ images, long long image_bytes,
                                                                 const long long* __restrict__ views, int n_views,
                                                                 const long long* __restrict__ node_key, long long n_nodes,
                                                                 double* __restrict__ sample, unsigned char* __restrict__ ok) {
  const long long n = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (n >= n_nodes) return;
  const long long key = node_key[n];
  double val[3] = {0.0, 0.0, 0.0};
  bool good = false;
  if (key >= 0) {
    const long long vertex = key / n_views, label = key % n_views;
    int h, w;
    const unsigned char* img;
    if (vertex < n_vertices && view_image(views, images, image_bytes, label, h, w, img)) {
      const float* q = vertices + 3 * vertex;
      good = image_value(cams + label * kCam, h, w, img, (double)q[0], (double)q[1], (double)q[2], val);
      if (!good) val[0] = val[1] = val[2] = 0.0;
    }
  }
  sample[3 * n] = val[0]; sample[3 * n + 1] = val[1]; sample[3 * n + 2] = val[2];
  ok[n] = good ? 1 : 0;
}

// The nodes of n's vertex as [first, first + count); false for a span that does not hold n or leaves the nodes.
__device__ __forceinline__ bool load_span(const int* __restrict__ span, long long n, long long n_nodes, int n_views,
                                          long long& first, long long& count) {
  first = span[2 * n]; count = span[2 * n + 1];
  return first >= 0 && count >= 1 && count <= n_views && first <= n && n < first + count && first + count <= n_nodes;
}

// Rule L3: one thread per node i, the pairs (i, j) with j after i in the vertex.  table [V][V][4]: cnt, dsum[3]; integer adds.
// The nodes of a workgroup are neighbours in the vertex order and share a few label pairs, and the whole scan has only V V table
// entries: the workgroup sums its pairs in a small hash table in LDS and adds every used slot to the table once.  A pair that
// finds no slot within kPairProbes adds to the table itself.  Integer sums: the result is the same in any order.
constexpr int kPairSlots = 512, kPairProbes = 8;

__global__ __launch_bounds__(kThreads) void level_pairs_kernel(const double* __restrict__ sample, const unsigned char* __restrict__ ok,
                                                               const long long* __restrict__ node_key, const int* __restrict__ span,
                                                               long long n_nodes, int n_views,
                                                               unsigned long long* __restrict__ table) {
  __shared__ int slot_key[kPairSlots];
  __shared__ unsigned long long slot_sum[kPairSlots][4];
  for (int s = threadIdx.x; s < kPairSlots; s += kThreads) {
    slot_key[s] = -1;
    slot_sum[s][0] = 0; slot_sum[s][1] = 0; slot_sum[s][2] = 0; slot_sum[s][3] = 0;
  }
  __syncthreads();
  const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
  long long first = 0, count = 0;
  const long long key = i < n_nodes ? node_key[i] : -1;
  if (key >= 0 && ok[i] != 0 && load_span(span, i, n_nodes, n_views, first, count)) {
    const long long vertex = key / n_views, a = key % n_views;
    long long qi[3];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) qi[ch] = (long long)floor(sample[3 * i + ch] * 256.0 + 0.5);
    const long long end = first + count;
    for (long long j = i + 1; j < end; ++j) {
      const long long kj = node_key[j];
      if (ok[j] == 0 || kj < 0 || kj / n_views != vertex) continue;
      const long long b = kj % n_views;
      if (b <= a) continue;                                              // keys ascend: never with the tables of rule L1
      const int entry = (int)(a * n_views + b);                          // < V V <= 2^18
      unsigned long long add[4] = {1ull, 0ull, 0ull, 0ull};
#pragma unroll
      for (int ch = 0; ch < 3; ++ch)                                     // two's complement: the int64 sum
        add[1 + ch] = (unsigned long long)(qi[ch] - (long long)floor(sample[3 * j + ch] * 256.0 + 0.5));
      unsigned h = ((unsigned)entry * 2654435761u) >> 23;                // 9 bits: kPairSlots
      unsigned long long* dst = table + 4 * (long long)entry;
      bool found = false;
      for (int probe = 0; probe < kPairProbes; ++probe) {
        if (!found) {
          const int prev = atomicCAS(&slot_key[h], -1, entry);
          if (prev == -1 || prev == entry) { dst = slot_sum[h]; found = true; }
          else h = (h + 1) & (kPairSlots - 1);
        }
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) atomicAdd(dst + q, add[q]);
    }
  }
  __syncthreads();
  for (int s = threadIdx.x; s < kPairSlots; s += kThreads) {
    const int entry = slot_key[s];
    if (entry < 0 || entry >= n_views * n_views) continue;               // n_views <= 512: no overflow
#pragma unroll
    for (int q = 0; q < 4; ++q) atomicAdd(table + 4 * (long long)entry + q, slot_sum[s][q]);
  }
}

// Rule L5: one thread per node, gathers only; g_in is the previous iteration, g_out the next.
__global__ __launch_bounds__(kThreads) void level_step_kernel(const double* __restrict__ sample, const unsigned char* __restrict__ ok,
                                                              const int* __restrict__ span, const long long* __restrict__ corner_start,
                                                              const long long* __restrict__ corner_list, long long n_list,
                                                              const int* __restrict__ corner_node, long long n_nodes,
                                                              long long n_faces, int n_views, double lambda,
                                                              const double* __restrict__ g_in, double* __restrict__ g_out) {
  const long long n = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (n >= n_nodes) return;
  const double g[3] = {g_in[3 * n], g_in[3 * n + 1], g_in[3 * n + 2]};
  double S[3] = {0.0, 0.0, 0.0}, T[3] = {0.0, 0.0, 0.0};
  long long c = 0, d = 0, first, count;
  if (ok[n] != 0 && load_span(span, n, n_nodes, n_views, first, count)) {
    const double s[3] = {sample[3 * n], sample[3 * n + 1], sample[3 * n + 2]};
    const long long end = first + count;
    for (long long m = first; m < end; ++m) {
      if (m == n || ok[m] == 0) continue;
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) S[ch] = S[ch] + ((sample[3 * m + ch] + g_in[3 * m + ch]) - s[ch]);
      ++c;
    }
  }
  const long long n_corners = 3 * n_faces, lo = corner_start[n], hi = corner_start[n + 1];
  if (lo >= 0 && lo <= hi && hi <= n_list) {
    for (long long k = lo; k < hi; ++k) {
      const long long corner = corner_list[k];
      if (corner < 0 || corner >= n_corners) continue;
      const long long f = corner / 3, q = corner - 3 * f;
#pragma unroll
      for (int step = 1; step <= 2; ++step) {
        const long long m = corner_node[3 * f + (q + step) % 3];
        if (m < 0 || m >= n_nodes) continue;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) T[ch] = T[ch] + g_in[3 * m + ch];
        ++d;
      }
    }
  }
  const double den = (double)c + lambda * (double)d;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch)
    g_out[3 * n + ch] = den > 0.0 ? g[ch] + CDS_TEXTURE_LEVEL_OMEGA * ((S[ch] + lambda * T[ch]) / den - g[ch]) : g[ch];
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

// The argument checks and the launch of both fills.  level: rule L6 from corner_node, g and n_nodes.
static int fill_dispatch(const float* vertices, const unsigned char* colors, long long n_vertices, const int* faces, long long n_faces,
                         const double* cams, const unsigned char* images, long long image_bytes, const long long* views, int n_views,
                         const int* view, const int* cell, const long long* order, const long long* starts, long long total,
                         int max_cell, int atlas_h, int atlas_w, unsigned char* atlas, int per_unit, bool level,
                         const int* corner_node, const double* g, long long n_nodes, void* stream) {
  int log2_w = -1;
  for (int s = 2; (1 << s) <= CDS_TEXTURE_MAX_SIZE; ++s)
    if ((1 << s) == atlas_w) log2_w = s;
  if (!cds_mesh::sizes_ok(n_vertices, n_faces) || n_views < 1 || image_bytes < 0 || total < 0 ||
      total > CDS_TEXTURE_MAX_UNITS || cell_steps(max_cell) < 0 || log2_w < 0 || (atlas_h != atlas_w && 2 * atlas_h != atlas_w) ||
      total > (long long)(atlas_h >> 2) * (atlas_w >> 2) || (per_unit != 0 && per_unit != 1))
    return CDS_EINVAL;
  if (!atlas || ((size_t)atlas & 3) != 0) return CDS_EINVAL;
  if (n_faces > 0 && (!vertices || !colors || !faces || !cams || !images || !views || !view || !cell || !order || !starts)) return CDS_EINVAL;
  if (level && (!cds_mesh::sizes_ok(n_nodes, 0) || (n_faces > 0 && !corner_node) || (n_nodes > 0 && !g))) return CDS_EINVAL;
  FillArgs a;
  a.vertices = vertices; a.colors = colors; a.n_vertices = n_vertices; a.faces = faces; a.n_faces = n_faces; a.cams = cams;
  a.images = images; a.image_bytes = image_bytes; a.views = views; a.n_views = n_views; a.view = view; a.cell = cell; a.order = order; a.starts = starts;
  a.total = n_faces > 0 ? total : 0; a.max_cell = max_cell; a.log2_w = log2_w; a.height = atlas_h; a.atlas = atlas;
  a.corner_node = corner_node; a.g = g; a.n_nodes = level ? n_nodes : 0;
  const long long texels = (long long)atlas_h * atlas_w;
  const dim3 units(blocks_for(texels / 16)), all(blocks_for(texels)), block(kThreads);
  hipStream_t st = (hipStream_t)stream;
  if (per_unit && level) hipLaunchKernelGGL(texture_fill_unit_kernel<true>, units, block, 0, st, a);
  else if (per_unit)     hipLaunchKernelGGL(texture_fill_unit_kernel<false>, units, block, 0, st, a);
  else if (level)        hipLaunchKernelGGL(texture_fill_texel_kernel<true>, all, block, 0, st, a);
  else                   hipLaunchKernelGGL(texture_fill_texel_kernel<false>, all, block, 0, st, a);
  return cds_launch_status();
}

extern "C" int cds_texture_fill(const float* vertices, const unsigned char* colors, long long n_vertices, const int* faces,
                                long long n_faces, const double* cams, const unsigned char* images, long long image_bytes,
                                const long long* views, int n_views, const int* view, const int* cell, const long long* order, const long long* starts, long long total,
                                int max_cell, int atlas_h, int atlas_w, unsigned char* atlas, int per_unit, void* stream) {
  return fill_dispatch(vertices, colors, n_vertices, faces, n_faces, cams, images, image_bytes, views, n_views, view, cell, order,
                       starts, total, max_cell, atlas_h, atlas_w, atlas, per_unit, false, nullptr, nullptr, 0, stream);
}

extern "C" int cds_texture_fill_level(const float* vertices, const unsigned char* colors, long long n_vertices, const int* faces,
                                      long long n_faces, const double* cams, const unsigned char* images, long long image_bytes,
                                      const long long* views, int n_views, const int* view, const int* cell, const long long* order,
                                      const long long* starts, long long total, int max_cell, int atlas_h, int atlas_w,
                                      unsigned char* atlas, int per_unit, const int* corner_node, const double* g, long long n_nodes,
                                      void* stream) {
  return fill_dispatch(vertices, colors, n_vertices, faces, n_faces, cams, images, image_bytes, views, n_views, view, cell, order,
                       starts, total, max_cell, atlas_h, atlas_w, atlas, per_unit, true, corner_node, g, n_nodes, stream);
}

extern "C" int cds_texture_level_samples(const float* vertices, long long n_vertices, const double* cams, const unsigned char* images,
                                         long long image_bytes, const long long* views, int n_views, const long long* node_key,
                                         long long n_nodes, double* sample, unsigned char* ok, void* stream) {
  if (!cds_mesh::sizes_ok(n_vertices, n_nodes) || n_views < 1 || n_views > CDS_TEXTURE_LEVEL_MAX_VIEWS || image_bytes < 0)
    return CDS_EINVAL;
  if (n_nodes == 0) return 0;
  if (!vertices || !cams || !images || !views || !node_key || !sample || !ok) return CDS_EINVAL;
  hipLaunchKernelGGL(level_samples_kernel, dim3(blocks_for(n_nodes)), dim3(kThreads), 0, (hipStream_t)stream, vertices, n_vertices,
                     cams, images, image_bytes, views, n_views, node_key, n_nodes, sample, ok);
  return cds_launch_status();
}

extern "C" int cds_texture_level_pairs(const double* sample, const unsigned char* ok, const long long* node_key, const int* span,
                                       long long n_nodes, int n_views, long long* table, void* stream) {
  if (!cds_mesh::sizes_ok(n_nodes, 0) || n_views < 1 || n_views > CDS_TEXTURE_LEVEL_MAX_VIEWS) return CDS_EINVAL;
  if (n_nodes == 0) return 0;
  if (!sample || !ok || !node_key || !span || !table) return CDS_EINVAL;
  hipLaunchKernelGGL(level_pairs_kernel, dim3(blocks_for(n_nodes)), dim3(kThreads), 0, (hipStream_t)stream, sample, ok, node_key,
                     span, n_nodes, n_views, reinterpret_cast<unsigned long long*>(table));
  return cds_launch_status();
}

extern "C" int cds_texture_level_step(const double* sample, const unsigned char* ok, const int* span, const long long* corner_start,
                                      const long long* corner_list, long long n_list, const int* corner_node, long long n_nodes,
                                      long long n_faces, int n_views, double lambda, const double* g_in, double* g_out, void* stream) {
  if (!cds_mesh::sizes_ok(n_nodes, n_faces) || n_list < 0 || n_list > 3 * n_faces || n_views < 1 || n_views > CDS_TEXTURE_LEVEL_MAX_VIEWS || !cds_mesh::finite_pos(lambda))
    return CDS_EINVAL;
  if (n_nodes == 0) return 0;
  if (!sample || !ok || !span || !corner_start || !corner_list || !corner_node || !g_in || !g_out || g_in == g_out) return CDS_EINVAL;
  hipLaunchKernelGGL(level_step_kernel, dim3(blocks_for(n_nodes)), dim3(kThreads), 0, (hipStream_t)stream, sample, ok, span,
                     corner_start, corner_list, n_list, corner_node, n_nodes, n_faces, n_views, lambda, g_in, g_out);
  return cds_launch_status();
}
