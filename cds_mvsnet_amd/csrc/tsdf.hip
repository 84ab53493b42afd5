// Meshing a scan (the rule is stated in include/cds_mvsnet_hip.h): a sparse truncated signed distance volume in
// blocks of 8x8x8 lattice points, and its zero level set as the triangles of the six Freudenthal tetrahedra of every cube.
//
//   cds_tsdf_integrate_f32   a chunk of views into the volume
//   cds_tsdf_integrate_w_f32 the same with a weight per pixel and, optionally, the depth interpolated between pixels (§1.14)
//   cds_tsdf_view_weights    those weights for one view: viewing angle against the depth map's normals, times a confidence
//   cds_tsdf_classify        per lattice point: which of its seven edges carry a vertex, how many triangles its cube gives
//   cds_tsdf_emit            vertices, colours, faces
//
// Integrate: one 512-thread workgroup owns one allocated block, one thread one lattice point.  The six accumulators of a point
// live in registers while the chunk's views are looped over, so the volume (24 bytes per point) is read and written once per
// launch, not once per view.  The chunk's cameras sit in LDS as doubles and are read wave-uniformly.  Before any per-point work
// one thread per view tests the block's bounding sphere against the view's frustum and depth range; the loop then skips the
// views that cannot see the block with a workgroup-uniform branch.  The test is conservative (the sphere is 0.1 % larger than the
// block), so it never changes a result.  No atomics: the view order is the loop order.
//
// Classify: a block with a one-point halo (10^3 points, through the dense block table) is staged in LDS as two bits per point
// (valid, inside); from it the 9^3 cubes that touch the block's points are marked processed or not, and every point decides its
// own seven edges and its own cube.  The edge flags are therefore written by the edge's owner alone.  Per-block totals are
// integer LDS atomics.
//
// Emit: a workgroup scans its block's counts (wave shuffles, eight wave totals in LDS), writes each point's first vertex number
// to `vstart` and its vertices, and in a second kernel every cube finds the vertex numbers of its edges through `vstart` and
// the owners' edge flags.  The order of vertices and faces is that of the rule by construction.
#include "cds_common.hpp"

namespace {

constexpr int kPts = 512;            // lattice points of a block
constexpr int kCam = 24;             // doubles per camera: R 0..8, t 9..11, K 12..20, largest kept depth 21
constexpr int kMaxChunk = CDS_TSDF_MAX_CHUNK;
constexpr double kCullRadius = 6.07; // in voxels: sqrt(3) * 3.5 = 6.0622 (block centre to its corner points), plus 0.1 %

struct TsdfFrame {
  double origin[3], voxel;
  int nb[3];
};

// ---------------------------------------------------------------------------------------------------------------- the cases
// Edges of a tetrahedron between its corners (lo, hi), lo < hi.
constexpr int kEdgeLo[6] = {0, 0, 0, 1, 1, 2}, kEdgeHi[6] = {1, 2, 3, 2, 3, 3};
constexpr int tet_edge(int i, int j) { return i < j ? (i == 0 ? j - 1 : i + j) : tet_edge(j, i); }   // (0,1)..(2,3) -> 0..5

struct TetCases {
  unsigned char n[16];               // triangles of the case
  unsigned char e[16][6];            // their vertices, as tetrahedron edges
};

// The 16 cases of a tetrahedron (v0, v1, v2, v3) with det[v1 - v0, v2 - v0, v3 - v0] > 0; bit i of the case: corner i is inside.
//   one corner i apart from the others j < k < l: the triangle (ij, ik, il).  With i inside and (i, j, k, l) an even permutation
//   its normal points away from i: take v_i as the origin and the other three as a right-handed basis, then
//   (e_k - e_j) x (e_l - e_j) = e_j + e_k + e_l.  (i, j, k, l) is even iff i is even (i transpositions bring it to the front).
//   An odd permutation, or i being the one OUTSIDE corner, each swap the last two vertices.
//   two inside i < j, two outside k < l: the quadrilateral (ik, il, jl, jk), split (q0, q1, q2), (q0, q2, q3); for the identity
//   its normal (q1 - q0) x (q2 - q0) = (0, 1/4, 1/4) has a positive product with (v2 + v3) / 2 - (v0 + v1) / 2: it faces the outside.
//   An odd permutation (i, j, k, l) swaps the last two vertices of both triangles.
constexpr TetCases make_tet_cases() {
  TetCases t{};
  for (int c = 0; c < 16; ++c) {
    int in[4] = {0, 0, 0, 0}, out[4] = {0, 0, 0, 0}, ni = 0, no = 0;
    for (int i = 0; i < 4; ++i) {
      if (c >> i & 1) in[ni++] = i; else out[no++] = i;
    }
    if (ni == 0 || ni == 4) continue;
    if (ni == 1 || no == 1) {
      const int i = ni == 1 ? in[0] : out[0];
      int r[3] = {0, 0, 0}, k = 0;
      for (int q = 0; q < 4; ++q)
        if (q != i) r[k++] = q;
      const bool flip = ((i & 1) != 0) != (no == 1);
      t.n[c] = 1;
      t.e[c][0] = (unsigned char)tet_edge(i, r[0]);
      t.e[c][1] = (unsigned char)tet_edge(i, flip ? r[2] : r[1]);
      t.e[c][2] = (unsigned char)tet_edge(i, flip ? r[1] : r[2]);
    } else {
      const int p[4] = {in[0], in[1], out[0], out[1]};
      int inv = 0;
      for (int a = 0; a < 4; ++a)
        for (int b = a + 1; b < 4; ++b) inv += p[a] > p[b];
      const int q[4] = {tet_edge(p[0], p[2]), tet_edge(p[0], p[3]), tet_edge(p[1], p[3]), tet_edge(p[1], p[2])};
      const bool flip = (inv & 1) != 0;
      t.n[c] = 2;
      t.e[c][0] = (unsigned char)q[0]; t.e[c][1] = (unsigned char)q[flip ? 2 : 1]; t.e[c][2] = (unsigned char)q[flip ? 1 : 2];
      t.e[c][3] = (unsigned char)q[0]; t.e[c][4] = (unsigned char)q[flip ? 3 : 2]; t.e[c][5] = (unsigned char)q[flip ? 2 : 3];
    }
  }
  return t;
}

__constant__ const TetCases kCases = make_tet_cases();
// The six axis orders (a, b, c), lexicographic: corners 000, e_a, e_a + e_b, 111 as bit masks (bit 0: x); the tetrahedron's
// determinant is the sign of the permutation.
__constant__ const unsigned char kTetCorner[6][4] = {{0, 1, 3, 7}, {0, 1, 5, 7}, {0, 2, 3, 7}, {0, 2, 6, 7}, {0, 4, 5, 7}, {0, 4, 6, 7}};
__constant__ const unsigned char kTetOdd[6] = {0, 1, 1, 0, 0, 1};
// Edge kinds in the rule's order (x, y, z, xy, xz, yz, xyz) as corner offsets, and the kind of an offset.
__constant__ const unsigned char kKindMask[7] = {1, 2, 4, 3, 5, 6, 7};
__constant__ const unsigned char kKindOf[8] = {255, 0, 1, 3, 2, 4, 5, 6};

// ------------------------------------------------------------------------------------------------------------------ helpers
struct BlockPos { int x, y, z; };

__device__ __forceinline__ BlockPos block_pos(int key, const TsdfFrame& f) {
  return {key % f.nb[0], (key / f.nb[0]) % f.nb[1], key / (f.nb[0] * f.nb[1])};
}

// The storage index of the lattice point at local coordinates (lx, ly, lz) in -1..8 of block `bp`, or -1 when its block is not
// allocated or lies outside the grid.
__device__ __forceinline__ long long locate(const int* __restrict__ table, const TsdfFrame& f, BlockPos bp, int lx, int ly, int lz,
                                            long long n_blocks) {
  const int bx = bp.x + (lx >> 3), by = bp.y + (ly >> 3), bz = bp.z + (lz >> 3);       // -1 >> 3 = -1, 8 >> 3 = 1
  if ((unsigned)bx >= (unsigned)f.nb[0] || (unsigned)by >= (unsigned)f.nb[1] || (unsigned)bz >= (unsigned)f.nb[2]) return -1;
  const int b = table[((long long)bz * f.nb[1] + by) * f.nb[0] + bx];
  if (b < 0 || b >= n_blocks) return -1;
  return (long long)b * kPts + (((lz & 7) * 8 + (ly & 7)) * 8 + (lx & 7));
}

// Exclusive prefix of one int per thread over the 512 threads of a workgroup, in thread order.
__device__ __forceinline__ int block_scan(int v, int* s_wave) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  int inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(inc, o, 64);
    if (lane >= o) inc += t;
  }
  __syncthreads();                   // s_wave may still be read from an earlier scan
  if (lane == 63) s_wave[wv] = inc;
  __syncthreads();
  int base = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) base += i < wv ? s_wave[i] : 0;
  return base + inc - v;
}

// ---------------------------------------------------------------------------------------------------------------- integrate
// The chunk's cameras into LDS, and per view whether it can see block `bp` at all (s_see); ends with a barrier.  Every quantity
// of the test is linear in the world point, so over the block's bounding sphere it stays within value(centre) +- |gradient| radius.
// A depth that cds_tsdf_integrate_w_f32 interpolates lies between kept depths of the view, so entry 21 bounds it as well.
__device__ __forceinline__ void stage_views(const double* __restrict__ cams, int nv, const TsdfFrame& f, BlockPos bp, double trunc,
                                            int h, int w, double* s_cam, int* s_see) {
  const int tid = threadIdx.x;
  for (int i = tid; i < nv * kCam; i += kPts) s_cam[i] = cams[i];
  __syncthreads();
  if (tid < nv) {
    const double* c = s_cam + tid * kCam;
    const double C0 = f.origin[0] + ((double)(8 * bp.x) + 3.5) * f.voxel, C1 = f.origin[1] + ((double)(8 * bp.y) + 3.5) * f.voxel,
                 C2 = f.origin[2] + ((double)(8 * bp.z) + 3.5) * f.voxel;
    const double rad = kCullRadius * f.voxel;
    double xc[3];
    for (int r = 0; r < 3; ++r) xc[r] = ((c[3 * r] * C0 + c[3 * r + 1] * C1) + c[3 * r + 2] * C2) + c[9 + r];
    const double nz = sqrt((c[6] * c[6] + c[7] * c[7]) + c[8] * c[8]);
    bool see = true;
    if (xc[2] + nz * rad <= 0.0) see = false;                          // all of it behind the camera
    if (xc[2] - nz * rad > c[21] + trunc) see = false;                 // all of it more than T behind every kept depth
    if (c[18] == 0.0 && c[19] == 0.0 && c[20] == 1.0) {                // p2 = z > 0: u >= 0 iff p0 >= 0, u < w iff p0 - w p2 < 0
      for (int r = 0; r < 2; ++r) {
        const double* k = c + 12 + 3 * r;
        const double lim = r == 0 ? (double)w : (double)h;
        double g[3], gw[3];
        for (int j = 0; j < 3; ++j) {
          g[j] = (k[0] * c[j] + k[1] * c[3 + j]) + k[2] * c[6 + j];
          gw[j] = g[j] - lim * c[6 + j];
        }
        const double p = (k[0] * xc[0] + k[1] * xc[1]) + k[2] * xc[2];
        const double ng = sqrt((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]);
        const double ngw = sqrt((gw[0] * gw[0] + gw[1] * gw[1]) + gw[2] * gw[2]);
        // the bounds are not 0: a quotient p0 / p2 that underflows to -0.0 passes u >= 0
        if (p + ng * rad < -1e-100) see = false;                       // all of it left of (above) the map
        if ((p - lim * xc[2]) - ngw * rad > 1e-100) see = false;       // all of it right of (below) the map
      }
    }
    s_see[tid] = see ? 1 : 0;
  }
  __syncthreads();
}

__global__ __launch_bounds__(512) void tsdf_integrate_kernel(const int* __restrict__ keys, TsdfFrame f, double trunc,
                                                             const float* __restrict__ depths,
                                                             const unsigned char* __restrict__ masks,
                                                             const unsigned char* __restrict__ images,
                                                             const double* __restrict__ cams, int nv, int h, int w,
                                                             float* __restrict__ sum, int* __restrict__ n, int* __restrict__ nc,
                                                             int* __restrict__ rgb, long long n_blocks) {
  __shared__ double s_cam[kMaxChunk * kCam];
  __shared__ int s_see[kMaxChunk];
  const int tid = threadIdx.x;
  const long long b = blockIdx.x;
  const BlockPos bp = block_pos(keys[b], f);
  stage_views(cams, nv, f, bp, trunc, h, w, s_cam, s_see);

  const int lx = tid & 7, ly = (tid >> 3) & 7, lz = tid >> 6;
  const double X0 = f.origin[0] + (double)(8 * bp.x + lx) * f.voxel, X1 = f.origin[1] + (double)(8 * bp.y + ly) * f.voxel,
               X2 = f.origin[2] + (double)(8 * bp.z + lz) * f.voxel;
  const long long p = b * kPts + tid, plane = n_blocks * kPts;
  float acc = sum[p];
  int cnt = n[p], ccnt = nc[p], cr = rgb[p], cg = rgb[plane + p], cb = rgb[2 * plane + p];
  const size_t hw = (size_t)h * w;
  for (int v = 0; v < nv; ++v) {
    if (!s_see[v]) continue;                                           // the same for the whole workgroup
    const double* c = s_cam + v * kCam;
    const double xc0 = ((c[0] * X0 + c[1] * X1) + c[2] * X2) + c[9];
    const double xc1 = ((c[3] * X0 + c[4] * X1) + c[5] * X2) + c[10];
    const double z = ((c[6] * X0 + c[7] * X1) + c[8] * X2) + c[11];
    if (!(z > 0.0)) continue;
    const double p0 = (c[12] * xc0 + c[13] * xc1) + c[14] * z;
    const double p1 = (c[15] * xc0 + c[16] * xc1) + c[17] * z;
    const double p2 = (c[18] * xc0 + c[19] * xc1) + c[20] * z;
    const double pu = p0 / p2, pv = p1 / p2;
    if (!(pu >= 0.0 && pu < (double)w && pv >= 0.0 && pv < (double)h)) continue;     // false for NaN
    const size_t q = (size_t)v * hw + (size_t)(int)pv * w + (size_t)(int)pu;         // 0 <= floor < w, h: truncation is floor
    const float d = depths[q];
    if (masks[q] == 0 || !(d > 0.f && d <= 3.402823466e+38f)) continue;
    const double sdf = (double)d - z;
    if (sdf < -trunc) continue;
    acc = acc + (float)fmin(1.0, sdf / trunc);
    ++cnt;
    if (sdf <= trunc) {
      const unsigned char* px = images + 3 * q;
      cr += px[0]; cg += px[1]; cb += px[2];
      ++ccnt;
    }
  }
  sum[p] = acc;
  n[p] = cnt; nc[p] = ccnt;
  rgb[p] = cr; rgb[plane + p] = cg; rgb[2 * plane + p] = cb;
}

__device__ __forceinline__ bool kept_depth(float d) { return d > 0.f && d <= 3.402823466e+38f; }    // false for NaN and +inf

// The weighted rule: tsdf_integrate_kernel with a weight per pixel and, with kInterp, the depth interpolated
// between the four pixel centres around (u, v) in inverse depth.  The nearest pixel decides as before whether the view counts
// and gives the weight and the colour; the interpolation only replaces the depth, and only where its four pixels are kept and
// within `jump` of each other.  `weights` and `wn` are both null or both set (the host checks it).
template <bool kInterp>
__global__ __launch_bounds__(512) void tsdf_integrate_w_kernel(const int* __restrict__ keys, TsdfFrame f, double trunc,
                                                               const float* __restrict__ depths,
                                                               const unsigned char* __restrict__ masks,
                                                               const unsigned char* __restrict__ images,
                                                               const unsigned char* __restrict__ weights, float jump,
                                                               const double* __restrict__ cams, int nv, int h, int w,
                                                               float* __restrict__ sum, int* __restrict__ n, int* __restrict__ nc,
                                                               int* __restrict__ rgb, int* __restrict__ wn, long long n_blocks) {
  __shared__ double s_cam[kMaxChunk * kCam];
  __shared__ int s_see[kMaxChunk];
  const int tid = threadIdx.x;
  const long long b = blockIdx.x;
  const BlockPos bp = block_pos(keys[b], f);
  stage_views(cams, nv, f, bp, trunc, h, w, s_cam, s_see);

  const int lx = tid & 7, ly = (tid >> 3) & 7, lz = tid >> 6;
  const double X0 = f.origin[0] + (double)(8 * bp.x + lx) * f.voxel, X1 = f.origin[1] + (double)(8 * bp.y + ly) * f.voxel,
               X2 = f.origin[2] + (double)(8 * bp.z + lz) * f.voxel;
  const long long p = b * kPts + tid, plane = n_blocks * kPts;
  float acc = sum[p];
  int cnt = n[p], ccnt = nc[p], cr = rgb[p], cg = rgb[plane + p], cb = rgb[2 * plane + p];
  int wcnt = weights ? wn[p] : 0;
  const size_t hw = (size_t)h * w;
  for (int v = 0; v < nv; ++v) {
    if (!s_see[v]) continue;                                           // the same for the whole workgroup
    const double* c = s_cam + v * kCam;
    const double xc0 = ((c[0] * X0 + c[1] * X1) + c[2] * X2) + c[9];
    const double xc1 = ((c[3] * X0 + c[4] * X1) + c[5] * X2) + c[10];
    const double z = ((c[6] * X0 + c[7] * X1) + c[8] * X2) + c[11];
    if (!(z > 0.0)) continue;
    const double p0 = (c[12] * xc0 + c[13] * xc1) + c[14] * z;
    const double p1 = (c[15] * xc0 + c[16] * xc1) + c[17] * z;
    const double p2 = (c[18] * xc0 + c[19] * xc1) + c[20] * z;
    const double pu = p0 / p2, pv = p1 / p2;
    if (!(pu >= 0.0 && pu < (double)w && pv >= 0.0 && pv < (double)h)) continue;     // false for NaN
    const size_t q = (size_t)v * hw + (size_t)(int)pv * w + (size_t)(int)pu;         // 0 <= floor < w, h: truncation is floor
    const float d = depths[q];
    if (masks[q] == 0 || !kept_depth(d)) continue;
    const int wq = weights ? (int)weights[q] : 1;
    if (wq == 0) continue;
    double dd = (double)d;
    if (kInterp) {
      const double a = pu - 0.5, bb = pv - 0.5;                        // >= -0.5: the floors are >= -1
      const double fa = floor(a), fb = floor(bb);
      const int x0 = (int)fa, y0 = (int)fb;
      if (x0 >= 0 && x0 + 1 < w && y0 >= 0 && y0 + 1 < h) {            // the four pixels lie inside the map
        const size_t q0 = (size_t)v * hw + (size_t)y0 * w + (size_t)x0;
        const float d00 = depths[q0], d10 = depths[q0 + 1], d01 = depths[q0 + w], d11 = depths[q0 + w + 1];
        const bool kept = masks[q0] != 0 && masks[q0 + 1] != 0 && masks[q0 + w] != 0 && masks[q0 + w + 1] != 0 &&
                          kept_depth(d00) && kept_depth(d10) && kept_depth(d01) && kept_depth(d11);
        const float lo = fminf(fminf(d00, d10), fminf(d01, d11)), hi = fmaxf(fmaxf(d00, d10), fmaxf(d01, d11));
        if (kept && (double)hi - (double)lo <= (double)jump * (double)lo) {
          const double fx = a - fa, fy = bb - fb;
          const double i00 = 1.0 / (double)d00, i10 = 1.0 / (double)d10, i01 = 1.0 / (double)d01, i11 = 1.0 / (double)d11;
          const double i0 = i00 + fx * (i10 - i00), i1 = i01 + fx * (i11 - i01);
          dd = 1.0 / (i0 + fy * (i1 - i0));
        }
      }
    }
    const double sdf = dd - z;
    if (sdf < -trunc) continue;
    acc = acc + (float)((double)wq * fmin(1.0, sdf / trunc));
    ++cnt;
    wcnt += wq;
    if (sdf <= trunc) {
      const unsigned char* px = images + 3 * q;
      cr += px[0]; cg += px[1]; cb += px[2];
      ++ccnt;
    }
  }
  sum[p] = acc;
  n[p] = cnt; nc[p] = ccnt;
  rgb[p] = cr; rgb[plane + p] = cg; rgb[2 * plane + p] = cb;
  if (weights) wn[p] = wcnt;
}

// The weight of every pixel of one view (the rule is in the header): one thread per pixel.
struct WeightCam {
  float fx, s, cx, fy, cy, R[9];         // K = [[fx, s, cx], [0, fy, cy], [0, 0, 1]] and the rotation of E, row-major
};

__global__ __launch_bounds__(256) void tsdf_view_weights_kernel(const float* __restrict__ depth,
                                                                const unsigned char* __restrict__ mask,
                                                                const float* __restrict__ normals,
                                                                const unsigned char* __restrict__ ok,
                                                                const float* __restrict__ conf, WeightCam cam, int h, int w,
                                                                unsigned char* __restrict__ weights) {
  const long long hw = (long long)h * w, p = (long long)blockIdx.x * 256 + threadIdx.x;
  if (p >= hw) return;
  if (mask[p] == 0 || !kept_depth(depth[p])) {
    weights[p] = 0;
    return;
  }
  double a = 1.0;
  if (normals) {
    a = 0.0;
    if (ok[p] != 0) {
      const int x = (int)(p % w), y = (int)(p / w);
      const double c1 = (((double)y + 0.5) - (double)cam.cy) / (double)cam.fy;
      const double c0 = ((((double)x + 0.5) - (double)cam.cx) - (double)cam.s * c1) / (double)cam.fx;
      const double n0 = (double)normals[p], n1 = (double)normals[hw + p], n2 = (double)normals[2 * hw + p];
      const double nc0 = ((double)cam.R[0] * n0 + (double)cam.R[1] * n1) + (double)cam.R[2] * n2;
      const double nc1 = ((double)cam.R[3] * n0 + (double)cam.R[4] * n1) + (double)cam.R[5] * n2;
      const double nc2 = ((double)cam.R[6] * n0 + (double)cam.R[7] * n1) + (double)cam.R[8] * n2;
      const double t = -((nc0 * c0 + nc1 * c1) + nc2) / sqrt((c0 * c0 + c1 * c1) + 1.0);
      a = !(t >= 0.0 && t <= 1.7976931348623157e308) ? 0.0 : t > 1.0 ? 1.0 : t;       // NaN, +-inf and negatives give 0
    }
  }
  double cf = 1.0;
  if (conf) {
    const double t = (double)conf[p];
    cf = !(t >= 0.0) ? 0.0 : t > 1.0 ? 1.0 : t;                        // NaN gives 0
  }
  const int wt = (int)floor(255.0 * (a * cf) + 0.5);
  weights[p] = (unsigned char)(wt < 1 ? 1 : wt > 255 ? 255 : wt);
}

// ----------------------------------------------------------------------------------------------------------------- classify
__global__ __launch_bounds__(512) void tsdf_classify_kernel(const int* __restrict__ keys, const int* __restrict__ table, TsdfFrame f,
                                                            const float* __restrict__ sum, const int* __restrict__ n,
                                                            int min_weight, long long n_blocks, unsigned char* __restrict__ vmask,
                                                            unsigned char* __restrict__ tcount, int* __restrict__ block_v,
                                                            int* __restrict__ block_t) {
  __shared__ unsigned char s_pt[1000];   // bit 0: valid, bit 1: inside; points -1..8 per axis
  __shared__ unsigned char s_cube[729];  // cubes with lower corner -1..7 per axis: all eight corners valid
  __shared__ int s_tot[2];
  const int tid = threadIdx.x;
  const long long b = blockIdx.x;
  const BlockPos bp = block_pos(keys[b], f);
  if (tid < 2) s_tot[tid] = 0;
  for (int c = tid; c < 1000; c += kPts) {
    const long long q = locate(table, f, bp, c % 10 - 1, (c / 10) % 10 - 1, c / 100 - 1, n_blocks);
    unsigned char st = 0;
    if (q >= 0) st = (unsigned char)((n[q] >= min_weight ? 1 : 0) | (sum[q] < 0.f ? 2 : 0));
    s_pt[c] = st;
  }
  __syncthreads();
  for (int c = tid; c < 729; c += kPts) {
    const int base = (c / 81) * 100 + ((c / 9) % 9) * 10 + c % 9;
    unsigned all = 1;
#pragma unroll
    for (int o = 0; o < 8; ++o) all &= s_pt[base + (o & 1) + ((o >> 1) & 1) * 10 + (o >> 2) * 100];
    s_cube[c] = (unsigned char)all;
  }
  __syncthreads();
  const int lx = tid & 7, ly = (tid >> 3) & 7, lz = tid >> 6;
  const int pc = (lz + 1) * 100 + (ly + 1) * 10 + lx + 1;              // this point in s_pt
  const int cc = (lz + 1) * 81 + (ly + 1) * 9 + lx + 1;                // its cube in s_cube
  const int in0 = s_pt[pc] >> 1;
  unsigned mask = 0;
#pragma unroll
  for (int kk = 0; kk < 7; ++kk) {
    const int d = kKindMask[kk];
    const int in1 = s_pt[pc + (d & 1) + ((d >> 1) & 1) * 10 + (d >> 2) * 100] >> 1;
    unsigned touched = 0;                                              // a processed cube that has this edge: lower corner L - o
#pragma unroll
    for (int o = 0; o < 8; ++o)
      if ((o & d) == 0) touched |= s_cube[cc - (o & 1) - ((o >> 1) & 1) * 9 - (o >> 2) * 81];
    if (touched && in0 != in1) mask |= 1u << kk;
  }
  int tris = 0;
  if (s_cube[cc]) {
    unsigned ins = 0;
#pragma unroll
    for (int o = 0; o < 8; ++o) ins |= (unsigned)(s_pt[pc + (o & 1) + ((o >> 1) & 1) * 10 + (o >> 2) * 100] >> 1) << o;
#pragma unroll
    for (int t = 0; t < 6; ++t) {
      unsigned cs = 0;
#pragma unroll
      for (int i = 0; i < 4; ++i) cs |= ((ins >> kTetCorner[t][i]) & 1u) << i;
      tris += kCases.n[cs];
    }
  }
  vmask[b * kPts + tid] = (unsigned char)mask;
  tcount[b * kPts + tid] = (unsigned char)tris;
  if (mask) atomicAdd(&s_tot[0], __popc(mask));                       // integer adds: the totals do not depend on their order
  if (tris) atomicAdd(&s_tot[1], tris);
  __syncthreads();
  if (tid == 0) { block_v[b] = s_tot[0]; block_t[b] = s_tot[1]; }
}

// --------------------------------------------------------------------------------------------------------------------- emit
__global__ __launch_bounds__(512) void tsdf_emit_vertices_kernel(const int* __restrict__ keys, const int* __restrict__ table,
                                                                 TsdfFrame f, const float* __restrict__ sum,
                                                                 const int* __restrict__ n, const int* __restrict__ nc,
                                                                 const int* __restrict__ rgb, long long n_blocks,
                                                                 const unsigned char* __restrict__ vmask,
                                                                 const int* __restrict__ block_vstart, long long n_vertices,
                                                                 int* __restrict__ vstart, float* __restrict__ vertices,
                                                                 unsigned char* __restrict__ colors) {
  __shared__ int s_wave[8];
  const int tid = threadIdx.x;
  const long long b = blockIdx.x, p = b * kPts + tid, plane = n_blocks * kPts;
  const BlockPos bp = block_pos(keys[b], f);
  const unsigned mask = vmask[p];
  const long long first = (long long)block_vstart[b] + block_scan(__popc(mask), s_wave);
  vstart[p] = (int)first;
  if (!mask) return;
  const int lx = tid & 7, ly = (tid >> 3) & 7, lz = tid >> 6;
  const int ia[3] = {8 * bp.x + lx, 8 * bp.y + ly, 8 * bp.z + lz};
  const double Da = (double)sum[p] / (double)n[p];
  const int nca = nc[p];
  long long out = first;
  for (int kk = 0; kk < 7; ++kk) {
    if (!(mask >> kk & 1u)) continue;
    const int d = kKindMask[kk];
    const int off[3] = {d & 1, (d >> 1) & 1, d >> 2};
    const long long q = locate(table, f, bp, lx + off[0], ly + off[1], lz + off[2], n_blocks);
    if (q < 0 || out < 0 || out >= n_vertices) { ++out; continue; }    // flags that do not belong to this volume: write nothing
    const double Db = (double)sum[q] / (double)n[q];
    const double tt = Da / (Da - Db);
    for (int a = 0; a < 3; ++a) {
      const double Xa = f.origin[a] + (double)ia[a] * f.voxel, Xb = f.origin[a] + (double)(ia[a] + off[a]) * f.voxel;
      vertices[3 * out + a] = (float)(Xa + tt * (Xb - Xa));
    }
    const int ncb = nc[q];
    for (int ch = 0; ch < 3; ++ch) {
      int col = 128;
      if (nca > 0 || ncb > 0) {
        // the endpoints' mean colours, rounded half up in integers; an endpoint without colour takes the other's
        long long ca = nca > 0 ? (2ll * rgb[ch * plane + p] + nca) / (2ll * nca) : 0;
        long long cb = ncb > 0 ? (2ll * rgb[ch * plane + q] + ncb) / (2ll * ncb) : ca;
        if (nca <= 0) ca = cb;
        const double val = floor(((double)ca + tt * (double)(cb - ca)) + 0.5);
        col = val < 0.0 ? 0 : val > 255.0 ? 255 : (int)val;
      }
      colors[3 * out + ch] = (unsigned char)col;
    }
    ++out;
  }
}

__global__ __launch_bounds__(512) void tsdf_emit_faces_kernel(const int* __restrict__ keys, const int* __restrict__ table,
                                                              TsdfFrame f, const float* __restrict__ sum, long long n_blocks,
                                                              const unsigned char* __restrict__ vmask,
                                                              const unsigned char* __restrict__ tcount,
                                                              const int* __restrict__ block_tstart,
                                                              const int* __restrict__ vstart, long long n_faces,
                                                              int* __restrict__ faces) {
  __shared__ int s_wave[8];
  const int tid = threadIdx.x;
  const long long b = blockIdx.x, p = b * kPts + tid;
  const BlockPos bp = block_pos(keys[b], f);
  const int tris = tcount[p];
  long long out = (long long)block_tstart[b] + block_scan(tris, s_wave);
  if (!tris) return;
  const int lx = tid & 7, ly = (tid >> 3) & 7, lz = tid >> 6;
  long long corner[8];
  unsigned ins = 0;
  bool ok = true;
#pragma unroll
  for (int o = 0; o < 8; ++o) {
    corner[o] = locate(table, f, bp, lx + (o & 1), ly + ((o >> 1) & 1), lz + (o >> 2), n_blocks);
    ok = ok && corner[o] >= 0;
    if (corner[o] >= 0) ins |= (sum[corner[o]] < 0.f ? 1u : 0u) << o;
  }
  if (!ok) return;                                                     // counts that do not belong to this volume
  for (int t = 0; t < 6; ++t) {
    unsigned cs = 0;
    for (int i = 0; i < 4; ++i) cs |= ((ins >> kTetCorner[t][i]) & 1u) << i;
    const int nt = kCases.n[cs];
    for (int k = 0; k < nt; ++k) {
      int id[3];
      for (int j = 0; j < 3; ++j) {
        const int e = kCases.e[cs][3 * k + j];
        const int lo = kTetCorner[t][kEdgeLo[e]], hi = kTetCorner[t][kEdgeHi[e]];
        const int kk = kKindOf[lo ^ hi];
        const long long owner = corner[lo];
        id[j] = vstart[owner] + __popc((unsigned)vmask[owner] & ((1u << kk) - 1u));
      }
      if (out >= 0 && out < n_faces) {
        const bool odd = kTetOdd[t] != 0;                              // a left-handed tetrahedron: the mirror image
        faces[3 * out] = id[0];
        faces[3 * out + 1] = id[odd ? 2 : 1];
        faces[3 * out + 2] = id[odd ? 1 : 2];
      }
      ++out;
    }
  }
}

bool frame_from_host(const double* frame_host, const int* dims_host, TsdfFrame& f) {
  if (!frame_host || !dims_host) return false;
  for (int a = 0; a < 3; ++a) {
    f.origin[a] = frame_host[a];
    f.nb[a] = dims_host[a];
    if (!(f.origin[a] == f.origin[a]) || f.nb[a] < 1) return false;
  }
  f.voxel = frame_host[3];
  if (!(f.voxel > 0.0) || !(f.voxel <= 1.7976931348623157e308)) return false;
  return (long long)f.nb[0] * f.nb[1] * f.nb[2] <= CDS_TSDF_MAX_CELLS && (long long)f.nb[0] * f.nb[1] <= CDS_TSDF_MAX_CELLS;
}

}  // namespace

extern "C" int cds_tsdf_integrate_f32(const int* keys, long long n_blocks, const double* frame_host, const int* dims_host,
                                      double trunc, const float* depths, const unsigned char* masks, const unsigned char* images,
                                      const double* cams, int n_views, int h, int w, float* sum, int* n, int* nc, int* rgb,
                                      void* stream) {
  TsdfFrame f;
  if (!frame_from_host(frame_host, dims_host, f) || n_blocks < 0 || n_blocks > CDS_TSDF_MAX_CELLS || n_views < 1 ||
      n_views > kMaxChunk || h < 1 || w < 1 || (long long)h * w * n_views > 0x7fffffffLL || !(trunc >= f.voxel) ||
      !(trunc <= 8.0 * f.voxel))
    return CDS_EINVAL;
  if (n_blocks == 0) return 0;
  if (!keys || !depths || !masks || !images || !cams || !sum || !n || !nc || !rgb) return CDS_EINVAL;
  hipLaunchKernelGGL(tsdf_integrate_kernel, dim3((unsigned)n_blocks), dim3(kPts), 0, (hipStream_t)stream, keys, f, trunc, depths,
                     masks, images, cams, n_views, h, w, sum, n, nc, rgb, n_blocks);
  return cds_launch_status();
}

extern "C" int cds_tsdf_integrate_w_f32(const int* keys, long long n_blocks, const double* frame_host, const int* dims_host,
                                        double trunc, const float* depths, const unsigned char* masks, const unsigned char* images,
                                        const double* cams, int n_views, int h, int w, float* sum, int* n, int* nc, int* rgb,
                                        const unsigned char* weights, int interp, float jump, int* wn, void* stream) {
  TsdfFrame f;
  if (!frame_from_host(frame_host, dims_host, f) || n_blocks < 0 || n_blocks > CDS_TSDF_MAX_CELLS || n_views < 1 ||
      n_views > kMaxChunk || h < 1 || w < 1 || (long long)h * w * n_views > 0x7fffffffLL || !(trunc >= f.voxel) ||
      !(trunc <= 8.0 * f.voxel) || (weights != nullptr) != (wn != nullptr) ||
      (interp != 0 && !(jump > 0.f && jump <= 3.402823466e+38f)))
    return CDS_EINVAL;
  if (n_blocks == 0) return 0;
  if (!keys || !depths || !masks || !images || !cams || !sum || !n || !nc || !rgb) return CDS_EINVAL;
  if (interp != 0)
    hipLaunchKernelGGL(tsdf_integrate_w_kernel<true>, dim3((unsigned)n_blocks), dim3(kPts), 0, (hipStream_t)stream, keys, f, trunc,
                       depths, masks, images, weights, jump, cams, n_views, h, w, sum, n, nc, rgb, wn, n_blocks);
  else
    hipLaunchKernelGGL(tsdf_integrate_w_kernel<false>, dim3((unsigned)n_blocks), dim3(kPts), 0, (hipStream_t)stream, keys, f, trunc,
                       depths, masks, images, weights, jump, cams, n_views, h, w, sum, n, nc, rgb, wn, n_blocks);
  return cds_launch_status();
}

extern "C" int cds_tsdf_view_weights(const float* depth, const unsigned char* mask, const float* normals, const unsigned char* ok,
                                     const float* conf, const float* cam_host, int h, int w, unsigned char* weights, void* stream) {
  if (!depth || !mask || !cam_host || !weights || (normals != nullptr) != (ok != nullptr) || h < 1 || w < 1 ||
      (long long)h * w > 0x7fffffffLL)
    return CDS_EINVAL;
  if (!(cam_host[3] == 0.f && cam_host[6] == 0.f && cam_host[7] == 0.f && cam_host[8] == 1.f)) return CDS_EINVAL;
  WeightCam cam;
  cam.fx = cam_host[0]; cam.s = cam_host[1]; cam.cx = cam_host[2]; cam.fy = cam_host[4]; cam.cy = cam_host[5];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) cam.R[3 * r + c] = cam_host[9 + 4 * r + c];
  hipLaunchKernelGGL(tsdf_view_weights_kernel, dim3((unsigned)(((long long)h * w + 255) / 256)), dim3(256), 0,
                     (hipStream_t)stream, depth, mask, normals, ok, conf, cam, h, w, weights);
  return cds_launch_status();
}

extern "C" int cds_tsdf_classify(const int* keys, const int* table, long long n_blocks, const double* frame_host,
                                 const int* dims_host, const float* sum, const int* n, int min_weight, unsigned char* vmask,
                                 unsigned char* tcount, int* block_vertices, int* block_faces, void* stream) {
  TsdfFrame f;
  if (!frame_from_host(frame_host, dims_host, f) || n_blocks < 0 || n_blocks > CDS_TSDF_MAX_CELLS || min_weight < 1)
    return CDS_EINVAL;
  if (n_blocks == 0) return 0;
  if (!keys || !table || !sum || !n || !vmask || !tcount || !block_vertices || !block_faces) return CDS_EINVAL;
  hipLaunchKernelGGL(tsdf_classify_kernel, dim3((unsigned)n_blocks), dim3(kPts), 0, (hipStream_t)stream, keys, table, f, sum, n,
                     min_weight, n_blocks, vmask, tcount, block_vertices, block_faces);
  return cds_launch_status();
}

extern "C" int cds_tsdf_emit(const int* keys, const int* table, long long n_blocks, const double* frame_host, const int* dims_host,
                             const float* sum, const int* n, const int* nc, const int* rgb, const unsigned char* vmask,
                             const unsigned char* tcount, const int* block_vstart, const int* block_tstart, long long n_vertices,
                             long long n_faces, int* vstart, float* vertices, unsigned char* colors, int* faces, void* stream) {
  TsdfFrame f;
  if (!frame_from_host(frame_host, dims_host, f) || n_blocks < 0 || n_blocks > CDS_TSDF_MAX_CELLS || n_vertices < 0 ||
      n_faces < 0 || n_vertices > 0x7fffffffLL || n_faces > 0x7fffffffLL)
    return CDS_EINVAL;
  if (n_blocks == 0) return 0;
  if (!keys || !table || !sum || !n || !nc || !rgb || !vmask || !tcount || !block_vstart || !block_tstart || !vstart ||
      (n_vertices > 0 && (!vertices || !colors)) || (n_faces > 0 && !faces))
    return CDS_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(tsdf_emit_vertices_kernel, dim3((unsigned)n_blocks), dim3(kPts), 0, st, keys, table, f, sum, n, nc, rgb,
                     n_blocks, vmask, block_vstart, n_vertices, vstart, vertices, colors);
  int rc = cds_launch_status();
  if (rc != 0 || n_faces == 0) return rc;
  hipLaunchKernelGGL(tsdf_emit_faces_kernel, dim3((unsigned)n_blocks), dim3(kPts), 0, st, keys, table, f, sum, n_blocks, vmask,
                     tcount, block_tstart, vstart, n_faces, faces);
  return cds_launch_status();
}
