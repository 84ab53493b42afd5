// The sparse uniform grid shared by pointcloud.hip (DTU evaluation), registration.hip (Tanks and Temples evaluation) and
// cloud_outlier.hip (outlier filters): frame, key packing, hash lookup, pruning bounds, the one neighbour walk (grid_walk) with
// its sinks, and the check of the C ABI's grid arguments (grid_view).  See pointcloud.hip for the layout.
//
// Everything here sits in an anonymous namespace: each translation unit gets its own copy, nothing is exported.
#pragma once
#include "cds_common.hpp"

namespace {

constexpr unsigned long long kEmpty = ~0ull;
constexpr unsigned long long kCoarse = 1ull << 63;
constexpr int kMaxAxis = 1 << 21;   // fine cells per axis (18 coarse bits + 3 local bits)

struct Frame {
  float ox, oy, oz, h, slop;
  int nx, ny, nz;
};

struct Table {
  const unsigned long long* keys;
  const int* vals;
  unsigned long long mask;
};

// a built grid as the query kernels read it (PointGrid of pointcloud.py)
struct GridView {
  const float4* pts;
  const int* cell_start;
  const unsigned long long* cell_keys;
  const int* coarse_start;
  Table t;
  Frame f;
};

__host__ __device__ __forceinline__ unsigned long long mix64(unsigned long long k) {   // murmur3 finaliser
  k ^= k >> 33;
  k *= 0xff51afd7ed558ccdull;
  k ^= k >> 33;
  k *= 0xc4ceb9fe1a85ec53ull;
  k ^= k >> 33;
  return k;
}

__device__ __forceinline__ unsigned long long coarse_bits(int cx, int cy, int cz) {
  return ((unsigned long long)cx << 36) | ((unsigned long long)cy << 18) | (unsigned long long)cz;
}

__device__ __forceinline__ unsigned long long fine_key(int x, int y, int z) {
  const unsigned long long local = (unsigned long long)(((x & 7) << 6) | ((y & 7) << 3) | (z & 7));
  return (coarse_bits(x >> 3, y >> 3, z >> 3) << 9) | local;
}

__device__ __forceinline__ void decode_fine(unsigned long long k, int& x, int& y, int& z) {
  const unsigned long long c = k >> 9;
  x = (int)(((c >> 36) & 0x3ffff) << 3) | (int)((k >> 6) & 7);
  y = (int)(((c >> 18) & 0x3ffff) << 3) | (int)((k >> 3) & 7);
  z = (int)((c & 0x3ffff) << 3) | (int)(k & 7);
}

// cell coordinate as a float (exact integer or +-huge); binning and queries use this one expression
__device__ __forceinline__ float cell_of(float p, float o, float h) { return floorf((p - o) / h); }

__device__ __forceinline__ int clamp_cell(float c, int n) { return (int)fminf(fmaxf(c, 0.0f), (float)(n - 1)); }

__device__ __forceinline__ int find(const Table& t, unsigned long long key) {
  unsigned long long s = mix64(key) & t.mask;
  while (true) {
    const unsigned long long k = t.keys[s];
    if (k == key) return t.vals[s];
    if (k == kEmpty) return -1;
    s = (s + 1) & t.mask;
  }
}

// squared distance from q to the box [lo, lo + w] on every axis, the box widened by slop
__device__ __forceinline__ float box_d2(float qx, float qy, float qz, float lx, float ly, float lz, float w, float slop) {
  const float ax = fmaxf(fmaxf(lx - slop - qx, qx - (lx + w + slop)), 0.0f);
  const float ay = fmaxf(fmaxf(ly - slop - qy, qy - (ly + w + slop)), 0.0f);
  const float az = fmaxf(fmaxf(lz - slop - qz, qz - (lz + w + slop)), 0.0f);
  return ax * ax + ay * ay + az * az;
}

// distance along one axis from q to the slab of coarse cells at coordinate c (fine cells [8c, 8c + 8))
__device__ __forceinline__ float slab_dist(float q, float o, float h, int c) {
  const float lo = o + (float)(8 * c) * h, hi = o + (float)(8 * c + 8) * h;
  return fmaxf(fmaxf(lo - q, q - hi), 0.0f);
}

// The walk hands every candidate to a sink, and the sink says what may be skipped:
//   bool skips(float lb2) const                    may a region whose points are all at least lb2 (squared) away be skipped?
//   void add(float d2, const float4& p, int j)     one candidate: d2 = dx*dx + dy*dy + dz*dz (fp32), the point, its sorted position
// NearestDist and NearestIndex are the two one-neighbour sinks; cloud_outlier.hip has KnnList, the k nearest.

// The smallest d2 below cap2, or cap2 (d2 starts at cap2).  An equal candidate changes nothing, so an equal region goes too.
struct NearestDist {
  float d2;
  __device__ __forceinline__ bool skips(float lb2) const { return lb2 >= d2; }
  __device__ __forceinline__ void add(float c, const float4&, int) { d2 = fminf(d2, c); }
};

// NearestDist that also says which point: index is its input index (the w lane of the point), pos its sorted position; among
// equal d2 the lowest input index.  Here an equal candidate may carry a lower index, so only a strictly farther region goes -
// or one at or beyond the cap, where nothing is accepted.  Starts as {cap2, cap2, 0x7fffffff, -1}.
struct NearestIndex {
  float d2, cap2;
  int index, pos;
  __device__ __forceinline__ bool skips(float lb2) const { return lb2 > d2 || lb2 >= cap2; }
  __device__ __forceinline__ void add(float c, const float4& p, int j) {
    const int idx = __float_as_int(p.w);
    // selects, not a branch: this is the innermost loop of nn_index_kernel and icp_sums_kernel (profiles/grid_walk.md)
    const bool take = c < d2 || (c == d2 && idx < index);
    d2 = take ? c : d2;
    index = take ? idx : index;
    pos = take ? j : pos;
  }
};

template <class Sink>
__device__ __forceinline__ void scan_cell(const float4* __restrict__ pts, int b, int e, float qx, float qy, float qz, Sink& s) {
  for (int j = b; j < e; ++j) {
    const float4 p = pts[j];
    const float dx = p.x - qx, dy = p.y - qy, dz = p.z - qz;
    s.add(dx * dx + dy * dy + dz * dz, p, j);
  }
}

// The neighbours of q in the grid, nearest cells first: the 27 fine cells around the query, then rings of coarse cells with
// slab, coarse-box and fine-box pruning.  Every bound is widened by the frame's slop, so a region is skipped only when the sink
// says that nothing in it can matter.
template <class Sink>
__device__ __forceinline__ void grid_walk(const GridView& g, float qx, float qy, float qz, Sink& s) {
  const Frame& f = g.f;
  const int ncx = (f.nx + 7) >> 3, ncy = (f.ny + 7) >> 3, ncz = (f.nz + 7) >> 3;
  const float fx = cell_of(qx, f.ox, f.h), fy = cell_of(qy, f.oy, f.h), fz = cell_of(qz, f.oz, f.h);
  const bool inside = fx >= 0.0f && fx < (float)f.nx && fy >= 0.0f && fy < (float)f.ny && fz >= 0.0f && fz < (float)f.nz;
  int ix = 0, iy = 0, iz = 0;
  bool done = false;
  if (inside) {
    // 1. the 27 fine cells around the query
    ix = (int)fx; iy = (int)fy; iz = (int)fz;
    for (int z = max(iz - 1, 0); z <= min(iz + 1, f.nz - 1); ++z)
      for (int y = max(iy - 1, 0); y <= min(iy + 1, f.ny - 1); ++y)
        for (int x = max(ix - 1, 0); x <= min(ix + 1, f.nx - 1); ++x) {
          const int c = find(g.t, fine_key(x, y, z));
          if (c >= 0) scan_cell(g.pts, g.cell_start[c], g.cell_start[c + 1], qx, qy, qz, s);
        }
    // nothing outside the 3x3x3 block is nearer than its boundary (sides at the grid's edge have nothing beyond them)
    float lb = INFINITY;
    if (ix - 1 > 0) lb = fminf(lb, qx - (f.ox + (float)(ix - 1) * f.h));
    if (ix + 2 < f.nx) lb = fminf(lb, f.ox + (float)(ix + 2) * f.h - qx);
    if (iy - 1 > 0) lb = fminf(lb, qy - (f.oy + (float)(iy - 1) * f.h));
    if (iy + 2 < f.ny) lb = fminf(lb, f.oy + (float)(iy + 2) * f.h - qy);
    if (iz - 1 > 0) lb = fminf(lb, qz - (f.oz + (float)(iz - 1) * f.h));
    if (iz + 2 < f.nz) lb = fminf(lb, f.oz + (float)(iz + 2) * f.h - qz);
    lb -= f.slop;
    done = lb > 0.0f && s.skips(lb * lb);
  }
  if (!done) {
    // 2. rings of coarse cells around the query's (clamped) coarse cell, nearest first
    const int ccx = clamp_cell(floorf(fx * 0.125f), ncx), ccy = clamp_cell(floorf(fy * 0.125f), ncy),
              ccz = clamp_cell(floorf(fz * 0.125f), ncz);
    const float hw = 8.0f * f.h;
    for (int R = 0;; ++R) {
      if (R > 0) {
        // every cell of ring R lies in one of the six slabs at coarse distance R; slabs outside the grid hold nothing
        float lb = INFINITY;
        if (ccx + R < ncx) lb = fminf(lb, slab_dist(qx, f.ox, f.h, ccx + R));
        if (ccx - R >= 0) lb = fminf(lb, slab_dist(qx, f.ox, f.h, ccx - R));
        if (ccy + R < ncy) lb = fminf(lb, slab_dist(qy, f.oy, f.h, ccy + R));
        if (ccy - R >= 0) lb = fminf(lb, slab_dist(qy, f.oy, f.h, ccy - R));
        if (ccz + R < ncz) lb = fminf(lb, slab_dist(qz, f.oz, f.h, ccz + R));
        if (ccz - R >= 0) lb = fminf(lb, slab_dist(qz, f.oz, f.h, ccz - R));
        if (lb == INFINITY) break;                      // the grid is exhausted
        lb -= f.slop;
        if (lb > 0.0f && s.skips(lb * lb)) break;
      }
      for (int cz = max(ccz - R, 0); cz <= min(ccz + R, ncz - 1); ++cz)
        for (int cy = max(ccy - R, 0); cy <= min(ccy + R, ncy - 1); ++cy) {
          const bool row = abs(cz - ccz) == R || abs(cy - ccy) == R;
          const int x0 = row ? max(ccx - R, 0) : ccx - R, x1 = row ? min(ccx + R, ncx - 1) : ccx + R;
          const int step = row || R == 0 ? 1 : 2 * R;
          for (int cx = x0; cx <= x1; cx += step) {
            if (cx < 0 || cx >= ncx) continue;
            if (s.skips(box_d2(qx, qy, qz, f.ox + (float)(8 * cx) * f.h, f.oy + (float)(8 * cy) * f.h, f.oz + (float)(8 * cz) * f.h,
                               hw, f.slop)))
              continue;
            const int c = find(g.t, coarse_bits(cx, cy, cz) | kCoarse);
            if (c < 0) continue;
            for (int fc = g.coarse_start[c]; fc < g.coarse_start[c + 1]; ++fc) {
              int x, y, z;
              decode_fine(g.cell_keys[fc], x, y, z);
              if (inside && abs(x - ix) <= 1 && abs(y - iy) <= 1 && abs(z - iz) <= 1) continue;   // done in step 1
              if (s.skips(box_d2(qx, qy, qz, f.ox + (float)x * f.h, f.oy + (float)y * f.h, f.oz + (float)z * f.h, f.h, f.slop)))
                continue;
              scan_cell(g.pts, g.cell_start[fc], g.cell_start[fc + 1], qx, qy, qz, s);
            }
          }
        }
    }
  }
}

inline bool read_frame(const float* fh, Frame& f) {
  if (!fh) return false;
  f.ox = fh[0]; f.oy = fh[1]; f.oz = fh[2]; f.h = fh[3]; f.slop = fh[4];
  f.nx = (int)fh[5]; f.ny = (int)fh[6]; f.nz = (int)fh[7];
  return f.h > 0.0f && f.slop >= 0.0f && f.nx >= 1 && f.ny >= 1 && f.nz >= 1 && f.nx <= kMaxAxis && f.ny <= kMaxAxis &&
         f.nz <= kMaxAxis && (float)f.nx == fh[5] && (float)f.ny == fh[6] && (float)f.nz == fh[7];
}

// The eight grid arguments of the C ABI as a GridView; false if a pointer is missing, log2_slots is outside 1..40 or the frame
// is not one (read_frame).
inline bool grid_view(const float* pts, const int* cell_start, const long long* cell_keys, const int* coarse_start,
                      const long long* table_keys, const int* table_vals, int log2_slots, const float* frame_host, GridView& g) {
  if (!pts || !cell_start || !cell_keys || !coarse_start || !table_keys || !table_vals || log2_slots < 1 || log2_slots > 40 ||
      !read_frame(frame_host, g.f))
    return false;
  g.pts = (const float4*)pts;
  g.cell_start = cell_start;
  g.cell_keys = (const unsigned long long*)cell_keys;
  g.coarse_start = coarse_start;
  g.t = Table{(const unsigned long long*)table_keys, table_vals, (1ull << log2_slots) - 1};
  return true;
}

inline int grid_blocks(long long n) { return (int)(n < 1 ? 1 : (n + 255) / 256 < 8192 ? (n + 255) / 256 : 8192); }

}  // namespace
