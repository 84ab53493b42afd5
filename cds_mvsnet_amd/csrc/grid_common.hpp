// The sparse uniform grid shared by pointcloud.hip (DTU evaluation) and registration.hip (Tanks and Temples evaluation): frame,
// key packing, hash lookup, pruning bounds and the nearest-neighbour walk.  See pointcloud.hip for the layout.
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

// What the walk has found so far.  d2: the smallest squared distance (starts at cap^2).  index / pos (WITH_INDEX only): the input
// index (w lane of the point) and the sorted position of the point that gave it; among equal d2 the lowest input index.
struct Nearest {
  float d2;
  int index, pos;
};

template <bool WITH_INDEX>
__device__ __forceinline__ void scan_points(const float4* __restrict__ pts, int b, int e, float qx, float qy, float qz, Nearest& n) {
  for (int j = b; j < e; ++j) {
    const float4 p = pts[j];
    const float dx = p.x - qx, dy = p.y - qy, dz = p.z - qz;
    const float d2 = dx * dx + dy * dy + dz * dz;
    if (WITH_INDEX) {
      const int idx = __float_as_int(p.w);
      if (d2 < n.d2 || (d2 == n.d2 && idx < n.index)) { n.d2 = d2; n.index = idx; n.pos = j; }
    } else {
      n.d2 = fminf(n.d2, d2);
    }
  }
}

// May a region whose points are all at least lb2 (squared) away be skipped?  For distances alone an equal candidate changes
// nothing.  With the index an equal candidate may carry a lower index, so only a strictly farther region goes - or one at or
// beyond the cap, where nothing is accepted.
template <bool WITH_INDEX>
__device__ __forceinline__ bool prunable(float lb2, float best2, float cap2) {
  return WITH_INDEX ? (lb2 > best2 || lb2 >= cap2) : lb2 >= best2;
}

// distance along one axis from q to the slab of coarse cells at coordinate c (fine cells [8c, 8c + 8))
__device__ __forceinline__ float slab_dist(float q, float o, float h, int c) {
  const float lo = o + (float)(8 * c) * h, hi = o + (float)(8 * c + 8) * h;
  return fmaxf(fmaxf(lo - q, q - hi), 0.0f);
}

// Capped nearest neighbour of q in the grid: 27 fine cells around the query, then coarse rings with box pruning.  -> n.d2, the
// smallest d2 = dx*dx + dy*dy + dz*dz (fp32) below cap2, or cap2; WITH_INDEX also which point (Nearest).
template <bool WITH_INDEX>
__device__ __forceinline__ Nearest nn_walk(const GridView& g, float qx, float qy, float qz, float cap2) {
  const Frame& f = g.f;
  const int ncx = (f.nx + 7) >> 3, ncy = (f.ny + 7) >> 3, ncz = (f.nz + 7) >> 3;
  Nearest n{cap2, 0x7fffffff, -1};
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
          if (c >= 0) scan_points<WITH_INDEX>(g.pts, g.cell_start[c], g.cell_start[c + 1], qx, qy, qz, n);
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
    done = lb > 0.0f && prunable<WITH_INDEX>(lb * lb, n.d2, cap2);
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
        if (lb == INFINITY) break;
        lb -= f.slop;
        if (lb > 0.0f && prunable<WITH_INDEX>(lb * lb, n.d2, cap2)) break;
      }
      for (int cz = max(ccz - R, 0); cz <= min(ccz + R, ncz - 1); ++cz)
        for (int cy = max(ccy - R, 0); cy <= min(ccy + R, ncy - 1); ++cy) {
          const bool row = abs(cz - ccz) == R || abs(cy - ccy) == R;
          const int x0 = row ? max(ccx - R, 0) : ccx - R, x1 = row ? min(ccx + R, ncx - 1) : ccx + R;
          const int step = row || R == 0 ? 1 : 2 * R;
          for (int cx = x0; cx <= x1; cx += step) {
            if (cx < 0 || cx >= ncx) continue;
            if (prunable<WITH_INDEX>(box_d2(qx, qy, qz, f.ox + (float)(8 * cx) * f.h, f.oy + (float)(8 * cy) * f.h,
                                            f.oz + (float)(8 * cz) * f.h, hw, f.slop), n.d2, cap2))
              continue;
            const int c = find(g.t, coarse_bits(cx, cy, cz) | kCoarse);
            if (c < 0) continue;
            for (int fc = g.coarse_start[c]; fc < g.coarse_start[c + 1]; ++fc) {
              int x, y, z;
              decode_fine(g.cell_keys[fc], x, y, z);
              if (inside && abs(x - ix) <= 1 && abs(y - iy) <= 1 && abs(z - iz) <= 1) continue;   // done in step 1
              if (prunable<WITH_INDEX>(box_d2(qx, qy, qz, f.ox + (float)x * f.h, f.oy + (float)y * f.h, f.oz + (float)z * f.h, f.h,
                                              f.slop), n.d2, cap2))
                continue;
              scan_points<WITH_INDEX>(g.pts, g.cell_start[fc], g.cell_start[fc + 1], qx, qy, qz, n);
            }
          }
        }
    }
  }
  return n;
}

// The walk of nn_walk<false> for a sink that keeps more than one candidate (the k nearest: cloud_outlier.hip).  The sink has
//   float bound() const   a region whose points are all at least this far (squared) cannot change it: the pruning threshold,
//                         nn_walk's best2 (an equal candidate changes nothing, so >= prunes, as prunable<false>)
//   void add(float d2)    one candidate, d2 = dx*dx + dy*dy + dz*dz as scan_points
// Same cells in the same order, same bounds; nn_walk itself is untouched so that its callers keep their bits.
template <class Sink>
__device__ __forceinline__ void sink_points(const float4* __restrict__ pts, int b, int e, float qx, float qy, float qz, Sink& s) {
  for (int j = b; j < e; ++j) {
    const float4 p = pts[j];
    const float dx = p.x - qx, dy = p.y - qy, dz = p.z - qz;
    s.add(dx * dx + dy * dy + dz * dz);
  }
}

template <class Sink>
__device__ __forceinline__ void knn_walk(const GridView& g, float qx, float qy, float qz, Sink& s) {
  const Frame& f = g.f;
  const int ncx = (f.nx + 7) >> 3, ncy = (f.ny + 7) >> 3, ncz = (f.nz + 7) >> 3;
  const float fx = cell_of(qx, f.ox, f.h), fy = cell_of(qy, f.oy, f.h), fz = cell_of(qz, f.oz, f.h);
  const bool inside = fx >= 0.0f && fx < (float)f.nx && fy >= 0.0f && fy < (float)f.ny && fz >= 0.0f && fz < (float)f.nz;
  int ix = 0, iy = 0, iz = 0;
  if (inside) {
    // 1. the 27 fine cells around the query
    ix = (int)fx; iy = (int)fy; iz = (int)fz;
    for (int z = max(iz - 1, 0); z <= min(iz + 1, f.nz - 1); ++z)
      for (int y = max(iy - 1, 0); y <= min(iy + 1, f.ny - 1); ++y)
        for (int x = max(ix - 1, 0); x <= min(ix + 1, f.nx - 1); ++x) {
          const int c = find(g.t, fine_key(x, y, z));
          if (c >= 0) sink_points(g.pts, g.cell_start[c], g.cell_start[c + 1], qx, qy, qz, s);
        }
    float lb = INFINITY;
    if (ix - 1 > 0) lb = fminf(lb, qx - (f.ox + (float)(ix - 1) * f.h));
    if (ix + 2 < f.nx) lb = fminf(lb, f.ox + (float)(ix + 2) * f.h - qx);
    if (iy - 1 > 0) lb = fminf(lb, qy - (f.oy + (float)(iy - 1) * f.h));
    if (iy + 2 < f.ny) lb = fminf(lb, f.oy + (float)(iy + 2) * f.h - qy);
    if (iz - 1 > 0) lb = fminf(lb, qz - (f.oz + (float)(iz - 1) * f.h));
    if (iz + 2 < f.nz) lb = fminf(lb, f.oz + (float)(iz + 2) * f.h - qz);
    lb -= f.slop;
    if (lb > 0.0f && lb * lb >= s.bound()) return;
  }
  // 2. rings of coarse cells around the query's (clamped) coarse cell, nearest first
  const int ccx = clamp_cell(floorf(fx * 0.125f), ncx), ccy = clamp_cell(floorf(fy * 0.125f), ncy),
            ccz = clamp_cell(floorf(fz * 0.125f), ncz);
  const float hw = 8.0f * f.h;
  for (int R = 0;; ++R) {
    if (R > 0) {
      float lb = INFINITY;
      if (ccx + R < ncx) lb = fminf(lb, slab_dist(qx, f.ox, f.h, ccx + R));
      if (ccx - R >= 0) lb = fminf(lb, slab_dist(qx, f.ox, f.h, ccx - R));
      if (ccy + R < ncy) lb = fminf(lb, slab_dist(qy, f.oy, f.h, ccy + R));
      if (ccy - R >= 0) lb = fminf(lb, slab_dist(qy, f.oy, f.h, ccy - R));
      if (ccz + R < ncz) lb = fminf(lb, slab_dist(qz, f.oz, f.h, ccz + R));
      if (ccz - R >= 0) lb = fminf(lb, slab_dist(qz, f.oz, f.h, ccz - R));
      if (lb == INFINITY) break;                      // the grid is exhausted
      lb -= f.slop;
      if (lb > 0.0f && lb * lb >= s.bound()) break;
    }
    for (int cz = max(ccz - R, 0); cz <= min(ccz + R, ncz - 1); ++cz)
      for (int cy = max(ccy - R, 0); cy <= min(ccy + R, ncy - 1); ++cy) {
        const bool row = abs(cz - ccz) == R || abs(cy - ccy) == R;
        const int x0 = row ? max(ccx - R, 0) : ccx - R, x1 = row ? min(ccx + R, ncx - 1) : ccx + R;
        const int step = row || R == 0 ? 1 : 2 * R;
        for (int cx = x0; cx <= x1; cx += step) {
          if (cx < 0 || cx >= ncx) continue;
          if (box_d2(qx, qy, qz, f.ox + (float)(8 * cx) * f.h, f.oy + (float)(8 * cy) * f.h, f.oz + (float)(8 * cz) * f.h, hw,
                     f.slop) >= s.bound())
            continue;
          const int c = find(g.t, coarse_bits(cx, cy, cz) | kCoarse);
          if (c < 0) continue;
          for (int fc = g.coarse_start[c]; fc < g.coarse_start[c + 1]; ++fc) {
            int x, y, z;
            decode_fine(g.cell_keys[fc], x, y, z);
            if (inside && abs(x - ix) <= 1 && abs(y - iy) <= 1 && abs(z - iz) <= 1) continue;   // done in step 1
            if (box_d2(qx, qy, qz, f.ox + (float)x * f.h, f.oy + (float)y * f.h, f.oz + (float)z * f.h, f.h, f.slop) >= s.bound())
              continue;
            sink_points(g.pts, g.cell_start[fc], g.cell_start[fc + 1], qx, qy, qz, s);
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

inline int grid_blocks(long long n) { return (int)(n < 1 ? 1 : (n + 255) / 256 < 8192 ? (n + 255) / 256 : 8192); }

}  // namespace
