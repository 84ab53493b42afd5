// Point-cloud evaluation kernels (DTU Acc / Comp protocol, evaluations/dtu/*.m of the reference; cds_mvsnet_amd/dtu_eval.py).
//
// A sparse uniform grid over a point set: fine cells of side h, addressed by 63-bit keys that put the coarse cell (8 x 8 x 8 fine
// cells) in the high bits and the fine position inside it in the low 9 bits.  Sorted by key, the points of one fine cell and the
// fine cells of one coarse cell are contiguous ranges (CSR arrays built on the host side with torch.sort / cumsum).  One open-
// addressing hash table maps a fine key to its fine-cell index and a coarse key (bit 63 set) to its coarse-cell index.
//
//   cds_grid_keys_f32        per point: the fine key of its cell (cell coordinates clamped to the grid)
//   cds_grid_hash_build      insert the unique fine and coarse keys (64-bit CAS; the table is independent of insertion order)
//   cds_nn_query_f32         capped nearest-neighbour distance (MaxDistCP.m), one query per lane in cell order:
//                            27 fine cells around the query, then coarse rings with box pruning; empty space costs one
//                            coarse lookup per 8^3 fine cells
//   cds_thin_round_f32       one round of the greedy thinning of reducePts_haa.m (cell side >= dst: 27 cells cover dst)
//
// Frame (frame_host, 8 floats): origin x y z, cell side h, slop, fine cells per axis nx ny nz.  `slop` bounds how far outside
// its nominal cell box fp32 binning can put a point; every pruning test is widened by it, so pruning never drops a candidate.
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

__device__ __forceinline__ float scan_points(const float4* __restrict__ pts, int b, int e, float qx, float qy, float qz,
                                             float best2) {
  for (int j = b; j < e; ++j) {
    const float4 p = pts[j];
    const float dx = p.x - qx, dy = p.y - qy, dz = p.z - qz;
    const float d2 = dx * dx + dy * dy + dz * dz;
    best2 = fminf(best2, d2);
  }
  return best2;
}

// distance along one axis from q to the slab of coarse cells at coordinate c (fine cells [8c, 8c + 8))
__device__ __forceinline__ float slab_dist(float q, float o, float h, int c) {
  const float lo = o + (float)(8 * c) * h, hi = o + (float)(8 * c + 8) * h;
  return fmaxf(fmaxf(lo - q, q - hi), 0.0f);
}

__global__ __launch_bounds__(256) void grid_keys_kernel(const float* __restrict__ pts, long long n, Frame f,
                                                        long long* __restrict__ keys) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const int x = clamp_cell(cell_of(pts[3 * i], f.ox, f.h), f.nx);
    const int y = clamp_cell(cell_of(pts[3 * i + 1], f.oy, f.h), f.ny);
    const int z = clamp_cell(cell_of(pts[3 * i + 2], f.oz, f.h), f.nz);
    keys[i] = (long long)fine_key(x, y, z);
  }
}

__global__ __launch_bounds__(256) void hash_clear_kernel(unsigned long long* __restrict__ keys, long long slots) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < slots; i += (long long)gridDim.x * blockDim.x)
    keys[i] = kEmpty;
}

// keys are unique: the slot a key ends in depends on the insertion order, what find() returns does not
__global__ __launch_bounds__(256) void hash_insert_kernel(const long long* __restrict__ in, long long n, long long n_fine,
                                                          unsigned long long* __restrict__ keys, int* __restrict__ vals,
                                                          unsigned long long mask) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const unsigned long long key = (unsigned long long)in[i];
    unsigned long long s = mix64(key) & mask;
    while (true) {
      const unsigned long long prev = atomicCAS(&keys[s], kEmpty, key);
      if (prev == kEmpty || prev == key) break;
      s = (s + 1) & mask;
    }
    vals[s] = (int)(i < n_fine ? i : i - n_fine);
  }
}

__global__ __launch_bounds__(256) void nn_query_kernel(const float* __restrict__ query, const long long* __restrict__ order,
                                                       long long m, const float4* __restrict__ pts,
                                                       const int* __restrict__ cell_start,
                                                       const unsigned long long* __restrict__ cell_keys,
                                                       const int* __restrict__ coarse_start, Table t, Frame f, float cap,
                                                       float* __restrict__ dist) {
  const int ncx = (f.nx + 7) >> 3, ncy = (f.ny + 7) >> 3, ncz = (f.nz + 7) >> 3;
  const float cap2 = cap * cap;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (long long)gridDim.x * blockDim.x) {
    const long long qi = order ? order[i] : i;
    const float qx = query[3 * qi], qy = query[3 * qi + 1], qz = query[3 * qi + 2];
    float best2 = cap2;
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
            const int c = find(t, fine_key(x, y, z));
            if (c >= 0) best2 = scan_points(pts, cell_start[c], cell_start[c + 1], qx, qy, qz, best2);
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
      done = lb > 0.0f && lb * lb >= best2;
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
          if (lb > 0.0f && lb * lb >= best2) break;
        }
        for (int cz = max(ccz - R, 0); cz <= min(ccz + R, ncz - 1); ++cz)
          for (int cy = max(ccy - R, 0); cy <= min(ccy + R, ncy - 1); ++cy) {
            const bool row = abs(cz - ccz) == R || abs(cy - ccy) == R;
            const int x0 = row ? max(ccx - R, 0) : ccx - R, x1 = row ? min(ccx + R, ncx - 1) : ccx + R;
            const int step = row || R == 0 ? 1 : 2 * R;
            for (int cx = x0; cx <= x1; cx += step) {
              if (cx < 0 || cx >= ncx) continue;
              if (box_d2(qx, qy, qz, f.ox + (float)(8 * cx) * f.h, f.oy + (float)(8 * cy) * f.h, f.oz + (float)(8 * cz) * f.h, hw,
                         f.slop) >= best2)
                continue;
              const int c = find(t, coarse_bits(cx, cy, cz) | kCoarse);
              if (c < 0) continue;
              for (int fc = coarse_start[c]; fc < coarse_start[c + 1]; ++fc) {
                int x, y, z;
                decode_fine(cell_keys[fc], x, y, z);
                if (inside && abs(x - ix) <= 1 && abs(y - iy) <= 1 && abs(z - iz) <= 1) continue;   // done in step 1
                if (box_d2(qx, qy, qz, f.ox + (float)x * f.h, f.oy + (float)y * f.h, f.oz + (float)z * f.h, f.h, f.slop) >= best2)
                  continue;
                best2 = scan_points(pts, cell_start[fc], cell_start[fc + 1], qx, qy, qz, best2);
              }
            }
          }
      }
    }
    dist[qi] = best2 < cap2 ? fminf(sqrtf(best2), cap) : cap;
  }
}

// One round of the greedy maximal independent set in rank order (reducePts_haa.m:19-31): an undecided point becomes KEPT once
// no lower-rank neighbour within dst is undecided or kept, REMOVED as soon as one is kept.  Decided states are final and each
// decision holds whatever the other lanes have written so far, so the result does not depend on timing.
__global__ __launch_bounds__(256) void thin_round_kernel(const float4* __restrict__ pts, const int* __restrict__ cell_start,
                                                         long long n, Table t, Frame f, float dst2,
                                                         unsigned char* __restrict__ state, int* __restrict__ undecided) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    if (state[i] != 0) continue;
    const float4 p = pts[i];
    const int rank = __float_as_int(p.w);
    const int ix = clamp_cell(cell_of(p.x, f.ox, f.h), f.nx), iy = clamp_cell(cell_of(p.y, f.oy, f.h), f.ny),
              iz = clamp_cell(cell_of(p.z, f.oz, f.h), f.nz);
    bool removed = false, pending = false;
    for (int z = max(iz - 1, 0); z <= min(iz + 1, f.nz - 1) && !removed; ++z)
      for (int y = max(iy - 1, 0); y <= min(iy + 1, f.ny - 1) && !removed; ++y)
        for (int x = max(ix - 1, 0); x <= min(ix + 1, f.nx - 1) && !removed; ++x) {
          const int c = find(t, fine_key(x, y, z));
          if (c < 0) continue;
          const int e = cell_start[c + 1];
          for (int j = cell_start[c]; j < e; ++j) {
            const float4 q = pts[j];
            if (__float_as_int(q.w) >= rank) continue;
            const float dx = q.x - p.x, dy = q.y - p.y, dz = q.z - p.z;
            if (dx * dx + dy * dy + dz * dz <= dst2) {
              const unsigned char s = __atomic_load_n(&state[j], __ATOMIC_RELAXED);
              if (s == 1) { removed = true; break; }
              if (s == 0) pending = true;
            }
          }
        }
    if (removed) state[i] = 2;
    else if (!pending) state[i] = 1;
    else if (undecided) atomicAdd(undecided, 1);
  }
}

bool read_frame(const float* fh, Frame& f) {
  if (!fh) return false;
  f.ox = fh[0]; f.oy = fh[1]; f.oz = fh[2]; f.h = fh[3]; f.slop = fh[4];
  f.nx = (int)fh[5]; f.ny = (int)fh[6]; f.nz = (int)fh[7];
  return f.h > 0.0f && f.slop >= 0.0f && f.nx >= 1 && f.ny >= 1 && f.nz >= 1 && f.nx <= kMaxAxis && f.ny <= kMaxAxis &&
         f.nz <= kMaxAxis && (float)f.nx == fh[5] && (float)f.ny == fh[6] && (float)f.nz == fh[7];
}

int grid_blocks(long long n) { return (int)(n < 1 ? 1 : (n + 255) / 256 < 8192 ? (n + 255) / 256 : 8192); }

}  // namespace

extern "C" int cds_grid_hash_log2_slots(long long n_keys) {
  if (n_keys < 0 || n_keys > (1ll << 33)) return CDS_EINVAL;
  int b = 6;
  while ((1ll << b) < 2 * n_keys) ++b;   // load factor <= 1/2
  return b;
}

extern "C" int cds_grid_keys_f32(const float* points, long long n, const float* frame_host, long long* keys, void* stream) {
  Frame f;
  if (n < 0 || (n > 0 && (!points || !keys)) || !read_frame(frame_host, f)) return CDS_EINVAL;
  if (n == 0) return 0;
  hipLaunchKernelGGL(grid_keys_kernel, dim3(grid_blocks(n)), dim3(256), 0, (hipStream_t)stream, points, n, f, keys);
  return cds_launch_status();
}

extern "C" int cds_grid_hash_build(const long long* keys, long long n_keys, long long n_fine, long long* table_keys,
                                   int* table_vals, int log2_slots, void* stream) {
  if (n_keys < 0 || n_fine < 0 || n_fine > n_keys || !table_keys || !table_vals || (n_keys > 0 && !keys) ||
      log2_slots < 1 || log2_slots > 40 || (1ll << log2_slots) < 2 * n_keys)
    return CDS_EINVAL;
  const long long slots = 1ll << log2_slots;
  hipLaunchKernelGGL(hash_clear_kernel, dim3(grid_blocks(slots)), dim3(256), 0, (hipStream_t)stream,
                     (unsigned long long*)table_keys, slots);
  if (n_keys > 0)
    hipLaunchKernelGGL(hash_insert_kernel, dim3(grid_blocks(n_keys)), dim3(256), 0, (hipStream_t)stream, keys, n_keys, n_fine,
                       (unsigned long long*)table_keys, table_vals, (unsigned long long)(slots - 1));
  return cds_launch_status();
}

extern "C" int cds_nn_query_f32(const float* query, const long long* order, long long m, const float* pts,
                                const int* cell_start, const long long* cell_keys, const int* coarse_start,
                                const long long* table_keys, const int* table_vals, int log2_slots, const float* frame_host,
                                float max_dist, float* dist, void* stream) {
  Frame f;
  if (m < 0 || !read_frame(frame_host, f) || !(max_dist >= 0.0f) || log2_slots < 1 || log2_slots > 40) return CDS_EINVAL;
  if (m == 0) return 0;
  if (!query || !pts || !cell_start || !cell_keys || !coarse_start || !table_keys || !table_vals || !dist) return CDS_EINVAL;
  const Table t{(const unsigned long long*)table_keys, table_vals, (1ull << log2_slots) - 1};
  hipLaunchKernelGGL(nn_query_kernel, dim3(grid_blocks(m)), dim3(256), 0, (hipStream_t)stream, query, order, m,
                     (const float4*)pts, cell_start, (const unsigned long long*)cell_keys, coarse_start, t, f, max_dist, dist);
  return cds_launch_status();
}

extern "C" int cds_thin_round_f32(const float* pts, const int* cell_start, long long n, const long long* table_keys,
                                  const int* table_vals, int log2_slots, const float* frame_host, float min_dist,
                                  unsigned char* state, int* undecided, void* stream) {
  Frame f;
  if (n < 0 || !read_frame(frame_host, f) || !(min_dist > 0.0f) || f.h < min_dist || log2_slots < 1 || log2_slots > 40)
    return CDS_EINVAL;
  if (n == 0) return 0;
  if (!pts || !cell_start || !table_keys || !table_vals || !state) return CDS_EINVAL;
  const Table t{(const unsigned long long*)table_keys, table_vals, (1ull << log2_slots) - 1};
  hipLaunchKernelGGL(thin_round_kernel, dim3(grid_blocks(n)), dim3(256), 0, (hipStream_t)stream, (const float4*)pts, cell_start,
                     n, t, f, min_dist * min_dist, state, undecided);
  return cds_launch_status();
}
