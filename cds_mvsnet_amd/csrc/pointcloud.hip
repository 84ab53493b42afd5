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
// The grid helpers, the neighbour walk (grid_walk, here with the NearestDist sink) and the check of the grid arguments live in
// grid_common.hpp; registration.hip and cloud_outlier.hip share them.
#include "grid_common.hpp"

namespace {

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
                                                       long long m, GridView g, float cap, float* __restrict__ dist) {
  const float cap2 = cap * cap;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (long long)gridDim.x * blockDim.x) {
    const long long qi = order ? order[i] : i;
    NearestDist s{cap2};
    grid_walk(g, query[3 * qi], query[3 * qi + 1], query[3 * qi + 2], s);
    dist[qi] = s.d2 < cap2 ? fminf(sqrtf(s.d2), cap) : cap;
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
  if (m == 0) return 0;                  // an empty query needs no grid: the pointers are not looked at
  GridView g;
  if (!query || !dist || !grid_view(pts, cell_start, cell_keys, coarse_start, table_keys, table_vals, log2_slots, frame_host, g))
    return CDS_EINVAL;
  hipLaunchKernelGGL(nn_query_kernel, dim3(grid_blocks(m)), dim3(256), 0, (hipStream_t)stream, query, order, m, g, max_dist, dist);
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
