// Taubin lambda|mu smoothing of a triangle mesh (the rule is stated in include/cds_mvsnet_hip.h): the vertex
// positions move, nothing else does.  The prefix sum over the counts, the sort of the few long segments and the reduction of the
// statistics are the caller's (torch).
//
//   cds_mesh_adj_count        one thread per face: the entries each of its vertices will receive (integer atomicAdd)
//   cds_mesh_adj_fill         one thread per face: the other end of every edge slot into the segment of each end, at an integer
//                             cursor per vertex
//   cds_mesh_adj_finish       one thread per vertex, the owner of its segment: sort (segments of at most CDS_MESH_ADJ_SMALL entries;
//                             the caller sorted the longer ones), multiplicities off the runs, flags, dedupe in place, rule 3, deg
//   cds_mesh_smooth_step_f32  one thread per vertex: one Jacobi step with a factor, from `in` to `out`
//   cds_mesh_smooth_limit_f32 one thread per vertex: the squared move, and the clamp of rule 6
//
// Nothing here depends on an order the hardware chooses: the atomics are on integers and only decide where inside a segment an
// entry lands, and the segment is then sorted and made a set; the sum of a vertex is one thread's serial fp64 chain in ascending
// neighbour order; every other word is written once.  No float atomics.  The library is built with -ffp-contract=off, so every
// fp64 product and sum below is rounded as written.
#include "mesh_common.hpp"

namespace {

using namespace cds_mesh;

constexpr int kGather = 8;                                               // neighbours whose loads are in flight together

// The slot k of a face is the edge (idx[k], idx[(k + 1) % 3]); a slot whose two corners are equal is dropped (rule 1).
__global__ __launch_bounds__(kThreads) void adj_count_kernel(const int* __restrict__ faces, long long n_faces, long long n_vertices,
                                                             int* __restrict__ count) {
  const long long face = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (face >= n_faces) return;
  int idx[3];
  if (!load_face(faces, face, n_vertices, idx)) return;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int a = idx[k], b = idx[(k + 1) % 3];
    if (a == b) continue;
    atomicAdd(&count[a], 1);
    atomicAdd(&count[b], 1);
  }
}

__device__ __forceinline__ void put(int owner, int other, const int* __restrict__ start, int* __restrict__ cursor,
                                    int* __restrict__ nbr, long long n_entries) {
  const long long at = (long long)start[owner] + atomicAdd(&cursor[owner], 1);
  if (at >= 0 && at < (long long)start[owner + 1] && at < n_entries) nbr[at] = other;   // a segment never grows past its count
}

__global__ __launch_bounds__(kThreads) void adj_fill_kernel(const int* __restrict__ faces, long long n_faces, long long n_vertices,
                                                            const int* __restrict__ start, int* __restrict__ cursor,
                                                            int* __restrict__ nbr, long long n_entries) {
  const long long face = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (face >= n_faces) return;
  int idx[3];
  if (!load_face(faces, face, n_vertices, idx)) return;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int a = idx[k], b = idx[(k + 1) % 3];
    if (a == b) continue;
    put(a, b, start, cursor, nbr, n_entries);
    put(b, a, start, cursor, nbr, n_entries);
  }
}

// The multiplicity of the edge {v, j} is the number of times j stands in v's segment.  flags: bit 0 boundary, bit 1 isolated.
__global__ __launch_bounds__(kThreads) void adj_finish_kernel(long long n_vertices, const int* __restrict__ start, int* __restrict__ nbr,
                                                              long long n_entries, int* __restrict__ deg,
                                                              unsigned char* __restrict__ flags) {
  const long long v = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (v >= n_vertices) return;
  const long long s = start[v], e = start[v + 1];
  if (s < 0 || e < s || e > n_entries) {                                 // offsets outside the array: touch nothing
    deg[v] = 0;
    flags[v] = CDS_MESH_ADJ_ISOLATED;
    return;
  }
  int* seg = nbr + s;
  const int len = (int)(e - s);
  if (len <= CDS_MESH_ADJ_SMALL) {                                       // insertion sort; the longer segments arrive sorted
    for (int i = 1; i < len; ++i) {
      const int x = seg[i];
      int k = i - 1;
      while (k >= 0 && seg[k] > x) {
        seg[k + 1] = seg[k];
        --k;
      }
      seg[k + 1] = x;
    }
  }
  bool boundary = false;
  for (int i = 0; i < len;) {                                            // a run of length 1 is a boundary edge
    int r = i + 1;
    while (r < len && seg[r] == seg[i]) ++r;
    boundary = boundary || r - i == 1;
    i = r;
  }
  int d = 0;
  for (int i = 0; i < len;) {                                            // the write index never passes the read index
    int r = i + 1;
    const int x = seg[i];
    while (r < len && seg[r] == x) ++r;
    if (!boundary || r - i == 1) seg[d++] = x;                           // rule 3
    i = r;
  }
  deg[v] = d;
  flags[v] = (unsigned char)((boundary ? CDS_MESH_ADJ_BOUNDARY : 0) | (d == 0 ? CDS_MESH_ADJ_ISOLATED : 0));
}

// The indices of a batch are loaded before its positions, so that kGather gathers of a lane are in flight behind one wait; the
// sum itself is sequential, in ascending neighbour order.  A vertex without neighbours, or one whose segment or neighbours lie
// outside the arrays, copies its bits.
__global__ __launch_bounds__(kThreads) void step_kernel(const float* __restrict__ in, float* __restrict__ out, long long n_vertices,
                                                        const int* __restrict__ start, const int* __restrict__ deg,
                                                        const int* __restrict__ nbr, double factor) {
  const long long v = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (v >= n_vertices) return;
  const long long s = start[v];
  const int d = deg[v];
  bool ok = d > 0 && s >= 0 && s + d <= (long long)start[v + 1];
  double sx = 0.0, sy = 0.0, sz = 0.0;
  for (int k0 = 0; ok && k0 < d; k0 += kGather) {
    int j[kGather];
#pragma unroll
    for (int u = 0; u < kGather; ++u) j[u] = k0 + u < d ? nbr[s + k0 + u] : (int)v;
    float x[kGather], y[kGather], z[kGather];
#pragma unroll
    for (int u = 0; u < kGather; ++u) {
      const bool inside = (unsigned long long)(long long)j[u] < (unsigned long long)n_vertices;
      ok = ok && inside;
      const long long at = inside ? j[u] : v;
      x[u] = in[3 * at];
      y[u] = in[3 * at + 1];
      z[u] = in[3 * at + 2];
    }
#pragma unroll
    for (int u = 0; u < kGather; ++u) {
      if (k0 + u < d) {
        sx += (double)x[u];
        sy += (double)y[u];
        sz += (double)z[u];
      }
    }
  }
  if (!ok) {
    const unsigned* src = reinterpret_cast<const unsigned*>(in);
    unsigned* dst = reinterpret_cast<unsigned*>(out);
#pragma unroll
    for (int c = 0; c < 3; ++c) dst[3 * v + c] = src[3 * v + c];
    return;
  }
  const double k = (double)d;
  const double px = (double)in[3 * v], py = (double)in[3 * v + 1], pz = (double)in[3 * v + 2];
  const double mx = sx / k, my = sy / k, mz = sz / k;
  out[3 * v] = (float)(px + factor * (mx - px));
  out[3 * v + 1] = (float)(py + factor * (my - py));
  out[3 * v + 2] = (float)(pz + factor * (mz - pz));
}

__global__ __launch_bounds__(kThreads) void limit_kernel(const float* __restrict__ original, float* __restrict__ vertices,
                                                         long long n_vertices, double max_move, double* __restrict__ move2_out,
                                                         unsigned char* __restrict__ clamped_out) {
  const long long v = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (v >= n_vertices) return;
  const double ox = (double)original[3 * v], oy = (double)original[3 * v + 1], oz = (double)original[3 * v + 2];
  const double dx = (double)vertices[3 * v] - ox, dy = (double)vertices[3 * v + 1] - oy, dz = (double)vertices[3 * v + 2] - oz;
  const double n2 = (dx * dx + dy * dy) + dz * dz;
  move2_out[v] = n2;
  const bool clamp = max_move > 0.0 && n2 > max_move * max_move;
  if (clamp) {
    const double scale = max_move / sqrt(n2);
    vertices[3 * v] = (float)(ox + dx * scale);
    vertices[3 * v + 1] = (float)(oy + dy * scale);
    vertices[3 * v + 2] = (float)(oz + dz * scale);
  }
  clamped_out[v] = clamp ? 1 : 0;
}

// 3 n_faces slots, two entries each, addressed by an int32.
inline bool entries_ok(long long n_faces) { return 6 * n_faces <= 0x7fffffffLL; }

}  // namespace

extern "C" int cds_mesh_adj_small(void) { return CDS_MESH_ADJ_SMALL; }

extern "C" int cds_mesh_adj_count(const int* faces, long long n_faces, long long n_vertices, int* count, void* stream) {
  if (!sizes_ok(n_vertices, n_faces) || !entries_ok(n_faces)) return CDS_EINVAL;
  if (n_faces == 0 || n_vertices == 0) return 0;
  if (!faces || !count) return CDS_EINVAL;
  hipLaunchKernelGGL(adj_count_kernel, dim3(blocks_for(n_faces)), dim3(kThreads), 0, (hipStream_t)stream, faces, n_faces, n_vertices,
                     count);
  return cds_launch_status();
}

extern "C" int cds_mesh_adj_fill(const int* faces, long long n_faces, long long n_vertices, const int* start, int* cursor, int* nbr,
                                 long long n_entries, void* stream) {
  if (!sizes_ok(n_vertices, n_faces) || !entries_ok(n_faces) || n_entries < 0 || n_entries > 6 * n_faces) return CDS_EINVAL;
  if (n_faces == 0 || n_vertices == 0 || n_entries == 0) return 0;
  if (!faces || !start || !cursor || !nbr) return CDS_EINVAL;
  hipLaunchKernelGGL(adj_fill_kernel, dim3(blocks_for(n_faces)), dim3(kThreads), 0, (hipStream_t)stream, faces, n_faces, n_vertices,
                     start, cursor, nbr, n_entries);
  return cds_launch_status();
}

extern "C" int cds_mesh_adj_finish(long long n_vertices, const int* start, int* nbr, long long n_entries, int* deg,
                                   unsigned char* flags, void* stream) {
  if (!sizes_ok(n_vertices, n_entries)) return CDS_EINVAL;
  if (n_vertices == 0) return 0;
  if (!start || !deg || !flags || (n_entries > 0 && !nbr)) return CDS_EINVAL;
  hipLaunchKernelGGL(adj_finish_kernel, dim3(blocks_for(n_vertices)), dim3(kThreads), 0, (hipStream_t)stream, n_vertices, start, nbr,
                     n_entries, deg, flags);
  return cds_launch_status();
}

extern "C" int cds_mesh_smooth_step_f32(const float* in, float* out, long long n_vertices, const int* start, const int* deg,
                                        const int* nbr, double factor, void* stream) {
  if (!sizes_ok(n_vertices, 0) || !(factor >= -kHuge && factor <= kHuge)) return CDS_EINVAL;
  if (n_vertices == 0) return 0;
  if (!in || !out || in == out || !start || !deg || !nbr) return CDS_EINVAL;
  hipLaunchKernelGGL(step_kernel, dim3(blocks_for(n_vertices)), dim3(kThreads), 0, (hipStream_t)stream, in, out, n_vertices, start,
                     deg, nbr, factor);
  return cds_launch_status();
}

extern "C" int cds_mesh_smooth_limit_f32(const float* original, float* vertices, long long n_vertices, double max_move,
                                         double* move2_out, unsigned char* clamped_out, void* stream) {
  if (!sizes_ok(n_vertices, 0) || !(max_move >= 0.0 && max_move <= kHuge)) return CDS_EINVAL;
  if (n_vertices == 0) return 0;
  if (!original || !vertices || original == vertices || !move2_out || !clamped_out) return CDS_EINVAL;
  hipLaunchKernelGGL(limit_kernel, dim3(blocks_for(n_vertices)), dim3(kThreads), 0, (hipStream_t)stream, original, vertices,
                     n_vertices, max_move, move2_out, clamped_out);
  return cds_launch_status();
}
