// Filling the small holes of a triangle mesh with centroid fans (the rule is stated in include/cds_mvsnet_hip.h):
// the input's rows stay bit for bit, one vertex and n faces are added per hole of 4 .. max_edges border edges, one face per hole
// of 3.  The sort of the edge keys, the list of the regular vertices, the prefix sums over the loop counts and the copies of the
// input's rows are the caller's (torch).
//
//   cds_mesh_fill_keys     one thread per face: one key per half-edge, (min << 31 | max) << 1 | direction; the sentinel for an
//                          invalid face
//   cds_mesh_fill_borders  one thread per sorted key: a run of one undirected key of length 1 is a border half-edge a -> b; it
//                          adds 1 to out[a] and in[b] (integer atomicAdd) and writes next[a] = b and prev[b] = a
//   cds_mesh_fill_init     one thread per vertex: regular iff out == 1 and in == 1; next = prev = -1 elsewhere; the start of the
//                          doubling
//   cds_mesh_fill_double   one thread per regular vertex: label = min(label, label[jump]), jump = jump[jump], from one pair of
//                          arrays into another (Jacobi, so a round reads nothing that it writes), along next and along prev
//   cds_mesh_fill_walk     one thread per regular vertex; the ones that are the minimum of both of their windows of the doubling
//                          walk `next` for at most max_edges steps: the edge count, the centre and its colour of a loop that closes
//   cds_mesh_fill_emit     one thread per regular vertex; the leader of a filled loop walks it again and writes its vertex and
//                          its faces at its offsets
//
// Every decision is taken on integers.  The atomics are integer adds, whose sums do not depend on the order; next[a] is written
// by several threads only where out[a] > 1, and is read only where out[a] == 1 (prev[b] and in[b] likewise).  The one
// floating-point sum is one thread's serial fp64 chain in loop order.  The walk is serial per leader, which is why max_edges ends
// at CDS_MESH_FILL_MAX_EDGES.
#include "mesh_common.hpp"

namespace {

using namespace cds_mesh;

constexpr long long kNoEdge = 0x7fffffffffffffffLL;                     // above every key: min < max < 2^31 gives less than 2^63 - 1
constexpr int kPoison = -1;                                              // the label of a vertex that is not regular: below every vertex

__device__ __forceinline__ bool inside(int v, long long n_vertices) {
  return (unsigned long long)(long long)v < (unsigned long long)n_vertices;
}

__global__ __launch_bounds__(kThreads) void keys_kernel(const int* __restrict__ faces, long long n_faces, long long n_vertices,
                                                        long long* __restrict__ keys) {
  const long long face = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (face >= n_faces) return;
  int idx[3];
  const bool ok = load_face(faces, face, n_vertices, idx) && idx[0] != idx[1] && idx[1] != idx[2] && idx[2] != idx[0];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int a = idx[k], b = idx[(k + 1) % 3];
    const long long lo = a < b ? a : b, hi = a < b ? b : a;
    keys[3 * face + k] = ok ? ((((lo << 31) | hi) << 1) | (a < b ? 0 : 1)) : kNoEdge;
  }
}

__global__ __launch_bounds__(kThreads) void borders_kernel(const long long* __restrict__ keys, long long n_keys, long long n_vertices,
                                                           int* __restrict__ out, int* __restrict__ in, int* __restrict__ next,
                                                           int* __restrict__ prev) {
  const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n_keys) return;
  const long long key = keys[i];
  if (key == kNoEdge || key < 0) return;
  const long long edge = key >> 1;
  if (i > 0 && (keys[i - 1] >> 1) == edge) return;
  if (i + 1 < n_keys && (keys[i + 1] >> 1) == edge) return;
  const int lo = (int)(edge >> 31), hi = (int)(edge & 0x7fffffffLL);
  if (!inside(lo, n_vertices) || !inside(hi, n_vertices) || lo == hi) return;
  const int a = (key & 1) ? hi : lo, b = (key & 1) ? lo : hi;
  atomicAdd(&out[a], 1);
  atomicAdd(&in[b], 1);
  next[a] = b;
  prev[b] = a;
}

// label and jump hold two chains, [2][V]: row 0 along next, row 1 along prev.
__global__ __launch_bounds__(kThreads) void init_kernel(long long n_vertices, const int* __restrict__ out, const int* __restrict__ in,
                                                        int* __restrict__ next, int* __restrict__ prev,
                                                        unsigned char* __restrict__ regular, int* __restrict__ label_a,
                                                        int* __restrict__ jump_a, int* __restrict__ label_b, int* __restrict__ jump_b) {
  const long long v = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (v >= n_vertices) return;
  const bool reg = out[v] == 1 && in[v] == 1 && inside(next[v], n_vertices) && inside(prev[v], n_vertices);
  regular[v] = reg ? 1 : 0;
  if (!reg) next[v] = prev[v] = -1;
  const int label = reg ? (int)v : kPoison;
  label_a[v] = label_b[v] = label_a[n_vertices + v] = label_b[n_vertices + v] = label;
  jump_a[v] = jump_b[v] = reg ? next[v] : (int)v;
  jump_a[n_vertices + v] = jump_b[n_vertices + v] = reg ? prev[v] : (int)v;
}

__global__ __launch_bounds__(kThreads) void double_kernel(const int* __restrict__ list, long long n_list, long long n_vertices,
                                                          const int* __restrict__ label_in, const int* __restrict__ jump_in,
                                                          int* __restrict__ label_out, int* __restrict__ jump_out) {
  const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n_list) return;
  const int v = list[i];
  if (!inside(v, n_vertices)) return;
#pragma unroll
  for (int dir = 0; dir < 2; ++dir) {
    const long long row = dir * n_vertices;
    const int j = jump_in[row + v];
    if (!inside(j, n_vertices)) {                                        // never from cds_mesh_fill_init: poison, and stay
      label_out[row + v] = kPoison;
      jump_out[row + v] = v;
      continue;
    }
    const int mine = label_in[row + v], theirs = label_in[row + j];
    label_out[row + v] = theirs < mine ? theirs : mine;
    jump_out[row + v] = jump_in[row + j];
  }
}

// The loop of v0, walked for at most max_edges edges -> its edge count, 0 unless it closes having met only regular vertices
// larger than v0.  Visit: what is done at every vertex of the loop, v0 first.
template <typename Visit>
__device__ __forceinline__ int walk(int v0, const int* __restrict__ next, const unsigned char* __restrict__ regular,
                                    long long n_vertices, int max_edges, Visit visit) {
  int v = v0, n = 0;
  do {
    if (n == max_edges || !inside(v, n_vertices) || !regular[v] || v < v0) return 0;
    visit(v, n);
    ++n;
    v = next[v];
  } while (v != v0);
  return n >= 3 ? n : 0;
}

__global__ __launch_bounds__(kThreads) void walk_kernel(const float* __restrict__ vertices, const unsigned char* __restrict__ colors,
                                                        long long n_vertices, const int* __restrict__ next,
                                                        const unsigned char* __restrict__ regular, const int* __restrict__ label,
                                                        const int* __restrict__ list, long long n_list, int max_edges,
                                                        int* __restrict__ edges, unsigned* __restrict__ centre,
                                                        unsigned char* __restrict__ centre_color) {
  const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n_list) return;
  const int v0 = list[i];
  double sum[3] = {0.0, 0.0, 0.0};
  int csum[3] = {0, 0, 0};
  int n = 0;
  if (inside(v0, n_vertices) && label[v0] == v0 && label[n_vertices + v0] == v0) {
    n = walk(v0, next, regular, n_vertices, max_edges, [&](int v, int) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        sum[c] += (double)vertices[3 * (long long)v + c];
        csum[c] += colors[3 * (long long)v + c];
      }
    });
  }
  edges[i] = n;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const double mean = sum[c] / (double)(n > 0 ? n : 1);
    centre[3 * i + c] = mean != mean ? 0x7fc00000u : __float_as_uint((float)mean);   // one NaN for every sum that is none
    centre_color[3 * i + c] = n > 0 ? (unsigned char)((2 * csum[c] + n) / (2 * n)) : 0;
  }
}

__global__ __launch_bounds__(kThreads) void emit_kernel(const int* __restrict__ next, const unsigned char* __restrict__ regular,
                                                        long long n_vertices, long long n_faces, const int* __restrict__ list,
                                                        long long n_list, int max_edges, const int* __restrict__ edges,
                                                        const long long* __restrict__ vertex_at, const long long* __restrict__ face_at,
                                                        const unsigned* __restrict__ centre, const unsigned char* __restrict__ centre_color,
                                                        long long new_vertices, long long new_faces, unsigned* __restrict__ vertices_out,
                                                        unsigned char* __restrict__ colors_out, int* __restrict__ faces_out) {
  const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n_list) return;
  const int n = edges[i], v0 = list[i];
  if (n < 3 || n > max_edges) return;
  const long long fat = face_at[i], vat = vertex_at[i];
  const int n_new = n == 3 ? 1 : n;
  if (fat < 0 || fat + n_new > new_faces) return;                        // offsets that are no prefix sums: write nothing
  int* f = faces_out + 3 * (n_faces + fat);
  if (n == 3) {
    int v[3] = {v0, v0, v0};
    if (walk(v0, next, regular, n_vertices, 3, [&](int x, int k) { v[k] = x; }) != 3) return;
    f[0] = v[0];
    f[1] = v[2];
    f[2] = v[1];
    return;
  }
  if (vat < 0 || vat >= new_vertices) return;
  const long long c = n_vertices + vat;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    vertices_out[3 * c + k] = centre[3 * i + k];
    colors_out[3 * c + k] = centre_color[3 * i + k];
  }
  walk(v0, next, regular, n_vertices, n, [&](int x, int k) {              // the face of the border half-edge x -> next[x], backwards
    f[3 * k] = next[x];
    f[3 * k + 1] = x;
    f[3 * k + 2] = (int)c;
  });
}

inline bool keys_ok(long long n_faces) { return 3 * n_faces <= 0x7fffffffLL; }
inline bool edges_ok(int max_edges) { return max_edges >= 3 && max_edges <= CDS_MESH_FILL_MAX_EDGES; }

}  // namespace

extern "C" int cds_mesh_fill_max_edges(void) { return CDS_MESH_FILL_MAX_EDGES; }

extern "C" int cds_mesh_fill_keys(const int* faces, long long n_faces, long long n_vertices, long long* keys, void* stream) {
  if (!sizes_ok(n_vertices, n_faces) || !keys_ok(n_faces)) return CDS_EINVAL;
  if (n_faces == 0) return 0;
  if (!faces || !keys) return CDS_EINVAL;
  hipLaunchKernelGGL(keys_kernel, dim3(blocks_for(n_faces)), dim3(kThreads), 0, (hipStream_t)stream, faces, n_faces, n_vertices, keys);
  return cds_launch_status();
}

extern "C" int cds_mesh_fill_borders(const long long* keys, long long n_keys, long long n_vertices, int* out, int* in, int* next,
                                     int* prev, void* stream) {
  if (!sizes_ok(n_vertices, n_keys)) return CDS_EINVAL;
  if (n_keys == 0 || n_vertices == 0) return 0;
  if (!keys || !out || !in || !next || !prev) return CDS_EINVAL;
  hipLaunchKernelGGL(borders_kernel, dim3(blocks_for(n_keys)), dim3(kThreads), 0, (hipStream_t)stream, keys, n_keys, n_vertices, out,
                     in, next, prev);
  return cds_launch_status();
}

extern "C" int cds_mesh_fill_init(long long n_vertices, const int* out, const int* in, int* next, int* prev, unsigned char* regular,
                                  int* label_a, int* jump_a, int* label_b, int* jump_b, void* stream) {
  if (!sizes_ok(n_vertices, 0)) return CDS_EINVAL;
  if (n_vertices == 0) return 0;
  if (!out || !in || !next || !prev || !regular || !label_a || !jump_a || !label_b || !jump_b || label_a == label_b || jump_a == jump_b)
    return CDS_EINVAL;
  hipLaunchKernelGGL(init_kernel, dim3(blocks_for(n_vertices)), dim3(kThreads), 0, (hipStream_t)stream, n_vertices, out, in, next,
                     prev, regular, label_a, jump_a, label_b, jump_b);
  return cds_launch_status();
}

extern "C" int cds_mesh_fill_double(const int* list, long long n_list, long long n_vertices, const int* label_in, const int* jump_in,
                                    int* label_out, int* jump_out, void* stream) {
  if (!sizes_ok(n_vertices, n_list) || n_list > n_vertices) return CDS_EINVAL;
  if (n_list == 0) return 0;
  if (!list || !label_in || !jump_in || !label_out || !jump_out || label_in == label_out || jump_in == jump_out) return CDS_EINVAL;
  hipLaunchKernelGGL(double_kernel, dim3(blocks_for(n_list)), dim3(kThreads), 0, (hipStream_t)stream, list, n_list, n_vertices,
                     label_in, jump_in, label_out, jump_out);
  return cds_launch_status();
}

extern "C" int cds_mesh_fill_walk(const float* vertices, const unsigned char* colors, long long n_vertices, const int* next,
                                  const unsigned char* regular, const int* label, const int* list, long long n_list, int max_edges,
                                  int* edges, float* centre, unsigned char* centre_color, void* stream) {
  if (!sizes_ok(n_vertices, n_list) || n_list > n_vertices || !edges_ok(max_edges)) return CDS_EINVAL;
  if (n_list == 0) return 0;
  if (!vertices || !colors || !next || !regular || !label || !list || !edges || !centre || !centre_color) return CDS_EINVAL;
  hipLaunchKernelGGL(walk_kernel, dim3(blocks_for(n_list)), dim3(kThreads), 0, (hipStream_t)stream, vertices, colors, n_vertices, next,
                     regular, label, list, n_list, max_edges, edges, reinterpret_cast<unsigned*>(centre), centre_color);
  return cds_launch_status();
}

extern "C" int cds_mesh_fill_emit(const int* next, const unsigned char* regular, long long n_vertices, long long n_faces,
                                  const int* list, long long n_list, int max_edges, const int* edges, const long long* vertex_at,
                                  const long long* face_at, const float* centre, const unsigned char* centre_color,
                                  long long new_vertices, long long new_faces, float* vertices_out, unsigned char* colors_out,
                                  int* faces_out, void* stream) {
  if (!sizes_ok(n_vertices, n_faces) || !sizes_ok(n_list, 0) || n_list > n_vertices || !edges_ok(max_edges) || new_vertices < 0 ||
      new_faces < 0 || !sizes_ok(n_vertices + new_vertices, n_faces + new_faces))
    return CDS_EINVAL;
  if (n_list == 0 || new_faces == 0) return 0;
  if (!next || !regular || !list || !edges || !vertex_at || !face_at || !centre || !centre_color || !faces_out ||
      (new_vertices > 0 && (!vertices_out || !colors_out)))
    return CDS_EINVAL;
  hipLaunchKernelGGL(emit_kernel, dim3(blocks_for(n_list)), dim3(kThreads), 0, (hipStream_t)stream, next, regular, n_vertices, n_faces,
                     list, n_list, max_edges, edges, vertex_at, face_at, reinterpret_cast<const unsigned*>(centre), centre_color,
                     new_vertices, new_faces, reinterpret_cast<unsigned*>(vertices_out), colors_out, faces_out);
  return cds_launch_status();
}
