// Connected components of a triangle mesh and the removal of the small ones (the rule is stated in
// include/cds_mvsnet_hip.h): labels, face counts and the compacted mesh, as a function of the integer input alone.
//
//   cds_mesh_cc_init     one thread per vertex: parent[v] = v
//   cds_mesh_cc_hook     one thread per face: the roots of its three vertices, the larger roots hooked under the smallest
//   cds_mesh_cc_jump     one thread per vertex: parent[v] = the root of v
//   cds_mesh_cc_count    one wave per 1024 faces: count[label of a face's first vertex] += 1, aggregated inside the wave first
//   cds_mesh_cc_mark     one thread per face: the keep flag of the face, and of its three vertices when it is kept
//   cds_mesh_cc_gather   one thread per vertex and per face: the kept rows at their new places, the faces renumbered
// The last one is cds_mesh_compact_dispatch (mesh_common.hpp), defined here: the same kernel, with packed colours, is
// cds_mesh_simplify_gather.  The face loader and the launch shape are those of mesh_common.hpp.
//
// The union-find keeps parent[x] <= x at every moment: init writes x, hook only lowers a word (atomicMin) and jump replaces
// a word by an ancestor of its vertex, which is not larger.  Three things follow.
//   Every walk along parent ends: the index strictly decreases until it meets a word that holds its own index, so a walk from x
//   takes at most x steps whatever other workgroups write meanwhile.  No loop of this file waits for another thread.
//   A vertex is only ever linked to a vertex of its own component (the two roots hook reads lie under two vertices of one face),
//   so the trees always refine the components; and the root of a tree is its smallest vertex.
//   The host repeats hook and jump until a hook pass lowers nothing.  In such a pass parent did not change, so every root it read
//   was a root, and every face saw its three vertices under one root: the trees are the components, and after the jump that
//   follows parent[v] is the smallest vertex of v's component, whatever order the memory operations of the earlier passes landed in.
// What a race can cost.  Inside hook, parent is read only through agent-scope relaxed atomic loads (and written only by
// atomicMin), so a read returns a value the word really held, if not the latest.  An older value is a valid, larger ancestor: the
// walk gets longer or ends on a vertex that has just stopped being a root.  atomicMin on such a vertex r either lowers nothing
// (the link is found again in the next pass, and whoever lowered parent[r] raised `changed`, so there is a next pass), or moves
// r's subtree from its parent m to the smaller root; the face that tied r to m is still in the list and ties the two trees again
// in the next pass, and this thread raised `changed`.  Either way the cost is a pass, never a wrong label.
#include "mesh_common.hpp"

namespace {

using namespace cds_mesh;

__device__ __forceinline__ int load_parent(const int* parent, long long x) {
  return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The root above x.  p < x on every step (a word that does not hold a smaller index ends the walk), so at most x steps.
__device__ __forceinline__ int find_root(const int* parent, int x) {
  for (;;) {
    const int p = load_parent(parent, x);
    if (p >= x || p < 0) return x;
    x = p;
  }
}

__global__ __launch_bounds__(kThreads) void cc_init_kernel(int* __restrict__ parent, long long n_vertices) {
  const long long v = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (v < n_vertices) parent[v] = (int)v;
}

__global__ __launch_bounds__(kThreads) void cc_hook_kernel(const int* __restrict__ faces, long long n_faces, long long n_vertices,
                                                           int* parent, int* changed) {
  const long long face = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (face >= n_faces) return;
  int idx[3];
  if (!load_face(faces, face, n_vertices, idx)) return;
  const int ra = find_root(parent, idx[0]), rb = find_root(parent, idx[1]), rc = find_root(parent, idx[2]);
  const int lo = min(ra, min(rb, rc));
  bool lowered = false;
  if (ra != lo) lowered = atomicMin(parent + ra, lo) > lo || lowered;
  if (rb != lo && rb != ra) lowered = atomicMin(parent + rb, lo) > lo || lowered;
  if (rc != lo && rc != ra && rc != rb) lowered = atomicMin(parent + rc, lo) > lo || lowered;
  if (lowered) *changed = 1;
}

// Roots do not change in this kernel, and a word another thread has already replaced holds an ancestor too: every walk ends on
// the root the tree had when the kernel started.
__global__ __launch_bounds__(kThreads) void cc_jump_kernel(int* parent, long long n_vertices) {
  const long long v = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (v >= n_vertices) return;
  const int p = load_parent(parent, v);
  if (p >= v || p < 0) return;
  const int r = find_root(parent, p);
  if (r != p) __hip_atomic_store(parent + v, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// One atomic per distinct label of a wave instead of one per face: the lanes that share the first pending lane's label are
// balloted, that lane adds their number, and the loop goes on with the rest.  Every turn retires its leader: at most 64 turns.
// A wave takes kCountChunks runs of 64 consecutive faces and keeps the sum of the first label it meets, the surface's in
// nearly every wave, in a register until the end: one add to that address per 1024 faces (profiles/mesh_components.md: with
// one add per 64 faces the 656 k adds to the surface's counter alone took 7.4 ms of a 42 M-face scan).
constexpr int kCountChunks = 16;

__global__ __launch_bounds__(kThreads) void cc_count_kernel(const int* __restrict__ faces, long long n_faces, long long n_vertices,
                                                            const int* __restrict__ label, int* __restrict__ count) {
  const int lane = threadIdx.x & (CDS_WAVE - 1);
  const long long wave = (long long)blockIdx.x * (kThreads / CDS_WAVE) + (threadIdx.x / CDS_WAVE);
  const long long first = wave * (CDS_WAVE * kCountChunks);
  int held = -1, held_n = 0;                                             // the same in every lane
  for (int chunk = 0; chunk < kCountChunks; ++chunk) {
    const long long face = first + (long long)chunk * CDS_WAVE + lane;
    int idx[3];
    bool active = face < n_faces;
    if (active) active = load_face(faces, face, n_vertices, idx);
    int mine = active ? label[idx[0]] : -1;
    if ((unsigned long long)(long long)mine >= (unsigned long long)n_vertices) { active = false; mine = -1; }
    unsigned long long todo = __ballot(active);
    for (int turn = 0; turn < CDS_WAVE && todo; ++turn) {
      const int leader = __ffsll((long long)todo) - 1;
      const int lead = __shfl(mine, leader);
      const unsigned long long same = __ballot(active && mine == lead) & todo;
      const int n = (int)__popcll(same);
      if (held < 0) held = lead;
      if (lead == held) held_n += n;
      else if (lane == leader) atomicAdd(count + lead, n);
      todo &= ~same;
    }
  }
  if (held_n > 0 && lane == 0) atomicAdd(count + held, held_n);
}

__global__ __launch_bounds__(kThreads) void cc_mark_kernel(const int* __restrict__ faces, long long n_faces, long long n_vertices,
                                                           const int* __restrict__ label, const unsigned char* __restrict__ keep,
                                                           unsigned char* __restrict__ face_keep, unsigned char* vertex_keep) {
  const long long face = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (face >= n_faces) return;
  int idx[3];
  bool kept = load_face(faces, face, n_vertices, idx);
  if (kept) {
    const int c = label[idx[0]];
    kept = (unsigned long long)(long long)c < (unsigned long long)n_vertices && keep[c] != 0;
  }
  face_keep[face] = kept ? 1 : 0;
  if (kept) { vertex_keep[idx[0]] = 1; vertex_keep[idx[1]] = 1; vertex_keep[idx[2]] = 1; }   // every writer stores the same byte
}

// Items 0 .. n_vertices - 1 are vertices, the rest faces.  *_new: the exclusive prefix sums of the keep flags.  Color: unsigned
// char for three bytes per row, unsigned for the packed word of cds_voxel_merge_f32.
template <typename Color>
__global__ __launch_bounds__(kThreads) void compact_kernel(const unsigned* __restrict__ vertices, const Color* __restrict__ colors,
                                                           const int* __restrict__ faces, long long n_vertices, long long n_faces,
                                                           const unsigned char* __restrict__ vertex_keep,
                                                           const int* __restrict__ vertex_new,
                                                           const unsigned char* __restrict__ face_keep,
                                                           const int* __restrict__ face_new, long long out_vertices,
                                                           long long out_faces, unsigned* __restrict__ vertices_out,
                                                           unsigned char* __restrict__ colors_out, int* __restrict__ faces_out) {
  const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (i < n_vertices) {
    if (!vertex_keep[i]) return;
    const long long j = vertex_new[i];
    if (j < 0 || j >= out_vertices) return;
#pragma unroll
    for (int k = 0; k < 3; ++k) vertices_out[3 * j + k] = vertices[3 * i + k];       // the bits, not the value
    if (!colors) return;
    if constexpr (sizeof(Color) == 1) {
#pragma unroll
      for (int k = 0; k < 3; ++k) colors_out[3 * j + k] = colors[3 * i + k];
    } else {
      const unsigned w = colors[i];
#pragma unroll
      for (int k = 0; k < 3; ++k) colors_out[3 * j + k] = (unsigned char)((w >> (8 * k)) & 255u);
    }
    return;
  }
  const long long face = i - n_vertices;
  if (face >= n_faces || !face_keep[face]) return;
  const long long j = face_new[face];
  int idx[3];
  if (j < 0 || j >= out_faces || !load_face(faces, face, n_vertices, idx)) return;
#pragma unroll
  for (int k = 0; k < 3; ++k) faces_out[3 * j + k] = vertex_new[idx[k]];
}

}  // namespace

extern "C" int cds_mesh_cc_init(int* parent, long long n_vertices, void* stream) {
  if (!sizes_ok(n_vertices, 0)) return CDS_EINVAL;
  if (n_vertices == 0) return 0;
  if (!parent) return CDS_EINVAL;
  hipLaunchKernelGGL(cc_init_kernel, dim3(blocks_for(n_vertices)), dim3(kThreads), 0, (hipStream_t)stream, parent, n_vertices);
  return cds_launch_status();
}

extern "C" int cds_mesh_cc_hook(const int* faces, long long n_faces, long long n_vertices, int* parent, int* changed,
                                void* stream) {
  if (!sizes_ok(n_vertices, n_faces)) return CDS_EINVAL;
  if (n_faces == 0 || n_vertices == 0) return 0;
  if (!faces || !parent || !changed) return CDS_EINVAL;
  hipLaunchKernelGGL(cc_hook_kernel, dim3(blocks_for(n_faces)), dim3(kThreads), 0, (hipStream_t)stream, faces, n_faces, n_vertices,
                     parent, changed);
  return cds_launch_status();
}

extern "C" int cds_mesh_cc_jump(int* parent, long long n_vertices, void* stream) {
  if (!sizes_ok(n_vertices, 0)) return CDS_EINVAL;
  if (n_vertices == 0) return 0;
  if (!parent) return CDS_EINVAL;
  hipLaunchKernelGGL(cc_jump_kernel, dim3(blocks_for(n_vertices)), dim3(kThreads), 0, (hipStream_t)stream, parent, n_vertices);
  return cds_launch_status();
}

extern "C" int cds_mesh_cc_count(const int* faces, long long n_faces, long long n_vertices, const int* label, int* count,
                                 void* stream) {
  if (!sizes_ok(n_vertices, n_faces)) return CDS_EINVAL;
  if (n_faces == 0 || n_vertices == 0) return 0;
  if (!faces || !label || !count) return CDS_EINVAL;
  const unsigned blocks = blocks_for((n_faces + kCountChunks - 1) / kCountChunks);      // a block takes kThreads kCountChunks faces
  hipLaunchKernelGGL(cc_count_kernel, dim3(blocks), dim3(kThreads), 0, (hipStream_t)stream, faces, n_faces, n_vertices, label,
                     count);
  return cds_launch_status();
}

extern "C" int cds_mesh_cc_mark(const int* faces, long long n_faces, long long n_vertices, const int* label,
                                const unsigned char* keep, unsigned char* face_keep, unsigned char* vertex_keep, void* stream) {
  if (!sizes_ok(n_vertices, n_faces)) return CDS_EINVAL;
  if (n_faces == 0 || n_vertices == 0) return 0;
  if (!faces || !label || !keep || !face_keep || !vertex_keep) return CDS_EINVAL;
  hipLaunchKernelGGL(cc_mark_kernel, dim3(blocks_for(n_faces)), dim3(kThreads), 0, (hipStream_t)stream, faces, n_faces, n_vertices,
                     label, keep, face_keep, vertex_keep);
  return cds_launch_status();
}

int cds_mesh_compact_dispatch(const float* vertices, const void* colors, bool packed, const int* faces, long long n_vertices,
                              long long n_faces, const unsigned char* vertex_keep, const int* vertex_new,
                              const unsigned char* face_keep, const int* face_new, long long out_vertices, long long out_faces,
                              float* vertices_out, unsigned char* colors_out, int* faces_out, void* stream) {
  if (!sizes_ok(n_vertices, n_faces) || !sizes_ok(out_vertices, out_faces) || out_vertices > n_vertices || out_faces > n_faces)
    return CDS_EINVAL;
  if (out_vertices == 0) return 0;                                       // no kept vertex: no kept face either
  if (!vertices || !vertex_keep || !vertex_new || !vertices_out || (colors && !colors_out)) return CDS_EINVAL;
  if (out_faces > 0 && (!faces || !face_keep || !face_new || !faces_out)) return CDS_EINVAL;
  if (out_faces == 0) n_faces = 0;                                       // vertex items only
  const auto launch = [&](auto kernel, auto* typed_colors) {
    hipLaunchKernelGGL(kernel, dim3(blocks_for(n_vertices + n_faces)), dim3(kThreads), 0, (hipStream_t)stream,
                       reinterpret_cast<const unsigned*>(vertices), typed_colors, faces, n_vertices, n_faces, vertex_keep, vertex_new,
                       face_keep, face_new, out_vertices, out_faces, reinterpret_cast<unsigned*>(vertices_out), colors_out, faces_out);
  };
  if (packed) launch(compact_kernel<unsigned>, static_cast<const unsigned*>(colors));
  else launch(compact_kernel<unsigned char>, static_cast<const unsigned char*>(colors));
  return cds_launch_status();
}

extern "C" int cds_mesh_cc_gather(const float* vertices, const unsigned char* colors, const int* faces, long long n_vertices,
                                  long long n_faces, const unsigned char* vertex_keep, const int* vertex_new,
                                  const unsigned char* face_keep, const int* face_new, long long out_vertices, long long out_faces,
                                  float* vertices_out, unsigned char* colors_out, int* faces_out, void* stream) {
  return cds_mesh_compact_dispatch(vertices, colors, false, faces, n_vertices, n_faces, vertex_keep, vertex_new, face_keep, face_new,
                                   out_vertices, out_faces, vertices_out, colors_out, faces_out, stream);
}
