// Surface samples of a triangle mesh (the rule is stated in include/cds_mvsnet_hip.h): every face is cut into n^2
// congruent sub-triangles by its barycentric lattice, n the smallest count that makes the longest edge of a sub-triangle <= spacing,
// and the centroid of every sub-triangle becomes a point with an interpolated colour and the face's index.  The prefix sum of the
// counts between the two kernels is the caller's (torch).
//
//   cds_mesh_sample_count   one thread per face: n (rule 1) and n^2
//   cds_mesh_sample_emit    one thread per four consecutive samples of a run: rule 2, in the order of rule 3
//
// Nothing here depends on an order the hardware chooses: every output word is written once, by the thread its index names.  No
// atomics.  The only floating-point decision is rule 1's test; the enumeration and the weights are integers.  The library is built
// with -ffp-contract=off, so every fp64 product, sum and quotient below is rounded as written.  The face loader, the finiteness
// test and the launch shape are those of mesh_common.hpp.
#include "mesh_common.hpp"

namespace {

using namespace cds_mesh;

constexpr int kPerThread = 4;                                            // consecutive samples of one thread: 16-byte stores
constexpr int kRun = kThreads * kPerThread;                              // consecutive samples of one pass of a workgroup
constexpr int kRunsPerBlock = 8;                                         // consecutive runs of one workgroup
constexpr int kMaxN = CDS_MESH_SAMPLE_MAX_N;

__device__ __forceinline__ double edge2(const double a[3], const double b[3]) {
  const double dx = a[0] - b[0], dy = a[1] - b[1], dz = a[2] - b[2];
  return (dx * dx + dy * dy) + dz * dz;
}

// Rule 1's test: n sub-edges of length spacing span the longest edge.
__device__ __forceinline__ bool spans(int n, double spacing, double l2) {
  const double s = (double)n * spacing;
  return s * s >= l2;
}

__global__ __launch_bounds__(kThreads) void count_kernel(const float* __restrict__ vertices, long long n_vertices,
                                                         const int* __restrict__ faces, long long n_faces, double spacing,
                                                         int* __restrict__ out_n, long long* __restrict__ out_n2) {
  const long long face = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (face >= n_faces) return;
  int idx[3], n = 0;
  if (load_face(faces, face, n_vertices, idx)) {
    double p[3][3];
    bool finite = true;
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        p[k][c] = (double)vertices[3 * (long long)idx[k] + c];
        finite = finite && is_finite(p[k][c]);
      }
    if (finite) {
      const double l2 = fmax(fmax(edge2(p[1], p[0]), edge2(p[2], p[1])), edge2(p[0], p[2]));
      const double guess = ceil(sqrt(l2) / spacing);                     // a start only: the two loops decide
      n = guess >= (double)(kMaxN + 1) ? kMaxN + 1 : (guess >= 1.0 ? (int)guess : 1);
      while (n > 1 && spans(n - 1, spacing, l2)) --n;
      while (n <= kMaxN && !spans(n, spacing, l2)) ++n;                   // stops at kMaxN + 1: the host sees the overflow
    }
  }
  out_n[face] = n;
  out_n2[face] = (long long)n * n;
}

// The last face in [lo, hi] whose offset is <= idx.  Faces without samples repeat the offset of the next face that has some, so
// the last of a run of equal offsets is the owner.  Reads offsets[lo .. hi] only.
__device__ __forceinline__ long long owner(const long long* __restrict__ offsets, long long lo, long long hi, long long idx) {
  while (lo < hi) {
    const long long mid = lo + (hi - lo + 1) / 2;
    if (offsets[mid] <= idx) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// The same for a face that is near lo (the next run of a workgroup starts where the last one ended): doubling steps from lo, then
// the search between the last two probes.  offsets[lo] <= idx is the caller's.
__device__ __forceinline__ long long owner_near(const long long* __restrict__ offsets, long long lo, long long hi, long long idx) {
  long long step = 1;
  while (lo + step <= hi && offsets[lo + step] <= idx) {
    lo += step;
    step *= 2;
  }
  return owner(offsets, lo, lo + step - 1 < hi ? lo + step - 1 : hi, idx);
}

struct Sample {
  float x, y, z;
  unsigned color;                                                        // r | g << 8 | b << 16
};

struct Corners {
  double p[3][3];
  int col[3][3];
};

// The corners of a face; false, and nothing read beyond the indices, for a face with an index outside the vertices.
__device__ __forceinline__ bool load_corners(const float* __restrict__ vertices, const unsigned char* __restrict__ colors,
                                             long long n_vertices, const int* __restrict__ faces, long long face, Corners& t) {
  int vi[3];
  if (!load_face(faces, face, n_vertices, vi)) return false;
#pragma unroll
  for (int k = 0; k < 3; ++k)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      t.p[k][c] = (double)vertices[3 * (long long)vi[k] + c];
      t.col[k][c] = (int)colors[3 * (long long)vi[k] + c];
    }
  return true;
}

// Sample k of a face with subdivision n (rule 2); the caller has checked 1 <= n <= kMaxN and 0 <= k < n n.
__device__ __forceinline__ Sample sample_of(const Corners& t, int n, int k) {
  // floor(sqrt(k)): k < 2^30 and r <= 2^15, so the fp32 guess is off by far less than 1 and one step each way makes it exact
  int r = (int)sqrtf((float)k);
  r -= (r * r > k) ? 1 : 0;
  r += ((r + 1) * (r + 1) <= k) ? 1 : 0;
  const int c = k - r * r, j = c >> 1;
  const int pp = (c & 1) ? 3 * r + 1 : 3 * r + 2, q = (c & 1) ? 3 * j + 2 : 3 * j + 1;
  const int wa = 3 * n - pp, wb = pp - q, wc = q;
  const double da = (double)wa, db = (double)wb, dc = (double)wc, d3n = (double)(3 * n);
  Sample s;
  s.x = (float)(((da * t.p[0][0] + db * t.p[1][0]) + dc * t.p[2][0]) / d3n);
  s.y = (float)(((da * t.p[0][1] + db * t.p[1][1]) + dc * t.p[2][1]) / d3n);
  s.z = (float)(((da * t.p[0][2] + db * t.p[1][2]) + dc * t.p[2][2]) / d3n);
  // (2 sum + 3 n) / (6 n) in integers: num < 2^26 and the quotient <= 255, so the fp32 guess is off by at most 1 and one step
  // each way makes it the integer quotient
  const int den = 6 * n;
  const float inv = 1.0f / (float)den;
  s.color = 0;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    const int num = 2 * (wa * t.col[0][ch] + wb * t.col[1][ch] + wc * t.col[2][ch]) + 3 * n;
    int v = (int)((float)num * inv);
    v -= (v * den > num) ? 1 : 0;
    v += ((v + 1) * den <= num) ? 1 : 0;
    s.color |= (unsigned)(v & 255) << (8 * ch);
  }
  return s;
}

// A workgroup owns kRunsPerBlock consecutive runs of kRun samples; thread t of it the kPerThread samples from run0 + t kPerThread
// of every run.  It finds the faces of a run's first and last sample by a search in the offsets, the first run's over all faces,
// the later ones' from where the run before ended (both the same in every thread: scalar loads).  A thread then names the face
// and the k of each of its samples (integers only) and computes them: from one load of the corners when all are of one face,
// else face by face.  A full group of kPerThread is stored as 16-byte (points, faces) and 4-byte (colours) words: 4 i samples
// start at byte 48 i, 12 i, 16 i of arrays the caller allocated, so the stores are aligned; the last, partial group of the output
// goes out sample by sample.
__device__ __forceinline__ void emit_run(const float* __restrict__ vertices, const unsigned char* __restrict__ colors,
                                         long long n_vertices, const int* __restrict__ faces, const int* __restrict__ n_of,
                                         const long long* __restrict__ offsets, long long n_points, long long run0, long long f_lo,
                                         long long f_hi, float* __restrict__ out_points, unsigned char* __restrict__ out_colors,
                                         int* __restrict__ out_face) {
  const long long first = run0 + (long long)threadIdx.x * kPerThread;
  if (first >= n_points) return;
  const int count = first + kPerThread <= n_points ? kPerThread : (int)(n_points - first);

  int fid[kPerThread], kk[kPerThread], nn[kPerThread];                   // nn 0: not a sample to write
  {
    long long f = -1, f_begin = 0, f_end = 0;                            // the face in hand and its samples [f_begin, f_end)
    int n = 0;
#pragma unroll
    for (int i = 0; i < kPerThread; ++i) {
      fid[i] = -1;
      kk[i] = nn[i] = 0;
      if (i >= count) continue;
      const long long idx = first + i;
      if (f < 0 || idx >= f_end) {                                       // another face: find it inside the run's faces
        if (f >= 0 && f + 1 <= f_hi && offsets[f + 1] <= idx && (f + 1 == f_hi || offsets[f + 2] > idx))
          f = f + 1;                                                     // runs of small faces: the next one, without a search
        else
          f = owner(offsets, f < 0 ? f_lo : f, f_hi, idx);
        f_begin = offsets[f];
        n = n_of[f];
        if (n < 1 || n > kMaxN) n = 0;
        f_end = f_begin + (long long)n * n;
      }
      if (idx < f_begin || idx >= f_end) continue;                       // offsets that do not fit the counts: write nothing
      fid[i] = (int)f;
      kk[i] = (int)(idx - f_begin);
      nn[i] = n;
    }
  }

  float pts[3 * kPerThread];
  unsigned col_word[kPerThread];
  bool valid[kPerThread];
#pragma unroll
  for (int i = 0; i < kPerThread; ++i) {
    valid[i] = false;
    pts[3 * i] = pts[3 * i + 1] = pts[3 * i + 2] = 0.f;
    col_word[i] = 0;
  }
  bool one_face = count == kPerThread && fid[0] == fid[kPerThread - 1];  // the faces ascend: the ones between are the same
#pragma unroll
  for (int i = 0; i < kPerThread; ++i) one_face = one_face && nn[i] > 0;
  if (one_face) {
    Corners t;
    if (load_corners(vertices, colors, n_vertices, faces, fid[0], t)) {
#pragma unroll
      for (int i = 0; i < kPerThread; ++i) {
        const Sample s = sample_of(t, nn[0], kk[i]);
        pts[3 * i] = s.x; pts[3 * i + 1] = s.y; pts[3 * i + 2] = s.z;
        col_word[i] = s.color;
        valid[i] = true;
      }
    }
  } else {
#pragma unroll
    for (int i = 0; i < kPerThread; ++i) {
      Corners t;
      if (nn[i] == 0 || !load_corners(vertices, colors, n_vertices, faces, fid[i], t)) continue;
      const Sample s = sample_of(t, nn[i], kk[i]);
      pts[3 * i] = s.x; pts[3 * i + 1] = s.y; pts[3 * i + 2] = s.z;
      col_word[i] = s.color;
      valid[i] = true;
    }
  }

  bool all = count == kPerThread;
#pragma unroll
  for (int i = 0; i < kPerThread; ++i) all = all && valid[i];
  if (all) {
    static_assert(kPerThread == 4, "the packing below is written for four samples");
    const long long g = first / kPerThread;
    cds_f4* po = reinterpret_cast<cds_f4*>(out_points) + 3 * g;
#pragma unroll
    for (int v = 0; v < 3; ++v) po[v] = cds_f4{pts[4 * v], pts[4 * v + 1], pts[4 * v + 2], pts[4 * v + 3]};
    unsigned* co = reinterpret_cast<unsigned*>(out_colors) + 3 * g;     // twelve bytes r g b r g b ... as three words
    co[0] = col_word[0] | (col_word[1] << 24);
    co[1] = (col_word[1] >> 8) | (col_word[2] << 16);
    co[2] = (col_word[2] >> 16) | (col_word[3] << 8);
    using cds_i4 = int __attribute__((ext_vector_type(4)));
    reinterpret_cast<cds_i4*>(out_face)[g] = cds_i4{fid[0], fid[1], fid[2], fid[3]};
    return;
  }
#pragma unroll
  for (int i = 0; i < kPerThread; ++i) {
    if (!valid[i]) continue;
    const long long idx = first + i;
    out_points[3 * idx] = pts[3 * i];
    out_points[3 * idx + 1] = pts[3 * i + 1];
    out_points[3 * idx + 2] = pts[3 * i + 2];
    out_colors[3 * idx] = (unsigned char)(col_word[i] & 255u);
    out_colors[3 * idx + 1] = (unsigned char)((col_word[i] >> 8) & 255u);
    out_colors[3 * idx + 2] = (unsigned char)((col_word[i] >> 16) & 255u);
    out_face[idx] = fid[i];
  }
}

__global__ __launch_bounds__(kThreads) void emit_kernel(const float* __restrict__ vertices, const unsigned char* __restrict__ colors,
                                                        long long n_vertices, const int* __restrict__ faces, long long n_faces,
                                                        const int* __restrict__ n_of, const long long* __restrict__ offsets,
                                                        long long n_points, float* __restrict__ out_points,
                                                        unsigned char* __restrict__ out_colors, int* __restrict__ out_face) {
  long long run0 = (long long)blockIdx.x * kRunsPerBlock * kRun, f_hi = 0;
  for (int r = 0; r < kRunsPerBlock && run0 < n_points; ++r, run0 += kRun) {
    const long long run1 = (run0 + kRun < n_points ? run0 + kRun : n_points) - 1;             // the run's last sample
    const long long f_lo = r == 0 ? owner(offsets, 0, n_faces - 1, run0) : owner_near(offsets, f_hi, n_faces - 1, run0);
    f_hi = owner_near(offsets, f_lo, n_faces - 1, run1);
    emit_run(vertices, colors, n_vertices, faces, n_of, offsets, n_points, run0, f_lo, f_hi, out_points, out_colors, out_face);
  }
}

}  // namespace

extern "C" int cds_mesh_sample_max_n(void) { return kMaxN; }

extern "C" int cds_mesh_sample_count(const float* vertices, long long n_vertices, const int* faces, long long n_faces,
                                     double spacing, int* out_n, long long* out_n2, void* stream) {
  if (!sizes_ok(n_vertices, n_faces) || !finite_pos(spacing)) return CDS_EINVAL;
  if (n_faces == 0) return 0;
  if (!faces || !out_n || !out_n2 || (n_vertices > 0 && !vertices)) return CDS_EINVAL;
  hipLaunchKernelGGL(count_kernel, dim3(blocks_for(n_faces)), dim3(kThreads), 0, (hipStream_t)stream, vertices, n_vertices, faces,
                     n_faces, spacing, out_n, out_n2);
  return cds_launch_status();
}

extern "C" int cds_mesh_sample_emit(const float* vertices, const unsigned char* colors, long long n_vertices, const int* faces,
                                    long long n_faces, const int* n, const long long* offsets, long long n_points,
                                    float* out_points, unsigned char* out_colors, int* out_face, void* stream) {
  if (!sizes_ok(n_vertices, n_faces) || n_points < 0 || n_points > 0x7fffffffLL) return CDS_EINVAL;
  if (n_faces == 0 || n_points == 0) return 0;
  if (!vertices || !colors || !faces || !n || !offsets || !out_points || !out_colors || !out_face) return CDS_EINVAL;
  // the 16-byte stores of a full group of four samples
  if ((reinterpret_cast<uintptr_t>(out_points) & 15u) || (reinterpret_cast<uintptr_t>(out_colors) & 15u) ||
      (reinterpret_cast<uintptr_t>(out_face) & 15u))
    return CDS_EINVAL;
  const long long per_block = (long long)kRunsPerBlock * kRun;
  hipLaunchKernelGGL(emit_kernel, dim3((unsigned)((n_points + per_block - 1) / per_block)), dim3(kThreads), 0, (hipStream_t)stream,
                     vertices, colors, n_vertices, faces, n_faces, n, offsets, n_points, out_points, out_colors, out_face);
  return cds_launch_status();
}
