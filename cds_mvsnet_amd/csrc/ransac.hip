// RANSAC over point correspondences for a similarity transform, the trajectory alignment of the Tanks and Temples protocol
// (cds_mvsnet_amd/tt_eval.py):
//
//   cds_ransac_similarity_f64   H hypotheses of k correspondences each, every one scored over all N, the best one returned
//
// One hypothesis per lane, 256-thread workgroups, all arithmetic in float64 (ransac_common.hpp holds what a lane computes).
// The N points are not staged in LDS: in the score loop every lane of a wave reads the same point, so the loads are scalar-cache
// loads that cost no vector memory instruction and no barrier, for any N.  A first kernel writes one best record per workgroup,
// a second (one workgroup) reduces them.  "Best" is a total order (larger count, then smaller err2, then smaller h), so the
// result does not depend on the shape of either reduction and two runs return identical bytes.
#include "cds_common.hpp"
#include "ransac_common.hpp"

namespace {

constexpr int REC = CDS_RANSAC_RECORD;   // h, count, err2, T[12]

// does (c1, e1, h1) come before (c2, e2, h2)?
__device__ __forceinline__ bool ransac_better(int c1, double e1, long long h1, int c2, double e2, long long h2) {
  return c1 > c2 || (c1 == c2 && (e1 < e2 || (e1 == e2 && h1 < h2)));
}

// The best (count, err2, h) of the workgroup's 256 candidates, valid in every thread.  h is unique per thread.
__device__ __forceinline__ void ransac_block_best(int& c, double& e, long long& h, int* sc, double* se, long long* sh) {
  const int t = threadIdx.x;
  sc[t] = c;
  se[t] = e;
  sh[t] = h;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (t < s && ransac_better(sc[t + s], se[t + s], sh[t + s], sc[t], se[t], sh[t])) {
      sc[t] = sc[t + s];
      se[t] = se[t + s];
      sh[t] = sh[t + s];
    }
    __syncthreads();
  }
  c = sc[0];
  e = se[0];
  h = sh[0];
}

// Pass 1.  Lane = hypothesis h; lanes past H take count -1 and lose against everything.  Record [g][15] of workgroup g: its best
// hypothesis (h as a double: H < 2^31), written by the lane that owns it.
template <int K>
__global__ __launch_bounds__(256) void ransac_hypotheses_kernel(const double* __restrict__ src, const double* __restrict__ dst,
                                                                long long n, long long H, double thr2, unsigned long long seed,
                                                                double* __restrict__ rec, int* __restrict__ all_count,
                                                                double* __restrict__ all_err2) {
  __shared__ int sc[256];
  __shared__ double se[256];
  __shared__ long long sh[256];
  const long long h = (long long)blockIdx.x * 256 + threadIdx.x;
  int count = -1;
  double err2 = INFINITY;
  double T[12];
#ifdef CDS_RANSAC_STAGE_LDS
  // A/B variant (scripts/build_variant.sh ldsstage -DCDS_RANSAC_STAGE_LDS; profiles/tt_trajectory.md): the same arithmetic with
  // the points staged in LDS, 256 at a time, instead of read through the scalar cache.  Every lane takes part in the barriers.
  constexpr int TILE = 256;
  __shared__ double tile[6 * TILE];
  bool ok = h < H && n >= K;
  if (ok) {
    long long draw[K];
    cds_ransac::sample<K>(seed, (unsigned long long)h, n, draw);
    ok = cds_ransac::estimate<K>(src, dst, draw, T);
  }
  int inl = 0;
  double sum = 0.0;
  for (long long base = 0; base < n; base += TILE) {
    const int m = (int)(n - base < TILE ? n - base : TILE);
    __syncthreads();
    for (int i = threadIdx.x; i < 3 * m; i += 256) {
      tile[i] = src[3 * base + i];
      tile[3 * TILE + i] = dst[3 * base + i];
    }
    __syncthreads();
    if (ok) {
      int c = 0;
      double e = 0.0;
      cds_ransac::score(tile, tile + 3 * TILE, m, T, thr2, c, e);      // a sum per tile: err2 may differ in its last bits for n > 256
      inl += c;
      sum += e;
    }
  }
  if (h < H) {
    count = ok ? inl : 0;
    err2 = ok ? sum : INFINITY;
    if (!ok)
      for (int i = 0; i < 12; ++i) T[i] = (i % 5 == 0) ? 1.0 : 0.0;
    if (all_count) all_count[h] = count;
    if (all_err2) all_err2[h] = err2;
  }
#else
  if (h < H) {
    cds_ransac::hypothesis<K>(src, dst, n, thr2, seed, (unsigned long long)h, count, err2, T);
    if (all_count) all_count[h] = count;
    if (all_err2) all_err2[h] = err2;
  }
#endif
  int bc = count;
  double be = err2;
  long long bh = h;
  ransac_block_best(bc, be, bh, sc, se, sh);
  if (bh == h) {                               // block 0 .. gridDim.x - 1 each hold at least one h < H, so the winner has a T
    double* __restrict__ r = rec + (size_t)blockIdx.x * REC;
    r[0] = (double)h;
    r[1] = (double)count;
    r[2] = err2;
#pragma unroll
    for (int i = 0; i < 12; ++i) r[3 + i] = T[i];
  }
}

// Pass 2.  One workgroup picks the best of the `groups` records -> out [15].  No record, or a best one that was rejected
// (err2 = +inf): h = -1, count 0, err2 +inf and the identity.
__global__ __launch_bounds__(256) void ransac_reduce_kernel(const double* __restrict__ rec, int groups, double* __restrict__ out) {
  __shared__ int sc[256];
  __shared__ double se[256];
  __shared__ long long sh[256];
  int c = -1, best = -1;
  double e = INFINITY;
  long long h = 0x7fffffffffffffffLL - 255 + threadIdx.x;      // distinct per thread, after every real h
  for (int i = threadIdx.x; i < groups; i += 256) {
    const double* r = rec + (size_t)i * REC;
    if (ransac_better((int)r[1], r[2], (long long)r[0], c, e, h)) {
      h = (long long)r[0];
      c = (int)r[1];
      e = r[2];
      best = i;
    }
  }
  const long long mine = h;
  ransac_block_best(c, e, h, sc, se, sh);
  if (mine != h) return;
  if (best < 0 || !(e < INFINITY)) {
    out[0] = -1.0;
    out[1] = 0.0;
    out[2] = INFINITY;
    for (int i = 0; i < 12; ++i) out[3 + i] = (i % 5 == 0) ? 1.0 : 0.0;
  } else {
    for (int i = 0; i < REC; ++i) out[i] = rec[(size_t)best * REC + i];
  }
}

template <int K>
void ransac_launch(int groups, hipStream_t st, const double* src, const double* dst, long long n, long long H, double thr2,
                   unsigned long long seed, double* ws, int* count, double* err2) {
  hipLaunchKernelGGL(ransac_hypotheses_kernel<K>, dim3(groups), dim3(256), 0, st, src, dst, n, H, thr2, seed, ws, count, err2);
}

}  // namespace

extern "C" int cds_ransac_similarity_f64(const double* src, const double* dst, long long n, long long hypotheses, int k,
                                         double threshold, unsigned long long seed, double* ws, long long ws_doubles, double* out,
                                         int* count, double* err2, void* stream) {
  if (n < 0 || n > 0x7fffffffLL || hypotheses < 0 || hypotheses > 0x7fffffffLL || k < CDS_RANSAC_MIN_SAMPLE ||
      k > CDS_RANSAC_MAX_SAMPLE || !(threshold >= 0.0) || !(threshold < INFINITY) || !out || (n > 0 && (!src || !dst)))
    return CDS_EINVAL;
  const int groups = (int)((hypotheses + 255) / 256);
  if (groups > 0 && (!ws || (long long)groups * REC > ws_doubles)) return CDS_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const double thr2 = threshold * threshold;
  if (groups > 0) {
    switch (k) {
      case 3: ransac_launch<3>(groups, st, src, dst, n, hypotheses, thr2, seed, ws, count, err2); break;
      case 4: ransac_launch<4>(groups, st, src, dst, n, hypotheses, thr2, seed, ws, count, err2); break;
      case 5: ransac_launch<5>(groups, st, src, dst, n, hypotheses, thr2, seed, ws, count, err2); break;
      case 6: ransac_launch<6>(groups, st, src, dst, n, hypotheses, thr2, seed, ws, count, err2); break;
      case 7: ransac_launch<7>(groups, st, src, dst, n, hypotheses, thr2, seed, ws, count, err2); break;
      default: ransac_launch<8>(groups, st, src, dst, n, hypotheses, thr2, seed, ws, count, err2); break;
    }
  }
  hipLaunchKernelGGL(ransac_reduce_kernel, dim3(1), dim3(256), 0, st, ws, groups, out);
  return cds_launch_status();
}
