// One RANSAC hypothesis of cds_ransac_similarity_f64 (ransac.hip; DESIGN.md 1.6, "Trajectory alignment"): the counter-based
// sample, the Umeyama similarity of the k pairs with an in-lane 3x3 SVD, and the score over all correspondences.  Plain C++
// in float64 with every product and sum written out (the library is built without contraction), callable from the host as
// well, so that a CPU build can step through exactly what a lane computes.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define CDS_HD __host__ __device__ __forceinline__
#else
#define CDS_HD inline
#endif

namespace cds_ransac {

constexpr double COLLINEAR_RATIO = 1e-9;      // a sample whose second singular value is <= this times the first is rejected

CDS_HD unsigned long long splitmix64(unsigned long long seed, unsigned long long c) {
  unsigned long long z = seed + (c + 1ull) * 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

CDS_HD unsigned long long mulhi64(unsigned long long a, unsigned long long b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __umul64hi(a, b);
#else
  return (unsigned long long)(((unsigned __int128)a * b) >> 64);
#endif
}

// K distinct indices of [0, n), n >= K, in draw order; hypothesis h depends on (seed, h) only.  Draw j takes
// r = floor(z (n - j) / 2^64) and steps over the earlier picks in ascending order: the r-th index not yet taken.
template <int K>
CDS_HD void sample(unsigned long long seed, unsigned long long h, long long n, long long draw[K]) {
  long long sorted[K];
#pragma unroll
  for (int j = 0; j < K; ++j) {
    long long r = (long long)mulhi64(splitmix64(seed, h * 8ull + (unsigned long long)j), (unsigned long long)(n - j));
#pragma unroll
    for (int i = 0; i < j; ++i)
      if (sorted[i] <= r) ++r;
    draw[j] = r;
    long long v = r;                           // insert: v carries the largest value met so far to the end
#pragma unroll
    for (int i = 0; i < j; ++i)
      if (sorted[i] > v) {
        const long long t = sorted[i];
        sorted[i] = v;
        v = t;
      }
    sorted[j] = v;
  }
}

// One-sided Jacobi step on columns p, q of G (and V): afterwards the two columns of G are orthogonal.  Returns whether it rotated.
CDS_HD bool jacobi_pair(double* gp, double* gq, double* vp, double* vq) {
  const double alpha = (gp[0] * gp[0] + gp[1] * gp[1]) + gp[2] * gp[2];
  const double beta = (gq[0] * gq[0] + gq[1] * gq[1]) + gq[2] * gq[2];
  const double gamma = (gp[0] * gq[0] + gp[1] * gq[1]) + gp[2] * gq[2];
  if (!(fabs(gamma) > 2.220446049250313e-16 * sqrt(alpha * beta))) return false;
  const double zeta = (beta - alpha) / (2.0 * gamma);
  const double t = (zeta < 0.0 ? -1.0 : 1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
  const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const double a = gp[r], b = gq[r];
    gp[r] = c * a - s * b;
    gq[r] = s * a + c * b;
    const double x = vp[r], y = vq[r];
    vp[r] = c * x - s * y;
    vq[r] = s * x + c * y;
  }
  return true;
}

CDS_HD void swap_columns(double* a, double* b) {
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const double t = a[r];
    a[r] = b[r];
    b[r] = t;
  }
}

CDS_HD bool is_finite(double x) { return x - x == 0.0; }

// Umeyama with scaling on the K pairs (p = src[draw[j]], q = dst[draw[j]]), sums in draw order -> T (rows of the 3x4).
// Returns false for a rejected hypothesis: variance of p zero, second singular value <= 1e-9 of the first, T not finite.
//
// The SVD of cov = U D V^T is a one-sided Jacobi iteration: G = cov V with V a product of plane rotations until the
// columns of G are orthogonal; then D = column norms (sorted descending) and U = G D^-1.  Only u1, u2 are divided out:
// with w = u1 x u2 the third left vector is +-w, and U E V^T with E = diag(1, 1, det(U) det(V)) is
// u1 v1^T + u2 v2^T + det(V) w v3^T whatever that sign, so a vanishing third singular value (three pairs, coplanar
// cameras) needs no special case; trace(D E) = d1 + d2 + det(V) (g3 . w).
template <int K>
CDS_HD bool estimate(const double* __restrict__ src, const double* __restrict__ dst, const long long draw[K], double T[12]) {
  double sp[3] = {0.0, 0.0, 0.0}, sq[3] = {0.0, 0.0, 0.0}, sqp[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, spp = 0.0;
#pragma unroll
  for (int j = 0; j < K; ++j) {
    const double p[3] = {src[3 * draw[j]], src[3 * draw[j] + 1], src[3 * draw[j] + 2]};
    const double q[3] = {dst[3 * draw[j]], dst[3 * draw[j] + 1], dst[3 * draw[j] + 2]};
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      sp[r] += p[r];
      sq[r] += q[r];
#pragma unroll
      for (int c = 0; c < 3; ++c) sqp[3 * r + c] += q[r] * p[c];
    }
    spp += (p[0] * p[0] + p[1] * p[1]) + p[2] * p[2];
  }
  const double n = (double)K;
  const double mp[3] = {sp[0] / n, sp[1] / n, sp[2] / n}, mq[3] = {sq[0] / n, sq[1] / n, sq[2] / n};
  const double var_p = spp / n - ((mp[0] * mp[0] + mp[1] * mp[1]) + mp[2] * mp[2]);
  double g[3][3], v[3][3];                     // [column][row]
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      g[c][r] = sqp[3 * r + c] / n - mq[r] * mp[c];
      v[c][r] = r == c ? 1.0 : 0.0;
    }
  for (int sweep = 0; sweep < 30; ++sweep) {   // converges quadratically: 4 to 6 sweeps in practice
    bool moved = jacobi_pair(g[0], g[1], v[0], v[1]);
    moved |= jacobi_pair(g[0], g[2], v[0], v[2]);
    moved |= jacobi_pair(g[1], g[2], v[1], v[2]);
    if (!moved) break;
  }
  double d[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) d[c] = sqrt((g[c][0] * g[c][0] + g[c][1] * g[c][1]) + g[c][2] * g[c][2]);
#define CDS_RANSAC_ORDER(a, b)        \
  if (d[a] < d[b]) {                  \
    const double t_ = d[a];           \
    d[a] = d[b];                      \
    d[b] = t_;                        \
    swap_columns(g[a], g[b]);         \
    swap_columns(v[a], v[b]);         \
  }
  CDS_RANSAC_ORDER(0, 1)
  CDS_RANSAC_ORDER(1, 2)
  CDS_RANSAC_ORDER(0, 1)
#undef CDS_RANSAC_ORDER
  if (!(var_p != 0.0) || !(d[1] > COLLINEAR_RATIO * d[0])) return false;
  const double u1[3] = {g[0][0] / d[0], g[0][1] / d[0], g[0][2] / d[0]};
  const double u2[3] = {g[1][0] / d[1], g[1][1] / d[1], g[1][2] / d[1]};
  const double w[3] = {u1[1] * u2[2] - u1[2] * u2[1], u1[2] * u2[0] - u1[0] * u2[2], u1[0] * u2[1] - u1[1] * u2[0]};
  const double det_v = (v[0][0] * (v[1][1] * v[2][2] - v[1][2] * v[2][1]) - v[0][1] * (v[1][0] * v[2][2] - v[1][2] * v[2][0])) +
                       v[0][2] * (v[1][0] * v[2][1] - v[1][1] * v[2][0]);
  const double e = det_v < 0.0 ? -1.0 : 1.0;
  const double scale = ((d[0] + d[1]) + e * ((g[2][0] * w[0] + g[2][1] * w[1]) + g[2][2] * w[2])) / var_p;
  bool ok = true;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    double R[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) R[c] = (u1[r] * v[0][c] + u2[r] * v[1][c]) + e * (w[r] * v[2][c]);
    T[4 * r] = scale * R[0];
    T[4 * r + 1] = scale * R[1];
    T[4 * r + 2] = scale * R[2];
    T[4 * r + 3] = mq[r] - scale * ((R[0] * mp[0] + R[1] * mp[1]) + R[2] * mp[2]);
#pragma unroll
    for (int c = 0; c < 4; ++c) ok = ok && is_finite(T[4 * r + c]);
  }
  return ok;
}

// count = #{i : |T src_i - dst_i|^2 < thr2}, err2 = the sum of those d2 in index order.  The addresses do not depend on the
// lane: on the device every lane of a wave reads the same point, through the scalar cache.
CDS_HD void score(const double* __restrict__ src, const double* __restrict__ dst, long long n, const double T[12], double thr2,
                  int& count, double& err2) {
  count = 0;
  err2 = 0.0;
  for (long long i = 0; i < n; ++i) {
    const double x = src[3 * i], y = src[3 * i + 1], z = src[3 * i + 2];
    const double dx = (((T[0] * x + T[1] * y) + T[2] * z) + T[3]) - dst[3 * i];
    const double dy = (((T[4] * x + T[5] * y) + T[6] * z) + T[7]) - dst[3 * i + 1];
    const double dz = (((T[8] * x + T[9] * y) + T[10] * z) + T[11]) - dst[3 * i + 2];
    const double d2 = (dx * dx + dy * dy) + dz * dz;
    if (d2 < thr2) {
      ++count;
      err2 += d2;
    }
  }
}

// The whole hypothesis h -> (count, err2, T); a rejected one (or n < K) gives count 0, err2 +inf and the identity.
template <int K>
CDS_HD void hypothesis(const double* __restrict__ src, const double* __restrict__ dst, long long n, double thr2,
                       unsigned long long seed, unsigned long long h, int& count, double& err2, double T[12]) {
  bool ok = n >= K;
  if (ok) {
    long long draw[K];
    sample<K>(seed, h, n, draw);
    ok = estimate<K>(src, dst, draw, T);
  }
  if (ok) {
    score(src, dst, n, T, thr2, count, err2);
  } else {
    count = 0;
    err2 = INFINITY;
#pragma unroll
    for (int i = 0; i < 12; ++i) T[i] = (i % 5 == 0) ? 1.0 : 0.0;
  }
}

}  // namespace cds_ransac
