// COLMAP sparse model -> MVSNet scene: the two float64 kernels of the converter (the reference's colmap2mvsnet.py scores
// every image pair in Python, colmap2mvsnet.py:279-293, and takes each image's depth range from its sparse points,
// colmap2mvsnet.py:357-373).  cds_mvsnet_amd/colmap.py drives these kernels; the rule is restated in float64 numpy in
// tests/colmap_ref.py.
//
//   colmap_pair_scores_kernel   S[i][j] for i < j: the sum over the points p that both images observe of
//                               c_i(p) w(theta_p), c_i(p) = how often image i (the lower index) observes p
//   colmap_obs_depth_kernel     z of every valid observation in its image's camera frame
//   colmap_depth_means_kernel   per image, from its z values in ascending order: the mean of the lowest num_min and of the
//                               highest num_max, each summed in ascending order by one lane
//
// Pair scores.  The observations arrive as a CSR over points: for point p the entries ptr[p] .. ptr[p + 1] - 1 hold the
// images that see it, ascending, each once, with its multiplicity cnt.  A track of length L yields L (L - 1) / 2 terms, and
// track lengths range from 2 to the number of images, so the work is balanced over TERMS: pair_off is the exclusive prefix
// sum of the per-point term counts, every lane takes kTermsPerLane consecutive terms, finds its first point with one binary
// search in pair_off and then walks (a, b), a < b, through the upper triangle of the track and on into the next tracks.
// The term of (p, a, b), with i = img[a] < j = img[b]:
//   u = c_i - x_p, v = c_j - x_p (camera centres c = -R^T t);  nothing if |u|^2 = 0 or |v|^2 = 0 (the point lies on a centre)
//   cosine = ((u.v) / sqrt(|u|^2)) / sqrt(|v|^2), clamped to [-1, 1];  theta = (180 / pi) acos(cosine)
//   w = exp(-((theta - theta0) (theta - theta0)) / (2 sigma^2)), sigma = sigma1 if theta <= theta0 else sigma2
// Every operation is a separately rounded double operation (-ffp-contract=off); dot products are ((x x + y y) + z z).
//
// Accumulation: multi-limb 64-bit fixed point, exact and free of any order.  w lies in (0, 1] but spans hundreds of binary
// orders (e^-153 = 2^-221 at theta = 180 degrees with the default parameters, less with a smaller sigma), and the selection
// needs the small end too: the reference ranks two images that share a point at any angle above two images that share
// nothing, and orders such pairs among themselves.  So a score is a number of `limbs` limbs of 40 bits, limb k in units of
// 2^-40(k+1), each limb an int64 of acc[k][i][j] with 23 bits of headroom.  The caller sizes `limbs` from theta0 and the
// sigmas so that the smallest weight the rule can produce still has its two leading limbs (cds_colmap_score_limbs: 7 at
// the defaults, at most 28, which covers every nonzero double; a weight that underflows to 0 in double adds nothing, as
// in the reference).  A term is split exactly (s = r 2^40, limb = floor(s), r = s - limb: all exact in double) and enters
// as its first nonzero limb and the one after it, times c_i, each with one integer global atomic add (a vector memory
// instruction): at least 40 significant bits, an absolute error below 2^-80 = q (CDS_COLMAP_SCORE_QUANTUM_LOG2) per
// occurrence.  Integer addition is associative, so every limb, and with it the matrix, is bit-identical from run to run
// whatever the order of arrival.  A limb may take 2^23 weighted terms before it could leave int64; the Python wrapper
// refuses a model in which an image has 2^22 or more valid observations.
// Shape of the atomics: a lane's consecutive terms share i and step through j; the lanes of a wave instruction sit 8 terms
// apart, so in a long track one instruction's adds fall 64 B apart in a row of the matrix, and in short tracks they
// scatter over the rows of neighbouring tracks (which, seen by the same window of cameras, often share a destination).
// Nothing is pre-summed; scripts/time_colmap.py reports the atomic bytes over the kernel time.
#include "cds_common.hpp"

namespace {

constexpr int kTermsPerLane = 8;
constexpr int kMaxLimbs = CDS_COLMAP_SCORE_MAX_LIMBS;
constexpr double kLimbScale = 1099511627776.0;    // 2^40: one limb

__device__ __forceinline__ long long row_start(long long a, long long L) { return a * (2 * L - a - 1) / 2; }

__global__ __launch_bounds__(256) void colmap_pair_scores_kernel(const long long* __restrict__ pair_off,
                                                                 const long long* __restrict__ ptr,
                                                                 const int* __restrict__ img, const int* __restrict__ cnt,
                                                                 const double* __restrict__ xyz,
                                                                 const double* __restrict__ centres, long long P,
                                                                 long long T, int N, double theta0, double sigma1,
                                                                 double sigma2, int limbs, unsigned long long* __restrict__ acc) {
  const long long t0 = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * kTermsPerLane;
  if (t0 >= T) return;
  // the point of term t0: the largest p with pair_off[p] <= t0 (points without a pair share their offset with the next)
  long long lo = 0, hi = P;                       // pair_off[lo] <= t0 < pair_off[hi] = T
  while (hi - lo > 1) {
    const long long mid = (lo + hi) >> 1;
    if (pair_off[mid] <= t0) lo = mid; else hi = mid;
  }
  long long p = lo;
  long long s = ptr[p], L = ptr[p + 1] - s;
  const long long k = t0 - pair_off[p];
  // (a, b) of the k-th entry of the strict upper triangle, rows first: closed form, then exact integer correction
  long long a = (long long)(((double)(2 * L - 1) - sqrt((double)((2 * L - 1) * (2 * L - 1) - 8 * k))) * 0.5);
  a = a < 0 ? 0 : (a > L - 2 ? L - 2 : a);
  while (row_start(a, L) > k) --a;
  while (a < L - 2 && row_start(a + 1, L) <= k) ++a;
  long long b = a + 1 + (k - row_start(a, L));
  const double inv2s1 = 2.0 * (sigma1 * sigma1), inv2s2 = 2.0 * (sigma2 * sigma2);
  const double deg = 180.0 / 3.141592653589793;
  double px = xyz[3 * p], py = xyz[3 * p + 1], pz = xyz[3 * p + 2];
  const long long tend = t0 + kTermsPerLane < T ? t0 + kTermsPerLane : T;
  for (long long t = t0; t < tend; ++t) {
    const int i = img[s + a], j = img[s + b];
    const double ux = centres[3 * i] - px, uy = centres[3 * i + 1] - py, uz = centres[3 * i + 2] - pz;
    const double vx = centres[3 * j] - px, vy = centres[3 * j + 1] - py, vz = centres[3 * j + 2] - pz;
    const double uu = (ux * ux + uy * uy) + uz * uz, vv = (vx * vx + vy * vy) + vz * vz;
    if (uu > 0.0 && vv > 0.0) {
      double c = (((ux * vx + uy * vy) + uz * vz) / sqrt(uu)) / sqrt(vv);
      c = c > 1.0 ? 1.0 : (c < -1.0 ? -1.0 : c);
      const double theta = deg * acos(c);
      const double d = theta - theta0;
      const double w = exp(-(d * d) / (theta <= theta0 ? inv2s1 : inv2s2));
      unsigned long long* dst = acc + (long long)i * N + j;
      const long long c_i = cnt[s + a];
      double r = w;
      for (int k = 0, emitted = 0; k < limbs && emitted < 2; ++k, dst += (long long)N * N) {
        const double sc = r * kLimbScale, limb = floor(sc);
        r = sc - limb;
        if (limb > 0.0) atomicAdd(dst, (unsigned long long)((long long)limb * c_i));
        if (limb > 0.0 || emitted) ++emitted;
      }
    }
    if (++b == L) {
      ++a;
      b = a + 1;
      if (a == L - 1) {                            // next track that has a pair (there is one while t + 1 < T)
        if (t + 1 >= tend) break;
        do {
          ++p;
          s = ptr[p];
          L = ptr[p + 1] - s;
        } while (L < 2);
        a = 0;
        b = 1;
        px = xyz[3 * p];
        py = xyz[3 * p + 1];
        pz = xyz[3 * p + 2];
      }
    }
  }
}

__global__ __launch_bounds__(256) void colmap_obs_depth_kernel(const int* __restrict__ obs_img,
                                                               const long long* __restrict__ obs_pt,
                                                               const double* __restrict__ xyz,
                                                               const double* __restrict__ zrow, long long n,
                                                               double* __restrict__ z) {
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (long long)gridDim.x * blockDim.x) {
    const double* r = zrow + 4 * (long long)obs_img[e];
    const double* x = xyz + 3 * obs_pt[e];
    z[e] = ((r[0] * x[0] + r[1] * x[1]) + r[2] * x[2]) + r[3];
  }
}

// lane 2 i: depth_min of image i, lane 2 i + 1: its depth_max; z_sorted holds image i's values ascending in
// obs_ptr[i] .. obs_ptr[i + 1] - 1
__global__ __launch_bounds__(64) void colmap_depth_means_kernel(const double* __restrict__ z_sorted,
                                                                const long long* __restrict__ obs_ptr,
                                                                const int* __restrict__ num_min,
                                                                const int* __restrict__ num_max, int N,
                                                                double* __restrict__ out) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= 2 * N) return;
  const int i = g >> 1;
  const long long s = obs_ptr[i], n = obs_ptr[i + 1] - s;
  long long m = (g & 1) ? num_max[i] : num_min[i];
  m = m < n ? m : n;
  const double* v = z_sorted + ((g & 1) ? s + n - m : s);
  double sum = 0.0;
  for (long long k = 0; k < m; ++k) sum = sum + v[k];
  out[g] = sum / (double)m;
}

}  // namespace

extern "C" int cds_colmap_score_quantum_log2(void) { return CDS_COLMAP_SCORE_QUANTUM_LOG2; }

// Limbs that hold the two leading limbs of the smallest weight of the rule: theta in [0, 180] puts the exponent at most at
// max(theta0^2 / (2 sigma1^2), (180 - theta0)^2 / (2 sigma2^2)) (theta0 outside [0, 180]: the larger distance to an end).
extern "C" int cds_colmap_score_limbs(double theta0, double sigma1, double sigma2) {
  if (!(sigma1 > 0.0) || !(sigma2 > 0.0) || !(theta0 == theta0)) return CDS_EINVAL;
  const double lo = fabs(theta0), hi = fabs(180.0 - theta0);
  const double e1 = lo * lo / (2.0 * sigma1 * sigma1), e2 = hi * hi / (2.0 * sigma2 * sigma2);
  const double e = theta0 <= 0.0 ? fmax(lo * lo, hi * hi) / (2.0 * sigma2 * sigma2)
                   : theta0 >= 180.0 ? fmax(lo * lo, hi * hi) / (2.0 * sigma1 * sigma1) : fmax(e1, e2);
  const double bits = e * 1.4426950408889634;              // w >= 2^-bits
  if (!(bits < 40.0 * (kMaxLimbs - 2))) return kMaxLimbs;
  return (int)(bits / 40.0) + 2;
}

extern "C" int cds_colmap_pair_scores_f64(const long long* pair_off, const long long* ptr, const int* img, const int* cnt,
                                          const double* xyz, const double* centres, long long P, long long T, int N,
                                          double theta0, double sigma1, double sigma2, int limbs, long long* acc,
                                          void* stream) {
  if (P < 1 || T < 0 || N < 1 || !pair_off || !ptr || !img || !cnt || !xyz || !centres || !acc || !(sigma1 > 0.0) ||
      !(sigma2 > 0.0) || limbs < 2 || limbs > kMaxLimbs)
    return CDS_EINVAL;
  if (T == 0) return 0;
  const long long lanes = (T + kTermsPerLane - 1) / kTermsPerLane;
  const long long blocks = (lanes + 255) / 256;
  if (blocks > INT32_MAX) return CDS_EINVAL;
  hipLaunchKernelGGL(colmap_pair_scores_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, pair_off, ptr, img,
                     cnt, xyz, centres, P, T, N, theta0, sigma1, sigma2, limbs, (unsigned long long*)acc);
  return cds_launch_status();
}

extern "C" int cds_colmap_obs_depth_f64(const int* obs_img, const long long* obs_pt, const double* xyz, const double* zrow,
                                        long long n, double* z, void* stream) {
  if (n < 1 || !obs_img || !obs_pt || !xyz || !zrow || !z) return CDS_EINVAL;
  const long long blocks = (n + 255) / 256 < 8192 ? (n + 255) / 256 : 8192;
  hipLaunchKernelGGL(colmap_obs_depth_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, obs_img, obs_pt, xyz,
                     zrow, n, z);
  return cds_launch_status();
}

extern "C" int cds_colmap_depth_ranges_f64(const double* z_sorted, const long long* obs_ptr, const int* num_min,
                                           const int* num_max, int N, double* out, void* stream) {
  if (N < 1 || !z_sorted || !obs_ptr || !num_min || !num_max || !out) return CDS_EINVAL;
  hipLaunchKernelGGL(colmap_depth_means_kernel, dim3((2 * N + 63) / 64), dim3(64), 0, (hipStream_t)stream, z_sorted, obs_ptr,
                     num_min, num_max, N, out);
  return cds_launch_status();
}
