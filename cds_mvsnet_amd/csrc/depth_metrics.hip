// Depth-map scoring against ground truth (reference: utils.py:134-167 Thres_metrics / AbsDepthError_metrics as trainer/trainer.py:140-164
// calls them, evaluations/precision.py:8-13,87-91) and the multi-scale ground truth the datasets prepare (datasets/dtu_yao.py:79-128,
// datasets/blended_dataset.py:79-120), on the device.  The reference formulation is ~12 masked-index / compare / mean passes per sample,
// each ending in a host read; here one pass over the pixels writes every sum the twelve validation scalars and the five precision
// scalars need.  As in loss.hip: 256-thread workgroups, fp64 sums in a fixed order (per-workgroup records, reduced by a second pass
// whose shape depends on the sizes only), no atomics - bit-reproducible run to run.
#include "cds_common.hpp"
#include "feat_common.hpp"

namespace {

constexpr int DM_MAX_T = CDS_DEPTH_METRICS_MAX_T;            // thresholds per image
constexpr int DM_MAX_GROUPS = CDS_DEPTH_METRICS_MAX_GROUPS;  // workgroups of the first pass (all images together)

// sum of v over the workgroup (256 threads), valid in every thread
__device__ __forceinline__ double dm_block_sum(double v, double* red) {
  v = wave_sum_f64(v);
  __syncthreads();                       // red may still be read from the previous call
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

// What one thread has seen.  Counts are integers (a thread sees < 2^31 pixels), sums are fp64 of fp32 values.  Every loop over the
// thresholds / bands is unrolled to the maximum with slots past T disabled by their limits, so the arrays live in registers.
struct DmAcc {
  unsigned n;
  double se, se2;
  unsigned over[DM_MAX_T];
  unsigned bn[DM_MAX_T + 1];
  double bs[DM_MAX_T + 1];
};

struct DmLimits {
  float thr[DM_MAX_T];         // slots >= T: +inf (no error exceeds it)
  float lo[DM_MAX_T + 1];      // band slots > T: lo = +inf, hi = -inf (no error lies in it)
  float hi[DM_MAX_T + 1];
};

__device__ __forceinline__ void dm_pixel(float est, float gt, float mask, const DmLimits& lim, DmAcc& a) {
  if (!(mask > 0.5f)) return;
  const float e = fabsf(est - gt);       // fp32, like the reference; every comparison below is fp32 against the fp32 threshold
  a.n += 1u;
  a.se += (double)e;
  a.se2 += (double)e * (double)e;        // exact square of the fp32 error
#pragma unroll
  for (int t = 0; t < DM_MAX_T; ++t) a.over[t] += e > lim.thr[t] ? 1u : 0u;
#pragma unroll
  for (int k = 0; k <= DM_MAX_T; ++k) {
    const bool in = e >= lim.lo[k] && e <= lim.hi[k];      // inclusive at both ends (utils.py:164)
    a.bn[k] += in ? 1u : 0u;
    a.bs[k] += in ? (double)e : 0.0;
  }
}

// Pass 1.  Workgroup (b, g) of `groups` per image strides over the pixels of image b only and writes record [b][g][3T + 5]:
// n, sum e, sum e^2, over[T], then (count, sum e) of the T + 1 bands.  vec: the three base pointers are 16-byte aligned; an image whose
// own offset b*hw is a multiple of 4 then reads float4, any other image (and the hw % 4 tail) reads scalars.
__global__ __launch_bounds__(256) void depth_metrics_kernel(const float* __restrict__ est, const float* __restrict__ gt,
                                                            const float* __restrict__ mask, const float* __restrict__ thr, float cap,
                                                            int T, long long hw, int groups, int vec, double* __restrict__ rec) {
  __shared__ double red[4];
  const int b = blockIdx.x / groups, g = blockIdx.x - b * groups;
  DmLimits lim;
#pragma unroll
  for (int t = 0; t < DM_MAX_T; ++t) lim.thr[t] = t < T ? thr[(size_t)b * T + t] : INFINITY;
#pragma unroll
  for (int k = 0; k <= DM_MAX_T; ++k) {
    lim.lo[k] = k > T ? INFINITY : (k == 0 ? 0.f : lim.thr[k - 1]);
    lim.hi[k] = k > T ? -INFINITY : (k == T ? cap : lim.thr[k]);
  }
  DmAcc a;
  a.n = 0u; a.se = 0.0; a.se2 = 0.0;
#pragma unroll
  for (int t = 0; t < DM_MAX_T; ++t) a.over[t] = 0u;
#pragma unroll
  for (int k = 0; k <= DM_MAX_T; ++k) { a.bn[k] = 0u; a.bs[k] = 0.0; }

  const size_t base = (size_t)b * (size_t)hw;
  const float* __restrict__ pe = est + base;
  const float* __restrict__ pg = gt + base;
  const float* __restrict__ pm = mask + base;
  const long long stride = (long long)groups * 256;
  const long long first = (long long)g * 256 + threadIdx.x;
  if (vec && (base & 3) == 0) {
    const long long nv = hw >> 2;
    const float4* __restrict__ ve = reinterpret_cast<const float4*>(pe);
    const float4* __restrict__ vg = reinterpret_cast<const float4*>(pg);
    const float4* __restrict__ vm = reinterpret_cast<const float4*>(pm);
    for (long long i = first; i < nv; i += stride) {
      const float4 m = vm[i], x = ve[i], y = vg[i];
      dm_pixel(x.x, y.x, m.x, lim, a);
      dm_pixel(x.y, y.y, m.y, lim, a);
      dm_pixel(x.z, y.z, m.z, lim, a);
      dm_pixel(x.w, y.w, m.w, lim, a);
    }
    for (long long i = (nv << 2) + first; i < hw; i += stride) dm_pixel(pe[i], pg[i], pm[i], lim, a);
  } else {
    for (long long i = first; i < hw; i += stride) dm_pixel(pe[i], pg[i], pm[i], lim, a);
  }

  const int NF = 3 * T + 5;
  double* __restrict__ r = rec + (size_t)blockIdx.x * NF;
  double v;
  v = dm_block_sum((double)a.n, red);  if (threadIdx.x == 0) r[0] = v;
  v = dm_block_sum(a.se, red);         if (threadIdx.x == 0) r[1] = v;
  v = dm_block_sum(a.se2, red);        if (threadIdx.x == 0) r[2] = v;
#pragma unroll
  for (int t = 0; t < DM_MAX_T; ++t) {
    if (t < T) {                                             // T is uniform: every thread takes the same branch
      v = dm_block_sum((double)a.over[t], red);
      if (threadIdx.x == 0) r[3 + t] = v;
    }
  }
#pragma unroll
  for (int k = 0; k <= DM_MAX_T; ++k) {
    if (k <= T) {
      v = dm_block_sum((double)a.bn[k], red);
      if (threadIdx.x == 0) r[3 + T + 2 * k] = v;
      v = dm_block_sum(a.bs[k], red);
      if (threadIdx.x == 0) r[3 + T + 2 * k + 1] = v;
    }
  }
}

// Pass 2.  Workgroup b sums the `groups` records of image b, field by field, in a fixed order -> out [b][3T + 5].
__global__ __launch_bounds__(256) void depth_metrics_reduce_kernel(const double* __restrict__ rec, int groups, int NF,
                                                                   double* __restrict__ out) {
  __shared__ double red[4];
  const double* __restrict__ r = rec + (size_t)blockIdx.x * groups * NF;
  for (int f = 0; f < NF; ++f) {
    double s = 0.0;
    for (int i = threadIdx.x; i < groups; i += 256) s += r[(size_t)i * NF + f];
    s = dm_block_sum(s, red);
    if (threadIdx.x == 0) out[(size_t)blockIdx.x * NF + f] = s;
  }
}

struct GtLevels {
  long long off[5];            // first element of level k in the packed outputs; off[levels] = total
  int w[4];                    // width of level k
  int levels;
};

// Element i of the packed pyramid: level k pixel (y, x) = level-0 pixel (y << k, x << k) = source (rows[y << k], cols[x << k]).
// A table entry outside the source gives depth 0 / mask 0 (the host wrapper refuses such tables; this keeps the read in bounds).
__global__ __launch_bounds__(256) void gt_pyramid_kernel(const float* __restrict__ src, const unsigned char* __restrict__ mask_src,
                                                         int mask_thresh, int Hs, int Ws, const int* __restrict__ rows,
                                                         const int* __restrict__ cols, GtLevels lv, float* __restrict__ depth_out,
                                                         float* __restrict__ mask_out) {
  const long long total = lv.off[lv.levels];
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    int k = 0;
    if (lv.levels > 1 && i >= lv.off[1]) k = 1;
    if (lv.levels > 2 && i >= lv.off[2]) k = 2;
    if (lv.levels > 3 && i >= lv.off[3]) k = 3;
    const long long p = i - lv.off[k];
    const int wk = lv.w[k];
    const int y = (int)(p / wk), x = (int)(p - (long long)y * wk);
    const int sy = rows[y << k], sx = cols[x << k];
    float d = 0.f, m = 0.f;
    if ((unsigned)sy < (unsigned)Hs && (unsigned)sx < (unsigned)Ws) {
      const size_t s = (size_t)sy * Ws + sx;
      d = src[s];
      m = mask_src ? ((int)mask_src[s] > mask_thresh ? 1.f : 0.f) : (d > 0.f ? 1.f : 0.f);
    }
    depth_out[i] = d;
    mask_out[i] = m;
  }
}

inline int dm_groups(int B, long long hw) {
  const long long per_image = DM_MAX_GROUPS / B < 1 ? 1 : DM_MAX_GROUPS / B;
  const long long want = (hw + 255) / 256;
  return (int)(want < per_image ? want : per_image);
}

}  // namespace

// est, gt, mask [B][hw] fp32; thr [B][T] fp32 on the DEVICE (NULL when T = 0), ascending per image (the caller checks);
// ws: workspace of ws_doubles >= CDS_DEPTH_METRICS_WS_DOUBLES(B) doubles; out [B][3T + 5] doubles.
extern "C" int cds_depth_metrics_f32(const float* est, const float* gt, const float* mask, const float* thr, float cap, int B,
                                     long long hw, int T, double* ws, long long ws_doubles, double* out, void* stream) {
  if (!est || !gt || !mask || !ws || !out || B < 1 || hw < 1 || T < 0 || T > DM_MAX_T || (T > 0 && !thr)) return CDS_EINVAL;
  const int groups = dm_groups(B, hw);
  const int NF = 3 * T + 5;
  if ((long long)B * groups * NF > ws_doubles) return CDS_EINVAL;
  if ((long long)B * groups > 0x7fffffffLL) return CDS_EINVAL;
  const int vec = ((reinterpret_cast<uintptr_t>(est) | reinterpret_cast<uintptr_t>(gt) | reinterpret_cast<uintptr_t>(mask)) & 15) == 0;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(depth_metrics_kernel, dim3((unsigned)(B * groups)), dim3(256), 0, st, est, gt, mask, thr, cap, T, hw, groups, vec, ws);
  hipLaunchKernelGGL(depth_metrics_reduce_kernel, dim3((unsigned)B), dim3(256), 0, st, ws, groups, NF, out);
  return cds_launch_status();
}

// src [Hs][Ws] fp32; mask_src [Hs][Ws] uint8 (mask = value > mask_thresh) or NULL (mask = depth > 0); rows [h], cols [w] int32 on the
// DEVICE; depth_out, mask_out: the levels packed one after the other, level k holding (h >> k) x (w >> k) floats.
extern "C" int cds_gt_pyramid_f32(const float* src, const unsigned char* mask_src, int mask_thresh, int Hs, int Ws, const int* rows,
                                  const int* cols, int h, int w, int levels, float* depth_out, float* mask_out, void* stream) {
  if (!src || !rows || !cols || !depth_out || !mask_out || Hs < 1 || Ws < 1 || h < 1 || w < 1 || levels < 1 || levels > 4) return CDS_EINVAL;
  const int step = 1 << (levels - 1);
  if (h % step || w % step) return CDS_EINVAL;
  GtLevels lv{};
  lv.levels = levels;
  long long off = 0;
  for (int k = 0; k < levels; ++k) {
    lv.off[k] = off;
    lv.w[k] = w >> k;
    off += (long long)(h >> k) * (w >> k);
  }
  lv.off[levels] = off;
  const long long blocks = (off + 255) / 256;
  hipLaunchKernelGGL(gt_pyramid_kernel, dim3((unsigned)(blocks > 4096 ? 4096 : blocks)), dim3(256), 0, (hipStream_t)stream, src, mask_src,
                     mask_thresh, Hs, Ws, rows, cols, lv, depth_out, mask_out);
  return cds_launch_status();
}
