// Depth-map fusion with a dynamic consistency check (the rule is stated in include/cds_mvsnet_hip.h).
// One thread per reference pixel, the launch shape and the re-projection of depth_fusion_kernel (fusion_common.hpp).
// Per source view the pixel distance e_v and the relative depth difference r_v = |rd - rz_v| / rd give the view's level
// l_v: the smallest n in [1, n_max] with in_range_v, e_v < n * dist_base and r_v < n * rel_base (n_max + 1: inconsistent).
// The pixel is admitted at the smallest n in [n_min, min(n_max, V)] at which at least n views have l_v <= n; the fused
// depth averages the reference depth with every view consistent at n_max.
// The counts c_n live in kMaxLevels registers: every index into them is a compile-time constant (unrolled loops), so
// nothing goes to scratch.
#include "fusion_common.hpp"

namespace {

constexpr int kMaxLevels = 16;   // cap of n_max

__global__ __launch_bounds__(256) void depth_fusion_dynamic_kernel(
    const float* __restrict__ ref_depth, const float* __restrict__ ref_conf, const float* __restrict__ src_depths,
    const float* __restrict__ src_confs, const float* __restrict__ cams, float* __restrict__ fused,
    float* __restrict__ mask_out, float* __restrict__ points, unsigned char* __restrict__ admit_out,
    unsigned char* __restrict__ levels_out, int V, int h, int w, float t0, float t1, float t2, float dist_base, float rel_base,
    int n_min, int n_max) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  const size_t hw = (size_t)h * w;
  if (p >= h * w) return;
  const int y = p / w, x = p % w;
  const float px = (float)x + 0.5f, py = (float)y + 0.5f;
  const float rd = ref_depth[p];
  int c[kMaxLevels];   // c[n-1] = #{v : l_v <= n}
#pragma unroll
  for (int i = 0; i < kMaxLevels; ++i) c[i] = 0;
  float sum_d = 0.f;
  int n_cons = 0;   // views consistent at n_max: they enter the average, in view order
  for (int v = 0; v < V; ++v) {
    const float* __restrict__ m = cams + (size_t)v * 100;
    const float* __restrict__ sd = src_depths + (size_t)v * hw;
    const float* __restrict__ sc = src_confs + (size_t)v * 3 * hw;
    bool in_range;
    const Xyd o = reproject(m, sd, sc, hw, h, w, px, py, rd, t0, t1, t2, in_range);
    const float dx = o.x - px, dy = o.y - py;
    const float e = sqrtf(dx * dx + dy * dy);
    const float r = fabsf(rd - o.d) / rd;   // rd == 0: NaN or inf, every comparison below is false
    int l = n_max + 1;
    if (in_range) {
      for (int n = 1; n <= n_max; ++n) {
        if (e < (float)n * dist_base && r < (float)n * rel_base) {
          l = n;
          break;
        }
      }
    }
    if (levels_out) levels_out[(size_t)v * hw + p] = (unsigned char)l;
#pragma unroll
    for (int i = 0; i < kMaxLevels; ++i) c[i] += (l <= i + 1) ? 1 : 0;
    if (l <= n_max) {
      sum_d += o.d;
      ++n_cons;
    }
  }
  const int n_top = min(n_max, V);
  int admit = 0;
#pragma unroll
  for (int i = kMaxLevels - 1; i >= 0; --i) {   // descending: the smallest admitting n is written last
    const int n = i + 1;
    if (n >= n_min && n <= n_top && c[i] >= n) admit = n;
  }
  const float ave = (rd + sum_d) / (1.0f + (float)n_cons);
  const bool keep = admit > 0 && prob_ok(ref_conf, hw, p, t0, t1, t2);
  fused[p] = ave;
  mask_out[p] = keep ? 1.0f : 0.0f;
  if (admit_out) admit_out[p] = (unsigned char)admit;
  store_world_point(cams, px, py, ave, points, hw, p);
}

}  // namespace

extern "C" int cds_depth_fusion_dynamic_f32(const float* ref_depth, const float* ref_conf, const float* src_depths,
                                            const float* src_confs, const float* cams, float* fused, float* mask,
                                            float* points, unsigned char* admit, unsigned char* levels, int V, int h, int w,
                                            const float* prob_thresh_host, float dist_base, float rel_base, int n_min,
                                            int n_max, void* stream) {
  if (!ref_depth || !ref_conf || !src_depths || !src_confs || !cams || !fused || !mask || !points || !prob_thresh_host ||
      V < 1 || h < 1 || w < 1 || n_min < 1 || n_max < n_min || n_max > kMaxLevels || !(dist_base > 0.f) || !(rel_base > 0.f))
    return CDS_EINVAL;
  hipLaunchKernelGGL(depth_fusion_dynamic_kernel, dim3(cds_ceil_div(h * w, 256)), dim3(256), 0, (hipStream_t)stream,
                     ref_depth, ref_conf, src_depths, src_confs, cams, fused, mask, points, admit, levels, V, h, w,
                     prob_thresh_host[0], prob_thresh_host[1], prob_thresh_host[2], dist_base, rel_base, n_min, n_max);
  return cds_launch_status();
}
