// Depth-map filtering + fusion (reference: fusion.py:7-114 and test.py:334-351).
// One thread per reference pixel.  For every source view: project the pixel (with the reference depth) into the source
// view, bilinearly sample — zero padding, align_corners=True — the map "source pixel -> (x, y, depth) re-projected into
// the reference view" (computed on the fly at the four taps from the probability-filtered source depth instead of being
// materialised as a [V,3,h,w] tensor), then apply the pixel-distance / relative-depth / in-range tests, count
// the consistent views and average the consistent depths (ave_fusion).  Output: fused depth, final mask
// (photometric AND geometric) and the world-space point of every pixel.
// The camera block layout, the chain and the four-tap sample are in fusion_common.hpp (shared with fusion_dynamic.hip).
#include "fusion_common.hpp"

namespace {

__global__ __launch_bounds__(256) void depth_fusion_kernel(const float* __restrict__ ref_depth,
                                                           const float* __restrict__ ref_conf,
                                                           const float* __restrict__ src_depths,
                                                           const float* __restrict__ src_confs,
                                                           const float* __restrict__ cams, float* __restrict__ fused,
                                                           float* __restrict__ mask_out, float* __restrict__ points,
                                                           float* __restrict__ view_masks, int V, int h, int w, float t0,
                                                           float t1, float t2, float dist_thresh, float depth_thresh,
                                                           float vthresh) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  const size_t hw = (size_t)h * w;
  if (p >= h * w) return;
  const int y = p / w, x = p % w;
  const float px = (float)x + 0.5f, py = (float)y + 0.5f;
  const float rd = ref_depth[p];
  float sum_m = 0.f, sum_d = 0.f;
  for (int v = 0; v < V; ++v) {
    const float* __restrict__ m = cams + (size_t)v * 100;
    const float* __restrict__ sd = src_depths + (size_t)v * hw;
    const float* __restrict__ sc = src_confs + (size_t)v * 3 * hw;
    bool in_range;
    const Xyd o = reproject(m, sd, sc, hw, h, w, px, py, rd, t0, t1, t2, in_range);
    const float rx = o.x, ry = o.y, rz = o.d;
    const float dx = rx - px, dy = ry - py;
    const bool dist_ok = sqrtf(dx * dx + dy * dy) < dist_thresh;
    const bool depth_ok = fabsf(rd - rz) < fmaxf(rd, rz) * depth_thresh;
    const float mv = (in_range && dist_ok && depth_ok) ? 1.0f : 0.0f;
    if (view_masks) view_masks[(size_t)v * hw + p] = mv;
    sum_m += mv;
    sum_d = fmaf(rz, mv, sum_d);
  }
  const bool vis_ok = sum_m >= vthresh - 1.1f;
  const float ave = (sum_d + rd) / (sum_m + 1.0f);
  const bool keep = vis_ok && prob_ok(ref_conf, hw, p, t0, t1, t2);
  fused[p] = ave;
  mask_out[p] = keep ? 1.0f : 0.0f;
  store_world_point(cams, px, py, ave, points, hw, p);
}

}  // namespace

extern "C" int cds_depth_fusion_f32(const float* ref_depth, const float* ref_conf, const float* src_depths,
                                    const float* src_confs, const float* cams, float* fused, float* mask, float* points,
                                    float* view_masks, int V, int h, int w, const float* prob_thresh_host,
                                    float dist_thresh, float depth_thresh, float view_thresh, void* stream) {
  if (!ref_depth || !ref_conf || !src_depths || !src_confs || !cams || !fused || !mask || !points || !prob_thresh_host ||
      V < 1 || h < 1 || w < 1)
    return CDS_EINVAL;
  hipLaunchKernelGGL(depth_fusion_kernel, dim3(cds_ceil_div(h * w, 256)), dim3(256), 0, (hipStream_t)stream, ref_depth,
                     ref_conf, src_depths, src_confs, cams, fused, mask, points, view_masks, V, h, w, prob_thresh_host[0],
                     prob_thresh_host[1], prob_thresh_host[2], dist_thresh, depth_thresh, view_thresh);
  return cds_launch_status();
}
