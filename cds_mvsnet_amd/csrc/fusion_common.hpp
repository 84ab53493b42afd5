// The re-projection shared by the depth-fusion kernels of fusion.hip (normal) and fusion_dynamic.hip (dynamic consistency):
// the camera chain, the probability filter, the four-tap sample of the "source pixel -> (x, y, depth) in the reference view"
// map and the world point of a fused depth.  The fp32 operation order here is part of both rules.
// Camera block per view (100 floats, row-major), chain "image -> camera -> world -> other camera -> image":
//   [0]  Kinv_ref 3x3  [9]  Einv_ref 4x4  [25] E_src 4x4  [41] K_src 3x3       (reference -> source)
//   [50] Kinv_src 3x3  [59] Einv_src 4x4  [75] E_ref 4x4  [91] K_ref 3x3       (source -> reference)
//
// Everything here sits in an anonymous namespace: each translation unit gets its own copy, nothing is exported.
#pragma once
#include "cds_common.hpp"

namespace {

struct Xyd {
  float x, y, d;
};

// img (x,y,1) with depth -> image coordinates in the other view and depth in the other camera (fusion.py:24-46)
__device__ __forceinline__ Xyd chain(const float* __restrict__ m, float px, float py, float depth) {
  // idx_img2cam: Kinv @ pix, normalised by its last component, times depth
  float cx = m[0] * px + m[1] * py + m[2];
  float cy = m[3] * px + m[4] * py + m[5];
  float cz = m[6] * px + m[7] * py + m[8];
  const float n = cz + 1e-9f;
  cx = cx / n * depth;
  cy = cy / n * depth;
  cz = cz / n * depth;
  // idx_cam2world: Einv @ (cx,cy,cz,1), normalised
  const float* e = m + 9;
  float wx = e[0] * cx + e[1] * cy + e[2] * cz + e[3];
  float wy = e[4] * cx + e[5] * cy + e[6] * cz + e[7];
  float wz = e[8] * cx + e[9] * cy + e[10] * cz + e[11];
  float ww = e[12] * cx + e[13] * cy + e[14] * cz + e[15];
  const float nw = ww + 1e-9f;
  wx /= nw; wy /= nw; wz /= nw; ww /= nw;
  // idx_world2cam: E_other @ world, normalised
  const float* f = m + 25;
  float ox = f[0] * wx + f[1] * wy + f[2] * wz + f[3] * ww;
  float oy = f[4] * wx + f[5] * wy + f[6] * wz + f[7] * ww;
  float oz = f[8] * wx + f[9] * wy + f[10] * wz + f[11] * ww;
  float ow = f[12] * wx + f[13] * wy + f[14] * wz + f[15] * ww;
  const float no = ow + 1e-9f;
  ox /= no; oy /= no; oz /= no; ow /= no;
  // idx_cam2img: K @ (xyz / w), normalised by z
  const float nq = ow + 1e-9f;
  const float qx = ox / nq, qy = oy / nq, qz = oz / nq;
  const float* k = m + 41;
  float ix = k[0] * qx + k[1] * qy + k[2] * qz;
  float iy = k[3] * qx + k[4] * qy + k[5] * qz;
  float iz = k[6] * qx + k[7] * qy + k[8] * qz;
  const float ni = iz + 1e-9f;
  Xyd r;
  r.x = ix / ni;
  r.y = iy / ni;
  r.d = oz;  // depth in the other camera (srcs2ref_idx_cam[..., 2])
  return r;
}

__device__ __forceinline__ bool prob_ok(const float* __restrict__ conf, size_t hw, size_t p, float t0, float t1, float t2) {
  return conf[p] > t0 && conf[hw + p] > t1 && conf[2 * hw + p] > t2;
}

// Reference pixel centre (px, py) with depth rd through source view (m, sd, sc): project into the source view, clamp the grid
// coordinates to +-1.1, take in_range before the sample, then sample the source -> reference (x, y, depth) map bilinearly
// (zero padding, align_corners=True), evaluated at the four taps from the probability-filtered source depth.
__device__ __forceinline__ Xyd reproject(const float* __restrict__ m, const float* __restrict__ sd,
                                         const float* __restrict__ sc, size_t hw, int h, int w, float px, float py, float rd,
                                         float t0, float t1, float t2, bool& in_range) {
  const Xyd q = chain(m, px, py, rd);
  float gx = q.x / (float)w * 2.0f - 1.0f;
  float gy = q.y / (float)h * 2.0f - 1.0f;
  gx = fminf(fmaxf(gx, -1.1f), 1.1f);
  gy = fminf(fmaxf(gy, -1.1f), 1.1f);
  in_range = (gx >= -1.0f) && (gx <= 1.0f) && (gy >= -1.0f) && (gy <= 1.0f);
  const float ix = (gx + 1.0f) * 0.5f * (float)(w - 1), iy = (gy + 1.0f) * 0.5f * (float)(h - 1);
  const float x0f = floorf(ix), y0f = floorf(iy);
  const float wx1 = ix - x0f, wx0 = 1.0f - wx1, wy1 = iy - y0f, wy0 = 1.0f - wy1;
  const int x0 = (int)x0f, y0 = (int)y0f;
  Xyd o;
  o.x = 0.f; o.y = 0.f; o.d = 0.f;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int xs = x0 + (t & 1), ys = y0 + (t >> 1);
    if (xs < 0 || xs >= w || ys < 0 || ys >= h) continue;   // zero padding
    const size_t sp = (size_t)ys * w + xs;
    const float d_s = prob_ok(sc, hw, sp, t0, t1, t2) ? sd[sp] : 0.f;   // src_depths *= prob_mask (test.py:336-338)
    const Xyd r = chain(m + 50, (float)xs + 0.5f, (float)ys + 0.5f, d_s);
    const float wt = ((t & 1) ? wx1 : wx0) * ((t >> 1) ? wy1 : wy0);
    o.x = fmaf(r.x, wt, o.x);
    o.y = fmaf(r.y, wt, o.y);
    o.d = fmaf(r.d, wt, o.d);
  }
  return o;
}

// world point of a fused depth (test.py:348-350): Einv_ref @ (Kinv_ref @ pix / z * depth), written to points [3][hw]
__device__ __forceinline__ void store_world_point(const float* __restrict__ m, float px, float py, float ave,
                                                  float* __restrict__ points, size_t hw, int p) {
  float cx = m[0] * px + m[1] * py + m[2], cy = m[3] * px + m[4] * py + m[5], cz = m[6] * px + m[7] * py + m[8];
  const float n = cz + 1e-9f;
  cx = cx / n * ave; cy = cy / n * ave; cz = cz / n * ave;
  const float* e = m + 9;
  const float ww = e[12] * cx + e[13] * cy + e[14] * cz + e[15] + 1e-9f;
  points[p] = (e[0] * cx + e[1] * cy + e[2] * cz + e[3]) / ww;
  points[hw + p] = (e[4] * cx + e[5] * cy + e[6] * cz + e[7]) / ww;
  points[2 * hw + p] = (e[8] * cx + e[9] * cy + e[10] * cz + e[11]) / ww;
}

}  // namespace
