// Shared pieces of the z-marching transposed-convolution kernels (deconv3d_zm.hip, deconv_prob_zm.hip): which column and z segment
// a workgroup owns, the staging of one input cell plane into the LDS ring, and the host's choice of the number of z segments.
#pragma once
#include "sbf_common.hpp"

namespace {

// Workgroup -> (column tx_i, ty_i; cell planes [a0, a1)): the columns of one z segment are consecutive workgroups after the XCD
// remap.  a0 >= a1: the segment is past the volume and the workgroup has nothing to do.
struct ZmColumn {
  int tx_i, ty_i, a0, a1;
};
__device__ __forceinline__ ZmColumn zm_column(int tiles_x, int ncols, int seg_len, int D) {
  const int wg = cds_xcd_remap(blockIdx.x, gridDim.x);
  const int col = wg % ncols, seg = wg / ncols;
  const int a0 = seg * seg_len;
  return {col % tiles_x, col / tiles_x, a0, min(D, a0 + seg_len)};
}

// Staging of one input cell plane by NTHR threads: item it = (cell p = it / ROUNDS in row-major IY x IX order, 8-channel round
// it % ROUNDS); thread t owns items t, t + NTHR, ...  init() fixes each item's element offset inside a plane of x[] (-1: outside the
// volume in y / x, or no such item) and its byte offset inside a ring slot; issue() loads a plane into registers with UNCONDITIONAL
// loads (an out-of-volume item reads element 0 of the last plane and is replaced by zeros: no exec-masked branch per item); deposit()
// splits and stores them into the slot the caller names (the ring arithmetic stays with the kernel).  The loads of issue() may be
// left in flight across other work before deposit().
// C supplies ROUNDS, IX, IXP, ROUNDB, NITEM.  LOWHALO: the column starts one cell below its first owned cell, so y / x can be < 0.
template <class C, int NTHR, bool F16, bool LOWHALO>
struct ZmCellStage {
  static constexpr int Cin = 8 * C::ROUNDS;
  static constexpr int IPT = (C::NITEM + NTHR - 1) / NTHR;
  int src[IPT], dst[IPT];
  float4 va[IPT], vb[IPT];

  __device__ __forceinline__ void init(int t, int X0, int Y0, int H, int W) {
#pragma unroll
    for (int h = 0; h < IPT; ++h) {
      const int it = h * NTHR + t;
      const int rd = it % C::ROUNDS, p = it / C::ROUNDS;
      const int row = p / C::IX, c = p - row * C::IX;
      const int gy = Y0 + row, gx = X0 + c;
      const bool ok = it < C::NITEM && (!LOWHALO || gy >= 0) && gy < H && (!LOWHALO || gx >= 0) && gx < W;
      src[h] = ok ? ((gy * W + gx) * Cin + rd * 8) : -1;
      dst[h] = it < C::NITEM ? rd * C::ROUNDB + (row * C::IXP + c) * POSB : -1;
    }
  }
  __device__ __forceinline__ void issue(const float* __restrict__ x, int plane, int D, int H, int W) {
    const bool pok = plane < D;
    const float* __restrict__ xp = x + (size_t)min(plane, D - 1) * H * W * Cin;
#pragma unroll
    for (int h = 0; h < IPT; ++h) {
      const bool ok = pok && src[h] >= 0;
      const float* s = xp + (ok ? src[h] : 0);
      const float4 a = *reinterpret_cast<const float4*>(s), b = *reinterpret_cast<const float4*>(s + 4);
      va[h] = ok ? a : make_float4(0.f, 0.f, 0.f, 0.f);
      vb[h] = ok ? b : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  }
  __device__ __forceinline__ void deposit(unsigned char* slot, float xs) const {
#pragma unroll
    for (int h = 0; h < IPT; ++h)
      if (dst[h] >= 0) {
        if (F16) split_store8_f16(slot + dst[h], va[h], vb[h], xs);
        else split_store8(slot + dst[h], va[h], vb[h]);
      }
  }
};

// z segments per column: whole rounds of 256 single-resident workgroups against the 1.5 cell planes a segment spends priming its
// ring (in units of one cell plane; the fused tail's two half-steps per plane scale every candidate alike).  env_name: A/B and test
// knob, read per launch.
inline int zm_pick_nseg(int wgs_per_seg, int D, int cap, const char* env_name) {
  int best = 1;
  double best_cost = 1e30;
  for (int n = 1; n <= min(D, cap); ++n) {
    const int len = cds_ceil_div(D, n);
    const int n_eff = cds_ceil_div(D, len);
    const double cost = (double)cds_ceil_div(wgs_per_seg * n_eff, 256) * (len + 1.5);
    if (cost < best_cost - 1e-9) { best_cost = cost; best = n; }
  }
  const int nseg_e = cds_env_int(env_name, 0);
  return nseg_e > 0 ? min(nseg_e, D) : best;
}

}  // namespace
