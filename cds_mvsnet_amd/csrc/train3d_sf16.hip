// Split-f16 training kernels of the CostRegNet stack (the opt-in train_ops.conv_arithmetic("split_f16") mode).  The arithmetic is the
// inference path's (sbf_common.hpp): every fp32 operand becomes two fp16 terms hi + lo of (value x a power-of-two tensor scale), three
// v_mfma_f32_16x16x32_f16 products per K-step (hi hi + hi lo + lo hi), fp32 accumulation, the exact 1 / (s_a s_b) rescale before a value
// leaves the workgroup.  What is new is the data flow of training:
//   cds_absmax_bound_f32        running max |x| of a tensor into a device slot (the operand without a producing kernel: conv0's input)
//   cds_sf16_pack_conv3d_f32    max |w| on the device, the hi / lo terms of the forward and data-gradient operands, 1 / s_w: one launch,
//                               no host read (weights change every step; the captured step stays capturable)
//   cds_conv3d_k3_sf16_f32      planar [B][C][D][H][W] k3 convolution, stride 1 / 2, or the transposed k3 s2 convolution (eight output
//                               parity classes, each a small convolution of the input grid): forward, and every data gradient
//   cds_conv3d_wgrad_sf16_f32   dw[a][b][tap] += sum g[a][o] xin[b][S o - 1 + tap], the cross-workgroup reduction of
//                               cds_conv3d_wgrad_f32 with the rescale applied before the atomics
// Operand scales come from device-resident upper bounds of max |x| (sf16_scale); a bound that is too large costs low-order bits only.
#include "sbf_common.hpp"

namespace {

constexpr int SF_TAPS = 28;   // 27 taps + one all-zero tap that pads the last K-step of a convolution

__global__ __launch_bounds__(256) void absmax_bound_kernel(const float* __restrict__ x, size_t n, float* __restrict__ bound) {
  float m = 0.f;
  if ((n & 3) == 0 && ((uintptr_t)x & 15) == 0) {
    const float4* __restrict__ x4 = reinterpret_cast<const float4*>(x);
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < (n >> 2); i += (size_t)gridDim.x * 256) {
      const float4 v = x4[i];
      m = fmaxf(m, fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w))));
    }
  } else {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) m = fmaxf(m, fabsf(x[i]));
  }
  sf16_publish_bound(m, bound);
}

// Packed operand of one layer and pass: [C/8][28 taps][2 terms][Mpad][8 channels] fp16, A[m][c][tap] of the GEMM y[m] = sum A x[c].
// (transpose t, flip f): t = 0: A[m][c][k] = w[m][c][k] (w [A=M][B=C]); t = 1: A[m][c][k] = w[c][m][f ? 26 - k : k] (w [A=C][B=M]).
__device__ __forceinline__ int sf16_pack_items(int A, int Bc, int t) {
  const int M = t ? Bc : A, C = t ? A : Bc;
  return (C / 8) * SF_TAPS * ((M + 15) / 16 * 16);
}
__device__ void sf16_pack_item(const float* __restrict__ w, int A, int Bc, int t, int f, float s, _Float16* __restrict__ dst, int it) {
  const int M = t ? Bc : A, Mp = (M + 15) / 16 * 16;
  const int mm = it % Mp, tap = (it / Mp) % SF_TAPS, cc = it / (Mp * SF_TAPS);
  float v[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int c = cc * 8 + j;
    v[j] = 0.f;
    if (tap < 27 && mm < M) v[j] = t ? w[((size_t)c * Bc + mm) * 27 + (f ? 26 - tap : tap)] : w[((size_t)mm * Bc + c) * 27 + tap];
  }
  uint32_t h[4], l[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) split2_f16(v[2 * j], v[2 * j + 1], s, h[j], l[j]);
  uint4* d = reinterpret_cast<uint4*>(dst + ((size_t)((cc * SF_TAPS + tap) * 2) * Mp + mm) * 8);
  d[0] = make_uint4(h[0], h[1], h[2], h[3]);
  d[Mp] = make_uint4(l[0], l[1], l[2], l[3]);
}

// A few workgroups, each of which takes max |w| itself (at most 64 x 64 x 27 floats, read as float4 from L2) and then packs its share of
// the items of both operands.  (One 1024-thread workgroup doing all of it was ~40 us per launch: a serial chain of strided loads.)
__global__ __launch_bounds__(256) void sf16_pack_conv3d_kernel(const float* __restrict__ w, int A, int Bc, int mode,
                                                               _Float16* __restrict__ fwd, _Float16* __restrict__ dg,
                                                               float* __restrict__ w_inv) {
  __shared__ float red[4];
  const int n = A * Bc * 27;                                        // a multiple of 4 (A, B multiples of 8)
  float m = 0.f;
  if (((uintptr_t)w & 15) == 0) {
    const float4* __restrict__ w4 = reinterpret_cast<const float4*>(w);
    for (int i = threadIdx.x; i < n / 4; i += 256) {
      const float4 v = w4[i];
      m = fmaxf(m, fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w))));
    }
  } else {
    for (int i = threadIdx.x; i < n; i += 256) m = fmaxf(m, fabsf(w[i]));
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  const float s = sf16_scale(m);
  if (blockIdx.x == 0 && threadIdx.x == 0) w_inv[0] = 1.0f / s;     // exact: s is a power of two
  // forward: Conv3d as stored, ConvTranspose3d transposed; data gradient: the stride-1 convolution's is flipped and transposed, the
  // stride-2 convolution's is the transposed convolution with the weights as stored (transposed view), the transposed convolution's is
  // the stride-2 convolution with the weights as stored
  const int tf = mode == 2, td = mode != 2, fd = mode == 0;
  const int nf = fwd ? sf16_pack_items(A, Bc, tf) : 0, nd = dg ? sf16_pack_items(A, Bc, td) : 0;
  for (int it = blockIdx.x * 256 + threadIdx.x; it < nf + nd; it += gridDim.x * 256) {
    if (it < nf)
      sf16_pack_item(w, A, Bc, tf, 0, s, fwd, it);
    else
      sf16_pack_item(w, A, Bc, td, fd, s, dg, it - nf);
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Convolution as a GEMM per workgroup: D[m][n] = sum_k A[m][k] X[k][n], m = output channel (Mpad = 16 MB), n = 16 voxels of one
// x-row of the output tile, k = (8-channel chunk, tap, channel).  A K-step of 32 = four taps x eight channels: lane l holds tap
// 4 g + l / 16 and the 8 channels of that tap.  Per 8-channel chunk the input halo is staged once in LDS, split, as [pos][term][8] fp16
// (one 16-byte read per operand term).  TR: the transposed k3 s2 convolution, one parity class (pz, py, px) of the output per
// blockIdx.z % 8: for o = 2 j + p the taps along a dimension are k = 1 (p = 0; input j) or k = 0, 2 (p = 1; inputs j + 1, j), so the
// class is a convolution of the input grid with 1..8 taps; its tile is in input coordinates.
// ---------------------------------------------------------------------------------------------------------------------------------
template <int S, int TZ, bool TR>
struct SfCfg {
  static constexpr int TX = 16, TY = 4;
  static constexpr int SS = TR ? 1 : S;
  static constexpr int HX = TR ? TX + 1 : (TX - 1) * S + 3, HY = TR ? TY + 1 : (TY - 1) * S + 3, HZ = TR ? TZ + 1 : (TZ - 1) * S + 3;
  static constexpr int NH = HX * HY * HZ;
  static constexpr int ROWS = TZ * TY, NQ = ROWS / 4;
  static constexpr int G = TR ? 2 : 7;          // K-steps per chunk (taps 4 g .. 4 g + 3)
};

template <int S, int TZ, bool TR, int MB>
__global__ __launch_bounds__(256) void conv3d_sf16_train_kernel(const float* __restrict__ x, const _Float16* __restrict__ wpk,
                                                                const float* __restrict__ w_inv, const float* __restrict__ x_bound,
                                                                float* __restrict__ y, int C, int M, int Di, int Hi, int Wi, int Do,
                                                                int Ho, int Wo, int tiles_x, int tiles_y) {
  using Cfg = SfCfg<S, TZ, TR>;
  __shared__ __attribute__((aligned(16))) uint4 lds[Cfg::NH * 2];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int col = lane & 15, kg = lane >> 4;
  const int b = blockIdx.y, cls = TR ? (int)blockIdx.z : 0;
  const int cpx = cls & 1, cpy = (cls >> 1) & 1, cpz = cls >> 2;
  int r = blockIdx.x;
  const int tx_i = r % tiles_x;
  r /= tiles_x;
  const int ty_i = r % tiles_y, tz_i = r / tiles_y;
  // tile origin: output voxels (convolution) or input voxels j of the class (transposed)
  const int o0x = tx_i * Cfg::TX, o0y = ty_i * Cfg::TY, o0z = tz_i * TZ;
  const int h0x = TR ? o0x : o0x * S - 1, h0y = TR ? o0y : o0y * S - 1, h0z = TR ? o0z : o0z * S - 1;
  const int Mp = MB * 16;
  const float xs = sf16_scale(x_bound[0]);
  const float scale_out = w_inv[0];
  const float xinv = 1.0f / xs;

  // this lane's taps of the G K-steps: LDS offset and weight tap (27 = the zero tap)
  int loff[Cfg::G], wtap[Cfg::G];
  {
    const int nx = TR ? (cpx ? 2 : 1) : 3, ny = TR ? (cpy ? 2 : 1) : 3, nz = TR ? (cpz ? 2 : 1) : 3;
    const int T = nx * ny * nz;
#pragma unroll
    for (int g = 0; g < Cfg::G; ++g) {
      const int t = 4 * g + kg;
      if (t >= T) {
        loff[g] = 0;
        wtap[g] = 27;
        continue;
      }
      const int ix = t % nx, iy = (t / nx) % ny, iz = t / (nx * ny);
      if (TR) {
        // p = 0: k = 1 at input j; p = 1: (k = 0 at j + 1, k = 2 at j)
        const int kx = cpx ? 2 * ix : 1, ky = cpy ? 2 * iy : 1, kz = cpz ? 2 * iz : 1;
        const int dx = cpx ? 1 - ix : 0, dy = cpy ? 1 - iy : 0, dz = cpz ? 1 - iz : 0;
        loff[g] = (dz * Cfg::HY + dy) * Cfg::HX + dx;
        wtap[g] = (kz * 3 + ky) * 3 + kx;
      } else {
        loff[g] = (iz * Cfg::HY + iy) * Cfg::HX + ix;
        wtap[g] = t;
      }
    }
  }
  int rowbase[Cfg::NQ];
#pragma unroll
  for (int q = 0; q < Cfg::NQ; ++q) {
    const int row = wave * Cfg::NQ + q, zz = row / Cfg::TY, yy = row % Cfg::TY;
    rowbase[q] = ((Cfg::SS * zz) * Cfg::HY + Cfg::SS * yy) * Cfg::HX + Cfg::SS * col;
  }
  f32x4 acc[MB][Cfg::NQ];
#pragma unroll
  for (int mb = 0; mb < MB; ++mb)
#pragma unroll
    for (int q = 0; q < Cfg::NQ; ++q) acc[mb][q] = (f32x4){0.f, 0.f, 0.f, 0.f};

  const size_t vin = (size_t)Di * Hi * Wi;
  for (int cc = 0; cc < C / 8; ++cc) {
    // a fresh partial sum per 8-channel chunk, added to the total after it: fp32 accumulation chains of 21 MFMAs, not 21 C / 8
    f32x4 part[MB][Cfg::NQ];
#pragma unroll
    for (int mb = 0; mb < MB; ++mb)
#pragma unroll
      for (int q = 0; q < Cfg::NQ; ++q) part[mb][q] = (f32x4){0.f, 0.f, 0.f, 0.f};
    __syncthreads();
    const float* __restrict__ xc = x + ((size_t)b * C + cc * 8) * vin;
    for (int p = tid; p < Cfg::NH; p += 256) {
      const int hx = p % Cfg::HX, hy = (p / Cfg::HX) % Cfg::HY, hz = p / (Cfg::HX * Cfg::HY);
      const int gx = h0x + hx, gy = h0y + hy, gz = h0z + hz;
      const bool ok = (unsigned)gx < (unsigned)Wi && (unsigned)gy < (unsigned)Hi && (unsigned)gz < (unsigned)Di;
      const size_t off = ok ? ((size_t)gz * Hi + gy) * Wi + gx : 0;
      float v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float t = xc[(size_t)j * vin + off];
        v[j] = ok ? t : 0.f;
      }
      uint32_t h[4], l[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) split2_f16(v[2 * j], v[2 * j + 1], xs, h[j], l[j]);
      lds[2 * p] = make_uint4(h[0], h[1], h[2], h[3]);
      lds[2 * p + 1] = make_uint4(l[0], l[1], l[2], l[3]);
    }
    __syncthreads();
#pragma unroll
    for (int g = 0; g < Cfg::G; ++g) {
      BV wa[MB][2];
#pragma unroll
      for (int mb = 0; mb < MB; ++mb) {
        const uint4* wp = reinterpret_cast<const uint4*>(wpk + ((size_t)((cc * SF_TAPS + wtap[g]) * 2) * Mp + mb * 16 + col) * 8);
        wa[mb][0].u = wp[0];
        wa[mb][1].u = wp[Mp];
      }
      BV xb[Cfg::NQ][2];
#pragma unroll
      for (int q = 0; q < Cfg::NQ; ++q) {
        const int pos = rowbase[q] + loff[g];
        xb[q][0].u = lds[2 * pos];
        xb[q][1].u = lds[2 * pos + 1];
      }
#pragma unroll
      for (int mb = 0; mb < MB; ++mb) {
        SF16_TERMS(part[mb], 0, Cfg::NQ, wa[mb], xb)
      }
    }
#pragma unroll
    for (int mb = 0; mb < MB; ++mb)
#pragma unroll
      for (int q = 0; q < Cfg::NQ; ++q) acc[mb][q] += part[mb][q];
  }
  // D: lane holds rows m = 4 kg + 0..3 of column n = col
#pragma unroll
  for (int q = 0; q < Cfg::NQ; ++q) {
    const int row = wave * Cfg::NQ + q, zz = row / Cfg::TY, yy = row % Cfg::TY;
    int ox = o0x + col, oy = o0y + yy, oz = o0z + zz;
    if (TR) {
      if (ox >= Wi || oy >= Hi || oz >= Di) continue;
      ox = 2 * ox + cpx;
      oy = 2 * oy + cpy;
      oz = 2 * oz + cpz;
    }
    if (ox >= Wo || oy >= Ho || oz >= Do) continue;
#pragma unroll
    for (int mb = 0; mb < MB; ++mb) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int m = mb * 16 + 4 * kg + e;
        if (m < M) y[(((size_t)b * M + m) * Do + oz) * Ho * (size_t)Wo + (size_t)oy * Wo + ox] = (acc[mb][q][e] * scale_out) * xinv;
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Weight gradient: cds_conv3d_wgrad_f32's MFMA kernel (same tiles, staging and cross-workgroup reduction) with K-steps of 32 voxels on
// the f16 matrix cores.  D[a][n] += A[a][k] B[k][n], a = 16 channels of g, n = (b, tap) column, k = voxel: lane l takes the voxels
// 8 r .. 8 r + 7 of the tile (one x-row, r = 4 ks + l / 16) and splits them from the fp32 LDS tile as it reads them.
// ---------------------------------------------------------------------------------------------------------------------------------
template <int S>
struct WsCfg {
  static constexpr int OX = 8, OY = 4, OZ = 4, NO = OX * OY * OZ;
  static constexpr int IX = (OX - 1) * S + 3, IY = (OY - 1) * S + 3, IZ = (OZ - 1) * S + 3;
  static constexpr int NI = IX * IY * IZ;
  static constexpr int GS = NO + 4;
};

template <typename Cfg, int S, int NQ>
__device__ __forceinline__ void wgrad_sf16_ksteps(const float* __restrict__ lg, const float* __restrict__ lx, int col, int kq,
                                                  const int* colofs, float gs, float xs, f32x4* acc) {
#pragma unroll
  for (int ks = 0; ks < Cfg::NO / 32; ++ks) {
    const int r = 4 * ks + kq, py = r % Cfg::OY, pz = r / Cfg::OY;
    const int base = ((pz * S) * Cfg::IY + py * S) * Cfg::IX;
    const float4 g0 = *reinterpret_cast<const float4*>(lg + col * Cfg::GS + 8 * r);
    const float4 g1 = *reinterpret_cast<const float4*>(lg + col * Cfg::GS + 8 * r + 4);
    BV ga[2];
    {
      uint32_t h[4], l[4];
      split2_f16(g0.x, g0.y, gs, h[0], l[0]);
      split2_f16(g0.z, g0.w, gs, h[1], l[1]);
      split2_f16(g1.x, g1.y, gs, h[2], l[2]);
      split2_f16(g1.z, g1.w, gs, h[3], l[3]);
      ga[0].u = make_uint4(h[0], h[1], h[2], h[3]);
      ga[1].u = make_uint4(l[0], l[1], l[2], l[3]);
    }
    BV xb[NQ][2];
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const float* __restrict__ xp = lx + colofs[q] + base;
      uint32_t h[4], l[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) split2_f16(xp[(2 * j) * S], xp[(2 * j + 1) * S], xs, h[j], l[j]);
      xb[q][0].u = make_uint4(h[0], h[1], h[2], h[3]);
      xb[q][1].u = make_uint4(l[0], l[1], l[2], l[3]);
    }
    SF16_TERMS(acc, 0, NQ, ga, xb)
  }
}

template <int S>
__global__ __launch_bounds__(256) void conv3d_wgrad_sf16_kernel(const float* __restrict__ g, const float* __restrict__ xin,
                                                                const float* __restrict__ g_bound, const float* __restrict__ x_bound,
                                                                float* __restrict__ dw, int B, int Ca, int Cb, int Do, int Ho, int Wo,
                                                                int Di, int Hi, int Wi, int tiles_x, int tiles_y, int ntiles,
                                                                int tiles_per_wg) {
  using Cfg = WsCfg<S>;
  __shared__ __attribute__((aligned(16))) float lg[16 * Cfg::GS];
  __shared__ __attribute__((aligned(16))) float lx[8 * Cfg::NI];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int col = lane & 15, kq = lane >> 4;
  const int a0 = blockIdx.y * 16, b0 = blockIdx.z * 8;
  const size_t vo = (size_t)Do * Ho * Wo, vi = (size_t)Di * Hi * Wi;
  const float gs = sf16_scale(g_bound[0]), xs = sf16_scale(x_bound[0]);
  const float ginv = 1.0f / gs, xinv = 1.0f / xs;
  constexpr int NBLK = 14, QW = 4;
  int colofs[QW];
#pragma unroll
  for (int q = 0; q < QW; ++q) {
    const int n = min((wave + 4 * q) * 16 + col, 8 * 27 - 1);
    const int bb = n / 27, tap = n - bb * 27;
    colofs[q] = bb * Cfg::NI + ((tap / 9) * Cfg::IY + (tap / 3) % 3) * Cfg::IX + tap % 3;
  }
  f32x4 acc[QW];
#pragma unroll
  for (int q = 0; q < QW; ++q) acc[q] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const int t0 = blockIdx.x * tiles_per_wg, t1 = min(ntiles * B, t0 + tiles_per_wg);
  constexpr int NG = (16 * Cfg::NO + 255) / 256, NX = (8 * Cfg::NI + 255) / 256;
  float rg[NG], rx[NX];
  int relg[NG], pkg[NG], relx[NX], pkx[NX];
#pragma unroll
  for (int e = 0; e < NG; ++e) {
    const int i = tid + 256 * e;
    const int ch = i / Cfg::NO, p = i - ch * Cfg::NO;
    const int px = p % Cfg::OX, py = (p / Cfg::OX) % Cfg::OY, pz = p / (Cfg::OX * Cfg::OY);
    relg[e] = ch * (int)vo + (pz * Ho + py) * Wo + px;
    pkg[e] = (i < 16 * Cfg::NO && a0 + ch < Ca) ? (px | (py << 8) | (pz << 16)) : -1;
  }
#pragma unroll
  for (int e = 0; e < NX; ++e) {
    const int i = tid + 256 * e;
    const int ch = i / Cfg::NI, p = i - ch * Cfg::NI;
    const int px = p % Cfg::IX, py = (p / Cfg::IX) % Cfg::IY, pz = p / (Cfg::IX * Cfg::IY);
    relx[e] = ch * (int)vi + (pz * Hi + py) * Wi + px;
    pkx[e] = (i < 8 * Cfg::NI && b0 + ch < Cb) ? (px | (py << 8) | (pz << 16)) : -1;
  }
  auto fetch = [&](int tile) {
    const int bi = tile / ntiles;
    int r = tile - bi * ntiles;
    const int tx_i = r % tiles_x;
    r /= tiles_x;
    const int ty_i = r % tiles_y, tz_i = r / tiles_y;
    const int ox0 = tx_i * Cfg::OX, oy0 = ty_i * Cfg::OY, oz0 = tz_i * Cfg::OZ;
    const float* __restrict__ gt = g + ((size_t)bi * Ca + a0) * vo + ((size_t)oz0 * Ho + oy0) * Wo + ox0;
    const int ix0 = ox0 * S - 1, iy0 = oy0 * S - 1, iz0 = oz0 * S - 1;
    const long long xbase = (long long)(((size_t)bi * Cb + b0) * vi) + ((long long)iz0 * Hi + iy0) * Wi + ix0;
#pragma unroll
    for (int e = 0; e < NG; ++e) {
      const int pk = pkg[e];
      const bool ok = pk >= 0 && ox0 + (pk & 255) < Wo && oy0 + ((pk >> 8) & 255) < Ho && oz0 + (pk >> 16) < Do;
      const float v = gt[ok ? relg[e] : 0];
      rg[e] = ok ? v : 0.f;
    }
#pragma unroll
    for (int e = 0; e < NX; ++e) {
      const int pk = pkx[e];
      const bool ok = pk >= 0 && (unsigned)(ix0 + (pk & 255)) < (unsigned)Wi && (unsigned)(iy0 + ((pk >> 8) & 255)) < (unsigned)Hi &&
                      (unsigned)(iz0 + (pk >> 16)) < (unsigned)Di;
      const float v = xin[ok ? xbase + relx[e] : 0];
      rx[e] = ok ? v : 0.f;
    }
  };
  if (t0 < t1) fetch(t0);
  for (int tile = t0; tile < t1; ++tile) {
    __syncthreads();
#pragma unroll
    for (int e = 0; e < NG; ++e) {
      const int i = tid + 256 * e;
      if (i < 16 * Cfg::NO) lg[(i / Cfg::NO) * Cfg::GS + i % Cfg::NO] = rg[e];
    }
#pragma unroll
    for (int e = 0; e < NX; ++e) {
      const int i = tid + 256 * e;
      if (i < 8 * Cfg::NI) lx[i] = rx[e];
    }
    __syncthreads();
    if (tile + 1 < t1) fetch(tile + 1);
    if (wave + 4 * (QW - 1) < NBLK)
      wgrad_sf16_ksteps<Cfg, S, QW>(lg, lx, col, kq, colofs, gs, xs, acc);
    else
      wgrad_sf16_ksteps<Cfg, S, QW - 1>(lg, lx, col, kq, colofs, gs, xs, acc);
  }
#pragma unroll
  for (int q = 0; q < QW; ++q) {
    const int n = (wave + 4 * q) * 16 + col;
    if (wave + 4 * q >= NBLK || n >= 8 * 27) continue;
    const int bb = n / 27, tap = n - bb * 27;
    if (b0 + bb >= Cb) continue;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int a = a0 + 4 * kq + e;
      if (a < Ca) atomicAdd(&dw[((size_t)a * Cb + b0 + bb) * 27 + tap], (acc[q][e] * ginv) * xinv);
    }
  }
}

template <int S, int TZ, bool TR, int MB>
void launch_conv_sf16(const float* x, const _Float16* wpk, const float* w_inv, const float* x_bound, float* y, int B, int C, int M,
                      int Di, int Hi, int Wi, int Do, int Ho, int Wo, hipStream_t st) {
  using Cfg = SfCfg<S, TZ, TR>;
  const int gx = TR ? Wi : Wo, gy = TR ? Hi : Ho, gz = TR ? Di : Do;     // the tiled grid
  const int tx = cds_ceil_div(gx, Cfg::TX), ty = cds_ceil_div(gy, Cfg::TY), tz = cds_ceil_div(gz, TZ);
  hipLaunchKernelGGL((conv3d_sf16_train_kernel<S, TZ, TR, MB>), dim3(tx * ty * tz, B, TR ? 8 : 1), dim3(256), 0, st, x, wpk, w_inv,
                     x_bound, y, C, M, Di, Hi, Wi, Do, Ho, Wo, tx, ty);
}

template <int MB>
void launch_conv_sf16_mode(const float* x, const _Float16* w, const float* w_inv, const float* x_bound, float* y, int B, int C, int M,
                           int Di, int Hi, int Wi, int mode, hipStream_t st) {
  if (mode == 0) {
    launch_conv_sf16<1, 4, false, MB>(x, w, w_inv, x_bound, y, B, C, M, Di, Hi, Wi, Di, Hi, Wi, st);
  } else if (mode == 1) {
    launch_conv_sf16<2, 2, false, MB>(x, w, w_inv, x_bound, y, B, C, M, Di, Hi, Wi, (Di - 1) / 2 + 1, (Hi - 1) / 2 + 1, (Wi - 1) / 2 + 1,
                                      st);
  } else {
    launch_conv_sf16<2, 4, true, MB>(x, w, w_inv, x_bound, y, B, C, M, Di, Hi, Wi, 2 * Di, 2 * Hi, 2 * Wi, st);
  }
}

}  // namespace

extern "C" int cds_absmax_bound_f32(const float* x, long long n, float* bound, void* stream) {
  if (!x || !bound || n < 1) return CDS_EINVAL;
  size_t blocks = ((size_t)n + 256 * 16 - 1) / (256 * 16);
  if (blocks > 512) blocks = 512;
  hipLaunchKernelGGL(absmax_bound_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x, (size_t)n, bound);
  return cds_launch_status();
}

extern "C" int cds_sf16_pack_conv3d_f32(const float* w, void* fwd, void* dgrad, float* w_inv, int A, int B, int mode, void* stream) {
  if (!w || !w_inv || (!fwd && !dgrad) || A < 1 || B < 1 || mode < 0 || mode > 2 || (A & 7) || (B & 7) || A > 64 || B > 64)
    return CDS_EINVAL;
  // items of both operands: (C / 8) 28 Mpad each, at most 2 x 8 x 28 x 64; about eight per thread
  const int items = 2 * (A / 8 > B / 8 ? A / 8 : B / 8) * SF_TAPS * 64;
  int wgs = cds_ceil_div(items, 256 * 8);
  if (wgs < 1) wgs = 1;
  hipLaunchKernelGGL(sf16_pack_conv3d_kernel, dim3(wgs), dim3(256), 0, (hipStream_t)stream, w, A, B, mode, (_Float16*)fwd,
                     (_Float16*)dgrad, w_inv);
  return cds_launch_status();
}

extern "C" int cds_conv3d_k3_sf16_f32(const float* x, const void* wpk, const float* w_inv, const float* x_bound, float* y, int B, int C,
                                      int M, int Di, int Hi, int Wi, int mode, void* stream) {
  if (!x || !wpk || !w_inv || !x_bound || !y || B < 1 || C < 8 || (C & 7) || M < 1 || M > 64 || Di < 1 || Hi < 1 || Wi < 1 ||
      mode < 0 || mode > 2)
    return CDS_EINVAL;
  const hipStream_t st = (hipStream_t)stream;
  const _Float16* w = (const _Float16*)wpk;
  switch ((M + 15) / 16) {                                             // the pack's Mpad = 16 MB
    case 1: launch_conv_sf16_mode<1>(x, w, w_inv, x_bound, y, B, C, M, Di, Hi, Wi, mode, st); break;
    case 2: launch_conv_sf16_mode<2>(x, w, w_inv, x_bound, y, B, C, M, Di, Hi, Wi, mode, st); break;
    case 3: launch_conv_sf16_mode<3>(x, w, w_inv, x_bound, y, B, C, M, Di, Hi, Wi, mode, st); break;
    default: launch_conv_sf16_mode<4>(x, w, w_inv, x_bound, y, B, C, M, Di, Hi, Wi, mode, st); break;
  }
  return cds_launch_status();
}

extern "C" int cds_conv3d_wgrad_sf16_f32(const float* g, const float* xin, const float* g_bound, const float* x_bound, float* dw, int B,
                                         int Ca, int Cb, int Do, int Ho, int Wo, int Di, int Hi, int Wi, int stride, void* stream) {
  if (!g || !xin || !g_bound || !x_bound || !dw || B < 1 || Ca < 1 || Cb < 1 || Do < 1 || Ho < 1 || Wo < 1 || Di < 1 || Hi < 1 ||
      Wi < 1 || (stride != 1 && stride != 2))
    return CDS_EINVAL;
  const int tx = cds_ceil_div(Wo, 8), ty = cds_ceil_div(Ho, 4), tz = cds_ceil_div(Do, 4);
  const int ntiles = tx * ty * tz;
  int per = cds_ceil_div(ntiles * B * cds_ceil_div(Ca, 16) * cds_ceil_div(Cb, 8), cds_env_int("CDS_WG3_WGS", 512));
  if (per < 1) per = 1;
  const dim3 gm(cds_ceil_div(ntiles * B, per), cds_ceil_div(Ca, 16), cds_ceil_div(Cb, 8));
  if (stride == 1)
    hipLaunchKernelGGL(conv3d_wgrad_sf16_kernel<1>, gm, dim3(256), 0, (hipStream_t)stream, g, xin, g_bound, x_bound, dw, B, Ca, Cb, Do,
                       Ho, Wo, Di, Hi, Wi, tx, ty, ntiles, per);
  else
    hipLaunchKernelGGL(conv3d_wgrad_sf16_kernel<2>, gm, dim3(256), 0, (hipStream_t)stream, g, xin, g_bound, x_bound, dw, B, Ca, Cb, Do,
                       Ho, Wo, Di, Hi, Wi, tx, ty, ntiles, per);
  return cds_launch_status();
}
