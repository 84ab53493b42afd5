// K4: ConvTranspose3d k3 s2 p1 op1 (+ folded BN shift, ReLU, U-Net residual; models/module.py:125-160, :310-312) to Cout = 16 with
// Cin = 32 - conv9 of CostRegNet - as a z-marching, class-per-wave kernel in split-bf16 arithmetic.
//
// Output voxel o = 2 a + p per axis: parity 0 takes kernel tap 1 of input cell a, parity 1 takes tap 2 of cell a and tap 0 of cell
// a + 1.  The 8 parity classes (pz, py, px) are 8 small convolutions over the SAME 2 x 2 x 2 cell neighbourhood with different
// weights, so (1) a class is given to one consumer wave, which keeps ALL its weights in registers for the whole march (4 rounds x
// 1 or 2 matrix operands: nothing but input cells is read from LDS in the loop), and (2) the K-steps are organised by cell offset,
// not by class: K-slot g = (dy, dx) of a 32-deep K-step at dz = 0, a second K-step at dz = 1 for the pz = 1 classes; slots a class
// does not use carry zero weights (12 MFMA K-steps per round over the 8 classes instead of 9, 2 operand reads per round and
// N-tile instead of 9: the tiled kernel this replaces ran its matrix pipe at 20 %).
// A workgroup owns a column of 16 x 8 input cells and marches along z over a ring of three input cell planes in LDS (all four
// 8-channel rounds of a plane resident, exact three-way bf16 split done by the 4 producer waves on the way in): one barrier per cell
// plane; every input cell is read from HBM once per column (+ the one-cell halo on the high sides).  Each SIMD holds one pz = 0 and
// one pz = 1 consumer wave (1 : 2 matrix work) and a producer.
#include "zm_common.hpp"

namespace {

template <int ROUNDS_, int TY_ = 8>
struct DZC {
  static constexpr int ROUNDS = ROUNDS_;
  static constexpr int TX = 16, TY = TY_;               // cells per plane: one N-tile per cell row
  static constexpr int IX = TX + 1, IY = TY + 1, IXP = 18;
  static constexpr int ROUNDB = IY * IXP * POSB;
  static constexpr int SLOTB = ROUNDS * ROUNDB;         // one input cell plane: [round][row][col][term][8] bf16
  static constexpr int NSLOT = 3;
  static constexpr int CW = 8, PW = 4, THREADS = (CW + PW) * 64;
  static constexpr int LDS = NSLOT * SLOTB;
  static constexpr int NITEM = IY * IX * ROUNDS;
};

// The producer waves of a column (X0, Y0) marching over the cell planes [a0, a1): load, split and deposit plane a + 2 while the
// consumers work on planes a and a + 1; out-of-volume cells are zeros.  One barrier per cell plane, matched by the consumers.
template <class C, bool F16>
__device__ __forceinline__ void dzm_produce(const float* __restrict__ x, unsigned char* lds, int ptid, int X0, int Y0, int D, int H, int W,
                                            int a0, int a1, float xs) {
  __builtin_amdgcn_s_setprio(3);               // A/B at M1: producers at 0 / 1 / 3: 355 / 351 / 345 us
  ZmCellStage<C, C::PW * 64, F16, false> stage;
  stage.init(ptid, X0, Y0, H, W);
  auto issue = [&](int plane) { stage.issue(x, plane, D, H, W); };
  auto deposit = [&](int plane) { stage.deposit(lds + (plane % C::NSLOT) * C::SLOTB, xs); };
  issue(a0);
  deposit(a0);
  issue(a0 + 1);
  deposit(a0 + 1);
  issue(a0 + 2);
  __syncthreads();                                  // #0: planes a0, a0 + 1 staged
  for (int a = a0; a < a1; ++a) {
    deposit(a + 2);                                 // slot of plane a - 1, which nobody reads any more
    issue(a + 3);
    __syncthreads();
  }
}

// F16: split-f16 arithmetic (sbf_common.hpp): two fp16 terms, three products per K-step, tensor scales from device bounds.
// BAL: the balanced cutting (zm_common.hpp): the workgroup walks the pieces of its range, one march each; the weights, the bias and
// the running bound stay, what follows from the column is set up again for every piece.
template <int ROUNDS, bool F16, bool BAL>
__global__ __launch_bounds__((DZC<ROUNDS>::THREADS), 3) void deconv3d_zm_kernel(
    const float* __restrict__ x, const uint4* __restrict__ wcls, const float* __restrict__ bias, const float* __restrict__ skip,
    float* __restrict__ out, int D, int H, int W, int tiles_x, int ncols, int seg_len, int act, const float* __restrict__ in_bound,
    float w_inv, float* __restrict__ out_bound) {
  using C = DZC<ROUNDS>;
  constexpr int NT = F16 ? 2 : 3;
  const float xs = F16 ? sf16_scale(in_bound[0]) : 1.0f;
  const float out_mul = F16 ? w_inv / xs : 1.0f;
  constexpr int Cout = 16;
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  ZmWalk<BAL> walk(ncols, D, seg_len, ZM_MINLEN_CELL);
  if (walk.empty()) return;
  const int Ho = 2 * H, Wo = 2 * W;

  if (wave >= C::CW) {
    do {
      const ZmColumn zc = walk.column(tiles_x);
      dzm_produce<C, F16>(x, lds, tid - C::CW * 64, zc.tx_i * C::TX, zc.ty_i * C::TY, D, H, W, zc.a0, zc.a1, xs);
    } while (BAL && walk.next_piece());
    return;
  }

  // ============================== consumers: wave = parity class ==============================
  const int pz = wave >> 2, py = (wave >> 1) & 1, px = wave & 1;
  if (pz) __builtin_amdgcn_s_setprio(1);         // twice the matrix work of its pz = 0 SIMD neighbour: 345 -> 329 us at M1
  const int j = lane & 15, g = lane >> 4;
  BV wlo[ROUNDS][3], whi[ROUNDS][3];                  // this class's weights: K-step at dz = 0 and (pz = 1) at dz = 1
  {
    const uint4* __restrict__ wp = wcls + (size_t)wave * ROUNDS * 2 * 3 * 64 + lane;
#pragma unroll
    for (int rd = 0; rd < ROUNDS; ++rd)
#pragma unroll
      for (int k = 0; k < NT; ++k) {
        wlo[rd][k].u = wp[((rd * 2 + 0) * 3 + k) * 64];
        whi[rd][k].u = wp[((rd * 2 + 1) * 3 + k) * 64];
      }
  }
  const float4 bv = bias ? *reinterpret_cast<const float4*>(bias + 4 * g) : make_float4(0.f, 0.f, 0.f, 0.f);
  const int b_off = (((g >> 1) * C::IXP) + j + (g & 1)) * POSB;       // slot g = (dy, dx)
  const size_t zstride = (size_t)Ho * Wo * Cout;
  float amax = 0.f;                                   // split-f16: running maximum of the magnitudes this lane stores
  do {
  const ZmColumn zc = walk.column(tiles_x);
  const int a0 = zc.a0, a1 = zc.a1;
  const int X0 = zc.tx_i * C::TX, Y0 = zc.ty_i * C::TY;
  const int xv = 2 * (X0 + j) + px;
  const bool x_ok = X0 + j < W;
  __syncthreads();                                    // #0
  for (int a = a0; a < a1; ++a) {
    const unsigned char* lo = lds + (a % C::NSLOT) * C::SLOTB + b_off;
    const unsigned char* hi = lds + ((a + 1) % C::NSLOT) * C::SLOTB + b_off;
    const size_t zbase = (size_t)(2 * a + pz) * zstride;
    const int nrows = min(C::TY, H - Y0);
    float4 skn = make_float4(0.f, 0.f, 0.f, 0.f);
    auto row_off = [&](int n) { return ((size_t)(2 * (Y0 + n) + py) * Wo + xv) * Cout + 4 * g; };
    if (skip && x_ok) skn = *reinterpret_cast<const float4*>(skip + zbase + row_off(0));
    asm volatile("" ::"v"(skn.x), "v"(skn.y), "v"(skn.z), "v"(skn.w));   // (the row loop's head then joins two states without pending loads)
    for (int n = 0; n < nrows; ++n) {
      const float4 sk = skn;
      if (skip && x_ok && n + 1 < nrows) skn = *reinterpret_cast<const float4*>(skip + zbase + row_off(n + 1));
      f32x4 acc[1] = {F16 ? (f32x4){0.f, 0.f, 0.f, 0.f} : (f32x4){bv.x, bv.y, bv.z, bv.w}};
      const unsigned char* lo_n = lo + n * C::IXP * POSB;
      const unsigned char* hi_n = hi + n * C::IXP * POSB;
#pragma unroll
      for (int rd = 0; rd < ROUNDS; ++rd) {
        BV b[1][3];
        b[0][0].u = *reinterpret_cast<const uint4*>(lo_n + rd * C::ROUNDB);
        b[0][1].u = *reinterpret_cast<const uint4*>(lo_n + rd * C::ROUNDB + 16);
        if constexpr (F16) {
          SF16_TERMS(acc, 0, 1, wlo[rd], b);
        } else {
          b[0][2].u = *reinterpret_cast<const uint4*>(lo_n + rd * C::ROUNDB + 32);
          SBF_TERMS(acc, 0, 1, wlo[rd], b);
        }
        if (pz) {
          BV c[1][3];
          c[0][0].u = *reinterpret_cast<const uint4*>(hi_n + rd * C::ROUNDB);
          c[0][1].u = *reinterpret_cast<const uint4*>(hi_n + rd * C::ROUNDB + 16);
          if constexpr (F16) {
            SF16_TERMS(acc, 0, 1, whi[rd], c);
          } else {
            c[0][2].u = *reinterpret_cast<const uint4*>(hi_n + rd * C::ROUNDB + 32);
            SBF_TERMS(acc, 0, 1, whi[rd], c);
          }
        }
      }
      // the next row's residual is taken delivery of BEFORE this row's store is issued (gfx9: one vmcnt for loads and stores, out of
      // order with respect to each other -> a wait for a load with a younger store in flight is a full drain)
      asm volatile("" ::"v"(skn.x), "v"(skn.y), "v"(skn.z), "v"(skn.w));
      if (x_ok) {
        float4 o = F16 ? sf16_rescale4(acc[0], out_mul, bv) : sbf_f4(acc[0]);   // split-bf16: the bias rode in the accumulator
        if (act == CDS_ACT_RELU) o = sbf_relu4(o);
        if (skip) o = sbf_add4(sk, o);
        if (F16) amax = sbf_amax4(amax, o);
        sbf_store4(out + zbase + row_off(n), o);
      }
    }
    __syncthreads();
  }
  } while (BAL && walk.next_piece());
  if (F16) sf16_publish_bound(amax, out_bound);
}


// conv7 of CostRegNet: the same transposed convolution at 64 -> 32 (+ BN shift, ReLU, residual), split-f16 only, as a sibling of the
// kernel above.  What differs: (1) the matrix operand is the tiled kernel's (ops.split_pack_deconv3d(w, f16=True), DTab<false> in
// conv3d_sbf.hip: 9 K-steps per round, K-slot g of class c = its g-th tap in (dz, dy, dx) order, so the lane groups of one K-step read
// different cell offsets INCLUDING dz; class 7 alone has a second K-step, its four dz = 1 taps), so the model keeps one packing of the
// layer for both kernels; (2) a column is 16 x 4 cells with all eight rounds resident (3 x 34 560 B of LDS); (3) the two 16-cout blocks
// are two workgroups of a column (gridDim.y): a wave's weights are 8 rounds x 2 terms x 4 = 64 VGPRs, 128 for class 7 - both blocks in
// one workgroup would be 256 for that wave.  The column's input is then staged twice, the second time from L2 / the memory-side cache.
constexpr int DZM64_W1L = 2;                          // rounds of class 7's second operand kept in LDS (1 KB per round and term)
template <bool BAL>
__global__ __launch_bounds__((DZC<8, 4>::THREADS), 3) void deconv3d_zm64_kernel(
    const float* __restrict__ x, const uint4* __restrict__ wsp, const float* __restrict__ bias, const float* __restrict__ skip,
    float* __restrict__ out, int D, int H, int W, int tiles_x, int ncols, int seg_len, int act, const float* __restrict__ in_bound,
    float w_inv, float* __restrict__ out_bound) {
  using C = DZC<8, 4>;
  constexpr int ROUNDS = 8, Cout = 32, NKS = 9, W1L = DZM64_W1L;
  const float xs = sf16_scale(in_bound[0]);
  const float out_mul = w_inv / xs;
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  ZmWalk<BAL> walk(ncols, D, seg_len, ZM_MINLEN_CELL);
  if (walk.empty()) return;
  const int mbtot = gridDim.y, mb0 = blockIdx.y;      // this workgroup's 16-cout block
  const int Ho = 2 * H, Wo = 2 * W;

  if (wave >= C::CW) {
    do {
      const ZmColumn zc = walk.column(tiles_x);
      dzm_produce<C, true>(x, lds, tid - C::CW * 64, zc.tx_i * C::TX, zc.ty_i * C::TY, D, H, W, zc.a0, zc.a1, xs);
    } while (BAL && walk.next_piece());
    return;
  }

  // ============================== consumers: wave = parity class ==============================
  const int pz = wave >> 2, py = (wave >> 1) & 1, px = wave & 1;
  const bool two = wave == 7;                         // the class with eight taps: a second K-step per round
  if (two) __builtin_amdgcn_s_setprio(1);
  const int j = lane & 15, g = lane >> 4;
  // K-step `wave` of every round; class 7: and K-step 8, whose last W1L rounds wait in LDS behind the ring (written and read by this
  // wave alone): with all 128 weight registers the wave spilled 10 VGPRs at the 168 that three waves per SIMD leave it
  BV w0[ROUNDS][2], w1[ROUNDS - W1L][2];
  unsigned char* w1l = lds + C::LDS + lane * 16;
  {
    const uint4* __restrict__ wp = wsp + lane;
#pragma unroll
    for (int rd = 0; rd < ROUNDS; ++rd)
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        w0[rd][k].u = wp[(size_t)(((rd * NKS + wave) * mbtot + mb0) * 3 + k) * 64];
        const uint4 v = wp[(size_t)(((rd * NKS + (two ? 8 : wave)) * mbtot + mb0) * 3 + k) * 64];
        if (rd < ROUNDS - W1L) w1[rd][k].u = v;
        else if (two) *reinterpret_cast<uint4*>(w1l + ((rd - (ROUNDS - W1L)) * 2 + k) * 1024) = v;
      }
  }
  const float4 bv = bias ? *reinterpret_cast<const float4*>(bias + mb0 * 16 + 4 * g) : make_float4(0.f, 0.f, 0.f, 0.f);
  // tap slot g of this class -> cell offset (DTab<false>::tap_d); a slot past the class's taps has zero weights and reads offset 0.
  // Class 7's second K-step is its first one a cell plane up.
  const int ny = 1 + py, nx = 1 + px;
  const bool live = g < (1 + pz) * ny * nx;
  const int dz = live ? g / (ny * nx) : 0, dy = live ? (g / nx) % ny : 0, dx = live ? g % nx : 0;
  const int b_off = ((dy * C::IXP) + j + dx) * POSB;
  const size_t zstride = (size_t)Ho * Wo * Cout;
  float amax = 0.f;                                   // running maximum of the magnitudes this lane stores
  do {
  const ZmColumn zc = walk.column(tiles_x);
  const int a0 = zc.a0, a1 = zc.a1;
  const int X0 = zc.tx_i * C::TX, Y0 = zc.ty_i * C::TY;
  const int xv = 2 * (X0 + j) + px;
  const bool x_ok = X0 + j < W;
  const int nrows = min(C::TY, H - Y0);
  __syncthreads();                                    // #0
  for (int a = a0; a < a1; ++a) {
    const unsigned char* p0 = lds + (a % C::NSLOT) * C::SLOTB + b_off;
    const unsigned char* hi = lds + ((a + 1) % C::NSLOT) * C::SLOTB + b_off;
    const unsigned char* lo = dz ? hi : p0;
    const size_t zbase = (size_t)(2 * a + pz) * zstride;
    float4 skn = make_float4(0.f, 0.f, 0.f, 0.f);
    auto row_off = [&](int n) { return ((size_t)(2 * (Y0 + n) + py) * Wo + xv) * Cout + mb0 * 16 + 4 * g; };
    if (skip && x_ok) skn = *reinterpret_cast<const float4*>(skip + zbase + row_off(0));
    asm volatile("" ::"v"(skn.x), "v"(skn.y), "v"(skn.z), "v"(skn.w));   // (see the row loop of the kernel above)
    for (int n = 0; n < nrows; ++n) {
      const float4 sk = skn;
      if (skip && x_ok && n + 1 < nrows) skn = *reinterpret_cast<const float4*>(skip + zbase + row_off(n + 1));
      f32x4 acc[1] = {(f32x4){0.f, 0.f, 0.f, 0.f}};
      const unsigned char* lo_n = lo + n * C::IXP * POSB;
      const unsigned char* hi_n = hi + n * C::IXP * POSB;
#pragma unroll
      for (int rd = 0; rd < ROUNDS; ++rd) {
        BV b[1][2];
        b[0][0].u = *reinterpret_cast<const uint4*>(lo_n + rd * C::ROUNDB);
        b[0][1].u = *reinterpret_cast<const uint4*>(lo_n + rd * C::ROUNDB + 16);
        SF16_TERMS(acc, 0, 1, w0[rd], b);
        if (two) {
          BV c[1][2];
          c[0][0].u = *reinterpret_cast<const uint4*>(hi_n + rd * C::ROUNDB);
          c[0][1].u = *reinterpret_cast<const uint4*>(hi_n + rd * C::ROUNDB + 16);
          if (rd < ROUNDS - W1L) {
            SF16_TERMS(acc, 0, 1, w1[rd < ROUNDS - W1L ? rd : 0], c);
          } else {
            BV wl[2];
            wl[0].u = *reinterpret_cast<const uint4*>(w1l + ((rd - (ROUNDS - W1L)) * 2 + 0) * 1024);
            wl[1].u = *reinterpret_cast<const uint4*>(w1l + ((rd - (ROUNDS - W1L)) * 2 + 1) * 1024);
            SF16_TERMS(acc, 0, 1, wl, c);
          }
        }
      }
      asm volatile("" ::"v"(skn.x), "v"(skn.y), "v"(skn.z), "v"(skn.w));   // the next row's residual arrives before this row's store
      if (x_ok) {
        float4 o = sf16_rescale4(acc[0], out_mul, bv);
        if (act == CDS_ACT_RELU) o = sbf_relu4(o);
        if (skip) o = sbf_add4(sk, o);
        amax = sbf_amax4(amax, o);
        sbf_store4(out + zbase + row_off(n), o);
      }
    }
    __syncthreads();
  }
  } while (BAL && walk.next_piece());
  sf16_publish_bound(amax, out_bound);
}

}  // namespace

// conv7 (ConvTranspose3d 64 -> 32, channels-last, split-f16) for cds_deconv3d_sf16_f32 (conv3d_sbf.hip): CDS_ZMG_UNSUPPORTED when the
// volume stays on the tiled kernel.  CDS_DZM_DEEP (A/B knob, like CDS_ZMG_DEEP): 0 = tiled kernel, 1 = z-march where columns x
// segments x cout blocks fill the 256 CUs, 2 = z-march whatever the size.
int cds_deconv3d_zm64_dispatch(const float* x, const void* wsp, const float* bias, const float* skip, float* out, int Cin, int Cout,
                               int D, int H, int W, int act, hipStream_t st, const float* in_bound, float w_inv, float* out_bound) {
  const int deep = cds_env_int("CDS_DZM_DEEP", 1);
  if (deep <= 0 || Cin != 64 || Cout != 32 || !in_bound) return CDS_ZMG_UNSUPPORTED;
  if ((long)2 * H * 2 * W * Cout >= (1l << 31) || (long)H * W * Cin >= (1l << 31)) return CDS_ZMG_UNSUPPORTED;   // 32-bit in-plane offsets
  using C = DZC<8, 4>;
  const int tiles_x = cds_ceil_div(W, C::TX), tiles_y = cds_ceil_div(H, C::TY);
  const int ncols = tiles_x * tiles_y;
  double ucost;
  const int seg_len = cds_ceil_div(D, zm_pick_nseg(ncols * 2, D, 24, "CDS_DZM_NSEG", &ucost));
  const int nseg = cds_ceil_div(D, seg_len);
  if (deep == 1 && ncols * nseg * 2 < 256) return CDS_ZMG_UNSUPPORTED;
  // balanced: each of the two cout blocks (gridDim.y) is cut over half of the CUs, so a workgroup keeps its block's weights
  const int nwg = max(1, zm_ncu() / 2);
  const bool bal = zm_choose_balanced(zm_balance_knob(), ucost, ncols, D, nwg, ZM_MINLEN_CELL, 1.5);
  auto launch = [&](auto b) {
    return cds_launch_lds<deconv3d_zm64_kernel<decltype(b)::value>>(
        160 * 1024, dim3(b ? nwg : ncols * nseg, 2), dim3(C::THREADS), C::LDS + DZM64_W1L * 2 * 1024, st, x,
        reinterpret_cast<const uint4*>(wsp), bias, skip, out, D, H, W, tiles_x, ncols, seg_len, act, in_bound, w_inv, out_bound);
  };
  return bal ? launch(std::true_type()) : launch(std::false_type());
}

// ConvTranspose3d k3 s2 p1 op1 (+bias +ReLU +residual) 32 -> 16 in split-bf16 arithmetic, channels-last: x [D][H][W][32] ->
// out [2D][2H][2W][16]; weight_cls from ops.split_pack_deconv_cls (int16 [8 classes][4 rounds][2][3][64][8]).
static int dzm_entry(const float* x, const void* weight_cls, const float* bias, const float* skip, float* out, int Cin, int Cout, int D,
                     int H, int W, int act, const float* in_bound, float w_inv, float* out_bound, void* stream) {
  if (!x || !weight_cls || !out || Cin != 32 || Cout != 16 || D < 1 || H < 1 || W < 1) return CDS_EINVAL;
  if ((long)2 * H * 2 * W * Cout >= (1l << 31) || (long)H * W * Cin >= (1l << 31)) return CDS_EINVAL;   // in-plane offsets are 32-bit
  using C = DZC<4>;
  hipStream_t st = (hipStream_t)stream;
  const int tiles_x = cds_ceil_div(W, C::TX), tiles_y = cds_ceil_div(H, C::TY);
  const int ncols = tiles_x * tiles_y;
  double ucost;
  const int seg_len = cds_ceil_div(D, zm_pick_nseg(ncols, D, 24, "CDS_DZM_NSEG", &ucost));
  const int nseg = cds_ceil_div(D, seg_len);
  const int nwg = zm_ncu();
  const bool bal = zm_choose_balanced(zm_balance_knob(), ucost, ncols, D, nwg, ZM_MINLEN_CELL, 1.5);
  // split-f16 where the caller gave the input's bound (the split-bf16 entry passes no bounds and w_inv = 1; its kernel reads none of them)
  auto launch = [&](auto f16, auto b) {
    return cds_launch_lds<deconv3d_zm_kernel<4, decltype(f16)::value, decltype(b)::value>>(
        160 * 1024, dim3(b ? nwg : ncols * nseg), dim3(C::THREADS), C::LDS, st, x, reinterpret_cast<const uint4*>(weight_cls), bias, skip,
        out, D, H, W, tiles_x, ncols, seg_len, act, in_bound, w_inv, out_bound);
  };
  if (bal) return in_bound ? launch(std::true_type(), std::true_type()) : launch(std::false_type(), std::true_type());
  return in_bound ? launch(std::true_type(), std::false_type()) : launch(std::false_type(), std::false_type());
}

// The cutting of zm_common.hpp for the tests, on the host (no GPU call).  cds_zm_partition: the pieces of workgroup wg as
// (column, first plane, one past the last plane) triples in out[3 * 8], a stage being `unit` planes of the `planes` of a column
// (conv3d_zmg: G output planes; the cell-plane kernels: 1); returns their number, which exceeds 8 where the layer keeps the uniform
// cutting (only the first 8 are then stored).  cds_zm_plan: what the host would run for a layer of `cols` columns of `planes`
// planes and ys cout splits (gridDim.y) on ncu workgroups under CDS_ZM_BALANCE = balance; family 0 = conv3d_zmg (stages of `unit`
// planes), 1 = the transposed convolutions (nseg cap 24), 2 = the fused tail (cap 16); out = {balanced?, segments of the uniform form, uniform cost, balanced
// cost} (costs in stages x 1000); returns 0.
extern "C" int cds_zm_partition(int cols, int planes, int unit, int nwg, int wg, int min_len, int* out) {
  if (cols < 1 || planes < 1 || unit < 1 || nwg < 1 || wg < 0 || wg >= nwg || min_len < 1 || !out) return CDS_EINVAL;
  ZmPiece pc[ZM_MAX_PIECES];
  const int n = zm_partition(cols, cds_ceil_div(planes, unit), nwg, wg, min_len, pc);
  for (int i = 0; i < min(n, ZM_MAX_PIECES); ++i) {
    out[3 * i] = pc[i].col;
    out[3 * i + 1] = pc[i].s0 * unit;
    out[3 * i + 2] = min(planes, pc[i].s1 * unit);
  }
  return n;
}
// the same for all nwg workgroups at once, up to cap pieces each: out[wg][1 + 3 cap] = {number of pieces, triples}
extern "C" int cds_zm_partition_all(int cols, int planes, int unit, int nwg, int min_len, int cap, int* out) {
  if (cols < 1 || planes < 1 || unit < 1 || nwg < 1 || min_len < 1 || cap < 1 || !out) return CDS_EINVAL;
  const int stages = cds_ceil_div(planes, unit);
  for (int wg = 0; wg < nwg; ++wg) {
    int* o = out + (size_t)wg * (1 + 3 * cap);
    const ZmRange r = zm_range(cols, stages, nwg, wg, min_len);
    int n = 0;
    for (int pos = r.lo; pos < r.hi; ++n) {
      const ZmPiece p = zm_piece_at(pos, r.hi, stages);
      if (n < cap) o[1 + 3 * n] = p.col, o[2 + 3 * n] = p.s0 * unit, o[3 + 3 * n] = min(planes, p.s1 * unit);
      pos = p.col * stages + p.s1;
    }
    o[0] = n;
  }
  return 0;
}
int cds_zmg_plan(int cols, int ys, int Do, int G, int ncu, int balance, int* nseg, double* ucost, double* bcost);   // conv3d_zmg.hip
extern "C" int cds_zm_plan(int family, int cols, int planes, int unit, int ys, int ncu, int balance, int* out) {
  if (family < 0 || family > 2 || cols < 1 || planes < 1 || unit < 1 || ys < 1 || ncu < 1 || !out) return CDS_EINVAL;
  int nseg = 0, bal = 0;
  double ucost = 0, bcost = 0;
  if (family == 0) {
    bal = cds_zmg_plan(cols, ys, planes, unit, ncu, balance, &nseg, &ucost, &bcost);
  } else {
    nseg = zm_pick_nseg(cols * ys, planes, family == 1 ? 24 : 16, "", &ucost);
    bal = zm_choose_balanced(balance, ucost, cols, planes, max(1, ncu / ys), ZM_MINLEN_CELL, 1.5, &bcost,
                             family == 2 ? ZM_BALANCE_MARGIN_TAIL : ZM_BALANCE_MARGIN);
  }
  out[0] = bal, out[1] = nseg, out[2] = (int)lrint(ucost * 1000), out[3] = (int)lrint(bcost * 1000);
  return 0;
}

extern "C" int cds_deconv3d_zm_f32(const float* x, const void* weight_cls, const float* bias, const float* skip, float* out,
                                   int Cin, int Cout, int D, int H, int W, int act, void* stream) {
  return dzm_entry(x, weight_cls, bias, skip, out, Cin, Cout, D, H, W, act, nullptr, 1.0f, nullptr, stream);
}

// The same layer in SPLIT-F16 arithmetic (sbf_common.hpp): weight_cls from ops.split_pack_deconv_cls(..., f16=True), w_inv_scale = 1 / its
// weight scale, in_bound a DEVICE scalar >= max |x|, out_bound a zeroed DEVICE scalar that receives max |out| (or NULL).
extern "C" int cds_deconv3d_zm_sf16_f32(const float* x, const void* weight_cls, const float* bias, const float* skip, float* out,
                                        int Cin, int Cout, int D, int H, int W, int act, const float* in_bound, float w_inv_scale,
                                        float* out_bound, void* stream) {
  if (!in_bound || !(w_inv_scale > 0.f)) return CDS_EINVAL;
  return dzm_entry(x, weight_cls, bias, skip, out, Cin, Cout, D, H, W, act, in_bound, w_inv_scale, out_bound, stream);
}
