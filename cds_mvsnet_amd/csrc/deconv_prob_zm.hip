// K4 tail, fused: conv11 (ConvTranspose3d 16 -> 8, k3 s2 p1 op1, BN folded, ReLU; models/module.py:125-160) + the conv0
// residual (models/module.py:498 `x = conv0 + self.conv11(x)`) + prob (Conv3d 8 -> 1, k3 p1, no bias; module.py:499), as ONE
// z-marching kernel: the full-resolution 8-channel volume between the two layers (2 x 2.0 GB of HBM traffic at 640x512x192)
// never leaves the CU.
//
// A workgroup owns a column of 30 x 6 input cells (60 x 12 output voxels) and walks it along z.  Per cell plane a it computes
// the transposed convolution on 32 x 8 cells (one cell of halo on every side: the prob convolution needs its neighbours' y)
// in split-bf16 arithmetic on the matrix cores, in two half-steps: output plane 2a (z parity 0: kernel tap kz = 1 of cell
// plane a) and output plane 2a + 1 (taps kz = 2 of plane a and kz = 0 of plane a + 1).  The consumer waves (one per cell row,
// two 16-cell N-tiles, rows of the matrix tile = (x parity, cout) as in deconv3d_sbf_ws_kernel) add bias, ReLU and the
// residual and write the finished plane as fp32 into an LDS double buffer; everything outside the volume is written as 0 (the
// zero padding of prob).  Four more waves - one per SIMD - (a) stage the next input cell plane (exact three-way bf16 split
// in registers, two plane slots in LDS) and (b) run the prob convolution on the plane finished in the half-step before, on the
// VALU in fp32 (plain v_fmac_f32 with the weight as a scalar operand): a lane owns one x column and three output rows, reads
// the 5 x 3 x 8-channel window of the new plane once and scatters it into the accumulators of output planes q - 1, q, q + 1
// (kz = 2, 1, 0); plane q - 1 is complete after that and is stored.  One workgroup barrier per half-step.
// Measured (profiles/r04_deconv_prob.md): 1120 us at 640x512x192 against 1656-1700 us for the two separate kernels; the prob
// waves are the critical path (648 FMAs per half-step and wave at ~6.8 cycles each beside the consumers' MFMAs).
//
// Operand sharing: the classes (z parity, y parity) of one half-step read the same input cells with different weights, so
// their B operands are loaded once: 3 operand reads per 8-channel round instead of the 5 of deconv3d_sbf_ws_kernel
//   half 1 (pz = 0): B1 = cells (dy, dx) in {0,1}^2 of plane a      -> A[0] (py = 0: dy = 1 slots are zero), A[1] (py = 1)
//   half 2 (pz = 1): B2 = cells (dz, dx) at dy = 0, B3 = at dy = 1  -> A[2] (py = 0) on B2; A[3] on B2 and A[4] on B3 (py = 1)
// with K-slot g = lane >> 4 of a 32-deep K-step = the cell offset, its 8 values = the 8 channels of the round.
//
// prob on the matrix cores (MF, split-f16 only; profiles/tail_prob_mfma.md): the consumers store y x s_y as two fp16 terms (32 B per
// voxel, the size of the fp32 plane), and the four prob waves run a GEMM over TAPS: one v_mfma_f32_16x16x32_f16 per (output row o,
// input row o + ky - 1, 16-wide x tile) with N = 16 x positions, K = [y_hi w_hi | y_lo w_hi | y_hi w_lo | spare] over the 8 channels
// and M row 4 kz' + kx = tap ((kz' + R) mod 3, ky, kx).  The three ky instructions chain in the accumulator; in the result lane group
// G holds kx = 0, 1, 2 of tap kz = (G + R) mod 3 at its x, so the kx sum is two DPP adds (row_shr:1, row_shl:1; lanes 2..13 of a tile
// are whole, tiles step by 12) and with R = (q + 1) mod 3 for y plane q group G always adds into the output plane p = q + 1 - kz with
// p = -G (mod 3): one accumulator register per (row, tile).  The group whose plane is complete stores it and clears.  Summation
// order: ky in the MFMA chain, kx centre / left / right, then the three planes in arrival order - independent of timing.
// y layout (MF): [row][term][x parity][slot = (x >> 1) ^ 8 (x & 1)][8 fp16]: the 16-byte operand reads of 16 consecutive x (even
// origin) touch 16 different 16-byte bank groups, the consumers' 8-byte stores (x = 2 j + px) are 2-way.
#include "zm_common.hpp"

namespace {

struct DPZ {
  static constexpr int CXC = 32, CYC = 8;            // computed cells per plane (halo included); one consumer wave per cell row
  static constexpr int CXR = CXC - 2, CYR = CYC - 2;  // owned cells
  static constexpr int NT = CXC / 16;
  static constexpr int IY = CYC + 1, IX = CXC + 1, IXP = 34;
  static constexpr int ROUNDS = 2;                   // Cin = 16
  static constexpr int ROUNDB = IY * IXP * POSB;
  static constexpr int SLOTB = ROUNDS * ROUNDB;      // one input cell plane: [round][row][col][term][8] bf16
  static constexpr int NA = 5;
  static constexpr int WB = ROUNDS * NA * 3 * 1024;  // split weights: [round][operand][term][lane] x 16 B
  static constexpr int YX = 2 * CXC, YY = 2 * CYC;
  static constexpr int YHALFB = YX * 16, YROWB = 2 * YHALFB;   // y plane: [row][channel half][x][4] fp32
  static constexpr int YB = YY * YROWB;
  static constexpr int CW = CYC, PW = 4, THREADS = (CW + PW) * 64;
  static constexpr int LDS = WB + 2 * SLOTB + 2 * YB;
  static constexpr int PR = 3;                       // output rows per prob lane: PW * PR = 2 * CYR
  static constexpr int NITEM = IY * IX * ROUNDS;     // (cell, round) staging items of one plane
  // prob on the matrix cores: x tiles of 16 read positions at origin MSTEP * t, whole outputs in lanes 2 .. 13
  static constexpr int MT = 5, MSTEP = 12;
  static constexpr int YTERMB = YROWB / 2, YPARB = YTERMB / 2;       // y plane: [row][term][x parity][slot][8] fp16
};
static_assert(DPZ::MT * DPZ::MSTEP == 2 * DPZ::CXR && (DPZ::MT - 1) * DPZ::MSTEP + 16 <= DPZ::YX, "prob x tiles");
static_assert(DPZ::PW * DPZ::PR == 2 * DPZ::CYR, "prob rows");
static_assert(DPZ::LDS <= 160 * 1024, "LDS budget");

// One v_fma_f32 with the (wave-uniform) weight as a scalar operand.  Written as an instruction because the compiler otherwise
// pairs adjacent channels into v_pk_fma_f32, and a packed fp32 instruction issued beside another wave's MFMAs costs far more
// than the two plain ones it replaces (measured here: 12-15 cycles per v_pk_fma_f32 in the prob waves).
__device__ __forceinline__ float dpz_fma(float d, float w, float acc) {
  asm("v_fmac_f32 %0, %1, %2" : "+v"(acc) : "s"(w), "v"(d));
  return acc;
}

// The value of the lane one to the left / right inside its row of 16 lanes (DPP row_shr:1 / row_shl:1); 0 where the row ends.
__device__ __forceinline__ float dpz_row_shr1(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x111, 0xF, 0xF, true));
}
__device__ __forceinline__ float dpz_row_shl1(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x101, 0xF, 0xF, true));
}

// F16: the transposed convolution in split-f16 arithmetic (sbf_common.hpp): two fp16 terms of x x (scale from the device bound in_bound),
// three products per K-step, exact rescaling before the BN shift; prob stays on the VALU in fp32 unless MF.
#define DPZ_TERMS(ACC, W, X)                                  \
  do {                                                        \
    if constexpr (F16) { SF16_TERMS(ACC, 0, C::NT, W, X); }   \
    else { SBF_TERMS(ACC, 0, C::NT, W, X); }                  \
  } while (0)
// MF: prob on the matrix cores (header comment).  pw is then the operand table of ops.split_pack_prob ([3 R][3 ky][64 lanes] x 16 B),
// p_inv 1 / its scale, and y is scaled by s_y from the bound skip_bound + y_gain * in_bound + max |bias| >= max |y|.
// BAL: the balanced cutting (zm_common.hpp): the workgroup walks the pieces of its range, one march each.  The LDS weight image, the
// prob waves' operands and the consumers' bias stay; the staging tables, the output and residual offsets, the border flag and the
// prob accumulators are set up again for every piece.
template <bool F16, bool MF, bool BAL>
__global__ __launch_bounds__(DPZ::THREADS, 3) void deconv_prob_zm_kernel(
    const float* __restrict__ x, const uint4* __restrict__ wsp, const float* __restrict__ bias, const float* __restrict__ skip,
    const float* __restrict__ pw, float* __restrict__ out, int D, int H, int W, int tiles_x, int ncols, int seg_len,
    const float* __restrict__ in_bound, float w_inv, const float* __restrict__ skip_bound, float y_gain, float p_inv) {
  static_assert(F16 || !MF, "the matrix-core prob form exists in split-f16 only");
  using C = DPZ;
  const float xs = F16 ? sf16_scale(in_bound[0]) : 1.0f;
  const float out_mul = F16 ? w_inv / xs : 1.0f;
  float ys = 1.0f;
  if constexpr (MF) {
    float bmax = 0.f;
    for (int i = 0; i < 8; ++i) bmax = fmaxf(bmax, fabsf(bias[i]));
    ys = sf16_scale(skip_bound[0] + y_gain * in_bound[0] + bmax);
  }
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  unsigned char* const inring = lds + C::WB;
  unsigned char* const ybuf = inring + 2 * C::SLOTB;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  ZmWalk<BAL> walk(ncols, D, seg_len, ZM_MINLEN_CELL);
  if (walk.empty()) return;
  const int Do = 2 * D, Ho = 2 * H, Wo = 2 * W;
  // what a march derives from its column and planes: set up by each branch for each of its pieces (set up once ahead of the branch
  // and updated between the pieces, the matrix-core form needs 8 more registers in the uniform cutting and spills in the balanced)
#define DPZ_PIECE()                                                                                               \
  const ZmColumn zc = walk.column(tiles_x);                                                                       \
  const int tx_i = zc.tx_i, ty_i = zc.ty_i, a0 = zc.a0, a1 = zc.a1;                                               \
  const int X0 = tx_i * C::CXR - 1, Y0 = ty_i * C::CYR - 1; /* first computed cell */                             \
  const int qs = a0 > 0 ? 2 * a0 - 1 : 0;                   /* first y plane this segment needs */                \
  const int qe = min(Do - 1, 2 * a1);                       /* last one */                                        \
  const int te = 2 * a1 + 1;                                /* last half-step */
  {
    uint4* wdst = reinterpret_cast<uint4*>(lds);
    for (int i = tid; i < C::WB / 16; i += C::THREADS) wdst[i] = wsp[i];
  }

  if (wave >= C::CW) {
    // ====================== producer / prob waves ======================
    __builtin_amdgcn_s_setprio(2);
    const int ptid = tid - C::CW * 64;
    // ---- staging of input cell planes ----
    ZmCellStage<C, C::PW * 64, F16, true> stage;    // (the prologue of a segment; inside the march the consumers stage)
    auto issue = [&](int plane) { stage.issue(x, plane, D, H, W); };
    auto deposit = [&](int plane) { stage.deposit(inring + (plane & 1) * C::SLOTB, xs); };
    if constexpr (MF) {
      // ---- prob on the matrix cores: wave = 3 output rows x MT x tiles; lane = (group g, read position n) ----
      const int n = lane & 15, g = lane >> 4, rg = wave - C::CW;
      const uint4* __restrict__ pwm = reinterpret_cast<const uint4*>(pw);
      BV wa[3][3];                                     // [rotation R][ky]
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) wa[r][ky].u = pwm[(r * 3 + ky) * 64 + lane];
      int b_off[C::MT];                                // operand byte offset inside a y row
#pragma unroll
      for (int t = 0; t < C::MT; ++t) {
        const int xl = C::MSTEP * t + n;               // y-plane x of this lane's read; its output is owned column xl - 2
        b_off[t] = (g & 1) * C::YTERMB + (xl & 1) * C::YPARB + (((xl >> 1) ^ ((xl & 1) << 3)) << 4);
      }
      const bool st_ok = g < 3 && n >= 2 && n <= 13;
      const float inv = p_inv / ys;
      float A[C::MT][C::PR];
      const int yrow0 = (C::PR * rg + 1) * C::YROWB;   // first of the PR + 2 input rows
      auto load_b = [&](BV (&b)[C::PR + 2], const unsigned char* yb, int t) {
#pragma unroll
        for (int rho = 0; rho < C::PR + 2; ++rho) b[rho].u = *reinterpret_cast<const uint4*>(yb + rho * C::YROWB + b_off[t]);
      };
      auto process = [&](int q, auto rc) {
        constexpr int R = decltype(rc)::value;
        const unsigned char* yb = ybuf + (q & 1) * C::YB + yrow0;
        BV b[2][C::PR + 2];
        load_b(b[0], yb, 0);
#pragma unroll
        for (int t = 0; t < C::MT; ++t) {
          if (t + 1 < C::MT) load_b(b[(t + 1) & 1], yb, t + 1);
          f32x4 d[C::PR];
#pragma unroll
          for (int r = 0; r < C::PR; ++r) {
            d[r] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ky = 0; ky < 3; ++ky) SF16_MFMA(d[r], wa[R][ky], b[t & 1][r + ky]);
          }
#pragma unroll
          for (int r = 0; r < C::PR; ++r) {
            float s = d[r][1] + dpz_row_shr1(d[r][0]);       // kx = 1 at x, kx = 0 from x - 1
            s = s + dpz_row_shl1(d[r][2]);                   // kx = 2 from x + 1
            A[t][r] = A[t][r] + s;
          }
        }
      };
      do {
      DPZ_PIECE()
      stage.init(ptid, X0, Y0, H, W);
      const int oy0 = ty_i * 2 * C::CYR + C::PR * rg;
      // outputs: tile t of row oy0 + r is element st_lane of the (wave-uniform) row pointer + MSTEP t, where x < Wo: MSTEP t < st_lim
      const int ox0 = tx_i * 2 * C::CXR + n - 2;
      const unsigned st_lane = st_ok ? oy0 * Wo + ox0 : 0;
      const int st_lim = st_ok ? Wo - ox0 : 0;
#pragma unroll
      for (int t = 0; t < C::MT; ++t)
#pragma unroll
        for (int r = 0; r < C::PR; ++r) A[t][r] = 0.f;
      const int ap = qs >> 1;
      issue(ap);
      deposit(ap);
      if (qs & 1) {
        issue(ap + 1);
        deposit(ap + 1);
      }
      __syncthreads();                            // #0
      for (int t = qs; t <= te; ++t) {
        const int q = t - 1;
        if (q >= qs && q <= qe) {
          const int R = (q + 1) % 3;
          if (R == 0) process(q, std::integral_constant<int, 0>());
          else if (R == 1) process(q, std::integral_constant<int, 1>());
          else process(q, std::integral_constant<int, 2>());
        }
        const int o = t - 2;                        // complete now; its owner is the lane group -o (mod 3)
        const bool own = g == (3 - (o + 3) % 3) % 3;
        if (o >= 2 * a0 && o < 2 * a1) {
          float* po = out + (size_t)o * Ho * Wo;
#pragma unroll
          for (int r = 0; r < C::PR; ++r)
            if (oy0 + r < Ho) {
#pragma unroll
              for (int tt = 0; tt < C::MT; ++tt)
                if (own && C::MSTEP * tt < st_lim) (po + r * Wo + C::MSTEP * tt)[st_lane] = A[tt][r] * inv;
            }
        }
#pragma unroll
        for (int tt = 0; tt < C::MT; ++tt)
#pragma unroll
          for (int r = 0; r < C::PR; ++r) A[tt][r] = own ? 0.f : A[tt][r];
        __syncthreads();
      }
      } while (BAL && walk.next_piece());
      return;
    }
    // ---- prob: lane = x column c of the owned 60, wave = 3 output rows ----
    const int c = ptid & 63, rg = ptid >> 6;
    const int yoff = (C::PR * rg + 1) * C::YROWB + (c + 1) * 16;    // window origin: local row 3 rg + 1, local x c + 1
    int st_off[C::PR];                                              // element offsets of this lane's outputs inside a plane
    float A[3][C::PR];
    // Six batches b = (dx, channel half) of 5 window rows x 4 channels and their 9 (ky, kz) x 4 weights.  The weights come
    // through the scalar cache into SGPRs; scalar and LDS loads share lgkmcnt and return out of order with respect to each
    // other, so every wait on either is a wait for ALL of both: the loads of batch b + 1 are therefore issued right AFTER the
    // one wait of batch b and have its ~430 cycles of FMAs to land, instead of being waited for the moment they were issued.
    const f32x4* __restrict__ pw4 = reinterpret_cast<const f32x4*>(pw);   // [dx][half][ky][kz] x 4 channels
    auto load_d = [&](f32x4 (&d)[C::PR + 2], const unsigned char* yb, int b) {
#pragma unroll
      for (int rho = 0; rho < C::PR + 2; ++rho)
        d[rho] = *reinterpret_cast<const f32x4*>(yb + rho * C::YROWB + (b & 1) * C::YHALFB + (b >> 1) * 16);
    };
    auto load_w = [&](f32x4 (&w)[9], int b) {
#pragma unroll
      for (int k = 0; k < 9; ++k) w[k] = pw4[b * 9 + k];
    };
    auto compute = [&](const f32x4 (&d)[C::PR + 2], const f32x4 (&w)[9]) {
#pragma unroll
      for (int ky = 0; ky < 3; ++ky)
#pragma unroll
        for (int kz = 0; kz < 3; ++kz) {
          const f32x4 wv = w[ky * 3 + kz];
#pragma unroll
          for (int r = 0; r < C::PR; ++r) {
            const f32x4 dv = d[r + ky];
            float acc = A[2 - kz][r];
            acc = dpz_fma(dv.x, wv.x, acc);
            acc = dpz_fma(dv.y, wv.y, acc);
            acc = dpz_fma(dv.z, wv.z, acc);
            acc = dpz_fma(dv.w, wv.w, acc);
            A[2 - kz][r] = acc;
          }
        }
    };
    f32x4 wq0[9], wq1[9];
    load_w(wq0, 0);                                  // batch 0 of the first plane; re-requested at the end of every plane
    auto process = [&](int q) {
      const unsigned char* yb = ybuf + (q & 1) * C::YB + yoff;
      f32x4 d0[C::PR + 2], d1[C::PR + 2];
      load_d(d0, yb, 0);
#define DPZ_BATCH(B, DC, WC, DN, WN)                                   \
      __builtin_amdgcn_s_waitcnt(0xC07F); /* lgkmcnt(0): batch B */    \
      __builtin_amdgcn_sched_barrier(0);                               \
      load_w(WN, ((B) + 1) % 6);                                       \
      if ((B) + 1 < 6) load_d(DN, yb, (B) + 1);                        \
      __builtin_amdgcn_sched_barrier(0);                               \
      compute(DC, WC);                                                 \
      __builtin_amdgcn_sched_barrier(0);
      DPZ_BATCH(0, d0, wq0, d1, wq1)
      DPZ_BATCH(1, d1, wq1, d0, wq0)
      DPZ_BATCH(2, d0, wq0, d1, wq1)
      DPZ_BATCH(3, d1, wq1, d0, wq0)
      DPZ_BATCH(4, d0, wq0, d1, wq1)
      DPZ_BATCH(5, d1, wq1, d0, wq0)
#undef DPZ_BATCH
    };
    do {
    DPZ_PIECE()
    stage.init(ptid, X0, Y0, H, W);
    const int ox = tx_i * 2 * C::CXR + c;
    const int oy0 = ty_i * 2 * C::CYR + C::PR * rg;
    const bool lane_ok = c < 2 * C::CXR && ox < Wo;
#pragma unroll
    for (int r = 0; r < C::PR; ++r) st_off[r] = (lane_ok && oy0 + r < Ho) ? (oy0 + r) * Wo + ox : -1;
#pragma unroll
    for (int s = 0; s < 3; ++s)
#pragma unroll
      for (int r = 0; r < C::PR; ++r) A[s][r] = 0.f;
    // prologue: the input planes of the first half-step
    const int ap = qs >> 1;
    issue(ap);
    deposit(ap);
    if (qs & 1) {
      issue(ap + 1);
      deposit(ap + 1);
    }
    // (inside the march the CONSUMERS stage: plane t / 2 + 1 during every even half-step t, see there)
    __syncthreads();                            // #0
    for (int t = qs; t <= te; ++t) {
      const int q = t - 1;
      if (q >= qs && q <= qe) process(q);
      const int o = t - 2;
      if (o >= 2 * a0 && o < 2 * a1) {
        float* po = out + (size_t)o * Ho * Wo;     // wave-uniform plane base + per-lane 32-bit offsets
#pragma unroll
        for (int r = 0; r < C::PR; ++r)
          if (st_off[r] >= 0) po[st_off[r]] = A[0][r];
      }
#pragma unroll
      for (int r = 0; r < C::PR; ++r) {
        A[0][r] = A[1][r];
        A[1][r] = A[2][r];
        A[2][r] = 0.f;
      }
      __syncthreads();
    }
    } while (BAL && walk.next_piece());
    return;
  }

  // ============================== consumers ==============================
  const int j = lane & 15, g = lane >> 4;
  const int px = g >> 1, co = 4 * (g & 1);
  const float4 bv = *reinterpret_cast<const float4*>(bias + co);
  const unsigned char* const wl = lds + lane * 16;
  // B operand offsets inside a plane slot (round 0, N-tile 0)
  const int b_h1 = ((wave + (g >> 1)) * C::IXP + j + (g & 1)) * POSB;
  const int b_h2a = (wave * C::IXP + j + (g & 1)) * POSB;
  const int b_h2b = b_h2a + C::IXP * POSB;
  do {
  DPZ_PIECE()
  // output voxels of this lane: x = 2 (X0 + 16 q + j) + px, y = 2 (Y0 + wave) + py
  int sk_off[2][C::NT];      // residual element offsets inside a z plane, -1 outside the volume
#pragma unroll
  for (int py = 0; py < 2; ++py)
#pragma unroll
    for (int q = 0; q < C::NT; ++q) {
      const int xv = 2 * (X0 + 16 * q + j) + px, yv = 2 * (Y0 + wave) + py;
      sk_off[py][q] = (xv >= 0 && xv < Wo && yv >= 0 && yv < Ho) ? (yv * Wo + xv) * 8 + co : -1;
    }
  const bool border = X0 < 0 || X0 + C::CXC > W || Y0 < 0 || Y0 + C::CYC > H;   // workgroup-uniform: only then is y masked
  // fp32 y: + py * YROWB + q * 32 * 16; MF (fp16 terms, x = 32 q + 2 j + px): hi at + py * YROWB + q * 16 * 16, lo one YTERMB further
  const int y_off = MF ? (2 * wave) * C::YROWB + px * C::YPARB + ((j ^ (px << 3)) << 4) + (g & 1) * 8
                       : (2 * wave) * C::YROWB + (g & 1) * C::YHALFB + (2 * j + px) * 16;
  const size_t zstride = (size_t)Ho * Wo * 8;
  float4 sk0[2][C::NT], sk1[2][C::NT];    // [py][q] of the even / odd half-steps
  auto load_skip = [&](float4 (&sk)[2][C::NT], int t) {
    if (t > qe) return;
    const float* __restrict__ sp = skip + (size_t)t * zstride;
#pragma unroll
    for (int py = 0; py < 2; ++py)
#pragma unroll
      for (int q = 0; q < C::NT; ++q) {
        const int o = sk_off[py][q];
        const float4 v = *reinterpret_cast<const float4*>(sp + max(o, 0));
        sk[py][q] = o >= 0 ? v : make_float4(0.f, 0.f, 0.f, 0.f);
      }
  };
  auto load_a = [&](BV (&wa)[3], int rd, int k) {
    const unsigned char* p = wl + (rd * C::NA + k) * 3 * 1024;
    wa[0].u = *reinterpret_cast<const uint4*>(p);
    wa[1].u = *reinterpret_cast<const uint4*>(p + 1024);
    if (!F16) wa[2].u = *reinterpret_cast<const uint4*>(p + 2048);
  };
  auto load_b = [&](BV (&bd)[C::NT][3], const unsigned char* p) {
#pragma unroll
    for (int q = 0; q < C::NT; ++q) {
      bd[q][0].u = *reinterpret_cast<const uint4*>(p + q * 16 * POSB);
      bd[q][1].u = *reinterpret_cast<const uint4*>(p + q * 16 * POSB + 16);
      if (!F16) bd[q][2].u = *reinterpret_cast<const uint4*>(p + q * 16 * POSB + 32);
    }
  };
  f32x4 acc[2][C::NT];
  auto epilogue = [&](const float4 (&sk)[2][C::NT], int par) {
    unsigned char* yb = ybuf + par * C::YB + y_off;
#pragma unroll
    for (int py = 0; py < 2; ++py)
#pragma unroll
      for (int q = 0; q < C::NT; ++q) {
        // split-f16: back to the layer's scale, then the BN shift (split-bf16: it rode in the accumulator).  sf16_rescale4 written as
        // whole-vector operations: with the componentwise form the compiler turns the border selects below into exec-masked branches
        f32x4 a = acc[py][q];
        if (F16) a = a * out_mul + (f32x4){bv.x, bv.y, bv.z, bv.w};
        float4 o = sbf_add4(sk[py][q], sbf_relu4(sbf_f4(a)));
        if (border && sk_off[py][q] < 0) o = make_float4(0.f, 0.f, 0.f, 0.f);
        if constexpr (MF) {
          uint32_t h0, l0, h1, l1;
          split2_f16(o.x, o.y, ys, h0, l0);
          split2_f16(o.z, o.w, ys, h1, l1);
          unsigned char* yp = yb + py * C::YROWB + q * 16 * 16;
          *reinterpret_cast<uint2*>(yp) = make_uint2(h0, h1);
          *reinterpret_cast<uint2*>(yp + C::YTERMB) = make_uint2(l0, l1);
        } else {
          *reinterpret_cast<float4*>(yb + py * C::YROWB + q * 32 * 16) = o;
        }
      }
  };
  // ---- input staging inside the march: plane t / 2 + 1 is loaded at the start of every EVEN half-step t (its slot held plane
  // t / 2 - 1, which nobody reads after the barrier before) and split + stored after the half-step's epilogue, in the ~2000 cycles
  // the consumers used to spend at that barrier waiting for the prob waves.  (The prob waves did this until round 5: 1600-1700
  // cycles of every even half-step on the kernel's critical chain; probe without any staging: 975 vs 1170 us.) ----
  ZmCellStage<C, C::CW * 64, F16, true> stage;
  stage.init(tid, X0, Y0, H, W);
  if (qs & 1) load_skip(sk1, qs); else load_skip(sk0, qs);
  __syncthreads();                                // #0
  for (int t = qs; t <= te; ++t) {
    if (t <= qe) {
      const int a = t >> 1;
      const unsigned char* cur = inring + (a & 1) * C::SLOTB;
#pragma unroll
      for (int py = 0; py < 2; ++py)
#pragma unroll
        for (int q = 0; q < C::NT; ++q)      // the BN shift rides in the accumulator (split-f16: added after the rescaling)
          acc[py][q] = F16 ? (f32x4){0.f, 0.f, 0.f, 0.f} : (f32x4){bv.x, bv.y, bv.z, bv.w};
      if (!(t & 1)) {
        // ---- z parity 0: plane 2 a from cell plane a ----
        stage.issue(x, a + 1, D, H, W);
        load_skip(sk1, t + 1);
        BV w0[3], w1[3], b0[C::NT][3], b1[C::NT][3];
        load_b(b0, cur + b_h1);
        load_a(w0, 0, 0);
        load_a(w1, 0, 1);
        load_b(b1, cur + C::ROUNDB + b_h1);
        __builtin_amdgcn_sched_barrier(0);
        DPZ_TERMS(acc[0], w0, b0);
        load_a(w0, 1, 0);
        __builtin_amdgcn_sched_barrier(0);
        DPZ_TERMS(acc[1], w1, b0);
        load_a(w1, 1, 1);
        __builtin_amdgcn_sched_barrier(0);
        DPZ_TERMS(acc[0], w0, b1);
        DPZ_TERMS(acc[1], w1, b1);
        epilogue(sk0, 0);
        stage.deposit(inring + ((a + 1) & 1) * C::SLOTB, xs);
      } else {
        // ---- z parity 1: plane 2 a + 1 from cell planes a (kz = 2) and a + 1 (kz = 0) ----
        load_skip(sk0, t + 1);
        const unsigned char* oth = inring + ((a + 1) & 1) * C::SLOTB;
        const unsigned char* bz = (g >> 1) ? oth : cur;
        BV w0[3], w1[3], b0[C::NT][3], b1[C::NT][3];
#pragma unroll
        for (int rd = 0; rd < C::ROUNDS; ++rd) {
          load_b(b0, bz + rd * C::ROUNDB + b_h2a);
          load_a(w0, rd, 2);
          load_a(w1, rd, 3);
          load_b(b1, bz + rd * C::ROUNDB + b_h2b);
          __builtin_amdgcn_sched_barrier(0);
          DPZ_TERMS(acc[0], w0, b0);
          load_a(w0, rd, 4);
          __builtin_amdgcn_sched_barrier(0);
          DPZ_TERMS(acc[1], w1, b0);
          DPZ_TERMS(acc[1], w0, b1);
        }
        epilogue(sk1, 1);
      }
    }
    __syncthreads();
  }
  } while (BAL && walk.next_piece());
#undef DPZ_PIECE
}

}  // namespace

// conv11 + residual + prob in one launch.  x [D][H][W][16] channels-last input cells, skip [2D][2H][2W][8] channels-last (conv0's
// output), weight_split from ops.split_pack_deconv_prob (int16 [2][5][3][64][8]), bias [8] (BN shift), prob_table from
// ops.pack_prob_table (float [3 kx][2 halves][3 ky][3 kz][4]); out [2D][2H][2W] fp32.
// skip_bound given: prob_table is the operand table of ops.split_pack_prob and prob runs on the matrix cores (split-f16 only).
static int dpz_entry(const float* x, const void* weight_split, const float* bias, const float* skip, const float* prob_table, float* out,
                     int D, int H, int W, const float* in_bound, float w_inv, void* stream, const float* skip_bound = nullptr,
                     float y_gain = 0.f, float p_inv = 1.f) {
  if (!x || !weight_split || !bias || !skip || !prob_table || !out || D < 1 || H < 1 || W < 1) return CDS_EINVAL;
  if ((long)2 * H * 2 * W * 8 >= (1l << 31) || (long)H * W * 16 >= (1l << 31)) return CDS_EINVAL;   // in-plane offsets are 32-bit
  using C = DPZ;
  hipStream_t st = (hipStream_t)stream;
  const int tiles_x = cds_ceil_div(W, C::CXR), tiles_y = cds_ceil_div(H, C::CYR);
  const int ncols = tiles_x * tiles_y;
  double ucost;
  const int seg_len = cds_ceil_div(D, zm_pick_nseg(ncols, D, 16, "CDS_DPZ_NSEG", &ucost));
  const int nseg = cds_ceil_div(D, seg_len);
  const int nwg = zm_ncu();
  const bool bal = zm_choose_balanced(zm_balance_knob(), ucost, ncols, D, nwg, ZM_MINLEN_CELL, 1.5, nullptr, ZM_BALANCE_MARGIN_TAIL);
  // the form follows from the bounds the caller gave (the forms without them ignore the arguments that go with them)
  auto launch = [&](auto f16, auto mf, auto b) {
    return cds_launch_lds<deconv_prob_zm_kernel<decltype(f16)::value, decltype(mf)::value, decltype(b)::value>>(
        160 * 1024, dim3(b ? nwg : ncols * nseg), dim3(C::THREADS), C::LDS, st, x, reinterpret_cast<const uint4*>(weight_split), bias, skip,
        prob_table, out, D, H, W, tiles_x, ncols, seg_len, in_bound, w_inv, skip_bound, y_gain, p_inv);
  };
  auto forms = [&](auto b) {
    if (skip_bound) return launch(std::true_type(), std::true_type(), b);
    return in_bound ? launch(std::true_type(), std::false_type(), b) : launch(std::false_type(), std::false_type(), b);
  };
  return bal ? forms(std::true_type()) : forms(std::false_type());
}

extern "C" int cds_deconv_prob_zm_f32(const float* x, const void* weight_split, const float* bias, const float* skip,
                                      const float* prob_table, float* out, int D, int H, int W, void* stream) {
  return dpz_entry(x, weight_split, bias, skip, prob_table, out, D, H, W, nullptr, 1.0f, stream);
}

// The same fused tail with the transposed convolution in SPLIT-F16 arithmetic: weight_split from ops.split_pack_deconv_prob(..., f16=True),
// w_inv_scale = 1 / its weight scale, in_bound a DEVICE scalar >= max |x| (conv9's out_bound).
extern "C" int cds_deconv_prob_zm_sf16_f32(const float* x, const void* weight_split, const float* bias, const float* skip,
                                           const float* prob_table, float* out, int D, int H, int W, const float* in_bound,
                                           float w_inv_scale, void* stream) {
  if (!in_bound || !(w_inv_scale > 0.f)) return CDS_EINVAL;
  return dpz_entry(x, weight_split, bias, skip, prob_table, out, D, H, W, in_bound, w_inv_scale, stream);
}

// The split-f16 tail with prob on the matrix cores as well.  prob_table from ops.pack_prob_table and prob_mfma / p_inv_scale from
// ops.split_pack_prob (fp16 (hi, lo) operands [3][3][64][8] and 1 / their scale); skip_bound a DEVICE scalar >= max |skip| (conv0's
// out_bound), y_gain >= max over cout of the sum of |folded conv11 weight|: skip_bound + y_gain * in_bound + max |bias| bounds the
// volume between the two layers, which is what its fp16 terms are scaled by.  CDS_DPZ_PROB_MFMA=0 (A/B knob, read per launch) runs
// prob on the VALU from prob_table instead: the kernel of cds_deconv_prob_zm_sf16_f32.
extern "C" int cds_deconv_prob_zm_sf16_mfma_f32(const float* x, const void* weight_split, const float* bias, const float* skip,
                                                const float* prob_table, const void* prob_mfma, float* out, int D, int H, int W,
                                                const float* in_bound, float w_inv_scale, const float* skip_bound, float y_gain,
                                                float p_inv_scale, void* stream) {
  if (!in_bound || !(w_inv_scale > 0.f) || !prob_mfma || !skip_bound || !(y_gain >= 0.f) || !(p_inv_scale > 0.f)) return CDS_EINVAL;
  const char* e = getenv("CDS_DPZ_PROB_MFMA");
  if (e && atoi(e) == 0) return dpz_entry(x, weight_split, bias, skip, prob_table, out, D, H, W, in_bound, w_inv_scale, stream);
  return dpz_entry(x, weight_split, bias, skip, static_cast<const float*>(prob_mfma), out, D, H, W, in_bound, w_inv_scale, stream,
                   skip_bound, y_gain, p_inv_scale);
}
