// K4, z-marching form of the 3x3x3 convolutions of CostRegNet, split-bf16 and split-f16: conv0 to conv3 and the three stride-1
// layers to 8 channels (the "pair" layers: Cin = 8 / 16 / 32) in both arithmetics, conv4 to conv6 in split-f16.
//
// What the tiled kernels of conv3d_sbf.hip pay (measured in rounds 2 / 3): a TX x 4 x TZ tile stages 2.4 input positions per
// output voxel at stride 1 and 11.6 at stride 2 (8 is the minimum), every 8-channel round of a tile is its own barrier stage, and
// the weights of every K-step stream through the consumer waves' vector-memory queue.  Here a workgroup owns a column of
// TXO x TYO output voxels and MARCHES along z:
//   * the staged input is a RING of z-planes in LDS ([plane][8-channel slice][row][x] x 48 B, the [term][8] bf16 position
//     format of sbf_common.hpp; split-f16 configurations may ask for two 16-byte term planes per slice instead: ZG::P32);
//     every input plane is loaded, split and stored ONCE per column: 1.33 (stride 1, 32 x 8) or 9.1-9.3 (stride 2) staged
//     positions per output voxel and no re-read along z;
//   * ONE workgroup barrier per G output planes whatever the channel count: all slices of a plane are resident together;
//   * the weights never move: the four consumer waves split the K dimension (8-channel rounds) and the 16-cout blocks between
//     them, so every wave keeps the <= 27 weight vectors of ITS (round, cout block) in registers for the whole kernel
//     (84 / 108 VGPRs) and its stage loop consists of LDS operand reads and MFMAs only.  Waves that split K exchange the
//     partial sums of half of their N-tiles through a double-buffered LDS area across the stage barrier and add them in a
//     fixed order (round 0 + round 1), so results do not depend on timing;
//   * the four producer waves issue unconditional loads: an out-of-volume position reads a 32-byte zero block in global memory
//     (a two-instruction address select) instead of an exec-masked branch per position.
// Same arithmetic, operand layout and weight packing (ops.split_pack_conv3d / split_pack_conv3d_pair) as the tiled kernels;
// reached through cds_conv3d_sbf_f32 (conv3d_sbf.hip), which keeps the tiled kernels for the shapes not covered here.
// Reference: models/module.py:80-116 (Conv3d + BatchNorm3d + ReLU), :270-315 (CostRegNet).
#include <stdlib.h>

#include <type_traits>

#include "cds_common.hpp"
#include "sbf_common.hpp"
#include "zm_common.hpp"

namespace {

__device__ __attribute__((aligned(32))) float g_zmg_zeros[8];   // what an out-of-volume position loads

// What a configuration may set (ZGDefaults); a layer's configuration is a struct that derives from it and names what differs.
// S: stride.  RD: 8-channel rounds of the input (Cin / 8).  MB: 16-cout blocks.  PAIR: Cout = 8, an MFMA column is a pair of x
// neighbours (ops.split_pack_conv3d_pair).  TXO x TYO: output voxels of a column.  G: output planes per stage.  NG: N-tiles per K-step.
// CW = 4: one consumer wave per SIMD (256-register budget); CW = 8: two per SIMD, 12 waves per workgroup, 168 registers: one
// MFMA-issuing wave per SIMD sustains one v_mfma_f32_16x16x32_bf16 per 10.0 ns, two sustain one per 8.1 ns (scripts/ubench), and the
// second wave's K-loop covers the first one's exchange / epilogue / barrier time.
// F16: split-f16 arithmetic (two fp16 terms per operand, three products per K-step, tensor scales from device bounds: sbf_common.hpp)
// instead of split-bf16 (three bf16 terms, six products); same staging geometry, term 2 of a position / weight vector unused.
// RPW: 8-channel rounds a consumer wave keeps (the K dimension is split over RD / RPW waves; the deep layers' Cin = 32 / 64 would
// otherwise need more consumer waves than a workgroup has).  YS: the cout blocks are split over gridDim.y (every one of the YS
// workgroups of a column stages the whole input ring and computes MB / YS cout blocks: Cout = 64).  PF: K-steps the LDS operand
// reads run ahead of their MFMAs (2: a wave with ONE N-tile per step has only three MFMAs to cover an LDS round trip).
// P32 (split-f16 only): 32-byte positions, term-planar inside a slice ([term][row][x] x 16 B) instead of the 48-byte
// [term 0 | term 1 | unused] position: the ring shrinks by a third (conv5: 163 200 -> 108 800 B, which is what lets a stride-2
// column of 32 input channels fit at all), 16 lanes on 16 consecutive x still read 16 different 16-byte bank groups, and the tap
// offsets stay compile-time constants.
// BALANCED: the layer may run in the balanced cutting (zm_common.hpp), whose walk over pieces keeps one or two more registers
// alive across the stage loop; false where the configuration has none left.
struct ZGDefaults {
  static constexpr int S = 1, RD = 1, MB = 1, TXO = 16, TYO = 8, G = 1, NG = 1, CW = 8, RPW = 1, YS = 1, PF = 1;
  static constexpr bool PAIR = false, F16 = false, P32 = false, BALANCED = true;
};
// the split-f16 sibling of a split-bf16 configuration that differs in nothing else
template <class P>
struct ZgF16 : P {
  static constexpr bool F16 = true;
};

// Consumer waves per SIMD as measured at the M1 / cascade shapes (profiles/r04_zmarch.md): two for everything but the 16 -> 8 and
// 32 -> 8 pair layers.
struct ZgPair8 : ZGDefaults {    // 8 -> 8 (conv0 at 8 channels): three output planes per stage
  static constexpr bool PAIR = true;
  static constexpr int TXO = 32, G = 3;
};
struct ZgPair16 : ZGDefaults {   // 16 -> 8 (conv0 of the 16-channel cascade stage)
  static constexpr bool PAIR = true;
  static constexpr int RD = 2, TXO = 32, NG = 4, CW = 4;
};
struct ZgPair32 : ZGDefaults {   // 32 -> 8 (conv0 of the 32-channel cascade stage): K split in four, the ring leaves room for three output rows per stage
  static constexpr bool PAIR = true;
  static constexpr int RD = 4, TXO = 32, TYO = 3, NG = 3, CW = 4;
};
struct ZgConv1 : ZGDefaults {    // 8 -> 16, stride 2
  static constexpr int S = 2;
};
struct ZgConv2 : ZGDefaults {    // 16 -> 16 (split-bf16: K split over wave pairs)
  static constexpr int RD = 2, TXO = 32;
};
struct ZgConv3 : ZGDefaults {    // 16 -> 32, stride 2 (split-bf16: K split over wave pairs)
  static constexpr int S = 2, RD = 2, MB = 2, TYO = 4;
};
// conv2, split-f16: both rounds of weights in one wave like conv3 below (no exchange through LDS, no finalising step), on the 32-byte
// ring with the uniform-base output address: 162 VGPRs, no scratch (with 64-bit per-lane output addresses: 168 and 2-4 spilled);
// profiles/zmarch_conv5.md: 325-338 -> 306-316 us in the M1 step
struct ZgConv2F16 : ZgF16<ZgConv2> {
  static constexpr int RPW = 2;
  static constexpr bool P32 = true;
};
// conv3, split-f16: both rounds of weights in one wave (RPW = 2: 112 registers of two fp16 terms, 162 VGPRs) instead of the K split
// over wave pairs that three bf16 terms need: no exchange through LDS and no finalising step (profiles/zmarch_conv7.md: 180-183 ->
// 157-162 us)
struct ZgConv3F16 : ZgF16<ZgConv3> {
  static constexpr int RPW = 2;
};
// conv4 (32 -> 32): K split over four waves x two cout blocks, 16 x 4 columns (ring 81 KB + 2 x 32 KB exchange)
struct ZgConv4F16 : ZgF16<ZGDefaults> {
  static constexpr int RD = 4, MB = 2, TYO = 4, PF = 2;
};
// conv5 (32 -> 64, stride 2): 16 x 2 output columns on the 32-byte ring (5 planes of 4 slices x 5 x 34 positions = 108 800 B; at
// 48 bytes per position 163 200 B: no stride-2 column of 32 channels fits), K split in two with two rounds of weights per wave
// x the four cout blocks = 8 consumer waves of 84 MFMAs per stage (2 x 8 KB exchange), 167 VGPRs; operand reads two K-steps
// ahead (PF = 2) would spill 14 of them.  profiles/zmarch_conv5.md: 133-139 us tiled -> 68-80 us in the M1 step
// Uniform cutting only: at 167 of 168 VGPRs the walk over pieces spills 19 registers (56 bytes of scratch).
struct ZgConv5F16 : ZgF16<ZGDefaults> {
  static constexpr int S = 2, RD = 4, MB = 4, TYO = 2, RPW = 2;
  static constexpr bool P32 = true, BALANCED = false;
};
// conv6 (64 -> 64): two rounds of weights per wave (K split over four waves), two cout blocks per workgroup and two workgroups
// (gridDim.y) per 16 x 2 column: the input is staged twice from L2 / the memory-side cache, against four times and stages of 42
// MFMAs per wave for a K split over eight waves with one cout block per workgroup (ring 108 KB + 2 x 16 KB exchange)
// Uniform cutting only: at 168 VGPRs the walk over pieces spills 6 registers (28 bytes of scratch).
struct ZgConv6F16 : ZgF16<ZGDefaults> {
  static constexpr int RD = 8, MB = 4, TYO = 2, RPW = 2, YS = 2;
  static constexpr bool BALANCED = false;
};

// The geometry that follows from a configuration P.
template <class P>
struct ZG {
  static constexpr int S = P::S, RD = P::RD, MB = P::MB, TXO = P::TXO, TYO = P::TYO, G = P::G, NG = P::NG;
  static constexpr bool F16 = P::F16;
  static constexpr int NT = F16 ? 2 : 3;                           // terms per operand
  static constexpr bool PAIR = P::PAIR, DEINT = PAIR || S == 2;
  static constexpr int CW = P::CW, PW = 4, THREADS = (CW + PW) * 64;
  static constexpr int RPW = P::RPW, YS = P::YS, PF = P::PF;
  static_assert(PF == 1 || (PF == 2 && 2 * NG * NT <= 15), "operand prefetch distance (lgkmcnt is a 4-bit count)");
  static_assert(RD % RPW == 0 && MB % YS == 0, "rounds per wave / cout split");
  static constexpr int KSPL = RD / RPW, MBS = MB / YS;            // wave = (RPW rounds, cout block, row part)
  static_assert(CW % (KSPL * MBS) == 0 && (KSPL == 1 || KSPL == 2 || KSPL == 4), "consumer waves");
  static constexpr int PARTS = CW / (KSPL * MBS);
  static constexpr int ROWS = TYO / PARTS;                        // output rows per consumer wave
  static constexpr int XT = TXO / (PAIR ? 32 : 16);
  static constexpr int NTW = ROWS * XT * G;                       // N-tiles per consumer wave and stage
  static_assert(TYO % PARTS == 0 && NTW % NG == 0 && (KSPL != 2 || NTW % 2 == 0), "tile split");
  static constexpr int KW = PAIR ? 4 : 3, KS = (9 * KW + 3) / 4;  // 7 K-steps of 4 taps (27 + 1 zero) | 9 of (kz, ky) x 4 x'
  static constexpr int IX = (TXO - 1) * S + 3, IY = (TYO - 1) * S + 3;
  static constexpr int IXH = DEINT ? (IX + 1) / 2 : 0;            // x parities de-interleaved (stride 2, pair columns)
  static constexpr int IXP = DEINT ? 2 * IXH : IX;
  // PB = bytes from a position to its x neighbour, TB = from its term 0 to its term 1
  static constexpr bool P32 = P::P32;
  static_assert(!P32 || F16, "the 32-byte position holds two terms");
  static constexpr int PB = P32 ? 16 : POSB, TB = P32 ? IY * IXP * 16 : 16;
  static constexpr int SLICEB = IY * IXP * (P32 ? 32 : POSB), PLANEB = RD * SLICEB;
  static constexpr int NINIT = 3 - S;                             // planes below the first stage's new ones
  static constexpr int NRES = S * (G - 1) + 3, NNEW = S * G, R = NRES + NNEW;
  static constexpr int RINGB = R * PLANEB;
  // one exchange buffer.  K split in two: every wave sends NTW / 2 N-tiles to its partner.  In four (the 32 -> 8 pair layer: the
  // ring leaves no room for more than three output rows per stage): a slot per (N-tile, source round); N-tile n is finalised by the
  // wave of round n % 4, which adds the four partial sums in the order of the rounds.
  static constexpr int XCH1 = KSPL == 2 ? CW * (NTW / 2) * 1024 : (KSPL == 4 ? CW * NTW * 1024 : 0);
  static constexpr int NFIN = KSPL == 4 ? (NTW + 3) / 4 : 1;          // N-tiles a wave finalises (K split in four)
  // tap of (K-step t, lane group gg): PAIR: (kz, ky) row t, x' = 0, 2, 1, 3 (the two groups of an LDS service group read the same
  // parity plane one position apart); else tap 4 t + gg, tap 27 = zero weights -> any resident position
  static constexpr int tap_of(int t, int gg) {
    const int tap = PAIR ? 4 * t + ((gg & 1) * 2 + (gg >> 1)) : 4 * t + gg;
    return tap > 9 * KW - 1 ? 9 * KW - 1 : tap;
  }
  static constexpr int tap_kz(int t, int gg) { return tap_of(t, gg) / (3 * KW); }
  static constexpr int tap_off(int t, int gg) {                   // byte offset of the tap inside a slice
    const int tap = tap_of(t, gg), ky = (tap / KW) % 3, kx = tap % KW;
    return (ky * IXP + (DEINT ? ((kx & 1) * IXH + (kx >> 1)) : kx)) * PB;
  }
  static constexpr int LDSB = RINGB + 2 * XCH1;
  static_assert(LDSB <= 160 * 1024, "LDS budget");
  static constexpr int NITEM = NNEW * IY * RD * IXP;              // staged positions per stage (incl. the de-interleave pad)
  static constexpr int PT = PW * 64, PPT = (NITEM + PT - 1) / PT;
};

// The uniform cutting has no walk: one unit per workgroup, from the index arithmetic in the kernel.
struct ZmgNoWalk {
  __device__ __forceinline__ ZmgNoWalk(int, int, int, int) {}
  __device__ __forceinline__ bool empty() const { return false; }
  __device__ __forceinline__ ZmColumn column(int) const { return {0, 0, 0, 0}; }
  __device__ __forceinline__ bool next_piece() { return false; }
};

// BAL: the balanced cutting (zm_common.hpp; a stage = G output planes, a column = tiles_x x tiles_y of them per cout split
// blockIdx.y): the workgroup walks the pieces of its range, one march each.  The consumer waves' weights, the bias and the running
// bound stay; the producers' item tables, lane_ok and the output bases are set up again for every piece.
template <class Cfg, bool BAL>
__global__ __launch_bounds__(Cfg::THREADS, 1) void conv3d_zmg_kernel(const float* __restrict__ x, const uint4* __restrict__ wsp,
                                                                  const float* __restrict__ bias, float* __restrict__ out, int Cout,
                                                                  int D, int H, int W, int Do, int Ho, int Wo, int act,
                                                                  int tiles_x, int tiles_y, int zseg,
                                                                  const float* __restrict__ in_bound, float w_inv,
                                                                  float* __restrict__ out_bound) {
  constexpr int S = Cfg::S, RD = Cfg::RD, G = Cfg::G, R = Cfg::R, Cin = 8 * RD, KS = Cfg::KS, NTW = Cfg::NTW, NG = Cfg::NG;
  constexpr bool PAIR = Cfg::PAIR, F16 = Cfg::F16;
  constexpr int NT = Cfg::NT;
  // split-f16: the input's scale from the bound its producer left, and what the accumulators are multiplied by at the end (exact)
  const float xs = F16 ? sf16_scale(in_bound[0]) : 1.0f;
  const float out_mul = F16 ? w_inv / xs : 1.0f;
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  std::conditional_t<BAL, ZmWalk<true>, ZmgNoWalk> walk(tiles_x * tiles_y, (Do + G - 1) / G, 0, ZM_MINLEN_ZMG);
  if (BAL && walk.empty()) return;
  // what a march derives from its unit.  Uniform cutting: unit = (column tx, ty; z segment), the z segments of a column are
  // consecutive workgroups; balanced: a piece of the walk (set again behind the barrier between two pieces).  [z0, z1): its output
  // planes; input plane zin0 is in ring slot 0 and plane p lives in slot (p - zin0) % R
  int tx_i, ty_i, z0, z1, nstages, gx0, gy0, zin0;
  auto set_piece = [&] {
    if constexpr (BAL) {
      const ZmColumn zc = walk.column(tiles_x);
      tx_i = zc.tx_i, ty_i = zc.ty_i, z0 = zc.a0 * G, z1 = min(Do, zc.a1 * G);
    } else {
      const int nseg = (Do + zseg - 1) / zseg;
      int unit = cds_xcd_remap(blockIdx.x, gridDim.x);
      const int seg = unit % nseg;
      unit /= nseg;
      tx_i = unit % tiles_x, ty_i = unit / tiles_x;
      z0 = seg * zseg, z1 = min(Do, z0 + zseg);
    }
    nstages = (z1 - z0 + G - 1) / G;
    gx0 = tx_i * Cfg::TXO * S - 1, gy0 = ty_i * Cfg::TYO * S - 1;
    zin0 = S * z0 - 1;
    return true;
  };
  set_piece();

  if (wave >= Cfg::CW) {
    // ============================== producers ==============================
    // The producers are the critical path of a stage (s_memtime probe, scripts/ubench/zmg_timeline_*: their split + LDS stores took
    // ~7000 of a conv0 stage's ~8400 cycles next to two MFMA-issuing waves per SIMD, and the consumers then waited for them at the
    // barrier): they issue ahead of the consumer waves whenever they have work.
#ifndef CDS_ZMG_PPRIO
#define CDS_ZMG_PPRIO 3
#endif
    __builtin_amdgcn_s_setprio(CDS_ZMG_PPRIO);
    constexpr int PT = Cfg::PT, PPT = Cfg::PPT;
    const int ptid = tid - Cfg::CW * 64;
    do {
    // item = one 8-channel position of the stage's NNEW new planes: x fastest, then slice, row, plane
    int s_pl[PPT], s_dst[PPT];
    long long s_off[PPT];                                         // element offset in x[] for plane index 0 of the volume
    unsigned okmask = 0;                                          // bit h: the item exists and its (y, x) is inside the volume
#pragma unroll
    for (int h = 0; h < PPT; ++h) {
      const int p = h * PT + ptid;
      const int q = p % Cfg::IXP, t1 = p / Cfg::IXP;
      const int rd = t1 % RD, t2 = t1 / RD;
      const int row = t2 % Cfg::IY, pl = t2 / Cfg::IY;
      const int c = Cfg::DEINT ? (2 * (q % Cfg::IXH) + q / Cfg::IXH) : q;
      const int gy = gy0 + row, gx = gx0 + c;
      const bool exists = p < Cfg::NITEM && c < Cfg::IX;
      s_pl[h] = pl;
      s_dst[h] = rd * Cfg::SLICEB + (row * Cfg::IXP + q) * Cfg::PB;
      s_off[h] = ((long long)gy * W + gx) * Cin + rd * 8;
      if (exists && (unsigned)gy < (unsigned)H && (unsigned)gx < (unsigned)W) okmask |= 1u << h;
      if (!exists) s_pl[h] = -1;
    }
    const long long plane_elems = (long long)H * W * Cin;
    float4 va[2][PPT], vb[2][PPT];
    // stage st: new input planes zin0 + st S G + NINIT + (0 .. NNEW - 1)
    auto issue = [&](int st, int set) {
      const int zn = zin0 + st * S * G + Cfg::NINIT;
#pragma unroll
      for (int h = 0; h < PPT; ++h) {
        const int z = zn + s_pl[h];
        const bool ok = ((okmask >> h) & 1u) && (unsigned)z < (unsigned)D;
        const float* __restrict__ src = ok ? x + ((long long)z * plane_elems + s_off[h]) : g_zmg_zeros;
        va[set][h] = *reinterpret_cast<const float4*>(src);
        vb[set][h] = *reinterpret_cast<const float4*>(src + 4);
      }
    };
    auto deposit = [&](int st, int set) {
      const int slot0 = (st * S * G + Cfg::NINIT) % R;
#pragma unroll
      for (int h = 0; h < PPT; ++h) {
        if (h + 1 == PPT && s_pl[h] < 0) continue;                 // only the last item of a thread can be missing
        int slot = slot0 + (s_pl[h] < 0 ? 0 : s_pl[h]);
        slot = slot >= R ? slot - R : slot;
        if (Cfg::P32) split_store8_f16_planar(lds + slot * Cfg::PLANEB + s_dst[h], Cfg::TB, va[set][h], vb[set][h], xs);
        else if (F16) split_store8_f16(lds + slot * Cfg::PLANEB + s_dst[h], va[set][h], vb[set][h], xs);
        else split_store8(lds + slot * Cfg::PLANEB + s_dst[h], va[set][h], vb[set][h]);
      }
    };
    // the NINIT lowest planes of the segment: loaded, split and stored directly
    for (int p = ptid; p < Cfg::NINIT * Cfg::IY * RD * Cfg::IXP; p += PT) {
      const int q = p % Cfg::IXP, t1 = p / Cfg::IXP;
      const int rd = t1 % RD, t2 = t1 / RD;
      const int row = t2 % Cfg::IY, pl = t2 / Cfg::IY;
      const int c = Cfg::DEINT ? (2 * (q % Cfg::IXH) + q / Cfg::IXH) : q;
      const int gz = zin0 + pl, gy = gy0 + row, gx = gx0 + c;
      const bool ok = c < Cfg::IX && (unsigned)gz < (unsigned)D && (unsigned)gy < (unsigned)H && (unsigned)gx < (unsigned)W;
      const float* __restrict__ src = ok ? x + (((long long)gz * H + gy) * W + gx) * Cin + rd * 8 : g_zmg_zeros;
      unsigned char* dst = lds + pl * Cfg::PLANEB + rd * Cfg::SLICEB + (row * Cfg::IXP + q) * Cfg::PB;
      if (Cfg::P32) split_store8_f16_planar(dst, Cfg::TB, *reinterpret_cast<const float4*>(src), *reinterpret_cast<const float4*>(src + 4), xs);
      else if (F16) split_store8_f16(dst, *reinterpret_cast<const float4*>(src), *reinterpret_cast<const float4*>(src + 4), xs);
      else split_store8(dst, *reinterpret_cast<const float4*>(src), *reinterpret_cast<const float4*>(src + 4));
    }
    issue(0, 0);
    if (nstages > 1) issue(1, 1);
    deposit(0, 0);
    if (nstages > 2) issue(2, 0);
    __syncthreads();                                   // #0: stage 0 staged
    for (int st = 0; st < nstages; st += 2) {
      if (st + 1 < nstages) {
        deposit(st + 1, 1);
        if (st + 3 < nstages) issue(st + 3, 1);
      }
      __syncthreads();                                 // #(st + 1): stage st consumed, stage st + 1 staged
      if (st + 1 >= nstages) break;
      if (st + 2 < nstages) {
        deposit(st + 2, 0);
        if (st + 4 < nstages) issue(st + 4, 0);
      }
      __syncthreads();                                 // #(st + 2)
    }
    } while (BAL && walk.next_piece() && set_piece());
    return;
  }

  // ============================== consumers: wave = (round k, cout block mbi, row part) ==============================
#ifndef CDS_ZMG_CPRIO
#define CDS_ZMG_CPRIO 2
#endif
  __builtin_amdgcn_s_setprio(CDS_ZMG_CPRIO);
  const int k = wave % Cfg::KSPL, mbi = (wave / Cfg::KSPL) % Cfg::MBS, part = wave / (Cfg::KSPL * Cfg::MBS);
  const int j = lane & 15, g = lane >> 4;
  // Two consumer waves per SIMD (CW = 8: waves w and w + 4 share one): the second one runs its epilogue AFTER the stage barrier
  // instead of before it, so each wave's address set-up / exchange / bias / ReLU / stores overlap with the other one's MFMAs instead
  // of both doing them in lock-step on either side of the barrier (which idled the matrix pipe for a third of every stage).
#ifdef CDS_ZMG_NOSKEW
  const bool late = false;                             // A/B knob
#else
  const bool late = Cfg::CW == 8 && wave >= 4;
#endif
  // byte offset of this lane inside a slice: its slice (round k), first row of its part, voxel j; PAIR: + the x' of its lane group
  // (x' = 0, 2, 1, 3: de-interleaved parity plane + half index), the (kz, ky) of a K-step being uniform
  const int lane_base = k * Cfg::RPW * Cfg::SLICEB + (part * Cfg::ROWS * S * Cfg::IXP + j) * Cfg::PB +
                        (PAIR ? (((g & 1) * 2 + (g >> 1)) & 1) * Cfg::IXH * Cfg::PB + ((((g & 1) * 2 + (g >> 1))) >> 1) * Cfg::PB : 0);
  // this wave's weights: [round k RPW + rr][K-step][cout block][term][lane]
  constexpr int RPW = Cfg::RPW;
  const int mbg = (Cfg::YS > 1 ? blockIdx.y * Cfg::MBS : 0) + mbi;   // cout block in the layer
  BV wres[RPW * KS][NT];
  {
    const uint4* __restrict__ wl = wsp + lane;
#pragma unroll
    for (int t = 0; t < RPW * KS; ++t) {
      const size_t o = (size_t)(((k * RPW * KS + t) * Cfg::MB + mbg) * 3) * 64;
#pragma unroll
      for (int tm = 0; tm < NT; ++tm) wres[t][tm].u = wl[o + 64 * tm];
    }
  }
  float amax = 0.f;                                    // running maximum of the magnitudes this lane stores (split-f16: the output's bound)
  const int co = PAIR ? 4 * (g & 1) : mbg * 16 + 4 * g;
  const float4 bv = (bias && co < Cout) ? *reinterpret_cast<const float4*>(bias + co) : make_float4(0.f, 0.f, 0.f, 0.f);
  // Balanced: of the lane's place in a column only xl (its x inside the column's first run) and its output offset inside the
  // column's first row stay in registers across the pieces; a piece adds wave-uniform values to them (one register more than the
  // uniform form keeps, none where that holds a 64-bit address per lane)
  const int xl = PAIR ? 2 * j + (g >> 1) : j;
  do {
  // N-tile n of this wave = (row r, x run xt, plane i): n = (r XT + xt) G + i
  constexpr int XW = PAIR ? 32 : 16;
  constexpr bool UBASE = Cfg::P32 || BAL;                // output address = wave-uniform 64-bit part + 32-bit lane offset
  const int oy0 = ty_i * Cfg::TYO + part * Cfg::ROWS;
  const int ox0 = tx_i * Cfg::TXO + xl;
  const int x_left = Wo - tx_i * Cfg::TXO;               // (wave-uniform) voxels from the column's first to the end of the row
  float* const obase = out + ((size_t)((size_t)z0 * Ho + oy0) * Wo + ox0) * Cout + co;   // this lane's voxel of N-tile 0, stage 0
  // P32 configurations (168-register budget, 112 of them weights): the same address as a wave-uniform 64-bit part (SGPRs) + a 32-bit
  // lane offset inside the column's first row, instead of 64-bit per-lane addresses that the compiler keeps in VGPRs across the stage
  // loop (the no-K-split conv2 spilled four registers for them)
  float* const obase_u = out + ((size_t)((size_t)z0 * Ho + oy0) * Wo + tx_i * Cfg::TXO) * Cout;
  const unsigned olane = BAL ? (unsigned)(xl * Cout + co) : (unsigned)((ox0 - tx_i * Cfg::TXO) * Cout + co);
  auto out_ptr = [&](int pl, int r, int xt) -> float* {
    const size_t o = ((size_t)((size_t)pl * Ho + r) * Wo + xt * XW) * Cout;
    return UBASE ? obase_u + o + olane : obase + o;
  };
  bool lane_ok[Cfg::XT];
#pragma unroll
  for (int xt = 0; xt < Cfg::XT; ++xt) lane_ok[xt] = (BAL ? xl + xt * XW < x_left : ox0 + xt * XW < Wo) && co < Cout;
  // the epilogue of N-tile n of stage st.  in_x(xt): is this lane's voxel of x run xt inside the volume - from the table where n is a
  // compile-time constant, computed where it is known only at run time (K split in four: n = 4 j + k)
  auto in_x_ct = [&](int xt) { return lane_ok[xt]; };
  auto in_x_rt = [&](int xt) { return (BAL ? xl + xt * XW < x_left : ox0 + xt * XW < Wo) && co < Cout; };
  auto store_tile = [&](int n, int st, const f32x4& a, auto in_x) {
    const int i = n % G, rx = n / G, xt = rx % Cfg::XT, r = rx / Cfg::XT;
    if (z0 + st * G + i >= z1 || oy0 + r >= Ho) return;            // wave-uniform
    if (!in_x(xt)) return;
    float4 o = F16 ? sf16_rescale4(a, out_mul, bv) : sbf_add4(sbf_f4(a), bv);
    if (act == CDS_ACT_RELU) o = sbf_relu4(o);
    if (F16) amax = sbf_amax4(amax, o);
    sbf_store4(out_ptr(st * G + i, r, xt), o);
  };
  unsigned char* xch = lds + Cfg::RINGB;                 // [buffer][sender wave][N-tile of its partner's half][lane] x 16 B
  constexpr int NH = NTW / 2;
  f32x4 acc[NTW];
  // K split in four with two rounds of weights per wave (112 registers): the finalising wave's own partial sum goes through the
  // exchange buffer too instead of staying in registers across the next K-loop
  constexpr bool KEEP4 = Cfg::RPW == 1;
  f32x4 keep[Cfg::KSPL == 2 ? NH : Cfg::NFIN];          // this wave's partial sums of the N-tiles it finalises, across the barrier
  const int xgrp = (wave / Cfg::KSPL) * NTW;            // first exchange slot row of this wave's (cout block, row part)
  // finish stage sp: bias / ReLU / store of this wave's outputs.  K split: N-tiles [k NH, (k + 1) NH) = round 0's partial sum +
  // round 1's (the partner's half arrived through exchange buffer sp & 1 before the stage barrier)
  auto finish = [&](int sp) {
    if (Cfg::KSPL == 2) {
      const unsigned char* src = xch + (sp & 1) * Cfg::XCH1 + ((wave ^ 1) * NH) * 1024 + lane * 16;
#pragma unroll
      for (int m = 0; m < NH; ++m) {
        const f32x4 o = *reinterpret_cast<const f32x4*>(src + m * 1024);
        store_tile(k * NH + m, sp, k == 0 ? keep[m] + o : o + keep[m], in_x_ct);
      }
    } else if (Cfg::KSPL == 4) {
#pragma unroll
      for (int jf = 0; jf < Cfg::NFIN; ++jf) {
        const int n = jf * 4 + k;
        if (n >= NTW) continue;                                      // wave-uniform
        const unsigned char* src = xch + (sp & 1) * Cfg::XCH1 + ((xgrp + n) * 4) * 1024 + lane * 16;
        f32x4 total = KEEP4 && k == 0 ? keep[jf] : *reinterpret_cast<const f32x4*>(src);
#pragma unroll
        for (int kk = 1; kk < 4; ++kk) total = total + (KEEP4 && kk == k ? keep[jf] : *reinterpret_cast<const f32x4*>(src + kk * 1024));
        store_tile(n, sp, total, in_x_rt);
      }
    } else {
#pragma unroll
      for (int n = 0; n < NTW; ++n) store_tile(n, sp, acc[n], in_x_ct);
    }
  };
  __syncthreads();                                     // #0
  for (int st = 0; st < nstages; ++st) {
    if (late && st > 0) finish(st - 1);
    // LDS byte offsets of this lane's operands.  PAIR: one per resident input plane (the tap row of a K-step is an immediate offset);
    // else one per (K-step, output plane): the four lane groups of a K-step sit in up to two planes (compile-time constants per lane
    // group: three selects per entry, no tables in registers)
    int vpl[PAIR ? Cfg::NRES : 1];
    int vaddr[PAIR ? 1 : KS][PAIR ? 1 : G];
    {
      int sl[Cfg::NRES];
      int slot = (st * S * G) % R;
#pragma unroll
      for (int u = 0; u < Cfg::NRES; ++u) {
        sl[u] = slot * Cfg::PLANEB;
        slot = slot + 1 >= R ? slot + 1 - R : slot + 1;
      }
      if (PAIR) {
#pragma unroll
        for (int u = 0; u < Cfg::NRES; ++u) vpl[u] = lane_base + sl[u];
      } else {
#pragma unroll
        for (int t = 0; t < KS; ++t)
#pragma unroll
          for (int i = 0; i < G; ++i) {
            const int o0 = sl[S * i + Cfg::tap_kz(t, 0)] + Cfg::tap_off(t, 0), o1 = sl[S * i + Cfg::tap_kz(t, 1)] + Cfg::tap_off(t, 1);
            const int o2 = sl[S * i + Cfg::tap_kz(t, 2)] + Cfg::tap_off(t, 2), o3 = sl[S * i + Cfg::tap_kz(t, 3)] + Cfg::tap_off(t, 3);
            vaddr[t][i] = lane_base + (g == 0 ? o0 : (g == 1 ? o1 : (g == 2 ? o2 : o3)));
          }
      }
    }
    constexpr int NGRP = NTW / NG, NS = RPW * KS * NGRP;   // the wave's rounds one after the other into the same accumulators
    constexpr int PF = Cfg::PF;
    BV bd[PF + 1][NG][NT];
    auto load_b = [&](int buf, int ss) {
      const int t = (ss / NGRP) % KS, rr = ss / (NGRP * KS), grp = ss % NGRP;
#pragma unroll
      for (int q = 0; q < NG; ++q) {
        const int n = grp * NG + q, i = n % G, rx = n / G, xt = rx % Cfg::XT, r = rx / Cfg::XT;
        // PAIR: K-step t = (kz, ky) = (t / 3, t % 3)
        const unsigned char* b = lds + (PAIR ? vpl[PAIR ? S * i + t / 3 : 0] + (t % 3) * Cfg::IXP * Cfg::PB : vaddr[PAIR ? 0 : t][PAIR ? 0 : i]) +
                                 (r * S * Cfg::IXP + xt * 16) * Cfg::PB + rr * Cfg::SLICEB;
        bd[buf][q][0].u = *reinterpret_cast<const uint4*>(b);
        bd[buf][q][1].u = *reinterpret_cast<const uint4*>(b + Cfg::TB);
        if (!F16) bd[buf][q][NT - 1].u = *reinterpret_cast<const uint4*>(b + 32);
      }
    };
    load_b(0, 0);
    if (PF == 2 && NS > 1) load_b(1, 1);
    // a wave that issues MFMAs back to back starves the other waves of its SIMD of issue slots (the producers' deposit went from
    // ~7000 to ~1100 cycles per stage once they outranked the consumers): the K-loop runs at the lowest priority, a consumer's
    // address set-up / exchange / epilogue above it, the producers above both
    __builtin_amdgcn_s_setprio(0);
#pragma unroll
    for (int t = 0; t < NTW; ++t) acc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ss = 0; ss < NS; ++ss) {
      const int t = ss / NGRP, grp = ss % NGRP, db = ss % (PF + 1);   // t = rr KS + K-step
      if (ss + PF < NS) load_b((ss + PF) % (PF + 1), ss + PF);
      __builtin_amdgcn_sched_barrier(0);
#ifndef CDS_ZMG_LAZYWAIT
      // ONE wait for all operands of this step (they were requested PF steps ago) instead of the compiler's lgkmcnt waits
      // BETWEEN the dependent MFMAs: an issue slot between two MFMAs on the same accumulator costs ~40 cycles of matrix pipe
      if (ss + PF < NS) __builtin_amdgcn_s_waitcnt(0xC07F | ((PF * NT * NG) << 8));   // lgkmcnt(PF NT NG): the next steps' requests stay in flight
      else if (PF == 2 && ss + 1 < NS) __builtin_amdgcn_s_waitcnt(0xC07F | ((NT * NG) << 8));
      else __builtin_amdgcn_s_waitcnt(0xC07F);
      __builtin_amdgcn_sched_barrier(0);
#endif
      if constexpr (F16) {
        SF16_TERMS(acc, grp * NG, NG, wres[t], bd[db]);
      } else {
        SBF_TERMS(acc, grp * NG, NG, wres[t], bd[db]);
      }
    }
    __builtin_amdgcn_s_setprio(CDS_ZMG_CPRIO);
    if (Cfg::KSPL == 2) {
      if (!late && st > 0) finish(st - 1);
      // partner's half -> exchange buffer (st & 1); own half stays in registers
      unsigned char* dst = xch + (st & 1) * Cfg::XCH1 + (wave * NH) * 1024 + lane * 16;
#pragma unroll
      for (int m = 0; m < NH; ++m) {
        *reinterpret_cast<f32x4*>(dst + m * 1024) = acc[(k ^ 1) * NH + m];
        keep[m] = acc[k * NH + m];
      }
    } else if (Cfg::KSPL == 4) {
      if (!late && st > 0) finish(st - 1);
      unsigned char* dst = xch + (st & 1) * Cfg::XCH1 + (xgrp * 4 + k) * 1024 + lane * 16;
#pragma unroll
      for (int n = 0; n < NTW; ++n) {
        if (KEEP4 && (n & 3) == k) keep[n >> 2] = acc[n];            // wave-uniform
        else *reinterpret_cast<f32x4*>(dst + n * 4096) = acc[n];
      }
    } else if (!late) {
      finish(st);
    }
    __syncthreads();                                   // #(st + 1)
  }
  if (Cfg::KSPL >= 2 || late) finish(nstages - 1);
  } while (BAL && walk.next_piece() && set_piece());
  if (F16) sf16_publish_bound(amax, out_bound);       // this wave's largest stored magnitude -> the bound the next layer scales by
}

// z segments per column: enough workgroups for the 256 CUs (one workgroup per CU: the ring takes most of the LDS) with full
// rounds of them, against the two or three stage times a segment spends filling its pipeline.
// cost_out: the model cost of the choice, < 0 where the knob forced it (the layer then keeps the uniform cutting).
inline int zmg_pick_nseg(int cols, int Do, int G, double* cost_out = nullptr) {
  const int nseg_env = cds_env_int("CDS_ZMG_NSEG", 0);   // A/B knob
  if (cost_out) *cost_out = -1.0;
  if (nseg_env > 0) return nseg_env;
  const int stages = cds_ceil_div(Do, G);
  int best = 1;
  double best_cost = 1e30;
  for (int n = 1; n <= 32 && n <= stages; ++n) {
    const int per = cds_ceil_div(stages, n);
    if (n > 1 && per < 6) break;
    const double cost = (double)cds_ceil_div(cols * cds_ceil_div(stages, per), 256) * (per + 2.5);
    if (cost < best_cost - 1e-9) { best_cost = cost; best = n; }
  }
  if (cost_out) *cost_out = best_cost;
  return best;
}

// The cutting of a layer of `cols` columns x ys cout splits: the uniform chooser's segments, and whether the balanced cutting runs
// instead (zm_common.hpp): each cout split is then cut over ncu / ys workgroups, so a workgroup keeps its weights.
struct ZmgPlan {
  int nseg, nwg;
  bool balanced;
  double ucost, bcost;
};
inline ZmgPlan zmg_plan(int cols, int ys, int Do, int G, int ncu, int balance) {
  ZmgPlan p;
  p.nseg = zmg_pick_nseg(cols * ys, Do, G, &p.ucost);
  p.nwg = max(1, ncu / ys);
  p.balanced = zm_choose_balanced(balance, p.ucost, cols, cds_ceil_div(Do, G), p.nwg, ZM_MINLEN_ZMG, 2.5, &p.bcost);
  return p;
}

template <class P>
int launch_zmg(const float* x, const void* wsp, const float* b, float* out, int Cout, int D, int H, int W, int act, hipStream_t st,
               const float* in_bound = nullptr, float w_inv = 1.f, float* out_bound = nullptr, int min_wgs = 0) {
  using Cfg = ZG<P>;
  constexpr int S = Cfg::S;
  const int Do = (D - 1) / S + 1, Ho = (H - 1) / S + 1, Wo = (W - 1) / S + 1;
  const int tx = cds_ceil_div(Wo, Cfg::TXO), ty = cds_ceil_div(Ho, Cfg::TYO);
  const ZmgPlan plan = zmg_plan(tx * ty, Cfg::YS, Do, Cfg::G, zm_ncu(), zm_balance_knob());
  int nseg = plan.nseg;
  const int zseg = cds_ceil_div(cds_ceil_div(Do, nseg), Cfg::G) * Cfg::G;
  nseg = cds_ceil_div(Do, zseg);
  if (min_wgs > 0 && tx * ty * nseg * Cfg::YS < min_wgs) return CDS_ZMG_UNSUPPORTED;   // too few columns to fill the chip
  if constexpr (P::BALANCED)
    if (plan.balanced)
      return cds_launch_lds<conv3d_zmg_kernel<Cfg, true>>(Cfg::LDSB, dim3(plan.nwg, Cfg::YS), dim3(Cfg::THREADS), Cfg::LDSB, st, x,
                                                          reinterpret_cast<const uint4*>(wsp), b, out, Cout, D, H, W, Do, Ho, Wo, act, tx,
                                                          ty, zseg, in_bound, w_inv, out_bound);
  return cds_launch_lds<conv3d_zmg_kernel<Cfg, false>>(Cfg::LDSB, dim3(tx * ty * nseg, Cfg::YS), dim3(Cfg::THREADS), Cfg::LDSB, st, x,
                                                       reinterpret_cast<const uint4*>(wsp), b, out, Cout, D, H, W, Do, Ho, Wo, act, tx, ty,
                                                       zseg, in_bound, w_inv, out_bound);
}

}  // namespace

// The plan of a layer for cds_zm_plan (deconv3d_zm.hip), on the host.
int cds_zmg_plan(int cols, int ys, int Do, int G, int ncu, int balance, int* nseg, double* ucost, double* bcost) {
  const ZmgPlan p = zmg_plan(cols, ys, Do, G, ncu, balance);
  *nseg = p.nseg, *ucost = p.ucost, *bcost = p.bcost;
  return p.balanced;
}

// Dispatch for cds_conv3d_sbf_f32 (conv3d_sbf.hip): returns CDS_ZMG_UNSUPPORTED when the shape stays on the tiled kernels.
// pair != 0: Cout == 8 with the pair-packed weights (ops.split_pack_conv3d_pair), stride 1.
int cds_conv3d_zmg_dispatch(const float* x, const void* wsp, const float* bias, float* out, int Cin, int Cout, int D, int H, int W,
                            int stride, int pair, int act, hipStream_t st, const float* in_bound, float w_inv, float* out_bound) {
  const bool f16 = in_bound != nullptr;   // split-f16 arithmetic, scales from device bounds (cds_conv3d_sf16_f32)
  // A/B knob CDS_ZMG=0: tiled kernels only (split-f16: for the deep layers only); read where it decides, a getenv is not free
  auto off = [] { return cds_env_is("CDS_ZMG", '0'); };
  if (!f16 && off()) return CDS_ZMG_UNSUPPORTED;
  auto run = [&](auto p, int min_wgs = 0) {
    return launch_zmg<decltype(p)>(x, wsp, bias, out, Cout, D, H, W, act, st, in_bound, w_inv, out_bound, min_wgs);
  };
  if (pair) {
    if (Cin == 8) return f16 ? run(ZgF16<ZgPair8>()) : run(ZgPair8());
    if (Cin == 16) return f16 ? run(ZgF16<ZgPair16>()) : run(ZgPair16());
    if (Cin == 32) return f16 ? run(ZgF16<ZgPair32>()) : run(ZgPair32());
    return CDS_ZMG_UNSUPPORTED;
  }
  if (stride == 2 && Cin == 8 && Cout == 16) return f16 ? run(ZgF16<ZgConv1>()) : run(ZgConv1());
  if (stride == 1 && Cin == 16 && Cout == 16) return f16 ? run(ZgConv2F16()) : run(ZgConv2());
  if (stride == 2 && Cin == 16 && Cout == 32) return f16 ? run(ZgConv3F16()) : run(ZgConv3());
  if (!f16) return CDS_ZMG_UNSUPPORTED;
  // The deep layers (conv4 32 -> 32, conv5 32 -> 64 stride 2, conv6 64 -> 64), split-f16 only.  CDS_ZMG_DEEP (A/B knob): 0 = tiled
  // kernels, 1 = z-march where columns x segments fill the 256 CUs (the few tiles of the cascade stages' deep layers stay on the
  // tiled kernels and their cout split), 2 = z-march whatever the size.
  const int deep = off() ? 0 : cds_env_int("CDS_ZMG_DEEP", 1);
  const int min_wgs = deep == 2 ? 0 : 256;
  if (deep <= 0) return CDS_ZMG_UNSUPPORTED;
  if (stride == 1 && Cin == 32 && Cout == 32) return run(ZgConv4F16(), min_wgs);
  if (stride == 2 && Cin == 32 && Cout == 64) return run(ZgConv5F16(), min_wgs);
  if (stride == 1 && Cin == 64 && Cout == 64) return run(ZgConv6F16(), min_wgs);
  return CDS_ZMG_UNSUPPORTED;
}
