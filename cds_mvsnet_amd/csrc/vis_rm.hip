// Visibility CNN (models/model.py:14,51) in ONE kernel that marches down the rows: cat(entropy, ref_nc) -> 3x3 2 -> 16 + ReLU ->
// 3x3 16 -> 16 + ReLU -> 3x3 16 -> 16 + ReLU -> 1x1 head 16 -> 1 + sigmoid, 8 bytes per pixel in, 4 bytes out.  The three launches
// it replaces (vis_layer1_cl_kernel and twice dynconv_cl_kernel<16,3,0,0,2>, feat_cl.hip) hand two [V][h][w][16] fp32 activations
// through memory; here they live in two LDS rings of four rows, already in the three-term bf16 position format of sbf_common.hpp
// (the split of an fp32 value is exact, so the hand-over loses nothing and the result is BIT-EQUAL to the three launches: layer 1
// is the same fmaf chain ci, ky, kx, layers 2 / 3 take the same K-steps and the same six products in the same order into one
// accumulator, the head is MODE 2's epilogue).
//
// Unit of work (numbered through cds_xcd_remap): view x column strip of VR_OWN = 60 output pixels x row segment [y0, y1).  Along x
// layer 2 is needed one pixel wider per side (62, four MFMA M-tiles) and layer 1 two (64 = the lanes of a wave); along y nothing is
// recomputed inside a segment, a segment only primes its rings.  Four waves, one barrier per step t:
//   every wave w  layer-1 row t, channels 4 w .. 4 w + 3 of all 64 positions (lane = position), from input rows t - 1 .. t + 1 (registers:
//                 a 3 x 3 window per map, one new row per step); its 72 weights are wave-uniform
//   waves 0 1     layer-2 row t - 2 from layer-1 rows t - 3 .. t - 1 (two M-tiles each)
//   waves 2 3     layer-3 row t - 4 from layer-2 rows t - 5 .. t - 3, head, sigmoid, store
// Layer 1 is VALU work (288 multiply-adds per position) and is spread over the four waves, i.e. the four SIMDs, so that it runs under
// the MFMAs of the other workgroups' waves on each of them; one producer wave of its own would put all of it on the SIMD it lands on.
// Row r of a ring lives in slot r & 3: the slot written in step t (row t resp. t - 2) held the row that was last read in step t - 1,
// and the barrier that ends step t - 1 lies between.  A layer-1 / layer-2 position OUTSIDE THE IMAGE holds zero (the next layer's zero
// padding), not the convolution evaluated there: rows < 0 or >= h, columns < 0 or >= w, a segment's priming rows included.  Every
// wave runs every step and every barrier; what a step has no row for is skipped by wave-uniform branches that contain no barrier.
// Operand roles as in feat_cl.hip (read the comment there): A = data from LDS, B = weights, held in registers for the whole march.
#include "zm_common.hpp"

namespace {

constexpr int VR_OWN = 60;                     // output columns of a strip; layer 2: 62 of 64 rows of four M-tiles, layer 1: 64
constexpr int VR_IXP = 66;                     // positions of a ring row: 64 written + 2 that only the discarded M-tile rows read
constexpr int VR_SLICEB = VR_IXP * POSB;       // one 8-channel slice of a row
constexpr int VR_ROWB = 2 * VR_SLICEB;
constexpr int VR_RINGB = 4 * VR_ROWB;          // four rows: three being read, one being written
constexpr int VR_NTHR = 256;
constexpr int VR_WG_PER_CU = 3;                // 50 KB of LDS each, three waves per SIMD (launch bounds below)

// sum over the 16 lanes of a DPP row (feat_cl.hip's row16_sum: the same four additions in the same order)
__device__ __forceinline__ float vr_row16_sum(float v) {
  v += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0xB1, 0xf, 0xf, true));   // quad_perm [1,0,3,2]
  v += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x4E, 0xf, 0xf, true));   // quad_perm [2,3,0,1]
  v += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x141, 0xf, 0xf, true));  // row_half_mirror
  v += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x140, 0xf, 0xf, true));  // row_mirror
  return v;
}

// three neighbours x - 1 .. x + 1 of row r of one map as they lie in memory: unconditional loads from a clamped row (wave-uniform
// part of the address) and clamped columns xcl[c] (they do not change during the march).  The caller replaces what lies outside the
// image by zero where it USES the values, one step later: a select next to the load would let the compiler put the load under a branch
// with the wait for it right behind
__device__ __forceinline__ void vr_load3(const float* __restrict__ map, int r, int H, int W, const unsigned (&xcl)[3], float (&o)[3]) {
  const float* __restrict__ rowp = map + min(max(r, 0), H - 1) * W;
#pragma unroll
  for (int c = 0; c < 3; ++c) o[c] = rowp[xcl[c]];
}

__device__ __forceinline__ void vr_fetch(const unsigned char* a, BV (&d)[3]) {
  d[0].u = *reinterpret_cast<const uint4*>(a);
  d[1].u = *reinterpret_cast<const uint4*>(a + 16);
  d[2].u = *reinterpret_cast<const uint4*>(a + 32);
}

__global__ __launch_bounds__(VR_NTHR, 3) void vis_rm_kernel(const float* __restrict__ ent, const float* __restrict__ nc,
                                                            const float* __restrict__ w0, const float* __restrict__ b0,
                                                            const uint4* __restrict__ ws1, const float* __restrict__ b1,
                                                            const uint4* __restrict__ ws2, const float* __restrict__ b2,
                                                            const float* __restrict__ head_w, const float* __restrict__ head_b,
                                                            float* __restrict__ out, int V, int H, int W, int strips, int seg_len) {
  __shared__ __attribute__((aligned(16))) unsigned char lds[2 * VR_RINGB];     // layer-1 ring | layer-2 ring
  const int unit = cds_xcd_remap(blockIdx.x, gridDim.x);
  const int per_seg = strips * V;
  const int seg = unit / per_seg, col = unit - seg * per_seg;
  const int img = col / strips, xs = (col - img * strips) * VR_OWN;
  const int y0 = seg * seg_len, y1 = min(H, y0 + seg_len);
  if (y0 >= y1) return;                        // a unit with no rows: the whole workgroup, before the first barrier
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int m = lane & 15, g = lane >> 4;
  // positions 64, 65 of every row and slice are never written by the march: defined values for the M-tile rows that read them (their
  // results are discarded).  The first reader runs three barriers later.
  if (tid < 2 * 4 * 2 * 2 * 3) {
    const int term = tid % 3, p = (tid / 3) & 1, rs = tid / 6;           // rs = (ring, slot, slice)
    *reinterpret_cast<uint4*>(lds + rs * VR_SLICEB + (64 + p) * POSB + term * 16) = make_uint4(0u, 0u, 0u, 0u);
  }
  const size_t img_off = (size_t)img * H * W;

  // ---- layer 1: lane = position, x = xs - 2 + lane; this wave's four channels ----
  const float* __restrict__ e_img = ent + img_off;
  const float* __restrict__ n_img = nc + img_off;
  const int x = xs - 2 + lane;
  const bool xin = (unsigned)x < (unsigned)W;
  const float* __restrict__ w0w = w0 + wave * 4;
  const float4 b0w = *reinterpret_cast<const float4*>(b0 + wave * 4);
  unsigned xcl[3];
  bool cok[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    cok[c] = (unsigned)(x - 1 + c) < (unsigned)W;
    xcl[c] = cok[c] ? x - 1 + c : 0;
  }
  // [map][input row t - 1 .. t + 1][x - 1 .. x + 1], and the row that enters the window in the NEXT step: its loads have a whole step
  float win[2][3][3], nxt[2][3];
#pragma unroll
  for (int k = 1; k < 3; ++k) {
    const bool rin = (unsigned)(y0 - 4 + k) < (unsigned)H;
    vr_load3(e_img, y0 - 4 + k, H, W, xcl, win[0][k]);
    vr_load3(n_img, y0 - 4 + k, H, W, xcl, win[1][k]);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      win[0][k][c] = rin && cok[c] ? win[0][k][c] : 0.f;
      win[1][k][c] = rin && cok[c] ? win[1][k][c] : 0.f;
    }
  }
  vr_load3(e_img, y0 - 1, H, W, xcl, nxt[0]);
  vr_load3(n_img, y0 - 1, H, W, xcl, nxt[1]);
  unsigned char* l1dst = lds + (wave >> 1) * VR_SLICEB + lane * POSB + (wave & 1) * 8;

  // ---- layers 2 / 3: waves 0, 1 layer 2 (row t - 2), waves 2, 3 layer 3 (row t - 4); M-tiles 2 cw, 2 cw + 1 of the row ----
  const bool l3 = wave >= 2;
  const int cw = wave & 1, lag = l3 ? 4 : 2;
  const unsigned char* src = lds + (l3 ? VR_RINGB : 0);
  BV wt[6][3];                                 // [K-step = slice * 3 + t][term]: this layer's weights, for the whole march
  {
    const uint4* __restrict__ wl = (l3 ? ws2 : ws1) + lane;
#pragma unroll
    for (int ks = 0; ks < 6; ++ks)
#pragma unroll
      for (int term = 0; term < 3; ++term) wt[ks][term].u = wl[(ks * 3 + term) * 64];
  }
  const float bv = (l3 ? b2 : b1)[m];
  const float hw_n = head_w[m], hb = head_b[0];
  // A operand: lane (m, g) supplies the 8 channels of tap 4 t + g for pixel m of its M-tile: source position m + kx, source row + ky
  int a_off[3], a_ky[3];
#pragma unroll
  for (int t = 0; t < 3; ++t) {
    int tap = 4 * t + g;
    if (tap > 8) tap = 8;                      // padded tap slots carry zero weights: any staged position
    a_ky[t] = tap / 3;
    a_off[t] = (cw * 32 + m + (tap - a_ky[t] * 3)) * POSB;
  }
  float* __restrict__ o_img = out + img_off;

  for (int t = y0 - 2; t < y1 + 4; ++t) {
    if (t <= y1 + 1) {                         // layer-1 rows y0 - 2 .. y1 + 1
      const bool rin1 = (unsigned)(t + 1) < (unsigned)H;    // the row that enters the window
#pragma unroll
      for (int ci = 0; ci < 2; ++ci)
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
          win[ci][0][kx] = win[ci][1][kx];
          win[ci][1][kx] = win[ci][2][kx];
          win[ci][2][kx] = rin1 && cok[kx] ? nxt[ci][kx] : 0.f;
        }
      vr_load3(e_img, t + 2, H, W, xcl, nxt[0]);
      vr_load3(n_img, t + 2, H, W, xcl, nxt[1]);
      float a1[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int k = 0; k < 18; ++k) {           // k = ci * 9 + ky * 3 + kx: the order of vis_layer1_cl_kernel
        const float v = win[k / 9][(k % 9) / 3][k % 3];
        const float4 w = *reinterpret_cast<const float4*>(w0w + k * 16);
        a1[0] = fmaf(v, w.x, a1[0]);
        a1[1] = fmaf(v, w.y, a1[1]);
        a1[2] = fmaf(v, w.z, a1[2]);
        a1[3] = fmaf(v, w.w, a1[3]);
      }
      const bool in = xin && (unsigned)t < (unsigned)H;     // outside the image: zero, not ReLU(bias + partial taps)
      const float o0 = in ? fmaxf(a1[0] + b0w.x, 0.f) : 0.f, o1 = in ? fmaxf(a1[1] + b0w.y, 0.f) : 0.f;
      const float o2 = in ? fmaxf(a1[2] + b0w.z, 0.f) : 0.f, o3 = in ? fmaxf(a1[3] + b0w.w, 0.f) : 0.f;
      uint32_t h0, m0, l0, h1, m1, l1;
      split2(o0, o1, h0, m0, l0);
      split2(o2, o3, h1, m1, l1);
      unsigned char* d = l1dst + (t & 3) * VR_ROWB;
      *reinterpret_cast<uint2*>(d) = make_uint2(h0, h1);
      *reinterpret_cast<uint2*>(d + 16) = make_uint2(m0, m1);
      *reinterpret_cast<uint2*>(d + 32) = make_uint2(l0, l1);
    }
    const int r = t - lag;                     // the row of layer 2 / 3 this wave computes
    if (l3 ? (r >= y0 && r < y1) : (r >= y0 - 1 && r <= y1)) {
      f32x4 acc[2] = {(f32x4){0.f, 0.f, 0.f, 0.f}, (f32x4){0.f, 0.f, 0.f, 0.f}};
      const int s0 = ((r - 1) & 3) * VR_ROWB, s1 = (r & 3) * VR_ROWB, s2 = ((r + 1) & 3) * VR_ROWB;
      // twelve half-steps h = (K-step = slice * 3 + kt, M-tile q): the operands of half-step h + 1 are fetched under the six MFMAs of
      // half-step h.  Each accumulator still takes its K-steps and its six products in the order of feat_cl.hip's K-loop.
      BV ax[2][3];                             // [h & 1][hi, mid, lo]
      const unsigned char* ap[3];              // per kt: this lane's tap of M-tile 0 in slice 0
#pragma unroll
      for (int kt = 0; kt < 3; ++kt) ap[kt] = src + (a_ky[kt] == 0 ? s0 : a_ky[kt] == 1 ? s1 : s2) + a_off[kt];
      vr_fetch(ap[0], ax[0]);
#pragma unroll
      for (int h = 0; h < 12; ++h) {
        if (h < 11) vr_fetch(ap[((h + 1) >> 1) % 3] + ((h + 1) / 6) * VR_SLICEB + ((h + 1) & 1) * 16 * POSB, ax[(h + 1) & 1]);
        __builtin_amdgcn_sched_barrier(0);
        const BV(&w)[3] = wt[h >> 1];
        const BV(&x)[3] = ax[h & 1];
        f32x4& c = acc[h & 1];
        SBF_MFMA(c, x[2], w[0]);               // order 2^-16 terms first
        SBF_MFMA(c, x[1], w[1]);
        SBF_MFMA(c, x[0], w[2]);
        SBF_MFMA(c, x[1], w[0]);               // 2^-8
        SBF_MFMA(c, x[0], w[1]);
        SBF_MFMA(c, x[0], w[0]);               // leading term
        __builtin_amdgcn_sched_barrier(0);
      }
      // lane (m, g) holds channel m of positions p = 32 cw + 16 q + 4 g + i of the row
      if (!l3) {
        // layer 2: bias + ReLU, zero outside the image, exact split, into the layer-2 ring; position p is column xs - 1 + p
        const bool rin = (unsigned)r < (unsigned)H;
        unsigned char* d0 = lds + VR_RINGB + (r & 3) * VR_ROWB + (m >> 3) * VR_SLICEB + (m & 7) * 2;
#pragma unroll
        for (int q = 0; q < 2; ++q) {
          const f32x4 a = acc[q];
          const int p = cw * 32 + q * 16 + g * 4, gx = xs - 1 + p;
          float v[4] = {fmaxf(a.x + bv, 0.f), fmaxf(a.y + bv, 0.f), fmaxf(a.z + bv, 0.f), fmaxf(a.w + bv, 0.f)};
#pragma unroll
          for (int i = 0; i < 4; ++i)
            if (!(rin && (unsigned)(gx + i) < (unsigned)W)) v[i] = 0.f;
#pragma unroll
          for (int i = 0; i < 4; i += 2) {
            uint32_t s[3];
            split2(v[i], v[i + 1], s[0], s[1], s[2]);
            unsigned char* d = d0 + (p + i) * POSB;
#pragma unroll
            for (int term = 0; term < 3; ++term) {
              *reinterpret_cast<uint16_t*>(d + term * 16) = (uint16_t)(s[term] & 0xffffu);
              *reinterpret_cast<uint16_t*>(d + POSB + term * 16) = (uint16_t)(s[term] >> 16);
            }
          }
        }
      } else {
        // layer 3: bias + ReLU, head dot over the 16 channels of a DPP row, sigmoid (feat_cl.hip MODE 2); position p is column xs + p.
        // After the sums every lane of a row holds all eight of them: lane m takes the sigmoid of sum m & 7 only and lanes m < 8 store
        float sum[8];
#pragma unroll
        for (int q = 0; q < 2; ++q) {
          const f32x4 a = acc[q];
          const float v[4] = {fmaxf(a.x + bv, 0.f), fmaxf(a.y + bv, 0.f), fmaxf(a.z + bv, 0.f), fmaxf(a.w + bv, 0.f)};
#pragma unroll
          for (int i = 0; i < 4; ++i) sum[q * 4 + i] = vr_row16_sum(v[i] * hw_n) + hb;
        }
        const int sel = m & 7;                 // (q, i) = (sel >> 2, sel & 3)
        float sacc = sum[0];
#pragma unroll
        for (int k = 1; k < 8; ++k) sacc = sel == k ? sum[k] : sacc;
        const float vis = 1.0f / (1.0f + expf(-sacc));
        const int p = cw * 32 + (sel >> 2) * 16 + g * 4 + (sel & 3);
        if (m < 8 && p < VR_OWN && xs + p < W) o_img[(size_t)r * W + xs + p] = vis;
      }
    }
    __syncthreads();
  }
}

}  // namespace

// cds_vis_cnn_rm_f32: the whole visibility CNN in one launch.  entropy, ref_nc [V][H][W]; w0 [2][9][16] (cout fastest) / b0 [16]:
// layer 1 as cds_vis_layer1_cl_f32 takes them; ws1, ws2 = ops.split_pack_dynconv([w]) of the two [16][16][3][3] layers with their
// biases b1, b2 [16]; head_w [16], head_b [1]; out [V][H][W], bit-equal to cds_vis_layer1_cl_f32 + 2 x cds_conv2d_k3_relu_cl_f32.
// CDS_VIS_NSEG: number of row segments (A/B and test knob; default zm_pick_nseg).
extern "C" int cds_vis_cnn_rm_f32(const float* entropy, const float* ref_nc, const float* w0, const float* b0, const void* ws1,
                                  const float* b1, const void* ws2, const float* b2, const float* head_w, const float* head_b,
                                  float* out, int V, int H, int W, void* stream) {
  if (!entropy || !ref_nc || !w0 || !b0 || !ws1 || !b1 || !ws2 || !b2 || !head_w || !head_b || !out || V < 1 || H < 1 || W < 1)
    return CDS_EINVAL;
  if ((long long)H * W > 0x7fffffffLL) return CDS_EINVAL;      // per-view element offsets are ints
  const int strips = cds_ceil_div(W, VR_OWN);
  if ((long long)strips * V > (1 << 24)) return CDS_EINVAL;
  const int nseg = zm_pick_nseg(cds_ceil_div(strips * V, VR_WG_PER_CU), H, 64, "CDS_VIS_NSEG");
  const int seg_len = cds_ceil_div(H, nseg);
  const long long units = (long long)strips * V * cds_ceil_div(H, seg_len);
  if (units > 0x7fffffffLL) return CDS_EINVAL;
  hipLaunchKernelGGL(vis_rm_kernel, dim3((unsigned)units), dim3(VR_NTHR), 0, (hipStream_t)stream, entropy, ref_nc, w0, b0,
                     reinterpret_cast<const uint4*>(ws1), b1, reinterpret_cast<const uint4*>(ws2), b2, head_w, head_b, out, V, H, W,
                     strips, seg_len);
  return cds_launch_status();
}
