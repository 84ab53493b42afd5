// Evaluation views from decoded bytes, and the side outputs of a depth map (reference: datasets/general_eval.py:88-118 - np.array(img,
// float32) / 255., the Tanks & Temples edge padding, cv2.resize of the float32 image to max_w x max_h - and test.py:216-248 - the three
// stage confidences and the image nearest-resized to the depth map's size, the image written as uint8).
//
// cds_eval_views_u8: the loader uploads the uint8 pixels as PIL decoded them; one launch does the division, the row padding (folded
// into the row tables as a clamp, no padded copy exists), OpenCV's float32 INTER_LINEAR and the HWC -> CHW transpose.  The arithmetic
// is OpenCV's generic (non-SIMD-reordered) path: horizontal pass S[s0] * (1.f - fx) + S[s1] * fx rounded to float32, then the vertical
// pass R0 * (1.f - fy) + R1 * fy.  EVERY multiply, add and subtract is rounded separately: they are written as __fmul_rn / __fadd_rn /
// __fsub_rn, which the compiler never contracts into an FMA (the file is also built with -ffp-contract=off like the rest of the
// library), so numpy float32 arithmetic in the same order reproduces the result bit for bit.  With every f = 0 (the padded source
// already has the target size) the output is exactly u8 / 255.  1 byte read and 4 bytes written per element, no LDS, no atomics.
//
// cds_eval_outputs_f32: one launch gathers the three confidence maps (each at its own resolution) and the reference image through
// nearest-neighbour index tables built on the host (mvs_io.nearest_resize's rule), writes conf3 [h][w][3] and the image as
// uint8(clip(v * 255.0f, 0, 255)): one rounded float32 multiply, then truncation, which is what numpy does for a float32 array.
#include "cds_common.hpp"

namespace {

constexpr int EV_K = 4;        // consecutive x of one output row per thread: one 16-byte store per channel plane

__device__ __forceinline__ int ev_clamp(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// one channel of one pixel: the four taps as bytes -> the two passes
__device__ __forceinline__ float ev_lerp2(unsigned a00, unsigned a01, unsigned a10, unsigned a11, float gx, float fx, float gy, float fy) {
  const float r0 = __fadd_rn(__fmul_rn((float)a00 / 255.0f, gx), __fmul_rn((float)a01 / 255.0f, fx));
  const float r1 = __fadd_rn(__fmul_rn((float)a10 / 255.0f, gx), __fmul_rn((float)a11 / 255.0f, fx));
  return __fadd_rn(__fmul_rn(r0, gy), __fmul_rn(r1, fy));
}

// Work item q = ((v * h) + y) * wq + xg with wq = ceil(w / 4): view v, output row y, columns 4 xg .. 4 xg + 3 (the scheme of
// image_batch_kernel, csrc/train_data.hip).  Table entries are clamped to the source here, so no table can take a read out of bounds
// (the host builds them in bounds; this is the guard).  vec: w % 4 == 0 and `out` is 16-byte aligned.
__global__ __launch_bounds__(256) void eval_views_kernel(const unsigned char* __restrict__ src, int Hs, int Ws,
                                                         const int* __restrict__ row0, const int* __restrict__ row1,
                                                         const float* __restrict__ fyt, const int* __restrict__ col0,
                                                         const int* __restrict__ col1, const float* __restrict__ fxt, int h, int w, int wq,
                                                         long long items, int vec, float* __restrict__ out) {
  const size_t plane = (size_t)h * (size_t)w;
  for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < items; q += (long long)gridDim.x * 256) {
    const long long iy = q / wq;
    const int xg = (int)(q - iy * wq);
    const long long i = iy / h;
    const int y = (int)(iy - i * h);
    const int x0 = xg * EV_K;
    const float fy = fyt[y];
    const float gy = __fsub_rn(1.0f, fy);
    const unsigned char* __restrict__ img = src + (size_t)i * Hs * (size_t)Ws * 3;
    const unsigned char* __restrict__ line0 = img + (size_t)ev_clamp(row0[y], Hs - 1) * (size_t)Ws * 3;
    const unsigned char* __restrict__ line1 = img + (size_t)ev_clamp(row1[y], Hs - 1) * (size_t)Ws * 3;
    float v[3][EV_K];
#pragma unroll
    for (int j = 0; j < EV_K; ++j) {
      const int x = x0 + j < w ? x0 + j : w - 1;              // a lane past the row repeats its last pixel; it is never stored
      const size_t s0 = (size_t)ev_clamp(col0[x], Ws - 1) * 3, s1 = (size_t)ev_clamp(col1[x], Ws - 1) * 3;
      const float fx = fxt[x];
      const float gx = __fsub_rn(1.0f, fx);
#pragma unroll
      for (int c = 0; c < 3; ++c)
        v[c][j] = ev_lerp2(line0[s0 + c], line0[s1 + c], line1[s0 + c], line1[s1 + c], gx, fx, gy, fy);
    }
    float* __restrict__ o = out + (size_t)i * 3 * plane + (size_t)y * w + x0;
    if (vec) {
#pragma unroll
      for (int c = 0; c < 3; ++c)
        *reinterpret_cast<float4*>(o + c * plane) = make_float4(v[c][0], v[c][1], v[c][2], v[c][3]);
    } else {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
#pragma unroll
        for (int j = 0; j < EV_K; ++j)
          if (x0 + j < w) o[c * plane + j] = v[c][j];
      }
    }
  }
}

struct EvalOutSrc {
  const float* c[3];           // stage confidences [Hk][Wk]
  int H[3], W[3];
  const float* img;            // [3][Hi][Wi]
  int Hi, Wi;
};

// Work item q = y * wq + xg: output row y, columns 4 xg .. 4 xg + 3.  tab = ys1 ys2 ys3 ysI [h each], xs1 xs2 xs3 xsI [w each].  The
// thread's 4 pixels are 48 contiguous bytes of conf3 and 12 of img_u8: vec (w % 4 == 0, conf3 16-byte and img_u8 4-byte aligned)
// writes them as three 16-byte and three 4-byte stores.
__global__ __launch_bounds__(256) void eval_outputs_kernel(EvalOutSrc s, const int* __restrict__ tab, int h, int w, int wq, long long items,
                                                           int vec, float* __restrict__ conf3, unsigned char* __restrict__ img_u8) {
  const int* __restrict__ xtab = tab + 4 * (size_t)h;
  for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < items; q += (long long)gridDim.x * 256) {
    const int y = (int)(q / wq);
    const int x0 = (int)(q - (long long)y * wq) * EV_K;
    float cf[EV_K * 3];
    unsigned char px[EV_K * 3];
#pragma unroll
    for (int j = 0; j < EV_K; ++j) {
      const int x = x0 + j < w ? x0 + j : w - 1;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const int sy = ev_clamp(tab[(size_t)k * h + y], s.H[k] - 1), sx = ev_clamp(xtab[(size_t)k * w + x], s.W[k] - 1);
        cf[j * 3 + k] = s.c[k][(size_t)sy * s.W[k] + sx];
      }
      const int sy = ev_clamp(tab[3 * (size_t)h + y], s.Hi - 1), sx = ev_clamp(xtab[3 * (size_t)w + x], s.Wi - 1);
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float t = __fmul_rn(s.img[((size_t)c * s.Hi + sy) * s.Wi + sx], 255.0f);
        px[j * 3 + c] = (unsigned char)(int)fminf(fmaxf(t, 0.0f), 255.0f);
      }
    }
    const size_t at = ((size_t)y * w + x0) * 3;
    if (vec) {
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        *reinterpret_cast<float4*>(conf3 + at + 4 * k) = make_float4(cf[4 * k], cf[4 * k + 1], cf[4 * k + 2], cf[4 * k + 3]);
        *reinterpret_cast<unsigned*>(img_u8 + at + 4 * k) =
            (unsigned)px[4 * k] | ((unsigned)px[4 * k + 1] << 8) | ((unsigned)px[4 * k + 2] << 16) | ((unsigned)px[4 * k + 3] << 24);
      }
    } else {
#pragma unroll
      for (int j = 0; j < EV_K; ++j) {
        if (x0 + j < w) {
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            conf3[at + j * 3 + c] = cf[j * 3 + c];
            img_u8[at + j * 3 + c] = px[j * 3 + c];
          }
        }
      }
    }
  }
}

inline unsigned ev_blocks(long long items) {
  const long long blocks = (items + 255) / 256;
  return (unsigned)(blocks > 16384 ? 16384 : blocks);
}

}  // namespace

// src [V][Hs][Ws][3] uint8; row0, row1 [h], col0, col1 [w] int32 and fy [h], fx [w] fp32 on the DEVICE; out [V][3][h][w] fp32.
extern "C" int cds_eval_views_u8(const unsigned char* src, int V, int Hs, int Ws, const int* row0, const int* row1, const float* fy,
                                 const int* col0, const int* col1, const float* fx, int h, int w, float* out, void* stream) {
  if (!src || !row0 || !row1 || !fy || !col0 || !col1 || !fx || !out || V < 1 || Hs < 1 || Ws < 1 || h < 1 || w < 1) return CDS_EINVAL;
  const void* words[] = {row0, row1, fy, col0, col1, fx, out};
  for (const void* p : words)
    if (reinterpret_cast<uintptr_t>(p) & 3) return CDS_EINVAL;
  const int wq = (w + EV_K - 1) / EV_K;
  const long long items = (long long)V * h * wq;
  const int vec = (w % EV_K == 0) && (reinterpret_cast<uintptr_t>(out) & 15) == 0;
  hipLaunchKernelGGL(eval_views_kernel, dim3(ev_blocks(items)), dim3(256), 0, (hipStream_t)stream, src, Hs, Ws, row0, row1, fy, col0, col1,
                     fx, h, w, wq, items, vec, out);
  return cds_launch_status();
}

// c1 [H1][W1], c2 [H2][W2], c3 [H3][W3], img [3][Hi][Wi] fp32; tab [4 h + 4 w] int32 on the DEVICE; conf3 [h][w][3] fp32,
// img_u8 [h][w][3] uint8.
extern "C" int cds_eval_outputs_f32(const float* c1, int H1, int W1, const float* c2, int H2, int W2, const float* c3, int H3, int W3,
                                    const float* img, int Hi, int Wi, const int* tab, int h, int w, float* conf3, unsigned char* img_u8,
                                    void* stream) {
  if (!c1 || !c2 || !c3 || !img || !tab || !conf3 || !img_u8 || h < 1 || w < 1) return CDS_EINVAL;
  if (H1 < 1 || W1 < 1 || H2 < 1 || W2 < 1 || H3 < 1 || W3 < 1 || Hi < 1 || Wi < 1) return CDS_EINVAL;
  const void* words[] = {c1, c2, c3, img, tab, conf3};
  for (const void* p : words)
    if (reinterpret_cast<uintptr_t>(p) & 3) return CDS_EINVAL;
  EvalOutSrc s;
  s.c[0] = c1; s.H[0] = H1; s.W[0] = W1;
  s.c[1] = c2; s.H[1] = H2; s.W[1] = W2;
  s.c[2] = c3; s.H[2] = H3; s.W[2] = W3;
  s.img = img; s.Hi = Hi; s.Wi = Wi;
  const int wq = (w + EV_K - 1) / EV_K;
  const long long items = (long long)h * wq;
  const int vec = (w % EV_K == 0) && (reinterpret_cast<uintptr_t>(conf3) & 15) == 0 && (reinterpret_cast<uintptr_t>(img_u8) & 3) == 0;
  hipLaunchKernelGGL(eval_outputs_kernel, dim3(ev_blocks(items)), dim3(256), 0, (hipStream_t)stream, s, tab, h, w, wq, items, vec, conf3,
                     img_u8);
  return cds_launch_status();
}
