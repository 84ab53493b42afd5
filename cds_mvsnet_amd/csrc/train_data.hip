// Training images from decoded bytes (reference: datasets/dtu_yao.py:73-77,176 and datasets/blended_dataset.py:79-92,165 -
// np.array(img, float32) / 255., centre crop, stack, transpose(0, 3, 1, 2) on the host, then the upload of 4 bytes per element).  Here
// the loader uploads the uint8 pixels as PIL decoded them, and one launch does the crop (a gather through the row / column tables of
// gt_pyramid), the HWC -> CHW transpose and the division: 1 byte read and 4 bytes written per element, no LDS, no atomics.
#include "cds_common.hpp"

namespace {

constexpr int IB_K = 4;        // consecutive x of one output row per thread: one 16-byte store per channel plane

// Work item q = ((i * h) + y) * wq + xg with wq = ceil(w / 4): image i, output row y, columns 4 xg .. 4 xg + 3.  The thread reads the
// 3 bytes of each of its pixels once (byte loads: a 3-byte pixel sits at any alignment, and the tables need not be contiguous), divides
// - a true fp32 division, x * (1 / 255.f) differs from numpy's x / 255. in the last bit for 126 of the 256 byte values - and writes the
// three planes.  vec: w % 4 == 0 and `out` is 16-byte aligned, so every group of four starts on a 16-byte boundary; otherwise scalar
// stores, bounded by w.  A table entry outside the source gives 0 (the host wrapper refuses such tables; this keeps the read in bounds).
__global__ __launch_bounds__(256) void image_batch_kernel(const unsigned char* __restrict__ src, int Hs, int Ws,
                                                          const int* __restrict__ rows, const int* __restrict__ cols, int h, int w, int wq,
                                                          long long items, int vec, float* __restrict__ out) {
  const size_t plane = (size_t)h * (size_t)w;
  for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < items; q += (long long)gridDim.x * 256) {
    const long long iy = q / wq;
    const int xg = (int)(q - iy * wq);
    const long long i = iy / h;
    const int y = (int)(iy - i * h);
    const int x0 = xg * IB_K;
    const int sy = rows[y];
    const bool row_ok = (unsigned)sy < (unsigned)Hs;
    const unsigned char* __restrict__ line = src + ((size_t)i * Hs + (size_t)(row_ok ? sy : 0)) * (size_t)Ws * 3;
    float v[3][IB_K];
#pragma unroll
    for (int j = 0; j < IB_K; ++j) {
      const int x = x0 + j;
      unsigned b0 = 0u, b1 = 0u, b2 = 0u;
      if (x < w) {
        const int sx = cols[x];
        if (row_ok && (unsigned)sx < (unsigned)Ws) {
          const unsigned char* __restrict__ p = line + (size_t)sx * 3;
          b0 = p[0]; b1 = p[1]; b2 = p[2];
        }
      }
      v[0][j] = (float)b0 / 255.0f;
      v[1][j] = (float)b1 / 255.0f;
      v[2][j] = (float)b2 / 255.0f;
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
        for (int j = 0; j < IB_K; ++j)
          if (x0 + j < w) o[c * plane + j] = v[c][j];
      }
    }
  }
}

}  // namespace

// src [n][Hs][Ws][3] uint8; rows [h], cols [w] int32 on the DEVICE; out [n][3][h][w] fp32.
extern "C" int cds_image_batch_u8(const unsigned char* src, int n, int Hs, int Ws, const int* rows, const int* cols, int h, int w,
                                  float* out, void* stream) {
  if (!src || !rows || !cols || !out || n < 1 || Hs < 1 || Ws < 1 || h < 1 || w < 1) return CDS_EINVAL;
  if ((reinterpret_cast<uintptr_t>(out) & 3) || (reinterpret_cast<uintptr_t>(rows) & 3) || (reinterpret_cast<uintptr_t>(cols) & 3))
    return CDS_EINVAL;
  const int wq = (w + IB_K - 1) / IB_K;
  const long long items = (long long)n * h * wq;
  const int vec = (w % IB_K == 0) && (reinterpret_cast<uintptr_t>(out) & 15) == 0;
  const long long blocks = (items + 255) / 256;
  hipLaunchKernelGGL(image_batch_kernel, dim3((unsigned)(blocks > 16384 ? 16384 : blocks)), dim3(256), 0, (hipStream_t)stream, src, Hs, Ws,
                     rows, cols, h, w, wq, items, vec, out);
  return cds_launch_status();
}
