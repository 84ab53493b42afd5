// Rendering a mesh into the views of a scan (the rule is stated in include/cds_mvsnet_hip.h): depth, face index,
// facing and colour per pixel, as a function of the input alone.
//
//   cds_raster_project   one thread per (view, vertex): rule 1, the snapped coordinates and the camera-space point
//   cds_raster_faces     one thread per (view, face): rules 2-5 for the faces of at most `large_px` candidate pixels; a larger
//                        face is only marked
//   cds_raster_large     one wave per listed (view, face): its 64 lanes stride the candidate pixels
//   cds_raster_resolve   one thread per pixel: rule 6 from the winning key
//
// Every decision is made in int64 or fp64, with the bracketing of the rule (the library is built with -ffp-contract=off).  The
// visibility reduction is a 64-bit unsigned minimum over keys (depth bits, face index): it does not depend on the order in which
// fragments arrive, so it is done with the vector memory atomic that atomicMin compiles to (global_atomic_umin_x2, no
// compare-and-swap loop), the only atomic of this file.  Every loop has its bound fixed before it starts: the candidate count of the face.
// The workgroup size, blocks_for and resolve's face loader are those of mesh_common.hpp; face_setup keeps its own bounds test, which
// it interleaves with the loads of xy.
#include "mesh_common.hpp"

namespace {

using cds_mesh::blocks_for;
using cds_mesh::face_plane;
using cds_mesh::FacePlane;
using cds_mesh::fragment_depth;
using cds_mesh::fragment_exists;
using cds_mesh::kThreads;
using cds_mesh::kUnusable;
using cds_mesh::load_point;
using cds_mesh::surface_weights;

constexpr int kCam = CDS_RASTER_CAM;           // doubles per camera: R 0..8, t 9..11, fx 12, s 13, cx 14, fy 15, cy 16

// Rules 2 and 3 up to the candidate box of one face in one view.
struct FaceSetup {
  long long X[3], Y[3];
  int g;                                       // sign of A
  int px0, py0, bw, bh;                        // candidate pixels: px0 .. px0 + bw - 1, py0 .. py0 + bh - 1
  long long count;                             // bw bh, 0 when the face is not drawn or no pixel centre lies in its box
};

__device__ __forceinline__ long long floor_div256(long long a) { return a >> 8; }   // arithmetic shift: floor for negatives too

__device__ __forceinline__ bool face_setup(const int* __restrict__ faces, const int* __restrict__ xy, long long face,
                                           long long n_vertices, int h, int w, int idx[3], FaceSetup& s) {
  s.count = 0;
  for (int k = 0; k < 3; ++k) {
    idx[k] = faces[3 * face + k];
    if ((unsigned long long)(long long)idx[k] >= (unsigned long long)n_vertices) return false;   // never read outside the mesh
    const int2 p = *reinterpret_cast<const int2*>(xy + 2 * (long long)idx[k]);
    if (p.x == kUnusable) return false;
    s.X[k] = p.x;
    s.Y[k] = p.y;
  }
  const long long A = (s.X[1] - s.X[0]) * (s.Y[2] - s.Y[0]) - (s.Y[1] - s.Y[0]) * (s.X[2] - s.X[0]);
  if (A == 0) return false;
  s.g = A > 0 ? 1 : -1;
  const long long xl = min(s.X[0], min(s.X[1], s.X[2])), xh = max(s.X[0], max(s.X[1], s.X[2]));
  const long long yl = min(s.Y[0], min(s.Y[1], s.Y[2])), yh = max(s.Y[0], max(s.Y[1], s.Y[2]));
  // the centre 256 p + 128 lies in [lo, hi]  iff  ceil((lo - 128) / 256) <= p <= floor((hi - 128) / 256)
  const long long px0 = max(0ll, floor_div256(xl - 128 + 255)), px1 = min((long long)w - 1, floor_div256(xh - 128));
  const long long py0 = max(0ll, floor_div256(yl - 128 + 255)), py1 = min((long long)h - 1, floor_div256(yh - 128));
  if (px1 < px0 || py1 < py0) return false;
  s.px0 = (int)px0; s.py0 = (int)py0;
  s.bw = (int)(px1 - px0 + 1); s.bh = (int)(py1 - py0 + 1);
  s.count = (long long)s.bw * s.bh;
  return true;
}

// Rule 3 for the pixel (px, py).
__device__ __forceinline__ bool covered(const FaceSetup& s, int px, int py) {
  const long long Qx = 256ll * px + 128, Qy = 256ll * py + 128;
  bool in = true;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const int j = i == 2 ? 0 : i + 1;
    const long long dx = s.g * (s.X[j] - s.X[i]), dy = s.g * (s.Y[j] - s.Y[i]);
    const long long E = dx * (Qy - s.Y[i]) - dy * (Qx - s.X[i]);
    in = in && (E > 0 || (E == 0 && (dy < 0 || (dy == 0 && dx > 0))));
  }
  return in;
}

// Rules 3-5 for candidate i of the face.
__device__ __forceinline__ void draw_candidate(const FaceSetup& s, const FacePlane& f, const double* __restrict__ cam, long long i,
                                               unsigned face, int w, unsigned long long* __restrict__ keys) {
  const int px = s.px0 + (int)(i % s.bw), py = s.py0 + (int)(i / s.bw);
  if (!covered(s, px, py)) return;
  double rx, ry;
  const double zf = fragment_depth(f, cam, px, py, rx, ry);
  if (!fragment_exists(zf)) return;
  const unsigned long long key = ((unsigned long long)__float_as_uint((float)zf) << 32) | face;
  atomicMin(keys + (size_t)py * w + px, key);
}

// ------------------------------------------------------------------------------------------------------------------ project
__global__ __launch_bounds__(kThreads) void raster_project_kernel(const float* __restrict__ vertices, long long n_vertices,
                                                                  const double* __restrict__ cams, int* __restrict__ xy,
                                                                  double* __restrict__ xc) {
  const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n_vertices) return;
  const int view = blockIdx.y;
  const double* c = cams + (long long)view * kCam;
  const cds_mesh::ViewPoint p = cds_mesh::view_point(c, vertices[3 * i], vertices[3 * i + 1], vertices[3 * i + 2]);   // rule 1
  int X, Y;
  cds_mesh::snap_point(p, X, Y);
  const long long o = (long long)view * n_vertices + i;
  xy[2 * o] = X;
  xy[2 * o + 1] = Y;
  xc[3 * o] = p.xc0; xc[3 * o + 1] = p.xc1; xc[3 * o + 2] = p.z;
}

// -------------------------------------------------------------------------------------------------------------------- faces
__global__ __launch_bounds__(kThreads) void raster_faces_kernel(const int* __restrict__ faces, long long n_faces,
                                                                long long n_vertices, const double* __restrict__ cams,
                                                                const int* __restrict__ xy, const double* __restrict__ xc, int h,
                                                                int w, long long large_px, unsigned long long* __restrict__ keys,
                                                                unsigned char* __restrict__ large) {
  const long long face = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (face >= n_faces) return;
  const int view = blockIdx.y;
  int idx[3];
  FaceSetup s;
  const bool drawn = face_setup(faces, xy + 2 * (long long)view * n_vertices, face, n_vertices, h, w, idx, s);
  const bool is_large = drawn && s.count > large_px;
  large[(long long)view * n_faces + face] = is_large ? 1 : 0;
  if (!drawn || is_large) return;
  const double* xcv = xc + 3 * (long long)view * n_vertices;
  double a[3], b[3], c[3];
  load_point(xcv, idx[0], a); load_point(xcv, idx[1], b); load_point(xcv, idx[2], c);
  const FacePlane f = face_plane(a, b, c);
  const double* cam = cams + (long long)view * kCam;
  unsigned long long* kv = keys + (size_t)view * h * w;
  const long long count = s.count;                                     // <= large_px
  for (long long i = 0; i < count; ++i) draw_candidate(s, f, cam, i, (unsigned)face, w, kv);
}

// One wave per entry of `list` (view n_faces + face); its lanes take the candidates lane, lane + 64, ...
__global__ __launch_bounds__(kThreads) void raster_large_kernel(const long long* __restrict__ list, long long n_list,
                                                                const int* __restrict__ faces, long long n_faces,
                                                                long long n_vertices, int n_views,
                                                                const double* __restrict__ cams, const int* __restrict__ xy,
                                                                const double* __restrict__ xc, int h, int w,
                                                                unsigned long long* __restrict__ keys) {
  const long long item = (long long)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
  if (item >= n_list) return;
  const long long e = list[item];
  if (e < 0 || e >= (long long)n_views * n_faces) return;              // an entry that does not belong to this chunk
  const int view = (int)(e / n_faces);
  const long long face = e % n_faces;
  int idx[3];
  FaceSetup s;
  if (!face_setup(faces, xy + 2 * (long long)view * n_vertices, face, n_vertices, h, w, idx, s)) return;
  const double* xcv = xc + 3 * (long long)view * n_vertices;
  double a[3], b[3], c[3];
  load_point(xcv, idx[0], a); load_point(xcv, idx[1], b); load_point(xcv, idx[2], c);
  const FacePlane f = face_plane(a, b, c);
  const double* cam = cams + (long long)view * kCam;
  unsigned long long* kv = keys + (size_t)view * h * w;
  const long long count = s.count;                                     // <= h w
  for (long long i = threadIdx.x & 63; i < count; i += 64) draw_candidate(s, f, cam, i, (unsigned)face, w, kv);
}

// ------------------------------------------------------------------------------------------------------------------ resolve
__global__ __launch_bounds__(kThreads) void raster_resolve_kernel(const unsigned long long* __restrict__ keys,
                                                                  const int* __restrict__ faces, long long n_faces,
                                                                  long long n_vertices, const double* __restrict__ cams,
                                                                  const double* __restrict__ xc,
                                                                  const unsigned char* __restrict__ colors, int h, int w,
                                                                  float* __restrict__ depth, int* __restrict__ face_out,
                                                                  unsigned char* __restrict__ front,
                                                                  unsigned char* __restrict__ valid,
                                                                  unsigned char* __restrict__ image) {
  const long long p = (long long)blockIdx.x * kThreads + threadIdx.x, hw = (long long)h * w;
  if (p >= hw) return;
  const int view = blockIdx.y;
  const size_t o = (size_t)view * hw + p;
  const unsigned long long key = keys[o];
  const long long face = (long long)(key & 0xffffffffull);
  float z = 0.f;
  int fo = -1;
  unsigned char fr = 0, rgb[3] = {0, 0, 0};
  int idx[3] = {0, 0, 0};
  const bool hit = key != ~0ull && face < n_faces && cds_mesh::load_face(faces, face, n_vertices, idx);
  if (hit) {
    z = __uint_as_float((unsigned)(key >> 32));
    fo = (int)face;
    const double* xcv = xc + 3 * (long long)view * n_vertices;
    double a[3], b[3], c[3];
    load_point(xcv, idx[0], a); load_point(xcv, idx[1], b); load_point(xcv, idx[2], c);
    const FacePlane f = face_plane(a, b, c);
    fr = f.d < 0.0 ? 1 : 0;
    if (colors && image) {
      double rx, ry;
      const double zf = fragment_depth(f, cams + (long long)view * kCam, (int)(p % w), (int)(p / w), rx, ry);
      double wt[3];
      surface_weights(f, a, b, c, zf, rx, ry, wt);
      for (int ch = 0; ch < 3; ++ch) {
        const double ca = colors[3 * (long long)idx[0] + ch], cb = colors[3 * (long long)idx[1] + ch],
                     cc = colors[3 * (long long)idx[2] + ch];
        const double val = (wt[0] * ca + wt[1] * cb) + wt[2] * cc;
        const double cl = val > 0.0 ? (val < 255.0 ? val : 255.0) : 0.0;       // NaN -> 0
        rgb[ch] = (unsigned char)(int)floor(cl + 0.5);
      }
    }
  }
  depth[o] = z;
  face_out[o] = fo;
  front[o] = fr;
  valid[o] = fr;                                                         // hit and front
  if (image) { image[3 * o] = rgb[0]; image[3 * o + 1] = rgb[1]; image[3 * o + 2] = rgb[2]; }
}

bool sizes_ok(long long n_vertices, long long n_faces, int n_views, int h, int w) {
  return n_vertices >= 0 && n_vertices <= 0x7fffffffLL && n_faces >= 0 && n_faces <= 0x7fffffffLL && n_views >= 1 &&
         n_views <= CDS_RASTER_MAX_CHUNK && h >= 1 && w >= 1 && (long long)h * w <= 0x7fffffffLL;
}

}  // namespace

extern "C" int cds_raster_project(const float* vertices, long long n_vertices, const double* cams, int n_views, int* xy, double* xc,
                                  void* stream) {
  if (!sizes_ok(n_vertices, 0, n_views, 1, 1)) return CDS_EINVAL;
  if (n_vertices == 0) return 0;
  if (!vertices || !cams || !xy || !xc) return CDS_EINVAL;
  hipLaunchKernelGGL(raster_project_kernel, dim3(blocks_for(n_vertices), (unsigned)n_views), dim3(kThreads), 0, (hipStream_t)stream,
                     vertices, n_vertices, cams, xy, xc);
  return cds_launch_status();
}

extern "C" int cds_raster_faces(const int* faces, long long n_faces, long long n_vertices, const double* cams, int n_views,
                                const int* xy, const double* xc, int h, int w, long long large_px, unsigned long long* keys,
                                unsigned char* large, void* stream) {
  if (!sizes_ok(n_vertices, n_faces, n_views, h, w) || large_px < 1) return CDS_EINVAL;
  if (n_faces == 0) return 0;
  if (!faces || !cams || !xy || !xc || !keys || !large) return CDS_EINVAL;
  hipLaunchKernelGGL(raster_faces_kernel, dim3(blocks_for(n_faces), (unsigned)n_views), dim3(kThreads), 0, (hipStream_t)stream, faces,
                     n_faces, n_vertices, cams, xy, xc, h, w, large_px, keys, large);
  return cds_launch_status();
}

extern "C" int cds_raster_large(const long long* list, long long n_list, const int* faces, long long n_faces, long long n_vertices,
                                const double* cams, int n_views, const int* xy, const double* xc, int h, int w,
                                unsigned long long* keys, void* stream) {
  if (!sizes_ok(n_vertices, n_faces, n_views, h, w) || n_list < 0 || n_list > CDS_RASTER_MAX_LIST) return CDS_EINVAL;
  if (n_list == 0 || n_faces == 0) return 0;
  if (!list || !faces || !cams || !xy || !xc || !keys) return CDS_EINVAL;
  const unsigned blocks = (unsigned)((n_list + kThreads / 64 - 1) / (kThreads / 64));
  hipLaunchKernelGGL(raster_large_kernel, dim3(blocks), dim3(kThreads), 0, (hipStream_t)stream, list, n_list, faces, n_faces,
                     n_vertices, n_views, cams, xy, xc, h, w, keys);
  return cds_launch_status();
}

extern "C" int cds_raster_resolve(const unsigned long long* keys, const int* faces, long long n_faces, long long n_vertices,
                                  const double* cams, int n_views, const double* xc, const unsigned char* colors, int h, int w,
                                  float* depth, int* face, unsigned char* front, unsigned char* valid, unsigned char* image,
                                  void* stream) {
  if (!sizes_ok(n_vertices, n_faces, n_views, h, w)) return CDS_EINVAL;
  if (!keys || !cams || !depth || !face || !front || !valid || (n_faces > 0 && (!faces || !xc))) return CDS_EINVAL;
  hipLaunchKernelGGL(raster_resolve_kernel, dim3(blocks_for((long long)h * w), (unsigned)n_views), dim3(kThreads), 0,
                     (hipStream_t)stream, keys, faces, n_faces, n_vertices, cams, xc, colors, h, w, depth, face, front, valid, image);
  return cds_launch_status();
}
