// Shared pieces of the z-marching transposed-convolution kernels (deconv3d_zm.hip, deconv_prob_zm.hip): which column and z segment
// a workgroup owns, the staging of one input cell plane into the LDS ring, and the host's choice of the number of z segments.
#pragma once
#include "sbf_common.hpp"

namespace {

// What a workgroup marches over: column (tx_i, ty_i), cell planes [a0, a1).  Uniform cutting: workgroup -> (column; z segment),
// the columns of one z segment are consecutive workgroups after the XCD remap; a0 >= a1: the segment is past the volume and the
// workgroup has nothing to do.  Balanced cutting: one of the workgroup's pieces (ZmWalk below).
struct ZmColumn {
  int tx_i, ty_i, a0, a1;
};

// ---------------------------------------------------------------------------------------------------------------------------------
// The BALANCED cutting of a z-march layer: one contiguous range per workgroup instead of columns x z segments equal units.
// The layer is the sequence of T = cols x stages slots, column-major (slot = col * stages + stage; a stage is what a kernel does
// between two barriers of its march: G output planes in conv3d_zmg.hip, a cell plane in the transposed-convolution kernels).
// Workgroup wg of nwg owns the slots [snap(wg T / nwg), snap((wg + 1) T / nwg)), cut at the column boundaries into PIECES
// (col, [s0, s1)); it walks its pieces one after the other and keeps what does not depend on the column (weights, bias, bound).
// The cutting is a pure function of (cols, stages, nwg, wg, min_len): no counter, no atomics, no workgroup waits for another, and
// every slot belongs to exactly one workgroup whatever the number of CUs that run them.
// snap() moves a boundary that would leave a piece shorter than min_len (a piece pays the priming of its ring like a whole column)
// to the column boundary on that side, so the short piece goes to the neighbour that holds the rest of its column.  It is applied
// to BOUNDARIES, the same way to a range's lower and its neighbour's upper end: with offset r of the boundary inside its column
//   r' = r rounded to the nearest multiple of q (ties up);  0 < r' < min_len -> 0;  r' > stages - min_len -> stages
// where q = 1 while the ranges are at least min_len long (T / nwg >= min_len: two boundaries inside a column are then min_len
// apart on their own) and q = min_len for shorter ranges (more workgroups than the layer has work for: the allowed cuts of a column
// are then the multiples of min_len up to stages - min_len, and the workgroups whose two boundaries snap to the same slot are
// empty).  snap() is monotone, so the ranges tile [0, T); every piece is a whole column or at least min_len long.
// Chosen min_len: ceil(P) + 1 stages for the P stages a piece spends priming: 4 for conv3d_zmg (P = 2.5), 3 for the cell-plane
// kernels (P = 1.5).
// ZM_MAX_PIECES bounds the pieces of one workgroup: a range of L = ceil(T / nwg) slots touches at most floor((L - 2) / stages) + 2
// columns (snapping moves a boundary to the end of its own column at most, never into another one), so 8 covers every layer with
// L <= 6 columns.  Where a layer would need more (few workgroups, many short columns: every piece primes its ring again) the host
// keeps the uniform cutting; the kernels walk a range whatever its number of pieces (they hold no table of them), the bound is what
// the host's cost model and the tests state.
constexpr int ZM_MAX_PIECES = 8;
constexpr int ZM_MINLEN_CELL = 3, ZM_MINLEN_ZMG = 4;

struct ZmRange {
  int lo, hi;   // slots [lo, hi); lo >= hi: the workgroup has nothing to do
};
struct ZmPiece {
  int col, s0, s1;   // stages [s0, s1) of column col
};
__host__ __device__ inline int zm_snap(long long b, int stages, int q, int min_len) {
  const long long col = b / stages;
  int r = (int)(b - col * stages);
  r = ((r + q / 2) / q) * q;
  if (r < min_len) r = 0;
  if (r > 0 && r > stages - min_len) r = stages;
  return (int)(col * stages + r);
}
__host__ __device__ inline ZmRange zm_range(int cols, int stages, int nwg, int wg, int min_len) {
  const long long T = (long long)cols * stages;
  const int q = T / nwg >= min_len ? 1 : min_len;
  return {zm_snap(wg * T / nwg, stages, q, min_len), zm_snap((wg + 1ll) * T / nwg, stages, q, min_len)};
}
// the piece of a range that starts at slot pos (lo <= pos < hi); the next one starts at col * stages + s1
__host__ __device__ inline ZmPiece zm_piece_at(int pos, int hi, int stages) {
  const int col = pos / stages, s0 = pos - col * stages;
  const int rest = hi - col * stages;
  return {col, s0, rest < stages ? rest : stages};
}
// All pieces of workgroup wg: returns their number (which may exceed ZM_MAX_PIECES: the layer then keeps the uniform cutting) and
// stores the first ZM_MAX_PIECES of them.
__host__ __device__ inline int zm_partition(int cols, int stages, int nwg, int wg, int min_len, ZmPiece* out) {
  const ZmRange r = zm_range(cols, stages, nwg, wg, min_len);
  int n = 0;
  for (int pos = r.lo; pos < r.hi; ++n) {
    const ZmPiece p = zm_piece_at(pos, r.hi, stages);
    if (n < ZM_MAX_PIECES) out[n] = p;
    pos = p.col * stages + p.s1;
  }
  return n;
}

// A workgroup's walk over its pieces (device side; the values are wave-uniform and kept in SGPRs).  BAL = false is the uniform
// cutting, one unit per workgroup, with the index arithmetic of zm_column(): a kernel writes
//   ZmWalk<BAL> walk(ncols, D, seg_len, min_len);  if (walk.empty()) return;
//   do { const ZmColumn zc = walk.column(tiles_x); ... one march ... } while (BAL && walk.next_piece());
// in its producer and in its consumer branch alike; next_piece() holds the one workgroup barrier between two pieces (the ring and
// whatever else of the LDS a march uses is free behind it), so both branches execute the same barriers.
template <bool BAL>
struct ZmWalk {
  int col, s0, s1, hi, stages;
  __device__ __forceinline__ ZmWalk(int cols, int stages_, int seg_len, int min_len) : stages(stages_) {
    const int wg = cds_xcd_remap(blockIdx.x, gridDim.x);
    if (BAL) {
      const ZmRange r = zm_range(cols, stages, gridDim.x, wg, min_len);
      hi = __builtin_amdgcn_readfirstlane(r.hi);
      set(__builtin_amdgcn_readfirstlane(r.lo));
    } else {
      col = wg % cols;
      s0 = (wg / cols) * seg_len;
      s1 = min(stages, s0 + seg_len);
      hi = 0;
    }
  }
  __device__ __forceinline__ void set(int pos) {
    if (pos < hi) {
      const ZmPiece p = zm_piece_at(pos, hi, stages);   // (integer division runs on the VALU: back to SGPRs)
      col = __builtin_amdgcn_readfirstlane(p.col), s0 = __builtin_amdgcn_readfirstlane(p.s0), s1 = __builtin_amdgcn_readfirstlane(p.s1);
    } else {
      col = 0, s0 = 0, s1 = 0;
    }
  }
  __device__ __forceinline__ bool empty() const { return s0 >= s1; }
  __device__ __forceinline__ ZmColumn column(int tiles_x) const {
    if (!BAL) return {col % tiles_x, col / tiles_x, s0, s1};
    const int ty_i = __builtin_amdgcn_readfirstlane(col / tiles_x);
    return {col - ty_i * tiles_x, ty_i, s0, s1};
  }
  __device__ __forceinline__ bool next_piece() {
    const int pos = col * stages + s1;
    if (pos >= hi) return false;
    set(pos);
    __syncthreads();
    return true;
  }
};

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
// cost_out: the model cost of the best candidate, or < 0 where the knob forced the number (the caller then keeps the uniform form).
inline int zm_pick_nseg(int wgs_per_seg, int D, int cap, const char* env_name, double* cost_out = nullptr) {
  int best = 1;
  double best_cost = 1e30;
  for (int n = 1; n <= min(D, cap); ++n) {
    const int len = cds_ceil_div(D, n);
    const int n_eff = cds_ceil_div(D, len);
    const double cost = (double)cds_ceil_div(wgs_per_seg * n_eff, 256) * (len + 1.5);
    if (cost < best_cost - 1e-9) { best_cost = cost; best = n; }
  }
  const int nseg_e = cds_env_int(env_name, 0);
  if (cost_out) *cost_out = nseg_e > 0 ? -1.0 : best_cost;
  return nseg_e > 0 ? min(nseg_e, D) : best;
}

// The number of workgroups a balanced layer is cut into: the device's CU count (one z-march workgroup per CU: its LDS), cached per
// device.  CDS_ZM_NCU (test and A/B knob, read per launch) overrides it: results do not depend on it.
inline int zm_ncu() {
  const int e = cds_env_int("CDS_ZM_NCU", 0);
  if (e > 0) return e;
  static std::atomic<int> cache[64];
  int d = 0;
  (void)hipGetDevice(&d);
  int v = cache[d & 63].load(std::memory_order_relaxed);
  if (v > 0) return v;
  if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, d) != hipSuccess || v < 1) {
    (void)hipGetLastError();
    v = 256;
  }
  cache[d & 63].store(v, std::memory_order_relaxed);
  return v;
}

// Model cost of the balanced cutting, in stages: the worst workgroup's slots + P for each of its pieces (every piece primes its
// ring; an upper bound: the pieces after a workgroup's first keep the weights).  max_pieces: of any workgroup.  The last result is
// remembered per thread: a layer asks for the same cutting on every call.
inline double zm_balanced_cost(int cols, int stages, int nwg, int min_len, double P, int* max_pieces) {
  struct Memo { int cols, stages, nwg, min_len, maxp; double P, cost; };
  thread_local Memo memo[8] = {};
  thread_local int next = 0;
  for (const Memo& m : memo)
    if (m.cols == cols && m.stages == stages && m.nwg == nwg && m.min_len == min_len && m.P == P) { *max_pieces = m.maxp; return m.cost; }
  double cost = 0;
  int maxp = 0;
  for (int wg = 0; wg < nwg; ++wg) {
    ZmPiece pc[ZM_MAX_PIECES];
    const ZmRange r = zm_range(cols, stages, nwg, wg, min_len);
    const int n = zm_partition(cols, stages, nwg, wg, min_len, pc);
    maxp = max(maxp, n);
    cost = fmax(cost, (r.hi - r.lo) + P * n);
  }
  memo[next] = {cols, stages, nwg, min_len, maxp, P, cost};
  next = (next + 1) % 8;
  *max_pieces = maxp;
  return cost;
}

// Which cutting runs.  balance: CDS_ZM_BALANCE (0 = uniform only, 1 = the model decides, 2 = balanced wherever the piece bound
// holds); uniform_cost: the uniform chooser's best cost, < 0 where an NSEG knob forced it (those keep their meaning: uniform).
// The model's two costs differ by what it does not know (a piece's real priming, the memory system): balanced runs by default only
// where it is at least `margin` cheaper.  Measured (profiles/zm_balance.md): with ZM_BALANCE_MARGIN the default never picked the
// slower form of a conv3d_zmg or deconv3d_zm layer; the fused tail needs ZM_BALANCE_MARGIN_TAIL (at M1 the model promises 6 % and
// the kernel, whose second, part-empty round runs with more bandwidth per CU, gives none).
constexpr double ZM_BALANCE_MARGIN = 0.02, ZM_BALANCE_MARGIN_TAIL = 0.08;
inline bool zm_choose_balanced(int balance, double uniform_cost, int cols, int stages, int nwg, int min_len, double P,
                               double* balanced_cost = nullptr, double margin = ZM_BALANCE_MARGIN) {
  int maxp = 0;
  const double bc = zm_balanced_cost(cols, stages, nwg, min_len, P, &maxp);
  if (balanced_cost) *balanced_cost = bc;
  if (balance <= 0 || uniform_cost < 0 || maxp > ZM_MAX_PIECES) return false;
  return balance >= 2 || bc < uniform_cost * (1.0 - margin);
}
inline int zm_balance_knob() { return cds_env_int("CDS_ZM_BALANCE", 1); }

}  // namespace
