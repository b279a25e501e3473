// Probe points: the temperature at a few owned points after EVERY step of a
// fused pass (kernels/probe_cone.hip, cpu::probe_cone).
//
// The value of a point after steps t+1 .. t+k depends only on the (2k+1)^2
// patch around it at step t, and during the pass t -> t+k that patch sits
// untouched in the pass's source buffer (the two fields ping-pong). The cone
// code advances the patch k levels between two planes — level s updates the
// points within radius k - s — with the golden's operations in the golden's
// order (models/reference.py ftcs_step), and stores the centre after every
// level. The march kernels are not involved.
//
// This header holds what the device kernel and its CPU twin share: the
// argument block and the update of one point.
#pragma once

#include <cmath>

#include "heat2d/kernels.hpp"

namespace heat2d {
namespace kern {

// planes of (2 kMaxTB + 1)^2 elements
constexpr int kProbeSide = 2 * kMaxTB + 1;

enum ProbeMode : int { kProbePlain = 0, kProbeSource = 1, kProbeMap = 2, kProbeFaces = 3 };

// One cone launch. Rows and columns are local indices of the slab layout L
// (row -1 / column -1: the frame where the slab holds it).
struct ProbeArgs {
  const void* src;     // the cycle's source field (allocation base, layout L)
  const void* source;  // MODE source: the per-step increment, in L's layout
  const void* rmap;    // MODE map
  const void* rx;      // MODE faces
  const void* ry;
  const int64_t* pts;  // P pairs (local row, column) of owned points
  void* hist;          // H, capacity x P elements of the field's dtype
  const int64_t* base; // history row of this cycle's first level (nullptr: 0)
  int64_t base0;       // added to *base (the CPU twin passes the row here)
  int64_t capacity;    // rows of H: a level at or beyond it is not stored
  int64_t P;
  SlabLayout L;
  // the grid as the march sees it (bc_layout): the pinned frame rows / columns;
  // out of the patch's reach on a periodic axis
  int64_t frame_r0, frame_r1, frame_c0, frame_c1;
  // insulated walls: the first / last owned row and column whose operand beyond
  // the wall is the point's own value (INT64_MIN: none)
  int64_t wall_r0, wall_r1, wall_c0, wall_c1;
  double r;
  int32_t k;
  // a source's gain schedule (nullptr: none): level s adds gain[*gain_pos + gain_pos0 + s - 1] * S
  const void* gain;
  const int64_t* gain_pos;  // the solver's position word (nullptr: 0)
  int64_t gain_pos0;
  // Robin walls (robin != 0; plain mode, arith exact / fma): the operand beyond a
  // wall line is the ghost value a * C + b with the wall's pair, in the field's
  // dtype: rob = {r0 a, b, r1 a, b, c0 a, b, c1 a, b}; an insulated axis beside
  // a Robin one holds (1, -0.0)
  int32_t robin;
  double rob[8];
  // the five-weight operator (w5 != 0; plain mode, arith exact / fma, Dirichlet or periodic
  // axes): wt = (wS, wE, wN, wW, wC) in the field's dtype, `r` is not used
  int32_t w5;
  double wt[5];
};

// The frame and wall lines of a slab under boundary bits `bc`.
// (robin: the launchers' pairs, kernels.hpp — read only with a Robin axis in bc)
inline void probe_bounds(ProbeArgs& a, const SlabLayout& L, int bc, const double* robin = nullptr) {
  const SlabLayout Lk = bc_layout(L, bc);
  const int64_t dc = L.cpad - Lk.cpad;  // the widened grid's column 0 is real column -dc
  a.L = L;
  a.frame_r0 = -1 - Lk.row0;
  a.frame_r1 = Lk.nrows_global - Lk.row0;
  a.frame_c0 = -1 - dc;
  a.frame_c1 = Lk.ncols - dc;
  const int64_t none = INT64_MIN;
  a.wall_r0 = (bc & kBcWallX) ? -L.row0 : none;
  a.wall_r1 = (bc & kBcWallX) ? L.nrows_global - 1 - L.row0 : none;
  a.wall_c0 = (bc & kBcWallY) ? 0 : none;
  a.wall_c1 = (bc & kBcWallY) ? L.ncols - 1 : none;
  a.robin = (bc & kBcRobin) ? 1 : 0;
  for (int i = 0; i < 8; ++i) a.rob[i] = (i & 1) ? -0.0 : 1.0;
  if (a.robin) {
    HEAT2D_REQUIRE(robin, "probe_cone: a Robin axis needs the walls' pairs");
    wall_pairs(bc, true, robin, a.rob);
    wall_pairs(bc, false, robin, a.rob + 4);
  }
}

__host__ __device__ inline float probe_fma(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__host__ __device__ inline double probe_fma(double a, double b, double c) { return __builtin_fma(a, b, c); }
// The value beyond a Robin wall from the adjacent point c: a * c + b, the product
// rounded, then the add; AR 1: one fma (the march's tb_impl.hpp rob_ghost).
template <typename T, int AR>
__host__ __device__ inline T probe_ghost(double a, T c, double b) {
  if (AR == 1) return probe_fma((T)a, c, (T)b);
  return (T)a * c + (T)b;
}

// One point's update (compiled with contraction off: every operation below
// rounds on its own unless it is written as an fma). c: centre; s, e, n, w:
// (i+1, j), (i, j+1), (i-1, j), (i, j-1); AR 0 exact, 1 fma, 2 jacobi.
//   plain:  coef[0] = r
//   source: coef[0] = r, coef[1] = S[i,j]; GAIN: coef[2] = the level's gain g,
//           upd + g * S (the product rounded, then the add; AR 1: fma(g, S, upd))
//   map:    coef[0] = R[i,j]
//   faces:  coef = RY[i,j], RX[i,j], RY[i-1,j], RX[i,j-1]
template <typename T, int MODE, int AR, bool GAIN = false>
__host__ __device__ inline T probe_update(T c, T s, T e, T n, T w, const T* coef) {
  if (MODE == kProbeFaces) {
    const T ds = s - c, de = e - c, dn = n - c, dw = w - c;
    if (AR == 1) return c + probe_fma(coef[3], dw, probe_fma(coef[2], dn, probe_fma(coef[1], de, coef[0] * ds)));
    return c + (((coef[0] * ds + coef[1] * de) + coef[2] * dn) + coef[3] * dw);
  }
  const T sum = ((s + e) + n) + w;
  const T r = coef[0];
  T upd;
  if (AR == 2) upd = r * sum;
  else if (AR == 1) upd = probe_fma(r, probe_fma(T(-4), c, sum), c);
  else upd = c + r * (sum - T(4) * c);
  if (MODE == kProbeSource) {
    if (GAIN) upd = AR == 1 ? probe_fma(coef[2], coef[1], upd) : upd + coef[2] * coef[1];
    else upd = upd + coef[1];
  }
  return upd;
}

// Level s of one probe's cone, point `idx` of the (2 (k - s) + 1)^2 updated at
// that level: from plane `in` into plane `out` (kProbeSide x kProbeSide).
// ROB: the operand beyond a wall line is the wall's ghost value (ProbeArgs::rob).
template <typename T, int MODE, int AR, bool GAIN = false, bool ROB = false>
__host__ __device__ inline void probe_point(const ProbeArgs& a, int64_t ci, int64_t cj, int s, int idx, const T* in,
                                            T* out) {
  const int w = 2 * (a.k - s) + 1;
  const int u = s + idx / w, v = s + idx % w;  // plane coordinates
  const int64_t row = ci - a.k + u, col = cj - a.k + v;
  if (row < a.frame_r0 || row > a.frame_r1 || col < a.frame_c0 || col > a.frame_c1) return;  // off the grid
  const int at = u * kProbeSide + v;
  const T c = in[at];
  if (row == a.frame_r0 || row == a.frame_r1 || col == a.frame_c0 || col == a.frame_c1) {
    out[at] = c;  // a Dirichlet frame line (or the unread image line of an insulated axis)
    return;
  }
  T so, ea, no, we;
  if (ROB) {
    so = row == a.wall_r1 ? probe_ghost<T, AR>(a.rob[2], c, a.rob[3]) : in[at + kProbeSide];
    ea = col == a.wall_c1 ? probe_ghost<T, AR>(a.rob[6], c, a.rob[7]) : in[at + 1];
    no = row == a.wall_r0 ? probe_ghost<T, AR>(a.rob[0], c, a.rob[1]) : in[at - kProbeSide];
    we = col == a.wall_c0 ? probe_ghost<T, AR>(a.rob[4], c, a.rob[5]) : in[at - 1];
  } else {
    so = row == a.wall_r1 ? c : in[at + kProbeSide];
    ea = col == a.wall_c1 ? c : in[at + 1];
    no = row == a.wall_r0 ? c : in[at - kProbeSide];
    we = col == a.wall_c0 ? c : in[at - 1];
  }
  T coef[4];
  const int64_t o = a.L.offset(row, col);
  if (MODE == kProbeFaces) {
    const T* rx = static_cast<const T*>(a.rx);
    const T* ry = static_cast<const T*>(a.ry);
    coef[0] = ry[o];
    coef[1] = rx[o];
    coef[2] = ry[o - a.L.pitch];
    coef[3] = rx[o - 1];
  } else if (MODE == kProbeMap) {
    coef[0] = static_cast<const T*>(a.rmap)[o];
  } else {
    coef[0] = (T)a.r;
    if (MODE == kProbeSource) coef[1] = static_cast<const T*>(a.source)[o];
    if (GAIN) coef[2] = static_cast<const T*>(a.gain)[(a.gain_pos ? *a.gain_pos : 0) + a.gain_pos0 + s - 1];
  }
  out[at] = probe_update<T, MODE, AR, GAIN>(c, so, ea, no, we, coef);
}

// The five-weight operator's update of one point (ProbeArgs::wt), the march's W5 rule: operands
// in the order S, E, N, W and last C, every product and sum rounded; AR 1: the first product,
// then one fma per further operand.
template <typename T, int AR>
__host__ __device__ inline T probe_update_w5(T c, T s, T e, T n, T w, const double* wt) {
  const T ws = (T)wt[0], we = (T)wt[1], wn = (T)wt[2], ww = (T)wt[3], wc = (T)wt[4];
  if (AR == 1) return probe_fma(wc, c, probe_fma(ww, w, probe_fma(wn, n, probe_fma(we, e, ws * s))));
  return (((ws * s + we * e) + wn * n) + ww * w) + wc * c;
}
// probe_point for the five-weight operator: frame lines keep their value, the ghost rows /
// columns of a periodic axis are read as they lie in the plane (as the plain cone).
template <typename T, int AR>
__host__ __device__ inline void probe_point_w5(const ProbeArgs& a, int64_t ci, int64_t cj, int s, int idx, const T* in,
                                               T* out) {
  const int w = 2 * (a.k - s) + 1;
  const int u = s + idx / w, v = s + idx % w;  // plane coordinates
  const int64_t row = ci - a.k + u, col = cj - a.k + v;
  if (row < a.frame_r0 || row > a.frame_r1 || col < a.frame_c0 || col > a.frame_c1) return;  // off the grid
  const int at = u * kProbeSide + v;
  const T c = in[at];
  if (row == a.frame_r0 || row == a.frame_r1 || col == a.frame_c0 || col == a.frame_c1) {
    out[at] = c;  // a Dirichlet frame line
    return;
  }
  out[at] = probe_update_w5<T, AR>(c, in[at + kProbeSide], in[at + 1], in[at - kProbeSide], in[at - 1], a.wt);
}

// Whether patch point (row, col) is loaded: on the grid and inside the allocation.
__host__ __device__ inline bool probe_loads(const ProbeArgs& a, int64_t row, int64_t col) {
  return row >= a.frame_r0 && row <= a.frame_r1 && col >= a.frame_c0 && col <= a.frame_c1 && row >= -a.L.halo &&
         row < a.L.nrows + a.L.halo && col >= -a.L.cpad && col < a.L.col_hi();
}

// The cone of every point, k levels from `src`, level s into H row base + s - 1.
// mode: ProbeMode, from the buffers given (source, else rmap, else rx / ry).
// Capture-safe; `base` is read on the device when the kernel runs.
void launch_probe_cone(DType dt, const ProbeArgs& a, int arith, hipStream_t stream);
// *base += k, one thread, behind a cone launch on the same stream.
void launch_probe_advance(int64_t* base, int k, hipStream_t stream);
// A gain schedule's position for the next cycle: *to = *from + k, one thread.
// The solver keeps two words, one per buffer parity: a cycle reads its own and
// writes the other's, on a stream ordered behind the previous cycle's launches
// (the other word's readers), so no launch ever sees a word move under it.
void launch_gain_step(const int64_t* from, int64_t* to, int k, hipStream_t stream);

}  // namespace kern

namespace cpu {
void probe_cone(DType dt, const kern::ProbeArgs& a, int arith);
}  // namespace cpu
}  // namespace heat2d
