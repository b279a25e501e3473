// heat2d device-kernel launchers (gfx950). Every launcher is capture-safe:
// no allocation, no synchronisation, only kernel launches on `stream`.
#pragma once

#include <hip/hip_runtime.h>

#include "heat2d/common.hpp"

namespace heat2d {
namespace kern {

// Tiling of one temporal-block launch. Filled by plan_tb(); exposed so tests
// and the autotuner can inspect / override it.
struct TbPlan {
  int32_t k;          // time steps fused in this launch (1..kMaxTB)
  int32_t vec;        // elements per lane (16 B: 4 fp32 / 2 fp64)
  int32_t strip_w;    // columns loaded per wave (64 * vec)
  int32_t useful_w;   // columns produced per wave (strip_w - 2*ceil(k, vec))
  int64_t tile_rows;  // output rows per wave tile
  int64_t nstrips;
  int64_t ntiles;
  int64_t nwaves;
  int64_t nblocks;    // 256-thread workgroups (4 independent waves each)
  int32_t skew;       // level pipeline skew (always 1: upward march, see tb_impl.hpp)
  int32_t blocks_per_cu;  // resident workgroups per CU (occupancy API)
  int32_t prefetch;   // level-0 row ring per wave (RING; RING-2 rows in flight)
  int32_t main;       // 1: interior-only (MAIN) kernel instance
};

// Plan a launch that advances rows [row_begin, row_end) of the slab by k steps.
// tile_rows == 0 selects the occupancy-driven row bands, > 0 bands of that many
// rows, < 0 -tile_rows segments (TbRect nb < 0; ntiles = -segments); cus > 0 plans for a
// stream restricted to that many CUs (comm-reserving CU mask).
// arith: 0 = reference arithmetic (every op rounded), 1 = contracted fma form,
// 2 = r == 1/4: (S + E + N + W) / 4 (tb_impl.hpp, March); the launchers below
// take it in their TbTerms.
TbPlan plan_tb(DType dt, const SlabLayout& L, int64_t row_begin, int64_t row_end, int k,
               int64_t tile_rows = 0, int cus = 0, int arith = 0);

// Boundary conditions (SolverConfig::bc_x / bc_y as one bit set, TbTerms::bc
// below). 0 = the Dirichlet frame on both axes.
//   kBcPeriodicX: no row is pinned — the slab is marched as a middle slab
//     whatever its place in the grid (bc_layout); its ghost rows are wrap
//     images, kept by the halo exchange (one rank: launch_wrap_rows).
//   kBcPeriodicY: no owned or ghost column is pinned — the kWrapCols ghost
//     columns on each side are wrap images of the owned columns, and every
//     launcher refreshes them over the rows it wrote (launch_wrap_cols, same
//     stream, right behind its stencil launch). The march itself is the
//     Dirichlet one, unchanged, on a grid widened by the ghost columns
//     (bc_layout): its "frame" columns are the pad columns beyond them. It
//     stores meaningless values into the ghost columns of the rows it writes
//     (level K there is cut off from its wrap neighbours; the straddling lane
//     adds up to V - 1 pad columns), which the fill overwrites: kWrapCols must
//     be >= the depth of any pass (kMaxTB) and >= V (4).
//   kBcInsulatedX / kBcInsulatedY: a zero-flux wall half a cell outside the
//     first and last owned row / column. The frame entry is the image of the
//     adjacent owned point (T[-1] = T[0], T[n] = T[n-1]). A mirrored ghost
//     layer would not give the golden's bits (its points add their operands in
//     the swapped order), so the layout is the Dirichlet one and the march has
//     device code of its own: tb_kernel_ins (tb_impl.hpp), in which a point
//     next to an insulated wall takes its own value for the operand beyond the
//     wall, at every level. Every launch that would use the general kernel
//     uses it; with insulated y the frame-column strips of an interior-kernel
//     launch become rects of it. The launchers refresh the frame images of
//     the rows they wrote (launch_ins_cols / launch_ins_rows, same stream).
//     Not with arith 3, nor the fused statistics; an axis is periodic or
//     insulated, not both.
//   kBcRobinX / kBcRobinY: a Robin (convective) wall in the insulated
//     geometry: the value beyond the wall is the affine ghost G = a * C + b of
//     the adjacent owned point C (the product rounded, then the add; arith 1:
//     fma(a, C, b)), with a pair (a, b) per wall (TbTerms::robin). G depends on
//     the level's own C, so it is formed inside the march at every level:
//     tb_kernel_rob (tb_impl.hpp, March with kFeatRob) takes the place of
//     tb_kernel_ins in every launch, and an insulated wall on the other axis
//     runs on it as (1, -0.0), which returns every C unchanged.
//     The launchers write the ghost values into the frame of the rows they
//     wrote (launch_rob_rows, then launch_rob_cols over the frame rows too:
//     the golden's x first, then y). Arith 0 / 1, depths 1..kMaxTBRob.
constexpr int kBcPeriodicX = 1, kBcPeriodicY = 2, kBcInsulatedX = 4, kBcInsulatedY = 8, kBcRobinX = 16, kBcRobinY = 32;
// an axis with walls half a cell outside its first and last owned point
constexpr int kBcWallX = kBcInsulatedX | kBcRobinX, kBcWallY = kBcInsulatedY | kBcRobinY;
constexpr int kBcRobin = kBcRobinX | kBcRobinY;
// The Robin pairs as the launchers take them: 8 values already converted to the
// field's dtype, {x_lo a, b, x_hi a, b, y_lo a, b, y_hi a, b} (x_lo: the wall
// before the first owned row, y_lo: before the first owned column); the entries
// of an axis that is not Robin are not read.
constexpr int kRobinXLo = 0, kRobinXHi = 2, kRobinYLo = 4, kRobinYHi = 6;
// (a_lo, b_lo, a_hi, b_hi) of the walls of one axis in a launch with a Robin
// axis: the axis' own pairs, or (1, -0.0) twice where it is insulated
inline void wall_pairs(int bc, bool x_axis, const double* robin, double out[4]) {
  const bool rob = (bc & (x_axis ? kBcRobinX : kBcRobinY)) != 0;
  for (int i = 0; i < 4; ++i) out[i] = rob ? robin[(x_axis ? kRobinXLo : kRobinYLo) + i] : ((i & 1) ? -0.0 : 1.0);
}
// A source's gain schedule as the launchers take it (TbTerms::gain below): the gain
// array and the position word, both in the launch's memory space.
struct GainRef {
  const void* g = nullptr;
  const int64_t* pos = nullptr;
};
// ghost columns per side kept as wrap images: the deepest pass (kMaxTB) reads that many
constexpr int64_t kWrapCols = kMaxTB;
static_assert(kWrapCols <= kColPad && kWrapCols >= 4, "ghost columns must fit the column padding");
// The layout the planners and kernels see. Periodic x: the global frame rows
// are moved out of reach of every march (row0 and nrows_global shifted by
// kBcRowShift), so each slab plans and runs as a middle slab: no edge kind 1 /
// 3 item, boundary bands on the interior kernel. Periodic y: column 0 of the
// widened grid is ghost column -kWrapCols, and it has ncols + 2 kWrapCols
// "owned" columns (same pitch, same memory): a garbage value entering from a
// pinned pad column moves one column per level, so after K <= kWrapCols levels
// it has not reached the real owned columns. Dirichlet: L itself.
constexpr int64_t kBcRowShift = int64_t(1) << 24;
inline SlabLayout bc_layout(SlabLayout L, int bc) {
  if (bc & kBcPeriodicX) {
    L.row0 += kBcRowShift;
    L.nrows_global += 2 * kBcRowShift;
  }
  if (bc & kBcPeriodicY) {
    L.cpad -= kWrapCols;
    L.ncols += 2 * kWrapCols;
  }
  return L;
}
// Ghost-column fill of rows [r0, r1) (ghost / frame rows allowed) and the
// k-row self wrap of whole padded rows: rows [nrows-k, nrows) -> [-k, 0),
// [0, k) -> [nrows, nrows+k) (periodic x on one rank).
void launch_wrap_cols(DType dt, void* field, const SlabLayout& L, int64_t r0, int64_t r1, hipStream_t stream);
void launch_wrap_rows(DType dt, void* field, const SlabLayout& L, int64_t k, hipStream_t stream);
// Insulated frame images. ins_cols: columns -1 <- 0 and ncols <- ncols - 1 of
// rows [r0, r1) (ghost / frame rows allowed). ins_rows: the whole padded row
// -1 <- 0 where the slab holds the global first row (lo) and nrows <- nrows - 1
// where it holds the last (hi); a slab off that edge is left alone.
void launch_ins_cols(DType dt, void* field, const SlabLayout& L, int64_t r0, int64_t r1, hipStream_t stream);
void launch_ins_rows(DType dt, void* field, const SlabLayout& L, bool lo, bool hi, hipStream_t stream);
// Robin frame images (the ghost values a * C + b in the form `arith` names: 0
// the product rounded then the add, 1 one fma), pairs as (a_lo, b_lo, a_hi,
// b_hi) in the field's dtype. rob_rows: the whole padded row -1 from row 0 where
// the slab holds the global first row (lo) and row nrows from row nrows - 1
// where it holds the last (hi). rob_cols: columns -1 and ncols of rows [r0, r1)
// (ghost / frame rows allowed). Rows first, then the columns over the frame
// rows too, gives the golden's corner entries. Capturable.
void launch_rob_rows(DType dt, void* field, const SlabLayout& L, bool lo, bool hi, const double* pairs, int arith,
                     hipStream_t stream);
void launch_rob_cols(DType dt, void* field, const SlabLayout& L, int64_t r0, int64_t r1, const double* pairs,
                     int arith, hipStream_t stream);

// The terms of a stencil launch: the arithmetic form, the boundary kinds and the
// optional buffers of the features. Every stencil launcher below (and its CPU
// twin cpu::tb) takes one; a default-constructed one is the plain Dirichlet
// march in reference arithmetic. Which terms go together, and in which kernel
// family a launch runs: stencil_tb.hip select_family.
struct TbTerms {
  // 0 = reference arithmetic (every op rounded), 1 = contracted fma form,
  // 2 = r == 1/4, 3 = any r with scaled levels (plan_tb above)
  int arith = 0;
  // the boundary kinds, kBcPeriodicX | ... | kBcRobinY above; 0 = the Dirichlet frame on both axes
  int bc = 0;
  // A heat source S in the field's layout and dtype, added at every fused level,
  // T' = update(T) + S (one separately rounded add per point and level) — the
  // per-step increment dt * f, holding -0.0 in every frame row / column and pad
  // entry so that pinned points keep their bits. With a source every rect of the
  // launch runs tb_kernel_src (tb_impl.hpp): Dirichlet on both axes, arith 0 / 1,
  // depths 1..kMaxTBSrc, no wave-pair plans. nullptr: no source.
  const void* source = nullptr;
  // The per-point diffusion number R in the field's layout and dtype, the
  // multiplier of every point's update at every fused level,
  // T' = C + R * (sum - 4C) — `r` is then not used. It holds +0.0 in every frame
  // row / column, pad entry and row outside the grid: that is the pinning, and a
  // 0 at an owned point holds that point. With a map every rect of the launch
  // runs tb_kernel_var (tb_impl.hpp): Dirichlet on both axes, arith 0 / 1,
  // depths 1..kMaxTBVar, no wave-pair plans, not together with a source.
  const void* rmap = nullptr;
  // Both or neither: the per-face diffusion numbers of the conservative form
  // div(k grad u) in the field's layout and dtype — rx at (i, j) the face between
  // (i, j) and (i, j+1), ry the face between (i, j) and (i+1, j) —,
  // T' = C + (((ry*(S-C) + rx*(E-C)) + ry[i-1]*(N-C)) + rx[j-1]*(W-C)) at every
  // fused level; `r` is then not used. They hold +0.0 in every pad entry and row
  // outside the grid and keep the faces next to the frame (frame column -1 of rx,
  // frame row -1 of ry). With faces every rect of the launch runs tb_kernel_div
  // (tb_impl.hpp): Dirichlet on both axes, arith 0 / 1, depths 1..kMaxTBDiv, no
  // wave-pair plans, not together with a source or a map.
  const void *rx = nullptr, *ry = nullptr;
  // Needs a source: a per-step gain schedule, level s of the pass adds
  // g[*pos + s - 1] * S — the product rounded, then the add; arith 1:
  // fma(g, S, update), one rounding. g: device array of the field's dtype,
  // readable up to *pos + k entries (the solver pads it by kMaxTBSrc); pos: a
  // device word, read when the kernel runs, so a captured launch takes the
  // position of its replay. Every rect runs tb_kernel_gain, tb_kernel_src's
  // launch shape. {}: the source as it is.
  GainRef gain{};
  // Needed with kBcRobinX / kBcRobinY in bc: the 8 values of the Robin walls'
  // pairs in the field's dtype (kRobinXLo ..), read on the host when the launch
  // is made and passed to tb_kernel_rob by value, so a captured launch keeps
  // them. Every launch that would run tb_kernel_ins runs tb_kernel_rob: arith
  // 0 / 1, depths 1..kMaxTBRob, no source / rmap / faces.
  const double* robin = nullptr;
  // The constant-coefficient five-point operator: 5 values (wS, wE, wN, wW, wC) already
  // converted to the field's dtype, T' = wS*S + wE*E + wN*N + wW*W + wC*C at every fused
  // level with S = T[i+1,j], E = T[i,j+1], N = T[i-1,j], W = T[i,j-1], C = T[i,j] — every
  // product and sum rounded, ((((wS*S + wE*E) + wN*N) + wW*W) + wC*C); arith 1:
  // p = wS*S, then p = fma(w, operand, p) for E, N, W and C — `r` is then not used. Read
  // on the host when the launch is made and passed to tb_kernel_w5 by value, so a captured
  // launch keeps them. Every rect of the launch runs tb_kernel_w5 (tb_impl.hpp): Dirichlet
  // or periodic axes, arith 0 / 1, depths 1..kMaxTBW5, no source / rmap / faces / gain, no
  // fused statistics, no wave-pair plans. nullptr: the scalar-r kernels.
  const double* weights = nullptr;
};

// dst(rows [row_begin,row_end)) = k FTCS steps of src. `src`/`dst` are
// allocation bases laid out per `L`. Requires k <= L.halo and the k ghost rows
// on both sides of the range to hold valid data at time t (Dirichlet rows are
// recognised from L.row0 / L.nrows_global and kept fixed).
void launch_tb(DType dt, const void* src, void* dst, const SlabLayout& L, int64_t row_begin, int64_t row_end, int k,
               double r, hipStream_t stream, int64_t tile_rows = 0, int cus = 0, const TbTerms& terms = {});
// Same for TWO disjoint row ranges [rb0, re0) and [rb1, re1) in one launch.
void launch_tb2(DType dt, const void* src, void* dst, const SlabLayout& L, int64_t rb0, int64_t re0, int64_t rb1,
                int64_t re1, int k, double r, hipStream_t stream, int64_t tile_rows = 0, int cus = 0,
                const TbTerms& terms = {});

// Split schedule of one cycle (k steps over the whole slab) into two launches
// on two streams:
//   MAIN: rows [band, n-band), all strips — the interior kernel (no frame-row
//         code: fewer registers), a persistent grid on all wave slots;
//   EDGE: the two boundary bands (all strips), general kernel.
// The caller orders them with events (solver.cpp). valid = 0: slab too thin
// or narrow for the split (use launch_tb on the whole slab); valid = 2: a
// single-launch plan (plan_single); valid = 3: the split run edge-first — the
// band launch alone, then the interior, both on the compute stream, with the
// halo exchange beside the interior (the autotuner's choice for slabs where
// the interior would otherwise share the chip with the band waves).
// nb > 0: nb row bands per strip (nb x strips work items); nb < 0: -nb equal
// segments of the strip-major row sequence (one work item each, crossing strip
// ends where they fall: equal rows per wave for any strip count).
struct TbRect {
  int64_t r0, r1, s0, s1, nb;
};
// rects of one launch (SplitPlan::rects, the kernel's TbArgs::rect)
constexpr int kMaxPlanRects = 6;
constexpr int32_t kPlanDynamic = 2;  // SplitPlan::flags
constexpr int32_t kPlanLead = 4;     // SplitPlan::flags (valid = 1)
constexpr int32_t kPlanPipe = 8;     // SplitPlan::flags (valid = 1 / 3): the main launch is the wave-pair kernel
struct SplitPlan {
  int32_t k, ring, valid, nedge;
  TbRect main;
  TbRect edge[4];
  int64_t main_waves, edge_waves, main_items, edge_items;
  // nrects > 0 (arith 2): `main` cut into frame-strip-weighted rects,
  // launched instead of `main` (stencil_tb.hip weight_main).
  // flags & kPlanDynamic: the main launch takes its items from a dynamic
  // queue (more items than waves; TbArgs::queue). flags & kPlanLead (valid 1,
  // exchanging slabs): the concurrent order with the band launch issued
  // FIRST — its waves take their slots before the interior's, the interior's
  // last-dispatched waves (its one-item waves) start behind them, and the
  // exchange follows the bands on the comm stream. flags & kPlanPipe (fp64,
  // depths with a tb_kernel_pipe instance): the main launch runs the
  // wave-pair kernel — its rects count WIDE strips (256 columns, 32 B per
  // lane), its items go to pairs of waves: main_waves counts pairs. The edge
  // rects keep the one-wave strips.
  int32_t nrects, flags;
  TbRect rects[kMaxPlanRects];
};
// The same plan with its boundary-band (EDGE) rects cut into `nb` row bands
// each (valid = 1 / 3; default 1): more, shorter band items — nb x as many
// waves for the latency-bound band launch, each marching B/nb + 2k rows
// instead of B + 2k.
SplitPlan with_edge_bands(DType dt, const SplitPlan& p, int64_t nb, int arith = 0);
// ring_override: 4 | 6 (0: default); main_bands: MAIN row bands (0: persistent default;
// < 0: -main_bands segments, TbRect)
// pipe: plan the main launch for the wave-pair kernel (kPlanPipe; needs pipe_available)
SplitPlan plan_split(DType dt, const SlabLayout& L, int k, int64_t band, int cus = 0, int spare_waves = 0,
                     int ring_override = 0, int64_t main_bands = 0, int arith = 0, bool pipe = false);
// Whether the wave-pair interior kernel exists for this dtype, depth and
// arithmetic form (an instance that keeps 2 waves/SIMD without scratch: fp64,
// depths 16..24, all four forms).
bool pipe_available(DType dt, int k, int arith);
// Strip width and useful width (columns) of a plan's main launch.
void plan_strip_shape(DType dt, const SplitPlan& p, int64_t* strip_w, int64_t* useful_w);
// The pair kernel's waits are bounded: a wave that gave up set a status word.
// Raises if any launch since the last call did, and clears the word (call
// after a synchronise; the field is invalid from that launch on).
void pipe_check();
// The alternative the autotuner weighs against the split (valid = 2): ONE
// general launch over the whole slab (no edge part), e.g. for small grids
// where the second launch costs more than it saves.
SplitPlan plan_single(DType dt, const SlabLayout& L, int k, int cus = 0, int ring_override = 0, int64_t bands = 0,
                      int arith = 0);
// Whether the plan's boundary-band launch runs on the interior kernel (its
// bands clear of the global frame rows: every middle rank) rather than the
// general one (1 wave/SIMD at deep fp64 depths).
bool edges_on_main(const SlabLayout& L, const SplitPlan& p);
// One boundary-band rect of the plan alone, on the interior kernel where it
// stays clear of the global frame rows, else the general one (edge ranks).
bool edge_rect_on_main(const SlabLayout& L, const SplitPlan& p, int i);
void launch_edge_rect(DType dt, const void* src, void* dst, const SlabLayout& L, const SplitPlan& p, int i, double r,
                      hipStream_t stream, const TbTerms& terms = {});
// queue: 2 device counters (zeroed once) for plans with flags & kPlanDynamic (dynamic items)
void launch_split(DType dt, const void* src, void* dst, const SlabLayout& L, const SplitPlan& p, bool main_part,
                  double r, hipStream_t stream, const TbTerms& terms = {}, uint32_t* queue = nullptr);

// Initial / boundary condition kinds (covers every IC of the reference
// variants, see models/presets.py for the mapping).
enum class IcKind : int32_t {
  Uniform = 0,   // interior = a, Dirichlet frame = b   (fortran/hip/heat.F90:274-282)
  Box = 1,       // a inside [x0,x1]x[y0,y1] (frame included), else b (fortran/serial/heat.f90:40-48)
  IndexBox = 2,  // a for global frame-index ranges [i0,i1) x [j0,j1), else b (python/serial/heat.py:25)
  Sine = 3,      // a * sin(kx*pi*(x-x0)/(x1-x0)) * sin(ky*pi*(y-y0)/(y1-y0)), frame = 0 (analytic oracle)
  Const = 4,     // a everywhere
};

struct IcParams {
  int32_t kind;
  double a, b;
  double x0, x1, y0, y1;     // box / sine extents
  int64_t i0, i1, j0, j1;    // index box (frame-inclusive global indices: frame row = 0)
  double kx, ky;             // sine mode numbers
  double pad;                // value for allocation padding outside the frame
};

// Fill the whole allocation (owned points, Dirichlet frame, ghost/pad rows)
// from the IC. `xcoord` has nrows_global+2 entries (frame-inclusive, entry 0
// is global row -1), `ycoord` has ncols+2 entries — both device arrays.
void launch_init(DType dt, void* field, const SlabLayout& L, const IcParams& ic,
                 const double* xcoord, const double* ycoord, hipStream_t stream);

// Statistics over the owned region: [sum, sum_sq, min, max, sum_sq_diff, max_abs_diff]
// (diff terms vs `other`, zero if other == nullptr). Deterministic two-pass
// reduction; `work` must hold stats_work_elems() doubles; result (6 doubles)
// written to `out` (device).
int64_t stats_work_elems();
void launch_stats(DType dt, const void* field, const void* other, const SlabLayout& L,
                  double* work, double* out, hipStream_t stream);

// One cycle of k steps over the whole slab (one general launch, like
// plan_single) that also reduces the statistics of the NEW field and its
// one-step residual T_k - T_{k-1} — [sum, sum_sq, min, max, sum_sq_diff,
// max_abs_diff], the launch_stats layout — fused into the march's stored
// level (no extra pass over the field): per-wave partials in `partials`
// (>= kNStat * max_stats_waves() doubles), then a fixed-order reduce into
// out6 (device). Deterministic for a given slab and device.
int64_t max_stats_waves();
// Diagnostics: per-wave {start, end, wave id, 0} (wall clock ticks) of the
// last tb_kernel launch when HEAT2D_WAVE_TIMES=1; returns the waves copied.
int64_t wave_times(uint64_t* out, int64_t max_waves);
// (bc: kBcPeriodicX only — with periodic y the march's widened grid would
// count ghost columns; the solver takes its unfused statistics path there)
void launch_tb_stats(DType dt, const void* src, void* dst, const SlabLayout& L, int k, double r, double* partials,
                     double* out6, hipStream_t stream, int arith = 0, int bc = 0);
void launch_reduce_partials(const double* partials, int64_t nparts, double* out6, hipStream_t stream);

// Field comparison (the bench's check of its timed field against an
// independent engine): rows [ra, ra + nrows) of `a` (layout La) against rows
// [rb, rb + nrows) of `b` (layout Lb), owned columns (La.ncols == Lb.ncols).
// out2 (device) = {max |a - b|, number of elements whose bit patterns differ}
// (NaN anywhere: max = NaN). `work` >= 2 * compare_work_blocks() doubles.
int64_t compare_work_blocks();
void launch_compare(DType dt, const void* a, const SlabLayout& La, int64_t ra, const void* b, const SlabLayout& Lb,
                    int64_t rb, int64_t nrows, double* work, double* out2, hipStream_t stream);

// Vectorised streaming copy / read (bandwidth roof probes; copy-swap mode).
void launch_copy(void* dst, const void* src, int64_t bytes, hipStream_t stream, int blocks = 0);
void launch_read(const void* src, int64_t bytes, unsigned* sink, hipStream_t stream, int blocks = 0);

// Pack/unpack `nrows` rows starting at local row `row` into / from a
// contiguous buffer of nrows*ncols elements (the owned columns only). Used for
// generic transports and host staging; the RCCL path sends rows in place.
void launch_pack_rows(DType dt, const void* field, const SlabLayout& L, int64_t row,
                      int64_t nrows, void* buf, hipStream_t stream);
void launch_unpack_rows(DType dt, void* field, const SlabLayout& L, int64_t row, int64_t nrows,
                        const void* buf, hipStream_t stream);

// IPC transport ordering (kernels/ipc_sync.hip): one 64-B slot per rank in
// host-shared memory; `ctrl` = {abort word, timed-out rank + 1}.
struct IpcSlot {
  uint64_t ready, done;
  uint64_t pad[6];
};
void launch_ipc_arrive(IpcSlot* slots, uint64_t* ctrl, int me, int p0, int p1, uint64_t timeout_ticks,
                       hipStream_t stream);
void launch_ipc_depart(IpcSlot* slots, int me, hipStream_t stream);

}  // namespace kern
}  // namespace heat2d
