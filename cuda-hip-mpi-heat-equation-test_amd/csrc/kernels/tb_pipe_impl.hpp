// The deep fp64 interior march split over a PAIR of waves with 32-byte lanes
// (tb_kernel_pipe; instantiated in tb_f64_pipe_*.hip, planned and launched by
// stencil_tb.hip; probe and measurements: tools/pipe_probe.hip,
// profiles/r7/pipe/).
//
// The one-wave strip (tb_kernel) carries all K levels in one wave's registers,
// which caps an fp64 lane at 16 B at depths 13 and up: 6 adds + 4 DPP moves per
// lane, level and row for 2 points (the r = 1/4 form), and 88 useful columns
// of 128 at K = 20. Here a PRODUCER wave marches levels 1..K1 (K1 =
// ceil(K/2)) and a CONSUMER wave levels K1+1..K of the same 256-column strip.
// Each keeps half the level registers, so 4 doubles per lane fit 2 waves/SIMD:
// 12 adds + 4 DPP moves for 4 points, and 216 useful columns of 256 at K = 20
// — 0.65x the lane-instructions per useful point and level.
//
// The hand-over is ONE-directional. Every level-K1 row goes through an LDS row
// FIFO of kPipeDepth rows of 2 KiB (two planes of 64 x 16 B: every
// ds_write_b128 / ds_read_b128 is contiguous over the lanes). Two monotonic
// row counters per pair (produced, consumed) live in LDS, written by all lanes
// of the owning wave (same value, same address: plain vector LDS stores) and
// read back through readfirstlane. There is no s_barrier in the march: the
// waves couple only through the FIFO, the producer up to kPipeDepth rows
// ahead. Data is ordered against the counters by s_waitcnt lgkmcnt(0) alone
// (the LDS executes one wave's accesses in order), so the producer's ring of
// global loads stays in flight: no vmcnt drain. A wave caches the last value
// it saw of the other's counter and polls (s_sleep) only when that is not
// enough. Index arithmetic: pipe_ring.hpp.
//
// Scaled levels (AR 2 / 3, kind 0): the producer hands over 4^K1 T (T /
// r^K1) as the march carries it; the consumer keeps scaling and unscales once
// at the store: per point the operations and their order are the one-wave
// march's, so the results are bitwise identical to tb_kernel's. Pinned kinds
// stay unscaled in both stages.
//
// A 256-thread workgroup is two pairs: waves 0 and 2 produce, 1 and 3 consume.
// A work item (tb_span / tb_piece over wide strips) belongs to a pair; both
// waves walk the same static item sequence, or, with the dynamic queue, the
// producer draws the item and passes its id through a 2-slot mailbox in the
// pair's header (an id >= nitems ends both loops).
//
// Every wait is bounded by the wall clock: a wave that gives up sets the
// pair's abort flag and a status word the host checks where it synchronises
// (kern::pipe_check); from then on neither wave waits and the consumer's
// stores are dropped. A bug shows as an error, not as a hung GPU.
#pragma once
#include "pipe_ring.hpp"
#include "tb_impl.hpp"

namespace heat2d {
namespace kern {
namespace tbimpl {

#ifndef HEAT2D_PIPE_DEPTH
#define HEAT2D_PIPE_DEPTH 8  // 2 pairs x 8 rows x 2 KiB = 32 KiB per workgroup: 2 workgroups per CU
#endif
constexpr int kPipeDepth = HEAT2D_PIPE_DEPTH;
constexpr int kPipeRowBytes = 64 * 32;
constexpr int kPipeRing = 4;  // level-0 ring of both stages (a producer ring of 6 spills at K = 20)
constexpr uint64_t kPipeTimeoutTicks = 200000000ull;  // 2 s of the 100 MHz wall clock
static_assert((kPipeDepth & (kPipeDepth - 1)) == 0, "FIFO depth must be a power of two");

// strip geometry of the pair kernel: from the TOTAL depth (TbShape ties it to one march's)
template <int K>
struct PipeShape {
  static constexpr int V = 4;
  static constexpr int KA = (K + V - 1) / V * V;
  static constexpr int W = 64 * V;
  static constexpr int U = W - 2 * KA;
  static constexpr int K1 = (K + 1) / 2, K2 = K - K1;
};

// One pair's LDS: the row FIFO, then the header words.
struct PipePairLds {
  alignas(16) char rows[kPipeDepth * kPipeRowBytes];
  uint32_t produced;   // rows the producer has published (monotonic over the launch)
  uint32_t consumed;   // rows the consumer has released
  uint32_t abort;      // a wait gave up: nobody waits any more
  uint32_t item_seq;   // dynamic queue: items the producer has handed over
  uint32_t item_id[2]; // ... and their ids (slot = sequence number & 1)
  uint32_t pad[2];
};

// A wave's side of the hand-over. All lanes execute every access.
struct PipeLink {
  PipePairLds* l;
  uint32_t* status;
  uint32_t seen;       // last value read of the OTHER wave's row counter
  uint32_t seen_item;  // consumer: last value read of item_seq
  uint32_t aborted;    // wave-uniform

  __device__ __forceinline__ static uint32_t ld(const uint32_t* p) {
    return (uint32_t)__builtin_amdgcn_readfirstlane(
        (int)__hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
  }
  __device__ __forceinline__ static void st(uint32_t* p, uint32_t v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  }
  // wait until counter `ctr` (cached in `cache`) has reached `need`
  __device__ __forceinline__ void wait_for(const uint32_t* ctr, uint32_t& cache, uint32_t need) {
    if (pipe::reached(cache, need) || aborted) return;
    uint64_t t_start = 0;
    uint32_t spins = 0;
    for (;;) {
      cache = ld(ctr);
      if (pipe::reached(cache, need)) break;
      if (ld(&l->abort)) {
        aborted = 1;
        break;
      }
      __builtin_amdgcn_s_sleep(2);
      if ((++spins & 255u) == 0) {
        const uint64_t now = wall_clock64();
        if (t_start == 0) t_start = now;
        if (pipe::timed_out(t_start, now, kPipeTimeoutTicks)) {
          st(&l->abort, 1u);
          *status = 1u;
          aborted = 1;
          break;
        }
      }
    }
    asm volatile("" ::: "memory");
  }
  // all earlier LDS accesses of this wave have completed; then publish v
  __device__ __forceinline__ void publish(uint32_t* ctr, uint32_t v) {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    st(ctr, v);
  }
};

// One stage of the pair: ROLE 0 the producer (level 0 from global memory,
// level K1 into the FIFO), ROLE 1 the consumer (level 0 from the FIFO, level
// K2 — level K of the cycle — to global memory). The arithmetic, the level
// registers and the descriptors are March's (one chain, NV = 2).
template <int K, int EK, int AR, int ROLE>
struct PipeStage {
  using P = PipeShape<K>;
  static constexpr int KS = ROLE == 0 ? P::K1 : P::K2;
  static constexpr int RING = kPipeRing, L = kPipeRing, V = 4, NV = 2;
  using M = March<double, NV, KS, EK, RING, AR, false, KS>;
  using VT = typename M::VT;
  using U4 = typename M::U4;
  M w;
  PipeLink lk;
  uint32_t q;        // FIFO index of the next row written (producer) / read (consumer)
  uint32_t qend;     // consumer: the item's last FIFO row + 1 (reads never wait past it)
  int32_t lds_lane;  // lane * 16

  __device__ __forceinline__ char* fifo_row(uint32_t idx) const {
    return lk.l->rows + pipe::slot(idx, kPipeDepth) * kPipeRowBytes + lds_lane;
  }
  __device__ __forceinline__ void refill(int slot, bool row_live) {
    if constexpr (ROLE == 0) {
      const __amdgpu_buffer_rsrc_t rs = row_rsrc(w.lp, row_live ? w.nrec : 0u);
#pragma unroll
      for (int v = 0; v < NV; ++v) {
        U4 b = __builtin_amdgcn_raw_buffer_load_b128(rs, w.ld_off + v * 16, 0, 0);
        w.Lb[slot][v] = __builtin_bit_cast(VT, b);
      }
      w.lp -= w.pitch_b;
    } else {
      // the rows read so far are in registers: release them, then take row q
      lk.publish(&lk.l->consumed, q);
      lk.wait_for(&lk.l->produced, lk.seen, pipe::read_need(q, qend));
      const char* p = fifo_row(q);
      w.Lb[slot][0] = *reinterpret_cast<const VT*>(p);
      w.Lb[slot][1] = *reinterpret_cast<const VT*>(p + 1024);
      // issue the reads here, a march row before the next release waits for them
      __builtin_amdgcn_sched_barrier(0);
      ++q;
    }
  }
  template <int PH, bool PRIME = false>
  __device__ __forceinline__ void step(int32_t m, int32_t nl = KS) {
    constexpr int P0 = PH % RING;
    constexpr int sN = P0, sC = (P0 + RING - 1) % RING, sS = (P0 + RING - 2) % RING;
    constexpr int cur = PH & 1, prv = cur ^ 1;
    if constexpr (ROLE == 0) {
      // the rows written so far are complete: publish them, then wait for room for row q
      lk.publish(&lk.l->produced, q);
      lk.wait_for(&lk.l->consumed, lk.seen, pipe::write_need(q, kPipeDepth));
    }
    double part[V], C0[V], N0[V];
    {
      double S0[V];
      w.unpack(w.Lb[sS], S0);
      w.unpack(w.Lb[sC], C0);
      w.partial(S0, C0, part);
    }
    __builtin_amdgcn_sched_barrier(0);
    refill(sS, m + 2 - RING >= w.mload);
    w.unpack(w.Lb[sN], N0);
#pragma unroll
    for (int s = 1; s <= KS; ++s) {
      if (PRIME && s > nl) continue;
      double C[V], N[V], out[V], nxtpart[V];
#pragma unroll
      for (int e = 0; e < V; ++e) {
        C[e] = s == 1 ? C0[e] : w.X[prv][s > 1 ? s - 2 : 0][e];
        N[e] = s == 1 ? N0[e] : w.X[cur][s > 1 ? s - 2 : 0][e];
      }
      if (s < KS) w.partial(w.X[cur][s - 1], w.X[prv][s - 1], nxtpart);
      w.update(part, C, N, 0, out);  // (the row only matters to frame-row kinds: none here)
      if (s < KS) {
#pragma unroll
        for (int e = 0; e < V; ++e) w.X[cur][s - 1][e] = out[e];
#pragma unroll
        for (int e = 0; e < V; ++e) part[e] = nxtpart[e];
      } else if constexpr (ROLE == 0) {
        char* p = fifo_row(q);
        VT a, b;
        a[0] = out[0];
        a[1] = out[1];
        b[0] = out[2];
        b[1] = out[3];
        *reinterpret_cast<VT*>(p) = a;
        *reinterpret_cast<VT*>(p + 1024) = b;
      } else {
        const int32_t row = m + KS;
        const bool live = (uint32_t)(row - w.t0) < (uint32_t)(w.t1 - w.t0);
        if constexpr (M::kScaled) {
          const double u = AR == 2 ? inv_pow4<double>(K) : w.fu;  // the whole cycle's scale
#pragma unroll
          for (int e = 0; e < V; ++e) out[e] *= u;
        }
        w.store_row(w.sp, live && !lk.aborted, out);
      }
    }
    if constexpr (ROLE == 0) ++q;
    else w.sp -= w.pitch_b;
  }
  template <int... I>
  __device__ __forceinline__ void body(int32_t m, std::integer_sequence<int, I...>) {
    (step<I>(m - I), ...);
  }
  template <int... I>
  __device__ __forceinline__ void body_prime(int32_t m, int32_t i, std::integer_sequence<int, I...>) {
    (step<I, true>(m - I, ChainShape<KS, KS>::levels_at(i + I)), ...);
  }
  // base: the pair's FIFO row count before this item; fifo_rows: the item's
  __device__ __forceinline__ void run(uint32_t base, uint32_t fifo_rows, int32_t bodies) {
    w.mload = w.t0 - KS;
    const int32_t mtop = w.t1 + KS - 1;
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
      for (int s = 0; s < M::KX; ++s)
#pragma unroll
        for (int e = 0; e < V; ++e) w.X[p][s][e] = 0.0;
    if constexpr (ROLE == 0) {
      q = base;
      w.lp = w.srow + (int64_t)mtop * w.pitch_b;
    } else {
      // the producer's first 2 K1 rows only prime its levels: released unread
      q = base + pipe::skip_rows(P::K1);
      qend = base + fifo_rows;
      w.sp = w.drow + (int64_t)(mtop + KS) * w.pitch_b;
    }
#pragma unroll
    for (int s = 0; s < RING - 2; ++s) refill(s, true);  // rows mtop, mtop - 1: both >= mload
#pragma unroll
    for (int s = RING - 2; s < RING; ++s)
#pragma unroll
      for (int v = 0; v < NV; ++v) w.Lb[s][v] = VT{};
    const int32_t pb = min(bodies, (int32_t)((2 * KS + L - 1) / L));
    int32_t m = mtop;
    int32_t b = 0;
#pragma unroll 1
    for (; b < pb; ++b) {
      body_prime(m, b * L, std::make_integer_sequence<int, L>{});
      m -= L;
    }
#pragma unroll 1
    for (; b < bodies; ++b) {
      body(m, std::make_integer_sequence<int, L>{});
      m -= L;
    }
    // the item's rows are all written / read: move the counter to the item's end
    if constexpr (ROLE == 0) lk.publish(&lk.l->produced, base + fifo_rows);
    else lk.publish(&lk.l->consumed, base + fifo_rows);
  }
};

// one stage's march of wide strip `strip`, output rows [t0, t1)
template <int K, int EK, int AR, int ROLE>
__device__ __forceinline__ void pipe_march(const double* src, double* dst, const TbArgs& a, double r, int64_t strip,
                                           int64_t t0, int64_t t1, int lane, PipeLink& lk, uint32_t base,
                                           const pipe::ItemRows& ir) {
  using P = PipeShape<K>;
  PipeStage<K, EK, AR, ROLE> s;
  auto& w = s.w;
  const int64_t u0 = strip * P::U, c0 = u0 - P::KA;
  const int64_t ustop = min(u0 + (int64_t)P::U, a.ncols);
  const int64_t mycol = c0 + (int64_t)lane * P::V;
  w.srow = reinterpret_cast<const char*>(src + a.col_lo);
  w.drow = reinterpret_cast<char*>(dst + a.col_lo);
  w.pitch_b = a.pitch * 8;
  w.nrec = (uint32_t)(a.pitch * 8);
  w.r = r;
  if constexpr (AR == 3) {
    w.fk = 1.0 - 4.0 * r;
    w.fb = a.fb;
    w.fu = a.fu;
    w.fu1 = a.fu1;
  }
  // the producer's output rows are the level-K1 rows the consumer needs
  w.t0 = (int32_t)t0 - (ROLE == 0 ? P::K2 : 0);
  w.t1 = (int32_t)t1 + (ROLE == 0 ? P::K2 : 0);
  w.fixed_lo = (int32_t)a.fixed_lo;
  w.fixed_hi = (int32_t)a.fixed_hi;
  const int32_t off = (int32_t)((mycol - a.col_lo) * 8);
  const bool in_alloc = (mycol >= a.col_lo) && (mycol + P::V <= a.col_hi);
  w.ld_off = in_alloc ? off : kOob;
  // (strip boundaries are multiples of V; the lane straddling ncols writes its
  // pinned elements back unchanged: see march())
  w.st_off = (in_alloc && mycol >= u0 && mycol < ustop) ? off : kOob;
  if constexpr ((EK & 2) != 0) {
#pragma unroll
    for (int e = 0; e < P::V; ++e) w.rl[e] = (mycol + e < 0 || mycol + e >= a.ncols) ? 0.0 : r;
  }
  s.lk = lk;
  s.lds_lane = lane * 16;
  s.run(base, ir.fifo_rows, ROLE == 0 ? ir.bodies_p : ir.bodies_c);
  lk = s.lk;
}

template <int K, int AR>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void tb_kernel_pipe(
    const double* __restrict__ src, double* __restrict__ dst, TbArgs a, double r, uint32_t* status) {
  using P = PipeShape<K>;
  __shared__ PipePairLds lds[2];
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int role = wv & 1;
  PipePairLds* l = &lds[wv >> 1];
  (&l->produced)[lane & 7] = 0u;  // the header words; both waves of the pair write the same zeros
  __syncthreads();                // the only barrier: before any hand-over
  const int64_t pid = (int64_t)blockIdx.x * 2 + (wv >> 1);  // a.nwaves counts PAIRS here
  if (pid >= a.nwaves) return;                             // both waves of the pair
  PipeLink lk{l, status, 0u, 0u, 0u};
  uint32_t base = 0, nhand = 0;
  int64_t it = pid;
  int32_t lin = tb_span<kMainRects>(a, it).lin;
  while (it < a.nitems) {
    int64_t strip, t0, t1;
    if (!tb_piece<kMainRects>(a, it, lin, strip, t0, t1)) {
      if (!a.queue) {
        it += a.nwaves;
      } else if (role == 0) {  // the producer draws the item and hands its id over
        it = next_item(a, it);
        PipeLink::st(&l->item_id[nhand & 1u], (uint32_t)it);
        ++nhand;
        lk.publish(&l->item_seq, nhand);
      } else {
        ++nhand;
        lk.wait_for(&l->item_seq, lk.seen_item, nhand);
        it = lk.aborted ? a.nitems : (int64_t)PipeLink::ld(&l->item_id[(nhand - 1u) & 1u]);
      }
      if (it < a.nitems) lin = tb_span<kMainRects>(a, it).lin;
      continue;
    }
    lin += (int32_t)(t1 - t0);
    const int64_t c0 = strip * P::U - P::KA;
    const bool frame = (c0 < 0) || (c0 + P::W > a.ncols);
    const pipe::ItemRows ir = pipe::item_rows((int32_t)(t1 - t0), P::K1, P::K2, kPipeRing, kPipeRing);
    if (role == 0) {
      if (frame) pipe_march<K, 2, AR, 0>(src, dst, a, r, strip, t0, t1, lane, lk, base, ir);
      else pipe_march<K, 0, AR, 0>(src, dst, a, r, strip, t0, t1, lane, lk, base, ir);
    } else {
      if (frame) pipe_march<K, 2, AR, 1>(src, dst, a, r, strip, t0, t1, lane, lk, base, ir);
      else pipe_march<K, 0, AR, 1>(src, dst, a, r, strip, t0, t1, lane, lk, base, ir);
    }
    base += ir.fifo_rows;
    if (lk.aborted) break;
  }
  if (role == 0) queue_exit(a);  // (counts a.nwaves finishers: the producers)
}

// Entry points, instantiated per arithmetic form in tb_f64_pipe_*.hip.
constexpr int kPipeMinK = 16, kPipeMaxK = 24;
template <int AR>
void dispatch_pipe(int k, unsigned nblocks, const double* src, double* dst, const TbArgs& a, double r,
                   uint32_t* status, hipStream_t s);
template <int AR>
int occupancy_blocks_pipe(int k);

#define H2D_PIPE_CASE(AR, KK)                                                                                    \
  case KK:                                                                                                       \
    hipLaunchKernelGGL((tb_kernel_pipe<KK, AR>), dim3(nblocks), dim3(256), 0, s, src, dst, a, r, status);        \
    return;
#define H2D_PIPE_OCC_CASE(AR, KK)                                                                                \
  case KK: {                                                                                                     \
    int nb = 0;                                                                                                  \
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, reinterpret_cast<const void*>(&tb_kernel_pipe<KK, AR>), \
                                                     256, 0) != hipSuccess)                                      \
      nb = 0;                                                                                                    \
    return nb;                                                                                                   \
  }
#define H2D_PIPE_CASES(M, AR) \
  M(AR, 16) M(AR, 17) M(AR, 18) M(AR, 19) M(AR, 20) M(AR, 21) M(AR, 22) M(AR, 23) M(AR, 24)
#define H2D_PIPE_UNIT(AR)                                                                                 \
  template <>                                                                                             \
  void dispatch_pipe<AR>(int k, unsigned nblocks, const double* src, double* dst, const TbArgs& a, double r, \
                         uint32_t* status, hipStream_t s) {                                               \
    switch (k) {                                                                                          \
      H2D_PIPE_CASES(H2D_PIPE_CASE, AR)                                                                   \
      default:                                                                                            \
        break;                                                                                            \
    }                                                                                                     \
    HEAT2D_REQUIRE(false, "temporal depth not instantiated for the wave-pair kernel");                    \
  }                                                                                                       \
  template <>                                                                                             \
  int occupancy_blocks_pipe<AR>(int k) {                                                                  \
    switch (k) {                                                                                          \
      H2D_PIPE_CASES(H2D_PIPE_OCC_CASE, AR)                                                               \
      default:                                                                                            \
        break;                                                                                            \
    }                                                                                                     \
    return 0;                                                                                             \
  }

}  // namespace tbimpl
}  // namespace kern
}  // namespace heat2d
