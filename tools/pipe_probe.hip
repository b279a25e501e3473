// Round 7 probe: the deep fp64 r = 1/4 interior march split over a PAIR of
// waves, with 32-byte lanes (4 doubles per lane, NV = 2).
//
// The one-wave strip (the production march, tb_impl.hpp; copied below as the
// baseline, as in tools/tile_probe.hip) carries all K levels in one wave's
// registers, which caps a lane at 16 B: 6 v_add_f64 + 4 DPP moves per lane,
// level and row for 2 points, and 88 useful columns of 128 at K = 20. Here a
// PRODUCER wave marches levels 1..K1 and a CONSUMER wave levels K1+1..K
// (K1 = ceil(K/2)) of the same 256-column strip. Each holds half the level
// registers, so 4 doubles per lane fit: 12 adds + 4 DPP moves for 4 points,
// and 216 useful columns of 256 at K = 20.
//
// The hand-over is ONE-directional: every level-K1 row (scaled by 4^K1, as
// the march carries it) goes through an LDS row FIFO of kDepth rows, 2 KiB
// each (two planes of 64 x 16 B, so each ds_write_b128 / ds_read_b128 is
// contiguous over the lanes). Two monotonic row counters per pair live in LDS
// (produced, consumed), written by all lanes of the owning wave (same value,
// same address) and read back through readfirstlane. No s_barrier: the waves
// couple only through the FIFO, the producer up to kDepth rows ahead. Data is
// ordered against the counters by s_waitcnt lgkmcnt(0) alone, so the
// producer's ring of global loads stays in flight. Each wave caches the last
// counter value it saw and polls (s_sleep) only when that is not enough.
//
// Every wait is bounded by the wall clock (kTimeoutTicks of the 100 MHz
// counter): a wave that gives up sets a status word in global memory and the
// pair's abort flag; from then on neither wave waits, the consumer's stores
// are dropped, and the host reports the status. A bug shows as a failed
// check, not as a hung GPU.
//
// Operation order per point is the strip's, so the output is checked bitwise
// against the strips over the whole interior. Both kernels are timed over
// the same row-band counts (best of 5 launches each).
//
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off
//     -I cuda-hip-mpi-heat-equation-test_amd/csrc/include
//     -I cuda-hip-mpi-heat-equation-test_amd/csrc/kernels tools/pipe_probe.hip -o pipe_probe
//   pipe_probe <n> <K: 20 | 24>
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>

#include "pipe_ring.hpp"
#include "tb_impl.hpp"

#define CK(x)                                                                          \
  do {                                                                                 \
    hipError_t e_ = (x);                                                               \
    if (e_ != hipSuccess) {                                                            \
      std::fprintf(stderr, "%s:%d %s: %s\n", __FILE__, __LINE__, #x, hipGetErrorString(e_)); \
      std::exit(1);                                                                    \
    }                                                                                  \
  } while (0)

#ifndef PP_DEPTH
#define PP_DEPTH 8  // FIFO rows per pair
#endif
#ifndef PP_RING_P
#define PP_RING_P 4  // producer's ring of global loads (6 spills at K = 20)
#endif

#ifndef PP_LATE
#define PP_LATE 0  // where the producer publishes (PMarch::hand_over)
#endif

namespace probe {
using namespace heat2d::kern::tbimpl;
namespace pr = heat2d::kern::pipe;

using VT = double __attribute__((ext_vector_type(2)));
using U4 = unsigned int __attribute__((ext_vector_type(4)));

struct Args {
  int64_t pitch;   // elements per row
  int64_t cpad;    // columns left of column 0 in the allocation
  int64_t nrows, ncols;
  int64_t nb;      // row bands
  int64_t nunits;  // strips per band
  int64_t nitems, nworkers;  // workers: waves (strips) or pairs (pipe)
  uint32_t* status;          // pipe: set when a wait gave up
};

// ---------------------------------------------------------------- baseline
// One wave per strip, 16-B lanes: March's fp64 kind-0 AR-2 path with the
// priming skip (the copy tools/tile_probe.hip carries, its tile logic removed).
template <int K, int CL, int RING>
struct SMarch {
  static constexpr int V = 2;
  using Ch = ChainShape<K, CL>;
  static constexpr int KX = K - 1;
  static constexpr int L = Ch::unroll(RING);
  const char* srow;
  char* drow;
  const char* lp;
  char* sp;
  int64_t pitch_b;
  uint32_t nrec;
  int32_t t0, t1, mlo, mload, ld_off, st_off;
  double X[3][KX][V];
  VT Lb[RING];

  __device__ __forceinline__ void load_row_p(const char* p, bool live, VT& out) const {
    const __amdgpu_buffer_rsrc_t rs = row_rsrc(p, live ? nrec : 0u);
    U4 b = __builtin_amdgcn_raw_buffer_load_b128(rs, ld_off, 0, 0);
    out = __builtin_bit_cast(VT, b);
  }
  __device__ __forceinline__ void store_row(char* p, bool live, const double (&o)[V]) const {
    const __amdgpu_buffer_rsrc_t rs = row_rsrc(p, live ? nrec : 0u);
    VT w;
    w[0] = o[0];
    w[1] = o[1];
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(U4, w), rs, st_off, 0, HEAT2D_STORE_AUX);
  }
  __device__ __forceinline__ static void unpack(const VT& x, double (&o)[V]) {
    o[0] = x[0];
    o[1] = x[1];
  }
  __device__ __forceinline__ void partial(const double (&Sx)[V], const double (&C)[V], double (&part)[V]) const {
    const double eastL = from_upper(C[0]);
    part[0] = Sx[0] + C[1];
    part[1] = Sx[1] + eastL;
  }
  __device__ __forceinline__ void update(const double (&part)[V], const double (&C)[V], const double (&N)[V],
                                         double (&out)[V]) const {
    const double west0 = from_lower(C[V - 1]);
    out[0] = (part[0] + N[0]) + west0;
    out[1] = (part[1] + N[1]) + C[0];
  }
  template <int PH, bool PRIME = false>
  __device__ __forceinline__ void step(int32_t m, int32_t nl = K) {
    constexpr int P0 = PH % RING;
    constexpr int sN = P0, sC = (P0 + RING - 1) % RING, sS = (P0 + RING - 2) % RING;
    double part[V], C0[V], N0[V];
    {
      double S0[V];
      unpack(Lb[sS], S0);
      unpack(Lb[sC], C0);
      partial(S0, C0, part);
    }
    {
      __builtin_amdgcn_sched_barrier(0);
      load_row_p(lp, m + 2 - RING >= mload, Lb[sS]);
      lp -= pitch_b;
    }
    unpack(Lb[sN], N0);
#pragma unroll
    for (int s = 1; s <= K; ++s) {
      if (PRIME && s > nl) continue;
      double C[V], N[V], out[V], nxtpart[V];
      const int d = Ch::delta(s);
      const int j = s > 1 ? s - 1 : 1;
#pragma unroll
      for (int e = 0; e < V; ++e) {
        C[e] = s == 1 ? C0[e] : X[Ch::slot(PH, d, j)][j - 1][e];
        N[e] = s == 1 ? N0[e] : X[Ch::slot(PH, d - 1, j)][j - 1][e];
      }
      const int ps = Ch::slot(PH, 0, s < K ? s : 1);
      if (s < K) partial(X[ps][s - 1], X[Ch::slot(PH, Ch::delta(s + 1), s)][s - 1], nxtpart);
      update(part, C, N, out);
      if (s < K) {
#pragma unroll
        for (int e = 0; e < V; ++e) X[ps][s - 1][e] = out[e];
#pragma unroll
        for (int e = 0; e < V; ++e) part[e] = nxtpart[e];
      } else {
        const int32_t row = m + Ch::off(K);
        const bool live = (uint32_t)(row - t0) < (uint32_t)(t1 - t0);
        constexpr double u = inv_pow4<double>(K);
#pragma unroll
        for (int e = 0; e < V; ++e) out[e] *= u;
        store_row(sp, live, out);
      }
    }
    sp -= pitch_b;
  }
  template <int... I>
  __device__ __forceinline__ void body(int32_t m, std::integer_sequence<int, I...>) {
    (step<I>(m - I), ...);
  }
  template <int... I>
  __device__ __forceinline__ void body_prime(int32_t m, int32_t i, std::integer_sequence<int, I...>) {
    (step<I, true>(m - I, Ch::levels_at(i + I)), ...);
  }
  __device__ __forceinline__ void run() {
    mload = t0 - K;
    mlo = t0 - Ch::off(K);
    const int32_t mtop = t1 + K - 1;
    lp = srow + (int64_t)(mtop + 2 - RING) * pitch_b;
    sp = drow + (int64_t)(mtop + Ch::off(K)) * pitch_b;
#pragma unroll
    for (int q = 0; q < RING - 2; ++q)
      load_row_p(srow + (int64_t)(mtop - q >= mload ? mtop - q : mload) * pitch_b, true, Lb[q]);
#pragma unroll
    for (int q = RING - 2; q < RING; ++q) Lb[q] = VT{};
#pragma unroll
    for (int p = 0; p < 3; ++p)
#pragma unroll
      for (int s = 0; s < KX; ++s)
#pragma unroll
        for (int e = 0; e < V; ++e) X[p][s][e] = 0.0;
    const int32_t iters = mtop - mlo + 1;
    const int32_t bodies = (iters + L - 1) / L;
    const int32_t pb = min(bodies, (int32_t)((Ch::prime_iters + L - 1) / L));
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
  }
};

template <int K>
struct StripCfg {
  // the production interior configuration at this depth: chains of 4 and a
  // ring of 6 up to K = 20; one chain and a ring of 4 (2 waves/SIMD floor) above
  static constexpr int CL = K <= 20 ? 4 : K;
  static constexpr int RING = K <= 20 ? 6 : 4;
  static constexpr int KA = (K + 1) / 2 * 2, W = 128, U = W - 2 * KA;
};

__device__ __forceinline__ void band_rows(const Args& a, int64_t band, int64_t& t0, int64_t& t1) {
  t0 = band * a.nrows / a.nb;
  t1 = (band + 1) * a.nrows / a.nb;
}

template <int K>
__global__ __launch_bounds__(128) __attribute__((amdgpu_waves_per_eu(2))) void strip_kernel(const double* src,
                                                                                              double* dst, Args a) {
  using C = StripCfg<K>;
  const int lane = threadIdx.x & 63;
  const int64_t wid = (int64_t)blockIdx.x * 2 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  for (int64_t it = wid; it < a.nitems; it += a.nworkers) {
    const int64_t band = it / a.nunits, s = it - band * a.nunits;
    int64_t t0, t1;
    band_rows(a, band, t0, t1);
    const int64_t u0 = s * C::U, c0 = u0 - C::KA, ustop = min(u0 + (int64_t)C::U, a.ncols);
    SMarch<K, C::CL, C::RING> w;
    w.srow = reinterpret_cast<const char*>(src - a.cpad);
    w.drow = reinterpret_cast<char*>(dst - a.cpad);
    w.pitch_b = a.pitch * 8;
    w.nrec = (uint32_t)(a.pitch * 8);
    w.t0 = (int32_t)t0;
    w.t1 = (int32_t)t1;
    const int64_t mycol = c0 + (int64_t)lane * 2;
    const bool in_alloc = mycol >= -a.cpad && mycol + 2 <= a.pitch - a.cpad;
    w.ld_off = in_alloc ? (int32_t)((mycol + a.cpad) * 8) : kOob;
    w.st_off = (in_alloc && mycol >= u0 && mycol < ustop) ? (int32_t)((mycol + a.cpad) * 8) : kOob;
    w.run();
  }
}

// -------------------------------------------------------------- pair pipeline
constexpr int kDepth = PP_DEPTH;
constexpr int kRowBytes = 64 * 32;
constexpr uint64_t kTimeoutTicks = 200000000ull;  // 2 s of the 100 MHz wall clock
static_assert((kDepth & (kDepth - 1)) == 0, "FIFO depth must be a power of two");

// One pair's LDS: the row FIFO, then the header words.
struct PairLds {
  alignas(16) char rows[kDepth * kRowBytes];
  uint32_t produced;  // rows the producer has published (monotonic over the items of the launch)
  uint32_t consumed;  // rows the consumer has released
  uint32_t abort;     // a wait gave up: nobody waits any more
  uint32_t pad;
};

// The wave's side of the hand-over. All lanes execute every access (same
// address, same value): no exec-masked branch, the counters are plain vector
// LDS accesses.
struct Link {
  PairLds* l;
  uint32_t* status;
  uint32_t seen;     // last value read of the OTHER wave's counter
  uint32_t aborted;  // wave-uniform

  __device__ __forceinline__ static uint32_t ld(const uint32_t* p) {
    return (uint32_t)__builtin_amdgcn_readfirstlane(
        (int)__hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
  }
  __device__ __forceinline__ static void st(uint32_t* p, uint32_t v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  }
  // wait until the other wave's counter `ctr` has reached `need`
  __device__ __forceinline__ void wait_for(const uint32_t* ctr, uint32_t need) {
    if (pr::reached(seen, need) || aborted) return;
    uint64_t t_start = 0;
    uint32_t spins = 0;
    for (;;) {
      seen = ld(ctr);
      if (pr::reached(seen, need)) break;
      if (ld(&l->abort)) {
        aborted = 1;
        break;
      }
      __builtin_amdgcn_s_sleep(2);
      if ((++spins & 255u) == 0) {
        const uint64_t now = wall_clock64();
        if (t_start == 0) t_start = now;
        if (pr::timed_out(t_start, now, kTimeoutTicks)) {
          st(&l->abort, 1u);
          *status = 1u;
          aborted = 1;
          break;
        }
      }
    }
    asm volatile("" ::: "memory");
  }
  // all earlier LDS accesses of this wave have completed; publish `v`
  __device__ __forceinline__ void publish(uint32_t* ctr, uint32_t v) {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    st(ctr, v);
  }
};

// ROLE 0: producer (level 0 from global memory, level KS into the FIFO);
// ROLE 1: consumer (level 0 from the FIFO, level KS scaled by 4^-KTOT to
// global memory). One chain, 4 doubles per lane.
template <int KS, int ROLE, int KTOT, int RING>
struct PMarch {
  static constexpr int V = 4, NV = 2;
  static constexpr int KX = KS > 1 ? KS - 1 : 1;
  static constexpr int L = RING;
  static constexpr int K1 = KTOT - (ROLE == 0 ? 0 : KS);  // consumer: the producer's depth
  static_assert(RING % 2 == 0 && RING >= 4, "ring must be even and >= 4");
  const char* srow;
  char* drow;
  const char* lp;
  char* sp;
  int64_t pitch_b;
  uint32_t nrec;
  int32_t t0, t1, mload, ld_off, st_off;  // [t0, t1): this stage's output rows
  uint32_t q;     // FIFO index of the next row written (producer) / read (consumer)
  uint32_t qend;  // consumer: FIFO rows of this item (reads never wait past it)
  int32_t lds_lane;  // lane * 16
  Link lk;
  double X[2][KX][V];
  VT Lb[RING][NV];

  __device__ __forceinline__ char* fifo_row(uint32_t idx) const {
    return lk.l->rows + pr::slot(idx, kDepth) * kRowBytes + lds_lane;
  }
  __device__ __forceinline__ void refill(int slot, int32_t row_live) {
    if constexpr (ROLE == 0) {
      const __amdgpu_buffer_rsrc_t rs = row_rsrc(lp, row_live ? nrec : 0u);
#pragma unroll
      for (int v = 0; v < NV; ++v) {
        U4 b = __builtin_amdgcn_raw_buffer_load_b128(rs, ld_off + v * 16, 0, 0);
        Lb[slot][v] = __builtin_bit_cast(VT, b);
      }
      lp -= pitch_b;
    } else {
      // rows read so far are in registers: release them, then take row q
      lk.publish(&lk.l->consumed, q);
      lk.wait_for(&lk.l->produced, pr::read_need(q, qend));
      const char* p = fifo_row(q);
      Lb[slot][0] = *reinterpret_cast<const VT*>(p);
      Lb[slot][1] = *reinterpret_cast<const VT*>(p + 1024);
      // issue the reads here, a march row before the next release waits for them
      __builtin_amdgcn_sched_barrier(0);
      ++q;
    }
  }
  // producer: the rows written so far are complete: publish them, then wait
  // for room for row q. PP_LATE 0: at the top of the march row (the LDS wait
  // follows the previous row's write closely); 1: just before the row's write
  // (a whole march row after the previous one, but the wait loop then sits in
  // the middle of the levels and costs registers: K = 24 spills).
  __device__ __forceinline__ void hand_over() {
    lk.publish(&lk.l->produced, q);
    lk.wait_for(&lk.l->consumed, pr::write_need(q, kDepth));
  }
  __device__ __forceinline__ void emit(const double (&o)[V]) {
    // producer: level KS of this march row into FIFO row q
    char* p = fifo_row(q);
    VT a, b;
    a[0] = o[0];
    a[1] = o[1];
    b[0] = o[2];
    b[1] = o[3];
    *reinterpret_cast<VT*>(p) = a;
    *reinterpret_cast<VT*>(p + 1024) = b;
  }
  __device__ __forceinline__ void store_row(char* p, bool live, const double (&o)[V]) const {
    const __amdgpu_buffer_rsrc_t rs = row_rsrc(p, live ? nrec : 0u);
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      VT w;
      w[0] = o[v * 2];
      w[1] = o[v * 2 + 1];
      __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(U4, w), rs, st_off + v * 16, 0, HEAT2D_STORE_AUX);
    }
  }
  __device__ __forceinline__ static void unpack(const VT (&x)[NV], double (&o)[V]) {
    o[0] = x[0][0];
    o[1] = x[0][1];
    o[2] = x[1][0];
    o[3] = x[1][1];
  }
  __device__ __forceinline__ void partial(const double (&Sx)[V], const double (&C)[V], double (&part)[V]) const {
    const double eastL = from_upper(C[0]);
#pragma unroll
    for (int e = 0; e < V; ++e) part[e] = Sx[e] + (e < V - 1 ? C[e + 1] : eastL);
  }
  __device__ __forceinline__ void update(const double (&part)[V], const double (&C)[V], const double (&N)[V],
                                         double (&out)[V]) const {
    const double west0 = from_lower(C[V - 1]);
#pragma unroll
    for (int e = 0; e < V; ++e) out[e] = (part[e] + N[e]) + (e > 0 ? C[e - 1] : west0);
  }
  template <int PH, bool PRIME = false>
  __device__ __forceinline__ void step(int32_t m, int32_t nl = KS) {
    constexpr int P0 = PH % RING;
    constexpr int sN = P0, sC = (P0 + RING - 1) % RING, sS = (P0 + RING - 2) % RING;
    constexpr int cur = PH & 1, prv = cur ^ 1;
    if constexpr (ROLE == 0 && !PP_LATE) hand_over();
    double part[V], C0[V], N0[V];
    {
      double S0[V];
      unpack(Lb[sS], S0);
      unpack(Lb[sC], C0);
      partial(S0, C0, part);
    }
    __builtin_amdgcn_sched_barrier(0);
    refill(sS, m + 2 - RING >= mload);
    unpack(Lb[sN], N0);
#pragma unroll
    for (int s = 1; s <= KS; ++s) {
      if (PRIME && s > nl) continue;
      double C[V], N[V], out[V], nxtpart[V];
#pragma unroll
      for (int e = 0; e < V; ++e) {
        C[e] = s == 1 ? C0[e] : X[prv][s - 2][e];
        N[e] = s == 1 ? N0[e] : X[cur][s - 2][e];
      }
      if (s < KS) partial(X[cur][s - 1], X[prv][s - 1], nxtpart);
      update(part, C, N, out);
      if (s < KS) {
#pragma unroll
        for (int e = 0; e < V; ++e) X[cur][s - 1][e] = out[e];
#pragma unroll
        for (int e = 0; e < V; ++e) part[e] = nxtpart[e];
      } else if constexpr (ROLE == 0) {
        if constexpr (PP_LATE) hand_over();
        emit(out);
      } else {
        const int32_t row = m + KS;
        const bool live = (uint32_t)(row - t0) < (uint32_t)(t1 - t0);
        constexpr double u = inv_pow4<double>(KTOT);
#pragma unroll
        for (int e = 0; e < V; ++e) out[e] *= u;
        store_row(sp, live && !lk.aborted, out);
      }
    }
    if constexpr (ROLE == 0) ++q;
    else sp -= pitch_b;
  }
  template <int... I>
  __device__ __forceinline__ void body(int32_t m, std::integer_sequence<int, I...>) {
    (step<I>(m - I), ...);
  }
  template <int... I>
  __device__ __forceinline__ void body_prime(int32_t m, int32_t i, std::integer_sequence<int, I...>) {
    (step<I, true>(m - I, ChainShape<KS, KS>::levels_at(i + I)), ...);
  }
  // base: the pair's FIFO row count before this item; nrows_p: FIFO rows of the item
  __device__ __forceinline__ void run(uint32_t base, uint32_t nrows_p, int32_t bodies) {
    mload = t0 - KS;
    const int32_t mtop = t1 + KS - 1;
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
      for (int s = 0; s < KX; ++s)
#pragma unroll
        for (int e = 0; e < V; ++e) X[p][s][e] = 0.0;
    if constexpr (ROLE == 0) {
      q = base;
      lp = srow + (int64_t)mtop * pitch_b;
#pragma unroll
      for (int s = 0; s < RING - 2; ++s) refill(s, true);  // rows mtop .. mtop - (RING - 3): all >= mload
    } else {
      // the producer's first 2 K1 rows only prime its levels: never read
      q = base + pr::skip_rows(K1);
      qend = base + nrows_p;
      sp = drow + (int64_t)(mtop + KS) * pitch_b;
#pragma unroll
      for (int s = 0; s < RING - 2; ++s) refill(s, true);
    }
#pragma unroll
    for (int s = RING - 2; s < RING; ++s)
#pragma unroll
      for (int v = 0; v < NV; ++v) Lb[s][v] = VT{};
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
    if constexpr (ROLE == 0) lk.publish(&lk.l->produced, base + nrows_p);
    else lk.publish(&lk.l->consumed, base + nrows_p);
  }
};

template <int K>
struct PipeCfg {
  static constexpr int K1 = (K + 1) / 2, K2 = K - K1;
  static constexpr int KA = (K + 3) / 4 * 4, W = 256, U = W - 2 * KA;
  static constexpr int RING_P = PP_RING_P, RING_C = 4;
};

// 256 threads = two pairs: waves 0 and 2 produce, waves 1 and 3 consume.
template <int K>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void pipe_kernel(const double* src,
                                                                                             double* dst, Args a) {
  using C = PipeCfg<K>;
  __shared__ PairLds lds[2];
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int role = w & 1;
  PairLds* l = &lds[w >> 1];
  (&l->produced)[lane & 3] = 0u;  // header words; both waves of the pair write the same zeros
  __syncthreads();                          // the only barrier: before any hand-over
  const int64_t pid = (int64_t)blockIdx.x * 2 + (w >> 1);
  Link lk{l, a.status, 0u, 0u};
  uint32_t base = 0;
  for (int64_t it = pid; it < a.nitems; it += a.nworkers) {
    const int64_t band = it / a.nunits, s = it - band * a.nunits;
    int64_t t0, t1;
    band_rows(a, band, t0, t1);
    const int64_t u0 = s * C::U, c0 = u0 - C::KA, ustop = min(u0 + (int64_t)C::U, a.ncols);
    const int64_t mycol = c0 + (int64_t)lane * 4;
    const bool in_alloc = mycol >= -a.cpad && mycol + 4 <= a.pitch - a.cpad;
    const int32_t off = in_alloc ? (int32_t)((mycol + a.cpad) * 8) : kOob;
    const pr::ItemRows ir = pr::item_rows((int32_t)(t1 - t0), C::K1, C::K2, C::RING_P, C::RING_C);
    if (role == 0) {
      PMarch<C::K1, 0, K, C::RING_P> m;
      m.lk = lk;
      m.srow = reinterpret_cast<const char*>(src - a.cpad);
      m.pitch_b = a.pitch * 8;
      m.nrec = (uint32_t)(a.pitch * 8);
      m.t0 = (int32_t)t0 - C::K2;  // level-K1 rows the consumer needs
      m.t1 = (int32_t)t1 + C::K2;
      m.ld_off = off;
      m.lds_lane = lane * 16;
      m.run(base, ir.fifo_rows, ir.bodies_p);
      lk = m.lk;
    } else {
      PMarch<C::K2, 1, K, C::RING_C> m;
      m.lk = lk;
      m.drow = reinterpret_cast<char*>(dst - a.cpad);
      m.pitch_b = a.pitch * 8;
      m.nrec = (uint32_t)(a.pitch * 8);
      m.t0 = (int32_t)t0;
      m.t1 = (int32_t)t1;
      m.st_off = (in_alloc && mycol >= u0 && mycol < ustop) ? off : kOob;
      m.lds_lane = lane * 16;
      m.run(base, ir.fifo_rows, ir.bodies_c);
      lk = m.lk;
    }
    base += ir.fifo_rows;
    if (lk.aborted) break;
  }
}

__global__ void fill_kernel(double* f, int64_t n, uint64_t seed) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    uint64_t x = (uint64_t)i * 0x9E3779B97F4A7C15ull + seed;
    x ^= x >> 31;
    x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 29;
    f[i] = 1.0 + (double)(x >> 11) * (1.0 / 9007199254740992.0);  // [1, 2)
  }
}

__global__ void compare_kernel(const double* a, const double* b, int64_t pitch, int64_t nrows, int64_t ncols,
                               unsigned long long* bad) {
  unsigned long long n = 0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nrows * ncols;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / ncols, c = i - r * ncols;
    const int64_t o = r * pitch + c;
    n += __double_as_longlong(a[o]) != __double_as_longlong(b[o]);
  }
  if (n) atomicAdd(bad, n);
}

template <int K>
int run(int64_t n) {
  using SC = StripCfg<K>;
  using PC = PipeCfg<K>;
  const int64_t halo = K + 8, cpad = 256, pitch = n + 2 * cpad;
  const int64_t rows_alloc = n + 2 * halo;
  const size_t bytes = (size_t)rows_alloc * pitch * 8;
  double *src, *dA, *dB;
  CK(hipMalloc(&src, bytes));
  CK(hipMalloc(&dA, bytes));
  CK(hipMalloc(&dB, bytes));
  uint32_t* status;
  unsigned long long* bad;
  CK(hipMalloc(&status, 4));
  CK(hipMemset(status, 0, 4));
  CK(hipMalloc(&bad, 8));
  const int64_t total = rows_alloc * pitch;
  hipLaunchKernelGGL(fill_kernel, dim3(4096), dim3(256), 0, 0, src, total, 12345ull);
  hipLaunchKernelGGL(fill_kernel, dim3(4096), dim3(256), 0, 0, dA, total, 777ull);
  hipLaunchKernelGGL(fill_kernel, dim3(4096), dim3(256), 0, 0, dB, total, 999ull);
  CK(hipDeviceSynchronize());
  const double* s0 = src + halo * pitch + cpad;  // (row 0, column 0)
  double* a0 = dA + halo * pitch + cpad;
  double* b0 = dB + halo * pitch + cpad;
  int dev = 0, ncu = 0;
  CK(hipGetDevice(&dev));
  CK(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev));
  const int64_t waves = (int64_t)ncu * 4 * 2;  // 2 waves per SIMD
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0));
  CK(hipEventCreate(&e1));
  auto status_now = [&] {
    uint32_t h = 0;
    CK(hipMemcpy(&h, status, 4, hipMemcpyDeviceToHost));
    return h;
  };
  auto timeit = [&](auto launch) {
    float best = 1e30f;
    for (int rep = 0; rep < 7; ++rep) {
      CK(hipEventRecord(e0, 0));
      launch();
      CK(hipEventRecord(e1, 0));
      CK(hipEventSynchronize(e1));
      float ms = 0.f;
      CK(hipEventElapsedTime(&ms, e0, e1));
      if (rep >= 2 && ms < best) best = ms;
    }
    return best;
  };
  const int64_t nstrips = (n + SC::U - 1) / SC::U, nwide = (n + PC::U - 1) / PC::U;
  std::printf("{\"n\": %lld, \"K\": %d, \"K1\": %d, \"K2\": %d, \"cus\": %d, \"fifo_rows\": %d, \"producer_ring\": %d, \"late_publish\": %d,\n",
              (long long)n, K, PC::K1, PC::K2, ncu, kDepth, PC::RING_P, PP_LATE);
  std::printf(" \"strip_useful_cols\": %d, \"pipe_useful_cols\": %d, \"strips\": %lld, \"wide_strips\": %lld, \"runs\": [\n",
              SC::U, PC::U, (long long)nstrips, (long long)nwide);
  // first a small pipe launch on its own: a wait that gives up ends the probe here
  {
    Args at{pitch, cpad, n, n, 1024, nwide, 8, 2, status};
    hipLaunchKernelGGL(pipe_kernel<K>, dim3(1), dim3(256), 0, 0, s0, b0, at);
    CK(hipDeviceSynchronize());
    if (status_now()) {
      std::printf("], \"error\": \"pipe wait timed out in the first launch\"}\n");
      return 4;
    }
  }
  float best_s = 1e30f, best_p = 1e30f;
  int64_t nb_s = 0, nb_p = 0;
  const int64_t bands[] = {6, 8, 11, 14, 19, 22, 27, 32};
  bool first = true;
  for (int64_t nb : bands) {
    Args as{pitch, cpad, n, n, nb, nstrips, nb * nstrips, std::min<int64_t>(waves, nb * nstrips), status};
    const unsigned gs = (unsigned)((as.nworkers + 1) / 2);
    const float ms_s = timeit([&] { hipLaunchKernelGGL(strip_kernel<K>, dim3(gs), dim3(128), 0, 0, s0, a0, as); });
    // pairs: half as many as waves, rounded down to whole workgroups of two
    const int64_t npairs = std::max<int64_t>(2, std::min<int64_t>(waves / 2, nb * nwide) / 2 * 2);
    Args ap{pitch, cpad, n, n, nb, nwide, nb * nwide, npairs, status};
    const float ms_p =
        timeit([&] { hipLaunchKernelGGL(pipe_kernel<K>, dim3((unsigned)(npairs / 2)), dim3(256), 0, 0, s0, b0, ap); });
    CK(hipGetLastError());
    const uint32_t st = status_now();
    std::printf("%s  {\"bands\": %lld, \"strip_ms\": %.4f, \"pipe_ms\": %.4f, \"status\": %u}", first ? "" : ",\n",
                (long long)nb, ms_s, ms_p, st);
    first = false;
    if (st) {
      std::printf("], \"error\": \"pipe wait timed out\"}\n");
      return 4;
    }
    if (ms_s < best_s) best_s = ms_s, nb_s = nb;
    if (ms_p < best_p) best_p = ms_p, nb_p = nb;
  }
  // bitwise check of the last launches (both wrote the whole n x n interior)
  CK(hipMemset(bad, 0, 8));
  hipLaunchKernelGGL(compare_kernel, dim3(4096), dim3(256), 0, 0, a0, b0, pitch, n, n, bad);
  unsigned long long hbad = 0;
  CK(hipMemcpy(&hbad, bad, 8, hipMemcpyDeviceToHost));
  const double pts = (double)n * n * K;
  std::printf("\n ],\n \"best_strip\": {\"bands\": %lld, \"ms\": %.4f, \"gpts\": %.1f},\n", (long long)nb_s, best_s,
              pts / best_s / 1e6);
  std::printf(" \"best_pipe\": {\"bands\": %lld, \"ms\": %.4f, \"gpts\": %.1f},\n", (long long)nb_p, best_p,
              pts / best_p / 1e6);
  std::printf(" \"pipe_over_strip\": %.4f, \"mismatches\": %llu}\n", best_s / best_p, hbad);
  CK(hipFree(bad));
  CK(hipFree(status));
  CK(hipFree(src));
  CK(hipFree(dA));
  CK(hipFree(dB));
  return hbad == 0 ? 0 : 3;
}
}  // namespace probe

int main(int argc, char** argv) {
  const int64_t n = argc > 1 ? std::atoll(argv[1]) : 32768;
  const int k = argc > 2 ? std::atoi(argv[2]) : 20;
  if (k == 20) return probe::run<20>(n);
  if (k == 24) return probe::run<24>(n);
  std::fprintf(stderr, "K must be 20 or 24\n");
  return 2;
}
