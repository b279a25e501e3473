// Index and wait arithmetic of the wave-pair row FIFO (tools/pipe_probe.hip):
// plain C++ shared by the device code and a host check
// (tests/host/pipe_ring_check.cpp, built with the host sanitizers).
//
// A pair hands rows over through a FIFO of `depth` rows (a power of two). Two
// 32-bit counters count rows monotonically over all the work items of a
// launch and may wrap: every comparison is on the signed difference, so it
// holds while the two sides are less than 2^31 rows apart.
//
// Rows of one work item (output rows [t0, t1), depths K1 + K2, march bodies
// of lp (producer) and lc (consumer) rows):
//   * the consumer marches nc = roundup(t1 - t0 + 2 K2, lc) rows and reads
//     lc - 2 rows ahead: nc + lc - 2 FIFO rows;
//   * the producer's first 2 K1 rows only prime its levels: the consumer
//     skips them (it releases them unread);
//   * the producer marches fifo_rows = roundup(2 K1 + nc + lc - 2, lp) rows,
//     one FIFO row each, and both waves advance their base by fifo_rows.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define HEAT2D_PIPE_HD __host__ __device__ __forceinline__
#else
#define HEAT2D_PIPE_HD inline
#endif

namespace heat2d {
namespace kern {
namespace pipe {

// counter value `have` has reached `need` (wrap-safe)
HEAT2D_PIPE_HD bool reached(uint32_t have, uint32_t need) { return (int32_t)(have - need) >= 0; }

// FIFO slot of row `idx`
HEAT2D_PIPE_HD uint32_t slot(uint32_t idx, uint32_t depth) { return idx & (depth - 1u); }

// The producer may write row q once `consumed` has reached this value: rows
// q - depth and older are released, so the slot is free.
HEAT2D_PIPE_HD uint32_t write_need(uint32_t q, uint32_t depth) { return q + 1u - depth; }

// The consumer may read row q once `produced` has reached this value; a read
// at or past the item's last row (qend) never waits for more than the item has.
HEAT2D_PIPE_HD uint32_t read_need(uint32_t q, uint32_t qend) { return reached(q + 1u, qend) ? qend : q + 1u; }

// rows at the head of an item the consumer releases unread
HEAT2D_PIPE_HD uint32_t skip_rows(int k1) { return 2u * (uint32_t)k1; }

// a wait that began at t_start has run out at `now` (free-running clock; wrap-safe)
HEAT2D_PIPE_HD bool timed_out(uint64_t t_start, uint64_t now, uint64_t limit) { return now - t_start > limit; }

struct ItemRows {
  int32_t bodies_p, bodies_c;  // march loop bodies of the producer / consumer
  uint32_t fifo_rows;          // FIFO rows of the item (= producer march rows)
};

HEAT2D_PIPE_HD ItemRows item_rows(int32_t out_rows, int k1, int k2, int lp, int lc) {
  ItemRows r;
  r.bodies_c = (out_rows + 2 * k2 + lc - 1) / lc;
  const int32_t need = 2 * k1 + r.bodies_c * lc + (lc - 2);
  r.bodies_p = (need + lp - 1) / lp;
  r.fifo_rows = (uint32_t)(r.bodies_p * lp);
  return r;
}

}  // namespace pipe
}  // namespace kern
}  // namespace heat2d
