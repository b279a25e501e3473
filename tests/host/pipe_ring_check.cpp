// Stand-alone host check of the wave-pair FIFO's index and wait arithmetic
// (csrc/kernels/pipe_ring.hpp), built with AddressSanitizer and
// UndefinedBehaviorSanitizer by tests/test_pipe_ring.py. It replays the two
// waves' protocol on the host, in every interleaving a bounded scheduler
// produces, with the counters starting anywhere (also just below 2^32):
//   * a slot is never written before its previous row was released, and never
//     read before it was published (checked on a shadow ring);
//   * neither side ever needs more than the other can deliver (no deadlock),
//     for every item shape, across several items back to back;
//   * the wait bound trips only past its limit, also across a clock wrap.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "pipe_ring.hpp"

namespace pr = heat2d::kern::pipe;

#define CHECK(c)                                                         \
  do {                                                                   \
    if (!(c)) {                                                          \
      std::fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #c); \
      std::exit(1);                                                      \
    }                                                                    \
  } while (0)

struct Sim {
  uint32_t depth;
  uint32_t produced, consumed;  // the LDS counters
  std::vector<uint32_t> ring;   // shadow: the row index a slot holds
  std::vector<char> full;       // shadow: written and not yet released
};

// One pair marching `items` items of out_rows[i] rows; `sched` picks which
// wave moves next (bit i of a xorshift stream). Returns the rows handed over.
static uint64_t run_pair(uint32_t start, uint32_t depth, int k1, int k2, int lp, int lc,
                         const std::vector<int32_t>& out_rows, uint64_t seed) {
  Sim s{depth, start, start, std::vector<uint32_t>(depth, 0), std::vector<char>(depth, 0)};
  uint64_t handed = 0;
  // producer state
  size_t pi = 0;
  uint32_t pbase = start, pq = start, pend = 0;
  bool pstarted = false;
  // consumer state
  size_t ci = 0;
  uint32_t cbase = start, cq = 0, cend = 0, creads = 0, cneed_reads = 0;
  bool cstarted = false;
  uint64_t x = seed | 1, stall = 0;
  while (pi < out_rows.size() || ci < out_rows.size()) {
    x ^= x << 13, x ^= x >> 7, x ^= x << 17;
    bool moved = false;
    if ((x & 1) && pi < out_rows.size()) {  // producer's turn
      const pr::ItemRows ir = pr::item_rows(out_rows[pi], k1, k2, lp, lc);
      if (!pstarted) {
        pq = pbase;
        pend = pbase + ir.fifo_rows;
        pstarted = true;
      }
      if (pq != pend) {
        s.produced = pq;  // publish the rows written so far (top of the march row)
        if (pr::reached(s.consumed, pr::write_need(pq, depth))) {
          const uint32_t sl = pr::slot(pq, depth);
          CHECK(sl < depth);
          // the slot's previous row must have been released
          CHECK(!s.full[sl] || pr::reached(s.consumed, s.ring[sl] + 1u));
          s.ring[sl] = pq;
          s.full[sl] = 1;
          ++pq;
          moved = true;
        }
      } else {
        s.produced = pend;  // end of item
        pbase = pend;
        pstarted = false;
        ++pi;
        moved = true;
      }
    } else if (ci < out_rows.size()) {  // consumer's turn
      const pr::ItemRows ir = pr::item_rows(out_rows[ci], k1, k2, lp, lc);
      if (!cstarted) {
        cq = cbase + pr::skip_rows(k1);
        cend = cbase + ir.fifo_rows;
        creads = 0;
        cneed_reads = (uint32_t)(ir.bodies_c * lc + lc - 2);
        CHECK(pr::reached(cend, cq + cneed_reads));  // every read lies inside the item
        cstarted = true;
      }
      if (creads < cneed_reads) {
        s.consumed = cq;  // release the rows read so far
        const uint32_t need = pr::read_need(cq, cend);
        CHECK(pr::reached(cend, need));  // never waits for more than the item has
        if (pr::reached(s.produced, need)) {
          const uint32_t sl = pr::slot(cq, depth);
          CHECK(s.full[sl] && s.ring[sl] == cq);  // published, and not overwritten
          ++cq;
          ++creads;
          ++handed;
          moved = true;
        }
      } else {
        s.consumed = cend;  // end of item
        cbase = cend;
        cstarted = false;
        ++ci;
        moved = true;
      }
    }
    stall = moved ? 0 : stall + 1;
    CHECK(stall < 1000);  // both sides blocked: a deadlock
  }
  CHECK(s.produced == s.consumed);
  return handed;
}

int main() {
  // counters and wrap
  CHECK(pr::reached(5u, 5u) && pr::reached(6u, 5u) && !pr::reached(4u, 5u));
  CHECK(pr::reached(3u, 0xfffffffeu) && !pr::reached(0xfffffffeu, 3u));  // across 2^32
  CHECK(pr::write_need(0u, 8u) == 0xfffffff9u && pr::reached(0u, pr::write_need(0u, 8u)));
  CHECK(pr::read_need(7u, 100u) == 8u && pr::read_need(99u, 100u) == 100u && pr::read_need(100u, 100u) == 100u);
  CHECK(pr::read_need(0xffffffffu, 5u) == 0u);  // q + 1 wraps to 0, still before the item's end
  for (uint32_t d : {2u, 4u, 8u, 16u})
    for (uint32_t i : {0u, 1u, d - 1u, d, 0xffffffffu, 0x80000000u}) CHECK(pr::slot(i, d) == i % d);
  // the wait bound
  CHECK(!pr::timed_out(100, 100, 50) && !pr::timed_out(100, 150, 50) && pr::timed_out(100, 151, 50));
  CHECK(!pr::timed_out(~0ull - 10, 5, 50) && pr::timed_out(~0ull - 10, 45, 50));  // clock wrap
  // item shapes: every depth split the kernel is built for, thin and tall items
  for (int k = 16; k <= 24; ++k) {
    const int k1 = (k + 1) / 2, k2 = k - k1;
    for (int32_t rows : {1, 2, 3, 7, 40, 81, 1213}) {
      const pr::ItemRows ir = pr::item_rows(rows, k1, k2, 4, 4);
      CHECK(ir.bodies_c * 4 >= rows + 2 * k2);
      CHECK(ir.fifo_rows == (uint32_t)ir.bodies_p * 4u);
      CHECK(ir.fifo_rows >= (uint32_t)(2 * k1 + ir.bodies_c * 4 + 2));
      CHECK(ir.fifo_rows > 8u);  // longer than the FIFO: the 2-slot item mailbox is safe
    }
  }
  // the protocol, many interleavings, counters starting near the wrap too
  uint64_t total = 0;
  for (uint32_t start : {0u, 0xffffff00u, 0xfffffffdu, 0x7ffffff0u})
    for (uint32_t depth : {2u, 8u})
      for (uint64_t seed = 1; seed <= 40; ++seed)
        total += run_pair(start, depth, 10, 10, 4, 4, {1, 40, 3, 123, 40, 1, 1}, seed * 0x9E3779B97F4A7C15ull);
  for (uint64_t seed = 1; seed <= 10; ++seed) {
    total += run_pair(0xffffffe0u, 8, 12, 12, 4, 4, {80, 5, 200}, seed);
    total += run_pair(17, 8, 10, 9, 6, 4, {33, 64, 2}, seed);  // K1 != K2, producer bodies of 6
  }
  std::printf("pipe_ring_check ok: %llu rows handed over\n", (unsigned long long)total);
  return 0;
}
