// CPU twins of the device kernels. They implement the same operations on the
// same SlabLayout with the same arithmetic order (built with
// -ffp-contract=off), so CPU, GPU, blocked and unblocked runs agree bitwise.
// This is also the native serial solver path that replaces
// fortran/serial/heat.f90 (whose k-inner loop over the strided index,
// :64-66, is cache-hostile; here the inner loop is the contiguous one).
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>
#include <thread>
#include <type_traits>
#include <vector>

#include "heat2d/probe.hpp"
#include "heat2d/runtime.hpp"

namespace heat2d {
namespace cpu {
namespace {

// Rows [begin, end) split over host threads; `row_cost` = elements per row.
// Below ~1M elements per call one thread is faster than spawning several
// (the 256^2 serial config runs ~3x faster that way).
template <typename F>
void parallel_rows(int64_t begin, int64_t end, F&& f, int64_t row_cost = 1 << 14) {
  const int64_t n = end - begin;
  if (n <= 0) return;
  int nt = num_threads();
  if (n < 64 || nt <= 1 || n * row_cost < (int64_t(1) << 20)) {
    f(begin, end);
    return;
  }
  nt = (int)std::min<int64_t>(nt, n / 32 > 0 ? n / 32 : 1);
  std::vector<std::thread> th;
  th.reserve(nt);
  const int64_t chunk = (n + nt - 1) / nt;
  for (int t = 0; t < nt; ++t) {
    const int64_t b = begin + t * chunk, e = std::min(end, b + chunk);
    if (b >= e) break;
    th.emplace_back([=, &f] { f(b, e); });
  }
  for (auto& x : th) x.join();
}

// One row of the FTCS update in the reference order
// T(x+1,y) + T(x,y+1) + T(x-1,y) + T(x,y-1) - 4*T(x,y), then C + r*(...) or
// its contracted form (the device kernel's arith 1, tb_impl.hpp). The fma form
// has a copy compiled for hosts with FMA3 (std::fma otherwise is a libm call
// per point: ~4x slower on the 256^2 serial config).
template <typename T>
void row_exact(const T* up, const T* mid, const T* dn, T* out, int64_t n, T r) {
  for (int64_t j = 0; j < n; ++j) {
    const T sum = ((dn[j] + mid[j + 1]) + up[j]) + mid[j - 1];
    out[j] = mid[j] + r * (sum - T(4) * mid[j]);
  }
}
template <typename T>
__attribute__((target("fma"))) void row_fma_hw(const T* up, const T* mid, const T* dn, T* out, int64_t n, T r) {
  for (int64_t j = 0; j < n; ++j) {
    const T sum = ((dn[j] + mid[j + 1]) + up[j]) + mid[j - 1];
    out[j] = std::fma(r, sum - T(4) * mid[j], mid[j]);
  }
}
template <typename T>
void row_fma_sw(const T* up, const T* mid, const T* dn, T* out, int64_t n, T r) {
  for (int64_t j = 0; j < n; ++j) {
    const T sum = ((dn[j] + mid[j + 1]) + up[j]) + mid[j - 1];
    out[j] = std::fma(r, sum - T(4) * mid[j], mid[j]);
  }
}
// ... with a diffusivity map: the multiplier is the map's element rm[j]
template <typename T>
void row_var_exact(const T* up, const T* mid, const T* dn, T* out, int64_t n, const T* rm) {
  for (int64_t j = 0; j < n; ++j) {
    const T sum = ((dn[j] + mid[j + 1]) + up[j]) + mid[j - 1];
    out[j] = mid[j] + rm[j] * (sum - T(4) * mid[j]);
  }
}
template <typename T>
__attribute__((target("fma"))) void row_var_fma_hw(const T* up, const T* mid, const T* dn, T* out, int64_t n, const T* rm) {
  for (int64_t j = 0; j < n; ++j) {
    const T sum = ((dn[j] + mid[j + 1]) + up[j]) + mid[j - 1];
    out[j] = std::fma(rm[j], std::fma(T(-4), mid[j], sum), mid[j]);
  }
}
template <typename T>
void row_var_fma_sw(const T* up, const T* mid, const T* dn, T* out, int64_t n, const T* rm) {
  for (int64_t j = 0; j < n; ++j) {
    const T sum = ((dn[j] + mid[j + 1]) + up[j]) + mid[j - 1];
    out[j] = std::fma(rm[j], std::fma(T(-4), mid[j], sum), mid[j]);
  }
}
// ... the conservative form from per-face diffusion numbers: xe = RX[row] (xe[j - 1] the west
// face), ys = RY[row], yn = RY[row - 1]; operands in the march's order S, E, N, W
template <typename T>
void row_div_exact(const T* up, const T* mid, const T* dn, T* out, int64_t n, const T* xe, const T* ys, const T* yn) {
  for (int64_t j = 0; j < n; ++j) {
    const T c = mid[j];
    const T flux = ((ys[j] * (dn[j] - c) + xe[j] * (mid[j + 1] - c)) + yn[j] * (up[j] - c)) + xe[j - 1] * (mid[j - 1] - c);
    out[j] = c + flux;
  }
}
template <typename T>
__attribute__((target("fma"))) void row_div_fma_hw(const T* up, const T* mid, const T* dn, T* out, int64_t n, const T* xe,
                                                   const T* ys, const T* yn) {
  for (int64_t j = 0; j < n; ++j) {
    const T c = mid[j];
    T p = ys[j] * (dn[j] - c);
    p = std::fma(xe[j], mid[j + 1] - c, p);
    p = std::fma(yn[j], up[j] - c, p);
    p = std::fma(xe[j - 1], mid[j - 1] - c, p);
    out[j] = c + p;
  }
}
template <typename T>
void row_div_fma_sw(const T* up, const T* mid, const T* dn, T* out, int64_t n, const T* xe, const T* ys, const T* yn) {
  for (int64_t j = 0; j < n; ++j) {
    const T c = mid[j];
    T p = ys[j] * (dn[j] - c);
    p = std::fma(xe[j], mid[j + 1] - c, p);
    p = std::fma(yn[j], up[j] - c, p);
    p = std::fma(xe[j - 1], mid[j - 1] - c, p);
    out[j] = c + p;
  }
}
// ... the five-weight operator, w = (wS, wE, wN, wW, wC): every product and sum rounded, in the
// march's order S, E, N, W and last C; arith 1: the first product, then four fmas
template <typename T>
void row_w5_exact(const T* up, const T* mid, const T* dn, T* out, int64_t n, const T* w) {
  for (int64_t j = 0; j < n; ++j)
    out[j] = (((w[0] * dn[j] + w[1] * mid[j + 1]) + w[2] * up[j]) + w[3] * mid[j - 1]) + w[4] * mid[j];
}
template <typename T>
__attribute__((target("fma"))) void row_w5_fma_hw(const T* up, const T* mid, const T* dn, T* out, int64_t n, const T* w) {
  for (int64_t j = 0; j < n; ++j) {
    T p = w[0] * dn[j];
    p = std::fma(w[1], mid[j + 1], p);
    p = std::fma(w[2], up[j], p);
    p = std::fma(w[3], mid[j - 1], p);
    out[j] = std::fma(w[4], mid[j], p);
  }
}
template <typename T>
void row_w5_fma_sw(const T* up, const T* mid, const T* dn, T* out, int64_t n, const T* w) {
  for (int64_t j = 0; j < n; ++j) {
    T p = w[0] * dn[j];
    p = std::fma(w[1], mid[j + 1], p);
    p = std::fma(w[2], up[j], p);
    p = std::fma(w[3], mid[j - 1], p);
    out[j] = std::fma(w[4], mid[j], p);
  }
}
// arith 2 (r == 1/4): the centre weight 1 - 4r is zero, r * sum (r*x exact)
template <typename T>
void row_jacobi(const T* up, const T* mid, const T* dn, T* out, int64_t n, T r) {
  for (int64_t j = 0; j < n; ++j) out[j] = r * (((dn[j] + mid[j + 1]) + up[j]) + mid[j - 1]);
}
bool host_has_fma() {
  static const bool v = __builtin_cpu_supports("fma");
  return v;
}

template <typename T>
void wrap_cols_impl(T* f, const SlabLayout& L, int64_t r0, int64_t r1) {
  for (int64_t i = r0; i < r1; ++i) {
    T* row = f + L.offset(i, 0);
    for (int64_t j = 0; j < kern::kWrapCols; ++j) {
      row[-1 - j] = row[L.ncols - 1 - j];
      row[L.ncols + j] = row[j];
    }
  }
}

template <typename T>
void ins_cols_impl(T* f, const SlabLayout& L, int64_t r0, int64_t r1) {
  for (int64_t i = r0; i < r1; ++i) {
    T* row = f + L.offset(i, 0);
    row[-1] = row[0];
    row[L.ncols] = row[L.ncols - 1];
  }
}

// The ghost value beyond a Robin wall (the device march's tb_impl.hpp rob_ghost): a * c + b, the
// product rounded, then the add (this file is built with -ffp-contract=off); arith 1: one fma.
template <typename T>
inline T rob_ghost(T a, T c, T b, int arith) {
  return arith == 1 ? kern::probe_fma(a, c, b) : a * c + b;
}
template <typename T>
void rob_cols_impl(T* f, const SlabLayout& L, int64_t r0, int64_t r1, const double* p, int arith) {
  for (int64_t i = r0; i < r1; ++i) {
    T* row = f + L.offset(i, 0);
    row[-1] = rob_ghost((T)p[0], row[0], (T)p[1], arith);
    row[L.ncols] = rob_ghost((T)p[2], row[L.ncols - 1], (T)p[3], arith);
  }
}
template <typename T>
void rob_row_impl(T* dst, const T* src, int64_t n, T a, T b, int arith) {
  for (int64_t j = 0; j < n; ++j) dst[j] = rob_ghost(a, src[j], b, arith);
}

// bc (kernels.hpp kBcPeriodicX / kBcPeriodicY), as the device march: periodic
// x pins no row, periodic y pins no column — level s is computed over the
// ghost columns [-(k - s), ncols + (k - s)) too, from level-0 wrap images k
// columns deep, and the ghost columns of the rows written are refreshed.
// kBcInsulatedX / kBcInsulatedY: at a point next to an insulated wall the
// operand from beyond the wall is the point's own value, at every level (the
// device march's substitution, tb_impl.hpp March INS) — here by giving the
// frame entry beside it that value before each level reads it; the frame
// images of the rows written are refreshed.
// kBcRobinX / kBcRobinY (rob: the walls' pairs, kernels.hpp): the same with
// the ghost value a * C + b in place of the point's own value (the device
// march's tb_impl.hpp March ROB), formed from each level's own C; an insulated
// axis beside a Robin one is the pair (1, -0.0). The frame of the rows written
// gets the ghost values, the wall rows first, then the columns over them.
// q (a heat source in the field's layout, Dirichlet axes only): every level adds
// its row of q to the updated owned points, T' = update + q, as an add of its
// own (the device march's tb_impl.hpp March SRC); pinned points are copied.
// gn (with q: the gains of the pass, gn[s - 1] for level s): level s adds
// gn[s - 1] * q — the product rounded, then the add; arith 1: one fma — the
// device march's tb_impl.hpp March GAIN.
// w5 (the five weights, Dirichlet or periodic axes): an owned point's update is the weighted
// sum of its five operands (the device march's tb_impl.hpp March W5); pinned points are copied.
// rm (a diffusivity map in the field's layout, Dirichlet axes only): the
// multiplier of an owned point's update is its element of rm instead of r (the
// device march's tb_impl.hpp March VAR); pinned points are copied.
// fx, fy (per-face diffusion numbers in the field's layout, Dirichlet axes only):
// the conservative form, an owned point's flux from its four faces (the device
// march's tb_impl.hpp March DIV); pinned points are copied.
template <typename T>
void tb_impl(const T* src, T* dst, const SlabLayout& L0, int64_t rb, int64_t re, int k, T r, int arith, int bc,
             const T* q = nullptr, const T* rm = nullptr, const T* fx = nullptr, const T* fy = nullptr,
             const T* gn = nullptr, const double* rob = nullptr, const double* w5 = nullptr) {
  const SlabLayout L = kern::bc_layout(L0, bc & kern::kBcPeriodicX);  // (the columns: free_cols below)
  const bool free_cols = (bc & kern::kBcPeriodicY) != 0;
  const bool robin = (bc & kern::kBcRobin) != 0;
  // (with a Robin axis the insulated walls run as Robin ones with (1, -0.0): wall_x / wall_y below)
  const bool ins_x = !robin && (bc & kern::kBcInsulatedX), ins_y = !robin && (bc & kern::kBcInsulatedY);
  const bool wall_x = robin && (bc & kern::kBcWallX), wall_y = robin && (bc & kern::kBcWallY);
  HEAT2D_REQUIRE(!((bc & kern::kBcWallX) && (bc & kern::kBcPeriodicX)) && !((bc & kern::kBcWallY) && free_cols),
                 "an axis is periodic or insulated, not both");
  HEAT2D_REQUIRE(!((bc & kern::kBcRobinX) && (bc & kern::kBcInsulatedX)) && !((bc & kern::kBcRobinY) && (bc & kern::kBcInsulatedY)),
                 "an axis is Robin or insulated, not both");
  double px[4] = {1.0, -0.0, 1.0, -0.0}, py[4] = {1.0, -0.0, 1.0, -0.0};
  if (robin) {
    HEAT2D_REQUIRE(rob && (arith == 0 || arith == 1), "Robin walls need their pairs and arith 0 (exact) or 1 (fma)");
    kern::wall_pairs(bc, true, rob, px);
    kern::wall_pairs(bc, false, rob, py);
  }
  if (free_cols) HEAT2D_REQUIRE(L.ncols >= kern::kWrapCols, "periodic y needs at least kWrapCols (24) owned columns");
  const int64_t R = re - rb + 2 * k;  // level-0 rows [rb-k, re+k)
  const int64_t P = L.pitch;
  std::vector<T> A((size_t)(R * P)), B((size_t)(R * P));
  std::memcpy(A.data(), src + L.offset(rb - k, -L.cpad), sizeof(T) * (size_t)(R * P));
  std::memcpy(B.data(), A.data(), sizeof(T) * (size_t)(R * P));
  const int64_t fixed_lo = -L.row0, fixed_hi = L.nrows_global - L.row0;
  const int64_t c = L.cpad;
  T* a = A.data();
  T* b = B.data();
  const T wt[5] = {w5 ? (T)w5[0] : T(0), w5 ? (T)w5[1] : T(0), w5 ? (T)w5[2] : T(0), w5 ? (T)w5[3] : T(0),
                   w5 ? (T)w5[4] : T(0)};
  auto* row_update = arith == 2   ? &row_jacobi<T>
                     : arith == 1 ? (host_has_fma() ? &row_fma_hw<T> : &row_fma_sw<T>)
                                  : &row_exact<T>;
  for (int s = 1; s <= k; ++s) {
    // insulated walls: level s - 1 rows [s - 1, R - s + 1) are read
    if (ins_y)
      for (int64_t li = s - 1; li < R - s + 1; ++li) {
        a[li * P + c - 1] = a[li * P + c];
        a[li * P + c + L.ncols] = a[li * P + c + L.ncols - 1];
      }
    if (ins_x)  // (after the columns; whole padded rows: periodic y's ghost columns too)
      for (const int64_t w : {fixed_lo - 1, fixed_hi}) {
        const int64_t li = w - (rb - k), from = w < fixed_lo ? li + 1 : li - 1;
        if (li >= s - 1 && li < R - s + 1 && from >= 0 && from < R) std::memcpy(a + li * P, a + from * P, sizeof(T) * (size_t)P);
      }
    // Robin walls: the ghost values of level s - 1, from its own values (no owned point reads a corner entry)
    if (wall_y)
      for (int64_t li = s - 1; li < R - s + 1; ++li) {
        a[li * P + c - 1] = rob_ghost((T)py[0], a[li * P + c], (T)py[1], arith);
        a[li * P + c + L.ncols] = rob_ghost((T)py[2], a[li * P + c + L.ncols - 1], (T)py[3], arith);
      }
    if (wall_x)  // (whole padded rows: periodic y's ghost columns too)
      for (const int64_t w : {fixed_lo - 1, fixed_hi}) {
        const bool lo = w < fixed_lo;
        const int64_t li = w - (rb - k), from = lo ? li + 1 : li - 1;
        if (li >= s - 1 && li < R - s + 1 && from >= 0 && from < R)
          rob_row_impl(a + li * P, a + from * P, P, (T)px[lo ? 0 : 2], (T)px[lo ? 1 : 3], arith);
      }
    parallel_rows(s, R - s, [&](int64_t lb, int64_t le) {
      for (int64_t li = lb; li < le; ++li) {
        const int64_t row = rb - k + li;  // local slab row
        const int64_t g = free_cols ? k - s : 0;  // ghost columns this level still needs
        const T* up = a + (li - 1) * P + c - g;
        const T* mid = a + li * P + c - g;
        const T* dn = a + (li + 1) * P + c - g;
        T* out = b + li * P + c - g;
        if (row < fixed_lo || row >= fixed_hi) {
          std::memcpy(out, mid, sizeof(T) * (size_t)(L.ncols + 2 * g));
          continue;
        }
        if (w5) {
          if (arith == 1) (host_has_fma() ? row_w5_fma_hw<T> : row_w5_fma_sw<T>)(up, mid, dn, out, L.ncols + 2 * g, wt);
          else row_w5_exact<T>(up, mid, dn, out, L.ncols + 2 * g, wt);
          continue;
        }
        if (fx) {
          const T *xe = fx + L.offset(row, 0), *ys = fy + L.offset(row, 0), *yn = fy + L.offset(row - 1, 0);
          if (arith == 1) (host_has_fma() ? row_div_fma_hw<T> : row_div_fma_sw<T>)(up, mid, dn, out, L.ncols, xe, ys, yn);
          else row_div_exact<T>(up, mid, dn, out, L.ncols, xe, ys, yn);
          continue;
        }
        if (rm) {
          const T* rr = rm + L.offset(row, 0);
          if (arith == 1) (host_has_fma() ? row_var_fma_hw<T> : row_var_fma_sw<T>)(up, mid, dn, out, L.ncols, rr);
          else row_var_exact<T>(up, mid, dn, out, L.ncols, rr);
          continue;
        }
        row_update(up, mid, dn, out, L.ncols + 2 * g, r);
        if (q) {
          const T* qr = q + L.offset(row, 0);
          if (gn) {
            const T gs = gn[s - 1];
            if (arith == 1)
              for (int64_t j = 0; j < L.ncols; ++j) out[j] = kern::probe_fma(gs, qr[j], out[j]);
            else
              for (int64_t j = 0; j < L.ncols; ++j) out[j] = out[j] + gs * qr[j];
          } else {
            for (int64_t j = 0; j < L.ncols; ++j) out[j] = out[j] + qr[j];
          }
        }
      }
    }, L.ncols);
    std::swap(a, b);
  }
  for (int64_t i = rb; i < re; ++i)
    std::memcpy(dst + L.offset(i, 0), a + (i - rb + k) * P + c, sizeof(T) * (size_t)L.ncols);
  if (free_cols) wrap_cols_impl(dst, L, rb, re);
  if (ins_y) ins_cols_impl(dst, L, rb, re);
  if (robin) {  // the golden's order: the wall rows (whole padded rows), then the columns over them
    const bool tlo = wall_x && L.row0 == 0 && rb <= 0 && re > 0;
    const bool thi = wall_x && L.row0 + L.nrows == L.nrows_global && rb < L.nrows && re >= L.nrows;
    if (tlo) rob_row_impl(dst + L.offset(-1, -L.cpad), dst + L.offset(0, -L.cpad), P, (T)px[0], (T)px[1], arith);
    if (thi) rob_row_impl(dst + L.offset(L.nrows, -L.cpad), dst + L.offset(L.nrows - 1, -L.cpad), P, (T)px[2], (T)px[3], arith);
    if (wall_y) rob_cols_impl(dst, L, rb - (tlo ? 1 : 0), re + (thi ? 1 : 0), py, arith);
  }
  if (ins_x) {
    const size_t rowb = sizeof(T) * (size_t)P;
    if (L.row0 == 0 && rb <= 0 && re > 0) std::memcpy(dst + L.offset(-1, -L.cpad), dst + L.offset(0, -L.cpad), rowb);
    if (L.row0 + L.nrows == L.nrows_global && rb < L.nrows && re >= L.nrows)
      std::memcpy(dst + L.offset(L.nrows, -L.cpad), dst + L.offset(L.nrows - 1, -L.cpad), rowb);
  }
}

template <typename T>
void init_impl(T* f, const SlabLayout& L, const kern::IcParams& ic, const double* xc, const double* yc) {
  parallel_rows(0, L.rows_alloc(), [&](int64_t b, int64_t e) {
    for (int64_t ia = b; ia < e; ++ia) {
      const int64_t i = ia - L.halo;
      const int64_t g = L.row0 + i;
      for (int64_t ja = 0; ja < L.pitch; ++ja) {
        const int64_t j = ja - L.cpad;
        double v;
        const bool in_frame = g >= -1 && g <= L.nrows_global && j >= -1 && j <= L.ncols;
        if (!in_frame) {
          v = ic.pad;
        } else {
          const bool frame = g < 0 || g >= L.nrows_global || j < 0 || j >= L.ncols;
          const double x = xc[g + 1], y = yc[j + 1];
          switch ((kern::IcKind)ic.kind) {
            case kern::IcKind::Uniform:
              v = frame ? ic.b : ic.a;
              break;
            case kern::IcKind::Box:
              v = (x <= ic.x1 && x >= ic.x0 && y <= ic.y1 && y >= ic.y0) ? ic.a : ic.b;
              break;
            case kern::IcKind::IndexBox: {
              const int64_t gi = g + 1, gj = j + 1;
              v = (gi >= ic.i0 && gi < ic.i1 && gj >= ic.j0 && gj < ic.j1) ? ic.a : ic.b;
              break;
            }
            case kern::IcKind::Sine:
              v = frame ? 0.0
                        : ic.a * std::sin(ic.kx * M_PI * (x - ic.x0) / (ic.x1 - ic.x0)) *
                              std::sin(ic.ky * M_PI * (y - ic.y0) / (ic.y1 - ic.y0));
              break;
            default:
              v = ic.a;
          }
        }
        f[ia * L.pitch + ja] = (T)v;
      }
    }
  });
}

template <typename T>
void stats_impl(const T* f, const T* o, const SlabLayout& L, double out[6]) {
  double s = 0, ss = 0, mn = DBL_MAX, mx = -DBL_MAX, dd = 0, md = 0;
  for (int64_t i = 0; i < L.nrows; ++i) {
    const T* row = f + L.offset(i, 0);
    const T* orow = o ? o + L.offset(i, 0) : nullptr;
    for (int64_t j = 0; j < L.ncols; ++j) {
      const double v = (double)row[j];
      s += v;
      ss += v * v;
      mn = std::fmin(mn, v);
      mx = std::fmax(mx, v);
      if (orow) {
        const double d = v - (double)orow[j];
        dd += d * d;
        md = std::fmax(md, std::fabs(d));
      }
    }
  }
  out[0] = s; out[1] = ss; out[2] = mn; out[3] = mx; out[4] = dd; out[5] = md;
}

}  // namespace

int num_threads() {
  static int n = [] {
    const char* e = std::getenv("HEAT2D_CPU_THREADS");
    int v = e ? std::atoi(e) : (int)std::thread::hardware_concurrency();
    return std::max(1, std::min(v, 64));
  }();
  return n;
}

void tb(DType dt, const void* src, void* dst, const SlabLayout& L, int64_t row_begin, int64_t row_end,
        int k, double r, const kern::TbTerms& terms) {
  int arith = terms.arith;
  const int bc = terms.bc;
  const void *source = terms.source, *rmap = terms.rmap, *rx = terms.rx, *ry = terms.ry;
  const kern::GainRef gain = terms.gain;
  const double *robin = terms.robin, *weights = terms.weights;
  HEAT2D_REQUIRE(k >= 1 && k <= L.halo, "k out of range");
  HEAT2D_REQUIRE(arith >= 0 && arith <= 3, "arith must be 0, 1, 2 or 3");
  HEAT2D_REQUIRE(arith != 2 || r == 0.25, "arith 2 (jacobi) needs r == 1/4 exactly");
  // arith 3 (the device kernels' scaled levels, tb_impl.hpp) is not bitwise
  // reproducible across launch plans; the CPU twin runs its unscaled
  // contracted form (arith 1), within the same stated bound of exact
  HEAT2D_REQUIRE(arith != 3 || !(bc & (kern::kBcInsulatedX | kern::kBcInsulatedY)),
                 "insulated boundaries have no arith 3 (fast) kernels");
  HEAT2D_REQUIRE(!(bc & kern::kBcRobin) || (robin && (arith == 0 || arith == 1)),
                 "Robin walls need their pairs and arith 0 (exact) or 1 (fma)");
  HEAT2D_REQUIRE(!source || ((arith == 0 || arith == 1) && bc == 0),
                 "a heat source needs arith 0 (exact) or 1 (fma) and Dirichlet boundaries on both axes");
  HEAT2D_REQUIRE(!rmap || ((arith == 0 || arith == 1) && bc == 0 && !source),
                 "a diffusivity map needs arith 0 (exact) or 1 (fma), Dirichlet boundaries on both axes and no heat source");
  HEAT2D_REQUIRE((rx != nullptr) == (ry != nullptr), "face coefficients need both buffers (rx and ry)");
  HEAT2D_REQUIRE(!rx || ((arith == 0 || arith == 1) && bc == 0 && !source && !rmap),
                 "face coefficients need arith 0 (exact) or 1 (fma), Dirichlet boundaries on both axes, no heat source and "
                 "no diffusivity map");
  HEAT2D_REQUIRE(!gain.g || (source && gain.pos), "a gain schedule needs a heat source and its position word");
  if (weights) {
    HEAT2D_REQUIRE(arith == 0 || arith == 1, "weights need arith 0 (exact) or 1 (fma)");
    HEAT2D_REQUIRE(!source && !rmap && !rx && !gain.g, "weights go with no heat source, diffusivity map, face coefficients or gain schedule");
    HEAT2D_REQUIRE(!(bc & (kern::kBcWallX | kern::kBcWallY)), "weights need Dirichlet or periodic axes: no insulated or Robin walls");
    for (int i = 0; i < 5; ++i) HEAT2D_REQUIRE(std::isfinite(weights[i]), "weights must be finite");
  }
  if (arith == 3) arith = 1;
  if (row_end <= row_begin) return;
  const int64_t gpos = gain.g ? *gain.pos : 0;
  if (dt == DType::F32)
    tb_impl<float>(static_cast<const float*>(src), static_cast<float*>(dst), L, row_begin, row_end, k, (float)r, arith, bc,
                   static_cast<const float*>(source), static_cast<const float*>(rmap), static_cast<const float*>(rx),
                   static_cast<const float*>(ry), gain.g ? static_cast<const float*>(gain.g) + gpos : nullptr, robin,
                   weights);
  else
    tb_impl<double>(static_cast<const double*>(src), static_cast<double*>(dst), L, row_begin, row_end, k, r, arith, bc,
                    static_cast<const double*>(source), static_cast<const double*>(rmap), static_cast<const double*>(rx),
                    static_cast<const double*>(ry), gain.g ? static_cast<const double*>(gain.g) + gpos : nullptr, robin,
                    weights);
}

void init(DType dt, void* field, const SlabLayout& L, const kern::IcParams& ic, const double* xc,
          const double* yc) {
  if (dt == DType::F32)
    init_impl<float>(static_cast<float*>(field), L, ic, xc, yc);
  else
    init_impl<double>(static_cast<double*>(field), L, ic, xc, yc);
}

void stats(DType dt, const void* field, const void* other, const SlabLayout& L, double out[6]) {
  if (dt == DType::F32)
    stats_impl<float>(static_cast<const float*>(field), static_cast<const float*>(other), L, out);
  else
    stats_impl<double>(static_cast<const double*>(field), static_cast<const double*>(other), L, out);
}

void wrap_cols(DType dt, void* field, const SlabLayout& L, int64_t r0, int64_t r1) {
  if (r1 <= r0) return;
  HEAT2D_REQUIRE(r0 >= -L.halo && r1 <= L.nrows + L.halo, "wrap_cols: rows outside the allocation");
  HEAT2D_REQUIRE(L.ncols >= kern::kWrapCols, "periodic y needs at least kWrapCols (24) owned columns");
  if (dt == DType::F32) wrap_cols_impl<float>(static_cast<float*>(field), L, r0, r1);
  else wrap_cols_impl<double>(static_cast<double*>(field), L, r0, r1);
}

void ins_cols(DType dt, void* field, const SlabLayout& L, int64_t r0, int64_t r1) {
  if (r1 <= r0) return;
  HEAT2D_REQUIRE(r0 >= -L.halo && r1 <= L.nrows + L.halo, "ins_cols: rows outside the allocation");
  if (dt == DType::F32) ins_cols_impl<float>(static_cast<float*>(field), L, r0, r1);
  else ins_cols_impl<double>(static_cast<double*>(field), L, r0, r1);
}

void rob_cols(DType dt, void* field, const SlabLayout& L, int64_t r0, int64_t r1, const double* pairs, int arith) {
  if (r1 <= r0) return;
  HEAT2D_REQUIRE(pairs && (arith == 0 || arith == 1), "rob_cols: the walls' pairs and arith 0 (exact) or 1 (fma)");
  HEAT2D_REQUIRE(r0 >= -L.halo && r1 <= L.nrows + L.halo, "rob_cols: rows outside the allocation");
  if (dt == DType::F32) rob_cols_impl<float>(static_cast<float*>(field), L, r0, r1, pairs, arith);
  else rob_cols_impl<double>(static_cast<double*>(field), L, r0, r1, pairs, arith);
}

void rob_rows(DType dt, void* field, const SlabLayout& L, bool lo, bool hi, const double* pairs, int arith) {
  HEAT2D_REQUIRE(pairs && (arith == 0 || arith == 1), "rob_rows: the walls' pairs and arith 0 (exact) or 1 (fma)");
  HEAT2D_REQUIRE(L.halo >= 1 && L.nrows >= 1, "rob_rows: no room for the frame rows");
  auto one = [&](int64_t to, int64_t from, double a, double b) {
    if (dt == DType::F32) {
      float* f = static_cast<float*>(field);
      rob_row_impl<float>(f + L.offset(to, -L.cpad), f + L.offset(from, -L.cpad), L.pitch, (float)a, (float)b, arith);
    } else {
      double* f = static_cast<double*>(field);
      rob_row_impl<double>(f + L.offset(to, -L.cpad), f + L.offset(from, -L.cpad), L.pitch, a, b, arith);
    }
  };
  if (lo && L.row0 == 0) one(-1, 0, pairs[0], pairs[1]);
  if (hi && L.row0 + L.nrows == L.nrows_global) one(L.nrows, L.nrows - 1, pairs[2], pairs[3]);
}

void ins_rows(DType dt, void* field, const SlabLayout& L, bool lo, bool hi) {
  HEAT2D_REQUIRE(L.halo >= 1 && L.nrows >= 1, "ins_rows: no room for the frame rows");
  const size_t es = dtype_size(dt), bytes = (size_t)L.pitch * es;
  char* base = static_cast<char*>(field);
  auto row = [&](int64_t i) { return base + (size_t)((i + L.halo) * L.pitch) * es; };
  if (lo && L.row0 == 0) std::memcpy(row(-1), row(0), bytes);
  if (hi && L.row0 + L.nrows == L.nrows_global) std::memcpy(row(L.nrows), row(L.nrows - 1), bytes);
}

void wrap_rows(DType dt, void* field, const SlabLayout& L, int64_t k) {
  if (k <= 0) return;
  HEAT2D_REQUIRE(k <= L.halo && k <= L.nrows, "wrap_rows: depth exceeds the halo or the owned rows");
  const size_t es = dtype_size(dt), bytes = (size_t)(k * L.pitch) * es;
  char* base = static_cast<char*>(field);
  auto row = [&](int64_t i) { return base + (size_t)((i + L.halo) * L.pitch) * es; };
  std::memcpy(row(-k), row(L.nrows - k), bytes);
  std::memcpy(row(L.nrows), row(0), bytes);
}

void pack_rows(DType dt, const void* field, const SlabLayout& L, int64_t row, int64_t nrows, void* buf) {
  const size_t es = dtype_size(dt);
  for (int64_t i = 0; i < nrows; ++i)
    std::memcpy(static_cast<char*>(buf) + (size_t)(i * L.ncols) * es,
                static_cast<const char*>(field) + (size_t)L.offset(row + i, 0) * es, (size_t)L.ncols * es);
}

void unpack_rows(DType dt, void* field, const SlabLayout& L, int64_t row, int64_t nrows, const void* buf) {
  const size_t es = dtype_size(dt);
  for (int64_t i = 0; i < nrows; ++i)
    std::memcpy(static_cast<char*>(field) + (size_t)L.offset(row + i, 0) * es,
                static_cast<const char*>(buf) + (size_t)(i * L.ncols) * es, (size_t)L.ncols * es);
}

// Twin of kernels/probe_cone.hip: the same levels over the same two planes,
// one probe after the other, through the shared probe_point (heat2d/probe.hpp).
namespace {
template <typename T, int MODE, int AR, bool GAIN = false, bool ROB = false>
void probe_cone_run(const kern::ProbeArgs& a) {
  constexpr int S = kern::kProbeSide;
  std::vector<T> planes((size_t)2 * S * S, T(0));
  T* plane[2] = {planes.data(), planes.data() + S * S};
  const T* src = static_cast<const T*>(a.src);
  T* hist = static_cast<T*>(a.hist);
  const int k = a.k, side = 2 * k + 1;
  const int64_t base = (a.base ? *a.base : 0) + a.base0;
  for (int64_t p = 0; p < a.P; ++p) {
    const int64_t ci = a.pts[2 * p], cj = a.pts[2 * p + 1];
    for (int idx = 0; idx < side * side; ++idx) {
      const int u = idx / side, v = idx % side;
      const int64_t row = ci - k + u, col = cj - k + v;
      if (kern::probe_loads(a, row, col)) plane[0][u * S + v] = src[a.L.offset(row, col)];
    }
    for (int s = 1; s <= k; ++s) {
      const int w = 2 * (k - s) + 1;
      for (int idx = 0; idx < w * w; ++idx)
        kern::probe_point<T, MODE, AR, GAIN, ROB>(a, ci, cj, s, idx, plane[(s - 1) & 1], plane[s & 1]);
      if (base + s - 1 < a.capacity) hist[(base + s - 1) * a.P + p] = plane[s & 1][k * S + k];
    }
  }
}
// ... of the five-weight operator (kernels/probe_cone.hip probe_cone_w5)
template <typename T, int AR>
void probe_cone_w5_run(const kern::ProbeArgs& a) {
  constexpr int S = kern::kProbeSide;
  std::vector<T> planes((size_t)2 * S * S);
  T* plane[2] = {planes.data(), planes.data() + (size_t)S * S};
  const T* src = static_cast<const T*>(a.src);
  T* hist = static_cast<T*>(a.hist);
  const int k = a.k, side = 2 * k + 1;
  const int64_t base = (a.base ? *a.base : 0) + a.base0;
  for (int64_t p = 0; p < a.P; ++p) {
    const int64_t ci = a.pts[2 * p], cj = a.pts[2 * p + 1];
    for (int idx = 0; idx < side * side; ++idx) {
      const int u = idx / side, v = idx % side;
      const int64_t row = ci - k + u, col = cj - k + v;
      if (kern::probe_loads(a, row, col)) plane[0][u * S + v] = src[a.L.offset(row, col)];
    }
    for (int s = 1; s <= k; ++s) {
      const int w = 2 * (k - s) + 1;
      for (int idx = 0; idx < w * w; ++idx) kern::probe_point_w5<T, AR>(a, ci, cj, s, idx, plane[(s - 1) & 1], plane[s & 1]);
      if (base + s - 1 < a.capacity) hist[(base + s - 1) * a.P + p] = plane[s & 1][k * S + k];
    }
  }
}
template <typename T, int MODE>
void probe_cone_mode(const kern::ProbeArgs& a, int arith) {
  if (arith == 0) probe_cone_run<T, MODE, 0>(a);
  else if (arith == 1) probe_cone_run<T, MODE, 1>(a);
  else if constexpr (MODE == kern::kProbePlain) probe_cone_run<T, MODE, 2>(a);
  else fail(__FILE__, __LINE__, "probe_cone: a source, a map or faces take arith exact or fma");
}
template <typename T>
void probe_cone_typed(const kern::ProbeArgs& a, int arith) {
  if (a.w5) {
    HEAT2D_REQUIRE(!a.source && !a.rmap && !a.rx && !a.gain && !a.robin && a.wall_r0 == INT64_MIN && a.wall_c0 == INT64_MIN &&
                       arith <= 1,
                   "probe_cone: weights take the plain mode, Dirichlet or periodic axes and arith exact or fma");
    if (arith == 0) probe_cone_w5_run<T, 0>(a);
    else probe_cone_w5_run<T, 1>(a);
  } else if (a.robin) {
    HEAT2D_REQUIRE(!a.source && !a.rmap && !a.rx && !a.gain && (arith == 0 || arith == 1),
                   "probe_cone: Robin walls take the plain mode and arith exact or fma");
    if (arith == 0) probe_cone_run<T, kern::kProbePlain, 0, false, true>(a);
    else probe_cone_run<T, kern::kProbePlain, 1, false, true>(a);
  } else if (a.gain) {
    HEAT2D_REQUIRE(a.source && (arith == 0 || arith == 1), "probe_cone: a gain schedule needs a source and arith exact or fma");
    if (arith == 0) probe_cone_run<T, kern::kProbeSource, 0, true>(a);
    else probe_cone_run<T, kern::kProbeSource, 1, true>(a);
  } else if (a.source) probe_cone_mode<T, kern::kProbeSource>(a, arith);
  else if (a.rmap) probe_cone_mode<T, kern::kProbeMap>(a, arith);
  else if (a.rx) probe_cone_mode<T, kern::kProbeFaces>(a, arith);
  else probe_cone_mode<T, kern::kProbePlain>(a, arith);
}
}  // namespace

void probe_cone(DType dt, const kern::ProbeArgs& a, int arith) {
  if (a.P <= 0) return;
  HEAT2D_REQUIRE(a.P <= kMaxProbes, "probe_cone: more than kMaxProbes points");
  HEAT2D_REQUIRE(a.k >= 1 && a.k <= kMaxTB && a.k <= a.L.halo, "probe_cone: depth outside [1, min(kMaxTB, halo)]");
  HEAT2D_REQUIRE(arith >= 0 && arith <= 2, "probe_cone: arith exact (0), fma (1) or jacobi (2)");
  HEAT2D_REQUIRE((a.rx == nullptr) == (a.ry == nullptr), "probe_cone: both face buffers or neither");
  if (dt == DType::F64) probe_cone_typed<double>(a, arith);
  else probe_cone_typed<float>(a, arith);
}

}  // namespace cpu
}  // namespace heat2d
