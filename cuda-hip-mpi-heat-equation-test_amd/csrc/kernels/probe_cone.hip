// Probe points (heat2d/probe.hpp): one 256-thread workgroup per probe and
// cycle advances the (2k+1)^2 patch around the probe k levels between two LDS
// planes and stores the centre after every level — the per-step history that a
// fused pass keeps in registers only.
//
// The patch is read from the cycle's SOURCE buffer, which the pass leaves
// untouched, so the kernel runs beside any stencil kernel and none of them
// changes. Pinning and boundaries are explicit (probe_point): frame lines keep
// their value, a point next to an insulated wall takes its own value for the
// operand beyond it, ghost rows / columns of a periodic axis are read as they
// lie in memory. Coefficients (source, map, faces) come from global memory at
// every level. No scratch, no waits, nothing shared between workgroups.
#include <hip/hip_runtime.h>

#include "heat2d/probe.hpp"

namespace heat2d {
namespace kern {
namespace {

template <typename T, int MODE, int AR>
__global__ __launch_bounds__(256) void probe_cone(ProbeArgs a) {
  __shared__ T plane[2][kProbeSide * kProbeSide];
  const int64_t p = blockIdx.x;
  const int64_t ci = a.pts[2 * p], cj = a.pts[2 * p + 1];
  const int k = a.k, side = 2 * k + 1;
  const T* src = static_cast<const T*>(a.src);
  for (int idx = threadIdx.x; idx < side * side; idx += 256) {
    const int u = idx / side, v = idx % side;
    const int64_t row = ci - k + u, col = cj - k + v;
    if (probe_loads(a, row, col)) plane[0][u * kProbeSide + v] = src[a.L.offset(row, col)];
  }
  __syncthreads();
  const int64_t base = (a.base ? *a.base : 0) + a.base0;
  T* hist = static_cast<T*>(a.hist);
  for (int s = 1; s <= k; ++s) {
    const int w = 2 * (k - s) + 1;
    const T* in = plane[(s - 1) & 1];
    T* out = plane[s & 1];
    for (int idx = threadIdx.x; idx < w * w; idx += 256) probe_point<T, MODE, AR>(a, ci, cj, s, idx, in, out);
    __syncthreads();
    if (threadIdx.x == 0 && base + s - 1 < a.capacity) hist[(base + s - 1) * a.P + p] = out[k * kProbeSide + k];
  }
}

// The source cone with a gain schedule (ProbeArgs::gain): the same planes and
// levels, level s scaled by its gain (probe_update GAIN).
template <typename T, int AR>
__global__ __launch_bounds__(256) void probe_cone_gain(ProbeArgs a) {
  __shared__ T plane[2][kProbeSide * kProbeSide];
  const int64_t p = blockIdx.x;
  const int64_t ci = a.pts[2 * p], cj = a.pts[2 * p + 1];
  const int k = a.k, side = 2 * k + 1;
  const T* src = static_cast<const T*>(a.src);
  for (int idx = threadIdx.x; idx < side * side; idx += 256) {
    const int u = idx / side, v = idx % side;
    const int64_t row = ci - k + u, col = cj - k + v;
    if (probe_loads(a, row, col)) plane[0][u * kProbeSide + v] = src[a.L.offset(row, col)];
  }
  __syncthreads();
  const int64_t base = (a.base ? *a.base : 0) + a.base0;
  T* hist = static_cast<T*>(a.hist);
  for (int s = 1; s <= k; ++s) {
    const int w = 2 * (k - s) + 1;
    const T* in = plane[(s - 1) & 1];
    T* out = plane[s & 1];
    for (int idx = threadIdx.x; idx < w * w; idx += 256) probe_point<T, kProbeSource, AR, true>(a, ci, cj, s, idx, in, out);
    __syncthreads();
    if (threadIdx.x == 0 && base + s - 1 < a.capacity) hist[(base + s - 1) * a.P + p] = out[k * kProbeSide + k];
  }
}

// The plain cone with Robin walls (ProbeArgs::rob): the same planes and levels,
// the operand beyond a wall the wall's ghost value (probe_point ROB).
template <typename T, int AR>
__global__ __launch_bounds__(256) void probe_cone_rob(ProbeArgs a) {
  __shared__ T plane[2][kProbeSide * kProbeSide];
  const int64_t p = blockIdx.x;
  const int64_t ci = a.pts[2 * p], cj = a.pts[2 * p + 1];
  const int k = a.k, side = 2 * k + 1;
  const T* src = static_cast<const T*>(a.src);
  for (int idx = threadIdx.x; idx < side * side; idx += 256) {
    const int u = idx / side, v = idx % side;
    const int64_t row = ci - k + u, col = cj - k + v;
    if (probe_loads(a, row, col)) plane[0][u * kProbeSide + v] = src[a.L.offset(row, col)];
  }
  __syncthreads();
  const int64_t base = (a.base ? *a.base : 0) + a.base0;
  T* hist = static_cast<T*>(a.hist);
  for (int s = 1; s <= k; ++s) {
    const int w = 2 * (k - s) + 1;
    const T* in = plane[(s - 1) & 1];
    T* out = plane[s & 1];
    for (int idx = threadIdx.x; idx < w * w; idx += 256)
      probe_point<T, kProbePlain, AR, false, true>(a, ci, cj, s, idx, in, out);
    __syncthreads();
    if (threadIdx.x == 0 && base + s - 1 < a.capacity) hist[(base + s - 1) * a.P + p] = out[k * kProbeSide + k];
  }
}

// The cone of the five-weight operator (ProbeArgs::wt): the same planes and levels,
// every point the weighted sum of its five operands (probe_point_w5).
template <typename T, int AR>
__global__ __launch_bounds__(256) void probe_cone_w5(ProbeArgs a) {
  __shared__ T plane[2][kProbeSide * kProbeSide];
  const int64_t p = blockIdx.x;
  const int64_t ci = a.pts[2 * p], cj = a.pts[2 * p + 1];
  const int k = a.k, side = 2 * k + 1;
  const T* src = static_cast<const T*>(a.src);
  for (int idx = threadIdx.x; idx < side * side; idx += 256) {
    const int u = idx / side, v = idx % side;
    const int64_t row = ci - k + u, col = cj - k + v;
    if (probe_loads(a, row, col)) plane[0][u * kProbeSide + v] = src[a.L.offset(row, col)];
  }
  __syncthreads();
  const int64_t base = (a.base ? *a.base : 0) + a.base0;
  T* hist = static_cast<T*>(a.hist);
  for (int s = 1; s <= k; ++s) {
    const int w = 2 * (k - s) + 1;
    const T* in = plane[(s - 1) & 1];
    T* out = plane[s & 1];
    for (int idx = threadIdx.x; idx < w * w; idx += 256) probe_point_w5<T, AR>(a, ci, cj, s, idx, in, out);
    __syncthreads();
    if (threadIdx.x == 0 && base + s - 1 < a.capacity) hist[(base + s - 1) * a.P + p] = out[k * kProbeSide + k];
  }
}

__global__ __launch_bounds__(64) void gain_step(const int64_t* from, int64_t* to, int k) {
  if (threadIdx.x == 0) *to = *from + k;
}

__global__ __launch_bounds__(64) void probe_advance(int64_t* base, int k) {
  if (threadIdx.x == 0) *base = *base + k;
}

template <typename T, int MODE>
void launch_mode(const ProbeArgs& a, int arith, hipStream_t stream) {
  const dim3 grid((unsigned)a.P), block(256);
  if (arith == 0) hipLaunchKernelGGL((probe_cone<T, MODE, 0>), grid, block, 0, stream, a);
  else if (arith == 1) hipLaunchKernelGGL((probe_cone<T, MODE, 1>), grid, block, 0, stream, a);
  else if constexpr (MODE == kProbePlain) hipLaunchKernelGGL((probe_cone<T, MODE, 2>), grid, block, 0, stream, a);
  else fail(__FILE__, __LINE__, "probe_cone: a source, a map or faces take arith exact or fma");
}

template <typename T>
void launch_typed(const ProbeArgs& a, int arith, hipStream_t stream) {
  if (a.w5) {
    const dim3 grid((unsigned)a.P), block(256);
    if (a.source || a.rmap || a.rx || a.gain || a.robin || a.wall_r0 != INT64_MIN || a.wall_c0 != INT64_MIN || arith > 1)
      fail(__FILE__, __LINE__, "probe_cone: weights take the plain mode, Dirichlet or periodic axes and arith exact or fma");
    if (arith == 0) hipLaunchKernelGGL((probe_cone_w5<T, 0>), grid, block, 0, stream, a);
    else hipLaunchKernelGGL((probe_cone_w5<T, 1>), grid, block, 0, stream, a);
  } else if (a.robin) {
    const dim3 grid((unsigned)a.P), block(256);
    if (a.source || a.rmap || a.rx || a.gain || arith > 1)
      fail(__FILE__, __LINE__, "probe_cone: Robin walls take the plain mode and arith exact or fma");
    if (arith == 0) hipLaunchKernelGGL((probe_cone_rob<T, 0>), grid, block, 0, stream, a);
    else hipLaunchKernelGGL((probe_cone_rob<T, 1>), grid, block, 0, stream, a);
  } else if (a.gain) {
    const dim3 grid((unsigned)a.P), block(256);
    if (!a.source || arith > 1) fail(__FILE__, __LINE__, "probe_cone: a gain schedule needs a source and arith exact or fma");
    if (arith == 0) hipLaunchKernelGGL((probe_cone_gain<T, 0>), grid, block, 0, stream, a);
    else hipLaunchKernelGGL((probe_cone_gain<T, 1>), grid, block, 0, stream, a);
  } else if (a.source) launch_mode<T, kProbeSource>(a, arith, stream);
  else if (a.rmap) launch_mode<T, kProbeMap>(a, arith, stream);
  else if (a.rx) launch_mode<T, kProbeFaces>(a, arith, stream);
  else launch_mode<T, kProbePlain>(a, arith, stream);
}

}  // namespace

void launch_probe_cone(DType dt, const ProbeArgs& a, int arith, hipStream_t stream) {
  if (a.P <= 0) return;
  HEAT2D_REQUIRE(a.P <= kMaxProbes, "probe_cone: more than kMaxProbes points");
  HEAT2D_REQUIRE(a.k >= 1 && a.k <= kMaxTB && a.k <= a.L.halo, "probe_cone: depth outside [1, min(kMaxTB, halo)]");
  HEAT2D_REQUIRE(arith >= 0 && arith <= 2, "probe_cone: arith exact (0), fma (1) or jacobi (2)");
  HEAT2D_REQUIRE((a.rx == nullptr) == (a.ry == nullptr), "probe_cone: both face buffers or neither");
  if (dt == DType::F64) launch_typed<double>(a, arith, stream);
  else launch_typed<float>(a, arith, stream);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) fail(__FILE__, __LINE__, std::string("probe_cone launch: ") + hipGetErrorString(e));
}

void launch_gain_step(const int64_t* from, int64_t* to, int k, hipStream_t stream) {
  hipLaunchKernelGGL(gain_step, dim3(1), dim3(64), 0, stream, from, to, k);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) fail(__FILE__, __LINE__, std::string("gain_step launch: ") + hipGetErrorString(e));
}

void launch_probe_advance(int64_t* base, int k, hipStream_t stream) {
  hipLaunchKernelGGL(probe_advance, dim3(1), dim3(64), 0, stream, base, k);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) fail(__FILE__, __LINE__, std::string("probe_advance launch: ") + hipGetErrorString(e));
}

}  // namespace kern
}  // namespace heat2d
