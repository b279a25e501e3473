// Instantiation unit: the heat-source stencil with a per-step gain schedule
// (float, ring 4, reference arithmetic AR = 0 and contracted fma AR = 1; see
// tb_impl.hpp tb_kernel_gain / March GAIN).
#include "tb_impl.hpp"

namespace heat2d {
namespace kern {
namespace tbimpl {
H2D_FEAT_UNIT(FamGain, float, 0, H2D_NO_CASES)
H2D_FEAT_UNIT(FamGain, float, 1, H2D_NO_CASES)
}  // namespace tbimpl
}  // namespace kern
}  // namespace heat2d
