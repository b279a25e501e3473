// Instantiation unit: the general temporal-blocked stencil of the five-weight operator
// (double, ring 4, contracted fma arithmetic AR = 1; see tb_impl.hpp tb_kernel_w5 / March W5).
#include "tb_impl.hpp"

namespace heat2d {
namespace kern {
namespace tbimpl {
H2D_FEAT_UNIT(FamW5, double, 1, H2D_TB_CASES_DEEP)
}  // namespace tbimpl
}  // namespace kern
}  // namespace heat2d
