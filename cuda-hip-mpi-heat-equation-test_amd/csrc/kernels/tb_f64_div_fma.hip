// Instantiation unit: the general temporal-blocked stencil of the conservative form div(k grad u)
// (double, ring 4, contracted fma arithmetic AR = 1; see tb_impl.hpp tb_kernel_div / March DIV).
#include "tb_impl.hpp"

namespace heat2d {
namespace kern {
namespace tbimpl {
H2D_FEAT_UNIT(FamDiv, double, 1, H2D_NO_CASES)
}  // namespace tbimpl
}  // namespace kern
}  // namespace heat2d
