// Instantiation unit: the general temporal-blocked stencil with a diffusivity map
// (double, ring 4, reference arithmetic AR = 0; see tb_impl.hpp tb_kernel_var / March VAR).
#include "tb_impl.hpp"

namespace heat2d {
namespace kern {
namespace tbimpl {
H2D_FEAT_UNIT(FamVar, double, 0, H2D_NO_CASES)
}  // namespace tbimpl
}  // namespace kern
}  // namespace heat2d
