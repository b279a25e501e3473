// Instantiation unit: the general temporal-blocked stencil with insulated edges
// (double, ring 4, r = 1/4 arithmetic AR = 2; see tb_impl.hpp tb_kernel_ins / March INS).
#include "tb_impl.hpp"

namespace heat2d {
namespace kern {
namespace tbimpl {
H2D_FEAT_UNIT(FamIns, double, 2, H2D_TB_CASES_DEEP)
}  // namespace tbimpl
}  // namespace kern
}  // namespace heat2d
