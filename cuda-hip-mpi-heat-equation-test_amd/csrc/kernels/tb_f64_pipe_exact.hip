// Instantiation unit (exact arithmetic, AR = 0): the wave-pair interior kernel, double, 32 B per lane,
// K = 16..24 (see tb_pipe_impl.hpp).
#include "tb_pipe_impl.hpp"

namespace heat2d {
namespace kern {
namespace tbimpl {
H2D_PIPE_UNIT(0)
}  // namespace tbimpl
}  // namespace kern
}  // namespace heat2d
