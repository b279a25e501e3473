// Instantiation unit (fast arithmetic, AR = 3): the wave-pair interior kernel, double, 32 B per lane,
// K = 16..24 (see tb_pipe_impl.hpp).
#include "tb_pipe_impl.hpp"

namespace heat2d {
namespace kern {
namespace tbimpl {
H2D_PIPE_UNIT(3)
}  // namespace tbimpl
}  // namespace kern
}  // namespace heat2d
