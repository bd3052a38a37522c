// life_block variant: BitsIO<1, kXlaneDpp> (see life_block_impl.hpp).
#include "life_block_launch.hpp"

namespace gol {
namespace hipk {

GOL_LIFE_VARIANT(launch_bits_w1_dpp) { return lb::launch_variant<lb::BitsIO<1, kXlaneDpp>>(p, out_rows, T, tune, ctx, s); }

}  // namespace hipk
}  // namespace gol
