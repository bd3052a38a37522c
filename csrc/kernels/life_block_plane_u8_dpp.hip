// Bounded-plane kernels (dead edges), variant u8_dpp: see life_block_launch.hpp.
#include "life_block_launch.hpp"

GOL_FEATURE_TU(lb::PlaneIO, plane, u8_dpp)
