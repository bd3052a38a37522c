// Bounded-plane kernels (dead edges), variant u8_dpp: see life_block_launch.hpp.
#include "life_block_launch.hpp"

GOL_PLANE_TU_U8_DPP
