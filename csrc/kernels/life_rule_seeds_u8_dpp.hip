// Rule kernels of seeds (life_rules.def), variant u8_dpp: see life_block_launch.hpp.
#include "life_block_launch.hpp"

GOL_RULE_TU_U8_DPP(seeds)
