// Rule kernels of seeds (life_rules.def), variant bits_dpp: see life_block_launch.hpp.
#include "life_block_launch.hpp"

GOL_RULE_TU_BITS_DPP(seeds)
