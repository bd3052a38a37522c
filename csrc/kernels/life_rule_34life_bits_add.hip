// Rule kernels of 34life (life_rules.def), variant bits_add: see life_block_launch.hpp.
#include "life_block_launch.hpp"

GOL_RULE_TU_BITS_ADD(34life)
