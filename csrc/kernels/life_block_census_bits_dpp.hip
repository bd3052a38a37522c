// Census kernels (per-generation live-cell counts), variant bits_dpp: see life_block_launch.hpp.
#include "life_block_launch.hpp"

GOL_FEATURE_TU(lb::CensusIO, census, bits_dpp)
