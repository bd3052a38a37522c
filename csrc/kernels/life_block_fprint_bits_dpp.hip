// Fingerprint kernels (per-generation grid fingerprints), variant bits_dpp: see life_block_launch.hpp.
#include "life_block_launch.hpp"

GOL_FPRINT_TU_BITS_DPP
