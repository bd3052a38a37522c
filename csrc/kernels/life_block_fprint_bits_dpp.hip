// Fingerprint kernels (per-generation grid fingerprints), variant bits_dpp: see life_block_launch.hpp.
#include "life_block_launch.hpp"

GOL_FEATURE_TU(lb::FingerprintIO, fprint, bits_dpp)
