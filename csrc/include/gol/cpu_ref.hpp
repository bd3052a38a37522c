// Serial reference engine with exactly the semantics of src/game.c (the
// canonical variant): toroidal B3/S23, an extinction test before
// every generation, a similarity test every SIMILARITY_FREQUENCY generations,
// "Generations" = generation - 1.  It evaluates every generation eagerly, so
// it is the oracle for the lazy termination logic of the engine, and the
// 256^2 CPU plumbing configuration of BASELINE.json.
#pragma once

#include <cstdint>
#include <vector>

#include "gol/common.hpp"

namespace gol {

struct RefResult {
  int64_t generations = 0;
  double loop_ms = 0;
  std::vector<int64_t> population;  // cpu_reference_run(..., census = true)
  std::vector<uint64_t> fingerprint;  // cpu_reference_run(..., fingerprint = true)
};

// `grid` holds H*W cells (0/1 or ASCII) and is overwritten with the final
// generation as 0/1 bytes.  threads > 1 splits the rows like the
// reference's OpenMP build (src/game_openmp.c:34).  `rule`: any Life-like
// rule without B0, applied by its plain per-cell definition (the reference
// itself is B3/S23 only): the exact oracle for "Generations" under any rule.
// `boundary`: Boundary::Dead counts neighbours outside the grid as dead (the
// bounded plane) instead of wrapping around the torus.
// `census`: RefResult::population receives the live cells of every generation
// the loop advanced through (entry i: generation 1 + i; `generations` entries).
// `fingerprint`: RefResult::fingerprint receives the grid fingerprint
// (gol/fingerprint.hpp) of the same generations.
RefResult cpu_reference_run(std::vector<uint8_t>& grid, int64_t W, int64_t H, int64_t gen_limit,
                            bool check_similarity, int sim_freq, int threads, Rule rule = Rule{},
                            Boundary boundary = Boundary::Torus, bool census = false, bool fingerprint = false);

}  // namespace gol
