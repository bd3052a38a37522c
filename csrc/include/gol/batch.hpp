// Batched small universes: B independent W x H grids of one rule and one
// boundary, each advanced until it repeats or reaches max_gens.
//
// The engine (engine.hpp) streams one huge grid through temporal blocks; a
// thousand 64 x 64 soups through it are a thousand launch-latency-bound runs.
// Here a universe is small enough to live in registers (hip engine: one row
// per lane, life_batch.hip) or in H machine words (cpu engine), and the stop
// test runs every generation on the cells themselves.
//
// Semantics, identical on every engine.  With max_period = P the state is
// saved at generations 0, P, 2P, ...  After computing generation t >= 1 it is
// compared with the snapshot of generation s = P * floor((t - 1) / P) - at
// t = s + P before the new snapshot is taken.  On equality the universe stops:
// generations = t, period = t - s, stop = extinction where the grid is empty
// (the period is then 1), else cycle.  A snapshot on a cycle of length
// L <= P first recurs at s + L and a snapshot off the cycle never recurs, so
// the period is the minimal one whenever it is <= P.  A universe that has not
// stopped after max_gens generations reports generations = max_gens,
// period = 0, stop = limit.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "gol/common.hpp"
#include "gol/tuning.hpp"

namespace gol {

// BatchResult::stop codes, and their names (gol_amd.BATCH_STOP).
enum BatchStop : uint8_t { kBatchLimit = 0, kBatchCycle = 1, kBatchExtinction = 2 };
constexpr const char* kBatchStopNames[] = {"limit", "cycle", "extinction"};

constexpr int64_t kBatchMax = int64_t(1) << 24;         // universes per call
constexpr int64_t kBatchMaxGens = int64_t(1) << 24;     // max_gens
constexpr int64_t kBatchMaxPeriod = int64_t(1) << 16;   // max_period

struct BatchConfig {
  int W = 64, H = 64;  // W in {32, 64}, H in {8, 16, 32, 64}
  Rule rule;
  Boundary boundary = Boundary::Torus;
  int64_t max_gens = 1024;
  int64_t max_period = 64;
  bool want_grids = false;
};

// What a batch starts from: B grids of 0/1 bytes, (B, H, W) row-major, or
// the seed of universe 0 (universe b is random_grid(W, H, seed + b, density)).
struct BatchInput {
  int64_t B = 0;
  const uint8_t* cells = nullptr;  // nullptr: random
  uint64_t seed = 1;
  double density = 0.5;
};

struct BatchResult {
  std::vector<int32_t> generations, period, population;
  std::vector<uint8_t> stop;   // BatchStop
  std::vector<uint8_t> grids;  // (B, H, W) 0/1 at each universe's own stop generation; empty unless want_grids
  double kernel_ms = 0;        // hip: the one kernel of the call (event pair); cpu: the loop's wall time
  std::string variant;
};

// Refuses what no engine runs, each message naming the limit it enforces:
// the shape, B, max_period, max_gens, B0 rules, cells other than 0/1.
void validate_batch(const BatchConfig& cfg, const BatchInput& in);

// threads <= 0: the global host pool.  Any rule without B0.
BatchResult run_batch_cpu(int threads, const BatchConfig& cfg, const BatchInput& in);
// One kernel launch on `device` (life_batch.hip).  B3/S23 and the rules of
// life_rules.def; tuning batch_vmove picks the vertical move.
BatchResult run_batch_hip(int device, const BatchConfig& cfg, const BatchInput& in,
                          const Tuning& tune = Tuning::from_env());

}  // namespace gol
