// Batched small universes: B independent W x H grids of one boundary and one
// rule (or one rule per universe, BatchConfig::rules), each advanced until it
// repeats or reaches max_gens.
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
  // Rule sweeps.  Empty: every universe runs `rule`.  Else R rules of K =
  // soups_per_rule universes each, B = R * K: universe u runs rules[u / K] on
  // soup `share_soups ? u % K : u`.  The soup index selects the cells read
  // (with share_soups the input holds K grids, not B) and the seed, seed + soup.
  // The hip engine then takes the rules as data (any rule without B0).
  std::vector<Rule> rules;
  int64_t soups_per_rule = 1;
  bool share_soups = false;
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
// the shape, B, max_period, max_gens, B0 rules (in `rules` with the index),
// K < 1, R * K outside 1..2^24 or other than B, cells other than 0/1.
void validate_batch(const BatchConfig& cfg, const BatchInput& in);

// The rule and the soup index of universe u (see BatchConfig::rules).
inline Rule batch_rule(const BatchConfig& cfg, int64_t u) {
  return cfg.rules.empty() ? cfg.rule : cfg.rules[size_t(u / cfg.soups_per_rule)];
}
inline int64_t batch_soup(const BatchConfig& cfg, int64_t u) {
  return !cfg.rules.empty() && cfg.share_soups ? u % cfg.soups_per_rule : u;
}
// Grids in BatchInput::cells.
inline int64_t batch_soups(const BatchConfig& cfg, const BatchInput& in) {
  return !cfg.rules.empty() && cfg.share_soups ? cfg.soups_per_rule : in.B;
}
// The Life-like rules without B0 in a fixed order (gol_amd.life_like_rules):
// rule i has birth mask (i & 0xFF) << 1 and survive mask i >> 8.
constexpr int64_t kLifeLikeRules = int64_t(1) << 17;
constexpr Rule life_like_rule(int64_t i) { return Rule{uint16_t((i & 0xFF) << 1), uint16_t(i >> 8)}; }

// The end of an engine's variant text: the rule, or "rule table R rules x K".
inline std::string batch_rule_text(const BatchConfig& cfg) {
  if (cfg.rules.empty()) return rule_string(cfg.rule);
  return "rule table " + std::to_string(cfg.rules.size()) + " rules x " + std::to_string(cfg.soups_per_rule);
}

// threads <= 0: the global host pool.  Any rule without B0.
BatchResult run_batch_cpu(int threads, const BatchConfig& cfg, const BatchInput& in);
// One kernel launch on `device` (life_batch.hip).  `rule`: B3/S23 and the rules
// of life_rules.def, compiled in; `rules`: any, read from a table on the device.
// Tuning batch_vmove picks the vertical move.
BatchResult run_batch_hip(int device, const BatchConfig& cfg, const BatchInput& in,
                          const Tuning& tune = Tuning::from_env());

}  // namespace gol
