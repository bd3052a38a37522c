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
//
// The cluster census (BatchConfig::clusters, find_clusters_*): what the final
// grid of a universe consists of.  Identical on every engine.  Distances and
// coordinates follow the universe's topology: the torus wraps on both axes,
// the bounded plane does not.
//   1. Two live cells are linked when their Chebyshev distance is at most 2
//      (their 3 x 3 neighbourhoods share a cell).
//   2. A cluster is a connected component of the live cells under that relation.
//   3. The clusters of a universe are ordered by their smallest cell in
//      row-major order (row first, then column).
//   4. Each axis of a cluster has an origin and an extent (cluster_axis).  With
//      occ the rows (columns) the cluster occupies and n = H (W): on the plane
//      the origin is min(occ) and the extent max - min + 1.  On the torus the
//      origin is the occupied coordinate o for which neither o - 1 nor o - 2
//      (mod n) is occupied - gaps inside a cluster are at most one coordinate
//      wide, so there is at most one - and the extent is 1 + max((p - o) mod n)
//      over the occupied p.  Without such an o the cluster spans the axis:
//      origin 0, extent n.
//   5. The signature is grid_fingerprint (fingerprint.hpp) of the cluster
//      translated to its origin, cell (y, x) at ((y - y0) mod H, (x - x0) mod W).
//      A cluster that spans no axis has the same signature at every position,
//      in every universe shape and on both boundaries; that of a spanning one
//      depends on its position on the spanned axis.
//   6. A record is (universe, signature, cells, height, width, spanning), the
//      extents being height (rows) and width (columns), spanning = kSpansX (the
//      columns) | kSpansY (the rows).  Records are sorted by universe, then
//      in the order of 3.
// A call holds at most kClusterRecordsMax records; on the hip engine a record
// takes 16 bytes of device memory (signature, cells, the packed extents), so
// the records' peak is 4 GiB, besides 8 bytes a universe (count and offset).
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
  bool clusters = false;  // the cluster census of the final grids (see above)
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

// The cluster records of a batch as parallel arrays, and clusters[u], the
// number of records of universe u (its records are contiguous).
constexpr int64_t kClusterRecordsMax = int64_t(1) << 28;  // records per call
enum ClusterSpan : uint8_t { kSpansX = 1, kSpansY = 2 };
struct ClusterCensus {
  std::vector<int32_t> clusters;  // per universe
  std::vector<int32_t> universe;
  std::vector<uint64_t> signature;
  std::vector<int32_t> cells;
  std::vector<int16_t> height, width;
  std::vector<uint8_t> spanning;
  double ms = 0;        // hip: the count and the emit kernel (event pairs); cpu: wall time
  double count_ms = 0;  // hip: the count kernel's share of ms
  size_t size() const { return signature.size(); }
};

struct BatchResult {
  std::vector<int32_t> generations, period, population;
  std::vector<uint8_t> stop;   // BatchStop
  std::vector<uint8_t> grids;  // (B, H, W) 0/1 at each universe's own stop generation; empty unless want_grids
  double kernel_ms = 0;        // hip: the one kernel of the call (event pair); cpu: the loop's wall time
  std::string variant;
  ClusterCensus census;        // empty unless BatchConfig::clusters (census.ms: clusters_ms)
};

// Origin and extent of a cluster on one axis from its n-bit occupancy mask m
// (item 4 above).  As a bit formula the torus' origin is the one bit of
// m & ~rotl(m, 1) & ~rotl(m, 2), rotating inside the n bits; no bit: spanning.
struct ClusterAxis {
  int origin, extent;
  bool spans;
};
GOL_HD inline uint64_t rotl_bits(uint64_t m, int s, int n) {
  const uint64_t field = n == 64 ? ~uint64_t(0) : (uint64_t(1) << n) - 1;
  return s == 0 ? m : ((m << s) | (m >> (n - s))) & field;
}
GOL_HD inline ClusterAxis cluster_axis(uint64_t m, int n, bool torus) {
  if (m == 0) return {0, 0, false};
  int o = __builtin_ctzll(m);
  if (torus) {
    const uint64_t first = m & ~rotl_bits(m, 1, n) & ~rotl_bits(m, 2, n);
    if (first == 0) return {0, n, true};
    o = __builtin_ctzll(first);
  }
  const uint64_t moved = rotl_bits(m, (n - o) % n, n);  // the origin at bit 0
  return {o, 64 - __builtin_clzll(moved), false};
}

// Exclusive scan of the per-universe counts; refuses a total above
// kClusterRecordsMax, naming the limit.  Returns the total.
int64_t cluster_offsets(const std::vector<int32_t>& counts, std::vector<int32_t>& offsets);

// The cluster census of B arbitrary 0/1 grids (B, H, W) of a batch shape.
// threads <= 0: the global host pool.
ClusterCensus find_clusters_cpu(int threads, int W, int H, Boundary boundary, int64_t B, const uint8_t* cells);
// The same on packed universes: H 64-bit rows each, cell x at bit x.
ClusterCensus find_clusters_rows(int threads, int W, int H, Boundary boundary, int64_t B, const uint64_t* rows);
ClusterCensus find_clusters_hip(int device, int W, int H, Boundary boundary, int64_t B, const uint8_t* cells,
                                const Tuning& tune = Tuning::from_env());

// The signature of the one cluster a w x h array of 0/1 holds, on plane
// semantics (any size); fails when it holds none or more than one.
uint64_t cluster_signature(const uint8_t* cells, int64_t w, int64_t h);
// The name of a signature (block, beehive, loaf, boat, tub, ship, pond,
// blinker, toad, beacon, glider, traffic light, ... in every phase and
// symmetric image), or its 16 hex digits.
std::string cluster_name(uint64_t signature);

// One line per kind of cluster: count descending, then signature.  stop_mask:
// bit c set takes the universes with BatchStop c (7: all); stop may be null.
struct ClusterKind {
  uint64_t signature;
  int32_t cells;
  int16_t height, width;
  uint8_t spanning;
  int64_t count;
};
std::vector<ClusterKind> cluster_table(const ClusterCensus& c, const uint8_t* stop = nullptr, unsigned stop_mask = 7);

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
