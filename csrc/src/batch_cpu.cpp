// Batched small universes on the host (gol/batch.hpp): the checks every
// engine shares, and the CPU engine - a universe is H 64-bit rows, a
// generation is the bit-sliced rule of common.hpp on their two 32-bit halves,
// and the universes are spread over the host thread pool.  It is the fast
// oracle of the HIP kernel (life_batch.hip).
#include "gol/batch.hpp"

#include <chrono>
#include <memory>

#include "gol/backend.hpp"
#include "gol/parallel.hpp"

namespace gol {

void validate_batch(const BatchConfig& cfg, const BatchInput& in) {
  const std::string shape = std::to_string(cfg.W) + " x " + std::to_string(cfg.H);
  if (cfg.W != 32 && cfg.W != 64)
    fail("batch: universes of " + shape + " cells: the width must be 32 or 64 (one or two 32-cell words per row)");
  if (cfg.H != 8 && cfg.H != 16 && cfg.H != 32 && cfg.H != 64)
    fail("batch: universes of " + shape + " cells: the height must be 8, 16, 32 or 64 (one row per lane of a wave)");
  if (in.B < 1 || in.B > kBatchMax)
    fail("batch: " + std::to_string(in.B) + " universes: a batch holds 1 to 2^24 = " + std::to_string(kBatchMax));
  if (cfg.max_period < 1 || cfg.max_period > kBatchMaxPeriod)
    fail("batch: max_period = " + std::to_string(cfg.max_period) + ": must be 1 to 2^16 = " +
         std::to_string(kBatchMaxPeriod));
  if (cfg.max_gens < 1 || cfg.max_gens > kBatchMaxGens)
    fail("batch: max_gens = " + std::to_string(cfg.max_gens) + ": must be 1 to 2^24 = " +
         std::to_string(kBatchMaxGens));
  require_no_b0(cfg.rule, rule_string(cfg.rule));
  if (!cfg.rules.empty()) {
    const int64_t R = int64_t(cfg.rules.size()), K = cfg.soups_per_rule;
    if (K < 1) fail("batch: " + std::to_string(K) + " soups per rule: must be at least 1");
    if (K > kBatchMax || R * K > kBatchMax)
      fail("batch: " + std::to_string(R) + " rules x " + std::to_string(K) + " soups: a batch holds 1 to 2^24 = " +
           std::to_string(kBatchMax) + " universes");
    if (in.B != R * K)
      fail("batch: " + std::to_string(in.B) + " universes, but " + std::to_string(R) + " rules x " +
           std::to_string(K) + " soups = " + std::to_string(R * K));
    for (int64_t r = 0; r < R; ++r)
      if (cfg.rules[size_t(r)].birth & 1u)
        fail("batch: rule " + std::to_string(r) + " of the list, " + rule_string(cfg.rules[size_t(r)]) +
             ": B0 is not supported (an empty universe would not stay empty)");
  }
  if (in.cells) {
    const int64_t n = batch_soups(cfg, in) * cfg.H * cfg.W;
    for (int64_t i = 0; i < n; ++i)
      if (in.cells[i] > 1)
        fail("batch: cell " + std::to_string(i % cfg.W) + " of row " + std::to_string(i / cfg.W % cfg.H) +
             " of universe " + std::to_string(i / (int64_t(cfg.W) * cfg.H)) + " is " + std::to_string(in.cells[i]) +
             ": the input holds 0 (dead) and 1 (live) only");
  }
}

namespace {

struct HSum64 {
  uint64_t h0, h1;
};

// One universe from its start to its stop; rows[] ends as the final grid.
template <bool kConway>
void run_universe(const BatchConfig& cfg, Rule rule, uint64_t* rows, int32_t& generations, int32_t& period) {
  const int W = cfg.W, H = cfg.H;
  const uint64_t mask = W == 64 ? ~uint64_t(0) : (uint64_t(1) << W) - 1;
  const bool torus = cfg.boundary == Boundary::Torus;
  uint64_t snap[64], nxt[64];
  HSum64 hs[64];
  for (int y = 0; y < H; ++y) snap[y] = rows[y];
  int64_t k = 0;  // generations since the snapshot
  for (int64_t t = 1; t <= cfg.max_gens; ++t) {
    for (int y = 0; y < H; ++y) {
      const uint64_t c = rows[y];
      const uint64_t l = ((c << 1) | (torus ? c >> (W - 1) : 0)) & mask;  // cell x-1 at bit x
      const uint64_t r = (c >> 1) | (torus ? (c << (W - 1)) & mask : 0);  // cell x+1 at bit x
      hs[y] = {l ^ c ^ r, (l & c) | (l & r) | (c & r)};
    }
    const HSum64 zero{0, 0};
    uint64_t diff = 0;
    for (int y = 0; y < H; ++y) {
      const HSum64& a = y > 0 ? hs[y - 1] : torus ? hs[H - 1] : zero;
      const HSum64& b = hs[y];
      const HSum64& c = y + 1 < H ? hs[y + 1] : torus ? hs[0] : zero;
      uint64_t out = 0;
      for (int half = 0; half < W / 32; ++half) {
        const int sh = 32 * half;
        const HSum ha{uint32_t(a.h0 >> sh), uint32_t(a.h1 >> sh)}, hb{uint32_t(b.h0 >> sh), uint32_t(b.h1 >> sh)},
            hc{uint32_t(c.h0 >> sh), uint32_t(c.h1 >> sh)};
        const uint32_t ctr = uint32_t(rows[y] >> sh);
        const uint32_t v = kConway ? rule_host(ha, hb, hc, ctr) : rule_host(rule, ha, hb, hc, ctr);
        out |= uint64_t(v) << sh;
      }
      nxt[y] = out;
      diff |= out ^ snap[y];
    }
    for (int y = 0; y < H; ++y) rows[y] = nxt[y];
    ++k;
    if (diff == 0) {
      generations = int32_t(t);
      period = int32_t(k);
      return;
    }
    if (k == cfg.max_period) {
      k = 0;
      for (int y = 0; y < H; ++y) snap[y] = rows[y];
    }
  }
  generations = int32_t(cfg.max_gens);
  period = 0;
}

}  // namespace

BatchResult run_batch_cpu(int threads, const BatchConfig& cfg, const BatchInput& in) {
  validate_batch(cfg, in);
  const int W = cfg.W, H = cfg.H;
  const int64_t B = in.B;
  BatchResult res;
  res.generations.assign(size_t(B), 0);
  res.period.assign(size_t(B), 0);
  res.population.assign(size_t(B), 0);
  res.stop.assign(size_t(B), 0);
  if (cfg.want_grids) res.grids.assign(size_t(B * H * W), 0);
  std::vector<uint64_t> final_rows(cfg.clusters ? size_t(B * H) : 0);  // what the cluster census reads
  const uint32_t th = density_thresh(in.density);
  const auto body = [&](int64_t b0, int64_t b1) {
    uint64_t rows[64];
    for (int64_t b = b0; b < b1; ++b) {
      const Rule rule = batch_rule(cfg, b);
      const int64_t soup = batch_soup(cfg, b);
      for (int y = 0; y < H; ++y) {
        uint64_t v = 0;
        for (int x = 0; x < W; ++x) {
          const bool live = in.cells ? in.cells[size_t((soup * H + y) * W + x)] != 0
                                     : rng_cell(in.seed + uint64_t(soup), y, x, th);
          v |= uint64_t(live) << x;
        }
        rows[y] = v;
      }
      if (rule_is_default(rule)) run_universe<true>(cfg, rule, rows, res.generations[size_t(b)], res.period[size_t(b)]);
      else run_universe<false>(cfg, rule, rows, res.generations[size_t(b)], res.period[size_t(b)]);
      int32_t pop = 0;
      for (int y = 0; y < H; ++y) pop += __builtin_popcountll(rows[y]);
      res.population[size_t(b)] = pop;
      res.stop[size_t(b)] = res.period[size_t(b)] == 0 ? kBatchLimit : pop == 0 ? kBatchExtinction : kBatchCycle;
      if (cfg.want_grids)
        for (int y = 0; y < H; ++y)
          for (int x = 0; x < W; ++x) res.grids[size_t((b * H + y) * W + x)] = uint8_t((rows[y] >> x) & 1u);
      if (cfg.clusters)
        for (int y = 0; y < H; ++y) final_rows[size_t(b * H + y)] = rows[y];
    }
  };
  const auto t0 = std::chrono::steady_clock::now();
  if (threads > 0) {
    ThreadPool pool(threads);
    pool.parallel_for(B, body);
  } else {
    global_pool().parallel_for(B, body);
  }
  res.kernel_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  res.variant = "batch cpu " + std::to_string(W) + "x" + std::to_string(H) + " " + boundary_name(cfg.boundary) +
                " rows64 " + batch_rule_text(cfg);
  if (cfg.clusters) res.census = find_clusters_rows(threads, W, H, cfg.boundary, B, final_rows.data());
  return res;
}

}  // namespace gol
