// Host-only self test of the runtime (engine, CPU backend, in-process thread
// transport, decomposition, text I/O) against the exact serial oracle.
// Built without HIP so it can run under AddressSanitizer / UBSan and
// ThreadSanitizer (the reference has no sanitizer coverage and
// its hybrid build relies on unchecked thread/MPI assumptions):
//
//   python gol_amd/native_build.py --selftest address   -> bin/gol_selftest_address
//   python gol_amd/native_build.py --selftest thread    -> bin/gol_selftest_thread
//
// T0 unit checks (decomposition math, text-format edge cases) come first.
// Every configuration runs P ranks as threads (ThreadHub/ThreadTransport),
// each with its own CPU backend, and compares the gathered grid and the
// "Generations" value with cpu_reference_run.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include <unistd.h>

#include "gol/backend.hpp"
#include "gol/batch.hpp"
#include "gol/cpu_ref.hpp"
#include "gol/decomp.hpp"
#include "gol/engine.hpp"
#include "gol/io.hpp"
#include "gol/transport.hpp"

using namespace gol;

namespace {

struct Case {
  int64_t W, H;
  std::string decomp;
  int P;
  Layout layout;
  int tmax, epoch, overlap;
  int64_t gens;
  uint64_t seed;
  double density;
};

std::vector<uint8_t> random_cells(int64_t W, int64_t H, uint64_t seed, double density) {
  std::vector<uint8_t> g(size_t(W * H));
  const uint32_t th = density_thresh(density);
  for (int64_t r = 0; r < H; ++r)
    for (int64_t c = 0; c < W; ++c) g[size_t(r * W + c)] = rng_cell(seed, r, c, th) ? 1 : 0;
  return g;
}

bool run_case(const Case& k) {
  std::vector<uint8_t> grid = random_cells(k.W, k.H, k.seed, k.density);
  std::vector<uint8_t> ref = grid;
  const RefResult rr = cpu_reference_run(ref, k.W, k.H, k.gens, true, 3, 1);

  auto hub = std::make_shared<ThreadHub>(k.P);
  std::vector<uint8_t> out(grid.size(), 0);
  std::vector<int64_t> gens(size_t(k.P), -1);
  std::vector<std::string> errs(size_t(k.P));
  std::vector<std::thread> ts;
  for (int r = 0; r < k.P; ++r) {
    ts.emplace_back([&, r] {
      try {
        auto be = make_cpu_backend(k.P == 1 ? 4 : 2);  // exercises the thread pool too
        ThreadTransport tr(hub, r, be.get());
        EngineConfig cfg;
        cfg.W = k.W;
        cfg.H = k.H;
        cfg.layout = k.layout;
        cfg.decomp = k.decomp;
        cfg.gen_limit = k.gens;
        cfg.tmax = k.tmax;
        cfg.epoch = k.epoch;
        cfg.overlap = k.overlap;
        cfg.poll_gens = 5;
        Engine eng(cfg, be.get(), &tr);
        eng.load_global(grid.data(), k.W);
        const RunResult res = eng.run();
        gens[size_t(r)] = res.generations;
        const Extent rows = eng.rows(), cols = eng.cols();
        std::vector<uint8_t> tile(size_t(rows.size() * cols.size()));
        eng.store_cells(tile.data(), cols.size(), false);
        for (int64_t i = 0; i < rows.size(); ++i)
          for (int64_t j = 0; j < cols.size(); ++j)
            out[size_t((rows.begin + i) * k.W + cols.begin + j)] = tile[size_t(i * cols.size() + j)];
      } catch (const std::exception& e) {
        errs[size_t(r)] = e.what();
      }
    });
  }
  for (auto& t : ts) t.join();
  bool ok = out == ref;
  for (int r = 0; r < k.P; ++r) {
    if (!errs[size_t(r)].empty()) {
      std::printf("  rank %d error: %s\n", r, errs[size_t(r)].c_str());
      ok = false;
    }
    if (gens[size_t(r)] != rr.generations) ok = false;
  }
  std::printf("%-4s %4lldx%-4lld %-4s P=%d T=%d D=%d overlap=%d gens=%lld ref=%lld -> %s\n",
              k.layout == Layout::Bits ? "bits" : "u8", (long long)k.W, (long long)k.H, k.decomp.c_str(), k.P,
              k.tmax, k.epoch, k.overlap, (long long)gens[0], (long long)rr.generations, ok ? "ok" : "MISMATCH");
  return ok;
}

// Allocation failures while an engine is built (tuning fault_alloc=N: the CPU
// backend's N-th allocation throws): N = 1, 2, ... until an engine is built
// and has run.  A failed attempt must leave nothing allocated - LeakSanitizer
// (the address build) reports what it does leave - and the attempt that gets
// through must still compute the oracle's result.
bool alloc_fault_case(const char* what, Layout layout, int u8_compute, const char* ring, const std::string& decomp,
                      int P, int min_ctor_faults) {
  const int64_t W = 64, H = 32, gens = 8;
  std::vector<uint8_t> grid = random_cells(W, H, 9, 0.4);
  std::vector<uint8_t> ref = grid;
  const RefResult rr = cpu_reference_run(ref, W, H, gens, true, 3, 1);

  auto hub = std::make_shared<ThreadHub>(P);
  std::vector<uint8_t> out(grid.size(), 0);
  const size_t np = size_t(P);
  std::vector<int> ctor_faults(np, 0), run_faults(np, 0);
  std::vector<std::string> errs(np);
  std::vector<std::thread> ts;
  for (int r = 0; r < P; ++r) {
    ts.emplace_back([&, r] {
      // Every rank makes the same allocations, so all of them fail at the
      // same N, before their engines first talk to each other.
      for (int n = 1; n <= 64; ++n) {
        bool built = false;
        try {
          Tuning tune = Tuning::from_env();
          tune.set("fault_alloc", std::to_string(n)).set("cpu_ring", ring);
          auto be = make_cpu_backend(2, -1, tune);
          ThreadTransport tr(hub, r, be.get());
          EngineConfig cfg;
          cfg.W = W;
          cfg.H = H;
          cfg.layout = layout;
          cfg.u8_compute = u8_compute;
          cfg.decomp = decomp;
          cfg.gen_limit = gens;
          cfg.poll_gens = 5;
          cfg.tune = tune;
          Engine eng(cfg, be.get(), &tr);
          built = true;
          if (std::string(ring) == "1" && !eng.row_ring()) fail("no row ring");
          eng.load_global(grid.data(), W);
          const RunResult res = eng.run();  // allocates the flags: one more N fails here
          if (res.generations != rr.generations) fail("generations differ from the oracle");
          const Extent rows = eng.rows(), cols = eng.cols();
          std::vector<uint8_t> tile(size_t(rows.size() * cols.size()));
          eng.store_cells(tile.data(), cols.size(), false);
          for (int64_t i = 0; i < rows.size(); ++i)
            for (int64_t j = 0; j < cols.size(); ++j)
              out[size_t((rows.begin + i) * W + cols.begin + j)] = tile[size_t(i * cols.size() + j)];
          return;
        } catch (const std::exception& e) {
          if (std::string(e.what()).find("allocation of") == std::string::npos) {
            errs[size_t(r)] = e.what();
            return;
          }
          ++(built ? run_faults : ctor_faults)[size_t(r)];
        }
      }
      errs[size_t(r)] = "no attempt got through";
    });
  }
  for (auto& t : ts) t.join();
  bool ok = out == ref;
  for (int r = 0; r < P; ++r) {
    if (!errs[size_t(r)].empty()) {
      std::printf("  rank %d error: %s\n", r, errs[size_t(r)].c_str());
      ok = false;
    }
    if (ctor_faults[size_t(r)] < min_ctor_faults || ctor_faults[size_t(r)] != ctor_faults[0]) ok = false;
  }
  std::printf("alloc faults %-22s %s P=%d: %d constructions and %d runs failed, then 8 generations -> %s\n", what,
              decomp.c_str(), P, ctor_faults[0], run_faults[0], ok ? "ok" : "MISMATCH");
  return ok;
}

bool text_roundtrip() {
  const int64_t W = 77, H = 31;
  std::vector<uint8_t> g = random_cells(W, H, 5, 0.4);
  const std::string path = std::string(std::getenv("TMPDIR") ? std::getenv("TMPDIR") : "/tmp") +
                           "/gol_selftest_" + std::to_string(::getpid()) + ".txt";
  write_text_grid(path, W, H, g.data());
  std::vector<uint8_t> back;
  read_text_grid(path, W, H, back);
  std::remove(path.c_str());
  const bool ok = back == g;
  std::printf("text round trip %lldx%lld -> %s\n", (long long)W, (long long)H, ok ? "ok" : "MISMATCH");
  return ok;
}

// The CPU batch engine (gol/batch.hpp) on a handful of 32 x 8 universes, on
// both boundaries, against a per-cell loop with the same snapshot schedule.
bool batch_case() {
  const int W = 32, H = 8;
  const int64_t B = 6, max_gens = 200, P = 4;
  bool ok = true;
  for (const Boundary bd : {Boundary::Torus, Boundary::Dead}) {
    std::vector<uint8_t> cells;
    for (int64_t b = 0; b < B; ++b) {
      const std::vector<uint8_t> g = random_cells(W, H, uint64_t(20 + b), 0.35);
      cells.insert(cells.end(), g.begin(), g.end());
    }
    BatchConfig cfg;
    cfg.W = W;
    cfg.H = H;
    cfg.boundary = bd;
    cfg.max_gens = max_gens;
    cfg.max_period = P;
    cfg.want_grids = true;
    cfg.clusters = true;
    BatchInput in;
    in.B = B;
    in.cells = cells.data();
    const BatchResult r = run_batch_cpu(3, cfg, in);
    // The cluster census of the run against the finder on its final grids and
    // on the start grids: the counts add up, every cell is in one cluster.
    const std::vector<uint8_t>* const both[] = {&r.grids, &cells};
    for (const std::vector<uint8_t>* grids : both) {
      const ClusterCensus c = find_clusters_cpu(2, W, H, bd, B, grids->data());
      int64_t records = 0, in_clusters = 0, live = 0;
      for (const int32_t n : c.clusters) records += n;
      for (const int32_t n : c.cells) in_clusters += n;
      for (const uint8_t v : *grids) live += v;
      bool same = records == int64_t(c.size()) && in_clusters == live;
      if (grids == &r.grids)
        same = same && c.clusters == r.census.clusters && c.signature == r.census.signature &&
               c.universe == r.census.universe && c.cells == r.census.cells && c.height == r.census.height &&
               c.width == r.census.width && c.spanning == r.census.spanning;
      if (!same) std::printf("  batch clusters (%s): census mismatch\n", boundary_name(bd));
      ok = ok && same;
    }
    for (int64_t b = 0; b < B; ++b) {
      std::vector<uint8_t> g(cells.begin() + b * W * H, cells.begin() + (b + 1) * W * H), snap = g, nxt(g.size());
      int32_t gens = int32_t(max_gens), period = 0;
      int64_t s = 0;
      for (int64_t t = 1; t <= max_gens; ++t) {
        for (int y = 0; y < H; ++y)
          for (int x = 0; x < W; ++x) {
            int n = 0;
            for (int dy = -1; dy <= 1; ++dy)
              for (int dx = -1; dx <= 1; ++dx) {
                if (dy == 0 && dx == 0) continue;
                int yy = y + dy, xx = x + dx;
                if (bd == Boundary::Torus) yy = (yy + H) % H, xx = (xx + W) % W;
                else if (yy < 0 || yy >= H || xx < 0 || xx >= W) continue;
                n += g[size_t(yy * W + xx)];
              }
            nxt[size_t(y * W + x)] = uint8_t(n == 3 || (n == 2 && g[size_t(y * W + x)]));
          }
        g = nxt;
        if (g == snap) {
          gens = int32_t(t), period = int32_t(t - s);
          break;
        }
        if (t - s == P) snap = g, s = t;
      }
      int32_t pop = 0;
      for (const uint8_t v : g) pop += v;
      const uint8_t stop = period == 0 ? kBatchLimit : pop == 0 ? kBatchExtinction : kBatchCycle;
      const bool same = r.generations[size_t(b)] == gens && r.period[size_t(b)] == period &&
                        r.stop[size_t(b)] == stop && r.population[size_t(b)] == pop &&
                        std::equal(g.begin(), g.end(), r.grids.begin() + b * W * H);
      if (!same)
        std::printf("  batch universe %lld (%s): got %d/%d/%s, want %d/%d/%s\n", (long long)b, boundary_name(bd),
                    r.generations[size_t(b)], r.period[size_t(b)], kBatchStopNames[r.stop[size_t(b)]], gens, period,
                    kBatchStopNames[stop]);
      ok = ok && same;
    }
  }
  const uint8_t block[4] = {1, 1, 1, 1}, two[5] = {1, 0, 0, 0, 1};
  bool named = cluster_name(cluster_signature(block, 2, 2)) == "block";
  try {
    (void)cluster_signature(two, 5, 1);
    named = false;
  } catch (const Error&) {
  }
  if (!named) std::printf("  batch clusters: the block's name, or two clusters taken for one\n");
  ok = ok && named;
  std::printf("batch cpu 32x8, 6 universes, torus and dead -> %s\n", ok ? "ok" : "MISMATCH");
  return ok;
}

// T0 unit checks: decomposition math and text-format edge cases.
bool unit_checks() {
  bool ok = true;
  auto check = [&](bool c, const char* what) {
    if (!c) std::printf("  unit check failed: %s\n", what);
    ok = ok && c;
  };
  // split_range: balanced, contiguous, covering
  for (int64_t n : {1, 7, 64, 1000, 32768})
    for (int p : {1, 2, 3, 8}) {
      int64_t next = 0;
      for (int i = 0; i < p; ++i) {
        const Extent e = split_range(n, p, i);
        check(e.begin == next && e.size() >= n / p && e.size() <= n / p + 1, "split_range");
        next = e.end;
      }
      check(next == n, "split_range covers");
    }
  // neighbours on a periodic Px x Py torus; north = previous rows (the
  // reference inverts N/S, src/game_mpi.c:293-294)
  for (int Px : {1, 2, 3, 4})
    for (int Py : {1, 2, 3}) {
      const Decomposition d(96 * Px, 10 * Py, Px, Py, 32);
      for (int r = 0; r < d.nranks(); ++r) {
        const auto nb = d.neighbors(r);
        const int px = d.px_of(r), py = d.py_of(r);
        check(nb[kNorth] == d.rank_of(px, py - 1) && nb[kSouth] == d.rank_of(px, py + 1), "N/S");
        check(nb[kWest] == d.rank_of(px - 1, py) && nb[kEast] == d.rank_of(px + 1, py), "W/E");
        check(nb[kNW] == d.rank_of(px - 1, py - 1) && nb[kSE] == d.rank_of(px + 1, py + 1), "corners");
        check(d.rows(nb[kNorth]).end % d.H == d.rows(r).begin, "north tile ends where mine starts");
        check(d.cols(r).begin % 32 == 0, "column splits word aligned");
      }
    }
  // short input file: an error, not a hang (the reference loops forever,
  // src/game.c:149-167)
  const std::string dir = std::getenv("TMPDIR") ? std::getenv("TMPDIR") : "/tmp";
  const std::string path = dir + "/gol_selftest_short_" + std::to_string(::getpid()) + ".txt";
  if (FILE* f = std::fopen(path.c_str(), "w")) {
    std::fputs("0101\n1010\n", f);
    std::fclose(f);
  }
  bool threw = false;
  std::vector<uint8_t> g;
  try {
    read_text_grid(path, 4, 3, g);
  } catch (const std::exception&) {
    threw = true;
  }
  check(threw, "short file raises");
  // CRLF line ends are accepted like '\n' (fgetc semantics skip both)
  if (FILE* f = std::fopen(path.c_str(), "w")) {
    std::fputs("0101\r\n1010\r\n0011\r\n", f);
    std::fclose(f);
  }
  g.clear();
  read_text_grid(path, 4, 3, g);
  const std::vector<uint8_t> want = {0, 1, 0, 1, 1, 0, 1, 0, 0, 0, 1, 1};
  check(g == want, "CRLF input");
  std::remove(path.c_str());
  std::printf("unit checks -> %s\n", ok ? "ok" : "FAILED");
  return ok;
}

}  // namespace

int main() {
  std::setvbuf(stdout, nullptr, _IOLBF, 0);  // progress survives a timeout kill
  const Case cases[] = {
      {96, 64, "1x2", 2, Layout::U8, 4, 8, 0, 40, 1, 0.5},
      {96, 64, "1x2", 2, Layout::U8, 4, 8, 1, 40, 1, 0.5},
      {128, 96, "2x2", 4, Layout::Bits, 8, 8, 1, 33, 2, 0.5},
      {100, 37, "1x3", 3, Layout::U8, 2, 6, -1, 50, 3, 0.5},
      {160, 90, "2x3", 6, Layout::U8, 4, 12, 1, 30, 4, 0.5},
      {64, 32, "2x1", 2, Layout::Bits, 16, 16, 0, 1000, 11, 0.2},  // terminates early
      {33, 17, "1x1", 1, Layout::U8, 16, 0, -1, 1000, 4, 0.35},
  };
  bool ok = unit_checks();
  for (const Case& k : cases) ok = run_case(k) && ok;
  // Ring, byte and bit buffers live (2 byte tiles + the alive word before the
  // engine stands); column buffers live (4 more).
  ok = alloc_fault_case("u8 on bit rings", Layout::U8, 1, "1", "1x1", 1, 3) && ok;
  ok = alloc_fault_case("bits, column halos", Layout::Bits, -1, "0", "2x2", 4, 7) && ok;
  ok = text_roundtrip() && ok;
  ok = batch_case() && ok;
  std::printf(ok ? "SELFTEST OK\n" : "SELFTEST FAILED\n");
  return ok ? 0 : 1;
}
