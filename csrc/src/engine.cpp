#include "gol/engine.hpp"

#include <algorithm>
#include <cstdio>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <optional>
#include <thread>

#include "gol/trace.hpp"

namespace gol {

namespace {
// Temporal block sizes built for every backend; 32 and 24 for the byte
// layout only (one grid read + write per pass, docs/PERFORMANCE.md).
constexpr int kTSizes[] = {32, 24, 16, 12, 8, 4, 2, 1};

// Phases of RunResult's device-time split.
enum Phase { kCompute = 0, kHalo = 1, kFill = 2, kReduce = 3, kPhases = 4 };
constexpr size_t kMaxPhaseSpans = size_t(1) << 16;  // per run; later spans go unmeasured

// Overlap auto trial: warm-up epochs (first launches autotune the chained
// groups), then kAutoTrials timed epochs of each schedule, alternating.
constexpr int64_t kAutoWarm = 2;
constexpr int kAutoTrials = 4;

int64_t min_tile_rows(const Decomposition& d) { return d.H / d.Py; }
int64_t min_tile_cols(const Decomposition& d) { return (d.W / d.col_unit / d.Px) * d.col_unit; }
}  // namespace

Engine::Engine(const EngineConfig& cfg, Backend* backend, Transport* transport)
    : cfg_(cfg), be_(backend), tr_(transport) {
  GOL_REQUIRE(be_ && tr_, "engine needs a backend and a transport");
  GOL_REQUIRE(cfg_.W > 0 && cfg_.H > 0, "grid dimensions must be positive");
  GOL_REQUIRE(cfg_.sim_freq > 0, "similarity frequency must be positive");
  GOL_REQUIRE(cfg_.gen_limit >= 0, "generation limit must be >= 0");
  GOL_REQUIRE(cfg_.rule.birth < 512 && cfg_.rule.survive < 512, "rule: neighbour counts are 0..8");
  require_no_b0(cfg_.rule, rule_string(cfg_.rule));
  rank_ = tr_->rank();
  plane_ = cfg_.boundary == Boundary::Dead;
  const BlockFeatures feat{plane_, cfg_.census, cfg_.fingerprint};
  census_.on = feat.census;
  fprint_.on = feat.fingerprint;
  plain_ = !feat.any();
  // Combinations a feature is not built for are refused, not run without it.
  if (plane_) {
    GOL_REQUIRE(!cfg_.self_exchange,
                "boundary=dead with self_exchange (--rehearse-rccl): the rehearsal sends a rank's rows to itself "
                "around the torus, which the bounded plane does not have");
    GOL_REQUIRE(cfg_.graphs <= 0,
                "boundary=dead with graphs=1: captured epochs are not built for the bounded plane");
  }
  for (const Series* s : {&census_, &fprint_}) {
    if (!s->on) continue;
    const std::string n = s->name;
    GOL_REQUIRE(!cfg_.self_exchange, n + "=1 with self_exchange (--rehearse-rccl): the rehearsal's one-rank communicator "
                                         "is not part of the " + n + "'s sum over ranks");
    GOL_REQUIRE(cfg_.graphs <= 0, n + "=1 with graphs=1: captured epochs are not built for the " + n);
  }
  if (cfg_.overlap == 1) cfg_.overlap = 3;  // "on" is the trigger schedule
  int64_t unit = (cfg_.layout == Layout::Bits || cfg_.W % 32 == 0) ? 32 : 1;
  if (cfg_.layout == Layout::Bits)
    GOL_REQUIRE(cfg_.W % 32 == 0, "bit-packed layout needs width % 32 == 0 (use the u8 layout)");
  dec_ = Decomposition::make(cfg_.W, cfg_.H, tr_->size(), cfg_.decomp, unit);

  // Byte layout computed on bit words (EngineConfig::u8_compute): the same
  // decision on every rank (configuration, backend kind and environment).
  if (cfg_.layout == Layout::U8 && cfg_.W % 32 == 0) {
    int mode = cfg_.u8_compute;
    if (mode < 0) mode = cfg_.tune.i("u8_via_bits");
    if (mode < 0) mode = be_->is_device();
    else mode = mode != 0;
    via_bits_ = mode == 1;
  }
  // Layout the temporal blocks run on.
  const Layout cl = via_bits_ ? Layout::Bits : cfg_.layout;
  const std::string refused = be_->refusal(cl, cfg_.rule, cfg_.boundary, feat);
  if (!refused.empty()) fail(refused);
  if (feat.fingerprint) {
    // The device kernels weigh whole 32-cell words: every tile must start on
    // the global word grid (the same answer on every rank).
    if (be_->is_device())
      for (int r = 0; r < dec_.nranks(); ++r)
        GOL_REQUIRE(dec_.cols(r).begin % 32 == 0,
                    "fingerprint=1 with decomposition " + dec_.describe() + " of a byte-layout grid " +
                        std::to_string(cfg_.W) + " cells wide: a tile starts at column " +
                        std::to_string(dec_.cols(r).begin) +
                        ", no multiple of 32, so its words do not line up with the fingerprint's word grid (use a "
                        "decomposition with Px = 1, a width that is a multiple of 32, or the cpu engine)");
  }
  // Every rank must take the same decision (a drifting frame or a schedule
  // that moves a halo exchange is only consistent in lockstep), so it is
  // made for the smallest tile of the decomposition, not this rank's.
  const Backend::KernelChoice kc =
      be_->choose_kernel(cl, min_tile_rows(dec_), std::max<int64_t>(1, min_tile_cols(dec_)), cfg_.tmax, cfg_.rule, feat);
  tmax_ = std::min(kc.tmax, cl == Layout::U8 && !plane_ ? 32 : 16);
  // Epoch depth: a deeper halo means fewer latency-bound exchanges (or local
  // periodic fills: two ~5 us launches each) but ~D redundant rows per epoch.
  // With the grouped kernel the per-rank tile costs the same from 8T to 24T
  // (profiles/sweep_epoch_group.jsonl; 4T is 4 % slower), so one rank uses 8T
  // and several ranks 16T: half the RCCL exchanges (4 per 1000 generations),
  // each one latency-bound.
  const bool row_exchange = dec_.Py > 1 || cfg_.self_exchange;
  int D = cfg_.epoch > 0 ? cfg_.epoch : (tr_->size() > 1 || cfg_.self_exchange ? 16 : 8) * tmax_;
  // A single rank on the plane has nothing to exchange or fill, so a deep
  // halo would only add rows of dead cells to every block: one block per epoch.
  if (plane_ && tr_->size() == 1 && cfg_.epoch <= 0) D = tmax_;
  if (dec_.Py > 1) D = int(std::min<int64_t>(D, min_tile_rows(dec_)));
  if (dec_.Px > 1) {
    int64_t cap = 32 * (min_tile_cols(dec_) / 32);
    GOL_REQUIRE(cap >= 1, "tiles narrower than 32 cells cannot exchange column halos");
    D = int(std::min<int64_t>(D, cap));
  }
  D_ = std::max(1, D);
  tmax_ = std::min(tmax_, D_);
  // A drifting kernel (one-sided window, Backend::drifts) consumes 2 cells of
  // left halo per generation and none on the right; it needs the tile to be
  // the whole torus width so that the drift is a relabeling of columns.
  // Never on the plane: the drift is a relabelling of torus columns.
  drift_ok_ = kc.drift && dec_.Px == 1 && cfg_.W % 32 == 0 && !plane_;
  // Whole-width tiles on a backend that wraps column reads (lane_cols in the
  // HIP kernels) never read their halo columns: no column fills.
  // The plane never wraps: its tiles keep halo columns (so every lane has a
  // word to address), which nothing fills - the kernels mask them.
  cols_filled_ = plane_ || !(dec_.Px == 1 && cfg_.W % 32 == 0 && be_->wraps_columns(cl));
  // A single-rank torus on a backend that also wraps row reads (the LDS-tiled
  // byte kernels): one block per epoch over the owned rows, no fills at all.
  rows_wrapped_ = !cols_filled_ && dec_.Px == 1 && dec_.Py == 1 && !cfg_.self_exchange && be_->wraps_rows(cl);
  if (rows_wrapped_) D_ = tmax_;  // one block per epoch; nothing to fill or exchange
  // Halo columns: none when the kernels wrap (smaller rows to exchange and
  // fill); else D cells per side, 2D on the left for the drifting window.
  int hw = cols_filled_ ? int(ceil_div(drift_ok_ ? 2 * int64_t(D_) : int64_t(D_), 32)) : 0;
  Extent r = rows(), c = cols();
  // Row ring (Backend::row_ring_halo): a single-rank torus whose row halos
  // are second mappings of its own owned rows.  Nothing is ever filled, and
  // every temporal block runs over exactly the owned rows, so an epoch is one
  // block (D = tmax, unless the configuration sets the epoch).
  // The rings are allocated here, before any geometry is committed: if the
  // backend cannot build them after all (address space, driver), the tile
  // falls back to plain buffers with periodic fills.
  int ring_dv = 0;
  Owned<> ring_bufs[2];
  if (dec_.Px == 1 && dec_.Py == 1 && !cfg_.self_exchange && !rows_wrapped_ && !plane_) {
    const TileGeom probe = TileGeom::make(cl, r.size(), c.size(), 0, hw);
    ring_dv = be_->row_ring_halo(probe.H, probe.pitch, tmax_);
    // The byte layout on bit words keeps its byte tiles too: the rings must
    // fit beside them (BASELINE config 5's share, 2 x 137 GB of bytes, has no
    // room for 2 x 17 GB of bit rings on a 288 GB GPU; its bit words then
    // live in the spare byte buffer with periodic fills).
    if (ring_dv > 0 && via_bits_) {
      const double bytes = 2.0 * double(TileGeom::make(cfg_.layout, r.size(), c.size(), 0, 0).bytes()) +
                           2.0 * double(TileGeom::make(cl, r.size(), c.size(), ring_dv, hw).bytes());
      if (bytes + double(size_t(1) << 31) > double(be_->mem_free())) ring_dv = 0;
    }
    if (ring_dv > 0) {
      const TileGeom gr = TileGeom::make(cl, r.size(), c.size(), ring_dv, hw);
      try {
        Owned<> tried[2];  // a ring that came before a failure goes with this scope
        for (auto& b : tried) {
          b = Owned<>(be_, be_->alloc_row_ring(gr));
          GOL_REQUIRE(b, "the backend returned no ring");
        }
        for (int i = 0; i < 2; ++i) ring_bufs[i] = std::move(tried[i]);
      } catch (const std::exception& e) {
        ring_dv = 0;
        ring_fallback_ = e.what();
        std::fprintf(stderr, "gol: WARNING: row ring unavailable (%s); periodic row fills instead\n", e.what());
      }
    }
  }
  if (via_bits_) {
    // The byte tile is storage only (owned cells, no halos); the epochs run
    // on its bit-word image, which carries the halos.
    g_ = TileGeom::make(cfg_.layout, r.size(), c.size(), 0, 0);
    gb_ = TileGeom::make(Layout::Bits, r.size(), c.size(), ring_dv > 0 ? ring_dv : D_, hw);
  } else {
    g_ = TileGeom::make(cfg_.layout, r.size(), c.size(), ring_dv > 0 ? ring_dv : D_, hw);
  }
  if (ring_dv > 0) {
    rows_ring_ = true;
    if (cfg_.epoch <= 0) D_ = tmax_;  // an epoch only paces the polls (and column fills) now
  }
  // Linked launches (Backend::KernelChoice::link): consecutive blocks of an
  // epoch overlap; anything else on the stream (fills, exchanges, polls)
  // joins the streams first.  Not with column fills between blocks.
  link_ = kc.link && !cols_filled_ && plain_;
  // Several ranks: every poll is a flag all-reduce on the compute stream
  // (latency-bound), so poll half as often; a stop is still exact and at most
  // two windows late.
  poll_gens_ = cfg_.poll_gens > 0 ? cfg_.poll_gens : (tr_->size() > 1 || cfg_.self_exchange) ? 512 : 256;
  // The rings are the compute tile's buffers (each owned once: moved).
  if (rows_ring_ && !via_bits_) {
    for (int i = 0; i < 2; ++i) buf_[i] = std::move(ring_bufs[i]);
  } else {
    for (auto& b : buf_) b = Owned<>(be_, be_->alloc(size_t(g_.bytes())));
  }
  if (via_bits_) {
    // The bit words live in the spare byte buffer (about an eighth of its
    // size per parity) unless a small tile's halo rows or pitch rounding do
    // not leave room, or they form a row ring.
    if (rows_ring_) {
      for (int i = 0; i < 2; ++i) bitbuf_[i] = std::move(ring_bufs[i]);
    } else if (2 * gb_.bytes() > g_.bytes()) {
      for (auto& b : bitbuf_) b = Owned<>(be_, be_->alloc(size_t(gb_.bytes())));
    }
  }
  alive_dev_ = Owned<uint32_t>(be_, be_->alloc(64));
  if (dec_.Px > 1) {
    const TileGeom& gc = compute_geom();  // the tile whose halos are exchanged
    size_t n = size_t(gc.span_bytes(32 * int64_t(gc.hw)) * gc.H);
    for (auto& b : colbuf_) b = Owned<>(be_, be_->alloc(n));
  }
  // Boundary-triggered sends (overlap = 3; last_block_trigger): row strips
  // on a backend that can count boundary groups done.  Byte tiles on bit
  // words too: the trigger runs on the bit image.
  // Plain engines only: the trigger rides on linked launches.
  const bool trigger_ok = row_exchange && dec_.Px == 1 && be_->supports_trigger() && plain_;
  trigger_ = trigger_ok && cfg_.overlap == 3;
  watchdog_s_ = cfg_.watchdog_s > 0 ? cfg_.watchdog_s : cfg_.tune.f("watchdog_s") > 0 ? cfg_.tune.f("watchdog_s") : 900.0;
  use_graphs_ = cfg_.graphs != 0 && be_->supports_graphs() && tr_->capturable() &&
                (cfg_.graphs > 0 || tr_->size() == 1) && plain_;
  if (use_graphs_) gen_dev_ = Owned<int64_t>(be_, be_->alloc(sizeof(int64_t)));
  if (use_graphs_) trigger_ = false;  // captured epochs stay on one stream
  // Overlap auto: measure both schedules on the real ranks (see auto_choose);
  // the one-GPU rehearsal has no xGMI latency in it, so on a multi-GPU node
  // the decision is taken from the node itself.
  auto_overlap_ = cfg_.overlap == -1 && trigger_ok && !use_graphs_;
  // Side polls: with a transport whose flag reduction has its own
  // communicator (RCCL), a poll's all-reduce and D2H copy run on the comm
  // stream after a mark on the compute stream, which never waits for them:
  // the reduction's latency leaves the critical path.  The halo exchanges
  // stay on the compute stream.
  // Opt-in (tuning side_poll=1): in the one-GPU RCCL rehearsal the cross-stream
  // hop cost ~10 us per poll, more than the 1-rank reduction it hides
  // (profiles/r02/side_poll_ab.jsonl); with 8 ranks the reduction is longer.
  // Single-rank poll copies on a side stream (poll_issue): a linked chain
  // continues across the poll (the rank tile's ring: 2.24 -> 2.17 ms per 1000
  // generations, 32768^2 -0.5 %), but with blocks of T <= 8 (8192^2, ~13 us
  // per linked block) it measured 5-10 % slower (profiles/r05/poll_side.jsonl).
  // Auto: deeper blocks only.
  const int pcs = cfg_.tune.i("poll_copy_side");
  poll_copy_side_ = pcs > 0 || (pcs < 0 && tmax_ > 8);
  // A single-rank device tile whose polls join the compute streams (T <= 8:
  // each join restarts the linked chain) polls every 1024 generations: 8192^2
  // 1.52 vs 1.62 ms per 1000 generations, 4096^2 1.20 vs 1.22 (medians of 8,
  // profiles/r06/poll_interval.jsonl).  A stop is still exact, and at most two
  // windows late.
  if (cfg_.poll_gens <= 0 && be_->is_device() && tr_->size() == 1 && !cfg_.self_exchange && !poll_copy_side_)
    poll_gens_ = 1024;
  // side_poll = -1 (default): after the overlap trial the ranks time both
  // poll placements (poll_trial_step) and keep the faster, as for overlap.
  const int sp = cfg_.tune.i("side_poll");
  const bool side_ok = tr_->side_reduce() && (be_->is_device() || cfg_.tune.on("cpu_side_poll")) && !use_graphs_ &&
                       (tr_->size() > 1 || cfg_.self_exchange);
  poll_side_ = side_ok && sp > 0 && !auto_overlap_;
  poll_trial_ = side_ok && sp < 0;
  // Quiet-tile skipping (gol/quiet.hpp): single-rank B3/S23 ring tiles in the
  // bit layout whose columns wrap, where every block covers exactly the owned
  // rows at the skipping kernel's block size (the tiles of a launch then form
  // a torus that is the same from block to block).  Everything else keeps
  // today's path.
  const Backend::QuietTuning qt = be_->quiet_mode();
  if (qt.mode != 0 && plain_ && cl == Layout::Bits && rule_is_default(cfg_.rule) && rows_ring_ && !cols_filled_ &&
      tr_->size() == 1 && !cfg_.self_exchange && !use_graphs_ && tmax_ == be_->quiet_block() && D_ == tmax_) {
    quiet_.mode = qt.mode;
    quiet_.scout = qt.scout;
    quiet_.on = qt.on;
    quiet_.off = qt.off;
    be_->quiet_prepare(compute_geom());
  }
  // Lazy tail (run_impl): single-rank ring tiles whose epochs are one block.
  tail_mode_ = cfg_.tune.i("lazy_tail");
  tail_ok_ = tail_mode_ != 0 && plain_ && rows_ring_ && D_ == tmax_ && tr_->size() == 1 && !cfg_.self_exchange &&
             !use_graphs_;
  if (tail_ok_) carry_ = Owned<uint32_t>(be_, be_->alloc(size_t(tmax_) * 4));
  gen_ = cfg_.start_gen;
}

void Engine::release_graphs() {
  for (auto& g : graph_) {
    if (g) be_->graph_destroy(g);
    g = nullptr;
  }
}

Engine::~Engine() {
  // Graphs and timing marks; the buffers go with their handles.
  release_graphs();
  otrial_.release();
  ptrial_.release();
  for (auto& sp : phase_spans_) {
    be_->timing_release(sp.a);
    be_->timing_release(sp.b);
  }
}

void Engine::load_cells(const uint8_t* cells, int64_t ld) {
  settle_pending(true);
  ahead_ = 0;          // a block chain ahead of gen_ goes with the old state
  bits_live_ = false;  // the byte tile is the state again
  be_->load_owned(buf_[cur_], g_, cells, ld);
  be_->synchronize();
  drift_ = 0;
}

void Engine::load_global(const uint8_t* grid, int64_t ld) {
  Extent r = rows(), c = cols();
  load_cells(grid + r.begin * ld + c.begin, ld);
}

void Engine::store_cells(uint8_t* cells, int64_t ld, bool ascii) {
  settle_pending(false);
  replay_tail();
  sync_bytes();
  normalize();
  be_->synchronize();
  be_->store_owned(buf_[cur_], g_, cells, ld, ascii);
}

void Engine::store_rows(uint8_t* cells, int64_t ld, int64_t r0, int64_t n, bool ascii) {
  GOL_REQUIRE(r0 >= 0 && n >= 0 && r0 + n <= g_.H, "store_rows: rows outside the tile");
  if (n == 0) return;
  settle_pending(false);
  replay_tail();
  sync_bytes();
  normalize();
  be_->synchronize();
  // A view of the band: the same pitch and halos, its first owned row at r0.
  TileGeom v = g_;
  v.H = n;
  be_->store_owned(static_cast<uint8_t*>(buf_[cur_].get()) + r0 * g_.pitch, v, cells, ld, ascii);
}

void Engine::init_random(uint64_t seed, double density) {
  settle_pending(true);
  ahead_ = 0;
  bits_live_ = false;
  be_->init_random(buf_[cur_], g_, seed, density, rows().begin, cols().begin);
  be_->synchronize();
  drift_ = 0;
}

void Engine::add_drift(int64_t cells) { drift_ = (drift_ + cells) % cfg_.W; }

void Engine::normalize() {
  replay_tail();
  sync_bytes();  // the rotation's target is the spare byte buffer, which holds the bit image
  if (drift_ == 0) return;
  settle_pending(true);  // the rotated copy has no halo rows
  be_->rotate_cols(buf_[cur_], buf_[cur_ ^ 1], g_, drift_);
  cur_ ^= 1;
  drift_ = 0;
}

int64_t Engine::alive_count() {
  replay_tail();
  be_->synchronize();
  const Tile s = state_tile();
  return be_->alive_count(s.cur(), s.g);
}

uint64_t Engine::fingerprint() {
  settle_pending(false);
  replay_tail();
  if (drift_ != 0) normalize();  // the fingerprint weighs every cell by its column
  const Tile s = state_tile();
  if (!fp_dev_) fp_dev_ = Owned<uint64_t>(be_, be_->alloc(8));
  be_->join_streams();
  be_->memset_async(fp_dev_, 0, 8);
  be_->fingerprint(s.cur(), s.g, rows().begin, cols().begin, fp_dev_);
  if (tr_->size() > 1) tr_->allreduce_sum_u64(fp_dev_, 1, be_->stream());
  be_->synchronize();
  uint64_t f = 0;
  be_->copy_d2h(&f, fp_dev_, 8);
  return f;
}

// ---- views --------------------------------------------------------------------
// Each prepares the grid like the existing call it resembles:
//   * settle_pending: a triggered halo exchange may still be writing the
//     buffers (invalidating it where the grid is about to change);
//   * replay_tail: a lazy tail left the block chain ahead of generation();
//   * sync_bytes: windows read and write the byte tile, so a live bit image is
//     unpacked first (density reads the image itself instead);
//   * normalize: coordinates are true ones, the stored frame may be drifted.
std::vector<uint64_t> Engine::density(int64_t bx, int64_t by) {
  GOL_REQUIRE(bx >= 1 && by >= 1, "density: block sizes must be at least 1");
  const int64_t nbx = ceil_div(cfg_.W, bx), nby = ceil_div(cfg_.H, by);
  const bool fits = nbx <= Backend::kDensityBlocksMax && nby <= Backend::kDensityBlocksMax &&
                    nbx * nby <= Backend::kDensityBlocksMax;
  std::vector<uint64_t> out(fits ? size_t(nbx * nby) : 0);  // too many: refused below, by name
  density(bx, by, out.data());
  return out;
}

void Engine::density(int64_t bx, int64_t by, uint64_t* out) {
  GOL_REQUIRE(bx >= 1 && by >= 1, "density: block sizes must be at least 1 (got " + std::to_string(by) + "x" +
                                      std::to_string(bx) + ")");
  const int64_t nbx = ceil_div(cfg_.W, bx), nby = ceil_div(cfg_.H, by);
  GOL_REQUIRE(nbx <= Backend::kDensityBlocksMax && nby <= Backend::kDensityBlocksMax &&
                  nbx * nby <= Backend::kDensityBlocksMax,
              "density: " + std::to_string(nby) + " x " + std::to_string(nbx) + " blocks of " + std::to_string(by) +
                  "x" + std::to_string(bx) + " cells are more than 2^24; use larger blocks");
  settle_pending(false);
  replay_tail();
  if (drift_ != 0) normalize();  // a block is a range of true columns
  const Tile s = state_tile();
  const size_t n = size_t(nbx * nby);
  if (!density_dev_ || density_len_ < n) {  // kept while it is large enough: a movie may alternate block sizes
    density_dev_.reset();
    density_host_.reset();
    density_dev_ = Owned<uint64_t>(be_, be_->alloc(n * 8));
    density_host_ = Owned<uint64_t>(be_, be_->alloc_host(n * 8), /*host=*/true);
    density_len_ = n;
  }
  be_->join_streams();
  be_->memset_async(density_dev_, 0, n * 8);
  be_->density(s.cur(), s.g, rows().begin, cols().begin, cfg_.H, cfg_.W, bx, by, density_dev_);
  if (tr_->size() > 1) tr_->allreduce_sum_u64(density_dev_, n, be_->stream());
  // Through the pinned mirror: a map of a few MiB copied straight into pageable
  // memory measured 20-30 ms per call (docs/PERFORMANCE.md).
  be_->copy_d2h_async_on(density_host_, density_dev_, n * 8, nullptr);
  be_->synchronize();
  std::copy(density_host_.get(), density_host_.get() + n, out);
}

void Engine::require_rect(const char* what, int64_t x, int64_t y, int64_t w, int64_t h) const {
  const std::string rect = "rectangle x=" + std::to_string(x) + " y=" + std::to_string(y) + " w=" + std::to_string(w) +
                           " h=" + std::to_string(h);
  GOL_REQUIRE(w >= 1 && h >= 1, std::string(what) + ": " + rect + " is empty");
  GOL_REQUIRE(x >= 0 && y >= 0 && w <= cfg_.W - x && h <= cfg_.H - y,
              std::string(what) + ": " + rect + " leaves the grid of " + std::to_string(cfg_.W) + " x " +
                  std::to_string(cfg_.H) + " cells (windows do not wrap)");
  GOL_REQUIRE(w <= Backend::kWindowCellsMax / h,
              std::string(what) + ": " + rect + " has more than 2^26 cells");
}

void Engine::store_window(int64_t x, int64_t y, int64_t w, int64_t h, uint8_t* cells, bool ascii) {
  require_rect("store_window", x, y, w, h);
  settle_pending(false);
  replay_tail();
  sync_bytes();
  normalize();
  be_->synchronize();
  if (tr_->size() == 1) {
    be_->store_window(buf_[cur_], g_, rows().begin, cols().begin, x, y, w, h, cells, ascii);
    return;
  }
  // The ranks' pieces are disjoint: each writes its own as 0/1 into a zeroed
  // window, and the sum over ranks (as 64-bit words) is the whole window.
  const size_t n = size_t(w * h), words = (n + 7) / 8;
  std::vector<uint8_t> mine(words * 8, 0);
  be_->store_window(buf_[cur_], g_, rows().begin, cols().begin, x, y, w, h, mine.data(), false);
  if (!window_dev_ || window_len_ != words) {
    window_dev_.reset();
    window_dev_ = Owned<uint64_t>(be_, be_->alloc(words * 8));
    window_len_ = words;
  }
  be_->copy_h2d(window_dev_, mine.data(), words * 8);
  tr_->allreduce_sum_u64(window_dev_, words, be_->stream());
  be_->synchronize();
  be_->copy_d2h(mine.data(), window_dev_, words * 8);
  const uint8_t base = ascii ? '0' : 0;
  for (size_t i = 0; i < n; ++i) cells[i] = uint8_t(base + mine[i]);
}

void Engine::place(int64_t x, int64_t y, int64_t w, int64_t h, const uint8_t* cells, int mode) {
  require_rect("place", x, y, w, h);
  GOL_REQUIRE(mode == Backend::kPlaceCopy || mode == Backend::kPlaceOr, "place: mode must be copy or or");
  // Like a load that keeps the rest of the grid: the byte tile becomes the
  // state (a run packs it again), no exchange stays pending, and every epoch
  // begins by exchanging or filling its halos (run_epoch), so none is assumed
  // valid across the write.
  settle_pending(true);
  replay_tail();
  sync_bytes();
  normalize();
  be_->place_window(buf_[cur_], g_, rows().begin, cols().begin, x, y, w, h, cells, mode);
  be_->quiet_invalidate();
  be_->synchronize();
}

// Whether the state tile differs from find_cycle's copy in any owned cell, on
// any rank.
bool Engine::differs_from_snapshot() {
  const Tile s = state_tile();
  be_->join_streams();
  be_->memset_async(alive_dev_, 0, 4);
  be_->tiles_differ(s.cur(), snap_.get(), s.g, alive_dev_);
  if (tr_->size() > 1) tr_->allreduce_max_u32(alive_dev_, 1, be_->stream());
  be_->synchronize();
  uint32_t differ = 0;
  be_->copy_d2h(&differ, alive_dev_, 4);
  return differ != 0;
}

CycleResult Engine::find_cycle(int64_t max_gens, int max_period, int64_t chunk) {
  GOL_REQUIRE(cfg_.fingerprint, "find_cycle needs fingerprint=1 (EngineConfig::fingerprint)");
  GOL_REQUIRE(max_period >= 1, "find_cycle: max_period must be at least 1");
  GOL_REQUIRE(chunk >= 0, "find_cycle: chunk must be >= 0");
  if (chunk == 0) chunk = 256;
  const int bits = cfg_.tune.i("cycle_match_bits");
  GOL_REQUIRE(bits >= 0 && bits <= 64, "cycle_match_bits must be 0..64");
  const uint64_t mask = bits >= 64 ? ~uint64_t(0) : (uint64_t(1) << bits) - 1;
  const auto t0 = std::chrono::steady_clock::now();
  CycleResult res;
  const int64_t g0 = gen_;
  // F[i]: the fingerprint of generation g0 + i.  Every rank holds the same
  // series, so every decision below is the same on every rank.
  std::vector<uint64_t> F{fingerprint()};
  const auto advance_to = [&](int64_t g, bool stop_early) {
    RunResult r = run_impl(g, stop_early);
    F.insert(F.end(), r.fingerprint.begin(), r.fingerprint.end());
    GOL_REQUIRE(int64_t(F.size()) == gen_ - g0 + 1, "find_cycle: the fingerprint series has a gap");
    return r;
  };
  const auto finish = [&](int64_t period, const char* why) {
    res.period = period;
    res.generation = gen_;
    res.stop_reason = why;
    // Backwards from the end of the series, on all 64 bits.
    int64_t e = int64_t(F.size()) - 1 - period;
    while (e > 0 && F[size_t(e - 1)] == F[size_t(e - 1 + period)]) --e;
    res.repeats_from = g0 + std::max<int64_t>(e, 0);
    res.fingerprint.assign(F.begin() + 1, F.end());
    res.loop_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return res;
  };
  int64_t floor = 0;  // index of the first generation that counts: the last failed confirmation's end
  while (gen_ < max_gens) {
    const RunResult r = advance_to(std::min(gen_ + chunk, max_gens), /*stop_early=*/true);
    // The change flags found grid(g) == grid(g - 1): exact, no confirmation.
    if (r.first_unchanged >= 0) return finish(1, r.extinct ? "extinction" : "cycle");
    const int64_t n = int64_t(F.size()) - 1;
    // A period needs p generations of history behind its p comparisons - except
    // with cycle_match_bits = 0, where a match is no evidence to wait for:
    // every period is a candidate at every search (tests: the rejection path).
    std::vector<int64_t> cand;
    for (int64_t p = 1; p <= max_period && (mask == 0 || n - 2 * p + 1 >= floor); ++p) {
      if (mask == 0) {
        cand.push_back(p);
        continue;
      }
      bool all = true;
      for (int64_t g = n; g > n - p && all; --g) all = ((F[size_t(g)] ^ F[size_t(g - p)]) & mask) == 0;
      if (all) cand.push_back(p);
    }
    if (cand.empty()) continue;
    // The candidates and their divisors, ascending: the minimal period
    // divides every period, so the first that compares equal is minimal.
    std::vector<int64_t> D;
    for (int64_t d = 1; d <= cand.back(); ++d)
      for (int64_t p : cand)
        if (p % d == 0) {
          D.push_back(d);
          break;
        }
    const int64_t G = gen_;
    if (G + D.back() > max_gens) continue;  // the limit comes first
    const Tile s = state_tile();
    const size_t bytes = size_t(s.g.bytes());
    if (!snap_ || snap_bytes_ < bytes) {
      snap_.reset();
      snap_ = Owned<>(be_, be_->alloc(bytes));
      snap_bytes_ = bytes;
    }
    be_->copy_owned_rows(snap_.get(), s.cur(), s.g);
    for (int64_t d : D) {
      advance_to(G + d, /*stop_early=*/false);
      if (!differs_from_snapshot()) {
        ++res.confirmations;
        return finish(d, "cycle");
      }
    }
    res.false_candidates += int64_t(cand.size());
    floor = int64_t(F.size()) - 1;
  }
  res.generation = gen_;
  res.fingerprint.assign(F.begin() + 1, F.end());
  res.loop_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return res;
}

int Engine::pick_T(int64_t remaining) const {
  if (rows_wrapped_) {  // the LDS-tiled byte kernels: T = 1, 2, 4, ... (powers of two)
    int t = 1;
    while (2 * t <= tmax_ && 2 * t <= remaining) t *= 2;
    return t;
  }
  for (int t : kTSizes)
    if (t <= tmax_ && t <= remaining) return t;
  return 1;
}

void Engine::fill(void* buf, const TileGeom& g, bool cols, bool rows) {
  void* t = phase_begin(nullptr);
  be_->fill_periodic(buf, g, cols, rows);
  phase_end(kFill, t, nullptr);
}

// Phase A of the halo exchange (halo_exchange_on) between ranks (Px > 1):
// west / east halo columns of the owned rows, packed into contiguous buffers
// (RCCL has no strided datatype, unlike the reference's MPI_Type_vector column).
void Engine::exchange_columns(void* buf, const TileGeom& g) {
  auto* base = static_cast<uint8_t*>(buf);
  const auto nb = neighbors();  // the plane: -1 on a side at the grid's edge, whose halo the kernels mask
  const int64_t H = g.H, pitch = g.pitch;
  void* t = phase_begin(nullptr);
  const int64_t halo = 32 * int64_t(g.hw);
  const int64_t span = g.span_bytes(halo);
  const int64_t r0 = g.row0();
  const bool west = nb[kWest] >= 0, east = nb[kEast] >= 0;
  if (west) be_->copy_2d_async(colbuf_[0], span, base + g.offset(r0, g.cell0()), pitch, span, H);
  if (east) be_->copy_2d_async(colbuf_[1], span, base + g.offset(r0, g.cell0() + g.W - halo), pitch, span, H);
  // Both operations of a pair go with their peer: with Px == 2 the torus's
  // west and east neighbour are one rank, and the plane keeps one of the two
  // pairs, matched in issue order as before.
  std::vector<P2POp> ops;
  if (west) ops.push_back({true, nb[kWest], colbuf_[0], size_t(span * H)});
  if (east) ops.push_back({false, nb[kEast], colbuf_[3], size_t(span * H)});
  if (east) ops.push_back({true, nb[kEast], colbuf_[1], size_t(span * H)});
  if (west) ops.push_back({false, nb[kWest], colbuf_[2], size_t(span * H)});
  if (!ops.empty()) tr_->exchange(ops, be_->stream());
  halo_bytes_ += (int64_t(west) + int64_t(east)) * span * H;
  if (west) be_->copy_2d_async(base + g.offset(r0, 0), pitch, colbuf_[2], span, span, H);
  if (east) be_->copy_2d_async(base + g.offset(r0, g.cell0() + g.W), pitch, colbuf_[3], span, span, H);
  phase_end(kHalo, t, nullptr);
}

// Two-phase halo exchange (columns, then full-width rows so the corner
// cells travel with the rows): 4 messages instead of the reference's 8
// per-generation messages with a strided MPI_Type_vector column
// (src/game_mpi.c:335-383).
void Engine::halo_exchange() {
  replay_tail();
  halo_exchange_on(buf_[cur_], g_);
}

void Engine::halo_exchange_on(void* buf, const TileGeom& g) {
  trace::Range tr("gol.halo_exchange");
  ++exchanges_;
  // Each direction's halos come from this tile's own periodic wrap (a fill,
  // or nothing where the kernels wrap their reads or the row halos alias the
  // owned rows: rows_wrapped_ and rows_ring_ are single-rank tiles) or from
  // the neighbours through the transport.
  const bool cols_local = dec_.Px == 1, rows_local = dec_.Py == 1 && !cfg_.self_exchange;
  // The plane fills nothing: what lies beyond the grid's edge is masked in
  // the kernels (BlockArgs::plane), so a single rank moves no data at all.
  const bool fill_cols = cols_local && cols_filled_ && !plane_;
  const bool fill_rows = rows_local && !rows_wrapped_ && !rows_ring_ && !plane_;
  // Nothing to move: no stream join either, so linked launches (GOL_LINK)
  // chain across such epochs.
  if (cols_local && rows_local && !fill_cols && !fill_rows) return;
  be_->join_streams();  // transports enqueue on the compute stream directly
  if (cols_local && rows_local) {  // one rank: its periodic fills in one launch
    fill(buf, g, fill_cols, fill_rows);
    return;
  }
  // Phase A: west/east halo columns of the owned rows.
  if (!cols_local)
    exchange_columns(buf, g);
  else if (fill_cols)
    fill(buf, g, /*cols=*/true, /*rows=*/false);
  // Phase B: north/south halo rows over the full padded width.
  if (rows_local) {
    if (fill_rows) fill(buf, g, /*cols=*/false, /*rows=*/true);
  } else {
    void* t = phase_begin(nullptr);
    const std::vector<P2POp> ops = row_ops(buf, g);
    if (!ops.empty()) tr_->exchange(ops, be_->stream());
    phase_end(kHalo, t, nullptr);
    halo_bytes_ += int64_t(ops.size() / 2) * g.Dv * g.pitch;
  }
}

// North / south halo rows over the full padded width, Dv rows each way.
std::vector<P2POp> Engine::row_ops(void* buf, const TileGeom& g) const {
  auto* base = static_cast<uint8_t*>(buf);
  const auto nb = neighbors();
  const int64_t Dv = g.Dv, H = g.H, pitch = g.pitch;
  const size_t bytes = size_t(Dv * pitch);
  const std::vector<P2POp> all = {
      {true, nb[kNorth], base + Dv * pitch, bytes},        // my top rows -> north's bottom halo
      {false, nb[kSouth], base + (Dv + H) * pitch, bytes},  // south's top rows -> my bottom halo
      {true, nb[kSouth], base + H * pitch, bytes},          // my bottom rows -> south's top halo
      {false, nb[kNorth], base, bytes},                     // north's bottom rows -> my top halo
  };
  std::vector<P2POp> ops;
  for (const P2POp& op : all)
    if (op.peer >= 0) ops.push_back(op);  // the plane: no partner beyond the grid's edge
  return ops;
}

void* Engine::bit_scratch(int i) const {
  if (bitbuf_[i]) return bitbuf_[i];
  return static_cast<uint8_t*>(buf_[cur_ ^ 1].get()) + i * gb_.bytes();
}

// The byte grid <-> its bit-word image in the spare byte buffer: a run packs
// the byte grid unless the image is already the state (bits_live_: the
// previous run's result, not unpacked since), and leaves its result in the
// image; the byte tile is brought up to date (sync_bytes) only when someone
// reads it or its buffers (read-out, bands, drift rotation, checkpoints, raw
// views), so back-to-back runs - bench.py's steps - pack and unpack once, not
// per run.  Loading or initialising the byte tile makes it the state again.
// A drifting bit kernel leaves the byte grid drifted by the same amount (a
// relabeling of columns, rotated out by normalize() like the bit layout's).
void Engine::sync_bytes() {
  replay_tail();  // the image at gen_, not at the spine
  if (!bits_live_) return;
  unpack_bits();
  bits_live_ = false;
}

void Engine::pack_bits() {
  bpar_ = 0;
  void* t = phase_begin(nullptr);
  be_->convert_rows(buf_[cur_], g_, bit_scratch(0), gb_, 0, g_.H);
  phase_end(kCompute, t, nullptr);
}

void Engine::unpack_bits() {
  void* t = phase_begin(nullptr);
  be_->convert_rows(bit_scratch(bpar_), gb_, buf_[cur_], g_, 0, g_.H);
  phase_end(kCompute, t, nullptr);
}

void Engine::run_epoch(int64_t d) {
  const bool sent_ahead = rows_pending_;
  // The previous epoch's last block sent this buffer's boundary rows
  // (stream-ordered before this epoch's first block).
  rows_pending_ = false;
  // The previous epoch ends here.
  if (auto_overlap_) auto_mark();
  // The halo exchange or fill and every temporal block run on the compute
  // tile.  For a byte tile on bit words that is its bit image (run_impl packs
  // the byte tile into it when a run starts; it is unpacked when the byte
  // tile is next read), whose per-generation flags are those of the same cells.
  std::optional<trace::Range> tr;
  if (via_bits_) tr.emplace("gol.epoch_via_bits");
  const Tile t = compute_tile();
  if (!sent_ahead) halo_exchange_on(t.cur(), t.g);
  // A partial epoch (d < D) needs only d halo rows: its trapezoid starts d
  // rows outside the owned rows, not D.
  const bool hot = trigger_ && send_next_ && d == D_;  // a full epoch of the trigger schedule
  int64_t a = D_ - d;
  while (d > 0) {
    const int T = pick_T(d);
    if (rows_ring_) a = t.g.Dv - T;  // every block covers exactly the owned rows
    const int64_t lo = a + T, hi = t.g.R() - a - T;
    if (hot && d == T)
      last_block_trigger(t.cur(), t.next(), t.g, T);
    else if (hot)
      hot_block(t.cur(), t.next(), t.g, T, lo, hi, d);
    else
      add_drift(launch(t.cur(), t.next(), t.g, T, lo, hi, gen_));
    t.par ^= 1;
    gen_ += T;
    a += T;
    d -= T;
  }
}

void Engine::settle_pending(bool invalidate) {
  if (!rows_pending_) return;
  be_->synchronize();
  if (invalidate) rows_pending_ = false;
}

// ---- lazy tail (tuning lazy_tail) -------------------------------------------
// A run whose last epoch is shorter than a block would finish on remainder
// blocks (pick_T: 1000 = 83 x 12 + 4): dense launches, after which the next
// run's first skipping block has no tile words to skip on and recomputes every
// tile.  Instead run_impl runs one ordinary full block there and reports its
// limit: gen_ = limit, while the block chain (the spine, gen_ + ahead_) is up
// to tmax - 1 generations further.  Nothing is lost: the block read one buffer
// and wrote the other, so its input - generation spine - tmax - is still
// there (on a row ring the halo rows are mappings of the owned rows), and the
// flags of (limit, spine] are on the device.
//   * The next run moves those flags to their new offsets (run_impl), advances
//     gen_ to min(limit, spine) with no launch and continues from the spine; a
//     stop inside the carried generations is found by its polls as any other.
//   * Anything that needs the grid at gen_ first rewinds to the block's input
//     and runs the remainder blocks after all (replay_tail), as a run without
//     lazy tails would have.
// Whether a run ends this way: tail_wanted().
bool Engine::tail_wanted() {
  if (!tail_ok_) return false;
  if (tail_mode_ > 0) return true;
  // Auto: where the full block is a skipping launch (about a quarter of the
  // remainder blocks' time on a settled grid, and it keeps the tile words
  // alive), unless the last one had to be replayed and the grid has been read
  // after every run since: such a caller would pay a wasted block per run.
  if (tail_hold_ || quiet_.mode == 0) return false;
  quiet_poll();
  return quiet_.mode > 0 || quiet_.skipping;
}

void Engine::replay_tail() {
  grid_read_ = true;
  if (ahead_ == 0) return;
  trace::Range tr("gol.replay_tail");
  const int64_t target = gen_;
  const Tile t = compute_tile();
  t.par ^= 1;  // the block's input is current again
  drift_ = tail_drift_;
  gen_ = target + ahead_ - tmax_;
  ahead_ = 0;
  no_flags_ = true;  // the run that reported these generations has their flags
  run_epoch(target - gen_);
  no_flags_ = false;
  ++tail_replays_;
  tail_hold_ = true;
}

// Trigger schedule (overlap = 3; Py > 1 or the one-rank RCCL rehearsal, Px
// == 1).  The reference exchanges halos and then waits (MPI_Startall +
// MPI_Waitall before evolve, src/game_mpi.c:392-403).  Here the last temporal
// block of a full epoch writes exactly the owned rows, and the next epoch's
// halos are the first and last Dv of them.  That block runs as one ordinary
// launch whose groups meeting those rows count themselves done on a device
// counter once their rows are written through.  With linked launches it runs
// on the second compute stream, and the first one - whose last work, the
// block before, is done - waits on the counter (Backend::trigger_stream) and
// sends the rows while the block's interior groups still run.  The next
// epoch's first block follows the exchange on that stream and links to the
// last block, so the chain is not restarted at the epoch boundary.  Nothing
// spins on the exchange: it is stream-ordered before the launch that reads
// the halo rows, and it waits only on work already running.  Measured on the
// one-GPU rehearsal: docs/PERFORMANCE.md.
void Engine::last_block_trigger(void* in, void* out, const TileGeom& g, int T) {
  trace::Range tr("gol.last_block_trigger");
  const int64_t Dv = g.Dv, H = g.H, pitch = g.pitch;
  const int64_t rows[4] = {Dv, 2 * Dv, H, H + Dv};
  add_drift(launch(in, out, g, T, Dv, Dv + H, gen_, rows));
  bool armed = false;
  void* s = be_->trigger_stream(&armed);  // not armed: after the whole block (a join)
  if (armed) ++triggered_sends_;
  if (cols_filled_) {  // column halos of the new rows (armed launches wrap their columns: never here)
    void* t = phase_begin(nullptr);
    be_->fill_cols_rows(out, g, Dv, H);
    phase_end(kFill, t, nullptr);
  }
  // Phase timing would join the streams (timing_mark): only when it is on.
  void* tx = phase_begin(s);
  tr_->exchange(row_ops(out, g), s ? s : be_->stream());
  phase_end(kHalo, tx, s);
  rows_pending_ = true;  // stream-ordered before the next block on the compute stream
  halo_bytes_ += 2 * Dv * pitch;
  ++exchanges_;
  ++boundary_sends_;
}

// An earlier block of a trigger epoch (d generations left before it): the
// groups in the light cone of the rows the epoch will send - the first and
// last Dv owned rows widened by the d - T generations still to come - run at
// top issue priority, so that region leads the interior and the last block's
// boundary groups finish ahead of the rest (last_block_trigger).
void Engine::hot_block(void* in, void* out, const TileGeom& g, int T, int64_t row_lo, int64_t row_hi, int64_t d) {
  const int64_t Dv = g.Dv, H = g.H, w = d - T;
  const int64_t rows[4] = {row_lo, 2 * Dv + w, H - w, row_hi};
  add_drift(launch(in, out, g, T, row_lo, row_hi, gen_, rows, /*hot_only=*/true));
}

int Engine::launch(void* in, void* out, const TileGeom& g, int T, int64_t row_lo, int64_t row_hi,
                   int64_t gen_base, const int64_t* trigger_rows, bool hot_only) {
  BlockArgs a;
  a.in = in;
  a.out = out;
  a.g = g;
  a.row_lo = row_lo;
  a.row_hi = row_hi;
  a.T = T;
  a.rule = cfg_.rule;
  a.gen_base = gen_base;
  if (capturing_) {
    // Replayable: the flags offset comes from gen_dev_ at run time.
    a.changed = flags_;
    a.gen_dev = gen_dev_;
    a.gen_rel = gen_base - epoch_start_ + 1;
  } else {
    a.changed = (flags_ && !no_flags_ && gen_base + T < flags_base_ + flags_len_ && gen_base >= flags_base_)
                    ? flags_.get()
                    : nullptr;
  }
  a.flags_base = flags_base_;
  for (const Series* s : {&census_, &fprint_}) {
    if (!s->run) continue;
    // Every block of a series' run lies in the window and records: a block
    // without flags (a lazy tail's replay) or beyond the window would lose or
    // double a generation of the series.  Its engines run no lazy tail and no
    // graphs, so neither arises.
    GOL_REQUIRE(!no_flags_ && !capturing_ && gen_base >= flags_base_ && gen_base + T < flags_base_ + flags_len_,
                std::string(s->name) + ": a temporal block outside the run's window");
    (s == &census_ ? a.census : a.fingerprint) = s->win.get();
  }
  if (fprint_.run) {
    a.global_row0 = rows().begin;
    a.global_col0 = cols().begin;
  }
  a.allow_drift = drift_ok_;
  a.full_width = dec_.Px == 1 && cfg_.W % 32 == 0 && !plane_;
  a.wrap_rows = rows_wrapped_;
  if (plane_) {
    // The grid's edge in this tile's padded coordinates; a side that borders
    // another rank's tile gets the tile's own bound, which masks nothing.
    const auto nb = neighbors();
    a.plane = true;
    a.grid_row_lo = nb[kNorth] < 0 ? g.Dv : 0;
    a.grid_row_hi = nb[kSouth] < 0 ? g.Dv + g.H : g.R();
    a.grid_cell_lo = nb[kWest] < 0 ? g.cell0() : 0;
    a.grid_cell_hi = nb[kEast] < 0 ? g.cell0() + g.W : 32 * g.Wp();
  }
  // Linked launches assume the device to themselves: not while transport
  // work may run beside them on the comm stream (side polls).  The trigger
  // schedule links: its sends start only once the boundary groups are done,
  // and the next epoch's first block follows them on the same stream.
  a.link = link_ && !poll_side_;
  if (trigger_rows) {
    a.trigger = !hot_only;
    a.hot = hot_only;
    for (int i = 0; i < 4; ++i) a.trigger_rows[i] = trigger_rows[i];
  }
  a.ring = rows_ring_;
  // Quiet-tile skipping: blocks of the skipping kernel's size over the owned
  // rows run it when the policy says so (on the DPP window: no drift, and the
  // drift accumulated so far stays where it is).  Any other block leaves the
  // next skipping block nothing to skip on (the backend sees to that).
  const bool quiet_size = quiet_.mode != 0 && !capturing_ && !trigger_rows && T == be_->quiet_block() &&
                          row_lo == g.Dv && row_hi == g.Dv + g.H;
  if (quiet_size) {
    quiet_poll();
    a.quiet = quiet_.next();
    if (a.quiet) {
      a.allow_drift = false;
      a.link = false;
    }
    quiet_.ran(a.quiet);
  }
  void* t = phase_begin(nullptr);
  const int drift = be_->run_block(a);
  phase_end(kCompute, t, nullptr);
  ++launches_;
  return drift;
}

// The newest report of the skipping kernel the device has published (host-
// mapped words: no synchronisation): feeds the policy, once per launch.
void Engine::quiet_poll() {
  int64_t seq = 0, tiles = 0, clean = 0, skipped = 0;
  if (!be_->quiet_report(&seq, &tiles, &clean, &skipped)) return;
  quiet_skipped_tiles_ = skipped;
  if (seq == quiet_seq_seen_) return;
  quiet_seq_seen_ = seq;
  quiet_.report(tiles, clean);
}

int64_t Engine::quiet_waves_skipped() {
  quiet_poll();
  return quiet_skipped_tiles_ * be_->quiet_tile_waves();
}

void Engine::step_block(int T, int64_t row_lo, int64_t row_hi) {
  GOL_REQUIRE(!via_bits_, "step_block: the byte tile has no halos when it computes on bit words (u8_compute)");
  replay_tail();
  add_drift(launch(buf_[cur_], buf_[cur_ ^ 1], g_, T, row_lo, row_hi, gen_));
  cur_ ^= 1;
  gen_ += T;
}

// Termination polls.  poll_issue() reduces the flags of generations
// (from, to] over ranks (MAX == logical OR) and starts their copy to the
// pinned mirror; poll_check() waits for that copy and scans it.  With lagged
// polling a window is checked only when the next one has been issued, by
// which time the device has long passed it, so the host never drains the
// queue; stopping up to one window late is exact because both stop
// conditions are absorbing.
Engine::Poll Engine::poll_issue(int64_t from, int64_t to) {
  Poll p;
  p.from = from;
  p.to = to;
  const int64_t n = to - from;
  if (n <= 0) return p;
  uint32_t* dev = flags_ + flag_offset(from);
  // A side stream that waits for the compute streams' tails without joining
  // them: side polls (the reduction on the flags communicator), and on one
  // rank the copy alone (nothing to reduce, poll_copy_side_) - a linked chain
  // then continues across the poll instead of restarting behind a join (a
  // join, the copy and the restart left the GPU idle ~20 us per poll).
  // Phase timing keeps the compute-stream path (it times the reduction there).
  void* side = nullptr;
  if (poll_side_ || (tr_->size() == 1 && !cfg_.self_exchange && !phase_timing_ && poll_copy_side_))
    side = be_->poll_side();
  if (side) {
    polled_side_ = true;
    void* t = phase_begin(side);
    // The one-rank RCCL rehearsal reduces too, through its 1-rank communicator.
    if (tr_->size() > 1 || cfg_.self_exchange) tr_->allreduce_max_u32(dev, size_t(n), side);
    be_->copy_d2h_async_on(flags_host_ + flag_offset(from), dev, size_t(n) * sizeof(uint32_t), side);
    phase_end(kReduce, t, side);
    p.ev = be_->event_record_on(side);
    ++polls_;
    return p;
  }
  be_->join_streams();  // transports enqueue on the compute stream directly
  void* t = phase_begin(nullptr);
  if (tr_->size() > 1) tr_->allreduce_max_u32(dev, size_t(n), be_->stream());
  be_->copy_d2h_async_on(flags_host_ + flag_offset(from), dev, size_t(n) * sizeof(uint32_t), nullptr);
  phase_end(kReduce, t, nullptr);
  p.ev = be_->event_record_on(nullptr);
  ++polls_;
  return p;
}

bool Engine::poll_check(Poll& p, int64_t* first_unchanged) {
  if (p.to <= p.from) return false;
  if (!be_->event_query(p.ev)) {
    // Watchdog: poll instead of blocking, check the communicator, and fail
    // with a message rather than hang forever on a dead peer or kernel.
    trace::Range tr("gol.poll_wait");
    const auto t0 = std::chrono::steady_clock::now();
    while (!be_->event_query(p.ev)) {
      tr_->check_health();
      const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
      if (s > watchdog_s_)
        fail("watchdog: generation " + std::to_string(p.to) + " not reached after " + std::to_string(s) +
             " s (GOL_WATCHDOG_S); a rank or kernel is stuck");
      // Fine-grained while the wait is short (the last poll of a run waits
      // for the run's last blocks: a coarse sleep there idles the GPU before
      // the next run), coarser later.
      // Spin (yield) for the first 2 ms: a sleep overshoots by the kernel's
      // timer slack (~50 us), which idled the GPU at every run boundary.
      if (s < 0.002)
        std::this_thread::yield();
      else
        std::this_thread::sleep_for(std::chrono::microseconds(s < 0.05 ? 20 : 500));
    }
  }
  be_->event_wait(p.ev);
  be_->event_destroy(p.ev);
  p.ev = nullptr;
  be_->check_device_errors();
  const uint32_t* h = flags_host_ + flag_offset(p.from);
  for (int64_t i = 0; i < p.to - p.from; ++i)
    if (h[i] == 0) {
      *first_unchanged = p.from + 1 + i;
      return true;
    }
  return false;
}

int64_t reported_generations(int64_t first_unchanged, bool extinct, int64_t limit, int64_t start_gen,
                             bool check_similarity, int sim_freq, int sim_phase, std::string* reason) {
  std::string why = "limit";
  int64_t gens = limit;
  if (first_unchanged >= 0 && first_unchanged <= limit) {
    why = "fixed_point";
    if (extinct) {
      // G_{g_f - 1} is the first empty grid: the loop's emptiness test stops
      // at the next iteration and reports g_f - 1 (src/game.c:177).
      gens = first_unchanged - 1;
      why = "extinction";
    } else if (check_similarity) {
      // Similarity checks happen at generations t > start_gen with
      // (t - start_gen + sim_phase) % F == 0 (counter reset only on a failed
      // check, src/game.c:181-189); the first one at or after g_f fires and
      // reports t - 1 (the break skips generation++).  The phase is anchored
      // at the configured start generation, so an earlier advance() or
      // run_until() on the same engine does not shift it.
      const int64_t F = sim_freq;
      const int64_t k = first_unchanged - start_gen + sim_phase;
      const int64_t tsim = first_unchanged + ((F - (k % F)) % F);
      if (tsim <= limit) {
        gens = tsim - 1;
        why = "similarity";
      }
    }
  }
  if (reason) *reason = why;
  return gens;
}

RunResult Engine::run() { return run_impl(cfg_.gen_limit, /*stop_early=*/true); }

RunResult Engine::run_until(int64_t limit) {
  return run_impl(std::min(limit, cfg_.gen_limit), /*stop_early=*/true);
}

RunResult Engine::advance(int64_t n) { return run_impl(gen_ + n, /*stop_early=*/false); }

RunResult Engine::run_impl(int64_t limit, bool stop_early) {
  RunResult res;
  const int64_t start = gen_;
  if (limit < start) limit = start;
  // Lazy tail, auto: a caller that read the grid after a replayed block and
  // after every run since keeps the remainder blocks.
  if (!grid_read_) tail_hold_ = false;
  grid_read_ = false;
  // (Re)allocate per-generation flags for (start, limit], and for the full
  // block a lazy tail may end the run on.
  const int64_t need = limit - start + 2 + (tail_ok_ ? tmax_ : 0);
  // The flags of the generations the block chain is ahead, (start, start +
  // ahead_], were recorded at the last run's offsets: staged through carry_
  // around the reset, stream-ordered (no host round trip between two runs).
  const int64_t carried = ahead_;
  if (carried > 0) {
    be_->join_streams();
    be_->copy_2d_async(carry_, carried * 4, flags_ + flag_offset(start), carried * 4, carried * 4, 1);
  }
  if (!flags_ || flags_len_ < need) {
    if (carried > 0) be_->synchronize();  // the copy reads the buffer that goes
    flags_.reset();
    flags_host_.reset();
    flags_len_ = std::max<int64_t>(need, 64);
    flags_ = Owned<uint32_t>(be_, be_->alloc(size_t(flags_len_) * 4));
    flags_host_ = Owned<uint32_t>(be_, be_->alloc_host(size_t(flags_len_) * 4), /*host=*/true);
    for (Series* s : {&census_, &fprint_}) s->win.reset();  // below: their length is the flags'
  }
  flags_base_ = start;
  be_->memset_async(flags_, 0, size_t(flags_len_) * 4);
  GOL_REQUIRE(!census_.on || ahead_ == 0, "census: a lazy tail is pending");
  GOL_REQUIRE(!fprint_.on || (ahead_ == 0 && drift_ == 0), "fingerprint: a lazy tail or a drifted frame is pending");
  struct SeriesRunEnd {  // also when the run throws
    Engine* e;
    ~SeriesRunEnd() { e->census_.run = e->fprint_.run = false; }
  } series_run_end{this};
  for (Series* s : {&census_, &fprint_}) {
    if (!s->on) continue;
    if (!s->win) s->win = Owned<uint64_t>(be_, be_->alloc(size_t(flags_len_) * 8));
    be_->memset_async(s->win, 0, size_t(flags_len_) * 8);
    s->run = true;
  }
  if (carried > 0)
    be_->copy_2d_async(flags_ + flag_offset(start), carried * 4, carry_.get(), carried * 4, carried * 4, 1);
  if (use_graphs_) {
    if (graph_flags_ != flags_) release_graphs();  // kernel arguments point at the flags
    graph_flags_ = flags_;
    be_->i64_async(gen_dev_, 0, /*add=*/false);  // first epoch starts at flags_base_
  }
  const int64_t g0 = graph_runs_;
  const int64_t e0 = exchanges_, p0 = polls_, l0 = launches_, hb0 = halo_bytes_, es0 = boundary_sends_;
  const int64_t lk0 = be_->linked_launches();
  trace::Range trace_run("gol.run");
  if (cfg_.timing_barriers) {
    settle_pending(false);  // one stream at a time on the communicator
    tr_->barrier();
    be_->synchronize();
  }
  // Without timing barriers (a caller that brackets the run itself, bench.py)
  // the flag reset stays queued ahead of the first block: no host round trip
  // between two runs (8192^2: ~2 % of a 1000-generation run).
  auto t0 = std::chrono::steady_clock::now();
  if (via_bits_ && !bits_live_) pack_bits();

  int64_t checked = start, found = -1;
  const int64_t poll_epochs = std::max<int64_t>(1, poll_gens_ / D_);
  int64_t epoch = 0;
  Poll pending;
  bool have_pending = false;
  while (gen_ < limit) {
    const int64_t d = std::min<int64_t>(D_, limit - gen_);
    send_next_ = gen_ + d < limit;
    if (ahead_ > 0) {
      // Generations the block chain has reached already (lazy tail): no
      // launch; their flags are in the window, polled like any others.
      const int64_t k = std::min(ahead_, limit - gen_);
      gen_ += k;
      ahead_ -= k;
    } else if (d < D_ && tail_wanted()) {
      // Lazy tail: one full block from the spine instead of the remainder
      // blocks; the generations beyond the limit belong to the next run.
      GOL_REQUIRE(gen_ + tmax_ < flags_base_ + flags_len_, "lazy tail: flag window too short");
      tail_drift_ = drift_;
      run_epoch(D_);
      ahead_ = gen_ - limit;
      gen_ = limit;
      ++tail_overshoots_;
    } else if (use_graphs_ && d == D_) {
      // Full epochs replay a captured graph; the only per-epoch input is the
      // device generation offset, advanced by the graph itself.  Graphs are
      // keyed by the parity of the buffer pair the epochs alternate over and
      // by the addresses baked into them (graph_key).
      int& cur = compute_tile().par;
      const int par = graph_key();
      if (!graph_[par]) {
        const int64_t k0 = launches_;
        const int64_t dr0 = drift_;
        capturing_ = true;
        epoch_start_ = gen_;
        be_->capture_begin();
        run_epoch(d);
        be_->i64_async(gen_dev_, D_, /*add=*/true);
        graph_[par] = be_->capture_end();
        capturing_ = false;
        graph_flip_[par] = cur ^ (par & 1);
        graph_kernels_[par] = launches_ - k0;
        graph_drift_[par] = ((drift_ - dr0) % cfg_.W + cfg_.W) % cfg_.W;
        be_->graph_launch(graph_[par]);  // capture only recorded it
      } else {
        be_->graph_launch(graph_[par]);
        cur ^= graph_flip_[par];
        add_drift(graph_drift_[par]);
        gen_ += D_;
        ++exchanges_;
        launches_ += graph_kernels_[par];
      }
      ++graph_runs_;
    } else {
      if (use_graphs_) be_->i64_async(gen_dev_, d, /*add=*/true);  // keep the offset in step
      if (auto_overlap_) auto_choose(d == D_ && send_next_);
      run_epoch(d);
    }
    ++epoch;
    if (stop_early && (epoch % poll_epochs == 0 || gen_ == limit)) {
      if (poll_trial_) poll_trial_step();
      Poll p = poll_issue(checked, gen_);
      checked = gen_;
      if (have_pending && poll_check(pending, &found)) {
        have_pending = false;
        if (p.ev) be_->event_destroy(p.ev);
        break;
      }
      pending = p;
      have_pending = true;
      if (!cfg_.lagged_poll || gen_ == limit) {
        have_pending = false;
        if (poll_check(pending, &found)) break;
      }
    }
  }
  if (have_pending) poll_check(pending, &found);
  census_.run = fprint_.run = false;
  if (via_bits_) bits_live_ = true;  // unpacked when the byte tile is next read (sync_bytes)
  // A poll issued just before an early stop may still run on the side stream
  // (the final alive reduction below uses the same communicator, and the
  // next run may reallocate the flags it reads).
  if (polled_side_) be_->synchronize_stream(be_->comm_stream());
  polled_side_ = false;
  be_->synchronize();
  be_->check_device_errors();
  otrial_.drop_open();  // an auto-trial epoch span does not continue into the next run
  ptrial_.drop_open();  // nor does a poll-trial window
  if (cfg_.timing_barriers) {
    settle_pending(false);
    tr_->barrier();
  }
  auto t1 = std::chrono::steady_clock::now();
  res.loop_ms = std::chrono::duration<double, std::milli>(t1 - t0).count();
  res.executed = gen_ - start;
  res.exchanges = exchanges_ - e0;
  res.polls = polls_ - p0;
  res.kernel_launches = launches_ - l0;
  res.overlapped = boundary_sends_ > es0;
  res.graph_launches = graph_runs_ - g0;
  res.halo_bytes = halo_bytes_ - hb0;
  res.linked_launches = be_->linked_launches() - lk0;
  res.generations = limit;
  collect_phases(res);
  // A series of (start, gen_]: summed over ranks (a fingerprint's shares add up
  // modulo 2^64) and copied once per run into its 64-bit entries.  (A stop
  // leaves gen_ at the last generation evaluated, and every generation up to
  // it was recorded.)
  const auto collect = [&](const Series& s, auto& out) {
    const int64_t n = gen_ - start;
    if (!s.on) return;
    out.resize(static_cast<size_t>(n));
    if (n <= 0) return;
    uint64_t* dev = s.win + flag_offset(start);
    if (tr_->size() > 1) tr_->allreduce_sum_u64(dev, size_t(n), be_->stream());
    be_->synchronize();
    be_->copy_d2h(out.data(), dev, size_t(n) * 8);
  };
  collect(census_, res.population);
  collect(fprint_, res.fingerprint);
  if (found >= 0) {
    res.first_unchanged = found;
    const Tile s = state_tile();
    be_->alive_any(s.cur(), s.g, alive_dev_);
    if (tr_->size() > 1) tr_->allreduce_max_u32(alive_dev_, 1, be_->stream());
    uint32_t alive = 0;
    be_->copy_d2h(&alive, alive_dev_, 4);
    res.extinct = !alive;
    res.generations = reported_generations(found, res.extinct, limit, cfg_.start_gen, cfg_.check_similarity,
                                           cfg_.sim_freq, cfg_.sim_phase, &res.stop_reason);
  }
  return res;
}

// ---- overlap auto trial ---------------------------------------------------
// The schedule of each full epoch is a function of the epoch count only, so
// every rank runs the same sequence, reaches the decision at the same epoch
// and issues the decision's all-reduce at the same point of its operation
// stream (RCCL matches operations by issue order).
void Engine::auto_choose(bool full_epoch) {
  int sched = 0;
  int trial = -1;
  if (full_epoch) {
    const int64_t i = auto_full_epochs_++;
    if (i >= kAutoWarm) {
      sched = ((i - kAutoWarm) % 2 == 0) ? 1 : 0;
      trial = sched;
    }
  }
  trigger_ = sched == 1;
  auto_sched_ = trial;
}

void Engine::auto_mark() {
  otrial_.close();
  if (otrial_.full(0) && otrial_.full(1)) {
    auto_decide();
    return;
  }
  otrial_.begin(auto_sched_);
}

// ---- trial bookkeeping ------------------------------------------------------
void Engine::Trial::close() {
  if (!open) return;
  void* end = be->timing_mark(nullptr);
  if (slot >= 0) {
    spans.push_back({slot, open, end});
    ++counts[slot];
  } else {
    be->timing_release(open);
    be->timing_release(end);
  }
  open = nullptr;
}

bool Engine::Trial::full(int s) const { return counts[s] >= kAutoTrials; }

void Engine::Trial::medians(Transport* tr, uint32_t* dev, double out[2]) {
  std::vector<double> ms[2];
  for (auto& sp : spans) {
    ms[sp.kind].push_back(be->timing_ms(sp.a, sp.b));
    be->timing_release(sp.a);
    be->timing_release(sp.b);
  }
  spans.clear();
  uint32_t v[2];
  for (int k = 0; k < 2; ++k) {
    std::sort(ms[k].begin(), ms[k].end());
    const double med = ms[k].empty() ? 0.0 : ms[k][ms[k].size() / 2];
    v[k] = uint32_t(std::min(4.0e9, std::max(0.0, med * 1e4)));  // 0.1 us units
  }
  be->copy_h2d(dev, v, sizeof(v));
  if (tr->size() > 1) tr->allreduce_max_u32(dev, 2, be->stream());
  be->copy_d2h(v, dev, sizeof(v));
  out[0] = v[0] * 1e-4;
  out[1] = v[1] * 1e-4;
}

void Engine::Trial::drop_open() {
  if (open) be->timing_release(open);
  open = nullptr;
}

void Engine::Trial::release() {
  for (auto& sp : spans) {
    be->timing_release(sp.a);
    be->timing_release(sp.b);
  }
  spans.clear();
  drop_open();
}

// Poll placement trial (tuning side_poll = -1).  Once the overlap trial has
// decided (and where polls do not ride the comm stream with the exchanges),
// the poll windows - from one termination poll to the next - alternate a
// poll whose flag all-reduce joins the compute stream and one that runs on a
// side stream through the transport's flags communicator (poll_side_, which
// also leaves linked launches off for that window: transport work may run
// beside them), after two warm-up windows; each window is timed from its
// poll's issue to the next's on the compute stream, and when kAutoTrials of
// each are in, at the same poll on every rank, the medians are MAX-reduced
// and every rank keeps the faster placement.  A side decision is then
// checked on kAutoTrials consecutive side windows (after one warm-up) and
// kept only if their median still beats the joined median: windows that
// alternate with joined ones can time faster than a run of side windows (the
// rehearsed rank tiles with the second linked stream on its own queue: side
// chosen, then 2x slower).  The reference all-reduces every generation on
// the critical path (src/game_mpi_collective.c:70-109).
void Engine::poll_trial_step() {
  if (auto_overlap_) return;  // the overlap trial runs first
  uint32_t* scratch = alive_dev_ + 4;
  ptrial_.close();
  if (!ptrial_verify_ && ptrial_.full(0) && ptrial_.full(1)) {
    ptrial_.medians(tr_, scratch, poll_ms_);
    if (poll_ms_[1] < 0.98 * poll_ms_[0]) {  // side wins the alternation: check a run of side windows
      ptrial_verify_ = true;
      ptrial_.counts[0] = ptrial_.counts[1] = 0;
      ptrial_polls_ = 0;
    } else {
      poll_side_ = false;
      poll_trial_ = false;
      poll_decided_ = true;
      return;
    }
  } else if (ptrial_verify_ && ptrial_.full(1)) {
    double v[2];
    ptrial_.medians(tr_, scratch, v);
    poll_side_steady_ms_ = v[1];
    poll_side_ = v[1] < poll_ms_[0];
    poll_trial_ = false;
    poll_decided_ = true;
    return;
  }
  const int64_t i = ptrial_polls_++;
  int mode;  // placement of the window that opens here: 0 joined, 1 side, -1 warm-up
  if (ptrial_verify_)
    mode = i < 1 ? -1 : 1;
  else
    mode = i < kAutoWarm ? -1 : int((i - kAutoWarm) % 2);
  poll_side_ = ptrial_verify_ || mode == 1;
  ptrial_.begin(mode);
}

std::string Engine::poll_mode() const {
  if (poll_trial_) return "auto:trial";
  if (poll_decided_) return poll_side_ ? "auto:side" : "auto:joined";
  return poll_side_ ? "side" : "joined";
}

void Engine::auto_decide() {
  // Slowest rank decides: every rank ends up with the same MAX values.
  otrial_.medians(tr_, alive_dev_ + 4, auto_ms_);
  const double v[2] = {auto_ms_[0], auto_ms_[1]};
  bool alt = v[1] < 0.98 * v[0];
  const std::string& forced = cfg_.tune.s("overlap_auto");  // fault injection (tests)
  GOL_REQUIRE(forced.empty() || forced == "plain" || forced == "trigger",
              "tuning overlap_auto=" + forced + ": plain or trigger");
  if (!forced.empty()) alt = forced == "trigger";
  trigger_ = alt;
  auto_overlap_ = false;
  auto_decided_ = true;
}

std::string Engine::overlap_mode() const {
  if (cfg_.overlap == 3) return trigger_ ? "trigger" : "off";
  if (cfg_.overlap == -1) {
    if (auto_overlap_) return "auto:trial";
    if (auto_decided_) return trigger_ ? "auto:trigger" : "auto:plain";
  }
  return "off";
}

// ---- phase timing -----------------------------------------------------------
void* Engine::phase_begin(void* stream) {
  if (!phase_timing_ || capturing_ || phase_spans_.size() >= kMaxPhaseSpans) return nullptr;
  return be_->timing_mark(stream);
}

void Engine::phase_end(int phase, void* a, void* stream) {
  if (!a) return;
  phase_spans_.push_back({phase, a, be_->timing_mark(stream)});
}

void Engine::collect_phases(RunResult& res) {
  if (!phase_timing_) return;
  double ms[kPhases] = {0, 0, 0, 0};
  for (auto& sp : phase_spans_) {
    ms[sp.kind] += be_->timing_ms(sp.a, sp.b);
    be_->timing_release(sp.a);
    be_->timing_release(sp.b);
  }
  phase_spans_.clear();
  res.phase_timed = true;
  res.compute_ms = ms[kCompute];
  res.halo_ms = ms[kHalo];
  res.fill_ms = ms[kFill];
  res.allreduce_ms = ms[kReduce];
}

}  // namespace gol
