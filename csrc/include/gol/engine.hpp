// The generation engine: one rank's tile, its double buffer, the epoch /
// temporal-block schedule, halo exchange and lazy exact termination.
//
// Reference loops: serial src/game.c:169-196, MPI src/game_mpi.c:385-422,
// CUDA src/game_cuda.cu:213-276.  All of them test termination every
// generation (a full scan + MPI_Allreduce, or a kernel + 4-byte D2H copy).
// Both stop conditions are absorbing: an empty grid stays
// empty (for every rule without B0, which is why B0 rules are refused) and
// G_t == G_{t-1} implies G_{t+k} == G_t (for any rule).  So the kernels record
// one "changed" flag per generation, the engine polls them every few hundred
// generations, and the reference's reported generation count is rebuilt
// exactly from the first unchanged generation g_f:
//   * grid at g_f empty   -> extinction, reports g_f - 1 (src/game.c:177)
//   * otherwise, with similarity checks every F gens -> the first check
//     t >= g_f reports t - 1 (the break skips generation++, src/game.c:186)
//   * otherwise -> GEN_LIMIT.
#pragma once

#include <memory>
#include <string>
#include <vector>

#include "gol/backend.hpp"
#include "gol/decomp.hpp"
#include "gol/quiet.hpp"
#include "gol/tile.hpp"
#include "gol/transport.hpp"

namespace gol {

struct EngineConfig {
  int64_t W = 0, H = 0;            // global grid (cells)
  Layout layout = Layout::Bits;
  Rule rule;                       // Life-like rule (common.hpp), default B3/S23; no B0
  // Torus (default) or the bounded plane, whose outside is dead in every
  // generation.  On the plane the edge is enforced inside the temporal blocks
  // (BlockArgs::plane), and everything that relies on the wrap is off: no row
  // ring, no wrapped rows or columns, no drifting frame, no folded strip, no
  // linked or chained launches, no quiet-tile skipping, no lazy tail, no
  // periodic fills; ranks exchange halos only across edges between ranks.
  Boundary boundary = Boundary::Torus;
  // Population census: every run also returns the number of live cells of
  // every generation it advanced through (RunResult::population), counted
  // inside the temporal blocks (BlockArgs::census) and summed over ranks.  Off
  // by default, and nothing changes when off.  A census engine runs no linked
  // or chained launches, no quiet-tile skipping, no lazy tail, no boundary
  // trigger and no graphs.
  bool census = false;
  // Grid fingerprint (gol/fingerprint.hpp): every run also returns a
  // position-dependent 64-bit fingerprint of every generation it advanced
  // through (RunResult::fingerprint), accumulated inside the temporal blocks
  // (BlockArgs::fingerprint) and summed over ranks modulo 2^64; the series
  // Engine::find_cycle searches.  Off by default, and nothing changes when
  // off.  A fingerprint engine is scheduled exactly like a census engine.
  bool fingerprint = false;
  std::string decomp = "auto";     // "auto" or "PxQ"
  int64_t gen_limit = 1000;        // GEN_LIMIT (src/game.c:6)
  bool check_similarity = true;    // CHECK_SIMILARITY (src/game.c:8)
  int sim_freq = 3;                // SIMILARITY_FREQUENCY (src/game.c:9)
  int64_t start_gen = 0;           // generation number of the loaded state (resume)
  int sim_phase = 0;               // similarity counter value at start_gen (resume)
  int tmax = 0;                    // max generations per kernel launch (0 = backend default)
  int epoch = 0;                   // generations per halo exchange (0 = auto)
  int poll_gens = 0;               // generations between termination polls (0 = auto)
  // Overlap the epoch's halo exchange with compute (row strips, Px == 1):
  //    3 trigger (1 on is the same): the last temporal block of a full epoch runs as usual, but
  //      its boundary groups count themselves done on a device counter; with
  //      linked launches that block runs on the second compute stream, and
  //      the first one - idle once the block before it is done - waits on the
  //      counter (Backend::trigger_stream) and sends the new boundary rows
  //      while the block's interior groups still run; the next epoch's first
  //      block follows the exchange on that stream and still links to the
  //      last block, so the chain runs through the epoch boundary.  No dual
  //      launch, no spinning consumer, no comm-stream hop; byte tiles on bit
  //      words included.  (Rounds 1-5 also had an early-boundary schedule - a
  //      dual launch of the boundary strips on the comm stream - and an edge-
  //      strip schedule; both measured slower and were removed, docs/HISTORY.md);
  //    0 off: everything on the compute stream;
  //   -1 auto: where the trigger schedule applies (row strips on a backend
  //      that supports it), the first epochs alternate it with the plain
  //      schedule, every rank times them with events, the per-epoch medians
  //      are MAX-reduced over ranks, and all ranks keep the faster one
  //      (GOL_OVERLAP_AUTO=plain|trigger forces the outcome after the trial,
  //      for tests); elsewhere as off.
  int overlap = -1;
  // Check each termination poll one poll window later, so the host never
  // drains the device queue (stops are absorbing, so running past is exact).
  bool lagged_poll = true;
  // Replay full epochs as captured HIP graphs (one per buffer parity):
  // -1 auto (single rank on a graph-capable backend), 0 off, 1 whenever the
  // backend and transport allow it.  Off by default: on ROCm 7 / MI355X the
  // replayed epochs measured 2-50% slower than stream launches
  // (profiles/sweep_graphs.jsonl); the host is never the bottleneck here.
  int graphs = 0;
  // Watchdog: fail (instead of hanging) when a termination poll waits on the
  // device longer than this many seconds (0: GOL_WATCHDOG_S or 900 s).
  double watchdog_s = 0;
  // Bracket each run's generation loop with a transport barrier (plus a
  // device sync) so loop_ms covers every rank's loop - the reference times
  // rank 0 only, with no barrier (src/game_mpi.c:385-424).  A caller that
  // brackets the run itself (bench.py) turns them off.
  bool timing_barriers = true;
  // Rehearsal of a multi-rank row-strip schedule on one rank: the north /
  // south halos go through the transport (a 1-rank RCCL communicator sending
  // to itself) instead of the local periodic fill, with the multi-rank epoch
  // depth and overlap.  Results are identical (the torus wraps to self).
  bool self_exchange = false;
  // Compute representation of the byte layout (width % 32 == 0):
  //    1 bits: the byte-per-cell grid stays the storage (load / store / read-
  //      out / drift rotation / alive count / checkpoints), but each run packs
  //      the owned rows into bit words inside the spare byte buffer, its
  //      epochs exchange or fill the halos there (8x fewer bytes) and run the
  //      bit-sliced temporal blocks, and the run ends by unpacking the owned
  //      rows back: two byte passes per run instead of one per temporal block
  //      (docs/PERFORMANCE.md);
  //    0 bytes: temporal blocks on the byte grid itself (the byte kernels);
  //   -1 auto: bits on a device backend (GOL_U8_VIA_BITS=0|1 overrides),
  //      else bytes.
  int u8_compute = -1;
  // Runtime tuning (gol/tuning.hpp): the engine's own knobs (u8_via_bits,
  // side_poll, cpu_side_poll, poll_copy_side, watchdog_s, overlap_auto) come from here; the
  // backend's from the Tuning it was constructed with.  Default: the table's
  // defaults under the GOL_* environment overrides.
  Tuning tune = Tuning::from_env();
};

struct RunResult {
  int64_t generations = 0;       // the reference's "Generations:" value
  int64_t executed = 0;          // generations actually evaluated in this run
  int64_t first_unchanged = -1;  // g_f, or -1 if no fixed point was seen
  bool extinct = false;
  std::string stop_reason = "limit";  // limit | extinction | similarity | fixed_point
  double loop_ms = 0;            // wall time of the generation loop (incl. final sync)
  int64_t exchanges = 0;         // halo exchanges performed
  int64_t polls = 0;             // termination polls performed
  int64_t kernel_launches = 0;
  bool overlapped = false;       // epochs ran with the overlapped halo exchange
  int64_t graph_launches = 0;    // epochs replayed from a captured HIP graph
  int64_t halo_bytes = 0;        // bytes this rank sent in halo exchanges
  int64_t linked_launches = 0;   // launches that overlapped the previous one (GOL_LINK)
  // Per-phase device time of this run (Engine::set_phase_timing; SURVEY
  // 5.1/5.5): temporal-block kernels, halo exchanges (pack / send / recv /
  // unpack), periodic halo fills, termination-flag reductions (all-reduce +
  // copy to the host).  Phases on different streams may overlap, so the sum
  // can exceed loop_ms; the rest of loop_ms is host gaps and idle device.
  bool phase_timed = false;
  double compute_ms = 0, halo_ms = 0, fill_ms = 0, allreduce_ms = 0;
  // EngineConfig::census: entry i is the live cells of the whole grid (the sum
  // over ranks, on every rank) at generation g0 + 1 + i, g0 the generation the
  // run started at; exactly Engine::generation() - g0 entries.  Empty when off.
  std::vector<int64_t> population;
  // EngineConfig::fingerprint: entry i is the fingerprint of the whole grid at
  // generation g0 + 1 + i (on every rank); Engine::generation() - g0 entries.
  // Empty when off.
  std::vector<uint64_t> fingerprint;
};

// Engine::find_cycle's result.  `period` and `generation` are exact: confirmed
// by comparing the cells of two generations.  `repeats_from` is fingerprint
// evidence.
struct CycleResult {
  int64_t period = 0;       // the cycle's minimal period; 0: none found
  // A generation confirmed to lie on the cycle (grid(generation) ==
  // grid(generation - period)); where the engine stops: Engine::generation().
  int64_t generation = 0;
  // The earliest generation since the call began from which the fingerprints
  // repeat with `period`: a lower bound on the generation the grid entered the
  // cycle at, and equal to it unless two different grids of the transient
  // collide (or the cycle was entered before the call).  -1 with period 0.
  int64_t repeats_from = -1;
  int64_t confirmations = 0;     // exact comparisons that found the repeat (0 or 1)
  int64_t false_candidates = 0;  // candidate periods that an exact comparison rejected
  std::string stop_reason = "limit";  // cycle | limit | extinction
  double loop_ms = 0;            // wall time of the call
  // The fingerprints of the generations the call advanced through (entry i:
  // generation g0 + 1 + i, g0 where the call began), as RunResult::fingerprint.
  std::vector<uint64_t> fingerprint;
};

// The reference's "Generations:" value of a run over (start_gen, limit] whose
// first unchanged generation is g_f = first_unchanged (-1: none), given
// whether the grid at g_f is empty; *reason (optional) receives limit |
// extinction | similarity | fixed_point.  Mirrored by utils/termination.py.
int64_t reported_generations(int64_t first_unchanged, bool extinct, int64_t limit, int64_t start_gen,
                             bool check_similarity, int sim_freq, int sim_phase, std::string* reason = nullptr);

class Engine {
 public:
  Engine(const EngineConfig& cfg, Backend* backend, Transport* transport);
  ~Engine();
  Engine(const Engine&) = delete;
  Engine& operator=(const Engine&) = delete;

  const EngineConfig& config() const { return cfg_; }
  const Decomposition& decomp() const { return dec_; }
  const TileGeom& geom() const { return g_; }
  // The tile the temporal blocks run on: geom(), or its bit-word image when
  // the byte layout computes on bit words (via_bits(); the byte tile then has
  // no halos).
  const TileGeom& compute_geom() const { return tile_geom(via_bits_); }
  int rank() const { return rank_; }
  Extent rows() const { return dec_.rows(rank_); }
  Extent cols() const { return dec_.cols(rank_); }
  int epoch_depth() const { return D_; }
  int tmax() const { return tmax_; }
  bool overlap() const { return trigger_; }
  // "off" | "trigger" | "auto:trial" | "auto:plain" | "auto:trigger".
  std::string overlap_mode() const;
  // Median epoch time (ms, MAX over ranks) of the plain and the trigger
  // schedule in the auto trial (-1: not measured).
  double trial_ms_plain() const { return auto_ms_[0]; }
  double trial_ms_trigger() const { return auto_ms_[1]; }
  // Termination polls: "joined" (the flag all-reduce on the compute stream),
  // "side" (a side stream, tuning side_poll=1), "auto:trial", "auto:side" or
  // "auto:joined" (side_poll = -1, decided on the ranks), and the trial's
  // per-window medians (ms, MAX over ranks; -1: not measured).
  std::string poll_mode() const;
  double poll_trial_ms_joined() const { return poll_ms_[0]; }
  double poll_trial_ms_side() const { return poll_ms_[1]; }
  // Median of the run of side windows that checked a side decision (-1: none).
  double poll_trial_ms_side_steady() const { return poll_side_steady_ms_; }
  // Epoch exchanges started by the boundary trigger so far (diagnostics).
  int64_t triggered_sends() const { return triggered_sends_; }
  // Sample per-phase device times into RunResult (event pairs around every
  // kernel, exchange, fill and reduction; adds a little launch overhead).
  void set_phase_timing(bool on) { phase_timing_ = on; }
  bool phase_timing() const { return phase_timing_; }
  bool graphs() const { return use_graphs_; }
  int64_t generation() const { return gen_; }
  void set_generation(int64_t g) {
    replay_tail();
    gen_ = g;
  }
  // Lazy tail (tuning lazy_tail; run_impl): the generation the block chain
  // has reached - generation(), or up to tmax() - 1 generations past it after
  // a run that ended on a full block instead of a remainder - and how many
  // runs ended that way / how many of those blocks a read of the grid had to
  // rewind and replay as remainder blocks (replay_tail).
  int64_t spine_generation() const { return gen_ + ahead_; }
  int64_t tail_overshoots() const { return tail_overshoots_; }
  int64_t tail_replays() const { return tail_replays_; }
  Backend* backend() const { return be_; }
  // The byte (or bit) tile's current buffer, brought up to date first.
  void* current_buffer() {
    replay_tail();
    sync_bytes();
    be_->quiet_invalidate();  // the caller may write through the pointer
    return buf_[cur_];
  }
  // Quiet-tile skipping (gol/quiet.hpp; tuning quiet_skip): "off" | "on" |
  // "auto:dense" | "auto:skipping"; T-generation blocks run by the dense
  // kernels, as detecting scouts and by the skipping kernel in skipping mode;
  // waves the skipping kernel launched and how many of them skipped their
  // tile (complete once a run has returned).
  std::string quiet_mode() const { return quiet_.name(); }
  int64_t quiet_blocks_dense() const { return quiet_.blocks_dense; }
  int64_t quiet_blocks_scout() const { return quiet_.blocks_scout; }
  int64_t quiet_blocks_skip() const { return quiet_.blocks_skip; }
  int64_t quiet_waves_launched() const { return be_->quiet_tiles_launched() * be_->quiet_tile_waves(); }
  int64_t quiet_waves_skipped();
  bool quiet_list() const { return quiet_.mode != 0 && be_->quiet_list(); }
  int64_t quiet_candidates() const { return be_->quiet_candidates(); }
  bool quiet_cols() const { return quiet_.mode != 0 && be_->quiet_cols(); }
  // {columns computed, columns of the tiles they were computed in} (complete once a run has returned).
  std::vector<int64_t> quiet_cols_counts() {
    quiet_poll();
    int64_t a = 0, b = 0;
    be_->quiet_cols_counts(&a, &b);
    return {a, b};
  }
  // Storage-frame drift (cells, mod W) left by drifting kernels
  // (Backend::drifts): stored column x holds true column x - drift.
  int64_t drift() const { return drift_; }
  // Whether temporal blocks may run the drifting (adder-window) kernel.
  bool drifting() const { return drift_ok_; }
  // Whether byte-layout epochs compute on bit words (EngineConfig::u8_compute).
  bool via_bits() const { return via_bits_; }
  // Whether the tile is a row ring (Backend::row_ring_halo): no row fills,
  // one temporal block per epoch over the owned rows.
  bool row_ring() const { return rows_ring_; }
  // Why a row ring this tile should have had could not be built (the
  // backend's error; the tile then runs with periodic row fills), or "".
  const std::string& row_ring_fallback() const { return ring_fallback_; }
  // Rotates the drift out of the current buffer (owned rows); every
  // read-out (store_cells) does this first.
  void normalize();

  // State I/O.  `cells` is this rank's owned tile (rows() x cols()).
  void load_cells(const uint8_t* cells, int64_t ld);
  // `grid` is the full global grid; this rank copies out its subarray.
  void load_global(const uint8_t* grid, int64_t ld);
  void store_cells(uint8_t* cells, int64_t ld, bool ascii);
  // Owned rows [r0, r0 + n) of the tile only (0 <= r0, r0 + n <= rows()):
  // checks a band of a grid whose whole-tile host copy would not fit.
  void store_rows(uint8_t* cells, int64_t ld, int64_t r0, int64_t n, bool ascii);
  void init_random(uint64_t seed, double density);
  int64_t alive_count();  // local owned cells
  // Fingerprint of the current grid (gol/fingerprint.hpp), summed over ranks:
  // every rank calls it.  Any engine, whatever EngineConfig::fingerprint says
  // (the HIP backend needs tiles that start on a multiple of 32 columns).
  uint64_t fingerprint();
  // Views of the current grid (Backend::density / store_window / place_window).
  // Every rank calls each of them with the same arguments; coordinates are
  // global and in the true frame (a drifted frame is rotated back first), and
  // a rectangle must lie inside the grid (no wrap, on either boundary).
  //
  // The population of every by x bx block of the grid, row-major, ceil(H/by)
  // x ceil(W/bx) blocks (at most Backend::kDensityBlocksMax), clipped at the
  // grid's edge; the same on every rank.  Reduced on the device over the tile
  // that holds the state (the bit image of a byte engine on bit words).
  std::vector<uint64_t> density(int64_t bx, int64_t by);
  // The same into caller memory of ceil(H/by) * ceil(W/bx) entries (checked
  // against the limit before anything is written).
  void density(int64_t bx, int64_t by, uint64_t* out);
  // The h x w cells at (x, y) into `cells` (dense, h x w; '0'/'1' when ascii
  // else 0/1), complete on every rank; w * h <= Backend::kWindowCellsMax.
  void store_window(int64_t x, int64_t y, int64_t w, int64_t h, uint8_t* cells, bool ascii);
  // Writes the dense h x w array `cells` (1 or '1': alive) into the grid at
  // (x, y), leaving the rest of the grid as it is: mode Backend::kPlaceCopy
  // overwrites the rectangle, kPlaceOr adds its live cells.  The generation
  // number stays.
  void place(int64_t x, int64_t y, int64_t w, int64_t h, const uint8_t* cells, int mode);

  // Runs from the current generation up to config().gen_limit with the
  // reference's termination semantics.
  RunResult run();
  // Same, but stops at `limit` (<= gen_limit) - used for chunked runs with
  // checkpoints; the result's generation count is relative to `limit`.
  RunResult run_until(int64_t limit);
  // Runs exactly n more generations (termination flags still recorded, but
  // no early stop): the bench path.
  RunResult advance(int64_t n);
  // Runs until the grid is confirmed to repeat with a period <= max_period, or
  // to generation max_gens (an absolute generation, like run_until's limit;
  // not bounded by gen_limit).  A loop above the run: chunks of `chunk`
  // generations (0: 256), then a search of the fingerprint series since the
  // call began for periods p whose last p generations all satisfy
  // F(g) == F(g - p); the candidates and their divisors are then confirmed
  // exactly, ascending, against a copy of the grid, so the first that matches
  // is the minimal period.  A chunk the change flags stop early is an exact
  // period 1 (stop_reason extinction if the grid is empty).  Needs
  // EngineConfig::fingerprint; every rank calls it and takes the same
  // decisions (the series is global).
  CycleResult find_cycle(int64_t max_gens, int max_period, int64_t chunk = 0);

  // Exchange halos of the current buffer (exposed for tests).
  void halo_exchange();
  // Performs one temporal block from the current buffer (tests).
  void step_block(int T, int64_t row_lo, int64_t row_hi);

 private:
  // A device (or pinned-host) allocation owned by the engine: released
  // through the backend it came from when the handle goes out of scope, so a
  // constructor that throws leaves nothing allocated.
  template <class T = void>
  class Owned {
   public:
    Owned() = default;
    Owned(Backend* be, void* p, bool host = false) : be_(be), p_(static_cast<T*>(p)), host_(host) {}
    Owned(Owned&& o) noexcept : be_(o.be_), p_(o.p_), host_(o.host_) { o.p_ = nullptr; }
    Owned& operator=(Owned&& o) noexcept {
      if (this != &o) {
        reset();
        be_ = o.be_, p_ = o.p_, host_ = o.host_;
        o.p_ = nullptr;
      }
      return *this;
    }
    ~Owned() { reset(); }
    void reset() {
      if (p_) host_ ? be_->release_host(p_) : be_->release(p_);
      p_ = nullptr;
    }
    T* get() const { return p_; }
    operator T*() const { return p_; }

   private:
    Backend* be_ = nullptr;
    T* p_ = nullptr;
    bool host_ = false;
  };
  // A timed span between two Backend::timing_mark marks, tagged with its
  // trial slot or its phase.
  struct Span {
    int kind;
    void* a;
    void* b;
  };
  // Bookkeeping of a run-time A/B trial (the overlap trial over epochs, the
  // poll placement trial over poll windows): spans of two alternating slots
  // timed on the compute stream, one of them open at a time.  The policy -
  // which slot comes next, when to decide and on what - stays with its trial.
  struct Trial {
    explicit Trial(Backend* b) : be(b) {}
    Backend* be;
    void* open = nullptr;  // start mark of the open span
    int slot = -1;         // its slot (-1: a warm-up span, not recorded)
    std::vector<Span> spans;
    int counts[2] = {0, 0};

    // Ends the open span (if any) at a mark taken now: recorded under its
    // slot, or both marks released when it was a warm-up.
    void close();
    void begin(int s) {
      open = be->timing_mark(nullptr);
      slot = s;
    }
    bool full(int s) const;  // kAutoTrials spans of slot s are in
    // Medians of the two slots' spans, MAX over ranks (the slowest rank
    // decides; every rank gets the same values), in ms; releases the spans.
    // `dev` is device scratch for two words.
    void medians(Transport* tr, uint32_t* dev, double out[2]);
    void drop_open();  // a span does not continue into the next run
    void release();
  };
  // One of the two images of the tile: the storage tile (bytes, or the bit
  // layout's words) or the bit-word image of a byte tile.  `par` is the parity
  // of the buffer that holds the current generation.
  struct Tile {
    const TileGeom& g;
    int& par;
    void* buf[2];
    void* cur() const { return buf[par]; }
    void* next() const { return buf[par ^ 1]; }
  };
  const TileGeom& tile_geom(bool bits) const { return bits ? gb_ : g_; }
  Tile tile(bool bits) {
    if (bits) return {gb_, bpar_, {bit_scratch(0), bit_scratch(1)}};
    return {g_, cur_, {buf_[0], buf_[1]}};
  }
  // The tile the temporal blocks alternate over during a run, and the one
  // that holds the state now (the bit image stays the state after a run until
  // the byte tile is read, sync_bytes).
  Tile compute_tile() { return tile(via_bits_); }
  Tile state_tile() { return tile(bits_live_); }

  struct Poll {
    int64_t from = 0, to = 0;
    void* ev = nullptr;
  };
  RunResult run_impl(int64_t limit, bool stop_early);
  Poll poll_issue(int64_t from, int64_t to);
  bool poll_check(Poll& p, int64_t* first_unchanged);
  // Offset of generation from + 1's flag in the flag window (device and mirror).
  int64_t flag_offset(int64_t from) const { return from + 1 - flags_base_; }
  int pick_T(int64_t remaining) const;
  // One temporal block in <in> -> <out> for generations (gen_base, gen_base+T];
  // returns the frame drift of the launch (cells).
  int launch(void* in, void* out, const TileGeom& g, int T, int64_t row_lo, int64_t row_hi, int64_t gen_base,
             const int64_t* trigger_rows = nullptr, bool hot_only = false);
  // A block of a trigger epoch before its last: the boundary rows' light
  // cone at top issue priority (engine.cpp).
  void hot_block(void* in, void* out, const TileGeom& g, int T, int64_t row_lo, int64_t row_hi, int64_t d);
  void add_drift(int64_t cells);
  // Phase-timed Backend::fill_periodic on the compute stream.
  void fill(void* buf, const TileGeom& g, bool cols, bool rows);
  void exchange_columns(void* buf, const TileGeom& g);
  // Without the operations whose peer is -1 (a side on the plane's edge).
  std::vector<P2POp> row_ops(void* buf, const TileGeom& g) const;
  std::array<int, 8> neighbors() const { return dec_.neighbors(rank_, plane_); }
  void halo_exchange_on(void* buf, const TileGeom& g);
  // Byte layout on bit words (EngineConfig::u8_compute = 1): the per-run
  // pack / unpack of the byte tile; the epochs run on compute_tile().
  void pack_bits();
  void unpack_bits();
  void sync_bytes();  // unpack a live bit image into the byte tile (pack_bits in engine.cpp)
  void* bit_scratch(int i) const;
  // Last block of a full epoch in the trigger schedule, in -> out on tile g
  // (the byte tile or its bit image); the caller flips its buffer parity.
  void last_block_trigger(void* in, void* out, const TileGeom& g, int T);
  // Waits for a triggered exchange still in flight; `invalidate` when the
  // buffers are about to change outside the schedule.
  void settle_pending(bool invalidate);
  void run_epoch(int64_t d);
  void release_graphs();
  int graph_key() const { return via_bits_ ? 2 * cur_ + bpar_ : cur_; }
  // Overlap auto trial (EngineConfig::overlap == -1): picks the schedule of
  // the next full epoch, records its start, and decides once enough epochs
  // of both schedules have been timed (at the same epoch on every rank).
  void auto_choose(bool full_epoch);
  void auto_mark();
  void auto_decide();
  void poll_trial_step();
  // Phase timing: a mark on `stream` (nullptr when off or capturing), and
  // the span [a, now] of `phase` on that stream.
  void* phase_begin(void* stream);
  void phase_end(int phase, void* a, void* stream);
  void collect_phases(RunResult& res);

  EngineConfig cfg_;
  Backend* be_;
  Transport* tr_;
  Decomposition dec_;
  int rank_ = 0;
  TileGeom g_;
  int D_ = 0, tmax_ = 0, poll_gens_ = 0;
  Owned<> buf_[2];
  int cur_ = 0;
  Owned<uint32_t> flags_;       // device: changed[t - flags_base_]
  Owned<uint32_t> flags_host_;  // pinned mirror
  int64_t flags_base_ = 0, flags_len_ = 0;
  Owned<uint32_t> alive_dev_;
  Owned<> colbuf_[4];  // send W, send E, recv W, recv E
  bool trigger_ = false;             // boundary-triggered sends (overlap = 3)
  int64_t triggered_sends_ = 0;
  bool send_next_ = false;           // the current epoch is followed by another one in this run
  bool rows_pending_ = false;        // halo rows of the compute tile's current buffer were sent by the last block
  int64_t boundary_sends_ = 0;      // exchanges sent from an epoch's last block (RunResult::overlapped)
  bool use_graphs_ = false, capturing_ = false;
  Owned<int64_t> gen_dev_;            // device: (epoch start - flags_base_) for graph replays
  int64_t epoch_start_ = 0;
  // Captured epochs, keyed by graph_key(): the parity of the buffer pair the
  // epochs alternate over and, for the byte layout on bit words, the byte
  // buffer the bit scratch lives in (bit_scratch depends on cur_, which
  // normalize() flips between runs).
  void* graph_[4] = {nullptr, nullptr, nullptr, nullptr};
  int graph_flip_[4] = {0, 0, 0, 0};
  int64_t graph_kernels_[4] = {0, 0, 0, 0};
  uint32_t* graph_flags_ = nullptr;   // flags buffer the graphs were captured with
  int64_t graph_runs_ = 0;
  int64_t halo_bytes_ = 0;
  double watchdog_s_ = 900;
  int64_t gen_ = 0;
  int64_t exchanges_ = 0, polls_ = 0, launches_ = 0;
  bool plane_ = false;      // EngineConfig::boundary == Boundary::Dead
  bool plain_ = true;       // a torus engine with no series: no plane, census or fingerprint
  // A fused per-generation series (EngineConfig::census, ::fingerprint): the
  // device window of 64-bit values, parallel to flags_ (same base and length,
  // zeroed with it), and whether a run is filling it (launches outside a run -
  // step_block - record nothing).
  struct Series {
    const char* name;  // in messages
    bool on = false;   // the configuration asks for it
    Owned<uint64_t> win;
    bool run = false;
  };
  Series census_{"census"}, fprint_{"fingerprint"};
  // The device word of fingerprint(); below, find_cycle's copy of the state tile.
  Owned<uint64_t> fp_dev_;
  // density()'s block map and store_window()'s window on the device (the
  // latter on multi-rank runs only), kept between calls and re-allocated
  // when a call needs more (density_len_) or another size (window_len_).
  Owned<uint64_t> density_dev_, density_host_, window_dev_;  // density_host_: the map's pinned mirror
  size_t density_len_ = 0, window_len_ = 0;
  void require_rect(const char* what, int64_t x, int64_t y, int64_t w, int64_t h) const;
  Owned<> snap_;
  size_t snap_bytes_ = 0;
  bool differs_from_snapshot();
  bool drift_ok_ = false;   // whole-width tile of 32-cell words on a drifting backend
  bool cols_filled_ = true; // column halos kept valid by fills (false: the backend wraps column reads)
  bool rows_wrapped_ = false; // single-rank torus read modulo its rows (no fills at all)
  bool rows_ring_ = false;    // row halos are second mappings of the owned rows (Backend::row_ring_halo)
  std::string ring_fallback_;  // alloc_row_ring's error when the ring fell back to fills
  bool link_ = false;         // blocks may run linked (Backend::KernelChoice::link; ring tiles only)
  bool via_bits_ = false;    // byte layout computed on bit words (compute_tile() is the bit image)
  TileGeom gb_;              // the tile in the bit layout (same rows, halos, words)
  Owned<> bitbuf_[2];        // own bit scratch when the spare byte buffer cannot hold it
  int bpar_ = 0;             // bit_scratch(bpar_) holds the current generation during a run
  bool bits_live_ = false;   // ... and after it, until the byte tile is read (sync_bytes)
  bool poll_side_ = false;   // termination polls reduce on the comm stream (Transport::side_reduce)
  bool polled_side_ = false;  // a poll of this run went to Backend::poll_side()
  bool poll_copy_side_ = true;  // tuning poll_copy_side: single-rank polls on Backend::poll_side()
  int64_t drift_ = 0;
  int64_t graph_drift_[4] = {0, 0, 0, 0};
  // Quiet-tile skipping: the policy (mode 0 where the tile is not eligible),
  // and the last report read from the backend.
  quiet::Policy quiet_;
  int64_t quiet_seq_seen_ = 0, quiet_skipped_tiles_ = 0;
  void quiet_poll();
  // Lazy tail (tuning lazy_tail).  ahead_ > 0: the compute tile's current
  // buffer holds generation gen_ + ahead_ (the spine), the other one still
  // holds the last block's input, generation gen_ + ahead_ - tmax_, and the
  // flags of (gen_, gen_ + ahead_] wait on the device for the next run.
  bool tail_ok_ = false;       // the tile may end a run on a full block (single-rank ring, D = tmax, no graphs)
  int tail_mode_ = 0;          // tuning lazy_tail
  int64_t ahead_ = 0;
  int64_t tail_drift_ = 0;     // drift_ before that block
  bool tail_hold_ = false;     // auto: the last such block was replayed for a read; remainder blocks until
  bool grid_read_ = false;     // ... a run follows a run with no read of the grid in between
  bool no_flags_ = false;      // launches of a replay record no flags
  int64_t tail_overshoots_ = 0, tail_replays_ = 0;
  Owned<uint32_t> carry_;      // device: the carried flags between a run's flag reset and their new offsets
  bool tail_wanted();
  // Brings the grid to generation gen_ when the block chain is ahead of it;
  // everything that reads or writes the grid outside a run calls it first.
  void replay_tail();
  // Overlap auto trial.
  bool auto_overlap_ = false;       // trial still running
  bool auto_decided_ = false;
  int auto_sched_ = 0;              // trial slot of the current epoch: 0 plain, 1 trigger, -1 warm-up
  int64_t auto_full_epochs_ = 0;    // full epochs seen so far
  Trial otrial_{be_};
  double auto_ms_[2] = {-1, -1};
  // Poll placement trial (tuning side_poll = -1, poll_trial_step): slot 0
  // joined, 1 side.
  bool poll_trial_ = false, poll_decided_ = false;
  int64_t ptrial_polls_ = 0;
  Trial ptrial_{be_};
  double poll_ms_[2] = {-1, -1};
  bool ptrial_verify_ = false;      // checking a side decision on consecutive side windows
  double poll_side_steady_ms_ = -1;
  // Phase timing.
  bool phase_timing_ = false;
  std::vector<Span> phase_spans_;
};

}  // namespace gol
