// Launch interfaces of the hand-written CDNA4 kernels (gfx950).
#pragma once

#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "gol/quiet.hpp"
#include "gol/tile.hpp"

namespace gol {
namespace hipk {

struct LifeBlockParams {
  const uint8_t* in;
  uint8_t* out;
  int64_t pitch;
  int64_t row_lo, row_hi;
  int Wp;          // padded words per row
  int ncolw;       // column waves (64*W-2 output words each)
  int nseg;        // row segments
  int seg_rows;    // output rows per segment (balanced: first seg_rem get +1)
  int seg_rem;
  int own_w0, own_w1;
  uint32_t last_mask;
  uint32_t* changed;  // changed[L] <-> generation gen_base + 1 + L (after resolving gen_dev)
  const int64_t* gen_dev;  // if set: changed += *gen_dev + gen_rel at run time (graph replay)
  int64_t gen_rel;
  // Grouped schedule (life_group_kernel): nseg = groups per column strip,
  // seg_rows/seg_rem = balanced OUTPUT rows per group, grp_q = output rows of
  // every wave of a group but the last.
  int grp_q;
  // Diagnostics (GOL_WG_TRACE): if set, every wave of the grouped kernel
  // writes {block<<8 | wave, XCC_ID<<32 | HW_ID, start, end} (s_memrealtime,
  // 100 MHz) at wg_trace[4 * (block * M + wave)], below kWgTraceWaves waves.
  uint64_t* wg_trace;
  // Device-visible error word (Mailbox::err, Backend::check_device_errors):
  // a kernel that has to give up (life_short_kernel's bounded LDS hand-off
  // wait) sets it instead of continuing silently with invalid rows.
  uint32_t* err;
  // Chained-group spin bound, log2 of polls (GOL_CHAIN_SPIN, default 16).
  int chain_spin_log2;
  // Wrap mode (BlockArgs::full_width): owned words per row, 0 = halo mode
  // (life_block_impl.hpp lane_cols).
  int wrap_w;
  // Folded last strip (life_group_kernel, wrap mode): `fold` groups per
  // block in sub-strips of fold_lanes lanes; 1 = no folding.
  int fold;
  int fold_lanes;
  // Chained groups (life_group_kernel, LaunchCtx::chain; null chain_buf =
  // off): the last wave of group g ends like an inner wave, with the inverted
  // triangle fed by group g + 1's wave 0 through global memory, so no group
  // boundary keeps a redundant triangle.  Per (strip, group) slot: wave 0's
  // saved boundary rows in chain_buf, and chain_flag = chain_seq once they are
  // written.  Every group is M x grp_q rows but a strip's last one, which ends
  // at chain_end.
  uint32_t* chain_buf;
  uint32_t* chain_flag;
  uint32_t chain_seq;
  int64_t chain_end;
  // Linked launches (LaunchCtx::link, life_group_kernel<..., LINK = true>):
  // this launch may run while the previous grouped launch, whose output is
  // its input, still runs.  Group (kcol, grp) first waits until every group
  // of that launch whose output rows it reads (its strip and the two beside
  // it) has published link_prev_flag[strip * link_prev_nseg + group] ==
  // link_prev_seq, and after its last store publishes link_flag[kcol * nseg
  // + grp] = link_seq.  Payload stores and input loads are sc1 (the no-
  // acquire valid form of cdna_hip_programming.md Guideline 16).
  uint32_t* link_flag;             // null: not a linked launch
  uint32_t link_seq;
  const uint32_t* link_prev_flag;  // null: nothing to wait for
  uint32_t link_prev_seq;
  int64_t link_prev_row_lo;
  int link_prev_nseg, link_prev_seg_rows, link_prev_seg_rem;
  // > 0: both launches cover the owned rows of a row ring of this many rows;
  // the rows a group reads beyond them wrap around the torus (link_wait).
  int64_t link_ring_rows;
  // Boundary trigger (BlockArgs::trigger / hot; linked launches only): the
  // groups grp in [bnd_g[0], bnd_g[1]) or [bnd_g[2], bnd_g[3]) - those whose
  // output rows meet the trigger rows, trigger_groups() - run at top issue
  // priority, and with bnd_count set each adds 1 to *bnd_count after its
  // link_flag store (a one-wave kernel on another stream waits on it,
  // launch_wait_counter).  Group indices, not rows, so the kernel's test is
  // a few scalar compares (row bounds in 64 bits cost the linked kernels
  // SGPR spills).
  unsigned long long* bnd_count;
  int bnd_g[4];
  // Fault injection (GOL_FAULT_DELAY_SPINS, tests): producers at the torus
  // seam - a linked launch's first and last groups - sleep this many s_sleep 127
  // rounds (~3.4 us each) before publishing, so a missing dependency wait
  // reads stale rows deterministically instead of by chance.
  int fault_delay;
  // Quiet-tile skipping (life_quiet_kernel, gol/quiet.hpp): one word per
  // (strip, group) tile.  quiet_prev: the previous block's words (null:
  // nothing may skip); quiet_next: this block's.  The counters at quiet_count
  // (kQuietCountBytes, below) pack, per launch, groups done (bits 0..19),
  // clean tiles (20..39) and skipped groups (40..59); the last group to finish
  // stores quiet_seq << 40 | clean << 20 | skipped to quiet_report[0]
  // (host-mapped) and resets them; quiet_report[1]: tiles skipped by all
  // launches so far.
  const uint32_t* quiet_prev;
  uint32_t* quiet_next;
  unsigned long long* quiet_count;
  unsigned long long* quiet_report;
  uint32_t quiet_seq;
  // The candidate list (life_quiet_kernel<..., LIST = true>; gol/quiet.hpp):
  // the launch runs the tiles of quiet_items - kQuietCounters inclusive
  // sub-list ends, then the sub-lists of quiet_cap entries each; null: every
  // tile - as item blockIdx.x (the looping kernel: further items from a
  // ticket, whatever its grid), and its computing tiles append the next
  // block's candidates to quiet_items_next, de-duplicated by
  // quiet_stamp[tile] == quiet_seq.  quiet_lc: the 64-bit words of
  // QuietListWords; quiet_fset: the flag-count set it updates.
  // quiet_report[2]: quiet_seq << 40 | the next block's candidates.
  const uint32_t* quiet_items;
  uint32_t* quiet_items_next;
  uint32_t* quiet_stamp;
  unsigned long long* quiet_lc;
  int quiet_cap;
  int quiet_fset;
  // Short waves (life_quiet_chunk_kernel): one-wave workgroups per item, and
  // the 64-bit word-and-arrival accumulator of every tile (zero between
  // launches).
  int quiet_chunks;
  unsigned long long* quiet_acc;
  // The column kernel (life_quiet_cols_kernel; gol/quiet.hpp, Column records):
  // the records that go with quiet_prev / quiet_next, quiet::kColLanes per
  // (tile, row band), quiet_bands bands per tile.  Null in launches of the
  // other bodies, which publish words without quiet::kCols.
  const uint32_t* quiet_rec_prev;
  uint32_t* quiet_rec_next;
  int quiet_bands;
  // Bounded plane (BlockArgs::plane; the kernels of lb::PlaneIO): the padded
  // rows [grid_row_lo, grid_row_hi) and padded words [grid_w0, grid_w1) that
  // lie inside the grid, and the in-grid cells of word grid_w1 - 1.  A side of
  // the tile that is not the grid's edge passes the tile's own bound, which
  // masks nothing.  Rows in 32 bits, as for bnd_g (SGPR budget).  Unused by
  // every other kernel.
  int grid_row_lo, grid_row_hi;
  int grid_w0, grid_w1;
  uint32_t grid_last_mask;
  // Census (BlockArgs::census; the kernels of lb::CensusIO): the 64-bit slot of
  // the block's first generation, one slot per generation, addressed like
  // `changed` (with gen_dev: census + *gen_dev + gen_rel).  Every wave or
  // group adds its count of each generation's live owned cells.  A census
  // launch is never a plane launch and passes the tile's owned rows in
  // grid_row_lo / grid_row_hi.  Null in every other launch.
  unsigned long long* census;
  // Fingerprint (BlockArgs::fingerprint; the kernels of lb::FingerprintIO;
  // gol/fingerprint.hpp): the 64-bit slot of the block's first generation,
  // addressed like `census`.  Every wave or group adds its share of each
  // generation's fingerprint: the owned words of the rows it counts (the
  // census's rows; grid_row_lo / grid_row_hi hold the tile's owned rows),
  // weighted by the keys of their global row - padded row r is global row
  // fp_row0 + r, in 32 bits as for bnd_g (SGPR budget) - and global word:
  // padded word own_w0 is global word fp_word0.  Null in every other launch.
  unsigned long long* fingerprint;
  int fp_row0;
  int fp_word0;
};

constexpr int64_t kWgTraceWaves = int64_t(1) << 20;

// Cross-lane primitive that moves the edge words between lanes.
//   kXlaneAdd: no cross-lane data op at all.  The horizontal window is
//   one-sided (cells x-2, x-1, x): both shifts are add-with-carry
//   (v_add_co / v_addc_co) whose per-lane carry masks move one lane up on the
//   SALU (s_lshl_b64).  Each generation then stores cell x-1 at bit x, so the
//   tile's storage frame drifts one cell to the right per generation; the
//   engine tracks the drift and rotates it out before any read-out
//   (Engine::normalize).  Measured (ubench_dpp_mix.hip, git e36884f): any DPP,
//   v_alignbit or v_cmp in a v_bitop3 stream drops the SIMD from ~2.4 to
//   ~4.5 cycles per instruction; add-with-carry ops do not.
//   kXlaneAuto (default): the adder window where the engine allows a drift
//   (HipBackend::choose_kernel: whole-width tiles that fill four waves per
//   SIMD at T = 12), the DPP window everywhere else.
enum Xlane : int { kXlaneAuto = -1, kXlaneDpp = 0, kXlaneAdd = 3 };

// Backend-owned state of linked launches (GOL_LINK; LifeBlockParams::link_*):
// consecutive grouped launches of an epoch alternate between two streams and
// overlap, ordered by per-group completion words instead of the stream.
struct LinkState {
  hipStream_t stream[2] = {nullptr, nullptr};  // [0] = the backend's compute stream
  hipEvent_t before[2] = {nullptr, nullptr};   // recorded on stream[i] just before its last launch
  int cur = 0;                                  // stream of the last launch
  bool prev_valid = false;                      // the last launch may be linked to
  const void* prev_out = nullptr;               // its output buffer
  double prev_share = 0.0;                      // its workgroups / how many of them fit on the CUs
  LifeBlockParams prev{};                       // its plan and completion words
  uint32_t* flags[3] = {nullptr, nullptr, nullptr};  // completion words, rotating per launch
  size_t flag_words = 0;
  uint32_t seq = 0;
  // The stream of the next launch already follows the last launch's start
  // (Backend::trigger_stream: its wait kernel returns only once that
  // launch's boundary groups are done), so a linked next launch needs no
  // cross-stream event wait (~10 us of device time on the epoch boundary).
  bool started = false;
};

// Boundary trigger of one launch (BlockArgs::trigger / hot; linked launches
// only): the groups meeting `rows` run at top issue priority, and in a
// counting launch each adds one to *counter once its rows are written.
struct TriggerReq {
  enum Kind { kNone, kHot, kCounting } kind = kNone;
  int64_t rows[4] = {0, 0, 0, 0};
  unsigned long long* counter = nullptr;
};

// The groups of a grouped plan whose output rows meet the trigger rows
// [r[0], r[1]) and [r[2], r[3]): index ranges [g[0], g[1]) and [g[2], g[3])
// (each contiguous: groups are ordered by row); returns how many groups meet
// either, per column strip (a folded strip publishes each of its groups once,
// so a counting launch makes ncolw times this many increments).
inline int trigger_groups(const LifeBlockParams& q, const int64_t* r, int* g) {
  int n = 0;
  g[0] = g[1] = g[2] = g[3] = 0;
  for (int s = 0; s < q.nseg; ++s) {
    const int64_t e = q.row_lo + int64_t(s) * q.seg_rows + std::min(s, q.seg_rem) + q.seg_rows + (s < q.seg_rem ? 1 : 0);
    const int64_t b = e - q.seg_rows - (s < q.seg_rem ? 1 : 0);
    bool any = false;
    for (int k = 0; k < 2; ++k)
      if (b < r[2 * k + 1] && e > r[2 * k]) {
        if (g[2 * k + 1] == 0) g[2 * k] = s;
        g[2 * k + 1] = s + 1;
        any = true;
      }
    n += any ? 1 : 0;
  }
  return n;
}

// Everything enqueued on stream[1] precedes what comes next on stream[0];
// the next launch starts a new chain.
inline void link_join(LinkState& L) {
  L.started = false;
  if (L.cur != 0) {
    (void)hipEventRecord(L.before[1], L.stream[1]);
    (void)hipStreamWaitEvent(L.stream[0], L.before[1], 0);
    L.cur = 0;
  }
  L.prev_valid = false;
}

// Backend-owned state of the quiet-tile skipping kernel (BlockArgs::quiet;
// gol/quiet.hpp): the two tile-word maps consecutive blocks alternate over,
// and what the last skipping-kernel launch was (quiet::may_follow).
struct QuietState {
  quiet::Launch prev{};            // prev.T == 0: no words to read
  int cur = 0;                     // map the last launch wrote
  uint32_t seq = 0;                // launches so far (24 bits reach the report)
  int64_t tiles = 0;               // tiles of the last launch
  int seg_rows = 96;               // output rows per group the plan aims at (tuning quiet_rows)
  // The candidate list (tuning quiet_list, quiet_grid).
  bool list = false;               // launches run the list kernel
  int grid = 0;                    // grid of a list launch: 0 every tile, n forced, -1 from the newest report
  bool listed = false;             // the last launch appended the next block's candidates
  uint32_t listed_since = 0;       // first launch of the unbroken run of appending launches (0: none)
  int items = 0;                   // item buffer the last launch appended to
  int fset = 0;                    // flag-count set the last launch updated
  int64_t grid_last = 0;           // groups of the last launch
  int chunks = -1;                 // tuning quiet_chunks: -1 by the reported list length, 1 off, n forced
  int64_t chunk_waves = 1024;      // tuning quiet_chunk_waves: most one-wave workgroups an automatic choice makes
  int chunks_last = 1;             // one-wave workgroups per item of the last launch (1: the grouped kernel)
  // The column kernel (tuning quiet_cols, quiet_col_group, quiet_col_items).
  int cols = 0;                    // 0 off, -1 by the reported list length, 1 every listed launch
  int col_group = 4;               // owned word columns per unit: 2, 4 or 8
  int64_t col_items = 42;          // quiet_cols auto: the longest reported list the column kernel runs
  bool cols_last = false;          // the last launch ran the column kernel
};

// Words the kernels write for the host: one fine-grained pinned host
// allocation, written through its device alias and read without a copy.
struct Mailbox {
  uint32_t err[4];  // LifeBlockParams::err: the code (check_device_errors), then a give-up's diagnostics
  unsigned long long quiet_report[5];  // LifeBlockParams::quiet_report
};

// Device memory that persists across launches, owned by the backend: one
// buffer per slot, grown on demand.  A grown buffer is new memory, zeroed
// where the slot says so (flags and words compared with sequence numbers) by
// a fill on the compute stream, which orders it before the launch it is for.
class Scratch {
 public:
  enum Slot {
    kChainFlags, kChainSlots, kLinkWordsA, kLinkWordsB, kLinkWordsC, kQuietMapA, kQuietMapB, kQuietCounters,
    kQuietList, kQuietRecA, kQuietRecB, kSlots
  };
  static constexpr Slot kLinkWords[3] = {kLinkWordsA, kLinkWordsB, kLinkWordsC};  // LinkState::flags
  // The two compute streams (the second may be null), which both drain before
  // a buffer is replaced; check_dev >= 0: every buffer handed out is checked
  // to live on that device (tuning check_device).
  void init(hipStream_t compute, hipStream_t linked, int check_dev) {
    streams_[0] = compute, streams_[1] = linked, check_dev_ = check_dev;
  }
  uint32_t* get(Slot slot, size_t bytes);  // at least `bytes` bytes of the slot's buffer
  // The chain flags' launch counter (0 = never written).
  uint32_t next_chain_seq() {
    if (++chain_seq_ == 0) chain_seq_ = 1;
    return chain_seq_;
  }
  void release();

 private:
  hipStream_t streams_[2] = {nullptr, nullptr};
  int check_dev_ = -1;
  void* buf_[kSlots] = {};
  size_t bytes_[kSlots] = {};
  uint32_t chain_seq_ = 0;
};

// Construction-time knobs of the launchers (Tuning, read once by HipBackend).
struct LifeTuning {
  int cus = 256;            // compute units of the device
  int target_waves = 0;     // waves per launch round (0 = occupancy x CUs x 4 SIMDs)
  int min_seg_rows = 16;    // lower bound on rows per wave segment
  int xlane = kXlaneAuto;   // cross-lane primitive
  bool u8_lds = false;      // byte layout: single-step LDS-tiled kernel (T = 1)
  int lds_rows = 32;        // rows per LDS tile (32 or 64)
  int lds_T = 8;            // generations per launch of the LDS-tiled byte kernel (1, 2, 4, 8; 16, 32 packed)
  bool lds_pack = true;     // LDS-tiled byte kernel evaluates on bit words packed in LDS (T >= 8)
  bool lds_xcd = false;     // packed LDS tiles: XCD-aware workgroup order (column-major runs per XCD)
  int lds_waves = 0;        // packed LDS tiles: waves per workgroup (8, 16; 0 = by grid size)
  int group = 8;            // grouped schedule, waves per workgroup sharing boundaries: 4, 8, -1 auto, 0 off
  int group_small = 4;      // the same for bit-layout blocks of T <= 8 (GOL_GROUP_SMALL; GOL_GROUP sets both)
  bool wrap = true;         // wrap mode on whole-width tiles (BlockArgs::full_width, lane_cols)
  bool fold = true;         // folded last strip in wrap mode (life_group_kernel)
  int chain = 0;            // chained groups (GOL_CHAIN): 0 off, 1 on, -1 autotuned per launch shape
  int chain_spin_log2 = 16;  // LifeBlockParams::chain_spin_log2
  int fault_delay = 0;  // LifeBlockParams::fault_delay (GOL_FAULT_DELAY_SPINS)
};

// What one launch_life_block call may use and was asked for, built by the
// backend for that launch alone.
struct LaunchCtx {
  Scratch* scratch = nullptr;    // the backend's, always set
  Mailbox* mail = nullptr;       // its device alias, always set
  const Mailbox* mail_host = nullptr;  // the host's view of it (the skipping kernel's reports)
  LinkState* link = nullptr;     // the launch may join a linked chain (null: it runs on the given stream)
  QuietState* quiet = nullptr;   // the launch may run the skipping kernel
  bool chain = false;            // chained groups (LifeBlockParams::chain_buf) where the plan allows
  uint64_t* wg_trace = nullptr;  // per-wave placement/timing record (LifeBlockParams::wg_trace)
  TriggerReq trigger;
};

// Which kernel a launch ran (the backend's launch census, Backend::launch_paths).
enum LaunchPath : int { kPathClassic, kPathGrouped, kPathChained, kPathLinked, kPathSkipping, kPathLdsTiled, kLaunchPaths };
constexpr const char* kLaunchPathNames[kLaunchPaths] = {"classic", "grouped", "chained", "linked", "skipping", "lds_tiled"};

struct LaunchResult {
  LaunchPath path = kPathClassic;  // kPathLinked: a launch that overlaps the previous one
  int drift = 0;  // storage-frame drift in cells (T for the adder window, else 0; BlockArgs::allow_drift)
  int64_t trigger_adds = 0;  // increments a counting launch makes to TriggerReq::counter (0: it carries none)
  int64_t quiet_tiles = 0;   // tiles of a skipping launch
};

LaunchResult launch_life_block(const BlockArgs& a, const LifeTuning& tune, const LaunchCtx& ctx, hipStream_t stream);
// The Life-like rules compiled for the HIP engine besides B3/S23
// (life_rules.def), and whether launch_life_block runs `r`.
std::vector<Rule> life_block_rules();
bool life_block_has_rule(Rule r);
// Description of the kernel variant the tuning selects for a layout, and of
// the one a plane, census or fingerprint engine runs (BlockArgs::features).
std::string life_block_variant(Layout layout, const LifeTuning& tune, BlockMode mode = BlockMode::Plain);
// Largest T that keeps 2 waves/SIMD for the variant's words-per-lane.
int life_block_max_T(Layout layout, const LifeTuning& tune);

// Compiled variants (one translation unit each): the DPP and adder windows,
// bit and byte layouts, one 32-cell word per lane.
#define GOL_LIFE_VARIANT(name) \
  LaunchResult name(const LifeBlockParams& p, int64_t out_rows, int T, const LifeTuning& tune, const LaunchCtx& ctx, hipStream_t s)
GOL_LIFE_VARIANT(launch_bits_w1_dpp);
GOL_LIFE_VARIANT(launch_u8_w1_dpp);
GOL_LIFE_VARIANT(launch_bits_w1_add);
GOL_LIFE_VARIANT(launch_u8_w1_add);
// The feature kernels (life_block_<name>_*.hip, launch_life_block's kModes):
// the bounded plane (lb::PlaneIO), the census (lb::CensusIO) and the
// fingerprint (lb::FingerprintIO), scheduled like the census.  DPP window only:
// the adder window's drifting frame is a relabelling of torus columns (it
// would count exactly too, but it is a second set of kernels).
GOL_LIFE_VARIANT(launch_plane_bits_dpp);
GOL_LIFE_VARIANT(launch_plane_u8_dpp);
GOL_LIFE_VARIANT(launch_census_bits_dpp);
GOL_LIFE_VARIANT(launch_census_u8_dpp);
GOL_LIFE_VARIANT(launch_fprint_bits_dpp);
GOL_LIFE_VARIANT(launch_fprint_u8_dpp);
// The quiet-tile skipping kernel (bit layout, DPP window, T = 12, 4-wave
// groups of short segments; life_block_bits_w1_dpp_quiet.hip): wrap-mode
// blocks over a row ring's owned rows only.  Returns the tiles launched, 0
// (nothing launched) where the block cannot be planned that way.
int64_t launch_bits_w1_dpp_quiet(const LifeBlockParams& p, int64_t out_rows, int T, const LaunchCtx& ctx, hipStream_t s);
// Output rows per row band of the column kernel (64 lanes less the cone), and
// the most bands per tile it is compiled to keep records for.
constexpr int kQuietColBandsMax = 4;
void prepare_bits_w1_dpp_quiet(Scratch& scratch, int64_t H, int64_t words, bool list);
constexpr int kQuietT = 12;
// LifeBlockParams::quiet_count, in 64-bit words a cache line apart: the
// launch's counter, the tiles skipped by all launches, kQuietCounters
// first-level counters.
constexpr unsigned kQuietCounters = 64;
constexpr int kQuietCountStride = 16;
constexpr size_t kQuietCountBytes = size_t(4 + kQuietCounters) * kQuietCountStride * 8;
// After the first-level counters, the column kernel's totals over all
// launches: word columns it computed, and owned word columns of the tiles it
// computed them in (quiet_report[3], [4]).
constexpr int kQuietColsComputed = 2 + int(kQuietCounters), kQuietColsOfTiles = 3 + int(kQuietCounters);
// LifeBlockParams::quiet_lc, in 64-bit words (a cache line per counter or
// slot): the append counts of the kQuietCounters sub-lists (tile %
// kQuietCounters), the two flag-count sets (slot tile % kQuietCounters,
// quiet::flag_words words each), the two launch-parity tickets.
struct QuietListWords {
  static constexpr int kAppend = 0;
  static constexpr int kFlags = kAppend + int(kQuietCounters) * kQuietCountStride;
  static constexpr int kFlagSet = int(kQuietCounters) * kQuietCountStride;
  static constexpr int kTicket = kFlags + 2 * kFlagSet;
  static constexpr int kWords = kTicket + 2 * kQuietCountStride;
};
// Scratch::kQuietList of a plan of `tiles` tiles: the 64-bit words, the
// stamps, two item buffers (kQuietCounters ends + kQuietCounters sub-lists),
// the chunk kernel's accumulators.
// Short waves: an item runs as kQuietChunksAuto one-wave workgroups when the
// newest reported list times that many fits QuietState::chunk_waves waves; at most kQuietChunksMax (the accumulator's arrival bits).
constexpr int kQuietChunksMax = 24;
constexpr int kQuietChunksAuto = 24;
struct QuietListLayout {
  int cap;
  size_t stamp, items[2], acc, bytes;  // byte offsets
  explicit QuietListLayout(int64_t tiles) {
    cap = int((tiles + kQuietCounters - 1) / kQuietCounters);
    const size_t item_bytes = size_t(kQuietCounters) * (1 + size_t(cap)) * 4;
    stamp = size_t(QuietListWords::kWords) * 8;
    items[0] = stamp + ((size_t(tiles) * 4 + 127) & ~size_t(127));
    items[1] = items[0] + ((item_bytes + 127) & ~size_t(127));
    acc = items[1] + ((item_bytes + 127) & ~size_t(127));
    bytes = acc + size_t(tiles) * 8;
  }
};

// Single-generation LDS-tiled byte-layout kernel (life_step_lds.hip).
void launch_life_step_lds(const BlockArgs& a, int lds_rows, bool wrap, hipStream_t stream);
// The same with T = 2, 4 or 8 generations per launch through two LDS row
// buffers (life_step_lds.hip life_lds_multi_kernel).
void launch_life_lds_multi(const BlockArgs& a, bool wrap, hipStream_t stream);
// The same tile packed to bit words in LDS (T = 8, 16 or 32 generations per
// launch, bit-sliced rule; life_step_lds.hip life_lds_bits_kernel).  Returns
// the drift of the stored frame (T with the adder window, which it runs
// where BlockArgs::allow_drift and the tile wraps its columns; else 0).
int launch_life_lds_bits(const BlockArgs& a, bool wrap, bool xcd_order, int waves, int cus, hipStream_t stream);

// Tile utility kernels (tile_ops.hip).
void launch_fill_cols(uint8_t* buf, const TileGeom& g, hipStream_t s);
// Column halos of padded rows [r0, r0 + nrows) only.
void launch_fill_cols_rows(uint8_t* buf, const TileGeom& g, int64_t r0, int64_t nrows, hipStream_t s);
void launch_fill_rows(uint8_t* buf, const TileGeom& g, hipStream_t s);
// Fused cols+rows periodic fill (bit layout); false if the geometry needs the two-launch path.
bool launch_fill_all(uint8_t* buf, const TileGeom& g, hipStream_t s);
void launch_alive(const uint8_t* buf, const TileGeom& g, uint32_t* any_flag,
                  unsigned long long* count, hipStream_t s);
// Owned rows [r0, r0+n) from a device staging array of 0/1-or-ASCII bytes.
void launch_load_rows(uint8_t* buf, const TileGeom& g, const uint8_t* stage, int64_t ld,
                      int64_t r0, int64_t n, hipStream_t s);
void launch_store_rows(const uint8_t* buf, const TileGeom& g, uint8_t* stage, int64_t ld,
                       int64_t r0, int64_t n, bool ascii, hipStream_t s);
void launch_i64(int64_t* p, int64_t v, bool add, hipStream_t s);
// Holds stream s until *counter >= target (one sleeping wave; error word 7
// after ~4 s): the boundary trigger's wait (Backend::trigger_stream).
void launch_wait_counter(const unsigned long long* counter, unsigned long long target, uint32_t* err, hipStream_t s);
void launch_init_random(uint8_t* buf, const TileGeom& g, uint64_t seed, uint32_t thresh24,
                        int64_t grow0, int64_t gcol0, hipStream_t s);
// Owned rows of `src` rotated left by `shift` cells (0 < shift < W) into
// `dst`: dst cell x = src cell (x + shift) mod W.  Undoes the adder window's
// storage drift.
void launch_rotate_cols(const uint8_t* src, uint8_t* dst, const TileGeom& g, int64_t shift, hipStream_t s);
// Owned rows [i0, i0 + nrows) of the owned cells, byte cells <-> bit words
// (the two geometries hold the same owned tile; halos and pitch may differ).
void launch_convert_rows(const uint8_t* src, const TileGeom& gs, uint8_t* dst, const TileGeom& gd, int64_t i0,
                         int64_t nrows, hipStream_t s);
// Adds the fingerprint share (gol/fingerprint.hpp) of the tile's owned cells to
// *out64: owned row 0 is global row global_row0, the first owned word global
// word global_word0.  Either layout; the last word's cells beyond W count as 0.
void launch_fingerprint(const uint8_t* buf, const TileGeom& g, int64_t global_row0, int64_t global_word0,
                        unsigned long long* out64, hipStream_t s);
// The owned rows of src (whole pitch) into dst, a tile buffer of the same
// geometry (src may be a row ring; dst's halo rows are left alone).
void launch_copy_owned_rows(const uint8_t* src, uint8_t* dst, const TileGeom& g, hipStream_t s);
// Sets *flag to 1 if any owned cell of two tiles of geometry g differs.
void launch_equal(const uint8_t* a, const uint8_t* b, const TileGeom& g, uint32_t* flag, hipStream_t s);

// View kernels (view_ops.hip; Backend::density / store_window / place_window).
// Adds the live owned cells of the tile to the global by x bx block map `out`
// (row-major, ceil(grid_w / bx) blocks per row); owned row 0 is global row
// global_row0, the first owned cell global cell global_col0.  Either layout.
void launch_density(const uint8_t* buf, const TileGeom& g, int64_t global_row0, int64_t global_col0, int64_t grid_h,
                    int64_t grid_w, int64_t bx, int64_t by, unsigned long long* out, hipStream_t s);
// The hh x ww owned cells from owned row r0, owned cell c0 on, into / from a
// dense device array of hh x ww bytes.
void launch_store_window(const uint8_t* buf, const TileGeom& g, int64_t r0, int64_t c0, int64_t ww, int64_t hh,
                         uint8_t* stage, bool ascii, hipStream_t s);
void launch_place_window(uint8_t* buf, const TileGeom& g, int64_t r0, int64_t c0, int64_t ww, int64_t hh,
                         const uint8_t* stage, bool copy, hipStream_t s);

}  // namespace hipk
}  // namespace gol
