// Quiet-tile skipping: the pure decision logic, shared by the HIP kernel
// (csrc/kernels/life_quiet_impl.hpp), the HIP backend, the engine and the CPU
// tests (bindings quiet_*).
//
// A temporal block of T generations reads one buffer and writes the other.
// If a region and its light cone hold what they held T generations ago, the
// block would write exactly what the destination buffer already holds (the
// state two blocks back, which equals the new one), so a workgroup of the
// skipping kernel may leave its tile alone.  A tile is one workgroup's output
// rows of one column strip of the launch plan; every block of the skipping
// kernel publishes one word per tile:
//   bits 0..15  the tile's per-level change flags (level L <-> generation L+1)
//   kDirty      some owned word of the tile differs from the block's input
//   kTop/kBot   ... in its first / last T rows (what the tiles above and
//               below read of it)
//   kLeft/kRight ... in its first / last owned word column (what the strips
//               beside it read: T <= 16 cells, less than one 32-cell word)
// A skipped tile re-publishes its previous word: with its whole cone unchanged
// every level row repeats the previous block's, flags included.
#pragma once

#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#define GOL_HD __host__ __device__
#else
#define GOL_HD
#endif

namespace gol {
namespace quiet {

constexpr uint32_t kFlagMask = 0xFFFFu;
constexpr uint32_t kDirty = 1u << 16, kTop = 1u << 17, kBot = 1u << 18, kLeft = 1u << 19, kRight = 1u << 20;
constexpr uint32_t kCols = 1u << 21;  // the tile's column records are valid (below: Column records)

// nb[3 * r + c]: the previous block's words of the tile (nb[4]) and its eight
// neighbours on the torus of tiles, row r - 1 below/above (0 = above), strip
// c - 1 beside (0 = left).  Corner tiles are read through their T x T-cell
// corner only, which is dirty only if both of its edges are.
GOL_HD inline bool may_skip(const uint32_t* nb) {
  const auto both = [](uint32_t w, uint32_t a, uint32_t b) { return (w & a) != 0u && (w & b) != 0u; };
  if (nb[4] & kDirty) return false;
  if ((nb[1] & kBot) || (nb[7] & kTop) || (nb[3] & kRight) || (nb[5] & kLeft)) return false;
  if (both(nb[0], kBot, kRight) || both(nb[2], kBot, kLeft)) return false;
  if (both(nb[6], kTop, kRight) || both(nb[8], kTop, kLeft)) return false;
  return true;
}

// ---- The candidate list (tuning quiet_list) ----
// A tile's skip test reads the nine words of its 3 x 3 neighbourhood.  A
// skipped tile republishes its word unchanged, so if no tile of that
// neighbourhood computed in block n, the nine words - and with them the
// decision, the rows and the tile's own word in both maps - are in block n + 1
// what they were in block n: only the neighbours of the tiles that computed
// need a launch - and of those only the neighbours of tiles whose word
// changed: a tile that computed and published the word it had published before
// (an oscillator or a glider inside a tile) leaves the tiles around it the
// inputs they had.  A tile that computed is launched in the next block in any
// case, where it writes the other map.
GOL_HD inline bool marks_neighbours(uint32_t old_word, uint32_t new_word) {
  return ((old_word ^ new_word) & ~kCols) != 0u;  // kCols says nothing about the tile's cells
}

// ---- Column records (tuning quiet_cols) ----
// What holds for a tile holds for each of its word columns: T <= 16 < 32
// cells, so the light cone of word column c over the tile's rows is columns
// c - 1 .. c + 1 over those rows and T rows above and below.  Beside its word a
// tile may publish one record per lane column (kColLanes of them: lane 0 and
// the lanes past the strip's owned columns are not used), the bits of a tile
// word restricted to that column: its level flags, kDirty, kTop, kBot.  The
// tile word is the OR of the owned columns' records, kLeft / kRight the dirty
// bits of the first and last owned column.  kCols in a tile word of a map:
// that map holds the tile's records of the block that published the word.
// Records are kept per row band of the tile (the column kernel's units), a
// reader ORs the bands.
constexpr int kColLanes = 64;
constexpr uint32_t kColMask = kFlagMask | kDirty | kTop | kBot;
// The record every column of a tile without valid records is taken to have.
GOL_HD inline uint32_t col_standin(uint32_t word) { return word & (kDirty | kTop | kBot); }
// Whether a column makes the columns beside it (and itself) recompute: above,
// same, below are its records in the tile above, the tile and the tile below.
GOL_HD inline bool col_source(uint32_t above, uint32_t same, uint32_t below) {
  return ((same & kDirty) | (above & kBot) | (below & kTop)) != 0u;
}
// src: bit j = col_source of lane column j of the strip, j = 1 .. own; bit 0
// that of the last owned column of the strip to the left, bit own + 1 that of
// the first owned column of the strip to the right.  Returns the owned
// columns whose cone holds a source.
GOL_HD inline uint64_t window_spread(uint64_t src, int own) {
  const uint64_t owned = ((own >= 63 ? ~0ull : (1ull << (own + 1)) - 1ull)) & ~1ull;
  return (src | src << 1 | src >> 1) & owned;
}
// The columns of the centre tile to recompute.  rec[i]: the kColLanes records
// of tile i of the neighbourhood (as may_skip's nb[], bands ORed), or null
// where words[i] lacks kCols (col_standin then).  own_l, own, own_r: owned
// columns of the strip to the left, the tile's strip and the strip to the
// right.  A tile whose own records are not valid recomputes every column.
GOL_HD inline uint64_t window(const uint32_t* const* rec, const uint32_t* words, int own_l, int own, int /*own_r*/) {
  const uint64_t owned = window_spread(~0ull, own);
  if (!(words[4] & kCols) || !rec[4]) return owned;
  const auto at = [&](int i, int j) { return (words[i] & kCols) && rec[i] ? rec[i][j] : col_standin(words[i]); };
  uint64_t src = 0;
  if (col_source(at(0, own_l), at(3, own_l), at(6, own_l))) src |= 1ull;
  for (int j = 1; j <= own; ++j)
    if (col_source(at(1, j), at(4, j), at(7, j))) src |= 1ull << j;
  if (col_source(at(2, 1), at(5, 1), at(8, 1))) src |= 1ull << (own + 1);
  return window_spread(src, own);
}
// The column kernel computes whole groups of `g` adjacent owned columns
// (group q: lane columns 1 + q g ...): the groups the window meets, one bit
// each, and the columns of those groups.  A computing tile whose window is
// empty (may_skip reads a corner tile more coarsely than the records do)
// computes its first group.
GOL_HD inline uint32_t window_groups(uint64_t win, int own, int g) {
  uint32_t hit = 0;
  for (int q = 0; q * g < own; ++q)
    if ((win >> (1 + q * g)) & ((1ull << g) - 1ull)) hit |= 1u << q;
  return hit ? hit : 1u;
}
GOL_HD inline uint64_t group_columns(uint32_t hit, int own, int g) {
  uint64_t m = 0;
  for (int q = 0; q * g < own; ++q)
    if ((hit >> q) & 1u) m |= ((1ull << g) - 1ull) << (1 + q * g);
  return m & window_spread(~0ull, own);
}

// Tile i (0..8, row-major as may_skip's nb[]) of the neighbourhood of tile
// (strip kcol, group grp) on the torus of ncolw x nseg tiles.  The relation is
// symmetric: the tiles that read a tile's word are its neighbourhood.
GOL_HD inline int neighbour(int kcol, int grp, int i, int ncolw, int nseg) {
  const int g = (grp + i / 3 - 1 + nseg) % nseg;
  const int k = (kcol + i % 3 - 1 + ncolw) % ncolw;
  return k * nseg + g;
}

// Change flags of the tiles that are not launched: per level, how many tiles'
// current word has the level's flag, kFlagsPerWord levels of kFlagBits bits
// to a 64-bit counter word (fewer than 2^20 tiles).  A computing tile adds the
// difference between its new and its old word; the borrows of a negative
// field cancel in the sum, which is the count of a set of tiles.
constexpr int kFlagBits = 21, kFlagsPerWord = 3;
constexpr int flag_words(int T) { return (T + kFlagsPerWord - 1) / kFlagsPerWord; }
GOL_HD inline unsigned long long flag_delta(uint32_t old_word, uint32_t new_word, int w) {
  unsigned long long d = 0;
  for (int j = 0; j < kFlagsPerWord; ++j) {
    const int L = w * kFlagsPerWord + j;
    if (L >= 16) break;
    const long long dl = (long long)((new_word >> L) & 1u) - (long long)((old_word >> L) & 1u);
    d += (unsigned long long)dl << (kFlagBits * j);
  }
  return d;
}
// The levels whose count in counter word w is not zero, as flag bits.
GOL_HD inline uint32_t flag_levels(unsigned long long count, int w) {
  uint32_t m = 0;
  for (int j = 0; j < kFlagsPerWord; ++j)
    if ((count >> (kFlagBits * j)) & ((1ull << kFlagBits) - 1)) m |= 1u << (w * kFlagsPerWord + j);
  return m & kFlagMask;
}

// What identifies the words a block published: a later block may read them
// only if it runs the same plan on the same buffers, swapped, and nothing
// else has written the grid in between (the engine's part: Chain::touch).
struct Launch {
  const void* in = nullptr;
  const void* out = nullptr;
  int T = 0;
  int64_t row_lo = 0, row_hi = 0, pitch = 0;
  int ncolw = 0, nseg = 0, seg_rows = 0, seg_rem = 0, grp_q = 0, wrap_w = 0;
};

inline bool same_plan(const Launch& a, const Launch& b) {
  return a.T == b.T && a.row_lo == b.row_lo && a.row_hi == b.row_hi && a.pitch == b.pitch && a.ncolw == b.ncolw &&
         a.nseg == b.nseg && a.seg_rows == b.seg_rows && a.seg_rem == b.seg_rem && a.grp_q == b.grp_q &&
         a.wrap_w == b.wrap_w;
}

// Whether block `cur` may skip on the words of block `prev`: `prev` was a
// detecting block (prev.T > 0), the plan is the same, and the buffers are
// prev's swapped - the destination still holds prev's input.
inline bool may_follow(const Launch& prev, const Launch& cur) {
  return prev.T > 0 && same_plan(prev, cur) && prev.in == cur.out && prev.out == cur.in;
}

// Engine policy (tuning quiet_skip): which kernel the next T-generation block
// runs.  Pure bookkeeping: a decision can never change a result, only which
// kernel computes it, so it may lag behind the device.
//   mode 0  never: today's kernels
//   mode 1  always the skipping kernel
//   mode -1 auto: the dense kernels, every `scout`-th block a detecting scout
//           (the skipping kernel; nothing precedes it, so nothing skips); once
//           a block reports at least `on` percent of its tiles clean, every
//           block runs the skipping kernel, until one reports fewer than
//           `off` percent skipped-or-clean tiles.
struct Policy {
  int mode = 0, scout = 128, on = 60, off = 35;
  bool skipping = false;
  int64_t since_scout = 0;
  int64_t blocks_dense = 0, blocks_scout = 0, blocks_skip = 0;

  // Whether the next block runs the skipping kernel.
  bool next() {
    if (mode == 0) return false;
    if (mode > 0 || skipping) return true;
    if (++since_scout >= scout) {
      since_scout = 0;
      return true;
    }
    return false;
  }
  void ran(bool quiet_kernel) {
    if (!quiet_kernel) ++blocks_dense;
    else if (mode < 0 && !skipping) ++blocks_scout;
    else ++blocks_skip;
  }
  // A block's report (possibly several blocks old): tiles, and how many of
  // them were clean after it (skipped tiles are clean).
  void report(int64_t tiles, int64_t clean) {
    if (mode >= 0 || tiles <= 0) return;
    const int64_t pct = 100 * clean / tiles;
    if (!skipping && pct >= on) skipping = true;
    else if (skipping && pct < off) {
      skipping = false;
      since_scout = 0;
    }
  }
  const char* name() const {
    return mode == 0 ? "off" : mode > 0 ? "on" : skipping ? "auto:skipping" : "auto:dense";
  }
};

#if !defined(__HIP_DEVICE_COMPILE__)
// Host model of the skipping kernel's candidate list, one call per block, as
// the kernel keeps it: two word maps, the launch stamps that de-duplicate the
// marks, the flag counts.  `fresh[t]` is the word tile t publishes if it
// computes in this block; `follow` false is a launch with no words to read
// (every tile computes, the next block evaluates every tile).
class ListModel {
 public:
  ListModel(int ncolw, int nseg, int T)
      : ncolw_(ncolw), nseg_(nseg), T_(T), stamp_(size_t(ncolw) * nseg, 0u), counts_(size_t(flag_words(T)), 0ull) {
    map_[0].assign(stamp_.size(), 0u);
    map_[1].assign(stamp_.size(), 0u);
  }
  // Runs one block; returns the tiles that computed, in launch order.
  std::vector<int> block(const std::vector<uint32_t>& fresh, bool follow) {
    const int tiles = int(stamp_.size());
    ++seq_;
    const std::vector<uint32_t>& prev = map_[cur_];
    std::vector<uint32_t>& next = map_[cur_ ^ 1];
    std::vector<int> items, marked, computed;
    if (!follow || all_) {
      for (int t = 0; t < tiles; ++t) items.push_back(t);
    } else {
      items = list_;
    }
    if (!follow) counts_.assign(counts_.size(), 0ull);
    launched_ = int64_t(items.size());
    for (int t : items) {
      const int kcol = t / nseg_, grp = t % nseg_;
      uint32_t nb[9];
      for (int i = 0; i < 9; ++i) nb[i] = prev[size_t(neighbour(kcol, grp, i, ncolw_, nseg_))];
      if (follow && may_skip(nb)) {
        next[size_t(t)] = nb[4];
        continue;
      }
      next[size_t(t)] = fresh[size_t(t)];
      computed.push_back(t);
      for (size_t w = 0; w < counts_.size(); ++w) counts_[w] += flag_delta(follow ? nb[4] : 0u, fresh[size_t(t)], int(w));
      if (!follow) continue;
      for (int i = 0; i < 9; ++i) {
        if (i != 4 && !marks_neighbours(nb[4], fresh[size_t(t)])) continue;
        const int n = neighbour(kcol, grp, i, ncolw_, nseg_);
        if (stamp_[size_t(n)] != seq_) {
          stamp_[size_t(n)] = seq_;
          marked.push_back(n);
        }
      }
    }
    list_ = marked;
    all_ = !follow;
    cur_ ^= 1;
    return computed;
  }
  // The tiles the next block launches (follow: as block()'s).
  std::vector<int> items(bool follow) const {
    if (follow && !all_) return list_;
    std::vector<int> v(stamp_.size());
    for (size_t t = 0; t < v.size(); ++t) v[t] = int(t);
    return v;
  }
  const std::vector<uint32_t>& words() const { return map_[cur_]; }       // the map the last block wrote
  const std::vector<uint32_t>& words_before() const { return map_[cur_ ^ 1]; }
  int64_t launched() const { return launched_; }                          // tiles the last block launched
  int64_t candidates() const { return all_ ? int64_t(stamp_.size()) : int64_t(list_.size()); }  // of the next block
  // Levels some tile's current word flags (what the kernel ORs into changed[]).
  uint32_t flags() const {
    uint32_t m = 0;
    for (size_t w = 0; w < counts_.size(); ++w) m |= flag_levels(counts_[w], int(w));
    return m & ((1u << T_) - 1u);
  }
  std::vector<int64_t> flag_counts() const {
    std::vector<int64_t> c(size_t(T_), 0);
    for (int L = 0; L < T_; ++L)
      c[size_t(L)] = int64_t((counts_[size_t(L / kFlagsPerWord)] >> (kFlagBits * (L % kFlagsPerWord))) & ((1ull << kFlagBits) - 1));
    return c;
  }

 private:
  int ncolw_, nseg_, T_, cur_ = 0;
  uint32_t seq_ = 0;
  bool all_ = true;
  int64_t launched_ = 0;
  std::vector<uint32_t> map_[2], stamp_;
  std::vector<int> list_;
  std::vector<unsigned long long> counts_;
};

// Host model of the column kernel on top of the list: per map, every tile's
// column records (bands ORed) and whether they are valid.  `fresh[t *
// kColLanes + j]` is the record column j of tile t publishes if it is
// computed in this block; `cols` false is a launch of the bodies that publish
// no records.  A computing tile of a column launch computes the groups of `g`
// columns its window meets and keeps the other columns' records; its word is
// the OR of both - which exactness makes the OR of all its fresh records.
class ColsModel {
 public:
  ColsModel(int ncolw, int nseg, int T, int last_own, int g)
      : list_(ncolw, nseg, T), ncolw_(ncolw), nseg_(nseg), last_own_(last_own), g_(g) {
    for (int m = 0; m < 2; ++m) {
      rec_[m].assign(size_t(ncolw) * nseg * kColLanes, 0u);
      valid_[m].assign(size_t(ncolw) * nseg, 0);
    }
  }
  int own(int kcol) const { return kcol == ncolw_ - 1 ? last_own_ : kColLanes - 2; }
  // The word of a tile from its columns' records.
  uint32_t word_of(const uint32_t* rec, int kcol) const {
    uint32_t w = 0;
    for (int j = 1; j <= own(kcol); ++j) w |= rec[j];
    if (rec[1] & kDirty) w |= kLeft;
    if (rec[own(kcol)] & kDirty) w |= kRight;
    return w;
  }
  // The window of tile t on the map the last block wrote.
  uint64_t window_of(int t) const {
    const int kcol = t / nseg_, grp = t % nseg_;
    const uint32_t* rec[9];
    uint32_t words[9];
    for (int i = 0; i < 9; ++i) {
      const int n = neighbour(kcol, grp, i, ncolw_, nseg_);
      words[i] = (list_.words()[size_t(n)] & ~kCols) | (valid_[cur_][size_t(n)] ? kCols : 0u);
      rec[i] = valid_[cur_][size_t(n)] ? &rec_[cur_][size_t(n) * kColLanes] : nullptr;
    }
    return window(rec, words, own((kcol + ncolw_ - 1) % ncolw_), own(kcol), own((kcol + 1) % ncolw_));
  }
  // Runs one block; returns per tile the columns computed (0: skipped or not launched).
  std::vector<uint64_t> block(const std::vector<uint32_t>& fresh, bool follow, bool cols) {
    const int tiles = ncolw_ * nseg_;
    const bool col_launch = cols && follow;
    std::vector<uint32_t> words(size_t(tiles), 0u), nrec(rec_[cur_ ^ 1]);
    std::vector<uint64_t> done(size_t(tiles), 0ull);
    const std::vector<int> items = list_.items(follow);
    for (int t : items) {
      const int kcol = t / nseg_;
      uint64_t cols_done = window_spread(~0ull, own(kcol));
      if (col_launch) cols_done = group_columns(window_groups(window_of(t), own(kcol), g_), own(kcol), g_);
      for (int j = 1; j <= own(kcol); ++j) {
        const size_t at = size_t(t) * kColLanes + j;
        nrec[at] = (cols_done >> j) & 1ull ? fresh[at] : rec_[cur_][at];
      }
      words[size_t(t)] = word_of(&nrec[size_t(t) * kColLanes], kcol);
      done[size_t(t)] = cols_done;
    }
    const std::vector<int> computed = list_.block(words, follow);
    std::vector<char> comp(size_t(tiles), 0);
    for (int t : computed) comp[size_t(t)] = 1;
    for (int t : items) {
      if (comp[size_t(t)]) {
        valid_[cur_ ^ 1][size_t(t)] = col_launch;
      } else {  // skipped: the word again, and (a column launch) its records
        valid_[cur_ ^ 1][size_t(t)] = col_launch && valid_[cur_][size_t(t)];
        for (int j = 0; j < kColLanes; ++j) nrec[size_t(t) * kColLanes + j] = rec_[cur_][size_t(t) * kColLanes + j];
        done[size_t(t)] = 0ull;
      }
    }
    rec_[cur_ ^ 1] = nrec;
    cur_ ^= 1;
    return done;
  }
  const ListModel& list() const { return list_; }
  const std::vector<uint32_t>& records() const { return rec_[cur_]; }
  bool valid(int t) const { return valid_[cur_][size_t(t)] != 0; }

 private:
  ListModel list_;
  int ncolw_, nseg_, last_own_, g_, cur_ = 0;
  std::vector<uint32_t> rec_[2];
  std::vector<char> valid_[2];
};
#endif  // !__HIP_DEVICE_COMPILE__

}  // namespace quiet
}  // namespace gol
