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
GOL_HD inline bool marks_neighbours(uint32_t old_word, uint32_t new_word) { return old_word != new_word; }

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
#endif  // !__HIP_DEVICE_COMPILE__

}  // namespace quiet
}  // namespace gol
