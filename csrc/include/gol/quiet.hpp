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

}  // namespace quiet
}  // namespace gol
