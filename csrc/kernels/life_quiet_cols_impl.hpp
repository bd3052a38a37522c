// The column kernel (gol/quiet.hpp, Column records; tuning quiet_cols): a
// third body for listed launches of the skipping kernel.  The grouped and the
// short-wave bodies recompute an active tile whole - every row of its 62 word
// columns - although what is active in it is almost always a spot a few words
// wide.  This body turns the wave round: the 64 lanes are rows, the word
// columns are registers, and a computing tile recomputes only the groups of
// G adjacent word columns whose light cone changed in the last block
// (quiet::window); the other columns keep their rows, as a skipped tile does,
// and their records.
//   Unit u of a launch = (item, row band, column group), one-wave workgroups
// striding over the units, right with any grid >= 1.  A band is 64 - 2T
// output rows of the tile with T rows of cone above and below (lane i holds
// row band + i - T); a unit loads G + 2 words of its lane's row - the group
// and a halo column on each side, at logical word indices, wrapped as
// lane_cols wraps them - and runs T levels on them: horizontal neighbours by
// funnel shifts between the column registers, vertical ones by one-lane wave
// shifts of the row's two horizontal-sum planes.  Level L + 1 is valid in
// lanes L + 1 .. 62 - L and, of a halo column, without the L + 1 cells at its
// outer edge (T <= 16 < 32).  The level-0 word stays in the lane, so the
// detection needs no reload.
//   Every unit of an item takes the same skip decision on the same nine words
// and derives the same window from the same records (a unit's input words are
// loaded alongside, before it knows whether it computes); the units of groups
// the window does not meet return once the window is known.  The others OR their share of the tile
// word into the tile's 64-bit accumulator and then add one to the arrival
// count in its upper half - two atomics of one lane on one word, so the OR
// precedes the add in that word's modification order; the unit whose add
// completes the count (bands x groups met, known to every unit) holds every
// share, stores the word and does what a group does for its tile.
#pragma once

#include "life_quiet_impl.hpp"

namespace gol {
namespace hipk {
namespace lb {

constexpr int kDppWaveShr1 = 0x138, kDppWaveShl1 = 0x130;

// OR over the wave's lanes.
__device__ __forceinline__ uint32_t wave_or(uint32_t v) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) v |= uint32_t(__shfl_xor(int(v), d, 64));
  return v;
}

template <int T, class IO, int G>
__global__ __launch_bounds__(64) void life_quiet_cols_kernel(const LifeBlockParams p) {
  static_assert(IO::W == 1 && IO::kBits && IO::XL == kXlaneDpp && IO::Rule::kDefault && T <= 16,
                "column kernel: bit layout, B3/S23");
  constexpr int kBandRows = 64 - 2 * T;
  constexpr int kWaveOut = wave_out_words<IO::XL, 1, 1>();
  constexpr int kGroupsMax = (kWaveOut + G - 1) / G;
  const int lane = threadIdx.x & 63;
  int n_items = int(__builtin_amdgcn_readlane(p.quiet_items[lane], 63));
  if (n_items == 0) {
    if (blockIdx.x == 0) quiet_complete<T, true>(p, 0ull, 0, lane);
    return;
  }
  const int nb = p.quiet_bands;
  const int upi = nb * kGroupsMax;  // units per item
  for (int u = blockIdx.x; u < n_items * upi; u += int(gridDim.x)) {
    const int item = u / upi;
    const int sub = u - item * upi;
    const int band = sub / kGroupsMax, q = sub - band * kGroupsMax;
    const int blk = quiet_item_tile(p, item, lane);
    const int kcol = blk / p.nseg;
    const int grp = blk - kcol * p.nseg;
    const int ww = p.wrap_w;
    const int own = min(kWaveOut, ww - kcol * kWaveOut);  // owned lane columns 1 .. own
    if (q * G >= own) continue;

    // The nine words, and with them (one round trip) the records this lane's
    // column reads: lanes 1 .. own the column itself in the tile and the tiles
    // above and below, lane 0 the last owned column of the strip to the left,
    // lane own + 1 the first of the strip to the right.
    const int side = lane == 0 ? 0 : lane == own + 1 ? 2 : 1;
    const int kside = (kcol + side - 1 + p.ncolw) % p.ncolw;
    const int jside = side == 1 ? lane : side == 2 ? 1 : min(kWaveOut, ww - kside * kWaveOut);
    uint32_t w = 0;
    if (lane < 9) w = p.quiet_prev[quiet::neighbour(kcol, grp, lane, p.ncolw, p.nseg)];
    // Branch-free, so that the loads are in flight together: every lane loads
    // (lanes past own + 1 a record nobody reads), bands past the last one load
    // the last one again.
    uint32_t r3[3] = {0u, 0u, 0u};
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      const int t = kside * p.nseg + (grp + r - 1 + p.nseg) % p.nseg;
      const uint32_t* const rt = p.quiet_rec_prev + size_t(t) * nb * quiet::kColLanes + jside;
#pragma unroll
      for (int b = 0; b < kQuietColBandsMax; ++b) r3[r] |= rt[min(b, nb - 1) * quiet::kColLanes];
    }
    // Rows: the tile's [G0, G1), the band's [b0, b0 + len) of them.  The
    // unit's input words are loaded now, before the words say whether it
    // computes: one round trip less on the chain of the tile that does.
    const int64_t G0 = p.row_lo + int64_t(grp) * p.seg_rows + min(grp, p.seg_rem);
    const int64_t G1 = G0 + p.seg_rows + (grp < p.seg_rem ? 1 : 0);
    const int64_t b0 = G0 + int64_t(band) * kBandRows;
    const int len = int(min<int64_t>(kBandRows, G1 - b0));
    const int hi = len + 2 * T - 1;  // last lane that holds a row of the band's cone
    const int64_t row = b0 - T + min(lane, max(hi, 0));
    const int j0 = 1 + q * G;                  // the group's first lane column
    const int lw0 = kcol * kWaveOut - 1 + j0;  // its logical word
    uint32_t c[G + 2];
    if (len > 0) {
      const uint32_t* const irow = reinterpret_cast<const uint32_t*>(p.in + row * p.pitch);
#pragma unroll
      for (int i = 0; i < G + 2; ++i) {
        const int lw = lw0 - 1 + i;
        c[i] = irow[p.own_w0 + ((lw % ww) + ww) % ww];
      }
    } else {
#pragma unroll
      for (int i = 0; i < G + 2; ++i) c[i] = 0u;
    }
    uint32_t nbw[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) nbw[i] = __builtin_amdgcn_readlane(w, i);
    if (quiet::may_skip(nbw)) {
      if (sub == 0) {  // re-publish the word, and its records with it
        const bool valid = (nbw[4] & quiet::kCols) != 0u;
        if (valid)
          for (int b = 0; b < nb; ++b) {
            const size_t at = (size_t(blk) * nb + b) * quiet::kColLanes + lane;
            p.quiet_rec_next[at] = p.quiet_rec_prev[at];
          }
        if (lane == 0) p.quiet_next[blk] = nbw[4];
        quiet_done_list<T, true>(p, item, n_items, true, true, lane);
      }
      continue;
    }
    const uint32_t old_word = nbw[4];

    // The window (quiet::window, with the lanes as columns).
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      const uint32_t wr = side == 0 ? nbw[3 * r] : side == 2 ? nbw[3 * r + 2] : nbw[3 * r + 1];
      if (!(wr & quiet::kCols)) r3[r] = quiet::col_standin(wr);
    }
    const uint64_t src = __ballot(lane <= own + 1 && quiet::col_source(r3[0], r3[1], r3[2]));
    const uint64_t win = (old_word & quiet::kCols) ? quiet::window_spread(src, own) : quiet::window_spread(~0ull, own);
    const uint32_t hit = quiet::window_groups(win, own, G);
    if (!((hit >> q) & 1u)) continue;
    const int nhit = __popc(hit);
    const bool first = (hit & ((1u << q) - 1u)) == 0u;  // the first group met: it also carries the columns not computed

    uint32_t share = 0;
    uint32_t rec[G];  // the band's records of the group's columns (a tile one row shorter may end before the band: none)
#pragma unroll
    for (int i = 0; i < G; ++i) rec[i] = 0u;
    if (len > 0) {
      uint32_t in0[G], fm[G];
      bool owned[G];
#pragma unroll
      for (int i = 0; i < G; ++i) {
        in0[i] = c[i + 1];
        owned[i] = j0 + i <= own;
        fm[i] = owned[i] ? (lw0 + i == ww - 1 ? p.last_mask : ~0u) : 0u;
      }
      // Levels L with L + 1 <= lane <= hi - L - 1 are valid in this lane.
      const int nvalid = max(0, min(min(lane, hi - lane), T));
      const uint32_t vmask = (1u << nvalid) - 1u;
      uint32_t f[G];
#pragma unroll
      for (int i = 0; i < G; ++i) f[i] = 0u;
#pragma unroll
      for (int L = 0; L < T; ++L) {
        uint32_t h0[G + 2], h1[G + 2];
#pragma unroll
        for (int i = 0; i < G + 2; ++i) {
          const uint32_t l = __builtin_amdgcn_alignbit(c[i], i == 0 ? 0u : c[i - 1], 31);       // cell x - 1
          const uint32_t r = __builtin_amdgcn_alignbit(i == G + 1 ? 0u : c[i + 1], c[i], 1);    // cell x + 1
          h0[i] = bop3<tt::XOR3>(l, c[i], r);
          h1[i] = bop3<tt::MAJ>(l, c[i], r);
        }
#pragma unroll
        for (int i = 0; i < G + 2; ++i) {
          const uint32_t a0 = uint32_t(__builtin_amdgcn_mov_dpp(int(h0[i]), kDppWaveShr1, 0xF, 0xF, true));  // row above
          const uint32_t a1 = uint32_t(__builtin_amdgcn_mov_dpp(int(h1[i]), kDppWaveShr1, 0xF, 0xF, true));
          const uint32_t d0 = uint32_t(__builtin_amdgcn_mov_dpp(int(h0[i]), kDppWaveShl1, 0xF, 0xF, true));  // row below
          const uint32_t d1 = uint32_t(__builtin_amdgcn_mov_dpp(int(h1[i]), kDppWaveShl1, 0xF, 0xF, true));
          const uint32_t nxt = rule(a0, a1, h0[i], h1[i], d0, d1, c[i]);
          if (i >= 1 && i <= G) f[i - 1] |= ((nxt ^ c[i]) & fm[i - 1]) != 0u ? 1u << L : 0u;
          c[i] = nxt;
        }
      }
      // Stores, and the detection against the level-0 words.
      const bool out_row = lane >= T && lane < T + len;
      const bool top = row < G0 + T, bot = row >= G1 - T;
      uint32_t* const orow = reinterpret_cast<uint32_t*>(p.out + row * p.pitch);
#pragma unroll
      for (int i = 0; i < G; ++i) {
        const int lw = lw0 + i;  // owned: 0 <= lw < ww
        if (out_row && owned[i]) orow[p.own_w0 + lw] = c[i + 1];
        const bool dirty = out_row && ((c[i + 1] ^ in0[i]) & fm[i]) != 0u;
        uint32_t v = f[i] & vmask;
        if (dirty) v |= quiet::kDirty | (top ? quiet::kTop : 0u) | (bot ? quiet::kBot : 0u);
        rec[i] = wave_or(v);
      }
    }
    // The band's records of the group's columns, and the unit's share.
    {
#pragma unroll
      for (int i = 0; i < G; ++i) {
        if (j0 + i > own) continue;  // wave-uniform
        if (lane == 0) p.quiet_rec_next[(size_t(blk) * nb + band) * quiet::kColLanes + j0 + i] = rec[i];
        share |= rec[i];
        if (j0 + i == 1 && (rec[i] & quiet::kDirty)) share |= quiet::kLeft;
        if (j0 + i == own && (rec[i] & quiet::kDirty)) share |= quiet::kRight;
      }
    }
    // The columns that are not computed keep this band's records.
    if (first) {
      const uint64_t done_cols = quiet::group_columns(hit, own, G);
      uint32_t keep = 0;
      const size_t at = (size_t(blk) * nb + band) * quiet::kColLanes + lane;
      const bool kept = lane >= 1 && lane <= own && !((done_cols >> lane) & 1ull);
      if (kept) {  // a tile without valid records computes every column
        keep = p.quiet_rec_prev[at];
        p.quiet_rec_next[at] = keep;
      }
      uint32_t kw = wave_or(keep);
      if (__ballot(kept && lane == 1 && (keep & quiet::kDirty)) != 0ull) kw |= quiet::kLeft;
      if (__ballot(kept && lane == own && (keep & quiet::kDirty)) != 0ull) kw |= quiet::kRight;
      share |= kw;
    }
    share = __builtin_amdgcn_readfirstlane(share);
    unsigned long long got = 0;
    if (lane == 0) {
      unsigned long long* const acc = p.quiet_acc + blk;
      if (share != 0u) (void)__hip_atomic_fetch_or(acc, (unsigned long long)share, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      got = __hip_atomic_fetch_add(acc, 1ull << 32, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    const uint32_t arrived = __builtin_amdgcn_readfirstlane(uint32_t(got >> 32)) + 1u;
    if (arrived != uint32_t(nb * nhit)) continue;  // another unit of the tile finishes it
    const uint32_t gw = __builtin_amdgcn_readfirstlane(uint32_t(got)) | quiet::kCols;
    if (lane == 0) {
      __hip_atomic_store(p.quiet_acc + blk, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      p.quiet_next[blk] = gw;
      __hip_atomic_fetch_add(p.quiet_count + kQuietCountStride * kQuietColsComputed,
                             (unsigned long long)__popcll(quiet::group_columns(hit, own, G)), __ATOMIC_RELAXED,
                             __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_fetch_add(p.quiet_count + kQuietCountStride * kQuietColsOfTiles, (unsigned long long)own,
                             __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    quiet_listed<T>(p, blk, kcol, grp, old_word, gw, lane);
    quiet_done_list<T, true>(p, item, n_items, (gw & quiet::kDirty) == 0u, false, lane);
  }
}

}  // namespace lb
}  // namespace hipk
}  // namespace gol
