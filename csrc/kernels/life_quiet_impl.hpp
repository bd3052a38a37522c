// Quiet-tile skipping (gol/quiet.hpp): the grouped temporal-blocking kernel of
// life_group_impl.hpp for the symmetric DPP window - whose storage frame does
// not move, so an unchanged tile needs no store at all - with
//   * detection fused into the row stores: for every output word it stores, a
//     wave reloads the input word at the same position (an L2 hit: the wave
//     read it about 2T rows earlier) and ORs out ^ in into per-lane
//     accumulators for the whole tile and for its first and last T rows; the
//     edge word columns fall out of the per-lane accumulator.  Each group
//     publishes one word per block (quiet::kDirty ... kRight and its change
//     flags);
//   * the skip test, wave-uniform and before the prologue: every wave of a
//     group reads the previous block's words of its tile and the eight tiles
//     around it (the torus of tiles: the block covers a row ring's owned rows
//     in wrap mode) and the whole group returns if quiet::may_skip allows.  A
//     skipping group re-publishes its word, ORs its stored flag mask into
//     changed[] and counts itself.  Skipping is per group: every wave of a
//     group takes the same decision, so no wave waits at a barrier for rows a
//     skipped wave never saved.
//   * the candidate list (LIST; gol/quiet.hpp, tuning quiet_list): a launch
//     runs only the tiles the last launch listed - those that computed, and
//     the neighbours of those whose word changed; nothing else can decide
//     differently - one item per group.  Tiles that are not launched keep
//     their rows and their words in both maps; their change flags reach
//     changed[] through per-level counts that follow every computing tile's
//     word, summed by the group that ends the launch (quiet_complete);
//   * short waves (life_quiet_chunk_kernel, tuning quiet_chunks): where the
//     list is short, every item runs as K one-wave workgroups of the classic
//     body instead of one 4-wave group;
//   * the column kernel (life_quiet_cols_impl.hpp, tuning quiet_cols): a
//     computing tile recomputes only the word columns near activity.  The
//     bodies here publish no column records: their words lack quiet::kCols.
// No folded strip, no chained or linked groups: the plan is regular, so the
// tile of block (strip, group) is the same rows and words in every launch of
// the same plan (quiet::may_follow).  No group ever waits for another.
#pragma once

#include "life_group_impl.hpp"

namespace gol {
namespace hipk {
namespace lb {

// Writer<IO> plus the detection.  The reload of row r is consumed one row
// later (or in finish()), so its latency hides behind a row's level bodies.
template <class IO>
struct QuietWriter {
  static_assert(IO::W == 1 && IO::kBits, "quiet tiles: bit layout, one word per lane");
  Writer<IO> w;
  const uint8_t* in;       // input row of Writer row index 0
  int top_end, bot_begin;  // row indices below / from which a row is one of the tile's first / last T
  uint32_t dall = 0, dtop = 0, dbot = 0;
  uint32_t pin = 0, pout = 0, ptop = 0, pbot = 0;
  __device__ __forceinline__ void flush() {
    const uint32_t d = pin ^ pout;
    dall |= d;
    dtop |= d & ptop;
    dbot |= d & pbot;
  }
  __device__ __forceinline__ void row(int64_t r, const Vec<1>& v) {
    flush();
    w.row(r, v);
    // Lanes that own no word read past num_records: the range check returns 0.
    const BufRsrc rs =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(in + r * w.pitch), short(0), int(w.pitch), kBufFlags);
    pin = __builtin_amdgcn_raw_buffer_load_b32(rs, w.own[0] ? w.col * 4 : Writer<IO>::kDrop, 0, 0);
    pout = v.w[0];  // lanes that own no word: masked out at the end (fmask)
    ptop = r < top_end ? ~0u : 0u;  // wave-uniform
    pbot = r >= bot_begin ? ~0u : 0u;
  }
};

// One report per launch, counted in two levels so that thousands of groups
// do not queue on one word: item i adds itself to counter i % 64 (a cache line
// each); the one that completes a counter adds its sum to the launch's
// counter, and the one that completes that (returns true, the totals in
// `tot`) resets it.  n_items: the items of the launch (a tile each); a launch
// of at most kQuietCounters items counts on the launch's counter at once (one
// atomic round trip less on the chain of the tile that ends the launch).
__device__ __forceinline__ bool quiet_count(const LifeBlockParams& p, int item, int n_items, bool clean, bool skipped,
                                            unsigned long long& tot) {
  const auto add = [](unsigned long long* c, unsigned long long v) {
    return __hip_atomic_fetch_add(c, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + v;
  };
  const auto put = [](unsigned long long* c, unsigned long long v) {
    __hip_atomic_store(c, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  };
  const unsigned long long mine = 1ull | (clean ? 1ull << 20 : 0ull) | (skipped ? 1ull << 40 : 0ull);
  if (unsigned(n_items) <= kQuietCounters) {  // nothing to spread: every first-level counter would take one item
    tot = add(p.quiet_count, mine);
    if ((tot & 0xFFFFFull) != unsigned(n_items)) return false;
    put(p.quiet_count, 0ull);
    return true;
  }
  const unsigned slot = unsigned(item) % kQuietCounters;
  unsigned long long* const c1 = p.quiet_count + kQuietCountStride * (2 + slot);
  tot = add(c1, mine);
  if ((tot & 0xFFFFFull) != (unsigned(n_items) - slot + kQuietCounters - 1) / kQuietCounters) return false;
  put(c1, 0ull);
  tot = add(p.quiet_count, tot);
  if ((tot & 0xFFFFFull) != unsigned(n_items)) return false;
  put(p.quiet_count, 0ull);
  return true;
}

// The launch's report (one lane): `clean` and `skipped` tiles of this launch,
// the tiles skipped by every launch so far - launches follow each other on
// one stream, so this lane is that word's only writer - and, from a list
// launch, the next block's candidates.  `before`: quiet_total(), which
// depends on nothing in the launch - the caller loads it together with
// whatever else it has to load.
__device__ __forceinline__ unsigned long long quiet_total(const LifeBlockParams& p) {
  return __hip_atomic_load(p.quiet_count + kQuietCountStride, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
template <bool LIST>
__device__ __forceinline__ void quiet_publish(const LifeBlockParams& p, unsigned long long before, unsigned long long clean,
                                              unsigned long long skipped, unsigned long long next_items) {
  unsigned long long* const call = p.quiet_count + kQuietCountStride;
  const unsigned long long all = before + skipped;
  __hip_atomic_store(call, all, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const unsigned long long seq = (unsigned long long)(p.quiet_seq & 0xFFFFFFu) << 40;
  __hip_atomic_store(p.quiet_report + 1, all, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  if constexpr (LIST) __hip_atomic_store(p.quiet_report + 2, seq | next_items, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  __hip_atomic_store(p.quiet_report, seq | (clean << 20) | skipped, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// The end of a list launch, by one whole wave, after every item has counted
// itself (`tot`: their totals; the tiles that were not launched are clean and
// skipped): the sub-lists' append counts become the next block's inclusive
// ends and are reset; changed[L] is set where some tile's current word flags
// level L (the flag counts: exact, launched or not); the other flag-count set
// and the next launch's ticket are zeroed.  Everything another group handed
// over is read with 64-bit agent-scope atomics, as it was written, and every
// load of this wave is issued before the first is used: the append count, the
// flag counts, the running total of quiet_publish and the column kernel's
// totals cost one round trip, not one after the other.
// COLS (the column kernel): its totals reach the host as well.
template <int T, bool COLS = false>
__device__ __forceinline__ void quiet_complete(const LifeBlockParams& p, unsigned long long tot, int n_items, int lane) {
  using LW = QuietListWords;
  unsigned long long* const cnt = p.quiet_lc + LW::kAppend + lane * kQuietCountStride;
  unsigned long long* const f = p.quiet_lc + LW::kFlags + p.quiet_fset * LW::kFlagSet + lane * kQuietCountStride;
  unsigned long long* const fo = p.quiet_lc + LW::kFlags + (p.quiet_fset ^ 1) * LW::kFlagSet + lane * kQuietCountStride;
  const unsigned long long appended = __hip_atomic_load(cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  unsigned long long fc[quiet::flag_words(T)];
#pragma unroll
  for (int w = 0; w < quiet::flag_words(T); ++w) fc[w] = __hip_atomic_load(f + w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const unsigned long long before = quiet_total(p);
  unsigned long long col_tot[2] = {0ull, 0ull};
  if constexpr (COLS) {
#pragma unroll
    for (int i = 0; i < 2; ++i)
      col_tot[i] = __hip_atomic_load(p.quiet_count + kQuietCountStride * (kQuietColsComputed + i), __ATOMIC_RELAXED,
                                     __HIP_MEMORY_SCOPE_AGENT);
  }
  uint32_t c = uint32_t(min(appended, (unsigned long long)p.quiet_cap));  // appends past the capacity were dropped (never: one per tile)
  __hip_atomic_store(cnt, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t t = uint32_t(__builtin_amdgcn_ds_bpermute(((lane - d) & 63) * 4, int(c)));  // lane - d's
    if (lane >= d) c += t;
  }
  p.quiet_items_next[lane] = c;
  const uint32_t n_next = __builtin_amdgcn_readlane(c, 63);
  uint32_t levels = 0;
#pragma unroll
  for (int w = 0; w < quiet::flag_words(T); ++w) {
    levels |= quiet::flag_levels(fc[w], w);
    __hip_atomic_store(fo + w, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  uint32_t any = 0;
#pragma unroll
  for (int L = 0; L < T; ++L) any |= (__ballot((levels >> L) & 1u) != 0ull ? 1u : 0u) << L;
  if (p.quiet_prev && p.changed && lane < T && ((any >> lane) & 1u)) p.changed[lane] = 1u;
  if (lane == 0) {
    __hip_atomic_store(p.quiet_lc + LW::kTicket + ((p.quiet_seq + 1) & 1u) * kQuietCountStride, 0ull, __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
    const unsigned long long rest = (unsigned long long)(p.ncolw * p.nseg - n_items);
    if constexpr (COLS) {
#pragma unroll
      for (int i = 0; i < 2; ++i) __hip_atomic_store(p.quiet_report + 3 + i, col_tot[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    // A launch with nothing to follow appended nothing: the next block runs every tile.
    quiet_publish<true>(p, before, ((tot >> 20) & 0xFFFFFull) + rest, (tot >> 40) + rest,
                        p.quiet_prev ? n_next : uint32_t(p.ncolw * p.nseg));
  }
}

// A whole wave counts item `item` of a list launch (lane 0 does) and ends the
// launch if it was the last.
template <int T, bool COLS = false>
__device__ __forceinline__ void quiet_done_list(const LifeBlockParams& p, int item, int n_items, bool clean, bool skipped,
                                                int lane) {
  unsigned long long tot = 0;
  int fin = 0;
  if (lane == 0) fin = quiet_count(p, item, n_items, clean, skipped, tot) ? 1 : 0;
  if (__builtin_amdgcn_readfirstlane(fin)) {
    const uint32_t lo = __builtin_amdgcn_readfirstlane(uint32_t(tot)), hi = __builtin_amdgcn_readfirstlane(uint32_t(tot >> 32));
    quiet_complete<T, COLS>(p, (unsigned long long)hi << 32 | lo, n_items, lane);
  }
}

// A skipped tile of the launch that counts the flags from zero (the block
// after a launch with nothing to follow: every tile is launched) adds its word.
template <int T>
__device__ __forceinline__ void quiet_recount(const LifeBlockParams& p, int blk, uint32_t word, int lane) {
  using LW = QuietListWords;
  if (lane < quiet::flag_words(T)) {
    const unsigned long long d = quiet::flag_delta(0u, word, lane);
    if (d != 0ull)
      __hip_atomic_fetch_add(p.quiet_lc + LW::kFlags + p.quiet_fset * LW::kFlagSet +
                                 (unsigned(blk) % kQuietCounters) * kQuietCountStride + lane,
                             d, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// What a computing tile of a list launch leaves for the next block and for
// the group that ends this one, by one whole wave once the tile's word `gw`
// is final (old_word: its word in the map this block read, 0 if none).
// Hand-over within a launch follows MI355X_MICROARCH.md, "Workgroup dispatch,
// XCD placement & inter-workgroup visibility", valid form "8-B agent atomics
// both sides": every word another group reads in this launch (append counts,
// flag counts, the counters of quiet_count, the chunk accumulators) is written
// and read with 64-bit agent-scope atomics only, and the wave waits for its
// own (s_waitcnt vmcnt(0)) before it counts itself - so no release or acquire
// fence, which would write back or invalidate a whole L2, is needed.  The
// plain stores (quiet_items_next, quiet_next, changed[], the rows) are read by
// later launches only: a reader of one of them within the launch would need
// those fences.
template <int T>
__device__ __forceinline__ void quiet_listed(const LifeBlockParams& p, int blk, int kcol, int grp, uint32_t old_word,
                                             uint32_t gw, int lane) {
  using LW = QuietListWords;
  // A launch with nothing to follow (a scout of the dense phase, the block
  // after an invalidation) sets changed[] itself, as the kernel without a list
  // does, and leaves the counts alone: the block after it, which launches
  // every tile, counts every word from zero (quiet_recount).
  if (!p.quiet_prev) {
    if (p.changed && lane < T && ((gw >> lane) & 1u)) p.changed[lane] = 1u;
    return;
  }
  const uint32_t counted = p.quiet_items ? old_word : 0u;
  // This tile is a candidate of the next block (its word says why it could
  // not skip), and so are the tiles that read its word if the word changed
  // (quiet::marks_neighbours), once each: the first to stamp a tile with
  // this launch's number appends it to the sub-list of its index.  (A
  // launch with no words to read computes every tile: the next block runs
  // them all and needs no list.)
  if (p.quiet_prev && lane < 9 && (lane == 4 || quiet::marks_neighbours(old_word, gw))) {
    const int t = quiet::neighbour(kcol, grp, lane, p.ncolw, p.nseg);
    if (__hip_atomic_exchange(p.quiet_stamp + t, p.quiet_seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != p.quiet_seq) {
      const unsigned s = unsigned(t) % kQuietCounters;
      const unsigned long long i = __hip_atomic_fetch_add(p.quiet_lc + LW::kAppend + s * kQuietCountStride, 1ull,
                                                          __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (i < (unsigned long long)p.quiet_cap) p.quiet_items_next[kQuietCounters + s * p.quiet_cap + unsigned(i)] = uint32_t(t);
    }
  }
  // The flag counts follow the tile's word: no atomic where nothing changed.
  if (lane < quiet::flag_words(T)) {
    const unsigned long long d = quiet::flag_delta(counted, gw, lane);
    if (d != 0ull)
      __hip_atomic_fetch_add(p.quiet_lc + LW::kFlags + p.quiet_fset * LW::kFlagSet +
                                 (unsigned(blk) % kQuietCounters) * kQuietCountStride + lane,
                             d, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  // The wave's atomics are performed before it counts itself: the group
  // that ends the launch reads them after every count.
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// One tile: the skip test, the block, the tile's word.  `item` of the
// launch's n_items counts it.
template <int T, class IO, int M, bool LIST>
__device__ __forceinline__ void quiet_tile(const LifeBlockParams& p, const int blk, const int item, const int n_items,
                                           const unsigned tid, uint32_t* saved, uint32_t* group_word) {
  constexpr int kSlot = (T - 1) * 2 * 64;  // dwords per boundary
  const int lane = tid & 63;
  const int m = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int kcol = blk / p.nseg;
  const int grp = blk - kcol * p.nseg;
  uint32_t* const ch = p.changed;  // never graph-replayed (gen_dev unset)

  // The tile is done (wave 0, lane 0 having stored its word): count it, and
  // end the launch with the last one.
  const auto done = [&](bool clean, bool skipped) {
    if constexpr (LIST) {
      quiet_done_list<T>(p, item, n_items, clean, skipped, lane);
    } else {
      unsigned long long tot = 0;
      if (lane == 0 && quiet_count(p, item, n_items, clean, skipped, tot))
        quiet_publish<false>(p, quiet_total(p), (tot >> 20) & 0xFFFFFull, tot >> 40, 0ull);
    }
  };

  uint32_t old_word = 0u;  // the tile's word in the map this block reads (none: its flags count from zero)
  if (p.quiet_prev) {  // wave-uniform: the nine words are the same for every wave of the group
    uint32_t w = 0;
    if (lane < 9) w = p.quiet_prev[quiet::neighbour(kcol, grp, lane, p.ncolw, p.nseg)];
    uint32_t nb[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) nb[i] = __builtin_amdgcn_readlane(w, i);
    if (quiet::may_skip(nb)) {
      if (m == 0) {
        if constexpr (!LIST) {  // a list launch: the flag counts already hold this word
          const uint32_t mask = nb[4] & quiet::kFlagMask;
          if (ch && lane < T && ((mask >> lane) & 1u)) ch[lane] = 1u;
        }
        if (lane == 0) p.quiet_next[blk] = nb[4] & ~quiet::kCols;  // this body copies no column records
        if constexpr (LIST) {
          if (!p.quiet_items) quiet_recount<T>(p, blk, nb[4], lane);
        }
        done(true, true);
      }
      return;
    }
    old_word = nb[4];
  }
  if (tid == 0) *group_word = 0u;  // ordered before its first use by the prologue barrier

  const auto group_end = [&](int g) {
    return p.row_lo + int64_t(g) * p.seg_rows + min(g, p.seg_rem) + p.seg_rows + (g < p.seg_rem ? 1 : 0);
  };
  const int64_t G1 = group_end(grp);
  const int64_t G0 = G1 - p.seg_rows - (grp < p.seg_rem ? 1 : 0);
  const int64_t in0 = G0 + int64_t(m) * p.grp_q - T;
  const bool last = m == M - 1;
  constexpr int kPro = 2 * T;
  const int kend = int(G1 + T - in0);
  const int kmain = last ? kend - (kend - kPro) % 3 : p.grp_q;
  const int nfull = last ? (kend - kPro) % 3 : 2 * T;

  const LaneCols<IO> lc = lane_cols<IO>(p, kcol, lane);
  const int64_t pitch = p.pitch;
  QuietWriter<IO> wr;
  RowReader<IO> rd;
  rd.ok[0] = lc.ok[0];
  wr.w.own[0] = lc.own[0];
  const uint32_t fmask = lc.fmask[0];

  Levels<T, 1> st;
#pragma unroll
  for (int L = 0; L < T; ++L) {
#pragma unroll
    for (int s = 0; s < 3; ++s) st.h0[L][s].w[0] = st.h1[L][s].w[0] = st.cc[L][s].w[0] = 0u;
    st.acc[L].w[0] = 0u;
  }

  rd.base = p.in + in0 * pitch;  // input row of step k: in0 + k
  rd.pitch = pitch;
  rd.kmax = last ? kend - 1 : kmain + 1;
  rd.off[0] = lc.off[0];
  rd.init();
  wr.w.out = p.out + in0 * pitch;  // level-T row of step k: in0 + k - T
  wr.w.pitch = pitch;
  wr.w.col = lc.store_col;
  wr.in = p.in + in0 * pitch;
  wr.top_end = int(G0 + T - in0);
  wr.bot_begin = int(G1 - T - in0);

  const LdsSaver<T, 1> saver{saved + m * kSlot, lane};
  prologue_tri<T, IO, 0>(st, rd, saver, NoBottom{});
  __syncthreads();  // every wave's boundary rows are in LDS

  int k = kPro;
  constexpr int S0 = kPro % 3, S1 = (S0 + 1) % 3, S2 = (S0 + 2) % 3;
  Prio prio((kmain - kPro) * T + epi_work<T>(nfull), false);
  for (; k + 3 <= kmain; k += 3) {
    prio.at((k - kPro) * T);
    wr.row(k - T, levels_full<T, IO, S0, 0, T>(st, rd.template take<S0>(k)));
    wr.row(k + 1 - T, levels_full<T, IO, S1, 0, T>(st, rd.template take<S1>(k + 1)));
    wr.row(k + 2 - T, levels_full<T, IO, S2, 0, T>(st, rd.template take<S2>(k + 2)));
  }
  prio.done0 = (kmain - kPro) * T;
  epilogue_tri<T, IO, 0, S0>(st, rd, saved + (last ? 0 : m + 1) * kSlot, lane, wr, k, nfull, prio);  // k == kmain
  prio.reset();
  wr.flush();

  // The wave's share of the tile word: change flags (as life_group_kernel's)
  // and the detection bits, masked to its owned words.
  uint32_t word = 0;
#pragma unroll
  for (int L = 0; L < T; ++L) word |= (__ballot((st.acc[L].w[0] & fmask) != 0u) != 0ull ? 1u : 0u) << L;
  if constexpr (!LIST) {
    if (ch && lane < T && ((word >> lane) & 1u)) ch[lane] = 1u;
  }
  const bool dirty = (wr.dall & fmask) != 0u;
  // First / last owned word column of the strip (wrap mode: logical words).
  constexpr int kWaveOut = wave_out_words<IO::XL, 1, 1>();
  const int lw = kcol * kWaveOut - 1 + lane;
  const bool left = lane == 1, right = lw == min(kcol * kWaveOut + kWaveOut, p.wrap_w) - 1;
  if (__ballot(dirty) != 0ull) word |= quiet::kDirty;
  if (__ballot((wr.dtop & fmask) != 0u) != 0ull) word |= quiet::kTop;
  if (__ballot((wr.dbot & fmask) != 0u) != 0ull) word |= quiet::kBot;
  if (__ballot(dirty && left) != 0ull) word |= quiet::kLeft;
  if (__ballot(dirty && right) != 0ull) word |= quiet::kRight;
  if (lane == 0) atomicOr(group_word, word);
  __syncthreads();
  if (m != 0) return;
  const uint32_t gw = *group_word;
  if (lane == 0) p.quiet_next[blk] = gw;
  if constexpr (LIST) quiet_listed<T>(p, blk, kcol, grp, old_word, gw, lane);
  done((gw & quiet::kDirty) == 0u, false);
}

// The tile of item `item` of a list launch (p.quiet_items null: every tile).
__device__ __forceinline__ int quiet_item_tile(const LifeBlockParams& p, int item, int lane) {
  if (!p.quiet_items) return item;
  // The sub-list whose range holds the item: as many ends are at or below it.
  const uint32_t end = p.quiet_items[lane];
  const int s = __builtin_amdgcn_readfirstlane(__popcll(__ballot(end <= uint32_t(item))));
  const uint32_t start = s > 0 ? __builtin_amdgcn_readlane(end, s - 1) : 0u;
  return __builtin_amdgcn_readfirstlane(p.quiet_items[kQuietCounters + s * p.quiet_cap + (item - int(start))]);
}

// LIST false: one workgroup per tile of the plan, blockIdx.x = strip * nseg +
// group.  LIST true: the candidate list (gol/quiet.hpp) - the launch's items
// are the tiles of p.quiet_items (null: every tile); groups beyond the list
// return.  Without LOOP the grid covers the list (the host launches one group
// per tile of the plan: it does not know the list's length) and group
// blockIdx.x runs item blockIdx.x.  With LOOP the grid may be any size >= 1: a
// group's first item is blockIdx.x, further ones come from the launch's
// ticket.  The loop costs registers (156 VGPRs against 122: three waves per
// SIMD instead of four), so it is a kernel of its own.
template <int T, class IO, int M, bool LIST = false, bool LOOP = false>
__global__ __launch_bounds__(64 * M) __attribute__((amdgpu_waves_per_eu(group_min_waves<T, IO>())))
void life_quiet_kernel(const LifeBlockParams p) {
  static_assert(IO::W == 1 && IO::XL == kXlaneDpp && IO::Rule::kDefault && T <= 16, "quiet tiles: DPP window, B3/S23");
  static_assert(LIST || !LOOP, "only a list launch loops");
  constexpr int kSlot = (T - 1) * 2 * 64;  // dwords per boundary
  __shared__ uint32_t saved[M * kSlot];
  __shared__ uint32_t group_word;
  if constexpr (!LIST) {
    quiet_tile<T, IO, M, false>(p, blockIdx.x, blockIdx.x, gridDim.x, threadIdx.x, saved, &group_word);
  } else {
    const int lane = threadIdx.x & 63;
    int n_items = p.ncolw * p.nseg;
    if (p.quiet_items) n_items = int(__builtin_amdgcn_readlane(p.quiet_items[lane], 63));
    if (n_items == 0) {  // nothing computed in the last block: nothing can change in this one
      if (blockIdx.x == 0 && threadIdx.x < 64) quiet_complete<T>(p, 0ull, 0, lane);
      return;
    }
    if constexpr (!LOOP) {
      const int item = blockIdx.x;
      if (item < n_items)
        quiet_tile<T, IO, M, true>(p, quiet_item_tile(p, item, lane), item, n_items, threadIdx.x, saved, &group_word);
    } else {
      __shared__ int next_item;
      for (int item = blockIdx.x; item < n_items;) {
        // Every iteration reads the parameters from the kernel-argument
        // segment anew and takes the thread index through an empty asm, so
        // that nothing derived from either is computed before the loop and
        // kept in registers across a tile: without it the kernel spills (63
        // SGPRs to lanes, 24 bytes of scratch at 168 VGPRs); with it, none.
        auto kargs = __builtin_amdgcn_kernarg_segment_ptr();
        asm volatile("" : "+s"(kargs));
        static_assert(sizeof(LifeBlockParams) % 4 == 0, "copied in dwords");
        const auto* const kw = (const __attribute__((address_space(4))) uint32_t*)kargs;  // scalar loads
        uint32_t qw[sizeof(LifeBlockParams) / 4];
#pragma unroll
        for (unsigned i = 0; i < sizeof(LifeBlockParams) / 4; ++i) qw[i] = kw[i];
        LifeBlockParams q;
        __builtin_memcpy(&q, qw, sizeof q);
        unsigned tid = threadIdx.x;
        asm volatile("" : "+v"(tid));
        quiet_tile<T, IO, M, true>(q, quiet_item_tile(q, item, int(tid & 63)), item, n_items, tid, saved, &group_word);
        if (int(gridDim.x) >= n_items) break;  // every item has a group of its own
        __syncthreads();  // the tile's LDS is free; every wave has read next_item
        if (threadIdx.x == 0)
          next_item = int(gridDim.x) + int(__hip_atomic_fetch_add(q.quiet_lc + QuietListWords::kTicket +
                                                                      (q.quiet_seq & 1u) * kQuietCountStride,
                                                                  1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
        __syncthreads();
        item = __builtin_amdgcn_readfirstlane(next_item);
      }
    }
  }
}

// Short waves for short lists (tuning quiet_chunks): the items of a list
// launch as K = p.quiet_chunks one-wave workgroups each, every one the classic
// body of life_block_kernel (a 2T-step prologue, no LDS, no barrier) over a
// K-th of the tile's output rows, so that an active tile's chain is 2T + rows
// / K steps long instead of a group's two triangles and a barrier.  Unit u =
// item * K + chunk; a wave runs units blockIdx.x, + gridDim.x, ...: right with
// any grid >= 1.  Every chunk wave of a tile reads the same nine words and
// takes the same decision; chunk 0 republishes for a skipped tile.  A
// computing tile's word is the OR of its waves' shares: each ORs its share
// and its arrival bit (32 + chunk) into the tile's 64-bit accumulator, and the
// wave that finds all other arrival bits there stores the word, resets the
// accumulator and does what a group does for its tile.  Nothing reads the new
// map or the rows within the launch.
template <int T, class IO>
__global__ __launch_bounds__(64) void life_quiet_chunk_kernel(const LifeBlockParams p) {
  static_assert(IO::W == 1 && IO::XL == kXlaneDpp && IO::Rule::kDefault && T <= 16, "quiet tiles: DPP window, B3/S23");
  const int lane = threadIdx.x & 63;
  const int K = p.quiet_chunks;
  int n_items = p.ncolw * p.nseg;
  if (p.quiet_items) n_items = int(__builtin_amdgcn_readlane(p.quiet_items[lane], 63));
  if (n_items == 0) {
    if (blockIdx.x == 0) quiet_complete<T>(p, 0ull, 0, lane);
    return;
  }
  for (int u = blockIdx.x; u < n_items * K; u += int(gridDim.x)) {
    const int item = u / K, chunk = u - item * K;
    const int blk = quiet_item_tile(p, item, lane);
    const int kcol = blk / p.nseg;
    const int grp = blk - kcol * p.nseg;
    uint32_t old_word = 0u;
    if (p.quiet_prev) {
      uint32_t w = 0;
      if (lane < 9) w = p.quiet_prev[quiet::neighbour(kcol, grp, lane, p.ncolw, p.nseg)];
      uint32_t nb[9];
#pragma unroll
      for (int i = 0; i < 9; ++i) nb[i] = __builtin_amdgcn_readlane(w, i);
      if (quiet::may_skip(nb)) {
        if (chunk == 0) {
          if (lane == 0) p.quiet_next[blk] = nb[4] & ~quiet::kCols;  // this body copies no column records
          if (!p.quiet_items) quiet_recount<T>(p, blk, nb[4], lane);
          quiet_done_list<T>(p, item, n_items, true, true, lane);
        }
        continue;
      }
      old_word = nb[4];
    }
    // The tile's rows [G0, G1), this wave's [o0, o1) of them (balanced).
    const int64_t G0 = p.row_lo + int64_t(grp) * p.seg_rows + min(grp, p.seg_rem);
    const int64_t G1 = G0 + p.seg_rows + (grp < p.seg_rem ? 1 : 0);
    const int64_t o0 = G0 + (G1 - G0) * chunk / K, o1 = G0 + (G1 - G0) * (chunk + 1) / K;

    const LaneCols<IO> lc = lane_cols<IO>(p, kcol, lane);
    const int64_t pitch = p.pitch;
    RowReader<IO> rd;
    QuietWriter<IO> wr;
    rd.ok[0] = lc.ok[0];
    wr.w.own[0] = lc.own[0];
    const uint32_t fmask = lc.fmask[0];
    Levels<T, 1> st;
#pragma unroll
    for (int L = 0; L < T; ++L) {
#pragma unroll
      for (int s = 0; s < 3; ++s) st.h0[L][s].w[0] = st.h1[L][s].w[0] = st.cc[L][s].w[0] = 0u;
      st.acc[L].w[0] = 0u;
    }
    constexpr int kPro = 2 * T;
    const int kend = kPro + int(o1 - o0);
    const int64_t in0 = o0 - T;
    rd.base = p.in + in0 * pitch;  // input row of step k: in0 + k
    rd.pitch = pitch;
    rd.kmax = kend - 1;
    rd.off[0] = lc.off[0];
    wr.w.out = p.out + in0 * pitch;  // level-T row of step k: in0 + k - T
    wr.w.pitch = pitch;
    wr.w.col = lc.store_col;
    wr.in = p.in + in0 * pitch;
    wr.top_end = int(G0 + T - in0);
    wr.bot_begin = int(G1 - T - in0);
    uint32_t word = 0;
    if (o0 < o1) {  // more chunks than rows: a wave without rows only arrives
      rd.init();
      prologue_tri<T, IO, 0>(st, rd, NoSave{}, NoBottom{});
      int k = kPro;
      constexpr int S0 = kPro % 3, S1 = (S0 + 1) % 3, S2 = (S0 + 2) % 3;
      for (; k + 3 <= kend; k += 3) {
        wr.row(k - T, levels_full<T, IO, S0, 0, T>(st, rd.template take<S0>(k)));
        wr.row(k + 1 - T, levels_full<T, IO, S1, 0, T>(st, rd.template take<S1>(k + 1)));
        wr.row(k + 2 - T, levels_full<T, IO, S2, 0, T>(st, rd.template take<S2>(k + 2)));
      }
      if (k < kend) {
        wr.row(k - T, levels_full<T, IO, S0, 0, T>(st, rd.template take<S0>(k)));
        if (k + 1 < kend) wr.row(k + 1 - T, levels_full<T, IO, S1, 0, T>(st, rd.template take<S1>(k + 1)));
      }
      wr.flush();
#pragma unroll
      for (int L = 0; L < T; ++L) word |= (__ballot((st.acc[L].w[0] & fmask) != 0u) != 0ull ? 1u : 0u) << L;
      const bool dirty = (wr.dall & fmask) != 0u;
      constexpr int kWaveOut = wave_out_words<IO::XL, 1, 1>();
      const int lw = kcol * kWaveOut - 1 + lane;
      const bool left = lane == 1, right = lw == min(kcol * kWaveOut + kWaveOut, p.wrap_w) - 1;
      if (__ballot(dirty) != 0ull) word |= quiet::kDirty;
      if (__ballot((wr.dtop & fmask) != 0u) != 0ull) word |= quiet::kTop;
      if (__ballot((wr.dbot & fmask) != 0u) != 0ull) word |= quiet::kBot;
      if (__ballot(dirty && left) != 0ull) word |= quiet::kLeft;
      if (__ballot(dirty && right) != 0ull) word |= quiet::kRight;
    }
    const unsigned long long mine = (unsigned long long)word | 1ull << (32 + chunk);
    unsigned long long got = 0;
    if (lane == 0) got = __hip_atomic_fetch_or(p.quiet_acc + blk, mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) | mine;
    const uint32_t arrived = __builtin_amdgcn_readfirstlane(uint32_t(got >> 32));
    if (arrived != (K >= 32 ? ~0u : (1u << K) - 1u)) continue;  // another wave of the tile finishes it
    const uint32_t gw = __builtin_amdgcn_readfirstlane(uint32_t(got));
    if (lane == 0) {
      __hip_atomic_store(p.quiet_acc + blk, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      p.quiet_next[blk] = gw;
    }
    quiet_listed<T>(p, blk, kcol, grp, old_word, gw, lane);
    quiet_done_list<T>(p, item, n_items, (gw & quiet::kDirty) == 0u, false, lane);
  }
}

// Plan: groups of about `seg` output rows (balanced), every wave but the last
// q rows with q >= 2T and (q - 2T) % 3 == 0 near the balance point, as
// plan_group.  Returns false when the rows are too few for one group.
template <int T, int M>
bool plan_quiet(LifeBlockParams& p, int64_t out_rows, int seg) {
  const int64_t min_rows = int64_t(M - 1) * 2 * T + 1;
  const int64_t n = std::min(std::max<int64_t>(1, out_rows / std::max<int64_t>(seg, min_rows)), out_rows / min_rows);
  if (n < 1) return false;
  const int64_t lo = out_rows / n, hi = lo + (out_rows % n ? 1 : 0);
  const int64_t ideal = std::max<int64_t>(2 * T, (hi + T - 1) / M);
  int q = 0;
  double span = 1e300;
  for (int64_t c = ideal - 3; c <= ideal + 3; ++c) {
    if (c < 2 * T || (c - 2 * T) % 3 != 0 || lo - int64_t(M - 1) * c < 0) continue;
    const double s = std::max<double>(double(c), double(hi - int64_t(M - 1) * c) + (T - 1));
    if (s < span) {
      span = s;
      q = int(c);
    }
  }
  if (q == 0) return false;
  p.nseg = int(n);
  p.seg_rows = int(lo);
  p.seg_rem = int(out_rows % n);
  p.grp_q = q;
  return true;
}

}  // namespace lb
}  // namespace hipk
}  // namespace gol
