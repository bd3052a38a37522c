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
// No folded strip, no chained or linked groups: the plan is regular, so the
// tile of block (strip, group) is the same rows and words in every launch of
// the same plan (quiet::may_follow).
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

template <int T, class IO, int M>
__global__ __launch_bounds__(64 * M) __attribute__((amdgpu_waves_per_eu(group_min_waves<T, IO>())))
void life_quiet_kernel(const LifeBlockParams p) {
  static_assert(IO::W == 1 && IO::XL == kXlaneDpp && IO::Rule::kDefault && T <= 16, "quiet tiles: DPP window, B3/S23");
  constexpr int kSlot = (T - 1) * 2 * 64;  // dwords per boundary
  __shared__ uint32_t saved[M * kSlot];
  __shared__ uint32_t group_word;
  const int lane = threadIdx.x & 63;
  const int m = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int blk = blockIdx.x;  // = the tile: strip * nseg + group
  const int kcol = blk / p.nseg;
  const int grp = blk - kcol * p.nseg;
  uint32_t* const ch = p.changed;  // never graph-replayed (gen_dev unset)

  // One report per launch, counted in two levels so that thousands of groups
  // do not queue on one word: group blk adds itself to counter blk % 64 (a
  // cache line each); the group that completes a counter adds its sum to the
  // launch's counter, and the one that completes that stores the totals.
  const auto count = [&](bool clean, bool skipped) {
    const auto add = [](unsigned long long* c, unsigned long long v) {
      return __hip_atomic_fetch_add(c, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + v;
    };
    const auto put = [](unsigned long long* c, unsigned long long v) {
      __hip_atomic_store(c, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    };
    const unsigned slot = unsigned(blk) % kQuietCounters;
    unsigned long long* const c1 = p.quiet_count + kQuietCountStride * (2 + slot);
    unsigned long long tot = add(c1, 1ull | (clean ? 1ull << 20 : 0ull) | (skipped ? 1ull << 40 : 0ull));
    if ((tot & 0xFFFFFull) != (gridDim.x - slot + kQuietCounters - 1) / kQuietCounters) return;
    put(c1, 0ull);
    tot = add(p.quiet_count, tot);
    if ((tot & 0xFFFFFull) != gridDim.x) return;
    put(p.quiet_count, 0ull);
    // Skipped tiles of every launch so far: launches follow each other on one
    // stream, so this group is the word's only writer.
    unsigned long long* const call = p.quiet_count + kQuietCountStride;
    const unsigned long long all = __hip_atomic_load(call, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + (tot >> 40);
    put(call, all);
    __hip_atomic_store(p.quiet_report + 1, all, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    const unsigned long long rep =
        ((unsigned long long)(p.quiet_seq & 0xFFFFFFu) << 40) | (((tot >> 20) & 0xFFFFFull) << 20) | (tot >> 40);
    __hip_atomic_store(p.quiet_report, rep, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  };

  if (p.quiet_prev) {  // wave-uniform: the nine words are the same for every wave of the group
    uint32_t w = 0;
    if (lane < 9) {
      const int g = (grp + lane / 3 - 1 + p.nseg) % p.nseg;
      const int k = (kcol + lane % 3 - 1 + p.ncolw) % p.ncolw;
      w = p.quiet_prev[k * p.nseg + g];
    }
    uint32_t nb[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) nb[i] = __builtin_amdgcn_readlane(w, i);
    if (quiet::may_skip(nb)) {
      if (m == 0) {
        const uint32_t mask = nb[4] & quiet::kFlagMask;
        if (ch && lane < T && ((mask >> lane) & 1u)) ch[lane] = 1u;
        if (lane == 0) {
          p.quiet_next[blk] = nb[4];
          count(true, true);
        }
      }
      return;
    }
  }
  if (threadIdx.x == 0) group_word = 0u;  // ordered before its first use by the prologue barrier

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
  if (ch && lane < T && ((word >> lane) & 1u)) ch[lane] = 1u;
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
  if (lane == 0) atomicOr(&group_word, word);
  __syncthreads();
  if (threadIdx.x == 0) {
    const uint32_t gw = group_word;
    p.quiet_next[blk] = gw;
    count((gw & quiet::kDirty) == 0u, false);
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
