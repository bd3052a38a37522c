// life_block variant: the quiet-tile skipping kernel (life_quiet_impl.hpp) on
// BitsIO<1, kXlaneDpp>, T = 12 in 4-wave groups.
#include "life_quiet_cols_impl.hpp"

namespace gol {
namespace hipk {

namespace {
constexpr int kQuietM = 4;
using QuietIO = lb::BitsIO<1, kXlaneDpp>;
constexpr int kColBandRows = 64 - 2 * kQuietT;

template <int G>
void launch_cols(const LifeBlockParams& p, int64_t grid, hipStream_t s) {
  hipLaunchKernelGGL((lb::life_quiet_cols_kernel<kQuietT, QuietIO, G>), dim3(unsigned(grid)), dim3(64), 0, s, p);
}
}  // namespace

// Up front, outside any timed run: the maps and counters of a tile of H rows
// and `words` owned words per row, whatever the plan, and the kernel's code
// object loaded (a first launch otherwise loads it).
void prepare_bits_w1_dpp_quiet(Scratch& scratch, int64_t H, int64_t words, bool list) {
  const int64_t min_rows = int64_t(kQuietM - 1) * 2 * kQuietT + 1;
  const int64_t tiles = ceil_div(words, int64_t(lb::wave_out_words<kXlaneDpp, 1>())) * std::max<int64_t>(1, H / min_rows);
  if (tiles >= (int64_t(1) << 20)) return;
  scratch.get(Scratch::kQuietMapA, size_t(tiles) * 4);
  scratch.get(Scratch::kQuietMapB, size_t(tiles) * 4);
  scratch.get(Scratch::kQuietCounters, kQuietCountBytes);
  hipFuncAttributes attr;
  if (list) {
    scratch.get(Scratch::kQuietList, QuietListLayout(tiles).bytes);
    (void)hipFuncGetAttributes(&attr, reinterpret_cast<const void*>(&lb::life_quiet_kernel<kQuietT, QuietIO, kQuietM, true, false>));
    (void)hipFuncGetAttributes(&attr, reinterpret_cast<const void*>(&lb::life_quiet_kernel<kQuietT, QuietIO, kQuietM, true, true>));
    (void)hipFuncGetAttributes(&attr, reinterpret_cast<const void*>(&lb::life_quiet_chunk_kernel<kQuietT, QuietIO>));
    // The column kernel's records: at most this many (tile, band) pairs,
    // whatever the plan (a band per kColBandRows rows and one more per tile).
    const int64_t strips = ceil_div(words, int64_t(lb::wave_out_words<kXlaneDpp, 1>()));
    const size_t rec_bytes = size_t(strips * (H / kColBandRows + 1) + tiles + tiles / 16) * quiet::kColLanes * 4;
    scratch.get(Scratch::kQuietRecA, rec_bytes);
    scratch.get(Scratch::kQuietRecB, rec_bytes);
    (void)hipFuncGetAttributes(&attr, reinterpret_cast<const void*>(&lb::life_quiet_cols_kernel<kQuietT, QuietIO, 2>));
    (void)hipFuncGetAttributes(&attr, reinterpret_cast<const void*>(&lb::life_quiet_cols_kernel<kQuietT, QuietIO, 4>));
    (void)hipFuncGetAttributes(&attr, reinterpret_cast<const void*>(&lb::life_quiet_cols_kernel<kQuietT, QuietIO, 8>));
  } else {
    (void)hipFuncGetAttributes(&attr, reinterpret_cast<const void*>(&lb::life_quiet_kernel<kQuietT, QuietIO, kQuietM, false>));
  }
  (void)hipGetLastError();
}

int64_t launch_bits_w1_dpp_quiet(const LifeBlockParams& p0, int64_t out_rows, int T, const LaunchCtx& ctx,
                                 hipStream_t s) {
  using IO = QuietIO;
  constexpr int M = kQuietM;
  QuietState* Q = ctx.quiet;
  // Wrap-mode blocks over exactly a row ring's owned rows: the tiles then form
  // a torus (life_quiet_kernel's neighbour words).  Stream launches only.
  if (!Q || T != kQuietT || p0.wrap_w <= 0 || p0.link_ring_rows != out_rows || p0.gen_dev) return 0;
  LifeBlockParams p = p0;
  p.ncolw = int(ceil_div(p.wrap_w, lb::wave_out_words<IO::XL, 1>()));
  p.fold = 1;
  p.fold_lanes = 64;
  if (!lb::plan_quiet<kQuietT, M>(p, out_rows, Q->seg_rows)) return 0;
  const int64_t tiles = int64_t(p.ncolw) * p.nseg;
  if (tiles >= (int64_t(1) << 20)) return 0;  // the packed counter's fields
  uint32_t* const maps[2] = {ctx.scratch->get(Scratch::kQuietMapA, size_t(tiles) * 4),
                             ctx.scratch->get(Scratch::kQuietMapB, size_t(tiles) * 4)};
  const quiet::Launch cur{p.in,    p.out,  T,          p.row_lo,   p.row_hi, p.pitch,
                          p.ncolw, p.nseg, p.seg_rows, p.seg_rem, p.grp_q,  p.wrap_w};
  const int next = Q->cur ^ 1;
  p.quiet_prev = quiet::may_follow(Q->prev, cur) ? maps[Q->cur] : nullptr;
  p.quiet_next = maps[next];
  p.quiet_count = reinterpret_cast<unsigned long long*>(ctx.scratch->get(Scratch::kQuietCounters, kQuietCountBytes));
  p.quiet_report = ctx.mail->quiet_report;
  p.quiet_seq = ++Q->seq;
  int64_t grid = tiles;
  if (Q->list) {
    // The candidate list: this launch's items are what the last launch
    // appended, if it followed a launch itself (else it computed every tile,
    // and every tile is evaluated now, which
    // counts the flags from zero, in the set the last launch zeroed).
    const QuietListLayout lay(tiles);
    uint8_t* const base = reinterpret_cast<uint8_t*>(ctx.scratch->get(Scratch::kQuietList, lay.bytes));
    const bool listed = p.quiet_prev && Q->listed;
    const int items_next = Q->items ^ 1;
    p.quiet_lc = reinterpret_cast<unsigned long long*>(base);
    p.quiet_stamp = reinterpret_cast<uint32_t*>(base + lay.stamp);
    p.quiet_items = listed ? reinterpret_cast<const uint32_t*>(base + lay.items[Q->items]) : nullptr;
    p.quiet_items_next = reinterpret_cast<uint32_t*>(base + lay.items[items_next]);
    p.quiet_cap = lay.cap;
    p.quiet_acc = reinterpret_cast<unsigned long long*>(base + lay.acc);
    if (p.quiet_prev && !listed) Q->fset ^= 1;
    p.quiet_fset = Q->fset;
    // What the newest finished launch reported for its successor (the host
    // does not know this launch's list length): valid if that launch listed.
    int64_t reported = -1;
    if (listed && ctx.mail_host) {
      const unsigned long long r = __atomic_load_n(&ctx.mail_host->quiet_report[2], __ATOMIC_ACQUIRE);
      int64_t n = int64_t((Q->seq - 1) & ~0xFFFFFFu) | int64_t(r >> 40);
      if (n > int64_t(Q->seq - 1)) n -= int64_t(1) << 24;
      if (r != 0 && Q->listed_since != 0 && n >= int64_t(Q->listed_since)) reported = int64_t(r & 0xFFFFFu);
    }
    const int64_t sized = reported >= 0 ? std::min<int64_t>(tiles, 2 * reported + 256) : tiles;
    // Short waves where the list is short: K one-wave workgroups per item,
    // forced (quiet_chunks = n: every list launch) or, by default, when K
    // times the reported length fits quiet_chunk_waves (-n: with K = n).  The
    // report lags, so twice that length and 256 items' worth of waves are
    // launched; the kernel strides over its units, whatever its grid.
    int K = 1;
    const int k_auto = Q->chunks < -1 ? -Q->chunks : kQuietChunksAuto;
    if (Q->chunks > 1) K = Q->chunks;
    else if (Q->chunks < 0 && reported >= 0 && reported * k_auto <= Q->chunk_waves) K = k_auto;
    K = std::max(1, std::min<int>(K, std::min<int>(kQuietChunksMax, p.seg_rows)));
    Q->chunks_last = K;
    // The grouped kernel's grid: by default one group per tile of the plan,
    // which covers any list - the groups beyond it return on their first load,
    // and the kernel needs no loop.  quiet_grid > 0 forces a grid, -1 takes
    // the size above; both run the looping kernel, right with any grid.
    // The column kernel (tuning quiet_cols): a listed launch - it reads a list
    // and the last launch's words - whose tiles fit its bands; forced, or by
    // default where the reported list is at most quiet_col_items long and
    // neither quiet_chunks nor quiet_grid forces another body.  Its units
    // stride over any grid, so it takes the short waves' sizing.
    const int bands = int(ceil_div(int64_t(p.seg_rows) + (p.seg_rem ? 1 : 0), int64_t(kColBandRows)));
    const bool cols = listed && bands <= kQuietColBandsMax &&
                      (Q->cols > 0 || (Q->cols < 0 && Q->chunks < 0 && Q->grid == 0 && reported >= 0 && reported <= Q->col_items));
    Q->cols_last = cols;
    if (cols) {
      const size_t rec_bytes = size_t(tiles) * bands * quiet::kColLanes * 4;
      uint32_t* const recs[2] = {ctx.scratch->get(Scratch::kQuietRecA, rec_bytes),
                                 ctx.scratch->get(Scratch::kQuietRecB, rec_bytes)};
      p.quiet_rec_prev = recs[Q->cur];
      p.quiet_rec_next = recs[next];
      p.quiet_bands = bands;
      Q->chunks_last = 1;
      grid = std::max<int64_t>(1, (Q->grid > 0 ? std::min<int64_t>(Q->grid, tiles) : sized) * kQuietChunksAuto);
      if (Q->col_group <= 2) launch_cols<2>(p, grid, s);
      else if (Q->col_group >= 8) launch_cols<8>(p, grid, s);
      else launch_cols<4>(p, grid, s);
    } else if (K > 1) {
      p.quiet_chunks = K;
      grid = (Q->grid > 0 ? std::min<int64_t>(Q->grid, tiles) : sized) * K;
      hipLaunchKernelGGL((lb::life_quiet_chunk_kernel<kQuietT, IO>), dim3(unsigned(grid)), dim3(64), 0, s, p);
    } else if (Q->grid != 0) {
      grid = Q->grid > 0 ? std::min<int64_t>(Q->grid, tiles) : sized;
      hipLaunchKernelGGL((lb::life_quiet_kernel<kQuietT, IO, M, true, true>), dim3(unsigned(grid)), dim3(64 * M), 0, s, p);
    } else {
      hipLaunchKernelGGL((lb::life_quiet_kernel<kQuietT, IO, M, true, false>), dim3(unsigned(grid)), dim3(64 * M), 0, s, p);
    }
    Q->listed = p.quiet_prev != nullptr;
    if (!Q->listed) Q->listed_since = 0;
    else if (Q->listed_since == 0) Q->listed_since = Q->seq;
    Q->items = items_next;
  } else {
    hipLaunchKernelGGL((lb::life_quiet_kernel<kQuietT, IO, M, false>), dim3(unsigned(tiles)), dim3(64 * M), 0, s, p);
  }
  Q->prev = cur;
  Q->cur = next;
  Q->tiles = tiles;
  Q->grid_last = grid;
  return tiles;
}

}  // namespace hipk
}  // namespace gol
