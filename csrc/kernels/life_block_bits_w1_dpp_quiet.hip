// life_block variant: the quiet-tile skipping kernel (life_quiet_impl.hpp) on
// BitsIO<1, kXlaneDpp>, T = 12 in 4-wave groups.
#include "life_quiet_impl.hpp"

namespace gol {
namespace hipk {

namespace {
constexpr int kQuietM = 4;
using QuietIO = lb::BitsIO<1, kXlaneDpp>;
}  // namespace

// Up front, outside any timed run: the maps and counters of a tile of H rows
// and `words` owned words per row, whatever the plan, and the kernel's code
// object loaded (a first launch otherwise loads it).
void prepare_bits_w1_dpp_quiet(Scratch& scratch, int64_t H, int64_t words) {
  const int64_t min_rows = int64_t(kQuietM - 1) * 2 * kQuietT + 1;
  const int64_t tiles = ceil_div(words, int64_t(lb::wave_out_words<kXlaneDpp, 1>())) * std::max<int64_t>(1, H / min_rows);
  if (tiles >= (int64_t(1) << 20)) return;
  scratch.get(Scratch::kQuietMapA, size_t(tiles) * 4);
  scratch.get(Scratch::kQuietMapB, size_t(tiles) * 4);
  scratch.get(Scratch::kQuietCounters, kQuietCountBytes);
  hipFuncAttributes attr;
  (void)hipFuncGetAttributes(&attr, reinterpret_cast<const void*>(&lb::life_quiet_kernel<kQuietT, QuietIO, kQuietM>));
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
  hipLaunchKernelGGL((lb::life_quiet_kernel<kQuietT, IO, M>), dim3(unsigned(tiles)), dim3(64 * M), 0, s, p);
  Q->prev = cur;
  Q->cur = next;
  Q->tiles = tiles;
  return tiles;
}

}  // namespace hipk
}  // namespace gol
