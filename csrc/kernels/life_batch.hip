// life_batch: many small universes per launch, each one in the registers of
// (a part of) one wave, with the cycle stop inside the kernel (gol/batch.hpp).
//
// The temporal-block kernels (life_block_impl.hpp) stream a huge grid through
// HBM.  A 64 x 64 torus is 128 words: it needs no streaming at all.
//   * Lane mapping: one row per lane, W/32 words per lane, so a wave holds
//     64/H universes (H = 64: one; H = 8: eight).  A partial last wave masks
//     its missing universes off: no load, no store, counted as stopped.
//   * A generation touches no memory.  Horizontal neighbours are funnel shifts
//     inside the lane (v_alignbit on the word or the word pair: a rotate on
//     the torus, zero fill on the bounded plane).  The horizontal sums
//     (h0, h1) go through the rule policies of life_block_impl.hpp unchanged;
//     what crosses lanes are h0 and h1 of the rows above and below - two
//     values per word and direction:
//       H = 64   the wave rotates, DPP wave_ror:1 / wave_rol:1
//       H = 16   the row rotates, DPP row_ror:1 / row_ror:15
//       H = 8, 32, and every height with tuning batch_vmove=bpermute:
//                ds_bpermute with lane indices computed once.
//     On the bounded plane the incoming values of a universe's first and last
//     row are zeroed.
//   * Stop test, every generation: per-lane XOR against the snapshot words,
//     one ballot, masked per universe.  A stopped universe keeps its words
//     through a per-lane select while the others of its wave go on; the wave
//     leaves the loop (uniformly) when all have stopped or at max_gens.  No
//     cross-wave waits, no atomics, no memory traffic in the loop.
//   * The state is read once (0/1 bytes packed in the lane, or generated in
//     the lane from the counter-based RNG, so a random soup never exists in
//     memory) and written at most once (only when the grids are asked for).
//   * The rule is a policy.  Compiled<R> folds one rule of life_rules.def in
//     at compile time.  RuleWord takes the rule as data: every lane loads its
//     universe's rule word once and expands it into 17 all-ones / all-zero
//     registers, the entries of the truth table over (centre, 3x3 sum); a
//     generation evaluates the table as a tree of v_bitop3 selects.  The
//     universes of one wave may all have different rules.
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "gol/backend.hpp"
#include "gol/batch.hpp"
#include "gol/hip_util.hpp"
#include "life_batch_common.hpp"
#include "life_block_impl.hpp"

namespace gol {
namespace hipk {
namespace batch {

struct Args {
  int64_t B;
  const uint8_t* cells;  // (B, H, W) 0/1 bytes, or nullptr: random
  uint64_t seed;
  uint32_t thresh;       // density_thresh()
  int max_gens, max_period;
  int32_t* generations;
  int32_t* period;
  int32_t* population;
  uint8_t* stop;
  uint32_t* words;       // (B, H, W/32) final words, or nullptr
  // Rule table (RuleWord only): universe u runs rule u / K on soup
  // share ? u % K : u; a word is birth | survive << 16.
  const uint32_t* rules;
  uint32_t K;
  uint32_t share;
};

// ---- rule policies ------------------------------------------------------------
// State: what a lane keeps of its universe's rule over the loop.  soup(): the
// index of the universe's cells and seed.  load() runs only for valid lanes.

// One rule of life_block_impl.hpp, folded in at compile time.
template <class R>
struct Compiled {
  struct State {};
  __device__ static __forceinline__ int64_t soup(const Args&, int64_t u) { return u; }
  __device__ static __forceinline__ void load(State&, const Args&, int64_t) {}
  __device__ static __forceinline__ uint32_t eval(const State&, uint32_t a0, uint32_t a1, uint32_t b0, uint32_t b1,
                                                  uint32_t c0, uint32_t c1, uint32_t ctr) {
    return R::eval(a0, a1, b0, b1, c0, c1, ctr);
  }
};

// The rule as data.  With S = 0..9 the 3x3 sum including the centre (bit
// planes s0..s3 as in common.hpp rule_host), next = ctr ? survive[S - 1] :
// birth[S].  A live centre has S >= 1, a dead one S <= 8 and B0 is refused, so
// the table's entry at S is E[S] = ctr ? sv[S - 1] : b[S] for S = 1..8,
// E[0] = 0 and E[9] = sv[8]: 8 selects on ctr, then a select tree over the
// bits of S (5 on s0, 2 on s1, 1 on s2, 1 on s3).  24 v_bitop3 / v_xor a word
// against Conway's 8.  The entries are per-lane values at every height.
struct RuleWord {
  struct State {
    uint32_t b[9] = {};   // b[n]: all ones where born at n neighbours (b[0] unused)
    uint32_t sv[9] = {};  // sv[n]: all ones where surviving at n neighbours
  };
  __device__ static __forceinline__ int64_t soup(const Args& a, int64_t u) {
    return a.share ? int64_t(uint32_t(u) % a.K) : u;
  }
  __device__ static __forceinline__ void load(State& st, const Args& a, int64_t u) {
    const uint32_t w = a.rules[uint32_t(u) / a.K];
#pragma unroll
    for (int n = 0; n < 9; ++n) {
      st.b[n] = 0u - ((w >> n) & 1u);
      st.sv[n] = 0u - ((w >> (16 + n)) & 1u);
    }
  }
  __device__ static __forceinline__ uint32_t eval(const State& st, uint32_t a0, uint32_t a1, uint32_t b0, uint32_t b1,
                                                  uint32_t c0, uint32_t c1, uint32_t ctr) {
    using lb::bop3;
    const uint32_t s0 = bop3<tt::XOR3>(a0, b0, c0);
    const uint32_t x1 = bop3<tt::MAJ>(a0, b0, c0);
    const uint32_t y0 = bop3<tt::XOR3>(a1, b1, c1);
    const uint32_t y1 = bop3<tt::MAJ>(a1, b1, c1);
    const uint32_t s1 = x1 ^ y0;
    const uint32_t s2 = bop3<tt::XOR_AND>(x1, y0, y1);
    const uint32_t s3 = bop3<tt::AND3>(x1, y0, y1);
    uint32_t e[10];
    e[0] = 0u;
#pragma unroll
    for (int n = 1; n <= 8; ++n) e[n] = bop3<tt::SEL>(ctr, st.sv[n - 1], st.b[n]);
    e[9] = st.sv[8];
    const uint32_t p01 = s0 & e[1];
    const uint32_t p23 = bop3<tt::SEL>(s0, e[3], e[2]);
    const uint32_t p45 = bop3<tt::SEL>(s0, e[5], e[4]);
    const uint32_t p67 = bop3<tt::SEL>(s0, e[7], e[6]);
    const uint32_t p89 = bop3<tt::SEL>(s0, e[9], e[8]);
    const uint32_t q03 = bop3<tt::SEL>(s1, p23, p01);
    const uint32_t q47 = bop3<tt::SEL>(s1, p67, p45);
    const uint32_t r07 = bop3<tt::SEL>(s2, q47, q03);
    return bop3<tt::SEL>(s3, p89, r07);
  }
};

template <int NW, int H, class Rule, bool DEAD, int VM>
__global__ __launch_bounds__(kBlock) void life_batch_kernel(const Args a) {
  using lb::bop3;
  constexpr int UPW = 64 / H;  // universes per wave
  const int lane = int(threadIdx.x) & 63;
  const int64_t wave = int64_t(blockIdx.x) * (kBlock / 64) + (int(threadIdx.x) >> 6);
  const int row = lane & (H - 1);
  const int base = lane & ~(H - 1);
  const int64_t u = wave * UPW + lane / H;
  const bool valid = u < a.B;

  // ---- the lane's row: packed from bytes, or drawn from the RNG -------------
  uint32_t c[NW];
#pragma unroll
  for (int i = 0; i < NW; ++i) c[i] = 0u;
  typename Rule::State rule;
  if (valid) {
    Rule::load(rule, a, u);
    const int64_t soup = Rule::soup(a, u);
    if (a.cells) {
      const uint32_t* src = reinterpret_cast<const uint32_t*>(a.cells + (soup * H + row) * int64_t(32 * NW));
      GOL_BATCH_PACK_ROW(NW, src, c)
    } else {
      const uint64_t seed = a.seed + uint64_t(soup);
#pragma unroll
      for (int i = 0; i < NW; ++i) {
        uint32_t w = 0;
        for (int j = 0; j < 32; ++j) w |= uint32_t(rng_cell(seed, row, 32 * i + j, a.thresh)) << j;
        c[i] = w;
      }
    }
  }

  // Lanes of the rows above and below (ds_bpermute addresses), the lanes of
  // this lane's universe as a ballot mask, the plane's dead rows.
  const int up4 = 4 * (base | ((row - 1) & (H - 1))), dn4 = 4 * (base | ((row + 1) & (H - 1)));
  const uint64_t mine = H == 64 ? ~uint64_t(0) : ((uint64_t(1) << (H & 63)) - 1) << base;
  const uint32_t up_keep = (DEAD && row == 0) ? 0u : ~0u, dn_keep = (DEAD && row == H - 1) ? 0u : ~0u;

  uint32_t snap[NW];
#pragma unroll
  for (int i = 0; i < NW; ++i) snap[i] = c[i];
  bool active = valid;
  int gens = a.max_gens, per = 0;
  int t = 0, k = 0;  // generation, generations since the snapshot (both wave-uniform)
  while (t < a.max_gens && __builtin_amdgcn_ballot_w64(active) != 0) {
    uint32_t h0[NW], h1[NW], nxt[NW];
#pragma unroll
    for (int i = 0; i < NW; ++i) {
      // Words left and right of word i in the row: the torus wraps, the plane ends in dead cells.
      const uint32_t lw = i > 0 ? c[i - 1] : DEAD ? 0u : c[NW - 1];
      const uint32_t rw = i + 1 < NW ? c[i + 1] : DEAD ? 0u : c[0];
      const uint32_t l = __builtin_amdgcn_alignbit(c[i], lw, 31);  // cell x-1 at bit x
      const uint32_t r = __builtin_amdgcn_alignbit(rw, c[i], 1);   // cell x+1 at bit x
      h0[i] = bop3<tt::XOR3>(l, c[i], r);
      h1[i] = bop3<tt::MAJ>(l, c[i], r);
    }
    uint32_t diff = 0;
#pragma unroll
    for (int i = 0; i < NW; ++i) {
      uint32_t a0 = vmove<H, VM, true>(h0[i], up4), a1 = vmove<H, VM, true>(h1[i], up4);
      uint32_t d0 = vmove<H, VM, false>(h0[i], dn4), d1 = vmove<H, VM, false>(h1[i], dn4);
      if constexpr (DEAD) {
        a0 &= up_keep, a1 &= up_keep;
        d0 &= dn_keep, d1 &= dn_keep;
      }
      nxt[i] = Rule::eval(rule, a0, a1, h0[i], h1[i], d0, d1, c[i]);
      diff |= nxt[i] ^ snap[i];
    }
    ++t, ++k;
    const uint64_t differs = __builtin_amdgcn_ballot_w64(diff != 0);
    const bool same = (differs & mine) == 0;
    // A stopped universe keeps its words; one that stops now takes this generation.
#pragma unroll
    for (int i = 0; i < NW; ++i) c[i] = active ? nxt[i] : c[i];
    const bool stops = active && same;
    gens = stops ? t : gens;
    per = stops ? k : per;
    active = active && !same;
    if (k == a.max_period) {  // after the compare: the snapshot of generation t
      k = 0;
#pragma unroll
      for (int i = 0; i < NW; ++i) snap[i] = c[i];
    }
  }

  // ---- epilogue: population per universe, one lane writes the results --------
  int pop = 0;
#pragma unroll
  for (int i = 0; i < NW; ++i) pop += __builtin_popcount(c[i]);
#pragma unroll
  for (int off = 1; off < H; off <<= 1) pop += __shfl_xor(pop, off, 64);
  if (valid) {
    if (row == 0) {
      a.generations[u] = gens;
      a.period[u] = per;
      a.population[u] = pop;
      a.stop[u] = per == 0 ? uint8_t(kBatchLimit) : pop == 0 ? uint8_t(kBatchExtinction) : uint8_t(kBatchCycle);
    }
    if (a.words) {
#pragma unroll
      for (int i = 0; i < NW; ++i) a.words[(u * H + row) * NW + i] = c[i];
    }
  }
}

using LaunchFn = void (*)(const Args&, int64_t waves, hipStream_t);

template <int NW, int H, class Rule, bool DEAD, int VM>
void launch(const Args& a, int64_t waves, hipStream_t s) {
  const int64_t blocks = ceil_div(waves, kBlock / 64);
  hipLaunchKernelGGL((life_batch_kernel<NW, H, Rule, DEAD, VM>), dim3(uint32_t(blocks)), dim3(kBlock), 0, s, a);
}

// [word count][height][boundary][vertical move] of one rule.
struct RuleTable {
  Rule rule;
  LaunchFn fn[2][4][2][2];
};

template <class R, int NW, int H>
void fill_shape(LaunchFn (&f)[2][2]) {
  constexpr int kDpp = has_dpp(H) ? kVmDpp : kVmBpermute;
  f[0][kVmDpp] = launch<NW, H, R, false, kDpp>;
  f[1][kVmDpp] = launch<NW, H, R, true, kDpp>;
  f[0][kVmBpermute] = launch<NW, H, R, false, kVmBpermute>;
  f[1][kVmBpermute] = launch<NW, H, R, true, kVmBpermute>;
}
template <class R, int NW>
void fill_words(LaunchFn (&f)[4][2][2]) {
  fill_shape<R, NW, 8>(f[0]);
  fill_shape<R, NW, 16>(f[1]);
  fill_shape<R, NW, 32>(f[2]);
  fill_shape<R, NW, 64>(f[3]);
}
template <class R>
RuleTable make_table(Rule rule) {
  RuleTable t;
  t.rule = rule;
  fill_words<R, 1>(t.fn[0]);
  fill_words<R, 2>(t.fn[1]);
  return t;
}

const std::vector<RuleTable>& tables() {
  static const std::vector<RuleTable> t = {
      make_table<Compiled<lb::Conway>>(Rule{}),
#define GOL_RULE(name, B, S) make_table<Compiled<lb::LifeLike<B, S>>>(Rule{B, S}),
#include "life_rules.def"
#undef GOL_RULE
  };
  return t;
}

// The kernels that take their rules from Args::rules.
const RuleTable& word_table() {
  static const RuleTable t = make_table<RuleWord>(Rule{0, 0});
  return t;
}

}  // namespace batch
}  // namespace hipk

BatchResult run_batch_hip(int device, const BatchConfig& cfg, const BatchInput& in, const Tuning& tune) {
  namespace hb = hipk::batch;
  validate_batch(cfg, in);
  const bool by_word = !cfg.rules.empty();
  const hb::RuleTable* table = by_word ? &hb::word_table() : nullptr;
  for (const hb::RuleTable& t : hb::tables())
    if (!by_word && t.rule == cfg.rule) table = &t;
  if (!table) {
    std::string have;
    for (const Rule r : hip_rules()) have += std::string(have.empty() ? "" : ", ") + rule_string(r);
    fail("rule " + rule_string(cfg.rule) + " is not compiled for the HIP engine (compiled: B3/S23, " + have +
         "; add a line to csrc/kernels/life_rules.def, or run it on the CPU engine)");
  }
  const int vm = hb::parse_vmove(tune, cfg.H);
  GOL_REQUIRE(hip_available(), "no HIP device available (HIP engine requested)");

  const int W = cfg.W, H = cfg.H, NW = W / 32, upw = 64 / H;
  const int64_t B = in.B, waves = ceil_div(B, upw);
  const int hi = H == 8 ? 0 : H == 16 ? 1 : H == 32 ? 2 : 3;
  const bool dead = cfg.boundary == Boundary::Dead;
  const hb::LaunchFn fn = table->fn[NW - 1][hi][dead ? 1 : 0][vm];

  DeviceScope scope(device);
  const size_t n_cells = in.cells ? size_t(batch_soups(cfg, in)) * H * W : 0;
  hb::DeviceBuf<uint8_t> d_cells(n_cells);
  hb::DeviceBuf<uint32_t> d_rules(cfg.rules.size());
  const size_t nb = size_t(B);
  hb::DeviceBuf<int32_t> d_gens(nb), d_per(nb), d_pop(nb);
  hb::DeviceBuf<uint8_t> d_stop(nb);
  // The cluster census reads the final words on the device.
  hb::DeviceBuf<uint32_t> d_words(cfg.want_grids || cfg.clusters ? size_t(B) * H * NW : 0);
  if (in.cells) HIP_CHECK(hipMemcpy(d_cells.p, in.cells, n_cells, hipMemcpyHostToDevice));
  if (by_word) {
    std::vector<uint32_t> words(cfg.rules.size());
    for (size_t r = 0; r < words.size(); ++r) words[r] = uint32_t(cfg.rules[r].birth) | uint32_t(cfg.rules[r].survive) << 16;
    HIP_CHECK(hipMemcpy(d_rules.p, words.data(), words.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
  }

  hb::Args a{};
  a.B = B;
  a.cells = d_cells.p;
  a.seed = in.seed;
  a.thresh = density_thresh(in.density);
  a.max_gens = int(cfg.max_gens);
  a.max_period = int(cfg.max_period);
  a.generations = d_gens.p;
  a.period = d_per.p;
  a.population = d_pop.p;
  a.stop = d_stop.p;
  a.words = d_words.p;
  a.rules = d_rules.p;
  a.K = uint32_t(by_word ? cfg.soups_per_rule : 1);
  a.share = cfg.share_soups ? 1u : 0u;

  BatchResult res;
  res.kernel_ms = hb::timed_launch([&] { fn(a, waves, nullptr); });

  res.generations.resize(size_t(B));
  res.period.resize(size_t(B));
  res.population.resize(size_t(B));
  res.stop.resize(size_t(B));
  HIP_CHECK(hipMemcpy(res.generations.data(), d_gens.p, size_t(B) * sizeof(int32_t), hipMemcpyDeviceToHost));
  HIP_CHECK(hipMemcpy(res.period.data(), d_per.p, size_t(B) * sizeof(int32_t), hipMemcpyDeviceToHost));
  HIP_CHECK(hipMemcpy(res.population.data(), d_pop.p, size_t(B) * sizeof(int32_t), hipMemcpyDeviceToHost));
  HIP_CHECK(hipMemcpy(res.stop.data(), d_stop.p, size_t(B), hipMemcpyDeviceToHost));
  if (cfg.want_grids) {
    std::vector<uint32_t> words(size_t(B) * H * NW);
    HIP_CHECK(hipMemcpy(words.data(), d_words.p, words.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    res.grids.resize(size_t(B) * H * W);
    for (size_t w = 0; w < words.size(); ++w)
      for (int j = 0; j < 32; ++j) res.grids[32 * w + size_t(j)] = uint8_t((words[w] >> j) & 1u);
  }
  const char* move = vm == hb::kVmBpermute ? "ds_bpermute" : H == 64 ? "dpp wave_ror/rol" : "dpp row_ror";
  res.variant = "batch " + std::to_string(W) + "x" + std::to_string(H) + " " + boundary_name(cfg.boundary) + " " +
                std::to_string(upw) + "/wave " + move + " " + batch_rule_text(cfg);
  if (cfg.clusters) res.census = hb::find_clusters_device(W, H, dead, vm, B, nullptr, d_words.p);
  return res;
}

}  // namespace gol
