// life_block dispatcher: validates the launch and picks the compiled kernel
// variant (layout x words-per-lane x cross-lane primitive).  The kernel
// itself is in life_block_impl.hpp / life_group_impl.hpp (schedules in
// life_block_launch.hpp).
#include "life_kernels.hpp"

#include <string>

#include "gol/common.hpp"

namespace gol {
namespace hipk {

namespace {

const char* xlane_name(int x) { return x == kXlaneAuto ? "auto(add|dpp)" : x == kXlaneAdd ? "add" : "dpp"; }

}  // namespace

// The rule kernels (life_rule_<name>_<variant>.hip), one table generated from
// life_rules.def.
#define GOL_RULE(name, B, S)                          \
  GOL_LIFE_VARIANT(launch_rule_##name##_bits_dpp);    \
  GOL_LIFE_VARIANT(launch_rule_##name##_bits_add);    \
  GOL_LIFE_VARIANT(launch_rule_##name##_u8_dpp);
#include "life_rules.def"
#undef GOL_RULE

namespace {

using VariantFn = LaunchResult (*)(const LifeBlockParams&, int64_t, int, const LifeTuning&, const LaunchCtx&, hipStream_t);
struct RuleKernels {
  const char* name;
  Rule rule;
  VariantFn bits_dpp, bits_add, u8_dpp;
};
const RuleKernels kRuleKernels[] = {
#define GOL_RULE(name, B, S) \
  {#name, Rule{B, S}, launch_rule_##name##_bits_dpp, launch_rule_##name##_bits_add, launch_rule_##name##_u8_dpp},
#include "life_rules.def"
#undef GOL_RULE
};

const RuleKernels* rule_kernels(Rule r) {
  for (const RuleKernels& k : kRuleKernels)
    if (k.rule == r) return &k;
  return nullptr;
}

// The feature kernels (BlockArgs::features), a family per mode: B3/S23 on the
// DPP window, T <= 16, never linked, chained or skipping.
struct ModeRow {
  const char* word;  // in the variant string, and "<word> kernels"
  const char* what;  // the launch in the launcher's messages
  const char* note;  // where a forced adder window has no kernels
  VariantFn bits, u8;
};
const ModeRow kModes[] = {
    {},  // BlockMode::Plain: launch_life_block picks among the variants itself
    {"plane", "boundary=dead", "on the plane", launch_plane_bits_dpp, launch_plane_u8_dpp},
    {"census", "census", "with the census", launch_census_bits_dpp, launch_census_u8_dpp},
    {"fingerprint", "fingerprint", "with the fingerprint", launch_fprint_bits_dpp, launch_fprint_u8_dpp},
};

// A launch fuses one of them at most.
BlockMode block_mode(const BlockArgs& a) {
  const BlockFeatures f = a.features();
  GOL_REQUIRE(!(f.census && f.fingerprint), "life_block: census and fingerprint in one launch");
  GOL_REQUIRE(!(f.plane && f.series()), "life_block: boundary=dead with a census or a fingerprint in one launch");
  return f.plane ? BlockMode::Plane : f.census ? BlockMode::Census : f.fingerprint ? BlockMode::Fingerprint : BlockMode::Plain;
}

}  // namespace

std::vector<Rule> life_block_rules() {
  std::vector<Rule> v;
  for (const RuleKernels& k : kRuleKernels) v.push_back(k.rule);
  return v;
}

bool life_block_has_rule(Rule r) { return rule_is_default(r) || rule_kernels(r) != nullptr; }

std::string life_block_variant(Layout layout, const LifeTuning& tune, BlockMode mode) {
  const bool grouped = tune.group != 0;
  const std::string lay = layout == Layout::Bits ? "bits" : "u8";
  const std::string group =
      grouped ? (tune.group < 0 ? std::string(" group=auto") : " group=" + std::to_string(tune.group)) : "";
  if (mode != BlockMode::Plain) {
    const ModeRow& m = kModes[int(mode)];
    return lay + " wpl=1 dpp " + m.word +
           (tune.xlane == kXlaneAdd ? std::string(" (xlane=add runs dpp: no adder window ") + m.note + ")" : "") + group +
           (mode != BlockMode::Plane ? std::string(tune.wrap ? " wrap" : "") + " (no fold, link, chain or skipping)" : "");
  }
  if (layout == Layout::U8 && tune.u8_lds)
    return tune.lds_T > 1 ? "u8 lds-tiled T=" + std::to_string(tune.lds_T) + (tune.lds_pack && tune.lds_T >= 8 ? " packed" : "")
                          : std::string("u8 lds-tiled single-step");
  return lay + " wpl=1 " + xlane_name(tune.xlane) + group +
         (grouped && tune.chain == 1 ? " chain" : grouped && tune.chain < 0 ? " chain=tuned" : "");
}

int life_block_max_T(Layout layout, const LifeTuning& tune) {
  if (layout == Layout::U8 && tune.u8_lds) return tune.lds_T;
  // Register budget for 2 waves/SIMD (<= 256 VGPRs): T <= 16 (one word per lane).
  return 16;
}

LaunchResult launch_life_block(const BlockArgs& a, const LifeTuning& tune, const LaunchCtx& ctx, hipStream_t stream) {
  const TileGeom& g = a.g;
  GOL_REQUIRE(a.row_lo - a.T >= 0 && a.row_hi + a.T <= g.R() && a.row_lo < a.row_hi,
              "life_block: row range outside the tile");
  GOL_REQUIRE(g.Wp() < (int64_t(1) << 30), "life_block: row too wide");
  // Row stores go through a buffer descriptor per row (num_records = pitch)
  // and drop non-owned lanes at offset 2^30 (life_block_impl.hpp Writer).
  GOL_REQUIRE(g.pitch < (int64_t(1) << 30), "life_block: row pitch must be < 1 GiB");
  GOL_REQUIRE(g.Wp() >= 1, "life_block: tile narrower than one lane's word");
  GOL_REQUIRE(g.pitch >= (g.layout == Layout::Bits ? 4 : 32) * g.Wp(), "life_block: pitch too small");
  LifeBlockParams p{};
  p.in = static_cast<const uint8_t*>(a.in);
  p.out = static_cast<uint8_t*>(a.out);
  p.pitch = g.pitch;
  p.row_lo = a.row_lo;
  p.row_hi = a.row_hi;
  p.Wp = int(g.Wp());
  p.own_w0 = int(g.cell0() / 32);
  p.own_w1 = int(ceil_div(g.cell0() + g.W, 32));
  const int64_t tail = (g.cell0() + g.W) % 32;
  p.last_mask = tail ? (0xFFFFFFFFu >> (32 - tail)) : 0xFFFFFFFFu;
  if (a.gen_dev) {
    p.changed = a.changed;  // resolved on the device: changed + *gen_dev + gen_rel
    p.gen_dev = a.changed ? a.gen_dev : nullptr;
    p.gen_rel = a.gen_rel;
  } else {
    p.changed = a.changed ? a.changed + (a.gen_base + 1 - a.flags_base) : nullptr;
  }
  p.wg_trace = ctx.wg_trace;
  p.err = ctx.mail->err;
  p.chain_spin_log2 = tune.chain_spin_log2;
  p.wrap_w = a.full_width && tune.wrap && g.W % 32 == 0 ? int(g.W / 32) : 0;
  p.fold = 1;
  p.fold_lanes = 64;
  p.link_ring_rows = a.ring && a.row_lo == g.Dv && a.row_hi == g.Dv + g.H ? g.H : 0;
  p.fault_delay = tune.fault_delay;
  const int64_t rows = a.row_hi - a.row_lo;
  const BlockMode mode = block_mode(a);
  if (mode != BlockMode::Plain) {
    // The plane, census and fingerprint kernels (lb::PlaneIO, CensusIO,
    // FingerprintIO): B3/S23 on the DPP window (a forced adder window runs the
    // DPP window too: its drifting frame is a relabelling of torus columns).
    // The engine refuses the combinations that have no such kernel before any
    // launch; these guard the launcher itself.
    const ModeRow& m = kModes[int(mode)];
    const bool series = mode != BlockMode::Plane;
    const auto msg = [&m](const char* tail) { return std::string("life_block: ") + m.what + tail; };
    GOL_REQUIRE(rule_is_default(a.rule), msg(" runs B3/S23 only on the HIP engine"));
    GOL_REQUIRE(!(g.layout == Layout::U8 && tune.u8_lds), msg(" with u8_kernel=lds"));
    // A series keeps wrapped column reads and the row ring: the owned words and
    // rows are counted once either way.
    GOL_REQUIRE(!a.allow_drift && !a.wrap_rows && !a.link && !a.quiet && (series ? !a.gen_dev : !a.full_width && !a.ring),
                msg(series ? " with a launch option it does not run with" : " with a torus-only launch option"));
    GOL_REQUIRE(a.T <= 16, std::string("life_block: ") + m.word + " kernels run temporal blocks of at most 16 generations");
    p.link_ring_rows = 0;
    if (!series) {
      GOL_REQUIRE(g.R() < (int64_t(1) << 30), "life_block: boundary=dead needs fewer than 2^30 tile rows");
      GOL_REQUIRE(a.grid_row_lo >= 0 && a.grid_row_lo < a.grid_row_hi && a.grid_row_hi <= g.R() &&
                      a.grid_cell_lo >= 0 && a.grid_cell_lo % 32 == 0 && a.grid_cell_lo < a.grid_cell_hi &&
                      a.grid_cell_hi <= 32 * g.Wp(),
                  "life_block: grid bounds outside the tile");
      p.wrap_w = 0;
      p.grid_row_lo = int(a.grid_row_lo);
      p.grid_row_hi = int(a.grid_row_hi);
      p.grid_w0 = int(a.grid_cell_lo / 32);
      p.grid_w1 = int(ceil_div(a.grid_cell_hi, 32));
      const int64_t gtail = a.grid_cell_hi % 32;
      p.grid_last_mask = gtail ? (0xFFFFFFFFu >> (32 - gtail)) : 0xFFFFFFFFu;
    } else {
      GOL_REQUIRE(a.gen_base >= a.flags_base, msg(" block before its window"));
      p.grid_row_lo = int(g.Dv);
      p.grid_row_hi = int(g.Dv + g.H);
      const int64_t slot = a.gen_base + 1 - a.flags_base;
      if (mode == BlockMode::Census) {
        // A wave's count of one generation stays below 2^31 (64 lanes x 32 cells x rows).
        GOL_REQUIRE(rows + 2 * a.T < (int64_t(1) << 20), "life_block: census needs blocks of fewer than 2^20 rows");
        p.census = reinterpret_cast<unsigned long long*>(a.census) + slot;
      } else {
        // Rows and words travel in 32 bits; the tile's first owned column is a
        // word boundary of the global grid (the engine refuses a byte
        // decomposition where it is not).
        GOL_REQUIRE(a.global_col0 % 32 == 0, "life_block: fingerprint tile off the global word grid");
        GOL_REQUIRE(a.global_row0 >= 0 && a.global_row0 + g.R() < (int64_t(1) << 31) &&
                        a.global_col0 / 32 + g.Wp() < (int64_t(1) << 31),
                    "life_block: fingerprint needs global rows and words below 2^31");
        p.fingerprint = reinterpret_cast<unsigned long long*>(a.fingerprint) + slot;
        p.fp_row0 = int(a.global_row0 - g.Dv);
        p.fp_word0 = int(a.global_col0 / 32);
      }
    }
    return (g.layout == Layout::U8 ? m.u8 : m.bits)(p, rows, a.T, tune, ctx, stream);
  }
  int x = tune.xlane == kXlaneAdd || tune.xlane == kXlaneAuto ? tune.xlane : kXlaneDpp;
  // Any rule but B3/S23: the kernels compiled from life_rules.def.
  const RuleKernels* rk = nullptr;
  if (!rule_is_default(a.rule)) {
    rk = rule_kernels(a.rule);
    if (!rk) {
      std::string have;
      for (const RuleKernels& k : kRuleKernels) have += std::string(have.empty() ? "" : ", ") + rule_string(k.rule);
      fail("rule " + rule_string(a.rule) + " is not compiled for the HIP engine (compiled: B3/S23, " + have +
           "; add a line to csrc/kernels/life_rules.def, or run it on the CPU engine)");
    }
    GOL_REQUIRE(!(g.layout == Layout::U8 && tune.u8_lds),
                "life_block: the LDS-tiled byte kernels run B3/S23 only (u8_kernel=lds with a rule)");
    GOL_REQUIRE(a.T <= 16, "life_block: rule kernels run temporal blocks of at most 16 generations");
  }
  if (g.layout == Layout::U8 && tune.u8_lds && (a.T == 1 || a.T == 2 || a.T == 4 || a.T == 8 || a.T == 16 || a.T == 32)) {
    // Packed tiles need 32-cell aligned rows (pitch) and owned cells.
    const bool pack = a.T >= 8 && (tune.lds_pack || a.T > 8) && g.pitch % 32 == 0 && g.cell0() % 32 == 0;
    GOL_REQUIRE(a.T <= 8 || pack, "life_block: LDS-tiled byte passes deeper than 8 need the packed tile");
    LaunchResult res;
    res.path = kPathLdsTiled;
    if (pack)
      res.drift = launch_life_lds_bits(a, tune.wrap, tune.lds_xcd, tune.lds_waves, tune.cus, stream);
    else if (a.T == 1)
      launch_life_step_lds(a, tune.lds_rows, tune.wrap, stream);
    else
      launch_life_lds_multi(a, tune.wrap, stream);
    return res;
  }
  // The adder window drifts the storage frame by T cells (see kXlaneAdd); the
  // engine allows that only for whole-width tiles of 32-cell words, and the
  // left halo must hold the 2T cells its one-sided light cone consumes (wrap
  // mode reads the wrapped owned words instead).
  // Quiet-tile skipping (BlockArgs::quiet): the detecting / skipping kernel
  // where the block can be planned for it; else the kernels below (any path
  // but kPathSkipping leaves the next skipping launch no words to read).
  if (ctx.quiet && a.quiet && !rk && g.layout == Layout::Bits) {
    LaunchResult res;
    res.path = kPathSkipping;
    res.quiet_tiles = launch_bits_w1_dpp_quiet(p, rows, a.T, ctx, stream);
    if (res.quiet_tiles > 0) return res;
  }
  if (x == kXlaneAuto) x = kXlaneAdd;  // the engine decided through allow_drift
  // The one-sided window also consumes 2T cells of its wave's single halo
  // word per pass, so passes deeper than 16 (the byte layout's T = 24 / 32)
  // run the DPP window.
  if (x == kXlaneAdd && !(a.allow_drift && a.T <= 16 && (p.wrap_w > 0 || 32 * g.hw >= 2 * a.T))) x = kXlaneDpp;
  const bool u8 = g.layout == Layout::U8;
  // No byte-layout adder variant of a rule: that request runs the DPP window.
  if (rk && u8) x = kXlaneDpp;
  const VariantFn fn = rk ? (x == kXlaneAdd ? rk->bits_add : u8 ? rk->u8_dpp : rk->bits_dpp)
                          : x == kXlaneAdd ? (u8 ? launch_u8_w1_add : launch_bits_w1_add)
                                           : (u8 ? launch_u8_w1_dpp : launch_bits_w1_dpp);
  LaunchResult res = fn(p, rows, a.T, tune, ctx, stream);
  res.drift = x == kXlaneAdd ? a.T : 0;
  return res;
}

}  // namespace hipk
}  // namespace gol
