// gol-mi355x: common types, error handling and the bit-sliced B3/S23 rule.
//
// The reference keeps one ASCII byte per cell and evaluates B3/S23 with
// nested branchy loops (serial: src/game.c:60-101; MPI ASCII-sum form:
// src/game_mpi.c:61-87; CUDA 1 thread/cell: src/game_cuda.cu:128-148).
// This framework evaluates the rule on 32 cells at once with bit-sliced
// adders, written so that every step maps onto one CDNA4 VALU instruction
// (v_bitop3_b32 / v_alignbit_b32 / DPP moves).  The host versions below are
// bit-exact emulations used by the CPU backend and the test oracles.
#pragma once

#include <cstddef>
#include <cstdint>
#include <stdexcept>
#include <string>

// Functions shared by host code and HIP kernels (e.g. the RNG) carry GOL_HD.
#if defined(__HIP__)
#define GOL_HD __host__ __device__
#else
#define GOL_HD
#endif

namespace gol {

enum class Layout : int { U8 = 0, Bits = 1 };

inline const char* layout_name(Layout l) { return l == Layout::Bits ? "bits" : "u8"; }

// What lies beyond the grid's edge.  Torus: the grid wraps (the reference's
// only world, and the default).  Dead: the bounded plane - cells outside
// [0, W) x [0, H) are dead in every generation.
enum class Boundary : int { Torus = 0, Dead = 1 };

inline const char* boundary_name(Boundary b) { return b == Boundary::Dead ? "dead" : "torus"; }

// Fail-stop error (the reference calls perror_exit / cudaSafeCall and exits:
// src/game.c:19-23, src/game_cuda.cu:18-27).  We throw so that Python callers
// get a RuntimeError; the CLI catches, prints and exits non-zero.
struct Error : std::runtime_error {
  using std::runtime_error::runtime_error;
};

[[noreturn]] void fail(const std::string& msg);

inline Boundary parse_boundary(const std::string& s) {
  if (s == "torus") return Boundary::Torus;
  if (s == "dead") return Boundary::Dead;
  fail("bad boundary '" + s + "' (want torus or dead)");
}

#define GOL_REQUIRE(cond, msg)                                                  \
  do {                                                                          \
    if (!(cond)) ::gol::fail(std::string(__FILE__) + ":" +                      \
                             std::to_string(__LINE__) + ": " + (msg));         \
  } while (0)

constexpr int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }
constexpr int64_t round_up(int64_t a, int64_t b) { return ceil_div(a, b) * b; }

// ---------------------------------------------------------------------------
// v_bitop3_b32 truth tables.  Operand k of bitop3(a, b, c) contributes the
// 8-bit pattern {0xF0, 0xCC, 0xAA}[k]; the immediate is the function applied
// to those patterns (same convention as LLVM's BitOp3 lowering).
// ---------------------------------------------------------------------------
namespace tt {
constexpr uint8_t A = 0xF0, B = 0xCC, C = 0xAA;
constexpr uint8_t XOR3 = A ^ B ^ C;                      // parity
constexpr uint8_t MAJ = (A & B) | (A & C) | (B & C);     // carry
constexpr uint8_t ANDN_XOR = uint8_t(~A & (B ^ C));      // ~a & (b ^ c)
constexpr uint8_t EQ_NE = uint8_t(~(A ^ B) & (A ^ C));   // (a == b) & (a != c)
constexpr uint8_t SEL = uint8_t((A & B) | (~A & C));     // a ? b : c
constexpr uint8_t OR_XOR = uint8_t(A | (B ^ C));         // a | (b ^ c)
constexpr uint8_t AND3 = A & B & C;
}  // namespace tt

// Host emulation of v_bitop3_b32 (bit-exact): each result bit is
// TT[(a<<2)|(b<<1)|c].
template <unsigned TT>
inline uint32_t bop3_host(uint32_t a, uint32_t b, uint32_t c) {
  uint32_t r = 0;
  if (TT & 0x01) r |= ~a & ~b & ~c;
  if (TT & 0x02) r |= ~a & ~b & c;
  if (TT & 0x04) r |= ~a & b & ~c;
  if (TT & 0x08) r |= ~a & b & c;
  if (TT & 0x10) r |= a & ~b & ~c;
  if (TT & 0x20) r |= a & ~b & c;
  if (TT & 0x40) r |= a & b & ~c;
  if (TT & 0x80) r |= a & b & c;
  return r;
}

// Funnel shift: low 32 bits of ((hi:lo) >> s), s in [0,31]  (v_alignbit_b32).
inline uint32_t alignbit_host(uint32_t hi, uint32_t lo, unsigned s) {
  return uint32_t(((uint64_t(hi) << 32) | lo) >> s);
}

// Bit order: bit j of word w holds cell x = 32*w + j (LSB = leftmost cell).
// Horizontal 3-sum of a row: (h1,h0) = L + C + R as a 2-bit number.
struct HSum {
  uint32_t h0, h1;
};

inline HSum hsum_host(uint32_t left_word, uint32_t c, uint32_t right_word) {
  uint32_t l = alignbit_host(c, left_word, 31);   // cell x-1 at bit of x
  uint32_t r = alignbit_host(right_word, c, 1);   // cell x+1 at bit of x
  return {bop3_host<tt::XOR3>(l, c, r), bop3_host<tt::MAJ>(l, c, r)};
}

// B3/S23 from three horizontal sums (rows above, centre, below) and the centre
// cells.  S = 3x3 sum including the centre = x0 + 2*(x1 + y0) + 4*y1;
// next = (S == 3) | (C & S == 4).
inline uint32_t rule_host(HSum a, HSum b, HSum c, uint32_t ctr) {
  uint32_t x0 = bop3_host<tt::XOR3>(a.h0, b.h0, c.h0);
  uint32_t x1 = bop3_host<tt::MAJ>(a.h0, b.h0, c.h0);
  uint32_t y0 = bop3_host<tt::XOR3>(a.h1, b.h1, c.h1);
  uint32_t y1 = bop3_host<tt::MAJ>(a.h1, b.h1, c.h1);
  uint32_t s3 = bop3_host<tt::ANDN_XOR>(y1, x1, y0);  // x0=1: S==3
  uint32_t s4 = bop3_host<tt::EQ_NE>(x1, y0, y1);     // x0=0: S==4
  return bop3_host<tt::SEL>(x0, s3, ctr & s4);
}

// ---------------------------------------------------------------------------
// Life-like (outer-totalistic) rules in B/S notation.  Bit n of `birth` /
// `survive`: a dead cell is born / a live cell survives at n live neighbours,
// n = 0..8.  B3/S23 is the default and keeps its own 7-op form above.
// ---------------------------------------------------------------------------
struct Rule {
  uint16_t birth = 1u << 3;
  uint16_t survive = (1u << 2) | (1u << 3);
};
constexpr bool operator==(Rule a, Rule b) { return a.birth == b.birth && a.survive == b.survive; }
constexpr bool operator!=(Rule a, Rule b) { return !(a == b); }
constexpr bool rule_is_default(Rule r) { return r == Rule{}; }

// The named rules parse_rule() accepts (gol_amd.RULES).
struct RuleName {
  const char* name;
  Rule rule;
};
constexpr RuleName kRuleNames[] = {
    {"life", {0x008, 0x00C}},      {"conway", {0x008, 0x00C}},    {"highlife", {0x048, 0x00C}},
    {"daynight", {0x1C8, 0x1D8}},  {"seeds", {0x004, 0x000}},     {"replicator", {0x0AA, 0x0AA}},
    {"lwod", {0x008, 0x1FF}},      {"34life", {0x018, 0x018}},
};

// Canonical text: B<digits>/S<digits>, digits ascending.
inline std::string rule_string(Rule r) {
  std::string s = "B";
  for (int n = 0; n <= 8; ++n)
    if ((r.birth >> n) & 1u) s += char('0' + n);
  s += "/S";
  for (int n = 0; n <= 8; ++n)
    if ((r.survive >> n) & 1u) s += char('0' + n);
  return s;
}

// B0 would make the empty grid come alive: the engine's lazy termination
// (engine.hpp) relies on "empty stays empty" being absorbing.
inline void require_no_b0(Rule r, const std::string& text) {
  if (r.birth & 1u)
    fail("rule '" + text + "': B0 is not supported (an empty grid would not stay empty, and the lazy extinction "
         "test relies on that)");
}

// "B36/S23", "b36s23", or a name of kRuleNames (case-insensitive).  Throws
// on malformed text, digit 9, repeated digits and B0.
inline Rule parse_rule(const std::string& text) {
  std::string t;
  for (const char c : text)
    if (c != ' ') t += char(c >= 'A' && c <= 'Z' ? c - 'A' + 'a' : c);
  for (const RuleName& n : kRuleNames)
    if (t == n.name) return n.rule;
  const auto bad = [&](const std::string& why) -> Rule {
    std::string names;
    for (const RuleName& n : kRuleNames) names += std::string(names.empty() ? "" : ", ") + n.name;
    fail("rule '" + text + "': " + why + " (expected B<digits>/S<digits> with digits 0-8, e.g. B36/S23, or one of: " +
         names + ")");
  };
  Rule r{0, 0};
  size_t i = 0;
  if (i >= t.size() || t[i] != 'b') return bad("does not start with B");
  ++i;
  const auto digits = [&](uint16_t& mask) -> bool {
    for (; i < t.size() && t[i] >= '0' && t[i] <= '9'; ++i) {
      if (t[i] == '9') return bad("a cell has at most 8 neighbours"), false;
      const uint16_t bit = uint16_t(1u << (t[i] - '0'));
      if (mask & bit) return bad(std::string("digit ") + t[i] + " is repeated"), false;
      mask = uint16_t(mask | bit);
    }
    return true;
  };
  digits(r.birth);
  if (i < t.size() && t[i] == '/') ++i;
  if (i >= t.size() || t[i] != 's') return bad("no S part");
  ++i;
  digits(r.survive);
  if (i != t.size()) return bad("unexpected '" + t.substr(i) + "'");
  require_no_b0(r, text);
  return r;
}

// The general bit-sliced rule.  From the partial sums of rule_host(), the
// four bits of S (0..9) are
//   s0 = x0, s1 = x1 ^ y0, s2 = (x1 & y0) ^ y1, s3 = x1 & y0 & y1
// and next = ctr ? FS(S) : FB(S) with FB(S) = birth[S], FS(S) = survive[S-1].
// For S <= 7 each of FB, FS is one bitop3 of (s2, s1, s0), whose truth-table
// index is S itself: tables `fb` and `fs`.  S = 8, 9 (s3 = 1, s2 = s1 = 0)
// index those tables at s0; the entries that come out wrong there are patched
// by at most two more ops on s3, chosen here at compile time:
//   * fs bit 0 is free (a live centre has S >= 1), so it holds survive[7]:
//     S = 8 with a live centre needs nothing;
//   * S = 8 with a dead centre reads fb bit 0 = 0: B8 needs FB |= s3 (S = 9
//     with a dead centre cannot occur);
//   * S = 9 reads fs bit 1 = survive[0]: where survive[8] differs,
//     FS |= s3 & s0, or FS &= ~(s3 & s0);
//   * B8, S7 and S8 together: one OR of s3 into the result covers all three.
// A rule with none of these (no B8, survive[8] == survive[0]) never forms s3.
struct RuleTables {
  uint8_t fb, fs;
  bool post_or;  // next |= s3
  bool b8;       // FB |= s3
  bool s9_set;   // FS |= s3 & s0
  bool s9_clr;   // FS &= ~(s3 & s0)
  constexpr bool needs_s3() const { return post_or || b8 || s9_set || s9_clr; }
};
constexpr RuleTables rule_tables(Rule r) {
  RuleTables t{};
  t.fb = uint8_t(r.birth & 0xFFu);
  t.fs = uint8_t(((r.survive << 1) & 0xFEu) | ((r.survive >> 7) & 1u));
  const bool b8 = (r.birth >> 8) & 1u, s7 = (r.survive >> 7) & 1u, s8 = (r.survive >> 8) & 1u,
             s0 = r.survive & 1u;
  if (b8 && s7 && s8) {
    t.post_or = true;
  } else {
    t.b8 = b8;
    t.s9_set = s8 && !s0;
    t.s9_clr = !s8 && s0;
  }
  return t;
}
namespace tt {
constexpr uint8_t XOR_AND = uint8_t((A & B) ^ C);      // (a & b) ^ c
constexpr uint8_t OR_AND = uint8_t(A | (B & C));       // a | (b & c)
constexpr uint8_t ANDN_AND = uint8_t(A & ~(B & C));    // a & ~(b & c)
}  // namespace tt

// v_bitop3_b32 with a run-time truth table.
inline uint32_t bop3_host(unsigned TT, uint32_t a, uint32_t b, uint32_t c) {
  uint32_t r = 0;
  for (unsigned i = 0; i < 8; ++i)
    if ((TT >> i) & 1u) r |= ((i & 4u) ? a : ~a) & ((i & 2u) ? b : ~b) & ((i & 1u) ? c : ~c);
  return r;
}

// Host emulation of the general rule: the ops of LifeLike<B, S>::eval
// (csrc/kernels/life_block_impl.hpp), with the tables taken at run time.
inline uint32_t rule_host(Rule rule, HSum a, HSum b, HSum c, uint32_t ctr) {
  const RuleTables t = rule_tables(rule);
  const uint32_t x0 = bop3_host<tt::XOR3>(a.h0, b.h0, c.h0);
  const uint32_t x1 = bop3_host<tt::MAJ>(a.h0, b.h0, c.h0);
  const uint32_t y0 = bop3_host<tt::XOR3>(a.h1, b.h1, c.h1);
  const uint32_t y1 = bop3_host<tt::MAJ>(a.h1, b.h1, c.h1);
  const uint32_t s1 = x1 ^ y0;
  const uint32_t s2 = bop3_host<tt::XOR_AND>(x1, y0, y1);
  const uint32_t s3 = t.needs_s3() ? bop3_host<tt::AND3>(x1, y0, y1) : 0u;
  uint32_t fb = bop3_host(t.fb, s2, s1, x0);
  uint32_t fs = bop3_host(t.fs, s2, s1, x0);
  if (t.b8) fb |= s3;
  if (t.s9_set) fs = bop3_host<tt::OR_AND>(fs, s3, x0);
  if (t.s9_clr) fs = bop3_host<tt::ANDN_AND>(fs, s3, x0);
  uint32_t nxt = bop3_host<tt::SEL>(ctr, fs, fb);
  if (t.post_or) nxt |= s3;
  return nxt;
}

}  // namespace gol
