// gol: command-line front end, contract-compatible with the reference's
// `./a.out <width> <height> <input_file>` (README.md:50-57, src/game.c:224-245).
//
//   gol 1024 1024 input.txt                 # like the serial build
//   gol 32768 32768 --random 7 --gpus 8     # 8 GPUs in one process
//   gol 96 96 in.txt --engine ref           # exact serial src/game.c loop
//
// Width/height default to 30 when <= 0 (src/game.c:233-236); without an
// input file (and no --random) nothing runs and only "Finished" is printed
// (src/game.c:238-241).  The compile-time knobs of the reference
// (GEN_LIMIT, CHECK_SIMILARITY, SIMILARITY_FREQUENCY: README.md:65) are
// runtime flags with the same defaults.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <functional>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "gol/backend.hpp"
#include "gol/batch.hpp"
#include "gol/checkpoint.hpp"
#include "gol/cpu_ref.hpp"
#include "gol/engine.hpp"
#include "gol/io.hpp"
#include "gol/transport.hpp"

using namespace gol;

namespace {

// A fingerprint as 16 hex digits.
std::string hex16(uint64_t v) {
  char b[24];
  std::snprintf(b, sizeof b, "%016llx", (unsigned long long)v);
  return b;
}

// A JSON string literal of s (quotes, backslashes and control bytes escaped):
// tuning values such as trace paths are arbitrary text.
std::string jstr(const std::string& s) {
  std::string o = "\"";
  for (const unsigned char c : s) {
    if (c == '"' || c == '\\') {
      o += '\\';
      o += char(c);
    } else if (c < 0x20) {
      char b[8];
      std::snprintf(b, sizeof b, "\\u%04x", c);
      o += b;
    } else {
      o += char(c);
    }
  }
  return o + "\"";
}

struct Options {
  int64_t W = 0, H = 0;
  std::string input;
  std::string engine = "auto";  // auto | hip | cpu | ref
  std::string layout = "auto";  // auto | bits | u8
  Rule rule;                    // --rule (default B3/S23)
  bool rule_set = false;
  Boundary boundary = Boundary::Torus;  // --boundary
  bool boundary_set = false;
  std::string census;  // --census PATH ("": off)
  bool census_on = false;  // --census, or a resumed checkpoint's setting
  std::string fprint;  // --fingerprint PATH ("": off)
  bool fprint_on = false;  // --fingerprint, --cycle, or a resumed checkpoint's setting
  int cycle = 0;  // --cycle P (0: off)
  std::string decomp = "auto";
  std::string comm = "auto";  // auto | thread | rccl (in-process ranks)
  std::string output;  // default: the matching reference build's file (see default_output)
  std::string style = "serial";  // serial | mpi | async | collective | openmp | cuda
  std::string metrics;
  int64_t gens = 1000;
  int sim_freq = 3;
  bool similarity = true;
  bool random = false;
  uint64_t seed = 1;
  double density = 0.5;
  int ranks = 1, gpus = 0, threads = 0, tmax = 0, epoch = 0, poll = 0, overlap = -1, graphs = 0;
  int u8_compute = -1;  // auto | bytes (0) | bits (1)
  bool show = false;
  bool phase_timing = false;  // per-phase device times in --metrics-json
  int64_t checkpoint_every = 0;     // generations between checkpoints (0: none)
  int64_t start_gen = 0;            // resume: generation of the loaded grid
  int sim_phase = 0;                // resume: similarity counter at start_gen
  std::string checkpoint_dir;       // where they go
  std::string resume;               // checkpoint directory to resume from
  bool gens_set = false, sim_set = false;
  Tuning tune = Tuning::from_env();  // --tune key=value over the GOL_* environment
  // Views of huge grids: patterns stamped after the input is loaded, a density
  // image of the final grid (and of every K-th generation), windows of it.
  struct Place {
    std::string file;
    bool centred = true;
    int64_t x = 0, y = 0;
  };
  struct Window {
    int64_t x = 0, y = 0, w = 0, h = 0;
    std::string path;
  };
  std::vector<Place> places;    // --place FILE[@X,Y], in the order given
  std::vector<Window> windows;  // --window X,Y,W,H:PATH
  std::string density_file;     // --density PATH ("": off)
  int64_t density_by = 0, density_bx = 0;  // --density-block (0: default_density_block)
  int64_t density_every = 0;    // --density-every K (0: the final grid only)
  // Batched small universes (gol/batch.hpp): --batch N soups of W x H cells,
  // seeds SEED, SEED + 1, ..., each run until it repeats or reaches --gens.
  int64_t batch = 0;            // --batch N (0: off)
  int64_t max_period = 64;      // --max-period P
  std::string batch_csv;        // --batch-csv PATH
  std::string batch_census;     // --batch-census PATH: the cluster census of the final grids
  // A rule per universe: --batch-rules FILE|all, R rules.  Without --soups
  // universe b runs rule b on the soup of seed SEED + b; with --soups K
  // universe r*K + j runs rule r on the soup of seed SEED + j.
  std::string batch_rules;      // --batch-rules FILE|all ("": one rule, --rule)
  int64_t soups = 0;            // --soups K (0: not given)
  std::string rules_csv;        // --rules-csv PATH
  std::string refused_with_batch;  // the first single-universe option given, if any
};

// "a,b,c" as integers; false unless exactly n of them.
bool parse_ints(const std::string& s, size_t n, int64_t* out) {
  size_t pos = 0;
  for (size_t k = 0; k < n; ++k) {
    size_t end = k + 1 < n ? s.find(',', pos) : s.size();
    if (end == std::string::npos || end == pos) return false;
    const std::string t = s.substr(pos, end - pos);
    char* rest = nullptr;
    out[k] = std::strtoll(t.c_str(), &rest, 10);
    if (*rest != 0) return false;
    pos = end + 1;
  }
  return true;
}

// The smallest power of two that gives at most 1024 blocks per side.
int64_t default_density_block(int64_t W, int64_t H) {
  int64_t b = 1;
  while (ceil_div(std::max(W, H), b) > 1024) b *= 2;
  return b;
}

// PATH with its %d (any flags and width, e.g. %06d) replaced by the generation.
bool has_generation_field(const std::string& path) {
  const size_t p = path.find('%');
  if (p == std::string::npos || path.find('%', p + 1) != std::string::npos) return false;
  size_t q = p + 1;
  while (q < path.size() && path[q] >= '0' && path[q] <= '9') ++q;
  return q < path.size() && path[q] == 'd';
}
std::string frame_path(const std::string& path, int64_t gen) {
  const size_t p = path.find('%'), q = path.find('d', p);
  const std::string spec = path.substr(p, q - p) + "lld";
  char b[64];
  std::snprintf(b, sizeof b, spec.c_str(), (long long)gen);
  return path.substr(0, p) + b + path.substr(q + 1);
}

struct Stamp {
  RlePattern pat;
  int64_t x = 0, y = 0;
};
// The --place patterns, read and checked against the rule and the grid.
std::vector<Stamp> load_stamps(const Options& o) {
  std::vector<Stamp> out;
  for (const Options::Place& pl : o.places) {
    std::ifstream f(pl.file, std::ios::binary);
    GOL_REQUIRE(f.good(), "--place: cannot read '" + pl.file + "'");
    const std::string text((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    Stamp s;
    try {
      s.pat = parse_rle(text);
    } catch (const std::exception& e) {
      throw Error("--place " + pl.file + ": " + e.what());
    }
    if (!s.pat.rule.empty()) {
      Rule r;
      try {
        r = parse_rule(s.pat.rule);
      } catch (const std::exception& e) {
        throw Error("--place " + pl.file + ": " + e.what());
      }
      if (r != o.rule)
        throw Error("--place " + pl.file + ": the pattern's rule " + rule_string(r) + " is not the engine's " +
                    rule_string(o.rule));
    }
    s.x = pl.centred ? (o.W - s.pat.w) / 2 : pl.x;
    s.y = pl.centred ? (o.H - s.pat.h) / 2 : pl.y;
    if (s.x < 0 || s.y < 0 || s.pat.w > o.W - s.x || s.pat.h > o.H - s.y)
      throw Error("--place " + pl.file + ": rectangle x=" + std::to_string(s.x) + " y=" + std::to_string(s.y) +
                  " w=" + std::to_string(s.pat.w) + " h=" + std::to_string(s.pat.h) + " leaves the grid of " +
                  std::to_string(o.W) + " x " + std::to_string(o.H) + " cells (patterns do not wrap)");
    out.push_back(std::move(s));
  }
  return out;
}

// A window of 0/1 cells as RLE (PATH ends in .rle) or in the text format.
void write_window(const Options::Window& w, const std::vector<uint8_t>& cells, Rule rule) {
  if (w.path.size() >= 4 && w.path.compare(w.path.size() - 4, 4, ".rle") == 0) {
    std::ofstream f(w.path, std::ios::binary);
    GOL_REQUIRE(f.good(), "--window: cannot write '" + w.path + "'");
    f << format_rle(cells.data(), w.w, w.h, rule_string(rule));
  } else {
    write_text_grid(w.path, w.w, w.h, cells.data());
  }
}

[[noreturn]] void usage(int code) {
  std::fprintf(code ? stderr : stdout,
               "usage: gol [width] [height] [input_file] [options]\n"
               "  --engine auto|hip|cpu|ref   compute engine (ref = exact serial game.c loop)\n"
               "  --layout auto|bits|u8       cell storage (bits needs width %% 32 == 0)\n"
               "  --u8-compute auto|bits|bytes  byte-layout epochs on bit words (packed once per\n"
               "                              epoch; auto: on the GPU) or on the bytes themselves\n"
               "  --rule NAME|B../S..         Life-like rule: B<digits>/S<digits> (e.g. B36/S23) or a name:\n"
               "                              life, highlife, daynight, seeds, replicator, lwod, 34life\n"
               "                              (default B3/S23; no B0; the hip engine runs the named ones,\n"
               "                              the cpu and ref engines any)\n"
               "  --boundary torus|dead       what lies beyond the grid's edge: the torus wraps (default);\n"
               "                              dead = a bounded plane whose outside is dead in every\n"
               "                              generation (hip engine: B3/S23 only; no lds kernels, graphs)\n"
               "  --census PATH               count the live cells of every generation inside the temporal\n"
               "                              blocks and write 'generation,population' lines to PATH (hip\n"
               "                              engine: B3/S23 on the torus; no lds kernels, graphs)\n"
               "  --fingerprint PATH          accumulate a position-dependent 64-bit fingerprint of every\n"
               "                              generation inside the temporal blocks and write\n"
               "                              'generation,fingerprint' lines (16 hex digits) to PATH (hip\n"
               "                              engine: B3/S23 on the torus; no lds kernels, graphs, census)\n"
               "  --cycle P                   run until the grid repeats with a period <= P (confirmed on the\n"
               "                              cells) or to the generation limit, and print a 'Cycle:' line\n"
               "  --gens N                    GEN_LIMIT (default 1000)\n"
               "  --sim-freq F                SIMILARITY_FREQUENCY (default 3)\n"
               "  --no-similarity             disable the similarity check\n"
               "  --random SEED[:DENSITY]     random initial grid instead of an input file\n"
               "  --output PATH|none          output file (default: the reference build's name for\n"
               "                              --style: ./game_output.out, ./mpi_output.out, ...)\n"
               "  --gpus N                    run on N GPUs in this process (one rank each)\n"
               "  --ranks N                   in-process ranks (subdomains; share devices)\n"
               "  --comm auto|thread|rccl     in-process halo transport (auto: rccl when every rank\n"
               "                              has a GPU of its own, else thread)\n"
               "  --decomp auto|PxQ           process grid (Px columns x Py rows)\n"
               "  --tmax T --epoch D --poll N temporal block, halo depth, poll interval\n"
               "  --overlap auto|on|off|trigger\n"
               "                              trigger = an epoch's new boundary rows are sent as soon\n"
               "                              as the groups writing them finish (on = trigger);\n"
               "                              off = no overlap; auto = time plain against trigger\n"
               "                              epochs on the ranks, keep the faster\n"
               "  --graphs auto|on|off        replay full epochs as captured HIP graphs\n"
               "  --threads N                 host threads for the cpu engine\n"
               "  --tune KEY=VALUE            runtime tuning (repeatable; --tune help lists the keys,\n"
               "                              their GOL_* overrides and defaults)\n"
               "  --style serial|mpi|async|collective|openmp|cuda\n"
               "                              stdout format and output name of that reference build\n"
               "  --metrics-json PATH         write run metrics as JSON\n"
               "  --phase-timing              time kernels / halos / fills / reductions (per-phase\n"
               "                              device times in --metrics-json; adds events to the loop)\n"
               "  --checkpoint-every K        write a checkpoint every K generations ...\n"
               "  --checkpoint-dir DIR        ... into DIR (grid-<gen>.txt + meta.json; crash-safe)\n"
               "  --resume DIR                continue from a checkpoint: same final grid and\n"
               "                              Generations line as the uninterrupted run\n"
               "  --place FILE[@X,Y]          stamp the RLE pattern FILE onto the loaded grid (live cells are\n"
               "                              added), its first cell at column X, row Y, or centred;\n"
               "                              repeatable, in order; with input 'none' the grid starts empty\n"
               "  --density PATH              write the block populations of the final grid as a PGM image\n"
               "  --density-block B|BYxBX     cells per block (default: the smallest power of two that gives\n"
               "                              at most 1024 blocks per side)\n"
               "  --density-every K           also one image per generation that is a multiple of K; PATH\n"
               "                              must contain %%d (any width), the generation\n"
               "  --window X,Y,W,H:PATH       write that rectangle of the final grid: RLE where PATH ends in\n"
               "                              .rle, else the text format; repeatable\n"
               "  --show                      print the final grid with VT100 escapes\n"
               "  --batch N                   run N independent random universes of width x height cells (width\n"
               "                              32 or 64, height 8, 16, 32 or 64; input 'none', --random SEED[:D]:\n"
               "                              universe b has seed SEED + b) until each repeats or reaches --gens;\n"
               "                              engines hip (B3/S23 and the named rules) and cpu; prints one summary\n"
               "                              line; not with the single-universe outputs and options\n"
               "  --max-period P              --batch: the largest period recognised, 1 to 65536 (default 64)\n"
               "  --batch-csv PATH            --batch: write 'universe,seed,generations,stop,period,population'\n"
               "                              lines, one per universe (stop: limit, cycle or extinction)\n"
               "  --batch-census PATH         --batch: find the clusters of every final grid (live cells at most 2\n"
               "                              cells apart) and write 'signature,name,cells,height,width,spanning,\n"
               "                              count', one line per kind of cluster, the most common first\n"
               "  --batch-rules FILE|all      --batch with a rule per universe, N = the number of rules R (an explicit\n"
               "                              --batch N must agree): FILE holds one rule per line (# comments and\n"
               "                              blank lines skipped), all = the 131072 Life-like rules without B0;\n"
               "                              universe b runs rule b on seed SEED + b; any rule on either engine;\n"
               "                              not with --rule; prints a second line 'Rules: R rules x K soups' and\n"
               "                              adds a 'rule' column after 'seed' to --batch-csv\n"
               "  --soups K                   --batch-rules: the cross product, N = R * K: universe r*K + j runs rule\n"
               "                              r on seed SEED + j\n"
               "  --rules-csv PATH            --batch-rules: write 'rule,soups,limit,cycle,extinction,\n"
               "                              mean_generations,max_generations,max_period,mean_population' lines,\n"
               "                              one per rule\n");
  std::exit(code);
}

Options parse(int argc, char** argv) {
  Options o;
  std::vector<std::string> pos;
  for (int i = 1; i < argc; ++i) {
    std::string a = argv[i];
    auto next = [&]() -> std::string {
      if (i + 1 >= argc) usage(2);
      return argv[++i];
    };
    // The options of one universe's run, which --batch refuses.
    static const char* kSingle[] = {"--output", "--census", "--fingerprint", "--cycle", "--density", "--density-block",
                                    "--density-every", "--window", "--place", "--checkpoint-every", "--checkpoint-dir",
                                    "--resume", "--decomp", "--show"};
    if (o.refused_with_batch.empty() && std::find_if(std::begin(kSingle), std::end(kSingle), [&](const char* k) {
          return a == k;
        }) != std::end(kSingle))
      o.refused_with_batch = a;
    if (a == "-h" || a == "--help") usage(0);
    else if (a == "--batch") {
      o.batch = std::atoll(next().c_str());
      if (o.batch < 1) throw Error("--batch: the number of universes must be at least 1");
    } else if (a == "--max-period") o.max_period = std::atoll(next().c_str());
    else if (a == "--batch-csv") o.batch_csv = next();
    else if (a == "--batch-census") o.batch_census = next();
    else if (a == "--batch-rules") o.batch_rules = next();
    else if (a == "--rules-csv") o.rules_csv = next();
    else if (a == "--soups") {
      o.soups = std::atoll(next().c_str());
      if (o.soups < 1) throw Error("--soups: the number of soups per rule must be at least 1");
    }
    else if (a == "--engine") o.engine = next();
    else if (a == "--layout") o.layout = next();
    else if (a == "--u8-compute") {
      std::string v = next();
      if (v != "auto" && v != "bits" && v != "bytes") usage(2);
      o.u8_compute = v == "bits" ? 1 : v == "bytes" ? 0 : -1;
    }
    else if (a == "--rule") o.rule = parse_rule(next()), o.rule_set = true;
    else if (a == "--boundary") o.boundary = parse_boundary(next()), o.boundary_set = true;
    else if (a == "--census") o.census = next(), o.census_on = true;
    else if (a == "--fingerprint") o.fprint = next(), o.fprint_on = true;
    else if (a == "--cycle") {
      o.cycle = std::atoi(next().c_str());
      if (o.cycle < 1) throw Error("--cycle: the largest period must be at least 1");
      o.fprint_on = true;
    }
    else if (a == "--decomp") o.decomp = next();
    else if (a == "--comm") o.comm = next();
    else if (a == "--gens") o.gens = std::atoll(next().c_str()), o.gens_set = true;
    else if (a == "--sim-freq") o.sim_freq = std::atoi(next().c_str()), o.sim_set = true;
    else if (a == "--no-similarity") o.similarity = false, o.sim_set = true;
    else if (a == "--checkpoint-every") o.checkpoint_every = std::atoll(next().c_str());
    else if (a == "--checkpoint-dir") o.checkpoint_dir = next();
    else if (a == "--resume") o.resume = next();
    else if (a == "--output") o.output = next();
    else if (a == "--style") o.style = next();
    else if (a == "--metrics-json") o.metrics = next();
    else if (a == "--gpus") o.gpus = std::atoi(next().c_str());
    else if (a == "--ranks") o.ranks = std::atoi(next().c_str());
    else if (a == "--threads") o.threads = std::atoi(next().c_str());
    else if (a == "--tune") {
      const std::string kv = next();
      if (kv == "help") {
        for (const TuningKey& k : tuning_keys())
          std::printf("%-22s %-13s %-27s default %-6s %s\n", k.key, k.cls, k.env, *k.dflt ? k.dflt : "''", k.doc);
        std::exit(0);
      }
      o.tune.set(kv);
    }
    else if (a == "--tmax") o.tmax = std::atoi(next().c_str());
    else if (a == "--epoch" || a == "--halo-depth") o.epoch = std::atoi(next().c_str());
    else if (a == "--poll" || a == "--poll-every") o.poll = std::atoi(next().c_str());
    else if (a == "--overlap") {
      std::string v = next();
      GOL_REQUIRE(v == "auto" || v == "on" || v == "off" || v == "trigger", "--overlap: auto, on, off or trigger");
      o.overlap = v == "on" ? 3 : v == "off" ? 0 : v == "trigger" ? 3 : -1;
    } else if (a == "--graphs") {
      std::string v = next();
      o.graphs = v == "on" ? 1 : v == "off" ? 0 : -1;
    }
    else if (a == "--place") {
      const std::string v = next();
      Options::Place pl;
      pl.file = v;
      const size_t at = v.rfind('@');
      int64_t xy[2];
      if (at != std::string::npos && parse_ints(v.substr(at + 1), 2, xy)) {
        pl.file = v.substr(0, at);
        pl.centred = false;
        pl.x = xy[0], pl.y = xy[1];
      }
      o.places.push_back(pl);
    } else if (a == "--density") o.density_file = next();
    else if (a == "--density-block") {
      const std::string v = next();
      const size_t x = v.find('x');
      char* rest = nullptr;
      o.density_by = std::strtoll(v.c_str(), &rest, 10);
      o.density_bx = o.density_by;
      if (x != std::string::npos) {
        if (rest != v.c_str() + x) throw Error("--density-block: B or BYxBX, got '" + v + "'");
        o.density_bx = std::strtoll(v.c_str() + x + 1, &rest, 10);
      }
      if (*rest != 0 || o.density_by < 1 || o.density_bx < 1) throw Error("--density-block: B or BYxBX, got '" + v + "'");
    } else if (a == "--density-every") {
      o.density_every = std::atoll(next().c_str());
      if (o.density_every < 1) throw Error("--density-every: K must be at least 1");
    } else if (a == "--window") {
      const std::string v = next();
      const size_t c = v.find(':');
      int64_t r[4];
      if (c == std::string::npos || c + 1 >= v.size() || !parse_ints(v.substr(0, c), 4, r))
        throw Error("--window: X,Y,W,H:PATH, got '" + v + "'");
      o.windows.push_back({r[0], r[1], r[2], r[3], v.substr(c + 1)});
    }
    else if (a == "--show") o.show = true;
    else if (a == "--phase-timing") o.phase_timing = true;
    else if (a == "--random") {
      std::string v = next();
      o.random = true;
      auto c = v.find(':');
      o.seed = std::strtoull(v.substr(0, c).c_str(), nullptr, 10);
      if (c != std::string::npos) o.density = std::atof(v.substr(c + 1).c_str());
    } else if (!a.empty() && a[0] == '-' && a.size() > 1) {
      std::fprintf(stderr, "unknown option %s\n", a.c_str());
      usage(2);
    } else pos.push_back(a);
  }
  if (pos.size() > 0) o.W = std::atoll(pos[0].c_str());
  if (pos.size() > 1) o.H = std::atoll(pos[1].c_str());
  if (pos.size() > 2) o.input = pos[2];
  if (o.batch_rules.empty() && (o.soups > 0 || !o.rules_csv.empty()))
    throw Error("--soups and --rules-csv need --batch-rules FILE|all");
  if (o.batch > 0 || !o.batch_rules.empty()) {
    if (!o.batch_rules.empty() && o.rule_set)
      throw Error("--batch-rules with --rule: the rules come from the list");
    if (o.input != "none" || !o.random)
      throw Error("--batch runs random soups: give the input 'none' and --random SEED[:DENSITY]");
    if (!o.refused_with_batch.empty())
      throw Error("--batch with " + o.refused_with_batch + ": a batch has no single grid to write, count, view or "
                  "checkpoint (its results go to --batch-csv and --metrics-json)");
    if (o.gpus > 1 || o.ranks > 1) throw Error("--batch runs on one device: not with --gpus or --ranks above 1");
    return o;
  }
  if (o.max_period != 64 || !o.batch_csv.empty()) throw Error("--max-period and --batch-csv need --batch N");
  if (!o.batch_census.empty()) throw Error("--batch-census needs --batch N or --batch-rules FILE|all");
  if (!o.resume.empty()) {
    // The checkpoint fixes the grid and the counters; --gens / --sim-freq /
    // --no-similarity given on the command line still win.
    const CheckpointMeta m = checkpoint_load(o.resume);
    if ((o.W > 0 && o.W != m.W) || (o.H > 0 && o.H != m.H))
      throw Error("--resume: checkpoint is " + std::to_string(m.W) + "x" + std::to_string(m.H) +
                  ", not the requested " + std::to_string(o.W) + "x" + std::to_string(o.H));
    // The rule is the checkpoint's; a different explicit --rule would continue
    // another automaton from this grid under the old generation count.
    const Rule ck_rule = parse_rule(m.rule);
    if (o.rule_set && o.rule != ck_rule)
      throw Error("--resume: checkpoint was taken with --rule " + m.rule + ", not " + rule_string(o.rule));
    o.rule = ck_rule;
    // So is the boundary.
    const Boundary ck_boundary = parse_boundary(m.boundary);
    if (o.boundary_set && o.boundary != ck_boundary)
      throw Error("--resume: checkpoint was taken with --boundary " + m.boundary + ", not " +
                  boundary_name(o.boundary));
    o.boundary = ck_boundary;
    // A census is per run: --census counts the resumed run whether or not the first one did.
    o.census_on = o.census_on || m.census;
    o.fprint_on = o.fprint_on || m.fingerprint;
    o.W = m.W;
    o.H = m.H;
    o.input = checkpoint_grid_path(o.resume);
    if (!o.gens_set) o.gens = m.gen_limit;
    // The checkpoint's similarity phase counts modulo its own frequency; a
    // different one would match neither the original run nor a fresh run
    // at the new frequency.
    if (o.sim_set && o.similarity && o.sim_freq != m.sim_freq)
      throw Error("--resume: checkpoint was taken with --sim-freq " + std::to_string(m.sim_freq) +
                  "; resuming with --sim-freq " + std::to_string(o.sim_freq) + " would shift the similarity checks");
    if (!o.sim_set) o.similarity = m.check_similarity;
    o.sim_freq = m.sim_freq;
    o.start_gen = m.generation;
    o.sim_phase = m.sim_phase;
    if (o.layout == "auto" && (m.layout == "bits" || m.layout == "u8")) o.layout = m.layout;
  }
  if (o.W <= 0) o.W = 30;
  if (o.H <= 0) o.H = 30;
  if (o.gpus > 0) o.ranks = o.gpus;
  if (o.density_every > 0) {
    if (o.density_file.empty()) throw Error("--density-every needs --density PATH");
    if (!has_generation_field(o.density_file))
      throw Error("--density-every: the path '" + o.density_file + "' needs one %d (any width) for the generation");
  } else if (!o.density_file.empty() && o.density_file.find('%') != std::string::npos && !has_generation_field(o.density_file)) {
    throw Error("--density: the path '" + o.density_file + "' may hold one %d (the generation) and no other %");
  }
  if (!o.density_file.empty()) {
    if (o.density_by == 0) o.density_by = o.density_bx = default_density_block(o.W, o.H);
  }
  for (const Options::Window& w : o.windows)
    if (w.w < 1 || w.h < 1 || w.x < 0 || w.y < 0 || w.w > o.W - w.x || w.h > o.H - w.y ||
        w.w > Backend::kWindowCellsMax / w.h)
      throw Error("--window: rectangle x=" + std::to_string(w.x) + " y=" + std::to_string(w.y) + " w=" +
                  std::to_string(w.w) + " h=" + std::to_string(w.h) + " must lie inside the grid of " +
                  std::to_string(o.W) + " x " + std::to_string(o.H) + " cells and hold at most 2^26 cells");
  // --metrics-json does not imply --phase-timing: the event pairs around
  // every kernel, exchange, fill and reduction would sit inside the timed
  // loop that loop_ms and cell_updates_per_s report.
  static const char* kStyles[] = {"serial", "mpi", "async", "collective", "openmp", "cuda"};
  if (std::find(std::begin(kStyles), std::end(kStyles), o.style) == std::end(kStyles)) usage(2);
  // Output file of the matching reference build: src/game.c:27,
  // src/game_mpi.c:29, src/game_mpi_async.c:432, src/game_mpi_collective.c:429,
  // src/game_openmp.c:445, src/game_cuda.cu:37.
  if (o.output.empty()) o.output = "./" + std::string(o.style == "serial" ? "game" : o.style) + "_output.out";
  return o;
}

void show(const std::vector<uint8_t>& g, int64_t W, int64_t H) {
  // VT100 viewer (src/game.c:42-58): reverse video for live cells.
  std::printf("\033[H");
  for (int64_t y = 0; y < H; ++y) {
    for (int64_t x = 0; x < W; ++x) std::printf(g[size_t(y * W + x)] ? "\033[07m  \033[m" : "  ");
    std::printf("\033[E");
  }
  std::fflush(stdout);
}

double ms_since(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// --batch-rules: the rules of FILE (one per line, # comments and blank lines
// skipped), or all Life-like rules without B0.
std::vector<Rule> load_batch_rules(const std::string& arg) {
  std::vector<Rule> rules;
  if (arg == "all") {
    for (int64_t i = 0; i < kLifeLikeRules; ++i) rules.push_back(life_like_rule(i));
    return rules;
  }
  std::ifstream f(arg);
  GOL_REQUIRE(f.good(), "--batch-rules: cannot read '" + arg + "'");
  std::string line;
  for (int64_t n = 1; std::getline(f, line); ++n) {
    const size_t hash = line.find('#');
    if (hash != std::string::npos) line.erase(hash);
    const size_t b = line.find_first_not_of(" \t\r"), e = line.find_last_not_of(" \t\r");
    if (b == std::string::npos) continue;
    try {
      rules.push_back(parse_rule(line.substr(b, e - b + 1)));
    } catch (const std::exception& ex) {
      throw Error("--batch-rules " + arg + ": line " + std::to_string(n) + ": " + ex.what());
    }
  }
  if (rules.empty()) throw Error("--batch-rules " + arg + ": the file names no rule");
  return rules;
}

// --batch: one call of the batch engine, the CSVs, the metrics and the summary.
int run_batch(const Options& o) {
  std::string engine = o.engine;
  if (engine == "auto") engine = hip_available() ? "hip" : "cpu";
  if (engine != "hip" && engine != "cpu") throw Error("--batch runs on --engine hip or cpu, not " + engine);
  BatchConfig cfg;
  cfg.W = int(std::min<int64_t>(o.W, 1 << 20));
  cfg.H = int(std::min<int64_t>(o.H, 1 << 20));
  cfg.rule = o.rule;
  cfg.boundary = o.boundary;
  cfg.max_gens = o.gens;
  cfg.max_period = o.max_period;
  cfg.clusters = !o.batch_census.empty();
  BatchInput in;
  in.B = o.batch;
  const bool by_rule = !o.batch_rules.empty();
  const int64_t K = std::max<int64_t>(o.soups, 1);
  if (by_rule) {
    cfg.rules = load_batch_rules(o.batch_rules);
    cfg.soups_per_rule = K;
    cfg.share_soups = o.soups > 0;
    const int64_t R = int64_t(cfg.rules.size());
    if (o.batch > 0 && (K > kBatchMax || o.batch != R * K))
      throw Error("--batch " + std::to_string(o.batch) + ": " + std::to_string(R) + " rules x " + std::to_string(K) +
                  " soups make " + std::to_string(R * K) + " universes");
    in.B = K > kBatchMax ? kBatchMax + 1 : R * K;
  }
  in.seed = o.seed;
  in.density = o.density;
  const BatchResult r = engine == "hip" ? run_batch_hip(0, cfg, in, o.tune) : run_batch_cpu(o.threads, cfg, in);
  int64_t counts[3] = {0, 0, 0};
  int32_t longest = 0;
  for (int64_t b = 0; b < in.B; ++b) {
    ++counts[r.stop[size_t(b)]];
    longest = std::max(longest, r.generations[size_t(b)]);
  }
  if (!o.batch_csv.empty()) {
    std::ofstream f(o.batch_csv);
    GOL_REQUIRE(f.good(), "--batch-csv: cannot write '" + o.batch_csv + "'");
    f << (by_rule ? "universe,seed,rule,generations,stop,period,population\n"
                  : "universe,seed,generations,stop,period,population\n");
    for (int64_t b = 0; b < in.B; ++b)
      f << b << "," << in.seed + uint64_t(batch_soup(cfg, b)) << ","
        << (by_rule ? rule_string(batch_rule(cfg, b)) + "," : std::string()) << r.generations[size_t(b)] << ","
        << kBatchStopNames[r.stop[size_t(b)]] << "," << r.period[size_t(b)] << "," << r.population[size_t(b)] << "\n";
  }
  if (!o.rules_csv.empty()) {
    std::ofstream f(o.rules_csv);
    GOL_REQUIRE(f.good(), "--rules-csv: cannot write '" + o.rules_csv + "'");
    f << "rule,soups,limit,cycle,extinction,mean_generations,max_generations,max_period,mean_population\n";
    for (size_t ri = 0; ri < cfg.rules.size(); ++ri) {
      int64_t c[3] = {0, 0, 0}, gens = 0, pop = 0;
      int32_t max_gens = 0, max_per = 0;
      for (size_t b = ri * size_t(K); b < (ri + 1) * size_t(K); ++b) {
        ++c[r.stop[b]];
        gens += r.generations[b], pop += r.population[b];
        max_gens = std::max(max_gens, r.generations[b]), max_per = std::max(max_per, r.period[b]);
      }
      char line[256];
      std::snprintf(line, sizeof line, "%s,%lld,%lld,%lld,%lld,%.6f,%d,%d,%.6f\n", rule_string(cfg.rules[ri]).c_str(),
                    (long long)K, (long long)c[0], (long long)c[1], (long long)c[2], double(gens) / double(K),
                    int(max_gens), int(max_per), double(pop) / double(K));
      f << line;
    }
  }
  std::vector<ClusterKind> kinds;
  if (cfg.clusters) {
    kinds = cluster_table(r.census);
    std::ofstream f(o.batch_census);
    GOL_REQUIRE(f.good(), "--batch-census: cannot write '" + o.batch_census + "'");
    f << "signature,name,cells,height,width,spanning,count\n";
    for (const ClusterKind& k : kinds) {
      char sig[17];
      std::snprintf(sig, sizeof sig, "%016llx", (unsigned long long)k.signature);
      f << sig << "," << cluster_name(k.signature) << "," << k.cells << "," << k.height << "," << k.width << ","
        << int(k.spanning) << "," << k.count << "\n";
    }
  }
  if (!o.metrics.empty()) {
    std::ofstream f(o.metrics);
    f << "{\"engine\": " << jstr(engine) << ", \"rule\": " << jstr(rule_string(o.rule))
      << ", \"boundary\": " << jstr(boundary_name(o.boundary)) << ", \"W\": " << o.W << ", \"H\": " << o.H
      << ", \"batch\": " << in.B << ", \"seed\": " << in.seed << ", \"density\": " << in.density
      << ", \"max_gens\": " << cfg.max_gens << ", \"max_period\": " << cfg.max_period
      << ", \"batch_kernel_ms\": " << r.kernel_ms << ", \"batch_variant\": " << jstr(r.variant)
      << ", \"limit\": " << counts[0] << ", \"cycle\": " << counts[1] << ", \"extinction\": " << counts[2]
      << ", \"max_generations\": " << longest;
    if (by_rule) f << ", \"batch_rules\": " << cfg.rules.size() << ", \"batch_soups\": " << K;
    if (cfg.clusters)
      f << ", \"batch_clusters\": " << r.census.size() << ", \"batch_cluster_kinds\": " << kinds.size()
        << ", \"batch_clusters_ms\": " << r.census.ms;
    f << "}\n";
  }
  std::printf("Batch: %lld universes: %lld limit, %lld cycle, %lld extinction; largest generations %d\n",
              (long long)in.B, (long long)counts[0], (long long)counts[1], (long long)counts[2], int(longest));
  if (by_rule) std::printf("Rules: %lld rules x %lld soups\n", (long long)cfg.rules.size(), (long long)K);
  if (cfg.clusters) {
    std::printf("Clusters: %lld in %lld universes, %lld kinds", (long long)r.census.size(), (long long)in.B,
                (long long)kinds.size());
    if (!kinds.empty())
      std::printf("; most common %s x%lld", cluster_name(kinds[0].signature).c_str(), (long long)kinds[0].count);
    std::printf("\n");
  }
  std::fflush(stdout);
  return 0;
}

int run(const Options& o) {
  if (o.batch > 0 || !o.batch_rules.empty()) return run_batch(o);
  // Input 'none' with patterns to place: the grid starts empty.
  const bool empty_start = o.input == "none" && !o.random && !o.places.empty() && o.resume.empty();
  const bool have_input = o.random || !o.input.empty();
  if (!have_input) {
    std::printf("Finished\n");
    return 0;
  }
  std::string engine = o.engine;
  if (engine == "auto") engine = hip_available() ? "hip" : "cpu";
  Layout layout = Layout::Bits;
  if (o.layout == "u8" || (o.layout == "auto" && o.W % 32 != 0)) layout = Layout::U8;
  else if (o.layout != "auto" && o.layout != "bits") throw Error("unknown layout " + o.layout);

  double read_ms = 0, write_ms = 0;
  RunResult res;
  std::vector<uint8_t> final_grid;
  const bool want_grid = o.output != "none" || o.show;

  if (engine == "ref" && (!o.resume.empty() || o.checkpoint_every > 0))
    throw Error("--engine ref is the plain serial loop from generation 0: no checkpoint / resume");
  if (o.cycle > 0 && (engine == "ref" || o.checkpoint_every > 0))
    throw Error("--cycle runs Engine::find_cycle: not with --engine ref (the plain serial loop) or --checkpoint-every");
  if (o.density_every > 0 && (engine == "ref" || o.cycle > 0))
    throw Error("--density-every runs the engine in chunks: not with --engine ref (the plain serial loop) or --cycle");
  const std::vector<Stamp> stamps = load_stamps(o);
  double density_ms = 0;
  int64_t density_frames = 0;
  // The final density image's name: the reported generation where the path has a %d.
  const auto density_path = [&](int64_t gen) {
    return has_generation_field(o.density_file) ? frame_path(o.density_file, gen) : o.density_file;
  };
  CycleResult cyc;
  if (engine == "ref") {
    // Exact serial semantics (src/game.c), every generation evaluated eagerly.
    auto t0 = std::chrono::steady_clock::now();
    std::vector<uint8_t> grid;
    if (o.random) {
      grid.resize(size_t(o.W * o.H));
      uint32_t th = density_thresh(o.density);
      for (int64_t r = 0; r < o.H; ++r)
        for (int64_t x = 0; x < o.W; ++x) grid[size_t(r * o.W + x)] = rng_cell(o.seed, r, x, th);
    } else if (empty_start) {
      grid.assign(size_t(o.W * o.H), 0);
    } else {
      read_text_grid(o.input, o.W, o.H, grid);
    }
    for (const Stamp& s : stamps)  // stamped on the host grid before the serial loop
      for (int64_t i = 0; i < s.pat.h; ++i)
        for (int64_t j = 0; j < s.pat.w; ++j)
          grid[size_t((s.y + i) * o.W + s.x + j)] |= s.pat.cells[size_t(i * s.pat.w + j)];
    read_ms = ms_since(t0);
    RefResult rr = cpu_reference_run(grid, o.W, o.H, o.gens, o.similarity, o.sim_freq, o.threads, o.rule,
                                     o.boundary, o.census_on, o.fprint_on);
    res.population = rr.population;
    res.fingerprint = rr.fingerprint;
    res.generations = rr.generations;
    res.loop_ms = rr.loop_ms;
    res.executed = rr.generations;
    final_grid = std::move(grid);
    if (o.output != "none") {
      auto t1 = std::chrono::steady_clock::now();
      write_text_grid(o.output, o.W, o.H, final_grid.data());
      write_ms = ms_since(t1);
    }
    if (!o.density_file.empty()) {
      const int64_t nbx = ceil_div(o.W, o.density_bx), nby = ceil_div(o.H, o.density_by);
      std::vector<uint64_t> counts(size_t(nbx * nby), 0);
      for (int64_t r = 0; r < o.H; ++r)
        for (int64_t x = 0; x < o.W; ++x)
          counts[size_t((r / o.density_by) * nbx + x / o.density_bx)] += final_grid[size_t(r * o.W + x)] != 0;
      write_pgm(density_path(res.generations), density_image(counts.data(), o.density_by, o.density_bx, o.H, o.W).data(),
                nbx, nby);
    }
    for (const Options::Window& w : o.windows) {
      std::vector<uint8_t> cells(size_t(w.w * w.h));
      for (int64_t i = 0; i < w.h; ++i)
        for (int64_t j = 0; j < w.w; ++j)
          cells[size_t(i * w.w + j)] = final_grid[size_t((w.y + i) * o.W + w.x + j)] != 0;
      write_window(w, cells, o.rule);
    }
  } else {
    const int P = std::max(1, o.ranks);
    EngineConfig cfg;
    cfg.W = o.W;
    cfg.H = o.H;
    cfg.layout = layout;
    cfg.rule = o.rule;
    cfg.boundary = o.boundary;
    cfg.census = o.census_on;
    cfg.fingerprint = o.fprint_on;
    cfg.decomp = o.decomp;
    cfg.gen_limit = o.gens;
    cfg.check_similarity = o.similarity;
    cfg.sim_freq = o.sim_freq;
    cfg.tmax = o.tmax;
    cfg.epoch = o.epoch;
    cfg.poll_gens = o.poll;
    cfg.overlap = o.overlap;
    cfg.graphs = o.graphs;
    cfg.u8_compute = o.u8_compute;
    cfg.start_gen = o.start_gen;
    cfg.sim_phase = o.sim_phase;
    cfg.tune = o.tune;
    int ndev = 1;
    if (engine == "hip") {
      GOL_REQUIRE(hip_available(), "--engine hip: no HIP device available");
      ndev = o.gpus > 0 ? o.gpus : 1;
    }
    std::vector<std::unique_ptr<Backend>> backends(P);
    std::vector<std::unique_ptr<Transport>> transports(P);
    std::vector<std::unique_ptr<Engine>> engines(P);
    auto hub = std::make_shared<ThreadHub>(P);
    // One process, P rank threads.  RCCL needs every rank on a GPU of its
    // own (it refuses duplicate devices in one communicator); ranks that
    // share devices, and CPU ranks, use the thread transport.
    std::string comm = o.comm;
    if (comm == "auto") comm = (engine == "hip" && P > 1 && P <= ndev) ? "rccl" : "thread";
    if (comm == "rccl" && P > 1) {
      GOL_REQUIRE(engine == "hip", "--comm rccl needs --engine hip");
      GOL_REQUIRE(P <= ndev, "--comm rccl needs one GPU per rank (--gpus N, not --ranks)");
    }
    std::vector<uint8_t> uid;
    if (comm == "rccl" && P > 1) uid = rccl_unique_id();
    for (int r = 0; r < P; ++r)
      backends[r] = engine == "hip" ? make_hip_backend(r % ndev, o.tune)
                                    : make_cpu_backend(o.threads > 0 ? o.threads : 0, -1, o.tune);
    if (P == 1) {
      transports[0] = std::make_unique<SelfTransport>();
    } else if (comm == "rccl") {
      std::vector<std::thread> th;
      std::vector<std::string> errs(P);
      for (int r = 0; r < P; ++r)
        th.emplace_back([&, r] {
          try {
            backends[r]->bind_thread();
            transports[r] = make_rccl_transport(uid, r, P, r % ndev, o.tune);
          } catch (const std::exception& e) {
            errs[r] = e.what();
          }
        });
      for (auto& t : th) t.join();
      for (auto& e : errs)
        if (!e.empty()) throw Error(e);
    } else {
      for (int r = 0; r < P; ++r) transports[r] = std::make_unique<ThreadTransport>(hub, r, backends[r].get(), o.tune);
    }
    for (int r = 0; r < P; ++r) {
      engines[r] = std::make_unique<Engine>(cfg, backends[r].get(), transports[r].get());
      engines[r]->set_phase_timing(o.phase_timing);
    }

    auto par = [&](const std::function<void(int)>& fn) {
      std::vector<std::thread> th;
      std::vector<std::string> errs(P);
      for (int r = 0; r < P; ++r)
        th.emplace_back([&, r] {
          try {
            backends[r]->bind_thread();  // a new thread starts on device 0
            fn(r);
          } catch (const std::exception& e) {
            errs[r] = e.what();
          }
        });
      for (auto& t : th) t.join();
      for (auto& e : errs)
        if (!e.empty()) throw Error(e);
    };

    auto t0 = std::chrono::steady_clock::now();
    std::vector<double> parse_ms(P, 0.0), load_ms(P, 0.0);
    par([&](int r) {
      Engine& e = *engines[r];
      if (o.random) {
        e.init_random(o.seed, o.density);
      } else if (empty_start) {
        e.init_random(0, 0.0);  // no cell alive
      } else {
        // Uninitialised host tile (a multi-GB zero fill would cost more than
        // the parallel read that overwrites it).
        const auto a = std::chrono::steady_clock::now();
        std::unique_ptr<uint8_t[]> tile(new uint8_t[size_t(e.rows().size() * e.cols().size())]);
        read_text_tile_into(o.input, o.W, o.H, e.rows(), e.cols(), tile.get(), e.cols().size());
        parse_ms[r] = ms_since(a);
        const auto b = std::chrono::steady_clock::now();
        e.load_cells(tile.get(), e.cols().size());
        load_ms[r] = ms_since(b);
      }
      for (const Stamp& s : stamps) e.place(s.x, s.y, s.pat.w, s.pat.h, s.pat.cells.data(), Backend::kPlaceOr);
    });
    read_ms = ms_since(t0);
    const double read_parse_ms = *std::max_element(parse_ms.begin(), parse_ms.end());
    const double read_load_ms = *std::max_element(load_ms.begin(), load_ms.end());
    // Generation loop, in chunks of --checkpoint-every generations when
    // checkpointing (each chunk ends with every rank's tile on disk).
    std::vector<RunResult> results(P);
    RunResult total;
    const int64_t limit = o.gens;
    int64_t checkpoints_written = 0;
    // One density image of the current grid (every rank takes part; rank 0's copy is written).
    const auto write_density = [&](int64_t gen) {
      std::vector<std::vector<uint64_t>> maps(P);
      const auto a = std::chrono::steady_clock::now();
      par([&](int r) { maps[r] = engines[r]->density(o.density_bx, o.density_by); });
      density_ms = ms_since(a);
      ++density_frames;
      write_pgm(density_path(gen), density_image(maps[0].data(), o.density_by, o.density_bx, o.H, o.W).data(),
                ceil_div(o.W, o.density_bx), ceil_div(o.H, o.density_by));
    };
    if (o.cycle > 0) {
      // --cycle: Engine::find_cycle instead of the run loop; every rank takes
      // the same decisions and returns the same result.
      const int64_t gen0 = engines[0]->generation();
      std::vector<CycleResult> cycles(P);
      par([&](int r) { cycles[r] = engines[r]->find_cycle(limit, o.cycle); });
      cyc = cycles[0];
      for (auto& c : cycles) total.loop_ms = std::max(total.loop_ms, c.loop_ms);
      total.executed = cyc.generation - gen0;
      total.generations = cyc.generation;
      total.stop_reason = cyc.stop_reason;
      total.extinct = cyc.stop_reason == "extinction";
      total.fingerprint = cyc.fingerprint;
    }
    // With --checkpoint-every and --density-every a chunk ends at the next
    // checkpoint or the next multiple of K, whichever comes first.
    int64_t next_checkpoint = o.checkpoint_every > 0 ? engines[0]->generation() + o.checkpoint_every : -1;
    for (; o.cycle == 0;) {
      const int64_t gen = engines[0]->generation();
      int64_t target = limit;
      if (next_checkpoint >= 0) target = std::min(target, next_checkpoint);
      if (o.density_every > 0) target = std::min(target, (gen / o.density_every + 1) * o.density_every);
      par([&](int r) { results[r] = engines[r]->run_until(target); });
      double ms = 0;
      for (auto& rr : results) ms = std::max(ms, rr.loop_ms);
      total.loop_ms += ms;
      total.executed += results[0].executed;
      total.exchanges += results[0].exchanges;
      total.polls += results[0].polls;
      total.kernel_launches += results[0].kernel_launches;
      // The chunks' series concatenate to the whole run's (every rank holds the global sum).
      total.population.insert(total.population.end(), results[0].population.begin(), results[0].population.end());
      total.fingerprint.insert(total.fingerprint.end(), results[0].fingerprint.begin(), results[0].fingerprint.end());
      // Per-phase device times: the slowest rank's, like loop_ms.
      for (auto& rr : results) {
        total.phase_timed = total.phase_timed || rr.phase_timed;
      }
      const RunResult* slow = &results[0];
      for (auto& rr : results)
        if (rr.loop_ms > slow->loop_ms) slow = &rr;
      total.compute_ms += slow->compute_ms;
      total.halo_ms += slow->halo_ms;
      total.fill_ms += slow->fill_ms;
      total.allreduce_ms += slow->allreduce_ms;
      const RunResult& last = results[0];
      if (last.first_unchanged >= 0 || engines[0]->generation() >= limit) {
        total.first_unchanged = last.first_unchanged;
        total.extinct = last.extinct;
        total.generations = reported_generations(last.first_unchanged, last.extinct, limit, o.start_gen,
                                                 o.similarity, o.sim_freq, o.sim_phase, &total.stop_reason);
        break;
      }
      if (o.density_every > 0 && engines[0]->generation() % o.density_every == 0)
        write_density(engines[0]->generation());
      const bool checkpoint_due = engines[0]->generation() == next_checkpoint;
      if (checkpoint_due) next_checkpoint += o.checkpoint_every;
      if (checkpoint_due && !o.checkpoint_dir.empty()) {
        const int64_t g = engines[0]->generation();
        const std::string grid_path = checkpoint_begin(o.checkpoint_dir, o.W, o.H, g);
        par([&](int r) {
          Engine& e = *engines[r];
          std::vector<uint8_t> tile(size_t(e.rows().size() * e.cols().size()));
          e.store_cells(tile.data(), e.cols().size(), false);
          write_text_tile(grid_path, o.W, o.H, e.rows(), e.cols(), tile.data(),
                          e.cols().size());
        });
        CheckpointMeta m;
        m.W = o.W;
        m.H = o.H;
        m.generation = g;
        m.sim_phase = sim_phase_at(g, o.start_gen, o.sim_phase, o.sim_freq);
        m.gen_limit = limit;
        m.check_similarity = o.similarity;
        m.sim_freq = o.sim_freq;
        m.layout = layout_name(layout);
        m.rule = rule_string(o.rule);
        m.boundary = boundary_name(o.boundary);
        m.census = o.census_on;
        m.fingerprint = o.fprint_on;
        // Fault injection (tests): die after the N-th checkpoint's tiles are
        // written, before it is committed.
        if (const int c = o.tune.i("fault_checkpoint_crash"))
          if (++checkpoints_written == c) std::_Exit(86);
        checkpoint_commit(o.checkpoint_dir, grid_path, m);
      }
    }
    res = total;
    if (!o.density_file.empty()) write_density(res.generations);
    for (const Options::Window& w : o.windows) {
      std::vector<std::vector<uint8_t>> cells(P, std::vector<uint8_t>(size_t(w.w * w.h)));
      par([&](int r) { engines[r]->store_window(w.x, w.y, w.w, w.h, cells[r].data(), false); });
      write_window(w, cells[0], o.rule);
    }

    std::vector<double> store_ms(P, 0.0), format_ms(P, 0.0);
    if (want_grid) {
      auto t1 = std::chrono::steady_clock::now();
      if (o.output != "none") create_text_file(o.output, o.W, o.H);
      if (o.show) final_grid.assign(size_t(o.W * o.H), 0);
      par([&](int r) {
        Engine& e = *engines[r];
        const auto a = std::chrono::steady_clock::now();
        std::unique_ptr<uint8_t[]> tile(new uint8_t[size_t(e.rows().size() * e.cols().size())]);
        e.store_cells(tile.get(), e.cols().size(), false);
        store_ms[r] = ms_since(a);
        const auto b = std::chrono::steady_clock::now();
        if (o.output != "none")
          write_text_tile(o.output, o.W, o.H, e.rows(), e.cols(), tile.get(), e.cols().size());
        format_ms[r] = ms_since(b);
        if (o.show)
          for (int64_t i = 0; i < e.rows().size(); ++i)
            std::memcpy(&final_grid[size_t((e.rows().begin + i) * o.W + e.cols().begin)],
                        &tile[size_t(i * e.cols().size())], size_t(e.cols().size()));
      });
      write_ms = ms_since(t1);
    }
    if (!o.metrics.empty()) {
      std::ofstream f(o.metrics);
      double cups = res.loop_ms > 0 ? double(o.W) * double(o.H) * double(res.executed) / (res.loop_ms * 1e-3) : 0;
      std::string tuning_changed = "{";
      for (const auto& kv : o.tune.changed())
        tuning_changed += (tuning_changed.size() > 1 ? ", " : "") + jstr(kv.first) + ": " + jstr(kv.second);
      tuning_changed += "}";
      f << "{\"engine\": " << jstr(engine) << ", \"backend\": " << jstr(backends[0]->name())
        << ", \"layout\": " << jstr(layout_name(layout)) << ", \"rule\": " << jstr(rule_string(o.rule))
        << ", \"boundary\": " << jstr(boundary_name(o.boundary))
        << ", \"ranks\": " << P
        << ", \"decomp\": " << jstr(engines[0]->decomp().describe()) << ", \"tuning\": " << jstr(o.tune.summary())
        << ", \"tuning_changed\": " << tuning_changed << ", \"W\": " << o.W
        << ", \"H\": " << o.H << ", \"generations\": " << res.generations
        << ", \"executed\": " << res.executed << ", \"stop_reason\": " << jstr(res.stop_reason)
        << ", \"loop_ms\": " << res.loop_ms << ", \"read_ms\": " << read_ms
        << ", \"read_parse_ms\": " << read_parse_ms << ", \"read_load_ms\": " << read_load_ms
        << ", \"write_ms\": " << write_ms
        << ", \"write_store_ms\": " << *std::max_element(store_ms.begin(), store_ms.end())
        << ", \"write_format_ms\": " << *std::max_element(format_ms.begin(), format_ms.end())
        << ", \"file_bytes\": " << o.H * (o.W + 1) << ", \"cell_updates_per_s\": " << cups
        << ", \"epoch\": " << engines[0]->epoch_depth() << ", \"tmax\": " << engines[0]->tmax()
        << ", \"exchanges\": " << res.exchanges << ", \"polls\": " << res.polls
        << ", \"kernel_launches\": " << res.kernel_launches << ", \"comm\": " << jstr(P > 1 ? comm : "self")
        << ", \"overlap_mode\": " << jstr(engines[0]->overlap_mode())
        << ", \"overlap_trial_ms_plain\": " << engines[0]->trial_ms_plain()
        << ", \"overlap_trial_ms_trigger\": " << engines[0]->trial_ms_trigger()
        << ", \"phase_timed\": " << (res.phase_timed ? "true" : "false") << ", \"compute_ms\": " << res.compute_ms
        << ", \"halo_ms\": " << res.halo_ms << ", \"fill_ms\": " << res.fill_ms
        << ", \"allreduce_ms\": " << res.allreduce_ms;
      if (!o.density_file.empty())
        f << ", \"density_block\": " << jstr(std::to_string(o.density_by) + "x" + std::to_string(o.density_bx))
          << ", \"density_ms\": " << density_ms << ", \"density_frames\": " << density_frames;
      if (o.census_on) {
        f << ", \"census\": true, \"population\": [";
        for (size_t i = 0; i < res.population.size(); ++i) f << (i ? ", " : "") << res.population[i];
        f << "]";
      }
      if (o.fprint_on) {
        f << ", \"fingerprint\": true, \"fingerprints\": [";
        for (size_t i = 0; i < res.fingerprint.size(); ++i) f << (i ? ", " : "") << jstr(hex16(res.fingerprint[i]));
        f << "]";
      }
      if (o.cycle > 0)
        f << ", \"cycle\": {\"period\": " << cyc.period << ", \"generation\": " << cyc.generation
          << ", \"repeats_from\": " << cyc.repeats_from << ", \"confirmations\": " << cyc.confirmations
          << ", \"false_candidates\": " << cyc.false_candidates << ", \"stop_reason\": " << jstr(cyc.stop_reason)
          << ", \"max_period\": " << o.cycle << "}";
      f << "}\n";
    }
  }
  // --fingerprint PATH: generation,fingerprint lines (16 hex digits), one per generation of the run.
  if (!o.fprint.empty()) {
    std::ofstream f(o.fprint);
    GOL_REQUIRE(f.good(), "--fingerprint: cannot write '" + o.fprint + "'");
    for (size_t i = 0; i < res.fingerprint.size(); ++i)
      f << o.start_gen + 1 + int64_t(i) << "," << hex16(res.fingerprint[i]) << "\n";
  }
  // --census PATH: generation,population lines, one per generation of the run.
  if (!o.census.empty()) {
    std::ofstream f(o.census);
    GOL_REQUIRE(f.good(), "--census: cannot write '" + o.census + "'");
    for (size_t i = 0; i < res.population.size(); ++i)
      f << o.start_gen + 1 + int64_t(i) << "," << res.population[i] << "\n";
  }

  // stdout contract of the matching reference build.
  if (o.style == "mpi" || o.style == "async" || o.style == "collective" || o.style == "openmp") {
    std::printf("Reading file:\t%.2lf msecs\n", read_ms);
    std::printf("Generations:\t%d\n", int(res.generations));
    std::printf("Execution time:\t%.2lf msecs\n", res.loop_ms);
    std::printf("Writing file:\t%.2lf msecs\n", write_ms);
    if (o.style != "openmp")  // every MPI process prints it (src/game_mpi.c:514)
      for (int r = 0; r < std::max(1, o.ranks); ++r) std::printf("Finished\n");
  } else if (o.style == "cuda") {
    std::printf("Generations:\t%d\n", int(res.generations));
    std::printf("Execution time:\t%.2f msecs\n", res.loop_ms);
    std::printf("Finished\n");
  } else {
    std::printf("Finished.\n\n");
    std::printf("Generations:\t%d\n", int(res.generations));
    std::printf("Execution time:\t%.2f msecs\n", res.loop_ms);
    std::printf("Finished\n");
  }
  // --cycle: one extra line after the usual output.  Period and generation are
  // confirmed on the cells; "repeat from" is fingerprint evidence.
  if (o.cycle > 0) {
    if (cyc.period > 0)
      std::printf("Cycle: period %lld at generation %lld (fingerprints repeat from %lld)\n", (long long)cyc.period,
                  (long long)cyc.generation, (long long)cyc.repeats_from);
    else
      std::printf("Cycle: none within %lld generations\n", (long long)o.gens);
  }
  std::fflush(stdout);
  if (o.show && !final_grid.empty()) show(final_grid, o.W, o.H);
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  try {
    return run(parse(argc, argv));
  } catch (const std::exception& e) {
    std::fprintf(stderr, "gol: error: %s\n", e.what());
    return 1;
  }
}
