// The cluster census on the host (gol/batch.hpp has the definition): a plain
// flood fill over each universe's packed rows on the host pool, the exclusive
// scan every engine shares, the signature of a single pattern, the table of
// names and the aggregation into kinds.  It is the oracle of the HIP kernel
// (life_batch_clusters.hip).
#include "gol/batch.hpp"

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <map>
#include <memory>
#include <mutex>
#include <tuple>
#include <unordered_map>

#include "gol/fingerprint.hpp"
#include "gol/parallel.hpp"

namespace gol {

int64_t cluster_offsets(const std::vector<int32_t>& counts, std::vector<int32_t>& offsets) {
  offsets.resize(counts.size());
  int64_t total = 0;
  for (size_t u = 0; u < counts.size(); ++u) {
    offsets[u] = int32_t(std::min(total, kClusterRecordsMax));
    total += counts[u];
  }
  if (total > kClusterRecordsMax)
    fail("batch: the cluster census holds " + std::to_string(total) + " records: a call holds at most 2^28 = " +
         std::to_string(kClusterRecordsMax) + " (run fewer universes per call)");
  return total;
}

namespace {

void check_shape(int W, int H, int64_t B) {
  BatchConfig cfg;
  cfg.W = W;
  cfg.H = H;
  BatchInput in;
  in.B = B;
  validate_batch(cfg, in);
}

// The records of universes [b0, b1) in order; `clusters` is shared.
struct Chunk {
  int64_t b0 = 0;
  std::vector<int32_t> universe, cells;
  std::vector<uint64_t> signature;
  std::vector<int16_t> height, width;
  std::vector<uint8_t> spanning;
};

int32_t universe_clusters(const uint64_t* rows, int W, int H, bool torus, int32_t u, Chunk& out) {
  uint64_t rest[64], comp[64];
  for (int y = 0; y < H; ++y) rest[y] = rows[y];
  std::vector<uint16_t> stack;  // y << 8 | x
  stack.reserve(size_t(W) * H);
  int32_t n = 0;
  for (int y = 0; y < H; ++y) {
    while (rest[y]) {
      for (int r = 0; r < H; ++r) comp[r] = 0;
      const int x = __builtin_ctzll(rest[y]);
      rest[y] &= ~(uint64_t(1) << x);
      comp[y] |= uint64_t(1) << x;
      stack.push_back(uint16_t(y << 8 | x));
      while (!stack.empty()) {
        const int cy = stack.back() >> 8, cx = stack.back() & 0xFF;
        stack.pop_back();
        for (int dy = -2; dy <= 2; ++dy)
          for (int dx = -2; dx <= 2; ++dx) {
            int ny = cy + dy, nx = cx + dx;
            if (torus) {
              ny = (ny + H) % H, nx = (nx + W) % W;
            } else if (ny < 0 || ny >= H || nx < 0 || nx >= W) {
              continue;
            }
            const uint64_t bit = uint64_t(1) << nx;
            if (rest[ny] & bit) {
              rest[ny] &= ~bit;
              comp[ny] |= bit;
              stack.push_back(uint16_t(ny << 8 | nx));
            }
          }
      }
      uint64_t row_mask = 0, col_mask = 0;
      int32_t cells = 0;
      for (int r = 0; r < H; ++r) {
        if (comp[r]) row_mask |= uint64_t(1) << r;
        col_mask |= comp[r];
        cells += __builtin_popcountll(comp[r]);
      }
      const ClusterAxis ay = cluster_axis(row_mask, H, torus), ax = cluster_axis(col_mask, W, torus);
      uint64_t sig = 0;
      for (int r = 0; r < H; ++r) {
        if (!comp[r]) continue;
        const uint64_t v = rotl_bits(comp[r], (W - ax.origin) % W, W);
        const uint64_t row = uint64_t(uint32_t(v)) * fingerprint_col_key(0) + (v >> 32) * fingerprint_col_key(1);
        sig += row * uint64_t(fingerprint_row_key(uint32_t((r - ay.origin + H) % H)));
      }
      out.universe.push_back(u);
      out.signature.push_back(sig);
      out.cells.push_back(cells);
      out.height.push_back(int16_t(ay.extent));
      out.width.push_back(int16_t(ax.extent));
      out.spanning.push_back(uint8_t((ax.spans ? kSpansX : 0) | (ay.spans ? kSpansY : 0)));
      ++n;
    }
  }
  return n;
}

}  // namespace

ClusterCensus find_clusters_rows(int threads, int W, int H, Boundary boundary, int64_t B, const uint64_t* rows) {
  check_shape(W, H, B);
  const bool torus = boundary == Boundary::Torus;
  ClusterCensus res;
  res.clusters.assign(size_t(B), 0);
  std::vector<std::unique_ptr<Chunk>> chunks;
  std::mutex mu;
  const auto body = [&](int64_t b0, int64_t b1) {
    auto ch = std::make_unique<Chunk>();
    ch->b0 = b0;
    for (int64_t b = b0; b < b1; ++b)
      res.clusters[size_t(b)] = universe_clusters(rows + b * H, W, H, torus, int32_t(b), *ch);
    std::lock_guard<std::mutex> lock(mu);
    chunks.push_back(std::move(ch));
  };
  const auto t0 = std::chrono::steady_clock::now();
  if (threads > 0) {
    ThreadPool pool(threads);
    pool.parallel_for(B, body);
  } else {
    global_pool().parallel_for(B, body);
  }
  std::vector<int32_t> offsets;
  const int64_t total = cluster_offsets(res.clusters, offsets);
  std::sort(chunks.begin(), chunks.end(), [](const auto& a, const auto& b) { return a->b0 < b->b0; });
  res.universe.reserve(size_t(total));
  res.signature.reserve(size_t(total));
  res.cells.reserve(size_t(total));
  res.height.reserve(size_t(total));
  res.width.reserve(size_t(total));
  res.spanning.reserve(size_t(total));
  for (const auto& ch : chunks) {
    res.universe.insert(res.universe.end(), ch->universe.begin(), ch->universe.end());
    res.signature.insert(res.signature.end(), ch->signature.begin(), ch->signature.end());
    res.cells.insert(res.cells.end(), ch->cells.begin(), ch->cells.end());
    res.height.insert(res.height.end(), ch->height.begin(), ch->height.end());
    res.width.insert(res.width.end(), ch->width.begin(), ch->width.end());
    res.spanning.insert(res.spanning.end(), ch->spanning.begin(), ch->spanning.end());
  }
  res.ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return res;
}

ClusterCensus find_clusters_cpu(int threads, int W, int H, Boundary boundary, int64_t B, const uint8_t* cells) {
  check_shape(W, H, B);
  std::vector<uint64_t> rows(size_t(B) * H);
  for (size_t r = 0; r < rows.size(); ++r) {
    uint64_t v = 0;
    for (int x = 0; x < W; ++x) {
      const uint8_t c = cells[r * size_t(W) + x];
      if (c > 1)
        fail("batch: cell " + std::to_string(x) + " of row " + std::to_string(r % H) + " of universe " +
             std::to_string(r / H) + " is " + std::to_string(c) + ": the input holds 0 (dead) and 1 (live) only");
      v |= uint64_t(c) << x;
    }
    rows[r] = v;
  }
  return find_clusters_rows(threads, W, H, boundary, B, rows.data());
}

uint64_t cluster_signature(const uint8_t* cells, int64_t w, int64_t h) {
  GOL_REQUIRE(w >= 1 && h >= 1, "cluster_signature: the array is empty");
  int64_t live = 0, first = -1;
  for (int64_t i = 0; i < w * h; ++i)
    if (cells[i]) {
      ++live;
      if (first < 0) first = i;
    }
  if (live == 0) fail("cluster_signature: the array holds no live cell, so no cluster");
  std::vector<uint8_t> seen(size_t(w * h), 0);
  std::vector<int64_t> stack{first};
  seen[size_t(first)] = 1;
  int64_t reached = 0, y0 = h, y1 = -1, x0 = w, x1 = -1;
  while (!stack.empty()) {
    const int64_t i = stack.back(), cy = i / w, cx = i % w;
    stack.pop_back();
    ++reached;
    y0 = std::min(y0, cy), y1 = std::max(y1, cy), x0 = std::min(x0, cx), x1 = std::max(x1, cx);
    for (int64_t ny = std::max<int64_t>(cy - 2, 0); ny <= std::min(cy + 2, h - 1); ++ny)
      for (int64_t nx = std::max<int64_t>(cx - 2, 0); nx <= std::min(cx + 2, w - 1); ++nx) {
        const int64_t j = ny * w + nx;
        if (cells[j] && !seen[size_t(j)]) {
          seen[size_t(j)] = 1;
          stack.push_back(j);
        }
      }
  }
  if (reached != live)
    fail("cluster_signature: the array holds more than one cluster (" + std::to_string(live - reached) + " of its " +
         std::to_string(live) + " live cells are further than 2 cells from the first one's cluster)");
  std::vector<uint8_t> box(size_t((y1 - y0 + 1) * (x1 - x0 + 1)));
  const int64_t bw = x1 - x0 + 1, bh = y1 - y0 + 1;
  for (int64_t y = 0; y < bh; ++y)
    for (int64_t x = 0; x < bw; ++x) box[size_t(y * bw + x)] = cells[(y0 + y) * w + x0 + x] ? 1 : 0;
  return grid_fingerprint(box.data(), bw, bw, bh);
}

namespace {

struct Named {
  const char* name;
  int period;
  std::vector<const char*> rows;
};

// Still lifes and oscillators of B3/S23 that soups leave, and the glider.
const std::vector<Named>& named_patterns() {
  static const std::vector<Named> p = {
      {"block", 1, {"OO", "OO"}},
      {"beehive", 1, {".OO.", "O..O", ".OO."}},
      {"loaf", 1, {".OO.", "O..O", ".O.O", "..O."}},
      {"boat", 1, {"OO.", "O.O", ".O."}},
      {"tub", 1, {".O.", "O.O", ".O."}},
      {"ship", 1, {"OO.", "O.O", ".OO"}},
      {"pond", 1, {".OO.", "O..O", "O..O", ".OO."}},
      {"barge", 1, {".O..", "O.O.", ".O.O", "..O."}},
      {"long boat", 1, {"OO..", "O.O.", ".O.O", "..O."}},
      {"mango", 1, {".OO..", "O..O.", ".O..O", "..OO."}},
      {"eater", 1, {"OO..", "O.O.", "..O.", "..OO"}},
      {"blinker", 2, {"OOO"}},
      {"toad", 2, {".OOO", "OOO."}},
      {"beacon", 2, {"OO..", "OO..", "..OO", "..OO"}},
      {"glider", 4, {".O.", "..O", "OOO"}},
      {"traffic light", 2, {"..OOO..", ".......", "O.....O", "O.....O", "O.....O", ".......", "..OOO.."}},
  };
  return p;
}

constexpr int kField = 32;  // the plane the named patterns evolve on

std::vector<uint8_t> life_step_plane(const std::vector<uint8_t>& g) {
  std::vector<uint8_t> out(g.size(), 0);
  for (int y = 0; y < kField; ++y)
    for (int x = 0; x < kField; ++x) {
      int n = 0;
      for (int dy = -1; dy <= 1; ++dy)
        for (int dx = -1; dx <= 1; ++dx) {
          const int yy = y + dy, xx = x + dx;
          if ((dy || dx) && yy >= 0 && yy < kField && xx >= 0 && xx < kField) n += g[size_t(yy * kField + xx)];
        }
      out[size_t(y * kField + x)] = uint8_t(n == 3 || (n == 2 && g[size_t(y * kField + x)]));
    }
  return out;
}

// Every phase of every named pattern in its 8 symmetric images; each image
// must be one cluster (cluster_signature fails otherwise).
const std::unordered_map<uint64_t, std::string>& name_table() {
  static const std::unordered_map<uint64_t, std::string> table = [] {
    std::unordered_map<uint64_t, std::string> t;
    for (const Named& p : named_patterns()) {
      std::vector<uint8_t> g(size_t(kField * kField), 0);
      for (size_t y = 0; y < p.rows.size(); ++y)
        for (size_t x = 0; p.rows[y][x]; ++x) g[(8 + y) * kField + 8 + x] = p.rows[y][x] == 'O';
      for (int phase = 0; phase < p.period; ++phase) {
        for (int image = 0; image < 8; ++image) {
          std::vector<uint8_t> im(g.size());
          for (int y = 0; y < kField; ++y)
            for (int x = 0; x < kField; ++x) {
              int sy = (image & 1) ? x : y, sx = (image & 1) ? y : x;
              if (image & 2) sy = kField - 1 - sy;
              if (image & 4) sx = kField - 1 - sx;
              im[size_t(y * kField + x)] = g[size_t(sy * kField + sx)];
            }
          const uint64_t sig = cluster_signature(im.data(), kField, kField);
          const auto it = t.emplace(sig, p.name).first;
          GOL_REQUIRE(it->second == p.name, std::string("cluster names: ") + p.name + " and " + it->second +
                                                " share a signature");
        }
        g = life_step_plane(g);
      }
    }
    return t;
  }();
  return table;
}

}  // namespace

std::string cluster_name(uint64_t signature) {
  const auto& t = name_table();
  const auto it = t.find(signature);
  if (it != t.end()) return it->second;
  char hex[17];
  std::snprintf(hex, sizeof hex, "%016llx", (unsigned long long)signature);
  return hex;
}

std::vector<ClusterKind> cluster_table(const ClusterCensus& c, const uint8_t* stop, unsigned stop_mask) {
  std::map<std::tuple<uint64_t, int32_t, int16_t, int16_t, uint8_t>, int64_t> kinds;
  for (size_t i = 0; i < c.size(); ++i) {
    if (stop && !((stop_mask >> stop[size_t(c.universe[i])]) & 1u)) continue;
    ++kinds[{c.signature[i], c.cells[i], c.height[i], c.width[i], c.spanning[i]}];
  }
  std::vector<ClusterKind> out;
  out.reserve(kinds.size());
  for (const auto& [k, n] : kinds)
    out.push_back({std::get<0>(k), std::get<1>(k), std::get<2>(k), std::get<3>(k), std::get<4>(k), n});
  // The map is in signature order: a stable sort keeps it among equal counts.
  std::stable_sort(out.begin(), out.end(), [](const ClusterKind& a, const ClusterKind& b) { return a.count > b.count; });
  return out;
}

}  // namespace gol
