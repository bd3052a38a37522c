// View kernels: a block-wise population count of a tile (the density map), a
// rectangle of cells read out of a tile, and a rectangle written into one.
//
// The reference can only print or write the whole grid (src/game.c:42-58,
// src/game_mpi_async.c:382-455).  Here a grid of 65536^2 cells and more is
// looked at through a map of block populations reduced on the device, and
// read or seeded through small windows, so the work is proportional to what
// is asked for: one streaming read for a map, the rectangle for a window.
#include <hip/hip_runtime.h>

#include "gol/backend.hpp"
#include "life_kernels.hpp"

namespace gol {
namespace hipk {
namespace {

constexpr int kBlock = 256;

// ---- density ----------------------------------------------------------------
// A work item is a piece of the tile: up to kPieceRows owned rows that lie in
// one global block row, by one chunk of kQuads quads.  A quad is four
// consecutive 32-cell words at a 4-word boundary of the padded row: in the bit
// layout one 16-byte load (a row pitch is a multiple of 256 bytes, so every
// quad of a row is 16-byte aligned and inside the row), in the byte layout
// eight of them.  A wave reads kQuads consecutive quads of one row (1 KiB of
// bit words), the workgroup's kBlock / kQuads waves take the piece's rows in
// turn.  A thread keeps its quad's column for the whole piece, so which global
// blocks its four words fall in is worked out once, and the counts stay in
// registers over the rows; they then go to the workgroup's bins in LDS (one
// per global block column the chunk meets), and each bin that is not zero is
// added to the output with one 64-bit atomic.  Words of the quad outside the
// owned words (halo columns next to the first and last owned word) are loaded
// with it and masked.
constexpr int kQuads = 64;
constexpr int kRowLanes = kBlock / kQuads;
constexpr int kChunkCells = kQuads * 128;
constexpr int kPieceRows = 128;
// Block columns a chunk can meet: one per cell (bx = 1); one per word where
// words are not cut.
constexpr int kBinsMax = kChunkCells, kBinsAligned = kQuads * 4;

struct DensityParams {
  const uint8_t* buf;
  int64_t pitch, row0;        // bytes per padded row, padded row of owned row 0
  int64_t H, W, nw;           // owned rows, owned cells, owned words
  int64_t hw;                 // padded word of owned word 0
  int64_t grow0, gcol0;       // global row and cell of the first owned row and cell
  int64_t bx, by, nbx;        // block size, global blocks per row of the map
  int64_t sub, ph;            // pieces per global block row, rows per piece
  int64_t piece0;             // global number of the tile's first piece
  int64_t npieces, nchunks;
  unsigned long long* out;
};

__host__ __device__ __forceinline__ int64_t imin(int64_t a, int64_t b) { return a < b ? a : b; }
__host__ __device__ __forceinline__ int64_t imax(int64_t a, int64_t b) { return a > b ? a : b; }

__device__ __forceinline__ uint32_t nibble_of(uint32_t v) {
  v = ((v & 0x7f7f7f7fu) + 0x7f7f7f7fu) | v;  // any nonzero byte -> top bit set
  return (((v >> 7) & 0x01010101u) * 0x01020408u) >> 24;
}
__device__ __forceinline__ uint32_t pack8(uint4 a, uint4 b) {
  return nibble_of(a.x) | nibble_of(a.y) << 4 | nibble_of(a.z) << 8 | nibble_of(a.w) << 12 | nibble_of(b.x) << 16 |
         nibble_of(b.y) << 20 | nibble_of(b.z) << 24 | nibble_of(b.w) << 28;
}
// Bits [lo, hi) of a word, 0 <= lo <= hi <= 32.
__device__ __forceinline__ uint32_t bit_range(int lo, int hi) {
  const uint32_t up = hi >= 32 ? 0xffffffffu : (1u << hi) - 1u;
  return up & ~((1u << lo) - 1u);  // lo < 32 wherever a range is not empty
}

// The four words of padded quad q of a row as cell bits.  `valid`: cells of
// each word that are owned (0: the word is not loaded in the byte layout).
template <Layout L>
__device__ __forceinline__ void load_quad(const uint8_t* row, int64_t q, const int valid[4], uint32_t w[4]) {
  if constexpr (L == Layout::Bits) {
    const uint4 v = *reinterpret_cast<const uint4*>(row + 16 * q);
    w[0] = v.x, w[1] = v.y, w[2] = v.z, w[3] = v.w;
  } else {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      w[u] = 0;
      if (valid[u]) {
        const uint4* p = reinterpret_cast<const uint4*>(row + 32 * (4 * q + u));
        w[u] = pack8(p[0], p[1]);
      }
    }
  }
}

// Aligned: every owned word lies in one block column (bx % 32 == 0 and the
// tile starts on a global word), whole-word popcounts.  Otherwise a word is
// cut at the block columns' edges: up to two parts are masked and counted in
// registers like whole words; a word cut into more (bx < 32) adds its parts to
// the bins row by row.
template <Layout L, bool Aligned>
__global__ __launch_bounds__(kBlock) void density_k(DensityParams p) {
  __shared__ uint32_t bins[Aligned ? kBinsAligned : kBinsMax];
  const int lane = threadIdx.x % kQuads, rl = threadIdx.x / kQuads;
  const int64_t items = p.npieces * p.nchunks;
  for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
    const int64_t pi = item / p.nchunks, ch = item - pi * p.nchunks;
    // The piece's rows, clipped to the tile (owned row numbers).
    const int64_t P = p.piece0 + pi, bi = P / p.sub, s = P - bi * p.sub;
    const int64_t g_lo = bi * p.by + s * p.ph, g_hi = imin(g_lo + p.ph, (bi + 1) * p.by);
    const int64_t ra = imax(g_lo, p.grow0) - p.grow0, rb = imin(g_hi, p.grow0 + p.H) - p.grow0;
    if (ra >= rb) continue;  // the same for the whole workgroup
    // The chunk's owned cells and the block columns they meet.
    const int64_t q0 = p.hw / 4 + ch * kQuads;
    const int64_t c_lo = imax(0, (4 * q0 - p.hw) * 32), c_hi = imin(p.W, (4 * (q0 + kQuads) - p.hw) * 32);
    const int64_t j0 = (p.gcol0 + c_lo) / p.bx;
    const int nb = int((p.gcol0 + c_hi - 1) / p.bx - j0) + 1;
    for (int b = threadIdx.x; b < nb; b += kBlock) bins[b] = 0;
    __syncthreads();

    // This thread's quad: owned cells, parts and bins of its four words.  One
    // division per thread: with bx >= 32 the block column of a word is that of
    // the word before it, or the next one.
    const int64_t q = q0 + lane;
    int valid[4], bin[4][2];
    uint32_t mask[4][2];
    bool many[4];
    const int64_t k_first = imax(0, 4 * q - p.hw);
    int64_t j = (p.gcol0 + 32 * k_first) / p.bx;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int64_t k = 4 * q + u - p.hw;
      valid[u] = (k < 0 || k >= p.nw) ? 0 : int(imin(32, p.W - 32 * k));
      const int64_t gc = p.gcol0 + 32 * k;
      bin[u][0] = bin[u][1] = 0;
      mask[u][0] = mask[u][1] = 0;
      many[u] = false;
      if (valid[u] == 0) continue;
      if (p.bx >= 32) {
        if ((j + 1) * p.bx <= gc) ++j;
      } else {
        j = gc / p.bx;
      }
      bin[u][0] = int(j - j0);
      if constexpr (Aligned) {
        mask[u][0] = 0xffffffffu;
      } else {
        const int e0 = int(imin(valid[u], (j + 1) * p.bx - gc));
        mask[u][0] = bit_range(0, e0);
        if (e0 < valid[u]) {
          const int e1 = int(imin(valid[u], e0 + p.bx));
          bin[u][1] = bin[u][0] + 1;
          mask[u][1] = bit_range(e0, e1);
          many[u] = e1 < valid[u];
        }
      }
    }

    uint32_t acc[4][2] = {{0, 0}, {0, 0}, {0, 0}, {0, 0}};
    const uint8_t* base = p.buf + (p.row0 + ra + rl) * p.pitch;
    // A quad past the last owned word may lie outside the row: not loaded.
    const int64_t r_end = (valid[0] | valid[1] | valid[2] | valid[3]) ? rb : 0;
#pragma unroll 4
    for (int64_t r = ra + rl; r < r_end; r += kRowLanes, base += kRowLanes * p.pitch) {
      uint32_t w[4];
      load_quad<L>(base, q, valid, w);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if constexpr (Aligned) {
          acc[u][0] += __popc(w[u] & mask[u][0]);
        } else if (!many[u]) {
          acc[u][0] += __popc(w[u] & mask[u][0]);
          acc[u][1] += __popc(w[u] & mask[u][1]);
        } else {
          // bx < 32: every part of the word to its bin.
          const int64_t gc = p.gcol0 + 32 * (4 * q + u - p.hw);
          int b = 0;
          for (int64_t jj = j0 + bin[u][0]; b < valid[u]; ++jj) {
            const int e = int(imin(valid[u], (jj + 1) * p.bx - gc));
            const uint32_t n = __popc(w[u] & bit_range(b, e));
            if (n) atomicAdd(&bins[jj - j0], n);
            b = e;
          }
        }
      }
    }
    // Registers -> bins: neighbouring parts of one bin are summed first.
    int cur = -1;
    uint32_t sum = 0;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
#pragma unroll
      for (int h = 0; h < (Aligned ? 1 : 2); ++h) {
        if (mask[u][h] == 0 || many[u]) continue;
        if (bin[u][h] != cur) {
          if (sum) atomicAdd(&bins[cur], sum);
          cur = bin[u][h];
          sum = 0;
        }
        sum += acc[u][h];
      }
    }
    if (sum) atomicAdd(&bins[cur], sum);
    __syncthreads();
    // Bins -> the map: one atomic per block the workgroup met.  The thread
    // that reads bin b is the one that zeroes it for the next item.
    for (int b = threadIdx.x; b < nb; b += kBlock) {
      const uint32_t v = bins[b];
      if (v) atomicAdd(p.out + bi * p.nbx + j0 + b, static_cast<unsigned long long>(v));
    }
  }
}

// ---- windows ------------------------------------------------------------------
// hh x ww cells whose first one is padded row `first_row`, padded cell `c0` of
// the tile, into or from a dense stage of hh x ww bytes.
__global__ void store_window_k(const uint8_t* buf, int64_t pitch, int64_t first_row, int64_t c0, int64_t ww, int64_t hh,
                               bool bits, uint8_t* stage, uint8_t base) {
  const int64_t total = hh * ww;
  for (int64_t t = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; t < total; t += int64_t(gridDim.x) * blockDim.x) {
    const int64_t i = t / ww, x = t - i * ww;
    const uint8_t* row = buf + (first_row + i) * pitch;
    const int64_t cell = c0 + x;
    const uint8_t v = bits ? uint8_t((reinterpret_cast<const uint32_t*>(row)[cell / 32] >> (cell % 32)) & 1u)
                           : uint8_t(row[cell] != 0);
    stage[t] = uint8_t(base + v);
  }
}

// One thread owns each destination word of each row: the words [wa, wa + nwr)
// that hold cells [c0, c0 + ww), the first and last of them in part.
__global__ void place_window_bits(uint32_t* buf, int64_t pitch_w, int64_t first_row, int64_t c0, int64_t ww, int64_t hh,
                                  int64_t wa, int64_t nwr, const uint8_t* stage, bool copy) {
  const int64_t total = hh * nwr;
  for (int64_t t = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; t < total; t += int64_t(gridDim.x) * blockDim.x) {
    const int64_t i = t / nwr, k = wa + (t - i * nwr);
    const int64_t x0 = 32 * k - c0;  // window column of the word's bit 0
    const int lo = int(imax(0, -x0)), hi = int(imin(32, ww - x0));
    const uint8_t* s = stage + i * ww + x0;
    uint32_t m = 0, v = 0;
    for (int b = lo; b < hi; ++b) {
      m |= 1u << b;
      v |= uint32_t(s[b] == 1 || s[b] == '1') << b;
    }
    uint32_t* word = buf + (first_row + i) * pitch_w + k;
    *word = copy ? ((*word & ~m) | v) : (*word | v);
  }
}

__global__ void place_window_u8(uint8_t* buf, int64_t pitch, int64_t first_row, int64_t c0, int64_t ww, int64_t hh,
                                const uint8_t* stage, bool copy) {
  const int64_t total = hh * ww;
  for (int64_t t = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; t < total; t += int64_t(gridDim.x) * blockDim.x) {
    const int64_t i = t / ww, x = t - i * ww;
    const uint8_t v = uint8_t(stage[t] == 1 || stage[t] == '1');
    uint8_t* cell = buf + (first_row + i) * pitch + c0 + x;
    if (copy || v) *cell = v;
  }
}

inline unsigned grid_for(int64_t n) {
  return unsigned(std::max<int64_t>(1, std::min<int64_t>(ceil_div(n, kBlock), 256 * 8 * 4)));
}

void require_window(const TileGeom& g, int64_t r0, int64_t c0, int64_t ww, int64_t hh, const char* what) {
  GOL_REQUIRE(ww > 0 && hh > 0 && r0 >= 0 && c0 >= 0 && r0 + hh <= g.H && c0 + ww <= g.W,
              std::string(what) + ": the rectangle leaves the tile's owned cells");
}

}  // namespace

void launch_density(const uint8_t* buf, const TileGeom& g, int64_t global_row0, int64_t global_col0, int64_t grid_h,
                    int64_t grid_w, int64_t bx, int64_t by, unsigned long long* out, hipStream_t s) {
  GOL_REQUIRE(bx >= 1 && by >= 1, "density: block sizes must be at least 1");
  GOL_REQUIRE(global_row0 >= 0 && global_col0 >= 0 && global_row0 + g.H <= grid_h && global_col0 + g.W <= grid_w,
              "density: the tile leaves the grid");
  const int64_t nbx = ceil_div(grid_w, bx), nby = ceil_div(grid_h, by);
  GOL_REQUIRE(nbx <= Backend::kDensityBlocksMax && nby <= Backend::kDensityBlocksMax &&
                  nbx * nby <= Backend::kDensityBlocksMax,
              "density: more than 2^24 blocks");
  GOL_REQUIRE(g.pitch % 16 == 0 && g.pitch >= (g.layout == Layout::Bits ? 4 : 32) * g.Wp(),
              "density: a row pitch must hold whole 16-byte quads");
  DensityParams p;
  p.buf = buf;
  p.pitch = g.pitch, p.row0 = g.row0();
  p.H = g.H, p.W = g.W, p.nw = ceil_div(g.W, 32), p.hw = g.hw;
  p.grow0 = global_row0, p.gcol0 = global_col0;
  p.bx = bx, p.by = by, p.nbx = nbx;
  p.sub = ceil_div(by, kPieceRows), p.ph = ceil_div(by, p.sub);
  const auto piece_of = [&](int64_t grow) {
    const int64_t i = grow / by;
    return i * p.sub + (grow - i * by) / p.ph;
  };
  p.piece0 = piece_of(global_row0);
  p.npieces = piece_of(global_row0 + g.H - 1) - p.piece0 + 1;
  p.nchunks = ceil_div((g.hw + p.nw - 1) / 4 - g.hw / 4 + 1, kQuads);
  p.out = out;
  const unsigned grid = unsigned(std::min<int64_t>(p.npieces * p.nchunks, int64_t(1) << 20));
  const bool aligned = g.layout == Layout::Bits && bx % 32 == 0 && global_col0 % 32 == 0;
  if (g.layout == Layout::Bits) {
    if (aligned)
      hipLaunchKernelGGL((density_k<Layout::Bits, true>), dim3(grid), dim3(kBlock), 0, s, p);
    else
      hipLaunchKernelGGL((density_k<Layout::Bits, false>), dim3(grid), dim3(kBlock), 0, s, p);
  } else {
    hipLaunchKernelGGL((density_k<Layout::U8, false>), dim3(grid), dim3(kBlock), 0, s, p);
  }
}

void launch_store_window(const uint8_t* buf, const TileGeom& g, int64_t r0, int64_t c0, int64_t ww, int64_t hh,
                         uint8_t* stage, bool ascii, hipStream_t s) {
  require_window(g, r0, c0, ww, hh, "store_window");
  hipLaunchKernelGGL(store_window_k, dim3(grid_for(hh * ww)), dim3(kBlock), 0, s, buf, g.pitch, g.row0() + r0,
                     g.cell0() + c0, ww, hh, g.layout == Layout::Bits, stage, uint8_t(ascii ? '0' : 0));
}

void launch_place_window(uint8_t* buf, const TileGeom& g, int64_t r0, int64_t c0, int64_t ww, int64_t hh,
                         const uint8_t* stage, bool copy, hipStream_t s) {
  require_window(g, r0, c0, ww, hh, "place_window");
  const int64_t pc0 = g.cell0() + c0;
  if (g.layout == Layout::Bits) {
    const int64_t wa = pc0 / 32, nwr = (pc0 + ww - 1) / 32 - wa + 1;
    hipLaunchKernelGGL(place_window_bits, dim3(grid_for(hh * nwr)), dim3(kBlock), 0, s,
                       reinterpret_cast<uint32_t*>(buf), g.pitch / 4, g.row0() + r0, pc0, ww, hh, wa, nwr, stage, copy);
  } else {
    hipLaunchKernelGGL(place_window_u8, dim3(grid_for(hh * ww)), dim3(kBlock), 0, s, buf, g.pitch, g.row0() + r0, pc0,
                       ww, hh, stage, copy);
  }
}

}  // namespace hipk
}  // namespace gol
