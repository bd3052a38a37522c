// The grid fingerprint (EngineConfig::fingerprint, Engine::find_cycle): a
// position-dependent 64-bit value of a W x H grid, identical on every engine.
//
//   word(y, j): the 32 cells (y, 32j .. 32j + 31), cell 32j + b at bit b; cells
//   at x >= W are 0.
//   F = sum over y in [0, H), j in [0, ceil(W / 32)) of word(y, j) * r(y) * A(j)   (mod 2^64)
//   r(y) = fmix32(y) | 1      (32 bits, zero-extended; the murmur3 finaliser)
//   A(j) = splitmix64(j) | 1  (64 bits)
//
// y and j are global coordinates.  F is a sum, so it does not depend on the
// decomposition, the layout or the order of evaluation: ranks add their shares
// modulo 2^64.  Equal grids have equal fingerprints; unequal grids may collide,
// so nothing reports a repeat on fingerprints alone (Engine::find_cycle
// confirms on the cells).
#pragma once

#include <cstdint>

#include "gol/common.hpp"

namespace gol {

GOL_HD inline uint32_t fingerprint_row_key(uint32_t y) {
  uint32_t h = y;
  h ^= h >> 16;
  h *= 0x85EBCA6Bu;
  h ^= h >> 13;
  h *= 0xC2B2AE35u;
  h ^= h >> 16;
  return h | 1u;
}

GOL_HD inline uint64_t fingerprint_col_key(uint64_t j) {
  uint64_t x = j + 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return (x ^ (x >> 31)) | 1ull;
}

// Host implementation over H x W cells of bytes (non-zero and not '0': alive;
// ld: row stride).  row0 / word0: the global row of cells' row 0 and the global
// word of its column 0 (a tile's share; 0, 0 for a whole grid).
inline uint64_t grid_fingerprint(const uint8_t* cells, int64_t ld, int64_t W, int64_t H, int64_t row0 = 0,
                                 int64_t word0 = 0) {
  uint64_t f = 0;
  for (int64_t y = 0; y < H; ++y) {
    uint64_t row = 0;
    for (int64_t j = 0; 32 * j < W; ++j) {
      uint32_t w = 0;
      for (int64_t b = 0; b < 32 && 32 * j + b < W; ++b) {
        const uint8_t c = cells[y * ld + 32 * j + b];
        if (c != 0 && c != '0') w |= 1u << b;
      }
      row += uint64_t(w) * fingerprint_col_key(uint64_t(word0 + j));
    }
    f += row * uint64_t(fingerprint_row_key(uint32_t(row0 + y)));
  }
  return f;
}

}  // namespace gol
