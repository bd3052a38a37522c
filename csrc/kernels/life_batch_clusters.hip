// life_batch_clusters: the cluster census of many small universes, each one in
// the registers of (a part of) one wave (gol/batch.hpp has the definition).
//
// The lane mapping is that of life_batch_kernel (life_batch.hip): one row per
// lane, W/32 words per lane, 64/H universes per wave, a partial last wave
// masked off.  Per universe, with every loop wave-uniform on a ballot and the
// universes of a wave predicated by their ballot mask `mine`:
//   * rest starts as the universe's live words.  While any universe of the
//     wave has cells left, comp is seeded with one bit: the lowest lane of the
//     universe whose rest is non-zero, the lowest set bit of its words - the
//     smallest cell in row-major order, so clusters come out in their order.
//   * comp = dilate2(comp) & rest until no lane of the universe changes.
//     comp never shrinks, so a universe that has converged keeps its comp
//     while the others of its wave go on.  dilate2 ORs the funnel shifts by
//     1 and 2 cells to both sides (a rotate on the torus, zero fill on the
//     plane), then that moved by 1 and 2 rows up and down (a 2-row move is two
//     vmoves).  On the plane what arrives across the universe's edge is masked
//     at both distances.
//   * Measuring: population by popcount and a cross-lane sum, the row mask
//     from the ballot, the column mask from an OR over the lanes, origin and
//     extent by cluster_axis, the signature from the lane's words rotated by
//     the column origin times the keys of grid_fingerprint, summed over the
//     lanes modulo 2^64.
//   * Lane row 0 writes the record, then rest &= ~comp.
// No LDS beyond what ds_bpermute needs, no atomics, no barriers and no memory
// traffic in the loops.
//
// Storage is exact: the kernel runs twice.  The count pass (EMIT = false)
// writes the number of clusters of every universe, the host scans them, the
// emit pass writes record offsets[u] + i of universe u.  A record is 16 bytes
// on the device: the signature, and (cells, height | width << 8 | spanning << 16).
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "gol/backend.hpp"
#include "gol/batch.hpp"
#include "gol/fingerprint.hpp"
#include "gol/hip_util.hpp"
#include "life_batch_common.hpp"

namespace gol {
namespace hipk {
namespace batch {

struct ClusterArgs {
  int64_t B;
  const uint8_t* cells;    // (B, H, W) 0/1 bytes, or
  const uint32_t* words;   // (B, H, W/32) packed words
  int32_t* counts;         // count pass: clusters per universe
  const int32_t* offsets;  // emit pass: first record of each universe
  int64_t total;           // emit pass: records in all
  uint64_t* signature;
  uint2* meta;
};

template <int NW, int H, bool DEAD, int VM, bool EMIT>
__global__ __launch_bounds__(kBlock) void life_batch_clusters_kernel(const ClusterArgs a) {
  constexpr int UPW = 64 / H, W = 32 * NW;
  const int lane = int(threadIdx.x) & 63;
  const int64_t wave = int64_t(blockIdx.x) * (kBlock / 64) + (int(threadIdx.x) >> 6);
  const int row = lane & (H - 1);
  const int base = lane & ~(H - 1);
  const int64_t u = wave * UPW + lane / H;
  const bool valid = u < a.B;

  uint32_t rest[NW];
#pragma unroll
  for (int i = 0; i < NW; ++i) rest[i] = 0u;
  if (valid) {
    if (a.cells) {
      const uint32_t* src = reinterpret_cast<const uint32_t*>(a.cells + (u * H + row) * int64_t(W));
      GOL_BATCH_PACK_ROW(NW, src, rest)
    } else {
#pragma unroll
      for (int i = 0; i < NW; ++i) rest[i] = a.words[(u * H + row) * NW + i];
    }
  }

  const int up4 = 4 * (base | ((row - 1) & (H - 1))), dn4 = 4 * (base | ((row + 1) & (H - 1)));
  const uint64_t mine = H == 64 ? ~uint64_t(0) : ((uint64_t(1) << (H & 63)) - 1) << base;
  // The plane: what a row takes from one and two rows above and below.
  const uint32_t up1 = (DEAD && row < 1) ? 0u : ~0u, up2 = (DEAD && row < 2) ? 0u : ~0u;
  const uint32_t dn1 = (DEAD && row > H - 2) ? 0u : ~0u, dn2 = (DEAD && row > H - 3) ? 0u : ~0u;

  int n = 0;  // clusters of this lane's universe so far
  for (;;) {
    uint32_t any = 0;
#pragma unroll
    for (int i = 0; i < NW; ++i) any |= rest[i];
    const uint64_t left = __builtin_amdgcn_ballot_w64(any != 0);
    if (left == 0) break;
    const uint64_t rows_left = left & mine;
    const bool act = rows_left != 0;  // this universe has a cluster to take
    const bool seed = act && lane == __builtin_ctzll(rows_left | (uint64_t(1) << 63));
    uint32_t comp[NW];
    {
      bool taken = !seed;
#pragma unroll
      for (int i = 0; i < NW; ++i) {
        comp[i] = taken ? 0u : rest[i] & (0u - rest[i]);
        taken = taken || rest[i] != 0;
      }
    }

    bool growing = act;
    while (__builtin_amdgcn_ballot_w64(growing) != 0) {
      uint32_t diff = 0, grown[NW];
#pragma unroll
      for (int i = 0; i < NW; ++i) {
        const uint32_t lw = i > 0 ? comp[i - 1] : DEAD ? 0u : comp[NW - 1];
        const uint32_t rw = i + 1 < NW ? comp[i + 1] : DEAD ? 0u : comp[0];
        const uint32_t h = comp[i] | __builtin_amdgcn_alignbit(comp[i], lw, 31) |  // cell x-1 at bit x
                           __builtin_amdgcn_alignbit(comp[i], lw, 30) |            // cell x-2
                           __builtin_amdgcn_alignbit(rw, comp[i], 1) |             // cell x+1
                           __builtin_amdgcn_alignbit(rw, comp[i], 2);              // cell x+2
        const uint32_t a1 = vmove<H, VM, true>(h, up4), a2 = vmove<H, VM, true>(a1, up4);
        const uint32_t b1 = vmove<H, VM, false>(h, dn4), b2 = vmove<H, VM, false>(b1, dn4);
        const uint32_t d = (h | (a1 & up1) | (a2 & up2) | (b1 & dn1) | (b2 & dn2)) & rest[i];
        diff |= d ^ comp[i];
        grown[i] = d;
      }
#pragma unroll
      for (int i = 0; i < NW; ++i) comp[i] = grown[i];
      const uint64_t changed = __builtin_amdgcn_ballot_w64(diff != 0);
      growing = growing && (changed & mine) != 0;
    }

    // ---- measuring ----------------------------------------------------------
    uint32_t nz = 0;
    int pop = 0;
    uint32_t cols[NW];
#pragma unroll
    for (int i = 0; i < NW; ++i) {
      nz |= comp[i];
      pop += __builtin_popcount(comp[i]);
      cols[i] = comp[i];
    }
    const uint64_t occupied = __builtin_amdgcn_ballot_w64(nz != 0);
    const uint64_t row_mask = H == 64 ? occupied : (occupied >> base) & ((uint64_t(1) << (H & 63)) - 1);
#pragma unroll
    for (int off = 1; off < H; off <<= 1) {
      pop += __shfl_xor(pop, off, 64);
#pragma unroll
      for (int i = 0; i < NW; ++i) cols[i] |= uint32_t(__shfl_xor(int(cols[i]), off, 64));
    }
    const uint64_t col_mask = NW == 1 ? uint64_t(cols[0]) : uint64_t(cols[0]) | uint64_t(cols[NW - 1]) << 32;
    const ClusterAxis ay = cluster_axis(row_mask, H, !DEAD), ax = cluster_axis(col_mask, W, !DEAD);
    uint64_t sig;
    if constexpr (NW == 1) {
      const uint32_t v = __builtin_amdgcn_alignbit(comp[0], comp[0], uint32_t(ax.origin));  // rotate right
      sig = uint64_t(v) * fingerprint_col_key(0);
    } else {
      const uint64_t v = rotl_bits(uint64_t(comp[0]) | uint64_t(comp[NW - 1]) << 32, (W - ax.origin) & (W - 1), W);
      sig = uint64_t(uint32_t(v)) * fingerprint_col_key(0) + (v >> 32) * fingerprint_col_key(1);
    }
    sig *= uint64_t(fingerprint_row_key(uint32_t((row - ay.origin) & (H - 1))));
#pragma unroll
    for (int off = 1; off < H; off <<= 1) sig += uint64_t(__shfl_xor((unsigned long long)sig, off, 64));

    if constexpr (EMIT) {
      if (act && valid && row == 0) {
        const int64_t at = int64_t(a.offsets[u]) + n;
        if (at < a.total) {
          a.signature[at] = sig;
          const uint32_t spanning = (ax.spans ? uint32_t(kSpansX) : 0u) | (ay.spans ? uint32_t(kSpansY) : 0u);
          a.meta[at] = make_uint2(uint32_t(pop), uint32_t(ay.extent) | uint32_t(ax.extent) << 8 | spanning << 16);
        }
      }
    }
    n += act ? 1 : 0;
    // No unroll pragma on the last loop of the body: it ends up on the
    // enclosing loop's back edge, which cannot be unrolled.
    for (int i = 0; i < NW; ++i) rest[i] &= ~comp[i];
  }
  if constexpr (!EMIT) {
    if (valid && row == 0) a.counts[u] = n;
  }
}

using ClusterFn = void (*)(const ClusterArgs&, int64_t waves, hipStream_t);

template <int NW, int H, bool DEAD, int VM, bool EMIT>
void launch_clusters(const ClusterArgs& a, int64_t waves, hipStream_t s) {
  const int64_t blocks = ceil_div(waves, kBlock / 64);
  hipLaunchKernelGGL((life_batch_clusters_kernel<NW, H, DEAD, VM, EMIT>), dim3(uint32_t(blocks)), dim3(kBlock), 0, s,
                     a);
}

// [word count][height][boundary][vertical move][emit]
struct ClusterTable {
  ClusterFn fn[2][4][2][2][2];
};

template <int NW, int H, bool DEAD>
void fill_cluster_moves(ClusterFn (&f)[2][2]) {
  constexpr int kDpp = has_dpp(H) ? kVmDpp : kVmBpermute;
  f[kVmDpp][0] = launch_clusters<NW, H, DEAD, kDpp, false>;
  f[kVmDpp][1] = launch_clusters<NW, H, DEAD, kDpp, true>;
  f[kVmBpermute][0] = launch_clusters<NW, H, DEAD, kVmBpermute, false>;
  f[kVmBpermute][1] = launch_clusters<NW, H, DEAD, kVmBpermute, true>;
}
template <int NW, int H>
void fill_cluster_shape(ClusterFn (&f)[2][2][2]) {
  fill_cluster_moves<NW, H, false>(f[0]);
  fill_cluster_moves<NW, H, true>(f[1]);
}
template <int NW>
void fill_cluster_words(ClusterFn (&f)[4][2][2][2]) {
  fill_cluster_shape<NW, 8>(f[0]);
  fill_cluster_shape<NW, 16>(f[1]);
  fill_cluster_shape<NW, 32>(f[2]);
  fill_cluster_shape<NW, 64>(f[3]);
}
const ClusterTable& cluster_kernels() {
  static const ClusterTable t = [] {
    ClusterTable c;
    fill_cluster_words<1>(c.fn[0]);
    fill_cluster_words<2>(c.fn[1]);
    return c;
  }();
  return t;
}

ClusterCensus find_clusters_device(int W, int H, bool dead, int vm, int64_t B, const uint8_t* d_cells,
                                   const uint32_t* d_words) {
  const int NW = W / 32, upw = 64 / H;
  const int64_t waves = ceil_div(B, upw);
  const int hi = H == 8 ? 0 : H == 16 ? 1 : H == 32 ? 2 : 3;
  const auto& fn = cluster_kernels().fn[NW - 1][hi][dead ? 1 : 0][vm];

  ClusterCensus res;
  res.clusters.resize(size_t(B));
  DeviceBuf<int32_t> d_counts{size_t(B)};
  ClusterArgs a{};
  a.B = B;
  a.cells = d_cells;
  a.words = d_words;
  a.counts = d_counts.p;
  res.count_ms = timed_launch([&] { fn[0](a, waves, nullptr); });
  HIP_CHECK(hipMemcpy(res.clusters.data(), d_counts.p, size_t(B) * sizeof(int32_t), hipMemcpyDeviceToHost));
  std::vector<int32_t> offsets;
  const int64_t total = cluster_offsets(res.clusters, offsets);  // refuses more than 2^28 records
  res.ms = res.count_ms;
  if (total == 0) return res;

  DeviceBuf<int32_t> d_offsets{size_t(B)};
  DeviceBuf<uint64_t> d_sig{size_t(total)};
  DeviceBuf<uint2> d_meta{size_t(total)};
  HIP_CHECK(hipMemcpy(d_offsets.p, offsets.data(), size_t(B) * sizeof(int32_t), hipMemcpyHostToDevice));
  a.counts = nullptr;
  a.offsets = d_offsets.p;
  a.total = total;
  a.signature = d_sig.p;
  a.meta = d_meta.p;
  res.ms += timed_launch([&] { fn[1](a, waves, nullptr); });

  res.signature.resize(size_t(total));
  std::vector<uint2> meta{size_t(total)};
  HIP_CHECK(hipMemcpy(res.signature.data(), d_sig.p, size_t(total) * sizeof(uint64_t), hipMemcpyDeviceToHost));
  HIP_CHECK(hipMemcpy(meta.data(), d_meta.p, size_t(total) * sizeof(uint2), hipMemcpyDeviceToHost));
  res.universe.resize(size_t(total));
  res.cells.resize(size_t(total));
  res.height.resize(size_t(total));
  res.width.resize(size_t(total));
  res.spanning.resize(size_t(total));
  for (int64_t u = 0; u < B; ++u)
    for (int32_t i = 0; i < res.clusters[size_t(u)]; ++i) res.universe[size_t(offsets[size_t(u)] + i)] = int32_t(u);
  for (size_t i = 0; i < size_t(total); ++i) {
    res.cells[i] = int32_t(meta[i].x);
    res.height[i] = int16_t(meta[i].y & 0xFF);
    res.width[i] = int16_t((meta[i].y >> 8) & 0xFF);
    res.spanning[i] = uint8_t(meta[i].y >> 16);
  }
  return res;
}

}  // namespace batch
}  // namespace hipk

ClusterCensus find_clusters_hip(int device, int W, int H, Boundary boundary, int64_t B, const uint8_t* cells,
                                const Tuning& tune) {
  namespace hb = hipk::batch;
  BatchConfig cfg;
  cfg.W = W;
  cfg.H = H;
  BatchInput in;
  in.B = B;
  in.cells = cells;
  validate_batch(cfg, in);
  GOL_REQUIRE(cells != nullptr, "find_clusters: no grids given");
  const int vm = hb::parse_vmove(tune, H);
  GOL_REQUIRE(hip_available(), "no HIP device available (HIP engine requested)");
  DeviceScope scope(device);
  const size_t n = size_t(B) * H * W;
  hb::DeviceBuf<uint8_t> d_cells{n};
  HIP_CHECK(hipMemcpy(d_cells.p, cells, n, hipMemcpyHostToDevice));
  return hb::find_clusters_device(W, H, boundary == Boundary::Dead, vm, B, d_cells.p, nullptr);
}

}  // namespace gol
