// What the batch kernels share (life_batch.hip, life_batch_clusters.hip): the
// workgroup size, the vertical move between the lanes of one universe, and the
// packing of a row of 0/1 bytes into the lane's words.  The lane mapping is
// described in life_batch.hip.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "gol/batch.hpp"
#include "gol/hip_util.hpp"
#include "gol/tuning.hpp"

namespace gol {
namespace hipk {
namespace batch {

constexpr int kBlock = 256;  // four independent waves per workgroup
constexpr int kVmDpp = 0, kVmBpermute = 1;

// Whether the height has a DPP move of its own (the others always permute).
constexpr bool has_dpp(int H) { return H == 64 || H == 16; }

// Lane i receives v of the lane one row above (kUp) or below within its
// universe of H lanes, wrapping inside the universe.  Every lane of a rotate
// has a source, so bound_ctrl changes no value: it only spares the move that
// would initialise the destination.
template <int H, int VM, bool kUp>
__device__ __forceinline__ uint32_t vmove(uint32_t v, int src4) {
  if constexpr (VM == kVmDpp && H == 64) {
    constexpr int ctrl = kUp ? 0x13C : 0x134;  // wave_ror:1 : wave_rol:1
    return uint32_t(__builtin_amdgcn_update_dpp(0, int(v), ctrl, 0xF, 0xF, true));
  } else if constexpr (VM == kVmDpp && H == 16) {
    constexpr int ctrl = kUp ? 0x121 : 0x12F;  // row_ror:1 : row_ror:15
    return uint32_t(__builtin_amdgcn_update_dpp(0, int(v), ctrl, 0xF, 0xF, true));
  } else {
    return uint32_t(__builtin_amdgcn_ds_bpermute(src4, int(v)));
  }
}

// A row of 32 * NW cells, one 0/1 byte each (src: const uint32_t*, the row's
// first byte, read as words of four cells), packed into c[]: cell 32 i + b at
// bit b of c[i].  A macro, not a function: the simulation kernel's code is
// then the same instruction for instruction as with the loop written in place
// (an inlined function schedules the prologue's loads differently).
#define GOL_BATCH_PACK_ROW(NW, src, c)                                                           \
  _Pragma("unroll") for (int i = 0; i < (NW); ++i) {                                             \
    uint32_t w = 0;                                                                              \
    _Pragma("unroll") for (int q = 0; q < 8; ++q) {                                              \
      const uint32_t v = (src)[8 * i + q]; /* four cells, one per byte */                        \
      w |= ((v & 1u) | ((v >> 7) & 2u) | ((v >> 14) & 4u) | ((v >> 21) & 8u)) << (4 * q);        \
    }                                                                                            \
    (c)[i] = w;                                                                                  \
  }

// ---- host side ------------------------------------------------------------------

template <class T>
struct DeviceBuf {
  T* p = nullptr;
  explicit DeviceBuf(size_t n) {
    if (n) HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&p), n * sizeof(T)));
  }
  ~DeviceBuf() {
    if (p) (void)hipFree(p);
  }
  DeviceBuf(const DeviceBuf&) = delete;
  DeviceBuf& operator=(const DeviceBuf&) = delete;
};

// Tuning batch_vmove for universes of height H: kVmDpp or kVmBpermute.
inline int parse_vmove(const Tuning& tune, int H) {
  const std::string& vm_text = tune.s("batch_vmove");
  GOL_REQUIRE(vm_text == "auto" || vm_text == "dpp" || vm_text == "bpermute",
              "tuning batch_vmove=" + vm_text + ": auto, dpp or bpermute");
  GOL_REQUIRE(vm_text != "dpp" || has_dpp(H),
              "tuning batch_vmove=dpp: heights 64 and 16 have a DPP move, " + std::to_string(H) + " permutes");
  return vm_text == "bpermute" || !has_dpp(H) ? kVmBpermute : kVmDpp;
}

// launch() on the null stream between an event pair, waited for: its milliseconds.
template <class Launch>
double timed_launch(Launch&& launch) {
  hipEvent_t e0 = nullptr, e1 = nullptr;
  HIP_CHECK(hipEventCreate(&e0));
  HIP_CHECK(hipEventCreate(&e1));
  float ms = 0;
  hipError_t err = hipEventRecord(e0, nullptr);
  if (err == hipSuccess) {
    launch();
    err = hipGetLastError();
  }
  if (err == hipSuccess) err = hipEventRecord(e1, nullptr);
  if (err == hipSuccess) err = hipEventSynchronize(e1);
  if (err == hipSuccess) err = hipEventElapsedTime(&ms, e0, e1);
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  HIP_CHECK(err);
  return ms;
}

// The cluster census of B universes on the current device (life_batch_clusters.hip):
// a count pass, the host's exclusive scan, an emit pass.  The grids are 0/1
// bytes (B, H, W) or packed words (B, H, W / 32), both device pointers, one of
// them null.  vm: kVmDpp or kVmBpermute.
ClusterCensus find_clusters_device(int W, int H, bool dead, int vm, int64_t B, const uint8_t* d_cells,
                                   const uint32_t* d_words);

}  // namespace batch
}  // namespace hipk
}  // namespace gol
