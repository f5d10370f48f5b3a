// kernels_slots.hip — the slot codec of packed plaintexts (slot_codec.h): k_slots_pack turns int64 values into plaintext rows
// mod n, k_slots_unpack turns plaintext rows into int64 values and one status byte per row.  A row is owned by a limb group of
// G lanes with K consecutive 32-bit words per lane; the (G, K) below are those host::slot_geometry picks.  Both kernels move
// bit fields and are bound by memory: no LDS, a handful of registers, a grid-stride walk over the rows.
#include <hip/hip_runtime.h>
#include <stdint.h>

// clang-format off
#include "wave_gfx950.h"
#include "mont_core.h"
#include "slot_codec.h"
// clang-format on

namespace phe {
namespace slots {

constexpr int kBlock = 256;  // threads per workgroup = 4 wavefronts = 256/G limb groups

template <int G, int K>
__global__ void __launch_bounds__(kBlock) k_slots_pack(SlotPackArgs A) {
    constexpr int kGroups = kBlock / G;
    slots_pack_body<G, K>(A, blockIdx.x * kGroups + threadIdx.x / G, gridDim.x * kGroups, threadIdx.x & 63u);
}

template <int G, int K>
__global__ void __launch_bounds__(kBlock) k_slots_unpack(SlotUnpackArgs A) {
    constexpr int kGroups = kBlock / G;
    slots_unpack_body<G, K>(A, blockIdx.x * kGroups + threadIdx.x / G, gridDim.x * kGroups, threadIdx.x & 63u);
}

// the (G, K) of host::slot_geometry
#define PHE_SLOTS_FOR_EACH_GK(X) X(16, 1) X(16, 2) X(16, 4) X(64, 2) X(64, 4) X(64, 8)

// -1: no kernel for that geometry
int launch_slots_pack(int G, int K, int blocks, hipStream_t st, const SlotPackArgs& A) {
    switch (G * 100 + K) {
#define X(GG, KK)                                                        \
    case GG * 100 + KK:                                                  \
        k_slots_pack<GG, KK><<<dim3(blocks), dim3(kBlock), 0, st>>>(A);  \
        return 0;
        PHE_SLOTS_FOR_EACH_GK(X)
#undef X
        default: return -1;
    }
}

// -1: no kernel for that geometry
int launch_slots_unpack(int G, int K, int blocks, hipStream_t st, const SlotUnpackArgs& A) {
    switch (G * 100 + K) {
#define X(GG, KK)                                                          \
    case GG * 100 + KK:                                                    \
        k_slots_unpack<GG, KK><<<dim3(blocks), dim3(kBlock), 0, st>>>(A);  \
        return 0;
        PHE_SLOTS_FOR_EACH_GK(X)
#undef X
        default: return -1;
    }
}

}  // namespace slots
}  // namespace phe
