// kernels_values.hip — the value codec of plain batches (value_codec.h): k_values_encode turns the 64-bit words of int64 /
// uint64 / float64 values into plaintext rows mod n (and, for floats, exponents), k_values_decode turns plaintext rows into one
// int64 or float64 word and one status byte per row.  A row is owned by a limb group of G lanes with K consecutive 32-bit words
// per lane; the (G, K) below are those host::slot_geometry picks.  Both kernels are bound by memory: no LDS, a handful of
// registers, a grid-stride walk over the rows, one 4 K-byte access per lane and row.
#include <hip/hip_runtime.h>
#include <stdint.h>

// clang-format off
#include "wave_gfx950.h"
#include "mont_core.h"
#include "slot_codec.h"
#include "value_codec.h"
// clang-format on

namespace phe {
namespace values {

constexpr int kBlock = 256;  // threads per workgroup = 4 wavefronts = 256/G limb groups

template <int G, int K>
__global__ void __launch_bounds__(kBlock) k_values_encode(ValueEncodeArgs A) {
    constexpr int kGroups = kBlock / G;
    values_encode_body<G, K>(A, blockIdx.x * kGroups + threadIdx.x / G, gridDim.x * kGroups, threadIdx.x & 63u);
}

template <int G, int K>
__global__ void __launch_bounds__(kBlock) k_values_decode(ValueDecodeArgs A) {
    constexpr int kGroups = kBlock / G;
    values_decode_body<G, K>(A, blockIdx.x * kGroups + threadIdx.x / G, gridDim.x * kGroups, threadIdx.x & 63u);
}

// the (G, K) of host::slot_geometry
#define PHE_VALUES_FOR_EACH_GK(X) X(16, 1) X(16, 2) X(16, 4) X(64, 2) X(64, 4) X(64, 8)

// -1: no kernel for that geometry
int launch_values_encode(int G, int K, int blocks, hipStream_t st, const ValueEncodeArgs& A) {
    switch (G * 100 + K) {
#define X(GG, KK)                                                           \
    case GG * 100 + KK:                                                     \
        k_values_encode<GG, KK><<<dim3(blocks), dim3(kBlock), 0, st>>>(A);  \
        return 0;
        PHE_VALUES_FOR_EACH_GK(X)
#undef X
        default: return -1;
    }
}

// -1: no kernel for that geometry
int launch_values_decode(int G, int K, int blocks, hipStream_t st, const ValueDecodeArgs& A) {
    switch (G * 100 + K) {
#define X(GG, KK)                                                           \
    case GG * 100 + KK:                                                     \
        k_values_decode<GG, KK><<<dim3(blocks), dim3(kBlock), 0, st>>>(A);  \
        return 0;
        PHE_VALUES_FOR_EACH_GK(X)
#undef X
        default: return -1;
    }
}

}  // namespace values
}  // namespace phe
