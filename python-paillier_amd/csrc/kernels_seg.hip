// kernels_seg.hip — the grouped-sum kernel (segment_core.h segment_reduce_body), the running-sum kernel (segment_scan_body:
// the same walk, storing after every product and starting from a carry) and the packing kernel (segment_pack_body: the walk
// from the top row of a task down, slot_bits squarings between two rows) for every pair geometry (G, L) that the parts
// kernels_s*.hip hold a k_pair_mul for: the rows it reads and writes are those resident pair rows.  Launch bounds, LDS stride
// and grid sizing are those of k_pair_mul (split_kernels.inc).
#include <hip/hip_runtime.h>
#include <stdint.h>

// clang-format off
#include "wave_gfx950.h"
#include "mont_core.h"
#include "split_core.h"
#include "segment_core.h"
// clang-format on

namespace phe {
namespace seg {

constexpr int kBlock = 256;  // threads per workgroup = 4 wavefronts = 256/G limb groups

// words between the LDS rows of two limb groups (split_kernels.inc split_lds_stride: odd for one lane per number)
template <int G, int L>
constexpr int lds_stride() {
    return G == 1 ? ((2 * G * L + kLdsPad) | 1) : 2 * G * L + kLdsPad;
}

template <int G, int L, bool PAIR>
__global__ void __launch_bounds__(kBlock, L >= 14 ? 2 : 1) k_segment_reduce(SegmentArgs A) {
    constexpr int kGroups = kBlock / G, kLdsStride = lds_stride<G, L>();
    __shared__ __attribute__((aligned(16))) uint32_t lds[kGroups * kLdsStride];
    const uint32_t grp = threadIdx.x / G;
    segment_reduce_body<G, L, PAIR>(A, lds + grp * kLdsStride, blockIdx.x * kGroups + grp, gridDim.x * kGroups, threadIdx.x & 63u);
}

template <int G, int L, bool PAIR>
__global__ void __launch_bounds__(kBlock, L >= 14 ? 2 : 1) k_segment_scan(ScanArgs A) {
    constexpr int kGroups = kBlock / G, kLdsStride = lds_stride<G, L>();
    __shared__ __attribute__((aligned(16))) uint32_t lds[kGroups * kLdsStride];
    const uint32_t grp = threadIdx.x / G;
    segment_scan_body<G, L, PAIR>(A, lds + grp * kLdsStride, blockIdx.x * kGroups + grp, gridDim.x * kGroups, threadIdx.x & 63u);
}

template <int G, int L, bool PAIR>
__global__ void __launch_bounds__(kBlock, L >= 14 ? 2 : 1) k_segment_pack(PackArgs A) {
    constexpr int kGroups = kBlock / G, kLdsStride = lds_stride<G, L>();
    __shared__ __attribute__((aligned(16))) uint32_t lds[kGroups * kLdsStride];
    const uint32_t grp = threadIdx.x / G;
    segment_pack_body<G, L, PAIR>(A, lds + grp * kLdsStride, blockIdx.x * kGroups + grp, gridDim.x * kGroups, threadIdx.x & 63u);
}

// the (G, L) of the PHE_FOR_EACH_L lists of kernels_s*.hip
#define PHE_SEG_FOR_EACH_GL(X)                                                                                        \
    X(1, 18)                                                                                                          \
    X(2, 9) X(2, 18) X(2, 27)                                                                                         \
    X(4, 5) X(4, 9) X(4, 14) X(4, 18) X(4, 27)                                                                        \
    X(8, 3) X(8, 5) X(8, 7) X(8, 9) X(8, 14) X(8, 18)                                                                 \
    X(16, 1) X(16, 2) X(16, 3) X(16, 4) X(16, 5) X(16, 7) X(16, 9) X(16, 14) X(16, 18)                                \
    X(64, 1) X(64, 2) X(64, 3) X(64, 5)

// -1: no kernel for that geometry
int launch_segment_reduce(int G, int L, int blocks, hipStream_t st, const SegmentArgs& A) {
    switch (G * 100 + L) {
#define X(GG, LL)                                                                                       \
    case GG * 100 + LL:                                                                                \
        if (A.rows_are_pair) k_segment_reduce<GG, LL, true><<<dim3(blocks), dim3(kBlock), 0, st>>>(A);  \
        else k_segment_reduce<GG, LL, false><<<dim3(blocks), dim3(kBlock), 0, st>>>(A);                 \
        return 0;
        PHE_SEG_FOR_EACH_GL(X)
#undef X
        default: return -1;
    }
}

// -1: no kernel for that geometry
int launch_segment_scan(int G, int L, int blocks, hipStream_t st, const ScanArgs& A) {
    switch (G * 100 + L) {
#define X(GG, LL)                                                                                     \
    case GG * 100 + LL:                                                                              \
        if (A.rows_are_pair) k_segment_scan<GG, LL, true><<<dim3(blocks), dim3(kBlock), 0, st>>>(A);  \
        else k_segment_scan<GG, LL, false><<<dim3(blocks), dim3(kBlock), 0, st>>>(A);                 \
        return 0;
        PHE_SEG_FOR_EACH_GL(X)
#undef X
        default: return -1;
    }
}

// -1: no kernel for that geometry
int launch_segment_pack(int G, int L, int blocks, hipStream_t st, const PackArgs& A) {
    switch (G * 100 + L) {
#define X(GG, LL)                                                                                     \
    case GG * 100 + LL:                                                                              \
        if (A.rows_are_pair) k_segment_pack<GG, LL, true><<<dim3(blocks), dim3(kBlock), 0, st>>>(A);  \
        else k_segment_pack<GG, LL, false><<<dim3(blocks), dim3(kBlock), 0, st>>>(A);                 \
        return 0;
        PHE_SEG_FOR_EACH_GL(X)
#undef X
        default: return -1;
    }
}

}  // namespace seg
}  // namespace phe
