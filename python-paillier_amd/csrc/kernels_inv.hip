// kernels_inv.hip — the two walks of the simultaneous inversion on pair rows (pair_invert.h: pair_invert_prefix_body, the running
// products of every block of rows and the blocks' totals; pair_invert_walk_body, the inverses from the inverse of a block's
// total) for every pair geometry (G, L) that the parts kernels_s*.hip hold a k_pair_mul for.  Launch bounds, LDS stride and grid
// sizing are those of the segment walks (kernels_seg.hip).
#include <hip/hip_runtime.h>
#include <stdint.h>

// clang-format off
#include "wave_gfx950.h"
#include "mont_core.h"
#include "split_core.h"
#include "pair_invert.h"
// clang-format on

namespace phe {
namespace inv {

constexpr int kBlock = 256;  // threads per workgroup = 4 wavefronts = 256/G limb groups

// words between the LDS rows of two limb groups (split_kernels.inc split_lds_stride: odd for one lane per number)
template <int G, int L>
constexpr int lds_stride() {
    return G == 1 ? ((2 * G * L + kLdsPad) | 1) : 2 * G * L + kLdsPad;
}

template <int G, int L>
__global__ void __launch_bounds__(kBlock, L >= 14 ? 2 : 1) k_pair_invert_prefix(PairInvertArgs A) {
    constexpr int kGroups = kBlock / G, kLdsStride = lds_stride<G, L>();
    __shared__ __attribute__((aligned(16))) uint32_t lds[kGroups * kLdsStride];
    const uint32_t grp = threadIdx.x / G;
    pair_invert_prefix_body<G, L>(A, lds + grp * kLdsStride, blockIdx.x * kGroups + grp, gridDim.x * kGroups, threadIdx.x & 63u);
}

template <int G, int L>
__global__ void __launch_bounds__(kBlock, L >= 14 ? 2 : 1) k_pair_invert_walk(PairInvertArgs A) {
    constexpr int kGroups = kBlock / G, kLdsStride = lds_stride<G, L>();
    __shared__ __attribute__((aligned(16))) uint32_t lds[kGroups * kLdsStride];
    const uint32_t grp = threadIdx.x / G;
    pair_invert_walk_body<G, L>(A, lds + grp * kLdsStride, blockIdx.x * kGroups + grp, gridDim.x * kGroups, threadIdx.x & 63u);
}

// the (G, L) of the PHE_FOR_EACH_L lists of kernels_s*.hip
#define PHE_INV_FOR_EACH_GL(X)                                                                                        \
    X(1, 18)                                                                                                          \
    X(2, 9) X(2, 18) X(2, 27)                                                                                         \
    X(4, 5) X(4, 9) X(4, 14) X(4, 18) X(4, 27)                                                                        \
    X(8, 3) X(8, 5) X(8, 7) X(8, 9) X(8, 14) X(8, 18)                                                                 \
    X(16, 1) X(16, 2) X(16, 3) X(16, 4) X(16, 5) X(16, 7) X(16, 9) X(16, 14) X(16, 18)                                \
    X(64, 1) X(64, 2) X(64, 3) X(64, 5)

// up: the walk back from the inverses of the totals; else the running products.  -1: no kernel for that geometry
int launch_pair_invert(int G, int L, bool up, int blocks, hipStream_t st, const PairInvertArgs& A) {
    switch (G * 100 + L) {
#define X(GG, LL)                                                                          \
    case GG * 100 + LL:                                                                   \
        if (up) k_pair_invert_walk<GG, LL><<<dim3(blocks), dim3(kBlock), 0, st>>>(A);      \
        else k_pair_invert_prefix<GG, LL><<<dim3(blocks), dim3(kBlock), 0, st>>>(A);       \
        return 0;
        PHE_INV_FOR_EACH_GL(X)
#undef X
        default: return -1;
    }
}

}  // namespace inv
}  // namespace phe
