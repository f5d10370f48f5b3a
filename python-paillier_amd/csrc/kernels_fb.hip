// kernels_fb.hip — the fixed-base comb kernel (fixed_base.h fixed_base_pow_body: powers of one base by many short exponents,
// a table look-up and a pair product per exponent digit) for every pair geometry (G, L) that the parts kernels_s*.hip hold a
// k_pair_mul for: the table, the rows it may start from and the rows it may leave are those resident pair rows.  Launch bounds,
// LDS stride and grid sizing are those of k_pair_mul (split_kernels.inc), as in kernels_seg.hip.
#include <hip/hip_runtime.h>
#include <stdint.h>

// clang-format off
#include "wave_gfx950.h"
#include "mont_core.h"
#include "split_core.h"
#include "fixed_base.h"
// clang-format on

namespace phe {
namespace fb {

constexpr int kBlock = 256;  // threads per workgroup = 4 wavefronts = 256/G limb groups

// words between the LDS rows of two limb groups (split_kernels.inc split_lds_stride: odd for one lane per number)
template <int G, int L>
constexpr int lds_stride() {
    return G == 1 ? ((2 * G * L + kLdsPad) | 1) : 2 * G * L + kLdsPad;
}

template <int G, int L, bool CONV, bool EXIT>
__global__ void __launch_bounds__(kBlock, L >= 14 ? 2 : 1) k_fixed_base_pow(FixedBaseArgs A) {
    constexpr int kGroups = kBlock / G, kLdsStride = lds_stride<G, L>();
    __shared__ __attribute__((aligned(16))) uint32_t lds[kGroups * kLdsStride];
    const uint32_t grp = threadIdx.x / G;
    fixed_base_pow_body<G, L, CONV, EXIT>(A, lds + grp * kLdsStride, blockIdx.x * kGroups + grp, gridDim.x * kGroups, threadIdx.x & 63u);
}

// the (G, L) of the PHE_FOR_EACH_L lists of kernels_s*.hip (the list of kernels_seg.hip)
#define PHE_FB_FOR_EACH_GL(X)                                                                                         \
    X(1, 18)                                                                                                          \
    X(2, 9) X(2, 18) X(2, 27)                                                                                         \
    X(4, 5) X(4, 9) X(4, 14) X(4, 18) X(4, 27)                                                                        \
    X(8, 3) X(8, 5) X(8, 7) X(8, 9) X(8, 14) X(8, 18)                                                                 \
    X(16, 1) X(16, 2) X(16, 3) X(16, 4) X(16, 5) X(16, 7) X(16, 9) X(16, 14) X(16, 18)                                \
    X(64, 1) X(64, 2) X(64, 3) X(64, 5)

// mul_is_residue: A.mul holds canonical residues (converted as they are read); exit: leave the pair form on the way out.
// -1: no kernel for that geometry
int launch_fixed_base_pow(int G, int L, int blocks, hipStream_t st, const FixedBaseArgs& A, bool mul_is_residue, bool exit) {
    switch (G * 100 + L) {
#define X(GG, LL)                                                                                                     \
    case GG * 100 + LL:                                                                                              \
        if (mul_is_residue && exit) k_fixed_base_pow<GG, LL, true, true><<<dim3(blocks), dim3(kBlock), 0, st>>>(A);    \
        else if (mul_is_residue) k_fixed_base_pow<GG, LL, true, false><<<dim3(blocks), dim3(kBlock), 0, st>>>(A);      \
        else if (exit) k_fixed_base_pow<GG, LL, false, true><<<dim3(blocks), dim3(kBlock), 0, st>>>(A);                \
        else k_fixed_base_pow<GG, LL, false, false><<<dim3(blocks), dim3(kBlock), 0, st>>>(A);                         \
        return 0;
        PHE_FB_FOR_EACH_GL(X)
#undef X
        default: return -1;
    }
}

}  // namespace fb
}  // namespace phe
