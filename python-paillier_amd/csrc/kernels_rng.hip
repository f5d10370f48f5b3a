// kernels_rng.hip — the ChaCha20 keystream kernel (chacha_rows.h chacha_rows_body): random exponent rows written where the
// fixed-base comb kernel (kernels_fb.hip) reads them.  One lane per 64-byte block, no LDS, no multiply-adds; key, nonce and
// counter travel in the kernel's arguments.
#include <hip/hip_runtime.h>
#include <stdint.h>

// clang-format off
#include "wave_gfx950.h"
#include "chacha_rows.h"
// clang-format on

namespace phe {
namespace rng {

constexpr int kBlock = 256;  // threads per workgroup = 256 keystream blocks per trip

__global__ void __launch_bounds__(kBlock) k_chacha_rows(ChaChaRowsArgs A) {
    chacha_rows_body(A, blockIdx.x * kBlock + threadIdx.x, gridDim.x * kBlock);
}

int launch_chacha_rows(int blocks, hipStream_t st, const ChaChaRowsArgs& A) {
    k_chacha_rows<<<dim3(blocks), dim3(kBlock), 0, st>>>(A);
    return 0;
}

}  // namespace rng
}  // namespace phe
