// TEST INFRASTRUCTURE — the keystream body of the device random draw (csrc/chacha_rows.h chacha_rows_body) compiled for the CPU on
// the wave emulator (wave_emu.h), beside emu_slots.cpp: tests/test_device_rng.py builds this file into a library of its own.
#include <stdint.h>

#include "wave_emu.h"
// clang-format off
#include "../../python-paillier_amd/csrc/chacha_rows.h"
// clang-format on

#include <string.h>

#include <stdexcept>
#include <string>

using namespace phe;

static thread_local std::string g_err;

extern "C" {

const char* emu_chacha_last_error(void) { return g_err.c_str(); }

// phe_hip_chacha20_rows_dev on `waves` emulated wavefronts, one lane per keystream block, striding over the blocks like the GPU
// grid does.  rc 3: the arguments the entry point refuses
int emu_chacha20_rows(const uint32_t* key, const uint32_t* nonce, uint32_t counter0, int bits, int limbs, uint32_t* out,
                      uint64_t rows, int waves) {
    try {
        if (!key || !nonce || !out || limbs < 1 || bits < 1 || bits > 32 * limbs) return 3;
        const uint64_t B = ((uint64_t)limbs + 15) / 16;
        if (rows > (((uint64_t)1 << 32) - counter0) / B) return 3;
        if (rows == 0) return 0;
        ChaChaRowsArgs A;
        memcpy(A.key, key, sizeof A.key);
        memcpy(A.nonce, nonce, sizeof A.nonce);
        A.counter0 = counter0;
        A.bits = bits;
        A.limbs = limbs;
        A.blocks_per_row = (int)B;
        A.out = out;
        A.rows = rows;
        if (waves < 1) waves = 1;
        for (int w = 0; w < waves; ++w)
            wave::run_wave([&](uint32_t lane) { chacha_rows_body(A, (uint32_t)w * 64u + lane, (uint32_t)(64 * waves)); });
        return 0;
    } catch (const std::exception& e) { g_err = e.what(); return 1; }
}

}  // extern "C"
