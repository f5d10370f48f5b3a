// TEST INFRASTRUCTURE — the value codec's device bodies (csrc/value_codec.h values_encode_body / values_decode_body) compiled for
// the CPU on the wave emulator (wave_emu.h), beside emu_slots.cpp: tests/test_value_codec.py builds this file into a library of
// its own.
#include <stdint.h>

#include "wave_emu.h"
// clang-format off
#include "../../python-paillier_amd/csrc/mont_core.h"
#include "../../python-paillier_amd/csrc/slot_codec.h"
#include "../../python-paillier_amd/csrc/value_codec.h"
// clang-format on

#include <stdexcept>
#include <string>
#include <vector>

using namespace phe;

static thread_local std::string g_err;

// the (G, K) of host::slot_geometry (the list of kernels_values.hip)
#define DISPATCH_VALUES(G_, K_, CALL)                                                 \
    switch ((G_) * 100 + (K_)) {                                                      \
        case 1601: { constexpr int GG = 16, KK = 1; CALL; break; }                    \
        case 1602: { constexpr int GG = 16, KK = 2; CALL; break; }                    \
        case 1604: { constexpr int GG = 16, KK = 4; CALL; break; }                    \
        case 6402: { constexpr int GG = 64, KK = 2; CALL; break; }                    \
        case 6404: { constexpr int GG = 64, KK = 4; CALL; break; }                    \
        case 6408: { constexpr int GG = 64, KK = 8; CALL; break; }                    \
        default: throw std::invalid_argument("unsupported geometry");                 \
    }

// `waves` wavefronts of 64/G limb groups stride over the rows like the GPU grid does
template <int G, int K>
static void run_encode(const ValueEncodeArgs& A, int waves) {
    constexpr int kPer = 64 / G;
    for (int w = 0; w < waves; ++w)
        wave::run_wave([&](uint32_t lane) { values_encode_body<G, K>(A, (uint32_t)w * kPer + lane / G, (uint32_t)(kPer * waves), lane); });
}
template <int G, int K>
static void run_decode(const ValueDecodeArgs& A, int waves) {
    constexpr int kPer = 64 / G;
    for (int w = 0; w < waves; ++w)
        wave::run_wave([&](uint32_t lane) { values_decode_body<G, K>(A, (uint32_t)w * kPer + lane / G, (uint32_t)(kPer * waves), lane); });
}

static SlotConsts consts_of(const std::vector<uint32_t>& rows, int width) {
    SlotConsts k;
    k.offset = rows.data();
    k.n = k.offset + width;
    k.max_int = k.n + width;
    k.neg_low = k.max_int + width;
    k.offset_neg = k.neg_low + width;
    return k;
}

extern "C" {

const char* emu_values_last_error(void) { return g_err.c_str(); }

// gk[0..1] = G, K of the key's plaintext rows.  rc 2: no geometry for that width, rc 3: max_int < 2^64
int emu_values_geometry(const uint32_t* n, int n_limbs, int* gk) {
    int G = 0, K = 0;
    if (!host::value_codec_key_ok(n, n_limbs)) return 3;
    if (!host::slot_geometry(n_limbs, G, K)) return 2;
    gk[0] = G; gk[1] = K;
    return 0;
}

// phe_hip_values_encode_dev.  rc 2: no geometry, rc 3: the arguments the entry point refuses
int emu_values_encode(const uint32_t* n, int n_limbs, const uint64_t* bits, uint64_t count, uint32_t kind, int32_t exponent,
                      uint32_t* m_rows, int32_t* exps, uint8_t* status, int waves) {
    try {
        int G = 0, K = 0;
        if (kind >= 4 || !host::value_codec_key_ok(n, n_limbs)) return 3;
        if (!host::slot_geometry(n_limbs, G, K)) return 2;
        if (kind == kValueFloatPrecision && (exponent < -300 || exponent > 300)) return 3;
        if (count == 0) return 0;
        if (!bits || !m_rows || !status || (kind == kValueFloat && !exps)) return 3;
        const std::vector<uint32_t> k = host::slot_const_rows(n, n_limbs, 0, 0, G * K);
        ValueEncodeArgs A;
        A.n = consts_of(k, G * K).n;
        A.bits = bits; A.count = count; A.kind = kind; A.exponent = exponent;
        A.m_rows = m_rows; A.exps = exps; A.status = status; A.n_limbs = n_limbs;
        if (waves < 1) waves = 1;
        DISPATCH_VALUES(G, K, (run_encode<GG, KK>(A, waves)));
        return 0;
    } catch (const std::exception& e) { g_err = e.what(); return 1; }
}

// phe_hip_values_decode_dev
int emu_values_decode(const uint32_t* n, int n_limbs, const uint32_t* m_rows, uint64_t rows, uint32_t kind, const int32_t* exps,
                      uint64_t* out, uint8_t* status, int waves) {
    try {
        int G = 0, K = 0;
        if (kind >= 2 || !host::value_codec_key_ok(n, n_limbs)) return 3;
        if (!host::slot_geometry(n_limbs, G, K)) return 2;
        if (rows == 0) return 0;
        if (!m_rows || !out || !status || (kind == kDecodeFloat && !exps)) return 3;
        const std::vector<uint32_t> k = host::slot_const_rows(n, n_limbs, 0, 0, G * K);
        ValueDecodeArgs A;
        A.k = consts_of(k, G * K);
        A.m_rows = m_rows; A.rows = rows; A.kind = kind; A.exps = exps; A.out = out; A.status = status; A.n_limbs = n_limbs;
        if (waves < 1) waves = 1;
        DISPATCH_VALUES(G, K, (run_decode<GG, KK>(A, waves)));
        return 0;
    } catch (const std::exception& e) { g_err = e.what(); return 1; }
}

}  // extern "C"
