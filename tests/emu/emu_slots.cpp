// TEST INFRASTRUCTURE — the slot codec's device bodies (csrc/slot_codec.h slots_pack_body / slots_unpack_body) compiled for the
// CPU on the wave emulator (wave_emu.h), beside emu_pack.cpp: tests/test_slots.py builds this file into a library of its own.
#include <stdint.h>

#include "wave_emu.h"
// clang-format off
#include "../../python-paillier_amd/csrc/mont_core.h"
#include "../../python-paillier_amd/csrc/slot_codec.h"
// clang-format on

#include <stdexcept>
#include <string>
#include <vector>

using namespace phe;

static thread_local std::string g_err;

// the (G, K) of host::slot_geometry (the list of kernels_slots.hip)
#define DISPATCH_SLOTS(G_, K_, CALL)                                                  \
    switch ((G_) * 100 + (K_)) {                                                      \
        case 1601: { constexpr int GG = 16, KK = 1; CALL; break; }                    \
        case 1602: { constexpr int GG = 16, KK = 2; CALL; break; }                    \
        case 1604: { constexpr int GG = 16, KK = 4; CALL; break; }                    \
        case 6402: { constexpr int GG = 64, KK = 2; CALL; break; }                    \
        case 6404: { constexpr int GG = 64, KK = 4; CALL; break; }                    \
        case 6408: { constexpr int GG = 64, KK = 8; CALL; break; }                    \
        default: throw std::invalid_argument("unsupported slot geometry");            \
    }

// `waves` wavefronts of 64/G limb groups stride over the rows like the GPU grid does
template <int G, int K>
static void run_pack(const SlotPackArgs& A, int waves) {
    constexpr int kPer = 64 / G;
    for (int w = 0; w < waves; ++w)
        wave::run_wave([&](uint32_t lane) { slots_pack_body<G, K>(A, (uint32_t)w * kPer + lane / G, (uint32_t)(kPer * waves), lane); });
}
template <int G, int K>
static void run_unpack(const SlotUnpackArgs& A, int waves) {
    constexpr int kPer = 64 / G;
    for (int w = 0; w < waves; ++w)
        wave::run_wave([&](uint32_t lane) { slots_unpack_body<G, K>(A, (uint32_t)w * kPer + lane / G, (uint32_t)(kPer * waves), lane); });
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

// the argument checks of phe_hip_slots_pack_dev / phe_hip_slots_unpack_dev (csrc/phe_hip.hip slots_check)
static bool shape_ok(const uint32_t* n, int n_limbs, uint32_t slots, uint32_t slot_bits) {
    return slots >= 1 && slot_bits >= 1 && slot_bits <= 64 &&
           (uint64_t)slots * slot_bits <= (uint64_t)host::slot_capacity_bits(n, n_limbs);
}

extern "C" {

const char* emu_slots_last_error(void) { return g_err.c_str(); }

// gk[0..2] = G, K of the key's plaintext rows and max_int.bit_length() - 1.  rc 2: no geometry for that width
int emu_slots_geometry(const uint32_t* n, int n_limbs, int* gk) {
    int G = 0, K = 0;
    if (!host::slot_geometry(n_limbs, G, K)) return 2;
    gk[0] = G; gk[1] = K; gk[2] = host::slot_capacity_bits(n, n_limbs);
    return 0;
}

// the constant rows host::slot_const_rows makes: out holds 5 * G * K words
int emu_slots_consts(const uint32_t* n, int n_limbs, uint32_t slots, uint32_t slot_bits, uint32_t* out) {
    int G = 0, K = 0;
    if (!host::slot_geometry(n_limbs, G, K)) return 2;
    const std::vector<uint32_t> rows = host::slot_const_rows(n, n_limbs, slots, slot_bits, G * K);
    for (size_t i = 0; i < rows.size(); ++i) out[i] = rows[i];
    return 0;
}

// phe_hip_slots_pack_dev.  rc 2: no geometry, rc 3: the arguments the entry point refuses
int emu_slots_pack(const uint32_t* n, int n_limbs, const int64_t* values, uint64_t count, uint32_t slots, uint32_t slot_bits,
                   uint32_t* m_rows, uint64_t rows, int waves) {
    try {
        int G = 0, K = 0;
        if (!host::slot_geometry(n_limbs, G, K)) return 2;
        if (!shape_ok(n, n_limbs, slots, slot_bits) || rows != (count + slots - 1) / slots) return 3;
        if (rows == 0) return 0;
        const std::vector<uint32_t> k = host::slot_const_rows(n, n_limbs, slots, slot_bits, G * K);
        SlotPackArgs A;
        A.k = consts_of(k, G * K);
        A.values = values; A.count = count; A.slots = slots; A.slot_bits = slot_bits;
        A.m_rows = m_rows; A.rows = rows; A.n_limbs = n_limbs;
        if (waves < 1) waves = 1;
        DISPATCH_SLOTS(G, K, (run_pack<GG, KK>(A, waves)));
        return 0;
    } catch (const std::exception& e) { g_err = e.what(); return 1; }
}

// phe_hip_slots_unpack_dev
int emu_slots_unpack(const uint32_t* n, int n_limbs, const uint32_t* m_rows, uint64_t rows, uint32_t slots, uint32_t slot_bits,
                     int64_t* values, uint8_t* status, int waves) {
    try {
        int G = 0, K = 0;
        if (!host::slot_geometry(n_limbs, G, K)) return 2;
        if (!shape_ok(n, n_limbs, slots, slot_bits)) return 3;
        if (rows == 0) return 0;
        const std::vector<uint32_t> k = host::slot_const_rows(n, n_limbs, slots, slot_bits, G * K);
        SlotUnpackArgs A;
        A.k = consts_of(k, G * K);
        A.m_rows = m_rows; A.rows = rows; A.slots = slots; A.slot_bits = slot_bits;
        A.values = values; A.status = status; A.n_limbs = n_limbs;
        if (waves < 1) waves = 1;
        DISPATCH_SLOTS(G, K, (run_unpack<GG, KK>(A, waves)));
        return 0;
    } catch (const std::exception& e) { g_err = e.what(); return 1; }
}

}  // extern "C"
