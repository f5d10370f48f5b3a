// TEST INFRASTRUCTURE — the fixed-base comb body (csrc/fixed_base.h fixed_base_pow_body) compiled for the CPU on the wave emulator
// (wave_emu.h), beside emu_segment.cpp and emu_pack.cpp: tests/test_short_obfuscators.py builds this file into a library of its
// own.  The table comes from the caller (pair rows made of Python integers through emu_pair_op).
#include <stdint.h>

#include "wave_emu.h"
// clang-format off
#include "../../python-paillier_amd/csrc/mont_core.h"
#include "../../python-paillier_amd/csrc/split_core.h"
#include "../../python-paillier_amd/csrc/fixed_base.h"
#include "../../python-paillier_amd/csrc/key_setup.h"
// clang-format on

#include <string.h>

#include <algorithm>
#include <stdexcept>
#include <string>
#include <vector>

using namespace phe;

static thread_local std::string g_err;

// geometries of the pair rungs of the golden keys (the list of emu_segment.cpp)
#define DISPATCH_FB(G_, L_, CALL)                                                     \
    switch ((G_) * 100 + (L_)) {                                                      \
        case 6401: { constexpr int GG = 64, LL = 1; CALL; break; }                    \
        case 6402: { constexpr int GG = 64, LL = 2; CALL; break; }                    \
        case 6403: { constexpr int GG = 64, LL = 3; CALL; break; }                    \
        case 1603: { constexpr int GG = 16, LL = 3; CALL; break; }                    \
        case 1605: { constexpr int GG = 16, LL = 5; CALL; break; }                    \
        case 1607: { constexpr int GG = 16, LL = 7; CALL; break; }                    \
        case 1609: { constexpr int GG = 16, LL = 9; CALL; break; }                    \
        case 118: { constexpr int GG = 1, LL = 18; CALL; break; }                     \
        case 209: { constexpr int GG = 2, LL = 9; CALL; break; }                      \
        case 218: { constexpr int GG = 2, LL = 18; CALL; break; }                     \
        case 227: { constexpr int GG = 2, LL = 27; CALL; break; }                     \
        case 405: { constexpr int GG = 4, LL = 5; CALL; break; }                      \
        case 409: { constexpr int GG = 4, LL = 9; CALL; break; }                      \
        case 414: { constexpr int GG = 4, LL = 14; CALL; break; }                     \
        case 418: { constexpr int GG = 4, LL = 18; CALL; break; }                     \
        case 427: { constexpr int GG = 4, LL = 27; CALL; break; }                     \
        case 803: { constexpr int GG = 8, LL = 3; CALL; break; }                      \
        case 805: { constexpr int GG = 8, LL = 5; CALL; break; }                      \
        case 807: { constexpr int GG = 8, LL = 7; CALL; break; }                      \
        case 809: { constexpr int GG = 8, LL = 9; CALL; break; }                      \
        case 814: { constexpr int GG = 8, LL = 14; CALL; break; }                     \
        default: throw std::invalid_argument("unsupported split geometry");           \
    }

static SplitConsts split_consts_of(const host::SplitPack& m) {
    SplitConsts c;
    c.nbar = c.kx = nullptr;
    c.n = m.n.data(); c.r1 = m.r1.data();
    c.e = m.e.data(); c.conv = m.conv.data(); c.nsq = m.nsq.data(); c.n0inv = m.n0inv; c.rows = m.rows;
    return c;
}

static int chunks_for(int limbs32, int H) { return std::max(1, (32 * limbs32 + 29 * H - 1) / (29 * H)); }

// `waves` wavefronts of 64/G limb groups stride over the rows like the GPU grid does
template <int G, int L, bool CONV, bool EXIT>
static void run_fb(FixedBaseArgs A, int waves) {
    constexpr int S2 = 2 * G * L, kPer = 64 / G;
    const uint32_t total = (uint32_t)(kPer * waves);
    for (int w = 0; w < waves; ++w) {
        std::vector<uint32_t> lds(kPer * (S2 + kLdsPad + 1));
        wave::run_wave([&](uint32_t lane) {
            const uint32_t grp = lane / G;
            fixed_base_pow_body<G, L, CONV, EXIT>(A, lds.data() + grp * (S2 + kLdsPad + 1), (uint32_t)w * kPer + grp, total, lane);
        });
    }
}

extern "C" {

const char* emu_fixed_base_last_error(void) { return g_err.c_str(); }

// phe_hip_fixed_base_pow_dev on the geometry build_public picks for n (group = 0: rung 0, whose rows the pair form has; group > 0:
// the wider rung of that group width, if it shares the rows' limb count) over the caller's table of
// ceil(exp_bits / window) * (2^window - 1) pair rows.  gl[0..2] = G, L, words of a pair row.  rc 2: no such geometry, rc 3: the
// arguments the entry point refuses.  out == nullptr: only report the geometry.
int emu_fixed_base_pow(const uint32_t* n, int n_limbs, int group, const uint32_t* table, int exp_bits, int window, const uint32_t* e,
                       int exp_limbs, const uint32_t* mul, int mul_is_pair, const uint32_t* m, uint32_t* out, int out_is_pair,
                       uint64_t batch, int waves, int* gl) {
    try {
        const host::PublicPlan P0 = host::build_public(n, n_limbs, 0);
        if (!P0.nsplit.G) return 2;
        host::SplitPack M = P0.nsplit;
        if (group > 0) {
            M = host::build_public(n, n_limbs, group).nsplit;
            if (M.G == 0 || M.H != P0.nsplit.H || M.rows != M.H) return 2;
        }
        if (gl) { gl[0] = M.G; gl[1] = M.L; gl[2] = 2 * P0.nsplit.H; }
        if (!out || batch == 0) return 0;
        if (!table || !e || exp_bits < 1 || window < 1 || window > kFixedBaseMaxWindow || window > exp_bits ||
            exp_limbs != (exp_bits + 31) / 32 || (m && out_is_pair))
            return 3;
        FixedBaseArgs A;
        memset(&A, 0, sizeof A);
        A.mod = split_consts_of(M);
        A.table = table;
        A.e = e;
        A.exp_limbs = exp_limbs;
        A.exp_bits = exp_bits;
        A.window = window;
        A.positions = (exp_bits + window - 1) / window;
        A.mul = mul;
        A.m = m;
        A.m_limbs = P0.s1;
        A.out = out;
        A.limbs = P0.s2;
        A.chunks = chunks_for(P0.s2, M.rows);
        A.batch = batch;
        if (waves < 1) waves = 1;
        const bool conv = mul && !mul_is_pair;
        if (conv && !out_is_pair) { DISPATCH_FB(M.G, M.L, (run_fb<GG, LL, true, true>(A, waves))); }
        else if (conv) { DISPATCH_FB(M.G, M.L, (run_fb<GG, LL, true, false>(A, waves))); }
        else if (!out_is_pair) { DISPATCH_FB(M.G, M.L, (run_fb<GG, LL, false, true>(A, waves))); }
        else { DISPATCH_FB(M.G, M.L, (run_fb<GG, LL, false, false>(A, waves))); }
        return 0;
    } catch (const std::exception& e) { g_err = e.what(); return 1; }
}

}  // extern "C"
