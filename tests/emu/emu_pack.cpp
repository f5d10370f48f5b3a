// TEST INFRASTRUCTURE — the packing device body (csrc/segment_core.h segment_pack_body) compiled for the CPU on the wave
// emulator (wave_emu.h), beside emu_segment.cpp and emu_scan.cpp: tests/test_pack.py builds this file into a library of its own.
#include <stdint.h>

#include "wave_emu.h"
// clang-format off
#include "../../python-paillier_amd/csrc/mont_core.h"
#include "../../python-paillier_amd/csrc/split_core.h"
#include "../../python-paillier_amd/csrc/segment_core.h"
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
#define DISPATCH_PACK(G_, L_, CALL)                                                   \
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

// `waves` wavefronts of 64/G limb groups stride over the tasks like the GPU grid does
template <int G, int L, bool PAIR>
static void run_pack(PackArgs A, int waves) {
    constexpr int S2 = 2 * G * L, kPer = 64 / G;
    const uint32_t total = (uint32_t)(kPer * waves);
    for (int w = 0; w < waves; ++w) {
        std::vector<uint32_t> lds(kPer * (S2 + kLdsPad + 1));
        wave::run_wave([&](uint32_t lane) {
            const uint32_t grp = lane / G;
            segment_pack_body<G, L, PAIR>(A, lds.data() + grp * (S2 + kLdsPad + 1), (uint32_t)w * kPer + grp, total, lane);
        });
    }
}

extern "C" {

const char* emu_pack_last_error(void) { return g_err.c_str(); }

// phe_hip_segment_pack_dev on the geometry build_public picks for n (group = 0: rung 0, whose rows the pair form has; group > 0:
// the wider rung of that group width, if it shares the rows' limb count).  gl[0..2] = G, L, words of a pair row.  rc 2: no such
// geometry, rc 3: the arguments the entry point refuses.  out == nullptr: only report the geometry.
int emu_segment_pack(const uint32_t* n, int n_limbs, int group, const uint32_t* rows, int rows_are_pair, uint64_t n_rows,
                     uint32_t slots, uint32_t slot_bits, uint32_t* out, uint64_t tasks, int waves, int* gl) {
    try {
        const host::PublicPlan P0 = host::build_public(n, n_limbs, 0);
        if (!P0.nsplit.G) return 2;
        host::SplitPack M = P0.nsplit;
        if (group > 0) {
            M = host::build_public(n, n_limbs, group).nsplit;
            if (M.G == 0 || M.H != P0.nsplit.H || M.rows != M.H) return 2;
        }
        if (gl) { gl[0] = M.G; gl[1] = M.L; gl[2] = 2 * P0.nsplit.H; }
        if (!out || tasks == 0) return 0;
        if (!rows || slots == 0 || slot_bits == 0 || tasks != (n_rows + slots - 1) / slots) return 3;
        PackArgs A;
        memset(&A, 0, sizeof A);
        A.mod = split_consts_of(M);
        A.rows = rows;
        A.rows_are_pair = rows_are_pair;
        A.limbs = P0.s2;
        A.chunks = chunks_for(P0.s2, M.rows);
        A.n_rows = n_rows;
        A.slots = slots;
        A.slot_bits = slot_bits;
        A.out = out;
        A.tasks = tasks;
        if (waves < 1) waves = 1;
        if (rows_are_pair) { DISPATCH_PACK(M.G, M.L, (run_pack<GG, LL, true>(A, waves))); }
        else { DISPATCH_PACK(M.G, M.L, (run_pack<GG, LL, false>(A, waves))); }
        return 0;
    } catch (const std::exception& e) { g_err = e.what(); return 1; }
}

}  // extern "C"
