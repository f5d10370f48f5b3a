// TEST INFRASTRUCTURE — the two walks of the simultaneous inversion on pair rows (csrc/pair_invert.h) compiled for the CPU on the
// wave emulator (wave_emu.h), beside emu_scan.cpp: tests/test_pair_invert.py builds this file into a library of its own.  The
// levels are those of the library (invert_levels), the root leaves and enters the form by the library's conversions
// (from_pair_body / to_pair_body) and is inverted by the library's host routine (host::big_invert_odd).
#include <stdint.h>

#include "wave_emu.h"
// clang-format off
#include "../../python-paillier_amd/csrc/mont_core.h"
#include "../../python-paillier_amd/csrc/split_core.h"
#include "../../python-paillier_amd/csrc/pair_invert.h"
#include "../../python-paillier_amd/csrc/key_setup.h"
// clang-format on

#include <string.h>

#include <algorithm>
#include <stdexcept>
#include <string>
#include <vector>

using namespace phe;

static thread_local std::string g_err;

// geometries of the pair rungs of the golden keys (the list of emu_scan.cpp)
#define DISPATCH_INV(G_, L_, CALL)                                                    \
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

// `waves` wavefronts of 64/G limb groups stride over the work like the GPU grid does; which: 0 the running products, 1 the walk
// back, 2 pair -> words, 3 words -> pair, 4 pair * pair
template <int G, int L>
static void run_waves(int which, const PairInvertArgs* I, const PairArgs* C, int waves) {
    constexpr int S2 = 2 * G * L, kPer = 64 / G;
    const uint32_t total = (uint32_t)(kPer * waves);
    for (int w = 0; w < waves; ++w) {
        std::vector<uint32_t> lds(kPer * (S2 + kLdsPad + 1));
        wave::run_wave([&](uint32_t lane) {
            const uint32_t grp = lane / G;
            uint32_t* row = lds.data() + grp * (S2 + kLdsPad + 1);
            const uint32_t slot = (uint32_t)w * kPer + grp;
            switch (which) {
                case 0: pair_invert_prefix_body<G, L>(*I, row, slot, total, lane); break;
                case 1: pair_invert_walk_body<G, L>(*I, row, slot, total, lane); break;
                case 2: from_pair_body<G, L>(*C, row, slot, total, lane); break;
                case 3: to_pair_body<G, L>(*C, row, slot, total, lane); break;
                default: pair_mul_body<G, L>(*C, row, slot, total, lane); break;
            }
        });
    }
}

struct Geometry {
    host::PublicPlan P0;
    host::SplitPack M;
    bool ok = false;
};
// the geometry build_public picks for n (group = 0: rung 0, whose rows the pair form has; group > 0: the wider rung of that
// group width, if it shares the rows' limb count)
static Geometry geometry_of(const uint32_t* n, int n_limbs, int group) {
    Geometry g;
    g.P0 = host::build_public(n, n_limbs, 0);
    if (!g.P0.nsplit.G) return g;
    g.M = g.P0.nsplit;
    if (group > 0) {
        g.M = host::build_public(n, n_limbs, group).nsplit;
        if (g.M.G == 0 || g.M.H != g.P0.nsplit.H || g.M.rows != g.M.H) return g;
    }
    g.ok = true;
    return g;
}

static void convert(const Geometry& g, bool into_form, const uint32_t* src, uint32_t* dst, uint64_t batch, int waves) {
    PairArgs A;
    memset(&A, 0, sizeof A);
    A.mod = split_consts_of(g.M);
    A.a = src;
    A.out = dst;
    A.limbs = g.P0.s2;
    A.chunks = chunks_for(g.P0.s2, g.M.rows);
    A.batch = batch;
    DISPATCH_INV(g.M.G, g.M.L, (run_waves<GG, LL>(into_form ? 3 : 2, nullptr, &A, waves)));
}

extern "C" {

const char* emu_inv_last_error(void) { return g_err.c_str(); }

// multiply-add lane-operations this library's bodies executed since the last reset (wave_emu.h mad_counter)
uint64_t emu_inv_mad_count(int reset) {
    const uint64_t v = wave::mad_counter();
    if (reset) wave::mad_counter() = 0;
    return v;
}

// gl[0..2] = G, L, words of a pair row.  rc 2: no such geometry
int emu_inv_geometry(const uint32_t* n, int n_limbs, int group, int* gl) {
    try {
        const Geometry g = geometry_of(n, n_limbs, group);
        if (!g.ok) return 2;
        gl[0] = g.M.G; gl[1] = g.M.L; gl[2] = 2 * g.P0.nsplit.H;
        return 0;
    } catch (const std::exception& e) { g_err = e.what(); return 1; }
}

// out[i] = a[i] * b[i] on pair rows: ONE pair product per row on one wavefront (what the multiply-add counts are measured in)
int emu_inv_pair_mul(const uint32_t* n, int n_limbs, int group, const uint32_t* a, const uint32_t* b, uint32_t* out, uint64_t batch) {
    try {
        const Geometry g = geometry_of(n, n_limbs, group);
        if (!g.ok) return 2;
        PairArgs A;
        memset(&A, 0, sizeof A);
        A.mod = split_consts_of(g.M);
        A.a = a; A.b = b; A.out = out;
        A.b_stride = (size_t)(2 * g.M.H);
        A.batch = batch;
        DISPATCH_INV(g.M.G, g.M.L, (run_waves<GG, LL>(4, nullptr, &A, 1)));
        return 0;
    } catch (const std::exception& e) { g_err = e.what(); return 1; }
}

// pair_invert_walk_body alone over GIVEN rows: out[r] for the rows of ceil(n_rows / block_rows) blocks from x, prefix and inv
int emu_pair_invert_walk(const uint32_t* n, int n_limbs, int group, const uint32_t* x, const uint32_t* prefix, const uint32_t* inv,
                         uint32_t* out, uint64_t n_rows, uint32_t block_rows, int waves) {
    try {
        const Geometry g = geometry_of(n, n_limbs, group);
        if (!g.ok) return 2;
        PairInvertArgs A;
        memset(&A, 0, sizeof A);
        A.mod = split_consts_of(g.M);
        A.x = x;
        A.prefix = const_cast<uint32_t*>(prefix);
        A.inv = inv;
        A.out = out;
        A.n_rows = n_rows;
        A.block_rows = block_rows;
        A.blocks = (n_rows + block_rows - 1) / block_rows;
        DISPATCH_INV(g.M.G, g.M.L, (run_waves<GG, LL>(1, &A, nullptr, std::max(1, waves))));
        return 0;
    } catch (const std::exception& e) { g_err = e.what(); return 1; }
}

// phe_hip_pair_invert_dev: pair_out[i] = pair_in[i]^-1 over the levels of invert_levels(batch, block_rows).  rc 3: a row is not a
// unit, *bad_index the first such row.  *conversion_mads: the multiply-adds of the root's way out of the form and back into it
// (their number depends on the root's value: the exit subtracts as often as the value needs).
int emu_pair_invert(const uint32_t* n, int n_limbs, int group, const uint32_t* pair_in, uint32_t* pair_out, uint64_t batch,
                    uint32_t block_rows, int waves, uint64_t* bad_index, uint64_t* conversion_mads) {
    try {
        const Geometry g = geometry_of(n, n_limbs, group);
        if (!g.ok) return 2;
        if (batch == 0) return 0;
        if (block_rows < 2) throw std::invalid_argument("block_rows must be at least 2");
        waves = std::max(1, waves);
        const size_t w = (size_t)2 * g.P0.nsplit.H, s2 = (size_t)g.P0.s2;
        const InvertLevels lv = invert_levels(batch, block_rows);
        const size_t top = lv.rows.size() - 1;
        // level k: input rows, running products, inverses (level 0: the caller's rows)
        std::vector<std::vector<uint32_t>> Xs(top + 1), Ps(top + 1), Is(top + 1);
        std::vector<const uint32_t*> X(top + 1);
        std::vector<uint32_t*> I(top + 1);
        for (size_t k = 0; k <= top; ++k) {
            Ps[k].assign(lv.rows[k] * w, 0u);
            if (k) { Xs[k].assign(lv.rows[k] * w, 0u); Is[k].assign(lv.rows[k] * w, 0u); }
            X[k] = k ? Xs[k].data() : pair_in;
            I[k] = k ? Is[k].data() : pair_out;
        }
        auto walk = [&](size_t k, bool up) {
            PairInvertArgs A;
            memset(&A, 0, sizeof A);
            A.mod = split_consts_of(g.M);
            A.x = X[k];
            A.prefix = Ps[k].data();
            A.totals = Xs[k + 1].data();
            A.inv = I[k + 1];
            A.out = I[k];
            A.n_rows = lv.rows[k];
            A.block_rows = lv.block[k];
            A.blocks = lv.rows[k + 1];
            DISPATCH_INV(g.M.G, g.M.L, (run_waves<GG, LL>(up ? 1 : 0, &A, nullptr, waves)));
        };
        for (size_t k = 0; k < top; ++k) walk(k, false);
        host::Big root(s2, 0u), rinv;
        uint64_t before = wave::mad_counter();
        convert(g, false, X[top], root.data(), 1, 1);
        uint64_t conversions = wave::mad_counter() - before;
        if (!host::big_invert_odd(root, g.P0.nsq32, rinv)) {
            std::vector<uint32_t> words(batch * s2);
            convert(g, false, pair_in, words.data(), batch, waves);
            for (uint64_t i = 0; i < batch; ++i) {
                host::Big x(words.begin() + (long)(i * s2), words.begin() + (long)((i + 1) * s2)), tmp;
                if (!host::big_invert_odd(x, g.P0.nsq32, tmp)) {
                    if (bad_index) *bad_index = i;
                    return 3;
                }
            }
            throw std::runtime_error("the root has no inverse although every row is a unit");
        }
        rinv.resize(s2, 0u);
        before = wave::mad_counter();
        convert(g, true, rinv.data(), I[top], 1, 1);
        conversions += wave::mad_counter() - before;
        if (conversion_mads) *conversion_mads = conversions;
        for (size_t k = top; k-- > 0;) walk(k, true);
        return 0;
    } catch (const std::exception& e) { g_err = e.what(); return 1; }
}

}  // extern "C"
