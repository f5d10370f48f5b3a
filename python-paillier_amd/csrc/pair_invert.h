// pair_invert.h — simultaneous inversion modulo n^2 of rows in the pair form: out[i] = X[i]^-1.
// invert(c, n^2) is what EncryptedNumber.__mul__ does to the ciphertext for a negative scalar (phe/paillier.py:745-749), hence
// what __neg__ and __sub__ do.  Montgomery's trick turns `rows` inversions into ONE inversion and three products per row; here
// on uniform blocks of B consecutive rows, one block per limb group, as two walks of the kind segment_core.h keeps (the running
// product in registers, one split_mul per step):
//
//   down (pair_invert_prefix_body)  block t owns the rows t*B .. min((t+1)*B, n_rows) of X.  It stores the running products
//                                   P[r] = X[first] * ... * X[r] and the last of them as the block's total T[t]: ONE product
//                                   per row, no second pass for the totals.
//   up   (pair_invert_walk_body)    block t starts from I = Inv_up[t], the inverse of its total, and goes from its last row down
//                                   to its first:  out[r] = I * P[r-1],  I <- I * X[r];  out[first] = I.  TWO products per row.
//
// The totals of a level are the rows of the next one (X_{k+1} = T_k) until one row is left; that root is inverted on the host
// (key_setup.h host::big_invert_odd) and the up walks run from the top level down (invert_levels below: the sizes; the launches
// are phe_hip.hip phe_hip_pair_invert_dev).  Rows over all levels: n * (1 + 1/(B-1)); the first row of a block costs no product
// in either walk (the down walk starts from it, the up walk ends with out[first] = I), so a level of n rows in blocks of B runs
// 3 * (n - blocks) products.
//
// Lock step: B is a kernel argument, the same in every group of every wavefront, so the loops need no ballot.  A row at or past
// n_rows (the ragged last block) and a slot past the last block still execute every product of the wave — by the pair of 1
// (mod.e), read from a valid address — and store nothing.  Lazy bounds are those of split_mul: X0 < 2n, X1 < 3n in and out.
// No atomics, nothing passes between workgroups inside a launch.
#pragma once

#include <stdint.h>

#include <vector>

namespace phe {

struct PairInvertArgs {
    SplitConsts mod;
    const uint32_t* x;    // (n_rows, 2H) pair rows: the level's input
    uint32_t* prefix;     // down: (n_rows, 2H) running products out;  up: the same rows in (never row `last` of a block)
    uint32_t* totals;     // down: (blocks, 2H) the last running product of every block
    const uint32_t* inv;  // up: (blocks, 2H) the inverse of every block's total
    uint32_t* out;        // up: (n_rows, 2H) the inverses; must not be x or prefix
    uint64_t n_rows;      // > 0, below 2^32
    uint32_t block_rows;  // B >= 2 (1 would make every level as long as the one below)
    uint64_t blocks;      // = ceil(n_rows / B)
};

// Sizes of the levels: rows[0] = batch, rows[k + 1] = ceil(rows[k] / block[k]) down to one row; block[k] = min(B, rows[k]) (a
// level shorter than a block is one block of exactly its rows: no idle steps).  The last entry (one row: the root) has no block.
struct InvertLevels {
    std::vector<uint64_t> rows;
    std::vector<uint32_t> block;
    uint64_t upper_rows = 0;  // rows of the levels 1.. together
};
inline InvertLevels invert_levels(uint64_t batch, uint32_t B) {
    InvertLevels lv;
    lv.rows.push_back(batch);
    while (lv.rows.back() > 1) {
        const uint64_t n = lv.rows.back();
        const uint32_t b = n < B ? (uint32_t)n : B;
        lv.block.push_back(b);
        lv.rows.push_back((n + b - 1) / b);
        lv.upper_rows += lv.rows.back();
    }
    return lv;
}

template <int G, int L>
PHE_DEV void pair_invert_prefix_body(const PairInvertArgs& A, uint32_t* lds_row, uint32_t slot, uint32_t total_slots, uint32_t lane) {
    constexpr int H = G * L, S2 = 2 * H;
    const Lanes<G> ln(lane);
    const uint32_t g = ln.g;
    SplitLane<G, L> K;
    load_row<L>(K.n, A.mod.n, g);
    K.n0inv = A.mod.n0inv;
    K.rows_ = A.mod.rows;
    K.row_a = lds_row;
    K.row_c = lds_row + H;
    const uint64_t n_iter = (A.blocks + total_slots - 1) / total_slots;
    for (uint64_t it = 0; it < n_iter; ++it) {
        const uint64_t t = slot + it * (uint64_t)total_slots;
        const bool live = t < A.blocks;
        const uint64_t first = live ? t * A.block_rows : 0;  // (< n_rows for a live block: blocks = ceil(n_rows / B))
        uint32_t X0[L], X1[L], Y0[L], Y1[L];
        for (uint32_t el = 0; el < A.block_rows; ++el) {
            const uint64_t r = first + el;
            const bool mine = live && r < A.n_rows;
            const uint32_t* src = wave::reread_vptr(mine ? A.x + r * (uint64_t)S2 : A.mod.e);
            if (el == 0) {  // the running product starts AS the first row
                load_row<L>(X0, src, g);
                load_row<L>(X1, src + H, g);
            } else {
                load_row<L>(Y0, src, g);
                load_row<L>(Y1, src + H, g);
                split_mul<G, L>(X0, X1, Y0, Y1, K, ln);
            }
            if (mine) {
                store_row<L>(A.prefix + r * (uint64_t)S2, X0, g);
                store_row<L>(A.prefix + r * (uint64_t)S2 + H, X1, g);
            }
        }
        if (live) {
            store_row<L>(A.totals + t * (uint64_t)S2, X0, g);
            store_row<L>(A.totals + t * (uint64_t)S2 + H, X1, g);
        }
    }
}

template <int G, int L>
PHE_DEV void pair_invert_walk_body(const PairInvertArgs& A, uint32_t* lds_row, uint32_t slot, uint32_t total_slots, uint32_t lane) {
    constexpr int H = G * L, S2 = 2 * H;
    const Lanes<G> ln(lane);
    const uint32_t g = ln.g;
    SplitLane<G, L> K;
    load_row<L>(K.n, A.mod.n, g);
    K.n0inv = A.mod.n0inv;
    K.rows_ = A.mod.rows;
    K.row_a = lds_row;
    K.row_c = lds_row + H;
    const uint64_t n_iter = (A.blocks + total_slots - 1) / total_slots;
    for (uint64_t it = 0; it < n_iter; ++it) {
        const uint64_t t = slot + it * (uint64_t)total_slots;
        const bool live = t < A.blocks;
        const uint64_t first = live ? t * A.block_rows : 0;
        uint32_t I0[L], I1[L], Y0[L], Y1[L];
        {
            const uint32_t* src = live ? A.inv + t * (uint64_t)S2 : A.mod.e;
            load_row<L>(I0, src, g);
            load_row<L>(I1, src + H, g);
        }
        for (uint32_t el = A.block_rows; el-- > 1;) {  // from the block's last row down to its second
            const uint64_t r = first + el;
            const bool mine = live && r < A.n_rows;
            // out[r] = I * P[r - 1]
            const uint32_t* p = wave::reread_vptr(mine ? A.prefix + (r - 1) * (uint64_t)S2 : A.mod.e);
            load_row<L>(Y0, p, g);
            load_row<L>(Y1, p + H, g);
            split_mul<G, L>(Y0, Y1, I0, I1, K, ln);  // (the product lands in its first operand: P[r - 1] * I, I kept)
            if (mine) {
                store_row<L>(A.out + r * (uint64_t)S2, Y0, g);
                store_row<L>(A.out + r * (uint64_t)S2 + H, Y1, g);
            }
            // I <- I * X[r]
            const uint32_t* x = wave::reread_vptr(mine ? A.x + r * (uint64_t)S2 : A.mod.e);
            load_row<L>(Y0, x, g);
            load_row<L>(Y1, x + H, g);
            split_mul<G, L>(I0, I1, Y0, Y1, K, ln);
        }
        if (live) {  // what is left is the inverse of the first row
            store_row<L>(A.out + first * (uint64_t)S2, I0, g);
            store_row<L>(A.out + first * (uint64_t)S2 + H, I1, g);
        }
    }
}

}  // namespace phe
