// fixed_base.h — powers of ONE base by many short exponents: out[i] = mul[i] * base^e[i] (* (1 + n*m[i])), in the pair form.
// The obfuscator of an encryption need not be r^n for a fresh r of the modulus' length (phe/paillier.py:137): with h = -x^2 mod n
// and h_s = h^n mod n^2 fixed once per key, h_s^rho for a short random rho is an n-th power too (the variant of Damgard, Jurik and
// Nielsen) — the ciphertext raw_encrypt(m, r_value = h^rho mod n) returns.  The base is the same for every row, so the
// exponentiation is a fixed-base comb: with the exponent cut into T = ceil(bits / w) digits of w bits,
//     base^e = prod_t  table[t][digit_t(e)],        table[t][d] = base^(d * 2^(w t)),  1 <= d < 2^w
// — T table look-ups and pair products (5*H^2 multiply-adds each) and NO squaring, against `bits` squarings and bits/5 products of
// the windowed ladder over a full-width exponent.
//
// The table: T * (2^w - 1) pair rows, entry (t, d) at row t * (2^w - 1) + (d - 1), built once per (base, bits, w) by the host
// with the pair entry points (phe_hip.hip phe_hip_fixed_base_set) and read-only here.  Every index into it is 64-bit.
//
// One limb group owns one output row, grid-strided like segment_core.h; the running product stays in registers.  Lock step: T and
// w are kernel arguments, the same in every group of every wavefront; a zero digit multiplies by the pair of 1 (mod.e), which
// leaves the accumulator's value as it is, unless the whole wavefront has a zero digit at that position — then the trip is
// skipped by all its groups together.  A slot past the last row works on the last row again and stores nothing.
#pragma once

namespace phe {

constexpr int kFixedBaseMaxWindow = 12;  // 2^w - 1 rows per position: 4095 at the widest

struct FixedBaseArgs {
    SplitConsts mod;
    const uint32_t* table;  // (positions * (2^window - 1), 2H) pair rows
    const uint32_t* e;      // (batch, exp_limbs) exponents in 32-bit words; bits at or above exp_bits are not read
    int exp_limbs;          // >= ceil(exp_bits / 32)
    int exp_bits;           // > 0
    int window;             // 1 .. kFixedBaseMaxWindow
    int positions;          // ceil(exp_bits / window)
    const uint32_t* mul;    // the value the product starts from, per row: nullptr (1), (batch, 2H) pair rows, or — for
                            // fixed_base_pow_body<.., CONV = true> — (batch, limbs) canonical residues in 32-bit words
    const uint32_t* m;      // EXIT only: plaintexts (batch, m_limbs) folded in as 1 + n*m, or nullptr
    int m_limbs;
    uint32_t* out;          // EXIT: (batch, limbs) canonical residues in 32-bit words; else (batch, 2H) pair rows
    int limbs;              // 32-bit words of a residue row
    int chunks;             // ceil(32*limbs / (29 rows))
    uint64_t batch;         // > 0
};

// digit `t` of the exponent row e: the bits [t*w, min(t*w + w, bits)) — a window may straddle two words
PHE_DEV uint32_t fixed_base_digit(const uint32_t* e, int t, int w, int bits) {
    const int lo = t * w;
    const int width = (bits - lo < w) ? bits - lo : w;
    const int j = lo >> 5, off = lo & 31;
    uint32_t v = e[j] >> off;
    if (off + width > 32) v |= e[j + 1] << (32 - off);  // (only then: the word above the last digit is never read)
    return v & ((1u << width) - 1u);
}

// CONV: mul holds canonical residues (never nullptr then); EXIT: leave the pair form on the way out (split_exit, the exit of
// from_pair_body, with the plaintext row folded in)
template <int G, int L, bool CONV, bool EXIT>
PHE_DEV void fixed_base_pow_body(const FixedBaseArgs& A, uint32_t* lds_row, uint32_t slot, uint32_t total_slots, uint32_t lane) {
    constexpr int H = G * L, S2 = 2 * H;
    const Lanes<G> ln(lane);
    const uint32_t g = ln.g;
    SplitLane<G, L> K;
    K.n0inv = A.mod.n0inv;
    K.rows_ = A.mod.rows;
    K.row_a = lds_row;
    K.row_c = lds_row + H;
    const uint64_t per_pos = ((uint64_t)1 << A.window) - 1;
    const uint64_t n_iter = (A.batch + total_slots - 1) / total_slots;
    for (uint64_t it = 0; it < n_iter; ++it) {
        uint64_t item = slot + it * (uint64_t)total_slots;
        const bool live = item < A.batch;
        if (!live) item = A.batch - 1;
        const uint32_t* ep = A.e + item * (uint64_t)A.exp_limbs;
        load_row<L>(K.n, wave::reread_ptr(A.mod.n), g);  // (per row, so that no copy of it has to survive the exit of the row before)
        uint32_t X0[L], X1[L], Y0[L], Y1[L];
        if constexpr (CONV) {
            split_conv<G, L>(X0, X1, A.mul + item * (uint64_t)A.limbs, A.limbs, A.chunks, A.mod, K, ln);
        } else {
            const uint32_t* start = A.mul ? A.mul + item * (uint64_t)S2 : wave::reread_ptr(A.mod.e);
            load_row<L>(X0, start, g);
            load_row<L>(X1, start + H, g);
        }
        for (int t = 0; t < A.positions; ++t) {
            const uint32_t d = fixed_base_digit(ep, t, A.window, A.exp_bits);
            if (wave::ballot(d != 0u) == 0) continue;  // the whole wavefront multiplies by 1 here
            const uint32_t* src = wave::reread_vptr(d ? A.table + ((uint64_t)t * per_pos + (d - 1u)) * (uint64_t)S2 : A.mod.e);
            const uint32_t gi = wave::reread(g);
            load_row<L>(Y0, src, gi);
            load_row<L>(Y1, src + H, gi);
            split_mul<G, L>(X0, X1, Y0, Y1, K, ln);
        }
        if constexpr (EXIT) {
            // (the modulus row is loaded again for the way out, and the row number re-read: one copy of n alive from the trips
            //  through the exit makes the compiler spill it where the exit is short of registers and reload it INSIDE the trips)
            SplitLane<G, L> KX;
            load_row<L>(KX.n, wave::reread_ptr(A.mod.n), wave::reread(g));
            KX.n0inv = A.mod.n0inv;
            KX.rows_ = A.mod.rows;
            KX.row_a = lds_row;
            KX.row_c = lds_row + H;
            const uint64_t row = wave::reread64(item);
            const uint32_t* mp = A.m ? A.m + row * (uint64_t)A.m_limbs : nullptr;
            split_exit<G, L>(A.out + row * (uint64_t)A.limbs, A.limbs, X0, X1, mp, A.m_limbs, A.mod, KX, ln, live);
        } else if (live) {
            uint32_t* dst = A.out + item * (uint64_t)S2;
            store_row<L>(dst, X0, g);
            store_row<L>(dst + H, X1, g);
        }
    }
}

}  // namespace phe
