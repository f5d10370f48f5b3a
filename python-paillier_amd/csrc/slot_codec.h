// slot_codec.h — the slot codec of packed plaintexts: int64 values <-> plaintext rows mod n.
//
// Conventions (those of EncryptedVector.pack / PaillierPrivateKey._unpack_plain, phe/ciphertext.py, phe/keys.py):
//   S = slots, B = slot_bits (1 <= B <= 64 here), S*B <= max_int.bit_length() - 1, half = 2^(B-1),
//   offset = sum_{j < S} half * 2^(B j).  Row b holds the values x[b*S + j]; values past the end count as 0.
//   pack:   u = sum_j (x_j + half) 2^(B j)   (pure bit placement: every x_j + half is a B-bit field, no carries),
//           v = u - offset, m = v if v >= 0 else v + n.
//   unpack: v = m if m <= max_int, m - n if m >= n - max_int, otherwise status 1 (the overflow gap of EncodedNumber.decode);
//           u = v + offset, status 2 unless 0 <= u < 2^(S B); x_j = ((u >> B j) & (2^B - 1)) - half.
//
// Lane mapping.  A row of n_limbs 32-bit words belongs to a limb group of G lanes; lane g keeps the K consecutive words
// [g K, (g+1) K) in registers, G K >= n_limbs (words at or above n_limbs are zero).  Consecutive lanes therefore load and store
// consecutive K-word pieces of a row: one contiguous span per group.  Borrows and carries cross the lanes by the look-ahead of
// mont_core.h (group_carry_in: two ballots and one 64-bit addition per chain), never by a lane-to-lane ripple.
//
// These bodies move bit fields: per row one subtraction and one conditional addition (pack), two comparisons and one addition
// (unpack).  They are bound by memory, not by arithmetic.
//
// Written only against the `wave::` primitives (lane-local C++, ballot, grp_down1) and mont_core.h's look-ahead, so that
// tests/emu/wave_emu.h runs them as they are.  Include after wave_gfx950.h (or wave_emu.h) and mont_core.h.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

namespace phe {

// constant rows of G*K words each (zero- or sign-extended above n_limbs), made by host::slot_const_rows
struct SlotConsts {
    const uint32_t* offset;      // half in every slot
    const uint32_t* n;
    const uint32_t* max_int;
    const uint32_t* neg_low;     // n - max_int: the least plaintext that stands for a negative number
    const uint32_t* offset_neg;  // offset - n modulo 2^(32 G K)
};
struct SlotPackArgs {
    SlotConsts k;
    const int64_t* values;
    uint64_t count;  // values; those at or beyond count are 0
    uint32_t slots, slot_bits;
    uint32_t* m_rows;  // (rows, n_limbs)
    uint64_t rows;
    int n_limbs;
};
struct SlotUnpackArgs {
    SlotConsts k;
    const uint32_t* m_rows;  // (rows, n_limbs)
    uint64_t rows;
    uint32_t slots, slot_bits;
    int64_t* values;  // rows * slots
    uint8_t* status;  // rows
    int n_limbs;
};

// d = a - b over the G*K words of a group; returns the borrow out of the top word (1: a < b)
template <int G, int K>
PHE_DEV uint32_t group_sub_words(uint32_t (&d)[K], const uint32_t (&a)[K], const uint32_t (&b)[K], const Lanes<G>& ln) {
    uint32_t br = 0, nz = 0;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const uint64_t v = (uint64_t)a[k] - b[k] - br;
        d[k] = (uint32_t)v;
        br = (uint32_t)(v >> 63);
        nz |= d[k];
    }
    // a lane that borrows has a non-zero difference: gen and prop are disjoint
    const uint64_t gen = wave::ballot(br != 0);
    const uint64_t prop = wave::ballot(nz == 0);
    uint64_t out_top;
    const uint64_t bin = group_carry_in<G>(gen, prop, out_top);
    uint32_t bi = lane_bit(bin, ln.lane);
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const uint64_t v = (uint64_t)d[k] - bi;
        d[k] = (uint32_t)v;
        bi = (uint32_t)(v >> 63);
    }
    return group_top_bit<G>(out_top, ln.lane);
}

// s = a + b modulo 2^(32 G K) over the words of a group
template <int G, int K>
PHE_DEV void group_add_words(uint32_t (&s)[K], const uint32_t (&a)[K], const uint32_t (&b)[K], const Lanes<G>& ln) {
    uint32_t c = 0, ones = 0xffffffffu;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const uint64_t v = (uint64_t)a[k] + b[k] + c;
        s[k] = (uint32_t)v;
        c = (uint32_t)(v >> 32);
        ones &= s[k];
    }
    // a lane that carries out has a sum of at most 2^(32 K) - 2: gen and prop are disjoint
    const uint64_t gen = wave::ballot(c != 0);
    const uint64_t prop = wave::ballot(ones == 0xffffffffu);
    uint64_t out_top;
    const uint64_t cin = group_carry_in<G>(gen, prop, out_top);
    uint32_t ci = lane_bit(cin, ln.lane);
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const uint64_t v = (uint64_t)s[k] + ci;
        s[k] = (uint32_t)v;
        ci = (uint32_t)(v >> 32);
    }
}

template <int K>
PHE_DEV void slot_load_row(uint32_t (&x)[K], const uint32_t* p, uint32_t g) {
#pragma unroll
    for (int k = 0; k < K; ++k) x[k] = p[g * K + k];
}

// values -> plaintext rows.  `group` of `total` limb groups strides over the rows; every lane of a wave makes the same number
// of trips (the ballots need all 64 lanes), rows beyond the end are computed on zeros and not stored.
template <int G, int K>
PHE_DEV void slots_pack_body(const SlotPackArgs& A, uint32_t group, uint32_t total, uint32_t lane) {
    const Lanes<G> ln(lane);
    const uint32_t S = A.slots, B = A.slot_bits;
    const uint64_t half = 1ull << (B - 1), mask = B == 64 ? ~0ull : (1ull << B) - 1ull;
    const uint32_t top_bit = S * B;  // <= 32 n_limbs
    uint32_t off[K], nn[K];
    slot_load_row<K>(off, A.k.offset, ln.g);
    slot_load_row<K>(nn, A.k.n, ln.g);
    for (uint64_t first = 0; first < A.rows; first += total) {
        const uint64_t row = first + group;
        const bool active = row < A.rows;
        uint32_t u[K];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const uint32_t base = 32u * (ln.g * K + k);  // the word holds bits [base, base + 32) of u
            uint32_t w = 0;
            if (active && base < top_bit) {
                for (uint32_t j = base / B; j < S && B * j < base + 32u; ++j) {  // the slots that overlap the word
                    const uint64_t idx = row * S + j;
                    const int64_t x = idx < A.count ? A.values[idx] : 0;
                    const uint64_t y = ((uint64_t)x + half) & mask;
                    const int sh = (int)(B * j) - (int)base;  // in (-B, 32)
                    w |= sh >= 0 ? (uint32_t)(y << sh) : (uint32_t)(y >> -sh);
                }
            }
            u[k] = w;
        }
        uint32_t d[K], add[K], m[K];
        const uint32_t neg = group_sub_words<G, K>(d, u, off, ln);  // v = u - offset; a final borrow: v < 0
#pragma unroll
        for (int k = 0; k < K; ++k) add[k] = neg ? nn[k] : 0u;
        group_add_words<G, K>(m, d, add, ln);  // v + n modulo 2^(32 G K): the carry out cancels the borrow
        if (active) {
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const uint32_t word = ln.g * K + k;
                if ((int)word < A.n_limbs) A.m_rows[row * (uint64_t)A.n_limbs + word] = m[k];
            }
        }
    }
}

// plaintext rows -> values and one status byte per row (0: fine, 1: m in the overflow gap, 2: u outside [0, 2^(S B))).
// The values of a row with a non-zero status are unspecified.
template <int G, int K>
PHE_DEV void slots_unpack_body(const SlotUnpackArgs& A, uint32_t group, uint32_t total, uint32_t lane) {
    const Lanes<G> ln(lane);
    const uint32_t S = A.slots, B = A.slot_bits;
    const uint64_t half = 1ull << (B - 1), mask = B == 64 ? ~0ull : (1ull << B) - 1ull;
    const uint32_t top_bit = S * B;
    uint64_t group_lanes = ~0ull;
    if constexpr (G < 64) group_lanes = ((1ull << G) - 1ull) << (ln.lane & ~(uint32_t)(G - 1));
    uint32_t off[K], offn[K], mx[K], lo[K];
    slot_load_row<K>(off, A.k.offset, ln.g);
    slot_load_row<K>(offn, A.k.offset_neg, ln.g);
    slot_load_row<K>(mx, A.k.max_int, ln.g);
    slot_load_row<K>(lo, A.k.neg_low, ln.g);
    for (uint64_t first = 0; first < A.rows; first += total) {
        const uint64_t row = first + group;
        const bool active = row < A.rows;
        uint32_t m[K], t[K], add[K], u[K];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const uint32_t word = ln.g * K + k;
            m[k] = (active && (int)word < A.n_limbs) ? A.m_rows[row * (uint64_t)A.n_limbs + word] : 0u;
        }
        const uint32_t above = group_sub_words<G, K>(t, mx, m, ln);  // max_int - m borrows: m > max_int
        const uint32_t below = group_sub_words<G, K>(t, m, lo, ln);  // m - (n - max_int) borrows: m < n - max_int
        // u = v + offset in one chain: m + offset, or m + (offset - n) modulo 2^(32 G K) for a negative number.  A result
        // below zero wraps to above 2^(32 G K) - n: its top bits are set and it fails the range test like one that is too large.
#pragma unroll
        for (int k = 0; k < K; ++k) add[k] = above ? offn[k] : off[k];
        group_add_words<G, K>(u, m, add, ln);
        uint32_t high = 0;  // the bits of u at or above S*B
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const uint32_t base = 32u * (ln.g * K + k);
            if (base >= top_bit) high |= u[k];
            else if (base + 32u > top_bit) high |= u[k] >> (top_bit - base);
        }
        const bool spill = (wave::ballot(high != 0) & group_lanes) != 0;
        // a slot starts in one word and may reach into the next two: the first two words of the lane above
        uint32_t e[K + 2];
#pragma unroll
        for (int k = 0; k < K; ++k) e[k] = u[k];
        e[K] = wave::grp_down1<G>(u[0], ln);
        if constexpr (K >= 2) e[K + 1] = wave::grp_down1<G>(u[1], ln);
        else e[K + 1] = wave::grp_down1<G>(e[K], ln);
        if (active) {
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const uint32_t base = 32u * (ln.g * K + k);
                if (base < top_bit) {
                    for (uint32_t j = (base + B - 1u) / B; j < S && B * j < base + 32u; ++j) {  // the slots that START in the word
                        const uint32_t o = B * j - base;  // in [0, 32)
                        uint64_t v = ((((uint64_t)e[k + 1]) << 32) | e[k]) >> o;
                        if (o) v |= (uint64_t)e[k + 2] << (64u - o);
                        A.values[row * S + j] = (int64_t)((v & mask) - half);
                    }
                }
            }
            if (ln.g == 0) A.status[row] = (above && below) ? (uint8_t)1 : spill ? (uint8_t)2 : (uint8_t)0;
        }
    }
}

namespace host {

// (G, K) for rows of n_limbs words: at most 4 words per lane up to 8192 bits; false: no kernel for that width
inline bool slot_geometry(int n_limbs, int& G, int& K) {
    if (n_limbs < 1 || n_limbs > 512) return false;
    if (n_limbs <= 16) { G = 16; K = 1; }
    else if (n_limbs <= 32) { G = 16; K = 2; }
    else if (n_limbs <= 64) { G = 16; K = 4; }
    else if (n_limbs <= 128) { G = 64; K = 2; }
    else if (n_limbs <= 256) { G = 64; K = 4; }
    else { G = 64; K = 8; }
    return true;
}

// max_int = n // 3 - 1 (phe/paillier.py:90), n_limbs words
inline std::vector<uint32_t> slot_max_int(const uint32_t* n, int n_limbs) {
    std::vector<uint32_t> q((size_t)n_limbs);
    uint64_t rem = 0;
    for (int i = n_limbs - 1; i >= 0; --i) {
        const uint64_t cur = (rem << 32) | n[i];
        q[(size_t)i] = (uint32_t)(cur / 3u);
        rem = cur % 3u;
    }
    for (int i = 0; i < n_limbs; ++i)
        if (q[(size_t)i]-- != 0u) break;
    return q;
}

// the most bits S*B may take: max_int.bit_length() - 1 (0 for a degenerate key)
inline int slot_capacity_bits(const uint32_t* n, int n_limbs) {
    const std::vector<uint32_t> mx = slot_max_int(n, n_limbs);
    for (int i = n_limbs - 1; i >= 0; --i)
        if (mx[(size_t)i]) {
            int b = 32;
            while (!(mx[(size_t)i] >> (b - 1))) --b;
            return 32 * i + b - 1;
        }
    return 0;
}

// the five rows of SlotConsts, `width` (>= n_limbs) words each: offset | n | max_int | n - max_int | offset - n
inline std::vector<uint32_t> slot_const_rows(const uint32_t* n, int n_limbs, uint32_t slots, uint32_t slot_bits, int width) {
    const size_t W = (size_t)width;
    std::vector<uint32_t> rows(5 * W, 0u);
    uint32_t *off = rows.data(), *nn = off + W, *mx = nn + W, *lo = mx + W, *offn = lo + W;
    for (uint32_t j = 0; j < slots; ++j) {
        const uint64_t bit = (uint64_t)slot_bits * j + slot_bits - 1u;
        if (bit / 32u < W) off[bit / 32u] |= 1u << (bit % 32u);
    }
    const std::vector<uint32_t> m = slot_max_int(n, n_limbs);
    for (int i = 0; i < n_limbs; ++i) { nn[i] = n[i]; mx[i] = m[(size_t)i]; }
    uint64_t br = 0;
    for (size_t i = 0; i < W; ++i) {
        const uint64_t v = (uint64_t)nn[i] - mx[i] - br;
        lo[i] = (uint32_t)v;
        br = v >> 63;
    }
    br = 0;
    for (size_t i = 0; i < W; ++i) {
        const uint64_t v = (uint64_t)off[i] - nn[i] - br;
        offn[i] = (uint32_t)v;
        br = v >> 63;
    }
    return rows;
}

}  // namespace host

}  // namespace phe
