// value_codec.h — the value codec of plain batches: int64 / uint64 / float64 values <-> plaintext rows mod n, one value per row.
//
// Conventions (those of EncodedNumber.encode / decode, phe/encoding.py:110-233, with BASE = 16):
//   a value is (-1)^neg * mag * 16^e with mag < 2^64; its plaintext is m = mag if mag == 0 or the value is not negative, else
//   n - mag.  The key has max_int >= 2^64 (the entry points refuse others), so no magnitude needs a range check.
//   encode, by `kind`:
//     0  int64:   mag = |x| (two's complement: -2^63 gives 2^63), e = 0
//     1  uint64:  mag = x, e = 0
//     2  float64 at its natural exponent (what np.frexp gives, as bit operations): sign, E (11 bits), frac (52 bits);
//        E = 0x7ff: status 1; E = 0, frac = 0: mag 0, e = -14; E = 0: s = 53 - bitlength(frac), imant = frac << s,
//        lsb = -1074 - s; otherwise imant = frac | 2^52, lsb = E - 1075; e = floor(lsb / 4), mag = imant << (lsb - 4 e) < 2^56
//     3  float64 under a precision, at the exponent e the caller gives: r = rint(x * 2^(-4 e)), ties to even (the scaling by
//        a power of two is exact); not finite: status 1; |r| >= 2^62: status 2 (the host encodes that batch); mag = |r|
//   decode: m >= n: status 3 (corrupted); m <= max_int: v = m; m >= n - max_int: v = m - n; in between: status 1 (the overflow
//     gap); |v| >= 2^64: status 2 (the host decodes that row).  kind 0: out = v as int64, outside [-2^63, 2^63): status 2.
//     kind 1: out = +-(double)|v| * 2^(4 exps[row]) — the conversion rounds to nearest even, the scaling is exact for
//     -240 <= exps[row] < 0 (the caller takes this route for those only).  The value of a row with a non-zero status is
//     unspecified.
//
// Lane mapping: that of slot_codec.h — a limb group of G lanes owns a row, lane g keeps the K consecutive words [g K, (g+1) K).
// Where K divides n_limbs (every compiled width but odd toy keys) a lane's piece moves as ONE access of 4 K bytes, so that a
// group reads or writes its row as one contiguous span of 16-byte (K = 4) or 8-byte (K = 2) pieces.  The 8 bytes of a value are
// read by every lane of its group (one address: a broadcast); exponent, status and decoded word are written by the group's
// first lane.  No LDS; a grid-stride walk over the rows; every lane of a wave makes the same number of trips (the ballots need
// all 64 lanes); rows beyond the end are computed on zeros and not stored.
//
// Written only against the `wave::` primitives and mont_core.h's look-ahead (through slot_codec.h's group_sub_words), so that
// tests/emu/wave_emu.h runs the bodies as they are.  Include after wave_gfx950.h (or wave_emu.h), mont_core.h and slot_codec.h.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace phe {

enum : uint32_t { kValueInt64 = 0, kValueUint64 = 1, kValueFloat = 2, kValueFloatPrecision = 3 };
enum : uint32_t { kDecodeInt64 = 0, kDecodeFloat = 1 };

struct ValueEncodeArgs {
    const uint32_t* n;     // G*K words, zero-extended (SlotConsts::n)
    const uint64_t* bits;  // the raw 64-bit words of the values
    uint64_t count;
    uint32_t kind;
    int32_t exponent;  // kind 3 only
    uint32_t* m_rows;  // (count, n_limbs)
    int32_t* exps;     // count, written for kind 2 (may be null otherwise)
    uint8_t* status;   // count
    int n_limbs;
};
struct ValueDecodeArgs {
    SlotConsts k;            // n, max_int and n - max_int are read
    const uint32_t* m_rows;  // (rows, n_limbs)
    uint64_t rows;
    uint32_t kind;
    const int32_t* exps;  // rows, kind 1
    uint64_t* out;        // rows: int64 or float64 words
    uint8_t* status;      // rows
    int n_limbs;
};

// the K words of lane g of a row: one access of 4 K bytes (16-byte pieces for K = 8) where `whole` (K divides n_limbs: the piece
// lies inside the row and is aligned to min(4 K, 16) bytes, given a row base aligned so), else word by word with the words at or
// beyond n_limbs read as 0 / not stored
template <int K>
PHE_DEV void value_load_piece(uint32_t (&x)[K], const uint32_t* row, uint32_t g, int n_limbs, bool whole) {
    if (whole) {
        if ((int)(g * K) < n_limbs) __builtin_memcpy(x, __builtin_assume_aligned(row + g * K, K >= 4 ? 16 : 4 * K), 4 * K);
        else {
#pragma unroll
            for (int k = 0; k < K; ++k) x[k] = 0u;
        }
        return;
    }
#pragma unroll
    for (int k = 0; k < K; ++k) x[k] = (int)(g * K + k) < n_limbs ? row[g * K + k] : 0u;
}
template <int K>
PHE_DEV void value_store_piece(uint32_t* row, const uint32_t (&x)[K], uint32_t g, int n_limbs, bool whole) {
    if (whole) {
        if ((int)(g * K) < n_limbs) __builtin_memcpy(__builtin_assume_aligned(row + g * K, K >= 4 ? 16 : 4 * K), x, 4 * K);
        return;
    }
#pragma unroll
    for (int k = 0; k < K; ++k)
        if ((int)(g * K + k) < n_limbs) row[g * K + k] = x[k];
}

// float64 word -> imant (53 bits, 0 for a zero) and lsb with |x| = imant * 2^lsb; false: inf / nan
PHE_DEV bool value_split_double(uint64_t w, uint64_t& imant, int& lsb) {
    const uint32_t E = (uint32_t)(w >> 52) & 0x7ffu;
    const uint64_t frac = w & ((1ull << 52) - 1ull);
    imant = 0;
    lsb = -1075;
    if (E == 0x7ffu) return false;
    if (E == 0u) {
        if (frac) {
            const int s = __builtin_clzll(frac) - 11;  // 53 - bitlength(frac)
            imant = frac << s;
            lsb = -1074 - s;
        }
    } else {
        imant = frac | (1ull << 52);
        lsb = (int)E - 1075;
    }
    return true;
}

// values -> plaintext rows, exponents (kind 2) and one status byte per row (0: fine, 1: inf / nan, 2: |r| >= 2^62 under a
// precision).  The row of a value with a non-zero status is 0.
template <int G, int K>
PHE_DEV void values_encode_body(const ValueEncodeArgs& A, uint32_t group, uint32_t total, uint32_t lane) {
    const Lanes<G> ln(lane);
    const bool whole = A.n_limbs % K == 0;
    uint32_t nn[K];
    slot_load_row<K>(nn, A.n, ln.g);
    for (uint64_t first = 0; first < A.count; first += total) {
        const uint64_t row = first + group;
        const bool active = row < A.count;
        const uint64_t w = active ? A.bits[row] : 0ull;
        uint64_t mag = 0;
        uint32_t neg = 0, st = 0;
        int32_t e = 0;
        if (A.kind == kValueInt64) {
            neg = (uint32_t)(w >> 63);
            mag = neg ? 0ull - w : w;
        } else if (A.kind == kValueUint64) {
            mag = w;
        } else {
            uint64_t imant;
            int lsb;
            neg = (uint32_t)(w >> 63);
            if (!value_split_double(w, imant, lsb)) {
                st = 1;
            } else if (A.kind == kValueFloat) {
                if (imant == 0) {
                    e = -14;  // frexp(0) = (0, 0): floor((0 - 53) / 4)
                } else {
                    e = lsb >> 2;  // floor(lsb / 4)
                    mag = imant << (lsb & 3);
                }
            } else if (imant) {
                e = A.exponent;
                const int64_t t = (int64_t)lsb - 4 * (int64_t)A.exponent;  // r = rint(imant * 2^t), imant in [2^52, 2^53)
                if (t >= 10) {
                    st = 2;
                } else if (t >= 0) {
                    mag = imant << t;
                } else if (t >= -53) {
                    const int u = (int)-t;
                    const uint64_t q = imant >> u, rem = imant & ((1ull << u) - 1ull), half = 1ull << (u - 1);
                    mag = q + ((rem > half || (rem == half && (q & 1ull))) ? 1ull : 0ull);
                }  // below 2^-54 of a unit: less than a half, 0
            }
        }
        if (st) mag = 0;
        uint32_t a[K], d[K];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const uint32_t word = ln.g * K + k;
            a[k] = word == 0u ? (uint32_t)mag : word == 1u ? (uint32_t)(mag >> 32) : 0u;
        }
        group_sub_words<G, K>(d, nn, a, ln);  // n - mag: the borrow may run through every word of the row
        const bool flip = neg && mag != 0;    // -0.0 and 0 give 0, never n
        if (active) {
#pragma unroll
            for (int k = 0; k < K; ++k) a[k] = flip ? d[k] : a[k];
            value_store_piece<K>(A.m_rows + row * (uint64_t)A.n_limbs, a, ln.g, A.n_limbs, whole);
            if (ln.g == 0) {
                A.status[row] = (uint8_t)st;
                if (A.kind == kValueFloat) A.exps[row] = e;
            }
        }
    }
}

// plaintext rows -> one int64 / float64 word and one status byte per row
template <int G, int K>
PHE_DEV void values_decode_body(const ValueDecodeArgs& A, uint32_t group, uint32_t total, uint32_t lane) {
    const Lanes<G> ln(lane);
    const bool whole = A.n_limbs % K == 0;
    uint64_t group_lanes = ~0ull;
    if constexpr (G < 64) group_lanes = ((1ull << G) - 1ull) << (ln.lane & ~(uint32_t)(G - 1));
    uint32_t nn[K], mx[K], lo[K];
    slot_load_row<K>(nn, A.k.n, ln.g);
    slot_load_row<K>(mx, A.k.max_int, ln.g);
    slot_load_row<K>(lo, A.k.neg_low, ln.g);
    for (uint64_t first = 0; first < A.rows; first += total) {
        const uint64_t row = first + group;
        const bool active = row < A.rows;
        uint32_t m[K], t[K], d[K];
        if (active) value_load_piece<K>(m, A.m_rows + row * (uint64_t)A.n_limbs, ln.g, A.n_limbs, whole);
        else {
#pragma unroll
            for (int k = 0; k < K; ++k) m[k] = 0u;
        }
        const uint32_t above = group_sub_words<G, K>(t, mx, m, ln);  // max_int - m borrows: m > max_int
        const uint32_t below = group_sub_words<G, K>(t, m, lo, ln);  // m - (n - max_int) borrows: m < n - max_int
        const uint32_t over = group_sub_words<G, K>(d, nn, m, ln);   // d = n - m: |v| of a negative number; borrows: m > n
        uint32_t dnz = 0, high = 0;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            dnz |= d[k];
            t[k] = above ? d[k] : m[k];  // |v|
            if (ln.g * K + k >= 2u) high |= t[k];
        }
        const bool is_n = (wave::ballot(dnz != 0) & group_lanes) == 0;   // m == n
        const bool wide = (wave::ballot(high != 0) & group_lanes) != 0;  // |v| >= 2^64
        uint32_t w1;
        if constexpr (K >= 2) w1 = t[1];
        else w1 = wave::grp_down1<G>(t[0], ln);
        if (active && ln.g == 0) {
            const uint64_t mag = ((uint64_t)w1 << 32) | t[0];
            uint32_t st = (over || is_n) ? 3u : (above && below) ? 1u : wide ? 2u : 0u;
            uint64_t out = 0;
            if (st == 0) {
                if (A.kind == kDecodeInt64) {
                    if (mag > (1ull << 63) - (above ? 0ull : 1ull)) st = 2;
                    out = above ? 0ull - mag : mag;
                } else {
                    // 2^(4 e) as a double: a normal number for -255 <= e < 0, so the product with a magnitude >= 1 is exact
                    const int64_t biased = 1023 + 4 * (int64_t)A.exps[row];
                    const uint64_t pw = (uint64_t)(biased < 1 ? 1 : biased > 2046 ? 2046 : biased) << 52;
                    double scale, v = (double)mag;  // round to nearest, ties to even
                    __builtin_memcpy(&scale, &pw, 8);
                    v *= scale;
                    if (above) v = -v;
                    __builtin_memcpy(&out, &v, 8);
                }
            }
            A.out[row] = out;
            A.status[row] = (uint8_t)st;
        }
    }
}

namespace host {

// true when max_int = n // 3 - 1 >= 2^64: every 64-bit magnitude is a valid plaintext and n has at least three words
inline bool value_codec_key_ok(const uint32_t* n, int n_limbs) {
    if (n_limbs < 3) return false;
    const std::vector<uint32_t> mx = slot_max_int(n, n_limbs);
    for (int i = 2; i < n_limbs; ++i)
        if (mx[(size_t)i]) return true;
    return false;
}

}  // namespace host

}  // namespace phe
