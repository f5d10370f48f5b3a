// chacha_rows.h — rows of random exponent words drawn on the device: the ChaCha20 keystream (RFC 8439, 20 rounds) of one 256-bit
// key laid out as (rows, limbs) 32-bit words, each row cut to `bits` bits.  The short obfuscator exponents rho of fixed_base.h
// are such rows: every value below 2^bits is valid, nothing is rejected, and the host draw of them from the kernel CSPRNG (one
// thread, 128 MB for 2^20 rows of 1024 bits) took longer than the comb kernel that reads them.
//
// The state of block c is the RFC's: words 0-3 the constants, 4-11 the key, 12 the 32-bit block counter c, 13-15 the nonce; ten
// double rounds, then the input state is added.  A row takes B = ceil(limbs / 16) blocks of its own: word w of row i is word
// w % 16 of block counter0 + i*B + w / 16.  What a row does not use of its last block is thrown away, never handed to the next
// row, so a row's words depend on (key, nonce, counter0, i, limbs) alone.  Bits at or above `bits` in limb (bits - 1) / 32 are
// cleared and the limbs above it are zero (the conventions of the host draw, phe/_engine.py random_bits_limbs).
//
// One lane owns one block: the sixteen state words stay in registers, and the lane stores the (up to) 64 bytes of its block as
// four 16-byte stores.  The blocks are grid-strided.  The host checks counter0 + rows*B <= 2^32 (phe_hip.hip), so a block's
// number fits 32 bits and the counter never wraps inside a launch.  Key and nonce are members of the argument struct: they reach
// the kernel in its argument segment and no device allocation holds them.
#pragma once

namespace phe {

struct ChaChaRowsArgs {
    uint32_t key[8];
    uint32_t nonce[3];
    uint32_t counter0;
    int bits;            // 1 .. 32 * limbs
    int limbs;           // words of an output row
    int blocks_per_row;  // B = ceil(limbs / 16)
    uint32_t* out;       // (rows, limbs)
    uint64_t rows;       // rows * B <= 2^32 - counter0
};

PHE_DEV uint32_t chacha_rotl(uint32_t x, int k) { return (x << k) | (x >> (32 - k)); }

#define PHE_CHACHA_QR(a, b, c, d)                 \
    do {                                          \
        a += b; d ^= a; d = chacha_rotl(d, 16);   \
        c += d; b ^= c; b = chacha_rotl(b, 12);   \
        a += b; d ^= a; d = chacha_rotl(d, 8);    \
        c += d; b ^= c; b = chacha_rotl(b, 7);    \
    } while (0)

// x[0..15] = the keystream block `counter` of (key, nonce)
PHE_DEV void chacha20_block(uint32_t (&x)[16], const ChaChaRowsArgs& A, uint32_t counter) {
    uint32_t s[16] = {0x61707865u, 0x3320646eu, 0x79622d32u, 0x6b206574u, A.key[0], A.key[1], A.key[2], A.key[3],
                      A.key[4],    A.key[5],    A.key[6],    A.key[7],    counter,  A.nonce[0], A.nonce[1], A.nonce[2]};
#pragma unroll
    for (int i = 0; i < 16; ++i) x[i] = s[i];
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        PHE_CHACHA_QR(x[0], x[4], x[8], x[12]);
        PHE_CHACHA_QR(x[1], x[5], x[9], x[13]);
        PHE_CHACHA_QR(x[2], x[6], x[10], x[14]);
        PHE_CHACHA_QR(x[3], x[7], x[11], x[15]);
        PHE_CHACHA_QR(x[0], x[5], x[10], x[15]);
        PHE_CHACHA_QR(x[1], x[6], x[11], x[12]);
        PHE_CHACHA_QR(x[2], x[7], x[8], x[13]);
        PHE_CHACHA_QR(x[3], x[4], x[9], x[14]);
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) x[i] += s[i];
}
#undef PHE_CHACHA_QR

// four words to a 4-byte aligned address as one 16-byte store (a row of an odd number of limbs starts at any word)
PHE_DEV void chacha_store4(uint32_t* p, uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
    typedef uint32_t __attribute__((vector_size(16), aligned(4))) u32x4_a4;
    *reinterpret_cast<u32x4_a4*>(p) = (u32x4_a4){a, b, c, d};
}

// `slot` of `total_slots` lanes walks the rows * B blocks
PHE_DEV void chacha_rows_body(const ChaChaRowsArgs& A, uint32_t slot, uint32_t total_slots) {
    const uint32_t B = (uint32_t)A.blocks_per_row;
    const uint64_t n_blocks = A.rows * B;  // <= 2^32
    const int top = (A.bits - 1) >> 5;     // the limb that holds the highest bit
    const uint32_t top_mask = 0xffffffffu >> (31 - ((A.bits - 1) & 31));
    for (uint64_t b = slot; b < n_blocks; b += total_slots) {
        const uint32_t blk = (uint32_t)b;
        const uint32_t row = blk / B, k = blk - row * B;
        uint32_t x[16];
        chacha20_block(x, A, A.counter0 + blk);
        const int w0 = (int)(16u * k);  // the block's first word in its row
        uint32_t* dst = A.out + (uint64_t)row * (uint64_t)A.limbs + w0;
        if (w0 + 15 >= top) {  // (uniform in a wavefront's lanes of one k: the block that holds the top limb, and those above)
#pragma unroll
            for (int j = 0; j < 16; ++j) x[j] = (w0 + j < top) ? x[j] : (w0 + j == top ? x[j] & top_mask : 0u);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int w = w0 + 4 * q;
            if (w + 4 <= A.limbs) {
                chacha_store4(dst + 4 * q, x[4 * q], x[4 * q + 1], x[4 * q + 2], x[4 * q + 3]);
            } else {  // the ragged end of a row: word by word, nothing past the row
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (w + j < A.limbs) dst[4 * q + j] = x[4 * q + j];
            }
        }
    }
}

}  // namespace phe
