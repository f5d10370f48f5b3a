"""ChaCha20 (RFC 8439, 20 rounds) expanded into rows of random exponent words on the host, numpy-vectorised over blocks.

The layout and the masking are those of the device kernel (csrc/chacha_rows.h): a row of `limbs` 32-bit words takes
B = ceil(limbs / 16) keystream blocks of its own, word w of row i is word w % 16 of block counter0 + i*B + w // 16, the unused
tail of a row's last block is thrown away, bits at or above `bits` are cleared.  It is the route of a backend without the
kernel, and the second implementation the kernel is compared against.
"""
import numpy as np

CONSTANTS = (0x61707865, 0x3320646E, 0x79622D32, 0x6B206574)
_CHUNK = 1 << 16      # blocks expanded at a time (16 state arrays of that many words)


def _words(seed, count, what):
    """`count` little-endian 32-bit words from bytes / bytearray, or a sequence of `count` integers"""
    if isinstance(seed, (bytes, bytearray, memoryview)):
        if len(seed) != 4 * count:
            raise ValueError("%s must be %d bytes" % (what, 4 * count))
        return np.frombuffer(bytes(seed), dtype="<u4").astype(np.uint32)
    arr = np.asarray(seed, dtype=np.uint32)
    if arr.shape != (count,):
        raise ValueError("%s must be %d words" % (what, count))
    return arr


def _rotl(x, k):
    return (x << np.uint32(k)) | (x >> np.uint32(32 - k))


def _quarter(x, a, b, c, d):
    x[a] += x[b]; x[d] ^= x[a]; x[d] = _rotl(x[d], 16)
    x[c] += x[d]; x[b] ^= x[c]; x[b] = _rotl(x[b], 12)
    x[a] += x[b]; x[d] ^= x[a]; x[d] = _rotl(x[d], 8)
    x[c] += x[d]; x[b] ^= x[c]; x[b] = _rotl(x[b], 7)


def chacha20_blocks(key, nonce, counter0, count):
    """(count, 16) uint32: the keystream blocks counter0 .. counter0 + count - 1 (the counter may not wrap)"""
    key, nonce = _words(key, 8, "key"), _words(nonce, 3, "nonce")
    counter0, count = int(counter0), int(count)
    if count < 0 or counter0 < 0 or counter0 + count > 1 << 32:
        raise ValueError("block counter out of range")
    out = np.empty((count, 16), np.uint32)
    for lo in range(0, count, _CHUNK):
        m = min(_CHUNK, count - lo)
        ctr = (np.arange(lo, lo + m, dtype=np.uint64) + np.uint64(counter0)).astype(np.uint32)
        start = [np.full(m, c, np.uint32) for c in CONSTANTS] + [np.full(m, k, np.uint32) for k in key] + [ctr] + \
                [np.full(m, v, np.uint32) for v in nonce]
        x = [s.copy() for s in start]
        for _ in range(10):
            _quarter(x, 0, 4, 8, 12); _quarter(x, 1, 5, 9, 13); _quarter(x, 2, 6, 10, 14); _quarter(x, 3, 7, 11, 15)
            _quarter(x, 0, 5, 10, 15); _quarter(x, 1, 6, 11, 12); _quarter(x, 2, 7, 8, 13); _quarter(x, 3, 4, 9, 14)
        for j in range(16):
            out[lo:lo + m, j] = x[j] + start[j]
    return out


def blocks_per_row(limbs):
    return (int(limbs) + 15) // 16


def chacha20_rows(key, nonce, counter0, bits, limbs, rows):
    """(rows, limbs) uint32: random values below 2^bits, the words csrc/chacha_rows.h writes for the same arguments"""
    bits, limbs, rows = int(bits), int(limbs), int(rows)
    if limbs < 1 or bits < 1 or bits > 32 * limbs:
        raise ValueError("bits must be in 1 .. 32 * limbs")
    B = blocks_per_row(limbs)
    if rows < 0 or int(counter0) < 0 or int(counter0) + rows * B > 1 << 32:
        raise ValueError("the block counter would wrap")
    out = chacha20_blocks(key, nonce, counter0, rows * B).reshape(rows, 16 * B)[:, :limbs].copy()
    top = (bits - 1) // 32
    out[:, top] &= np.uint32(0xFFFFFFFF >> (31 - (bits - 1) % 32))
    out[:, top + 1:] = 0
    return out
