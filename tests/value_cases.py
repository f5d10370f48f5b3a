"""TEST INFRASTRUCTURE — the cases tests/test_value_codec.py (CPU wave emulator) and tests/test_gpu_value_codec.py (the kernels)
share for the value codec (csrc/value_codec.h), and the codec itself in Python integers: what both are compared with.

The encode reference is EncodedNumber.encode(pk, v, precision) element by element, the decode reference is
EncodedNumber(pk, m, e).decode().  Status bytes — encode: 1 for inf / nan, 2 for a mantissa of 2^62 or more under a precision;
decode: 3 for m >= n, 1 for the overflow gap, 2 for |v| >= 2^64 or an integer outside int64."""
import math
import random
import struct
import sys

import numpy as np

from conftest import PKG

if PKG not in sys.path:
    sys.path.insert(0, PKG)

from phe.codec import EncodedNumber  # noqa: E402

KIND_INT64, KIND_UINT64, KIND_FLOAT, KIND_PRECISION = 0, 1, 2, 3
OUT_INT64, OUT_FLOAT = 0, 1
PRECISIONS = (1e-6, 2.0 ** -20, 1.0, 1e-12)
DECODE_EXPONENTS = (-1, -14, -64, -240)
M64 = (1 << 64) - 1


class Key:
    """what EncodedNumber needs of a public key; n need not be a product of two primes for the codec"""

    def __init__(self, n):
        self.n, self.max_int = n, n // 3 - 1


def crafted_modulus(words):
    """an odd n of `words` words whose words 1 .. words - 2 are zero: n - mag borrows through every lane of the group"""
    return (0x9E3779B1 << (32 * (words - 1))) | 5


def f2b(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def b2f(w):
    return struct.unpack("<d", struct.pack("<Q", w))[0]


def to_limbs(xs, words):
    raw = b"".join(int(x).to_bytes(4 * words, "little") for x in xs)
    return np.frombuffer(raw, np.uint32).reshape(len(xs), words).copy()


def to_ints(arr):
    w = arr.shape[1] * 4
    raw = np.ascontiguousarray(arr).tobytes()
    return [int.from_bytes(raw[i * w:(i + 1) * w], "little") for i in range(arr.shape[0])]


def exponent_of(precision):
    return EncodedNumber._natural_exponent(0.0, precision)


# ---- the codec in Python integers ---------------------------------------------------------------------------------------------
def encode_ref(key, word, kind, precision=None):
    """(m, exponent, status) of one 64-bit value word; m = 0 where the status is not 0"""
    if kind == KIND_INT64:
        v = word - (1 << 64) if word >> 63 else word
    elif kind == KIND_UINT64:
        v = word
    else:
        v = b2f(word)
        if math.isinf(v) or math.isnan(v):
            return 0, None, 1
    e = EncodedNumber.encode(key, v, precision=precision if kind == KIND_PRECISION else None)
    if kind == KIND_PRECISION:
        signed = e.encoding if e.encoding <= key.max_int else e.encoding - key.n
        if abs(signed) >= 1 << 62:
            return 0, e.exponent, 2
    return e.encoding, e.exponent, 0


def decode_ref(key, m, exponent, kind):
    """(status, 64-bit word or None)"""
    n, max_int = key.n, key.max_int
    if m >= n:
        return 3, None
    if m <= max_int:
        v = m
    elif m >= n - max_int:
        v = m - n
    else:
        return 1, None
    if abs(v) >= 1 << 64:
        return 2, None
    if kind == OUT_INT64:
        if not -(1 << 63) <= v < 1 << 63:
            return 2, None
        assert EncodedNumber(key, m, 0).decode() == v
        return 0, v & M64
    return 0, f2b(EncodedNumber(key, m, exponent).decode())


# ---- values -------------------------------------------------------------------------------------------------------------------
def borrow_magnitudes(n):
    n_lo = n & M64
    return [m for m in (n_lo - 1, n_lo, n_lo + 1) if 0 < m]


def int64_words(n, rng, count):
    vals = [0, 1, -1, (1 << 63) - 1, -(1 << 63), (1 << 32) - 1, -((1 << 32) - 1), 1 << 32, -(1 << 32)]
    vals += [-m for m in borrow_magnitudes(n) if m <= 1 << 63] + [m for m in borrow_magnitudes(n) if m < 1 << 63]
    while len(vals) < count:
        vals.append(rng.randint(-(1 << 63), (1 << 63) - 1) >> rng.choice((0, 0, 17, 40, 62)))
    return [v & M64 for v in vals]


def uint64_words(n, rng, count):
    vals = [0, 1 << 63, M64] + [m for m in borrow_magnitudes(n) if m <= M64]
    while len(vals) < count:
        vals.append(rng.getrandbits(64) >> rng.choice((0, 0, 31, 63)))
    return vals


def float_words(rng, count, non_finite=True):
    top = sys.float_info.max
    vals = [0.0, -0.0, 5e-324, -5e-324, 3 * 5e-324, 2.0 ** -1022 - 5e-324, 2.0 ** -1022, top, -top, 1.0, 2.0, 4.0, 8.0, 16.0,
            0.1, -0.1]
    words = [f2b(v) for v in vals]
    while len(words) < count:
        w = rng.getrandbits(64)
        if (w >> 52) & 0x7ff != 0x7ff:
            words.append(w)
    if non_finite:                                                     # each alone between good rows
        for k, bad in enumerate((float("inf"), float("-inf"), float("nan"))):
            words[20 + 7 * k] = f2b(bad)
        words[-1] = 0xfff0000000000001                                 # a negative signalling nan, last
    return words


def precision_words(precision, rng, count, n=None):
    """values around the scale 16^e of a precision: rounding ties, |r| just below and at 2^62, tiny and huge ones, random ones"""
    e = exponent_of(precision)
    scale = 2.0 ** (4 * e)
    units = [0.0, -0.0, 0.5, -0.5, 1.5, -1.5, 2.5, -2.5, 2.0 ** 40 + 0.5, 0.5 + 2.0 ** -40, 0.5 - 2.0 ** -40, 2.0 ** -53, 2.0 ** -54,
             0.75, 0.25, 1.0, -1.0, 2.0 ** 62 - 2.0 ** 9, 2.0 ** 62, -(2.0 ** 62 - 2.0 ** 9), 2.0 ** 52 + 1.0, 2.0 ** 53 - 1.0]
    if n is not None:
        units += [float(m) * s for m in borrow_magnitudes(n) if m < 1 << 53 for s in (1, -1)]
    vals = [u * scale for u in units] + [5e-324, -5e-324, 2.0 ** -1022]
    while len(vals) < count:
        vals.append(rng.uniform(-1, 1) * 2.0 ** rng.randint(-60, 61) * scale)
    return [f2b(v) for v in vals], e


def decode_rows(n, kind):
    """(m, expected status): the rows of the issue's list, each to be set between two good rows"""
    max_int = n // 3 - 1
    wide = 2 if kind == OUT_INT64 else 0                               # beyond int64, within 64 bits: fine as a float
    return [(0, 0), (1, 0), (n - 1, 0), (max_int, 2), (max_int + 1, 1), (n - max_int - 1, 1), (n - max_int, 2), (n, 3), (n + 1, 3),
            ((1 << 63) - 1, 0), (1 << 63, wide), (n - (1 << 63), 0), (n - (1 << 63) - 1, wide), (M64, wide), (1 << 64, 2),
            (n - (1 << 64), 2), (n - M64, wide)]


ROUNDING_MAGNITUDES = ((1 << 53) + 1, (1 << 53) + 3, (1 << 54) + 2, (1 << 54) + 6, M64, (1 << 64) - 1024, (1 << 64) - 1025,
                       (1 << 64) - 3072)


# ---- the checks both suites run -----------------------------------------------------------------------------------------------
def check_encode(encode, n, seed, count=300):
    """encode(words uint64 array, kind, exponent) -> (m_rows (count, n_limbs) uint32, exps int32 or None, status uint8), against
    EncodedNumber.encode for all four kinds.  Returns the statuses seen."""
    key, rng = Key(n), random.Random(seed)
    words_n = (n.bit_length() + 31) // 32
    seen = set()
    sets = [(KIND_INT64, None, int64_words(n, rng, count), 0), (KIND_UINT64, None, uint64_words(n, rng, count), 0),
            (KIND_FLOAT, None, float_words(rng, count), 0)]
    for precision in PRECISIONS:
        words, e = precision_words(precision, rng, count // 2, n)
        sets.append((KIND_PRECISION, precision, words, e))
    for kind, precision, words, e in sets:
        want = [encode_ref(key, w, kind, precision) for w in words]
        for sub in (words, words[:1], words[:5]):
            rows, exps, status = encode(np.array(sub, dtype=np.uint64), kind, e)
            assert rows.shape == (len(sub), words_n)
            ref = want[:len(sub)]
            assert status.tolist() == [st for _, _, st in ref], (kind, precision, "status")
            assert to_ints(rows) == [m for m, _, _ in ref], (kind, precision, "rows")
            if kind == KIND_FLOAT:
                assert [x for x, (_, _, st) in zip(exps.tolist(), ref) if st == 0] == [x for _, x, st in ref if st == 0], (kind, "exps")
            else:
                assert all(x == e for _, x, st in ref if st == 0)
        seen |= {st for _, _, st in want}
        if kind == KIND_PRECISION:
            ties = [m if m <= key.max_int else m - n for m, _, _ in want[:9]]
            assert ties == [0, 0, 0, 0, 2, -2, 2, -2, 1 << 40]         # half to even
            assert [st for _, _, st in want[17:20]] == [0, 2, 0]       # just below 2^62, at it, and below on the other side
    assert seen == {0, 1, 2}
    return seen


def check_decode(decode, n, seed, count=300):
    """decode(m_rows (rows, n_limbs) uint32, kind, exps int32 array or None) -> (uint64 words, uint8 status), against
    EncodedNumber.decode for both kinds: the listed rows between good rows, the rounding magnitudes at every exponent, random
    magnitudes of both signs."""
    key, rng = Key(n), random.Random(seed)
    words_n = (n.bit_length() + 31) // 32
    for kind in (OUT_INT64, OUT_FLOAT):
        ms, es, expect = [], [], []

        def good():
            mag = rng.getrandbits(rng.choice((63, 40, 20, 1)))
            return mag if rng.random() < 0.5 or mag == 0 else n - mag
        for m, st in decode_rows(n, kind):
            ms += [good(), m]
            expect += [0, st]
        if kind == OUT_FLOAT:
            for mag in ROUNDING_MAGNITUDES:
                ms += [mag, n - mag]
                expect += [0, 0]
        while len(ms) < count:
            ms.append(good())
            expect.append(0)
        if kind == OUT_FLOAT:
            es = [DECODE_EXPONENTS[i % 4] for i in range(len(ms))]
            for mag in ROUNDING_MAGNITUDES:                            # ... every rounding magnitude at every exponent
                for e in DECODE_EXPONENTS:
                    ms += [mag, n - mag]
                    es += [e, e]
                    expect += [0, 0]
        else:
            es = [0] * len(ms)
        ref = [decode_ref(key, m, e, kind) for m, e in zip(ms, es)]
        assert [st for st, _ in ref] == expect, (kind, "the cases' own expectation")
        for rows in (len(ms), 1, 5):
            exps = np.array(es[:rows], dtype=np.int32) if kind == OUT_FLOAT else None
            out, status = decode(to_limbs(ms[:rows], words_n), kind, exps)
            assert status.tolist() == expect[:rows], (kind, "status")
            got = out.tolist()
            for i in range(rows):
                if expect[i] == 0:
                    assert got[i] == ref[i][1], (kind, i, hex(ms[i]), es[i])
