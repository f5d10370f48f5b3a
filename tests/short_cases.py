"""TEST INFRASTRUCTURE shared by tests/test_short_obfuscators.py and tests/test_gpu_short_obfuscators.py: the exponent sets and
the integer formulas of the short-exponent obfuscators (PaillierPublicKey.enable_short_obfuscators).

Expected values are Python integers: the obfuscator pow(h_s, rho, n^2), the encryption (1 + n*m) * pow(h_s, rho, n^2) mod n^2
and the re-randomisation c * pow(h_s, rho, n^2) mod n^2 for h = -x^2 mod n, h_s = pow(h, n, n^2).  CPython's pow of a 1024-bit
exponent modulo a 2048-bit key's n^2 takes tens of milliseconds: a test keeps its DISTINCT exponents to 64 at the most
(`obfuscators` caches them) and reuses them across its rows, rho_i = set[i mod 61]."""
import random

import numpy as np

X_FIXED = 0x1F3D5B79A2C4E6F81357  # the unit h is made of in every test (coprime to each golden n: asserted by base_of)


def base_of(n, x=X_FIXED):
    """(h, h_s) for the unit x"""
    from math import gcd
    assert gcd(x, n) == 1
    h = (-x * x) % n
    return h, pow(h, n, n * n)


def edge_exponents(bits, w, count=61, seed=0):
    """at most `count` distinct exponents below 2^bits: 0, 1, 2^bits - 1, the lone top bit, d * 2^(w t) for t in {0, T - 1} and
    d in {1, 2^w - 1} (at t = T - 1: d up to the top digit's width), then random ones"""
    T = -(-bits // w)
    top_width = bits - w * (T - 1)
    edge = [0, 1, (1 << bits) - 1, 1 << (bits - 1), (1 << w) - 1 if w <= bits else 1,
            1 << (w * (T - 1)), ((1 << top_width) - 1) << (w * (T - 1))]
    out = []
    for v in edge:
        v &= (1 << bits) - 1
        if v not in out:
            out.append(v)
    rng = random.Random(1000 * bits + w + seed)
    while len(out) < count:
        v = rng.randrange(1 << bits)
        if v not in out:
            out.append(v)
    return out[:count]


class Obfuscators:
    """pow(h_s, rho, n^2), each distinct rho once"""

    def __init__(self, hs, n):
        self.hs, self.n2, self.seen = hs, n * n, {}

    def __call__(self, rho):
        v = self.seen.get(rho)
        if v is None:
            assert len(self.seen) < 64, "a test keeps its distinct exponents to 64"
            v = self.seen[rho] = pow(self.hs, rho, self.n2)
        return v


def comb_table(hs, n, bits, w):
    """the entries (t, d), 1 <= d < 2^w, of the comb table as Python integers, row t * (2^w - 1) + d - 1: h_s^(d * 2^(w t)) by
    repeated products (entry (t, d) = entry (t, d - 1) * entry (t, 1))"""
    n2 = n * n
    out, base = [], hs
    for _ in range(-(-bits // w)):
        v = 1
        for _ in range(1, 1 << w):
            v = v * base % n2
            out.append(v)
        base = v * base % n2
    return out


def limbs(xs, words):
    raw = b"".join(int(x).to_bytes(4 * words, "little") for x in xs)
    return np.frombuffer(raw, np.uint32).reshape(len(xs), words).copy()


def ints(arr):
    w = arr.shape[1] * 4
    raw = arr.tobytes()
    return [int.from_bytes(raw[i * w:(i + 1) * w], "little") for i in range(arr.shape[0])]
