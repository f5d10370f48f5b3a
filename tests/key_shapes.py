"""Private keys whose two primes are not twins in size or carry structure (TEST HELPER, not a conftest).

tests/golden/key_shapes_primes.json (tests/golden/gen_key_shapes.py) holds the primes only; everything else is derived here on
Python integers, the way the reference derives it (phe/paillier.py:217-235, restated in oracle/paillier_oracle.py PyPrivate).
The rows a key is tried on are the places where the CRT tail leans on m_p < p < q:

    plaintexts    0, 1, n - 1, p, q, p - 1, q - 1, n - q, n - p, q - p, (q - p) p mod n and three random ones, each encrypted with
                  a random unit r
    ciphertexts   1, n^2 - 1, 1 + n, a multiple of p and a multiple of q (c^(p-1) mod p^2 = 0: the reference's l_function floors
                  (0 - 1) // p to -1, csrc/decrypt_tail.h tail_l_function has a branch for it)

The expected plaintext of EVERY row is PyPrivate.raw_decrypt on CPython ints; for the encrypted rows it must also be m."""
import json
import math
import os
import random

from oracle.paillier_oracle import PyPrivate, PyPublic

HERE = os.path.dirname(os.path.abspath(__file__))

# what each shape reaches (the table of the fixture's generator, for messages and the recorded GPU run)
NAMES = ("one_bit", "one_word", "regroup_a", "regroup_b", "regroup_c", "wide_a", "wide_b", "tiny_p", "twins", "proth",
         "proth_unequal", "edges", "late_256", "late_2048")
WIDE = ("wide_a", "wide_b", "late_2048")                                    # 2048-bit keys: the emulator runs them on fewer rungs

# the refusals of csrc/key_setup.h a key may meet at context creation (build_tail, build_private, build_modulus)
REFUSALS = ("p and q too unbalanced", "expected p < q", "modulus too wide for the compiled kernels (max 8344 bits)")


def limbs_for_bits(bits):
    return max(1, (bits + 31) // 32)


class ShapeKey:
    """one key of the zoo on Python integers; p < q"""

    def __init__(self, name, p, q):
        assert p < q
        self.name, self.p, self.q = name, p, q
        self.n = p * q
        self.nsq = self.n * self.n
        self.py = PyPrivate(PyPublic(self.n), q, p)            # (handed over in the wrong order: the reference sorts them)
        assert (self.py.p, self.py.q) == (p, q)
        self.hp, self.hq, self.p_inverse = self.py.hp, self.py.hq, self.py.p_inverse
        self.s1 = limbs_for_bits(self.n.bit_length())
        self.s2 = 2 * self.s1
        self.pq = limbs_for_bits(q.bit_length())

    def constants(self):
        return (self.p, self.q, self.hp, self.hq, self.p_inverse)

    def encrypt(self, m, r):
        return (1 + self.n * m) % self.nsq * pow(r, self.n, self.nsq) % self.nsq

    def decrypt(self, c):
        return self.py.raw_decrypt(c)

    def unit(self, rng):
        while True:
            r = rng.randrange(1, self.n)
            if math.gcd(r, self.n) == 1:
                return r

    def plaintexts(self, rng):
        p, q, n = self.p, self.q, self.n
        named = [(0, "m = 0"), (1, "m = 1"), (n - 1, "m = n - 1"), (p, "m = p"), (q, "m = q"), (p - 1, "m = p - 1"),
                 (q - 1, "m = q - 1"), (n - q, "m = n - q"), (n - p, "m = n - p"), (q - p, "m = q - p"),
                 ((q - p) * p % n, "m = (q - p) p mod n")]
        return named + [(rng.randrange(n), "m random") for _ in range(3)]

    def rows(self, seed=0):
        """[(c, m, tag)]: the fixed rows of the module docstring, 19 of them; m is what the reference's raw_decrypt gives"""
        rng = random.Random("rows %s %d" % (self.name, seed))
        out = []
        for m, tag in self.plaintexts(rng):
            c = self.encrypt(m, self.unit(rng))
            assert self.decrypt(c) == m, (self.name, tag)
            out.append((c, m, tag))
        direct = [(1, "c = 1"), (self.nsq - 1, "c = n^2 - 1"), (1 + self.n, "c = 1 + n"),
                  (self.p * rng.randrange(1, self.nsq // self.p), "c = k p"), (self.q * rng.randrange(1, self.nsq // self.q), "c = k q")]
        for c, tag in direct:
            out.append((c, self.decrypt(c), tag))
        # both borrow branches of d = m_q - m_p (+ q) are there by construction: m = p has m_p = 0 <= m_q, m = q has m_q = 0 < m_p
        assert any(m % self.q < m % self.p for _, m, _ in out) and any(m % self.q >= m % self.p for _, m, _ in out)
        return out

    def encrypt_rows(self, seed=0):
        """[(m, r, c, tag)] for raw_encrypt: the named plaintexts with random units r, and r = 1, r = n - 1"""
        rng = random.Random("encrypt rows %s %d" % (self.name, seed))
        ms = self.plaintexts(rng)
        rs = [self.unit(rng) for _ in ms]
        rs[0], rs[1] = 1, self.n - 1
        return [(m, r, self.encrypt(m, r), tag) for (m, tag), r in zip(ms, rs)]

    def random_rows(self, count, seed=1):
        """[(c, m)] of random plaintexts: r^n is computed ONCE per call and multiplied up (count may be thousands), so every row
        is a valid ciphertext with a different obfuscator"""
        rng = random.Random("random rows %s %d" % (self.name, seed))
        step = pow(self.unit(rng), self.n, self.nsq)
        rn, out = step, []
        for _ in range(count):
            m = rng.randrange(self.n)
            out.append(((1 + self.n * m) % self.nsq * rn % self.nsq, m))
            rn = rn * step % self.nsq
        return out


_zoo = None


def zoo():
    """{name: ShapeKey} of the committed primes, in the fixture's order"""
    global _zoo
    if _zoo is None:
        with open(os.path.join(HERE, "golden", "key_shapes_primes.json")) as f:
            raw = json.load(f)
        assert tuple(raw) == NAMES, tuple(raw)
        _zoo = {name: ShapeKey(name, int(v["p"], 16), int(v["q"], 16)) for name, v in raw.items()}
    return _zoo


def trailing_zeros(x):
    return (x & -x).bit_length() - 1


def first_mismatch(got, want, tags):
    for i, (g, w) in enumerate(zip(got, want)):
        if g != w:
            wrong = sum(1 for x, y in zip(got, want) if x != y)
            return "row %d (%s): %d of %d rows wrong" % (i, tags[i], wrong, len(want))
    return None if len(got) == len(want) else "row count %d != %d" % (len(got), len(want))


# ---- the refusal boundary: 256-bit keys from p of 16 bits upwards -----------------------------------------------------------------
SWEEP_N_BITS = 256
SWEEP_P_BITS = tuple(range(16, 121, 8))


def _is_prime(x):
    from lookahead import strong_probable_prime
    if x < 2:
        return False
    small = (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37)
    for s in small:
        if x % s == 0:
            return x == s
    return all(strong_probable_prime(x, a) for a in small)


def sweep_key(p_bits):
    """a seeded key with p of p_bits bits and n of exactly SWEEP_N_BITS bits"""
    rng = random.Random("sweep %d" % p_bits)

    def prime(bits):
        while True:
            x = rng.getrandbits(bits) | (1 << (bits - 1)) | 1
            if _is_prime(x):
                return x
    while True:
        p, q = prime(p_bits), prime(SWEEP_N_BITS - p_bits)
        if p < q and (p * q).bit_length() == SWEEP_N_BITS and math.gcd(p * q, (p - 1) * (q - 1)) == 1:
            return ShapeKey("sweep_%d" % p_bits, p, q)
