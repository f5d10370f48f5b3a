#!/usr/bin/env python3
"""Prime pairs whose two primes are NOT twins in size or carry structure (tests/key_shapes.py, tests/test_key_shapes.py,
tests/test_gpu_key_shapes.py): unequal lengths inside one limb count, one 32-bit word apart, far enough apart that the CRT
halves' geometries disagree, adjacent primes, Proth primes (p - 1 = k 2^a: a squarings-only tail of the exponent schedule) and
primes next to a power of two, and two pairs one byte either side of balanced.  Every pair is drawn from a fixed seed per name
and tested here with a Miller-Rabin of 24 fixed bases; only the primes are stored, smaller one first, and the tests derive
everything else on Python integers.
    python tests/golden/gen_key_shapes.py > tests/golden/key_shapes_primes.json"""
import json
import math
import random

SMALL = [3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37, 41, 43, 47, 53, 59, 61, 67, 71, 73, 79, 83, 89, 97]
BASES = [2] + SMALL[:23]


def is_prime(n):
    """Miller-Rabin to 24 fixed bases after trial division"""
    if n < 2:
        return False
    for s in [2] + SMALL:
        if n % s == 0:
            return n == s
    d, s = n - 1, 0
    while d % 2 == 0:
        d, s = d // 2, s + 1
    for a in BASES:
        x = pow(a, d, n)
        if x == 1 or x == n - 1:
            continue
        for _ in range(s - 1):
            x = x * x % n
            if x == n - 1:
                break
        else:
            return False
    return True


def random_prime(bits, rng, top_two=False):
    while True:
        cand = rng.getrandbits(bits) | (1 << (bits - 1)) | 1
        if top_two:
            cand |= 1 << (bits - 2)
        if is_prime(cand):
            return cand


def proth_prime(bits, a, rng):
    """k 2^a + 1 of exactly `bits` bits, k odd"""
    while True:
        k = rng.getrandbits(bits - a) | (1 << (bits - a - 1)) | 1
        cand = (k << a) + 1
        if is_prime(cand):
            return cand


def next_prime(x):
    x += 1 + (x & 1)                                          # the next odd number above x
    while not is_prime(x):
        x += 2
    return x


def prev_prime(x):
    x -= 1 + (x & 1)
    while not is_prime(x):
        x -= 2
    return x


def usable(p, q, n_bits=None):
    """a Paillier key: p != q, gcd(n, (p - 1)(q - 1)) = 1 (the unequal lengths allow p | q - 1), and n of the length asked for"""
    n = p * q
    return p < q and math.gcd(n, (p - 1) * (q - 1)) == 1 and (n_bits is None or n.bit_length() == n_bits)


def unequal(name, p_bits, q_bits):
    rng = random.Random("key shape " + name)
    while True:
        p, q = random_prime(p_bits, rng), random_prime(q_bits, rng)
        if usable(p, q, p_bits + q_bits):
            return p, q


def twins():
    rng = random.Random("key shape twins")
    while True:
        p = random_prime(512, rng, top_two=True)
        q = next_prime(p)
        if usable(p, q, 1024):
            return p, q


def proth(name, p_bits, a_p, q_bits, a_q):
    rng = random.Random("key shape " + name)
    while True:
        p, q = proth_prime(p_bits, a_p, rng), proth_prime(q_bits, a_q, rng)
        if p > q and p_bits == q_bits:
            p, q = q, p
        if usable(p, q, p_bits + q_bits):
            return p, q


def edges():
    p, q = next_prime(1 << 511), prev_prime(1 << 512)
    assert usable(p, q)
    return p, q


SHAPES = [
    ("one_bit", lambda: unequal("one_bit", 511, 513)),
    ("one_word", lambda: unequal("one_word", 496, 528)),
    ("regroup_a", lambda: unequal("regroup_a", 448, 576)),
    ("regroup_b", lambda: unequal("regroup_b", 384, 640)),
    ("regroup_c", lambda: unequal("regroup_c", 256, 768)),
    ("wide_a", lambda: unequal("wide_a", 1000, 1048)),
    ("wide_b", lambda: unequal("wide_b", 928, 1120)),
    ("tiny_p", lambda: unequal("tiny_p", 33, 223)),
    ("twins", twins),
    ("proth", lambda: proth("proth", 512, 180, 512, 200)),
    ("proth_unequal", lambda: proth("proth_unequal", 200, 150, 312, 250)),
    ("edges", edges),
    # unequal lengths whose SCALED moduli (29 bits more each) still need one count of limbs: the 16-lane late sweeps keep their
    # constants (key_setup.h build_private drops both quick packs otherwise), as they do for balanced keys of these sizes
    ("late_256", lambda: unequal("late_256", 120, 136)),
    ("late_2048", lambda: unequal("late_2048", 1016, 1032)),
]


if __name__ == "__main__":
    out = {}
    for name, make in SHAPES:
        p, q = make()
        out[name] = {"p": "%x" % p, "q": "%x" % q}
    print(json.dumps(out, indent=1))
