"""EncryptedVector.pack / PaillierPrivateKey.decrypt_packed — many small plaintexts per ciphertext — on a GPU-less box: the
public methods on the emulator backend (which has no packing kernel: every row to its own power by _raw_mul, then segment_sum),
the host unpacking on plaintexts packed by hand, and the device body itself (csrc/segment_core.h segment_pack_body) compiled for
the CPU wave emulator.

Expected ciphertexts are Python integers, prod_j pow(c_j, 1 << (B*j), n^2) mod n^2 over the aligned rows — the reference's chain
c_0*1 + c_1*(1 << B) + ... (EncryptedNumber.__mul__ -> _raw_mul, phe/paillier.py:721-751; __add__ -> _raw_add, :705-719) —
and expected plaintexts are the values that went in: never what the code under test returns."""
import ctypes
import os
import random
import subprocess
import sys

import numpy as np
import pytest

from conftest import PKG, ROOT, load_golden

if PKG not in sys.path:
    sys.path.insert(0, PKG)

from phe import paillier  # noqa: E402
from phe.ciphertext import EncryptedVector  # noqa: E402

H = lambda s: int(s, 16)


@pytest.fixture
def emu_keys(monkeypatch):
    import emu_backend
    emu_backend.install(monkeypatch)

    def make(bits):
        g = load_golden(bits)
        pub = paillier.PaillierPublicKey(H(g["n"]))
        return pub, paillier.PaillierPrivateKey(pub, H(g["p"]), H(g["q"]))
    return make


def integer_pack(vec, S, B):
    """row b: prod_j c[b*S + j] ^ (2^(B*j)) mod n^2 over the ciphertexts aligned to the smallest exponent, in Python integers"""
    n2 = vec.public_key.nsquare
    cs = vec.decrease_exponent_to(int(vec.exponent_array.min())).ciphertexts(False)
    want = []
    for b in range(0, len(cs), S):
        v = 1
        for j, c in enumerate(cs[b:b + S]):
            v = v * pow(c, 1 << (B * j), n2) % n2
        want.append(v)
    return want


def bound_of(pub):
    return pub.max_int.bit_length() - 1


# ---- pack on the emulator backend (no packing kernel there: the composition) --------------------------------------------------
@pytest.mark.parametrize("bits", [256, 1024])
def test_pack_on_the_emulator_backend(emu_keys, bits):
    pub, priv = emu_keys(bits)
    eng = pub._get_engine()
    assert not eng.has_segment_pack() and not hasattr(eng.ctx, "segment_pack_dev")
    rng = np.random.RandomState(bits)
    widest = bound_of(pub) // 64                                   # the largest S for B = 64 that the bound allows
    assert widest * 64 <= bound_of(pub) < (widest + 1) * 64 and widest >= 3
    for S, B in [(4, 16), (1, 9), (2, 1), (widest, 64)]:
        n = 3 * S + 2                                              # ragged: the last output row has two slots of S
        x = [int(v) for v in rng.randint(-3, 4, n)] if B > 1 else [-int(v) for v in rng.randint(0, 2, n)]
        vec = pub.encrypt_batch(x)
        assert not vec.on_device
        out = vec.pack(S, B)
        assert not out.on_device and not out._pair
        assert len(out) == -(-n // S) and set(out.exponents) == {0}
        assert out.ciphertexts(False) == integer_pack(vec, S, B), (S, B)
        assert priv.decrypt_packed(out, S, B, count=n) == x, (S, B)
        assert vec.pack(np.int64(S), np.int32(B)).ciphertexts(False) == out.ciphertexts(False)
    # S = 1: the aligned rows themselves
    vec = pub.encrypt_batch([1.5, 2, -3])
    assert vec.pack(1, 40).ciphertexts(False) == vec.decrease_exponent_to(min(vec.exponents)).ciphertexts(False)


def test_pack_mixed_exponents_round_trip_and_additivity(emu_keys):
    pub, priv = emu_keys(256)
    rng = np.random.RandomState(7)
    a = [float(v) for v in rng.randint(-40, 40, 5) / 8.0] + [int(v) for v in rng.randint(-50, 50, 6)]
    b = [float(v) for v in rng.randint(-40, 40, 11) / 4.0]
    a = [a[i] for i in rng.permutation(11)]
    va, vb = pub.encrypt_batch(a), pub.encrypt_batch(b)
    assert len(set(va.exponents)) > 1
    low = min(va.exponents)
    S, B = 3, 80                                                   # 53-bit mantissas at the common exponent, and headroom
    pa = va.pack(S, B)
    assert len(pa) == 4 and set(pa.exponents) == {low}             # the exponent is carried by the result
    assert pa.ciphertexts(False) == integer_pack(va, S, B)
    assert priv.decrypt_packed(pa, S, B, count=11) == a            # the round trip
    assert priv.decrypt_packed(pa, S, B) == a + [0.0]              # the slot past the end: an encryption of 0
    both = pa + vb.pack(S, B)                                      # packed vectors add slot by slot
    assert priv.decrypt_packed(both, S, B, count=11) == [x + y for x, y in zip(a, b)]
    # the whole vector in one row
    ints_ = [int(v) for v in rng.randint(-2 ** 15, 2 ** 15, 7)]
    vi = pub.encrypt_batch(ints_)
    assert priv.decrypt_packed(vi.pack(7, 17), 7, 17) == ints_


def test_pack_errors_and_empty_vector(emu_keys):
    pub, priv = emu_keys(256)
    vec = pub.encrypt_batch(list(range(10)))
    bound = bound_of(pub)
    for bad in (2.0, "2", None, True, np.float64(2), np.bool_(True)):
        with pytest.raises(TypeError):
            vec.pack(bad, 8)
        with pytest.raises(TypeError):
            vec.pack(2, bad)
        with pytest.raises(TypeError):
            priv.decrypt_packed(vec, bad, 8)
        with pytest.raises(TypeError):
            priv.decrypt_packed(vec, 2, bad)
    for bad in (0, -1):
        with pytest.raises(ValueError):
            vec.pack(bad, 8)
        with pytest.raises(ValueError):
            vec.pack(2, bad)
        with pytest.raises(ValueError):
            priv.decrypt_packed(vec, bad, 8)
        with pytest.raises(ValueError):
            priv.decrypt_packed(vec, 2, bad)
    with pytest.raises(ValueError, match=str(bound)):
        vec.pack(bound + 1, 1)
    with pytest.raises(ValueError, match=str(bound)):
        vec.pack(2, bound // 2 + 1)
    assert len(vec.pack(bound, 1)) == 1                            # the bound itself is allowed
    empty = vec[:0].pack(4, 8)
    assert len(empty) == 0 and empty.ciphertexts(False) == [] and not empty.on_device
    assert priv.decrypt_packed(empty, 4, 8) == []
    packed = vec.pack(5, 8)
    for bad in (-1, 11):
        with pytest.raises(ValueError):
            priv.decrypt_packed(packed, 5, 8, count=bad)
    g = load_golden(1024)
    other_pub = paillier.PaillierPublicKey(H(g["n"]))
    other = paillier.PaillierPrivateKey(other_pub, H(g["p"]), H(g["q"]))
    with pytest.raises(ValueError):
        other.decrypt_packed(packed, 5, 8)                         # the errors of decrypt_batch
    with pytest.raises(TypeError):
        priv.decrypt_packed([1, 2], 5, 8)


# ---- decrypt_packed on plaintexts packed by hand ------------------------------------------------------------------------------
def packed_vector(pub, rows, S, B, exponents=0, rng=None):
    """an EncryptedVector whose row b is raw_encrypt(sum_j rows[b][j] * 2^(B*j) mod n)"""
    rng = rng or random.Random(1)
    cts = pub.raw_encrypt_batch([sum(d << (B * j) for j, d in enumerate(row)) % pub.n for row in rows],
                                [rng.randrange(1, pub.n) for _ in rows])           # (raw_encrypt, all rows in one call)
    return EncryptedVector.from_ciphertexts(pub, cts, exponents)


@pytest.mark.parametrize("bits", [256, 1024])
@pytest.mark.parametrize("B", [1, 5, 63, 64, 65])
def test_decrypt_packed_extreme_slots(emu_keys, bits, B):
    pub, priv = emu_keys(bits)
    S = min(bound_of(pub) // B, 11)
    lo, hi = -(1 << (B - 1)), (1 << (B - 1)) - 1
    rng = random.Random(B)
    rows = [[lo] * S, [hi] * S,
            [lo if j % 2 else hi for j in range(S)], [hi if j % 2 else lo for j in range(S)],   # borrows run the whole length
            [0] * S, [-1 if B > 1 else 0] * S, [0] * (S - 1) + [lo], [lo] + [0] * (S - 1),
            [rng.randint(lo, hi) for _ in range(S)]]
    vec = packed_vector(pub, rows, S, B)
    flat = [d for row in rows for d in row]
    got = priv.decrypt_packed(vec, S, B)
    assert got == flat and all(type(v) is int for v in got)
    assert priv.decrypt_packed(vec[:2], S, B, count=S + 1) == flat[:S + 1]
    assert priv.decrypt_packed(vec[:1], S, B, count=0) == []
    assert priv.decrypt_packed(vec[:1], S, B, Encoding=paillier.EncodedNumber) == flat[:S]


def test_decrypt_packed_floats_and_custom_encoding(emu_keys):
    pub, priv = emu_keys(256)
    S, B = 4, 60
    rows = [[3, -5, 0, (1 << 52) + 1], [-(1 << 59), (1 << 59) - 1, 7, -1]]
    # one exponent for all rows (the vectorised route), one per row (mixed: the row-by-row route); integers beyond 2^53 round as
    # the reference's true division does
    for exps in (-3, [-3, -14], [0, -2]):
        vec = packed_vector(pub, rows, S, B, exps)
        e = exps if isinstance(exps, list) else [exps] * 2
        want = [paillier.EncodedNumber(pub, d % pub.n, e[b]).decode() for b, row in enumerate(rows) for d in row]
        got = priv.decrypt_packed(vec, S, B)
        assert got == want and [type(v) for v in got] == [type(v) for v in want]
    assert priv.decrypt_packed(packed_vector(pub, rows, S, B, -3), S, B)[1] == -5 / 16.0 ** 3

    class Base2(paillier.EncodedNumber):
        BASE = 2
        LOG2_BASE = 1.0

    vec = packed_vector(pub, rows, S, B, -3)
    assert priv.decrypt_packed(vec, S, B, Encoding=Base2) == [d / 8.0 for row in rows for d in row]


def test_decrypt_packed_overflow(emu_keys):
    pub, priv = emu_keys(256)
    S, B = 3, 8
    rng = random.Random(3)
    enc = lambda m: EncryptedVector.from_ciphertexts(pub, [pub.raw_encrypt(m % pub.n, rng.randrange(1, pub.n))], 0)
    top = sum(127 << (B * j) for j in range(S))                    # the largest value three slots of 8 bits hold
    low = sum(-128 << (B * j) for j in range(S))
    assert priv.decrypt_packed(enc(top), S, B) == [127] * 3
    assert priv.decrypt_packed(enc(low), S, B) == [-128] * 3
    for m in (top + 1, low - 1, 1 << (S * B), -(1 << (S * B))):    # a value that needs slot S
        with pytest.raises(OverflowError):
            priv.decrypt_packed(enc(m), S, B)
    for m in (pub.max_int + 1, pub.n - pub.max_int - 1):           # a plaintext in the gap
        with pytest.raises(OverflowError):
            priv.decrypt_packed(enc(m), S, B)
    assert priv.decrypt_packed(enc(top), S + 1, B) == [127] * 3 + [0]


# ---- the device body on the wave emulator -------------------------------------------------------------------------------------
EMU_DIR = os.path.join(ROOT, "tests", "emu")


def build_emu_lib(source, name):
    """tests/emu/<source> built beside libphe_emu.so (same flags as tests/emu/Makefile and the fixture of test_cumsum.py)"""
    src, lib = os.path.join(EMU_DIR, source), os.path.join(EMU_DIR, name)
    csrc = os.path.join(PKG, "csrc")
    deps = [src, os.path.join(EMU_DIR, "wave_emu.h")] + [os.path.join(csrc, h) for h in
                                                         ("mont_core.h", "split_core.h", "segment_core.h", "key_setup.h")]
    if not os.path.exists(lib) or any(os.path.getmtime(d) > os.path.getmtime(lib) for d in deps):
        subprocess.check_call([os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra",
                               "-Wno-unused-parameter", "-Wno-unknown-pragmas", "-o", lib, src, "-lpthread"], cwd=EMU_DIR)
    return ctypes.CDLL(lib)


@pytest.fixture(scope="module")
def pack_lib():
    L = build_emu_lib("emu_pack.cpp", "libphe_emu_pack.so")
    L.emu_pack_last_error.restype = ctypes.c_char_p
    return L


@pytest.fixture(scope="module")
def emu():
    from emu_lib import Emu
    return Emu()


def limbs(xs, words):
    raw = b"".join(int(x).to_bytes(4 * words, "little") for x in xs)
    return np.frombuffer(raw, np.uint32).reshape(len(xs), words).copy()


def ints(arr):
    w = arr.shape[1] * 4
    raw = arr.tobytes()
    return [int.from_bytes(raw[i * w:(i + 1) * w], "little") for i in range(arr.shape[0])]


def P(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None else None


PATTERN = 0xA5C3F00F


# the grid of test_cumsum.py: rung 0 of each key, and the 8-lane rung that serves small batches of a 2048-bit key's rows
@pytest.mark.parametrize("bits, group, geometry", [(1024, 0, (2, 18)), (2048, 0, (4, 18)), (3072, 0, (4, 27)), (2048, 8, (8, 9))])
def test_device_body_on_the_wave_emulator(pack_lib, emu, bits, group, geometry):
    g = load_golden(bits)
    n = H(g["n"])
    n2, s1 = n * n, (n.bit_length() + 31) // 32
    n_arr = limbs([n], s1)[0]
    gl = (ctypes.c_int * 3)()
    assert pack_lib.emu_segment_pack(P(n_arr), s1, group, None, 0, ctypes.c_uint64(0), 1, 1, None, ctypes.c_uint64(0), 1, gl) == 0
    G, L, words = gl
    assert (G, L) == geometry and words == emu.pair_words(n_arr)
    per_wave = 64 // G
    rng = random.Random(bits + group)
    # edge residues among random ones, in the first rows: 1, n^2 - 1, n, and a value above n^2 that still fits the words
    n_max = 3 * (per_wave + 1)
    vals = [rng.randrange(1, n2) for _ in range(n_max)]
    vals[0:4] = [1, n2 - 1, n, (1 << (64 * s1)) - 1]
    residues = limbs(vals, 2 * s1)
    pairs = emu.pair_op(n_arr, 0, residues)

    def run(is_pair, n_rows, S, B, waves):
        tasks = -(-n_rows // S)
        rows = np.ascontiguousarray((pairs if is_pair else residues)[:n_rows])
        out = np.full((tasks + 1, words), PATTERN, np.uint32)      # one row more than the tasks: it must stay as it is
        rc = pack_lib.emu_segment_pack(P(n_arr), s1, group, P(rows), is_pair, ctypes.c_uint64(n_rows), S, B, P(out),
                                       ctypes.c_uint64(tasks), waves, None)
        assert rc == 0, pack_lib.emu_pack_last_error()
        assert np.all(out[tasks] == PATTERN)
        want = []
        for b in range(0, n_rows, S):
            v = 1
            for j, c in enumerate(vals[b:min(b + S, n_rows)]):
                v = v * pow(c, 1 << (B * j), n2) % n2
            want.append(v)
        assert ints(emu.pair_op(n_arr, 1, out[:tasks], group=group)) == want, (is_pair, n_rows, S, B, waves)

    for is_pair in (0, 1):
        run(is_pair, 3, 3, 29, 1)                                  # one task: every other group of the wavefront idle
        run(is_pair, 2, 3, 3, 1)                                   # ... and ragged: its top slot is past the end
        run(is_pair, 1, 1, 1, 1)                                   # one slot: the row itself
        # tasks one more than a wavefront's groups on one wavefront (a second round with one live group), with a ragged last
        # task; then on two wavefronts, the second almost idle
        run(is_pair, 2 * per_wave + 1, 2, 3, 1)
        run(is_pair, 3 * per_wave + 1, 3, 1, 2)
        run(is_pair, 3 * (per_wave + 1), 3, 3, 2)                  # ... and with a full last task
    assert pack_lib.emu_segment_pack(P(n_arr), s1, group, P(residues), 0, ctypes.c_uint64(5), 2, 3, P(pairs), ctypes.c_uint64(2),
                                     1, None) == 3                 # tasks != ceil(n_rows / slots)
