"""The slot codec of packed plaintexts on a GPU-less box: the two device bodies (csrc/slot_codec.h slots_pack_body /
slots_unpack_body) compiled for the CPU wave emulator against Python integers, and the public interface
(PaillierPublicKey.encrypt_packed, PaillierPrivateKey.decrypt_packed(as_array=...)) on the emulator backend, which has no codec
kernels: the host packing route.

Expected plaintext rows are Python integers (tests/slots_cases.py), expected ciphertexts are (1 + n V) * pow(r, n, n^2) mod n^2,
expected mantissas come from EncodedNumber.encode: never what the code under test returns."""
import ctypes
import random
import sys

import numpy as np
import pytest

from conftest import PKG, load_golden

if PKG not in sys.path:
    sys.path.insert(0, PKG)

import slots_cases as sc  # noqa: E402
from phe import paillier  # noqa: E402
from phe.ciphertext import EncryptedVector  # noqa: E402
from test_pack import build_emu_lib  # noqa: E402

H = lambda s: int(s, 16)
PATTERN = 0xA5C3F00F


def P(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None else None


# ---- the device bodies on the wave emulator -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def slots_lib():
    L = build_emu_lib("emu_slots.cpp", "libphe_emu_slots.so")
    L.emu_slots_last_error.restype = ctypes.c_char_p
    return L


class EmuCodec:
    """emu_slots.cpp for one key: pack / unpack on `waves` emulated wavefronts, with guard elements behind every output"""

    def __init__(self, L, bits, waves=3):
        self.L, self.waves = L, waves
        self.n = H(load_golden(bits)["n"])
        self.words = (self.n.bit_length() + 31) // 32
        self.n_arr = sc.to_limbs([self.n], self.words)[0]
        gk = (ctypes.c_int * 3)()
        assert L.emu_slots_geometry(P(self.n_arr), self.words, gk) == 0
        self.G, self.K, self.bound = gk

    def pack(self, values, S, B, rc=0):
        values = np.ascontiguousarray(values, dtype=np.int64)
        rows = -(-len(values) // S)
        out = np.full((rows + 1, self.words), PATTERN, np.uint32)      # one row more than needed: it must stay as it is
        got = self.L.emu_slots_pack(P(self.n_arr), self.words, P(values), ctypes.c_uint64(len(values)), S, B, P(out),
                                    ctypes.c_uint64(rows), self.waves)
        assert got == rc, self.L.emu_slots_last_error()
        assert np.all(out[rows] == PATTERN)
        return out[:rows]

    def unpack(self, m_rows, S, B, rc=0):
        m_rows = np.ascontiguousarray(m_rows, dtype=np.uint32)
        rows = m_rows.shape[0]
        values = np.full(rows * S + 1, 0x5A5A5A5A5A5A5A5A, np.int64)
        status = np.full(rows + 1, 0x77, np.uint8)
        got = self.L.emu_slots_unpack(P(self.n_arr), self.words, P(m_rows), ctypes.c_uint64(rows), S, B, P(values), P(status),
                                      self.waves)
        assert got == rc, self.L.emu_slots_last_error()
        assert values[-1] == 0x5A5A5A5A5A5A5A5A and status[-1] == 0x77
        return values[:-1], status[:-1]


@pytest.mark.parametrize("bits, geometry", [(1024, (16, 2)), (2048, (16, 4)), (3072, (64, 2))])
def test_device_bodies_on_the_wave_emulator(slots_lib, bits, geometry):
    codec = EmuCodec(slots_lib, bits)
    assert (codec.G, codec.K) == geometry and codec.bound == sc.bound_of(codec.n)
    assert codec.G * codec.K >= codec.words
    shapes = set()
    for B in sc.B_VALUES:
        for S in sc.slot_counts(codec.n, B):
            sc.check_codec(codec.pack, codec.unpack, codec.n, S, B, seed=bits + B)
            shapes.add((S * B) % 32 != 0)
            shapes.add("small" if S * B < 32 else "wide")
    assert shapes == {True, False, "small", "wide"}                    # S*B off a word boundary and below one word were among them
    # the constant rows the host makes for the kernels, against Python integers
    S, B = 5, 33
    width = codec.G * codec.K
    rows = np.zeros((5, width), np.uint32)
    assert slots_lib.emu_slots_consts(P(codec.n_arr), codec.words, S, B, P(rows)) == 0
    n, max_int, off = codec.n, codec.n // 3 - 1, sc.offset_of(S, B)
    assert sc.to_ints(rows) == [off, n, max_int, n - max_int, (off - n) % (1 << (32 * width))]


@pytest.mark.parametrize("bits", [1024, 3072])
def test_device_bodies_row_counts(slots_lib, bits):
    """0, 1 and S - 1 values, a ragged last row, and more rows than the emulated wavefronts hold groups (several trips)"""
    for waves in (1, 5):
        codec = EmuCodec(slots_lib, bits, waves)
        per_round = waves * (64 // codec.G)
        rng = random.Random(bits + waves)
        for S, B in ((4, 29), (3, 64), (1, 7)):
            lo, hi = -(1 << (B - 1)), (1 << (B - 1)) - 1
            for count in (0, 1, S - 1, 2 * S + 1, 67 * S + S - 1, per_round * S + 1):
                x = [rng.randint(lo, hi) for _ in range(count)]
                rows = -(-count // S)
                got = codec.pack(sc.as_int64(x), S, B)
                padded = x + [0] * (rows * S - count)
                assert sc.to_ints(got) == [sc.pack_int(padded[b * S:(b + 1) * S], B, codec.n) for b in range(rows)], (S, B, count)
                values, status = codec.unpack(got, S, B)
                assert values.tolist() == padded and not status.any(), (S, B, count)


def test_device_bodies_refuse_what_the_entry_points_refuse(slots_lib):
    codec = EmuCodec(slots_lib, 1024)
    x = np.zeros(8, np.int64)
    m = np.zeros((2, codec.words), np.uint32)
    for S, B in ((0, 8), (4, 0), (4, 65), (codec.bound // 8 + 1, 8)):
        rows = 2
        out = np.zeros((rows, codec.words), np.uint32)
        assert slots_lib.emu_slots_pack(P(codec.n_arr), codec.words, P(x), ctypes.c_uint64(8), S, B, P(out), ctypes.c_uint64(rows), 1) == 3
        assert slots_lib.emu_slots_unpack(P(codec.n_arr), codec.words, P(m), ctypes.c_uint64(2), S, B, P(x), P(np.zeros(2, np.uint8)), 1) == 3
    out = np.zeros((3, codec.words), np.uint32)
    assert slots_lib.emu_slots_pack(P(codec.n_arr), codec.words, P(x), ctypes.c_uint64(8), 4, 8, P(out), ctypes.c_uint64(3), 1) == 3
    assert len(codec.pack(x, codec.bound // 8, 8)) == 1                # the bound itself is allowed


# ---- the public interface on the emulator backend (no codec kernels: the host route) ------------------------------------------
@pytest.fixture
def emu_keys(monkeypatch):
    import emu_backend
    emu_backend.install(monkeypatch)

    def make(bits):
        g = load_golden(bits)
        pub = paillier.PaillierPublicKey(H(g["n"]))
        return pub, paillier.PaillierPrivateKey(pub, H(g["p"]), H(g["q"]))
    return make


def expected_rows(pub, mantissas, S, B, rs):
    """raw_encrypt(V_b mod n, r_b) in Python integers, V_b = sum_j x_j 2^(B j)"""
    n, n2 = pub.n, pub.nsquare
    out = []
    for b, r in enumerate(rs):
        V = sum(x << (B * j) for j, x in enumerate(mantissas[b * S:(b + 1) * S]))
        out.append((1 + n * (V % n)) * pow(r, n, n2) % n2)
    return out


@pytest.mark.parametrize("bits", [256, 1024])
def test_encrypt_packed_rows_are_raw_encrypt_of_the_packed_value(emu_keys, bits):
    pub, priv = emu_keys(bits)
    eng = pub._get_engine()
    assert not eng.has_slot_codec() and not hasattr(eng.ctx, "slots_pack_dev")
    rng = random.Random(bits)
    bound = pub.max_int.bit_length() - 1
    shapes = ((4, 16), (1, 9), (3, 1), (bound // 64, 64), (2, 65), (bound // 7, 7)) if bits == 256 else ((bound // 64, 64),)
    for S, B in shapes:
        count = 2 * S + max(1, S - 1)                                  # ragged: the last row lacks a slot (S > 1)
        lo, hi = -(1 << (B - 1)), (1 << (B - 1)) - 1
        x = [rng.randint(lo, hi) for _ in range(count)]
        x[:2] = [lo, hi]
        rows = -(-count // S)
        rs = [rng.randrange(1, pub.n) for _ in range(rows)]
        vec = pub.encrypt_packed(x, S, B, r_values=rs)
        assert isinstance(vec, EncryptedVector) and len(vec) == rows and set(vec.exponents) == {0} and not vec.on_device
        assert vec.ciphertexts(False) == expected_rows(pub, x, S, B, rs), (S, B)
        assert priv.decrypt_packed(vec, S, B, count=count) == x, (S, B)
        if B <= 64 and bits == 256:                                    # the same through numpy: an int64 array, and np integers
            arr = pub.encrypt_packed(np.array(x, dtype=np.int64), np.int64(S), np.int32(B), r_values=rs)
            assert arr.ciphertexts(False) == vec.ciphertexts(False)
    if bits != 256:
        return
    # B = 65 takes the Python-integer route: values beyond int64
    x = [-(1 << 64), (1 << 64) - 1, 12345678901234567890]
    rs = [rng.randrange(1, pub.n) for _ in range(2)]
    vec = pub.encrypt_packed(x, 2, 65, r_values=rs)
    assert vec.ciphertexts(False) == expected_rows(pub, x, 2, 65, rs)
    assert priv.decrypt_packed(vec, 2, 65, count=3) == x
    # fresh obfuscators: not reproducible, but the round trip holds and the rows are marked obfuscated
    vec = pub.encrypt_packed(list(range(-5, 6)), 4, 8)
    assert priv.decrypt_packed(vec, 4, 8, count=11) == list(range(-5, 6))
    assert priv.decrypt_packed(vec, 4, 8) == list(range(-5, 6)) + [0]


def test_encrypt_packed_floats_adds_with_pack_and_scales(emu_keys):
    pub, priv = emu_keys(256)
    rng = np.random.RandomState(5)
    S, B = 5, 40
    x = rng.randint(-1000, 1000, 13) / 64.0
    y = rng.randint(-1000, 1000, 13) / 64.0
    vx = pub.encrypt_packed(x, S, B, precision=2.0 ** -8)
    assert set(vx.exponents) == {-2} and len(vx) == 3
    assert priv.decrypt_packed(vx, S, B, count=13) == x.tolist()      # floats with a precision: the round trip is exact here
    # a packed vector adds slot by slot to what EncryptedVector.pack makes of an ordinary one at the same exponent
    vy = pub.encrypt_batch([float(v) for v in y], precision=2.0 ** -8)
    both = vx + vy.pack(S, B)
    assert priv.decrypt_packed(both, S, B, count=13) == (x + y).tolist()
    assert priv.decrypt_packed(vx * 3, S, B, count=13) == (x * 3).tolist()          # `* k` scales every slot
    ints = [int(v) for v in rng.randint(-2 ** 20, 2 ** 20, 9)]
    vi = pub.encrypt_packed(ints, 4, 32) + pub.encrypt_batch(ints).pack(4, 32)
    assert priv.decrypt_packed(vi, 4, 32, count=9) == [2 * v for v in ints]


def test_encrypt_packed_mantissas_are_those_of_encode(emu_keys):
    pub, priv = emu_keys(256)
    rng = np.random.RandomState(11)
    precision = 2.0 ** -8                                              # exponent -2: the mantissa is round(v * 256)
    ties = np.array([0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 3.5, 1.0, -1.0, 0.0]) / 256.0          # on a rounding tie: half to even
    near = np.array([0.5 + 2.0 ** -40, 0.5 - 2.0 ** -40, -0.5 - 2.0 ** -40, 1e-300, -1e-300]) / 256.0
    x = np.concatenate([ties, near, rng.uniform(-1e4, 1e4, 20), rng.uniform(-1, 1, 20) * 2.0 ** -9])
    want = []
    for v in x.tolist():
        e = paillier.EncodedNumber.encode(pub, v, precision=precision)
        assert e.exponent == -2
        want.append(e.encoding if e.encoding <= pub.max_int else e.encoding - pub.n)
    assert want[:7] == [0, 2, 2, 0, -2, -2, 4]
    S, B = 3, 48
    rows = -(-len(x) // S)
    rs = [int(v) for v in rng.randint(1, 2 ** 31, rows)]
    for values in (x, x.tolist(), [np.float64(v) for v in x]):        # the array, a homogeneous list, and element by element
        vec = pub.encrypt_packed(values, S, B, precision=precision, r_values=rs)
        assert set(vec.exponents) == {-2}
        assert vec.ciphertexts(False) == expected_rows(pub, want, S, B, rs)
    got = priv.decrypt_packed(vec, S, B, count=len(x))
    assert got == [m / 256.0 for m in want]
    # floats without a precision encode each at its own exponent: equal exponents pass, others are refused by index
    same = np.array([1.5, 1.25, -1.75])
    vec = pub.encrypt_packed(same, 3, 60, r_values=[7])
    e = [paillier.EncodedNumber.encode(pub, float(v)) for v in same]
    assert {v.exponent for v in e} == set(vec.exponents) and len(set(vec.exponents)) == 1
    signed = [v.encoding if v.encoding <= pub.max_int else v.encoding - pub.n for v in e]
    assert vec.ciphertexts(False) == expected_rows(pub, signed, 3, 60, [7])
    for values in (np.array([1.5, 1.25, 1000.0, 2000.0]), [1.5, 1.25, 1000.0, 2000.0], [1.5, 1.25, np.float64(1000.0)]):
        with pytest.raises(ValueError, match="index 2"):
            pub.encrypt_packed(values, 2, 60)
    with pytest.raises(ValueError, match="index 1"):
        pub.encrypt_packed([1, 2.5], 2, 60)                            # an int and a float: exponents 0 and -13


def test_encrypt_packed_errors_and_empty(emu_keys):
    pub, priv = emu_keys(256)
    bound = pub.max_int.bit_length() - 1
    x = list(range(10))
    for bad in (2.0, "2", None, True, np.float64(2), np.bool_(True)):
        with pytest.raises(TypeError, match="slots must be an integer"):
            pub.encrypt_packed(x, bad, 8)
        with pytest.raises(TypeError, match="slot_bits must be an integer"):
            pub.encrypt_packed(x, 2, bad)
    for bad in (0, -1):
        with pytest.raises(ValueError, match="slots must be at least 1"):
            pub.encrypt_packed(x, bad, 8)
        with pytest.raises(ValueError, match="slot_bits must be at least 1"):
            pub.encrypt_packed(x, 2, bad)
    # the bound of pack(), with its message
    vec = pub.encrypt_batch(x)
    for S, B in ((bound + 1, 1), (2, bound // 2 + 1)):
        with pytest.raises(ValueError) as theirs:
            vec.pack(S, B)
        with pytest.raises(ValueError) as ours:
            pub.encrypt_packed(x, S, B)
        assert str(ours.value) == str(theirs.value) and str(bound) in str(ours.value)
    assert len(pub.encrypt_packed([0, -1] * 5, bound, 1)) == 1        # the bound itself is allowed
    # a mantissa outside the slot, by index: arrays, lists, Python integers beyond int64
    for values in ([1, 2, 128, 300], np.array([1, 2, 128, 300]), [1, 2, 128, 1 << 70]):
        with pytest.raises(ValueError, match="index 2"):
            pub.encrypt_packed(values, 2, 8)
    with pytest.raises(ValueError, match="index 1"):
        pub.encrypt_packed(np.array([0, -129, 500]), 2, 8)
    assert len(pub.encrypt_packed([127, -128], 2, 8)) == 1
    with pytest.raises(ValueError, match="index 0"):
        pub.encrypt_packed([0.75], 1, 8, precision=1.0 / 4096)         # mantissa 0.75 * 4096 = 3072
    with pytest.raises(ValueError):
        pub.encrypt_packed([float("inf")], 1, 8, precision=0.5)
    with pytest.raises(ValueError, match="r_values"):
        pub.encrypt_packed(x, 4, 8, r_values=[3, 5])                   # three rows
    for empty in ([], np.zeros(0, np.int64), np.zeros(0)):
        vec = pub.encrypt_packed(empty, 4, 8)
        assert len(vec) == 0 and vec.ciphertexts(False) == [] and not vec.on_device
        assert priv.decrypt_packed(vec, 4, 8) == []
    one = pub.encrypt_packed([5, -6, 7], 1, 8, r_values=[2, 3, 4])     # slots == 1: the values themselves
    assert one.ciphertexts(False) == pub.raw_encrypt_batch([5, -6 % pub.n, 7], [2, 3, 4])


def test_decrypt_packed_as_array(emu_keys):
    pub, priv = emu_keys(256)
    rng = np.random.RandomState(3)
    S, B = 6, 20
    x = rng.randint(-2 ** 19, 2 ** 19, 20)
    vec = pub.encrypt_packed(x, S, B)
    got = priv.decrypt_packed(vec, S, B, as_array=True)
    assert isinstance(got, np.ndarray) and got.dtype == np.int64 and got.shape == (24,)
    assert got.tolist() == x.tolist() + [0] * 4
    got = priv.decrypt_packed(vec, S, B, count=20, as_array=True)
    assert got.dtype == np.int64 and np.array_equal(got, x)
    assert priv.decrypt_packed(vec, S, B, count=0, as_array=True).shape == (0,)
    assert priv.decrypt_packed(vec, S, B, count=20, as_array=False) == x.tolist()
    f = x / 256.0
    fvec = pub.encrypt_packed(f, S, B, precision=2.0 ** -8)
    got = priv.decrypt_packed(fvec, S, B, count=20, as_array=True)
    assert got.dtype == np.float64 and np.array_equal(got, f)
    empty = priv.decrypt_packed(vec[:0], S, B, as_array=True)
    assert isinstance(empty, np.ndarray) and empty.shape == (0,)
    # where the array form does not apply
    wide = pub.encrypt_packed([1, 2, 3], 3, 65)
    with pytest.raises(ValueError, match="slot_bits"):
        priv.decrypt_packed(wide, 3, 65, as_array=True)

    class Base2(paillier.EncodedNumber):
        BASE = 2
        LOG2_BASE = 1.0

    with pytest.raises(ValueError, match="Encoding"):
        priv.decrypt_packed(vec, S, B, Encoding=Base2, as_array=True)
    mixed = EncryptedVector.from_ciphertexts(pub, vec.ciphertexts(False), [0, -2, 0, 0])
    with pytest.raises(ValueError, match="exponents"):
        priv.decrypt_packed(mixed, S, B, as_array=True)
    assert len(priv.decrypt_packed(mixed, S, B)) == 24                 # the list form still takes them
    up = EncryptedVector.from_ciphertexts(pub, vec.ciphertexts(False), 1)
    with pytest.raises(ValueError, match="exponents"):
        priv.decrypt_packed(up, S, B, as_array=True)
    # the errors of the list form, in the array form: the overflow gap and a value that does not fit
    enc = lambda m: EncryptedVector.from_ciphertexts(pub, [pub.raw_encrypt(m % pub.n, 17)], 0)
    with pytest.raises(OverflowError, match="Overflow detected"):
        priv.decrypt_packed(enc(pub.max_int + 1), S, B, as_array=True)
    with pytest.raises(OverflowError, match="does not fit"):
        priv.decrypt_packed(enc(1 << (S * B)), S, B, as_array=True)


def test_federated_example_packed_matches_plaintext(emu_keys, monkeypatch):
    """examples/federated_learning_batched.py run_packed: gradients quantised to 2^-32, packed, added and unpacked reproduce the
    plaintext aggregation to the quantisation step.  Bound: every entry of the mean gradient is off by at most 2^-33, the weights
    after two rounds by 1.5 * 2 * 2^-33 < 4e-10 each, a prediction (11 features below 0.2 in size) by < 1e-9 and the mean squared
    error (residuals of a few hundred) by < 1e-6 of about 2e4: rtol 1e-8 leaves two orders of magnitude."""
    import os
    from conftest import ROOT
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import federated_learning_batched as fed
    from test_federated_example import plaintext_rounds
    errors, _ = fed.run_packed(key_length=256, n_rounds=2, verbose=False)
    assert np.allclose(errors, plaintext_rounds(2), rtol=1e-8)
