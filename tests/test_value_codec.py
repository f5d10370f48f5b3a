"""The value codec of plain batches on a GPU-less box: the two device bodies (csrc/value_codec.h values_encode_body /
values_decode_body) compiled for the CPU wave emulator against Python integers, and the public interface
(PaillierPublicKey.encrypt_batch, PaillierPrivateKey.decrypt_batch(as_array=...)) on the host and emulator backends, which have
no codec kernels: the host routes.

Expected plaintext rows and exponents come from EncodedNumber.encode, expected values from EncodedNumber.decode
(tests/value_cases.py), expected ciphertexts are (1 + n m) * pow(r, n, n^2) mod n^2: never what the code under test returns."""
import ctypes
import os
import random
import sys

import numpy as np
import pytest

from conftest import PKG, load_golden

if PKG not in sys.path:
    sys.path.insert(0, PKG)

import value_cases as vc  # noqa: E402
from phe import paillier  # noqa: E402
from phe.ciphertext import EncryptedVector  # noqa: E402
from test_pack import EMU_DIR, build_emu_lib  # noqa: E402

H = lambda s: int(s, 16)
PATTERN = 0xA5C3F00F


def P(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None else None


# ---- the device bodies on the wave emulator -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def values_lib():
    lib = os.path.join(EMU_DIR, "libphe_emu_values.so")
    headers = [os.path.join(PKG, "csrc", h) for h in ("slot_codec.h", "value_codec.h")]
    if os.path.exists(lib) and any(os.path.getmtime(h) > os.path.getmtime(lib) for h in headers):
        os.remove(lib)                                                 # (build_emu_lib does not know these two headers)
    L = build_emu_lib("emu_values.cpp", "libphe_emu_values.so")
    L.emu_values_last_error.restype = ctypes.c_char_p
    return L


class EmuCodec:
    """emu_values.cpp for one modulus: encode / decode on `waves` emulated wavefronts, with guard elements behind every output"""

    def __init__(self, L, n, waves=3):
        self.L, self.waves, self.n = L, waves, n
        self.words = (n.bit_length() + 31) // 32
        self.n_arr = vc.to_limbs([n], self.words)[0]
        gk = (ctypes.c_int * 2)()
        assert L.emu_values_geometry(P(self.n_arr), self.words, gk) == 0
        self.G, self.K = gk

    def encode(self, words, kind, exponent, rc=0):
        words = np.ascontiguousarray(words, dtype=np.uint64)
        count = len(words)
        rows = np.full((count + 1, self.words), PATTERN, np.uint32)    # one row more than needed: it must stay as it is
        exps = np.full(count + 1, 0x5A5A5A5A, np.int32) if kind == vc.KIND_FLOAT else None
        status = np.full(count + 1, 0x77, np.uint8)
        got = self.L.emu_values_encode(P(self.n_arr), self.words, P(words), ctypes.c_uint64(count), kind, int(exponent or 0),
                                       P(rows), P(exps), P(status), self.waves)
        assert got == rc, self.L.emu_values_last_error()
        assert np.all(rows[count] == PATTERN) and status[-1] == 0x77 and (exps is None or exps[-1] == 0x5A5A5A5A)
        return rows[:count], None if exps is None else exps[:count], status[:count]

    def decode(self, m_rows, kind, exps, rc=0):
        m_rows = np.ascontiguousarray(m_rows, dtype=np.uint32)
        rows = m_rows.shape[0]
        out = np.full(rows + 1, 0x5A5A5A5A5A5A5A5A, np.uint64)
        status = np.full(rows + 1, 0x77, np.uint8)
        got = self.L.emu_values_decode(P(self.n_arr), self.words, P(m_rows), ctypes.c_uint64(rows), kind, P(exps), P(out), P(status),
                                       self.waves)
        assert got == rc, self.L.emu_values_last_error()
        assert out[-1] == 0x5A5A5A5A5A5A5A5A and status[-1] == 0x77
        return out[:-1], status[:-1]


def modulus(bits):
    return H(load_golden(bits)["n"])


# every (G, K) of host::slot_geometry: the golden keys reach the first five, a crafted modulus of 16384 bits the last
GEOMETRIES = [(256, (16, 1)), (1024, (16, 2)), (2048, (16, 4)), (3072, (64, 2)), (8192, (64, 4)), (16384, (64, 8))]


@pytest.mark.parametrize("bits, geometry", GEOMETRIES)
def test_device_bodies_on_the_wave_emulator(values_lib, bits, geometry):
    n = modulus(bits) if bits <= 8192 else vc.crafted_modulus(bits // 32) + (0x1234567 << 70)
    codec = EmuCodec(values_lib, n, waves=3)
    assert (codec.G, codec.K) == geometry and codec.G * codec.K >= codec.words
    count = 301 if bits <= 3072 else 71
    assert count % (3 * (64 // codec.G)) != 0                          # no multiple of the groups in flight: a ragged last trip
    vc.check_encode(codec.encode, n, seed=bits, count=count)
    vc.check_decode(codec.decode, n, seed=bits + 1, count=count)


@pytest.mark.parametrize("words, geometry", [(8, (16, 1)), (7, (16, 1)), (32, (16, 2)), (31, (16, 2)), (64, (16, 4)), (96, (64, 2))])
def test_borrow_through_every_lane(values_lib, words, geometry):
    """an odd modulus whose middle words are zero: n - mag borrows from word 0 to the top word, across every lane of the group
    (and, for 7 and 31 words, a row width the lanes' pieces do not divide: the word-by-word stores)"""
    n = vc.crafted_modulus(words)
    codec = EmuCodec(values_lib, n, waves=2)
    assert (codec.G, codec.K) == geometry
    rows, _, status = codec.encode(np.array([(-6) & vc.M64, (-5) & vc.M64, (-4) & vc.M64, 6], dtype=np.uint64), vc.KIND_INT64, 0)
    assert vc.to_ints(rows) == [n - 6, n - 5, n - 4, 6] and not status.any()
    assert vc.to_ints(rows)[0] >> 64 == (n >> 64) - 1                  # the borrow reached the top word
    vc.check_encode(codec.encode, n, seed=words, count=70)
    vc.check_decode(codec.decode, n, seed=words + 1, count=70)


def test_device_bodies_refuse_what_the_entry_points_refuse(values_lib):
    codec = EmuCodec(values_lib, modulus(1024))
    words = np.zeros(4, np.uint64)
    codec.encode(words, 4, 0, rc=3)                                    # an unknown kind
    codec.encode(words, vc.KIND_PRECISION, 301, rc=3)
    codec.encode(words, vc.KIND_PRECISION, -301, rc=3)
    m = np.zeros((2, codec.words), np.uint32)
    codec.decode(m, 2, None, rc=3)
    codec.decode(m, vc.OUT_FLOAT, None, rc=3)                          # the float kind needs exponents
    rows = np.zeros((4, codec.words), np.uint32)
    status = np.zeros(4, np.uint8)
    L = values_lib
    assert L.emu_values_encode(P(codec.n_arr), codec.words, P(words), ctypes.c_uint64(4), vc.KIND_FLOAT, 0, P(rows), None, P(status), 1) == 3
    assert L.emu_values_encode(P(codec.n_arr), codec.words, None, ctypes.c_uint64(4), 0, 0, P(rows), None, P(status), 1) == 3
    assert L.emu_values_encode(P(codec.n_arr), codec.words, None, ctypes.c_uint64(0), 0, 0, None, None, None, 1) == 0   # nothing to do
    # keys with max_int < 2^64: 64 bits, and the least width that passes
    small = (1 << 65) + 1
    assert small // 3 - 1 < 1 << 64
    arr = vc.to_limbs([small], 3)[0]
    gk = (ctypes.c_int * 2)()
    assert L.emu_values_geometry(P(arr), 3, gk) == 3
    assert L.emu_values_encode(P(arr), 3, P(words), ctypes.c_uint64(4), 0, 0, P(rows), None, P(status), 1) == 3
    out = np.zeros(2, np.uint64)
    assert L.emu_values_decode(P(arr), 3, P(m), ctypes.c_uint64(2), 0, None, P(out), P(status), 1) == 3
    least = 3 * ((1 << 64) + 1)                                        # max_int = 2^64 exactly
    codec = EmuCodec(values_lib, least | 1 if least % 2 == 0 else least)
    rows, _, status = codec.encode(np.array([vc.M64, 1], dtype=np.uint64), vc.KIND_UINT64, 0)
    assert vc.to_ints(rows) == [vc.M64, 1]


# ---- the public interface on the libgmp and emulator backends (no codec kernels: the host routes) -----------------------------
def _install(backend, monkeypatch):
    if backend == "host":
        import host_backend
        host_backend.install(monkeypatch)
    else:
        import emu_backend
        emu_backend.install(monkeypatch)

    def make(bits):
        g = load_golden(bits)
        pub = paillier.PaillierPublicKey(H(g["n"]))
        return pub, paillier.PaillierPrivateKey(pub, H(g["p"]), H(g["q"]))
    return make


@pytest.fixture(params=["host", "emu"])
def keys(request, monkeypatch):
    return _install(request.param, monkeypatch)


@pytest.fixture
def host_keys(monkeypatch):
    """the libgmp stand-in alone: for the test that encrypts some sixty rows one by one"""
    return _install("host", monkeypatch)


def enc_rows(pub, ms, r=17):
    return [pub.raw_encrypt(m, r + i) for i, m in enumerate(ms)]


def test_the_stand_in_backends_have_no_value_codec(keys):
    pub, priv = keys(256)
    for eng in (pub._get_engine(), priv._get_engine()):
        assert not eng.has_value_codec() and not hasattr(eng.ctx, "values_encode_dev")


def test_the_binding_names_the_entries_and_the_abi():
    from phe import _native
    assert {"phe_hip_values_encode_dev", "phe_hip_values_decode_dev"} <= set(_native.EXPORTED_SYMBOLS)
    assert _native.ABI_VERSION == 14 and _native.lib().phe_hip_abi_version() == 14
    # (another test module may have left a stand-in in _native.Context: the mirrored argument lists are the library handle's)
    L = _native.lib()
    assert len(L.phe_hip_values_encode_dev.argtypes) == 9 and len(L.phe_hip_values_decode_dev.argtypes) == 8


def test_encrypt_batch_keeps_its_bits_and_exponents(keys, monkeypatch):
    """encrypt_batch with and without a precision under fixed r_values: the rows are raw_encrypt(EncodedNumber.encode(v), r),
    whatever VALUE_CODEC_DEVICE_MIN says (these backends have no codec: the host encoding)"""
    from phe import keys as keys_module
    pub, _ = keys(256)
    rng = random.Random(5)
    n, n2 = pub.n, pub.nsquare
    ints = np.array([0, 1, -1, 2 ** 63 - 1, -2 ** 63, 12345, -99999], dtype=np.int64)
    uints = np.array([0, 2 ** 63, 2 ** 64 - 1], dtype=np.uint64)
    floats = np.array([0.0, -0.0, 0.1, -0.1, 5e-324, 1.5, 2.5, -3.75, 1e300], dtype=np.float64)
    cases = [(ints, None), (uints, None), (floats, None), (floats[:8], 1e-6), (floats[:8].tolist(), 2.0 ** -20), (ints.tolist(), None)]
    for minimum in (0, keys_module.VALUE_CODEC_DEVICE_MIN, 1 << 40):
        monkeypatch.setattr(keys_module, "VALUE_CODEC_DEVICE_MIN", minimum)
        for values, precision in cases:
            seq = values.tolist() if isinstance(values, np.ndarray) else values
            rs = [rng.randrange(1, n) for _ in seq]
            want = [paillier.EncodedNumber.encode(pub, v, precision=precision) for v in seq]
            vec = pub.encrypt_batch(values, precision=precision, r_values=rs)
            assert list(vec.exponents) == [e.exponent for e in want]
            assert vec.ciphertexts(False) == [(1 + n * e.encoding) * pow(r, n, n2) % n2 for e, r in zip(want, rs)]
    with pytest.raises(ValueError, match="cannot encode inf / nan"):
        pub.encrypt_batch(np.array([1.0, float("inf")]))


def test_decrypt_batch_as_array_equals_the_list(keys):
    pub, priv = keys(256)
    rng = np.random.RandomState(3)
    ints = np.concatenate([rng.randint(-2 ** 62, 2 ** 62, 20), [2 ** 63 - 1, -2 ** 63, 0]]).astype(np.int64)
    vec = pub.encrypt_batch(ints)
    got = priv.decrypt_batch(vec, as_array=True)
    assert isinstance(got, np.ndarray) and got.dtype == np.int64 and got.tolist() == priv.decrypt_batch(vec) == ints.tolist()
    assert priv.decrypt_batch(vec, as_array=False) == ints.tolist()
    floats = np.concatenate([rng.uniform(-1e6, 1e6, 20), [0.0, -0.0, 5e-324, 0.1, -1e-300]])
    for precision in (None, 1e-6):
        fvec = pub.encrypt_batch(floats[:20] if precision else floats, precision=precision)
        got = priv.decrypt_batch(fvec, as_array=True)
        want = priv.decrypt_batch(fvec)
        assert got.dtype == np.float64 and got.view(np.uint64).tolist() == np.asarray(want, dtype=np.float64).view(np.uint64).tolist()
    assert np.array_equal(priv.decrypt_batch(pub.encrypt_batch(floats)), np.where(floats == 0, 0.0, floats))
    # EncryptedNumbers, the per-device list form, and the empty vector
    numbers = [pub.encrypt(int(v)) for v in ints[:3]]
    assert priv.decrypt_batch(numbers, as_array=True).tolist() == ints[:3].tolist()
    both = priv.decrypt_batch([vec[:5], vec[5:]], as_array=True)
    assert both.dtype == np.int64 and both.tolist() == ints.tolist()
    for empty in (vec[:0], [vec[:0], vec[:0]]):
        got = priv.decrypt_batch(empty, as_array=True)
        assert isinstance(got, np.ndarray) and got.shape == (0,) and got.dtype == np.int64
    assert priv.decrypt_batch([vec[:0], fvec], as_array=True).dtype == np.float64


def test_decrypt_batch_as_array_errors(host_keys):
    pub, priv = host_keys(256)
    n, max_int = pub.n, pub.max_int
    good = [5, n - 7, 0]

    class Base2(paillier.EncodedNumber):
        BASE = 2
        LOG2_BASE = 1.0

    vec = EncryptedVector.from_ciphertexts(pub, enc_rows(pub, good), 0)
    assert priv.decrypt_batch(vec, as_array=True).tolist() == [5, -7, 0]
    with pytest.raises(ValueError, match="Encoding"):
        priv.decrypt_batch(vec, Encoding=Base2, as_array=True)
    assert priv.decrypt_batch(vec, Encoding=paillier.EncodedNumber, as_array=True).tolist() == [5, -7, 0]
    for exps in ([0, -2, 0], 1, [-1, -1, 2]):
        bad = EncryptedVector.from_ciphertexts(pub, enc_rows(pub, good), exps)
        with pytest.raises(ValueError, match="exponents"):
            priv.decrypt_batch(bad, as_array=True)
        assert len(priv.decrypt_batch(bad)) == 3                       # the list form still takes them
    with pytest.raises(ValueError, match="exponents"):
        priv.decrypt_batch([vec, EncryptedVector.from_ciphertexts(pub, enc_rows(pub, good), -3)], as_array=True)
    other = paillier.PaillierPublicKey(H(load_golden(1024)["n"]))
    with pytest.raises(ValueError, match="different key"):
        priv.decrypt_batch(EncryptedVector.from_ciphertexts(other, [1, 2], 0), as_array=True)
    gap, wide = max_int + 1, 1 << 63
    for exponent in (0, -3):
        for ms, error, message in ((good + [gap] + good, OverflowError, "Overflow detected"),
                                   (good + [n - max_int - 1], OverflowError, "Overflow detected")):
            with pytest.raises(error, match=message):
                priv.decrypt_batch(EncryptedVector.from_ciphertexts(pub, enc_rows(pub, ms), exponent), as_array=True)
            with pytest.raises(error, match=message):
                priv.decrypt_batch(EncryptedVector.from_ciphertexts(pub, enc_rows(pub, ms), exponent))
    # an integer outside int64: only the array form minds; the lowest row decides between it and a gap row
    for m in (wide, n - wide - 1, 1 << 64, n - (1 << 70)):
        with pytest.raises(OverflowError, match="int64"):
            priv.decrypt_batch(EncryptedVector.from_ciphertexts(pub, enc_rows(pub, good + [m]), 0), as_array=True)
        as_float = priv.decrypt_batch(EncryptedVector.from_ciphertexts(pub, enc_rows(pub, good + [m]), -2), as_array=True)
        signed = m if m <= max_int else m - n
        assert as_float.dtype == np.float64 and as_float[3] == signed / 256.0
    assert priv.decrypt_batch(EncryptedVector.from_ciphertexts(pub, enc_rows(pub, [n - wide]), 0), as_array=True).tolist() == [-2 ** 63]
    with pytest.raises(OverflowError, match="int64"):
        priv.decrypt_batch(EncryptedVector.from_ciphertexts(pub, enc_rows(pub, good + [wide, gap]), 0), as_array=True)
    with pytest.raises(OverflowError, match="Overflow detected"):
        priv.decrypt_batch(EncryptedVector.from_ciphertexts(pub, enc_rows(pub, good + [gap, wide]), 0), as_array=True)
    # (a decrypted plaintext is below n: the kernels' status 3 is covered at the codec level above)
