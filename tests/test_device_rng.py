"""The device draw of the short obfuscator exponents (enable_short_obfuscators(device_rng=True)) on a GPU-less box: the ChaCha20
keystream rows of csrc/chacha_rows.h compiled for the CPU wave emulator (tests/emu/emu_chacha.cpp), the numpy expander
phe/_chacha.py, and the public methods on the emulator backends of tests/test_short_obfuscators.py.

The yardstick is the scalar block function below, written from the pseudocode of RFC 8439 section 2.3.1 with Python integers; it
shares no code with phe/_chacha.py or the device header.  The known answer is the block of RFC 8439 section 2.3.2."""
import ctypes
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from conftest import PKG, load_golden

if PKG not in sys.path:
    sys.path.insert(0, PKG)

from phe import _chacha, _engine, keys, paillier  # noqa: E402
from phe.ciphertext import EncryptedVector  # noqa: E402

from short_cases import X_FIXED, Obfuscators, base_of, ints  # noqa: E402
from test_short_obfuscators import encodings, resident_emulator_context  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
EMU_DIR = os.path.join(HERE, "emu")
H = lambda s: int(s, 16)
M32 = 0xFFFFFFFF
PATTERN = 0xA5C3F00F

RFC_KEY = bytes(range(32))
RFC_NONCE = (0x09000000, 0x4A000000, 0x00000000)
RFC_BLOCK = [int(w, 16) for w in ("e4e7f110 15593bd1 1fdd0f50 c47120a3 c7f4d1c7 0368c033 9aaa2204 4e6cd4c3 "
                                  "466482d2 09aa9f07 05d7c214 a2028bd9 d19c12b5 b94e16de e883d0cb 4e3c50a2").split()]

LAYOUTS = [(1, 1), (31, 1), (64, 2), (500, 16), (512, 16), (513, 17), (1000, 32), (1024, 32), (1536, 48), (1024, 34)]
ROWS = [1, 63, 64, 65, 1000]


# ---- the yardstick: RFC 8439 section 2.3.1, one block, Python integers -------------------------------------------------------
def scalar_block(key_words, nonce_words, counter):
    def rotl(v, k):
        return ((v << k) & M32) | (v >> (32 - k))

    def quarter(s, a, b, c, d):
        s[a] = (s[a] + s[b]) & M32; s[d] = rotl(s[d] ^ s[a], 16)
        s[c] = (s[c] + s[d]) & M32; s[b] = rotl(s[b] ^ s[c], 12)
        s[a] = (s[a] + s[b]) & M32; s[d] = rotl(s[d] ^ s[a], 8)
        s[c] = (s[c] + s[d]) & M32; s[b] = rotl(s[b] ^ s[c], 7)

    state = [0x61707865, 0x3320646E, 0x79622D32, 0x6B206574] + list(key_words) + [counter & M32] + list(nonce_words)
    s = list(state)
    for _ in range(10):
        quarter(s, 0, 4, 8, 12); quarter(s, 1, 5, 9, 13); quarter(s, 2, 6, 10, 14); quarter(s, 3, 7, 11, 15)
        quarter(s, 0, 5, 10, 15); quarter(s, 1, 6, 11, 12); quarter(s, 2, 7, 8, 13); quarter(s, 3, 4, 9, 14)
    return [(a + b) & M32 for a, b in zip(s, state)]


def key_words(key):
    return [int.from_bytes(key[4 * i:4 * i + 4], "little") for i in range(8)]


def scalar_rows(key, nonce, counter0, bits, limbs, row_numbers):
    """the rows `row_numbers` of the layout, as Python integers per word"""
    B = -(-limbs // 16)
    kw = key_words(key)
    out = []
    for i in row_numbers:
        words = []
        for k in range(B):
            words += scalar_block(kw, nonce, counter0 + i * B + k)
        value = sum(w << (32 * j) for j, w in enumerate(words[:limbs])) & ((1 << bits) - 1)
        out.append([(value >> (32 * j)) & M32 for j in range(limbs)])
    return out


def P(a):
    return a.ctypes.data_as(ctypes.c_void_p)


@pytest.fixture(scope="module")
def chacha_lib():
    src, lib = os.path.join(EMU_DIR, "emu_chacha.cpp"), os.path.join(EMU_DIR, "libphe_emu_chacha.so")
    deps = [src, os.path.join(EMU_DIR, "wave_emu.h"), os.path.join(PKG, "csrc", "chacha_rows.h")]
    if not os.path.exists(lib) or any(os.path.getmtime(d) > os.path.getmtime(lib) for d in deps):
        subprocess.check_call([os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra",
                               "-Wno-unused-parameter", "-Wno-unknown-pragmas", "-o", lib, src, "-lpthread"], cwd=EMU_DIR)
    return ctypes.CDLL(lib)


def emulated(L, key, nonce, counter0, bits, limbs, rows, waves=3, rc=0):
    """the device body on `waves` emulated wavefronts, with a guard row behind the output"""
    out = np.full((rows + 1, limbs), PATTERN, np.uint32)
    k = np.array(key_words(key), np.uint32)
    v = np.array(nonce, np.uint32)
    got = L.emu_chacha20_rows(P(k), P(v), ctypes.c_uint32(counter0), bits, limbs, P(out), ctypes.c_uint64(rows), waves)
    assert got == rc
    assert np.all(out[rows] == PATTERN)                                 # nothing behind the last row was written
    return out[:rows]


# ---- known answer ------------------------------------------------------------------------------------------------------------
def test_known_answer_rfc8439(chacha_lib):
    assert scalar_block(key_words(RFC_KEY), RFC_NONCE, 1) == RFC_BLOCK
    assert _chacha.chacha20_blocks(RFC_KEY, RFC_NONCE, 1, 1)[0].tolist() == RFC_BLOCK
    assert _chacha.chacha20_rows(RFC_KEY, RFC_NONCE, 1, 512, 16, 1)[0].tolist() == RFC_BLOCK
    assert emulated(chacha_lib, RFC_KEY, RFC_NONCE, 1, 512, 16, 1)[0].tolist() == RFC_BLOCK


def test_keystream_against_openssl():
    exe = shutil.which("openssl")
    if exe is None:
        pytest.skip("no openssl binary")
    # openssl's 16-byte IV is the 32-bit little-endian counter followed by the 96-bit nonce
    iv = (1).to_bytes(4, "little") + b"".join(w.to_bytes(4, "little") for w in RFC_NONCE)
    run = subprocess.run([exe, "enc", "-chacha20", "-K", RFC_KEY.hex(), "-iv", iv.hex()], input=bytes(256), capture_output=True)
    if run.returncode != 0 or len(run.stdout) != 256:
        pytest.skip("this openssl has no chacha20 stream cipher")
    want = np.frombuffer(run.stdout, "<u4").astype(np.uint32).reshape(4, 16)
    assert want[0].tolist() == RFC_BLOCK
    assert np.array_equal(_chacha.chacha20_blocks(RFC_KEY, RFC_NONCE, 1, 4), want)
    kw = key_words(RFC_KEY)
    assert [scalar_block(kw, RFC_NONCE, 1 + k) for k in range(4)] == want.tolist()


# ---- layout, masking, bounds -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits, limbs", LAYOUTS)
def test_layout_masking_and_bounds(chacha_lib, bits, limbs):
    key = bytes((7 * i + bits) & 0xFF for i in range(32))
    nonce = (bits, 0x01020304, limbs)
    counter0 = 5
    for rows in ROWS:
        dev = emulated(chacha_lib, key, nonce, counter0, bits, limbs, rows)
        host = _chacha.chacha20_rows(key, nonce, counter0, bits, limbs, rows)
        assert host.shape == (rows, limbs) and host.dtype == np.uint32
        assert np.array_equal(dev, host)
        picked = sorted({0, rows // 2, rows - 1})
        assert dev[picked].tolist() == scalar_rows(key, nonce, counter0, bits, limbs, picked)
        if rows <= 65:
            assert dev.tolist() == scalar_rows(key, nonce, counter0, bits, limbs, range(rows))
        # masking: every value below 2^bits, limbs above ceil(bits / 32) zero
        top = (bits - 1) // 32
        assert not dev[:, top + 1:].any()
        assert int(dev[:, top].max()) < 1 << (bits - 32 * top)
        assert all(v < 1 << bits for v in ints(dev[:3]))
    # the tail of a row's last block is thrown away: a row depends on its number alone, not on what the row before left
    B = -(-limbs // 16)
    again = _chacha.chacha20_rows(key, nonce, counter0 + 3 * B, bits, limbs, 4)
    assert np.array_equal(again, _chacha.chacha20_rows(key, nonce, counter0, bits, limbs, 7)[3:])


@pytest.mark.parametrize("bits, limbs, rows", [(1024, 32, 5), (513, 17, 64), (31, 1, 65)])
def test_counter_reaches_its_end_but_never_wraps(chacha_lib, bits, limbs, rows):
    B = -(-limbs // 16)
    last = (1 << 32) - rows * B                                         # the last block of the call is block 2^32 - 1
    dev = emulated(chacha_lib, RFC_KEY, RFC_NONCE, last, bits, limbs, rows)
    assert np.array_equal(dev, _chacha.chacha20_rows(RFC_KEY, RFC_NONCE, last, bits, limbs, rows))
    assert dev.tolist() == scalar_rows(RFC_KEY, RFC_NONCE, last, bits, limbs, range(rows))
    emulated(chacha_lib, RFC_KEY, RFC_NONCE, last + 1, bits, limbs, rows, rc=3)
    with pytest.raises(ValueError):
        _chacha.chacha20_rows(RFC_KEY, RFC_NONCE, last + 1, bits, limbs, rows)


def test_arguments_refused(chacha_lib):
    for bits, limbs in ((0, 1), (33, 1), (1025, 32), (-1, 4)):
        emulated(chacha_lib, RFC_KEY, RFC_NONCE, 0, bits, limbs, 2, rc=3)
        with pytest.raises(ValueError):
            _chacha.chacha20_rows(RFC_KEY, RFC_NONCE, 0, bits, limbs, 2)
    assert emulated(chacha_lib, RFC_KEY, RFC_NONCE, 0, 64, 2, 0).shape == (0, 2)
    assert _chacha.chacha20_rows(RFC_KEY, RFC_NONCE, 0, 64, 2, 0).shape == (0, 2)
    with pytest.raises(ValueError):
        _chacha.chacha20_rows(RFC_KEY[:31], RFC_NONCE, 0, 64, 2, 1)


# ---- the public interface on the emulator backends -------------------------------------------------------------------------------
class Seeds:
    """_engine.fresh_seed patched to record the bytearrays it hands out (still read from the real /dev/urandom), and
    random_bits_limbs to count — or refuse — the host draws"""

    def __init__(self, monkeypatch):
        self.handed, self.copies, self.host_draws, self.refuse = [], [], 0, False
        real_seed, real_bits = _engine.fresh_seed, _engine.random_bits_limbs

        def fresh_seed():
            seed = real_seed()
            assert isinstance(seed, bytearray) and len(seed) == 32
            self.handed.append(seed)
            self.copies.append(bytes(seed))
            return seed

        def random_bits_limbs(bits, count, limbs_, out=None):
            assert not self.refuse, "a batch route drew through random_bits_limbs"
            self.host_draws += 1
            return real_bits(bits, count, limbs_, out)
        monkeypatch.setattr(_engine, "fresh_seed", fresh_seed)
        monkeypatch.setattr(_engine, "random_bits_limbs", random_bits_limbs)

    def rhos(self, k, bits, count):
        """the exponents seed number k expands to"""
        return ints(_chacha.chacha20_rows(self.copies[k], (0, 0, 0), 0, bits, (bits + 31) // 32, count))

    def check_wiped(self):
        assert all(not any(seed) for seed in self.handed)               # overwritten once the call has returned
        assert all(any(c) for c in self.copies) and len(set(self.copies)) == len(self.copies)     # and never used twice


def make_keys(bits=256):
    g = load_golden(bits)
    pub = paillier.PaillierPublicKey(H(g["n"]))
    return pub, paillier.PaillierPrivateKey(pub, H(g["p"]), H(g["q"]))


def test_flag_and_property(monkeypatch):
    import emu_backend
    emu_backend.install(monkeypatch)
    pub, _ = make_keys()
    assert pub.short_obfuscator_device_rng is False
    pub.enable_short_obfuscators(x=X_FIXED)
    assert pub.short_obfuscator_device_rng is False and not pub._get_engine().short_device_rng()      # off by default
    pub.enable_short_obfuscators(x=X_FIXED, device_rng=True)
    assert pub.short_obfuscator_device_rng is True and pub._get_engine().short_device_rng()
    other = paillier.PaillierPublicKey(pub.n)
    assert other == pub and hash(other) == hash(pub)                     # not part of the key
    import pickle
    assert pickle.loads(pickle.dumps(pub)).short_obfuscator_device_rng is False
    with pytest.raises(AttributeError):
        pub.short_obfuscator_device_rng = False
    pub.disable_short_obfuscators()
    assert pub.short_obfuscator_device_rng is False and not pub._get_engine().short_device_rng()
    pub.enable_short_obfuscators(x=X_FIXED)                               # and it does not come back by itself
    assert pub.short_obfuscator_device_rng is False


def test_batches_on_the_emulator_backend(monkeypatch):
    """the backend without resident rows: encrypt_batch and whole-vector obfuscate draw through the host expander"""
    import emu_backend
    emu_backend.install(monkeypatch)
    pub, priv = make_keys()
    n, n2 = pub.n, pub.nsquare
    h, hs = base_of(n)
    obf = Obfuscators(hs, n)
    seeds = Seeds(monkeypatch)
    pub.enable_short_obfuscators(bits=40, x=X_FIXED, device_rng=True)
    seeds.refuse = True
    values = [5, -6, 0.75, 1e-3, 7]
    ms = encodings(pub, values)
    vec = pub.encrypt_batch(values)
    assert len(seeds.handed) == 1
    rho = seeds.rhos(0, 40, len(values))
    assert vec.ciphertexts(False) == [(1 + n * m) * obf(r) % n2 for m, r in zip(ms, rho)]
    assert vec.ciphertexts(False) == pub.raw_encrypt_batch(ms, r_values=[pow(h, r, n) for r in rho])
    assert priv.decrypt_batch(vec) == values
    again = pub.encrypt_batch(values)                                    # a second call: another seed, other ciphertexts
    assert len(seeds.handed) == 2
    assert again.ciphertexts(False) == [(1 + n * m) * obf(r) % n2 for m, r in zip(ms, seeds.rhos(1, 40, len(values)))]
    assert again.ciphertexts(False) != vec.ciphertexts(False)
    cs = [12345, n2 - 2, 99]
    plain = EncryptedVector.from_ciphertexts(pub, cs)
    assert plain.obfuscate().ciphertexts(False) == [c * obf(r) % n2 for c, r in zip(cs, seeds.rhos(2, 40, 3))]
    seeds.check_wiped()
    # the scalar call reads its 128 bytes directly
    seeds.refuse = False
    one = pub.encrypt(41)
    assert seeds.host_draws == 1 and len(seeds.handed) == 3 and priv.decrypt(one) == 41
    # explicit exponents are what they were
    assert pub.encrypt_batch(values, rho_values=rho).ciphertexts(False) == vec.ciphertexts(False)
    assert len(seeds.handed) == 3
    # device_rng off: the host draw, no seed
    pub.enable_short_obfuscators(bits=40, x=X_FIXED)
    pub.encrypt_batch(values)
    assert seeds.host_draws == 2 and len(seeds.handed) == 3


def test_chunked_routes_on_the_resident_emulator_backend(monkeypatch):
    """the backend with resident rows and no keystream kernel: raw_encrypt_fresh, the pool and short_fresh_dev draw a seed per
    chunk and upload what the host expander makes of it"""
    from phe import _native
    monkeypatch.setattr(_native, "Context", resident_emulator_context())
    monkeypatch.setattr(keys, "SCALAR_POOL_REFILL", 4)
    pub, priv = make_keys()
    n, n2 = pub.n, pub.nsquare
    _, hs = base_of(n)
    obf = Obfuscators(hs, n)
    seeds = Seeds(monkeypatch)
    pub.enable_short_obfuscators(bits=48, x=X_FIXED, device_rng=True)
    eng = pub._get_engine()
    assert not hasattr(eng.ctx, "chacha20_rows_dev")
    seeds.refuse = True
    values = [3.0, -4.0, 5.5, 6.0, 7.0]
    ms = encodings(pub, values)
    vec = pub.encrypt_batch(np.array(values), device=True)               # (an array, too many rows for the scalar refill)
    assert len(seeds.handed) == 1
    assert vec.ciphertexts(False) == [(1 + n * m) * obf(r) % n2 for m, r in zip(ms, seeds.rhos(0, 48, 5))]
    assert priv.decrypt_batch(vec.to_host()) == values                    # (the stand-in context has no resident decrypt)
    # the pool, then the batch that consumes it
    assert pub.precompute_obfuscators(7) == 7 and len(seeds.handed) == 2
    pool = [obf(r) for r in seeds.rhos(1, 48, 7)]
    assert eng.peek_obfuscators(7) == pool
    vec = pub.encrypt_batch(np.array(values))
    assert vec.ciphertexts(False) == [(1 + n * m) * o % n2 for m, o in zip(ms, pool)]
    assert pub.obfuscators_available() == 2 and len(seeds.handed) == 2
    pub.discard_obfuscators()
    # whole-vector obfuscation of resident rows
    cs = [12345, n2 - 2, 99, 4, 5, 6]
    got = eng.short_fresh_dev(len(cs), mul=eng.upload_cipher(cs))
    assert len(seeds.handed) == 3
    assert eng.to_ints(got.to_host()) == [c * obf(r) % n2 for c, r in zip(cs, seeds.rhos(2, 48, len(cs)))]
    seeds.check_wiped()
    # a part of the vector keeps the host draw
    seeds.refuse = False
    got = eng.to_ints(eng.short_fresh_dev(len(cs), mul=eng.upload_cipher(cs), rows=[1, 4]).to_host())
    assert seeds.host_draws == 1 and len(seeds.handed) == 3
    assert [g == c for g, c in zip(got, cs)] == [True, False, True, True, False, True]


def test_random_bits_dev_cuts_a_draw_that_would_wrap(monkeypatch):
    """more blocks than one counter holds: parts, each under its own seed (the arithmetic only: nothing that large is drawn)"""
    assert _engine._seeded_parts(10, 32) == [(0, 10)]
    parts = _engine._seeded_parts((1 << 31) + 5, 32)
    assert parts == [(0, 1 << 31), (1 << 31, (1 << 31) + 5)]
    assert all((hi - lo) * 2 <= 1 << 32 for lo, hi in parts)
    assert _engine._seeded_parts((1 << 32) // 3 + 1, 34)[0][1] * 3 <= 1 << 32
    assert _engine._seeded_parts(0, 16) == []


def test_a_seed_comes_from_the_kernel_csprng_alone(monkeypatch):
    reads = []
    real = _engine._urandom_into

    def recording(view):
        real(view)
        reads.append(len(memoryview(view).cast("B")))
    monkeypatch.setattr(_engine, "_urandom_into", recording)
    a, b = _engine.fresh_seed(), _engine.fresh_seed()
    assert reads == [32, 32] and isinstance(a, bytearray) and len(a) == 32 and a != b and any(a)
    rows = _engine.seeded_bits_limbs(100, 9, 4)
    assert reads == [32, 32, 32] and rows.shape == (9, 4) and len({tuple(r) for r in rows.tolist()}) == 9
    assert int(rows[:, 3].max()) < 1 << 4
