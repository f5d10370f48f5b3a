"""Short-exponent obfuscators (PaillierPublicKey.enable_short_obfuscators: h_s^rho for h = -x^2 mod n, h_s = h^n mod n^2 and a
short random rho, instead of r^n) on a GPU-less box: the public methods on the emulator backend (which has no comb kernel: the
composition powmod of the broadcast h_s, then add_plain / raw_add), the exponent draw, and the device body itself
(csrc/fixed_base.h fixed_base_pow_body) compiled for the CPU wave emulator.

Expected values are Python integers (tests/short_cases.py): the obfuscator pow(h_s, rho, n^2), the encryption
(1 + n*m) * pow(h_s, rho, n^2) mod n^2 — which is the reference's raw_encrypt(m, r_value=pow(h, rho, n)),
phe/paillier.py:102-139 — and the re-randomisation c * pow(h_s, rho, n^2) mod n^2: never what the code under test returns."""
import ctypes
import os
import pickle
import random
import subprocess
import sys

import numpy as np
import pytest

from conftest import PKG, ROOT, load_golden

if PKG not in sys.path:
    sys.path.insert(0, PKG)

from phe import _engine, keys, paillier  # noqa: E402
from phe.ciphertext import EncryptedVector  # noqa: E402

from short_cases import X_FIXED, Obfuscators, base_of, comb_table, edge_exponents, ints, limbs  # noqa: E402

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


def encodings(pub, values):
    return [paillier.EncodedNumber.encode(pub, v).encoding for v in values]


# ---- the public methods on the emulator backend -----------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [256, 1024])
def test_public_api_on_the_emulator_backend(emu_keys, bits):
    pub, priv = emu_keys(bits)
    n, n2 = pub.n, pub.nsquare
    h, hs = base_of(n)
    assert pub.short_obfuscator_base is None and pub.short_obfuscator_bits is None
    assert pub.enable_short_obfuscators(x=X_FIXED) == hs
    assert pub.short_obfuscator_base == hs and pub.short_obfuscator_bits == bits // 2
    eng = pub._get_engine()
    assert eng.short_base() == (hs, bits // 2) and not eng.has_fixed_base()      # no kernel on this backend: the composition
    assert eng.short_table_info() == {"bits": 0, "window": 0, "positions": 0, "table_bytes": 0}
    obf = Obfuscators(hs, n)
    values = [0, 1, -1, 2.5, -3.25, 123456789, -(1 << 40), 1e-3, 7]
    rhos = edge_exponents(bits // 2, 4, count=len(values))
    ms = encodings(pub, values)
    want = [(1 + n * m) * obf(r) % n2 for m, r in zip(ms, rhos)]
    vec = pub.encrypt_batch(values, rho_values=rhos)
    assert vec.ciphertexts(False) == want
    assert want == pub.raw_encrypt_batch(ms, r_values=[pow(h, r, n) for r in rhos])     # the reference's raw_encrypt with r = h^rho
    assert priv.decrypt_batch(vec) == values
    # the exponents as limb rows
    el = (bits // 2 + 31) // 32
    assert pub.encrypt_batch(values, rho_values=limbs(rhos, el)).ciphertexts(False) == want
    # encrypt_packed: one exponent per packed row
    ints_ = [3, -4, 5, -6, 7, 100, -128]
    S, B = 3, 8
    packed = pub.encrypt_packed(ints_, S, B, rho_values=rhos[:3])
    rows = [sum(x << (B * j) for j, x in enumerate(ints_[b:b + S])) % n for b in range(0, len(ints_), S)]
    assert packed.ciphertexts(False) == [(1 + n * m) * obf(r) % n2 for m, r in zip(rows, rhos[:3])]
    assert priv.decrypt_packed(packed, S, B, count=len(ints_)) == ints_
    # obfuscate: every row times its h_s^rho
    rng = random.Random(bits)
    cs = [rng.randrange(1, n2) for _ in range(4)]
    plain = EncryptedVector.from_ciphertexts(pub, cs)
    assert plain.obfuscate(rho_values=rhos[2:6]) is plain
    assert plain.ciphertexts(False) == [c * obf(r) % n2 for c, r in zip(cs, rhos[2:6])]
    # the same table of obfuscators from a ready h_s
    pub.disable_short_obfuscators()
    assert pub.short_obfuscator_base is None and pub._get_engine().short_base() is None
    assert pub.enable_short_obfuscators(hs=hs) == hs
    assert pub.encrypt_batch(values, rho_values=rhos).ciphertexts(False) == want
    # off again: the reference's obfuscators, bit for bit
    pub.disable_short_obfuscators()
    r = [rng.randrange(1, n) for _ in values[:3]]
    got = pub.encrypt_batch(values[:3], r_values=r).ciphertexts(False)
    assert got == [(1 + n * m) * pow(rv, n, n2) % n2 for m, rv in zip(ms, r)]


def test_fresh_draws_on_the_emulator_backend(emu_keys, monkeypatch):
    """every freshly drawn obfuscator is h_s^rho for the rho that random_bits_limbs returned"""
    pub, priv = emu_keys(256)
    n, n2 = pub.n, pub.nsquare
    _, hs = base_of(n)
    pub.enable_short_obfuscators(bits=40, x=X_FIXED)
    drawn = []
    real = _engine.random_bits_limbs

    def recording(bits, count, limbs_, out=None):
        got = real(bits, count, limbs_, out)
        assert bits == 40 and limbs_ == 2
        drawn.extend(ints(got))
        return got
    monkeypatch.setattr(_engine, "random_bits_limbs", recording)
    obf = Obfuscators(hs, n)
    values = [5, -6, 0.75]
    ms = encodings(pub, values)
    vec = pub.encrypt_batch(values)
    assert len(drawn) == 3 and len(set(drawn)) == 3
    assert vec.ciphertexts(False) == [(1 + n * m) * obf(r) % n2 for m, r in zip(ms, drawn)]
    assert priv.decrypt_batch(vec) == values
    one = pub.encrypt(41)                                                        # scalar encrypt
    assert one.ciphertext(False) == (1 + n * 41) * obf(drawn[3]) % n2 and priv.decrypt(one) == 41
    packed = pub.encrypt_packed([1, -2, 3], 2, 8)
    assert packed.ciphertexts(False) == [(1 + n * m) * obf(r) % n2 for m, r in zip([(1 - (2 << 8)) % n, 3], drawn[4:6])]
    cs = [12345, n2 - 2]
    plain = EncryptedVector.from_ciphertexts(pub, cs)
    assert plain.obfuscate().ciphertexts(False) == [c * obf(r) % n2 for c, r in zip(cs, drawn[6:8])]
    number = paillier.EncryptedNumber(pub, 777)
    number.obfuscate()                                                           # EncryptedNumber.obfuscate
    assert number.ciphertext(False) == 777 * obf(drawn[8]) % n2 and len(drawn) == 9
    assert all(0 <= r < 1 << 40 for r in drawn)


def test_setting_is_not_part_of_the_key(emu_keys):
    pub, _ = emu_keys(256)
    other = paillier.PaillierPublicKey(pub.n)
    pub.enable_short_obfuscators(x=X_FIXED)
    assert pub == other and hash(pub) == hash(other)
    back = pickle.loads(pickle.dumps(pub))
    assert back == pub and back.short_obfuscator_base is None and back.short_obfuscator_bits is None


def test_errors(emu_keys):
    pub, _ = emu_keys(256)
    n = pub.n
    g = load_golden(256)
    values = [1, 2, 3]
    with pytest.raises(ValueError, match="enable_short_obfuscators"):
        pub.encrypt_batch(values, rho_values=[1, 2, 3])                          # short obfuscators are off
    with pytest.raises(ValueError):
        pub.encrypt_packed(values, 1, 8, rho_values=[1, 2, 3])
    with pytest.raises(ValueError):
        EncryptedVector.from_ciphertexts(pub, values).obfuscate(rho_values=[1, 2, 3])
    for bad in (0, -1, n.bit_length() + 1):
        with pytest.raises(ValueError):
            pub.enable_short_obfuscators(bits=bad)
    for bad in (8.0, "8", True, np.float64(8)):
        with pytest.raises(TypeError):
            pub.enable_short_obfuscators(bits=bad)
    with pytest.raises(ValueError):
        pub.enable_short_obfuscators(x=H(g["p"]))                                # shares a factor with n
    with pytest.raises(ValueError):
        pub.enable_short_obfuscators(x=3 * H(g["q"]) % n)
    _, hs = base_of(n)
    with pytest.raises(ValueError):
        pub.enable_short_obfuscators(x=X_FIXED, hs=hs)                           # exclusive
    for bad in (0, 1, n * n, n * n + 5, H(g["p"]), -3):
        with pytest.raises(ValueError):
            pub.enable_short_obfuscators(hs=bad)
    assert pub.short_obfuscator_base is None                                     # nothing above enabled anything
    assert pub.enable_short_obfuscators(bits=n.bit_length(), x=X_FIXED) == hs    # the bounds themselves are allowed
    assert pub.enable_short_obfuscators(bits=1, hs=hs) == hs and pub.short_obfuscator_bits == 1
    pub.enable_short_obfuscators(bits=40, x=X_FIXED)
    with pytest.raises(ValueError):
        pub.encrypt_batch(values, r_values=[1, 2, 3], rho_values=[1, 2, 3])      # not both
    with pytest.raises(ValueError):
        EncryptedVector.from_ciphertexts(pub, values).obfuscate(r_values=[1, 2, 3], rho_values=[1, 2, 3])
    with pytest.raises(ValueError):
        pub.encrypt_packed(values, 1, 8, r_values=[1, 2, 3], rho_values=[1, 2, 3])
    for bad in ([1, 2], [1, 2, 3, 4], np.zeros((2, 2), np.uint32), np.zeros((3, 1), np.uint32), np.zeros((3, 2), np.uint64)):
        with pytest.raises(ValueError):
            pub.encrypt_batch(values, rho_values=bad)                            # the length, the shape
    with pytest.raises(ValueError):
        pub.encrypt_packed(values, 2, 8, rho_values=[1, 2, 3])                   # one exponent per packed ROW: two rows here
    with pytest.raises(ValueError, match=r"rho_values\[1\]"):
        pub.encrypt_batch(values, rho_values=[0, 1 << 40, 5])                    # outside [0, 2^bits): the index is named
    with pytest.raises(ValueError, match=r"rho_values\[2\]"):
        pub.encrypt_batch(values, rho_values=[0, 1, -1])
    rows = np.zeros((3, 2), np.uint32)
    rows[2, 1] = 1 << 8                                                          # bit 40
    with pytest.raises(ValueError, match=r"rho_values\[2\]"):
        pub.encrypt_batch(values, rho_values=rows)
    rows[2, 1] = (1 << 8) - 1
    assert len(pub.encrypt_batch(values, rho_values=rows)) == 3                  # 2^40 - 2^32: the largest top word
    with pytest.raises(TypeError):
        pub.encrypt_batch(values, rho_values=[1, 2.0, 3])


# ---- a pool of obfuscators made ahead of time ---------------------------------------------------------------------------------
def resident_emulator_context():
    """the emulator context with the resident-row calls that the obfuscator pool goes through, on host memory (a device pointer
    is the address of a numpy block): what the engine composes without the comb kernel, call for call"""
    from emu_backend import EmuContext

    class ResidentEmuContext(EmuContext):
        def __init__(self, *a, **kw):
            EmuContext.__init__(self, *a, **kw)
            self._blocks = {}

        def malloc(self, nbytes):
            block = np.zeros((nbytes + 3) // 4, np.uint32)
            self._blocks[block.ctypes.data] = block
            return block.ctypes.data

        def free(self, ptr, nbytes):
            self._blocks.pop(ptr, None)

        @staticmethod
        def _rows(ptr, rows, cols):
            return np.ctypeslib.as_array((ctypes.c_uint32 * (rows * cols)).from_address(ptr)).reshape(rows, cols)

        def h2d(self, ptr, arr):
            self._rows(ptr, 1, arr.size)[0] = arr.reshape(-1)

        def d2h(self, arr, ptr):
            arr.reshape(-1)[:] = self._rows(ptr, 1, arr.size)[0]

        def d2d(self, dst, src, nbytes, stream=0):
            self._rows(dst, 1, nbytes // 4)[0] = self._rows(src, 1, nbytes // 4)[0]

        def sync(self, stream=0):
            pass

        def powmod_dev(self, base, e, exp_limbs, bits, out, batch, stream=0):
            self._rows(out, batch, self.ct_limbs)[:] = self.powmod(self._rows(base, batch, self.ct_limbs).copy(),
                                                                   self._rows(e, batch, exp_limbs).copy())

        def mulmod_dev(self, a, b, out, batch, stream=0):
            self._rows(out, batch, self.ct_limbs)[:] = self.mulmod(self._rows(a, batch, self.ct_limbs).copy(),
                                                                   self._rows(b, batch, self.ct_limbs).copy())

        def add_plain_dev(self, c, m, out, batch, stream=0):
            self._rows(out, batch, self.ct_limbs)[:] = self.add_plain(self._rows(c, batch, self.ct_limbs).copy(),
                                                                      self._rows(m, batch, self.n_limbs).copy())

        def encrypt_dev(self, m, r, out, batch, stream=0):
            self._rows(out, batch, self.ct_limbs)[:] = self.encrypt(self._rows(m, batch, self.n_limbs).copy(),
                                                                    self._rows(r, batch, self.n_limbs).copy())
    return ResidentEmuContext


def test_pool_of_short_obfuscators(monkeypatch):
    """precompute_obfuscators(k), then encrypt_batch: the pool holds pow(h_s, rho, n^2) for the drawn rho, each used once"""
    from phe import _native
    monkeypatch.setattr(_native, "Context", resident_emulator_context())
    g = load_golden(256)
    pub = paillier.PaillierPublicKey(H(g["n"]))
    priv = paillier.PaillierPrivateKey(pub, H(g["p"]), H(g["q"]))
    n, n2 = pub.n, pub.nsquare
    _, hs = base_of(n)
    drawn = []
    real = _engine.random_bits_limbs

    def recording(bits, count, limbs_, out=None):
        got = real(bits, count, limbs_, out)
        drawn.extend(ints(got))
        return got
    monkeypatch.setattr(_engine, "random_bits_limbs", recording)
    monkeypatch.setattr(keys, "SCALAR_POOL_REFILL", 4)
    eng = pub._get_engine()
    r_old = [5, 7]
    eng._obf.add(eng.upload_cipher([pow(r, n, n2) for r in r_old]))               # two rows made before: they stay valid
    pub.enable_short_obfuscators(bits=48, x=X_FIXED)
    assert pub.precompute_obfuscators(7) == 9 and len(drawn) == 7
    obf = Obfuscators(hs, n)
    pool = [pow(r, n, n2) for r in r_old] + [obf(r) for r in drawn]
    assert pub._get_engine().peek_obfuscators(9) == pool
    values = [3.0, -4.0, 5.5, 6.0, 7.0]
    vec = pub.encrypt_batch(np.array(values))                                   # (an array: the route that takes pool rows)
    assert vec.ciphertexts(False) == [(1 + n * m) * o % n2 for m, o in zip(encodings(pub, values), pool)]
    assert pub.obfuscators_available() == 4 and pub._get_engine().peek_obfuscators(4) == pool[5:]     # each row consumed once
    assert priv.decrypt_batch(vec) == values
    one = pub.encrypt(9)                                                         # the scalar call takes the next row
    assert one.ciphertext(False) == (1 + n * 9) * pool[5] % n2
    pub.discard_obfuscators()
    two = pub.encrypt(10)                                                        # dry: refilled with short obfuscators
    assert len(drawn) == 7 + 4 and two.ciphertext(False) == (1 + n * 10) * obf(drawn[7]) % n2


# ---- the exponent draw ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [1, 31, 32, 33, 127, 1024])
def test_random_bits_limbs(bits):
    words = (bits + 31) // 32
    a = _engine.random_bits_limbs(bits, 256, words)
    assert a.shape == (256, words) and a.dtype == np.uint32
    vals = ints(a)
    assert all(0 <= v < 1 << bits for v in vals)                                 # nothing at or above `bits`
    tops = [(v >> (bits - 1)) & 1 for v in vals]
    assert 0 in tops and 1 in tops                                               # (each fails with probability 2^-256)
    b = _engine.random_bits_limbs(bits, 256, words)
    assert not np.array_equal(a, b)
    wide = _engine.random_bits_limbs(bits, 256, words + 2)                       # rows wider than the exponent: the rest is zero
    assert all(0 <= v < 1 << bits for v in ints(wide))
    out = np.full((5, words), 0xFFFFFFFF, np.uint32)
    assert _engine.random_bits_limbs(bits, 5, words, out=out) is out and all(v < 1 << bits for v in ints(out))
    assert _engine.random_bits_limbs(bits, 0, words).shape == (0, words)
    with pytest.raises(ValueError):
        _engine.random_bits_limbs(32 * words + 1, 4, words)


# ---- the device body on the wave emulator -------------------------------------------------------------------------------------
EMU_DIR = os.path.join(ROOT, "tests", "emu")


def build_emu_lib(source, name):
    """tests/emu/<source> built beside libphe_emu.so (same flags as tests/emu/Makefile and the fixture of test_pack.py)"""
    src, lib = os.path.join(EMU_DIR, source), os.path.join(EMU_DIR, name)
    csrc = os.path.join(PKG, "csrc")
    deps = [src, os.path.join(EMU_DIR, "wave_emu.h")] + [os.path.join(csrc, h) for h in
                                                         ("mont_core.h", "split_core.h", "fixed_base.h", "key_setup.h")]
    if not os.path.exists(lib) or any(os.path.getmtime(d) > os.path.getmtime(lib) for d in deps):
        subprocess.check_call([os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra",
                               "-Wno-unused-parameter", "-Wno-unknown-pragmas", "-o", lib, src, "-lpthread"], cwd=EMU_DIR)
    return ctypes.CDLL(lib)


@pytest.fixture(scope="module")
def fb_lib():
    L = build_emu_lib("emu_fixed_base.cpp", "libphe_emu_fixed_base.so")
    L.emu_fixed_base_last_error.restype = ctypes.c_char_p
    return L


@pytest.fixture(scope="module")
def emu():
    from emu_lib import Emu
    return Emu()


def P(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None else None


PATTERN = 0xA5C3F00F


# rung 0 of each key and the wider rung that shares its rows' limb count (the 3072-bit key has none)
@pytest.mark.parametrize("bits, group, geometry", [(1024, 0, (2, 18)), (1024, 4, (4, 9)), (2048, 0, (4, 18)), (2048, 8, (8, 9)),
                                                   (3072, 0, (4, 27))])
def test_device_body_on_the_wave_emulator(fb_lib, emu, bits, group, geometry):
    g = load_golden(bits)
    n = H(g["n"])
    n2, s1 = n * n, (n.bit_length() + 31) // 32
    n_arr = limbs([n], s1)[0]
    gl = (ctypes.c_int * 3)()
    assert fb_lib.emu_fixed_base_pow(P(n_arr), s1, group, None, 0, 0, None, 0, None, 0, None, None, 0, ctypes.c_uint64(0), 1,
                                     gl) == 0
    G, L, words = gl
    assert (G, L) == geometry and words == emu.pair_words(n_arr)
    per_wave = 64 // G
    _, hs = base_of(n)
    rng = random.Random(bits + group)
    n_max = 2 * per_wave + 1

    def check(eb, w, row_counts, sample_table=False, every_mode=True, waves=2):
        T = -(-eb // w)
        per_pos = (1 << w) - 1
        entries = comb_table(hs, n, eb, w)
        assert len(entries) == T * per_pos
        table = emu.pair_op(n_arr, 0, limbs(entries, 2 * s1))
        if sample_table:
            # entries read back through from_pair: first, last, (T - 1, 1), three random — against pow, not the products above
            picks = [(0, 1), (T - 1, per_pos), (T - 1, 1)] + [(rng.randrange(T), rng.randrange(1, per_pos + 1)) for _ in range(3)]
            rows = np.ascontiguousarray(table[[t * per_pos + d - 1 for t, d in picks]])
            assert ints(emu.pair_op(n_arr, 1, rows)) == [pow(hs, d << (w * t), n2) for t, d in picks]
        el = (eb + 31) // 32
        rhos = edge_exponents(eb, w, count=min(n_max, 1 << eb))
        rhos = [rhos[i % len(rhos)] for i in range(n_max)]
        powers = {r: pow(hs, r, n2) for r in set(rhos)}
        e = limbs(rhos, el)
        ms = [0, 1, n - 1] + [rng.randrange(n) for _ in range(n_max - 3)]
        cs = [1, n2 - 1] + [rng.randrange(1, n2) for _ in range(n_max - 2)]
        m_arr, c_arr = limbs(ms, s1), limbs(cs, 2 * s1)
        c_pair = emu.pair_op(n_arr, 0, c_arr)

        def run(rows, mul, mul_is_pair, m, out_is_pair):
            out = np.full((rows + 1, words if out_is_pair else 2 * s1), PATTERN, np.uint32)    # one row more: it must stay
            rc = fb_lib.emu_fixed_base_pow(P(n_arr), s1, group, P(table), eb, w, P(np.ascontiguousarray(e[:rows])), el,
                                           P(np.ascontiguousarray(mul[:rows])) if mul is not None else None, mul_is_pair,
                                           P(np.ascontiguousarray(m[:rows])) if m is not None else None, P(out), out_is_pair,
                                           ctypes.c_uint64(rows), waves, None)
            assert rc == 0, fb_lib.emu_fixed_base_last_error()
            assert np.all(out[rows] == PATTERN)
            got = ints(emu.pair_op(n_arr, 1, out[:rows], group=group)) if out_is_pair else ints(out[:rows])
            want = [powers[r] * (cs[i] if mul is not None else 1) * (1 + n * ms[i] if m is not None else 1) % n2
                    for i, r in enumerate(rhos[:rows])]
            assert got == want, (eb, w, rows, mul is not None, mul_is_pair, m is not None, out_is_pair)

        for rows in row_counts:
            if not every_mode or rows < per_wave + 1:                           # (below a full wavefront: the two ends only)
                run(rows, None, 0, None, 1)
                run(rows, c_arr, 0, m_arr, 0)
                continue
            for out_is_pair in (0, 1):
                run(rows, None, 0, None, out_is_pair)                           # plain
                run(rows, c_pair, 1, None, out_is_pair)                         # from a pair row
                run(rows, c_arr, 0, None, out_is_pair)                          # from a canonical residue, converted as it is read
            run(rows, None, 0, m_arr, 0)                                        # the plaintext folded in on the way out
            run(rows, c_arr, 0, m_arr, 0)
            run(rows, c_pair, 1, m_arr, 0)
        return table, e, el

    all_rows = [1, per_wave - 1, per_wave, per_wave + 1, 2 * per_wave + 1]
    check(13, 4, all_rows, sample_table=True)             # a few windows; 13 is a multiple neither of the window nor of 32
    check(45, 7, [per_wave + 1])                          # windows that straddle a 32-bit word, a ragged top digit
    check(8, 8, [3])                                      # one position
    # the default length, once per key: every trip of a full-length exponent, in the two modes that share no code on the way in
    # and out, three rows on one wavefront (the emulator runs a wavefront's trips at some milliseconds each, whatever the rows)
    table, e, el = check(n.bit_length() // 2, 4, [3], sample_table=True, every_mode=False, waves=1)
    # what the entry point refuses
    out = np.zeros((1, words), np.uint32)
    eb = n.bit_length() // 2
    args = lambda **kw: [kw.get(k, v) for k, v in (("bits", eb), ("w", 4), ("e", P(e)), ("el", el), ("mul", None), ("mp", 0),
                                                   ("m", None), ("out", P(out)), ("op", 1))]
    call = lambda **kw: fb_lib.emu_fixed_base_pow(P(n_arr), s1, group, P(table), *args(**kw), ctypes.c_uint64(1), 1, None)
    assert call() == 0
    assert call(m=P(limbs([1], s1))) == 3                 # a plaintext with pair rows out
    assert call(el=el + 1) == 3 and call(el=el - 1) == 3  # exponent rows of another width
    assert call(w=0) == 3 and call(w=13) == 3 and call(bits=0) == 3
