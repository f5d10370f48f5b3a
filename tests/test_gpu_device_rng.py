"""The device draw of the short obfuscator exponents on the GPU (csrc/chacha_rows.h through phe_hip_chacha20_rows_dev, and
enable_short_obfuscators(device_rng=True) above it).  The keystream kernel is compared word for word with the numpy expander
phe/_chacha.py (itself held to RFC 8439 and to a scalar implementation by tests/test_device_rng.py); every ciphertext of the
public routes must be the Python-integer formula (1 + n*m) * pow(h_s, rho, n^2) mod n^2 for the rho that the recorded seed of
its chunk expands to."""
import sys

import numpy as np
import pytest

from conftest import PKG, load_golden

if PKG not in sys.path:
    sys.path.insert(0, PKG)

from phe import _chacha, _engine, paillier  # noqa: E402
from phe._device import DeviceArray  # noqa: E402
from phe.ciphertext import EncryptedVector  # noqa: E402

from short_cases import X_FIXED, base_of, ints  # noqa: E402

pytestmark = pytest.mark.gpu

H = lambda s: int(s, 16)
PATTERN = 0xA5C3F00F

RFC_KEY = bytes(range(32))
RFC_NONCE = (0x09000000, 0x4A000000, 0x00000000)
RFC_BLOCK = [int(w, 16) for w in ("e4e7f110 15593bd1 1fdd0f50 c47120a3 c7f4d1c7 0368c033 9aaa2204 4e6cd4c3 "
                                  "466482d2 09aa9f07 05d7c214 a2028bd9 d19c12b5 b94e16de e883d0cb 4e3c50a2").split()]
LAYOUTS = [(1, 1), (31, 1), (64, 2), (500, 16), (512, 16), (513, 17), (1000, 32), (1024, 32), (1536, 48), (1024, 34)]
ROWS = [1, 63, 64, 65, 1000]


def keypair(bits):
    g = load_golden(bits)
    pub = paillier.PaillierPublicKey(H(g["n"]))
    priv = paillier.PaillierPrivateKey(pub, H(g["p"]), H(g["q"]))
    priv._get_engine()                               # the key pair's engine from the start: the public key works through it
    return pub, priv


@pytest.fixture(scope="module")
def ctx():
    pub, _ = keypair(256)
    return pub._get_engine().ctx


def device_rows(ctx, key, nonce, counter0, bits, limbs, rows):
    """phe_hip_chacha20_rows_dev into a buffer with a guard row behind the output, which must stay as it was"""
    guarded = np.full((rows + 1, limbs), PATTERN, np.uint32)
    out = DeviceArray.from_host(ctx, guarded)
    ctx.chacha20_rows_dev(key, nonce, counter0, bits, limbs, out.ptr, rows)
    ctx.sync()
    got = out.to_host()
    assert np.all(got[rows] == PATTERN)
    return got[:rows]


def test_known_answer_rfc8439(ctx):
    assert device_rows(ctx, RFC_KEY, RFC_NONCE, 1, 512, 16, 1)[0].tolist() == RFC_BLOCK
    words = [int.from_bytes(RFC_KEY[4 * i:4 * i + 4], "little") for i in range(8)]
    assert device_rows(ctx, words, list(RFC_NONCE), 1, 512, 16, 1)[0].tolist() == RFC_BLOCK      # the key as words


@pytest.mark.parametrize("bits, limbs", LAYOUTS)
def test_layout_against_the_host_expander(ctx, bits, limbs):
    key = bytes((11 * i + bits) & 0xFF for i in range(32))
    nonce = (limbs, 0x0A0B0C0D, bits)
    for rows in ROWS:
        got = device_rows(ctx, key, nonce, 9, bits, limbs, rows)
        assert np.array_equal(got, _chacha.chacha20_rows(key, nonce, 9, bits, limbs, rows))
    # the counter may reach its end; at one width more blocks than the largest grid has lanes (the grid-stride walk: 8 workgroups
    # of 256 lanes per compute unit, 2^19 lanes on 256 units)
    B = -(-limbs // 16)
    rows = (1 << 19) + 77 if (bits, limbs) == (512, 16) else 65
    last = (1 << 32) - rows * B
    got = device_rows(ctx, key, nonce, last, bits, limbs, rows)
    assert np.array_equal(got, _chacha.chacha20_rows(key, nonce, last, bits, limbs, rows))


def test_arguments_refused_before_any_launch(ctx):
    out = DeviceArray.from_host(ctx, np.full((4, 32), PATTERN, np.uint32))
    bad = [dict(key=None), dict(nonce=None), dict(out=None), dict(bits=0), dict(bits=1025), dict(bits=-5),
           dict(counter0=(1 << 32) - 2 * 3 + 1), dict(limbs=0)]
    for change in bad:
        a = dict(key=RFC_KEY, nonce=RFC_NONCE, counter0=0, bits=1024, limbs=32, out=out.ptr, rows=3)
        a.update(change)
        with pytest.raises(ValueError) as err:
            ctx.chacha20_rows_dev(a["key"], a["nonce"], a["counter0"], a["bits"], a["limbs"], a["out"], a["rows"])
        assert RFC_KEY.hex() not in str(err.value) and "03020100" not in str(err.value)
    ctx.chacha20_rows_dev(RFC_KEY, RFC_NONCE, 0, 1024, 32, out.ptr, 0)                          # no rows: fine, nothing launched
    ctx.sync()
    assert np.all(out.to_host() == PATTERN)                                                    # nothing was written by any of them
    ctx.chacha20_rows_dev(RFC_KEY, RFC_NONCE, (1 << 32) - 2 * 3, 1024, 32, out.ptr, 3)          # the last counter itself is allowed
    ctx.sync()
    got = out.to_host()
    assert np.array_equal(got[:3], _chacha.chacha20_rows(RFC_KEY, RFC_NONCE, (1 << 32) - 6, 1024, 32, 3)) and np.all(got[3] == PATTERN)


# ---- the public routes under recorded seeds ------------------------------------------------------------------------------------
class Recorded:
    def __init__(self, monkeypatch):
        self.handed, self.copies = [], []
        real = _engine.fresh_seed

        def fresh_seed():
            seed = real()
            self.handed.append(seed)
            self.copies.append(bytes(seed))
            return seed

        def no_host_draw(*a, **kw):
            raise AssertionError("a batch route drew through random_bits_limbs")
        monkeypatch.setattr(_engine, "fresh_seed", fresh_seed)
        monkeypatch.setattr(_engine, "random_bits_limbs", no_host_draw)

    def rhos(self, k, bits, count):
        return ints(_chacha.chacha20_rows(self.copies[k], (0, 0, 0), 0, bits, (bits + 31) // 32, count))

    def check_wiped(self):
        assert all(not any(seed) for seed in self.handed)
        assert len(set(self.copies)) == len(self.copies) and all(any(c) for c in self.copies)


class Powers:
    """pow(h_s, rho, n^2) for many rho of up to 128 bits, with Python integers: eight table entries multiplied per exponent (the
    tables of h_s^(d * 2^(16 t)) are made once) instead of 128 squarings each — CPython's pow takes about 0.1 ms at this size, and one test
    wants 98309 of them.  The first rows of every call are held to pow itself."""

    def __init__(self, hs, n2):
        self.hs, self.n2, self.tables = hs, n2, []
        for t in range(8):
            step, row = pow(hs, 1 << (16 * t), n2), [1] * 65536
            for d in range(1, 65536):
                row[d] = row[d - 1] * step % n2
            self.tables.append(row)

    def __call__(self, rhos):
        n2, T = self.n2, self.tables
        out = []
        for r in rhos:
            assert 0 <= r < 1 << 128
            v = T[0][r & 65535]
            for t in range(1, 8):
                v = v * T[t][(r >> (16 * t)) & 65535] % n2
            out.append(v)
        assert out[:20] == [pow(self.hs, r, n2) for r in rhos[:20]]
        return out


@pytest.fixture(scope="module")
def small():
    pub, priv = keypair(256)
    _, hs = base_of(pub.n)
    assert pub.enable_short_obfuscators(x=X_FIXED, device_rng=True) == hs
    assert pub.short_obfuscator_device_rng and pub._get_engine().has_fixed_base()
    assert hasattr(pub._get_engine().ctx, "chacha20_rows_dev")
    return pub, priv, Powers(hs, pub.nsquare)


def test_encrypt_batch_over_three_chunks(small, monkeypatch):
    pub, priv, powers = small
    n, n2, bits = pub.n, pub.nsquare, pub.short_obfuscator_bits
    pub.discard_obfuscators()
    rec = Recorded(monkeypatch)
    sizes = [32768, 65536, 5]
    count = sum(sizes)
    values = np.random.Generator(np.random.PCG64(13)).integers(-10 ** 12, 10 ** 12, count)
    vec = pub.encrypt_batch(values, device=True)
    assert vec.on_device and len(rec.handed) == 3                       # one seed per chunk
    rho = [r for k, size in enumerate(sizes) for r in rec.rhos(k, bits, size)]
    assert len(set(rho)) == count and max(rho) < 1 << bits
    got = vec.ciphertexts(False)
    assert got == [(1 + n * (int(v) % n)) * o % n2 for v, o in zip(values, powers(rho))]
    assert priv.decrypt_batch(vec) == values.tolist()
    rec.check_wiped()
    host = pub.encrypt_batch(values[:1100])                             # host result: the same route, downloaded
    assert not host.on_device and len(rec.handed) == 4
    assert host.ciphertexts(False) == [(1 + n * (int(v) % n)) * o % n2 for v, o in zip(values, powers(rec.rhos(3, bits, 1100)))]
    rec.check_wiped()


def test_pool_and_whole_vector_obfuscate(small, monkeypatch):
    pub, priv, powers = small
    n, n2, bits = pub.n, pub.nsquare, pub.short_obfuscator_bits
    pub.discard_obfuscators()
    rec = Recorded(monkeypatch)
    assert pub.precompute_obfuscators(1000) == 1000 and len(rec.handed) == 1
    power = powers(rec.rhos(0, bits, 1000))
    values = np.random.Generator(np.random.PCG64(14)).integers(-10 ** 12, 10 ** 12, 1000)
    vec = pub.encrypt_batch(values, device=True)
    assert len(rec.handed) == 1 and pub.obfuscators_available() == 0
    assert vec.ciphertexts(False) == [(1 + n * (int(v) % n)) * o % n2 for v, o in zip(values, power)]
    assert priv.decrypt_batch(vec) == values.tolist()
    # whole-vector obfuscate of resident rows, canonical and in the pair form (too many rows for the small-vector pool refill)
    rs = np.random.Generator(np.random.PCG64(15))
    cs = [int.from_bytes(rs.bytes(n2.bit_length() // 8 - 1), "little") | 1 for _ in range(1500)]
    cs[0] = n2 - 1
    for k, make in ((1, lambda v: v.to_device()), (2, lambda v: v.to_pair())):
        vec = make(EncryptedVector.from_ciphertexts(pub, cs))
        assert vec.obfuscate() is vec and vec.on_device and len(rec.handed) == k + 1
        assert vec.ciphertexts(False) == [c * o % n2 for c, o in zip(cs, powers(rec.rhos(k, bits, 1500)))]
    rec.check_wiped()


def test_no_stuck_counter_or_seed():
    """a smoke check, not a statistical test: no two rows of one draw are equal, and no two draws are equal"""
    pub, _ = keypair(1024)
    eng = pub._get_engine()
    a = eng.random_bits_dev(512, 4096, 16)
    b = eng.random_bits_dev(512, 4096, 16)
    eng.ctx.sync()
    a, b = a.to_host(), b.to_host()
    assert a.shape == b.shape == (4096, 16)
    assert len({r.tobytes() for r in a}) == 4096 and len({r.tobytes() for r in b}) == 4096
    assert not {r.tobytes() for r in a} & {r.tobytes() for r in b}
    assert a.any(axis=0).all() and b.any(axis=0).all()                   # every word column is filled
