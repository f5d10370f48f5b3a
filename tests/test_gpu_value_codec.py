"""The value codec of plain batches on the GPU (csrc/value_codec.h through phe_hip_values_encode_dev / phe_hip_values_decode_dev):
the two kernels against EncodedNumber.encode / decode in Python integers (tests/value_cases.py) — no encryption involved —,
then PaillierPublicKey.encrypt_batch bit for bit with the device encoding on and off, and
PaillierPrivateKey.decrypt_batch(as_array=True) against the list route.  Flagged rows are ordinary data here: a status byte,
never a fault."""
import random
import sys

import numpy as np
import pytest

from conftest import PKG, load_golden

if PKG not in sys.path:
    sys.path.insert(0, PKG)

import value_cases as vc  # noqa: E402
from phe import keys as keys_module  # noqa: E402
from phe import paillier  # noqa: E402
from phe._device import DeviceArray  # noqa: E402
from phe.ciphertext import EncryptedVector  # noqa: E402

pytestmark = pytest.mark.gpu

H = lambda s: int(s, 16)
_keys = {}


def keypair(bits):
    """one key pair (one GPU context) per width for the whole module"""
    if bits not in _keys:
        g = load_golden(bits)
        pub = paillier.PaillierPublicKey(H(g["n"]))
        _keys[bits] = (pub, paillier.PaillierPrivateKey(pub, H(g["p"]), H(g["q"])))
    return _keys[bits]


def kernel_encode(eng):
    """the encode entry on uploaded words, every output downloaded: (rows, exps or None, status)"""
    def encode(words, kind, exponent):
        count = len(words)
        bits = DeviceArray.from_host(eng.ctx, np.ascontiguousarray(words, dtype=np.uint64).view(np.uint32))
        rows, stat = DeviceArray(eng.ctx, count, eng.n_limbs), DeviceArray(eng.ctx, (count + 3) // 4, 1)
        e_dev = DeviceArray(eng.ctx, count, 1) if kind == vc.KIND_FLOAT else None
        eng.ctx.values_encode_dev(bits.ptr, count, kind, int(exponent or 0), rows.ptr, e_dev.ptr if e_dev else None, stat.ptr)
        eng.ctx.sync()
        status = np.empty(count, np.uint8)
        eng.ctx.d2h(status, stat.ptr)
        exps = None
        if e_dev is not None:
            exps = np.empty(count, np.int32)
            eng.ctx.d2h(exps, e_dev.ptr)
        return rows.to_host(), exps, status
    return encode


def test_the_backend_has_the_value_codec():
    pub, priv = keypair(1024)
    assert pub._get_engine().has_value_codec() and priv._get_engine().has_value_codec()


# ---- the kernels alone --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits, group", [(256, 16), (1024, 16), (2048, 16), (3072, 64), (8192, 64)])
def test_kernels_against_python_integers(bits, group):
    pub, _ = keypair(bits)
    eng = pub._get_engine()
    count = 301
    assert count % (256 // group) != 0                                 # not a multiple of the rows of a workgroup
    vc.check_encode(kernel_encode(eng), pub.n, seed=bits, count=count)
    decode = lambda m_rows, kind, exps: eng.values_decode_dev(DeviceArray.from_host(eng.ctx, m_rows), kind, exps)
    vc.check_decode(decode, pub.n, seed=bits + 1, count=count)


def test_engine_encode_and_refused_arguments():
    pub, _ = keypair(2048)
    eng = pub._get_engine()
    key = vc.Key(pub.n)
    rng = random.Random(7)
    # the engine's form: resident rows and the exponents; inf / nan raise, a mantissa of 2^62 under a precision gives None
    words = vc.float_words(rng, 67, non_finite=False)
    rows, exps = eng.values_encode_dev(np.array(words, dtype=np.uint64).view(np.float64))
    want = [vc.encode_ref(key, w, vc.KIND_FLOAT) for w in words]
    assert isinstance(rows, DeviceArray) and rows.shape == (67, eng.n_limbs) and exps.dtype == np.int64
    assert vc.to_ints(rows.to_host()) == [m for m, _, _ in want] and exps.tolist() == [e for _, e, _ in want]
    rows, exps = eng.values_encode_dev(np.array([3, -4], dtype=np.int64))
    assert vc.to_ints(rows.to_host()) == [3, pub.n - 4] and exps.tolist() == [0, 0]
    rows, e = eng.values_encode_dev(np.array([0.5, 1.5, -2.5]) / 65536.0, precision_exponent=-4)
    assert vc.to_ints(rows.to_host()) == [0, 2, pub.n - 2] and e == -4
    for bad in (float("inf"), float("nan")):
        with pytest.raises(ValueError, match="cannot encode inf / nan"):
            eng.values_encode_dev(np.array([1.0, bad, 2.0]))
        with pytest.raises(ValueError, match="cannot encode inf / nan"):
            eng.values_encode_dev(np.array([1.0, bad, 2.0 ** 80]), precision_exponent=0)
    assert eng.values_encode_dev(np.array([1.0, 2.0 ** 62]), precision_exponent=0) is None
    assert eng.values_encode_dev(np.zeros(0))[0].shape == (0, eng.n_limbs)
    with pytest.raises(TypeError):
        eng.values_encode_dev(np.zeros(3, np.float32))
    with pytest.raises(TypeError):
        eng.values_encode_dev(np.zeros(3, np.int64), precision_exponent=-2)
    # what the entry points refuse
    buf = DeviceArray(eng.ctx, 4, eng.n_limbs)
    small = DeviceArray(eng.ctx, 8, 1)
    with pytest.raises(ValueError, match="kind"):
        eng.ctx.values_encode_dev(small.ptr, 4, 4, 0, buf.ptr, small.ptr, small.ptr)
    with pytest.raises(ValueError, match="kind"):
        eng.ctx.values_decode_dev(buf.ptr, 4, 2, small.ptr, small.ptr, small.ptr)
    with pytest.raises(ValueError, match="exponent"):
        eng.ctx.values_encode_dev(small.ptr, 4, 3, 301, buf.ptr, None, small.ptr)
    with pytest.raises(ValueError, match="null"):
        eng.ctx.values_encode_dev(None, 4, 0, 0, buf.ptr, None, small.ptr)
    with pytest.raises(ValueError, match="null"):
        eng.ctx.values_encode_dev(small.ptr, 4, 2, 0, buf.ptr, None, small.ptr)       # the float kind writes exponents
    with pytest.raises(ValueError, match="null"):
        eng.ctx.values_decode_dev(buf.ptr, 4, 1, None, small.ptr, small.ptr)
    eng.ctx.values_encode_dev(None, 0, 0, 0, None, None, None)                          # nothing to do


# ---- end to end ---------------------------------------------------------------------------------------------------------------
def batches(pub, rng, count):
    """(values, precision) of the four kinds, the edge values of the shared cases among them"""
    ints = np.array(vc.int64_words(pub.n, rng, count), dtype=np.uint64).view(np.int64)
    uints = np.array(vc.uint64_words(pub.n, rng, count), dtype=np.uint64)
    floats = np.array(vc.float_words(rng, count, non_finite=False), dtype=np.uint64).view(np.float64)
    words = [w for w in vc.precision_words(1e-6, rng, count)[0] if abs(vc.b2f(w)) * 2.0 ** 20 < 2.0 ** 62]
    scaled = np.array(words, dtype=np.uint64).view(np.float64)
    return [(ints, None), (uints, None), (floats, None), (scaled, 1e-6)]


def reference_rows(pub, values, precision):
    enc = [paillier.EncodedNumber.encode(pub, v, precision=precision) for v in values.tolist()]
    return [e.encoding for e in enc], [e.exponent for e in enc]


@pytest.mark.parametrize("bits", [1024, 2048])
def test_encrypt_batch_bit_for_bit(bits, monkeypatch):
    pub, priv = keypair(bits)
    priv._get_engine()                                                 # (the key pair's engine serves the public key from here on)
    eng = pub._get_engine()
    pub.discard_obfuscators()
    rng = random.Random(bits)
    n, n2 = pub.n, pub.nsquare
    count = 131
    r_all = [rng.randrange(1, n) for _ in range(count)]
    rn_all = [pow(r, n, n2) for r in r_all]                            # (one set of obfuscators for the four kinds)
    for values, precision in batches(pub, rng, count):
        ms, es = reference_rows(pub, values, precision)
        rs = r_all[:len(ms)]
        want = [(1 + n * m) * rn % n2 for m, rn in zip(ms, rn_all)]
        for minimum in (0, 1 << 40):                                   # the device encoding, and the host encoding
            monkeypatch.setattr(keys_module, "VALUE_CODEC_DEVICE_MIN", minimum)
            for device in (False, True):
                vec = pub.encrypt_batch(values, precision=precision, r_values=rs, device=device)
                assert vec.on_device == device and list(vec.exponents) == es
                assert vec.ciphertexts(False) == want, (values.dtype, precision, minimum, device)
            # the pool route: obfuscators made ahead of time, each used once, in order (the host encoding under a precision
            # yields Python integers, which never took the pool)
            if precision is not None and minimum:
                continue
            pub.precompute_obfuscators(len(ms))
            rns = eng.peek_obfuscators(len(ms))
            pooled = pub.encrypt_batch(values, precision=precision, device=True)
            assert pub.obfuscators_available() == 0 and list(pooled.exponents) == es
            assert pooled.ciphertexts(False) == [(1 + n * m) * rn % n2 for m, rn in zip(ms, rns)]
    # a batch that cannot be encoded raises before any pool obfuscator is taken
    monkeypatch.setattr(keys_module, "VALUE_CODEC_DEVICE_MIN", 0)
    pub.precompute_obfuscators(8)
    with pytest.raises(ValueError, match="cannot encode inf / nan"):
        pub.encrypt_batch(np.array([1.0, float("nan"), 2.0]), device=True)
    assert pub.obfuscators_available() == 8
    # a mantissa of 2^62 under a precision: the host encodes that batch, same bits
    big = np.array([2.0 ** 62, 1.0, -2.0 ** 70])
    ms, es = reference_rows(pub, big, 1.0)
    vec = pub.encrypt_batch(big, precision=1.0, r_values=[3, 5, 7])
    assert list(vec.exponents) == es and vec.ciphertexts(False) == [(1 + n * m) * pow(r, n, n2) % n2 for m, r in zip(ms, (3, 5, 7))]
    pub.discard_obfuscators()


@pytest.mark.parametrize("bits", [1024, 2048])
def test_encrypt_batch_short_obfuscators(bits, monkeypatch):
    pub, priv = keypair(bits)
    priv._get_engine()
    rng = random.Random(bits + 1)
    n, n2 = pub.n, pub.nsquare
    pub.discard_obfuscators()
    hs = pub.enable_short_obfuscators(bits=128, x=rng.randrange(2, 1 << 64) | 1)
    try:
        rho_bits = pub.short_obfuscator_bits
        assert hs == pub.short_obfuscator_base
        for values, precision in batches(pub, rng, 131):
            ms, es = reference_rows(pub, values, precision)
            rhos = [rng.getrandbits(rho_bits) for _ in ms]
            want = [(1 + n * m) * pow(hs, rho, n2) % n2 for m, rho in zip(ms, rhos)]
            for minimum in (0, 1 << 40):
                monkeypatch.setattr(keys_module, "VALUE_CODEC_DEVICE_MIN", minimum)
                for device in (False, True):
                    vec = pub.encrypt_batch(values, precision=precision, rho_values=rhos, device=device)
                    assert vec.on_device == device and list(vec.exponents) == es
                    assert vec.ciphertexts(False) == want, (values.dtype, precision, minimum, device)
                # fresh short obfuscators: not reproducible, but every row decrypts to its plaintext
                fresh = pub.encrypt_batch(values, precision=precision, device=True)
                assert priv.raw_decrypt_batch(fresh.ciphertexts(False)) == ms
    finally:
        pub.disable_short_obfuscators()
        pub.discard_obfuscators()


@pytest.mark.parametrize("bits", [1024, 2048])
def test_decrypt_batch_as_array_equals_the_list_route(bits):
    pub, priv = keypair(bits)
    eng = priv._get_engine()
    assert eng.has_value_codec()
    rng = random.Random(bits + 2)
    n = pub.n
    ints, uints, floats, scaled = [v for v, _ in batches(pub, rng, 257)]
    small = uints[uints < np.uint64(1 << 63)]
    zeros = np.array([0.0, -0.0, 1.0, -1.0])                           # (-0.0 encodes as 0 and comes back as 0.0 on both routes)
    below = floats[np.abs(floats) < 2.0 ** 52]                         # (from 2^52 on a float's natural exponent is 0 or more)
    for values, precision, dtype in ((ints, None, np.int64), (small, None, np.int64), (below[np.abs(below) > 1e-250], None, np.float64),
                                     (scaled, 1e-6, np.float64), (zeros, 2.0 ** -8, np.float64)):
        vec = pub.encrypt_batch(values, precision=precision, device=True)
        want = priv.decrypt_batch(vec)
        for v in (vec, vec.to_host()):
            got = priv.decrypt_batch(v, as_array=True)
            assert isinstance(got, np.ndarray) and got.dtype == dtype and got.shape == (len(values),)
            assert got.view(np.uint64).tolist() == np.asarray(want, dtype=dtype).view(np.uint64).tolist()
    # floats whose exponents reach below -240 take the list route into the same array; mantissas beyond 64 bits are decoded on
    # the host row by row
    deep = pub.encrypt_batch(below, device=True)
    assert int(deep.exponent_array.min()) < -240
    got = priv.decrypt_batch(deep, as_array=True)
    assert got.view(np.uint64).tolist() == np.asarray(priv.decrypt_batch(deep), dtype=np.float64).view(np.uint64).tolist()
    wide = [5, n - 9, (1 << 64) + 3, n - (1 << 100) - 1, 1 << 900, n - (1 << 64), (1 << 64) - 1]
    vec = EncryptedVector.from_ciphertexts(pub, [pub.raw_encrypt(m, 11 + i) for i, m in enumerate(wide)], -3)
    got = priv.decrypt_batch(vec, as_array=True)
    assert got.dtype == np.float64 and got.tolist() == priv.decrypt_batch(vec)
    assert got.tolist() == [(m if m <= pub.max_int else m - n) / 4096.0 for m in wide]
    # the per-device list form
    vec = pub.encrypt_batch(ints, device=True)
    both = priv.decrypt_batch([vec[:100], vec[100:]], as_array=True)
    assert both.dtype == np.int64 and np.array_equal(both, ints)
    # the chunked generator: several chunks, resident and host rows
    for store in (vec.limbs(be_secure=False), vec.to_host().limbs(be_secure=False)):
        seen, parts = [], []
        for lo, hi, words, status, fetch in eng.raw_decrypt_decode_chunks(store, 0, chunk=100):
            assert words.dtype == np.uint64 and words.shape == (hi - lo,) and status.shape == (hi - lo,) and not status.any()
            seen.append((lo, hi))
            parts.append(words.view(np.int64))
            assert vc.to_ints(fetch([0, hi - lo - 1])) == [int(ints[lo]) % n, int(ints[hi - 1]) % n]
        assert seen == [(0, 100), (100, 200), (200, 257)] and np.array_equal(np.concatenate(parts), ints)


@pytest.mark.parametrize("bits", [1024, 2048])
def test_decrypt_batch_as_array_exceptions_in_row_order(bits):
    pub, priv = keypair(bits)
    n, max_int = pub.n, pub.max_int
    good = [5, n - 7, 0, 1 << 40]
    gap, wide = max_int + 1, 1 << 63
    enc = lambda ms, e: EncryptedVector.from_ciphertexts(pub, [pub.raw_encrypt(m, 23 + i) for i, m in enumerate(ms)], e)
    assert priv.decrypt_batch(enc(good, 0), as_array=True).tolist() == [5, -7, 0, 1 << 40]
    for host in (False, True):
        place = (lambda v: v) if host else (lambda v: v.to_device() if hasattr(v, "to_device") else v)
        with pytest.raises(OverflowError, match="int64"):
            priv.decrypt_batch(place(enc(good + [wide, gap] + good, 0)), as_array=True)
        with pytest.raises(OverflowError, match="Overflow detected"):
            priv.decrypt_batch(place(enc(good + [gap, wide] + good, 0)), as_array=True)
        with pytest.raises(OverflowError, match="Overflow detected"):
            priv.decrypt_batch(place(enc(good + [1 << 80, n - max_int - 1], -2)), as_array=True)
        got = priv.decrypt_batch(place(enc(good + [wide, n - wide - 1], -2)), as_array=True)      # fine as floats
        assert got.tolist() == [5 / 256.0, -7 / 256.0, 0.0, (1 << 40) / 256.0, wide / 256.0, -(wide + 1) / 256.0]
    for exps in ([0, -2, 0, 0], 1):
        with pytest.raises(ValueError, match="exponents"):
            priv.decrypt_batch(enc(good, exps), as_array=True)
    with pytest.raises(ValueError, match="Encoding"):
        class Base2(paillier.EncodedNumber):
            BASE = 2
            LOG2_BASE = 1.0
        priv.decrypt_batch(enc(good, 0), Encoding=Base2, as_array=True)
    assert priv.decrypt_batch(enc(good, 0), as_array=True).tolist() == [5, -7, 0, 1 << 40]       # the engine goes on working
