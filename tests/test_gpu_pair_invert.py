"""Inversion on rows in the pair form on the GPU (csrc/pair_invert.h through phe_hip_pair_invert_dev) and what rides on it:
-vec, a - b and vec.dot(w) with signed weights on pair-resident vectors (vec * k with negative scalars beside them).  Every expected value is
a Python integer — pow(c, -1, n^2) and the chain pow(inv or c, |k|, n^2) of phe/paillier.py:745-751 — never another route of the
code under test; the host vector's result is compared as well, not instead."""
import sys

import numpy as np
import pytest

from conftest import PKG, load_golden

if PKG not in sys.path:
    sys.path.insert(0, PKG)

from phe import _engine, _native, paillier  # noqa: E402
from phe._device import DeviceArray  # noqa: E402
from phe.ciphertext import EncryptedVector  # noqa: E402

pytestmark = pytest.mark.gpu

H = lambda s: int(s, 16)


def keypair(bits):
    g = load_golden(bits)
    pub = paillier.PaillierPublicKey(H(g["n"]))
    return pub, paillier.PaillierPrivateKey(pub, H(g["p"]), H(g["q"]))


def pair_geometry(ctx):
    code = ctx.last_launch()["geom_pub"]
    assert 2 * (code // 100) * (code % 100) == ctx.pair_words(), code                    # a rung that serves the pair rows
    return code // 100


def mixed(rs, n):
    """n numbers, floats and integers in turn-about blocks: the exponents differ"""
    x = [float(v) for v in rs.standard_normal(n)]
    for i in range(0, n, 3):
        x[i] = int(rs.integers(-99, 99))
    return x


@pytest.fixture(scope="module")
def residues():
    """per key width: 70 residues modulo n^2 (edge values among random units) and their inverses in Python integers, made once"""
    made = {}
    for bits in (1024, 2048, 3072):
        pub, _ = keypair(bits)
        rs = np.random.Generator(np.random.PCG64(bits))
        n2 = pub.nsquare
        values = [int.from_bytes(rs.bytes(bits // 4 + 8), "little") % (n2 - 2) + 2 for _ in range(70)]
        values[0:3] = [1, n2 - 1, pub.n + 1]
        made[bits] = (values, [pow(v, -1, n2) for v in values])
    return made


def pair_rows(eng, values):
    return eng.to_pair_dev(eng.upload_cipher(_native.ints_to_limbs(values, eng.ct_limbs)))


def residues_of(eng, pair):
    return eng.to_ints(eng.from_pair_dev(pair).to_host())


# ---- the raw inversion ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [1024, 2048])
def test_raw_inversion_at_every_depth(monkeypatch, residues, bits):
    """blocks of 4: 70 rows make the levels 70 -> 18 -> 5 -> 2 -> 1; lengths around the block, one row (no level at all)"""
    monkeypatch.setattr(_engine, "PAIR_INVERT_BLOCK_ROWS", 4)
    pub, _ = keypair(bits)
    eng = pub._get_engine()
    assert eng.has_pair_invert()
    values, want = residues[bits]
    for length in (1, 2, 3, 4, 5, 17, 70):
        store = pair_rows(eng, values[:length])
        out = eng.pair_invert_dev(store)
        assert out.rows == length and out.cols == eng.pair_form() and out.ptr != store.ptr
        assert residues_of(eng, out) == want[:length], length
        assert residues_of(eng, store) == values[:length]                                 # the input rows stay as they are


def test_raw_inversion_3072_default_block(residues):
    pub, _ = keypair(3072)
    eng = pub._get_engine()
    values, want = residues[3072]
    assert residues_of(eng, eng.pair_invert_dev(pair_rows(eng, values))) == want


def test_many_rows_and_the_small_batch_rung():
    """2^16 + 3 rows with the default block: X * out == 1 (mod n^2) and out < n^2 for EVERY row, which pins the inverse; a strided
    sample and both ends against pow(c, -1, n^2) itself.  The geometry of the rows' own level is not the one a 6-row call takes."""
    pub, _ = keypair(2048)
    eng = pub._get_engine()
    ctx = eng.ctx
    n2 = pub.nsquare
    rs = np.random.Generator(np.random.PCG64(16))
    count = (1 << 16) + 3
    words = rs.integers(0, 1 << 32, size=(count, eng.ct_limbs), dtype=np.uint64).astype(np.uint32)
    words[:, -1] = 0                                                                      # below n^2; units but for a chance of 2^-1000
    store = eng.to_pair_dev(eng.upload_cipher(words))
    out = eng.pair_invert_dev(store)
    g_big = pair_geometry(ctx)
    xs, got = eng.to_ints(words), residues_of(eng, out)
    assert all(o < n2 for o in got)
    assert all(x * o % n2 == 1 for x, o in zip(xs, got))
    for i in list(range(0, count, count // 255))[:256] + [0, count - 1]:
        assert got[i] == pow(xs[i], -1, n2), i
    small = eng.pair_invert_dev(store.rows_view(0, 6))
    g_small = pair_geometry(ctx)
    assert residues_of(eng, small) == got[:6]
    # (the pair rows of a 2048-bit key are served by 4 lanes per number, rung 0, and by 8: a single block takes the wide rung)
    assert g_small == 8 and g_big != g_small


def test_argument_errors_are_return_codes():
    pub, _ = keypair(1024)
    eng = pub._get_engine()
    ctx = eng.ctx
    store = pair_rows(eng, [3, 5, 7])
    out = DeviceArray(ctx, 3, eng.pair_form())
    with pytest.raises(ValueError):
        ctx.pair_invert_dev(store.ptr, out.ptr, 3, 1)                                     # a block of one row
    with pytest.raises(ValueError):
        ctx.pair_invert_dev(store.ptr, store.ptr, 3)                                      # in place
    with pytest.raises(ValueError):
        ctx.pair_invert_dev(None, out.ptr, 3)
    with pytest.raises(ValueError):
        ctx.pair_invert_dev(store.ptr, None, 3)
    ctx.pair_invert_dev(None, None, 0)                                                    # nothing to do
    ctx.pair_invert_dev(store.ptr, out.ptr, 3, 2)
    n2 = pub.nsquare
    assert residues_of(eng, out) == [pow(v, -1, n2) for v in (3, 5, 7)]
    ctx.release_scratch()                                                                 # the levels' buffer goes and comes back
    ctx.pair_invert_dev(store.ptr, out.ptr, 3)
    assert residues_of(eng, out) == [pow(v, -1, n2) for v in (3, 5, 7)]


# ---- the public operations --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def vectors():
    """per key width: two host vectors of 70 rows with mixed exponents, their clear values, made once"""
    made = {}
    for bits in (1024, 2048):
        pub, priv = keypair(bits)
        rs = np.random.Generator(np.random.PCG64(bits + 1))
        xa, xb = mixed(rs, 70), mixed(rs, 70)
        a, b = pub.encrypt_batch(xa), pub.encrypt_batch(xb)
        assert len(set(a.exponents)) > 1
        made[bits] = (pub, priv, a, b, xa, xb)
    return made


def scalar_variants(rs):
    """mixed-sign int64 with about 10 % and about 60 % negative (both branches of _inverted_where_pair), +-1 only, with zeros"""
    out = {}
    for name, share in (("few_negative", 0.1), ("most_negative", 0.6)):
        k = rs.integers(1, 1 << 40, 70)
        k[rs.random(70) < share] *= -1
        assert 0 < (k < 0).sum() and ((k < 0).sum() * 4 < 70) == (name == "few_negative")
        out[name] = k
    out["plus_minus_one"] = np.where(rs.random(70) < 0.5, -1, 1).astype(np.int64)
    zeros = rs.integers(-1000, 1000, 70)
    zeros[[0, 7, 69]] = 0
    out["with_zeros"] = zeros
    return out


def integer_mul(vec, k):
    """the chain of phe/paillier.py:745-751 in Python integers: pow(invert(c) if k < 0 else c, |k|, n^2)"""
    n2 = vec.public_key.nsquare
    return [pow(pow(c, -1, n2) if s < 0 else c, abs(int(s)), n2) for c, s in zip(vec.ciphertexts(False), k)]


def check_in_form(out, host_out, want):
    assert out._pair and out.on_device
    assert out.ciphertexts(False) == want
    assert host_out.ciphertexts(False) == want and not host_out.on_device
    assert out.exponents == host_out.exponents
    assert np.array_equal(out._obfuscated, host_out._obfuscated)


@pytest.mark.parametrize("bits", [1024, 2048])
def test_negation_and_subtraction_stay_in_the_form(vectors, bits):
    pub, priv, a, b, xa, xb = vectors[bits]
    eng = pub._get_engine()
    assert eng.has_pair_invert()
    n2 = pub.nsquare
    pa, pb = a.to_device().to_pair(), b.to_device().to_pair()
    assert pa._pair and pb._pair
    # -v
    neg = -pa
    check_in_form(neg, -a, [pow(c, -1, n2) for c in a.ciphertexts(False)])
    assert np.allclose(np.array(priv.decrypt_batch(neg), dtype=float), -np.array(xa, dtype=float), rtol=0, atol=1e-9)
    # a - b with mixed exponents: -b is made in the form; the alignment inside `+` (decrease_exponent_to, as before) then
    # works on residues, so the bits, the exponents and the values are checked here and the form below
    diff, host_diff = pa - pb, a - b
    assert diff.on_device and diff.exponents == host_diff.exponents
    base = paillier.EncodedNumber.BASE
    want = []
    for x, y, ea, eb in zip(a.ciphertexts(False), b.ciphertexts(False), a.exponents, b.exponents):
        t = min(ea, eb)                                                                   # (phe/paillier.py:570-601: c^(BASE^delta))
        want.append(pow(x, base ** (ea - t), n2) * pow(pow(y, -1, n2), base ** (eb - t), n2) % n2)
    assert diff.ciphertexts(False) == host_diff.ciphertexts(False) == want
    assert np.allclose(np.array(priv.decrypt_batch(diff), dtype=float), np.array(xa, dtype=float) - np.array(xb, dtype=float),
                       rtol=0, atol=1e-9)
    # a - b at one exponent: one inversion and one pair product, still in the form; (a - b) + b decrypts to a
    rs = np.random.Generator(np.random.PCG64(bits + 5))
    xi, xj = [int(v) for v in rs.integers(-999, 999, 70)], [int(v) for v in rs.integers(-999, 999, 70)]
    hi, hj = pub.encrypt_batch(xi), pub.encrypt_batch(xj)
    pi, pj = hi.to_device().to_pair(), hj.to_device().to_pair()
    diff = pi - pj
    assert diff._pair and diff.on_device and pi._pair and pj._pair
    assert diff.ciphertexts(False) == (hi - hj).ciphertexts(False) == [x * pow(y, -1, n2) % n2 for x, y in zip(
        hi.ciphertexts(False), hj.ciphertexts(False))]
    assert priv.decrypt_batch(diff) == [x - y for x, y in zip(xi, xj)]
    back = diff + pj
    assert back._pair and priv.decrypt_batch(back) == xi
    # v * k with negative scalars keeps the route it had (tests/test_gpu_ladder.py::test_encrypted_vector_in_pair_form pins that
    # such a product comes back as residues): the bits, the exponents and the values beside those of -v and a - b above
    rs = np.random.Generator(np.random.PCG64(bits + 2))
    for name, k in scalar_variants(rs).items():
        out, host_out = a.to_device().to_pair() * k, a * k
        assert out.on_device and out.ciphertexts(False) == host_out.ciphertexts(False) == integer_mul(a, k), name
        assert out.exponents == host_out.exponents and np.array_equal(out._obfuscated, host_out._obfuscated)
        assert np.allclose(np.array(priv.decrypt_batch(out), dtype=float), np.array(xa, dtype=float) * k, rtol=1e-12, atol=1e-6), name
    w = rs.standard_normal(70)
    out, host_out = a.to_device().to_pair() * w, a * w
    assert out.exponents == host_out.exponents and len(set(out.exponents)) > 1
    assert out.ciphertexts(False) == host_out.ciphertexts(False)
    assert np.allclose(np.array(priv.decrypt_batch(out), dtype=float), np.array(xa, dtype=float) * w, rtol=1e-9, atol=1e-9)
    # -v of a vector with mixed exponents keeps them (phe/paillier.py: the scalar -1 has exponent 0)
    assert (-pa).exponents == a.exponents and pa._pair


@pytest.mark.parametrize("bits", [1024, 2048])
def test_dot_with_signed_weights_reads_the_rows_in_the_form(monkeypatch, vectors, bits):
    """with PAIR_INVERT_MIN_ROWS out of the way the 70 rows are inverted in the form; with the shipped threshold they are too
    few and the present route gives the same bits"""
    pub, priv, a, _, xa, _ = vectors[bits]
    shipped = a.to_device().to_pair().dot(np.where(np.arange(70) % 3 == 0, -2, 5))
    assert _engine.PAIR_INVERT_MIN_ROWS > 70
    assert shipped.ciphertext(False) == a.dot(np.where(np.arange(70) % 3 == 0, -2, 5)).ciphertext(False)
    monkeypatch.setattr(_engine, "PAIR_INVERT_MIN_ROWS", 0)
    eng = pub._get_engine()
    n2 = pub.nsquare
    pa = a.to_device().to_pair()
    rs = np.random.Generator(np.random.PCG64(bits + 3))
    calls = []
    keep = eng._inverted_where_pair
    eng._inverted_where_pair = lambda store, neg: calls.append(int(np.sum(neg))) or keep(store, neg)
    try:
        for name, k in scalar_variants(rs).items():
            calls.clear()
            got, host = pa.dot(k), a.dot(k)
            assert calls == [int((k < 0).sum())], name                                    # the rows were inverted in the form
            assert pa._pair                                                               # ... and stayed in it
            # the chain of `*` and `+` in Python integers: every term aligned to the smallest exponent, then multiplied up
            terms = a * k
            aligned = terms.decrease_exponent_to(int(terms.exponent_array.min())).ciphertexts(False)
            want = 1
            for c in aligned:
                want = want * c % n2
            assert got.ciphertext(False) == want == host.ciphertext(False), name
            assert got.exponent == host.exponent
            assert abs(priv.decrypt(got) - float(np.dot(np.array(xa, dtype=float), k))) <= 1e-6 * max(1.0, float(np.abs(k).max()))
        w = rs.standard_normal(70)
        got, host = pa.dot(w), a.dot(w)
        assert got.ciphertext(False) == host.ciphertext(False) and got.exponent == host.exponent
        assert abs(priv.decrypt(got) - float(np.dot(np.array(xa, dtype=float), w))) < 1e-9
    finally:
        del eng._inverted_where_pair


# ---- errors and the fallback ------------------------------------------------------------------------------------------------------
def test_a_row_without_inverse_is_named():
    pub, _ = keypair(1024)
    eng = pub._get_engine()
    rs = np.random.Generator(np.random.PCG64(4))
    host = pub.encrypt_batch([int(v) for v in rs.integers(-50, 50, 40)])
    words = host._limbs.copy()
    words[5] = _native.ints_to_limbs([pub.n], eng.ct_limbs)[0]                            # the "ciphertext" n: no inverse modulo n^2
    vec = EncryptedVector(pub, eng.upload_cipher(words), host.exponent_array.copy()).to_pair()
    assert vec._pair
    with pytest.raises(ZeroDivisionError) as info:
        -vec
    assert info.value.bad_index == 5
    k = np.ones(40, dtype=np.int64)
    k[[5, 9]] = -3                                                                        # two rows gathered: the bad one is row 0 of them
    with pytest.raises(ZeroDivisionError) as info:
        vec * k
    assert info.value.bad_index == 5
    k[5] = 3
    assert len(vec * k) == 40                                                             # row 9 alone has an inverse


def test_without_the_pair_form_the_present_route_serves(monkeypatch, vectors):
    """PHE_HIP_PAIR_FORM=0: no inversion in the form — the same expressions, the same bits"""
    pub0, _, a, b, _, _ = vectors[1024]
    rs = np.random.Generator(np.random.PCG64(6))
    k = scalar_variants(rs)["most_negative"]
    pa, pb = a.to_device().to_pair(), b.to_device().to_pair()
    monkeypatch.setattr(_engine, "PAIR_INVERT_MIN_ROWS", 0)                               # (dot inverts in the form at any length)
    want = [(-pa).ciphertexts(False), (pa - pb).ciphertexts(False), (pa * k).ciphertexts(False), pa.dot(k).ciphertext(False)]
    assert want[2] == integer_mul(a, k)
    monkeypatch.setenv("PHE_HIP_PAIR_FORM", "0")
    pub = paillier.PaillierPublicKey(pub0.n)
    eng = pub._get_engine()
    assert not eng.pair_form() and not eng.has_pair_invert()
    da = EncryptedVector(pub, eng.upload_cipher(a._limbs), a.exponent_array.copy()).to_pair()
    db = EncryptedVector(pub, eng.upload_cipher(b._limbs), b.exponent_array.copy()).to_pair()
    assert not da._pair
    got = [(-da).ciphertexts(False), (da - db).ciphertexts(False), (da * k).ciphertexts(False), da.dot(k).ciphertext(False)]
    assert got == want
