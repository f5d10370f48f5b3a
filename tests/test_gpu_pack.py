"""EncryptedVector.pack / PaillierPrivateKey.decrypt_packed on the GPU (csrc/segment_core.h segment_pack_body through
phe_hip_segment_pack_dev): every output row must be the Python-integer product prod_j c[b*S + j] ^ (2^(B*j)) mod n^2 over the
aligned rows — the reference's chain c_0*1 + c_1*(1 << B) + ... (EncryptedNumber.__mul__ -> _raw_mul, phe/paillier.py:721-751;
__add__ -> _raw_add, :705-719) — whatever form the input is in and whichever route computes it, and the plaintexts that come
back must be the values that went in."""
import sys

import numpy as np
import pytest

from conftest import PKG, load_golden

if PKG not in sys.path:
    sys.path.insert(0, PKG)

from phe import _engine, paillier  # noqa: E402
from phe.ciphertext import EncryptedVector  # noqa: E402

pytestmark = pytest.mark.gpu

H = lambda s: int(s, 16)


def keypair(bits):
    g = load_golden(bits)
    pub = paillier.PaillierPublicKey(H(g["n"]))
    return pub, paillier.PaillierPrivateKey(pub, H(g["p"]), H(g["q"]))


def integer_pack(cs, S, B, n2, horner=None):
    """row b: prod_j cs[b*S + j] ^ (2^(B*j)) mod n^2 in Python integers.  Up to two output rows by the formula as it stands;
    longer lists by Horner's rule on integers (B squarings per row instead of B*j: the formula itself takes Python seconds at
    2000 rows of a 2048-bit key), which test_every_row_against_the_integer_formula checks against the formula on short lists."""
    horner = len(cs) > 2 * S if horner is None else horner
    want = []
    for b in range(0, len(cs), S):
        v = 1
        if horner:
            for c in reversed(cs[b:b + S]):
                v = pow(v, 1 << B, n2) * c % n2
        else:
            for j, c in enumerate(cs[b:b + S]):
                v = v * pow(c, 1 << (B * j), n2) % n2
        want.append(v)
    return want


def pair_geometry(ctx):
    code = ctx.last_launch()["geom_pub"]
    assert 2 * (code // 100) * (code % 100) == ctx.pair_words(), code                    # a rung that serves the pair rows
    return code // 100


def mixed(rs, n):
    """n numbers, floats and integers in turn-about blocks: the exponents differ; negative values among them"""
    x = [float(v) for v in rs.standard_normal(n)]
    for i in range(0, n, 3):
        x[i] = int(rs.integers(-99, 99))
    return x


def widest(pub, B):
    return (pub.max_int.bit_length() - 1) // B


@pytest.fixture(scope="module")
def pools():
    """per key width: the longest vector any shape below needs (resident, integers: one exponent) and its ciphertexts, made once"""
    made = {}
    for bits in (1024, 2048):
        pub, _ = keypair(bits)
        S = widest(pub, 64)
        assert S == {1024: 15, 2048: 31}[bits]
        rs = np.random.Generator(np.random.PCG64(bits))
        dev = pub.encrypt_batch([int(v) for v in rs.integers(-1000, 1000, 67 * S + S - 1)], device=True)
        made[bits] = (dev, dev.ciphertexts(False))
    return made


@pytest.mark.parametrize("bits", [1024, 2048])
@pytest.mark.parametrize("shape", [(1, 7), (2, 1), (5, 29), (4, 33), ("widest", 64)])
def test_every_row_against_the_integer_formula(pools, bits, shape):
    dev, cs = pools[bits]
    pub = dev.public_key
    n2 = pub.nsquare
    S, B = shape
    S = widest(pub, B) if S == "widest" else S
    assert pub._get_engine().has_segment_pack()
    # the longest list once, by Horner's rule on integers; a shorter one shares its full tasks and has its own ragged one.  The
    # formula as it stands anchors both on the list of 2 S - 1 rows
    longest = integer_pack(cs[:67 * S + max(1, S - 1)], S, B, n2, horner=True)

    def want_for(length):
        full, rest = divmod(length, S)
        return longest[:full] + (integer_pack(cs[full * S:length], S, B, n2, horner=True) if rest else [])

    assert want_for(2 * S - 1) == integer_pack(cs[:2 * S - 1], S, B, n2, horner=False)
    for length in sorted({S * k + r for k in (1, 67) for r in (0, 1, S - 1)}):
        want = want_for(length)
        vec = dev[:length]
        out = vec.pack(S, B)
        assert out.on_device and not out._pair and len(out) == -(-length // S) == len(want)
        assert out.exponents == [0] * len(want) and (S == 1 or not out._obfuscated.any())        # (S = 1: the rows themselves)
        assert out.ciphertexts(False) == want, (S, B, length)
        pair = vec.to_pair()
        out = pair.pack(S, B)                                                             # the loop over pair rows
        assert out._pair and pair._pair
        assert out.ciphertexts(False) == want, (S, B, length)


@pytest.mark.parametrize("bits", [1024, 2048])
def test_every_input_form_gives_the_same_bits(bits):
    pub, priv = keypair(bits)
    n2 = pub.nsquare
    rs = np.random.Generator(np.random.PCG64(bits + 1))
    S, B = 5, 29
    x = [int(v) for v in rs.integers(-1000, 1000, 3 * S + 2)]
    y = [int(v) for v in rs.integers(-1000, 1000, 3 * S + 2)]
    host = pub.encrypt_batch(x)
    want = integer_pack(host.ciphertexts(False), S, B, n2)
    dev = host.to_device()
    pair = dev.to_pair()
    a, b, p = host.pack(S, B), dev.pack(S, B), pair.pack(S, B)
    assert not a.on_device and b.on_device and not b._pair and p.on_device and p._pair
    assert pair._pair                                                                     # the input is left in the form
    assert a.ciphertexts(False) == b.ciphertexts(False) == p.ciphertexts(False) == want
    assert priv.decrypt_packed(p, S, B, count=len(x)) == x
    # Montgomery debt: the lazy sum of two resident vectors is read through _plain_rows() and keeps its debt
    other = pub.encrypt_batch(y, device=True)
    lazy = dev + other
    assert lazy._debt == 1
    out = lazy.pack(S, B)
    assert lazy._debt == 1 and out.on_device and not out._pair and out._debt == 0
    sums = [c * d % n2 for c, d in zip(host.ciphertexts(False), other.ciphertexts(False))]
    assert out.ciphertexts(False) == integer_pack(sums, S, B, n2)
    assert priv.decrypt_packed(out, S, B, count=len(x)) == [u + v for u, v in zip(x, y)]
    assert lazy.pack(1, 7).ciphertexts(False) == sums                                     # S = 1: the aligned rows
    assert len(dev[:0].pack(S, B)) == 0 and dev[:0].pack(S, B).on_device
    with pytest.raises(ValueError):
        dev.pack(widest(pub, 64) + 1, 64)


def test_many_light_tasks_and_the_small_batch_rung():
    pub, _ = keypair(2048)
    eng = pub._get_engine()
    ctx = eng.ctx
    n2 = pub.nsquare
    rs = np.random.Generator(np.random.PCG64(12))
    S, B = 2, 3
    n_out = (1 << 16) + 1
    n_rows = 2 * n_out - 1                                                                # the last task is ragged
    words = rs.integers(0, 1 << 32, size=(n_rows, eng.ct_limbs), dtype=np.uint64).astype(np.uint32)
    words[:, -1] = 0                                                                      # any residues below n^2 serve
    full = EncryptedVector(pub, eng.upload_cipher(words), np.zeros(n_rows, dtype=np.int64)).to_pair()
    out = full.pack(S, B)
    geometry = {"2^16 + 1 tasks": pair_geometry(ctx)}
    assert out._pair and len(out) == n_out
    cs = eng.to_ints(words)
    got = eng.to_ints(out._plain_rows().to_host())
    assert got[:-1] == [cs[i] * pow(cs[i + 1], 8, n2) % n2 for i in range(0, n_rows - 1, 2)]
    assert got[-1] == cs[-1]
    small = full[:3].to_pair()
    out3 = small.pack(S, B)
    geometry["2 tasks"] = pair_geometry(ctx)
    assert out3.ciphertexts(False) == [cs[0] * pow(cs[1], 8, n2) % n2, cs[2]]
    # The pair rows of a 2048-bit key are served by 4 lanes per number (rung 0) and by 8 (the only wider rung with their limb
    # count).  2^16 + 1 tasks are two full rounds of four-lane groups on 256 CUs: rung 0; two tasks fill nothing: the wider rung.
    assert len(set(geometry.values())) >= 2, geometry


def test_the_histogram_flow():
    """segment_sum(ids, 64).cumsum(block=64).pack(S, B), then decrypt_packed: F histograms, their left-child sums, packed"""
    pub, priv = keypair(2048)
    rs = np.random.Generator(np.random.PCG64(13))
    n, F, bins = 4000, 3, 64
    # gradients on a grid of 2^-20 in [-1, 1]: a float's own exponent is at least -18 (base 16), so aligned mantissas stay below
    # 2^72, any sum of 4000 of them below 2^84 — slots of 96 bits; and every sum is exact in float64
    x = rs.integers(-(1 << 20), (1 << 20) + 1, n) / float(1 << 20)
    ids = rs.integers(-1, bins, size=(F, n))
    B = 96
    S = widest(pub, B)
    assert S == 21
    enc = pub.encrypt_batch([float(v) for v in x], device=True)
    assert min(enc.exponents) >= -18
    left = enc.segment_sum(ids, bins).cumsum(block=bins)
    packed = left.pack(S, B)
    assert len(packed) == -(-F * bins // S) == 10 and packed.on_device
    got = priv.decrypt_packed(packed, S, B, count=F * bins)
    clear = np.stack([np.bincount(row[row >= 0], weights=x[row >= 0], minlength=bins) for row in ids])
    assert np.allclose(np.array(got, dtype=float), np.cumsum(clear, axis=1).ravel(), rtol=0, atol=1e-9)
    assert got == priv.decrypt_batch(left)                                                # what one decrypt per number gives


def test_without_the_kernel_the_composition_gives_the_same_bits(monkeypatch):
    pub, priv = keypair(1024)
    n2 = pub.nsquare
    rs = np.random.Generator(np.random.PCG64(14))
    x = mixed(rs, 33)
    host = pub.encrypt_batch(x)
    cs = host.decrease_exponent_to(min(host.exponents)).ciphertexts(False)
    shapes = [(5, 29), (widest(pub, 80), 80)]
    kernel = {shape: host.to_device().pack(*shape).ciphertexts(False) for shape in shapes}
    monkeypatch.setattr(_engine.Engine, "has_segment_pack", lambda self: False)
    for S, B in shapes:
        want = integer_pack(cs, S, B, n2)
        assert kernel[(S, B)] == want
        for vec in (host, host.to_device(), host.to_device().to_pair()):
            out = vec.pack(S, B)
            assert out.on_device == vec.on_device and out._pair == vec._pair
            assert out.ciphertexts(False) == want, (S, B)
            assert out.exponents == [min(host.exponents)] * len(want)
    assert priv.decrypt_packed(host.to_device().pack(*shapes[1]), *shapes[1], count=33) == x


def test_mixed_exponents_and_negative_values_round_trip():
    pub, priv = keypair(2048)
    rs = np.random.Generator(np.random.PCG64(15))
    x, y = mixed(rs, 70), mixed(rs, 70)
    B = 96                                                                                # 53-bit mantissas at the smallest exponent
    S = widest(pub, B)
    va, vb = pub.encrypt_batch(x, device=True), pub.encrypt_batch(y, device=True)
    assert len(set(va.exponents)) > 1 and min(va.exponents + vb.exponents) >= -21     # |x| < 2^7: below 2^91
    pa = va.pack(S, B)
    assert set(pa.exponents) == {min(va.exponents)}
    assert priv.decrypt_packed(pa, S, B, count=70) == x
    assert priv.decrypt_packed(va.to_host().pack(S, B), S, B, count=70) == x
    both = pa.to_pair() + vb.to_pair().pack(S, B)                                         # packed vectors add slot by slot
    assert priv.decrypt_packed(both, S, B, count=70) == [u + v for u, v in zip(x, y)]
    tail = priv.decrypt_packed(pa, S, B)[70:]
    assert tail == [0.0] * (len(pa) * S - 70)
