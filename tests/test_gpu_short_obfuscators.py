"""Short-exponent obfuscators on the GPU (csrc/fixed_base.h fixed_base_pow_body through phe_hip_fixed_base_pow_dev): whichever
route makes it, every ciphertext must be the Python-integer formula of tests/short_cases.py — (1 + n*m) * pow(h_s, rho, n^2)
mod n^2 for an encryption (the reference's raw_encrypt(m, r_value=pow(h, rho, n)), phe/paillier.py:102-139) and
c * pow(h_s, rho, n^2) mod n^2 for a re-randomisation — and what is decrypted must be what went in.  At most 61 distinct
exponents per key (CPython's pow at this size takes tens of milliseconds), reused across the rows: rho_i = set[i mod 61]."""
import sys

import numpy as np
import pytest

from conftest import PKG, load_golden

if PKG not in sys.path:
    sys.path.insert(0, PKG)

from phe import _engine, paillier  # noqa: E402
from phe._engine import Engine  # noqa: E402
from phe.ciphertext import EncryptedVector  # noqa: E402

from short_cases import X_FIXED, base_of, edge_exponents, ints, limbs  # noqa: E402

pytestmark = pytest.mark.gpu

H = lambda s: int(s, 16)


def keypair(bits):
    g = load_golden(bits)
    pub = paillier.PaillierPublicKey(H(g["n"]))
    return pub, paillier.PaillierPrivateKey(pub, H(g["p"]), H(g["q"]))


class Case:
    """one key with short obfuscators on at the default length, its 61 exponents and their powers (Python integers, made once)"""

    def __init__(self, bits):
        self.pub, self.priv = keypair(bits)
        self.n, self.n2 = self.pub.n, self.pub.nsquare
        self.h, self.hs = base_of(self.n)
        assert self.pub.enable_short_obfuscators(x=X_FIXED) == self.hs
        self.bits = self.pub.short_obfuscator_bits
        assert self.bits == bits // 2
        self.priv._get_engine()                      # the key pair's engine from the start: the public key works through it
        eng = self.pub._get_engine()
        assert eng.has_fixed_base()
        self.info = eng.short_table_info()
        self.set = edge_exponents(self.bits, self.info["window"])
        self.power = [pow(self.hs, r, self.n2) for r in self.set]
        self.el = (self.bits + 31) // 32
        self.set_limbs = limbs(self.set, self.el)

    def rho(self, rows):
        """(exponent rows, their obfuscators) for rho_i = set[i mod 61]"""
        idx = np.arange(rows) % len(self.set)
        return np.ascontiguousarray(self.set_limbs[idx]), [self.power[i] for i in idx]


@pytest.fixture(scope="module")
def cases():
    made = {}

    def get(bits):
        if bits not in made:
            made[bits] = Case(bits)
        return made[bits]
    return get


def fixed_draws(monkeypatch, case):
    """random_bits_limbs hands out set[0], set[1], ... in turn, starting over with every call"""
    def fake(bits, count, width, out=None):
        assert bits == case.bits and width == case.el
        rows = case.rho(count)[0]
        if out is None:
            return rows
        out[:] = rows
        return out
    monkeypatch.setattr(_engine, "random_bits_limbs", fake)


@pytest.mark.parametrize("bits", [1024, 2048])
@pytest.mark.parametrize("rows", [1, 2, 17, 16 * 67 + 15])
def test_every_row_against_the_formula(cases, monkeypatch, bits, rows):
    k = cases(bits)
    pub, n, n2, eng = k.pub, k.n, k.n2, k.pub._get_engine()
    rho, power = k.rho(rows)
    rs = np.random.Generator(np.random.PCG64(bits + rows))
    values = rs.integers(-10 ** 12, 10 ** 12, rows)
    want = [(1 + n * (int(v) % n)) * o % n2 for v, o in zip(values, power)]
    host = pub.encrypt_batch(values, rho_values=rho)                              # host result
    assert not host.on_device and host.ciphertexts(False) == want
    if rows == 17:                                                                # the reference's raw_encrypt with r = h^rho
        assert want == pub.raw_encrypt_batch([int(v) % n for v in values], r_values=[pow(k.h, r, n) for r in k.set[:17]])
        assert pub.encrypt_batch(values, rho_values=k.set[:17]).ciphertexts(False) == want      # exponents as integers
    dev = pub.encrypt_batch(values, rho_values=rho, device=True)                  # resident result
    assert dev.on_device and dev.ciphertexts(False) == want
    assert k.priv.decrypt_batch(dev) == values.tolist()
    # the pool route: obfuscators made ahead of time for the exponents that the draw hands out, as pair rows
    fixed_draws(monkeypatch, k)
    pub.discard_obfuscators()
    assert pub.precompute_obfuscators(rows) == rows
    assert eng._obf.blocks[0][0].cols == eng.pair_form() != eng.ct_limbs
    if rows <= 17:
        assert eng.peek_obfuscators(rows) == power
    pooled = pub.encrypt_batch(values, device=True)
    assert pooled.ciphertexts(False) == want and pub.obfuscators_available() == 0
    # obfuscate: resident canonical rows, and pair rows (which stay in the form)
    cs = [int.from_bytes(rs.bytes(n2.bit_length() // 8 - 1), "little") | 1 for _ in range(rows)]
    cs[0] = n2 - 1
    want_c = [c * o % n2 for c, o in zip(cs, power)]
    vec = EncryptedVector.from_ciphertexts(pub, cs).to_device()
    assert vec.obfuscate(rho_values=rho).ciphertexts(False) == want_c and vec.on_device and not vec._pair
    pair = EncryptedVector.from_ciphertexts(pub, cs).to_pair()
    pair.obfuscate(rho_values=rho)
    assert pair._pair and pair._obfuscated.all() and pair.ciphertexts(False) == want_c
    # fresh draws (the pool refilled for a small vector, drawn on the spot for a large one): pair rows stay in the form
    fresh = EncryptedVector.from_ciphertexts(pub, cs).to_pair()
    pub.discard_obfuscators()
    fresh.obfuscate()
    assert fresh._pair and fresh.ciphertexts(False) == want_c
    plain = EncryptedVector.from_ciphertexts(pub, cs).to_device()                 # ... and resident canonical rows
    pub.discard_obfuscators()
    assert plain.obfuscate().ciphertexts(False) == want_c
    pub.discard_obfuscators()
    # encrypt_packed: one exponent per packed row
    S, B = 3, 41
    small = rs.integers(-2 ** 40, 2 ** 40, rows * S - 1)
    padded = np.append(small, 0).reshape(rows, S)
    ms = [sum(int(x) << (B * j) for j, x in enumerate(row)) % n for row in padded]
    packed = pub.encrypt_packed(small, S, B, rho_values=rho, device=True)
    assert packed.ciphertexts(False) == [(1 + n * m) * o % n2 for m, o in zip(ms, power)]


def test_every_row_on_the_3072_bit_key(cases):
    k = cases(3072)
    rows = 17
    rho, power = k.rho(rows)
    values = np.arange(-8, 9, dtype=np.int64) * 10 ** 9
    want = [(1 + k.n * (int(v) % k.n)) * o % k.n2 for v, o in zip(values, power)]
    assert k.pub.encrypt_batch(values, rho_values=rho).ciphertexts(False) == want
    dev = k.pub.encrypt_batch(values, rho_values=rho, device=True)
    assert dev.ciphertexts(False) == want and k.priv.decrypt_batch(dev) == values.tolist()
    pair = EncryptedVector.from_ciphertexts(k.pub, want).to_pair()
    pair.obfuscate(rho_values=rho)
    assert pair._pair and pair.ciphertexts(False) == [c * o % k.n2 for c, o in zip(want, power)]


def test_65537_rows_and_then_three(cases):
    k = cases(2048)
    pub, n, n2 = k.pub, k.n, k.n2
    eng = pub._get_engine()
    rows = (1 << 16) + 1
    rho, power = k.rho(rows)
    values = np.arange(rows, dtype=np.int64) * 1000003 - (1 << 35)                # a different plaintext in every row
    dev = pub.encrypt_batch(values, rho_values=rho, device=True)
    wide = eng.ctx.last_launch()["geom_pub"]
    got = dev.ciphertexts(False)
    for i in range(rows):
        assert got[i] == (1 + n * (int(values[i]) % n)) * power[i] % n2, i
    few = pub.encrypt_batch(values[:3], rho_values=rho[:3], device=True)
    narrow = eng.ctx.last_launch()["geom_pub"]
    assert few.ciphertexts(False) == got[:3]
    for code in (wide, narrow):
        assert 2 * (code // 100) * (code % 100) == eng.pair_form(), code          # a rung that serves the pair rows
    assert wide != narrow, (wide, narrow)                                         # the picker of the pair kernels: two geometries


@pytest.mark.parametrize("bits", [1024, 2048])
def test_without_the_kernel_the_composition_gives_the_same_bits(cases, monkeypatch, bits):
    k = cases(bits)
    pub, n, n2 = k.pub, k.n, k.n2
    rows = 67
    rho, power = k.rho(rows)
    rs = np.random.Generator(np.random.PCG64(bits))
    values = rs.integers(-10 ** 9, 10 ** 9, rows)
    cs = [int.from_bytes(rs.bytes(n2.bit_length() // 8 - 1), "little") | 1 for _ in range(rows)]

    def all_routes():
        out = [pub.encrypt_batch(values, rho_values=rho).ciphertexts(False),
               pub.encrypt_batch(values, rho_values=rho, device=True).ciphertexts(False)]
        for make in (lambda v: v, lambda v: v.to_device(), lambda v: v.to_pair()):      # host, resident and pair inputs
            vec = make(EncryptedVector.from_ciphertexts(pub, cs))
            out.append(vec.obfuscate(rho_values=rho).ciphertexts(False))
        return out
    with_kernel = all_routes()
    assert with_kernel[0] == [(1 + n * (int(v) % n)) * o % n2 for v, o in zip(values, power)]
    assert with_kernel[2] == [c * o % n2 for c, o in zip(cs, power)]
    monkeypatch.setattr(Engine, "has_fixed_base", lambda self: False)
    assert not pub._get_engine().has_fixed_base()
    assert all_routes() == with_kernel


def test_fresh_draws(cases):
    k = cases(2048)
    pub, priv = k.pub, k.priv
    pub.discard_obfuscators()
    rows = 4096
    values = np.full(rows, 42, dtype=np.int64)
    vec = pub.encrypt_batch(values, device=True)
    got = vec.ciphertexts(False)
    assert len(set(got)) == rows
    assert priv.decrypt_batch(vec) == [42] * rows
    host = pub.encrypt_batch(values)
    assert len(set(host.ciphertexts(False)) | set(got)) == 2 * rows and priv.decrypt_batch(host) == [42] * rows
    small = np.arange(-3000, 3001, dtype=np.int64)
    packed = pub.encrypt_packed(small, 31, 64, device=True)
    assert priv.decrypt_packed(packed, 31, 64, count=len(small)) == small.tolist()
    number = pub.encrypt(3.5)                                                     # the scalar call, through the pool refill
    assert priv.decrypt(number) == 3.5


def test_table_entries_and_a_second_base(cases):
    k = cases(1024)
    pub, n, n2 = k.pub, k.n, k.n2
    eng = pub._get_engine()
    info = eng.short_table_info()
    w, T = info["window"], info["positions"]
    per_pos = (1 << w) - 1
    assert info["bits"] == k.bits and 1 <= w <= 12 and T == -(-k.bits // w)
    assert info["table_bytes"] == T * per_pos * eng.pair_form() * 4
    rs = np.random.Generator(np.random.PCG64(5))
    picks = [(0, 1), (T - 1, per_pos), (T - 1, 1)] + [(int(rs.integers(T)), int(rs.integers(1, per_pos + 1))) for _ in range(3)]
    for t, d in picks:
        row = eng.short_table_rows_dev(t * per_pos + d - 1, 1)
        assert ints(eng.from_pair_dev(row).to_host()) == [pow(k.hs, d << (w * t), n2)], (t, d)
    with pytest.raises(ValueError):
        eng.short_table_rows_dev(T * per_pos, 1)                                  # beyond the table
    # a second base replaces the first: new ciphertexts follow the new h_s
    x2 = X_FIXED + 2
    _, hs2 = base_of(n, x2)
    try:
        assert pub.enable_short_obfuscators(bits=33, x=x2) == hs2
        eng = pub._get_engine()
        info2 = eng.short_table_info()
        assert info2["bits"] == 33 and info2["positions"] == -(-33 // info2["window"])
        rhos = [0, 1, (1 << 33) - 1, 1 << 32, 0x155555555]
        vec = pub.encrypt_batch([7] * 5, rho_values=rhos, device=True)
        assert vec.ciphertexts(False) == [(1 + 7 * n) * pow(hs2, r, n2) % n2 for r in rhos]
        pub.disable_short_obfuscators()
        assert eng.ctx.fixed_base_info() == {"bits": 0, "window": 0, "positions": 0, "table_bytes": 0}
        with pytest.raises(ValueError):
            eng.ctx.fixed_base_pow_dev(0, 2, None, False, None, 0, True, 1)       # no table: refused before anything is read
    finally:
        pub.enable_short_obfuscators(x=X_FIXED)                                   # (the module's shared case goes on as it was)
