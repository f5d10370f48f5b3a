"""Private keys whose primes are unequal in length or structured (tests/key_shapes.py, tests/golden/key_shapes_primes.json) through
the device headers on the CPU wave emulator: csrc/key_setup.h (build_tail pads the shorter prime to h = words of q and insists on
p < q, build_private sizes both halves from q^2 and rebuilds the halves' pair geometries where p and q disagree, build_tail_wave
and build_owner_lift size everything from q), csrc/decrypt_tail.h (one conditional + q rests on m_p < p < q) and build_schedule's
squarings-only last op (Proth primes).  Every other private key of the suite has primes of one bit length and no structure.
Expected values: CPython ints (oracle/paillier_oracle.py PyPrivate), cross-checked against libgmp."""
import random
import sys

import pytest

from conftest import PKG

if PKG not in sys.path:
    sys.path.insert(0, PKG)

import key_shapes as ks  # noqa: E402
from oracle.paillier_oracle import int_to_limbs, ints_to_limbs, limbs_to_ints  # noqa: E402


@pytest.fixture(scope="module")
def emu():
    from emu_lib import Emu
    e = Emu()
    e.set_engine(True)
    return e


def key_arrays(key):
    return [int_to_limbs(v, key.pq) for v in key.constants()]


def groups_of(name):
    return (0, 16) if name in ks.WIDE else (0, 4, 16, 64)      # (a whole-wave run of a 2048-bit key's rows takes ~23 s here)


def decrypt_all_ways(emu, key, groups):
    """the fixed rows on every group width in `groups` with both tails; raises RuntimeError (the emulator's) where key_setup.h
    refuses the key.  Narrow groups run all 19 rows under each tail.  From 16 lanes on, where an emulated row of a 1024-bit key costs
    0.3 ... 0.6 s and nearly all of it is the two half-exponentiations, every row runs ONCE on the group: the rows are dealt out
    between the tails, even ones to the per-thread tail and odd ones to the wave tail (both orders of m_p, m_q and a c = k p or
    k q row fall to each) — the tails read only the canonical x_p, x_q words, whatever group made them.  For keys above 512 bits
    these wide groups also leave out the eight rows whose like is still there: m = 0, 1, p - 1, q - 1, n - p and the random ones."""
    rows = key.rows()
    few = [r for r in rows if r[2] not in ("m = 0", "m = 1", "m = p - 1", "m = q - 1", "m = n - p", "m random")]
    assert len(rows) == 19 and len(few) == 11
    arrs = key_arrays(key)
    try:
        for group in groups:
            emu.set_group(group)
            for wave_tail in (False, True):
                emu.set_wave_tail(wave_tail)
                part = rows if group < 16 else (few if key.n.bit_length() > 512 else rows)[int(wave_tail)::2]
                assert any(m % key.q < m % key.p for _, m, _ in part) and any(m % key.q >= m % key.p for _, m, _ in part)
                got = limbs_to_ints(emu.decrypt(*arrs, key.s1, ints_to_limbs([r[0] for r in part], key.s2)))
                bad = ks.first_mismatch(got, [r[1] for r in part], [r[2] for r in part])
                assert bad is None, "%s group %d, %s tail: %s" % (key.name, group, "wave" if wave_tail else "per-thread", bad)
    finally:
        emu.set_group(0)
        emu.set_wave_tail(False)


def test_the_zoo_is_what_its_table_says():
    """the shapes the fixture promises, checked on the committed primes (gen_key_shapes.py is not run by the suite)"""
    zoo = ks.zoo()
    bits = {name: (k.p.bit_length(), k.q.bit_length()) for name, k in zoo.items()}
    assert bits == {"one_bit": (511, 513), "one_word": (496, 528), "regroup_a": (448, 576), "regroup_b": (384, 640),
                    "regroup_c": (256, 768), "wide_a": (1000, 1048), "wide_b": (928, 1120), "tiny_p": (33, 223),
                    "twins": (512, 512), "proth": (512, 512), "proth_unequal": (200, 312), "edges": (512, 512),
                    "late_256": (120, 136), "late_2048": (1016, 1032)}
    for k in zoo.values():
        assert k.p < k.q and ks._is_prime(k.p) and ks._is_prime(k.q)
    t = zoo["twins"]
    assert not any(ks._is_prime(x) for x in range(t.p + 2, t.q, 2))
    assert min(ks.trailing_zeros(zoo["proth"].p - 1), ks.trailing_zeros(zoo["proth"].q - 1)) >= 180
    assert (ks.trailing_zeros(zoo["proth_unequal"].p - 1), ks.trailing_zeros(zoo["proth_unequal"].q - 1)) == (150, 250)
    e = zoo["edges"]
    assert not any(ks._is_prime(x) for x in range((1 << 511) + 1, e.p, 2)) and not any(ks._is_prime(x) for x in range(e.q + 2, 1 << 512, 2))
    for k in (e.p, e.p * e.p):                                  # top limb all zeros below the leading bit ...
        assert k >> (k.bit_length() - 30) == 1 << 29
    for k in (e.q, e.q * e.q):                                  # ... and all ones
        assert k >> (k.bit_length() - 30) == (1 << 30) - 1


def test_the_two_references_agree_on_every_row(c_oracle):
    """PyPrivate.raw_decrypt (CPython pow, the reference's floor division restated) against libgmp, multiples of p and q included"""
    for key in ks.zoo().values():
        rows = key.rows()
        c = ints_to_limbs([r[0] for r in rows], key.s2)
        got = c_oracle.decrypt(int_to_limbs(key.n, key.s1), int_to_limbs(key.p, key.pq), int_to_limbs(key.q, key.pq), c, nthreads=4)
        assert limbs_to_ints(got) == [r[1] for r in rows], key.name
        assert c_oracle.private_constants(key.n, key.q, key.p, key.s1, key.pq) == key.constants(), key.name


@pytest.mark.parametrize("name", ks.NAMES)
def test_no_zoo_key_is_refused_and_every_rung_and_tail_decrypts(emu, name):
    decrypt_all_ways(emu, ks.zoo()[name], groups_of(name))


@pytest.mark.parametrize("name", ks.NAMES)
def test_encrypt_and_the_key_owners_encrypt(emu, name):
    """raw_encrypt under the zoo's n (Proth primes give n = 1 mod 2^180: long zero runs in the exponent n) and, where the key has
    the geometries for it, by its CRT halves (build_owner_lift: p^2 < q^2, the lift's width from q^2)"""
    key = ks.zoo()[name]
    er = key.encrypt_rows()
    if name in ks.WIDE:
        er = er[:2] + er[4:5] + er[11:12]                       # (~1 s per emulated 2048-bit row: r = 1, n - 1; m = q; a random row)
    n = int_to_limbs(key.n, key.s1)
    m, r = ints_to_limbs([x[0] for x in er], key.s1), ints_to_limbs([x[1] for x in er], key.s1)
    want, tags = [x[2] for x in er], [x[3] for x in er]
    emu.set_group(0)
    bad = ks.first_mismatch(limbs_to_ints(emu.encrypt(n, m, r)), want, tags)
    assert bad is None, "%s encrypt: %s" % (name, bad)
    out = emu.encrypt_owner(n, *key_arrays(key), m, r)
    if out is not None:
        bad = ks.first_mismatch(limbs_to_ints(out), want, tags)
        assert bad is None, "%s encrypt_owner: %s" % (name, bad)
    if name == "one_bit":
        assert out is not None                                  # as for the balanced 1024-bit keys


@pytest.mark.parametrize("name", ks.NAMES)
def test_the_small_batch_kernels_where_the_key_has_their_constants(emu, name):
    """wave pairs (Lw = max(Lp, Lq) for both halves) and the late sweeps on the 16-lane rung (the two quick packs must agree on
    their row count or both are dropped): three rows each where key_setup.h built the constants, the emulator's refusal otherwise"""
    key = ks.zoo()[name]
    rows = key.rows()
    rows = [rows[i] for i in (2, 4, 17)]                         # m = n - 1, m = q (m_q < m_p), c = k p
    c = ints_to_limbs([r[0] for r in rows], key.s2)
    want, tags = [r[1] for r in rows], [r[2] for r in rows]
    arrs = key_arrays(key)
    ran = 0
    try:
        for group, pairs, late in ((64, True, False), (16, False, True)):
            emu.set_group(group), emu.set_wave_pairs(pairs), emu.set_late(late), emu.set_wave_tail(True)
            try:
                got = limbs_to_ints(emu.decrypt(*arrs, key.s1, c))
            except RuntimeError as ex:
                assert str(ex) in ("no wave-pair constants for this key", "no late kernel for this key / group",
                                   "no wave-pair kernel for this L"), ex
                continue
            ran += 1
            bad = ks.first_mismatch(got, want, tags)
            assert bad is None, "%s group %d pairs %s late %s: %s" % (name, group, pairs, late, bad)
    finally:
        emu.set_group(0), emu.set_wave_pairs(False), emu.set_late(False), emu.set_wave_tail(False)
    if name in ("late_256", "late_2048"):
        assert ran == 2, ran                                     # what these two keys are in the zoo for


# ---- the drop-in API on the emulator backend ----------------------------------------------------------------------------------------
@pytest.fixture
def emu_api(monkeypatch):
    import emu_backend
    emu_backend.install(monkeypatch)
    import phe
    return phe


@pytest.mark.parametrize("name", ks.NAMES)
def test_primes_in_the_wrong_order_through_the_drop_in_api(emu_api, name):
    """PaillierPrivateKey(pub, q, p), as the reference takes it: an encoded float and n - 1"""
    phe = emu_api
    key = ks.zoo()[name]
    pub = phe.PaillierPublicKey(key.n)
    priv = phe.PaillierPrivateKey(pub, key.q, key.p)
    assert (priv.p, priv.q, priv.hp, priv.hq, priv.p_inverse) == key.constants()
    rng = random.Random("api " + name)
    c = key.encrypt(key.n - 1, key.unit(rng))
    assert priv.raw_decrypt(c) == key.n - 1
    x = -12.5
    enc = phe.EncodedNumber.encode(pub, x)
    number = phe.EncryptedNumber(pub, key.encrypt(enc.encoding, key.unit(rng)), enc.exponent)
    assert priv.decrypt(number) == x


@pytest.mark.parametrize("name", ["one_bit", "regroup_a"])
def test_from_totient_rebuilds_the_key(emu_api, name):
    phe = emu_api
    key = ks.zoo()[name]
    pub = phe.PaillierPublicKey(key.n)
    priv = phe.PaillierPrivateKey.from_totient(pub, (key.p - 1) * (key.q - 1))
    assert (priv.p, priv.q, priv.hp, priv.hq, priv.p_inverse) == key.constants()
    assert priv == phe.PaillierPrivateKey(pub, key.q, key.p)
    c = key.encrypt(key.q - key.p, key.unit(random.Random("totient " + name)))
    assert priv.raw_decrypt(c) == key.q - key.p


# ---- where key_setup.h starts to refuse ---------------------------------------------------------------------------------------------
def test_the_refusal_boundary_of_256_bit_keys(emu):
    """n of 256 bits, p of 16, 24, ..., 120 bits: a key either builds and decrypts every fixed row on the automatic rung and on the whole wave, both tails, or
    building its plans for the automatic rung (what context creation runs; the library turns the exception into ValueError) raises
    with one of key_setup.h's refusals.  A forced group width whose plans are refused is a rung the library's ladder leaves out
    (phe_hip_ctx_create_private skips it): the other widths must still decrypt.  A wrong plaintext or any other exception fails.
    The refused splits are printed (DESIGN.md "Key shapes" records them)."""
    refused, no_rung = {}, {}
    for p_bits in ks.SWEEP_P_BITS:
        key = ks.sweep_key(p_bits)
        assert key.p.bit_length() == p_bits and key.n.bit_length() == ks.SWEEP_N_BITS
        arrs = key_arrays(key)
        try:
            emu.set_group(0)
            emu.private_split_geometry(*arrs, key.s1)             # build_private alone
        except RuntimeError as ex:
            assert str(ex) in ks.REFUSALS, (p_bits, ex)
            refused[p_bits] = str(ex)
            continue
        groups = [0]
        for group in (64,):                                      # the narrowest and the widest layout of the halves
            try:
                emu.set_group(group)
                emu.private_split_geometry(*arrs, key.s1)
                groups.append(group)
            except RuntimeError as ex:
                assert str(ex) in ks.REFUSALS, (p_bits, group, ex)
                no_rung.setdefault(p_bits, []).append(group)
            finally:
                emu.set_group(0)
        decrypt_all_ways(emu, key, groups)
    print("refused at context creation:", refused)
    print("forced widths without a rung:", no_rung)
    assert len(refused) < len(ks.SWEEP_P_BITS)                   # (the balanced end of the sweep is served)
