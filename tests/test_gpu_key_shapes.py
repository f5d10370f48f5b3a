"""GPU tests (run with -m gpu on an MI355X): private keys whose primes are unequal in length or structured (tests/key_shapes.py,
tests/golden/key_shapes_primes.json) through the LIBRARY's own dispatch — the private ladder built per key, launch_crt_halves
(side by side, wave pairs, the late sweeps or two launches, each guarded by the two halves' geometries agreeing), both CRT tails
and the key owner's encryption.  The CPU emulator (tests/test_key_shapes.py) runs the same keys through the device headers but
makes these choices itself.  Expected plaintexts come from CPython ints (oracle/paillier_oracle.py PyPrivate: the reference's
formulas, its floor division included); nothing here reads the reference, and every key and row is valid input to it."""
import random
import sys

import numpy as np
import pytest

from conftest import PKG, load_golden

if PKG not in sys.path:
    sys.path.insert(0, PKG)

import key_shapes as ks  # noqa: E402

pytestmark = pytest.mark.gpu

BATCHES = (5, 300, 3000)
PATH_NAMES = (("UNIT", 1), ("OWNER", 2), ("SIDE_BY_SIDE", 4), ("PIPELINED", 8), ("FUSED_OBFUSCATE", 16), ("WAVE_PAIRS", 32),
              ("WAVE_TAIL", 64), ("LATE", 128), ("TABLE_MUL", 256), ("TILE_MUL", 512))
GOLDEN_SIZES = (256, 1024, 2048)                              # the balanced keys the zoo's paths are compared with


@pytest.fixture(scope="module")
def native():
    from phe import _native
    assert _native.device_count() >= 1
    return _native


def make_ctx(native, key):
    return native.Context(key.n, *key.constants(), n_limbs=key.s1)


def path_names(path):
    return "+".join(name for name, bit in PATH_NAMES if path & bit) or "-"


def golden_key(key_bits):
    g = load_golden(key_bits)
    return ks.ShapeKey("golden_%d" % key_bits, int(g["p"], 16), int(g["q"], 16))


_auto = {}


def auto_run(native, key):
    """decrypt of 5, 300 and 3000 rows (the fixed rows, then random ones) with the rung left to the library:
    {batch: (mismatch or None, last_launch)} and the context's private ladder; run once per key"""
    if key.name not in _auto:
        ctx = make_ctx(native, key)
        _, priv = ctx.ladder()
        fixed = key.rows()
        rows = [(c, m, tag) for c, m, tag in fixed] + [(c, m, "random") for c, m in key.random_rows(max(BATCHES) - len(fixed))]
        c = native.ints_to_limbs([r[0] for r in rows], key.s2)
        out = {}
        for batch in BATCHES:
            got = native.limbs_to_ints(ctx.decrypt(c[:batch]))
            out[batch] = (ks.first_mismatch(got, [r[1] for r in rows[:batch]], [r[2] for r in rows[:batch]]), ctx.last_launch())
        ctx.close()
        _auto[key.name] = (priv, out)
    return _auto[key.name]


@pytest.mark.parametrize("name", ks.NAMES)
def test_every_private_rung_decrypts_the_fixed_rows(native, c_oracle, name):
    """set_group(width) for every width of the key's private ladder: the plaintext bits of all 19 rows, libgmp's as well, and the
    geometry that ran is one of the ladder's"""
    key = ks.zoo()[name]
    ctx = make_ctx(native, key)
    _, priv = ctx.ladder()
    assert priv, priv
    rows = key.rows()
    c = native.ints_to_limbs([r[0] for r in rows], key.s2)
    want, tags = [r[1] for r in rows], [r[2] for r in rows]
    n_arr, p_arr, q_arr = (native.int_to_limbs(v, w) for v, w in ((key.n, key.s1), (key.p, key.pq), (key.q, key.pq)))
    assert native.limbs_to_ints(c_oracle.decrypt(n_arr, p_arr, q_arr, c, nthreads=4)) == want      # the two references agree
    try:
        for width in sorted({code // 100 for code in priv}):
            ctx.set_group(width)
            got = native.limbs_to_ints(ctx.decrypt(c))
            info = ctx.last_launch()
            print("%-14s group %2d -> geom %4d  %s" % (name, width, info["geom_priv"], path_names(info["path"])))
            bad = ks.first_mismatch(got, want, tags)
            assert bad is None, "%s group %d (ladder %s, ran %s): %s" % (name, width, priv, info, bad)
            assert info["geom_priv"] in priv, (name, width, priv, info)
    finally:
        ctx.set_group(0)
        ctx.close()


@pytest.mark.parametrize("name", ks.NAMES)
def test_batches_of_5_300_and_3000_rows_with_the_rung_left_to_the_library(native, name):
    key = ks.zoo()[name]
    priv, out = auto_run(native, key)
    for batch in BATCHES:
        bad, info = out[batch]
        assert bad is None, "%s batch %d (ladder %s, ran %s): %s" % (name, batch, priv, info, bad)
        assert info["geom_priv"] in priv, (name, batch, priv, info)


def test_unequal_keys_take_every_path_the_balanced_keys_take(native):
    """Over the zoo, every PATH_* bit the balanced golden key of the same size reports for these batch sizes is reported by an
    unequal key of that size too (no golden key has the 512 bits of proth_unequal: it is in the table only).  The table of
    key x batch -> (geometry, path bits) is printed: it shows which keys left side-by-side and the wave pairs.  LATE is reported by
    late_256 and late_2048 alone: the 16-lane late sweeps need both scaled moduli on one row count (key_setup.h build_private), so
    tiny_p, wide_a and wide_b run the textbook 16-lane kernel where the balanced key runs late."""
    zoo = ks.zoo()
    lines, taken = [], {}
    for name in ks.NAMES:
        key = zoo[name]
        priv, out = auto_run(native, key)
        for batch in BATCHES:
            bad, info = out[batch]
            assert bad is None, (name, batch, bad)
            taken.setdefault((32 * key.s1, batch), set()).add(info["path"])
            lines.append("%-14s %4d/%-4d ladder %-28s batch %4d -> geom %4d  %s" % (
                name, key.p.bit_length(), key.q.bit_length(), priv, batch, info["geom_priv"], path_names(info["path"])))
    missing = []
    for key_bits in GOLDEN_SIZES:
        key = golden_key(key_bits)
        priv, out = auto_run(native, key)
        for batch in BATCHES:
            bad, info = out[batch]
            assert bad is None, (key.name, batch, bad)
            lines.append("%-14s %4d/%-4d ladder %-28s batch %4d -> geom %4d  %s" % (
                key.name, key.p.bit_length(), key.q.bit_length(), priv, batch, info["geom_priv"], path_names(info["path"])))
            seen = 0
            for path in taken.get((key_bits, batch), ()):
                seen |= path
            if info["path"] & ~seen:
                missing.append((key_bits, batch, path_names(info["path"] & ~seen)))
    print("\nkey x batch -> (geometry, path bits) of decrypt, the rung left to the library")
    print("\n".join(lines))
    assert not missing, missing


@pytest.mark.parametrize("name", ["one_word", "regroup_a", "wide_b"])
def test_the_per_thread_tail_on_unequal_primes(native, name, monkeypatch):
    """PHE_HIP_NO_WAVE_TAIL: k_decrypt_tail (csrc/decrypt_tail.h: h = words of q, p zero-padded, one conditional + q) on every
    private rung for the fixed rows, and on 300 rows with the rung left to the library"""
    key = ks.zoo()[name]
    monkeypatch.setenv("PHE_HIP_NO_WAVE_TAIL", "1")
    ctx = make_ctx(native, key)
    _, priv = ctx.ladder()
    fixed = key.rows()
    rows = [(c, m, tag) for c, m, tag in fixed] + [(c, m, "random") for c, m in key.random_rows(300 - len(fixed), seed=2)]
    c = native.ints_to_limbs([r[0] for r in rows], key.s2)
    want, tags = [r[1] for r in rows], [r[2] for r in rows]
    try:
        for width in sorted({code // 100 for code in priv}):
            ctx.set_group(width)
            got = native.limbs_to_ints(ctx.decrypt(c[:len(fixed)]))
            info = ctx.last_launch()
            assert not info["path"] & ctx.PATH_WAVE_TAIL, info
            bad = ks.first_mismatch(got, want[:len(fixed)], tags)
            assert bad is None, "%s group %d (%s): %s" % (name, width, info, bad)
        ctx.set_group(0)
        got = native.limbs_to_ints(ctx.decrypt(c))
        assert not ctx.last_launch()["path"] & ctx.PATH_WAVE_TAIL
        bad = ks.first_mismatch(got, want, tags)
        assert bad is None, "%s 300 rows (%s): %s" % (name, ctx.last_launch(), bad)
    finally:
        ctx.set_group(0)
        ctx.close()


@pytest.mark.parametrize("name", ks.NAMES)
def test_key_owner_encryption_where_it_is_offered(native, name):
    """encrypt_owner (r^n from the CRT halves mod p^2 and q^2, lifted: key_setup.h build_owner_lift relies on p^2 < q^2) gives the
    bits of encrypt and of CPython, a handful of rows and 300; where the library does not offer it the call raises ValueError.
    It is offered for one_bit as it is for the golden 1024-bit key."""
    key = ks.zoo()[name]
    ctx = make_ctx(native, key)
    er = key.encrypt_rows()
    try:
        for reps in (1, 22):                                       # 14 rows, and 308: another rung of the halves
            m = native.ints_to_limbs([r[0] for r in er] * reps, key.s1)
            r = native.ints_to_limbs([r[1] for r in er] * reps, key.s1)
            want, tags = [r[2] for r in er] * reps, [r[3] for r in er] * reps
            bad = ks.first_mismatch(native.limbs_to_ints(ctx.encrypt(m, r)), want, tags)
            assert bad is None, "%s encrypt of %d rows (%s): %s" % (name, len(want), ctx.last_launch(), bad)
            if ctx.owner_encrypt_offered():
                got = native.limbs_to_ints(ctx.encrypt_owner(m, r))
                info = ctx.last_launch()
                assert info["path"] & ctx.PATH_OWNER, info
                bad = ks.first_mismatch(got, want, tags)
                assert bad is None, "%s encrypt_owner of %d rows (%s): %s" % (name, len(want), info, bad)
            else:
                with pytest.raises(ValueError):
                    ctx.encrypt_owner(m, r)
        print("%-14s owner encryption %s" % (name, "offered" if ctx.owner_encrypt_offered() else "not offered"))
        if name == "one_bit":
            assert ctx.owner_encrypt_offered()
    finally:
        ctx.close()


def test_drop_in_api_round_trip_with_the_primes_in_the_wrong_order(native):
    """regroup_b (384 / 640 bits) through phe.PaillierPrivateKey(pub, q, p), as the reference takes it"""
    import phe
    key = ks.zoo()["regroup_b"]
    pub = phe.PaillierPublicKey(key.n)
    priv = phe.PaillierPrivateKey(pub, key.q, key.p)
    assert (priv.p, priv.q, priv.hp, priv.hq, priv.p_inverse) == key.constants()
    assert priv.decrypt(pub.encrypt(-12.5)) == -12.5
    assert priv.raw_decrypt(pub.raw_encrypt(key.n - 1, r_value=key.unit(random.Random(5)))) == key.n - 1
    xs = np.arange(40, dtype=np.float64) / 4 - 3
    assert priv.decrypt_batch(pub.encrypt_batch(xs)) == xs.tolist()
