"""GPU side of tests/test_lookahead.py (run with -m gpu on an MI355X): result-first rows through the C-ABI.

The ciphertext t is chosen first, with its radix-2^29 digits laid out on the lanes of a limb group so that whole lanes equal
n^2's, are all ones, all zero, next to 0 or n^2, or straddle the two halves of the split exit (tests/lookahead.py); the inputs
follow from the private key.  The library picks its rung from the batch size and its settings, so ONE batch holds the rows of
every layout a rung of this key can end on (every (G, L) of the context's ladder as a pair of halves, with the row counts of the
plain and of the scaled-modulus form, and n^2's full-width geometries), and that batch goes through every rung and setting.
Every result is compared with the chosen target and with the libgmp oracle.  Nothing here reads the reference tree."""
import os
import random
import sys

import numpy as np
import pytest

from conftest import PKG, load_golden

if PKG not in sys.path:
    sys.path.insert(0, PKG)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import lookahead as la  # noqa: E402

pytestmark = pytest.mark.gpu

KEY_BITS = 1024
FULL_GL = {16: (1, 2, 3, 5, 7, 9, 14, 18), 8: (5, 9, 14, 18, 27), 4: (9, 18, 27, 36), 2: (18, 36)}   # csrc/kernels_g*.hip


def H(x):
    return int(x, 16)


@pytest.fixture(scope="module")
def native():
    from phe import _native
    assert _native.device_count() >= 1
    return _native


def _ctx(native, g, private=True):
    if private:
        return native.Context(H(g["n"]), H(g["p"]), H(g["q"]), H(g["hp"]), H(g["hq"]), H(g["p_inverse"]), n_limbs=g["key_bits"] // 32)
    return native.Context(H(g["n"]), n_limbs=g["key_bits"] // 32)


def layouts_of(n, ladder_pub):
    """(nl, L, half) of every way a kernel of this key lays n^2 out for its last subtraction (csrc/key_setup.h build_split /
    build_quick / pick_geometry restated): the ladder's rungs as two halves of `rows` digits — rows = G L, the least multiple of
    the whole wave's trip, or the least multiple of L that covers the scaled modulus k n — and the full-width geometries"""
    bits = n.bit_length()
    need = -(-(bits + 4) // 29)
    k = (-pow(n, -1, 1 << 29)) % (1 << 29)
    need_scaled = -(-((n * k).bit_length() + 4) // 29)
    out = set()
    for code in ladder_pub:
        G, L = code // 100, code % 100
        rows = {G * L}
        if G == 64:
            trip = (4 if L == 1 else 2) * L
            rows = {min(64 * L, -(-need // trip) * trip)}
        if G >= 16:
            rows.add(-(-need_scaled // L) * L)
        for r in rows:
            if r <= G * L:
                out.add((2 * r // L, L, r // L))
    need_sq = -(-(2 * bits + 4) // 29)
    for G, Ls in FULL_GL.items():
        fit = [L for L in Ls if G * L >= need_sq]
        if fit:
            out.add((G, min(fit), None))
    return sorted(out, key=lambda x: (x[0], x[1], x[2] or 0))


@pytest.fixture(scope="module")
def rows(native):
    """the batch: [(t, tag)], with its encrypt / obfuscate / powmod / product preimages, for the 1024-bit golden key"""
    g = load_golden(KEY_BITS)
    key = la.KeyMath(H(g["p"]), H(g["q"]))
    ctx = _ctx(native, g, private=False)
    pub, _ = ctx.ladder()
    ctx.close()
    rng = random.Random(9000)
    M = key.nsq
    batch = []
    for nl, L, half in layouts_of(key.n, pub):
        arrives = lambda t: la.borrow_arrives(t, M, nl, L)
        fam = {}
        for f in la.FAMILIES:
            ts = la.unit_targets(la.family_targets(M, nl, L, rng, f, half), key.n)
            fam[f] = la.thin_cells(ts, arrives)              # every run start, with the borrow arriving and without: none is lost
            assert {la.run_start(tag) for _, tag in ts} == {la.run_start(tag) for _, tag in fam[f]}, f
            for want in (True, False):
                if any(bool(arrives(t)) == want for t, _ in ts):
                    assert any(bool(arrives(t)) == want for t, _ in fam[f]), (f, want)
        assert any(arrives(t) for t, _ in fam["EQ"]) and any(not arrives(t) for t, _ in fam["EQ"])
        if max(g_ for g_, v in enumerate(la.split_lanes(M, nl, L)) if v) > 1:   # (on two lanes the only lane that can propagate is EQ's)
            assert any(arrives(t) for t, _ in fam["HALF"]) and any(not arrives(t) for t, _ in fam["HALF"])
        assert all(any(not arrives(t) for t, _ in fam[f]) for f in ("ONES", "ZERO", "NEAR"))
        per = max(1, 128 // nl) if half else 64 // nl
        part = la.batch_layout(fam, min(per, 16), rng, lambda: la.random_unit(M, rng), 16)
        batch += [(t, "%dx%d %s" % (nl, L, tag)) for t, tag in part]
    s1, s2 = KEY_BITS // 32, KEY_BITS // 16
    enc = [key.preimage_encrypt(t, check=i % 97 == 0) for i, (t, _) in enumerate(batch)]   # (every row is checked against libgmp below)
    obf = [key.preimage_obfuscate(t, rng, pre, check=i % 97 == 0) for i, ((t, _), pre) in enumerate(zip(batch, enc))]
    ks = [key.coprime_exponent((3, rng.getrandbits(17) | 1, rng.getrandbits(64) | 1, rng.randrange(key.n >> 1) | 1)[i % 4])
          for i in range(len(batch))]
    bases = [key.preimage_powmod(t, k, check=i % 97 == 0) for i, ((t, _), k) in enumerate(zip(batch, ks))]
    import adversarial
    a, b = adversarial.pairs_for([t for t, _ in batch], M, rng, n_root=key.n)
    L_ = native.ints_to_limbs
    return {"g": g, "key": key, "rows": batch, "want": L_([t for t, _ in batch], s2),
            "m": L_([m for m, _ in enc], s1), "r": L_([r for _, r in enc], s1),
            "c_in": L_([c for c, _ in obf], s2), "r_obf": L_([r for _, r in obf], s1),
            "base": L_(bases, s2), "k": L_(ks, s1), "a": L_(a, s2), "b": L_(b, s2)}


def _tile(arr, count):
    reps = -(-count // arr.shape[0])
    return np.ascontiguousarray(np.tile(arr, (reps, 1))[:count])


def _same(got, want, rows, what):
    if np.array_equal(got, want):
        return
    bad = np.nonzero((got != want).any(axis=1))[0]
    i = int(bad[0])
    raise AssertionError("%s: row %d (%s) differs; %d of %d rows wrong" % (what, i, rows[i % len(rows)][1], len(bad), len(want)))


def _hot_path(native, ctx, R, c_oracle, count, what, decrypt=True, oracle=True):
    """the batch (tiled to `count` rows) through encrypt, obfuscate, powmod, the product and decrypt of ctx"""
    want = _tile(R["want"], count)
    m, r = _tile(R["m"], count), _tile(R["r"], count)
    got = ctx.encrypt(m, r)
    _same(got, want, R["rows"], what + " encrypt")
    if oracle:
        n_arr = native.int_to_limbs(R["key"].n, KEY_BITS // 32)
        _same(got, c_oracle.encrypt(n_arr, m, r, nthreads=16), R["rows"], what + " encrypt vs libgmp")
    _same(ctx.obfuscate(_tile(R["c_in"], count), _tile(R["r_obf"], count)), want, R["rows"], what + " obfuscate")
    _same(ctx.powmod(_tile(R["base"], count), _tile(R["k"], count)), want, R["rows"], what + " powmod")
    _same(ctx.mulmod(_tile(R["a"], count), _tile(R["b"], count)), want, R["rows"], what + " mulmod")
    if decrypt and ctx.has_private:
        _same(ctx.decrypt(want), m, R["rows"], what + " decrypt")


def test_the_layouts_cover_the_ladder(native, rows):
    g = rows["g"]
    ctx = _ctx(native, g)
    pub, _ = ctx.ladder()
    lays = layouts_of(rows["key"].n, pub)
    for code in pub:
        assert any(half and L == code % 100 for _, L, half in lays), (code, lays)
    assert any(half is None for _, _, half in lays)
    ctx.close()


def test_every_rung_returns_the_chosen_rows(native, rows, c_oracle):
    """PHE_HIP_GROUP rungs and auto, at a whole number of waves + 11"""
    ctx = _ctx(native, rows["g"])
    pub, priv = ctx.ladder()
    count = 64 * (-(-len(rows["rows"]) // 64)) + 11
    for width in [0] + sorted({c // 100 for c in pub + priv}):
        ctx.set_group(width)
        _hot_path(native, ctx, rows, c_oracle, count, "group %d" % width, oracle=(width == 0))
    ctx.set_group(0)
    ctx.close()


def test_the_item_loop_wraps_on_the_chosen_rows(native, rows, c_oracle):
    """one batch beyond the rows in flight: every group runs more than one item"""
    ctx = _ctx(native, rows["g"])
    count = int(ctx.info()["rows_in_flight"]) + 64 * 3 + 11
    _hot_path(native, ctx, rows, c_oracle, count, "%d rows" % count)
    ctx.close()


@pytest.mark.parametrize("env", ["PHE_HIP_ENGINE=full", "PHE_HIP_FORCE_UNIT=1", "PHE_HIP_NO_UNIT=1", "PHE_HIP_NO_LATE=1",
                                 "PHE_HIP_NO_WAVE_PAIRS=1"])
def test_settings_return_the_chosen_rows(native, rows, c_oracle, env, monkeypatch):
    name, value = env.split("=")
    monkeypatch.setenv(name, value)
    ctx = _ctx(native, rows["g"])
    count = 64 * (-(-len(rows["rows"]) // 64)) + 11
    _hot_path(native, ctx, rows, c_oracle, count, env, oracle=False)
    for small in (3, 40):                                    # the small-batch rungs under this setting
        for start in range(0, len(rows["rows"]) - small, max(1, len(rows["rows"]) // 6)):
            part = dict(rows, **{k: rows[k][start:start + small] for k in ("want", "m", "r", "c_in", "r_obf", "base", "k", "a", "b")})
            part["rows"] = rows["rows"][start:start + small]
            _hot_path(native, ctx, part, c_oracle, small, "%s, %d rows from %d" % (env, small, start), oracle=False)
    if name == "PHE_HIP_NO_WAVE_PAIRS":                      # the rungs of 16 lanes and the whole wave on their late single-wave sweeps
        for width in (16, 64):
            ctx.set_group(width)
            _hot_path(native, ctx, rows, c_oracle, count, "%s group %d" % (env, width), oracle=False)
            ctx.encrypt(rows["m"][:40], rows["r"][:40])
            assert ctx.last_launch()["path"] & ctx.PATH_LATE, width
        ctx.set_group(0)
    ctx.close()


def test_small_batches_run_wave_pairs_and_the_wave_tail_on_the_chosen_rows(native, rows, c_oracle):
    """a handful of rows (wave pairs) up to a few hundred (the small-batch rungs), taken from every part of the batch; the paths
    that ran are read back from the context"""
    ctx = _ctx(native, rows["g"])
    seen = 0
    n_rows = len(rows["rows"])
    for small in (1, 2, 7, 60, 111, 700):
        for start in range(0, n_rows - small, max(1, n_rows // 12)):
            sl = slice(start, start + small)
            got = ctx.encrypt(rows["m"][sl], rows["r"][sl])
            seen |= ctx.last_launch()["path"]
            _same(got, rows["want"][sl], rows["rows"][sl], "encrypt of %d rows from %d" % (small, start))
            _same(ctx.decrypt(rows["want"][sl]), rows["m"][sl], rows["rows"][sl], "decrypt of %d rows from %d" % (small, start))
            seen |= ctx.last_launch()["path"]
            _same(ctx.powmod(rows["base"][sl], rows["k"][sl]), rows["want"][sl], rows["rows"][sl], "powmod of %d rows from %d" % (small, start))
    assert seen & ctx.PATH_WAVE_PAIRS and seen & ctx.PATH_WAVE_TAIL, seen
    ctx.close()


def test_both_decrypt_tails_agree_on_the_chosen_rows(native, rows, monkeypatch):
    ctx = _ctx(native, rows["g"])
    sl = slice(0, 200)
    with_tail = ctx.decrypt(rows["want"][sl])
    assert ctx.last_launch()["path"] & ctx.PATH_WAVE_TAIL
    ctx.close()
    monkeypatch.setenv("PHE_HIP_NO_WAVE_TAIL", "1")
    ctx = _ctx(native, rows["g"])
    without = ctx.decrypt(rows["want"][sl])
    assert not ctx.last_launch()["path"] & ctx.PATH_WAVE_TAIL
    ctx.close()
    _same(with_tail, rows["m"][sl], rows["rows"][sl], "wave tail")
    _same(without, rows["m"][sl], rows["rows"][sl], "per-thread tail")


def test_encrypted_vector_operators_return_the_chosen_rows(native, rows):
    """`+` between two vectors (host rows, resident rows, resident rows in the pair form) and `*` by integer scalars, on operands
    whose product / power is the chosen row"""
    from phe import paillier
    pub = paillier.PaillierPublicKey(rows["key"].n)
    count = len(rows["rows"])
    want = [t for t, _ in rows["rows"]]
    zeros = np.zeros(count, dtype=np.int64)
    a = paillier.EncryptedVector(pub, rows["a"].copy(), zeros, obfuscated=True)
    b = paillier.EncryptedVector(pub, rows["b"].copy(), zeros, obfuscated=True)
    for what, x, y in (("host", a, b), ("resident", a.to_device(), b.to_device()), ("pair form", a.to_pair(), b.to_device())):
        got = (x + y).ciphertexts(be_secure=False)
        bad = la.first_mismatch(got, want, [tag for _, tag in rows["rows"]])
        assert bad is None, "EncryptedVector + (%s): %s" % (what, bad)
    short = [i for i in range(count) if i % 4 < 2]           # the rows whose exponent is 3 or a 17-bit integer (see the fixture)
    ks = [int(v) for v in native.limbs_to_ints(rows["k"][short])]
    base = paillier.EncryptedVector(pub, rows["base"][short].copy(), zeros[:len(short)], obfuscated=True)
    for what, x in (("host", base), ("resident", base.to_device())):
        got = (x * ks).ciphertexts(be_secure=False)
        bad = la.first_mismatch(got, [want[i] for i in short], [rows["rows"][i][1] for i in short])
        assert bad is None, "EncryptedVector * (%s): %s" % (what, bad)


def _tail_contexts(native, g_or_key, monkeypatch):
    """(context with the wave tail, context with the per-thread tail)"""
    make = (lambda: _ctx(native, g_or_key)) if isinstance(g_or_key, dict) else g_or_key
    with_tail = make()
    monkeypatch.setenv("PHE_HIP_NO_WAVE_TAIL", "1")
    without = make()
    monkeypatch.delenv("PHE_HIP_NO_WAVE_TAIL")
    return with_tail, without


def test_both_decrypt_tails_return_the_chosen_plaintexts(native, rows, c_oracle, monkeypatch):
    """the plaintexts chosen through the intermediates of the CRT tail (lookahead.decrypt_rows: m_p and u laid out against p and q,
    x_p = 0 mod W^k, u = 0, u = q - 1, m_q = m_p, m_q < m_p) through both tails on every rung of the CRT halves, a handful and a
    batch of whole waves + 11"""
    key, g = rows["key"], rows["g"]
    rng = random.Random(9100)
    drows = la.decrypt_rows(key, rng, 64)
    s1 = KEY_BITS // 32
    c = native.ints_to_limbs([key.ciphertext_of(m, rng) for m, _ in drows], 2 * s1)
    want = native.ints_to_limbs([m for m, _ in drows], s1)
    n_arr = native.int_to_limbs(key.n, s1)
    p_arr, q_arr = native.int_to_limbs(key.p, s1 // 2), native.int_to_limbs(key.q, s1 // 2)
    _same(c_oracle.decrypt(n_arr, p_arr, q_arr, c, nthreads=8), want, drows, "libgmp")
    with_tail, without = _tail_contexts(native, g, monkeypatch)
    _, priv = with_tail.ladder()
    count = 64 * (-(-len(drows) // 64)) + 11
    for width in [0] + sorted({code // 100 for code in priv}):
        for ctx, name in ((with_tail, "wave tail"), (without, "per-thread tail")):
            ctx.set_group(width)
            _same(ctx.decrypt(_tile(c, count)), _tile(want, count), drows, "%s group %d" % (name, width))
            for start in range(0, len(drows) - 5, 7):
                _same(ctx.decrypt(c[start:start + 5]), want[start:start + 5], drows[start:], "%s group %d, 5 rows from %d" % (name, width, start))
            assert bool(ctx.last_launch()["path"] & ctx.PATH_WAVE_TAIL) == (ctx is with_tail)
    with_tail.close()
    without.close()


def test_multiexp_returns_the_chosen_products(native, rows):
    """phe_hip_multiexp: the product of three powers is the chosen row, the last base solved for; one call per target, on every
    rung; then all of them in ONE call whose product is the product of the targets"""
    key = rows["key"]
    M = key.nsq
    rng = random.Random(9200)
    s2 = KEY_BITS // 16
    picked = rows["rows"][::max(1, len(rows["rows"]) // 160)]
    calls = []
    for t, tag in picked:
        b0, b1 = la.random_unit(M, rng), la.random_unit(M, rng)
        e0, e1, e2 = rng.getrandbits(56), rng.getrandbits(64) | 1, key.coprime_exponent(rng.getrandbits(64) | 1)
        rest = pow(b0, e0, M) * pow(b1, e1, M) % M
        b2 = key.preimage_powmod(t * pow(rest, -1, M) % M, e2)
        calls.append((native.ints_to_limbs([b0, b1, b2], s2), native.ints_to_limbs([e0, e1, e2], 2), t, tag))
    ctx = _ctx(native, rows["g"], private=False)
    pub, _ = ctx.ladder()
    for width in [0] + sorted({code // 100 for code in pub}):
        ctx.set_group(width)
        for base, exps, t, tag in calls:
            got = native.limbs_to_ints(ctx.multiexp(base, exps))[0]
            assert got == t, "multiexp group %d: %s" % (width, tag)
    ctx.set_group(0)
    total = 1
    for _, _, t, _ in calls:
        total = total * t % M
    got = ctx.multiexp(np.concatenate([c[0] for c in calls]), np.concatenate([c[1] for c in calls]))
    assert native.limbs_to_ints(got)[0] == total
    ctx.close()


def test_owner_encrypt_returns_the_chosen_rows(native, rows):
    """raw_encrypt by the key owner (CRT halves, crt_lift_body, the product with 1 + n m) on every rung, whole waves + 11 and a
    handful: the chosen ciphertexts"""
    ctx = _ctx(native, rows["g"])
    assert ctx.owner_encrypt_offered()
    _, priv = ctx.ladder()
    count = 64 * (-(-len(rows["rows"]) // 64)) + 11
    seen = 0
    for width in [0] + sorted({code // 100 for code in priv}):
        ctx.set_group(width)
        _same(ctx.encrypt_owner(_tile(rows["m"], count), _tile(rows["r"], count)), _tile(rows["want"], count), rows["rows"], "owner encrypt group %d" % width)
        seen |= ctx.last_launch()["path"]
        for start in range(0, len(rows["rows"]) - 5, max(1, len(rows["rows"]) // 24)):
            sl = slice(start, start + 5)
            _same(ctx.encrypt_owner(rows["m"][sl], rows["r"][sl]), rows["want"][sl], rows["rows"][sl], "owner encrypt group %d, 5 rows from %d" % (width, start))
    assert seen & ctx.PATH_OWNER
    ctx.set_group(0)
    ctx.close()


def test_a_key_off_the_limb_grid_returns_the_chosen_rows(native, c_oracle, monkeypatch):
    """a 968-bit key (seeded primes): n, p and q fill neither their rows of words nor their rungs — padding lanes at the top of every
    group.  encrypt returns the chosen t (laid out on this key's own ladder) on every rung, both tails the chosen m"""
    bits = 968
    key, hp, hq = la.off_grid_key(bits)
    s1 = 2 * ((bits + 63) // 64)
    make = lambda: native.Context(key.n, key.p, key.q, hp, hq, pow(key.p, -1, key.q), n_limbs=s1)
    ctx, plain_tail = _tail_contexts(native, make, monkeypatch)
    pub, priv = ctx.ladder()
    rng = random.Random(9300)
    M = key.nsq
    batch = []
    for nl, L, half in layouts_of(key.n, pub):
        arrives = lambda t: la.borrow_arrives(t, M, nl, L)
        for f in la.FAMILIES:
            ts = la.thin_cells(la.unit_targets(la.family_targets(M, nl, L, rng, f, half), key.n), arrives)
            batch += [(t, "%dx%d %s" % (nl, L, tag)) for t, tag in ts[::2]]
    pre = [key.preimage_encrypt(t, check=i % 97 == 0) for i, (t, _) in enumerate(batch)]
    want = native.ints_to_limbs([t for t, _ in batch], 2 * s1)
    m, r = native.ints_to_limbs([x for x, _ in pre], s1), native.ints_to_limbs([y for _, y in pre], s1)
    drows = la.decrypt_rows(key, rng, 24)
    dc = native.ints_to_limbs([key.ciphertext_of(x, rng) for x, _ in drows], 2 * s1)
    dwant = native.ints_to_limbs([x for x, _ in drows], s1)
    count = 64 * (-(-len(batch) // 64)) + 11
    _same(c_oracle.encrypt(native.int_to_limbs(key.n, s1), m, r, nthreads=16), want, batch, "libgmp")
    for width in [0] + sorted({code // 100 for code in pub + priv}):
        for c in (ctx, plain_tail):
            c.set_group(width)
            _same(c.encrypt(_tile(m, count), _tile(r, count)), _tile(want, count), batch, "encrypt group %d" % width)
            _same(c.encrypt(m[:7], r[:7]), want[:7], batch, "encrypt group %d, 7 rows" % width)
            _same(c.decrypt(_tile(want, count)), _tile(m, count), batch, "decrypt group %d" % width)
            _same(c.decrypt(dc), dwant, drows, "decrypt of the chosen plaintexts, group %d" % width)
    ctx.close()
    plain_tail.close()
