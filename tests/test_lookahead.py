"""The carry / borrow look-ahead between the lanes of a limb group, function by function and kernel by kernel (CPU wave emulator).

Every kernel but the tile product leaves its lazily reduced form through group_carry_in, normalize_full, cond_sub, canonicalize
(csrc/mont_core.h) and cond_sub_pair (csrc/split_core.h).  Their propagate term only matters when a whole lane is all ones or
equal to the modulus's lane, which random rows never are; tests/lookahead.py builds such lanes on purpose.  The references are
Python integers and a lane-by-lane ripple; nothing here is taken from the code under test but its output.

COVERAGE MAP.  Counted with a throw-away counter inside the callers of group_carry_in (a scratch copy, not committed), per function
and (G, L), first over the CPU suite as it was (its 282 tests less the four of test_profiles_fresh.py, which pin the sources'
hash), then with this module added.  The second count is ONE snapshot, taken when the module held the function-level tests and the
encrypt / obfuscate / powmod / product / decrypt / Miller-Rabin rows; the multiexp, owner-encrypt, off-grid and table-product
tests came later and were not counted (they can only add hits).  A letter means that the
event happened at least once:
    M  a lane that propagates AND receives a carry, below the group's top lane          t  the same in the top lane
    T  ... in the top lane while the next group of the wave generates                   Z  lane 0 propagates beside a neighbour's carry-out
    p  the same on all-zero padding lanes above the modulus (cond_sub, cond_sub_pair; normalize_full knows no modulus: M / t)
    S  canonicalize's second subtraction taken      H  the low half's borrow handed to the high half through a propagating top lane
    K  cond_sub_pair's `take`
    (geometry, the old suite > with this module; letters in the order M t T Z p S H K)
    cond_sub
        1x18  -------- > -----S--    2x9   ---Z---- > -tTZpS--    2x18  -tTZ---- > -tTZpS--    2x27  -tTZ---- > -tTZ-S--
        2x36  -tTZ---- > -tTZ-S--    4x5   -------- > MtTZpS--    4x9   -------- > MtTZpS--    4x14  not run  > MtTZ-S--
        4x18  MtTZ---- > MtTZ-S--    4x27  MtTZ---- > MtTZ-S--    4x36  MtTZp--- > MtTZpS--    8x3   --TZp--- > MtTZpS--
        8x5   MtTZp--- > MtTZpS--    8x7   -------- > MtTZ-S--    8x9   MtTZ---- > MtTZ-S--    8x14  -------- > MtTZ-S--
        8x18  MtT-p--- > MtTZpS--    8x27  MtT----- > MtTZ-S--    16x1  M-TZp--- > MtTZpS--    16x2  M-TZp--- > MtTZpS--
        16x3  M-TZp--- > MtTZpS--    16x4  --TZp--- > MtTZpS--    16x5  M-TZpS-- > MtTZpS--    16x7  MtT----- > MtTZ-S--
        16x9  MtTZpS-- > MtTZpS--    16x14 MtT----- > MtTZ-S--    16x18 ---Z---- > MtTZ-S--    64x1  M---p--- > Mt--pS--
        64x2  M---p--- > Mt--pS--    64x3  ----p--- > Mt--pS--    64x5  not run  > Mt---S--
    cond_sub_pair(high)
        1x18  -------K > -------K    2x9   ---Z---- > -tTZp--K    2x18  -tTZ---K > -tTZ---K    2x27  -tTZ---K > -tTZ---K
        4x5   -------- > MtTZp--K    4x9   -------- > MtTZ---K    4x14  not run  > MtTZ---K    4x18  MtTZ---K > MtTZ---K
        4x27  ---Z---- > MtTZ---K    8x3   --T-p--- > MtTZp--K    8x5   M-TZp--K > MtTZp--K    8x7   -------- > MtTZ---K
        8x9   ---Z---- > MtTZ---K    8x14  -------- > MtTZ---K    8x18  not run  > MtTZ---K    16x1  M-T-p--- > MtTZp--K
        16x2  --T-p--- > MtTZp--K    16x3  M-TZp--- > MtTZp--K    16x4  --T-p--- > MtTZp--K    16x5  M-T-p--- > MtTZp--K
        16x7  M-T-p--- > MtTZp--K    16x9  not run  > MtTZ---K    16x14 not run  > MtTZ---K    16x18 -------- > MtTZ---K
        64x1  M---p--K > Mt--p--K    64x2  M---p--K > Mt--p--K    64x3  ----p--- > Mt--p--K    64x5  not run  > Mt-----K
    cond_sub_pair(low)
        1x18  -------- > --------    2x9   ---Z---- > -tTZp-H-    2x18  -tTZ--H- > -tTZ--H-    2x27  -tTZ--H- > -tTZ--H-
        4x5   -------- > MtTZp-H-    4x9   -------- > MtTZ--H-    4x14  not run  > MtTZ--H-    4x18  MtTZp-H- > MtTZp-H-
        4x27  ---Zp--- > MtTZp-H-    8x3   --T-p-H- > MtTZp-H-    8x5   MtTZ--H- > MtTZ--H-    8x7   -------- > MtTZ--H-
        8x9   ---Zp--- > MtTZp-H-    8x14  -------- > MtTZ--H-    8x18  not run  > MtTZ--H-    16x1  MtTZp-H- > MtTZp-H-
        16x2  --T-p-H- > MtTZp-H-    16x3  M-TZp-H- > MtTZp-H-    16x4  --T-p-H- > MtTZp-H-    16x5  --T-p-H- > MtTZp-H-
        16x7  -------- > MtTZ--H-    16x9  not run  > MtTZ--H-    16x14 not run  > MtTZ--H-    16x18 -------- > MtTZ--H-
        64x1  M---p-H- > Mt--p-H-    64x2  M---p-H- > Mt--p-H-    64x3  ----p-H- > Mt--p-H-    64x5  not run  > Mt----H-
    normalize_full
        1x18  -------- > --------    2x9   -------- > -tTZ----    2x18  -------- > -tTZ----    2x27  -------- > -tTZ----
        2x36  -------- > -tTZ----    4x5   -------- > MtTZ----    4x9   -------- > MtTZ----    4x14  not run  > MtTZ----
        4x18  M------- > MtTZ----    4x27  M------- > MtTZ----    4x36  M------- > MtTZ----    8x3   -------- > MtTZ----
        8x5   -------- > MtTZ----    8x7   -------- > MtTZ----    8x9   M------- > MtTZ----    8x14  -------- > MtTZ----
        8x18  M------- > MtTZ----    8x27  -------- > MtTZ----    16x1  M------- > MtTZ----    16x2  -------- > MtTZ----
        16x3  -------- > MtTZ----    16x4  -------- > MtTZ----    16x5  MtT----- > MtTZ----    16x7  -------- > MtTZ----
        16x9  M------- > MtTZ----    16x14 -------- > MtTZ----    16x18 -------- > MtTZ----    64x1  -------- > Mt------
        64x2  -------- > Mt------    64x3  -------- > Mt------    64x5  not run  > Mt------
("not run": no test instantiated the function on that geometry.  One lane (1x18) has nothing to propagate to, two lanes have no
middle lane, the whole wave (64xL) has no neighbour, p needs a modulus that leaves lanes of its group empty: every other cell is filled.  cond_sub counts its calls alone and inside
canonicalize; cond_sub_pair exists for the split-modulus geometries only.)

MUTANTS.  Built for the emulator only, on a scratch copy, never committed; each line names the tests of this module that fail
(function level / kernel level).
    pm without ~top                      group_carry_in (both), normalize_full, cond_sub, canonicalize, cond_sub_pair / encrypt,
                                         obfuscate, powmod, products, Miller-Rabin
    gs without ~lane0                    group_carry_in (both), normalize_full, cond_sub, canonicalize, cond_sub_pair / encrypt and
                                         obfuscate at 1024 bits (keys that fill their rung: at 256 bits the top lanes are padding)
    prop & cin -> prop                   group_carry_in (both), cond_sub, canonicalize, cond_sub_pair / encrypt, obfuscate, powmod,
                                         products, both decrypt tails, Miller-Rabin
    normalize_full without second pass   normalize_full, canonicalize / encrypt, obfuscate, powmod, products, decrypt, Miller-Rabin
    canonicalize with one subtraction    canonicalize / the table product (csrc/mul_table.h, 16 x 5 and 16 x 9: the one kernel
                                         whose canonicalize receives a value up to 3N — where the old suite's S came from; the
                                         other kernels canonicalize a Montgomery product's value, below 2N)
    cond_sub_pair without low borrow     cond_sub_pair / encrypt, obfuscate, powmod, decrypt (multiexp, off-grid keys: same exit)
    take inverted                        cond_sub_pair / encrypt, obfuscate, powmod, decrypt
    the wave tail's + q dropped          (not a lane function) / decrypt on the wave tail, every rung
"""
import math
import os
import random
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import lookahead as la  # noqa: E402
from emu_lib import Emu  # noqa: E402

MASK = la.MASK

# every (G, L) a kernel is compiled for (csrc/kernels_g*.hip: full width, kernels_s*.hip: split modulus)
FULL_GL = [(16, L) for L in (1, 2, 3, 5, 7, 9, 14, 18)] + [(8, L) for L in (5, 9, 14, 18, 27)] + \
          [(4, L) for L in (9, 18, 27, 36)] + [(2, 18), (2, 36)]
SPLIT_GL = [(64, L) for L in (1, 2, 3, 5)] + [(16, L) for L in (1, 2, 3, 4, 5, 7, 9, 14, 18)] + \
           [(8, L) for L in (3, 5, 7, 9, 14, 18)] + [(4, L) for L in (5, 9, 14, 18, 27)] + [(2, L) for L in (9, 18, 27)] + [(1, 18)]
ALL_GL = sorted(set(FULL_GL) | set(SPLIT_GL))


@pytest.fixture(scope="module")
def emu():
    return Emu()


# ---- group_carry_in -----------------------------------------------------------------------------------------------------------
def _check_carry(emu, G, gens, props):
    cin, out = emu.group_carry_in(G, gens, props)
    lane0 = sum(1 << b for b in range(0, 64, G))
    top = lane0 << (G - 1)
    for g, p, c, o in zip(gens, props, cin.tolist(), out.tolist()):
        want_c, want_o = la.ripple(G, g, p)
        assert c == want_c, "G=%d gen=%016x prop=%016x: cin %016x, ripple %016x" % (G, g, p, c, want_c)
        assert o == want_o, "G=%d gen=%016x prop=%016x: out_top %016x, ripple %016x" % (G, g, p, o, want_o)
        assert c & lane0 == 0 and o & ~top == 0            # nothing enters a lane 0, nothing but top lanes reports a carry out


def _masks_of(kinds, shift):
    gen = sum(1 << (shift + i) for i, k in enumerate(kinds) if k == "G")
    prop = sum(1 << (shift + i) for i, k in enumerate(kinds) if k == "P")
    return gen, prop


def _random_disjoint(rng, density):
    gen = prop = 0
    for b in range(64):
        x = rng.random()
        if x < density:
            prop |= 1 << b
        elif x < density + (1 - density) / 2:
            gen |= 1 << b
    return gen, prop


@pytest.mark.parametrize("G", [1, 2, 4, 8])
def test_group_carry_in_every_assignment_in_every_group_position(emu, G):
    """all 3^G disjoint generate / propagate assignments of one group, alone in the wave, in every group position with random
    neighbours, and with the worst neighbours: every other lane of the wave generating, every other lane propagating"""
    import itertools
    rng = random.Random(7100 + G)
    gens, props = [], []
    all_lanes = (1 << 64) - 1
    for kinds in itertools.product("PGK", repeat=G):
        for pos in range(64 // G):
            g1, p1 = _masks_of(kinds, pos * G)
            field = ((1 << G) - 1) << (pos * G)
            rg, rp = _random_disjoint(rng, rng.choice((0.2, 0.5, 0.8)))
            for og, op in ((0, 0), (rg, rp), (all_lanes, 0), (0, all_lanes)):
                gens.append(g1 | (og & ~field))
                props.append(p1 | (op & ~field))
    _check_carry(emu, G, gens, props)


@pytest.mark.parametrize("G", [16, 64])
def test_group_carry_in_runs_and_random_masks_on_wide_groups(emu, G):
    rng = random.Random(7200 + G)
    gens, props = [], []
    all_lanes = (1 << 64) - 1
    for kinds in la.patterns(G, rng, random_count=400):
        for pos in range(64 // G):
            g1, p1 = _masks_of(kinds, pos * G)
            field = ((1 << G) - 1) << (pos * G)
            rg, rp = _random_disjoint(rng, rng.choice((0.2, 0.5, 0.9)))
            for og, op in ((rg, rp), (all_lanes, 0), (0, all_lanes)):
                gens.append(g1 | (og & ~field))
                props.append(p1 | (op & ~field))
    for density in (0.05, 0.3, 0.6, 0.9, 0.98):
        for _ in range(2000):
            g1, p1 = _random_disjoint(rng, density)
            gens.append(g1)
            props.append(p1)
    _check_carry(emu, G, gens, props)


def test_the_ripple_reference_on_hand_made_cases():
    """the reference itself: a carry walks through propagate lanes, stops at the group's top, and is reported there"""
    assert la.ripple(4, 0b0001, 0b0110) == (0b1110, 0)                       # generated in lane 0, dies in lane 3 (kill)
    assert la.ripple(4, 0b0001, 0b1110) == (0b1110, 0b1000)                  # ... runs out of the top
    assert la.ripple(4, 0b0000_1000, 0b1111_0000) == (0, 0b1000)             # a top lane's carry does not enter the next group
    assert la.ripple(4, 0b0000_0001, 0b1111_1110) == (0b1110, 0b1000)        # a run through the top does not either
    assert la.ripple(1, 0b01, 0b10) == (0, 0b01)
    assert la.receives("GPPKP") == [1, 2] and la.carry_out("KGP") == 1 and la.carry_out("GPK") == 0


# ---- the lane-level functions -------------------------------------------------------------------------------------------------
def _cases_to_waves(emu, G, L, op, cases, rng, pair=False):
    """cases: (t_limbs, u_limbs or None, check(out_limbs)) per NUMBER; packed into waves in three orders, run, every group checked
    on its own.  Returns the number of groups checked."""
    per = 64 // G
    rows = la.pack_waves(cases, per, rng)
    shape = (len(rows), 2, per, G * L) if pair else (len(rows), per, G * L)
    t = np.zeros(shape, np.uint32)
    has_u = cases[0][1] is not None
    u = np.zeros(shape, np.uint32) if has_u else None
    for w, row in enumerate(rows):
        for r, (tl, ul, _) in enumerate(row):
            if pair:
                t[w, 0, r], t[w, 1, r] = tl[:G * L], tl[G * L:]
                u[w, 0, r], u[w, 1, r] = ul[:G * L], ul[G * L:]
            else:
                t[w, r] = tl
                if has_u:
                    u[w, r] = ul
    out = emu.lane_op(G, L, op, t, u)
    for w, row in enumerate(rows):
        for r, (_, _, check) in enumerate(row):
            got = out[w, :, r].reshape(-1).tolist() if pair else out[w, r].tolist()
            check(got, "%s G=%d L=%d wave %d group %d" % (op, G, L, w, r))
    return len(rows) * per


def _all_patterns(G, rng, n=None):
    n = n or G
    pats = la.patterns(n, rng)
    if n == G:
        pats += la.neighbour_wave(G, rng) * 2                # (consecutive in the first packing order: see pack_waves)
    return pats


def _assert_cells(pats, n, what):
    """the positions the propagate term must be exercised at, by construction: a middle lane, a run into the top lane that carries
    out, a run from lane 0 — each with a carry arriving where one can"""
    if n == 1:
        return
    hits = [(p, la.receives(p)) for p in pats]
    assert any(h and 0 < min(h) and max(h) < n - 1 for _, h in hits) or n == 2, what + ": no middle lane"
    assert any(n - 1 in h and la.carry_out(p) for p, h in hits), what + ": no run through the top lane"
    assert any(p[0] == "P" for p in pats), what + ": no run from lane 0"
    assert any(p[-1] == "P" and n - 1 not in la.receives(p) for p in pats), what + ": no idle propagate top lane"


@pytest.mark.parametrize("G,L", ALL_GL)
def test_normalize_full_lanes_of_ones(emu, G, L):
    """almost-normalised limbs in, canonical digits of the same value out (modulo R = 2^(29 G L): a carry out of the top lane is
    dropped, as on the device, and must not reach the next group)"""
    rng = random.Random(7300 + 100 * G + L)
    pats = _all_patterns(G, rng)
    _assert_cells(pats, G, "normalize_full")
    R = 1 << (29 * G * L)
    cases = []
    for kinds in pats:
        limbs = la.lanes_of_ones(kinds, L, rng)
        assert max(limbs) < (1 << 29) + la.SLOP
        want = la.digits(la.value(limbs) % R, G * L)

        def check(got, where, want=want, kinds=kinds):
            assert got == want, "%s lanes %s" % (where, kinds)
        cases.append((limbs, None, check))
    _cases_to_waves(emu, G, L, "normalize_full", cases, rng)


@pytest.mark.parametrize("G,L", ALL_GL)
def test_add_normalize_keeps_the_value_and_the_limb_bound(emu, G, L):
    """t + u for two almost-normalised numbers whose sum stays below R: the value is kept, every limb comes back below 2^29 + 2^8,
    and a lane's carry goes to the lane above of the SAME group only"""
    rng = random.Random(7400 + 100 * G + L)
    S = G * L
    cases = []
    for i in range(3 * (64 // G) + 8):
        style = i % 4
        if style == 0:                                       # the largest almost-normalised limbs everywhere but the top lane's top
            a = [(1 << 29) + la.SLOP - 1] * S
            b = [(1 << 29) + la.SLOP - 1] * S
        elif style == 1:
            a = [MASK] * S
            b = [1] + [0] * (S - 1)
        else:
            a = la.sloppy(la.digits(rng.getrandbits(29 * S), S), rng)
            b = la.sloppy(la.digits(rng.getrandbits(29 * S), S), rng)
        if style == 1:
            a[S - 1] = MASK - 1                              # (room in the top limb: the sum stays below R)
        else:
            a[S - 1], b[S - 1] = rng.randrange(1 << 27), rng.randrange(1 << 27)
        total = la.value(a) + la.value(b)
        assert total < (1 << (29 * S))

        def check(got, where, total=total):
            assert la.value(got) == total, where
            assert max(got) < (1 << 29) + la.SLOP, where
        cases.append((a, b, check))
    _cases_to_waves(emu, G, L, "add_normalize", cases, rng)


def _cond_sub_cases(G, L, rng, pats):
    cases = []
    for kinds in pats:
        ref = la.reference_lanes(G, L, rng)
        t = la.join_lanes(la.lanes_against(kinds, ref, L, rng), L)
        n = la.join_lanes(ref, L)
        want = la.digits(t - n if t >= n else t, G * L)
        assert (la.carry_out(kinds) == 1) == (t < n)         # the kinds say which branch this is

        def check(got, where, want=want, kinds=kinds):
            assert got == want, "%s lanes %s" % (where, kinds)
        cases.append((la.digits(t, G * L), la.digits(n, G * L), check))
    return cases


@pytest.mark.parametrize("G,L", ALL_GL)
def test_cond_sub_lanes_equal_to_the_modulus(emu, G, L):
    """canonical t, any n: t - n where t >= n, t otherwise; every group has a modulus of its own"""
    rng = random.Random(7500 + 100 * G + L)
    pats = _all_patterns(G, rng)
    _assert_cells(pats, G, "cond_sub")
    assert any(la.carry_out(p) for p in pats) and any(not la.carry_out(p) for p in pats)
    _cases_to_waves(emu, G, L, "cond_sub", _cond_sub_cases(G, L, rng, pats), rng)


@pytest.mark.parametrize("G,L", ALL_GL)
def test_canonicalize_zero_one_and_two_subtractions(emu, G, L):
    """almost-normalised v in [0, 3N) -> v mod N.  v = w + k N with the lanes of w laid out against N's, so that the look-ahead of
    the FIRST subtraction (k = 0), of the SECOND (k = 1) and of both (k = 2, w < N) meets lanes that propagate"""
    rng = random.Random(7600 + 100 * G + L)
    pats = _all_patterns(G, rng)
    _assert_cells(pats, G, "canonicalize")
    cases, subs = [], set()
    for i, kinds in enumerate(pats):
        ref = la.reference_lanes(G, L, rng, top_room_bits=4)  # R >= 16 N, as key_setup.h picks geometries
        n = la.join_lanes(ref, L)
        w = la.join_lanes(la.lanes_against(kinds, ref, L, rng, top_cap=2 * ref[-1] - 1), L)
        assert w < 2 * n
        for k in ((0, 1) if w >= n else (0, 1, 2)):
            v = w + k * n
            subs.add(v // n)
            limbs = la.sloppy(la.digits(v, G * L), rng) if (i + k) % 2 else la.digits(v, G * L)
            want = la.digits(v % n, G * L)

            def check(got, where, want=want, kinds=kinds, k=k):
                assert got == want, "%s lanes %s + %d N" % (where, kinds, k)
            cases.append((limbs, la.digits(n, G * L), check))
    assert subs == {0, 1, 2}
    _cases_to_waves(emu, G, L, "canonicalize", cases, rng)


@pytest.mark.parametrize("G,L", SPLIT_GL)
def test_cond_sub_pair_hands_the_borrow_from_the_low_half_to_the_high_half(emu, G, L):
    """canonical (lo, hi) of 2 G lanes minus (mlo, mhi) where that is not negative.  The kinds run over the 2 G lanes of the whole
    number; on top of the common patterns: a low half that propagates completely (a borrow from lane 0 reaches lane 0 of the high
    half through out_lo), with the high half's lane 0 equal, smaller, larger, and larger by exactly the borrow"""
    rng = random.Random(7700 + 100 * G + L)
    n2 = 2 * G
    pats = la.patterns(n2, rng, exhaustive_upto=4, random_count=16)
    for lo0 in "GK":                                         # the hand-over, with and without a borrow to hand over
        lo = lo0 + "P" * (G - 1) if G > 1 else lo0
        for hi0 in "PGK":
            for rest in ("K", "G", "P"):
                pats.append(lo + hi0 + (rest * (G - 1)))
    if G > 1:
        pats += ["P" * G + "G" + "K" * (G - 1), "P" * n2, "G" + "P" * (n2 - 1), "K" + "P" * (n2 - 1)]
    _assert_cells(pats, n2, "cond_sub_pair")
    assert any(p[:G] == ("G" + "P" * (G - 1)) and p[G] == "P" for p in pats)
    H = G * L
    cases, taken = [], set()
    for i, kinds in enumerate(pats):
        ref = la.reference_lanes(n2, L, rng)
        tl = la.lanes_against(kinds, ref, L, rng)
        if i % 5 == 0 and ref[G] < la._lane_max(L) and la.carry_out(kinds[:G]):
            tl[G] = ref[G] + 1                               # the high half's lane 0 becomes ZERO once the borrow has arrived
        t, m = la.join_lanes(tl, L), la.join_lanes(ref, L)
        want = la.digits(t - m if t >= m else t, 2 * H)
        taken.add(t >= m)

        def check(got, where, want=want, kinds=kinds):
            assert got == want, "%s lanes %s" % (where, kinds)
        cases.append((la.digits(t, 2 * H), la.digits(m, 2 * H), check))
    assert taken == {True, False}
    _cases_to_waves(emu, G, L, "cond_sub_pair", cases, rng, pair=True)


# ---- the kernels, result first ------------------------------------------------------------------------------------------------
from conftest import load_golden  # noqa: E402
from oracle.paillier_oracle import int_to_limbs, ints_to_limbs, limbs_to_ints  # noqa: E402

# (name, split engine, group, scaled modulus, late sweeps, wave pairs): every rung of emu_encrypt / emu_powmod_n2
RUNGS = [("split-auto", True, 0, False, False, False), ("split-g2", True, 2, False, False, False),
         ("split-g4", True, 4, False, False, False), ("split-g8", True, 8, False, False, False),
         ("split-g16", True, 16, False, False, False), ("split-g64", True, 64, False, False, False),
         ("split-unit", True, 0, True, False, False), ("split-g16-late", True, 16, False, True, False),
         ("split-g64-late", True, 64, False, True, False), ("split-g64-pairs", True, 64, False, False, True),
         ("full-auto", False, 0, False, False, False), ("full-g2", False, 2, False, False, False),
         ("full-g4", False, 4, False, False, False), ("full-g8", False, 8, False, False, False),
         ("full-g16", False, 16, False, False, False)]
RUNG = {r[0]: r for r in RUNGS}
class _Rung:
    def __init__(self, emu, name):
        self.emu, self.cfg = emu, RUNG[name]

    def __enter__(self):
        _, split, group, unit, late, pairs = self.cfg
        e = self.emu
        e.set_engine(split), e.set_group(group), e.set_unit(unit), e.set_late(late), e.set_wave_pairs(pairs)
        return e

    def __exit__(self, *exc):
        e = self.emu
        e.set_engine(True), e.set_group(0), e.set_unit(True), e.set_late(False), e.set_wave_pairs(False)


def _key(key_bits):
    g = load_golden(key_bits)
    return la.KeyMath(int(g["p"], 16), int(g["q"], 16))


def _result_first_rows(emu, key, n_arr, op, rng, all_starts=True):
    """(rows, M, nl, L): the batch of targets for the rung that is set, laid out on the lanes its last subtraction runs on.
    256 bits: every row family_targets makes (every run start, three or four run lengths, borrow arriving and not).  1024 bits:
    one row per (run start, borrow arrives or not) — every start, both cases.  all_starts=False (the whole-wave rungs at 1024 bits
    other than encrypt on its plain and its wave-pair form — the two row counts a whole-wave number can have; 0.85 s per emulated
    row on 72 / 74 lanes): the edges, the half boundary and every 12th start.
    Asserted here: no run start is lost, and every family holds a row with the borrow arriving and one without where it can."""
    pair, G, L, digits = emu.exit_layout(n_arr, op)
    nl, half = (2 * digits // L, digits // L) if pair else (G, None)
    M = key.nsq
    small = key.n.bit_length() <= 256
    arrives = lambda t: la.borrow_arrives(t, M, nl, L)
    top = max(g for g, v in enumerate(la.split_lanes(M, nl, L)) if v)
    fam = {}
    for f in la.FAMILIES:
        full = la.unit_targets(la.family_targets(M, nl, L, rng, f, half, stride=1 if all_starts else 12), key.n)
        fam[f] = full if small else la.thin_cells(full, arrives)
        starts = {la.run_start(tag) for _, tag in full} - {None}
        assert starts == {la.run_start(tag) for _, tag in fam[f]} - {None}, f
        if f in ("EQ", "ONES", "ZERO") and top > 0 and all_starts:
            missing = set(range(top + 1)) - starts
            assert not missing or (f == "EQ" and missing <= {top}), (f, sorted(missing))   # (EQ from the top lane alone: t >= M)
        for want in (True, False):                           # a borrow arriving at a lane equal to M's, and none: kept if made
            if any(bool(arrives(t)) == want for t, _ in full):
                assert any(bool(arrives(t)) == want for t, _ in fam[f]), (f, want)
    if top > 0:                                              # by construction in EQ and HALF (pairs) ...
        assert any(arrives(t) for t, _ in fam["EQ"]) and any(not arrives(t) for t, _ in fam["EQ"])
    if top > 1:
        assert any(arrives(t) for t, _ in fam["HALF"]) and any(not arrives(t) for t, _ in fam["HALF"])
        for f in ("ONES", "ZERO", "NEAR"):                   # ... and wherever M's digits allow it in the others
            assert any(not arrives(t) for t, _ in fam[f]), f
    per = 64 // G
    rows = la.batch_layout(fam, per, rng, lambda: la.random_unit(M, rng), per * (4 if per <= 8 else 2))
    return rows, M, nl, L


def _all_starts(key_bits, rung):
    return key_bits <= 256 or RUNG[rung][2] != 64


def _check(got, rows, what):
    bad = la.first_mismatch(limbs_to_ints(got), [t for t, _ in rows], [tag for _, tag in rows])
    assert bad is None, "%s: %s" % (what, bad)


@pytest.mark.parametrize("rung", [r[0] for r in RUNGS])
@pytest.mark.parametrize("key_bits", [256, 1024])
def test_encrypt_returns_the_chosen_ciphertext(emu, key_bits, rung):
    """t chosen on the lanes of the rung's last subtraction (EQ / ONES / ZERO / NEAR / HALF, whole waves, one row per wave in every
    group position, top-lane row beside lane-0 row, ragged end); m and r follow from the private key; the kernel must return t.
    Every run start on every rung at 256 and 1024 bits, but for the late form of the whole-wave rung at 1024 bits (its layout is the
    wave pairs', which carries every start; see _result_first_rows)."""
    key = _key(key_bits)
    s1 = key_bits // 32
    n_arr = int_to_limbs(key.n, s1)
    rng = random.Random(8000 + key_bits + len(rung))
    with _Rung(emu, rung) as e:
        rows, M, nl, L = _result_first_rows(e, key, n_arr, "encrypt", rng, _all_starts(key_bits, rung) or rung in ("split-g64", "split-g64-pairs"))
        pre = [key.preimage_encrypt(t, check=i % 16 == 0) for i, (t, _) in enumerate(rows)]
        got = e.encrypt(n_arr, ints_to_limbs([m for m, _ in pre], s1), ints_to_limbs([r for _, r in pre], s1))
        assert e.last_exit() == e.exit_layout(n_arr, "encrypt")     # the lanes the rows were laid out on are the ones that ran
    _check(got, rows, "encrypt %d %s on %d lanes of %d" % (key_bits, rung, nl, L))


OTHER_RUNGS = ["split-auto", "split-g2", "split-g4", "split-g8", "split-g16", "split-g64", "split-g16-late", "split-g64-pairs",
               "full-auto", "full-g8"]


@pytest.mark.parametrize("rung", OTHER_RUNGS)
@pytest.mark.parametrize("key_bits", [256, 1024])
def test_obfuscate_returns_the_chosen_ciphertext(emu, key_bits, rung):
    """as above through the obfuscate form (c_in r^n): c_in another encryption of t's plaintext.  On the late rungs the last
    subtraction is the product kernel's canonicalize on n^2's full-width geometry, and the rows are laid out on that."""
    key = _key(key_bits)
    s1 = key_bits // 32
    n_arr = int_to_limbs(key.n, s1)
    rng = random.Random(8100 + key_bits + len(rung))
    with _Rung(emu, rung) as e:
        rows, M, nl, L = _result_first_rows(e, key, n_arr, "obfuscate", rng, _all_starts(key_bits, rung))
        pre = [key.preimage_obfuscate(t, rng, check=i % 16 == 0) for i, (t, _) in enumerate(rows)]
        got = e.obfuscate(n_arr, ints_to_limbs([c for c, _ in pre], 2 * s1), ints_to_limbs([r for _, r in pre], s1))
        assert e.last_exit() == e.exit_layout(n_arr, "obfuscate")     # the lanes the rows were laid out on are the ones that ran
    _check(got, rows, "obfuscate %d %s on %d lanes of %d" % (key_bits, rung, nl, L))


@pytest.mark.parametrize("rung", OTHER_RUNGS)
@pytest.mark.parametrize("key_bits", [256, 1024])
def test_powmod_returns_the_chosen_power(emu, key_bits, rung):
    """base = t^(k^-1 mod n lambda) for exponents k coprime to n lambda: 3, 17-bit, 64-bit and full-width k in one batch"""
    key = _key(key_bits)
    s1 = key_bits // 32
    n_arr = int_to_limbs(key.n, s1)
    rng = random.Random(8200 + key_bits + len(rung))
    with _Rung(emu, rung) as e:
        rows, M, nl, L = _result_first_rows(e, key, n_arr, "powmod", rng, _all_starts(key_bits, rung))
        ks = [key.coprime_exponent((3, rng.getrandbits(17) | 1, rng.getrandbits(64) | 1, rng.randrange(key.n >> 1) | 1)[i % 4])
              for i in range(len(rows))]
        bases = [key.preimage_powmod(t, k, check=i % 16 == 0) for i, ((t, _), k) in enumerate(zip(rows, ks))]
        got = e.powmod_n2(n_arr, ints_to_limbs(bases, 2 * s1), ints_to_limbs(ks, s1))
        assert e.last_exit() == e.exit_layout(n_arr, "powmod")     # the lanes the rows were laid out on are the ones that ran
    _check(got, rows, "powmod %d %s on %d lanes of %d" % (key_bits, rung, nl, L))


@pytest.mark.parametrize("group", [0, 2, 4, 8, 16])
@pytest.mark.parametrize("key_bits", [256, 1024])
def test_products_return_the_chosen_residue(emu, key_bits, group):
    """a b = t (mod n^2) through the staged product (csrc/mul_io.h) and the plain body, t on the lanes of n^2's geometry"""
    key = _key(key_bits)
    s2 = key_bits // 16
    M = key.nsq
    M_arr = int_to_limbs(M, s2)
    rng = random.Random(8300 + key_bits + group)
    import adversarial
    emu.set_group(group)
    try:
        G, L = emu.modulus_geometry(M_arr)
        fam = {f: la.family_targets(M, G, L, rng, f) for f in la.FAMILIES}
        rows = la.batch_layout(fam, 64 // G, rng, lambda: rng.randrange(M), 64)
        a, b = adversarial.pairs_for([t for t, _ in rows], M, rng, n_root=key.n)
        assert all(x * y % M == t for x, y, (t, _) in zip(a, b, rows))
        for staged in (1, 0):
            emu.L.emu_set_mul_io(staged)
            got = emu.mulmod(M_arr, ints_to_limbs(a, s2), ints_to_limbs(b, s2))
            _check(got, rows, "mulmod %d group %d staged %d on %d lanes of %d" % (key_bits, group, staged, G, L))
    finally:
        emu.set_group(0)
        emu.L.emu_set_mul_io(1)


_decrypt_rows = la.decrypt_rows


@pytest.mark.parametrize("rung", ["split-auto", "split-g2", "split-g4", "split-g8", "split-g16", "split-g64", "split-g16-late",
                                  "split-g64-pairs", "full-auto"])
@pytest.mark.parametrize("key_bits", [256, 1024])
def test_both_decrypt_tails_return_the_chosen_plaintext(emu, key_bits, rung):
    """the per-thread tail (decrypt_tail_one) and the tail on one wavefront per ciphertext must both give m, on every rung of the
    CRT halves"""
    key = _key(key_bits)
    g = load_golden(key_bits)
    s1, h = key_bits // 32, key_bits // 64
    rng = random.Random(8400 + key_bits + len(rung))
    rows = _decrypt_rows(key, rng, 6 if key_bits == 256 else 2)
    if key_bits == 1024 and RUNG[rung][2] >= 16:
        rows = la.thin_decrypt_rows(rows, 8, key)            # (0.5 ... 1 s per emulated row on these rungs; the edge rows all stay)
    assert key.decrypt(key.ciphertext_of(rows[0][0], rng)) == rows[0][0]
    c = ints_to_limbs([key.ciphertext_of(m, rng) for m, _ in rows], 2 * s1)
    keyarr = [int_to_limbs(int(g[k], 16), h) for k in ("p", "q", "hp", "hq", "p_inverse")]
    with _Rung(emu, rung) as e:
        try:
            for tail in (True, False):
                e.set_wave_tail(tail)
                got = limbs_to_ints(e.decrypt(*keyarr, s1, c))
                bad = la.first_mismatch(got, [m for m, _ in rows], [tag for _, tag in rows])
                assert bad is None, "decrypt %d %s wave tail %s: %s" % (key_bits, rung, tail, bad)
        finally:
            e.set_wave_tail(False)


_strong_probable_prime = la.strong_probable_prime


@pytest.mark.parametrize("k,c", [(127, 1), (255, 19), (521, 1), (128, 3), (256, 189), (512, 569), (250, 207), (1023, 361)])
def test_miller_rabin_on_moduli_with_whole_lanes_of_ones(emu, k, c):
    """csrc/primality.h on n = 2^k - c (primes and composites: every lane but the lowest is all ones, so each comparison with n and
    each subtraction of n meets lanes that propagate), with bases whose power a^d is 1, n - 1, or neither, and bases next to n"""
    n = (1 << k) - c
    words = -(-k // 32)
    rng = random.Random(8500 + k)
    d, s = n - 1, 0
    while d % 2 == 0:
        d, s = d // 2, s + 1
    b = rng.randrange(2, n - 1)
    bases = [2, 3, n - 1, n - 2, 1, pow(b, 1 << s, n), pow(b, 1 << max(0, s - 1), n), b, (1 << (k - 1)) - 1, (1 << (k - 1)) + 1,
             n - (1 << 29), n >> 1] + [rng.randrange(2, n - 1) for _ in range(4)]
    bases = [a for a in bases if 0 < a < n]
    want = [_strong_probable_prime(n, a) for a in bases]
    assert any(pow(a, d, n) in (1, n - 1) for a in bases)
    got = emu.miller_rabin(ints_to_limbs([n] * len(bases), words), ints_to_limbs(bases, words))
    assert got.tolist() == want, (k, c, [i for i, (x, y) in enumerate(zip(got.tolist(), want)) if x != y])


def _table_fold_remainder(a, b, N, info):
    """r = y - q^ N as csrc/mul_table.h forms it for a * b: y = lo + sum f_i (W^(P+i) mod N) over the limbs f_i of a b above limb
    P = info["split"]; q^ = floor(yd * inv) - 1 (0 below 1) with yd the four limbs of y from info["base"] on, summed in doubles in
    the kernel's order, inv = info["inv"] (key_setup.h build_table_mul).  canonicalize subtracts N floor(r / N) times."""
    W, P = 1 << 29, info["split"]
    T = a * b
    y, hi, i = T & ((1 << (29 * P)) - 1), T >> (29 * P), 0
    while hi:
        y += (hi & MASK) * pow(W, P + i, N)
        hi >>= 29
        i += 1
    assert i <= info["digits"]
    l0, l1, l2, l3 = [float((y >> (29 * (info["base"] + k))) & MASK) for k in range(4)]
    assert y >> (29 * (info["base"] + 4)) == 0
    yd = (l3 * 536870912.0 + l2) * 288230376151711744.0 + (l1 * 536870912.0 + l0)
    qd = math.floor(yd * info["inv"])
    return y - (int(qd) - 1 if qd >= 1.0 else 0) * N


# ---- the other callers: the table product's canonicalize, multiexp, the key owner's encrypt, keys off the limb grid ------------
@pytest.mark.parametrize("key_bits", [1024, 2048])
def test_table_product_returns_the_chosen_residue_through_two_subtractions(emu, key_bits):
    """csrc/mul_table.h (k_mulmod_table: one plain product, one fold against the key's table) ends in canonicalize on a value
    r = y - q^ N below 3 N, q^ one or two below floor(y / N): the ONE kernel whose canonicalize takes its second subtraction (16 x 5
    at 1024 bits, 16 x 9 at 2048: where the old suite's hits came from).  q^ comes from a double-precision product on four limbs of
    y; _table_fold_remainder restates the fold and that estimate on Python integers and IEEE doubles, so the test ASSERTS that
    rows with r in [2N, 3N) — two subtractions — and in [N, 2N) are in the batch (about one row in 25 and one in 600 take two:
    hence the ladders of small residues besides the lane families).  The emulator-only mutant `canonicalize with one subtraction`
    gets exactly the predicted rows wrong."""
    import adversarial
    key = _key(key_bits)
    M, s2 = key.nsq, key_bits // 16
    M_arr = int_to_limbs(M, s2)
    rng = random.Random(8600 + key_bits)
    L = {1024: 5, 2048: 9}[key_bits]
    assert 16 * L * 29 >= M.bit_length() + 4
    rows = []
    for f in la.FAMILIES:
        full = la.family_targets(M, 16, L, rng, f)
        rows += full if f in ("NEAR", "HALF") else la.thin_cells(full, lambda t: la.borrow_arrives(t, M, 16, L))
    rows += [(rng.randrange(1 << e), "small < 2^%d" % e) for e in range(1, 2 * key_bits - 60, 97)]
    rows += [(M - 1 - rng.randrange(1 << e), "n^2 - small < 2^%d" % e) for e in range(1, 2 * key_bits - 60, 193)]
    rows += [(i, "t = %d" % i) for i in range(48)] + [(rng.randrange(1 << 29), "one digit") for _ in range(2400)]
    rows += [(rng.randrange(1 << 58), "two digits") for _ in range(24)]
    a, b = adversarial.pairs_for([t for t, _ in rows], M, rng, n_root=key.n)
    info = emu.table_mul_info(M_arr, 16)
    assert info is not None and info["L"] == L
    rem = [_table_fold_remainder(x, y, M, info) for x, y in zip(a, b)]
    assert all(0 <= r < 3 * M and r % M == t for r, (t, _) in zip(rem, rows))
    twice = [i for i, r in enumerate(rem) if r >= 2 * M]
    assert len(twice) >= 3 and any(M <= r < 2 * M for r in rem), len(twice)   # the second subtraction is in the batch, by the restated estimate
    got = emu.mulmod_table(M_arr, ints_to_limbs(a, s2), ints_to_limbs(b, s2))
    assert got is not None
    _check(got, rows, "table product %d" % key_bits)


@pytest.mark.parametrize("rung", ["split-auto", "split-g2", "split-g4", "split-g8", "split-g16", "split-g64"])
@pytest.mark.parametrize("key_bits", [256, 1024])
def test_multiexp_returns_the_chosen_product(emu, key_bits, rung):
    """k_multiexp_split's way out (split_exit with no plaintext): every chunk of three bases has its product chosen, the last base
    solved for: b_2 = (t / (b_0^e_0 b_1^e_1))^(1 / e_2)"""
    key = _key(key_bits)
    s1, s2 = key_bits // 32, key_bits // 16
    n_arr = int_to_limbs(key.n, s1)
    rng = random.Random(8700 + key_bits + len(rung))
    M = key.nsq
    with _Rung(emu, rung) as e:
        rows, M, nl, L = _result_first_rows(e, key, n_arr, "powmod", rng, _all_starts(key_bits, rung))
        if key_bits == 1024 and RUNG[rung][2] == 64:
            rows = rows[::3]                                 # (three exponentiations per row on 72 lanes)
        bases, exps = [], []
        for t, _ in rows:
            b0, b1 = la.random_unit(M, rng), la.random_unit(M, rng)
            e0, e1, e2 = rng.getrandbits(56), rng.getrandbits(64) | 1, key.coprime_exponent(rng.getrandbits(64) | 1)
            rest = pow(b0, e0, M) * pow(b1, e1, M) % M
            b2 = key.preimage_powmod(t * pow(rest, -1, M) % M, e2)
            bases += [b0, b1, b2]
            exps += [e0, e1, e2]
        assert pow(bases[0], exps[0], M) * pow(bases[1], exps[1], M) * pow(bases[2], exps[2], M) % M == rows[0][0]
        parts = e.multiexp_n2(n_arr, ints_to_limbs(bases, s2), ints_to_limbs(exps, 2), 3)
    assert parts is not None and parts.shape == (len(rows), 1, s2)
    _check(parts[:, 0], rows, "multiexp %d %s on %d lanes of %d" % (key_bits, rung, nl, L))


@pytest.mark.parametrize("rung", ["split-auto", "split-g8", "split-g16", "split-g16-late", "split-g64"])
@pytest.mark.parametrize("key_bits", [256, 1024])
def test_owner_encrypt_returns_the_chosen_ciphertext(emu, key_bits, rung):
    """raw_encrypt by the key owner: r^n from the CRT halves (half-decrypt exit modulo p^2 and q^2), crt_lift_body, then the
    product with 1 + n m, whose canonicalize on n^2's full-width geometry is the last subtraction: t is laid out on that.  The
    lift's own word u = (r^n mod n^2) // p^2 cannot be chosen: r^n is an n-th residue, one of phi(n) values, fixed by t."""
    key = _key(key_bits)
    g = load_golden(key_bits)
    s1, h = key_bits // 32, key_bits // 64
    n_arr = int_to_limbs(key.n, s1)
    keyarr = [int_to_limbs(int(g[k], 16), h) for k in ("p", "q", "hp", "hq", "p_inverse")]
    rng = random.Random(8800 + key_bits + len(rung))
    M = key.nsq
    with _Rung(emu, rung) as e:
        e.set_late(False)
        G, L = e.modulus_geometry(int_to_limbs(M, 2 * s1))
        if (G, L) in ((4, 36), (2, 36)):                     # (the products take the light geometry: phe_hip.hip light_geometry)
            G, L = 2 * G, 18
        e.set_late(RUNG[rung][4])
        arrives = lambda t: la.borrow_arrives(t, M, G, L)
        rows = []
        for f in la.FAMILIES:
            full = la.unit_targets(la.family_targets(M, G, L, rng, f), key.n)
            rows += full if key_bits == 256 else la.thin_cells(full, arrives)
        if key_bits == 1024 and RUNG[rung][2] >= 16:
            rows = rows[::3]                                 # (the lanes are the product's, the same on every rung)
        pre = [key.preimage_encrypt(t, check=i % 16 == 0) for i, (t, _) in enumerate(rows)]
        got = e.encrypt_owner(n_arr, *keyarr, ints_to_limbs([m for m, _ in pre], s1), ints_to_limbs([r for _, r in pre], s1))
    assert got is not None
    _check(got, rows, "owner encrypt %d %s on %d lanes of %d" % (key_bits, rung, G, L))


@pytest.mark.parametrize("rung", ["split-auto", "split-g8", "split-g16", "split-g64", "full-auto"])
@pytest.mark.parametrize("key_bits", [232, 968])
def test_keys_off_the_limb_grid_return_the_chosen_rows(emu, key_bits, rung):
    """n of 232 and 968 bits (seeded primes): n, p and q do not fill their 32-bit rows nor their rungs, so the top lanes of every
    group are padding.  encrypt returns the chosen t, both decrypt tails the chosen m"""
    key, hp, hq = la.off_grid_key(key_bits)
    p, q, n = key.p, key.q, key.n
    s1 = 2 * ((key_bits + 63) // 64)
    n_arr = int_to_limbs(n, s1)
    keyarr = [int_to_limbs(v, s1 // 2) for v in (p, q, hp, hq, pow(p, -1, q))]
    rng = random.Random(8900 + key_bits + len(rung))
    with _Rung(emu, rung) as e:
        try:
            rows, M, nl, L = _result_first_rows(e, key, n_arr, "encrypt", rng, True)
            if key_bits > 256 and RUNG[rung][2] >= 16:
                rows = rows[::4]
            pre = [key.preimage_encrypt(t, check=i % 16 == 0) for i, (t, _) in enumerate(rows)]
            got = e.encrypt(n_arr, ints_to_limbs([m for m, _ in pre], s1), ints_to_limbs([r for _, r in pre], s1))
            _check(got, rows, "encrypt %d %s on %d lanes of %d" % (key_bits, rung, nl, L))
            drows = _decrypt_rows(key, rng, 3 if key_bits < 256 else 1)
            if key_bits > 256 and RUNG[rung][2] >= 16:
                drows = la.thin_decrypt_rows(drows, 4, key)
            c = ints_to_limbs([key.ciphertext_of(m, rng) for m, _ in drows], 2 * s1)
            for tail in (True, False):
                e.set_wave_tail(tail)
                bad = la.first_mismatch(limbs_to_ints(e.decrypt(*keyarr, s1, c)), [m for m, _ in drows], [tag for _, tag in drows])
                assert bad is None, "decrypt %d %s wave tail %s: %s" % (key_bits, rung, tail, bad)
        finally:
            e.set_wave_tail(False)
