"""Lane patterns for the carry / borrow look-ahead of a limb group (TEST HELPER, not a conftest).

csrc/mont_core.h group_carry_in resolves the carries between the G lanes of a group from two ballots: the lanes that GENERATE a
carry (or borrow) and the lanes that would PROPAGATE one.  A lane propagates only when all its L digits are special — 2^29 - 1
(normalize_full) or equal to the modulus's digits (cond_sub, cond_sub_pair) — which random data never produces.  Here every lane
of a number is given a KIND first and the digits follow:

    'P'  propagate   all ones / equal to the reference lane
    'G'  generate    carries out of its own sweep / smaller than the reference lane (a borrow leaves it)
    'K'  kill        neither: an arriving carry stops here

and, for the kernels, the RESULT is laid out on the lanes of a geometry (G, L) first and the kernel's inputs are derived from it
with the private key (see preimage_* below).  Everything here works on Python integers; the geometry is an argument, never read
back from the code under test."""
import itertools
import math

DIGIT = 29
MASK = (1 << DIGIT) - 1
SLOP = 256                                                     # almost-normalised limbs are < 2^29 + 2^8 (mont_core.h)


# ---- lanes <-> integers -------------------------------------------------------------------------------------------------------
def split_lanes(x, G, L):
    m = (1 << (DIGIT * L)) - 1
    return [(x >> (DIGIT * L * g)) & m for g in range(G)]


def join_lanes(lanes, L):
    return sum(v << (DIGIT * L * g) for g, v in enumerate(lanes))


def digits(x, count):
    return [(x >> (DIGIT * j)) & MASK for j in range(count)]


def value(limbs):
    return sum(int(v) << (DIGIT * j) for j, v in enumerate(limbs))


# ---- the reference: a ripple, lane by lane ------------------------------------------------------------------------------------
def ripple(G, gen, prop):
    """(cin, out_top) of 64-bit ballots the slow way: the carry walks up the lanes of each group and never leaves it"""
    cin = out = 0
    for base in range(0, 64, G):
        c = 0
        for lane in range(base, base + G):
            cin |= c << lane
            c = ((gen >> lane) & 1) | (((prop >> lane) & 1) & c)
        out |= c << (base + G - 1)
    return cin, out


def receives(kinds):
    """for a string of lane kinds: the lanes that are 'P' AND have a carry arriving (the only place the propagate term matters)"""
    c, hit = 0, []
    for g, k in enumerate(kinds):
        if k == "P" and c:
            hit.append(g)
        c = 1 if k == "G" else (c if k == "P" else 0)
    return hit


def carry_out(kinds):
    c = 0
    for k in kinds:
        c = 1 if k == "G" else (c if k == "P" else 0)
    return c


# ---- lane-kind patterns -------------------------------------------------------------------------------------------------------
def patterns(n, rng, exhaustive_upto=4, random_count=24):
    """strings over 'PGK' for a number of n lanes: all 3^n for short numbers; otherwise every run of 'P' lanes at every position,
    with the lane below generating and not, the rest of the lanes 'G' / 'K' at random; a second run elsewhere; all lanes above
    lane 0; and seeded random strings.  (For n = 64 or more the run positions are the edges, the middle and a seeded sample.)"""
    if n <= exhaustive_upto:
        return ["".join(p) for p in itertools.product("PGK", repeat=n)]
    out = []
    starts = range(n) if n <= 16 else sorted({0, 1, 2, n // 2 - 1, n // 2, n - 3, n - 2, n - 1} | {rng.randrange(n) for _ in range(8)})
    for a in starts:
        lengths = range(1, n - a + 1) if n <= 16 else sorted({1, 2, 3, n - a} | {rng.randrange(1, n - a + 1)})
        for ln in lengths:
            if ln > n - a:
                continue
            for below in "GK":
                s = [rng.choice("GKK") for _ in range(n)]
                s[a:a + ln] = "P" * ln
                if a > 0:
                    s[a - 1] = below
                if a + ln < n:
                    s[a + ln] = rng.choice("GK")
                out.append("".join(s))
    for below in "GK":                                         # everything above lane 0, and everything
        out.append(below + "P" * (n - 1))
    out.append("P" * n)
    for _ in range(random_count):                              # two runs, and free strings rich in 'P'
        out.append("".join(rng.choice("PPGK") for _ in range(n)))
    return out


def neighbour_wave(G, rng):
    """64/G patterns for consecutive groups of one wave, alternating a run that ENDS in the top lane with the lane below generating
    (the group carries out) and a run that STARTS in lane 0 (which a leaked carry would ripple through)"""
    out = []
    for i in range(64 // G):
        if G == 1:
            out.append("GP"[i % 2])
        elif i % 2 == 0:
            run = 1 + (i // 2) % (G - 1)
            out.append("K" * (G - 1 - run) + "G" + "P" * run)
        else:
            run = 1 + (i // 2) % (G - 1)
            out.append("P" * run + "K" * (G - run))
    return out


def pack_waves(cases, per_wave, rng):
    """cases -> rows of `per_wave`, three times: in order, rotated by one place, and shuffled (so that a case meets different
    neighbours and sits in different groups of the wave); the last row is filled up with cases drawn again"""
    orders = [list(cases), list(cases[1:]) + list(cases[:1]), rng.sample(list(cases), len(cases))]
    rows = []
    for order in orders:
        while len(order) % per_wave:
            order.append(rng.choice(cases))
        rows += [order[i:i + per_wave] for i in range(0, len(order), per_wave)]
    return rows


# ---- digits for a kind --------------------------------------------------------------------------------------------------------
def _lane_max(L):
    return (1 << (DIGIT * L)) - 1


def reference_lanes(G, L, rng, top_room_bits=0):
    """a modulus laid out on lanes: every lane strictly inside (0, max) so that a smaller and a larger lane exist; odd; the top lane
    leaves `top_room_bits` leading zero bits (R >= 16 N in the kernels: 4)"""
    lanes = []
    for g in range(G):
        hi = _lane_max(L) >> (top_room_bits if g == G - 1 else 0)
        style = rng.randrange(4)
        if style == 0:
            v = rng.randrange(2, hi - 1)
        elif style == 1:
            v = 2 + rng.randrange(1 << DIGIT) % (hi - 3)       # small lane: only its low digit(s) are non-zero
        elif style == 2:
            v = hi - 2 - rng.randrange(1 << DIGIT) % (hi - 3)  # lane next to all ones
        else:
            v = rng.randrange(2, hi - 1) & ~MASK | 1           # zero low digit region but odd
        lanes.append(max(2, min(hi - 2, v)))
    lanes[0] |= 1
    return lanes


def lanes_against(kinds, ref, L, rng, top_cap=None):
    """lanes of a number whose lane g is equal to ('P'), smaller than ('G') or larger than ('K') ref[g]; smaller / larger by one,
    in the top digit only, or at random.  top_cap: the top lane stays at or below it (a value below 2 N)"""
    out = []
    for g, k in enumerate(kinds):
        r = ref[g]
        if k == "P":
            v = r
        elif k == "G":
            v = (r - 1, rng.randrange(0, r), 0, r - (r & MASK) if r & MASK else r - 1)[rng.randrange(4)]
        else:
            hi = _lane_max(L)
            if top_cap is not None and g == len(kinds) - 1:
                hi = max(r + 1, min(hi, top_cap))
            v = (r + 1, rng.randrange(r + 1, hi + 1), hi, min(hi, r + (1 << (DIGIT * (L - 1)))))[rng.randrange(4)]
        out.append(v)
    return out


def lanes_of_ones(kinds, L, rng):
    """ALMOST-NORMALISED limbs (a list of G * L) of a number whose lane g, after its own carry sweep, is all ones ('P'), has carried
    out ('G') or neither ('K').  'G' lanes: a top limb of 2^29 + x, or a limb of 2^29 + x below limbs that are all ones (the carry
    runs through the rest of the lane).  'K' lanes may hold such limbs too, below a limb that absorbs the carry."""
    limbs = []
    for k in kinds:
        if k == "P":
            lane = [MASK] * L
        elif k == "G":
            lane = [rng.randrange(MASK + 1) for _ in range(L)]
            j = rng.randrange(L)
            lane[j] = (1 << DIGIT) + rng.randrange(SLOP)
            style = rng.randrange(3)
            for i in range(j + 1, L):
                lane[i] = MASK if style < 2 else (1 << DIGIT) + rng.randrange(SLOP)
            if style == 1:
                lane[:j] = [MASK] * j                          # all ones below the limb that overflows
        else:
            lane = [rng.randrange(MASK + 1) for _ in range(L)]
            style = rng.randrange(4)
            if style == 0:
                lane = [MASK] * L
                lane[rng.randrange(L)] = rng.randrange(MASK)   # ones but for one digit
            elif style == 1 and L > 1:
                j = rng.randrange(L - 1)
                lane[j] = (1 << DIGIT) + rng.randrange(SLOP)
                lane[j + 1] = rng.randrange(MASK - 1)          # absorbs the carry
            elif style == 2:
                lane = [0] * L
            if all(v == MASK for v in lane):
                lane[0] = MASK - 1
        limbs += lane
    return limbs


def sloppy(limbs, rng, p=0.7):
    """same value, some limbs pushed to the almost-normalised range (< 2^29 + 2^8) by borrowing from the limb above"""
    limbs = list(limbs)
    for k in range(len(limbs) - 1):
        if limbs[k] < SLOP and limbs[k + 1] >= 1 and rng.random() < p:
            limbs[k] += 1 << DIGIT
            limbs[k + 1] -= 1
    return limbs


# ---- result-first rows for the kernels ----------------------------------------------------------------------------------------
FAMILIES = ("EQ", "ONES", "ZERO", "NEAR", "HALF")


def _positions(top, half, rng, stride=1):
    """lanes a run starts at: every lane up to M's top lane.  stride > 1 (asked for by name, only where a row costs most): the
    edges, both sides of the half boundary and every stride-th lane"""
    if stride <= 1:
        return list(range(top + 1))
    keep = {0, 1, 2, top - 2, top - 1, top} | set(range(0, top + 1, stride))
    if half:
        keep |= {half - 2, half - 1, half, half + 1}
    return sorted(g for g in keep if 0 <= g <= top)


def family_targets(M, nl, L, rng, family, half=None, stride=1):
    """Targets in [0, M) laid out on nl lanes of L digits: a list of (t, tag).  M is the modulus the kernel's last conditional
    subtraction compares with (n^2 for ciphertexts); half: the lane where the high half of a pair starts (split_exit), or None.
    Lanes above M's top lane hold zeros in t and in M alike (padding: they always propagate).  EQ holds, for every run, a row where
    a borrow arrives at the run and a row where none does; the other families do whenever the digits allow it (see the tags)."""
    mask = _lane_max(L)
    ml = split_lanes(M, nl, L)
    top = max(g for g in range(nl) if ml[g])                   # the highest lane M reaches
    out = []

    def rand_lanes():
        return [rng.randrange(mask + 1) for _ in range(top + 1)]

    def smaller(r):
        return rng.choice((r - 1, rng.randrange(r), 0))

    def larger(r):
        return rng.choice((r + 1, rng.randrange(r + 1, mask + 1), mask))

    def close_below(lanes, first_free):
        """lanes[first_free ..] are free: make the value smaller than M there (the top lane smaller, or equal and the next one ...)"""
        g = top
        while g > first_free and rng.random() < 0.25:          # some rows equal M in the top lanes too: longer borrow chains
            lanes[g] = ml[g]
            g -= 1
        while g >= first_free and ml[g] == 0:
            lanes[g] = 0
            g -= 1
        if g < first_free:
            return None
        lanes[g] = smaller(ml[g])
        return lanes

    def borrow_tag(lanes):
        kinds = "".join("P" if v == r else ("G" if v < r else "K") for v, r in zip(lanes, ml))
        return " kinds=%s hit=%s" % (kinds, receives(kinds))

    if top == 0 and family in ("EQ", "HALF"):                  # M on ONE lane: no lane to propagate through, the NEAR rows stand in
        family = "NEAR"
    if family == "EQ":
        for a in _positions(top, half, rng, stride):
            for ln in sorted({1, 2, 3, max(1, top - a)}):
                if a + ln > top + 1:
                    continue
                for arrives in ((True, False) if a > 0 else (False,)):
                    lanes = rand_lanes()
                    lanes[a:a + ln] = ml[a:a + ln]
                    if a > 0:
                        r = ml[a - 1]
                        if (arrives and r == 0) or (not arrives and r == mask):
                            continue
                        lanes[a - 1] = smaller(r) if arrives else larger(r)
                    if a + ln <= top:
                        if close_below(lanes, a + ln) is None:
                            continue
                    elif not arrives:
                        continue                               # equal up to the top and no borrow: t >= M, not a residue
                    v = join_lanes(lanes, L)
                    assert v < M
                    out.append((v, "EQ run %d+%d%s %s%s" % (a, ln, " top" if a + ln == top + 1 else "", "borrow" if arrives else "none", borrow_tag(lanes))))
    elif family in ("ONES", "ZERO"):
        fill = mask if family == "ONES" else 0
        for a in _positions(top, half, rng, stride):
            for ln in sorted({1, 2, top + 1 - a}):
                if a + ln > top + 1:
                    continue
                for below in ("G", "K"):                       # the lane below the run smaller / larger than M's
                    lanes = rand_lanes()
                    lanes[a:a + ln] = [fill] * ln
                    if a > 0 and 0 < ml[a - 1] < mask:
                        lanes[a - 1] = smaller(ml[a - 1]) if below == "G" else larger(ml[a - 1])
                    if a + ln <= top:
                        if close_below(lanes, a + ln) is None:
                            continue
                    v = join_lanes(lanes, L)
                    if v >= M:                                 # (a run of ones through the top lane: shorten it by M's leading digits)
                        v = (v & ((1 << (M.bit_length() - 1)) - 1))
                    out.append((v, "%s run %d+%d%s" % (family, a, ln, borrow_tag(split_lanes(v, top + 1, L)))))
    elif family == "NEAR":
        one_lane = 1 << (DIGIT * L)
        small = [0, 1, 2, rng.randrange(3, 1 << DIGIT), one_lane - 1, one_lane, one_lane + 1, rng.randrange(one_lane, one_lane << DIGIT)]
        small = [s % M for s in small]
        out += [(s, "NEAR small") for s in small] + [(M - s, "NEAR M-small") for s in small if s]
    elif family == "HALF":                                     # patterns across the boundary between the two halves of a pair
        h = half if half else max(1, (top + 1) // 2)
        h = min(h, top)
        for lo_kind in ("eq", "ones", "zero"):
            for arrives in (True, False):
                for hk in ("eq", "ones", "zero", "any"):
                    lanes = rand_lanes()
                    lanes[:h] = {"eq": ml[:h], "ones": [mask] * h, "zero": [0] * h}[lo_kind]
                    if lo_kind == "eq":                        # the whole low half propagates: lane 0 decides whether a borrow enters
                        r = ml[0]
                        lanes[0] = smaller(r) if arrives else (larger(r) if r < mask else r)
                    elif not arrives:
                        continue
                    free = h
                    if hk != "any" and h < top:
                        lanes[h] = {"eq": ml[h], "ones": mask, "zero": 0}[hk]
                        free = h + 1
                    if close_below(lanes, free) is None:
                        continue
                    v = join_lanes(lanes, L)
                    if v < M:
                        out.append((v, "HALF %s|%s%s" % (lo_kind, hk, borrow_tag(lanes))))
    else:
        raise ValueError(family)
    assert out and all(0 <= t < M for t, _ in out), family
    return out


def borrow_arrives(t, M, nl, L):
    """the lanes of t (against M, on nl lanes of L digits) that equal M's lane AND have a borrow arriving: the Python predicate for
    'this row runs the propagate term of the final subtraction' (t is the subtraction's input whenever t < M is the result)"""
    ml = split_lanes(M, nl, L)
    top = max(g for g in range(nl) if ml[g])
    kinds = "".join("P" if v == r else ("G" if v < r else "K") for v, r in zip(split_lanes(t, nl, L), ml))
    return [g for g in receives(kinds) if g <= top]            # (the padding lanes above M always propagate: not counted)


def unit_targets(ts, n):
    """every target made a unit modulo n^2 (a ciphertext must be one): a target that shares a factor with n is REPLACED by the same
    lanes with the low digit moved until it is one — never dropped"""
    out = []
    for t, tag in ts:
        t0, step = t, 0
        while math.gcd(t, n) != 1 or t == 0 or (t != t0 and any(t == u for u, _ in out)):
            step += 1
            t = (t0 + step * (1 << DIGIT) + step) % (n * n)    # digit 1 and digit 0 move: the lanes above keep their pattern
        out.append((t, tag if t == t0 else tag + " (moved to a unit)"))
    return out


class KeyMath:
    """the private key's view of a Paillier key, on Python integers (the formulas of the reference's raw_decrypt / raw_encrypt;
    powers modulo n^2 go through p^2 and q^2, four times cheaper)"""

    def __init__(self, p, q):
        self.p, self.q, self.n = p, q, p * q
        self.nsq = self.n * self.n
        self.psq, self.qsq = p * p, q * q
        self.psq_inv = pow(self.psq, -1, self.qsq)
        self.lam = (p - 1) * (q - 1) // math.gcd(p - 1, q - 1)
        self.lam_inv = pow(self.lam, -1, self.n)
        self.n_inv_lam = pow(self.n, -1, self.lam)

    def pow_nsq(self, b, e):
        """b^e mod n^2 for a unit b and e >= 0"""
        xp = pow(b % self.psq, e % (self.p * (self.p - 1)), self.psq)
        xq = pow(b % self.qsq, e % (self.q * (self.q - 1)), self.qsq)
        return xp + self.psq * ((xq - xp) * self.psq_inv % self.qsq)

    def decrypt(self, c):
        return (self.pow_nsq(c, self.lam) - 1) // self.n * self.lam_inv % self.n

    def preimage_encrypt(self, t, check=False):
        """(m, r) with (1 + n m) r^n = t (mod n^2) for a unit t"""
        m = self.decrypt(t)
        r = pow(t % self.n, self.n_inv_lam, self.n)
        if check:
            assert (1 + self.n * m) * pow(r, self.n, self.nsq) % self.nsq == t
        return m, r

    def preimage_obfuscate(self, t, rng, pre=None, check=False):
        """(c_in, r) with c_in r^n = t: c_in is another encryption of t's plaintext (pre: preimage_encrypt(t), if at hand)"""
        m, r = pre or self.preimage_encrypt(t)
        s = random_unit(self.n, rng)
        c_in = (1 + self.n * m) * self.pow_nsq(s, self.n) % self.nsq
        r2 = r * pow(s, -1, self.n) % self.n
        if check:
            assert c_in * pow(r2, self.n, self.nsq) % self.nsq == t
        return c_in, r2

    def preimage_powmod(self, t, k, check=False):
        """base with base^k = t (mod n^2), for k coprime to n lambda"""
        base = self.pow_nsq(t, pow(k, -1, self.n * self.lam))
        if check:
            assert pow(base, k, self.nsq) == t
        return base

    def ciphertext_of(self, m, rng):
        return (1 + self.n * m) * self.pow_nsq(random_unit(self.n, rng), self.n) % self.nsq

    def coprime_exponent(self, k):
        while math.gcd(k, self.n * self.lam) != 1:
            k += 2
        return k


def first_mismatch(got, want, tags):
    for i, (g, w) in enumerate(zip(got, want)):
        if g != w:
            wrong = sum(1 for x, y in zip(got, want) if x != y)
            return "row %d (%s): %d of %d rows wrong" % (i, tags[i], wrong, len(want))
    return None if len(got) == len(want) else "row count %d != %d" % (len(got), len(want))


def thin(ts, k, keep=None):
    """at most k of the rows, evenly spaced; keep(t): a predicate of which a row that satisfies it and one that does not survive"""
    if len(ts) <= k:
        return list(ts)
    step = len(ts) / float(k)
    out = [ts[int(i * step)] for i in range(k)]
    if keep is not None:
        for want in (True, False):
            if not any(bool(keep(t)) == want for t, _ in out):
                out += [row for row in ts if bool(keep(row[0])) == want][:1]
    return out


def run_start(tag):
    """the lane a row's run starts at (EQ / ONES / ZERO rows), or None"""
    part = tag.split()
    return int(part[2].split("+")[0]) if len(part) > 2 and part[1] == "run" else None


def thin_cells(ts, arrives):
    """one row per (run start, borrow arrives or not): no run start and no borrow case of a start is lost; rows without a run start
    (NEAR, HALF) are all kept"""
    seen, out = set(), []
    for t, tag in ts:
        a = run_start(tag)
        cell = (a, bool(arrives(t)))
        if a is None or cell not in seen:
            seen.add(cell)
            out.append((t, tag))
    return out


def thin_decrypt_rows(rows, k, key):
    """decrypt_rows thinned to about k of the family rows ("m_p ..." / "u ..."); the named edge rows are ALL kept, and so are a
    row with m_q < m_p and one with m_q >= m_p (both branches of d = m_q - m_p (+ q))"""
    family = [r for r in rows if r[1].startswith(("m_p ", "u "))]
    edges = [r for r in rows if not r[1].startswith(("m_p ", "u "))]
    out = thin(family, k, lambda m: m % key.q < m % key.p) + edges
    assert any(m % key.q < m % key.p for m, _ in out) and any(m % key.q >= m % key.p for m, _ in out)
    assert len(edges) >= 7 and all(r in out for r in edges)
    return out


def random_unit(n, rng, below=None):
    while True:
        x = rng.randrange(2, below or n)
        if math.gcd(x, n) == 1:
            return x


def batch_layout(fam_rows, per, rng, ordinary, budget):
    """family rows -> one batch, a list of (t, tag), for a kernel whose wave holds `per` numbers (row i runs in group i mod per of its
    wave while the batch is a whole number of waves):
      whole      every family's rows, family after family, in whole waves (the last one filled up with the first rows again)
      one        waves of ordinary rows with ONE row of EQ / HALF, in every group position (per <= 8) or at the edges and the middle
      neighbour  consecutive groups holding a row whose run ends in M's top lane with a borrow, and a row whose run starts in lane 0
      ragged     11 more rows (per > 1): the last wave is not full
    ordinary(): a fresh ordinary target.  budget: rows the 'one' waves may take together (at least one wave)."""
    rows = [r for f in FAMILIES for r in fam_rows[f]]
    i = 0
    while len(rows) % per:                                     # (whole waves: the first rows again)
        rows.append((rows[i][0], rows[i][1] + " (again)"))
        i += 1
    special = [r for r in fam_rows["EQ"] if "borrow" in r[1]] + list(fam_rows["HALF"])
    places = list(range(per)) if per <= 8 else [0, 1, per // 2, per - 2, per - 1]
    places = places[:max(1, budget // per)]
    for j, pos in enumerate(places):
        wave = [(ordinary(), "ordinary") for _ in range(per)]
        t, tag = special[j % len(special)]
        wave[pos] = (t, "one@%d %s" % (pos, tag))
        rows += wave
    if per > 1:
        tops = [r for r in fam_rows["EQ"] if " top " in r[1]] or special
        lows = [r for r in fam_rows["EQ"] if r[1].startswith("EQ run 0+")] or special
        for j in range(min(per // 2, 4)):
            rows += [(tops[j % len(tops)][0], "neighbour-top " + tops[j % len(tops)][1]),
                     (lows[j % len(lows)][0], "neighbour-low " + lows[j % len(lows)][1])]
        while len(rows) % per:
            rows.append((ordinary(), "ordinary"))
        pool = [r for f in FAMILIES for r in fam_rows[f][:3]]
        rows += [(pool[(5 * j) % len(pool)][0], "ragged " + pool[(5 * j) % len(pool)][1]) for j in range(11)]
    return rows


def strong_probable_prime(n, a):
    d, s = n - 1, 0
    while d % 2 == 0:
        d, s = d // 2, s + 1
    x = pow(a, d, n)
    if x == 1 or x == n - 1:
        return True
    for _ in range(s - 1):
        x = x * x % n
        if x == n - 1:
            return True
    return False


def _prime(bits, rng):
    while True:
        x = rng.getrandbits(bits) | (1 << (bits - 1)) | 1
        if all(x % s for s in (3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37)) and all(strong_probable_prime(x, a) for a in (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37)):
            return x


def off_grid_key(key_bits):
    """(KeyMath, hp, hq) of a seeded key whose n has exactly key_bits bits (not a multiple of 32 or 29: n, p and q fill neither
    their rows of 32-bit words nor their rungs)"""
    import random
    rng = random.Random(8900 + key_bits)
    while True:
        p, q = sorted((_prime(key_bits // 2, rng), _prime(key_bits // 2, rng)))
        if p != q and (p * q).bit_length() == key_bits and math.gcd(p * q, (p - 1) * (q - 1)) == 1:
            break
    n = p * q
    hp = pow((pow(n + 1, p - 1, p * p) - 1) // p, -1, p)       # the reference's h_function
    hq = pow((pow(n + 1, q - 1, q * q) - 1) // q, -1, q)
    return KeyMath(p, q), hp, hq


def decrypt_rows(key, rng, count):
    """plaintexts m = m_p + p u chosen through the intermediates of the CRT tail (csrc/decrypt_tail.h, split_core.h
    decrypt_tail_wave_body): m_p and u laid out against p and q on the tail's lanes (one digit per lane up to ~1800-bit primes),
    x_p = c^(p-1) mod p^2 = 1 + p L_p with its low k digits zero (the borrow of x_p - 1 runs through k digits), u = 0, u = q - 1,
    m_q = m_p, m_q < m_p.  -> [(m, tag)]"""
    p, q = key.p, key.q
    nl = -(-(q.bit_length() + 4) // 29)
    q_inv_p = pow(q, -1, p)
    out = []
    for f in FAMILIES:
        mps = thin(family_targets(p, nl, 1, rng, f), count, lambda t: borrow_arrives(t, p, nl, 1))
        us = thin(family_targets(q, nl, 1, rng, f), count, lambda t: borrow_arrives(t, q, nl, 1))
        out += [(mp + p * rng.randrange(q), "m_p " + tag) for mp, tag in mps]
        out += [(rng.randrange(p) + p * u, "u " + tag) for u, tag in us]
    for k in sorted({1, 2, 5, max(1, nl - 2)}):
        W = 1 << (29 * k)
        if W >= p:
            continue
        lp = (-pow(p, -1, W)) % W + W * rng.randrange(p // W - 1)
        assert lp < p and (1 + p * lp) % W == 0
        mp = -lp * q_inv_p % p                               # x_p = (1 + n m)^(p-1) = 1 - p q m_p (mod p^2): L_p = -q m_p mod p
        out.append((mp + p * rng.randrange(q), "x_p = 0 mod W^%d" % k))
    small = rng.randrange(min(p, q))
    out += [(small, "u = 0, m_q = m_p"), (p - 1, "u = 0, m_p = p - 1"), (rng.randrange(p) + p * (q - 1), "u = q - 1"),
            (p - 1 + p * (q - 1), "m = n - 1"), (0, "m = 0"), (p, "m = p"), (q, "m = q")]
    below = [m for m, _ in out if m % q < m % p]
    assert below and len(below) < len(out)                   # both borrow branches of d = m_q - m_p (+ q), by construction
    return out
