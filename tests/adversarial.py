"""Adversarial operand pairs for every kernel that computes a*b mod N (TEST HELPER, not a conftest).

The product kernels of csrc/mul_tile.h and csrc/mul_table.h take floor(y / N) from a double-precision estimate, and
tile_settle_blocks resolves the carries between its column blocks with a generate / propagate look-ahead.  On random rows the
second-order carry branches fire about once in 2^27 rows, so random batches never execute them.  Here the RESULT t is chosen
first, then a is a random unit and b = t * a^-1 mod N: the kernel must return exactly t.  Residues whose digits in a column
block are all zero make that block carry out a second time (the look-ahead's `generate`), blocks of all-ones digits are its
`propagate`, residues next to 0 or N put the tile on the three-candidate path, residues around N * 2^-11 straddle the guard.

Geometry comes from the modulus (tile_shape mirrors key_setup.h build_table_mul / mul_tile.h TileShape), never from a kernel's
output: digits are 29 bits, a column block is CW digits, the workgroup has W blocks."""
import math

DIGIT = 29

# residues that keep the single-candidate (fast) path in a tile of their own; O1 / O2 fire nothing in the shipped kernel: pinned
FAST_FAMILIES = ("Z1", "Z2", "Z3", "Zall", "O1", "O2", "ZO")
FAMILIES = ("random",) + FAST_FAMILIES + ("Near", "Guard", "NearZ", "Wide")
LAYOUTS = ("whole", "one", "alternate", "ragged", "ragged_near")
ONE_ROW_LANES = (0, 1, 31, 32, 62, 63)


def tile_shape(modulus_bits):
    """(CW, W) of the tile kernel the library takes for a modulus N of this many bits (key_setup.h build_table_mul as phe_hip.hip
    calls it: the 8-wave shape first, lanes filled to within 16 columns); None where it offers no tiles"""
    need = -(-(modulus_bits + 38) // DIGIT)
    if 72 - 16 < need <= 72:
        return 9, 8
    for L in (9, 14):
        if 16 * L - 16 < need <= 16 * L:
            return L, 16
    return None


def _block_mask(CW, w, k=1):
    return ((1 << (DIGIT * CW * k)) - 1) << (DIGIT * CW * w)


def _inner_blocks(N, CW, W, k=1, clear=8):
    """first blocks w of runs w .. w + k - 1 that lie below the top `clear` bits of N: zeroing or filling them leaves a residue from
    the middle of [0, N) in the middle.  (At the golden widths the top block holds N's leading bits and is never in the list.)"""
    return [w for w in range(W) if DIGIT * CW * (w + k) <= N.bit_length() - clear]


def _mid(N, rng):
    return rng.randrange(N >> 1, N - (N >> 3))


def _near_values(N, CW, rng):
    small = [0, 1, 2, 3, rng.randrange(4, 1 << DIGIT), rng.randrange(1 << DIGIT, 1 << (DIGIT * CW))]
    return small + [N - x for x in small[1:]]


def _guard_values(N, rng, count):
    """floor(N 2^-e) + d and N - floor(N 2^-e) + d for e = 11 (the guard), 13 and 10; d spread over +- N 2^-(e+1): evenly where
    there are rows enough, drawn otherwise"""
    out = []
    steps = -(-count // 6)
    for i in range(count):
        e = (11, 13, 10)[i % 3]
        base, span = N >> e, N >> (e + 1)
        d = -span + 2 * span * (i // 6) // (steps - 1) if steps >= 3 else rng.randrange(-span, span + 1)
        out.append(base + d if (i // 3) % 2 == 0 else N - base + d)
    return out


def family_residues(N, CW, W, rng, family, count):
    """`count` residues t of one family (see the module docstring and each branch)"""
    out = []
    if family == "random":
        return [rng.randrange(N >> 4, N - (N >> 4)) for _ in range(count)]
    if family in ("Z1", "Z2", "Z3", "O1", "O2"):
        k = int(family[1])
        ws = _inner_blocks(N, CW, W, k)
        assert ws, family
        first = rng.randrange(len(ws))                        # (a single row is not always the lowest block)
        for i in range(count):
            m = _block_mask(CW, ws[(first + i) % len(ws)], k)
            out.append(_mid(N, rng) & ~m if family[0] == "Z" else _mid(N, rng) | m)
        return out
    if family == "Zall":                                      # blocks 1 .. the last one below N's leading bits: the carry runs into the top
        hi = _inner_blocks(N, CW, W)[-1]
        assert hi >= 1
        return [_mid(N, rng) & ~_block_mask(CW, 1, hi) for _ in range(count)]
    if family == "ZO":                                        # a zero block directly below an all-ones block, and the reverse
        ws = _inner_blocks(N, CW, W, 2)
        for i in range(count):
            w = ws[(i // 2) % len(ws)]
            z, o = (w, w + 1) if i % 2 == 0 else (w + 1, w)
            out.append((_mid(N, rng) & ~_block_mask(CW, z)) | _block_mask(CW, o))
        return out
    if family == "Near":
        while len(out) < count + 11:
            out += _near_values(N, CW, rng)
        first = rng.randrange(11)                             # (a single row is not always 0)
        return out[first:first + count]
    if family == "Guard":
        return _guard_values(N, rng, count)
    if family == "NearZ":                                     # next to 0 / N or at the guard, AND a zero block: the look-ahead inside
        ws = _inner_blocks(N, CW, W, 2, clear=24)             # the three-candidate loop
        guards = _guard_values(N, rng, count)
        for i in range(count):
            w = ws[(i // 4) % len(ws)]
            kind = i % 4
            if kind == 0:                                     # small: nothing above block w + 1, block w zero
                t = rng.randrange(1 << (DIGIT * CW * (w + 1)), 1 << (DIGIT * CW * (w + 2))) & ~_block_mask(CW, w)
            elif kind == 1:                                   # N - small with a zero block (and one with two)
                t = (N - 1 - rng.randrange(1 << DIGIT)) & ~_block_mask(CW, w, 1 + (i // 4) % 2)
            else:
                t = guards[i] & ~_block_mask(CW, w, 1 + (i // 4) % 2)
            out.append(t)
        return out
    raise ValueError(family)


def _unit(N, n_root, rng, below=None):
    while True:
        x = rng.randrange(2, below or N)
        if math.gcd(x, n_root) == 1:
            return x


def _batch_inverse(xs, N):
    """Montgomery's trick: one modular inverse and three products per element"""
    prefix = [1]
    for x in xs:
        prefix.append(prefix[-1] * x % N)
    inv = pow(prefix[-1], -1, N)
    out = [0] * len(xs)
    for i in range(len(xs) - 1, -1, -1):
        out[i] = inv * prefix[i] % N
        inv = inv * xs[i] % N
    return out


def pairs_for(ts, N, rng, n_root=None, wide=None, row_bits=None):
    """a, b with a * b = t (mod N) for every t of `ts`; a a random unit, b = t / a.  wide[i] (or None): 1 the chosen operand + the
    largest multiple of N that fits the row, 2 also the derived one, -1 / -2 the same with the operands swapped.  A row whose
    operand cannot be widened draws again (it is replaced, never dropped)."""
    n_root = n_root or N
    wide = wide or [0] * len(ts)
    top = (1 << row_bits) if row_bits else 0
    room = top - N if top else 0                              # x + N fits the row iff x < room
    xs = [_unit(N, n_root, rng, below=min(N, room) if wd and 0 < room else None) for wd in wide]
    ys = [t * ix % N for t, ix in zip(ts, _batch_inverse(xs, N))]
    a, b = [], []
    for i, (t, wd) in enumerate(zip(ts, wide)):
        x, y = xs[i], ys[i]
        if wd:
            assert room > 2, "rows no wider than the modulus hold no wide operand"
            tries = 0
            while abs(wd) == 2 and y >= room and tries < 64:  # the derived operand must fit too: another unit of the same family
                x = _unit(N, n_root, rng, below=min(N, room))
                y = t * pow(x, -1, N) % N
                tries += 1
            x += (top - 1 - x) // N * N
            if abs(wd) == 2 and y < room:
                y += (top - 1 - y) // N * N
            assert x >= N and x < top and y < top
        if wd < 0:
            x, y = y, x
        a.append(x)
        b.append(y)
    return a, b


def _wide_rows(N, CW, W, rng, count, row_bits):
    """operands that are not residues: x + k N with the largest k the row holds (the row's top bits set where N leaves room: the
    largest y, the estimate's widest input), one operand or both; the product is still congruent to the chosen t"""
    room = (1 << row_bits) - N
    both = room * 8 >= N                                      # a derived operand below `room` is likely enough to draw
    kinds = (1, -1, 2, -2) if both else (1, -1)
    fams = ("random", "Z2", "Near", "Zall", "Guard")
    ts = [family_residues(N, CW, W, rng, fams[i % len(fams)], 1)[0] for i in range(count)]
    return ts, [kinds[(i // len(fams)) % len(kinds)] for i in range(count)]


def adversarial_pairs(N, row_bits, CW, W, rng, layout="whole", families=FAMILIES, tiles_per_family=1, n_root=None):
    """-> (a, b, want, family): lists of Python integers and the family name of every row; a[i] * b[i] % N == want[i] (asserted by
    the callers on Python integers).  Tiles are 64 rows.
      whole        whole tiles of one family, `tiles_per_family` tiles each
      one          tiles of 63 random residues and ONE family row, at lanes 0, 1, 31, 32, 62, 63 (six tiles per family)
      alternate    tiles of a fast-only family with one Near row each (lane moving): the family's rows on the three-candidate path
      ragged       one tile of random residues and a last tile of 11 live rows, taken from `families` in turn (batch = 11 mod 64)
      ragged_near  63 + 11 rows of random residues whose LAST live row is a Near row: the lanes past the batch read it (the kernel
                   clamps the row index)"""
    ts, fam, wide = [], [], []

    def add(values, name, wd=None):
        ts.extend(values)
        fam.extend([name] * len(values))
        wide.extend(wd or [0] * len(values))

    def rows_of(family, count):
        if family == "Wide":
            return _wide_rows(N, CW, W, rng, count, row_bits)
        return family_residues(N, CW, W, rng, family, count), None

    if layout == "whole":
        for f in families:
            v, wd = rows_of(f, 64 * tiles_per_family)
            add(v, f, wd)
    elif layout == "one":
        for f in families:
            for lane in ONE_ROW_LANES:
                v, wd = rows_of(f, 1)
                add(family_residues(N, CW, W, rng, "random", lane), "random")
                add(v, f, wd)
                add(family_residues(N, CW, W, rng, "random", 63 - lane), "random")
    elif layout == "alternate":
        for i, f in enumerate(fm for fm in families if fm in FAST_FAMILIES):
            lane = ONE_ROW_LANES[i % len(ONE_ROW_LANES)]
            v = family_residues(N, CW, W, rng, f, 63)
            add(v[:lane], f)
            add(family_residues(N, CW, W, rng, "Near", i + 1)[-1:], "Near")
            add(v[lane:], f)
    elif layout == "ragged":
        add(family_residues(N, CW, W, rng, "random", 64), "random")
        for i in range(11):
            f = families[i % len(families)]
            v, wd = rows_of(f, i + 1)
            add(v[-1:], f, wd[-1:] if wd else None)
    elif layout == "ragged_near":
        add(family_residues(N, CW, W, rng, "random", 64 + 10), "random")
        add(family_residues(N, CW, W, rng, "Near", len(families) + 7)[-1:], "Near")
    else:
        raise ValueError(layout)
    a, b = pairs_for(ts, N, rng, n_root=n_root, wide=wide, row_bits=row_bits)
    return a, b, [t % N for t in ts], fam


def fill_batch(N, row_bits, CW, W, rng, rows, n_root=None):
    """exactly `rows` rows for a GPU batch: every family x tile layout once, then whole tiles of the families in turn up to the last
    whole tile, and a ragged last tile of family rows that ends on a Near row"""
    a, b, want, fam = [], [], [], []

    def take(part):
        for dst, src in zip((a, b, want, fam), part):
            dst.extend(src)

    for layout in ("whole", "one", "alternate"):
        take(adversarial_pairs(N, row_bits, CW, W, rng, layout, n_root=n_root))
    assert len(a) % 64 == 0 and len(a) <= rows, (len(a), rows)
    tail = rows % 64
    whole = (rows - tail - len(a)) // 64
    if whole:
        per = -(-whole // len(FAMILIES))
        part = adversarial_pairs(N, row_bits, CW, W, rng, "whole", tiles_per_family=per, n_root=n_root)
        take([v[:64 * whole] for v in part])
    if tail:                                                  # family rows in turn (Wide left out: no row width here), a Near row last
        fams = [f for f in FAMILIES if f not in ("random", "Wide")]
        ts, names = [], []
        for i in range(tail - 1):
            names.append(fams[i % len(fams)])
            ts.append(family_residues(N, CW, W, rng, names[-1], i + 1)[-1])
        names.append("Near")
        ts.append(family_residues(N, CW, W, rng, "Near", 2)[-1])
        pa, pb = pairs_for(ts, N, rng, n_root=n_root)
        take((pa, pb, ts, names))
    assert len(a) == len(b) == len(want) == len(fam) == rows
    return a, b, want, fam


def first_mismatch(got, want, fam):
    """None, or 'family / tile / lane' of the first row that differs — the only thing a failing test prints"""
    for i, (g, w) in enumerate(zip(got, want)):
        if g != w:
            wrong = sum(1 for x, y in zip(got, want) if x != y)
            return "%s / tile %d / lane %d (%d of %d rows wrong)" % (fam[i], i // 64, i % 64, wrong, len(want))
    return None if len(got) == len(want) else "row count %d != %d" % (len(got), len(want))


def extremal_moduli(key_bits, rng):
    """n of `key_bits` bits with the top limbs 0100...0 (2^(k-1) + small odd) and all ones (2^k - small odd): where the relative
    error of the estimate's 64-bit reciprocal and y / N are extreme.  Not products of two primes: the product kernels need none."""
    lo = (1 << (key_bits - 1)) + (rng.randrange(1 << 20) | 1)
    hi = (1 << key_bits) - (rng.randrange(1 << 20) | 1)
    return {"low": lo, "high": hi}
