"""CPU tests of the quotient estimate and the carry look-ahead of the product kernels (csrc/mul_tile.h tile_settle_blocks,
csrc/mul_table.h, the staged Montgomery product) on the wave emulator, with operand pairs built so that the branches random rows
reach once in 2^27 rows run on EVERY row (tests/adversarial.py): the result t is chosen, a is a random unit, b = t / a; the
kernel must return exactly t.  The reference is Python integer arithmetic; every generated row is compared.

Which path a tile took is asserted, not assumed: the emulator counts multiply-adds (the single candidate of the settle against
three) and the non-zero generate / propagate words the look-ahead posts (wave_emu.h flag_counter — a count of the emulator's own,
the device compiles nothing of it).

That these tests can fail was checked with six mutants of the device headers, built for the emulator only on a separate copy of the tree (never
committed, never run on a device).  Wrong rows of a 64-row tile at 1024 / 2048 / 3072 bits, whole tiles unless said otherwise:
  (a) the single candidate's re-ripple ignores propagate       Z2 54 / 60 / 60, Z3 and Zall 64 / 64 / 64; random, Z1, O1, O2, ZO, Near, Guard: 0
  (b) the three-candidate look-ahead ignores propagate         Near 28 / 29 / 28, NearZ 36 / 38 / 38, Wide 33 / 30 / 35, Z2 + one Near row
                                                               54 / 59 / 60, Zall + one Near row 63 / 64 / 63
  (c) verdict bit 1 never set                                  Near 28 / 29 / 28, Wide 21 / 19 / 23, Zall + one Near row 63 / 64 / 63; NearZ aborts
                                                               (the emulator's PHE_BOUNDS: no candidate valid)
  (d) the guard widened to 0 < frac < 1                        the residues survive but for a row or two (the estimate is rarely wrong by a floor):
                                                               caught by the PATH assertions — every tile with a Near / NearZ row takes one
                                                               candidate — and by the direct drive at the guard
  (e) the quotient not lowered before the three candidates     Near, NearZ, Wide abort (PHE_BOUNDS: no candidate valid)
  (f) mul_table.h's estimate used without its - 1              table in LDS: Near 26 / 30, NearZ 16 / 16, Wide 5 / 8 (1024 / 2048 bits)
The tile and table tests of tests/test_emu_core.py as they stood before this file pass on (a), (d) and (f) — the coverage added here;
their tile of edge pairs already failed on (b) and aborted on (c) and (e)."""
import math
import random

import numpy as np
import pytest

import adversarial as adv
from conftest import load_golden
from emu_lib import Emu
from oracle.paillier_oracle import int_to_limbs, ints_to_limbs, limbs_to_ints

DIGIT = adv.DIGIT
SHAPES = {1024: (9, 8), 2048: (9, 16), 3072: (14, 16)}      # key bits -> (CW, W): mul_tile.h TileShape<9, 8>, <9, 16>, <14, 16>
GUARD = 2.0 ** -11                                          # tile_settle_blocks: one candidate iff every fraction keeps this far from 0 and 1
EST_ERR = 2.0 ** -12                                        # bound of the estimate's error (the comment above the guard in mul_tile.h)


@pytest.fixture(scope="module")
def emu():
    return Emu()


def golden_n(key_bits):
    return int(load_golden(key_bits)["n"], 16)


def moduli(key_bits):
    """(name, n, row words of n^2): the golden key, the two extremal moduli of its width, and for 2048 / 3072 bits a modulus off
    the limb grid (1920 / 3040 bits: fewer digits than columns, the top block partly or wholly empty)"""
    rng = random.Random(7 * key_bits)
    out = [("golden", golden_n(key_bits), key_bits // 16)]
    out += [(name, n, key_bits // 16) for name, n in adv.extremal_moduli(key_bits, rng).items()]
    off = {2048: 1920, 3072: 3040}.get(key_bits)
    if off:
        out.append(("off-grid", rng.getrandbits(off) | (1 << (off - 1)) | 1, -(-off // 128) * 8))
    return out


def run_tiles(emu, N, s2, a, b, W, blocks):
    out = emu.mulmod_table(int_to_limbs(N, s2), ints_to_limbs(a, s2), ints_to_limbs(b, s2), tiles=True, blocks=blocks, waves=W)
    assert out is not None
    return limbs_to_ints(out)


def sure_path(ts, N):
    """'slow' if some residue's t / N is surely inside the guard, 'fast' if all are surely outside, None where rounding decides
    (EST_ERR either side of the guard)"""
    fr = [min(t, N - t) / N for t in ts]
    if any(f < GUARD - EST_ERR for f in fr):
        return "slow"
    return "fast" if all(f > GUARD + EST_ERR for f in fr) else None


def special_blocks(t, CW, W, N):
    """(zero, ones): does t have a block w >= 1 of all-zero digits / a block of all-ones digits below N's leading bits"""
    zero = ones = False
    if t == 0:                                               # (b = 0: the product and the fold are 0, nothing carries anywhere)
        return zero, ones
    for w in range(W):
        if DIGIT * CW * (w + 1) > N.bit_length() - 8:
            break
        m = adv._block_mask(CW, w)
        zero |= w >= 1 and t & m == 0
        ones |= t & m == m
    return zero, ones


@pytest.mark.parametrize("blocks", [1, 2])
@pytest.mark.parametrize("key_bits", [1024, 2048, 3072])
def test_every_family_in_every_tile_layout_by_tiles(emu, key_bits, blocks):
    """mul_tile.h on all three tile shapes, one and two emulated workgroups, every modulus of moduli(): every residue family of
    tests/adversarial.py in every tile layout (whole tiles, one family row among 63 ordinary ones at lanes 0, 1, 31, 32, 62, 63,
    fast-only families with one Near row, ragged last tiles of family rows and with a Near row as the row the dead lanes read).
    Every row against the residue it was built for."""
    CW, W = SHAPES[key_bits]
    for name, n, s2 in moduli(key_bits):
        N = n * n
        assert adv.tile_shape(N.bit_length()) == (CW, W), name
        rng = random.Random(key_bits + 31 * blocks + len(name))
        for layout in adv.LAYOUTS:
            fams = adv.FAMILIES if name == "golden" or layout != "one" else ("Z2", "Zall", "Near", "Guard", "NearZ", "Wide")
            a, b, want, fam = adv.adversarial_pairs(N, 32 * s2, CW, W, rng, layout, families=fams, n_root=n)
            assert all(x * y % N == t for x, y, t in zip(a, b, want)) and max(max(a), max(b)) < 1 << (32 * s2)
            assert len(a) % 64 == (11 if layout.startswith("ragged") else 0)
            got = run_tiles(emu, N, s2, a, b, W, blocks)
            assert adv.first_mismatch(got, want, fam) is None, (name, layout, adv.first_mismatch(got, want, fam))


@pytest.mark.parametrize("key_bits", [1024, 2048, 3072])
def test_the_path_of_every_tile_and_the_look_ahead_are_what_the_rows_ask_for(emu, key_bits):
    """Branch execution, tile by tile (one emulated workgroup, one tile a call).  The multiply-adds per element are those of the
    single candidate (11,160 at 1024 bits: the count of record) where every residue is surely outside the guard, and 2 x 2 x S more —
    two further candidates of two multiply-adds a column — where one is surely inside; tiles that rounding decides (Guard) are run
    and compared but not asserted on.  The look-ahead's flag words: none on a single-candidate tile of ordinary residues, at least
    one per row with a zero block above block 0 (the block carries out a second time: generate) or an all-ones block (propagate)."""
    CW, W = SHAPES[key_bits]
    S = CW * W
    n = golden_n(key_bits)
    N, s2 = n * n, key_bits // 16
    rng = random.Random(key_bits + 5)
    emu.mad_count()
    a, b, want, fam = adv.adversarial_pairs(N, 32 * s2, CW, W, rng, "whole", families=("random",), n_root=n)
    assert run_tiles(emu, N, s2, a, b, W, 1) == want
    single = emu.mad_count() // 64
    assert key_bits != 1024 or single == 11160
    seen = {"fast": 0, "slow": 0, None: 0}
    fired = {}
    for layout in adv.LAYOUTS:
        a, b, want, fam = adv.adversarial_pairs(N, 32 * s2, CW, W, rng, layout, n_root=n)
        assert all(x * y % N == t for x, y, t in zip(a, b, want))
        for t0 in range(0, len(a), 64):
            rows = slice(t0, t0 + 64)
            emu.mad_count(), emu.flag_count()
            got = run_tiles(emu, N, s2, a[rows], b[rows], W, 1)
            mads, flags = emu.mad_count() // 64, emu.flag_count()
            where = (layout, t0 // 64, sorted(set(fam[rows])))
            assert adv.first_mismatch(got, want[rows], fam[rows]) is None, (where, adv.first_mismatch(got, want[rows], fam[rows]))
            path = sure_path(want[rows], N)
            seen[path] += 1
            assert mads in (single, single + 4 * S), where
            if path is not None:
                assert mads == (single if path == "fast" else single + 4 * S), (where, path)
            marks = [special_blocks(t, CW, W, N) for t in want[rows]]
            need = sum(1 for z, o in marks if z or o)
            assert flags >= need, (where, flags, need)
            if path == "fast" and need == 0:
                assert flags == 0, (where, flags)
            for f in set(fam[rows]) - {"random"}:
                fired[f] = fired.get(f, 0) + flags
    assert seen["fast"] >= 20 and seen["slow"] >= 20, seen
    assert all(fired[f] > 0 for f in ("Z1", "Z2", "Z3", "Zall", "ZO", "O1", "O2", "NearZ")), fired


@pytest.mark.parametrize("key_bits", [1024, 2048])
def test_near_guard_and_wide_rows_through_the_table_in_lds_and_the_staged_product(emu, key_bits):
    """mul_table.h (the table in LDS: floor(estimate) - 1, then conditional subtractions) and the staged Montgomery product
    (mul_io.h / mont_core.h: emu.mulmod) on the residues next to a multiple of N, around the guard, and on operands above N — where an
    estimate used one too high or a missed final subtraction shows.  Golden key and extremal moduli; every row."""
    CW, W = SHAPES[key_bits]
    for name, n, s2 in moduli(key_bits)[:3]:
        N = n * n
        rng = random.Random(key_bits + 77 + len(name))
        a, b, want, fam = adv.adversarial_pairs(N, 32 * s2, CW, W, rng, "whole", families=("Near", "Guard", "NearZ", "Wide", "Zall"), n_root=n)
        a2, b2, want2, fam2 = adv.adversarial_pairs(N, 32 * s2, CW, W, rng, "ragged_near", n_root=n)
        a, b, want, fam = a + a2, b + b2, want + want2, fam + fam2
        assert all(x * y % N == t for x, y, t in zip(a, b, want))
        Nl, al, bl = int_to_limbs(N, s2), ints_to_limbs(a, s2), ints_to_limbs(b, s2)
        in_lds = emu.mulmod_table(Nl, al, bl)
        assert in_lds is not None
        assert adv.first_mismatch(limbs_to_ints(in_lds), want, fam) is None, (name, adv.first_mismatch(limbs_to_ints(in_lds), want, fam))
        staged = limbs_to_ints(emu.mulmod(Nl, al, bl))
        assert adv.first_mismatch(staged, want, fam) is None, (name, adv.first_mismatch(staged, want, fam))


# ---- tile_settle_blocks on its own: fold results that no product reaches ------------------------------------------------------------

class Settle:
    """One modulus on one tile shape: splits an integer y into the digits and block carries tile_settle_blocks takes, predicts its
    quotient estimate with the kernel's own sequence of double-precision operations (Python floats are IEEE doubles and nothing
    is contracted on the host), and runs the emulator."""

    def __init__(self, emu, N, s2, CW, W):
        self.emu, self.N, self.s2, self.CW, self.W, self.S = emu, N, s2, CW, W, CW * W
        self.Nl = int_to_limbs(N, s2)
        info = emu.table_mul_info(self.Nl, W)
        assert info is not None and info["S"] == self.S and info["L"] == CW
        self.base, self.inv, self.P = info["base"], info["inv"], info["split"]
        self.wb = -(-self.base // CW)                          # first block that starts at or above limb `base`
        self.off = self.wb * CW - self.base

    def split(self, Y, carries):
        """digits of Y - sum_w carries[w] W^(CW (w + 1)) (the carries are shrunk from the top until that is not negative)"""
        carries = list(carries) + [0] * (self.W - len(carries))
        carries[self.W - 1] = 0                                # (nothing leaves the top block: y < W^S)
        weight = lambda w: 1 << (DIGIT * self.CW * (w + 1))
        rest = Y - sum(c * weight(w) for w, c in enumerate(carries))
        for w in range(self.W - 2, -1, -1):
            if rest >= 0:
                break
            rest += carries[w] * weight(w)
            carries[w] = 0
        assert 0 <= rest < 1 << (DIGIT * self.S) and all(0 <= c < 1 << 38 for c in carries)
        return [(rest >> (DIGIT * k)) & ((1 << DIGIT) - 1) for k in range(self.S)], carries

    def estimate(self, y, carries):
        """(qd, frac) as tile_settle_blocks computes them"""
        e = [float(y[self.base + i]) for i in range(4)]
        yd = (e[3] * 536870912.0 + e[2]) * 288230376151711744.0 + (e[1] * 536870912.0 + e[0])
        if 1 <= self.wb < self.W and self.off <= 3:
            yd += float(carries[self.wb - 1]) * float(1 << (DIGIT * self.off))
        qe = yd * self.inv
        qd = math.floor(qe)
        return qd, qe - qd

    def takes_one_candidate(self, y, carries):
        qd, frac = self.estimate(y, carries)
        return qd >= 1.0 and 0.00048828125 < frac < 0.99951171875

    def run(self, rows):
        """rows: [(y digits, carries)] of one tile -> (residues, multiply-adds per lane, flag words)"""
        self.emu.mad_count(), self.emu.flag_count()
        out = self.emu.settle_blocks(self.Nl, np.array([y for y, _ in rows], np.uint32), np.array([c for _, c in rows], np.uint64), self.W)
        assert out is not None
        return limbs_to_ints(out), self.emu.mad_count() // 64, self.emu.flag_count()


def settle_cases(key_bits):
    CW, W = SHAPES[key_bits]
    for name, n, s2 in moduli(key_bits):
        yield name, n * n, s2, CW, W


MAXC = (1 << 38) - 1                                         # the largest block carry the settle's comment allows
MAXQ = (1 << 38) - 1                                         # y / N just under 2^38: the largest quotient


@pytest.mark.parametrize("key_bits", [1024, 2048, 3072])
def test_settle_alone_on_crafted_digits_carries_and_quotients(emu, key_bits):
    """tile_settle_blocks driven directly (emu_settle_blocks): y = q N + t handed over as digits and block carries, the reference
    y mod N = t on Python integers from the digits passed in.  Quotients 0 (y < N: the estimate's floor is 0), 1, 2^38 - 1 (the
    documented maximum) and in between; block carries 0, 2^38 - 1 in every block, and random ones; residues with zero blocks (a
    block of all ones above a block that carries out, a carry into the top block), all-ones blocks, next to 0 and N.  Whole tiles of
    64, the path of the tile as the kernel's own estimate (repeated here on IEEE doubles) decides it."""
    for name, N, s2, CW, W in settle_cases(key_bits):
        st = Settle(emu, N, s2, CW, W)
        rng = random.Random(key_bits + 3 * len(name))
        fams = ("random", "Z2", "Zall", "ZO", "O2", "Near", "NearZ", "Guard")
        for q_kind in ("zero", "one", "mid", "max"):
            for c_kind in ("none", "max", "random"):
                ts, fam = [], []
                for f in fams:
                    v = adv.family_residues(N, CW, W, rng, f, 8)
                    ts += v
                    fam += [f] * len(v)
                rows, want = [], []
                for t in ts:
                    q = {"zero": 0, "one": 1, "mid": rng.randrange(2, MAXQ), "max": MAXQ}[q_kind]
                    Y = q * N + t
                    cs = {"none": [0] * W, "max": [MAXC] * W, "random": [rng.randrange(MAXC + 1) for _ in range(W)]}[c_kind]
                    y, cs = st.split(Y, cs)
                    assert sum(d << (DIGIT * k) for k, d in enumerate(y)) + sum(c << (DIGIT * CW * (w + 1)) for w, c in enumerate(cs)) == Y
                    rows.append((y, cs))
                    want.append(Y % N)
                assert want == ts
                got, mads, flags = st.run(rows)
                where = (name, q_kind, c_kind)
                assert adv.first_mismatch(got, want, fam) is None, (where, adv.first_mismatch(got, want, fam))
                one = all(st.takes_one_candidate(y, cs) for y, cs in rows)
                assert not one, where                         # (the Near rows)
                assert mads == 3 * 2 * st.S, (where, mads)
                assert flags > 0, where
                # the same rows without the ones next to 0, N and the guard: the single candidate (the estimate's floor is taken as it is)
                keep = [i for i, f in enumerate(fam) if f not in ("Near", "NearZ", "Guard")]
                rows2 = [rows[i] for i in keep]
                got, mads, flags = st.run(rows2)
                assert adv.first_mismatch(got, [want[i] for i in keep], [fam[i] for i in keep]) is None, where
                one = all(st.takes_one_candidate(y, cs) for y, cs in rows2)
                assert one == (q_kind != "zero"), where       # (qd = 0: three candidates whatever the fraction)
                assert mads == (2 * st.S if one else 3 * 2 * st.S), (where, mads)
                assert flags > 0, where


@pytest.mark.parametrize("key_bits", [1024, 2048, 3072])
def test_settle_alone_within_a_few_ulp_of_the_guard(emu, key_bits):
    """The fraction of the estimate within a few steps of 2^-11 and of 1 - 2^-11, found by bisection on the kernel's own double
    arithmetic: y moves by W^base (the lowest limb the estimate reads) from the last y that takes three candidates to the first
    that takes one.  Either side the residue is y mod N, and the path is the one the fraction asks for — for a small quotient
    (fraction steps of ~2^-52) and for one near 2^37 (steps of 2^-15), without a carry among the estimate's limbs and with one."""
    for name, N, s2, CW, W in settle_cases(key_bits):
        st = Settle(emu, N, s2, CW, W)
        rng = random.Random(key_bits + 9 * len(name))
        step = 1 << (DIGIT * st.base)
        for q in (1, 5, (1 << 37) + rng.randrange(1 << 30)):
            for side in ("low", "high"):
                for with_carry in (False, True):
                    def rows_at(d):
                        Y = q * N + ((N >> 11) if side == "low" else N - (N >> 11)) + d * step
                        cs = [0] * W
                        if with_carry and st.wb >= 1:
                            cs[st.wb - 1] = MAXC if q > 5 else 1
                        return Y, st.split(Y, cs)
                    span = max(4, (N >> 13) // step)
                    lo, hi = -span, span                      # takes_one_candidate: low side False -> True, high side True -> False
                    first = st.takes_one_candidate(*rows_at(lo)[1])
                    assert first == (side == "high") and st.takes_one_candidate(*rows_at(hi)[1]) != first, (name, q, side)
                    while hi - lo > 1:
                        mid = (lo + hi) // 2
                        if st.takes_one_candidate(*rows_at(mid)[1]) == first:
                            lo = mid
                        else:
                            hi = mid
                    for d in range(lo - 2, hi + 3):
                        Y, row = rows_at(d)
                        got, mads, _ = st.run([row])           # a tile of one live row: the dead lanes repeat it
                        where = (name, q, side, with_carry, d - lo)
                        assert got == [Y % N], where
                        assert mads == (2 * st.S if st.takes_one_candidate(*row) else 3 * 2 * st.S), where
