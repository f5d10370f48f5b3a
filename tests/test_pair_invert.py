"""Inversion modulo n^2 on rows in the pair form — invert(c, n^2) of the negative-scalar branch of EncryptedNumber.__mul__
(phe/paillier.py:745-749) — on a GPU-less box: the device bodies (csrc/pair_invert.h) compiled for the CPU wave emulator, over
the library's own levels (invert_levels), and the host logic that picks the rows to invert (Engine._inverted_where_pair)
against a stub backend.

Expected values are Python integers: pow(c, -1, n^2) and products modulo n^2 — never another route of the code under test."""
import ctypes
import os
import random
import subprocess
import sys
import threading

import numpy as np
import pytest

from conftest import PKG, ROOT, load_golden

if PKG not in sys.path:
    sys.path.insert(0, PKG)

from phe import _engine  # noqa: E402
from phe._device import DeviceArray  # noqa: E402

H = lambda s: int(s, 16)
EMU_DIR = os.path.join(ROOT, "tests", "emu")
PATTERN = 0xA5C3F00F

# the geometries of test_cumsum.py: rung 0 of each key, and the 8-lane rung that serves small batches of a 2048-bit key's rows
GEOMETRIES = [(1024, 0, (2, 18)), (2048, 0, (4, 18)), (3072, 0, (4, 27)), (2048, 8, (8, 9))]


def build_emu_lib(source, name):
    """tests/emu/<source> built beside libphe_emu.so (same flags as tests/emu/Makefile and build_emu_lib of test_cumsum.py)"""
    src, lib = os.path.join(EMU_DIR, source), os.path.join(EMU_DIR, name)
    csrc = os.path.join(PKG, "csrc")
    deps = [src, os.path.join(EMU_DIR, "wave_emu.h")] + [os.path.join(csrc, h) for h in
                                                         ("mont_core.h", "split_core.h", "pair_invert.h", "key_setup.h")]
    if not os.path.exists(lib) or any(os.path.getmtime(d) > os.path.getmtime(lib) for d in deps):
        subprocess.check_call([os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra",
                               "-Wno-unused-parameter", "-Wno-unknown-pragmas", "-o", lib, src, "-lpthread"], cwd=EMU_DIR)
    return ctypes.CDLL(lib)


@pytest.fixture(scope="module")
def inv_lib():
    L = build_emu_lib("emu_invert.cpp", "libphe_emu_invert.so")
    L.emu_inv_last_error.restype = ctypes.c_char_p
    L.emu_inv_mad_count.restype = ctypes.c_uint64
    return L


@pytest.fixture(scope="module")
def emu():
    from emu_lib import Emu
    return Emu()


def limbs(xs, words):
    raw = b"".join(int(x).to_bytes(4 * words, "little") for x in xs)
    return np.frombuffer(raw, np.uint32).reshape(len(xs), words).copy()


def ints(arr):
    w = arr.shape[1] * 4
    raw = arr.tobytes()
    return [int.from_bytes(raw[i * w:(i + 1) * w], "little") for i in range(arr.shape[0])]


def P(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None else None


class Key:
    def __init__(self, inv_lib, emu, bits, group, geometry):
        g = load_golden(bits)
        self.n, self.p = H(g["n"]), H(g["p"])
        self.n2, self.s1 = self.n * self.n, (self.n.bit_length() + 31) // 32
        self.n_arr = limbs([self.n], self.s1)[0]
        self.lib, self.emu, self.group = inv_lib, emu, group
        gl = (ctypes.c_int * 3)()
        assert inv_lib.emu_inv_geometry(P(self.n_arr), self.s1, group, gl) == 0
        self.G, self.L, self.words = gl
        assert (self.G, self.L) == geometry and self.words == emu.pair_words(self.n_arr)

    def to_pair(self, values):
        return self.emu.pair_op(self.n_arr, 0, limbs(values, 2 * self.s1))

    def from_pair(self, rows):
        return ints(self.emu.pair_op(self.n_arr, 1, rows, group=self.group))

    def invert(self, pairs, block, waves=2):
        out = np.full(pairs.shape, PATTERN, np.uint32)
        bad, conv = ctypes.c_uint64(0xFFFFFFFF), ctypes.c_uint64(0)
        rc = self.lib.emu_pair_invert(P(self.n_arr), self.s1, self.group, P(pairs), P(out), ctypes.c_uint64(pairs.shape[0]), block,
                                      waves, ctypes.byref(bad), ctypes.byref(conv))
        assert rc in (0, 3), self.lib.emu_inv_last_error()
        self.conversion_mads = conv.value
        return (out, None) if rc == 0 else (None, bad.value)

    def units(self, rng, count):
        """random units modulo n^2 (a multiple of p or q among random residues has probability 2^-500)"""
        return [rng.randrange(2, self.n2) for _ in range(count)]


@pytest.fixture(scope="module")
def keys(inv_lib, emu):
    made = {}

    def get(bits, group, geometry):
        if (bits, group) not in made:
            made[(bits, group)] = Key(inv_lib, emu, bits, group, geometry)
        return made[(bits, group)]
    return get


# ---- the up walk alone ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits, group, geometry", GEOMETRIES)
@pytest.mark.parametrize("block", [2, 3, 16])
def test_up_walk_alone(keys, bits, group, geometry, block):
    """arbitrary X, arbitrary P (NOT the prefixes of X) and arbitrary Inv_up: row r of block t must be
    Inv_up[t] * prod_{j > r, j in the block} X[j] * P[r - 1], with P[first - 1] = 1 — the order of the walk, whatever the rest of
    the inversion does.  Two emulated waves, the second partly filled, the last block ragged with a single row; rows past the end
    keep a fill pattern."""
    k = keys(bits, group, geometry)
    per_wave = 64 // k.G
    blocks = per_wave + max(1, per_wave // 2)
    n_rows = (blocks - 1) * block + 1
    assert blocks % (2 * per_wave) != 0 and n_rows % block == 1
    rng = random.Random(1000 * bits + 10 * group + block)
    above = (1 << (64 * k.s1)) - 1                                                        # above n^2, still fits the words
    xv = [rng.randrange(1, k.n2) for _ in range(n_rows)]
    pv = [rng.randrange(1, k.n2) for _ in range(n_rows)]
    iv = [rng.randrange(1, k.n2) for _ in range(blocks)]
    xv[0:3] = [1, k.n2 - 1, above]                                                        # edge residues inside the first blocks
    pv[0:3] = [k.n2 - 1, above, 1]
    iv[0:3] = [above, 1, k.n2 - 1]
    x, p, inv = k.to_pair(xv), k.to_pair(pv), k.to_pair(iv)
    out = np.full((n_rows + 3, k.words), PATTERN, np.uint32)
    rc = k.lib.emu_pair_invert_walk(P(k.n_arr), k.s1, group, P(x), P(p), P(inv), P(out), ctypes.c_uint64(n_rows), block, 2)
    assert rc == 0, k.lib.emu_inv_last_error()
    want = []
    for t in range(blocks):
        first, last = t * block, min((t + 1) * block, n_rows)
        for r in range(first, last):
            v = iv[t]
            for j in range(r + 1, last):
                v = v * xv[j] % k.n2
            want.append(v * (pv[r - 1] if r > first else 1) % k.n2)
    assert k.from_pair(out[:n_rows]) == want
    assert np.all(out[n_rows:] == PATTERN)                                                # rows of no block: left as they were


# ---- the full inversion ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits, group, geometry", GEOMETRIES)
def test_full_inversion(keys, bits, group, geometry):
    """every row: X * out == 1 and out == pow(c, -1, n^2).  Blocks of 2 make the levels of 9 rows 9 -> 5 -> 3 -> 2 -> 1."""
    k = keys(bits, group, geometry)
    rng = random.Random(bits + group)
    values = k.units(rng, 70)
    values[0:3] = [1, k.n2 - 1, k.n + 1]
    pairs = k.to_pair(values)
    want = [pow(v, -1, k.n2) for v in values]
    for block, batches in ((2, (1, 2, 3, 9)), (16, (15, 16, 17, 70))):
        for batch in batches:
            out, bad = k.invert(pairs[:batch], block)
            assert bad is None, (block, batch)
            got = k.from_pair(out)
            assert all(v * o % k.n2 == 1 for v, o in zip(values, got)), (block, batch)
            assert got == want[:batch], (block, batch)


@pytest.mark.parametrize("bits, group, geometry", GEOMETRIES[:2])
def test_non_units_are_found(keys, bits, group, geometry):
    k = keys(bits, group, geometry)
    rng = random.Random(bits)
    values = k.units(rng, 9)
    values[3], values[6] = k.n, k.p * rng.randrange(2, k.n)
    for block in (2, 16):
        assert k.invert(k.to_pair(values), block) == (None, 3)
    values[3], values[2], values[5] = rng.randrange(2, k.n2), k.p * rng.randrange(2, k.n), k.n
    assert k.invert(k.to_pair(values), 2) == (None, 2)
    assert k.invert(k.to_pair(values[2:3]), 2) == (None, 0)                               # one row, no level at all


@pytest.mark.parametrize("bits, group, geometry", GEOMETRIES)
def test_three_products_per_row(keys, bits, group, geometry):
    """The multiply-adds of a whole inversion of 70 rows in blocks of 16, in the emulator's unit: the counter counts the
    lane-operations of WHOLE wavefronts (a limb group without a row multiplies by 1 in lock step), so one "pair product" here is
    one split_mul executed by a wavefront — measured by running one pair product through the same counter, never assumed.  One
    wavefront holds the 5 blocks of level 0 and the one block of level 1 (70 -> 5 -> 1 rows), so a level's cost in this unit is
    the steps of its walks.  The bound: 3 products per row over 70 + ceil(70 / 15) rows, plus the two conversions of the root
    (what the same counter saw between their start and their end; the inversion of ONE row is nothing else).  Below it, exactly:
    the first row of a block costs nothing in either walk, so a level costs 3 * (block_rows - 1) steps — a fourth product per row
    (totals by a second pass) cannot hide.  (The emulator libraries of one process share the counter: it is reset before every
    measured call, and the values are compared after the counts are taken.)"""
    k = keys(bits, group, geometry)
    rng = random.Random(7 * bits + group)
    values = k.units(rng, 70)
    pairs = k.to_pair(values)
    one = np.zeros((1, k.words), np.uint32)
    k.lib.emu_inv_mad_count(1)
    assert k.lib.emu_inv_pair_mul(P(k.n_arr), k.s1, group, P(pairs[:1]), P(pairs[1:2]), P(one), ctypes.c_uint64(1)) == 0
    product = int(k.lib.emu_inv_mad_count(1))
    out1, bad1 = k.invert(pairs[:1], 16, waves=1)
    assert int(k.lib.emu_inv_mad_count(1)) == k.conversion_mads > 0
    out, bad = k.invert(pairs, 16, waves=1)
    mads, conversions = int(k.lib.emu_inv_mad_count(1)), k.conversion_mads
    assert product > 0 and k.from_pair(one) == [values[0] * values[1] % k.n2]
    assert bad1 is None and k.from_pair(out1) == [pow(values[0], -1, k.n2)]
    assert bad is None and k.from_pair(out) == [pow(v, -1, k.n2) for v in values]
    assert mads <= 3 * (70 + -(-70 // 15)) * product + conversions
    assert mads == 3 * ((16 - 1) + (5 - 1)) * product + conversions


# ---- the host logic: which rows are inverted, and where a failure is reported --------------------------------------------------------
class StubBackend:
    """device memory as host arrays; "inversion" is the bitwise complement of a row, a row of zeros has no inverse"""

    def __init__(self):
        self.mem, self.next, self.calls = {}, 0x1000, []

    def malloc(self, nbytes):
        self.next += 0x1000
        self.mem[self.next] = np.zeros(nbytes, np.uint8)
        return self.next

    def free(self, ptr, nbytes):
        self.mem.pop(ptr, None)

    def h2d(self, ptr, arr):
        raw = np.ascontiguousarray(arr).view(np.uint8).ravel()
        self.mem[ptr][:raw.size] = raw

    def d2h(self, out, ptr):
        out.view(np.uint8).ravel()[:] = self.mem[ptr][:out.nbytes]

    def d2d(self, dst, src, nbytes):
        self.mem[dst][:nbytes] = self.mem[src][:nbytes]

    def sync(self):
        pass

    def rows(self, ptr, rows, limbs):
        return self.mem[ptr][:rows * limbs * 4].view(np.uint32).reshape(rows, limbs)

    def gather_rows_dev(self, src, src_rows, idx, dst, limbs, count):
        self.calls.append(("gather", count))
        self.rows(dst, count, limbs)[:] = self.rows(src, src_rows, limbs)[self.rows(idx, count, 1)[:, 0].astype(np.int64)]

    def scatter_rows_dev(self, src, idx, dst, dst_rows, limbs, count):
        self.calls.append(("scatter", count))
        self.rows(dst, dst_rows, limbs)[self.rows(idx, count, 1)[:, 0].astype(np.int64)] = self.rows(src, count, limbs)

    def select_rows_dev(self, a, b, mask, out, limbs, batch):
        self.calls.append(("select", batch))
        m = self.mem[mask][:batch].astype(bool)
        self.rows(out, batch, limbs)[:] = np.where(m[:, None], self.rows(b, batch, limbs), self.rows(a, batch, limbs))

    def pair_invert_dev(self, src, dst, batch, block_rows=0):
        self.calls.append(("invert", batch, block_rows))
        rows = self.rows(src, batch, self.words)
        dead = np.nonzero(~rows.any(axis=1))[0]
        if len(dead):
            err = ZeroDivisionError("invert() no inverse exists")
            err.bad_index = int(dead[0])
            raise err
        self.rows(dst, batch, self.words)[:] = ~rows


@pytest.fixture
def stub_engine():
    eng = object.__new__(_engine.Engine)                                                  # no native context behind it
    eng._lock = threading.RLock()
    eng.ctx = StubBackend()
    eng.ctx.words = 6
    return eng


def test_inverted_where_pair_picks_the_rows(stub_engine, monkeypatch):
    eng, ctx = stub_engine, stub_engine.ctx
    rs = np.random.RandomState(3)
    rows = rs.randint(1, 1 << 31, size=(40, 6)).astype(np.uint32)
    store = DeviceArray.from_host(ctx, rows)
    for negatives, route in (([5, 9], "gather"), ([0, 39], "gather"), (list(range(9)), "gather"), (list(range(10)), "select"),
                             (list(range(0, 40, 2)), "select"), (list(range(40)), "select")):
        neg = np.zeros(40, bool)
        neg[negatives] = True
        ctx.calls.clear()
        base = eng._inverted_where_pair(store, neg)
        assert base.ptr != store.ptr and np.array_equal(store.to_host(), rows)            # the input rows stay as they are
        assert np.array_equal(base.to_host(), np.where(neg[:, None], ~rows, rows)), negatives
        if route == "gather":                                                             # under a quarter: only those rows
            assert ctx.calls == [("gather", len(negatives)), ("invert", len(negatives), _engine.PAIR_INVERT_BLOCK_ROWS),
                                 ("scatter", len(negatives))]
        else:
            assert ctx.calls == [("invert", 40, _engine.PAIR_INVERT_BLOCK_ROWS), ("select", 40)]
    monkeypatch.setattr(_engine, "PAIR_INVERT_BLOCK_ROWS", 4)                             # the default block is the module constant
    ctx.calls.clear()
    eng.pair_invert_dev(store)
    eng.pair_invert_dev(store, block=7)
    assert ctx.calls == [("invert", 40, 4), ("invert", 40, 7)]


def test_inverted_where_pair_reports_the_callers_row(stub_engine):
    eng, ctx = stub_engine, stub_engine.ctx
    rows = np.arange(1, 241, dtype=np.uint32).reshape(40, 6)
    rows[5] = 0                                                                           # no inverse
    rows[9] = 0
    store = DeviceArray.from_host(ctx, rows)
    # (a quarter or more: the WHOLE vector is inverted, as _inverted_where does — its first row without an inverse is reported)
    for negatives, want in (([5, 9], 5), ([9], 9), ([3, 9, 20], 9), (list(range(40)), 5), (list(range(6, 40)), 5)):
        neg = np.zeros(40, bool)
        neg[negatives] = True
        with pytest.raises(ZeroDivisionError) as info:
            eng._inverted_where_pair(store, neg)
        assert info.value.bad_index == want, negatives


def test_the_default_block_is_one_figure():
    """the library's default (block_rows == 0 in phe_hip_pair_invert_dev) and the engine's PAIR_INVERT_BLOCK_ROWS are the same
    number, and the header says it"""
    import re
    with open(os.path.join(PKG, "csrc", "phe_hip.hip")) as f:
        in_library = re.search(r"constexpr uint32_t kPairInvertBlockRows = (\d+);", f.read())
    with open(os.path.join(ROOT, "include", "phe_hip.h")) as f:
        in_header = re.search(r"block_rows == 0: the library's default \((\d+)\)", f.read())
    assert in_library and in_header
    assert int(in_library.group(1)) == int(in_header.group(1)) == _engine.PAIR_INVERT_BLOCK_ROWS
