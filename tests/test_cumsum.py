"""EncryptedVector.cumsum — running homomorphic sums — on a GPU-less box: the planner (phe/_engine.py plan_scan, pure numpy), the
public method on the emulator backend (which has no running-sum kernel: log-step doubling with the element-wise product) and the
device body itself (csrc/segment_core.h segment_scan_body) compiled for the CPU wave emulator.

Expected values are Python-integer running products modulo n^2 over the aligned ciphertexts — the reference's chain of
EncryptedNumber.__add__ = _raw_add (phe/paillier.py:705-719: mulmod(a, b, nsquare)), every prefix kept — never what the code
under test returns."""
import ctypes
import os
import random
import subprocess
import sys

import numpy as np
import pytest

from conftest import PKG, ROOT, load_golden

if PKG not in sys.path:
    sys.path.insert(0, PKG)

from phe import _engine, paillier  # noqa: E402

H = lambda s: int(s, 16)
NONE = 0xFFFFFFFF


# ---- the planner ------------------------------------------------------------------------------------------------------------
def walk(plan, cap):
    """the plan run on lists (a product is a concatenation, so the ORDER of the rows behind an output row shows too): down the
    levels the totals of every task, up again the scans from the carries.  Returns the list behind every output row."""
    inputs = [[[i] for i in range(plan.n_rows)]]
    for task_ptr, carry_idx, n_rows, seq_len in plan.levels:
        tp = task_ptr.astype(np.int64)
        tasks = len(tp) - 1
        assert task_ptr.dtype == np.uint64 and n_rows == len(inputs[-1]) and n_rows % seq_len == 0
        assert np.all(np.diff(tp) >= 0) and (tasks == 0 or (tp[0] == 0 and tp[-1] == n_rows))
        assert tasks == 0 or int(np.diff(tp).max()) <= cap                               # no task above the cap
        for t in range(tasks):
            if tp[t + 1] > tp[t]:
                assert tp[t] // seq_len == (tp[t + 1] - 1) // seq_len                    # no task crosses a sequence boundary
        if carry_idx is not None:
            assert carry_idx.dtype == np.uint32 and len(carry_idx) == tasks
            for t in range(tasks):
                first_of_sequence = tp[t] % seq_len == 0
                assert int(carry_idx[t]) == (NONE if first_of_sequence else t - 1)       # a sequence's first task: no carry
        inputs.append([sum(inputs[-1][tp[t]:tp[t + 1]], []) for t in range(tasks)])
    assert plan.levels[-1][1] is None                                                    # the last level scans without carries
    carry = None
    for (task_ptr, carry_idx, n_rows, _), rows in reversed(list(zip(plan.levels, inputs))):
        tp = task_ptr.astype(np.int64)
        out = [None] * n_rows
        for t in range(len(tp) - 1):
            acc = []
            if carry_idx is not None and int(carry_idx[t]) != NONE:
                acc = carry[int(carry_idx[t])]
            for r in range(tp[t], tp[t + 1]):
                acc = acc + rows[r]
                assert out[r] is None
                out[r] = acc
        assert all(o is not None for o in out)                                           # every row is owned by exactly one task
        carry = out
    return carry


def levels_for(longest, cap):
    """ceil(log_cap(longest)) in integers (at least the one level that makes the output rows)"""
    k, reach = 1, cap
    while reach < longest:
        k, reach = k + 1, reach * cap
    return k


@pytest.mark.parametrize("cap", [2, 4, 32])
def test_plan_gives_every_row_its_prefix(cap):
    for length in [0, 1, 2, cap - 1, cap, cap + 1, cap * cap, cap * cap + 1, 70]:
        # one sequence (block None and block = len), rows on their own, sequences of 5, and three sequences of `length`
        for n_rows, block in [(length, None), (length, length), (length, 1), (5 * length, 5), (3 * length, length)]:
            if block == 0:
                continue
            plan = _engine.plan_scan(n_rows, block, cap)
            seq = n_rows if block is None else block
            got = walk(plan, cap)
            assert got == [list(range(i - i % seq, i + 1)) for i in range(n_rows)], (n_rows, block)
            assert len(plan.levels) == levels_for(seq, cap), (n_rows, block)
            assert plan.n_rows == n_rows
            assert len(plan.levels[-1][0]) - 1 == (n_rows // seq if n_rows else 0)       # one task per sequence at the end


def test_plan_default_cap_is_the_module_constant(monkeypatch):
    monkeypatch.setattr(_engine, "SCAN_TASK_ROWS", 3)
    plan = _engine.plan_scan(10)
    assert len(plan.levels) == 3 and int(np.diff(plan.levels[0][0].astype(np.int64)).max()) <= 3
    assert walk(plan, 3) == [list(range(i + 1)) for i in range(10)]
    with pytest.raises(ValueError):
        _engine.plan_scan(10, None, 1)


# ---- the public method on the emulator backend (no running-sum kernel there: log-step doubling) ------------------------------
@pytest.fixture
def emu_keys(monkeypatch):
    import emu_backend
    emu_backend.install(monkeypatch)

    def make(bits):
        g = load_golden(bits)
        pub = paillier.PaillierPublicKey(H(g["n"]))
        return pub, paillier.PaillierPrivateKey(pub, H(g["p"]), H(g["q"]))
    return make


def integer_running_products(vec, block=None):
    """row i: the product of the ciphertexts (aligned to the smallest exponent) of its sequence up to i, modulo n^2, in Python
    integers"""
    n2 = vec.public_key.nsquare
    cs = vec.decrease_exponent_to(int(vec.exponent_array.min())).ciphertexts(False)
    block = len(cs) if block is None else block
    want, v = [], 1
    for i, c in enumerate(cs):
        v = c % n2 if i % block == 0 else v * c % n2
        want.append(v)
    return want


@pytest.mark.parametrize("bits", [256, 1024])
def test_api_on_the_emulator_backend(emu_keys, bits):
    pub, priv = emu_keys(bits)
    assert not pub._get_engine().has_segment_scan()
    rng = np.random.RandomState(bits)
    x = [float(v) for v in rng.randn(20)] + [int(v) for v in rng.randint(-50, 50, 20)]    # mixed exponents
    order = rng.permutation(40)
    x = [x[i] for i in order]
    vec = pub.encrypt_batch(x)
    assert len(set(vec.exponents)) > 1
    aligned = vec.decrease_exponent_to(min(vec.exponents))
    clear = np.array(x, dtype=float)
    for block in (None, 8, 1, 40):
        out = vec.cumsum(block) if block is not None else vec.cumsum()
        assert len(out) == 40 and not out.on_device
        assert set(out.exponents) == {min(vec.exponents)}
        assert not out._obfuscated.any()
        got = out.ciphertexts(False)
        assert got == integer_running_products(vec, block), block
        b = 40 if block is None else block
        for i in (0, 1, 7, 8, 23, 39):
            start = i - i % b
            assert aligned[start:i + 1].sum().ciphertext(False) == got[i], (block, i)
        dec = np.array(priv.decrypt_batch(out), dtype=float)
        assert np.allclose(dec, clear.reshape(-1, b).cumsum(axis=1).ravel(), rtol=0, atol=1e-9), block
    assert vec.cumsum(1).ciphertexts(False) == aligned.ciphertexts(False)                 # block = 1: the aligned rows
    assert vec.cumsum().ciphertexts(False)[0] == aligned.ciphertexts(False)[0]            # row 0: the aligned input row 0
    assert vec.cumsum(np.int64(8)).ciphertexts(False) == vec.cumsum(8).ciphertexts(False)


def test_api_errors_and_empty_vector(emu_keys):
    pub, _ = emu_keys(256)
    vec = pub.encrypt_batch(list(range(40)))
    with pytest.raises(ValueError):
        vec.cumsum(block=0)
    with pytest.raises(ValueError):
        vec.cumsum(block=-8)
    with pytest.raises(ValueError):
        vec.cumsum(block=7)                                                               # 40 rows are not blocks of 7
    with pytest.raises(TypeError):
        vec.cumsum(block=2.5)
    with pytest.raises(TypeError):
        vec.cumsum(block="8")
    empty = vec[:0].cumsum()
    assert len(empty) == 0 and empty.ciphertexts(False) == []
    assert len(vec[:0].cumsum(block=4)) == 0


# ---- the device body on the wave emulator -------------------------------------------------------------------------------------
EMU_DIR = os.path.join(ROOT, "tests", "emu")


def build_emu_lib(source, name):
    """tests/emu/<source> built beside libphe_emu.so (same flags as tests/emu/Makefile and the fixture of test_segment_sum.py)"""
    src, lib = os.path.join(EMU_DIR, source), os.path.join(EMU_DIR, name)
    csrc = os.path.join(PKG, "csrc")
    deps = [src, os.path.join(EMU_DIR, "wave_emu.h")] + [os.path.join(csrc, h) for h in
                                                         ("mont_core.h", "split_core.h", "segment_core.h", "key_setup.h")]
    if not os.path.exists(lib) or any(os.path.getmtime(d) > os.path.getmtime(lib) for d in deps):
        subprocess.check_call([os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra",
                               "-Wno-unused-parameter", "-Wno-unknown-pragmas", "-o", lib, src, "-lpthread"], cwd=EMU_DIR)
    return ctypes.CDLL(lib)


@pytest.fixture(scope="module")
def scan_lib():
    L = build_emu_lib("emu_scan.cpp", "libphe_emu_scan.so")
    L.emu_scan_last_error.restype = ctypes.c_char_p
    return L


@pytest.fixture(scope="module")
def seg_lib():
    L = build_emu_lib("emu_segment.cpp", "libphe_emu_seg.so")
    L.emu_seg_last_error.restype = ctypes.c_char_p
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


PATTERN = 0xA5C3F00F


# the geometries of test_segment_sum.py: rung 0 of each key, and the 8-lane rung that serves small batches of a 2048-bit key's rows
@pytest.mark.parametrize("bits, group, geometry", [(1024, 0, (2, 18)), (2048, 0, (4, 18)), (3072, 0, (4, 27)), (2048, 8, (8, 9))])
def test_device_body_on_the_wave_emulator(scan_lib, seg_lib, emu, bits, group, geometry):
    g = load_golden(bits)
    n = H(g["n"])
    n2, s1 = n * n, (n.bit_length() + 31) // 32
    n_arr = limbs([n], s1)[0]
    gl = (ctypes.c_int * 3)()
    assert scan_lib.emu_segment_scan(P(n_arr), s1, group, None, 0, ctypes.c_uint64(0), None, None, None, None, ctypes.c_uint64(0), 1,
                                     gl) == 0
    G, L, words = gl
    assert (G, L) == geometry and words == emu.pair_words(n_arr)
    per_wave = 64 // G
    rng = random.Random(bits + group)
    # every wave sees the lengths 0, 1, 2, 7 and 23 side by side; two waves stride over the tasks and the last round of the
    # second one is only partly filled
    pattern = [0, 1, 2, 7, 23]
    tasks = 2 * per_wave + per_wave + max(1, per_wave // 2)
    counts = [pattern[(t + t // per_wave) % 5] for t in range(tasks)]
    assert set(counts[:per_wave]) == set(pattern) and tasks % (2 * per_wave) != 0
    # rows 0, 1 and the last three belong to no task
    task_ptr = (2 + np.concatenate([[0], np.cumsum(counts)])).astype(np.uint64)
    n_rows = int(task_ptr[-1]) + 3
    # edge residues among random ones, inside the first tasks: 1, n^2 - 1, n, and a value above n^2 that still fits the words
    vals = [rng.randrange(1, n2) for _ in range(n_rows)]
    vals[2:6] = [1, n2 - 1, n, (1 << (64 * s1)) - 1]
    residues = limbs(vals, 2 * s1)
    pairs = emu.pair_op(n_arr, 0, residues)
    # carries: any row of the table, in any order, the pair of 1 among them, and every fifth task without one
    carry_vals = [1, n2 - 1] + [rng.randrange(1, n2) for _ in range(tasks - 2)]
    carry = emu.pair_op(n_arr, 0, limbs(carry_vals, 2 * s1))
    carry_idx = np.array([NONE if t % 5 == 4 else (7 * t + 3) % tasks for t in range(tasks)], np.uint32)
    carry_idx[3] = 0                                                                      # (the 7-row task of the first wave: from 1)

    def run(rows, is_pair, n_rows_, tp, cy, ci, n_tasks):
        out = np.full((n_rows_, words), PATTERN, np.uint32)
        rc = scan_lib.emu_segment_scan(P(n_arr), s1, group, P(rows), is_pair, ctypes.c_uint64(n_rows_), P(tp), P(cy), P(ci), P(out),
                                       ctypes.c_uint64(n_tasks), 2, None)
        assert rc == 0, scan_lib.emu_scan_last_error()
        return out

    def expected(tp, values, starts):
        want = {}
        for t in range(len(tp) - 1):
            v = starts[t]
            for r in range(int(tp[t]), int(tp[t + 1])):
                v = v * values[r] % n2
                want[r] = v
        return want

    def check(out, want):
        owned = sorted(want)
        assert ints(emu.pair_op(n_arr, 1, out[owned], group=group)) == [want[r] for r in owned]
        rest = np.setdiff1d(np.arange(out.shape[0]), owned)
        assert np.all(out[rest] == PATTERN)                                               # rows of no task: left as they were

    no_carry = expected(task_ptr, vals, [1] * tasks)
    with_carry = expected(task_ptr, vals, [1 if int(c) == NONE else carry_vals[int(c)] for c in carry_idx])
    assert len(no_carry) == sum(counts) == n_rows - 5
    for is_pair in (0, 1):
        rows = pairs if is_pair else residues
        check(run(rows, is_pair, n_rows, task_ptr, None, None, tasks), no_carry)
        check(run(rows, is_pair, n_rows, task_ptr, carry, None, tasks), no_carry)         # carry rows without numbers: from 1
        check(run(rows, is_pair, n_rows, task_ptr, carry, carry_idx, tasks), with_carry)

    # one full two-level scan by plan_scan: two sequences of 35 rows in tasks of at most 6 — the totals of the tasks by the
    # grouped-sum body, their scan, and the scan of the rows from those carries
    plan = _engine.plan_scan(70, 35, 6)
    assert len(plan.levels) == 2
    (tp0, ci0, rows0, _), (tp1, ci1, rows1, _) = plan.levels
    assert rows0 == 70 and ci0 is not None and ci1 is None and rows1 == len(tp0) - 1 == 12
    for is_pair in (0, 1):
        rows = (pairs if is_pair else residues)[2:72]
        totals = np.zeros((rows1, words), np.uint32)
        rc = seg_lib.emu_segment_reduce(P(n_arr), s1, group, P(rows), is_pair, ctypes.c_uint64(70), P(tp0), None, None, P(totals),
                                        ctypes.c_uint64(rows1), 2, None)
        assert rc == 0, seg_lib.emu_seg_last_error()
        carries = run(totals, 1, rows1, tp1, None, None, len(tp1) - 1)
        out = run(rows, is_pair, 70, tp0, carries, ci0, rows1)
        want, v = [], 1
        for i in range(70):
            v = vals[2 + i] % n2 if i % 35 == 0 else v * vals[2 + i] % n2
            want.append(v)
        assert ints(emu.pair_op(n_arr, 1, out, group=group)) == want
