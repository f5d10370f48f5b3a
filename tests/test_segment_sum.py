"""EncryptedVector.segment_sum — grouped homomorphic sums — on a GPU-less box: the planner (phe/_engine.py plan_segments, pure
numpy), the public method on the emulator backend (which has no grouped-sum kernel: the route of rounds of element-wise products)
and the device body itself (csrc/segment_core.h segment_reduce_body) compiled for the CPU wave emulator.

Expected values are Python-integer products of the members modulo n^2 — per group the reference's chain of
EncryptedNumber.__add__ = _raw_add (phe/paillier.py:705-719: mulmod(a, b, nsquare)) — never what the code under test returns."""
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


# ---- the planner ------------------------------------------------------------------------------------------------------------
def walk(plan, n_rows):
    """the multiset of vector rows behind every output row, by running the plan on lists"""
    cur = None
    for level, (task_ptr, idx, order) in enumerate(plan.levels):
        tp = task_ptr.astype(np.int64)
        assert tp[0] == 0 and np.all(np.diff(tp) >= 0)
        assert sorted(order.tolist()) == list(range(len(tp) - 1))                       # a permutation of the tasks
        lengths = np.diff(tp)
        assert np.all(np.diff(lengths[order]) <= 0)                                      # longest first
        if level == 0:
            assert idx is not None and idx.dtype == np.uint32 and len(idx) == tp[-1]
            assert idx.size == 0 or int(idx.max()) < n_rows
            cur = [sorted(idx[tp[t]:tp[t + 1]].tolist()) for t in range(len(tp) - 1)]
        else:
            assert idx is None and tp[-1] == len(cur)                                    # every partial is taken exactly once
            cur = [sorted(sum(cur[tp[t]:tp[t + 1]], [])) for t in range(len(tp) - 1)]
    return cur


def levels_for(longest, cap):
    """ceil(log_cap(longest)) in integers (at least the one level that makes the output rows)"""
    k, reach = 1, cap
    while reach < longest:
        k, reach = k + 1, reach * cap
    return k


@pytest.mark.parametrize("cap", [2, 4, 32])
def test_plan_partitions_every_segment_once(cap):
    rng = np.random.RandomState(cap)
    sizes = [0, 1, 2, 3, cap - 1, cap, cap + 1, 2 * cap, cap * cap, cap * cap + 1, 70, 0]
    ids = np.repeat(np.arange(len(sizes)), sizes)
    ids = np.concatenate([ids, np.full(9, -1)])                                          # rows left out
    rng.shuffle(ids)
    plan = _engine.plan_segments(ids, len(sizes), cap)
    assert plan.n_out == len(sizes)
    for task_ptr, _, _ in plan.levels:
        assert int(np.diff(task_ptr.astype(np.int64)).max()) <= cap                      # no task above the cap
    got = walk(plan, len(ids))
    assert got == [sorted(np.nonzero(ids == s)[0].tolist()) for s in range(len(sizes))]
    assert got[0] == [] and got[-1] == [] and len(got[1]) == 1                           # empty and single-row segments
    assert len(plan.levels) == levels_for(max(sizes), cap)
    assert len(plan.levels[-1][2]) == len(sizes)                                         # one task per segment at the end


@pytest.mark.parametrize("longest, cap", [(1, 4), (4, 4), (5, 4), (16, 4), (17, 4), (64, 4), (65, 4), (70, 4), (33, 32), (1025, 32)])
def test_plan_level_count_is_the_logarithm(longest, cap):
    plan = _engine.plan_segments(np.zeros(longest, np.int64), 1, cap)
    assert len(plan.levels) == levels_for(longest, cap)
    assert walk(plan, longest) == [list(range(longest))]


def test_plan_default_cap_is_the_module_constant(monkeypatch):
    monkeypatch.setattr(_engine, "SEGMENT_TASK_ROWS", 3)
    plan = _engine.plan_segments(np.zeros(10, np.int64), 1)
    assert len(plan.levels) == 3 and int(np.diff(plan.levels[0][0].astype(np.int64)).max()) <= 3


def test_plan_two_dimensional_ids():
    """(F, rows) ids: output row f * n_segments + s, every grouping over the same rows"""
    rng = np.random.RandomState(5)
    ids = rng.randint(-1, 4, size=(3, 50))
    plan = _engine.plan_segments(ids, 4, 4)
    assert plan.n_out == 12
    got = walk(plan, 50)
    assert got == [sorted(np.nonzero(ids[f] == s)[0].tolist()) for f in range(3) for s in range(4)]


def test_plan_without_rows_or_segments():
    plan = _engine.plan_segments(np.zeros(0, np.int64), 3, 4)
    assert plan.n_out == 3 and len(plan.levels) == 1 and walk(plan, 0) == [[], [], []]
    plan = _engine.plan_segments(np.full(5, -1), 0, 4)
    assert plan.n_out == 0 and len(plan.levels[0][2]) == 0


# ---- the public method on the emulator backend (no grouped-sum kernel there: rounds of element-wise products) ----------------
@pytest.fixture
def emu_keys(monkeypatch):
    import emu_backend
    emu_backend.install(monkeypatch)

    def make(bits):
        g = load_golden(bits)
        pub = paillier.PaillierPublicKey(H(g["n"]))
        return pub, paillier.PaillierPrivateKey(pub, H(g["p"]), H(g["q"]))
    return make


def integer_products(vec, ids, num_segments):
    """per segment the product of the members' ciphertexts (aligned to the smallest exponent) modulo n^2, in Python integers"""
    n2 = vec.public_key.nsquare
    aligned = vec.decrease_exponent_to(int(vec.exponent_array.min()))
    cs = aligned.ciphertexts(False)
    want = []
    for row in np.atleast_2d(ids):
        for s in range(num_segments):
            v = 1
            for i in np.nonzero(row == s)[0]:
                v = v * cs[int(i)] % n2
            want.append(v)
    return want


@pytest.mark.parametrize("bits", [256, 1024])
def test_api_on_the_emulator_backend(emu_keys, bits):
    pub, priv = emu_keys(bits)
    rng = np.random.RandomState(bits)
    x = [float(v) for v in rng.randn(20)] + [int(v) for v in rng.randint(-50, 50, 20)]    # mixed exponents
    vec = pub.encrypt_batch(x)
    assert len(set(vec.exponents)) > 1
    ids = rng.randint(-1, 6, 40)
    ids[ids == 3] = 2                                                                     # segment 3 stays empty, 6 too
    out = vec.segment_sum(ids, 7)
    assert len(out) == 7 and not out.on_device
    assert set(out.exponents) == {min(vec.exponents)}
    want = integer_products(vec, ids, 7)
    assert out.ciphertexts(False) == want
    assert want[3] == 1 and want[6] == 1                                                  # no members: the ciphertext 1
    aligned = vec.decrease_exponent_to(min(vec.exponents))
    for s in (0, 1, 2, 4, 5):
        members = np.nonzero(ids == s)[0]
        assert len(members)
        assert aligned[members].sum().ciphertext(False) == out.ciphertexts(False)[s]
    used = ids >= 0
    dec = np.array(priv.decrypt_batch(out), dtype=float)
    assert np.allclose(dec, np.bincount(ids[used], weights=np.array(x, dtype=float)[used], minlength=7), rtol=0, atol=1e-9)
    assert vec.segment_sum(ids).ciphertexts(False) == want[:int(ids.max()) + 1]           # num_segments defaults to max + 1
    # the histogram form
    ids2 = np.stack([ids, rng.randint(0, 7, 40), np.full(40, -1)])
    out2 = vec.segment_sum(ids2, 7)
    assert len(out2) == 21 and out2.ciphertexts(False) == integer_products(vec, ids2, 7)
    assert out2.ciphertexts(False)[14:] == [1] * 7


def test_api_errors_and_empty_vector(emu_keys):
    pub, _ = emu_keys(256)
    vec = pub.encrypt_batch([1, 2, 3])
    with pytest.raises(ValueError):
        vec.segment_sum([0, 1, 2], 2)                                                     # 2 is outside [0, 2)
    with pytest.raises(ValueError):
        vec.segment_sum([0, -2, 1])
    with pytest.raises(ValueError):
        vec.segment_sum([0, 1])                                                           # one id per row
    with pytest.raises(ValueError):
        vec.segment_sum(np.zeros((2, 2), int))
    with pytest.raises(ValueError):
        vec.segment_sum([0, 0, 0], -1)
    with pytest.raises(TypeError):
        vec.segment_sum([0.0, 1.0, 2.0])
    empty = vec[:0].segment_sum([], 3)
    assert len(empty) == 3 and empty.ciphertexts(False) == [1, 1, 1]
    assert len(vec.segment_sum([-1, -1, -1])) == 0


# ---- the device body on the wave emulator -------------------------------------------------------------------------------------
EMU_DIR = os.path.join(ROOT, "tests", "emu")


@pytest.fixture(scope="module")
def seg_lib():
    """tests/emu/emu_segment.cpp built beside libphe_emu.so (same flags as tests/emu/Makefile)"""
    src, lib = os.path.join(EMU_DIR, "emu_segment.cpp"), os.path.join(EMU_DIR, "libphe_emu_seg.so")
    csrc = os.path.join(PKG, "csrc")
    deps = [src, os.path.join(EMU_DIR, "wave_emu.h")] + [os.path.join(csrc, h) for h in
                                                         ("mont_core.h", "split_core.h", "segment_core.h", "key_setup.h")]
    if not os.path.exists(lib) or any(os.path.getmtime(d) > os.path.getmtime(lib) for d in deps):
        subprocess.check_call([os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra",
                               "-Wno-unused-parameter", "-Wno-unknown-pragmas", "-o", lib, src, "-lpthread"], cwd=EMU_DIR)
    L = ctypes.CDLL(lib)
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


# the rung of every group size the golden keys select: rung 0 of each key, and the 8-lane rung that serves small batches of
# a 2048-bit key's rows (the 16- and 64-lane rungs of these keys have other limb counts: no pair rows for them)
@pytest.mark.parametrize("bits, group, geometry", [(1024, 0, (2, 18)), (2048, 0, (4, 18)), (3072, 0, (4, 27)), (2048, 8, (8, 9))])
def test_device_body_on_the_wave_emulator(seg_lib, emu, bits, group, geometry):
    g = load_golden(bits)
    n = H(g["n"])
    n2, s1 = n * n, (n.bit_length() + 31) // 32
    n_arr = limbs([n], s1)[0]
    gl = (ctypes.c_int * 3)()
    assert seg_lib.emu_segment_reduce(P(n_arr), s1, group, None, 0, ctypes.c_uint64(0), None, None, None, None, ctypes.c_uint64(0), 1,
                                      gl) == 0
    G, L, words = gl
    assert (G, L) == geometry and words == emu.pair_words(n_arr)
    per_wave = 64 // G
    rng = random.Random(bits + group)
    long_one = 23
    # every wave sees the lengths 0, 1, 2, 7 and a much longer one side by side; two waves stride over the tasks and the last
    # round of the second one is only partly filled
    pattern = [0, 1, 2, 7, long_one]
    tasks = 2 * per_wave + per_wave + max(1, per_wave // 2)
    counts = [pattern[(t + t // per_wave) % 5] for t in range(tasks)]
    assert set(counts[:per_wave]) == set(pattern) and tasks % (2 * per_wave) != 0
    n_rows = 29
    # edge residues among random ones: 1, n^2 - 1, n, and a value above n^2 that still fits the words
    vals = [1, n2 - 1, n, (1 << (64 * s1)) - 1] + [rng.randrange(1, n2) for _ in range(n_rows - 4)]
    residues = limbs(vals, 2 * s1)
    pairs = emu.pair_op(n_arr, 0, residues)
    task_ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    idx = np.array([rng.randrange(n_rows) for _ in range(int(task_ptr[-1]))], np.uint32)
    order = np.argsort(-np.array(counts), kind="stable").astype(np.uint32)

    def run(rows, is_pair, n_rows_, tp, ix, od, n_tasks):
        out = np.zeros((n_tasks, words), np.uint32)
        rc = seg_lib.emu_segment_reduce(P(n_arr), s1, group, P(rows), is_pair, ctypes.c_uint64(n_rows_), P(tp), P(ix), P(od), P(out),
                                        ctypes.c_uint64(n_tasks), 2, None)
        assert rc == 0, seg_lib.emu_seg_last_error()
        return out

    def products(rows_of_task, values):
        want = []
        for members in rows_of_task:
            v = 1
            for k in members:
                v = v * values[int(k)] % n2
            want.append(v)
        return want

    want = products([idx[int(task_ptr[t]):int(task_ptr[t + 1])] for t in range(tasks)], vals)
    assert want.count(1) >= counts.count(0)                                               # an empty task: the pair of 1
    partial = None
    for is_pair in (0, 1):
        for od in (None, order):
            out = run(pairs if is_pair else residues, is_pair, n_rows, task_ptr, idx, od, tasks)
            assert ints(emu.pair_op(n_arr, 1, out, group=group)) == want, (is_pair, od is not None)
            partial = out
    # idx == NULL: runs of the partial products themselves (the later levels), with and without an order
    counts2 = [0, 1, 2, 7] + [tasks - 10]
    tp2 = np.concatenate([[0], np.cumsum(counts2)]).astype(np.uint64)
    want2 = products([range(int(tp2[t]), int(tp2[t + 1])) for t in range(len(counts2))], want)
    for od in (None, np.argsort(-np.array(counts2), kind="stable").astype(np.uint32)):
        out2 = run(partial, 1, tasks, tp2, None, od, len(counts2))
        assert ints(emu.pair_op(n_arr, 1, out2, group=group)) == want2
    # ... and over residues without an index: the rows first .. first + count
    out3 = run(residues, 0, n_rows, np.array([0, 5, 5, n_rows], np.uint64), None, None, 3)
    assert ints(emu.pair_op(n_arr, 1, out3, group=group)) == products([range(0, 5), [], range(5, n_rows)], vals)
