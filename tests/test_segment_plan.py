"""The device planner of the grouped sums on a GPU-less box: csrc/segment_plan.h compiled for the CPU wave emulator
(tests/emu/emu_plan.cpp) and driven through Engine.plan_segments_dev, and the public interface that rests on it —
EncryptedVector.segment_sum through the device plan, with node= / num_nodes= and with PaillierPublicKey.segment_ids — on an emulator
context defined here.

The yardstick of every plan is phe._engine.plan_segments (numpy: stable argsort, bincount, repeat, cumsum), compared element
for element; the yardstick of every ciphertext is the Python-integer product of the members modulo n^2."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import PKG, load_golden

if PKG not in sys.path:
    sys.path.insert(0, PKG)

from phe import _engine, _native, paillier  # noqa: E402
from phe.ciphertext import EncryptedVector, ResidentSegmentIds  # noqa: E402

from plan_cases import assert_same_plan, cases, composed  # noqa: E402
from test_short_obfuscators import resident_emulator_context  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
EMU_DIR = os.path.join(HERE, "emu")
H = lambda s: int(s, 16)
U64 = ctypes.c_uint64


@pytest.fixture(scope="module")
def plan_lib():
    src, lib = os.path.join(EMU_DIR, "emu_plan.cpp"), os.path.join(EMU_DIR, "libphe_emu_plan.so")
    deps = [src, os.path.join(EMU_DIR, "wave_emu.h"), os.path.join(PKG, "csrc", "segment_plan.h")]
    if not os.path.exists(lib) or any(os.path.getmtime(d) > os.path.getmtime(lib) for d in deps):
        subprocess.check_call([os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra",
                               "-Wno-unused-parameter", "-Wno-unknown-pragmas", "-o", lib, src, "-lpthread"], cwd=EMU_DIR)
    L = ctypes.CDLL(lib)
    L.emu_plan_last_error.restype = ctypes.c_char_p
    return L


def planner_context(L):
    """the resident emulator context with the calls grouped sums go through: the planner entry points served by the device
    header on the wave emulator, and — the stand-in part — a "pair form" that is the canonical residue itself, multiplied by
    Python integers (the reduce kernel has tests of its own: tests/test_segment_sum.py)"""
    vp = ctypes.c_void_p

    class PlannerEmuContext(resident_emulator_context()):
        plan_calls = 0

        def pair_words(self):
            return self.ct_limbs

        def to_pair_dev(self, c, pair, batch, stream=0):
            self._rows(pair, batch, self.ct_limbs)[:] = self._rows(c, batch, self.ct_limbs)

        def from_pair_dev(self, pair, m, c, batch, stream=0):
            assert m is None
            self._rows(c, batch, self.ct_limbs)[:] = self._rows(pair, batch, self.ct_limbs)

        def segment_reduce_dev(self, rows, rows_are_pair, n_rows, task_ptr, idx, order, out, tasks, stream=0):
            n2 = self.n * self.n
            vals = _native.limbs_to_ints(self._rows(rows, n_rows, self.ct_limbs)) if n_rows else []
            tp = self._rows(task_ptr, 1, 2 * (tasks + 1))[0].view(np.uint64)
            members = self._rows(idx, 1, int(tp[-1]))[0] if idx is not None and tp[-1] else None
            assert sorted(self._rows(order, 1, tasks)[0].tolist()) == list(range(tasks))
            prods = []
            for t in range(tasks):
                v = 1
                for j in range(int(tp[t]), int(tp[t + 1])):
                    v = v * vals[int(members[j]) if idx is not None else j] % n2
                prods.append(v)
            self._rows(out, tasks, self.ct_limbs)[:] = _native.ints_to_limbs(prods, self.ct_limbs)

        def segment_plan_sort_dev(self, ids, node, groupings, rows, n_segments, n_nodes, idx, counts, stream=0):
            type(self).plan_calls += 1
            rc = L.emu_segment_plan_sort(vp(ids), vp(node), U64(groupings), U64(rows), U64(n_segments), U64(n_nodes), vp(idx),
                                         vp(counts), 3)
            if rc == 3:
                raise ValueError("refused")
            assert rc == 0, L.emu_plan_last_error()

        def segment_plan_level_dev(self, counts, n_out, cap, per, task_ptr, order, tasks, stream=0):
            rc = L.emu_segment_plan_level(vp(counts), U64(n_out), ctypes.c_uint32(cap), vp(per), vp(task_ptr), vp(order), U64(tasks), 3)
            if rc == 3:
                raise ValueError("refused")
            assert rc == 0, L.emu_plan_last_error()
    return PlannerEmuContext


@pytest.fixture
def planner_keys(monkeypatch, plan_lib):
    ctx_class = planner_context(plan_lib)
    monkeypatch.setattr(_native, "Context", ctx_class)
    g = load_golden(256)
    pub = paillier.PaillierPublicKey(H(g["n"]))
    return pub, paillier.PaillierPrivateKey(pub, H(g["p"]), H(g["q"])), ctx_class


# ---- the planner ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", cases(), ids=lambda c: c[0])
def test_device_plan_is_the_numpy_plan(planner_keys, case):
    _, ids, S, node, K, cap = case
    eng = planner_keys[0]._get_engine()
    assert eng.has_segment_planner()
    ids2 = np.atleast_2d(np.asarray(ids, dtype=np.int64))
    want_ids, want_S = composed(ids2, S, node, K)
    want = _engine.plan_segments(want_ids, want_S, cap)
    got = eng.plan_segments_dev(eng.upload_ids(ids2), S, eng.upload_ids(node) if node is not None else None, K, cap)
    assert got.tasks == want.tasks and got.n_idx == want.n_idx and got.n_out == want.n_out
    assert_same_plan(got.to_host(), want)
    if ids2.size and not (want_ids >= 0).any():
        assert got.n_idx == 0


def test_stable_order_within_a_segment(planner_keys):
    eng = planner_keys[0]._get_engine()
    got = eng.plan_segments_dev(eng.upload_ids(np.zeros((1, 300), np.int64)), 1).to_host()
    assert got.levels[0][1].tolist() == list(range(300))
    ids = np.arange(500)[::-1].copy()
    got = eng.plan_segments_dev(eng.upload_ids(ids[None, :]), 500).to_host()
    assert got.levels[0][1].tolist() == list(range(499, -1, -1))


def test_default_cap_is_read_at_call_time(planner_keys, monkeypatch):
    eng = planner_keys[0]._get_engine()
    monkeypatch.setattr(_engine, "SEGMENT_TASK_ROWS", 3)
    got = eng.plan_segments_dev(eng.upload_ids(np.zeros((1, 10), np.int64)), 1)
    assert len(got.tasks) == 3
    assert_same_plan(got.to_host(), _engine.plan_segments(np.zeros(10, np.int64), 1))
    with pytest.raises(ValueError):
        eng.plan_segments_dev(eng.upload_ids(np.zeros((1, 10), np.int64)), 1, cap=1)


def test_no_output_rows(planner_keys):
    eng = planner_keys[0]._get_engine()
    got = eng.plan_segments_dev(eng.upload_ids(np.full((1, 5), -1)), 0)
    assert got.n_out == 0 and got.tasks == [0] and got.n_idx == 0


def test_entry_points_refuse_what_the_header_says(plan_lib):
    L = plan_lib
    one = np.zeros(8, np.uint32)
    p = one.ctypes.data_as(ctypes.c_void_p)
    sort = lambda ids, F, rows, S, K, idx, counts: L.emu_segment_plan_sort(ids, None, U64(F), U64(rows), U64(S), U64(K), idx, counts, 1)
    assert sort(p, 1, 4, 2, 1, p, None) == 3                              # null counts
    assert sort(None, 1, 4, 2, 1, p, p) == 3                              # null ids with rows
    assert sort(p, 1, 4, 0, 1, p, p) == 3                                 # no segments for rows
    assert sort(p, 1, 4, 2, 0, p, p) == 3                                 # no nodes
    assert sort(p, 1 << 16, 1 << 16, 2, 1, p, p) == 3                     # F * rows = 2^32
    assert sort(p, 1, 4, (1 << 32) - 1, 1, p, p) == 3                     # n_out = 2^32 - 1
    assert sort(None, 1, 0, 0, 1, None, p) == 0 and one[0] == 0           # no rows, no segments: only the number kept
    level = lambda counts, n_out, cap, tasks: L.emu_segment_plan_level(counts, U64(n_out), ctypes.c_uint32(cap), p, p, p, U64(tasks), 1)
    assert level(None, 1, 4, 1) == 3 and level(p, 1, 1, 1) == 3 and level(p, 0, 4, 0) == 3 and level(p, 2, 4, 1) == 3


# ---- the public interface ------------------------------------------------------------------------------------------------------
def integer_products(vec, ids, num_segments):
    n2 = vec.public_key.nsquare
    cs = vec.decrease_exponent_to(int(vec.exponent_array.min())).ciphertexts(False)
    want = []
    for row in np.atleast_2d(ids):
        for s in range(num_segments):
            v = 1
            for i in np.nonzero(row == s)[0]:
                v = v * cs[int(i)] % n2
            want.append(v)
    return want


def test_segment_sum_through_the_device_plan(planner_keys, monkeypatch):
    pub, priv, ctx_class = planner_keys
    rng = np.random.RandomState(256)
    x = [float(v) for v in rng.randn(20)] + [int(v) for v in rng.randint(-50, 50, 20)]    # mixed exponents
    vec = pub.encrypt_batch(x)
    ids = rng.randint(-1, 6, size=(3, 40))
    ids[ids == 3] = 2                                                                     # segment 3 stays empty
    want = integer_products(vec, ids, 7)
    # below the threshold: the numpy planner, as before
    monkeypatch.setattr(_engine, "SEGMENT_PLAN_DEVICE_MIN", 3 * 40 + 1)
    before = ctx_class.plan_calls
    host_planned = vec.segment_sum(ids, 7)
    assert ctx_class.plan_calls == before and host_planned.ciphertexts(False) == want
    # at the threshold: the device planner, the same ciphertexts in every input form
    monkeypatch.setattr(_engine, "SEGMENT_PLAN_DEVICE_MIN", 3 * 40)
    dev_planned = vec.segment_sum(ids, 7)
    assert ctx_class.plan_calls == before + 1 and not dev_planned.on_device
    assert dev_planned.ciphertexts(False) == host_planned.ciphertexts(False)
    assert dev_planned.exponents == host_planned.exponents
    resident = vec.to_device()
    assert resident.segment_sum(ids, 7).ciphertexts(False) == want
    pair = resident.to_pair()
    out = pair.segment_sum(ids, 7)
    assert out._pair and out.ciphertexts(False) == want
    assert vec.segment_sum(ids[0]).ciphertexts(False) == want[:int(ids[0].max()) + 1]   # one grouping, num_segments by default
    # ResidentSegmentIds: one upload, then nothing of the ids moves
    monkeypatch.setattr(_engine, "SEGMENT_PLAN_DEVICE_MIN", 0)
    held = pub.segment_ids(ids, 7)
    assert isinstance(held, ResidentSegmentIds) and held.shape == (3, 40) and held.num_segments == 7 and len(held) == 40
    uploads = []
    eng = pub._get_engine()
    real = eng.upload_ids
    monkeypatch.setattr(eng, "upload_ids", lambda a: uploads.append(np.shape(a)) or real(a))
    assert vec.segment_sum(held).ciphertexts(False) == want
    assert resident.segment_sum(held, 7).ciphertexts(False) == want
    assert uploads == [(3, 40)]
    # node=: by definition the composed call
    node = rng.randint(-1, 3, 40)
    composed_ids, composed_S = composed(ids, 7, node, 3)
    want_nodes = integer_products(vec, composed_ids, composed_S)
    uploads.clear()
    got = vec.segment_sum(held, node=node, num_nodes=3)
    assert uploads == [(40,)]                                                             # only the node numbers went up
    assert len(got) == 3 * 3 * 7 and got.ciphertexts(False) == want_nodes
    assert vec.segment_sum(ids, 7, node=node).ciphertexts(False) == want_nodes           # num_nodes defaults to max + 1
    monkeypatch.setattr(_engine, "SEGMENT_PLAN_DEVICE_MIN", 1 << 30)                      # ... and on the numpy planner
    calls = ctx_class.plan_calls
    assert vec.segment_sum(ids, 7, node=node, num_nodes=3).ciphertexts(False) == want_nodes
    assert vec.segment_sum(held, node=node, num_nodes=3).ciphertexts(False) == want_nodes
    assert ctx_class.plan_calls == calls
    dec = np.array(priv.decrypt_batch(got.to_host() if got.on_device else got), dtype=float)
    weights = np.array(x, dtype=float)
    for f in range(3):
        used = composed_ids[f] >= 0
        assert np.allclose(dec[f * 21:(f + 1) * 21], np.bincount(composed_ids[f][used], weights=weights[used], minlength=21),
                           rtol=0, atol=1e-9)


def test_node_without_the_planner_is_the_composed_call(monkeypatch):
    """the emulator backend has neither the reduce kernel nor the planner: node= is computed by its definition"""
    import emu_backend
    emu_backend.install(monkeypatch)
    g = load_golden(256)
    pub = paillier.PaillierPublicKey(H(g["n"]))
    assert not pub._get_engine().has_segment_planner()
    rng = np.random.RandomState(7)
    vec = pub.encrypt_batch([int(v) for v in rng.randint(-50, 50, 30)])
    ids, node = rng.randint(-1, 4, size=(2, 30)), rng.randint(-1, 2, 30)
    cid, cS = composed(ids, 4, node, 2)
    want = integer_products(vec, cid, cS)
    assert vec.segment_sum(ids, 4, node=node, num_nodes=2).ciphertexts(False) == want
    assert vec.segment_sum(pub.segment_ids(ids, 4), node=node, num_nodes=2).ciphertexts(False) == want
    assert vec.segment_sum(pub.segment_ids(ids[0], 4)).ciphertexts(False) == integer_products(vec, ids[0], 4)


def test_error_cases(planner_keys, monkeypatch):
    pub, _, _ = planner_keys
    monkeypatch.setattr(_engine, "SEGMENT_PLAN_DEVICE_MIN", 0)
    vec = EncryptedVector.from_ciphertexts(pub, [12345, pub.nsquare - 2, 99])             # (any residues serve a product)
    with pytest.raises(ValueError):
        vec.segment_sum(pub.segment_ids([0, 1], 2))                                       # wrong length
    with pytest.raises(ValueError):
        vec.segment_sum([0, 1, 1], 2, node=[0, 0])                                        # wrong length of node
    with pytest.raises(ValueError):
        vec.segment_sum([0, 1, 1], 2, node=[[0, 0, 0]])
    with pytest.raises(TypeError):
        vec.segment_sum([0, 1, 1], 2, node=[0.0, 1.0, 0.0])
    with pytest.raises(ValueError):
        vec.segment_sum([0, 1, 1], 2, node=[0, 2, 0], num_nodes=2)                        # 2 is outside [0, 2)
    with pytest.raises(ValueError):
        vec.segment_sum([0, 1, 1], 2, node=[0, -2, 0])
    with pytest.raises(ValueError):
        vec.segment_sum([0, 1, 1], 2, num_nodes=2)                                        # num_nodes without node
    with pytest.raises(ValueError):
        vec.segment_sum(pub.segment_ids([0, 1, 1], 2), 3)                                 # made for another number of segments
    other = paillier.PaillierPublicKey(pub.n + 2)
    with pytest.raises(ValueError):
        vec.segment_sum(other.segment_ids([0, 1, 1], 2))                                  # ids of another key
    with pytest.raises(TypeError):
        pub.segment_ids([0.5, 1.0])
    with pytest.raises(ValueError):
        pub.segment_ids([0, 5], 3)
    with pytest.raises(ValueError) as err:
        vec.segment_sum([0, 7, 9], 2)
    assert "segment id 7" in str(err.value)                                               # the first bad id is still named
    assert vec.segment_sum([-1, -1, -1], node=[0, 0, 0]).ciphertexts(False) == []
    assert vec.segment_sum([0, 1, 1], 2, node=[-1, -1, -1]).ciphertexts(False) == []       # no node at all: num_nodes is 0
    assert vec[:0].segment_sum([], 3).ciphertexts(False) == [1, 1, 1]
    assert vec.segment_sum([1, 0, 1], 2).ciphertexts(False) == [pub.nsquare - 2, 12345 * 99 % pub.nsquare]
