"""The device planner of the grouped sums on the GPU (csrc/segment_plan.h through phe_hip_segment_plan_sort_dev /
phe_hip_segment_plan_level_dev) and the public calls that rest on it.  Every plan is compared element for element with the numpy
planner phe._engine.plan_segments; every ciphertext with the Python-integer product of the members modulo n^2 — per group the
reference's chain of EncryptedNumber.__add__ = _raw_add (phe/paillier.py:705-719)."""
import sys

import numpy as np
import pytest

from conftest import PKG, load_golden

if PKG not in sys.path:
    sys.path.insert(0, PKG)

from phe import _engine, paillier  # noqa: E402

from plan_cases import assert_same_plan, cases, composed  # noqa: E402

pytestmark = pytest.mark.gpu

H = lambda s: int(s, 16)


def keypair(bits):
    g = load_golden(bits)
    pub = paillier.PaillierPublicKey(H(g["n"]))
    return pub, paillier.PaillierPrivateKey(pub, H(g["p"]), H(g["q"]))


@pytest.fixture(scope="module")
def engine():
    eng = keypair(1024)[0]._get_engine()
    assert eng.has_segment_planner() and eng.has_segment_reduce()
    return eng


def device_plan(eng, ids, S, node, K, cap):
    ids2 = np.atleast_2d(np.asarray(ids, dtype=np.int64))
    got = eng.plan_segments_dev(eng.upload_ids(ids2), S, eng.upload_ids(node) if node is not None else None, K, cap)
    want_ids, want_S = composed(ids2, S, node, K)
    return got, _engine.plan_segments(want_ids, want_S, cap)


@pytest.mark.parametrize("case", cases(), ids=lambda c: c[0])
def test_device_plan_is_the_numpy_plan(engine, case):
    _, ids, S, node, K, cap = case
    got, want = device_plan(engine, ids, S, node, K, cap)
    assert got.tasks == want.tasks and got.n_idx == want.n_idx and got.n_out == want.n_out
    assert_same_plan(got.to_host(), want)


def test_several_blocks_and_three_passes(engine):
    """2^16 + 1 rows in two groupings over 70,000 segments each: 140,000 output rows (three digit passes), 65 tiles per pass,
    and prefix sums over more than one chunk.  Index arrays only."""
    rs = np.random.Generator(np.random.PCG64(14))
    rows = (1 << 16) + 1
    ids = rs.integers(-1, 70000, size=(2, rows))
    ids[0, :3000] = 69999                                                                  # a long segment: several levels
    got, want = device_plan(engine, ids, 70000, None, 1, None)
    assert len(want.levels) >= 3
    assert_same_plan(got.to_host(), want)
    again, _ = device_plan(engine, ids, 70000, None, 1, None)                              # no atomics: the same arrays every time
    assert_same_plan(again.to_host(), want)


def integer_products(vec, ids, num_segments):
    """per segment the product of the members' ciphertexts (aligned to the smallest exponent) modulo n^2, in Python integers"""
    n2 = vec.public_key.nsquare
    cs = vec.decrease_exponent_to(int(vec.exponent_array.min())).ciphertexts(False)
    want = []
    for row in np.atleast_2d(ids):
        order = np.argsort(row, kind="stable")
        bounds = np.searchsorted(row[order], np.arange(num_segments + 1))
        for s in range(num_segments):
            v = 1
            for i in order[bounds[s]:bounds[s + 1]]:
                v = v * cs[int(i)] % n2
            want.append(v)
    return want


@pytest.mark.parametrize("cap", [None, 4])
def test_host_planned_and_device_planned_bits(monkeypatch, cap):
    """300 rows, 12 shuffled ragged segments, three groupings: host-planned and device-planned segment_sum on host, resident and
    pair-resident input give the same ciphertexts, the integer products"""
    if cap is not None:
        monkeypatch.setattr(_engine, "SEGMENT_TASK_ROWS", cap)
    c = _engine.SEGMENT_TASK_ROWS
    pub, _ = keypair(1024)
    sizes = [0, 1, 2, 3, c - 1, c, c + 1, 70, 5, 0, 9, 2 * c]
    rs = np.random.Generator(np.random.PCG64(1024 + c))
    ids = []
    for _ in range(3):
        row = np.concatenate([np.repeat(np.arange(12), sizes), np.full(300 - sum(sizes), -1)])
        rs.shuffle(row)
        ids.append(row)
    ids = np.stack(ids)
    x = np.concatenate([rs.standard_normal(150), rs.integers(-99, 99, 150).astype(float)])
    host = pub.encrypt_batch([float(v) for v in x[:150]] + [int(v) for v in x[150:]])     # mixed exponents
    want = integer_products(host, ids, 12)
    dev = host.to_device()
    pair = dev.to_pair()
    eng = pub._get_engine()
    calls = []
    real = eng.plan_segments_dev
    monkeypatch.setattr(eng, "plan_segments_dev", lambda *a, **kw: calls.append(1) or real(*a, **kw))
    results = {}
    for route, threshold in (("host", 1 << 40), ("device", 0)):
        monkeypatch.setattr(_engine, "SEGMENT_PLAN_DEVICE_MIN", threshold)
        before = len(calls)
        a, b, p = host.segment_sum(ids, 12), dev.segment_sum(ids, 12), pair.segment_sum(ids, 12)
        assert len(calls) - before == (3 if route == "device" else 0)
        assert not a.on_device and b.on_device and not b._pair and p.on_device and p._pair
        results[route] = [a.ciphertexts(False), b.ciphertexts(False), p.ciphertexts(False)]
        assert a.exponents == b.exponents == p.exponents == [min(host.exponents)] * 36
    assert results["host"] == [want, want, want]
    assert results["device"] == [want, want, want]
    assert want[0] == 1 and want[9] == 1                                                  # no members: the ciphertext 1


def test_resident_ids_with_two_node_arrays(monkeypatch):
    monkeypatch.setattr(_engine, "SEGMENT_PLAN_DEVICE_MIN", 0)
    pub, _ = keypair(1024)
    rs = np.random.Generator(np.random.PCG64(5))
    vec = pub.encrypt_batch([int(v) for v in rs.integers(-1000, 1000, 200)], device=True)
    pair = vec.to_pair()
    bins = rs.integers(-1, 6, size=(2, 200))
    held = pub.segment_ids(bins, 6)
    eng = pub._get_engine()
    uploads = []
    real = eng.upload_ids
    monkeypatch.setattr(eng, "upload_ids", lambda a: uploads.append(np.shape(a)) or real(a))
    for seed in (1, 2):
        node = np.random.Generator(np.random.PCG64(seed)).integers(-1, 4, 200)
        cid, cS = composed(bins, 6, node, 4)
        want = integer_products(vec, cid, cS)
        out = vec.segment_sum(held, node=node, num_nodes=4)
        assert len(out) == 2 * 4 * 6 and out.on_device and not out._pair and out.ciphertexts(False) == want
        monkeypatch.setattr(_engine, "SEGMENT_PLAN_DEVICE_MIN", 1 << 40)
        assert vec.segment_sum(cid, cS).ciphertexts(False) == want                         # the numpy-composed, host-planned call
        monkeypatch.setattr(_engine, "SEGMENT_PLAN_DEVICE_MIN", 0)
        out = pair.segment_sum(held, node=node, num_nodes=4)
        assert out._pair and out.ciphertexts(False) == want                                # pair form in, pair form out
    assert uploads == [(2, 200), (200,), (200,), (200,), (200,)]                           # the bins went up once
