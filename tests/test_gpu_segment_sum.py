"""EncryptedVector.segment_sum on the GPU (csrc/segment_core.h through phe_hip_segment_reduce_dev): every row must be the
Python-integer product of its members modulo n^2 — per group the reference's chain of EncryptedNumber.__add__ = _raw_add
(phe/paillier.py:705-719) — whatever form the input is in and whichever route computes it."""
import sys

import numpy as np
import pytest

from conftest import PKG, load_golden

if PKG not in sys.path:
    sys.path.insert(0, PKG)

from phe import _engine, paillier  # noqa: E402

pytestmark = pytest.mark.gpu

H = lambda s: int(s, 16)


def keypair(bits):
    g = load_golden(bits)
    pub = paillier.PaillierPublicKey(H(g["n"]))
    return pub, paillier.PaillierPrivateKey(pub, H(g["p"]), H(g["q"]))


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


def pair_geometry(ctx):
    code = ctx.last_launch()["geom_pub"]
    assert 2 * (code // 100) * (code % 100) == ctx.pair_words(), code                    # a rung that serves the pair rows
    return code // 100


@pytest.mark.parametrize("bits", [1024, 2048])
@pytest.mark.parametrize("cap", [None, 4])
def test_ragged_segments_in_every_input_form(monkeypatch, bits, cap):
    """300 rows in 12 shuffled segments whose sizes straddle the task cap; with the cap at 4 the segment of 70 rows takes
    ceil(log_4(70)) = 4 levels.  Host, resident and pair-resident input: the same bits, the integer product."""
    if cap is not None:
        monkeypatch.setattr(_engine, "SEGMENT_TASK_ROWS", cap)
    c = _engine.SEGMENT_TASK_ROWS
    pub, _ = keypair(bits)
    sizes = [0, 1, 2, 3, c - 1, c, c + 1, 70, 5, 0, 9, 2 * c]
    assert sum(sizes) < 300
    ids = np.concatenate([np.repeat(np.arange(12), sizes), np.full(300 - sum(sizes), -1)])    # the other rows are left out
    rs = np.random.Generator(np.random.PCG64(bits + c))
    rs.shuffle(ids)
    plan = _engine.plan_segments(ids, 12)
    longest, levels, reach = max(sizes), 1, c
    while reach < longest:
        levels, reach = levels + 1, reach * c
    assert len(plan.levels) == levels and (cap is None or levels == 4)
    x = np.concatenate([rs.standard_normal(150), rs.integers(-99, 99, 150).astype(float)])
    host = pub.encrypt_batch([float(v) for v in x[:150]] + [int(v) for v in x[150:]])     # mixed exponents
    assert len(set(host.exponents)) > 1
    want = integer_products(host, ids, 12)
    dev = host.to_device()
    pair = dev.to_pair()
    assert pair._pair
    a, b, p = host.segment_sum(ids, 12), dev.segment_sum(ids, 12), pair.segment_sum(ids, 12)
    assert not a.on_device and b.on_device and not b._pair and p.on_device
    assert a.ciphertexts(False) == want
    assert b.ciphertexts(False) == want
    assert p.ciphertexts(False) == want
    assert a.exponents == b.exponents == p.exponents == [min(host.exponents)] * 12
    assert want[0] == 1 and want[9] == 1                                                  # no members: the ciphertext 1
    # a vector already aligned and in the pair form stays there
    aligned = dev.decrease_exponent_to(min(host.exponents)).to_pair()
    q = aligned.segment_sum(ids, 12)
    assert q._pair and q.ciphertexts(False) == want
    members = np.nonzero(ids == 7)[0]
    assert host.decrease_exponent_to(min(host.exponents))[members].sum().ciphertext(False) == want[7]


def test_many_short_tasks_and_the_small_batch_rung():
    pub, _ = keypair(1024)
    rs = np.random.Generator(np.random.PCG64(11))
    n_seg = 4096
    vec = pub.encrypt_batch([int(v) for v in rs.integers(-1000, 1000, 2 * n_seg)], device=True).to_pair()
    ids = np.repeat(np.arange(n_seg), 2)
    rs.shuffle(ids)
    ctx = pub._get_engine().ctx
    out = vec.segment_sum(ids, n_seg)
    g_big = pair_geometry(ctx)
    assert out._pair and out.ciphertexts(False) == integer_products(vec, ids, n_seg)
    small = vec[:6].to_pair()
    ids3 = np.array([2, 0, 1, 1, 0, 2])
    out3 = small.segment_sum(ids3, 3)
    g_small = pair_geometry(ctx)
    assert g_small >= g_big                                                               # three tasks: a rung of wider groups, if any
    assert out3.ciphertexts(False) == integer_products(small, ids3, 3)


def test_histogram_form():
    pub, _ = keypair(2048)
    rs = np.random.Generator(np.random.PCG64(3))
    vec = pub.encrypt_batch([float(v) for v in rs.standard_normal(200)])
    ids = rs.integers(-1, 5, size=(3, 200))
    want = integer_products(vec, ids, 5)
    for v in (vec, vec.to_device(), vec.to_device().to_pair()):
        out = v.segment_sum(ids, 5)
        assert len(out) == 15 and out.ciphertexts(False) == want                          # row f * num_segments + s
        one_by_one = sum((v.segment_sum(ids[f], 5).ciphertexts(False) for f in range(3)), [])
        assert out.ciphertexts(False) == one_by_one


def test_same_bits_as_matvec_with_an_indicator_matrix():
    sp = pytest.importorskip("scipy.sparse")
    pub, _ = keypair(2048)
    rs = np.random.Generator(np.random.PCG64(4))
    vec = pub.encrypt_batch([int(v) for v in rs.integers(-500, 500, 200)], device=True)   # one exponent: matvec aligns per row
    ids = rs.integers(0, 9, 200)
    ids[ids == 4] = 3                                                                     # an empty row
    M = sp.csr_matrix((np.ones(200, dtype=np.int64), (ids, np.arange(200))), shape=(9, 200))
    a, b = vec.segment_sum(ids, 9), vec.matvec(M)
    assert a.ciphertexts(False) == b.ciphertexts(False) == integer_products(vec, ids, 9)
    assert a.exponents == b.exponents


def test_without_split_engine_the_products_go_by_rounds(monkeypatch):
    """PHE_HIP_ENGINE=full: no pair form, no grouped-sum kernel — rounds of the element-wise product, the same bits"""
    g = load_golden(1024)
    rs = np.random.Generator(np.random.PCG64(6))
    x = [float(v) for v in rs.standard_normal(30)] + [int(v) for v in rs.integers(-9, 9, 31)]
    r_values = [int(v) for v in rs.integers(2, 1 << 62, 61)]
    ids = rs.integers(-1, 5, 61)
    ids2 = np.stack([ids, rs.integers(0, 6, 61)])
    ref_vec = paillier.PaillierPublicKey(H(g["n"])).encrypt_batch(x, r_values=r_values)
    want, want2 = integer_products(ref_vec, ids, 6), integer_products(ref_vec, ids2, 6)
    assert ref_vec.segment_sum(ids, 6).ciphertexts(False) == want                         # (the kernel's route)
    monkeypatch.setenv("PHE_HIP_ENGINE", "full")
    pub = paillier.PaillierPublicKey(H(g["n"]))
    eng = pub._get_engine()
    assert eng.ctx.info()["engine_pub"] != "split" and not eng.has_segment_reduce()
    for vec in (pub.encrypt_batch(x, r_values=r_values), pub.encrypt_batch(x, r_values=r_values, device=True)):
        out = vec.segment_sum(ids, 6)
        assert out.on_device == vec.on_device
        assert out.ciphertexts(False) == want and out.exponents == [min(vec.exponents)] * 6
        assert vec.segment_sum(ids2, 6).ciphertexts(False) == want2


@pytest.mark.parametrize("bits", [1024, 2048])
def test_decrypted_sums_are_the_bincount(bits):
    pub, priv = keypair(bits)
    rs = np.random.Generator(np.random.PCG64(bits))
    x = rs.standard_normal(500)
    ids = rs.integers(-1, 16, 500)
    out = pub.encrypt_batch([float(v) for v in x], device=True).segment_sum(ids, 16)
    used = ids >= 0
    want = np.bincount(ids[used], weights=x[used], minlength=16)
    # the encoding keeps 53 bits of every float exactly and the sums are exact; np.bincount rounds once per addition
    assert np.allclose(priv.decrypt_batch(out), want, rtol=0, atol=len(x) * np.finfo(float).eps * np.abs(x).sum())
