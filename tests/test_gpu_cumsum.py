"""EncryptedVector.cumsum on the GPU (csrc/segment_core.h segment_scan_body through phe_hip_segment_scan_dev): every row must be
the Python-integer running product of its sequence modulo n^2 — the reference's chain of EncryptedNumber.__add__ = _raw_add
(phe/paillier.py:705-719), every prefix kept — whatever form the input is in and whichever route computes it."""
import sys

import numpy as np
import pytest

from conftest import PKG, load_golden

if PKG not in sys.path:
    sys.path.insert(0, PKG)

from phe import _engine, paillier  # noqa: E402
from phe.ciphertext import EncryptedVector  # noqa: E402

pytestmark = pytest.mark.gpu

H = lambda s: int(s, 16)


def keypair(bits):
    g = load_golden(bits)
    pub = paillier.PaillierPublicKey(H(g["n"]))
    return pub, paillier.PaillierPrivateKey(pub, H(g["p"]), H(g["q"]))


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


def pair_geometry(ctx):
    code = ctx.last_launch()["geom_pub"]
    assert 2 * (code // 100) * (code % 100) == ctx.pair_words(), code                    # a rung that serves the pair rows
    return code // 100


def mixed(rs, n):
    """n numbers, floats and integers in turn-about blocks: the exponents differ"""
    x = [float(v) for v in rs.standard_normal(n)]
    for i in range(0, n, 3):
        x[i] = int(rs.integers(-99, 99))
    return x


@pytest.fixture(scope="module")
def ragged():
    """per key width: 70 encrypted rows of mixed exponents (host vector) and their integer running products, made once"""
    made = {}
    for bits in (1024, 2048):
        pub, _ = keypair(bits)
        rs = np.random.Generator(np.random.PCG64(bits))
        host = pub.encrypt_batch(mixed(rs, 70))
        assert len(set(host.exponents)) > 1
        made[bits] = (host, integer_running_products(host))
    return made


@pytest.mark.parametrize("bits", [1024, 2048])
@pytest.mark.parametrize("cap", [None, 4])
def test_ragged_depth_in_every_input_form(monkeypatch, ragged, bits, cap):
    """lengths around the task cap; with the cap at 4, 70 rows make 18 -> 5 -> 2 tasks: four levels, every one of them and the
    single-level exit.  Host, resident and pair-resident input: the same bits, the integer running products."""
    if cap is not None:
        monkeypatch.setattr(_engine, "SCAN_TASK_ROWS", cap)
        assert [len(lv[0]) - 1 for lv in _engine.plan_scan(70).levels] == [18, 5, 2, 1]
    host70, want70 = ragged[bits]
    eng = host70.public_key._get_engine()
    assert eng.has_segment_scan()
    for length in (1, 2, 3, 4, 5, 17, 70):
        host = host70[:length]
        want = want70[:length] if min(host.exponents) == min(host70.exponents) else integer_running_products(host)
        dev = host.to_device()
        pair = dev.to_pair()
        assert pair._pair
        a, b, p = host.cumsum(), dev.cumsum(), pair.cumsum()
        assert not a.on_device and b.on_device and not b._pair and p.on_device
        assert a.ciphertexts(False) == want, length
        assert b.ciphertexts(False) == want, length
        assert p.ciphertexts(False) == want, length
        assert a.exponents == b.exponents == p.exponents == [min(host.exponents)] * length
        assert not a._obfuscated.any() and not b._obfuscated.any() and not p._obfuscated.any()


def test_block_form():
    pub, priv = keypair(2048)
    rs = np.random.Generator(np.random.PCG64(5))
    x = mixed(rs, 65)
    host = pub.encrypt_batch(x)
    aligned = host.decrease_exponent_to(min(host.exponents))
    for vec in (host, host.to_device(), host.to_device().to_pair()):
        out = vec.cumsum(block=5)                                                         # 13 tasks: no wavefront filled evenly
        assert out.ciphertexts(False) == integer_running_products(host, 5)
        assert vec.cumsum(block=65).ciphertexts(False) == vec.cumsum().ciphertexts(False) == integer_running_products(host)
        assert vec.cumsum(block=1).ciphertexts(False) == aligned.ciphertexts(False)
    dec = np.array(priv.decrypt_batch(host.to_device().cumsum(block=5)), dtype=float)
    assert np.allclose(dec, np.array(x, dtype=float).reshape(13, 5).cumsum(axis=1).ravel(), rtol=0, atol=1e-9)
    with pytest.raises(ValueError):
        host.to_device().cumsum(block=7)
    with pytest.raises(TypeError):
        host.to_device().cumsum(block=2.5)
    assert len(host.to_device()[:0].cumsum()) == 0


def test_histograms_then_left_child_sums():
    """segment_sum(ids2d, S).cumsum(block=S) end to end: F histograms, then the running sum over the bins of each"""
    pub, priv = keypair(1024)
    rs = np.random.Generator(np.random.PCG64(8))
    x = rs.standard_normal(300)
    F, S = 3, 7
    ids = rs.integers(-1, S, size=(F, 300))
    enc = pub.encrypt_batch([float(v) for v in x], device=True)
    left = enc.segment_sum(ids, S).cumsum(block=S)
    assert len(left) == F * S
    clear = np.stack([np.bincount(row[row >= 0], weights=x[row >= 0], minlength=S) for row in ids])
    assert np.allclose(np.array(priv.decrypt_batch(left), dtype=float), np.cumsum(clear, axis=1).ravel(), rtol=0, atol=1e-9)


def test_many_short_sequences_and_the_small_batch_rung():
    pub, _ = keypair(2048)
    rs = np.random.Generator(np.random.PCG64(11))
    n_blocks = 4096
    vec = pub.encrypt_batch([int(v) for v in rs.integers(-1000, 1000, 3 * n_blocks)], device=True).to_pair()
    ctx = pub._get_engine().ctx
    out = vec.cumsum(block=3)
    g_big = pair_geometry(ctx)
    assert out._pair and out.ciphertexts(False) == integer_running_products(vec, 3)
    small = vec[:6].to_pair()
    out6 = small.cumsum()
    g_small = pair_geometry(ctx)
    assert out6.ciphertexts(False) == integer_running_products(small)
    # The pair rows of a 2048-bit key are served by 4 lanes per number (rung 0) and by 8 (the only wider rung with their limb
    # count).  256 CUs hold 2 x 64 four-lane groups each: 4096 tasks fill an eighth of them, and the ladder already gives them
    # the 8-lane rung, like the single task of 6 rows — the two runs above cannot differ in geometry.  2^16 tasks are two full
    # rounds of four-lane groups (four of eight-lane ones): rung 0, which the single task must not take.
    assert g_small == 8 and g_big in (4, 8)
    eng = pub._get_engine()
    n_tasks = 1 << 16
    words = rs.integers(0, 1 << 32, size=(2 * n_tasks, eng.ct_limbs), dtype=np.uint64).astype(np.uint32)
    words[:, -1] = 0                                                                      # any residues below n^2 serve a product
    full = EncryptedVector(pub, eng.upload_cipher(words), np.zeros(2 * n_tasks, dtype=np.int64)).to_pair()
    out_full = full.cumsum(block=2)
    g_full = pair_geometry(ctx)
    assert g_full == 4 and g_full != g_small
    got = out_full._plain_rows().to_host()
    assert np.array_equal(got[0::2], words[0::2])                                         # the first row of every block: itself
    cs = eng.to_ints(words)
    n2 = pub.nsquare
    assert eng.to_ints(got[1::2]) == [cs[i] * cs[i + 1] % n2 for i in range(0, 2 * n_tasks, 2)]


def test_without_split_engine_the_sums_go_by_doubling(monkeypatch):
    """PHE_HIP_ENGINE=full: no pair form, no running-sum kernel — log-step doubling, the same bits as the kernel's route"""
    g = load_golden(1024)
    rs = np.random.Generator(np.random.PCG64(6))
    x = mixed(rs, 60)
    r_values = [int(v) for v in rs.integers(2, 1 << 62, 60)]
    ref_vec = paillier.PaillierPublicKey(H(g["n"])).encrypt_batch(x, r_values=r_values)
    want, want12 = integer_running_products(ref_vec), integer_running_products(ref_vec, 12)
    assert ref_vec._eng().has_segment_scan()
    assert ref_vec.cumsum().ciphertexts(False) == want                                    # (the kernel's route)
    assert ref_vec.to_device().cumsum(block=12).ciphertexts(False) == want12
    monkeypatch.setenv("PHE_HIP_ENGINE", "full")
    pub = paillier.PaillierPublicKey(H(g["n"]))
    eng = pub._get_engine()
    assert eng.ctx.info()["engine_pub"] != "split" and not eng.has_segment_scan()
    for vec in (pub.encrypt_batch(x, r_values=r_values), pub.encrypt_batch(x, r_values=r_values, device=True)):
        out = vec.cumsum()
        assert out.on_device == vec.on_device
        assert out.ciphertexts(False) == want and out.exponents == [min(vec.exponents)] * 60
        assert vec.cumsum(block=12).ciphertexts(False) == want12
        assert vec.cumsum(block=1).ciphertexts(False) == vec.decrease_exponent_to(min(vec.exponents)).ciphertexts(False)


def test_a_result_in_the_pair_form_stays_in_it():
    pub, priv = keypair(2048)
    rs = np.random.Generator(np.random.PCG64(9))
    x = [int(v) for v in rs.integers(-500, 500, 40)]
    vec = pub.encrypt_batch(x, device=True).to_pair()
    out = vec.cumsum()
    assert out._pair and out.on_device
    want = integer_running_products(vec)
    both = out + vec                                                                      # (one pair product, still in the form)
    assert both._pair
    n2 = pub.nsquare
    assert both.ciphertexts(False) == [a * b % n2 for a, b in zip(want, vec.ciphertexts(False))]
    assert out.ciphertexts(False) == want                                                 # converts to the same residues
    assert np.allclose(np.array(priv.decrypt_batch(out), dtype=float), np.cumsum(x), rtol=0, atol=1e-9)
