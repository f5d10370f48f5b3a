"""The slot codec of packed plaintexts on the GPU (csrc/slot_codec.h through phe_hip_slots_pack_dev / phe_hip_slots_unpack_dev):
the two kernels on uploaded rows against Python integers — no encryption involved —, then PaillierPublicKey.encrypt_packed
bit for bit against (1 + n V) * pow(r, n, n^2) mod n^2 and PaillierPrivateKey.decrypt_packed against the host unpacking of the
same plaintext rows.  Overflow rows are ordinary data here: a status byte, never a fault."""
import random
import sys

import numpy as np
import pytest

from conftest import PKG, load_golden

if PKG not in sys.path:
    sys.path.insert(0, PKG)

import slots_cases as sc  # noqa: E402
from phe import paillier  # noqa: E402
from phe._device import DeviceArray  # noqa: E402
from phe.ciphertext import EncryptedVector  # noqa: E402

pytestmark = pytest.mark.gpu

H = lambda s: int(s, 16)
_keys = {}


def keypair(bits):
    """one key pair (one GPU context) per width for the whole module"""
    if bits not in _keys:
        g = load_golden(bits)
        pub = paillier.PaillierPublicKey(H(g["n"]))
        _keys[bits] = (pub, paillier.PaillierPrivateKey(pub, H(g["p"]), H(g["q"])))
    return _keys[bits]


def widest(pub, B):
    return (pub.max_int.bit_length() - 1) // B


def test_the_backend_has_the_slot_codec():
    pub, priv = keypair(1024)
    assert pub._get_engine().has_slot_codec() and priv._get_engine().has_slot_codec()


# ---- the kernels alone --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", sc.B_VALUES)
@pytest.mark.parametrize("bits, group", [(1024, 16), (2048, 16), (3072, 64)])
def test_kernels_against_python_integers(bits, group, B):
    pub, _ = keypair(bits)
    eng = pub._get_engine()
    pack = lambda values, S, B: eng.slots_pack_dev(values, S, B).to_host()
    unpack = lambda m_rows, S, B: eng.slots_unpack_dev(DeviceArray.from_host(eng.ctx, m_rows), S, B)
    for S in sc.slot_counts(pub.n, B):
        # a few hundred rows, not a multiple of the 256 / group rows of a workgroup, the last one ragged
        sc.check_codec(pack, unpack, pub.n, S, B, seed=bits + B, min_rows=200, not_a_multiple_of=256 // group)


def test_kernel_row_counts_and_refused_arguments():
    pub, _ = keypair(2048)
    eng = pub._get_engine()
    rng = random.Random(9)
    S, B = 5, 33
    lo, hi = -(1 << (B - 1)), (1 << (B - 1)) - 1
    for count in (0, 1, S - 1, S, 67 * S + S - 1):
        x = [rng.randint(lo, hi) for _ in range(count)]
        rows = -(-count // S)
        dev = eng.slots_pack_dev(sc.as_int64(x), S, B)
        assert dev.shape == (rows, eng.n_limbs)
        padded = x + [0] * (rows * S - count)
        assert sc.to_ints(dev.to_host()) == [sc.pack_int(padded[b * S:(b + 1) * S], B, pub.n) for b in range(rows)]
        values, status = eng.slots_unpack_dev(dev, S, B)
        assert values.tolist() == padded and status.shape == (rows,) and not status.any()
    bound = pub.max_int.bit_length() - 1
    vals = DeviceArray.from_host(eng.ctx, np.zeros(16, np.uint32))
    rows_ = DeviceArray(eng.ctx, 2, eng.n_limbs)
    for S, B in ((0, 8), (4, 0), (4, 65), (bound // 8 + 1, 8)):
        with pytest.raises(ValueError):
            eng.ctx.slots_pack_dev(vals.ptr, 8, S, B, rows_.ptr, 2)
        with pytest.raises(ValueError):
            eng.ctx.slots_unpack_dev(rows_.ptr, 2, S, B, vals.ptr, vals.ptr)
    with pytest.raises(ValueError, match="rows"):
        eng.ctx.slots_pack_dev(vals.ptr, 8, 4, 8, rows_.ptr, 3)
    with pytest.raises(ValueError, match="null"):
        eng.ctx.slots_pack_dev(None, 8, 4, 8, rows_.ptr, 2)


# ---- end to end ---------------------------------------------------------------------------------------------------------------
def expected_rows(pub, mantissas, S, B, rns):
    """(1 + n (V_b mod n)) * rn_b mod n^2 in Python integers, V_b = sum_j x_j 2^(B j), rn_b = r_b^n mod n^2"""
    n, n2 = pub.n, pub.nsquare
    out = []
    for b, rn in enumerate(rns):
        V = sum(x << (B * j) for j, x in enumerate(mantissas[b * S:(b + 1) * S]))
        out.append((1 + n * (V % n)) * rn % n2)
    return out


@pytest.mark.parametrize("bits", [1024, 2048])
def test_encrypt_packed_bit_for_bit(bits):
    pub, priv = keypair(bits)
    priv._get_engine()                                                 # (the key pair's engine serves the public key from here on)
    eng = pub._get_engine()
    pub.discard_obfuscators()
    rng = random.Random(bits)
    n, n2 = pub.n, pub.nsquare
    for S, B in ((widest(pub, 64), 64), (7, 33), (widest(pub, 65), 65)):     # (B = 65: packed on the host, same bits)
        count = 10 * S - 3
        rows = -(-count // S)
        lo, hi = -(1 << (B - 1)), (1 << (B - 1)) - 1
        x = [rng.randint(lo, hi) for _ in range(count)]
        x[:2] = [lo, hi]
        rs = [rng.randrange(1, n) for _ in range(rows)]
        want = expected_rows(pub, x, S, B, [pow(r, n, n2) for r in rs])
        values = np.array(x, dtype=np.int64) if B <= 64 else x
        host = pub.encrypt_packed(values, S, B, r_values=rs)
        assert not host.on_device and host.ciphertexts(False) == want, (S, B)
        dev = pub.encrypt_packed(values, S, B, r_values=rs, device=True)
        assert dev.on_device and len(dev) == rows and dev.ciphertexts(False) == want, (S, B)
        assert priv.decrypt_packed(dev, S, B, count=count) == x
        # the pool route: obfuscators made ahead of time, each used once, in order
        pub.precompute_obfuscators(rows)
        rns = eng.peek_obfuscators(rows)
        pooled = pub.encrypt_packed(values, S, B, device=True)
        assert pub.obfuscators_available() == 0
        assert pooled.ciphertexts(False) == expected_rows(pub, x, S, B, rns), (S, B)
    # fresh obfuscators drawn on the spot (more rows than a pool refill serves): the round trip
    S, B = 2, 16
    x = np.array([rng.randint(-2 ** 15, 2 ** 15 - 1) for _ in range(2 * 1100 + 1)], dtype=np.int64)
    for device in (False, True):
        vec = pub.encrypt_packed(x, S, B, device=device)
        assert vec.on_device == device and len(vec) == 1101
        assert np.array_equal(priv.decrypt_packed(vec, S, B, count=len(x), as_array=True), x)
    pub.discard_obfuscators()


@pytest.mark.parametrize("bits", [1024, 2048])
def test_decrypt_packed_equals_the_host_unpacking(bits):
    pub, priv = keypair(bits)
    eng = priv._get_engine()
    assert eng.has_slot_codec()
    rng = np.random.RandomState(bits)
    S, B = widest(pub, 40), 40
    count = 10 * S - 2
    x = rng.randint(-2 ** 39, 2 ** 39, count)
    for values, precision, dtype in ((x, None, np.int64), (x / 4096.0, 2.0 ** -12, np.float64)):
        vec = pub.encrypt_packed(values, S, B, precision=precision, device=True)
        plain = eng.raw_decrypt_dev(vec.limbs(be_secure=False))                        # the same plaintext rows, on the host
        want = priv._unpack_plain(plain, vec.exponent_array, S, B, None)
        assert want[:count] == values.tolist()
        got = priv.decrypt_packed(vec, S, B)
        assert got == want and [type(v) for v in got[:3]] == [type(v) for v in want[:3]]
        assert priv.decrypt_packed(vec, S, B, count=count) == want[:count]
        assert priv.decrypt_packed(vec.to_host(), S, B, count=S + 1) == want[:S + 1]   # a host vector: uploaded by chunks
        arr = priv.decrypt_packed(vec, S, B, count=count, as_array=True)
        assert isinstance(arr, np.ndarray) and arr.dtype == dtype and arr.tolist() == want[:count]
        assert priv.decrypt_packed(vec, S, B, as_array=True).shape == (len(vec) * S,)
    # rows that raise: the lowest row decides, and both routes say the same
    good = pub.encrypt_packed(x, S, B).ciphertexts(False)
    enc = lambda m: pub.raw_encrypt(m % pub.n, 12345)
    gap, wide = enc(pub.max_int + 1), enc(1 << (S * B))
    for cts, message in ((good[:3] + [gap] + good[3:5] + [wide], "Overflow detected"), (good[:2] + [wide, gap], "does not fit")):
        vec = EncryptedVector.from_ciphertexts(pub, cts, 0)
        plain = eng.raw_decrypt(vec.limbs(be_secure=False))
        with pytest.raises(OverflowError, match=message):
            priv._unpack_plain(plain, vec.exponent_array, S, B, None)
        for as_array in (False, True):
            with pytest.raises(OverflowError, match=message):
                priv.decrypt_packed(vec, S, B, as_array=as_array)
    assert priv.decrypt_packed(EncryptedVector.from_ciphertexts(pub, good[:2], 0), S, B) == x[:2 * S].tolist()


def test_chunked_generator_many_chunks_and_early_exit():
    pub, priv = keypair(1024)
    eng = priv._get_engine()
    rng = np.random.RandomState(4)
    S, B = 6, 50
    x = rng.randint(-2 ** 49, 2 ** 49, 23 * S)
    vec = pub.encrypt_packed(x, S, B, device=True)
    for store in (vec.limbs(be_secure=False), vec.to_host().limbs(be_secure=False)):   # resident rows, and host rows
        seen, parts = [], []
        for lo, hi, values, status in eng.raw_decrypt_unpack_chunks(store, S, B, chunk=5):
            assert values.dtype == np.int64 and values.shape == ((hi - lo) * S,) and status.shape == (hi - lo,) and not status.any()
            seen.append((lo, hi))
            parts.append(values)
        assert seen == [(0, 5), (5, 10), (10, 15), (15, 20), (20, 23)]
        assert np.array_equal(np.concatenate(parts), x)
    # an overflow row in the second chunk: the consumer stops there, the generator's cleanup waits for the chunk in flight
    cts = vec.ciphertexts(False)
    cts[7] = pub.raw_encrypt(pub.max_int + 1, 99)
    bad = EncryptedVector.from_ciphertexts(pub, cts, 0)
    chunks = eng.raw_decrypt_unpack_chunks(bad.limbs(be_secure=False), S, B, chunk=5)
    lo, hi, values, status = next(chunks)
    assert (lo, hi) == (0, 5) and not status.any()
    lo, hi, values, status = next(chunks)
    assert status.tolist() == [0, 0, 1, 0, 0]
    chunks.close()
    with pytest.raises(OverflowError, match="Overflow detected"):
        priv.decrypt_packed(bad, S, B)
    assert priv.decrypt_packed(vec, S, B) == x.tolist()                # the engine goes on working


def test_federated_example_packed_on_gpu():
    """examples/federated_learning_batched.py run_packed, the full 50 rounds at 2048 bits: the plaintext aggregation to the
    quantisation step 2^-32.  Bound: the weights are off by at most 1.5 * 50 * 2^-33 < 9e-9 each, a prediction by < 2e-8, the mean
    squared error (residuals of a few hundred) by < 2e-5 of about 3775: rtol 1e-7 leaves a factor of ten."""
    import os
    from conftest import ROOT
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import federated_learning_batched as fed
    from test_federated_example import plaintext_rounds
    errors, _ = fed.run_packed(key_length=2048, verbose=False)
    assert np.allclose(errors, plaintext_rounds(fed.N_ROUNDS), rtol=1e-7)
    assert ["%.2f" % e for e in errors] == ["3775.50"] * 5
