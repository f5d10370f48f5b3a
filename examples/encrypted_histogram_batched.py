#!/usr/bin/env python3
"""Gradient histograms for one tree node of federated gradient boosting — batched, on the GPU backend.

The protocol of vertically federated boosting: the party that holds the labels encrypts the gradient of every sample and
sends the ciphertexts to a party that holds other features of the same samples.  To propose splits that party needs, for
each of ITS features and each bin of that feature, the sum of the gradients of the node's samples that fall into the bin
— sums of ciphertexts by group, which it computes without being able to decrypt any of them — and sends the encrypted
histograms back.  With the reference that is one chain of EncryptedNumber `+` per (feature, bin); here it is ONE call:

    hist = enc_gradients.segment_sum(bins, n_bins)     # bins: (features, samples) bin numbers, -1 = not in this node

i.e. one limb group per (feature, bin) walks its samples with the running product in registers: one pair product per
sample and feature.  The label holder decrypts the histograms; they equal np.bincount on the plaintext gradients.

A split at threshold b sends the bins 0 .. b to the left child, so what the label holder scores is, per feature, the RUNNING
sum over the bins — which the feature holder can form on the ciphertexts as well, before they go back:

    left = hist.cumsum(block=n_bins)                    # per feature: sum of the gradients left of every threshold

The sums are small next to a plaintext of the key (a 53-bit mantissa at the vector's exponent, plus the bits that adding the
samples adds), so the feature holder packs several of them into every ciphertext it sends back, and the label holder pays one
decrypt per packed row instead of one per number:

    packed = left.pack(slots, slot_bits)                # slot j of row b: sum number b * slots + j
    sums = privkey.decrypt_packed(packed, slots, slot_bits, count=len(left))

python examples/encrypted_histogram_batched.py [key_length] [samples] [features] [bins]
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "python-paillier_amd"))

import phe as paillier  # noqa: E402


def run(key_length=1024, n_samples=2048, n_features=4, n_bins=16, device=None, verbose=True):
    rng = np.random.RandomState(7)
    # the label holder: logistic-loss gradients p - y of the current model (here: of a constant prediction plus noise)
    y = rng.randint(0, 2, n_samples)
    gradients = 1.0 / (1.0 + np.exp(-rng.randn(n_samples))) - y
    # the feature holder: its features binned by quantiles, and the samples of the node being split (the others get -1)
    features = rng.randn(n_features, n_samples)
    bins = np.stack([np.searchsorted(np.quantile(f, np.linspace(0, 1, n_bins + 1)[1:-1]), f) for f in features])
    in_node = rng.rand(n_samples) < 0.6
    bins[:, ~in_node] = -1

    pubkey, privkey = paillier.generate_paillier_keypair(n_length=key_length)
    if device is None:
        device = hasattr(pubkey._get_engine().ctx, "encrypt_dev")
    t0 = time.perf_counter()
    enc_gradients = pubkey.encrypt_batch(gradients, device=device)             # label holder, one launch
    t1 = time.perf_counter()
    enc_hist = enc_gradients.segment_sum(bins, n_bins)                          # feature holder: all features and bins at once
    t2 = time.perf_counter()
    hist = np.array(privkey.decrypt_batch(enc_hist)).reshape(n_features, n_bins)     # label holder, one launch
    t3 = time.perf_counter()
    enc_left = enc_hist.cumsum(block=n_bins)                                    # feature holder: left-child sums of every threshold
    t4 = time.perf_counter()
    left = np.array(privkey.decrypt_batch(enc_left)).reshape(n_features, n_bins)
    # the feature holder packs the sums before they go back.  The exponent of the rows is public and |gradient| < 1, so a sum of at
    # most n_samples gradients is below n_samples * BASE^-exponent in magnitude: that many bits, and one for the sign, per slot
    t5 = time.perf_counter()
    slot_bits = 1 + int(np.ceil(np.log2(n_samples))) + 4 * -min(enc_left.exponents)
    slots = (pubkey.max_int.bit_length() - 1) // slot_bits
    enc_packed = enc_left.pack(slots, slot_bits)
    t6 = time.perf_counter()
    unpacked = np.array(privkey.decrypt_packed(enc_packed, slots, slot_bits, count=len(enc_left))).reshape(n_features, n_bins)
    t7 = time.perf_counter()

    clear = np.stack([np.bincount(b[in_node], weights=gradients[in_node], minlength=n_bins) for b in bins])
    err = float(np.max(np.abs(hist - clear)))
    err_left = float(np.max(np.abs(left - np.cumsum(clear, axis=1))))
    if verbose:
        print("key %d bits, %d samples (%d in the node), %d features x %d bins" % (key_length, n_samples, in_node.sum(), n_features, n_bins))
        print("encrypt the gradients:        %.3f s" % (t1 - t0))
        print("encrypted histograms:         %.3f s  (%.2e sample-feature additions/s)"
              % (t2 - t1, n_features * in_node.sum() / (t2 - t1)))
        print("decrypt the histograms:       %.3f s" % (t3 - t2))
        print("max |histogram - np.bincount| %.3e" % err)
        print("encrypted left-child sums:    %.3f s  (cumsum over the %d bins of every feature)" % (t4 - t3, n_bins))
        print("max |left sums - np.cumsum|   %.3e" % err_left)
        print("pack the left-child sums:     %.3f s  (%d ciphertexts of %d slots x %d bits instead of %d)"
              % (t6 - t5, len(enc_packed), slots, slot_bits, len(enc_left)))
        print("decrypt the packed sums:      %.3f s  (max |unpacked - decrypted one by one| %.3e)"
              % (t7 - t6, float(np.max(np.abs(unpacked - left)))))
    assert np.array_equal(unpacked, left)
    assert err < 1e-9, err
    assert err_left < 1e-9, err_left
    return hist, clear


if __name__ == "__main__":
    run(*[int(a) for a in sys.argv[1:]])
