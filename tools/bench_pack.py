#!/usr/bin/env python3
"""Ciphertext packing (EncryptedVector.pack / PaillierPrivateKey.decrypt_packed; csrc/segment_core.h segment_pack_body) on
resident rows, 2048-bit key and 2^20 rows by default:

  (a) the kernel alone: pair form in and out at (slots, slot_bits) = (31, 64) and (15, 128); canonical residues in and out
      (conversion as the rows are read, exit from the pair form) at (31, 64)
  (b) the public call vec.pack(31, 64) on the vector in the pair form and as canonical residues
  (c) the kernel against the composition a user has without it, (vec * weights).segment_sum(ids) with weights
      1 << (B * (i % S)) and ids i // S, on the first 2^--log2-compose rows (every row raised to its own power: seconds at
      2^16 rows), interleaved, the same bits required; beside the measured ratio the one that the squaring and product
      counts of the two routes predict, in multiply-adds (a pair squaring 4 L H, a pair product 5 L H: csrc/split_core.h)
  (d) the key holder's side: decrypt_batch of the 2^20 numbers against decrypt_packed of their 2^20 / 31 packed rows, and the
      host unpacking of the decrypted rows alone (PaillierPrivateKey._unpack_plain)

Wall clock (time.perf_counter) around calls that end in a stream synchronisation; --repeats runs each, interleaved where two
routes are compared (one more round warms up and is dropped); rows/s counts INPUT rows (values).

  python tools/bench_pack.py [--key-bits 2048] [--log2-rows 20] [--log2-compose 16] [--repeats 5]  > profiles/rNN_pack.json"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "python-paillier_amd")):
    sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--key-bits", type=int, default=2048)
    ap.add_argument("--log2-rows", type=int, default=20)
    ap.add_argument("--log2-compose", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    import numpy as np
    from phe import paillier

    n_rows = 1 << args.log2_rows
    g = json.load(open(os.path.join(ROOT, "tests", "golden", "paillier_%d.json" % args.key_bits)))
    pub = paillier.PaillierPublicKey(int(g["n"], 16))
    priv = paillier.PaillierPrivateKey(pub, int(g["p"], 16), int(g["q"], 16))
    eng = pub._get_engine()
    assert eng.has_segment_pack(), "no packing kernel for this key width"
    bound = pub.max_int.bit_length() - 1
    wide, narrow = (bound // 64, 64), (bound // 128, 128)
    res = {"key_bits": args.key_bits, "rows": n_rows, "repeats": args.repeats,
           "timing": "time.perf_counter around calls that end in one stream synchronisation; interleaved where compared"}
    rs = np.random.Generator(np.random.PCG64(10))
    values = rs.integers(-(1 << 40), 1 << 40, n_rows)                     # sums of a histogram: well inside a 64-bit slot
    vec = pub.encrypt_batch(values, device=True)
    vec._limbs                                                            # (settled canonical residues)
    pair = vec.to_pair()
    store = vec._store

    def wall(fn):
        t0 = time.perf_counter()
        out = fn()
        return time.perf_counter() - t0, out

    def summary(times, rows=n_rows):
        return {"rows_per_s_best": rows / min(times), "rows_per_s_worst": rows / max(times),
                "rows_per_s_median": rows / sorted(times)[len(times) // 2], "slowest_over_fastest": max(times) / min(times),
                "ms": [round(t * 1e3, 3) for t in times]}

    def repeat(fns):
        times = {k: [] for k in fns}
        for rep in range(args.repeats + 1):                               # (the first round warms up and is dropped)
            for k, fn in fns.items():
                t, _ = wall(fn)
                if rep:
                    times[k].append(t)
        return times

    # ---- (a) the kernel alone, (b) the public call ----------------------------------------------------------------------------------------
    t = repeat({
        "pair_%dx%d" % wide: lambda: eng.segment_pack_dev(pair._store, True, *wide, want_pair=True),
        "pair_%dx%d" % narrow: lambda: eng.segment_pack_dev(pair._store, True, *narrow, want_pair=True),
        "residues_%dx%d" % wide: lambda: eng.segment_pack_dev(store, False, *wide),
        "api_pair_%dx%d" % wide: lambda: pair.pack(*wide),
        "api_residues_%dx%d" % wide: lambda: vec.pack(*wide),
    })
    res["kernel"] = {k: summary(v) for k, v in t.items() if not k.startswith("api_")}
    res["public_call"] = {k[4:]: summary(v) for k, v in t.items() if k.startswith("api_")}
    eng.segment_pack_dev(pair._store, True, *wide, want_pair=True)
    res["kernel_geom_pub"] = eng.ctx.last_launch()["geom_pub"]

    # ---- (c) the kernel against (vec * weights).segment_sum(ids) ---------------------------------------------------------------------------
    S, B = wide
    m = min(n_rows, 1 << args.log2_compose)
    part = vec[:m]
    index = np.arange(m, dtype=np.int64)
    weights = [1 << (B * j) for j in (index % S).tolist()]
    ids = index // S
    t = repeat({"kernel": lambda: part.pack(S, B), "composition": lambda: (part * weights).segment_sum(ids)})
    med = lambda ts: sorted(ts)[len(ts) // 2]
    same = bool(np.array_equal(part.pack(S, B)._limbs.to_host(), (part * weights).segment_sum(ids)._limbs.to_host()))
    # multiply-adds in units of L H: Horner B squarings per row but the top one of a task and one product; the composition raises
    # row j to 2^(B j) (B j squarings, no product: one set bit) and joins the rows of a task with one product each
    horner = 4.0 * B * (S - 1) / S + 5.0
    composed = 4.0 * B * (S - 1) / 2.0 + 5.0
    res["against_composition"] = {"rows": m, "slots": S, "slot_bits": B, "kernel": summary(t["kernel"], m),
                                  "composition": summary(t["composition"], m),
                                  "speedup_median": med(t["composition"]) / med(t["kernel"]),
                                  "slowest_kernel_beats_fastest_composition": max(t["kernel"]) < min(t["composition"]),
                                  "speedup_predicted_by_operation_counts": composed / horner, "same_bits": same}

    # ---- (d) the key holder: one decrypt per number against one per packed row --------------------------------------------------------------
    packed = vec.pack(S, B)
    t = repeat({"decrypt_batch": lambda: priv.decrypt_batch(vec), "decrypt_packed": lambda: priv.decrypt_packed(packed, S, B, count=n_rows)})
    plain = priv._get_engine().raw_decrypt_dev(packed._limbs)
    exps = packed.exponent_array
    tu = repeat({"unpack": lambda: priv._unpack_plain(plain, exps, S, B, None)})
    ok = priv.decrypt_packed(packed, S, B, count=n_rows) == values.tolist()
    res["key_holder"] = {"packed_rows": len(packed), "decrypt_batch": summary(t["decrypt_batch"]),
                         "decrypt_packed": summary(t["decrypt_packed"]), "host_unpack_alone": summary(tu["unpack"]),
                         "speedup_median": med(t["decrypt_batch"]) / med(t["decrypt_packed"]),
                         "values_come_back": bool(ok)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
