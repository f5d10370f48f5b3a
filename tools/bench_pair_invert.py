#!/usr/bin/env python3
"""Inversion on pair rows (csrc/pair_invert.h; Engine.pair_invert_dev) against the route it replaces, one key width per process,
pair-resident vectors of 2^12, 2^16 and 2^20 rows by default.  The parent's route is the SAME build with the engine reporting
no pair inversion: from_pair_dev -> invert_dev -> to_pair_dev for the inversion alone, and for the public calls whatever
EncryptedVector does without it (the rows out of the form, the product tree of phe_hip_invert_dev, powmod_dev).

  (1) the inversion alone, pair rows in and out
  (2) -v, a - b and v.dot(w) with signed weights on pair-resident vectors (the dot with PAIR_INVERT_MIN_ROWS at 0, so that the
      form is measured at every length: the threshold is read off this)
  (3) the block size of the walks, {4, 8, 16, 32, 64}, at every size (the shipped PAIR_INVERT_BLOCK_ROWS is the fastest at the
      largest size)
  (4) for information: canonical rows in and out — invert_dev against to_pair_dev + the new inversion + from_pair_dev

The two routes alternate within one process; --repeats timed rounds after one warm-up round that is dropped.  Every comparison
carries `meets`: the new route's slowest repeat is not slower than the parent route's fastest.  `predicted` is the ratio of the
operation counts (3 x 16 against 3 x 5 limb-product units per row, include/phe_hip.h), printed beside the measurement; it is no
bar.  Wall clock (time.perf_counter) around calls that end in a stream synchronisation.

  python tools/bench_pair_invert.py --key-bits 2048 > part.json      (profiles/r16_pair_invert.json joins the three widths)"""
import argparse
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--key-bits", type=int, default=2048)
ap.add_argument("--log2-rows", type=int, nargs="*", default=[12, 16, 20])
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--blocks", type=int, nargs="*", default=[4, 8, 16, 32, 64])
ap.add_argument("--skip", nargs="*", default=[], choices=["inversion", "public", "blocks", "canonical"])
args = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "python-paillier_amd")):
    sys.path.insert(0, p)


def main():
    import numpy as np
    from phe import _engine, paillier
    from phe._device import DeviceArray
    from phe.ciphertext import EncryptedVector

    g = json.load(open(os.path.join(ROOT, "tests", "golden", "paillier_%d.json" % args.key_bits)))
    pub = paillier.PaillierPublicKey(int(g["n"], 16))
    eng = pub._get_engine()
    ctx = eng.ctx
    assert eng.has_pair_invert()
    res = {"key_bits": args.key_bits, "repeats": args.repeats, "block_rows_in_this_build": _engine.PAIR_INVERT_BLOCK_ROWS,
           "dot_min_rows_in_this_build": _engine.PAIR_INVERT_MIN_ROWS,
           "condition": "meets = the new route's slowest repeat <= the parent route's fastest repeat",
           "predicted": "48 / 15 = 3.2 limb-product units per row for the inversion itself; more with the saved conversions",
           "timing": "time.perf_counter around calls that end in one stream synchronisation; the routes alternate", "sizes": {}}
    rs = np.random.Generator(np.random.PCG64(16))

    def summary(times):
        return {"ms_best": round(min(times) * 1e3, 3), "ms_worst": round(max(times) * 1e3, 3), "ms": [round(t * 1e3, 3) for t in times]}

    def repeat(fns):
        times = {k: [] for k in fns}
        for rep in range(args.repeats + 1):                               # (the first round warms up and is dropped)
            for k, fn in fns.items():
                t0 = time.perf_counter()
                fn()
                ctx.sync()
                if rep:
                    times[k].append(time.perf_counter() - t0)
        return times

    def compare(t, parent="parent", new="new"):
        out = {k: summary(v) for k, v in t.items()}
        out["meets"] = bool(max(t[new]) <= min(t[parent]))
        out["parent_best_over_new_worst"] = round(min(t[parent]) / max(t[new]), 2)
        out["parent_best_over_new_best"] = round(min(t[parent]) / min(t[new]), 2)
        return out

    def parent(fn):
        def run():
            eng.has_pair_invert = lambda: False                           # (an instance attribute: the class method comes back below)
            try:
                return fn()
            finally:
                del eng.has_pair_invert
        return run

    def random_rows(count):
        words = rs.integers(0, 1 << 32, size=(count, eng.ct_limbs), dtype=np.uint64).astype(np.uint32)
        words[:, -1] = 0                                                  # below n^2; units but for a chance of 2^-500
        return eng.upload_cipher(words)

    for log2 in args.log2_rows:
        count = 1 << log2
        out = res["sizes"]["2^%d" % log2] = {"rows": count}
        canon = random_rows(count)
        store = eng.to_pair_dev(canon)

        def parent_inversion():
            c = eng.from_pair_dev(store)
            inv = DeviceArray(ctx, count, eng.ct_limbs)
            ctx.invert_dev(c.ptr, inv.ptr, count)
            return eng.to_pair_dev(inv)
        if "inversion" not in args.skip:
            t = repeat({"parent": parent_inversion, "new": lambda: eng.pair_invert_dev(store)})
            out["inversion"] = compare(t)
            a, b = eng.from_pair_dev(parent_inversion()).to_host(), eng.from_pair_dev(eng.pair_invert_dev(store)).to_host()
            out["inversion"]["same_bits"] = bool(np.array_equal(a, b))
        if "blocks" not in args.skip:
            t = repeat({str(b): (lambda b=b: eng.pair_invert_dev(store, block=b)) for b in args.blocks})
            out["blocks"] = {k: summary(v) for k, v in t.items()}
            out["blocks"]["fastest_by_best"] = int(min(t, key=lambda k: min(t[k])))
            out["blocks"]["fastest_by_worst"] = int(min(t, key=lambda k: max(t[k])))
        if "canonical" not in args.skip:
            def through_the_form():
                return eng.from_pair_dev(eng.pair_invert_dev(eng.to_pair_dev(canon)))

            def tree():
                inv = DeviceArray(ctx, count, eng.ct_limbs)
                ctx.invert_dev(canon.ptr, inv.ptr, count)
                return inv
            out["canonical_rows_information_only"] = compare(repeat({"parent": tree, "new": through_the_form}))
        if "public" not in args.skip:
            other = eng.to_pair_dev(random_rows(count))
            exps = np.zeros(count, dtype=np.int64)
            # (a vector that the parent's route has read is no longer in the form: every call gets its own view of the pair rows)
            v = lambda: EncryptedVector(pub, store, exps, _pair=True)
            w = lambda: EncryptedVector(pub, other, exps, _pair=True)
            weights = rs.standard_normal(count)
            def dot():                                                    # (the form at every length: what the threshold is set from)
                keep, _engine.PAIR_INVERT_MIN_ROWS = _engine.PAIR_INVERT_MIN_ROWS, 0
                try:
                    return v().dot(weights)
                finally:
                    _engine.PAIR_INVERT_MIN_ROWS = keep
            for name, fn in (("neg", lambda: -v()), ("sub", lambda: v() - w()), ("dot_signed", dot)):
                out[name] = compare(repeat({"parent": parent(fn), "new": fn}))
            out["dot_signed"]["public_call_takes_the_form"] = bool(count >= _engine.PAIR_INVERT_MIN_ROWS)
            new_rows, parent_rows = -v(), parent(lambda: -v())()
            out["neg"]["new_in_form"], out["neg"]["parent_in_form"] = bool(new_rows._pair), bool(parent_rows._pair)
            out["neg"]["same_bits"] = bool(np.array_equal(new_rows._plain_rows().to_host(), parent_rows._plain_rows().to_host()))
            del other
        del canon, store
        ctx.release_scratch()
    res["does_not_meet"] = [size + " " + name for size, s in res["sizes"].items()
                            for name in ("inversion", "neg", "sub", "dot_signed") if name in s and not s[name]["meets"]]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
