#!/usr/bin/env python3
"""The value codec of plain batches (csrc/value_codec.h; Engine.values_encode_dev / raw_decrypt_decode_chunks) against the host
encoding and decoding it replaces, one key width per process, 2^20 values by default.  The host route is the SAME build with
keys.VALUE_CODEC_DEVICE_MIN out of reach (encrypt) or the engine reporting no codec (decrypt): what the parent commit does.

  (1) the two kernels alone on resident operands, --inner launches per timing and one synchronisation, beside a
      device-to-device copy of the same number of bytes.  Bytes: 8 per value + 4 n_limbs per row + 1 status byte (+ 4 per
      exponent for floats), each counted once
  (2) encrypt_batch(device=True) of int64, float64 at its natural exponents and float64 with precision=1e-6 on three obfuscator
      routes: a filled pool (refilled outside the timing), short obfuscators with the device draw, the default fresh route
  (3) decrypt_batch as a list, as_array on the host route, as_array on the device route, for int64 and float64 rows
  (4) the encoding step alone (host: encode_signed + signed_to_limbs + upload; device: values_encode_dev) from 2^8 to 2^16
      values: the crossover behind keys.VALUE_CODEC_DEVICE_MIN

Host and device routes alternate within one process; --repeats timed rounds after one warm-up round that is dropped (the
default fresh route and the host encoding under a precision, which take seconds per call, run --slow-repeats rounds and say so).
Every comparison carries `meets`: the device route's slowest repeat is not slower than the host route's fastest.
Wall clock (time.perf_counter) around calls that end in a stream synchronisation.

  python tools/bench_value_codec.py --key-bits 2048 > part.json      (profiles/r15_value_codec.json joins the three widths)"""
import argparse
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--key-bits", type=int, default=2048)
ap.add_argument("--log2-values", type=int, default=20)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--slow-repeats", type=int, default=2)
ap.add_argument("--inner", type=int, default=20)
ap.add_argument("--skip", nargs="*", default=[], choices=["kernels", "encrypt", "decrypt", "sweep"])
args = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "python-paillier_amd")):
    sys.path.insert(0, p)


def main():
    import numpy as np
    from phe import keys, paillier
    from phe._device import DeviceArray
    from phe.codec import EncodedNumber

    count = 1 << args.log2_values
    g = json.load(open(os.path.join(ROOT, "tests", "golden", "paillier_%d.json" % args.key_bits)))
    pub = paillier.PaillierPublicKey(int(g["n"], 16))
    priv = paillier.PaillierPrivateKey(pub, int(g["p"], 16), int(g["q"], 16))
    eng = priv._get_engine()
    ctx = eng.ctx
    assert eng.has_value_codec() and pub._get_engine().has_value_codec()
    res = {"key_bits": args.key_bits, "values": count, "repeats": args.repeats, "slow_repeats": args.slow_repeats,
           "condition": "meets = the device route's slowest repeat <= the host route's fastest repeat",
           "timing": "time.perf_counter around calls that end in one stream synchronisation; host and device routes alternate"}
    rs = np.random.Generator(np.random.PCG64(15))
    data = {"int64": (rs.integers(-(1 << 40), 1 << 40, count), None),
            "float64": (rs.standard_normal(count), None),
            "float64_precision_1e-6": (rs.standard_normal(count) * 1000.0, 1e-6)}

    def summary(times):
        return {"ms_best": round(min(times) * 1e3, 3), "ms_worst": round(max(times) * 1e3, 3),
                "ms_median": round(sorted(times)[len(times) // 2] * 1e3, 3), "ms": [round(t * 1e3, 3) for t in times]}

    def repeat(fns, repeats, before=None, warm=True):
        times = {k: [] for k in fns}
        for rep in range(repeats + (1 if warm else 0)):                   # (the first round warms up and is dropped)
            for k, fn in fns.items():
                if before:
                    before()
                t0 = time.perf_counter()
                fn()
                if rep or not warm:
                    times[k].append(time.perf_counter() - t0)
        return times

    def compare(t, host="host", device="device"):
        out = {k: summary(v) for k, v in t.items()}
        out["meets"] = bool(max(t[device]) <= min(t[host]))
        out["host_best_over_device_worst"] = round(min(t[host]) / max(t[device]), 2)
        return out

    med = lambda ts: sorted(ts)[len(ts) // 2]
    exponent = EncodedNumber._natural_exponent(0.0, 1e-6)

    # ---- (1) the kernels alone ----------------------------------------------------------------------------------------------
    if "kernels" not in args.skip:
        m_dev = DeviceArray(ctx, count, eng.n_limbs)
        stat, e_dev, out_v = DeviceArray(ctx, (count + 3) // 4, 1), DeviceArray(ctx, count, 1), DeviceArray(ctx, count, 2)
        row_bytes = 4 * eng.n_limbs * count
        words = {k: DeviceArray.from_host(ctx, np.ascontiguousarray(v).view(np.uint32)) for k, (v, _) in data.items()}

        def many(fn):
            def run():
                for _ in range(args.inner):
                    fn()
                ctx.sync()
            return run
        copy_bytes = row_bytes + 9 * count
        src, dst = DeviceArray(ctx, (copy_bytes // 2 + 3) // 4, 1), DeviceArray(ctx, (copy_bytes // 2 + 3) // 4, 1)
        fns = {"encode_int64": many(lambda: ctx.values_encode_dev(words["int64"].ptr, count, 0, 0, m_dev.ptr, None, stat.ptr)),
               "encode_float64": many(lambda: ctx.values_encode_dev(words["float64"].ptr, count, 2, 0, m_dev.ptr, e_dev.ptr, stat.ptr)),
               "encode_float64_precision": many(lambda: ctx.values_encode_dev(words["float64_precision_1e-6"].ptr, count, 3, exponent,
                                                                              m_dev.ptr, None, stat.ptr)),
               "decode_int64": None, "decode_float64": None,
               # a copy moves every byte twice (read + write): half of the bytes copied = the bytes moved
               "d2d_copy_same_bytes": many(lambda: ctx.d2d(dst.ptr, src.ptr, copy_bytes // 2))}
        ints_dev, _ = eng.values_encode_dev(data["int64"][0])
        flo_dev, flo_exps = eng.values_encode_dev(data["float64_precision_1e-6"][0], exponent)
        fe_dev = DeviceArray.from_host(ctx, np.full(count, flo_exps, np.int32).view(np.uint32))
        fns["decode_int64"] = many(lambda: ctx.values_decode_dev(ints_dev.ptr, count, 0, None, out_v.ptr, stat.ptr))
        fns["decode_float64"] = many(lambda: ctx.values_decode_dev(flo_dev.ptr, count, 1, fe_dev.ptr, out_v.ptr, stat.ptr))
        t = repeat(fns, args.repeats)
        per = lambda ts: [x / args.inner for x in ts]
        nbytes = {"encode_int64": copy_bytes, "encode_float64": copy_bytes + 4 * count, "encode_float64_precision": copy_bytes,
                  "decode_int64": copy_bytes, "decode_float64": copy_bytes + 4 * count, "d2d_copy_same_bytes": copy_bytes}
        res["kernels"] = {"launches_per_timing": args.inner}
        for k in fns:
            res["kernels"][k] = dict(summary(per(t[k])), bytes=nbytes[k], gb_per_s_median=round(nbytes[k] / med(per(t[k])) / 1e9, 1))
        copy_rate = copy_bytes / med(per(t["d2d_copy_same_bytes"]))
        for k in fns:
            res["kernels"][k]["of_the_copy_rate"] = round(nbytes[k] / med(per(t[k])) / copy_rate, 2)
        back, status = eng.values_decode_dev(ints_dev, 0)
        res["kernels"]["round_trip_ok"] = bool(np.array_equal(back.view(np.int64), data["int64"][0]) and not status.any())
        del m_dev, ints_dev, flo_dev, src, dst, words

    def route(minimum, fn):
        def run():
            keep, keys.VALUE_CODEC_DEVICE_MIN = keys.VALUE_CODEC_DEVICE_MIN, minimum
            try:
                return fn()
            finally:
                keys.VALUE_CODEC_DEVICE_MIN = keep
        return run

    # ---- (2) encrypt_batch(device=True) -------------------------------------------------------------------------------------
    if "encrypt" not in args.skip:
        res["encrypt"] = {}

        def refill():
            # the pool is filled outside the timing, from short obfuscators, which stay on for this route (what the rows were
            # made of does not matter to the online part: one pair product per row, and a filled pool is taken first)
            pub.discard_obfuscators()
            pub.precompute_obfuscators(count)
        for name in ("filled_pool", "short_obfuscators_device_draw", "default_fresh"):
            pub.discard_obfuscators()
            before = None
            if name != "default_fresh":
                pub.enable_short_obfuscators(device_rng=True)
            if name == "filled_pool":
                before = refill
            out = res["encrypt"][name] = {}
            for kind, (values, precision) in data.items():
                call = lambda: pub.encrypt_batch(values, precision=precision, device=True)
                slow_host = precision is not None                          # the host walks the array with one Fraction per element
                repeats = args.slow_repeats if name == "default_fresh" else args.repeats
                if slow_host:
                    t = repeat({"device": route(0, call)}, repeats, before)
                    t.update(repeat({"host": route(1 << 62, call)}, args.slow_repeats, before, warm=False))
                else:
                    t = repeat({"host": route(1 << 62, call), "device": route(0, call)}, repeats, before)
                out[kind] = compare(t)
                out[kind]["repeats"] = {k: len(v) for k, v in t.items()}
            pub.disable_short_obfuscators()
            pub.discard_obfuscators()

    # ---- (3) decrypt_batch --------------------------------------------------------------------------------------------------
    if "decrypt" not in args.skip:
        res["decrypt"] = {}
        pub.enable_short_obfuscators(device_rng=True)
        vectors = {"int64": pub.encrypt_batch(data["int64"][0], device=True),
                   "float64_precision_1e-6": pub.encrypt_batch(data["float64_precision_1e-6"][0], precision=1e-6, device=True)}
        pub.disable_short_obfuscators()

        def on_host(vec):
            def run():
                eng.has_value_codec = lambda: False                       # (an instance attribute: the class method comes back below)
                try:
                    return priv.decrypt_batch(vec, as_array=True)
                finally:
                    del eng.has_value_codec
            return run
        for kind, vec in vectors.items():
            t = repeat({"list": lambda: priv.decrypt_batch(vec), "as_array_host": on_host(vec),
                        "as_array_device": lambda: priv.decrypt_batch(vec, as_array=True)}, args.repeats)
            out = res["decrypt"][kind] = {k: summary(v) for k, v in t.items()}
            for host in ("list", "as_array_host"):
                out["meets_against_" + host] = bool(max(t["as_array_device"]) <= min(t[host]))
                out[host + "_best_over_device_worst"] = round(min(t[host]) / max(t["as_array_device"]), 2)
            same = on_host(vec)()
            out["same_bits"] = bool(np.array_equal(same.view(np.uint64), priv.decrypt_batch(vec, as_array=True).view(np.uint64)))
        del vectors

    # ---- (4) the encoding step alone, 2^8 .. 2^16 ---------------------------------------------------------------------------
    if "sweep" not in args.skip:
        res["sweep"] = {}

        def host_encode(values):
            mag, neg, _ = EncodedNumber.encode_signed(values)
            m = DeviceArray.from_host(ctx, EncodedNumber.signed_to_limbs(pub, mag, neg, eng.n_limbs))
            ctx.sync()
            return m
        crossover = {}
        for kind in ("int64", "float64"):
            out = res["sweep"][kind] = {}
            meets = {}
            for log2 in range(8, 17):
                values = data[kind][0][:1 << log2]
                t = repeat({"host": lambda: host_encode(values), "device": lambda: eng.values_encode_dev(values)}, args.repeats)
                out["2^%d" % log2] = compare(t)
                meets[log2] = out["2^%d" % log2]["meets"]
            # the least size from which the condition holds at every larger size measured
            good = [log2 for log2 in range(8, 17) if all(meets[k] for k in range(log2, 17))]
            crossover[kind] = (1 << good[0]) if good else None
        res["sweep"]["crossover"] = crossover
        res["sweep"]["VALUE_CODEC_DEVICE_MIN_in_this_build"] = keys.VALUE_CODEC_DEVICE_MIN
    print(json.dumps(res))


if __name__ == "__main__":
    main()
