#!/usr/bin/env python3
"""The draw of the short obfuscator exponents on the device (enable_short_obfuscators(device_rng=True); csrc/chacha_rows.h)
against the host draw it replaces, 2^20 values by default, keys of 1024, 2048 and 3072 bits (rho of half the modulus length),
results resident.  Per key width, in ONE process and one run:

  (a) the draw alone: random_bits_limbs into a reused host buffer plus its upload, against Engine.random_bits_dev (a seed from the
      kernel CSPRNG, the keystream kernel, one synchronisation); ms and GB/s of exponent bytes
  (b) the public call: encrypt_batch(device=True) with device_rng off and on
  (c) precompute_obfuscators(2^20) with device_rng off and on
  (d) the comb kernel alone on resident exponents: the floor of (b), and what the keystream kernel is a share of

The comparison is always host route against device route of the SAME run.  The one condition recorded per width and comparison:
the device route's slowest repeat is not slower than the host route's fastest ("device_max_le_host_min").

Wall clock (time.perf_counter) around calls that end in one stream synchronisation; --repeats runs each, the sides of a comparison
alternating (one more round warms up and is dropped); min - max reported.

  python tools/bench_device_rng.py [--keys 1024,2048,3072] [--log2-values 20] [--repeats 5]  > profiles/rNN_device_rng.json"""
import argparse
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--keys", default="1024,2048,3072")
ap.add_argument("--log2-values", type=int, default=20)
ap.add_argument("--repeats", type=int, default=5)
args = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "python-paillier_amd")):
    sys.path.insert(0, p)


def main():
    import numpy as np
    from phe import _engine, paillier
    from phe._device import DeviceArray

    count = 1 << args.log2_values

    def summary(times):
        return {"ms_min": round(min(times) * 1e3, 3), "ms_max": round(max(times) * 1e3, 3),
                "ms": [round(t * 1e3, 3) for t in times]}

    def repeat(fns, repeats=args.repeats):
        times = {k: [] for k in fns}
        for rep in range(repeats + 1):                                # (the first round warms up and is dropped)
            for k, fn in fns.items():
                t0 = time.perf_counter()
                fn()
                if rep:
                    times[k].append(time.perf_counter() - t0)
        return times

    def compare(host, device):
        return {"host": summary(host), "device": summary(device),
                "speedup": {"min": round(min(host) / max(device), 2), "max": round(max(host) / min(device), 2)},
                "device_max_le_host_min": bool(max(device) <= min(host))}

    def key(bits):
        g = json.load(open(os.path.join(ROOT, "tests", "golden", "paillier_%d.json" % bits)))
        return paillier.PaillierPublicKey(int(g["n"], 16))     # public keys only: the party that encrypts holds no private key

    res = {"values": count, "repeats": args.repeats,
           "timing": "time.perf_counter around calls that end in one stream synchronisation; the sides of a comparison alternate; "
                     "min - max of the repeats; host and device route in the same run",
           "keys": {}}
    values = np.random.Generator(np.random.PCG64(13)).integers(-(1 << 40), 1 << 40, count)
    for kb in [int(b) for b in args.keys.split(",")]:
        host_key, dev_key = key(kb), key(kb)                   # two keys, two contexts: device_rng off / on, the same h_s
        x = 12345678901234567891
        host_key.enable_short_obfuscators(x=x)
        dev_key.enable_short_obfuscators(x=x, device_rng=True)
        bits = host_key.short_obfuscator_bits
        el = (bits + 31) // 32
        eng = dev_key._get_engine()
        ctx = eng.ctx
        info = eng.short_table_info()
        host_key._get_engine().short_table_info()                     # (both tables built before anything is timed)
        nbytes = count * el * 4
        row = {"exp_bits": bits, "exp_limbs": el, "exponent_bytes": nbytes, "window": info["window"], "positions": info["positions"]}

        # ---- (a) the draw alone ----------------------------------------------------------------------------------------------------
        rho = np.empty((count, el), np.uint32)

        def host_draw():
            _engine.random_bits_limbs(bits, count, el, out=rho)
            DeviceArray.from_host(ctx, rho)                           # (a synchronous copy)

        def device_draw():
            eng.random_bits_dev(bits, count, el)
            ctx.sync()
        t = repeat({"host": host_draw, "device": device_draw})
        row["draw"] = compare(t["host"], t["device"])
        row["draw"]["GB_per_s"] = {k: round(nbytes / min(v) / 1e9, 2) for k, v in t.items()}
        split = repeat({"draw": lambda: _engine.random_bits_limbs(bits, count, el, out=rho),
                        "upload": lambda: DeviceArray.from_host(ctx, rho)})
        row["draw"]["host_phases"] = {k: summary(v) for k, v in split.items()}

        # ---- (d) the comb kernel alone ---------------------------------------------------------------------------------------------
        e_dev = eng.random_bits_dev(bits, count, el)
        m_dev = DeviceArray.from_host(ctx, np.zeros((count, eng.n_limbs), np.uint32))
        out = DeviceArray(ctx, count, eng.ct_limbs)

        def comb():
            ctx.fixed_base_pow_dev(e_dev.ptr, el, None, False, m_dev.ptr, out.ptr, False, count)
            ctx.sync()
        tk = repeat({"kernel": comb})["kernel"]
        row["comb_kernel_alone"] = summary(tk)
        row["device_draw_share_of_comb_kernel"] = round(min(t["device"]) / min(tk), 4)
        del e_dev, m_dev, out

        # ---- (b) the public call ---------------------------------------------------------------------------------------------------
        def call(k):
            def run():
                k.discard_obfuscators()
                k.encrypt_batch(values, device=True)
            return run
        t = repeat({"host": call(host_key), "device": call(dev_key)})
        row["encrypt_batch"] = compare(t["host"], t["device"])
        row["encrypt_batch"]["device_over_comb_kernel_ms"] = round((min(t["device"]) - min(tk)) * 1e3, 3)

        # ---- (c) the pool ----------------------------------------------------------------------------------------------------------
        def fill(k):
            def run():
                k.discard_obfuscators()
                k.precompute_obfuscators(count)
            return run
        t = repeat({"host": fill(host_key), "device": fill(dev_key)})
        row["precompute_obfuscators"] = compare(t["host"], t["device"])
        host_key.discard_obfuscators()
        dev_key.discard_obfuscators()
        host_key.disable_short_obfuscators()
        dev_key.disable_short_obfuscators()
        res["keys"][str(kb)] = row
        del host_key, dev_key, eng, ctx
    res["condition_met_everywhere"] = all(row[k]["device_max_le_host_min"] for row in res["keys"].values()
                                          for k in ("draw", "encrypt_batch", "precompute_obfuscators"))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
