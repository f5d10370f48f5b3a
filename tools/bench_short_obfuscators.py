#!/usr/bin/env python3
"""Short-exponent obfuscators (PaillierPublicKey.enable_short_obfuscators; csrc/fixed_base.h), 2048-bit key, the default
exponent length and 2^20 int64 values by default, results resident:

  (a) the public call: encrypt_batch with short obfuscators on against the same call with them off (the path of a build without
      them), alternating in one process; with the phases of the short route alone: the draw of rho (host, /dev/urandom), its
      upload, the kernel on resident exponents
  (b) the kernel alone on resident exponents: rows/s and pair products/s (positions per row, zero digits included), canonical
      rows out with the plaintext folded in and pair rows out, beside pair_mul_dev of the same number of rows in the same run —
      the ceiling of anything made of pair products
  (c) 2^16 rows against the composition a build without the kernel runs: powmod_dev of the broadcast h_s by the same rho, then
      add_plain_dev; same bits asserted
  (d) the window sweep: (b) for every window of --windows at every key width of --sweep-keys, with the table bytes and the time
      to build the table
  (e) precompute_obfuscators(2^20) both ways

Beside the measured ratios of (a) and (c): what the operation counts predict with DESIGN.md's costs (a pair squaring 3.56 H^2, a
pair product 5 H^2): T = ceil(bits / w) products against key_bits squarings + key_bits / 5 + 30 products (the 2^5-ary ladder of
the full-width exponent) for (a), against bits squarings + bits / 5 + 30 products for (c).

Wall clock (time.perf_counter) around calls that end in a stream synchronisation; --repeats runs each, the sides of a comparison
alternating (one more round warms up and is dropped); min - max reported.

  python tools/bench_short_obfuscators.py [--key-bits 2048] [--log2-values 20] [--repeats 5]  > profiles/rNN_short_obfuscators.json"""
import argparse
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--key-bits", type=int, default=2048)
ap.add_argument("--log2-values", type=int, default=20)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--windows", default="4,5,6,7,8,9,10")
ap.add_argument("--sweep-keys", default="1024,2048,3072")
ap.add_argument("--only", choices=["sweep"], default=None, help="sweep: part (d) alone")
args = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "python-paillier_amd")):
    sys.path.insert(0, p)

SQUARING, PRODUCT = 3.56, 5.0                                        # multiply-adds in units of H^2


def ladder_cost(bits):
    return bits * SQUARING + (bits / 5.0 + 30) * PRODUCT


def main():
    import numpy as np
    from phe import _engine, paillier
    from phe._device import DeviceArray

    count = 1 << args.log2_values
    windows = [int(w) for w in args.windows.split(",")]

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

    def ratio(slow, fast):
        return {"min": round(min(slow) / max(fast), 2), "max": round(max(slow) / min(fast), 2)}

    def key(bits):
        g = json.load(open(os.path.join(ROOT, "tests", "golden", "paillier_%d.json" % bits)))
        return paillier.PaillierPublicKey(int(g["n"], 16))     # public keys only: the party that encrypts holds no private key

    def set_window(eng, w):
        """the table of the engine's base at window w (0: the library's choice); returns (info, seconds to build)"""
        hs, bits = eng.short_base()
        t0 = time.perf_counter()
        eng.ctx.fixed_base_set(hs, bits, w)
        eng.ctx.sync()
        dt = time.perf_counter() - t0
        eng._short_table = True
        return eng.ctx.fixed_base_info(), dt

    pub, pub_off = key(args.key_bits), key(args.key_bits)          # two keys, two contexts: short obfuscators on / off
    eng = pub._get_engine()
    ctx = eng.ctx
    res = {"key_bits": args.key_bits, "values": count, "repeats": args.repeats,
           "timing": "time.perf_counter around calls that end in one stream synchronisation; the sides of a comparison alternate; "
                     "min - max of the repeats",
           "costs_in_H2": {"pair_squaring": SQUARING, "pair_product": PRODUCT}}
    rs = np.random.Generator(np.random.PCG64(12))
    values = rs.integers(-(1 << 40), 1 << 40, count)
    hs = pub.enable_short_obfuscators()
    bits = pub.short_obfuscator_bits
    el = (bits + 31) // 32
    info = pub._get_engine().short_table_info()
    res["exp_bits"], res["shipped_window"] = bits, info
    T = info["positions"]

    if args.only == "sweep":
        sweep(res, pub, count, windows, key, set_window, repeat, summary)
        print(json.dumps(res))
        return

    # ---- (a) the public call ---------------------------------------------------------------------------------------------------------------
    def call(k):
        def run():
            k.discard_obfuscators()
            k.encrypt_batch(values, device=True)
        return run
    t = repeat({"short_off": call(pub_off), "short_on": call(pub)})
    rho = _engine.random_bits_limbs(bits, count, el)
    e_dev = DeviceArray.from_host(ctx, rho)
    m_host = np.zeros((count, eng.n_limbs), np.uint32)              # (the plaintext's value does not enter the time)
    m_host[:, :2] = np.abs(values).astype(np.uint64).view(np.uint32).reshape(count, 2)
    m_dev = DeviceArray.from_host(ctx, m_host)
    out_c, out_p = DeviceArray(ctx, count, eng.ct_limbs), DeviceArray(ctx, count, eng.pair_form())

    def kernel(out, pair, m):
        def run():
            ctx.fixed_base_pow_dev(e_dev.ptr, el, None, False, m.ptr if m is not None else None, out.ptr, pair, count)
            ctx.sync()
        return run
    ph = repeat({"draw_rho": lambda: _engine.random_bits_limbs(bits, count, el, out=rho),
                 "upload_rho": lambda: DeviceArray.from_host(ctx, rho),
                 "kernel": kernel(out_c, False, m_dev)})
    res["public_call"] = {"short_off": summary(t["short_off"]), "short_on": summary(t["short_on"]),
                          "speedup": ratio(t["short_off"], t["short_on"]),
                          "predicted_by_operation_counts": round(ladder_cost(args.key_bits) / (T * PRODUCT), 2),
                          "phases_of_the_short_route": {k: summary(v) for k, v in ph.items()},
                          "share_of_the_draw": round(min(ph["draw_rho"]) / min(t["short_on"]), 2),
                          "rows_per_s": {k: round(count / min(t[k])) for k in t}}

    # ---- (b) the kernel alone --------------------------------------------------------------------------------------------------------------
    a_pair = out_p
    b_pair = DeviceArray(ctx, count, eng.pair_form())
    ctx.fixed_base_pow_dev(e_dev.ptr, el, None, False, None, a_pair.ptr, True, count)
    ctx.d2d(b_pair.ptr, a_pair.ptr, a_pair.nbytes)
    ctx.sync()
    scratch = DeviceArray(ctx, count, eng.pair_form())

    def pair_mul():
        ctx.pair_mul_dev(a_pair.ptr, b_pair.ptr, False, scratch.ptr, count)
        ctx.sync()
    out2 = DeviceArray(ctx, count, eng.pair_form())
    t = repeat({"canonical_out_with_plaintext": kernel(out_c, False, m_dev), "pair_out": kernel(out2, True, None),
                "pair_mul_dev": pair_mul})
    res["kernel_alone"] = {k: dict(summary(v), rows_per_s=round(count / min(v))) for k, v in t.items()}
    res["kernel_alone"]["pair_products_per_row"] = T
    for k in ("canonical_out_with_plaintext", "pair_out"):
        res["kernel_alone"][k]["pair_products_per_s"] = round(count * T / min(t[k]))
    res["kernel_alone"]["pair_out_share_of_pair_mul_rate"] = round(count * T / min(t["pair_out"]) / (count / min(t["pair_mul_dev"])), 3)
    res["kernel_alone"]["exit_ms"] = round((min(t["canonical_out_with_plaintext"]) - min(t["pair_out"])) * 1e3, 3)

    # ---- (c) against the composition without the kernel --------------------------------------------------------------------------------------
    small = 1 << 16
    base = DeviceArray.from_host(ctx, np.tile(eng.cipher_limbs([hs]), (small, 1)))
    tmp, out_k, out_o = (DeviceArray(ctx, small, eng.ct_limbs) for _ in range(3))

    def composed():
        ctx.powmod_dev(base.ptr, e_dev.ptr, el, bits, tmp.ptr, small)
        ctx.add_plain_dev(tmp.ptr, m_dev.ptr, out_o.ptr, small)
        ctx.sync()

    def comb():
        ctx.fixed_base_pow_dev(e_dev.ptr, el, None, False, m_dev.ptr, out_k.ptr, False, small)
        ctx.sync()
    t = repeat({"composition": composed, "kernel": comb})
    res["against_the_composition"] = {"rows": small, "composition": summary(t["composition"]), "kernel": summary(t["kernel"]),
                                      "speedup": ratio(t["composition"], t["kernel"]),
                                      "predicted_by_operation_counts": round(ladder_cost(bits) / (T * PRODUCT), 2),
                                      "same_bits": bool(np.array_equal(out_k.to_host(), out_o.to_host()))}

    # ---- (e) the pool ----------------------------------------------------------------------------------------------------------------------
    def fill(k):
        def run():
            k.discard_obfuscators()
            k.precompute_obfuscators(count)
        return run
    t = repeat({"short_off": fill(pub_off), "short_on": fill(pub)})
    pub.discard_obfuscators()
    pub_off.discard_obfuscators()
    res["pool_fill"] = {"short_off": summary(t["short_off"]), "short_on": summary(t["short_on"]),
                        "speedup": ratio(t["short_off"], t["short_on"])}
    del base, tmp, out_k, out_o, a_pair, b_pair, scratch, out2, out_c, out_p

    sweep(res, pub, count, windows, key, set_window, repeat, summary)
    print(json.dumps(res))


def sweep(res, pub, count, windows, key, set_window, repeat, summary):
    """(d) the window sweep: the kernel alone (canonical rows out, a plaintext folded in) for every window at every key width"""
    import numpy as np
    from phe import _engine
    from phe._device import DeviceArray
    res["window_sweep"] = {}
    for kb in [int(b) for b in args.sweep_keys.split(",")]:
        pub_k = pub if kb == args.key_bits else key(kb)
        pub_k.enable_short_obfuscators(x=12345678901234567891)
        eng_k = pub_k._get_engine()
        kbits = pub_k.short_obfuscator_bits
        kel = (kbits + 31) // 32
        e_k = DeviceArray.from_host(eng_k.ctx, _engine.random_bits_limbs(kbits, count, kel))
        m_k = DeviceArray.from_host(eng_k.ctx, np.zeros((count, eng_k.n_limbs), np.uint32))
        o_k = DeviceArray(eng_k.ctx, count, eng_k.ct_limbs)
        rows = {}
        for w in windows:
            inf, build_s = set_window(eng_k, w)

            def run():
                eng_k.ctx.fixed_base_pow_dev(e_k.ptr, kel, None, False, m_k.ptr, o_k.ptr, False, count)
                eng_k.ctx.sync()
            tw = repeat({"kernel": run})["kernel"]
            rows[str(w)] = dict(summary(tw), positions=inf["positions"], table_bytes=inf["table_bytes"],
                                table_build_ms=round(build_s * 1e3, 1), rows_per_s=round(count / min(tw)))
        best = min(rows, key=lambda w: rows[w]["ms_min"])
        inf, _ = set_window(eng_k, 0)
        res["window_sweep"][str(kb)] = {"exp_bits": kbits, "windows": rows, "fastest_window": int(best),
                                        "shipped_window": inf["window"]}
        pub_k.disable_short_obfuscators()


if __name__ == "__main__":
    main()
