#!/usr/bin/env python3
"""Encryption-side packing and the slot codec kernels (PaillierPublicKey.encrypt_packed / PaillierPrivateKey.decrypt_packed;
csrc/slot_codec.h), 2048-bit key and 2^20 int64 values by default, (slots, slot_bits) = the widest S at 64 bits:

  (a) encrypt_packed against encrypt_batch of the same values, whole public calls, both device=True, interleaved; the packing
      step alone (upload of the values + kernel) and the upload alone; and, for the record, the widest S at 128 bits, which is
      packed on the host
  (b) decrypt_packed of the packed rows as a list and with as_array=True, and with the lists unpacked on the host
      (keys.PACKED_LISTS_THROUGH_CODEC = False: the route a build without the kernels takes); --only key_holder prints this
      part alone and runs on any revision that has decrypt_packed (tools/exp/gpu_ab_decrypt_packed.sh alternates two trees)
  (c) the two kernels alone on resident operands, --inner launches per timing and one synchronisation, against a
      device-to-device copy of the same number of bytes in the same run: the ceiling of a kernel that only moves bits.  Bytes:
      8 per value + 4 n_limbs per row (+ 1 status byte per row for unpack), each counted once

Wall clock (time.perf_counter) around calls that end in a stream synchronisation; --repeats runs each, interleaved (one more
round warms up and is dropped).

  python tools/bench_slots.py [--key-bits 2048] [--log2-values 20] [--repeats 5] [--only key_holder]  > profiles/rNN_slots.json"""
import argparse
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--key-bits", type=int, default=2048)
ap.add_argument("--log2-values", type=int, default=20)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--inner", type=int, default=50)
ap.add_argument("--only", choices=["key_holder"], default=None)
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                help="the checkout whose package is measured (default: this one)")
args = ap.parse_args()
ROOT = os.path.abspath(args.tree)
for p in (ROOT, os.path.join(ROOT, "python-paillier_amd")):
    sys.path.insert(0, p)


def main():
    import numpy as np
    from phe import keys, paillier

    count = 1 << args.log2_values
    g = json.load(open(os.path.join(ROOT, "tests", "golden", "paillier_%d.json" % args.key_bits)))
    pub = paillier.PaillierPublicKey(int(g["n"], 16))
    priv = paillier.PaillierPrivateKey(pub, int(g["p"], 16), int(g["q"], 16))
    eng = priv._get_engine()
    bound = pub.max_int.bit_length() - 1
    S, B = bound // 64, 64
    rows = -(-count // S)
    res = {"key_bits": args.key_bits, "values": count, "slots": S, "slot_bits": B, "packed_rows": rows, "repeats": args.repeats,
           "tree": os.path.basename(ROOT),
           "timing": "time.perf_counter around calls that end in one stream synchronisation; interleaved where compared"}
    rs = np.random.Generator(np.random.PCG64(11))
    values = rs.integers(-(1 << 40), 1 << 40, count)                     # quantised gradients / histogram sums: inside a 64-bit slot

    def summary(times):
        return {"ms_best": round(min(times) * 1e3, 3), "ms_worst": round(max(times) * 1e3, 3),
                "ms_median": round(sorted(times)[len(times) // 2] * 1e3, 3), "slowest_over_fastest": round(max(times) / min(times), 3),
                "ms": [round(t * 1e3, 3) for t in times]}

    def repeat(fns, repeats=args.repeats):
        times = {k: [] for k in fns}
        for rep in range(repeats + 1):                                    # (the first round warms up and is dropped)
            for k, fn in fns.items():
                t0 = time.perf_counter()
                fn()
                if rep:
                    times[k].append(time.perf_counter() - t0)
        return times

    med = lambda ts: sorted(ts)[len(ts) // 2]
    has_codec = hasattr(eng, "has_slot_codec") and eng.has_slot_codec()
    res["slot_codec"] = bool(has_codec)

    # ---- (b) the key holder ---------------------------------------------------------------------------------------------------------------
    if hasattr(pub, "encrypt_packed"):
        packed = pub.encrypt_packed(values, S, B, device=True)
    else:
        packed = pub.encrypt_batch(values, device=True).pack(S, B)       # (a revision without encrypt_packed: the same plaintext rows)
    packed._limbs
    fns = {"list": lambda: priv.decrypt_packed(packed, S, B, count=count)}
    if has_codec:
        fns["as_array"] = lambda: priv.decrypt_packed(packed, S, B, count=count, as_array=True)

        def host_lists():
            keep, keys.PACKED_LISTS_THROUGH_CODEC = keys.PACKED_LISTS_THROUGH_CODEC, False
            try:
                return priv.decrypt_packed(packed, S, B, count=count)
            finally:
                keys.PACKED_LISTS_THROUGH_CODEC = keep
        fns["list_unpacked_on_the_host"] = host_lists
    t = repeat(fns)
    res["key_holder"] = {k: summary(v) for k, v in t.items()}
    res["key_holder"]["values_come_back"] = bool(priv.decrypt_packed(packed, S, B, count=count) == values.tolist())
    if has_codec:
        res["key_holder"]["lists_through_codec_by_default"] = bool(keys.PACKED_LISTS_THROUGH_CODEC)
    if args.only == "key_holder":
        print(json.dumps(res))
        return

    # ---- (a) encrypt_packed against encrypt_batch ------------------------------------------------------------------------------------------
    from phe._device import DeviceArray
    pub.discard_obfuscators()
    t = repeat({"encrypt_batch": lambda: pub.encrypt_batch(values, device=True),
                "encrypt_packed": lambda: pub.encrypt_packed(values, S, B, device=True),
                "packing_step": lambda: eng.slots_pack_dev(values, S, B),
                "upload_of_the_values": lambda: DeviceArray.from_host(eng.ctx, values.view(np.uint32))}, repeats=min(args.repeats, 3))
    res["encrypt"] = {k: summary(v) for k, v in t.items()}
    res["encrypt"]["speedup_median"] = round(med(t["encrypt_batch"]) / med(t["encrypt_packed"]), 2)
    res["encrypt"]["exponentiations"] = {"encrypt_batch": count, "encrypt_packed": rows, "ratio": round(count / rows, 2)}
    res["encrypt"]["values_per_s_median"] = {k: round(count / med(t[k])) for k in ("encrypt_batch", "encrypt_packed")}
    S2, B2 = bound // 128, 128
    wide_values = values.tolist()
    t2 = repeat({"encrypt_packed": lambda: pub.encrypt_packed(wide_values, S2, B2, device=True),
                 "host_packing_alone": lambda: pub._pack_plain_host(wide_values, S2, B2)}, repeats=2)
    res["encrypt_%dx%d_host_route" % (S2, B2)] = {k: summary(v) for k, v in t2.items()}
    res["encrypt_%dx%d_host_route" % (S2, B2)]["packed_rows"] = -(-count // S2)

    # ---- (c) the kernels alone ------------------------------------------------------------------------------------------------------------------
    ctx = eng.ctx
    v_dev = DeviceArray.from_host(ctx, values.view(np.uint32))
    m_dev = DeviceArray(ctx, rows, eng.n_limbs)
    out_v, out_s = DeviceArray(ctx, rows * S, 2), DeviceArray(ctx, (rows + 3) // 4, 1)
    pack_bytes = 8 * count + 4 * eng.n_limbs * rows
    unpack_bytes = 8 * rows * S + 4 * eng.n_limbs * rows + rows
    src, dst = DeviceArray(ctx, (pack_bytes + 3) // 4, 1), DeviceArray(ctx, (pack_bytes + 3) // 4, 1)

    def many(fn):
        def run():
            for _ in range(args.inner):
                fn()
            ctx.sync()
        return run
    t = repeat({"pack": many(lambda: ctx.slots_pack_dev(v_dev.ptr, count, S, B, m_dev.ptr, rows)),
                "unpack": many(lambda: ctx.slots_unpack_dev(m_dev.ptr, rows, S, B, out_v.ptr, out_s.ptr)),
                # a copy moves every byte twice (read + write): half of pack_bytes copied = pack_bytes moved
                "d2d_copy_same_bytes": many(lambda: ctx.d2d(dst.ptr, src.ptr, pack_bytes // 2))})
    per = lambda ts: [x / args.inner for x in ts]
    res["kernels"] = {"launches_per_timing": args.inner,
                      "pack": dict(summary(per(t["pack"])), bytes=pack_bytes, gb_per_s_median=round(pack_bytes / med(per(t["pack"])) / 1e9, 1)),
                      "unpack": dict(summary(per(t["unpack"])), bytes=unpack_bytes,
                                     gb_per_s_median=round(unpack_bytes / med(per(t["unpack"])) / 1e9, 1)),
                      "d2d_copy_same_bytes": dict(summary(per(t["d2d_copy_same_bytes"])), bytes_moved=pack_bytes,
                                                  gb_per_s_median=round(pack_bytes / med(per(t["d2d_copy_same_bytes"])) / 1e9, 1))}
    values_back, status = eng.slots_unpack_dev(m_dev, S, B)
    res["kernels"]["round_trip_ok"] = bool(np.array_equal(values_back[:count], values) and not status.any())
    print(json.dumps(res))


if __name__ == "__main__":
    main()
