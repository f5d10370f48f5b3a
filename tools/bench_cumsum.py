#!/usr/bin/env python3
"""Running homomorphic sums (EncryptedVector.cumsum; csrc/segment_core.h segment_scan_body) on resident rows, 2048-bit key by
default:

  1. 2^20 rows, one sequence, pair form in and out              2. the same rows as canonical residues (entry + exit conversion)
  3. the pair rows as 4096 blocks of 256 (the histogram form)   4. the task cap swept over powers of two on shapes 1 and 3
  5. log-step doubling with pair products on slices of the same pair rows: what a user has without the kernel

Shapes 1 - 3 are timed twice: "api" is the wall clock of the public call (planning on the host, upload of the index arrays,
kernels, exit from the pair form where the input is not in it), "device" the wall clock of the queued kernels of an uploaded
plan up to their one synchronisation.  Runs of the contenders are interleaved, --repeats each (one more round warms up and is
dropped); rows/s counts input rows.  tools/bench_sweep.py --ops pair_add in the same run gives the box's rate of plain pair
products: a plan executes (1 + 1/cap + ...) products per row for the totals and one per row for the scan, so half of that rate
is the ceiling.  The results of 1, 2 and 5 are compared bit for bit after the exit from the pair form, and the first rows with
Python-integer running products.

  python tools/bench_cumsum.py [--key-bits 2048] [--log2-rows 20] [--block 256] [--repeats 5]  > profiles/rNN_cumsum.json"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "python-paillier_amd")):
    sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--key-bits", type=int, default=2048)
    ap.add_argument("--log2-rows", type=int, default=20)
    ap.add_argument("--block", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--caps", default="8,16,32,64,128,256")
    ap.add_argument("--no-pair-add", action="store_true", help="skip the tools/bench_sweep.py run")
    args = ap.parse_args()
    import numpy as np
    from phe import _engine, paillier
    from phe._device import DeviceArray
    from phe.ciphertext import EncryptedVector

    n_rows = 1 << args.log2_rows
    res = {"key_bits": args.key_bits, "rows": n_rows, "block": args.block, "repeats": args.repeats,
           "timing": "time.perf_counter around calls that end in one stream synchronisation; interleaved"}
    if not args.no_pair_add:
        # the box's rate of plain pair products, from the same run (its own process: it sizes its buffers itself)
        out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "bench_sweep.py"), "--key-bits", str(args.key_bits),
                              "--ops", "pair_add", "--min", str(args.log2_rows), "--max", str(args.log2_rows)],
                             stdout=subprocess.PIPE, check=True, timeout=600)
        sweep_res = json.loads(out.stdout.decode().strip().splitlines()[-1])
        res["device"] = sweep_res["device"]
        point = sweep_res["points"][-1]["pair_add"]
        res["pair_add"] = {"per_s": point["per_s"], "ms": point["ms"], "geom": point["geom"], "bit_exact": point["bit_exact"]}
    g = json.load(open(os.path.join(ROOT, "tests", "golden", "paillier_%d.json" % args.key_bits)))
    pub = paillier.PaillierPublicKey(int(g["n"], 16))
    eng = pub._get_engine()
    assert eng.has_segment_scan(), "no running-sum kernel for this key width"
    rs = np.random.Generator(np.random.PCG64(9))
    # any residues serve a product: random words with the top one cleared (below n^2), made in blocks of 2^16 rows
    store = DeviceArray(eng.ctx, n_rows, eng.ct_limbs)
    for lo in range(0, n_rows, 1 << 16):
        block = rs.integers(0, 1 << 32, size=(min(1 << 16, n_rows - lo), eng.ct_limbs), dtype=np.uint64).astype(np.uint32)
        block[:, -1] = 0
        eng.ctx.h2d(store.ptr + lo * eng.ct_limbs * 4, block)
        if lo == 0:
            first_block = block
    zeros = np.zeros(n_rows, dtype=np.int64)
    vec = EncryptedVector(pub, store, zeros)
    pair = vec.to_pair()
    words = eng.pair_form()

    def wall(fn):
        t0 = time.perf_counter()
        out = fn()
        return time.perf_counter() - t0, out

    def summary(times, rows=n_rows):
        return {"rows_per_s_best": rows / min(times), "rows_per_s_worst": rows / max(times),
                "rows_per_s_median": rows / sorted(times)[len(times) // 2], "slowest_over_fastest": max(times) / min(times),
                "ms": [round(t * 1e3, 3) for t in times]}

    def products_per_row(plan):
        """pair products the plan executes per input row: every level but the last is reduced, every level is scanned"""
        reduced = sum(lv[2] for lv in plan.levels[:-1])
        scanned = sum(lv[2] for lv in plan.levels)
        return (reduced + scanned) / plan.n_rows

    # ---- the sweep of the task cap (device time), shapes 1 and 3 -----------------------------------------------------------------
    caps = [int(c) for c in args.caps.split(",")]
    plans = {}
    for cap in caps:
        for name, blk in (("one_sequence", None), ("blocks", args.block)):
            plan = _engine.plan_scan(n_rows, blk, cap)
            plans[cap, name] = (plan, eng.scan_upload(plan))
    sweep = {key: [] for key in plans}
    for rep in range(args.repeats + 1):                                   # (the first round warms up and is dropped)
        for key, (plan, dev) in plans.items():
            t, _ = wall(lambda: eng.scan_launch_dev(pair._store, True, plan, dev, want_pair=True))
            if rep:
                sweep[key].append(t)
    res["cap_sweep"] = {str(cap): {name: dict(summary(sweep[cap, name]), levels=len(plans[cap, name][0].levels),
                                              tasks_level0=len(plans[cap, name][0].levels[0][0]) - 1,
                                              products_per_row=products_per_row(plans[cap, name][0]))
                                   for name in ("one_sequence", "blocks")} for cap in caps}
    res["cap_best_of_sweep"] = max(caps, key=lambda c: min(res["cap_sweep"][str(c)][k]["rows_per_s_median"]
                                                           for k in ("one_sequence", "blocks")))
    res["cap_module_constant"] = _engine.SCAN_TASK_ROWS
    plans.clear()

    # ---- the contender: log-step doubling, one launch of pair products per level, every level through HBM ---------------------------
    def doubling(cur):
        d = 1
        while d < n_rows:
            nxt = DeviceArray(eng.ctx, n_rows, words)
            eng.ctx.d2d(nxt.ptr, cur.ptr, d * words * 4)                  # rows 0 .. d are final
            eng.ctx.pair_mul_dev(cur.ptr + d * words * 4, cur.ptr, False, nxt.ptr + d * words * 4, n_rows - d)
            eng.ctx.sync()
            cur, d = nxt, 2 * d
        return cur

    # ---- shapes 1 - 3 with the module constant and the contender, interleaved ------------------------------------------------------------
    plan1 = _engine.plan_scan(n_rows)
    plan3 = _engine.plan_scan(n_rows, args.block)
    dev1, dev3 = eng.scan_upload(plan1), eng.scan_upload(plan3)
    shapes = {
        "pair": (lambda: pair.cumsum(), lambda: eng.scan_launch_dev(pair._store, True, plan1, dev1, True)),
        "residues": (lambda: vec.cumsum(), lambda: eng.scan_launch_dev(store, False, plan1, dev1)),
        "pair_blocks": (lambda: pair.cumsum(block=args.block), lambda: eng.scan_launch_dev(pair._store, True, plan3, dev3, True)),
    }
    times = {k: {"api": [], "device": []} for k in shapes}
    t_doubling = []
    for rep in range(args.repeats + 1):
        for k, (api, device) in shapes.items():
            ta, _ = wall(api)
            td, _ = wall(device)
            if rep:
                times[k]["api"].append(ta)
                times[k]["device"].append(td)
        tl, _ = wall(lambda: doubling(pair._store))
        if rep:
            t_doubling.append(tl)
    res["shapes"] = {k: {"api": summary(times[k]["api"]), "device": summary(times[k]["device"])} for k in shapes}
    res["shapes"]["pair"]["products_per_row"] = res["shapes"]["residues"]["products_per_row"] = products_per_row(plan1)
    res["shapes"]["pair_blocks"]["products_per_row"] = products_per_row(plan3)
    if "pair_add" in res:
        for k in shapes:
            res["shapes"][k]["device_median_as_fraction_of_pair_add"] = res["shapes"][k]["device"]["rows_per_s_median"] / res["pair_add"]["per_s"]
    levels = (n_rows - 1).bit_length()
    res["doubling"] = dict(summary(t_doubling), launches=levels, products_per_row=(levels * n_rows - (n_rows - 1)) / n_rows)
    med = lambda ts: sorted(ts)[len(ts) // 2]
    res["doubling"]["kernel_speedup_median"] = med(t_doubling) / med(times["pair"]["device"])
    res["doubling"]["slowest_kernel_beats_fastest_doubling"] = max(times["pair"]["device"]) < min(t_doubling)
    res["doubling"]["speedup_predicted_by_product_counts"] = res["doubling"]["products_per_row"] / res["shapes"]["pair"]["products_per_row"]

    # ---- the same bits: kernel on pair rows, kernel on residues, doubling; the first rows against Python integers ------------------
    a = eng.from_pair_dev(eng.scan_launch_dev(pair._store, True, plan1, dev1, True)).to_host()
    same_res = bool(np.array_equal(a, eng.scan_launch_dev(store, False, plan1, dev1).to_host()))
    same_dbl = bool(np.array_equal(a, eng.from_pair_dev(doubling(pair._store)).to_host()))
    n2, v, sample_ok = pub.nsquare, 1, True
    for i in range(min(64, n_rows)):
        v = v * int.from_bytes(first_block[i].tobytes(), "little") % n2
        sample_ok = sample_ok and int.from_bytes(a[i].tobytes(), "little") == v
    if 2 * args.block <= min(n_rows, len(first_block)):                  # the second block starts from its own first row
        blocks = pair.cumsum(block=args.block)._plain_rows().rows_view(args.block, args.block + 3).to_host()
        v = 1
        for i in range(3):
            v = v * int.from_bytes(first_block[args.block + i].tobytes(), "little") % n2
            sample_ok = sample_ok and int.from_bytes(blocks[i].tobytes(), "little") == v
    res["same_bits"] = {"residues_as_pair": same_res, "doubling_as_kernel": same_dbl, "sample_equals_integer_products": bool(sample_ok)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
