#!/usr/bin/env python3
"""Grouped homomorphic sums (EncryptedVector.segment_sum; csrc/segment_core.h) on resident rows, 2048-bit key by default:

  1. 2^20 rows, 256 segments, rows as canonical residues          2. the same rows in the pair form
  3. the pair rows with F = 8 groupings (the histogram form)      4. 2^16 rows against matvec(indicator_csr) on the same rows

Every shape is timed twice: "api" is the wall clock of the public call (planning on the host, upload of the index arrays,
kernels, exit from the pair form), "device" the wall clock of the queued kernels of an uploaded plan up to their one
synchronisation.  Runs of the contenders are interleaved, --repeats each; rows/s counts input rows (times F for shape 3).
A sweep of the task cap (phe/_engine.py SEGMENT_TASK_ROWS) over powers of two on shapes 1 and 2 picks the module constant, and
tools/bench_sweep.py --ops pair_add in the same run gives the box's rate of plain pair products to set the rates against.
The 2^16 results are compared bit for bit with matvec's and, on a sample of segments, with Python-integer products.

  python tools/bench_segment_sum.py [--key-bits 2048] [--log2-rows 20] [--segments 256] [--repeats 5]  > profiles/rNN_segment_sum.json"""
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
    ap.add_argument("--log2-matvec-rows", type=int, default=16)
    ap.add_argument("--segments", type=int, default=256)
    ap.add_argument("--features", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--caps", default="8,16,32,64,128,256")
    ap.add_argument("--no-pair-add", action="store_true", help="skip the tools/bench_sweep.py run")
    args = ap.parse_args()
    import numpy as np
    from phe import _engine, paillier
    from phe._device import DeviceArray
    from phe.ciphertext import EncryptedVector

    res = {"key_bits": args.key_bits, "rows": 1 << args.log2_rows, "segments": args.segments, "features": args.features,
           "repeats": args.repeats, "timing": "time.perf_counter around calls that end in one stream synchronisation; interleaved"}
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
    assert eng.has_segment_reduce(), "no grouped-sum kernel for this key width"
    n_rows, n_mv = 1 << args.log2_rows, 1 << args.log2_matvec_rows
    rs = np.random.Generator(np.random.PCG64(8))
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
    ids = rs.integers(0, args.segments, n_rows)
    ids_f = rs.integers(0, args.segments, (args.features, n_rows))

    def wall(fn):
        t0 = time.perf_counter()
        out = fn()
        return time.perf_counter() - t0, out

    def summary(times, rows):
        return {"rows_per_s_best": rows / min(times), "rows_per_s_worst": rows / max(times),
                "rows_per_s_median": rows / sorted(times)[len(times) // 2], "ms": [round(t * 1e3, 3) for t in times]}

    # ---- the sweep of the task cap (device time) ---------------------------------------------------------------------------
    caps = [int(c) for c in args.caps.split(",")]
    plans = {}
    for cap in caps:
        plan = _engine.plan_segments(ids, args.segments, cap)
        plans[cap] = (plan, eng.segment_upload(plan))
    sweep = {cap: {"residues": [], "pair": []} for cap in caps}
    for rep in range(args.repeats + 1):                                   # (the first round warms up and is dropped)
        for cap in caps:
            plan, dev = plans[cap]
            for name, rows, is_pair in (("residues", store, False), ("pair", pair._store, True)):
                t, _ = wall(lambda: eng.segment_launch_dev(rows, is_pair, plan, dev, want_pair=True))
                if rep:
                    sweep[cap][name].append(t)
    res["cap_sweep"] = {str(cap): {"levels": len(plans[cap][0].levels), "tasks_level0": len(plans[cap][0].levels[0][2]),
                                   "residues": summary(sweep[cap]["residues"], n_rows), "pair": summary(sweep[cap]["pair"], n_rows)}
                        for cap in caps}
    best = max(caps, key=lambda c: min(res["cap_sweep"][str(c)][k]["rows_per_s_median"] for k in ("residues", "pair")))
    res["cap_best_of_sweep"] = best
    res["cap_module_constant"] = _engine.SEGMENT_TASK_ROWS
    plans.clear()

    # ---- shapes 1 - 3 with the module constant: the public call and the kernels alone, interleaved -------------------------------
    plan1 = _engine.plan_segments(ids, args.segments)
    plan3 = _engine.plan_segments(ids_f, args.segments)
    dev1, dev3 = eng.segment_upload(plan1), eng.segment_upload(plan3)
    shapes = {
        "residues": (lambda: vec.segment_sum(ids, args.segments), lambda: eng.segment_launch_dev(store, False, plan1, dev1), n_rows),
        "pair": (lambda: pair.segment_sum(ids, args.segments), lambda: eng.segment_launch_dev(pair._store, True, plan1, dev1, True),
                 n_rows),
        "pair_features": (lambda: pair.segment_sum(ids_f, args.segments),
                          lambda: eng.segment_launch_dev(pair._store, True, plan3, dev3, True), n_rows * args.features),
    }
    times = {k: {"api": [], "device": []} for k in shapes}
    for rep in range(args.repeats + 1):
        for k, (api, device, _) in shapes.items():
            ta, _ = wall(api)
            td, _ = wall(device)
            if rep:
                times[k]["api"].append(ta)
                times[k]["device"].append(td)
    res["shapes"] = {k: {"input_rows": shapes[k][2], "api": summary(times[k]["api"], shapes[k][2]),
                         "device": summary(times[k]["device"], shapes[k][2])} for k in shapes}
    if "pair_add" in res:
        for k in shapes:
            res["shapes"][k]["device_median_as_fraction_of_pair_add"] = res["shapes"][k]["device"]["rows_per_s_median"] / res["pair_add"]["per_s"]

    # ---- shape 4: against matvec with the 0/1 matrix of the same grouping -------------------------------------------------------
    try:
        import scipy.sparse as sp
    except ImportError:
        sp = None
    sub = EncryptedVector(pub, store.rows_view(0, n_mv), zeros[:n_mv])
    ids_mv = ids[:n_mv]
    mv = {"rows": n_mv}
    if sp is None:
        mv["not_measured"] = "scipy is not installed: no indicator matrix to hand to matvec"
    else:
        M = sp.csr_matrix((np.ones(n_mv, dtype=np.int64), (ids_mv, np.arange(n_mv))), shape=(args.segments, n_mv))
        t_seg, t_mat, a = [], [], None
        for rep in range(args.repeats + 1):
            ts, a = wall(lambda: sub.segment_sum(ids_mv, args.segments))
            tm, b = wall(lambda: sub.matvec(M))
            if rep:
                t_seg.append(ts)
                t_mat.append(tm)
        ca, cb = a.ciphertexts(False), b.ciphertexts(False)
        n2 = pub.nsquare
        vals = [int.from_bytes(first_block[i].tobytes(), "little") for i in range(min(n_mv, len(first_block)))]
        sample_ok = True
        for s in range(min(4, args.segments)):
            v = 1
            for i in np.nonzero(ids_mv[:len(vals)] == s)[0]:
                v = v * vals[int(i)] % n2
            if n_mv <= len(vals):
                sample_ok = sample_ok and ca[s] == v
        mv.update({"segment_sum": summary(t_seg, n_mv), "matvec": summary(t_mat, n_mv), "same_bits_as_matvec": ca == cb,
                   "sample_equals_integer_product": bool(sample_ok),
                   "slowest_segment_sum_over_fastest_matvec": max(t_seg) / min(t_mat),
                   "speedup_median": sorted(t_mat)[len(t_mat) // 2] / sorted(t_seg)[len(t_seg) // 2],
                   "slowest_segment_sum_beats_fastest_matvec": max(t_seg) < min(t_mat)})
    res["against_matvec"] = mv
    print(json.dumps(res))


if __name__ == "__main__":
    main()
