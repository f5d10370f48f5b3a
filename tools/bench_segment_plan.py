#!/usr/bin/env python3
"""The planner of the grouped sums on the device (csrc/segment_plan.h; Engine.plan_segments_dev) against the numpy planner it
mirrors (phe/_engine.py plan_segments + Engine.segment_upload), 2048-bit key by default, one run, routes interleaved:

  1. planning alone     2^20 rows x 256 segments, F = 1, 8, 32 groupings; F = 8 once more with a node array of K = 8 nodes.
                        "host": plan_segments on host ids and the upload of its index arrays; "device": plan_segments_dev on
                        resident ids (and a resident node array).
  2. the public call    EncryptedVector.segment_sum on pair rows at the shapes of profiles/r08_segment_sum.json (F = 1 and 8), the
                        numpy planner ("host": SEGMENT_PLAN_DEVICE_MIN above the shape), the device planner with host ids
                        ("device": the ids go up as int32) and with PaillierPublicKey.segment_ids ("resident"); beside each the
                        kernels alone of the same run ("kernels": an uploaded plan queued and waited for once).
  3. the threshold      planning alone at F * rows = 2^10 ... 2^24 in powers of four (one grouping, 256 segments): the smallest
                        size from which on the device route's slowest repeat stays at or below the host route's fastest is the
                        crossover that phe/_engine.py SEGMENT_PLAN_DEVICE_MIN quotes.

Every time is time.perf_counter around a call that ends in a stream synchronisation (plan_segments_dev ends in one; the host route
is followed by one); the first round of every loop warms up and is dropped.  Per comparison the project's usual condition is
stated: "slowest device repeat <= fastest host repeat".  The device plan of every measured shape is compared with the host plan
element for element before it is timed.

  python tools/bench_segment_plan.py [--key-bits 2048] [--log2-rows 20] [--segments 256] [--repeats 5]  > profiles/rNN_segment_plan.json"""
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
    ap.add_argument("--segments", type=int, default=256)
    ap.add_argument("--groupings", default="1,8,32")
    ap.add_argument("--nodes", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sweep-min", type=int, default=10)
    ap.add_argument("--sweep-max", type=int, default=24)
    ap.add_argument("--no-public-call", action="store_true", help="planning and the threshold only (no ciphertext rows are made)")
    args = ap.parse_args()
    import numpy as np
    from phe import _engine, paillier
    from phe._device import DeviceArray
    from phe.ciphertext import EncryptedVector

    g = json.load(open(os.path.join(ROOT, "tests", "golden", "paillier_%d.json" % args.key_bits)))
    pub = paillier.PaillierPublicKey(int(g["n"], 16))
    eng = pub._get_engine()
    assert eng.has_segment_reduce() and eng.has_segment_planner(), "no grouped-sum kernel or no device planner"
    n_rows, S, K = 1 << args.log2_rows, args.segments, args.nodes
    rs = np.random.Generator(np.random.PCG64(14))
    res = {"key_bits": args.key_bits, "rows": n_rows, "segments": S, "nodes": K, "repeats": args.repeats,
           "task_cap": _engine.SEGMENT_TASK_ROWS,
           "timing": "time.perf_counter around calls that end in one stream synchronisation; routes interleaved; first round dropped",
           "condition": "slowest device repeat <= fastest host repeat"}

    def wall(fn):
        t0 = time.perf_counter()
        out = fn()
        return time.perf_counter() - t0, out

    def ms(times):
        return {"min_ms": round(min(times) * 1e3, 3), "max_ms": round(max(times) * 1e3, 3),
                "median_ms": round(sorted(times)[len(times) // 2] * 1e3, 3), "ms": [round(t * 1e3, 3) for t in times]}

    def compare(host, device):
        return {"host": ms(host), "device": ms(device), "speedup_median": sorted(host)[len(host) // 2] / sorted(device)[len(device) // 2],
                "slowest_device_over_fastest_host": max(device) / min(host), "condition_met": max(device) <= min(host)}

    def same_plan(dev_plan, host_plan):
        got = dev_plan.to_host()
        if len(got.levels) != len(host_plan.levels):
            return False
        for (tp, idx, order), (tp_w, idx_w, order_w) in zip(got.levels, host_plan.levels):
            if not (np.array_equal(tp, tp_w) and np.array_equal(order, order_w)):
                return False
            if (idx is None) != (idx_w is None) or (idx is not None and not np.array_equal(idx, idx_w)):
                return False
        return True

    def composed(ids, node):
        return (np.where((node >= 0) & (ids >= 0), node * S + ids, -1), K * S) if node is not None else (ids, S)

    def host_route(ids, node):
        cid, cS = composed(ids, node)
        plan = _engine.plan_segments(cid, cS)
        dev = eng.segment_upload(plan)
        eng.ctx.sync()
        return plan, dev

    def planning(ids, node):
        """host: numpy plan + upload; device: plan_segments_dev on resident ids.  Interleaved."""
        ids_dev = eng.upload_ids(ids)
        node_dev = eng.upload_ids(node) if node is not None else None
        k = K if node is not None else 1
        host_plan, _ = host_route(ids, node)
        ok = same_plan(eng.plan_segments_dev(ids_dev, S, node_dev, k), host_plan)
        th, td = [], []
        for rep in range(args.repeats + 1):
            a, _ = wall(lambda: host_route(ids, node))
            b, _ = wall(lambda: eng.plan_segments_dev(ids_dev, S, node_dev, k))
            if rep:
                th.append(a)
                td.append(b)
        out = compare(th, td)
        out.update({"pairs": int(ids.size), "levels": len(host_plan.levels), "same_arrays_as_host_plan": bool(ok)})
        return out

    # ---- 1. planning alone -------------------------------------------------------------------------------------------------------
    res["planning"] = {}
    for F in [int(v) for v in args.groupings.split(",")]:
        res["planning"]["F%d" % F] = planning(rs.integers(0, S, (F, n_rows)), None)
    res["planning"]["F8_nodes%d" % K] = planning(rs.integers(0, S, (8, n_rows)), rs.integers(-1, K, n_rows))

    # ---- 3. the threshold --------------------------------------------------------------------------------------------------------
    sweep = {}
    for lg in range(args.sweep_min, args.sweep_max + 1, 2):
        sweep[str(1 << lg)] = planning(rs.integers(0, S, (1, 1 << lg)), None)
    res["threshold_sweep"] = sweep
    sizes = sorted(int(k) for k in sweep)
    crossover = None
    for size in reversed(sizes):                                         # the smallest size from which on the condition holds
        if sweep[str(size)]["condition_met"]:
            crossover = size
        else:
            break
    res["crossover_pairs"] = crossover
    res["module_constant"] = _engine.SEGMENT_PLAN_DEVICE_MIN

    # ---- 2. the public call on pair rows -----------------------------------------------------------------------------------------
    if not args.no_public_call:
        store = DeviceArray(eng.ctx, n_rows, eng.ct_limbs)
        for lo in range(0, n_rows, 1 << 16):                              # any residues serve a product (tools/bench_segment_sum.py)
            block = rs.integers(0, 1 << 32, size=(min(1 << 16, n_rows - lo), eng.ct_limbs), dtype=np.uint64).astype(np.uint32)
            block[:, -1] = 0
            eng.ctx.h2d(store.ptr + lo * eng.ct_limbs * 4, block)
        pair = EncryptedVector(pub, store, np.zeros(n_rows, dtype=np.int64)).to_pair()
        res["public_call"] = {}
        constant = _engine.SEGMENT_PLAN_DEVICE_MIN
        for F in (1, 8):
            ids = rs.integers(0, S, n_rows) if F == 1 else rs.integers(0, S, (F, n_rows))
            held = pub.segment_ids(ids, S)
            plan, dev = host_route(ids, None)

            def call(threshold, what):
                _engine.SEGMENT_PLAN_DEVICE_MIN = threshold
                try:
                    return pair.segment_sum(what, S)
                finally:
                    _engine.SEGMENT_PLAN_DEVICE_MIN = constant
            routes = {"host": lambda: call(1 << 62, ids), "device": lambda: call(0, ids), "resident": lambda: call(0, held),
                      "kernels": lambda: eng.segment_launch_dev(pair._store, True, plan, dev, True)}
            base = call(1 << 62, ids).ciphertexts(False)[:64]
            same = all(fn().ciphertexts(False)[:64] == base for fn in (routes["device"], routes["resident"]))
            times = {k: [] for k in routes}
            for rep in range(args.repeats + 1):
                for k, fn in routes.items():
                    t, _ = wall(fn)
                    if rep:
                        times[k].append(t)
            entry = {k: ms(v) for k, v in times.items()}
            entry["device_vs_host"] = compare(times["host"], times["device"])
            entry["resident_vs_host"] = compare(times["host"], times["resident"])
            entry["same_first_64_ciphertexts"] = bool(same)
            res["public_call"]["F%d" % F] = entry
    print(json.dumps(res))


if __name__ == "__main__":
    main()
