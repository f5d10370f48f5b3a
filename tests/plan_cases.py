"""TEST INFRASTRUCTURE: the shapes the device planner of the grouped sums (csrc/segment_plan.h) is compared with the numpy planner
on — shared by tests/test_segment_plan.py (wave emulator) and tests/test_gpu_segment_plan.py (GPU).  Every comparison is exact:
each level's task_ptr, idx and order must be element for element what phe._engine.plan_segments returns."""
import numpy as np

TILE = 2048          # csrc/segment_plan.h kTile: the pairs of one workgroup in one pass


def composed(ids, n_segments, node, n_nodes):
    """the DEFINITION of node=: the ids of one call over n_nodes * n_segments segments"""
    ids = np.asarray(ids, dtype=np.int64)
    if node is None:
        return ids, n_segments
    node = np.asarray(node, dtype=np.int64)
    return np.where((node >= 0) & (ids >= 0), node * n_segments + ids, -1), n_nodes * n_segments


def _shuffled_sizes(sizes, extra, seed):
    ids = np.concatenate([np.repeat(np.arange(len(sizes)), sizes), np.full(extra, -1)]).astype(np.int64)
    np.random.RandomState(seed).shuffle(ids)
    return ids


def cases():
    """[(name, ids (rows,) or (F, rows), n_segments, node or None, n_nodes, cap)]"""
    out = []
    rs = np.random.RandomState(14)
    # row counts: around a wavefront, around one workgroup tile, and past three tiles (block offsets from the cross-block scan)
    for rows in (0, 1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 3 * TILE + 1):
        out.append(("rows_%d" % rows, rs.randint(-1, 5, rows), 5, None, 1, 16))
    out.append(("stable_one_segment", np.zeros(300, np.int64), 1, None, 1, 16))
    out.append(("stable_past_a_tile", np.zeros(TILE + 70, np.int64), 1, None, 1, 16))
    out.append(("all_dropped", np.full(100, -1), 3, None, 1, 16))
    out.append(("distinct_reversed", np.arange(500)[::-1].copy(), 500, None, 1, 16))
    # one, two and three digit passes; keys that differ in their top digit only
    for S in (1, 255, 256, 257, 65535, 65536, 65537):
        ids = rs.randint(-1, S, 700)
        twins = [k for k in (5, 5 + 256, 5 + 65536, 5 + 2 * 256, S - 1, 0) if k < S]
        ids[:3 * len(twins)] = np.tile(twins, 3)
        rs.shuffle(ids)
        out.append(("segments_%d" % S, ids, S, None, 1, 16))
    for F in (1, 2, 3):
        out.append(("groupings_%d" % F, rs.randint(-1, 7, size=(F, 200)), 7, None, 1, 16))
    out.append(("groupings_3_past_a_tile", rs.randint(-1, 300, size=(3, 900)), 300, None, 1, 16))
    out.append(("empty_segments", rs.choice([2, 3, 6, 7], 150), 10, None, 1, 16))
    # segment sizes around the cap; caps 2 and 4 force three or more levels
    for cap in (2, 4, 16):
        sizes = [cap - 1, cap, cap + 1, 2 * cap, cap * cap + 1, 0, 1]
        out.append(("sizes_cap_%d" % cap, _shuffled_sizes(sizes, 9, cap), len(sizes), None, 1, cap))
        out.append(("long_cap_%d" % cap, _shuffled_sizes([70, 3], 2, cap), 2, None, 1, cap))
    # the node form: a mask (one node) and three nodes with rows in none of them
    mask = rs.randint(-1, 1, 300)
    out.append(("node_mask", rs.randint(-1, 5, size=(2, 300)), 5, mask, 1, 16))
    out.append(("node_three", rs.randint(-1, 5, size=(2, 300)), 5, rs.randint(-1, 3, 300), 3, 4))
    out.append(("node_one_grouping", rs.randint(0, 9, 130), 9, rs.randint(-1, 3, 130), 3, 16))
    return out


def assert_same_plan(got, want):
    """got, want: SegmentPlan of numpy arrays"""
    assert got.n_out == want.n_out and len(got.levels) == len(want.levels)
    for level, ((tp, idx, order), (tp_w, idx_w, order_w)) in enumerate(zip(got.levels, want.levels)):
        assert tp.dtype == np.uint64 and np.array_equal(tp, tp_w), ("task_ptr", level)
        assert (idx is None) == (idx_w is None) == (level > 0)
        if idx is not None:
            assert idx.dtype == np.uint32 and np.array_equal(idx, idx_w), ("idx", level)
        assert order.dtype == np.uint32 and np.array_equal(order, order_w), ("order", level)
