"""TEST INFRASTRUCTURE — the cases tests/test_slots.py (CPU wave emulator) and tests/test_gpu_slots.py (the kernels) share for
the slot codec (csrc/slot_codec.h), and the codec itself in Python integers: what both are compared with.

Conventions: S slots of B bits, half = 2^(B-1), offset = sum_j half 2^(B j); row b holds x[b S + j], values past the end are 0;
pack: m = (sum_j x_j 2^(B j)) mod n; unpack: v = m if m <= max_int, m - n if m >= n - max_int, else status 1; u = v + offset,
status 2 unless 0 <= u < 2^(S B); x_j = ((u >> B j) & (2^B - 1)) - half."""
import random

import numpy as np

# B: 1 (up to 32 slots per word), 7 / 29 (cuts in mid-word), 31 / 32 / 33 (a slot equals or straddles a word), 63 (a slot across
# three words), 64 (the int64 boundary)
B_VALUES = (1, 7, 29, 31, 32, 33, 63, 64)


def bound_of(n):
    return (n // 3 - 1).bit_length() - 1


def slot_counts(n, B):
    """S = 1, 2, a middling one (odd, so that S*B is no multiple of 32 for every B but 32 and 64) and the widest the key allows"""
    widest = bound_of(n) // B
    return sorted({1, 2, (widest // 2) | 1, widest})


def offset_of(S, B):
    return sum(1 << (B * j + B - 1) for j in range(S))


def pack_int(row, B, n):
    return sum(x << (B * j) for j, x in enumerate(row)) % n


def unpack_int(m, S, B, n):
    """(status, values or None)"""
    max_int = n // 3 - 1
    if m <= max_int:
        v = m
    elif m >= n - max_int:
        v = m - n
    else:
        return 1, None
    u = v + offset_of(S, B)
    if u < 0 or u >> (S * B):
        return 2, None
    half = 1 << (B - 1)
    return 0, [((u >> (B * j)) & ((1 << B) - 1)) - half for j in range(S)]


def pattern_rows(S, B, rng, n_random=3):
    """rows that stress the borrow and carry chains: all -half (v = -offset), all half - 1, all 0 (u = offset), all -1, 0 with
    x_0 = -1 (m = n - 1: a borrow through every word and a carry back), only the top slot at +1 / -1, and random ones.
    (B = 1: a slot holds -1 or 0, so +1 becomes 0.)"""
    lo, hi = -(1 << (B - 1)), (1 << (B - 1)) - 1
    one = min(1, hi)
    rows = [[lo] * S, [hi] * S, [0] * S, [-1] * S, [-1] + [0] * (S - 1), [0] * (S - 1) + [one], [0] * (S - 1) + [-1]]
    rows += [[rng.randint(lo, hi) for _ in range(S)] for _ in range(n_random)]
    return rows


def status_rows(S, B, n):
    """(m, status) pairs: the ends of the two ranges (accepted by the range test, then too wide: 2), their neighbours in the gap
    (1), u = 2^(S B) - 1 and u = 0 (fine), u = 2^(S B) and u = -1 (2)"""
    max_int = n // 3 - 1
    off = offset_of(S, B)
    return [(max_int, 2), (n - max_int, 2), (max_int + 1, 1), (n - max_int - 1, 1),
            (((1 << (S * B)) - 1 - off) % n, 0), ((0 - off) % n, 0), (((1 << (S * B)) - off) % n, 2), ((-1 - off) % n, 2)]


def to_limbs(xs, words):
    raw = b"".join(int(x).to_bytes(4 * words, "little") for x in xs)
    return np.frombuffer(raw, np.uint32).reshape(len(xs), words).copy()


def to_ints(arr):
    w = arr.shape[1] * 4
    raw = np.ascontiguousarray(arr).tobytes()
    return [int.from_bytes(raw[i * w:(i + 1) * w], "little") for i in range(arr.shape[0])]


def as_int64(values):
    """Python ints in [-2^63, 2^63) -> int64 array"""
    return np.array(values, dtype=np.int64) if len(values) else np.zeros(0, dtype=np.int64)


def check_codec(pack, unpack, n, S, B, seed, min_rows=0, not_a_multiple_of=None, ragged=True):
    """pack(values int64, S, B) -> (rows, n_limbs) uint32 and unpack(m_rows, S, B) -> (int64 values, uint8 status) against Python
    integers on the pattern rows (repeated with fresh random rows up to min_rows; the row count, ragged row included, is kept
    off the multiples of not_a_multiple_of), a ragged last row, the round trip, and the status rows set among good rows."""
    words = (n.bit_length() + 31) // 32
    rng = random.Random(seed)
    rows = pattern_rows(S, B, rng)
    while len(rows) < min_rows:
        rows += pattern_rows(S, B, rng, n_random=5)
    if not_a_multiple_of and (len(rows) + (1 if ragged and S > 1 else 0)) % not_a_multiple_of == 0:
        rows += pattern_rows(S, B, rng, n_random=0)[:1]
    flat = [x for row in rows for x in row]
    if ragged and S > 1:
        tail = [rng.randint(-(1 << (B - 1)), (1 << (B - 1)) - 1) for _ in range(S - 1)]      # S - 1 values: the top slot is past the end
        flat += tail
        rows = rows + [tail + [0]]
    want = [pack_int(row, B, n) for row in rows]
    got = pack(as_int64(flat), S, B)
    assert got.shape == (len(rows), words)
    assert to_ints(got) == want, (S, B, "pack")
    vals, status = unpack(got, S, B)
    assert not status.any(), (S, B, "status of packed rows")
    assert vals.reshape(-1).tolist() == [x for row in rows for x in row], (S, B, "round trip")
    # the status rows, each between two good rows: only that row is flagged, and the good rows still decode
    cases = status_rows(S, B, n)
    ms, expect = [], []
    for k, (m, st) in enumerate(cases):
        ms += [want[k % len(want)], m]
        expect += [0, st]
    ms.append(want[-1])
    expect.append(0)
    vals, status = unpack(to_limbs(ms, words), S, B)
    assert status.tolist() == expect, (S, B, "status")
    vals = vals.reshape(len(ms), S)
    for k, (m, st) in enumerate(zip(ms, expect)):
        ref_st, ref_vals = unpack_int(m, S, B, n)
        assert ref_st == st
        if st == 0:
            assert vals[k].tolist() == ref_vals, (S, B, "values beside a flagged row", k)
