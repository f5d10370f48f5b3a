"""Per-key engines: the only place where Python integers meet the C-ABI.

An Engine owns one native Context (include/phe_hip.h) for one key on one GPU and exposes the five
hot functions of the reference on *batches* of Python ints or uint32 limb arrays:

    reference (scalar, phe/paillier.py)                  here (batched, HIP)
    PaillierPublicKey.raw_encrypt      :102-139    ->    Engine.raw_encrypt
    EncryptedNumber.obfuscate          :603-624    ->    Engine.obfuscate
    PaillierPrivateKey.raw_decrypt     :328-374    ->    Engine.raw_decrypt
    EncryptedNumber._raw_add           :705-719    ->    Engine.raw_add
    EncryptedNumber._raw_mul           :721-751    ->    Engine.raw_mul   (both branches)

There is no CPU implementation behind these: if lib/libphe_hip.so or a GPU is missing, they raise.
"""
import os
import threading

import numpy as np

from . import _chacha, _native
from ._device import DeviceArray


def default_device():
    """One process per GPU: LOCAL_RANK picks the device unless PHE_HIP_DEVICE overrides it.  A single process that fans out
    over several devices (PHE_HIP_DEVICES, phe/fleet.py) keeps its ordinary engine on the first of them."""
    v = os.environ.get("PHE_HIP_DEVICE")
    if v is not None and v.strip() != "":
        return int(v)
    from . import fleet
    devices = fleet.configured_devices()
    if devices:
        return devices[0]
    v = os.environ.get("LOCAL_RANK")
    if v is not None and v.strip() != "":
        return int(v)
    return 0


def random_lt_n(n, count):
    """`count` cryptographically random integers in [1, n) as Python ints (see random_lt_n_limbs)."""
    limbs = (n.bit_length() + 31) // 32
    return _native.limbs_to_ints(random_lt_n_limbs(n, count, limbs)) if count else []


_urandom = None


def _urandom_into(view):
    """Fill a writable buffer from the kernel CSPRNG (/dev/urandom, what os.urandom and random.SystemRandom read)
    without an intermediate bytes object."""
    global _urandom
    if _urandom is None:
        _urandom = open("/dev/urandom", "rb", buffering=0)
    mv = memoryview(view).cast("B")
    got = 0
    while got < len(mv):
        k = _urandom.readinto(mv[got:])
        if not k:
            raise OSError("/dev/urandom returned no data")
        got += k


def random_lt_n_limbs(n, count, limbs, out=None):
    """`count` cryptographically random integers in [1, n) as a (count, limbs) uint32 array — the bulk form of
    PaillierPublicKey.get_random_lt_n (phe/paillier.py:141-143, random.SystemRandom().randrange(1, n)): same
    source (the kernel CSPRNG), same distribution (rejection sampling on bit_length(n-1) bits), vectorised with
    numpy.  `out`: optional (count, limbs) uint32 array to fill (saves the first-touch cost of a fresh buffer)."""
    k = (n - 1).bit_length()
    top_limb, top_bits = (k - 1) // 32, k - 32 * ((k - 1) // 32)
    top_mask = np.uint32((1 << top_bits) - 1) if top_bits < 32 else np.uint32(0xffffffff)
    n_arr = _native.int_to_limbs(n, limbs)
    if out is None:
        out = np.empty((count, limbs), dtype=np.uint32)
    if count == 0:
        return out
    _urandom_into(out)
    rows = None                                  # None = every row (column views, no gather)
    while True:
        sub = out if rows is None else out[rows]
        if top_bits < 32:
            sub[:, top_limb] &= top_mask
        if top_limb + 1 < limbs:
            sub[:, top_limb + 1:] = 0
        # rows that are >= n (lexicographic compare from the most significant limb down) or zero are redrawn
        lt = np.zeros(len(sub), dtype=bool)
        undecided = np.ones(len(sub), dtype=bool)
        for j in range(top_limb, -1, -1):
            col = sub[:, j]
            lt |= undecided & (col < n_arr[j])
            undecided &= (col == n_arr[j])
            if not undecided.any():
                break
        maybe_zero = lt & (sub[:, top_limb] == 0)
        if maybe_zero.any():
            idx = np.nonzero(maybe_zero)[0]
            lt[idx] = sub[idx].any(axis=1)
        if rows is not None:
            out[rows] = sub
        bad = np.nonzero(~lt)[0]
        if len(bad) == 0:
            return out
        rows = bad if rows is None else rows[bad]
        fresh = np.empty((len(rows), limbs), dtype=np.uint32)
        _urandom_into(fresh)
        out[rows] = fresh


def random_bits_limbs(bits, count, limbs, out=None):
    """`count` cryptographically random integers in [0, 2^bits) as a (count, limbs) uint32 array: the short exponents rho of
    the short-exponent obfuscators (Engine.set_short_base), from the same kernel CSPRNG as random_lt_n_limbs — every value of
    the range is a valid exponent, so nothing is redrawn.  `out`: optional (count, limbs) uint32 array to fill."""
    bits, limbs = int(bits), int(limbs)
    if bits < 1 or bits > 32 * limbs:
        raise ValueError("bits must lie in [1, %d]" % (32 * limbs))
    if out is None:
        out = np.empty((count, limbs), dtype=np.uint32)
    if count == 0:
        return out
    _urandom_into(out)
    top_limb, top_bits = (bits - 1) // 32, bits - 32 * ((bits - 1) // 32)
    if top_bits < 32:
        out[:, top_limb] &= np.uint32((1 << top_bits) - 1)
    if top_limb + 1 < limbs:
        out[:, top_limb + 1:] = 0
    return out


def fresh_seed():
    """32 bytes from the kernel CSPRNG in a bytearray: the ChaCha20 key of ONE launch of the device draw (Engine.random_bits_dev,
    csrc/chacha_rows.h).  The only source of seeds — no clock, no pid, no `random`, no environment override — and the caller
    overwrites the bytearray with zeros as soon as the launch call has returned: a seed is as sensitive as the exponents it
    expands to."""
    seed = bytearray(32)
    _urandom_into(seed)
    return seed


_SEED_NONCE = (0, 0, 0)      # a seed keys one launch and is never used again: the nonce and the first counter are 0


def _seeded_parts(count, limbs):
    """[lo, hi) row ranges of a seeded draw: one launch takes at most 2^32 keystream blocks (the block counter never wraps)"""
    step = (1 << 32) // _chacha.blocks_per_row(limbs)
    return [(lo, min(count, lo + step)) for lo in range(0, count, step)]


def seeded_bits_limbs(bits, count, limbs):
    """random_bits_limbs by the host expander (phe/_chacha.py) under fresh seeds: the draw of the short exponents while the
    key's device_rng setting is on, where rows are wanted on the host"""
    bits, limbs = int(bits), int(limbs)
    if bits < 1 or bits > 32 * limbs:
        raise ValueError("bits must lie in [1, %d]" % (32 * limbs))
    out = np.empty((count, limbs), dtype=np.uint32)
    for lo, hi in _seeded_parts(count, limbs):
        seed = fresh_seed()
        try:
            out[lo:hi] = _chacha.chacha20_rows(seed, _SEED_NONCE, 0, bits, limbs, hi - lo)
        finally:
            seed[:] = bytes(len(seed))
    return out


class ObfuscatorPool:
    """Obfuscators r^n mod n^2 made ahead of time, each handed out ONCE (two ciphertexts sharing one reveal m1 - m2).
    The pool is an object of its own with its own lock because it outlives the engine it was filled through: when a key
    pair's private engine takes over from the public one (keys.PaillierPrivateKey._get_engine) both engines hold the SAME
    pool, so a thread still inside the old engine and a thread inside the new one cannot be handed the same rows.
    blocks: [DeviceArray, rows already used]; form: "pair" (rows in the engine's pair form) or "u32"."""

    def __init__(self):
        self.lock = threading.RLock()
        self.blocks = []

    def available(self):
        with self.lock:
            return sum(b.rows - used for b, used in self.blocks)

    def add(self, block):
        with self.lock:
            self.blocks.append([block, 0])

    def clear(self):
        with self.lock:
            self.blocks = []

    def take(self, count):
        """views of `count` unused rows (a list of DeviceArray views), or None if the pool is short; consumed"""
        with self.lock:
            if count <= 0 or sum(b.rows - used for b, used in self.blocks) < count:
                return None
            parts, need = [], count
            while need:
                block, used = self.blocks[0]
                k = min(need, block.rows - used)
                parts.append(block.rows_view(used, used + k))
                self.blocks[0][1] = used + k
                need -= k
                if self.blocks[0][1] == block.rows:
                    self.blocks.pop(0)
            return parts


# ---- grouped sums (EncryptedVector.segment_sum; csrc/segment_core.h) ------------------------------------------------------
# One limb group multiplies the rows of one TASK; a segment longer than this is cut into tasks of (almost) equal length, and
# the partial products are reduced by further levels of the same kernel.  Short tasks fill the GPU when the segments are few
# and keep the groups of a wavefront in step; long ones leave fewer partials to store and read again.  Measured with
# tools/bench_segment_sum.py (profiles/r08_segment_sum.json: 2048-bit key, 2^20 rows, 256 segments, kernels alone), caps
# 8 / 16 / 32 / 64 / 128 / 256: 203 / 196 / 174 / 125 / 120 / 104 M rows/s on residues, 637 / 638 / 570 / 399 / 404 / 378 M rows/s
# on pair rows.  8 and 16 tie within the spread of the repeats; 16 makes one level less.
SEGMENT_TASK_ROWS = 16


def _ranges(counts):
    """0 .. c-1 for every c of counts, concatenated"""
    counts = np.asarray(counts, dtype=np.int64)
    total = int(counts.sum())
    return np.arange(total, dtype=np.int64) - np.repeat(np.cumsum(counts) - counts, counts)


class SegmentPlan:
    """What Engine.segment_reduce_dev launches: `levels` is a list of (task_ptr uint64 (tasks + 1), idx uint32 or None, order
    uint32 (tasks)); level 0 reads the vector's rows through idx, every later level reads the partial products of the level
    before (idx None: task t covers the partials task_ptr[t] .. task_ptr[t + 1]).  The last level has one task per segment."""

    def __init__(self, levels, n_out):
        self.levels, self.n_out = levels, n_out

    @property
    def tasks(self):
        """tasks of every level"""
        return [len(order) for _, _, order in self.levels]

    @property
    def n_idx(self):
        """entries of level 0's idx: the (grouping, row) pairs that belong to a segment"""
        return len(self.levels[0][1])


# The numpy planner below (a stable argsort, a bincount, per level a repeat, a cumsum and a second argsort, then the index arrays
# going up) takes 14.1 - 15.8 ms for one grouping of 2^20 rows and 135 - 138 ms for eight; Engine.plan_segments_dev makes the same
# arrays on the device in 0.29 - 0.30 / 0.57 - 0.61 ms.  Its route costs some twenty launches and one small download however few
# the ids are, so EncryptedVector.segment_sum keeps the numpy planner below this many (grouping, row) pairs.  Measured with
# tools/bench_segment_plan.py (profiles/r14_segment_plan.json: planning alone, one grouping, 256 segments, F * rows = 2^10 ...
# 2^24 in powers of four, host / device in ms): 0.11 - 0.12 / 0.10 - 0.12 at 2^10 (a tie), 0.19 - 0.21 / 0.14 - 0.16 at 2^12,
# 0.25 - 0.28 / 0.15 at 2^14, 0.54 - 0.58 / 0.19 - 0.20 at 2^16, 2.05 - 2.13 / 0.19 - 0.21 at 2^18, 8.8 - 9.8 / 0.28 - 0.30 at
# 2^20, 74 - 77 / 0.39 - 0.43 at 2^22, 353 - 359 / 0.87 - 0.90 at 2^24.  2^12 is the crossover: the smallest size from which on
# the device route's slowest repeat is not above the host route's fastest.
SEGMENT_PLAN_DEVICE_MIN = 1 << 12


class DeviceSegmentPlan:
    """A SegmentPlan made and kept on the device (Engine.plan_segments_dev): `dev` is what Engine.segment_upload returns for a
    host plan — [(task_ptr, idx or None, order) DeviceArrays, ...] —, `tasks` the tasks of every level and `n_idx` the entries of
    idx that count (the block behind them is as long as the ids and its tail unspecified)."""

    def __init__(self, dev, tasks, n_out, n_idx):
        self.dev, self.tasks, self.n_out, self.n_idx = dev, tasks, n_out, n_idx

    def to_host(self):
        """the plan as a SegmentPlan of numpy arrays (tests, measurements)"""
        levels = []
        for (tp, idx, order), tasks in zip(self.dev, self.tasks):
            levels.append((tp.to_host().reshape(-1).view(np.uint64)[:tasks + 1].copy(),
                           idx.to_host().reshape(-1)[:self.n_idx].copy() if idx is not None else None,
                           order.to_host().reshape(-1)[:tasks].copy()))
        return SegmentPlan(levels, self.n_out)


def plan_segments(seg_ids, n_segments, cap=None):
    """seg_ids: (rows,) integers in [-1, n_segments) — -1 leaves the row out — or (F, rows): F groupings of the same rows, whose
    segment s of grouping f is output row f * n_segments + s.  Pure numpy; the ids are taken as valid."""
    cap = int(SEGMENT_TASK_ROWS if cap is None else cap)
    if cap < 2:
        raise ValueError("a task must be allowed at least two rows")
    ids = np.asarray(seg_ids, dtype=np.int64)
    if ids.ndim == 1:
        ids = ids[None, :]
    f, n = ids.shape
    n_out = f * int(n_segments)
    keep = ids >= 0
    group = (ids + np.arange(f, dtype=np.int64)[:, None] * int(n_segments))[keep]
    rows = np.broadcast_to(np.arange(n, dtype=np.int64), ids.shape)[keep]
    key = group.astype(np.uint16) if n_out <= 1 << 16 else group              # (16-bit keys: numpy sorts them by radix)
    idx = rows[np.argsort(key, kind="stable")].astype(np.uint32)             # the members of segment 0, of segment 1, ...
    counts = np.bincount(group, minlength=n_out).astype(np.int64) if n_out else np.zeros(0, np.int64)
    levels = []
    while True:
        per = np.maximum(1, -(-counts // cap))                                # tasks of every segment (an empty one: one empty task)
        seg = np.repeat(np.arange(n_out, dtype=np.int64), per)
        starts = (np.cumsum(counts) - counts)[seg] + (_ranges(per) * counts[seg]) // per[seg]
        task_ptr = np.append(starts, counts.sum()).astype(np.uint64)          # tasks are contiguous: each ends where the next starts
        order = np.argsort(-np.diff(task_ptr.astype(np.int64)), kind="stable").astype(np.uint32)
        levels.append((task_ptr, idx if not levels else None, order))
        if n_out == 0 or int(per.max()) <= 1:
            return SegmentPlan(levels, n_out)
        counts = per


# ---- running sums (EncryptedVector.cumsum; csrc/segment_core.h segment_scan_body) --------------------------------------------
# One limb group walks the consecutive rows of one TASK and stores the running product after every row; a sequence longer than
# this is cut into tasks of (almost) equal length, whose totals are reduced (segment_reduce_body), scanned in turn, and handed
# to the tasks as carries.  Short tasks fill the GPU and keep the groups of a wavefront in step; long ones leave fewer totals
# to reduce, store and scan again (1/cap of the rows per level).  Measured with tools/bench_cumsum.py
# (profiles/r09_cumsum.json: 2048-bit key, 2^20 pair rows in and out, kernels alone), caps 8 / 16 / 32 / 64 / 128 / 256:
# 315 / 300 / 275 / 211 / 173 / 101 M rows/s as one sequence (7 / 5 / 4 / 4 / 3 / 3 levels), 389 / 429 / 443 / 410 / 345 / 389
# M rows/s as 4096 blocks of 256 (the last: one task per block, no carries).  The long sequence wants 8, the histogram form 32;
# 16 is within 5 % of the best on either (the repeats spread by 2 - 6 %).
SCAN_TASK_ROWS = 16
SCAN_NO_CARRY = 0xFFFFFFFF

# ---- inversion on pair rows (Engine.pair_invert_dev; csrc/pair_invert.h) ---------------------------------------------------------
# One limb group walks a block of this many consecutive rows, once down (running products) and once up (inverses); the blocks'
# totals are the rows of the next level.  Short blocks fill the GPU and keep the dependent chain of a walk short; long ones leave
# fewer rows to the upper levels (1/(B - 1) of the rows in all) and fewer launches.  The products do not depend on it: the
# first row of a block costs none in either walk, so a level of n rows costs 3 (n - blocks) and all levels 3 (rows - 1).
# Measured with tools/bench_pair_invert.py (profiles/r16_pair_invert.json), blocks of 4 / 8 / 16 / 32 / 64: the shortest are
# the fastest at every size and key width measured (2^12, 2^16 and 2^20 rows).
PAIR_INVERT_BLOCK_ROWS = 4
# EncryptedVector.dot with signed weights inverts its rows in the form from this many rows on.  Below it the present route
# serves (the rows out of the form, phe_hip_invert_dev, phe_hip_multiexp_dev): at 3072 bits the multi-exponentiation over pair
# rows takes about 2.4 ms longer than the one over residues whatever the length, which the inversion wins back only from 2^16
# rows on (profiles/r16_pair_invert.json; at 1024 and 2048 bits the form wins at every size measured, from 2^8 rows on).  -vec and a - b are not slower
# at any size measured and take the form at every length.
PAIR_INVERT_MIN_ROWS = 1 << 16


class ScanPlan:
    """What Engine.scan_launch_dev launches: `levels` is a list of (task_ptr uint64 (tasks + 1), carry_idx uint32 (tasks) or
    None, n_rows, seq_len).  Level 0 covers the vector's rows, level k + 1 the totals of level k's tasks (one row per task).
    Task t of a level owns the consecutive rows task_ptr[t] .. task_ptr[t + 1], all inside one sequence of seq_len rows;
    carry_idx[t] is the row of the NEXT level's scan that holds the product of everything before the task in its sequence
    (t - 1), or SCAN_NO_CARRY for the first task of a sequence.  The last level has one task per sequence and no carries."""

    def __init__(self, levels, n_rows, block):
        self.levels, self.n_rows, self.block = levels, n_rows, block


def plan_scan(n_rows, block=None, cap=None):
    """The levels of a running sum over n_rows rows as n_rows / block sequences of `block` rows each (None: one sequence).
    Pure numpy; n_rows is taken to be a multiple of block."""
    cap = int(SCAN_TASK_ROWS if cap is None else cap)
    if cap < 2:
        raise ValueError("a task must be allowed at least two rows")
    n_rows = int(n_rows)
    seq_len = max(1, n_rows if block is None else int(block))
    n_seq = n_rows // seq_len
    levels, rows = [], n_rows
    while True:
        per = -(-seq_len // cap)                                              # tasks of every sequence, of (almost) equal length
        within = np.tile(np.arange(per, dtype=np.int64), n_seq)
        starts = np.repeat(np.arange(n_seq, dtype=np.int64) * seq_len, per) + (within * seq_len) // per
        task_ptr = np.append(starts, rows).astype(np.uint64)                  # tasks are contiguous: each ends where the next starts
        carry_idx = None
        if per > 1:
            carry_idx = np.where(within == 0, SCAN_NO_CARRY, np.arange(len(within), dtype=np.int64) - 1).astype(np.uint32)
        levels.append((task_ptr, carry_idx, rows, seq_len))
        if per == 1:
            return ScanPlan(levels, n_rows, seq_len)
        rows, seq_len = n_seq * per, per


# Every public Engine method runs under the engine's re-entrant lock (see _native.serialised).  A key's engine owns
# shared state: the obfuscator pool, whose entries must never be handed out twice (two ciphertexts sharing r^n reveal
# m1 - m2), the host staging buffers, the native context's window tables and launch stream.
@_native.serialised
class Engine:
    def __init__(self, n, p=None, q=None, hp=None, hq=None, p_inverse=None, device=None):
        self._lock = threading.RLock()
        self.n = n
        self.nsquare = n * n
        self.max_int = n // 3 - 1
        self.device = default_device() if device is None else device
        self.ctx = _native.Context(n, p, q, hp, hq, p_inverse, device=self.device)
        self.n_limbs = self.ctx.n_limbs
        self.ct_limbs = self.ctx.ct_limbs
        self._obf = ObfuscatorPool()

    # ---- reusable host staging (a fresh 32 MB numpy buffer costs more in page faults than the kernel it feeds) ---
    def scratch(self, name, rows, cols):
        """A (rows, cols) uint32 view of a grow-only buffer owned by this engine; contents are transient: valid
        until the next scratch(name, ...) call."""
        if not hasattr(self, "_scratch"):
            self._scratch = {}
        need = rows * cols
        buf = self._scratch.get(name)
        if buf is None or buf.size < need:
            buf = np.empty(max(need, 1), dtype=np.uint32)
            self._scratch[name] = buf
        return buf[:need].reshape(rows, cols)

    # ---- limb helpers -------------------------------------------------------------------------
    def plain_limbs(self, ints):
        return _native.ints_to_limbs(ints, self.n_limbs)

    def cipher_limbs(self, ints):
        return _native.ints_to_limbs(ints, self.ct_limbs)

    @staticmethod
    def to_ints(arr):
        return _native.limbs_to_ints(arr)

    def _as_plain(self, x):
        return x if isinstance(x, np.ndarray) else self.plain_limbs(x)

    def _as_cipher(self, x):
        # Python ints are reduced mod n^2 on the way in (the reference's mulmod/powmod accept any int and
        # reduce implicitly; the kernels want residues)
        return x if isinstance(x, np.ndarray) else self.cipher_limbs([v % self.nsquare for v in x])

    # ---- the five hot functions (limb arrays in, limb arrays out) ------------------------------
    def owner_encrypt(self):
        """True when this engine holds the private key and the library offers the CRT form of raw_encrypt for the key
        width (include/phe_hip.h phe_hip_encrypt_owner_dev): r^n mod n^2 from r^n mod p^2 and r^n mod q^2 — about half
        the multiply-adds, the same bits.  Every encryption path of the engine takes it then."""
        ok = self.__dict__.get("_owner_ok")
        if ok is None:
            probe = getattr(self.ctx, "owner_encrypt_offered", None)
            ok = self._owner_ok = bool(probe()) if probe and os.environ.get("PHE_HIP_OWNER_ENCRYPT", "1") != "0" else False
        return ok

    def _encrypt_dev(self, m_ptr, r_ptr, c_ptr, rows, stream=0):
        fn = self.ctx.encrypt_owner_dev if self.owner_encrypt() else self.ctx.encrypt_dev
        fn(m_ptr, r_ptr, c_ptr, rows, stream)

    def raw_encrypt(self, m, r):
        """(1 + n*m) * r^n mod n^2 per row.  m is reduced mod n on the way in (value-identical to the
        reference's `% nsquare`, which lets m = n, n+1 wrap to 0, 1: phe/tests/paillier_test.py:114-126)."""
        if not isinstance(m, np.ndarray):
            m = self.plain_limbs([v % self.n for v in m])
        if self.owner_encrypt():
            return self.ctx.encrypt_owner(m, self._as_plain(r))
        return self.ctx.encrypt(m, self._as_plain(r))

    def obfuscate(self, c, r):
        c, r = self._as_cipher(c), self._as_plain(r)
        if self.owner_encrypt():
            # r^n through the key owner's CRT halves (raw_encrypt of the plaintext 0), then one product: same bits
            rn = self.ctx.encrypt_owner(np.zeros((r.shape[0], self.n_limbs), dtype=np.uint32), r)
            return self.ctx.mulmod(c, rn)
        return self.ctx.obfuscate(c, r)

    def _obfuscate_dev(self, c_ptr, r_ptr, out_ptr, rows, stream=0):
        """c * r^n on resident rows: the fused / composed public kernels, or — for a key owner — r^n from the CRT halves
        into `out`, then the product with c in place"""
        if not self.owner_encrypt():
            self.ctx.obfuscate_dev(c_ptr, r_ptr, out_ptr, rows, stream)
            return
        zeros = self.__dict__.get("_zero_plain")
        if zeros is None or zeros.rows < rows:
            zeros = self._zero_plain = DeviceArray.from_host(self.ctx, np.zeros((max(rows, 1 << 16), self.n_limbs), dtype=np.uint32))
        self.ctx.encrypt_owner_dev(zeros.ptr, r_ptr, out_ptr, rows, stream)
        self.ctx.mulmod_dev(c_ptr, out_ptr, out_ptr, rows, stream)

    def raw_decrypt(self, c):
        return self.ctx.decrypt(self._as_cipher(c))

    def raw_add(self, a, b):
        return self.ctx.mulmod(self._as_cipher(a), self._as_cipher(b))

    def add_plain(self, c, plaintexts):
        """c * (1 + n*m) mod n^2 per row: E(a) + b for a plaintext encoding b (phe/paillier.py:673-675)."""
        if not isinstance(plaintexts, np.ndarray):
            plaintexts = self.plain_limbs([v % self.n for v in plaintexts])
        return self.ctx.add_plain(self._as_cipher(c), plaintexts)

    def raw_mul(self, c, scalars):
        """Per row: powmod(c, s, n^2) if s < n - max_int, else powmod(invert(c, n^2), n - s, n^2) — the same
        partition as phe/paillier.py:745-751 (the two branches give different ciphertext bits).
        `scalars` are Python ints already validated to lie in [0, n)."""
        c = self._as_cipher(c)
        n, threshold = self.n, self.n - self.max_int
        neg = [i for i, s in enumerate(scalars) if s >= threshold]
        exps = [n - s if s >= threshold else s for s in scalars]
        base = c
        if neg:
            base = c.copy()
            idx = np.asarray(neg, dtype=np.int64)
            base[idx] = self.ctx.invert(np.ascontiguousarray(c[idx]))
        width = max(1, (max(e.bit_length() for e in exps) + 31) // 32) if exps else 1
        return self.ctx.powmod(base, _native.ints_to_limbs(exps, width))

    @staticmethod
    def _mag_limbs(mag):
        mag = np.ascontiguousarray(mag, dtype=np.uint64)
        bits = int(mag.max()).bit_length() if len(mag) else 1
        return mag.view(np.uint32).reshape(len(mag), 2)[:, :1 if bits <= 32 else 2].copy(), max(bits, 1)

    def raw_mul_signed(self, c, mag, neg):
        """raw_mul for scalars given as sign + 64-bit magnitude (the array form of the codec): a negative scalar -v
        is the residue n - v >= n - max_int, so it takes the inverse branch with exponent v (phe/paillier.py:745-749)."""
        c = self._as_cipher(c)
        exps, _ = self._mag_limbs(mag)
        base = c
        if neg.any():
            idx = np.nonzero(neg)[0]
            base = c.copy()
            base[idx] = self.ctx.invert(np.ascontiguousarray(c[idx]))
        return self.ctx.powmod(base, exps)

    def _inverted_where(self, c, neg):
        """a vector equal to c with the rows where `neg` holds replaced by invert(c_i, n^2): the base of the negative-scalar branch
        of _raw_mul (phe/paillier.py:745-749).  Few negative rows (under a quarter): only those are inverted — gathered, inverted
        as a batch of their own (the simultaneous-inversion tree costs 3 products per row it is given), scattered into a copy;
        otherwise the whole vector is inverted and selected per row.  ZeroDivisionError carries the row's index in c."""
        neg = np.asarray(neg, dtype=bool)
        count = int(neg.sum())
        if count * 4 < c.rows and hasattr(self.ctx, "gather_rows_dev"):
            idx = np.nonzero(neg)[0].astype(np.uint32)
            idx_d = DeviceArray.from_host(self.ctx, idx)
            sub = DeviceArray(self.ctx, count, self.ct_limbs)
            self.ctx.gather_rows_dev(c.ptr, c.rows, idx_d.ptr, sub.ptr, self.ct_limbs, count)
            inv = DeviceArray(self.ctx, count, self.ct_limbs)
            try:
                self.ctx.invert_dev(sub.ptr, inv.ptr, count)
            except ZeroDivisionError as e:
                if getattr(e, "bad_index", None) is not None and e.bad_index < count:
                    e.bad_index = int(idx[e.bad_index])
                raise
            base = c.copy()
            self.ctx.scatter_rows_dev(inv.ptr, idx_d.ptr, base.ptr, base.rows, self.ct_limbs, count)
            self.ctx.sync()
            return base
        inv = DeviceArray(self.ctx, c.rows, self.ct_limbs)
        self.ctx.invert_dev(c.ptr, inv.ptr, c.rows)
        mask = DeviceArray.from_host(self.ctx, neg.astype(np.uint8), dtype=np.uint8)
        base = DeviceArray(self.ctx, c.rows, self.ct_limbs)
        self.ctx.select_rows_dev(c.ptr, inv.ptr, mask.ptr, base.ptr, self.ct_limbs, c.rows)
        self.ctx.sync()
        return base

    def raw_mul_signed_dev(self, c, mag, neg):
        exps, bits = self._mag_limbs(mag)
        base = c
        if neg.any():
            base = self._inverted_where(c, neg)
        e = DeviceArray.from_host(self.ctx, exps)
        out = DeviceArray(self.ctx, base.rows, self.ct_limbs)
        self.ctx.powmod_dev(base.ptr, e.ptr, exps.shape[1], bits, out.ptr, base.rows)
        self.ctx.sync()
        return out

    def __del__(self):
        try:
            st = self.__dict__.get("_stream")
            if st:
                self.ctx.stream_destroy(st)
        except Exception:
            pass

    @staticmethod
    def shifted_limbs(mag, shift_bits):
        """(mag[i] << shift_bits[i]) as little-endian uint32 limb rows, without a Python integer per element: the
        exponents k_i * BASE^delta_i of an aligned dot product (mag: uint64 magnitudes, shift_bits: int64 >= 0).
        Returns (limbs (batch, width), largest bit length)."""
        mag = np.ascontiguousarray(mag, dtype=np.uint64).reshape(-1)
        sh = np.ascontiguousarray(shift_bits, dtype=np.int64).reshape(-1)
        count = len(mag)
        top = int(mag.max()) if count else 0
        if top == 0:
            return np.zeros((count, 1), dtype=np.uint32), 1
        nz = mag != 0
        sh = np.where(nz, sh, 0)              # a zero stays zero whatever its shift: it must not size or index the rows
        # exact bit length of every magnitude: float64 log2 can be off by one near powers of two, so fix it up
        bl = np.zeros(count, dtype=np.int64)
        est = np.floor(np.log2(mag[nz].astype(np.float64))).astype(np.int64) + 1
        est = np.minimum(est, 64)
        m_nz = mag[nz]
        too_big = (est > 1) & ((m_nz >> (est - 1).astype(np.uint64)) == 0)
        est[too_big] -= 1
        too_small = (est < 64) & ((m_nz >> np.minimum(est, 63).astype(np.uint64)) != 0)
        est[too_small] += 1
        bl[nz] = est
        bits = int((bl + sh).max())
        width = max(1, (bits + 31) // 32)
        out = np.zeros((count, width + 3), dtype=np.uint32)       # 3 spill words, cut off below
        word = sh >> 5
        bo = (sh & 31).astype(np.uint64)
        lo = mag << bo                                            # low 64 bits of the shifted value
        hi = np.where(bo == 0, np.uint64(0), mag >> ((np.uint64(64) - bo) & np.uint64(63)))   # the bits shifted out
        rows = np.arange(count)
        out[rows, word] = (lo & np.uint64(0xffffffff)).astype(np.uint32)
        out[rows, word + 1] = (lo >> np.uint64(32)).astype(np.uint32)
        out[rows, word + 2] = hi.astype(np.uint32)
        return np.ascontiguousarray(out[:, :width]), max(bits, 1)

    @staticmethod
    def _exp_limbs(exps):
        """exponents (uint64 array or Python ints) -> (batch, width) uint32 limbs and the largest bit length"""
        if isinstance(exps, np.ndarray):
            return Engine._mag_limbs(exps)
        exps = list(exps)
        bits = max(1, max((e.bit_length() for e in exps), default=1))
        return _native.ints_to_limbs(exps, (bits + 31) // 32), bits

    def raw_dot(self, c, exps, neg):
        """prod_i b_i^e_i mod n^2 with b_i = c_i, or invert(c_i, n^2) where neg[i] — the ciphertext of sum_i k_i * x_i
        exactly as a chain of _raw_mul (phe/paillier.py:745-751: scalars at or above n - max_int take the inverted
        base with exponent n - k) and _raw_add (:705-719) leaves it: the product of canonical residues does not
        depend on the order of the factors.  One k_multiexp_split launch plus the k_mulmod tree over its chunk
        products (include/phe_hip.h phe_hip_multiexp).  c: host limb array or DeviceArray.  Returns a Python int."""
        limbs, bits = exps if isinstance(exps, tuple) else self._exp_limbs(exps)
        neg = np.asarray(neg, dtype=bool)
        if isinstance(c, DeviceArray) and self.pair_form() and c.cols == self.pair_form() != self.ct_limbs:
            # rows resident in the pair form: the multi-exponentiation reads them as they are — no conversion of every ciphertext
            # into the form (include/phe_hip.h phe_hip_pair_multiexp_rows_dev); the rows of negative scalars are inverted in the
            # form first (phe_hip_pair_invert_dev), where the backend can
            if neg.any():
                if not self.has_pair_invert():
                    raise ValueError("pair-form rows take non-negative scalars only")
                c = self._inverted_where_pair(c, neg)
            e = DeviceArray.from_host(self.ctx, limbs)
            out = DeviceArray(self.ctx, 1, self.ct_limbs)
            self.ctx.pair_multiexp_rows_dev(c.ptr, e.ptr, limbs.shape[1], bits, out.ptr, c.rows, 1)
            self.ctx.sync()
            return self.to_ints(out.to_host())[0]
        if isinstance(c, DeviceArray):
            base = c
            if neg.any():
                inv = DeviceArray(self.ctx, c.rows, self.ct_limbs)
                self.ctx.invert_dev(c.ptr, inv.ptr, c.rows)
                mask = DeviceArray.from_host(self.ctx, neg.astype(np.uint8), dtype=np.uint8)
                base = DeviceArray(self.ctx, c.rows, self.ct_limbs)
                self.ctx.select_rows_dev(c.ptr, inv.ptr, mask.ptr, base.ptr, self.ct_limbs, c.rows)
            e = DeviceArray.from_host(self.ctx, limbs)
            out = DeviceArray(self.ctx, 1, self.ct_limbs)
            self.ctx.multiexp_dev(base.ptr, e.ptr, limbs.shape[1], bits, out.ptr, c.rows)
            self.ctx.sync()
            return self.to_ints(out.to_host())[0]
        base = self._as_cipher(c)
        if neg.any():
            idx = np.nonzero(neg)[0]
            base = base.copy()
            base[idx] = self.ctx.invert(np.ascontiguousarray(base[idx]))
        return self.to_ints(self.ctx.multiexp(base, limbs))[0]

    def raw_matvec(self, c, exps, neg):
        """rows of raw_dot over the same ciphertexts: out[r] = prod_i b_i^exps[r][i] mod n^2, b_i = c_i or
        invert(c_i, n^2) where neg[r][i] (include/phe_hip.h phe_hip_multiexp_rows_dev: the tables of a chunk of
        ciphertexts serve a block of rows; the vector is inverted once with the simultaneous-inversion tree when any
        entry is negative).  exps: (rows, batch) uint64 array or list of rows of Python ints; neg: (rows, batch) bool.
        c: host limb array or DeviceArray; returns the same kind, (rows, ct_limbs)."""
        neg = np.asarray(neg, dtype=bool)
        rows, batch = neg.shape
        if isinstance(exps, tuple):                              # (limb rows (rows*batch, width), bits): shifted_limbs
            limbs, bits = exps[0].reshape(rows, batch, -1), exps[1]
        elif isinstance(exps, np.ndarray):
            e64 = np.ascontiguousarray(exps, dtype=np.uint64)
            bits = int(e64.max()).bit_length() if e64.size else 1
            limbs = e64.view(np.uint32).reshape(rows, batch, 2)[:, :, :1 if bits <= 32 else 2].copy()
        else:
            bits = max(1, max((v.bit_length() for row in exps for v in row), default=1))
            width = (bits + 31) // 32
            limbs = np.stack([_native.ints_to_limbs(list(row), width) for row in exps]) if rows else np.zeros((0, batch, width), np.uint32)
        bits = max(bits, 1)
        on_dev = isinstance(c, DeviceArray)
        any_neg = bool(neg.any())
        if on_dev and self.pair_form() and c.cols == self.pair_form() != self.ct_limbs:
            if any_neg:
                raise ValueError("pair-form rows take non-negative scalars only")
            e = DeviceArray.from_host(self.ctx, limbs.reshape(rows * batch, -1))
            out = DeviceArray(self.ctx, rows, self.ct_limbs)
            self.ctx.pair_multiexp_rows_dev(c.ptr, e.ptr, limbs.shape[2], bits, out.ptr, batch, rows)
            self.ctx.sync()
            return out
        info = self.ctx.info()
        if not (info.get("emulated") or info.get("engine_pub") == "split"):
            # keys without a split geometry: row by row on the single-row entry point
            out = [self.raw_dot(c, (np.ascontiguousarray(limbs[r]), bits), neg[r]) for r in range(rows)]
            host = self.cipher_limbs(out)
            return DeviceArray.from_host(self.ctx, host) if on_dev else host
        if on_dev:
            inv = None
            if any_neg:
                inv = DeviceArray(self.ctx, c.rows, self.ct_limbs)
                self.ctx.invert_dev(c.ptr, inv.ptr, c.rows)
            e = DeviceArray.from_host(self.ctx, limbs.reshape(rows * batch, -1))
            mask = DeviceArray.from_host(self.ctx, neg.astype(np.uint8).reshape(-1), dtype=np.uint8) if any_neg else None
            out = DeviceArray(self.ctx, rows, self.ct_limbs)
            self.ctx.multiexp_rows_dev(c.ptr, inv.ptr if inv else None, e.ptr, mask.ptr if mask else None, limbs.shape[2], bits,
                                       out.ptr, batch, rows)
            self.ctx.sync()
            return out
        base = self._as_cipher(c)
        inv = self.ctx.invert(base) if any_neg else None
        return self.ctx.multiexp_rows(base, inv, limbs, neg.astype(np.uint8) if any_neg else None)

    def has_split_engine(self):
        info = self.ctx.info()
        return bool(info.get("emulated") or info.get("engine_pub") == "split")

    def raw_matvec_csr(self, c, row_ptr, cols, exps, neg, rows):
        """out[r] = prod over the entries of row r of b[col]^exp (b = c[col], or its inverse where neg[entry]): the
        table-lookup form of raw_matvec (include/phe_hip.h phe_hip_multiexp_csr_dev) — tables of the whole vector
        once, then one ladder per row over its entries only.  row_ptr / cols: CSR (None, None = dense rows);
        exps: (limb rows (entries, width), bits) as shifted_limbs returns them; neg: (entries,) bool or None.
        Rows are visited longest first.  c: host limb array or DeviceArray; returns the same kind."""
        limbs, bits = exps
        any_neg = neg is not None and bool(np.asarray(neg).any())
        order = None
        if row_ptr is not None:
            row_ptr = np.ascontiguousarray(row_ptr, dtype=np.uint64)
            counts = np.diff(row_ptr.astype(np.int64))
            order = np.argsort(-counts, kind="stable").astype(np.uint32)
        if isinstance(c, DeviceArray):
            inv = None
            if any_neg:
                inv = DeviceArray(self.ctx, c.rows, self.ct_limbs)
                self.ctx.invert_dev(c.ptr, inv.ptr, c.rows)
            dev = lambda a, dt: DeviceArray.from_host(self.ctx, np.ascontiguousarray(a, dtype=dt).reshape(-1), dtype=dt)
            e = DeviceArray.from_host(self.ctx, limbs)
            rp = DeviceArray.from_host(self.ctx, row_ptr.view(np.uint32).reshape(-1, 2)) if row_ptr is not None else None
            cl = DeviceArray.from_host(self.ctx, np.ascontiguousarray(cols, dtype=np.uint32)) if cols is not None else None
            ng = dev(np.asarray(neg).astype(np.uint8), np.uint8) if any_neg else None
            od = DeviceArray.from_host(self.ctx, order) if order is not None else None
            out = DeviceArray(self.ctx, rows, self.ct_limbs)
            ptr = lambda a: a.ptr if a is not None else None
            self.ctx.multiexp_csr_dev(c.ptr, ptr(inv), c.rows, ptr(rp), ptr(cl), e.ptr, ptr(ng), limbs.shape[1], bits, ptr(od),
                                      out.ptr, rows)
            self.ctx.sync()
            return out
        base = self._as_cipher(c)
        inv = self.ctx.invert(base) if any_neg else None
        return self.ctx.multiexp_csr(base, inv, row_ptr, cols, limbs, np.asarray(neg).astype(np.uint8) if any_neg else None,
                                     order, rows)

    # ---- the decimal wire format of ciphertext vectors (docs/serialisation.rst:24-43; str(int) / int(str) per
    #      element in the reference) ---------------------------------------------------------------------------
    def decimal_strings(self, c):
        """ciphertext rows (host limb array or DeviceArray) -> list of str, exactly [str(int) ...]: the base
        conversion runs on the device (csrc/radix_conv.h), the host only strips the '0' padding"""
        if isinstance(c, DeviceArray):
            digits = self.ctx.to_decimal_dev(c.ptr, c.cols, c.rows)
        else:
            digits = self.ctx.to_decimal(c)
        width = digits.shape[1]
        raw = digits.tobytes()
        return [raw[i:i + width].lstrip(b"0").decode("ascii") or "0" for i in range(0, len(raw), width)]

    def limbs_from_decimal(self, strings, words=None):
        """list of decimal strings -> (rows, words) limb array (int(str) per element in the reference, then the
        reduction the kernels expect is the caller's business).  ValueError for anything int() would reject here
        (signs, spaces and underscores are not part of the wire format) or a value beyond `words` words."""
        words = words or self.ct_limbs
        if not strings:
            return np.zeros((0, words), dtype=np.uint32)
        width = max(1, max(len(s) for s in strings))
        raw = b"".join(s.encode("ascii").rjust(width, b"0") for s in strings)
        digits = np.frombuffer(raw, dtype=np.uint8).reshape(len(strings), width)
        return self.ctx.from_decimal(digits, words)

    def powmod_n2(self, base, exps):
        exps = list(exps)
        width = max(1, (max(e.bit_length() for e in exps) + 31) // 32) if exps else 1
        return self.ctx.powmod(self._as_cipher(base), _native.ints_to_limbs(exps, width))

    def invert_n2(self, a):
        return self.ctx.invert(self._as_cipher(a))

    # ---- the same five functions on device-resident arrays (DeviceArray in, DeviceArray out) --------------
    def upload_plain(self, ints_or_limbs):
        return DeviceArray.from_host(self.ctx, self._as_plain(ints_or_limbs))

    def upload_cipher(self, ints_or_limbs):
        return DeviceArray.from_host(self.ctx, self._as_cipher(ints_or_limbs))

    def raw_encrypt_dev(self, m, r):
        """m: Python ints, limb rows, or RESIDENT plaintext rows (a DeviceArray, e.g. of slots_pack_dev: they stay in HBM)"""
        if not isinstance(m, DeviceArray):
            m = self.upload_plain([v % self.n for v in m] if not isinstance(m, np.ndarray) else m)
        r = self.upload_plain(r)
        if r.rows != m.rows:
            raise ValueError("%d obfuscators for %d plaintexts" % (r.rows, m.rows))
        out = DeviceArray(self.ctx, m.rows, self.ct_limbs)
        self._encrypt_dev(m.ptr, r.ptr, out.ptr, m.rows)
        self.ctx.sync()
        return out

    def _launch_stream(self):
        """a non-blocking stream for pipelined launches (created on first use; 0 = NULL stream if the backend has none)"""
        st = self.__dict__.get("_stream")
        if st is None:
            st = self.ctx.stream_create() if hasattr(self.ctx, "stream_create") else 0
            self._stream = st
        return st

    def raw_encrypt_fresh(self, m, device):
        """raw_encrypt with freshly drawn obfuscators, in chunks: the draw (the kernel CSPRNG, host side) and the upload
        of chunk k+1 overlap the kernel of chunk k — the kernels are queued on a non-blocking stream, so the blocking
        copies (NULL stream) do not wait for them; the first chunk is half size to shorten the exposed prologue.
        m: (count, n_limbs) plaintext limbs, on the host or RESIDENT (a DeviceArray: its rows are read where they are).
        Returns a DeviceArray or a host array."""
        resident = isinstance(m, DeviceArray)
        count = m.rows if resident else m.shape[0]
        st = self._launch_stream()
        short = self.short_base()
        el = (short[1] + 31) // 32 if short else 0
        seeded = bool(short) and self.short_device_rng()  # rho drawn where the comb kernel reads it: no host buffer, no upload
        out = DeviceArray(self.ctx, count, self.ct_limbs)
        host = None if device else np.empty((count, self.ct_limbs), dtype=np.uint32)
        keep = []                                         # operand buffers stay alive until the final sync
        lo, chunk, prev = 0, 1 << 15, None                # chunks are multiples of the groups in flight (32768 at 2048 bits)
        while lo < count:
            hi = min(count, lo + chunk)
            if seeded:
                r = None
            elif short:                                   # short-exponent obfuscators: rho instead of r, h_s^rho instead of r^n
                r = random_bits_limbs(short[1], hi - lo, el, out=self.scratch("rho", hi - lo, el))
            else:
                r = random_lt_n_limbs(self.n, hi - lo, self.n_limbs, out=self.scratch("r", hi - lo, self.n_limbs))
            m_d = m.rows_view(lo, hi) if resident else DeviceArray.from_host(self.ctx, m[lo:hi])
            if seeded:
                r_d = self.random_bits_dev(short[1], hi - lo, el, st)
            else:
                r_d = DeviceArray.from_host(self.ctx, r)  # synchronous copy: the scratch buffer is free again
            keep += [m_d, r_d]
            if host is not None and st:
                self.ctx.sync(st)                         # the previous chunk is complete (its successor starts right away)
            if short:
                self._short_launch(r_d, None, False, m_d, out.rows_view(lo, hi), False, st, keep)
            else:
                self._encrypt_dev(m_d.ptr, r_d.ptr, out.rows_view(lo, hi).ptr, hi - lo, st)
            if host is not None and st and prev is not None:
                self.ctx.d2h(host[prev[0]:prev[1]], out.rows_view(*prev).ptr)     # download under this chunk's kernel
            prev = (lo, hi)
            lo, chunk = hi, 1 << 16
        self.ctx.sync(st)
        if host is None:
            return out
        if st and prev is not None:
            self.ctx.d2h(host[prev[0]:prev[1]], out.rows_view(*prev).ptr)
            return host
        return out.to_host()

    # ---- offline / online split: obfuscators r^n mod n^2 made ahead of time -------------------------------------------
    # r^n is the expensive factor of an encryption and does not depend on the plaintext (phe/paillier.py:137 draws r
    # and exponentiates at encryption time).  A pool of them, each used ONCE, turns the online part of encrypt_batch /
    # obfuscate into one product per element: c = (1 + n m) * r^n — the same value raw_encrypt(m, r) returns for that r.
    def fill_obfuscator_pool(self, count):
        """draw `count` fresh r in [1, n) and keep r^n mod n^2 in HBM (raw_encrypt of the plaintext 0: 1 + n*0 = 1) — as
        rows of the engine's pair form where it has one: the online part of an encryption is then one exit from that form
        with the plaintext folded in (Engine.encrypt_from_obfuscators)"""
        if count <= 0:
            return self.obfuscators_available()
        if self.short_base():
            # short-exponent obfuscators h_s^rho: the comb leaves pair rows directly (no exit and no conversion back)
            self._obf.add(self.short_fresh_dev(count, want_pair=bool(self.pair_form())))
            return self.obfuscators_available()
        zeros = np.zeros((count, self.n_limbs), dtype=np.uint32)
        block = self.raw_encrypt_fresh(zeros, device=True)
        if self.pair_form():
            block = self.to_pair_dev(block)
        self._obf.add(block)
        return self.obfuscators_available()

    def clear_obfuscator_pool(self):
        """drop the obfuscators made ahead of time (nothing was handed out twice; the unused ones are simply forgotten)"""
        self._obf.clear()

    def obfuscators_available(self):
        return self._obf.available()

    def take_pool_rows(self, count):
        """`count` unused pool rows as ONE DeviceArray (a view where possible), or None; consumed.  The rows come in the form
        the engine works in NOW (pair_form(): pair rows, else ciphertext words): a block filled through another engine of the
        key pair, or under another PHE_HIP_PAIR_FORM setting, may be in the other form — every part is brought to one form
        BEFORE the parts are joined (a copy at the wrong row stride would corrupt the obfuscators)."""
        parts = self._obf.take(count)
        if parts is None:
            return None
        want = self.pair_form() or self.ct_limbs
        if want not in {part.cols for part in parts}:     # (an emulated / full-width engine never sees pair blocks)
            want = parts[0].cols

        def normal(part):
            if part.cols == want:
                return part
            return self.from_pair_dev(part) if want == self.ct_limbs else self.to_pair_dev(part)
        parts = [normal(part) for part in parts]
        if len(parts) == 1:
            return parts[0]
        out = DeviceArray(self.ctx, count, want)
        lo = 0
        for part in parts:
            self.ctx.d2d(out.ptr + lo * want * 4, part.ptr, part.nbytes)
            lo += part.rows
        self.ctx.sync()
        return out

    _take_pool_rows = take_pool_rows

    def take_obfuscators(self, count):
        """`count` unused obfuscators r^n mod n^2 as plain ciphertext rows (DeviceArray of ct_limbs words), or None if
        the pool is short; they are consumed: nothing is handed out twice"""
        rows = self.take_pool_rows(count)
        if rows is None or rows.cols == self.ct_limbs:
            return rows
        return self.from_pair_dev(rows)

    def encrypt_from_obfuscators(self, plaintexts):
        """raw_encrypt(m_i, r_i) for pooled r_i (each used once): (1 + n*m_i) * r_i^n mod n^2 as a DeviceArray, or None
        if the pool is short.  plaintexts: (count, n_limbs) limb rows, Python ints, or resident rows (a DeviceArray)."""
        if not isinstance(plaintexts, (np.ndarray, DeviceArray)):
            plaintexts = self.plain_limbs([v % self.n for v in plaintexts])
        rows = self.take_pool_rows(plaintexts.shape[0])
        if rows is None:
            return None
        if rows.cols == self.ct_limbs:
            return self.add_plain_dev(rows, plaintexts)
        return self.from_pair_dev(rows, plaintexts)

    def peek_obfuscators(self, count):
        """the next `count` unused obfuscators r^n mod n^2 as Python ints, WITHOUT consuming them (tests, diagnostics)"""
        out = []
        with self._obf.lock:
            for block, used in self._obf.blocks:
                k = min(count - len(out), block.rows - used)
                if k <= 0:
                    break
                view = block.rows_view(used, used + k)
                if view.cols != self.ct_limbs:
                    view = self.from_pair_dev(view)
                out += self.to_ints(view.to_host())
        return out

    # ---- resident rows in the pair form (include/phe_hip.h "pair form") ---------------------------------------------------
    def pair_form(self):
        """words of a pair-form row (0: not offered — no split-modulus engine, an emulated backend, PHE_HIP_PAIR_FORM=0)"""
        w = self.__dict__.get("_pair_words")
        if w is None:
            probe = getattr(self.ctx, "pair_words", None)
            w = self._pair_words = int(probe()) if probe and os.environ.get("PHE_HIP_PAIR_FORM", "1") != "0" else 0
        return w

    def to_pair_dev(self, c):
        out = DeviceArray(self.ctx, c.rows, self.pair_form())
        self.ctx.to_pair_dev(c.ptr, out.ptr, c.rows)
        self.ctx.sync()
        return out

    def from_pair_dev(self, pair, plaintexts=None):
        """pair rows -> canonical ciphertext rows; with plaintexts (limb rows / DeviceArray) the residue of x * (1 + n*m)"""
        m = None
        if plaintexts is not None:
            m = plaintexts if isinstance(plaintexts, DeviceArray) else self.upload_plain(plaintexts)
        out = DeviceArray(self.ctx, pair.rows, self.ct_limbs)
        self.ctx.from_pair_dev(pair.ptr, m.ptr if m is not None else None, out.ptr, pair.rows)
        self.ctx.sync()
        return out

    def pair_mul_dev(self, a, b):
        """row-wise product of two pair-form vectors (b with one row: that row for every a): one homomorphic addition"""
        out = DeviceArray(self.ctx, a.rows, a.cols)
        self.ctx.pair_mul_dev(a.ptr, b.ptr, b.rows == 1 and a.rows != 1, out.ptr, a.rows)
        self.ctx.sync()
        return out

    def pair_mul_scalars_dev(self, pair, mag):
        """row-wise power a[i]^mag[i] of a pair-form vector, the result in pair form: _raw_mul by non-negative scalars on resident
        rows, without the conversion in and the exit of powmod_dev"""
        exps, bits = self._mag_limbs(mag)
        e = DeviceArray.from_host(self.ctx, exps)
        out = DeviceArray(self.ctx, pair.rows, pair.cols)
        self.ctx.pair_powmod_dev(pair.ptr, e.ptr, exps.shape[1], bits, out.ptr, pair.rows)
        self.ctx.sync()
        return out

    def pair_reduce_dev(self, pair):
        """the product of all rows of a pair-form vector as one pair row (the tree of EncryptedVector.sum, one call)"""
        out = DeviceArray(self.ctx, 1, pair.cols)
        self.ctx.pair_reduce_dev(pair.ptr, pair.rows, out.ptr)
        self.ctx.sync()
        return out

    # ---- inversion on resident rows (include/phe_hip.h phe_hip_pair_invert_dev) --------------------------------------------
    def has_pair_invert(self):
        """True when inversion has its kernel on pair rows: the pair form is offered and the backend has the entry point"""
        return bool(self.pair_form()) and hasattr(self.ctx, "pair_invert_dev")

    def pair_dot_inverts(self, rows):
        """True when a dot product with signed weights over `rows` pair rows inverts them in the form (PAIR_INVERT_MIN_ROWS)"""
        return self.has_pair_invert() and rows >= PAIR_INVERT_MIN_ROWS

    def pair_invert_dev(self, store, block=None):
        """out[i] = invert(store[i], n^2) on rows in the pair form, pair rows out (phe/paillier.py:745-749 without leaving the
        form): Montgomery's trick on blocks of `block` rows (None: PAIR_INVERT_BLOCK_ROWS).  ZeroDivisionError carries the first
        row that is not a unit as bad_index."""
        out = DeviceArray(self.ctx, store.rows, store.cols)
        self.ctx.pair_invert_dev(store.ptr, out.ptr, store.rows, int(PAIR_INVERT_BLOCK_ROWS if block is None else block))
        return out

    def _inverted_where_pair(self, store, neg):
        """_inverted_where on rows in the pair form: `store` with the rows where `neg` holds replaced by their inverses, in the
        form.  Few negative rows (under a quarter): gathered, inverted as a batch of their own, scattered into a copy; otherwise
        the whole vector is inverted and selected per row.  ZeroDivisionError carries the row's index in store."""
        neg = np.asarray(neg, dtype=bool)
        count = int(neg.sum())
        words = store.cols
        if count * 4 < store.rows:
            idx = np.nonzero(neg)[0].astype(np.uint32)
            idx_d = DeviceArray.from_host(self.ctx, idx)
            sub = DeviceArray(self.ctx, count, words)
            self.ctx.gather_rows_dev(store.ptr, store.rows, idx_d.ptr, sub.ptr, words, count)
            try:
                inv = self.pair_invert_dev(sub)
            except ZeroDivisionError as e:
                if getattr(e, "bad_index", None) is not None and e.bad_index < count:
                    e.bad_index = int(idx[e.bad_index])
                raise
            base = store.copy()
            self.ctx.scatter_rows_dev(inv.ptr, idx_d.ptr, base.ptr, base.rows, words, count)
            self.ctx.sync()
            return base
        inv = self.pair_invert_dev(store)
        mask = DeviceArray.from_host(self.ctx, neg.astype(np.uint8), dtype=np.uint8)
        base = DeviceArray(self.ctx, store.rows, words)
        self.ctx.select_rows_dev(store.ptr, inv.ptr, mask.ptr, base.ptr, words, store.rows)
        self.ctx.sync()
        return base

    # ---- grouped sums on resident rows (include/phe_hip.h phe_hip_segment_reduce_dev) ------------------------------------
    def has_segment_reduce(self):
        """True when grouped sums have their kernel: the pair form is offered and the backend has the entry point"""
        return bool(self.pair_form()) and hasattr(self.ctx, "segment_reduce_dev")

    def segment_reduce_dev(self, store, is_pair, seg_ids, n_segments, want_pair=False):
        """out[f * n_segments + s] = the product of the rows i of `store` with seg_ids[f][i] == s (plan_segments): per segment the
        chain of _raw_add (phe/paillier.py:705-719) that summing its members is.  store: resident rows, pair form (is_pair) or
        canonical residues; returns a DeviceArray of canonical residues, or of pair rows (want_pair).  Every level's index arrays
        are uploaded before the first launch; the levels are queued back to back and waited for once."""
        plan = plan_segments(seg_ids, n_segments, SEGMENT_TASK_ROWS)
        if plan.n_out == 0:
            return DeviceArray(self.ctx, 0, self.pair_form() if want_pair else self.ct_limbs)
        return self.segment_launch_dev(store, is_pair, plan, self.segment_upload(plan), want_pair)

    def segment_reduce_ids_dev(self, store, is_pair, ids_dev, n_segments, node_dev=None, n_nodes=1, want_pair=False):
        """segment_reduce_dev over ids that are resident already (plan_segments_dev): nothing but the members of every output row
        comes down, nothing goes up"""
        plan = self.plan_segments_dev(ids_dev, n_segments, node_dev, n_nodes, SEGMENT_TASK_ROWS)
        if plan.n_out == 0:
            return DeviceArray(self.ctx, 0, self.pair_form() if want_pair else self.ct_limbs)
        return self.segment_launch_dev(store, is_pair, plan, plan.dev, want_pair)

    def upload_ids(self, ids):
        """integers that fit 32 bits (validated segment ids, node numbers) as resident int32: (F, rows), or (rows, 1) from (rows,)"""
        return DeviceArray.from_host(self.ctx, np.ascontiguousarray(ids, dtype=np.int32).view(np.uint32))

    def segment_upload(self, plan):
        """the index arrays of every level of a SegmentPlan as device blocks: [(task_ptr, idx or None, order), ...]"""
        return [(DeviceArray.from_host(self.ctx, task_ptr.view(np.uint32).reshape(-1, 2)),
                 DeviceArray.from_host(self.ctx, idx) if idx is not None else None,
                 DeviceArray.from_host(self.ctx, order)) for task_ptr, idx, order in plan.levels]

    # ---- the planner on the device (include/phe_hip.h phe_hip_segment_plan_sort_dev / _level_dev) --------------------------
    def has_segment_planner(self):
        """True when the backend plans grouped sums from resident ids"""
        return hasattr(self.ctx, "segment_plan_sort_dev") and hasattr(self.ctx, "segment_plan_level_dev")

    @staticmethod
    def segment_planner_fits(groupings, rows, n_out):
        """the sizes the device planner takes: 32-bit positions and keys, one key to spare for the entries left out"""
        return groupings * rows < 1 << 32 and n_out <= (1 << 32) - 2

    def plan_segments_dev(self, ids_dev, n_segments, node_dev=None, n_nodes=1, cap=None):
        """plan_segments on the device -> DeviceSegmentPlan.  ids_dev: a DeviceArray of shape (F, rows) holding int32 ids in
        [-1, n_segments); node_dev: (rows, 1) int32 in [-1, n_nodes) or None.  Output row (f * n_nodes + node[i]) * n_segments +
        ids[f][i]; an entry whose id or node is -1 belongs to none.  Every level's task_ptr, idx and order are element for
        element those of plan_segments(where((node >= 0) & (ids >= 0), node * n_segments + ids, -1), n_nodes * n_segments, cap).
        One download: the members of every output row, from which the host sizes the levels."""
        cap = int(SEGMENT_TASK_ROWS if cap is None else cap)
        if cap < 2:
            raise ValueError("a task must be allowed at least two rows")
        f, n = ids_dev.rows, ids_dev.cols
        n_out = f * int(n_nodes) * int(n_segments)
        if n_out == 0:                                       # no output rows: nothing to sort, the plan is one empty level
            plan = plan_segments(np.full((max(f, 1), n), -1, np.int64), 0, cap)
            return DeviceSegmentPlan(self.segment_upload(plan), plan.tasks, 0, 0)
        if not self.segment_planner_fits(f, n, n_out):
            raise ValueError("the device planner takes F * rows < 2^32 and at most 2^32 - 2 output rows")
        idx = DeviceArray(self.ctx, max(1, f * n), 1)
        counts_d = DeviceArray(self.ctx, n_out + 1, 1)
        self.ctx.segment_plan_sort_dev(ids_dev.ptr, node_dev.ptr if node_dev is not None else None, f, n, int(n_segments),
                                       int(n_nodes), idx.ptr, counts_d.ptr)
        host = counts_d.to_host().reshape(-1)
        counts, n_idx = host[:n_out].astype(np.int64), int(host[n_out])
        dev, tasks_of, alive = [], [], []
        while True:
            per = np.maximum(1, -(-counts // cap))
            tasks = int(per.sum())
            if tasks >= 1 << 32:
                raise ValueError("the device planner takes fewer than 2^32 tasks per level")
            per_d, tp_d, order_d = DeviceArray(self.ctx, n_out, 1), DeviceArray(self.ctx, tasks + 1, 2), DeviceArray(self.ctx, tasks, 1)
            self.ctx.segment_plan_level_dev(counts_d.ptr, n_out, cap, per_d.ptr, tp_d.ptr, order_d.ptr, tasks)
            dev.append((tp_d, idx if not dev else None, order_d))
            tasks_of.append(tasks)
            if int(per.max()) <= 1:
                self.ctx.sync()                              # (counts_d / per_d of the levels are read until here)
                return DeviceSegmentPlan(dev, tasks_of, n_out, n_idx)
            alive.append(counts_d)                           # (a level's counts stay allocated while its launches may run)
            counts, counts_d = per, per_d

    def segment_launch_dev(self, store, is_pair, plan, dev, want_pair=False):
        """the levels of a plan over `store`, queued back to back; one synchronisation.  plan: a SegmentPlan with `dev` what
        segment_upload made of it, or a DeviceSegmentPlan with its own `dev`"""
        words = self.pair_form()
        if not is_pair and plan.n_idx > store.rows > 0:
            store, is_pair = self.to_pair_dev(store), True   # several groupings read every row: into the form once, not F times
        keep = [store]                                       # operands stay alive until the final synchronisation
        rows, rows_are_pair, n_rows = store, is_pair, store.rows
        for tasks, (tp_d, idx_d, order_d) in zip(plan.tasks, dev):
            out = DeviceArray(self.ctx, tasks, words)
            self.ctx.segment_reduce_dev(rows.ptr, rows_are_pair, n_rows, tp_d.ptr, idx_d.ptr if idx_d is not None else None,
                                        order_d.ptr, out.ptr, tasks)
            keep.append(out)
            rows, rows_are_pair, n_rows = out, True, tasks
        if want_pair:
            self.ctx.sync()
            return rows
        return self.from_pair_dev(rows)                      # (synchronises)

    # ---- running sums on resident rows (include/phe_hip.h phe_hip_segment_scan_dev) --------------------------------------
    def has_segment_scan(self):
        """True when running sums have their kernel: the pair form is offered and the backend has both entry points"""
        return self.has_segment_reduce() and hasattr(self.ctx, "segment_scan_dev")

    def segment_scan_dev(self, store, is_pair, block=None, want_pair=False):
        """out[i] = the product of the rows of `store` from the start of row i's sequence of `block` rows (None: of the vector)
        up to and including i (plan_scan): every prefix of the chain of _raw_add (phe/paillier.py:705-719).  store: resident
        rows, pair form (is_pair) or canonical residues; returns a DeviceArray of canonical residues, or of pair rows
        (want_pair)."""
        if store.rows == 0:
            return DeviceArray(self.ctx, 0, self.pair_form() if want_pair else self.ct_limbs)
        plan = plan_scan(store.rows, block, SCAN_TASK_ROWS)
        return self.scan_launch_dev(store, is_pair, plan, self.scan_upload(plan), want_pair)

    def scan_upload(self, plan):
        """the index arrays of every level of a ScanPlan as device blocks: [(task_ptr, carry_idx or None), ...]"""
        return [(DeviceArray.from_host(self.ctx, task_ptr.view(np.uint32).reshape(-1, 2)),
                 DeviceArray.from_host(self.ctx, carry_idx) if carry_idx is not None else None)
                for task_ptr, carry_idx, _, _ in plan.levels]

    def scan_launch_dev(self, store, is_pair, plan, dev, want_pair=False):
        """the launches of an uploaded plan (scan_upload) over `store`, queued back to back; one synchronisation.  Down the
        levels the totals of every level's tasks (segment_reduce_dev, idx NULL, over the level's own task_ptr); the last
        level — one task per sequence — is scanned without carries; then up again, every level scanned from the carries that
        the scan of its totals is."""
        words = self.pair_form()
        if store.rows != plan.n_rows or store.cols != (words if is_pair else self.ct_limbs):
            raise ValueError("the plan was made for %d rows, the store has %d rows of %d words" % (plan.n_rows, store.rows, store.cols))
        if not is_pair and len(plan.levels) > 1:
            store, is_pair = self.to_pair_dev(store), True   # the reduce and the scan both read every row: into the form once
        keep = [store]                                       # operands stay alive until the final synchronisation
        inputs = [(store, is_pair)]
        for (task_ptr, _, n_rows, _), (tp_d, _) in zip(plan.levels[:-1], dev):
            tasks = len(task_ptr) - 1
            totals = DeviceArray(self.ctx, tasks, words)
            rows, rows_are_pair = inputs[-1]
            self.ctx.segment_reduce_dev(rows.ptr, rows_are_pair, n_rows, tp_d.ptr, None, None, totals.ptr, tasks)
            keep.append(totals)
            inputs.append((totals, True))
        carry = None
        for (task_ptr, carry_idx, n_rows, _), (tp_d, ci_d), (rows, rows_are_pair) in reversed(list(zip(plan.levels, dev, inputs))):
            out = DeviceArray(self.ctx, n_rows, words)
            self.ctx.segment_scan_dev(rows.ptr, rows_are_pair, n_rows, tp_d.ptr, carry.ptr if carry is not None else None,
                                      ci_d.ptr if (ci_d is not None and carry is not None) else None, out.ptr, len(task_ptr) - 1)
            keep.append(out)
            carry = out
        if want_pair:
            self.ctx.sync()
            return carry
        return self.from_pair_dev(carry)                     # (synchronises)

    # ---- ciphertext packing on resident rows (include/phe_hip.h phe_hip_segment_pack_dev) ------------------------------------
    def has_segment_pack(self):
        """True when packing has its kernel: the pair form is offered and the backend has the entry point"""
        return bool(self.pair_form()) and hasattr(self.ctx, "segment_pack_dev")

    def segment_pack_dev(self, store, is_pair, slots, slot_bits, want_pair=False):
        """out[t] = prod_{j < slots} store[t * slots + j] ^ (2^(slot_bits * j)) over ceil(rows / slots) output rows, rows past
        the end counting as 1: the chain c_0*1 + c_1*(1 << B) + ... of _raw_mul (phe/paillier.py:721-751) and _raw_add
        (:705-719) by Horner's rule, one launch, nothing planned on the host.  store: resident rows, pair form (is_pair) or
        canonical residues; returns a DeviceArray of canonical residues, or of pair rows (want_pair)."""
        words = self.pair_form()
        if store.rows == 0:
            return DeviceArray(self.ctx, 0, words if want_pair else self.ct_limbs)
        if store.cols != (words if is_pair else self.ct_limbs):
            raise ValueError("the store has rows of %d words" % store.cols)
        tasks = -(-store.rows // int(slots))
        out = DeviceArray(self.ctx, tasks, words)
        self.ctx.segment_pack_dev(store.ptr, is_pair, store.rows, int(slots), int(slot_bits), out.ptr, tasks)
        if want_pair:
            self.ctx.sync()
            return out
        return self.from_pair_dev(out)                       # (synchronises)

    # ---- the slot codec of packed plaintexts (include/phe_hip.h phe_hip_slots_pack_dev / phe_hip_slots_unpack_dev) ---------------
    def has_slot_codec(self):
        """True when the backend has both entries of the slot codec (slot_bits up to 64)"""
        return hasattr(self.ctx, "slots_pack_dev") and hasattr(self.ctx, "slots_unpack_dev")

    def slots_pack_dev(self, values, slots, slot_bits):
        """int64 values -> RESIDENT plaintext rows: row b = (sum_j values[b * slots + j] * 2^(slot_bits * j)) mod n, values past
        the end counting as 0.  Every value must lie in [-2^(slot_bits - 1), 2^(slot_bits - 1)): the caller checks that."""
        values = np.ascontiguousarray(values, dtype=np.int64).reshape(-1)
        slots, slot_bits = int(slots), int(slot_bits)
        rows = -(-len(values) // slots)
        out = DeviceArray(self.ctx, rows, self.n_limbs)
        if rows:
            v = DeviceArray.from_host(self.ctx, values.view(np.uint32))      # (an int64 is two words)
            self.ctx.slots_pack_dev(v.ptr, len(values), slots, slot_bits, out.ptr, rows)
            self.ctx.sync()
        return out

    def slots_unpack_dev(self, plain, slots, slot_bits):
        """resident plaintext rows -> (int64 array of rows * slots values, uint8 status per row) on the host.  Status 1: the
        plaintext lies between max_int and n - max_int, 2: the number does not fit slots * slot_bits bits; the values of such
        a row mean nothing."""
        slots, slot_bits = int(slots), int(slot_bits)
        rows = plain.rows
        values, status = np.empty(rows * slots, dtype=np.int64), np.empty(rows, dtype=np.uint8)
        if rows:
            if plain.cols != self.n_limbs:
                raise ValueError("the rows have %d words" % plain.cols)
            v, s = DeviceArray(self.ctx, rows * slots, 2), DeviceArray(self.ctx, (rows + 3) // 4, 1)
            self.ctx.slots_unpack_dev(plain.ptr, rows, slots, slot_bits, v.ptr, s.ptr)
            self.ctx.sync()
            self.ctx.d2h(values, v.ptr)
            self.ctx.d2h(status, s.ptr)
        return values, status

    def raw_decrypt_unpack_chunks(self, c, slots, slot_bits, chunk=1 << 16):
        """raw_decrypt + slot unpacking of packed rows as a generator of (lo, hi, int64 values of rows [lo, hi), status bytes):
        raw_decrypt_dev_chunks / raw_decrypt_host_chunks with the unpack kernel queued behind each chunk's decrypt on the same
        stream, so that values and status come down instead of limb rows — the plaintext rows never leave HBM.  c: a resident
        vector (DeviceArray) or host limb rows, uploaded chunk by chunk under the kernels of the chunk before.  The engine's
        lock is taken around each step, never across a yield."""
        slots, slot_bits = int(slots), int(slot_bits)
        with self._lock:
            st = self._launch_stream()
        resident = isinstance(c, DeviceArray)
        rows = c.rows if resident else c.shape[0]
        if rows == 0:
            return
        bounds = [(lo, min(rows, lo + chunk)) for lo in range(0, rows, chunk)]
        staged, running = {}, {}

        def stage(k):
            lo, hi = bounds[k]
            staged[k] = (c.rows_view(lo, hi) if resident else DeviceArray.from_host(self.ctx, c[lo:hi]),
                         DeviceArray(self.ctx, hi - lo, self.n_limbs), DeviceArray(self.ctx, (hi - lo) * slots, 2),
                         DeviceArray(self.ctx, (hi - lo + 3) // 4, 1))

        def launch(k):
            lo, hi = bounds[k]
            src, plain, vals, stat = running[k] = staged.pop(k)
            self.ctx.decrypt_dev(src.ptr, plain.ptr, hi - lo, st)
            self.ctx.slots_unpack_dev(plain.ptr, hi - lo, slots, slot_bits, vals.ptr, stat.ptr, st)
        try:
            with self._lock:
                stage(0)
                launch(0)
            for k, (lo, hi) in enumerate(bounds):
                with self._lock:
                    if k + 1 < len(bounds):
                        stage(k + 1)                             # upload under the kernels of chunk k
                    self.ctx.sync(st)                            # chunk k is complete
                    if k + 1 < len(bounds):
                        launch(k + 1)
                    _, _, vals, stat = running.pop(k)
                    values, status = np.empty((hi - lo) * slots, dtype=np.int64), np.empty(hi - lo, dtype=np.uint8)
                    self.ctx.d2h(values, vals.ptr)               # blocking copies on the NULL stream, under chunk k+1
                    self.ctx.d2h(status, stat.ptr)
                    del vals, stat
                yield lo, hi, values, status
        finally:
            # a consumer that stops early (an overflow row) drops the generator with the next chunk's kernels still writing:
            # wait for them before the blocks return to the size-keyed pool
            self.ctx.sync(st)
            running.clear()
            staged.clear()

    # ---- the value codec of plain batches (include/phe_hip.h phe_hip_values_encode_dev / phe_hip_values_decode_dev) -------------
    VALUE_KINDS = {"i": 0, "u": 1, "f": 2}                 # numpy dtype kind -> `kind` of the encode kernel (3: float + precision)

    def has_value_codec(self):
        """True when the backend has both entries of the value codec and the key leaves room for every 64-bit magnitude"""
        return (hasattr(self.ctx, "values_encode_dev") and hasattr(self.ctx, "values_decode_dev")
                and self.n_limbs >= 4 and self.max_int >= 1 << 64)

    def values_encode_dev(self, array, precision_exponent=None):
        """int64 / uint64 / float64 array -> (RESIDENT plaintext rows, exponents): row i is the encoding
        EncodedNumber.encode picks for array[i], formed on the device from the 8 bytes of the value.  The exponents come back
        as an int64 array on the host — or, with precision_exponent (float64 only: every value at that one exponent, the
        mantissa rounded half to even), as that integer.  inf / nan: ValueError.  None when a mantissa under a precision
        reaches 2^62: the caller encodes on the host."""
        array = np.ascontiguousarray(array).reshape(-1)
        if array.dtype.kind not in self.VALUE_KINDS or array.dtype.itemsize != 8:
            raise TypeError("the value codec takes int64, uint64 and float64 arrays, not %s" % array.dtype)
        kind = self.VALUE_KINDS[array.dtype.kind]
        if precision_exponent is not None:
            if kind != 2:
                raise TypeError("a precision applies to float64 arrays")
            kind = 3
        count = len(array)
        out = DeviceArray(self.ctx, count, self.n_limbs)
        if kind == 2:
            exps = np.empty(count, dtype=np.int64)
        elif kind == 3:
            exps = int(precision_exponent)
        else:
            exps = np.zeros(count, dtype=np.int64)
        if count == 0:
            return out, exps
        bits = DeviceArray.from_host(self.ctx, array.view(np.uint32))        # (a 64-bit word is two)
        stat = DeviceArray(self.ctx, (count + 3) // 4, 1)
        e_dev = DeviceArray(self.ctx, count, 1) if kind == 2 else None
        self.ctx.values_encode_dev(bits.ptr, count, kind, exps if kind == 3 else 0, out.ptr, e_dev.ptr if e_dev else None, stat.ptr)
        self.ctx.sync()
        status = np.empty(count, dtype=np.uint8)
        self.ctx.d2h(status, stat.ptr)
        if status.any():
            if (status == 1).any():
                raise ValueError("cannot encode inf / nan")
            return None
        if kind == 2:
            e32 = np.empty(count, dtype=np.int32)
            self.ctx.d2h(e32, e_dev.ptr)
            exps[:] = e32
        return out, exps

    def values_decode_dev(self, plain, kind, exps=None):
        """resident plaintext rows -> (uint64 words: int64 values for kind 0, float64 values for kind 1 — view them —, uint8
        status per row) on the host.  exps: the rows' exponents (kind 1).  Status 1: the overflow gap, 2: beyond 64 bits (or
        int64), 3: m >= n; the word of such a row means nothing."""
        rows = plain.rows
        out, status = np.empty(rows, dtype=np.uint64), np.empty(rows, dtype=np.uint8)
        if rows:
            if plain.cols != self.n_limbs:
                raise ValueError("the rows have %d words" % plain.cols)
            e_dev = DeviceArray.from_host(self.ctx, np.ascontiguousarray(exps, dtype=np.int32).view(np.uint32)) if kind == 1 else None
            if e_dev is not None and e_dev.rows != rows:
                raise ValueError("%d exponents for %d rows" % (e_dev.rows, rows))
            v, s = DeviceArray(self.ctx, rows, 2), DeviceArray(self.ctx, (rows + 3) // 4, 1)
            self.ctx.values_decode_dev(plain.ptr, rows, kind, e_dev.ptr if e_dev else None, v.ptr, s.ptr)
            self.ctx.sync()
            self.ctx.d2h(out, v.ptr)
            self.ctx.d2h(status, s.ptr)
        return out, status

    def raw_decrypt_decode_chunks(self, c, kind, exps=None, chunk=1 << 16):
        """raw_decrypt + decoding as a generator of (lo, hi, uint64 words of rows [lo, hi), status bytes, fetch): the twin of
        raw_decrypt_unpack_chunks with the decode kernel queued behind each chunk's decrypt on the same stream, so that 8 bytes
        and a status byte per row come down instead of limb rows.  kind 0: int64 words, kind 1: float64 words at the exponents
        `exps` (one per row of c, each in [-240, 0)).  fetch(indices) downloads the plaintext rows of the chunk at those indices
        (relative to lo) as host limbs — for the rows whose status says that the host must decode them; it is valid until the
        generator is advanced.  c: a resident vector (DeviceArray) or host limb rows.  The engine's lock is taken around each
        step, never across a yield."""
        with self._lock:
            st = self._launch_stream()
        resident = isinstance(c, DeviceArray)
        rows = c.rows if resident else c.shape[0]
        if rows == 0:
            return
        e32 = np.ascontiguousarray(exps, dtype=np.int32) if kind == 1 else None
        bounds = [(lo, min(rows, lo + chunk)) for lo in range(0, rows, chunk)]
        staged, running = {}, {}

        def stage(k):
            lo, hi = bounds[k]
            staged[k] = (c.rows_view(lo, hi) if resident else DeviceArray.from_host(self.ctx, c[lo:hi]),
                         DeviceArray(self.ctx, hi - lo, self.n_limbs), DeviceArray(self.ctx, hi - lo, 2),
                         DeviceArray(self.ctx, (hi - lo + 3) // 4, 1),
                         DeviceArray.from_host(self.ctx, e32[lo:hi].view(np.uint32)) if kind == 1 else None)

        def launch(k):
            lo, hi = bounds[k]
            src, plain, vals, stat, e_dev = running[k] = staged.pop(k)
            self.ctx.decrypt_dev(src.ptr, plain.ptr, hi - lo, st)
            self.ctx.values_decode_dev(plain.ptr, hi - lo, kind, e_dev.ptr if e_dev else None, vals.ptr, stat.ptr, st)
        try:
            with self._lock:
                stage(0)
                launch(0)
            for k, (lo, hi) in enumerate(bounds):
                with self._lock:
                    if k + 1 < len(bounds):
                        stage(k + 1)                             # upload under the kernels of chunk k
                    self.ctx.sync(st)                            # chunk k is complete
                    if k + 1 < len(bounds):
                        launch(k + 1)
                    _, plain, vals, stat, _ = running.pop(k)
                    values, status = np.empty(hi - lo, dtype=np.uint64), np.empty(hi - lo, dtype=np.uint8)
                    self.ctx.d2h(values, vals.ptr)               # blocking copies on the NULL stream, under chunk k+1
                    self.ctx.d2h(status, stat.ptr)
                    del vals, stat

                def fetch(indices, plain=plain):
                    with self._lock:
                        idx = DeviceArray.from_host(self.ctx, np.ascontiguousarray(indices, dtype=np.uint32))
                        sub = DeviceArray(self.ctx, idx.rows, self.n_limbs)
                        self.ctx.gather_rows_dev(plain.ptr, plain.rows, idx.ptr, sub.ptr, self.n_limbs, idx.rows)
                        self.ctx.sync()
                        return sub.to_host()
                yield lo, hi, values, status, fetch
                del fetch, plain
        finally:
            # a consumer that stops early (an overflow row) drops the generator with the next chunk's kernels still writing:
            # wait for them before the blocks return to the size-keyed pool
            self.ctx.sync(st)
            running.clear()
            staged.clear()

    def obfuscate_fresh_dev(self, c, rows=None):
        """obfuscate_dev with freshly drawn obfuscators, chunked like raw_encrypt_fresh (draw and upload of the next
        chunk under the kernels of the current one).  rows: indices that get a fresh r (None = all); the others get
        r = 1 (c * 1^n = c, still canonical)."""
        count = c.rows
        if self.short_base():
            return self.short_fresh_dev(count, mul=c, rows=rows)
        st = self._launch_stream()
        need = None
        if rows is not None:
            need = np.zeros(count, dtype=bool)
            need[rows] = True
        out = DeviceArray(self.ctx, count, self.ct_limbs)
        keep = []
        lo, chunk = 0, 1 << 15
        while lo < count:
            hi = min(count, lo + chunk)
            if need is None:
                r = random_lt_n_limbs(self.n, hi - lo, self.n_limbs, out=self.scratch("r", hi - lo, self.n_limbs))
            else:
                r = self.scratch("r", hi - lo, self.n_limbs)
                r[:] = 0
                r[:, 0] = 1
                sel = np.nonzero(need[lo:hi])[0]
                if len(sel):
                    r[sel] = random_lt_n_limbs(self.n, len(sel), self.n_limbs)
            r_d = DeviceArray.from_host(self.ctx, r)
            keep.append(r_d)
            self._obfuscate_dev(c.rows_view(lo, hi).ptr, r_d.ptr, out.rows_view(lo, hi).ptr, hi - lo, st)
            lo, chunk = hi, 1 << 16
        self.ctx.sync(st)
        return out

    # ---- short-exponent obfuscators: h_s^rho for a fixed h_s = h^n mod n^2 and short random rho (csrc/fixed_base.h) -------------
    # With h = -x^2 mod n, h_s^rho = (h^rho)^n is an n-th power like r^n, so it blinds a ciphertext the same way and decrypts the
    # same; c = (1 + n m) * h_s^rho is bit for bit raw_encrypt(m, r_value = h^rho mod n) (phe/paillier.py:102-139).  The base is
    # the same for every row: a fixed-base comb over a table kept by the native context, ceil(bits / w) pair products per row and
    # no squaring (include/phe_hip.h phe_hip_fixed_base_pow_dev).  The setting is the key's (PaillierPublicKey
    # .enable_short_obfuscators); every engine of the key is told it and builds its own table on first use.
    def short_base(self):
        """(h_s, bits) while short-exponent obfuscators are on, else None"""
        return self.__dict__.get("_short")

    def set_short_base(self, hs, bits=0):
        """draw every fresh obfuscator as hs^rho, rho uniform in [0, 2^bits), from now on (hs None: r^n again).  The table of a
        base set before is dropped; the new one is built when the kernel first needs it."""
        if self.__dict__.get("_short_table"):
            self.ctx.fixed_base_clear()
        self._short_table = False
        self._short_rows = None
        if hs is None:
            self._short = None
            return
        hs, bits = int(hs), int(bits)
        if not 1 < hs < self.nsquare:
            raise ValueError("h_s must lie in (1, n^2)")
        if not 1 <= bits <= self.n.bit_length():
            raise ValueError("bits must lie in [1, %d]" % self.n.bit_length())
        self._short = (hs, bits)

    def short_device_rng(self):
        """True while the short exponents of whole batches are ChaCha20 output under per-launch seeds (set_short_device_rng)"""
        return bool(self.__dict__.get("_short_rng"))

    def set_short_device_rng(self, on):
        """the key's device_rng setting (PaillierPublicKey.enable_short_obfuscators); nothing is built or kept for it"""
        self._short_rng = bool(on)

    def random_bits_dev(self, bits, count, limbs, st=0):
        """`count` random integers in [0, 2^bits) as resident (count, limbs) rows, queued on stream `st`: the ChaCha20 keystream
        (RFC 8439) of a fresh 32-byte seed from the kernel CSPRNG (fresh_seed), nonce 0, from block 0 on, expanded by the kernel
        of csrc/chacha_rows.h — or, on a backend without it, by the host expander (phe/_chacha.py, same words) and uploaded.
        One seed per launch, handed to the kernel in its arguments and overwritten here as soon as the launch call has returned;
        nothing is kept between calls, so a forked process, another thread and every engine of a fleet draw seeds of their own.
        A draw of more than 2^32 blocks is cut, each part under its own seed."""
        bits, limbs = int(bits), int(limbs)
        if bits < 1 or bits > 32 * limbs:
            raise ValueError("bits must lie in [1, %d]" % (32 * limbs))
        out = DeviceArray(self.ctx, count, limbs)
        kernel = hasattr(self.ctx, "chacha20_rows_dev")
        for lo, hi in _seeded_parts(count, limbs):
            part = out.rows_view(lo, hi)
            seed = fresh_seed()
            try:
                if kernel:
                    self.ctx.chacha20_rows_dev(seed, _SEED_NONCE, 0, bits, limbs, part.ptr, hi - lo, st)
                else:
                    self.ctx.h2d(part.ptr, _chacha.chacha20_rows(seed, _SEED_NONCE, 0, bits, limbs, hi - lo))
            finally:
                seed[:] = bytes(len(seed))
        return out

    def has_fixed_base(self):
        """True when h_s^rho has its kernel: a base is set, the pair form is offered and the backend has the entry points"""
        return self.short_base() is not None and bool(self.pair_form()) and hasattr(self.ctx, "fixed_base_pow_dev")

    def _short_table_ready(self):
        if not self.__dict__.get("_short_table"):
            hs, bits = self._short
            self.ctx.fixed_base_set(hs, bits, int(os.environ.get("PHE_HIP_SHORT_WINDOW", "0") or 0))
            self._short_table = True

    def short_table_info(self):
        """{"bits", "window", "positions", "table_bytes"} of the comb table (built now if it was not yet); all 0 without the
        kernel"""
        if not self.has_fixed_base():
            return {"bits": 0, "window": 0, "positions": 0, "table_bytes": 0}
        self._short_table_ready()
        return self.ctx.fixed_base_info()

    def short_table_rows_dev(self, first, count):
        """`count` rows of the comb table from row `first` on, as pair rows (entry (t, d) is row t * (2^window - 1) + d - 1)"""
        self._short_table_ready()
        out = DeviceArray(self.ctx, count, self.pair_form())
        self.ctx.fixed_base_rows_dev(first, count, out.ptr)
        self.ctx.sync()
        return out

    def _short_launch(self, e, mul, mul_is_pair, m, out, out_is_pair, st, keep):
        """queue out[i] = mul[i] * h_s^e[i] (* (1 + n*m[i])) on stream `st` (all operands resident; m only with canonical
        output): the comb kernel, or — without it — the composition of existing calls: powmod of the broadcast h_s by e, raw_add
        with mul, add_plain with m.  Same canonical residues either way.  Temporaries are appended to `keep`."""
        hs, bits = self._short
        el, rows = (bits + 31) // 32, e.rows
        if e.cols != el:
            raise ValueError("exponents of %d bits come as rows of %d words, not %d" % (bits, el, e.cols))
        if m is not None and out_is_pair:
            raise ValueError("a plaintext is folded in on the way out of the pair form only")
        if self.has_fixed_base():
            self._short_table_ready()
            self.ctx.fixed_base_pow_dev(e.ptr, el, mul.ptr if mul is not None else None, mul_is_pair,
                                        m.ptr if m is not None else None, out.ptr, out_is_pair, rows, st)
            return
        base = self.__dict__.get("_short_rows")
        if base is None or base.rows < rows:
            base = self._short_rows = DeviceArray.from_host(self.ctx, np.tile(self.cipher_limbs([hs]), (max(rows, 1 << 12), 1)))
        cur = out if not (out_is_pair or mul is not None or m is not None) else DeviceArray(self.ctx, rows, self.ct_limbs)
        self.ctx.powmod_dev(base.ptr, e.ptr, el, bits, cur.ptr, rows, st)
        keep += [base, cur]
        if mul is not None:
            if mul_is_pair:
                plain = DeviceArray(self.ctx, rows, self.ct_limbs)
                self.ctx.from_pair_dev(mul.ptr, None, plain.ptr, rows, st)
                keep.append(plain)
                mul = plain
            nxt = out if not (out_is_pair or m is not None) else DeviceArray(self.ctx, rows, self.ct_limbs)
            self.ctx.mulmod_dev(mul.ptr, cur.ptr, nxt.ptr, rows, st)
            keep.append(nxt)
            cur = nxt
        if m is not None:
            self.ctx.add_plain_dev(cur.ptr, m.ptr, out.ptr, rows, st)
        elif out_is_pair:
            self.ctx.to_pair_dev(cur.ptr, out.ptr, rows, st)

    def short_pow_dev(self, rho, mul=None, mul_is_pair=False, m=None, want_pair=False):
        """out[i] = mul[i] * h_s^rho[i] (* (1 + n*m[i])) on resident rows.  rho: (count, ceil(bits / 32)) uint32 rows, host or
        resident; mul: None (1), resident pair rows (mul_is_pair) or canonical residues; m: plaintext limb rows, host or resident
        (canonical output only).  Returns canonical residues, or pair rows (want_pair)."""
        e = rho if isinstance(rho, DeviceArray) else DeviceArray.from_host(self.ctx, rho)
        if m is not None and not isinstance(m, DeviceArray):
            m = self.upload_plain([v % self.n for v in m] if not isinstance(m, np.ndarray) else m)
        for name, other in (("mul", mul), ("m", m)):
            if other is not None and other.rows != e.rows:
                raise ValueError("%d rows of %s for %d exponents" % (other.rows, name, e.rows))
        out = DeviceArray(self.ctx, e.rows, self.pair_form() if want_pair else self.ct_limbs)
        if e.rows:
            keep = []
            self._short_launch(e, mul, mul_is_pair, m, out, want_pair, 0, keep)
            self.ctx.sync()
        return out

    def short_pow(self, rho, mul=None, m=None):
        """short_pow_dev for host rows (rho and mul: limb rows, m: limb rows or Python ints), host rows out; on a backend
        without resident rows the same composition through its host entry points"""
        rho = np.ascontiguousarray(rho, dtype=np.uint32)
        if m is not None and not isinstance(m, np.ndarray):
            m = self.plain_limbs([v % self.n for v in m])
        if hasattr(self.ctx, "powmod_dev"):
            mul_d = DeviceArray.from_host(self.ctx, mul) if mul is not None else None
            return self.short_pow_dev(rho, mul_d, False, m).to_host()
        hs, bits = self._short
        if rho.shape[0] == 0:
            return np.zeros((0, self.ct_limbs), dtype=np.uint32)
        out = self.ctx.powmod(np.tile(self.cipher_limbs([hs]), (rho.shape[0], 1)), rho)
        if mul is not None:
            out = self.ctx.mulmod(np.ascontiguousarray(mul), out)
        if m is not None:
            out = self.ctx.add_plain(out, m)
        return out

    def short_fresh_dev(self, count, mul=None, mul_is_pair=False, m=None, want_pair=False, rows=None):
        """short_pow_dev with freshly drawn exponents, in chunks like raw_encrypt_fresh: the draw (the kernel CSPRNG, host side)
        and the upload of chunk k+1 overlap the kernel of chunk k.  mul / m: resident rows or None; rows: the indices that get a
        fresh rho (None: all) — the others get rho = 0, h_s^0 = 1.  With the key's device_rng setting and rows None, every
        chunk's exponents are drawn on the device under a seed of its own (random_bits_dev): no host buffer, no upload."""
        hs, bits = self._short
        el = (bits + 31) // 32
        st = self._launch_stream()
        out = DeviceArray(self.ctx, count, self.pair_form() if want_pair else self.ct_limbs)
        need = None
        if rows is not None:
            need = np.zeros(count, dtype=bool)
            need[rows] = True
        keep = []
        lo, chunk = 0, 1 << 15
        while lo < count:
            hi = min(count, lo + chunk)
            if need is None and self.short_device_rng():
                e_d = self.random_bits_dev(bits, hi - lo, el, st)
            else:                                             # (a part of the vector: the rows that get rho = 0 are picked on the host)
                rho = random_bits_limbs(bits, hi - lo, el, out=self.scratch("rho", hi - lo, el))
                if need is not None:
                    rho[~need[lo:hi]] = 0
                e_d = DeviceArray.from_host(self.ctx, rho)    # synchronous copy: the scratch buffer is free again
            keep.append(e_d)
            self._short_launch(e_d, mul.rows_view(lo, hi) if mul is not None else None, mul_is_pair,
                               m.rows_view(lo, hi) if m is not None else None, out.rows_view(lo, hi), want_pair, st, keep)
            lo, chunk = hi, 1 << 16
        self.ctx.sync(st)
        return out

    def obfuscate_dev(self, c, r):
        r = self.upload_plain(r)
        out = DeviceArray(self.ctx, c.rows, self.ct_limbs)
        self._obfuscate_dev(c.ptr, r.ptr, out.ptr, c.rows)
        self.ctx.sync()
        return out

    def raw_decrypt_dev(self, c):
        out = DeviceArray(self.ctx, c.rows, self.n_limbs)
        self.ctx.decrypt_dev(c.ptr, out.ptr, c.rows)
        self.ctx.sync()
        return out.to_host()

    def raw_decrypt_dev_chunks(self, c, chunk=1 << 16):
        """raw_decrypt of a resident vector as a generator of (lo, hi, plaintext limbs on the host): while the caller
        works on one chunk (download + decoding), the kernels of the next one run — they are queued on the engine's
        non-blocking stream right after the finished chunk is awaited, and the blocking download does not wait for them.
        (A generator: the engine's lock is taken around each step, never across a yield — see _native.serialised.)"""
        with self._lock:
            st = self._launch_stream()
        rows = c.rows
        if rows <= chunk or not st:
            if rows:
                yield 0, rows, self.raw_decrypt_dev(c)
            return
        with self._lock:
            out = DeviceArray(self.ctx, rows, self.n_limbs)

        def launch(lo):
            hi = min(rows, lo + chunk)
            self.ctx.decrypt_dev(c.rows_view(lo, hi).ptr, out.rows_view(lo, hi).ptr, hi - lo, st)
            return hi
        try:
            with self._lock:
                lo, hi = 0, launch(0)
            while lo < rows:
                with self._lock:
                    self.ctx.sync(st)                           # chunk [lo, hi) is complete
                    nxt = launch(hi) if hi < rows else hi
                    host = out.rows_view(lo, hi).to_host()      # blocking copy on the NULL stream, under the next kernels
                yield lo, hi, host
                lo, hi = hi, nxt
        finally:
            # a consumer that stops early (e.g. OverflowError while decoding a row) drops the generator with the next
            # chunk's kernels still writing into `out`: wait for them before the block returns to the size-keyed pool
            self.ctx.sync(st)

    def raw_decrypt_host_chunks(self, c, chunk=1 << 16):
        """raw_decrypt_dev_chunks for a HOST limb array: the upload of chunk k+1 and the download + decoding of chunk k
        both happen while kernels run (uploads and downloads are blocking copies on the NULL stream, the kernels are
        queued on the engine's non-blocking stream)."""
        with self._lock:
            st = self._launch_stream()
        rows = c.shape[0]
        if rows <= chunk or not st:
            if rows:
                yield 0, rows, self.raw_decrypt(c)
            return
        bounds = [(lo, min(rows, lo + chunk)) for lo in range(0, rows, chunk)]
        inputs, outputs = {}, {}

        def stage(k):
            lo, hi = bounds[k]
            inputs[k] = DeviceArray.from_host(self.ctx, c[lo:hi])
            outputs[k] = DeviceArray(self.ctx, hi - lo, self.n_limbs)

        def launch(k):
            lo, hi = bounds[k]
            self.ctx.decrypt_dev(inputs[k].ptr, outputs[k].ptr, hi - lo, st)
        try:
            with self._lock:
                stage(0)
                launch(0)
            for k, (lo, hi) in enumerate(bounds):
                with self._lock:
                    if k + 1 < len(bounds):
                        stage(k + 1)                             # upload under the kernels of chunk k
                    self.ctx.sync(st)                            # chunk k is complete
                    if k + 1 < len(bounds):
                        launch(k + 1)
                    host = outputs.pop(k).to_host()              # download under chunk k+1
                    inputs.pop(k)
                yield lo, hi, host                               # the caller decodes under chunk k+1
        finally:
            self.ctx.sync(st)                                    # see raw_decrypt_dev_chunks: nothing in flight on release

    def raw_add_dev(self, a, b):
        out = DeviceArray(self.ctx, a.rows, self.ct_limbs)
        self.ctx.mulmod_dev(a.ptr, b.ptr, out.ptr, a.rows)
        self.ctx.sync()
        return out

    # ---- chains of additions on resident vectors: one Montgomery product per addition ("Montgomery debt") -------------
    # _raw_add is mulmod(a, b, n^2) (phe/paillier.py:705-719): on the device two Montgomery products, a*b/R and then *R^2/R.
    # A resident vector may instead hold x * R^-d mod n^2 for a vector-wide integer d (its debt): the product of two such
    # rows by ONE Montgomery product is (x_a x_b) * R^-(d_a + d_b + 1), and one product with the constant R^(d+1) mod n^2
    # gives the plain residues back when they are needed (download, decrypt, scalar multiplication, ...).  A chain of k
    # additions costs k + 1 products instead of 2k; what leaves the vector is the same canonical residue as before.
    def lazy_products(self):
        """True when the backend offers the one-product entry (include/phe_hip.h phe_hip_montmul_dev)"""
        ok = self.__dict__.get("_lazy_ok")
        if ok is None:
            ok = hasattr(self.ctx, "montmul_dev") and hasattr(self.ctx, "malloc")
            if ok:
                try:
                    self._mont_radix()
                except ValueError:                    # no full-width geometry for n^2 (keys above ~4170 bits)
                    ok = False
            self._lazy_ok = ok
        return ok

    def _mont_radix(self):
        R = self.__dict__.get("_mont_R")
        if R is None:
            R = self._mont_R = 1 << self.ctx.mont_radix_bits()
        return R

    def _mont_const_row(self, power):
        """the row R^power mod n^2 on the device (cached per power)"""
        rows = self.__dict__.setdefault("_mont_rows", {})
        row = rows.get(power)
        if row is None:
            if len(rows) > 256:
                rows.clear()
            row = rows[power] = DeviceArray.from_host(self.ctx, self.cipher_limbs([pow(self._mont_radix(), power, self.nsquare)]))
        return row

    def montmul_dev(self, a, b, stream=None):
        """row-wise a * b / R mod n^2 (canonical): the debts of the operands add up, plus one.  stream: queue the launch
        there and return without waiting (the caller synchronises that stream once, at the end of its chain; blocks freed in
        between are only reused by later launches of the SAME stream, i.e. in order); None: complete on return"""
        out = DeviceArray(self.ctx, a.rows, self.ct_limbs)
        self.ctx.montmul_dev(a.ptr, b.ptr, False, out.ptr, a.rows, stream or 0)
        if stream is None:
            self.ctx.sync()
        return out

    def scale_dev(self, a, power, stream=None):
        """row-wise a * R^power mod n^2 by one product with the constant R^(power + 1): power = d settles a debt of d,
        a negative power takes a row further into debt (to meet a partner's)"""
        const = self._mont_const_row(power + 1)                 # (uploaded with a blocking copy: complete before the launch)
        out = DeviceArray(self.ctx, a.rows, self.ct_limbs)
        self.ctx.montmul_dev(a.ptr, const.ptr, True, out.ptr, a.rows, stream or 0)
        if stream is None:
            self.ctx.sync()
        else:
            out._keep_const = const     # queued, not run yet: the constant lives as long as the result (the cache may evict it)
        return out

    def montmul_tree_dev(self, store, debt):
        """The pairwise product tree of EncryptedVector.sum over resident rows that hold x * R^-debt: ONE Montgomery product
        per node (a level turns debt d into 2d + 1; an unpaired last row is taken to the new debt by a product with a constant,
        written into the level's spare row), every level queued on the engine's launch stream, settled once at the root.
        Returns the root as a one-row DeviceArray of plain residues.  A public method: the whole tree runs under the engine's
        lock (stream creation and the constant-row cache are check-then-set)."""
        st = self._launch_stream() or None
        keep = [store]                                       # operands stay alive until the final synchronisation
        while store.rows > 1:
            half, odd = store.rows // 2, store.rows % 2
            merged = DeviceArray(self.ctx, half + odd, store.cols)
            self.ctx.montmul_dev(store.rows_view(0, half).ptr, store.rows_view(half, 2 * half).ptr, False, merged.ptr, half, st or 0)
            if odd:                                           # the row left over is taken to the new debt: * R^-(debt+1)
                const = self._mont_const_row(-(debt + 1) + 1)
                keep.append(const)                            # (the cache may evict the row while the queued kernel still reads it)
                self.ctx.montmul_dev(store.rows_view(2 * half, 2 * half + 1).ptr, const.ptr, True,
                                     merged.rows_view(half, half + 1).ptr, 1, st or 0)
            keep.append(merged)
            store, debt = merged, 2 * debt + 1
        root = self.scale_dev(store, debt, stream=st) if debt else store
        self.ctx.sync(st or 0)
        return root

    def add_plain_dev(self, c, plaintexts):
        if isinstance(plaintexts, DeviceArray):
            m = plaintexts
        else:
            m = self.upload_plain([v % self.n for v in plaintexts] if not isinstance(plaintexts, np.ndarray) else plaintexts)
        out = DeviceArray(self.ctx, c.rows, self.ct_limbs)
        self.ctx.add_plain_dev(c.ptr, m.ptr, out.ptr, c.rows)
        self.ctx.sync()
        return out

    def powmod_dev(self, base, exps):
        """exps: Python ints, or (limb rows (batch, width), largest bit length) as shifted_limbs returns them"""
        if isinstance(exps, tuple):
            limbs, bits = exps
        else:
            exps = list(exps)
            bits = max(1, max(e.bit_length() for e in exps))
            limbs = _native.ints_to_limbs(exps, (bits + 31) // 32)
        width = limbs.shape[1]
        e = DeviceArray.from_host(self.ctx, limbs)
        out = DeviceArray(self.ctx, base.rows, self.ct_limbs)
        self.ctx.powmod_dev(base.ptr, e.ptr, width, bits, out.ptr, base.rows)
        self.ctx.sync()
        return out

    def raw_mul_dev(self, c, scalars):
        """Engine.raw_mul with the ciphertexts staying in HBM: the inverse branch (phe/paillier.py:745-749) is taken
        by inverting the whole vector on the device (3 modmuls per row) and selecting per row."""
        n, threshold = self.n, self.n - self.max_int
        neg = np.fromiter((s >= threshold for s in scalars), dtype=np.uint8, count=len(scalars))
        exps = [n - s if s >= threshold else s for s in scalars]
        base = self._inverted_where(c, neg) if neg.any() else c
        return self.powmod_dev(base, exps)
