// segment_plan.h — the planner of the grouped sums on the device: from resident segment ids to the index arrays that
// segment_core.h segment_reduce_body reads (task_ptr, idx, order of every level), element for element what the numpy planner
// phe/_engine.py plan_segments returns for the same ids.  The host planner is a stable argsort over F * rows keys, a bincount and,
// per level, a repeat, a cumsum and a second argsort; here all of it is a least-significant-digit radix sort of (key, row)
// pairs, binary searches in the sorted keys and two prefix sums.
//
// Keys.  Entry (f, i) of ids (F, rows) has the key f*S + ids[f][i], or, with a node array, (f*K + node[i])*S + ids[f][i]; an
// entry whose id or node is negative is dropped: it gets the key n_out = F*K*S, sorts behind every output row, and idx is cut at
// the first such key.  The value of an entry is its row number i.
//
// One pass of the sort (8-bit digits, ceil(bits(largest key) / 8) passes) is three steps:
//   count    a workgroup of kWaves wavefronts owns a tile of kTile consecutive pairs and writes how many of them carry each of
//            the 256 digits into hist[digit][block];
//   scan     one exclusive prefix sum over hist in (digit, block) order: where the block's pairs of a digit go;
//   scatter  the workgroup ranks every pair among the pairs of its tile with the same digit and stores it at base + rank.
// The rank is exact and in tile order, which makes the sort stable and its result a function of the input alone — no atomic
// anywhere: a lane's match mask (the lanes of its wavefront with the same digit) is the AND of one ballot per digit bit, its rank
// among them the popcount below the lane; the lowest lane of a match group adds the group's size to the wavefront's own row of
// digit counts in LDS (ordinary loads and stores: one writer per word), and after a workgroup barrier thread d turns column d of
// the kWaves rows into bases.  A tile is laid out wavefront-major, then item, then lane, and ranked in that order.
//
// The prefix sums (hist, and the task offsets below) run in place on 32-bit words: every workgroup scans a chunk of kScanChunk
// words and leaves its total in sums[], one workgroup scans sums[], and a third launch adds sums[chunk] to the chunks behind the
// first.  Every total here is bounded by the number of pairs (< 2^32) or of tasks (< 2^32, checked by the caller).
//
// counts[k], the members of output row k, is lower_bound(k + 1) - lower_bound(k) in the sorted keys, one thread per row, and
// counts[n_out] = lower_bound(n_out) is the number of entries kept.  A level of tasks follows from the counts of the level
// before: per[k] = max(1, ceil(counts[k] / cap)) tasks for row k, task t of row k starts at start[k] + (t * counts[k]) / per[k]
// (start, and the task offsets, are exclusive prefix sums of counts and per); one thread per task finds its row by a binary search
// in the offsets.  order, the tasks longest first and stable, is one more sort of the same kind: of the task numbers by the key
// cap - length.  The next level's counts are this level's per.
//
// The bodies are written against wave:: (wave_gfx950.h on the device, tests/emu/wave_emu.h on the host: tests/emu/emu_plan.cpp),
// and the order of the launches (plan_sort, plan_level) is a template over the launcher, so the emulator runs the same sequence.
#pragma once

namespace phe {
namespace plan {

constexpr int kWaves = 4;                          // wavefronts of a workgroup
constexpr int kThreads = 64 * kWaves;
constexpr int kItems = 8;                          // pairs of a lane in a tile
constexpr uint32_t kTile = kThreads * kItems;      // pairs of a workgroup in one pass
constexpr int kDigits = 256;
constexpr int kScanItems = 8;                      // consecutive words of a thread in a scanned chunk
constexpr uint32_t kScanChunk = kThreads * kScanItems;
constexpr int kLdsWords = kWaves * kDigits;        // the digit counts of every wavefront (the scans use 2 * kThreads of them)
static_assert(kThreads == kDigits, "thread d of a workgroup owns digit d");
static_assert(2 * kThreads <= kLdsWords, "the scan's two buffers share the area of the digit counts");

struct KeysArgs {
    const int32_t* ids;   // (F, rows) in [-1, S)
    const int32_t* node;  // (rows,) in [-1, K), or null (K == 1)
    uint64_t n;           // F * rows < 2^32
    uint32_t rows, S, K;
    uint32_t n_out;       // F * K * S <= 2^32 - 2: the key of a dropped entry
    uint32_t* keys;       // (n)
};

struct PassArgs {
    const uint32_t* keys_in;
    const uint32_t* vals_in;  // null: the value of pair e is e % rows_mod (rows_mod == 0: e itself)
    uint32_t* keys_out;
    uint32_t* vals_out;
    uint32_t* hist;           // (kDigits, n_blocks): counts after count_body, bases after the scan
    uint64_t n;               // pairs, < 2^32
    uint32_t n_blocks;        // ceil(n / kTile)
    uint32_t rows_mod;
    int shift;                // 8 * pass
};

struct TasksArgs {
    const uint32_t* counts;  // (n_out) members of every row at this level
    const uint32_t* per;     // (n_out) tasks of every row
    const uint32_t* off;     // (n_out) exclusive prefix sum of per
    const uint32_t* start;   // (n_out) exclusive prefix sum of counts
    uint64_t n_out;
    uint64_t tasks;          // the sum of per, < 2^32
    uint32_t cap;
    uint64_t* task_ptr;      // (tasks + 1)
    uint32_t* keys;          // (tasks) cap - length of the task
};

// ---- keys ----------------------------------------------------------------------------------------------------------------------
PHE_DEV void keys_body(const KeysArgs& A, uint64_t slot, uint64_t total_slots) {
    for (uint64_t e = slot; e < A.n; e += total_slots) {
        const uint32_t f = (uint32_t)(e / A.rows), i = (uint32_t)(e - (uint64_t)f * A.rows);
        const uint32_t id = (uint32_t)A.ids[e];
        const uint32_t nd = A.node ? (uint32_t)A.node[i] : 0u;
        const bool keep = id < A.S && nd < A.K;  // (a negative one is above either bound as an unsigned number)
        A.keys[e] = keep ? (uint32_t)(((uint64_t)f * A.K + nd) * A.S + id) : A.n_out;
    }
}

// ---- one tile of a pass: digits, and ranks among the pairs of the tile's earlier items of this wavefront ------------------------
// wcount: kWaves rows of kDigits words in LDS.  After the call row wv holds the wavefront's digit counts, key[k] the key of the
// lane's item k and rank[k] the number of pairs with the same digit in the wavefront's items before it and in the lanes below it.
// Every lane of the wavefront makes every ballot: a lane past the end of the array takes part with valid == false.
PHE_DEV void tile_digits(const PassArgs& A, uint32_t block, uint32_t wv, uint32_t lane, uint32_t* wcount, uint32_t (&key)[kItems],
                         uint32_t (&rank)[kItems]) {
    uint32_t* mine = wcount + wv * kDigits;
#pragma unroll
    for (int j = 0; j < kDigits / 64; ++j) mine[lane + 64 * j] = 0u;
    wave::lds_fence();
    const uint64_t base = (uint64_t)block * kTile + (uint64_t)wv * (64 * kItems);
    const uint64_t below_me = ((uint64_t)1 << lane) - 1;
#pragma unroll
    for (int k = 0; k < kItems; ++k) {
        const uint64_t e = base + (uint64_t)k * 64 + lane;
        const bool valid = e < A.n;
        const uint32_t kk = valid ? A.keys_in[e] : 0u;
        const uint32_t d = (kk >> A.shift) & (kDigits - 1);
        uint64_t match = wave::ballot(valid);
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const bool bit = (d >> b) & 1u;
            const uint64_t m = wave::ballot(bit);
            match &= bit ? m : ~m;
        }
        const uint32_t below = (uint32_t)__builtin_popcountll(match & below_me);
        PHE_BOUNDS(d < (uint32_t)kDigits);
        const uint32_t prior = valid ? mine[d] : 0u;
        wave::lds_fence();  // every lane of the match group has read the count before its lowest lane replaces it
        if (valid && below == 0u) mine[d] = prior + (uint32_t)__builtin_popcountll(match);
        wave::lds_fence();
        key[k] = kk;
        rank[k] = prior + below;
    }
}

PHE_DEV void count_body(const PassArgs& A, uint32_t block, uint32_t t, uint32_t* lds) {
    uint32_t key[kItems], rank[kItems];
    tile_digits(A, block, t >> 6, t & 63u, lds, key, rank);
    wave::block_barrier();
    uint32_t sum = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) sum += lds[w * kDigits + t];
    A.hist[(uint64_t)t * A.n_blocks + block] = sum;
}

PHE_DEV void scatter_body(const PassArgs& A, uint32_t block, uint32_t t, uint32_t* lds) {
    const uint32_t wv = t >> 6, lane = t & 63u;
    uint32_t key[kItems], rank[kItems];
    tile_digits(A, block, wv, lane, lds, key, rank);
    wave::block_barrier();
    uint32_t run = A.hist[(uint64_t)t * A.n_blocks + block];  // where the tile's pairs of digit t begin
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
        const uint32_t c = lds[w * kDigits + t];
        lds[w * kDigits + t] = run;
        run += c;
    }
    wave::block_barrier();
    const uint64_t base = (uint64_t)block * kTile + (uint64_t)wv * (64 * kItems);
#pragma unroll
    for (int k = 0; k < kItems; ++k) {
        const uint64_t e = base + (uint64_t)k * 64 + lane;
        if (e < A.n) {
            const uint32_t d = (key[k] >> A.shift) & (kDigits - 1);
            const uint64_t pos = (uint64_t)lds[wv * kDigits + d] + rank[k];
            const uint32_t v = A.vals_in ? A.vals_in[e] : (uint32_t)(A.rows_mod ? e % A.rows_mod : e);
            if (pos < A.n) {  // (always, by the counts: nothing is ever stored outside the arrays)
                A.keys_out[pos] = key[k];
                A.vals_out[pos] = v;
            }
        }
    }
}

// ---- prefix sums ---------------------------------------------------------------------------------------------------------------
// exclusive prefix sum of one word per thread over the workgroup, in 2 * kThreads words of LDS; total: the sum of all
PHE_DEV uint32_t block_exclusive(uint32_t x, uint32_t t, uint32_t* lds, uint32_t& total) {
    wave::block_barrier();  // (the call before may still be reading the area)
    lds[t] = x;
    wave::block_barrier();
    int cur = 0;
    for (int off = 1; off < kThreads; off <<= 1) {
        uint32_t v = lds[cur * kThreads + t];
        if (t >= (uint32_t)off) v += lds[cur * kThreads + t - off];
        lds[(cur ^ 1) * kThreads + t] = v;
        wave::block_barrier();
        cur ^= 1;
    }
    total = lds[cur * kThreads + kThreads - 1];
    return lds[cur * kThreads + t] - x;
}

// chunk `block` of a (n words) scanned in place, its total to sums[block]
PHE_DEV void scan_chunks_body(uint32_t* a, uint64_t n, uint32_t* sums, uint32_t block, uint32_t t, uint32_t* lds) {
    const uint64_t first = (uint64_t)block * kScanChunk + (uint64_t)t * kScanItems;
    uint32_t v[kScanItems], sum = 0;
#pragma unroll
    for (int j = 0; j < kScanItems; ++j) {
        v[j] = first + j < n ? a[first + j] : 0u;
        sum += v[j];
    }
    uint32_t total;
    uint32_t run = block_exclusive(sum, t, lds, total);
#pragma unroll
    for (int j = 0; j < kScanItems; ++j) {
        if (first + j < n) a[first + j] = run;
        run += v[j];
    }
    if (t == 0) sums[block] = total;
}

// sums (m words) scanned in place by ONE workgroup
PHE_DEV void scan_sums_body(uint32_t* sums, uint64_t m, uint32_t t, uint32_t* lds) {
    uint32_t carry = 0;
    for (uint64_t first = 0; first < m; first += kThreads) {
        const bool in = first + t < m;
        const uint32_t x = in ? sums[first + t] : 0u;
        uint32_t total;
        const uint32_t ex = block_exclusive(x, t, lds, total);
        if (in) sums[first + t] = carry + ex;
        carry += total;
    }
}

PHE_DEV void scan_apply_body(uint32_t* a, uint64_t n, const uint32_t* sums, uint64_t slot, uint64_t total_slots) {
    for (uint64_t i = kScanChunk + slot; i < n; i += total_slots) a[i] += sums[i / kScanChunk];
}

// ---- counts, tasks -------------------------------------------------------------------------------------------------------------
// the first position of sorted keys (n of them) whose key is not below x
PHE_DEV uint64_t lower_bound(const uint32_t* keys, uint64_t n, uint32_t x) {
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (keys[mid] < x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// counts (n_out + 1): the members of every output row, then the number of entries kept
PHE_DEV void counts_body(const uint32_t* keys, uint64_t n, uint32_t n_out, uint32_t* counts, uint64_t slot, uint64_t total_slots) {
    for (uint64_t k = slot; k <= n_out; k += total_slots) {
        const uint64_t lo = lower_bound(keys, n, (uint32_t)k);
        counts[k] = (uint32_t)(k < n_out ? lower_bound(keys, n, (uint32_t)k + 1u) - lo : lo);
    }
}

PHE_DEV void per_body(const uint32_t* counts, uint64_t n_out, uint32_t cap, uint32_t* per, uint32_t* off, uint32_t* start,
                      uint64_t slot, uint64_t total_slots) {
    for (uint64_t k = slot; k < n_out; k += total_slots) {
        const uint32_t c = counts[k];
        const uint32_t p = c ? (uint32_t)(((uint64_t)c + cap - 1) / cap) : 1u;  // (an empty row: one empty task)
        per[k] = p;
        off[k] = p;
        start[k] = c;
    }
}

PHE_DEV void tasks_body(const TasksArgs& A, uint64_t slot, uint64_t total_slots) {
    for (uint64_t t = slot; t < A.tasks; t += total_slots) {
        uint64_t lo = 0, hi = A.n_out;  // the last row whose offset is not above t (per >= 1: the offsets rise strictly)
        while (hi - lo > 1) {
            const uint64_t mid = lo + (hi - lo) / 2;
            if (A.off[mid] <= t) lo = mid;
            else hi = mid;
        }
        const uint64_t tt = t - A.off[lo], c = A.counts[lo], p = A.per[lo];
        const uint64_t s0 = A.start[lo] + (tt * c) / p, s1 = A.start[lo] + ((tt + 1) * c) / p;
        A.task_ptr[t] = s0;
        if (t + 1 == A.tasks) A.task_ptr[A.tasks] = s1;  // (tasks are contiguous: each ends where the next starts)
        A.keys[t] = A.cap - (uint32_t)(s1 - s0);
    }
}

// ---- the order of the launches (host) ------------------------------------------------------------------------------------------
inline int digit_passes(uint64_t largest_key) {
    int bits = 0;
    for (; largest_key; largest_key >>= 1) ++bits;
    return (bits + 7) / 8;
}
inline uint64_t blocks_for(uint64_t n, uint64_t per_block) { return (n + per_block - 1) / per_block; }
inline uint64_t hist_words(uint64_t n) { return (uint64_t)kDigits * blocks_for(n, kTile); }
inline uint64_t sums_words(uint64_t n) { return blocks_for(n, kScanChunk) + 1; }

struct SortBuffers {
    uint32_t* keys[2];
    uint32_t* vals[2];
    uint32_t* hist;
    uint32_t* sums;
};
inline uint64_t sort_words(uint64_t n) { return 4 * n + hist_words(n) + sums_words(hist_words(n)); }
inline SortBuffers carve_sort(uint32_t* p, uint64_t n) {
    SortBuffers B;
    B.keys[0] = p;
    B.keys[1] = p + n;
    B.vals[0] = p + 2 * n;
    B.vals[1] = p + 3 * n;
    B.hist = p + 4 * n;
    B.sums = B.hist + hist_words(n);
    return B;
}
// words of scratch of plan_sort over n = F * rows entries, and of plan_level over n_out rows and `tasks` tasks
inline uint64_t plan_sort_words(uint64_t n) { return sort_words(n); }
inline uint64_t plan_level_words(uint64_t n_out, uint64_t tasks) { return 2 * n_out + sums_words(n_out) + sort_words(tasks); }

template <class Launch>
void exclusive_scan(Launch& go, uint32_t* a, uint64_t n, uint32_t* sums) {
    const uint64_t chunks = blocks_for(n, kScanChunk);
    if (chunks == 0) return;
    go.scan_chunks(a, n, sums, chunks);
    if (chunks > 1) {
        go.scan_sums(sums, chunks);
        go.scan_apply(a, n, sums);
    }
}

// n pairs (B.keys[0], implicit or B.vals) sorted by `passes` digits; the values of the last pass go to vals_final.
// Returns which of B.keys holds the sorted keys.
template <class Launch>
int radix_sort(Launch& go, const SortBuffers& B, uint64_t n, int passes, uint32_t rows_mod, uint32_t* vals_final) {
    int src = 0;
    const uint32_t* vals_in = nullptr;
    for (int p = 0; p < passes; ++p) {
        PassArgs A;
        A.keys_in = B.keys[src];
        A.vals_in = vals_in;
        A.keys_out = B.keys[src ^ 1];
        A.vals_out = p == passes - 1 ? vals_final : B.vals[p & 1];
        A.hist = B.hist;
        A.n = n;
        A.n_blocks = (uint32_t)blocks_for(n, kTile);
        A.rows_mod = rows_mod;
        A.shift = 8 * p;
        go.count(A);
        exclusive_scan(go, B.hist, hist_words(n), B.sums);
        go.scatter(A);
        vals_in = A.vals_out;
        src ^= 1;
    }
    return src;
}

// idx_out (F * rows words; the first counts_out[n_out] are the plan's idx) and counts_out (n_out + 1) from resident ids
template <class Launch>
void plan_sort(Launch& go, const int32_t* ids, const int32_t* node, uint64_t F, uint64_t rows, uint32_t S, uint32_t K,
               uint32_t* idx_out, uint32_t* counts_out, uint32_t* scratch) {
    const uint64_t n = F * rows;
    const uint32_t n_out = (uint32_t)(F * K * S);
    const SortBuffers B = carve_sort(scratch, n);
    int src = 0;
    if (n) {
        KeysArgs A;
        A.ids = ids;
        A.node = node;
        A.n = n;
        A.rows = (uint32_t)rows;
        A.S = S;
        A.K = K;
        A.n_out = n_out;
        A.keys = B.keys[0];
        go.keys(A);
        src = radix_sort(go, B, n, digit_passes(n_out), (uint32_t)rows, idx_out);
    }
    go.counts(B.keys[src], n, n_out, counts_out);
}

// one level: per_out (the next level's counts), task_ptr_out (tasks + 1) and order_out (tasks) from the level's counts
template <class Launch>
void plan_level(Launch& go, const uint32_t* counts, uint64_t n_out, uint32_t cap, uint32_t* per_out, uint64_t* task_ptr_out,
                uint32_t* order_out, uint64_t tasks, uint32_t* scratch) {
    uint32_t* off = scratch;
    uint32_t* start = off + n_out;
    uint32_t* sums = start + n_out;
    const SortBuffers B = carve_sort(sums + sums_words(n_out), tasks);
    go.per(counts, n_out, cap, per_out, off, start);
    exclusive_scan(go, off, n_out, sums);
    exclusive_scan(go, start, n_out, sums);
    TasksArgs A;
    A.counts = counts;
    A.per = per_out;
    A.off = off;
    A.start = start;
    A.n_out = n_out;
    A.tasks = tasks;
    A.cap = cap;
    A.task_ptr = task_ptr_out;
    A.keys = B.keys[0];
    go.tasks(A);
    radix_sort(go, B, tasks, digit_passes(cap), 0u, order_out);
}

}  // namespace plan
}  // namespace phe
