// segment_core.h — grouped homomorphic sums: out[task] = the product of a RUN of ciphertext rows, in the pair form.
// Summing ciphertexts by group (gradient histograms of federated boosting, per-class aggregation, group-by) is a chain of
// EncryptedNumber.__add__ = _raw_add per group (phe/paillier.py:705-719: mulmod(a, b, n^2)); the product of residues does not
// depend on the order.  On rows in the pair form (split_core.h "resident ciphertext rows") one addition is ONE pair product, and a
// limb group that walks the rows of its segment keeps the running product in registers: one split_mul per input row (plus one
// split_conv where the rows arrive as 32-bit-word residues), nothing stored but the segment's product.
//
// One limb group owns one TASK: the run idx[first .. first + count) of row numbers (idx == nullptr: the rows first .. first + count
// themselves — the partial products of an earlier level).  The host cuts long segments into tasks of bounded length and reduces
// the partials by further levels of the same kernel (phe/_engine.py segment_reduce_dev), so that a wavefront's groups carry
// similar loads; `order` hands the tasks out longest first, as multiexp_lookup_body takes its rows.
//
// The groups of a wavefront run the loop to the wavefront's LONGEST task: split_mul and split_conv move operands between the
// lanes and through the group's LDS row in lock step, so a group that has run out of rows (or a slot past the last task) still
// executes every product of the wave — by the pair of 1 (mod.e), which leaves the value of its accumulator as it is — reads a
// valid address (row 0) where the wave converts residues, and stores nothing for a slot past the end.
#pragma once

namespace phe {

struct SegmentArgs {
    SplitConsts mod;
    const uint32_t* rows;      // rows_are_pair: (n_rows, 2H) pair rows; else (n_rows, limbs) canonical residues in 32-bit words
    int rows_are_pair;         // (the launcher picks segment_reduce_body<G, L, PAIR> by it)
    int limbs;                 // 32-bit words of a residue row
    int chunks;                // ceil(32*limbs / (29 rows))
    uint64_t n_rows;           // > 0 whenever a task has rows; every row number is clamped below it
    const uint64_t* task_ptr;  // (tasks + 1) offsets into idx (or into the rows themselves when idx == nullptr)
    const uint32_t* idx;       // row number of every entry, or nullptr
    const uint32_t* order;     // (tasks) visiting order, or nullptr
    uint32_t* out;             // (tasks, 2H) pair rows: out[t] = prod of task t's rows; the pair of 1 for an empty task
    uint64_t tasks;            // > 0
};

// PAIR: the rows are pair rows (A.rows_are_pair, which the launcher turns into this compile-time switch: the loop over pair rows
// keeps the registers of pair_mul_body, the one over residues those of split_conv beside the running product)
template <int G, int L, bool PAIR>
PHE_DEV void segment_reduce_body(const SegmentArgs& A, uint32_t* lds_row, uint32_t slot, uint32_t total_slots, uint32_t lane) {
    constexpr int H = G * L, S2 = 2 * H;
    const Lanes<G> ln(lane);
    const uint32_t g = ln.g;
    SplitLane<G, L> K;
    load_row<L>(K.n, A.mod.n, g);
    K.n0inv = A.mod.n0inv;
    K.rows_ = A.mod.rows;
    K.row_a = lds_row;
    K.row_c = lds_row + H;
    const uint64_t n_iter = (A.tasks + total_slots - 1) / total_slots;
    for (uint64_t it = 0; it < n_iter; ++it) {
        uint64_t pos = slot + it * (uint64_t)total_slots;
        const bool live = pos < A.tasks;
        if (!live) pos = A.tasks - 1;
        const uint64_t t = A.order ? (uint64_t)A.order[pos] : pos;
        const uint64_t first = A.task_ptr[t];
        const uint64_t count = (live && A.n_rows) ? A.task_ptr[t + 1] - first : 0;
        uint32_t X0[L], X1[L], Y0[L], Y1[L];
        load_row<L>(X0, wave::reread_ptr(A.mod.e), g);
        load_row<L>(X1, wave::reread_ptr(A.mod.e) + H, g);
        for (uint64_t el = 0; wave::ballot(el < count) != 0; ++el) {  // to the wavefront's longest task
            const bool mine = el < count;
            uint64_t r = 0;
            if (mine) {
                r = A.idx ? (uint64_t)A.idx[first + el] : first + el;
                r = r < A.n_rows ? r : A.n_rows - 1;
            }
            if constexpr (PAIR) {
                const uint32_t* src = mine ? A.rows + r * (uint64_t)S2 : A.mod.e;
                load_row<L>(Y0, src, g);
                load_row<L>(Y1, src + H, g);
            } else {
                split_conv<G, L>(Y0, Y1, A.rows + r * (uint64_t)A.limbs, A.limbs, A.chunks, A.mod, K, ln);
                if (!mine) {
                    load_row<L>(Y0, wave::reread_ptr(A.mod.e), g);
                    load_row<L>(Y1, wave::reread_ptr(A.mod.e) + H, g);
                }
            }
            split_mul<G, L>(X0, X1, Y0, Y1, K, ln);
        }
        if (live) {
            store_row<L>(A.out + t * (uint64_t)S2, X0, g);
            store_row<L>(A.out + t * (uint64_t)S2 + H, X1, g);
        }
    }
}

// ---- running sums: out[row] = the product of the rows of its task up to and including `row`, times the task's carry ------------
// A cumulative sum of ciphertexts (EncryptedVector.cumsum) is the same chain of _raw_add with every prefix kept: the walk of
// segment_reduce_body that STORES AFTER EVERY PRODUCT and STARTS FROM A CARRY.  Task t owns the consecutive rows
// task_ptr[t] .. task_ptr[t + 1] (the host cuts every sequence into tasks of near-equal length: no idx, no order); its carry —
// the product of everything before the task in its sequence — was made by an earlier launch (phe/_engine.py plan_scan: the
// tasks' totals by segment_reduce_body, scanned in turn).  Nothing passes between workgroups inside the kernel.
struct ScanArgs {
    SplitConsts mod;
    const uint32_t* rows;       // rows_are_pair: (n_rows, 2H) pair rows; else (n_rows, limbs) canonical residues in 32-bit words
    int rows_are_pair;          // (the launcher picks segment_scan_body<G, L, PAIR> by it)
    int limbs;                  // 32-bit words of a residue row
    int chunks;                 // ceil(32*limbs / (29 rows))
    uint64_t n_rows;            // rows of `rows` and of `out`: a row number at or above it is neither read nor stored
    const uint64_t* task_ptr;   // (tasks + 1) offsets: task t owns the rows task_ptr[t] .. task_ptr[t + 1]
    const uint32_t* carry;      // (tasks, 2H) pair rows, or nullptr
    const uint32_t* carry_idx;  // (tasks) row of `carry` a task starts from (< tasks), 0xFFFFFFFF: from 1; or nullptr
    uint32_t* out;              // (n_rows, 2H) pair rows; a row that no task owns is left as it is
    uint64_t tasks;             // > 0
};

constexpr uint32_t kScanNoCarry = 0xFFFFFFFFu;

// The lock-step rules are those of segment_reduce_body: to the wavefront's longest task, a group that has run out multiplying
// by the pair of 1 from a valid address and storing nothing.
template <int G, int L, bool PAIR>
PHE_DEV void segment_scan_body(const ScanArgs& A, uint32_t* lds_row, uint32_t slot, uint32_t total_slots, uint32_t lane) {
    constexpr int H = G * L, S2 = 2 * H;
    const Lanes<G> ln(lane);
    const uint32_t g = ln.g;
    SplitLane<G, L> K;
    load_row<L>(K.n, A.mod.n, g);
    K.n0inv = A.mod.n0inv;
    K.rows_ = A.mod.rows;
    K.row_a = lds_row;
    K.row_c = lds_row + H;
    const uint64_t n_iter = (A.tasks + total_slots - 1) / total_slots;
    for (uint64_t it = 0; it < n_iter; ++it) {
        uint64_t t = slot + it * (uint64_t)total_slots;
        const bool live = t < A.tasks;
        if (!live) t = A.tasks - 1;
        const uint64_t first = A.task_ptr[t];
        const uint64_t last = A.task_ptr[t + 1] < A.n_rows ? A.task_ptr[t + 1] : A.n_rows;
        const uint64_t count = (live && first < last) ? last - first : 0;
        const uint32_t* start = wave::reread_ptr(A.mod.e);
        if (live && A.carry && A.carry_idx) {
            const uint32_t c = A.carry_idx[t];
            if (c != kScanNoCarry) start = A.carry + (c < A.tasks ? (uint64_t)c : A.tasks - 1) * (uint64_t)S2;
        }
        uint32_t X0[L], X1[L], Y0[L], Y1[L];
        load_row<L>(X0, start, g);
        load_row<L>(X1, start + H, g);
        for (uint64_t el = 0; wave::ballot(el < count) != 0; ++el) {  // to the wavefront's longest task
            const bool mine = el < count;
            const uint64_t r = mine ? first + el : 0;                // (< n_rows: count stops at it)
            if constexpr (PAIR) {
                const uint32_t* src = mine ? A.rows + r * (uint64_t)S2 : A.mod.e;
                load_row<L>(Y0, src, g);
                load_row<L>(Y1, src + H, g);
            } else {
                split_conv<G, L>(Y0, Y1, A.rows + r * (uint64_t)A.limbs, A.limbs, A.chunks, A.mod, K, ln);
                if (!mine) {
                    load_row<L>(Y0, wave::reread_ptr(A.mod.e), g);
                    load_row<L>(Y1, wave::reread_ptr(A.mod.e) + H, g);
                }
            }
            split_mul<G, L>(X0, X1, Y0, Y1, K, ln);
            if (mine) {
                store_row<L>(A.out + r * (uint64_t)S2, X0, g);
                store_row<L>(A.out + r * (uint64_t)S2 + H, X1, g);
            }
        }
    }
}

// ---- packing: out[t] = prod_{j < slots} rows[t*slots + j] ^ (2^(slot_bits*j)) — many small plaintexts in one ciphertext ------
// E(x_0) * E(x_1)^(2^B) * E(x_2)^(2^(2B)) * ... encrypts x_0 + x_1 2^B + x_2 2^(2B) + ... (EncryptedVector.pack): with the
// reference the chain c_0*1 + c_1*(1 << B) + ..., every term EncryptedNumber.__mul__ -> _raw_mul (phe/paillier.py:721-751,
// powmod(c, 2^(B j), n^2)), joined by __add__ -> _raw_add (:705-719).  Horner's rule from the top slot down,
// acc <- acc^(2^B) * c_j, shares the squarings between the slots: B squarings and one product per input row, the accumulator
// in registers as in the two walks above.  Task t owns the CONSECUTIVE rows t*slots .. t*slots + slots; a row at or past
// n_rows (the ragged last task) contributes the ciphertext 1.
// Lock step: the trip counts slots and slot_bits are kernel arguments, the same in every group of every wavefront, so the loops
// need no ballot; a slot past the last task and a row past the end still execute every squaring and product of the wave — the
// product by the pair of 1 (mod.e), read from a valid address (row 0 where the wave converts residues) — and a slot past the
// last task stores nothing.
struct PackArgs {
    SplitConsts mod;
    const uint32_t* rows;  // rows_are_pair: (n_rows, 2H) pair rows; else (n_rows, limbs) canonical residues in 32-bit words
    int rows_are_pair;     // (the launcher picks segment_pack_body<G, L, PAIR> by it)
    int limbs;             // 32-bit words of a residue row
    int chunks;            // ceil(32*limbs / (29 rows))
    uint64_t n_rows;       // > 0; a row number at or above it is not read
    uint32_t slots;        // > 0: input rows per output row
    uint32_t slot_bits;    // > 0: squarings between two slots
    uint32_t* out;         // (tasks, 2H) pair rows
    uint64_t tasks;        // > 0, = ceil(n_rows / slots), at most 2^32
};

template <int G, int L, bool PAIR>
PHE_DEV void segment_pack_body(const PackArgs& A, uint32_t* lds_row, uint32_t slot, uint32_t total_slots, uint32_t lane) {
    constexpr int H = G * L, S2 = 2 * H;
    const Lanes<G> ln(lane);
    const uint32_t g = ln.g;
    SplitLane<G, L> K;
    load_row<L>(K.n, A.mod.n, g);
    K.n0inv = A.mod.n0inv;
    K.rows_ = A.mod.rows;
    K.row_a = lds_row;
    K.row_c = lds_row + H;
    const uint64_t n_iter = (A.tasks + total_slots - 1) / total_slots;
    for (uint64_t it = 0; it < n_iter; ++it) {
        // (every per-lane index in ONE register across the squarings: tasks <= 2^32, and `base`, `left` are wave-uniform)
        const uint64_t base = it * (uint64_t)total_slots, left = A.tasks - base;
        const bool live = left > 0xFFFFFFFFull || slot < (uint32_t)left;
        const uint32_t t = live ? (uint32_t)base + slot : 0u;  // (task 0 is always there)
        uint32_t X0[L], X1[L], Y0[L], Y1[L];
        load_row<L>(X0, wave::reread_ptr(A.mod.e), g);
        load_row<L>(X1, wave::reread_ptr(A.mod.e) + H, g);
        for (uint32_t el = A.slots; el-- > 0;) {  // from the top slot down
            if (el + 1 != A.slots)
                for (uint32_t s = 0; s < A.slot_bits; ++s) split_square<G, L>(X0, X1, K, ln);
            uint64_t r = (uint64_t)t * A.slots + el;
            const bool mine = live && r < A.n_rows;
            if (!mine) r = 0;
            if constexpr (PAIR) {
                // (the row's address and the lane position are re-read here: left to itself the compiler loads the row before
                //  the squarings, keeps it alive across them and spills other values for it)
                const uint32_t* src = wave::reread_vptr(mine ? A.rows + r * (uint64_t)S2 : A.mod.e);
                const uint32_t gi = wave::reread(g);
                load_row<L>(Y0, src, gi);
                load_row<L>(Y1, src + H, gi);
            } else {
                split_conv<G, L>(Y0, Y1, A.rows + r * (uint64_t)A.limbs, A.limbs, A.chunks, A.mod, K, ln);
                if (!mine) {
                    load_row<L>(Y0, wave::reread_ptr(A.mod.e), g);
                    load_row<L>(Y1, wave::reread_ptr(A.mod.e) + H, g);
                }
            }
            split_mul<G, L>(X0, X1, Y0, Y1, K, ln);
        }
        if (live) {
            uint32_t* dst = A.out + (uint64_t)wave::reread(t) * S2;
            store_row<L>(dst, X0, g);
            store_row<L>(dst + H, X1, g);
        }
    }
}

}  // namespace phe
