// TEST INFRASTRUCTURE — the device planner of the grouped sums (csrc/segment_plan.h) compiled for the CPU on the wave emulator
// (wave_emu.h), beside emu_chacha.cpp: tests/test_segment_plan.py builds this file into a library of its own.  The launcher
// below runs every workgroup of a launch as kWaves emulated wavefronts (one host thread each, joined by block_barrier) over an
// LDS area of its own, one workgroup after the other; the order of the launches is the header's (plan_sort, plan_level).
#include <stdint.h>

#include "wave_emu.h"
// clang-format off
#include "../../python-paillier_amd/csrc/segment_plan.h"
// clang-format on

#include <algorithm>
#include <stdexcept>
#include <string>
#include <vector>

using namespace phe::plan;

static thread_local std::string g_err;

namespace {

struct EmuLaunch {
    int strided_blocks;  // workgroups of the grid-strided launches (the GPU sizes them by its compute units)

    template <class Body>  // body(block, thread, lds): one workgroup per block
    void blocks(uint64_t n_blocks, const Body& body) {
        for (uint64_t b = 0; b < n_blocks; ++b) {
            std::vector<uint32_t> lds((size_t)kLdsWords, 0xA5A5A5A5u);
            wave::run_block(kWaves, [&](uint32_t wv, uint32_t lane) { body((uint32_t)b, wv * 64u + lane, lds.data()); });
        }
    }
    template <class Body>  // body(slot, total_slots): no LDS, no barrier
    void strided(uint64_t n, const Body& body) {
        const uint64_t waves = std::max<uint64_t>(1, std::min<uint64_t>(blocks_for(n, 64), (uint64_t)strided_blocks * kWaves));
        for (uint64_t w = 0; w < waves; ++w) wave::run_wave([&](uint32_t lane) { body(w * 64u + lane, waves * 64u); });
    }

    void keys(const KeysArgs& A) { strided(A.n, [&](uint64_t s, uint64_t t) { keys_body(A, s, t); }); }
    void count(const PassArgs& A) { blocks(A.n_blocks, [&](uint32_t b, uint32_t t, uint32_t* lds) { count_body(A, b, t, lds); }); }
    void scatter(const PassArgs& A) { blocks(A.n_blocks, [&](uint32_t b, uint32_t t, uint32_t* lds) { scatter_body(A, b, t, lds); }); }
    void scan_chunks(uint32_t* a, uint64_t n, uint32_t* sums, uint64_t chunks) {
        blocks(chunks, [&](uint32_t b, uint32_t t, uint32_t* lds) { scan_chunks_body(a, n, sums, b, t, lds); });
    }
    void scan_sums(uint32_t* sums, uint64_t m) {
        blocks(1, [&](uint32_t, uint32_t t, uint32_t* lds) { scan_sums_body(sums, m, t, lds); });
    }
    void scan_apply(uint32_t* a, uint64_t n, const uint32_t* sums) {
        strided(n, [&](uint64_t s, uint64_t t) { scan_apply_body(a, n, sums, s, t); });
    }
    void counts(const uint32_t* keys, uint64_t n, uint32_t n_out, uint32_t* out) {
        strided((uint64_t)n_out + 1, [&](uint64_t s, uint64_t t) { counts_body(keys, n, n_out, out, s, t); });
    }
    void per(const uint32_t* counts, uint64_t n_out, uint32_t cap, uint32_t* per_out, uint32_t* off, uint32_t* start) {
        strided(n_out, [&](uint64_t s, uint64_t t) { per_body(counts, n_out, cap, per_out, off, start, s, t); });
    }
    void tasks(const TasksArgs& A) { strided(A.tasks, [&](uint64_t s, uint64_t t) { tasks_body(A, s, t); }); }
};

const uint32_t kGuard = 0xC3C3C3C3u;

// scratch with a guard word behind it: the launches must stay inside what plan_*_words promises
struct Scratch {
    std::vector<uint32_t> w;
    explicit Scratch(uint64_t words) : w((size_t)words + 1, kGuard) {}
    uint32_t* data() { return w.data(); }
    void check() const {
        if (w.back() != kGuard) throw std::runtime_error("a launch wrote behind its scratch");
    }
};

// the argument checks of the C entry points (phe_hip.hip): 3 = refused
int sort_refused(const void* ids, uint64_t F, uint64_t rows, uint64_t S, uint64_t K, const void* idx_out, const void* counts_out) {
    if (!counts_out || (F && rows && (!ids || !idx_out))) return 3;
    if (K == 0 || (S == 0 && rows > 0)) return 3;
    if (F >= ((uint64_t)1 << 32) || rows >= ((uint64_t)1 << 32) || F * rows >= ((uint64_t)1 << 32)) return 3;
    if (S >= ((uint64_t)1 << 32) || K >= ((uint64_t)1 << 32) || K * S >= ((uint64_t)1 << 32)) return 3;
    if (F * (K * S) > 0xFFFFFFFEull) return 3;
    return 0;
}

}  // namespace

extern "C" {

const char* emu_plan_last_error(void) { return g_err.c_str(); }

// phe_hip_segment_plan_sort_dev: idx_out (F * rows), counts_out (F * K * S + 1, the last one the number of entries kept)
int emu_segment_plan_sort(const int32_t* ids, const int32_t* node, uint64_t F, uint64_t rows, uint64_t S, uint64_t K,
                          uint32_t* idx_out, uint32_t* counts_out, int strided_blocks) {
    try {
        if (int rc = sort_refused(ids, F, rows, S, K, idx_out, counts_out)) return rc;
        Scratch scratch(plan_sort_words(F * rows));
        EmuLaunch go{std::max(1, strided_blocks)};
        plan_sort(go, ids, node, F, rows, (uint32_t)S, (uint32_t)K, idx_out, counts_out, scratch.data());
        scratch.check();
        return 0;
    } catch (const std::exception& e) { g_err = e.what(); return 1; }
}

// phe_hip_segment_plan_level_dev
int emu_segment_plan_level(const uint32_t* counts, uint64_t n_out, uint32_t cap, uint32_t* per_out, uint64_t* task_ptr_out,
                           uint32_t* order_out, uint64_t tasks, int strided_blocks) {
    try {
        if (!counts || !per_out || !task_ptr_out || !order_out || cap < 2 || n_out == 0 || tasks < n_out ||
            tasks >= ((uint64_t)1 << 32) || n_out >= ((uint64_t)1 << 32))
            return 3;
        Scratch scratch(plan_level_words(n_out, tasks));
        EmuLaunch go{std::max(1, strided_blocks)};
        plan_level(go, counts, n_out, cap, per_out, task_ptr_out, order_out, tasks, scratch.data());
        scratch.check();
        return 0;
    } catch (const std::exception& e) { g_err = e.what(); return 1; }
}

}  // extern "C"
