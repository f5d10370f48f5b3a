// kernels_plan.hip — the kernels of the device planner of the grouped sums (segment_plan.h): keys from resident ids, the three
// steps of a radix pass, the chunked prefix sums, counts by binary search and the tasks of a level.  No multiply-adds; the tile
// kernels hold kItems (key, rank) pairs of a lane in registers and kLdsWords words of LDS per workgroup.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

// clang-format off
#include "wave_gfx950.h"
#include "segment_plan.h"
// clang-format on

namespace phe {
namespace plan {

__global__ void __launch_bounds__(kThreads) k_plan_keys(KeysArgs A) {
    keys_body(A, (uint64_t)blockIdx.x * kThreads + threadIdx.x, (uint64_t)gridDim.x * kThreads);
}
__global__ void __launch_bounds__(kThreads) k_plan_count(PassArgs A) {
    __shared__ uint32_t lds[kLdsWords];
    count_body(A, blockIdx.x, threadIdx.x, lds);
}
__global__ void __launch_bounds__(kThreads) k_plan_scatter(PassArgs A) {
    __shared__ uint32_t lds[kLdsWords];
    scatter_body(A, blockIdx.x, threadIdx.x, lds);
}
__global__ void __launch_bounds__(kThreads) k_plan_scan_chunks(uint32_t* a, uint64_t n, uint32_t* sums) {
    __shared__ uint32_t lds[2 * kThreads];
    scan_chunks_body(a, n, sums, blockIdx.x, threadIdx.x, lds);
}
__global__ void __launch_bounds__(kThreads) k_plan_scan_sums(uint32_t* sums, uint64_t m) {
    __shared__ uint32_t lds[2 * kThreads];
    scan_sums_body(sums, m, threadIdx.x, lds);
}
__global__ void __launch_bounds__(kThreads) k_plan_scan_apply(uint32_t* a, uint64_t n, const uint32_t* sums) {
    scan_apply_body(a, n, sums, (uint64_t)blockIdx.x * kThreads + threadIdx.x, (uint64_t)gridDim.x * kThreads);
}
__global__ void __launch_bounds__(kThreads) k_plan_counts(const uint32_t* keys, uint64_t n, uint32_t n_out, uint32_t* counts) {
    counts_body(keys, n, n_out, counts, (uint64_t)blockIdx.x * kThreads + threadIdx.x, (uint64_t)gridDim.x * kThreads);
}
__global__ void __launch_bounds__(kThreads) k_plan_per(const uint32_t* counts, uint64_t n_out, uint32_t cap, uint32_t* per,
                                                       uint32_t* off, uint32_t* start) {
    per_body(counts, n_out, cap, per, off, start, (uint64_t)blockIdx.x * kThreads + threadIdx.x, (uint64_t)gridDim.x * kThreads);
}
__global__ void __launch_bounds__(kThreads) k_plan_tasks(TasksArgs A) {
    tasks_body(A, (uint64_t)blockIdx.x * kThreads + threadIdx.x, (uint64_t)gridDim.x * kThreads);
}

namespace {

// the launcher segment_plan.h plan_sort / plan_level are written against
struct HipLaunch {
    hipStream_t st;
    uint64_t max_blocks;  // of a grid-strided launch: enough workgroups to fill the device eight times over

    dim3 strided(uint64_t n) const { return dim3((unsigned)std::max<uint64_t>(1, std::min(blocks_for(n, kThreads), max_blocks))); }
    void keys(const KeysArgs& A) { k_plan_keys<<<strided(A.n), dim3(kThreads), 0, st>>>(A); }
    void count(const PassArgs& A) { k_plan_count<<<dim3(A.n_blocks), dim3(kThreads), 0, st>>>(A); }
    void scatter(const PassArgs& A) { k_plan_scatter<<<dim3(A.n_blocks), dim3(kThreads), 0, st>>>(A); }
    void scan_chunks(uint32_t* a, uint64_t n, uint32_t* sums, uint64_t chunks) {
        k_plan_scan_chunks<<<dim3((unsigned)chunks), dim3(kThreads), 0, st>>>(a, n, sums);
    }
    void scan_sums(uint32_t* sums, uint64_t m) { k_plan_scan_sums<<<dim3(1), dim3(kThreads), 0, st>>>(sums, m); }
    void scan_apply(uint32_t* a, uint64_t n, const uint32_t* sums) { k_plan_scan_apply<<<strided(n), dim3(kThreads), 0, st>>>(a, n, sums); }
    void counts(const uint32_t* keys, uint64_t n, uint32_t n_out, uint32_t* out) {
        k_plan_counts<<<strided((uint64_t)n_out + 1), dim3(kThreads), 0, st>>>(keys, n, n_out, out);
    }
    void per(const uint32_t* counts, uint64_t n_out, uint32_t cap, uint32_t* per_out, uint32_t* off, uint32_t* start) {
        k_plan_per<<<strided(n_out), dim3(kThreads), 0, st>>>(counts, n_out, cap, per_out, off, start);
    }
    void tasks(const TasksArgs& A) { k_plan_tasks<<<strided(A.tasks), dim3(kThreads), 0, st>>>(A); }
};

}  // namespace

void launch_plan_sort(int n_cus, hipStream_t st, const int32_t* ids, const int32_t* node, uint64_t F, uint64_t rows, uint32_t S,
                      uint32_t K, uint32_t* idx_out, uint32_t* counts_out, uint32_t* scratch) {
    HipLaunch go{st, (uint64_t)n_cus * 8};
    plan_sort(go, ids, node, F, rows, S, K, idx_out, counts_out, scratch);
}

void launch_plan_level(int n_cus, hipStream_t st, const uint32_t* counts, uint64_t n_out, uint32_t cap, uint32_t* per_out,
                       uint64_t* task_ptr_out, uint32_t* order_out, uint64_t tasks, uint32_t* scratch) {
    HipLaunch go{st, (uint64_t)n_cus * 8};
    plan_level(go, counts, n_out, cap, per_out, task_ptr_out, order_out, tasks, scratch);
}

}  // namespace plan
}  // namespace phe
