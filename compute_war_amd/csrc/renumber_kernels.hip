// renumber_kernels.hip -- the chunk store gives directory slots back: cw_dev_store_renumber moves the kept
// entries of a directory to dense values [new_base, new_base + K) of a new directory and writes the ascending (from, to) pairs that
// cw_dev_translate_refs and cw_dev_dedupe_revalue take.  Entries move bit for bit: no stored byte moves, nothing is decoded and no
// entry is judged.  Nothing here keeps state between calls.
//
// Five steps, each behind a kernel boundary: flags[idx] = "entry idx is kept" with the count of the non-zero entries that are not
// (one atomic per workgroup); the index-only scan of pack_kernels.hip over the flags, which gives every kept entry its rank and, at
// [dir_entries], K; a zero fill of the new directory; the scatter, one lane per old entry; one thread that reports.  Fill, scatter
// and finish evaluate the same verdict from K, so a call that is refused writes nothing but its result.
//
// Scratch, per stream: 72 + 12 * dir_entries bytes -- a 64-byte head (the dropped count at [0]), the ranks (u64, dir_entries + 1)
// and the flags (u32) behind them.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cw_device.h"
#include "store_device.h"

namespace cw {

namespace {

using namespace chunkstore;

// flags[idx] = 1 for a kept entry (not all zero, and flagged when live is given), else 0; *n_dropped += the non-zero entries not kept
__global__ void __launch_bounds__(kThreads)
renumber_flags_kernel(const uint4 *__restrict__ dir, uint64_t dir_entries, const uint32_t *__restrict__ live, uint32_t *__restrict__ flags,
                      unsigned long long *__restrict__ n_dropped)
{
    __shared__ uint32_t wsum[kThreads / 64];
    const uint64_t threads = (uint64_t)gridDim.x * kThreads;
    uint32_t dropped = 0; // (a thread sees at most dir_entries / threads + 1 < 2^32 entries)
    for (uint64_t idx = (uint64_t)blockIdx.x * kThreads + threadIdx.x; idx < dir_entries; idx += threads) {
        const Entry e(dir[idx]);
        const bool keep = e.nonzero && (!live || live[idx] != 0);
        flags[idx] = keep;
        dropped += e.nonzero && !keep;
    }
    const uint32_t all = group_sum(dropped, wsum);
    if (threadIdx.x == 0 && all) __hip_atomic_fetch_add(n_dropped, (unsigned long long)all, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// where the K kept entries go, and what fill, scatter and finish are gated on
struct Placement {
    uint64_t new_base, new_dir_base, new_dir_entries, max_pairs; // (new_dir_base + new_dir_entries does not wrap: the host checked)

    // 2: [new_base, new_base + K) wraps or leaves the new directory (an empty range leaves nothing); else 1: more pairs than room
    __device__ __forceinline__ uint32_t verdict(uint64_t K) const
    {
        if (K != 0) {
            if (new_base + K < new_base || new_base < new_dir_base) return 2u;
            const uint64_t first = new_base - new_dir_base;
            if (first > new_dir_entries || K > new_dir_entries - first) return 2u;
        }
        return K > max_pairs ? 1u : 0u;
    }
};

__global__ void __launch_bounds__(kThreads)
renumber_fill_kernel(const unsigned long long *__restrict__ rank, uint64_t dir_entries, Placement p, uint4 *__restrict__ new_dir)
{
    if (p.verdict(rank[dir_entries])) return;
    const uint64_t threads = (uint64_t)gridDim.x * kThreads;
    for (uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x; i < p.new_dir_entries; i += threads) new_dir[i] = make_uint4(0u, 0u, 0u, 0u);
}

// One lane per old entry.  Verdict 0: a kept entry's rank k < K <= max_pairs, and new_base + k lies inside the new directory.
__global__ void __launch_bounds__(kThreads)
renumber_scatter_kernel(const uint4 *__restrict__ dir, uint64_t dir_base, uint64_t dir_entries, const uint32_t *__restrict__ flags,
                        const unsigned long long *__restrict__ rank, Placement p, uint4 *__restrict__ new_dir, uint64_t *__restrict__ from,
                        uint64_t *__restrict__ to)
{
    if (p.verdict(rank[dir_entries])) return;
    const uint64_t threads = (uint64_t)gridDim.x * kThreads;
    for (uint64_t idx = (uint64_t)blockIdx.x * kThreads + threadIdx.x; idx < dir_entries; idx += threads) {
        if (flags[idx] == 0) continue;
        const uint64_t k = rank[idx];
        from[k] = dir_base + idx;
        to[k] = p.new_base + k;
        new_dir[p.new_base + k - p.new_dir_base] = dir[idx];
    }
}

// one thread, behind the scatter: the result
__global__ void __launch_bounds__(64)
renumber_finish_kernel(const unsigned long long *__restrict__ rank, uint64_t dir_entries, const unsigned long long *__restrict__ n_dropped,
                       Placement p, uint64_t *__restrict__ result)
{
    if (threadIdx.x != 0) return;
    const uint64_t K = rank[dir_entries];
    result[0] = p.verdict(K);
    result[1] = K;
    result[2] = p.new_base + K;
    result[3] = *n_dropped;
}

// per stream: the dropped count at [0], the ranks (u64, dir_entries + 1) from byte 64, the flags (u32) behind them
StreamScratch<DeviceBuf> renumber_spaces;

} // namespace

hipError_t store_renumber_launch(const void *dir, uint64_t dir_base, size_t dir_entries, const uint32_t *live, uint64_t new_base, void *new_dir,
                                 uint64_t new_dir_base, size_t new_dir_entries, uint64_t *from, uint64_t *to, size_t max_pairs, uint64_t *result,
                                 hipStream_t stream)
{
    auto &w = renumber_spaces.at(stream);
    LaunchLock sequence(w.launch); // head, ranks and flags are shared by the launches below
    ScanScratch s;
    hipError_t e = scan_scratch(w, dir_entries, stream, s);
    if (e != hipSuccess) return e;
    unsigned long long *head = s.head_as<unsigned long long>();
    uint32_t *flags = s.sizes;
    const uint4 *entries = static_cast<const uint4 *>(dir);
    hipLaunchKernelGGL(renumber_flags_kernel, dim3(lane_grid(dir_entries)), dim3(kThreads), 0, stream, entries, (uint64_t)dir_entries, live, flags,
                       head);
    // rank[idx] = the kept entries below idx, for idx <= dir_entries
    if ((e = pack_launch(nullptr, 0, flags, dir_entries, nullptr, s.off, stream)) != hipSuccess) return e;
    const unsigned long long *r = s.offsets();
    const Placement p{new_base, new_dir_base, (uint64_t)new_dir_entries, (uint64_t)max_pairs};
    if (new_dir_entries)
        hipLaunchKernelGGL(renumber_fill_kernel, dim3(lane_grid(new_dir_entries)), dim3(kThreads), 0, stream, r, (uint64_t)dir_entries, p,
                           static_cast<uint4 *>(new_dir));
    if (new_dir_entries && max_pairs) // (else a kept entry gives verdict 2 or 1, and without one there is nothing to place)
        hipLaunchKernelGGL(renumber_scatter_kernel, dim3(lane_grid(dir_entries)), dim3(kThreads), 0, stream, entries, dir_base,
                           (uint64_t)dir_entries, flags, r, p, static_cast<uint4 *>(new_dir), from, to);
    hipLaunchKernelGGL(renumber_finish_kernel, dim3(1), dim3(64), 0, stream, r, (uint64_t)dir_entries, head, p, result);
    return hipGetLastError();
}

} // namespace cw
