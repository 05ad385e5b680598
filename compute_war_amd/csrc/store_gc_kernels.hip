// store_gc_kernels.hip -- the chunk store forgets: cw_dev_store_mark sets a flag for every directory entry
// a kept recipe names, cw_dev_store_compact moves the flagged entries' stored bytes back to back into a new store and writes the
// directory that goes with it.  Mark and sweep, not reference counts: a mark is a plain store of 1, so marking twice changes
// nothing and nothing can underflow.  Nothing here keeps state between calls, and nothing decodes: extents move as they are.
//
// Mark: one lane per recipe position; positions that name no entry of the directory are counted, one atomic per workgroup.
//
// Compact mirrors the append of restore_kernels.hip: per entry its stored size or 0 when it is not kept, with the "a kept entry is
// unsound" flag and the kept / dropped counts (one atomic each per workgroup); the index-only scan of pack_kernels.hip over those
// sizes; a copy that also writes the new directory; one thread that sets the cursor and reports.  Copy and finish evaluate the same
// verdict, so a compaction that does not fit, or that would have to follow an unsound entry, changes nothing.  Everything that one
// kernel reads of another's output lies behind a kernel boundary.
//
// Scratch, per stream: 72 + 12 * dir_entries bytes -- a 64-byte head (the flag word at [0], the kept count at byte 8, the dropped
// count at byte 16), the scan's offsets (u64, dir_entries + 1) and the sizes (u32) behind them.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cw_device.h"
#include "store_device.h"

namespace cw {

namespace {

using namespace chunkstore;

// ---- mark --------------------------------------------------------------------------------------------------------------------
// live[ref[j] - dir_base] = 1 for every position j < min(*d_count, max_count) that names an entry; the others are counted
__global__ void __launch_bounds__(kThreads)
store_mark_kernel(const uint64_t *__restrict__ ref, const uint64_t *__restrict__ d_count, uint64_t max_count, uint64_t dir_base,
                  uint64_t dir_entries, uint32_t *__restrict__ live, unsigned long long *__restrict__ n_outside)
{
    __shared__ uint32_t wsum[kThreads / 64];
    const uint64_t n = umin64(*d_count, max_count), threads = (uint64_t)gridDim.x * kThreads;
    uint32_t outside = 0; // (a thread sees at most max_count / threads + 1 < 2^32 positions)
    for (uint64_t j = (uint64_t)blockIdx.x * kThreads + threadIdx.x; j < n; j += threads) {
        uint64_t idx;
        if (names_entry(ref[j], dir_base, dir_entries, idx)) live[idx] = 1u; // racing stores of the same value
        else outside++;
    }
    const uint32_t all = group_sum(outside, wsum);
    if (threadIdx.x == 0 && all) __hip_atomic_fetch_add(n_outside, (unsigned long long)all, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- compact -----------------------------------------------------------------------------------------------------------------
struct GcHead { // the first 24 of the scratch's 64 head bytes
    uint32_t unsound, pad;
    unsigned long long kept, dropped;
};

// sizes[idx] = the stored bytes of a kept entry, else 0; head: an unsound kept entry, the kept and the dropped (non-zero, not kept) counts
__global__ void __launch_bounds__(kThreads)
gc_sizes_kernel(const uint4 *__restrict__ dir, uint64_t dir_entries, const uint32_t *__restrict__ live, uint64_t store_bytes,
                uint32_t *__restrict__ sizes, GcHead *__restrict__ head)
{
    __shared__ uint32_t wsum[kThreads / 64];
    const uint64_t threads = (uint64_t)gridDim.x * kThreads;
    uint32_t kept = 0, dropped = 0;
    bool unsound = false;
    for (uint64_t idx = (uint64_t)blockIdx.x * kThreads + threadIdx.x; idx < dir_entries; idx += threads) {
        const Entry e(dir[idx]);
        const bool keep = e.nonzero && live[idx] != 0;
        sizes[idx] = keep ? e.stored : 0u;
        kept += keep;
        dropped += e.nonzero && !keep;
        unsound |= keep && !e.sound(store_bytes);
    }
    const uint32_t k = group_sum(kept, wsum), d = group_sum(dropped, wsum), u = group_sum(unsound, wsum);
    if (threadIdx.x != 0) return;
    if (k) __hip_atomic_fetch_add(&head->kept, (unsigned long long)k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (d) __hip_atomic_fetch_add(&head->dropped, (unsigned long long)d, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (u) atomicOr(&head->unsound, 1u);
}

// what the copy and the cursor are gated on: every kept entry can be followed, and the kept bytes fit
__device__ __forceinline__ uint32_t gc_verdict(uint32_t unsound, uint64_t total, uint64_t new_store_bytes)
{
    if (unsound) return 2u;
    return total > new_store_bytes ? 1u : 0u;
}

// A wavefront takes 64 entries at a time (directories are sparse: duplicates and dropped chunks have zero entries): every lane reads
// its entry and flag, the wavefront copies the kept extents of those 64 one after the other with all lanes, then every lane writes
// its entry of the new directory -- which may be the old one: a wavefront writes only the 64 entries it has read, and only behind
// their copies.  (dir and new_dir may be equal: no __restrict__ on them.)
__global__ void __launch_bounds__(64)
gc_copy_kernel(const uint8_t *__restrict__ store, uint64_t store_bytes, const uint4 *dir, uint64_t dir_entries, const uint32_t *__restrict__ live,
               const unsigned long long *__restrict__ off, const GcHead *__restrict__ head, uint8_t *__restrict__ new_store, uint64_t new_store_bytes,
               uint4 *new_dir)
{
    if (gc_verdict(head->unsound, off[dir_entries], new_store_bytes)) return;
    const uint64_t lanes = (uint64_t)gridDim.x * 64;
    for (uint64_t first = (uint64_t)blockIdx.x * 64; first < dir_entries; first += lanes) { // (wave-uniform: the copies need every lane)
        const uint64_t idx = first + threadIdx.x;
        bool keep = false;
        uint64_t from = 0, to = 0;
        uint32_t stored = 0, word = 0;
        if (idx < dir_entries) {
            const Entry e(dir[idx]);
            keep = e.nonzero && live[idx] != 0; // verdict 0: it is sound, and [to, to + stored) lies below the total
            from = e.pos;
            stored = e.stored;
            word = e.word;
            to = off[idx];
        }
        wave_copy(keep, store, from, new_store, to, stored);
        if (idx < dir_entries) new_dir[idx] = keep ? make_uint4((uint32_t)to, (uint32_t)(to >> 32), stored, word) : make_uint4(0u, 0u, 0u, 0u);
    }
}

// one thread, behind the copy: the cursor and the result
__global__ void __launch_bounds__(64)
gc_finish_kernel(const unsigned long long *__restrict__ off, uint64_t dir_entries, const GcHead *__restrict__ head, uint64_t new_store_bytes,
                 uint64_t *__restrict__ new_used, uint64_t *__restrict__ result)
{
    if (threadIdx.x != 0) return;
    const uint64_t total = off[dir_entries];
    const uint32_t verdict = gc_verdict(head->unsound, total, new_store_bytes);
    result[0] = verdict;
    result[1] = total;
    result[2] = head->kept;
    result[3] = head->dropped;
    if (verdict == 0) *new_used = total;
}

// per stream: the head at [0], the scan's offsets (u64, dir_entries + 1) from byte 64, the sizes (u32) behind them
StreamScratch<DeviceBuf> gc_spaces;
static_assert(sizeof(GcHead) <= kScratchHead, "the head holds the flag and both counts");

} // namespace

hipError_t store_mark_launch(const uint64_t *ref, const uint64_t *d_count, size_t max_count, uint64_t dir_base, size_t dir_entries,
                             uint32_t *live, uint64_t *n_outside, hipStream_t stream)
{
    if (max_count == 0) return hipSuccess;
    hipLaunchKernelGGL(store_mark_kernel, dim3(lane_grid(max_count)), dim3(kThreads), 0, stream, ref, d_count, (uint64_t)max_count, dir_base,
                       (uint64_t)dir_entries, live, reinterpret_cast<unsigned long long *>(n_outside));
    return hipGetLastError();
}

hipError_t store_compact_launch(const uint8_t *store, size_t store_bytes, const void *dir, size_t dir_entries, const uint32_t *live,
                                uint8_t *new_store, size_t new_store_bytes, uint64_t *new_used, void *new_dir, uint64_t *result,
                                hipStream_t stream)
{
    auto &w = gc_spaces.at(stream);
    LaunchLock sequence(w.launch); // head, sizes and offsets are shared by the launches below
    ScanScratch s;
    hipError_t e = scan_scratch(w, dir_entries, stream, s);
    if (e != hipSuccess) return e;
    GcHead *head = s.head_as<GcHead>();
    const uint4 *entries = static_cast<const uint4 *>(dir);
    hipLaunchKernelGGL(gc_sizes_kernel, dim3(lane_grid(dir_entries)), dim3(kThreads), 0, stream, entries, (uint64_t)dir_entries, live,
                       (uint64_t)store_bytes, s.sizes, head);
    // off[idx] = sum of sizes[0..idx) for idx <= dir_entries
    if ((e = pack_launch(nullptr, 0, s.sizes, dir_entries, nullptr, s.off, stream)) != hipSuccess) return e;
    const unsigned long long *o = s.offsets();
    // a wavefront per 64 entries
    hipLaunchKernelGGL(gc_copy_kernel, dim3(wave_grid((dir_entries + 63) / 64)), dim3(64), 0, stream, store, (uint64_t)store_bytes, entries, (uint64_t)dir_entries, live,
                       o, head, new_store, (uint64_t)new_store_bytes, static_cast<uint4 *>(new_dir));
    hipLaunchKernelGGL(gc_finish_kernel, dim3(1), dim3(64), 0, stream, o, (uint64_t)dir_entries, head, (uint64_t)new_store_bytes, new_used,
                       result);
    return hipGetLastError();
}

} // namespace cw
