// scrub_kernels.hip -- one window of a scrub (semantics: the public header's cw_dev_store_verify): the stored
// chunks of the directory entries [c, e) are decoded into the caller's work buffer, hashed, and judged against the digests the index
// holds for their values.  The heavy steps are the library's own: the restore of restore_kernels.hip, the per-chunk hash, and a sweep
// of the index's table (dedupe_kernels.hip).  This file plans the window in front of them and merges the verdicts behind them.
//
// Plan: classify the entries [c, E), E = min(dir_entries, c + entry_cap): need[k] = the length of a selected entry that is sound by
// store_device.h's rule (it will be decoded), else 0, and verdict[k] = SKIPPED, UNSOUND or -- for an entry that will be
// decoded -- ORPHAN, which the table sweep lowers.  The index-only pack scan over need gives raw_off; the window ends at the largest
// e with raw_off[e - c] <= work_bytes (raw_off does not decrease, so exactly one lane finds it).  The window's recipe names the
// entries that will be decoded by their own values and every other one by CW_DEDUPE_MISS, which the restore refuses without a load.
// Finish: the restore's status overrides the sweep's verdict (1 stays 1; a refusal, which the plan's checks rule out, counts as
// UNSOUND), d_status[c..e) is written, the totals grow by per-workgroup counts, the cursor moves.  Everything that one kernel reads
// of another's output lies behind a kernel boundary, and only the last kernel writes what the caller sees: a call whose cursor is at
// or past dir_entries plans an empty window and writes nothing.
//
// Scratch, per stream: 72 + (28 + digest bytes) * W bytes, W = min(CW_SCRUB_ENTRIES, dir_entries) -- a 64-byte head (c, e - c, E - c),
// the digests, raw_off (u64, W + 1), the recipe's refs (u64), and need, the restore's statuses and the verdicts (u32 each).

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cw_device.h"
#include "store_device.h"

namespace cw {

namespace {

using namespace chunkstore;

constexpr uint32_t kOk = 0, kMalformed = 1, kUnsound = 2, kMismatch = 3, kOrphan = 4, kSkipped = 5; // CW_SCRUB_*

struct ScrubHead { // the first 24 of the scratch's 64 head bytes
    unsigned long long c, n, m; // the cursor as the call found it, e - c, E - c
};

// need and verdict of the entries [c, E); the head
__global__ void __launch_bounds__(kThreads)
scrub_classify_kernel(const uint4 *__restrict__ dir, uint64_t dir_entries, uint64_t store_bytes, const uint32_t *__restrict__ live,
                      const uint64_t *__restrict__ d_cursor, uint64_t entry_cap, uint32_t *__restrict__ need, uint32_t *__restrict__ verdict,
                      ScrubHead *__restrict__ head)
{
    const uint64_t c = *d_cursor, m = c < dir_entries ? umin64(entry_cap, dir_entries - c) : 0, threads = (uint64_t)gridDim.x * kThreads;
    for (uint64_t k = (uint64_t)blockIdx.x * kThreads + threadIdx.x; k < m; k += threads) {
        const uint64_t idx = c + k;
        const Entry e(dir[idx]);
        const bool selected = live ? live[idx] != 0 : e.nonzero, decode = selected && e.sound(store_bytes);
        need[k] = decode ? e.len() : 0u;
        verdict[k] = !selected ? kSkipped : decode ? kOrphan : kUnsound;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        head->c = c;
        head->n = 0;
        head->m = m;
    }
}

// the window's recipe and its end: raw_off[0] = 0 and raw_off[1] <= 65536 <= work_bytes, so some k + 1 in (0, m] qualifies
__global__ void __launch_bounds__(kThreads)
scrub_recipe_kernel(const unsigned long long *__restrict__ raw_off, uint64_t dir_base, uint64_t work_bytes, const uint32_t *__restrict__ verdict,
                    uint64_t *__restrict__ ref, ScrubHead *head)
{
    const uint64_t c = head->c, m = head->m, threads = (uint64_t)gridDim.x * kThreads;
    for (uint64_t k = (uint64_t)blockIdx.x * kThreads + threadIdx.x; k < m; k += threads) {
        ref[k] = verdict[k] == kOrphan ? dir_base + c + k : UINT64_MAX;
        if (raw_off[k + 1] <= work_bytes && (k + 1 == m || raw_off[k + 2] > work_bytes)) head->n = k + 1;
    }
}

// d_status[c..e), the totals {checked, ok, malformed, unsound, mismatch, orphan, raw bytes, windows}, the cursor
__global__ void __launch_bounds__(kThreads)
scrub_finish_kernel(const ScrubHead *__restrict__ head, const unsigned long long *__restrict__ raw_off, const uint32_t *__restrict__ verdict,
                    const uint32_t *__restrict__ decoded, uint32_t *__restrict__ status, uint64_t *__restrict__ d_cursor,
                    unsigned long long *__restrict__ totals)
{
    __shared__ uint32_t wsum[kThreads / 64];
    const uint64_t c = head->c, n = head->n, threads = (uint64_t)gridDim.x * kThreads;
    uint32_t ok = 0, malformed = 0, unsound = 0, mismatch = 0, orphan = 0; // (a thread sees at most W / threads + 1 < 2^32 entries)
    for (uint64_t k = (uint64_t)blockIdx.x * kThreads + threadIdx.x; k < n; k += threads) {
        uint32_t s = verdict[k];
        if (s != kSkipped && s != kUnsound) {
            const uint32_t r = decoded[k];
            if (r) s = r == 1 ? kMalformed : kUnsound;
        }
        status[c + k] = s;
        ok += s == kOk;
        malformed += s == kMalformed;
        unsound += s == kUnsound;
        mismatch += s == kMismatch;
        orphan += s == kOrphan;
    }
    const uint32_t o = group_sum(ok, wsum), b = group_sum(malformed, wsum), u = group_sum(unsound, wsum), x = group_sum(mismatch, wsum),
                   r = group_sum(orphan, wsum);
    if (threadIdx.x != 0 || n == 0) return;
    const uint32_t counts[6] = {o + b + u + x + r, o, b, u, x, r};
#pragma unroll
    for (int t = 0; t < 6; t++)
        if (counts[t]) __hip_atomic_fetch_add(totals + t, (unsigned long long)counts[t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (blockIdx.x != 0) return;
    __hip_atomic_fetch_add(totals + 6, raw_off[n], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_fetch_add(totals + 7, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    *d_cursor = c + n;
}

// per stream: the layout of the header comment
StreamScratch<DeviceBuf> scrub_spaces;
static_assert(sizeof(ScrubHead) <= kScratchHead, "the head holds the cursor and both counts");

} // namespace

size_t store_verify_window(size_t dir_entries, long knob)
{
    size_t cap = knob > 0 ? (size_t)knob : (size_t)1 << 20;
    if (cap < 64) cap = 64;
    return cap < dir_entries ? cap : dir_entries;
}

size_t store_verify_scratch_bytes(size_t window, unsigned digest_bytes) { return kScratchHead + 8 + (28 + (size_t)digest_bytes) * window; }

hipError_t store_verify_launch(int lzf, const uint8_t *store, size_t store_bytes, const void *dir, uint64_t dir_base, size_t dir_entries,
                               const uint32_t *live, uint64_t *d_cursor, uint8_t *work, size_t work_bytes, size_t window, unsigned digest_bytes,
                               uint32_t *status, uint64_t *totals, const ScrubJudge &judge, hipStream_t stream)
{
    auto &w = scrub_spaces.at(stream);
    LaunchLock sequence(w.launch); // the head and the window's arrays are shared by the launches below
    hipError_t e = w.reserve(store_verify_scratch_bytes(window, digest_bytes), (size_t)1 << 20);
    if (e != hipSuccess) return e;
    ScrubHead *head = w.as<ScrubHead>();
    uint8_t *dig = w.as<uint8_t>() + kScratchHead;
    uint64_t *raw_off = reinterpret_cast<uint64_t *>(dig + (size_t)digest_bytes * window), *ref = raw_off + window + 1;
    uint32_t *need = reinterpret_cast<uint32_t *>(ref + window), *decoded = need + window, *verdict = decoded + window;
    const uint4 *entries = static_cast<const uint4 *>(dir);
    const uint64_t *n = reinterpret_cast<const uint64_t *>(&head->n), *m = reinterpret_cast<const uint64_t *>(&head->m);
    const unsigned long long *o = reinterpret_cast<const unsigned long long *>(raw_off);
    const dim3 g(lane_grid(window)), b(kThreads);
    hipLaunchKernelGGL(scrub_classify_kernel, g, b, 0, stream, entries, (uint64_t)dir_entries, (uint64_t)store_bytes, live, d_cursor, (uint64_t)window,
                       need, verdict, head);
    // raw_off[k] = sum of need[0..k) for k <= E - c (an empty window: raw_off[0] = 0)
    if ((e = chunk_pack_launch(0, nullptr, nullptr, nullptr, m, window, need, nullptr, raw_off, stream)) != hipSuccess) return e;
    hipLaunchKernelGGL(scrub_recipe_kernel, g, b, 0, stream, o, dir_base, (uint64_t)work_bytes, verdict, ref, head);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if ((e = chunk_restore_launch(lzf, store, store_bytes, dir, dir_base, dir_entries, ref, raw_off, n, window, work, work_bytes, decoded, stream)) !=
        hipSuccess)
        return e;
    const ScrubWindow win{reinterpret_cast<const uint64_t *>(head), raw_off, n, window, decoded, dig, verdict};
    if ((e = judge.fn(judge.ctx, win)) != hipSuccess) return e;
    hipLaunchKernelGGL(scrub_finish_kernel, g, b, 0, stream, head, o, verdict, decoded, status, d_cursor, reinterpret_cast<unsigned long long *>(totals));
    return hipGetLastError();
}

} // namespace cw
