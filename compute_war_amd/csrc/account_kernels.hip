// account_kernels.hip -- the chunk store accounts: cw_dev_store_account computes, from the recipes of one call,
// the reverse references of a directory -- per entry how many positions name it and which stream owns it, per stream what it shares
// with no other stream of the call and how much of it sits in flagged entries.  Counts on demand, not maintained ones: nothing here
// keeps state between calls, no entry is judged and nothing is decoded.
//
// Four steps, each behind a kernel boundary: the check of the stream index, which leaves the verdict in the scratch head; a clear of
// the per-entry words and of the outputs that are summed into; the positions pass, one lane per position; the entries pass, one lane
// per entry.  Every kernel behind the check reads the verdict and returns when it is 1, so a refused call writes nothing but its
// verdict.  Everything summed is an integer and min / max do not depend on order: the result is a function of the arguments.
//
// Scratch, per stream: 64 + 12 * dir_entries bytes (the header promises at most 72 + 12 * dir_entries) -- a 64-byte head (the verdict
// at [0]) and three u32 words per entry behind it (the count, the lowest and the highest stream that name the entry).

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cw_device.h"
#include "store_device.h"

namespace cw {

namespace {

using namespace chunkstore;

constexpr uint32_t kOwnerNone = 0xFFFFFFFFu, kOwnerShared = 0xFFFFFFFEu; // CW_OWNER_NONE, CW_OWNER_SHARED
typedef unsigned long long u64;

// cw_stream_account as the eight u64 words the kernels add to
enum { kPositions, kMissing, kLogicalBytes, kUniqueChunks, kUniqueStored, kUniqueRaw, kFlaggedPositions, kFlaggedBytes, kAcctWords };

__device__ __forceinline__ void add64(u64 *p, u64 v)
{
    if (v) __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- 1. the check ------------------------------------------------------------------------------------------------------------------
// *verdict |= 1 when first[0] != 0, when a pair decreases or when first[nstreams] > max_positions (the host zeroed it)
__global__ void __launch_bounds__(kThreads)
account_check_kernel(const uint64_t *__restrict__ first, uint64_t nstreams, uint64_t max_positions, uint32_t *__restrict__ verdict)
{
    __shared__ u64 wsum[kThreads / 64];
    const uint64_t threads = (uint64_t)gridDim.x * kThreads, t = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    uint32_t bad = t == 0 && (first[0] != 0 || first[nstreams] > max_positions);
    for (uint64_t f = t; f < nstreams; f += threads) bad |= first[f] > first[f + 1];
    const u64 all = group_sum(bad, wsum);
    if (threadIdx.x == 0 && all) atomicOr(verdict, 1u);
}

// ---- 2. the clear ------------------------------------------------------------------------------------------------------------------
// totals[0] = the verdict; verdict 0: the per-entry words (count 0, lowest 2^32 - 1, highest 0), acct and totals[1..7] to zero
__global__ void __launch_bounds__(kThreads)
account_clear_kernel(const uint32_t *__restrict__ verdict, uint64_t dir_entries, uint64_t nstreams, uint32_t *__restrict__ count,
                     uint32_t *__restrict__ lowest, uint32_t *__restrict__ highest, uint64_t *__restrict__ acct, uint64_t *__restrict__ totals)
{
    const uint32_t v = *verdict;
    const uint64_t threads = (uint64_t)gridDim.x * kThreads, t = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (t == 0) totals[0] = v;
    if (v) return; // (words 1..7 keep what they hold)
    if (t >= 1 && t < 8) totals[t] = 0;
    for (uint64_t idx = t; idx < dir_entries; idx += threads) {
        count[idx] = 0u;
        lowest[idx] = 0xFFFFFFFFu;
        highest[idx] = 0u;
    }
    for (uint64_t w = t; w < nstreams * kAcctWords; w += threads) acct[w] = 0;
}

// ---- 3. the positions --------------------------------------------------------------------------------------------------------------
// the last f with first[f] <= p; verdict 0: first[0] = 0 <= p < first[nstreams], and first[lo] <= p < first[hi] holds throughout
__device__ __forceinline__ uint32_t stream_of(const uint64_t *__restrict__ first, uint32_t nstreams, uint64_t p)
{
    uint32_t lo = 0, hi = nstreams;
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (first[mid] <= p) lo = mid;
        else hi = mid;
    }
    return lo;
}

// One lane per position, 64 consecutive positions per wavefront.  A wavefront whose positions lie in one stream (the common case:
// found with one search for its first position and one load) sums over its lanes and issues one atomic per field; one that
// straddles a stream boundary searches per lane and adds per lane.
__global__ void __launch_bounds__(kThreads)
account_positions_kernel(const uint32_t *__restrict__ verdict, const uint64_t *__restrict__ ref, const uint64_t *__restrict__ first,
                         uint32_t nstreams, const uint4 *__restrict__ dir, uint64_t dir_base, uint64_t dir_entries,
                         const uint32_t *__restrict__ flag, uint32_t *__restrict__ count, uint32_t *__restrict__ lowest,
                         uint32_t *__restrict__ highest, u64 *__restrict__ acct, u64 *__restrict__ totals)
{
    __shared__ u64 wsum[kThreads / 64];
    if (*verdict) return;
    const uint64_t n = first[nstreams], threads = (uint64_t)gridDim.x * kThreads;
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t all_missing = 0; // (a thread sees at most n / threads + 1 < 2^32 positions)
    for (uint64_t p0 = (uint64_t)blockIdx.x * kThreads + (threadIdx.x & ~63u); p0 < n; p0 += threads) { // (wave-uniform)
        const uint64_t p = p0 + lane;
        const bool active = p < n;
        // the stream of the wavefront's first position, and whether its last position lies in it too
        const uint64_t w0 = ((uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)(p0 >> 32)) << 32) | __builtin_amdgcn_readfirstlane((uint32_t)p0);
        const uint32_t f0 = stream_of(first, nstreams, w0);
        const uint64_t w_last = umin64(w0 + 63, n - 1);
        const bool one_stream = w_last < first[f0 + 1];
        const uint32_t f = one_stream || !active ? f0 : stream_of(first, nstreams, p);

        uint32_t missing = 0, len = 0, flagged = 0;
        if (active) {
            uint64_t idx;
            missing = 1;
            if (names_entry(ref[p], dir_base, dir_entries, idx)) {
                const Entry e(dir[idx]);
                if (e.nonzero) {
                    missing = 0;
                    len = e.len();
                    flagged = flag && flag[idx] != 0;
                    atomicAdd(&count[idx], 1u);
                    atomicMin(&lowest[idx], f);
                    atomicMax(&highest[idx], f);
                }
            }
        }
        all_missing += missing;
        const uint32_t flagged_len = flagged ? len : 0u;
        if (one_stream) { // (64 lengths of at most 2^17 - 1 sum below 2^32)
            const uint32_t s_pos = wave_sum(active), s_miss = wave_sum(missing), s_len = wave_sum(len), s_flag = wave_sum(flagged),
                           s_flen = wave_sum(flagged_len);
            if (lane == 0) {
                u64 *a = acct + (uint64_t)f0 * kAcctWords;
                add64(a + kPositions, s_pos);
                add64(a + kMissing, s_miss);
                add64(a + kLogicalBytes, s_len);
                add64(a + kFlaggedPositions, s_flag);
                add64(a + kFlaggedBytes, s_flen);
            }
        } else if (active) {
            u64 *a = acct + (uint64_t)f * kAcctWords;
            add64(a + kPositions, 1);
            add64(a + kMissing, missing);
            add64(a + kLogicalBytes, len);
            add64(a + kFlaggedPositions, flagged);
            add64(a + kFlaggedBytes, flagged_len);
        }
    }
    const u64 all = group_sum(all_missing, wsum);
    if (threadIdx.x == 0) add64(totals + 7, all);
}

// ---- 4. the entries ----------------------------------------------------------------------------------------------------------------
// One lane per entry: none / one / shared from lowest == highest, the per-entry outputs, the owner's unique_* and the totals (one
// atomic per workgroup and word).  The owners of a wavefront's entries are few -- a stream's new chunks take consecutive values --
// so the wavefront sums per distinct owner, up to kOwnerRounds of them, before the lanes left over add on their own.
constexpr int kOwnerRounds = 4;

__global__ void __launch_bounds__(kThreads)
account_entries_kernel(const uint32_t *__restrict__ verdict, const uint4 *__restrict__ dir, uint64_t dir_entries,
                       const uint32_t *__restrict__ count, const uint32_t *__restrict__ lowest, const uint32_t *__restrict__ highest,
                       uint32_t *__restrict__ refcount, uint32_t *__restrict__ owner, u64 *__restrict__ acct, u64 *__restrict__ totals)
{
    __shared__ u64 wsum[kThreads / 64];
    if (*verdict) return;
    const uint64_t threads = (uint64_t)gridDim.x * kThreads;
    const uint32_t lane = threadIdx.x & 63u;
    u64 nonzero = 0, nonzero_stored = 0, referenced = 0, referenced_stored = 0, shared = 0, shared_stored = 0;
    for (uint64_t i0 = (uint64_t)blockIdx.x * kThreads + (threadIdx.x & ~63u); i0 < dir_entries; i0 += threads) { // (wave-uniform)
        const uint64_t idx = i0 + lane;
        uint32_t own = kOwnerNone, stored = 0, len = 0;
        if (idx < dir_entries) {
            const Entry e(dir[idx]);
            const uint32_t c = count[idx]; // (c != 0: a position named the entry, which is then not all zero)
            const bool nz = e.nonzero;
            stored = e.stored;
            len = e.len();
            if (c) own = lowest[idx] == highest[idx] ? lowest[idx] : kOwnerShared;
            if (refcount) refcount[idx] = c;
            if (owner) owner[idx] = own;
            nonzero += nz;
            nonzero_stored += nz ? stored : 0u;
            referenced += c != 0;
            referenced_stored += c ? stored : 0u;
            shared += own == kOwnerShared;
            shared_stored += own == kOwnerShared ? stored : 0u;
        }
        bool pending = own < kOwnerShared; // one stream names the entry
        for (int round = 0; round < kOwnerRounds; round++) {
            const u64 left = __ballot(pending);
            if (!left) break;
            const uint32_t o = (uint32_t)__shfl((int)own, __ffsll((long long)left) - 1, 64);
            const bool mine = pending && own == o;
            // (stored is any u32: its sum takes both halves; 64 lengths sum below 2^32)
            const uint32_t s_n = wave_sum(mine), s_lo = wave_sum(mine ? stored & 0xFFFFu : 0u), s_hi = wave_sum(mine ? stored >> 16 : 0u),
                           s_len = wave_sum(mine ? len : 0u);
            if (lane == 0) {
                u64 *a = acct + (uint64_t)o * kAcctWords;
                add64(a + kUniqueChunks, s_n);
                add64(a + kUniqueStored, ((u64)s_hi << 16) + s_lo);
                add64(a + kUniqueRaw, s_len);
            }
            pending = pending && !mine;
        }
        if (pending) {
            u64 *a = acct + (uint64_t)own * kAcctWords;
            add64(a + kUniqueChunks, 1);
            add64(a + kUniqueStored, stored);
            add64(a + kUniqueRaw, len);
        }
    }
    const u64 t1 = group_sum(nonzero, wsum), t2 = group_sum(nonzero_stored, wsum), t3 = group_sum(referenced, wsum),
              t4 = group_sum(referenced_stored, wsum), t5 = group_sum(shared, wsum), t6 = group_sum(shared_stored, wsum);
    if (threadIdx.x != 0) return;
    add64(totals + 1, t1);
    add64(totals + 2, t2);
    add64(totals + 3, t3);
    add64(totals + 4, t4);
    add64(totals + 5, t5);
    add64(totals + 6, t6);
}

// per stream: the verdict at [0], the counts, the lowest and the highest streams (u32, dir_entries each) from byte 64
StreamScratch<DeviceBuf> account_spaces;

} // namespace

hipError_t store_account_launch(const uint64_t *ref, const uint64_t *first, size_t nstreams, size_t max_positions, const void *dir,
                                uint64_t dir_base, size_t dir_entries, const uint32_t *flag, void *acct, uint32_t *refcount, uint32_t *owner,
                                uint64_t *totals, hipStream_t stream)
{
    auto &w = account_spaces.at(stream);
    LaunchLock sequence(w.launch); // the head and the per-entry words are shared by the launches below
    hipError_t e = w.reserve(kScratchHead + dir_entries * 12, (size_t)1 << 20);
    if (e != hipSuccess) return e;
    uint32_t *verdict = w.as<uint32_t>();
    uint32_t *count = reinterpret_cast<uint32_t *>(w.as<uint8_t>() + kScratchHead), *lowest = count + dir_entries, *highest = lowest + dir_entries;
    if ((e = hipMemsetAsync(verdict, 0, kScratchHead, stream)) != hipSuccess) return e;
    const uint4 *entries = static_cast<const uint4 *>(dir);
    u64 *a = static_cast<u64 *>(acct), *t = reinterpret_cast<u64 *>(totals);
    hipLaunchKernelGGL(account_check_kernel, dim3(lane_grid(nstreams)), dim3(kThreads), 0, stream, first, (uint64_t)nstreams,
                       (uint64_t)max_positions, verdict);
    const size_t clears = dir_entries > nstreams * kAcctWords ? dir_entries : nstreams * kAcctWords;
    hipLaunchKernelGGL(account_clear_kernel, dim3(lane_grid(clears)), dim3(kThreads), 0, stream, verdict, (uint64_t)dir_entries,
                       (uint64_t)nstreams, count, lowest, highest, static_cast<uint64_t *>(acct), totals);
    if (max_positions) // (else verdict 0 means no position)
        hipLaunchKernelGGL(account_positions_kernel, dim3(lane_grid(max_positions)), dim3(kThreads), 0, stream, verdict, ref, first,
                           (uint32_t)nstreams, entries, dir_base, (uint64_t)dir_entries, flag, count, lowest, highest, a, t);
    hipLaunchKernelGGL(account_entries_kernel, dim3(lane_grid(dir_entries)), dim3(kThreads), 0, stream, verdict, entries, (uint64_t)dir_entries,
                       count, lowest, highest, refcount, owner, a, t);
    return hipGetLastError();
}

} // namespace cw
