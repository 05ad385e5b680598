// dedupe_kernels.hip -- device-resident fingerprint index (cw_dedupe_*, cw_dev_dedupe): batched lookup-or-insert of full
// digests in an open-addressed table with linear probing, on gfx950.  The reference has no counterpart: HashAndCompress.cpp
// computes the digests and drops them (:257).
//
// Table (allocated once by cw_dedupe_create; capacity a power of two >= 2 x max_entries, so the load stays <= 0.5):
//   state[cap]   u64   EMPTY, PENDING(owner block of the running call) or COMMITTED
//   min_idx[cap] u32   lowest block index of the running call that reached the slot (UINT32_MAX between calls)
//   value[cap]   u64   value of the committed digest (base + i of the block that inserted it)
//   key[cap][W]  u64   the committed digest, all of it (W = 2 / 4 / 8 words)
//
// One call is three kernels plus the index-only pack scan (pack_kernels.hip) for the compaction:
//   probe    one lane per block.  Lanes of a wavefront with equal digests elect the lowest lane; only these leaders touch
//            the table.  Each probe step is ONE agent-scope 64-bit CAS EMPTY -> PENDING(leader); what it returns is the only
//            read of `state` (per-XCD L2s are not coherent, MI355X_MICROARCH.md).  EMPTY: claimed; PENDING(k): compare with
//            the batch's digest k; COMMITTED: compare with key[slot], a match is a hit on an earlier call's entry.  A claim or
//            a PENDING match does atomicMin(min_idx[slot], leader); followers copy the leader's record.
//   resolve  one lane per block, after the kernel boundary: ref = stored value (hit) or base + min_idx[slot]; the block with
//            min_idx[slot] == i is new and commits the slot (key, value, then state).  Nothing else here reads state, key
//            or value, so the commits race with nothing.
//   scatter  new_idx[off[i]] = i for the new blocks, min_idx of their slots back to UINT32_MAX (here and not in resolve,
//            where other lanes still read it), *n_new and count += n_new.
// Every leader with digest D walks the same probe sequence and slots only ever fill, so all of them stop at the same slot:
// the committed one if D was inserted earlier, else the first slot one of them claimed.  min_idx then holds the lowest block
// index with digest D whatever the schedule was -- the result of a sequential loop over the batch.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cw_device.h"

namespace cw {

namespace {

constexpr unsigned kThreads = 256;
constexpr uint64_t kEmpty = 0, kPending = 1ull << 32, kCommitted = 2ull << 32;
// per-block record of the probe: the slot, with kHit when the digest was committed by an earlier call; kNoSlot = bound reached
constexpr uint64_t kHit = 1ull << 63, kNoSlot = 1ull << 62, kSlotMask = kNoSlot - 1;

__device__ __forceinline__ uint64_t mix64(uint64_t z)
{
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}

// home slot hash: a splitmix64 chain over EVERY word, order-dependent (digests that share a prefix, or whose words are a
// permutation of each other, still spread)
template <int W>
__device__ __forceinline__ uint64_t fold(const uint64_t (&d)[W])
{
    uint64_t h = 0x9E3779B97F4A7C15ULL;
    for (int w = 0; w < W; w++) h = mix64(h ^ d[w]) + 0x9E3779B97F4A7C15ULL;
    return h;
}

template <int W>
__device__ __forceinline__ bool same(const uint64_t *__restrict__ p, const uint64_t (&d)[W])
{
    bool eq = true;
    for (int w = 0; w < W; w++) eq &= p[w] == d[w];
    return eq;
}

template <int W>
__global__ void __launch_bounds__(kThreads)
dedupe_probe_kernel(const uint64_t *__restrict__ dig, uint32_t n, uint64_t *__restrict__ state, uint32_t *__restrict__ min_idx,
                    const uint64_t *__restrict__ value, const uint64_t *__restrict__ key, uint64_t mask, uint64_t *__restrict__ rec,
                    uint64_t *__restrict__ ref, unsigned long long *__restrict__ err)
{
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u, wave_first = i - lane;
    const bool valid = i < n;
    uint64_t d[W];
    for (int w = 0; w < W; w++) d[w] = valid ? dig[(size_t)i * W + w] : 0;
    const uint64_t h = fold(d);

    // wave-combine: per round the lowest unresolved lane r is broadcast; lanes whose fold matches r's compare the full digest
    // (r's from the batch array) and take r as their leader.  r resolves itself, so a round per distinct digest of the wave.
    uint32_t leader = lane;
    bool open = valid;
    for (unsigned long long todo = __ballot(open); todo; todo = __ballot(open)) {
        const uint32_t r = __builtin_amdgcn_readfirstlane((uint32_t)__builtin_ctzll(todo));
        const uint64_t hr = __shfl(h, (int)r, 64);
        if (open && hr == h && same<W>(dig + (size_t)(wave_first + r) * W, d)) {
            leader = r;
            open = false;
        }
    }

    uint64_t rv = kNoSlot, hv = 0;
    if (valid && leader == lane) {
        uint64_t slot = h & mask;
        for (uint64_t step = 0; step <= mask; step++, slot = (slot + 1) & mask) { // bounded: the load <= 0.5 ends it far sooner
            uint64_t old = kEmpty;
            __hip_atomic_compare_exchange_strong(state + slot, &old, kPending | i, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                 __HIP_MEMORY_SCOPE_AGENT);
            if (old == kEmpty) { rv = slot; break; } // claimed
            if (old == kCommitted) {
                if (same<W>(key + slot * W, d)) { rv = kHit | slot; hv = value[slot]; break; }
            } else if ((uint32_t)old < n && same<W>(dig + (size_t)(uint32_t)old * W, d)) { // PENDING(owner): its digest is in the batch
                rv = slot;
                break;
            }
        }
        if (rv == kNoSlot) __hip_atomic_fetch_or(err, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else if (!(rv & kHit)) __hip_atomic_fetch_min(min_idx + rv, i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    rv = __shfl(rv, (int)leader, 64);
    hv = __shfl(hv, (int)leader, 64);
    if (!valid) return;
    rec[i] = rv;
    if (rv & kHit) ref[i] = hv;
}

template <int W>
__global__ void __launch_bounds__(kThreads)
dedupe_resolve_kernel(const uint64_t *__restrict__ dig, uint32_t n, uint64_t base, const uint32_t *__restrict__ min_idx,
                      uint64_t *__restrict__ state, uint64_t *__restrict__ value, uint64_t *__restrict__ key,
                      const uint64_t *__restrict__ rec, uint64_t *__restrict__ ref, uint32_t *__restrict__ flags)
{
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const uint64_t rv = rec[i];
    if (rv & (kHit | kNoSlot)) { // hit: ref came from the probe; no slot: the call failed (reported by the host)
        if (rv & kNoSlot) ref[i] = UINT64_MAX;
        flags[i] = 0;
        return;
    }
    const uint64_t slot = rv & kSlotMask;
    const uint32_t m = __hip_atomic_load(min_idx + slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    ref[i] = base + m;
    flags[i] = m == i;
    if (m != i) return;
    for (int w = 0; w < W; w++) key[slot * W + w] = dig[(size_t)i * W + w];
    value[slot] = base + i;
    __hip_atomic_store(state + slot, kCommitted, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ void __launch_bounds__(kThreads)
dedupe_scatter_kernel(const uint32_t *__restrict__ flags, const unsigned long long *__restrict__ off, uint32_t n,
                      const uint64_t *__restrict__ rec, uint32_t *__restrict__ min_idx, uint32_t *__restrict__ new_idx,
                      uint64_t *__restrict__ n_new, uint64_t *__restrict__ count)
{
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    if (flags[i]) {
        new_idx[off[i]] = i;
        min_idx[rec[i] & kSlotMask] = UINT32_MAX;
    }
    if (i == 0) { // one lane of the grid; calls on an index are serialised, so the count has no other writer
        const uint64_t t = off[n];
        *n_new = t;
        *count += t;
    }
}

// new block new_idx[j] -> slot j of dst (block_bytes apart): a workgroup per block, 16-byte loads and stores when aligned
__global__ void __launch_bounds__(kThreads)
dedupe_gather_kernel(const uint8_t *__restrict__ src, size_t bb, size_t stride, const uint32_t *__restrict__ new_idx, size_t n_new,
                     uint8_t *__restrict__ dst, bool vec)
{
    for (size_t j = blockIdx.x; j < n_new; j += gridDim.x) {
        const uint8_t *s = src + (size_t)new_idx[j] * stride;
        uint8_t *o = dst + j * bb;
        if (vec) {
            for (size_t k = threadIdx.x; k < bb / 16; k += kThreads)
                reinterpret_cast<uint4 *>(o)[k] = reinterpret_cast<const uint4 *>(s)[k];
        } else {
            for (size_t k = threadIdx.x; k < bb; k += kThreads) o[k] = s[k];
        }
    }
}

unsigned grid_of(uint32_t n) { return (n + kThreads - 1) / kThreads; }

} // namespace

hipError_t dedupe_probe_launch(unsigned words, const uint64_t *dig, uint32_t n, uint64_t *state, uint32_t *min_idx, const uint64_t *value,
                               const uint64_t *key, uint64_t mask, uint64_t *rec, uint64_t *ref, unsigned long long *err, hipStream_t s)
{
    const dim3 g(grid_of(n)), b(kThreads);
    switch (words) {
    case 2: hipLaunchKernelGGL(dedupe_probe_kernel<2>, g, b, 0, s, dig, n, state, min_idx, value, key, mask, rec, ref, err); break;
    case 4: hipLaunchKernelGGL(dedupe_probe_kernel<4>, g, b, 0, s, dig, n, state, min_idx, value, key, mask, rec, ref, err); break;
    case 8: hipLaunchKernelGGL(dedupe_probe_kernel<8>, g, b, 0, s, dig, n, state, min_idx, value, key, mask, rec, ref, err); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t dedupe_resolve_launch(unsigned words, const uint64_t *dig, uint32_t n, uint64_t base, const uint32_t *min_idx, uint64_t *state,
                                 uint64_t *value, uint64_t *key, const uint64_t *rec, uint64_t *ref, uint32_t *flags, hipStream_t s)
{
    const dim3 g(grid_of(n)), b(kThreads);
    switch (words) {
    case 2: hipLaunchKernelGGL(dedupe_resolve_kernel<2>, g, b, 0, s, dig, n, base, min_idx, state, value, key, rec, ref, flags); break;
    case 4: hipLaunchKernelGGL(dedupe_resolve_kernel<4>, g, b, 0, s, dig, n, base, min_idx, state, value, key, rec, ref, flags); break;
    case 8: hipLaunchKernelGGL(dedupe_resolve_kernel<8>, g, b, 0, s, dig, n, base, min_idx, state, value, key, rec, ref, flags); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t dedupe_scatter_launch(const uint32_t *flags, const uint64_t *off, uint32_t n, const uint64_t *rec, uint32_t *min_idx,
                                 uint32_t *new_idx, uint64_t *n_new, uint64_t *count, hipStream_t s)
{
    hipLaunchKernelGGL(dedupe_scatter_kernel, dim3(grid_of(n)), dim3(kThreads), 0, s, flags,
                       reinterpret_cast<const unsigned long long *>(off), n, rec, min_idx, new_idx, n_new, count);
    return hipGetLastError();
}

hipError_t dedupe_gather_launch(const uint8_t *src, size_t block_bytes, size_t src_stride, const uint32_t *new_idx, size_t n_new,
                                uint8_t *dst, hipStream_t s)
{
    if (n_new == 0) return hipSuccess;
    const bool vec = ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst) | block_bytes | src_stride) & 15) == 0;
    const size_t grid = n_new < 65536 ? n_new : 65536;
    hipLaunchKernelGGL(dedupe_gather_kernel, dim3((unsigned)grid), dim3(kThreads), 0, s, src, block_bytes, src_stride, new_idx, n_new,
                       dst, vec);
    return hipGetLastError();
}

} // namespace cw
