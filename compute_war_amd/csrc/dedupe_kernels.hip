// dedupe_kernels.hip -- device-resident fingerprint index (cw_dedupe_*, cw_dev_dedupe*): batched lookup-or-insert of full
// digests in an open-addressed table with linear probing, on gfx950, and the index's lifecycle: read-only lookup, export, the export of
// a directory's flagged entries in value order (cw_dev_dedupe_export_live), the rehash of cw_dedupe_resize, the filtered rehash of cw_dedupe_retain and the
// values rewritten in place by cw_dev_dedupe_revalue.  The reference has no counterpart: HashAndCompress.cpp computes the digests and drops them (:257,
// SURVEY.md D3).
//
// Table (allocated by cw_dedupe_create and again by cw_dedupe_resize; capacity a power of two >= 2 x max_entries, so the load stays <= 0.5):
//   state[cap]   u64   EMPTY, PENDING(owner block of the running call) or COMMITTED
//   min_idx[cap] u32   lowest block index of the running call that reached the slot (UINT32_MAX between calls)
//   value[cap]   u64   value of the committed digest (base + i, or values[i], of the block that inserted it)
//   key[cap][W]  u64   the committed digest, all of it (W = 2 / 4 / 8 words)
//
// One inserting call is three kernels plus the index-only pack scan (pack_kernels.hip) for the compaction:
//   probe    one lane per block.  Lanes of a wavefront with equal digests elect the lowest lane; only these leaders touch
//            the table.  Each probe step is ONE agent-scope 64-bit CAS EMPTY -> PENDING(leader); what it returns is the only
//            read of `state` (per-XCD L2s are not coherent, MI355X_MICROARCH.md).  EMPTY: claimed; PENDING(k): compare with
//            the batch's digest k; COMMITTED: compare with key[slot], a match is a hit on an earlier call's entry.  A claim or
//            a PENDING match does atomicMin(min_idx[slot], leader); followers copy the leader's record.
//   resolve  one lane per block, after the kernel boundary: ref = stored value (hit) or the value of block min_idx[slot]; the block with
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

// kValues: block j carries values[j] (cw_dev_dedupe_insert) instead of base + j
template <int W, bool kValues>
__global__ void __launch_bounds__(kThreads)
dedupe_resolve_kernel(const uint64_t *__restrict__ dig, uint32_t n, uint64_t base, const uint64_t *__restrict__ values,
                      const uint32_t *__restrict__ min_idx, uint64_t *__restrict__ state, uint64_t *__restrict__ value,
                      uint64_t *__restrict__ key, const uint64_t *__restrict__ rec, uint64_t *__restrict__ ref, uint32_t *__restrict__ flags)
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
    const uint64_t v = kValues ? values[m] : base + m;
    ref[i] = v;
    flags[i] = m == i;
    if (m != i) return;
    for (int w = 0; w < W; w++) key[slot * W + w] = dig[(size_t)i * W + w];
    value[slot] = v;
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

// ---- lifecycle: read-only lookup, export, rehash (protocol notes: the head of this file) ----------

// Read-only query, one lane per digest: the probe's fold and bounded walk with PLAIN loads of state.  Calls on an index are
// serialised and a dependent kernel boundary lies between this kernel and every earlier commit, so nothing changes the table
// while it runs (inside the inserting probe that does not hold).  EMPTY ends the walk as a miss; between calls no slot is PENDING.
// The only atomic is the hit count: ballot + population count per wavefront, the workgroup's four counts added up through LDS, then
// one atomic per workgroup (16,384 same-address atomics, one per wavefront of a 2^20 batch, cost more than the walks: DESIGN.md
// section 10).  The error word only ever holds 0 or 1: a plain store sets it.
template <int W>
__global__ void __launch_bounds__(kThreads)
dedupe_lookup_kernel(const uint64_t *__restrict__ dig, uint32_t n, const uint64_t *__restrict__ state, const uint64_t *__restrict__ value,
                     const uint64_t *__restrict__ key, uint64_t mask, uint64_t *__restrict__ ref, unsigned long long *__restrict__ n_found,
                     unsigned long long *__restrict__ err)
{
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    const bool valid = i < n;
    bool hit = false;
    if (valid) {
        uint64_t d[W];
        for (int w = 0; w < W; w++) d[w] = dig[(size_t)i * W + w];
        uint64_t slot = fold(d) & mask, out = UINT64_MAX, step = 0;
        for (; step <= mask; step++, slot = (slot + 1) & mask) {
            const uint64_t st = state[slot];
            if (st == kEmpty) break;
            if (st == kCommitted && same<W>(key + slot * W, d)) { out = value[slot]; hit = true; break; }
        }
        if (step > mask) *err = 1ull; // no EMPTY slot in the whole table: it is inconsistent (the load is <= 0.5)
        ref[i] = out;
    }
    __shared__ uint32_t whits[kThreads / 64];
    const unsigned long long hits = __ballot(hit);
    if ((threadIdx.x & 63u) == 0) whits[threadIdx.x >> 6] = (uint32_t)__builtin_popcountll(hits);
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t all = 0;
        for (uint32_t w = 0; w < kThreads / 64; w++) all += whits[w];
        if (all) __hip_atomic_fetch_add(n_found, (unsigned long long)all, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// Export is a stream compaction over state[cap] in tiles of kThreads slots: committed slots per tile, the index-only pack scan
// over the tile counts (offs[ntiles + 1]), then a pass that finds each committed slot's place inside its tile again with ballots.
__device__ __forceinline__ uint64_t tile_rank(bool c, uint32_t *wcount, uint32_t *total)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const unsigned long long b = __ballot(c);
    if (lane == 0) wcount[wave] = (uint32_t)__builtin_popcountll(b);
    __syncthreads();
    uint32_t before = (uint32_t)__builtin_popcountll(b & ((1ull << lane) - 1ull)), all = 0;
    for (uint32_t w = 0; w < kThreads / 64; w++) {
        if (w < wave) before += wcount[w];
        all += wcount[w];
    }
    __syncthreads(); // the next tile writes wcount again
    *total = all;
    return before;
}

__global__ void __launch_bounds__(kThreads)
dedupe_export_count_kernel(const uint64_t *__restrict__ state, uint64_t cap, uint64_t ntiles, uint32_t *__restrict__ counts)
{
    __shared__ uint32_t wcount[kThreads / 64];
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint64_t slot = tile * kThreads + threadIdx.x;
        uint32_t total;
        (void)tile_rank(slot < cap && state[slot] == kCommitted, wcount, &total);
        if (threadIdx.x == 0) counts[tile] = total;
    }
}

// pairs [first, first + max_out) of the slot order go to out_dig / out_val [0, max_out); *d_n = the entry count (d_n may be NULL)
template <int W>
__global__ void __launch_bounds__(kThreads)
dedupe_export_scatter_kernel(const uint64_t *__restrict__ state, const uint64_t *__restrict__ value, const uint64_t *__restrict__ key,
                             uint64_t cap, uint64_t ntiles, const unsigned long long *__restrict__ offs, uint64_t first, uint64_t max_out,
                             uint64_t *__restrict__ out_dig, uint64_t *__restrict__ out_val, uint64_t *__restrict__ d_n, bool vec)
{
    __shared__ uint32_t wcount[kThreads / 64];
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint64_t t0 = offs[tile], t1 = offs[tile + 1];
        if (t1 <= first || (t0 >= first && t0 - first >= max_out)) continue; // the same for every lane of the workgroup
        const uint64_t slot = tile * kThreads + threadIdx.x;
        const bool c = slot < cap && state[slot] == kCommitted;
        uint32_t total;
        const uint64_t pos = t0 + tile_rank(c, wcount, &total);
        if (!c || pos < first || pos - first >= max_out) continue;
        const uint64_t j = pos - first;
        const uint4 *k = reinterpret_cast<const uint4 *>(key + slot * W); // the key array is 16-byte aligned, W is even
        if (vec) {
            for (int q = 0; q < W / 2; q++) reinterpret_cast<uint4 *>(out_dig + j * W)[q] = k[q];
        } else {
            for (int q = 0; q < W / 2; q++) {
                const uint4 v = k[q];
                out_dig[j * W + 2 * q] = (uint64_t)v.x | (uint64_t)v.y << 32;
                out_dig[j * W + 2 * q + 1] = (uint64_t)v.z | (uint64_t)v.w << 32;
            }
        }
        out_val[j] = value[slot];
    }
    if (d_n && blockIdx.x == 0 && threadIdx.x == 0) *d_n = offs[ntiles];
}

// Rehash into an empty table (cw_dedupe_resize): one lane per old slot.  All keys are distinct and nothing reads keys while this
// runs, so a committed entry walks from its new home slot with one agent-scope CAS EMPTY -> COMMITTED per step until it claims a
// slot, then stores key and value: no PENDING phase, no key compares.  Bounded by the new table's size.  The claim walk (shared with
// the retain below) returns the slot it claimed for digest d, or kNoSlot when it reached the bound.
template <int W>
__device__ __forceinline__ uint64_t claim_committed(uint64_t *__restrict__ state, const uint64_t (&d)[W], uint64_t mask)
{
    uint64_t slot = fold(d) & mask;
    for (uint64_t step = 0; step <= mask; step++, slot = (slot + 1) & mask) {
        uint64_t old = kEmpty;
        __hip_atomic_compare_exchange_strong(state + slot, &old, kCommitted, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (old == kEmpty) return slot;
    }
    return kNoSlot;
}

template <int W>
__global__ void __launch_bounds__(kThreads)
dedupe_rehash_kernel(const uint64_t *__restrict__ old_state, const uint64_t *__restrict__ old_value, const uint64_t *__restrict__ old_key,
                     uint64_t old_cap, uint64_t *__restrict__ state, uint64_t *__restrict__ value, uint64_t *__restrict__ key, uint64_t mask,
                     unsigned long long *__restrict__ err)
{
    for (uint64_t o = (uint64_t)blockIdx.x * kThreads + threadIdx.x; o < old_cap; o += (uint64_t)gridDim.x * kThreads) {
        if (old_state[o] != kCommitted) continue;
        uint64_t d[W];
        for (int w = 0; w < W; w++) d[w] = old_key[o * W + w];
        const uint64_t slot = claim_committed(state, d, mask);
        if (slot == kNoSlot) { *err = 1ull; continue; }
        for (int w = 0; w < W; w++) key[slot * W + w] = d[w];
        value[slot] = old_value[o];
    }
}

// Retain (cw_dedupe_retain): the rehash with a filter.  A committed entry with value v is kept when v names no entry of the directory
// (v - dir_base >= dir_entries in u64) or that entry's flag is set; only kept entries are rehashed, so the new table is what inserting
// them into an empty one gives and no slot ever had to be emptied.  live is complete before the launch (a kernel boundary behind the
// marks).  The kept entries are counted whether or not they found a slot: each lane's count summed per wavefront, then through
// LDS, then one atomic per workgroup, for the reason the lookup counts its hits that way.  state == NULL only counts.
template <int W>
__global__ void __launch_bounds__(kThreads)
dedupe_retain_kernel(const uint64_t *__restrict__ old_state, const uint64_t *__restrict__ old_value, const uint64_t *__restrict__ old_key,
                     uint64_t old_cap, const uint32_t *__restrict__ live, uint64_t dir_base, uint64_t dir_entries, uint64_t *__restrict__ state,
                     uint64_t *__restrict__ value, uint64_t *__restrict__ key, uint64_t mask, unsigned long long *__restrict__ n_kept,
                     unsigned long long *__restrict__ err)
{
    uint32_t mine = 0; // (a lane sees at most old_cap / (gridDim.x * kThreads) + 1 < 2^32 slots)
    for (uint64_t o = (uint64_t)blockIdx.x * kThreads + threadIdx.x; o < old_cap; o += (uint64_t)gridDim.x * kThreads) {
        if (old_state[o] != kCommitted) continue;
        const uint64_t v = old_value[o], idx = v - dir_base;
        if (idx < dir_entries && live[idx] == 0) continue;
        mine++;
        if (!state) continue;
        uint64_t d[W];
        for (int w = 0; w < W; w++) d[w] = old_key[o * W + w];
        const uint64_t slot = claim_committed(state, d, mask);
        if (slot == kNoSlot) { *err = 1ull; continue; }
        for (int w = 0; w < W; w++) key[slot * W + w] = d[w];
        value[slot] = v;
    }
    __shared__ uint32_t wkept[kThreads / 64];
    for (int off = 32; off > 0; off >>= 1) mine += __shfl_down(mine, off, 64);
    if ((threadIdx.x & 63u) == 0) wkept[threadIdx.x >> 6] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t all = 0;
        for (uint32_t w = 0; w < kThreads / 64; w++) all += wkept[w];
        if (all) __hip_atomic_fetch_add(n_kept, (unsigned long long)all, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// ---- the digests behind a directory's flagged entries (cw_dev_dedupe_export_live) -----------------------
// The export with a filter and an order: the table maps digest -> value, this answers "the digests of the values live[] flags", in
// ascending value.  Three kernels, each behind a kernel boundary: flags[idx] = live[idx] != 0, whose index-only pack scan gives every
// flagged idx its rank; a fill that writes (CW_DEDUPE_MISS, zero digest) to every rank below max_out, so a flagged value the table
// lacks is answered without a second pass; one sweep of the table that places each committed entry with a flagged value at its rank.
__global__ void __launch_bounds__(kThreads)
dedupe_live_flags_kernel(const uint32_t *__restrict__ live, uint64_t dir_entries, uint32_t *__restrict__ flags)
{
    for (uint64_t idx = (uint64_t)blockIdx.x * kThreads + threadIdx.x; idx < dir_entries; idx += (uint64_t)gridDim.x * kThreads)
        flags[idx] = live[idx] != 0;
}

// result = {L, 0}: the sweep counts its hits into result[1]
template <int W>
__global__ void __launch_bounds__(kThreads)
dedupe_live_fill_kernel(const uint32_t *__restrict__ live, uint64_t dir_entries, const unsigned long long *__restrict__ rank, uint64_t max_out,
                        uint64_t *__restrict__ out_dig, uint64_t *__restrict__ out_val, uint64_t *__restrict__ result)
{
    for (uint64_t idx = (uint64_t)blockIdx.x * kThreads + threadIdx.x; idx < dir_entries; idx += (uint64_t)gridDim.x * kThreads) {
        const uint64_t k = rank[idx];
        if (live[idx] == 0 || k >= max_out) continue;
        out_val[k] = UINT64_MAX;
        for (int w = 0; w < W; w++) out_dig[k * W + w] = 0;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        result[0] = rank[dir_entries];
        result[1] = 0;
    }
}

// One lane per slot, plain loads of the table as in the lookup.  A hit claims its rank with one 64-bit CAS CW_DEDUPE_MISS -> value
// on out_val and only the claimant writes the digest: of two entries that carry the same flagged value, one digest is written whole.
// The hits are counted whether they claim or not, per workgroup as the retain counts.
template <int W>
__global__ void __launch_bounds__(kThreads)
dedupe_live_sweep_kernel(const uint64_t *__restrict__ state, const uint64_t *__restrict__ value, const uint64_t *__restrict__ key, uint64_t cap,
                         const uint32_t *__restrict__ live, uint64_t dir_base, uint64_t dir_entries, const unsigned long long *__restrict__ rank,
                         uint64_t max_out, uint64_t *__restrict__ out_dig, uint64_t *out_val, unsigned long long *__restrict__ n_hits)
{
    uint32_t mine = 0; // (a lane sees at most cap / (gridDim.x * kThreads) + 1 < 2^32 slots)
    for (uint64_t o = (uint64_t)blockIdx.x * kThreads + threadIdx.x; o < cap; o += (uint64_t)gridDim.x * kThreads) {
        if (state[o] != kCommitted) continue;
        const uint64_t v = value[o], idx = v - dir_base;
        if (idx >= dir_entries || live[idx] == 0) continue;
        mine++;
        const uint64_t k = rank[idx];
        if (k >= max_out) continue;
        uint64_t old = UINT64_MAX;
        __hip_atomic_compare_exchange_strong(out_val + k, &old, v, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (old != UINT64_MAX) continue; // another entry with this value came first
        for (int w = 0; w < W; w++) out_dig[k * W + w] = key[o * W + w];
    }
    __shared__ uint32_t whits[kThreads / 64];
    for (int off = 32; off > 0; off >>= 1) mine += __shfl_down(mine, off, 64);
    if ((threadIdx.x & 63u) == 0) whits[threadIdx.x >> 6] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t all = 0;
        for (uint32_t w = 0; w < kThreads / 64; w++) all += whits[w];
        if (all) __hip_atomic_fetch_add(n_hits, (unsigned long long)all, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// ---- the compare of a scrub window (cw_dev_store_verify) ------------------------------------------------
// One lane per slot, plain loads as above.  head = {c, n}: the window is the directory entries [c, c + n).  A committed slot whose
// value names entry c + k of the window, decoded (decoded[k] == 0), compares its key with the digest computed from the stored bytes
// and lowers verdict[k] -- ORPHAN (4) when the sweep starts -- with one atomic min: 0 on equality, else 3.  Of several slots that
// carry one value, a match by any of them leaves 0 whatever the order.  The table is only read.
template <int W>
__global__ void __launch_bounds__(kThreads)
dedupe_verify_sweep_kernel(const uint64_t *__restrict__ state, const uint64_t *__restrict__ value, const uint64_t *__restrict__ key, uint64_t cap,
                           uint64_t dir_base, const uint64_t *__restrict__ head, const uint32_t *__restrict__ decoded,
                           const uint64_t *__restrict__ dig, uint32_t *__restrict__ verdict)
{
    const uint64_t c = head[0], n = head[1];
    if (n == 0) return;
    for (uint64_t o = (uint64_t)blockIdx.x * kThreads + threadIdx.x; o < cap; o += (uint64_t)gridDim.x * kThreads) {
        if (state[o] != kCommitted) continue;
        const uint64_t idx = value[o] - dir_base, k = idx - c; // a value below the base, or an entry below the window, wraps out of range
        if (idx < c || k >= n || decoded[k] != 0) continue;
        bool eq = true;
        for (int w = 0; w < W; w++) eq &= key[o * W + w] == dig[k * W + w];
        __hip_atomic_fetch_min(verdict + k, eq ? 0u : 3u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// ---- values through a list of pairs (cw_dev_dedupe_revalue) ---------------------------------------------
// What translate_refs_kernel does to a recipe, done to value[]: the keys, the states and the count stay, so nothing is rehashed.  Two
// sweeps, one lane per slot, plain loads of state and value as in the lookup.  The count sweep looks every committed value up in the
// ascending from[0..np) with a binary search: a hit is a translation, a miss inside [range_base, range_base + range_entries) is
// stale; both are counted per workgroup as the retain counts.  Behind the kernel boundary the apply sweep does nothing when an entry
// is stale, else repeats the search and stores to[k] over the value -- plain stores: each slot is read and written by one lane, once,
// and the index serialises its calls.  Block 0's first thread reports.
// the pair that from[k] == v names, or np
__device__ __forceinline__ uint64_t revalue_find(const uint64_t *__restrict__ from, uint64_t np, uint64_t v)
{
    uint64_t lo = 0, hi = np; // the first pair with from >= v
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (from[mid] < v) lo = mid + 1;
        else hi = mid;
    }
    return lo < np && from[lo] == v ? lo : np;
}

__global__ void __launch_bounds__(kThreads)
dedupe_revalue_count_kernel(const uint64_t *__restrict__ state, const uint64_t *__restrict__ value, uint64_t cap,
                            const uint64_t *__restrict__ from, const uint64_t *__restrict__ d_npairs, uint64_t max_pairs, uint64_t range_base,
                            uint64_t range_entries, unsigned long long *__restrict__ head)
{
    const uint64_t np = umin64(*d_npairs, max_pairs);
    uint32_t hits = 0, stale = 0; // (a lane sees at most cap / (gridDim.x * kThreads) + 1 < 2^32 slots)
    for (uint64_t o = (uint64_t)blockIdx.x * kThreads + threadIdx.x; o < cap; o += (uint64_t)gridDim.x * kThreads) {
        if (state[o] != kCommitted) continue;
        const uint64_t v = value[o];
        if (revalue_find(from, np, v) < np) hits++;
        else if (v - range_base < range_entries) stale++; // a value below the base wraps out of range
    }
    __shared__ uint32_t whits[kThreads / 64], wstale[kThreads / 64];
    for (int off = 32; off > 0; off >>= 1) {
        hits += __shfl_down(hits, off, 64);
        stale += __shfl_down(stale, off, 64);
    }
    if ((threadIdx.x & 63u) == 0) {
        whits[threadIdx.x >> 6] = hits;
        wstale[threadIdx.x >> 6] = stale;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    uint32_t h = 0, s = 0;
    for (uint32_t w = 0; w < kThreads / 64; w++) {
        h += whits[w];
        s += wstale[w];
    }
    if (h) __hip_atomic_fetch_add(head, (unsigned long long)h, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (s) __hip_atomic_fetch_add(head + 1, (unsigned long long)s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ void __launch_bounds__(kThreads)
dedupe_revalue_apply_kernel(const uint64_t *__restrict__ state, uint64_t *__restrict__ value, uint64_t cap, const uint64_t *__restrict__ from,
                            const uint64_t *__restrict__ to, const uint64_t *__restrict__ d_npairs, uint64_t max_pairs,
                            const unsigned long long *__restrict__ head, uint64_t *__restrict__ result)
{
    const uint64_t n_hits = head[0], n_stale = head[1];
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        result[0] = n_stale != 0;
        result[1] = n_hits;
        result[2] = n_stale;
    }
    if (n_stale != 0 || n_hits == 0) return;
    const uint64_t np = umin64(*d_npairs, max_pairs);
    for (uint64_t o = (uint64_t)blockIdx.x * kThreads + threadIdx.x; o < cap; o += (uint64_t)gridDim.x * kThreads) {
        if (state[o] != kCommitted) continue;
        const uint64_t k = revalue_find(from, np, value[o]);
        if (k < np) value[o] = to[k];
    }
}

unsigned grid_of(uint32_t n) { return (n + kThreads - 1) / kThreads; }
// grid-stride kernels over `tiles` tiles of kThreads slots
unsigned grid_stride_of(uint64_t tiles) { return (unsigned)(tiles < (1u << 20) ? tiles : (1u << 20)); }

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

hipError_t dedupe_resolve_launch(unsigned words, const uint64_t *dig, uint32_t n, uint64_t base, const uint64_t *values, const uint32_t *min_idx,
                                 uint64_t *state, uint64_t *value, uint64_t *key, const uint64_t *rec, uint64_t *ref, uint32_t *flags, hipStream_t s)
{
    const dim3 g(grid_of(n)), b(kThreads);
#define CW_RESOLVE(W, V) hipLaunchKernelGGL((dedupe_resolve_kernel<W, V>), g, b, 0, s, dig, n, base, values, min_idx, state, value, key, rec, ref, flags)
    switch (words) {
    case 2: if (values) CW_RESOLVE(2, true); else CW_RESOLVE(2, false); break;
    case 4: if (values) CW_RESOLVE(4, true); else CW_RESOLVE(4, false); break;
    case 8: if (values) CW_RESOLVE(8, true); else CW_RESOLVE(8, false); break;
    default: return hipErrorInvalidValue;
    }
#undef CW_RESOLVE
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

hipError_t dedupe_lookup_launch(unsigned words, const uint64_t *dig, uint32_t n, const uint64_t *state, const uint64_t *value, const uint64_t *key,
                                uint64_t mask, uint64_t *ref, uint64_t *n_found, unsigned long long *err, hipStream_t s)
{
    hipError_t e = hipMemsetAsync(n_found, 0, sizeof(uint64_t), s);
    if (e != hipSuccess) return e;
    const dim3 g(grid_of(n)), b(kThreads);
    unsigned long long *nf = reinterpret_cast<unsigned long long *>(n_found);
    switch (words) {
    case 2: hipLaunchKernelGGL(dedupe_lookup_kernel<2>, g, b, 0, s, dig, n, state, value, key, mask, ref, nf, err); break;
    case 4: hipLaunchKernelGGL(dedupe_lookup_kernel<4>, g, b, 0, s, dig, n, state, value, key, mask, ref, nf, err); break;
    case 8: hipLaunchKernelGGL(dedupe_lookup_kernel<8>, g, b, 0, s, dig, n, state, value, key, mask, ref, nf, err); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

uint64_t dedupe_export_tiles(uint64_t cap) { return (cap + kThreads - 1) / kThreads; }

hipError_t dedupe_export_scan_launch(const uint64_t *state, uint64_t cap, uint32_t *counts, uint64_t *offs, hipStream_t s)
{
    const uint64_t ntiles = dedupe_export_tiles(cap);
    hipLaunchKernelGGL(dedupe_export_count_kernel, dim3(grid_stride_of(ntiles)), dim3(kThreads), 0, s, state, cap, ntiles, counts);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? pack_launch(nullptr, 0, counts, ntiles, nullptr, offs, s) : e;
}

hipError_t dedupe_export_scatter_launch(unsigned words, const uint64_t *state, const uint64_t *value, const uint64_t *key, uint64_t cap,
                                        const uint64_t *offs, uint64_t first, uint64_t max_out, uint64_t *out_dig, uint64_t *out_val, uint64_t *d_n,
                                        hipStream_t s)
{
    const uint64_t ntiles = dedupe_export_tiles(cap);
    const dim3 g(grid_stride_of(ntiles)), b(kThreads);
    const unsigned long long *off = reinterpret_cast<const unsigned long long *>(offs);
    const bool vec = (reinterpret_cast<uintptr_t>(out_dig) & 15) == 0;
    switch (words) {
    case 2: hipLaunchKernelGGL(dedupe_export_scatter_kernel<2>, g, b, 0, s, state, value, key, cap, ntiles, off, first, max_out, out_dig, out_val, d_n, vec); break;
    case 4: hipLaunchKernelGGL(dedupe_export_scatter_kernel<4>, g, b, 0, s, state, value, key, cap, ntiles, off, first, max_out, out_dig, out_val, d_n, vec); break;
    case 8: hipLaunchKernelGGL(dedupe_export_scatter_kernel<8>, g, b, 0, s, state, value, key, cap, ntiles, off, first, max_out, out_dig, out_val, d_n, vec); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// flags[dir_entries] (u32) and rank[dir_entries + 1] are the caller's scratch; result[2] = {flagged entries, table entries with a flagged value}
hipError_t dedupe_export_live_launch(unsigned words, const uint64_t *state, const uint64_t *value, const uint64_t *key, uint64_t cap,
                                     const uint32_t *live, uint64_t dir_base, uint64_t dir_entries, uint32_t *flags, uint64_t *rank, uint64_t max_out,
                                     uint64_t *out_dig, uint64_t *out_val, uint64_t *result, hipStream_t s)
{
    const dim3 g(grid_stride_of(dedupe_export_tiles(dir_entries))), gt(grid_stride_of(dedupe_export_tiles(cap))), b(kThreads);
    hipLaunchKernelGGL(dedupe_live_flags_kernel, g, b, 0, s, live, dir_entries, flags);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || (e = pack_launch(nullptr, 0, flags, dir_entries, nullptr, rank, s)) != hipSuccess) return e;
    const unsigned long long *r = reinterpret_cast<const unsigned long long *>(rank);
    unsigned long long *hits = reinterpret_cast<unsigned long long *>(result + 1);
#define CW_LIVE(W)                                                                                                                                \
    hipLaunchKernelGGL(dedupe_live_fill_kernel<W>, g, b, 0, s, live, dir_entries, r, max_out, out_dig, out_val, result);                         \
    hipLaunchKernelGGL(dedupe_live_sweep_kernel<W>, gt, b, 0, s, state, value, key, cap, live, dir_base, dir_entries, r, max_out, out_dig, out_val, hits)
    switch (words) {
    case 2: CW_LIVE(2); break;
    case 4: CW_LIVE(4); break;
    case 8: CW_LIVE(8); break;
    default: return hipErrorInvalidValue;
    }
#undef CW_LIVE
    return hipGetLastError();
}

hipError_t dedupe_verify_launch(unsigned words, const uint64_t *state, const uint64_t *value, const uint64_t *key, uint64_t cap, uint64_t dir_base,
                                const uint64_t *head, const uint32_t *decoded, const uint64_t *digests, uint32_t *verdict, hipStream_t s)
{
    const dim3 g(grid_stride_of(dedupe_export_tiles(cap))), b(kThreads);
    switch (words) {
    case 2: hipLaunchKernelGGL(dedupe_verify_sweep_kernel<2>, g, b, 0, s, state, value, key, cap, dir_base, head, decoded, digests, verdict); break;
    case 4: hipLaunchKernelGGL(dedupe_verify_sweep_kernel<4>, g, b, 0, s, state, value, key, cap, dir_base, head, decoded, digests, verdict); break;
    case 8: hipLaunchKernelGGL(dedupe_verify_sweep_kernel<8>, g, b, 0, s, state, value, key, cap, dir_base, head, decoded, digests, verdict); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t dedupe_rehash_launch(unsigned words, const uint64_t *old_state, const uint64_t *old_value, const uint64_t *old_key, uint64_t old_cap,
                                uint64_t *state, uint64_t *value, uint64_t *key, uint64_t mask, unsigned long long *err, hipStream_t s)
{
    const dim3 g(grid_stride_of(dedupe_export_tiles(old_cap))), b(kThreads);
    switch (words) {
    case 2: hipLaunchKernelGGL(dedupe_rehash_kernel<2>, g, b, 0, s, old_state, old_value, old_key, old_cap, state, value, key, mask, err); break;
    case 4: hipLaunchKernelGGL(dedupe_rehash_kernel<4>, g, b, 0, s, old_state, old_value, old_key, old_cap, state, value, key, mask, err); break;
    case 8: hipLaunchKernelGGL(dedupe_rehash_kernel<8>, g, b, 0, s, old_state, old_value, old_key, old_cap, state, value, key, mask, err); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// state == NULL: *n_kept += the entries the keep rule keeps, nothing is written; else they are rehashed as well
hipError_t dedupe_retain_launch(unsigned words, const uint64_t *old_state, const uint64_t *old_value, const uint64_t *old_key, uint64_t old_cap,
                                const uint32_t *live, uint64_t dir_base, uint64_t dir_entries, uint64_t *state, uint64_t *value, uint64_t *key,
                                uint64_t mask, unsigned long long *n_kept, unsigned long long *err, hipStream_t s)
{
    const dim3 g(grid_stride_of(dedupe_export_tiles(old_cap))), b(kThreads);
#define CW_RETAIN(W) hipLaunchKernelGGL(dedupe_retain_kernel<W>, g, b, 0, s, old_state, old_value, old_key, old_cap, live, dir_base, dir_entries, state, value, key, mask, n_kept, err)
    switch (words) {
    case 2: CW_RETAIN(2); break;
    case 4: CW_RETAIN(4); break;
    case 8: CW_RETAIN(8); break;
    default: return hipErrorInvalidValue;
    }
#undef CW_RETAIN
    return hipGetLastError();
}

hipError_t dedupe_revalue_launch(const uint64_t *state, uint64_t *value, uint64_t cap, const uint64_t *from, const uint64_t *to,
                                 const uint64_t *d_npairs, uint64_t max_pairs, uint64_t range_base, uint64_t range_entries, uint64_t *head,
                                 uint64_t *result, hipStream_t s)
{
    const hipError_t e = hipMemsetAsync(head, 0, 2 * sizeof(uint64_t), s);
    if (e != hipSuccess) return e;
    const dim3 g(grid_stride_of(dedupe_export_tiles(cap))), b(kThreads);
    unsigned long long *h = reinterpret_cast<unsigned long long *>(head);
    hipLaunchKernelGGL(dedupe_revalue_count_kernel, g, b, 0, s, state, value, cap, from, d_npairs, max_pairs, range_base, range_entries, h);
    hipLaunchKernelGGL(dedupe_revalue_apply_kernel, g, b, 0, s, state, value, cap, from, to, d_npairs, max_pairs, h, result);
    return hipGetLastError();
}

} // namespace cw
