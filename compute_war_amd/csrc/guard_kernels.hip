// guard_kernels.hip -- XOR guard stripes over the store's bytes (semantics: the public header's
// cw_dev_store_guard_update, _check and _rebuild).  With S = stripe, G = group and W = G * S, store byte p lies in stripe p / S, which is
// member (p / S) % G of group p / W, at column p % S; guard[g * S + c] is the XOR of the bytes of group g at column c below the
// cursor `covered`.  S is a multiple of 16 and both buffers are 16-byte aligned, so a 16-byte guard word and the G store words it
// sums never straddle a stripe.
//
// Update: a lane per guard word that [from, to) = [*d_covered, *d_used) touches.  Only the first and the last group of the range can
// be touched in part; a group touched in fewer than S / 16 words names them by their first column, wrapping at S.  The lane loads the
// members' words that lie whole in the range one after the other with nothing between them, masks the at most two that the range
// cuts, and does one read-modify-write: no two lanes own the same word, so there are no atomics.  A second kernel moves the cursor and
// reports: everything the first one wrote lies behind a kernel boundary when `covered` changes.
// Check: a lane per guard word of the groups below the cursor, the same sum over [0, covered) compared with the word; a flag per group
// in the scratch, counted and copied out by one workgroup.
// Rebuild: an extent of at most 65536 <= S bytes crosses at most one stripe boundary, so it is at most two PIECES, each in one stripe:
// (group, member, columns [c0, c1)).  Two pieces collide iff they share the group, differ in the member and their columns overlap --
// then some byte of the one meets another byte of the other in a guard byte.  Pieces of one extent never do (their columns are
// [c, S) and [0, c') with c' <= c), nor do pieces of a value named twice (same member), so the test needs no position.  The pieces
// are counting-sorted by group (count -> scan -> scatter) and a position tests its pieces against their own groups' buckets only.
// A wavefront per rebuilt position then sums guard and members in aligned 4-byte words.
//
// Scratch, per stream: check 64 + 4 * N bytes, rebuild 80 + 28 * max_count + 16 * N bytes, N = the groups of store_bytes.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cw_device.h"
#include "guard_device.h"
#include "store_device.h"

namespace cw {

namespace {

using namespace chunkstore;
using namespace guardstripes; // the geometry, the members' sum, pieces, positions and verdicts: guard_device.h

// ---- update --------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kThreads)
guard_fold_kernel(const uint8_t *__restrict__ store, uint64_t store_bytes, const uint64_t *__restrict__ d_used, const uint64_t *__restrict__ d_covered,
                  Geometry geo, uint4 *__restrict__ guard)
{
    const uint64_t from = *d_covered, to = *d_used;
    if (update_verdict(from, to, store_bytes) || from == to) return;
    const uint64_t g0 = from / geo.W, g1 = (to - 1) / geo.W, words = geo.words();
    uint64_t first0, n0, first1 = 0, n1 = 0;
    touched(geo, g0, from, to, first0, n0);
    if (g1 > g0) touched(geo, g1, from, to, first1, n1);
    const uint64_t mid = g1 > g0 ? (g1 - g0 - 1) * words : 0, total = n0 + mid + n1, threads = (uint64_t)gridDim.x * kThreads;
    for (uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x; i < total; i += threads) {
        uint64_t g, cw;
        if (i < n0) {
            g = g0;
            cw = (first0 + i) & (words - 1);
        } else if (i - n0 < mid) {
            g = g0 + 1 + ((i - n0) >> (geo.shift - 4));
            cw = (i - n0) & (words - 1);
        } else {
            g = g1;
            cw = (first1 + (i - n0 - mid)) & (words - 1);
        }
        const uint4 sum = members_sum(store, geo, g * geo.W + (cw << 4), from, to);
        uint4 *word = guard + g * words + cw;
        *word = *word ^ sum;
    }
}

// one thread, behind the fold: the cursor and the result
__global__ void __launch_bounds__(64)
guard_update_finish_kernel(uint64_t store_bytes, const uint64_t *__restrict__ d_used, uint64_t *__restrict__ d_covered, uint64_t *__restrict__ result)
{
    if (threadIdx.x == 0) update_finish(store_bytes, d_used, d_covered, result);
}

// ---- check ---------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kThreads)
guard_compare_kernel(const uint8_t *__restrict__ store, uint64_t store_bytes, const uint64_t *__restrict__ d_covered, Geometry geo,
                     const uint4 *__restrict__ guard, uint32_t *__restrict__ flags)
{
    const uint64_t covered = *d_covered;
    if (covered > store_bytes) return;
    const uint64_t words = geo.words(), total = (covered + geo.W - 1) / geo.W * words, threads = (uint64_t)gridDim.x * kThreads;
    for (uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x; i < total; i += threads) {
        const uint64_t g = i >> (geo.shift - 4), cw = i & (words - 1);
        if (differ(members_sum(store, geo, g * geo.W + (cw << 4), 0, covered), guard[i])) flags[g] = 1u; // (every writer writes 1)
    }
}

// one workgroup: the flags counted and copied out
__global__ void __launch_bounds__(kThreads)
guard_check_finish_kernel(uint64_t store_bytes, const uint64_t *__restrict__ d_covered, Geometry geo, const uint32_t *__restrict__ flags,
                          uint32_t *__restrict__ group_bad, uint64_t *__restrict__ result)
{
    __shared__ uint64_t wsum[kThreads / 64];
    __shared__ unsigned long long lowest;
    const uint64_t covered = *d_covered;
    const bool ok = covered <= store_bytes;
    const uint64_t groups = ok ? (covered + geo.W - 1) / geo.W : 0;
    if (threadIdx.x == 0) lowest = ~0ull;
    __syncthreads();
    uint64_t bad = 0, low = ~0ull;
    for (uint64_t g = threadIdx.x; g < groups; g += kThreads) {
        const uint32_t f = flags[g];
        if (group_bad) group_bad[g] = f;
        if (f && low == ~0ull) low = g;
        bad += f;
    }
    if (low != ~0ull) atomicMin(&lowest, (unsigned long long)low);
    const uint64_t all = group_sum<uint64_t>(bad, wsum); // (its barriers also order the atomicMin in front of the read below)
    if (threadIdx.x != 0) return;
    result[0] = ok ? 0 : 1;
    result[1] = groups;
    result[2] = all;
    result[3] = lowest;
}

// ---- rebuild -------------------------------------------------------------------------------------------------------------------------
// count[g] += the pieces of the protected positions in group g; the head
__global__ void __launch_bounds__(kThreads)
rebuild_count_kernel(Positions P, Geometry geo, uint64_t groups, uint32_t *__restrict__ count, RebuildHead *__restrict__ head)
{
    rebuild_count(P, geo, groups, count, head);
}

// sorted[first[g] ..) = the pieces of group g, in any order
__global__ void __launch_bounds__(kThreads)
rebuild_scatter_kernel(Positions P, Geometry geo, const unsigned long long *__restrict__ first, uint32_t *__restrict__ cursor, uint2 *__restrict__ sorted)
{
    rebuild_scatter(P, geo, first, cursor, sorted);
}

// a piece of another member of the same group with a column in common
__device__ __forceinline__ bool collides(const Piece &p, const unsigned long long *__restrict__ first, const uint2 *__restrict__ sorted)
{
    for (uint64_t j = first[p.g], e = first[p.g + 1]; j < e; j++) {
        const uint2 o = sorted[j];
        const uint32_t m = o.y >> 24, len = o.y & 0xFFFFFFu;
        if (m != p.m && o.x < p.c0 + p.len && p.c0 < o.x + len) return true;
    }
    return false;
}

// status[k], sizes[k] = the stored bytes of a position that will be rebuilt, else 0; head->rebuilt
__global__ void __launch_bounds__(kThreads)
rebuild_status_kernel(Positions P, Geometry geo, const unsigned long long *__restrict__ first, const uint2 *__restrict__ sorted,
                      uint32_t *__restrict__ sizes, uint32_t *__restrict__ status, RebuildHead *__restrict__ head)
{
    __shared__ uint32_t wsum[kThreads / 64];
    const uint64_t n = P.n(), cov = P.covered(), threads = (uint64_t)gridDim.x * kThreads;
    uint32_t rebuilt = 0; // (a thread sees at most max_count / threads + 1 < 2^32 positions)
    for (uint64_t k = (uint64_t)blockIdx.x * kThreads + threadIdx.x; k < n; k += threads) {
        uint64_t pos;
        uint32_t stored, s = 2;
        uint4 raw;
        if (P.is_protected(k, cov, pos, stored, raw)) {
            Piece p[2];
            pieces_of(geo, pos, stored, p);
            s = collides(p[0], first, sorted) || (p[1].len && collides(p[1], first, sorted)) ? 1u : 0u;
        }
        status[k] = s;
        sizes[k] = s == 0 ? stored : 0u;
        rebuilt += s == 0;
    }
    const uint32_t all = group_sum(rebuilt, wsum);
    if (threadIdx.x == 0 && all) __hip_atomic_fetch_add(&head->rebuilt, (unsigned long long)all, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// a wavefront per position: a rebuilt extent to out + off[k], byte = guard byte ^ the other members' bytes below the cursor; out_loc[k]
__global__ void __launch_bounds__(64)
rebuild_copy_kernel(const uint8_t *__restrict__ store, Positions P, Geometry geo, const uint8_t *__restrict__ guard,
                    const unsigned long long *__restrict__ off, const uint32_t *__restrict__ status, const RebuildHead *__restrict__ head,
                    uint8_t *__restrict__ out, uint64_t out_bytes, uint4 *__restrict__ out_loc)
{
    const uint64_t n = P.n(), cov = P.covered();
    if (rebuild_verdict(head, off[n], out_bytes)) return;
    for (uint64_t k = blockIdx.x; k < n; k += gridDim.x) {
        uint64_t pos;
        uint32_t stored;
        uint4 raw;
        if (status[k] != 0 || !P.is_protected(k, cov, pos, stored, raw)) { // (a position with status 0 is protected)
            if (threadIdx.x == 0) out_loc[k] = make_uint4(0, 0, 0, 0);
            continue;
        }
        const uint64_t to = off[k], end = pos + stored, t0 = pos >> geo.shift, g0 = t0 / geo.G;
        const uint32_t m0 = (uint32_t)(t0 - g0 * geo.G);
        for (uint64_t q = (pos & ~3ull) + 4 * threadIdx.x; q < end; q += 4 * 64) {
            // the word's stripe is the extent's first or the one behind it
            const bool next = (q >> geo.shift) != t0, wraps = next && m0 + 1 == geo.G;
            const uint64_t g = wraps ? g0 + 1 : g0, c = q & (geo.S - 1), base = g * geo.W + c;
            const uint32_t self = wraps ? 0u : m0 + next;
            uint32_t v = *reinterpret_cast<const uint32_t *>(guard + g * geo.S + c);
#pragma unroll 4
            for (uint32_t m = 0; m < geo.G; m++) {
                const uint64_t p = base + ((uint64_t)m << geo.shift);
                if (p >= cov) break;
                if (m != self) v ^= word_below(store, p, cov);
            }
#pragma unroll
            for (uint32_t i = 0; i < 4; i++)
                if (q + i >= pos && q + i < end) out[to + (q + i - pos)] = (uint8_t)(v >> (8 * i));
        }
        if (threadIdx.x == 0) out_loc[k] = Entry(raw).at(to);
    }
}

__global__ void __launch_bounds__(64)
rebuild_finish_kernel(Positions P, const unsigned long long *__restrict__ off, const RebuildHead *__restrict__ head, uint64_t out_bytes,
                      uint64_t *__restrict__ result)
{
    if (threadIdx.x != 0) return;
    const uint64_t n = P.n(), total = off[n];
    result[0] = rebuild_verdict(head, total, out_bytes);
    result[1] = total;
    result[2] = n;
    result[3] = head->rebuilt;
}

// per stream: check's flags behind a 64-byte head; rebuild's layout in store_guard_rebuild_launch
StreamScratch<DeviceBuf> guard_spaces;
static_assert(sizeof(RebuildHead) <= kScratchHead, "the head holds the three words");

} // namespace

size_t store_guard_groups(size_t store_bytes, size_t stripe, unsigned group)
{
    const size_t w = stripe * group;
    return store_bytes / w + (store_bytes % w != 0);
}

size_t store_guard_check_scratch_bytes(size_t groups) { return kScratchHead + 4 * groups; }
size_t store_guard_rebuild_scratch_bytes(size_t max_count, size_t groups) { return kScratchHead + 16 + 28 * max_count + 16 * groups; }

hipError_t store_guard_update_launch(const uint8_t *store, size_t store_bytes, const uint64_t *d_used, uint64_t *d_covered, size_t stripe,
                                     unsigned group, void *guard, uint64_t *result, hipStream_t stream)
{
    const Geometry geo = geometry(stripe, group);
    const size_t words = store_guard_groups(store_bytes, stripe, group) * (stripe / 16);
    if (words)
        hipLaunchKernelGGL(guard_fold_kernel, dim3(lane_grid(words)), dim3(kThreads), 0, stream, store, (uint64_t)store_bytes, d_used, d_covered, geo,
                           static_cast<uint4 *>(guard));
    hipLaunchKernelGGL(guard_update_finish_kernel, dim3(1), dim3(64), 0, stream, (uint64_t)store_bytes, d_used, d_covered, result);
    return hipGetLastError();
}

hipError_t store_guard_check_launch(const uint8_t *store, size_t store_bytes, const uint64_t *d_covered, size_t stripe, unsigned group,
                                    const void *guard, uint32_t *group_bad, uint64_t *result, hipStream_t stream)
{
    const Geometry geo = geometry(stripe, group);
    const size_t groups = store_guard_groups(store_bytes, stripe, group);
    auto &w = guard_spaces.at(stream);
    LaunchLock sequence(w.launch); // the flags are shared by the launches below
    hipError_t e = w.reserve(store_guard_check_scratch_bytes(groups), (size_t)1 << 20);
    if (e != hipSuccess) return e;
    uint32_t *flags = reinterpret_cast<uint32_t *>(w.as<uint8_t>() + kScratchHead);
    if (groups) {
        if ((e = hipMemsetAsync(flags, 0, 4 * groups, stream)) != hipSuccess) return e;
        hipLaunchKernelGGL(guard_compare_kernel, dim3(lane_grid(groups * (stripe / 16))), dim3(kThreads), 0, stream, store, (uint64_t)store_bytes,
                           d_covered, geo, static_cast<const uint4 *>(guard), flags);
    }
    hipLaunchKernelGGL(guard_check_finish_kernel, dim3(1), dim3(kThreads), 0, stream, (uint64_t)store_bytes, d_covered, geo, flags, group_bad, result);
    return hipGetLastError();
}

hipError_t store_guard_rebuild_launch(const uint8_t *store, size_t store_bytes, const void *dir, uint64_t dir_base, size_t dir_entries,
                                      const uint64_t *d_covered, size_t stripe, unsigned group, const void *guard, const uint64_t *values,
                                      const uint64_t *d_count, size_t max_count, uint8_t *out, size_t out_bytes, void *out_loc, uint32_t *status,
                                      uint64_t *result, hipStream_t stream)
{
    const Geometry geo = geometry(stripe, group);
    const size_t groups = store_guard_groups(store_bytes, stripe, group), n = max_count;
    auto &w = guard_spaces.at(stream);
    LaunchLock sequence(w.launch); // the head and the arrays are shared by the launches below
    hipError_t e = w.reserve(store_guard_rebuild_scratch_bytes(n, groups), (size_t)1 << 20);
    if (e != hipSuccess) return e;
    // the head; two scans -- the positions' sizes and the groups' piece counts -- each as a ScanScratch; the sorted pieces; the cursors
    ScanScratch pos, grp;
    pos.head = grp.head = w.as<uint8_t>();
    pos.off = reinterpret_cast<uint64_t *>(pos.head + kScratchHead);
    grp.off = pos.off + n + 1;
    uint2 *sorted = reinterpret_cast<uint2 *>(grp.off + groups + 1);
    pos.sizes = reinterpret_cast<uint32_t *>(sorted + 2 * n);
    grp.sizes = pos.sizes + n;
    uint32_t *cursor = grp.sizes + groups;
    RebuildHead *head = pos.head_as<RebuildHead>();
    if ((e = hipMemsetAsync(head, 0, kScratchHead, stream)) != hipSuccess) return e;
    if (groups && (e = hipMemsetAsync(grp.sizes, 0, 8 * groups, stream)) != hipSuccess) return e; // the counts and the cursors
    const Positions P{static_cast<const uint4 *>(dir), dir_base, (uint64_t)dir_entries, (uint64_t)store_bytes, values, d_count, (uint64_t)n, d_covered};
    const dim3 g(lane_grid(n ? n : 1)), b(kThreads);
    hipLaunchKernelGGL(rebuild_count_kernel, g, b, 0, stream, P, geo, (uint64_t)groups, grp.sizes, head);
    // first[g] = the pieces of the groups below g
    if ((e = chunk_pack_launch(0, nullptr, nullptr, nullptr, reinterpret_cast<const uint64_t *>(&head->groups), groups, grp.sizes, nullptr, grp.off,
                               stream)) != hipSuccess)
        return e;
    if (n) {
        hipLaunchKernelGGL(rebuild_scatter_kernel, g, b, 0, stream, P, geo, grp.offsets(), cursor, sorted);
        hipLaunchKernelGGL(rebuild_status_kernel, g, b, 0, stream, P, geo, grp.offsets(), sorted, pos.sizes, status, head);
    }
    // off[k] = the rebuilt bytes of the positions below k
    if ((e = chunk_pack_launch(0, nullptr, nullptr, nullptr, d_count, n, pos.sizes, nullptr, pos.off, stream)) != hipSuccess) return e;
    if (n)
        hipLaunchKernelGGL(rebuild_copy_kernel, dim3(wave_grid(n)), dim3(64), 0, stream, store, P, geo, static_cast<const uint8_t *>(guard), pos.offsets(),
                           status, head, out, (uint64_t)out_bytes, static_cast<uint4 *>(out_loc));
    hipLaunchKernelGGL(rebuild_finish_kernel, dim3(1), dim3(64), 0, stream, P, pos.offsets(), head, (uint64_t)out_bytes, result);
    return hipGetLastError();
}

} // namespace cw
