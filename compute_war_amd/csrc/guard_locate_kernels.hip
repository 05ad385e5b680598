// guard_locate_kernels.hip -- which directory entries the guard's syndromes suspect (semantics: the public
// header's cw_dev_store_guard_locate and cw_dev_store_guard2_locate).  Geometry and sums are guard_sums.h's.  A CELL is one guard byte:
// group g, column c.  P' = the guard byte XOR its members' store bytes below the cursor, Q' the same for the second syndrome.  A cell
// is dirty when P' != 0 (dual: or Q' != 0).  One wrong store byte, in member m, gives Q' = 2^m (x) P' -- so a dirty cell of a dual
// guard with P' != 0, Q' != 0 and log2(Q' / P') = m < the cell's members below the cursor is LOCATED(m); every other dirty cell is
// AMBIGUOUS (a single guard's always; a guard byte of its own; two or more wrong bytes).
//
// Sweep: a lane per 16-byte guard word of the groups below the cursor, exactly guard_compare_kernel's sums.  A wavefront's 64 words
// are neighbours (the words of a group are a multiple of 64), so one ballot is their 64 dirty bits and lane 0 stores it: every bitmap
// word below the cursor is written, nothing is zeroed and there are no atomics on the bitmap.  A lane with a dirty word classifies its
// 16 cells for the counts.
// Entries: a lane per directory entry.  A protected extent is at most two pieces, each inside one stripe, whose guard words are
// neighbours in the bitmap: the lane walks the bitmap 64 bits at a time and only for a set bit recomputes the word's sums and
// classifies the bytes of its own extent in it.  Dirty words are rare, so the walk is one bitmap load per 1024 stored bytes.
// log2 comes from exp / log tables in LDS, built by repeated doubling at kernel start as the dual rebuild builds them; the single
// guard's instantiations hold no tables.  A finish kernel of one thread writes d_result.
//
// Scratch, per stream: 64 + ceil(store_bytes / W) * S / 128 bytes -- the counters, zeroed in-stream, and a bit per guard word.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cw_device.h"
#include "guard_sums.h"
#include "store_device.h"

namespace cw {

namespace {

using namespace chunkstore;
using namespace guardsums;

struct LocateHead { // the first 40 of the scratch's 64 head bytes
    unsigned long long dirty, located, ambiguous, suspects, unjudged;
};
static_assert(sizeof(LocateHead) <= kScratchHead, "the head holds the five counters");

// gf_log[2^i] = i for i < 255, by repeated doubling; every lane walks the powers and writes its share
__device__ __forceinline__ void build_log(uint8_t *gf_log)
{
    uint32_t x = 1;
    for (uint32_t i = 0; i < 255; i++) {
        if ((i & (kThreads - 1)) == threadIdx.x) gf_log[x] = (uint8_t)i;
        x = xtime(x) & 0xFFu;
    }
    if (threadIdx.x == 0) gf_log[0] = 0; // (never indexed: zero is tested for)
    __syncthreads();
}

constexpr uint32_t kClean = 0x100u, kAmbiguous = 0x101u; // a cell's class; a value below 256 is LOCATED(that member)

// the class of a cell with the differences pb, qb and `members` members below the cursor
template <bool Dual>
__device__ __forceinline__ uint32_t classify(uint32_t pb, uint32_t qb, uint32_t members, const uint8_t *gf_log)
{
    if constexpr (!Dual) return pb ? kAmbiguous : kClean;
    else {
        if ((pb | qb) == 0) return kClean;
        if (pb == 0 || qb == 0) return kAmbiguous;
        const uint32_t lq = gf_log[qb], lp = gf_log[pb], k = lq >= lp ? lq - lp : lq + 255u - lp;
        return k < members ? k : kAmbiguous;
    }
}

// the members m < G of column c of group g with g * W + m * S + c < covered
__device__ __forceinline__ uint32_t members_below(const Geometry &geo, uint64_t at, uint64_t covered)
{
    return at >= covered ? 0u : (uint32_t)umin64(geo.G, ((covered - 1 - at) >> geo.shift) + 1);
}

// P' and Q' of guard word i = (group g, column word cw)
template <bool Dual>
__device__ __forceinline__ Sums differences(const uint8_t *__restrict__ store, const Geometry &geo, uint64_t g, uint64_t cw, uint64_t covered,
                                            const uint4 *__restrict__ guard_p, const uint4 *__restrict__ guard_q)
{
    const uint64_t i = g * geo.words() + cw;
    Sums s = members_sums<Dual>(store, geo, g * geo.W + (cw << 4), 0, covered);
    s.p = s.p ^ guard_p[i];
    if constexpr (Dual) s.q = s.q ^ guard_q[i];
    return s;
}

__device__ __forceinline__ uint32_t byte_of(const uint4 w, uint32_t b) // b is a constant after unrolling
{
    const uint32_t d = b < 4 ? w.x : b < 8 ? w.y : b < 12 ? w.z : w.w;
    return (d >> (8 * (b & 3u))) & 0xFFu;
}

// ---- the sweep -----------------------------------------------------------------------------------------------------------------------
template <bool Dual>
__global__ void __launch_bounds__(kThreads)
locate_sweep_kernel(const uint8_t *__restrict__ store, uint64_t store_bytes, const uint64_t *__restrict__ d_covered, Geometry geo,
                    const uint4 *__restrict__ guard_p, const uint4 *__restrict__ guard_q, unsigned long long *__restrict__ bitmap,
                    LocateHead *__restrict__ head)
{
    __shared__ uint8_t gf_log[Dual ? 256 : 1];
    __shared__ uint64_t wsum[kThreads / 64];
    const uint64_t covered = *d_covered;
    if (covered > store_bytes) return;
    if constexpr (Dual) build_log(gf_log);
    const uint64_t words = geo.words(), total = (covered + geo.W - 1) / geo.W * words, threads = (uint64_t)gridDim.x * kThreads;
    uint64_t dirty = 0, located = 0;
    // (total is a multiple of 64 and a wavefront's first i is one, so a wavefront is in the loop with all its lanes or with none)
    for (uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x; i < total; i += threads) {
        const uint64_t g = i >> (geo.shift - 4), cw = i & (words - 1);
        const Sums d = differences<Dual>(store, geo, g, cw, covered, guard_p, guard_q);
        bool any = differ(d.p, make_uint4(0, 0, 0, 0));
        if constexpr (Dual) any = any || differ(d.q, make_uint4(0, 0, 0, 0));
        const unsigned long long bits = __ballot(any);
        if ((threadIdx.x & 63u) == 0) bitmap[i >> 6] = bits;
        if (!any) continue;
        const uint64_t at = g * geo.W + (cw << 4);
#pragma unroll
        for (uint32_t b = 0; b < 16; b++) {
            const uint32_t c = classify<Dual>(byte_of(d.p, b), byte_of(d.q, b), members_below(geo, at + b, covered), gf_log);
            dirty += c != kClean;
            located += c < kClean;
        }
    }
    const uint64_t all_dirty = group_sum<uint64_t>(dirty, wsum), all_located = group_sum<uint64_t>(located, wsum);
    if (threadIdx.x != 0 || all_dirty == 0) return;
    __hip_atomic_fetch_add(&head->dirty, (unsigned long long)all_dirty, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_fetch_add(&head->ambiguous, (unsigned long long)(all_dirty - all_located), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (all_located) __hip_atomic_fetch_add(&head->located, (unsigned long long)all_located, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- the entries ---------------------------------------------------------------------------------------------------------------------
// The bits of the bytes [lo, hi) of one stripe -- member m of group g, lo < hi, both below the cursor -- through the bitmap
template <bool Dual>
__device__ __forceinline__ uint32_t piece_bits(const uint8_t *__restrict__ store, const Geometry &geo, uint64_t lo, uint64_t hi, uint64_t covered,
                                               const uint4 *__restrict__ guard_p, const uint4 *__restrict__ guard_q,
                                               const unsigned long long *__restrict__ bitmap, const uint8_t *gf_log)
{
    const uint64_t t = lo >> geo.shift, g = t / geo.G, first = g * geo.words();
    const uint32_t m = (uint32_t)(t - g * geo.G);
    const uint64_t stripe_at = t << geo.shift;                                       // the stripe's first byte
    const uint64_t i0 = first + ((lo - stripe_at) >> 4), i1 = first + ((hi - 1 - stripe_at) >> 4); // its guard words, inclusive
    uint32_t out = 0;
    for (uint64_t w = i0 >> 6; w <= i1 >> 6; w++) {
        unsigned long long bits = bitmap[w];
        if (w == i0 >> 6) bits &= ~0ull << (i0 & 63u);
        if (w == i1 >> 6) bits &= ~0ull >> (63u - (uint32_t)(i1 & 63u));
        while (bits) {
            const uint64_t i = (w << 6) + (uint32_t)(__ffsll((long long)bits) - 1);
            bits &= bits - 1;
            const uint64_t cw = i - first, at = g * geo.W + (cw << 4), mine = stripe_at + (cw << 4); // member 0's word, the piece's
            const Sums d = differences<Dual>(store, geo, g, cw, covered, guard_p, guard_q);
#pragma unroll 1 // (dirty words are rare; unrolled, the sixteen classifications cost scalar-register spills)
            for (uint32_t b = 0; b < 16; b++) {
                if (mine + b < lo || mine + b >= hi) continue;
                const uint32_t c = classify<Dual>(byte_of(d.p, b), byte_of(d.q, b), members_below(geo, at + b, covered), gf_log);
                out |= c == kAmbiguous ? 2u : c == m ? 1u : 0u;
            }
        }
    }
    return out;
}

template <bool Dual>
__global__ void __launch_bounds__(kThreads)
locate_entries_kernel(const uint8_t *__restrict__ store, uint64_t store_bytes, const uint4 *__restrict__ dir, uint64_t dir_entries,
                      const uint64_t *__restrict__ d_covered, Geometry geo, const uint4 *__restrict__ guard_p, const uint4 *__restrict__ guard_q,
                      const unsigned long long *__restrict__ bitmap, uint32_t *__restrict__ suspect, LocateHead *__restrict__ head)
{
    __shared__ uint8_t gf_log[Dual ? 256 : 1];
    __shared__ uint32_t wsum[kThreads / 64];
    const uint64_t covered = *d_covered;
    if (covered > store_bytes) return;
    if constexpr (Dual) build_log(gf_log);
    const uint64_t threads = (uint64_t)gridDim.x * kThreads;
    uint32_t suspects = 0, unjudged = 0; // (a thread sees at most dir_entries / threads + 1 < 2^32 entries)
    for (uint64_t idx = (uint64_t)blockIdx.x * kThreads + threadIdx.x; idx < dir_entries; idx += threads) {
        const Entry e(dir[idx]);
        uint32_t v = 0;
        if (e.nonzero) {
            if (!e.sound(store_bytes) || e.pos + e.stored > covered) v = 4u;
            else {
                // at most two pieces: stored <= 65536 <= S.  (One copy of the walk in the code: two cost scalar-register spills)
                const uint64_t end = e.pos + e.stored;
#pragma unroll 1
                for (uint64_t lo = e.pos; lo < end;) {
                    const uint64_t cut = umin64(end, (lo | (geo.S - 1)) + 1);
                    v |= piece_bits<Dual>(store, geo, lo, cut, covered, guard_p, guard_q, bitmap, gf_log);
                    lo = cut;
                }
            }
        }
        suspect[idx] = v;
        suspects += (v & 3u) != 0;
        unjudged += v == 4u;
    }
    const uint32_t all_suspects = group_sum(suspects, wsum), all_unjudged = group_sum(unjudged, wsum);
    if (threadIdx.x != 0) return;
    if (all_suspects) __hip_atomic_fetch_add(&head->suspects, (unsigned long long)all_suspects, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (all_unjudged) __hip_atomic_fetch_add(&head->unjudged, (unsigned long long)all_unjudged, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// one thread, behind both: the result.  With verdict 1 the counters are the zeros the head was set to
__global__ void __launch_bounds__(64)
locate_finish_kernel(uint64_t store_bytes, const uint64_t *__restrict__ d_covered, Geometry geo, const LocateHead *__restrict__ head,
                     uint64_t *__restrict__ result)
{
    if (threadIdx.x != 0) return;
    const uint64_t covered = *d_covered;
    const bool ok = covered <= store_bytes;
    result[0] = ok ? 0 : 1;
    result[1] = ok ? (covered + geo.W - 1) / geo.W : 0;
    result[2] = head->dirty;
    result[3] = head->located;
    result[4] = head->ambiguous;
    result[5] = head->suspects;
    result[6] = head->unjudged;
    result[7] = 0;
}

// per stream, for both parities: the counters in the 64-byte head, then a bit per guard word of the store's groups
StreamScratch<DeviceBuf> locate_spaces;

template <bool Dual>
hipError_t locate_launch(const uint8_t *store, size_t store_bytes, const uint4 *dir, size_t dir_entries, const uint64_t *d_covered, const Geometry &geo,
                         size_t groups, const uint4 *guard_p, const uint4 *guard_q, uint32_t *suspect, uint64_t *result, hipStream_t stream)
{
    auto &w = locate_spaces.at(stream);
    LaunchLock sequence(w.launch); // the head and the bitmap are shared by the launches below
    hipError_t e = w.reserve(store_guard_locate_scratch_bytes(groups, (size_t)geo.S), (size_t)1 << 20);
    if (e != hipSuccess) return e;
    LocateHead *head = w.as<LocateHead>();
    unsigned long long *bitmap = reinterpret_cast<unsigned long long *>(w.as<uint8_t>() + kScratchHead);
    if ((e = hipMemsetAsync(head, 0, kScratchHead, stream)) != hipSuccess) return e;
    if (groups)
        hipLaunchKernelGGL(locate_sweep_kernel<Dual>, dim3(lane_grid(groups * (geo.S / 16))), dim3(kThreads), 0, stream, store, (uint64_t)store_bytes,
                           d_covered, geo, guard_p, guard_q, bitmap, head);
    // (an empty store protects nothing: its entries read no bit)
    hipLaunchKernelGGL(locate_entries_kernel<Dual>, dim3(lane_grid(dir_entries)), dim3(kThreads), 0, stream, store, (uint64_t)store_bytes, dir,
                       (uint64_t)dir_entries, d_covered, geo, guard_p, guard_q, bitmap, suspect, head);
    hipLaunchKernelGGL(locate_finish_kernel, dim3(1), dim3(64), 0, stream, (uint64_t)store_bytes, d_covered, geo, head, result);
    return hipGetLastError();
}

} // namespace

size_t store_guard_locate_scratch_bytes(size_t groups, size_t stripe) { return kScratchHead + groups * (stripe / 128); }

hipError_t store_guard_locate_launch(const uint8_t *store, size_t store_bytes, const void *dir, size_t dir_entries, const uint64_t *d_covered,
                                     size_t stripe, unsigned group, const void *guard_p, const void *guard_q, uint32_t *suspect, uint64_t *result,
                                     hipStream_t stream)
{
    const Geometry geo = geometry(stripe, group);
    const size_t groups = store_guard_groups(store_bytes, stripe, group);
    const auto launch = guard_q ? locate_launch<true> : locate_launch<false>;
    return launch(store, store_bytes, static_cast<const uint4 *>(dir), dir_entries, d_covered, geo, groups, static_cast<const uint4 *>(guard_p),
                  static_cast<const uint4 *>(guard_q), suspect, result, stream);
}

} // namespace cw
