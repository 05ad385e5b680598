// guard2_kernels.hip -- the dual guard: a second syndrome Q, weighted over GF(2^8), beside the XOR guard P of guard_kernels.hip
// (semantics: the public header's cw_dev_store_guard2_update, _check and _rebuild).  Geometry, cursor, pieces
// and positions are section 28's (guard_device.h).  The field is GF(2^8) with x^8 + x^4 + x^3 + x^2 + 1 (0x11D) and generator 2; with
// m = (p / S) % G the member of store byte p,
//     P[g * S + c] = XOR of store[p],        Q[g * S + c] = XOR of 2^m (x) store[p]      over the p < covered of group g and column c.
// 2 has order 255, so G <= 255 and the weights of a group's members differ.
//
// Update: a lane per 16-byte guard word the range touches, as in guard_fold_kernel: the same words, the same masks at the two cut
// words, the members' words loaded from the highest member down, because Q is accumulated by Horner's rule, acc = 2 (x) acc ^ word,
// with the doubling done on packed dwords (xtime).  Two read-modify-writes, no tables, no LDS, no atomics; the cursor moves in a second
// kernel.  The P word written is guard_fold_kernel's.
// Check: the same two sums over [0, covered) compared with the two words; a flag per group and syndrome in the scratch, no atomics.
// Rebuild: positions, protection rule, pieces and the counting sort by group are section 28's.  A piece is HOT when two pieces of two
// other members of its bucket overlap it in a common column: three different store bytes in one guard cell.  A position is rebuilt
// (status 0) unless one of its pieces is hot.  A rebuilt position's extent in d_out first serves as its PARTNER MAP: every byte gets
// 0xFF, then the member of the one other listed piece that covers its column, if any (two kernels: the map of a status-0 position is
// single-valued, so concurrent writers write equal bytes).  The copy kernel then runs a wavefront per position in aligned 4-byte
// words: P'' and Q'' = the guard words less every member's word but its own, then per byte either P'' (no partner) or
//     (Q'' ^ 2^o (x) P'') (x) inv(2^m ^ 2^o)          (partner in member o: its stored byte, known or not, cancels)
// with exp / log tables of the field built in LDS at kernel start.  No scratch beyond section 28's.
//
// Scratch, per stream: check 64 + 8 * N bytes, rebuild 80 + 28 * max_count + 16 * N bytes, N = the groups of store_bytes.  Work of
// the rebuild: linear in n and in the rebuilt bytes plus, per piece, its bucket once for the sort, once more for every piece of the
// bucket that overlaps it (the hot test), and the overlapped columns once per overlapping piece (the map).

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cw_device.h"
#include "guard_device.h"
#include "store_device.h"

namespace cw {

namespace {

using namespace chunkstore;
using namespace guardstripes;

constexpr uint32_t kNoPartner = 0xFFu; // in the partner map: members are below 255

// 2 (x) every byte of x
__device__ __forceinline__ uint32_t xtime(uint32_t x) { return ((x & 0x7f7f7f7fu) << 1) ^ (((x >> 7) & 0x01010101u) * 0x1du); }
__device__ __forceinline__ uint4 xtime(const uint4 x) { return make_uint4(xtime(x.x), xtime(x.y), xtime(x.z), xtime(x.w)); }

struct Sums {
    uint4 p, q;
};

// P and Q over the members m < G of the store words at base + m * S, bytes outside [lo, hi) as zero: Horner from the highest member
// that contributes down to the lowest, then the doublings of the members below it
__device__ __forceinline__ Sums members_sums(const uint8_t *__restrict__ store, const Geometry &geo, uint64_t base, uint64_t lo, uint64_t hi)
{
    const Members r(geo, base, lo, hi);
    Sums s{make_uint4(0, 0, 0, 0), make_uint4(0, 0, 0, 0)};
    if (r.above) s.p = s.q = word_in(store, base + (r.mb << geo.shift), lo, hi);
#pragma unroll 8
    for (uint64_t m = r.mb; m-- > r.ma;) {
        const uint4 w = *reinterpret_cast<const uint4 *>(store + base + (m << geo.shift));
        s.p = s.p ^ w;
        s.q = xtime(s.q) ^ w;
    }
    if (r.below) {
        const uint4 w = word_in(store, base + ((r.ma - 1) << geo.shift), lo, hi);
        s.p = s.p ^ w;
        s.q = xtime(s.q) ^ w;
    }
    // (members ma - 1, [ma, mb) and mb are neighbours, so every step above was one doubling)
    for (uint64_t low = r.below ? r.ma - 1 : umin64(r.ma, r.mb); low > 0; low--) s.q = xtime(s.q);
    return s;
}

// ---- update --------------------------------------------------------------------------------------------------------------------------
// The guard words a non-empty range [from, to) touches, one index i < total each: only the first and the last group of the range can
// be touched in part
struct Touched {
    uint64_t g0, g1, first0, n0, first1, n1, mid, total;
    __device__ __forceinline__ Touched(const Geometry &geo, uint64_t from, uint64_t to)
    {
        g0 = from / geo.W;
        g1 = (to - 1) / geo.W;
        first1 = n1 = 0;
        touched(geo, g0, from, to, first0, n0);
        if (g1 > g0) touched(geo, g1, from, to, first1, n1);
        mid = g1 > g0 ? (g1 - g0 - 1) * geo.words() : 0;
        total = n0 + mid + n1;
    }
    // word i: its group and its column word
    __device__ __forceinline__ void at(const Geometry &geo, uint64_t i, uint64_t &g, uint64_t &cw) const
    {
        const uint64_t words = geo.words();
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
    }
};

__global__ void __launch_bounds__(kThreads)
guard2_fold_kernel(const uint8_t *__restrict__ store, uint64_t store_bytes, const uint64_t *__restrict__ d_used, const uint64_t *__restrict__ d_covered,
                   Geometry geo, uint4 *__restrict__ guard_p, uint4 *__restrict__ guard_q)
{
    const uint64_t from = *d_covered, to = *d_used;
    if (update_verdict(from, to, store_bytes) || from == to) return;
    const Touched t(geo, from, to);
    const uint64_t threads = (uint64_t)gridDim.x * kThreads;
    for (uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x; i < t.total; i += threads) {
        uint64_t g, cw;
        t.at(geo, i, g, cw);
        const Sums s = members_sums(store, geo, g * geo.W + (cw << 4), from, to);
        const uint64_t at = g * geo.words() + cw;
        guard_p[at] = guard_p[at] ^ s.p;
        guard_q[at] = guard_q[at] ^ s.q;
    }
}

// one thread, behind the fold: the cursor and the result
__global__ void __launch_bounds__(64)
guard2_update_finish_kernel(uint64_t store_bytes, const uint64_t *__restrict__ d_used, uint64_t *__restrict__ d_covered, uint64_t *__restrict__ result)
{
    if (threadIdx.x == 0) update_finish(store_bytes, d_used, d_covered, result);
}

// ---- check ---------------------------------------------------------------------------------------------------------------------------
// flags[g] for P and flags[groups + g] for Q
__global__ void __launch_bounds__(kThreads)
guard2_compare_kernel(const uint8_t *__restrict__ store, uint64_t store_bytes, const uint64_t *__restrict__ d_covered, Geometry geo, uint64_t groups,
                      const uint4 *__restrict__ guard_p, const uint4 *__restrict__ guard_q, uint32_t *__restrict__ flags)
{
    const uint64_t covered = *d_covered;
    if (covered > store_bytes) return;
    const uint64_t words = geo.words(), total = (covered + geo.W - 1) / geo.W * words, threads = (uint64_t)gridDim.x * kThreads;
    for (uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x; i < total; i += threads) {
        const uint64_t g = i >> (geo.shift - 4), cw = i & (words - 1);
        const Sums s = members_sums(store, geo, g * geo.W + (cw << 4), 0, covered);
        if (differ(s.p, guard_p[i])) flags[g] = 1u; // (every writer writes 1)
        if (differ(s.q, guard_q[i])) flags[groups + g] = 1u;
    }
}

// one workgroup: the flags counted and copied out, bit 0 for P and bit 1 for Q
__global__ void __launch_bounds__(kThreads)
guard2_check_finish_kernel(uint64_t store_bytes, const uint64_t *__restrict__ d_covered, Geometry geo, uint64_t all_groups,
                           const uint32_t *__restrict__ flags, uint32_t *__restrict__ group_bad, uint64_t *__restrict__ result)
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
        const uint32_t f = flags[g] | flags[all_groups + g] << 1;
        if (group_bad) group_bad[g] = f;
        if (f && low == ~0ull) low = g;
        bad += f != 0;
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
struct Rebuild2Head : RebuildHead { // the first 32 of the scratch's 64 head bytes
    unsigned long long paired;      // the rebuilt positions with a partner: those that needed Q
};

// count[g] += the pieces of the protected positions in group g; the head
__global__ void __launch_bounds__(kThreads)
rebuild2_count_kernel(Positions P, Geometry geo, uint64_t groups, uint32_t *__restrict__ count, Rebuild2Head *__restrict__ head)
{
    rebuild_count(P, geo, groups, count, head);
}

// sorted[first[g] ..) = the pieces of group g, in any order
__global__ void __launch_bounds__(kThreads)
rebuild2_scatter_kernel(Positions P, Geometry geo, const unsigned long long *__restrict__ first, uint32_t *__restrict__ cursor, uint2 *__restrict__ sorted)
{
    rebuild_scatter(P, geo, first, cursor, sorted);
}

struct Other { // a sorted piece against a piece p: the columns [a, z) they share, when it is of another member
    uint32_t m, a, z;
    __device__ __forceinline__ Other(const uint2 o, const Piece &p) : m(o.y >> 24)
    {
        const uint32_t end = o.x + (o.y & 0xFFFFFFu), mine = p.c0 + p.len;
        a = o.x > p.c0 ? o.x : p.c0;
        z = end < mine ? end : mine;
    }
    __device__ __forceinline__ bool overlaps(const Piece &p) const { return m != p.m && a < z; }
};

// two pieces of two other members of the group with a column in common with each other and with p
__device__ __forceinline__ bool hot(const Piece &p, const unsigned long long *__restrict__ first, const uint2 *__restrict__ sorted)
{
    const uint64_t e = first[p.g + 1];
    for (uint64_t j = first[p.g]; j < e; j++) {
        const Other o(sorted[j], p);
        if (!o.overlaps(p)) continue;
        for (uint64_t i = j + 1; i < e; i++) {
            const uint2 t = sorted[i];
            const uint32_t m = t.y >> 24;
            if (m != p.m && m != o.m && t.x < o.z && o.a < t.x + (t.y & 0xFFFFFFu)) return true;
        }
    }
    return false;
}

// status[k], sizes[k] = the stored bytes of a position that will be rebuilt, else 0; head->rebuilt
__global__ void __launch_bounds__(kThreads)
rebuild2_status_kernel(Positions P, Geometry geo, const unsigned long long *__restrict__ first, const uint2 *__restrict__ sorted,
                       uint32_t *__restrict__ sizes, uint32_t *__restrict__ status, Rebuild2Head *__restrict__ head)
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
            s = hot(p[0], first, sorted) || (p[1].len && hot(p[1], first, sorted)) ? 1u : 0u;
        }
        status[k] = s;
        sizes[k] = s == 0 ? stored : 0u;
        rebuilt += s == 0;
    }
    const uint32_t all = group_sum(rebuilt, wsum);
    if (threadIdx.x == 0 && all) __hip_atomic_fetch_add(&head->rebuilt, (unsigned long long)all, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// a wavefront per position: the partner map of a rebuilt extent starts as "no partner"
__global__ void __launch_bounds__(64)
rebuild2_fill_kernel(Positions P, const unsigned long long *__restrict__ off, const uint32_t *__restrict__ status, const Rebuild2Head *__restrict__ head,
                     uint8_t *__restrict__ out, uint64_t out_bytes)
{
    const uint64_t n = P.n();
    if (rebuild_verdict(head, off[n], out_bytes)) return;
    for (uint64_t k = blockIdx.x; k < n; k += gridDim.x) {
        if (status[k] != 0) continue;
        const uint64_t to = off[k], end = off[k + 1]; // (the sizes of the positions that are not rebuilt are 0)
        for (uint64_t i = to + threadIdx.x; i < end; i += 64) out[i] = (uint8_t)kNoPartner;
    }
}

// a wavefront per position: the members of the other listed pieces over the columns they share with a rebuilt extent, into its map;
// head->paired.  The count is taken whatever the verdict is, the map is written only when the payload will be
__global__ void __launch_bounds__(64)
rebuild2_pair_kernel(Positions P, Geometry geo, const unsigned long long *__restrict__ first, const uint2 *__restrict__ sorted,
                     const unsigned long long *__restrict__ off, const uint32_t *__restrict__ status, Rebuild2Head *__restrict__ head,
                     uint8_t *__restrict__ out, uint64_t out_bytes)
{
    const uint64_t n = P.n(), cov = P.covered();
    const bool write = rebuild_verdict(head, off[n], out_bytes) == 0;
    for (uint64_t k = blockIdx.x; k < n; k += gridDim.x) {
        uint64_t pos;
        uint32_t stored;
        uint4 raw;
        if (status[k] != 0 || !P.is_protected(k, cov, pos, stored, raw)) continue; // (a position with status 0 is protected)
        Piece p[2];
        pieces_of(geo, pos, stored, p);
        bool paired = false;
#pragma unroll
        for (uint32_t h = 0; h < 2; h++) {
            if (p[h].len == 0) continue;
            const uint64_t to = off[k] + (h ? p[0].len : 0u); // the piece's first byte in d_out
            for (uint64_t j = first[p[h].g], e = first[p[h].g + 1]; j < e; j++) {
                const Other o(sorted[j], p[h]);
                if (!o.overlaps(p[h])) continue;
                paired = true;
                if (write)
                    for (uint32_t c = o.a + threadIdx.x; c < o.z; c += 64) out[to + (c - p[h].c0)] = (uint8_t)o.m;
            }
        }
        if (paired && threadIdx.x == 0) __hip_atomic_fetch_add(&head->paired, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// the word of an extent that starts in stripe t0 = member m0 of group g0: its stripe is the extent's first or the one behind it
struct WordAt {
    uint64_t g, c, base; // group, column, the store position of member 0's word
    uint32_t self;       // the extent's own member there
    __device__ __forceinline__ WordAt(const Geometry &geo, uint64_t q, uint64_t t0, uint64_t g0, uint32_t m0)
    {
        const bool next = (q >> geo.shift) != t0, wraps = next && m0 + 1 == geo.G;
        g = wraps ? g0 + 1 : g0;
        c = q & (geo.S - 1);
        base = g * geo.W + c;
        self = wraps ? 0u : m0 + next;
    }
};

// A wavefront per position: a rebuilt extent to out + off[k], over its own partner map; out_loc[k].  P'' and Q'' are the guard words
// less the words of every member but the extent's own below the cursor; a byte without a partner is P'', a byte whose partner is
// member o is (Q'' ^ 2^o (x) P'') (x) inv(2^self ^ 2^o).  gf_exp[i] = 2^i for i < 510 and gf_log[2^i] = i, built by repeated doubling
__global__ void __launch_bounds__(64)
rebuild2_copy_kernel(const uint8_t *__restrict__ store, Positions P, Geometry geo, const uint8_t *__restrict__ guard_p, const uint8_t *__restrict__ guard_q,
                     const unsigned long long *__restrict__ off, const uint32_t *__restrict__ status, const Rebuild2Head *__restrict__ head,
                     uint8_t *out, uint64_t out_bytes, uint4 *__restrict__ out_loc)
{
    __shared__ uint8_t gf_exp[512], gf_log[256];
    const uint64_t n = P.n(), cov = P.covered();
    if (rebuild_verdict(head, off[n], out_bytes)) return;
    uint32_t x = 1;
    for (uint32_t i = 0; i < 255; i++) { // every lane walks the powers and writes its share
        if ((i & 63u) == threadIdx.x) {
            gf_exp[i] = (uint8_t)x;
            gf_exp[i + 255] = (uint8_t)x;
            gf_log[x] = (uint8_t)i;
        }
        x = xtime(x) & 0xFFu;
    }
    if (threadIdx.x < 2) gf_exp[510 + threadIdx.x] = 0; // (never indexed: log t + 255 - log d <= 509)
    if (threadIdx.x == 0) gf_log[0] = 0;                // (never indexed: zero is tested for)
    __syncthreads();
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
            const WordAt w(geo, q, t0, g0, m0);
            uint32_t vp = *reinterpret_cast<const uint32_t *>(guard_p + w.g * geo.S + w.c);
            uint32_t vq = *reinterpret_cast<const uint32_t *>(guard_q + w.g * geo.S + w.c), acc = 0;
            // the members with a byte of this word below the cursor (the extent's own is one of them), from the highest down
#pragma unroll 4
            for (uint32_t m = (uint32_t)umin64(geo.G, ((cov - 1 - w.base) >> geo.shift) + 1); m-- > 0;) {
                const uint32_t word = m != w.self ? word_below(store, w.base + ((uint64_t)m << geo.shift), cov) : 0u;
                vp ^= word;
                acc = xtime(acc) ^ word;
            }
            vq ^= acc;
#pragma unroll
            for (uint32_t i = 0; i < 4; i++) {
                if (q + i < pos || q + i >= end) continue;
                uint8_t *at = out + to + (q + i - pos);
                const uint32_t o = *at, pb = (vp >> (8 * i)) & 0xFFu, qb = (vq >> (8 * i)) & 0xFFu;
                uint32_t v = pb;
                if (o != kNoPartner) {
                    const uint32_t t = qb ^ (pb ? gf_exp[o + gf_log[pb]] : 0u);
                    v = t ? gf_exp[gf_log[t] + 255u - gf_log[gf_exp[w.self] ^ gf_exp[o]]] : 0u;
                }
                *at = (uint8_t)v;
            }
        }
        if (threadIdx.x == 0) out_loc[k] = Entry(raw).at(to);
    }
}

__global__ void __launch_bounds__(64)
rebuild2_finish_kernel(Positions P, const unsigned long long *__restrict__ off, const Rebuild2Head *__restrict__ head, uint64_t out_bytes,
                       uint64_t *__restrict__ result)
{
    if (threadIdx.x != 0) return;
    const uint64_t n = P.n(), total = off[n];
    result[0] = rebuild_verdict(head, total, out_bytes);
    result[1] = total;
    result[2] = n;
    result[3] = head->rebuilt;
    result[4] = head->paired;
}

// per stream: check's flags behind a 64-byte head; rebuild's layout in store_guard2_rebuild_launch
StreamScratch<DeviceBuf> guard2_spaces;
static_assert(sizeof(Rebuild2Head) <= kScratchHead, "the head holds the four words");

} // namespace

size_t store_guard2_check_scratch_bytes(size_t groups) { return kScratchHead + 8 * groups; }

hipError_t store_guard2_update_launch(const uint8_t *store, size_t store_bytes, const uint64_t *d_used, uint64_t *d_covered, size_t stripe,
                                      unsigned group, void *guard_p, void *guard_q, uint64_t *result, hipStream_t stream)
{
    const Geometry geo = geometry(stripe, group);
    const size_t words = store_guard_groups(store_bytes, stripe, group) * (stripe / 16);
    if (words)
        hipLaunchKernelGGL(guard2_fold_kernel, dim3(lane_grid(words)), dim3(kThreads), 0, stream, store, (uint64_t)store_bytes, d_used, d_covered, geo,
                           static_cast<uint4 *>(guard_p), static_cast<uint4 *>(guard_q));
    hipLaunchKernelGGL(guard2_update_finish_kernel, dim3(1), dim3(64), 0, stream, (uint64_t)store_bytes, d_used, d_covered, result);
    return hipGetLastError();
}

hipError_t store_guard2_check_launch(const uint8_t *store, size_t store_bytes, const uint64_t *d_covered, size_t stripe, unsigned group,
                                     const void *guard_p, const void *guard_q, uint32_t *group_bad, uint64_t *result, hipStream_t stream)
{
    const Geometry geo = geometry(stripe, group);
    const size_t groups = store_guard_groups(store_bytes, stripe, group);
    auto &w = guard2_spaces.at(stream);
    LaunchLock sequence(w.launch); // the flags are shared by the launches below
    hipError_t e = w.reserve(store_guard2_check_scratch_bytes(groups), (size_t)1 << 20);
    if (e != hipSuccess) return e;
    uint32_t *flags = reinterpret_cast<uint32_t *>(w.as<uint8_t>() + kScratchHead);
    if (groups) {
        if ((e = hipMemsetAsync(flags, 0, 8 * groups, stream)) != hipSuccess) return e;
        hipLaunchKernelGGL(guard2_compare_kernel, dim3(lane_grid(groups * (stripe / 16))), dim3(kThreads), 0, stream, store, (uint64_t)store_bytes,
                           d_covered, geo, (uint64_t)groups, static_cast<const uint4 *>(guard_p), static_cast<const uint4 *>(guard_q), flags);
    }
    hipLaunchKernelGGL(guard2_check_finish_kernel, dim3(1), dim3(kThreads), 0, stream, (uint64_t)store_bytes, d_covered, geo, (uint64_t)groups, flags,
                       group_bad, result);
    return hipGetLastError();
}

hipError_t store_guard2_rebuild_launch(const uint8_t *store, size_t store_bytes, const void *dir, uint64_t dir_base, size_t dir_entries,
                                       const uint64_t *d_covered, size_t stripe, unsigned group, const void *guard_p, const void *guard_q,
                                       const uint64_t *values, const uint64_t *d_count, size_t max_count, uint8_t *out, size_t out_bytes, void *out_loc,
                                       uint32_t *status, uint64_t *result, hipStream_t stream)
{
    const Geometry geo = geometry(stripe, group);
    const size_t groups = store_guard_groups(store_bytes, stripe, group), n = max_count;
    auto &w = guard2_spaces.at(stream);
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
    Rebuild2Head *head = pos.head_as<Rebuild2Head>();
    if ((e = hipMemsetAsync(head, 0, kScratchHead, stream)) != hipSuccess) return e;
    if (groups && (e = hipMemsetAsync(grp.sizes, 0, 8 * groups, stream)) != hipSuccess) return e; // the counts and the cursors
    const Positions P{static_cast<const uint4 *>(dir), dir_base, (uint64_t)dir_entries, (uint64_t)store_bytes, values, d_count, (uint64_t)n, d_covered};
    const dim3 g(lane_grid(n ? n : 1)), b(kThreads), waves(wave_grid(n ? n : 1)), wave(64);
    hipLaunchKernelGGL(rebuild2_count_kernel, g, b, 0, stream, P, geo, (uint64_t)groups, grp.sizes, head);
    // first[g] = the pieces of the groups below g
    if ((e = chunk_pack_launch(0, nullptr, nullptr, nullptr, reinterpret_cast<const uint64_t *>(&head->groups), groups, grp.sizes, nullptr, grp.off,
                               stream)) != hipSuccess)
        return e;
    if (n) {
        hipLaunchKernelGGL(rebuild2_scatter_kernel, g, b, 0, stream, P, geo, grp.offsets(), cursor, sorted);
        hipLaunchKernelGGL(rebuild2_status_kernel, g, b, 0, stream, P, geo, grp.offsets(), sorted, pos.sizes, status, head);
    }
    // off[k] = the rebuilt bytes of the positions below k
    if ((e = chunk_pack_launch(0, nullptr, nullptr, nullptr, d_count, n, pos.sizes, nullptr, pos.off, stream)) != hipSuccess) return e;
    if (n) {
        // the partner maps in d_out, each step behind a kernel boundary, then the extents over them
        hipLaunchKernelGGL(rebuild2_fill_kernel, waves, wave, 0, stream, P, pos.offsets(), status, head, out, (uint64_t)out_bytes);
        hipLaunchKernelGGL(rebuild2_pair_kernel, waves, wave, 0, stream, P, geo, grp.offsets(), sorted, pos.offsets(), status, head, out,
                           (uint64_t)out_bytes);
        hipLaunchKernelGGL(rebuild2_copy_kernel, waves, wave, 0, stream, store, P, geo, static_cast<const uint8_t *>(guard_p),
                           static_cast<const uint8_t *>(guard_q), pos.offsets(), status, head, out, (uint64_t)out_bytes, static_cast<uint4 *>(out_loc));
    }
    hipLaunchKernelGGL(rebuild2_finish_kernel, dim3(1), dim3(64), 0, stream, P, pos.offsets(), head, (uint64_t)out_bytes, result);
    return hipGetLastError();
}

} // namespace cw
