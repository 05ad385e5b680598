// guard_kernels.hip -- guard stripes over the store's bytes, with one syndrome or two (DESIGN.md sections 28 and 29; semantics: the
// public header's cw_dev_store_guard_update, _check and _rebuild and their cw_dev_store_guard2_ forms).  With S = stripe, G = group
// and W = G * S, store byte p lies in stripe p / S, which is member m = (p / S) % G of group p / W, at column p % S.  Over the bytes
// p below the cursor `covered` of group g and column c,
//     P[g * S + c] = XOR of store[p]          and, on a dual guard,          Q[g * S + c] = XOR of 2^m (x) store[p]
// in GF(2^8) with x^8 + x^4 + x^3 + x^2 + 1 (0x11D) and generator 2.  2 has order 255, so a dual guard has G <= 255 and the weights
// of a group's members differ.  S is a multiple of 16 and all buffers are 16-byte aligned, so a 16-byte guard word and the G store
// words it sums never straddle a stripe.  Every kernel that the second syndrome changes is a template over `Dual`; a launcher takes
// guard_q == nullptr for the single guard, and both parities share one scratch per stream.
//
// Update: a lane per guard word that [from, to) = [*d_covered, *d_used) touches.  Only the first and the last group of the range can
// be touched in part; a group touched in fewer than S / 16 words names them by their first column, wrapping at S.  The lane loads the
// members' words that lie whole in the range one after the other with nothing between them, masks the at most two that the range
// cuts, and does one read-modify-write: no two lanes own the same word, so there are no atomics.  A second kernel moves the cursor and
// reports: everything the first one wrote lies behind a kernel boundary when `covered` changes.  Dual: the members' words are loaded
// from the highest member down, because Q is accumulated by Horner's rule, acc = 2 (x) acc ^ word, with the doubling done on packed
// dwords (xtime), and Q gets a read-modify-write of its own; no tables, no LDS.  The P word written is the single guard's.
// Check: a lane per guard word of the groups below the cursor, the same sum over [0, covered) compared with the word; a flag per group
// in the scratch, counted and copied out by one workgroup.  Dual: a second flag per group for Q, bit 1 of what is copied out.
// Rebuild: an extent of at most 65536 <= S bytes crosses at most one stripe boundary, so it is at most two PIECES, each in one stripe:
// (group, member, columns [c0, c1)).  Two pieces collide iff they share the group, differ in the member and their columns overlap --
// then some byte of the one meets another byte of the other in a guard byte.  Pieces of one extent never do (their columns are
// [c, S) and [0, c') with c' <= c), nor do pieces of a value named twice (same member), so the test needs no position.  The pieces
// are counting-sorted by group (count -> scan -> scatter) and a position tests its pieces against their own groups' buckets only: it
// is rebuilt (status 0) unless one of its pieces collides.  A wavefront per rebuilt position then sums guard and members in aligned
// 4-byte words.  Dual: a position is rebuilt unless one of its pieces is HOT -- two pieces of two other members of its bucket overlap
// it in a common column: three different store bytes in one guard cell.  A rebuilt position's extent in d_out first serves as its
// PARTNER MAP: every byte gets 0xFF, then the member of the one other listed piece that covers its column, if any (two kernels: the
// map of a status-0 position is single-valued, so concurrent writers write equal bytes).  The copy then computes P'' and Q'' = the
// guard words less every member's word but its own, and per byte either P'' (no partner) or
//     (Q'' ^ 2^o (x) P'') (x) inv(2^m ^ 2^o)          (partner in member o: its stored byte, known or not, cancels)
// with exp / log tables of the field built in LDS at kernel start.
// The copy is one template: both parities walk the same positions, words and tail mask, and every dual part -- the tables, the Q
// word, the partner map's loads -- sits under `if constexpr`, so the single instantiation holds no LDS and keeps its registers.
//
// Scratch, per stream: check 64 + 4 * N bytes (dual 64 + 8 * N), rebuild 80 + 28 * max_count + 16 * N bytes, N = the groups of
// store_bytes.  Work of the dual rebuild: linear in n and in the rebuilt bytes plus, per piece, its bucket once for the sort, once
// more for every piece of the bucket that overlaps it (the hot test), and the overlapped columns once per overlapping piece (the map).

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "cw_device.h"
#include "guard_sums.h"
#include "store_device.h"

namespace cw {

namespace {

using namespace chunkstore;
using namespace guardsums;

// ---- update --------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t update_verdict(uint64_t from, uint64_t to, uint64_t store_bytes) { return from > to || to > store_bytes ? 1u : 0u; }

// The guard words a non-empty range [from, to) touches, one index i < total each: only the first and the last group of the range can
// be touched in part
struct Touched {
    uint64_t g0, g1, first0, n0, first1, n1, mid, total;
    __device__ __forceinline__ Touched(const Geometry &geo, uint64_t from, uint64_t to)
    {
        g0 = from / geo.W;
        g1 = (to - 1) / geo.W;
        first1 = n1 = 0;
        in_group(geo, g0, from, to, first0, n0);
        if (g1 > g0) in_group(geo, g1, from, to, first1, n1);
        mid = g1 > g0 ? (g1 - g0 - 1) * geo.words() : 0;
        total = n0 + mid + n1;
    }
    // the guard words of group g that [from, to) touches: `count` of them from column word `first` on, wrapping at S / 16
    __device__ __forceinline__ static void in_group(const Geometry &geo, uint64_t g, uint64_t from, uint64_t to, uint64_t &first, uint64_t &count)
    {
        const uint64_t lo = from > g * geo.W ? from : g * geo.W, hi = umin64(to, (g + 1) * geo.W);
        const uint64_t n = ((hi - 1) >> 4) - (lo >> 4) + 1; // the 16-byte words of [lo, hi), lo < hi
        const bool all = n >= geo.words();
        first = all ? 0 : (lo & (geo.S - 1)) >> 4;
        count = all ? geo.words() : n;
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

template <bool Dual>
__global__ void __launch_bounds__(kThreads)
guard_fold_kernel(const uint8_t *__restrict__ store, uint64_t store_bytes, const uint64_t *__restrict__ d_used, const uint64_t *__restrict__ d_covered,
                  Geometry geo, uint4 *__restrict__ guard_p, uint4 *__restrict__ guard_q)
{
    const uint64_t from = *d_covered, to = *d_used;
    if (update_verdict(from, to, store_bytes) || from == to) return;
    const Touched t(geo, from, to);
    const uint64_t threads = (uint64_t)gridDim.x * kThreads;
    for (uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x; i < t.total; i += threads) {
        uint64_t g, cw;
        t.at(geo, i, g, cw);
        const Sums s = members_sums<Dual>(store, geo, g * geo.W + (cw << 4), from, to);
        const uint64_t at = g * geo.words() + cw;
        guard_p[at] = guard_p[at] ^ s.p;
        if constexpr (Dual) guard_q[at] = guard_q[at] ^ s.q;
    }
}

// one thread, behind the fold: the cursor and the result
__global__ void __launch_bounds__(64)
guard_update_finish_kernel(uint64_t store_bytes, const uint64_t *__restrict__ d_used, uint64_t *__restrict__ d_covered, uint64_t *__restrict__ result)
{
    if (threadIdx.x != 0) return;
    const uint64_t from = *d_covered, to = *d_used;
    const uint32_t verdict = update_verdict(from, to, store_bytes);
    result[0] = verdict;
    result[1] = from;
    result[2] = to;
    result[3] = verdict ? 0 : to - from;
    if (verdict == 0) *d_covered = to;
}

// ---- check ---------------------------------------------------------------------------------------------------------------------------
// flags[g] for P and, with Dual, flags[groups + g] for Q
template <bool Dual>
__global__ void __launch_bounds__(kThreads)
guard_compare_kernel(const uint8_t *__restrict__ store, uint64_t store_bytes, const uint64_t *__restrict__ d_covered, Geometry geo, uint64_t groups,
                     const uint4 *__restrict__ guard_p, const uint4 *__restrict__ guard_q, uint32_t *__restrict__ flags)
{
    const uint64_t covered = *d_covered;
    if (covered > store_bytes) return;
    const uint64_t words = geo.words(), total = (covered + geo.W - 1) / geo.W * words, threads = (uint64_t)gridDim.x * kThreads;
    for (uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x; i < total; i += threads) {
        const uint64_t g = i >> (geo.shift - 4), cw = i & (words - 1);
        const Sums s = members_sums<Dual>(store, geo, g * geo.W + (cw << 4), 0, covered);
        if (differ(s.p, guard_p[i])) flags[g] = 1u; // (every writer writes 1)
        if constexpr (Dual)
            if (differ(s.q, guard_q[i])) flags[groups + g] = 1u;
    }
}

// one workgroup: the flags counted and copied out, bit 0 for P and, with Dual, bit 1 for Q
template <bool Dual>
__global__ void __launch_bounds__(kThreads)
guard_check_finish_kernel(uint64_t store_bytes, const uint64_t *__restrict__ d_covered, Geometry geo, uint64_t all_groups,
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
        uint32_t f = flags[g];
        if constexpr (Dual) f |= flags[all_groups + g] << 1;
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
struct Piece {
    uint64_t g;
    uint32_t m, c0, len; // len == 0: no piece
};

// the at most two pieces of the extent [pos, pos + stored), 1 <= stored <= 65536 <= S
__device__ __forceinline__ void pieces_of(const Geometry &geo, uint64_t pos, uint32_t stored, Piece out[2])
{
    const uint64_t t = pos >> geo.shift, c = pos & (geo.S - 1);
    const uint32_t head = (uint32_t)umin64(stored, geo.S - c);
    const uint64_t g = t / geo.G;
    const uint32_t m = (uint32_t)(t - g * geo.G);
    out[0] = Piece{g, m, (uint32_t)c, head};
    const bool wraps = m + 1 == geo.G;
    out[1] = Piece{wraps ? g + 1 : g, wraps ? 0u : m + 1, 0u, stored - head};
}

__device__ __forceinline__ uint2 packed(const Piece &p) { return make_uint2(p.c0, p.len | p.m << 24); } // len <= 65536 < 2^24, m < 256

struct RebuildHead { // the first 32 of the scratch's 64 head bytes
    unsigned long long rebuilt, groups, consistent;
    unsigned long long paired; // dual: the rebuilt positions with a partner, those that needed Q
};

struct Positions {
    const uint4 *dir;
    uint64_t dir_base, dir_entries, store_bytes;
    const uint64_t *values, *d_count;
    uint64_t max_count;
    const uint64_t *d_covered;
    __device__ __forceinline__ uint64_t n() const { return umin64(*d_count, max_count); }
    // an inconsistent cursor protects nothing
    __device__ __forceinline__ uint64_t covered() const { return *d_covered <= store_bytes ? *d_covered : 0; }
    // position k's entry when it is protected: it names a sound entry that ends at or below the cursor
    __device__ __forceinline__ bool is_protected(uint64_t k, uint64_t cov, uint64_t &pos, uint32_t &stored, uint4 &raw) const
    {
        uint64_t idx;
        if (!names_entry(values[k], dir_base, dir_entries, idx)) return false;
        raw = dir[idx];
        const Entry e(raw);
        pos = e.pos;
        stored = e.stored;
        return e.nonzero && e.sound(store_bytes) && e.pos + e.stored <= cov;
    }
};

__device__ __forceinline__ uint32_t rebuild_verdict(const RebuildHead *head, uint64_t total, uint64_t out_bytes)
{
    if (!head->consistent) return 2u;
    return total > out_bytes ? 1u : 0u;
}

// the 4 bytes at store + p (p % 4 == 0) with the bytes at or above `covered` read as zero; p < covered
__device__ __forceinline__ uint32_t word_below(const uint8_t *__restrict__ store, uint64_t p, uint64_t covered)
{
    if (p + 4 <= covered) return *reinterpret_cast<const uint32_t *>(store + p);
    uint32_t v = 0;
    for (uint32_t i = 0; p + i < covered; i++) v |= (uint32_t)store[p + i] << (8 * i);
    return v;
}

// the counting sort by group, a lane per position: count[g] += the pieces of the protected positions in group g; the head
__global__ void __launch_bounds__(kThreads)
rebuild_count_kernel(Positions P, Geometry geo, uint64_t groups, uint32_t *__restrict__ count, RebuildHead *__restrict__ head)
{
    const uint64_t n = P.n(), cov = P.covered(), threads = (uint64_t)gridDim.x * kThreads;
    for (uint64_t k = (uint64_t)blockIdx.x * kThreads + threadIdx.x; k < n; k += threads) {
        uint64_t pos;
        uint32_t stored;
        uint4 raw;
        if (!P.is_protected(k, cov, pos, stored, raw)) continue;
        Piece p[2];
        pieces_of(geo, pos, stored, p);
        atomicAdd(count + p[0].g, 1u);
        if (p[1].len) atomicAdd(count + p[1].g, 1u);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        head->groups = groups;
        head->consistent = *P.d_covered <= P.store_bytes;
    }
}

// ... and sorted[first[g] ..) = the pieces of group g, in any order
__global__ void __launch_bounds__(kThreads)
rebuild_scatter_kernel(Positions P, Geometry geo, const unsigned long long *__restrict__ first, uint32_t *__restrict__ cursor, uint2 *__restrict__ sorted)
{
    const uint64_t n = P.n(), cov = P.covered(), threads = (uint64_t)gridDim.x * kThreads;
    for (uint64_t k = (uint64_t)blockIdx.x * kThreads + threadIdx.x; k < n; k += threads) {
        uint64_t pos;
        uint32_t stored;
        uint4 raw;
        if (!P.is_protected(k, cov, pos, stored, raw)) continue;
        Piece p[2];
        pieces_of(geo, pos, stored, p);
        sorted[first[p[0].g] + atomicAdd(cursor + p[0].g, 1u)] = packed(p[0]);
        if (p[1].len) sorted[first[p[1].g] + atomicAdd(cursor + p[1].g, 1u)] = packed(p[1]);
    }
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

// The single guard's test: a piece of another member of the group with a column in common with p.  The dual guard's (hot): two
// such pieces, of two different members, with a column in common with each other as well
template <bool Dual>
__device__ __forceinline__ bool unrecoverable(const Piece &p, const unsigned long long *__restrict__ first, const uint2 *__restrict__ sorted)
{
    const uint64_t e = first[p.g + 1];
    for (uint64_t j = first[p.g]; j < e; j++) {
        const Other o(sorted[j], p);
        if (!o.overlaps(p)) continue;
        if constexpr (!Dual) return true;
        else
            for (uint64_t i = j + 1; i < e; i++) {
                const uint2 t = sorted[i];
                const uint32_t m = t.y >> 24;
                if (m != p.m && m != o.m && t.x < o.z && o.a < t.x + (t.y & 0xFFFFFFu)) return true;
            }
    }
    return false;
}

// status[k], sizes[k] = the stored bytes of a position that will be rebuilt, else 0; head->rebuilt
template <bool Dual>
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
            s = unrecoverable<Dual>(p[0], first, sorted) || (p[1].len && unrecoverable<Dual>(p[1], first, sorted)) ? 1u : 0u;
        }
        status[k] = s;
        sizes[k] = s == 0 ? stored : 0u;
        rebuilt += s == 0;
    }
    const uint32_t all = group_sum(rebuilt, wsum);
    if (threadIdx.x == 0 && all) __hip_atomic_fetch_add(&head->rebuilt, (unsigned long long)all, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

constexpr uint32_t kNoPartner = 0xFFu; // in the partner map: members are below 255

// dual; a wavefront per position: the partner map of a rebuilt extent starts as "no partner"
__global__ void __launch_bounds__(64)
rebuild2_fill_kernel(Positions P, const unsigned long long *__restrict__ off, const uint32_t *__restrict__ status, const RebuildHead *__restrict__ head,
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

// dual; a wavefront per position: the members of the other listed pieces over the columns they share with a rebuilt extent, into its
// map; head->paired.  The count is taken whatever the verdict is, the map is written only when the payload will be
__global__ void __launch_bounds__(64)
rebuild2_pair_kernel(Positions P, Geometry geo, const unsigned long long *__restrict__ first, const uint2 *__restrict__ sorted,
                     const unsigned long long *__restrict__ off, const uint32_t *__restrict__ status, RebuildHead *__restrict__ head,
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

// A wavefront per position: a rebuilt extent to out + off[k], byte = guard byte ^ the other members' bytes below the cursor; out_loc[k].
// Dual: over the extent's own partner map.  P'' and Q'' are the guard words less the words of every member but the extent's own
// below the cursor; a byte without a partner is P'', a byte whose partner is member o is (Q'' ^ 2^o (x) P'') (x) inv(2^self ^ 2^o).
// gf_exp[i] = 2^i for i < 510 and gf_log[2^i] = i, built by repeated doubling.  (The dual copy loads its map through `out`, so only
// the single copy's `out` is __restrict__.)
template <bool Dual>
__global__ void __launch_bounds__(64)
rebuild_copy_kernel(const uint8_t *__restrict__ store, Positions P, Geometry geo, const uint8_t *__restrict__ guard_p, const uint8_t *__restrict__ guard_q,
                    const unsigned long long *__restrict__ off, const uint32_t *__restrict__ status, const RebuildHead *__restrict__ head,
                    std::conditional_t<Dual, uint8_t *, uint8_t *__restrict__> out, uint64_t out_bytes, uint4 *__restrict__ out_loc)
{
    __shared__ uint8_t gf_exp[Dual ? 512 : 1], gf_log[Dual ? 256 : 1]; // (never touched, so never allocated, unless Dual)
    const uint64_t n = P.n(), cov = P.covered();
    if (rebuild_verdict(head, off[n], out_bytes)) return;
    if constexpr (Dual) {
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
    }
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
            uint32_t vp = *reinterpret_cast<const uint32_t *>(guard_p + w.g * geo.S + w.c), vq = 0;
            if constexpr (!Dual) {
#pragma unroll 4
                for (uint32_t m = 0; m < geo.G; m++) {
                    const uint64_t p = w.base + ((uint64_t)m << geo.shift);
                    if (p >= cov) break;
                    if (m != w.self) vp ^= word_below(store, p, cov);
                }
            } else {
                vq = *reinterpret_cast<const uint32_t *>(guard_q + w.g * geo.S + w.c);
                uint32_t acc = 0;
                // the members with a byte of this word below the cursor (the extent's own is one of them), from the highest down
#pragma unroll 4
                for (uint32_t m = (uint32_t)umin64(geo.G, ((cov - 1 - w.base) >> geo.shift) + 1); m-- > 0;) {
                    const uint32_t word = m != w.self ? word_below(store, w.base + ((uint64_t)m << geo.shift), cov) : 0u;
                    vp ^= word;
                    acc = xtime(acc) ^ word;
                }
                vq ^= acc;
            }
#pragma unroll
            for (uint32_t i = 0; i < 4; i++) {
                if (q + i < pos || q + i >= end) continue;
                uint8_t *at = out + to + (q + i - pos);
                uint32_t v = (vp >> (8 * i)) & 0xFFu;
                if constexpr (Dual) {
                    const uint32_t o = *at, pb = v, qb = (vq >> (8 * i)) & 0xFFu;
                    if (o != kNoPartner) {
                        const uint32_t t = qb ^ (pb ? gf_exp[o + gf_log[pb]] : 0u);
                        v = t ? gf_exp[gf_log[t] + 255u - gf_log[gf_exp[w.self] ^ gf_exp[o]]] : 0u;
                    }
                }
                *at = (uint8_t)v;
            }
        }
        if (threadIdx.x == 0) out_loc[k] = Entry(raw).at(to);
    }
}

// result[4], the positions that needed Q, only with Dual: the single call's result holds four words
template <bool Dual>
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
    if constexpr (Dual) result[4] = head->paired;
}

// per stream, for both parities: check's flags behind a 64-byte head; rebuild's layout in RebuildScratch
StreamScratch<DeviceBuf> guard_spaces;
static_assert(sizeof(RebuildHead) <= kScratchHead, "the head holds the four words");

// The rebuild's scratch over n positions and the groups of the store: the head; two scans -- the positions' sizes and the groups'
// piece counts -- each as a ScanScratch; the sorted pieces; the cursors behind the counts, so that one memset clears both
struct RebuildScratch {
    ScanScratch pos, grp;
    uint2 *sorted;
    uint32_t *cursor;
    RebuildHead *head;
    RebuildScratch(uint8_t *base, size_t n, size_t groups)
    {
        pos.head = grp.head = base;
        pos.off = reinterpret_cast<uint64_t *>(base + kScratchHead);
        grp.off = pos.off + n + 1;
        sorted = reinterpret_cast<uint2 *>(grp.off + groups + 1);
        pos.sizes = reinterpret_cast<uint32_t *>(sorted + 2 * n);
        grp.sizes = pos.sizes + n;
        cursor = grp.sizes + groups;
        head = pos.head_as<RebuildHead>();
    }
};

} // namespace

size_t store_guard_groups(size_t store_bytes, size_t stripe, unsigned group)
{
    const size_t w = stripe * group;
    return store_bytes / w + (store_bytes % w != 0);
}

size_t store_guard_check_scratch_bytes(size_t groups, bool dual) { return kScratchHead + (dual ? 8 : 4) * groups; }
size_t store_guard_rebuild_scratch_bytes(size_t max_count, size_t groups) { return kScratchHead + 16 + 28 * max_count + 16 * groups; }

hipError_t store_guard_update_launch(const uint8_t *store, size_t store_bytes, const uint64_t *d_used, uint64_t *d_covered, size_t stripe,
                                     unsigned group, void *guard_p, void *guard_q, uint64_t *result, hipStream_t stream)
{
    const Geometry geo = geometry(stripe, group);
    const size_t words = store_guard_groups(store_bytes, stripe, group) * (stripe / 16);
    if (words)
        hipLaunchKernelGGL(guard_q ? guard_fold_kernel<true> : guard_fold_kernel<false>, dim3(lane_grid(words)), dim3(kThreads), 0, stream, store,
                           (uint64_t)store_bytes, d_used, d_covered, geo, static_cast<uint4 *>(guard_p), static_cast<uint4 *>(guard_q));
    hipLaunchKernelGGL(guard_update_finish_kernel, dim3(1), dim3(64), 0, stream, (uint64_t)store_bytes, d_used, d_covered, result);
    return hipGetLastError();
}

hipError_t store_guard_check_launch(const uint8_t *store, size_t store_bytes, const uint64_t *d_covered, size_t stripe, unsigned group,
                                    const void *guard_p, const void *guard_q, uint32_t *group_bad, uint64_t *result, hipStream_t stream)
{
    const Geometry geo = geometry(stripe, group);
    const size_t groups = store_guard_groups(store_bytes, stripe, group);
    const bool dual = guard_q != nullptr;
    auto &w = guard_spaces.at(stream);
    LaunchLock sequence(w.launch); // the flags are shared by the launches below
    hipError_t e = w.reserve(store_guard_check_scratch_bytes(groups, dual), (size_t)1 << 20);
    if (e != hipSuccess) return e;
    uint32_t *flags = reinterpret_cast<uint32_t *>(w.as<uint8_t>() + kScratchHead);
    if (groups) {
        if ((e = hipMemsetAsync(flags, 0, (dual ? 8 : 4) * groups, stream)) != hipSuccess) return e;
        hipLaunchKernelGGL(dual ? guard_compare_kernel<true> : guard_compare_kernel<false>, dim3(lane_grid(groups * (stripe / 16))), dim3(kThreads), 0,
                           stream, store, (uint64_t)store_bytes, d_covered, geo, (uint64_t)groups, static_cast<const uint4 *>(guard_p),
                           static_cast<const uint4 *>(guard_q), flags);
    }
    hipLaunchKernelGGL(dual ? guard_check_finish_kernel<true> : guard_check_finish_kernel<false>, dim3(1), dim3(kThreads), 0, stream,
                       (uint64_t)store_bytes, d_covered, geo, (uint64_t)groups, flags, group_bad, result);
    return hipGetLastError();
}

hipError_t store_guard_rebuild_launch(const uint8_t *store, size_t store_bytes, const void *dir, uint64_t dir_base, size_t dir_entries,
                                      const uint64_t *d_covered, size_t stripe, unsigned group, const void *guard_p, const void *guard_q,
                                      const uint64_t *values, const uint64_t *d_count, size_t max_count, uint8_t *out, size_t out_bytes, void *out_loc,
                                      uint32_t *status, uint64_t *result, hipStream_t stream)
{
    const Geometry geo = geometry(stripe, group);
    const size_t groups = store_guard_groups(store_bytes, stripe, group), n = max_count;
    const bool dual = guard_q != nullptr;
    auto &w = guard_spaces.at(stream);
    LaunchLock sequence(w.launch); // the head and the arrays are shared by the launches below
    hipError_t e = w.reserve(store_guard_rebuild_scratch_bytes(n, groups), (size_t)1 << 20);
    if (e != hipSuccess) return e;
    const RebuildScratch s(w.as<uint8_t>(), n, groups);
    if ((e = hipMemsetAsync(s.head, 0, kScratchHead, stream)) != hipSuccess) return e;
    if (groups && (e = hipMemsetAsync(s.grp.sizes, 0, 8 * groups, stream)) != hipSuccess) return e; // the counts and the cursors
    const Positions P{static_cast<const uint4 *>(dir), dir_base, (uint64_t)dir_entries, (uint64_t)store_bytes, values, d_count, (uint64_t)n, d_covered};
    const dim3 g(lane_grid(n ? n : 1)), b(kThreads), waves(wave_grid(n ? n : 1)), wave(64);
    hipLaunchKernelGGL(rebuild_count_kernel, g, b, 0, stream, P, geo, (uint64_t)groups, s.grp.sizes, s.head);
    // first[g] = the pieces of the groups below g
    if ((e = chunk_pack_launch(0, nullptr, nullptr, nullptr, reinterpret_cast<const uint64_t *>(&s.head->groups), groups, s.grp.sizes, nullptr,
                               s.grp.off, stream)) != hipSuccess)
        return e;
    if (n) {
        hipLaunchKernelGGL(rebuild_scatter_kernel, g, b, 0, stream, P, geo, s.grp.offsets(), s.cursor, s.sorted);
        hipLaunchKernelGGL(dual ? rebuild_status_kernel<true> : rebuild_status_kernel<false>, g, b, 0, stream, P, geo, s.grp.offsets(), s.sorted,
                           s.pos.sizes, status, s.head);
    }
    // off[k] = the rebuilt bytes of the positions below k
    if ((e = chunk_pack_launch(0, nullptr, nullptr, nullptr, d_count, n, s.pos.sizes, nullptr, s.pos.off, stream)) != hipSuccess) return e;
    if (n) {
        if (dual) { // the partner maps in d_out, each step behind a kernel boundary, then the extents over them
            hipLaunchKernelGGL(rebuild2_fill_kernel, waves, wave, 0, stream, P, s.pos.offsets(), status, s.head, out, (uint64_t)out_bytes);
            hipLaunchKernelGGL(rebuild2_pair_kernel, waves, wave, 0, stream, P, geo, s.grp.offsets(), s.sorted, s.pos.offsets(), status, s.head, out,
                               (uint64_t)out_bytes);
        }
        hipLaunchKernelGGL(dual ? rebuild_copy_kernel<true> : rebuild_copy_kernel<false>, waves, wave, 0, stream, store, P, geo,
                           static_cast<const uint8_t *>(guard_p), static_cast<const uint8_t *>(guard_q), s.pos.offsets(), status, s.head, out,
                           (uint64_t)out_bytes, static_cast<uint4 *>(out_loc));
    }
    hipLaunchKernelGGL(dual ? rebuild_finish_kernel<true> : rebuild_finish_kernel<false>, dim3(1), dim3(64), 0, stream, P, s.pos.offsets(), s.head,
                       (uint64_t)out_bytes, result);
    return hipGetLastError();
}

} // namespace cw
