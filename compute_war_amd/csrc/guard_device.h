// guard_device.h -- what guard_kernels.hip (the XOR guard) and guard2_kernels.hip (the dual guard, section 29)
// share: the geometry, the masked 16-byte store word and the range rule of a group's members, the update's verdict and the guard
// words a range touches in one group, an extent's pieces, the listed positions with their protection rule, the counting sort of
// the pieces by group and the rebuild's verdict.  Nothing here holds state.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cw_device.h"
#include "store_device.h"

namespace cw {
namespace guardstripes {

using namespace chunkstore;

struct Geometry {
    uint64_t S, W;     // stripe bytes (a power of two), group bytes
    uint32_t G, shift; // members per group, log2(S)
    __device__ __forceinline__ uint64_t words() const { return S >> 4; } // guard words per group
};

__device__ __forceinline__ uint4 operator^(const uint4 a, const uint4 b) { return make_uint4(a.x ^ b.x, a.y ^ b.y, a.z ^ b.z, a.w ^ b.w); }
__device__ __forceinline__ bool differ(const uint4 a, const uint4 b) { return ((a.x ^ b.x) | (a.y ^ b.y) | (a.z ^ b.z) | (a.w ^ b.w)) != 0; }

// the 16 bytes at store + p (p % 16 == 0) with every byte outside [lo, hi) read as zero; no load leaves [lo, hi)
__device__ __forceinline__ uint4 word_in(const uint8_t *__restrict__ store, uint64_t p, uint64_t lo, uint64_t hi)
{
    if (p >= lo && p + 16 <= hi) return *reinterpret_cast<const uint4 *>(store + p);
    uint64_t l = 0, h = 0;
    const uint64_t a = p > lo ? p : lo, b = umin64(p + 16, hi);
    for (uint64_t q = a; q < b; q++) {
        const uint32_t i = (uint32_t)(q - p);
        if (i < 8) l |= (uint64_t)store[q] << (8 * i);
        else h |= (uint64_t)store[q] << (8 * (i - 8));
    }
    return make_uint4((uint32_t)l, (uint32_t)(l >> 32), (uint32_t)h, (uint32_t)(h >> 32));
}

// The members m < G of the store words at base + m * S, against the range [lo, hi): those whose word lies whole in the range are
// [ma, mb); the range cuts at most the words of members ma - 1 and mb (one word when ma > mb)
struct Members {
    uint64_t ma, mb;
    bool below, above; // the range cuts the word of member ma - 1, of member mb
    __device__ __forceinline__ Members(const Geometry &geo, uint64_t base, uint64_t lo, uint64_t hi)
    {
        const uint64_t G = geo.G;
        ma = lo <= base ? 0 : umin64(G, (lo - base + geo.S - 1) >> geo.shift);
        mb = hi < base + 16 ? 0 : umin64(G, ((hi - base - 16) >> geo.shift) + 1);
        below = ma > 0 && ma - 1 != mb;
        above = mb < G && mb + 1 >= ma;
    }
};

// XOR over the members of the store words, bytes outside [lo, hi) as zero: the whole words loaded back to back
__device__ __forceinline__ uint4 members_sum(const uint8_t *__restrict__ store, const Geometry &geo, uint64_t base, uint64_t lo, uint64_t hi)
{
    const Members r(geo, base, lo, hi);
    uint4 acc = make_uint4(0, 0, 0, 0);
#pragma unroll 8
    for (uint64_t m = r.ma; m < r.mb; m++) acc = acc ^ *reinterpret_cast<const uint4 *>(store + base + (m << geo.shift));
    if (r.below) acc = acc ^ word_in(store, base + ((r.ma - 1) << geo.shift), lo, hi);
    if (r.above) acc = acc ^ word_in(store, base + (r.mb << geo.shift), lo, hi);
    return acc;
}

// ---- update --------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t update_verdict(uint64_t from, uint64_t to, uint64_t store_bytes) { return from > to || to > store_bytes ? 1u : 0u; }

// the guard words of group g that [from, to) touches: `count` of them from column word `first` on, wrapping at S / 16
__device__ __forceinline__ void touched(const Geometry &geo, uint64_t g, uint64_t from, uint64_t to, uint64_t &first, uint64_t &count)
{
    const uint64_t lo = from > g * geo.W ? from : g * geo.W, hi = umin64(to, (g + 1) * geo.W);
    const uint64_t n = ((hi - 1) >> 4) - (lo >> 4) + 1; // the 16-byte words of [lo, hi), lo < hi
    const bool all = n >= geo.words();
    first = all ? 0 : (lo & (geo.S - 1)) >> 4;
    count = all ? geo.words() : n;
}

// one thread, behind the fold: the cursor and the result
__device__ __forceinline__ void update_finish(uint64_t store_bytes, const uint64_t *__restrict__ d_used, uint64_t *__restrict__ d_covered,
                                              uint64_t *__restrict__ result)
{
    const uint64_t from = *d_covered, to = *d_used;
    const uint32_t verdict = update_verdict(from, to, store_bytes);
    result[0] = verdict;
    result[1] = from;
    result[2] = to;
    result[3] = verdict ? 0 : to - from;
    if (verdict == 0) *d_covered = to;
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

struct RebuildHead { // the first 24 of the scratch's 64 head bytes
    unsigned long long rebuilt, groups, consistent;
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

// the counting sort by group, a lane per position: count[g] += the pieces of the protected positions in group g; the head
__device__ __forceinline__ void rebuild_count(const Positions &P, const Geometry &geo, uint64_t groups, uint32_t *__restrict__ count,
                                              RebuildHead *__restrict__ head)
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
__device__ __forceinline__ void rebuild_scatter(const Positions &P, const Geometry &geo, const unsigned long long *__restrict__ first,
                                                uint32_t *__restrict__ cursor, uint2 *__restrict__ sorted)
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

inline Geometry geometry(size_t stripe, unsigned group)
{
    uint32_t shift = 0;
    while (((size_t)1 << shift) < stripe) shift++;
    return Geometry{(uint64_t)stripe, (uint64_t)stripe * group, group, shift};
}

} // namespace guardstripes
} // namespace cw
