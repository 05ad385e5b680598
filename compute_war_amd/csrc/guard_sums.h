// guard_sums.h -- what the guard's kernel files share (guard_kernels.hip, guard_locate_kernels.hip): the geometry of the stripes and
// the sums P and Q over the members of one 16-byte guard word (DESIGN.md sections 28 and 29).  With S = stripe, G = group and
// W = G * S, store byte p is member m = (p / S) % G of group p / W, at column p % S; S is a multiple of 16 and all buffers are
// 16-byte aligned, so a guard word and the G store words it sums never straddle a stripe.  Nothing here holds state.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cw_device.h"

namespace cw {
namespace guardsums {

struct Geometry {
    uint64_t S, W;     // stripe bytes (a power of two), group bytes
    uint32_t G, shift; // members per group, log2(S)
    __device__ __forceinline__ uint64_t words() const { return S >> 4; } // guard words per group
};

inline Geometry geometry(size_t stripe, unsigned group)
{
    uint32_t shift = 0;
    while (((size_t)1 << shift) < stripe) shift++;
    return Geometry{(uint64_t)stripe, (uint64_t)stripe * group, group, shift};
}

__device__ __forceinline__ uint4 operator^(const uint4 a, const uint4 b) { return make_uint4(a.x ^ b.x, a.y ^ b.y, a.z ^ b.z, a.w ^ b.w); }
__device__ __forceinline__ bool differ(const uint4 a, const uint4 b) { return ((a.x ^ b.x) | (a.y ^ b.y) | (a.z ^ b.z) | (a.w ^ b.w)) != 0; }

// 2 (x) every byte of x
__device__ __forceinline__ uint32_t xtime(uint32_t x) { return ((x & 0x7f7f7f7fu) << 1) ^ (((x >> 7) & 0x01010101u) * 0x1du); }
__device__ __forceinline__ uint4 xtime(const uint4 x) { return make_uint4(xtime(x.x), xtime(x.y), xtime(x.z), xtime(x.w)); }

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

struct Sums {
    uint4 p, q; // q: of a dual guard only
};

// P, and with Dual Q, over the members of the store words, bytes outside [lo, hi) as zero.  The two load orders are deliberate:
// the single guard loads the whole words back to back, from the lowest member up; the dual guard runs Horner's rule from the
// highest member that contributes down to the lowest, then the doublings of the members below it
template <bool Dual>
__device__ __forceinline__ Sums members_sums(const uint8_t *__restrict__ store, const Geometry &geo, uint64_t base, uint64_t lo, uint64_t hi)
{
    const Members r(geo, base, lo, hi);
    Sums s{make_uint4(0, 0, 0, 0), make_uint4(0, 0, 0, 0)};
    if constexpr (!Dual) {
#pragma unroll 8
        for (uint64_t m = r.ma; m < r.mb; m++) s.p = s.p ^ *reinterpret_cast<const uint4 *>(store + base + (m << geo.shift));
        if (r.below) s.p = s.p ^ word_in(store, base + ((r.ma - 1) << geo.shift), lo, hi);
        if (r.above) s.p = s.p ^ word_in(store, base + (r.mb << geo.shift), lo, hi);
    } else {
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
    }
    return s;
}

} // namespace guardsums
} // namespace cw
