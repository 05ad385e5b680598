// store_device.h -- what the chunk store's kernel files share (restore_, read_, store_gc_, renumber_, account_, replicate_, scrub_
// guard_ and guard_locate_kernels.hip): the directory entry and its soundness rule, the value -> index rules of a directory, the workgroup and
// wavefront sums, the wavefront's copy of its lanes' extents, and on the host side the scan scratch and the three grid rules.
// Each file keeps its own StreamScratch registry (launch functions nest on a stream); nothing here holds state.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cw_device.h"
#include "lz_device.h"
#include "stream_scratch.h"

namespace cw {
namespace chunkstore {

constexpr unsigned kThreads = 256;
constexpr uint32_t kRawFlag = 0x80000000u, kLenMask = 0x1FFFFu; // cw_chunk_loc::raw (CW_CHUNK_RAW; bits 17..30 stay 0)

// ---- device: a directory entry --------------------------------------------------------------------------------------------------
struct Entry {
    uint64_t pos;
    uint32_t stored, word;
    bool nonzero;
    __device__ __forceinline__ explicit Entry(const uint4 e) : pos((uint64_t)e.y << 32 | e.x), stored(e.z), word(e.w), nonzero((e.x | e.y | e.z | e.w) != 0) {}
    __device__ __forceinline__ uint32_t len() const { return word & kLenMask; }
    __device__ __forceinline__ bool raw() const { return (word & kRawFlag) != 0; }
    // The store's integrity rule, as far as it needs no recipe, against the buffer of `bytes` bytes the entry points into: the
    // reserved bits are zero, 1 <= len <= 65536, stored != 0, a raw entry has stored == len, pos <= bytes and stored <= bytes - pos.
    // An all-zero entry fails it: its length is 0.  Nothing may be loaded or stored through an entry that fails.
    __device__ __forceinline__ bool sound(uint64_t bytes) const
    {
        return (word & ~(kRawFlag | kLenMask)) == 0 && len() != 0 && len() <= kMaxChunkBytes && stored != 0 && (!raw() || stored == len()) &&
               pos <= bytes && stored <= bytes - pos;
    }
    // the same chunk stored at `to`
    __device__ __forceinline__ uint4 at(uint64_t to) const { return make_uint4((uint32_t)to, (uint32_t)(to >> 32), stored, word); }
};

// ---- device: value -> directory index --------------------------------------------------------------------------------------------
// idx = the entry `value` names; false when it names none (a value below the base wraps out of range, CW_DEDUPE_MISS with it)
__device__ __forceinline__ bool names_entry(uint64_t value, uint64_t dir_base, uint64_t dir_entries, uint64_t &idx)
{
    idx = value - dir_base;
    return idx < dir_entries;
}

// directory entry of the chunk with value base + k (neither sum may wrap), or, with `values`, with value values[k]
struct Directory {
    uint4 *entries;
    uint64_t base, dir_base, dir_entries;
    const uint64_t *values; // NULL: counted up from base
    // kListed = false: a caller that never has a list (the append) says so, and its index() holds neither the test nor the load
    template <bool kListed = true> __device__ __forceinline__ bool index(uint64_t k, uint64_t &idx) const
    {
        const uint64_t *list = kListed ? values : nullptr;
        const uint64_t v = list ? list[k] : base + k;
        idx = v - dir_base;
        return (list || v >= base) && v >= dir_base && idx < dir_entries;
    }
    // the replace keeps a chunk's length: an entry whose own length field is sound (1..65536) takes no other length
    __device__ __forceinline__ bool keeps_length(uint64_t idx, uint32_t word) const
    {
        const uint32_t len = entries[idx].w & kLenMask;
        return len == 0 || len > kMaxChunkBytes || len == (word & kLenMask);
    }
};

// ---- device: sums and copies ------------------------------------------------------------------------------------------------------
// (the value parameter is not deduced: callers pass flags and u32 counts whatever T sums them)
template <class T> struct SumOf { typedef T type; };

// the wavefront's sum of v in lane 0 (every lane calls)
template <class T = uint32_t> __device__ __forceinline__ T wave_sum(typename SumOf<T>::type v)
{
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

// the workgroup's sum of v in thread 0 (kThreads threads, every one of them calls); T is wsum's
template <class T> __device__ __forceinline__ T group_sum(typename SumOf<T>::type v, T *wsum)
{
    v = wave_sum<T>(v);
    if ((threadIdx.x & 63u) == 0) wsum[threadIdx.x >> 6] = v;
    __syncthreads();
    T all = 0;
    for (uint32_t w = 0; w < kThreads / 64; w++) all += wsum[w];
    __syncthreads(); // the next sum writes wsum again
    return all;
}

// The lanes with `have` set each name an extent: the wavefront copies these extents one after the other, in lane order, each with
// all 64 lanes.  For workgroups of one wavefront, all of whose lanes call.  An address is a buffer of the kernel's and the lane's
// offset into it: only the offsets go through the shuffles, so the copy still knows that it reads and writes two __restrict__
// buffers and keeps its 16 loads in flight (with whole addresses shuffled it waits for every load before the next store).
// from_slot: lane k's source lies in its own slot of that many bytes, at from + k * from_slot + from_off -- k is the lane's index in
// the wavefront, so `from` is the wavefront's first slot and only lanes that own a slot may set `have` (read_edges_kernel's buffers).
__device__ __forceinline__ void wave_copy(bool have, const uint8_t *__restrict__ from, uint64_t from_off, uint8_t *__restrict__ to, uint64_t to_off,
                                          uint32_t len, uint64_t from_slot = 0)
{
    unsigned long long copies = __ballot(have);
    while (copies) {
        const int k = __ffsll((long long)copies) - 1;
        copies &= copies - 1;
        const uint64_t f = __shfl((unsigned long long)from_off, k, 64), t = __shfl((unsigned long long)to_off, k, 64);
        lz::copy_g2g(to + t, from + (uint64_t)k * from_slot + f, (uint32_t)__shfl((int)len, k, 64), threadIdx.x);
    }
}

// ---- host: the scan scratch and the grids ------------------------------------------------------------------------------------------
constexpr size_t kScratchHead = 64; // every store scratch starts with a head of this many bytes

// What a sizes -> scan -> copy -> finish sequence over n items keeps per stream: the head (zeroed in front of every sequence), the
// scan's offsets (u64, n + 1) and the sizes (u32, n) behind them: 72 + 12 * n bytes, as the public header promises.
struct ScanScratch {
    uint8_t *head;
    uint64_t *off;
    uint32_t *sizes;
    template <class T> T *head_as() const { return reinterpret_cast<T *>(head); }
    const unsigned long long *offsets() const { return reinterpret_cast<const unsigned long long *>(off); } // as the kernels read them
};
inline hipError_t scan_scratch(DeviceBuf &buf, size_t n, hipStream_t stream, ScanScratch &s)
{
    const hipError_t e = buf.reserve(kScratchHead + (n + 1) * 8 + n * 4, (size_t)1 << 20);
    if (e != hipSuccess) return e;
    s.head = buf.as<uint8_t>();
    s.off = reinterpret_cast<uint64_t *>(s.head + kScratchHead);
    s.sizes = reinterpret_cast<uint32_t *>(s.off + n + 1);
    return hipMemsetAsync(s.head, 0, kScratchHead, stream);
}

// a lane per item, grid-stride
inline unsigned lane_grid(size_t n)
{
    const size_t grid = (n + kThreads - 1) / kThreads;
    return (unsigned)(grid < 256 * 8 ? grid : 256 * 8);
}
// a wavefront per item, grid-stride
inline unsigned wave_grid(size_t n) { return (unsigned)(n < 256 * 32 ? n : 256 * 32); }
// a wavefront per 64 items, each lane decoding one
inline unsigned decode_grid(size_t n)
{
    const size_t grid = (n + 63) / 64;
    return (unsigned)(grid < 256 * 8 ? grid : 256 * 8);
}

} // namespace chunkstore
} // namespace cw
