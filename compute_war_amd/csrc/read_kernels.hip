// read_kernels.hip -- byte ranges of a deduplicated stream: cw_dev_read_ranges gives back stream bytes
// [off, off + len) of a recipe over the chunk store without rebuilding the stream.  Nothing here keeps state between calls.
//
// Four steps, each behind a kernel boundary of the one before:
//   plan    a lane per range: the range's own verdict (status 3 or 0), its first touched position and its piece count
//           (piece = a touched position), found by binary search in the recipe's offsets
//   scan    the piece counts -> piece offsets and their total (pack_launch, index only)
//   pieces  a lane per piece, 64 at a time: the entry's soundness (store_device.h); a compressed chunk that lies wholly inside its
//           range is decoded straight into the destination, raw entries are copied by the whole wavefront clipped to the range
//   edges   a lane per edge slot (2k: the first piece of range k, 2k + 1: its last): a compressed chunk the range covers only in
//           part is decoded WHOLE into the lane's own 64 KiB buffer (an LZ chunk decodes only from its start), then the wavefront
//           copies the covered window out of it.  The wavefront that wrote a buffer is the one that reads it.
// Every field of a range, a recipe position and a directory entry is checked before anything is loaded or stored through it.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cw_device.h"
#include "lane_codec.h"
#include "lz_device.h"
#include "store_device.h"

namespace cw {

namespace {

using namespace lane;
using namespace chunkstore;

// the store, its directory and the recipe, as cw_dev_restore_chunks takes them
struct Recipe {
    const uint8_t *store;
    uint64_t store_bytes;
    const uint4 *dir;
    uint64_t dir_base, dir_entries;
    const uint64_t *ref, *raw_off, *d_count;
    uint64_t max_count;
    __device__ __forceinline__ uint64_t count() const { return umin64(*d_count, max_count); }
};
struct Ranges {
    const uint64_t *off, *len, *dst, *d_n;
    uint64_t max_ranges;
    __device__ __forceinline__ uint64_t count() const { return umin64(*d_n, max_ranges); }
};

// the smallest i in [1, n] with v[i] > x, n where there is none (v non-decreasing; any other list still gives an i in [1, n])
__device__ __forceinline__ uint64_t first_above(const uint64_t *__restrict__ v, uint64_t n, uint64_t x)
{
    uint64_t lo = 1, hi = n;
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if (v[mid] > x) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

// ---- plan --------------------------------------------------------------------------------------------------------------------
// status[k] for k < R; first[k] and pieces[k] for every k < max_ranges (0 pieces: refused, empty, or behind R), which the scan sums
__global__ void __launch_bounds__(kThreads)
read_plan_kernel(Recipe c, Ranges r, uint64_t dst_bytes, uint32_t *__restrict__ first, uint32_t *__restrict__ pieces,
                 uint32_t *__restrict__ status)
{
    const uint64_t n = c.count(), R = r.count(), threads = (uint64_t)gridDim.x * kThreads;
    for (uint64_t k = (uint64_t)blockIdx.x * kThreads + threadIdx.x; k < r.max_ranges; k += threads) {
        uint32_t j0 = 0, cnt = 0;
        if (k < R) {
            const uint64_t a = r.off[k], len = r.len[k], to = r.dst[k];
            uint32_t verdict = 0;
            if (len) {
                verdict = 3;
                if (n && a + len >= a && to + len >= to && to + len <= dst_bytes && a >= c.raw_off[0] && a + len <= c.raw_off[n]) {
                    // off[j0] <= a < off[j0 + 1] and off[j1] <= a + len - 1 < off[j1 + 1]: both extents are non-empty
                    const uint64_t p0 = first_above(c.raw_off, n, a) - 1, p1 = first_above(c.raw_off, n, a + len - 1) - 1;
                    verdict = 0;
                    j0 = (uint32_t)p0;
                    cnt = p1 >= p0 ? (uint32_t)(p1 - p0 + 1) : 0u; // (a list out of contract: max_count < 2^32 either way)
                }
            }
            status[k] = verdict;
        }
        first[k] = j0;
        pieces[k] = cnt;
    }
}

// ---- a piece ------------------------------------------------------------------------------------------------------------------
// What position j means to range [a, a + len): restore_chunks_kernel's checks of the recipe and store_device.h's rule for the entry, with
// the range's destination check (made by the plan) in the place of the chunk's.
struct Piece {
    bool touched = false; // a non-empty (or decreasing) raw extent: an empty one is touched by no range
    bool refuse = true, raw = false, whole = false;
    uint64_t pos = 0, rs = 0;
    uint32_t stored = 0, len = 0;
    uint32_t lo = 0, n = 0; // the window: chunk bytes [lo, lo + n) are stream bytes of the range

    __device__ __forceinline__ void look(const Recipe &c, uint64_t j, uint64_t a, uint64_t alen)
    {
        const uint64_t r = c.ref[j], re = c.raw_off[j + 1], idx = r - c.dir_base;
        rs = c.raw_off[j];
        touched = rs != re;
        if (!touched) return;
        if (r >= c.dir_base && idx < c.dir_entries && rs < re && re - rs <= kMaxChunkBytes) {
            // Entry::sound (store_device.h) and `len != re - rs`, in this kernel's own spelling: cw_dev_read_ranges measured 1-2 %
            // slower over 4 KiB ranges with the lookup and the rule taken from the header, in either of two forms
            // (profiles/r22_store_device_ab.txt); tests/test_gpu_store_entry.py holds the two spellings together
            const uint4 e = c.dir[idx];
            pos = (uint64_t)e.y << 32 | e.x;
            stored = e.z;
            len = e.w & kLenMask;
            raw = (e.w & kRawFlag) != 0;
            refuse = (e.w & ~(kRawFlag | kLenMask)) != 0 || len == 0 || len > kMaxChunkBytes || len != re - rs || stored == 0 ||
                     (raw && stored != len) || pos > c.store_bytes || stored > c.store_bytes - pos;
        }
        if (refuse) return;
        const uint64_t end = a + alen, from = rs > a ? rs : a, till = re < end ? re : end; // (a + alen does not wrap: the plan)
        whole = a <= rs && re <= end;
        if (from < till) { lo = (uint32_t)(from - rs); n = (uint32_t)(till - from); }
    }
};

// 64 pieces at a time.  off[0 .. max_ranges] = the scan of the piece counts; piece p belongs to the range k with off[k] <= p < off[k + 1]
template <int ALG>
__global__ void __launch_bounds__(64)
read_pieces_kernel(Recipe c, Ranges r, const uint32_t *__restrict__ first_pos, const unsigned long long *__restrict__ off,
                   uint8_t *__restrict__ dst, uint32_t *__restrict__ status)
{
    const uint64_t total = off[r.max_ranges], lanes = (uint64_t)gridDim.x * 64;
    for (uint64_t first = (uint64_t)blockIdx.x * 64; first < total; first += lanes) { // (wave-uniform: the copies below need every lane)
        const uint64_t p = first + threadIdx.x;
        Piece q;
        uint64_t k = 0, to = 0; // to: where the chunk's byte 0 would go in dst (only ever used with the window added)
        if (p < total) {
            k = first_above(reinterpret_cast<const uint64_t *>(off), r.max_ranges, p) - 1;
            const uint64_t a = r.off[k];
            q.look(c, first_pos[k] + (p - off[k]), a, r.len[k]);
            to = r.dst[k] + (q.rs - a);
        }
        // (cw_dev_decompress_chunks skips a compressed extent above 2^24 bytes with status 1: the same verdict here)
        const bool decode = q.touched && !q.refuse && !q.raw && q.whole, skip = !decode || q.stored > (1u << 24);
        const bool bad = lane_decode<ALG>(c.store + (skip ? 0 : q.pos), skip ? 0u : q.stored, dst + (skip ? 0 : to), skip ? 0u : q.len, skip);
        if (q.touched && (q.refuse || (decode && bad))) atomicMax(status + k, q.refuse ? 2u : 1u);
        wave_copy(q.touched && !q.refuse && q.raw && q.n != 0, c.store, q.pos + q.lo, dst, to + q.lo, q.n);
    }
}

// Edge lane L < nbuf owns bufs + L * 64 KiB and takes the edge slots L, L + nbuf, ...  Slot 2k is the first piece of range k, slot
// 2k + 1 its last (none when the range has one piece).  The entry checks are the pieces kernel's, which has reported a refusal already.
// Only the first kEdgeLanes lanes of a wavefront are edge lanes (the copies use all 64): the buffers bound the number of decoders, and
// 16,384 of them as whole wavefronts would be one wavefront per compute unit, three of its four SIMDs idle.
constexpr uint32_t kEdgeLanes = 16;
static_assert(kEdgeLanes <= 64, "an edge lane's buffer is found by its index in the wavefront (wave_copy's from_slot)");
template <int ALG>
__global__ void __launch_bounds__(64)
read_edges_kernel(Recipe c, Ranges r, const uint32_t *__restrict__ first_pos, const uint32_t *__restrict__ pieces, uint8_t *__restrict__ bufs,
                  uint64_t nbuf, uint8_t *__restrict__ dst, uint32_t *__restrict__ status)
{
    const uint64_t slots = 2 * r.count(), lane = (uint64_t)blockIdx.x * kEdgeLanes + threadIdx.x;
    const bool mine = threadIdx.x < kEdgeLanes && lane < nbuf;
    uint8_t *buf = bufs + (mine ? lane : 0) * (uint64_t)kMaxChunkBytes;
    for (uint64_t first = 0; first < slots; first += nbuf) { // (wave-uniform: the copies below need every lane)
        const uint64_t s = first + lane, k = s >> 1;
        Piece q;
        uint64_t to = 0;
        if (mine && s < slots) {
            const uint32_t cnt = pieces[k];
            if (cnt > (uint32_t)(s & 1)) { // slot 2k + 1 only with two pieces or more
                const uint64_t a = r.off[k];
                q.look(c, (uint64_t)first_pos[k] + ((s & 1) ? cnt - 1 : 0u), a, r.len[k]);
                to = r.dst[k] + (q.rs - a);
            }
        }
        const bool decode = q.touched && !q.refuse && !q.raw && !q.whole, skip = !decode || q.stored > (1u << 24);
        const bool bad = lane_decode<ALG>(c.store + (skip ? 0 : q.pos), skip ? 0u : q.stored, buf, skip ? 0u : q.len, skip);
        if (decode && bad) atomicMax(status + k, 1u);
        // (a wavefront's own vector memory operations are performed in order: the fence only keeps the compiler from moving them)
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        // (a decoding lane is an edge lane: its buffer is the threadIdx.x-th of the wavefront's)
        wave_copy(decode && !bad && q.n != 0, bufs + (uint64_t)blockIdx.x * kEdgeLanes * kMaxChunkBytes, q.lo, dst, to + q.lo, q.n, kMaxChunkBytes);
    }
}

// per stream: the plan (a head of 64 bytes, the scan's offsets (u64, max_ranges + 1), first[] and pieces[] (u32) behind them) and the
// edge lanes' decode buffers
struct ReadSpace {
    DeviceBuf plan, bufs;
    size_t lane_limit = 0; // edge lanes an allocation that failed left this stream with (0: no limit met)
    void release()
    {
        lane_limit = 0;
        (void)plan.release();
        (void)bufs.release();
    }
};
StreamScratch<ReadSpace> read_spaces;
// 16,384 edge lanes (1 GiB of buffers): an eighth of the lanes the restore's grid keeps decoding (256 * 8 wavefronts of 64), spread
// over 1,024 wavefronts, one on every SIMD.  The restore's lane count would take 8 GiB of scratch per stream for the edges alone.
constexpr size_t kMaxEdgeLanes = 16384, kMinEdgeLanes = 64;

} // namespace

hipError_t read_ranges_launch(int lzf, const uint8_t *store, size_t store_bytes, const void *dir, uint64_t dir_base, size_t dir_entries,
                              const uint64_t *ref, const uint64_t *raw_offsets, const uint64_t *d_count, size_t max_count,
                              const uint64_t *range_off, const uint64_t *range_len, const uint64_t *range_dst, const uint64_t *d_nranges,
                              size_t max_ranges, uint8_t *dst, size_t dst_bytes, uint32_t *status, hipStream_t stream)
{
    if (max_ranges == 0) return hipSuccess;
    auto &w = read_spaces.at(stream);
    LaunchLock sequence(w.launch); // plan and buffers are shared by the launches below
    hipError_t e;
    const size_t plan_bytes = kScratchHead + (max_ranges + 1) * 8 + max_ranges * 8;
    // (a buffer is only replaced by a larger one: the queued launches of this stream that use the old one have to finish first)
    if (w.plan.bytes() && w.plan.bytes() < plan_bytes && (e = hipStreamSynchronize(stream)) != hipSuccess) return e;
    if ((e = w.plan.reserve(plan_bytes, 4096)) != hipSuccess) return e;
    // one buffer per edge slot, up to the cap; an allocation that fails is retried with half the lanes, down to 64
    size_t nbuf = 2 * max_ranges < kMaxEdgeLanes ? 2 * max_ranges : kMaxEdgeLanes;
    if (w.lane_limit && nbuf > w.lane_limit) nbuf = w.lane_limit;
    if (w.bufs.bytes() < nbuf * kMaxChunkBytes) {
        if (w.bufs.bytes() && (e = hipStreamSynchronize(stream)) != hipSuccess) return e;
        for (;;) {
            if ((e = w.bufs.reserve(nbuf * kMaxChunkBytes)) == hipSuccess) break;
            (void)hipGetLastError();
            if (nbuf <= kMinEdgeLanes) return hipErrorOutOfMemory;
            nbuf = nbuf / 2 < kMinEdgeLanes ? kMinEdgeLanes : nbuf / 2;
            w.lane_limit = nbuf;
        }
    }
    unsigned long long *off = reinterpret_cast<unsigned long long *>(w.plan.as<uint8_t>() + kScratchHead);
    uint32_t *first = reinterpret_cast<uint32_t *>(off + max_ranges + 1), *pieces = first + max_ranges;
    const Recipe c{store, (uint64_t)store_bytes, static_cast<const uint4 *>(dir), dir_base, (uint64_t)dir_entries, ref, raw_offsets, d_count,
                   (uint64_t)max_count};
    const Ranges r{range_off, range_len, range_dst, d_nranges, (uint64_t)max_ranges};

    hipLaunchKernelGGL(read_plan_kernel, dim3(lane_grid(max_ranges)), dim3(kThreads), 0, stream, c, r, (uint64_t)dst_bytes, first, pieces, status);
    // off[k] = sum of pieces[0..k) for k <= max_ranges
    if ((e = pack_launch(nullptr, 0, pieces, max_ranges, nullptr, reinterpret_cast<uint64_t *>(off), stream)) != hipSuccess) return e;
    // at most max_count pieces per range
    const size_t most = max_count && max_ranges > ((size_t)1 << 40) / max_count ? (size_t)1 << 40 : max_ranges * max_count;
    const unsigned grid = decode_grid(most);
    const size_t edge_grid = (nbuf + kEdgeLanes - 1) / kEdgeLanes;
    if (grid && lzf) {
        hipLaunchKernelGGL(read_pieces_kernel<1>, dim3(grid), dim3(64), 0, stream, c, r, first, off, dst, status);
        hipLaunchKernelGGL(read_edges_kernel<1>, dim3((unsigned)edge_grid), dim3(64), 0, stream, c, r, first, pieces, w.bufs.as<uint8_t>(),
                           (uint64_t)nbuf, dst, status);
    } else if (grid) {
        hipLaunchKernelGGL(read_pieces_kernel<0>, dim3(grid), dim3(64), 0, stream, c, r, first, off, dst, status);
        hipLaunchKernelGGL(read_edges_kernel<0>, dim3((unsigned)edge_grid), dim3(64), 0, stream, c, r, first, pieces, w.bufs.as<uint8_t>(),
                           (uint64_t)nbuf, dst, status);
    }
    return hipGetLastError();
}

size_t read_ranges_scratch_bytes(size_t max_ranges)
{
    const size_t nbuf = 2 * max_ranges < kMaxEdgeLanes ? 2 * max_ranges : kMaxEdgeLanes;
    return max_ranges ? kScratchHead + 8 + 16 * max_ranges + nbuf * kMaxChunkBytes : 0;
}

} // namespace cw
