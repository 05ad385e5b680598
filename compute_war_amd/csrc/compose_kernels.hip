// compose_kernels.hip -- the device steps of composing a stream from stored ranges and new bytes.
// cw_dev_cdc_resync_windows is cw_dev_cdc_resync over many windows chunked in one cw_dev_cdc_streams call: for every window, the
// first of its cuts behind new_from that lands on one of the old cuts the window may keep.  It changes no count: a round of
// cw_store_compose only chunks.  cw_dev_scatter_extents copies extents between two device buffers (the new bytes of the windows
// out of the uploaded payload), checked as cw_dev_apply_delta checks its ops and tiled by bytes as its copy is.
//
// The resync, two steps behind a kernel boundary.  The search: one lane per new cut g in [1, N]; the lane finds its window by
// binary search in the stream index (the smallest w with first[w + 1] >= g, so g = first[w + 1] is w's last cut and never w + 1's
// cut 0), skips the last cut unless the window is final, and looks x + shift up in the window's own old range.  Lanes ascend with
// g and windows are runs of g, so among the hits of a wavefront the lowest of a window is the one whose nearest lower hit lies in
// another window: only that lane does the atomicMin on the window's scratch word, which the host preset to all ones.  The finish:
// one lane per window reads the minimum, repeats the one search for s and writes the window's four words.
// The count and every index read from the lists are clamped: no load leaves new[0 .. max_new], first[0 .. nwin], win[0 .. nwin) or
// old[0 .. max_old).
//
// The scatter: a check, one lane per extent, whose lowest bad extent lands in result[2] by atomicMin; then the copy, a wavefront
// per tile of the DESTINATION BUFFER (16 KiB): the tile's first extent by binary search over the ascending destinations, then 64
// extents at a time, each lane clipping one to the tile (store_device.h: wave_copy).  A tile no extent touches costs its search.
//
// Scratch of the resync, per stream: 64 + 8 * nwin bytes (a head and the minima).  The scatter keeps none.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cw_device.h"
#include "lz_device.h"
#include "store_device.h"

namespace cw {

namespace {

using namespace chunkstore;

typedef unsigned long long u64;
constexpr u64 kNone = ~0ull;

// cw_resync_window
struct Window {
    uint64_t new_from, shift, old_first, old_count, final_;
    __device__ __forceinline__ explicit Window(const uint64_t *__restrict__ p) : new_from(p[0]), shift(p[1]), old_first(p[2]), old_count(p[3]), final_(p[4]) {}
};

// the lowest i in [0, n) with list[i] >= x, n when there is none (list ascending)
__device__ __forceinline__ uint64_t lower_bound(const uint64_t *__restrict__ list, uint64_t n, uint64_t x)
{
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if (list[mid] < x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// the window's old range clamped into old[0 .. max_old): its first index and its count
__device__ __forceinline__ void old_range(const Window &w, uint64_t max_old, uint64_t &lo, uint64_t &n)
{
    lo = umin64(w.old_first, max_old);
    n = umin64(w.old_count, max_old - lo);
}

__global__ void __launch_bounds__(kThreads)
windows_search_kernel(const uint64_t *__restrict__ fresh, const uint64_t *__restrict__ d_new_count, uint64_t max_new,
                      const uint64_t *__restrict__ first, const uint64_t *__restrict__ win, uint64_t nwin, const uint64_t *__restrict__ old,
                      uint64_t max_old, u64 *__restrict__ best)
{
    const uint64_t n = umin64(*d_new_count, max_new), threads = (uint64_t)gridDim.x * kThreads;
    const uint32_t lane = threadIdx.x & 63u;
    // (the trip count is the workgroup's: every lane of a wavefront takes part in the ballot and the shuffle)
    for (uint64_t at = (uint64_t)blockIdx.x * kThreads; at < n; at += threads) {
        const uint64_t g = at + threadIdx.x + 1;
        bool hit = false;
        uint64_t w = 0;
        if (g <= n) {
            w = lower_bound(first + 1, nwin, g); // the smallest w with first[w + 1] >= g
            if (w < nwin) {
                const Window me(win + 5 * w);
                const bool last = umin64(first[w + 1], n) == g;
                const uint64_t x = fresh[g];
                if ((!last || me.final_) && x >= me.new_from) {
                    uint64_t lo, count;
                    old_range(me, max_old, lo, count);
                    const uint64_t s = lower_bound(old + lo, count, x + me.shift);
                    hit = s < count && old[lo + s] == x + me.shift;
                }
            }
        }
        const u64 hits = __ballot(hit), below = hits & ((1ull << lane) - 1);
        const int prev = below ? 63 - __clzll((long long)below) : (int)lane;
        const uint64_t w_prev = __shfl((unsigned long long)w, prev, 64);
        if (hit && (!below || w_prev != w)) atomicMin(best + w, (u64)g);
    }
}

// result[4 * w ..] = {verdict, t, s, new[first[w] + t]}
__global__ void __launch_bounds__(kThreads)
windows_finish_kernel(const uint64_t *__restrict__ fresh, const uint64_t *__restrict__ d_new_count, uint64_t max_new,
                      const uint64_t *__restrict__ first, const uint64_t *__restrict__ win, uint64_t nwin, const uint64_t *__restrict__ old,
                      uint64_t max_old, const u64 *__restrict__ best, uint64_t *__restrict__ result)
{
    const uint64_t n = umin64(*d_new_count, max_new), threads = (uint64_t)gridDim.x * kThreads;
    for (uint64_t w = (uint64_t)blockIdx.x * kThreads + threadIdx.x; w < nwin; w += threads) {
        const uint64_t g = best[w], from = umin64(first[w], n);
        uint64_t v = 1, t = 0, s = 0, x = 0;
        if (g >= 1 && g <= n && g > from) {
            const Window me(win + 5 * w);
            uint64_t lo, count;
            old_range(me, max_old, lo, count);
            x = fresh[g];
            v = 0;
            t = g - from;
            s = lo + umin64(lower_bound(old + lo, count, x + me.shift), count);
        }
        result[4 * w] = v;
        result[4 * w + 1] = t;
        result[4 * w + 2] = s;
        result[4 * w + 3] = x;
    }
}

StreamScratch<DeviceBuf> windows_spaces; // per stream: the head, then a minimum per window

// ---- the scatter --------------------------------------------------------------------------------------------------------------------
struct Extent {
    uint64_t src_off, dst_off, len;
    __device__ __forceinline__ explicit Extent(const uint64_t *__restrict__ p) : src_off(p[0]), dst_off(p[1]), len(p[2]) {}
};

// result[2] (preset to all ones) = the lowest extent that is bad: it is empty, it leaves a buffer or wraps, or it starts in front of
// the end of the one before
__global__ void __launch_bounds__(kThreads)
scatter_check_kernel(const uint64_t *__restrict__ ext, const uint64_t *__restrict__ d_n, uint64_t max_n, uint64_t src_bytes, uint64_t dst_bytes,
                     u64 *__restrict__ result)
{
    const uint64_t n = umin64(*d_n, max_n), threads = (uint64_t)gridDim.x * kThreads;
    uint64_t lowest = kNone;
    for (uint64_t k = (uint64_t)blockIdx.x * kThreads + threadIdx.x; k < n; k += threads) {
        const Extent e(ext + 3 * k);
        bool good = e.len != 0 && e.len <= src_bytes && e.src_off <= src_bytes - e.len && e.len <= dst_bytes && e.dst_off <= dst_bytes - e.len;
        if (k) { // (the one before may itself be bad: then it is the lower of the two)
            const Extent b(ext + 3 * (k - 1));
            good = good && b.dst_off + b.len >= b.dst_off && e.dst_off >= b.dst_off + b.len;
        }
        if (!good && lowest == kNone) lowest = k;
    }
    if (lowest != kNone) atomicMin(result + 2, (u64)lowest);
}

// the largest k in [0, n) with ext[k].dst_off <= x, 0 when there is none (checked list: the destinations ascend)
__device__ __forceinline__ uint64_t extent_at(const uint64_t *__restrict__ ext, uint64_t n, uint64_t x)
{
    uint64_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if (ext[3 * mid + 1] <= x) lo = mid;
        else hi = mid;
    }
    return lo;
}

// A wavefront per tile of the destination buffer, grid-stride.  Every wavefront reaches the verdict on its own, from result[2], and
// returns at once unless it is 0; thread 0 of workgroup 0 writes result[0], [1] and [3].
__global__ void __launch_bounds__(64)
scatter_copy_kernel(const uint8_t *__restrict__ src, const uint64_t *__restrict__ ext, const uint64_t *__restrict__ d_n, uint64_t max_n,
                    uint8_t *__restrict__ dst, uint64_t dst_bytes, uint32_t tile_shift, uint64_t *__restrict__ result)
{
    const uint64_t n = umin64(*d_n, max_n);
    const bool bad = result[2] != kNone;
    // (checked list: the last extent ends inside the destination, and no extent lies behind it)
    const uint64_t reach = bad || n == 0 ? 0 : ext[3 * (n - 1) + 1] + ext[3 * (n - 1) + 2];
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        result[0] = bad ? 1 : 0;
        result[1] = reach;
        result[3] = n;
    }
    if (bad || n == 0) return;
    const uint64_t tile = (uint64_t)1 << tile_shift, begin = ext[1] >> tile_shift, tiles = (umin64(reach, dst_bytes) + tile - 1) >> tile_shift;
    for (uint64_t w = begin + blockIdx.x; w < tiles; w += gridDim.x) { // (wave-uniform: the copies below need every lane)
        const uint64_t t0 = w << tile_shift, t1 = t0 + tile;
        for (uint64_t at = extent_at(ext, n, t0); at < n; at += 64) {
            const uint64_t k = at + threadIdx.x;
            bool have = false, behind = true;
            uint64_t from = 0, to = 0;
            uint32_t len = 0;
            if (k < n) {
                const Extent e(ext + 3 * k);
                const uint64_t lo = e.dst_off > t0 ? e.dst_off : t0, hi = umin64(e.dst_off + e.len, t1);
                behind = e.dst_off >= t1;
                have = lo < hi;
                if (have) {
                    from = e.src_off + (lo - e.dst_off);
                    to = lo;
                    len = (uint32_t)(hi - lo); // (at most a tile)
                }
            }
            wave_copy(have, src, from, dst, to, len);
            if (__ballot(behind)) break; // the destinations ascend: nothing behind this lane's extent touches the tile
        }
    }
}

} // namespace

hipError_t cdc_resync_windows_launch(const uint64_t *new_offsets, const uint64_t *d_new_count, size_t max_new, const uint64_t *stream_first,
                                     const void *win, size_t nwin, const uint64_t *old_offsets, size_t max_old, uint64_t *result, hipStream_t stream)
{
    if (nwin == 0) return hipSuccess;
    auto &w = windows_spaces.at(stream);
    LaunchLock sequence(w.launch); // the minima are shared by the launches below
    hipError_t e = w.reserve(kScratchHead + nwin * 8, (size_t)1 << 20);
    if (e != hipSuccess) return e;
    u64 *best = reinterpret_cast<u64 *>(w.as<uint8_t>() + kScratchHead);
    if ((e = hipMemsetAsync(best, 0xFF, nwin * 8, stream)) != hipSuccess) return e;
    const uint64_t *list = static_cast<const uint64_t *>(win);
    if (max_new)
        hipLaunchKernelGGL(windows_search_kernel, dim3(lane_grid(max_new)), dim3(kThreads), 0, stream, new_offsets, d_new_count, (uint64_t)max_new,
                           stream_first, list, (uint64_t)nwin, old_offsets, (uint64_t)max_old, best);
    hipLaunchKernelGGL(windows_finish_kernel, dim3(lane_grid(nwin)), dim3(kThreads), 0, stream, new_offsets, d_new_count, (uint64_t)max_new,
                       stream_first, list, (uint64_t)nwin, old_offsets, (uint64_t)max_old, best, result);
    return hipGetLastError();
}

hipError_t scatter_extents_launch(const uint8_t *src, size_t src_bytes, const uint64_t *ext, const uint64_t *d_n, size_t max_n, uint8_t *dst,
                                  size_t dst_bytes, uint64_t *result, hipStream_t stream)
{
    constexpr unsigned kTileShift = 14; // 16 KiB, one round of copy_g2g's loads: cw_dev_apply_delta's default tile
    hipError_t e = hipMemsetAsync(result, 0xFF, 4 * sizeof(uint64_t), stream); // (result[2]: no bad extent yet)
    if (e != hipSuccess) return e;
    if (max_n)
        hipLaunchKernelGGL(scatter_check_kernel, dim3(lane_grid(max_n)), dim3(kThreads), 0, stream, ext, d_n, (uint64_t)max_n, (uint64_t)src_bytes,
                           (uint64_t)dst_bytes, reinterpret_cast<u64 *>(result));
    const size_t tiles = (dst_bytes + ((size_t)1 << kTileShift) - 1) >> kTileShift;
    hipLaunchKernelGGL(scatter_copy_kernel, dim3(wave_grid(tiles ? tiles : 1)), dim3(64), 0, stream, src, ext, d_n, (uint64_t)max_n, dst,
                       (uint64_t)dst_bytes, kTileShift, result);
    return hipGetLastError();
}

} // namespace cw
