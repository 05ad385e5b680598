// patch_kernels.hip -- the device step of an in-place edit: cw_dev_cdc_resync finds, among the cuts of a
// re-chunked window, the first one behind the edit that lands on a cut of the old stream, and shortens the window's chunk count to
// it on the device, so that the hash, the dedupe, the codec and the append queued behind it work on exactly the kept chunks.
//
// Two steps behind a kernel boundary.  The search: one lane per new cut t in [1, N]; a cut at or behind new_from looks its shifted
// position up in the old cuts by binary search (the lowest s with old[s] >= the position), and the lowest t that hits goes through a
// wavefront minimum, a workgroup minimum and one atomicMin per workgroup into the scratch head, which the host preset to all ones.
// The finish: one lane reads the minimum, repeats the one search for s, and writes the result and the count.  Both counts are read
// on the device and clamped; no load leaves new[0 .. max_new] or old[0 .. max_old].
//
// Scratch, per stream: the 64-byte head (the minimum at [0]).

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cw_device.h"
#include "store_device.h"

namespace cw {

namespace {

using namespace chunkstore;

typedef unsigned long long u64;
constexpr u64 kNone = ~0ull;

// the lowest s in [0, count] with old[s] >= x, or count + 1 when there is none (old[0 .. count] ascending)
__device__ __forceinline__ uint64_t lower_bound(const uint64_t *__restrict__ old, uint64_t count, uint64_t x)
{
    uint64_t lo = 0, hi = count + 1;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (old[mid] < x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ u64 wave_min(u64 v)
{
    for (int off = 32; off > 0; off >>= 1) {
        const u64 o = __shfl_down(v, off, 64);
        v = o < v ? o : v;
    }
    return v;
}

__global__ void __launch_bounds__(kThreads)
resync_search_kernel(const uint64_t *__restrict__ fresh, const uint64_t *__restrict__ d_new_count, uint64_t max_new,
                     const uint64_t *__restrict__ old, const uint64_t *__restrict__ d_old_count, uint64_t max_old, uint64_t new_from,
                     uint64_t shift, u64 *__restrict__ best)
{
    __shared__ u64 wmin[kThreads / 64];
    const uint64_t n = umin64(*d_new_count, max_new), o = umin64(*d_old_count, max_old);
    const uint64_t threads = (uint64_t)gridDim.x * kThreads;
    u64 mine = kNone;
    // (ascending t per lane: the first hit is the lane's lowest)
    for (uint64_t t = 1 + (uint64_t)blockIdx.x * kThreads + threadIdx.x; t <= n && mine == kNone; t += threads) {
        const uint64_t x = fresh[t];
        if (x < new_from) continue;
        const uint64_t s = lower_bound(old, o, x + shift);
        if (s <= o && old[s] == x + shift) mine = t;
    }
    mine = wave_min(mine);
    if ((threadIdx.x & 63u) == 0) wmin[threadIdx.x >> 6] = mine;
    __syncthreads();
    if (threadIdx.x != 0) return;
    u64 all = kNone;
    for (uint32_t w = 0; w < kThreads / 64; w++) all = wmin[w] < all ? wmin[w] : all;
    if (all != kNone) atomicMin(best, all);
}

// result = {verdict, t, s, new[t]}; found: *d_new_count = t; not found: *d_new_count = 0 unless keep_all
__global__ void resync_finish_kernel(const uint64_t *__restrict__ fresh, uint64_t *__restrict__ d_new_count, uint64_t max_new,
                                     const uint64_t *__restrict__ old, const uint64_t *__restrict__ d_old_count, uint64_t max_old,
                                     uint64_t shift, uint32_t keep_all, const u64 *__restrict__ best, uint64_t *__restrict__ result)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const uint64_t n = umin64(*d_new_count, max_new), o = umin64(*d_old_count, max_old), t = *best;
    if (t >= 1 && t <= n) {
        const uint64_t x = fresh[t];
        result[0] = 0;
        result[1] = t;
        result[2] = umin64(lower_bound(old, o, x + shift), o);
        result[3] = x;
        *d_new_count = t;
        return;
    }
    result[0] = 1;
    result[1] = 0;
    result[2] = 0;
    result[3] = 0;
    if (!keep_all) *d_new_count = 0;
}

StreamScratch<DeviceBuf> resync_spaces; // per stream: the head, with the minimum at [0]

} // namespace

hipError_t cdc_resync_launch(const uint64_t *new_offsets, uint64_t *d_new_count, size_t max_new, const uint64_t *old_offsets,
                             const uint64_t *d_old_count, size_t max_old, uint64_t new_from, uint64_t shift, int keep_all, uint64_t *result,
                             hipStream_t stream)
{
    auto &w = resync_spaces.at(stream);
    LaunchLock sequence(w.launch); // the minimum is shared by the launches below
    hipError_t e = w.reserve(kScratchHead, (size_t)1 << 20);
    if (e != hipSuccess) return e;
    u64 *best = w.as<u64>();
    if ((e = hipMemsetAsync(best, 0xFF, kScratchHead, stream)) != hipSuccess) return e;
    if (max_new)
        hipLaunchKernelGGL(resync_search_kernel, dim3(lane_grid(max_new)), dim3(kThreads), 0, stream, new_offsets, d_new_count, (uint64_t)max_new,
                           old_offsets, d_old_count, (uint64_t)max_old, new_from, shift, best);
    hipLaunchKernelGGL(resync_finish_kernel, dim3(1), dim3(64), 0, stream, new_offsets, d_new_count, (uint64_t)max_new, old_offsets, d_old_count,
                       (uint64_t)max_old, shift, keep_all ? 1u : 0u, best, result);
    return hipGetLastError();
}

} // namespace cw
