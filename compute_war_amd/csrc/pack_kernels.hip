// pack_kernels.hip -- packed output stream: the compressed blocks leave the codec kernels in
// fixed-stride slots (slot i at dst + i * dst_stride, sizes[i] bytes used); this turns them into one contiguous
// stream plus a block index: offsets[i] = sum of sizes[0..i) as u64, offsets[nblocks] = total.  A block that did
// not fit (sizes[i] == 0, LZF) occupies no bytes in the stream -- its index entry is empty and the caller keeps the
// raw block, as the reference's callers do (HashAndCompress.cpp:247-252).
//
// Three small kernels for the exclusive scan (tile sums, scan of the tile sums by one workgroup, tile offsets) and
// one copy kernel: a wavefront per slot, 16-byte aligned stores fed by unaligned loads.  The host batch API uses
// the packed stream to bring a whole batch back in ONE device-to-host copy instead of one per block.
//
// cw_dev_pack_chunks is the same scan and copy for the chunk codecs' slots (chunk_codec_kernels.hip): the count is read on the device
// and a position's slot is found through cw_chunk_slot_offset instead of a stride.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cw_device.h"
#include "lz_device.h"
#include "stream_scratch.h"

namespace cw {

namespace {

constexpr unsigned kTile = 4096, kThreads = 256, kPerThread = kTile / kThreads;

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v)
{
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

__device__ __forceinline__ void tile_sums(const uint32_t *__restrict__ sizes, size_t n, unsigned long long *__restrict__ partial)
{
    __shared__ unsigned long long wsum[kThreads / 64];
    const size_t base = (size_t)blockIdx.x * kTile;
    unsigned long long s = 0;
    for (unsigned k = 0; k < kPerThread; k++) {
        const size_t i = base + k * kThreads + threadIdx.x;
        if (i < n) s += sizes[i];
    }
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

__global__ void __launch_bounds__(kThreads)
tile_sums_kernel(const uint32_t *__restrict__ sizes, size_t n, unsigned long long *__restrict__ partial)
{
    tile_sums(sizes, n, partial);
}

// one workgroup: exclusive scan of the tile sums in place
__global__ void __launch_bounds__(kThreads)
scan_partials_kernel(unsigned long long *__restrict__ partial, size_t ntiles)
{
    __shared__ unsigned long long buf[kThreads];
    unsigned long long carry = 0;
    for (size_t base = 0; base < ntiles; base += kThreads) {
        const size_t i = base + threadIdx.x;
        const unsigned long long v = i < ntiles ? partial[i] : 0;
        buf[threadIdx.x] = v;
        __syncthreads();
        for (unsigned d = 1; d < kThreads; d <<= 1) { // Hillis-Steele inclusive scan
            const unsigned long long add = threadIdx.x >= d ? buf[threadIdx.x - d] : 0;
            __syncthreads();
            buf[threadIdx.x] += add;
            __syncthreads();
        }
        if (i < ntiles) partial[i] = carry + buf[threadIdx.x] - v;
        carry += buf[kThreads - 1];
        __syncthreads();
    }
}

__device__ __forceinline__ void tile_offsets(const uint32_t *__restrict__ sizes, size_t n, const unsigned long long *__restrict__ partial,
                                             unsigned long long *__restrict__ offsets)
{
    __shared__ unsigned long long buf[kThreads];
    // thread t owns kPerThread consecutive entries of the tile
    const size_t first = (size_t)blockIdx.x * kTile + (size_t)threadIdx.x * kPerThread;
    uint32_t v[kPerThread];
    unsigned long long s = 0;
    for (unsigned k = 0; k < kPerThread; k++) {
        v[k] = first + k < n ? sizes[first + k] : 0;
        s += v[k];
    }
    buf[threadIdx.x] = s;
    __syncthreads();
    for (unsigned d = 1; d < kThreads; d <<= 1) {
        const unsigned long long add = threadIdx.x >= d ? buf[threadIdx.x - d] : 0;
        __syncthreads();
        buf[threadIdx.x] += add;
        __syncthreads();
    }
    unsigned long long off = partial[blockIdx.x] + buf[threadIdx.x] - s;
    for (unsigned k = 0; k < kPerThread; k++) {
        if (first + k < n) offsets[first + k] = off;
        off += v[k];
        if (first + k + 1 == n) offsets[n] = off; // total
    }
}

__global__ void __launch_bounds__(kThreads)
tile_offsets_kernel(const uint32_t *__restrict__ sizes, size_t n, const unsigned long long *__restrict__ partial,
                    unsigned long long *__restrict__ offsets)
{
    tile_offsets(sizes, n, partial, offsets);
}

__global__ void __launch_bounds__(64)
pack_copy_kernel(const uint8_t *__restrict__ slots, size_t slot_stride, const uint32_t *__restrict__ sizes,
                 const unsigned long long *__restrict__ offsets, size_t n, uint8_t *__restrict__ out)
{
    const uint32_t lane = threadIdx.x;
    for (size_t i = blockIdx.x; i < n; i += gridDim.x) {
        const uint32_t len = sizes[i];
        if (len) lz::copy_g2g(out + offsets[i], slots + i * slot_stride, len, lane);
    }
}

// ---- the same for chunk slots (cw_dev_pack_chunks): the count n = min(*d_count, max_count) is read on the device, the grids are
// sized from max_count, sizes behind n count as 0 (tiles behind n sum to 0) and offsets behind entry n are not written ----
__global__ void __launch_bounds__(kThreads)
chunk_tile_sums_kernel(const uint32_t *__restrict__ sizes, const uint64_t *__restrict__ d_count, size_t max_count,
                       unsigned long long *__restrict__ partial)
{
    const size_t n = *d_count < max_count ? (size_t)*d_count : max_count;
    tile_sums(sizes, n, partial);
}

__global__ void __launch_bounds__(kThreads)
chunk_tile_offsets_kernel(const uint32_t *__restrict__ sizes, const uint64_t *__restrict__ d_count, size_t max_count,
                          const unsigned long long *__restrict__ partial, unsigned long long *__restrict__ offsets)
{
    const size_t n = *d_count < max_count ? (size_t)*d_count : max_count;
    if (n == 0 && blockIdx.x == 0 && threadIdx.x == 0) offsets[0] = 0;
    tile_offsets(sizes, n, partial, offsets);
}

// position i's bytes are in the slot of chunk sel[i] (chunk i without a selection); a position of size 0 has no slot to look at
__global__ void __launch_bounds__(64)
chunk_pack_copy_kernel(const uint8_t *__restrict__ slots, bool lz4, const uint64_t *__restrict__ chunk_offsets, const uint32_t *__restrict__ sel,
                       const uint32_t *__restrict__ sizes, const unsigned long long *__restrict__ offsets, const uint64_t *__restrict__ d_count,
                       size_t max_count, uint8_t *__restrict__ out)
{
    const size_t n = *d_count < max_count ? (size_t)*d_count : max_count;
    const uint32_t lane = threadIdx.x;
    for (size_t i = blockIdx.x; i < n; i += gridDim.x) {
        const uint32_t len = sizes[i];
        if (len == 0) continue;
        const uint64_t c = sel ? sel[i] : i;
        lz::copy_g2g(out + offsets[i], slots + chunk_slot_offset(lz4, chunk_offsets[c], c), len, lane);
    }
}

StreamScratch<DeviceBuf> partials; // per stream: the tile sums

} // namespace

hipError_t pack_launch(const uint8_t *slots, size_t slot_stride, const uint32_t *sizes, size_t nblocks, uint8_t *packed,
                       uint64_t *offsets, hipStream_t stream)
{
    if (nblocks == 0) return hipMemsetAsync(offsets, 0, sizeof(uint64_t), stream);
    const size_t ntiles = (nblocks + kTile - 1) / kTile;
    auto &w = partials.at(stream);
    LaunchLock sequence(w.launch); // the tile partials are shared by the launches below
    const hipError_t e = w.reserve(ntiles * sizeof(unsigned long long), 1024 * sizeof(unsigned long long));
    if (e != hipSuccess) return e;
    unsigned long long *partial = w.as<unsigned long long>();
    unsigned long long *off = reinterpret_cast<unsigned long long *>(offsets);
    hipLaunchKernelGGL(tile_sums_kernel, dim3((unsigned)ntiles), dim3(kThreads), 0, stream, sizes, nblocks, partial);
    hipLaunchKernelGGL(scan_partials_kernel, dim3(1), dim3(kThreads), 0, stream, partial, ntiles);
    hipLaunchKernelGGL(tile_offsets_kernel, dim3((unsigned)ntiles), dim3(kThreads), 0, stream, sizes, nblocks, partial, off);
    if (packed) {
        const size_t grid = nblocks < 256 * 32 ? nblocks : 256 * 32;
        hipLaunchKernelGGL(pack_copy_kernel, dim3((unsigned)grid), dim3(64), 0, stream, slots, slot_stride, sizes, off, nblocks, packed);
    }
    return hipGetLastError();
}

hipError_t chunk_pack_launch(int lzf, const uint8_t *slots, const uint64_t *chunk_offsets, const uint32_t *sel, const uint64_t *d_count,
                             size_t max_count, const uint32_t *sizes, uint8_t *packed, uint64_t *offsets, hipStream_t stream)
{
    if (max_count == 0) return hipMemsetAsync(offsets, 0, sizeof(uint64_t), stream);
    const size_t ntiles = (max_count + kTile - 1) / kTile;
    auto &w = partials.at(stream);
    LaunchLock sequence(w.launch); // the tile partials are shared by the launches below
    const hipError_t e = w.reserve(ntiles * sizeof(unsigned long long), 1024 * sizeof(unsigned long long));
    if (e != hipSuccess) return e;
    unsigned long long *partial = w.as<unsigned long long>();
    unsigned long long *off = reinterpret_cast<unsigned long long *>(offsets);
    hipLaunchKernelGGL(chunk_tile_sums_kernel, dim3((unsigned)ntiles), dim3(kThreads), 0, stream, sizes, d_count, max_count, partial);
    hipLaunchKernelGGL(scan_partials_kernel, dim3(1), dim3(kThreads), 0, stream, partial, ntiles);
    hipLaunchKernelGGL(chunk_tile_offsets_kernel, dim3((unsigned)ntiles), dim3(kThreads), 0, stream, sizes, d_count, max_count, partial, off);
    if (packed) {
        const size_t grid = max_count < 256 * 32 ? max_count : 256 * 32;
        hipLaunchKernelGGL(chunk_pack_copy_kernel, dim3((unsigned)grid), dim3(64), 0, stream, slots, lzf == 0, chunk_offsets, sel, sizes, off,
                           d_count, max_count, packed);
    }
    return hipGetLastError();
}

} // namespace cw
