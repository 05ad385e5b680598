// replicate_kernels.hip -- chunk bundles between stores: cw_dev_store_export_chunks takes the stored bytes of
// the entries a list of values names out of a store, back to back and with a cw_chunk_loc each; cw_dev_store_import_chunks appends
// such extents to another store under new values; cw_dev_translate_refs rewrites a recipe from the sender's values to the
// receiver's; cw_dev_store_replace_chunks is the import with the values given instead of counted up from a
// base, for chunks that come back under the values they had.  Nothing decodes: extents move in their stored form.  Nothing here keeps
// state between calls.
//
// Export and import mirror the append of restore_kernels.hip: per position its stored size (0 when the position is refused) with
// the refusal flags; the index-only pack scan over those sizes; a wavefront-per-position copy that also writes the position's entry;
// one thread that reports (and, for the import, moves the cursor).  Copy and finish evaluate the same verdict, so a call that is
// refused changes nothing.  An entry is checked against the buffer it points into before anything is loaded through it, and the copy
// runs only when every position passed.  Everything that one kernel reads of another's output lies behind a kernel boundary.
//
// Translate: one lane per recipe position, a binary search in the ascending list of pairs; the misses are counted, one atomic per
// workgroup.
//
// Scratch of export and import, per stream: 72 + 12 * max_count bytes -- a 64-byte head (the flag word at [0]), the scan's offsets
// (u64, max_count + 1) and the sizes (u32) behind them.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cw_device.h"
#include "store_device.h"

namespace cw {

namespace {

using namespace chunkstore;

constexpr uint32_t kUnsound = 1u, kOutside = 2u, kLength = 4u; // the head's flag word

// ---- export ------------------------------------------------------------------------------------------------------------------
// sizes[k] = the stored bytes of the entry values[k] names, 0 and the flag when it names none or an unsound one
__global__ void __launch_bounds__(kThreads)
export_sizes_kernel(const uint4 *__restrict__ dir, uint64_t dir_base, uint64_t dir_entries, uint64_t store_bytes, const uint64_t *__restrict__ values,
                    const uint64_t *__restrict__ d_count, uint64_t max_count, uint32_t *__restrict__ sizes, uint32_t *__restrict__ flags)
{
    const uint64_t n = umin64(*d_count, max_count), threads = (uint64_t)gridDim.x * kThreads;
    bool bad = false;
    for (uint64_t k = (uint64_t)blockIdx.x * kThreads + threadIdx.x; k < n; k += threads) {
        uint64_t idx;
        uint32_t s = 0;
        if (names_entry(values[k], dir_base, dir_entries, idx)) {
            const Entry e(dir[idx]);
            if (e.sound(store_bytes)) s = e.stored;
        }
        sizes[k] = s;
        bad |= s == 0;
    }
    if (bad) atomicOr(flags, kUnsound);
}

__device__ __forceinline__ uint32_t export_verdict(uint32_t flags, uint64_t total, uint64_t out_bytes)
{
    if (flags) return 2u;
    return total > out_bytes ? 1u : 0u;
}

// a wavefront per position: the entry's stored bytes to out + off[k], then out_loc[k]
__global__ void __launch_bounds__(64)
export_copy_kernel(const uint8_t *__restrict__ store, const uint4 *__restrict__ dir, uint64_t dir_base, uint64_t dir_entries,
                   const uint64_t *__restrict__ values, const uint64_t *__restrict__ d_count, uint64_t max_count,
                   const unsigned long long *__restrict__ off, const uint32_t *__restrict__ flags, uint8_t *__restrict__ out, uint64_t out_bytes,
                   uint4 *__restrict__ out_loc)
{
    const uint64_t n = umin64(*d_count, max_count);
    if (export_verdict(*flags, off[n], out_bytes)) return;
    for (uint64_t k = blockIdx.x; k < n; k += gridDim.x) {
        uint64_t idx;
        if (!names_entry(values[k], dir_base, dir_entries, idx)) continue; // (no flag: every position names a sound entry)
        const Entry e(dir[idx]);
        const uint64_t to = off[k];
        lz::copy_g2g(out + to, store + e.pos, e.stored, threadIdx.x);
        if (threadIdx.x == 0) out_loc[k] = e.at(to);
    }
}

__global__ void __launch_bounds__(64)
export_finish_kernel(const uint64_t *__restrict__ d_count, uint64_t max_count, const unsigned long long *__restrict__ off,
                     const uint32_t *__restrict__ flags, uint64_t out_bytes, uint64_t *__restrict__ result)
{
    if (threadIdx.x != 0) return;
    const uint64_t n = umin64(*d_count, max_count), total = off[n];
    result[0] = export_verdict(*flags, total, out_bytes);
    result[1] = total;
    result[2] = n;
}

// ---- import ------------------------------------------------------------------------------------------------------------------
// the selected positions of a bundle of min(*d_count, max_count) chunks: position j is chunk sel[j] (sel == NULL: chunk j)
struct Selection {
    const uint64_t *d_count;
    const uint32_t *sel;
    const uint64_t *d_nsel;
    uint64_t max_count;
    __device__ __forceinline__ uint64_t nchunks() const { return umin64(*d_count, max_count); }
    __device__ __forceinline__ uint64_t npos() const { return sel ? umin64(*d_nsel, max_count) : nchunks(); }
    __device__ __forceinline__ uint64_t chunk(uint64_t j) const { return sel ? sel[j] : j; }
};

// (Directory d: values == NULL is the import, chunk k carries base + k; else the replace, position k carries values[k])
// sizes[j] = the stored bytes of position j's chunk, 0 and kUnsound when the bundle has no such chunk or its entry is unsound or
// leaves in_bytes; kOutside when a sound position's value has no directory entry; kLength when the replace would change the length
// of the entry it names
__global__ void __launch_bounds__(kThreads)
import_sizes_kernel(const uint4 *__restrict__ in_loc, uint64_t in_bytes, Selection c, Directory d, uint32_t *__restrict__ sizes,
                    uint32_t *__restrict__ flags)
{
    const uint64_t n = c.nchunks(), npos = c.npos(), threads = (uint64_t)gridDim.x * kThreads;
    uint32_t mine = 0;
    for (uint64_t j = (uint64_t)blockIdx.x * kThreads + threadIdx.x; j < npos; j += threads) {
        const uint64_t k = c.chunk(j);
        uint32_t s = 0, word = 0;
        if (k < n) {
            const Entry e(in_loc[k]);
            if (e.sound(in_bytes)) s = e.stored;
            word = e.word;
        }
        sizes[j] = s;
        uint64_t idx;
        if (s == 0) mine |= kUnsound;
        else if (!d.index(k, idx)) mine |= kOutside;
        else if (d.values && !d.keeps_length(idx, word)) mine |= kLength;
    }
    if (mine) atomicOr(flags, mine);
}

__device__ __forceinline__ uint32_t import_verdict(uint32_t flags, uint64_t used, uint64_t total, uint64_t store_bytes)
{
    if (flags & kUnsound) return 3u;
    if (used > store_bytes || total > store_bytes - used) return 1u;
    return flags & kOutside ? 2u : flags & kLength ? 4u : 0u;
}

// a wavefront per position: the chunk's stored bytes to store + *d_used + off[j], then its directory entry
__global__ void __launch_bounds__(64)
import_copy_kernel(const uint8_t *__restrict__ in, const uint4 *__restrict__ in_loc, Selection c, Directory d,
                   const unsigned long long *__restrict__ off, const uint32_t *__restrict__ flags, uint8_t *__restrict__ store, uint64_t store_bytes,
                   const uint64_t *__restrict__ d_used)
{
    const uint64_t n = c.nchunks(), npos = c.npos(), used = *d_used;
    if (import_verdict(*flags, used, off[npos], store_bytes)) return;
    for (uint64_t j = blockIdx.x; j < npos; j += gridDim.x) {
        const uint64_t k = c.chunk(j);
        uint64_t idx;
        if (k >= n || !d.index(k, idx)) continue; // (no flag: every position has a sound chunk and a directory entry)
        const Entry e(in_loc[k]);
        const uint64_t to = used + off[j];
        lz::copy_g2g(store + to, in + e.pos, e.stored, threadIdx.x);
        if (threadIdx.x == 0) d.entries[idx] = e.at(to);
    }
}

// one thread, behind the copy: the cursor and the result
__global__ void __launch_bounds__(64)
import_finish_kernel(Selection c, const unsigned long long *__restrict__ off, const uint32_t *__restrict__ flags, uint64_t store_bytes,
                     uint64_t *__restrict__ d_used, uint64_t *__restrict__ result)
{
    if (threadIdx.x != 0) return;
    const uint64_t used = *d_used, total = off[c.npos()];
    const uint32_t verdict = import_verdict(*flags, used, total, store_bytes);
    result[0] = verdict;
    result[1] = total;
    if (verdict == 0) *d_used = used + total;
}

// ---- translate ---------------------------------------------------------------------------------------------------------------
// out[j] = to[k] where from[k] == ref[j], else CW_DEDUPE_MISS and counted (out may be ref: a lane reads its position before it writes it)
__global__ void __launch_bounds__(kThreads)
translate_refs_kernel(const uint64_t *ref, const uint64_t *__restrict__ d_count, uint64_t max_count, const uint64_t *__restrict__ from,
                      const uint64_t *__restrict__ to, const uint64_t *__restrict__ d_npairs, uint64_t max_pairs, uint64_t *out,
                      unsigned long long *__restrict__ n_missing)
{
    __shared__ uint32_t wsum[kThreads / 64];
    const uint64_t n = umin64(*d_count, max_count), np = umin64(*d_npairs, max_pairs), threads = (uint64_t)gridDim.x * kThreads;
    uint32_t missing = 0; // (a thread sees at most max_count / threads + 1 < 2^32 positions)
    for (uint64_t j = (uint64_t)blockIdx.x * kThreads + threadIdx.x; j < n; j += threads) {
        const uint64_t r = ref[j];
        uint64_t lo = 0, hi = np; // the first pair with from >= r
        while (lo < hi) {
            const uint64_t mid = lo + (hi - lo) / 2;
            if (from[mid] < r) lo = mid + 1;
            else hi = mid;
        }
        const bool hit = lo < np && from[lo] == r;
        out[j] = hit ? to[lo] : UINT64_MAX;
        missing += !hit;
    }
    const uint32_t all = group_sum(missing, wsum);
    if (threadIdx.x == 0 && all) __hip_atomic_fetch_add(n_missing, (unsigned long long)all, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// per stream: the flag word at [0], the scan's offsets (u64, max_count + 1) from byte 64, the sizes (u32) behind them
StreamScratch<DeviceBuf> replicate_spaces;

} // namespace

hipError_t store_export_launch(const uint8_t *store, size_t store_bytes, const void *dir, uint64_t dir_base, size_t dir_entries,
                               const uint64_t *values, const uint64_t *d_count, size_t max_count, uint8_t *out, size_t out_bytes, void *out_loc,
                               uint64_t *result, hipStream_t stream)
{
    auto &w = replicate_spaces.at(stream);
    LaunchLock sequence(w.launch); // flags, sizes and offsets are shared by the launches below
    ScanScratch s;
    hipError_t e = scan_scratch(w, max_count, stream, s);
    if (e != hipSuccess) return e;
    uint32_t *flags = s.head_as<uint32_t>();
    const uint4 *entries = static_cast<const uint4 *>(dir);
    if (max_count)
        hipLaunchKernelGGL(export_sizes_kernel, dim3(lane_grid(max_count)), dim3(kThreads), 0, stream, entries, dir_base, (uint64_t)dir_entries,
                           (uint64_t)store_bytes, values, d_count, (uint64_t)max_count, s.sizes, flags);
    // off[k] = sum of sizes[0..k) for k <= n (max_count == 0: off[0] = 0)
    if ((e = chunk_pack_launch(0, nullptr, nullptr, nullptr, d_count, max_count, s.sizes, nullptr, s.off, stream)) != hipSuccess) return e;
    const unsigned long long *o = s.offsets();
    if (max_count)
        hipLaunchKernelGGL(export_copy_kernel, dim3(wave_grid(max_count)), dim3(64), 0, stream, store, entries, dir_base, (uint64_t)dir_entries, values,
                           d_count, (uint64_t)max_count, o, flags, out, (uint64_t)out_bytes, static_cast<uint4 *>(out_loc));
    hipLaunchKernelGGL(export_finish_kernel, dim3(1), dim3(64), 0, stream, d_count, (uint64_t)max_count, o, flags, (uint64_t)out_bytes, result);
    return hipGetLastError();
}

namespace {
// values == NULL: the import (chunk k carries base + k); else the replace (position k carries values[k], no selection)
hipError_t import_launch(const uint8_t *in, size_t in_bytes, const void *in_loc, const uint64_t *d_count, size_t max_count, const uint32_t *sel,
                         const uint64_t *d_nsel, uint64_t base, const uint64_t *values, uint8_t *store, size_t store_bytes, uint64_t *d_used, void *dir,
                         uint64_t dir_base, size_t dir_entries, uint64_t *result, hipStream_t stream)
{
    auto &w = replicate_spaces.at(stream);
    LaunchLock sequence(w.launch); // flags, sizes and offsets are shared by the launches below
    ScanScratch s;
    hipError_t e = scan_scratch(w, max_count, stream, s);
    if (e != hipSuccess) return e;
    uint32_t *flags = s.head_as<uint32_t>();
    const uint4 *locs = static_cast<const uint4 *>(in_loc);
    const Selection c{d_count, sel, d_nsel, (uint64_t)max_count};
    const Directory d{static_cast<uint4 *>(dir), base, dir_base, (uint64_t)dir_entries, values};
    if (max_count)
        hipLaunchKernelGGL(import_sizes_kernel, dim3(lane_grid(max_count)), dim3(kThreads), 0, stream, locs, (uint64_t)in_bytes, c, d, s.sizes, flags);
    if ((e = chunk_pack_launch(0, nullptr, nullptr, nullptr, sel ? d_nsel : d_count, max_count, s.sizes, nullptr, s.off, stream)) != hipSuccess) return e;
    const unsigned long long *o = s.offsets();
    if (max_count)
        hipLaunchKernelGGL(import_copy_kernel, dim3(wave_grid(max_count)), dim3(64), 0, stream, in, locs, c, d, o, flags, store, (uint64_t)store_bytes,
                           d_used);
    hipLaunchKernelGGL(import_finish_kernel, dim3(1), dim3(64), 0, stream, c, o, flags, (uint64_t)store_bytes, d_used, result);
    return hipGetLastError();
}
} // namespace

hipError_t store_import_launch(const uint8_t *in, size_t in_bytes, const void *in_loc, const uint64_t *d_count, size_t max_count,
                               const uint32_t *sel, const uint64_t *d_nsel, uint64_t base, uint8_t *store, size_t store_bytes, uint64_t *d_used,
                               void *dir, uint64_t dir_base, size_t dir_entries, uint64_t *result, hipStream_t stream)
{
    return import_launch(in, in_bytes, in_loc, d_count, max_count, sel, d_nsel, base, nullptr, store, store_bytes, d_used, dir, dir_base, dir_entries,
                         result, stream);
}

hipError_t store_replace_launch(const uint8_t *in, size_t in_bytes, const void *in_loc, const uint64_t *values, const uint64_t *d_count,
                                size_t max_count, uint8_t *store, size_t store_bytes, uint64_t *d_used, void *dir, uint64_t dir_base,
                                size_t dir_entries, uint64_t *result, hipStream_t stream)
{
    return import_launch(in, in_bytes, in_loc, d_count, max_count, nullptr, nullptr, 0, values, store, store_bytes, d_used, dir, dir_base, dir_entries,
                         result, stream);
}

hipError_t translate_refs_launch(const uint64_t *ref, const uint64_t *d_count, size_t max_count, const uint64_t *from, const uint64_t *to,
                                 const uint64_t *d_npairs, size_t max_pairs, uint64_t *out, uint64_t *n_missing, hipStream_t stream)
{
    if (max_count == 0) return hipSuccess;
    hipLaunchKernelGGL(translate_refs_kernel, dim3(lane_grid(max_count)), dim3(kThreads), 0, stream, ref, d_count, (uint64_t)max_count, from, to, d_npairs,
                       (uint64_t)max_pairs, out, reinterpret_cast<unsigned long long *>(n_missing));
    return hipGetLastError();
}

} // namespace cw
