// restore_kernels.hip -- the chunk store: cw_dev_store_chunks appends the new chunks of one compressing call
// to a store the caller owns, cw_dev_restore_chunks rebuilds a stream from the values cw_dev_dedupe wrote.  The store is three plain
// device buffers: the bytes, an append cursor, and a directory of 16-byte entries {pos, stored, length | raw flag} indexed by
// value - dir_base.  Nothing here keeps state between calls.
//
// Append: the effective size of every position (the compressed size when 0 < s < l, else the chunk's length: it is then kept raw)
// and the directory-range verdict, an exclusive scan of those sizes (chunk_pack_launch, index only), a wavefront-per-position copy
// from the slot or from the source that also writes the entry, and one thread that moves the cursor and reports.  The copy and the
// cursor are gated on the same test, so a call that does not fit, or that names an entry outside the directory, changes nothing.
//
// Restore: decompress_chunks_kernel's lane-per-position form with the compressed extent taken from the directory entry; entries kept
// raw are copied by the whole wavefront afterwards.  Every field of an entry is checked against the store, the raw extent and the
// destination before anything is loaded or stored through it: a tampered directory gets statuses, never an access out of bounds.

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

// ---- append ------------------------------------------------------------------------------------------------------------------
// eff[j] = bytes position j occupies in the store (0: out of contract); *flags |= 1 if an in-contract chunk has no directory entry
__global__ void __launch_bounds__(kThreads)
store_sizes_kernel(ChunkList c, const uint32_t *__restrict__ sizes, Directory d, uint32_t *__restrict__ eff, uint32_t *__restrict__ flags)
{
    const uint64_t npos = c.npos(), count = c.nchunks(), threads = (uint64_t)gridDim.x * kThreads;
    bool outside = false;
    for (uint64_t j = (uint64_t)blockIdx.x * kThreads + threadIdx.x; j < npos; j += threads) {
        uint64_t i, start, idx;
        const uint32_t l = c.chunk(j, count, i, start);
        uint32_t e = 0;
        if (l) {
            const uint32_t s = sizes[j];
            e = s > 0 && s < l ? s : l;
            outside |= !d.index<false>(i, idx); // (the append has no list of values: chunk i carries base + i)
        }
        eff[j] = e;
    }
    if (outside) atomicOr(flags, 1u);
}

// what the copy and the cursor are gated on: the directory holds every chunk and the total fits behind the cursor
__device__ __forceinline__ uint32_t store_verdict(uint64_t used, uint64_t total, uint64_t store_bytes, uint32_t flags)
{
    if (used > store_bytes || total > store_bytes - used) return 1u;
    return flags ? 2u : 0u;
}

// a wavefront per position: eff[j] bytes from the chunk's slot (compressed: eff < l) or from the source (raw: eff == l) to
// store + *d_used + off[j], then the entry
__global__ void __launch_bounds__(64)
store_copy_kernel(const uint8_t *__restrict__ src, ChunkList c, const uint8_t *__restrict__ slots, bool lz4, const uint32_t *__restrict__ eff,
                  const unsigned long long *__restrict__ off, const uint32_t *__restrict__ flags, Directory d, uint8_t *__restrict__ store,
                  uint64_t store_bytes, const uint64_t *__restrict__ d_used)
{
    const uint64_t npos = c.npos(), count = c.nchunks(), used = *d_used;
    if (store_verdict(used, off[npos], store_bytes, *flags)) return;
    const uint32_t lane = threadIdx.x;
    for (uint64_t j = blockIdx.x; j < npos; j += gridDim.x) {
        const uint32_t e = eff[j];
        if (e == 0) continue;
        uint64_t i, start, idx;
        const uint32_t l = c.chunk(j, count, i, start);
        if (!d.index<false>(i, idx)) continue; // (no flag: every in-contract chunk has an entry)
        const bool raw = e == l;
        const uint64_t pos = used + off[j];
        lz::copy_g2g(store + pos, raw ? src + start : slots + chunk_slot_offset(lz4, start, i), e, lane);
        if (lane == 0) d.entries[idx] = make_uint4((uint32_t)pos, (uint32_t)(pos >> 32), e, l | (raw ? kRawFlag : 0u));
    }
}

// one thread, behind the copy: the cursor and the result
__global__ void __launch_bounds__(64)
store_finish_kernel(ChunkList c, const unsigned long long *__restrict__ off, const uint32_t *__restrict__ flags, uint64_t store_bytes,
                    uint64_t *__restrict__ d_used, uint64_t *__restrict__ result)
{
    if (threadIdx.x != 0) return;
    const uint64_t used = *d_used, total = off[c.npos()];
    const uint32_t verdict = store_verdict(used, total, store_bytes, *flags);
    result[0] = verdict;
    result[1] = total;
    if (verdict == 0) *d_used = used + total;
}

// ---- restore -----------------------------------------------------------------------------------------------------------------
// A wavefront takes 64 positions at a time: every lane checks its position's recipe and entry, the lanes with a compressed entry
// decode it (lane_decode), then the wavefront copies the raw entries of those 64 positions one after the other.  status: 0 = the
// extent holds the chunk; 1 = malformed stored bytes; 2 = refused, nothing loaded from the store and nothing stored.
template <int ALG>
__global__ void __launch_bounds__(64)
restore_chunks_kernel(const uint8_t *__restrict__ store, uint64_t store_bytes, const uint4 *__restrict__ dir, uint64_t dir_base, uint64_t dir_entries,
                      const uint64_t *__restrict__ ref, const uint64_t *__restrict__ raw_off, const uint64_t *__restrict__ d_count,
                      uint64_t max_count, uint8_t *__restrict__ dst, uint64_t dst_bytes, uint32_t *__restrict__ status)
{
    const uint64_t total = umin64(*d_count, max_count), lanes = (uint64_t)gridDim.x * 64;
    for (uint64_t first = (uint64_t)blockIdx.x * 64; first < total; first += lanes) { // (wave-uniform: the copies below need every lane)
        const uint64_t j = first + threadIdx.x;
        bool refuse = true, raw = false;
        uint64_t pos = 0, rs = 0;
        uint32_t stored = 0, len = 0;
        if (j < total) {
            const uint64_t r = ref[j], re = raw_off[j + 1];
            uint64_t idx;
            const bool named = names_entry(r, dir_base, dir_entries, idx); // (in front of the condition: no branch of its own)
            rs = raw_off[j];
            // (r >= dir_base: a directory whose values wrap has no entry for a value below its base)
            if (r >= dir_base && named && rs <= re && re - rs <= kMaxChunkBytes && re <= dst_bytes) {
                const Entry e(dir[idx]);
                pos = e.pos;
                stored = e.stored;
                len = e.len();
                raw = e.raw();
                refuse = !e.sound(store_bytes) || len != re - rs;
            }
        }
        // (cw_dev_decompress_chunks skips a compressed extent above 2^24 bytes with status 1: the same verdict here)
        const bool skip = refuse || raw || stored > (1u << 24);
        const bool bad = lane_decode<ALG>(store + (skip ? 0 : pos), skip ? 0u : stored, dst + (skip ? 0 : rs), skip ? 0u : len, skip);
        if (j < total) status[j] = refuse ? 2u : raw ? 0u : bad ? 1u : 0u;
        wave_copy(!refuse && raw, store, pos, dst, rs, len);
    }
}

// per stream: the flags word at [0], the scan's offsets (u64, max_chunks + 1) from byte 64, the effective sizes (u32) behind them
StreamScratch<DeviceBuf> store_spaces;

} // namespace

hipError_t chunk_store_launch(int lzf, const uint8_t *src, size_t src_bytes, const uint64_t *offsets, const uint64_t *d_nchunks, size_t max_chunks,
                              const uint32_t *sel, const uint64_t *d_nsel, const uint8_t *slots, const uint32_t *sizes, uint64_t base,
                              uint8_t *store, size_t store_bytes, uint64_t *d_used, void *dir, uint64_t dir_base, size_t dir_entries,
                              uint64_t *result, hipStream_t stream)
{
    auto &w = store_spaces.at(stream);
    LaunchLock sequence(w.launch); // flags, sizes and offsets are shared by the launches below
    ScanScratch s;
    hipError_t e = scan_scratch(w, max_chunks, stream, s);
    if (e != hipSuccess) return e;
    uint32_t *flags = s.head_as<uint32_t>(), *eff = s.sizes;
    const ChunkList c{offsets, d_nchunks, sel, d_nsel, (uint64_t)max_chunks, (uint64_t)src_bytes};
    const Directory d{static_cast<uint4 *>(dir), base, dir_base, (uint64_t)dir_entries, nullptr};
    if (max_chunks)
        hipLaunchKernelGGL(store_sizes_kernel, dim3(lane_grid(max_chunks)), dim3(kThreads), 0, stream, c, sizes, d, eff, flags);
    // off[j] = sum of eff[0..j) for j <= n, n = the number of positions (max_chunks == 0: off[0] = 0)
    if ((e = chunk_pack_launch(lzf, nullptr, nullptr, nullptr, sel ? d_nsel : d_nchunks, max_chunks, eff, nullptr, s.off, stream)) != hipSuccess)
        return e;
    const unsigned long long *o = s.offsets();
    if (max_chunks)
        hipLaunchKernelGGL(store_copy_kernel, dim3(wave_grid(max_chunks)), dim3(64), 0, stream, src, c, slots, lzf == 0, eff, o, flags, d, store,
                           (uint64_t)store_bytes, d_used);
    hipLaunchKernelGGL(store_finish_kernel, dim3(1), dim3(64), 0, stream, c, o, flags, (uint64_t)store_bytes, d_used, result);
    return hipGetLastError();
}

hipError_t chunk_restore_launch(int lzf, const uint8_t *store, size_t store_bytes, const void *dir, uint64_t dir_base, size_t dir_entries,
                                const uint64_t *ref, const uint64_t *raw_offsets, const uint64_t *d_count, size_t max_count, uint8_t *dst,
                                size_t dst_bytes, uint32_t *status, hipStream_t stream)
{
    if (max_count == 0) return hipSuccess;
    const unsigned grid = decode_grid(max_count);
    const uint4 *entries = static_cast<const uint4 *>(dir);
    if (lzf)
        hipLaunchKernelGGL(restore_chunks_kernel<1>, dim3(grid), dim3(64), 0, stream, store, (uint64_t)store_bytes, entries, dir_base,
                           (uint64_t)dir_entries, ref, raw_offsets, d_count, (uint64_t)max_count, dst, (uint64_t)dst_bytes, status);
    else
        hipLaunchKernelGGL(restore_chunks_kernel<0>, dim3(grid), dim3(64), 0, stream, store, (uint64_t)store_bytes, entries, dir_base,
                           (uint64_t)dir_entries, ref, raw_offsets, d_count, (uint64_t)max_count, dst, (uint64_t)dst_bytes, status);
    return hipGetLastError();
}

} // namespace cw
