// chunk_codec_kernels.hip -- LZ4 / LZF over content-defined chunks: every chunk has its own length,
// 1 .. 65536 bytes, given by an offset list on the device (cw_dev_cdc's), optionally a selection of it (cw_dev_dedupe's list
// of new chunks).  The fixed-size parsers are all tied to one block size per launch; what carries over is the lane-per-block
// form (lz4_lanes_kernel, lzf_lanes_kernel: DESIGN.md 4.3): a LANE owns a chunk and runs the serial parser as it stands, its
// hash table in global memory, bound by the random lines the memory system retires once the chip holds tens of thousands of
// chains -- which chunking supplies (4 GiB at the 8 KiB defaults are 459 k chunks).  The parsers' and the decoders' loops are the
// fixed-size kernels' own (lane_codec.h); here the length, the limits derived from it, the source and the slot are lane values,
// and:
//   * the table is not zeroed per chunk (32 KiB / 256 KiB against ~9 KiB of input): entries carry an epoch, an entry of another
//     epoch reads as the zeroed table would, and the lane's epoch outlives the launch in a word per lane;
//   * chunks are taken longest first from a counting sort of the positions (lengths span 32x: the lanes of a wavefront then
//     finish together), through one work counter;
//   * compressed chunk i goes to the slot cw_chunk_slot_offset(alg, offsets[i], i), known before the parse.
// The decoder is decompress_lanes_kernel's with per-lane extents.  Out-of-contract chunks (empty, longer than 65536, decreasing,
// past the source) get size 0 and are never loaded or stored.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cw_device.h"
#include "lane_codec.h"
#include "stream_scratch.h"

namespace cw {

namespace {

using namespace lane;

constexpr uint32_t kMaxChunk = kMaxChunkBytes;
constexpr uint32_t kLz4Slots = 1u << 13, kLzfSlots = 1u << 16; // u32 entries: 32 KiB / 256 KiB per lane

// (the positions of a call and the chunk behind each: ChunkList, cw_device.h)

// ---- order: positions by length, longest first (counting sort over 64-byte classes; out-of-contract chunks last) -----------
constexpr unsigned kBuckets = 1025, kSortThreads = 256, kSortPer = 8, kSortTile = kSortThreads * kSortPer;

__device__ __forceinline__ uint32_t order_bucket(uint32_t len) { return 1024u - ((len + 63u) >> 6); }

// A workgroup counts its tile in LDS and adds only the classes it met to the global histogram: one global atomic per
// (workgroup, class) instead of one per chunk.
__global__ void __launch_bounds__(kSortThreads)
chunk_order_hist_kernel(ChunkList c, uint32_t *__restrict__ hist)
{
    __shared__ uint32_t h[kBuckets];
    const uint64_t npos = c.npos(), count = c.nchunks(), base = (uint64_t)blockIdx.x * kSortTile;
    if (base >= npos) return;
    for (unsigned b = threadIdx.x; b < kBuckets; b += kSortThreads) h[b] = 0;
    __syncthreads();
#pragma unroll
    for (unsigned k = 0; k < kSortPer; k++) {
        const uint64_t j = base + k * kSortThreads + threadIdx.x;
        if (j < npos) {
            uint64_t i, s;
            atomicAdd(&h[order_bucket(c.chunk(j, count, i, s))], 1u);
        }
    }
    __syncthreads();
    for (unsigned b = threadIdx.x; b < kBuckets; b += kSortThreads)
        if (h[b]) atomicAdd(&hist[b], h[b]);
}

// one workgroup: exclusive scan of the class counts in place
__global__ void __launch_bounds__(1024)
chunk_order_scan_kernel(uint32_t *__restrict__ hist)
{
    __shared__ uint32_t part[1024];
    const uint32_t v = hist[threadIdx.x];
    part[threadIdx.x] = v;
    __syncthreads();
    for (unsigned d = 1; d < 1024; d <<= 1) {
        const uint32_t add = threadIdx.x >= d ? part[threadIdx.x - d] : 0;
        __syncthreads();
        part[threadIdx.x] += add;
        __syncthreads();
    }
    hist[threadIdx.x] = part[threadIdx.x] - v;
    if (threadIdx.x == 1023) hist[1024] = part[1023]; // the out-of-contract class comes last
}

// The same tiles: a position's rank within its class and workgroup comes from the LDS count, the workgroup reserves its share
// of every class it met with one global atomic, and the positions go to their places.  (Within a class the order depends on
// which workgroup reserves first: any order of equal classes serves.)
__global__ void __launch_bounds__(kSortThreads)
chunk_order_scatter_kernel(ChunkList c, uint32_t *__restrict__ cursor, uint32_t *__restrict__ order)
{
    __shared__ uint32_t h[kBuckets];
    const uint64_t npos = c.npos(), count = c.nchunks(), base = (uint64_t)blockIdx.x * kSortTile;
    if (base >= npos) return;
    for (unsigned b = threadIdx.x; b < kBuckets; b += kSortThreads) h[b] = 0;
    __syncthreads();
    uint32_t bucket[kSortPer], rank[kSortPer];
#pragma unroll
    for (unsigned k = 0; k < kSortPer; k++) {
        const uint64_t j = base + k * kSortThreads + threadIdx.x;
        bucket[k] = 0; rank[k] = 0;
        if (j < npos) {
            uint64_t i, s;
            bucket[k] = order_bucket(c.chunk(j, count, i, s));
            rank[k] = atomicAdd(&h[bucket[k]], 1u);
        }
    }
    __syncthreads();
    for (unsigned b = threadIdx.x; b < kBuckets; b += kSortThreads)
        if (h[b]) h[b] = atomicAdd(&cursor[b], h[b]);
    __syncthreads();
#pragma unroll
    for (unsigned k = 0; k < kSortPer; k++) {
        const uint64_t j = base + k * kSortThreads + threadIdx.x;
        if (j < npos) order[h[bucket[k]] + rank[k]] = (uint32_t)j;
    }
}

// ---- the parsers -----------------------------------------------------------------------------------------------------------
// up to 4 bytes at ip, none from behind the chunk (n can be 3: no dword read one position early, as lzf_rd does)
__device__ __forceinline__ uint32_t chunk_rd(const uint8_t *g, uint32_t ip, uint32_t n)
{
    if (ip + 4 <= n) return rd32(g, ip);
    uint32_t v = 0;
    for (uint32_t k = 0; k < 4; k++) if (ip + k < n) v |= (uint32_t)g[ip + k] << (8 * k);
    return v;
}

// The positions of a call as a source of the lane parsers (lane_codec.h): taken in `order` through one work counter; the chunk's
// length and everything derived from it are lane values.  An out-of-contract chunk gets size 0, nothing of it is loaded or
// stored, and the lane asks again.  No bail-out for chunks that do not compress (out of scope: DESIGN.md 12).
template <bool LZ4>
struct ChunkWork {
    static constexpr bool kShort = true; // LZ4: n < 13 is last literals only; LZF: n < 3 has no position to hash
    const uint8_t *const src; const ChunkList &c; const uint64_t npos, count;
    const uint32_t *const order; uint8_t *const dst; uint32_t *const sizes; unsigned long long *const work;
    const uint8_t *g; uint8_t *out;
    uint32_t blk, n, mflimit, matchlimit; // (mflimit, matchlimit: LZ4, read only where n >= 13)
    __device__ __forceinline__ Take take()
    {
        const unsigned long long qi = atomicAdd(work, 1ull);
        if (qi >= npos) return Take::kDone;
        blk = order[qi];
        uint64_t i, start;
        n = c.chunk(blk, count, i, start);
        if (n == 0) { sizes[blk] = 0; return Take::kAgain; }
        g = src + start;
        out = dst + chunk_slot_offset(LZ4, start, i);
        mflimit = n - kMFLimit; matchlimit = n - kLastLiterals;
        return Take::kTaken;
    }
    __device__ __forceinline__ uint32_t rd(uint32_t ip) const { return chunk_rd(g, ip, n); }
    __device__ __forceinline__ bool keep(uint32_t, uint32_t) const { return true; }
};

// The tables are not zeroed per chunk: an entry carries the epoch of the parse that wrote it, an entry of another epoch reads as
// the zeroed table would, and the table is zeroed when the epoch wraps.  epoch = 0 on a fresh (zeroed) table.
template <uint32_t SLOTS, uint32_t EPOCHS>
__device__ __forceinline__ void chunk_tab_begin(uint32_t *tab, uint32_t &epoch)
{
    if (++epoch == EPOCHS) {
        uint4 *t4 = reinterpret_cast<uint4 *>(tab);
#pragma unroll 4 // (once per EPOCHS parses: unrolled further, its store addresses were the kernels' peak register demand)
        for (uint32_t k = 0; k < SLOTS * 4 / 16; k++) t4[k] = make_uint4(0, 0, 0, 0);
        epoch = 1;
    }
}
// 8 further bits of the hash product (lz4_lanes_kernel's fingerprint, shortened to make room for the epoch)
__device__ __forceinline__ uint32_t fp8(uint32_t v) { return ((v * 2654435761u) >> 11) & 0xFFu; }
// LZ4: epoch:8 | fingerprint:8 | position:16.  An entry whose upper half is not (epoch, fingerprint of the 4 bytes looked up) is
// not a candidate: either it is of another chunk or it holds other bytes.
struct Lz4ChunkTab {
    static constexpr bool kNameFirst = true;
    uint32_t *tab, epoch;
    __device__ __forceinline__ uint32_t get(uint32_t h, uint32_t v, bool &maybe) const
    {
        const uint32_t e = tab[h];
        maybe = (e >> 16) == ((epoch << 8) | fp8(v));
        return e & 0xFFFFu;
    }
    __device__ __forceinline__ void put(uint32_t h, uint32_t v, uint32_t pos) const { tab[h] = (epoch << 24) | (fp8(v) << 16) | pos; }
    __device__ __forceinline__ void begin() { chunk_tab_begin<kLz4Slots, 256>(tab, epoch); }
};
// LZF: epoch:16 | position:16
struct LzfChunkTab {
    uint32_t *tab, epoch;
    __device__ __forceinline__ uint32_t get(uint32_t slot) const
    {
        const uint32_t e = tab[slot];
        return (e >> 16) == epoch ? e & 0xFFFFu : 0u;
    }
    __device__ __forceinline__ void put(uint32_t slot, uint32_t pos) const { tab[slot] = (epoch << 16) | pos; }
    __device__ __forceinline__ void begin() { chunk_tab_begin<kLzfSlots, 65536>(tab, epoch); }
};

__global__ void __launch_bounds__(64)
lz4_chunks_kernel(const uint8_t *__restrict__ src, ChunkList c, const uint32_t *__restrict__ order, uint8_t *__restrict__ dst,
                  uint32_t *__restrict__ sizes, uint32_t *__restrict__ tables, uint32_t *__restrict__ epochs, unsigned long long *__restrict__ work)
{
    const uint64_t npos = c.npos();
    if ((uint64_t)blockIdx.x * 64 >= npos) return; // fewer positions than lanes: the first workgroups take them with every lane busy
    const size_t lane_id = (size_t)blockIdx.x * 64 + threadIdx.x;
    ChunkWork<true> s{src, c, npos, c.nchunks(), order, dst, sizes, work, src, dst};
    Lz4ChunkTab t{tables + lane_id * kLz4Slots, epochs[lane_id]};
    lz4_lane_run(s, t);
    epochs[lane_id] = t.epoch; // the lane's epoch outlives the launch
}

__global__ void __launch_bounds__(64)
lzf_chunks_kernel(const uint8_t *__restrict__ src, ChunkList c, const uint32_t *__restrict__ order, uint8_t *__restrict__ dst,
                  uint32_t *__restrict__ sizes, uint32_t *__restrict__ tables, uint32_t *__restrict__ epochs, unsigned long long *__restrict__ work)
{
    const uint64_t npos = c.npos();
    if ((uint64_t)blockIdx.x * 64 >= npos) return;
    const size_t lane_id = (size_t)blockIdx.x * 64 + threadIdx.x;
    ChunkWork<false> s{src, c, npos, c.nchunks(), order, dst, sizes, work, src, dst};
    LzfChunkTab t{tables + lane_id * kLzfSlots, epochs[lane_id]};
    lzf_lane_run(s, t);
    epochs[lane_id] = t.epoch;
}

// ---- decoder -----------------------------------------------------------------------------------------------------------------
// decompress_lanes_kernel's decoder (lane_decode) with the compressed extent [comp_off[j], comp_off[j+1]) and the raw extent
// [raw_off[j], raw_off[j+1]) as lane values.  status: 0 = well formed and exactly the raw extent produced; 1 otherwise, including
// an empty compressed extent and a raw extent that is decreasing, longer than 65536 or past dst_bytes (then nothing is loaded or
// stored).
template <int ALG>
__global__ void __launch_bounds__(64)
decompress_chunks_kernel(const uint8_t *__restrict__ comp, const uint64_t *__restrict__ comp_off, const uint64_t *__restrict__ raw_off,
                         const uint64_t *__restrict__ d_count, uint64_t max_count, uint8_t *__restrict__ dst, uint64_t dst_bytes,
                         uint32_t *__restrict__ status)
{
    const uint64_t total = umin64(*d_count, max_count), lanes = (uint64_t)gridDim.x * 64;
    for (uint64_t j = (uint64_t)blockIdx.x * 64 + threadIdx.x; j < total; j += lanes) {
        const uint64_t cs = comp_off[j], ce = comp_off[j + 1], rs = raw_off[j], re = raw_off[j + 1];
        const bool skip = ce <= cs || ce - cs > (1u << 24) || re < rs || re - rs > kMaxChunk || re > dst_bytes;
        const uint8_t *in = comp + (skip ? 0 : cs);
        uint8_t *d = dst + (skip ? 0 : rs);
        const uint32_t n = skip ? 0u : (uint32_t)(ce - cs), raw_bytes = skip ? 0u : (uint32_t)(re - rs);
        status[j] = lane_decode<ALG>(in, n, d, raw_bytes, skip) ? 1u : 0u;
    }
}

// ---- per-stream scratch ----------------------------------------------------------------------------------------------------
struct ChunkSpace {
    DeviceBuf sort;                 // class counts, the work counter, the order
    DeviceBuf tabs[2], epochs[2];   // lane tables and the lanes' epochs, LZ4 / LZF
    size_t grid_limit[2] = {0, 0};  // workgroups of lanes an allocation that failed left this stream with (0: no limit met)
    void release()
    {
        grid_limit[0] = grid_limit[1] = 0;
        (void)sort.release();
        for (int a = 0; a < 2; a++) { (void)tabs[a].release(); (void)epochs[a].release(); }
    }
};
StreamScratch<ChunkSpace> chunk_spaces;
constexpr size_t kSortHead = 2048; // u32 words in front of the order: kBuckets counts, then the work counter at [kWorkWord]
constexpr size_t kWorkWord = 1032;  // (8-byte aligned: a 64-bit counter, which npos + one draw per lane cannot wrap)

} // namespace

size_t chunk_lane_table_bytes(int lzf) { return (size_t)(lzf ? kLzfSlots : kLz4Slots) * 4; }

hipError_t chunk_compress_launch(int lzf, const uint8_t *src, size_t src_bytes, const uint64_t *offsets, const uint64_t *d_nchunks,
                                 size_t max_chunks, const uint32_t *sel, const uint64_t *d_nsel, uint8_t *dst, uint32_t *sizes,
                                 hipStream_t stream)
{
    if (max_chunks == 0) return hipSuccess;
    auto &w = chunk_spaces.at(stream);
    // sort, work counter, tables and epochs are shared by the launches below: another thread's call on the same stream queues
    // its sequence before or after this one, never in between
    LaunchLock sequence(w.launch);
    hipError_t e = w.sort.reserve((kSortHead + max_chunks) * 4, (size_t)1 << 20);
    if (e != hipSuccess) return e;
    // lanes: a wavefront of 64 per workgroup, 8 (LZ4) / 4 (LZF: 256 KiB of table per lane) wavefronts per CU at most; no more than
    // max_chunks, and no more than one per 4 KiB of source (at the 8 KiB defaults every chunk still gets a lane; with smaller chunks
    // a lane takes several), so that the tables are in proportion to the input and not to the caller's bound on the chunk count.
    // A table allocation that fails is retried with half the lanes, and the stream keeps to what it got.
    size_t grid = (max_chunks + 63) / 64;
    const size_t cap = 256 * (size_t)(lzf ? 4 : 8), tab_bytes = chunk_lane_table_bytes(lzf), by_bytes = src_bytes / (4096 * 64) + 1;
    if (grid > by_bytes) grid = by_bytes;
    if (grid > cap) grid = cap;
    if (w.grid_limit[lzf] && grid > w.grid_limit[lzf]) grid = w.grid_limit[lzf];
    DeviceBuf &tabs = w.tabs[lzf], &epochs = w.epochs[lzf];
    if (tabs.bytes() < grid * 64 * tab_bytes) {
        // (a table is only replaced by a larger one: the queued launches of this stream that use the old one have to finish first)
        if (tabs.bytes() && (e = hipStreamSynchronize(stream)) != hipSuccess) return e;
        for (;;) {
            e = tabs.reserve(grid * 64 * tab_bytes);
            if (e == hipSuccess) e = epochs.reserve(cap * 64 * 4);
            if (e == hipSuccess) break;
            (void)hipGetLastError();
            (void)tabs.release();
            if (grid == 1) return hipErrorOutOfMemory;
            grid = (grid + 1) / 2;
            w.grid_limit[lzf] = grid;
        }
        // fresh tables: all entries and all epochs 0, so that no entry is of a lane's first epoch (1)
        if ((e = hipMemsetAsync(tabs.as<void>(), 0, tabs.bytes(), stream)) != hipSuccess) return e;
        if ((e = hipMemsetAsync(epochs.as<void>(), 0, epochs.bytes(), stream)) != hipSuccess) return e;
    }
    uint32_t *head = w.sort.as<uint32_t>(), *order = head + kSortHead;
    if ((e = hipMemsetAsync(head, 0, kSortHead * 4, stream)) != hipSuccess) return e;
    const ChunkList c{offsets, d_nchunks, sel, d_nsel, (uint64_t)max_chunks, (uint64_t)src_bytes};
    const unsigned sgrid = (unsigned)((max_chunks + kSortTile - 1) / kSortTile);
    hipLaunchKernelGGL(chunk_order_hist_kernel, dim3(sgrid), dim3(kSortThreads), 0, stream, c, head);
    hipLaunchKernelGGL(chunk_order_scan_kernel, dim3(1), dim3(1024), 0, stream, head);
    hipLaunchKernelGGL(chunk_order_scatter_kernel, dim3(sgrid), dim3(kSortThreads), 0, stream, c, head, order);
    if (lzf) {
        hipLaunchKernelGGL(lzf_chunks_kernel, dim3((unsigned)grid), dim3(64), 0, stream, src, c, order, dst, sizes, tabs.as<uint32_t>(),
                           epochs.as<uint32_t>(), reinterpret_cast<unsigned long long *>(head + kWorkWord));
        note_kernels(0, "cw::lzf_chunks_kernel");
    } else {
        hipLaunchKernelGGL(lz4_chunks_kernel, dim3((unsigned)grid), dim3(64), 0, stream, src, c, order, dst, sizes, tabs.as<uint32_t>(),
                           epochs.as<uint32_t>(), reinterpret_cast<unsigned long long *>(head + kWorkWord));
        note_kernels(0, "cw::lz4_chunks_kernel");
    }
    return hipGetLastError();
}

hipError_t chunk_decompress_launch(int lzf, const uint8_t *comp, const uint64_t *comp_offsets, const uint64_t *raw_offsets,
                                   const uint64_t *d_count, size_t max_count, uint8_t *dst, size_t dst_bytes, uint32_t *status,
                                   hipStream_t stream)
{
    if (max_count == 0) return hipSuccess;
    size_t grid = (max_count + 63) / 64;
    if (grid > 256 * 8) grid = 256 * 8;
    if (lzf)
        hipLaunchKernelGGL(decompress_chunks_kernel<1>, dim3((unsigned)grid), dim3(64), 0, stream, comp, comp_offsets, raw_offsets, d_count,
                           (uint64_t)max_count, dst, (uint64_t)dst_bytes, status);
    else
        hipLaunchKernelGGL(decompress_chunks_kernel<0>, dim3((unsigned)grid), dim3(64), 0, stream, comp, comp_offsets, raw_offsets, d_count,
                           (uint64_t)max_count, dst, (uint64_t)dst_bytes, status);
    return hipGetLastError();
}

} // namespace cw
