// cw_device.h -- internal declarations shared by the HIP translation units of libcwhc.so.
// Not part of the public boundary (that is include/cw_hashcompress.h).
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "knobs.h"

#ifndef CW_SKEIN_THREADS
#define CW_SKEIN_THREADS 64 // one wavefront per workgroup: lanes never communicate, small groups spread evenly
#endif

namespace cw {

// Diagnostic build only (-DCW_CLOCK_STAMP, tools/clock_probe.py): the clock a kernel actually runs at.  Lane 0 of a workgroup
// reads s_memtime (shader cycles) and s_memrealtime (a constant 100 MHz counter) when the workgroup starts and when it ends;
// the four values go to a buffer nothing else reads, and the host takes, per workgroup, d(memtime) / d(memrealtime) x 100 MHz
// (MI355X_MICROARCH.md, "DVFS give-back" item 6).  In the product build no stamp executes.
#ifdef CW_CLOCK_STAMP
constexpr unsigned kClockSlots = 1024;
struct ClockScope {
    unsigned long long m0 = 0, r0 = 0;
    unsigned long long *rec;
    bool on;
    __device__ ClockScope(unsigned long long *buf, unsigned wg) : rec(buf + 4 * (wg % kClockSlots)), on(threadIdx.x == 0)
    {
        if (on) { m0 = __builtin_amdgcn_s_memtime(); r0 = __builtin_amdgcn_s_memrealtime(); }
    }
    __device__ ~ClockScope()
    {
        if (on) {
            const unsigned long long m1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
            rec[0] = m0; rec[1] = r0; rec[2] = m1; rec[3] = r1;
        }
    }
};
#define CW_CLOCK_SCOPE(buf) ClockScope clock_scope_(buf, blockIdx.x)
// keyed: the kClockSlots records are cut into 8 groups of 128, one per `key` (the slice kernel's launch index within a pass), so
// that the launches that overlap the codec and those that run after it are reported apart
#define CW_CLOCK_SCOPE_KEYED(buf, key) ClockScope clock_scope_(buf, ((unsigned)(key) % 8u) * 128u + blockIdx.x % 128u)
// which: 0 = the Skein slice kernel, 1 = the LZ4 span scan; out = kClockSlots x {m0, r0, m1, r1}
hipError_t skein_clock_read(unsigned long long *out);
hipError_t lz4_clock_read(unsigned long long *out);
#else
#define CW_CLOCK_SCOPE(buf) do { } while (0)
#define CW_CLOCK_SCOPE_KEYED(buf, key) do { } while (0)
#endif

struct SkeinIV { uint64_t w[8]; };

// The launch functions note which kernels they used, per calling thread (kind 0 = codec, 1 = hash): cw_profile_kernels
// hands the names to the caller so that a benchmark reports what ran instead of guessing it from its arguments.
void note_kernels(int kind, const char *names);
// host: chaining value after the configuration block (Skein_*_Init)
void skein_compute_iv(int state_words, unsigned hash_bits, SkeinIV *iv, uint64_t tree_info = 0);
// tree hashing of every block (one wavefront per block, lane = leaf/node); digest = hash_bits / 8 bytes per block
hipError_t skein_tree_launch(int state_words, const uint8_t *src, size_t block_bytes, size_t src_stride, size_t nblocks,
                             unsigned hash_bits, unsigned leaf, unsigned node, unsigned max_level, uint8_t *digests, hipStream_t stream);

// device launches (async on `stream`) of what the plan says (launch_plan.h: hash_plan); src_stride = distance between consecutive
// blocks in bytes.  skein_launch: one kernel, or the sliced launches of a long message (see skein_kernels.hip)
struct HashPlan;
hipError_t skein_launch(const HashPlan &p, const uint8_t *src, size_t block_bytes, size_t src_stride, size_t nblocks, const SkeinIV &iv,
                        uint8_t *digests, unsigned digest_bytes, hipStream_t stream);
hipError_t sha256_launch(const HashPlan &p, const uint8_t *src, size_t block_bytes, size_t src_stride, size_t nblocks, uint8_t *digests,
                         hipStream_t stream);
// after_scan (optional): called ONCE, right behind the launch of the scan and in front of everything else, if the call gets that far (the caller
// checks): what it enqueues on other streams runs beside the scan; what it makes `stream` wait for, the parsers wait for
struct AfterScan { hipError_t (*fn)(void *ctx); void *ctx; };
hipError_t lz4_launch(const uint8_t *src, size_t block_bytes, size_t src_stride, size_t nblocks, uint8_t *dst,
                      size_t dst_stride, uint32_t *sizes, hipStream_t stream, const AfterScan *after_scan = nullptr);
const uint32_t *lz4_queued_blocks_word(hipStream_t stream);
hipError_t lzf_launch(const uint8_t *src, size_t block_bytes, size_t src_stride, size_t nblocks, uint8_t *dst,
                      size_t dst_stride, uint32_t *sizes, hipStream_t stream);
enum class Lz4Vtab : uint8_t; // (launch_plan.h)
// LZ4 scalar-thread parsers (lz4_vtab_kernel.hip; the plan chooses the member, the grid and the LDS bytes): they parse blocks of the
// scan's queue (counters[0] = head, counters[1] = length) while more than `reserve` are left, if the queue's length lies in
// [min_queued, max_queued)
hipError_t lz4_vtab_launch(Lz4Vtab kernel, uint32_t grid, uint32_t lds, hipStream_t stream, const uint8_t *src, uint32_t n, size_t src_stride, uint8_t *dst,
                           size_t dst_stride, uint32_t *sizes, const uint32_t *queue, uint32_t *counters, uint32_t min_queued, uint32_t max_queued,
                           uint32_t reserve);
hipError_t decompress_launch(int alg, const uint8_t *comp, size_t comp_stride, const uint32_t *sizes, size_t nblocks, uint8_t *dst,
                             size_t block_bytes, uint32_t *status, hipStream_t stream);
// packed stream: offsets[i] = sum sizes[0..i) (nblocks + 1 entries); slot i copied to packed + offsets[i] (packed may be NULL)
hipError_t pack_launch(const uint8_t *slots, size_t slot_stride, const uint32_t *sizes, size_t nblocks, uint8_t *packed,
                       uint64_t *offsets, hipStream_t stream);
// Per-stream scratch of the launch sequences (queues, link arrays, scan partials, side streams: stream_scratch.h), in every
// registry of the library.  For ONE stream of the current device: called by whoever owns the stream before destroying it, so
// that a short-lived calling thread does not leave gigabytes of lane tables behind and a recycled stream handle does not
// inherit a stale entry.  All of it: cw_shutdown.
void release_stream_workspaces(hipStream_t stream);
void release_all_workspaces();
// fingerprint index (dedupe_kernels.hip): words = u64 words per digest (2 / 4 / 8); mask = slots - 1; rec / flags = per-block
// scratch of the call; off = exclusive scan of flags (pack_launch, index only); err |= 1 if a probe reached the bound
hipError_t dedupe_probe_launch(unsigned words, const uint64_t *dig, uint32_t n, uint64_t *state, uint32_t *min_idx, const uint64_t *value,
                               const uint64_t *key, uint64_t mask, uint64_t *rec, uint64_t *ref, unsigned long long *err, hipStream_t s);
// values != NULL: block j carries values[j] instead of base + j (cw_dev_dedupe_insert)
hipError_t dedupe_resolve_launch(unsigned words, const uint64_t *dig, uint32_t n, uint64_t base, const uint64_t *values, const uint32_t *min_idx,
                                 uint64_t *state, uint64_t *value, uint64_t *key, const uint64_t *rec, uint64_t *ref, uint32_t *flags, hipStream_t s);
hipError_t dedupe_scatter_launch(const uint32_t *flags, const uint64_t *off, uint32_t n, const uint64_t *rec, uint32_t *min_idx,
                                 uint32_t *new_idx, uint64_t *n_new, uint64_t *count, hipStream_t s);
// read-only: ref[i] = the stored value or UINT64_MAX, *n_found = hits (zeroed on the stream first); err = 1 if a walk found no EMPTY slot
hipError_t dedupe_lookup_launch(unsigned words, const uint64_t *dig, uint32_t n, const uint64_t *state, const uint64_t *value, const uint64_t *key,
                                uint64_t mask, uint64_t *ref, uint64_t *n_found, unsigned long long *err, hipStream_t s);
// export = compaction of the committed slots in slot order, in tiles of 256 slots: counts[tiles] (u32) and offs[tiles + 1] are the
// caller's scratch; the scatter writes pairs [first, first + max_out) of that order and the entry count to *d_n (may be NULL)
uint64_t dedupe_export_tiles(uint64_t cap);
hipError_t dedupe_export_scan_launch(const uint64_t *state, uint64_t cap, uint32_t *counts, uint64_t *offs, hipStream_t s);
hipError_t dedupe_export_scatter_launch(unsigned words, const uint64_t *state, const uint64_t *value, const uint64_t *key, uint64_t cap,
                                        const uint64_t *offs, uint64_t first, uint64_t max_out, uint64_t *out_dig, uint64_t *out_val, uint64_t *d_n,
                                        hipStream_t s);
// the digests of the flagged directory entries' values in ascending value (cw_dev_dedupe_export_live): flags[dir_entries] (u32) and
// rank[dir_entries + 1] are the caller's scratch; result[2] = {flagged entries, table entries with a flagged value}
hipError_t dedupe_export_live_launch(unsigned words, const uint64_t *state, const uint64_t *value, const uint64_t *key, uint64_t cap,
                                     const uint32_t *live, uint64_t dir_base, uint64_t dir_entries, uint32_t *flags, uint64_t *rank, uint64_t max_out,
                                     uint64_t *out_dig, uint64_t *out_val, uint64_t *result, hipStream_t s);
// every committed entry of the old table into the (empty) new one; err = 1 if an entry found no slot
hipError_t dedupe_rehash_launch(unsigned words, const uint64_t *old_state, const uint64_t *old_value, const uint64_t *old_key, uint64_t old_cap,
                                uint64_t *state, uint64_t *value, uint64_t *key, uint64_t mask, unsigned long long *err, hipStream_t s);
// the rehash of the entries whose value names no entry of [dir_base, dir_base + dir_entries) or a flagged one (live[v - dir_base] != 0);
// *n_kept += their number.  state == NULL: only counts
hipError_t dedupe_retain_launch(unsigned words, const uint64_t *old_state, const uint64_t *old_value, const uint64_t *old_key, uint64_t old_cap,
                                const uint32_t *live, uint64_t dir_base, uint64_t dir_entries, uint64_t *state, uint64_t *value, uint64_t *key,
                                uint64_t mask, unsigned long long *n_kept, unsigned long long *err, hipStream_t s);
// values through the ascending pairs from[0..min(*d_npairs, max_pairs)) -> to (cw_dev_dedupe_revalue): head[2] is the caller's scratch
// (hits, stale); result[3] = {verdict, hits, stale}; value[] changes only when no committed entry is stale
hipError_t dedupe_revalue_launch(const uint64_t *state, uint64_t *value, uint64_t cap, const uint64_t *from, const uint64_t *to,
                                 const uint64_t *d_npairs, uint64_t max_pairs, uint64_t range_base, uint64_t range_entries, uint64_t *head,
                                 uint64_t *result, hipStream_t s);
// block new_idx[j] (src_stride apart in src) -> dst + j * block_bytes, for j < n_new
hipError_t dedupe_gather_launch(const uint8_t *src, size_t block_bytes, size_t src_stride, const uint32_t *new_idx, size_t n_new,
                                uint8_t *dst, hipStream_t s);
// content-defined chunking (cdc_kernels.hip): gear = 256 entries in HOST memory (copied into the stream's workspace)
struct CdcParams { uint32_t min_size, normal_size, max_size; uint64_t mask_s, mask_l; const uint64_t *gear; };
// the resolve's segment: CW_CDC_SEGMENT bytes (>= max_size), by default 256 KiB rounded up to a multiple of max_size
uint64_t cdc_segment_bytes(uint32_t max_size, long knob);
size_t cdc_workspace_bytes(size_t nbytes, uint32_t min_size, uint64_t seg);
// offsets[0..K] and *nchunks = K on the device; at most nbytes / min_size + 2 offsets are written
hipError_t cdc_launch(const CdcParams &p, const uint8_t *src, size_t nbytes, int final_, uint64_t *offsets, size_t max_offsets,
                      uint64_t *nchunks, uint64_t seg, hipStream_t stream);
// many streams in one buffer (cw_dev_cdc_streams): ends[nstreams], first[nstreams + 1] and *result on the device; at most
// nbytes / min_size + nstreams + 1 offsets are written
// final_ = 0 (cw_dev_cdc_streams_part): the last stream is open and its chain stops where less than max_size is left
struct CdcStreams { const uint64_t *ends; size_t nstreams; uint64_t *first, *result; int final_ = 1; };
size_t cdc_streams_workspace_bytes(size_t nbytes, size_t nstreams, uint32_t min_size, uint64_t seg);
hipError_t cdc_streams_launch(const CdcParams &p, const uint8_t *src, size_t nbytes, const CdcStreams &st, uint64_t *offsets, size_t max_offsets,
                              uint64_t *nchunks, uint64_t seg, hipStream_t stream);
// the resync of an edit's window (patch_kernels.hip; semantics: the public header's cw_dev_cdc_resync)
hipError_t cdc_resync_launch(const uint64_t *new_offsets, uint64_t *d_new_count, size_t max_new, const uint64_t *old_offsets,
                             const uint64_t *d_old_count, size_t max_old, uint64_t new_from, uint64_t shift, int keep_all, uint64_t *result,
                             hipStream_t stream);
// orders the chunks i < min(*d_n, max_chunks) by (length >> step_shift), longest first, into a permutation in the stream's
// workspace, and calls hash.fn(hash.ctx, perm) to queue the hash that reads it -- both under the workspace's launch lock
struct ChunkHash { hipError_t (*fn)(void *ctx, const uint32_t *perm); void *ctx; };
hipError_t chunk_hash_launch(const uint64_t *offsets, const uint64_t *d_n, size_t max_chunks, size_t src_bytes, unsigned step_shift,
                             const ChunkHash &hash, hipStream_t stream);
// digest of chunk perm[j] = [offsets[i], offsets[i + 1]) clamped to [0, src_bytes), for j < min(*d_n, max_chunks), at digests + i * digest_bytes
hipError_t skein_chunks_launch(int state_words, const uint8_t *src, size_t src_bytes, const uint64_t *offsets, const uint32_t *perm,
                               const uint64_t *d_n, size_t max_chunks, const SkeinIV &iv, uint8_t *digests, unsigned digest_bytes,
                               hipStream_t stream);
hipError_t sha256_chunks_launch(const uint8_t *src, size_t src_bytes, const uint64_t *offsets, const uint32_t *perm, const uint64_t *d_n,
                                size_t max_chunks, uint8_t *digests, hipStream_t stream);

// Message bytes of a chunk that starts at any byte: the NG aligned 16-byte granules from a16, each clamped to `last` (the last
// granule that holds a byte of the source), then shifted down by sh = 0..15 bytes with v_alignbyte_b32 -- 4 * (NG - 1) dwords.
template <int NG>
__device__ __forceinline__ void chunk_granules(uint32_t (&d)[4 * NG], const uint8_t *a16, const uint8_t *last)
{
#pragma unroll
    for (int g = 0; g < NG; g++) {
        const uint8_t *q = a16 + 16 * g;
        const uint4 v = *reinterpret_cast<const uint4 *>(q < last ? q : last);
        d[4 * g] = v.x; d[4 * g + 1] = v.y; d[4 * g + 2] = v.z; d[4 * g + 3] = v.w;
    }
}
template <int NG>
__device__ __forceinline__ void chunk_shift(uint32_t (&out)[4 * (NG - 1)], const uint32_t (&d)[4 * NG], unsigned sh)
{
    const unsigned ds = sh >> 2, bs = sh & 3;
    uint32_t sel[4 * (NG - 1) + 1];
#pragma unroll
    for (int k = 0; k <= 4 * (NG - 1); k++) {
        const uint32_t a0 = d[k], a1 = d[k + 1 < 4 * NG ? k + 1 : k], a2 = d[k + 2 < 4 * NG ? k + 2 : k], a3 = d[k + 3 < 4 * NG ? k + 3 : k];
        sel[k] = ds == 0 ? a0 : ds == 1 ? a1 : ds == 2 ? a2 : a3;
    }
#pragma unroll
    for (int k = 0; k < 4 * (NG - 1); k++) out[k] = __builtin_amdgcn_alignbyte(sel[k + 1], sel[k], bs);
}
// keeps the bytes of dword k (at source position pos + 4k) that lie before end
__device__ __forceinline__ uint32_t chunk_keep(uint32_t v, int64_t valid)
{
    return valid >= 4 ? v : valid <= 0 ? 0u : v & ((1u << (8 * (unsigned)valid)) - 1u);
}

// ---- codecs over chunks (chunk_codec_kernels.hip, pack_kernels.hip; semantics: the public header) ------------------------
// where compressed chunk i, at input offset o, goes in the slot buffer (cw_chunk_slot_offset)
__host__ __device__ inline uint64_t chunk_slot_offset(bool lz4, uint64_t o, uint64_t i)
{
    return lz4 ? (o + o / 255 + 32 * i) & ~(uint64_t)15 : o;
}
__device__ __forceinline__ uint64_t umin64(uint64_t a, uint64_t b) { return a < b ? a : b; }
constexpr uint32_t kMaxChunkBytes = 65536; // CW_MAX_BLOCK_BYTES
// The positions of a call over chunks and the chunk behind each (cw_dev_compress_chunks' arguments; cw_dev_store_chunks reads the
// same list behind it).
struct ChunkList {
    const uint64_t *offsets, *d_nchunks;
    const uint32_t *sel;      // NULL: position j is chunk j
    const uint64_t *d_nsel;
    uint64_t max_chunks, src_bytes;

    __device__ __forceinline__ uint64_t nchunks() const { return umin64(*d_nchunks, max_chunks); }
    __device__ __forceinline__ uint64_t npos() const { return sel ? umin64(*d_nsel, max_chunks) : nchunks(); }
    // chunk of position j and its length; 0 = out of contract (then nothing of it may be loaded or stored)
    __device__ __forceinline__ uint32_t chunk(uint64_t j, uint64_t count, uint64_t &i, uint64_t &start) const
    {
        i = sel ? sel[j] : j;
        start = 0;
        if (i >= count) return 0;
        const uint64_t s = offsets[i], e = offsets[i + 1];
        if (!(s < e && e <= src_bytes && e - s <= kMaxChunkBytes)) return 0;
        start = s;
        return (uint32_t)(e - s);
    }
};
// bytes of table per lane of the chunk parsers (the workspace holds up to 131,072 / 65,536 of them, LZ4 / LZF)
size_t chunk_lane_table_bytes(int lzf);
// sel == NULL: every chunk i < min(*d_nchunks, max_chunks); else the chunks sel[j], j < min(*d_nsel, max_chunks); sizes per position
hipError_t chunk_compress_launch(int lzf, const uint8_t *src, size_t src_bytes, const uint64_t *offsets, const uint64_t *d_nchunks,
                                 size_t max_chunks, const uint32_t *sel, const uint64_t *d_nsel, uint8_t *dst, uint32_t *sizes,
                                 hipStream_t stream);
hipError_t chunk_decompress_launch(int lzf, const uint8_t *comp, const uint64_t *comp_offsets, const uint64_t *raw_offsets,
                                   const uint64_t *d_count, size_t max_count, uint8_t *dst, size_t dst_bytes, uint32_t *status,
                                   hipStream_t stream);
// pack_launch for chunk slots and a count on the device: packed_offsets[0..n], n = min(*d_count, max_count)
hipError_t chunk_pack_launch(int lzf, const uint8_t *slots, const uint64_t *offsets, const uint32_t *sel, const uint64_t *d_count,
                             size_t max_count, const uint32_t *sizes, uint8_t *packed, uint64_t *packed_offsets, hipStream_t stream);

// the chunk store (restore_kernels.hip; semantics: the public header).  dir: cw_chunk_loc entries, 16-byte aligned
hipError_t chunk_store_launch(int lzf, const uint8_t *src, size_t src_bytes, const uint64_t *offsets, const uint64_t *d_nchunks, size_t max_chunks,
                              const uint32_t *sel, const uint64_t *d_nsel, const uint8_t *slots, const uint32_t *sizes, uint64_t base,
                              uint8_t *store, size_t store_bytes, uint64_t *d_used, void *dir, uint64_t dir_base, size_t dir_entries,
                              uint64_t *result, hipStream_t stream);
hipError_t chunk_restore_launch(int lzf, const uint8_t *store, size_t store_bytes, const void *dir, uint64_t dir_base, size_t dir_entries,
                                const uint64_t *ref, const uint64_t *raw_offsets, const uint64_t *d_count, size_t max_count, uint8_t *dst,
                                size_t dst_bytes, uint32_t *status, hipStream_t stream);
// a streamed ingest (ingest_kernels.hip; semantics: the public header's cw_dev_ingest_commit and cw_dev_ingest_commit_streams).  One
// pair of kernels and one launch mutex per stream serve both commits: ingest_commit_launch is ingest_commit_streams_launch with the
// empty list {nullptr, 0, 0, 0, nullptr, 0}.  piece_counts_launch: counts[0..4) = min(*d_nchunks, max_chunks), the bytes those chunks
// cover, *d_used, *d_verdict
struct CommitStreams { const uint64_t *first; uint64_t nstreams, first_stream, skip_first; uint64_t *rec_first; uint64_t first_cap; };
hipError_t ingest_commit_launch(const uint64_t *ref, const uint64_t *offsets, const uint64_t *d_nchunks, size_t max_chunks, const uint64_t *d_n_new,
                                const uint64_t *store_result, uint64_t stream_off, uint64_t *rec_ref, uint64_t *rec_off, uint64_t *d_rec_count,
                                size_t rec_cap, uint64_t *stats, uint64_t *d_verdict, hipStream_t stream);
hipError_t piece_counts_launch(const uint64_t *offsets, const uint64_t *d_nchunks, size_t max_chunks, const uint64_t *d_used,
                               const uint64_t *d_verdict, uint64_t *counts, hipStream_t stream);
hipError_t ingest_commit_streams_launch(const uint64_t *ref, const uint64_t *offsets, const uint64_t *d_nchunks, size_t max_chunks,
                                        const uint64_t *d_n_new, const uint64_t *store_result, uint64_t stream_off, uint64_t *rec_ref,
                                        uint64_t *rec_off, uint64_t *d_rec_count, size_t rec_cap, uint64_t *stats, uint64_t *d_verdict,
                                        const CommitStreams &cs, hipStream_t stream);
// byte ranges of a restored stream (read_kernels.hip; semantics: the public header).  The recipe as chunk_restore_launch takes it
hipError_t read_ranges_launch(int lzf, const uint8_t *store, size_t store_bytes, const void *dir, uint64_t dir_base, size_t dir_entries,
                              const uint64_t *ref, const uint64_t *raw_offsets, const uint64_t *d_count, size_t max_count,
                              const uint64_t *range_off, const uint64_t *range_len, const uint64_t *range_dst, const uint64_t *d_nranges,
                              size_t max_ranges, uint8_t *dst, size_t dst_bytes, uint32_t *status, hipStream_t stream);
size_t read_ranges_scratch_bytes(size_t max_ranges); // what a call reserves at most

// mark and compact (store_gc_kernels.hip; semantics: the public header).  new_dir may be dir itself
hipError_t store_mark_launch(const uint64_t *ref, const uint64_t *d_count, size_t max_count, uint64_t dir_base, size_t dir_entries,
                             uint32_t *live, uint64_t *n_outside, hipStream_t stream);
hipError_t store_compact_launch(const uint8_t *store, size_t store_bytes, const void *dir, size_t dir_entries, const uint32_t *live,
                                uint8_t *new_store, size_t new_store_bytes, uint64_t *new_used, void *new_dir, uint64_t *result,
                                hipStream_t stream);

// renumber (renumber_kernels.hip; semantics: the public header).  live may be NULL; new_dir, from and to may be when their counts are 0
hipError_t store_renumber_launch(const void *dir, uint64_t dir_base, size_t dir_entries, const uint32_t *live, uint64_t new_base, void *new_dir,
                                 uint64_t new_dir_base, size_t new_dir_entries, uint64_t *from, uint64_t *to, size_t max_pairs, uint64_t *result,
                                 hipStream_t stream);

// account (account_kernels.hip; semantics: the public header).  acct: cw_stream_account[nstreams]; flag, refcount and owner may be
// NULL, ref may be when max_positions is 0
hipError_t store_account_launch(const uint64_t *ref, const uint64_t *first, size_t nstreams, size_t max_positions, const void *dir,
                                uint64_t dir_base, size_t dir_entries, const uint32_t *flag, void *acct, uint32_t *refcount, uint32_t *owner,
                                uint64_t *totals, hipStream_t stream);

// recipe diff and delta apply (delta_kernels.hip; semantics: the public header).  ops: cw_delta_op entries; src and the four range
// arrays may be NULL
hipError_t recipe_diff_launch(const uint64_t *ref_a, const uint64_t *off_a, const uint64_t *d_na, size_t max_a, const uint64_t *ref_b,
                              const uint64_t *off_b, const uint64_t *d_nb, size_t max_b, uint64_t dir_base, size_t dir_entries, void *ops,
                              size_t max_ops, uint64_t *nops, uint64_t *src, uint64_t *new_off, uint64_t *new_len, uint64_t *new_dst,
                              uint64_t *nnew, uint64_t *totals, hipStream_t stream);
size_t recipe_diff_scratch_bytes(size_t max_b, size_t dir_entries);
unsigned apply_delta_tile_shift(long knob_kib); // CW_DELTA_TILE: 16, 64 or 256 (KiB); anything else is the default
hipError_t apply_delta_launch(const uint8_t *old, size_t old_bytes, const uint8_t *payload, size_t payload_bytes, const void *ops,
                              const uint64_t *d_nops, size_t max_ops, uint8_t *dst, size_t dst_bytes, unsigned tile_shift, uint64_t *result,
                              hipStream_t stream);

// the device steps of a compose (compose_kernels.hip; semantics: the public header).  win: cw_resync_window entries; ext: three words
// per extent (src_off, dst_off, len)
hipError_t cdc_resync_windows_launch(const uint64_t *new_offsets, const uint64_t *d_new_count, size_t max_new, const uint64_t *stream_first,
                                     const void *win, size_t nwin, const uint64_t *old_offsets, size_t max_old, uint64_t *result, hipStream_t stream);
hipError_t scatter_extents_launch(const uint8_t *src, size_t src_bytes, const uint64_t *ext, const uint64_t *d_n, size_t max_n, uint8_t *dst,
                                  size_t dst_bytes, uint64_t *result, hipStream_t stream);

// chunk bundles between stores (replicate_kernels.hip; semantics: the public header).  loc / dir: cw_chunk_loc entries, 16-byte aligned
hipError_t store_export_launch(const uint8_t *store, size_t store_bytes, const void *dir, uint64_t dir_base, size_t dir_entries,
                               const uint64_t *values, const uint64_t *d_count, size_t max_count, uint8_t *out, size_t out_bytes, void *out_loc,
                               uint64_t *result, hipStream_t stream);
hipError_t store_import_launch(const uint8_t *in, size_t in_bytes, const void *in_loc, const uint64_t *d_count, size_t max_count,
                               const uint32_t *sel, const uint64_t *d_nsel, uint64_t base, uint8_t *store, size_t store_bytes, uint64_t *d_used,
                               void *dir, uint64_t dir_base, size_t dir_entries, uint64_t *result, hipStream_t stream);
hipError_t translate_refs_launch(const uint64_t *ref, const uint64_t *d_count, size_t max_count, const uint64_t *from, const uint64_t *to,
                                 const uint64_t *d_npairs, size_t max_pairs, uint64_t *out, uint64_t *n_missing, hipStream_t stream);
// cw_dev_store_replace_chunks: the import with the values given (position k carries values[k]) and no selection
hipError_t store_replace_launch(const uint8_t *in, size_t in_bytes, const void *in_loc, const uint64_t *values, const uint64_t *d_count,
                                size_t max_count, uint8_t *store, size_t store_bytes, uint64_t *d_used, void *dir, uint64_t dir_base,
                                size_t dir_entries, uint64_t *result, hipStream_t stream);

// one window of a scrub (scrub_kernels.hip; semantics: the public header's cw_dev_store_verify).  The window in the stream's scratch,
// as the judge sees it behind the restore: head[0] = c, head[1] = e - c (= *d_count); raw_off[0 .. e - c] the decoded chunks' extents
// in the work buffer; decoded[k] = the restore's status; verdict[k] = CW_SCRUB_ORPHAN for the entries that were decoded
struct ScrubWindow {
    const uint64_t *head, *raw_off, *d_count;
    size_t max_entries;
    const uint32_t *decoded;
    uint8_t *digests;   // of the window's chunks, for the judge to fill
    uint32_t *verdict;  // for the judge to lower
};
// queues the hash of the window's chunks and the sweep of the table that compares: called once, under the scratch's launch lock
struct ScrubJudge { hipError_t (*fn)(void *ctx, const ScrubWindow &w); void *ctx; };
size_t store_verify_window(size_t dir_entries, long knob); // W = min(CW_SCRUB_ENTRIES (default 2^20, at least 64), dir_entries)
size_t store_verify_scratch_bytes(size_t window, unsigned digest_bytes);
hipError_t store_verify_launch(int lzf, const uint8_t *store, size_t store_bytes, const void *dir, uint64_t dir_base, size_t dir_entries,
                               const uint32_t *live, uint64_t *d_cursor, uint8_t *work, size_t work_bytes, size_t window, unsigned digest_bytes,
                               uint32_t *status, uint64_t *totals, const ScrubJudge &judge, hipStream_t stream);
// the table sweep of a scrub window (dedupe_kernels.hip): a committed slot whose value names a decoded entry of the window lowers
// verdict[k] to 0 when its key is digests[k], else to 3
hipError_t dedupe_verify_launch(unsigned words, const uint64_t *state, const uint64_t *value, const uint64_t *key, uint64_t cap, uint64_t dir_base,
                                const uint64_t *head, const uint32_t *decoded, const uint64_t *digests, uint32_t *verdict, hipStream_t s);

// Guard stripes over the store's bytes (guard_kernels.hip; semantics: the public header): the XOR guard P and, when guard_q is not
// NULL, the GF(2^8) syndrome Q beside it (the dual guard, group <= 255).  The geometry is checked by the caller; groups = the groups
// of store_bytes, ceil(store_bytes / (stripe * group)); group_bad, out and out_loc may be NULL as the header says.  result is [4],
// the dual rebuild's [5]
size_t store_guard_groups(size_t store_bytes, size_t stripe, unsigned group);
size_t store_guard_check_scratch_bytes(size_t groups, bool dual);
size_t store_guard_rebuild_scratch_bytes(size_t max_count, size_t groups);
hipError_t store_guard_update_launch(const uint8_t *store, size_t store_bytes, const uint64_t *d_used, uint64_t *d_covered, size_t stripe,
                                     unsigned group, void *guard_p, void *guard_q, uint64_t *result, hipStream_t stream);
hipError_t store_guard_check_launch(const uint8_t *store, size_t store_bytes, const uint64_t *d_covered, size_t stripe, unsigned group,
                                    const void *guard_p, const void *guard_q, uint32_t *group_bad, uint64_t *result, hipStream_t stream);
hipError_t store_guard_rebuild_launch(const uint8_t *store, size_t store_bytes, const void *dir, uint64_t dir_base, size_t dir_entries,
                                      const uint64_t *d_covered, size_t stripe, unsigned group, const void *guard_p, const void *guard_q,
                                      const uint64_t *values, const uint64_t *d_count, size_t max_count, uint8_t *out, size_t out_bytes, void *out_loc,
                                      uint32_t *status, uint64_t *result, hipStream_t stream);
// The entries the syndromes suspect (guard_locate_kernels.hip): suspect is u32[dir_entries], result is [8]; scratch per stream
size_t store_guard_locate_scratch_bytes(size_t groups, size_t stripe);
hipError_t store_guard_locate_launch(const uint8_t *store, size_t store_bytes, const void *dir, size_t dir_entries, const uint64_t *d_covered,
                                     size_t stripe, unsigned group, const void *guard_p, const void *guard_q, uint32_t *suspect, uint64_t *result,
                                     hipStream_t stream);

hipError_t sum_sizes_launch(const uint32_t *sizes, size_t n, uint32_t raw_bytes, uint64_t *totals, hipStream_t stream);
hipError_t gen_random_launch(uint64_t seed, uint64_t first_block, size_t nblocks, size_t block_bytes, uint8_t *dst,
                             hipStream_t stream);
hipError_t gen_mixed_launch(uint64_t seed, uint64_t first_block, size_t nblocks, size_t block_bytes, uint8_t *dst,
                            hipStream_t stream);

} // namespace cw
