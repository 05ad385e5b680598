/*
 * cw_hashcompress.h -- C ABI of libcwhc.so: the MI355X (gfx950) back end for the reference's
 * per-block hash + front-end compression hot path.
 *
 * Every entry point names the reference interface it replaces (paths relative to the
 * reference repository).  Plain pointers and sizes only; no C++/torch types cross this line.
 *
 *   slots      doHashing / doCompression          src/hashandcompress/HashAndCompress.cpp:111,119
 *   hashes     doSkeinHashing                     src/hashandcompress/HashAndCompress.cpp:121-134
 *              doSHA256MBHashing                  src/hashandcompress/HashAndCompress.cpp:136-158
 *              HashBlockSkein256/SHA256/SHA256MB  src/hashing_perf/hash.cpp:5-77
 *   codecs     lz4 / lzf lambdas                  src/hashandcompress/HashAndCompress.cpp:342-355
 *   GPU seam   initializeGpu()                    src/hashandcompress/HashAndCompress.cpp:95-98
 *              class HashOffload                  src/hashandcompress/HashOffload.h:13-64
 *              hashing_offload_entry_point        src/hashandcompress/HashAndCompress.cpp:160-183
 *
 * Threading: every function may be called concurrently from any number of host threads
 * (the reference calls its slots from --c-threads workers, :398-402); each calling thread
 * gets its own HIP streams and staging buffers per device.  The cw_dev_* functions may also be
 * called from several threads on the SAME stream: each call's launch sequence is queued
 * atomically (a per-(device, stream) mutex), so the calls execute in some serial order.
 *
 * Devices: cw_init(d) / cw_set_device(d) initialise device d (if needed) and make it the calling
 * thread's device; threads that never choose use the first initialised device.  Device pointers
 * and streams passed to cw_dev_* must belong to the calling thread's device.
 *
 * There is NO CPU fallback: every compute entry point fails (CW_ERR_NO_DEVICE / abort in the
 * void slot wrappers) when no gfx950 device is usable.
 */
#ifndef CW_HASHCOMPRESS_H
#define CW_HASHCOMPRESS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes -------------------------------------------------------------------------- */
enum {
    CW_OK = 0,
    CW_ERR_NO_DEVICE = -1,   /* no usable HIP device / cw_init not possible */
    CW_ERR_BAD_ARG = -2,     /* unknown algorithm, NULL pointer, size out of the supported range */
    CW_ERR_HIP = -3,         /* a HIP runtime call failed; see cw_last_error() */
    CW_ERR_STATE = -4,       /* offload object used out of order (HashOffload's asserts) */
    CW_ERR_NOMEM = -5
};

/* --hash-alg values of the driver (:361-370) plus the north-star Skein-512-512 */
typedef enum cw_hash_alg {
    CW_HASH_SKEIN512 = 0,      /* Skein-512, 512-bit digest (reference_code/skein, skein.c:226-408) */
    CW_HASH_SKEIN256_128 = 1,  /* "skein": Skein-256, 128-bit digest (kHashSizeBytesSkein=16, hash.h:16) */
    CW_HASH_SHA256 = 2,        /* "sha256mb": FIPS 180-4 SHA-256 of each block (kHashSizeBytesSHA=32) */
    CW_HASH_NONE = 3
} cw_hash_alg;

/* --comp-alg values of the driver (:342-355) */
typedef enum cw_comp_alg {
    CW_COMP_LZ4 = 0,           /* LZ4_compress_default(s, d, l, 2*l), LZ4 v1.8.2 */
    CW_COMP_LZF = 1,           /* lzf_compress(s, l, d, l-1), liblzf HLOG 16 / VERY_FAST */
    CW_COMP_NONE = 2
} cw_comp_alg;

/* ---- lifecycle: initializeGpu() (:95-98) and the shutdown hook (:182) ----------------------- */
int  cw_init(int device);            /* initialise `device` (idempotent) and make it the calling thread's device */
void cw_shutdown(void);              /* every initialised device: synchronise, free the library's scratch */
int  cw_device_count(void);          /* usable gfx950 devices (0 when none) */
int  cw_set_device(int device);      /* = cw_init: the device the calling thread's next calls run on (--devices) */
int  cw_get_device(void);            /* the calling thread's device, -1 before any cw_init */
const char *cw_last_error(void);     /* message of the calling thread's last failure */
const char *cw_version(void);

/* ---- sizes ---------------------------------------------------------------------------------- */
size_t cw_digest_bytes(int hash_alg);                        /* 64 / 16 / 32 / 0 */
size_t cw_compress_bound(int comp_alg, size_t block_bytes);  /* output slot a block may need:
                                                                lz4: l + l/255 + 16 (LZ4_compressBound); lzf: l */
#define CW_MAX_BLOCK_BYTES 65536u   /* LZ4's 16-bit-table regime of the reference (< 65547) */

/* ---- the two slots, host pointers, synchronous -- drop-in for the reference's function objects --
 * void doHashing(const char* src, char* dst, int count)  hashes `count` consecutive blocks of
 * cw_get_block_size() bytes at src into count consecutive digests at dst (:121-133).
 * size_t doCompression(const char* src, char* dst, size_t len) compresses one block; returns the
 * compressed size, 0 = did not fit (lzf, lzf.h:59-64).  dst capacity is 2*len (lz4) / len-1 (lzf),
 * as the reference's callers provide (:234-239, :346, :353).
 * The void slots abort() with a message on a device error, since the reference's slots cannot
 * report one (SURVEY.md 8b "Errors").                                                            */
void   cw_set_block_size(size_t block_bytes);   /* the reference's global blockSize (:89), default 4096 */
size_t cw_get_block_size(void);
void   cw_hash_skein(const char *src, char *dst, int count);      /* doSkeinHashing: Skein-256-128 */
void   cw_hash_skein512(const char *src, char *dst, int count);   /* Skein-512-512 */
void   cw_hash_sha256mb(const char *src, char *dst, int count);   /* doSHA256MBHashing (digests ARE returned) */
size_t cw_compress_lz4(const char *src, char *dst, size_t len);
size_t cw_compress_lzf(const char *src, char *dst, size_t len);
/* The decoders the reference times beside the compressors (src/compression_perf/src/experiment.cpp:118,256):
 *   int LZ4_decompress_safe(src, dst, csize, dst_cap)           -> decoded bytes, < 0 = malformed
 *   unsigned lzf_decompress(src, csize, dst, dst_cap)           -> decoded bytes, 0 = error (lzf.h:83-97)
 * One difference: the device decoder is told the decoded size, so a slot must decode to exactly
 * cw_get_block_size() bytes (what every caller in the reference expects); anything else is "malformed". */
int      cw_decompress_lz4(const char *src, char *dst, int csize, int dst_cap);
unsigned cw_decompress_lzf(const void *src, unsigned csize, void *dst, unsigned dst_cap);

/* ---- batched host API: many blocks per call (H2D, kernels, D2H on the caller's stream) --------
 * src: nblocks * block_bytes contiguous; digests: nblocks * cw_digest_bytes(); dst: nblocks slots of
 * dst_stride >= cw_compress_bound(); sizes[i] = compressed bytes of block i (0 = did not fit).
 * Any of digests / (dst,sizes) may be NULL to skip that half.  This is ProcessBlock (:231-261) for
 * a whole read-unit or file at once.                                                              */
int cw_hash_blocks(int hash_alg, const void *src, size_t block_bytes, size_t nblocks, void *digests);
int cw_compress_blocks(int comp_alg, const void *src, size_t block_bytes, size_t nblocks,
                       void *dst, size_t dst_stride, uint32_t *sizes);
int cw_hash_and_compress_blocks(int hash_alg, int comp_alg, const void *src, size_t block_bytes,
                                size_t nblocks, void *digests, void *dst, size_t dst_stride,
                                uint32_t *sizes);
/* Same work, packed output: the compressed blocks arrive as ONE stream (block i at packed + offsets[i], sizes[i] bytes;
 * offsets has nblocks + 1 entries, the last one the total; a block that did not fit occupies nothing) -- the device
 * packs the slots (cw_dev_pack) so only compressed bytes cross the bus, and with a page-locked `packed` buffer they land
 * in place with no copy on the host.  packed_cap must cover the total (nblocks * cw_compress_bound() always does). */
int cw_hash_and_compress_packed(int hash_alg, int comp_alg, const void *src, size_t block_bytes,
                                size_t nblocks, void *digests, void *packed, size_t packed_cap,
                                uint64_t *offsets, uint32_t *sizes);
/* Both forms run as a three-stage pipeline (host->device copy of chunk k+1 | kernels of chunk k | device->host copy of
 * chunk k-1: what HashOffload::Start()/Complete() were meant to be, HashOffload.h:26-40).  The copy engines read and
 * write page-locked host memory in place; other buffers go through pinned staging with one memcpy.  Chunks are 512 MiB
 * (4.6 GiB of device memory per calling thread and device, plus the codecs' per-stream scratch: up to 4 GiB (LZ4) / 8 GiB (LZF)
 * of lane-parser tables on each of the three slot streams once a chunk is large enough for the lanes -- a device that cannot give
 * them runs the call without the lanes instead of failing it); with page-locked buffers on both sides, chunks of blocks
 * above 4 KiB grow to 2 GiB once the first results show that the data compresses (18.5 GiB then), because the codecs
 * reach their rate only on tens of thousands of blocks at a time.  To get buffers the engines can use directly:       */
/* initializeGpu() (:95-98) for the calling thread: its context on its device plus everything the batch path would allocate
 * on first use for batches of up to nblocks blocks (pinned_io: the caller's buffers are page-locked, no staging needed) */
int   cw_prepare(int hash_alg, int comp_alg, size_t block_bytes, size_t nblocks, int pinned_io);
void *cw_host_alloc(size_t bytes);               /* page-locked host memory (NULL on failure) */
void  cw_host_free(void *p);
int   cw_host_register(void *p, size_t bytes);   /* page-lock an existing buffer (e.g. the driver's read units) */
int   cw_host_unregister(void *p);
/* decode nblocks slots (comp_stride apart, sizes[i] bytes each) into nblocks * block_bytes at dst;
 * status[i] = 0 iff slot i is well formed and yields exactly block_bytes (see cw_dev_decompress).  */
/* host-buffer form of cw_dev_hash_tree */
int cw_hash_tree_blocks(int hash_alg, const void *src, size_t block_bytes, size_t nblocks, unsigned leaf, unsigned node,
                        unsigned max_level, void *digests);
int cw_decompress_blocks(int comp_alg, const void *comp, size_t comp_stride, const uint32_t *sizes,
                         size_t nblocks, void *dst, size_t block_bytes, uint32_t *status);

/* ---- device-resident API: every pointer is device memory, work is queued on `stream`
 *      (a hipStream_t passed as void*; NULL = the default stream) and NOT synchronised -----------
 * src_stride = bytes between consecutive blocks (>= block_bytes).                                 */
int cw_dev_hash(int hash_alg, const void *d_src, size_t block_bytes, size_t src_stride, size_t nblocks,
                void *d_digests, void *stream);
int cw_dev_compress(int comp_alg, const void *d_src, size_t block_bytes, size_t src_stride,
                    size_t nblocks, void *d_dst, size_t dst_stride, uint32_t *d_sizes, void *stream);
int cw_dev_hash_and_compress(int hash_alg, int comp_alg, const void *d_src, size_t block_bytes,
                             size_t src_stride, size_t nblocks, void *d_digests, void *d_dst,
                             size_t dst_stride, uint32_t *d_sizes, void *stream);
/* Decoders (the reference calls LZ4_decompress_safe / lzf_decompress only to time them,
 * src/compression_perf/src/experiment.cpp:118,256): decode nblocks compressed slots (comp_stride apart, d_sizes[i]
 * bytes each) into nblocks * block_bytes at d_dst; d_status[i] = 0 iff slot i is well formed and yields exactly
 * block_bytes.  Used as the reference-independent round-trip verifier of the compressors.
 * The verdict is a property of the slot alone: it does not depend on nblocks, block_bytes' size class or any knob
 * that routes a batch to one decoder kernel or another.  A valid stream may be longer than block_bytes (LZF: up to
 * 2 * block_bytes with 1-byte literal runs); it is valid if it fits the slot, d_sizes[i] <= comp_stride.  A size of 0
 * or beyond comp_stride gives status 1 and nothing is read or written.  The bytes of a block with status 1 are
 * unspecified; nothing outside a slot's block_bytes of d_dst is ever written.                                     */
int cw_dev_decompress(int comp_alg, const void *d_comp, size_t comp_stride, const uint32_t *d_sizes, size_t nblocks,
                      void *d_dst, size_t block_bytes, uint32_t *d_status, void *stream);
/* Skein tree hashing of every block (the reference's Skein_TreeHash,
 * reference_code/skein/Additional_Implementations/skein_test.c:616-680, tree fields skein.h:209-210): leaves of
 * state_bytes << leaf bytes, nodes of state_bytes << node bytes, at most max_level levels (>= 2; 255 = unlimited).
 * NOT the digest of cw_dev_hash -- tree mode changes the configuration block -- but one wavefront hashes a block with
 * lane-per-leaf parallelism, so a few large blocks already fill the GPU.  hash_alg: CW_HASH_SKEIN512 (64-byte digests)
 * or CW_HASH_SKEIN256_128 (16-byte digests).  The level buffers live in LDS: (block_bytes >> leaf) * 1.5 <= 64 KiB.   */
int cw_dev_hash_tree(int hash_alg, const void *d_src, size_t block_bytes, size_t src_stride, size_t nblocks,
                     unsigned leaf, unsigned node, unsigned max_level, void *d_digests, void *stream);
/* Packed output stream + block index: d_offsets[i] = sum of d_sizes[0..i) (u64, nblocks + 1
 * entries, the last one is the total); slot i's d_sizes[i] bytes are copied to d_packed + d_offsets[i].  A block that
 * did not fit (size 0) occupies nothing.  d_packed may be NULL: index only.  d_packed needs sum(d_sizes) bytes
 * (at most nblocks * slot_stride).                                                                              */
int cw_dev_pack(const void *d_slots, size_t slot_stride, const uint32_t *d_sizes, size_t nblocks,
                void *d_packed, uint64_t *d_offsets, void *stream);
/* synthetic input: u64 word w of block b = splitmix64(seed ^ (b << 13 | w)) */
int cw_dev_gen_random(uint64_t seed, uint64_t first_block, size_t nblocks, size_t block_bytes,
                      void *d_dst, void *stream);
/* compressible synthetic mix: even blocks as cw_dev_gen_random, odd blocks = a 64-byte motif repeated with
 * every byte replaced by a random one with probability 1/16 (exact definition: csrc/misc_kernels.hip, host twin
 * oracle/hc_oracle.c) -- so that the codecs' match/emit loops are timed, not only their incompressible fast path */
int cw_dev_gen_mixed(uint64_t seed, uint64_t first_block, size_t nblocks, size_t block_bytes,
                     void *d_dst, void *stream);
/* d_totals[0] += sum of sizes (a 0 counts as raw_bytes: stored uncompressed); d_totals[1] += #zeros */
int cw_dev_sum_sizes(const uint32_t *d_sizes, size_t nblocks, uint32_t raw_bytes, uint64_t *d_totals,
                     void *stream);

/* ---- dedupe index: a device-resident fingerprint index next to the fingerprint engine ------------
 * The reference has no counterpart: HashAndCompress.cpp computes each block's digest and discards it (:257).
 * An index belongs to one hash algorithm and stores FULL digests, each with a 64-bit value.  Open addressing with
 * linear probing over a power of two >= 2 * max_entries slots, allocated on the calling thread's device (once, unless
 * cw_dedupe_resize rebuilds it): 20 + digest bytes per slot (Skein-512 84 B, SHA-256 52 B, Skein-256-128 36 B; 16 Mi Skein-512 entries = 2.7 GiB),
 * plus per-call scratch of 20 B per block (and the fused call's gather buffer, n_new * block_bytes).
 * Calls on one index are serialised on the device whatever stream they come on (each waits for the previous call). */
typedef struct cw_dedupe cw_dedupe_t;
cw_dedupe_t *cw_dedupe_create(int hash_alg, size_t max_entries);   /* NULL + cw_last_error() on failure / no device */
void         cw_dedupe_destroy(cw_dedupe_t *x);                    /* waits for the index's last call */
int          cw_dedupe_count(cw_dedupe_t *x, uint64_t *count);    /* entries; synchronises on the index's last call */
/* Lookup-or-insert of nblocks digests (d_digests 8-byte aligned, cw_digest_bytes() each); block i has the value base + i.
 * d_ref[i] = value of the block's first occurrence: the stored value if an earlier call inserted the digest, else base + j
 * for the lowest j of this call with the same digest.  Block i is new iff j == i; d_new_idx[0..n_new) lists the new blocks
 * in ascending order, *d_n_new = n_new, and they are inserted with base + i.  Deterministic: what a sequential loop over the
 * batch gives.  CW_ERR_NOMEM (index unchanged, nothing launched) when count + nblocks > max_entries; CW_ERR_BAD_ARG when
 * nblocks > 2^32 - 256 (indices are u32 on the device) or base + nblocks wraps.  All pointers device memory; queued on `stream`, not synchronised.
 * d_ref[nblocks] u64, d_new_idx[nblocks] u32 (first n_new valid), *d_n_new u64.                                        */
int cw_dev_dedupe(cw_dedupe_t *x, const void *d_digests, size_t nblocks, uint64_t base,
                  uint64_t *d_ref, uint32_t *d_new_idx, uint64_t *d_n_new, void *stream);
/* hash every block (d_digests) -> dedupe -> compress ONLY the new blocks: compressed block new_idx[j] in slot j of
 * d_dst, its size in d_sizes[j] (0 = did not fit, as cw_dev_compress), so cw_dev_pack over (d_dst, d_sizes, n_new) gives
 * the stream of new blocks.  Synchronises the stream once, after the dedupe step (the codecs' launch policy needs the
 * block count on the host); *n_new returns that count.  Duplicates are never compressed.  Hash and codec run one after
 * the other here (cw_dev_hash_and_compress runs them side by side).                                                  */
int cw_dev_hash_dedupe_compress(cw_dedupe_t *x, int comp_alg, const void *d_src, size_t block_bytes,
                                size_t src_stride, size_t nblocks, uint64_t base, void *d_digests,
                                uint64_t *d_ref, uint32_t *d_new_idx, void *d_dst, size_t dst_stride,
                                uint32_t *d_sizes, size_t *n_new, void *stream);

/* ---- the index's lifecycle: read-only lookup, explicit values, export / import, resize ----
 * The cw_dev_* calls below follow cw_dev_dedupe's rules: all pointers device memory, queued on `stream` and not
 * synchronised, serialised with every other call on the index; a wrong device, a NULL pointer, a d_digests that is not
 * 8-byte aligned or n > 2^32 - 256 gives CW_ERR_BAD_ARG with nothing launched; n == 0 is a no-op.                    */
#define CW_DEDUPE_MISS UINT64_MAX
/* Read-only query: d_ref[i] = the stored value of digest i, or CW_DEDUPE_MISS when the index does not hold it;
 * *d_n_found (u64) = the number of hits.  The index is unchanged and nothing is counted against max_entries, so it works
 * on a full index.                                                                                                    */
int cw_dev_dedupe_lookup(cw_dedupe_t *x, const void *d_digests, size_t n, uint64_t *d_ref,
                         uint64_t *d_n_found, void *stream);
/* cw_dev_dedupe with explicit values: block i carries d_values[i] instead of base + i.  A digest that an earlier call
 * inserted keeps its stored value; within the batch the lowest index j with that digest wins, d_ref[i] = the winning
 * value, d_new_idx lists the inserted blocks in ascending order.  Deterministic.  CW_ERR_NOMEM (index unchanged) when
 * count + n > max_entries.  The value UINT64_MAX is reserved: an entry stored with it cannot be told from a miss by
 * cw_dev_dedupe_lookup.                                                                                               */
int cw_dev_dedupe_insert(cw_dedupe_t *x, const void *d_digests, const uint64_t *d_values, size_t n,
                         uint64_t *d_ref, uint32_t *d_new_idx, uint64_t *d_n_new, void *stream);
/* The entries as parallel arrays: d_digests[j] (cw_digest_bytes() each) with d_values[j].  *d_n (u64) = the entry count of
 * the index; exactly min(*d_n, max_out) pairs are written and nothing beyond them, so *d_n > max_out means truncated
 * (max_out == 0 just counts; the arrays may be NULL then).  The order is unspecified, but two exports of an unchanged
 * index give the same bytes.  16-byte stores when d_digests is 16-byte aligned.  Scratch of the index: 12 B per 256
 * slots.                                                                                                              */
int cw_dev_dedupe_export(cw_dedupe_t *x, void *d_digests, uint64_t *d_values, size_t max_out, uint64_t *d_n,
                         void *stream);
/* From values to digests, for the entries of a chunk store's directory that d_live[dir_entries] (u32, cw_dev_store_mark's flags)
 * marks: the export with a filter and an order.  With L = the number of idx < dir_entries with
 * d_live[idx] != 0: the k-th such idx in ascending order gets d_values[k] = dir_base + idx and d_digests[k] = the digest the index
 * stores with that value; when the index holds no entry with that value, d_values[k] = CW_DEDUPE_MISS and d_digests[k] is all zero.
 * d_result[2] (u64) = {L, the number of index entries whose value is flagged}.  Exactly min(L, max_out) slots are written and
 * nothing behind them (max_out == 0 just counts; the arrays may be NULL then).  Index entries whose value lies outside
 * [dir_base, dir_base + dir_entries) are ignored.  Two entries may carry the same flagged value (cw_dev_dedupe_insert allows it):
 * then one of their digests is written, whole, and d_result[1] > L; d_result[1] == L with no CW_DEDUPE_MISS among the values
 * means the index and the flags agree one to one.  The index is unchanged, nothing is counted against max_entries (it works on
 * a full index), and two calls on an unchanged index and d_live give the same bytes unless values repeat.  No load leaves
 * d_live[0..dir_entries).  CW_ERR_BAD_ARG with nothing launched: a NULL pointer, a d_digests, d_values or d_result that is not
 * 8-byte aligned, dir_entries == 0, dir_entries or max_out > 2^32 - 256, a wrong device.  A rank scan over the flags, a fill, one
 * sweep of the table.  Scratch of the index: 12 B per directory entry.                                                          */
int cw_dev_dedupe_export_live(cw_dedupe_t *x, const uint32_t *d_live, uint64_t dir_base, size_t dir_entries,
                              void *d_digests, uint64_t *d_values, size_t max_out, uint64_t *d_result /* [2] */, void *stream);
/* Host forms, synchronous, host buffers: staged through device buffers of the index in pieces of 2^20 pairs.
 * export: *n = the entry count, min(*n, max_out) pairs written.  import: cw_dev_dedupe_insert of the n pairs in order,
 * *n_inserted = how many were new; the whole n is admitted up front, CW_ERR_NOMEM (index unchanged) when
 * count + n > max_entries.  n may exceed 2^32 - 256.                                                                   */
int cw_dedupe_export(cw_dedupe_t *x, void *digests, uint64_t *values, size_t max_out, size_t *n);
int cw_dedupe_import(cw_dedupe_t *x, const void *digests, const uint64_t *values, size_t n, size_t *n_inserted);
/* CW_TESTING: pairs per piece of the two host forms (0 = the default, 2^20; at most 2^32 - 256) */
int cw_dedupe_set_stage_entries(cw_dedupe_t *x, size_t entries);
/* Synchronous: waits for the index's last call, allocates a table for new_max_entries (slots as cw_dedupe_create
 * computes them), rehashes every entry into it on the device and frees the old table; the handle stays the same.  Old and
 * new table are live at once during the call: (20 + digest bytes) x (old slots + new slots).  When the slot count does not
 * change only max_entries does.  CW_ERR_BAD_ARG when new_max_entries is 0, above 2^40 or below the entry count;
 * CW_ERR_NOMEM when the new table cannot be allocated -- the index is then unchanged and usable.  Every lookup answers as
 * before; the order of cw_dev_dedupe_export may differ.  The pattern for a full index: on CW_ERR_NOMEM from an inserting
 * call, resize, then repeat the call.                                                                                 */
int cw_dedupe_resize(cw_dedupe_t *x, size_t new_max_entries);
int cw_dedupe_max_entries(cw_dedupe_t *x, size_t *max_entries);

/* ---- content-defined chunking ---------------------------------------------------------------
 * Cuts a byte stream where its content says, so that an insertion or a deletion moves only the cuts near it and the
 * chunks after it keep their digests (fixed blocks all shift).  Parameters m = min_size, a = normal_size, M = max_size,
 * mask_s, mask_l, gear[256]; 64 <= m <= a <= M <= 2^24, else CW_ERR_BAD_ARG.
 *   H(-1) = 0, H(i) = 2 H(i-1) + gear[b[i]] mod 2^64: the sum over k < 64 of gear[b[i-k]] << k, a function of the 64
 *   bytes ending at i.  Cuts: c_0 = 0; from a cut c < n with r = n - c: r <= m -> the next cut is n; else with
 *   e = c + min(M, r), z = c + min(a, r) the next cut is the smallest x in [c+m, z) with H(x-1) & mask_s == 0, else the
 *   smallest x in [z, e) with H(x-1) & mask_l == 0, else e.
 *   final = 0 (streaming): the chain stops at the first cut c with c + M > n, and c is the number of bytes consumed; pass
 *   b[c..) plus the data that follows to the next call.  Because m >= 64, every test reads only bytes of its own chunk,
 *   so pieces chunked this way give exactly the cuts of one final = 1 call over the whole stream.
 * This is FastCDC's normalized chunking with one deliberate difference: FastCDC restarts its fingerprint at c + m for
 * every chunk, so its first ~64 tests depend on where the chunk starts.  Here H runs over the stream and is never reset,
 * so every position's candidate bits are computed in parallel with no knowledge of the cuts.                          */
typedef struct cw_cdc_params {
    uint32_t min_size, normal_size, max_size, reserved;   /* reserved = 0 */
    uint64_t mask_s, mask_l;
    const uint64_t *gear;                                 /* 256 entries in host memory; NULL = the default table */
} cw_cdc_params;
/* normal a power of two in [256, 2^21]: min = normal / 4, max = normal * 8, mask_s = the top log2(normal) + 2 bits,
 * mask_l = the top log2(normal) - 2 bits, gear = NULL (gear[v] = splitmix64(v), the generator of cw_dev_gen_random).
 * Another normal_size is clamped to [256, 2^21] and rounded down to a power of two.  Host only, needs no device.      */
void cw_cdc_default_params(cw_cdc_params *p, uint32_t normal_size);
/* d_offsets[0..K] = c_0..c_K and *d_nchunks = K (u64), device memory.  max_offsets >= nbytes / min_size + 2, checked on
 * the host, so the device can never overflow.  final = 0: c_K = bytes consumed.  Queued on `stream`, not synchronised.
 * Scratch: a workspace per stream in device memory (freed by cw_shutdown and when the library releases the stream),
 * about nbytes / 4 for the candidate bitmaps plus 16 * nbytes / min_size for the cut lists of the resolve's segments
 * (CW_CDC_SEGMENT bytes each, >= max_size; default 256 KiB rounded up to a multiple of max_size).  d_src may have any
 * alignment; the scan loads the 16-byte-aligned granules that overlap d_src[0..nbytes), and no byte outside that range
 * enters a result.                                                                                                   */
int cw_dev_cdc(const cw_cdc_params *p, const void *d_src, size_t nbytes, int final,
               uint64_t *d_offsets, size_t max_offsets, uint64_t *d_nchunks, void *stream);
/* digest of every chunk [d_offsets[i], d_offsets[i+1]) for i < min(*d_nchunks, max_chunks), each the digest cw_dev_hash
 * gives for that message (Skein-512-512, Skein-256-128, SHA-256), at d_digests + i * cw_digest_bytes(hash_alg).  The count
 * is read on the DEVICE, so cdc -> hash_chunks -> (one synchronise) -> cw_dev_dedupe needs no host round trip in between.
 * Offsets are clamped to [0, src_bytes] and a decreasing pair hashes as empty: only 16-byte-aligned granules that overlap
 * d_src[0..src_bytes) are loaded, and no byte outside it enters a digest.  Digests past the count are not written.
 * max_chunks <= 2^32 - 256.  Scratch: a per-stream workspace of 16 KiB + 4 * max_chunks bytes (the chunk order: chunks
 * are hashed longest first so that the lanes of a wavefront finish together), freed like cw_dev_cdc's.               */
int cw_dev_hash_chunks(int hash_alg, const void *d_src, size_t src_bytes, const uint64_t *d_offsets,
                       const uint64_t *d_nchunks, size_t max_chunks, void *d_digests, void *stream);
/* host buffers, synchronous: chunks (and hashes, unless hash_alg == CW_HASH_NONE) any nbytes through pieces of at most
 * 256 MiB on the device, using the final = 0 contract between pieces; offsets[0..*nchunks] (max_offsets >= nbytes /
 * min_size + 2), digests[*nchunks].  Uses the calling thread's staging buffers and the workspaces of its stream.      */
int cw_cdc_hash(const cw_cdc_params *p, int hash_alg, const void *src, size_t nbytes,
                uint64_t *offsets, size_t max_offsets, size_t *nchunks, void *digests);
/* Many streams in one device buffer, each cut as if alone.  Stream f is d_src[d_ends[f-1] .. d_ends[f]) with
 * d_ends[-1] = 0: d_ends[nstreams] (u64, device memory) is non-decreasing and its last entry is nbytes; equal neighbours are empty
 * streams; nstreams is a host count.  Every stream is complete (an open last stream: cw_dev_cdc_streams_part).
 *   d_offsets[0..K]   the cuts of every non-empty stream as cw_dev_cdc(final = 1) over that stream alone gives them, shifted by the
 *                     stream's start, in order: strictly ascending, d_offsets[0] = 0, d_offsets[K] = nbytes.  An empty stream gives no
 *                     chunk.  *d_nchunks = K <= nbytes / min_size + nstreams (a stream of L bytes has at most L / min_size + 1 chunks).
 *   d_stream_first[0..nstreams]   [f] = the index of stream f's first chunk, for an empty stream that of the next stream's first chunk,
 *                     [nstreams] = K: stream f's chunks are positions [first[f], first[f+1]) and its cuts d_offsets[first[f] ..
 *                     first[f+1]] - d_offsets[first[f]].
 *   *d_result (u64, 8-byte aligned)   the verdict on d_ends, decided on the device before anything else is written: 1 when d_ends
 *                     decreases anywhere or its last entry is not nbytes -- then *d_nchunks = 0, d_offsets[0] = 0, every
 *                     d_stream_first[f] = 0 and nothing else is written -- else 0.
 * Whatever d_ends holds, no load leaves d_ends[0..nstreams) or the 16-byte-aligned granules that overlap d_src[0..nbytes), and no store
 * leaves d_offsets[0..max_offsets), d_stream_first[0..nstreams], the two scalars or the workspace.
 * CW_ERR_BAD_ARG, before anything is launched: what cw_dev_cdc refuses, a NULL pointer (d_src may be NULL when nbytes is 0, d_ends
 * when nstreams is 0), a d_result that is not 8-byte aligned, nstreams > 2^32 - 256, nstreams == 0 with nbytes != 0, and max_offsets <
 * nbytes / min_size + nstreams + 1.  nstreams == 0 (nbytes == 0) gives zero chunks and verdict 0.  With nstreams == 1 the cuts are
 * cw_dev_cdc(final = 1)'s.  Queued on `stream`, not synchronised.
 * Scratch: cw_dev_cdc's workspace, with cut lists that also hold every stream end (a segment's two lists hold nstreams_inside_it more
 * cuts each: 16 * nstreams bytes in all, so a segment full of one-byte streams fits) and 4 bytes per segment: a host function of nbytes,
 * nstreams and CW_CDC_SEGMENT.  A step of the resolve finds its stream's end by a binary search among the ends inside its segment.  */
int cw_dev_cdc_streams(const cw_cdc_params *p, const void *d_src, size_t nbytes, const uint64_t *d_ends, size_t nstreams,
                       uint64_t *d_offsets, size_t max_offsets, uint64_t *d_nchunks,
                       uint64_t *d_stream_first /* [nstreams + 1] */, uint64_t *d_result, void *stream);
/* cw_dev_cdc_streams over a piece of a longer run of streams: the last stream may be open.  final = 1 is
 * cw_dev_cdc_streams exactly: the same outputs byte for byte, the same refusals, the same verdict rule.  final = 0: streams
 * 0 .. nstreams - 2 are complete and chunked to their ends; stream nstreams - 1 = [s, nbytes), s = d_ends[nstreams - 2] (0 when nstreams
 * is 1), is the part seen so far of a stream that goes on, and its cuts are what cw_dev_cdc(final = 0) over d_src[s .. nbytes) alone
 * gives, shifted by s: the chain stops at the first cut c >= s with c + max_size > nbytes.  A cut inside a complete stream is never
 * terminal for that reason.  d_offsets[K] = the bytes consumed, at least s and less than max_size below nbytes; d_stream_first[nstreams]
 * = K; d_stream_first[nstreams - 1] = the index of the open stream's first chunk, K when nothing of it was consumed.  The caller
 * carries d_src[d_offsets[K] .. nbytes) in front of the next piece, whose stream 0 then continues the open stream: every cut is a
 * restart point (cw_dev_cdc's final = 0 contract).  nstreams == 1 gives cw_dev_cdc(final = 0)'s cuts; nbytes == 0 gives K = 0.
 * d_ends' last entry is nbytes in both forms.  The bound K <= nbytes / min_size + nstreams, the verdict on d_ends, the memory-safety
 * sentence, CW_ERR_BAD_ARG and the scratch are those of cw_dev_cdc_streams.  Queued on `stream`, not synchronised.                 */
int cw_dev_cdc_streams_part(const cw_cdc_params *p, const void *d_src, size_t nbytes, const uint64_t *d_ends, size_t nstreams, int final,
                            uint64_t *d_offsets, size_t max_offsets, uint64_t *d_nchunks,
                            uint64_t *d_stream_first /* [nstreams + 1] */, uint64_t *d_result, void *stream);

/* ---- codecs over chunks ----------------------------------------------------------------------
 * The codec calls above take one block size per call; these take an offset list as cw_dev_cdc writes it, every chunk
 * [d_offsets[i], d_offsets[i+1]) with a length of its own, 1 .. 65536 = CW_MAX_BLOCK_BYTES bytes (the range of
 * cw_cdc_default_params(p, 8192) and below).  Formats and parsers are those of cw_dev_compress: LZ4 output is byte for
 * byte LZ4_compress_default(chunk, dst, l, bound(l)) of v1.8.2 (l < 13: literals only), LZF output lzf_compress(chunk, l,
 * dst, l - 1) with size 0 = did not fit.
 *
 * Slots.  Compressed chunk i of input offset o = d_offsets[i] is written at d_dst + cw_chunk_slot_offset(comp_alg, o, i):
 *     LZ4: (o + o / 255 + 32 * i) & ~15          LZF: o
 * a position known before the parse.  floor((o + l) / 255) - floor(o / 255) >= floor(l / 255), so consecutive LZ4 slots
 * of ascending, non-overlapping chunks are at least l + l / 255 + 16 = cw_compress_bound(LZ4, l) apart and 16-byte aligned
 * relative to d_dst; an LZF chunk's output is shorter than l.  cw_chunk_slots_bytes(comp_alg, src_bytes, max_chunks) =
 * cw_chunk_slot_offset(comp_alg, src_bytes, max_chunks) + 16 bytes hold every slot: about 1.004 * src_bytes + 32 *
 * max_chunks.  Both are host functions, need no device, and are normative: callers compute slot positions with them.    */
uint64_t cw_chunk_slot_offset(int comp_alg, uint64_t o, uint64_t i);
size_t   cw_chunk_slots_bytes(int comp_alg, size_t src_bytes, size_t max_chunks);
/* Compresses the chunks of positions j: d_sel == NULL -> position j is chunk i = j, for j < min(*d_nchunks, max_chunks);
 * else chunk i = d_sel[j] for j < min(*d_nsel, max_chunks) (u32 indices and a u64 count: cw_dev_dedupe's d_new_idx and
 * d_n_new; entries are expected to be distinct -- two positions naming one chunk write the same bytes to the same slot).
 * Both counts are read on the DEVICE; nothing synchronises.  The output goes to the CHUNK's slot (above), its size to the
 * POSITION: d_sizes[j].  Out of contract, and given d_sizes[j] = 0 with nothing loaded and nothing stored: a chunk index
 * >= min(*d_nchunks, max_chunks), a length of 0 or above 65536, a decreasing pair, an offset past src_bytes -- also a
 * chunk that only ENDS past src_bytes: it is refused whole, where cw_dev_hash_chunks clamps it and hashes the part inside.  Slots of
 * chunks that are not selected and d_sizes past the count are not touched; only bytes [0, d_sizes[j]) of a slot (LZF
 * that did not fit: [0, l)) are written.  Slots are disjoint when the in-contract chunks ascend without overlap (what
 * cw_dev_cdc writes); for any other list they may overlap and only memory safety holds: no load outside
 * d_src[0..src_bytes), no store outside d_dst[0..dst_bytes), since slot(o, i) + bound(l) <= slot(o + l, i + 1) <=
 * slot(src_bytes, max_chunks).  CW_ERR_BAD_ARG, before anything is launched: dst_bytes < cw_chunk_slots_bytes(comp_alg,
 * src_bytes, max_chunks), max_chunks > 2^32 - 256, an unknown codec, NULL pointers (d_sel may be NULL; d_nsel then too).
 * Scratch, per stream, freed like cw_dev_cdc's: 8 KiB + 4 * max_chunks bytes for the order (chunks are parsed longest
 * first, one chunk per lane) and one hash table per lane, 32 KiB (LZ4) / 256 KiB (LZF) each, for min(max_chunks, one per 4 KiB
 * of src_bytes, 131,072 (LZ4) / 65,536 (LZF)) lanes, rounded up to 64: 8 / 64 bytes of table per source byte of the largest call
 * on the stream, 4 GiB / 16 GiB at most; fewer lanes if that cannot be had (the stream then keeps to that number).          */
int cw_dev_compress_chunks(int comp_alg, const void *d_src, size_t src_bytes,
                           const uint64_t *d_offsets, const uint64_t *d_nchunks, size_t max_chunks,
                           const uint32_t *d_sel, const uint64_t *d_nsel,
                           void *d_dst, size_t dst_bytes, uint32_t *d_sizes, void *stream);
/* cw_dev_pack for those slots, the count read on the device: with n = min(*d_count, max_count), d_packed_offsets[j] = sum
 * of d_sizes[0..j) for j <= n (entry n = the total; entries behind it are not written), and the slot of chunk d_sel[j]
 * (chunk j if d_sel == NULL) is copied to d_packed + d_packed_offsets[j].  d_packed == NULL: the index only.  d_offsets:
 * the chunk offsets the slots were computed from.  max_count <= 2^32 - 256.                                           */
int cw_dev_pack_chunks(int comp_alg, const void *d_slots, const uint64_t *d_offsets,
                       const uint32_t *d_sel, const uint64_t *d_count, size_t max_count,
                       const uint32_t *d_sizes, void *d_packed, uint64_t *d_packed_offsets, void *stream);
/* Position j < min(*d_count, max_count) decodes d_comp[d_comp_offsets[j] .. d_comp_offsets[j+1]) into
 * d_dst[d_raw_offsets[j] .. d_raw_offsets[j+1]).  d_status[j] = 0 iff the input is well formed and yields exactly that
 * many bytes (the rules of cw_dev_decompress; an empty compressed extent gives 1, so an LZF chunk that did not fit does).
 * A raw extent that is longer than 65536, decreasing, or reaches past dst_bytes is skipped with status 1.  No store leaves
 * a position's raw extent, no load its compressed extent; the bytes of a raw extent with status 1 are unspecified, except
 * that a skipped or empty-input position writes nothing.  One chunk per lane; no scratch.                             */
int cw_dev_decompress_chunks(int comp_alg, const void *d_comp, const uint64_t *d_comp_offsets,
                             const uint64_t *d_raw_offsets, const uint64_t *d_count, size_t max_count,
                             void *d_dst, size_t dst_bytes, uint32_t *d_status, void *stream);
/* cw_dev_cdc -> cw_dev_hash_chunks (the index's algorithm) -> ONE synchronise of the stream that reads the chunk count
 * (cw_dev_dedupe needs it on the host) -> cw_dev_dedupe with value base + i for chunk i -> cw_dev_compress_chunks with
 * d_sel = d_new_idx, d_nsel = d_n_new and max_chunks = max_offsets - 1: only the new chunks are compressed, and n_new
 * stays on the device, so cw_dev_pack_chunks(comp_alg, d_dst, d_offsets, d_new_idx, d_n_new, ...) can be queued behind it
 * without another synchronise.  Every output equals what those five calls give.  *nchunks = the chunk count (final = 0:
 * d_offsets[*nchunks] = bytes consumed).  dst_bytes >= cw_chunk_slots_bytes(comp_alg, nbytes, max_offsets - 1).
 * CW_ERR_NOMEM when count + *nchunks > max_entries: offsets and digests are written and *nchunks is returned (cw_dedupe_resize,
 * then call again), nothing is inserted, nothing compressed.  CW_ERR_BAD_ARG, at the same point, when base + *nchunks wraps.
 * Calls on one index are serialised as cw_dev_dedupe's.                                                               */
int cw_dev_cdc_dedupe_compress(cw_dedupe_t *x, const cw_cdc_params *p, int comp_alg,
                               const void *d_src, size_t nbytes, int final, uint64_t base,
                               uint64_t *d_offsets, size_t max_offsets, uint64_t *d_nchunks,
                               void *d_digests, uint64_t *d_ref, uint32_t *d_new_idx, uint64_t *d_n_new,
                               void *d_dst, size_t dst_bytes, uint32_t *d_sizes,
                               size_t *nchunks, void *stream);
/* cw_dev_cdc_dedupe_compress with cw_dev_cdc_streams as its chunker: the arguments of both (no `final`), chunk i of the whole buffer
 * carries value base + i.  max_offsets >= nbytes / min_size + nstreams + 1 and dst_bytes >= cw_chunk_slots_bytes(comp_alg, nbytes,
 * max_offsets - 1).  Its one synchronise brings the chunk count AND the verdict to the host: verdict 1 gives CW_ERR_BAD_ARG with
 * *nchunks = 0, nothing inserted and nothing compressed (*d_result stays 1).  The CW_ERR_NOMEM and wrap rules are those of
 * cw_dev_cdc_dedupe_compress.  cw_dev_store_chunks, cw_dev_pack_chunks, cw_dev_restore_chunks and cw_dev_read_ranges work behind it
 * unchanged (they see only offsets); a recipe per stream is positions [first[f], first[f+1]) of d_ref with the cuts rebased.      */
int cw_dev_cdc_streams_dedupe_compress(cw_dedupe_t *x, const cw_cdc_params *p, int comp_alg,
                                       const void *d_src, size_t nbytes, const uint64_t *d_ends, size_t nstreams, uint64_t base,
                                       uint64_t *d_offsets, size_t max_offsets, uint64_t *d_nchunks,
                                       uint64_t *d_stream_first, uint64_t *d_result,
                                       void *d_digests, uint64_t *d_ref, uint32_t *d_new_idx, uint64_t *d_n_new,
                                       void *d_dst, size_t dst_bytes, uint32_t *d_sizes,
                                       size_t *nchunks, void *stream);
/* cw_dev_cdc_streams_dedupe_compress with cw_dev_cdc_streams_part as its chunker: `final` behind nstreams, everything else as there.
 * final = 0: d_offsets[*nchunks] = the bytes consumed, and only the chunks in front of it are hashed, inserted and compressed.       */
int cw_dev_cdc_streams_part_dedupe_compress(cw_dedupe_t *x, const cw_cdc_params *p, int comp_alg,
                                            const void *d_src, size_t nbytes, const uint64_t *d_ends, size_t nstreams, int final,
                                            uint64_t base, uint64_t *d_offsets, size_t max_offsets, uint64_t *d_nchunks,
                                            uint64_t *d_stream_first, uint64_t *d_result,
                                            void *d_digests, uint64_t *d_ref, uint32_t *d_new_idx, uint64_t *d_n_new,
                                            void *d_dst, size_t dst_bytes, uint32_t *d_sizes,
                                            size_t *nchunks, void *stream);

/* ---- chunk store: keep the new chunks, restore deduplicated streams ---------------------------------
 * The read side of the dedupe path.  The library keeps no state: the CALLER owns three plain device buffers, and all three
 * zeroed are an empty store:
 *     d_store[store_bytes]     the stored bytes, appended without padding
 *     *d_used (u64)            the append cursor: bytes of d_store in use
 *     d_dir[dir_entries]       where each chunk lies, indexed by value - dir_base; value = what the index stores for the chunk
 *                              (base + i), so restoring needs no hash lookup.  16-byte aligned; 16 B per ingested chunk.
 * One store is used from one stream at a time (the calls read and write *d_used and the directory in stream order and do
 * not serialise against other streams); different stores may be used from different streams and threads.              */
typedef struct cw_chunk_loc {   /* 16 bytes; all zero = no such chunk */
    uint64_t pos;               /* first byte in the store */
    uint32_t stored;            /* bytes stored there */
    uint32_t raw;               /* bits 0..16: the chunk's length, 1..65536; bit 31: stored uncompressed; bits 17..30: 0 */
} cw_chunk_loc;
#define CW_CHUNK_RAW 0x80000000u
/* Appends the chunks of one cw_dev_compress_chunks / cw_dev_cdc_dedupe_compress call: comp_alg, d_src, src_bytes, d_offsets,
 * d_nchunks, max_chunks, d_sel / d_nsel (that call's selection: cw_dev_dedupe's d_new_idx / d_n_new; NULL / NULL = every chunk),
 * d_slots (its d_dst) and d_sizes exactly as that call got and left them.  With n = min(*d_nsel, max_chunks) (no selection:
 * min(*d_nchunks, max_chunks)), position j < n, chunk i = d_sel[j], l its length and s = d_sizes[j]:
 *   stored form   0 < s < l: the s compressed bytes of the chunk's slot; otherwise the l bytes of d_src, with CW_CHUNK_RAW set --
 *                 one rule for both codecs: an LZF chunk that did not fit and an LZ4 chunk that grew are kept, and restored by a copy.
 *   placement     position j at *d_used + the stored bytes of the positions before it; d_dir[base + i - dir_base] = {pos, stored,
 *                 l | flag}; then *d_used grows by the total.
 *   out of contract (as cw_dev_compress_chunks defines it: index >= the chunk count, length 0 or above 65536, a decreasing pair,
 *                 an end past src_bytes): stores nothing, gets no entry.
 * All or nothing, decided on the device: d_result[1] = the total either way; d_result[0] = 1 when *d_used + total > store_bytes,
 * else 2 when an in-contract chunk's base + i - dir_base lies outside [0, dir_entries) (or base + i wraps), else 0.  When it is
 * not 0, no store byte, no directory entry and not *d_used change.  Nothing synchronises: the call can be queued directly behind
 * the compressing call.  Two positions naming one chunk store it twice; either entry stays.
 * CW_ERR_BAD_ARG before anything is launched: a NULL pointer (d_sel and d_nsel may be NULL together; d_src when src_bytes is 0;
 * d_store when store_bytes is 0), an unknown codec, max_chunks > 2^32 - 256, dir_entries == 0, a d_dir that is not 16-byte
 * aligned, a d_used or d_result that is not 8-byte aligned.  Scratch, per stream: 72 + 12 * max_chunks bytes.                */
int cw_dev_store_chunks(int comp_alg, const void *d_src, size_t src_bytes, const uint64_t *d_offsets,
                        const uint64_t *d_nchunks, size_t max_chunks, const uint32_t *d_sel, const uint64_t *d_nsel,
                        const void *d_slots, const uint32_t *d_sizes, uint64_t base,
                        void *d_store, size_t store_bytes, uint64_t *d_used,
                        cw_chunk_loc *d_dir, uint64_t dir_base, size_t dir_entries,
                        uint64_t *d_result, void *stream);
/* Rebuilds a stream from its recipe: position j < min(*d_count, max_count) is the chunk of value d_ref[j] (as cw_dev_dedupe
 * wrote it) and goes to d_dst[d_raw_offsets[j] .. d_raw_offsets[j+1]).  d_status[j] =
 *   0  the entry exists, its length is the raw extent's, and the decoder (or the copy) produced exactly that many bytes;
 *   1  the stored bytes are malformed: cw_dev_decompress_chunks' verdict on the same bytes (the extent's bytes are unspecified);
 *   2  refused, nothing loaded from the store and nothing written: d_ref[j] outside [dir_base, dir_base + dir_entries) (so
 *      CW_DEDUPE_MISS), an entry with length 0 or above 65536 or with bits 17..30 set (so an all-zero entry), a length that is
 *      not the raw extent's, stored == 0, a raw entry with stored != length, pos + stored > store_bytes, a raw extent that is
 *      decreasing, longer than 65536 or past dst_bytes.
 * No load leaves d_store[0..store_bytes), d_dir[0..dir_entries) or the recipe, no store position j's raw extent, whatever the
 * store and the directory hold; positions behind the count are not touched.  A chunk named twice is decoded twice.  Compressed
 * entries are decoded one per lane, raw entries copied by the whole wavefront; no scratch.  CW_ERR_BAD_ARG: a NULL pointer
 * (d_dst when dst_bytes is 0 and d_store when store_bytes is 0 may be), an unknown codec, max_count > 2^32 - 256,
 * dir_entries == 0, a d_dir that is not 16-byte aligned.  Not synchronised.                                                 */
int cw_dev_restore_chunks(int comp_alg, const void *d_store, size_t store_bytes, const cw_chunk_loc *d_dir,
                          uint64_t dir_base, size_t dir_entries, const uint64_t *d_ref, const uint64_t *d_raw_offsets,
                          const uint64_t *d_count, size_t max_count, void *d_dst, size_t dst_bytes,
                          uint32_t *d_status, void *stream);
/* Byte ranges of a stream without rebuilding it.  The store, the directory and the recipe are
 * cw_dev_restore_chunks' arguments; n = min(*d_count, max_count) and R = min(*d_nranges, max_ranges) are read on the device, and
 * nothing behind position n of the recipe or entry R of the range arrays is read.  Stream coordinates are d_raw_offsets' own: the
 * stream is [d_raw_offsets[0], d_raw_offsets[n]), and d_raw_offsets[0] need not be 0.  Range k < R is the stream bytes
 * [a, a + len), a = d_range_off[k], len = d_range_len[k]; stream byte x of it goes to d_dst[d_range_dst[k] + (x - a)].  Position j
 * is touched by a range iff its raw extent [d_raw_offsets[j], d_raw_offsets[j+1]) is non-empty and intersects the range.
 * d_status[k] (one u32 per range; no d_status[k] with k >= R is written) =
 *   3  the range is refused, nothing is read from the store and nothing written: len > 0 and a < d_raw_offsets[0], a + len wraps
 *      or exceeds d_raw_offsets[n], n == 0, d_range_dst[k] + len wraps or exceeds dst_bytes.  len == 0 is never refused: it gives
 *      0 and reads and writes nothing, whatever a and d_range_dst[k] are;
 *   otherwise the largest status among the touched positions, each judged exactly as cw_dev_restore_chunks judges it, except
 *      that the destination check is the range's and not the chunk's:
 *   2  d_ref[j] outside [dir_base, dir_base + dir_entries); an entry with length 0, a length above 65536 or bits 17..30 set; a
 *      length that is not the raw extent's; stored == 0; a raw entry with stored != length; pos + stored > store_bytes; a raw
 *      extent that is decreasing or longer than 65536;
 *   1  the stored bytes are malformed: the decoder's verdict on the WHOLE chunk, so a range that ends before the damaged spot of
 *      a chunk still gets 1 -- the verdict is a property of the stored chunk, as everywhere else in this library;
 *   0  every byte of the range's destination extent holds the stream's byte.
 * A range with a status other than 0 leaves the bytes inside its own destination extent unspecified.  Whatever the store, the
 * directory, the recipe and the range arrays hold, no load leaves d_store[0..store_bytes), d_dir[0..dir_entries), the recipe or the
 * range arrays, and no store leaves d_dst[d_range_dst[k] .. + len) of a range k with a status other than 3, or d_status[0..R).
 * Ranges may overlap in the stream and name the same chunks: each is served on its own, a chunk named twice is decoded twice.
 * Ranges whose destination extents overlap are the caller's business.  d_raw_offsets[0..n] is expected to be non-decreasing (what
 * cw_dev_cdc writes); for any other list, which positions a range is taken to touch is unspecified -- every position taken is
 * still checked as above, and the sentence on loads and stores holds unchanged.
 * A compressed chunk that lies wholly inside its range is decoded straight into d_dst, raw entries are copied clipped to the
 * range; the at most two compressed chunks a range covers only in part (its first and its last) are decoded whole into scratch
 * and their covered bytes copied out.  Scratch, per stream and freed like cw_dev_cdc's: 72 + 16 * max_ranges bytes (the first
 * touched position, the piece count and the scanned piece offset of every range) and one 64 KiB decode buffer per edge lane,
 * min(2 * max_ranges, 16384) of them (1 GiB at most; 384 KiB for three ranges); if the device cannot give the buffers the call
 * runs with half the lanes, and so on down to 64, before it fails with CW_ERR_NOMEM.
 * CW_ERR_BAD_ARG before anything is launched: a NULL pointer (d_store when store_bytes is 0 and d_dst when dst_bytes is 0 may be),
 * an unknown codec, max_count or max_ranges > 2^32 - 256, dir_entries == 0, a d_dir that is not 16-byte aligned.
 * max_ranges == 0 is a no-op.  Not synchronised.                                                                              */
int cw_dev_read_ranges(int comp_alg, const void *d_store, size_t store_bytes, const cw_chunk_loc *d_dir,
                       uint64_t dir_base, size_t dir_entries, const uint64_t *d_ref, const uint64_t *d_raw_offsets,
                       const uint64_t *d_count, size_t max_count,
                       const uint64_t *d_range_off, const uint64_t *d_range_len, const uint64_t *d_range_dst,
                       const uint64_t *d_nranges, size_t max_ranges,
                       void *d_dst, size_t dst_bytes, uint32_t *d_status, void *stream);

/* ---- the chunk store from host buffers: pipelined ingest and restore of any size ------------------------
 * The calls above take a buffer that already lies in device memory, next to its slots, in one call.  These take host memory of any
 * size and stream it through the device.  The caller-owned triple of cw_dev_store_chunks as one argument:                         */
typedef struct cw_store {
    void *d_store; size_t store_bytes; uint64_t *d_used;
    cw_chunk_loc *d_dir; uint64_t dir_base; size_t dir_entries;
} cw_store;
typedef struct cw_ingest_stats {   /* of one cw_store_ingest call, over the pieces that went in */
    uint64_t bytes, chunks, new_chunks, stored_bytes, pieces, reserved[3];
} cw_ingest_stats;
/* Chunks, hashes, dedupes and compresses src[0..nbytes) and appends its new chunks to the store.  Synchronous; host pointers except
 * inside *st.  The stream crosses the device in pieces: CW_STORE_PIECE fresh bytes each (default 256 MiB, raised to max_size; taken as
 * given otherwise) in front of which lie the bytes behind the previous piece's last cut, fewer than max_size.  Every piece but the
 * last is chunked with final = 0, the last with final = 1: cw_cdc_hash's contract.  Chunk i of the whole stream has value base + i.
 *   result        Cuts, refs, the store bytes [0, *d_used), the directory and the index are byte for byte what ONE
 *                 cw_dev_cdc_dedupe_compress + cw_dev_store_chunks over the whole stream leaves: the cuts by the final = 0 contract, the
 *                 store because the append places positions in selection order without padding.  refs[*nchunks] and
 *                 offsets[*nchunks + 1] are in stream coordinates; *consumed = offsets[*nchunks].
 *   admission     No piece leaves the index ahead of the store.  A piece's one synchronise brings its chunk count k, the bytes it
 *                 consumes and *d_used to the host, and before anything is inserted the piece is admitted: count + k <= max_entries
 *                 (the index's own check); [base_k, base_k + k) inside [dir_base, dir_base + dir_entries), exactly; and, conservatively,
 *                 *d_used + the bytes consumed <= store_bytes.  A chunk's stored form is never longer than the chunk, so an admitted
 *                 append cannot be refused (if it is: CW_ERR_STATE, a bug).  The price of the conservatism: a nearly full store refuses
 *                 a piece of duplicates that a one-call ingest would have taken.
 *   refusal       CW_ERR_NOMEM: *nchunks and *consumed cover the pieces before the refused one; index, store and directory are exactly
 *                 what ingesting src[0, *consumed) as a whole stream gives, and the recipe so far restores those bytes.  Make room
 *                 (cw_dedupe_resize, or compaction into a larger store) and call again with src + *consumed, nbytes - *consumed,
 *                 base + *nchunks: *consumed is a cut, so the resumed run's cuts are the uninterrupted run's.  Not all or nothing:
 *                 consistent at every piece boundary, and resumable.
 *   CW_ERR_BAD_ARG, before the device is touched: a NULL pointer (src may be NULL when nbytes is 0; stats may be NULL), what
 *                 cw_dev_cdc and the codecs refuse, max_size > CW_MAX_BLOCK_BYTES (a longer chunk stores nothing and could never be
 *                 restored), max_offsets < nbytes / min_size + 2, a d_dir that is not 16-byte or a d_used that is not 8-byte aligned,
 *                 dir_entries == 0, base + nbytes / min_size + 1 wrapping.  nbytes == 0: CW_OK, 0 chunks, offsets[0] = 0.
 * The upload of piece k + 1 runs beside the kernels of piece k.  All kernels go on the calling thread's one stream (the codecs' lane
 * tables are per stream), uploads on its copy stream, into two buffers used alternately; fresh bytes always land at the same offset of
 * a buffer (max_size rounded up to 256) and the carry is copied in front of them, so no upload waits for a count.  Page-locked src
 * (cw_host_alloc / cw_host_register) is read in place, other memory goes through two pinned staging buffers with one memcpy.
 * Scratch of the calling thread's context (grows only, freed with the context), for a piece of P bytes, max_size M, min_size m and
 * c = (M + P) / m + 2: two source buffers of P + M (rounded) bytes, cw_chunk_slots_bytes(P + M, c - 1) of slots, c * (64 + 8 + 8 + 4 + 4)
 * bytes of digests, offsets, refs, new-chunk list and sizes, and 16 bytes per nbytes / m + 2 for the recipe.  At the default piece
 * and cw_cdc_default_params(8192) (m = 2048, M = 65536): 512.1 MiB + 261.1 MiB + 11.0 MiB = 784.2 MiB per calling thread, plus the
 * recipe (8 MiB per GiB of input) and, for pageable src, 512 MiB of pinned staging.  An input shorter than a piece takes buffers of its own size. */
int cw_store_ingest(cw_dedupe_t *x, const cw_cdc_params *p, int comp_alg, const cw_store *st,
                    const void *src, size_t nbytes, uint64_t base,
                    uint64_t *refs, uint64_t *offsets, size_t max_offsets,
                    size_t *nchunks, size_t *consumed, cw_ingest_stats *stats /* may be NULL */);
/* The device step behind a piece's cw_dev_store_chunks that assembles the recipe on the device, for callers that stream
 * device-resident pieces themselves (cw_store_ingest uses it).  Every count is read on the device, nothing synchronises.  With
 * n = min(*d_nchunks, max_chunks) and c = *d_rec_count: d_rec_ref[c + j] = d_ref[j] for j < n, d_rec_off[c + j] = stream_off +
 * d_offsets[j] for j <= n, then *d_rec_count = c + n; d_stats (cw_ingest_stats' layout) accumulates bytes += d_offsets[n] -
 * d_offsets[0], chunks += n, new_chunks += *d_n_new, stored_bytes += d_store_result[1], pieces += 1.  All or nothing, decided on the
 * device: *d_verdict = 1 when d_store_result[0] != 0 (the append was refused), else 2 when c + n + 1 > rec_cap, else 0; when it is
 * not 0, no recipe entry, no count and no statistic changes.  No load leaves d_ref[0..max_chunks) or d_offsets[0..max_chunks], no
 * store d_rec_ref / d_rec_off [0..rec_cap).  CW_ERR_BAD_ARG before anything is launched: a NULL pointer (d_store_result and d_stats
 * may be), a pointer that is not 8-byte aligned, max_chunks > 2^32 - 256.  No scratch.                                              */
int cw_dev_ingest_commit(const uint64_t *d_ref, const uint64_t *d_offsets, const uint64_t *d_nchunks, size_t max_chunks,
                         const uint64_t *d_n_new, const uint64_t *d_store_result /* may be NULL */, uint64_t stream_off,
                         uint64_t *d_rec_ref, uint64_t *d_rec_off, uint64_t *d_rec_count, size_t rec_cap,
                         uint64_t *d_stats /* [8], may be NULL */, uint64_t *d_verdict, void *stream);
/* cw_dev_ingest_commit for a piece of many streams (cw_dev_cdc_streams_part): the same arguments, rules and verdicts, and the
 * recipe's stream index on the device.  d_stream_first is the piece's own (d_stream_first[0..nstreams_piece) is read), first_stream
 * the index, in the whole run, of the piece's stream 0, and skip_first (0 or 1) is 1 when the piece's stream 0 continues a stream
 * whose entry an earlier piece wrote.  With c = *d_rec_count before the call: d_rec_first[first_stream + f] = c + d_stream_first[f]
 * for skip_first <= f < nstreams_piece.  An open stream's entry is written by the piece in which the stream first appears, also when
 * nothing of it was consumed: its first chunk is then the next piece's first.  The caller writes the entry behind the last stream
 * when the run ends.  *d_verdict = 1 and 2 as cw_dev_ingest_commit, else 3 when first_stream + nstreams_piece > first_cap, else 0;
 * when it is not 0 nothing changes.  Every count is read on the device, nothing synchronises, and no load or store leaves the arrays:
 * cw_dev_ingest_commit's, d_stream_first[0..nstreams_piece) and d_rec_first[0..first_cap).  CW_ERR_BAD_ARG before anything is
 * launched: what cw_dev_ingest_commit refuses, a NULL or misaligned d_stream_first or d_rec_first, nstreams_piece > 2^32 - 256, a
 * skip_first other than 0 and 1.  No scratch.                                                                                     */
int cw_dev_ingest_commit_streams(const uint64_t *d_ref, const uint64_t *d_offsets, const uint64_t *d_nchunks, size_t max_chunks,
                                 const uint64_t *d_n_new, const uint64_t *d_store_result /* may be NULL */, uint64_t stream_off,
                                 uint64_t *d_rec_ref, uint64_t *d_rec_off, uint64_t *d_rec_count, size_t rec_cap,
                                 uint64_t *d_stats /* [8], may be NULL */, uint64_t *d_verdict,
                                 const uint64_t *d_stream_first, size_t nstreams_piece, uint64_t first_stream, int skip_first,
                                 uint64_t *d_rec_first, size_t first_cap, void *stream);
/* cw_store_ingest for many host streams of any number and total size: stream f is srcs[f][0..lens[f]), every
 * stream is cut as if alone, and a stream may span pieces.  Synchronous; host pointers except inside *st.
 *   result        Coordinates are those of the concatenation of the spans.  refs, offsets, stream_first, the store bytes [0, *d_used),
 *                 the directory and the index are byte for byte what ONE cw_dev_cdc_streams_dedupe_compress + cw_dev_store_chunks over
 *                 the concatenation leaves, and what a loop of cw_store_ingest over the spans with base advancing leaves.  Chunk i of
 *                 the whole run has value base + i; stream f's recipe is positions [stream_first[f], stream_first[f+1]) with the cuts
 *                 rebased; stream_first[nstreams] = *nchunks.
 *   pieces        The concatenation is cut as cw_store_ingest cuts one stream: CW_STORE_PIECE fresh bytes plus the carry in front.  A
 *                 piece takes every stream end not yet taken that lies at or before its last byte's end, leading empty streams and
 *                 repeated ends included.  When the last taken end is not the piece's end, the piece gets its own length as a further
 *                 end and is chunked with final = 0 (cw_dev_cdc_streams_part), else with final = 1.  The piece's ends go to the device
 *                 rebased to the piece's origin; a pass over lens before the first piece finds the largest stream count of any piece,
 *                 which sizes the per-piece arrays: a piece's max_offsets is (max_size + piece) / min_size + streams_in_piece + 1.
 *   source        The fresh bytes of a piece are read in place when every span that contributes to them is page-locked and the spans
 *                 lie back to back in memory (srcs[f + 1] == srcs[f] + lens[f]); otherwise they are gathered into the two pinned
 *                 staging buffers with one memcpy per span part.
 *   admission     cw_store_ingest's, per piece, before anything is inserted.
 *   refusal       CW_ERR_NOMEM: *nchunks, *consumed and *streams_done cover the pieces that went in; *streams_done = the number of
 *                 streams whose end is at or below *consumed; stream_first[0 .. *streams_done] is valid and stream_first[*streams_done
 *                 + 1] = *nchunks (the stream that was cut, if any, is positions [stream_first[*streams_done], *nchunks)).  Everything
 *                 is what ingesting that prefix gives.  Resume with the spans from *streams_done on, the first shortened by what was
 *                 consumed of it, and base + *nchunks: *consumed is a cut, so the cuts are the uninterrupted run's.
 *   CW_ERR_BAD_ARG, before the device is touched: what cw_store_ingest refuses, a NULL srcs or lens with nstreams != 0, a NULL span
 *                 with a non-zero length, a sum of lens that wraps, nstreams > 2^32 - 256, max_offsets < nbytes / min_size + nstreams
 *                 + 1 (nbytes = the sum of lens).  nstreams == 0: CW_OK with nothing done.  stats->pieces counts pieces.
 * Events and buffers are cw_store_ingest's, except that a piece's ends are copied on the kernel stream in front of its kernels: their
 * rebasing needs the carry, which the previous piece's synchronise brings.  Scratch: cw_store_ingest's with c = (M + P) / m + S + 1
 * for the largest stream count S of a piece, 16 bytes per S for the ends and the piece's stream index, 8 bytes per stream for the
 * recipe's, and 16 bytes per nbytes / m + nstreams + 1 for the recipe.                                                             */
int cw_store_ingest_streams(cw_dedupe_t *x, const cw_cdc_params *p, int comp_alg, const cw_store *st,
                            const void *const *srcs, const uint64_t *lens, size_t nstreams, uint64_t base,
                            uint64_t *refs, uint64_t *offsets, size_t max_offsets, uint64_t *stream_first /* [nstreams + 1] */,
                            size_t *nchunks, uint64_t *consumed, size_t *streams_done, cw_ingest_stats *stats /* may be NULL */);
/* Rebuilds the stream of a recipe into host memory: stream byte x goes to dst[x - offsets[0]].  Synchronous.  The recipe is cut into
 * windows of whole positions whose raw bytes fit a piece (CW_STORE_PIECE, raised to 65536); each window's offsets are rebased and
 * uploaded, cw_dev_restore_chunks writes into one of two device buffers, and a window's download runs beside the next window's
 * kernel.  status[j] (may be NULL) = cw_dev_restore_chunks' status of position j, *n_bad = how many are not 0; the call is CW_OK
 * whatever they are, like cw_decompress_blocks, and the bytes of a position with a status other than 0 are unspecified inside its own
 * extent.  A page-locked dst is written in place.  CW_ERR_BAD_ARG: a NULL pointer, what cw_dev_restore_chunks refuses,
 * dst_bytes < offsets[nchunks] - offsets[0], a decreasing offsets array, a position longer than 65536.                              */
int cw_store_restore(int comp_alg, const cw_store *st, const uint64_t *refs, const uint64_t *offsets, size_t nchunks,
                     void *dst, size_t dst_bytes, uint32_t *status /* [nchunks], may be NULL */, size_t *n_bad);

/* ---- the chunk store edits a stream in place: patch, append, truncate -----------------------------------
 * The device step of an edit: which of the cuts of a re-chunked window lands on a cut of the old stream.  Both counts are read on the
 * device: N = min(*d_new_count, max_new), O = min(*d_old_count, max_old); d_new_offsets[0 .. N] and d_old_offsets[0 .. O] are cuts as
 * cw_dev_cdc writes them, the old ones ascending.  The call finds the smallest t in [1, N] with d_new_offsets[t] >= new_from and
 * d_new_offsets[t] + shift (mod 2^64) == d_old_offsets[s] for some s in [0, O] (the lowest such s), and writes
 * d_result[0 .. 4) = {verdict, t, s, d_new_offsets[t]}: verdict 0 = found, and *d_new_count becomes t; verdict 1 = not found,
 * d_result[1 .. 4) = 0, and *d_new_count stays as it is when keep_all is set and becomes 0 otherwise.  Index 0 of the new cuts never
 * matches.  Every call queued behind this one on `stream` reads its count on the device: cw_dev_hash_chunks, the dedupe and
 * cw_dev_compress_chunks then work on exactly the kept chunks and cw_dev_store_chunks stores exactly their new ones; with none kept each
 * is a no-op, without a host round trip.  No load leaves d_new_offsets[0 .. max_new] or d_old_offsets[0 .. max_old]; nothing else is
 * written.  Scratch, per stream: 64 bytes.  Not synchronised.
 * CW_ERR_BAD_ARG before the device is touched: a NULL pointer, a pointer that is not 8-byte aligned, max_new or max_old > 2^32 - 256,
 * a keep_all other than 0 and 1.                                                                                                    */
int cw_dev_cdc_resync(const uint64_t *d_new_offsets, uint64_t *d_new_count /* in, out */, size_t max_new,
                      const uint64_t *d_old_offsets, const uint64_t *d_old_count, size_t max_old,
                      uint64_t new_from, uint64_t shift, int keep_all, uint64_t *d_result /* [4] */, void *stream);
typedef struct cw_patch_stats {   /* of one cw_store_patch call; the window is the last attempt's */
    uint64_t window_bytes, window_chunks, new_chunks, stored_bytes, attempts, first_position, resume_position, reused_positions;
} cw_patch_stats;
/* Replaces bytes [edit_off, edit_off + remove_bytes) of a stored stream by insert[0 .. insert_bytes) and gives the edited stream's
 * recipe, without restoring or re-ingesting the stream.  Synchronous; host pointers except inside *st.  The old recipe is refs[nchunks]
 * and offsets[nchunks + 1]; coordinates are zero-based: the stream is offsets[nchunks] - offsets[0] bytes long and the new offsets
 * start at 0.  out_refs / out_offsets must not overlap refs / offsets.
 *   result        *out_nchunks, out_refs, out_offsets, the store bytes [0, *d_used), the directory and the index are exactly what
 *                 cw_store_ingest of the whole edited stream with the same base leaves, given that the index still holds every chunk of
 *                 the old recipe: the cuts bit for bit, a new chunk's value base + i for window chunk i.  The store only appends, so
 *                 the OLD recipe stays valid: versions of a stream share their chunks.
 *   rule          With cuts c_0 .. c_K of the old stream, a = edit_off, b = a + remove_bytes, delta = insert_bytes - remove_bytes:
 *                 j = the chunk that holds byte a (the last chunk when a is the stream's end, 0 when K is 0).  The window is the edited
 *                 stream from c_j to W + delta, W = the first old cut >= b + lookahead, or the end; it is chunked with final = (W is
 *                 the end).  The first window cut x_t, t >= 1, at or behind b + delta for which x_t - delta is an old cut c_s ends the
 *                 window's part: the new recipe is old positions [0, j), window chunks [0, t), old positions [s, K) with their cuts
 *                 shifted by delta.  A final window without such a cut is kept whole and no tail follows; any other window without one
 *                 inserts nothing anywhere, the lookahead doubles and the attempt is repeated.  lookahead 0 = 4 * max_size; a smaller
 *                 value is raised to 2 * max_size.
 *   attempt       Only positions [j, e] of the old recipe (c_e = W) are uploaded; their bytes [c_j, a) and [b, W) are rebuilt on the
 *                 device around the uploaded insert (cw_dev_read_ranges); then cw_dev_cdc, cw_dev_cdc_resync, the hash, ONE synchronise
 *                 (the kept count, the resync result, the store cursor and the read statuses), admission, the dedupe of the kept chunks,
 *                 the codec over the new ones and cw_dev_store_chunks: cw_store_ingest's piece with the resync behind the chunker.
 *   all or nothing  Nothing is inserted into index, directory or store before the window's old bytes were all read with status 0, a
 *                 resync was found or the window was final, and the kept chunks were admitted exactly as a piece of cw_store_ingest
 *                 is (index room for t, the directory for [base, base + t), the store conservatively against the kept bytes).
 *                 CW_ERR_NOMEM (not admitted, or the window and its lists do not fit on the device: fall back to restore + ingest)
 *                 and CW_ERR_BAD_ARG naming the first position that did not restore and its status (found by restoring the window's
 *                 positions once more, whole; when that restore cannot get its buffers the message gives the window's positions and
 *                 the two read statuses and says so) both leave index, store, directory and the old recipe as they were.
 *   CW_ERR_BAD_ARG, before the device is touched: what cw_store_ingest refuses (max_size > CW_MAX_BLOCK_BYTES included), edit_off +
 *                 remove_bytes wrapping or beyond the stream, a NULL insert with insert_bytes != 0, max_out < (stream bytes -
 *                 remove_bytes + insert_bytes) / min_size + 2, offsets that decrease in the located window.
 * The window and its lists live in the calling thread's context scratch (grows only): a stream that never resynchronises (all zero, or
 * periodic) grows the window by doubling until it reaches the end of the stream.                                                     */
int cw_store_patch(cw_dedupe_t *x, const cw_cdc_params *p, int comp_alg, const cw_store *st,
                   const uint64_t *refs, const uint64_t *offsets, size_t nchunks,
                   uint64_t edit_off, uint64_t remove_bytes, const void *insert, size_t insert_bytes,
                   uint64_t base, size_t lookahead /* 0 = default */,
                   uint64_t *out_refs, uint64_t *out_offsets, size_t max_out, size_t *out_nchunks,
                   cw_patch_stats *stats /* may be NULL */);

/* ---- the store forgets: mark, compact, and the index's retain ----------------------------------------
 * Mark and sweep over the same caller-owned buffers, plus one more the caller owns: d_live[dir_entries] (u32), a flag per
 * directory entry.  To drop streams: zero d_live and *d_n_outside, mark every recipe that stays, compact, retain.  Marking is
 * idempotent and needs no atomics on the flags; no call keeps state, every decision is made on the device, every call is all or
 * nothing.  Values are not renumbered: a dropped chunk's directory entry stays zero (16 B), and base keeps counting upward.   */
/* With n = min(*d_count, max_count), read on the device: for each position j < n, idx = d_ref[j] - dir_base in u64 (a value
 * below the base wraps out of range); idx < dir_entries sets d_live[idx] = 1 (a plain store), any other position -- CW_DEDUPE_MISS
 * always -- is counted: *d_n_outside (u64) += their number, so several marks accumulate.  Positions behind n are not read.
 * CW_ERR_BAD_ARG before anything is launched: a NULL pointer, max_count > 2^32 - 256, dir_entries == 0, a d_n_outside that is
 * not 8-byte aligned.  No scratch.  Not synchronised.                                                                         */
int cw_dev_store_mark(const uint64_t *d_ref, const uint64_t *d_count, size_t max_count,
                      uint64_t dir_base, size_t dir_entries, uint32_t *d_live,
                      uint64_t *d_n_outside, void *stream);
/* Moves the kept entries' stored bytes into a new store.  No codec: extents move as they are.
 *   kept          entry idx is kept iff d_live[idx] != 0 and the entry is not all zero (a flag on an all-zero entry -- what a
 *                 failed append leaves -- keeps nothing).  A kept entry must be sound by cw_dev_restore_chunks' entry checks:
 *                 length 1..65536, bits 17..30 zero, stored != 0, a raw entry has stored == length, pos + stored <= store_bytes.
 *   placement     kept entries back to back from byte 0 of d_new_store in ascending idx, without padding;
 *                 d_new_dir[idx] = {new pos, stored, raw}, every other entry of d_new_dir all zero; *d_new_used = the total.
 *   d_result[4]   {verdict, the kept entries' stored bytes summed, the kept count, the count of non-zero entries not kept}; the
 *                 last three are written whatever the verdict is.
 *   verdict       2 when a kept entry is unsound, else 1 when the total > new_store_bytes, else 0.  When it is not 0, no byte of
 *                 d_new_store, no entry of d_new_dir and not *d_new_used change: new_store_bytes == 0 with d_new_store == NULL is
 *                 a dry run, and d_result[1] says how much room to provide.  An unsound entry that is not kept is dropped like
 *                 any other.
 * d_new_dir may be d_dir itself (the directory is compacted in place; the old store's bytes stay, only the directory forgets) or
 * must not overlap it.  The old store and its directory are never written unless d_new_dir == d_dir.  No load leaves
 * d_store[0..store_bytes), d_dir[0..dir_entries) or d_live[0..dir_entries) whatever they hold; no store leaves the new buffers.
 * CW_ERR_BAD_ARG before anything is launched: a NULL pointer (d_store when store_bytes is 0 and d_new_store when new_store_bytes
 * is 0 may be), dir_entries == 0, a directory that is not 16-byte aligned, a d_new_used or d_result that is not 8-byte aligned,
 * [d_new_store, +new_store_bytes) overlapping [d_store, +store_bytes), a d_new_dir that overlaps d_dir without being equal to it.
 * Scratch, per stream: 72 + 12 * dir_entries bytes.  Not synchronised.                                                        */
int cw_dev_store_compact(const void *d_store, size_t store_bytes, const cw_chunk_loc *d_dir, size_t dir_entries,
                         const uint32_t *d_live,
                         void *d_new_store, size_t new_store_bytes, uint64_t *d_new_used, cw_chunk_loc *d_new_dir,
                         uint64_t *d_result /* [4] */, void *stream);
/* The index's side, synchronous like cw_dedupe_resize: waits for the index's last call, always allocates and clears a fresh table
 * for new_max_entries (0 = as it is), and rehashes on the device every entry whose value v it keeps: v - dir_base >= dir_entries
 * (in u64: the value belongs to no entry of this directory) or d_live[v - dir_base] != 0.  The other entries are gone; a digest
 * that was dropped can be inserted again.  d_live (device memory) must be complete when the call is made: synchronise the stream
 * that marked.  *n_removed (may be NULL) = the old count - the kept count.  A rebuild, so the table is what inserting the kept
 * entries into an empty index gives: slots only ever fill within a table's life.  CW_ERR_BAD_ARG: a NULL d_live,
 * dir_entries == 0, new_max_entries above 2^40, or -- found out on the device, the index unchanged -- below the kept count;
 * CW_ERR_NOMEM (index unchanged) when the new table cannot be allocated.  Old and new table are live at once during the call. */
int cw_dedupe_retain(cw_dedupe_t *x, const uint32_t *d_live, uint64_t dir_base, size_t dir_entries,
                     size_t new_max_entries /* 0 = as it is */, uint64_t *n_removed);

/* ---- the directory gives slots back: renumber, and the index's revalue ---------------------------------
 * Compaction leaves a dropped chunk's directory entry zero and base counting upward; a duplicate chunk takes a value and no entry.
 * Renumbering moves the kept entries to the dense values [new_base, new_base + K) of a new directory, which can be as small as K
 * plus headroom.  Three things name a value and change together: the directory (cw_dev_store_renumber), every kept recipe
 * (cw_dev_translate_refs with the pairs that call wrote) and the index (cw_dev_dedupe_revalue with the same pairs).  Both calls
 * follow the store's conventions: device pointers, queued on `stream`, nothing synchronises, every decision made on the device,
 * all or nothing.                                                                                                                */
/* Moves directory entries to dense values.  No stored byte moves and no entry is judged: an unsound entry moves as it is.
 *   kept          entry idx is kept iff it is not all zero and (d_live == NULL or d_live[idx] != 0): cw_dev_store_compact's rule,
 *                 with cw_dev_store_verify's "d_live == NULL selects every non-zero entry".  K = the kept entries, r(idx) = the
 *                 kept entries below idx.
 *   placement     for a kept idx with k = r(idx): d_from[k] = dir_base + idx and d_to[k] = new_base + k, both strictly ascending
 *                 (the pairs cw_dev_translate_refs and cw_dev_dedupe_revalue take), and d_new_dir[new_base + k - new_dir_base] =
 *                 d_dir[idx] bit for bit.  Every other entry of d_new_dir[0..new_dir_entries) is written all zero.
 *   d_result[4]   {verdict, K, new_base + K (the next base), the count of non-zero entries not kept}; the last three are written
 *                 whatever the verdict is.
 *   verdict       2 when new_base + K wraps or [new_base, new_base + K) is not inside [new_dir_base, new_dir_base +
 *                 new_dir_entries) (with K == 0 the range is empty and inside); else 1 when K > max_pairs; else 0.  When it is
 *                 not 0, no byte of d_new_dir, d_from and d_to changes: max_pairs == 0 with d_from == d_to == NULL and
 *                 new_dir_entries == 0 with d_new_dir == NULL is a dry run, and d_result[1] says how much room to provide.
 * d_dir is never written; there is no in-place form.  No load leaves d_dir[0..dir_entries) or d_live[0..dir_entries) whatever
 * they hold; no store leaves d_new_dir[0..new_dir_entries), d_from / d_to[0..max_pairs), d_result and the scratch.
 * CW_ERR_BAD_ARG before anything is launched: a NULL pointer (d_live may be NULL; d_new_dir when new_dir_entries is 0 and d_from,
 * d_to when max_pairs is 0 may be), dir_entries == 0, a dir_entries, new_dir_entries or max_pairs above 2^32 - 256, a directory
 * that is not 16-byte aligned, a d_from, d_to or d_result that is not 8-byte aligned, d_new_dir[0..new_dir_entries) overlapping
 * d_dir[0..dir_entries), new_dir_base + new_dir_entries wrapping.  Scratch, per stream: 72 + 12 * dir_entries bytes.
 * Not synchronised.                                                                                                             */
int cw_dev_store_renumber(const cw_chunk_loc *d_dir, uint64_t dir_base, size_t dir_entries,
                          const uint32_t *d_live /* may be NULL */, uint64_t new_base,
                          cw_chunk_loc *d_new_dir, uint64_t new_dir_base, size_t new_dir_entries,
                          uint64_t *d_from, uint64_t *d_to, size_t max_pairs,
                          uint64_t *d_result /* [4] */, void *stream);
/* Does to the index what cw_dev_translate_refs does to a recipe, in place: the table keeps its values apart from its keys, so a
 * value changes without a rehash.  The count, the keys, the slot states and max_entries do not change, and a full index is fine.
 * Serialised with the index's other calls.  p = min(*d_npairs, max_pairs), read on the device; d_from[0..p) is ascending (for any
 * other list, which pair a value hits is unspecified and only memory safety holds).  For every entry with value v: a binary-search
 * hit d_from[k] == v is a translation to d_to[k]; otherwise, when v - range_base < range_entries (in u64), the entry is STALE -- it
 * carries a value of the range that no pair names and would collide with renumbered values later; any other entry is left alone
 * (values outside the range belong to other directories).  d_result[3] = {verdict, entries translated, stale entries}: verdict 1
 * when an entry is stale, and then no value changes; else 0, and every translation is applied.  range_entries == 0: nothing is
 * stale.  p == 0: counts only.  Two entries that carry one value are both translated.  Every slot is read once and written at most
 * once, so the old and the new values may overlap (dense values [dir_base, dir_base + K) out of [dir_base, dir_base +
 * dir_entries)).  No load leaves d_from / d_to[0..p) or the table.  CW_ERR_BAD_ARG before anything is launched: a NULL pointer, a
 * pointer that is not 8-byte aligned, max_pairs > 2^32 - 256, range_base + range_entries wrapping, an index of another device.
 * Scratch: 64 bytes of the index.  Not synchronised.                                                                            */
int cw_dev_dedupe_revalue(cw_dedupe_t *x, const uint64_t *d_from, const uint64_t *d_to, const uint64_t *d_npairs, size_t max_pairs,
                          uint64_t range_base, uint64_t range_entries, uint64_t *d_result /* [3] */, void *stream);

/* ---- per-stream accounting and reverse references ------------------------------------------------------
 * "What does dropping this stream give back?" and "which streams do these damaged chunks hurt?" are one computation: reverse
 * references from directory entries to the streams that name them.  The store keeps no reference counts (section 15: mark and
 * sweep); these are computed on demand from the recipes the caller passes, exact for that set, and nothing is kept between calls.
 * The call follows the store's conventions: device pointers, counts read on the device, queued on `stream`, nothing synchronises,
 * every decision made on the device.  Everything summed is an integer, so the result is bit for bit a function of the arguments. */
typedef struct cw_stream_account {   /* 64 bytes, one per stream of the call */
    uint64_t positions;          /* positions of the stream: d_first[f+1] - d_first[f] */
    uint64_t missing;            /* positions that name no stored chunk: d_ref - dir_base outside [0, dir_entries) in u64
                                    (so CW_DEDUPE_MISS and values below the base), or an all-zero entry */
    uint64_t logical_bytes;      /* the entry's length (bits 0..16 of raw) summed over the other positions */
    uint64_t unique_chunks;      /* entries this stream names and no other stream of the call does */
    uint64_t unique_stored;      /* their `stored` summed: what dropping this stream alone lets compact give back */
    uint64_t unique_raw;         /* their lengths summed, each entry once */
    uint64_t flagged_positions;  /* non-missing positions whose entry idx has d_flag[idx] != 0; 0 when d_flag == NULL */
    uint64_t flagged_bytes;      /* those positions' lengths summed: the stream bytes that sit in flagged chunks */
} cw_stream_account;
#define CW_OWNER_NONE   0xFFFFFFFFu   /* no position names the entry (every all-zero entry) */
#define CW_OWNER_SHARED 0xFFFFFFFEu   /* positions of at least two different streams name it */
/* Accounts the streams of one call against a directory.
 *   streams       d_ref is the concatenation of the recipes' refs, d_first[nstreams + 1] the index of each stream's first position
 *                 (what cw_dev_ingest_commit_streams and cw_dev_cdc_streams write): stream f is positions [d_first[f],
 *                 d_first[f+1]), equal neighbours are an empty stream, and n = d_first[nstreams] is read on the device.
 *   verdict       d_totals[0], decided on the device before anything else is written: 1 when d_first[0] != 0, when a pair
 *                 decreases or when n > max_positions, and then not a byte of d_acct, d_refcount, d_owner or d_totals[1..7]
 *                 changes; else 0.
 *   rules         no entry is judged (cw_dev_store_renumber's rule: a non-zero entry counts with its fields as they are).  A
 *                 position that names an all-zero entry is missing and enters no count of that entry.  d_refcount[idx] = the
 *                 non-missing positions of all streams that name idx; d_owner[idx] = the one stream that names idx, or
 *                 CW_OWNER_NONE / CW_OWNER_SHARED.  d_flag has the shape of d_live and of cw_store_scrub's status: one u32 per
 *                 entry, any non-zero value is a flag.
 *   d_totals[8]   {verdict, the non-zero entries, their stored summed, the referenced entries, their stored summed, the shared
 *                 entries, their stored summed, the missing positions of all streams}.  [1] - [3] entries are unreferenced: what
 *                 a compact that keeps these recipes drops.  Every output is written whole, not accumulated.
 * A stream's count of distinct entries among the shared ones is not computed; a call over that stream alone gives it as
 * unique_chunks.  Whatever the buffers hold, no load leaves d_ref[0..min(n, max_positions)), d_first[0..nstreams],
 * d_dir[0..dir_entries) or d_flag[0..dir_entries), and no store leaves the outputs and the scratch.  CW_ERR_BAD_ARG before anything
 * is launched: a NULL pointer (d_flag, d_refcount and d_owner may be NULL; d_ref may be when max_positions is 0), nstreams == 0 or
 * > 2^32 - 258 (the two sentinels), max_positions > 2^32 - 256, dir_entries == 0 or > 2^32 - 256, a directory that is not 16-byte
 * aligned, a d_ref, d_first, d_acct or d_totals that is not 8-byte aligned.  Scratch, per stream: at most 72 + 12 * dir_entries
 * bytes.  Not synchronised.                                                                                                       */
int cw_dev_store_account(const uint64_t *d_ref, const uint64_t *d_first, size_t nstreams, size_t max_positions,
                         const cw_chunk_loc *d_dir, uint64_t dir_base, size_t dir_entries,
                         const uint32_t *d_flag /* may be NULL */,
                         cw_stream_account *d_acct /* [nstreams] */,
                         uint32_t *d_refcount /* [dir_entries], may be NULL */, uint32_t *d_owner /* [dir_entries], may be NULL */,
                         uint64_t *d_totals /* [8] */, void *stream);

/* ---- what changed between two recipes, and a version shipped as a delta ---------------------------------
 * A patched stream and its parent share every chunk but the few around the edit.  Equal refs mean equal bytes, so what changed
 * between two recipes is decided from the recipes alone, and handing version B to someone who holds version A as plain bytes takes
 * only the bytes of the chunks that are new.  A delta is a list of ops that tile B back to back, each either a copy out of A or a
 * run of new bytes out of a payload, and the payload.  Both calls follow the store's conventions: device pointers, counts read on
 * the device, queued on `stream`, nothing synchronises, every decision made on the device and all or nothing.                     */
#define CW_DELTA_NONE UINT64_MAX
typedef struct cw_delta_op {   /* 32 bytes; offsets are zero-based (x - off[0] on each side) */
    uint64_t b_off;              /* where the op starts in B; the ops tile B back to back from 0 */
    uint64_t len;                /* its bytes, at least 1 */
    uint64_t a_off;              /* a copy: where its bytes lie in A; a new op: CW_DELTA_NONE */
    uint64_t payload_off;        /* a new op: where its bytes lie in the payload; a copy: CW_DELTA_NONE */
} cw_delta_op;
/* The ops that turn stream A into stream B, from their recipes alone.
 *   recipes       A is d_ref_a[0..na), d_off_a[0..na] with na = min(*d_na, max_a), B likewise: what the ingests, cw_store_patch and
 *                 cw_dev_translate_refs write, in any coordinates (cw_dev_restore_chunks' d_raw_offsets).  dir_base and dir_entries
 *                 are the value range of the directory: they bound a per-entry table, the directory itself is not read.
 *   verdict       d_totals[0], decided on the device before anything else is written: 1 unless both offset lists ascend strictly in
 *                 extents of 1..65536 bytes (what the library writes), and then no other byte of any output changes.
 *   source        of B position i, in zero-based offsets.  IN PLACE: an A position starts at the same offset with the same ref and
 *                 the same length; the source is that offset.  Else MOVED: the lowest A position that names the same ref, if its
 *                 length is that of i; the source is its offset.  Else NEW: CW_DELTA_NONE.  A ref outside [dir_base, dir_base +
 *                 dir_entries), CW_DEDUPE_MISS among them, names no chunk: such a position of A is no source and such a position of
 *                 B is new.  d_src[i] (optional) = the source of i < nb.
 *   ops           position i starts an op unless it continues the one before: both are new, or both are copies and source(i) ==
 *                 source(i-1) + length(i-1).  The new ops' bytes are numbered back to back in op order: payload_off.  d_ops[0..ops)
 *                 and *d_nops = ops.  More ops than max_ops: verdict 2, *d_nops = *d_nnew = 0, no op and no range is written, the
 *                 totals are complete -- max_ops == 0 (d_ops may then be NULL) is the dry run that sizes the buffers.
 *   ranges        optional, all four or none: the new ops as d_new_off / d_new_len / d_new_dst [0..*d_nnew) (room for max_ops each),
 *                 offsets in B's own coordinates and destinations equal to payload_off, so cw_dev_read_ranges over recipe B queues
 *                 directly behind this call and its d_dst is the payload.
 *   d_totals[8]   {verdict, ops, new ops, in-place bytes, moved bytes, new bytes, matched positions, nb}.
 * Everything is an integer and the table is built with atomicMin, which does not depend on order: every output is bit for bit a
 * function of the arguments.  A run of one repeated chunk that shifts costs one op per chunk (the lowest position wins); in place
 * it is one op.  Whatever the buffers hold, no load leaves d_ref_x[0..max_x), d_off_x[0..max_x] or the scratch, and no store leaves
 * the outputs and the scratch.  CW_ERR_BAD_ARG before anything is launched: a NULL pointer (d_src may be NULL, the four range
 * pointers may be together, d_ops may be when max_ops is 0), a pointer that is not 8-byte aligned, max_a, max_b or dir_entries
 * above 2^32 - 256, dir_entries == 0.  Scratch, per stream: at most 96 + 4 * dir_entries + 44 * max_b bytes.  Not synchronised.  */
int cw_dev_recipe_diff(const uint64_t *d_ref_a, const uint64_t *d_off_a, const uint64_t *d_na, size_t max_a,
                       const uint64_t *d_ref_b, const uint64_t *d_off_b, const uint64_t *d_nb, size_t max_b,
                       uint64_t dir_base, size_t dir_entries,
                       cw_delta_op *d_ops /* [max_ops] */, size_t max_ops, uint64_t *d_nops,
                       uint64_t *d_src /* [max_b], may be NULL */,
                       uint64_t *d_new_off, uint64_t *d_new_len, uint64_t *d_new_dst /* [max_ops] each */, uint64_t *d_nnew /* may be NULL together */,
                       uint64_t *d_totals /* [8] */, void *stream);
/* Rebuilds B's bytes from A's plain bytes d_old[0..old_bytes), a payload and n = min(*d_nops, max_ops) ops.  A delta may come from
 * a file, so nothing of the list is trusted.  d_result[4] = {verdict, total, the lowest bad op or CW_DELTA_NONE, n}.  Verdict 1, a
 * malformed list (total is then 0): an op that does not start where the one before ends (op 0: at 0), has len 0 or an end that
 * wraps, has both or neither of a_off and payload_off equal to CW_DELTA_NONE, or has a_off + len > old_bytes or payload_off + len >
 * payload_bytes.  Else verdict 2 when total = the end of the last op > dst_bytes.  Else 0, and d_dst[0..total) is B.  With a verdict
 * other than 0 not a byte of d_dst changes.  Whatever the ops hold, no load leaves d_old, d_payload or d_ops[0..n) and no store
 * leaves d_dst[0..total) and d_result.  The copy is tiled by output (CW_DELTA_TILE KiB per wavefront), so an op of one byte and one
 * of gigabytes cost what their bytes cost.  CW_ERR_BAD_ARG before anything is launched: a NULL pointer (d_old, d_payload, d_dst and
 * d_ops may be when their size is 0), a d_ops, d_nops or d_result that is not 8-byte aligned, max_ops > 2^32 - 256, [d_dst,
 * +dst_bytes) overlapping [d_old, +old_bytes) or [d_payload, +payload_bytes).  No scratch.  Not synchronised.                     */
int cw_dev_apply_delta(const void *d_old, size_t old_bytes, const void *d_payload, size_t payload_bytes,
                       const cw_delta_op *d_ops, const uint64_t *d_nops, size_t max_ops,
                       void *d_dst, size_t dst_bytes, uint64_t *d_result /* [4] */, void *stream);

/* ---- compose a stored stream from stored ranges and new bytes --------------------------------------------
 * cw_dev_cdc_resync for many windows chunked by one cw_dev_cdc_streams call.  N = min(*d_new_count, max_new) is read on the device;
 * window w's cuts are d_new_offsets[first[w] .. first[w+1]], first = d_stream_first[0 .. nwin].  For every window the call finds the
 * smallest t >= 1 whose cut x = d_new_offsets[first[w] + t] has x >= new_from and x + shift (mod 2^64) equal to one of the old cuts
 * d_old_offsets[old_first .. old_first + old_count) (ascending; the range is clamped into [0, max_old)).  The window's last cut, which
 * the window's end forced, is not tested unless `final` is set.  d_result[4 * w ..] = {0, t, s, x} with s the index of the old cut in
 * d_old_offsets, or {1, 0, 0, 0}.  A cut never matches through another window's old range.  No count changes and nothing else is
 * written; no load leaves d_new_offsets[0 .. max_new], d_stream_first[0 .. nwin], d_win[0 .. nwin) or d_old_offsets[0 .. max_old),
 * whatever they hold.  nwin == 0 is a no-op.  Scratch, per stream: 64 + 8 * nwin bytes.  Not synchronised.
 * CW_ERR_BAD_ARG before the device is touched: a NULL pointer (d_old_offsets may be NULL when max_old is 0), a pointer that is not
 * 8-byte aligned, max_new, max_old or nwin > 2^32 - 256.                                                                            */
typedef struct cw_resync_window {   /* 40 bytes */
    uint64_t new_from, shift, old_first, old_count, final;
} cw_resync_window;
int cw_dev_cdc_resync_windows(const uint64_t *d_new_offsets, const uint64_t *d_new_count, size_t max_new,
                              const uint64_t *d_stream_first /* [nwin + 1] */, const cw_resync_window *d_win, size_t nwin,
                              const uint64_t *d_old_offsets, size_t max_old, uint64_t *d_result /* [4 * nwin] */, void *stream);
/* Copies n = min(*d_n, max_n) extents from d_src to d_dst; extent k is the three words d_ext[3 * k ..] = {src_off, dst_off, len}.
 * Nothing of the list is trusted.  d_result[4] = {verdict, the end of the last extent in d_dst, the lowest bad extent or CW_DELTA_NONE,
 * n}.  Verdict 1 (the end is then 0): an extent with len 0, one that leaves d_src[0 .. src_bytes) or d_dst[0 .. dst_bytes) or wraps,
 * or one whose dst_off lies in front of the end of the extent before it (the destinations ascend without overlap); then not a byte of
 * d_dst changes.  The copy is tiled by the bytes of d_dst (16 KiB per wavefront), so an extent of one byte and one of gigabytes cost
 * what their bytes cost.  Whatever the list holds, no load leaves d_src or d_ext[0 .. 3 * max_n) and no store leaves the extents'
 * destinations and d_result.  CW_ERR_BAD_ARG before anything is launched: a NULL pointer (d_src, d_dst and d_ext may be when their
 * size is 0), a d_ext, d_n or d_result that is not 8-byte aligned, max_n > 2^32 - 256, d_dst overlapping d_src.  No scratch.  Not
 * synchronised.                                                                                                                     */
int cw_dev_scatter_extents(const void *d_src, size_t src_bytes, const uint64_t *d_ext /* [3 * max_n] */, const uint64_t *d_n, size_t max_n,
                           void *d_dst, size_t dst_bytes, uint64_t *d_result /* [4] */, void *stream);
typedef struct cw_compose_stats {   /* of one cw_store_compose call */
    uint64_t windows, rounds, merged_windows, rebuilt_bytes, rebuilt_chunks, new_chunks, stored_bytes, kept_positions;
} cw_compose_stats;
/* Builds a new stored stream B from ranges of streams the store already holds and new bytes, without restoring or re-ingesting
 * anything.  Synchronous; host pointers except inside *st.
 *   source        A is the recipe refs[nchunks], offsets[nchunks + 1] (zero-based: A is offsets[nchunks] - offsets[0] bytes).  With
 *                 stream_first[nstreams + 1] (as cw_dev_store_account takes it) A is the concatenation of nstreams stored streams,
 *                 stream f being positions [stream_first[f], stream_first[f + 1]); NULL means one stream.
 *   ops           ops[nops] tile B from 0 as cw_dev_apply_delta's do: each a copy of A's bytes [a_off, a_off + len) or len new bytes
 *                 at payload_off of payload[0 .. payload_bytes).
 *   result        *out_nchunks, out_refs, out_offsets, the store bytes, the directory and the index are what cw_store_ingest of B's
 *                 bytes leaves, given that the index still holds every chunk of A: the cuts bit for bit.  A chunk of B is KEPT -- it
 *                 takes A's ref and is not read, hashed or stored -- exactly when a copy holds it whole as position s of A, it starts
 *                 at or behind the copy's start in B, and s is not the last position of its stream (whose end the stream's end
 *                 forced) unless it ends B as well; adjacent copies that continue each other count as one, and a copy is split at
 *                 the stream ends of A inside it.  Every other chunk is REBUILT: read back or taken from the payload, hashed,
 *                 deduplicated, compressed and appended, rebuilt chunk i of the call in B order with value base + i.  The caller
 *                 advances base by stats->rebuilt_chunks.  The store only appends, so A stays valid.
 *   procedure     A copy with kept candidates is an anchor.  Between two anchors lies a window: it starts where the candidates of
 *                 the anchor before end and reaches lookahead bytes (0 = 4 * max_size, at least 2 * max_size) into its own anchor.
 *                 A round materialises all unresolved windows on the device (cw_dev_read_ranges, cw_dev_scatter_extents), chunks
 *                 them in one cw_dev_cdc_streams call and looks for each window's landing (cw_dev_cdc_resync_windows): one
 *                 synchronise.  A window without a landing doubles its lookahead; one that has covered its whole anchor drops the
 *                 anchor and merges into the next window, once every window in front of it is resolved.  Behind the last anchor a
 *                 final window runs to B's end.  Then ONE commit: the rebuilt extents of all windows through
 *                 cw_dev_cdc_streams_dedupe_compress and cw_dev_store_chunks.
 *   all or nothing  Nothing is inserted into index, directory or store before every range was read with status 0, each extent chunked
 *                 into exactly the chunks its round found (else CW_ERR_STATE), and the rebuilt chunks were admitted exactly as a piece
 *                 of cw_store_ingest is.  CW_ERR_NOMEM (not admitted, or the windows do not fit on the device) and CW_ERR_BAD_ARG (a
 *                 range that does not restore) leave index, store, directory and A as they were.
 *   CW_ERR_BAD_ARG, before the device is touched: what cw_store_patch refuses of index, parameters, codec and store; a NULL among
 *                 refs (nchunks != 0), offsets, ops (nops != 0), out_refs, out_offsets, out_nchunks; a NULL payload with payload_bytes
 *                 != 0; an op list cw_dev_apply_delta would call malformed over A's bytes and the payload, naming the lowest bad op; a
 *                 stream_first that does not start at 0, decreases or does not end at nchunks; max_out < B's bytes / min_size + 2; base
 *                 + that bound wrapping; offsets that decrease, when an op copies (the plan searches the whole list).
 * nops == 0 gives the empty recipe (*out_nchunks = 0, out_offsets[0] = 0) with no device work.                                      */
int cw_store_compose(cw_dedupe_t *x, const cw_cdc_params *p, int comp_alg, const cw_store *st,
                     const uint64_t *refs, const uint64_t *offsets, size_t nchunks,
                     const uint64_t *stream_first /* may be NULL */, size_t nstreams,
                     const cw_delta_op *ops, size_t nops, const void *payload, size_t payload_bytes,
                     uint64_t base, size_t lookahead /* 0 = default */,
                     uint64_t *out_refs, uint64_t *out_offsets, size_t max_out, size_t *out_nchunks,
                     cw_compose_stats *stats /* may be NULL */);

/* ---- chunk bundles: stored chunks from one store to another -------------------------------------------
 * A bundle is a manifest and a payload.  The manifest lists the n distinct chunks a set of recipes names, in ascending value of
 * the sending store: digest[k], value[k] and loc[k] (a cw_chunk_loc whose pos is relative to the payload; all zero = listed but
 * not carried).  The payload holds the carried chunks' stored bytes back to back.  Stored form is the store's own (compressed, or
 * raw with CW_CHUNK_RAW): nothing on the path decodes or encodes, so sender and receiver agree on codec and hash algorithm.
 * The manifest comes from cw_dev_store_mark + cw_dev_dedupe_export_live, the payload from cw_dev_store_export_chunks; the receiver
 * runs cw_dev_dedupe over the manifest's digests, cw_dev_store_import_chunks with that call's selection, and
 * cw_dev_translate_refs over every recipe.  The calls follow the store's conventions: device pointers, counts read on the device,
 * queued on `stream`, nothing synchronises, every decision made on the device and all or nothing.                               */
/* Takes stored chunks out by value.  n = min(*d_count, max_count); position k < n names the directory entry of value d_values[k],
 * which must exist and be sound by cw_dev_store_compact's entry checks.  The entries' stored bytes go to d_out back to back in
 * position order, d_out_loc[k] = {pos in d_out, stored, raw word}.  d_result[3] = {verdict, the total bytes, n}: verdict 2 when a
 * position names no entry of the directory (CW_DEDUPE_MISS does), an all-zero entry or an unsound one -- the total then counts
 * the other positions; else 1 when the total > out_bytes; else 0.  With a verdict other than 0 no byte of d_out and no
 * d_out_loc changes: out_bytes == 0 with d_out == NULL is a dry run that reports the room needed.  A value named twice is
 * exported twice.  No load leaves d_store[0..store_bytes), d_dir[0..dir_entries) or d_values[0..n), whatever they hold.
 * CW_ERR_BAD_ARG before anything is launched: a NULL pointer (d_store when store_bytes is 0 and d_out when out_bytes is 0 may
 * be), max_count > 2^32 - 256, dir_entries == 0, a d_dir or d_out_loc that is not 16-byte aligned, a d_values, d_count or
 * d_result that is not 8-byte aligned, [d_out, +out_bytes) overlapping [d_store, +store_bytes).  Scratch, per stream:
 * 72 + 12 * max_count bytes.                                                                                                   */
int cw_dev_store_export_chunks(const void *d_store, size_t store_bytes, const cw_chunk_loc *d_dir, uint64_t dir_base,
                               size_t dir_entries, const uint64_t *d_values, const uint64_t *d_count, size_t max_count,
                               void *d_out, size_t out_bytes, cw_chunk_loc *d_out_loc, uint64_t *d_result /* [3] */, void *stream);
/* cw_dev_store_chunks for chunks that arrive in stored form: a bundle of n = min(*d_count, max_count) chunks, d_in_loc[k]
 * pointing into d_in[0..in_bytes).  d_sel / d_nsel select as cw_dev_store_chunks' do (cw_dev_dedupe's d_new_idx / d_n_new over
 * the manifest's digests; NULL / NULL = every chunk; at most max_count positions).  Selected position j names chunk k = d_sel[j]:
 * its bytes d_in[loc.pos .. + loc.stored) are appended at *d_used + the stored bytes of the selected positions before it,
 * d_dir[base + k - dir_base] = {new pos, stored, raw word}, then *d_used grows by the total.  d_result[2] = {verdict, the total}:
 * verdict 3 when a selected k >= n or a selected entry is all zero, unsound by cw_dev_store_compact's checks or leaves in_bytes
 * (the total then counts the other positions); else 1 when *d_used + total > store_bytes; else 2 when a selected base + k leaves
 * [dir_base, dir_base + dir_entries) or wraps; else 0.  With a verdict other than 0, no store byte, no directory entry and not
 * *d_used change.  Two positions naming one chunk store it twice; either entry stays.  No load leaves d_in[0..in_bytes),
 * d_in_loc[0..n) or the selection.  CW_ERR_BAD_ARG before anything is launched: a NULL pointer (d_sel and d_nsel may be NULL
 * together; d_in when in_bytes is 0; d_store when store_bytes is 0), max_count > 2^32 - 256, dir_entries == 0, a d_in_loc or d_dir
 * that is not 16-byte aligned, a d_count, d_nsel, d_used or d_result that is not 8-byte aligned, [d_in, +in_bytes) overlapping
 * [d_store, +store_bytes).  Scratch, per stream: 72 + 12 * max_count bytes.                                                    */
int cw_dev_store_import_chunks(const void *d_in, size_t in_bytes, const cw_chunk_loc *d_in_loc, const uint64_t *d_count,
                               size_t max_count, const uint32_t *d_sel, const uint64_t *d_nsel, uint64_t base,
                               void *d_store, size_t store_bytes, uint64_t *d_used,
                               cw_chunk_loc *d_dir, uint64_t dir_base, size_t dir_entries, uint64_t *d_result /* [2] */, void *stream);
/* Rewrites a recipe from one store's values to another's.  d_from[0..p), p = min(*d_npairs, max_pairs), is ascending (what
 * cw_dev_dedupe_export_live writes when the index holds every flagged value); for each position j < min(*d_count, max_count) a binary search of
 * d_ref[j] in d_from: a hit at k gives d_out[j] = d_to[k], any other position gives CW_DEDUPE_MISS and is counted:
 * *d_n_missing (u64) += their number, so several calls accumulate as cw_dev_store_mark's counter does.  d_out may be d_ref.  With
 * d_to = the d_ref cw_dev_dedupe wrote for the manifest's digests, the sender's recipe becomes the receiver's.  CW_ERR_BAD_ARG
 * before anything is launched: a NULL pointer, a pointer that is not 8-byte aligned, max_count or max_pairs > 2^32 - 256.
 * No scratch.                                                                                                                  */
int cw_dev_translate_refs(const uint64_t *d_ref, const uint64_t *d_count, size_t max_count,
                          const uint64_t *d_from, const uint64_t *d_to, const uint64_t *d_npairs, size_t max_pairs,
                          uint64_t *d_out, uint64_t *d_n_missing, void *stream);

/* ---- scrub and repair: is what the store holds still good? ---------------------------------------------
 * A scrub walks the directory and checks every stored chunk once, in bounded memory, against the digest the index holds for its
 * value; a chunk found damaged can be put back, in stored form and under its own value, from a peer that holds it (a store the
 * streams were replicated to).  The calls follow the store's conventions: device pointers, counts read on the device, queued on
 * `stream`, nothing synchronises.                                                                                               */
#define CW_SCRUB_OK 0         /* sound, decodes to its length, hashes to a digest the index holds for this value */
#define CW_SCRUB_MALFORMED 1  /* the decoder's verdict on the stored bytes (cw_dev_restore_chunks' status 1) */
#define CW_SCRUB_UNSOUND 2    /* the entry fails cw_dev_store_compact's entry checks, or is all zero while d_live flags it */
#define CW_SCRUB_MISMATCH 3   /* decodes, the index holds the value, none of its digests for it equals the computed one */
#define CW_SCRUB_ORPHAN 4     /* decodes, but no index entry carries this value: cannot be judged */
#define CW_SCRUB_SKIPPED 5    /* not selected: all zero with d_live == NULL, or d_live[idx] == 0 */
/* One window of a scrub.  The hash algorithm is the index's; the call is serialised with the index's other calls and leaves the
 * index unchanged, as cw_dev_dedupe_lookup and cw_dev_dedupe_export_live do.
 *   window        Let c = *d_cursor.  If c >= dir_entries the call writes nothing at all.  Otherwise E = min(dir_entries, c +
 *                 entry_cap), entry_cap = CW_SCRUB_ENTRIES (default 2^20, at least 64).  Entry idx is SELECTED iff, with d_live ==
 *                 NULL, it is not all zero, or, with d_live given, d_live[idx] != 0.  It is DECODABLE iff it is selected and sound
 *                 by cw_dev_store_compact's entry checks (length 1..65536, bits 17..30 zero, stored != 0, a raw entry has stored ==
 *                 length, pos + stored <= store_bytes).  need(idx) = its length when decodable, else 0.  e is the largest index in
 *                 (c, E] with the sum of need over [c, e) <= work_bytes; work_bytes >= 65536, so e > c.  Then *d_cursor = e.
 *   statuses      Every d_status[idx] with c <= idx < e is written, nothing outside [c, e) is.  A decodable entry goes through
 *                 cw_dev_restore_chunks' own checks and decoder into d_work, back to back from byte 0, and is hashed there; one sweep
 *                 of the index's table then compares: of the index entries that carry the value dir_base + idx, a match by any gives
 *                 0, none matching gives 3, no such entry gives 4.  A decodable entry whose stored bytes are malformed gets 1; a
 *                 selected entry that is not decodable 2; an entry that is not selected 5.  An entry's status is a property of the
 *                 store, the directory, the flags and the index: it does not depend on work_bytes, CW_SCRUB_ENTRIES or where a
 *                 window starts.
 *   totals        d_totals[8] (u64) += {checked, ok, malformed, unsound, mismatch, orphan, raw bytes hashed, windows}, so that a loop
 *                 of windows sums as cw_dev_store_mark's counter does: checked = the sum of the five counts behind it (skipped
 *                 entries are not counted), raw bytes hashed = the sum of need over [c, e), windows += 1.
 * Whatever the store, the directory and the flags hold, no load leaves d_store[0..store_bytes), d_dir[0..dir_entries),
 * d_live[0..dir_entries) or the table, and no store leaves d_work[0..work_bytes), d_status[c..e), the cursor, the totals or the
 * scratch.  The bytes of d_work are unspecified afterwards.
 * CW_ERR_BAD_ARG before anything is launched: a NULL pointer (d_live may be NULL; d_store when store_bytes is 0), an unknown codec,
 * dir_entries == 0 or above 2^32 - 256, work_bytes < 65536, a d_dir that is not 16-byte aligned, a d_cursor or d_totals that is not
 * 8-byte aligned, an index of another device.  Scratch, per stream: 72 + (28 + digest bytes) * W bytes, W = min(entry_cap,
 * dir_entries) (92 MiB at the default for 64-byte digests and 2^20 entries or more), plus cw_dev_hash_chunks' 4 bytes per window
 * entry.  Not synchronised.                                                                                                      */
int cw_dev_store_verify(cw_dedupe_t *x, int comp_alg,
                        const void *d_store, size_t store_bytes, const cw_chunk_loc *d_dir, uint64_t dir_base, size_t dir_entries,
                        const uint32_t *d_live /* may be NULL */, uint64_t *d_cursor /* in/out */,
                        void *d_work, size_t work_bytes,
                        uint32_t *d_status /* [dir_entries] */, uint64_t *d_totals /* [8], accumulates */, void *stream);
typedef struct cw_scrub_stats { uint64_t checked, ok, malformed, unsound, mismatch, orphan, raw_bytes, windows; } cw_scrub_stats;
/* The whole directory, synchronous: a work buffer of CW_STORE_PIECE bytes (default 256 MiB, raised to 65536) from the calling
 * thread's context scratch (grows only), a zeroed cursor and totals, cw_dev_store_verify until the cursor reaches dir_entries with
 * one synchronise per window, then the statuses (host, may be NULL) and the totals (may be NULL) come down.  d_live is device
 * memory and must be complete when the call is made.  CW_OK whatever the statuses are, like cw_store_restore.  CW_ERR_BAD_ARG: a
 * NULL index or store, what cw_dev_store_verify refuses.                                                                         */
int cw_store_scrub(cw_dedupe_t *x, int comp_alg, const cw_store *st, const uint32_t *d_live /* device, may be NULL */,
                   uint32_t *status /* host, [dir_entries], may be NULL */, cw_scrub_stats *stats /* may be NULL */);
/* cw_dev_store_import_chunks with explicit values and no selection: puts stored chunks back under their own values.  For position
 * k < n = min(*d_count, max_count): its bytes d_in[loc.pos .. + loc.stored), loc = d_in_loc[k], are appended at *d_used + the stored
 * bytes of the positions before it, d_dir[d_values[k] - dir_base] = {new pos, stored, raw word}, then *d_used grows by the total.
 * d_result[2] = {verdict, the total}: verdict 3 when an incoming entry is all zero, unsound by cw_dev_store_compact's checks or
 * leaves in_bytes (the total then counts the other positions); else 1 when *d_used + total > store_bytes; else 2 when a value lies
 * outside [dir_base, dir_base + dir_entries); else 4 when the entry a position names has, in the length field of its raw word, a
 * length in 1..65536 that differs from the incoming length -- a replacement keeps the chunk's length, or every recipe's offsets
 * would lie; an all-zero entry, or one whose own length field is unsound, takes any length; else 0.  With a verdict other than 0,
 * no store byte, no directory entry and not *d_used change.  The replaced chunk's old bytes stay where they are until the next
 * compaction.  A value named twice is stored twice, and either entry stays.  No load leaves d_in[0..in_bytes), d_in_loc[0..n),
 * d_values[0..n) or d_dir[0..dir_entries).  CW_ERR_BAD_ARG before anything is launched: a NULL pointer (d_in when in_bytes is 0
 * and d_store when store_bytes is 0 may be), max_count > 2^32 - 256, dir_entries == 0, a d_in_loc or d_dir that is not 16-byte
 * aligned, a d_values, d_count, d_used or d_result that is not 8-byte aligned, [d_in, +in_bytes) overlapping [d_store,
 * +store_bytes).  Scratch, per stream: 72 + 12 * max_count bytes.                                                                */
int cw_dev_store_replace_chunks(const void *d_in, size_t in_bytes, const cw_chunk_loc *d_in_loc, const uint64_t *d_values,
                                const uint64_t *d_count, size_t max_count,
                                void *d_store, size_t store_bytes, uint64_t *d_used,
                                cw_chunk_loc *d_dir, uint64_t dir_base, size_t dir_entries, uint64_t *d_result /* [2] */, void *stream);

/* ---- guard stripes: XOR redundancy over the stored bytes, repair without a peer --------------------------
 * Two parameters: `stripe` = S, a power of two with 65536 <= S <= 2^30, and `group` = G, 1 <= G <= 256; W = G * S.  Store byte p
 * belongs to group p / W and column p % S.  The guard is a caller-owned device buffer like the store's triple, with a u64 cursor
 * `covered` beside it: for every group g and column c
 *     d_guard[g * S + c] = the XOR of d_store[p] over all p < covered with p / W == g and p % S == c.
 * A zeroed guard with covered == 0 guards an empty store; the guard is 1 / G of the store.  The store only appends, so the bytes
 * below `covered` never change and an update folds in only what was appended.  A stored extent is at most 65536 <= S bytes, so it
 * never meets one of its own bytes in a column, whatever boundaries it straddles: any one extent can be rebuilt from the guard and
 * the other bytes of its groups.  The calls follow the store's conventions: device pointers, counts and cursors read on the device,
 * queued on `stream`, nothing synchronises, every decision made on the device and all or nothing.  All three refuse with
 * CW_ERR_BAD_ARG before anything is launched: a NULL pointer (d_store may be NULL when store_bytes is 0, and what each call names), a
 * stripe or group outside the bounds above, guard_bytes < cw_store_guard_bytes(store_bytes, stripe, group), more than 2^32 - 256
 * groups, a d_store or d_guard that is not 16-byte aligned, [d_guard, +guard_bytes) overlapping [d_store, +store_bytes).           */
#define CW_GUARD_MIN_STRIPE 65536u
#define CW_GUARD_MAX_STRIPE (1u << 30)
#define CW_GUARD_MAX_GROUP 256u
/* The guard bytes a store of store_bytes bytes needs: ceil(store_bytes / W) * S; 0 for a geometry that is not allowed.  Host only. */
size_t cw_store_guard_bytes(size_t store_bytes, size_t stripe, unsigned group);
/* Folds d_store[from, to), from = *d_covered and to = *d_used, into the guard, then sets *d_covered = to.  d_result[4] = {verdict,
 * from, to, the bytes folded}.  Verdict 1 when from > to or to > store_bytes: then no guard byte and not the cursor change and the
 * bytes folded are 0.  Every byte of the range is folded exactly once, and the cursor is written by a second kernel, behind every
 * guard byte: the call can be queued directly behind any call that appends, and a second call behind it folds nothing.  One lane
 * owns each 16-byte guard word the range touches, loads the at most G store words behind it, masks the bytes outside the range and
 * does one read-modify-write; there are no atomics.  Whatever the cursors hold, no load leaves d_store[from, to) or the guard words
 * of the groups of [from, to), and no store leaves those guard words, *d_covered and d_result.  CW_ERR_BAD_ARG also for: a NULL
 * d_used, d_covered or d_result, or one that is not 8-byte aligned.  No scratch.                                                 */
int cw_dev_store_guard_update(const void *d_store, size_t store_bytes, const uint64_t *d_used, uint64_t *d_covered /* in/out */,
                              size_t stripe, unsigned group, void *d_guard, size_t guard_bytes, uint64_t *d_result /* [4] */, void *stream);
/* Recomputes the XOR over d_store[0, *d_covered) and compares it with the guard, every column of the N = ceil(*d_covered / W) groups
 * below the cursor: a group differs when a store byte below the cursor changed -- whether or not a live entry names it -- or a
 * guard byte did.  d_result[4] = {verdict, N, the groups that differ, the lowest such group or ~0}; d_group_bad (u32 per group, may be
 * NULL) gets 1 or 0 for each group below N.  Verdict 1 when *d_covered > store_bytes: N is then 0.  Nothing else is written, and no
 * load leaves d_store[0, *d_covered) or the guard bytes of those groups.  CW_ERR_BAD_ARG also for: a NULL d_covered or d_result, or
 * one that is not 8-byte aligned; a d_group_bad that is not 4-byte aligned.  Scratch, per stream: 64 + 4 * ceil(store_bytes / W).   */
int cw_dev_store_guard_check(const void *d_store, size_t store_bytes, const uint64_t *d_covered, size_t stripe, unsigned group,
                             const void *d_guard, size_t guard_bytes, uint32_t *d_group_bad /* may be NULL */, uint64_t *d_result /* [4] */,
                             void *stream);
/* Rebuilds stored chunks from the guard and the other bytes of their groups.  n = min(*d_count, max_count); position k < n names the
 * directory entry of value d_values[k], as cw_dev_store_export_chunks' positions do.  d_status[k] (u32) =
 *   2 (unprotected)  the value names no entry, or the entry is all zero, unsound by cw_dev_store_compact's entry checks, or ends above
 *                    *d_covered.  An unprotected position has no extent and takes no part in what follows.
 *   1 (collides)     with E the SET of bytes in the extents of all other positions: some byte p of the extent has a byte p' != p in E
 *                    with the same group and the same column.  A value named twice does not collide with itself (those are the same
 *                    bytes).  The test is a symmetric "exists": the statuses are a function of the arguments alone.
 *   0 (rebuilt)      every byte is the guard byte XOR the other members' bytes of its column below *d_covered.
 * The rebuilt extents go to d_out back to back in position order, d_out_loc[k] = {pos in d_out, stored, raw word}, all zero for a
 * position that was not rebuilt.  d_result[4] = {verdict, the total bytes, n, the positions rebuilt}.  Verdict 2 when *d_covered >
 * store_bytes: every position is then unprotected.  Else verdict 1 when the total > out_bytes.  With a verdict other than 0 no byte of
 * d_out and no d_out_loc changes, while d_status and d_result are written: out_bytes == 0 with d_out == NULL is the dry run.  The
 * rebuild trusts the bytes of the other members: damage there that the list does not name gives wrong bytes, so the caller verifies
 * the result by digest.  The work is linear in n plus, per position, the listed extents that share one of its at most two groups.
 * Whatever the buffers hold, no load leaves d_store[0, *d_covered), the guard, d_dir[0..dir_entries) or d_values[0..n), and no store
 * leaves the rebuilt extents' places in d_out, d_out_loc[0..n), d_status[0..n) and d_result.  CW_ERR_BAD_ARG also for: a NULL pointer
 * (d_out may be NULL when out_bytes is 0), max_count > 2^32 - 256, dir_entries == 0, a d_dir or d_out_loc that is not 16-byte
 * aligned, a d_covered, d_values, d_count or d_result that is not 8-byte aligned, a d_status that is not 4-byte aligned, [d_out,
 * +out_bytes) overlapping the store or the guard.  Scratch, per stream: 80 + 28 * max_count + 16 * ceil(store_bytes / W) bytes.    */
int cw_dev_store_guard_rebuild(const void *d_store, size_t store_bytes, const cw_chunk_loc *d_dir, uint64_t dir_base, size_t dir_entries,
                               const uint64_t *d_covered, size_t stripe, unsigned group, const void *d_guard, size_t guard_bytes,
                               const uint64_t *d_values, const uint64_t *d_count, size_t max_count, void *d_out, size_t out_bytes,
                               cw_chunk_loc *d_out_loc, uint32_t *d_status /* [max_count] */, uint64_t *d_result /* [4] */, void *stream);

/* ---- the dual guard: a second syndrome, so two damaged chunks that meet in a guard byte are both rebuilt ----
 * Beside the XOR guard P = d_guard_p, which is exactly the d_guard of the calls above, a second buffer Q = d_guard_q of the same
 * size, cw_store_guard_bytes.  The field is GF(2^8) with the polynomial x^8 + x^4 + x^3 + x^2 + 1 (0x11D) and the generator 2; with
 * m = (p / S) % G the member of store byte p,
 *     d_guard_q[g * S + c] = the XOR of 2^m (x) d_store[p] over all p < covered with p / W == g and p % S == c.
 * 2 has order 255, so the members' weights differ only for G <= 255: the dual calls refuse group = 256.  A guard cell then gives
 * back two unknown bytes: with the unknown bytes of a cell in members m and o, and P', Q' the cell's guard bytes less every known
 * member's byte below the cursor,  D_m = (Q' ^ 2^o (x) P') (x) inv(2^m ^ 2^o);  with one unknown, D_m = P'.  One cursor serves both
 * buffers.  The three calls follow the conventions of the guard calls above and refuse what they refuse (d_guard_p in d_guard's
 * place, reported under d_guard's name); also, with CW_ERR_BAD_ARG before anything is launched: group > 255, a NULL d_guard_q, one
 * that is not 16-byte aligned, [d_guard_q, +guard_bytes) overlapping the store or [d_guard_p, +guard_bytes).                       */
#define CW_GUARD2_MAX_GROUP 255u
/* cw_dev_store_guard_update for both buffers: folds d_store[from, to), from = *d_covered and to = *d_used, into P and Q, then sets
 * *d_covered = to.  d_result[4] and the verdict are cw_dev_store_guard_update's, and the P bytes written are bit for bit what that
 * call writes for the same arguments.  One lane owns the two 16-byte guard words of a (group, column word) the range touches, loads
 * the at most G store words behind them from the highest member down, masks the bytes outside the range, accumulates Q by Horner's
 * rule with the doubling done on packed dwords, and does two read-modify-writes; there are no tables and no atomics, and the cursor is
 * written by a second kernel.  Whatever the cursors hold, no load leaves d_store[from, to) or the P and Q words of the groups of
 * [from, to), and no store leaves those words, *d_covered and d_result.  No scratch.                                              */
int cw_dev_store_guard2_update(const void *d_store, size_t store_bytes, const uint64_t *d_used, uint64_t *d_covered /* in/out */,
                               size_t stripe, unsigned group, void *d_guard_p, void *d_guard_q, size_t guard_bytes,
                               uint64_t *d_result /* [4] */, void *stream);
/* cw_dev_store_guard_check for both buffers.  d_group_bad[g] (u32 per group below N, may be NULL) = bit 0 when a P word of the group
 * differs, bit 1 when a Q word does: a changed store byte sets both, a changed guard byte its own.  d_result[4] = {verdict, N, the
 * groups with any bit, the lowest such group or ~0}.  Nothing else is written, and no load leaves d_store[0, *d_covered) or the P and
 * Q bytes of those groups.  Scratch, per stream: 64 + 8 * ceil(store_bytes / W).                                                  */
int cw_dev_store_guard2_check(const void *d_store, size_t store_bytes, const uint64_t *d_covered, size_t stripe, unsigned group,
                              const void *d_guard_p, const void *d_guard_q, size_t guard_bytes, uint32_t *d_group_bad /* may be NULL */,
                              uint64_t *d_result /* [4] */, void *stream);
/* cw_dev_store_guard_rebuild with the second syndrome: positions, the statuses' meaning, d_out, d_out_loc and the verdicts are that
 * call's, except that
 *   1 (collides)     some guard cell of the extent holds three or more DIFFERENT store bytes of the protected listed extents (its own
 *                    among them): three different members cover that column of that group.  A value named twice and overlapping
 *                    entries of one stripe are the same member and never count against each other.  Still a symmetric "exists".
 *   0 (rebuilt)      every byte by the formula above: every other protected listed byte of its cell counts as unknown, whether or not
 *                    that other position is itself rebuilt, and every other member's byte below *d_covered as known.
 * d_result[5] = {verdict, the total bytes, n, the positions rebuilt, the rebuilt positions that have a partner in some cell -- those
 * that needed Q}; the fifth word is counted whatever the verdict is.  While it runs, a rebuilt position's place in d_out holds a
 * byte per byte of working state; with a verdict other than 0 no byte of d_out and no d_out_loc changes.  The work is linear in n and
 * in the rebuilt bytes plus, per piece of a position (at most two), its group's listed pieces once, once more for each of them that
 * overlaps it, and the overlapped columns once per overlapping piece.  Whatever the buffers hold, no load leaves
 * d_store[0, *d_covered), the two guards, d_dir[0..dir_entries), d_values[0..n) or the rebuilt extents' places in d_out, and no store
 * leaves those places, d_out_loc[0..n), d_status[0..n) and d_result.  CW_ERR_BAD_ARG also for what cw_dev_store_guard_rebuild refuses,
 * and [d_out, +out_bytes) overlapping either guard.  Scratch, per stream: 80 + 28 * max_count + 16 * ceil(store_bytes / W) bytes,
 * as for the single guard.                                                                                                        */
int cw_dev_store_guard2_rebuild(const void *d_store, size_t store_bytes, const cw_chunk_loc *d_dir, uint64_t dir_base, size_t dir_entries,
                                const uint64_t *d_covered, size_t stripe, unsigned group, const void *d_guard_p, const void *d_guard_q,
                                size_t guard_bytes, const uint64_t *d_values, const uint64_t *d_count, size_t max_count, void *d_out,
                                size_t out_bytes, cw_chunk_loc *d_out_loc, uint32_t *d_status /* [max_count] */, uint64_t *d_result /* [5] */,
                                void *stream);

/* ---- locating damage from the syndromes: which entries to scrub, in the time of a check ---------------------
 * A CELL is one guard byte: group g < N = ceil(*d_covered / W), column c < S.  Its members below the cursor are the store positions
 * q_m = g * W + m * S + c < *d_covered, m < G.  P' = the guard byte XOR those store bytes; Q' (dual call only) = the Q byte XOR the
 * XOR of 2^m (x) d_store[q_m].  A cell is DIRTY when P' != 0, on the dual call when P' != 0 or Q' != 0.  A dirty cell is
 *   LOCATED(m)   dual call only: P' != 0, Q' != 0 and Q' == 2^m (x) P' for an m with q_m < *d_covered (unique, as G <= 255): what one
 *                wrong store byte, in member m, leaves behind -- the RAID-6 error-location identity;
 *   AMBIGUOUS    otherwise: every dirty cell of the single guard; a dual cell where only one syndrome differs (typically a damaged
 *                guard byte); a dual cell with no such m (two or more wrong bytes).
 * An entry is PROTECTED as for cw_dev_store_guard_rebuild: not all zero, sound, and pos + stored <= *d_covered.  d_suspect[idx], one u32
 * per directory entry idx < dir_entries (dir_base shifts none of them):
 *   0            an all-zero entry, or a protected entry none of whose bytes is flagged;
 *   bit 0        some byte p of its extent lies in a cell LOCATED(m) with m = the member of p, (p / S) % G;
 *   bit 1        some byte of its extent lies in an AMBIGUOUS cell;
 *   4 exactly    the entry is not all zero and not protected: it cannot be judged.
 * d_result[8] = {verdict, N, the dirty cells, the located cells, the ambiguous cells, the entries with bit 0 or bit 1, the entries
 * with value 4, 0}.  Verdict 1 when *d_covered > store_bytes: then only d_result is written, {1, 0, 0, 0, 0, 0, 0, 0}.  Every output
 * is an integer count, so the outputs are bit for bit a function of the arguments.  The syndromes hint, they do not judge: two wrong
 * bytes of one cell can look like one wrong byte of a third member, so a caller scrubs the suspects before it mends them.  d_suspect
 * is d_live-shaped: it can be handed as it is to cw_dev_store_verify and cw_store_scrub, where non-zero selects, and to
 * cw_dev_store_account's d_flag.  Whatever the buffers hold, no load leaves d_store[0, *d_covered), the guard bytes of the N groups or
 * d_dir[0..dir_entries), and no store leaves d_suspect[0..dir_entries), d_result or the per-stream scratch.  The calls do not
 * synchronise: they can be queued behind an update.  A lane per 16-byte guard word sums as the check does and a ballot per wavefront
 * stores its 64 dirty bits; a lane per entry then walks its extent's bits and re-sums only the dirty words.  CW_ERR_BAD_ARG, before
 * anything is launched, for whatever the check calls refuse, a NULL d_dir, d_covered, d_suspect or d_result, dir_entries == 0 or above
 * 2^32 - 256, a d_dir that is not 16-byte aligned, a d_suspect that is not 4-byte aligned.  Scratch, per stream:
 * 64 + ceil(store_bytes / W) * S / 128 bytes.                                                                                      */
int cw_dev_store_guard_locate(const void *d_store, size_t store_bytes, const cw_chunk_loc *d_dir, uint64_t dir_base, size_t dir_entries,
                              const uint64_t *d_covered, size_t stripe, unsigned group, const void *d_guard, size_t guard_bytes,
                              uint32_t *d_suspect /* [dir_entries] */, uint64_t *d_result /* [8] */, void *stream);
int cw_dev_store_guard2_locate(const void *d_store, size_t store_bytes, const cw_chunk_loc *d_dir, uint64_t dir_base, size_t dir_entries,
                               const uint64_t *d_covered, size_t stripe, unsigned group, const void *d_guard_p, const void *d_guard_q,
                               size_t guard_bytes, uint32_t *d_suspect /* [dir_entries] */, uint64_t *d_result /* [8] */, void *stream);

/* plain device memory on the calling thread's device, for C callers of cw_dev_* (the host programs link no HIP runtime) */
void *cw_dev_alloc(size_t bytes);                                   /* NULL on failure */
void  cw_dev_free(void *d_p);
int   cw_dev_upload(void *d_dst, const void *src, size_t bytes);    /* synchronous copies */
int   cw_dev_download(void *dst, const void *d_src, size_t bytes);
int   cw_dev_synchronize(void);                                     /* all work queued on the calling thread's device */

/* ---- kernel timing (the reference times with std::chrono around its calls, hash.cpp:11-18, HashAndCompress.cpp:397-406;
 *      device work is asynchronous, so the library brackets its own launches with HIP events on the stream each
 *      kernel is launched on).  Per calling thread.  Kinds: [0] codec kernels, [1] hash kernel, [2] reserved.       */
void cw_profile_enable(int on);
int  cw_profile_read(double ms_sum[3], unsigned count[3], int reset);   /* synchronises on the recorded events */
/* names of the kernels the calling thread's latest codec (kind 0) / hash (kind 1) launch used, as rocprofv3 prints them */
int  cw_profile_kernels(int kind, char *buf, size_t cap);

/* ---- CW_TESTING: tuning and test knobs -----------------------------------------------------------------------------
 * Every knob the launch policy reads (thresholds such as CW_LZ4_LANES / CW_LZF_LANES / CW_LZ4_VTAB, CW_LANES_*, CW_LZF_ROUND,
 * CW_LZ_FORCE_REDO, CW_DECODE_LANES, CW_HOST_*CHUNK_MB, CW_STORE_PIECE, ...; README.md lists them) is read PER CALL: the value given
 * here wins, the environment variable of the same name is the default.  value = NULL removes an override; a name the
 * library does not read is refused with CW_ERR_BAD_ARG.  A launch sees the knobs as they were when it started, so setting
 * them while other threads compute is safe.  Not part of the reference's interface (it has no tunables beyond its CLI);
 * meant for tests and profiling.                                                                                      */
int  cw_tune_set(const char *key, const char *value);
void cw_tune_reset(void);
/* What cw_dev_compress would launch for nblocks blocks of block_bytes under the knobs as they are now, without a device:
 * line 1 = the kernels as cw_profile_kernels reports them after such a call; then one `key=value` line per field of the launch
 * plan (kernels, grids, LDS bytes, streams, thresholds, reserves, workspace bytes), in a fixed order.  src_misalign stands for
 * (src | src_stride) & 15, dst_misalign for (dst | dst_stride) & 15.  CW_ERR_BAD_ARG: sizes the call would refuse, or a buffer
 * that is too small.                                                                                                     */
int  cw_plan_describe(int comp_alg, size_t block_bytes, size_t nblocks, unsigned src_misalign, unsigned dst_misalign, char *buf,
                      size_t cap);
/* The same for cw_dev_hash: line 1 = the hash kernels as cw_profile_kernels(1, ...) reports them after such a call; for a Skein call
 * that goes out in sliced launches, one `slice=b..e interior=0|1` line per launch follows (steps [b, e) of every block, the output
 * transform being a block's last step; interior = the all-message-steps kernel).  src_misalign stands for (src | src_stride) & 15,
 * digest_misalign for d_digests & 15.  may_slice = 0 describes the one caller that never slices, HashOffload; every other call
 * that hashes fixed-size blocks is described by may_slice = 1.  CW_ERR_BAD_ARG: what cw_dev_hash refuses (an unknown hash_alg,
 * block_bytes > CW_MAX_BLOCK_BYTES), or a buffer that is too small.                                                        */
int  cw_hash_plan_describe(int hash_alg, size_t block_bytes, size_t nblocks, unsigned src_misalign, unsigned digest_misalign,
                           int may_slice, char *buf, size_t cap);

/* ---- HashOffload (HashOffload.h:13-64): batch object + the offload thread that drains it -------
 * Lifecycle  hInit --Enqueue--> hQueued --Start--> hOffloaded --Complete--> hComplete.
 * Start() = "xfer data, load kernel" (:26-31): async H2D + hash kernel + async D2H on the object's stream.
 * Complete() = "wait for and reap the results" (:33-40): blocks, then runs on_complete(arg).       */
typedef struct cw_offload cw_offload_t;
enum { CW_OFFLOAD_INIT = 0, CW_OFFLOAD_QUEUED = 1, CW_OFFLOAD_OFFLOADED = 2, CW_OFFLOAD_COMPLETE = 3,
       CW_OFFLOAD_FAILED = 4 /* Start()/Complete() failed: nothing is in flight, cw_offload_error() says why;
                                Reset() makes the object usable again */ };

cw_offload_t *cw_offload_create(int hash_alg, int n_blocks, size_t block_bytes);   /* HashOffload(int nBlocks) */
void cw_offload_destroy(cw_offload_t *h);
int  cw_offload_reset(cw_offload_t *h, char *data, char *results,
                      void (*on_complete)(void *), void *arg);                     /* Reset(d, r, f) */
int  cw_offload_enqueue(cw_offload_t *h);                                          /* Enqueue() */
int  cw_offload_start(cw_offload_t *h);                                            /* Start() */
int  cw_offload_complete(cw_offload_t *h);                                         /* Complete() */
int  cw_offload_completed(const cw_offload_t *h);                                  /* Completed() */
int  cw_offload_state(const cw_offload_t *h);
int  cw_offload_error(const cw_offload_t *h);                                      /* CW_OK, or why the state is hFailed */
int  cw_offload_do(cw_offload_t *h);                                               /* DoOffload() */

/* hashing_offload_entry_point (:160-183): one consumer thread popping a queue of HashOffload* */
int  cw_offload_thread_start(void);
int  cw_offload_submit(cw_offload_t *h);   /* Enqueue() + push + notify (the producer the reference never wrote);
                                              on_complete runs on the offload thread also when the offload FAILED --
                                              check cw_offload_completed() / cw_offload_error() in it */
void cw_offload_thread_stop(void);         /* allWorkFinished = true; join */

/* ---- several GPUs of one node (BASELINE.json configs[4]) ----------------------------------------------
 * The reference's only parallelism is worker threads over independent blocks (HashAndCompress.cpp:398-403); its dormant
 * --gpu-offload seam (:305,331) has one device at most.  Here the block index space is cut into contiguous shards, one
 * per device, each processed with the single-device entry points above (one host thread per device, cw_set_device);
 * the only exchange is the result gather after a pass, over RCCL (xGMI between the GPUs of the node):
 * ncclAllGather of the digests, ncclAllReduce(sum, u64) of the byte totals.  RCCL is loaded (dlopen) by cw_mgpu_create
 * only.                                                                                                             */
/* shard g of G over n units: [*first, *last) = [g*n/G, (g+1)*n/G) */
void cw_shard_range(size_t n, int g, int G, size_t *first, size_t *last);
typedef struct cw_mgpu cw_mgpu_t;
cw_mgpu_t *cw_mgpu_create(const int *devices, int ndev);   /* cw_init on each + ncclCommInitAll; NULL on failure */
void cw_mgpu_destroy(cw_mgpu_t *m);
int  cw_mgpu_ndev(const cw_mgpu_t *m);
int  cw_mgpu_device(const cw_mgpu_t *m, int rank);
const char *cw_mgpu_last_error(void);
/* The gather: rank g contributes bytes_each bytes at d_local[g] (its shard's digests, padded to the largest shard) and
 * ntotals u64 at d_totals[g]; afterwards d_all[g] on EVERY device holds all ranks' contributions in rank order
 * (ndev * bytes_each bytes) and d_totals[g] the element-wise sums.  The work that produced the inputs must be complete
 * (synchronise its streams first).  Either half may be skipped (bytes_each = 0 / ntotals = 0).  Blocking.            */
int  cw_mgpu_gather(cw_mgpu_t *m, const void *const *d_local, size_t bytes_each, void *const *d_all,
                    uint64_t *const *d_totals, size_t ntotals);

#ifdef __cplusplus
}
#endif
#endif /* CW_HASHCOMPRESS_H */
