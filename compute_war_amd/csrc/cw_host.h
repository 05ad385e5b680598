// cw_host.h -- what the host files of libcwhc.so share (internal).  cw_api.hip defines errors, devices, contexts and the fixed-block
// launches declared here; cw_chunks.hip defines the chunk helpers, cw_dedupe.hip the fused call's internal form at the end.
// cw_offload.hip and cw_ingest.hip only use them.
#pragma once

#include <hip/hip_runtime.h>

#include "../../include/cw_hashcompress.h"
#include "cw_device.h"
#include "stream_scratch.h"

namespace cw {
namespace host {

// ---- errors: one message per calling thread (cw_last_error) ----
int fail(int code, const char *fmt, ...); // records the message, returns code

#define HIP_TRY(expr)                                                                                          \
    do {                                                                                                       \
        hipError_t e_ = (expr);                                                                                \
        if (e_ != hipSuccess) return ::cw::host::fail(CW_ERR_HIP, "%s: %s", #expr, hipGetErrorString(e_));     \
    } while (0)

// the result of a launch: CW_OK, or the failure recorded as "<what>: <HIP's text>"
int launched(hipError_t e, const char *what);       // CW_ERR_HIP whatever failed
int launched_nomem(hipError_t e, const char *what); // CW_ERR_NOMEM for hipErrorOutOfMemory, else CW_ERR_HIP

// ---- devices and contexts ----
int current_device();                    // the calling thread's device, -1 before any cw_init
int ensure_init();                       // every entry point: initialise on first use, make the library's device the thread's HIP device
int ctx_stream(hipStream_t *s);          // the stream of the calling thread's context on its device (created on first use)
const cw::SkeinIV &skein_iv(int nw);     // nw = 8: Skein-512-512, else Skein-256-128

// ---- optional per-thread kernel timing (cw_profile_*) ----
enum { PROF_CODEC = 0, PROF_HASH = 1, PROF_OTHER = 2, PROF_KINDS = 3 };
struct ProfScope { // brackets the launches made during its lifetime on `stream`
    int kind; hipStream_t stream; hipEvent_t a = nullptr;
    ProfScope(int k, hipStream_t s);
    ~ProfScope();
};

struct DevBuf { // cw::DeviceBuf with a floor of 1 MiB and the library's error codes; p = the buffer, for the many places that pass it on
    cw::DeviceBuf buf;
    void *p = nullptr;
    int reserve(size_t n)
    {
        const hipError_t e = buf.reserve(n, (size_t)1 << 20);
        p = buf.as<void>();
        return e == hipSuccess ? CW_OK : fail(CW_ERR_NOMEM, "hipMalloc(%zu): %s", n < (1u << 20) ? (size_t)1 << 20 : n, hipGetErrorString(e));
    }
    void release() { (void)buf.release(); p = nullptr; }
};

struct PinnedBuf { // page-locked host staging: the only kind of host memory a copy engine reads or writes at bus speed
    void *p = nullptr;
    size_t cap = 0;
    int reserve(size_t n)
    {
        if (n <= cap) return CW_OK;
        if (p) (void)hipHostFree(p);
        p = nullptr; cap = 0;
        size_t want = n < (1u << 20) ? (1u << 20) : n;
        hipError_t e = hipHostMalloc(&p, want, hipHostMallocDefault);
        if (e != hipSuccess) return fail(CW_ERR_NOMEM, "hipHostMalloc(%zu): %s", want, hipGetErrorString(e));
        cap = want;
        return CW_OK;
    }
    void release() { if (p) (void)hipHostFree(p); p = nullptr; cap = 0; }
};
bool is_pinned(const void *p); // page-locked host memory (cw_host_alloc / cw_host_register): the copy engines use it in place

// What cw_store_ingest / cw_store_ingest_streams (one piece loop, cw_ingest.hip's struct Ingest) and cw_store_restore keep per calling
// thread and device; grows only, freed with the context.
// Index 0 / 1: the two buffers the pieces (windows) alternate between.
struct StoreCtx {
    DevBuf src[2];                                   // ingest: a piece's carry + fresh bytes; restore: a window's bytes
    DevBuf off, dig, ref, new_idx, sizes, slots;     // ingest: one piece's lists and codec slots
    DevBuf rec_ref, rec_off, words;                  // ingest: the recipe as it grows; the counts, results and statistics
    DevBuf ends, first, rec_first;                   // ingest of many streams: a piece's ends and stream index, the recipe's stream index
    PinnedBuf h_ends;                                // the piece's ends on their way up
    DevBuf meta[2], status[2];                       // restore: a window's count | refs | offsets, and its statuses
    PinnedBuf stage[2], h_meta[2], h_status[2], h_words;
    hipEvent_t ev_up[2] = {nullptr, nullptr}, ev_done[2] = {nullptr, nullptr}; // upload into buffer b done; buffer b free again
    hipEvent_t ev_kernel[2] = {nullptr, nullptr};                              // restore: the window's kernel done
    int open();
    void release();
};
// the calling thread's context: its kernel stream, its two copy streams and its StoreCtx (opened)
int ctx_store(StoreCtx **c, hipStream_t *stream, hipStream_t *s_h2d, hipStream_t *s_d2h);

// ---- argument checks written once ----
int check_block(size_t block_bytes);              // <= CW_MAX_BLOCK_BYTES
int check_codec(int comp_alg);                    // LZ4 or LZF
int check_count(const char *name, size_t n);      // <= 2^32 - 256: block and chunk indices are u32 on the device, one lane per item

// ---- fixed-block launches ----
// sliced: long Skein messages (>= 256 steps, >= 4096 blocks) are hashed in several launches of short-lived wavefronts
int dev_hash(int alg, const uint8_t *d_src, size_t bb, size_t stride, size_t n, uint8_t *d_dig, hipStream_t s, bool sliced = false);
int dev_compress(int alg, const uint8_t *d_src, size_t bb, size_t stride, size_t n, uint8_t *d_dst, size_t dst_stride, uint32_t *d_sizes,
                 hipStream_t s, const cw::AfterScan *after_scan = nullptr);

// ---- content-defined chunks (cw_chunks.hip) ----
int cdc_params(const cw_cdc_params *p, cw::CdcParams *out); // checked and with the default gear filled in
int dev_cdc(const cw::CdcParams &p, const uint8_t *d_src, size_t nbytes, int final_, uint64_t *d_offsets, size_t max_offsets, uint64_t *d_nchunks,
            hipStream_t s);
// the streams of cw_dev_cdc_streams: d_ends[nstreams], d_first[nstreams + 1] and *d_result on the device
// (final_ = 0: the last stream is open, cw_dev_cdc_streams_part)
struct StreamList { const uint64_t *d_ends; size_t nstreams; uint64_t *d_first, *d_result; int final_ = 1; };
// everything cw_dev_cdc_streams refuses behind its parameters, none of it needing a device
int cdc_streams_args(const cw::CdcParams &cp, const void *d_src, size_t nbytes, const StreamList &sl, const uint64_t *d_offsets, size_t max_offsets,
                     const uint64_t *d_nchunks);
int dev_cdc_streams(const cw::CdcParams &p, const uint8_t *d_src, size_t nbytes, const StreamList &sl, uint64_t *d_offsets, size_t max_offsets,
                    uint64_t *d_nchunks, hipStream_t s);
int dev_hash_chunks(int alg, const uint8_t *d_src, size_t src_bytes, const uint64_t *d_offsets, const uint64_t *d_nchunks, size_t max_chunks,
                    uint8_t *d_dig, hipStream_t s);
// everything cw_dev_compress_chunks refuses, none of it needing a device
int compress_chunks_args(int comp_alg, const void *d_src, size_t src_bytes, const uint64_t *d_offsets, const uint64_t *d_nchunks, size_t max_chunks,
                         const uint32_t *d_sel, const uint64_t *d_nsel, const void *d_dst, size_t dst_bytes, const uint32_t *d_sizes);
int dev_compress_chunks(int comp_alg, const uint8_t *d_src, size_t src_bytes, const uint64_t *d_offsets, const uint64_t *d_nchunks, size_t max_chunks,
                        const uint32_t *d_sel, const uint64_t *d_nsel, uint8_t *d_dst, uint32_t *d_sizes, hipStream_t s);


// ---- the fused chunk call's internal form (cw_dedupe.hip) ----
// cw_store_ingest's part in a piece's one synchronise: the chunk count, the bytes consumed, *d_used and *d_verdict (the previous
// piece's commit) come back together through d_counts -> h_counts (pinned), and admit(self, k, h_counts) runs beside the index's own
// admission, before anything is inserted.  Whatever it returns other than CW_OK ends the call there.
struct PieceAdmit {
    const uint64_t *d_used, *d_verdict;
    uint64_t *d_counts, *h_counts; // d_counts[4]; h_counts[5]: with streams, [4] takes the verdict on d_ends
    int (*admit)(void *self, size_t k, const uint64_t *h_counts);
    void *self;
    bool *inserted; // set once the piece's chunks are queued for the index: a failure behind that point is no refusal
    // cw_store_patch: called between the chunker and the hash, for what shortens *d_nchunks on the device (cw_dev_cdc_resync) and for
    // the copies that ride on the piece's one synchronise; whatever it returns other than CW_OK ends the call there
    int (*after_cdc)(void *self, hipStream_t s) = nullptr;
};
// cw_dev_cdc_dedupe_compress is this with hook == nullptr and streams == nullptr; cw_dev_cdc_streams_dedupe_compress gives `streams`
// (the chunker is then cw_dev_cdc_streams_part with streams->final_, final_ is not read, and the verdict on d_ends comes back with the
// chunk count, in a word of its own)
int dev_cdc_dedupe_compress(cw_dedupe_t *x, const cw_cdc_params *p, int comp_alg, const void *d_src, size_t nbytes, int final_, uint64_t base,
                            uint64_t *d_offsets, size_t max_offsets, uint64_t *d_nchunks, void *d_digests, uint64_t *d_ref, uint32_t *d_new_idx,
                            uint64_t *d_n_new, void *d_dst, size_t dst_bytes, uint32_t *d_sizes, size_t *nchunks, hipStream_t s,
                            const PieceAdmit *hook, const StreamList *streams = nullptr);

} // namespace host
} // namespace cw
