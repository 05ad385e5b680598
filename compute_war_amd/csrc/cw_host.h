// cw_host.h -- what the host files of libcwhc.so share (internal).  cw_api.hip defines errors, devices, contexts and the fixed-block
// launches declared here; cw_chunks.hip defines the chunk helpers at the end.  cw_dedupe.hip and cw_offload.hip only use them.
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
int dev_hash_chunks(int alg, const uint8_t *d_src, size_t src_bytes, const uint64_t *d_offsets, const uint64_t *d_nchunks, size_t max_chunks,
                    uint8_t *d_dig, hipStream_t s);
// everything cw_dev_compress_chunks refuses, none of it needing a device
int compress_chunks_args(int comp_alg, const void *d_src, size_t src_bytes, const uint64_t *d_offsets, const uint64_t *d_nchunks, size_t max_chunks,
                         const uint32_t *d_sel, const uint64_t *d_nsel, const void *d_dst, size_t dst_bytes, const uint32_t *d_sizes);
int dev_compress_chunks(int comp_alg, const uint8_t *d_src, size_t src_bytes, const uint64_t *d_offsets, const uint64_t *d_nchunks, size_t max_chunks,
                        const uint32_t *d_sel, const uint64_t *d_nsel, uint8_t *d_dst, uint32_t *d_sizes, hipStream_t s);

} // namespace host
} // namespace cw
