// cw_api.hip -- the core of the host side of libcwhc.so (the C ABI of include/cw_hashcompress.h over the HIP kernels): errors, devices and
// per-thread contexts, the knob table, the fixed-block device API, profiling, the pipelined host batch path and the reference's slots.
// What the other host files share is declared in cw_host.h and defined here: cw_chunks.hip (content-defined chunks and the chunk store),
// cw_dedupe.hip (the dedupe index and the calls fused with it) and cw_offload.hip (the HashOffload object and its thread).
//
// Structure: a set of initialised devices (cw_init = the reference's empty initializeGpu(),
// src/hashandcompress/HashAndCompress.cpp:95-98) with one "current device" per calling host thread (cw_set_device;
// threads that never choose use the first initialised device), one lazily created context per (thread, device) --
// own HIP streams + growable device/pinned staging buffers, because the reference invokes its slots from --c-threads
// workers with no locking, :398-402 --, and the pipelined host batch path (what HashOffload::Start()/Complete() were meant
// to be, HashOffload.h:26-40).
//
// No CPU fallback exists: every compute path ends in a kernel launch or an error.

#include <atomic>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "cw_host.h"
#include "launch_plan.h"

using namespace cw::host;

namespace {
thread_local char t_err[512] = "";

// ---- optional per-thread kernel timing (cw_profile_*): HIP events on the stream each kernel is launched on ----
struct ProfSpan { int kind; hipEvent_t a, b; };
thread_local bool t_prof_on = false;
thread_local std::vector<ProfSpan> t_prof;
} // namespace

int cw::host::fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(t_err, sizeof t_err, fmt, ap);
    va_end(ap);
    return code;
}

int cw::host::launched(hipError_t e, const char *what) { return e == hipSuccess ? CW_OK : fail(CW_ERR_HIP, "%s: %s", what, hipGetErrorString(e)); }
int cw::host::launched_nomem(hipError_t e, const char *what)
{
    return e == hipErrorOutOfMemory ? fail(CW_ERR_NOMEM, "%s: %s", what, hipGetErrorString(e)) : launched(e, what);
}

cw::host::ProfScope::ProfScope(int k, hipStream_t s) : kind(k), stream(s)
{
    if (t_prof_on && hipEventCreate(&a) == hipSuccess) (void)hipEventRecord(a, stream);
}
cw::host::ProfScope::~ProfScope()
{
    if (!a) return;
    hipEvent_t b = nullptr;
    if (hipEventCreate(&b) == hipSuccess) { (void)hipEventRecord(b, stream); t_prof.push_back({kind, a, b}); }
    else (void)hipEventDestroy(a);
}

// ---- devices ----------------------------------------------------------------------------------------
namespace {
constexpr int kMaxDevices = 16;
std::mutex g_lock;
std::atomic<int> g_default{-1};        // first initialised device: what threads use that never chose one
std::atomic<uint32_t> g_mask{0};       // initialised devices
thread_local int t_device = -1;        // the calling thread's device (cw_init / cw_set_device), -1 = g_default
cw::SkeinIV g_iv512_512, g_iv256_128;  // host-computed, device independent
std::atomic<size_t> g_block_size{4096}; // the reference's global blockSize (:89)
} // namespace

int cw::host::current_device()
{
    const int d = t_device;
    return d >= 0 && ((g_mask.load(std::memory_order_acquire) >> d) & 1u) ? d : g_default.load(std::memory_order_acquire);
}

int cw::host::ensure_init()
{
    int d = current_device();
    if (d < 0) {
        const int rc = cw_init(t_device >= 0 ? t_device : 0);
        if (rc != CW_OK) return rc;
        d = current_device();
    }
    HIP_TRY(hipSetDevice(d));
    return CW_OK;
}

const cw::SkeinIV &cw::host::skein_iv(int nw) { return nw == 8 ? g_iv512_512 : g_iv256_128; }

// ---- per-(thread, device) context ---------------------------------------------------------------------
namespace {
// one chunk of the host batch path in flight: device buffers, pinned staging, the events of its three stages
constexpr int kSlots = 3;
struct Slot {
    DevBuf src, dst, pack, sizes, offs, dig;
    PinnedBuf h_src, h_meta, h_pack;
    hipStream_t stream = nullptr; // this chunk's kernels: codec on `stream`, hash beside it on `side`
    cw::SideStream side;
    hipEvent_t ev_h2d = nullptr, ev_meta = nullptr, ev_payload = nullptr;
    size_t first = 0, n = 0;
    uint64_t total = 0;
    bool borrowed = false; // stream and side's stream belong to the thread's first slot (CW_HOST_SHARED_STREAMS)
    int open(const Slot *lender = nullptr)
    {
        if (ev_h2d) return CW_OK;
        if (lender && lender->stream) {
            stream = lender->stream; borrowed = true;
        } else {
            HIP_TRY(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
        }
        HIP_TRY(side.open(cw::SideStream::least, borrowed ? lender->side.stream : nullptr));
        HIP_TRY(hipEventCreateWithFlags(&ev_meta, hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&ev_payload, hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&ev_h2d, hipEventDisableTiming));
        return CW_OK;
    }
    void release()
    {
        src.release(); dst.release(); pack.release(); sizes.release(); offs.release(); dig.release();
        h_src.release(); h_meta.release(); h_pack.release();
        if (stream && !borrowed) { cw::release_stream_workspaces(stream); (void)hipStreamDestroy(stream); }
        if (side.stream && !side.borrowed) cw::release_stream_workspaces(side.stream);
        side.release();
        borrowed = false;
        if (ev_meta) (void)hipEventDestroy(ev_meta);
        if (ev_payload) (void)hipEventDestroy(ev_payload);
        if (ev_h2d) (void)hipEventDestroy(ev_h2d);
        stream = nullptr; ev_meta = ev_payload = ev_h2d = nullptr;
    }
};

// what the last fused LZ4 call of this thread left behind for the next one: the share of its blocks that the scan queued for the parsers
// (copied back asynchronously; read when it has arrived, never waited for)
struct FusedHint { uint32_t *h_queued = nullptr; hipEvent_t ev = nullptr; bool pending = false; size_t blocks_of_copy = 0; float queued_share = 0.f; };

struct ThreadCtx {
    int device = -1;
    FusedHint hint;
    hipStream_t stream = nullptr;            // kernels of the host-buffer entry points
    hipStream_t s_h2d = nullptr, s_d2h = nullptr; // the two copy directions of the pipelined batch path
    // fork/join for the fused call: the hash runs on `side` beside the codec on the caller's stream
    cw::SideStream side;
    DevBuf src, dst, dig, sizes;             // unpipelined helpers (decompress, tree hash)
    Slot slot[kSlots];
    StoreCtx store;                          // cw_store_ingest / cw_store_restore
    int open(int dev)
    {
        if (stream) return CW_OK;
        device = dev;
        HIP_TRY(hipSetDevice(dev));
        HIP_TRY(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
        HIP_TRY(hipStreamCreateWithFlags(&s_h2d, hipStreamNonBlocking));
        HIP_TRY(hipStreamCreateWithFlags(&s_d2h, hipStreamNonBlocking));
        HIP_TRY(side.open(cw::SideStream::least)); // the hash is the long, ALU-bound kernel: it yields dispatch slots to the codec
        return CW_OK;
    }
    ~ThreadCtx()
    {
        if (!stream) return;
        (void)hipSetDevice(device);
        src.release(); dst.release(); dig.release(); sizes.release();
        for (Slot &s : slot) s.release();
        store.release();
        if (hint.ev) (void)hipEventDestroy(hint.ev);
        if (hint.h_queued) (void)hipHostFree(hint.h_queued);
        cw::release_stream_workspaces(side.stream); cw::release_stream_workspaces(stream);
        side.release();
        (void)hipStreamDestroy(s_h2d); (void)hipStreamDestroy(s_d2h); (void)hipStreamDestroy(stream);
    }
};
struct ThreadCtxSet { std::unique_ptr<ThreadCtx> of[kMaxDevices]; };
thread_local ThreadCtxSet t_ctxs;

// the calling thread's context on its current device (created on first use)
int thread_ctx(ThreadCtx **out)
{
    int rc = ensure_init();
    if (rc != CW_OK) return rc;
    const int d = current_device();
    std::unique_ptr<ThreadCtx> &c = t_ctxs.of[d];
    if (!c) c.reset(new ThreadCtx);
    if ((rc = c->open(d)) != CW_OK) return rc;
    *out = c.get();
    return CW_OK;
}

const size_t kMaxChunkBytes = (size_t)256 << 20; // host-API staging granularity
} // namespace

int cw::host::ctx_stream(hipStream_t *s)
{
    ThreadCtx *c;
    const int rc = thread_ctx(&c);
    if (rc == CW_OK) *s = c->stream;
    return rc;
}

int cw::host::ctx_store(StoreCtx **c, hipStream_t *stream, hipStream_t *s_h2d, hipStream_t *s_d2h)
{
    ThreadCtx *t;
    int rc = thread_ctx(&t);
    if (rc != CW_OK || (rc = t->store.open()) != CW_OK) return rc;
    *c = &t->store; *stream = t->stream; *s_h2d = t->s_h2d; *s_d2h = t->s_d2h;
    return CW_OK;
}

bool cw::host::is_pinned(const void *p)
{
    hipPointerAttribute_t a;
    if (!p || hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return false; }
    return a.type == hipMemoryTypeHost;
}

int cw::host::check_block(size_t block_bytes)
{
    if (block_bytes > CW_MAX_BLOCK_BYTES) return fail(CW_ERR_BAD_ARG, "block_bytes %zu > %u", block_bytes, CW_MAX_BLOCK_BYTES);
    return CW_OK;
}
int cw::host::check_codec(int comp_alg)
{
    return comp_alg == CW_COMP_LZ4 || comp_alg == CW_COMP_LZF ? CW_OK : fail(CW_ERR_BAD_ARG, "unknown compression algorithm %d", comp_alg);
}
int cw::host::check_count(const char *name, size_t n)
{
    return n <= ((size_t)1 << 32) - 256 ? CW_OK : fail(CW_ERR_BAD_ARG, "%s %zu > 2^32 - 256", name, n);
}

// the state words of the plan's call (launch_plan.h): 8 / 4 for the two Skeins, 0 for SHA-256, -1 for no hash kernel at all
static int hash_state_words(int alg)
{
    return alg == CW_HASH_SKEIN512 ? 8 : alg == CW_HASH_SKEIN256_128 ? 4 : alg == CW_HASH_SHA256 ? 0 : -1;
}

// plan (launch_plan.cpp: every decision), enqueue
int cw::host::dev_hash(int alg, const uint8_t *d_src, size_t bb, size_t stride, size_t n, uint8_t *d_dig, hipStream_t s, bool sliced)
{
    ProfScope prof(PROF_HASH, s);
    if (alg == CW_HASH_NONE) return CW_OK;
    const int nw = hash_state_words(alg);
    if (nw < 0) return fail(CW_ERR_BAD_ARG, "unknown hash algorithm %d", alg);
    const cw::HashPlan p = cw::hash_plan(cw::hash_call(nw, d_src, bb, stride, n, d_dig, sliced), cw::knobs());
    return launched(nw ? cw::skein_launch(p, d_src, bb, stride, n, skein_iv(nw), d_dig, nw == 8 ? 64 : 16, s)
                       : cw::sha256_launch(p, d_src, bb, stride, n, d_dig, s),
                    "hash launch");
}

int cw::host::dev_compress(int alg, const uint8_t *d_src, size_t bb, size_t stride, size_t n, uint8_t *d_dst, size_t dst_stride,
                           uint32_t *d_sizes, hipStream_t s, const cw::AfterScan *after_scan)
{
    if (alg == CW_COMP_NONE) return CW_OK;
    if (int rc = check_codec(alg)) return rc;
    if (bb == 0) return fail(CW_ERR_BAD_ARG, "compression needs block_bytes > 0");
    if (dst_stride < cw_compress_bound(alg, bb))
        return fail(CW_ERR_BAD_ARG, "dst_stride %zu < bound %zu", dst_stride, cw_compress_bound(alg, bb));
    ProfScope prof(PROF_CODEC, s);
    return launched(alg == CW_COMP_LZ4 ? cw::lz4_launch(d_src, bb, stride, n, d_dst, dst_stride, d_sizes, s, after_scan)
                                       : cw::lzf_launch(d_src, bb, stride, n, d_dst, dst_stride, d_sizes, s),
                    "compress launch");
}

namespace {
thread_local char t_kernels[2][320] = {"", ""};

[[noreturn]] void die(const char *what)
{
    fprintf(stderr, "libcwhc: %s failed: %s\n", what, t_err);
    abort();
}

} // namespace

// Tuning and test knobs (cw::Knobs).  This table is the only code that knows their names and how their values read; an unset knob
// keeps the field's initial value.  A knob's value is what cw_tune_set gave it, else the environment variable of the same name (read
// once, for the whole table, on first use).
namespace {
using cw::Knobs;
void positive(int &f, const char *v) { if (atoi(v) > 0) f = atoi(v); }
void positive(long &f, const char *v) { if (atol(v) > 0) f = atol(v); }

struct KnobDef { const char *name; void (*decode)(Knobs &k, const char *v); };
const KnobDef kKnobTable[] = {
    {"CW_SKEIN_SLICED", [](Knobs &k, const char *v) { k.skein_sliced = v[0] != '0'; }},
    {"CW_LZ4_LANES_FP", [](Knobs &k, const char *v) { k.lz4_lanes_fp = v[0] != '0'; }},
    {"CW_LZF_STHREAD", [](Knobs &k, const char *v) { k.lzf_sthread = v[0] != '0'; }},
    {"CW_SERIAL", [](Knobs &k, const char *v) { k.serial = v[0] == '1'; }},
    {"CW_DEBUG_HOST", [](Knobs &k, const char *v) { k.debug_host = v[0] == '1'; }},
    {"CW_PREPARE_COLD", [](Knobs &k, const char *v) { k.prepare_cold = v[0] == '1'; }},
    {"CW_FUSED_GATE", [](Knobs &k, const char *v) { k.fused_gate = v[0] == '1'; }},
    {"CW_HOST_SHARED_STREAMS", [](Knobs &k, const char *v) { k.host_shared_streams = v[0] == '1'; }},
    {"CW_LANES_CONCURRENT", [](Knobs &k, const char *v) { k.lanes_concurrent = v[0] != '0'; }},
    {"CW_SIDE_PRIO", [](Knobs &k, const char *v) { k.side_prio = v[0] == '0' ? cw::SidePrio::none : v[0] == '2' ? cw::SidePrio::both : cw::SidePrio::lanes; }},
    {"CW_LZ4_MODE", [](Knobs &k, const char *v) {
         k.lz4_mode = !strcmp(v, "scan") ? cw::Lz4Mode::scan : !strcmp(v, "generic") ? cw::Lz4Mode::generic
                    : !strcmp(v, "stream") ? cw::Lz4Mode::stream : !strcmp(v, "cut") ? cw::Lz4Mode::cut : cw::Lz4Mode::normal; }},
    {"CW_LZF_MODE", [](Knobs &k, const char *v) { k.lzf_mode = !strcmp(v, "cut") ? cw::LzfMode::cut : !strcmp(v, "table") ? cw::LzfMode::table : cw::LzfMode::normal; }},
    {"CW_SKEIN_MODE", [](Knobs &k, const char *v) { k.skein_mode = !strcmp(v, "steps") ? cw::SkeinMode::steps : cw::SkeinMode::lines; }},
    {"CW_LZ4_PARSE", [](Knobs &k, const char *v) { k.lz4_parse_fp = !strcmp(v, "fp"); }},
    {"CW_DEBUG_LZF", [](Knobs &k, const char *) { k.debug_lzf = true; }},
    {"CW_SCAN_WPC", [](Knobs &k, const char *v) { positive(k.scan_wpc, v); }},
    {"CW_PARSE_WPC", [](Knobs &k, const char *v) { positive(k.parse_wpc, v); }},
    {"CW_LANES_WPC", [](Knobs &k, const char *v) { positive(k.lanes_wpc, v); }},
    {"CW_LANES_RESERVE", [](Knobs &k, const char *v) { positive(k.lanes_reserve, v); }},
    {"CW_VTAB_WPC", [](Knobs &k, const char *v) { positive(k.vtab_wpc, v); }},
    {"CW_LZF_ST_WPC", [](Knobs &k, const char *v) { positive(k.lzf_st_wpc, v); }},
    {"CW_LZF_ROUND", [](Knobs &k, const char *v) { positive(k.lzf_round, v); }},
    {"CW_LZF_LDS_MAX", [](Knobs &k, const char *v) { positive(k.lzf_lds_max, v); }},
    {"CW_SKEIN_NSLICES", [](Knobs &k, const char *v) { positive(k.skein_nslices, v); }},
    {"CW_HOST_CHUNK_MB", [](Knobs &k, const char *v) { positive(k.host_chunk_mb, v); }},
    {"CW_HOST_BIG_CHUNK_MB", [](Knobs &k, const char *v) { positive(k.host_big_chunk_mb, v); }},
    {"CW_CDC_SEGMENT", [](Knobs &k, const char *v) { positive(k.cdc_segment, v); }},
    {"CW_STORE_PIECE", [](Knobs &k, const char *v) { positive(k.store_piece, v); }},
    {"CW_SCRUB_ENTRIES", [](Knobs &k, const char *v) { positive(k.scrub_entries, v); }},
    {"CW_DELTA_TILE", [](Knobs &k, const char *v) { positive(k.delta_tile, v); }},
    {"CW_LZ_FORCE_REDO", [](Knobs &k, const char *v) { k.force_redo = atoi(v) > 0; }},
    {"CW_LZF_SHARE_GIVE_UP", [](Knobs &k, const char *v) { k.lzf_share_give_up = atoi(v) > 0; }},
    {"CW_LZ4_LANES", [](Knobs &k, const char *v) { k.lz4_lanes = atoi(v); }},
    {"CW_LZF_LANES", [](Knobs &k, const char *v) { k.lzf_lanes = atoi(v); }},
    {"CW_DECODE_LANES", [](Knobs &k, const char *v) { k.decode_lanes = atoi(v); }},
    {"CW_LANES_LEAVE", [](Knobs &k, const char *v) { k.lanes_leave = atoi(v); }},
    {"CW_VTAB_MIN", [](Knobs &k, const char *v) { k.vtab_min = atoi(v); }},
    {"CW_VTAB_MAX", [](Knobs &k, const char *v) { k.vtab_max = atoi(v); }},
    {"CW_VTAB_RESERVE", [](Knobs &k, const char *v) { k.vtab_reserve = atoi(v); }},
    {"CW_LZ4_VTAB", [](Knobs &k, const char *v) { k.lz4_vtab = atoi(v); }},
    {"CW_LZ4_LANES_RING", [](Knobs &k, const char *v) { k.lz4_lanes_ring = atoi(v); }},
    {"CW_LZ4_HEADW", [](Knobs &k, const char *v) { k.lz4_headw = atoi(v); }},
    {"CW_LZ4_LTAB", [](Knobs &k, const char *v) { k.lz4_ltab = atoi(v); }},
    {"CW_VTAB_GEN", [](Knobs &k, const char *v) { k.vtab_gen = atoi(v); }},
    {"CW_LZ4_STAGE_MAX", [](Knobs &k, const char *v) { if (atoi(v) >= 0) k.lz4_stage_max = atoi(v); }},
};
constexpr size_t kKnobs = sizeof kKnobTable / sizeof kKnobTable[0];

struct KnobValue { bool set = false; std::string value; };
std::mutex tune_lock;
KnobValue tune_over[kKnobs], tune_env[kKnobs]; // cw_tune_set; the environment
bool tune_env_read = false;
} // namespace

cw::Knobs cw::knobs()
{
    Knobs k;
    std::lock_guard<std::mutex> g(tune_lock);
    if (!tune_env_read) {
        for (size_t i = 0; i < kKnobs; i++)
            if (const char *v = getenv(kKnobTable[i].name)) tune_env[i] = {true, v};
        tune_env_read = true;
    }
    for (size_t i = 0; i < kKnobs; i++) {
        const KnobValue &v = tune_over[i].set ? tune_over[i] : tune_env[i];
        if (v.set) kKnobTable[i].decode(k, v.value.c_str());
    }
    return k;
}

void cw::release_stream_workspaces(hipStream_t stream)
{
    (void)hipStreamSynchronize(stream); // nothing of the stream's may still use what is freed here
    for (cw::ScratchRegistry *r = cw::ScratchRegistry::head(); r; r = r->next) r->release(stream);
}

void cw::release_all_workspaces()
{
    for (cw::ScratchRegistry *r = cw::ScratchRegistry::head(); r; r = r->next) r->release_all();
}

void cw::note_kernels(int kind, const char *names)
{
    if (kind < 0 || kind > 1) return;
    strncpy(t_kernels[kind], names, sizeof t_kernels[kind] - 1);
    t_kernels[kind][sizeof t_kernels[kind] - 1] = 0;
}

extern "C" {

// ---- knobs (CW_TESTING section of the header) -------------------------------------------------------
int cw_tune_set(const char *key, const char *value)
{
    for (size_t i = 0; key && i < kKnobs; i++) {
        if (strcmp(kKnobTable[i].name, key) != 0) continue;
        std::lock_guard<std::mutex> g(tune_lock);
        tune_over[i] = value ? KnobValue{true, value} : KnobValue{};
        return CW_OK;
    }
    return fail(CW_ERR_BAD_ARG, "unknown knob %s", key ? key : "(null)");
}
void cw_tune_reset(void)
{
    std::lock_guard<std::mutex> g(tune_lock);
    for (KnobValue &o : tune_over) o = KnobValue{};
}

int cw_plan_describe(int comp_alg, size_t block_bytes, size_t nblocks, unsigned src_misalign, unsigned dst_misalign, char *buf, size_t cap)
{
    if (int bad = check_codec(comp_alg)) return bad;
    if (!(comp_alg == CW_COMP_LZ4 ? cw::lz4_call_valid(block_bytes, nblocks) : cw::lzf_call_valid(block_bytes, nblocks)))
        return fail(CW_ERR_BAD_ARG, "cw_plan_describe: %zu blocks of %zu bytes is not a call the codec accepts", nblocks, block_bytes);
    const cw::CodecCall call = {(uint32_t)block_bytes, nblocks, (unsigned)((src_misalign | block_bytes) & 15), (unsigned)((src_misalign | block_bytes) & 3), dst_misalign & 15};
    const cw::Knobs kn = cw::knobs();
    std::string text;
    if (nblocks == 0) text = "\n"; // (such a call launches nothing)
    else if (comp_alg == CW_COMP_LZ4) { const cw::Lz4Plan p = cw::lz4_plan(call, kn); text = std::string(cw::describe(p).text) + "\n" + cw::dump(p); }
    else { const cw::LzfPlan p = cw::lzf_plan(call, kn); text = std::string(cw::describe(p).text) + "\n" + cw::dump(p); }
    if (!buf || cap <= text.size()) return fail(CW_ERR_BAD_ARG, "cw_plan_describe: the text needs a buffer of %zu bytes", text.size() + 1);
    memcpy(buf, text.c_str(), text.size() + 1);
    return CW_OK;
}

int cw_hash_plan_describe(int hash_alg, size_t block_bytes, size_t nblocks, unsigned src_misalign, unsigned digest_misalign, int may_slice,
                          char *buf, size_t cap)
{
    const int nw = hash_state_words(hash_alg);
    if (nw < 0 && hash_alg != CW_HASH_NONE) return fail(CW_ERR_BAD_ARG, "unknown hash algorithm %d", hash_alg);
    if (int bad = check_block(block_bytes)) return bad;
    std::string text = "\n"; // (no blocks, no hash: such a call launches nothing)
    if (nblocks && nw >= 0) {
        const cw::HashPlan p = cw::hash_plan({nw, block_bytes, nblocks, src_misalign & 15, digest_misalign & 15, may_slice != 0}, cw::knobs());
        text = std::string(cw::describe(p).text) + "\n" + cw::dump(p);
    }
    if (!buf || cap <= text.size()) return fail(CW_ERR_BAD_ARG, "cw_hash_plan_describe: the text needs a buffer of %zu bytes", text.size() + 1);
    memcpy(buf, text.c_str(), text.size() + 1);
    return CW_OK;
}

// ---- lifecycle ------------------------------------------------------------------------------------
int cw_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int cw_init(int device)
{
    std::lock_guard<std::mutex> g(g_lock);
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) return fail(CW_ERR_NO_DEVICE, "no HIP device (%s)", hipGetErrorString(e));
    if (device < 0 || device >= n || device >= kMaxDevices) return fail(CW_ERR_BAD_ARG, "device %d out of range (count %d)", device, n);
    if (!((g_mask.load() >> device) & 1u)) {
        hipDeviceProp_t prop;
        HIP_TRY(hipGetDeviceProperties(&prop, device));
        if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
            return fail(CW_ERR_NO_DEVICE, "device %d is %s; libcwhc is built for gfx950 only", device, prop.gcnArchName);
        if (g_mask.load() == 0) {
            cw::skein_compute_iv(8, 512, &g_iv512_512);
            cw::skein_compute_iv(4, 128, &g_iv256_128);
        }
        g_mask.fetch_or(1u << device, std::memory_order_release);
        if (g_default.load() < 0) g_default.store(device, std::memory_order_release);
    }
    HIP_TRY(hipSetDevice(device));
    t_device = device; // the calling thread works on this device from now on
    return CW_OK;
}

int cw_set_device(int device) { return cw_init(device); }
int cw_get_device(void) { return current_device(); }

void cw_shutdown(void)
{
    cw_offload_thread_stop();
    std::lock_guard<std::mutex> g(g_lock);
    const uint32_t mask = g_mask.load();
    if (!mask) return;
    for (int d = 0; d < kMaxDevices; d++)
        if ((mask >> d) & 1u) {
            (void)hipSetDevice(d);
            (void)hipDeviceSynchronize();
        }
    cw::release_all_workspaces();
    g_mask.store(0);
    g_default.store(-1);
    t_device = -1;
}

const char *cw_last_error(void) { return t_err; }
const char *cw_version(void) { return "compute-war_amd 0.1 (gfx950)"; }

size_t cw_digest_bytes(int hash_alg)
{
    switch (hash_alg) {
    case CW_HASH_SKEIN512: return 64;
    case CW_HASH_SKEIN256_128: return 16;
    case CW_HASH_SHA256: return 32;
    default: return 0;
    }
}

size_t cw_compress_bound(int comp_alg, size_t l)
{
    if (comp_alg == CW_COMP_LZ4) return l + l / 255 + 16; // LZ4_compressBound (lz4.h:156); the reference's 2*l covers it for l >= 17
    if (comp_alg == CW_COMP_LZF) return l ? l : 1; // out_len = l-1 usable (:346)
    return 0;
}

void cw_set_block_size(size_t b) { g_block_size.store(b); }
size_t cw_get_block_size(void) { return g_block_size.load(); }

// ---- device-resident API ------------------------------------------------------------------------------
int cw_dev_hash(int hash_alg, const void *d_src, size_t block_bytes, size_t src_stride, size_t nblocks, void *d_digests,
                void *stream)
{
    int rc = ensure_init();
    if (rc != CW_OK) return rc;
    if (nblocks == 0) return CW_OK;
    if (!d_src || !d_digests) return fail(CW_ERR_BAD_ARG, "NULL device pointer");
    if ((rc = check_block(block_bytes)) != CW_OK) return rc;
    if (src_stride < block_bytes) return fail(CW_ERR_BAD_ARG, "src_stride < block_bytes");
    // long Skein messages in sliced launches here too: alone they are as fast as the one-launch kernel (46.6 ms per Mi blocks
    // either way, slightly ahead on small batches), and the hot kernel is then the same with and without a codec beside it
    return dev_hash(hash_alg, (const uint8_t *)d_src, block_bytes, src_stride, nblocks, (uint8_t *)d_digests, (hipStream_t)stream, true);
}

int cw_dev_compress(int comp_alg, const void *d_src, size_t block_bytes, size_t src_stride, size_t nblocks, void *d_dst,
                    size_t dst_stride, uint32_t *d_sizes, void *stream)
{
    int rc = ensure_init();
    if (rc != CW_OK) return rc;
    if (nblocks == 0) return CW_OK;
    if (!d_src || !d_dst || !d_sizes) return fail(CW_ERR_BAD_ARG, "NULL device pointer");
    if ((rc = check_block(block_bytes)) != CW_OK) return rc;
    if (src_stride < block_bytes) return fail(CW_ERR_BAD_ARG, "src_stride < block_bytes");
    return dev_compress(comp_alg, (const uint8_t *)d_src, block_bytes, src_stride, nblocks, (uint8_t *)d_dst, dst_stride, d_sizes,
                        (hipStream_t)stream);
}

// ProcessBlock (:243-257) compresses, then hashes; the two only share their read-only input, so they run side by
// side: the codec (latency/memory bound, few issue slots, persistent grid) goes first on the caller's stream so its
// workgroups are resident before the hash (pure integer VALU, one long-lived wavefront per 64 blocks) fills the rest of
// every CU from the context's low-priority side stream; the side stream is joined before the call's work counts as done.
static int dev_fused(cw::SideStream &side_s, int hash_alg, int comp_alg, const uint8_t *d_src, size_t block_bytes, size_t src_stride, size_t nblocks,
                     uint8_t *d_digests, uint8_t *d_dst, size_t dst_stride, uint32_t *d_sizes, hipStream_t main_s)
{
    int rc;
    const cw::Knobs kn = cw::knobs();
    if (kn.serial) { // CW_SERIAL=1: both kernels on the caller's stream (profiling knob)
        rc = dev_compress(comp_alg, d_src, block_bytes, src_stride, nblocks, d_dst, dst_stride, d_sizes, main_s);
        return rc == CW_OK ? dev_hash(hash_alg, d_src, block_bytes, src_stride, nblocks, d_digests, main_s, true) : rc;
    }
    cw::SideStream::Fork fork(side_s, main_s); // (a return before the join below still joins)
    HIP_TRY(fork.err);
    const hipStream_t side = side_s.stream;
    // Side by side pays when the codec is light -- incompressible input, where it is the scan alone (the headline: 61.7 ms against 72.9 one after
    // the other).  On compressible input the parsers fill every CU with wavefronts that stay until the queue is empty; a hash kernel that arrives
    // beside them trickles in behind, ends with the call and costs the parsers more than it takes alone (Skein-256 over 1 Mi blocks of 4 KiB:
    // 3.5 ms alone, but the fused call 97.7 ms against 84.8 one after the other; 51,728 blocks 8.7 against 6.8 ms).  Which input a call has is known
    // on the device only -- but calls come in streams of alike ones, so the LAST LZ4 call's queued share decides (copied back asynchronously, used
    // when it has arrived): a quarter or more of the blocks queued, at least 16 Ki blocks (fewer leave CUs idle for the hash anyway), and blocks of
    // at most 4 KiB => the hash is enqueued right behind the scan, runs beside it, and the PARSERS WAIT FOR IT.  Measured, fused call gated / not:
    // Skein-256 + LZ4, 1 Mi blocks of 4 KiB 93.3 / 104.2 ms, SHA-256 + LZ4 92.2 / 101.6, 51,728 blocks 7.15 / 7.55; blocks of 64 KiB, where the
    // scalar-thread parsers leave the vector ALUs to the hash: 64 Ki blocks 94.8 / 91.1 ms, the mix 43.4 / 42.2, 256 Ki blocks 370.6 / 372.0 -- so
    // those stay side by side.  (Always gating costs the headline 2.7 ms: its empty-queue parser and redo launches then run behind the hash.)
    struct Gate { int hash_alg; const uint8_t *src; size_t bb, stride, n; uint8_t *dig; hipStream_t side; cw::SideStream::Fork *fork; int rc; bool called; };
    Gate gate = {hash_alg, d_src, block_bytes, src_stride, nblocks, d_digests, side, &fork, CW_OK, false};
    const cw::AfterScan hook = {[](void *p) -> hipError_t {
                                    Gate *g = static_cast<Gate *>(p);
                                    g->called = true;
                                    g->rc = dev_hash(g->hash_alg, g->src, g->bb, g->stride, g->n, g->dig, g->side, true);
                                    return g->rc != CW_OK ? hipErrorUnknown : g->fork->join();
                                }, &gate};
    ThreadCtx *tc = nullptr;
    FusedHint *hint = comp_alg == CW_COMP_LZ4 && thread_ctx(&tc) == CW_OK ? &tc->hint : nullptr;
    if (hint && hint->pending) {
        const hipError_t q = hipEventQuery(hint->ev);
        if (q == hipSuccess) {
            hint->pending = false;
            if (hint->blocks_of_copy) hint->queued_share = (float)*hint->h_queued / (float)hint->blocks_of_copy;
        } else if (q == hipErrorNotReady) {
            (void)hipGetLastError(); // (not an error; any other pending error stays for whoever asks next)
        }
    }
    // CW_FUSED_GATE: 0 = never, 1 = always (profiling knob)
    const bool gated = hint && (kn.fused_gate ? *kn.fused_gate : block_bytes <= 4096 && nblocks >= 16384 && hint->queued_share >= 0.25f);
    rc = dev_compress(comp_alg, d_src, block_bytes, src_stride, nblocks, d_dst, dst_stride, d_sizes, main_s, gated ? &hook : nullptr);
    if (gate.called && gate.rc != CW_OK) return gate.rc;
    if (rc == CW_OK && !gate.called) rc = dev_hash(hash_alg, d_src, block_bytes, src_stride, nblocks, d_digests, side, true);
    HIP_TRY(fork.join());
    if (rc == CW_OK && hint && !hint->pending) { // this call's queued share, for the next call
        const uint32_t *word = cw::lz4_queued_blocks_word(main_s);
        if (word) {
            if (!hint->h_queued) HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&hint->h_queued), 64, hipHostMallocDefault));
            if (!hint->ev) HIP_TRY(hipEventCreateWithFlags(&hint->ev, hipEventDisableTiming));
            HIP_TRY(hipMemcpyAsync(hint->h_queued, word, sizeof(uint32_t), hipMemcpyDeviceToHost, main_s));
            HIP_TRY(hipEventRecord(hint->ev, main_s));
            hint->pending = true;
            hint->blocks_of_copy = nblocks;
        }
    }
    return rc;
}

int cw_dev_hash_and_compress(int hash_alg, int comp_alg, const void *d_src, size_t block_bytes, size_t src_stride,
                             size_t nblocks, void *d_digests, void *d_dst, size_t dst_stride, uint32_t *d_sizes, void *stream)
{
    if (comp_alg == CW_COMP_NONE) return cw_dev_hash(hash_alg, d_src, block_bytes, src_stride, nblocks, d_digests, stream);
    if (hash_alg == CW_HASH_NONE)
        return cw_dev_compress(comp_alg, d_src, block_bytes, src_stride, nblocks, d_dst, dst_stride, d_sizes, stream);
    ThreadCtx *c;
    int rc = thread_ctx(&c);
    if (rc != CW_OK) return rc;
    if (nblocks == 0) return CW_OK;
    if (!d_src || !d_dst || !d_sizes || !d_digests) return fail(CW_ERR_BAD_ARG, "NULL device pointer");
    if ((rc = check_block(block_bytes)) != CW_OK) return rc;
    if (src_stride < block_bytes) return fail(CW_ERR_BAD_ARG, "src_stride < block_bytes");
    return dev_fused(c->side, hash_alg, comp_alg, (const uint8_t *)d_src, block_bytes, src_stride, nblocks, (uint8_t *)d_digests, (uint8_t *)d_dst,
                     dst_stride, d_sizes, (hipStream_t)stream);
}

int cw_dev_decompress(int comp_alg, const void *d_comp, size_t comp_stride, const uint32_t *d_sizes, size_t nblocks, void *d_dst,
                      size_t block_bytes, uint32_t *d_status, void *stream)
{
    int rc = ensure_init();
    if (rc != CW_OK) return rc;
    if (nblocks == 0) return CW_OK;
    if (!d_comp || !d_sizes || !d_dst || !d_status) return fail(CW_ERR_BAD_ARG, "NULL device pointer");
    if (int bad = check_codec(comp_alg)) return bad;
    if (block_bytes == 0 || (rc = check_block(block_bytes)) != CW_OK) return rc ? rc : fail(CW_ERR_BAD_ARG, "block_bytes == 0");
    return launched(cw::decompress_launch(comp_alg == CW_COMP_LZ4 ? 0 : 1, (const uint8_t *)d_comp, comp_stride, d_sizes, nblocks,
                                         (uint8_t *)d_dst, block_bytes, d_status, (hipStream_t)stream), "decompress launch");
}

int cw_dev_hash_tree(int hash_alg, const void *d_src, size_t block_bytes, size_t src_stride, size_t nblocks, unsigned leaf, unsigned node,
                     unsigned max_level, void *d_digests, void *stream)
{
    int rc = ensure_init();
    if (rc != CW_OK) return rc;
    if (nblocks == 0) return CW_OK;
    if (!d_src || !d_digests) return fail(CW_ERR_BAD_ARG, "NULL device pointer");
    if ((rc = check_block(block_bytes)) != CW_OK) return rc;
    if (hash_alg != CW_HASH_SKEIN512 && hash_alg != CW_HASH_SKEIN256_128) return fail(CW_ERR_BAD_ARG, "tree hashing is defined for the Skein algorithms only");
    hipError_t e = cw::skein_tree_launch(hash_alg == CW_HASH_SKEIN512 ? 8 : 4, (const uint8_t *)d_src, block_bytes,
                                         src_stride ? src_stride : block_bytes, nblocks, hash_alg == CW_HASH_SKEIN512 ? 512u : 128u, leaf,
                                         node, max_level, (uint8_t *)d_digests, (hipStream_t)stream);
    if (e == hipErrorInvalidValue) return fail(CW_ERR_BAD_ARG, "tree parameters leaf=%u node=%u maxLevel=%u not usable for %zu-byte blocks", leaf, node, max_level, block_bytes);
    return launched(e, "tree hash launch");
}

int cw_dev_pack(const void *d_slots, size_t slot_stride, const uint32_t *d_sizes, size_t nblocks, void *d_packed, uint64_t *d_offsets,
                void *stream)
{
    int rc = ensure_init();
    if (rc != CW_OK) return rc;
    if (!d_offsets || (nblocks && (!d_sizes || (d_packed && !d_slots)))) return fail(CW_ERR_BAD_ARG, "NULL device pointer");
    return launched(cw::pack_launch((const uint8_t *)d_slots, slot_stride, d_sizes, nblocks, (uint8_t *)d_packed, d_offsets,
                                   (hipStream_t)stream), "pack launch");
}

static int dev_gen(bool mixed, uint64_t seed, uint64_t first_block, size_t nblocks, size_t block_bytes, void *d_dst, hipStream_t s)
{
    if (int rc = ensure_init()) return rc;
    if (!d_dst) return fail(CW_ERR_BAD_ARG, "NULL device pointer");
    if (block_bytes % 16 || block_bytes > CW_MAX_BLOCK_BYTES) return fail(CW_ERR_BAD_ARG, "block_bytes must be a multiple of 16, <= 65536");
    return launched(mixed ? cw::gen_mixed_launch(seed, first_block, nblocks, block_bytes, (uint8_t *)d_dst, s)
                          : cw::gen_random_launch(seed, first_block, nblocks, block_bytes, (uint8_t *)d_dst, s),
                    "gen launch");
}
int cw_dev_gen_random(uint64_t seed, uint64_t first_block, size_t nblocks, size_t block_bytes, void *d_dst, void *stream)
{
    return dev_gen(false, seed, first_block, nblocks, block_bytes, d_dst, (hipStream_t)stream);
}
int cw_dev_gen_mixed(uint64_t seed, uint64_t first_block, size_t nblocks, size_t block_bytes, void *d_dst, void *stream)
{
    return dev_gen(true, seed, first_block, nblocks, block_bytes, d_dst, (hipStream_t)stream);
}

int cw_dev_sum_sizes(const uint32_t *d_sizes, size_t nblocks, uint32_t raw_bytes, uint64_t *d_totals, void *stream)
{
    int rc = ensure_init();
    if (rc != CW_OK) return rc;
    if (!d_sizes || !d_totals) return fail(CW_ERR_BAD_ARG, "NULL device pointer");
    return launched(cw::sum_sizes_launch(d_sizes, nblocks, raw_bytes, d_totals, (hipStream_t)stream), "sum launch");
}

// plain device memory for C callers of the cw_dev_* functions (the host programs link no HIP runtime themselves)
void *cw_dev_alloc(size_t bytes)
{
    if (ensure_init() != CW_OK) return nullptr;
    void *p = nullptr;
    hipError_t e = hipMalloc(&p, bytes ? bytes : 1);
    if (e != hipSuccess) { fail(CW_ERR_NOMEM, "hipMalloc(%zu): %s", bytes, hipGetErrorString(e)); return nullptr; }
    return p;
}
void cw_dev_free(void *d_p) { if (d_p) (void)hipFree(d_p); }
int cw_dev_upload(void *d_dst, const void *src, size_t bytes)
{
    int rc = ensure_init();
    if (rc != CW_OK) return rc;
    HIP_TRY(hipMemcpy(d_dst, src, bytes, hipMemcpyHostToDevice));
    return CW_OK;
}
int cw_dev_download(void *dst, const void *d_src, size_t bytes)
{
    int rc = ensure_init();
    if (rc != CW_OK) return rc;
    HIP_TRY(hipMemcpy(dst, d_src, bytes, hipMemcpyDeviceToHost));
    return CW_OK;
}
int cw_dev_synchronize(void)
{
    int rc = ensure_init();
    if (rc != CW_OK) return rc;
    HIP_TRY(hipDeviceSynchronize());
    return CW_OK;
}

#ifdef CW_CLOCK_STAMP
// diagnostic build only (tools/clock_probe.py): the in-kernel clock stamps of the last launches
int cw_debug_clock_read(int which, unsigned long long *out)
{
    int rc = ensure_init();
    if (rc != CW_OK) return rc;
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(which == 0 ? cw::skein_clock_read(out) : cw::lz4_clock_read(out));
    return CW_OK;
}
#endif

void cw_profile_enable(int on) { t_prof_on = on != 0; }

int cw_profile_read(double ms_sum[3], unsigned count[3], int reset)
{
    for (int k = 0; k < PROF_KINDS; k++) { ms_sum[k] = 0; count[k] = 0; }
    for (ProfSpan &p : t_prof) {
        float ms = 0;
        HIP_TRY(hipEventSynchronize(p.b));
        HIP_TRY(hipEventElapsedTime(&ms, p.a, p.b));
        ms_sum[p.kind] += ms;
        count[p.kind]++;
    }
    if (reset) {
        for (ProfSpan &p : t_prof) { (void)hipEventDestroy(p.a); (void)hipEventDestroy(p.b); }
        t_prof.clear();
    }
    return CW_OK;
}

int cw_profile_kernels(int kind, char *buf, size_t cap)
{
    if (kind < 0 || kind > 1 || !buf || cap == 0) return fail(CW_ERR_BAD_ARG, "cw_profile_kernels: kind 0 (codec) or 1 (hash), a buffer");
    strncpy(buf, t_kernels[kind], cap - 1);
    buf[cap - 1] = 0;
    return CW_OK;
}

// ---- batched host API ------------------------------------------------------------------------------------
// The pipelined batch path: what HashOffload::Start() ("xfer data, load kernel") and Complete() ("wait for and reap the
// results", HashOffload.h:26-40) were meant to be, for a whole batch.  The batch is cut into chunks and three of them are
// in flight at any time, each in a Slot with its own device buffers, pinned staging and streams:
//   s_h2d      chunk k+1 crosses the bus host -> device
//   slot.stream / slot.side   chunk k: codec and hash side by side, then the slots are packed into one stream on the device
//              (pack_kernels.hip) so that only the compressed bytes cross the bus back; sizes, the total and the digests
//              follow on the same stream
//   s_d2h      chunk k-1's packed payload crosses device -> host
//   host       meanwhile the calling thread moves chunk k-2's payload from pinned staging into the caller's slots.
// Host memory the copy engines touch directly must be page-locked: a caller's buffer that is (cw_host_alloc /
// cw_host_register) is used in place, anything else goes through the slot's pinned staging with one memcpy.
namespace {
struct HostJob {
    int hash_alg, comp_alg;
    const uint8_t *src; size_t bb, nblocks;
    uint8_t *digests; uint8_t *dst; size_t dst_stride; uint32_t *sizes;
    uint8_t *packed; size_t packed_cap; uint64_t *offsets; // packed-output form (dst == NULL)
    bool do_hash, do_comp, src_pinned, packed_pinned;
    size_t db, d_stride;
    uint64_t packed_off;
};

size_t meta_off_total(size_t n) { return (n * 4 + 7) & ~(size_t)7; }
size_t meta_off_dig(size_t n) { return meta_off_total(n) + 8; }

int slot_reserve(HostJob &j, Slot &s, size_t n, bool stage_src, bool stage_pack, const Slot *lender = nullptr);

// The slots of a thread's pipeline share ONE pair of kernel streams (the first slot's) unless the job's codec is LZF (CW_HOST_SHARED_STREAMS=0|1
// forces either; decided when a slot is first opened).  HIP multiplexes streams onto four hardware queues per priority level, and kernels -- and the
// small device-to-host copies of a chunk's sizes and digests -- that land on one queue wait for each other: with a stream pair per slot (plus the
// codec's side streams per slot stream) the pipeline had sixteen streams, and its timeline showed a chunk's copies and kernels waiting behind
// another chunk's long kernels.  The chunks' kernels do not gain from overlapping each other anyway.  8 GiB through
// cw_hash_and_compress_packed, own streams -> shared: corpus, Skein-512 + LZ4, 64 KiB 24.1 -> 26.0 GB/s; Skein-256 + LZ4, 4 KiB 22.6 -> 33.4;
// SHA-256 + LZ4, 4 KiB 23.0 -> 33.5; noise 41.4 -> 43.6; SHA-256 + LZF, 4 KiB 25.5 -> 25.6, 64 KiB 17.6 -> 15.9 (its rounds of link and parse
// kernels do overlap across chunks).
const Slot *shared_lender(const cw::Knobs &kn, ThreadCtx &c, const HostJob &j, const Slot &s)
{
    const bool share = kn.host_shared_streams ? *kn.host_shared_streams : j.comp_alg != CW_COMP_LZF;
    if (!share || &s == &c.slot[0]) return nullptr;
    return c.slot[0].open() == CW_OK ? &c.slot[0] : nullptr;
}

// the kernels of a chunk of n blocks in the slot's device buffers: codec and hash, then the pack of the slots (a hash-only job has no
// slots, sizes or packed stream to touch)
int slot_kernels(const HostJob &j, Slot &s, size_t n)
{
    int rc;
    if (j.do_comp && j.do_hash)
        rc = dev_fused(s.side, j.hash_alg, j.comp_alg, (const uint8_t *)s.src.p, j.bb, j.bb, n, (uint8_t *)s.dig.p, (uint8_t *)s.dst.p,
                       j.d_stride, (uint32_t *)s.sizes.p, s.stream);
    else if (j.do_comp)
        rc = dev_compress(j.comp_alg, (const uint8_t *)s.src.p, j.bb, j.bb, n, (uint8_t *)s.dst.p, j.d_stride, (uint32_t *)s.sizes.p, s.stream);
    else
        rc = dev_hash(j.hash_alg, (const uint8_t *)s.src.p, j.bb, j.bb, n, (uint8_t *)s.dig.p, s.stream, true);
    if (rc != CW_OK || !j.do_comp) return rc;
    return launched(cw::pack_launch((const uint8_t *)s.dst.p, j.d_stride, (const uint32_t *)s.sizes.p, n, (uint8_t *)s.pack.p, (uint64_t *)s.offs.p, s.stream),
                    "pack launch");
}

int pipe_issue(const cw::Knobs &kn, ThreadCtx &c, HostJob &j, Slot &s, size_t first, size_t n)
{
    int rc = slot_reserve(j, s, n, !j.src_pinned, !(j.packed && j.packed_pinned), shared_lender(kn, c, j, s));
    if (rc != CW_OK) return rc;
    s.first = first; s.n = n; s.total = 0;
    const size_t bytes = n * j.bb;
    const uint8_t *hsrc = j.src + first * j.bb;
    if (!j.src_pinned && bytes) {
        memcpy(s.h_src.p, hsrc, bytes);
        hsrc = (const uint8_t *)s.h_src.p;
    }
    if (bytes) HIP_TRY(hipMemcpyAsync(s.src.p, hsrc, bytes, hipMemcpyHostToDevice, c.s_h2d));
    HIP_TRY(hipEventRecord(s.ev_h2d, c.s_h2d));
    HIP_TRY(hipStreamWaitEvent(s.stream, s.ev_h2d, 0));
    uint8_t *meta = (uint8_t *)s.h_meta.p;
    if ((rc = slot_kernels(j, s, n)) != CW_OK) return rc;
    if (j.do_comp) {
        HIP_TRY(hipMemcpyAsync(meta, s.sizes.p, n * 4, hipMemcpyDeviceToHost, s.stream));
        HIP_TRY(hipMemcpyAsync(meta + meta_off_total(n), (const uint64_t *)s.offs.p + n, 8, hipMemcpyDeviceToHost, s.stream));
    }
    if (j.do_hash) HIP_TRY(hipMemcpyAsync(meta + meta_off_dig(n), s.dig.p, n * j.db, hipMemcpyDeviceToHost, s.stream));
    HIP_TRY(hipEventRecord(s.ev_meta, s.stream));
    return CW_OK;
}

// sizes, total and digests of the slot's chunk are on the host: hand them out and start the payload's way back
int pipe_reap(ThreadCtx &c, HostJob &j, Slot &s)
{
    HIP_TRY(hipEventSynchronize(s.ev_meta));
    const uint8_t *meta = (const uint8_t *)s.h_meta.p;
    const size_t n = s.n;
    if (j.do_hash) memcpy(j.digests + s.first * j.db, meta + meta_off_dig(n), n * j.db);
    if (j.do_comp) {
        const uint32_t *sz = (const uint32_t *)meta;
        memcpy(j.sizes + s.first, sz, n * 4);
        memcpy(&s.total, meta + meta_off_total(n), 8);
        if (j.dst) {
            for (size_t i = 0; i < n; i++)
                if (sz[i] > j.dst_stride) return fail(CW_ERR_BAD_ARG, "block %zu: %u bytes exceed dst_stride %zu", s.first + i, sz[i], j.dst_stride);
        } else {
            if (j.packed_off + s.total > j.packed_cap)
                return fail(CW_ERR_BAD_ARG, "packed stream needs more than the %zu bytes provided", j.packed_cap);
            uint64_t o = j.packed_off;
            for (size_t i = 0; i < n; i++) { j.offsets[s.first + i] = o; o += sz[i]; }
        }
        HIP_TRY(hipStreamWaitEvent(c.s_d2h, s.ev_meta, 0));
        if (s.total) {
            void *to = j.packed && j.packed_pinned ? (void *)(j.packed + j.packed_off) : s.h_pack.p;
            HIP_TRY(hipMemcpyAsync(to, s.pack.p, s.total, hipMemcpyDeviceToHost, c.s_d2h));
        }
        HIP_TRY(hipEventRecord(s.ev_payload, c.s_d2h));
        if (!j.dst) { s.first = (size_t)j.packed_off; j.packed_off += s.total; } // first now = the chunk's place in the packed stream
    }
    return CW_OK;
}

// the payload of the slot's chunk is in pinned staging: move it to where the caller wants it
int pipe_finish(HostJob &j, Slot &s)
{
    if (!j.do_comp) return CW_OK;
    HIP_TRY(hipEventSynchronize(s.ev_payload));
    if (!s.total) return CW_OK;
    const uint8_t *from = (const uint8_t *)s.h_pack.p;
    if (j.dst) {
        const uint32_t *sz = (const uint32_t *)s.h_meta.p; // still this chunk's: the slot is not reused before this returns
        for (size_t i = 0; i < s.n; i++) {
            memcpy(j.dst + (s.first + i) * j.dst_stride, from, sz[i]);
            from += sz[i];
        }
    } else if (!j.packed_pinned) {
        memcpy(j.packed + s.first, from, s.total);
    }
    return CW_OK;
}

void pipe_drain(ThreadCtx &c)
{
    (void)hipStreamSynchronize(c.s_h2d);
    for (Slot &s : c.slot) { if (s.stream) { (void)hipStreamSynchronize(s.stream); (void)hipStreamSynchronize(s.side.stream); } }
    (void)hipStreamSynchronize(c.s_d2h);
}

// chunk: a chunk's kernels cost 8-10 ms almost whatever its size (a 64 KiB Skein block is a serial chain of 1,025 steps, 8 hash
// launches of ~0.5 ms each even for a few thousand blocks, plus scan / parse / pack launches), and the kernels of successive
// chunks do not overlap each other in practice (rocprofv3 timeline; more hardware queues -- GPU_MAX_HW_QUEUES -- did not
// change that and made 4 KiB blocks 7x slower).  So a chunk of large blocks must carry enough bytes for that time to hide
// behind its own host->device copy: 64 / 128 / 256 / 512 MiB measured 21.7 / 27.8 / 28.0 / 45.7 GB/s on random 64 KiB blocks
// (the last is the link's duplex rate).  Three slots x (input + slots + packed stream) = 4.6 GiB of device memory per calling
// thread at 512 MiB.  CW_HOST_CHUNK_MB overrides.
size_t pipeline_chunk(const cw::Knobs &kn, size_t bb, size_t nblocks)
{
    // 512 MiB: the chunk's kernels cost 8-10 ms whatever its size and do not overlap across chunks, and a chunk of 4 KiB blocks has
    // to be large enough for the lane parsers to run beside the LDS-resident ones (8 GiB of 4 KiB corpus blocks, Skein-256 + LZ4 /
    // SHA-256 + LZF: chunks of 64 MiB 29.5 / 18.8 GB/s, 512 MiB 38.6 / 27.2, 1 GiB 40.0 / 20.8; random data 47 -> 45-47 GB/s)
    size_t chunk_bytes = kn.host_chunk_mb ? (size_t)kn.host_chunk_mb << 20 : (size_t)512 << 20;
    size_t chunk = chunk_bytes / (bb ? bb : 1);
    if (chunk == 0) chunk = 1;
    if (chunk > nblocks) chunk = nblocks;
    if (nblocks > chunk && nblocks < 3 * chunk) chunk = (nblocks + 2) / 3; // a small batch still gets three stages
    return chunk ? chunk : 1;
}

// device buffers, pinned staging, streams and events of one slot for chunks of n blocks (idempotent; grows only)
int slot_reserve(HostJob &j, Slot &s, size_t n, bool stage_src, bool stage_pack, const Slot *lender)
{
    int rc = s.open(lender);
    if (rc != CW_OK) return rc;
    if ((rc = s.src.reserve(n * j.bb + 16)) != CW_OK) return rc;
    if (j.do_hash && (rc = s.dig.reserve(n * j.db)) != CW_OK) return rc;
    if (j.do_comp && ((rc = s.dst.reserve(n * j.d_stride)) != CW_OK || (rc = s.sizes.reserve(n * 4)) != CW_OK ||
                      (rc = s.pack.reserve(n * j.d_stride)) != CW_OK || (rc = s.offs.reserve((n + 1) * 8)) != CW_OK))
        return rc;
    if ((rc = s.h_meta.reserve(meta_off_dig(n) + n * j.db)) != CW_OK) return rc;
    if (j.do_comp && stage_pack && (rc = s.h_pack.reserve(n * j.d_stride)) != CW_OK) return rc;
    if (stage_src && n * j.bb && (rc = s.h_src.reserve(n * j.bb)) != CW_OK) return rc;
    return CW_OK;
}

// Chunks of compressible blocks > 4 KiB grow once the first results are in.  A 512 MiB chunk is 8,192 blocks of 64 KiB: the regime of the
// wavefront-per-block parsers (13 GB/s LZ4, 8.5 GB/s LZF on text), and the codec, not the link, bounds the call.  2 GiB are 32 Ki blocks,
// which the lane parsers take (the number of blocks in a call): 8 GiB of the corpus in page-locked memory, Skein-512 + LZ4
// 23.0 -> 31.0 GB/s, SHA-256 + LZF 11.4 -> 24.5.  Noise stays with 512 MiB (45.7 GB/s; 40.5 with 2 GiB chunks: fill and drain).  Only
// with the caller's buffers page-locked (no 2 GiB of staging per slot) and CW_HOST_CHUNK_MB unset; 18.5 GiB of device memory per calling
// thread once grown.
constexpr size_t kBigChunkBytes = (size_t)2 << 30;

// blocks of a grown chunk, or 0 when chunks of this job never grow
size_t grown_chunk(const cw::Knobs &kn, const HostJob &j, size_t chunk, bool pinned_io)
{
    // CW_HOST_BIG_CHUNK_MB (test knob): the grown chunk's size, and growth although CW_HOST_CHUNK_MB is set
    const size_t big = (kn.host_big_chunk_mb ? (size_t)kn.host_big_chunk_mb << 20 : kBigChunkBytes) / (j.bb ? j.bb : 1);
    const bool may = (kn.host_big_chunk_mb || !kn.host_chunk_mb) && j.do_comp && j.bb > 4096 && pinned_io && big > chunk;
    return may ? big : 0;
}

// grown chunks need 3 x (input + slots + packed stream) of device memory per calling thread: only when the device has it to spare
// (many host threads on one device each run a pipeline of their own)
bool room_to_grow(const ThreadCtx &c, const HostJob &j, size_t big)
{
    if (c.slot[0].src.buf.bytes() >= big * j.bb && c.slot[kSlots - 1].src.buf.bytes() >= big * j.bb) return true; // grown before
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) { (void)hipGetLastError(); return false; }
    // + the lane parsers' tables on each slot stream (LZ4 4 GiB, LZF 8 GiB at most; lz4_kernel.hip / lzf_kernel.hip allocate them on the first
    //   large chunk and fall back to the parsers without lanes when the device cannot give them)
    const size_t lane_tabs = kSlots * (j.comp_alg == CW_COMP_LZF ? (size_t)8 << 30 : (size_t)4 << 30);
    const size_t need = kSlots * big * (j.bb + 2 * j.d_stride + 64) + lane_tabs;
    return free_b > need + ((size_t)16 << 30);
}

int host_pipeline(HostJob &j)
{
    ThreadCtx *cp;
    int rc = thread_ctx(&cp);
    if (rc != CW_OK) return rc;
    ThreadCtx &c = *cp;
    if (j.nblocks == 0 || (!j.do_hash && !j.do_comp)) { if (j.offsets) j.offsets[0] = 0; return CW_OK; }
    const cw::Knobs kn = cw::knobs();
    const size_t chunk = pipeline_chunk(kn, j.bb, j.nblocks);
    j.src_pinned = is_pinned(j.src);
    j.packed_pinned = j.packed && is_pinned(j.packed);
    j.packed_off = 0;
    const size_t big = grown_chunk(kn, j, chunk, j.src_pinned && j.packed_pinned);
    const bool may_grow = big != 0 && j.nblocks > 2 * chunk && room_to_grow(c, j, big);
    size_t next = 0, issued = 0, seen_in = 0, seen_out = 0; // blocks handed out; chunks issued; bytes in / out of the chunks reaped so far
    for (size_t k = 0; rc == CW_OK && (next < j.nblocks || k < issued + 2); k++) {
        if (next < j.nblocks) {
            const size_t left = j.nblocks - next;
            size_t n = left < chunk ? left : chunk;
            if (may_grow && seen_in && seen_in / 10 * 9 >= seen_out && left > chunk) // compressible so far (>= 10 % saved)
                n = left >= 2 * big ? big : left > big ? (left + 1) / 2 : left;
            if (kn.debug_host) fprintf(stderr, "cw host pipeline: chunk %zu = %zu blocks of %zu B\n", issued, n, j.bb); // (tests)
            rc = pipe_issue(kn, c, j, c.slot[k % kSlots], next, n);
            next += n;
            issued++;
        }
        if (rc == CW_OK && k >= 1 && k - 1 < issued) {
            Slot &s = c.slot[(k - 1) % kSlots];
            rc = pipe_reap(c, j, s);
            seen_in += s.n * j.bb;
            seen_out += s.total;
            if (may_grow) { // a block that did not fit (LZF: size 0) is kept raw by the caller: it counts as not compressed
                const uint32_t *sz = (const uint32_t *)s.h_meta.p;
                size_t raw = 0;
                for (size_t i = 0; i < s.n; i++) raw += sz[i] == 0;
                seen_out += raw * j.bb;
            }
        }
        if (rc == CW_OK && k >= 2 && k - 2 < issued) rc = pipe_finish(j, c.slot[(k - 2) % kSlots]);
    }
    if (rc != CW_OK) { pipe_drain(c); return rc; }
    if (j.offsets) j.offsets[j.nblocks] = j.packed_off;
    return CW_OK;
}

int host_job_init(HostJob &j, int hash_alg, int comp_alg, const void *src, size_t block_bytes, size_t nblocks, void *digests, bool want_comp)
{
    memset(&j, 0, sizeof j);
    j.hash_alg = hash_alg; j.comp_alg = comp_alg; j.src = (const uint8_t *)src; j.bb = block_bytes; j.nblocks = nblocks;
    j.digests = (uint8_t *)digests;
    j.do_hash = hash_alg != CW_HASH_NONE && digests != nullptr;
    j.do_comp = comp_alg != CW_COMP_NONE && want_comp;
    if (nblocks == 0 || (!j.do_hash && !j.do_comp)) return CW_OK;
    if (!src && block_bytes) return fail(CW_ERR_BAD_ARG, "NULL src");
    int rc = check_block(block_bytes);
    if (rc != CW_OK) return rc;
    j.db = cw_digest_bytes(hash_alg);
    if (j.do_hash && j.db == 0) return fail(CW_ERR_BAD_ARG, "unknown hash algorithm %d", hash_alg);
    const size_t bound = j.do_comp ? cw_compress_bound(comp_alg, block_bytes) : 0;
    if (j.do_comp && bound == 0) return fail(CW_ERR_BAD_ARG, "unknown compression algorithm %d", comp_alg);
    if (j.do_comp && block_bytes == 0) return fail(CW_ERR_BAD_ARG, "compression needs block_bytes > 0");
    // The caller's slot may be the reference's (2*l for lz4, l-1 for lzf, :234-239); device slots use the bound.
    j.d_stride = (bound + 15) & ~(size_t)15;
    return CW_OK;
}
} // namespace

int cw_hash_and_compress_blocks(int hash_alg, int comp_alg, const void *src, size_t block_bytes, size_t nblocks, void *digests,
                                void *dst, size_t dst_stride, uint32_t *sizes)
{
    HostJob j;
    int rc = host_job_init(j, hash_alg, comp_alg, src, block_bytes, nblocks, digests, dst != nullptr && sizes != nullptr);
    if (rc != CW_OK) return rc;
    j.dst = (uint8_t *)dst; j.dst_stride = dst_stride; j.sizes = sizes;
    return host_pipeline(j);
}

int cw_hash_and_compress_packed(int hash_alg, int comp_alg, const void *src, size_t block_bytes, size_t nblocks, void *digests,
                                void *packed, size_t packed_cap, uint64_t *offsets, uint32_t *sizes)
{
    if (int bad = check_codec(comp_alg)) return bad;
    if (nblocks && (!packed || !offsets || !sizes)) return fail(CW_ERR_BAD_ARG, "NULL packed/offsets/sizes");
    HostJob j;
    int rc = host_job_init(j, hash_alg, comp_alg, src, block_bytes, nblocks, digests, true);
    if (rc != CW_OK) return rc;
    j.packed = (uint8_t *)packed; j.packed_cap = packed_cap; j.offsets = offsets; j.sizes = sizes;
    return host_pipeline(j);
}

// initializeGpu() (HashAndCompress.cpp:95-98) for the calling thread: its context on its device and everything the batch
// path allocates on first use for batches of up to nblocks blocks, so that a timed run starts with warm buffers
int cw_prepare(int hash_alg, int comp_alg, size_t block_bytes, size_t nblocks, int pinned_io)
{
    ThreadCtx *c;
    int rc = thread_ctx(&c);
    if (rc != CW_OK || nblocks == 0) return rc;
    HostJob j;
    int dummy = 0;
    if ((rc = host_job_init(j, hash_alg, comp_alg, &dummy, block_bytes, nblocks, &dummy, true)) != CW_OK) return rc;
    if (!j.do_hash && !j.do_comp) return CW_OK; // (CW_HASH_NONE, CW_COMP_NONE): nothing a batch would allocate
    const cw::Knobs kn = cw::knobs();
    size_t chunk = pipeline_chunk(kn, block_bytes, nblocks);
    // a batch whose chunks may grow (host_pipeline): buffers, workspaces and lane tables for the grown chunk, so that the growth costs
    // no allocation inside a timed window (18.5 GiB of device memory per calling thread)
    const size_t big = grown_chunk(kn, j, chunk, pinned_io != 0);
    if (big && nblocks > 2 * chunk && room_to_grow(*c, j, big)) chunk = nblocks - 2 * chunk < big ? nblocks - 2 * chunk : big;
    for (Slot &s : c->slot)
        if ((rc = slot_reserve(j, s, chunk, !pinned_io, !pinned_io, shared_lender(kn, *c, j, s))) != CW_OK) return rc;
    // One chunk's kernels on every slot (over whatever its device buffers hold): the codecs' per-stream workspaces -- queues, link
    // arrays, the lane parsers' tables -- are allocated here instead of inside the first timed batch, and the device leaves its
    // idle clocks.  Then a few copies each way to wake the link (the first pass after idle ran at 25-29 GB/s against 45.7).
    // CW_PREPARE_COLD=1 skips both.
    if (kn.prepare_cold) return CW_OK;
    for (Slot &s : c->slot)
        if ((rc = slot_kernels(j, s, chunk)) != CW_OK) return rc;
    void *h = nullptr;
    const size_t wb = (size_t)64 << 20 < chunk * block_bytes ? (size_t)64 << 20 : chunk * block_bytes;
    if (hipHostMalloc(&h, 2 * wb, hipHostMallocPortable) == hipSuccess) {
        for (int k = 0; k < 6; k++) {
            (void)hipMemcpyAsync(c->slot[1].src.p, h, wb, hipMemcpyHostToDevice, c->s_h2d);
            (void)hipMemcpyAsync((uint8_t *)h + wb, c->slot[2].src.p, wb, hipMemcpyDeviceToHost, c->s_d2h);
        }
    }
    pipe_drain(*c);
    if (h) (void)hipHostFree(h);
    (void)hipGetLastError();
    return CW_OK;
}

// page-locked host memory for the batch path (hipHostMalloc / hipHostRegister): buffers the copy engines use in place
void *cw_host_alloc(size_t bytes)
{
    if (ensure_init() != CW_OK) return nullptr;
    void *p = nullptr;
    hipError_t e = hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocPortable);
    if (e != hipSuccess) { fail(CW_ERR_NOMEM, "hipHostMalloc(%zu): %s", bytes, hipGetErrorString(e)); return nullptr; }
    return p;
}
void cw_host_free(void *p) { if (p) (void)hipHostFree(p); }
int cw_host_register(void *p, size_t bytes)
{
    int rc = ensure_init();
    if (rc != CW_OK) return rc;
    HIP_TRY(hipHostRegister(p, bytes, hipHostRegisterPortable));
    return CW_OK;
}
int cw_host_unregister(void *p)
{
    HIP_TRY(hipHostUnregister(p));
    return CW_OK;
}

int cw_hash_tree_blocks(int hash_alg, const void *src, size_t block_bytes, size_t nblocks, unsigned leaf, unsigned node, unsigned max_level,
                        void *digests)
{
    ThreadCtx *cp;
    int rc = thread_ctx(&cp);
    if (rc != CW_OK) return rc;
    ThreadCtx &c = *cp;
    if (nblocks == 0) return CW_OK;
    if ((!src && block_bytes) || !digests) return fail(CW_ERR_BAD_ARG, "NULL pointer");
    if ((rc = check_block(block_bytes)) != CW_OK) return rc;
    const size_t db = cw_digest_bytes(hash_alg);
    if (db == 0) return fail(CW_ERR_BAD_ARG, "unknown hash algorithm %d", hash_alg);
    size_t chunk = kMaxChunkBytes / (block_bytes + 64);
    if (chunk == 0) chunk = 1;
    if (chunk > nblocks) chunk = nblocks;
    if ((rc = c.src.reserve(chunk * block_bytes + 16)) != CW_OK || (rc = c.dig.reserve(chunk * db)) != CW_OK) return rc;
    for (size_t first = 0; first < nblocks; first += chunk) {
        const size_t n = nblocks - first < chunk ? nblocks - first : chunk;
        if (block_bytes) HIP_TRY(hipMemcpyAsync(c.src.p, (const uint8_t *)src + first * block_bytes, n * block_bytes, hipMemcpyHostToDevice, c.stream));
        if ((rc = cw_dev_hash_tree(hash_alg, c.src.p, block_bytes, block_bytes, n, leaf, node, max_level, c.dig.p, c.stream)) != CW_OK) return rc;
        HIP_TRY(hipMemcpyAsync((uint8_t *)digests + first * db, c.dig.p, n * db, hipMemcpyDeviceToHost, c.stream));
        HIP_TRY(hipStreamSynchronize(c.stream));
    }
    return CW_OK;
}

int cw_hash_blocks(int hash_alg, const void *src, size_t block_bytes, size_t nblocks, void *digests)
{
    if (!digests && nblocks) return fail(CW_ERR_BAD_ARG, "NULL digests");
    if (hash_alg == CW_HASH_NONE || cw_digest_bytes(hash_alg) == 0) return fail(CW_ERR_BAD_ARG, "unknown hash algorithm %d", hash_alg);
    return cw_hash_and_compress_blocks(hash_alg, CW_COMP_NONE, src, block_bytes, nblocks, digests, nullptr, 0, nullptr);
}

int cw_compress_blocks(int comp_alg, const void *src, size_t block_bytes, size_t nblocks, void *dst, size_t dst_stride,
                       uint32_t *sizes)
{
    if ((!dst || !sizes) && nblocks) return fail(CW_ERR_BAD_ARG, "NULL dst/sizes");
    if (int bad = check_codec(comp_alg)) return bad;
    return cw_hash_and_compress_blocks(CW_HASH_NONE, comp_alg, src, block_bytes, nblocks, nullptr, dst, dst_stride, sizes);
}

int cw_decompress_blocks(int comp_alg, const void *comp, size_t comp_stride, const uint32_t *sizes, size_t nblocks, void *dst,
                         size_t block_bytes, uint32_t *status)
{
    ThreadCtx *cp;
    int rc = thread_ctx(&cp);
    if (rc != CW_OK) return rc;
    ThreadCtx &c = *cp;
    if (nblocks == 0) return CW_OK;
    if (!comp || !sizes || !dst || !status) return fail(CW_ERR_BAD_ARG, "NULL pointer");
    if (int bad = check_codec(comp_alg)) return bad;
    if (block_bytes == 0 || (rc = check_block(block_bytes)) != CW_OK) return rc ? rc : fail(CW_ERR_BAD_ARG, "block_bytes == 0");
    const size_t d_stride = (comp_stride + 15) & ~(size_t)15;
    size_t chunk = kMaxChunkBytes / (d_stride + block_bytes + 8);
    if (chunk == 0) chunk = 1;
    if (chunk > nblocks) chunk = nblocks;
    if ((rc = c.src.reserve(chunk * d_stride + 16)) != CW_OK || (rc = c.dst.reserve(chunk * block_bytes)) != CW_OK ||
        (rc = c.sizes.reserve(chunk * 4)) != CW_OK || (rc = c.dig.reserve(chunk * 4)) != CW_OK)
        return rc;
    for (size_t first = 0; first < nblocks; first += chunk) {
        const size_t n = nblocks - first < chunk ? nblocks - first : chunk;
        for (size_t i = 0; i < n; i++) { // only the bytes each slot holds cross the bus
            const uint32_t sz = sizes[first + i];
            if (sz > comp_stride) return fail(CW_ERR_BAD_ARG, "block %zu: %u bytes exceed comp_stride %zu", first + i, sz, comp_stride);
            if (sz) HIP_TRY(hipMemcpyAsync((uint8_t *)c.src.p + i * d_stride, (const uint8_t *)comp + (first + i) * comp_stride, sz,
                                           hipMemcpyHostToDevice, c.stream));
        }
        HIP_TRY(hipMemcpyAsync(c.sizes.p, sizes + first, n * 4, hipMemcpyHostToDevice, c.stream));
        rc = cw_dev_decompress(comp_alg, c.src.p, d_stride, (const uint32_t *)c.sizes.p, n, c.dst.p, block_bytes, (uint32_t *)c.dig.p,
                               c.stream);
        if (rc != CW_OK) return rc;
        HIP_TRY(hipMemcpyAsync((uint8_t *)dst + first * block_bytes, c.dst.p, n * block_bytes, hipMemcpyDeviceToHost, c.stream));
        HIP_TRY(hipMemcpyAsync(status + first, c.dig.p, n * 4, hipMemcpyDeviceToHost, c.stream));
        HIP_TRY(hipStreamSynchronize(c.stream));
    }
    return CW_OK;
}

// ---- the reference's slots ----------------------------------------------------------------------------------
void cw_hash_skein(const char *src, char *dst, int count)
{
    if (count > 0 && cw_hash_blocks(CW_HASH_SKEIN256_128, src, cw_get_block_size(), (size_t)count, dst) != CW_OK) die("cw_hash_skein");
}

void cw_hash_skein512(const char *src, char *dst, int count)
{
    if (count > 0 && cw_hash_blocks(CW_HASH_SKEIN512, src, cw_get_block_size(), (size_t)count, dst) != CW_OK) die("cw_hash_skein512");
}

void cw_hash_sha256mb(const char *src, char *dst, int count)
{
    if (count > 0 && cw_hash_blocks(CW_HASH_SHA256, src, cw_get_block_size(), (size_t)count, dst) != CW_OK) die("cw_hash_sha256mb");
}

size_t cw_compress_lz4(const char *src, char *dst, size_t len)
{
    uint32_t sz = 0;
    if (len == 0) return 0;
    // the reference's caller provides 2*len (:353); output that cannot fit it reports 0 like LZ4 would
    int rc = cw_compress_blocks(CW_COMP_LZ4, src, len, 1, dst, 2 * len, &sz);
    if (rc == CW_ERR_BAD_ARG && strstr(t_err, "exceed dst_stride")) return 0;
    if (rc != CW_OK) die("cw_compress_lz4");
    return sz;
}

size_t cw_compress_lzf(const char *src, char *dst, size_t len)
{
    uint32_t sz = 0;
    if (len < 2) return 0; // lzf_compress(in, len, out, len-1) cannot fit anything
    if (cw_compress_blocks(CW_COMP_LZF, src, len, 1, dst, len - 1, &sz) != CW_OK) die("cw_compress_lzf");
    return sz;
}

int cw_decompress_lz4(const char *src, char *dst, int csize, int dst_cap)
{
    const size_t bb = cw_get_block_size();
    uint32_t sz = csize > 0 ? (uint32_t)csize : 0, st = 1;
    if (csize <= 0 || dst_cap < 0 || (size_t)dst_cap < bb) return -1;
    if (cw_decompress_blocks(CW_COMP_LZ4, src, sz, &sz, 1, dst, bb, &st) != CW_OK) die("cw_decompress_lz4");
    return st == 0 ? (int)bb : -1;
}

unsigned cw_decompress_lzf(const void *src, unsigned csize, void *dst, unsigned dst_cap)
{
    const size_t bb = cw_get_block_size();
    uint32_t sz = csize, st = 1;
    if (csize == 0 || dst_cap < bb) return 0;
    if (cw_decompress_blocks(CW_COMP_LZF, src, sz, &sz, 1, dst, bb, &st) != CW_OK) die("cw_decompress_lzf");
    return st == 0 ? (unsigned)bb : 0;
}

// Pieces of at most kMaxChunkBytes: each piece is chunked with final = 0 (the last with final = 1); the bytes after the last
// cut of a piece -- fewer than max_size -- are copied to the front of the next piece's buffer.
int cw_cdc_hash(const cw_cdc_params *p, int hash_alg, const void *src, size_t nbytes, uint64_t *offsets, size_t max_offsets,
                size_t *nchunks, void *digests)
{
    cw::CdcParams cp;
    int rc = cdc_params(p, &cp);
    if (rc != CW_OK) return rc;
    if (hash_alg < 0 || hash_alg > CW_HASH_NONE) return fail(CW_ERR_BAD_ARG, "unknown hash algorithm %d", hash_alg);
    if (!offsets || !nchunks || (nbytes && !src) || (hash_alg != CW_HASH_NONE && !digests)) return fail(CW_ERR_BAD_ARG, "NULL pointer");
    if (max_offsets < nbytes / cp.min_size + 2)
        return fail(CW_ERR_BAD_ARG, "max_offsets %zu < nbytes / min_size + 2 = %zu", max_offsets, nbytes / cp.min_size + 2);
    ThreadCtx *c;
    if ((rc = thread_ctx(&c)) != CW_OK) return rc;
    const hipStream_t s = c->stream;
    const size_t piece = kMaxChunkBytes, dbytes = cw_digest_bytes(hash_alg);
    const size_t cap = (piece + cp.max_size) / cp.min_size + 2; // offsets of one piece
    if ((rc = c->src.reserve(piece + cp.max_size)) != CW_OK) return rc;
    if ((rc = c->sizes.reserve(cap * 8 + 64)) != CW_OK) return rc;
    if (hash_alg != CW_HASH_NONE && (rc = c->dig.reserve(cap * dbytes)) != CW_OK) return rc;
    uint8_t *d_buf = (uint8_t *)c->src.p;
    uint64_t *d_off = (uint64_t *)c->sizes.p, *d_k = d_off + cap;
    size_t done = 0, carry = 0, k_total = 0; // done: stream bytes consumed; carry: bytes at the front of d_buf
    offsets[0] = 0;
    for (;;) {
        const size_t take = nbytes - done - carry < piece ? nbytes - done - carry : piece;
        const int fin = done + carry + take == nbytes;
        HIP_TRY(hipMemcpyAsync(d_buf + carry, (const uint8_t *)src + done + carry, take, hipMemcpyHostToDevice, s));
        const size_t len = carry + take;
        if ((rc = dev_cdc(cp, d_buf, len, fin, d_off, cap, d_k, s)) != CW_OK) return rc;
        if (hash_alg != CW_HASH_NONE && (rc = dev_hash_chunks(hash_alg, d_buf, len, d_off, d_k, cap, (uint8_t *)c->dig.p, s)) != CW_OK)
            return rc;
        uint64_t k = 0;
        HIP_TRY(hipMemcpyAsync(&k, d_k, 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        if (k_total + k + 1 > max_offsets) return fail(CW_ERR_BAD_ARG, "max_offsets %zu too small", max_offsets);
        std::vector<uint64_t> h(k + 1);
        HIP_TRY(hipMemcpyAsync(h.data(), d_off, (k + 1) * 8, hipMemcpyDeviceToHost, s));
        if (hash_alg != CW_HASH_NONE && k)
            HIP_TRY(hipMemcpyAsync((uint8_t *)digests + k_total * dbytes, c->dig.p, k * dbytes, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        for (uint64_t i = 1; i <= k; i++) offsets[k_total + i] = done + h[i];
        k_total += k;
        const size_t used = h[k];
        if (fin) break;
        // the tail after the last cut (< max_size bytes) moves to the front of the buffer
        carry = len - used;
        if (carry) HIP_TRY(hipMemcpyAsync(d_buf, d_buf + used, carry, hipMemcpyDeviceToDevice, s));
        done += used;
    }
    *nchunks = k_total;
    return CW_OK;
}

} // extern "C"
