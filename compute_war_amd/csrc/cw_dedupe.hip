// cw_dedupe.hip -- host side of the dedupe index (kernels and protocol: dedupe_kernels.hip; semantics: the public header): the index
// object and its table, insert / lookup / export / export of the live entries / import, the rebuild behind resize and retain, and the two fused calls that end in
// the codec over the new blocks or chunks only.
//
// The calls of one index are serialised: each takes the index's lock and goes through dedupe_on_stream, which orders its work behind
// the last call's (`last`) whatever stream that came on.

#include <mutex>

#include "cw_host.h"

using namespace cw::host;

namespace {
// the table of an index: one allocation, state | value | key | min_idx | ctrl
struct DedupeTable {
    void *mem = nullptr;
    uint64_t *state = nullptr, *value = nullptr, *key = nullptr;
    uint64_t *ctrl = nullptr; // [0] count, [1] a probe / lookup / rehash walk reached its bound, [2] n_new of the fused call
    uint32_t *min_idx = nullptr;
};
} // namespace

struct cw_dedupe {
    int device = -1, hash_alg = 0;
    unsigned words = 0;              // u64 words per digest
    size_t max_entries = 0;
    uint64_t cap = 0;                // slots: a power of two >= 2 x max_entries
    DedupeTable t;
    uint64_t *h_ctrl = nullptr;      // pinned: the fused call's copy of ctrl[1..2]
    DevBuf rec, flags, offs, gather; // per-call scratch, shared by the calls because they are serialised
    DevBuf stage_dig, stage_val, stage_out; // the host forms' pieces: digests | values | ref, new_idx, n_new of an import piece
    size_t stage_entries = (size_t)1 << 20; // pairs per piece (cw_dedupe_set_stage_entries)
    hipEvent_t last = nullptr;       // the last call's work: the next call's stream waits for it
    uint64_t count_bound = 0;        // upper bound on ctrl[0] (every block of every call counted)
    std::mutex lock;                 // guards `last`, the scratch and count_bound
};

namespace {
// checks shared by the dedupe calls
int dedupe_args(cw_dedupe *x, size_t nblocks, uint64_t base)
{
    int rc = ensure_init();
    if (rc != CW_OK) return rc;
    if (!x) return fail(CW_ERR_BAD_ARG, "NULL dedupe index");
    if (current_device() != x->device) return fail(CW_ERR_BAD_ARG, "dedupe index of device %d used on device %d", x->device, current_device());
    if ((rc = check_count("nblocks", nblocks)) != CW_OK) return rc;
    if (base > UINT64_MAX - nblocks) return fail(CW_ERR_BAD_ARG, "base + nblocks wraps");
    return CW_OK;
}

// the device pointers of a call that takes digests: all given (`all_there`), the digests readable as u64 words
int dedupe_dev_ptrs(bool all_there, const void *d_digests)
{
    if (!all_there) return fail(CW_ERR_BAD_ARG, "NULL device pointer");
    if ((uintptr_t)d_digests % 8) return fail(CW_ERR_BAD_ARG, "d_digests must be 8-byte aligned");
    return CW_OK;
}

// The one way a call queues work of the index on a stream: x->lock is held to the end of `body`, s waits for the last call's work
// first, and whatever body queued is the new `last` on every way out of it.  body's failure wins over a failed record.
template <class Body> int dedupe_on_stream(cw_dedupe *x, hipStream_t s, Body body)
{
    std::lock_guard<std::mutex> g(x->lock);
    HIP_TRY(hipStreamWaitEvent(s, x->last, 0));
    const int rc = body();
    const hipError_t e = hipEventRecord(x->last, s);
    return rc != CW_OK ? rc : launched(e, "hipEventRecord(x->last, s)");
}

int dedupe_inconsistent() { return fail(CW_ERR_HIP, "dedupe index: a probe reached its bound (the table is inconsistent)"); }

// x->lock held: the exact count, once the last call has finished
int dedupe_read_count(cw_dedupe *x, uint64_t *count)
{
    HIP_TRY(hipEventSynchronize(x->last));
    uint64_t c[2];
    HIP_TRY(hipMemcpy(c, x->t.ctrl, sizeof c, hipMemcpyDeviceToHost));
    if (c[1]) return dedupe_inconsistent();
    x->count_bound = *count = c[0];
    return CW_OK;
}

// x->lock held: refuse a call that could overflow the table.  The host bound only grows, so only when it would refuse is the
// exact count read.
int dedupe_admit(cw_dedupe *x, size_t n)
{
    if (x->count_bound + n <= x->max_entries) return CW_OK;
    uint64_t count = 0;
    const int rc = dedupe_read_count(x, &count);
    if (rc != CW_OK || count + n <= x->max_entries) return rc;
    return fail(CW_ERR_NOMEM, "dedupe index full: %llu entries + %zu blocks > max_entries %zu", (unsigned long long)count, n, x->max_entries);
}

// x->lock held: index-owned scratch of at least `bytes`; growing frees a buffer the last call may still use
int dedupe_scratch(cw_dedupe *x, DevBuf &b, size_t bytes)
{
    if (b.buf.bytes() < bytes) HIP_TRY(hipEventSynchronize(x->last));
    return b.reserve(bytes);
}

// x->lock held, admitted: probe, resolve, index-only pack scan of the new flags, scatter -- queued on s.  values != NULL: block i
// carries values[i] instead of base + i.
int dedupe_enqueue(cw_dedupe *x, const uint64_t *dig, uint32_t n, uint64_t base, const uint64_t *values, uint64_t *ref, uint32_t *new_idx,
                   uint64_t *d_n_new, hipStream_t s)
{
    int rc;
    if ((rc = dedupe_scratch(x, x->rec, (size_t)n * 8)) != CW_OK || (rc = dedupe_scratch(x, x->flags, (size_t)n * 4)) != CW_OK ||
        (rc = dedupe_scratch(x, x->offs, ((size_t)n + 1) * 8)) != CW_OK)
        return rc;
    const DedupeTable &t = x->t;
    uint64_t *rec = (uint64_t *)x->rec.p, *off = (uint64_t *)x->offs.p;
    uint32_t *flags = (uint32_t *)x->flags.p;
    x->count_bound += n; // from the first launch on, the table may change
    hipError_t e = cw::dedupe_probe_launch(x->words, dig, n, t.state, t.min_idx, t.value, t.key, x->cap - 1, rec, ref,
                                           reinterpret_cast<unsigned long long *>(t.ctrl + 1), s);
    if (e == hipSuccess) e = cw::dedupe_resolve_launch(x->words, dig, n, base, values, t.min_idx, t.state, t.value, t.key, rec, ref, flags, s);
    if (e == hipSuccess) e = cw::pack_launch(nullptr, 0, flags, n, nullptr, off, s);
    if (e == hipSuccess) e = cw::dedupe_scatter_launch(flags, off, n, rec, t.min_idx, new_idx, d_n_new, t.ctrl, s);
    return launched(e, "dedupe launch");
}

// cw_dev_dedupe (values NULL, by_value false) and cw_dev_dedupe_insert (by_value)
int dedupe_insert(cw_dedupe *x, const void *d_digests, size_t n, uint64_t base, bool by_value, const uint64_t *d_values, uint64_t *d_ref,
                  uint32_t *d_new_idx, uint64_t *d_n_new, hipStream_t s)
{
    int rc = dedupe_args(x, n, base);
    if (rc != CW_OK || n == 0) return rc;
    if ((rc = dedupe_dev_ptrs(d_digests && (d_values || !by_value) && d_ref && d_new_idx && d_n_new, d_digests)) != CW_OK) return rc;
    return dedupe_on_stream(x, s, [&]() -> int {
        const int ok = dedupe_admit(x, n);
        return ok != CW_OK ? ok : dedupe_enqueue(x, (const uint64_t *)d_digests, (uint32_t)n, base, d_values, d_ref, d_new_idx, d_n_new, s);
    });
}

uint64_t dedupe_cap(size_t max_entries)
{
    uint64_t cap = 2;
    while (cap < 2 * (uint64_t)max_entries) cap <<= 1;
    return cap;
}
size_t dedupe_table_bytes(uint64_t cap, size_t db) { return cap * (20 + db) + 4 * sizeof(uint64_t); }
// allocated and emptied (state EMPTY, min_idx UINT32_MAX, ctrl 0) on stream s, not synchronised; on failure nothing is held
hipError_t dedupe_table_alloc(uint64_t cap, size_t db, hipStream_t s, DedupeTable *t)
{
    hipError_t e = hipMalloc(&t->mem, dedupe_table_bytes(cap, db));
    if (e != hipSuccess) { t->mem = nullptr; return e; }
    uint8_t *p = (uint8_t *)t->mem;
    t->state = (uint64_t *)p;
    t->value = (uint64_t *)(p + cap * 8);
    t->key = (uint64_t *)(p + cap * 16);
    t->min_idx = (uint32_t *)(p + cap * (16 + db));
    t->ctrl = (uint64_t *)(p + cap * (20 + db)); // cap is even: 8-byte aligned
    e = hipMemsetAsync(t->state, 0, cap * 8, s);
    if (e == hipSuccess) e = hipMemsetAsync(t->min_idx, 0xFF, cap * 4, s);
    if (e == hipSuccess) e = hipMemsetAsync(t->ctrl, 0, 4 * sizeof(uint64_t), s);
    if (e != hipSuccess) { (void)hipFree(t->mem); t->mem = nullptr; }
    return e;
}

// x->lock held, the count read (so the old table is idle, and the lock keeps new calls out): a table for max_entries beside the old
// one, filled by `fill` on the NULL stream, takes the old one's place.  fill(t, cap, c) returns after a synchronise with c[0] = the
// new table's entries and c[1] = its walks' error word; when it fails or c[1] is set the index is unchanged.  `who` names the call.
template <class Fill> int dedupe_rebuild(cw_dedupe *x, const char *who, size_t max_entries, Fill fill)
{
    const uint64_t cap = dedupe_cap(max_entries);
    const size_t db = (size_t)x->words * 8;
    DedupeTable t;
    const hipError_t e = dedupe_table_alloc(cap, db, nullptr, &t);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(e == hipErrorOutOfMemory ? CW_ERR_NOMEM : CW_ERR_HIP, "%s(%zu entries, %zu bytes beside the old table): %s", who, max_entries,
                    dedupe_table_bytes(cap, db), hipGetErrorString(e));
    }
    uint64_t c[2] = {0, 0};
    int rc = fill(t, cap, c);
    if (rc == CW_OK && c[1]) rc = fail(CW_ERR_HIP, "%s: an entry found no slot in the new table (the index is unchanged)", who);
    if (rc != CW_OK) { (void)hipFree(t.mem); return rc; }
    void *old = x->t.mem;
    x->t = t;
    x->cap = cap;
    x->max_entries = max_entries;
    x->count_bound = c[0];
    HIP_TRY(hipEventRecord(x->last, nullptr));
    HIP_TRY(hipFree(old));
    return CW_OK;
}

// x->lock held, s waits for x->last: tile counts and their scan into the index's scratch (flags = counts, offs)
int dedupe_export_scan(cw_dedupe *x, hipStream_t s)
{
    const uint64_t ntiles = cw::dedupe_export_tiles(x->cap);
    int rc;
    if ((rc = dedupe_scratch(x, x->flags, ntiles * 4)) != CW_OK || (rc = dedupe_scratch(x, x->offs, (ntiles + 1) * 8)) != CW_OK) return rc;
    return launched(cw::dedupe_export_scan_launch(x->t.state, x->cap, (uint32_t *)x->flags.p, (uint64_t *)x->offs.p, s), "dedupe export scan launch");
}
int dedupe_export_scatter(cw_dedupe *x, uint64_t first, uint64_t max_out, void *d_digests, uint64_t *d_values, uint64_t *d_n, hipStream_t s)
{
    return launched(cw::dedupe_export_scatter_launch(x->words, x->t.state, x->t.value, x->t.key, x->cap, (const uint64_t *)x->offs.p, first, max_out,
                                                     (uint64_t *)d_digests, d_values, d_n, s),
                    "dedupe export launch");
}
} // namespace

extern "C" {

cw_dedupe_t *cw_dedupe_create(int hash_alg, size_t max_entries)
{
    if (ensure_init() != CW_OK) return nullptr;
    const size_t db = cw_digest_bytes(hash_alg);
    if (db == 0 || max_entries == 0 || max_entries > ((size_t)1 << 40)) {
        fail(CW_ERR_BAD_ARG, "cw_dedupe_create: hash algorithm %d / max_entries %zu not usable", hash_alg, max_entries);
        return nullptr;
    }
    cw_dedupe *x = new cw_dedupe;
    x->device = current_device();
    x->hash_alg = hash_alg;
    x->words = (unsigned)(db / 8);
    x->cap = dedupe_cap(max_entries);
    x->max_entries = max_entries;
    hipError_t e = dedupe_table_alloc(x->cap, db, nullptr, &x->t);
    if (e == hipSuccess) e = hipDeviceSynchronize(); // the calls come on other streams
    if (e == hipSuccess) e = hipHostMalloc(reinterpret_cast<void **>(&x->h_ctrl), 2 * sizeof(uint64_t), hipHostMallocDefault);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&x->last, hipEventDisableTiming);
    if (e != hipSuccess) {
        fail(e == hipErrorOutOfMemory ? CW_ERR_NOMEM : CW_ERR_HIP, "cw_dedupe_create(%zu entries, %zu bytes): %s", max_entries,
             dedupe_table_bytes(x->cap, db), hipGetErrorString(e));
        cw_dedupe_destroy(x);
        return nullptr;
    }
    return x;
}

void cw_dedupe_destroy(cw_dedupe_t *x)
{
    if (!x) return;
    (void)hipSetDevice(x->device);
    if (x->last) { (void)hipEventSynchronize(x->last); (void)hipEventDestroy(x->last); }
    x->rec.release(); x->flags.release(); x->offs.release(); x->gather.release();
    x->stage_dig.release(); x->stage_val.release(); x->stage_out.release();
    if (x->t.mem) (void)hipFree(x->t.mem);
    if (x->h_ctrl) (void)hipHostFree(x->h_ctrl);
    delete x;
}

int cw_dedupe_count(cw_dedupe_t *x, uint64_t *count)
{
    int rc = dedupe_args(x, 0, 0);
    if (rc != CW_OK) return rc;
    if (!count) return fail(CW_ERR_BAD_ARG, "NULL count");
    std::lock_guard<std::mutex> g(x->lock);
    return dedupe_read_count(x, count);
}

int cw_dedupe_max_entries(cw_dedupe_t *x, size_t *max_entries)
{
    if (!x || !max_entries) return fail(CW_ERR_BAD_ARG, "NULL %s", x ? "max_entries" : "dedupe index");
    std::lock_guard<std::mutex> g(x->lock);
    *max_entries = x->max_entries;
    return CW_OK;
}

int cw_dedupe_set_stage_entries(cw_dedupe_t *x, size_t entries)
{
    if (!x) return fail(CW_ERR_BAD_ARG, "NULL dedupe index");
    if (int rc = check_count("stage entries", entries)) return rc;
    std::lock_guard<std::mutex> g(x->lock);
    x->stage_entries = entries ? entries : (size_t)1 << 20;
    return CW_OK;
}

int cw_dev_dedupe(cw_dedupe_t *x, const void *d_digests, size_t nblocks, uint64_t base, uint64_t *d_ref, uint32_t *d_new_idx,
                  uint64_t *d_n_new, void *stream)
{
    return dedupe_insert(x, d_digests, nblocks, base, false, nullptr, d_ref, d_new_idx, d_n_new, (hipStream_t)stream);
}

int cw_dev_dedupe_insert(cw_dedupe_t *x, const void *d_digests, const uint64_t *d_values, size_t n, uint64_t *d_ref, uint32_t *d_new_idx,
                         uint64_t *d_n_new, void *stream)
{
    return dedupe_insert(x, d_digests, n, 0, true, d_values, d_ref, d_new_idx, d_n_new, (hipStream_t)stream);
}

int cw_dev_dedupe_lookup(cw_dedupe_t *x, const void *d_digests, size_t n, uint64_t *d_ref, uint64_t *d_n_found, void *stream)
{
    int rc = dedupe_args(x, n, 0);
    if (rc != CW_OK || n == 0) return rc;
    if ((rc = dedupe_dev_ptrs(d_digests && d_ref && d_n_found, d_digests)) != CW_OK) return rc;
    const hipStream_t s = (hipStream_t)stream;
    return dedupe_on_stream(x, s, [&]() -> int {
        return launched(cw::dedupe_lookup_launch(x->words, (const uint64_t *)d_digests, (uint32_t)n, x->t.state, x->t.value, x->t.key, x->cap - 1, d_ref,
                                                 d_n_found, reinterpret_cast<unsigned long long *>(x->t.ctrl + 1), s),
                        "dedupe lookup launch");
    });
}

int cw_dev_dedupe_export(cw_dedupe_t *x, void *d_digests, uint64_t *d_values, size_t max_out, uint64_t *d_n, void *stream)
{
    int rc = dedupe_args(x, 0, 0);
    if (rc != CW_OK) return rc;
    if ((rc = dedupe_dev_ptrs(d_n && (!max_out || (d_digests && d_values)), d_digests)) != CW_OK) return rc;
    const hipStream_t s = (hipStream_t)stream;
    return dedupe_on_stream(x, s, [&]() -> int {
        const int ok = dedupe_export_scan(x, s);
        return ok != CW_OK ? ok : dedupe_export_scatter(x, 0, max_out, d_digests, d_values, d_n, s);
    });
}

int cw_dev_dedupe_export_live(cw_dedupe_t *x, const uint32_t *d_live, uint64_t dir_base, size_t dir_entries, void *d_digests, uint64_t *d_values,
                              size_t max_out, uint64_t *d_result, void *stream)
{
    int rc;
    if (!x || !d_live || !d_result || (max_out && (!d_digests || !d_values))) return fail(CW_ERR_BAD_ARG, "NULL %s", x ? "pointer" : "dedupe index");
    if (((uintptr_t)d_digests | (uintptr_t)d_values | (uintptr_t)d_result) % 8)
        return fail(CW_ERR_BAD_ARG, "d_digests / d_values / d_result not 8-byte aligned");
    if (dir_entries == 0) return fail(CW_ERR_BAD_ARG, "dir_entries is 0");
    if ((rc = check_count("dir_entries", dir_entries)) != CW_OK || (rc = check_count("max_out", max_out)) != CW_OK) return rc;
    if ((rc = dedupe_args(x, 0, 0)) != CW_OK) return rc;
    const hipStream_t s = (hipStream_t)stream;
    return dedupe_on_stream(x, s, [&]() -> int { // the flags and their ranks go into the index's scratch (flags, offs)
        int ok;
        if ((ok = dedupe_scratch(x, x->flags, dir_entries * 4)) != CW_OK || (ok = dedupe_scratch(x, x->offs, (dir_entries + 1) * 8)) != CW_OK) return ok;
        return launched(cw::dedupe_export_live_launch(x->words, x->t.state, x->t.value, x->t.key, x->cap, d_live, dir_base, dir_entries,
                                                      (uint32_t *)x->flags.p, (uint64_t *)x->offs.p, max_out, (uint64_t *)d_digests, d_values, d_result, s),
                        "dedupe export live launch");
    });
}

// The index's side of a renumbering: values change in place (value[] lies apart from the keys), so there is no rebuild and the count
// bound stays.  The two counters go into the index's scratch (rec).
int cw_dev_dedupe_revalue(cw_dedupe_t *x, const uint64_t *d_from, const uint64_t *d_to, const uint64_t *d_npairs, size_t max_pairs,
                          uint64_t range_base, uint64_t range_entries, uint64_t *d_result, void *stream)
{
    int rc;
    if (!x || !d_from || !d_to || !d_npairs || !d_result) return fail(CW_ERR_BAD_ARG, "NULL %s", x ? "pointer" : "dedupe index");
    if (((uintptr_t)d_from | (uintptr_t)d_to | (uintptr_t)d_npairs | (uintptr_t)d_result) % 8)
        return fail(CW_ERR_BAD_ARG, "d_from / d_to / d_npairs / d_result not 8-byte aligned");
    if ((rc = check_count("max_pairs", max_pairs)) != CW_OK) return rc;
    if (range_base > UINT64_MAX - range_entries) return fail(CW_ERR_BAD_ARG, "range_base + range_entries wraps");
    if ((rc = dedupe_args(x, 0, 0)) != CW_OK) return rc;
    const hipStream_t s = (hipStream_t)stream;
    return dedupe_on_stream(x, s, [&]() -> int {
        const int ok = dedupe_scratch(x, x->rec, 64);
        if (ok != CW_OK) return ok;
        return launched(cw::dedupe_revalue_launch(x->t.state, x->t.value, x->cap, d_from, d_to, d_npairs, max_pairs, range_base, range_entries,
                                                  (uint64_t *)x->rec.p, d_result, s),
                        "dedupe revalue launch");
    });
}

// One window of a scrub: the plan, the restore and the finish are scrub_kernels.hip's; between restore and finish the index judges --
// the hash of the window's chunks, then one sweep of the table.  Read-only for the index, serialised with its other calls.
int cw_dev_store_verify(cw_dedupe_t *x, int comp_alg, const void *d_store, size_t store_bytes, const cw_chunk_loc *d_dir, uint64_t dir_base,
                        size_t dir_entries, const uint32_t *d_live, uint64_t *d_cursor, void *d_work, size_t work_bytes, uint32_t *d_status,
                        uint64_t *d_totals, void *stream)
{
    int rc;
    if (!x || !d_dir || !d_cursor || !d_work || !d_status || !d_totals || (store_bytes && !d_store))
        return fail(CW_ERR_BAD_ARG, "NULL %s", x ? "pointer" : "dedupe index");
    if ((rc = check_codec(comp_alg)) != CW_OK) return rc;
    if (dir_entries == 0) return fail(CW_ERR_BAD_ARG, "dir_entries is 0");
    if ((rc = check_count("dir_entries", dir_entries)) != CW_OK) return rc;
    if (work_bytes < CW_MAX_BLOCK_BYTES) return fail(CW_ERR_BAD_ARG, "work_bytes %zu < %u", work_bytes, CW_MAX_BLOCK_BYTES);
    if ((uintptr_t)d_dir % 16) return fail(CW_ERR_BAD_ARG, "d_dir is not 16-byte aligned");
    if (((uintptr_t)d_cursor | (uintptr_t)d_totals) % 8) return fail(CW_ERR_BAD_ARG, "d_cursor / d_totals not 8-byte aligned");
    if ((rc = dedupe_args(x, 0, 0)) != CW_OK) return rc;
    const hipStream_t s = (hipStream_t)stream;
    const size_t window = cw::store_verify_window(dir_entries, cw::knobs().scrub_entries);
    return dedupe_on_stream(x, s, [&]() -> int {
        struct Judge { cw_dedupe *x; uint8_t *work; size_t work_bytes; uint64_t dir_base; hipStream_t s; int rc; };
        Judge j{x, (uint8_t *)d_work, work_bytes, dir_base, s, CW_OK};
        const cw::ScrubJudge judge{[](void *ctx, const cw::ScrubWindow &w) {
                                       Judge &j = *static_cast<Judge *>(ctx);
                                       j.rc = dev_hash_chunks(j.x->hash_alg, j.work, j.work_bytes, w.raw_off, w.d_count, w.max_entries, w.digests, j.s);
                                       if (j.rc != CW_OK) return hipErrorUnknown; // (the message is recorded)
                                       const DedupeTable &t = j.x->t;
                                       return cw::dedupe_verify_launch(j.x->words, t.state, t.value, t.key, j.x->cap, j.dir_base, w.head, w.decoded,
                                                                       (const uint64_t *)w.digests, w.verdict, j.s);
                                   },
                                   &j};
        const hipError_t e = cw::store_verify_launch(comp_alg == CW_COMP_LZF, (const uint8_t *)d_store, store_bytes, d_dir, dir_base, dir_entries, d_live,
                                                     d_cursor, (uint8_t *)d_work, work_bytes, window, x->words * 8, d_status, d_totals, judge, s);
        if (j.rc != CW_OK) return j.rc;
        if (e == hipErrorOutOfMemory)
            return fail(CW_ERR_NOMEM, "scrub scratch (%zu bytes): %s", cw::store_verify_scratch_bytes(window, x->words * 8), hipGetErrorString(e));
        return launched(e, "store verify launch");
    });
}

int cw_dedupe_export(cw_dedupe_t *x, void *digests, uint64_t *values, size_t max_out, size_t *n)
{
    int rc = dedupe_args(x, 0, 0);
    if (rc != CW_OK) return rc;
    if (!n || (max_out && (!digests || !values))) return fail(CW_ERR_BAD_ARG, "NULL pointer");
    hipStream_t s;
    if ((rc = ctx_stream(&s)) != CW_OK) return rc;
    const size_t db = (size_t)x->words * 8;
    return dedupe_on_stream(x, s, [&]() -> int {
        int rc = dedupe_export_scan(x, s);
        if (rc != CW_OK) return rc;
        uint64_t total = 0;
        HIP_TRY(hipMemcpyAsync(&total, (const uint64_t *)x->offs.p + cw::dedupe_export_tiles(x->cap), sizeof total, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        const size_t want = total < max_out ? (size_t)total : max_out, piece = x->stage_entries < want ? x->stage_entries : want;
        if (piece && ((rc = dedupe_scratch(x, x->stage_dig, piece * db)) != CW_OK || (rc = dedupe_scratch(x, x->stage_val, piece * 8)) != CW_OK)) return rc;
        for (size_t first = 0; first < want; first += piece) {
            const size_t k = want - first < piece ? want - first : piece;
            if ((rc = dedupe_export_scatter(x, first, k, x->stage_dig.p, (uint64_t *)x->stage_val.p, nullptr, s)) != CW_OK) return rc;
            HIP_TRY(hipMemcpyAsync((uint8_t *)digests + first * db, x->stage_dig.p, k * db, hipMemcpyDeviceToHost, s));
            HIP_TRY(hipMemcpyAsync(values + first, x->stage_val.p, k * 8, hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s)); // the next piece overwrites the staging buffers
        }
        *n = (size_t)total;
        return CW_OK;
    });
}

int cw_dedupe_import(cw_dedupe_t *x, const void *digests, const uint64_t *values, size_t n, size_t *n_inserted)
{
    if (n_inserted) *n_inserted = 0;
    int rc = dedupe_args(x, 0, 0);
    if (rc != CW_OK) return rc;
    if (!n_inserted || (n && (!digests || !values))) return fail(CW_ERR_BAD_ARG, "NULL pointer");
    if (n == 0) return CW_OK;
    hipStream_t s;
    if ((rc = ctx_stream(&s)) != CW_OK) return rc;
    const size_t db = (size_t)x->words * 8;
    return dedupe_on_stream(x, s, [&]() -> int {
        int rc = dedupe_admit(x, n); // the whole import: count only grows by what the pieces insert, so no piece can overflow
        if (rc != CW_OK) return rc;
        const size_t piece = x->stage_entries < n ? x->stage_entries : n;
        if ((rc = dedupe_scratch(x, x->stage_dig, piece * db)) != CW_OK || (rc = dedupe_scratch(x, x->stage_val, piece * 8)) != CW_OK ||
            (rc = dedupe_scratch(x, x->stage_out, piece * 12 + 16)) != CW_OK)
            return rc;
        uint64_t *d_ref = (uint64_t *)x->stage_out.p, *d_k = d_ref + piece;
        uint32_t *d_new = (uint32_t *)(d_k + 1);
        size_t inserted = 0;
        for (size_t first = 0; first < n; first += piece) {
            const size_t k = n - first < piece ? n - first : piece;
            uint64_t k_new = 0;
            HIP_TRY(hipMemcpyAsync(x->stage_dig.p, (const uint8_t *)digests + first * db, k * db, hipMemcpyHostToDevice, s));
            HIP_TRY(hipMemcpyAsync(x->stage_val.p, values + first, k * 8, hipMemcpyHostToDevice, s));
            rc = dedupe_enqueue(x, (const uint64_t *)x->stage_dig.p, (uint32_t)k, 0, (const uint64_t *)x->stage_val.p, d_ref, d_new, d_k, s);
            if (rc != CW_OK) return rc;
            HIP_TRY(hipMemcpyAsync(&k_new, d_k, sizeof k_new, hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s)); // the next piece overwrites the staging buffers
            inserted += (size_t)k_new;
        }
        *n_inserted = inserted;
        return CW_OK;
    });
}

int cw_dedupe_resize(cw_dedupe_t *x, size_t new_max_entries)
{
    int rc = dedupe_args(x, 0, 0);
    if (rc != CW_OK) return rc;
    std::lock_guard<std::mutex> g(x->lock);
    uint64_t count = 0;
    if ((rc = dedupe_read_count(x, &count)) != CW_OK) return rc;
    if (new_max_entries == 0 || new_max_entries > ((size_t)1 << 40) || new_max_entries < count)
        return fail(CW_ERR_BAD_ARG, "cw_dedupe_resize: max_entries %zu not in [max(1, count = %llu), 2^40]", new_max_entries, (unsigned long long)count);
    if (dedupe_cap(new_max_entries) == x->cap) { // the same table serves
        x->max_entries = new_max_entries;
        return CW_OK;
    }
    // rehash every entry, and carry ctrl over
    return dedupe_rebuild(x, "cw_dedupe_resize", new_max_entries, [&](const DedupeTable &t, uint64_t cap, uint64_t *c) -> int {
        c[0] = count;
        hipError_t e = cw::dedupe_rehash_launch(x->words, x->t.state, x->t.value, x->t.key, x->cap, t.state, t.value, t.key, cap - 1,
                                                reinterpret_cast<unsigned long long *>(t.ctrl + 1), nullptr);
        if (e == hipSuccess) e = hipMemcpyAsync(&c[1], t.ctrl + 1, sizeof c[1], hipMemcpyDeviceToHost, nullptr);
        if (e == hipSuccess) e = hipMemcpyAsync(t.ctrl, x->t.ctrl, 4 * sizeof(uint64_t), hipMemcpyDeviceToDevice, nullptr);
        if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
        return launched(e, "cw_dedupe_resize");
    });
}

// cw_dedupe_resize with a filter (the keep rule: dedupe_retain_kernel).  When the new table could not hold every entry of the old one
// (new_max_entries below the old count) the kept entries are counted first, by the same kernel without a table: rehashing more
// entries than the table has slots would walk the whole table once per entry that finds none.
int cw_dedupe_retain(cw_dedupe_t *x, const uint32_t *d_live, uint64_t dir_base, size_t dir_entries, size_t new_max_entries, uint64_t *n_removed)
{
    if (!x || !d_live) return fail(CW_ERR_BAD_ARG, "cw_dedupe_retain: NULL %s", x ? "d_live" : "dedupe index");
    if (dir_entries == 0) return fail(CW_ERR_BAD_ARG, "cw_dedupe_retain: dir_entries is 0");
    if (new_max_entries > ((size_t)1 << 40)) return fail(CW_ERR_BAD_ARG, "cw_dedupe_retain: max_entries %zu > 2^40", new_max_entries);
    int rc = dedupe_args(x, 0, 0);
    if (rc != CW_OK) return rc;
    std::lock_guard<std::mutex> g(x->lock);
    uint64_t count = 0, kept = 0;
    if ((rc = dedupe_read_count(x, &count)) != CW_OK) return rc;
    const size_t want = new_max_entries ? new_max_entries : x->max_entries;
    rc = dedupe_rebuild(x, "cw_dedupe_retain", want, [&](const DedupeTable &t, uint64_t cap, uint64_t *c) -> int {
        // t.ctrl[0] counts the kept entries, t.ctrl[1] takes the walks' error word
        unsigned long long *kept_d = reinterpret_cast<unsigned long long *>(t.ctrl), *err_d = kept_d + 1;
        const DedupeTable &o = x->t;
        hipError_t e = hipSuccess;
        if (want < count) {
            e = cw::dedupe_retain_launch(x->words, o.state, o.value, o.key, x->cap, d_live, dir_base, dir_entries, nullptr, nullptr, nullptr, 0, kept_d,
                                         err_d, nullptr);
            if (e == hipSuccess) e = hipMemcpyAsync(c, t.ctrl, 2 * sizeof *c, hipMemcpyDeviceToHost, nullptr);
            if (e == hipSuccess) e = hipMemsetAsync(t.ctrl, 0, 2 * sizeof *c, nullptr);
            if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
        }
        if (e == hipSuccess && c[0] <= want) {
            e = cw::dedupe_retain_launch(x->words, o.state, o.value, o.key, x->cap, d_live, dir_base, dir_entries, t.state, t.value, t.key, cap - 1,
                                         kept_d, err_d, nullptr);
            if (e == hipSuccess) e = hipMemcpyAsync(c, t.ctrl, 2 * sizeof *c, hipMemcpyDeviceToHost, nullptr);
            if (e == hipSuccess) e = hipMemcpyAsync(t.ctrl + 2, o.ctrl + 2, 2 * sizeof(uint64_t), hipMemcpyDeviceToDevice, nullptr);
            if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
        }
        if (e != hipSuccess) return launched(e, "cw_dedupe_retain");
        if ((kept = c[0]) > want)
            return fail(CW_ERR_BAD_ARG, "cw_dedupe_retain: max_entries %zu below the %llu kept entries (the index is unchanged)", want,
                        (unsigned long long)c[0]);
        return CW_OK;
    });
    if (rc == CW_OK && n_removed) *n_removed = count - kept;
    return rc;
}

// hash -> dedupe -> one 16-byte copy back + a synchronise -> the codec over the new blocks only.  The codec cannot start before
// the dedupe result, so hash and codec do not overlap as in the fused hash-and-compress call.
int cw_dev_hash_dedupe_compress(cw_dedupe_t *x, int comp_alg, const void *d_src, size_t block_bytes, size_t src_stride, size_t nblocks,
                                uint64_t base, void *d_digests, uint64_t *d_ref, uint32_t *d_new_idx, void *d_dst, size_t dst_stride,
                                uint32_t *d_sizes, size_t *n_new, void *stream)
{
    if (n_new) *n_new = 0;
    int rc = dedupe_args(x, nblocks, base);
    if (rc != CW_OK) return rc;
    if (!n_new) return fail(CW_ERR_BAD_ARG, "NULL n_new");
    if ((rc = check_codec(comp_alg)) != CW_OK || nblocks == 0) return rc;
    if ((rc = dedupe_dev_ptrs(d_src && d_digests && d_ref && d_new_idx && d_dst && d_sizes, d_digests)) != CW_OK) return rc;
    if (block_bytes == 0 || (rc = check_block(block_bytes)) != CW_OK) return rc ? rc : fail(CW_ERR_BAD_ARG, "block_bytes == 0");
    if (src_stride < block_bytes) return fail(CW_ERR_BAD_ARG, "src_stride < block_bytes");
    if (dst_stride < cw_compress_bound(comp_alg, block_bytes))
        return fail(CW_ERR_BAD_ARG, "dst_stride %zu < bound %zu", dst_stride, cw_compress_bound(comp_alg, block_bytes));
    const hipStream_t s = (hipStream_t)stream;
    const uint8_t *src = (const uint8_t *)d_src;
    return dedupe_on_stream(x, s, [&]() -> int { // (the lock is held to the end: the gather buffer is the index's)
        int rc = dedupe_admit(x, nblocks);
        if (rc == CW_OK) rc = dev_hash(x->hash_alg, src, block_bytes, src_stride, nblocks, (uint8_t *)d_digests, s, true);
        if (rc == CW_OK) rc = dedupe_enqueue(x, (const uint64_t *)d_digests, (uint32_t)nblocks, base, nullptr, d_ref, d_new_idx, x->t.ctrl + 2, s);
        if (rc != CW_OK) return rc;
        HIP_TRY(hipMemcpyAsync(x->h_ctrl, x->t.ctrl + 1, 2 * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        if (x->h_ctrl[0]) return dedupe_inconsistent();
        const size_t k = (size_t)x->h_ctrl[1];
        if (k == nblocks) { // all new: the codec on the caller's blocks, slots as cw_dev_hash_and_compress
            rc = dev_compress(comp_alg, src, block_bytes, src_stride, nblocks, (uint8_t *)d_dst, dst_stride, d_sizes, s);
        } else if (k) { // (the stream is idle here, and it waited for the last call: nothing uses the old buffer)
            if ((rc = x->gather.reserve(k * block_bytes)) != CW_OK) return rc;
            rc = launched(cw::dedupe_gather_launch(src, block_bytes, src_stride, d_new_idx, k, (uint8_t *)x->gather.p, s), "gather launch");
            if (rc == CW_OK)
                rc = dev_compress(comp_alg, (const uint8_t *)x->gather.p, block_bytes, block_bytes, k, (uint8_t *)d_dst, dst_stride, d_sizes, s);
        }
        if (rc == CW_OK) *n_new = k;
        return rc;
    });
}

} // extern "C"

// cdc -> hash of every chunk -> one small copy back + a synchronise (the dedupe's admit check and launch need the count on the
// host) -> dedupe -> the chunk codec over the new chunks, selected on the device: n_new never comes back to the host.  With a hook
// (cw_store_ingest's pieces) the copy also carries the bytes consumed, the store's cursor and the last commit's verdict, and the
// hook's admission runs beside the index's, before anything is inserted.
int cw::host::dev_cdc_dedupe_compress(cw_dedupe_t *x, const cw_cdc_params *p, int comp_alg, const void *d_src, size_t nbytes, int final_, uint64_t base,
                                      uint64_t *d_offsets, size_t max_offsets, uint64_t *d_nchunks, void *d_digests, uint64_t *d_ref,
                                      uint32_t *d_new_idx, uint64_t *d_n_new, void *d_dst, size_t dst_bytes, uint32_t *d_sizes, size_t *nchunks,
                                      hipStream_t s, const PieceAdmit *hook, const StreamList *streams)
{
    if (nchunks) *nchunks = 0;
    cw::CdcParams cp;
    int rc = cdc_params(p, &cp);
    if (rc != CW_OK) return rc;
    if (!nchunks) return fail(CW_ERR_BAD_ARG, "NULL nchunks");
    if (!d_offsets || !d_nchunks || !d_digests || !d_ref || !d_new_idx || !d_n_new || (nbytes && !d_src)) return fail(CW_ERR_BAD_ARG, "NULL pointer");
    if (streams) {
        if ((rc = cdc_streams_args(cp, d_src, nbytes, *streams, d_offsets, max_offsets, d_nchunks)) != CW_OK) return rc;
    } else if (max_offsets < nbytes / cp.min_size + 2) {
        return fail(CW_ERR_BAD_ARG, "max_offsets %zu < nbytes / min_size + 2 = %zu", max_offsets, nbytes / cp.min_size + 2);
    }
    if ((rc = dedupe_dev_ptrs(true, d_digests)) != CW_OK) return rc;
    const size_t max_chunks = max_offsets - 1;
    if ((rc = compress_chunks_args(comp_alg, d_src, nbytes, d_offsets, d_nchunks, max_chunks, d_new_idx, d_n_new, d_dst, dst_bytes, d_sizes)) != CW_OK)
        return rc;
    if ((rc = dedupe_args(x, 0, base)) != CW_OK) return rc; // (base + the chunk count: checked when the count is known, as cw_dev_dedupe would)
    const uint8_t *src = (const uint8_t *)d_src;
    return dedupe_on_stream(x, s, [&]() -> int {
        int rc = streams ? dev_cdc_streams(cp, src, nbytes, *streams, d_offsets, max_offsets, d_nchunks, s)
                         : dev_cdc(cp, src, nbytes, final_ ? 1 : 0, d_offsets, max_offsets, d_nchunks, s);
        if (rc == CW_OK && hook && hook->after_cdc) rc = hook->after_cdc(hook->self, s);
        if (rc == CW_OK) rc = dev_hash_chunks(x->hash_alg, src, nbytes, d_offsets, d_nchunks, max_chunks, (uint8_t *)d_digests, s);
        if (rc != CW_OK) return rc;
        uint64_t *h_counts = hook ? hook->h_counts : x->h_ctrl;
        if (hook) {
            rc = launched(cw::piece_counts_launch(d_offsets, d_nchunks, max_chunks, hook->d_used, hook->d_verdict, hook->d_counts, s), "piece counts launch");
            if (rc != CW_OK) return rc;
            HIP_TRY(hipMemcpyAsync(h_counts, hook->d_counts, 4 * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
        } else {
            HIP_TRY(hipMemcpyAsync(h_counts, d_nchunks, sizeof(uint64_t), hipMemcpyDeviceToHost, s));
        }
        // the verdict on d_ends has a word of its own: with a hook, h_counts[1] is the bytes consumed
        uint64_t *h_ends_verdict = h_counts + (hook ? 4 : 1);
        if (streams) HIP_TRY(hipMemcpyAsync(h_ends_verdict, streams->d_result, sizeof(uint64_t), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        if (streams && *h_ends_verdict) return fail(CW_ERR_BAD_ARG, "d_ends decreases or does not end at nbytes = %zu", nbytes);
        const size_t k = (size_t)h_counts[0];
        *nchunks = k;
        if (hook && (rc = hook->admit(hook->self, k, h_counts)) != CW_OK) return rc;
        if (k == 0) { // (an empty input: cw_dev_dedupe would launch nothing)
            HIP_TRY(hipMemsetAsync(d_n_new, 0, sizeof(uint64_t), s));
            return CW_OK;
        }
        if (base > UINT64_MAX - k) return fail(CW_ERR_BAD_ARG, "base + nchunks wraps");
        if ((rc = dedupe_admit(x, k)) != CW_OK) return rc; // offsets and digests are written; nothing inserted, nothing compressed
        rc = dedupe_enqueue(x, (const uint64_t *)d_digests, (uint32_t)k, base, nullptr, d_ref, d_new_idx, d_n_new, s);
        if (rc != CW_OK) return rc;
        if (hook) *hook->inserted = true;
        return dev_compress_chunks(comp_alg, src, nbytes, d_offsets, d_nchunks, max_chunks, d_new_idx, d_n_new, (uint8_t *)d_dst, d_sizes, s);
    });
}

extern "C" int cw_dev_cdc_dedupe_compress(cw_dedupe_t *x, const cw_cdc_params *p, int comp_alg, const void *d_src, size_t nbytes, int final,
                                          uint64_t base, uint64_t *d_offsets, size_t max_offsets, uint64_t *d_nchunks, void *d_digests,
                                          uint64_t *d_ref, uint32_t *d_new_idx, uint64_t *d_n_new, void *d_dst, size_t dst_bytes, uint32_t *d_sizes,
                                          size_t *nchunks, void *stream)
{
    return dev_cdc_dedupe_compress(x, p, comp_alg, d_src, nbytes, final, base, d_offsets, max_offsets, d_nchunks, d_digests, d_ref, d_new_idx, d_n_new,
                                   d_dst, dst_bytes, d_sizes, nchunks, (hipStream_t)stream, nullptr);
}

extern "C" int cw_dev_cdc_streams_dedupe_compress(cw_dedupe_t *x, const cw_cdc_params *p, int comp_alg, const void *d_src, size_t nbytes,
                                                  const uint64_t *d_ends, size_t nstreams, uint64_t base, uint64_t *d_offsets, size_t max_offsets,
                                                  uint64_t *d_nchunks, uint64_t *d_stream_first, uint64_t *d_result, void *d_digests,
                                                  uint64_t *d_ref, uint32_t *d_new_idx, uint64_t *d_n_new, void *d_dst, size_t dst_bytes,
                                                  uint32_t *d_sizes, size_t *nchunks, void *stream)
{
    const StreamList sl{d_ends, nstreams, d_stream_first, d_result};
    return dev_cdc_dedupe_compress(x, p, comp_alg, d_src, nbytes, 1, base, d_offsets, max_offsets, d_nchunks, d_digests, d_ref, d_new_idx, d_n_new,
                                   d_dst, dst_bytes, d_sizes, nchunks, (hipStream_t)stream, nullptr, &sl);
}

extern "C" int cw_dev_cdc_streams_part_dedupe_compress(cw_dedupe_t *x, const cw_cdc_params *p, int comp_alg, const void *d_src, size_t nbytes,
                                                       const uint64_t *d_ends, size_t nstreams, int final, uint64_t base, uint64_t *d_offsets,
                                                       size_t max_offsets, uint64_t *d_nchunks, uint64_t *d_stream_first, uint64_t *d_result,
                                                       void *d_digests, uint64_t *d_ref, uint32_t *d_new_idx, uint64_t *d_n_new, void *d_dst,
                                                       size_t dst_bytes, uint32_t *d_sizes, size_t *nchunks, void *stream)
{
    const StreamList sl{d_ends, nstreams, d_stream_first, d_result, final ? 1 : 0};
    return dev_cdc_dedupe_compress(x, p, comp_alg, d_src, nbytes, 1, base, d_offsets, max_offsets, d_nchunks, d_digests, d_ref, d_new_idx, d_n_new,
                                   d_dst, dst_bytes, d_sizes, nchunks, (hipStream_t)stream, nullptr, &sl);
}
