// cw_ingest.hip -- the chunk store's host-buffer calls (DESIGN.md sections 18 and 21; semantics: the public header): cw_store_ingest
// streams a host buffer of any size through the device in pieces, cw_store_ingest_streams does the same over many host streams,
// cw_store_restore streams a recipe back in windows, and cw_dev_ingest_commit / cw_dev_ingest_commit_streams are the device step that
// assembles a recipe piece by piece (kernels: ingest_kernels.hip).  cw_store_patch edits a stored stream in place (DESIGN.md section 25;
// struct Patch, one piece of the same kind over a window rebuilt on the device), with cw_dev_cdc_resync as its device step (kernels:
// patch_kernels.hip).  cw_store_compose builds a stream from ranges of stored streams and new bytes (struct
// Compose: rounds that only chunk the windows between the kept ranges, then one piece over everything rebuilt), with
// cw_dev_cdc_resync_windows and cw_dev_scatter_extents as its device steps (kernels: compose_kernels.hip).
//
// Both ingests are one loop (struct Ingest) over a list of host spans; cw_store_ingest's one buffer is a single span.  With the stream
// index (cw_store_ingest_streams) a piece is chunked by cw_dev_cdc_streams_part with the stream ends that fall into it and committed by
// cw_dev_ingest_commit_streams, and its ends are copied on the kernel stream in front of its kernels, since their rebasing needs the
// carry; without it a piece is chunked by cw_dev_cdc and committed by cw_dev_ingest_commit.
//
// Ingest, piece i in buffer b = i & 1 (F = max_size rounded up to 256, P = the fresh bytes per piece):
//     s_h2d    wait ev_done[b] (piece i-2 has left the buffer) | fresh bytes -> buf[b] + F | record ev_up[b]
//     stream   [ends -> device] | wait ev_up[b] | cdc, hash, counts | SYNCHRONISE, admit | dedupe, codec, append, commit
//              | carry -> buf[b^1] + F - carry | record ev_done[b]
// The upload of piece i+1 is queued before piece i's kernels, so it runs beside them; its address does not depend on any count.
// Restore, window w in buffer b = w & 1:
//     s_h2d    count | refs | rebased offsets -> meta[b] | record ev_up[b]
//     stream   wait ev_up[b] | restore into src[b] | record ev_kernel[b]
//     s_d2h    wait ev_kernel[b] | bytes and statuses -> host | record ev_done[b]
// and the host takes window w-2 out of its buffer (waiting for ev_done[b]) before it queues window w into it.

#include <string.h>

#include <vector>

#include "cw_host.h"

using namespace cw::host;

int cw::host::StoreCtx::open()
{
    if (ev_up[0]) return CW_OK;
    for (int b = 0; b < 2; b++) {
        HIP_TRY(hipEventCreateWithFlags(&ev_up[b], hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&ev_done[b], hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&ev_kernel[b], hipEventDisableTiming));
    }
    return CW_OK;
}

void cw::host::StoreCtx::release()
{
    for (int b = 0; b < 2; b++) {
        src[b].release(); meta[b].release(); status[b].release();
        stage[b].release(); h_meta[b].release(); h_status[b].release();
        if (ev_up[b]) (void)hipEventDestroy(ev_up[b]);
        if (ev_done[b]) (void)hipEventDestroy(ev_done[b]);
        if (ev_kernel[b]) (void)hipEventDestroy(ev_kernel[b]);
        ev_up[b] = ev_done[b] = ev_kernel[b] = nullptr;
    }
    off.release(); dig.release(); ref.release(); new_idx.release(); sizes.release(); slots.release();
    rec_ref.release(); rec_off.release(); words.release(); h_words.release();
    ends.release(); first.release(); rec_first.release(); h_ends.release();
}

namespace {

const size_t kDefaultPiece = (size_t)256 << 20; // the fresh bytes per piece (CW_STORE_PIECE): the piece of cw_cdc_hash
const size_t kWindowPositions = (size_t)1 << 24; // positions per restore window at most (empty positions take no bytes)

// u64 words of StoreCtx::words (device) and h_words (pinned)
// (W_COUNTS: four on the device, five on the host, where the fifth takes W_ENDS, the verdict on a piece's stream ends)
// (W_RESYNC: cw_store_patch's four words of cw_dev_cdc_resync)
enum { W_NCHUNKS = 0, W_NNEW = 1, W_RESULT = 2, W_COUNTS = 4, W_VERDICT = 9, W_REC_COUNT = 10, W_ENDS = 11, W_RESYNC = 12, W_STATS = 16, W_WORDS = 24 };

// the bytes of a piece (ingest) or a window (restore, scrub): CW_STORE_PIECE or the default, and no less than `floor`
size_t piece_bytes(size_t floor)
{
    const long knob = cw::knobs().store_piece;
    const size_t piece = knob ? (size_t)knob : kDefaultPiece;
    return piece < floor ? floor : piece;
}

int check_store(const cw_store *st)
{
    if (!st) return fail(CW_ERR_BAD_ARG, "NULL store");
    if (!st->d_used || !st->d_dir || (st->store_bytes && !st->d_store)) return fail(CW_ERR_BAD_ARG, "NULL pointer in the store");
    if (st->dir_entries == 0) return fail(CW_ERR_BAD_ARG, "dir_entries is 0");
    if ((uintptr_t)st->d_dir & 15) return fail(CW_ERR_BAD_ARG, "d_dir is not 16-byte aligned");
    if ((uintptr_t)st->d_used & 7) return fail(CW_ERR_BAD_ARG, "d_used not 8-byte aligned");
    return CW_OK;
}

// whatever happens, nothing of the call is in flight when it returns: the caller's buffers and the staging are free again
void drain(hipStream_t s, hipStream_t s_copy)
{
    (void)hipStreamSynchronize(s_copy);
    (void)hipStreamSynchronize(s);
}

// the admission of one piece (PieceAdmit::admit): the last commit went through, the directory holds [base_k, base_k + k), and the
// store holds the piece even if every chunk of it were new and kept raw
struct Admission {
    const cw_store *st;
    uint64_t base_k;
};
int admit_piece(void *self, size_t k, const uint64_t *h)
{
    const Admission &a = *static_cast<const Admission *>(self);
    const cw_store &st = *a.st;
    const uint64_t consumed = h[1], used = h[2];
    if (h[3]) return fail(CW_ERR_STATE, "cw_store_ingest: an admitted piece was not committed (verdict %llu)", (unsigned long long)h[3]);
    if (k && (a.base_k < st.dir_base || a.base_k - st.dir_base > st.dir_entries || k > st.dir_entries - (a.base_k - st.dir_base)))
        return fail(CW_ERR_NOMEM, "chunk store: values %llu .. +%zu leave the directory [%llu, +%zu)", (unsigned long long)a.base_k, k,
                    (unsigned long long)st.dir_base, st.dir_entries);
    if (used > st.store_bytes || consumed > st.store_bytes - used)
        return fail(CW_ERR_NOMEM, "chunk store: a piece of %llu bytes may not fit behind %llu of %zu", (unsigned long long)consumed,
                    (unsigned long long)used, st.store_bytes);
    return CW_OK;
}

// The pipelined ingest of the concatenation of host spans.  indexed (cw_store_ingest_streams): every span is a stream with an entry in
// the recipe's stream index.  A piece then takes the stream ends not yet taken that lie at or before its end; when the last of them is
// not the piece's end, the piece's own length is one more end and its last stream is open.  Not indexed (cw_store_ingest): the spans are
// one stream, no ends, the plain chunker and the plain commit.
struct Ingest {
    const char *name;                                 // the public call: the prefix of its CW_ERR_STATE messages
    cw_dedupe_t *x; const cw_cdc_params *p; int comp_alg; const cw_store *st;
    const uint8_t *const *srcs; const uint64_t *lens; size_t nspans; uint64_t total, base;
    bool indexed;
    StoreCtx *c = nullptr; hipStream_t s = nullptr, s_h2d = nullptr;
    size_t piece = 0, front = 0, cap = 0, slots_bytes = 0, rec_cap = 0; // P, F, a piece's max_offsets, its slot bytes, the recipe's entries
    size_t most = 1;                                  // the largest stream count of a piece
    size_t k_total = 0; uint64_t done = 0;            // chunks and bytes of the pieces that went in
    size_t taken = 0; uint64_t taken_end = 0;         // indexed: the streams whose end a piece has taken, and the last of those ends
    bool open = false;                                // indexed: the last piece that went in left its last stream open (its entry is written)
    size_t up_f = 0; uint64_t up_at = 0;              // the upload's cursor: the span of the next fresh byte and the byte's place in it

    size_t pieces() const { return (size_t)((total + piece - 1) / piece); }
    uint64_t piece_end(size_t i) const { return total - i * piece < piece ? total : (uint64_t)(i + 1) * piece; }

    // the largest stream count of any piece: the ends a piece takes do not depend on the carries
    size_t most_streams() const
    {
        size_t f = 0, most_ = 1;
        uint64_t cum = 0;
        for (size_t i = 0, n = pieces(); i < n; i++) {
            const uint64_t end = piece_end(i);
            size_t t = 0;
            while (f < nspans && cum + lens[f] <= end) { cum += lens[f++]; t++; }
            const size_t ns = t + (t && cum == end ? 0 : 1);
            if (ns > most_) most_ = ns;
        }
        return most_;
    }

    // The pieces' size and everything they need on the device (total > 0).  With one stream most = 1, and cap, rec_cap and slots_bytes
    // are cw_store_ingest's (max_size + P) / min_size + 2 and nbytes / min_size + 2; with many they are cw_store_ingest_streams'.
    int prepare(const cw::CdcParams &cp)
    {
        piece = piece_bytes(cp.max_size);
        if (piece > total) piece = total > cp.max_size ? (size_t)total : cp.max_size; // one piece: no more than it needs
        front = ((size_t)cp.max_size + 255) & ~(size_t)255;
        most = indexed ? most_streams() : 1;
        cap = (cp.max_size + piece) / cp.min_size + most + 1;
        slots_bytes = cw_chunk_slots_bytes(comp_alg, cp.max_size + piece, cap - 1);
        rec_cap = (size_t)(total / cp.min_size) + nspans + 1;
        // one pageable buffer is staged piece by piece: both staging buffers before the first piece is queued, so that running out of
        // page-locked memory fails the call with nothing ingested (the streams of an indexed call reserve theirs when a piece needs it)
        const bool stage_now = !indexed && !is_pinned(srcs[0]);
        int rc;
        for (size_t b = 0, two = pieces() > 1 ? 2 : 1; b < two; b++) {
            if ((rc = c->src[b].reserve(front + piece + 16)) != CW_OK) return rc; // (+16: the scan loads whole granules)
            if (stage_now && (rc = c->stage[b].reserve(piece)) != CW_OK) return rc;
        }
        if ((rc = c->off.reserve(cap * 8)) != CW_OK || (rc = c->dig.reserve(cap * 64)) != CW_OK || (rc = c->ref.reserve(cap * 8)) != CW_OK ||
            (rc = c->new_idx.reserve(cap * 4)) != CW_OK || (rc = c->sizes.reserve(cap * 4)) != CW_OK || (rc = c->slots.reserve(slots_bytes)) != CW_OK ||
            (rc = c->rec_ref.reserve(rec_cap * 8)) != CW_OK || (rc = c->rec_off.reserve(rec_cap * 8)) != CW_OK)
            return rc;
        if (indexed && ((rc = c->ends.reserve(most * 8)) != CW_OK || (rc = c->first.reserve((most + 1) * 8)) != CW_OK ||
                        (rc = c->h_ends.reserve(most * 8)) != CW_OK || (rc = c->rec_first.reserve((nspans + 1) * 8)) != CW_OK))
            return rc;
        if ((rc = c->words.reserve(W_WORDS * 8)) != CW_OK || (rc = c->h_words.reserve(W_WORDS * 8)) != CW_OK) return rc;
        HIP_TRY(hipMemsetAsync(c->words.p, 0, W_WORDS * 8, s));
        HIP_TRY(hipMemsetAsync(c->rec_off.p, 0, 8, s));
        return CW_OK;
    }

    int upload(size_t i)
    {
        const int b = (int)(i & 1);
        const size_t take = (size_t)(piece_end(i) - (uint64_t)i * piece);
        // the span parts behind the fresh bytes: in place when they lie back to back in page-locked memory (one span: when it is page-locked)
        size_t f = up_f;
        uint64_t at = up_at;
        const uint8_t *first = nullptr, *next = nullptr;
        bool in_place = true;
        for (size_t left = take; left;) {
            while (at == lens[f]) { f++; at = 0; }
            const size_t n = lens[f] - at < left ? (size_t)(lens[f] - at) : left;
            const uint8_t *q = srcs[f] + at;
            if (!first) first = q;
            else if (q != next) in_place = false;
            if (in_place && at == 0 && !is_pinned(q)) in_place = false;
            next = q + n; at += n; left -= n;
        }
        if (in_place && first && !is_pinned(first)) in_place = false; // (the first part may start inside its span)
        const void *from = first;
        if (!in_place) {
            int rc = c->stage[b].reserve(piece);
            if (rc != CW_OK) return rc;
            if (i >= 2) HIP_TRY(hipEventSynchronize(c->ev_up[b])); // the staging buffer's last copy has left it
            uint8_t *to = (uint8_t *)c->stage[b].p;
            f = up_f; at = up_at;
            for (size_t left = take; left;) {
                while (at == lens[f]) { f++; at = 0; }
                const size_t n = lens[f] - at < left ? (size_t)(lens[f] - at) : left;
                memcpy(to, srcs[f] + at, n);
                to += n; at += n; left -= n;
            }
            from = c->stage[b].p;
        }
        up_f = f; up_at = at;
        if (i >= 2) HIP_TRY(hipStreamWaitEvent(s_h2d, c->ev_done[b], 0));
        HIP_TRY(hipMemcpyAsync((uint8_t *)c->src[b].p + front, from, take, hipMemcpyHostToDevice, s_h2d));
        HIP_TRY(hipEventRecord(c->ev_up[b], s_h2d));
        return CW_OK;
    }

    // CW_OK with *refused set: the piece did not go in and nothing changed
    int run(bool *refused)
    {
        uint64_t *w = (uint64_t *)c->words.p, *h = (uint64_t *)c->h_words.p, *h_ends = (uint64_t *)c->h_ends.p;
        const size_t n = pieces();
        size_t carry = 0;
        int rc = upload(0);
        for (size_t i = 0; rc == CW_OK && i < n; i++) {
            const int b = (int)(i & 1);
            if (i + 1 < n && (rc = upload(i + 1)) != CW_OK) return rc;
            const uint64_t end = piece_end(i);
            const size_t take = (size_t)(end - (uint64_t)i * piece), len = carry + take;
            // indexed, the piece's streams: the ends it takes, rebased to its origin (= done), and its own length when its last stream
            // stays open.  closed: the chunker cuts at the piece's end
            size_t t = 0, ns = 0;
            uint64_t cum = taken_end;
            bool closed = i + 1 == n;
            if (indexed) {
                if (done + len != end) return fail(CW_ERR_STATE, "%s: piece %zu does not start where the last one stopped", name, i);
                while (taken + t < nspans && cum + lens[taken + t] <= end) { cum += lens[taken + t]; h_ends[t++] = cum - done; }
                closed = t && cum == end;
                if (!closed) h_ends[t] = len;
                ns = t + (closed ? 0 : 1);
                if (ns > most) return fail(CW_ERR_STATE, "%s: %zu streams in a piece sized for %zu", name, ns, most);
                HIP_TRY(hipMemcpyAsync(c->ends.p, h_ends, ns * 8, hipMemcpyHostToDevice, s)); // (the last piece's copy left h_ends before its synchronise)
            }
            uint8_t *d_piece = (uint8_t *)c->src[b].p + front - carry;
            HIP_TRY(hipStreamWaitEvent(s, c->ev_up[b], 0));
            Admission a{st, base + k_total};
            bool inserted = false;
            PieceAdmit hook{st->d_used, w + W_VERDICT, w + W_COUNTS, h + W_COUNTS, admit_piece, &a, &inserted};
            const StreamList sl{(const uint64_t *)c->ends.p, ns, (uint64_t *)c->first.p, w + W_ENDS, closed ? 1 : 0};
            size_t k = 0;
            rc = dev_cdc_dedupe_compress(x, p, comp_alg, d_piece, len, closed, a.base_k, (uint64_t *)c->off.p, cap, w + W_NCHUNKS, c->dig.p,
                                         (uint64_t *)c->ref.p, (uint32_t *)c->new_idx.p, w + W_NNEW, c->slots.p, slots_bytes, (uint32_t *)c->sizes.p, &k,
                                         s, &hook, indexed ? &sl : nullptr);
            if (rc == CW_ERR_NOMEM && !inserted) { *refused = true; return CW_OK; }
            if (rc == CW_ERR_NOMEM) return fail(CW_ERR_STATE, "%s: device memory ran out behind an admitted piece", name);
            if (indexed && rc == CW_ERR_BAD_ARG) return fail(CW_ERR_STATE, "%s: the ends of piece %zu were refused", name, i);
            if (rc != CW_OK) return rc;
            rc = cw_dev_store_chunks(comp_alg, d_piece, len, (uint64_t *)c->off.p, w + W_NCHUNKS, cap - 1, (uint32_t *)c->new_idx.p, w + W_NNEW,
                                     c->slots.p, (uint32_t *)c->sizes.p, a.base_k, st->d_store, st->store_bytes, st->d_used, st->d_dir, st->dir_base,
                                     st->dir_entries, w + W_RESULT, s);
            if (rc == CW_OK && indexed)
                rc = cw_dev_ingest_commit_streams((uint64_t *)c->ref.p, (uint64_t *)c->off.p, w + W_NCHUNKS, cap - 1, w + W_NNEW, w + W_RESULT, done,
                                                  (uint64_t *)c->rec_ref.p, (uint64_t *)c->rec_off.p, w + W_REC_COUNT, rec_cap, w + W_STATS,
                                                  w + W_VERDICT, (const uint64_t *)c->first.p, ns, taken, open ? 1 : 0, (uint64_t *)c->rec_first.p,
                                                  nspans + 1, s);
            else if (rc == CW_OK)
                rc = cw_dev_ingest_commit((uint64_t *)c->ref.p, (uint64_t *)c->off.p, w + W_NCHUNKS, cap - 1, w + W_NNEW, w + W_RESULT, done,
                                          (uint64_t *)c->rec_ref.p, (uint64_t *)c->rec_off.p, w + W_REC_COUNT, rec_cap, w + W_STATS, w + W_VERDICT, s);
            if (rc != CW_OK) return rc == CW_ERR_NOMEM ? fail(CW_ERR_STATE, "%s: no scratch behind an admitted piece", name) : rc;
            const size_t consumed = (size_t)h[W_COUNTS + 1];
            if (indexed && closed && consumed != len) return fail(CW_ERR_STATE, "%s: a closed piece of %zu bytes consumed %zu", name, len, consumed);
            if (i + 1 < n) { // the bytes behind the last cut (< max_size) go in front of the next piece's fresh bytes
                carry = len - consumed;
                if (carry > front) return fail(CW_ERR_STATE, "%s: a carry of %zu bytes", name, carry);
                if (carry) HIP_TRY(hipMemcpyAsync((uint8_t *)c->src[b ^ 1].p + front - carry, d_piece + consumed, carry, hipMemcpyDeviceToDevice, s));
            }
            HIP_TRY(hipEventRecord(c->ev_done[b], s));
            k_total += k;
            done += consumed;
            if (indexed) { taken += t; taken_end = cum; open = !closed; }
        }
        return rc;
    }

    // The pieces, and what they left: *k chunks, their refs and offsets[0 .. *k] and the statistics, with nothing of the call in flight.
    // CW_OK with *refused set: a piece was refused, and the recipe is that of the pieces before it
    int run_and_collect(uint64_t *refs, uint64_t *offsets, size_t max_offsets, cw_ingest_stats *stats, size_t *k, bool *refused)
    {
        int rc = run(refused);
        uint64_t *h = (uint64_t *)c->h_words.p;
        if (rc == CW_OK) {
            const hipError_t e = hipMemcpyAsync(h + W_VERDICT, (uint64_t *)c->words.p + W_VERDICT, (W_WORDS - W_VERDICT) * 8, hipMemcpyDeviceToHost, s);
            if (e != hipSuccess) rc = fail(CW_ERR_HIP, "%s: the counts: %s", name, hipGetErrorString(e));
        }
        drain(s, s_h2d);
        if (rc != CW_OK) return rc;
        *k = (size_t)h[W_REC_COUNT];
        if (h[W_VERDICT] || *k != k_total || *k + 1 > max_offsets)
            return fail(CW_ERR_STATE, "%s: an admitted piece was not committed (verdict %llu, %zu of %zu chunks)", name, (unsigned long long)h[W_VERDICT],
                        *k, k_total);
        if (*k) HIP_TRY(hipMemcpy(refs, c->rec_ref.p, *k * 8, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(offsets, c->rec_off.p, (*k + 1) * 8, hipMemcpyDeviceToHost));
        if (stats) memcpy(stats, h + W_STATS, 5 * sizeof(uint64_t));
        return CW_OK;
    }
};

// One edit of a stored stream (cw_store_patch).  An attempt is one piece of Ingest's kind -- the same fused call
// with the same admission -- over a window rebuilt on the device instead of uploaded, with cw_dev_cdc_resync behind the chunker:
//     stream   count | ranges | refs | rebased cuts -> meta[0] | read ranges into src[0] around the insert | insert -> src[0] + head
//              | cdc, resync, hash, counts | SYNCHRONISE: statuses, verdict, admit | dedupe, codec, append | refs, cuts -> host
// Everything is queued on the context's kernel stream.  meta[0], in u64 words: the count of uploaded positions, the range count (2),
// the ranges' offsets, lengths and destinations, the refs of positions [j, e) and the cuts of [j, e] rebased to c_j.
struct Patch {
    enum { M_COUNT = 0, M_NRANGES = 1, M_ROFF = 2, M_RLEN = 4, M_RDST = 6, M_REFS = 8 };
    cw_dedupe_t *x; const cw_cdc_params *p; int comp_alg; const cw_store *st;
    const uint64_t *refs, *offsets; size_t K;
    uint64_t a, remove; const uint8_t *insert; size_t ins; uint64_t base; size_t max_out;
    StoreCtx *c = nullptr; hipStream_t s = nullptr;
    size_t j = 0, e = 0, cap = 0;                    // the attempt: old positions [j, e) lie in the window; its max_offsets
    uint64_t head = 0, tail = 0, wb = 0;             // the old bytes in front of and behind the insert, and the window's bytes
    bool final_ = false, retry = false, unrestored = false;
    size_t k = 0, resume = 0;                        // what the attempt keeps: k window chunks, then old positions [resume, K)

    uint64_t cut(size_t i) const { return offsets[i] - offsets[0]; }
    uint64_t *meta() const { return (uint64_t *)c->meta[0].p; }

    // j and e for a lookahead: c_j <= a (the last chunk when a is the end), c_e = W >= b.  CW_ERR_BAD_ARG when [j, e] does not ascend
    int locate(uint64_t look)
    {
        const uint64_t n = cut(K), b = a + remove;
        size_t lo = 0, hi = K; // the last i in [0, K] with cut(i) <= a
        while (lo < hi) {
            const size_t mid = lo + (hi - lo + 1) / 2;
            if (cut(mid) <= a) lo = mid;
            else hi = mid - 1;
        }
        j = K && lo == K ? K - 1 : lo;
        lo = j; hi = K; // the first i in [j, K] with cut(i) >= b + look, or K
        if (look <= n - b)
            while (lo < hi) {
                const size_t mid = lo + (hi - lo) / 2;
                if (cut(mid) >= b + look) hi = mid;
                else lo = mid + 1;
            }
        e = hi;
        for (size_t i = j; i < e; i++)
            if (offsets[i + 1] < offsets[i]) return fail(CW_ERR_BAD_ARG, "offsets decrease at position %zu", i);
        if (cut(j) > a || cut(e) < b || (K && e <= j)) return fail(CW_ERR_BAD_ARG, "offsets do not ascend around position %zu", j);
        final_ = e == K;
        head = a - cut(j); tail = cut(e) - b; wb = head + ins + tail;
        return CW_OK;
    }

    static int after_cdc(void *self, hipStream_t s)
    {
        Patch &t = *static_cast<Patch *>(self);
        uint64_t *w = (uint64_t *)t.c->words.p, *h = (uint64_t *)t.c->h_words.p, *m = t.meta();
        const size_t np = t.e - t.j;
        int rc = cw_dev_cdc_resync((uint64_t *)t.c->off.p, w + W_NCHUNKS, t.cap - 1, m + M_REFS + np, m + M_COUNT, np, t.head + t.ins,
                                   t.remove - (uint64_t)t.ins, t.final_ ? 1 : 0, w + W_RESYNC, s);
        if (rc != CW_OK) return rc;
        HIP_TRY(hipMemcpyAsync(h + W_RESYNC, w + W_RESYNC, 4 * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(t.c->h_status[0].p, t.c->status[0].p, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        return CW_OK;
    }

    // behind the attempt's synchronise, before anything is inserted: the window was read, it ends (a resync, or the stream's end), the
    // recipe fits, and the kept chunks are admitted as a piece of cw_store_ingest is
    static int admit(void *self, size_t k, const uint64_t *hc)
    {
        Patch &t = *static_cast<Patch *>(self);
        const uint64_t *r = (const uint64_t *)t.c->h_words.p + W_RESYNC;
        const uint32_t *got = (const uint32_t *)t.c->h_status[0].p;
        if (got[0] || got[1]) {
            t.unrestored = true;
            return fail(CW_ERR_BAD_ARG, "cw_store_patch: the window's old bytes were not read (statuses %u, %u)", got[0], got[1]);
        }
        if (r[0] && !t.final_) {
            t.retry = true;
            return k ? fail(CW_ERR_STATE, "cw_store_patch: %zu chunks kept without a resync", k) : CW_OK;
        }
        if (!r[0] && (r[1] != k || r[2] > t.e - t.j)) return fail(CW_ERR_STATE, "cw_store_patch: resync at %llu, %zu chunks kept", (unsigned long long)r[1], k);
        t.k = k;
        t.resume = r[0] ? t.K : t.j + (size_t)r[2];
        if (t.j + k + (t.K - t.resume) + 1 > t.max_out) return fail(CW_ERR_STATE, "cw_store_patch: %zu chunks do not fit max_out %zu", t.j + k + (t.K - t.resume), t.max_out);
        Admission adm{t.st, t.base};
        return admit_piece(&adm, k, hc);
    }

    // the first position of the window that does not restore, for the message: the window's positions once more, whole
    int diagnose()
    {
        const size_t np = e - j;
        const uint64_t bytes = cut(e) - cut(j);
        uint64_t *m = meta();
        if (c->src[1].reserve(bytes + 16) == CW_OK && c->status[1].reserve(np * 4) == CW_OK && c->h_status[1].reserve(np * 4) == CW_OK &&
            cw_dev_restore_chunks(comp_alg, st->d_store, st->store_bytes, st->d_dir, st->dir_base, st->dir_entries, m + M_REFS, m + M_REFS + np,
                                  m + M_COUNT, np, c->src[1].p, bytes, (uint32_t *)c->status[1].p, s) == CW_OK &&
            hipMemcpyAsync(c->h_status[1].p, c->status[1].p, np * 4, hipMemcpyDeviceToHost, s) == hipSuccess && hipStreamSynchronize(s) == hipSuccess) {
            const uint32_t *got = (const uint32_t *)c->h_status[1].p;
            for (size_t i = 0; i < np; i++)
                if (got[i] && (cut(j + i) < a || cut(j + i + 1) > a + remove))
                    return fail(CW_ERR_BAD_ARG, "cw_store_patch: position %zu (ref %llu) does not restore: status %u", j + i,
                                (unsigned long long)refs[j + i], got[i]);
        }
        const uint32_t *got = (const uint32_t *)c->h_status[0].p;
        return fail(CW_ERR_BAD_ARG, "cw_store_patch: a position in [%zu, %zu) does not restore (which one could not be determined): statuses %u, %u of "
                                    "the bytes in front of and behind the edit", j, e, got[0], got[1]);
    }

    // one attempt: CW_OK with retry set = no resync in a window that is not final, nothing changed
    int attempt(const cw::CdcParams &cp, uint64_t *out_refs, uint64_t *out_offsets, cw_patch_stats *stats)
    {
        const size_t np = e - j;
        int rc;
        if (wb / cp.min_size > SIZE_MAX - 2) return fail(CW_ERR_NOMEM, "cw_store_patch: a window of %llu bytes", (unsigned long long)wb);
        cap = (size_t)(wb / cp.min_size) + 2;
        if (check_count("window chunks", cap) != CW_OK || check_count("window positions", np) != CW_OK)
            return fail(CW_ERR_NOMEM, "cw_store_patch: a window of %llu bytes and %zu positions", (unsigned long long)wb, np);
        const size_t slots_bytes = cw_chunk_slots_bytes(comp_alg, wb, cap - 1), meta_words = M_REFS + 2 * np + 1;
        if ((rc = c->src[0].reserve(wb + 16)) != CW_OK || (rc = c->off.reserve(cap * 8)) != CW_OK || (rc = c->dig.reserve(cap * 64)) != CW_OK ||
            (rc = c->ref.reserve(cap * 8)) != CW_OK || (rc = c->new_idx.reserve(cap * 4)) != CW_OK || (rc = c->sizes.reserve(cap * 4)) != CW_OK ||
            (rc = c->slots.reserve(slots_bytes)) != CW_OK || (rc = c->meta[0].reserve(meta_words * 8)) != CW_OK ||
            (rc = c->h_meta[0].reserve(meta_words * 8)) != CW_OK || (rc = c->h_meta[1].reserve(2 * cap * 8)) != CW_OK || (rc = c->status[0].reserve(8)) != CW_OK || (rc = c->h_status[0].reserve(8)) != CW_OK ||
            (rc = c->words.reserve(W_WORDS * 8)) != CW_OK || (rc = c->h_words.reserve(W_WORDS * 8)) != CW_OK)
            return rc;
        uint64_t *w = (uint64_t *)c->words.p, *h = (uint64_t *)c->h_words.p, *m = (uint64_t *)c->h_meta[0].p, *d_m = meta();
        uint8_t *window = (uint8_t *)c->src[0].p;
        const uint64_t cj = cut(j);
        m[M_COUNT] = np; m[M_NRANGES] = 2;
        m[M_ROFF] = 0; m[M_RLEN] = head; m[M_RDST] = 0;
        m[M_ROFF + 1] = a + remove - cj; m[M_RLEN + 1] = tail; m[M_RDST + 1] = head + ins;
        if (np) memcpy(m + M_REFS, refs + j, np * 8);
        for (size_t i = 0; i <= np; i++) m[M_REFS + np + i] = cut(j + i) - cj;
        HIP_TRY(hipMemsetAsync(w, 0, W_WORDS * 8, s));
        HIP_TRY(hipMemsetAsync(c->status[0].p, 0, 8, s));
        HIP_TRY(hipMemcpyAsync(d_m, m, meta_words * 8, hipMemcpyHostToDevice, s));
        if (np && (head || tail) &&
            (rc = cw_dev_read_ranges(comp_alg, st->d_store, st->store_bytes, st->d_dir, st->dir_base, st->dir_entries, d_m + M_REFS, d_m + M_REFS + np,
                                     d_m + M_COUNT, np, d_m + M_ROFF, d_m + M_RLEN, d_m + M_RDST, d_m + M_NRANGES, 2, window, wb,
                                     (uint32_t *)c->status[0].p, s)) != CW_OK)
            return rc;
        if (ins) HIP_TRY(hipMemcpyAsync(window + head, insert, ins, hipMemcpyHostToDevice, s));
        bool inserted = false;
        retry = unrestored = false;
        PieceAdmit hook{st->d_used, w + W_VERDICT, w + W_COUNTS, h + W_COUNTS, admit, this, &inserted, after_cdc};
        size_t found = 0;
        rc = dev_cdc_dedupe_compress(x, p, comp_alg, window, wb, final_ ? 1 : 0, base, (uint64_t *)c->off.p, cap, w + W_NCHUNKS, c->dig.p,
                                     (uint64_t *)c->ref.p, (uint32_t *)c->new_idx.p, w + W_NNEW, c->slots.p, slots_bytes, (uint32_t *)c->sizes.p, &found,
                                     s, &hook);
        if (unrestored) return diagnose();
        if (rc == CW_ERR_NOMEM && inserted) return fail(CW_ERR_STATE, "cw_store_patch: device memory ran out behind an admitted window");
        if (rc != CW_OK || retry) return rc;
        rc = cw_dev_store_chunks(comp_alg, window, wb, (uint64_t *)c->off.p, w + W_NCHUNKS, cap - 1, (uint32_t *)c->new_idx.p, w + W_NNEW, c->slots.p,
                                 (uint32_t *)c->sizes.p, base, st->d_store, st->store_bytes, st->d_used, st->d_dir, st->dir_base, st->dir_entries,
                                 w + W_RESULT, s);
        if (rc != CW_OK) return rc == CW_ERR_NOMEM ? fail(CW_ERR_STATE, "cw_store_patch: no scratch behind an admitted window") : rc;
        // the kept refs and cuts come down on the same stream into pinned memory (k <= cap - 1 is known since the admission): one more
        // synchronise, and no copy on the null stream, which would wait for every other thread's stream
        uint64_t *h_ref = (uint64_t *)c->h_meta[1].p, *h_off = h_ref + cap;
        HIP_TRY(hipMemcpyAsync(h + W_NNEW, w + W_NNEW, 3 * sizeof(uint64_t), hipMemcpyDeviceToHost, s)); // (W_NNEW, W_RESULT[2])
        if (k) HIP_TRY(hipMemcpyAsync(h_ref, c->ref.p, k * 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(h_off, c->off.p, (k + 1) * 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        if (h[W_RESULT]) return fail(CW_ERR_STATE, "cw_store_patch: an admitted window was not stored (verdict %llu)", (unsigned long long)h[W_RESULT]);
        // the splice: old positions [0, j), the window's k chunks, old positions [resume, K) shifted by delta
        if (k) memcpy(out_refs + j, h_ref, k * 8);
        for (size_t i = 0; i <= k; i++) out_offsets[j + i] = h_off[i] + cj;
        stats->window_bytes = wb; stats->window_chunks = k; stats->new_chunks = h[W_NNEW]; stats->stored_bytes = h[W_RESULT + 1];
        return CW_OK;
    }
};

// A stream composed from ranges of stored streams and new bytes (cw_store_compose).  The plan is the host's:
// the copies merged and split at A's stream ends, the anchors [p, q) by binary search, a window in front of every anchor and a final
// one behind the last.  A round materialises the unresolved windows back to back in src[0] and only chunks them:
//     stream   lists -> meta[1] | read ranges of A into src[0] | scatter the new bytes out of src[1] | cdc_streams | resync_windows
//              | statuses, results, words -> host | SYNCHRONISE
// and the commit is one piece of Ingest's kind over the rebuilt extents of all windows, each a stream of its own:
//     stream   lists | read ranges | scatter | cdc_streams, hash, counts | SYNCHRONISE: statuses, stream index, admit | dedupe, codec,
//              append | refs, cuts -> host | SYNCHRONISE
// src[1] holds the payload and meta[0] the recipe of A (count | refs | zero-based cuts), both uploaded once.
struct Compose {
    struct Anchor { uint64_t b, d; size_t p, q; };   // a copy piece at b of B with keepable positions [p, q) of A; d = a - b (mod 2^64)
    struct Window {
        uint64_t start; long anchor;                 // where it starts in B; the anchor it runs into, -1 for the final window
        uint64_t look;
        bool resolved = false, discard = false, ran = false, exhausted = false;
        uint64_t t = 0, end = 0; size_t s = 0;       // resolved: t chunks in [start, end), then positions [s, q) of the anchor
        uint64_t at = 0, tried = 0; size_t slot = 0; // the round: where it lies in src[0], where it ends in B, its index among the round's
    };
    struct Span { uint64_t start, end; };            // a stretch of B to materialise
    cw_dedupe_t *x; const cw_cdc_params *p; int comp_alg; const cw_store *st;
    const uint64_t *refs; size_t K; const uint64_t *stream_first; size_t nstreams;
    const cw_delta_op *ops; size_t nops; const uint8_t *payload; size_t payload_bytes;
    uint64_t base, nb, look0; size_t max_out;
    cw_compose_stats *stats;
    StoreCtx *c = nullptr; hipStream_t s = nullptr;
    std::vector<uint64_t> cuts, lists;               // A's zero-based cuts; a round's lists on their way up
    std::vector<Anchor> anchors;
    std::vector<Window> wins;
    std::vector<Span> spans;
    size_t nranges = 0, next = 0, cap = 0, slots_bytes = 0; uint64_t total = 0; // of the spans materialised last
    bool uploaded = false, unread = false;

    uint64_t in_b(const Anchor &a, size_t i) const { return cuts[i] - a.d; } // cut i of A in B's coordinates, through anchor a
    // the first i in [lo, hi) with v[i] >= x, hi when there is none
    static size_t lower(const std::vector<uint64_t> &v, size_t lo, size_t hi, uint64_t x)
    {
        while (lo < hi) {
            const size_t mid = lo + (hi - lo) / 2;
            if (v[mid] < x) lo = mid + 1;
            else hi = mid;
        }
        return lo;
    }
    bool ends_stream(size_t q) const // position q - 1 is the last of its stream
    {
        if (!stream_first) return q == K;
        size_t lo = 1, hi = nstreams + 1;
        while (lo < hi) {
            const size_t mid = lo + (hi - lo) / 2;
            if (stream_first[mid] < q) lo = mid + 1;
            else hi = mid;
        }
        return lo <= nstreams && stream_first[lo] == q;
    }

    void add_piece(uint64_t b, uint64_t n, uint64_t a)
    {
        size_t pp = lower(cuts, 0, K + 1, a), q = lower(cuts, 0, K + 1, a + n); // (a + n <= cuts[K]: the ops were checked)
        if (cuts[q] != a + n) q--;                                               // the last cut at or below a + n
        if (q > pp && ends_stream(q) && cuts[q] - a + b != nb) q--;
        if (q > pp) anchors.push_back(Anchor{b, a - b, pp, q});
    }

    // merged copies, split at the stream ends of A that lie inside them
    void add_copy(uint64_t b, uint64_t n, uint64_t a)
    {
        uint64_t lo = a;
        for (size_t f = 1; stream_first && f < nstreams; f++) { // (the ends ascend with f)
            const uint64_t e = cuts[stream_first[f]];
            if (e <= lo) continue;
            if (e >= a + n) break;
            add_piece(b + (lo - a), e - lo, lo);
            lo = e;
        }
        add_piece(b + (lo - a), a + n - lo, lo);
    }

    void plan()
    {
        bool open = false;
        uint64_t mb = 0, mn = 0, ma = 0;
        for (size_t k = 0; k < nops; k++) {
            const cw_delta_op &o = ops[k];
            if (o.a_off == CW_DELTA_NONE) continue;
            if (open && mb + mn == o.b_off && ma + mn == o.a_off) { mn += o.len; continue; }
            if (open) add_copy(mb, mn, ma);
            open = true; mb = o.b_off; mn = o.len; ma = o.a_off;
        }
        if (open) add_copy(mb, mn, ma);
        uint64_t start = 0;
        for (size_t i = 0; i < anchors.size(); i++) {
            const Anchor &a = anchors[i];
            Window w{start, (long)i, look0};
            if (in_b(a, a.p) == start) { w.resolved = true; w.s = a.p; w.end = start; } // kept from where the region starts: no window
            else stats->windows++;
            wins.push_back(w);
            start = in_b(a, a.q);
        }
        if (start < nb) { wins.push_back(Window{start, -1, look0}); stats->windows++; }
    }

    // the recipe of A and the payload, once, in front of the first device work
    int upload()
    {
        if (uploaded) return CW_OK;
        int rc;
        if ((rc = check_count("nchunks", K)) != CW_OK) return fail(CW_ERR_NOMEM, "cw_store_compose: a source of %zu positions", K);
        if ((rc = c->meta[0].reserve((2 * K + 2) * 8)) != CW_OK || (rc = c->src[1].reserve(payload_bytes + 16)) != CW_OK ||
            (rc = c->words.reserve(W_WORDS * 8)) != CW_OK || (rc = c->h_words.reserve(W_WORDS * 8)) != CW_OK)
            return rc;
        uint64_t *m = (uint64_t *)c->meta[0].p;
        const uint64_t count = K;
        HIP_TRY(hipMemcpyAsync(m, &count, 8, hipMemcpyHostToDevice, s));
        if (K) HIP_TRY(hipMemcpyAsync(m + 1, refs, K * 8, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(m + 1 + K, cuts.data(), (K + 1) * 8, hipMemcpyHostToDevice, s));
        if (payload_bytes) HIP_TRY(hipMemcpyAsync(c->src[1].p, payload, payload_bytes, hipMemcpyHostToDevice, s));
        HIP_TRY(hipStreamSynchronize(s)); // (`count` leaves the stack)
        uploaded = true;
        return CW_OK;
    }

    // Queues what fills src[0] with the spans' bytes back to back, and reserves what a chunker over them needs.  lists, in u64 words:
    // nranges | next | range offsets, lengths, destinations [nranges each] | extents [3 * next] | the spans' ends [n] | `extra` words
    int materialise(size_t extra, uint64_t **d_ends, uint64_t **d_extra, std::vector<uint64_t> **host)
    {
        const size_t n = spans.size();
        std::vector<uint64_t> roff, rlen, rdst, ext, ends;
        total = 0;
        for (const Span &sp : spans) {
            size_t lo = 0, hi = nops; // the op that holds byte sp.start
            while (hi - lo > 1) {
                const size_t mid = lo + (hi - lo) / 2;
                if (ops[mid].b_off <= sp.start) lo = mid;
                else hi = mid;
            }
            for (size_t k = lo; k < nops && ops[k].b_off < sp.end; k++) {
                const cw_delta_op &o = ops[k];
                const uint64_t from = o.b_off > sp.start ? o.b_off : sp.start, to = o.b_off + o.len < sp.end ? o.b_off + o.len : sp.end;
                if (from >= to) continue;
                const uint64_t dst = total + (from - sp.start);
                if (o.a_off != CW_DELTA_NONE) { roff.push_back(o.a_off + (from - o.b_off)); rlen.push_back(to - from); rdst.push_back(dst); }
                else { ext.push_back(o.payload_off + (from - o.b_off)); ext.push_back(dst); ext.push_back(to - from); }
            }
            total += sp.end - sp.start;
            ends.push_back(total);
        }
        nranges = roff.size(); next = ext.size() / 3;
        const cw::CdcParams cp = params();
        if (total / cp.min_size > SIZE_MAX - n - 1) return fail(CW_ERR_NOMEM, "cw_store_compose: windows of %llu bytes", (unsigned long long)total);
        cap = (size_t)(total / cp.min_size) + n + 1;
        if (check_count("window chunks", cap) != CW_OK || check_count("windows", n) != CW_OK || check_count("ranges", nranges) != CW_OK ||
            check_count("extents", next) != CW_OK)
            return fail(CW_ERR_NOMEM, "cw_store_compose: %zu windows of %llu bytes in %zu ranges and %zu extents", n, (unsigned long long)total, nranges, next);
        lists.clear();
        lists.push_back(nranges); lists.push_back(next);
        lists.insert(lists.end(), roff.begin(), roff.end()); lists.insert(lists.end(), rlen.begin(), rlen.end());
        lists.insert(lists.end(), rdst.begin(), rdst.end()); lists.insert(lists.end(), ext.begin(), ext.end());
        const size_t at_ends = lists.size();
        lists.insert(lists.end(), ends.begin(), ends.end());
        const size_t at_extra = lists.size();
        lists.resize(at_extra + extra, 0);
        int rc;
        if ((rc = upload()) != CW_OK) return rc;
        if ((rc = c->src[0].reserve(total + 16)) != CW_OK || (rc = c->meta[1].reserve(lists.size() * 8)) != CW_OK ||
            (rc = c->h_meta[1].reserve(lists.size() * 8)) != CW_OK || (rc = c->off.reserve(cap * 8)) != CW_OK ||
            (rc = c->first.reserve((n + 1) * 8)) != CW_OK || (rc = c->status[0].reserve((nranges + 1) * 4)) != CW_OK ||
            (rc = c->h_status[0].reserve((nranges + 1) * 4)) != CW_OK)
            return rc;
        uint64_t *d = (uint64_t *)c->meta[1].p;
        *d_ends = d + at_ends; *d_extra = d + at_extra; *host = &lists;
        return CW_OK;
    }

    // behind materialise, once the caller has filled the extra words: the lists go up, the bytes are rebuilt
    int fill()
    {
        uint64_t *d = (uint64_t *)c->meta[1].p, *w = (uint64_t *)c->words.p, *m = (uint64_t *)c->meta[0].p;
        memcpy(c->h_meta[1].p, lists.data(), lists.size() * 8);
        HIP_TRY(hipMemsetAsync(w, 0, W_WORDS * 8, s));
        HIP_TRY(hipMemsetAsync(c->status[0].p, 0, (nranges + 1) * 4, s));
        HIP_TRY(hipMemcpyAsync(d, c->h_meta[1].p, lists.size() * 8, hipMemcpyHostToDevice, s));
        int rc;
        if (nranges && (rc = cw_dev_read_ranges(comp_alg, st->d_store, st->store_bytes, st->d_dir, st->dir_base, st->dir_entries, m + 1, m + 1 + K, m, K,
                                                d + 2, d + 2 + nranges, d + 2 + 2 * nranges, d, nranges, c->src[0].p, (size_t)total,
                                                (uint32_t *)c->status[0].p, s)) != CW_OK)
            return rc;
        if (next && (rc = cw_dev_scatter_extents(c->src[1].p, payload_bytes, d + 2 + 3 * nranges, d + 1, next, c->src[0].p, (size_t)total, w + W_RESYNC, s)) != CW_OK)
            return rc;
        return CW_OK;
    }

    // behind the synchronise that brought statuses and words down
    int check_filled()
    {
        const uint64_t *h = (const uint64_t *)c->h_words.p;
        const uint32_t *got = (const uint32_t *)c->h_status[0].p;
        if (next && h[W_RESYNC]) return fail(CW_ERR_STATE, "cw_store_compose: extent %llu of the new bytes was refused", (unsigned long long)h[W_RESYNC + 2]);
        for (size_t r = 0; r < nranges; r++)
            if (got[r]) {
                unread = true;
                return fail(CW_ERR_BAD_ARG, "cw_store_compose: %llu bytes of the source at offset %llu were not read: status %u (a position there does not restore)",
                            (unsigned long long)lists[2 + nranges + r], (unsigned long long)lists[2 + r], got[r]);
            }
        return CW_OK;
    }

    cw::CdcParams params() const { cw::CdcParams cp; (void)cdc_params(p, &cp); return cp; }

    // one round over the unresolved windows; the windows' state afterwards is the model's (tests/compose_model.py)
    int round()
    {
        spans.clear();
        for (Window &w : wins) {
            w.ran = false;
            if (w.resolved) continue;
            if (w.anchor < 0) { w.tried = nb; w.exhausted = false; }
            else {
                const Anchor &a = anchors[(size_t)w.anchor];
                const uint64_t from = (a.b > w.start ? a.b : w.start) - a.b + (a.b + a.d), target = w.look > UINT64_MAX - from ? UINT64_MAX : from + w.look;
                size_t e = lower(cuts, a.p, a.q + 1, target);
                if (e > a.q) e = a.q;
                w.tried = in_b(a, e); w.exhausted = e == a.q;
            }
            w.ran = true; w.slot = spans.size();
            spans.push_back(Span{w.start, w.tried});
        }
        const size_t n = spans.size();
        uint64_t *d_ends, *d_win;
        std::vector<uint64_t> *l;
        int rc = materialise(5 * n, &d_ends, &d_win, &l);
        if (rc != CW_OK) return rc;
        uint64_t *spec = l->data() + (l->size() - 5 * n), at = 0;
        for (Window &w : wins) {
            if (!w.ran) continue;
            w.at = at;
            uint64_t *q = spec + 5 * w.slot;
            if (w.anchor < 0) { q[0] = q[1] = q[2] = q[3] = 0; q[4] = 1; }
            else {
                const Anchor &a = anchors[(size_t)w.anchor];
                q[0] = (a.b > w.start ? a.b : w.start) - w.start + at; q[1] = a.d + w.start - at; q[2] = a.p; q[3] = a.q - a.p; q[4] = w.tried == nb;
            }
            at += w.tried - w.start;
        }
        if ((rc = c->rec_ref.reserve(4 * n * 8)) != CW_OK || (rc = c->h_meta[0].reserve((5 * n + 1) * 8)) != CW_OK || (rc = fill()) != CW_OK) return rc;
        uint64_t *w = (uint64_t *)c->words.p, *h = (uint64_t *)c->h_words.p, *m = (uint64_t *)c->meta[0].p;
        const StreamList sl{d_ends, n, (uint64_t *)c->first.p, w + W_ENDS};
        const cw::CdcParams cp = params();
        if ((rc = cdc_streams_args(cp, c->src[0].p, (size_t)total, sl, (uint64_t *)c->off.p, cap, w + W_NCHUNKS)) != CW_OK) return fail(CW_ERR_STATE, "cw_store_compose: the chunker refused the windows");
        if ((rc = dev_cdc_streams(cp, (const uint8_t *)c->src[0].p, (size_t)total, sl, (uint64_t *)c->off.p, cap, w + W_NCHUNKS, s)) != CW_OK) return rc;
        if ((rc = cw_dev_cdc_resync_windows((uint64_t *)c->off.p, w + W_NCHUNKS, cap - 1, (uint64_t *)c->first.p, (const cw_resync_window *)d_win, n,
                                            m + 1 + K, K + 1, (uint64_t *)c->rec_ref.p, s)) != CW_OK)
            return rc;
        HIP_TRY(hipMemcpyAsync(c->h_meta[0].p, c->rec_ref.p, 4 * n * 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync((uint64_t *)c->h_meta[0].p + 4 * n, c->first.p, (n + 1) * 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(c->h_status[0].p, c->status[0].p, (nranges + 1) * 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(h, w, W_WORDS * 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        if ((rc = check_filled()) != CW_OK) return rc;
        if (h[W_ENDS]) return fail(CW_ERR_STATE, "cw_store_compose: the windows' ends were refused");
        stats->rounds++;

        const uint64_t *res = (const uint64_t *)c->h_meta[0].p, *first = res + 4 * n;
        bool settled = true; // every window in front of this one is resolved
        for (size_t i = 0; i < wins.size();) {
            Window &v = wins[i++];
            if (v.discard) { v.discard = false; settled = false; continue; }
            if (!v.ran) { settled = settled && v.resolved; continue; }
            const uint64_t *r = res + 4 * v.slot;
            if (v.anchor < 0) { v.resolved = true; v.end = nb; v.t = first[v.slot + 1] - first[v.slot]; } // kept whole
            else if (r[0] == 0) {
                const Anchor &a = anchors[(size_t)v.anchor];
                if (r[2] < a.p || r[2] >= a.q) return fail(CW_ERR_STATE, "cw_store_compose: a landing at position %llu outside [%zu, %zu)", (unsigned long long)r[2], a.p, a.q);
                v.resolved = true; v.t = r[1]; v.s = (size_t)r[2]; v.end = r[3] - v.at + v.start;
            } else if (!v.exhausted) {
                v.look = v.look > UINT64_MAX / 2 ? UINT64_MAX : v.look * 2;
                settled = false;
            } else if (!settled) {
                settled = false; // its start is not known to be a true cut yet: it waits
            } else { // the anchor is dropped: the window merges into the next one
                stats->merged_windows++;
                const uint64_t start = v.start;
                if (i == wins.size()) wins.push_back(Window{start, -1, look0});
                Window &nxt = wins[i];
                nxt.start = start; nxt.resolved = false; nxt.discard = nxt.ran;
                wins.erase(wins.begin() + (long)(i - 1));
                i--;
            }
        }
        return CW_OK;
    }

    // the commit's hooks: the statuses and the stream index ride on the piece's one synchronise
    static int after_cdc(void *self, hipStream_t s)
    {
        Compose &t = *static_cast<Compose *>(self);
        const size_t n = t.spans.size();
        HIP_TRY(hipMemcpyAsync(t.c->h_status[0].p, t.c->status[0].p, (t.nranges + 1) * 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(t.c->h_meta[0].p, t.c->first.p, (n + 1) * 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync((uint64_t *)t.c->h_words.p + W_RESYNC, (uint64_t *)t.c->words.p + W_RESYNC, 4 * 8, hipMemcpyDeviceToHost, s));
        return CW_OK;
    }
    static int admit(void *self, size_t k, const uint64_t *hc)
    {
        Compose &t = *static_cast<Compose *>(self);
        int rc = t.check_filled();
        if (rc != CW_OK) return rc;
        const uint64_t *first = (const uint64_t *)t.c->h_meta[0].p;
        size_t e = 0;
        for (const Window &w : t.wins) {
            if (w.end <= w.start) continue;
            if (first[e + 1] - first[e] != w.t)
                return fail(CW_ERR_STATE, "cw_store_compose: the extent at %llu chunked into %llu chunks, its round found %llu", (unsigned long long)w.start,
                            (unsigned long long)(first[e + 1] - first[e]), (unsigned long long)w.t);
            e++;
        }
        if (k != t.stats->rebuilt_chunks) return fail(CW_ERR_STATE, "cw_store_compose: %zu rebuilt chunks, the rounds found %llu", k, (unsigned long long)t.stats->rebuilt_chunks);
        if (k + t.stats->kept_positions + 1 > t.max_out) return fail(CW_ERR_STATE, "cw_store_compose: %llu chunks do not fit max_out %zu", (unsigned long long)(k + t.stats->kept_positions), t.max_out);
        Admission adm{t.st, t.base};
        return admit_piece(&adm, k, hc);
    }

    int commit(uint64_t *out_refs, uint64_t *out_offsets, size_t *out_n)
    {
        spans.clear();
        stats->rebuilt_chunks = stats->rebuilt_bytes = stats->kept_positions = 0;
        for (const Window &w : wins) {
            if (w.end > w.start) { spans.push_back(Span{w.start, w.end}); stats->rebuilt_chunks += w.t; stats->rebuilt_bytes += w.end - w.start; }
            if (w.anchor >= 0) stats->kept_positions += anchors[(size_t)w.anchor].q - w.s;
        }
        const size_t n = spans.size();
        uint64_t *h = (uint64_t *)c->h_words.p;
        const uint64_t *h_ref = nullptr, *h_off = nullptr, *first = nullptr;
        if (n) {
            uint64_t *d_ends, *d_extra;
            std::vector<uint64_t> *l;
            int rc = materialise(0, &d_ends, &d_extra, &l);
            if (rc != CW_OK) return rc;
            slots_bytes = cw_chunk_slots_bytes(comp_alg, (size_t)total, cap - 1);
            if ((rc = c->dig.reserve(cap * 64)) != CW_OK || (rc = c->ref.reserve(cap * 8)) != CW_OK || (rc = c->new_idx.reserve(cap * 4)) != CW_OK ||
                (rc = c->sizes.reserve(cap * 4)) != CW_OK || (rc = c->slots.reserve(slots_bytes)) != CW_OK || (rc = c->h_meta[0].reserve((n + 1 + 2 * cap) * 8)) != CW_OK ||
                (rc = fill()) != CW_OK)
                return rc;
            uint64_t *w = (uint64_t *)c->words.p;
            bool inserted = false;
            PieceAdmit hook{st->d_used, w + W_VERDICT, w + W_COUNTS, h + W_COUNTS, admit, this, &inserted, after_cdc};
            const StreamList sl{d_ends, n, (uint64_t *)c->first.p, w + W_ENDS};
            size_t k = 0;
            rc = dev_cdc_dedupe_compress(x, p, comp_alg, c->src[0].p, (size_t)total, 1, base, (uint64_t *)c->off.p, cap, w + W_NCHUNKS, c->dig.p,
                                         (uint64_t *)c->ref.p, (uint32_t *)c->new_idx.p, w + W_NNEW, c->slots.p, slots_bytes, (uint32_t *)c->sizes.p, &k, s,
                                         &hook, &sl);
            if (rc == CW_ERR_NOMEM && inserted) return fail(CW_ERR_STATE, "cw_store_compose: device memory ran out behind the admitted extents");
            if (rc == CW_ERR_BAD_ARG && !unread) return fail(CW_ERR_STATE, "cw_store_compose: the extents' ends were refused");
            if (rc != CW_OK) return rc;
            rc = cw_dev_store_chunks(comp_alg, c->src[0].p, (size_t)total, (uint64_t *)c->off.p, w + W_NCHUNKS, cap - 1, (uint32_t *)c->new_idx.p, w + W_NNEW,
                                     c->slots.p, (uint32_t *)c->sizes.p, base, st->d_store, st->store_bytes, st->d_used, st->d_dir, st->dir_base,
                                     st->dir_entries, w + W_RESULT, s);
            if (rc != CW_OK) return rc == CW_ERR_NOMEM ? fail(CW_ERR_STATE, "cw_store_compose: no scratch behind the admitted extents") : rc;
            uint64_t *down = (uint64_t *)c->h_meta[0].p + n + 1;
            HIP_TRY(hipMemcpyAsync(h + W_NNEW, w + W_NNEW, 3 * sizeof(uint64_t), hipMemcpyDeviceToHost, s)); // (W_NNEW, W_RESULT[2])
            if (k) HIP_TRY(hipMemcpyAsync(down, c->ref.p, k * 8, hipMemcpyDeviceToHost, s));
            HIP_TRY(hipMemcpyAsync(down + cap, c->off.p, (k + 1) * 8, hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s));
            if (h[W_RESULT]) return fail(CW_ERR_STATE, "cw_store_compose: the admitted extents were not stored (verdict %llu)", (unsigned long long)h[W_RESULT]);
            stats->new_chunks = h[W_NNEW]; stats->stored_bytes = h[W_RESULT + 1];
            first = (const uint64_t *)c->h_meta[0].p; h_ref = down; h_off = down + cap;
        } else if (stats->kept_positions + 1 > max_out) {
            return fail(CW_ERR_STATE, "cw_store_compose: %llu chunks do not fit max_out %zu", (unsigned long long)stats->kept_positions, max_out);
        }
        // the splice, window by window: its extent's chunks, then the kept positions shifted into B
        size_t at = 0, e = 0;
        uint64_t lay = 0; // where the extent lies in src[0]
        out_offsets[0] = 0;
        for (const Window &w : wins) {
            if (out_offsets[at] != w.start) return fail(CW_ERR_STATE, "cw_store_compose: the recipe reaches %llu where a window starts at %llu", (unsigned long long)out_offsets[at], (unsigned long long)w.start);
            if (w.end > w.start) {
                for (uint64_t g = first[e]; g < first[e + 1]; g++, at++) { out_refs[at] = h_ref[g]; out_offsets[at + 1] = h_off[g + 1] - lay + w.start; }
                lay += w.end - w.start; e++;
            }
            if (w.anchor < 0) continue;
            const Anchor &a = anchors[(size_t)w.anchor];
            for (size_t i = w.s; i < a.q; i++, at++) { out_refs[at] = refs[i]; out_offsets[at + 1] = in_b(a, i + 1); }
        }
        if (out_offsets[at] != nb) return fail(CW_ERR_STATE, "cw_store_compose: the recipe ends at %llu of %llu bytes", (unsigned long long)out_offsets[at], (unsigned long long)nb);
        *out_n = at;
        return CW_OK;
    }
};

} // namespace

extern "C" {

int cw_dev_ingest_commit(const uint64_t *d_ref, const uint64_t *d_offsets, const uint64_t *d_nchunks, size_t max_chunks, const uint64_t *d_n_new,
                         const uint64_t *d_store_result, uint64_t stream_off, uint64_t *d_rec_ref, uint64_t *d_rec_off, uint64_t *d_rec_count,
                         size_t rec_cap, uint64_t *d_stats, uint64_t *d_verdict, void *stream)
{
    int rc = check_count("max_chunks", max_chunks);
    if (rc != CW_OK) return rc;
    if (!d_ref || !d_offsets || !d_nchunks || !d_n_new || !d_rec_ref || !d_rec_off || !d_rec_count || !d_verdict)
        return fail(CW_ERR_BAD_ARG, "NULL pointer");
    if (((uintptr_t)d_ref | (uintptr_t)d_offsets | (uintptr_t)d_nchunks | (uintptr_t)d_n_new | (uintptr_t)d_store_result | (uintptr_t)d_rec_ref |
         (uintptr_t)d_rec_off | (uintptr_t)d_rec_count | (uintptr_t)d_stats | (uintptr_t)d_verdict) & 7)
        return fail(CW_ERR_BAD_ARG, "a pointer is not 8-byte aligned");
    if ((rc = ensure_init()) != CW_OK) return rc;
    return launched(cw::ingest_commit_launch(d_ref, d_offsets, d_nchunks, max_chunks, d_n_new, d_store_result, stream_off, d_rec_ref, d_rec_off,
                                             d_rec_count, rec_cap, d_stats, d_verdict, (hipStream_t)stream),
                    "ingest commit launch");
}

int cw_store_ingest(cw_dedupe_t *x, const cw_cdc_params *p, int comp_alg, const cw_store *st, const void *src, size_t nbytes, uint64_t base,
                    uint64_t *refs, uint64_t *offsets, size_t max_offsets, size_t *nchunks, size_t *consumed, cw_ingest_stats *stats)
{
    if (nchunks) *nchunks = 0;
    if (consumed) *consumed = 0;
    if (stats) memset(stats, 0, sizeof *stats);
    cw::CdcParams cp;
    int rc = cdc_params(p, &cp);
    if (rc != CW_OK || (rc = check_codec(comp_alg)) != CW_OK) return rc;
    if (!x || !refs || !offsets || !nchunks || !consumed || (nbytes && !src)) return fail(CW_ERR_BAD_ARG, "NULL pointer");
    if (cp.max_size > CW_MAX_BLOCK_BYTES) return fail(CW_ERR_BAD_ARG, "max_size %u > %u: such a chunk cannot be stored", cp.max_size, CW_MAX_BLOCK_BYTES);
    if (max_offsets < nbytes / cp.min_size + 2)
        return fail(CW_ERR_BAD_ARG, "max_offsets %zu < nbytes / min_size + 2 = %zu", max_offsets, nbytes / cp.min_size + 2);
    if ((rc = check_store(st)) != CW_OK) return rc;
    if (base > UINT64_MAX - (nbytes / cp.min_size + 1)) return fail(CW_ERR_BAD_ARG, "base + nbytes / min_size + 1 wraps");
    const uint8_t *const span = (const uint8_t *)src;
    const uint64_t len = nbytes;
    Ingest g{"cw_store_ingest", x, p, comp_alg, st, &span, &len, 1, len, base, false};
    hipStream_t s_d2h;
    if ((rc = ctx_store(&g.c, &g.s, &g.s_h2d, &s_d2h)) != CW_OK) return rc;
    offsets[0] = 0;
    if (nbytes == 0) return CW_OK;

    size_t k = 0;
    bool refused = false;
    if ((rc = g.prepare(cp)) != CW_OK || (rc = g.run_and_collect(refs, offsets, max_offsets, stats, &k, &refused)) != CW_OK) return rc;
    *nchunks = k;
    *consumed = (size_t)offsets[k];
    if (refused) return CW_ERR_NOMEM; // (the message is the admission's)
    return *consumed == nbytes ? CW_OK : fail(CW_ERR_STATE, "cw_store_ingest: %zu of %zu bytes went in", *consumed, nbytes);
}

int cw_dev_ingest_commit_streams(const uint64_t *d_ref, const uint64_t *d_offsets, const uint64_t *d_nchunks, size_t max_chunks,
                                 const uint64_t *d_n_new, const uint64_t *d_store_result, uint64_t stream_off, uint64_t *d_rec_ref,
                                 uint64_t *d_rec_off, uint64_t *d_rec_count, size_t rec_cap, uint64_t *d_stats, uint64_t *d_verdict,
                                 const uint64_t *d_stream_first, size_t nstreams_piece, uint64_t first_stream, int skip_first,
                                 uint64_t *d_rec_first, size_t first_cap, void *stream)
{
    int rc = check_count("max_chunks", max_chunks);
    if (rc != CW_OK || (rc = check_count("nstreams_piece", nstreams_piece)) != CW_OK) return rc;
    if (!d_ref || !d_offsets || !d_nchunks || !d_n_new || !d_rec_ref || !d_rec_off || !d_rec_count || !d_verdict || !d_stream_first || !d_rec_first)
        return fail(CW_ERR_BAD_ARG, "NULL pointer");
    if (((uintptr_t)d_ref | (uintptr_t)d_offsets | (uintptr_t)d_nchunks | (uintptr_t)d_n_new | (uintptr_t)d_store_result | (uintptr_t)d_rec_ref |
         (uintptr_t)d_rec_off | (uintptr_t)d_rec_count | (uintptr_t)d_stats | (uintptr_t)d_verdict | (uintptr_t)d_stream_first | (uintptr_t)d_rec_first) & 7)
        return fail(CW_ERR_BAD_ARG, "a pointer is not 8-byte aligned");
    if (skip_first != 0 && skip_first != 1) return fail(CW_ERR_BAD_ARG, "skip_first is %d, not 0 or 1", skip_first);
    if ((rc = ensure_init()) != CW_OK) return rc;
    const cw::CommitStreams cs{d_stream_first, nstreams_piece, first_stream, (uint64_t)skip_first, d_rec_first, first_cap};
    return launched(cw::ingest_commit_streams_launch(d_ref, d_offsets, d_nchunks, max_chunks, d_n_new, d_store_result, stream_off, d_rec_ref, d_rec_off,
                                                     d_rec_count, rec_cap, d_stats, d_verdict, cs, (hipStream_t)stream),
                    "ingest commit streams launch");
}

int cw_store_ingest_streams(cw_dedupe_t *x, const cw_cdc_params *p, int comp_alg, const cw_store *st, const void *const *srcs, const uint64_t *lens,
                            size_t nstreams, uint64_t base, uint64_t *refs, uint64_t *offsets, size_t max_offsets, uint64_t *stream_first,
                            size_t *nchunks, uint64_t *consumed, size_t *streams_done, cw_ingest_stats *stats)
{
    if (nchunks) *nchunks = 0;
    if (consumed) *consumed = 0;
    if (streams_done) *streams_done = 0;
    if (stats) memset(stats, 0, sizeof *stats);
    cw::CdcParams cp;
    int rc = cdc_params(p, &cp);
    if (rc != CW_OK || (rc = check_codec(comp_alg)) != CW_OK) return rc;
    if (!x || !refs || !offsets || !stream_first || !nchunks || !consumed || !streams_done || (nstreams && (!srcs || !lens)))
        return fail(CW_ERR_BAD_ARG, "NULL pointer");
    if (cp.max_size > CW_MAX_BLOCK_BYTES) return fail(CW_ERR_BAD_ARG, "max_size %u > %u: such a chunk cannot be stored", cp.max_size, CW_MAX_BLOCK_BYTES);
    if ((rc = check_count("nstreams", nstreams)) != CW_OK) return rc;
    uint64_t total = 0;
    for (size_t f = 0; f < nstreams; f++) {
        if (lens[f] && !srcs[f]) return fail(CW_ERR_BAD_ARG, "span %zu is NULL and %llu bytes long", f, (unsigned long long)lens[f]);
        if (lens[f] > UINT64_MAX - total) return fail(CW_ERR_BAD_ARG, "the sum of lens wraps at span %zu", f);
        total += lens[f];
    }
    if (max_offsets < total / cp.min_size + nstreams + 1)
        return fail(CW_ERR_BAD_ARG, "max_offsets %zu < nbytes / min_size + nstreams + 1 = %llu", max_offsets,
                    (unsigned long long)(total / cp.min_size + nstreams + 1));
    if ((rc = check_store(st)) != CW_OK) return rc;
    if (base > UINT64_MAX - (total / cp.min_size + nstreams)) return fail(CW_ERR_BAD_ARG, "base + nbytes / min_size + nstreams wraps");
    Ingest g{"cw_store_ingest_streams", x, p, comp_alg, st, (const uint8_t *const *)srcs, lens, nstreams, total, base, true};
    hipStream_t s_d2h;
    if ((rc = ctx_store(&g.c, &g.s, &g.s_h2d, &s_d2h)) != CW_OK) return rc;
    offsets[0] = 0;
    for (size_t f = 0; f <= nstreams; f++) stream_first[f] = 0;
    *streams_done = nstreams;
    if (total == 0) return CW_OK; // (no stream, or empty ones only: no chunk, no piece)
    *streams_done = 0;

    size_t k = 0;
    bool refused = false;
    if ((rc = g.prepare(cp)) != CW_OK || (rc = g.run_and_collect(refs, offsets, max_offsets, stats, &k, &refused)) != CW_OK) return rc;
    // the stream index: the entries the pieces wrote, then the stream that was not begun (or the end) and the entry behind it
    const size_t written = g.taken + (g.open ? 1 : 0);
    if (written) HIP_TRY(hipMemcpy(stream_first, g.c->rec_first.p, written * 8, hipMemcpyDeviceToHost));
    for (size_t f = written; f <= nstreams && f <= g.taken + 1; f++) stream_first[f] = k;
    *nchunks = k;
    *consumed = offsets[k];
    *streams_done = g.taken;
    if (refused) return CW_ERR_NOMEM; // (the message is the admission's)
    return *consumed == total && g.taken == nstreams ? CW_OK
                                                     : fail(CW_ERR_STATE, "cw_store_ingest_streams: %llu of %llu bytes went in",
                                                            (unsigned long long)*consumed, (unsigned long long)total);
}

int cw_store_restore(int comp_alg, const cw_store *st, const uint64_t *refs, const uint64_t *offsets, size_t nchunks, void *dst, size_t dst_bytes,
                     uint32_t *status, size_t *n_bad)
{
    if (n_bad) *n_bad = 0;
    int rc = check_codec(comp_alg);
    if (rc != CW_OK || (rc = check_store(st)) != CW_OK) return rc;
    if (!offsets || !n_bad || (nchunks && !refs)) return fail(CW_ERR_BAD_ARG, "NULL pointer");
    // the windows: whole positions whose raw bytes fit a piece
    const size_t piece = piece_bytes(CW_MAX_BLOCK_BYTES);
    std::vector<size_t> first; // first position of every window, and the end
    size_t in_window = 0, most = 0, widest = 0;
    for (size_t j = 0; j < nchunks; j++) {
        if (offsets[j + 1] < offsets[j]) return fail(CW_ERR_BAD_ARG, "offsets decrease at position %zu", j);
        const uint64_t l = offsets[j + 1] - offsets[j];
        if (l > CW_MAX_BLOCK_BYTES) return fail(CW_ERR_BAD_ARG, "position %zu is %llu bytes long (> %u)", j, (unsigned long long)l, CW_MAX_BLOCK_BYTES);
        if (first.empty() || in_window + l > piece || j - first.back() == kWindowPositions) {
            first.push_back(j);
            in_window = 0;
        }
        in_window += (size_t)l;
        if (in_window > widest) widest = in_window;
        if (j + 1 - first.back() > most) most = j + 1 - first.back();
    }
    first.push_back(nchunks);
    const uint64_t total = nchunks ? offsets[nchunks] - offsets[0] : 0;
    if (dst_bytes < total) return fail(CW_ERR_BAD_ARG, "dst_bytes %zu < the stream's %llu bytes", dst_bytes, (unsigned long long)total);
    if (total && !dst) return fail(CW_ERR_BAD_ARG, "NULL dst");
    StoreCtx *cp;
    hipStream_t s, s_h2d, s_d2h;
    if ((rc = ctx_store(&cp, &s, &s_h2d, &s_d2h)) != CW_OK) return rc;
    if (nchunks == 0) return CW_OK;
    StoreCtx &c = *cp;
    const size_t windows = first.size() - 1, meta_bytes = 8 + most * 8 + (most + 1) * 8;
    const bool pinned = total == 0 || is_pinned(dst);
    for (size_t b = 0; b < (windows > 1 ? 2u : 1u); b++) {
        if ((rc = c.src[b].reserve(widest + 16)) != CW_OK || (rc = c.meta[b].reserve(meta_bytes)) != CW_OK || (rc = c.status[b].reserve(most * 4)) != CW_OK ||
            (rc = c.h_meta[b].reserve(meta_bytes)) != CW_OK || (rc = c.h_status[b].reserve(most * 4)) != CW_OK)
            return rc;
        if (!pinned && (rc = c.stage[b].reserve(widest)) != CW_OK) return rc;
    }
    size_t bad = 0;
    // window w has arrived: out of the staging, statuses to the caller
    auto finish = [&](size_t w) -> int {
        const int b = (int)(w & 1);
        const size_t j0 = first[w], n = first[w + 1] - j0, bytes = (size_t)(offsets[first[w + 1]] - offsets[j0]);
        HIP_TRY(hipEventSynchronize(c.ev_done[b]));
        if (!pinned && bytes) memcpy((uint8_t *)dst + (offsets[j0] - offsets[0]), c.stage[b].p, bytes);
        const uint32_t *got = (const uint32_t *)c.h_status[b].p;
        for (size_t j = 0; j < n; j++) bad += got[j] != 0;
        if (status) memcpy(status + j0, got, n * 4);
        return CW_OK;
    };
    auto run = [&]() -> int {
        for (size_t w = 0; w < windows; w++) {
            const int b = (int)(w & 1);
            int rc;
            if (w >= 2 && (rc = finish(w - 2)) != CW_OK) return rc;
            const size_t j0 = first[w], n = first[w + 1] - j0, bytes = (size_t)(offsets[first[w + 1]] - offsets[j0]);
            uint64_t *m = (uint64_t *)c.h_meta[b].p, *d_m = (uint64_t *)c.meta[b].p;
            m[0] = n;
            memcpy(m + 1, refs + j0, n * 8);
            for (size_t j = 0; j <= n; j++) m[1 + n + j] = offsets[j0 + j] - offsets[j0];
            HIP_TRY(hipMemcpyAsync(d_m, m, 8 + n * 8 + (n + 1) * 8, hipMemcpyHostToDevice, s_h2d));
            HIP_TRY(hipEventRecord(c.ev_up[b], s_h2d));
            HIP_TRY(hipStreamWaitEvent(s, c.ev_up[b], 0));
            rc = cw_dev_restore_chunks(comp_alg, st->d_store, st->store_bytes, st->d_dir, st->dir_base, st->dir_entries, d_m + 1, d_m + 1 + n, d_m, n,
                                       c.src[b].p, bytes, (uint32_t *)c.status[b].p, s);
            if (rc != CW_OK) return rc;
            HIP_TRY(hipEventRecord(c.ev_kernel[b], s));
            HIP_TRY(hipStreamWaitEvent(s_d2h, c.ev_kernel[b], 0));
            void *to = pinned ? (void *)((uint8_t *)dst + (offsets[j0] - offsets[0])) : c.stage[b].p;
            if (bytes) HIP_TRY(hipMemcpyAsync(to, c.src[b].p, bytes, hipMemcpyDeviceToHost, s_d2h));
            HIP_TRY(hipMemcpyAsync(c.h_status[b].p, c.status[b].p, n * 4, hipMemcpyDeviceToHost, s_d2h));
            HIP_TRY(hipEventRecord(c.ev_done[b], s_d2h));
        }
        for (size_t w = windows >= 2 ? windows - 2 : 0; w < windows; w++)
            if (int rc = finish(w)) return rc;
        return CW_OK;
    };
    rc = run();
    drain(s, s_h2d);
    (void)hipStreamSynchronize(s_d2h);
    if (rc == CW_OK) *n_bad = bad;
    return rc;
}

int cw_dev_cdc_resync(const uint64_t *d_new_offsets, uint64_t *d_new_count, size_t max_new, const uint64_t *d_old_offsets,
                      const uint64_t *d_old_count, size_t max_old, uint64_t new_from, uint64_t shift, int keep_all, uint64_t *d_result, void *stream)
{
    int rc = check_count("max_new", max_new);
    if (rc != CW_OK || (rc = check_count("max_old", max_old)) != CW_OK) return rc;
    if (!d_new_offsets) return fail(CW_ERR_BAD_ARG, "NULL d_new_offsets");
    if (!d_new_count) return fail(CW_ERR_BAD_ARG, "NULL d_new_count");
    if (!d_old_offsets) return fail(CW_ERR_BAD_ARG, "NULL d_old_offsets");
    if (!d_old_count) return fail(CW_ERR_BAD_ARG, "NULL d_old_count");
    if (!d_result) return fail(CW_ERR_BAD_ARG, "NULL d_result");
    if (((uintptr_t)d_new_offsets | (uintptr_t)d_new_count | (uintptr_t)d_old_offsets | (uintptr_t)d_old_count | (uintptr_t)d_result) & 7)
        return fail(CW_ERR_BAD_ARG, "a pointer is not 8-byte aligned");
    if (keep_all != 0 && keep_all != 1) return fail(CW_ERR_BAD_ARG, "keep_all is %d, not 0 or 1", keep_all);
    if ((rc = ensure_init()) != CW_OK) return rc;
    return launched_nomem(cw::cdc_resync_launch(d_new_offsets, d_new_count, max_new, d_old_offsets, d_old_count, max_old, new_from, shift, keep_all,
                                                d_result, (hipStream_t)stream),
                          "cdc resync launch");
}

int cw_store_patch(cw_dedupe_t *x, const cw_cdc_params *p, int comp_alg, const cw_store *st, const uint64_t *refs, const uint64_t *offsets,
                   size_t nchunks, uint64_t edit_off, uint64_t remove_bytes, const void *insert, size_t insert_bytes, uint64_t base, size_t lookahead,
                   uint64_t *out_refs, uint64_t *out_offsets, size_t max_out, size_t *out_nchunks, cw_patch_stats *stats)
{
    if (out_nchunks) *out_nchunks = 0;
    cw_patch_stats local;
    if (!stats) stats = &local;
    memset(stats, 0, sizeof *stats);
    cw::CdcParams cp;
    int rc = cdc_params(p, &cp);
    if (rc != CW_OK || (rc = check_codec(comp_alg)) != CW_OK) return rc;
    if (!x) return fail(CW_ERR_BAD_ARG, "NULL dedupe index");
    if (!offsets || (nchunks && !refs)) return fail(CW_ERR_BAD_ARG, "NULL recipe (refs / offsets)");
    if (!out_refs || !out_offsets || !out_nchunks) return fail(CW_ERR_BAD_ARG, "NULL out_refs / out_offsets / out_nchunks");
    if (insert_bytes && !insert) return fail(CW_ERR_BAD_ARG, "NULL insert with insert_bytes %zu", insert_bytes);
    if (cp.max_size > CW_MAX_BLOCK_BYTES) return fail(CW_ERR_BAD_ARG, "max_size %u > %u: such a chunk cannot be stored", cp.max_size, CW_MAX_BLOCK_BYTES);
    if (offsets[nchunks] < offsets[0]) return fail(CW_ERR_BAD_ARG, "offsets end below their start");
    const uint64_t n = offsets[nchunks] - offsets[0];
    if (edit_off > n || remove_bytes > n - edit_off)
        return fail(CW_ERR_BAD_ARG, "edit_off %llu + remove_bytes %llu leaves the stream's %llu bytes", (unsigned long long)edit_off,
                    (unsigned long long)remove_bytes, (unsigned long long)n);
    if (insert_bytes > UINT64_MAX - (n - remove_bytes)) return fail(CW_ERR_BAD_ARG, "insert_bytes %zu: the edited stream's length wraps", insert_bytes);
    const uint64_t edited = n - remove_bytes + insert_bytes;
    if (max_out < edited / cp.min_size + 2)
        return fail(CW_ERR_BAD_ARG, "max_out %zu < edited bytes / min_size + 2 = %llu", max_out, (unsigned long long)(edited / cp.min_size + 2));
    if ((rc = check_store(st)) != CW_OK) return rc;
    if (base > UINT64_MAX - (edited / cp.min_size + 1)) return fail(CW_ERR_BAD_ARG, "base + edited bytes / min_size + 1 wraps");
    Patch t{x, p, comp_alg, st, refs, offsets, nchunks, edit_off, remove_bytes, (const uint8_t *)insert, insert_bytes, base, max_out};
    uint64_t look = lookahead ? lookahead : (uint64_t)4 * cp.max_size;
    if (look < (uint64_t)2 * cp.max_size) look = (uint64_t)2 * cp.max_size;
    if ((rc = t.locate(look)) != CW_OK) return rc;
    hipStream_t s_h2d, s_d2h;
    if ((rc = ctx_store(&t.c, &t.s, &s_h2d, &s_d2h)) != CW_OK) return rc;

    for (;;) {
        stats->attempts++;
        if (t.wb == 0) { // the stream ends at c_j and nothing is put behind it: no window, no device
            t.k = 0; t.resume = t.K; t.retry = false;
            out_offsets[t.j] = t.cut(t.j);
        } else {
            rc = t.attempt(cp, out_refs, out_offsets, stats);
            if (rc != CW_OK) (void)hipStreamSynchronize(t.s); // nothing of the call is in flight when it returns
            if (rc != CW_OK) return rc;
        }
        if (!t.retry) break;
        look = look > UINT64_MAX / 2 ? UINT64_MAX : look * 2;
        if ((rc = t.locate(look)) != CW_OK) return rc;
    }
    const int64_t delta = (int64_t)(insert_bytes - remove_bytes);
    if (t.j) memcpy(out_refs, refs, t.j * 8);
    for (size_t i = 0; i < t.j; i++) out_offsets[i] = t.cut(i);
    const size_t at = t.j + t.k, rest = nchunks - t.resume;
    if (out_offsets[at] != (t.resume == nchunks ? edited : t.cut(t.resume) + (uint64_t)delta))
        return fail(CW_ERR_STATE, "cw_store_patch: the window ends at %llu, not where old position %zu begins", (unsigned long long)out_offsets[at], t.resume);
    if (rest) memcpy(out_refs + at, refs + t.resume, rest * 8);
    for (size_t i = 1; i <= rest; i++) out_offsets[at + i] = t.cut(t.resume + i) + (uint64_t)delta;
    *out_nchunks = at + rest;
    stats->first_position = t.j; stats->resume_position = t.resume; stats->reused_positions = t.j + rest;
    return CW_OK;
}

static_assert(sizeof(cw_resync_window) == 40 && sizeof(cw_compose_stats) == 64, "five and eight u64 words");

int cw_dev_cdc_resync_windows(const uint64_t *d_new_offsets, const uint64_t *d_new_count, size_t max_new, const uint64_t *d_stream_first,
                              const cw_resync_window *d_win, size_t nwin, const uint64_t *d_old_offsets, size_t max_old, uint64_t *d_result,
                              void *stream)
{
    int rc = check_count("max_new", max_new);
    if (rc != CW_OK || (rc = check_count("max_old", max_old)) != CW_OK || (rc = check_count("nwin", nwin)) != CW_OK) return rc;
    if (!d_new_offsets) return fail(CW_ERR_BAD_ARG, "NULL d_new_offsets");
    if (!d_new_count) return fail(CW_ERR_BAD_ARG, "NULL d_new_count");
    if (!d_stream_first) return fail(CW_ERR_BAD_ARG, "NULL d_stream_first");
    if (!d_win) return fail(CW_ERR_BAD_ARG, "NULL d_win");
    if (!d_old_offsets && max_old) return fail(CW_ERR_BAD_ARG, "NULL d_old_offsets");
    if (!d_result) return fail(CW_ERR_BAD_ARG, "NULL d_result");
    if (((uintptr_t)d_new_offsets | (uintptr_t)d_new_count | (uintptr_t)d_stream_first | (uintptr_t)d_win | (uintptr_t)d_old_offsets | (uintptr_t)d_result) & 7)
        return fail(CW_ERR_BAD_ARG, "a pointer is not 8-byte aligned");
    if ((rc = ensure_init()) != CW_OK) return rc;
    return launched_nomem(cw::cdc_resync_windows_launch(d_new_offsets, d_new_count, max_new, d_stream_first, d_win, nwin, d_old_offsets, max_old, d_result,
                                                        (hipStream_t)stream),
                          "cdc resync windows launch");
}

int cw_dev_scatter_extents(const void *d_src, size_t src_bytes, const uint64_t *d_ext, const uint64_t *d_n, size_t max_n, void *d_dst, size_t dst_bytes,
                           uint64_t *d_result, void *stream)
{
    int rc = check_count("max_n", max_n);
    if (rc != CW_OK) return rc;
    const char *null = !d_n ? "d_n" : !d_result ? "d_result" : max_n && !d_ext ? "d_ext" : src_bytes && !d_src ? "d_src" : dst_bytes && !d_dst ? "d_dst" : NULL;
    if (null) return fail(CW_ERR_BAD_ARG, "NULL pointer: %s", null);
    if (((uintptr_t)d_ext | (uintptr_t)d_n | (uintptr_t)d_result) & 7) return fail(CW_ERR_BAD_ARG, "d_ext, d_n or d_result is not 8-byte aligned");
    const uintptr_t a = (uintptr_t)d_src, b = (uintptr_t)d_dst;
    if (src_bytes && dst_bytes && a < b + dst_bytes && b < a + src_bytes) return fail(CW_ERR_BAD_ARG, "d_dst overlaps d_src");
    if ((rc = ensure_init()) != CW_OK) return rc;
    ProfScope prof(PROF_CODEC, (hipStream_t)stream);
    return launched(cw::scatter_extents_launch((const uint8_t *)d_src, src_bytes, d_ext, d_n, max_n, (uint8_t *)d_dst, dst_bytes, d_result,
                                               (hipStream_t)stream),
                    "scatter extents launch");
}

int cw_store_compose(cw_dedupe_t *x, const cw_cdc_params *p, int comp_alg, const cw_store *st, const uint64_t *refs, const uint64_t *offsets,
                     size_t nchunks, const uint64_t *stream_first, size_t nstreams, const cw_delta_op *ops, size_t nops, const void *payload,
                     size_t payload_bytes, uint64_t base, size_t lookahead, uint64_t *out_refs, uint64_t *out_offsets, size_t max_out,
                     size_t *out_nchunks, cw_compose_stats *stats)
{
    if (out_nchunks) *out_nchunks = 0;
    cw_compose_stats local;
    if (!stats) stats = &local;
    memset(stats, 0, sizeof *stats);
    cw::CdcParams cp;
    int rc = cdc_params(p, &cp);
    if (rc != CW_OK || (rc = check_codec(comp_alg)) != CW_OK) return rc;
    if (!x) return fail(CW_ERR_BAD_ARG, "NULL dedupe index");
    if (!offsets || (nchunks && !refs)) return fail(CW_ERR_BAD_ARG, "NULL recipe (refs / offsets)");
    if (nops && !ops) return fail(CW_ERR_BAD_ARG, "NULL ops with nops %zu", nops);
    if (!out_refs || !out_offsets || !out_nchunks) return fail(CW_ERR_BAD_ARG, "NULL out_refs / out_offsets / out_nchunks");
    if (payload_bytes && !payload) return fail(CW_ERR_BAD_ARG, "NULL payload with payload_bytes %zu", payload_bytes);
    if (cp.max_size > CW_MAX_BLOCK_BYTES) return fail(CW_ERR_BAD_ARG, "max_size %u > %u: such a chunk cannot be stored", cp.max_size, CW_MAX_BLOCK_BYTES);
    if (offsets[nchunks] < offsets[0]) return fail(CW_ERR_BAD_ARG, "offsets end below their start");
    const uint64_t na = offsets[nchunks] - offsets[0];
    if (stream_first) {
        if (stream_first[0] != 0) return fail(CW_ERR_BAD_ARG, "stream_first starts at %llu, not 0", (unsigned long long)stream_first[0]);
        for (size_t f = 0; f < nstreams; f++)
            if (stream_first[f + 1] < stream_first[f]) return fail(CW_ERR_BAD_ARG, "stream_first decreases at stream %zu", f);
        if (stream_first[nstreams] != nchunks)
            return fail(CW_ERR_BAD_ARG, "stream_first ends at %llu, not at nchunks %zu", (unsigned long long)stream_first[nstreams], nchunks);
    }
    // the op list, by cw_dev_apply_delta's rule over A's bytes and the payload
    uint64_t nb = 0;
    bool copies = false;
    for (size_t k = 0; k < nops; k++) {
        const cw_delta_op &o = ops[k];
        const bool copy = o.a_off != CW_DELTA_NONE, fresh = o.payload_off != CW_DELTA_NONE;
        const uint64_t room = copy ? na : (uint64_t)payload_bytes, from = copy ? o.a_off : o.payload_off;
        const char *why = o.b_off != nb ? "does not start where the one before ends" : o.len == 0 ? "has len 0" : o.b_off + o.len < o.b_off ? "wraps"
                        : copy == fresh ? "names both sources or neither" : o.len > room || from > room - o.len ? (copy ? "leaves the source's bytes" : "leaves the payload") : NULL;
        if (why) return fail(CW_ERR_BAD_ARG, "op %zu of %zu %s", k, nops, why);
        nb = o.b_off + o.len;
        copies = copies || copy;
    }
    if (max_out < nb / cp.min_size + 2)
        return fail(CW_ERR_BAD_ARG, "max_out %zu < composed bytes / min_size + 2 = %llu", max_out, (unsigned long long)(nb / cp.min_size + 2));
    if ((rc = check_store(st)) != CW_OK) return rc;
    if (base > UINT64_MAX - (nb / cp.min_size + 1)) return fail(CW_ERR_BAD_ARG, "base + composed bytes / min_size + 1 wraps");
    if (copies) // (the plan searches the whole list)
        for (size_t i = 0; i < nchunks; i++)
            if (offsets[i + 1] < offsets[i]) return fail(CW_ERR_BAD_ARG, "offsets decrease at position %zu", i);
    uint64_t look = lookahead ? lookahead : (uint64_t)4 * cp.max_size;
    if (look < (uint64_t)2 * cp.max_size) look = (uint64_t)2 * cp.max_size;
    Compose t{x, p, comp_alg, st, refs, nchunks, stream_first, stream_first ? nstreams : 1, ops, nops, (const uint8_t *)payload, payload_bytes, base, nb, look, max_out, stats};
    out_offsets[0] = 0;
    if (nops == 0) return CW_OK; // the empty stream: no device
    hipStream_t s_h2d, s_d2h;
    if ((rc = ctx_store(&t.c, &t.s, &s_h2d, &s_d2h)) != CW_OK) return rc;
    t.cuts.resize(nchunks + 1);
    for (size_t i = 0; i <= nchunks; i++) t.cuts[i] = offsets[i] - offsets[0];
    t.plan();
    auto run = [&]() -> int {
        for (;;) {
            bool open = false;
            for (const Compose::Window &w : t.wins) open = open || !w.resolved;
            if (!open) break;
            if (int rc = t.round()) return rc;
        }
        size_t k = 0;
        if (int rc = t.commit(out_refs, out_offsets, &k)) return rc;
        *out_nchunks = k;
        return CW_OK;
    };
    rc = run();
    if (rc != CW_OK) (void)hipStreamSynchronize(t.s); // nothing of the call is in flight when it returns
    return rc;
}

// The whole directory through cw_dev_store_verify, window by window: the work buffer is the context's first
// source buffer, cursor and totals are nine words of its first meta buffer, the statuses its first status buffer.  One synchronise per
// window brings the cursor back; nothing else crosses the bus until the end.
int cw_store_scrub(cw_dedupe_t *x, int comp_alg, const cw_store *st, const uint32_t *d_live, uint32_t *status, cw_scrub_stats *stats)
{
    int rc = check_codec(comp_alg);
    if (rc != CW_OK || (rc = check_store(st)) != CW_OK) return rc;
    if (!x) return fail(CW_ERR_BAD_ARG, "NULL dedupe index");
    if ((rc = check_count("dir_entries", st->dir_entries)) != CW_OK) return rc;
    const size_t piece = piece_bytes(CW_MAX_BLOCK_BYTES);
    StoreCtx *cp;
    hipStream_t s, s_h2d, s_d2h;
    if ((rc = ctx_store(&cp, &s, &s_h2d, &s_d2h)) != CW_OK) return rc;
    StoreCtx &c = *cp;
    const size_t n = st->dir_entries;
    if ((rc = c.src[0].reserve(piece)) != CW_OK || (rc = c.status[0].reserve(n * 4)) != CW_OK || (rc = c.meta[0].reserve(9 * 8)) != CW_OK) return rc;
    uint64_t *d_words = (uint64_t *)c.meta[0].p, h_words[9] = {0}; // the cursor, then the totals
    auto run = [&]() -> int {
        HIP_TRY(hipMemsetAsync(d_words, 0, sizeof h_words, s));
        for (uint64_t cursor = 0; cursor < n;) {
            const int rc = cw_dev_store_verify(x, comp_alg, st->d_store, st->store_bytes, st->d_dir, st->dir_base, n, d_live, d_words, c.src[0].p, piece,
                                               (uint32_t *)c.status[0].p, d_words + 1, s);
            if (rc != CW_OK) return rc;
            HIP_TRY(hipMemcpyAsync(h_words, d_words, sizeof(uint64_t), hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s));
            if (h_words[0] <= cursor) return fail(CW_ERR_STATE, "cw_store_scrub: the cursor stays at %llu", (unsigned long long)cursor);
            cursor = h_words[0];
        }
        HIP_TRY(hipMemcpyAsync(h_words, d_words, sizeof h_words, hipMemcpyDeviceToHost, s));
        if (status) HIP_TRY(hipMemcpyAsync(status, c.status[0].p, n * 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        return CW_OK;
    };
    rc = run();
    (void)hipStreamSynchronize(s);
    if (rc == CW_OK && stats) memcpy(stats, h_words + 1, sizeof *stats);
    return rc;
}

} // extern "C"
