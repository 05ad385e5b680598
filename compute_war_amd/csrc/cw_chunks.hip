// cw_chunks.hip -- host side of the device-resident calls over content-defined chunks: the cut (kernels: cdc_kernels.hip), the per-chunk
// hash, the chunk codecs and their pack (chunk_codec_kernels.hip, pack_kernels.hip), the chunk store (restore_kernels.hip), its ranged reads (read_kernels.hip),
// its mark and compact (store_gc_kernels.hip), its renumbering (renumber_kernels.hip), its accounting (account_kernels.hip), its chunk bundles (replicate_kernels.hip) and its recipe diff and delta (delta_kernels.hip).  Semantics: the public header.  Every refusal here comes before the device is touched.

#include "cw_host.h"

using namespace cw::host;

namespace {

uint64_t splitmix64_host(uint64_t x)
{
    uint64_t z = x + 0x9E3779B97F4A7C15ULL;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}

struct DefaultGear {
    uint64_t g[256];
    DefaultGear() { for (int v = 0; v < 256; v++) g[v] = splitmix64_host((uint64_t)v); }
};
const DefaultGear kDefaultGear;

// `bits`: the pointers of `names` or-ed together
int check_dir_aligned(uintptr_t bits, const char *names) { return bits & 15 ? fail(CW_ERR_BAD_ARG, "%s is not 16-byte aligned", names) : CW_OK; }
int check_word_aligned(uintptr_t bits, const char *names) { return bits & 7 ? fail(CW_ERR_BAD_ARG, "%s not 8-byte aligned", names) : CW_OK; }

// [a, a + an) and [b, b + bn) share a byte
bool ranges_overlap(const void *a, size_t an, const void *b, size_t bn)
{
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return an && bn && x < y + bn && y < x + an;
}

} // namespace

int cw::host::cdc_params(const cw_cdc_params *p, cw::CdcParams *out)
{
    if (!p) return fail(CW_ERR_BAD_ARG, "NULL cdc params");
    if (p->reserved != 0) return fail(CW_ERR_BAD_ARG, "cdc params: reserved must be 0");
    if (!(64 <= p->min_size && p->min_size <= p->normal_size && p->normal_size <= p->max_size && p->max_size <= (1u << 24)))
        return fail(CW_ERR_BAD_ARG, "cdc params: need 64 <= min %u <= normal %u <= max %u <= 2^24", p->min_size, p->normal_size, p->max_size);
    *out = cw::CdcParams{p->min_size, p->normal_size, p->max_size, p->mask_s, p->mask_l, p->gear ? p->gear : kDefaultGear.g};
    return CW_OK;
}

int cw::host::dev_cdc(const cw::CdcParams &p, const uint8_t *d_src, size_t nbytes, int final_, uint64_t *d_offsets, size_t max_offsets,
                      uint64_t *d_nchunks, hipStream_t s)
{
    const uint64_t seg = cw::cdc_segment_bytes(p.max_size, cw::knobs().cdc_segment);
    ProfScope prof(PROF_HASH, s);
    hipError_t e = cw::cdc_launch(p, d_src, nbytes, final_, d_offsets, max_offsets, d_nchunks, seg, s);
    if (e == hipErrorOutOfMemory) return fail(CW_ERR_NOMEM, "cdc workspace (%zu bytes): %s", cw::cdc_workspace_bytes(nbytes, p.min_size, seg),
                                              hipGetErrorString(e));
    return launched(e, "cdc launch");
}

int cw::host::cdc_streams_args(const cw::CdcParams &cp, const void *d_src, size_t nbytes, const StreamList &sl, const uint64_t *d_offsets,
                                size_t max_offsets, const uint64_t *d_nchunks)
{
    if (!d_offsets || !d_nchunks || !sl.d_first || !sl.d_result || (nbytes && !d_src) || (sl.nstreams && !sl.d_ends))
        return fail(CW_ERR_BAD_ARG, "NULL pointer");
    if (int rc = check_word_aligned((uintptr_t)sl.d_result, "d_result")) return rc;
    if (int rc = check_count("nstreams", sl.nstreams)) return rc;
    if (sl.nstreams == 0 && nbytes) return fail(CW_ERR_BAD_ARG, "nstreams is 0 and nbytes is %zu", nbytes);
    const size_t need = nbytes / cp.min_size + sl.nstreams + 1;
    if (max_offsets < need) return fail(CW_ERR_BAD_ARG, "max_offsets %zu < nbytes / min_size + nstreams + 1 = %zu", max_offsets, need);
    return CW_OK;
}

int cw::host::dev_cdc_streams(const cw::CdcParams &p, const uint8_t *d_src, size_t nbytes, const StreamList &sl, uint64_t *d_offsets,
                              size_t max_offsets, uint64_t *d_nchunks, hipStream_t s)
{
    const uint64_t seg = cw::cdc_segment_bytes(p.max_size, cw::knobs().cdc_segment);
    ProfScope prof(PROF_HASH, s);
    const cw::CdcStreams st{sl.d_ends, sl.nstreams, sl.d_first, sl.d_result, sl.final_};
    hipError_t e = cw::cdc_streams_launch(p, d_src, nbytes, st, d_offsets, max_offsets, d_nchunks, seg, s);
    if (e == hipErrorOutOfMemory)
        return fail(CW_ERR_NOMEM, "cdc workspace (%zu bytes): %s", cw::cdc_streams_workspace_bytes(nbytes, sl.nstreams, p.min_size, seg),
                    hipGetErrorString(e));
    return launched(e, "cdc streams launch");
}

int cw::host::dev_hash_chunks(int alg, const uint8_t *d_src, size_t src_bytes, const uint64_t *d_offsets, const uint64_t *d_nchunks,
                              size_t max_chunks, uint8_t *d_dig, hipStream_t s)
{
    if (alg == CW_HASH_NONE) return CW_OK;
    if (alg != CW_HASH_SKEIN512 && alg != CW_HASH_SKEIN256_128 && alg != CW_HASH_SHA256) return fail(CW_ERR_BAD_ARG, "unknown hash algorithm %d", alg);
    if (int rc = check_count("max_chunks", max_chunks)) return rc;
    if (max_chunks == 0) return CW_OK;
    ProfScope prof(PROF_HASH, s);
    struct Call { int alg; const uint8_t *src; size_t src_bytes; const uint64_t *off, *n; size_t max; uint8_t *dig; hipStream_t s; };
    Call call{alg, d_src, src_bytes, d_offsets, d_nchunks, max_chunks, d_dig, s};
    const cw::ChunkHash hash{[](void *ctx, const uint32_t *perm) {
                                 const Call &k = *static_cast<const Call *>(ctx);
                                 if (k.alg == CW_HASH_SHA256) return cw::sha256_chunks_launch(k.src, k.src_bytes, k.off, perm, k.n, k.max, k.dig, k.s);
                                 const int nw = k.alg == CW_HASH_SKEIN512 ? 8 : 4;
                                 return cw::skein_chunks_launch(nw, k.src, k.src_bytes, k.off, perm, k.n, k.max, skein_iv(nw), k.dig, nw == 8 ? 64 : 16, k.s);
                             },
                             &call};
    // the step counts the sort orders by: 64-byte steps (Skein-512, SHA-256) or 32-byte steps (Skein-256)
    return launched_nomem(cw::chunk_hash_launch(d_offsets, d_nchunks, max_chunks, src_bytes, alg == CW_HASH_SKEIN256_128 ? 5 : 6, hash, s),
                          "hash chunks launch");
}

int cw::host::compress_chunks_args(int comp_alg, const void *d_src, size_t src_bytes, const uint64_t *d_offsets, const uint64_t *d_nchunks,
                                   size_t max_chunks, const uint32_t *d_sel, const uint64_t *d_nsel, const void *d_dst, size_t dst_bytes,
                                   const uint32_t *d_sizes)
{
    int rc;
    if ((rc = check_codec(comp_alg)) != CW_OK || (rc = check_count("max_chunks", max_chunks)) != CW_OK) return rc;
    if (src_bytes > ((size_t)1 << 62)) return fail(CW_ERR_BAD_ARG, "src_bytes %zu not usable", src_bytes);
    if (!d_offsets || !d_nchunks || !d_dst || !d_sizes || (src_bytes && !d_src) || (d_sel && !d_nsel)) return fail(CW_ERR_BAD_ARG, "NULL pointer");
    const size_t need = (size_t)cw::chunk_slot_offset(comp_alg == CW_COMP_LZ4, src_bytes, max_chunks) + 16;
    if (dst_bytes < need) return fail(CW_ERR_BAD_ARG, "dst_bytes %zu < cw_chunk_slots_bytes = %zu", dst_bytes, need);
    return CW_OK;
}

int cw::host::dev_compress_chunks(int comp_alg, const uint8_t *d_src, size_t src_bytes, const uint64_t *d_offsets, const uint64_t *d_nchunks,
                                  size_t max_chunks, const uint32_t *d_sel, const uint64_t *d_nsel, uint8_t *d_dst, uint32_t *d_sizes, hipStream_t s)
{
    ProfScope prof(PROF_CODEC, s);
    const hipError_t e = cw::chunk_compress_launch(comp_alg == CW_COMP_LZF, d_src, src_bytes, d_offsets, d_nchunks, max_chunks, d_sel, d_nsel,
                                                   d_dst, d_sizes, s);
    if (e == hipErrorOutOfMemory)
        return fail(CW_ERR_NOMEM, "chunk parser workspace (order %zu bytes, lane tables of %zu bytes each): %s", (2048 + max_chunks) * 4,
                    cw::chunk_lane_table_bytes(comp_alg == CW_COMP_LZF), hipGetErrorString(e));
    return launched(e, "compress chunks launch");
}

extern "C" {

void cw_cdc_default_params(cw_cdc_params *p, uint32_t normal_size)
{
    if (!p) return;
    // normal_size is clamped to [256, 2^21] and rounded down to a power of two, so every field is defined and valid
    unsigned lg = 8;
    while (lg < 21 && (1u << (lg + 1)) <= normal_size) lg++;
    const uint32_t normal = 1u << lg;
    p->min_size = normal / 4;
    p->normal_size = normal;
    p->max_size = normal * 8;
    p->reserved = 0;
    p->mask_s = ~0ull << (64 - (lg + 2));
    p->mask_l = ~0ull << (64 - (lg - 2));
    p->gear = NULL;
}

int cw_dev_cdc(const cw_cdc_params *p, const void *d_src, size_t nbytes, int final, uint64_t *d_offsets, size_t max_offsets,
               uint64_t *d_nchunks, void *stream)
{
    cw::CdcParams cp;
    int rc = cdc_params(p, &cp);
    if (rc != CW_OK) return rc;
    if (!d_offsets || !d_nchunks || (nbytes && !d_src)) return fail(CW_ERR_BAD_ARG, "NULL pointer");
    if (max_offsets < nbytes / cp.min_size + 2)
        return fail(CW_ERR_BAD_ARG, "max_offsets %zu < nbytes / min_size + 2 = %zu", max_offsets, nbytes / cp.min_size + 2);
    if ((rc = ensure_init()) != CW_OK) return rc;
    return dev_cdc(cp, (const uint8_t *)d_src, nbytes, final ? 1 : 0, d_offsets, max_offsets, d_nchunks, (hipStream_t)stream);
}

int cw_dev_cdc_streams(const cw_cdc_params *p, const void *d_src, size_t nbytes, const uint64_t *d_ends, size_t nstreams, uint64_t *d_offsets,
                       size_t max_offsets, uint64_t *d_nchunks, uint64_t *d_stream_first, uint64_t *d_result, void *stream)
{
    return cw_dev_cdc_streams_part(p, d_src, nbytes, d_ends, nstreams, 1, d_offsets, max_offsets, d_nchunks, d_stream_first, d_result, stream);
}

int cw_dev_cdc_streams_part(const cw_cdc_params *p, const void *d_src, size_t nbytes, const uint64_t *d_ends, size_t nstreams, int final,
                            uint64_t *d_offsets, size_t max_offsets, uint64_t *d_nchunks, uint64_t *d_stream_first, uint64_t *d_result, void *stream)
{
    cw::CdcParams cp;
    int rc = cdc_params(p, &cp);
    if (rc != CW_OK) return rc;
    const StreamList sl{d_ends, nstreams, d_stream_first, d_result, final ? 1 : 0};
    if ((rc = cdc_streams_args(cp, d_src, nbytes, sl, d_offsets, max_offsets, d_nchunks)) != CW_OK) return rc;
    if ((rc = ensure_init()) != CW_OK) return rc;
    return dev_cdc_streams(cp, (const uint8_t *)d_src, nbytes, sl, d_offsets, max_offsets, d_nchunks, (hipStream_t)stream);
}

int cw_dev_hash_chunks(int hash_alg, const void *d_src, size_t src_bytes, const uint64_t *d_offsets, const uint64_t *d_nchunks,
                       size_t max_chunks, void *d_digests, void *stream)
{
    if (hash_alg < 0 || hash_alg > CW_HASH_NONE) return fail(CW_ERR_BAD_ARG, "unknown hash algorithm %d", hash_alg);
    if (hash_alg != CW_HASH_NONE && max_chunks && (!d_offsets || !d_nchunks || !d_digests || (src_bytes && !d_src)))
        return fail(CW_ERR_BAD_ARG, "NULL pointer");
    int rc = ensure_init();
    if (rc != CW_OK) return rc;
    return dev_hash_chunks(hash_alg, (const uint8_t *)d_src, src_bytes, d_offsets, d_nchunks, max_chunks, (uint8_t *)d_digests,
                           (hipStream_t)stream);
}

uint64_t cw_chunk_slot_offset(int comp_alg, uint64_t o, uint64_t i) { return cw::chunk_slot_offset(comp_alg != CW_COMP_LZF, o, i); }
size_t cw_chunk_slots_bytes(int comp_alg, size_t src_bytes, size_t max_chunks)
{
    return (size_t)cw_chunk_slot_offset(comp_alg, src_bytes, max_chunks) + 16;
}

int cw_dev_compress_chunks(int comp_alg, const void *d_src, size_t src_bytes, const uint64_t *d_offsets, const uint64_t *d_nchunks,
                           size_t max_chunks, const uint32_t *d_sel, const uint64_t *d_nsel, void *d_dst, size_t dst_bytes,
                           uint32_t *d_sizes, void *stream)
{
    int rc = compress_chunks_args(comp_alg, d_src, src_bytes, d_offsets, d_nchunks, max_chunks, d_sel, d_nsel, d_dst, dst_bytes, d_sizes);
    if (rc != CW_OK) return rc;
    if ((rc = ensure_init()) != CW_OK) return rc;
    return dev_compress_chunks(comp_alg, (const uint8_t *)d_src, src_bytes, d_offsets, d_nchunks, max_chunks, d_sel, d_nsel, (uint8_t *)d_dst,
                               d_sizes, (hipStream_t)stream);
}

int cw_dev_pack_chunks(int comp_alg, const void *d_slots, const uint64_t *d_offsets, const uint32_t *d_sel, const uint64_t *d_count,
                       size_t max_count, const uint32_t *d_sizes, void *d_packed, uint64_t *d_packed_offsets, void *stream)
{
    int rc;
    if ((rc = check_codec(comp_alg)) != CW_OK || (rc = check_count("max_count", max_count)) != CW_OK) return rc;
    if (!d_packed_offsets || (max_count && (!d_count || !d_sizes || (d_packed && (!d_slots || !d_offsets)))))
        return fail(CW_ERR_BAD_ARG, "NULL pointer");
    if ((rc = ensure_init()) != CW_OK) return rc;
    return launched_nomem(cw::chunk_pack_launch(comp_alg == CW_COMP_LZF, (const uint8_t *)d_slots, d_offsets, d_sel, d_count, max_count, d_sizes,
                                                (uint8_t *)d_packed, d_packed_offsets, (hipStream_t)stream),
                          "pack chunks launch");
}

int cw_dev_decompress_chunks(int comp_alg, const void *d_comp, const uint64_t *d_comp_offsets, const uint64_t *d_raw_offsets,
                             const uint64_t *d_count, size_t max_count, void *d_dst, size_t dst_bytes, uint32_t *d_status, void *stream)
{
    int rc;
    if ((rc = check_codec(comp_alg)) != CW_OK || (rc = check_count("max_count", max_count)) != CW_OK) return rc;
    if (max_count && (!d_comp || !d_comp_offsets || !d_raw_offsets || !d_count || !d_status || (dst_bytes && !d_dst)))
        return fail(CW_ERR_BAD_ARG, "NULL pointer");
    if ((rc = ensure_init()) != CW_OK) return rc;
    ProfScope prof(PROF_CODEC, (hipStream_t)stream);
    return launched(cw::chunk_decompress_launch(comp_alg == CW_COMP_LZF, (const uint8_t *)d_comp, d_comp_offsets, d_raw_offsets, d_count, max_count,
                                                (uint8_t *)d_dst, dst_bytes, d_status, (hipStream_t)stream),
                    "decompress chunks launch");
}

// ---- the chunk store (kernels: restore_kernels.hip) -------------------------------------------------------------------------
static_assert(sizeof(cw_chunk_loc) == 16, "cw_chunk_loc is one 16-byte store");

int cw_dev_store_chunks(int comp_alg, const void *d_src, size_t src_bytes, const uint64_t *d_offsets, const uint64_t *d_nchunks,
                        size_t max_chunks, const uint32_t *d_sel, const uint64_t *d_nsel, const void *d_slots, const uint32_t *d_sizes,
                        uint64_t base, void *d_store, size_t store_bytes, uint64_t *d_used, cw_chunk_loc *d_dir, uint64_t dir_base,
                        size_t dir_entries, uint64_t *d_result, void *stream)
{
    int rc;
    if ((rc = check_codec(comp_alg)) != CW_OK || (rc = check_count("max_chunks", max_chunks)) != CW_OK) return rc;
    if (!d_offsets || !d_nchunks || !d_slots || !d_sizes || !d_used || !d_dir || !d_result || (src_bytes && !d_src) || (store_bytes && !d_store) ||
        !d_sel != !d_nsel)
        return fail(CW_ERR_BAD_ARG, "NULL pointer");
    if (dir_entries == 0) return fail(CW_ERR_BAD_ARG, "dir_entries is 0");
    if ((rc = check_dir_aligned((uintptr_t)d_dir, "d_dir")) != CW_OK) return rc;
    if ((rc = check_word_aligned((uintptr_t)d_used | (uintptr_t)d_result, "d_used / d_result")) != CW_OK) return rc;
    if ((rc = ensure_init()) != CW_OK) return rc;
    return launched_nomem(cw::chunk_store_launch(comp_alg == CW_COMP_LZF, (const uint8_t *)d_src, src_bytes, d_offsets, d_nchunks, max_chunks, d_sel,
                                                 d_nsel, (const uint8_t *)d_slots, d_sizes, base, (uint8_t *)d_store, store_bytes, d_used, d_dir,
                                                 dir_base, dir_entries, d_result, (hipStream_t)stream),
                          "store chunks launch");
}

int cw_dev_restore_chunks(int comp_alg, const void *d_store, size_t store_bytes, const cw_chunk_loc *d_dir, uint64_t dir_base,
                          size_t dir_entries, const uint64_t *d_ref, const uint64_t *d_raw_offsets, const uint64_t *d_count, size_t max_count,
                          void *d_dst, size_t dst_bytes, uint32_t *d_status, void *stream)
{
    int rc;
    if ((rc = check_codec(comp_alg)) != CW_OK || (rc = check_count("max_count", max_count)) != CW_OK) return rc;
    if (!d_dir || !d_ref || !d_raw_offsets || !d_count || !d_status || (store_bytes && !d_store) || (dst_bytes && !d_dst))
        return fail(CW_ERR_BAD_ARG, "NULL pointer");
    if (dir_entries == 0) return fail(CW_ERR_BAD_ARG, "dir_entries is 0");
    if ((rc = check_dir_aligned((uintptr_t)d_dir, "d_dir")) != CW_OK) return rc;
    if ((rc = ensure_init()) != CW_OK) return rc;
    ProfScope prof(PROF_CODEC, (hipStream_t)stream);
    return launched(cw::chunk_restore_launch(comp_alg == CW_COMP_LZF, (const uint8_t *)d_store, store_bytes, d_dir, dir_base, dir_entries, d_ref,
                                             d_raw_offsets, d_count, max_count, (uint8_t *)d_dst, dst_bytes, d_status, (hipStream_t)stream),
                    "restore chunks launch");
}

int cw_dev_read_ranges(int comp_alg, const void *d_store, size_t store_bytes, const cw_chunk_loc *d_dir, uint64_t dir_base, size_t dir_entries,
                       const uint64_t *d_ref, const uint64_t *d_raw_offsets, const uint64_t *d_count, size_t max_count,
                       const uint64_t *d_range_off, const uint64_t *d_range_len, const uint64_t *d_range_dst, const uint64_t *d_nranges,
                       size_t max_ranges, void *d_dst, size_t dst_bytes, uint32_t *d_status, void *stream)
{
    int rc;
    if ((rc = check_codec(comp_alg)) != CW_OK || (rc = check_count("max_count", max_count)) != CW_OK ||
        (rc = check_count("max_ranges", max_ranges)) != CW_OK)
        return rc;
    if (!d_dir || !d_ref || !d_raw_offsets || !d_count || !d_range_off || !d_range_len || !d_range_dst || !d_nranges || !d_status ||
        (store_bytes && !d_store) || (dst_bytes && !d_dst))
        return fail(CW_ERR_BAD_ARG, "NULL pointer");
    if (dir_entries == 0) return fail(CW_ERR_BAD_ARG, "dir_entries is 0");
    if ((rc = check_dir_aligned((uintptr_t)d_dir, "d_dir")) != CW_OK) return rc;
    if ((rc = ensure_init()) != CW_OK) return rc;
    ProfScope prof(PROF_CODEC, (hipStream_t)stream);
    const hipError_t e = cw::read_ranges_launch(comp_alg == CW_COMP_LZF, (const uint8_t *)d_store, store_bytes, d_dir, dir_base, dir_entries, d_ref,
                                                d_raw_offsets, d_count, max_count, d_range_off, d_range_len, d_range_dst, d_nranges, max_ranges,
                                                (uint8_t *)d_dst, dst_bytes, d_status, (hipStream_t)stream);
    if (e == hipErrorOutOfMemory)
        return fail(CW_ERR_NOMEM, "read ranges scratch (up to %zu bytes): %s", cw::read_ranges_scratch_bytes(max_ranges), hipGetErrorString(e));
    return launched(e, "read ranges launch");
}

// ---- the chunk store forgets: mark and compact (kernels: store_gc_kernels.hip) -------------------------------------------------
int cw_dev_store_mark(const uint64_t *d_ref, const uint64_t *d_count, size_t max_count, uint64_t dir_base, size_t dir_entries, uint32_t *d_live,
                      uint64_t *d_n_outside, void *stream)
{
    int rc = check_count("max_count", max_count);
    if (rc != CW_OK) return rc;
    if (!d_ref || !d_count || !d_live || !d_n_outside) return fail(CW_ERR_BAD_ARG, "NULL pointer");
    if (dir_entries == 0) return fail(CW_ERR_BAD_ARG, "dir_entries is 0");
    if ((rc = check_word_aligned((uintptr_t)d_n_outside, "d_n_outside")) != CW_OK) return rc;
    if ((rc = ensure_init()) != CW_OK) return rc;
    return launched(cw::store_mark_launch(d_ref, d_count, max_count, dir_base, dir_entries, d_live, d_n_outside, (hipStream_t)stream),
                    "store mark launch");
}

int cw_dev_store_compact(const void *d_store, size_t store_bytes, const cw_chunk_loc *d_dir, size_t dir_entries, const uint32_t *d_live,
                         void *d_new_store, size_t new_store_bytes, uint64_t *d_new_used, cw_chunk_loc *d_new_dir, uint64_t *d_result,
                         void *stream)
{
    int rc;
    if (!d_dir || !d_live || !d_new_used || !d_new_dir || !d_result || (store_bytes && !d_store) || (new_store_bytes && !d_new_store))
        return fail(CW_ERR_BAD_ARG, "NULL pointer");
    if (dir_entries == 0) return fail(CW_ERR_BAD_ARG, "dir_entries is 0");
    if ((rc = check_dir_aligned((uintptr_t)d_dir | (uintptr_t)d_new_dir, "d_dir / d_new_dir")) != CW_OK) return rc;
    if ((rc = check_word_aligned((uintptr_t)d_new_used | (uintptr_t)d_result, "d_new_used / d_result")) != CW_OK) return rc;
    if (ranges_overlap(d_store, store_bytes, d_new_store, new_store_bytes)) return fail(CW_ERR_BAD_ARG, "d_new_store overlaps d_store");
    if (d_new_dir != d_dir && ranges_overlap(d_dir, dir_entries * sizeof(cw_chunk_loc), d_new_dir, dir_entries * sizeof(cw_chunk_loc)))
        return fail(CW_ERR_BAD_ARG, "d_new_dir overlaps d_dir without being d_dir");
    if ((rc = ensure_init()) != CW_OK) return rc;
    return launched_nomem(cw::store_compact_launch((const uint8_t *)d_store, store_bytes, d_dir, dir_entries, d_live, (uint8_t *)d_new_store,
                                                   new_store_bytes, d_new_used, d_new_dir, d_result, (hipStream_t)stream),
                          "store compact launch");
}

// ---- the directory gives slots back: renumber (kernels: renumber_kernels.hip) --------------------------------------------------
int cw_dev_store_renumber(const cw_chunk_loc *d_dir, uint64_t dir_base, size_t dir_entries, const uint32_t *d_live, uint64_t new_base,
                          cw_chunk_loc *d_new_dir, uint64_t new_dir_base, size_t new_dir_entries, uint64_t *d_from, uint64_t *d_to, size_t max_pairs,
                          uint64_t *d_result, void *stream)
{
    int rc;
    if (!d_dir || !d_result || (new_dir_entries && !d_new_dir) || (max_pairs && (!d_from || !d_to))) return fail(CW_ERR_BAD_ARG, "NULL pointer");
    if (dir_entries == 0) return fail(CW_ERR_BAD_ARG, "dir_entries is 0");
    if ((rc = check_count("dir_entries", dir_entries)) != CW_OK || (rc = check_count("new_dir_entries", new_dir_entries)) != CW_OK ||
        (rc = check_count("max_pairs", max_pairs)) != CW_OK)
        return rc;
    if ((rc = check_dir_aligned((uintptr_t)d_dir | (uintptr_t)d_new_dir, "d_dir / d_new_dir")) != CW_OK) return rc;
    if ((rc = check_word_aligned((uintptr_t)d_from | (uintptr_t)d_to | (uintptr_t)d_result, "d_from / d_to / d_result")) != CW_OK) return rc;
    if (ranges_overlap(d_dir, dir_entries * sizeof(cw_chunk_loc), d_new_dir, new_dir_entries * sizeof(cw_chunk_loc)))
        return fail(CW_ERR_BAD_ARG, "d_new_dir overlaps d_dir");
    if (new_dir_base > UINT64_MAX - new_dir_entries) return fail(CW_ERR_BAD_ARG, "new_dir_base + new_dir_entries wraps");
    if ((rc = ensure_init()) != CW_OK) return rc;
    return launched_nomem(cw::store_renumber_launch(d_dir, dir_base, dir_entries, d_live, new_base, d_new_dir, new_dir_base, new_dir_entries, d_from,
                                                    d_to, max_pairs, d_result, (hipStream_t)stream),
                          "store renumber launch");
}

// ---- per-stream accounting and reverse references: account (kernels: account_kernels.hip) --------------------------------------
int cw_dev_store_account(const uint64_t *d_ref, const uint64_t *d_first, size_t nstreams, size_t max_positions, const cw_chunk_loc *d_dir,
                         uint64_t dir_base, size_t dir_entries, const uint32_t *d_flag, cw_stream_account *d_acct, uint32_t *d_refcount,
                         uint32_t *d_owner, uint64_t *d_totals, void *stream)
{
    int rc;
    const char *null = !d_first ? "d_first" : !d_dir ? "d_dir" : !d_acct ? "d_acct" : !d_totals ? "d_totals" : max_positions && !d_ref ? "d_ref" : NULL;
    if (null) return fail(CW_ERR_BAD_ARG, "NULL pointer: %s", null);
    if (nstreams == 0) return fail(CW_ERR_BAD_ARG, "nstreams is 0");
    if (nstreams > ((size_t)1 << 32) - 258) return fail(CW_ERR_BAD_ARG, "nstreams %zu > 2^32 - 258", nstreams); // (CW_OWNER_SHARED, CW_OWNER_NONE)
    if (dir_entries == 0) return fail(CW_ERR_BAD_ARG, "dir_entries is 0");
    if ((rc = check_count("max_positions", max_positions)) != CW_OK || (rc = check_count("dir_entries", dir_entries)) != CW_OK) return rc;
    if ((rc = check_dir_aligned((uintptr_t)d_dir, "d_dir")) != CW_OK) return rc;
    if ((rc = check_word_aligned((uintptr_t)d_ref | (uintptr_t)d_first | (uintptr_t)d_acct | (uintptr_t)d_totals,
                                 "d_ref / d_first / d_acct / d_totals")) != CW_OK)
        return rc;
    if ((rc = ensure_init()) != CW_OK) return rc;
    return launched_nomem(cw::store_account_launch(d_ref, d_first, nstreams, max_positions, d_dir, dir_base, dir_entries, d_flag, d_acct, d_refcount,
                                                   d_owner, d_totals, (hipStream_t)stream),
                          "store account launch");
}

// ---- what changed between two recipes, and a version as a delta (kernels: delta_kernels.hip) -------------------------------------
static_assert(sizeof(cw_delta_op) == 32, "cw_delta_op is four u64 words");

int cw_dev_recipe_diff(const uint64_t *d_ref_a, const uint64_t *d_off_a, const uint64_t *d_na, size_t max_a, const uint64_t *d_ref_b,
                       const uint64_t *d_off_b, const uint64_t *d_nb, size_t max_b, uint64_t dir_base, size_t dir_entries, cw_delta_op *d_ops,
                       size_t max_ops, uint64_t *d_nops, uint64_t *d_src, uint64_t *d_new_off, uint64_t *d_new_len, uint64_t *d_new_dst,
                       uint64_t *d_nnew, uint64_t *d_totals, void *stream)
{
    int rc;
    const char *null = !d_ref_a ? "d_ref_a" : !d_off_a ? "d_off_a" : !d_na ? "d_na" : !d_ref_b ? "d_ref_b" : !d_off_b ? "d_off_b" : !d_nb ? "d_nb"
                     : !d_nops ? "d_nops" : !d_totals ? "d_totals" : max_ops && !d_ops ? "d_ops" : NULL;
    if (null) return fail(CW_ERR_BAD_ARG, "NULL pointer: %s", null);
    const int ranges = !!d_new_off + !!d_new_len + !!d_new_dst + !!d_nnew;
    if (ranges != 0 && ranges != 4) return fail(CW_ERR_BAD_ARG, "NULL pointer: d_new_off, d_new_len, d_new_dst and d_nnew go together");
    if (dir_entries == 0) return fail(CW_ERR_BAD_ARG, "dir_entries is 0");
    if ((rc = check_count("max_a", max_a)) != CW_OK || (rc = check_count("max_b", max_b)) != CW_OK ||
        (rc = check_count("dir_entries", dir_entries)) != CW_OK)
        return rc;
    const struct { const void *p; const char *name; } words[] = {
        {d_ref_a, "d_ref_a"}, {d_off_a, "d_off_a"}, {d_na, "d_na"}, {d_ref_b, "d_ref_b"}, {d_off_b, "d_off_b"}, {d_nb, "d_nb"}, {d_ops, "d_ops"},
        {d_nops, "d_nops"}, {d_src, "d_src"}, {d_new_off, "d_new_off"}, {d_new_len, "d_new_len"}, {d_new_dst, "d_new_dst"}, {d_nnew, "d_nnew"},
        {d_totals, "d_totals"}};
    for (const auto &w : words)
        if ((rc = check_word_aligned((uintptr_t)w.p, w.name)) != CW_OK) return rc;
    if ((rc = ensure_init()) != CW_OK) return rc;
    const hipError_t e = cw::recipe_diff_launch(d_ref_a, d_off_a, d_na, max_a, d_ref_b, d_off_b, d_nb, max_b, dir_base, dir_entries, d_ops, max_ops,
                                                d_nops, d_src, d_new_off, d_new_len, d_new_dst, d_nnew, d_totals, (hipStream_t)stream);
    if (e == hipErrorOutOfMemory)
        return fail(CW_ERR_NOMEM, "recipe diff scratch (%zu bytes): %s", cw::recipe_diff_scratch_bytes(max_b, dir_entries), hipGetErrorString(e));
    return launched(e, "recipe diff launch");
}

int cw_dev_apply_delta(const void *d_old, size_t old_bytes, const void *d_payload, size_t payload_bytes, const cw_delta_op *d_ops,
                       const uint64_t *d_nops, size_t max_ops, void *d_dst, size_t dst_bytes, uint64_t *d_result, void *stream)
{
    int rc;
    const char *null = !d_nops ? "d_nops" : !d_result ? "d_result" : max_ops && !d_ops ? "d_ops" : old_bytes && !d_old ? "d_old"
                     : payload_bytes && !d_payload ? "d_payload" : dst_bytes && !d_dst ? "d_dst" : NULL;
    if (null) return fail(CW_ERR_BAD_ARG, "NULL pointer: %s", null);
    if ((rc = check_count("max_ops", max_ops)) != CW_OK) return rc;
    if ((rc = check_word_aligned((uintptr_t)d_ops, "d_ops")) != CW_OK || (rc = check_word_aligned((uintptr_t)d_nops, "d_nops")) != CW_OK ||
        (rc = check_word_aligned((uintptr_t)d_result, "d_result")) != CW_OK)
        return rc;
    if (ranges_overlap(d_dst, dst_bytes, d_old, old_bytes)) return fail(CW_ERR_BAD_ARG, "d_dst overlaps d_old");
    if (ranges_overlap(d_dst, dst_bytes, d_payload, payload_bytes)) return fail(CW_ERR_BAD_ARG, "d_dst overlaps d_payload");
    if ((rc = ensure_init()) != CW_OK) return rc;
    ProfScope prof(PROF_CODEC, (hipStream_t)stream);
    return launched(cw::apply_delta_launch((const uint8_t *)d_old, old_bytes, (const uint8_t *)d_payload, payload_bytes, d_ops, d_nops, max_ops,
                                           (uint8_t *)d_dst, dst_bytes, cw::apply_delta_tile_shift(cw::knobs().delta_tile), d_result,
                                           (hipStream_t)stream),
                    "apply delta launch");
}

// ---- chunk bundles between stores: export, import, translate (kernels: replicate_kernels.hip) ----------------------------------
int cw_dev_store_export_chunks(const void *d_store, size_t store_bytes, const cw_chunk_loc *d_dir, uint64_t dir_base, size_t dir_entries,
                               const uint64_t *d_values, const uint64_t *d_count, size_t max_count, void *d_out, size_t out_bytes,
                               cw_chunk_loc *d_out_loc, uint64_t *d_result, void *stream)
{
    int rc = check_count("max_count", max_count);
    if (rc != CW_OK) return rc;
    if (!d_dir || !d_values || !d_count || !d_out_loc || !d_result || (store_bytes && !d_store) || (out_bytes && !d_out))
        return fail(CW_ERR_BAD_ARG, "NULL pointer");
    if (dir_entries == 0) return fail(CW_ERR_BAD_ARG, "dir_entries is 0");
    if ((rc = check_dir_aligned((uintptr_t)d_dir | (uintptr_t)d_out_loc, "d_dir / d_out_loc")) != CW_OK) return rc;
    if ((rc = check_word_aligned((uintptr_t)d_values | (uintptr_t)d_count | (uintptr_t)d_result, "d_values / d_count / d_result")) != CW_OK) return rc;
    if (ranges_overlap(d_store, store_bytes, d_out, out_bytes)) return fail(CW_ERR_BAD_ARG, "d_out overlaps d_store");
    if ((rc = ensure_init()) != CW_OK) return rc;
    return launched_nomem(cw::store_export_launch((const uint8_t *)d_store, store_bytes, d_dir, dir_base, dir_entries, d_values, d_count, max_count,
                                                  (uint8_t *)d_out, out_bytes, d_out_loc, d_result, (hipStream_t)stream),
                          "store export launch");
}

int cw_dev_store_import_chunks(const void *d_in, size_t in_bytes, const cw_chunk_loc *d_in_loc, const uint64_t *d_count, size_t max_count,
                               const uint32_t *d_sel, const uint64_t *d_nsel, uint64_t base, void *d_store, size_t store_bytes, uint64_t *d_used,
                               cw_chunk_loc *d_dir, uint64_t dir_base, size_t dir_entries, uint64_t *d_result, void *stream)
{
    int rc = check_count("max_count", max_count);
    if (rc != CW_OK) return rc;
    if (!d_in_loc || !d_count || !d_used || !d_dir || !d_result || (in_bytes && !d_in) || (store_bytes && !d_store) || !d_sel != !d_nsel)
        return fail(CW_ERR_BAD_ARG, "NULL pointer");
    if (dir_entries == 0) return fail(CW_ERR_BAD_ARG, "dir_entries is 0");
    if ((rc = check_dir_aligned((uintptr_t)d_in_loc | (uintptr_t)d_dir, "d_in_loc / d_dir")) != CW_OK) return rc;
    if ((rc = check_word_aligned((uintptr_t)d_count | (uintptr_t)d_nsel | (uintptr_t)d_used | (uintptr_t)d_result,
                                 "d_count / d_nsel / d_used / d_result")) != CW_OK)
        return rc;
    if (ranges_overlap(d_in, in_bytes, d_store, store_bytes)) return fail(CW_ERR_BAD_ARG, "d_in overlaps d_store");
    if ((rc = ensure_init()) != CW_OK) return rc;
    return launched_nomem(cw::store_import_launch((const uint8_t *)d_in, in_bytes, d_in_loc, d_count, max_count, d_sel, d_nsel, base,
                                                  (uint8_t *)d_store, store_bytes, d_used, d_dir, dir_base, dir_entries, d_result, (hipStream_t)stream),
                          "store import launch");
}

int cw_dev_store_replace_chunks(const void *d_in, size_t in_bytes, const cw_chunk_loc *d_in_loc, const uint64_t *d_values, const uint64_t *d_count,
                                size_t max_count, void *d_store, size_t store_bytes, uint64_t *d_used, cw_chunk_loc *d_dir, uint64_t dir_base,
                                size_t dir_entries, uint64_t *d_result, void *stream)
{
    int rc = check_count("max_count", max_count);
    if (rc != CW_OK) return rc;
    if (!d_in_loc || !d_values || !d_count || !d_used || !d_dir || !d_result || (in_bytes && !d_in) || (store_bytes && !d_store))
        return fail(CW_ERR_BAD_ARG, "NULL pointer");
    if (dir_entries == 0) return fail(CW_ERR_BAD_ARG, "dir_entries is 0");
    if ((rc = check_dir_aligned((uintptr_t)d_in_loc | (uintptr_t)d_dir, "d_in_loc / d_dir")) != CW_OK) return rc;
    if ((rc = check_word_aligned((uintptr_t)d_values | (uintptr_t)d_count | (uintptr_t)d_used | (uintptr_t)d_result,
                                 "d_values / d_count / d_used / d_result")) != CW_OK)
        return rc;
    if (ranges_overlap(d_in, in_bytes, d_store, store_bytes)) return fail(CW_ERR_BAD_ARG, "d_in overlaps d_store");
    if ((rc = ensure_init()) != CW_OK) return rc;
    return launched_nomem(cw::store_replace_launch((const uint8_t *)d_in, in_bytes, d_in_loc, d_values, d_count, max_count, (uint8_t *)d_store,
                                                   store_bytes, d_used, d_dir, dir_base, dir_entries, d_result, (hipStream_t)stream),
                          "store replace launch");
}

int cw_dev_translate_refs(const uint64_t *d_ref, const uint64_t *d_count, size_t max_count, const uint64_t *d_from, const uint64_t *d_to,
                          const uint64_t *d_npairs, size_t max_pairs, uint64_t *d_out, uint64_t *d_n_missing, void *stream)
{
    int rc;
    if ((rc = check_count("max_count", max_count)) != CW_OK || (rc = check_count("max_pairs", max_pairs)) != CW_OK) return rc;
    if (!d_ref || !d_count || !d_from || !d_to || !d_npairs || !d_out || !d_n_missing) return fail(CW_ERR_BAD_ARG, "NULL pointer");
    if ((rc = check_word_aligned((uintptr_t)d_ref | (uintptr_t)d_count | (uintptr_t)d_from | (uintptr_t)d_to | (uintptr_t)d_npairs | (uintptr_t)d_out |
                                     (uintptr_t)d_n_missing,
                                 "a u64 pointer is")) != CW_OK)
        return rc;
    if ((rc = ensure_init()) != CW_OK) return rc;
    return launched(cw::translate_refs_launch(d_ref, d_count, max_count, d_from, d_to, d_npairs, max_pairs, d_out, d_n_missing, (hipStream_t)stream),
                    "translate refs launch");
}

// ---- guard stripes over the store's bytes, P alone or P and Q: update, check, rebuild (kernels: guard_kernels.hip), locate ------
size_t cw_store_guard_bytes(size_t store_bytes, size_t stripe, unsigned group)
{
    if (stripe < CW_GUARD_MIN_STRIPE || stripe > CW_GUARD_MAX_STRIPE || (stripe & (stripe - 1)) || group < 1 || group > CW_GUARD_MAX_GROUP) return 0;
    return cw::store_guard_groups(store_bytes, stripe, group) * stripe;
}

// Each operation has a single entry (P alone; d_guard_q is NULL) and a dual one (P and the GF(2^8) syndrome Q): `dual` says which was called.
// What the three operations refuse of store, geometry and guards; the dual entries refuse a missing Q first and the rest of Q last
static int guard_args(bool dual, const void *d_store, size_t store_bytes, size_t stripe, unsigned group, const void *d_guard, const void *d_guard_q,
                      size_t guard_bytes)
{
    int rc;
    if (dual && !d_guard_q) return fail(CW_ERR_BAD_ARG, "NULL pointer: d_guard_q");
    if (!d_guard || (store_bytes && !d_store)) return fail(CW_ERR_BAD_ARG, "NULL pointer: %s", !d_guard ? "d_guard" : "d_store");
    if (cw_store_guard_bytes(1, stripe, group) == 0)
        return fail(CW_ERR_BAD_ARG, "stripe %zu is no power of two in [65536, 2^30] or group %u is not in [1, 256]", stripe, group);
    if (guard_bytes < cw_store_guard_bytes(store_bytes, stripe, group))
        return fail(CW_ERR_BAD_ARG, "guard_bytes %zu < %zu, what a store of %zu bytes needs", guard_bytes, cw_store_guard_bytes(store_bytes, stripe, group),
                    store_bytes);
    if ((rc = check_count("the groups of store_bytes", cw::store_guard_groups(store_bytes, stripe, group))) != CW_OK) return rc;
    if ((rc = check_dir_aligned((uintptr_t)d_store | (uintptr_t)d_guard, "d_store / d_guard")) != CW_OK) return rc;
    if (ranges_overlap(d_store, store_bytes, d_guard, guard_bytes)) return fail(CW_ERR_BAD_ARG, "d_guard overlaps d_store");
    if (!dual) return CW_OK;
    if (group > CW_GUARD2_MAX_GROUP) return fail(CW_ERR_BAD_ARG, "group %u is not in [1, 255]: the dual guard's stripe weights 2^m repeat after 255", group);
    if ((rc = check_dir_aligned((uintptr_t)d_guard_q, "d_guard_q")) != CW_OK) return rc;
    if (ranges_overlap(d_store, store_bytes, d_guard_q, guard_bytes)) return fail(CW_ERR_BAD_ARG, "d_guard_q overlaps d_store");
    if (ranges_overlap(d_guard, guard_bytes, d_guard_q, guard_bytes)) return fail(CW_ERR_BAD_ARG, "d_guard_q overlaps d_guard_p");
    return CW_OK;
}

static int guard_update(bool dual, const void *d_store, size_t store_bytes, const uint64_t *d_used, uint64_t *d_covered, size_t stripe, unsigned group,
                        void *d_guard, void *d_guard_q, size_t guard_bytes, uint64_t *d_result, void *stream)
{
    int rc;
    const char *null = !d_used ? "d_used" : !d_covered ? "d_covered" : !d_result ? "d_result" : NULL;
    if (null) return fail(CW_ERR_BAD_ARG, "NULL pointer: %s", null);
    if ((rc = guard_args(dual, d_store, store_bytes, stripe, group, d_guard, d_guard_q, guard_bytes)) != CW_OK) return rc;
    if ((rc = check_word_aligned((uintptr_t)d_used | (uintptr_t)d_covered | (uintptr_t)d_result, "d_used / d_covered / d_result")) != CW_OK) return rc;
    if ((rc = ensure_init()) != CW_OK) return rc;
    return launched(cw::store_guard_update_launch((const uint8_t *)d_store, store_bytes, d_used, d_covered, stripe, group, d_guard, d_guard_q, d_result,
                                                  (hipStream_t)stream),
                    dual ? "store guard2 update launch" : "store guard update launch");
}

static int guard_check(bool dual, const void *d_store, size_t store_bytes, const uint64_t *d_covered, size_t stripe, unsigned group, const void *d_guard,
                       const void *d_guard_q, size_t guard_bytes, uint32_t *d_group_bad, uint64_t *d_result, void *stream)
{
    int rc;
    const char *null = !d_covered ? "d_covered" : !d_result ? "d_result" : NULL;
    if (null) return fail(CW_ERR_BAD_ARG, "NULL pointer: %s", null);
    if ((rc = guard_args(dual, d_store, store_bytes, stripe, group, d_guard, d_guard_q, guard_bytes)) != CW_OK) return rc;
    if ((rc = check_word_aligned((uintptr_t)d_covered | (uintptr_t)d_result, "d_covered / d_result")) != CW_OK) return rc;
    if ((uintptr_t)d_group_bad & 3) return fail(CW_ERR_BAD_ARG, "d_group_bad is not 4-byte aligned");
    if ((rc = ensure_init()) != CW_OK) return rc;
    return launched_nomem(cw::store_guard_check_launch((const uint8_t *)d_store, store_bytes, d_covered, stripe, group, d_guard, d_guard_q, d_group_bad,
                                                       d_result, (hipStream_t)stream),
                          dual ? "store guard2 check launch" : "store guard check launch");
}

static int guard_rebuild(bool dual, const void *d_store, size_t store_bytes, const cw_chunk_loc *d_dir, uint64_t dir_base, size_t dir_entries,
                         const uint64_t *d_covered, size_t stripe, unsigned group, const void *d_guard, const void *d_guard_q, size_t guard_bytes,
                         const uint64_t *d_values, const uint64_t *d_count, size_t max_count, void *d_out, size_t out_bytes, cw_chunk_loc *d_out_loc,
                         uint32_t *d_status, uint64_t *d_result, void *stream)
{
    int rc = check_count("max_count", max_count);
    if (rc != CW_OK) return rc;
    const char *null = !d_dir ? "d_dir" : !d_covered ? "d_covered" : !d_values ? "d_values" : !d_count ? "d_count" : !d_out_loc ? "d_out_loc"
                     : !d_status ? "d_status" : !d_result ? "d_result" : out_bytes && !d_out ? "d_out" : NULL;
    if (null) return fail(CW_ERR_BAD_ARG, "NULL pointer: %s", null);
    if (dir_entries == 0) return fail(CW_ERR_BAD_ARG, "dir_entries is 0");
    if ((rc = guard_args(dual, d_store, store_bytes, stripe, group, d_guard, d_guard_q, guard_bytes)) != CW_OK) return rc;
    if ((rc = check_dir_aligned((uintptr_t)d_dir | (uintptr_t)d_out_loc, "d_dir / d_out_loc")) != CW_OK) return rc;
    if ((rc = check_word_aligned((uintptr_t)d_covered | (uintptr_t)d_values | (uintptr_t)d_count | (uintptr_t)d_result,
                                 "d_covered / d_values / d_count / d_result")) != CW_OK)
        return rc;
    if ((uintptr_t)d_status & 3) return fail(CW_ERR_BAD_ARG, "d_status is not 4-byte aligned");
    if (ranges_overlap(d_store, store_bytes, d_out, out_bytes)) return fail(CW_ERR_BAD_ARG, "d_out overlaps d_store");
    if (ranges_overlap(d_guard, guard_bytes, d_out, out_bytes)) return fail(CW_ERR_BAD_ARG, "d_out overlaps %s", dual ? "d_guard_p" : "d_guard");
    if (dual && ranges_overlap(d_guard_q, guard_bytes, d_out, out_bytes)) return fail(CW_ERR_BAD_ARG, "d_out overlaps d_guard_q");
    if ((rc = ensure_init()) != CW_OK) return rc;
    return launched_nomem(cw::store_guard_rebuild_launch((const uint8_t *)d_store, store_bytes, d_dir, dir_base, dir_entries, d_covered, stripe, group,
                                                         d_guard, d_guard_q, d_values, d_count, max_count, (uint8_t *)d_out, out_bytes, d_out_loc, d_status,
                                                         d_result, (hipStream_t)stream),
                          dual ? "store guard2 rebuild launch" : "store guard rebuild launch");
}

// (kernels: guard_locate_kernels.hip; dir_base shifts no entry: the output is per entry, not per value)
static int guard_locate(bool dual, const void *d_store, size_t store_bytes, const cw_chunk_loc *d_dir, uint64_t dir_base, size_t dir_entries,
                        const uint64_t *d_covered, size_t stripe, unsigned group, const void *d_guard, const void *d_guard_q, size_t guard_bytes,
                        uint32_t *d_suspect, uint64_t *d_result, void *stream)
{
    (void)dir_base;
    int rc;
    const char *null = !d_dir ? "d_dir" : !d_covered ? "d_covered" : !d_suspect ? "d_suspect" : !d_result ? "d_result" : NULL;
    if (null) return fail(CW_ERR_BAD_ARG, "NULL pointer: %s", null);
    if (dir_entries == 0) return fail(CW_ERR_BAD_ARG, "dir_entries is 0");
    if ((rc = check_count("dir_entries", dir_entries)) != CW_OK) return rc;
    if ((rc = guard_args(dual, d_store, store_bytes, stripe, group, d_guard, d_guard_q, guard_bytes)) != CW_OK) return rc;
    if ((rc = check_dir_aligned((uintptr_t)d_dir, "d_dir")) != CW_OK) return rc;
    if ((rc = check_word_aligned((uintptr_t)d_covered | (uintptr_t)d_result, "d_covered / d_result")) != CW_OK) return rc;
    if ((uintptr_t)d_suspect & 3) return fail(CW_ERR_BAD_ARG, "d_suspect is not 4-byte aligned");
    if ((rc = ensure_init()) != CW_OK) return rc;
    return launched_nomem(cw::store_guard_locate_launch((const uint8_t *)d_store, store_bytes, d_dir, dir_entries, d_covered, stripe, group, d_guard,
                                                        d_guard_q, d_suspect, d_result, (hipStream_t)stream),
                          dual ? "store guard2 locate launch" : "store guard locate launch");
}

int cw_dev_store_guard_update(const void *d_store, size_t store_bytes, const uint64_t *d_used, uint64_t *d_covered, size_t stripe, unsigned group,
                              void *d_guard, size_t guard_bytes, uint64_t *d_result, void *stream)
{
    return guard_update(false, d_store, store_bytes, d_used, d_covered, stripe, group, d_guard, NULL, guard_bytes, d_result, stream);
}

int cw_dev_store_guard2_update(const void *d_store, size_t store_bytes, const uint64_t *d_used, uint64_t *d_covered, size_t stripe, unsigned group,
                               void *d_guard_p, void *d_guard_q, size_t guard_bytes, uint64_t *d_result, void *stream)
{
    return guard_update(true, d_store, store_bytes, d_used, d_covered, stripe, group, d_guard_p, d_guard_q, guard_bytes, d_result, stream);
}

int cw_dev_store_guard_check(const void *d_store, size_t store_bytes, const uint64_t *d_covered, size_t stripe, unsigned group, const void *d_guard,
                             size_t guard_bytes, uint32_t *d_group_bad, uint64_t *d_result, void *stream)
{
    return guard_check(false, d_store, store_bytes, d_covered, stripe, group, d_guard, NULL, guard_bytes, d_group_bad, d_result, stream);
}

int cw_dev_store_guard2_check(const void *d_store, size_t store_bytes, const uint64_t *d_covered, size_t stripe, unsigned group,
                              const void *d_guard_p, const void *d_guard_q, size_t guard_bytes, uint32_t *d_group_bad, uint64_t *d_result, void *stream)
{
    return guard_check(true, d_store, store_bytes, d_covered, stripe, group, d_guard_p, d_guard_q, guard_bytes, d_group_bad, d_result, stream);
}

int cw_dev_store_guard_rebuild(const void *d_store, size_t store_bytes, const cw_chunk_loc *d_dir, uint64_t dir_base, size_t dir_entries,
                               const uint64_t *d_covered, size_t stripe, unsigned group, const void *d_guard, size_t guard_bytes,
                               const uint64_t *d_values, const uint64_t *d_count, size_t max_count, void *d_out, size_t out_bytes,
                               cw_chunk_loc *d_out_loc, uint32_t *d_status, uint64_t *d_result, void *stream)
{
    return guard_rebuild(false, d_store, store_bytes, d_dir, dir_base, dir_entries, d_covered, stripe, group, d_guard, NULL, guard_bytes, d_values, d_count,
                         max_count, d_out, out_bytes, d_out_loc, d_status, d_result, stream);
}

int cw_dev_store_guard2_rebuild(const void *d_store, size_t store_bytes, const cw_chunk_loc *d_dir, uint64_t dir_base, size_t dir_entries,
                                const uint64_t *d_covered, size_t stripe, unsigned group, const void *d_guard_p, const void *d_guard_q,
                                size_t guard_bytes, const uint64_t *d_values, const uint64_t *d_count, size_t max_count, void *d_out, size_t out_bytes,
                                cw_chunk_loc *d_out_loc, uint32_t *d_status, uint64_t *d_result, void *stream)
{
    return guard_rebuild(true, d_store, store_bytes, d_dir, dir_base, dir_entries, d_covered, stripe, group, d_guard_p, d_guard_q, guard_bytes, d_values,
                         d_count, max_count, d_out, out_bytes, d_out_loc, d_status, d_result, stream);
}

int cw_dev_store_guard_locate(const void *d_store, size_t store_bytes, const cw_chunk_loc *d_dir, uint64_t dir_base, size_t dir_entries,
                              const uint64_t *d_covered, size_t stripe, unsigned group, const void *d_guard, size_t guard_bytes, uint32_t *d_suspect,
                              uint64_t *d_result, void *stream)
{
    return guard_locate(false, d_store, store_bytes, d_dir, dir_base, dir_entries, d_covered, stripe, group, d_guard, NULL, guard_bytes, d_suspect,
                        d_result, stream);
}

int cw_dev_store_guard2_locate(const void *d_store, size_t store_bytes, const cw_chunk_loc *d_dir, uint64_t dir_base, size_t dir_entries,
                               const uint64_t *d_covered, size_t stripe, unsigned group, const void *d_guard_p, const void *d_guard_q,
                               size_t guard_bytes, uint32_t *d_suspect, uint64_t *d_result, void *stream)
{
    return guard_locate(true, d_store, store_bytes, d_dir, dir_base, dir_entries, d_covered, stripe, group, d_guard_p, d_guard_q, guard_bytes, d_suspect,
                        d_result, stream);
}

} // extern "C"
