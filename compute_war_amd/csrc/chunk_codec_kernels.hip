// chunk_codec_kernels.hip -- LZ4 / LZF over content-defined chunks: every chunk has its own length,
// 1 .. 65536 bytes, given by an offset list on the device (cw_dev_cdc's), optionally a selection of it (cw_dev_dedupe's list
// of new chunks).  The fixed-size parsers are all tied to one block size per launch; what carries over is the lane-per-block
// form (lz4_lanes_kernel, lzf_lanes_kernel: DESIGN.md 4.3): a LANE owns a chunk and runs the serial parser as it stands, its
// hash table in global memory, bound by the random lines the memory system retires once the chip holds tens of thousands of
// chains -- which chunking supplies (4 GiB at the 8 KiB defaults are 459 k chunks).  Here the length, the limits derived from
// it, the source and the slot are lane values, and:
//   * the table is not zeroed per chunk (32 KiB / 256 KiB against ~9 KiB of input): entries carry an epoch, an entry of another
//     epoch reads as the zeroed table would, and the lane's epoch outlives the launch in a word per lane;
//   * chunks are taken longest first from a counting sort of the positions (lengths span 32x: the lanes of a wavefront then
//     finish together), through one work counter;
//   * compressed chunk i goes to the slot cw_chunk_slot_offset(alg, offsets[i], i), known before the parse.
// The decoder is decompress_lanes_kernel with per-lane extents.  Out-of-contract chunks (empty, longer than 65536, decreasing,
// past the source) get size 0 and are never loaded or stored.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cw_device.h"
#include "lz_device.h"
#include "stream_scratch.h"

namespace cw {

namespace {

using lz::rd32;

constexpr uint32_t kMaxChunk = 65536;
constexpr uint32_t kMinMatch = 4, kLastLiterals = 5, kMFLimit = 12;
constexpr uint32_t kLz4Slots = 1u << 13, kLzfSlots = 1u << 16; // u32 entries: 32 KiB / 256 KiB per lane
constexpr uint32_t kMaxOff = 1u << 13, kMaxRef = (1u << 8) + (1u << 3), kMaxLit = 32;

__device__ __forceinline__ uint64_t umin64(uint64_t a, uint64_t b) { return a < b ? a : b; }

// ---- the positions of a call and the chunk behind each -------------------------------------------------------------------
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
        if (!(s < e && e <= src_bytes && e - s <= kMaxChunk)) return 0;
        start = s;
        return (uint32_t)(e - s);
    }
};

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

// ---- LZ4 -------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t hash13(uint32_t v) { return (v * 2654435761u) >> 19; }
// 8 further bits of the hash product (lz4_lanes_kernel's fingerprint, shortened to make room for the epoch)
__device__ __forceinline__ uint32_t fp8(uint32_t v) { return ((v * 2654435761u) >> 11) & 0xFFu; }
__device__ __forceinline__ uint4 ld16g(const uint8_t *p)
{
    uint4 v;
    __builtin_memcpy(&v, p, 16); // unaligned global_load_dwordx4
    return v;
}
__device__ __forceinline__ void lane_put_len(uint8_t *__restrict__ out, uint32_t &op, uint32_t extra)
{
    while (extra >= 255) { out[op++] = 255; extra -= 255; }
    out[op++] = (uint8_t)extra;
}
// 4 bytes at byte offset s (4 <= s <= 12) of a 16-byte window held in (x, y, z, w)
__device__ __forceinline__ uint32_t win_at(const uint4 &q, uint32_t s)
{
    return s < 8 ? __builtin_amdgcn_alignbyte(q.z, q.y, s & 3u) : s < 12 ? __builtin_amdgcn_alignbyte(q.w, q.z, s & 3u) : q.w;
}
// stores exactly cnt (1..16) bytes of (a, b)
__device__ __forceinline__ void store_upto16(uint8_t *p, uint64_t a, uint64_t b, uint32_t cnt)
{
    if (cnt & 16) { __builtin_memcpy(p, &a, 8); __builtin_memcpy(p + 8, &b, 8); return; }
    if (cnt & 8) { __builtin_memcpy(p, &a, 8); a = b; p += 8; }
    if (cnt & 4) { const uint32_t t = (uint32_t)a; __builtin_memcpy(p, &t, 4); a >>= 32; p += 4; }
    if (cnt & 2) { const uint16_t t = (uint16_t)a; __builtin_memcpy(p, &t, 2); a >>= 16; p += 2; }
    if (cnt & 1) *p = (uint8_t)a;
}

enum : uint32_t { LS_NEXT = 0, LS_PROBE = 1, LS_EMIT = 2, LS_TAIL = 3, LS_EXIT = 4 };

// lz4_lanes_kernel's loop (lz4_kernel.hip has the reasoning: states, the window requested an iteration ahead, the literals
// stored an iteration late) with the chunk's length n in a lane register.  Table entry: epoch:8 | fingerprint:8 | position:16.
// An entry whose upper half is not (epoch, fingerprint of the 4 bytes looked up) is not a candidate: either it is of another
// chunk -- the zeroed table's "position 0", which can only match the chunk's first 4 bytes, and those are entered by name when
// the chunk is taken, as kLaneFp does -- or it holds other bytes.  All loads stay inside the chunk (n >= 13 on this path: the
// parser's own limits see to it), shorter chunks are last literals only.  The literal copies may overshoot by up to 7 bytes
// into what the sequence's offset and the bytes behind it overwrite, never past the output's final size.
__global__ void __launch_bounds__(64)
lz4_chunks_kernel(const uint8_t *__restrict__ src, ChunkList c, const uint32_t *__restrict__ order, uint8_t *__restrict__ dst,
                  uint32_t *__restrict__ sizes, uint32_t *__restrict__ tables, uint32_t *__restrict__ epochs, unsigned long long *__restrict__ work)
{
    const uint64_t npos = c.npos(), count = c.nchunks();
    if ((uint64_t)blockIdx.x * 64 >= npos) return; // fewer positions than lanes: the first workgroups take them with every lane busy
    const size_t lane_id = (size_t)blockIdx.x * 64 + threadIdx.x;
    uint32_t *tab = tables + lane_id * kLz4Slots;
    uint32_t epoch = epochs[lane_id]; // 0 on a fresh (zeroed) table
    uint32_t n = 0, mflimit = 0, matchlimit = 0;
    auto tab_get = [&](uint32_t h, uint32_t v, bool &maybe) -> uint32_t {
        const uint32_t e = tab[h];
        maybe = (e >> 16) == ((epoch << 8) | fp8(v));
        return e & 0xFFFFu;
    };
    auto tab_put = [&](uint32_t h, uint32_t v, uint32_t pos) { tab[h] = (epoch << 24) | (fp8(v) << 16) | pos; };

    uint32_t state = LS_NEXT;
    const uint8_t *g = src;
    uint8_t *out = dst;
    uint32_t blk = 0, ip = 0, anchor = 0, op = 0, step = 1, nb = 64, match = 0, first_lo = 0, first_hi = 0;
    bool retest = false;
    uint4 own = make_uint4(0, 0, 0, 0), cd = make_uint4(0, 0, 0, 0);
    uint32_t vcur = 0, v2cur = 0;
    bool have_v = false;
    uint64_t pend_a = 0, pend_b = 0;
    uint8_t *pend_dst = nullptr;
    uint32_t pend_n = 0;

    while (__ballot(state != LS_EXIT)) {
        if (pend_n) { // exactly pend_n (1..16) bytes: what follows them in the slot is already written
            store_upto16(pend_dst, pend_a, pend_b, pend_n);
            pend_n = 0;
        }
        if (state == LS_NEXT) {
            const unsigned long long qi = atomicAdd(work, 1ull);
            if (qi >= npos) {
                state = LS_EXIT;
            } else {
                blk = order[qi];
                uint64_t i, start;
                n = c.chunk(blk, count, i, start);
                if (n == 0) {
                    sizes[blk] = 0; // out of contract: nothing loaded, nothing stored; the lane asks again
                } else {
                    g = src + start;
                    out = dst + chunk_slot_offset(true, start, i);
                    anchor = 0; op = 0;
                    if (n < kMFLimit + 1) {
                        state = LS_TAIL;
                    } else {
                        mflimit = n - kMFLimit; matchlimit = n - kLastLiterals;
                        if (++epoch == 256) {
                            uint4 *t4 = reinterpret_cast<uint4 *>(tab);
                            for (uint32_t k = 0; k < kLz4Slots * 4 / 16; k++) t4[k] = make_uint4(0, 0, 0, 0);
                            epoch = 1;
                        }
                        first_lo = rd32(g, 0); first_hi = rd32(g, 4);
                        tab_put(hash13(first_lo), first_lo, 0);
                        ip = 1; step = 1; nb = 64; retest = false;
                        own.x = 0; own.y = rd32(g, 1); own.z = rd32(g, 5); own.w = rd32(g, 9); // no "before" at the chunk's start
                        have_v = false;
                        state = LS_PROBE;
                    }
                }
            }
        }

        if (state == LS_PROBE) {
            const uint32_t next = ip + step;
            if (!retest && next > mflimit + 1) {
                state = LS_TAIL;
            } else {
                const uint32_t v = have_v ? vcur : own.y;
                if (retest) { // LZ4_putPosition(ip - 2) in front of the re-test
                    const uint32_t v2 = have_v ? v2cur : (own.x >> 16) | (own.y << 16);
                    tab_put(hash13(v2), v2, ip - 2);
                }
                const uint32_t h = hash13(v);
                bool maybe;
                match = tab_get(h, v, maybe);
                tab_put(h, v, ip);
                uint32_t cat = ~v;
                if (maybe) {
                    if (match >= 4) { cd = ld16g(g + match - 4); cat = cd.y; }
                    else cat = __builtin_amdgcn_alignbyte(first_hi, first_lo, match);
                }
                if (cat == v) {
                    state = LS_EMIT;
                } else {
                    uint32_t nip;
                    if (retest) { nip = ip + 1; step = 1; nb = 64; retest = false; }
                    else { nip = next; step = nb >> 6; nb++; }
                    const uint32_t s = nip - ip + 4;
                    have_v = s <= 12 && ip >= 4;
                    if (have_v) vcur = win_at(own, s);
                    ip = nip;
                    // (ip = mflimit + 1 is never probed, the next iteration sends it to TAIL: keep its request inside the chunk)
                    const uint32_t rp = ip <= mflimit ? ip : mflimit;
                    if (rp >= 4) own = ld16g(g + rp - 4); // [rp - 4, rp + 12), rp + 12 <= n
                    else { own.x = 0; own.y = rd32(g, rp); own.z = rd32(g, rp + 4); own.w = rd32(g, rp + 8); have_v = false; } // (16 bytes from rp may leave a short chunk)
                }
            }
        }

        if (state == LS_EMIT) {
            // own = [ip-4, ip+12) and cd = [match-4, match+12) (match >= 4), both as found by the probe
            const uint32_t ip0 = ip;
            const bool windows = ip >= 4 && match >= 4;
            uint32_t nf = 0; // equal bytes behind the 4 that matched
            bool nf_open = true;
            if (windows) {
                const uint64_t x = ((uint64_t)own.w << 32 | own.z) ^ ((uint64_t)cd.w << 32 | cd.z);
                nf = x ? (uint32_t)__builtin_ctzll(x) >> 3 : 8u;
                nf_open = nf == 8;
                const uint32_t lim = matchlimit - (ip0 + kMinMatch);
                if (nf >= lim) { nf = lim; nf_open = false; }
            }
            // ---- catch-up over the pending literals (a re-test has none: anchor == ip) ----
            if (!retest) {
                if (windows) {
                    const uint32_t room = ip - anchor < match ? ip - anchor : match;
                    const uint32_t y = own.x ^ cd.x;
                    uint32_t back = y ? (uint32_t)__builtin_clz(y) >> 3 : 4u;
                    if (back > room) back = room;
                    ip -= back; match -= back;
                    if (back == 4) while (ip > anchor && match > 0 && g[ip - 1] == g[match - 1]) { ip--; match--; }
                } else {
                    while (ip > anchor && match > 0 && g[ip - 1] == g[match - 1]) { ip--; match--; }
                }
            }
            // ---- literals: 8 or 16 bytes requested now and stored next iteration; longer runs copied here ----
            const uint32_t lit = ip - anchor, tok = op++;
            uint32_t token;
            if (lit >= 15) { token = 15u << 4; lane_put_len(out, op, lit - 15); }
            else token = lit << 4;
            if (lit) {
                // (8 bytes from anchor stay inside the chunk: anchor + 8 <= ip + 7 <= n - 5; 16 only for runs of 9 and more)
                __builtin_memcpy(&pend_a, g + anchor, 8);
                if (lit > 8) __builtin_memcpy(&pend_b, g + anchor + 8, 8);
                pend_dst = out + op;
                pend_n = lit < 16 ? lit : 16;
                for (uint32_t k = 16; k < lit; k += 8) { // the overshoot (< 8 bytes) lands where the offset and what follows are written next
                    uint64_t q;
                    __builtin_memcpy(&q, g + anchor + k, 8);
                    __builtin_memcpy(out + op + k, &q, 8);
                }
            }
            op += lit;
            // ---- offset, match length ----
            const uint32_t off = ip - match;
            out[op] = (uint8_t)off; out[op + 1] = (uint8_t)(off >> 8);
            op += 2;
            uint32_t mc = ip0 - ip + nf; // the bytes taken back, the 4 that matched and the nf behind them are one run
            if (nf_open) {
                const uint32_t a = ip + kMinMatch, b = match + kMinMatch;
                while (a + mc + 8 <= matchlimit) {
                    uint64_t x, y;
                    __builtin_memcpy(&x, g + a + mc, 8);
                    __builtin_memcpy(&y, g + b + mc, 8);
                    const uint64_t d = x ^ y;
                    if (d) { mc += (uint32_t)__builtin_ctzll(d) >> 3; break; }
                    mc += 8;
                }
                if (a + mc + 8 > matchlimit) while (a + mc < matchlimit && g[a + mc] == g[b + mc]) mc++;
            }
            if (mc >= 15) { token += 15; lane_put_len(out, op, mc - 15); }
            else token += mc;
            out[tok] = (uint8_t)token;
            ip += kMinMatch + mc;
            anchor = ip;
            if (ip > mflimit) {
                state = LS_TAIL;
            } else {
                const uint32_t s = ip - ip0 + 4;
                have_v = windows && s <= 12;
                if (have_v) { vcur = win_at(own, s); v2cur = win_at(own, s - 2); }
                own = ld16g(g + ip - 4); // ip >= 5, ip + 12 <= n
                retest = true;
                state = LS_PROBE;
            }
        }

        if (state == LS_TAIL) {
            const uint32_t run = n - anchor;
            if (run >= 15) { out[op++] = 15u << 4; lane_put_len(out, op, run - 15); }
            else out[op++] = (uint8_t)(run << 4);
            uint32_t k = 0;
            for (; k + 16 <= run; k += 16) {
                uint4 q;
                __builtin_memcpy(&q, g + anchor + k, 16);
                __builtin_memcpy(out + op + k, &q, 16);
            }
            for (; k < run; k++) out[op + k] = g[anchor + k];
            op += run;
            sizes[blk] = op;
            state = LS_NEXT;
        }
    }
    epochs[lane_id] = epoch;
}

// ---- LZF -------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t lzf_slot(uint32_t b0, uint32_t b1, uint32_t b2)
{
    // IDX(hval) = ((hval >> 8) - hval*5) & 0xFFFF with hval = b0<<16 | b1<<8 | b2 (VERY_FAST, HLOG 16)
    return (((b0 << 8) | b1) - (((b1 << 8) | b2) * 5u)) & 0xFFFFu;
}
// up to 4 bytes at ip, none from behind the chunk
__device__ __forceinline__ uint32_t chunk_rd(const uint8_t *g, uint32_t ip, uint32_t n)
{
    if (ip + 4 <= n) return rd32(g, ip);
    uint32_t v = 0;
    for (uint32_t k = 0; k < 4; k++) if (ip + k < n) v |= (uint32_t)g[ip + k] << (8 * k);
    return v;
}

// lzf_lanes_kernel's loop (liblzf's, one position per iteration) with the chunk's length in a lane register and out_len = n - 1
// as the reference calls it.  Table entry: epoch:16 | position:16; another epoch reads as 0, which liblzf takes for "no
// reference".  No bail-out for chunks that do not compress (out of scope: DESIGN.md 12); size 0 = did not fit.
__global__ void __launch_bounds__(64)
lzf_chunks_kernel(const uint8_t *__restrict__ src, ChunkList c, const uint32_t *__restrict__ order, uint8_t *__restrict__ dst,
                  uint32_t *__restrict__ sizes, uint32_t *__restrict__ tables, uint32_t *__restrict__ epochs, unsigned long long *__restrict__ work)
{
    const uint64_t npos = c.npos(), count = c.nchunks();
    if ((uint64_t)blockIdx.x * 64 >= npos) return;
    const size_t lane_id = (size_t)blockIdx.x * 64 + threadIdx.x;
    uint32_t *tab = tables + lane_id * kLzfSlots;
    uint32_t epoch = epochs[lane_id];
    auto tab_get = [&](uint32_t slot) -> uint32_t {
        const uint32_t e = tab[slot];
        return (e >> 16) == epoch ? e & 0xFFFFu : 0u;
    };
    auto tab_put = [&](uint32_t slot, uint32_t pos) { tab[slot] = (epoch << 16) | pos; };
    enum : uint32_t { NEXT = 0, STEP = 1, TAIL = 2, EXIT = 3 };
    uint32_t state = NEXT, ip = 0, op = 0, lit = 0, v = 0, n = 0, cap = 0, blk = 0;
    const uint8_t *g = src;
    uint8_t *out = dst;
    bool fail = false;

    while (__ballot(state != EXIT)) {
        if (state == NEXT) {
            const unsigned long long qi = atomicAdd(work, 1ull);
            if (qi >= npos) {
                state = EXIT;
            } else {
                blk = order[qi];
                uint64_t i, start;
                n = c.chunk(blk, count, i, start);
                if (n == 0) {
                    sizes[blk] = 0;
                } else {
                    g = src + start;
                    out = dst + chunk_slot_offset(false, start, i);
                    cap = n - 1;
                    if (++epoch == 65536) {
                        uint4 *t4 = reinterpret_cast<uint4 *>(tab);
                        for (uint32_t k = 0; k < kLzfSlots * 4 / 16; k++) t4[k] = make_uint4(0, 0, 0, 0);
                        epoch = 1;
                    }
                    ip = 0; op = 1; lit = 0; fail = false; // op = 1: the first literal run's control byte is reserved
                    if (n >= 3) { v = chunk_rd(g, 0, n); state = STEP; }
                    else state = TAIL;
                }
            }
        }

        if (state == STEP) { // ip + 2 < n; v = the bytes at ip
            const uint32_t b0 = v & 0xFFu, b1 = (v >> 8) & 0xFFu, b2 = (v >> 16) & 0xFFu;
            const uint32_t slot = lzf_slot(b0, b1, b2);
            const uint32_t ref = tab_get(slot);
            tab_put(slot, ip);
            bool is_match = false;
            if (ref > 0 && ip - ref - 1 < kMaxOff) is_match = ((rd32(g, ref) ^ v) & 0xFFFFFFu) == 0; // ref + 4 <= ip + 3 <= n
            if (is_match) {
                uint32_t maxlen = n - ip - 2;
                if (maxlen > kMaxRef) maxlen = kMaxRef;
                if (op + 4 >= cap && op - (lit == 0) + 4 >= cap) {
                    fail = true; state = TAIL;
                } else {
                    if (lit) out[op - lit - 1] = (uint8_t)(lit - 1);
                    else op -= 1;
                    // equal bytes from index 3 on, as far as the reference's loops can look
                    const uint32_t room = (n - ip < kMaxRef + 2 ? n - ip : kMaxRef + 2) - 3;
                    uint32_t eq = 0;
                    while (eq + 8 <= room) {
                        uint64_t x, y;
                        __builtin_memcpy(&x, g + ref + 3 + eq, 8);
                        __builtin_memcpy(&y, g + ip + 3 + eq, 8);
                        const uint64_t d = x ^ y;
                        if (d) { eq += (uint32_t)__builtin_ctzll(d) >> 3; break; }
                        eq += 8;
                    }
                    if (eq + 8 > room) while (eq < room && g[ref + 3 + eq] == g[ip + 3 + eq]) eq++;
                    uint32_t len;
                    if (maxlen > 16) { // 16 unrolled compares without a bound, then the bounded loop
                        if (eq < 16) len = 3 + eq;
                        else { len = 3 + eq < maxlen ? 3 + eq : maxlen; if (len < 19) len = 19; }
                    } else {
                        len = 3 + eq < maxlen ? 3 + eq : maxlen;
                        if (len < 3) len = 3;
                    }
                    const uint32_t off = ip - ref - 1, l2 = len - 2;
                    if (l2 < 7) {
                        out[op] = (uint8_t)((off >> 8) + (l2 << 5));
                        out[op + 1] = (uint8_t)off;
                        op += 2;
                    } else {
                        out[op] = (uint8_t)((off >> 8) + (7u << 5));
                        out[op + 1] = (uint8_t)(l2 - 7);
                        out[op + 2] = (uint8_t)off;
                        op += 3;
                    }
                    lit = 0; op += 1;
                    ip += len;
                    if (ip + 2 >= n) {
                        state = TAIL;
                    } else { // VERY_FAST: only the last two positions of the match are inserted
                        const uint32_t w = rd32(g, ip - 2); // bytes ip-2 .. ip+1
                        tab_put(lzf_slot(w & 0xFFu, (w >> 8) & 0xFFu, (w >> 16) & 0xFFu), ip - 2);
                        tab_put(lzf_slot((w >> 8) & 0xFFu, (w >> 16) & 0xFFu, w >> 24), ip - 1);
                        v = chunk_rd(g, ip, n);
                    }
                }
            } else {
                if (op >= cap) {
                    fail = true; state = TAIL;
                } else {
                    lit++;
                    out[op++] = (uint8_t)b0;
                    if (lit == kMaxLit) { out[op - lit - 1] = (uint8_t)(kMaxLit - 1); lit = 0; op++; }
                    ip++;
                    if (ip + 2 < n) v = (v >> 8) | ((uint32_t)(ip + 3 < n ? g[ip + 3] : 0u) << 24);
                    else state = TAIL;
                }
            }
        }

        if (state == TAIL) {
            if (!fail) {
                if (op + 3 > cap) {
                    fail = true;
                } else {
                    while (ip < n) {
                        lit++;
                        out[op++] = g[ip++];
                        if (lit == kMaxLit) { out[op - lit - 1] = (uint8_t)(kMaxLit - 1); lit = 0; op++; }
                    }
                    if (lit) out[op - lit - 1] = (uint8_t)(lit - 1);
                    else op -= 1;
                }
            }
            sizes[blk] = fail ? 0u : op;
            state = NEXT;
        }
    }
    epochs[lane_id] = epoch;
}

// ---- decoders ----------------------------------------------------------------------------------------------------------------
// d[op .. op+len) = d[op-off ..), the format's overlapping copy; off >= 1, op - off >= 0, op + len <= cap (checked by the caller)
__device__ __forceinline__ void lane_copy_match(uint8_t *d, uint32_t op, uint32_t off, uint32_t len, uint32_t cap)
{
    const uint32_t base = op - off, end = op + len;
    uint32_t dist = off;
    while (op < end) {
        while (dist < 16 && 2 * dist <= op - base) dist *= 2; // any multiple of off that is already written is a period
        const uint32_t left = end - op, piece = left < 16 ? left : 16, cnt = piece < dist ? piece : dist;
        const uint32_t s = op - dist;
        if (s + 16 <= cap) {
            uint64_t a, b;
            __builtin_memcpy(&a, d + s, 8);
            __builtin_memcpy(&b, d + s + 8, 8);
            store_upto16(d + op, a, b, cnt);
        } else {
            for (uint32_t k = 0; k < cnt; k++) d[op + k] = d[s + k];
        }
        op += cnt;
    }
}
// d[op .. op+len) = in[ip ..): literal bytes; ip + len <= n and op + len <= cap checked by the caller
__device__ __forceinline__ void lane_copy_literals(uint8_t *d, uint32_t op, const uint8_t *in, uint32_t ip, uint32_t len, uint32_t n)
{
    for (uint32_t k = 0; k < len; k += 16) {
        const uint32_t cnt = len - k < 16 ? len - k : 16;
        if (ip + k + 16 <= n) {
            uint64_t a, b;
            __builtin_memcpy(&a, in + ip + k, 8);
            __builtin_memcpy(&b, in + ip + k + 8, 8);
            store_upto16(d + op + k, a, b, cnt);
        } else {
            for (uint32_t j = 0; j < cnt; j++) d[op + k + j] = in[ip + k + j];
        }
    }
}

// decompress_lanes_kernel with the compressed extent [comp_off[j], comp_off[j+1]) and the raw extent [raw_off[j], raw_off[j+1])
// as lane values: every step is checked against them, as there against n and block_bytes.  status: 0 = well formed and exactly
// the raw extent produced; 1 otherwise, including an empty compressed extent and a raw extent that is decreasing, longer than
// 65536 or past dst_bytes (then nothing is loaded or stored).
template <int ALG>
__global__ void __launch_bounds__(64)
decompress_chunks_kernel(const uint8_t *__restrict__ comp, const uint64_t *__restrict__ comp_off, const uint64_t *__restrict__ raw_off,
                         const uint64_t *__restrict__ d_count, uint64_t max_count, uint8_t *__restrict__ dst, uint64_t dst_bytes,
                         uint32_t *__restrict__ status)
{
    const uint64_t total = umin64(*d_count, max_count), lanes = (uint64_t)gridDim.x * 64;
    for (uint64_t j = (uint64_t)blockIdx.x * 64 + threadIdx.x; j < total; j += lanes) {
        const uint64_t cs = comp_off[j], ce = comp_off[j + 1], rs = raw_off[j], re = raw_off[j + 1];
        bool bad = ce <= cs || ce - cs > (1u << 24) || re < rs || re - rs > kMaxChunk || re > dst_bytes;
        const uint8_t *in = comp + (bad ? 0 : cs);
        uint8_t *d = dst + (bad ? 0 : rs);
        const uint32_t n = bad ? 0u : (uint32_t)(ce - cs), block_bytes = bad ? 0u : (uint32_t)(re - rs);
        uint32_t ip = 0, op = 0;
        if (ALG == 0) {
            while (!bad) {
                if (ip >= n) { bad = true; break; }
                // token, a literal run of up to 13 bytes and the offset in one window when the extent has 16 bytes left
                uint32_t w0 = 0, w1 = 0, w2 = 0, w3 = 0;
                const bool win = ip + 16 <= n;
                if (win) { uint4 q; __builtin_memcpy(&q, in + ip, 16); w0 = q.x; w1 = q.y; w2 = q.z; w3 = q.w; }
                const uint32_t tok = win ? w0 & 0xFFu : in[ip];
                uint32_t lit = tok >> 4, ml = tok & 15;
                uint32_t off;
                if (win && lit <= 13) {
                    if (lit > block_bytes - op) { bad = true; break; }
                    const uint64_t lo = (uint64_t)w1 << 32 | w0, hi = (uint64_t)w3 << 32 | w2;
                    const uint64_t a = lo >> 8 | hi << 56, b = hi >> 8;
                    if (lit) store_upto16(d + op, a, b, lit);
                    op += lit;
                    ip += 1 + lit;
                    if (ip == n) break;
                    const uint32_t sh = (1 + lit) * 8; // offset = window bytes [1 + lit, 3 + lit)
                    const uint64_t o = sh < 64 ? (lo >> sh | (sh ? hi << (64 - sh) : 0)) : hi >> (sh - 64);
                    off = (uint32_t)o & 0xFFFFu;
                    ip += 2;
                } else {
                    ip++;
                    if (lit == 15) {
                        uint32_t x;
                        do { if (ip >= n) { bad = true; break; } x = in[ip]; ip++; lit += x; } while (x == 255);
                        if (bad) break;
                    }
                    if (lit > n - ip || lit > block_bytes - op) { bad = true; break; }
                    lane_copy_literals(d, op, in, ip, lit, n);
                    ip += lit; op += lit;
                    if (ip == n) break; // last sequence: literals only
                    if (n - ip < 2) { bad = true; break; }
                    off = (uint32_t)in[ip] | ((uint32_t)in[ip + 1] << 8);
                    ip += 2;
                }
                if (off == 0 || off > op) { bad = true; break; }
                if (ml == 15) {
                    uint32_t x;
                    do { if (ip >= n) { bad = true; break; } x = in[ip]; ip++; ml += x; } while (x == 255);
                    if (bad) break;
                }
                if (ml > block_bytes || ml + 4 > block_bytes - op) { bad = true; break; }
                ml += 4;
                lane_copy_match(d, op, off, ml, block_bytes);
                op += ml;
            }
        } else {
            while (!bad && ip < n) {
                const uint32_t ctrl = in[ip]; ip++;
                if (ctrl < 32) {
                    const uint32_t run = ctrl + 1;
                    if (run > n - ip || run > block_bytes - op) { bad = true; break; }
                    lane_copy_literals(d, op, in, ip, run, n);
                    ip += run; op += run;
                } else {
                    uint32_t len = ctrl >> 5;
                    if (ip >= n) { bad = true; break; }
                    if (len == 7) { len += in[ip]; ip++; if (ip >= n) { bad = true; break; } }
                    const uint32_t off = (((ctrl & 0x1f) << 8) | in[ip]) + 1; ip++;
                    len += 2;
                    if (off > op || len > block_bytes - op) { bad = true; break; }
                    lane_copy_match(d, op, off, len, block_bytes);
                    op += len;
                }
            }
        }
        if (op != block_bytes) bad = true;
        status[j] = bad ? 1u : 0u;
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
