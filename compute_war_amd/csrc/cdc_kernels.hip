// cdc_kernels.hip -- content-defined chunking for gfx950.
//
// Semantics (include/cw_hashcompress.h): window gear hash H(i) = 2 H(i-1) + gear[b[i]] over the whole stream, never reset,
// and FastCDC's normalized cut rule with min / normal / max sizes m <= a <= M.  Because H(i) depends only on the 64 bytes
// ending at i, the candidate bits of every position are computed in parallel with no knowledge of the cuts.
//
// 1. scan: lane k owns virtual positions [64k, 64k + 64) (virtual = real + the 16-byte misalignment of d_src); it runs the
//    recurrence over the 64 bytes before its run (warm-up) and then its own 64 bytes, with a copy of the gear table per bank
//    pair in LDS (conflict-free ds_read_b64).  Out: two bitmaps (H & mask_s == 0, H & mask_l == 0), one u64 per lane, and
//    per wave (4 KiB) a level-1 summary of four maps: "some bit set" and "some bit clear" for each bitmap.
// 2. summary: levels 2 and 3 (256 KiB, 16 MiB), so that a search for the next candidate -- or the next non-candidate --
//    crosses a degenerate run of any length in a few loads.
// 3. resolve, on segments of S bytes (S >= M): spec walks the chain of every segment from its first byte (lane per segment);
//    merge re-walks each segment from the previous segment's exit until it lands on a cut of its own chain; fixup (one
//    wavefront) follows the true chain only where a merge failed, which happens in runs where chains keep their phase.
//    Every walk steps over runs without candidates by c += k*M and over runs where every position is a candidate by
//    c += k*m, using the summaries.  count + pack_launch (index only) + write produce d_offsets and the chunk count.
// 4. chunk sort for cw_dev_hash_chunks: a counting sort of the chunks by Threefish / SHA-256 step count (longest first), so
//    that the lanes of a wavefront hash chunks of about the same length.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cw_device.h"
#include "stream_scratch.h"

namespace cw {

namespace {

constexpr unsigned kScanThreads = 512;
constexpr uint64_t kEnd = ~0ull;

__device__ __forceinline__ uint64_t ctz64(uint64_t v) { return (uint64_t)__builtin_ctzll(v); }
__host__ __device__ __forceinline__ uint64_t umin(uint64_t a, uint64_t b) { return a < b ? a : b; }

// ---- 1. candidate scan ------------------------------------------------------------------------------------------------
// HI: both masks have a zero low word, so only the high word of H is tested.  EDGE: the wavefront's 4 KiB touch the first
// or the last bytes of the stream (bytes before d_src contribute 0 to H; positions outside [0, n) are never candidates).
// 16 bytes per iteration: granule i + 1 is loaded while granule i runs through the recurrence.
template <bool HI, bool EDGE>
__device__ __forceinline__ void scan_slice(const uint64_t *__restrict__ tab, unsigned copy, const uint8_t *__restrict__ base,
                                           uint64_t last_granule, uint64_t q0, uint64_t off, uint64_t nv, uint64_t ms, uint64_t ml,
                                           uint64_t &ws, uint64_t &wl)
{
    const uint32_t msh = (uint32_t)(ms >> 32), msl = (uint32_t)ms, mlh = (uint32_t)(ml >> 32), mll = (uint32_t)ml;
    auto granule = [&](int i) __attribute__((always_inline)) {
        const int64_t gi = (int64_t)(q0 >> 4) - 4 + i;
        const uint64_t g = gi < 0 ? 0 : ((uint64_t)gi > last_granule ? last_granule : (uint64_t)gi);
        return *reinterpret_cast<const uint4 *>(base + g * 16);
    };
    uint64_t h = 0, s = 0, l = 0;
    uint4 cur = granule(0);
#pragma unroll 1
    for (int i = 0; i < 8; i++) {
        const uint4 nxt = granule(i + 1 < 8 ? i + 1 : 7);
        const uint32_t d[4] = {cur.x, cur.y, cur.z, cur.w};
#pragma unroll
        for (int j = 0; j < 16; j++) {
            const uint32_t b = (d[j >> 2] >> (8 * (j & 3))) & 0xFF;
            uint64_t g = tab[(b << 5) | copy];
            const int pos = 16 * i + j - 64; // position within the slice (< 0: the warm-up bytes before it)
            if (EDGE && ((int64_t)q0 + pos < 0 || (uint64_t)((int64_t)q0 + pos) < off)) g = 0;
            h = (h << 1) + g;
            if (i >= 4) {
                const uint32_t hh = (uint32_t)(h >> 32), hl = (uint32_t)h;
                bool cs = (hh & msh) == 0, cl = (hh & mlh) == 0;
                if (!HI) { cs = cs && (hl & msl) == 0; cl = cl && (hl & mll) == 0; }
                if (EDGE) {
                    const uint64_t q = q0 + pos;
                    const bool in = q >= off && q < nv;
                    cs = cs && in; cl = cl && in;
                }
                s |= (uint64_t)cs << pos;
                l |= (uint64_t)cl << pos;
            }
        }
        cur = nxt;
    }
    ws = s;
    wl = l;
}

template <bool HI>
__global__ void __launch_bounds__(kScanThreads)
cdc_scan_kernel(const uint8_t *__restrict__ base, uint64_t off, uint64_t n, const uint64_t *__restrict__ gear, uint64_t ms, uint64_t ml,
                uint64_t *__restrict__ l0s, uint64_t *__restrict__ l0l, uint64_t *__restrict__ l1, uint64_t nwords, uint64_t nspans)
{
    __shared__ uint64_t tab[256 * 32]; // entry v, copy c at v * 32 + c: lane l reads copy l % 32, bank pair 2 (l % 32)
    for (unsigned i = threadIdx.x; i < 256 * 32; i += blockDim.x) tab[i] = gear[i >> 5];
    __syncthreads();
    const unsigned lane = threadIdx.x & 63, copy = threadIdx.x & 31;
    const uint64_t nv = n + off, last_granule = (nv - 1) >> 4;
    const uint64_t waves = (uint64_t)gridDim.x * (kScanThreads / 64);
    for (uint64_t span = (uint64_t)blockIdx.x * (kScanThreads / 64) + (threadIdx.x >> 6); span < nspans; span += waves) {
        // lane: the 64 positions [q0, q0 + 64), after the 64 bytes before them; granules are clamped into the stream and the
        // bytes they bring from outside it are masked (EDGE)
        const uint64_t word = span * 64 + lane, q0 = word * 64;
        const bool edge = span == 0 || (span + 1) * 4096 > nv; // wave-uniform
        uint64_t ws, wl;
        if (edge) scan_slice<HI, true>(tab, copy, base, last_granule, q0, off, nv, ms, ml, ws, wl);
        else scan_slice<HI, false>(tab, copy, base, last_granule, q0, off, nv, ms, ml, ws, wl);
        const bool have = word < nwords;
        if (have) { l0s[word] = ws; l0l[word] = wl; }
        const uint64_t b0 = __ballot(have && ws != 0), b1 = __ballot(have && wl != 0);
        const uint64_t b2 = __ballot(have && ws != ~0ull), b3 = __ballot(have && wl != ~0ull);
        if (lane == 0) {
            l1[span * 4 + 0] = b0; l1[span * 4 + 1] = b1; l1[span * 4 + 2] = b2; l1[span * 4 + 3] = b3;
        }
    }
}

// ---- 2. summaries: out entry j, map k = "some entry of in[64j .. 64j + 64) of map k is nonzero" ---------------------------
__global__ void __launch_bounds__(256)
cdc_summary_kernel(const uint64_t *__restrict__ in, uint64_t nin, uint64_t *__restrict__ out, uint64_t nout)
{
    const unsigned lane = threadIdx.x & 63;
    const uint64_t waves = (uint64_t)gridDim.x * 4;
    for (uint64_t j = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); j < nout; j += waves) {
        const uint64_t i = j * 64 + lane;
        uint64_t v[4] = {0, 0, 0, 0};
        if (i < nin) {
#pragma unroll
            for (int k = 0; k < 4; k++) v[k] = in[i * 4 + k];
        }
        uint64_t b[4];
#pragma unroll
        for (int k = 0; k < 4; k++) b[k] = __ballot(v[k] != 0);
        if (lane == 0) {
#pragma unroll
            for (int k = 0; k < 4; k++) out[j * 4 + k] = b[k];
        }
    }
}

// ---- 3. resolve ---------------------------------------------------------------------------------------------------------
struct Cdc { // few pointers: the resolve kernels keep the walk's state in scalar registers
    const uint64_t *l0; // mask_s words, then mask_l words
    const uint64_t *lv; // summaries: level 1 (n1 entries), 2 (n2), 3, four u64 per entry
    uint64_t nwords, n1, n2, off, n, seg, nseg;
    uint32_t m, a, M, cap; // cap = cuts one segment can hold
    int final_;
    uint64_t *segs; // per segment: list[cap], pre[cap], exit_spec, exit_walk, the notmerged bits, then cnt, start, precnt (u32)
    __device__ uint64_t *list(uint64_t g) const { return segs + g * cap; }
    __device__ uint64_t *pre(uint64_t g) const { return segs + (nseg + g) * cap; }
    __device__ uint64_t *exit_spec() const { return segs + 2 * nseg * cap; }
    __device__ uint64_t *exit_walk() const { return exit_spec() + nseg; }
    __device__ uint64_t *notmerged() const { return exit_spec() + 2 * nseg; }
    __device__ uint32_t *cnt() const { return reinterpret_cast<uint32_t *>(notmerged() + (nseg + 63) / 64); }
    __device__ uint32_t *start() const { return cnt() + nseg; }
    __device__ uint32_t *precnt() const { return cnt() + 2 * nseg; }
};

// map: 0 = mask_s candidates, 1 = mask_l candidates, 2 / 3 = the positions that are NOT a candidate of 0 / 1
__device__ __forceinline__ uint64_t word0(const Cdc &c, int map, uint64_t w)
{
    const uint64_t v = c.l0[(map & 1) * c.nwords + w];
    return map >= 2 ? ~v : v;
}

// first word index in [w, wlast] whose level-1 summary bit is set, else kEnd
__device__ uint64_t next_word(const Cdc &c, int map, uint64_t w, uint64_t wlast)
{
    for (;;) {
        if (w > wlast) return kEnd;
        const uint64_t i1 = w >> 6;
        const uint64_t b1 = c.lv[i1 * 4 + map] & (~0ull << (w & 63));
        if (b1) { const uint64_t r = (i1 << 6) + ctz64(b1); return r <= wlast ? r : kEnd; }
        const uint64_t j = i1 + 1; // level-1 entry
        if ((j << 6) > wlast) return kEnd;
        const uint64_t b2 = c.lv[(c.n1 + (j >> 6)) * 4 + map] & (~0ull << (j & 63));
        if (b2) { w = (((j >> 6) << 6) + ctz64(b2)) << 6; continue; }
        uint64_t k = (j >> 6) + 1; // level-2 entry
        for (;;) {
            if ((k << 12) > wlast) return kEnd;
            const uint64_t b3 = c.lv[(c.n1 + c.n2 + (k >> 6)) * 4 + map] & (~0ull << (k & 63));
            if (b3) { w = (((k >> 6) << 6) + ctz64(b3)) << 12; break; }
            k = ((k >> 6) + 1) << 6;
        }
    }
}

// first real position p in [lo, hi) whose bit is set in `map`, else hi
__device__ uint64_t first_bit(const Cdc &c, int map, uint64_t lo, uint64_t hi)
{
    if (lo >= hi) return hi;
    const uint64_t q = lo + c.off, qhi = hi + c.off;
    uint64_t w = q >> 6;
    uint64_t b = word0(c, map, w) & (~0ull << (q & 63));
    if (!b) {
        w = next_word(c, map, w + 1, (qhi - 1) >> 6);
        if (w == kEnd) return hi;
        b = word0(c, map, w);
    }
    const uint64_t p = (w << 6) + ctz64(b);
    return p < qhi ? p - c.off : hi;
}

__device__ __forceinline__ bool terminal(const Cdc &c, uint64_t cut) { return c.final_ ? cut == c.n : cut + c.M > c.n; }

// From a non-terminal cut: the next cuts are cut + stride * i, i = 1..k.  k > 1 only across a run without candidates
// (stride M) or a run where every position is a candidate (stride m), and then only while every start leaves M bytes;
// k stops at the first cut >= bound.
struct Step { uint64_t stride, k; };
__device__ Step cdc_step(const Cdc &c, uint64_t cut, uint64_t bound)
{
    const uint64_t n = c.n, r = n - cut, m = c.m, M = c.M;
    if (r <= m) return {r, 1};
    const uint64_t kb = bound > cut ? (bound - cut + m - 1) / m : 1; // m-steps to reach the bound (an upper bound for M-steps too)
    const bool room = cut + M <= n;
    if (room && m == M) { // every chunk has size M
        const uint64_t k = umin((n - cut) / M, umin((bound > cut ? (bound - cut + M - 1) / M : 1), kb));
        return {M, k ? k : 1};
    }
    const uint64_t e = cut + umin(M, r), z = cut + umin(c.a, r);
    const uint64_t lim = umin(n, (bound > cut ? bound : cut) + M);
    // the searches run one after the other through ONE inlined first_bit (it is large): 0 = mask_s range, 1 = mask_l range,
    // 2 / 3 = the next candidates of either kind past cut + M - 1, 4 = the next non-candidate
    uint64_t x = e, q = lim;
    int phase = 0, map = 0;
    uint64_t lo = cut + m - 1, hi = z - 1;
    for (;;) {
        const uint64_t p = first_bit(c, map, lo, hi);
        if (phase == 0) {
            if (p < hi) x = p + 1;
            else { phase = 1; map = 1; lo = z - 1; hi = e - 1; continue; }
        } else if (phase == 1) {
            x = p < hi ? p + 1 : e;
        } else if (phase == 2) {
            q = p; phase = 3; map = 1; continue;
        } else if (phase == 3) {
            q = umin(q, p); // no candidate in [cut + m - 1, q): how many M-steps see none
            uint64_t k = (q + 1 - cut) / M;
            k = umin(k, (n - cut) / M);
            k = umin(k, bound > cut ? (bound - cut + M - 1) / M : 1);
            return {M, k ? k : 1};
        } else { // phase 4: every position in [cut + m - 1, p) is a candidate: how many m-steps in a row find one
            uint64_t k = (p - cut) / m;
            k = umin(k, (n - M - cut) / m + 1);
            k = umin(k, kb);
            return {m, k ? k : 1};
        }
        // x is the next cut
        if (!room) return {x - cut, 1};
        if (x == cut + M) { phase = 2; map = 0; lo = cut + M - 1; hi = lim; continue; }
        if (x == cut + m) { phase = 4; map = m < c.a ? 2 : 3; lo = cut + m - 1; hi = lim; continue; }
        return {x - cut, 1};
    }
}

// spec: the chain of segment g from g * S (cuts in [gS, (g+1)S) into list, the first cut >= (g+1)S into exit_spec, kEnd if the
// chain ends first)
__global__ void __launch_bounds__(64)
cdc_spec_kernel(Cdc c, uint64_t nseg)
{
    const uint64_t g = (uint64_t)blockIdx.x * 64 + threadIdx.x;
    if (g >= nseg) return;
    uint64_t *list = c.list(g);
    const uint64_t bound = (g + 1) * c.seg;
    uint64_t cut = g * c.seg;
    uint32_t k = 0;
    list[k++] = cut;
    uint64_t ex = kEnd;
    while (!terminal(c, cut)) {
        const Step s = cdc_step(c, cut, bound);
        uint64_t i = 1;
        for (; i <= s.k; i++) {
            const uint64_t nc = cut + s.stride * i;
            if (nc >= bound) break;
            list[k++] = nc;
        }
        if (i <= s.k) { ex = cut + s.stride * i; break; }
        cut += s.stride * s.k;
    }
    c.cnt()[g] = k;
    c.exit_spec()[g] = ex;
}

// Walks from `cut` (a true cut in segment g) until it lands on a cut of segment g's own chain (merged: start = its index) or
// leaves the segment.  The cuts before the landing go to pre.  Returns true when merged; *ex = the exit of the walked chain.
__device__ bool walk_segment(const Cdc &c, uint64_t g, uint64_t cut, uint32_t *pcount, uint64_t *ex)
{
    const uint64_t *list = c.list(g);
    uint64_t *pre = c.pre(g);
    const uint32_t cnt = c.cnt()[g];
    const uint64_t bound = (g + 1) * c.seg;
    uint32_t j = 0, P = 0;
    for (;;) {
        // cut is a true cut inside segment g
        while (j < cnt && list[j] < cut) j++;
        if (j < cnt && list[j] == cut) {
            c.start()[g] = j; c.precnt()[g] = P; *pcount = P; *ex = c.exit_spec()[g];
            return true;
        }
        pre[P++] = cut;
        if (terminal(c, cut)) break;
        const Step s = cdc_step(c, cut, bound);
        uint64_t i = 1;
        for (; i < s.k; i++) { // the progression's inner cuts: each may land on the chain too
            const uint64_t nc = cut + s.stride * i;
            while (j < cnt && list[j] < nc) j++;
            if (j < cnt && list[j] == nc) break;
            pre[P++] = nc;
        }
        cut += s.stride * i;
        if (cut >= bound) { c.start()[g] = cnt; c.precnt()[g] = P; *pcount = P; *ex = cut; return false; }
    }
    c.start()[g] = cnt; c.precnt()[g] = P; *pcount = P; *ex = kEnd;
    return false;
}

// merge: segment g walked from the spec exit of segment g - 1
__global__ void __launch_bounds__(64)
cdc_merge_kernel(Cdc c, uint64_t nseg)
{
    const uint64_t g = (uint64_t)blockIdx.x * 64 + threadIdx.x;
    if (g >= nseg) return;
    if (g == 0) { c.start()[0] = 0; c.precnt()[0] = 0; c.exit_walk()[0] = c.exit_spec()[0]; return; }
    const uint64_t entry = c.exit_spec()[g - 1];
    if (entry == kEnd) { c.start()[g] = c.cnt()[g]; c.precnt()[g] = 0; c.exit_walk()[g] = kEnd; return; }
    uint32_t P;
    uint64_t ex;
    if (!walk_segment(c, g, entry, &P, &ex)) atomicOr(reinterpret_cast<unsigned long long *>(c.notmerged() + (g >> 6)), 1ull << (g & 63));
    c.exit_walk()[g] = ex;
}

// the progression t + stride * i, 1 <= i < k: the index of its first cut in segment h (every later segment starts past t), and its
// number of cuts in h
__device__ __forceinline__ uint64_t prog_lo(const Cdc &c, uint64_t t, uint64_t stride, uint64_t h)
{
    const uint64_t s = h * c.seg;
    return s <= t ? 1 : (s - t + stride - 1) / stride; // >= 1
}
__device__ __forceinline__ uint64_t prog_count(const Cdc &c, uint64_t t, uint64_t stride, uint64_t k, uint64_t h)
{
    const uint64_t lo = prog_lo(c, t, stride, h), hi = umin(k, prog_lo(c, t, stride, h + 1));
    return hi > lo ? hi - lo : 0;
}

// fixup (one wavefront): follows the true chain wherever a segment's merge walk did not land on its own chain.  The walk is
// not bounded by segments: across a run without candidates (or of all candidates) cdc_step returns the whole run as one
// progression, whose cuts the lanes write into the lists of the segments it covers, so a run of any length costs one step
// and a lane-parallel fill.  The segments past the end of the chain are emptied lane-parallel.
__global__ void __launch_bounds__(64)
cdc_fixup_kernel(Cdc params, uint64_t nseg)
{
    // The walk's parameters are read from LDS: there is no scalar LDS read, so they live in vector registers and the scalar
    // file keeps the walk's control state (with the parameters in scalar registers the kernel needs more than it has).
    __shared__ Cdc shared_params;
    const unsigned lane = threadIdx.x;
    if (lane == 0) shared_params = params;
    __syncthreads();
    const Cdc &c = shared_params;
    const uint64_t nbits = (nseg + 63) / 64;
    uint64_t g = 1;
    for (;;) {
        // the next segment >= g whose merge walk failed
        uint64_t g0 = kEnd;
        for (uint64_t w = g >> 6; w < nbits && g0 == kEnd; w += 64) {
            const uint64_t i = w + lane;
            uint64_t v = i < nbits ? c.notmerged()[i] : 0;
            if (i == (g >> 6)) v &= ~0ull << (g & 63);
            const uint64_t b = __ballot(v != 0);
            if (b) {
                const unsigned src = (unsigned)ctz64(b);
                g0 = ((w + src) << 6) + ctz64(__shfl(v, src, 64));
            }
        }
        if (g0 == kEnd || g0 + 1 >= nseg) return;
        uint64_t t = c.exit_walk()[g0];
        if (t == c.exit_spec()[g0]) { g = g0 + 1; continue; } // the next segment's merge walk started where the true chain enters
        // walk the true chain from t until it lands on a segment's own chain; h = the segment of t, P = cuts already in its pre
        uint64_t h = t == kEnd ? g0 : t / c.seg;
        uint32_t P = 0, j = 0;
        for (;;) {
            if (t == kEnd) {
                for (uint64_t e = h + 1 + lane; e < nseg; e += 64) { c.precnt()[e] = 0; c.start()[e] = c.cnt()[e]; }
                return;
            }
            const uint64_t *list = c.list(h);
            const uint32_t cnt = c.cnt()[h];
            while (j < cnt && list[j] < t) j++;
            if (j < cnt && list[j] == t) { // landed: from here segment h's own chain is the true one
                if (lane == 0) { c.start()[h] = j; c.precnt()[h] = P; }
                g = h + 1;
                break;
            }
            if (lane == 0) c.pre(h)[P] = t;
            P++;
            if (terminal(c, t)) {
                if (lane == 0) { c.start()[h] = cnt; c.precnt()[h] = P; }
                t = kEnd;
                continue;
            }
            const Step st = cdc_step(c, t, c.n);
            const uint64_t nt = t + st.stride * st.k, hn = nt / c.seg;
            if (st.k > 1) {
                for (uint64_t i = 1 + lane; i < st.k; i += 64) {
                    const uint64_t q = t + st.stride * i, hq = q / c.seg;
                    c.pre(hq)[(hq == h ? P : 0) + (i - prog_lo(c, t, st.stride, hq))] = q;
                }
            }
            if (hn == h) {
                P += (uint32_t)(st.k - 1);
            } else {
                if (lane == 0) { c.start()[h] = cnt; c.precnt()[h] = P + (uint32_t)prog_count(c, t, st.stride, st.k, h); }
                for (uint64_t e = h + 1 + lane; e < hn; e += 64) {
                    c.start()[e] = c.cnt()[e];
                    c.precnt()[e] = (uint32_t)prog_count(c, t, st.stride, st.k, e);
                }
                P = (uint32_t)prog_count(c, t, st.stride, st.k, hn);
                j = 0;
                h = hn;
            }
            t = nt;
        }
        if (g >= nseg) return;
    }
}

__global__ void __launch_bounds__(256)
cdc_count_kernel(Cdc c, uint64_t nseg, uint32_t *__restrict__ counts)
{
    const uint64_t g = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (g < nseg) counts[g] = c.precnt()[g] + (c.cnt()[g] - c.start()[g]);
}

__global__ void __launch_bounds__(64)
cdc_write_kernel(Cdc c, uint64_t nseg, const uint64_t *__restrict__ segoff, uint64_t *__restrict__ out, uint64_t max_out,
                 uint64_t *__restrict__ nchunks)
{
    const uint64_t g = blockIdx.x;
    const unsigned lane = threadIdx.x;
    const uint64_t base = segoff[g];
    const uint32_t P = c.precnt()[g], s = c.start()[g], k = c.cnt()[g];
    const uint64_t *pre = c.pre(g), *list = c.list(g);
    // the chain has at most nbytes / min_size + 2 cuts, which the host checked max_out against; the bound is kept anyway
    for (uint32_t i = lane; i < P; i += 64) if (base + i < max_out) out[base + i] = pre[i];
    for (uint32_t i = s + lane; i < k; i += 64) if (base + P + (i - s) < max_out) out[base + P + (i - s)] = list[i];
    if (g == 0 && lane == 0) *nchunks = segoff[nseg] - 1;
}

// ---- 4. chunk sort by step count (longest first) ----------------------------------------------------------------------
constexpr unsigned kBuckets = 4096;

__device__ __forceinline__ uint32_t chunk_key(const uint64_t *offsets, uint64_t i, uint64_t src_bytes, unsigned step_shift)
{
    uint64_t s = offsets[i], e = offsets[i + 1];
    s = umin(s, src_bytes); e = umin(e, src_bytes);
    const uint64_t len = e > s ? e - s : 0;
    const uint64_t steps = umin(len >> step_shift, kBuckets - 1);
    return (uint32_t)(kBuckets - 1 - steps);
}

__global__ void __launch_bounds__(256)
chunk_hist_kernel(const uint64_t *__restrict__ offsets, const uint64_t *__restrict__ d_n, uint64_t max_chunks, uint64_t src_bytes,
                  unsigned step_shift, uint32_t *__restrict__ hist)
{
    const uint64_t k = umin(*d_n, max_chunks);
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < k; i += (uint64_t)gridDim.x * 256)
        atomicAdd(&hist[chunk_key(offsets, i, src_bytes, step_shift)], 1u);
}

// one workgroup: exclusive scan of the kBuckets counts in place
__global__ void __launch_bounds__(1024)
chunk_scan_kernel(uint32_t *__restrict__ hist)
{
    __shared__ uint32_t part[1024];
    constexpr unsigned per = kBuckets / 1024;
    uint32_t v[per], s = 0;
#pragma unroll
    for (unsigned k = 0; k < per; k++) { v[k] = hist[threadIdx.x * per + k]; s += v[k]; }
    part[threadIdx.x] = s;
    __syncthreads();
    for (unsigned d = 1; d < 1024; d <<= 1) {
        const uint32_t add = threadIdx.x >= d ? part[threadIdx.x - d] : 0;
        __syncthreads();
        part[threadIdx.x] += add;
        __syncthreads();
    }
    uint32_t o = part[threadIdx.x] - s;
#pragma unroll
    for (unsigned k = 0; k < per; k++) { hist[threadIdx.x * per + k] = o; o += v[k]; }
}

__global__ void __launch_bounds__(256)
chunk_scatter_kernel(const uint64_t *__restrict__ offsets, const uint64_t *__restrict__ d_n, uint64_t max_chunks, uint64_t src_bytes,
                     unsigned step_shift, uint32_t *__restrict__ cursor, uint32_t *__restrict__ perm)
{
    const uint64_t k = umin(*d_n, max_chunks);
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < k; i += (uint64_t)gridDim.x * 256)
        perm[atomicAdd(&cursor[chunk_key(offsets, i, src_bytes, step_shift)], 1u)] = (uint32_t)i;
}

// ---- per-stream workspace -----------------------------------------------------------------------------------------------
// two registries: chunk_hash_launch holds its entry's launch lock while the hash it calls queues on the same stream
StreamScratch<DeviceBuf> scan_space, sort_space;
constexpr size_t kFloor = (size_t)1 << 20;

size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }

} // namespace

uint64_t cdc_segment_bytes(uint32_t max_size, long knob)
{
    uint64_t s = knob > 0 ? (uint64_t)knob : ((uint64_t)256 << 10);
    if (s < max_size) s = max_size;
    if (knob <= 0) s = (s + max_size - 1) / max_size * max_size; // in phase with every segment start in a run of M-steps
    return s;
}

size_t cdc_workspace_bytes(size_t nbytes, uint32_t min_size, uint64_t seg)
{
    const uint64_t nv = nbytes + 15, nwords = (nv + 63) / 64, n1 = (nwords + 63) / 64, n2 = (n1 + 63) / 64, n3 = (n2 + 63) / 64;
    const uint64_t nseg = nbytes / seg + 1, cap = seg / min_size + 2;
    return 2048 + up256(2 * nwords * 8) + up256(4 * 8 * (n1 + n2 + n3)) +
           up256(2 * nseg * cap * 8 + 2 * nseg * 8 + (nseg + 63) / 64 * 8 + 3 * nseg * 4) + up256(nseg * 4) + up256((nseg + 1) * 8);
}

hipError_t cdc_launch(const CdcParams &p, const uint8_t *src, size_t nbytes, int final_, uint64_t *offsets, size_t max_offsets,
                      uint64_t *nchunks, uint64_t seg, hipStream_t stream)
{
    if (nbytes == 0) {
        hipError_t e = hipMemsetAsync(offsets, 0, sizeof(uint64_t), stream);
        return e != hipSuccess ? e : hipMemsetAsync(nchunks, 0, sizeof(uint64_t), stream);
    }
    const uint64_t off = reinterpret_cast<uintptr_t>(src) & 15;
    const uint8_t *base = src - off;
    const uint64_t nv = nbytes + off, nwords = (nv + 63) / 64, n1 = (nwords + 63) / 64, n2 = (n1 + 63) / 64, n3 = (n2 + 63) / 64;
    const uint64_t nseg = nbytes / seg + 1, cap = seg / p.min_size + 2;
    auto &space = scan_space.at(stream);
    LaunchLock sequence(space.launch); // the scratch is shared by the launches below
    hipError_t e = space.reserve(cdc_workspace_bytes(nbytes, p.min_size, seg), kFloor);
    if (e != hipSuccess) return e;
    uint8_t *w = space.as<uint8_t>();
    auto take = [&](size_t bytes) { uint8_t *r = w; w += up256(bytes); return r; };
    uint64_t *gear = reinterpret_cast<uint64_t *>(take(2048));
    uint64_t *l0 = reinterpret_cast<uint64_t *>(take(2 * nwords * 8));
    uint64_t *lv = reinterpret_cast<uint64_t *>(take(4 * 8 * (n1 + n2 + n3)));
    uint64_t *segs = reinterpret_cast<uint64_t *>(take(2 * nseg * cap * 8 + 2 * nseg * 8 + (nseg + 63) / 64 * 8 + 3 * nseg * 4));
    uint64_t *notmerged = segs + 2 * nseg * cap + 2 * nseg;
    uint32_t *counts = reinterpret_cast<uint32_t *>(take(nseg * 4));
    uint64_t *segoff = reinterpret_cast<uint64_t *>(take((nseg + 1) * 8));

    e = hipMemcpyAsync(gear, p.gear, 2048, hipMemcpyHostToDevice, stream);
    if (e == hipSuccess) e = hipMemsetAsync(notmerged, 0, (nseg + 63) / 64 * 8, stream);
    if (e != hipSuccess) return e;
    const bool hi = (uint32_t)p.mask_s == 0 && (uint32_t)p.mask_l == 0;
    // 8 wavefronts per workgroup, one span each; 2 workgroups per CU (64 KiB of LDS tables each), grid-stride beyond 512
    const unsigned scan_grid = (unsigned)(n1 < 4096 ? (n1 + 7) / 8 : 512);
    if (hi) hipLaunchKernelGGL((cdc_scan_kernel<true>), dim3(scan_grid), dim3(kScanThreads), 0, stream, base, off, (uint64_t)nbytes, gear,
                               p.mask_s, p.mask_l, l0, l0 + nwords, lv, nwords, n1);
    else hipLaunchKernelGGL((cdc_scan_kernel<false>), dim3(scan_grid), dim3(kScanThreads), 0, stream, base, off, (uint64_t)nbytes, gear,
                            p.mask_s, p.mask_l, l0, l0 + nwords, lv, nwords, n1);
    uint64_t *l1 = lv, *l2 = lv + 4 * n1, *l3 = lv + 4 * (n1 + n2);
    hipLaunchKernelGGL(cdc_summary_kernel, dim3((unsigned)umin((n2 + 3) / 4, 1024)), dim3(256), 0, stream, l1, n1, l2, n2);
    hipLaunchKernelGGL(cdc_summary_kernel, dim3((unsigned)umin((n3 + 3) / 4, 1024)), dim3(256), 0, stream, l2, n2, l3, n3);

    Cdc c;
    c.l0 = l0; c.lv = lv;
    c.nwords = nwords; c.n1 = n1; c.n2 = n2; c.off = off; c.n = nbytes; c.seg = seg; c.nseg = nseg;
    c.m = p.min_size; c.a = p.normal_size; c.M = p.max_size; c.cap = (uint32_t)cap; c.final_ = final_;
    c.segs = segs;
    const unsigned sg = (unsigned)((nseg + 63) / 64);
    hipLaunchKernelGGL(cdc_spec_kernel, dim3(sg), dim3(64), 0, stream, c, nseg);
    hipLaunchKernelGGL(cdc_merge_kernel, dim3(sg), dim3(64), 0, stream, c, nseg);
    hipLaunchKernelGGL(cdc_fixup_kernel, dim3(1), dim3(64), 0, stream, c, nseg);
    hipLaunchKernelGGL(cdc_count_kernel, dim3((unsigned)((nseg + 255) / 256)), dim3(256), 0, stream, c, nseg, counts);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    e = pack_launch(nullptr, 0, counts, nseg, nullptr, segoff, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(cdc_write_kernel, dim3((unsigned)nseg), dim3(64), 0, stream, c, nseg, segoff, offsets, (uint64_t)max_offsets, nchunks);
    note_kernels(1, "cw::cdc_scan_kernel, cw::cdc_spec_kernel, cw::cdc_merge_kernel, cw::cdc_fixup_kernel");
    return hipGetLastError();
}

hipError_t chunk_hash_launch(const uint64_t *offsets, const uint64_t *d_n, size_t max_chunks, size_t src_bytes, unsigned step_shift,
                             const ChunkHash &hash, hipStream_t stream)
{
    auto &space = sort_space.at(stream);
    // the sort and the hash that reads its permutation are queued under one lock: another thread's call on the same stream
    // cannot rewrite (or reallocate) the permutation in between
    LaunchLock sequence(space.launch);
    hipError_t e = space.reserve(kBuckets * 4 + max_chunks * 4, kFloor);
    if (e != hipSuccess) return e;
    uint32_t *hist = space.as<uint32_t>(), *perm = hist + kBuckets;
    e = hipMemsetAsync(hist, 0, kBuckets * 4, stream);
    if (e != hipSuccess) return e;
    const unsigned grid = (unsigned)umin((max_chunks + 255) / 256, 2048);
    hipLaunchKernelGGL(chunk_hist_kernel, dim3(grid), dim3(256), 0, stream, offsets, d_n, (uint64_t)max_chunks, (uint64_t)src_bytes,
                       step_shift, hist);
    hipLaunchKernelGGL(chunk_scan_kernel, dim3(1), dim3(1024), 0, stream, hist);
    hipLaunchKernelGGL(chunk_scatter_kernel, dim3(grid), dim3(256), 0, stream, offsets, d_n, (uint64_t)max_chunks, (uint64_t)src_bytes,
                       step_shift, hist, perm);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    return hash.fn(hash.ctx, perm);
}

} // namespace cw
