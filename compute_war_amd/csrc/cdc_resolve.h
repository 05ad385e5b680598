// cdc_resolve.h -- the cut resolve of content-defined chunking (DESIGN.md sections 11 and 19), shared by its two forms: one stream
// (cdc_kernels.hip instantiates the kernels over Cdc) and many streams in one buffer (cdc_streams_kernels.hip, over CdcS).  What differs
// between them is decided at compile time (C::kStreams): the single-stream kernels carry no trace of the stream form.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cw_device.h"

namespace cw {

struct Cdc { // few pointers: the resolve kernels keep the walk's state in scalar registers
    const uint64_t *l0; // mask_s words, then mask_l words
    const uint64_t *lv; // summaries: level 1 (n1 entries), 2 (n2), 3, four u64 per entry
    uint64_t nwords, n1, n2, off, n, seg, nseg;
    uint32_t m, a, M, cap; // cap = cuts one segment can hold
    int final_;
    static constexpr bool kStreams = false;
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

// The stream form: d_ends[nstreams] (validated: non-decreasing, last = n), eidx[g] = the number of ends below g * seg for g <= nseg,
// so the ends inside segment g are ends[eidx[g] .. eidx[g + 1]) and its lists start cap * g + eidx[g] entries in: a list of segment g
// holds cap + eidx[g + 1] - eidx[g] cuts (a cut that is no stream end lies min_size behind the cut before it).
struct CdcS : Cdc {
    const uint64_t *ends;
    const uint32_t *eidx;
    const uint64_t *verdict; // != 0: d_ends was refused, the resolve touches nothing
    uint64_t nstreams;
    static constexpr bool kStreams = true;
    __device__ uint64_t total() const { return nseg * cap + nstreams; }
    __device__ uint64_t *list(uint64_t g) const { return segs + g * cap + eidx[g]; }
    __device__ uint64_t *pre(uint64_t g) const { return segs + total() + g * cap + eidx[g]; }
    __device__ uint64_t *exit_spec() const { return segs + 2 * total(); }
    // (stated again: Cdc's would build on Cdc's exit_spec)
    __device__ uint64_t *exit_walk() const { return exit_spec() + nseg; }
    __device__ uint64_t *notmerged() const { return exit_spec() + 2 * nseg; }
    __device__ uint32_t *cnt() const { return reinterpret_cast<uint32_t *>(notmerged() + (nseg + 63) / 64); }
    __device__ uint32_t *start() const { return cnt() + nseg; }
    __device__ uint32_t *precnt() const { return cnt() + 2 * nseg; }
};

// the stream form's launches (cdc_streams_kernels.hip), queued by cdc_kernels.hip's launch under the workspace's lock, in this order
// around the scan: the verdict on d_ends, then (refused, or nbytes == 0) the empty result, else eidx
hipError_t cdc_streams_verdict_launch(const CdcStreams &st, size_t nbytes, uint64_t seg, uint64_t nseg, uint32_t *eidx, uint64_t *offsets,
                                      uint64_t *nchunks, hipStream_t stream);
// spec, merge, fixup, count
hipError_t cdc_streams_resolve_launch(const CdcS &c, uint32_t *counts, hipStream_t stream);
// write, then d_stream_first
hipError_t cdc_streams_write_launch(const CdcS &c, const CdcStreams &st, const uint64_t *segoff, uint64_t *offsets, size_t max_offsets,
                                    uint64_t *nchunks, hipStream_t stream);

namespace {

constexpr uint64_t kEnd = ~0ull;

__device__ __forceinline__ uint64_t ctz64(uint64_t v) { return (uint64_t)__builtin_ctzll(v); }
__host__ __device__ __forceinline__ uint64_t umin(uint64_t a, uint64_t b) { return a < b ? a : b; }

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

// Where a chain stops.  One stream: at n (final), else at the first cut that leaves less than max_size.  Streams: the complete ones are
// chunked to their ends whatever is left behind them, so only a cut at or behind the start of the last stream can stop short of n, and
// only when that stream is open (final_ == 0: cw_dev_cdc_streams_part).  The start is read where a cut first leaves less than max_size.
template <class C> __device__ __forceinline__ bool terminal(const C &c, uint64_t cut)
{
    if constexpr (!C::kStreams) {
        return c.final_ ? cut == c.n : cut + c.M > c.n;
    } else {
        if (cut + c.M <= c.n) return false;
        return c.final_ ? cut == c.n : cut >= (c.nstreams > 1 ? c.ends[c.nstreams - 2] : 0);
    }
}

// the end a step from the non-terminal `cut` sees: the stream's, or (streams) the smallest end above cut, which lies among the ends of
// cut's segment or is the first one behind them; the last end is n > cut
template <class C> __device__ __forceinline__ uint64_t end_above(const C &c, uint64_t cut)
{
    if constexpr (!C::kStreams) {
        return c.n;
    } else {
        const uint64_t g = umin(cut / c.seg, c.nseg - 1);
        uint64_t lo = c.eidx[g], hi = umin(c.eidx[g + 1], c.nstreams - 1);
        while (lo < hi) {
            const uint64_t mid = lo + (hi - lo) / 2;
            if (c.ends[mid] > cut) hi = mid; else lo = mid + 1;
        }
        return c.ends[umin(lo, c.nstreams - 1)];
    }
}

// From a non-terminal cut: the next cuts are cut + stride * i, i = 1..k.  k > 1 only across a run without candidates
// (stride M) or a run where every position is a candidate (stride m), and then only while every start leaves M bytes;
// k stops at the first cut >= bound.
struct Step { uint64_t stride, k; };
template <class C> __device__ Step cdc_step(const C &c, uint64_t cut, uint64_t bound)
{
    const uint64_t n = end_above(c, cut), r = n - cut, m = c.m, M = c.M;
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
template <class C> __global__ void __launch_bounds__(64)
cdc_spec_kernel(C c, uint64_t nseg)
{
    if constexpr (C::kStreams) { if (*c.verdict) return; }
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
template <class C> __device__ bool walk_segment(const C &c, uint64_t g, uint64_t cut, uint32_t *pcount, uint64_t *ex)
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
template <class C> __global__ void __launch_bounds__(64)
cdc_merge_kernel(C params, uint64_t nseg)
{
    // (streams: the parameters are read from LDS, as in the fixup and for its reason: with eight more scalar registers of arguments
    // the walk's control state would spill)
    const C *pc = &params;
    if constexpr (C::kStreams) {
        if (*params.verdict) return;
        __shared__ C shared_params;
        if (threadIdx.x == 0) shared_params = params;
        __syncthreads();
        pc = &shared_params;
    }
    const C &c = *pc;
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
template <class C> __global__ void __launch_bounds__(64)
cdc_fixup_kernel(C params, uint64_t nseg)
{
    if constexpr (C::kStreams) { if (*params.verdict) return; }
    // The walk's parameters are read from LDS: there is no scalar LDS read, so they live in vector registers and the scalar
    // file keeps the walk's control state (with the parameters in scalar registers the kernel needs more than it has).
    __shared__ C shared_params;
    const unsigned lane = threadIdx.x;
    if (lane == 0) shared_params = params;
    __syncthreads();
    const C &c = shared_params;
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

template <class C> __global__ void __launch_bounds__(256)
cdc_count_kernel(C c, uint64_t nseg, uint32_t *__restrict__ counts)
{
    const uint64_t g = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if constexpr (C::kStreams) { if (*c.verdict) { if (g < nseg) counts[g] = 0; return; } }
    if (g < nseg) counts[g] = c.precnt()[g] + (c.cnt()[g] - c.start()[g]);
}

template <class C> __global__ void __launch_bounds__(64)
cdc_write_kernel(C c, uint64_t nseg, const uint64_t *__restrict__ segoff, uint64_t *__restrict__ out, uint64_t max_out,
                 uint64_t *__restrict__ nchunks)
{
    if constexpr (C::kStreams) { if (*c.verdict) return; }
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

} // namespace
} // namespace cw
