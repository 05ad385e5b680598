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
//    The resolve's code is cdc_resolve.h; its other instantiation, over many streams in one buffer (cw_dev_cdc_streams), and that
//    form's own kernels are cdc_streams_kernels.hip.  The launch below serves both: the workspace and the scan are the same.
// 4. chunk sort for cw_dev_hash_chunks: a counting sort of the chunks by Threefish / SHA-256 step count (longest first), so
//    that the lanes of a wavefront hash chunks of about the same length.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cdc_resolve.h"
#include "cw_device.h"
#include "stream_scratch.h"

namespace cw {

namespace {

constexpr unsigned kScanThreads = 512;

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

// ---- 3. resolve: cdc_resolve.h (instantiated over Cdc by the launch below) ----------------------------------------------------

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

// the stream form's lists hold nstreams more cuts in all (each end lies in one segment), twice; eidx is u32[nseg + 1]
size_t cdc_streams_workspace_bytes(size_t nbytes, size_t nstreams, uint32_t min_size, uint64_t seg)
{
    const uint64_t nseg = nbytes / seg + 1;
    return cdc_workspace_bytes(nbytes, min_size, seg) + up256(2 * nstreams * 8) + up256((nseg + 1) * 4);
}

namespace {
// the launches of both forms: st == nullptr is cw_dev_cdc, else final_ is st's and nbytes > 0
hipError_t cdc_launch_any(const CdcParams &p, const uint8_t *src, size_t nbytes, int final_, uint64_t *offsets, size_t max_offsets,
                          uint64_t *nchunks, uint64_t seg, const CdcStreams *st, hipStream_t stream)
{
    const uint64_t off = reinterpret_cast<uintptr_t>(src) & 15;
    const uint8_t *base = src - off;
    const uint64_t nv = nbytes + off, nwords = (nv + 63) / 64, n1 = (nwords + 63) / 64, n2 = (n1 + 63) / 64, n3 = (n2 + 63) / 64;
    const uint64_t nseg = nbytes / seg + 1, cap = seg / p.min_size + 2;
    auto &space = scan_space.at(stream);
    LaunchLock sequence(space.launch); // the scratch is shared by the launches below
    const size_t nstreams = st ? st->nstreams : 0;
    hipError_t e = space.reserve(st ? cdc_streams_workspace_bytes(nbytes, nstreams, p.min_size, seg) : cdc_workspace_bytes(nbytes, p.min_size, seg), kFloor);
    if (e != hipSuccess) return e;
    uint8_t *w = space.as<uint8_t>();
    auto take = [&](size_t bytes) { uint8_t *r = w; w += up256(bytes); return r; };
    uint64_t *gear = reinterpret_cast<uint64_t *>(take(2048));
    uint64_t *l0 = reinterpret_cast<uint64_t *>(take(2 * nwords * 8));
    uint64_t *lv = reinterpret_cast<uint64_t *>(take(4 * 8 * (n1 + n2 + n3)));
    const uint64_t cuts = nseg * cap + nstreams; // the entries of all lists (and of all pres)
    uint64_t *segs = reinterpret_cast<uint64_t *>(take(2 * cuts * 8 + 2 * nseg * 8 + (nseg + 63) / 64 * 8 + 3 * nseg * 4));
    uint64_t *notmerged = segs + 2 * cuts + 2 * nseg;
    uint32_t *counts = reinterpret_cast<uint32_t *>(take(nseg * 4));
    uint64_t *segoff = reinterpret_cast<uint64_t *>(take((nseg + 1) * 8));
    uint32_t *eidx = st ? reinterpret_cast<uint32_t *>(take((nseg + 1) * 4)) : nullptr;

    e = hipMemcpyAsync(gear, p.gear, 2048, hipMemcpyHostToDevice, stream);
    if (e == hipSuccess) e = hipMemsetAsync(notmerged, 0, (nseg + 63) / 64 * 8, stream);
    if (e != hipSuccess) return e;
    if (st) { // the verdict comes first; behind it either the empty result or eidx
        if ((e = cdc_streams_verdict_launch(*st, nbytes, seg, nseg, eidx, offsets, nchunks, stream)) != hipSuccess) return e;
    }
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

    CdcS c; // (the single-stream kernels take its Cdc part)
    c.l0 = l0; c.lv = lv;
    c.nwords = nwords; c.n1 = n1; c.n2 = n2; c.off = off; c.n = nbytes; c.seg = seg; c.nseg = nseg;
    c.m = p.min_size; c.a = p.normal_size; c.M = p.max_size; c.cap = (uint32_t)cap; c.final_ = final_;
    c.segs = segs;
    const unsigned sg = (unsigned)((nseg + 63) / 64), cg = (unsigned)((nseg + 255) / 256);
    if (st) {
        c.ends = st->ends; c.eidx = eidx; c.verdict = st->result; c.nstreams = nstreams;
        if ((e = cdc_streams_resolve_launch(c, counts, stream)) != hipSuccess) return e;
    } else {
        const Cdc &c1 = c;
        hipLaunchKernelGGL(cdc_spec_kernel<Cdc>, dim3(sg), dim3(64), 0, stream, c1, nseg);
        hipLaunchKernelGGL(cdc_merge_kernel<Cdc>, dim3(sg), dim3(64), 0, stream, c1, nseg);
        hipLaunchKernelGGL(cdc_fixup_kernel<Cdc>, dim3(1), dim3(64), 0, stream, c1, nseg);
        hipLaunchKernelGGL(cdc_count_kernel<Cdc>, dim3(cg), dim3(256), 0, stream, c1, nseg, counts);
    }
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    e = pack_launch(nullptr, 0, counts, nseg, nullptr, segoff, stream);
    if (e != hipSuccess) return e;
    if (st) {
        return cdc_streams_write_launch(c, *st, segoff, offsets, max_offsets, nchunks, stream);
    } else {
        hipLaunchKernelGGL(cdc_write_kernel<Cdc>, dim3((unsigned)nseg), dim3(64), 0, stream, static_cast<const Cdc &>(c), nseg, segoff, offsets,
                           (uint64_t)max_offsets, nchunks);
        note_kernels(1, "cw::cdc_scan_kernel, cw::cdc_spec_kernel, cw::cdc_merge_kernel, cw::cdc_fixup_kernel");
    }
    return hipGetLastError();
}
} // namespace

hipError_t cdc_launch(const CdcParams &p, const uint8_t *src, size_t nbytes, int final_, uint64_t *offsets, size_t max_offsets,
                      uint64_t *nchunks, uint64_t seg, hipStream_t stream)
{
    if (nbytes == 0) {
        hipError_t e = hipMemsetAsync(offsets, 0, sizeof(uint64_t), stream);
        return e != hipSuccess ? e : hipMemsetAsync(nchunks, 0, sizeof(uint64_t), stream);
    }
    return cdc_launch_any(p, src, nbytes, final_, offsets, max_offsets, nchunks, seg, nullptr, stream);
}

hipError_t cdc_streams_launch(const CdcParams &p, const uint8_t *src, size_t nbytes, const CdcStreams &st, uint64_t *offsets, size_t max_offsets,
                              uint64_t *nchunks, uint64_t seg, hipStream_t stream)
{
    if (nbytes) return cdc_launch_any(p, src, nbytes, st.final_ ? 1 : 0, offsets, max_offsets, nchunks, seg, &st, stream);
    // no byte, no chunk: the verdict (streams that are all empty) and the empty result
    return cdc_streams_verdict_launch(st, 0, seg, 1, nullptr, offsets, nchunks, stream);
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
