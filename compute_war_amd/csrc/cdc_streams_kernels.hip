// cdc_streams_kernels.hip -- content-defined chunking of many streams in one device buffer (cw_dev_cdc_streams)
// for gfx950: the resolve of cdc_resolve.h instantiated over CdcS, where a step from `cut` sees as n the smallest stream end above cut
// (so a stream's end is an ordinary cut and the next stream starts there), the lists of segment g hold seg / m + 2 + (ends inside g)
// cuts, and every kernel first reads the verdict on d_ends; and the form's own three kernels: the verdict, the per-segment end index,
// and d_stream_first.  The candidate scan and the summaries are cdc_kernels.hip's, unchanged: H is never reset and every test at
// x >= c + m, m >= 64, reads only bytes at or behind c, so a cut forced at a stream's first byte changes nothing a scan computed.

#include "cdc_resolve.h"

namespace cw {

namespace {

// the verdict (zeroed before): 1 when d_ends decreases anywhere or does not end at n
__global__ void __launch_bounds__(256)
cdc_ends_check_kernel(const uint64_t *__restrict__ ends, uint64_t nstreams, uint64_t n, uint64_t *__restrict__ verdict)
{
    for (uint64_t f = (uint64_t)blockIdx.x * 256 + threadIdx.x; f < nstreams; f += (uint64_t)gridDim.x * 256) {
        const uint64_t e = ends[f], before = f ? ends[f - 1] : 0;
        if (e < before || (f + 1 == nstreams && e != n)) *verdict = 1;
    }
}

// first index in [0, count) with v[index] >= x, else count
__device__ __forceinline__ uint64_t lower_bound(const uint64_t *__restrict__ v, uint64_t count, uint64_t x)
{
    uint64_t lo = 0, hi = count;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (v[mid] < x) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// behind the verdict: refused ends (or n == 0, where no chunk exists) -> the empty result; else eidx[g] for g <= nseg
__global__ void __launch_bounds__(256)
cdc_streams_init_kernel(const uint64_t *__restrict__ ends, uint64_t nstreams, uint64_t n, uint64_t seg, uint64_t nseg,
                        const uint64_t *__restrict__ verdict, uint32_t *__restrict__ eidx, uint64_t *__restrict__ out,
                        uint64_t *__restrict__ nchunks, uint64_t *__restrict__ first)
{
    const uint64_t i0 = (uint64_t)blockIdx.x * 256 + threadIdx.x, step = (uint64_t)gridDim.x * 256;
    if (*verdict || n == 0) {
        if (i0 == 0) { out[0] = 0; *nchunks = 0; }
        for (uint64_t f = i0; f <= nstreams; f += step) first[f] = 0;
        return;
    }
    for (uint64_t g = i0; g <= nseg; g += step) eidx[g] = (uint32_t)lower_bound(ends, nstreams, g * seg);
}

// behind the write: first[f] = the index of the first cut at or behind stream f's start, first[nstreams] = K
__global__ void __launch_bounds__(256)
cdc_stream_first_kernel(const uint64_t *__restrict__ ends, uint64_t nstreams, const uint64_t *__restrict__ verdict,
                        const uint64_t *__restrict__ offsets, const uint64_t *__restrict__ nchunks, uint64_t max_out,
                        uint64_t *__restrict__ first)
{
    if (*verdict) return;
    const uint64_t k = umin(*nchunks, max_out - 1);
    for (uint64_t f = (uint64_t)blockIdx.x * 256 + threadIdx.x; f <= nstreams; f += (uint64_t)gridDim.x * 256)
        first[f] = f == nstreams ? k : lower_bound(offsets, k + 1, f ? ends[f - 1] : 0);
}

unsigned grid256(uint64_t items) { return (unsigned)umin((items + 255) / 256, 4096); }

} // namespace

hipError_t cdc_streams_verdict_launch(const CdcStreams &st, size_t nbytes, uint64_t seg, uint64_t nseg, uint32_t *eidx, uint64_t *offsets,
                                      uint64_t *nchunks, hipStream_t stream)
{
    const hipError_t e = hipMemsetAsync(st.result, 0, sizeof(uint64_t), stream);
    if (e != hipSuccess) return e;
    if (st.nstreams)
        hipLaunchKernelGGL(cdc_ends_check_kernel, dim3(grid256(st.nstreams)), dim3(256), 0, stream, st.ends, (uint64_t)st.nstreams, (uint64_t)nbytes,
                           st.result);
    const uint64_t items = (nseg > st.nstreams ? nseg : st.nstreams) + 1;
    hipLaunchKernelGGL(cdc_streams_init_kernel, dim3(grid256(items)), dim3(256), 0, stream, st.ends, (uint64_t)st.nstreams, (uint64_t)nbytes, seg,
                       nseg, st.result, eidx, offsets, nchunks, st.first);
    return hipGetLastError();
}

hipError_t cdc_streams_resolve_launch(const CdcS &c, uint32_t *counts, hipStream_t stream)
{
    const uint64_t nseg = c.nseg;
    const unsigned sg = (unsigned)((nseg + 63) / 64);
    hipLaunchKernelGGL(cdc_spec_kernel<CdcS>, dim3(sg), dim3(64), 0, stream, c, nseg);
    hipLaunchKernelGGL(cdc_merge_kernel<CdcS>, dim3(sg), dim3(64), 0, stream, c, nseg);
    hipLaunchKernelGGL(cdc_fixup_kernel<CdcS>, dim3(1), dim3(64), 0, stream, c, nseg);
    hipLaunchKernelGGL(cdc_count_kernel<CdcS>, dim3((unsigned)((nseg + 255) / 256)), dim3(256), 0, stream, c, nseg, counts);
    return hipGetLastError();
}

hipError_t cdc_streams_write_launch(const CdcS &c, const CdcStreams &st, const uint64_t *segoff, uint64_t *offsets, size_t max_offsets,
                                    uint64_t *nchunks, hipStream_t stream)
{
    hipLaunchKernelGGL(cdc_write_kernel<CdcS>, dim3((unsigned)c.nseg), dim3(64), 0, stream, c, c.nseg, segoff, offsets, (uint64_t)max_offsets, nchunks);
    hipLaunchKernelGGL(cdc_stream_first_kernel, dim3(grid256(st.nstreams + 1)), dim3(256), 0, stream, st.ends, (uint64_t)st.nstreams, st.result, offsets,
                       nchunks, (uint64_t)max_offsets, st.first);
    note_kernels(1, "cw::cdc_scan_kernel, cw::cdc_spec_kernel<CdcS>, cw::cdc_merge_kernel<CdcS>, cw::cdc_fixup_kernel<CdcS>");
    return hipGetLastError();
}

} // namespace cw
