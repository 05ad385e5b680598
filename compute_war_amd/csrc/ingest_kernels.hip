// ingest_kernels.hip -- the device side of a streamed ingest (DESIGN.md sections 18 and 21): the commit that appends one piece's refs
// and cuts to the recipe that grows on the device, and the counts a piece's one synchronise brings to the host.
//
// Commit: the append's shape (restore_kernels.hip).  A copy kernel whose every workgroup reads the recipe's cursor and the store's
// verdict, and one thread behind it that moves the cursor, adds to the statistics and reports.  Both are gated on the same verdict
// function, and the cursor is written only by the one thread, after the copy: a piece that is not committed changes nothing, in the
// recipe or in its stream index.  One pair of kernels serves cw_dev_ingest_commit and cw_dev_ingest_commit_streams: the first is the
// second with the empty stream list, for which verdict 3 cannot arise and the index loop runs zero times.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cw_device.h"
#include "stream_scratch.h"

namespace cw {

namespace {

constexpr unsigned kThreads = 256;

// what the copy and the cursor are gated on.  1: the store refused the piece; 2: its n refs and n + 1 cuts do not fit behind the c
// entries of the recipe (c + n + 1 > rec_cap, without wrapping); 3: its streams do not fit the stream index (first_stream + nstreams >
// first_cap, without wrapping)
__device__ __forceinline__ uint32_t commit_verdict(const uint64_t *store_result, uint64_t c, uint64_t n, uint64_t rec_cap, const CommitStreams &cs)
{
    if (store_result && store_result[0] != 0) return 1u;
    if (c >= rec_cap || n > rec_cap - c - 1) return 2u;
    return cs.first_stream > cs.first_cap || cs.nstreams > cs.first_cap - cs.first_stream ? 3u : 0u;
}

__global__ void __launch_bounds__(kThreads)
commit_copy_kernel(const uint64_t *__restrict__ ref, const uint64_t *__restrict__ offsets, const uint64_t *__restrict__ d_nchunks, uint64_t max_chunks,
                   const uint64_t *__restrict__ store_result, uint64_t stream_off, uint64_t *__restrict__ rec_ref, uint64_t *__restrict__ rec_off,
                   const uint64_t *__restrict__ d_rec_count, uint64_t rec_cap, CommitStreams cs)
{
    const uint64_t n = umin64(*d_nchunks, max_chunks), c = *d_rec_count, threads = (uint64_t)gridDim.x * kThreads;
    if (commit_verdict(store_result, c, n, rec_cap, cs)) return;
    const uint64_t i0 = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    for (uint64_t j = i0; j <= n; j += threads) {
        rec_off[c + j] = stream_off + offsets[j];
        if (j < n) rec_ref[c + j] = ref[j];
    }
    // (a stream's first chunk is at most the piece's count: an index past it can only come from a caller's own array)
    for (uint64_t f = cs.skip_first + i0; f < cs.nstreams; f += threads) cs.rec_first[cs.first_stream + f] = c + umin64(cs.first[f], n);
}

// one thread, behind the copy: the cursor, the statistics {bytes, chunks, new chunks, stored bytes, pieces} and the verdict
__global__ void __launch_bounds__(64)
commit_finish_kernel(const uint64_t *__restrict__ offsets, const uint64_t *__restrict__ d_nchunks, uint64_t max_chunks,
                     const uint64_t *__restrict__ d_n_new, const uint64_t *__restrict__ store_result, uint64_t *__restrict__ d_rec_count,
                     uint64_t rec_cap, uint64_t *__restrict__ stats, uint64_t *__restrict__ d_verdict, CommitStreams cs)
{
    if (threadIdx.x != 0) return;
    const uint64_t n = umin64(*d_nchunks, max_chunks), c = *d_rec_count;
    const uint32_t verdict = commit_verdict(store_result, c, n, rec_cap, cs);
    *d_verdict = verdict;
    if (verdict) return;
    *d_rec_count = c + n;
    if (stats) {
        stats[0] += offsets[n] - offsets[0];
        stats[1] += n;
        stats[2] += *d_n_new;
        if (store_result) stats[3] += store_result[1];
        stats[4] += 1;
    }
}

// one thread: what the host needs to admit a piece -- its chunk count, the bytes its chunks consume, the store's cursor and the
// verdict of the commit before it -- in one place, so that one copy brings them back
__global__ void __launch_bounds__(64)
piece_counts_kernel(const uint64_t *__restrict__ offsets, const uint64_t *__restrict__ d_nchunks, uint64_t max_chunks,
                    const uint64_t *__restrict__ d_used, const uint64_t *__restrict__ d_verdict, uint64_t *__restrict__ counts)
{
    if (threadIdx.x != 0) return;
    const uint64_t n = umin64(*d_nchunks, max_chunks);
    counts[0] = n;
    counts[1] = offsets[n] - offsets[0];
    counts[2] = *d_used;
    counts[3] = *d_verdict;
}

// per stream: nothing but the launch mutex -- two threads that commit to one recipe on one stream, with or without a stream list,
// queue copy and finish as pairs
struct NoScratch { void release() {} };
StreamScratch<NoScratch> commit_sequences;

} // namespace

hipError_t ingest_commit_streams_launch(const uint64_t *ref, const uint64_t *offsets, const uint64_t *d_nchunks, size_t max_chunks,
                                        const uint64_t *d_n_new, const uint64_t *store_result, uint64_t stream_off, uint64_t *rec_ref,
                                        uint64_t *rec_off, uint64_t *d_rec_count, size_t rec_cap, uint64_t *stats, uint64_t *d_verdict,
                                        const CommitStreams &cs, hipStream_t stream)
{
    LaunchLock sequence(commit_sequences.at(stream).launch); // the finish of one call moves the cursor the next call's copy reads
    const size_t items = (max_chunks + 1 > cs.nstreams ? max_chunks + 1 : (size_t)cs.nstreams);
    size_t grid = (items + kThreads - 1) / kThreads;
    if (grid > 256 * 8) grid = 256 * 8;
    if (grid == 0) grid = 1;
    hipLaunchKernelGGL(commit_copy_kernel, dim3((unsigned)grid), dim3(kThreads), 0, stream, ref, offsets, d_nchunks, (uint64_t)max_chunks, store_result,
                       stream_off, rec_ref, rec_off, d_rec_count, (uint64_t)rec_cap, cs);
    hipLaunchKernelGGL(commit_finish_kernel, dim3(1), dim3(64), 0, stream, offsets, d_nchunks, (uint64_t)max_chunks, d_n_new, store_result, d_rec_count,
                       (uint64_t)rec_cap, stats, d_verdict, cs);
    return hipGetLastError();
}

hipError_t ingest_commit_launch(const uint64_t *ref, const uint64_t *offsets, const uint64_t *d_nchunks, size_t max_chunks, const uint64_t *d_n_new,
                                const uint64_t *store_result, uint64_t stream_off, uint64_t *rec_ref, uint64_t *rec_off, uint64_t *d_rec_count,
                                size_t rec_cap, uint64_t *stats, uint64_t *d_verdict, hipStream_t stream)
{
    return ingest_commit_streams_launch(ref, offsets, d_nchunks, max_chunks, d_n_new, store_result, stream_off, rec_ref, rec_off, d_rec_count, rec_cap,
                                        stats, d_verdict, CommitStreams{nullptr, 0, 0, 0, nullptr, 0}, stream);
}

hipError_t piece_counts_launch(const uint64_t *offsets, const uint64_t *d_nchunks, size_t max_chunks, const uint64_t *d_used,
                               const uint64_t *d_verdict, uint64_t *counts, hipStream_t stream)
{
    hipLaunchKernelGGL(piece_counts_kernel, dim3(1), dim3(64), 0, stream, offsets, d_nchunks, (uint64_t)max_chunks, d_used, d_verdict, counts);
    return hipGetLastError();
}

} // namespace cw
