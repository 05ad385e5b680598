// decompress_kernels.hip -- LZ4-block and LZF decoders for gfx950, one compressed block per wavefront.
//
// The reference decompresses only to time it (LZ4_decompress_safe / lzf_decompress in
// src/compression_perf/src/experiment.cpp:118,256).  Here the decoders are the
// reference-independent verifier of the compressors at full scale: encode -> decode -> compare on the device.
// Format-level decoders (LZ4 block format; LZF stream format, src/compression_perf/include/lzf/lzf.h:83-95),
// bounds-checked like the "safe" variants: a malformed or truncated input gives status 1, never an
// out-of-bounds access -- a size that exceeds the slot (comp_stride) is malformed too, and every length is checked
// against what is left before it is added, so no sum can wrap.
//
// Three kernels decode the same formats (the wavefront decoder with the slot staged in LDS, the same reading the slot from
// global memory, and the lane-per-block decoder); which one a batch is routed to depends on its size and the block size, the
// verdict on a slot does not: status 0 iff the stream is well formed, lies inside its slot and yields exactly block_bytes.
// A valid stream may be longer than its block (LZF: 32-byte literal runs give bs + bs/32, 1-byte runs 2*bs).
//
// A wavefront first copies its compressed block into LDS if it fits the staging buffer (coalesced; parsing token by token
// from global memory costs a dependent ~1 us round trip per token), decodes it into a second LDS buffer (sequences are
// serial, their byte copies are 64 lanes wide; an overlapping match -- offset < length -- is copied in rounds of `offset`
// bytes) and then streams the block out.

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include "cw_device.h"
#include "lane_codec.h"

namespace cw {

namespace {
__device__ __forceinline__ uint32_t bcast(uint32_t x) { return __builtin_amdgcn_readfirstlane(x); }

// out[op .. op+len) = out[op-off ..): overlapping copy, `off` bytes per round at most
__device__ __forceinline__ void copy_match(uint8_t *out, uint32_t op, uint32_t off, uint32_t len, uint32_t lane)
{
    const uint32_t round = off < 64 ? off : 64;
    for (uint32_t done = 0; done < len; done += round) {
        const uint32_t k = done + lane;
        uint8_t b = 0;
        const bool act = lane < round && k < len;
        if (act) b = out[op + k - off];
        __syncthreads(); // all reads of this round before its writes (and LDS ordering across rounds)
        if (act) out[op + k] = b;
        __syncthreads();
    }
}
// One block's sequences, the whole wavefront in step: in[0, n) -> out[0, raw_bytes) (LDS).  Returns bad; op = bytes produced.
// Inlined once per address space of `in` (the staged slot in LDS, the slot itself in global memory).
template <int ALG>
__device__ __forceinline__ bool wave_decode(const uint8_t *in, uint32_t n, uint8_t *out, uint32_t raw_bytes, uint32_t lane, bool bad,
                                            uint32_t &op_out)
{
    uint32_t ip = 0, op = 0;
    if (ALG == 0) {
        while (!bad) {
            if (ip >= n) { bad = true; break; }
            const uint32_t tok = bcast(in[ip]); ip++;
            uint32_t lit = tok >> 4;
            if (lit == 15) {
                uint32_t c;
                do { if (ip >= n) { bad = true; break; } c = bcast(in[ip]); ip++; lit += c; } while (c == 255);
                if (bad) break;
            }
            if (lit > n - ip || lit > raw_bytes - op) { bad = true; break; } // ip <= n, op <= raw_bytes: no wrap
            for (uint32_t i = lane; i < lit; i += 64) out[op + i] = in[ip + i];
            ip += lit; op += lit;
            if (ip == n) break; // last sequence: literals only
            if (n - ip < 2) { bad = true; break; }
            const uint32_t off = bcast((uint32_t)in[ip] | ((uint32_t)in[ip + 1] << 8)); ip += 2;
            if (off == 0 || off > op) { bad = true; break; }
            uint32_t ml = tok & 15;
            if (ml == 15) {
                uint32_t c;
                do { if (ip >= n) { bad = true; break; } c = bcast(in[ip]); ip++; ml += c; } while (c == 255);
                if (bad) break;
            }
            if (ml > raw_bytes || ml + 4 > raw_bytes - op) { bad = true; break; }
            ml += 4;
            copy_match(out, op, off, ml, lane);
            op += ml;
        }
    } else {
        while (!bad && ip < n) {
            const uint32_t ctrl = bcast(in[ip]); ip++;
            if (ctrl < 32) {
                const uint32_t run = ctrl + 1;
                if (run > n - ip || run > raw_bytes - op) { bad = true; break; }
                if (lane < run) out[op + lane] = in[ip + lane];
                ip += run; op += run;
            } else {
                uint32_t len = ctrl >> 5;
                if (ip >= n) { bad = true; break; }
                if (len == 7) { len += bcast(in[ip]); ip++; if (ip >= n) { bad = true; break; } }
                const uint32_t off = (((ctrl & 0x1f) << 8) | bcast(in[ip])) + 1; ip++;
                len += 2;
                if (off > op || len > raw_bytes - op) { bad = true; break; }
                copy_match(out, op, off, len, lane);
                op += len;
            }
        }
    }
    op_out = op;
    return bad;
}
} // namespace

// status[i]: 0 = ok and exactly block_bytes produced, 1 = malformed / wrong size (including sizes[i] == 0, LZF's "did not
// fit": such a block was stored raw and there is nothing to decode) or a size larger than the slot.
template <int ALG, bool STAGE_IN> // ALG: 0 = LZ4, 1 = LZF; STAGE_IN: compressed slot copied to LDS first
__global__ void __launch_bounds__(64)
decompress_kernel(const uint8_t *__restrict__ comp, size_t comp_stride, const uint32_t *__restrict__ sizes, size_t nblocks,
                  uint8_t *__restrict__ dst, uint32_t block_bytes, uint32_t *__restrict__ status, uint32_t in_cap)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t out[]; // block_bytes (rounded to 16), then in_cap bytes of input
    uint8_t *cin = out + ((block_bytes + 15u) & ~15u);
    const uint32_t lane = threadIdx.x;
    for (size_t blk = blockIdx.x; blk < nblocks; blk += gridDim.x) {
        const uint8_t *gin = comp + blk * comp_stride;
        const uint32_t n = sizes[blk];
        uint32_t op = 0;
        // inside the slot; below 2^24 bytes no run of 255s can wrap a length
        bool bad = n == 0 || n > comp_stride || n > (1u << 24);
        // A slot longer than the staging buffer is decoded from where it lies: the verdict never depends on in_cap.  (A valid LZF
        // stream can be longer than its block, up to twice with 1-byte literal runs; the staging buffer holds block_bytes.)
        const bool staged = STAGE_IN && n <= in_cap;
        __syncthreads();
        if (staged && !bad) {
            if ((reinterpret_cast<uintptr_t>(gin) & 15) == 0) {
                for (uint32_t i = lane; i < n / 16; i += 64) reinterpret_cast<uint4 *>(cin)[i] = reinterpret_cast<const uint4 *>(gin)[i];
                for (uint32_t i = (n & ~15u) + lane; i < n; i += 64) cin[i] = gin[i]; // never read past the slot's bytes
            } else {
                for (uint32_t i = lane; i < n; i += 64) cin[i] = gin[i];
            }
        }
        __syncthreads();
        if (__builtin_expect(staged, STAGE_IN)) bad = wave_decode<ALG>(cin, n, out, block_bytes, lane, bad, op);
        else bad = wave_decode<ALG>(gin, n, out, block_bytes, lane, bad, op);
        __syncthreads();
        if (op != block_bytes) bad = true;
        if (!bad) {
            uint8_t *d = dst + blk * (size_t)block_bytes;
            for (uint32_t i = lane; i < block_bytes; i += 64) d[i] = out[i];
        }
        if (lane == 0) status[blk] = bad ? 1u : 0u;
    }
}

// ---------------------------------------------------------------------------------------------------
// Lane-per-block decoders for large batches of large blocks.  A 64 KiB block fills the LDS budget of the wavefront decoder
// with its output alone (two blocks per CU) and its token chain is serial: 7.7 / 6.0 GB/s.  Here a LANE decodes a block
// straight from its slot into its place in dst -- the decoder's loop as it stands (lane_decode in lane_codec.h, shared with the
// decoder over content-defined chunks), 64 per wavefront, bound like the lane-per-block parsers by the lines the memory system
// retires.  Same checks as above: nothing is read outside [0, n) of the slot or written outside the block.
// ---------------------------------------------------------------------------------------------------
template <int ALG>
__global__ void __launch_bounds__(64)
decompress_lanes_kernel(const uint8_t *__restrict__ comp, size_t comp_stride, const uint32_t *__restrict__ sizes, size_t nblocks,
                        uint8_t *__restrict__ dst, uint32_t block_bytes, uint32_t *__restrict__ status)
{
    const size_t lanes = (size_t)gridDim.x * 64;
    for (size_t blk = (size_t)blockIdx.x * 64 + threadIdx.x; blk < nblocks; blk += lanes) {
        const uint8_t *in = comp + blk * comp_stride;
        uint8_t *d = dst + blk * (size_t)block_bytes;
        const uint32_t n = sizes[blk];
        const bool skip = n == 0 || n > comp_stride || n > (1u << 24);
        status[blk] = lane::lane_decode<ALG>(in, n, d, block_bytes, skip) ? 1u : 0u;
    }
}

hipError_t decompress_launch(int alg, const uint8_t *comp, size_t comp_stride, const uint32_t *sizes, size_t nblocks, uint8_t *dst,
                             size_t block_bytes, uint32_t *status, hipStream_t stream)
{
    if (nblocks == 0) return hipSuccess;
    if (block_bytes == 0 || block_bytes > 65536) return hipErrorInvalidValue;
    // Large batches: one block per lane (CW_DECODE_LANES=0 off / =N threshold in blocks).  A lane needs ~0.37 (LZ4) / 0.57 (LZF) us
    // per KiB of block whatever the batch, the wavefront decoders run at 75 / 44 / 22 / 8 GB/s for 4 / 8 / 16 / 64 KiB blocks of
    // text: the lanes win from about 128 MiB of blocks on, and never below ~3,000 blocks (measured: 64 KiB x 2,048 6.1 vs 7.9 GB/s,
    // x 4,096 11.1 vs 7.8, x 65,536 97.7 vs 7.9; 4 KiB x 512 Ki 109.6 vs 75.5).  Unlike the wavefront decoder, which assembles a
    // block in LDS and only stores it when it decoded cleanly, a lane writes as it goes: the bytes of a block with status 1 are
    // unspecified either way.
    const Knobs kn = knobs();
    const size_t by_bytes = ((size_t)128 << 20) / block_bytes;
    const size_t lane_min = kn.decode_lanes ? (size_t)*kn.decode_lanes : (by_bytes > 4096 ? by_bytes : 4096);
    if (lane_min && nblocks >= lane_min) {
        const size_t wpc = kn.lanes_wpc ? (size_t)kn.lanes_wpc : 8;
        size_t lgrid = (nblocks + 63) / 64;
        if (lgrid > 256 * wpc) lgrid = 256 * wpc;
        if (alg == 0)
            hipLaunchKernelGGL(decompress_lanes_kernel<0>, dim3((unsigned)lgrid), dim3(64), 0, stream, comp, comp_stride, sizes, nblocks, dst,
                               (uint32_t)block_bytes, status);
        else
            hipLaunchKernelGGL(decompress_lanes_kernel<1>, dim3((unsigned)lgrid), dim3(64), 0, stream, comp, comp_stride, sizes, nblocks, dst,
                               (uint32_t)block_bytes, status);
        return hipGetLastError();
    }
    // LDS: the decoded block, and -- if at least four blocks per CU still fit (blocks up to ~16 KiB: 4 KiB text decodes
    // 2.2x faster, 64 KiB 1.6x slower with it) -- the compressed slot (at most the codec's bound)
    const uint32_t out_bytes = (uint32_t)((block_bytes + 15) & ~(size_t)15);
    uint32_t in_cap = (uint32_t)(((alg == 0 ? block_bytes + block_bytes / 255 + 16 : block_bytes) + 15) & ~(size_t)15);
    const bool stage_in = out_bytes + in_cap <= 40 * 1024;
    if (!stage_in) in_cap = 0;
    const uint32_t lds = out_bytes + in_cap;
    const size_t per_cu = (160u * 1024u) / lds;
    const size_t want = 256 * (per_cu > 16 ? 16 : per_cu ? per_cu : 1), grid = nblocks < want ? nblocks : want;
    static bool attr_set = false;
    if (!attr_set) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(decompress_kernel<0, false>), hipFuncAttributeMaxDynamicSharedMemorySize, 65536);
        if (e == hipSuccess) e = hipFuncSetAttribute(reinterpret_cast<const void *>(decompress_kernel<1, false>), hipFuncAttributeMaxDynamicSharedMemorySize, 65536);
        if (e != hipSuccess) return e;
        attr_set = true;
    }
#define CW_DECODE(A, S) hipLaunchKernelGGL((decompress_kernel<A, S>), dim3((unsigned)grid), dim3(64), lds, stream, comp, comp_stride, sizes, \
                                           nblocks, dst, (uint32_t)block_bytes, status, in_cap)
    if (alg == 0 && stage_in) CW_DECODE(0, true);
    else if (alg == 0) CW_DECODE(0, false);
    else if (stage_in) CW_DECODE(1, true);
    else CW_DECODE(1, false);
#undef CW_DECODE
    return hipGetLastError();
}

} // namespace cw
