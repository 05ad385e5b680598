// sha256_kernel.hip -- FIPS 180-4 SHA-256 of every storage block, one block per lane (gfx950).
//
// Replaces doSHA256MBHashing (src/hashandcompress/HashAndCompress.cpp:136-158) and
// HashBlockSHA256 / HashBlockSHA256MB (src/hashing_perf/hash.cpp:28-77).  The reference's "multi-buffer"
// manager runs N independent messages in the lanes of an AVX register; here the 64 lanes of a
// wavefront are the buffers: lane i hashes block i, all lanes in lockstep, pure 32-bit VALU
// (v_alignbit_b32 rotates, v_bfi_b32 choose/majority, v_xor3/v_add3).  Unlike the reference (which
// drops the digests, :151-155) the 32-byte big-endian digests are written out.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cw_device.h"
#include "launch_plan.h"

namespace cw {

__constant__ uint32_t K256[64] = {
    0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5,
    0xd807aa98, 0x12835b01, 0x243185be, 0x550c7dc3, 0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174,
    0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc, 0x2de92c6f, 0x4a7484aa, 0x5cb0a9dc, 0x76f988da,
    0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147, 0x06ca6351, 0x14292967,
    0x27b70a85, 0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85,
    0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3, 0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070,
    0x19a4c116, 0x1e376c08, 0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f, 0x682e6ff3,
    0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208, 0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2};

static __device__ __forceinline__ uint32_t rotr(uint32_t x, int r) { return __builtin_amdgcn_alignbit(x, x, r); }
// a ^ b ^ c in one v_bitop3_b32 (truth table 0x96); hipcc emits two v_xor_b32 for the plain expression
static __device__ __forceinline__ uint32_t xor3(uint32_t a, uint32_t b, uint32_t c) { return __builtin_amdgcn_bitop3_b32(a, b, c, 0x96); }

// one 64-byte compression; w[] holds the 16 big-endian message words and is consumed as the rolling schedule
static __device__ __forceinline__ void sha256_compress(uint32_t (&h)[8], uint32_t (&w)[16])
{
    uint32_t a = h[0], b = h[1], c = h[2], d = h[3], e = h[4], f = h[5], g = h[6], hh = h[7];
#pragma unroll
    for (int i = 0; i < 64; i++) {
        if (i >= 16) {
            const uint32_t w15 = w[(i - 15) & 15], w2 = w[(i - 2) & 15];
            const uint32_t s0 = xor3(rotr(w15, 7), rotr(w15, 18), w15 >> 3);
            const uint32_t s1 = xor3(rotr(w2, 17), rotr(w2, 19), w2 >> 10);
            w[i & 15] = w[i & 15] + s0 + w[(i - 7) & 15] + s1;
        }
        const uint32_t S1 = xor3(rotr(e, 6), rotr(e, 11), rotr(e, 25));
        const uint32_t ch = (e & f) | (~e & g);
        const uint32_t t1 = hh + S1 + ch + K256[i] + w[i & 15];
        const uint32_t S0 = xor3(rotr(a, 2), rotr(a, 13), rotr(a, 22));
        const uint32_t mj = (a & b) | (c & (a | b));
        const uint32_t t2 = S0 + mj;
        hh = g; g = f; f = e; e = d + t1;
        d = c; c = b; b = a; a = t1 + t2;
    }
    h[0] += a; h[1] += b; h[2] += c; h[3] += d; h[4] += e; h[5] += f; h[6] += g; h[7] += hh;
}

template <bool ALIGNED16>
static __device__ __forceinline__ void load_chunk(uint32_t (&w)[16], const uint8_t *p)
{
    if (ALIGNED16) {
        const uint4 *q = reinterpret_cast<const uint4 *>(p);
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const uint4 v = q[i];
            w[4 * i] = __builtin_bswap32(v.x); w[4 * i + 1] = __builtin_bswap32(v.y);
            w[4 * i + 2] = __builtin_bswap32(v.z); w[4 * i + 3] = __builtin_bswap32(v.w);
        }
    } else {
#pragma unroll
        for (int i = 0; i < 16; i++)
            w[i] = ((uint32_t)p[4 * i] << 24) | ((uint32_t)p[4 * i + 1] << 16) | ((uint32_t)p[4 * i + 2] << 8) | p[4 * i + 3];
    }
}

// padding chunk `which` (0 or 1) of a message whose last partial chunk holds `rem` bytes at p (cold path)
static __device__ __noinline__ void load_padding(uint32_t (&w)[16], const uint8_t *p, unsigned rem, unsigned which, uint64_t bits, bool two)
{
#pragma unroll
    for (int i = 0; i < 16; i++) {
        uint32_t v = 0;
        for (int b = 0; b < 4; b++) {
            const unsigned idx = which * 64 + 4 * i + b;
            uint32_t byte = 0;
            if (idx < rem) byte = p[idx];
            else if (idx == rem) byte = 0x80;
            v = (v << 8) | byte;
        }
        w[i] = v;
    }
    if (which == (two ? 1u : 0u)) { w[14] = (uint32_t)(bits >> 32); w[15] = (uint32_t)bits; }
}

// RAGGED=false: block_bytes is a multiple of 64, so the single padding chunk is a wave-uniform constant.
template <bool ALIGNED16, bool RAGGED>
__global__ void __launch_bounds__(CW_SKEIN_THREADS)
sha256_blocks_kernel(const uint8_t *__restrict__ src, size_t block_bytes, size_t src_stride, size_t nblocks,
                     uint8_t *__restrict__ digests)
{
    const size_t gid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= nblocks) return;
    const uint8_t *p = src + gid * src_stride;
    const size_t nfull = block_bytes / 64;
    const unsigned rem = RAGGED ? (unsigned)(block_bytes % 64) : 0;
    const bool two = rem >= 56;                 // 0x80 + length do not fit the partial chunk
    const size_t nsteps = nfull + 1 + (two ? 1 : 0);
    const uint64_t bits = (uint64_t)block_bytes * 8;

    uint32_t h[8] = {0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19};
    uint32_t w[16];

    if (RAGGED) {
        auto fetch = [&](uint32_t (&dst)[16], size_t step) __attribute__((always_inline)) {
            if (step < nfull) load_chunk<ALIGNED16>(dst, p + step * 64);
            else load_padding(dst, p + nfull * 64, rem, (unsigned)(step - nfull), bits, two);
        };
        fetch(w, 0);
#pragma unroll 1
        for (size_t step = 0; step < nsteps; step++) {
            uint32_t nx[16];
            if (step + 1 < nsteps) fetch(nx, step + 1);
            sha256_compress(h, w);
#pragma unroll
            for (int i = 0; i < 16; i++) w[i] = nx[i];
        }
    } else {
        // Hot path.  The next chunk's loads are issued unconditionally (the padding step re-reads the last chunk and
        // is replaced) and are only touched AFTER this chunk's 64 rounds: a branch around the loads, or a byte swap
        // right behind them, makes hipcc put s_waitcnt vmcnt(0) in front of the rounds and nothing overlaps.
        load_chunk<ALIGNED16>(w, p);
#pragma unroll 1
        for (size_t step = 0; step < nsteps; step++) {
            const size_t nxt = step + 1;
            const bool msg = nxt < nfull; // wave-uniform
            const uint8_t *q = p + (msg ? nxt : nfull - 1) * 64;
            uint32_t raw[16];
            if (ALIGNED16) {
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    const uint4 v = reinterpret_cast<const uint4 *>(q)[i];
                    raw[4 * i] = v.x; raw[4 * i + 1] = v.y; raw[4 * i + 2] = v.z; raw[4 * i + 3] = v.w;
                }
            } else {
                load_chunk<false>(raw, q);
            }
            sha256_compress(h, w);
#pragma unroll
            for (int i = 0; i < 16; i++) {
                const uint32_t v = ALIGNED16 ? __builtin_bswap32(raw[i]) : raw[i];
                const uint32_t pad = i == 0 ? 0x80000000u : i == 14 ? (uint32_t)(bits >> 32) : i == 15 ? (uint32_t)bits : 0u;
                w[i] = msg ? v : pad;
            }
        }
    }

    uint8_t *o = digests + gid * 32;
    if ((reinterpret_cast<uintptr_t>(o) & 15) == 0) {
        uint4 *out = reinterpret_cast<uint4 *>(o);
        out[0] = make_uint4(__builtin_bswap32(h[0]), __builtin_bswap32(h[1]), __builtin_bswap32(h[2]), __builtin_bswap32(h[3]));
        out[1] = make_uint4(__builtin_bswap32(h[4]), __builtin_bswap32(h[5]), __builtin_bswap32(h[6]), __builtin_bswap32(h[7]));
    } else { // any alignment: big-endian bytes
#pragma unroll
        for (int k = 0; k < 32; k++) o[k] = (uint8_t)(h[k >> 2] >> (24 - 8 * (k & 3)));
    }
}

// Variable-length chunks (cw_dev_hash_chunks): lane j hashes chunk perm[j], starting at any byte.  Each 64-byte step comes from
// five aligned granules shifted by the chunk's misalignment; the bytes past the chunk, the 0x80 terminator and the length are
// applied only on the steps that reach the chunk's end.
__global__ void __launch_bounds__(CW_SKEIN_THREADS)
sha256_chunks_kernel(const uint8_t *__restrict__ src, size_t src_bytes, const uint64_t *__restrict__ offsets, const uint32_t *__restrict__ perm,
                     const uint64_t *__restrict__ d_n, size_t max_chunks, uint8_t *__restrict__ digests)
{
    const size_t k = *d_n < max_chunks ? *d_n : max_chunks;
    const size_t gid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= k) return;
    const uint32_t ci = perm[gid];
    uint64_t s = offsets[ci], e = offsets[ci + 1];
    s = s < src_bytes ? s : src_bytes;
    e = e < src_bytes ? e : src_bytes;
    if (e < s) e = s;
    const uint64_t len = e - s;
    const size_t nsteps = len / 64 + 1 + ((len % 64) >= 56 ? 1 : 0);
    const uint64_t bits = len * 8;
    const unsigned sh = (unsigned)(reinterpret_cast<uintptr_t>(src + s) & 15);
    const uint8_t *a0 = src + s - sh;
    const uint8_t *last = reinterpret_cast<const uint8_t *>(reinterpret_cast<uintptr_t>(src + (e ? e - 1 : 0)) & ~(uintptr_t)15);

    uint32_t h[8] = {0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19};
    auto message = [&](uint32_t (&w)[16], const uint32_t (&raw)[20], size_t st) __attribute__((always_inline)) {
        uint32_t d[16];
        chunk_shift<5>(d, raw, sh);
        const int64_t left = (int64_t)len - (int64_t)(st * 64);
        if (left < 64) {
#pragma unroll
            for (int j = 0; j < 16; j++) {
                const int64_t v = left - 4 * j;
                d[j] = chunk_keep(d[j], v) | (v >= 0 && v < 4 ? 0x80u << (8 * (unsigned)v) : 0u);
            }
        }
#pragma unroll
        for (int j = 0; j < 16; j++) w[j] = __builtin_bswap32(d[j]);
        if (st + 1 == nsteps) { w[14] = (uint32_t)(bits >> 32); w[15] = (uint32_t)bits; }
    };
    uint32_t raw[20], w[16];
    if (src_bytes) chunk_granules<5>(raw, a0, last);
    else {
#pragma unroll
        for (int j = 0; j < 20; j++) raw[j] = 0;
    }
    message(w, raw, 0);
#pragma unroll 1
    for (size_t st = 0; st < nsteps; st++) {
        if (src_bytes) chunk_granules<5>(raw, a0 + (st + 1) * 64, last);
        sha256_compress(h, w);
        if (st + 1 < nsteps) message(w, raw, st + 1);
    }

    uint8_t *o = digests + (size_t)ci * 32;
    if ((reinterpret_cast<uintptr_t>(o) & 15) == 0) {
        uint4 *out = reinterpret_cast<uint4 *>(o);
        out[0] = make_uint4(__builtin_bswap32(h[0]), __builtin_bswap32(h[1]), __builtin_bswap32(h[2]), __builtin_bswap32(h[3]));
        out[1] = make_uint4(__builtin_bswap32(h[4]), __builtin_bswap32(h[5]), __builtin_bswap32(h[6]), __builtin_bswap32(h[7]));
    } else {
#pragma unroll
        for (int j = 0; j < 32; j++) o[j] = (uint8_t)(h[j >> 2] >> (24 - 8 * (j & 3)));
    }
}

hipError_t sha256_chunks_launch(const uint8_t *src, size_t src_bytes, const uint64_t *offsets, const uint32_t *perm, const uint64_t *d_n,
                                size_t max_chunks, uint8_t *digests, hipStream_t stream)
{
    if (max_chunks == 0) return hipSuccess;
    const dim3 grid((unsigned)((max_chunks + CW_SKEIN_THREADS - 1) / CW_SKEIN_THREADS)), block(CW_SKEIN_THREADS);
    hipLaunchKernelGGL(sha256_chunks_kernel, grid, block, 0, stream, src, src_bytes, offsets, perm, d_n, max_chunks, digests);
    note_kernels(1, "cw::sha256_chunks_kernel");
    return hipGetLastError();
}

// ---- the kernel family of the launch (launch_plan.h): member, name as rocprofv3 prints it, kernel ----
namespace {
struct Sha256Row { bool aligned, ragged; const char *name; decltype(sha256_blocks_kernel<true, true>) *fn; };
#define CW_ROW(A, R) {A, R, "cw::sha256_blocks_kernel<" #A ", " #R ">", sha256_blocks_kernel<A, R>}
const Sha256Row kSha256Kernels[] = {CW_ROW(true, false), CW_ROW(true, true), CW_ROW(false, false), CW_ROW(false, true)};
#undef CW_ROW
const Sha256Row &sha256_row(bool aligned, bool ragged) { return kSha256Kernels[(aligned ? 0 : 2) + (ragged ? 1 : 0)]; }
} // namespace
const char *sha256_kernel_name(bool aligned, bool ragged) { return sha256_row(aligned, ragged).name; }

hipError_t sha256_launch(const HashPlan &p, const uint8_t *src, size_t block_bytes, size_t src_stride, size_t nblocks, uint8_t *digests,
                         hipStream_t stream)
{
    if (nblocks == 0) return hipSuccess;
    const Sha256Row &row = sha256_row(p.aligned, p.ragged);
    hipLaunchKernelGGL(row.fn, dim3(p.grid), dim3(CW_SKEIN_THREADS), 0, stream, src, block_bytes, src_stride, nblocks, digests);
    note_kernels(1, row.name);
    return hipGetLastError();
}

} // namespace cw
