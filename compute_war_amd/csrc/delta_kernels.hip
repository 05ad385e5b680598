// delta_kernels.hip -- what changed between two recipes, and a version shipped as a delta.
// cw_dev_recipe_diff turns two recipes into copy / new ops without reading a byte of data: equal refs mean equal bytes.
// cw_dev_apply_delta rebuilds the new stream from the old one's plain bytes, the ops and the new ops' bytes (the payload).
// Nothing here keeps state between calls, no directory entry is read and nothing is decoded.
//
// The diff, each step behind a kernel boundary of the one before:
//   check    both offset lists ascend strictly in extents of 1..65536 bytes, else the verdict in the scratch head is 1; every kernel
//            behind it reads the verdict and returns when it is 1, so a refused call writes nothing but its verdict
//   clear    the per-entry table to all ones, d_totals[1..7] to zero
//   index    a lane per A position: atomicMin of the position into the table word of the entry it names
//   source   a lane per B position: in place (one binary search in A's offsets), else moved (the table), else new; the byte sums
//   flags    a lane per B position up to max_b: does it start an op, does it start a new op, its new bytes (0 behind the count)
//   scan     three times pack_launch, index only: op ranks, new-op ranks, payload offsets
//   emit     a lane per B position: the one that starts op r writes it (its end: a binary search in the ranks) and its range
// Everything is an integer and atomicMin does not depend on order: the outputs are a function of the arguments.
//
// The apply: a check of the untrusted op list, a lane per op, whose lowest bad op lands in d_result[2] by atomicMin; then the copy,
// tiled by OUTPUT, a wavefront per tile: the tile's first op by binary search, then 64 ops at a time, each lane clipping one op to
// the tile and the wavefront copying the clipped extents one after the other (store_device.h: wave_copy).  An op of a byte and one
// of gigabytes cost what their bytes cost.
//
// Scratch of the diff, per stream: 88 + 4 * dir_entries (rounded up to 8) + 44 * max_b bytes -- a 64-byte head (the verdict at
// [0]), the table, the sources (u64), three scans' offsets (u64, max_b + 1 each) and their sizes (u32).  The apply keeps none.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cw_device.h"
#include "lz_device.h"
#include "store_device.h"

namespace cw {

namespace {

using namespace chunkstore;

typedef unsigned long long u64;
constexpr uint64_t kNone = ~0ull;          // CW_DELTA_NONE
constexpr uint32_t kNoPosition = ~0u;      // a table word no A position has lowered

__device__ __forceinline__ void add64(u64 *p, u64 v)
{
    if (v) __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// one side of the diff: ref[0..n), off[0..n], n = min(*d_n, max)
struct Side {
    const uint64_t *ref, *off, *d_n;
    uint64_t cap;
    __device__ __forceinline__ uint64_t count() const { return umin64(*d_n, cap); }
};

// ---- 1. the check ------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kThreads)
diff_check_kernel(Side a, Side b, uint32_t *__restrict__ verdict)
{
    __shared__ u64 wsum[kThreads / 64];
    const uint64_t na = a.count(), nb = b.count(), threads = (uint64_t)gridDim.x * kThreads, t = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    uint32_t bad = 0;
    for (uint64_t j = t; j < na; j += threads) {
        const uint64_t s = a.off[j], e = a.off[j + 1];
        bad |= !(s < e && e - s <= kMaxChunkBytes);
    }
    for (uint64_t j = t; j < nb; j += threads) {
        const uint64_t s = b.off[j], e = b.off[j + 1];
        bad |= !(s < e && e - s <= kMaxChunkBytes);
    }
    const u64 all = group_sum(bad, wsum);
    if (threadIdx.x == 0 && all) atomicOr(verdict, 1u);
}

// ---- 2. the clear ------------------------------------------------------------------------------------------------------------------
// totals[0] = the verdict; verdict 0: the table to all ones, totals[1..7] to zero
__global__ void __launch_bounds__(kThreads)
diff_clear_kernel(const uint32_t *__restrict__ verdict, uint64_t dir_entries, uint32_t *__restrict__ table, uint64_t *__restrict__ totals)
{
    const uint32_t v = *verdict;
    const uint64_t threads = (uint64_t)gridDim.x * kThreads, t = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (t == 0) totals[0] = v;
    if (v) return; // (words 1..7 keep what they hold)
    if (t >= 1 && t < 8) totals[t] = 0;
    for (uint64_t idx = t; idx < dir_entries; idx += threads) table[idx] = kNoPosition;
}

// ---- 3. the index of A ---------------------------------------------------------------------------------------------------------------
// table[idx] = the lowest A position that names entry idx (positions are below 2^32 - 256: the host)
__global__ void __launch_bounds__(kThreads)
diff_index_kernel(const uint32_t *__restrict__ verdict, Side a, uint64_t dir_base, uint64_t dir_entries, uint32_t *__restrict__ table)
{
    if (*verdict) return;
    const uint64_t na = a.count(), threads = (uint64_t)gridDim.x * kThreads;
    for (uint64_t j = (uint64_t)blockIdx.x * kThreads + threadIdx.x; j < na; j += threads) {
        uint64_t idx;
        if (names_entry(a.ref[j], dir_base, dir_entries, idx)) atomicMin(&table[idx], (uint32_t)j);
    }
}

// ---- 4. the sources ------------------------------------------------------------------------------------------------------------------
// the smallest j in [0, n] with off[j] - off[0] >= x, n where there is none (verdict 0: off ascends, so the differences do not wrap)
__device__ __forceinline__ uint64_t first_at_least(const uint64_t *__restrict__ off, uint64_t n, uint64_t x)
{
    const uint64_t base = off[0];
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if (off[mid] - base >= x) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

// src[i] (and d_src[i]) for i < nb; totals[3..7] += the in-place, moved and new bytes, the matched positions, the positions
__global__ void __launch_bounds__(kThreads)
diff_source_kernel(const uint32_t *__restrict__ verdict, Side a, Side b, uint64_t dir_base, uint64_t dir_entries,
                   const uint32_t *__restrict__ table, uint64_t *__restrict__ src, uint64_t *__restrict__ d_src, u64 *__restrict__ totals)
{
    __shared__ u64 wsum[kThreads / 64];
    if (*verdict) return;
    const uint64_t na = a.count(), nb = b.count(), threads = (uint64_t)gridDim.x * kThreads;
    u64 in_place = 0, moved = 0, fresh = 0, matched = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x; i < nb; i += threads) {
        const uint64_t s = b.off[i], len = b.off[i + 1] - s, zb = s - b.off[0], r = b.ref[i];
        uint64_t idx, from = kNone;
        if (names_entry(r, dir_base, dir_entries, idx)) {
            const uint64_t j = first_at_least(a.off, na, zb); // (na == 0: j = 0 = na, nothing is loaded through it)
            if (j < na && a.off[j] - a.off[0] == zb && a.ref[j] == r && a.off[j + 1] - a.off[j] == len) {
                from = zb;
                in_place += len;
            } else {
                const uint32_t low = table[idx]; // (a position the index pass saw: below na)
                if (low != kNoPosition && a.off[(uint64_t)low + 1] - a.off[low] == len) {
                    from = a.off[low] - a.off[0];
                    moved += len;
                }
            }
        }
        if (from == kNone) fresh += len;
        else matched++;
        src[i] = from;
        if (d_src) d_src[i] = from;
    }
    const u64 t3 = group_sum(in_place, wsum), t4 = group_sum(moved, wsum), t5 = group_sum(fresh, wsum), t6 = group_sum(matched, wsum);
    if (threadIdx.x != 0) return;
    add64(totals + 3, t3);
    add64(totals + 4, t4);
    add64(totals + 5, t5);
    add64(totals + 6, t6);
    if (blockIdx.x == 0) totals[7] = nb;
}

// ---- 5. the flags ------------------------------------------------------------------------------------------------------------------
// for every i < max_b, zero behind the count: start[i] = position i starts an op, new_start[i] = ... a new op, new_len[i] = its
// length when it is new.  Position i continues the op of i - 1 when both are new, or both are copies and src[i] == src[i-1] + len(i-1).
__global__ void __launch_bounds__(kThreads)
diff_flags_kernel(const uint32_t *__restrict__ verdict, Side b, const uint64_t *__restrict__ src, uint32_t *__restrict__ start,
                  uint32_t *__restrict__ new_start, uint32_t *__restrict__ new_len)
{
    if (*verdict) return;
    const uint64_t nb = b.count(), threads = (uint64_t)gridDim.x * kThreads;
    for (uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x; i < b.cap; i += threads) {
        uint32_t st = 0, ns = 0, nl = 0;
        if (i < nb) {
            const uint64_t s = src[i], at = b.off[i];
            st = 1;
            if (i) {
                const uint64_t p = src[i - 1], before = at - b.off[i - 1];
                st = !((s == kNone && p == kNone) || (s != kNone && p != kNone && s == p + before));
            }
            ns = st && s == kNone;
            nl = s == kNone ? (uint32_t)(b.off[i + 1] - at) : 0u; // (verdict 0: at most 65536)
        }
        start[i] = st;
        new_start[i] = ns;
        new_len[i] = nl;
    }
}

// ---- 6. the ops ------------------------------------------------------------------------------------------------------------------
struct DiffOut {
    uint64_t *ops;      // cw_delta_op: {b_off, len, a_off, payload_off}
    uint64_t max_ops;
    uint64_t *nops, *new_off, *new_len, *new_dst, *nnew; // the range arrays may be NULL, all four
};

// rank[i] = the ops that start in front of i, for i <= max_b (so rank[max_b] = the ops); new_rank and payload likewise.  The lane of
// the position that starts op r writes it: the op ends where op r + 1 starts, the first p behind i with rank[p + 1] > r + 1, or at nb.
__global__ void __launch_bounds__(kThreads)
diff_emit_kernel(const uint32_t *__restrict__ verdict, Side b, const uint64_t *__restrict__ src, const uint32_t *__restrict__ start,
                 const u64 *__restrict__ rank, const u64 *__restrict__ new_rank, const u64 *__restrict__ payload, DiffOut out,
                 uint64_t *__restrict__ totals)
{
    if (*verdict) return;
    const uint64_t nb = b.count(), threads = (uint64_t)gridDim.x * kThreads, t = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    const uint64_t nops = rank[b.cap], nnew = new_rank[b.cap];
    const bool fits = nops <= out.max_ops;
    if (t == 0) {
        totals[1] = nops;
        totals[2] = nnew;
        if (!fits) totals[0] = 2;
        *out.nops = fits ? nops : 0;
        if (out.nnew) *out.nnew = fits ? nnew : 0;
    }
    if (!fits) return;
    for (uint64_t i = t; i < nb; i += threads) {
        if (!start[i]) continue;
        const uint64_t r = rank[i]; // (rank[i + 1] = r + 1)
        uint64_t lo = i + 1, hi = b.cap + 1; // the smallest p in (i, max_b] with rank[p] > r + 1, max_b + 1 where there is none
        while (lo < hi) {
            const uint64_t mid = lo + ((hi - lo) >> 1);
            if (rank[mid] > r + 1) hi = mid;
            else lo = mid + 1;
        }
        const uint64_t next = lo > b.cap ? nb : lo - 1, at = b.off[i], len = b.off[next] - at, from = src[i];
        const bool fresh = from == kNone;
        uint64_t *op = out.ops + 4 * r;
        op[0] = at - b.off[0];
        op[1] = len;
        op[2] = from;
        op[3] = fresh ? payload[i] : kNone;
        if (fresh && out.new_off) {
            const uint64_t q = new_rank[i];
            out.new_off[q] = at;
            out.new_len[q] = len;
            out.new_dst[q] = payload[i];
        }
    }
}

// per stream: the head, the table, the sources, the three scans
StreamScratch<DeviceBuf> diff_spaces;

// ---- the apply ------------------------------------------------------------------------------------------------------------------
struct Op {
    uint64_t b_off, len, a_off, payload_off;
    __device__ __forceinline__ explicit Op(const uint64_t *__restrict__ p) : b_off(p[0]), len(p[1]), a_off(p[2]), payload_off(p[3]) {}
};

// result[2] (preset to all ones) = the lowest op that is malformed: it does not start where the one before ends (op 0: at 0), it is
// empty, its end wraps, it names both sources or neither, or it leaves its source
__global__ void __launch_bounds__(kThreads)
apply_check_kernel(const uint64_t *__restrict__ ops, const uint64_t *__restrict__ d_nops, uint64_t max_ops, uint64_t old_bytes,
                   uint64_t payload_bytes, u64 *__restrict__ result)
{
    const uint64_t n = umin64(*d_nops, max_ops), threads = (uint64_t)gridDim.x * kThreads;
    uint64_t lowest = kNone;
    for (uint64_t k = (uint64_t)blockIdx.x * kThreads + threadIdx.x; k < n; k += threads) {
        const Op op(ops + 4 * k);
        const uint64_t expect = k ? ops[4 * (k - 1)] + ops[4 * (k - 1) + 1] : 0;
        const bool copy = op.a_off != kNone, fresh = op.payload_off != kNone;
        const uint64_t room = copy ? old_bytes : payload_bytes, from = copy ? op.a_off : op.payload_off;
        const bool good = op.b_off == expect && op.len != 0 && op.b_off + op.len > op.b_off && copy != fresh && op.len <= room &&
                          from <= room - op.len;
        if (!good && lowest == kNone) lowest = k;
    }
    if (lowest != kNone) atomicMin(result + 2, (u64)lowest);
}

// the largest k in [0, n) with ops[k].b_off <= x (checked list: op 0 starts at 0 and the starts ascend)
__device__ __forceinline__ uint64_t op_at(const uint64_t *__restrict__ ops, uint64_t n, uint64_t x)
{
    uint64_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if (ops[4 * mid] <= x) lo = mid;
        else hi = mid;
    }
    return lo;
}

// A wavefront per tile of the destination, grid-stride.  Every wavefront reaches the call's verdict on its own, from result[2] and
// the last op, and returns at once unless it is 0; thread 0 of workgroup 0 writes result[0], [1] and [3].
__global__ void __launch_bounds__(64)
apply_copy_kernel(const uint8_t *__restrict__ old, const uint8_t *__restrict__ payload, const uint64_t *__restrict__ ops,
                  const uint64_t *__restrict__ d_nops, uint64_t max_ops, uint8_t *__restrict__ dst, uint64_t dst_bytes, uint32_t tile_shift,
                  uint64_t *__restrict__ result)
{
    const uint64_t n = umin64(*d_nops, max_ops);
    const bool malformed = result[2] != kNone;
    const uint64_t total = malformed || n == 0 ? 0 : ops[4 * (n - 1)] + ops[4 * (n - 1) + 1];
    const uint32_t verdict = malformed ? 1u : total > dst_bytes ? 2u : 0u;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        result[0] = verdict;
        result[1] = total;
        result[3] = n;
    }
    if (verdict) return;
    const uint64_t tile = (uint64_t)1 << tile_shift, tiles = (total + tile - 1) >> tile_shift;
    for (uint64_t w = blockIdx.x; w < tiles; w += gridDim.x) { // (wave-uniform: the copies below need every lane)
        const uint64_t t0 = w << tile_shift, t1 = umin64(t0 + tile, total);
        for (uint64_t first = op_at(ops, n, t0); first < n; first += 64) {
            const uint64_t k = first + threadIdx.x;
            bool have = false, copy = false;
            uint64_t from = 0, to = 0;
            uint32_t len = 0;
            if (k < n) {
                const Op op(ops + 4 * k);
                const uint64_t lo = op.b_off > t0 ? op.b_off : t0, hi = umin64(op.b_off + op.len, t1);
                have = lo < hi; // (an op behind the tile: none)
                copy = op.a_off != kNone;
                if (have) {
                    from = (copy ? op.a_off : op.payload_off) + (lo - op.b_off);
                    to = lo;
                    len = (uint32_t)(hi - lo); // (at most a tile: 256 KiB)
                }
            }
            wave_copy(have && copy, old, from, dst, to, len);
            wave_copy(have && !copy, payload, from, dst, to, len);
            if (__ballot(have) != ~0ull) break; // the ops tile the output: a lane without a piece is behind the tile or the list
        }
    }
}

} // namespace

hipError_t recipe_diff_launch(const uint64_t *ref_a, const uint64_t *off_a, const uint64_t *d_na, size_t max_a, const uint64_t *ref_b,
                              const uint64_t *off_b, const uint64_t *d_nb, size_t max_b, uint64_t dir_base, size_t dir_entries, void *ops,
                              size_t max_ops, uint64_t *nops, uint64_t *src, uint64_t *new_off, uint64_t *new_len, uint64_t *new_dst,
                              uint64_t *nnew, uint64_t *totals, hipStream_t stream)
{
    auto &w = diff_spaces.at(stream);
    LaunchLock sequence(w.launch); // the head, the table and the scans are shared by the launches below
    hipError_t e = w.reserve(recipe_diff_scratch_bytes(max_b, dir_entries), (size_t)1 << 20);
    if (e != hipSuccess) return e;
    uint8_t *head = w.as<uint8_t>();
    uint32_t *verdict = w.as<uint32_t>(), *table = reinterpret_cast<uint32_t *>(head + kScratchHead);
    uint64_t *sources = reinterpret_cast<uint64_t *>(head + kScratchHead + ((dir_entries * 4 + 7) & ~(size_t)7));
    ScanScratch rank{head, sources + max_b, nullptr}, new_rank{head, rank.off + max_b + 1, nullptr}, payload{head, new_rank.off + max_b + 1, nullptr};
    rank.sizes = reinterpret_cast<uint32_t *>(payload.off + max_b + 1);
    new_rank.sizes = rank.sizes + max_b;
    payload.sizes = new_rank.sizes + max_b;
    if ((e = hipMemsetAsync(head, 0, kScratchHead, stream)) != hipSuccess) return e;
    const Side a{ref_a, off_a, d_na, (uint64_t)max_a}, b{ref_b, off_b, d_nb, (uint64_t)max_b};
    const size_t most = max_a > max_b ? max_a : max_b;
    if (most) hipLaunchKernelGGL(diff_check_kernel, dim3(lane_grid(most)), dim3(kThreads), 0, stream, a, b, verdict);
    hipLaunchKernelGGL(diff_clear_kernel, dim3(lane_grid(dir_entries)), dim3(kThreads), 0, stream, verdict, (uint64_t)dir_entries, table, totals);
    if (max_a)
        hipLaunchKernelGGL(diff_index_kernel, dim3(lane_grid(max_a)), dim3(kThreads), 0, stream, verdict, a, dir_base, (uint64_t)dir_entries, table);
    if (max_b) {
        hipLaunchKernelGGL(diff_source_kernel, dim3(lane_grid(max_b)), dim3(kThreads), 0, stream, verdict, a, b, dir_base, (uint64_t)dir_entries,
                           table, sources, src, reinterpret_cast<u64 *>(totals));
        hipLaunchKernelGGL(diff_flags_kernel, dim3(lane_grid(max_b)), dim3(kThreads), 0, stream, verdict, b, sources, rank.sizes, new_rank.sizes,
                           payload.sizes);
    }
    // (max_b == 0: each scan is its one word, 0.  A refused call's scans run over what the scratch holds and are read by nobody)
    for (const ScanScratch *s : {&rank, &new_rank, &payload})
        if ((e = pack_launch(nullptr, 0, s->sizes, max_b, nullptr, s->off, stream)) != hipSuccess) return e;
    const DiffOut out{static_cast<uint64_t *>(ops), (uint64_t)max_ops, nops, new_off, new_len, new_dst, nnew};
    hipLaunchKernelGGL(diff_emit_kernel, dim3(lane_grid(max_b ? max_b : 1)), dim3(kThreads), 0, stream, verdict, b, sources, rank.sizes, rank.offsets(),
                       new_rank.offsets(), payload.offsets(), out, totals);
    return hipGetLastError();
}

size_t recipe_diff_scratch_bytes(size_t max_b, size_t dir_entries)
{
    return kScratchHead + ((dir_entries * 4 + 7) & ~(size_t)7) + max_b * 8 + 3 * (max_b + 1) * 8 + 3 * max_b * 4;
}

// 16 KiB, one round of copy_g2g's loads: over 4 GiB the three sizes measured 1.66 / 1.69 / 1.69 ms (profiles/r24_delta_probe.json)
unsigned apply_delta_tile_shift(long knob_kib) { return knob_kib == 64 ? 16u : knob_kib == 256 ? 18u : 14u; }

hipError_t apply_delta_launch(const uint8_t *old, size_t old_bytes, const uint8_t *payload, size_t payload_bytes, const void *ops,
                              const uint64_t *d_nops, size_t max_ops, uint8_t *dst, size_t dst_bytes, unsigned tile_shift, uint64_t *result,
                              hipStream_t stream)
{
    hipError_t e = hipMemsetAsync(result, 0xFF, 4 * sizeof(uint64_t), stream); // (result[2]: no bad op yet)
    if (e != hipSuccess) return e;
    const uint64_t *list = static_cast<const uint64_t *>(ops);
    if (max_ops)
        hipLaunchKernelGGL(apply_check_kernel, dim3(lane_grid(max_ops)), dim3(kThreads), 0, stream, list, d_nops, (uint64_t)max_ops,
                           (uint64_t)old_bytes, (uint64_t)payload_bytes, reinterpret_cast<u64 *>(result));
    const size_t tiles = (dst_bytes + ((size_t)1 << tile_shift) - 1) >> tile_shift; // (verdict 0: total <= dst_bytes)
    hipLaunchKernelGGL(apply_copy_kernel, dim3(wave_grid(tiles ? tiles : 1)), dim3(64), 0, stream, old, payload, list, d_nops, (uint64_t)max_ops, dst,
                       (uint64_t)dst_bytes, tile_shift, result);
    return hipGetLastError();
}

} // namespace cw
