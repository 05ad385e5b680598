// launch_plan.h -- what an LZ4 / LZF compression call and a hash call launch, decided apart from the code that enqueues it.
//
// lz4_plan / lzf_plan are pure: no HIP call, no allocation, no global, no environment -- the call's sizes and alignment facts and one
// knobs snapshot in, every decision of the launch out: the kernel of every stage (a member of its family), grids, LDS bytes, streams,
// the side streams' priority pool, every scalar the kernels get, and the bytes the launch has to reserve.  lz4_launch / lzf_launch
// (lz4_kernel.hip, lzf_kernel.hip) plan, reserve and enqueue; describe() is what cw_profile_kernels reports; dump() is the whole plan
// as text (cw_plan_describe: the policy can be read at any batch size without a device).  The thresholds and the measurements behind
// them are in launch_plan.cpp, beside the decision each serves.
#pragma once

#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "knobs.h"

namespace cw {

// ---- sizes the kernels and the plans share -----------------------------------------------------------------------------------
constexpr uint32_t kTabBytes = (1u << 13) * 2;   // LZ4: 8192 x u16
constexpr uint32_t kStageMax = 16384;            // LZ4 parse kernel: blocks up to this size are staged in LDS
constexpr uint32_t kFpBytes = (1u << 13) / 2;    // LZ4 fingerprint parser: 4-bit fingerprint per table slot
constexpr uint32_t kChunk = 4096;                // LZ4 scan: bytes of a block per lane and step; the span scan's smallest block
constexpr uint32_t kLzfTabBytes = (1u << 16) * 2; // LZF: 65,536 x u16
constexpr uint32_t kInLdsMax = 16384;            // LZF: blocks up to this size are staged in LDS next to the table
constexpr uint32_t kChainMax = 16384;            // LZF link/chain kernels: bytes of a block per piece
constexpr uint32_t kShareSpinCap = 1u << 20;     // LZF LaneShare: polls of ~64 cycles: tens of milliseconds, against the microsecond a claim takes

// ---- kernel families: one enum value per member that is launched ----------------------------------------------------------------
enum class Lz4ScanSpan : uint8_t { unaligned, aligned };                   // lz4_scan_span_kernel<ALIGNED>
enum class Lz4Parse : uint8_t { global, staged, fp8, fp16, fp32 };         // lz4_parse_kernel<STAGED> / lz4_parse_fp_kernel<HEADW>
enum class Lz4Lanes : uint8_t { plain, tagged, fp };                       // lz4_lanes_kernel<MODE>
enum class Lz4Ring : uint8_t { k1, k2, k4, k8 };                           // lz4_lanes_ring_kernel<K>
enum class Lz4Blocks : uint8_t { global, staged };                         // lz4_blocks_kernel<STAGED>
enum class Lz4Vtab : uint8_t { gen2, gen3, lds_table };                    // lz4_vtab2_kernel / lz4_vtab3_kernel<LDSTAB>
enum class LzfLanes : uint8_t { plain, tagged };                           // lzf_lanes_kernel<TAGGED>
enum class LzfChain : uint8_t { small, big, sthread };                     // lzf_chain_kernel<BIG> / lzf_sthread_kernel
enum class LzfParse : uint8_t { global, staged };                          // lzf_parse_kernel<STAGED>

// A family's table, beside its kernels: the member, its name as rocprofv3 prints it, the kernel.  The launch takes the pointer and
// the description the name from the same row.
template <class E, class Fn>
struct KernelRow { E id; const char *name; Fn *fn; };
template <class E, class Fn, size_t N>
inline const KernelRow<E, Fn> &kernel_row(const KernelRow<E, Fn> (&table)[N], E id)
{
    for (const auto &r : table)
        if (r.id == id) return r;
    abort(); // a plan names members of the table only
}
// (defined beside the tables: lz4_kernel.hip, lz4_vtab_kernel.hip, lzf_kernel.hip)
const char *kernel_name(Lz4ScanSpan k);
const char *kernel_name(Lz4Parse k);
const char *kernel_name(Lz4Lanes k);
const char *kernel_name(Lz4Ring k);
const char *kernel_name(Lz4Blocks k);
const char *kernel_name(Lz4Vtab k);
const char *kernel_name(LzfLanes k);
const char *kernel_name(LzfChain k);
const char *kernel_name(LzfParse k);

// ---- the call ---------------------------------------------------------------------------------------------------------------------
struct CodecCall {
    uint32_t n;          // bytes per block
    size_t nblocks;
    unsigned src_n_mis16; // (src | src_stride | n) & 15
    unsigned src_mis4;    // (src | src_stride) & 3
    unsigned dst_mis16;   // (dst | dst_stride) & 15
};
inline CodecCall codec_call(const void *src, size_t block_bytes, size_t src_stride, size_t nblocks, const void *dst, size_t dst_stride)
{
    const uintptr_t s = reinterpret_cast<uintptr_t>(src) | src_stride, d = reinterpret_cast<uintptr_t>(dst) | dst_stride;
    return {(uint32_t)block_bytes, nblocks, (unsigned)((s | block_bytes) & 15), (unsigned)(s & 3), (unsigned)(d & 15)};
}
// what the launch functions refuse (hipErrorInvalidValue)
inline bool lz4_call_valid(size_t block_bytes, size_t nblocks) { return block_bytes != 0 && block_bytes <= 65536 && nblocks <= 0xFFFFFFFFull; }
inline bool lzf_call_valid(size_t block_bytes, size_t) { return block_bytes != 0 && block_bytes <= 65536; }

enum class Target : uint8_t { caller, lanes_side, vtab_side }; // the stream a stage is enqueued on
enum class SidePool : uint8_t { normal, greatest };            // the pool of hardware queues a side stream comes from
struct Stage {
    bool on = false;
    uint32_t grid = 0, lds = 0; // workgroups of 64 threads; dynamic LDS bytes
    Target stream = Target::caller;
};
constexpr uint32_t kNoMax = 0xFFFFFFFFu;

struct Lz4Plan {
    bool staged = false;          // blocks parsed from an LDS copy
    // scan: span + stream (what does not fill a span), or the generic one
    Stage scan_span, scan_stream, scan_generic;
    Lz4ScanSpan scan_span_kernel = Lz4ScanSpan::aligned;
    uint32_t lg = 0, nspans = 0;  // span scan: log2(n / 4 KiB), spans of 64 KiB
    size_t done = 0, rest = 0;    // blocks the span scan covers; blocks of the stream scan
    bool stop_after_scan = false; // CW_LZ4_MODE=scan
    // lane-per-block parser: one of lz4_lanes_kernel<>, lz4_lanes_ring_auto_kernel, lz4_lanes_ring_kernel<>
    enum class LanesForm : uint8_t { table, ring_auto, ring };
    Stage lanes;
    LanesForm lanes_form = LanesForm::table;
    Lz4Lanes lanes_kernel = Lz4Lanes::tagged;
    Lz4Ring ring_kernel = Lz4Ring::k1;
    SidePool lanes_pool = SidePool::normal;
    uint32_t lmin = 0, reserve = 0, reserve_wide = 0, wide_from = 0, lane_leave = 0;
    size_t lane_tab_bytes = 0;
    // register-table parser
    Stage vtab;
    Lz4Vtab vtab_kernel = Lz4Vtab::gen3;
    SidePool vtab_pool = SidePool::normal;
    uint32_t vmin = 0, vmax = kNoMax, vres = 0;
    int gen = 0;
    // the parser on the caller's stream: the LDS-table scalar-thread parser or a wavefront parser
    Stage ltab, parse;
    Lz4Parse parse_kernel = Lz4Parse::global;
    uint32_t force_redo = 0;
    // redo pass (CW_LZ4_MODE=cut: the only parser, over the scan's queue)
    Stage redo;
    Lz4Blocks redo_kernel = Lz4Blocks::global;
    bool cut_only = false;
    size_t queue_bytes = 0, queue_min_bytes = 0; // counters + two queues; what the first call on a stream reserves at least
};

struct LzfPlan {
    enum class Path : uint8_t { rounds, parse, cut }; // link/chain rounds (+ lanes); the table parser; the write/read-back kernel alone
    Path path = Path::rounds;
    // the table parser and the final pass
    Stage parse, blocks;
    LzfParse parse_kernel = LzfParse::global;
    uint32_t in_lds = 0, force_redo = 0, blocks_pass = 1;
    // rounds
    bool big = false, beside = false; // blocks beyond the LDS-resident links; lanes beside the rounds
    uint32_t n2 = 0;                  // bytes per block in the link array / 2
    size_t chunk = 0, hb_chunk = 0;   // blocks per round; per round of the hand-back pass
    bool rounds_over_batch = false, rounds_over_handback = false;
    LzfChain chain_kernel = LzfChain::small;
    uint32_t links_lds = 0, chain_lds = 0;
    size_t per_cu = 0, st_cu = 0;     // chain workgroups per CU: wavefront-wide forms; the scalar-thread form
    uint32_t spin_cap = 0;
    Stage lanes;
    LzfLanes lanes_kernel = LzfLanes::plain;
    SidePool lanes_pool = SidePool::normal;
    uint32_t lane_reserve = 0;
    size_t links_bytes = 0, lane_tab_bytes = 0, handback_bytes = 0;
};

// lanes_allowed = false: the plan of a call whose lane tables could not be reserved -- what the launch goes on with after that
Lz4Plan lz4_plan(const CodecCall &call, const Knobs &kn, bool lanes_allowed = true);
LzfPlan lzf_plan(const CodecCall &call, const Knobs &kn, bool lanes_allowed = true);

// ---- hashes -------------------------------------------------------------------------------------------------------------------------
// hash_plan is pure like the two above: which instantiation a cw_dev_hash-like call runs, whether a Skein call is cut into sliced
// launches, and then every launch's steps.  skein_launch / sha256_launch (skein_kernels.hip, sha256_kernel.hip) enqueue what it says;
// cw_hash_plan_describe prints it without a device.
enum class SkeinForm : uint8_t { steps, ragged, lines }; // skein_blocks_kernel<NW, A, false> / <NW, A, true> / skein_lines_kernel<NW, A>
// (defined beside the kernels' tables: skein_kernels.hip, sha256_kernel.hip)
const char *skein_kernel_name(int state_words, SkeinForm form, bool aligned);
const char *skein_slice_kernel_name(int state_words, bool interior);
const char *sha256_kernel_name(bool aligned, bool ragged);

constexpr size_t kHashThreads = 64;        // lanes (= blocks) per workgroup of every hash kernel (CW_SKEIN_THREADS)
constexpr uint32_t kSkeinSlices = 8;       // launches of a sliced hash unless CW_SKEIN_NSLICES says otherwise
constexpr size_t kSlicedMinBlocks = 4096;  // sliced launches: from this many blocks on ...
constexpr size_t kSlicedMinSteps = 256;    // ... and this many steps (message steps + the output transform) per block

struct HashCall {
    int state_words;       // 8 = Skein-512, 4 = Skein-256, 0 = SHA-256
    size_t block_bytes, nblocks;
    unsigned src_mis16;    // (src | src_stride) & 15
    unsigned digest_mis16; // digests & 15
    bool may_slice;        // the caller lets long Skein messages go out in sliced launches (all but HashOffload)
};
inline HashCall hash_call(int state_words, const void *src, size_t block_bytes, size_t src_stride, size_t nblocks, const void *digests,
                          bool may_slice)
{
    return {state_words, block_bytes, nblocks, (unsigned)((reinterpret_cast<uintptr_t>(src) | src_stride) & 15),
            (unsigned)(reinterpret_cast<uintptr_t>(digests) & 15), may_slice};
}
// one launch of a sliced hash: steps [begin, end) of every block.  interior: the steps and the line prefetched behind them all lie
// inside the message (skein_slice_kernel<8, true, true>)
struct SkeinSlice { size_t begin, end; bool interior; };
struct HashPlan {
    int state_words = 0;
    uint32_t grid = 0;                   // workgroups of kHashThreads lanes, the same for every launch of the call
    bool aligned = false, ragged = false; // 16-byte aligned source; block_bytes is 0 or no multiple of the step
    SkeinForm form = SkeinForm::lines;   // Skein, one launch
    bool sliced = false;
    size_t total = 0, slice_steps = 0;   // sliced: steps per block (message steps + output transform); steps per launch
    size_t state_bytes = 0;              // sliced: the chaining values between the launches
    std::vector<SkeinSlice> slices;      // sliced: the launches, in order
};
HashPlan hash_plan(const HashCall &call, const Knobs &kn);

// the kernels of a plan as cw_profile_kernels reports them (at most 319 characters)
struct Description { char text[320]; };
Description describe(const Lz4Plan &p);
Description describe(const LzfPlan &p);
Description describe(const HashPlan &p);
// one `key=value` line per field, in the order of the structs
std::string dump(const Lz4Plan &p);
std::string dump(const LzfPlan &p);
// one `slice=begin..end interior=0|1` line per launch of a sliced hash, nothing otherwise
std::string dump(const HashPlan &p);

} // namespace cw
