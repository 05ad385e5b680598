// launch_plan.cpp -- the launch policy of the LZ4 and LZF compressors and of the hashes (launch_plan.h): thresholds, their
// measurements, and the description and dump of a plan.  Host code only.
#include "launch_plan.h"

#include <stdarg.h>
#include <stdio.h>
#include <string.h>

namespace cw {

namespace {

// ---- LZ4 ----------------------------------------------------------------------------------------------------------------------------
// blocks > 4 KiB: below kLaneMidBlocks queued blocks the wavefront-per-block parser's 13-14 GB/s win; [mid, wide): lanes with two
// positions per iteration (every lane holds one block: latency regime), from kLaneWideBlocks on one (random-line regime); lz4_plan
// Round 3: below kLaneMidBlocks the two scalar-thread parsers (table in vector registers / in LDS, lz4_vtab_kernel.hip) win (corpus, 64 KiB: 12 Ki /
// 16 Ki / 20 Ki blocks 23.9 / 27.3 / 29.0 GB/s against the lanes' 15.4 / 19.5 / ~22), so the lanes start later than in round 2 (10,240), and from there on
// they run BESIDE those two: in the one-block-per-lane regime there are no lanes for kLaneLeave blocks of the queue and the lanes leave kLaneShare
// blocks (two thirds of a small call) alone; from kLaneWideBlocks on they leave kLaneShareWide.  One launch for both regimes (lz4_lanes_ring_auto_kernel).
constexpr uint32_t kLaneMidBlocks = 22528, kLaneWideBlocks = 98304; // (blocks <= 32 KiB: higher lower thresholds, lz4_plan)
constexpr bool kLtabDefault = true; // corpus, 64 KiB, alone on the queue: 8 Ki / 16 Ki / 48 Ki blocks 16.1 / 17.5 / 18.6 GB/s against the wavefront parser's 14.6 / 15.8 / 16.6; beside the register form 23.3 / 26.7 against 22.2 / 25.4
constexpr size_t kLaneLeave = 18432;   // blocks > 4 KiB, calls below kLaneWideBlocks: this many blocks get no lane (lz4_plan has the measurements)
constexpr uint32_t kLaneShare = 24576, kLaneShareWide = 32768;     // blocks of the queue the lanes leave to the other parsers (K = 2 / K = 1 regime); K = 2: at most two thirds of
                                                                   // the call -- since the lanes no longer take the whole queue at once (kLaneLeave) they pay from 22 Ki blocks on: corpus,
                                                                   // 64 KiB, 20 Ki / 24 Ki / 28 Ki blocks without lanes 29.0 / 29.4 / 29.8 GB/s, with 28.2 / 31.7 / 35.3 (16 Ki left);
                                                                   // 56 Ki / 72 Ki blocks with 16 Ki left 39.9-43.9 / 43.2-48.1, with 24 Ki 47.1 / 48.2-48.7
constexpr uint32_t kLaneMinSmall = 61440;  // LDS-staged blocks: lanes beside the LDS-resident parser from 60 Ki blocks on (64 Ki blocks of text: 28.5 against 25.7 GB/s)

// ---- LZF ----------------------------------------------------------------------------------------------------------------------------
// A lane needs ~66 ms for a 64 KiB block of text however few lanes there are, the link/chain kernels run at 8.5 GB/s: the lanes win
// from ~9 Ki compressible blocks on (text, 64 KiB, 12 Ki / 16 Ki / 20 Ki / 24 Ki blocks: 13.2 / 16.3 / 13.6 / 15.2 GB/s against 8.5; the dip
// is the second wavefront on some CUs' SIMDs).  A batch that is a third noise or more goes back to the chain kernels anyway.
constexpr uint32_t kLzfLaneMinBlocks = 12288;
constexpr uint32_t kLzfLaneMinSmall = 28672;  // blocks <= 4 KiB: lanes beside the rounds from 28 Ki blocks on (text, 32 Ki / 40 Ki / 64 Ki blocks: 16.1 / 19.5 / 21 against 13.5 GB/s)
constexpr size_t kLzfBesideRound = 16384;     // ... in rounds of 16 Ki blocks, the last 16 Ki unclaimed blocks left to the rounds.  4 KiB blocks, text /
                                              // 50 % noise / noise, GB/s -- 1 Mi blocks: rounds of 8 Ki 29.8 / 24.7 / 52.9, 16 Ki 33.1 / 29.0 / 57.7,
                                              // 32 Ki 32.6 / 30.9 / 59.2; 96 Ki blocks: 25.6 / 36.3 / 50.5, 26.2 / 39.3 / 53.6, 23.1 / 36.4 / 55.0
// blocks > 16 KiB: lanes beside the scalar-thread rounds from 52 Ki blocks on; from 96 Ki blocks on rounds of 8 Ki blocks and as many left to the rounds, below
// (every lane gets one block; the rounds get what they manage in that time) rounds of 4 Ki and 12 Ki blocks left.  Corpus, 64 KiB, lanes alone -> beside:
// 48 Ki blocks 27.0 -> 26.3-27.6 (not used), 56 Ki 27.0 -> 29.1, 64 Ki 27.3 -> 29.0, 80 Ki 26.4 -> 34.8, 128 Ki 27.3 -> 31.0, 256 Ki 29.4 -> 35.2 GB/s
constexpr size_t kLzfBigBesideMin = 53248, kLzfBigBesideWide = 98304, kLzfBigBesideRound = 8192, kLzfBigBesideRoundMid = 4096, kLzfBigBesideReserveMid = 12288;
constexpr uint32_t kLzfBesideReserve = 16384, kLzfBesideReserveFew = 8192; // blocks left to the rounds; below 48 Ki blocks (32 Ki blocks: 16.1 against 13.2 GB/s with 16 Ki)

template <class T>
T at_most(T v, T cap) { return v < cap ? v : cap; }

} // namespace

Lz4Plan lz4_plan(const CodecCall &call, const Knobs &kn, bool lanes_allowed)
{
    Lz4Plan p;
    const uint32_t n = call.n;
    const size_t nblocks = call.nblocks;
    // counters[8] + two queues of as many entries as the call has blocks (the first call on a stream: at least 4096)
    p.queue_bytes = (2 * nblocks + 8) * sizeof(uint32_t);
    p.queue_min_bytes = (2 * 4096 + 8) * sizeof(uint32_t);
    // CW_LZ4_STAGE_MAX (profiling knob): largest block parsed from an LDS copy
    // measured on text: 4 KiB 26.0 (staged) vs 22.4 GB/s (global); 8 KiB 18.1 vs 20.6; 16 KiB 11.5 vs 18.7 -- blocks per CU win
    const uint32_t stage_max = kn.lz4_stage_max ? (uint32_t)*kn.lz4_stage_max : 4096u;
    const bool staged = p.staged = n <= (stage_max < kStageMax ? stage_max : kStageMax);
    // staged bytes are read as aligned dwords: a size that is not a multiple of 4 gets 16 bytes of slack behind it
    uint32_t lds = kTabBytes + (staged ? ((n + 15u) & ~15u) + (n % 4 ? 16u : 0u) : 0u);

    // scan: one wavefront per workgroup, 32 KiB of LDS each -> 5 per CU; the grid-stride loop walks the rest
    // CW_LZ4_MODE=generic forces the gather-based scan (profiling knob)
    const bool streamable = call.src_n_mis16 == 0 && kn.lz4_mode != Lz4Mode::generic;
    if (streamable) {
        // CW_SCAN_WPC: scan wavefronts per CU (profiling knob; 4 = all that fit)
        const size_t wpc = kn.scan_wpc ? (size_t)kn.scan_wpc : 4;
        // power-of-two sizes 4 KiB .. 64 KiB go through the span kernel, 64 KiB of whole blocks per pull; what does not
        // fill a span (and every other size) through the per-block streaming kernel.  CW_LZ4_MODE=stream: the latter only.
        const bool pow2 = n >= kChunk && (n & (n - 1)) == 0 && kn.lz4_mode != Lz4Mode::stream;
        while (pow2 && (kChunk << p.lg) < n) p.lg++;
        const size_t run = pow2 ? (size_t)(16u >> p.lg) : 1;
        const size_t nspans = pow2 ? nblocks / run : 0;
        p.nspans = (uint32_t)nspans;
        p.done = nspans * run;
        if (nspans) {
            // 40 KiB of LDS each -> at most 4 per CU
            // 16-byte aligned slots: the literal runs go out as aligned lines (any other slot alignment: misaligned 16-byte stores)
            p.scan_span = {true, (uint32_t)at_most(nspans, 256 * wpc), 0, Target::caller};
            p.scan_span_kernel = call.dst_mis16 == 0 ? Lz4ScanSpan::aligned : Lz4ScanSpan::unaligned;
        }
        if (p.done < nblocks) {
            p.rest = nblocks - p.done;
            p.scan_stream = {true, (uint32_t)at_most(p.rest, 256 * wpc), 0, Target::caller};
        }
    } else {
        p.scan_generic = {true, (uint32_t)at_most<size_t>(nblocks, 256 * 5), 0, Target::caller};
    }
    // CW_LZ4_MODE=scan stops after the scan kernel (queued blocks keep sizes[i] = 0xFFFFFFFF): a profiling knob
    if ((p.stop_after_scan = kn.lz4_mode == Lz4Mode::scan)) return p;

    // parse: queued blocks only; LDS admits 160 KiB / lds workgroups per CU
    // CW_LZ4_PARSE=fp: blocks read from global memory go through the fingerprint parser (20 KiB of LDS, 8 blocks per CU).
    // Measured on text at 64 KiB: 11.9 GB/s against 14.2 GB/s for the second generation with its 10 blocks per CU -- both
    // are bound by the instruction latency of one sequence's serial chain (tools/parse_stamp.hip), not by candidate
    // traffic, so the extra blocks win; the second generation stays the default.
    const bool use_fp = !staged && kn.lz4_parse_fp;
    const int headw = kn.lz4_headw.value_or(16); // CW_LZ4_HEADW: head batch width of the fingerprint parser (profiling knob: 8, 16, 32)
    if (use_fp) lds = kTabBytes + kFpBytes;
    const size_t per_cu = (160u * 1024u) / lds ? (160u * 1024u) / lds : 1;
    // Large batches: the lane-per-block parser.  Two regimes:
    //  * blocks read from global memory (> 4 KiB), from kLaneMidBlocks queued blocks on: the lanes take the whole queue, the
    //    wavefront-per-block parser only what they leave (running it beside the lanes gains nothing there: both end up waiting
    //    for the same memory system -- 33.1 vs 34.2 GB/s);
    //  * LDS-staged blocks (<= 4 KiB), from kLaneMinSmall blocks on: the lanes run BESIDE the LDS-resident parser on a second
    //    stream, both pulling from the scan's queue -- one is bound by LDS capacity and its chain latency, the other by random
    //    memory accesses, and the rates add (4 KiB text: 26.2 -> 40.1 GB/s).
    // The kernel looks at the queue length on the device and leaves everything to the wavefront parser below the threshold.
    // CW_LZ4_LANES=0 switches it off, =N sets the threshold (1: every queued block, in the tests); CW_LANES_WPC = its
    // wavefronts per CU, CW_LANES_CONCURRENT=0|1 forces the regime, CW_LANES_RESERVE the blocks left to the wavefronts.
    // measured break-even with the wavefront parser on text (GB/s, wavefront parser / lanes): 64 KiB 16 Ki blocks 14.2 / 20.9; 16 KiB 16 Ki
    // blocks 18.3 / 17.4, 24 Ki 18.3 / 20.7; 8 KiB 24 Ki blocks 20.9 / 18.5, 32 Ki 20.4 / 22.7 (on small blocks the wavefront parser
    // is faster and a lane slower per byte: every block starts on an empty table, and has one to zero)
    const uint32_t lane_min = kn.lz4_lanes ? (uint32_t)*kn.lz4_lanes
                              : staged ? kLaneMinSmall : n > 32768 ? kLaneMidBlocks : n > 16384 ? 40960u : n > 8192 ? 61440u : 98304u;
    // (16 KiB blocks: the register-table + wavefront parsers 25.7 / 27.9 / 29.3 GB/s at 16 Ki / 32 Ki / 64 Ki blocks against the lanes' 19.5 / 25.0 / 30.1;
    //  8 KiB blocks: 25.5 / 28.8 / 30.0 at 16 Ki / 48 Ki / 96 Ki blocks against 21.4 / 21.3 / 30.3)
    // CW_LZ4_LANES_RING: 0 = input from global memory (lz4_lanes_kernel); 1, 2, 4, 8 = the ring form with that many positions per
    // iteration whatever the queue's length.  Unset: the ring form, K chosen ON THE DEVICE by the queue's length -- two launches,
    // each of which returns at once unless the length lies in its range:
    //   [kLaneMidBlocks, kLaneWideBlocks)  K = 2.  Every lane holds one block and the call lasts as long as one lane needs for
    //       one block: latency, not lines, so the second position's table entry and candidate requested together with the
    //       first's pay (text, 64 KiB, 16 Ki / 24 Ki / 32 Ki blocks: 21.1 / 26.0 / 29.9 GB/s against 16.4 / 21.0 / 27.0 with K = 1
    //       and 14.2 for the wavefront parser, which keeps everything below ~10 Ki blocks: 8 Ki blocks 13.5 against 11.8);
    //   [kLaneWideBlocks, ...)             K = 1.  Enough chains to be bound by the memory system's random lines, where the
    //       lines of the speculative second position only cost (64 Ki blocks: 38.3 against 35.6 GB/s).
    //   K = 4 / 8 are never better (16 Ki blocks: 20.0 / 16.4 GB/s): each position adds instructions to every iteration.
    const int lanes_ring = kn.lz4_lanes_ring.value_or(-1); // -1: by queue length
    // CW_LANES_CONCURRENT=0: one after the other on the caller's stream (the lanes take the whole queue); default: side by side
    const bool lanes_concurrent = kn.lanes_concurrent.value_or(true);
    bool lanes_beside = false;
    if (lanes_allowed && !use_fp && lane_min && nblocks >= lane_min && n >= 64) {
        const size_t lwpc = kn.lanes_wpc ? (size_t)kn.lanes_wpc : 8;
        size_t lgrid = (nblocks + 63) / 64, lcap = 256 * lwpc;
        // LDS-staged blocks, lanes beside the wavefront parser: lanes for about half of the blocks (2 .. 8 wavefronts per CU).  With
        // fewer lanes each is faster (less traffic per probe in flight), and a batch of 64 Ki .. 256 Ki blocks is over before a lane
        // has parsed more than two or three (text, 4 KiB, 80 Ki / 128 Ki / 256 Ki blocks: 2 wavefronts per CU 34.4 / 33.6 / 35.6 GB/s,
        // 4: 27.7 / 39.6 / 36.5, 8: 24.9 / 26.0 / 39.0-41.0; the wavefront parser alone 25.8)
        if (staged && !kn.lanes_wpc) lcap = nblocks / 128 < 512 ? 512 : nblocks / 128 > 2048 ? 2048 : nblocks / 128;
        if (lgrid > lcap) lgrid = lcap;
        // blocks > 4 KiB, lanes beside the on-chip parsers, calls below kLaneWideBlocks (every lane gets ONE block and the call lasts as long as a lane
        // needs for it, 60-110 ms depending on how many lanes run): no lanes for the ~18 Ki blocks the two on-chip parsers get through in that time.
        // A grid with a lane for every block takes the whole queue in its first microseconds (every lane passes the "leave `reserve` blocks" check
        // before any has drawn) and the on-chip parsers get nothing: 64 Ki blocks, the lanes' kernel 110 ms, the two scalar-thread kernels beside
        // it 15 ms each.  Corpus, 64 KiB, share of the blocks with a lane 100 / 85 / 72 / 60 / 50 %, GB/s: 32 Ki blocks 32.5 / 33.5 / 33.0 / 35.2 / 37.6,
        // 48 Ki 42.5 / 43.2 / 44.1 / 46.8 / 39.2, 64 Ki 41.1 / 42.9 / 47.3 / 45.2 / 42.1 (best: all but 16-19 Ki blocks); 128 Ki and 256 Ki blocks
        // (lanes take several blocks each, the reserve works): 47.8 / 42.6 / 46.5 / 44.6 / 44.7 and 47.6-49.1, no trend.
        // (the kernel applies the same rule to the queue's length, which may be shorter than the call: blocks the scan has dealt with are not queued)
        // CW_LANES_LEAVE: blocks of such a call that get no lane (profiling knob; 0 = a lane for every block)
        const size_t leave = kn.lanes_leave ? (size_t)*kn.lanes_leave : kLaneLeave;
        if (!staged && leave && lanes_concurrent && lane_min > 1) {
            p.lane_leave = (uint32_t)leave;
            const size_t want = nblocks > leave + 4096 ? (nblocks - leave + 63) / 64 : 64;
            if (nblocks < kLaneWideBlocks && lgrid > want) lgrid = want;
        }
        // (entries of 4 bytes for blocks > 4 KiB); up to 4 GiB: a nearly full device does without the lanes instead of failing the call
        p.lane_tab_bytes = lgrid * 64 * (size_t)kTabBytes * 2;
        lanes_beside = lanes_concurrent;
        p.lmin = lane_min;
        if (lanes_beside) {
            // The lanes' and the register-table parser's streams come from the HIGH-PRIORITY pool of hardware queues (CW_SIDE_PRIO=0: the normal one,
            // =1: the lanes' only).  HIP multiplexes its streams onto four hardware queues per priority level, and kernels of different streams
            // that land on one queue run one after the other.  A device-resident call has four streams and is not affected; the host pipeline has
            // three slots with four streams each plus two for copies, and its timeline (rocprofv3 --kernel-trace) showed a chunk's two scalar-thread
            // kernels starting the moment ITS OWN lanes kernel had ended, 108 ms late.  With the side streams in another pool a chunk's kernels
            // no longer share a queue with each other: host path over the corpus 20.5-21.0 -> 24.0-24.3 GB/s (GPU_MAX_HW_QUEUES=8 on top: 24.7-24.9);
            // the device-resident legs and the headline are unchanged (16 GiB corpus leg 44-48 -> 49.6).
            p.lanes_pool = kn.side_prio != SidePrio::none ? SidePool::greatest : SidePool::normal;
            // what the wavefront parser gets through while a lane parses its last block: 4 KiB text, 1 Mi blocks: 8 Ki..40 Ki 40-43 GB/s, 48 Ki 39.8;
            // 256 Ki blocks: 16 Ki / 28 Ki / 40 Ki 37.4 / 39.0 / 41.0
            // blocks > 4 KiB (round 3; corpus, 64 KiB, lanes alone -> lanes beside the other two, GB/s): two positions per iteration, 32 Ki blocks
            // 29.4 -> 31.0 (reserve 24 Ki), 48 Ki 34.0 -> 40.7 (16-24 Ki), 64 Ki 37.2 -> 40.6 (32 Ki); one position: 128 Ki 44.9 -> 48.3 (32 Ki), 256 Ki 42.8 -> 46.7
            p.reserve = kn.lanes_reserve ? (uint32_t)kn.lanes_reserve : (staged ? 32768u : kLaneShare);
            if (!staged && !kn.lanes_reserve && p.reserve > nblocks / 3 * 2) p.reserve = (uint32_t)(nblocks / 3 * 2);
            p.reserve_wide = kn.lanes_reserve ? (uint32_t)kn.lanes_reserve : kLaneShareWide;
            if (lane_min > 1 && p.lmin < p.reserve + p.reserve / 4) p.lmin = p.reserve + p.reserve / 4; // (CW_LZ4_LANES=1 in the tests: no reserve)
            if (lane_min == 1) p.reserve = p.reserve_wide = 0;
        }
        p.lanes = {true, (uint32_t)lgrid, 0, lanes_beside ? Target::lanes_side : Target::caller};
        if (n <= 4096) {
            p.lanes_form = Lz4Plan::LanesForm::table;
            p.lanes_kernel = Lz4Lanes::tagged;
        } else if (lanes_ring < 0) {
            // ONE launch, the number of positions per iteration chosen on the device by the queue's length (lz4_lanes_ring_auto_kernel)
            p.lanes_form = Lz4Plan::LanesForm::ring_auto;
            p.wide_from = p.lmin < kLaneWideBlocks ? kLaneWideBlocks : p.lmin;
        } else if (lanes_ring == 1 || lanes_ring == 2 || lanes_ring == 4 || lanes_ring == 8) {
            p.lanes_form = Lz4Plan::LanesForm::ring;
            p.ring_kernel = lanes_ring == 1 ? Lz4Ring::k1 : lanes_ring == 2 ? Lz4Ring::k2 : lanes_ring == 4 ? Lz4Ring::k4 : Lz4Ring::k8;
        } else {
            // CW_LZ4_LANES_FP=0 (profiling knob): 16-bit table entries without fingerprints for blocks > 4 KiB
            p.lanes_form = Lz4Plan::LanesForm::table;
            p.lanes_kernel = kn.lz4_lanes_fp ? Lz4Lanes::fp : Lz4Lanes::plain;
        }
    }
    // The register-table parser (lz4_vtab_kernel.hip): 16 more chains per CU than the LDS admits, no table traffic.  It runs BESIDE the
    // wavefront parser on a second stream, both pulling from the scan's queue, whenever the lanes do not take the whole queue
    // (text, 64 KiB blocks, wavefront parser alone -> both: 3,233 blocks 11.8 -> 15.7 GB/s, 8 Ki 13.3 -> 21.6, 16 Ki 24.5 against the
    // lanes' 19.5; beside the lanes in their random-line regime it gains nothing -- they keep the memory system busy and its
    // candidate fetches wait).  CW_LZ4_VTAB: 0 = off, 1 = on the caller's stream AHEAD of the wavefront parser (it takes the whole
    // queue: tests), 2 = beside (default); CW_VTAB_MIN / CW_VTAB_MAX = queue lengths between which it runs (checked on the device),
    // CW_VTAB_RESERVE = blocks it leaves to the others, CW_VTAB_WPC = its wavefronts per CU (at most 16), CW_VTAB_GEN = kernel generation.
    const int vt_mode = kn.lz4_vtab.value_or(2);
    // CW_LZ4_MODE=cut parses with the first-generation (write/read-back) kernel only (profiling knob)
    const bool cut_only = p.cut_only = kn.lz4_mode == Lz4Mode::cut;
    if (vt_mode > 0 && !use_fp && !cut_only && n >= 64 && nblocks >= 64 && call.src_mis4 == 0) { // (the scalar loads are dword loads)
        // LDS-staged blocks: a small queue is the LDS-resident parser's (4 Ki blocks of 4 KiB: 19.4 GB/s alone against 14.5 with the register-table
        // parser's 4,096 wavefronts taking a block each; 16 Ki blocks 23.8 -> 24.5, 32 Ki 25.1 -> 28.0, 51,728 25.6 -> 29.5)
        p.vmin = kn.vtab_min ? (uint32_t)*kn.vtab_min : staged ? 12288u : 1u;
        p.vres = kn.vtab_reserve ? (uint32_t)*kn.vtab_reserve : 0u;
        // lanes that take the whole queue (blocks > 4 KiB) start at lane_min queued blocks: the register-table parser stays below
        p.vmax = kn.vtab_max ? (uint32_t)*kn.vtab_max : (p.lanes.on && !lanes_beside ? lane_min : kNoMax);
        // grid: as many single-wavefront workgroups as the register file admits (128 VGPRs -> 4 per SIMD, 16 per CU), at most one per queued block
        const size_t vwpc = kn.vtab_wpc ? (size_t)kn.vtab_wpc : 16;
        p.vtab = {true, (uint32_t)at_most(256 * vwpc, nblocks), 0, vt_mode == 2 ? Target::vtab_side : Target::caller};
        if (vt_mode == 2) p.vtab_pool = kn.side_prio == SidePrio::both ? SidePool::greatest : SidePool::normal;
        // gen (CW_VTAB_GEN): 2 = batches of four items (vector loads), 3 = the scalar chain with the VALU's help.  Default by measurement (GB/s alone,
        // 16 wavefronts per CU; (1) = the all-scalar first form, removed): text, 64 KiB blocks, 8 Ki blocks 18.4 (1) / 13.7 (2) / 20.8 (3),
        // 3,233 blocks 13.6 / 11.3 / 17.1; corpus, 4 KiB blocks 15.4-16.0 (1) against 17.8-17.9 (2)
        p.gen = kn.vtab_gen.value_or(0);
        if (p.gen != 2 && p.gen != 3) p.gen = n <= 4096 ? 2 : 3;
        p.vtab_kernel = p.gen == 3 ? Lz4Vtab::gen3 : Lz4Vtab::gen2;
    }
    const size_t pwpc = kn.parse_wpc ? (size_t)kn.parse_wpc : 10; // CW_PARSE_WPC: parse wavefronts per CU (profiling knob; default: all the LDS admits)
    const uint32_t grid = (uint32_t)at_most(nblocks, 256 * at_most(per_cu, pwpc));
    // CW_LZ_FORCE_REDO=1: the exchange kernel hands every block back, as if its lane-order check had failed (test knob)
    p.force_redo = kn.force_redo ? 1u : 0u;
    if (!cut_only) {
        // blocks read from global memory: the scalar-thread parser with its table in LDS (lz4_vtab3_kernel<true>) in the place of the round-2
        // wavefront parser; CW_LZ4_LTAB=0 keeps the latter (and the forced-redo test knob and unaligned sources need it)
        const bool use_ltab = !staged && !use_fp && !p.force_redo && n >= 64 && call.src_mis4 == 0 &&
                              (kn.lz4_ltab ? *kn.lz4_ltab != 0 : kLtabDefault);
        if (use_ltab) {
            // ten single-wavefront workgroups per CU at most (16 KiB of LDS each)
            p.ltab = {true, (uint32_t)at_most(256 * (pwpc < 10 ? pwpc : 10), nblocks), kTabBytes, Target::caller};
        } else {
            p.parse = {true, grid, lds, Target::caller};
            p.parse_kernel = staged ? Lz4Parse::staged : !use_fp ? Lz4Parse::global : headw == 32 ? Lz4Parse::fp32 : headw == 8 ? Lz4Parse::fp8 : Lz4Parse::fp16;
        }
    }
    // blocks the exchange-based parser handed back (none, unless the LDS ever applies lanes out of order)
    p.redo = {true, grid, lds, Target::caller};
    p.redo_kernel = staged ? Lz4Blocks::staged : Lz4Blocks::global;
    return p;
}

LzfPlan lzf_plan(const CodecCall &call, const Knobs &kn, bool lanes_allowed)
{
    LzfPlan p;
    const uint32_t n = call.n;
    const size_t nblocks = call.nblocks;
    p.in_lds = n <= kInLdsMax ? 1u : 0u;
    const uint32_t lds = kLzfTabBytes + (p.in_lds ? ((n + 15u) & ~15u) + 16u : 0u); // 16 bytes of slack for dword reads
    const uint32_t grid = (uint32_t)at_most<size_t>(nblocks, 256); // the 128 KiB table admits one workgroup per CU
    // CW_LZF_MODE=cut: write/read-back kernel only; =table: exchange kernel with the 128 KiB table also for small blocks
    const bool cut_only = kn.lzf_mode == LzfMode::cut, table_only = kn.lzf_mode == LzfMode::table;
    p.force_redo = kn.force_redo ? 1u : 0u; // CW_LZ_FORCE_REDO: test knob, see lz4_plan
    p.blocks = {true, grid, lds, Target::caller};
    if (cut_only || table_only || n < 16) {
        p.path = cut_only ? LzfPlan::Path::cut : LzfPlan::Path::parse;
        p.blocks_pass = cut_only ? 0u : 1u;
        if (!cut_only) {
            p.parse = {true, grid, lds, Target::caller};
            p.parse_kernel = p.in_lds ? LzfParse::staged : LzfParse::global;
        }
        return p;
    }
    // links for a round of blocks, then the chain parser over that round
    // CW_LZF_LDS_MAX (profiling knob): largest block parsed from LDS-resident links
    // measured (text): 4 KiB 13.2 (LDS) vs 12.4 GB/s (global links); 8 KiB 7.2 vs 10.6; 16 KiB 3.7 vs 9.3 -- blocks per CU win
    const uint32_t lds_max = kn.lzf_lds_max ? (uint32_t)kn.lzf_lds_max : 4096u;
    const bool big = p.big = n > (lds_max < kChainMax ? lds_max : kChainMax);
    const uint32_t n2 = p.n2 = (n + 63u) & ~63u;
    const size_t ws_bytes = big ? (size_t)1 << 30 : (size_t)256 << 20; // links per round
    // (blocks of 4-8 KiB: the chain kernels win up to ~18 Ki blocks -- text, 8 KiB, 16 Ki blocks 11.0 against 10.6 GB/s, 24 Ki 11.3 / 13.0)
    const size_t lane_min = kn.lzf_lanes ? (size_t)*kn.lzf_lanes : (big ? (n > 8192 ? kLzfLaneMinBlocks : 18432u) : kLzfLaneMinSmall);
    // (what the call asks for: its rounds and link array are sized by it even when the lane tables cannot be had, lanes_allowed == false)
    const bool lanes_wanted = lane_min && nblocks >= lane_min;
    // blocks > 4 KiB: the scalar-thread form of the chain parser (CW_LZF_STHREAD=0: the wavefront-wide one); needs dword-aligned blocks
    const size_t st_wpc = kn.lzf_st_wpc ? (size_t)kn.lzf_st_wpc : 20;
    const bool sthread = big && kn.lzf_sthread && call.src_mis4 == 0;
    // lanes BESIDE the rounds: blocks <= 4 KiB always; larger blocks from kLzfBigBesideMin blocks on, and only with the scalar-thread
    // parser in the rounds (with the wavefront-wide chain kernel in the rounds: 256 Ki blocks 27.7 -> 27.7 GB/s)
    const bool big_beside = sthread && n > 16384 && nblocks >= kLzfBigBesideMin;
    const bool beside_wanted = lanes_wanted && kn.lanes_concurrent.value_or(!big || big_beside);
    // CW_LZF_ROUND (test knob): blocks per round (many rounds on small data)
    const size_t round_max = ws_bytes / (2 * (size_t)n2); // blocks per round that the link workspace admits
    const size_t chunk_cap = kn.lzf_round ? (size_t)kn.lzf_round : beside_wanted ? (big ? (nblocks < kLzfBigBesideWide ? kLzfBigBesideRoundMid : kLzfBigBesideRound) : kLzfBesideRound) : round_max;
    p.chunk = at_most(nblocks, at_most(chunk_cap, round_max));
    // Large batches: the lane-per-block parser (CW_LZF_LANES=0 off, =N threshold, 1 = every block, in the tests; CW_LANES_WPC
    // wavefronts per CU).  Blocks > 4 KiB from kLzfLaneMinBlocks on: the lanes take the whole batch.  Blocks that fit the
    // LDS-resident chain parser, from kLzfLaneMinSmall on: the lanes run BESIDE the link/chain rounds on a second stream,
    // pulling from the top of the batch while the rounds climb from the bottom (LaneShare) -- one side is bound by LDS
    // capacity and chain latency, the other by random memory accesses.
    const size_t want_reserve = kn.lanes_reserve ? (size_t)kn.lanes_reserve : big ? (nblocks < kLzfBigBesideWide ? kLzfBigBesideReserveMid : kLzfBigBesideRound) : nblocks < 49152 ? kLzfBesideReserveFew : kLzfBesideReserve;
    p.hb_chunk = at_most(nblocks, round_max); // rounds of the hand-back pass
    p.links_bytes = (lanes_wanted && p.hb_chunk > p.chunk ? p.hb_chunk : p.chunk) * n2 * sizeof(uint16_t);
    const bool use_lanes = lanes_wanted && lanes_allowed;
    p.beside = beside_wanted && lanes_allowed;
    if (use_lanes) {
        const size_t lwpc = kn.lanes_wpc ? (size_t)kn.lanes_wpc : 4;
        size_t lgrid = at_most((nblocks + 63) / 64, 256 * lwpc); // workgroups of the lane-per-block kernel
        if (p.beside && lgrid * 64 + want_reserve > nblocks) lgrid = nblocks > want_reserve + 64 ? (nblocks - want_reserve) / 64 : 1; // (no lane without a block)
        // up to 8 GiB: a nearly full device does without the lanes instead of failing the call
        p.lane_tab_bytes = lgrid * 64 * (size_t)kLzfTabBytes;
        p.handback_bytes = nblocks * sizeof(uint32_t); // a block is handed back once at most
        p.lanes = {true, (uint32_t)lgrid, 0, p.beside ? Target::lanes_side : Target::caller};
        p.lanes_kernel = n <= 4096 ? LzfLanes::tagged : LzfLanes::plain;
        if (p.beside) {
            p.lane_reserve = (uint32_t)want_reserve;
            if (p.lane_reserve < 1) p.lane_reserve = 1; // (0 means "on their own" to the kernel; the protocol itself needs no reserve)
        }
    }
    p.links_lds = kLzfTabBytes + ((big ? kChainMax + 16 : n) + 15u) / 16u * 16u + 32u;
    const uint32_t wave_lds = big ? n2 / 8 + 16u : 2 * n2 + ((n + 15u) & ~15u) + 16u;
    p.per_cu = at_most<size_t>((160u * 1024u) / (wave_lds + 64), big ? 20 : 16);
    // (n2 / 8 bytes of LDS per workgroup: 20 per CU at 64 KiB; smaller blocks: as many wavefronts as measured to pay)
    p.st_cu = at_most<size_t>((160u * 1024u) / (n2 / 8), st_wpc);
    p.chain_kernel = sthread ? LzfChain::sthread : big ? LzfChain::big : LzfChain::small;
    p.chain_lds = sthread ? n2 / 8 : wave_lds;
    // CW_LZF_SHARE_GIVE_UP (test knob): every workgroup but a round's claimant gives up at once
    p.spin_cap = kn.lzf_share_give_up ? 0u : kShareSpinCap;
    p.rounds_over_batch = !use_lanes || p.beside;
    p.rounds_over_handback = use_lanes;
    return p;
}

// ---- hashes ---------------------------------------------------------------------------------------------------------------------------
HashPlan hash_plan(const HashCall &call, const Knobs &kn)
{
    HashPlan p;
    const int nw = p.state_words = call.state_words;
    const size_t bb = nw ? (size_t)nw * 8 : 64;
    p.grid = (uint32_t)((call.nblocks + kHashThreads - 1) / kHashThreads);
    p.aligned = call.src_mis16 == 0;
    // (an empty message is "ragged" too: its only step is padding, and the hot kernels' first load would read bytes that are not there)
    p.ragged = call.block_bytes == 0 || call.block_bytes % bb != 0;
    if (!nw) return p; // SHA-256: one kernel family, the member by (aligned, ragged)
    // Long Skein messages go out in sliced launches (skein_kernels.hip has the measurements); CW_SKEIN_SLICED=0: never (profiling knob)
    if (call.may_slice && kn.skein_sliced && call.nblocks >= kSlicedMinBlocks && !p.ragged && call.block_bytes / bb + 1 >= kSlicedMinSteps &&
        p.aligned && call.digest_mis16 == 0) {
        p.sliced = true;
        const size_t total = p.total = call.block_bytes / bb + 1, spl = 128 / bb;
        const size_t nsl = kn.skein_nslices ? (size_t)kn.skein_nslices : kSkeinSlices; // CW_SKEIN_NSLICES: profiling knob
        size_t slice_steps = (total + nsl - 1) / nsl;
        p.slice_steps = slice_steps = (slice_steps + spl - 1) / spl * spl; // whole 128-byte lines
        p.state_bytes = call.nblocks * (size_t)nw * sizeof(uint64_t);
        for (size_t b = 0; b < total; b += slice_steps) {
            const size_t e = b + slice_steps < total ? b + slice_steps : total;
            // 8 words only: for 4 words hipcc moves a quarter of the mask-free line request to the loop top
            const bool interior = nw == 8 && (e - b) % spl == 0 && e + spl <= total - 1; // the slice and its prefetches stay inside the message
            p.slices.push_back({b, e, interior});
        }
        return p;
    }
    // Two hot kernels for aligned, whole-step blocks: the line kernel (105 VGPRs, every cache line fetched once) and
    // the step kernel (92 VGPRs, 64 bytes per step, ~40 % of the lines fetched twice).  Alone they are equally fast;
    // beside codec wavefronts the step kernel keeps 4 instead of 3 hash wavefronts per SIMD, which helped at 512 Ki
    // blocks (32.7 vs 36-42 ms) and made no difference at 1 Mi blocks (68 vs 69 ms), so no caller asks for it;
    // CW_SKEIN_MODE=steps|lines overrides (profiling knob).
    const bool steps = kn.skein_mode == SkeinMode::steps;
    p.form = p.ragged ? SkeinForm::ragged : p.aligned && steps ? SkeinForm::steps : SkeinForm::lines;
    return p;
}

// ---- description ----------------------------------------------------------------------------------------------------------------------
namespace {
// parts joined by " + "; a part that does not fit is cut at the buffer's end
__attribute__((format(printf, 2, 3))) void add(Description &d, const char *fmt, ...)
{
    const size_t used = strlen(d.text);
    if (used && used + 3 < sizeof d.text) strcat(d.text, " + ");
    const size_t at = strlen(d.text);
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(d.text + at, sizeof d.text - at, fmt, ap);
    va_end(ap);
}
// the LZF rounds repeat their kernels: a name is listed once, and only whole
void add_once(Description &d, const char *name, const char *tag = "")
{
    char part[sizeof d.text];
    const size_t len = (size_t)snprintf(part, sizeof part, "%s%s", name, tag);
    if (strstr(d.text, part)) return;
    const size_t used = strlen(d.text);
    if (used + len + 4 < sizeof d.text) { if (used) strcat(d.text, " + "); strcat(d.text, part); }
}
const char *side_tag(const Stage &s) { return s.stream == Target::caller ? "" : " [side stream]"; }
} // namespace

// names as rocprofv3 prints them; a kernel that decides on the device whether the queue's length is in its range carries the range
Description describe(const Lz4Plan &p)
{
    Description d = {""};
    if (p.scan_span.on) add(d, "%s", kernel_name(p.scan_span_kernel));
    if (p.scan_stream.on) add(d, "cw::lz4_scan_stream_kernel");
    if (p.scan_generic.on) add(d, "cw::lz4_scan_kernel");
    if (p.stop_after_scan) return d;
    if (p.lanes.on) {
        if (p.lanes_form == Lz4Plan::LanesForm::ring_auto)
            add(d, "cw::lz4_lanes_ring_auto_kernel (queue >= %u: two positions per iteration, >= %u: one)%s", p.lmin, p.wide_from, side_tag(p.lanes));
        else
            add(d, "%s (queue >= %u)%s", p.lanes_form == Lz4Plan::LanesForm::ring ? kernel_name(p.ring_kernel) : kernel_name(p.lanes_kernel), p.lmin,
                side_tag(p.lanes));
    }
    if (p.vtab.on) {
        if (p.vmax != kNoMax) add(d, "%s (queue < %u)%s", kernel_name(p.vtab_kernel), p.vmax, side_tag(p.vtab));
        else add(d, "%s%s", kernel_name(p.vtab_kernel), side_tag(p.vtab));
    }
    if (p.ltab.on) add(d, "%s", kernel_name(Lz4Vtab::lds_table));
    if (p.parse.on) add(d, "%s", kernel_name(p.parse_kernel));
    if (p.cut_only) add(d, "%s", kernel_name(p.redo_kernel)); // (otherwise the redo pass finds an empty list unless the LDS ever applied an exchange's lanes out of order)
    return d;
}

Description describe(const LzfPlan &p)
{
    Description d = {""};
    if (p.path == LzfPlan::Path::parse) add_once(d, kernel_name(p.parse_kernel));
    if (p.path == LzfPlan::Path::cut) add_once(d, "cw::lzf_blocks_kernel");
    if (p.path != LzfPlan::Path::rounds) return d;
    if (p.lanes.on) add_once(d, kernel_name(p.lanes_kernel), side_tag(p.lanes));
    if (p.rounds_over_batch) { add_once(d, "cw::lzf_links_kernel"); add_once(d, kernel_name(p.chain_kernel)); }
    if (p.rounds_over_handback) { add_once(d, "cw::lzf_links_kernel (handed-back blocks)"); add_once(d, kernel_name(p.chain_kernel)); }
    return d;
}

Description describe(const HashPlan &p)
{
    Description d = {""};
    if (!p.state_words) {
        add(d, "%s", sha256_kernel_name(p.aligned, p.ragged));
    } else if (p.sliced) {
        bool interior = false;
        for (const SkeinSlice &s : p.slices) interior |= s.interior;
        if (interior) add(d, "%s", skein_slice_kernel_name(p.state_words, true));
        add(d, "%s", skein_slice_kernel_name(p.state_words, false)); // (a hash's last launch is never interior)
    } else {
        add(d, "%s", skein_kernel_name(p.state_words, p.form, p.aligned));
    }
    return d;
}

// ---- dump -----------------------------------------------------------------------------------------------------------------------------
namespace {
struct Dump {
    std::string out;
    void kv(const char *key, unsigned long long v) { out += key; out += '='; out += std::to_string(v); out += '\n'; }
    void kv(const char *key, const char *v) { out += key; out += '='; out += v; out += '\n'; }
    void stage(const char *key, const Stage &s) // a stage is one field: `off`, or grid (workgroups of 64), LDS bytes and stream
    {
        static const char *const target[] = {"caller", "lanes_side", "vtab_side"};
        kv(key, s.on ? ("grid " + std::to_string(s.grid) + " lds " + std::to_string(s.lds) + " on " + target[(int)s.stream]).c_str() : "off");
    }
};
const char *pool_name(SidePool p) { return p == SidePool::greatest ? "greatest" : "normal"; }
} // namespace

std::string dump(const Lz4Plan &p)
{
    Dump d;
    d.kv("staged", p.staged);
    d.stage("scan_span", p.scan_span);
    d.kv("scan_span.kernel", kernel_name(p.scan_span_kernel));
    d.stage("scan_stream", p.scan_stream);
    d.stage("scan_generic", p.scan_generic);
    d.kv("lg", p.lg); d.kv("nspans", p.nspans); d.kv("done", p.done); d.kv("rest", p.rest);
    d.kv("stop_after_scan", p.stop_after_scan);
    d.stage("lanes", p.lanes);
    d.kv("lanes.form", p.lanes_form == Lz4Plan::LanesForm::table ? "table" : p.lanes_form == Lz4Plan::LanesForm::ring ? "ring" : "ring_auto");
    d.kv("lanes.kernel", kernel_name(p.lanes_kernel));
    d.kv("lanes.ring_kernel", kernel_name(p.ring_kernel));
    d.kv("lanes.pool", pool_name(p.lanes_pool));
    d.kv("lmin", p.lmin); d.kv("reserve", p.reserve); d.kv("reserve_wide", p.reserve_wide); d.kv("wide_from", p.wide_from);
    d.kv("lane_leave", p.lane_leave);
    d.kv("lane_tab_bytes", p.lane_tab_bytes);
    d.stage("vtab", p.vtab);
    d.kv("vtab.kernel", kernel_name(p.vtab_kernel));
    d.kv("vtab.pool", pool_name(p.vtab_pool));
    d.kv("vmin", p.vmin); d.kv("vmax", p.vmax); d.kv("vres", p.vres); d.kv("gen", (unsigned long long)p.gen);
    d.stage("ltab", p.ltab);
    d.stage("parse", p.parse);
    d.kv("parse.kernel", kernel_name(p.parse_kernel));
    d.kv("force_redo", p.force_redo);
    d.stage("redo", p.redo);
    d.kv("redo.kernel", kernel_name(p.redo_kernel));
    d.kv("cut_only", p.cut_only);
    d.kv("queue_bytes", p.queue_bytes); d.kv("queue_min_bytes", p.queue_min_bytes);
    return d.out;
}

std::string dump(const HashPlan &p)
{
    std::string out;
    for (const SkeinSlice &s : p.slices)
        out += "slice=" + std::to_string(s.begin) + ".." + std::to_string(s.end) + " interior=" + (s.interior ? "1" : "0") + "\n";
    return out;
}

std::string dump(const LzfPlan &p)
{
    Dump d;
    d.kv("path", p.path == LzfPlan::Path::rounds ? "rounds" : p.path == LzfPlan::Path::parse ? "parse" : "cut");
    d.stage("parse", p.parse);
    d.kv("parse.kernel", kernel_name(p.parse_kernel));
    d.stage("blocks", p.blocks);
    d.kv("in_lds", p.in_lds); d.kv("force_redo", p.force_redo); d.kv("blocks_pass", p.blocks_pass);
    d.kv("big", p.big); d.kv("beside", p.beside);
    d.kv("n2", p.n2); d.kv("chunk", p.chunk); d.kv("hb_chunk", p.hb_chunk);
    d.kv("rounds_over_batch", p.rounds_over_batch); d.kv("rounds_over_handback", p.rounds_over_handback);
    d.kv("chain.kernel", kernel_name(p.chain_kernel));
    d.kv("links_lds", p.links_lds); d.kv("chain_lds", p.chain_lds);
    d.kv("per_cu", p.per_cu); d.kv("st_cu", p.st_cu); d.kv("spin_cap", p.spin_cap);
    d.stage("lanes", p.lanes);
    d.kv("lanes.kernel", kernel_name(p.lanes_kernel));
    d.kv("lanes.pool", pool_name(p.lanes_pool));
    d.kv("lane_reserve", p.lane_reserve);
    d.kv("links_bytes", p.links_bytes); d.kv("lane_tab_bytes", p.lane_tab_bytes); d.kv("handback_bytes", p.handback_bytes);
    return d.out;
}

} // namespace cw
