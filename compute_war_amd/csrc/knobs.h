// knobs.h -- the tuning / test knobs, decoded: one typed snapshot per call.  No HIP here: the launch plans (launch_plan.h) read a
// snapshot without a device.
#pragma once

#include <stdint.h>

#include <optional>

namespace cw {

// The tuning / test knobs (CW_TESTING in the public header), decoded.  A knob's value is what cw_tune_set gave it, else the
// environment variable of the same name; the table in cw_api.hip is the only code that knows their names and formats.  Knobs
// marked "> 0" hold the value only when it is a positive number and 0 otherwise; std::nullopt = unset.  Defaults that depend on
// the call stay where the call decides.
enum class Lz4Mode : uint8_t { normal, scan, generic, stream, cut }; // CW_LZ4_MODE (other values: normal)
enum class LzfMode : uint8_t { normal, cut, table };                // CW_LZF_MODE (other values: normal)
enum class SkeinMode : uint8_t { unset, steps, lines };             // CW_SKEIN_MODE: unset / "steps" / any other value
enum class SidePrio : uint8_t { both, lanes, none };                // CW_SIDE_PRIO: unset or 2... / other / 0...: streams on the high-priority pool
struct Knobs {
    // first character
    bool skein_sliced = true, lz4_lanes_fp = true, lzf_sthread = true; // off iff it starts with '0'
    bool serial = false, debug_host = false, prepare_cold = false;     // on iff it starts with '1'
    std::optional<bool> fused_gate, host_shared_streams;               // set: starts with '1'
    std::optional<bool> lanes_concurrent;                              // set: does not start with '0'
    SidePrio side_prio = SidePrio::both;
    // strings, presence
    Lz4Mode lz4_mode = Lz4Mode::normal;
    LzfMode lzf_mode = LzfMode::normal;
    SkeinMode skein_mode = SkeinMode::unset;
    bool lz4_parse_fp = false; // CW_LZ4_PARSE == "fp"
    bool debug_lzf = false;    // set, to any value
    // > 0
    int scan_wpc = 0, parse_wpc = 0, lanes_wpc = 0, lanes_reserve = 0, vtab_wpc = 0, lzf_st_wpc = 0, lzf_round = 0, lzf_lds_max = 0,
        skein_nslices = 0;
    long host_chunk_mb = 0, host_big_chunk_mb = 0, cdc_segment = 0, store_piece = 0, scrub_entries = 0, delta_tile = 0;
    bool force_redo = false, lzf_share_give_up = false; // CW_LZ_FORCE_REDO, CW_LZF_SHARE_GIVE_UP
    // set: atoi of the value ("" = 0)
    std::optional<int> lz4_lanes, lzf_lanes, decode_lanes, lanes_leave, vtab_min, vtab_max, vtab_reserve, lz4_vtab, lz4_lanes_ring,
        lz4_headw, lz4_ltab, vtab_gen;
    std::optional<int> lz4_stage_max; // set: atoi of the value if it is >= 0
};
// The knobs as they are now: each launch function takes one snapshot when it starts, so tests sweep settings in one process.
Knobs knobs();

} // namespace cw
