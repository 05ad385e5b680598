// lane_codec.h -- the lane-per-block codecs, written once: a LANE owns a block or a chunk and runs the serial
// LZ4 / LZF parser or decoder as it stands.  The fixed-size kernels (lz4_lanes_kernel, lzf_lanes_kernel, decompress_lanes_kernel)
// and the kernels over content-defined chunks (chunk_codec_kernels.hip) all run the loops below; what differs between them is
// handed in as two small policy objects:
//   Src  where work comes from and where it goes: g (the input), out (the slot), blk (the index sizes[] is written at), n and
//        the limits derived from it.  take() answers kDone (no more work), kTaken (g, out, blk -- and n, if it is a lane value
//        -- are set) or kAgain (nothing to parse, sizes[] already written: ask again).  For fixed blocks n and its limits are
//        const members set from the kernel argument, so they stay launch-uniform (scalar registers); the chunk sources write
//        them in take().  kShort says whether inputs too short for the parser's own limits can occur.
//   Tab  the lane's hash table in global memory: the entry format, and begin(), which makes the table read as empty for the next
//        input (zeroes it, or moves on to the next epoch).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lz_device.h"

namespace cw {
namespace lane {

using lz::rd32;

constexpr uint32_t kMinMatch = 4, kLastLiterals = 5, kMFLimit = 12;                    // LZ4
constexpr uint32_t kMaxOff = 1u << 13, kMaxRef = (1u << 8) + (1u << 3), kMaxLit = 32;  // LZF

enum class Take : uint32_t { kDone, kTaken, kAgain };

__device__ __forceinline__ uint32_t hash13(uint32_t v) { return (v * 2654435761u) >> 19; }
__device__ __forceinline__ uint4 ld16g(const uint8_t *p)
{
    uint4 v;
    __builtin_memcpy(&v, p, 16); // unaligned global_load_dwordx4
    return v;
}
__device__ __forceinline__ void lane_put_len(uint8_t *__restrict__ out, uint32_t &op, uint32_t extra)
{
    while (extra >= 255) { out[op++] = 255; extra -= 255; }
    out[op++] = (uint8_t)extra;
}
// 4 bytes at byte offset s (4 <= s <= 12) of a 16-byte window held in (x, y, z, w)
__device__ __forceinline__ uint32_t win_at(const uint4 &q, uint32_t s)
{
    return s < 8 ? __builtin_amdgcn_alignbyte(q.z, q.y, s & 3u) : s < 12 ? __builtin_amdgcn_alignbyte(q.w, q.z, s & 3u) : q.w;
}
// stores exactly cnt (1..16) bytes of (a, b)
__device__ __forceinline__ void store_upto16(uint8_t *p, uint64_t a, uint64_t b, uint32_t cnt)
{
    if (cnt & 16) { __builtin_memcpy(p, &a, 8); __builtin_memcpy(p + 8, &b, 8); return; }
    if (cnt & 8) { __builtin_memcpy(p, &a, 8); a = b; p += 8; }
    if (cnt & 4) { const uint32_t t = (uint32_t)a; __builtin_memcpy(p, &t, 4); a >>= 32; p += 4; }
    if (cnt & 2) { const uint16_t t = (uint16_t)a; __builtin_memcpy(p, &t, 2); a >>= 16; p += 2; }
    if (cnt & 1) *p = (uint8_t)a;
}
__device__ __forceinline__ uint32_t lzf_slot(uint32_t b0, uint32_t b1, uint32_t b2)
{
    // IDX(hval) = ((hval >> 8) - hval*5) & 0xFFFF with hval = b0<<16 | b1<<8 | b2 (VERY_FAST, HLOG 16)
    return (((b0 << 8) | b1) - (((b1 << 8) | b2) * 5u)) & 0xFFFFu;
}

// ---------------------------------------------------------------------------------------------------
// LZ4.  Every lane is in one of the states below; an iteration of the wavefront's loop runs one step of every lane:
//   PROBE   the parser's search loop body, or the re-test right after a match (same table traffic, different follow-up)
//   EMIT    a match was found: catch-up, literals, offset, match length; then PROBE (as a re-test) or TAIL
//   TAIL    last literals, size; then NEXT
//   NEXT    take the next block or chunk, clean the table
// Per iteration a lane's dependent memory chain is: its 16 bytes around ip -> table slot -> the candidate's 16 bytes.
//
// Tab::get(h, v, maybe) returns the slot's position and whether the bytes there can be the 4 bytes v at all; an entry that is
// not of this input reads as the zeroed table would: position 0, which can only match the input's first 4 bytes.  Where an entry
// says whose it is (kNameFirst), those 4 bytes are entered by name when the input is taken: tab[hash(first 4 bytes)] = 0 is what
// an empty table already says, the entry then says whose 0 it is.
// All loads stay inside the input: n >= 13 in PROBE and EMIT (the parser's own limits see to it; shorter inputs, which only a
// kShort source has, are last literals only).  The literal copies may overshoot by up to 7 bytes into what the sequence's offset
// and the bytes behind it overwrite, never past the output's final size.
// ---------------------------------------------------------------------------------------------------
enum : uint32_t { LS_NEXT = 0, LS_PROBE = 1, LS_EMIT = 2, LS_TAIL = 3, LS_EXIT = 4 };

template <class Src, class Tab>
__device__ __forceinline__ void lz4_lane_run(Src &s, Tab &t)
{
    uint32_t state = LS_NEXT;
    uint32_t ip = 0, anchor = 0, op = 0, step = 1, nb = 64, match = 0, first_lo = 0, first_hi = 0;
    bool retest = false;
    // own = the 16 bytes [ip-4, ip+12), requested one iteration ahead; vcur = the 4 bytes at ip, cut out of the previous
    // window when it reached that far (have_v), so that the table lookup never waits for the request
    uint4 own = make_uint4(0, 0, 0, 0), cd = make_uint4(0, 0, 0, 0);
    uint32_t vcur = 0, v2cur = 0;
    bool have_v = false;
    // literals of the last sequence on their way from memory: stored one iteration later (their load is then long done)
    uint64_t pend_a = 0, pend_b = 0;
    uint8_t *pend_dst = nullptr;
    uint32_t pend_n = 0;

    while (__ballot(state != LS_EXIT)) {
        // everything requested during the previous iteration is waited for here, once
        if (pend_n) { // exactly pend_n (1..16) bytes: what follows them in the slot is already written
            store_upto16(pend_dst, pend_a, pend_b, pend_n);
            pend_n = 0;
        }
        if (state == LS_NEXT) {
            const Take got = s.take();
            if (got == Take::kDone) {
                state = LS_EXIT;
            } else if (got == Take::kTaken) {
                const uint8_t *g = s.g;
                anchor = 0; op = 0;
                if (Src::kShort && s.n < kMFLimit + 1) {
                    state = LS_TAIL;
                } else {
                    t.begin();
                    first_lo = rd32(g, 0); first_hi = rd32(g, 4);
                    if (Tab::kNameFirst) t.put(hash13(first_lo), first_lo, 0);
                    ip = 1; step = 1; nb = 64; retest = false;
                    own.x = 0; own.y = rd32(g, 1); own.z = rd32(g, 5); own.w = rd32(g, 9); // no "before" at the input's start
                    have_v = false;
                    state = LS_PROBE;
                }
            }
        }
        const uint8_t *g = s.g;
        uint8_t *out = s.out;

        if (state == LS_PROBE) {
            const uint32_t next = ip + step;
            if (!retest && next > s.mflimit + 1) {
                state = LS_TAIL;
            } else {
                const uint32_t v = have_v ? vcur : own.y;
                if (retest) { // LZ4_putPosition(ip - 2) in front of the re-test
                    const uint32_t v2 = have_v ? v2cur : (own.x >> 16) | (own.y << 16);
                    t.put(hash13(v2), v2, ip - 2);
                }
                const uint32_t h = hash13(v);
                bool maybe;
                match = t.get(h, v, maybe);
                t.put(h, v, ip);
                uint32_t cat = ~v;
                if (maybe) {
                    if (match >= 4) { cd = ld16g(g + match - 4); cat = cd.y; }
                    else cat = __builtin_amdgcn_alignbyte(first_hi, first_lo, match);
                }
                if (cat == v) {
                    state = LS_EMIT; // (own was requested for this ip an iteration ago: it is here by now)
                } else {
                    uint32_t nip;
                    if (retest) { nip = ip + 1; step = 1; nb = 64; retest = false; }
                    else { nip = next; step = nb >> 6; nb++; }
                    // the next position's 4 bytes, from the window if it reaches (it is the window of `ip` only if that
                    // has arrived, which it has unless this iteration ran on vcur: then the request is still the one for ip)
                    const uint32_t sh = nip - ip + 4;
                    have_v = sh <= 12 && ip >= 4;
                    if (have_v) vcur = win_at(own, sh);
                    ip = nip;
                    // (ip = mflimit + 1 is never probed, the next iteration sends it to TAIL: keep its request inside the input)
                    const uint32_t rp = ip <= s.mflimit ? ip : s.mflimit;
                    if (Src::kShort) { // 16 bytes from rp < 4 may leave a short input: three dwords, rp + 12 <= n
                        if (rp >= 4) own = ld16g(g + rp - 4); // [rp - 4, rp + 12)
                        else { own.x = 0; own.y = rd32(g, rp); own.z = rd32(g, rp + 4); own.w = rd32(g, rp + 8); have_v = false; }
                    } else {
                        own = ld16g(g + rp - (rp >= 4 ? 4 : 0));
                        if (rp < 4) { own.w = own.z; own.z = own.y; own.y = own.x; own.x = 0; have_v = false; }
                    }
                }
            }
        }

        if (state == LS_EMIT) {
            // own = [ip-4, ip+12) and cd = [match-4, match+12) (match >= 4), both as found by the probe
            const uint32_t ip0 = ip;
            const bool windows = ip >= 4 && match >= 4;
            uint32_t nf = 0; // equal bytes behind the 4 that matched
            bool nf_open = true;
            if (windows) {
                const uint64_t x = ((uint64_t)own.w << 32 | own.z) ^ ((uint64_t)cd.w << 32 | cd.z);
                nf = x ? (uint32_t)__builtin_ctzll(x) >> 3 : 8u;
                nf_open = nf == 8;
                const uint32_t lim = s.matchlimit - (ip0 + kMinMatch);
                if (nf >= lim) { nf = lim; nf_open = false; }
            }
            // ---- catch-up over the pending literals (a re-test has none: anchor == ip) ----
            if (!retest) {
                if (windows) {
                    const uint32_t room = ip - anchor < match ? ip - anchor : match;
                    const uint32_t y = own.x ^ cd.x;
                    uint32_t back = y ? (uint32_t)__builtin_clz(y) >> 3 : 4u;
                    if (back > room) back = room;
                    ip -= back; match -= back;
                    if (back == 4) while (ip > anchor && match > 0 && g[ip - 1] == g[match - 1]) { ip--; match--; }
                } else {
                    while (ip > anchor && match > 0 && g[ip - 1] == g[match - 1]) { ip--; match--; }
                }
            }
            // ---- literals: 8 or 16 bytes requested now and stored next iteration; longer runs copied here ----
            const uint32_t lit = ip - anchor, tok = op++;
            uint32_t token;
            if (lit >= 15) { token = 15u << 4; lane_put_len(out, op, lit - 15); }
            else token = lit << 4;
            if (lit) {
                // (8 bytes from anchor stay inside the input: anchor + 8 <= ip + 7 <= n - 5; 16 only for runs of 9 and more)
                __builtin_memcpy(&pend_a, g + anchor, 8);
                if (lit > 8) __builtin_memcpy(&pend_b, g + anchor + 8, 8);
                pend_dst = out + op;
                pend_n = lit < 16 ? lit : 16;
                for (uint32_t k = 16; k < lit; k += 8) { // runs beyond 16 (0.3 % on text): 8 bytes at a time, the overshoot (< 8
                    uint64_t q;                          // bytes) lands where the offset and what follows are written next
                    __builtin_memcpy(&q, g + anchor + k, 8);
                    __builtin_memcpy(out + op + k, &q, 8);
                }
            }
            op += lit;
            // ---- offset, match length ----
            const uint32_t off = ip - match;
            out[op] = (uint8_t)off; out[op + 1] = (uint8_t)(off >> 8);
            op += 2;
            // the bytes taken back, the 4 that matched and the nf behind them are one run: mc = (ip0 - ip) + nf (+ what memory adds)
            uint32_t mc = ip0 - ip + nf;
            if (nf_open) {
                const uint32_t a = ip + kMinMatch, b = match + kMinMatch;
                while (a + mc + 8 <= s.matchlimit) {
                    uint64_t x, y;
                    __builtin_memcpy(&x, g + a + mc, 8);
                    __builtin_memcpy(&y, g + b + mc, 8);
                    const uint64_t d = x ^ y;
                    if (d) { mc += (uint32_t)__builtin_ctzll(d) >> 3; break; }
                    mc += 8;
                }
                if (a + mc + 8 > s.matchlimit) while (a + mc < s.matchlimit && g[a + mc] == g[b + mc]) mc++;
            }
            if (mc >= 15) { token += 15; lane_put_len(out, op, mc - 15); }
            else token += mc;
            out[tok] = (uint8_t)token;
            ip += kMinMatch + mc;
            anchor = ip;
            if (ip > s.mflimit) {
                state = LS_TAIL;
            } else {
                // the re-test's values out of the old window when the match was short enough (mend + 4 <= ip0 + 12)
                const uint32_t sh = ip - ip0 + 4;
                have_v = windows && sh <= 12;
                if (have_v) { vcur = win_at(own, sh); v2cur = win_at(own, sh - 2); }
                own = ld16g(g + ip - 4); // ip >= 5, ip + 12 <= n
                retest = true;
                state = LS_PROBE;
            }
        }

        if (state == LS_TAIL) {
            const uint32_t run = s.n - anchor;
            if (run >= 15) { out[op++] = 15u << 4; lane_put_len(out, op, run - 15); }
            else out[op++] = (uint8_t)(run << 4);
            uint32_t k = 0;
            for (; k + 16 <= run; k += 16) {
                uint4 q;
                __builtin_memcpy(&q, g + anchor + k, 16);
                __builtin_memcpy(out + op + k, &q, 16);
            }
            for (; k < run; k++) out[op + k] = g[anchor + k];
            op += run;
            s.sizes[s.blk] = op;
            state = LS_NEXT;
        }
    }
}

// ---------------------------------------------------------------------------------------------------
// LZF: liblzf's loop as it stands, one position per iteration -- hash the next three bytes, exchange the table slot, test the
// reference, emit a literal or a match -- with out_len = cap = n - 1 as the reference is called.  No links, no skip flags, no
// lane-order assumption: the parse is the serial one.  Tab::get(slot) returns the slot's position, 0 (which liblzf takes for "no
// reference") for an entry that is not of this input.  Src also supplies
//   rd(ip)        the up to 4 bytes at ip (ip + 2 < n), none read from behind the input
//   keep(ip, op)  asked before every step: false = the lane gives the input up as it stands (the source has seen to sizes[] or
//                 whoever parses it instead) and takes the next
// size 0 = did not fit.
// ---------------------------------------------------------------------------------------------------
template <class Src, class Tab>
__device__ __forceinline__ void lzf_lane_run(Src &s, Tab &t)
{
    enum : uint32_t { NEXT = 0, STEP = 1, TAIL = 2, EXIT = 3 };
    uint32_t state = NEXT, ip = 0, op = 0, lit = 0, v = 0;
    bool fail = false;

    while (__ballot(state != EXIT)) {
        if (state == NEXT) {
            const Take got = s.take();
            if (got == Take::kDone) {
                state = EXIT;
            } else if (got == Take::kTaken) {
                t.begin();
                ip = 0; op = 1; lit = 0; fail = false; // op = 1: the first literal run's control byte is reserved
                if (!Src::kShort || s.n >= 3) { v = s.rd(0); state = STEP; }
                else state = TAIL;
            }
        }
        const uint8_t *g = s.g;
        uint8_t *out = s.out;
        const uint32_t n = s.n, cap = n - 1;

        if (state == STEP && !s.keep(ip, op)) state = NEXT;

        if (state == STEP) { // ip + 2 < n; v = the bytes at ip (requested an iteration ago)
            const uint32_t b0 = v & 0xFFu, b1 = (v >> 8) & 0xFFu, b2 = (v >> 16) & 0xFFu;
            const uint32_t slot = lzf_slot(b0, b1, b2);
            const uint32_t ref = t.get(slot);
            t.put(slot, ip);
            bool is_match = false;
            if (ref > 0 && ip - ref - 1 < kMaxOff) is_match = ((rd32(g, ref) ^ v) & 0xFFFFFFu) == 0; // ref + 4 <= ip + 3 <= n
            if (is_match) {
                uint32_t maxlen = n - ip - 2;
                if (maxlen > kMaxRef) maxlen = kMaxRef;
                if (op + 4 >= cap && op - (lit == 0) + 4 >= cap) {
                    fail = true; state = TAIL;
                } else {
                    if (lit) out[op - lit - 1] = (uint8_t)(lit - 1);
                    else op -= 1;
                    // equal bytes from index 3 on, as far as the reference's loops can look
                    const uint32_t room = (n - ip < kMaxRef + 2 ? n - ip : kMaxRef + 2) - 3;
                    uint32_t eq = 0;
                    while (eq + 8 <= room) {
                        uint64_t x, y;
                        __builtin_memcpy(&x, g + ref + 3 + eq, 8);
                        __builtin_memcpy(&y, g + ip + 3 + eq, 8);
                        const uint64_t d = x ^ y;
                        if (d) { eq += (uint32_t)__builtin_ctzll(d) >> 3; break; }
                        eq += 8;
                    }
                    if (eq + 8 > room) while (eq < room && g[ref + 3 + eq] == g[ip + 3 + eq]) eq++;
                    uint32_t len;
                    if (maxlen > 16) { // 16 unrolled compares without a bound, then the bounded loop
                        if (eq < 16) len = 3 + eq;
                        else { len = 3 + eq < maxlen ? 3 + eq : maxlen; if (len < 19) len = 19; }
                    } else {
                        len = 3 + eq < maxlen ? 3 + eq : maxlen;
                        if (len < 3) len = 3;
                    }
                    const uint32_t off = ip - ref - 1, l2 = len - 2;
                    if (l2 < 7) {
                        out[op] = (uint8_t)((off >> 8) + (l2 << 5));
                        out[op + 1] = (uint8_t)off;
                        op += 2;
                    } else {
                        out[op] = (uint8_t)((off >> 8) + (7u << 5));
                        out[op + 1] = (uint8_t)(l2 - 7);
                        out[op + 2] = (uint8_t)off;
                        op += 3;
                    }
                    lit = 0; op += 1;
                    ip += len;
                    if (ip + 2 >= n) {
                        state = TAIL;
                    } else { // VERY_FAST: only the last two positions of the match are inserted
                        const uint32_t w = rd32(g, ip - 2); // bytes ip-2 .. ip+1
                        t.put(lzf_slot(w & 0xFFu, (w >> 8) & 0xFFu, (w >> 16) & 0xFFu), ip - 2);
                        t.put(lzf_slot((w >> 8) & 0xFFu, (w >> 16) & 0xFFu, w >> 24), ip - 1);
                        v = s.rd(ip);
                    }
                }
            } else {
                if (op >= cap) {
                    fail = true; state = TAIL;
                } else {
                    lit++;
                    out[op++] = (uint8_t)b0;
                    if (lit == kMaxLit) { out[op - lit - 1] = (uint8_t)(kMaxLit - 1); lit = 0; op++; }
                    ip++;
                    if (ip + 2 < n) v = (v >> 8) | ((uint32_t)(ip + 3 < n ? g[ip + 3] : 0u) << 24);
                    else state = TAIL;
                }
            }
        }

        if (state == TAIL) {
            if (!fail) {
                if (op + 3 > cap) {
                    fail = true;
                } else {
                    while (ip < n) {
                        lit++;
                        out[op++] = g[ip++];
                        if (lit == kMaxLit) { out[op - lit - 1] = (uint8_t)(kMaxLit - 1); lit = 0; op++; }
                    }
                    if (lit) out[op - lit - 1] = (uint8_t)(lit - 1);
                    else op -= 1;
                }
            }
            s.sizes[s.blk] = fail ? 0u : op;
            state = NEXT;
        }
    }
}

// ---------------------------------------------------------------------------------------------------
// Decoders: the format's loop as it stands, a lane per block or chunk.  Per sequence one 16-byte window of the compressed stream
// (token, short literal run and offset in one load when they fit), the literals' store, the match's load(s) from the lane's own
// earlier output and its store(s).  A match closer than 16 bytes is copied at a multiple of its offset (the output is periodic
// there), doubling until 16-byte pieces go through.  Nothing is read outside [0, n) of `in` or written outside [0, raw_bytes)
// of `d`: every step is checked against them.
// ---------------------------------------------------------------------------------------------------
// d[op .. op+len) = d[op-off ..), the format's overlapping copy; off >= 1, op - off >= 0, op + len <= cap (checked by the caller)
__device__ __forceinline__ void lane_copy_match(uint8_t *d, uint32_t op, uint32_t off, uint32_t len, uint32_t cap)
{
    const uint32_t base = op - off, end = op + len;
    uint32_t dist = off;
    while (op < end) {
        while (dist < 16 && 2 * dist <= op - base) dist *= 2; // any multiple of off that is already written is a period
        const uint32_t left = end - op, piece = left < 16 ? left : 16, cnt = piece < dist ? piece : dist;
        const uint32_t s = op - dist;
        if (s + 16 <= cap) {
            uint64_t a, b;
            __builtin_memcpy(&a, d + s, 8);
            __builtin_memcpy(&b, d + s + 8, 8);
            store_upto16(d + op, a, b, cnt);
        } else {
            for (uint32_t k = 0; k < cnt; k++) d[op + k] = d[s + k];
        }
        op += cnt;
    }
}
// d[op .. op+len) = in[ip ..): literal bytes; ip + len <= n and op + len <= cap checked by the caller
__device__ __forceinline__ void lane_copy_literals(uint8_t *d, uint32_t op, const uint8_t *in, uint32_t ip, uint32_t len, uint32_t n)
{
    for (uint32_t k = 0; k < len; k += 16) {
        const uint32_t cnt = len - k < 16 ? len - k : 16;
        if (ip + k + 16 <= n) {
            uint64_t a, b;
            __builtin_memcpy(&a, in + ip + k, 8);
            __builtin_memcpy(&b, in + ip + k + 8, 8);
            store_upto16(d + op + k, a, b, cnt);
        } else {
            for (uint32_t j = 0; j < cnt; j++) d[op + k + j] = in[ip + k + j];
        }
    }
}

// ALG 0 = LZ4, 1 = LZF.  Decodes in[0, n) into d[0, raw_bytes); returns true (bad) unless the stream is well formed and produced
// exactly raw_bytes.  bad = the caller's verdict on the extents themselves: set, nothing is loaded or stored.
template <int ALG>
__device__ __forceinline__ bool lane_decode(const uint8_t *in, uint32_t n, uint8_t *d, uint32_t raw_bytes, bool bad)
{
    uint32_t ip = 0, op = 0;
    if (ALG == 0) {
        while (!bad) {
            if (ip >= n) { bad = true; break; }
            // token, a literal run of up to 13 bytes and the offset in one window when the stream has 16 bytes left
            uint32_t w0 = 0, w1 = 0, w2 = 0, w3 = 0;
            const bool win = ip + 16 <= n;
            if (win) { uint4 q; __builtin_memcpy(&q, in + ip, 16); w0 = q.x; w1 = q.y; w2 = q.z; w3 = q.w; }
            const uint32_t tok = win ? w0 & 0xFFu : in[ip];
            uint32_t lit = tok >> 4, ml = tok & 15;
            uint32_t off = 0;
            if (win && lit <= 13) {
                if (lit > raw_bytes - op) { bad = true; break; }
                // literals = window bytes [1, 1 + lit)
                const uint64_t lo = (uint64_t)w1 << 32 | w0, hi = (uint64_t)w3 << 32 | w2;
                const uint64_t a = lo >> 8 | hi << 56, b = hi >> 8;
                if (lit) store_upto16(d + op, a, b, lit);
                op += lit;
                ip += 1 + lit;
                if (ip == n) break; // (a window means 16 bytes were left: not the last sequence unless lit == 15.. never here)
                const uint32_t sh = (1 + lit) * 8; // offset = window bytes [1 + lit, 3 + lit)
                const uint64_t o = sh < 64 ? (lo >> sh | (sh ? hi << (64 - sh) : 0)) : hi >> (sh - 64);
                off = (uint32_t)o & 0xFFFFu;
                ip += 2;
            } else {
                ip++;
                if (lit == 15) {
                    uint32_t c;
                    do { if (ip >= n) { bad = true; break; } c = in[ip]; ip++; lit += c; } while (c == 255);
                    if (bad) break;
                }
                if (lit > n - ip || lit > raw_bytes - op) { bad = true; break; }
                lane_copy_literals(d, op, in, ip, lit, n);
                ip += lit; op += lit;
                if (ip == n) break; // last sequence: literals only
                if (n - ip < 2) { bad = true; break; }
                off = (uint32_t)in[ip] | ((uint32_t)in[ip + 1] << 8);
                ip += 2;
            }
            if (off == 0 || off > op) { bad = true; break; }
            if (ml == 15) {
                uint32_t c;
                do { if (ip >= n) { bad = true; break; } c = in[ip]; ip++; ml += c; } while (c == 255);
                if (bad) break;
            }
            if (ml > raw_bytes || ml + 4 > raw_bytes - op) { bad = true; break; }
            ml += 4;
            lane_copy_match(d, op, off, ml, raw_bytes);
            op += ml;
        }
    } else {
        while (!bad && ip < n) {
            const uint32_t ctrl = in[ip]; ip++;
            if (ctrl < 32) {
                const uint32_t run = ctrl + 1;
                if (run > n - ip || run > raw_bytes - op) { bad = true; break; }
                lane_copy_literals(d, op, in, ip, run, n);
                ip += run; op += run;
            } else {
                uint32_t len = ctrl >> 5;
                if (ip >= n) { bad = true; break; }
                if (len == 7) { len += in[ip]; ip++; if (ip >= n) { bad = true; break; } }
                const uint32_t off = (((ctrl & 0x1f) << 8) | in[ip]) + 1; ip++;
                len += 2;
                if (off > op || len > raw_bytes - op) { bad = true; break; }
                lane_copy_match(d, op, off, len, raw_bytes);
                op += len;
            }
        }
    }
    if (op != raw_bytes) bad = true;
    return bad;
}

} // namespace lane
} // namespace cw
