"""Reference model of composing a stream from stored ranges and new bytes (include/cw_hashcompress.h: cw_store_compose and
cw_dev_cdc_resync_windows), over ``cdc_model.chunk`` only, so that ``chunk(B)`` is an independent check.

Source A is the concatenation of one or more stored streams: its cuts c_0 = 0 .. c_K and, with several streams, ``first`` (stream f
is positions [first[f], first[f+1]), as cw_dev_store_account takes it).  An op is the tuple (b_off, len, a_off, payload_off) of
``delta_model``: the ops tile B from 0, each a copy out of A or new bytes out of the payload.

``anchors`` states the rule (which positions of A a copy may keep), ``kept_by_rule`` the definition of the result over ``chunk(B)``,
and ``compose`` the procedure of cw_store_compose: windows between anchors, rounds that only chunk, landings, doubled lookaheads and
merges across exhausted anchors.  ``CASES`` names the inputs that reach each edge; the GPU test runs the same table."""
from __future__ import annotations

from bisect import bisect_left, bisect_right

import numpy as np

import cdc_model as CM

M = 1 << 64
NONE = M - 1                                     # CW_DELTA_NONE
P = CM.default_params(256)                       # 64 / 256 / 2048: the parameters of every case below


def copy(b, n, a):
    return (b, n, a, NONE)


def new(b, n, pay):
    return (b, n, NONE, pay)


def tile(parts):
    """ops from ("copy", a_off, len) and ("new", bytes) parts, and the payload"""
    ops, payload, b = [], b"", 0
    for part in parts:
        if part[0] == "copy":
            if part[2]:
                ops.append(copy(b, part[2], part[1]))
                b += part[2]
        elif len(part[1]):
            ops.append(new(b, len(part[1]), len(payload)))
            payload += bytes(part[1])
            b += len(part[1])
    return ops, payload


def build(a: bytes, ops, payload: bytes) -> bytes:
    out = bytearray()
    for b, n, src, pay in ops:
        assert b == len(out) and n >= 1 and (src == NONE) != (pay == NONE)
        part = a[src:src + n] if src != NONE else payload[pay:pay + n]
        assert len(part) == n
        out += part
    return bytes(out)


def join(streams, p=P):
    """(A, cuts, first) of the concatenation of ``streams``, each chunked alone"""
    cuts, first, at = [0], [0], 0
    for s in streams:
        cuts += [at + c for c in CM.chunk(s, p)[1:]]
        at += len(s)
        first.append(len(cuts) - 1)
    return b"".join(streams), cuts, first


def pieces(ops, cuts, first):
    """the copies as (b, len, a): adjacent copies that continue each other merged, then split at every stream end of A inside them"""
    merged = []
    for b, n, a, _ in ops:
        if a == NONE:
            continue
        if merged and merged[-1][0] + merged[-1][1] == b and merged[-1][2] + merged[-1][1] == a:
            merged[-1][1] += n
        else:
            merged.append([b, n, a])
    ends = sorted({cuts[f] for f in first[1:-1]})
    out = []
    for b, n, a in merged:
        lo = a
        for e in ends[bisect_right(ends, a):bisect_left(ends, a + n)]:
            out.append((b + lo - a, e - lo, lo))
            lo = e
        out.append((b + lo - a, a + n - lo, lo))
    return out


def anchors(ops, cuts, first, nb):
    """(b, d, p, q) of every copy piece with keepable positions [p, q), q > p, d = a - b (mod 2^64), in B order"""
    last = set(first[1:])                        # s is the last position of its stream when s + 1 is in here
    out = []
    for b, n, a in pieces(ops, cuts, first):
        p, q = bisect_left(cuts, a), bisect_right(cuts, a + n) - 1
        if q > p and q in last and cuts[q] - a + b != nb:
            q -= 1
        if q > p:
            out.append((b, (a - b) % M, p, q))
    return out


def kept_by_rule(ops, cuts, first, b_cuts):
    """the definition: {x: s} for every chunk [x, x') of B that an anchor keeps as position s of A"""
    nb = b_cuts[-1]
    keep = {}
    for b, d, p, q in anchors(ops, cuts, first, nb):
        a = (b + d) % M
        for s in range(p, q):
            x = cuts[s] - a + b
            i = bisect_left(b_cuts, x)
            if i < len(b_cuts) - 1 and b_cuts[i] == x:
                assert x not in keep
                keep[x] = s
    return keep


def resync_windows(x, first, wins, old):
    """cw_dev_cdc_resync_windows over plain lists: [verdict, t, s, x_t] per window.  x = all cuts, window w's are x[first[w] ..
    first[w+1]]; wins = (new_from, shift, old_first, old_count, final); s is an index into ``old``."""
    out = []
    for w, (new_from, shift, old_first, old_count, final) in enumerate(wins):
        lo, hi = first[w], first[w + 1]
        mine = list(old[old_first:old_first + old_count])
        hit = [1, 0, 0, 0]
        for g in range(lo + 1, hi + 1 if final else hi):
            y = (x[g] + shift) % M
            i = bisect_left(mine, y)
            if x[g] >= new_from and i < len(mine) and mine[i] == y:
                hit = [0, g - lo, old_first + i, x[g]]
                break
        out.append(hit)
    return out


class Window:
    def __init__(self, start, anchor, look):
        self.start, self.anchor, self.look = start, anchor, look   # anchor: (b, d, p, q), or None for the final window
        self.resolved, self.discard = False, False
        self.t = self.s = self.end = 0                              # resolved: t chunks in [start, end), then positions [s, q)


def compose(a: bytes, cuts, first, ops, payload: bytes, p=P, lookahead: int = 0):
    """dict(cuts, kept, stats, extents): the procedure.  cuts = B's; kept = {x: s}; extents = [(lo, hi, t)] in B order."""
    b_bytes = build(a, ops, payload)
    nb = len(b_bytes)
    stats = dict(windows=0, rounds=0, merged_windows=0, rebuilt_bytes=0, rebuilt_chunks=0, kept_positions=0)
    look0 = max(lookahead or 4 * p["max"], 2 * p["max"])
    wins, start = [], 0
    for anc in anchors(ops, cuts, first, nb):
        b, d, pp, q = anc
        w = Window(start, anc, look0)
        if cuts[pp] - (b + d) % M + b == start:  # the anchor starts on an A cut where the region starts: kept from there, no window
            w.resolved, w.s, w.end = True, pp, start
        else:
            stats["windows"] += 1
        wins.append(w)
        start = cuts[q] - (b + d) % M + b
    if start < nb:
        wins.append(Window(start, None, look0))
        stats["windows"] += 1

    while any(not w.resolved for w in wins):
        stats["rounds"] += 1
        # the round: every unresolved window, chunked as a stream of its own
        active = [w for w in wins if not w.resolved]
        x, wfirst, specs, at = [0], [0], [], 0
        for w in active:
            if w.anchor is None:
                end, w.exhausted = nb, False
            else:
                b, d, pp, q = w.anchor
                a0 = (b + d) % M
                e = bisect_left(cuts, max(b, w.start) + w.look + a0 - b, pp, q + 1)
                e = min(e, q)
                end, w.exhausted = cuts[e] - a0 + b, e == q
            part = CM.chunk(b_bytes[w.start:end], p)
            x += [at + c for c in part[1:]]
            wfirst.append(len(x) - 1)
            if w.anchor is None:
                specs.append((0, 0, 0, 0, 1))
            else:
                specs.append((max(b, w.start) - w.start + at, (d + w.start - at) % M, pp, q - pp, 1 if end == nb else 0))
            w.at, w.tried_end, w.n = at, end, len(part) - 1
            at += end - w.start
        res = dict(zip(map(id, active), resync_windows(x, wfirst, specs, cuts)))
        # after the round, in B order; settled = every window in front of this one is resolved
        settled, i = True, 0
        while i < len(wins):
            w = wins[i]
            i += 1
            if w.discard:
                w.discard, settled = False, False
                continue
            if id(w) not in res:
                settled = settled and w.resolved  # (a window a merge has just reopened)
                continue
            verdict, t, s, xt = res[id(w)]
            if w.anchor is None:
                w.resolved, w.t, w.end = True, w.n, nb
            elif verdict == 0:
                w.resolved, w.t, w.s, w.end = True, t, s, xt - w.at + w.start
            elif not w.exhausted:
                w.look *= 2
                settled = False
            elif not settled:
                settled = False                   # its start is not known to be a true cut yet: it waits
            else:                                 # the anchor is dropped: the window merges into the next one
                stats["merged_windows"] += 1
                if i == len(wins):
                    wins.append(Window(w.start, None, look0))
                nxt = wins[i]
                nxt.start, nxt.resolved, nxt.discard = w.start, False, id(nxt) in res
                del wins[i - 1]
                i -= 1

    out, kept, extents = [0], {}, []
    for w in wins:
        assert out[-1] == w.start
        if w.end > w.start:
            part = CM.chunk(b_bytes[w.start:w.end], p)
            assert len(part) - 1 == w.t, "an extent chunks into what its round found"
            out += [w.start + c for c in part[1:]]
            extents.append((w.start, w.end, w.t))
            stats["rebuilt_bytes"] += w.end - w.start
            stats["rebuilt_chunks"] += w.t
        if w.anchor is not None:
            b, d, pp, q = w.anchor
            a0 = (b + d) % M
            for s in range(w.s, q):
                kept[cuts[s] - a0 + b] = s
                out.append(cuts[s + 1] - a0 + b)
            stats["kept_positions"] += q - w.s
    assert out[-1] == nb
    return dict(cuts=out, kept=kept, stats=stats, extents=extents, bytes=b_bytes)


# ---- the named cases -------------------------------------------------------------------------------------------------------------
def _noise(seed, n):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def _case(name, streams, parts, lookahead=0, **expect):
    a, cuts, first = join(streams)
    ops, payload = tile(parts(a, cuts, first))
    return dict(name=name, streams=streams, a=a, cuts=cuts, first=first, ops=ops, payload=payload, lookahead=lookahead, expect=expect)


def cases():
    """The table: each case with what it has to reach (``expect``: exact statistics, or ``min_`` bounds), checked by the model test."""
    n1, n2, n3 = _noise(1, 60000), _noise(2, 30000), _noise(3, 20000)
    zero = bytes(50000)
    out = [
        _case("landing in the first round", [n1], lambda a, c, f: [("copy", 0, 20000), ("new", _noise(10, 777)), ("copy", 20500, 39500)],
              rounds=1, merged_windows=0, windows=1),
        # the first cut of A that the window can land on lies behind the first lookahead: a stretch of zeros, shifted by 5, in front of it
        _case("a second round", [bytes(20000) + n2], lambda a, c, f: [("new", b"x" * 10), ("copy", 5, len(a) - 5)],
              lookahead=1, min_rounds=2, merged_windows=0, windows=1),
        _case("a merge across an exhausted anchor", [n1],
              lambda a, c, f: [("copy", 0, c[20]), ("new", b"y" * 50), ("copy", c[31], c[32] - c[31]), ("new", b"z" * 70), ("copy", c[40], c[-1] - c[40])],
              merged_windows=1, windows=2),
        _case("an anchor kept from byte 0", [n1], lambda a, c, f: [("copy", c[5], c[50] - c[5]), ("new", _noise(11, 300))], windows=1, rounds=1),
        _case("a final window", [n1], lambda a, c, f: [("copy", 0, 30000), ("new", _noise(12, 9000))], rounds=1, windows=1),
        _case("no anchor at all", [n2], lambda a, c, f: [("new", _noise(13, 40000))], windows=1, rounds=1, kept_positions=0),
        _case("a moved copy and a copy used twice", [n1],
              lambda a, c, f: [("copy", 40000, 15000), ("copy", 0, 25000), ("new", b"mid" * 99), ("copy", 0, 25000), ("copy", 40000, 20000)], rounds=1),
        _case("a copy to A's end that is B's end", [n1], lambda a, c, f: [("new", _noise(14, 500)), ("copy", 30000, 30000)], rounds=1, windows=1),
        _case("a copy to A's end that is not B's end", [n1], lambda a, c, f: [("copy", 30000, 30000), ("new", _noise(15, 500))], rounds=1),
        _case("a copy across a stream end of a joined source", [n2, n3, n2[:7000]],
              lambda a, c, f: [("copy", 1000, 30000 + 20000 + 7000 - 1000)], rounds=1),
        _case("an all-zero source that never lands", [zero], lambda a, c, f: [("copy", 0, 20000), ("new", b"\x00" * 100), ("copy", 20000, 30000)],
              lookahead=1, min_rounds=3),
        _case("nops == 0", [n2], lambda a, c, f: [], windows=0, rounds=0, kept_positions=0),
    ]
    return out
