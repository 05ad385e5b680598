"""Reference model of an in-place edit of a chunked stream (include/cw_hashcompress.h: cw_store_patch).

Old stream S of n bytes with cuts c_0 = 0 .. c_K = n; the edit (a, r, ins) replaces S[a .. a + r) by ins.  ``patch`` re-chunks from
the start of the chunk that holds byte a and stops at the first new cut that lands on an old cut behind the edit; everything
before and after keeps its cuts.  Stated over ``cdc_model.chunk`` only, so that ``chunk(edited)`` is an independent check."""
from __future__ import annotations

import bisect

import cdc_model as CM


def edited(old: bytes, a: int, r: int, ins: bytes) -> bytes:
    return old[:a] + ins + old[a + r:]


def restart(cuts, a: int) -> int:
    """The chunk that holds byte a: the last one when a == n (its end was forced by the end of the stream), 0 when there is none."""
    k = len(cuts) - 1
    return min(bisect.bisect_right(cuts, a) - 1, k - 1) if k else 0


def window_end(cuts, b: int, lookahead: int) -> int:
    """W: the first old cut >= b + lookahead, or n."""
    i = bisect.bisect_left(cuts, b + lookahead)
    return cuts[i] if i < len(cuts) else cuts[-1]


def resync(x, old, new_from: int, shift: int, keep_all: bool):
    """cw_dev_cdc_resync over plain lists: (verdict, t, s, x[t], kept count) for new cuts x[0..N] and old cuts old[0..O]."""
    at = {c: s for s, c in reversed(list(enumerate(old)))}
    for t in range(1, len(x)):
        if x[t] >= new_from and (x[t] + shift) % (1 << 64) in at:
            return 0, t, at[(x[t] + shift) % (1 << 64)], x[t], t
    return 1, 0, 0, 0, len(x) - 1 if keep_all else 0


def patch(old: bytes, cuts, p: dict, a: int, r: int, ins: bytes, lookahead: int = 0):
    """(j, t, s, new cuts, attempts): positions [0, j) of the old recipe, t chunks of the window, old positions [s, K) shifted."""
    n, k = len(old), len(cuts) - 1
    assert cuts[0] == 0 and cuts[-1] == n and 0 <= a and 0 <= r and a + r <= n
    b, delta, b2 = a + r, len(ins) - r, a + len(ins)
    new = edited(old, a, r, ins)
    j = restart(cuts, a)
    look = max(lookahead or 4 * p["max"], 2 * p["max"])
    attempts = 0
    while True:
        attempts += 1
        w = window_end(cuts, b, look)
        final = w == n
        x = [cuts[j] + c for c in CM.chunk(new[cuts[j]:w + delta], p, final=final)]
        verdict, t, s, _, kept = resync(x, cuts, b2, -delta % (1 << 64), final)
        if verdict == 0:
            return j, t, s, cuts[:j] + x[:t + 1] + [c + delta for c in cuts[s + 1:]], attempts
        if final:
            return j, kept, k, cuts[:j] + x, attempts
        look *= 2
