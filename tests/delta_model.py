"""Reference model of the recipe diff and of the delta it yields (include/cw_hashcompress.h: cw_dev_recipe_diff and
cw_dev_apply_delta), over plain lists.

A recipe is (ref[0..n), off[0..n]): position j is the chunk of value ref[j] and covers stream bytes [off[j], off[j+1]).  Equal refs
mean equal bytes, so ``diff`` looks at no data.  An op is the tuple (b_off, len, a_off, payload_off) in zero-based coordinates,
exactly one of a_off and payload_off being NONE.  ``apply`` rebuilds the new bytes from the old ones and the payload; ``check`` is
the verdict cw_dev_apply_delta reaches on an op list it does not trust."""
from __future__ import annotations

from bisect import bisect_left

M = 1 << 64
NONE = M - 1              # CW_DELTA_NONE
MAX_CHUNK = 65536
TOTALS = ("verdict", "ops", "new_ops", "in_place_bytes", "moved_bytes", "new_bytes", "matched_positions", "positions")


def sound(off, n) -> bool:
    """off[0..n] ascends strictly and every extent is 1..65536 bytes"""
    return all(0 < int(off[j + 1]) - int(off[j]) <= MAX_CHUNK for j in range(n))


def sources(ref_a, off_a, ref_b, off_b, dir_base, dir_entries):
    """(src, kind) per position of B: src = the zero-based offset in A its bytes come from or NONE; kind 0 new, 1 in place, 2 moved"""
    na, nb = len(ref_a), len(ref_b)
    za = [int(off_a[j]) - int(off_a[0]) for j in range(na + 1)] if na else [0]
    lowest = {}                                   # directory index -> the lowest A position that names it
    for j in range(na):
        idx = (int(ref_a[j]) - dir_base) % M
        if idx < dir_entries and idx not in lowest:
            lowest[idx] = j
    src, kind = [], []
    for i in range(nb):
        zb, length, r = int(off_b[i]) - int(off_b[0]), int(off_b[i + 1]) - int(off_b[i]), int(ref_b[i])
        idx = (r - dir_base) % M
        s, k = NONE, 0
        if idx < dir_entries:
            j = bisect_left(za, zb, 0, na)        # the A position that starts at zb, if there is one
            if j < na and za[j] == zb and int(ref_a[j]) == r and za[j + 1] - za[j] == length:
                s, k = zb, 1
            else:
                j = lowest.get(idx)
                if j is not None and za[j + 1] - za[j] == length:
                    s, k = za[j], 2
        src.append(s)
        kind.append(k)
    return src, kind


def diff(ref_a, off_a, ref_b, off_b, dir_base=0, dir_entries=1 << 32, max_ops=None):
    """dict(verdict, ops, src, ranges, totals): what cw_dev_recipe_diff writes.  verdict 1: nothing else is defined (None).  verdict 2
    (more ops than max_ops): ops and ranges are empty, src and totals are complete.  ranges = the new ops as (off in B's raw
    coordinates, len, payload_off)."""
    na, nb = len(ref_a), len(ref_b)
    assert len(off_a) >= na + 1 and len(off_b) >= nb + 1
    if not (sound(off_a, na) and sound(off_b, nb)):
        return dict(verdict=1, ops=None, src=None, ranges=None, totals=[1] + [None] * 7)
    src, kind = sources(ref_a, off_a, ref_b, off_b, dir_base, dir_entries)
    b0 = int(off_b[0]) if nb else 0
    ops, payload = [], 0
    for i in range(nb):
        length = int(off_b[i + 1]) - int(off_b[i])
        new = src[i] == NONE
        if i and ((new and src[i - 1] == NONE) or
                  (not new and src[i - 1] != NONE and src[i] == src[i - 1] + int(off_b[i]) - int(off_b[i - 1]))):
            ops[-1][1] += length
        else:
            ops.append([int(off_b[i]) - b0, length, src[i], NONE] if not new else [int(off_b[i]) - b0, length, NONE, payload])
        if new:
            payload += length
    ops = [tuple(o) for o in ops]
    lens = [int(off_b[i + 1]) - int(off_b[i]) for i in range(nb)]
    by = lambda k: sum(n for n, kk in zip(lens, kind) if kk == k)  # noqa: E731
    new_ops = [o for o in ops if o[2] == NONE]
    totals = [0, len(ops), len(new_ops), by(1), by(2), by(0), sum(k != 0 for k in kind), nb]
    if max_ops is not None and len(ops) > max_ops:
        totals[0] = 2
        return dict(verdict=2, ops=[], src=src, ranges=[], totals=totals)
    return dict(verdict=0, ops=ops, src=src, ranges=[(o[0] + b0, o[1], o[3]) for o in new_ops], totals=totals)


def payload_of(new: bytes, ops) -> bytes:
    """the new ops' bytes back to back, in op order: what a delta carries"""
    return b"".join(new[o[0]:o[0] + o[1]] for o in ops if o[2] == NONE)


def check(ops, old_bytes: int, payload_bytes: int, dst_bytes: int):
    """(verdict, total, lowest bad op or NONE, n) as cw_dev_apply_delta's d_result: 1 = a malformed list (total 0), 2 = the
    destination is too small"""
    end = 0
    for k, (b, n, a, p) in enumerate(ops):
        ok = b == end and n >= 1 and b + n < M and (a == NONE) != (p == NONE)
        ok = ok and ((n <= old_bytes and a <= old_bytes - n) if a != NONE else (n <= payload_bytes and p <= payload_bytes - n))
        if not ok:
            return 1, 0, k, len(ops)
        end = b + n
    return (2 if end > dst_bytes else 0), end, NONE, len(ops)


def apply(old: bytes, payload: bytes, ops) -> bytes:
    verdict, total, bad, _ = check(ops, len(old), len(payload), M)
    if verdict:
        raise ValueError(f"op {bad} is malformed")
    out = bytearray(total)
    for b, n, a, p in ops:
        out[b:b + n] = old[a:a + n] if a != NONE else payload[p:p + n]
    return bytes(out)
