"""cw_dev_read_ranges in plain Python, on top of restore_model.restore: every position of the recipe is restored once (without
the chunk's destination check, which the ranged call does not have), and a range's verdict and bytes are put together from the
positions it touches, as the header states them."""
from __future__ import annotations

import restore_model as RM

U64 = 1 << 64


def read(store, store_bytes, directory, dir_base, refs, raw_offsets, ranges, dst_bytes, decode):
    """One call: [(status, bytes or None)] per range of `ranges` = [(offset, length, destination offset)]."""
    n = len(refs)
    ro = [int(v) for v in raw_offsets[:n + 1]]
    pieces = RM.restore(store, store_bytes, directory, dir_base, refs, ro, U64, decode)
    out = []
    for a, length, to in ranges:
        if length == 0:
            out.append((0, b""))
        elif n == 0 or a < ro[0] or a + length >= U64 or a + length > ro[n] or to + length >= U64 or to + length > dst_bytes:
            out.append((3, None))
        else:
            touched = [j for j in range(n) if ro[j] < ro[j + 1] and ro[j] < a + length and a < ro[j + 1]]
            status = max(pieces[j][0] for j in touched)
            got = b"".join(pieces[j][1][max(a, ro[j]) - ro[j]:min(a + length, ro[j + 1]) - ro[j]] for j in touched) if status == 0 else None
            out.append((status, got))
    return out
