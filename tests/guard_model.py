"""XOR guard stripes in plain numpy: what cw_store_guard_bytes, cw_dev_store_guard_update, cw_dev_store_guard_check and
cw_dev_store_guard_rebuild give (include/cw_hashcompress.h), byte by byte and by brute force over small stores.

S = stripe, G = group, W = G * S.  Store byte p belongs to group p // W and column p % S, and guard[g * S + c] is the XOR of the store
bytes below the cursor `covered` with that group and column.  Nothing here knows about stripes' members, words, pieces or buckets:
the guard is summed byte by byte, a collision is two different bytes of the listed extents in one (group, column) cell, and a rebuilt
byte is the guard byte XOR every other byte of its cell below the cursor.
"""
import numpy as np

import restore_model as RM

S_MIN, S_MAX, G_MAX = 65536, 1 << 30, 256
REBUILT, COLLIDES, UNPROTECTED = 0, 1, 2
NONE = 2 ** 64 - 1


def geometry_ok(S: int, G: int) -> bool:
    return S_MIN <= S <= S_MAX and S & (S - 1) == 0 and 1 <= G <= G_MAX


def guard_bytes(store_bytes: int, S: int, G: int) -> int:
    """cw_store_guard_bytes."""
    return -(-store_bytes // (G * S)) * S if geometry_ok(S, G) else 0


def cells(p, S: int, G: int):
    """The guard index of every store position in p (an int64 array)."""
    p = np.asarray(p, np.int64)
    return p // (G * S) * S + p % S


def fold(guard, store, lo: int, hi: int, S: int, G: int) -> None:
    """guard ^= the store bytes [lo, hi), each into its cell."""
    p = np.arange(lo, hi, dtype=np.int64)
    np.bitwise_xor.at(guard, cells(p, S, G), np.asarray(store[lo:hi], np.uint8))


def guard_of(store, covered: int, S: int, G: int, store_bytes: int):
    """The guard of the bytes below `covered`, from nothing."""
    guard = np.zeros(guard_bytes(store_bytes, S, G), np.uint8)
    fold(guard, store, 0, covered, S, G)
    return guard


def update(guard, store, store_bytes: int, used: int, covered: int, S: int, G: int):
    """One cw_dev_store_guard_update call: (d_result[4], the new cursor); the guard changes in place."""
    if covered > used or used > store_bytes:
        return [1, covered, used, 0], covered
    fold(guard, store, covered, used, S, G)
    return [0, covered, used, used - covered], used


def check(guard, store, store_bytes: int, covered: int, S: int, G: int):
    """One cw_dev_store_guard_check call: (d_result[4], the flag of every group below the cursor)."""
    if covered > store_bytes:
        return [1, 0, 0, NONE], np.zeros(0, np.uint32)
    n = -(-covered // (G * S))
    want = guard_of(store, covered, S, G, store_bytes)
    bad = (want[:n * S].reshape(n, S) != np.asarray(guard[:n * S]).reshape(n, S)).any(axis=1).astype(np.uint32)
    which = np.nonzero(bad)[0]
    return [0, n, len(which), int(which[0]) if len(which) else NONE], bad


def sound(entry, store_bytes: int) -> bool:
    """Entry::sound of store_device.h (cw_dev_store_compact's entry checks)."""
    pos, stored, word = (int(v) for v in entry)
    length, raw = word & RM.LEN_MASK, bool(word & RM.RAW)
    return (word & ~(RM.RAW | RM.LEN_MASK)) == 0 and 1 <= length <= 65536 and stored != 0 and (not raw or stored == length) and \
        pos <= store_bytes and stored <= store_bytes - pos


def extent_of(directory, dir_base: int, value: int, store_bytes: int, covered: int):
    """(pos, stored) of a protected position, else None."""
    idx = value - dir_base
    if value < dir_base or idx >= len(directory):
        return None
    e = directory[idx]
    if not any(int(v) for v in e) or not sound(e, store_bytes) or int(e["pos"]) + int(e["stored"]) > covered:
        return None
    return int(e["pos"]), int(e["stored"])


def rebuild(store, store_bytes: int, directory, dir_base: int, covered: int, S: int, G: int, guard, values, out_bytes: int):
    """One cw_dev_store_guard_rebuild call: (d_result[4], statuses, the payload or None, d_out_loc as RM.LOC or None); payload and
    locs are None unless the verdict is 0."""
    values = [int(v) for v in values]
    n = len(values)
    status = np.full(n, UNPROTECTED, np.uint32)
    if covered > store_bytes:
        return [2, 0, n, 0], status, None, None
    store, guard, W = np.asarray(store, np.uint8), np.asarray(guard, np.uint8), G * S
    ext = [extent_of(directory, dir_base, v, store_bytes, covered) for v in values]
    # the SET of bytes the protected positions list, and the cells that hold two different ones
    listed = [np.arange(e[0], e[0] + e[1], dtype=np.int64) for e in ext if e is not None]
    hot = np.zeros(0, np.int64)
    if listed:
        cell, count = np.unique(cells(np.unique(np.concatenate(listed)), S, G), return_counts=True)
        hot = cell[count > 1]
    out, locs, at = [], np.zeros(n, RM.LOC), 0
    for k, e in enumerate(ext):
        if e is None:
            continue
        p = np.arange(e[0], e[0] + e[1], dtype=np.int64)
        if np.isin(cells(p, S, G), hot).any():
            status[k] = COLLIDES
            continue
        status[k] = REBUILT
        v = guard[cells(p, S, G)].copy()
        for m in range(G):
            q = p // W * W + m * S + p % S
            take = (q < covered) & (q != p)
            v[take] ^= store[q[take]]
        locs[k] = (at, e[1], int(directory[values[k] - dir_base]["raw"]))
        out.append(v)
        at += len(v)
    total, rebuilt = at, int((status == REBUILT).sum())
    if total > out_bytes:
        return [1, total, n, rebuilt], status, None, None
    return [0, total, n, rebuilt], status, np.concatenate(out) if out else np.zeros(0, np.uint8), locs


# ---- the named cases ---------------------------------------------------------------------------------------------------------------------
S = 65536


def entry(pos: int, stored: int):
    """A raw entry of `stored` bytes at pos."""
    return (pos, stored, RM.RAW | (stored & RM.LEN_MASK))


def update_ranges(G: int, S: int = S, store_bytes: int = None):
    """{name: (covered, used)} over a store of 6 stripes and 37 bytes, or of ``store_bytes`` >= 2 * S + 1002."""
    W, store_bytes = G * S, 6 * S + 37 if store_bytes is None else store_bytes
    r = {}
    for n in (1, 15, 16, 17):
        for at in (0, 1, 15):
            r[f"{n} bytes at {at} mod 16"] = (S + 4096 + at, S + 4096 + at + n)
    r["inside one stripe"] = (S + 100, S + 30000)
    r["across a stripe boundary"] = (S - 1000, S + 1001)
    r["across a group boundary"] = (W - 77, W + 33)
    r["W bytes"] = (S // 2 + 5, S // 2 + 5 + W)
    r["more than W bytes"] = (3, min(W + S + 900, store_bytes))
    r["everything"] = (0, store_bytes)
    assert all(a <= b <= store_bytes for a, b in r.values()), (G, S, store_bytes)
    r["nothing"] = (S + 7, S + 7)
    return r


STORE_BYTES = 6 * S + 37


def rebuild_cases(G: int, S: int = S, store_bytes: int = None):
    """{name: (directory entries, values, covered, the statuses wanted)} over a store of 6 stripes and 37 bytes, or of ``store_bytes``
    >= max(6 * S, G * S + S); dir_base 0; the statuses are the cases' own claim, which the tests hold against the brute-force rebuild."""
    W = G * S
    full = 6 * S + 37 if store_bytes is None else store_bytes
    assert full >= max(6 * S, W + S), (G, S, full)
    c = {}
    c["one byte"] = ([entry(S + 5, 1)], [0], full, [0])
    c["S bytes from mid-stripe"] = ([entry(S // 2 + 3, min(S, 65536))], [0], full, [0])
    if S > 65536:
        c["65536 bytes from the last column"] = ([entry(S - 1, 65536)], [0], full, [0])
    c["across a stripe boundary"] = ([entry(S - 700, 1500)], [0], full, [0])
    c["across a group boundary"] = ([entry(W - 901, 2000)], [0], full, [0])
    # two extents of one group, in different stripes, whose columns touch but do not overlap
    c["adjacent columns"] = ([entry(100, 400), entry(S + 500, 300)], [0, 1], full, [0, 0])
    if G > 1:
        # ... and sharing exactly one column (499), with a third extent elsewhere
        c["one shared column"] = ([entry(100, 400), entry(S + 499, 300), entry(W + 9000, 777)], [0, 1, 2], full, [1, 1, 0])
    c["a value twice"] = ([entry(3 * S - 50, 4000)], [0, 0], full, [0, 0])
    c["ends at covered"] = ([entry(4 * S + 10, 990)], [0], 4 * S + 1000, [0])
    c["ends above covered"] = ([entry(4 * S + 10, 991)], [0], 4 * S + 1000, [2])
    c["unprotected"] = ([(0, 0, 0), (S, 0, RM.RAW | 5), entry(5 * S, 100)], [0, 1, 7, RM.MISS, 2], full, [2, 2, 2, 2, 0])
    if G == G_MAX:
        # the two highest members at disjoint columns, then with columns in common; the last member into the next group beside member 254
        c["members 254 and 255"] = ([entry(254 * S + 70, 4000), entry(255 * S + 5000, 4000)], [0, 1], full, [0, 0])
        c["members 254 and 255 collide"] = ([entry(254 * S + 70, 4000), entry(255 * S + 2000, 4000)], [0, 1], full, [1, 1])
        c["from member 255 into the next group"] = ([entry(W - 600, 1500), entry(254 * S + 62000, 500)], [0, 1], full, [0, 0])
        c["from member 255 into the next group, colliding"] = ([entry(W - 600, 1500), entry(255 * S - 300, 200)], [0, 1], full, [1, 1])
    return c
