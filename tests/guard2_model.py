"""The dual guard in plain numpy: what cw_dev_store_guard2_update, cw_dev_store_guard2_check and cw_dev_store_guard2_rebuild give
(include/cw_hashcompress.h), byte by byte and by brute force over small stores.

S, G, W, groups, columns and the XOR guard P are guard_model's.  The field is GF(2^8) with x^8 + x^4 + x^3 + x^2 + 1 (0x11D), built here
by repeated doubling alone; Q[g * S + c] is the XOR of 2^m (x) store[p] over the bytes below the cursor of that group and column, m =
(p // S) % G.  Nothing here knows about words, pieces or buckets: Q is summed byte by byte, a cell is hot when three different listed
bytes lie in it, and a rebuilt byte D of member m with the cell's one other listed byte in member o is
    D = (Q' ^ 2^o (x) P') (x) inv(2^m ^ 2^o),        P', Q' = the guard bytes less every known byte of the cell below the cursor,
or P' when the cell holds no other listed byte.
"""
import numpy as np

import guard_model as GM
import restore_model as RM
from guard_model import NONE, REBUILT, COLLIDES, UNPROTECTED, S, STORE_BYTES, cells, entry, extent_of, guard_bytes  # noqa: F401

G2_MAX = 255
POLY = 0x11D


def double(x: int) -> int:
    """2 (x) x."""
    x <<= 1
    return x ^ POLY if x & 0x100 else x


def times(a: int, b: int) -> int:
    """a (x) b: b doubled once per bit of a."""
    r = 0
    while a:
        if a & 1:
            r ^= b
        a, b = a >> 1, double(b)
    return r


POW = np.zeros(255, np.uint8)                      # POW[i] = 2^i, i < 255
_x = 1
for _i in range(255):
    POW[_i] = _x
    _x = double(_x)
MUL = np.array([[times(a, b) for b in range(256)] for a in range(256)], np.uint8)
INV = np.zeros(256, np.uint8)                      # INV[a] (x) a == 1, a != 0
for _a in range(1, 256):
    INV[_a] = int(np.nonzero(MUL[_a] == 1)[0][0])


def geometry_ok(S: int, G: int) -> bool:
    return GM.geometry_ok(S, G) and G <= G2_MAX


def members(p, S: int, G: int):
    p = np.asarray(p, np.int64)
    return p // S % G


def fold_q(guard_q, store, lo: int, hi: int, S: int, G: int) -> None:
    """guard_q ^= 2^m (x) the store bytes [lo, hi), each into its cell."""
    p = np.arange(lo, hi, dtype=np.int64)
    np.bitwise_xor.at(guard_q, cells(p, S, G), MUL[POW[members(p, S, G)], np.asarray(store[lo:hi], np.uint8)])


def guards_of(store, covered: int, S: int, G: int, store_bytes: int):
    """(P, Q) of the bytes below `covered`, from nothing."""
    p, q = (np.zeros(guard_bytes(store_bytes, S, G), np.uint8) for _ in range(2))
    GM.fold(p, store, 0, covered, S, G)
    fold_q(q, store, 0, covered, S, G)
    return p, q


def update(guard_p, guard_q, store, store_bytes: int, used: int, covered: int, S: int, G: int):
    """One cw_dev_store_guard2_update call: (d_result[4], the new cursor); both guards change in place."""
    if covered > used or used > store_bytes:
        return [1, covered, used, 0], covered
    GM.fold(guard_p, store, covered, used, S, G)
    fold_q(guard_q, store, covered, used, S, G)
    return [0, covered, used, used - covered], used


def check(guard_p, guard_q, store, store_bytes: int, covered: int, S: int, G: int):
    """One cw_dev_store_guard2_check call: (d_result[4], the bits of every group below the cursor)."""
    if covered > store_bytes:
        return [1, 0, 0, NONE], np.zeros(0, np.uint32)
    n = -(-covered // (G * S))
    bits = np.zeros(n, np.uint32)
    for bit, want, have in zip((1, 2), guards_of(store, covered, S, G, store_bytes), (guard_p, guard_q)):
        bits |= (want[:n * S].reshape(n, S) != np.asarray(have[:n * S]).reshape(n, S)).any(axis=1).astype(np.uint32) * np.uint32(bit)
    which = np.nonzero(bits)[0]
    return [0, n, len(which), int(which[0]) if len(which) else NONE], bits


def rebuild(store, store_bytes: int, directory, dir_base: int, covered: int, S: int, G: int, guard_p, guard_q, values, out_bytes: int):
    """One cw_dev_store_guard2_rebuild call: (d_result[5], statuses, the payload or None, d_out_loc as RM.LOC or None); payload and
    locs are None unless the verdict is 0."""
    values = [int(v) for v in values]
    n = len(values)
    status = np.full(n, UNPROTECTED, np.uint32)
    if covered > store_bytes:
        return [2, 0, n, 0, 0], status, None, None
    store, guard_p, guard_q, W = np.asarray(store, np.uint8), np.asarray(guard_p, np.uint8), np.asarray(guard_q, np.uint8), G * S
    ext = [extent_of(directory, dir_base, v, store_bytes, covered) for v in values]
    # the SET of bytes the protected positions list, sorted by cell; the cells that hold three different ones
    listed = [np.arange(e[0], e[0] + e[1], dtype=np.int64) for e in ext if e is not None]
    lb = np.unique(np.concatenate(listed)) if listed else np.zeros(0, np.int64)
    lb = lb[np.argsort(cells(lb, S, G), kind="stable")]
    lc = cells(lb, S, G)
    cell, count = np.unique(lc, return_counts=True)
    hot = cell[count > 2]
    out, locs, paired, at = [], np.zeros(n, RM.LOC), 0, 0
    for k, e in enumerate(ext):
        if e is None:
            continue
        p = np.arange(e[0], e[0] + e[1], dtype=np.int64)
        c = cells(p, S, G)
        if np.isin(c, hot).any():
            status[k] = COLLIDES
            continue
        status[k] = REBUILT
        # the one other listed byte of each cell, or -1: a cell that is not hot lists p and at most one more
        lo, hi = np.searchsorted(lc, c, "left"), np.searchsorted(lc, c, "right")
        first, last = lb[lo], lb[hi - 1]
        other = np.where(hi - lo == 2, np.where(first == p, last, first), -1)
        pp, qq = guard_p[c].copy(), guard_q[c].copy()
        for m in range(G):
            q = p // W * W + m * S + p % S
            take = (q < covered) & (q != p) & (q != other)                       # the known bytes of the cell
            pp[take] ^= store[q[take]]
            qq[take] ^= MUL[POW[m], store[q[take]]]
        v, two = pp.copy(), other >= 0
        wm, wo = POW[members(p[two], S, G)], POW[members(other[two], S, G)]
        v[two] = MUL[qq[two] ^ MUL[wo, pp[two]], INV[wm ^ wo]]
        paired += bool(two.any())
        locs[k] = (at, e[1], int(directory[values[k] - dir_base]["raw"]))
        out.append(v)
        at += len(v)
    total, rebuilt = at, int((status == REBUILT).sum())
    if total > out_bytes:
        return [1, total, n, rebuilt, paired], status, None, None
    return [0, total, n, rebuilt, paired], status, np.concatenate(out) if out else np.zeros(0, np.uint8), locs


# ---- the named cases ---------------------------------------------------------------------------------------------------------------------
STORE_BYTES_255 = 255 * S + S + 37               # one whole group of 255 stripes, one stripe of the next and a few bytes


def update_range_255():
    """(covered, used) across the boundary from member 254 of group 0 to member 0 of group 1, G = 255."""
    return 255 * S - 4099, 255 * S + 5003


def rebuild_cases(G: int, store_bytes: int = STORE_BYTES, S: int = S, single: bool = None):
    """{name: (directory entries, values, covered, the statuses wanted, the positions that need Q)}: guard_model's cases -- "one shared
    column" now rebuilds all three -- and the ones the second syndrome adds.  dir_base 0; statuses and the need for Q are the cases'
    own claims, which the tests hold against the two brute-force rebuilds.  ``single`` says whether guard_model's cases are among them:
    by default, over the store of 6 stripes and 37 bytes only."""
    W, full = G * S, store_bytes
    c = {}
    if store_bytes == STORE_BYTES and S == GM.S if single is None else single:
        for name, (entries, values, covered, wanted) in GM.rebuild_cases(G, S, store_bytes).items():
            c[name] = (entries, values, covered, wanted, [])
        if G > 1:
            e, v, cov, _, _ = c["one shared column"]
            c["one shared column"] = (e, v, cov, [0, 0, 0], [0, 1])
    if G > 1:
        hi = G - 1                                # the highest member; members 0 and hi of group 0
        c["a pair that overlaps wholly"] = ([entry(1000, 3000), entry(hi * S + 1000, 3000)], [0, 1], full, [0, 0], [0, 1])
        # the boundary inside one 4-byte word: the one ends at column 4k + 2, the other (member hi) starts at column 4k + 1
        c["a boundary inside a word"] = ([entry(4 * 500 - 300, 302), entry(hi * S + 4 * 500 + 1, 200)], [0, 1], full, [0, 0], [0, 1])
        c["a value twice with a partner"] = ([entry(7000, 900), entry(hi * S + 7500, 900)], [0, 1, 0], full, [0, 0, 0], [0, 1, 2])
        c["a partner that ends at covered"] = ([entry(20000, 500), entry(hi * S + 20100, 400)], [0, 1], hi * S + 20500, [0, 0], [0, 1])
        c["a listed extent above covered"] = ([entry(20000, 500), entry(hi * S + 20100, 401)], [0, 1], hi * S + 20500, [0, 2], [])
        c["members 0 and G - 1"] = ([entry(33, 65536 - 33), entry(hi * S + 5, 65000)], [1, 0], full, [0, 0], [0, 1])
        # a pair across a group boundary: the first in member G - 1 wrapping to member 0 of group 1, the partner in member 1 of group 1
        if store_bytes >= W + 2 * S:
            c["a pair across a group boundary"] = ([entry(W - 600, 1500), entry(W + S + 200, 1000)], [0, 1], full, [0, 0], [0, 1])
    if G == 2:
        # nothing can be hot: three extents over one column are two members
        c["G = 2: three extents, two members"] = ([entry(100, 500), entry(S + 200, 500), entry(300, 500)], [0, 1, 2], full, [0, 0, 0], [0, 1, 2])
    if G > 2:
        c["three members over one column"] = ([entry(9000, 100), entry(S + 9050, 100), entry(2 * S + 9099, 100), entry(40000, 50)], [0, 1, 2, 3],
                                              full, [1, 1, 1, 0], [])
        c["three extents, pairwise at disjoint columns"] = ([entry(1000, 200), entry(S + 1150, 200), entry(2 * S + 900, 150)], [0, 1, 2], full,
                                                            [0, 0, 0], [0, 1, 2])
        # A meets only B; B is hot elsewhere with C and D
        c["a partner that is hot elsewhere"] = ([entry(50000, 100), entry(S + 50050, 1000), entry(50900, 50), entry(2 * S + 50920, 50)],
                                                [0, 1, 2, 3], full, [0, 1, 1, 1], [0])
    if G == 255:
        c["members 253 and 254"] = ([entry(253 * S + 70, 4000), entry(254 * S + 2000, 4000)], [0, 1], full, [0, 0], [0, 1])
    return c
