"""Locating damage from the guard's syndromes in plain numpy: what cw_dev_store_guard_locate and cw_dev_store_guard2_locate give
(include/cw_hashcompress.h), cell by cell and byte by byte over small stores.

S, G, W, groups, columns, members and the field are guard_model's and guard2_model's.  A CELL is one guard byte (group g, column c);
its members below the cursor are the store positions g * W + m * S + c < covered.  P' = the guard byte XOR those bytes, Q' = the Q
byte XOR the XOR of 2^m (x) those bytes.  A cell is dirty when P' != 0 (dual: or Q' != 0); a dirty dual cell with P' != 0, Q' != 0 and
Q' == 2^m (x) P' for a member m below the cursor is LOCATED(m); every other dirty cell is AMBIGUOUS.  Nothing here knows about words,
pieces or bitmaps: every cell gets its class, and an entry's bits are read off the classes of its bytes' cells, one byte at a time.
"""
import numpy as np

import guard2_model as G2
import guard_model as GM
import restore_model as RM
from guard_model import S, entry

CLEAN, AMBIGUOUS = -1, -2                      # a cell's class; m >= 0 is LOCATED(m)
LOCATED_BIT, AMBIGUOUS_BIT, UNJUDGED = 1, 2, 4


def syndromes(store, covered: int, S: int, G: int):
    """(P, Q, members) per cell of the N = ceil(covered / W) groups: the sums over the store bytes below the cursor, and how many
    members each cell has there.  The bytes at and above the cursor count as zero, which adds nothing to either sum."""
    W = G * S
    n = -(-covered // W)
    b = np.zeros(n * W, np.uint8)
    b[:covered] = np.asarray(store[:covered], np.uint8)
    b = b.reshape(n, G, S)
    weight = G2.POW[np.arange(G) % 255]                 # (G = 256 has no Q: the weights repeat, and the single call never reads it)
    p = np.bitwise_xor.reduce(b, axis=1)
    q = np.bitwise_xor.reduce(G2.MUL[weight[None, :, None], b], axis=1)
    below = (np.arange(n * W, dtype=np.int64).reshape(n, G, S) < covered).sum(axis=1)
    return p.reshape(-1), q.reshape(-1), below.reshape(-1)


def classes(store, covered: int, S: int, G: int, guard_p, guard_q=None):
    """(class, P', Q') per cell below the cursor; Q' is None for the single guard."""
    p, q, below = syndromes(store, covered, S, G)
    n = len(p)
    dp = p ^ np.asarray(guard_p[:n], np.uint8)
    cls = np.full(n, CLEAN, np.int32)
    if guard_q is None:
        cls[dp != 0] = AMBIGUOUS
        return cls, dp, None
    dq = q ^ np.asarray(guard_q[:n], np.uint8)
    cls[(dp != 0) | (dq != 0)] = AMBIGUOUS
    both = np.nonzero((dp != 0) & (dq != 0))[0]
    for m in range(min(G, G2.G2_MAX)):
        hit = both[(m < below[both]) & (G2.MUL[G2.POW[m], dp[both]] == dq[both])]
        assert (cls[hit] == AMBIGUOUS).all(), "two members fit one cell"
        cls[hit] = m
    return cls, dp, dq


def locate(store, store_bytes: int, directory, covered: int, S: int, G: int, guard_p, guard_q=None):
    """One cw_dev_store_guard_locate call, or with guard_q one cw_dev_store_guard2_locate call: (d_result[8], d_suspect or None).
    ``directory`` is RM.LOC records; dir_base plays no part."""
    directory = np.asarray(directory).view(RM.LOC).reshape(-1)
    if covered > store_bytes:
        return [1, 0, 0, 0, 0, 0, 0, 0], None
    cls, _, _ = classes(store, covered, S, G, guard_p, guard_q)
    suspect = np.zeros(len(directory), np.uint32)
    for k, e in enumerate(directory):
        if not any(int(v) for v in e):
            continue
        ext = GM.extent_of(directory, 0, k, store_bytes, covered)
        if ext is None:
            suspect[k] = UNJUDGED
            continue
        p = np.arange(ext[0], ext[0] + ext[1], dtype=np.int64)
        c = cls[GM.cells(p, S, G)]
        suspect[k] = LOCATED_BIT * bool((c == G2.members(p, S, G)).any()) | AMBIGUOUS_BIT * bool((c == AMBIGUOUS).any())
    n = -(-covered // (G * S))
    dirty, located, ambiguous = int((cls != CLEAN).sum()), int((cls >= 0).sum()), int((cls == AMBIGUOUS).sum())
    return [0, n, dirty, located, ambiguous, int(((suspect & 3) != 0).sum()), int((suspect == UNJUDGED).sum()), 0], suspect


def records(entries):
    """The hand-built entries as RM.LOC records."""
    d = np.zeros(len(entries), RM.LOC)
    for k, e in enumerate(entries):
        d[k] = e
    return d


# ---- the named cases ---------------------------------------------------------------------------------------------------------------------
def store_bytes_of(G: int, S: int = S) -> int:
    """The existing small store of 6 stripes and 37 bytes where it holds a whole group and a stripe of the next; else one whole group,
    one stripe and 37 bytes; for the largest groups, 255 and 256, W + S exactly."""
    W = G * S
    if W + S + 37 <= GM.STORE_BYTES:
        return GM.STORE_BYTES
    return W + S if G >= 255 else W + S + 37


def ratio(pd: int, qd: int) -> int:
    """log2(qd / pd): the k with 2^k (x) pd == qd; pd, qd != 0."""
    return int(np.nonzero(G2.MUL[G2.POW, pd] == qd)[0][0])


def two_errors(m: int, o: int, members: int, alias: bool):
    """Deltas (a, b) of two wrong bytes of one cell, in members m and o: P' = a ^ b and Q' = 2^m a ^ 2^o b, both non-zero, with
    k = log2(Q' / P').  alias: k < members and k not in (m, o), so the pair looks like one wrong byte of member k; else k >= members, no
    member fits.  (None, None, None) when no pair exists -- with 255 members every pair aliases, with two none does."""
    if members < 3 if alias else members >= 255:
        return None, None, None
    for a in range(1, 256):
        for b in range(1, 256):
            pd, qd = a ^ b, int(G2.MUL[G2.POW[m], a]) ^ int(G2.MUL[G2.POW[o], b])
            if pd == 0 or qd == 0:
                continue
            k = ratio(pd, qd)
            if (k < members and k not in (m, o)) if alias else k >= members:
                return a, b, k
    return None, None, None


class Case:
    """Entries, the cursor, the damage -- ("s" | "p" | "q", index, xor) on the store, P or Q -- and the case's own claim: the suspect
    words wanted from the single call and from the dual call, which the tests hold against the model."""

    def __init__(self, entries, damage, single, dual, covered=None, cells=None):
        self.entries, self.damage, self.single, self.dual, self.covered, self.cells = entries, damage, single, dual, covered, cells or {}


def cases(G: int, S: int = S):
    """{name: Case} over a store of store_bytes_of(G) bytes.  ``cells`` of a case: {store position: the class its cell must have on
    the dual call}, the edge the case is there for."""
    W, full = G * S, store_bytes_of(G, S)
    hi = G - 1                                                  # the highest member; its stripe of group 0 is whole
    last = (full - 1) // W * W                                  # the last group: fewer than G members, or for G = 1 a part of one
    x = 0x5C
    c = {}
    c["no damage"] = Case([entry(100, 400), entry(S - 700, 1500), entry(W - 901, 2000)], [], [0, 0, 0], [0, 0, 0])
    e = [entry(S + 5, 300), entry(2 * S + 1600, 64)]
    c["an extent's first byte"] = Case(e, [("s", S + 5, x)], [2, 0], [1, 0], cells={S + 5: (1 % G)})
    c["an extent's last byte"] = Case(e, [("s", S + 304, x)], [2, 0], [1, 0])
    c["the byte behind an extent"] = Case(e, [("s", S + 305, x)], [0, 0], [0, 0])
    c["pos % 16 == 0"] = Case(e, [("s", 2 * S + 1600, 1)], [0, 2], [0, 1])
    c["pos % 16 == 15"] = Case(e, [("s", 2 * S + 1615, 0x80)], [0, 2], [0, 1])
    c["member 0"] = Case([entry(4096, 500)], [("s", 4200, x)], [2], [1], cells={4200: 0})
    c["member G - 1"] = Case([entry(hi * S + 4096, 500)], [("s", hi * S + 4200, x)], [2], [1], cells={hi * S + 4200: hi})
    c["position covered - 1"] = Case([entry(full - 20, 20)], [("s", full - 1, x)], [2], [1])
    n = min(200, full - last - 3)
    c["a cell of the last group"] = Case([entry(last + 3, n)], [("s", last + 10, x)], [2], [1], cells={last + 10: 0})
    cov = full - 11
    c["covered not a multiple of 16"] = Case([entry(cov - 30, 30), entry(cov - 5, 10), entry(100, 50)], [("s", cov - 1, x), ("s", 120, 7)],
                                             [2, 4, 2], [1, 4, 1], covered=cov)
    e = [entry(S - 700, 1500), entry(3 * S + 5000, 9)]
    c["across a stripe boundary, both pieces"] = Case(e, [("s", S - 10, x), ("s", S + 10, 3)], [2, 0], [1, 0])
    c["across a stripe boundary, the first piece"] = Case(e, [("s", S - 1, x)], [2, 0], [1, 0])
    c["across a stripe boundary, the second piece"] = Case(e, [("s", S, x)], [2, 0], [1, 0])
    e = [entry(W - 901, 2000)]
    c["across a group boundary, both pieces"] = Case(e, [("s", W - 5, x), ("s", W + 5, 9)], [2], [1], cells={W - 5: hi, W + 5: 0})
    c["across a group boundary, the first piece"] = Case(e, [("s", W - 901, x)], [2], [1])
    c["across a group boundary, the second piece"] = Case(e, [("s", W + 1098, x)], [2], [1])
    # a byte no entry names, in another member of the entry's columns: the single guard suspects the entry, the dual guard locates
    # the byte in a member the entry is not in.  (G = 1: no other member; the damaged byte lies in another group)
    at = hi * S + 200 if G > 1 else 2 * S + 200
    c["a byte no entry names"] = Case([entry(100, 400)], [("s", at, x)], [2 if G > 1 else 0], [0], cells={at: hi if G > 1 else 0})
    c["a changed P byte"] = Case([entry(100, 400), entry(3 * S, 90)], [("p", 150, x)], [2, 0], [2, 0], cells={150: AMBIGUOUS})
    c["a changed Q byte"] = Case([entry(100, 400), entry(3 * S, 90)], [("q", 150, x)], [0, 0], [2, 0], cells={150: AMBIGUOUS})
    c["two entries over one extent"] = Case([entry(5000, 700), entry(5000, 700), entry(5700, 5)], [("s", 5100, x)], [2, 2, 0], [1, 1, 0])
    c["unsound, all-zero and above-cursor entries"] = Case(
        [(0, 0, 0), (S, 0, RM.RAW | 5), (100, 50, RM.RAW | 50 | 1 << 20), entry(cov - 5, 10), entry(full - 3, 4), entry(100, 50), (0, 0, 0)],
        [("s", 120, x)], [0, 4, 4, 4, 4, 2, 0], [0, 4, 4, 4, 4, 1, 0], covered=cov)
    if G > 1:
        # two wrong bytes of members 0 and 1 in one cell, each in an entry; a third entry in member 2's place of that column when
        # there is one (G = 2: in the next group, beside the point)
        e = [entry(1000, 300), entry(S + 1000, 300), entry(2 * S + 1000, 300)]
        members = min(G, -(-(full - 1100) // S))
        third = 2 if G > 2 else 0
        c["two wrong bytes, equal deltas"] = Case(e, [("s", 1100, x), ("s", S + 1100, x)], [0, 0, 0], [2, 2, third], cells={1100: AMBIGUOUS})
        a, b, k = two_errors(0, 1, members, alias=False)
        if a is not None:
            c["two wrong bytes, different deltas"] = Case(e, [("s", 1100, a), ("s", S + 1100, b)], [2, 2, third], [2, 2, third],
                                                          cells={1100: AMBIGUOUS})
        a, b, k = two_errors(0, 1, members, alias=True)
        if a is not None:
            # the pair looks like one wrong byte of member k: neither damaged entry is suspected, and an entry there would be
            e = e[:2] + [entry(k * S + 1000, 300)]
            c["two wrong bytes that alias"] = Case(e, [("s", 1100, a), ("s", S + 1100, b)], [2, 2, 2], [0, 0, 1], cells={1100: k})
    return c


def damaged(store, guard_p, guard_q, damage):
    """Copies of (store, P, Q) with a case's damage applied; Q may be None."""
    out = {"s": np.array(store, copy=True), "p": np.array(guard_p, copy=True), "q": None if guard_q is None else np.array(guard_q, copy=True)}
    for what, at, xor in damage:
        if out[what] is not None:
            out[what][at] ^= np.uint8(xor)
    return out["s"], out["p"], out["q"]
