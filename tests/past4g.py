"""Helpers of the tests that put byte positions past 2^32 through the chunk path.  No GPU import at module
level: everything here but ``tiled_source`` is plain numpy and is itself tested on the CPU, in tests/test_past4g_model.py.

Four devices carry a position over ``B = 2^32`` without a source that the Python models would have to walk:

* **hand-made cuts** (``hand_cuts``): 64 KiB chunks everywhere but in *the window* ``[B - 1 MiB, B + 1 MiB)``, where a few hundred chunks
  of 1 .. 65536 bytes lie at odd offsets.  The oracle sees the window's bytes only; the bulk is pinned to the fixed-block calls.
* **the restart property** of the chunker: ``chunk(data)[j:] == c_j + chunk(data[c_j:])`` whenever ``min_size >= 64`` (the hash window is
  64 bytes and no candidate lies within ``min_size`` of a cut), so the cuts of a suffix that starts at a cut are the tail of the whole
  stream's cuts, and relative to the suffix every offset is small.
* **the lifted twin** of a store: the same calls on a store whose cursor started at ``L`` leave the ordinary store's state under
  ``pos -> pos + L`` (``translate`` / ``same_directory``).  Its guard is a plain shift of the ordinary guard by ``L / W`` groups only when
  ``L`` is a multiple of the group size ``W = stripe * group`` (``guard_lift``): the bytes below ``L`` are zero and add nothing to P or Q,
  and a stripe keeps its member index within its group.
* **the tiled recipe** (``tiled_recipe``), below.

``tiled_recipe`` repeats a small stream's recipe until its offsets pass ``B``: a valid recipe of the stream ``bytes * R`` over a store
of a few MiB.  ``spliced`` states the equivalence the patch / compose tests rest on."""
from __future__ import annotations

import numpy as np

B = 1 << 32
MIB = 1 << 20
N = B + 8 * MIB                                    # the smallest source that has a window and whole blocks behind it
WIN_LO, WIN_HI = B - MIB, B + MIB
BLOCK = 65536
VARIANTS = ("ends", "straddle")                    # a cut at B and a chunk over B exclude each other: two cut lists
_LENGTHS = (1, 2, 3, 15, 16, 17, 255, 256, 257, 4095, 4097, 65535, 65536)


# ---- hand-made cuts -----------------------------------------------------------------------------------------------------------------
def anchors(variant: str, b: int = B) -> list:
    """The cuts a variant has to contain: "ends" has chunks that end at b - 1, b and b + 1; "straddle" has one chunk of 65536 bytes
    that starts at b - 17, a position = 15 (mod 16) just below b, and so lies over b with its first byte below it."""
    return [b - 1, b, b + 1] if variant == "ends" else [b - 17, b - 17 + BLOCK]


def hand_cuts(variant: str, n: int = N, b: int = B, half: int = MIB) -> np.ndarray:
    """Cuts 0 .. n (u64): 64 KiB chunks up to b - half, chunks of 1 .. 65536 bytes at odd offsets through the anchors up to b + half,
    64 KiB chunks again up to n.  ``b``, ``half`` and ``n`` are multiples of 64 KiB."""
    assert b % BLOCK == 0 and half % BLOCK == 0 and n % BLOCK == 0 and half >= 2 * BLOCK and n >= b + half
    rng = np.random.default_rng(VARIANTS.index(variant) + 41)
    lo, hi = b - half, b + half
    cuts, pos = list(range(0, lo + 1, BLOCK)), lo
    for stop in anchors(variant, b) + [hi]:
        while pos < stop:
            l = int(rng.choice(_LENGTHS)) if rng.random() < 0.25 else int(rng.integers(1, 12000))
            pos += stop - pos if stop - pos == BLOCK and pos == b - 17 else min(l, stop - pos)   # a chunk never passes an anchor
            cuts.append(pos)
    return np.array(cuts + list(range(hi + BLOCK, n + 1, BLOCK)), np.uint64)


def window_chunks(cuts, b: int = B, half: int = MIB) -> np.ndarray:
    """The chunks that lie in the window."""
    c = np.asarray(cuts, np.uint64).astype(np.int64)
    return np.nonzero((c[:-1] >= b - half) & (c[1:] <= b + half))[0]


def reaches(starts, ends, b: int = B) -> dict:
    """How many extents [start, end) end at or below b, start at or above it, and lie over it."""
    s, e = np.asarray(starts, np.uint64).astype(np.int64), np.asarray(ends, np.uint64).astype(np.int64)
    keep = e > s
    s, e = s[keep], e[keep]
    return dict(below=int((e <= b).sum()), above=int((s >= b).sum()), over=int(((s < b) & (e > b)).sum()))


def assert_reaches(starts, ends, what: str, b: int = B, over: bool = True) -> None:
    """A run whose compared extents stayed on one side of b fails rather than passing."""
    r = reaches(starts, ends, b)
    assert r["below"] and r["above"] and (r["over"] or not over), (what, "did not reach both sides of 2^32", r)


def tiled_source(torch, corpus: np.ndarray, n: int, noise, b: int = B, half: int = MIB):
    """``n`` bytes on the device: the corpus tiled, with every third 64 KiB block of the window replaced by ``noise(first, count, dst)``
    (incompressible bytes, so LZF both accepts and refuses chunks in the window).  Blocks 15 and 16 of the window, on either side of
    b, are text: a chunk across b compresses with both codecs."""
    src = torch.from_numpy(corpus).cuda().repeat(n // len(corpus) + 1)[:n].contiguous()
    for j in range(2, 2 * half // BLOCK, 3):
        at = b - half + j * BLOCK
        noise(at // BLOCK, 1, src[at:at + BLOCK])
    return src


# ---- tiled recipes ------------------------------------------------------------------------------------------------------------------
def tiled_recipe(refs, offsets, R: int):
    """(refs, offsets) of the stream ``bytes * R``: the refs R times, the offsets accumulated."""
    refs, off = np.asarray(refs, np.uint64), np.asarray(offsets, np.uint64)
    off = off - off[0]
    T, K = int(off[-1]), len(refs)
    tiles = (np.arange(R, dtype=np.uint64) * np.uint64(T))[:, None] + off[None, :K]
    return np.tile(refs, R), np.concatenate([tiles.reshape(-1), np.array([R * T], np.uint64)])


def tiles_for(T: int, past: int = B + 2 * MIB) -> int:
    """The fewest tiles of T bytes that pass ``past``."""
    return past // T + 1


def spliced(refs, offsets, R: int, head: int, m: int, mid_refs, mid_offsets):
    """The long result of an edit inside the tiles [head, head + m) of an R-tile recipe, from the short run of the same edit (its offsets
    less head * T) on an m-tile recipe: the ``head`` untouched tiles before, the short run's recipe, the R - head - m untouched tiles
    after, with the offsets shifted.  It holds when the edit's window stays inside the m tiles and, for an edit that leaves tiles
    behind it, when the short run resynchronised before its last tile's end.  It rests on the restart property: the window starts at
    a cut of the old recipe, and whatever a chunker does from a cut on depends on nothing before it."""
    refs, off = np.asarray(refs, np.uint64), np.asarray(offsets, np.uint64)
    T = int(off[-1] - off[0])
    mid_refs, mid_off = np.asarray(mid_refs, np.uint64), np.asarray(mid_offsets, np.uint64)
    grown = int(mid_off[-1]) - m * T                                       # what the edit added to the stream (may be negative)
    head_r, head_o = tiled_recipe(refs, off, head)
    tail_r, tail_o = tiled_recipe(refs, off, R - head - m)
    return (np.concatenate([head_r, mid_refs, tail_r]),
            np.concatenate([head_o[:-1], mid_off[:-1] + np.uint64(head * T), tail_o + np.uint64((head + m) * T + grown)]))


# ---- the lifted twin ----------------------------------------------------------------------------------------------------------------
LOC = np.dtype([("pos", "<u8"), ("stored", "<u4"), ("raw", "<u4")])          # cw_chunk_loc


def translate(directory, lift: int) -> np.ndarray:
    """The directory of the lifted twin: every non-zero entry's ``pos`` moved up by ``lift``; an all-zero entry names no chunk and stays."""
    d = np.array(np.asarray(directory).view(LOC).reshape(-1), copy=True)
    live = (d["pos"] != 0) | (d["stored"] != 0) | (d["raw"] != 0)
    d["pos"][live] += np.uint64(lift)
    return d


def same_directory(plain, twin, lift: int):
    """None when ``twin`` is ``plain`` under pos -> pos + lift, else (index, twin's entry, the entry wanted, how many differ)."""
    want, got = translate(plain, lift), np.asarray(twin).view(LOC).reshape(-1)
    if len(want) != len(got):
        return (-1, len(got), len(want), abs(len(got) - len(want)))
    bad = np.nonzero(want != got)[0]
    return None if len(bad) == 0 else (int(bad[0]), got[bad[0]].tolist(), want[bad[0]].tolist(), len(bad))


def extents(directory):
    """(starts, ends) of the non-zero entries' stored bytes."""
    d = np.asarray(directory).view(LOC).reshape(-1)
    d = d[d["stored"] != 0]
    return d["pos"], d["pos"] + d["stored"].astype(np.uint64)


def lift_over(directory, b: int = B) -> int:
    """The lift that puts b into the middle of the stored chunk nearest to the middle of the stored bytes: about half of the store
    then lies below b, and one entry lies over it."""
    s, e = extents(directory)
    assert len(s), "nothing stored"
    mid = int(e.max()) // 2
    i = int(np.argmin(np.abs((s + e).astype(np.int64) // 2 - mid)))
    at = int(s[i]) + max(int(e[i] - s[i]) // 2, 1)
    return b - at


def guard_lift(peak: int, W: int, b: int = B, over: bool = True) -> int:
    """The lift of a store that gets protected: a multiple of the group size W = stripe * group, the only lifts under which the twin's
    guard is the ordinary guard shifted by whole groups.  The largest one below b when the store's ``peak`` bytes then still pass b
    (and ``over`` asks for it), else the first one from b on (which may be b itself)."""
    below = (b - 1) // W * W
    return below if over and below + peak > b else -(-b // W) * W


def same_guard(plain, twin, lift: int, stripe: int, group: int, equal=np.array_equal):
    """None when the twin's guard (P or Q; numpy arrays, or device tensors with ``equal=torch.equal``) is the plain one moved up by
    lift / W groups over zero groups, else a reason.  The twin's last group may end with its store."""
    W = stripe * group
    assert lift % W == 0, "the guard of a twin is a shift only for a lift of whole groups"
    at = lift // W * stripe
    n = min(len(plain), len(twin) - at)
    if n < len(plain) - stripe or len(twin) > at + len(plain):
        return ("size", len(twin), at + len(plain))
    if bool(twin[:at].any()):
        return ("a group below the lift is not zero",)
    if not equal(twin[at:at + n], plain[:n]) or bool(plain[n:].any()):
        return ("guard bytes differ",)
    return None
