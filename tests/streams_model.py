"""Reference model of content-defined chunking over many streams in one buffer (cw_dev_cdc_streams).

``chunk_streams`` is the definition: every stream chunked alone by cdc_model.chunk, the cuts shifted by the stream's start.
``chunk_chain`` is what the device does: ONE chain over the concatenation, with H running over the whole buffer, in which a
step from a cut sees as n the smallest stream end above the cut.  The two must agree (tests/test_cdc_streams_abi.py); that they
do is the independence argument of the design: a test at x >= c + m, m >= 64, reads only bytes at or behind c.

The case table of tests/test_gpu_cdc_streams.py is built here, so that the CPU suite can establish from the model that each
case reaches its edge."""
from __future__ import annotations

import functools

import numpy as np

import cdc_model as CM
from conftest import corpus_file

P1K = CM.default_params(1024)                                   # chunks of 256 .. 8192 bytes
MIN, AVG, MAX = P1K["min"], P1K["avg"], P1K["max"]
P_ALL = dict(P1K, gear=np.zeros(256, np.uint64))                # H = 0: every position is a candidate, every chunk is min_size
P_NONE = dict(P1K, gear=np.full(256, 1 << 63, np.uint64))       # H = 2^63: no position is one, every chunk is max_size
SEGMENTS = {"one_max": 8192, "default": 256 << 10}              # CW_CDC_SEGMENT = 8192, and the default for max_size 8192


def chunk_streams(streams, p: dict):
    """(offsets[0..K], first[0..nstreams]): the per-stream definition."""
    offsets, first, start = [0], [], 0
    for s in streams:
        first.append(len(offsets) - 1)
        if len(s):
            offsets += [start + c for c in CM.chunk(s, p)[1:]]
            start += len(s)
    first.append(len(offsets) - 1)
    return offsets, first


def ends_of(streams) -> list[int]:
    return [int(v) for v in np.cumsum([len(s) for s in streams], dtype=np.uint64)]


def chunk_chain(streams, p: dict):
    """One chain over the concatenation; each step sees the end of the stream it stands in (an upper bound in the ends, which
    skips repeated ends).  first[f] = the lower bound of stream f's start in the cuts."""
    data = b"".join(bytes(s) for s in streams)
    ends = np.array(ends_of(streams), dtype=np.int64)
    total = len(data)
    a = np.frombuffer(data, dtype=np.uint8)
    H = CM.window_hash(a, CM._gear(p))
    cs = np.flatnonzero((H & np.uint64(p["mask_s"])) == 0) + 1
    cl = np.flatnonzero((H & np.uint64(p["mask_l"])) == 0) + 1
    m, A, M = p["min"], p["avg"], p["max"]
    cuts, c = [0], 0
    while c != total:
        n = int(ends[np.searchsorted(ends, c, side="right")])
        r = n - c
        if r <= m:
            c = n
        else:
            e, z = c + min(M, r), c + min(A, r)
            i = np.searchsorted(cs, c + m)
            if i < len(cs) and cs[i] < z:
                c = int(cs[i])
            else:
                j = np.searchsorted(cl, z)
                c = int(cl[j]) if j < len(cl) and cl[j] < e else e
        cuts.append(c)
    starts = [0] + [int(e) for e in ends[:-1]] if len(streams) else []
    first = [int(np.searchsorted(cuts, s, side="left")) for s in starts] + [len(cuts) - 1]
    return cuts, first


def per_stream_cuts(offsets, first):
    """The recipe cuts of every stream, rebased to 0 ([0] for an empty stream)."""
    return [[c - offsets[a] for c in offsets[a:b + 1]] if b > a else [0] for a, b in zip(first[:-1], first[1:])]


def max_cuts_in_a_segment(offsets, seg: int) -> int:
    return int(np.bincount(np.asarray(offsets[:-1], dtype=np.int64) // seg).max()) if len(offsets) > 1 else 0


# ---- the cases -------------------------------------------------------------------------------------------------------------
def noise(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


@functools.lru_cache(None)
def text():
    return corpus_file("lcet10.txt") + corpus_file("plrabn12.txt")


def split(data: bytes, lengths):
    out, at = [], 0
    for n in lengths:
        out.append(data[at:at + n])
        at += n
    assert at <= len(data)
    return out


LADDER = [0, MIN, 0, 0, MIN + 1, 0, MAX, 0, MAX + 1, 0, 63, 0, 64, 0, 65, 0, 0]   # empty streams first, last, doubled and between
ZERO_RUNS = [5 * MAX + 77, 3, 2 * MAX, 7 * MAX + 1]
ALL_LENGTHS = [10 * MIN + 3, MIN, 2 * MIN + 255, 1, 40 * MIN + 100]
NONE_LENGTHS = [3 * MAX + 5, MAX, 2 * MAX - 1, 9 * MAX + 100]
BLOCK = 40000


def edge_lengths(S):
    return [S - 1, 1, S, S + 1, S - 1, 2 * S]


def dup_streams():
    block = text()[300000:300000 + BLOCK]
    return [noise(7001, 21), block, noise(12345, 22), noise(333, 23), block, noise(5000, 24)]


# name -> (S -> the streams, the chunking parameters); S = the resolve's segment in bytes
CASES = {
    "one_byte_x3000": (lambda S: split(noise(3000, 1), [1] * 3000), P1K),
    "ladder": (lambda S: split(text()[1000:], LADDER), P1K),
    "segment_edges": (lambda S: split(text()[:6 * S + 1] if 6 * S + 1 <= len(text()) else noise(6 * S + 1, 2), edge_lengths(S)), P1K),
    "zero_runs": (lambda S: [noise(12345, 3) + bytes(ZERO_RUNS[0])] + [bytes(n) for n in ZERO_RUNS[1:]], P1K),
    "all_candidates": (lambda S: split(noise(sum(ALL_LENGTHS), 4), ALL_LENGTHS), P_ALL),
    "no_candidates": (lambda S: split(noise(sum(NONE_LENGTHS), 5), NONE_LENGTHS), P_NONE),
    "one_text_300k": (lambda S: [text()[:300000]], P1K),
    "no_streams": (lambda S: [], P1K),
    "one_empty": (lambda S: [b""], P1K),
    "dup_block": (lambda S: dup_streams(), P1K),
}


@functools.lru_cache(None)
def case(name: str, S: int):
    """(streams, params, offsets, first) of a case at segment size S, computed once."""
    build, p = CASES[name]
    streams = build(S)
    offsets, first = chunk_streams(streams, p)
    return streams, p, offsets, first
