"""Encoder inputs built for an edge: plaintext blocks that take the serial LZ4 / LZF parsers to the rules a parallel restatement
gets wrong (the encoders' counterpart of lz_streams.py, which builds the decoders' inputs).

Pure Python plus numpy, fixed seeds: no GPU, no ctypes.  A block is a list of operations realised as plaintext -- fresh noise
for literals, copies from a chosen distance for matches (lz_streams._copy), the byte behind a copy changed where it would extend
it and the byte in front of it where it would let it start earlier, compressible filler in front of the part under test so that
LZ4's search step is 1 where it matters and an LZF block still fits n - 1 bytes.  Whether a block reaches its edge is not taken
on trust: test_lz_inputs.py confirms every family from the oracle's own parsed output (lz_streams.lz4_parse / lzf_parse), and the
few constructions that depend on the hash table's state (a distance of 8192 bytes, the probe schedule) are drawn again with the
next seed until the oracle -- the `oracle` argument of case_set -- takes them as intended.

A family member that cannot exist at a block size is left out, as in lz_streams.py: distance 8192 in a 70-byte block, a step of 2
in a block the search leaves after 58 probes, LZ4 offsets 65534 / 65535 in any block of at most 65536 bytes (a match starts at
n - 12 at the latest; the largest offset a block allows, n - 12, takes their place).

lzf_model(block, cap) is a second implementation of liblzf's compressor as SURVEY.md 8(a) row A6 specifies it, written from that
row alone; it also says which of the three "did not fit" checks gave up.
"""
from __future__ import annotations

import importlib.util
import os
from dataclasses import dataclass

import numpy as np

import lz_streams as Z

SIZES = (70, 1000, 4093, 4096, 5001, 16384, 16385, 65533, 65536)
LZF_FAMILIES = ("fit_margin", "tail_match", "match_len", "distance", "ref_is_0", "lit_run", "reinsert", "straddle")
LZ4_FAMILIES = ("end_rules", "len_fields", "distance", "pos0", "catch_up", "retest", "skip", "straddle")
FIT_CONSTRUCTIONS = ("text_noise", "noise_text", "noise_text_repeat", "filler_noise")
FIT_WINDOW = 48
LZ4_LENGTHS = (14, 15, 16, 269, 270, 271, 524, 525, 526)


def _load_walk():
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "lz_probe_count.py")
    spec = importlib.util.spec_from_file_location("lz_probe_count", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.lz4_walk


lz4_walk = _load_walk()


@dataclass(frozen=True)
class Case:
    codec: str
    family: str
    kind: str            # the member: what the block was built to reach
    plain: bytes
    at: int | None       # where the operation under test starts
    arg: int | None      # its parameter (a length, a distance, k of n - k, ...)


# ---- spans of a parsed stream: (kind "L" | "M", start in the plaintext, length, distance or None) ---------------------------
def lzf_spans(ops):
    out, pos = [], 0
    for op in ops:
        if op[0] == "L":
            out.append(("L", pos, len(op[1]), None)); pos += len(op[1])
        else:
            out.append(("M", pos, op[2], op[1])); pos += op[2]
    return out


def lz4_spans(seqs):
    out, pos = [], 0
    for lit, off, ml in seqs:
        out.append(("L", pos, len(lit), None)); pos += len(lit)
        if off is not None:
            out.append(("M", pos, ml, off)); pos += ml
    return out


def match_at(spans, pos):
    return next((s for s in spans if s[0] == "M" and s[1] == pos), None)


def matches_within(spans, a, b):
    return [s for s in spans if s[0] == "M" and s[1] < b and s[1] + s[2] > a]


# ---- the block builder --------------------------------------------------------------------------------------------------------
class DoesNotFit(Exception):
    pass


def _pool(codec: str, variant: int, total: int = 65536 + 64):
    """Compressible filler that refers only to itself: literal runs of 1..4 bytes between copies of up to 40 bytes from at most
    48 bytes back.  Blocks take disjoint slices of it, so no slice repeats another inside one block."""
    key = (codec, variant)
    if key not in _POOLS:
        rng = np.random.default_rng([77, variant, 0 if codec == "lz4" else 1])
        mm = 4 if codec == "lz4" else 3
        p = bytearray(rng.bytes(6))
        while len(p) < total:
            dist = int(rng.integers(1, min(len(p), 48) + 1))
            if len(p) > dist and p[-1] == p[-1 - dist]:
                p[-1] = (p[-1] + 1) & 255
            Z._copy(p, dist, int(rng.integers(mm, 12 if rng.random() < 0.5 else 40)))
            cont = p[len(p) - dist]
            lit = bytearray(rng.bytes(int(rng.integers(1, 5))))
            if lit[0] == cont:
                lit[0] = (lit[0] + 1) & 255
            p += lit
        _POOLS[key] = bytes(p[:total])
    return _POOLS[key]


_POOLS = {}


class Block:
    """Operations (see build()) appended to a plaintext; marks remember where named operations start."""

    def __init__(self, codec, n, rng, variant):
        self.codec, self.n, self.rng = codec, n, rng
        self.p = bytearray()
        self.cont = None      # the byte that would lengthen the copy just made
        self.literal = False  # the last byte is a literal of this builder's (it may be changed)
        self.pool, self.cur = _pool(codec, variant), 0
        self.marks = {}

    def _join(self, data: bytearray):
        if data and self.cont is not None and data[0] == self.cont:
            data[0] = (data[0] + 1) & 255
        self.cont = None
        self.p += data

    def lit(self, k):
        if k > 0:
            self._join(bytearray(self.rng.bytes(k)))
            self.literal = True

    def fill(self, k):
        if k < 0 or self.cur + k > len(self.pool):
            raise DoesNotFit
        if 0 < k < 12:
            return self.lit(k)
        if k:
            self._join(bytearray(self.pool[self.cur:self.cur + k]))
            self.cur += k
            self.literal = True   # (the end of a slice may be the end of a filler copy: changing it only shortens that copy)

    def fill_to(self, pos):
        self.fill(pos - len(self.p))

    def copy(self, src, length):
        dist = len(self.p) - src
        if src < 0 or dist < 1 or length < 1:
            raise DoesNotFit
        if self.literal and src > 0:
            avoid = {self.p[src - 1]}
            while self.p[-1] in avoid:   # the byte in front must not let the match start earlier
                self.p[-1] = (self.p[-1] + 1) & 255
        Z._copy(self.p, dist, length)
        self.cont = self.p[len(self.p) - dist]
        self.literal = False


def build(codec, n, seed, ops, variant=0):
    """ops: ("L", k) noise | ("F", k) filler | ("F@", pos) filler up to pos | ("F*",) filler up to what the rest needs |
    ("S", name, k) noise that a later copy reads | ("@", name) a mark | ("C", name, offset, length) a copy from mark + offset.
    Returns (plaintext of exactly n bytes, marks) or None when the operations do not fit n bytes."""
    size = lambda o: o[1] if o[0] in ("L", "F") else o[2] if o[0] == "S" else o[3] if o[0] == "C" else 0
    rng = np.random.default_rng(list(seed))
    b = Block(codec, n, rng, variant)
    try:
        for i, o in enumerate(ops):
            if o[0] == "L":
                b.lit(o[1])
            elif o[0] == "F":
                b.fill(o[1])
            elif o[0] == "F@":
                b.fill_to(o[1])
            elif o[0] == "F*":
                b.fill_to(n - sum(size(x) for x in ops[i + 1:]))
            elif o[0] == "S":
                b.marks[o[1]] = len(b.p)
                b.lit(o[2])
            elif o[0] == "@":
                b.marks[o[1]] = len(b.p)
            else:
                b.copy(b.marks[o[1]] + o[2], o[3])
    except DoesNotFit:
        return None
    if len(b.p) != n:
        return None
    return bytes(b.p), b.marks


# ---- the plain-Python LZF model ----------------------------------------------------------------------
def lzf_model(block: bytes, cap: int):
    """(stream, refused_by): lzf_compress(block, len(block), out, cap) restated from the survey's row, not from the oracle's C.
    refused_by is None and stream the output when it fits; else stream is b"" and refused_by says which check gave up:
    "match" (no room for the longest match form in front of a match), "literal" (no room for one more literal byte) or "tail"
    (no room for the at most three bytes still missing at the end)."""
    n = len(block)
    if n == 0 or cap <= 0:
        return b"", "tail"
    a = np.frombuffer(block, np.uint8).astype(np.uint32)
    slots = []
    if n >= 3:
        h = (a[:-2] << 16) | (a[1:-1] << 8) | a[2:]
        slots = ((((h >> 8) - h * 5) & 0xFFFF).astype(np.int64)).tolist()
    tab = [0] * 65536
    out = bytearray(1)          # the control byte of the literal run that is open
    lit = 0
    ip, end = 0, n
    while ip < end - 2:
        s = slots[ip]
        ref = tab[s]
        tab[s] = ip
        if 0 < ref < ip and ip - ref - 1 < 8192 and block[ref:ref + 3] == block[ip:ip + 3]:
            if len(out) - (lit == 0) + 4 >= cap:
                return b"", "match"
            if lit:
                out[-lit - 1] = lit - 1
            else:
                out.pop()
            off = ip - ref - 1
            maxlen = min(end - ip - 2, 264)
            length = 2
            if maxlen > 16:     # sixteen compares without a bound, then the bounded loop
                stopped = False
                for _ in range(16):
                    length += 1
                    if block[ref + length] != block[ip + length]:
                        stopped = True
                        break
                if not stopped:
                    length += 1
                    while length < maxlen and block[ref + length] == block[ip + length]:
                        length += 1
            else:
                length += 1
                while length < maxlen and block[ref + length] == block[ip + length]:
                    length += 1
            length -= 2
            if length < 7:
                out.append((off >> 8) + (length << 5))
            else:
                out.append((off >> 8) + (7 << 5))
                out.append(length - 7)
            out.append(off & 0xFF)
            out.append(0)
            lit = 0
            ip += length + 2
            if ip >= end - 2:
                break
            tab[slots[ip - 2]] = ip - 2     # VERY_FAST: only the match's last two positions enter the table
            tab[slots[ip - 1]] = ip - 1
        else:
            if len(out) >= cap:
                return b"", "literal"
            out.append(block[ip])
            ip += 1
            lit += 1
            if lit == 32:
                out[-33] = 31
                out.append(0)
                lit = 0
    if len(out) + 3 > cap:
        return b"", "tail"
    while ip < end:
        out.append(block[ip])
        ip += 1
        lit += 1
        if lit == 32:
            out[-33] = 31
            out.append(0)
            lit = 0
    if lit:
        out[-lit - 1] = lit - 1
    else:
        out.pop()
    return bytes(out), None


# ---- LZF families -------------------------------------------------------------------------------------------------------------
def _text(k, rng):
    words = [bytes(rng.integers(97, 123, int(rng.integers(2, 10)), dtype=np.uint8)) for _ in range(96)]
    out = bytearray()
    while len(out) < k:
        out += words[int(rng.integers(0, len(words)))] + b" "
    return bytes(out[:k])


def fit_block(construction, n, t, seed=0):
    """The block of one fit_margin construction with t bytes of noise: the boundary between its two parts slides, the bytes of
    either part stay where they are counted from (text from its start, noise from its start)."""
    key = (construction, n, seed)
    if key not in _FIT_PARTS:
        rng = np.random.default_rng([11, FIT_CONSTRUCTIONS.index(construction), n, seed])
        _FIT_PARTS[key] = (_text(n, rng), rng.bytes(n), _pool("lzf", 3)[:n])
    text, noise, filler = _FIT_PARTS[key]
    if construction == "text_noise":
        return text[:n - t] + noise[:t]
    if construction == "filler_noise":
        return filler[:n - t] + noise[:t]
    if construction == "noise_text":
        return noise[:t] + text[:n - t]
    body = bytearray(noise[:t] + text[:n - t])
    r = min(19, (n - t) // 3)
    if r >= 3:                                   # the text's end repeats what lies 2 r bytes in front of it
        body[n - r:] = body[n - 3 * r:n - 2 * r]
    return bytes(body)


_FIT_PARTS = {}


def fit_crossing(construction, n, oracle, seed=0):
    """The smallest number of noise bytes (found by bisection; the size grows with it but for the parser's local choices) at
    which the stream at cap 2 n is longer than n - 1 bytes."""
    size = lambda t: len(oracle.lzf_compress(fit_block(construction, n, t, seed), cap=2 * n))
    lo, hi = 0, n - 1
    if size(lo) > n - 1:
        return 0
    if size(hi) <= n - 1:
        return hi
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if size(mid) > n - 1:
            hi = mid
        else:
            lo = mid
    return hi


def fit_class(block, oracle):
    """("accepted", margin n - 1 - size) or ("refused", how many bytes the complete stream is longer than n - 1; <= 0: it would
    have fitted)."""
    n = len(block)
    got = oracle.lzf_compress(block)
    if got:
        return "accepted", n - 1 - len(got)
    return "refused", len(oracle.lzf_compress(block, cap=2 * n)) - (n - 1)


def _lzf_fit_margin(n, oracle):
    out = []
    for c in FIT_CONSTRUCTIONS:
        for seed in range(2):
            t0 = fit_crossing(c, n, oracle, seed)
            window = FIT_WINDOW if seed == 0 else FIT_WINDOW // 4
            for t in range(max(0, t0 - window), min(n - 1, t0 + window) + 1):
                out.append(Case("lzf", "fit_margin", c, fit_block(c, n, t, seed), n - t if c.endswith("noise") else t, t))
    return out


def _lzf_specs(n, v):
    S = {f: [] for f in LZF_FAMILIES if f != "fit_margin"}
    for k in range(3, 31):
        S["tail_match"].append(("k", k, [("L", 2), ("F*",), ("S", "a", k), ("F", 5), ("@", "x"), ("C", "a", 0, k)], "x"))
    for L in list(range(3, 22)) + list(range(262, 268)):
        S["match_len"].append(("len", L, [("L", 2), ("F*",), ("S", "a", L), ("F", 5), ("@", "x"), ("C", "a", 0, L), ("F", 24)], "x"))
    for d in (1, 2, 3, 255, 256, 257, 8191, 8192, 8193):
        if d < 8:
            ops = [("L", 2), ("F*",), ("S", "a", d), ("@", "x"), ("C", "a", 0, 10), ("F", 24)]
        else:
            ops = [("L", 2), ("F*",), ("S", "a", 8), ("F", d - 8), ("@", "x"), ("C", "a", 0, 8), ("F", 24)]
        S["distance"].append(("dist", d, ops, "x"))
    for gap in (11, 40):
        S["ref_is_0"].append(("first20", gap, [("S", "a", 20), ("F", gap), ("@", "x"), ("C", "a", 0, 20), ("F*",)], "x"))
    for R in (31, 32, 33, 63, 64, 65):
        S["lit_run"].append(("between", R, [("L", 2), ("F*",), ("S", "r", 6), ("S", "a", 6), ("F", 5), ("C", "r", 0, 5), ("@", "x"),
                                            ("L", R), ("C", "a", 0, 6), ("F", 4)], "x"))
    S["lit_run"].append(("before_end", 32, [("L", 2), ("F*",), ("S", "r", 6), ("F", 5), ("C", "r", 0, 6), ("@", "x"), ("L", 32)], "x"))
    for j in (1, 2, 3, 4):    # the second repeat starts j bytes in front of the first match's end
        S["reinsert"].append(("last", j, [("L", 2), ("F*",), ("S", "a", 12), ("F", 6), ("@", "m"), ("C", "a", 0, 12), ("L", 8), ("F", 6),
                                          ("@", "x"), ("C", "m", 12 - j, 7), ("F", 6)], "x"))
    step = 16384 if n > 16384 else 4096
    for m in range(step, n, step):
        for s in (1, 2, 3):
            for e in (1, 2, 3):
                if s + e >= 3:
                    S["straddle"].append(("match", m, [("L", 2), ("F@", m - s - 6 - (s + e)), ("S", "a", s + e), ("F", 6), ("@", "x"),
                                                       ("C", "a", 0, s + e), ("F*",)], "x"))
        for start in [m - s for s in (1, 2, 3)] + [m + e - 32 for e in (1, 2, 3)]:
            S["straddle"].append(("run32", m, [("L", 2), ("F@", start - 23), ("S", "r", 6), ("S", "a", 6), ("F", 5), ("C", "r", 0, 6), ("@", "x"),
                                               ("L", 32), ("C", "a", 0, 6), ("F*",)], "x"))
    return S


# ---- LZ4 families -------------------------------------------------------------------------------------------------------------
def lz4_schedule(count):
    """The positions the search probes from the block's start while nothing matches: 64 at step 1, 64 at step 2, ..."""
    out, fwd, step, nb = [], 1, 1, 64
    for _ in range(count):
        out.append(fwd)
        fwd += step
        step = nb >> 6
        nb += 1
    return out


def _lz4_specs(n, v):
    S = {f: [] for f in LZ4_FAMILIES}
    for k in range(4, 25):
        S["end_rules"].append(("k", k, [("F*",), ("S", "a", k), ("F", 7), ("@", "x"), ("C", "a", 0, k)], "x"))
    for period in (1, 7, 30):
        S["end_rules"].append(("through_end", period, [("F*",), ("S", "a", period), ("@", "x"), ("C", "a", 0, 60)], "x"))
    for L in LZ4_LENGTHS:
        S["len_fields"].append(("literals", L, [("F*",), ("S", "r", 6), ("S", "a", 10), ("F", 6), ("C", "r", 0, 5), ("@", "x"), ("L", L),
                                                ("C", "a", 0, 10), ("F", 24)], "x"))
    for M in LZ4_LENGTHS:
        for M in (M, M + 4):
            S["len_fields"].append(("match", M, [("F*",), ("S", "a", M), ("F", 6), ("@", "x"), ("C", "a", 0, M), ("F", 24)], "x"))
    for d in (1, 2, 3, 4, 255, 256, 257):
        if d < 8:
            ops = [("F*",), ("S", "a", d), ("@", "x"), ("C", "a", 0, 12), ("F", 24)]
        else:
            ops = [("F*",), ("S", "a", 8), ("F", d - 8), ("@", "x"), ("C", "a", 0, 8), ("F", 24)]
        S["distance"].append(("dist", d, ops, "x"))
    for lead in (0, 1):   # the largest offsets a block allows: a match at n - 12 that reaches position 0 / 1
        S["distance"].append(("dist", n - 12 - lead, [("L", lead), ("S", "a", 8), ("F@", n - 12), ("@", "x"), ("C", "a", 0, 7), ("L", 5)], "x"))
    for gap in (20, 492):
        S["pos0"].append(("first8", gap, [("S", "a", 8), ("F", gap), ("@", "x"), ("C", "a", 0, 6), ("F*",)], "x"))
    S["pos0"].append(("noise", None, [("L", n)], None))
    # catch-up: behind a match whose last bytes the table does not hold (one byte back, to the anchor) ...
    for j in (1, 3):
        S["catch_up"].append(("anchor", j, [("F*",), ("S", "u", 8), ("F", 6), ("S", "v", 6), ("F", 6), ("@", "s"), ("C", "u", 0, 8), ("L", 8), ("F", 8),
                                            ("C", "v", 0, 6), ("@", "x"), ("C", "s", 8 - j, j + 8), ("F", 24)], "x"))
    # ... and where the search steps over the repeat's first bytes: b bytes back, stopped by a mismatch (the source at 2) or by
    # position 0 (the source at 0)
    probes = lz4_schedule(64 * 9 + 8)
    for b in range(1, 9):
        zone = [p for i, p in enumerate(probes) if i >= 64 * b + 2 and i < 64 * (b + 1)]
        for P in zone[v % 8::24]:
            S["catch_up"].append(("back", b, [("L", 2), ("S", "a", 20), ("L", P - b - 22), ("@", "x"), ("C", "a", 0, 16), ("F*",)], "x"))
            if b <= 2:
                S["catch_up"].append(("to_0", b, [("S", "a", 20), ("L", P - b - 20), ("@", "x"), ("C", "a", 0, 12), ("F*",)], "x"))
    for c in range(2, 7):
        ops = [("F*",)] + [o for i in range(c) for o in (("S", f"a{i}", 6), ("L", 1))] + [("F", 6), ("@", "x")]
        ops += [("C", f"a{i}", 0, 6) for i in reversed(range(c))] + [("F", 24)]   # (sources in order would be one long match)
        S["retest"].append(("chain", c, ops, "x"))
    for s in list(range(60, 72)) + list(range(186, 200)):     # a 4-byte repeat: found only where the search probes
        S["skip"].append(("start", s, [("S", "a", 12), ("L", s - 12), ("@", "x"), ("C", "a", 4, 4), ("L", 9), ("F*",)], "x"))
    for m in range(4096, n, 4096):
        for s in (1, 2, 3):
            for e in (1, 2, 3):
                if s + e >= 4:
                    S["straddle"].append(("match", m, [("F@", m - s - 6 - (s + e)), ("S", "a", s + e), ("F", 6), ("@", "x"),
                                                       ("C", "a", 0, s + e), ("F*",)], "x"))
        for start in [m - s for s in (1, 2, 3)] + [m + e - 20 for e in (1, 2, 3)]:
            S["straddle"].append(("run20", m, [("F@", start - 23), ("S", "r", 6), ("S", "a", 6), ("F", 5), ("C", "r", 0, 6), ("@", "x"),
                                               ("L", 20), ("C", "a", 0, 6), ("F*",)], "x"))
    return S


# ---- did the oracle take the block as intended? ----------------------------------------------------------------------------------
def spans_of(case, oracle):
    if case.codec == "lz4":
        return lz4_spans(Z.lz4_parse(oracle.lz4_compress(case.plain)))
    return lzf_spans(Z.lzf_parse(oracle.lzf_compress(case.plain, cap=2 * len(case.plain))))


def reached(case, spans):
    """True when the oracle's parse shows the member's edge (for members that must NOT be found: that it was not)."""
    n, at, arg, kind, fam = len(case.plain), case.at, case.arg, case.kind, case.family
    m = match_at(spans, at) if at is not None else None
    if case.codec == "lzf":
        if fam == "fit_margin":
            return True
        if fam == "tail_match":       # the last match begins at n - k and what is left behind it is 0, 1 or 2 literals
            last = [s for s in spans if s[0] == "M"][-1:]
            return bool(last) and last[0][1] == at and n - (last[0][1] + last[0][2]) <= 2
        if fam == "match_len":
            return m is not None and m[2] == min(arg, 264)
        if fam == "distance":
            if arg == 8193:
                return not matches_within(spans, at, at + 8)
            return m is not None and m[3] == arg
        if fam == "ref_is_0":         # found one byte late: position 1 is the first a reference may name
            m = match_at(spans, at + 1)
            return m is not None and m[3] == at and m[2] == 19 and match_at(spans, at) is None
        if fam in ("lit_run", "straddle") and kind != "match":
            runs = [s for s in spans if s[0] == "L" and at <= s[1] < at + arg] if fam == "lit_run" else \
                [s for s in spans if s[0] == "L" and at <= s[1] < at + 32]
            want = arg if fam == "lit_run" else 32
            lens = [s[2] for s in runs]
            ok = runs and runs[0][1] == at and sum(lens) == want and all(x == 32 for x in lens[:-1])
            if kind == "before_end":
                ok = ok and at + 32 == n
            return bool(ok)
        if fam == "straddle":
            return m is not None and at < arg < at + m[2]
        if fam == "reinsert":         # found inside the previous match for its last two positions only
            inside = m is not None and m[3] == 6 + 8 + arg
            return inside if arg <= 2 else not inside
    else:
        if fam == "end_rules":
            if kind == "k":           # taken from k = 12 on, and then 5 literals are left
                return (m is not None and m[1] + m[2] == n - 5) if arg >= 12 else not matches_within(spans, at, n)
            return m is not None and m[1] + m[2] == n - 5
        if fam == "len_fields":
            if kind == "literals":
                return any(s[0] == "L" and s[1] == at and s[2] == arg for s in spans) and match_at(spans, at + arg) is not None
            return m is not None and m[2] == arg
        if fam == "distance":
            return m is not None and m[3] == arg
        if fam == "pos0":
            return kind == "noise" and len(spans) == 1 or m is not None and m[3] == at
        if fam == "retest":           # arg matches in a row, arg - 1 of them with no literal in front
            chain = [match_at(spans, at + 6 * i) for i in range(arg)]
            return all(c is not None and c[2] == 6 for c in chain)
        if fam == "straddle":
            if kind == "match":
                return m is not None and at < arg < at + m[2]
            return any(s[0] == "L" and s[1] == at and s[2] == 20 for s in spans)
        if fam in ("catch_up", "skip"):
            probes, seqs = lz4_walk(case.plain)
            if fam == "skip":         # found exactly when the search probes its first byte
                return (m is not None) == (at in probes) and (m is not None or not matches_within(spans, at, at + 4))
            seq = next((q for q in seqs if q[2] == at), None)
            if seq is None or seq[1] < 1:
                return False
            if kind == "anchor":
                return seq[3] == 0
            if kind == "to_0":
                return seq[1] == arg and seq[4] == at
            return seq[1] == arg
    return False


# ---- the case sets --------------------------------------------------------------------------------------------------------------
_SETS = {}


def cases(codec: str, n: int, oracle):
    """The cases of one codec and block size in a fixed order.  A member is built with seeds 0, 1, ... until the oracle reaches
    its edge (at most 6; a member that never does stays out), then the whole list again with further seeds while the set has
    fewer than 150 blocks."""
    if (codec, n) in _SETS:
        return _SETS[codec, n]
    out = _lzf_fit_margin(n, oracle) if codec == "lzf" else []
    specs, families = (_lzf_specs, LZF_FAMILIES) if codec == "lzf" else (_lz4_specs, LZ4_FAMILIES)
    v0 = 0
    while v0 == 0 or (len(out) < 150 and v0 < 48):
        for fam, members in specs(n, v0).items():
            for i, (kind, arg, ops, mark) in enumerate(members):
                for v in range(v0, v0 + 6):
                    built = build(codec, n, (5, n, families.index(fam), i, v), ops, variant=(i + v) % 3)
                    if built is None:      # does not fit n bytes: with no seed
                        break
                    c = Case(codec, fam, kind, built[0], built[1].get(mark), arg)
                    if reached(c, spans_of(c, oracle)):
                        out.append(c)
                        break
        v0 += 6
    if len(out) > 800:
        raise AssertionError((codec, n, len(out)))
    _SETS[codec, n] = out
    return out


def case_set(codec: str, n: int, oracle):
    """[(family, plaintext of exactly n bytes)]"""
    return [(c.family, c.plain) for c in cases(codec, n, oracle)]


def small_sizes(codec: str):
    """[(n, plaintext)] for n = 1..40: the sizes at which the parsers leave before their loops start (LZ4 below 13 bytes, LZF
    below 3) or right after; noise, one byte repeated, a period of 3 and a second half that repeats the first."""
    rng = np.random.default_rng([9, 0 if codec == "lz4" else 1])
    out = []
    for n in range(1, 41):
        half = rng.bytes((n + 1) // 2)
        out += [(n, rng.bytes(n)), (n, bytes([int(rng.integers(0, 256))]) * n), (n, (rng.bytes(3) * 14)[:n]), (n, (half + half)[:n])]
    return out


def census(oracle, sizes=SIZES):
    """{codec: {size: {family: count}}} plus the fit_margin classes per size: what tests/golden/lz_inputs_census.json pins."""
    out = {"cases": {}, "fit_margin": {}}
    for codec in ("lz4", "lzf"):
        out["cases"][codec] = {}
        for n in sizes:
            count = {}
            for c in cases(codec, n, oracle):
                count[c.family] = count.get(c.family, 0) + 1
            out["cases"][codec][str(n)] = count
    for n in sizes:
        cls = {}
        for c in cases("lzf", n, oracle):
            if c.family == "fit_margin":
                verdict, by = fit_class(c.plain, oracle)
                key = f"accepted_margin_{by}" if verdict == "accepted" and by <= 4 else "accepted_margin_5_or_more" if verdict == "accepted" else \
                    "refused_fits" if by <= 0 else f"refused_long_{by}" if by <= 4 else "refused_long_5_or_more"
                cls[key] = cls.get(key, 0) + 1
        out["fit_margin"][str(n)] = dict(sorted(cls.items()))
    return out
