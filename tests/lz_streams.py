"""LZ4-block and LZF streams built from sequence lists: the decoders' inputs that no encoder here produces.

Pure Python: no GPU, no ctypes.  ``lz4_block`` / ``lzf_stream`` serialise a list of sequences and compute the plaintext
themselves, so for a valid built stream the expected bytes do not depend on any decoder.  ``case_set`` is the fixed-seed
mix the decoder differential (test_gpu_decoders.py) feeds to every door and test_lz_streams.py pins on the CPU:

  valid families    what LZ4 1.8.2 / liblzf never emit but the formats allow (every length-field boundary, every small offset,
                    matches that reach byte 0 or end at / near the block's last byte, streams longer than their block)
  malformed edits   one named edit of a valid stream each (a built one, or an encoder's output the caller passes in)

A family member that cannot exist at a block size (a 524-byte literal run in a 70-byte block, offset 65535 in any block of
at most 65536 bytes: a match needs 4 more) is left out; every family keeps members at every size the tests use.

LZ4 sequences:  (literals: bytes, offset: int, match_len: int >= 4), the last one (literals, None, None).
LZF operations: ("L", bytes of 1..32) and ("M", offset 1..8192, length 3..264).
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

LZ4_FAMILIES = ("lit_len", "match_len", "offset", "offset_is_op", "match_to_end", "match_in_last5", "match_in_last12",
                "tail_sweep", "all_literal", "encoded")
LZF_FAMILIES = ("lit_run", "match_len", "offset", "offset_is_op", "ends_with_match", "match_near_end", "expand_runs32",
                "expand_runs1", "encoded")
COMMON_EDITS = ("flip1", "rand3", "trunc", "junk", "offset_op_plus_1", "match_overruns_output_by_1", "literals_overrun_input_by_1",
                "literals_overrun_output_by_1")
LZ4_EDITS = COMMON_EDITS + ("offset_0", "ff_chain_literals", "ff_chain_match", "no_last_sequence")
LZF_EDITS = COMMON_EDITS + ("len7_last_byte", "len7_second_to_last_byte")


@dataclass(frozen=True)
class Case:
    codec: str            # "lz4" | "lzf"
    stream: bytes
    family: str           # the valid family the stream is, or was derived from
    edit: str | None      # None: a valid stream
    plain: bytes | None   # the builder's own plaintext (valid built streams only)


# ---- serialisers ------------------------------------------------------------------------------------------------------------
def _copy(plain: bytearray, off: int, n: int) -> bool:
    """plain += the format's overlapping copy of n bytes from `off` back; False when the offset is outside the output."""
    if off < 1 or off > len(plain):
        return False
    start = len(plain) - off
    if off >= n:
        plain += plain[start:start + n]
    else:
        period = bytes(plain[start:])
        plain += (period * (n // off + 1))[:n]
    return True


def _lz4_ext(n: int) -> bytes:
    """The bytes after a nibble of 15 for a field holding n >= 15."""
    n -= 15
    return b"\xff" * (n // 255) + bytes([n % 255])


def lz4_block(seqs):
    """(stream, plaintext) of an LZ4 block; plaintext is None when a match points outside the output."""
    s, plain, ok = bytearray(), bytearray(), True
    for lit, off, ml in seqs:
        s.append(min(len(lit), 15) << 4 | (0 if off is None else min(ml - 4, 15)))
        if len(lit) >= 15:
            s += _lz4_ext(len(lit))
        s += lit
        plain += lit
        if off is None:
            continue
        s += bytes([off & 0xFF, off >> 8])
        if ml - 4 >= 15:
            s += _lz4_ext(ml - 4)
        ok = ok and _copy(plain, off, ml)
    return bytes(s), bytes(plain) if ok else None


def lzf_stream(ops):
    """(stream, plaintext) of an LZF stream; plaintext is None when a match points outside the output."""
    s, plain, ok = bytearray(), bytearray(), True
    for op in ops:
        if op[0] == "L":
            assert 1 <= len(op[1]) <= 32
            s.append(len(op[1]) - 1)
            s += op[1]
            plain += op[1]
        else:
            _, off, n = op
            assert 1 <= off <= 8192 and 3 <= n <= 264
            o, l2 = off - 1, n - 2
            s += bytes([l2 << 5 | o >> 8, o & 0xFF]) if l2 < 7 else bytes([7 << 5 | o >> 8, l2 - 7, o & 0xFF])
            ok = ok and _copy(plain, off, n)
    return bytes(s), bytes(plain) if ok else None


# ---- parsers of VALID streams (to find the fields an edit changes in an encoder's output) ---------------------------------------
def lz4_parse(s: bytes):
    seqs, ip = [], 0
    while True:
        tok = s[ip]; ip += 1
        lit = tok >> 4
        if lit == 15:
            while True:
                c = s[ip]; ip += 1; lit += c
                if c != 255:
                    break
        literals = s[ip:ip + lit]; ip += lit
        if ip == len(s):
            seqs.append((literals, None, None))
            return seqs
        off = s[ip] | s[ip + 1] << 8; ip += 2
        ml = tok & 15
        if ml == 15:
            while True:
                c = s[ip]; ip += 1; ml += c
                if c != 255:
                    break
        seqs.append((literals, off, ml + 4))


def lzf_parse(s: bytes):
    ops, ip = [], 0
    while ip < len(s):
        c = s[ip]; ip += 1
        if c < 32:
            ops.append(("L", s[ip:ip + c + 1])); ip += c + 1
        else:
            n = c >> 5
            if n == 7:
                n += s[ip]; ip += 1
            ops.append(("M", ((c & 31) << 8 | s[ip]) + 1, n + 2)); ip += 1
    return ops


# ---- random valid filler in front of the sequences under test -------------------------------------------------------------------
def _lz4_filler(total: int, rng, big: bool):
    """Random sequences that yield exactly `total` bytes and end with a match (total == 0 or >= 5)."""
    assert total == 0 or total >= 5
    seqs, op, left = [], 0, total
    while left > 0:
        if left > 700 if big else left > 80:
            lit = int(rng.integers(0 if op else 1, 21))
            ml = int(rng.integers(4, 600)) if big and rng.random() < 0.3 else int(rng.integers(4, 40))
        else:
            lit, ml = left - 4, 4
        off = int(rng.integers(1, op + lit + 1))
        if rng.random() < 0.3:
            off = min(off, int(rng.integers(1, 20)))
        seqs.append((rng.bytes(lit), off, ml))
        op += lit + ml
        left -= lit + ml
    return seqs


def _lzf_filler(total: int, rng, big: bool):
    ops, op, left = [], 0, total
    while left > 0:
        if left > 300 and op and rng.random() < 0.6:
            n = int(rng.integers(3, 265)) if big or rng.random() < 0.1 else int(rng.integers(3, 40))
            off = int(rng.integers(1, min(op, 8192) + 1))
            if rng.random() < 0.3:
                off = min(off, int(rng.integers(1, 20)))
            ops.append(("M", off, n))
        else:
            n = min(left, int(rng.integers(1, 33 if rng.random() < 0.2 else 9)))
            ops.append(("L", rng.bytes(n)))
        op += n
        left -= n
    return ops


def lz4_compose(bs: int, items, tail: int, rng):
    """Filler, then items [(literal count, offset or "op", match length)], then a last sequence of `tail` literals: exactly bs
    bytes of plaintext.  None when the items do not fit the block."""
    fill = bs - sum(l + m for l, _, m in items) - tail
    if fill < 0 or 0 < fill < 5:
        return None
    seqs = _lz4_filler(fill, rng, bs > 8192)
    op = fill
    for l, off, m in items:
        op += l
        off = op if off == "op" else off
        if not 1 <= off <= op:
            return None
        seqs.append((rng.bytes(l), off, m))
        op += m
    return seqs + [(rng.bytes(tail), None, None)]


def lzf_compose(bs: int, ops_tail, rng):
    """Filler, then ops_tail (offsets may be "op"): exactly bs bytes of plaintext.  None when they do not fit."""
    fill = bs - sum(len(o[1]) if o[0] == "L" else o[2] for o in ops_tail)
    if fill < 0:
        return None
    ops, op = _lzf_filler(fill, rng, bs > 8192), fill
    for o in ops_tail:
        if o[0] == "M":
            off = op if o[1] == "op" else o[1]
            if not 1 <= off <= min(op, 8192):
                return None
            o = ("M", off, o[2])
            op += o[2]
        else:
            op += len(o[1])
        ops.append(o)
    return ops


def lzf_runs(plain: bytes, run: int):
    """plain as literal runs of `run` bytes: bs + ceil(bs / run) bytes of stream, 2 * bs for run == 1."""
    return [("L", plain[i:i + run]) for i in range(0, len(plain), run)]


def lzf_of_length(bs: int, length: int, rng):
    """A valid all-literal LZF stream of exactly `length` bytes for a bs-byte block: x 1-byte runs, then 32-byte runs.
    Possible for bs + ceil(bs / 32) <= length <= 2 * bs."""
    plain = rng.bytes(bs)
    for x in range(bs + 1):
        if 2 * x + (bs - x) + (bs - x + 31) // 32 == length:
            return lzf_runs(plain[:x], 1) + lzf_runs(plain[x:], 32)
    return None


# ---- the valid families -----------------------------------------------------------------------------------------------------------
def _thin(seq, keep: float, rng):
    seq = list(seq)
    return seq if keep >= 1 else [x for x in seq if rng.random() < keep]


def lz4_valid(bs: int, rng, keep: float = 1.0):
    """[(family, sequences)] of valid LZ4 blocks of bs bytes."""
    out = []

    def add(family, seqs):
        if seqs is not None:
            out.append((family, seqs))

    for L in list(range(17)) + [269, 270, 271, 524, 525]:         # the literal-length field: nibble, 1, 2 and 3 extension bytes
        add("lit_len", lz4_compose(bs, [(L, int(rng.integers(1, 6)), 4)], 3, rng))
    for M in list(range(4, 21)) + [273, 274, 528, 529]:            # the match-length field, overlapping and not
        add("match_len", lz4_compose(bs, [(2, int(rng.integers(1, 9)), M)], 5, rng))
        add("match_len", lz4_compose(bs, [(9, int(rng.integers(40, 60)), M)], 0, rng))
    for O in list(range(1, 71)) + [255, 256, 4095, 4096, 65535]:   # (65535 fits no block of <= 65536 bytes; kept for larger ones)
        add("offset", lz4_compose(bs, [(3, O, 6), (1, O, 21)], 2, rng))
    add("offset", [(rng.bytes(bs - 4), bs - 4, 4), (b"", None, None)])  # the largest offset a block allows, and it reaches byte 0
    for l, m, t in ((1, 4, 0), (5, 18, 7), (14, 30, 1)):
        add("offset_is_op", lz4_compose(bs, [(l, "op", m)], t, rng))
    add("offset_is_op", [(rng.bytes(7), 7, bs - 7), (b"", None, None)])
    if bs >= 64:  # at the block's start, the rest behind it
        add("offset_is_op", [(rng.bytes(9), 9, 17)] + _lz4_filler(bs - 26 - 6, rng, bs > 8192) + [(rng.bytes(6), None, None)])
    # tail sweep: the last match sequence has 0..15 literals, the literal-only last sequence 0..20 bytes
    for ml_lit in range(16):
        for last in _thin(range(21), keep, rng):
            family = "match_to_end" if last == 0 else "match_in_last5" if last < 5 else "match_in_last12" if last < 12 else "tail_sweep"
            add(family, lz4_compose(bs, [(ml_lit, int(rng.integers(1, 17)), int(rng.integers(4, 13)))], last, rng))
    add("all_literal", [(rng.bytes(bs), None, None)])
    return out


def lzf_valid(bs: int, rng, keep: float = 1.0):
    """[(family, operations)] of valid LZF streams of bs bytes."""
    out = []

    def add(family, ops):
        if ops is not None:
            out.append((family, ops))

    for R in range(1, 33):
        add("lit_run", lzf_compose(bs, [("L", rng.bytes(R)), ("M", int(rng.integers(1, 6)), 5), ("L", rng.bytes(2))], rng))
    for n in list(range(3, 11)) + [263, 264]:                      # 2-byte and 3-byte forms, the longest match
        add("match_len", lzf_compose(bs, [("M", int(rng.integers(1, 9)), n), ("L", rng.bytes(3))], rng))
        add("match_len", lzf_compose(bs, [("L", rng.bytes(4)), ("M", int(rng.integers(40, 60)), n)], rng))
    for O in list(range(1, 71)) + [255, 256, 257, 8191, 8192]:
        add("offset", lzf_compose(bs, [("M", O, 7), ("L", rng.bytes(1)), ("M", O, 23), ("L", rng.bytes(2))], rng))
    for pre, n in ((1, 3), (6, 19), (31, 264)):
        add("offset_is_op", lzf_compose(bs, [("L", rng.bytes(pre)), ("M", "op", n), ("L", rng.bytes(1))], rng))
    if bs >= 64:  # at the stream's start (the only place for it in a block of more than 8192 bytes), the rest behind it
        add("offset_is_op", [("L", rng.bytes(11)), ("M", 11, 30)] + _lzf_filler(bs - 41, rng, bs > 8192))
    # matches of 3..40 bytes at offsets 1..40 that end at bs, bs - 1 .. bs - 17
    for end in range(18):
        for n in _thin(range(3 + end % 2, 41, 2), keep, rng):
            off = 1 + (n * 7 + end * 3) % 40
            add("ends_with_match" if end == 0 else "match_near_end",
                lzf_compose(bs, [("M", off, n)] + ([("L", rng.bytes(end))] if end else []), rng))
    plain = rng.bytes(bs)
    add("expand_runs32", lzf_runs(plain, 32))
    add("expand_runs1", lzf_runs(plain, 1))
    return out


# ---- the malformed edits ------------------------------------------------------------------------------------------------------------
def _random_edits(stream: bytes, rng):
    n = len(stream)
    a = bytearray(stream)
    a[int(rng.integers(0, n))] ^= int(rng.integers(1, 256))
    yield "flip1", bytes(a)
    a = bytearray(stream)
    for p in rng.integers(0, n, 3):
        a[int(p)] = int(rng.integers(0, 256))
    yield "rand3", bytes(a)
    cut = int(rng.integers(1, 21))
    if cut < n:
        yield "trunc", stream[:-cut]
    yield "junk", stream + rng.bytes(int(rng.integers(1, 4)))


def lz4_edits(seqs, bs: int, rng):
    """(edit, stream) for each structural edit the valid block `seqs` allows."""
    matches = [i for i, s in enumerate(seqs) if s[1] is not None]
    if matches:
        k = matches[int(rng.integers(0, len(matches)))]
        op = sum(len(l) + m for l, _, m in seqs[:k]) + len(seqs[k][0])   # bytes of output when the match starts
        lit, _, ml = seqs[k]
        if op + 1 <= 0xFFFF:
            yield "offset_op_plus_1", lz4_block(seqs[:k] + [(lit, op + 1, ml)] + seqs[k + 1:])[0]
        yield "offset_0", lz4_block(seqs[:k] + [(lit, 0, ml)] + seqs[k + 1:])[0]
        # 0xFF length chains that run to the end of the input: the literal field of sequence k, the match field of sequence k
        stream, _ = lz4_block(seqs)
        at = len(lz4_block(seqs[:k])[0])
        yield "ff_chain_literals", stream[:at] + bytes([0xF0 | stream[at] & 15]) + b"\xff" * (len(stream) - at - 1)
        head = lz4_block(seqs[:k] + [(lit, seqs[k][1], 19)])[0][:-1]      # ... token with match nibble 15, literals, offset
        if len(stream) > len(head):
            yield "ff_chain_match", head + b"\xff" * (len(stream) - len(head))
        last = matches[-1]
        rest = sum(len(l) + (m or 0) for l, _, m in seqs[last + 1:])
        lit, off, ml = seqs[last]
        yield "match_overruns_output_by_1", lz4_block(seqs[:last] + [(lit, off, ml + rest + 1)] + seqs[last + 1:])[0]
        if rest == 0:  # the match ends the block: without the (empty) last sequence the stream stops right after a match
            yield "no_last_sequence", lz4_block(seqs[:last + 1])[0]
    tail = seqs[-1][0]
    more = tail + rng.bytes(1)
    yield "literals_overrun_input_by_1", lz4_block(seqs[:-1] + [(more, None, None)])[0][:-1]
    yield "literals_overrun_output_by_1", lz4_block(seqs[:-1] + [(more, None, None)])[0]


def lzf_edits(ops, bs: int, rng):
    matches = [i for i, o in enumerate(ops) if o[0] == "M"]
    runs = [i for i, o in enumerate(ops) if o[0] == "L"]
    size = lambda o: len(o[1]) if o[0] == "L" else o[2]

    def raw(op):  # an operation whose fields the serialiser would refuse
        _, off, n = op
        o, l2 = off - 1, n - 2
        return bytes([l2 << 5 | o >> 8, o & 0xFF]) if l2 < 7 else bytes([7 << 5 | o >> 8, l2 - 7, o & 0xFF])

    if matches:
        k = matches[int(rng.integers(0, len(matches)))]
        op = sum(size(o) for o in ops[:k])
        if op + 1 <= 8192:
            yield "offset_op_plus_1", lzf_stream(ops[:k])[0] + raw(("M", op + 1, ops[k][2])) + lzf_stream(ops[k + 1:])[0]
        last = matches[-1]
        rest = sum(size(o) for o in ops[last + 1:])
        if ops[last][2] + rest + 1 <= 264:
            yield "match_overruns_output_by_1", (lzf_stream(ops[:last])[0] + raw(("M", ops[last][1], ops[last][2] + rest + 1)) +
                                                 lzf_stream(ops[last + 1:])[0])
    if runs:
        last = runs[-1]
        body = ops[last][1]
        if len(body) < 32:
            grown = lzf_stream(ops[:last] + [("L", body + rng.bytes(1))])[0]
            after = lzf_stream(ops[last + 1:])[0]
            if not after:  # the run ends the stream: its count says one byte more than the input holds
                yield "literals_overrun_input_by_1", grown[:-1]
            rest = sum(size(o) for o in ops[last + 1:])
            if rest == 0:
                yield "literals_overrun_output_by_1", grown
        elif last == len(ops) - 1:
            yield "literals_overrun_input_by_1", lzf_stream(ops)[0][:-1]
            yield "literals_overrun_output_by_1", lzf_stream(ops + [("L", rng.bytes(1))])[0]
    # a control byte of a long match (len field 7) with nothing, or only its length byte, behind it
    head = lzf_stream(ops[:-1])[0]
    if head:
        yield "len7_last_byte", head + bytes([0xE0 | int(rng.integers(0, 32))])
        yield "len7_second_to_last_byte", head + bytes([0xE0 | int(rng.integers(0, 32)), int(rng.integers(0, 256))])


# ---- the case set ---------------------------------------------------------------------------------------------------------------
def case_set(codec: str, bs: int, encoded, seed: int = 2024):
    """The decoder differential's cases for one codec and block size, in a fixed order.  `encoded` is a list of valid streams of
    bs-byte blocks from an encoder (the caller's: this module has none); they are cases themselves and bases of edits."""
    rng = np.random.default_rng([seed, bs, 0 if codec == "lz4" else 1])
    keep = 1.0 if bs <= 8192 else 0.5 if bs < 65536 else 0.25
    build, parse, valid, edits = ((lz4_block, lz4_parse, lz4_valid, lz4_edits) if codec == "lz4" else
                                  (lzf_stream, lzf_parse, lzf_valid, lzf_edits))
    cases, bases = [], []
    members = valid(bs, rng, keep)
    if keep < 1:  # thin the per-value families too, but keep every family and both expanding streams
        seen, thinned = set(), []
        for fam, seqs in members:
            if fam not in seen or fam.startswith("expand") or rng.random() < keep:
                thinned.append((fam, seqs))
            seen.add(fam)
        members = thinned
    for fam, seqs in members:
        stream, plain = build(seqs)
        assert plain is not None and len(plain) == bs, (fam, len(plain or b""))
        cases.append(Case(codec, stream, fam, None, plain))
        bases.append((fam, seqs, stream))
    for stream in encoded:
        cases.append(Case(codec, stream, "encoded", None, None))
    enc_bases = [("encoded", parse(s), s) for s in encoded]
    # structural edits: of every encoded stream, and of every few built ones (each family at least once)
    seen = set()
    for i, (fam, seqs, stream) in enumerate(enc_bases + bases):
        if fam == "encoded" or fam not in seen or i % max(1, int(6 / keep)) == 0:
            seen.add(fam)
            for edit, bad in edits(seqs, bs, rng):
                cases.append(Case(codec, bad, fam, edit, None))
    # random edits: mostly of encoded streams (long literal runs: a changed byte is often still a valid stream)
    rounds = max(3, int(round(4 * keep)))
    for fam, _, stream in enc_bases * rounds + bases[::max(1, int(8 / keep))]:
        for edit, bad in _random_edits(stream, rng):
            cases.append(Case(codec, bad, fam, edit, None))
    return cases


def encoded_bases(encode, bs: int, corpus: bytes):
    """Valid streams of an encoder for bs-byte blocks: corpus blocks, a zero block, a period-3 block (b"" = did not fit: left out)."""
    blocks = [corpus[o:o + bs] for o in range(0, min(len(corpus) - bs + 1, 12 * bs), bs)]
    blocks += [bytes(bs), (b"abc" * (bs // 3 + 1))[:bs]]
    return [s for s in (encode(b) for b in blocks) if s]


def verdicts(decode, cases, bs: int):
    """[(status, bytes or None)]: status 0 iff `decode(stream, bs)` (the oracle's decoder) returns exactly bs bytes."""
    out = []
    for c in cases:
        got = decode(c.stream, bs) if c.stream else None
        ok = got is not None and len(got) == bs
        out.append((0, got) if ok else (1, None))
    return out


# ---- what the two test modules share ------------------------------------------------------------------------------------------------
def stages_slot(codec: str, bs: int) -> bool:
    """cw_dev_decompress's rule for the wavefront decoder (decompress_launch): the compressed slot is copied to LDS when the
    decoded block (rounded up to 16) plus a staging buffer of the codec's usual bound (LZ4: bs + bs / 255 + 16, LZF: bs; rounded up
    to 16) fit 40 KiB."""
    up16 = lambda x: (x + 15) & ~15
    return up16(bs) + up16(bs + bs // 255 + 16 if codec == "lz4" else bs) <= 40 * 1024


def staging_pair(codec: str):
    """(the largest block size whose slot is staged, the smallest whose slot is not): 20432 / 20433 for LZ4 (40960 against 40992
    bytes of LDS), 20480 / 20481 for LZF (40960 against 40992)."""
    last = max(bs for bs in range(16384, 24576) if stages_slot(codec, bs))
    assert not stages_slot(codec, last + 1)
    return last, last + 1


def block_sizes(codec: str):
    return [70, 4093, 4096, *staging_pair(codec), 65536]


_SETS = {}


def oracle_set(oracle, codec: str, bs: int, corpus: bytes):
    """(cases, verdicts) of one codec and block size with `oracle` (the CPU oracle package) as encoder of the base streams and as
    judge; built once per process."""
    if (codec, bs) not in _SETS:
        enc, dec = (oracle.lz4_compress, oracle.lz4_decompress) if codec == "lz4" else (oracle.lzf_compress, oracle.lzf_decompress)
        cases = case_set(codec, bs, encoded_bases(enc, bs, corpus))
        _SETS[codec, bs] = (cases, verdicts(dec, cases, bs))
    return _SETS[codec, bs]
