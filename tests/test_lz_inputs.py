"""The encoder inputs of lz_inputs.py pinned on the CPU: every block is what the oracle's stream decodes to, every family reaches
its edge in the oracle's own parsed output (a family without a confirmed member at a size fails), the fit_margin family holds
the accepted and refused cases within four bytes of n - 1, the plain-Python LZF model equals the oracle and names the check that
refused, the LZ4 walk of tools/lz_probe_count.py equals the oracle's sequences, and the census of the sets is the committed one."""
import json
import os

import numpy as np
import pytest

import lz_inputs as I
import lz_streams as Z
from conftest import GOLDEN

SETS = [(codec, n) for codec in ("lz4", "lzf") for n in I.SIZES]
MODEL_SIZES = [n for n in I.SIZES if n <= 5001] + [65536]


def _by_family(cases):
    out = {}
    for c in cases:
        out.setdefault(c.family, []).append(c)
    return out


def _expected_families(codec, n):
    """Which families can exist at n (module docstring of lz_inputs.py)."""
    if codec == "lzf":
        return [f for f in I.LZF_FAMILIES if f != "straddle" or n > 4096]
    return [f for f in I.LZ4_FAMILIES if (f not in ("catch_up", "skip") or n >= 1000) and (f != "straddle" or n > 4096 + 48)]


@pytest.mark.parametrize("codec,n", SETS)
def test_the_oracles_stream_decodes_to_the_block(oracle, codec, n):
    cases = I.cases(codec, n, oracle)
    assert 150 <= len(cases) <= 800
    assert I.case_set(codec, n, oracle) == [(c.family, c.plain) for c in cases]
    for c in cases:
        assert len(c.plain) == n
        if codec == "lz4":
            assert oracle.lz4_decompress(oracle.lz4_compress(c.plain), n) == c.plain
        else:
            full = oracle.lzf_compress(c.plain, cap=2 * n)
            assert oracle.lzf_decompress(full, n) == c.plain
            got = oracle.lzf_compress(c.plain)
            assert got in (b"", full) and (got or len(full) + 4 >= n - 1), (c.family, c.kind, c.arg)   # gives up only near the cap


@pytest.mark.parametrize("codec,n", SETS)
def test_every_family_reaches_its_edge_in_the_oracles_output(oracle, codec, n):
    cases = I.cases(codec, n, oracle)
    fam = _by_family(cases)
    assert list(fam) == _expected_families(codec, n)
    spans = {id(c): I.spans_of(c, oracle) for c in cases}
    for c in cases:
        assert I.reached(c, spans[id(c)]), (c.family, c.kind, c.arg)
    args = lambda f, kind=None: {c.arg for c in fam.get(f, []) if kind is None or c.kind == kind}
    accepted = lambda f: [c for c in fam[f] if oracle.lzf_compress(c.plain)]
    if codec == "lzf":
        for f in fam:      # the edge is in a stream the encoder really returns, not only in the one at cap 2 n
            assert accepted(f), f
        left = {n - (s[-1][1] + s[-1][2]) if s[-1][0] == "M" else s[-1][2] for s in (spans[id(c)] for c in fam["tail_match"])}
        assert left == {0, 1, 2}                          # the last operation is a match, or 1 or 2 literals follow it
        assert args("tail_match") == set(range(3, 31)) if n > 70 else args("tail_match") >= set(range(3, 30))
        k19 = next(c for c in fam["tail_match"] if c.arg == 19)
        assert spans[id(k19)][-1] == ("M", n - 19, 19, 24)   # 16 compares without a bound, one more before the bound is read
        assert args("match_len") >= set(range(3, 20)) and (n < 1000 or args("match_len") >= {17, 18, 19, 262, 263, 264, 265, 266, 267})
        assert args("distance") >= {1, 2, 3} and (n < 1000 or args("distance") >= {255, 256, 257})
        if n >= 16384:
            assert args("distance") >= {8191, 8192, 8193}
            for c in fam["distance"]:
                found = I.match_at(spans[id(c)], c.at)
                assert (found is None) == (c.arg == 8193) and (found is None or found[3] == c.arg)
        for c in fam["ref_is_0"]:
            m = I.match_at(spans[id(c)], c.at + 1)
            assert m[3] == m[1] - 1 and m[2] == 19        # offset = position - 1: position 0 is never a reference
        assert args("lit_run", "between") >= {31, 32, 33} and (n < 1000 or args("lit_run", "between") == {31, 32, 33, 63, 64, 65})
        assert n < 1000 or args("lit_run", "before_end") == {32}
        assert args("reinsert") == {1, 2, 3, 4}
        if "straddle" in fam:
            step = 16384 if n > 16384 else 4096
            inner = set(range(step, n - 48, step))
            assert args("straddle", "match") >= inner and args("straddle", "run32") >= inner
    else:
        for c in cases:    # no match starts behind n - 12, and at least 5 literals end the block
            s = spans[id(c)]
            assert all(x[1] <= n - 12 for x in s if x[0] == "M") and s[-1][0] == "L" and s[-1][2] >= 5
        assert args("end_rules", "k") == set(range(4, 25)) and args("end_rules", "through_end") >= {1, 7}
        taken = {c.arg for c in fam["end_rules"] if c.kind == "k" and I.match_at(spans[id(c)], c.at)}
        assert taken == set(range(12, 25))
        fit = [L for L in I.LZ4_LENGTHS if L + 60 < n]
        assert args("len_fields", "literals") >= set(fit) and args("len_fields", "match") >= {L + d for L in fit if 2 * L + 40 < n for d in (0, 4)}
        assert args("distance") >= {1, 2, 3, 4, n - 12, n - 13} and (n < 1000 or args("distance") >= {255, 256, 257})
        assert {c.kind for c in fam["pos0"]} == {"first8", "noise"}
        for c in fam["pos0"]:
            assert c.kind == "noise" or I.match_at(spans[id(c)], c.at)[3] == c.at     # the match is position 0
        assert args("retest") == ({2, 3, 4, 5, 6} if n >= 1000 else {2, 3})    # (a chain of 4 and its sources need 82 bytes)
        for c in fam["retest"]:
            s = spans[id(c)]
            i = s.index(I.match_at(s, c.at))
            assert [x[0] for x in s[i:i + 2 * c.arg - 1]] == ["M", "L"] * (c.arg - 1) + ["M"]
            assert all(x[2] == 0 for x in s[i + 1:i + 2 * c.arg - 1:2])                 # literal counts of 0
        if "skip" in fam:
            found = {I.match_at(spans[id(c)], c.at) is not None for c in fam["skip"] if c.arg >= 186}
            assert found == {True, False}
            assert all(I.match_at(spans[id(c)], c.at) for c in fam["skip"] if c.arg <= 64)   # step 1: nothing is stepped over
            backs = args("catch_up", "back")
            assert backs >= ({1, 2, 3, 4} if n < 4093 else set(range(1, 9)))
            assert args("catch_up", "anchor") and args("catch_up", "to_0") >= {1, 2}
        if "straddle" in fam:
            inner = set(range(4096, n - 48, 4096))
            assert args("straddle", "match") >= inner and args("straddle", "run20") >= inner


def test_a_block_that_lost_its_edge_is_not_confirmed(oracle):
    """The confirmation looks at the edge: with the copy under test replaced by noise no member passes it (members whose edge is
    that nothing is found are left out)."""
    rng = np.random.default_rng(3)
    for codec in ("lz4", "lzf"):
        seen = set()
        for c in I.cases(codec, 16384, oracle):
            negative = (c.family, c.arg) == ("distance", 8193) or (c.family == "end_rules" and c.kind == "k" and c.arg < 12) or \
                c.family in ("fit_margin", "skip") or c.kind in ("noise", "run32", "run20", "between", "before_end", "literals")
            if negative or (c.family, c.kind) in seen:
                continue
            seen.add((c.family, c.kind))
            broken = bytearray(c.plain)
            span = I.match_at(I.spans_of(c, oracle), c.at + (c.family == "ref_is_0"))
            broken[span[1]:span[1] + span[2]] = rng.bytes(span[2])
            broken = I.Case(c.codec, c.family, c.kind, bytes(broken), c.at, c.arg)
            assert not I.reached(broken, I.spans_of(broken, oracle)), (codec, c.family, c.kind, c.arg)
        assert len(seen) >= 6, seen


@pytest.mark.parametrize("n", I.SIZES)
def test_fit_margin_holds_both_verdicts_within_four_bytes_of_the_cap(oracle, n):
    cases = [c for c in I.cases("lzf", n, oracle) if c.family == "fit_margin"]
    assert {c.kind for c in cases} == set(I.FIT_CONSTRUCTIONS)
    for kind in I.FIT_CONSTRUCTIONS:      # every tail length within 48 of the crossing
        t0 = I.fit_crossing(kind, n, oracle)
        have = {c.arg for c in cases if c.kind == kind}
        assert have >= set(range(max(0, t0 - I.FIT_WINDOW), min(n - 1, t0 + I.FIT_WINDOW) + 1))
    classes = [I.fit_class(c.plain, oracle) for c in cases]
    margins = {by for verdict, by in classes if verdict == "accepted"}
    assert margins >= {1, 2, 3, 4}
    assert sum(1 for verdict, by in classes if verdict == "refused" and 1 <= by <= 4) >= 10
    assert sum(1 for verdict, by in classes if verdict == "refused" and by <= 0) >= 2   # refused although the stream would have fitted


@pytest.mark.parametrize("n", MODEL_SIZES)
def test_the_lzf_model_equals_the_oracle_and_names_the_check_that_refused(oracle, n):
    cases = I.cases("lzf", n, oracle)
    if n > 5001:
        cases = [c for c in cases if c.family in ("fit_margin", "tail_match")]
    refused = {"match": 0, "literal": 0, "tail": 0}
    for c in cases:
        stream, why = I.lzf_model(c.plain, n - 1)
        assert stream == oracle.lzf_compress(c.plain), (c.family, c.kind, c.arg)
        assert (why is None) == bool(stream)
        if why:
            refused[why] += 1
        if n <= 5001 and c.family != "fit_margin":
            assert I.lzf_model(c.plain, 2 * n) == (oracle.lzf_compress(c.plain, cap=2 * n), None)
    assert min(refused.values()) >= 2, refused


def test_the_lz4_walk_equals_the_oracles_sequences(oracle):
    for n in (1000, 4093, 5001):
        for c in I.cases("lz4", n, oracle):
            probes, seqs = I.lz4_walk(c.plain)
            want = Z.lz4_parse(oracle.lz4_compress(c.plain))
            assert [(q[3], q[4], q[5]) for q in seqs] == [(len(lit), off, ml) for lit, off, ml in want], (c.family, c.kind, c.arg)
            assert probes == sorted(set(probes)) and all(q[0] is None or q[0] in probes for q in seqs)
    noise = np.random.default_rng(1).bytes(1000)
    probes = I.lz4_walk(noise)[0]
    assert len(probes) > 200 and probes == I.lz4_schedule(len(probes))   # nothing matches: the schedule alone


def test_small_sizes_cover_one_to_forty(oracle):
    for codec in ("lz4", "lzf"):
        blocks = I.small_sizes(codec)
        assert sorted({n for n, _ in blocks}) == list(range(1, 41)) and all(len(b) == n for n, b in blocks)


def test_the_census_is_the_committed_one(oracle):
    with open(os.path.join(GOLDEN, "lz_inputs_census.json")) as f:
        want = json.load(f)
    assert I.census(oracle) == want
