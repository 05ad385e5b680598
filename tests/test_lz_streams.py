"""The stream builder of the decoder differential (lz_streams.py) and its case mix, on the CPU: what the builder says a valid
stream decodes to is what the oracle's decoders give, and every set the GPU tests use holds enough accepted and enough rejected
streams, every valid family and every named edit."""
import collections

import pytest

import lz_streams as Z
from conftest import corpus_file

SETS = [(codec, bs) for codec in ("lz4", "lzf") for bs in Z.block_sizes(codec)]


@pytest.fixture(scope="module")
def corpus():
    return corpus_file("alice29.txt")


def test_serialisers_on_hand_written_streams():
    # LZ4: 3 literals, match of 6 at offset 2 (overlapping), last sequence of 5 literals
    s, p = Z.lz4_block([(b"abc", 2, 6), (b"vwxyz", None, None)])
    assert s == bytes([0x32]) + b"abc" + bytes([2, 0, 0x50]) + b"vwxyz" and p == b"abcbcbcbcvwxyz"
    # length fields of 15 + 255 + 0 (literals) and 4 + 15 + 3 (match)
    s, p = Z.lz4_block([(bytes(270), 1, 22), (b"", None, None)])
    assert s == bytes([0xFF, 255, 0]) + bytes(270) + bytes([1, 0, 3, 0x00]) and p == bytes(292)
    assert Z.lz4_parse(s) == [(bytes(270), 1, 22), (b"", None, None)]
    assert Z.lz4_block([(b"ab", 3, 4), (b"", None, None)])[1] is None  # offset before the block
    # LZF: run of 2, match of 8 at offset 2 (2-byte form), match of 9 at offset 257 is 3 bytes: 0xE1 (len field 7, offset high 1), 0, 0
    s, p = Z.lzf_stream([("L", b"ab"), ("M", 2, 8)])
    assert s == bytes([1]) + b"ab" + bytes([6 << 5, 1]) and p == b"ab" * 5
    ops = [("L", bytes(range(32)))] * 9 + [("M", 257, 9)]
    s, p = Z.lzf_stream(ops)
    assert s[-3:] == bytes([0xE1, 0, 0]) and len(p) == 297 and p[-9:] == p[31:40] and Z.lzf_parse(s) == ops


def test_staging_pair_straddles_the_lds_rule():
    assert Z.staging_pair("lz4") == (20432, 20433) and Z.staging_pair("lzf") == (20480, 20481)


def test_expanding_lzf_streams_are_longer_than_their_block(oracle, corpus):
    """32-byte and 1-byte literal runs over a 4096-byte block: 4224 and 8192 bytes of stream, valid for the oracle's decoder."""
    blk = corpus[:4096]
    for run, want in ((32, 4224), (1, 8192)):
        s, p = Z.lzf_stream(Z.lzf_runs(blk, run))
        assert len(s) == want and p == blk and oracle.lzf_decompress(s, 4096) == blk


def test_lzf_stream_of_any_length(oracle):
    import numpy as np
    rng = np.random.default_rng(3)
    for length in (4093 + 128, 4093 + 129, 6001, 2 * 4093 - 1, 2 * 4093):
        s, p = Z.lzf_stream(Z.lzf_of_length(4093, length, rng))
        assert len(s) == length and oracle.lzf_decompress(s, 4093) == p


@pytest.mark.parametrize("codec,bs", SETS)
def test_case_set(oracle, corpus, codec, bs):
    cases, verdict = Z.oracle_set(oracle, codec, bs, corpus)
    assert 150 <= len(cases) <= 2000
    # valid built streams: the oracle's decode is the builder's plaintext
    for c, (st, got) in zip(cases, verdict):
        if c.edit is None:
            assert st == 0, c.family
            if c.plain is not None:
                assert got == c.plain, c.family
    # the mix: both verdicts well represented, every family accepted, every edit rejected at least once
    accepted = sum(1 for st, _ in verdict if st == 0)
    assert 0.15 * len(cases) <= accepted <= 0.85 * len(cases)
    fam = collections.Counter(c.family for c, (st, _) in zip(cases, verdict) if c.edit is None and st == 0)
    rej = collections.Counter(c.edit for c, (st, _) in zip(cases, verdict) if c.edit is not None and st == 1)
    assert [f for f in (Z.LZ4_FAMILIES if codec == "lz4" else Z.LZF_FAMILIES) if not fam[f]] == []
    assert [e for e in (Z.LZ4_EDITS if codec == "lz4" else Z.LZF_EDITS) if not rej[e]] == []
    if codec == "lzf":  # longer than the block, and than the wavefront decoder's staging buffer
        assert sum(1 for c in cases if c.edit is None and len(c.stream) > ((bs + 15) & ~15)) >= 2


@pytest.mark.parametrize("bs", [4093, 4096])
def test_lz4_tail_sweep_puts_a_token_at_each_of_the_last_18_bytes(bs):
    """lane_decode reads a sequence through a 16-byte window while 16 bytes are left: a token starts at every n - 18 .. n - 1."""
    import numpy as np
    rng = np.random.default_rng(5)
    seen = set()
    for family, seqs in Z.lz4_valid(bs, rng):
        if family in ("match_to_end", "match_in_last5", "match_in_last12", "tail_sweep"):
            n = len(Z.lz4_block(seqs)[0])
            seen |= {n - len(Z.lz4_block(seqs[:k])[0]) for k in (len(seqs) - 2, len(seqs) - 1)}
    assert set(range(1, 19)) <= seen
