"""Pin the Skein oracle to the reference's own vectors:
NIST KAT files of reference_code/skein/KAT_MCT and oracle/_ref (reference C compiled in place)."""
import pytest

from conftest import anchor_input, load_golden, seeded_block


@pytest.mark.parametrize("bits", [512, 256])
def test_short_and_long_kat(oracle, bits):
    g = load_golden(f"skein_kat_{bits}.json")
    fn = oracle.skein512 if bits == 512 else oracle.skein256
    n = 0
    for rec in g["short"] + g["long"]:
        msg = bytes.fromhex(rec["msg"])
        assert fn(msg, bits, msg_bits=rec["len"]).hex() == rec["md"], f"Len={rec['len']}"
        n += 1
    assert n > 300


@pytest.mark.parametrize("bits", [512, 256])
def test_montecarlo_kat(oracle, bits):
    """genKAT.c genMonteCarlo: Msg(128 B) <- MD || Msg[:128-len(MD)], 1000 times per checkpoint."""
    g = load_golden(f"skein_kat_{bits}.json")["montecarlo"]
    fn = oracle.skein512 if bits == 512 else oracle.skein256
    msg = bytes.fromhex(g["seed"])
    nb = bits // 8
    for want in g["md"][:3]:
        for _ in range(1000):
            md = fn(msg, bits)
            msg = md + msg[:128 - nb]
        assert md.hex() == want


def test_block_digests_vs_reference_build(oracle):
    """4096/65536-byte blocks and Skein-256-128: sizes/variants no KAT reaches; expected values come
    from oracle/_ref (the reference's Optimized_64bit C) via tools/make_golden.py."""
    g = load_golden("skein_ref_blocks.json")
    for rec in g["blocks"]:
        d = seeded_block(rec["seed"], rec["n"], rec["kind"])
        assert oracle.skein512(d, 512).hex() == rec["skein512_512"]
        assert oracle.skein256(d, 128).hex() == rec["skein256_128"]
        assert oracle.skein256(d, 256).hex() == rec["skein256_256"]


def test_survey_anchors(oracle):
    for a in load_golden("survey_anchors.json")["anchors"]:
        d = anchor_input(a["input"], a["n"])
        assert oracle.skein512(d, 512).hex().startswith(a["skein512_prefix"])
        assert oracle.skein256(d, 128).hex() == a["skein256_128"]


def test_live_reference_build_when_present(oracle):
    """Fresh inputs against oracle/_ref's digests of them: stored in skein_ref_live.json (tools/make_golden.py --live), and
    also computed live where oracle/_ref was built (this container, or shipped prebuilt)."""
    g = load_golden("skein_ref_live.json")["blocks"]
    assert [rec["n"] for rec in g] == [0, 1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 4096, 65536, 70001]
    live = oracle.ref_available()
    for rec in g:
        d = seeded_block(rec["seed"], rec["n"], rec["kind"])
        assert oracle.skein512(d, 512).hex() == rec["skein512_512"]
        assert oracle.skein256(d, 128).hex() == rec["skein256_128"]
        assert oracle.skein512(d, 256).hex() == rec["skein512_256"]   # config-block IV path
        assert oracle.skein512(d, 160).hex() == rec["skein512_160"]
        if live:
            assert oracle.skein512(d, 512) == oracle.ref_skein512(d, 512)
            assert oracle.skein256(d, 128) == oracle.ref_skein256(d, 128)
            assert oracle.skein512(d, 256) == oracle.ref_skein512(d, 256)
            assert oracle.skein512(d, 160) == oracle.ref_skein512(d, 160)


def test_iv_512_is_config_block_ubi(oracle):
    # first word of SKEIN_512_IV_512 as vendored (skein_iv.h:124-134), value is data not code
    iv = oracle.skein_iv(8, 512)
    z = oracle.skein512(b"", 512)
    assert len(z) == 64 and iv.shape == (8,)
    # the ShortMsgKAT Len=0 digest exercises exactly IV -> final(empty) -> output
    g = load_golden("skein_kat_512.json")
    assert z.hex() == g["short"][0]["md"]


def test_tree_mode_matches_reference_golden_kat(oracle):
    """Skein tree hashing against every Skein-256 / Skein-512 tree vector of the reference's
    KAT_MCT/skein_golden_kat.txt (leaf/node/maxLevel 2/2/2, 1/2/3 and 2/1/255)."""
    vecs = load_golden("skein_kat_tree.json")["vectors"]
    assert len(vecs) == 23
    for v in vecs:
        got = oracle.skein_tree(v["state_bits"], bytes.fromhex(v["msg"]), v["hash_bits"], v["leaf"], v["node"], v["max_level"])
        assert got.hex() == v["digest"], v


def test_tree_mode_degenerate_cases(oracle):
    # a message that fits one leaf is still not the sequential hash (tree fields change the configuration block)
    msg = bytes(range(64))
    assert oracle.skein_tree(512, msg, 512, 1, 1, 2) != oracle.skein512(msg, 512)
    assert len(oracle.skein_tree(256, b"", 128, 1, 1, 255)) == 16
    with pytest.raises(ValueError):
        oracle.skein_tree(512, msg, 512, 0, 1, 2)


def test_threefish_round_by_round_against_reference_internals(oracle):
    """the reference ships a round-by-round dump of its SKEIN_DEBUG build
    (KAT_MCT/skein_golden_kat_short_internals.txt, callouts skein.h:246-254); the oracle's Threefish reproduces every state of
    the file's Threefish-256 and -512 call records (tests/golden/skein_internals.json, extracted by tools/make_golden.py
    --internals): after the initial key injection, after each of the 72 rounds, after each of the 18 key injections.
    The oracle is written in the textbook form (MIX, then move the words); the reference's code renames operands instead and
    dumps the words where it holds them, which inside a group of four rounds lags the textbook order by the remaining word
    permutations -- the only mapping applied here."""
    import numpy as np
    perm = {4: [0, 3, 2, 1], 8: [2, 1, 4, 7, 6, 5, 0, 3]}
    calls = load_golden("skein_internals.json")["calls"]
    assert {c["state_words"] for c in calls} == {4, 8} and len(calls) >= 4
    for c in calls:
        nw = c["state_words"]
        block = np.array(c["block_words"], dtype="<u8").tobytes()
        trace, chain = oracle.threefish_trace(nw, c["key"], c["tweak"], block)
        exp = np.array(c["states"], dtype=np.uint64)
        row = 0
        for rec in range(91):
            # record 0: initial injection; then groups of (4 rounds, 1 injection)
            j = 0 if rec == 0 else (rec - 1) % 5 + 1          # 1..4 = round within its group, 5 = the injection behind it
            k = (4 - j) % 4 if j in (1, 2, 3) else 0           # word permutations the reference's operand order is behind by
            idx = list(range(nw))
            for _ in range(k):
                idx = [idx[p] for p in perm[nw]]
            assert np.array_equal(exp[rec], trace[rec][idx]), (nw, rec)
            row += 1
        assert np.array_equal(chain, trace[90] ^ np.array(c["block_words"], dtype=np.uint64))   # feed-forward
