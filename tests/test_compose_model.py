"""tests/compose_model.py against ``cdc_model.chunk(B)``: the anchors / windows / rounds procedure of cw_store_compose gives exactly
the cuts of the whole composed stream and keeps exactly the positions the rule names, on seeded op lists over noise, all-zero,
periodic and mixed sources of one to three joined streams, and every named case of the table reaches the edge it is named for."""
import numpy as np
import pytest

import cdc_model as CM
import compose_model as XM

P = XM.P


def source(kind: str, n: int, rng) -> bytes:
    if kind == "zero":
        return bytes(n)
    if kind == "periodic":
        return (bytes(range(7, 7 + 37)) * (n // 37 + 1))[:n]
    if kind == "mixed":
        third = n // 3
        return rng.integers(0, 256, third, dtype=np.uint8).tobytes() + bytes(third) + (bytes(range(11, 11 + 53)) * (third // 53 + 2))[:n - 2 * third]
    return rng.integers(0, 256, n, dtype=np.uint8).tobytes()


def op_list(a: bytes, cuts, first, rng):
    """Copies that start and end on cuts, beside them and anywhere, that continue each other, overlap, move backwards and reach A's
    end; new runs of 1 .. 3000 bytes; sometimes nothing but copies or nothing but new bytes."""
    n = len(a)
    spots = sorted(set(cuts) | {cuts[f] for f in first})

    def place():
        r = int(rng.integers(0, 4))
        x = int(spots[int(rng.integers(0, len(spots)))]) if r < 2 else int(rng.integers(0, n + 1))
        return min(max(x + (int(rng.integers(-1, 2)) if r == 1 else 0), 0), n)

    parts, at = [], None
    style = int(rng.integers(0, 8))
    for _ in range(int(rng.integers(1, 9))):
        if n and (style == 0 or (style != 1 and rng.integers(0, 3) > 0)):
            lo = at if at is not None and rng.integers(0, 4) == 0 else place()
            hi = n if rng.integers(0, 5) == 0 else place()
            if hi < lo:
                lo, hi = hi, lo
            if rng.integers(0, 3) == 0:
                hi = min(hi, lo + int(rng.integers(1, 5000)))
            parts.append(("copy", lo, hi - lo))
            at = hi
        else:
            m = int(rng.integers(1, 3001)) if rng.integers(0, 4) else int(rng.integers(1, 70))
            parts.append(("new", bytes(m) if rng.integers(0, 5) == 0 else rng.integers(0, 256, m, dtype=np.uint8).tobytes()))
    return XM.tile(parts)


def check(a, cuts, first, ops, payload, lookahead=0):
    got = XM.compose(a, cuts, first, ops, payload, P, lookahead)
    want = CM.chunk(got["bytes"], P)
    assert got["cuts"] == want, (len(a), ops, lookahead)
    assert got["kept"] == XM.kept_by_rule(ops, cuts, first, want), (len(a), ops, lookahead)
    assert got["stats"]["rebuilt_chunks"] + got["stats"]["kept_positions"] == len(want) - 1
    return got


@pytest.mark.parametrize("half", [0, 1])
def test_procedure_gives_the_cuts_of_the_composed_stream_and_keeps_what_the_rule_names(half):
    rng = np.random.default_rng(2700 + half)
    seen = dict(rounds2=0, merged=0, kept=0, lists=0)
    for kind in ("noise", "zero", "periodic", "mixed"):
        for nstreams in (1, 2, 3):
            for rep in range(2):
                streams = [source(kind, int(rng.integers(1, 9000)) if rep else int(rng.integers(3000, 16000)), rng) for _ in range(nstreams)]
                a, cuts, first = XM.join(streams)
                for _ in range(50):
                    ops, payload = op_list(a, cuts, first, rng)
                    got = check(a, cuts, first, ops, payload, lookahead=int(rng.integers(0, 2)))
                    st = got["stats"]
                    seen["rounds2"] += st["rounds"] >= 2
                    seen["merged"] += st["merged_windows"] > 0
                    seen["kept"] += st["kept_positions"] > 0
                    seen["lists"] += 1
    assert seen["lists"] == 1200 and seen["rounds2"] > 20 and seen["merged"] > 20 and seen["kept"] > 300, seen


def test_anchor_rule_on_a_joined_source():
    a, cuts, first = XM.join([bytes(range(256)) * 20, bytes(range(255, -1, -1)) * 12])
    k, e = len(cuts) - 1, first[1]
    nb = len(a)
    # the whole of A: every position but the last of stream 0 is keepable, the last of stream 1 because it ends B
    assert XM.anchors([XM.copy(0, nb, 0)], cuts, first, nb) == [(0, 0, 0, e - 1), (cuts[e], 0, e, k)]
    # ... and it is not when something follows
    ops = [XM.copy(0, nb, 0), XM.new(nb, 5, 0)]
    assert XM.anchors(ops, cuts, first, nb + 5) == [(0, 0, 0, e - 1), (cuts[e], 0, e, k - 1)]
    # a copy that holds no whole chunk is no anchor; adjacent copies that continue each other are one
    assert XM.anchors([XM.copy(0, cuts[1] - 1, 0)], cuts, first, cuts[1] - 1) == []
    ops = [XM.copy(0, 100, cuts[2]), XM.copy(100, cuts[4] - cuts[2] - 100, cuts[2] + 100)]
    assert XM.anchors(ops, cuts, first, cuts[4] - cuts[2]) == [(0, cuts[2], 2, 4)]


CASES = XM.cases()


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_named_case_reaches_its_edge(case):
    if not case["ops"]:
        got = XM.compose(case["a"], case["cuts"], case["first"], [], b"", P)
        assert got["cuts"] == [0] and got["stats"]["rounds"] == 0
        return
    got = check(case["a"], case["cuts"], case["first"], case["ops"], case["payload"], case["lookahead"])
    for key, want in case["expect"].items():
        if key.startswith("min_"):
            assert got["stats"][key[4:]] >= want, (key, got["stats"])
        else:
            assert got["stats"][key] == want, (key, got["stats"])
    name, st, kept, ops = case["name"], got["stats"], got["kept"], case["ops"]
    if name == "an anchor kept from byte 0":
        assert 0 in kept and got["extents"][0][0] > 0
    if name == "a final window":
        assert got["extents"][-1][1] == len(got["bytes"]) and st["kept_positions"] > 0
    if name == "no anchor at all":
        assert got["extents"] == [(0, len(got["bytes"]), len(got["cuts"]) - 1)]
    if name == "a moved copy and a copy used twice":
        assert len(set(kept.values())) < len(kept) and st["kept_positions"] > 100
    if name == "a copy to A's end that is B's end":
        assert len(case["cuts"]) - 2 in kept.values()
    if name == "a copy to A's end that is not B's end":
        assert len(case["cuts"]) - 2 not in kept.values() and len(case["cuts"]) - 3 in kept.values()
    if name == "a copy across a stream end of a joined source":
        first = case["first"]
        held = set(kept.values())
        assert first[1] - 1 not in held and first[2] - 1 not in held and first[3] - 1 in held   # (the last one ends B as well)
        assert all(any(s in held for s in range(first[f], first[f + 1])) for f in range(3)) and st["windows"] == 3
    if name == "an all-zero source that never lands":
        assert st["merged_windows"] == 1 and got["extents"][-1][1] == len(got["bytes"])


def test_resync_windows_model():
    old = [0, 100, 250, 400, 900]
    x = [0, 50, 120, 300, 300 + 80, 300 + 130, 300 + 200]
    first = [0, 3, 6]
    # window 0: cut 120 + 130 = 250 is old[2]; window 1 (buffer offset 300): only its last cut hits, which counts when final
    wins = [(0, 130, 0, 5, 0), (0, (900 - 500) % XM.M, 0, 5, 0)]
    assert XM.resync_windows(x, first, wins, old) == [[0, 2, 2, 120], [1, 0, 0, 0]]
    wins[1] = (0, 400, 0, 5, 1)
    assert XM.resync_windows(x, first, wins, old)[1] == [0, 3, 4, 500]
    # below new_from, and outside the window's own old range
    assert XM.resync_windows(x, first, [(121, 130, 0, 5, 0), (0, 0, 0, 0, 0)], old)[0] == [1, 0, 0, 0]
    assert XM.resync_windows(x, first, [(0, 130, 3, 2, 0), (0, 0, 0, 0, 0)], old)[0] == [1, 0, 0, 0]
