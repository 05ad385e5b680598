"""The diff rule and the delta it yields (tests/delta_model.py) over real cuts: a stream of text, a zero run and noise is chunked by
cdc_model.chunk, content hashes stand for refs, and a few hundred seeded edits check that the delta rebuilds the new bytes from the
old ones, both ways, and that the ops say what the rule says they say."""
import hashlib

import numpy as np
import pytest

import cdc_model as CM
import delta_model as DM
from conftest import corpus_file

P = CM.default_params(1024)          # chunks of 256 .. 8192 bytes
TRIALS = 240


def base_stream() -> bytes:
    rng = np.random.default_rng(26)
    return corpus_file("alice29.txt")[:60000] + bytes(200_000) + rng.integers(0, 256, 40_000, dtype=np.uint8).tobytes()


class Refs:
    """content hash -> a dense value, as a store's index would hand them out"""

    def __init__(self, dir_base=7):
        self.dir_base, self.values = dir_base, {}

    def recipe(self, data: bytes):
        cuts = CM.chunk(data, P)
        refs = [self.values.setdefault(hashlib.blake2b(data[a:b], digest_size=16).digest(), self.dir_base + len(self.values))
                for a, b in zip(cuts, cuts[1:])]
        return refs, cuts

    @property
    def entries(self):
        return max(len(self.values), 1)


def edited(rng, data: bytes) -> bytes:
    """0 to 5 edits: overwrite, insert, removal, append, truncation"""
    out = bytearray(data)
    for _ in range(int(rng.integers(0, 6))):
        kind, n = int(rng.integers(0, 5)), len(out)
        at, size = int(rng.integers(0, n + 1)), int(rng.integers(1, 5000))
        fresh = rng.integers(0, 256, size, dtype=np.uint8).tobytes()
        if kind == 0:
            out[at:at + size] = fresh[:max(min(size, n - at), 0)]
        elif kind == 1:
            out[at:at] = fresh
        elif kind == 2:
            del out[at:at + size]
        elif kind == 3:
            out += fresh
        else:
            del out[max(n - size, 0):]
    return bytes(out)


def tiles(ops, nbytes):
    end = 0
    for b, n, a, p in ops:
        assert b == end and n >= 1 and (a == DM.NONE) != (p == DM.NONE), (b, n, a, p)
        end += n
    assert end == nbytes


@pytest.fixture(scope="module")
def base():
    data = base_stream()
    refs = Refs()
    return data, refs, refs.recipe(data)


def test_delta_rebuilds_the_new_stream_both_ways(base):
    old, refs, (ref_a, off_a) = base
    rng = np.random.default_rng(2600)
    seen = dict(empty=0, identical=0, moved=0, new=0, copy_ops=0)
    for trial in range(TRIALS):
        new = edited(rng, old)
        ref_b, off_b = refs.recipe(new)
        for (ra, oa, da), (rb, ob, db) in (((ref_a, off_a, old), (ref_b, off_b, new)), ((ref_b, off_b, new), (ref_a, off_a, old))):
            d = DM.diff(ra, oa, rb, ob, refs.dir_base, refs.entries)
            assert d["verdict"] == 0
            ops, t = d["ops"], d["totals"]
            tiles(ops, len(db))
            assert all(a + n <= len(da) for _, n, a, _ in ops if a != DM.NONE), "a copy op leaves A"
            payload = DM.payload_of(db, ops)
            assert DM.apply(da, payload, ops) == db
            # the new bytes are the lengths of the positions whose ref A lacks
            in_a = set(ra)
            lacks = sum(ob[i + 1] - ob[i] for i in range(len(rb)) if rb[i] not in in_a)
            assert t[5] == len(payload) == lacks and t[3] + t[4] + t[5] == len(db) and t[7] == len(rb)
            assert t[1] == len(ops) and t[2] == sum(a == DM.NONE for _, _, a, _ in ops) == len(d["ranges"])
            assert [(o - ob[0], n, p) for o, n, p in d["ranges"]] == [(b, n, p) for b, n, a, p in ops if a == DM.NONE]
            assert len(d["src"]) == len(rb)
            seen["empty"] += len(db) == 0
            seen["identical"] += da == db
            seen["moved"] += t[4] > 0
            seen["new"] += t[5] > 0
            seen["copy_ops"] += t[1] - t[2]
    assert seen["moved"] > 50 and seen["new"] > 50 and seen["identical"] > 5, seen


def test_a_recipe_against_itself_is_one_in_place_op(base):
    old, refs, (ref_a, off_a) = base
    d = DM.diff(ref_a, off_a, ref_a, off_a, refs.dir_base, refs.entries)
    assert d["ops"] == [(0, len(old), 0, DM.NONE)] and d["totals"] == [0, 1, 0, len(old), 0, 0, len(ref_a), len(ref_a)]
    assert DM.diff([], [0], [], [5], 0, 1)["ops"] == []                               # two empty streams: no op
    assert DM.diff(ref_a, off_a, [], [0], refs.dir_base, refs.entries)["totals"] == [0, 0, 0, 0, 0, 0, 0, 0]
    shifted = [o + 12345 for o in off_a]                                              # any coordinates
    assert DM.diff(ref_a, shifted, ref_a, off_a, refs.dir_base, refs.entries)["ops"] == d["ops"]


def test_a_shifted_run_of_one_chunk_costs_an_op_per_chunk(base):
    """The lowest-position rule inside the 200 KB zero run (chunks of max_size, all one ref): after an insert in front of it every
    chunk of the run is `moved` from the run's first chunk, one op each; in place the run is one op."""
    old, refs, (ref_a, off_a) = base
    new = old[:100] + b"x" * 37 + old[100:]
    ref_b, off_b = refs.recipe(new)
    d = DM.diff(ref_a, off_a, ref_b, off_b, refs.dir_base, refs.entries)
    run = 200_000 // P["max"]
    assert run <= d["totals"][1] <= run + 12, d["totals"]
    assert DM.apply(old, DM.payload_of(new, d["ops"]), d["ops"]) == new


def test_verdicts_and_the_dry_run():
    ref, off = [5, 6, 7], [0, 10, 30, 31]
    assert DM.diff(ref, [0, 10, 10, 31], ref, off)["verdict"] == 1                     # an equal pair
    assert DM.diff(ref, off, ref, [0, 10, 9, 31])["verdict"] == 1                      # a decreasing pair
    assert DM.diff(ref, [0, 10, 10 + 65537, 70000], ref, off)["verdict"] == 1          # an extent of 65,537
    assert DM.diff(ref, [0, 10, 10 + 65536, 70000], ref, off)["verdict"] == 0
    full = DM.diff([5, 6], [0, 10, 30], [9, 5, 9, 6], [0, 3, 13, 20, 40])
    assert full["ops"] == [(0, 3, DM.NONE, 0), (3, 10, 0, DM.NONE), (13, 7, DM.NONE, 3), (20, 20, 10, DM.NONE)]
    dry = DM.diff([5, 6], [0, 10, 30], [9, 5, 9, 6], [0, 3, 13, 20, 40], max_ops=3)
    assert dry["verdict"] == 2 and dry["ops"] == [] and dry["ranges"] == [] and dry["totals"][1:] == full["totals"][1:]
    # outside the directory: always new, and no source
    out = DM.diff([5, DM.NONE, 2], [0, 1, 2, 3], [5, DM.NONE, 2, 8], [0, 1, 2, 3, 4], dir_base=3, dir_entries=5)
    assert out["src"] == [0, DM.NONE, DM.NONE, DM.NONE] and out["ops"] == [(0, 1, 0, DM.NONE), (1, 3, DM.NONE, 0)]
    # equal ref, other length: new; an in-place match beats a lower position
    assert DM.diff([5], [0, 10], [5], [0, 11])["src"] == [DM.NONE]
    assert DM.diff([5, 6, 5], [0, 4, 8, 12], [6, 6, 5], [0, 4, 8, 12])["src"] == [4, 4, 8]


def test_check_names_the_lowest_bad_op():
    good = [(0, 5, 0, DM.NONE), (5, 3, DM.NONE, 0), (8, 2, 8, DM.NONE)]
    assert DM.check(good, 10, 3, 10) == (0, 10, DM.NONE, 3) and DM.check(good, 10, 3, 9) == (2, 10, DM.NONE, 3)
    assert DM.check([], 0, 0, 0) == (0, 0, DM.NONE, 0)
    bad = {
        "gap": [(0, 5, 0, DM.NONE), (6, 3, DM.NONE, 0)], "overlap": [(0, 5, 0, DM.NONE), (4, 3, DM.NONE, 0)],
        "empty": [(0, 5, 0, DM.NONE), (5, 0, DM.NONE, 0)], "both": [(0, 5, 0, DM.NONE), (5, 3, DM.NONE, DM.NONE)],
        "neither": [(0, 5, 0, DM.NONE), (5, 3, 0, 0)], "wrap": [(0, 5, 0, DM.NONE), (5, DM.M - 5, 0, DM.NONE)],
        "old": [(0, 5, 0, DM.NONE), (5, 3, 8, DM.NONE)], "payload": [(0, 5, 0, DM.NONE), (5, 3, DM.NONE, 1)],
        "start": [(0, 5, 0, DM.NONE), (1, 5, 0, DM.NONE)]}
    for name, ops in bad.items():
        assert DM.check(ops, 10, 3, 100) == (1, 0, 1, 2), name
    assert DM.check([(1, 5, 0, DM.NONE)], 10, 3, 100)[:3] == (1, 0, 0)                # op 0 starts at 0
    with pytest.raises(ValueError):
        DM.apply(bytes(10), bytes(3), bad["gap"])
