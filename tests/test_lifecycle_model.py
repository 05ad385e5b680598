"""tests/lifecycle_model.py alone: every life-cycle script runs through the whole-store model, the store's invariants hold after every
step, a refused step changes nothing, and each script reaches the edge it is named for -- so the GPU run of the same steps
(tests/test_gpu_lifecycle.py) cannot miss it silently."""
import numpy as np
import pytest

import cdc_model as CM
import guard2_model as G2
import lifecycle_model as LM
import restore_model as RM

ALGS = ["lz4", "lzf"]
P = LM.P


def invariants(s: LM.Store, where):
    values = s.m.values
    damaged = s.hurt
    for name, st in s.streams.items():
        assert st.cuts == (CM.chunk(st.bytes, P) if st.bytes else [0]), (where, name)
        assert st.refs == [values[c] for c in st.chunks()], (where, name, "a ref is not the value of its content")
        if not damaged:
            got = RM.restore(s.m.blob, s.store_bytes, s.m.directory, s.dir_base, st.refs, st.cuts, st.cuts[-1], s.m.decode())
            assert all(status == 0 for status, _ in got) and b"".join(piece for _, piece in got) == st.bytes, (where, name)
    assert len(set(values.values())) == len(values), (where, "two contents share a value")
    for v in values.values():
        idx = v - s.dir_base
        assert not 0 <= idx < s.dir_entries or any(int(x) for x in s.m.directory[idx]), (where, v, "a value of the directory names a zero entry")
    assert set(values) == s.made, (where, len(values), len(s.made))
    assert s.dir_base <= s.base and s.used <= s.store_bytes and len(values) <= s.max_entries
    g = s.guard
    if g is not None:                                                    # after every step, refused or not: the cursor is ``used``
        assert g.covered == s.used and len(g.P) == G2.guard_bytes(max(s.store_bytes, 1), g.stripe, g.group), where
        assert (g.Q is None) == (g.parity == 1) and (g.Q is None or len(g.Q) == len(g.P)), where
        if not s.flipped:                                                # ... and the guard is exact, zero tail included
            p, q = G2.guards_of(s._stored(), s.used, g.stripe, g.group, max(s.store_bytes, 1))
            assert (g.P == p).all() and (g.Q is None or (g.Q == q).all()), (where, "the guard is not exact")
            assert s.guard_check()["count"] == 0, where


def play(sc, oracle, alg):
    """(step index, op, args, result, the stores) after every step of the script on a fresh model"""
    stores = LM.new_stores(oracle, alg, sc["specs"])
    for i, (op, args, expect) in enumerate(sc["steps"]):
        before = {n: s.snapshot() for n, s in stores.items()}
        got = LM.run(stores, op, args)
        assert got["code"] == expect, (sc["name"], i, op, got)
        same = {n: s.snapshot() for n, s in stores.items()} == before
        if (expect and op not in LM.PARTIAL) or op in READ_ONLY:
            assert same, (sc["name"], i, op, "changed the state")
        for n, s in stores.items():
            invariants(s, (sc["name"], i, op, n))
        yield i, op, args, dict(got, same=same), stores


READ_ONLY = ("scrub", "account", "affected", "restore", "read_ranges", "diff", "save_load", "restore_many_stream", "guard_check")


@pytest.mark.parametrize("name", LM.NAMES)
@pytest.mark.parametrize("alg", ALGS)
def test_script_keeps_the_invariants_and_reaches_its_edge(oracle, alg, name):
    reaches_its_edge(LM.script(oracle, alg, name), oracle, alg, name)


@pytest.mark.parametrize("name", LM.UNGUARDED)
@pytest.mark.parametrize("alg", ALGS)
def test_protected_script_keeps_the_invariants_and_reaches_its_edge(oracle, alg, name):
    """The same steps behind a ``protect`` on every store: the same edges, and after every step, refused or not, an exact guard."""
    sc = LM.protected(LM.script(oracle, alg, name), alg)
    assert [op for op, _, _ in sc["steps"][:len(sc["specs"])]] == ["protect"] * len(sc["specs"])
    reaches_its_edge(sc, oracle, alg, name)


def reaches_its_edge(sc, oracle, alg, name):
    notes = {(i, key): value for key, hits in sc["notes"].items() for i, value in hits}
    seen, prev = set(), {}
    for i, op, args, got, stores in play(sc, oracle, alg):
        s = stores[args.get("store", "P")]
        state = dict(base=s.base, K=s.stored_chunks(), holes=s.holes(), contents=set(s.m.values), entries=s.dir_entries, used=s.used)
        was = prev.get(args.get("store", "P"), state)
        for (at, key), value in notes.items():
            if at != i:
                continue
            seen.add(key)
            if key == "full":
                assert s.base == s.dir_base + s.dir_entries, (name, i, "the directory is not exactly full")
            elif key == "room":
                assert s.dir_entries - state["K"] == value and s.base == s.dir_base + state["K"] and value >= 1
            elif key == "refused":
                assert got["code"] == -5 and got["why"] == value and s.base == was["base"], (name, i, got)
            elif key == "dropped":
                dropped, new_chunks = value
                assert got["dropped_contents"] == dropped == was["contents"] - state["contents"] and len(dropped) == new_chunks > 0
                prev["dropped"] = dropped
            elif key == "rebuilt":
                assert state["contents"] - was["contents"] == prev["dropped"] and got["new_chunks"] == len(prev["dropped"]) == value
                assert s.base == was["base"] + got["window_chunks"]
            elif key == "all_duplicates":
                lo, hi = got["window"]
                assert got["t"] == value and got["new_chunks"] == 0 and state["holes"] == was["holes"] + value and state["K"] == was["K"]
                assert s.streams[args["dst"]].bytes[lo:hi] == bytes(hi - lo), "the window lies inside the zero run"
            elif key == "renumbered":
                assert state["K"] == was["K"] and was["holes"] >= 3 and state["holes"] == 0 and s.base == was["base"] - was["holes"]
            elif key == "damaged":
                assert got["damaged"] == value and len(value) == 2
                assert sorted(int(got["status"][v - s.dir_base]) for v in value)[1] == 3, "the raw chunk decodes and does not hash"
            elif key == "affected":
                assert [(i, n) for i, n, _ in got["affected"]] == [(0, value)], "the scrub's damage names A, at two positions"
            elif key == "clean":
                assert got["damaged"] == []
            elif key == "window_reads":
                old = s.streams[args["src"]]
                assert (old.cuts[got["j"]], old.cuts[got["j"] + 1]) == value, "the window does not begin with the replaced chunk"
            elif key == "negotiated":
                assert 0 < value[0] < value[1]
            elif key == "cut_in_carry":
                assert LM.cut_in_carry(args["data"], value) and len(got["run"].pieces) >= 4
            elif key == "edges":
                assert len(value) >= 3
            elif key == "edits":
                prev["edits"] = value
            elif key == "reports":
                assert got["damaged"] == value and value, (name, i, got["damaged"])
                prev["reports"] = value
            elif key == "all_paired":                                    # every damaged chunk has a partner, and all come back
                assert got["repaired"] == prev["reports"] and got["paired"] == 2 * value == len(got["repaired"]) and value >= 2, (name, i, got)
                assert not (got["collided"] or got["unprotected"] or got["failed"] or got["no_digest"]) and not s.hurt and not s.flipped
            elif key == "repair":
                assert {k: got[k] for k in value} == value, (name, i, got)
            elif key == "guard_check":
                assert {k: got[k] for k in value} == value, (name, i, got)
            elif key == "nothing_changed":                               # the stored bytes, the guards and the cursor among it
                assert got["same"], (name, i)
            elif key == "some_failed":
                assert got["failed"] and sorted(got["failed"] + got["repaired"] + got["collided"]) == value, (name, i, got)
            elif key == "fresh_guard":
                g = s.guard
                assert (g.stripe, g.group, g.parity) == value[:3] and len(g.P) != value[3] and g.covered == s.used and not s.flipped
            elif key == "part_way":
                total = sum(len(d) for d in args.get("datas", [args.get("data", b"")]))
                assert got["code"] == -5 and got["why"] == "store" and 0 < value == got["run"].consumed < total, (name, i, value)
                assert s.guard.covered == s.used > was["used"] and not got["same"]
        if op == "diff" and "edits" in prev:
            new_ops = [o for o in got["ops"] if o[2] == LM.NONE]
            at, shift = [], 0
            for o, r, d in prev["edits"]:                                # where each edit lies in the new stream
                at.append((o + shift, o + shift + len(d)))
                shift += len(d) - r
            assert len(new_ops) == len(at)
            for (b, n, _, _), (lo, hi) in zip(new_ops, at):
                assert b <= lo and hi <= b + n and n <= hi - lo + 6 * P["max"], (name, "a new op does not cover exactly one edit", (b, n), (lo, hi))
        if op == "delta_round_trip":
            new = s.streams[args["new"]]
            assert got["plain"] == new.bytes and s.streams[args["dst"]].refs == new.refs and got["inside"]["new_chunks"] == 0
        prev[args.get("store", "P")] = state
    assert seen == set(sc["notes"]), (name, "a note was not reached")


def test_every_script_is_there_and_small(oracle):
    for alg in ALGS:
        got = LM.scripts(oracle, alg)
        assert [sc["name"] for sc in got] == list(LM.NAMES)
        for sc in got:
            for op, args, _ in sc["steps"]:
                for d in [args.get("data", b"")] + list(args.get("datas", [])):
                    assert len(d) <= 60000
    assert np.dtype(RM.LOC).itemsize == 16
