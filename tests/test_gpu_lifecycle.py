"""The chunk store's life cycle on the GPU: every script of tests/lifecycle_model.py runs step by step on ``cw.ChunkStore`` and on the
whole-store model, and after every step the whole device state is compared with the model, exactly: ``used()``, the stored bytes, the
directory, the index as {digest: value}, ``base`` / ``dir_base`` / ``dir_entries``, every live recipe's refs and offsets,
``restore(recipe, verify=True)`` and the statistics of the last patch and compose; of a protected store also the guard's geometry, its
cursor (``protected_bytes() == used()``), the whole of ``d_guard`` and ``d_guard_q`` and ``guard_check(detail=True)``.  After a refused
step the device state is what it was before the step -- but for the prefix that a streamed ingest leaves, which is the model's.  The
eight unguarded scripts run once more with ``protect`` as the first step on every store.  What each script has to reach is asserted on
the model alone, in tests/test_lifecycle_model.py."""
import numpy as np
import pytest

import lifecycle_model as LM
import restore_model as RM

pytestmark = pytest.mark.gpu
ALGS = ["lz4", "lzf"]
DIGEST = {}
TOTALS = ("nonzero", "nonzero_stored", "referenced", "referenced_stored", "shared", "shared_stored", "missing")   # of an Account


@pytest.fixture(scope="module")
def cw():
    import torch  # noqa: F401  (one HIP runtime for torch and libcwhc.so)
    import compute_war_amd as cw
    cw.init(0)
    yield cw
    cw.tune_reset()


def digest(oracle, content: bytes) -> bytes:
    if content not in DIGEST:
        DIGEST[content] = oracle.skein512(content)
    return DIGEST[content]


def guard_state(cs):
    """The guard of a protected store: geometry, cursor, and every byte of P and Q."""
    if cs.d_guard is None:
        return None
    return (cs.stripe, cs.group, cs.d_guard_q is None, cs.protected_bytes(), cs.d_guard.cpu().numpy().tobytes(),
            None if cs.d_guard_q is None else cs.d_guard_q.cpu().numpy().tobytes())


def device_state(cs):
    """Everything of a store that a refused step must leave alone (the index as a set of pairs: a retain rebuilds its table)."""
    dig, val = cs.index.export()
    return (frozenset((bytes(d), int(v)) for d, v in zip(dig, val)), cs.d_dir.cpu().numpy().tobytes(), cs.used(),
            cs.d_store[:cs.used()].cpu().numpy().tobytes(), cs.base, cs.dir_base, cs.dir_entries, cs.store_bytes, guard_state(cs))


class Env:
    """The device side of a script: the stores by name, the recipes by (store, stream name), the last scrub report of each store."""

    def __init__(self, cw, oracle, alg, specs, tmp_path):
        self.cw, self.oracle, self.tmp_path, self.stores, self.recipes, self.reports = cw, oracle, tmp_path, {}, {}, {}
        for name, kw in specs.items():
            self.stores[name] = cw.ChunkStore(cw.DedupeIndex("skein512", kw["max_entries"]), alg, cw.CdcParams.default(256), kw["store_bytes"],
                                              kw["dir_entries"], kw["dir_base"])

    def close(self):
        for cs in self.stores.values():
            cs.index.close()

    def same_as_model(self, models, where):
        for name, cs in self.stores.items():
            m, at = models[name], (where, name)
            used = cs.used()
            assert used == m.used, at
            assert cs.d_store[:used].cpu().numpy().tobytes() == bytes(m.m.blob), (at, "stored bytes")
            got = cs.d_dir.cpu().numpy().view(RM.LOC)
            assert len(got) == len(m.m.directory), at
            bad = np.nonzero(got != m.m.directory)[0]
            assert len(bad) == 0, (at, "entry", int(bad[0]), got[bad[0]], m.m.directory[bad[0]], len(bad))
            dig, val = cs.index.export()
            have = {bytes(d): int(v) for d, v in zip(dig, val)}
            want = {digest(self.oracle, c): v for c, v in m.m.values.items()}
            assert len(have) == len(val) and have == want, (at, "index", len(have), len(want), sorted(set(have.values()) ^ set(want.values()))[:8])
            assert (cs.base, cs.dir_base, cs.dir_entries, cs.store_bytes) == (m.base, m.dir_base, m.dir_entries, m.store_bytes), at
            g = m.guard
            assert (cs.d_guard is None) == (g is None), at
            if g is not None:
                assert cs.protected_bytes() == used == g.covered, (at, "cursor", cs.protected_bytes(), g.covered)
                assert guard_state(cs) == (g.stripe, g.group, g.Q is None, g.covered, g.P.tobytes(), None if g.Q is None else g.Q.tobytes()), (at, "guard")
                want = m.guard_check()
                assert cs.guard_check(detail=True) == (want["count"], want["groups"], want["bits"]), (at, "guard_check")
            damaged = m.hurt
            for stream, st in m.streams.items():
                r = self.recipes[name, stream]
                assert r.refs.tolist() == st.refs and r.offsets.tolist() == st.cuts, (at, stream, "recipe")
                if not damaged:
                    assert cs.restore(r, verify=True) == st.bytes, (at, stream, "restore")

    def step(self, op, args, want):
        """One step on the device; ``want`` is the model's result of the same step.  Raises what the store raises."""
        cw, args = self.cw, dict(args)
        store = args.pop("store", "P")
        cs = self.stores[store]
        R = lambda n: self.recipes[store, n]  # noqa: E731

        def piece(size, call):
            cw.tune_set("CW_STORE_PIECE", str(size))
            try:
                return call()
            finally:
                cw.tune_set("CW_STORE_PIECE", None)

        def parts_of(parts):
            return [(R(p[0]), p[1], p[2]) if isinstance(p, tuple) else p for p in parts]

        def composed(recipe):
            self.recipes[store, args["dst"]] = recipe
            assert {k: cs.last_compose[k] for k in ("rebuilt_chunks", "new_chunks", "stored_bytes")} == \
                {k: want[k] for k in ("rebuilt_chunks", "new_chunks", "stored_bytes")}, cs.last_compose

        if op == "ingest":
            self.recipes[store, args["name"]] = cs.ingest(args["data"])
        elif op == "ingest_many":
            for n, r in zip(args["names"], cs.ingest_many(args["datas"])):
                self.recipes[store, n] = r
        elif op in LM.PARTIAL:                                               # a refusal leaves the recipes of the prefix that went in
            one = op == "ingest_stream"
            names, refusal = [args["name"]] if one else args["names"], None
            try:
                got = piece(args["piece"], lambda: [cs.ingest_stream(args["data"])] if one else cs.ingest_many_stream(args["datas"]))
            except cw.CwError as e:
                refusal = e
                got = [e.recipe] if one else e.recipes + [e.partial] * (e.partial is not None)
                assert (e.consumed, e.nchunks) == (want["run"].consumed, want["run"].nchunks), (e.consumed, e.nchunks)
            for n, r in zip(names, got):
                self.recipes[store, n] = r
            assert {k: cs.last_stats[k] for k in want["stats"]} == want["stats"], cs.last_stats
            if refusal is not None:
                raise refusal
        elif op == "patch":
            self.recipes[store, args["dst"]] = cs.patch(R(args["src"]), args["a"], args["r"], args["ins"], args.get("lookahead", 0))
            assert {k: cs.last_patch[k] for k in ("window_chunks", "new_chunks", "stored_bytes")} == \
                {k: want[k] for k in ("window_chunks", "new_chunks", "stored_bytes")}, cs.last_patch
            assert (cs.last_patch["first_position"], cs.last_patch["resume_position"], cs.last_patch["attempts"]) == (want["j"], want["s"], want["attempts"])
        elif op == "compose":
            composed(cs.compose(parts_of(args["parts"]), args.get("lookahead", 0)))
        elif op == "concat":
            composed(cs.concat([R(n) for n in args["names"]]))
        elif op == "edit":
            composed(cs.edit(R(args["src"]), args["edits"]))
        elif op == "delta_round_trip":
            old, new = R(args["old"]), R(args["new"])
            d = cs.delta(old, new)
            assert [tuple(int(v) for v in o) for o in d.ops.tolist()] == want["ops"] and d.payload.tobytes() == want["payload"]
            assert cw.apply_delta(cs.restore(old), d) == want["plain"]
            self.recipes[store, args["dst"]] = cs.apply_delta(old, d)
            assert {k: cs.last_compose[k] for k in ("rebuilt_chunks", "new_chunks", "stored_bytes")} == \
                {k: want["inside"][k] for k in ("rebuilt_chunks", "new_chunks", "stored_bytes")}, cs.last_compose
        elif op == "diff":
            d = cs.diff(R(args["old"]), R(args["new"]))
            assert [tuple(int(v) for v in o) for o in d.ops.tolist()] == want["ops"] and d.src.tolist() == want["src"]
            assert [d.totals[k] for k in cw.DIFF_TOTALS] == want["totals"]
        elif op == "compact":
            got = cs.compact([R(n) for n in args["keep"]], args.get("store_bytes"))
            assert got == {k: want[k] for k in ("kept", "dropped", "bytes_before", "bytes_after", "removed")}, got
        elif op == "renumber":
            for n, r in zip(args["keep"], cs.renumber([R(n) for n in args["keep"]], args.get("dir_entries"), args.get("dir_base"))):
                self.recipes[store, n] = r
        elif op == "restore":
            assert cs.restore(R(args["name"]), verify=True) == want["bytes"]
        elif op == "read_ranges":
            assert cs.read_ranges(R(args["name"]), args["ranges"]) == want["bytes"]
        elif op == "account":
            a = cs.account([R(n) for n in args["names"]])
            for k in want["streams"].dtype.names:
                assert a.streams[k].tolist() == want["streams"][k].tolist(), k
            assert a.refcount.tolist() == want["refcount"].tolist() and a.owner.tolist() == want["owner"].tolist()
            assert [a.totals[k] for k in TOTALS] == want["totals"]
        elif op in ("corrupt", "corrupt_unlisted"):
            cs.d_store[want["pos"]:want["pos"] + 1].bitwise_xor_(0xFF)
        elif op == "corrupt_guard":
            (cs.d_guard, cs.d_guard_q)[args["which"]][want["at"]:want["at"] + 1].bitwise_xor_(0xFF)
        elif op == "protect":
            cs.protect(**args)
        elif op == "guard_check":
            assert cs.guard_check(detail=True) == (want["count"], want["groups"], want["bits"])
        elif op == "repair_local":
            got = cs.repair_local(self.reports[store], **args)
            assert got == {k: want[k] for k in ("repaired", "collided", "unprotected", "failed", "no_digest")}, got
            assert cs.last_repair == dict(paired=want["paired"]), cs.last_repair
        elif op == "scrub":
            rep = cs.scrub(None if args.get("keep") is None else [R(n) for n in args["keep"]])
            assert rep.status.tolist() == want["status"].tolist() and rep.damaged.tolist() == want["damaged"]
            self.reports[store] = rep
        elif op == "affected":
            assert cs.affected([R(n) for n in args["names"]], self.reports[store]) == want["affected"]
        elif op == "repair_from":
            got = cs.repair_from(self.stores[args["peer"]], self.reports[store])
            assert got == {k: want[k] for k in ("repaired", "unavailable", "no_digest")}, got
        elif op == "replicate_to":
            to = args["to"]
            mine = [R(n) for n in args["names"]]
            if args.get("negotiate", True):
                theirs = cs.replicate_to(self.stores[to], mine)
            else:                                                            # every chunk travels, through a file
                path = str(self.tmp_path / f"{store}_to_{to}.npz")
                cs.export_bundle(mine).save(path)
                bundle = cw.Bundle.load(path)
                assert int(bundle.carried.sum()) == len(bundle.values) == want["listed"] == want["carried"]
                theirs = self.stores[to].import_bundle(bundle)
            for n, r in zip(args["as_names"], theirs):
                self.recipes[to, n] = r
        elif op == "save_load":
            path = str(self.tmp_path / f"{store}.npz")
            cs.save(path)
            loaded = cw.ChunkStore.load(path)
            cs.index.close()
            self.stores[store] = loaded
            assert [loaded.restore(R(n), verify=True) for n in args["names"]] == want["bytes"]
        elif op == "restore_many_stream":
            assert cs.restore_many_stream([R(n) for n in args["names"]]) == want["bytes"]
        else:
            raise AssertionError(f"no such step: {op}")


@pytest.mark.parametrize("name", LM.NAMES)
@pytest.mark.parametrize("alg", ALGS)
def test_script_leaves_what_the_model_leaves_after_every_step(cw, oracle, tmp_path, alg, name):
    leaves_what_the_model_leaves(cw, oracle, tmp_path, alg, name, LM.script(oracle, alg, name))


@pytest.mark.parametrize("name", LM.UNGUARDED)
@pytest.mark.parametrize("alg", ALGS)
def test_protected_script_leaves_what_the_model_leaves_after_every_step(cw, oracle, tmp_path, alg, name):
    leaves_what_the_model_leaves(cw, oracle, tmp_path, alg, name, LM.protected(LM.script(oracle, alg, name), alg))


def leaves_what_the_model_leaves(cw, oracle, tmp_path, alg, name, sc):
    models = LM.new_stores(oracle, alg, sc["specs"])
    env = Env(cw, oracle, alg, sc["specs"], tmp_path)
    try:
        for i, (op, args, expect) in enumerate(sc["steps"]):
            where = (name, i, op)
            want = LM.run(models, op, args)
            assert want["code"] == expect, where
            if expect:
                before = {n: device_state(cs) for n, cs in env.stores.items()}
                with pytest.raises(cw.CwError) as e:
                    env.step(op, args, want)
                assert e.value.code == expect, (where, str(e.value))
                if op not in LM.PARTIAL or want["run"].consumed == 0:
                    assert {n: device_state(cs) for n, cs in env.stores.items()} == before, (where, "a refused step changed the device state")
            else:
                env.step(op, args, want)
            env.same_as_model(models, where)
    finally:
        env.close()
