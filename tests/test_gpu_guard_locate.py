"""Locating damage from the guard's syndromes on the GPU (cw_dev_store_guard_locate, cw_dev_store_guard2_locate and
cw.ChunkStore.guard_locate / scrub(values=) / heal): everything compared exactly with guard_locate_model.py.
S = 65536 with G in {1, 2, 4, 16} through both calls, G = 255 through the dual call and G = 256 through the single one, hand-built
directories with poison around d_suspect and d_result; one store whose cursor lies above 2^32; then whole stores of corpus text at
parity 1 and 2: protect, ingest, damage, heal."""
import numpy as np
import pytest

import guard_locate_model as LM
import guard_model as GM
import past4g
from test_gpu_guard import DIR_BASE, Guard, _dev_bytes, _dev_u64, _stream, _sync, _u64, directory_of, text

pytestmark = pytest.mark.gpu

S = LM.S
PAD = 64                                                   # poisoned u32 words around d_suspect
POISON32, POISON64 = 0xEEEEEEEE, 0xEEEEEEEEEEEEEEEE
GEOMETRIES = [(G, dual) for G in (1, 2, 4, 16) for dual in (False, True)] + [(255, True), (256, False)]
# the cases of the two largest groups, whose model walks 16 MiB per case: what the number of members can change
LARGE = ("no damage", "member 0", "member G - 1", "position covered - 1", "a cell of the last group", "across a group boundary, both pieces",
         "a byte no entry names", "a changed Q byte", "two wrong bytes, equal deltas", "two wrong bytes that alias",
         "unsound, all-zero and above-cursor entries")


@pytest.fixture(scope="module")
def cw():
    import torch  # noqa: F401  (one HIP runtime for torch and libcwhc.so)
    import compute_war_amd as cw
    cw.init(0)
    yield cw
    cw.tune_reset()


@pytest.fixture(scope="module")
def stores(cw):
    """Per G: noise on the host and on the device (written only between a case's damage and its undoing), and the model's clean
    (P, Q) per cursor, each computed once."""
    cache = {}

    def get(G, covered):
        if G not in cache:
            host = np.random.default_rng(31 + G).integers(0, 256, LM.store_bytes_of(G), dtype=np.uint8)
            cache[G] = (host, _dev_bytes(host), {})
        host, dev, guards = cache[G]
        if covered not in guards:
            p, q, _ = LM.syndromes(host, covered, S, G)
            size = GM.guard_bytes(len(host), S, G)
            guards[covered] = (np.pad(p, (0, size - len(p))), np.pad(q, (0, size - len(q))))
        return host, dev, guards[covered]
    return get


def locate(cw, d_store, store_bytes, directory, dir_base, covered, G, p, q, d_p=None, d_q=None):
    """One call (dual when q is not None) with poison around both outputs: (d_result[8], d_suspect or None when it is still poison).
    p and q are host arrays put between poisoned pads, unless the device pointers d_p / d_q and the guards' size p are given."""
    n = len(directory)
    if d_p is None:
        gp, gq = Guard(p, covered), None if q is None else Guard(q, covered)
        d_p, d_q, size, d_covered = gp.ptr(), None if q is None else gq.ptr(), gp.size, gp.d_covered
    else:
        size, d_covered = p, _dev_u64([covered])
    d_dir = _dev_bytes(directory)
    suspect = _dev_bytes(np.full(n + 2 * PAD, POISON32, np.uint32))
    result = _dev_u64([POISON64] * 10)
    _sync()
    if d_q is None:
        cw.dev_store_guard_locate(d_store.data_ptr(), store_bytes, d_dir.data_ptr(), dir_base, n, d_covered.data_ptr(), S, G, d_p, size,
                                  suspect.data_ptr() + 4 * PAD, result.data_ptr() + 8, _stream())
    else:
        cw.dev_store_guard2_locate(d_store.data_ptr(), store_bytes, d_dir.data_ptr(), dir_base, n, d_covered.data_ptr(), S, G, d_p, d_q, size,
                                   suspect.data_ptr() + 4 * PAD, result.data_ptr() + 8, _stream())
    _sync()
    r, s = _u64(result).tolist(), suspect.cpu().numpy().view(np.uint32)
    assert r[0] == POISON64 and r[9] == POISON64, "a store left d_result"
    assert (s[:PAD] == POISON32).all() and (s[PAD + n:] == POISON32).all(), "a store left d_suspect"
    assert int(_u64(d_covered)[0]) == covered
    body = s[PAD:PAD + n]
    return r[1:9], None if (body == POISON32).all() else body.copy()


@pytest.mark.parametrize("G,dual", GEOMETRIES)
def test_named_cases(cw, stores, G, dual):
    for k, (name, case) in enumerate(LM.cases(G).items()):
        if G >= 255 and name not in LARGE:
            continue
        full = LM.store_bytes_of(G)
        covered = full if case.covered is None else case.covered
        host, dev, (p, q) = stores(G, covered)
        s, dp, dq = LM.damaged(host, p, q if dual else None, case.damage)
        directory = LM.records(case.entries)
        want_result, want = LM.locate(s, full, directory, covered, S, G, dp, dq)
        assert want.tolist() == (case.dual if dual else case.single), name
        hurt = [(at, xor) for what, at, xor in case.damage if what == "s"]
        for at, xor in hurt:
            dev[at] ^= xor
        try:
            result, suspect = locate(cw, dev, full, directory, DIR_BASE if k & 1 else 0, covered, G, dp, dq)
        finally:
            for at, xor in hurt:
                dev[at] ^= xor
            _sync()
        print(f"G {G} dual {dual} {name}: result {result} suspect {None if suspect is None else suspect.tolist()}")
        assert result == want_result, name
        assert suspect is not None and suspect.tolist() == want.tolist(), name
        if not case.damage:
            assert result[2:6] == [0, 0, 0, 0], name


@pytest.mark.parametrize("G,dual", [(2, False), (4, True)])
def test_many_entries_and_scattered_damage(cw, stores, G, dual):
    """More entries than one workgroup has lanes, extents of every length from 1 to 65536 laid end to end, and damage scattered over
    store, P and Q: a second look at everything at once, with several dirty words in one entry and in one bitmap word."""
    full = LM.store_bytes_of(G)
    host, dev, (p, q) = stores(G, full)
    rng = np.random.default_rng(G)
    entries, at = [], 3
    while at < full:
        n = int(min(rng.choice([1, 2, 15, 16, 17, 100, 700, 4096, 65535, 65536]) if rng.random() < 0.03 else rng.integers(1, 300), full - at))
        entries.append(LM.entry(at, n) if rng.random() < 0.95 else (0, 0, 0))
        at += n + int(rng.integers(0, 3))
    assert len(entries) > 2 * 256, "more than two workgroups of lanes"
    damage = [("s", int(a), int(x)) for a, x in zip(rng.integers(0, full, 40), rng.integers(1, 256, 40))]
    damage += [("s", damage[0][1] + 1, 9), ("s", damage[0][1] + 17, 9), ("s", (damage[1][1] + S) % (G * S), 77)]   # neighbours; one cell twice
    damage += [("p", int(a), 1) for a in rng.integers(0, len(p), 5)] + [("q", int(a), 1) for a in rng.integers(0, len(p), 5)]
    s, dp, dq = LM.damaged(host, p, q if dual else None, damage)
    directory = LM.records(entries)
    want_result, want = LM.locate(s, full, directory, full, S, G, dp, dq)
    assert want_result[4] and (want_result[3] or not dual) and 0 < want_result[5] < len(entries)
    torn = _dev_bytes(s)
    result, suspect = locate(cw, torn, full, directory, 7, full, G, dp, dq)
    print(f"G {G} dual {dual}: result {result}")
    assert result == want_result and suspect.tolist() == want.tolist()


@pytest.mark.parametrize("G,dual", [(2, False), (2, True), (16, True)])
def test_a_cursor_above_the_store_is_refused(cw, stores, G, dual):
    full = LM.store_bytes_of(G)
    host, dev, (p, q) = stores(G, full)
    directory = LM.records([LM.entry(100, 400), (0, 0, 0)])
    for covered in (full + 1, 1 << 40):
        result, suspect = locate(cw, dev, full, directory, 0, covered, G, p, q if dual else None)
        assert result == [1, 0, 0, 0, 0, 0, 0, 0] == LM.locate(host, full, directory, covered, S, G, p, q if dual else None)[0]
        assert suspect is None
    # an empty store: every entry that is not all zero is unjudged
    empty = _dev_bytes(np.zeros(16, np.uint8))
    result, suspect = locate(cw, empty, 0, directory, 0, 0, G, np.zeros(0, np.uint8), np.zeros(0, np.uint8) if dual else None)
    assert result == [0, 0, 0, 0, 0, 0, 1, 0] and suspect.tolist() == [4, 0]


@pytest.mark.parametrize("dual", [False, True])
def test_past_4g(cw, dual):
    """A zeroed store of 2^32 + 4 MiB bytes whose cursor lies above 2^32, G = 16: entries and damage on both sides
    of 2^32 and an entry over it.  Every byte and guard byte outside the damage is zero, so the model, evaluated on the four groups
    around 2^32 and below the cursor with every position moved down by whole groups, counts what the call counts over the whole store."""
    import torch
    G, B, MIB = 16, past4g.B, past4g.MIB
    W = G * S
    store_bytes, covered = B + 4 * MIB, B + 2 * MIB + 12345
    lo, groups = B - 2 * W, 5                                                        # the window: groups B / W - 2 .. B / W + 2
    entries = [LM.entry(B - 700, 1500), LM.entry(B - 5 * S + 100, 400), LM.entry(B + 2 * S + 50, 300), LM.entry(B + W + S + 7, 100),
               LM.entry(B - W - 30, 31), LM.entry(covered - 5, 10), (0, 0, 0), LM.entry(B - 65536, 65536), LM.entry(B, 65536)]
    damage = [(B - 10, 0x5C), (B + 10, 3), (B - 5 * S + 200, 1), (B + 2 * S + 100, 0x80), (B + W + S + 7, 7), (B - W - 1, 0xFF),
              (B + 3 * S + 5000, 5), (B - 1, 0x11), (B + 65535, 0x22)]               # (B + 3 S + 5000: a byte no entry names)
    starts, ends = [e[0] for e in entries if e[1]], [e[0] + e[1] for e in entries if e[1]]
    past4g.assert_reaches(starts, ends, "the entries")
    past4g.assert_reaches([a for a, _ in damage], [a + 1 for a, _ in damage], "the damage", over=False)
    size = GM.guard_bytes(store_bytes, S, G)
    store = torch.zeros(store_bytes, dtype=torch.uint8, device="cuda")
    d_p = torch.zeros(size, dtype=torch.uint8, device="cuda")
    d_q = torch.zeros(size, dtype=torch.uint8, device="cuda") if dual else None
    for at, x in damage:
        store[at] = x
    d_p[(B // W + 1) * S + 9000] = 1                                                     # a changed P byte no entry is under
    _sync()
    directory = LM.records(entries)
    result, suspect = locate(cw, store, store_bytes, directory, DIR_BASE, covered, G, size, None, d_p.data_ptr(), d_q.data_ptr() if dual else None)
    # the model on the window
    shifted = LM.records([(e[0] - lo, e[1], e[2]) if e[1] else e for e in entries])
    win = store[lo:lo + groups * W].cpu().numpy()
    g0 = lo // W * S
    wp = d_p[g0:g0 + groups * S].cpu().numpy()
    wq = d_q[g0:g0 + groups * S].cpu().numpy() if dual else None
    want_result, want = LM.locate(win, store_bytes - lo, shifted, covered - lo, S, G, wp, wq)
    want_result[1] += lo // W
    print(f"dual {dual}: result {result} suspect {suspect.tolist()}")
    assert result == want_result and suspect.tolist() == want.tolist()
    assert result[1] == -(-covered // W) and result[2] == len(damage) + 1 and (want != 0).sum() >= 7
    if dual:
        assert result[3] == len(damage) and suspect.tolist() == [1, 1, 1, 1, 1, 4, 0, 1, 1]


# ---- whole stores -------------------------------------------------------------------------------------------------------------------------
def _store(cw, index, alg, parity, G):
    data = text()
    streams = [data[:450000], data[380000:900000], data[900000:1300000]]
    cs = cw.ChunkStore(index, alg, cw.CdcParams(normal_size=1024), 2 << 20, 2000, DIR_BASE)
    cs.protect(stripe=S, group=G, parity=parity)
    recs = [cs.ingest(s) for s in streams]
    return cs, streams, recs


def _victims(d, G, count, apart):
    """`count` stored chunks, spread over the store, and the position of one byte in each.  With ``apart`` no two of the bytes share a
    guard cell; without it the first two bytes do, in different members, and the rest keep apart."""
    full = [i for i in range(len(d)) if d[i]["stored"]]
    picks, at, cells = [], [], np.zeros(0, np.int64)
    for i in full[3::max(1, len(full) // (count + 1))]:
        pos, stored = int(d[i]["pos"]), int(d[i]["stored"])
        mine = GM.cells(np.arange(pos, pos + stored), S, G)
        if len(np.intersect1d(mine, cells)):                     # (no two picked extents meet in a cell: a parity-1 store rebuilds them all)
            continue
        picks.append(i), at.append(pos + stored // 2)
        cells = np.concatenate([cells, mine])
        if len(picks) == count:
            break
    if not apart:
        # a second chunk with a byte in the first one's cell: the same group and column, the next stripe
        p = at[0] + S if (at[0] // S) % G + 1 < G else at[0] - S
        i = next(j for j in full if int(d[j]["pos"]) <= p < int(d[j]["pos"]) + int(d[j]["stored"]))
        assert i not in picks and GM.cells(p, S, G) == GM.cells(at[0], S, G)
        picks.append(i), at.append(p)
    assert len(picks) >= count
    return picks, at


@pytest.mark.parametrize("alg", ["lz4", "lzf"])
@pytest.mark.parametrize("parity", [1, 2])
def test_heal_whole_store(cw, alg, parity):
    G = 4
    index = cw.DedupeIndex("skein", 8192)
    try:
        cs, streams, recs = _store(cw, index, alg, parity, G)
        used, d = cs.used(), directory_of(cs)
        assert used > 2 * G * S, "more than two groups"
        # a clean store heals to nothing, and no scrub window runs
        clean = cs.guard_locate()
        assert not clean.status.any() and clean.totals == dict(groups=-(-used // (G * S)), dirty_cells=0, located_cells=0, ambiguous_cells=0,
                                                               suspects=0, unprotected=0)
        assert cs.heal() == dict(repaired=[], collided=[], unprotected=[], failed=[], no_digest=[], suspects=[], located=[], ambiguous=[],
                                 cleared=[], windows=0, groups_left=0)
        before = cs.d_store.cpu().numpy().copy()
        picks, at = _victims(d, G, 6, apart=True)
        # the condition on the input: no two changed bytes share a guard cell (asserted from the directory, on the CPU)
        assert len({int(GM.cells(p, S, G)) for p in at}) == len(at)
        assert all(int(d[i]["pos"]) <= p < int(d[i]["pos"]) + int(d[i]["stored"]) for i, p in zip(picks, at))
        for p in at:
            cs.d_store[p] ^= 0x5C
        _sync()
        victims = sorted(DIR_BASE + i for i in picks)
        full_scrub = cs.scrub()
        assert full_scrub.damaged.tolist() == victims
        found = cs.guard_locate()
        model = LM.locate(cs.d_store.cpu().numpy(), cs.store_bytes, d, used, S, G, cs.d_guard.cpu().numpy(),
                          cs.d_guard_q.cpu().numpy() if parity == 2 else None)
        assert (found.status == model[1]).all() and [found.totals[k] for k in ("groups", "dirty_cells", "located_cells", "ambiguous_cells",
                                                                                "suspects", "unprotected")] == model[0][1:7]
        assert set(found.suspects.tolist()) >= set(victims)
        # the targeted scrub judges the selected entries as the full one did, and leaves the rest unselected
        targeted = cs.scrub(values=found)
        sel = found.suspects.astype(np.int64) - DIR_BASE
        assert (targeted.status[sel] == full_scrub.status[sel]).all() and targeted.damaged.tolist() == victims
        assert targeted.stats["checked"] == len(sel) and (np.delete(targeted.status, sel) == 5).all()
        assert cs.scrub(values=victims).damaged.tolist() == victims and cs.scrub(values=[]).stats["checked"] == 0
        with pytest.raises(ValueError):
            cs.scrub(keep=recs, values=victims)
        for outside in (DIR_BASE - 1, DIR_BASE + cs.dir_entries):
            with pytest.raises(cw.CwError) as e:
                cs.scrub(values=[victims[0], outside])
            assert e.value.code == -2
        out = cs.heal()
        print(f"{alg} parity {parity}: {len(out['suspects'])} suspects, {len(out['cleared'])} cleared, {out['windows']} windows")
        assert set(out["suspects"]) >= set(victims) and out["repaired"] == victims
        assert out["collided"] == out["unprotected"] == out["failed"] == out["no_digest"] == [] and out["groups_left"] == 0
        assert sorted(out["cleared"]) == sorted(set(out["suspects"]) - set(victims)) and out["windows"] >= 1
        if parity == 2:
            assert out["suspects"] == victims == out["located"] and out["cleared"] == [] and out["ambiguous"] == []
        else:
            assert out["located"] == [] and out["ambiguous"] == out["suspects"]
        assert (cs.d_store.cpu().numpy() == before).all() and cs.guard_check() == (0, [])
        for r, s in zip(recs, streams):
            assert cs.restore(r, verify=True) == s
        assert cs.heal()["suspects"] == []
    finally:
        index.close()


def test_heal_two_bytes_in_one_cell(cw):
    """Parity 2, two damaged chunks that meet in a guard cell: the cell is ambiguous or aliases, the scrub of the suspects and a second
    heal decide.  Damage in the guard itself and in a byte no entry names stays, and shows in groups_left."""
    G = 4
    index = cw.DedupeIndex("skein", 8192)
    try:
        cs, streams, recs = _store(cw, index, "lz4", 2, G)
        used, d = cs.used(), directory_of(cs)
        before = cs.d_store.cpu().numpy().copy()
        picks, at = _victims(d, G, 3, apart=False)
        for p in at:
            cs.d_store[p] ^= 0x5C                                    # equal deltas: P' == 0 in the shared cell
        _sync()
        victims = sorted(DIR_BASE + i for i in picks)
        assert cs.scrub().damaged.tolist() == victims
        out = cs.heal()
        assert set(out["suspects"]) >= set(victims) and out["repaired"] == victims and out["groups_left"] == 0
        assert set(out["ambiguous"]) >= {DIR_BASE + picks[0], DIR_BASE + picks[-1]} and cs.last_repair["paired"] >= 2
        assert (cs.d_store.cpu().numpy() == before).all()
        # a guard byte of its own: a suspect or more, all cleared, nothing written, one group left
        p = at[1]
        cs.d_guard_q[int(GM.cells(p, S, G))] ^= 1
        _sync()
        out = cs.heal()
        assert DIR_BASE + picks[1] in out["suspects"] and out["cleared"] == out["suspects"] == out["ambiguous"] and out["repaired"] == []
        assert out["groups_left"] == 1 and cs.guard_check(detail=True) == (1, [p // (G * S)], [2])
        assert (cs.d_store.cpu().numpy() == before).all()
        cs.d_guard_q[int(GM.cells(p, S, G))] ^= 1
        _sync()
        assert cs.heal()["groups_left"] == 0
        for r, s in zip(recs, streams):
            assert cs.restore(r, verify=True) == s
    finally:
        index.close()


def test_an_unprotected_store_has_no_guard_to_read(cw):
    index = cw.DedupeIndex("skein", 1024)
    try:
        cs = cw.ChunkStore(index, "lz4", cw.CdcParams(normal_size=1024), 1 << 20, 600, DIR_BASE)
        cs.ingest(text()[:100000])
        for call in (cs.guard_locate, cs.heal):
            with pytest.raises(cw.CwError) as e:
                call()
            assert e.value.code == -4
        assert cs.scrub(values=[DIR_BASE]).stats["checked"] == 1
    finally:
        index.close()
