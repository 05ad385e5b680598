"""Editing a stored stream in place on the GPU: cw_dev_cdc_resync against a three-line numpy model on built cut lists, and
cw.ChunkStore.patch / write / append / truncate / patch_many against the ingest of the whole edited stream into a clone of the store
(``save`` / ``load``) and against tests/patch_model.py.

Device buffers of the direct calls carry canaries: guard words behind every input would match if they were read, outputs are
prefilled, have guard words behind them and are compared whole."""
import threading

import numpy as np
import pytest

import cdc_model as CM
import patch_model as PM
from conftest import corpus_file

pytestmark = pytest.mark.gpu
M = 1 << 64
POISON = 0xA5A5A5A5A5A5A5A5
G = 4                   # guard words behind every buffer
ALGS = ["lz4", "lzf"]
P256 = CM.default_params(256)       # 64 / 256 / 2048


@pytest.fixture(scope="module")
def cw():
    import torch  # noqa: F401  (one HIP runtime for torch and libcwhc.so)
    import compute_war_amd as cw
    cw.init(0)
    yield cw
    cw.tune_reset()


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _dev_u64(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.uint64).view(np.int64).copy()).cuda()


def _host_u64(t):
    return t.cpu().numpy().view(np.uint64)


# ---- 1. cw_dev_cdc_resync on built cut lists -----------------------------------------------------------------------------------------
def resync_model(new, n, old, o, new_from, shift, keep_all, count):
    """(result[4], *d_new_count afterwards) for N = n, O = o and a count word that held ``count``."""
    with np.errstate(over="ignore"):
        hit = np.flatnonzero((new[1:n + 1] >= np.uint64(new_from)) & np.isin(new[1:n + 1] + np.uint64(shift), old[:o + 1]))
        if len(hit) == 0:
            return [1, 0, 0, 0], count if keep_all else 0
        t = int(hit[0]) + 1
        return [0, t, int(np.searchsorted(old[:o + 1], new[t] + np.uint64(shift))), int(new[t])], t


def resync_call(cw, new, old, new_from, shift, keep_all, max_new=None, max_old=None, new_count=None, old_count=None, behind_new=0, behind_old=0):
    import torch
    new, old = np.asarray(new, np.uint64), np.asarray(old, np.uint64)
    max_new = len(new) - 1 if max_new is None else max_new
    max_old = len(old) - 1 if max_old is None else max_old
    new_count = max_new if new_count is None else new_count
    old_count = max_old if old_count is None else old_count
    d_new = _dev_u64(np.concatenate([new[:max_new + 1], np.full(G, behind_new, np.uint64)]))
    d_old = _dev_u64(np.concatenate([old[:max_old + 1], np.full(G, behind_old, np.uint64)]))
    d_nc = _dev_u64([POISON, new_count] + [POISON] * G)
    d_oc = _dev_u64([old_count] + [POISON] * G)
    d_res = _dev_u64([POISON] * (4 + G))
    torch.cuda.synchronize()
    cw.dev_cdc_resync(d_new.data_ptr(), d_nc.data_ptr() + 8, max_new, d_old.data_ptr(), d_oc.data_ptr(), max_old, new_from, shift, keep_all,
                      d_res.data_ptr(), _stream())
    torch.cuda.synchronize()
    res, nc = _host_u64(d_res), _host_u64(d_nc)
    want, want_count = resync_model(new, min(new_count, max_new), old, min(old_count, max_old), new_from % M, shift % M, keep_all, new_count)
    assert res[:4].tolist() == want, (res[:4].tolist(), want, max_new, max_old, new_from, keep_all)
    assert (res[4:] == POISON).all() and nc[0] == POISON and (nc[2:] == POISON).all(), "guards around d_result / d_new_count"
    assert int(nc[1]) == want_count, (int(nc[1]), want_count)
    assert _host_u64(d_oc)[0] == old_count and (_host_u64(d_new)[:max_new + 1] == new[:max_new + 1]).all(), "an input was written"
    return want


def built_cuts(n, o, shift):
    """Old cuts 20 * s; new cuts that match none of them under ``shift`` (7 + 20 * t - shift, ascending)."""
    old = np.arange(o + 1, dtype=np.uint64) * np.uint64(20)
    new = (np.arange(n + 1, dtype=np.int64) * 20 + 7 - shift).astype(np.uint64)
    return new, old


def place(new, old, t, shift, s=None):
    """A match at new cut t with old cut s (default: the nearest, so the list stays ascending)."""
    s = min(t, len(old) - 1) if s is None else s
    new[t] = np.uint64((int(old[s]) - shift) % M)
    return s


@pytest.mark.parametrize("n", [1, 63, 64, 65, 256, 257, 1025])
def test_resync_finds_the_first_cut_that_lands_on_an_old_cut(cw, n):
    for o in (0, 1, 1000):
        shift = -3
        spots = sorted({t for t in (1, n, 63, 64, 65, 255, 256, 257) if 1 <= t <= n})
        for t in spots:                                                  # the only match, at the edges of wavefronts and workgroups
            new, old = built_cuts(n, o, shift)
            s = place(new, old, t, shift)
            assert resync_call(cw, new, old, 0, shift, False)[:3] == [0, t, s]
            assert resync_call(cw, new, old, int(new[t]), shift, True)[:3] == [0, t, s]          # new_from is inclusive
            assert resync_call(cw, new, old, int(new[t]) + 1, shift, False)[0] == 1              # a match only below new_from
        for t1, t2 in zip(spots, spots[1:]):                             # two matches: the smaller t wins
            new, old = built_cuts(n, o, shift)
            s = place(new, old, t1, shift)
            place(new, old, t2, shift)
            assert resync_call(cw, new, old, 0, shift, False)[:3] == [0, t1, s]
        new, old = built_cuts(n, o, shift)                               # a match at index 0 of the new cuts is ignored
        place(new, old, 0, shift)
        assert resync_call(cw, new, old, 0, shift, False) == [1, 0, 0, 0]
        assert resync_call(cw, new, old, 0, shift, True) == [1, 0, 0, 0]
        # no match, while the words behind both lists would match if they were read; counts far above max_*
        new, old = built_cuts(n, o, shift)
        for keep_all in (False, True):
            assert resync_call(cw, new, old, 0, shift, keep_all, new_count=1 << 40, old_count=(1 << 63) + 5, behind_new=int(old[0]) - shift,
                               behind_old=int(new[1]) + shift) == [1, 0, 0, 0]
        # counts below the lists' lengths hide what lies behind them
        if n >= 64:
            new, old = built_cuts(n, o, shift)
            s = place(new, old, n, shift)
            assert resync_call(cw, new, old, 0, shift, False, new_count=n - 1)[0] == 1
            assert resync_call(cw, new, old, 0, shift, False, new_count=n)[:3] == [0, n, s]
            if o and s == o:
                assert resync_call(cw, new, old, 0, shift, False, old_count=o - 1)[0] == 1
        # a shift that wraps: the window starts below delta (new cut + shift passes 2^64)
        new, old = built_cuts(n, o, 0)
        new += np.uint64(5000)
        t = spots[len(spots) // 2]
        s = place(new, old, t, -5000 - 13)
        assert resync_call(cw, new, old, 0, M - 5000 - 13, False)[:3] == [0, t, s]
    # no new cuts at all
    assert resync_call(cw, [0], [0, 5], 0, 0, True, max_new=0) == [1, 0, 0, 0]
    assert resync_call(cw, [0, 5], [0, 5], 0, 0, False, new_count=0) == [1, 0, 0, 0]


# ---- 2. ChunkStore.patch against the ingest of the edited stream -----------------------------------------------------------------------
def noise(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def text():
    return corpus_file("alice29.txt")


def new_store(cw, alg, normal=256, max_entries=1 << 14, store_bytes=2 << 20, dir_entries=1 << 14, dir_base=7):
    return cw.ChunkStore(cw.DedupeIndex("skein512", max_entries), alg, cw.CdcParams.default(normal), store_bytes, dir_entries, dir_base)


def stored(cs):
    return cs.d_store[:cs.used()].cpu().numpy().tobytes()


def first_seen(refs):
    """Per position, the first position with the same value: equal for two recipes iff they share values at the same pairs."""
    _, first, inverse = np.unique(refs, return_index=True, return_inverse=True)
    return first[inverse]


def model_stats(old: bytes, cuts, p, a, r, ins, lookahead):
    j, t, s, new_cuts, attempts = PM.patch(old, cuts, p, a, r, ins, lookahead)
    look = max(lookahead or 4 * p["max"], 2 * p["max"]) << (attempts - 1)
    window = PM.window_end(cuts, a + r, look) + len(ins) - r - cuts[j]
    return dict(window_bytes=window, window_chunks=t, attempts=attempts, first_position=j, resume_position=s,
                reused_positions=j + len(cuts) - 1 - s), new_cuts


def patch_and_compare(cw, cs, clone, recipe, old: bytes, a, r, ins, p=P256, lookahead=0, how=None, shared=None):
    """Patch ``cs``, ingest the edited stream into ``clone`` (which held what ``cs`` held), and compare everything.  ``shared``: the
    base below which both stores number alike (default: ``cs.base``, for a clone just made)."""
    edited = PM.edited(old, a, r, ins)
    base, count, used = cs.base, cs.index.count(), cs.used()
    assert (count, used) == (clone.index.count(), clone.used())
    new = how(cs) if how else cs.patch(recipe, a, r, ins, lookahead)
    stats = dict(cs.last_patch)
    want = clone.ingest(edited)
    want_stats, want_cuts = model_stats(old, recipe.offsets.tolist(), p, a, r, ins, lookahead)
    assert new.offsets.tolist() == want.offsets.tolist() == want_cuts, (a, r, len(ins))
    assert cs.restore(new, verify=True) == edited
    assert cs.restore(recipe) == old
    assert cs.index.count() == clone.index.count() and cs.used() == clone.used() and stored(cs) == stored(clone)
    j, t, s = stats["first_position"], stats["window_chunks"], stats["resume_position"]
    assert new.refs[:j].tolist() == recipe.refs[:j].tolist() and new.refs[j + t:].tolist() == recipe.refs[s:].tolist()
    assert first_seen(new.refs).tolist() == first_seen(want.refs).tolist()
    shared = base if shared is None else shared
    below = (new.refs < np.uint64(shared)) | (want.refs < np.uint64(shared))
    assert (new.refs[below] == want.refs[below]).all()
    assert {k: stats[k] for k in want_stats} == want_stats, (stats, want_stats)
    assert stats["new_chunks"] == cs.index.count() - count and stats["stored_bytes"] == cs.used() - used
    assert cs.base == base + t
    return new, edited


def edit_classes(old: bytes, cuts):
    """(name, offset, remove, insert, lookahead): the classes of tests/test_patch_model.py, and the ones only a store has."""
    n, k = len(old), len(cuts) - 1
    mid = cuts[k // 2]
    return [
        ("insert at 0", 0, 0, noise(300, 1), 0),
        ("append", n, 0, noise(3000, 2), 0),
        ("replace inside a chunk", mid + 5, 10, noise(10, 3), 0),
        ("insert at a cut", mid, 0, noise(1, 4), 0),
        ("remove one byte before a cut", mid - 1, 1, b"", 0),
        ("inside the first chunk", cuts[1] // 2, 1, noise(70, 5), 0),
        ("inside the last chunk", (cuts[-2] + n) // 2, 0, noise(70, 6), 0),
        ("remove to the end", mid + 9, n - mid - 9, b"", 0),
        ("truncate at a cut", mid, n - mid, b"", 0),
        ("remove everything", 0, n, b"", 0),
        ("no-op", mid + 1, 0, b"", 0),
        ("identical bytes", mid - 40, 900, old[mid - 40:mid + 860], 0),
        ("an insert longer than the lookahead", cuts[3] + 1, 2, noise(4 * 2048 + 1500, 7), 0),
        ("a removal over many chunks", cuts[2] + 3, cuts[min(k - 1, 40)] - cuts[2], noise(5, 8), 0),
        ("bytes the store holds", cuts[5], 0, old[cuts[9]:cuts[14]], 0),
        ("a small lookahead", mid + 3, 0, noise(2, 9), 1),
    ]


DATA = {"random": lambda: noise(100000, 11), "text": text, "zero": lambda: bytes(40000)}


@pytest.mark.parametrize("kind", ["random", "text", "zero"])
@pytest.mark.parametrize("alg", ALGS)
def test_patch_leaves_what_ingesting_the_edited_stream_leaves(cw, tmp_path, alg, kind):
    old = DATA[kind]()
    assert len(old) <= 256 << 10
    cuts = CM.chunk(old, P256)
    path = str(tmp_path / "store.npz")
    seen = set()
    for name, a, r, ins, lookahead in edit_classes(old, cuts):
        cs = new_store(cw, alg)
        try:
            recipe = cs.ingest(old)
            assert recipe.offsets.tolist() == cuts
            raw_share = cs.used() / len(old)
            assert raw_share > 0.99 if kind == "random" else raw_share < 0.97     # random data is stored raw, the others compressed
            cs.save(path)
            clone = cw.ChunkStore.load(path)
            try:
                used = cs.used()
                patch_and_compare(cw, cs, clone, recipe, old, a, r, ins, lookahead=lookahead)
                st = cs.last_patch
                if name in ("no-op", "identical bytes", "bytes the store holds", "truncate at a cut", "remove everything") and kind != "zero":
                    assert st["new_chunks"] == 0 and cs.used() == used, name
                seen.add("several attempts" if st["attempts"] > 1 else "one attempt")
                seen.add("grown to the end" if st["attempts"] > 1 and st["resume_position"] == len(cuts) - 1 else "resync")
            finally:
                clone.index.close()
        finally:
            cs.index.close()
    # zeros never resynchronise: a shifting edit grows the window to the end, with a small lookahead in several attempts
    assert seen >= ({"several attempts", "grown to the end"} if kind == "zero" else {"one attempt", "resync"}), seen


@pytest.mark.parametrize("alg", ALGS)
def test_patch_with_the_default_parameters(cw, tmp_path, alg):
    p = CM.default_params(8192)
    lcet = corpus_file("lcet10.txt")
    old = (lcet * ((1 << 20) // len(lcet) + 1))[:1 << 20]
    cs = new_store(cw, alg, normal=8192, store_bytes=4 << 20)
    try:
        recipe = cs.ingest(old)
        path = str(tmp_path / "store.npz")
        cs.save(path)
        clone = cw.ChunkStore.load(path)
        try:
            shared = cs.base
            new, edited = patch_and_compare(cw, cs, clone, recipe, old, 300000, 4096, noise(4096, 21), p=p)
            assert cs.last_patch["attempts"] == 1 and 0 < cs.last_patch["window_chunks"] < len(recipe.refs) // 2
            patch_and_compare(cw, cs, clone, new, edited, len(edited), 0, noise(65536, 22), p=p, shared=shared)
        finally:
            clone.index.close()
    finally:
        cs.index.close()


@pytest.mark.parametrize("alg", ALGS)
def test_patch_of_an_empty_stream(cw, tmp_path, alg):
    """K == 0: no position is uploaded, nothing is read from the store, and the window is final with c_0 as its only old cut."""
    cs = new_store(cw, alg)
    try:
        cs.ingest(noise(5000, 80))                                       # (the store holds another stream)
        path = str(tmp_path / "store.npz")
        cs.save(path)
        clone = cw.ChunkStore.load(path)
        try:
            shared, empty = cs.base, cw.Recipe([], [0])
            new, edited = patch_and_compare(cw, cs, clone, empty, b"", 0, 0, noise(700, 82))
            st = cs.last_patch
            assert (st["first_position"], st["resume_position"], st["reused_positions"], st["attempts"]) == (0, 0, 0, 1)
            assert st["window_chunks"] == len(new.refs) == 3 and st["window_bytes"] == 700 and st["new_chunks"] == 3
            before = state(cs)
            none, _ = patch_and_compare(cw, cs, clone, empty, b"", 0, 0, b"", shared=shared)   # an empty insert: an empty stream again
            assert len(none.refs) == 0 and none.offsets.tolist() == [0] and state(cs) == before
            assert cs.last_patch["window_bytes"] == 0 and cs.last_patch["attempts"] == 1
            patch_and_compare(cw, cs, clone, empty, b"", 0, 0, text()[:3000], shared=shared)
        finally:
            clone.index.close()
    finally:
        cs.index.close()


@pytest.mark.parametrize("alg", ALGS)
def test_resync_in_the_second_attempt(cw, tmp_path, alg):
    """Zeros, then random bytes, a one-byte insert at 0 and the smallest lookahead: the first window (to 4096) lies in the zeros and
    finds no resync, so the device zeroes the count and nothing is inserted; the second (to the first old cut at or behind 8192)
    is not final and resynchronises at the first cut in the random bytes."""
    old = bytes(6000) + noise(14000, 81)
    cs = new_store(cw, alg)
    try:
        recipe = cs.ingest(old)
        assert recipe.offsets[:3].tolist() == [0, 2048, 4096]
        path = str(tmp_path / "store.npz")
        cs.save(path)
        clone = cw.ChunkStore.load(path)
        try:
            patch_and_compare(cw, cs, clone, recipe, old, 0, 0, b"\x01", lookahead=1)
            st = cs.last_patch
            assert st["attempts"] == 2 and st["resume_position"] < len(recipe.refs) and st["first_position"] == 0
            assert st["window_chunks"] == 3 and st["window_bytes"] < len(old) // 2               # the second window is not final
        finally:
            clone.index.close()
    finally:
        cs.index.close()


@pytest.mark.parametrize("alg", ALGS)
def test_five_patches_in_a_row_and_patch_many(cw, tmp_path, alg):
    old = text()[:120000]
    cs = new_store(cw, alg)
    try:
        recipe = cs.ingest(old)
        path = str(tmp_path / "store.npz")
        cs.save(path)
        clone = cw.ChunkStore.load(path)
        try:
            versions, shared = [(recipe, old)], cs.base
            cur, cur_bytes = recipe, old
            for a, r, ins, how in ([
                    (50000, 4096, noise(4096, 31), lambda c, rec: c.write(rec, 50000, noise(4096, 31))),
                    (None, 0, noise(9000, 32), lambda c, rec: c.append(rec, noise(9000, 32))),
                    (70001, None, b"", lambda c, rec: c.truncate(rec, 70001)),
                    (69000, 1001, noise(3000, 33), lambda c, rec: c.write(rec, 69000, noise(3000, 33))),       # a write past the end extends
                    (10, 20000, b"", lambda c, rec: c.patch(rec, 10, 20000, b""))]):
                a = len(cur_bytes) if a is None else a
                r = len(cur_bytes) - a if r is None else r
                cur, cur_bytes = patch_and_compare(cw, cs, clone, cur, cur_bytes, a, r, ins, how=lambda c, rec=cur, how=how: how(c, rec),
                                                   shared=shared)
                versions.append((cur, cur_bytes))
            for rec, data in versions:                                   # every version still restores: they share their chunks
                assert cs.restore(rec, verify=True) == data
            # patch_many: three edits in the old stream's coordinates, applied from the highest offset down
            edits = [(100, 50, noise(700, 41)), (30000, 0, noise(10, 42)), (60000, 5000, b"")]
            base, many = cs.base, cs.patch_many(recipe, edits)
            want_bytes = old
            for a, r, ins in sorted(edits, reverse=True):
                want_bytes = PM.edited(want_bytes, a, r, ins)
                clone.ingest(want_bytes)
            assert many.offsets.tolist() == CM.chunk(want_bytes, P256) and cs.restore(many, verify=True) == want_bytes
            assert cs.index.count() == clone.index.count() and stored(cs) == stored(clone) and cs.base > base
            with pytest.raises(ValueError):
                cs.patch_many(recipe, [(100, 50, b"a"), (149, 1, b"b")])
        finally:
            clone.index.close()
    finally:
        cs.index.close()


# ---- 3. refusals change nothing ---------------------------------------------------------------------------------------------------------
def state(cs):
    dig, val = cs.index.export()
    return dig.tobytes(), val.tobytes(), cs.d_dir.cpu().numpy().tobytes(), cs.used(), cs.base, stored(cs)


@pytest.mark.parametrize("alg", ALGS)
def test_refusals_leave_everything_as_it_was(cw, alg):
    old = noise(60000, 51)
    k = len(CM.chunk(old, P256)) - 1
    # the store too small, the directory full, the index full
    for what, kw in (("store", dict(store_bytes=60000 + 100)), ("directory", dict(dir_entries=k)), ("index", dict(max_entries=k))):
        cs = new_store(cw, alg, **kw)
        try:
            recipe = cs.ingest(old)
            before = state(cs)
            with pytest.raises(cw.CwError) as e:
                cs.patch(recipe, 30000, 100, noise(5000, 52))
            assert e.value.code == -5, what
            assert state(cs) == before, what
            assert cs.restore(recipe, verify=True) == old
        finally:
            cs.index.close()
    # a window position whose directory entry was zeroed
    cs = new_store(cw, alg)
    try:
        recipe = cs.ingest(old)
        j = int(np.searchsorted(recipe.offsets, 30000, side="right")) - 1
        for hurt in (j, j + 2):                                           # in front of the edit, and behind it
            entry = cs.d_dir.view(-1, 2)[int(recipe.refs[hurt]) - cs.dir_base]
            saved = entry.clone()
            entry.zero_()
            before = state(cs)
            with pytest.raises(cw.CwError) as e:
                cs.patch(recipe, 30000 if hurt == j else int(recipe.offsets[j]), 100, noise(50, 53))
            assert e.value.code == -2 and f"position {hurt} " in str(e.value) and "status 2" in str(e.value), str(e.value)
            assert state(cs) == before
            entry.copy_(saved)
        assert cs.restore(cs.patch(recipe, 30000, 100, noise(50, 53))) == PM.edited(old, 30000, 100, noise(50, 53))
        with pytest.raises(cw.CwError) as e:                              # an edit that leaves the stream
            cs.patch(recipe, 59999, 2, b"")
        assert e.value.code == -2
    finally:
        cs.index.close()


# ---- 4. two host threads ------------------------------------------------------------------------------------------------------------------
def test_two_threads_patch_two_stores(cw):
    datas = [noise(80000, 61), text()[:80000]]
    stores = [new_store(cw, alg) for alg in ALGS]
    try:
        recipes = [cs.ingest(d) for cs, d in zip(stores, datas)]
        out, errors = [None, None], []

        def work(i):
            try:
                cw.init(0)
                rec, data = recipes[i], datas[i]
                for step in range(4):
                    a, ins = 7000 * (step + 1) + i, noise(1000 + 300 * step, 70 + 10 * i + step)
                    rec, data = stores[i].patch(rec, a, 500, ins), PM.edited(data, a, 500, ins)
                out[i] = (rec, data)
            except Exception as e:  # noqa: BLE001
                errors.append(e)

        threads = [threading.Thread(target=work, args=(i,)) for i in range(2)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        assert not errors, errors
        for cs, (rec, data), recipe, old in zip(stores, out, recipes, datas):
            assert rec.offsets.tolist() == CM.chunk(data, P256)
            assert cs.restore(rec, verify=True) == data and cs.restore(recipe) == old
    finally:
        for cs in stores:
            cs.index.close()
