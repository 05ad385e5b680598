"""Renumber and revalue on the GPU (cw_dev_store_renumber, cw_dev_dedupe_revalue, cw.ChunkStore.renumber) against the numpy model
of tests/renumber_model.py, byte for byte.

Device buffers carry canaries: every output buffer is prefilled with FILL and compared whole, the new directory has guard entries
in front and behind, the pair arrays and the result words have guards behind them.  The directory sizes are the edges of the
256-lane workgroups and of the 4,096-entry scan tile of pack_kernels.hip."""
import numpy as np
import pytest

import cdc_model as CM
import renumber_model as NM
import store_gc_model as GM
from conftest import corpus_file
from test_gpu_chunk_codec import _dev_u64, _stream, _u64
from test_gpu_dedupe_lifecycle import WIDTHS, Model as IndexModel, check_call, check_lookup

pytestmark = pytest.mark.gpu
FILL = 0xA5
POISON = 0xA5A5A5A5A5A5A5A5
G = 4                   # guard entries on each side of the new directory, guard words behind the pairs
ALGS = ["lz4", "lzf"]
P1K = CM.default_params(1024)
SIZES = [1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 8193]
M = NM.M


@pytest.fixture(scope="module")
def cw():
    import torch  # noqa: F401  (one HIP runtime for torch and libcwhc.so)
    import compute_war_amd as cw
    cw.init(0)
    yield cw
    cw.tune_reset()


def _dev(a: np.ndarray):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


# ---- 1. hand-built directories -------------------------------------------------------------------------------------------------
def hand_directory(n, seed, sparse):
    """Random entries at every index (sparse: about a third all zero, never the first or the last); entry 0 is unsound in every
    field -- a position past any store, stored == 0, reserved bits set -- and is moved as it is."""
    rng = np.random.default_rng(seed)
    d = np.zeros(n, NM.LOC)
    d["pos"], d["stored"] = rng.integers(0, 1 << 48, n), rng.integers(1, 301, n)
    d["raw"] = rng.integers(1, 65537, n) | (rng.random(n) < 0.3) * 0x80000000
    if sparse:
        gone = rng.random(n) < 0.33
        gone[[0, -1]] = False
        d[gone] = (0, 0, 0)
    d[0] = ((1 << 63) + 5, 0, 0x7FFE0000)
    return d


def patterns(n):
    """name -> (directory, live or None)"""
    full, sparse = hand_directory(n, 100 + n, False), hand_directory(n, 200 + n, True)
    live = lambda f: f(np.zeros(n, np.uint32))  # noqa: E731

    def at(idx, v=1):
        def f(a):
            a[idx] = v
            return a
        return f
    i = np.arange(n)
    return {
        "all": (full, np.ones(n, np.uint32)),
        "none": (full, np.zeros(n, np.uint32)),                          # non-zero entries with the flag clear, all of them
        "third": (sparse, live(at(slice(None, None, 3), 7))),             # any non-zero value is a flag
        "wave": (full, ((i % 128) < 64).astype(np.uint32)),              # whole wavefronts of 64, then a gap of 64
        "first": (sparse, live(at(0))),
        "last": (sparse, live(at(-1))),
        "zero_flagged": (sparse, np.ones(n, np.uint32)),                 # flags on all-zero entries keep nothing
        "null": (sparse, None),                                          # d_live == NULL: every non-zero entry
    }


def renumber_call(cw, d, dir_base, live, new_base, new_dir_base, new_dir_entries, max_pairs):
    """One cw_dev_store_renumber into poisoned buffers, compared whole with the model; returns the model's result."""
    import torch
    want, want_dir, want_from, want_to = NM.renumber(d, dir_base, live, new_base, new_dir_base, new_dir_entries, max_pairs)
    d_dir, d_live = _dev(d), None if live is None else _dev(live)
    dirbuf = torch.full(((new_dir_entries + 2 * G) * 16,), FILL, dtype=torch.uint8, device="cuda")
    frm = torch.full(((max_pairs + G) * 8,), FILL, dtype=torch.uint8, device="cuda")
    to = torch.full(((max_pairs + G) * 8,), FILL, dtype=torch.uint8, device="cuda")
    res = torch.full((5 * 8,), FILL, dtype=torch.uint8, device="cuda")
    cw.dev_store_renumber(d_dir.data_ptr(), dir_base, len(d), 0 if live is None else d_live.data_ptr(), new_base,
                          dirbuf.data_ptr() + 16 * G if new_dir_entries else 0, new_dir_base, new_dir_entries,
                          frm.data_ptr() if max_pairs else 0, to.data_ptr() if max_pairs else 0, max_pairs, res.data_ptr(), _stream())
    torch.cuda.synchronize()
    got = res.cpu().numpy().view(np.uint64)
    assert got[:4].tolist() == want and got[4] == POISON, (got.tolist(), want)
    assert d_dir.cpu().numpy().tobytes() == d.tobytes(), "d_dir was written"
    nd, f, t = dirbuf.cpu().numpy(), frm.cpu().numpy().view(np.uint64), to.cpu().numpy().view(np.uint64)
    assert (nd[:16 * G] == FILL).all() and (nd[len(nd) - 16 * G:] == FILL).all(), "directory guards"
    K = want[1]
    if want[0] == 0:
        body = nd[16 * G:len(nd) - 16 * G].view(NM.LOC)
        bad = np.nonzero(body != want_dir)[0]
        assert len(bad) == 0, ("entry", int(bad[0]), body[bad[0]], want_dir[bad[0]], len(bad))
        assert np.array_equal(f[:K], want_from) and np.array_equal(t[:K], want_to)
        assert (f[K:] == POISON).all() and (t[K:] == POISON).all(), "words behind the pairs were written"
    else:
        assert (nd == FILL).all() and (f == POISON).all() and (t == POISON).all(), "a refused renumbering wrote an output buffer"
    return want


@pytest.mark.parametrize("n", SIZES)
def test_hand_built_directories(cw, n):
    seen = set()
    for name, (d, live) in patterns(n).items():
        K = NM.renumber(d, 0, live, 0, 0, n, n)[0][1]
        seen.add(K)
        # room to spare on every side: new_dir_base != new_base, pairs and entries behind the last one
        want = renumber_call(cw, d, 5, live, 1002, 1000, K + 5, K + 2)
        assert want == [0, K, 1002 + K, int(NM.nonzero(d).sum()) - K], name
        # exactly enough of everything, the new values inside the old range
        assert renumber_call(cw, d, 5, live, 5 + n // 2, 5 + n // 2, max(K, 1), K)[0] == 0, name
    assert {0, 1, n} <= seen


def test_more_entries_than_lanes(cw):
    """The kernels' grids stop at 2,048 workgroups of 256 lanes: behind that many entries a lane takes a second one."""
    n = 2048 * 256 + 257
    p = patterns(n)
    for name in ("third", "null"):
        d, live = p[name]
        K = NM.renumber(d, 0, live, 0, 0, n, n)[0][1]
        assert K > n // 5 and renumber_call(cw, d, 1 << 40, live, 9, 7, K + 3, K)[0] == 0, name
    assert renumber_call(cw, d, 1 << 40, live, 9, 7, K + 3, K - 1)[0] == 1             # refused: every buffer keeps its poison
    assert renumber_call(cw, d, 1 << 40, live, 9, 7, K + 1, K)[0] == 2


@pytest.mark.parametrize("n", SIZES)
def test_verdicts_and_all_or_nothing(cw, n):
    p = patterns(n)
    d, live = p["third"]
    K = NM.renumber(d, 0, live, 0, 0, n, n)[0][1]
    assert K >= 1
    v = lambda *a: renumber_call(cw, d, 5, live, *a)[0]  # noqa: E731  (new_base, new_dir_base, new_dir_entries, max_pairs)
    assert v(40, 40, K, K - 1) == 1                                  # K - 1 == 0: with NULL d_from / d_to
    assert v(40, 40, K, K) == 0
    assert v(40, 40, 0, 0) == 2                                      # the dry run reports K; K entries are not inside no directory
    assert v(40, 40, K - 1, K) == 2                                  # one entry too small
    assert v(41, 40, K, K) == 2                                      # ... at the other end
    assert v(39, 40, K + 1, K) == 2                                  # new_base below new_dir_base
    assert v(M - K, M - K - 1, K, K) == 2                            # new_base + K wraps
    assert v(M - K - 1, M - K - 1, K, K) == 0                        # the last values there are
    assert v(40, 40, K - 1, K - 1) == 2                              # both: 2 wins
    d0, live0 = p["none"]
    assert renumber_call(cw, d0, 5, live0, 40, 40, 0, 0) == [0, 0, 40, n]      # nothing kept: the dry run's verdict is 0
    assert renumber_call(cw, d0, 5, live0, 39, 40, 3, 0) == [0, 0, 39, n]      # ... an empty range is inside; the directory is zeroed
    zero = np.zeros(n, NM.LOC)
    assert renumber_call(cw, zero, 0, None, 0, 0, 2, 2) == [0, 0, 0, 0]


# ---- 2. revalue ----------------------------------------------------------------------------------------------------------------
def revalue_call(idx, frm, to, npairs, max_pairs, range_base, range_entries):
    """One cw_dev_dedupe_revalue; the pair arrays hold max_pairs words and a guard that sorts behind every value."""
    import torch
    d_from, d_to = _dev_u64(list(frm[:max_pairs]) + [M - 1]), _dev_u64(list(to[:max_pairs]) + [POISON])
    d_np, res = _dev_u64([npairs]), _dev_u64([POISON] * 4)
    idx.dev_revalue(d_from.data_ptr(), d_to.data_ptr(), d_np.data_ptr(), max_pairs, range_base, range_entries, res.data_ptr(), _stream())
    torch.cuda.synchronize()
    got = _u64(res)
    assert got[3] == POISON
    return got[:3].tolist()


def check_revalue(idx, model, digests, frm, to, npairs, max_pairs, range_base, range_entries):
    keys = list(model.table)
    want, after = NM.revalue([model.table[k] for k in keys], frm, to, npairs, max_pairs, range_base, range_entries)
    n = idx.count()
    assert revalue_call(idx, frm, to, npairs, max_pairs, range_base, range_entries) == want
    model.table = dict(zip(keys, after))
    check_lookup(idx, model, digests)
    assert idx.count() == n == len(keys)
    return want


@pytest.mark.parametrize("max_entries", [1, 100, 5000])
@pytest.mark.parametrize("alg,db", WIDTHS)
def test_revalue(cw, alg, db, max_entries):
    rng = np.random.default_rng(db + max_entries)
    n, base = max_entries, 1000                                         # a full index: count == max_entries
    R = 3 * n + 10
    digests = rng.integers(0, 256, (n, db), dtype=np.uint8)
    values = np.array([base + 3 * (i // 2) if i % 2 == 0 else 10 ** 12 + i for i in range(n)], np.uint64)
    if n >= 4:
        values[2] = values[0]                                            # two entries share one value
    with cw.DedupeIndex(alg, max_entries) as idx:
        model = IndexModel()
        check_call(idx, model, digests, values=values)
        assert idx.count() == max_entries
        inside = sorted(set(int(v) for v in values if base <= v < base + R))
        outside = sorted(set(int(v) for v in values) - set(inside))
        n_inside = sum(base <= int(v) < base + R for v in values)
        # a value of the range that no pair names: verdict 1, and the table's bytes are as they were
        before = idx.export()
        want = check_revalue(idx, model, digests, inside[1:], [7 * 10 ** 11 + k for k in range(len(inside) - 1)], len(inside) - 1,
                             len(inside) - 1, base, R)
        assert want == [1, n_inside - (2 if n >= 4 else 1), 2 if n >= 4 else 1]
        after = idx.export()
        assert before[0].tobytes() == after[0].tobytes() and before[1].tobytes() == after[1].tobytes()
        # p == 0: counts only
        assert check_revalue(idx, model, digests, inside, inside, 0, len(inside), base, R) == [1, 0, n_inside]
        assert check_revalue(idx, model, digests, inside, inside, len(inside), 0, base, 0) == [0, 0, 0]
        # *d_npairs above max_pairs is clamped; no range: the values no pair names stay, nothing is stale
        half = len(outside) // 2
        want = check_revalue(idx, model, digests, outside, [2 * 10 ** 12 + k for k in range(len(outside))], 10 ** 9, half, 0, 0)
        assert want == [0, half, 0]
        # dense renumbering downward: old and new values overlap (base + 3 is the new value of one entry and the old one of another),
        # each entry is translated exactly once, both entries of the shared value are, the values outside the range stay
        want = check_revalue(idx, model, digests, inside, [base + k for k in range(len(inside))], len(inside), len(inside), base, R)
        assert want == [0, n_inside, 0]
        assert sorted(set(v for v in model.table.values() if v < 10 ** 11)) == [base + k for k in range(len(inside))]
        assert sum(v >= 10 ** 12 for v in model.table.values()) == n - n_inside


# ---- 3. end to end through cw.ChunkStore -----------------------------------------------------------------------------------------
def _index_bytes(idx):
    dig, val = idx.export()
    return dig.tobytes(), val.tobytes()


def _three(cw, alg, dir_entries=512, dir_base=40):
    a, b, c = GM.three_streams(corpus_file("alice29.txt"), corpus_file("kennedy.xls"))
    idx = cw.DedupeIndex("skein512", 2048)
    cs = cw.ChunkStore(idx, alg, cw.CdcParams.default(1024), 1 << 20, dir_entries, dir_base=dir_base)
    return cs, (a, b, c), tuple(cs.ingest(x) for x in (a, b, c))


@pytest.mark.parametrize("alg", ALGS)
def test_renumber_after_compact(cw, alg, tmp_path):
    cs, (a, b, c), (ra, rb, rc) = _three(cw, alg)
    with cs.index as idx:
        assert cs.base == 40 + len(ra.refs) + len(rb.refs) + len(rc.refs)
        got = cs.compact([ra, rc])
        K = got["kept"]
        assert got["dropped"] > 0 and idx.count() == K < cs.base - 40
        used = cs.used()
        na, nc = cs.renumber([ra, rc], dir_entries=K)                  # exactly K entries
        assert (cs.dir_entries, cs.dir_base, cs.base, cs.used(), idx.count()) == (K, 40, 40 + K, used, K)
        assert np.array_equal(na.offsets, ra.offsets) and np.array_equal(nc.offsets, rc.offsets)
        both = np.concatenate([na.refs, nc.refs])
        assert sorted(set(both.tolist())) == list(range(40, 40 + K)) and not np.array_equal(nc.refs, rc.refs)
        # the order of first occurrence is the order of the values, as it was before
        old = np.concatenate([ra.refs, rc.refs])
        assert np.array_equal(np.argsort(old, kind="stable"), np.argsort(both, kind="stable"))
        assert cs.restore(na, verify=True) == a and cs.restore(nc, verify=True) == c
        assert cs.read_ranges(nc, [(0, 10), (89990, 300), (len(c) - 7, 7)]) == [c[:10], c[89990:90290], c[-7:]]
        report = cs.scrub()
        assert report.clean and len(report.orphans) == 0 and report.stats["checked"] == report.stats["ok"] == K
        with pytest.raises(cw.CwError):
            cs.restore(rc)                                                # the old recipes are stale
        # again, into a larger directory at another base: ingestion goes on from base = dir_base + K
        na, nc = cs.renumber([na, nc], dir_entries=K + 300, dir_base=7)
        assert (cs.dir_entries, cs.dir_base, cs.base, idx.count()) == (K + 300, 7, 7 + K, K)
        assert cs.restore(na, verify=True) == a and cs.restore(nc, verify=True) == c
        nb = cs.ingest_stream(b)
        fresh = sorted(set(nb.refs.tolist()) - set(na.refs.tolist()) - set(nc.refs.tolist()))
        assert fresh and fresh[0] >= 7 + K and cs.base == 7 + K + len(nb.refs) and idx.count() == K + len(fresh) == K + got["dropped"]
        assert cs.restore(nb, verify=True) == b and cs.scrub().clean
        # a renumbered store replicates, and saves and loads
        with cw.DedupeIndex("skein512", 2048) as idx2:
            peer = cw.ChunkStore(idx2, alg, cw.CdcParams.default(1024), 1 << 20, 512)
            pa, pb = cs.replicate_to(peer, [na, nb])
            assert peer.restore(pa, verify=True) == a and peer.restore(pb, verify=True) == b
        path = str(tmp_path / "store.npz")
        cs.save(path)
        base = cs.base
    cs2 = cw.ChunkStore.load(path)
    try:
        assert (cs2.dir_entries, cs2.dir_base, cs2.base) == (K + 300, 7, base)
        assert cs2.restore(na, verify=True) == a and cs2.restore(nb, verify=True) == b and cs2.restore(nc, verify=True) == c
    finally:
        cs2.index.close()


@pytest.mark.parametrize("alg", ALGS)
def test_a_refused_renumber_changes_nothing(cw, alg):
    import torch
    cs, (a, b, c), (ra, rb, rc) = _three(cw, alg)
    with cs.index as idx:
        # the directory forgets the second stream and the index does not: mark and compact without the index's retain, which is
        # what cw.ChunkStore.compact does behind them.  The index then holds values of the directory that no entry carries.
        n, s = cs.dir_entries, _stream()
        live, n_out = torch.zeros(n, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda")
        new_store, new_used = torch.zeros(cs.store_bytes, dtype=torch.uint8, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda")
        new_dir, result = torch.zeros(n * 2, dtype=torch.int64, device="cuda"), torch.zeros(4, dtype=torch.int64, device="cuda")
        marks = [(_dev_u64(r.refs), _dev_u64([len(r.refs)]), len(r.refs)) for r in (ra, rc)]       # (kept alive until the calls have run)
        for d_ref, d_count, k in marks:
            cw.dev_store_mark(d_ref.data_ptr(), d_count.data_ptr(), k, cs.dir_base, n, live.data_ptr(), n_out.data_ptr(), s)
        cw.dev_store_compact(cs.d_store.data_ptr(), cs.store_bytes, cs.d_dir.data_ptr(), n, live.data_ptr(), new_store.data_ptr(), cs.store_bytes,
                             new_used.data_ptr(), new_dir.data_ptr(), result.data_ptr(), s)
        torch.cuda.synchronize()
        verdict, _, kept, dropped = _u64(result).tolist()
        assert verdict == 0 and dropped > 0 and int(n_out.item()) == 0
        cs.d_store, cs.d_used, cs.d_dir = new_store, new_used, new_dir
        state = (cs.d_dir.data_ptr(), cs.dir_entries, cs.dir_base, cs.base, cs.used())
        index = _index_bytes(idx)

        def unchanged():
            assert (cs.d_dir.data_ptr(), cs.dir_entries, cs.dir_base, cs.base, cs.used()) == state and _index_bytes(idx) == index
            assert cs.restore(ra) == a and cs.restore(rc) == c

        with pytest.raises(cw.CwError) as e:
            cs.renumber([ra, rc])
        assert "compact first" in str(e.value) and e.value.code == -2 and e.value.stale == dropped, str(e.value)
        unchanged()
        # compact first: now the index forgets too
        assert cs.compact([ra, rc])["removed"] == dropped
        state = (cs.d_dir.data_ptr(), cs.dir_entries, cs.dir_base, cs.base, cs.used())
        index = _index_bytes(idx)
        with pytest.raises(cw.CwError) as e:
            cs.renumber([ra, rb, rc])                                     # a recipe that names dropped chunks
        assert e.value.code == -2 and not hasattr(e.value, "stale")
        unchanged()
        with pytest.raises(cw.CwError) as e:
            cs.renumber([ra, rc], dir_entries=kept - 1)
        assert e.value.code == -5 and e.value.needed == kept
        unchanged()
        na, nc = cs.renumber([ra, rc], dir_entries=kept)
        assert cs.restore(na, verify=True) == a and cs.restore(nc, verify=True) == c and ra.refs[0] == 40 == na.refs[0]


# ---- 4. the rotation: what the feature is for ------------------------------------------------------------------------------------
def _generations(count=6):
    """Backups of one file: the text with 24 KiB of each generation's own in the middle; about four chunks in five are shared."""
    text = corpus_file("alice29.txt")[:120000]
    return [text[:50000] + np.random.default_rng(900 + g).bytes(24576) + text[50000:] for g in range(count)]


def test_rotation_needs_renumber(cw):
    gens = _generations()
    cuts = [CM.chunk(g, P1K) for g in gens]
    k = [len(c) - 1 for c in cuts]
    distinct = [len({g[c[i]:c[i + 1]] for i in range(len(c) - 1)}) for g, c in zip(gens, cuts)]
    D = max(k[i] + k[i + 1] for i in range(len(k) - 1))
    # preconditions, from the CPU model's chunk counts: two generations fit the directory, a third does not, and the kept
    # generation's distinct chunks plus a new generation do
    assert all(k[i] + k[i + 1] <= D for i in range(len(k) - 1)) and k[0] + k[1] + k[2] > D
    assert all(distinct[i] + k[i + 1] <= D for i in range(len(k) - 1)) and min(k) > 100

    # without renumber: the one before last is dropped, the third generation still does not fit, and the store is as it was
    with cw.DedupeIndex("skein512", 2048) as idx:
        cs = cw.ChunkStore(idx, "lz4", cw.CdcParams.default(1024), 1 << 20, D)
        r0, r1 = cs.ingest_stream(gens[0]), cs.ingest_stream(gens[1])
        assert (len(r0.refs), len(r1.refs)) == (k[0], k[1]) and cs.base == k[0] + k[1]
        got = cs.compact([r1])
        assert got["kept"] == distinct[1] and got["dropped"] > 0
        state = (cs.base, cs.used(), idx.count(), _index_bytes(idx), cs.d_dir.cpu().numpy().tobytes())
        with pytest.raises(cw.CwError) as e:
            cs.ingest_stream(gens[2])
        assert e.value.code == -5 and e.value.consumed == 0 and e.value.nchunks == 0
        assert (cs.base, cs.used(), idx.count(), _index_bytes(idx), cs.d_dir.cpu().numpy().tobytes()) == state
        assert cs.restore(r1, verify=True) == gens[1]

    # with compact + renumber after each drop, every generation goes through the same directory
    with cw.DedupeIndex("skein512", 2048) as idx:
        cs = cw.ChunkStore(idx, "lz4", cw.CdcParams.default(1024), 1 << 20, D)
        last = None
        for g, data in enumerate(gens):
            recipe = cs.ingest_stream(data)
            assert len(recipe.refs) == k[g] and cs.restore(recipe, verify=True) == data
            if last is not None:
                assert cs.restore(last, verify=True) == gens[g - 1]      # both kept generations restore
            assert cs.compact([recipe])["kept"] == distinct[g]           # the one before last goes
            (last,) = cs.renumber([recipe])
            assert (cs.dir_entries, cs.base, idx.count()) == (D, distinct[g], distinct[g])
            assert cs.restore(last, verify=True) == data
        assert cs.scrub().clean
