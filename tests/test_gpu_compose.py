"""Composing a stored stream from stored ranges and new bytes on the GPU: cw_dev_cdc_resync_windows and cw_dev_scatter_extents against
their models on built lists, and cw_store_compose / cw.ChunkStore.compose, apply_delta, edit and concat against tests/compose_model.py
and against the ingest of the composed bytes into a clone of the store (``save`` / ``load``).

Device buffers of the direct calls carry canaries: guard words behind every input would match if they were read, outputs are
prefilled, have guard words behind them and are compared whole."""
import ctypes

import numpy as np
import pytest

import cdc_model as CM
import compose_model as XM
import patch_model as PM
from conftest import corpus_file

pytestmark = pytest.mark.gpu
M = 1 << 64
NONE = M - 1
POISON = 0xA5A5A5A5A5A5A5A5
G = 4                   # guard words behind every buffer
ALGS = ["lz4", "lzf"]
P256 = XM.P             # 64 / 256 / 2048


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


def _dev_u8(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.uint8).copy()).cuda()


def _host_u64(t):
    return t.cpu().numpy().view(np.uint64)


def noise(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


# ---- 1. cw_dev_cdc_resync_windows on built lists ------------------------------------------------------------------------------------
SIZES = (1, 2, 64, 65, 256)     # cuts per window
OLD = 6                         # old cuts per window


def built_windows(nwin, seed):
    """New cuts 1000 * g; window w has SIZES[w % 5] cuts and the old range [OLD * w, OLD * (w + 1)), odd values that no shifted cut
    equals until ``place`` puts one in.  Scenario w % 6: 0 nothing; 1 two hits, the lower wins; 2 a hit at the last cut only, not final;
    3 the same, final; 4 a hit below new_from (and one behind it when the window has three cuts); 5 a hit that only the next window's
    old range holds."""
    rng = np.random.default_rng(seed)
    first = np.concatenate([[0], np.cumsum([SIZES[w % 5] for w in range(nwin)])]).astype(np.uint64)
    x = np.arange(int(first[-1]) + 1, dtype=np.uint64) * np.uint64(1000)
    old = (np.arange(OLD * (nwin + 1), dtype=np.uint64) * np.uint64(2) + np.uint64(1)) + np.uint64(10 ** 9)
    wins = np.zeros(nwin, dtype=[(k, "<u8") for k in ("new_from", "shift", "old_first", "old_count", "final")])
    for w in range(nwin):
        lo, n = int(first[w]), SIZES[w % 5]
        shift = (int(rng.integers(1, 1 << 20)) * 2 - (lo * 1000 if w % 2 else 0)) % M        # even, and wrapping for every other window
        wins[w] = (0, shift, OLD * w, OLD, 0)
        hits, kind = [], w % 6
        if kind == 1:
            hits = sorted({lo + max(1, n // 2), lo + max(1, n - 1)})
        elif kind in (2, 3):
            hits, wins[w]["final"] = [lo + n], kind == 3
        elif kind == 4:
            hits = [lo + 1] + ([lo + n - 1] if n >= 3 else [])
            wins[w]["new_from"] = int(x[lo + 1]) + 1
        if kind == 5:                                                                          # the neighbour's range holds it, first
            if n >= 2:
                old[OLD * (w + 1)] = np.uint64((int(x[lo + max(1, n // 2)]) + shift) % M)
            continue
        for j, g in enumerate(hits):                                                           # (even, and below every odd filler)
            old[OLD * w + OLD - len(hits) + j] = np.uint64((int(x[g]) + shift) % M)
        old[OLD * w:OLD * (w + 1)].sort()
    return x, first, wins, old


def windows_call(cw, x, first, wins, old, max_new=None, new_count=None, max_old=None):
    import torch
    nwin = len(wins)
    max_new = len(x) - 1 if max_new is None else max_new
    new_count = max_new if new_count is None else new_count
    max_old = len(old) if max_old is None else max_old
    n = min(new_count, max_new)
    # behind the new cuts: values that would land; behind the old cuts: values a new cut would land on
    behind_new = (int(old[int(wins[0]["old_first"])]) - int(wins[0]["shift"])) % M
    behind_old = (int(x[1]) + int(wins[0]["shift"])) % M
    d_x = _dev_u64(np.concatenate([x[:max_new + 1], np.full(G, behind_new, np.uint64)]))
    d_old = _dev_u64(np.concatenate([old[:max_old], np.full(G, behind_old, np.uint64)]))
    d_first = _dev_u64(np.concatenate([first, np.full(G, POISON, np.uint64)]))
    d_win = _dev_u64(np.concatenate([wins.view(np.uint64), np.full(G, POISON, np.uint64)]))
    d_nc = _dev_u64([POISON, new_count, POISON])
    d_res = _dev_u64([POISON] * (4 * nwin + G))
    torch.cuda.synchronize()
    cw.dev_cdc_resync_windows(d_x.data_ptr(), d_nc.data_ptr() + 8, max_new, d_first.data_ptr(), d_win.data_ptr(), nwin, d_old.data_ptr(), max_old,
                              d_res.data_ptr(), _stream())
    torch.cuda.synchronize()
    res = _host_u64(d_res)
    clamped = [min(int(f), n) for f in first]
    specs = []
    for w in wins:
        lo = min(int(w["old_first"]), max_old)
        specs.append((int(w["new_from"]), int(w["shift"]), lo, min(int(w["old_count"]), max_old - lo), int(w["final"])))
    want = XM.resync_windows([int(v) for v in x[:n + 1]] + [0], clamped, specs, [int(v) for v in old[:max_old]])
    got = res[:4 * nwin].reshape(nwin, 4).tolist()
    assert got == want, [(w, g, e) for w, (g, e) in enumerate(zip(got, want)) if g != e][:5]
    assert (res[4 * nwin:] == POISON).all(), "guard behind d_result"
    assert _host_u64(d_nc).tolist() == [POISON, new_count, POISON], "the count was written"
    assert (_host_u64(d_x)[:max_new + 1] == x[:max_new + 1]).all() and (_host_u64(d_first)[:nwin + 1] == first).all(), "an input was written"
    return want


@pytest.mark.parametrize("nwin", [1, 63, 64, 65, 257])
def test_resync_windows_finds_each_windows_first_landing(cw, nwin):
    x, first, wins, old = built_windows(nwin, 100 + nwin)
    want = windows_call(cw, x, first, wins, old)
    kinds = {w % 6: want[w] for w in range(nwin) if SIZES[w % 5] >= 3}
    for w, r in enumerate(want):
        lo, n, kind = int(first[w]), SIZES[w % 5], w % 6
        if kind in (0, 2, 5) or (kind == 4 and n < 3) or (kind == 1 and n == 1):     # (a window of one cut has only its last)
            assert r == [1, 0, 0, 0], (w, kind, r)
        elif kind == 1:
            assert r[:2] == [0, max(1, n // 2)] and OLD * w <= r[2] < OLD * (w + 1), (w, r)
        elif kind == 3:
            assert r[:2] == [0, n] and r[3] == int(x[lo + n]), (w, r)
        else:
            assert r[:2] == [0, n - 1], (w, r)
    assert nwin < 63 or set(kinds) == set(range(6))
    # counts: far above max_new, and below it -- the windows behind the count have no cuts, the one it falls into ends there
    windows_call(cw, x, first, wins, old, new_count=1 << 40)
    for n in {int(first[-1]) - 1, int(first[nwin // 2]) + 1, int(first[nwin // 2]), 1, 0}:
        if 0 <= n <= int(first[-1]):
            windows_call(cw, x, first, wins, old, new_count=n)
    # an old list shorter than the windows' ranges say: the ranges are clamped into it
    windows_call(cw, x, first, wins, old, max_old=max(OLD * nwin // 2, 1))
    windows_call(cw, x, first, wins, old, max_old=0)
    windows_call(cw, x, first, wins, old, max_new=0)


# ---- 2. cw_dev_scatter_extents --------------------------------------------------------------------------------------------------------
TILE = 16384


def scatter_call(cw, src: bytes, ext, dst_bytes, n=None, max_n=None):
    """One call into a canary-filled destination, compared whole with the model; returns the result words."""
    import torch
    ext = np.asarray(ext, np.uint64).reshape(-1, 3)
    max_n = len(ext) if max_n is None else max_n
    n_word = max_n if n is None else n
    d_src = _dev_u8(np.concatenate([np.frombuffer(src, np.uint8), np.full(64, 0x5A, np.uint8)]))
    d_ext = _dev_u64(np.concatenate([ext.reshape(-1), np.array([0, 0, 1] * 2, np.uint64)]))   # (behind the list: extents that would copy)
    d_n = _dev_u64([n_word, POISON])
    d_dst = _dev_u8(np.full(dst_bytes + 64, 0xA5, np.uint8))
    d_res = _dev_u64([POISON] * (4 + G))
    torch.cuda.synchronize()
    cw.dev_scatter_extents(d_src.data_ptr(), len(src), d_ext.data_ptr(), d_n.data_ptr(), max_n, d_dst.data_ptr(), dst_bytes, d_res.data_ptr(), _stream())
    torch.cuda.synchronize()
    count = min(n_word, max_n)
    want, bad, end = np.full(dst_bytes + 64, 0xA5, np.uint8), NONE, 0
    for k, (s, d, length) in enumerate(ext[:count].tolist()):
        ok = length >= 1 and s + length <= len(src) and d + length <= dst_bytes and d >= end
        if not ok:
            bad = k
            break
        end = d + length
    if bad == NONE:
        for s, d, length in ext[:count].tolist():
            want[d:d + length] = np.frombuffer(src, np.uint8)[s:s + length]
    res = _host_u64(d_res)
    assert res[:4].tolist() == [int(bad != NONE), 0 if bad != NONE else end, bad, count], res[:4].tolist()
    assert (res[4:] == POISON).all()
    assert (d_dst.cpu().numpy() == want).all(), "the destination differs from the model" if bad == NONE else "a refused call wrote"
    return res[:4].tolist()


def test_scatter_extents_copies_what_the_model_copies(cw):
    src = noise(200000, 7)
    lengths = [1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 1, 3 * TILE + 17]
    rng = np.random.default_rng(8)
    for gap in (0, 1, 5000, 3 * TILE + 5):                              # back to back, a byte apart, tiles that no extent touches
        ext, at = [], int(rng.integers(0, 40))
        for length in lengths:
            ext.append((int(rng.integers(0, len(src) - length + 1)), at, length))
            at += length + gap
        assert scatter_call(cw, src, ext, at + 100)[0] == 0
        assert scatter_call(cw, src, ext, at - gap)[0] == 0             # the last extent ends the destination
        assert scatter_call(cw, src, ext, at + 100, n=1 << 50)[3] == len(ext)       # a count far above max_n
        assert scatter_call(cw, src, ext, at + 100, n=4)[3] == 4        # ... and below: the extents behind it are not copied
    many = [(int(rng.integers(0, len(src) - 70)), 100 * k + int(rng.integers(0, 30)), int(rng.integers(1, 71))) for k in range(300)]
    assert scatter_call(cw, src, many, 100 * 300 + 100)[0] == 0          # more extents than a wavefront takes at once, several per tile
    assert scatter_call(cw, src, [(len(src) - 1, 0, 1)], 1) == [0, 1, NONE, 1]
    assert scatter_call(cw, src, [], 100, max_n=0) == [0, 0, NONE, 0]


def test_scatter_extents_refuses_every_kind_of_bad_extent(cw):
    src = noise(50000, 9)
    good = [(100, 10, 500), (0, 600, 70), (7, 20000, 1), (40000, 20001, 10000)]
    bads = [(5, 700, 0),                       # empty
            (49999, 700, 2), (50001, 700, 1),  # leaves the source
            (M - 5, 700, 10), (5, 700, M - 2),  # wraps
            (5, 39990, 11), (5, 40001, 1),     # leaves the destination
            (5, M - 3, 10),                    # the destination wraps
            (5, 669, 1), (5, 600, 1), (5, 0, 1)]  # overlaps or lies in front of the extent before
    for bad in bads:
        r = scatter_call(cw, src, good[:2] + [bad] + good[2:], 40000)
        assert r[0] == 1 and r[2] == 2, (bad, r)
    for bad in bads[:3]:                                                 # the first extent of the list
        r = scatter_call(cw, src, [bad] + [(s, d + 1000, n) for s, d, n in good[:3]], 40000)
        assert r[0] == 1 and r[2] == 0, (bad, r)
    # two bad extents: the lower is named
    r = scatter_call(cw, src, [good[0], (5, 700, 0), good[2], (5, 100, 1)], 40000)
    assert r[:3] == [1, 0, 1]


# ---- 3. cw_store_compose against the model and the ingest of the composed bytes -------------------------------------------------------
def new_store(cw, alg, max_entries=1 << 14, store_bytes=2 << 20, dir_entries=1 << 14, dir_base=7):
    return cw.ChunkStore(cw.DedupeIndex("skein512", max_entries), alg, cw.CdcParams.default(256), store_bytes, dir_entries, dir_base)


def stored(cs):
    return cs.d_store[:cs.used()].cpu().numpy().tobytes()


def first_seen(refs):
    _, first, inverse = np.unique(refs, return_index=True, return_inverse=True)
    return first[inverse]


def digests(cs):
    dig, _ = cs.index.export()
    return sorted(bytes(d) for d in dig)


def state(cs):
    dig, val = cs.index.export()
    return dig.tobytes(), val.tobytes(), cs.d_dir.cpu().numpy().tobytes(), cs.used(), cs.base, stored(cs)


def joined(recipes):
    starts = np.concatenate([np.zeros(1, np.uint64), np.cumsum([r.nbytes for r in recipes], dtype=np.uint64)])
    refs = np.concatenate([r.refs for r in recipes])
    offs = np.concatenate([np.zeros(1, np.uint64)] + [r.offsets[1:] + starts[i] for i, r in enumerate(recipes)])
    first = np.concatenate([np.zeros(1, np.uint64), np.cumsum([len(r.refs) for r in recipes], dtype=np.uint64)])
    return refs, offs, first


CASES = XM.cases()
MODEL = {}


def model_of(case):
    """The model's result for a case, computed once"""
    if case["name"] not in MODEL:
        MODEL[case["name"]] = XM.compose(case["a"], case["cuts"], case["first"], case["ops"], case["payload"], P256, case["lookahead"])
    return MODEL[case["name"]]


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
@pytest.mark.parametrize("alg", ALGS)
def test_named_case_leaves_what_ingesting_the_composed_bytes_leaves(cw, tmp_path, alg, case):
    want = model_of(case)
    b_bytes = want["bytes"]
    cs = new_store(cw, alg)
    try:
        recipes = [cs.ingest(s) for s in case["streams"]]
        refs, offs, first = joined(recipes)
        assert offs.tolist() == case["cuts"] and first.tolist() == case["first"]
        path = str(tmp_path / "store.npz")
        cs.save(path)
        clone = cw.ChunkStore.load(path)
        try:
            count, used, base = cs.index.count(), cs.used(), cs.base
            ops = np.array(case["ops"], dtype=cw.DELTA_OP_DTYPE) if case["ops"] else np.zeros(0, cw.DELTA_OP_DTYPE)
            out_refs, out_offs, stats = cw.store_compose(cs.index, cs.params, cs.comp_alg, cs._triple(), refs, offs, ops, case["payload"], cs.base,
                                                         case["lookahead"], first if len(recipes) > 1 else None)
            cs.base += stats["rebuilt_chunks"]
            new = cw.Recipe(out_refs, out_offs)
            assert new.offsets.tolist() == want["cuts"] == CM.chunk(b_bytes, P256)
            assert cs.restore(new, verify=True) == b_bytes
            for r, s in zip(recipes, case["streams"]):
                assert cs.restore(r) == s
            ingested = clone.ingest(b_bytes)
            assert ingested.offsets.tolist() == new.offsets.tolist()
            assert cs.used() == clone.used() and stored(cs) == stored(clone)
            assert cs.index.count() == clone.index.count() and digests(cs) == digests(clone)
            assert first_seen(new.refs).tolist() == first_seen(ingested.refs).tolist()
            for x, s in want["kept"].items():                            # a kept chunk carries A's ref
                assert int(new.refs[want["cuts"].index(x)]) == int(refs[s])
            for key in ("windows", "rounds", "merged_windows", "kept_positions", "rebuilt_chunks", "rebuilt_bytes"):
                assert stats[key] == want["stats"][key], (key, stats, want["stats"])
            assert stats["new_chunks"] == cs.index.count() - count and stats["stored_bytes"] == cs.used() - used
            assert cs.base == base + want["stats"]["rebuilt_chunks"]
        finally:
            clone.index.close()
    finally:
        cs.index.close()


@pytest.mark.parametrize("alg", ALGS)
def test_delta_edit_and_concat_inside_the_store(cw, alg):
    old = corpus_file("alice29.txt")[:120000]
    cs = new_store(cw, alg)
    try:
        recipe = cs.ingest(old)
        # a new version made by five patches, shipped as a delta and applied inside the store
        cur, cur_bytes = recipe, old
        for a, r, ins in ((50000, 4096, noise(4096, 31)), (len(old), 0, noise(9000, 32)), (70001, 3000, b""), (69000, 1001, noise(3000, 33)),
                          (10, 20000, b"")):
            cur, cur_bytes = cs.patch(cur, a, r, ins), PM.edited(cur_bytes, a, r, ins)
        delta = cs.delta(recipe, cur)
        count, used = cs.index.count(), cs.used()
        got = cs.apply_delta(recipe, delta)
        assert got.offsets.tolist() == cur.offsets.tolist() == CM.chunk(cur_bytes, P256)
        assert cs.restore(got, verify=True) == cur_bytes and got.refs.tolist() == cur.refs.tolist()
        assert (cs.index.count(), cs.used()) == (count, used) and cs.last_compose["new_chunks"] == 0    # every chunk of it was stored
        assert 0 < cs.last_compose["rebuilt_chunks"] < len(cur.refs) // 4 and cs.last_compose["kept_positions"] > len(cur.refs) // 2
        with pytest.raises(cw.CwError) as e:
            cs.apply_delta(cur, delta)                                   # made against another size
        assert e.value.code == -2
        broken = cw.Delta(delta.ops.copy(), delta.payload, delta.old_bytes, delta.new_bytes)
        broken.ops["a_off"][0] = len(old) + 5
        with pytest.raises(cw.CwError) as e:
            cs.apply_delta(recipe, broken)
        assert e.value.code == -2 and "op 0" in str(e.value)
        # edit = patch_many in one call
        edits = [(100, 50, noise(700, 41)), (30000, 0, noise(10, 42)), (60000, 5000, b""), (119000, 1000, noise(5, 43))]
        many = cs.patch_many(recipe, edits)
        base = cs.base
        once = cs.edit(recipe, edits)
        assert once.offsets.tolist() == many.offsets.tolist() and cs.restore(once, verify=True) == cs.restore(many)
        assert once.refs.tolist() == many.refs.tolist() and cs.base == base + cs.last_compose["rebuilt_chunks"]
        assert cs.last_compose["rounds"] == 1 and cs.last_compose["windows"] == 4
        with pytest.raises(ValueError):
            cs.edit(recipe, [(100, 50, b"a"), (149, 1, b"b")])
        # concat of three streams, and a server-side copy of a range
        parts = [noise(30000, 51), corpus_file("alice29.txt")[120000:140000], noise(7000, 52)]
        recipes = [cs.ingest(p) for p in parts]
        whole = cs.concat(recipes)
        assert cs.restore(whole, verify=True) == b"".join(parts) and whole.offsets.tolist() == CM.chunk(b"".join(parts), P256)
        # (stream 0 is kept from byte 0 without a window; one window across each of the two stream ends inside)
        assert cs.last_compose["windows"] == 2 and cs.last_compose["kept_positions"] > len(whole.refs) * 3 // 4
        piece = cs.compose([(recipes[0], 5000, 20000), b"--", (recipe, 0, 1000)])
        assert cs.restore(piece, verify=True) == parts[0][5000:25000] + b"--" + old[:1000]
        assert piece.offsets.tolist() == CM.chunk(parts[0][5000:25000] + b"--" + old[:1000], P256)
    finally:
        cs.index.close()


@pytest.mark.parametrize("alg", ALGS)
def test_refusals_leave_everything_as_it_was(cw, alg):
    old = noise(60000, 61)
    k = len(CM.chunk(old, P256)) - 1
    parts = lambda r: [(r, 0, 30000), noise(5000, 62), (r, 30500, 29500)]  # noqa: E731
    for what, kw in (("store", dict(store_bytes=60000 + 100)), ("directory", dict(dir_entries=k)), ("index", dict(max_entries=k))):
        cs = new_store(cw, alg, **kw)
        try:
            recipe = cs.ingest(old)
            before = state(cs)
            with pytest.raises(cw.CwError) as e:
                cs.compose(parts(recipe))
            assert e.value.code == -5, what
            assert state(cs) == before, what
            assert cs.restore(recipe, verify=True) == old
        finally:
            cs.index.close()
    cs = new_store(cw, alg)
    try:
        recipe = cs.ingest(old)
        # a damaged stored chunk inside a window: the position that holds byte 30600 lies behind the new bytes, in front of the landing
        j = int(np.searchsorted(recipe.offsets, 30600, side="right")) - 1
        entry = cs.d_dir.view(-1, 2)[int(recipe.refs[j]) - cs.dir_base]
        saved = entry.clone()
        entry.zero_()
        before = state(cs)
        with pytest.raises(cw.CwError) as e:
            cs.compose(parts(recipe))
        assert e.value.code == -2 and "status 2" in str(e.value), str(e.value)
        assert state(cs) == before
        entry.copy_(saved)
        before = state(cs)
        # max_out one short
        ops, payload = XM.tile([("copy", 0, 30000), ("new", noise(5000, 62)), ("copy", 30500, 29500)])
        ops = np.array(ops, dtype=cw.DELTA_OP_DTYPE)
        pay = np.frombuffer(payload, np.uint8)
        need = (60000 + 5000 - 500) // 64 + 2
        out_refs, out_offs, n, triple = np.zeros(need, np.uint64), np.zeros(need, np.uint64), ctypes.c_size_t(5), cs._triple()
        call = lambda cap: cw.lib().cw_store_compose(cs.index._x(), ctypes.byref(cs.params), cs.comp_alg, ctypes.byref(triple), recipe.refs.ctypes.data,  # noqa: E731
                                                     recipe.offsets.ctypes.data, len(recipe.refs), None, 0, ops.ctypes.data, len(ops), pay.ctypes.data,
                                                     pay.size, cs.base, 0, out_refs.ctypes.data, out_offs.ctypes.data, cap, ctypes.byref(n), None)
        assert call(need - 1) == -2 and b"max_out" in cw.lib().cw_last_error() and n.value == 0
        assert state(cs) == before
        assert call(need) == 0 and out_offs[:n.value + 1].tolist() == CM.chunk(XM.build(old, ops.tolist(), payload), P256)
        cs.base += n.value                                               # (no more than that were rebuilt)
        assert cs.restore(cs.compose(parts(recipe)), verify=True) == old[:30000] + noise(5000, 62) + old[30500:]
    finally:
        cs.index.close()
