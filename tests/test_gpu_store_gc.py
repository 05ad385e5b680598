"""Mark, compact and retain on the GPU (cw_dev_store_mark, cw_dev_store_compact, cw_dedupe_retain, cw.ChunkStore.compact) against
the plain-Python model of tests/store_gc_model.py.

Device buffers carry canaries: the new store is prefilled with FILL and compared whole, the new directory has guard entries in
front and behind, flags and result words have guards behind them."""
import numpy as np
import pytest

import cdc_model as CM
import restore_model as RM
import store_gc_model as GM
from conftest import corpus_file
from test_gpu_chunk_codec import _dev_u64, _stream, _u64
from test_gpu_dedupe_lifecycle import WIDTHS, Model as IndexModel, check_call, check_lookup, crafted_digests, run_dedupe
from test_gpu_restore import ingest_both, restore_call, same_as_model

pytestmark = pytest.mark.gpu
FILL = 0xA5
GUARD = 256
DIR_GUARD = 4           # guard entries on each side of the new directory
ALGS = ["lz4", "lzf"]
P1K = CM.default_params(1024)
BAD_ARG = -2


@pytest.fixture(scope="module")
def cw():
    import torch  # noqa: F401  (one HIP runtime for torch and libcwhc.so)
    import compute_war_amd as cw
    cw.init(0)
    yield cw
    cw.tune_reset()


@pytest.fixture(scope="module")
def O(oracle):
    return oracle


def _dev(a: np.ndarray):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


# ---- 1. three streams through cw.ChunkStore ------------------------------------------------------------------------------------
@pytest.mark.parametrize("alg", ALGS)
def test_drop_one_stream_of_three(cw, O, alg):
    a, b, c = GM.three_streams(corpus_file("alice29.txt"), corpus_file("kennedy.xls"))
    with cw.DedupeIndex("skein512", 2048) as idx:
        cs = cw.ChunkStore(idx, alg, cw.CdcParams.default(1024), 1 << 20, 512)
        m = RM.Model(O, alg, cs.store_bytes, 512)
        (ra, _), (rb, new_b), (rc, _) = (ingest_both(cs, m, data, P1K) for data in (a, b, c))
        assert idx.count() == len(m.values)
        live, outside = GM.mark(ra.refs, 0, 512)
        live, outside = GM.mark(rc.refs, 0, 512, live, outside)
        only_b = sorted(set(rb.refs.tolist()) - set(ra.refs.tolist()) - set(rc.refs.tolist()))
        verdict, result, blob, new_dir = GM.compact(m.blob, m.store_bytes, m.directory, live, cs.store_bytes)
        assert (verdict, outside) == (0, 0) and 0 < len(only_b) == result[3]
        old_store, old_bytes = cs.d_store, bytes(m.blob)

        got = cs.compact([ra, rc])
        assert got == dict(kept=result[2], dropped=result[3], bytes_before=len(old_bytes), bytes_after=len(blob), removed=len(only_b))
        assert cs.d_store.data_ptr() != old_store.data_ptr() and old_store[:len(old_bytes)].cpu().numpy().tobytes() == old_bytes
        m.blob, m.directory, m.values = bytearray(blob), new_dir, GM.retain(m.values, live, 0, 512)
        same_as_model(cs, m)                                          # new store bytes, cursor and directory
        assert not cs.d_store[len(blob):].any().item()                # nothing behind the cursor
        assert idx.count() == len(m.values)
        assert cs.restore(ra, verify=True) == a and cs.restore(rc, verify=True) == c
        status, out = restore_call(cw, alg, cs.d_store.data_ptr(), cs.store_bytes, cs.d_dir.data_ptr(), 0, 512, rb.refs, rb.offsets, len(b))
        want = [s for s, _ in RM.restore(m.blob, m.store_bytes, m.directory, 0, rb.refs.tolist(), rb.offsets.tolist(), len(b), m.decode())]
        assert status[:len(want)].tolist() == want and want.count(2) == sum(r in only_b for r in rb.refs.tolist()) > 0
        with pytest.raises(cw.CwError):
            cs.restore(rb)
        # the dropped stream again: exactly its own chunks are new, stored behind the kept ones under new values
        base = cs.base
        rb2, new_b2 = ingest_both(cs, m, b, P1K)
        assert new_b2 == new_b and len(new_b2) == len(only_b) and sorted(set(rb2.refs.tolist()) - set(ra.refs.tolist()) - set(rc.refs.tolist())) == \
            [base + i for i in new_b2]
        assert idx.count() == len(m.values)
        assert cs.restore(rb2, verify=True) == b and cs.restore(ra, verify=True) == a and cs.restore(rc, verify=True) == c
        # a new store too small for the kept chunks: the error says how much, and nothing has changed
        with pytest.raises(cw.CwError) as e:
            cs.compact([ra, rc], store_bytes=len(blob) - 1)
        assert e.value.code == -5 and e.value.needed == len(blob)
        same_as_model(cs, m)
        assert idx.count() == len(m.values) and cs.restore(rb2, verify=True) == b
        # a recipe that names values this store never had
        with pytest.raises(cw.CwError) as e:
            cs.compact([ra, cw.Recipe([600, RM.MISS], [0, 10, 20])])
        assert e.value.code == BAD_ARG
        same_as_model(cs, m)
        assert idx.count() == len(m.values)
        assert cs.compact([ra, rb2, rc], store_bytes=len(m.blob))["removed"] == 0     # everything kept, into exactly enough room
        same_as_model(cs, m)


# ---- hand-built stores -----------------------------------------------------------------------------------------------------------
N_HAND = 9000           # more than two 4,096-entry scan tiles


class Hand:
    """A store made on the host: about half the entries zero, stored 1..300 bytes at every residue of pos mod 16, one raw
    65,536-byte entry; every byte of the store random, gaps between the extents included."""

    def __init__(self, n=N_HAND, seed=17):
        rng = np.random.default_rng(seed)
        self.n = n
        self.directory = np.zeros(n, RM.LOC)
        pos, big = 0, n // 2 + 1
        for i in range(n):
            if i == big:
                stored, word = 65536, 65536 | RM.RAW
            elif i != n - 1 and rng.random() < 0.5:
                continue
            else:
                stored = int(rng.integers(1, 301))
                word = (stored | RM.RAW) if rng.random() < 0.3 else int(rng.integers(stored + 1, 65537))
            pos += int(rng.integers(0, 6))
            self.directory[i] = (pos, stored, word)
            pos += stored
        self.store_bytes = pos + 7
        self.store = rng.integers(0, 256, self.store_bytes, dtype=np.uint8)
        nz = self.directory["raw"] != 0
        assert 0.4 * n < nz.sum() < 0.6 * n and set((self.directory["pos"][nz] % 16).tolist()) == set(range(16))
        assert self.directory["stored"][nz].min() == 1 and self.directory["stored"][nz & (np.arange(n) != big)].max() == 300
        self.d_store, self.d_dir = _dev(self.store), _dev(self.directory)

    def live(self, pattern):
        live = np.zeros(self.n, np.uint32)
        if pattern == "all":
            live[:] = 1
        elif pattern == "third":
            live[::3] = 7                  # any non-zero value is a flag
        elif pattern == "wave":
            live[4096 + 64:4096 + 128] = 1   # one wavefront's 64 entries, with the 65,536-byte entry outside
        elif pattern == "last":
            live[-1] = 1
        else:
            assert pattern == "none"
        return live


@pytest.fixture(scope="module")
def hand(cw):
    return Hand()


class Target:
    """The buffers a compaction writes, with their canaries."""

    def __init__(self, new_store_bytes, n, shift=0, in_place_of=None, dry=False):
        import torch
        self.n, self.bytes, self.dry, self.shift = n, new_store_bytes, dry, shift
        self.buf = torch.full((GUARD + shift + new_store_bytes + GUARD,), FILL, dtype=torch.uint8, device="cuda")
        self.dirbuf = torch.full(((n + 2 * DIR_GUARD) * 2,), -1, dtype=torch.int64, device="cuda")
        if in_place_of is not None:
            self.dirbuf[2 * DIR_GUARD:-2 * DIR_GUARD] = in_place_of.view(torch.int64)
        self.used = torch.full((2,), -1, dtype=torch.int64, device="cuda")
        self.result = torch.full((5,), -1, dtype=torch.int64, device="cuda")
        self.d_store = 0 if dry else self.buf.data_ptr() + GUARD + shift
        self.d_dir = self.dirbuf.data_ptr() + 16 * DIR_GUARD

    def fetch(self):
        import torch
        torch.cuda.synchronize()
        host, d = self.buf.cpu().numpy(), self.dirbuf.cpu().numpy()
        lo = GUARD + self.shift
        assert (host[:lo] == FILL).all() and (host[lo + self.bytes:] == FILL).all(), "store guards"
        assert (d[:2 * DIR_GUARD] == -1).all() and (d[-2 * DIR_GUARD:] == -1).all(), "directory guards"
        used, result = _u64(self.used), _u64(self.result)
        assert used[1] == RM.MISS and result[4] == RM.MISS, "cursor / result guards"
        return host[lo:lo + self.bytes], d[2 * DIR_GUARD:-2 * DIR_GUARD].copy(), int(used[0]), result[:4].tolist()


def compact_call(cw, h: Hand, d_dir, live, t: Target, in_place=False, store_bytes=None):
    d_live = _dev(np.concatenate([live, np.full(4, 0xFFFFFFFF, np.uint32)]))
    import torch
    torch.cuda.synchronize()
    cw.dev_store_compact(h.d_store.data_ptr(), h.store_bytes if store_bytes is None else store_bytes, t.d_dir if in_place else d_dir.data_ptr(),
                         h.n, d_live.data_ptr(), t.d_store, 0 if t.dry else t.bytes, t.used.data_ptr(), t.d_dir, t.result.data_ptr(), _stream())
    return t.fetch()


def check_unchanged(got, n, want_result, directory_before=None):
    store, d, used, result = got
    assert result == want_result
    assert (store == FILL).all() and used == RM.MISS, "a refused compaction wrote the new store or the cursor"
    assert (d == -1).all() if directory_before is None else (d.view(RM.LOC) == directory_before).all(), "a refused compaction wrote the new directory"


def check_compacted(got, model):
    store, d, used, result = got
    verdict, want_result, blob, new_dir = model
    assert verdict == 0 and result == want_result and used == len(blob)
    diff = np.nonzero(store[:len(blob)] != np.frombuffer(blob, np.uint8))[0]
    assert len(diff) == 0, ("store differs at", int(diff[0]), len(diff))
    assert (store[len(blob):] == FILL).all(), "bytes behind the total were written"
    bad = np.nonzero(d.view(RM.LOC) != new_dir)[0]
    assert len(bad) == 0, ("entry", int(bad[0]), d.view(RM.LOC)[bad[0]], new_dir[bad[0]], len(bad))


# ---- 2. every live pattern ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift,pattern", list(enumerate(["all", "none", "third", "wave", "last"])))
def test_hand_built_store(cw, hand, pattern, shift):
    live = hand.live(pattern)
    model = GM.compact(hand.store, hand.store_bytes, hand.directory, live, hand.store_bytes)
    nz = int(np.count_nonzero(hand.directory["raw"]))
    assert model[1][2] + model[1][3] == nz and (model[1][2] > 0) == (pattern != "none")
    if pattern == "wave":
        assert 20 < model[1][2] < 45
    # exactly enough room, at a destination of another alignment each time
    check_compacted(compact_call(cw, hand, hand.d_dir, live, Target(model[1][1], hand.n, shift=3 * shift)), model)
    assert hand.d_store.cpu().numpy().tobytes() == hand.store.tobytes() and hand.d_dir.cpu().numpy().tobytes() == hand.directory.tobytes()


# ---- 3. all or nothing -----------------------------------------------------------------------------------------------------------
def test_too_small_and_dry_run_change_nothing(cw, hand):
    live = hand.live("third")
    verdict, result, blob, _ = GM.compact(hand.store, hand.store_bytes, hand.directory, live, hand.store_bytes)
    total = len(blob)
    assert verdict == 0 and total > 65536
    check_unchanged(compact_call(cw, hand, hand.d_dir, live, Target(total - 1, hand.n)), hand.n, [1] + result[1:])
    check_unchanged(compact_call(cw, hand, hand.d_dir, live, Target(16, hand.n, dry=True)), hand.n, [1] + result[1:])   # NULL / 0
    # nothing kept: the dry run's verdict is 0, the new directory is all zero and the cursor 0
    store, d, used, result = compact_call(cw, hand, hand.d_dir, hand.live("none"), Target(16, hand.n, dry=True))
    assert result == [0, 0, 0, int(np.count_nonzero(hand.directory["raw"]))] and used == 0 and not d.any() and (store == FILL).all()


def _unsound(hand, live):
    """(name, entry index, the damaged entry): each on an entry that is kept under `live`."""
    d = hand.directory
    kept = [i for i in range(hand.n) if live[i] and d[i]["raw"]]
    comp = next(i for i in kept if not d[i]["raw"] & RM.RAW)
    raw = next(i for i in kept if d[i]["raw"] & RM.RAW)
    pos, stored, word = (int(v) for v in d[comp])
    rpos, rstored, rword = (int(v) for v in d[raw])
    return [("pos = store_bytes", comp, (hand.store_bytes, stored, word)),
            ("one byte past the store", comp, (hand.store_bytes - stored + 1, stored, word)),
            ("pos + stored wraps", comp, (2 ** 64 - 1, stored, word)),
            ("a reserved bit", comp, (pos, stored, word | 1 << 20)),
            ("stored = 0", comp, (pos, 0, word)),
            ("raw with stored != length", raw, (rpos, rstored - 1 if rstored > 1 else 2, rword)),
            ("length above 65536", comp, (pos, stored, 65537)),
            ("length 0, only pos set", comp, (5, 0, 0))]


def test_an_unsound_kept_entry_refuses_and_an_unmarked_one_is_dropped(cw, hand):
    live = hand.live("third")
    for name, i, entry in _unsound(hand, live):
        bad = hand.directory.copy()
        bad[i] = entry
        d_bad = _dev(bad)
        model = GM.compact(hand.store, hand.store_bytes, bad, live, hand.store_bytes)
        assert model[0] == 2, name
        check_unchanged(compact_call(cw, hand, d_bad, live, Target(hand.store_bytes, hand.n)), hand.n, model[1])
        # the same entry not marked: dropped like any other
        off = live.copy()
        off[i] = 0
        model = GM.compact(hand.store, hand.store_bytes, bad, off, hand.store_bytes)
        assert model[0] == 0 and model[3][i]["raw"] == 0, name
        check_compacted(compact_call(cw, hand, d_bad, off, Target(hand.store_bytes, hand.n)), model)
    # a store shorter than its directory says: the entries past it are unsound when kept, and nothing is loaded from there
    short = int(hand.directory[hand.n // 2]["pos"])
    model = GM.compact(hand.store, short, hand.directory, live, hand.store_bytes)
    assert model[0] == 2
    check_unchanged(compact_call(cw, hand, hand.d_dir, live, Target(hand.store_bytes, hand.n), store_bytes=short), hand.n, model[1])


# ---- 4. the directory in place ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", ["third", "wave"])
def test_directory_in_place(cw, hand, pattern):
    live = hand.live(pattern)
    model = GM.compact(hand.store, hand.store_bytes, hand.directory, live, hand.store_bytes)
    separate = compact_call(cw, hand, hand.d_dir, live, Target(model[1][1] + 64, hand.n))
    check_compacted(separate, model)
    t = Target(model[1][1] + 64, hand.n, in_place_of=hand.d_dir)
    in_place = compact_call(cw, hand, None, live, t, in_place=True)
    check_compacted(in_place, model)
    assert in_place[1].tobytes() == separate[1].tobytes()
    assert hand.d_store.cpu().numpy().tobytes() == hand.store.tobytes()      # the old store's bytes stay in both forms
    # in place and refused: the directory is as it was
    t = Target(model[1][1] - 1, hand.n, in_place_of=hand.d_dir)
    check_unchanged(compact_call(cw, hand, None, live, t, in_place=True), hand.n, [1] + model[1][1:], directory_before=hand.directory)


# ---- 5. mark ------------------------------------------------------------------------------------------------------------------------
def test_mark(cw):
    import torch
    rng = np.random.default_rng(23)
    base, entries, n = 1000, 5000, 3000
    refs = rng.integers(base, base + entries, n).astype(np.uint64)
    refs[::7] = rng.integers(0, base, len(refs[::7]))            # below the base
    refs[5], refs[6], refs[8], refs[9] = base + entries, RM.MISS, base - 1, base + entries - 1
    refs[10] = base
    tail = np.full(64, base + 1, np.uint64)                         # behind the count: never read (they would set live[1])
    refs[refs == base + 1] = base + 2
    d_ref = _dev_u64(np.concatenate([refs, tail]))
    live = torch.zeros(entries + 8, dtype=torch.int32, device="cuda")
    live[entries:] = -1
    n_out = _dev_u64([0, 99])
    counts = []                                                      # (kept alive until the calls have run)

    def call(count, max_count, d=d_ref):
        counts.append(_dev_u64([count]))
        cw.dev_store_mark(d.data_ptr(), counts[-1].data_ptr(), max_count, base, entries, live.data_ptr(), n_out.data_ptr(), _stream())

    torch.cuda.synchronize()

    def state():
        torch.cuda.synchronize()
        h = live.cpu().numpy().view(np.uint32)
        assert (h[entries:] == 0xFFFFFFFF).all() and _u64(n_out)[1] == 99, "guards"
        return h[:entries].copy(), int(_u64(n_out)[0])

    call(10 ** 12, n)                                               # *d_count above max_count
    want, outside = GM.mark(refs, base, entries)
    got = state()
    assert (got[0] == want).all() and got[1] == outside and want[1] == 0 and want[0] == 1 and want[-1] == 1 and outside > n // 7
    call(n, n + 64)                                                 # twice: the flags stay, the count accumulates
    got = state()
    assert (got[0] == want).all() and got[1] == 2 * outside
    call(0, n)                                                      # nothing
    assert state()[1] == 2 * outside
    call(100, n + 64)                                               # *d_count below max_count
    assert state()[1] == 2 * outside + GM.mark(refs[:100], base, entries)[1]
    more = _dev_u64([base + 1, RM.MISS, base + 1])
    call(3, 3, more)
    want[1] = 1
    got = state()
    assert (got[0] == want).all() and got[1] == 2 * outside + GM.mark(refs[:100], base, entries)[1] + 1


# ---- 6. retain ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alg,db", WIDTHS)
def test_retain(cw, alg, db):
    import torch
    rng = np.random.default_rng(31 + db)
    n, base, entries = 6000, 1 << 20, 4000
    d = crafted_digests(db, n, seed=300 + db, dups=False)
    u64 = lambda v: np.asarray(v, np.uint64)  # noqa: E731
    values = np.concatenate([u64(base + rng.permutation(entries)), u64(rng.integers(0, base, 1000)),
                             u64(base + entries + rng.integers(0, 1 << 40, 999)), u64([RM.MISS - 1])])
    values = values[rng.permutation(n)]
    live = (rng.random(entries) < 0.4).astype(np.uint32) * 5
    d_live = _dev(live)
    with cw.DedupeIndex(alg, 8192) as idx:
        model = IndexModel()
        check_call(idx, model, d[:3000], values=values[:3000])
        check_call(idx, model, d[3000:], values=values[3000:])
        kept = GM.retain(model.table, live, base, entries)
        dropped = [i for i in range(n) if d[i].tobytes() not in kept]
        assert 2000 < len(dropped) < 2800 and len(kept) == n - len(dropped)
        torch.cuda.synchronize()
        # below the kept count: refused on the device's word, and every lookup answers as before
        for too_small in (len(kept) - 1, 100):
            with pytest.raises(cw.CwError) as e:
                idx.retain(d_live.data_ptr(), base, entries, too_small)
            assert e.value.code == BAD_ARG
            assert idx.count() == n and idx.max_entries == 8192
        check_lookup(idx, model, d)
        # a smaller table that still holds the kept entries
        assert idx.retain(d_live.data_ptr(), base, entries, len(kept)) == len(dropped)
        model.table = kept
        assert idx.count() == len(kept) and idx.max_entries == len(kept)
        ref = check_lookup(idx, model, d)                              # kept: their values; dropped: CW_DEDUPE_MISS
        assert (ref[dropped] == RM.MISS).all() and (ref != RM.MISS).sum() == len(kept)
        # full now: a dropped digest goes in again only after a retain that makes room
        with pytest.raises(cw.CwError) as e:
            run_dedupe(idx, d[dropped[:8]], values=np.arange(8, dtype=np.uint64))
        assert e.value.code == -5
        assert idx.retain(d_live.data_ptr(), base, entries, 8192) == 0
        assert idx.count() == len(kept) and idx.max_entries == 8192
        check_lookup(idx, model, d)
        check_call(idx, model, d[dropped], values=np.arange(7, 7 + len(dropped), dtype=np.uint64))   # new values
        check_lookup(idx, model, d)
        # max_entries as it is; the entries just inserted have values outside the directory and stay
        assert idx.retain(d_live.data_ptr(), base, entries) == 0 and idx.count() == n
        # nothing live and a directory that spans every value: the index is empty, and works
        d_none = torch.zeros(16, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        assert idx.retain(d_none.data_ptr(), base, 16) == len([v for v in model.table.values() if base <= v < base + 16])
        with cw.DedupeIndex(alg, 8192) as idx2:
            m2 = IndexModel()
            check_call(idx2, m2, d[:2000], base=0)
            z = torch.zeros(2000, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            assert idx2.retain(z.data_ptr(), 0, 2000) == 2000 and idx2.count() == 0
            m2.table = {}
            check_lookup(idx2, m2, d[:2000])
            check_call(idx2, m2, d[1000:3000], base=5000)               # cw_dev_dedupe on the emptied index
            check_lookup(idx2, m2, d)


# ---- 7. save / load of a compacted store ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alg", ALGS)
def test_save_load_of_a_compacted_store(cw, O, alg, tmp_path):
    a, b, c = GM.three_streams(corpus_file("alice29.txt"), corpus_file("kennedy.xls"))
    path = str(tmp_path / "store.npz")
    with cw.DedupeIndex("skein512", 2048) as idx:
        cs = cw.ChunkStore(idx, alg, cw.CdcParams.default(1024), 1 << 20, 512, dir_base=40)
        ra, rb, rc = (cs.ingest(data) for data in (a, b, c))
        before = idx.count()
        got = cs.compact([ra, rc], store_bytes=200_000)
        assert got["removed"] == got["dropped"] > 0 and got["bytes_after"] < got["bytes_before"] and cs.store_bytes == 200_000
        assert idx.count() == before - got["removed"] == got["kept"]
        cs.save(path)
        used, base = cs.used(), cs.base
    cs2 = cw.ChunkStore.load(path)
    try:
        assert cs2.used() == used == got["bytes_after"] and cs2.base == base and cs2.index.count() == got["kept"]
        assert cs2.restore(ra, verify=True) == a and cs2.restore(rc, verify=True) == c
        with pytest.raises(cw.CwError):
            cs2.restore(rb)
        rb2 = cs2.ingest(b)                                              # and it goes on
        assert cs2.restore(rb2, verify=True) == b and cs2.index.count() == before
    finally:
        cs2.index.close()
