"""Stream offsets past 2^32 over a small store.  A stream A of about 2 MiB is ingested once; its recipe repeated
R times with the offsets accumulated (tests/past4g.py: ``tiled_recipe``) is a valid recipe of ``A.bytes * R``, more than 2^32 + 2 MiB
long, over a store of a few MiB.  Restore, verify, ranged reads, accounting, diff / delta, patch and compose run over it: every
recipe offset, range offset, op offset and stream total past 2^32 is one a kernel computed with.  The big results stay on the device;
the models see the arrays, or the few tiles around 2^32."""
import numpy as np
import pytest

import account_model as AM
import delta_model as DM
import past4g as P4
import read_model as RD
import restore_model as RM
from conftest import corpus_file, corpus_large_file

pytestmark = pytest.mark.gpu
B, MIB = P4.B, P4.MIB
ALGS = ["lz4", "lzf"]
TOTALS = ("nonzero", "nonzero_stored", "referenced", "referenced_stored", "shared", "shared_stored", "missing")


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


def _dev_u64(values):
    import torch
    return torch.from_numpy(np.asarray(values, np.uint64).view(np.int64).copy()).cuda()


def stream_a():
    """about 2 MiB: text, a table, noise (stored raw) and text again"""
    noise = np.random.default_rng(12).integers(0, 256, 300000, dtype=np.uint8).tobytes()
    return corpus_large_file("bible.txt")[:1200000] + corpus_file("kennedy.xls")[:400000] + noise + corpus_file("alice29.txt")


class Tiled:
    def __init__(self, cw, alg):
        self.cw, self.alg = cw, alg
        self.cs = cw.ChunkStore(cw.DedupeIndex("skein512", 1 << 13), alg, cw.CdcParams.default(8192), 32 * MIB, 4096, 11)
        self.a = stream_a()
        self.A = self.cs.ingest(self.a)
        edit = np.random.default_rng(13).integers(0, 256, 700, dtype=np.uint8).tobytes()
        self.a2 = self.a[:900000] + edit + self.a[900000:]                    # A': A with 700 bytes inserted
        self.A2 = self.cs.ingest(self.a2)
        self.T, self.K = len(self.a), len(self.A.refs)
        self.R = P4.tiles_for(self.T, B + 4 * self.T)                         # four whole tiles above 2^32: room for an edit's three
        self.recipe = cw.Recipe(*P4.tiled_recipe(self.A.refs, self.A.offsets, self.R))
        assert self.R * self.T > B + 2 * MIB and self.recipe.nbytes == self.R * self.T and self.K > 100

    def tiles(self, m):
        return self.cw.Recipe(*P4.tiled_recipe(self.A.refs, self.A.offsets, m))

    def host_store(self):
        cs = self.cs
        return cs.d_store[:cs.used()].cpu().numpy(), cs.d_dir.cpu().numpy().view(RM.LOC)

    def decode(self, oracle):
        return oracle.lz4_decompress if self.alg == "lz4" else oracle.lzf_decompress


@pytest.fixture(scope="module", params=ALGS)
def tiled(cw, request):
    import torch
    t = Tiled(cw, request.param)
    yield t
    t.cs.index.close()
    del t.cs
    torch.cuda.empty_cache()


@pytest.fixture(autouse=True)
def _free():
    yield
    import torch
    torch.cuda.empty_cache()


def test_restore_and_verify_on_the_device(cw, tiled):
    import torch
    cs, r = tiled.cs, tiled.recipe
    k, n, s = len(r.refs), r.nbytes, _stream()
    d_ref, d_raw, d_count = _dev_u64(r.refs), _dev_u64(r.offsets), _dev_u64([k])
    out, status = torch.full((n,), 0x5C, dtype=torch.uint8, device="cuda"), torch.full((k,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    cw.dev_restore_chunks(cs.comp_alg, cs.d_store.data_ptr(), cs.store_bytes, cs.d_dir.data_ptr(), cs.dir_base, cs.dir_entries, d_ref.data_ptr(),
                          d_raw.data_ptr(), d_count.data_ptr(), k, out.data_ptr(), n, status.data_ptr(), s)
    torch.cuda.synchronize()
    assert not bool(status.any()), status.nonzero()[:4].tolist()
    want = torch.from_numpy(np.frombuffer(tiled.a, np.uint8).copy()).cuda().repeat(tiled.R)
    assert torch.equal(out, want), (out != want).nonzero()[:4].tolist()
    del want
    # restore(verify=True)'s hashing and lookup, on the device: every answer is the recipe's ref
    db = cw.digest_bytes(cs.index.hash_alg)
    dig, found, n_found = torch.zeros(k * db, dtype=torch.uint8, device="cuda"), torch.full((k,), -1, dtype=torch.int64, device="cuda"), _dev_u64([0])
    torch.cuda.synchronize()
    cw.dev_hash_chunks(cs.index.hash_alg, out.data_ptr(), n, d_raw.data_ptr(), d_count.data_ptr(), k, dig.data_ptr(), s)
    cs.index.dev_lookup(dig.data_ptr(), k, found.data_ptr(), n_found.data_ptr(), s)
    torch.cuda.synchronize()
    assert torch.equal(found, d_ref) and int(n_found.item()) == k
    P4.assert_reaches(r.offsets[:-1], r.offsets[1:], "restored extents")


def _around(tiled):
    """(the chunk of the tiled recipe that holds byte 2^32, the tile it lies in)"""
    off = tiled.recipe.offsets.astype(np.int64)
    j = int(np.searchsorted(off, B, side="right")) - 1
    return off, j, B // tiled.T


def test_read_ranges_around_2_32(cw, oracle, tiled):
    import torch
    cs, r = tiled.cs, tiled.recipe
    off, j, tb = _around(tiled)
    assert off[j] + 10 <= B and B + 10 <= off[j + 1], "2^32 lies well inside a chunk of the tiled stream"
    total = r.nbytes
    ranges = [(B - 1000, 999), (B - 1000, 1000), (B - 1000, 1001), (B - 10, 20), (int(off[j]) - 100, B + 100 - (int(off[j]) - 100)),
              (B + 5000, 70000), (B, 0), (B + 3, 1), (total - 100, 200), (total - 100, 100)]
    lens = np.array([l for _, l in ranges], np.uint64)
    dsts = np.concatenate([[0], np.cumsum(lens, dtype=np.uint64)])
    m, k = len(ranges), len(r.refs)
    out, status = torch.full((int(dsts[-1]) + 8,), 0x5C, dtype=torch.uint8, device="cuda"), torch.full((m,), -1, dtype=torch.int32, device="cuda")
    d = [_dev_u64(v) for v in (r.refs, r.offsets, [k], [o for o, _ in ranges], lens, dsts[:-1], [m])]
    torch.cuda.synchronize()
    cw.dev_read_ranges(cs.comp_alg, cs.d_store.data_ptr(), cs.store_bytes, cs.d_dir.data_ptr(), cs.dir_base, cs.dir_entries, d[0].data_ptr(),
                       d[1].data_ptr(), d[2].data_ptr(), k, d[3].data_ptr(), d[4].data_ptr(), d[5].data_ptr(), d[6].data_ptr(), m, out.data_ptr(),
                       int(dsts[-1]), status.data_ptr(), _stream())
    torch.cuda.synchronize()
    host, st = out.cpu().numpy(), status.cpu().numpy().tolist()
    # the model over the tiles around 2^32, and over the last tile for the ranges at the stream's end
    blob, directory = tiled.host_store()
    K, T = tiled.K, tiled.T
    want = []
    for lo_t, hi_t, some in ((tb - 1, tb + 2, ranges[:8]), (tiled.R - 1, tiled.R, ranges[8:])):
        sub = [(o, l, int(dsts[ranges.index((o, l))])) for o, l in some]
        want += RD.read(blob, cs.store_bytes, directory, cs.dir_base, r.refs[lo_t * K:hi_t * K], r.offsets[lo_t * K:hi_t * K + 1], sub, int(dsts[-1]),
                        tiled.decode(oracle))
        assert all(lo_t * T <= o and o + l <= hi_t * T or (o, l) == ranges[8] for o, l in some)
    assert st == [s for s, _ in want] == [0] * 8 + [3, 0], st
    whole = np.frombuffer(tiled.a, np.uint8)
    for i, ((o, l), (s, piece)) in enumerate(zip(ranges, want)):
        if s == 0:
            assert host[int(dsts[i]):int(dsts[i + 1])].tobytes() == piece == np.take(whole, np.arange(o, o + l) % T).tobytes(), (i, o, l)
    assert (host[int(dsts[8]):int(dsts[9])] == 0x5C).all() and (host[int(dsts[-1]):] == 0x5C).all()     # the refused range wrote nothing
    P4.assert_reaches([o for o, _ in ranges], [o + l for o, l in ranges], "ranges")


def test_account_of_the_tiled_stream(cw, tiled):
    cs = tiled.cs
    got = cs.account([tiled.recipe, tiled.A])
    directory = cs.d_dir.cpu().numpy().view(AM.LOC)
    refs = np.concatenate([tiled.recipe.refs, tiled.A.refs])
    verdict, streams, refcount, owner, totals = AM.account_np(refs, [0, len(tiled.recipe.refs), len(refs)], directory, cs.dir_base, None)
    assert verdict == 0
    for f in AM.FIELDS:
        assert got.streams[f].tolist() == streams[f].tolist(), f
    assert got.refcount.tolist() == refcount.tolist() and got.owner.tolist() == owner.tolist()
    assert [got.totals[k] for k in TOTALS] == [int(v) for v in totals[1:]]
    assert int(got.streams["logical_bytes"][0]) == tiled.R * tiled.T > B and int(got.refcount.max()) >= tiled.R + 1


def _copy_with_a_changed_tile(tiled, t):
    """the tiled recipe with tile t replaced by the recipe of A'"""
    K, A, A2 = tiled.K, tiled.A, tiled.A2
    head, tail = tiled.tiles(t), tiled.tiles(tiled.R - t - 1)
    grown = A2.nbytes
    refs = np.concatenate([head.refs, A2.refs, tail.refs])
    offs = np.concatenate([head.offsets[:-1], A2.offsets[:-1] - A2.offsets[0] + np.uint64(t * tiled.T), tail.offsets + np.uint64(t * tiled.T + grown)])
    return tiled.cw.Recipe(refs, offs)


def test_diff_and_delta_above_2_32(cw, tiled):
    cs, old = tiled.cs, tiled.recipe
    t = B // tiled.T + 1                                                      # a tile wholly above 2^32
    new = _copy_with_a_changed_tile(tiled, t)
    assert t * tiled.T > B and t < tiled.R - 3 and new.nbytes == old.nbytes + 700
    d = cs.diff(old, new)
    want = DM.diff(old.refs.tolist(), old.offsets.tolist(), new.refs.tolist(), new.offsets.tolist(), cs.dir_base, cs.dir_entries, 4096)
    assert want["verdict"] == 0 and [tuple(int(v) for v in o) for o in d.ops.tolist()] == want["ops"]
    assert d.src.tolist() == want["src"] and [d.totals[k] for k in cw.DIFF_TOTALS] == want["totals"][1:]
    news = [o for o in want["ops"] if o[2] == DM.NONE]
    assert news and all(o[0] > B for o in news) and sum(1 for o in want["ops"] if o[0] > B and o[2] != DM.NONE) >= 3 and want["ops"][0][0] == 0
    assert d.changed_ranges() == [(o[0], o[1]) for o in news]
    # the delta: the new ops' bytes by ranged reads of the new recipe (cs.delta would bring 4 GiB to the host), applied in the store
    payload = b"".join(cs.read_ranges(new, [(o[0], o[1]) for o in news]))
    a2 = np.frombuffer(tiled.a2, np.uint8)
    assert payload == b"".join(a2[o[0] - t * tiled.T:o[0] - t * tiled.T + o[1]].tobytes() for o in news)
    made = cs.apply_delta(old, cw.Delta(d.ops, np.frombuffer(payload, np.uint8), old.nbytes, new.nbytes))
    assert np.array_equal(made.refs, new.refs) and np.array_equal(made.offsets, new.offsets)
    assert cs.last_compose["new_chunks"] == 0


# ---- patch / compose: the same edit on the tiled recipe and on the few tiles around it --------------------------------------------
def _pair(cw, tiled, tmp_path):
    """two stores loaded from one saved file: new chunks get the same values in both"""
    path = str(tmp_path / "tiled.npz")
    tiled.cs.save(path)
    return cw.ChunkStore.load(path), cw.ChunkStore.load(path)


def _noise(seed, n):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


EDITS = [("write", 3, lambda T: (T + 400000, 7000, _noise(31, 7000))),       # (name, tiles of the short run, the edit in them)
         ("append", 2, lambda T: (2 * T, 0, _noise(33, 30000))),
         ("truncate", 2, lambda T: (2 * T - 31000, 31000, b""))]


@pytest.mark.parametrize("name,m,edit", EDITS, ids=[e[0] for e in EDITS])
def test_patch_above_2_32_is_the_short_patch_spliced(cw, tiled, tmp_path, name, m, edit):
    long_cs, short_cs = _pair(cw, tiled, tmp_path)
    try:
        T, R = tiled.T, tiled.R
        head = R - m if name != "write" else B // T + 1                       # the write lies in a tile wholly above 2^32
        at, r, ins = edit(T)
        assert head * T + at > B and head + m <= R
        short = short_cs.patch(tiled.tiles(m), at, r, ins)
        long_ = long_cs.patch(tiled.recipe, head * T + at, r, ins)
        want_refs, want_off = P4.spliced(tiled.A.refs, tiled.A.offsets, R, head, m, short.refs, short.offsets)
        assert np.array_equal(long_.refs, want_refs) and np.array_equal(long_.offsets, want_off)
        keys = ("window_chunks", "new_chunks", "stored_bytes", "attempts")
        assert {k: long_cs.last_patch[k] for k in keys} == {k: short_cs.last_patch[k] for k in keys}
        assert long_cs.last_patch["first_position"] == short_cs.last_patch["first_position"] + head * tiled.K
        assert long_cs.used() == short_cs.used() and long_cs.base == short_cs.base
        assert torch_equal(long_cs.d_store, short_cs.d_store) and torch_equal(long_cs.d_dir, short_cs.d_dir)
        assert name == "truncate" or long_cs.last_patch["new_chunks"] > 0
    finally:
        long_cs.index.close()
        short_cs.index.close()


def torch_equal(a, b):
    import torch
    return torch.equal(a, b)


def test_compose_and_concat_above_2_32(cw, tiled, tmp_path):
    long_cs, short_cs = _pair(cw, tiled, tmp_path)
    try:
        T, R, m = tiled.T, tiled.R, 3
        head = B // T + 1
        new1, new2 = _noise(41, 9000), _noise(42, 50)

        def parts(recipe, base, end):                                        # two splices inside the tile behind ``base``
            x, y, z = base + T + 300000, base + T + 500000, base + T + 1100000
            return [(recipe, 0, x), new1, (recipe, y, z - y), new2, (recipe, z + 10, end - z - 10)]

        short = short_cs.compose(parts(tiled.tiles(m), 0, m * T))
        long_ = long_cs.compose(parts(tiled.recipe, head * T, R * T))
        want_refs, want_off = P4.spliced(tiled.A.refs, tiled.A.offsets, R, head, m, short.refs, short.offsets)
        assert np.array_equal(long_.refs, want_refs) and np.array_equal(long_.offsets, want_off)
        keys = ("rebuilt_chunks", "new_chunks", "stored_bytes")
        assert {k: long_cs.last_compose[k] for k in keys} == {k: short_cs.last_compose[k] for k in keys} and long_cs.last_compose["new_chunks"] > 0
        assert long_cs.used() == short_cs.used() and torch_equal(long_cs.d_store, short_cs.d_store) and torch_equal(long_cs.d_dir, short_cs.d_dir)
        # concat: offsets past 2^33; the tiled offsets of 2 R tiles but for the chunks around the joint
        both = long_cs.concat([tiled.recipe, tiled.recipe])
        twice = P4.tiled_recipe(tiled.A.refs, tiled.A.offsets, 2 * R)[1]
        odd = np.setxor1d(both.offsets, twice).astype(np.int64)
        assert int(both.offsets[-1]) == 2 * R * T > 1 << 33 and len(odd) <= 32 and (odd > R * T - 65536).all() and (odd < R * T + 8 * 65536).all()
        assert np.array_equal(both.refs[-tiled.K:], tiled.A.refs) and np.array_equal(both.refs[:tiled.K], tiled.A.refs)
    finally:
        long_cs.index.close()
        short_cs.index.close()
