"""The chunk store on the GPU (cw_dev_store_chunks, cw_dev_restore_chunks, cw.ChunkStore) against the plain-Python model of
tests/restore_model.py, which takes its compressed bytes and its decoders' verdicts from the CPU oracle.

Device buffers carry canaries: the store bytes and the destination are prefilled with FILL and compared whole against the
model's image, the directory has guard entries in front and behind, sizes / statuses past a count keep their -1."""
import threading

import numpy as np
import pytest

import cdc_model as CM
import lz_streams as LS
import restore_model as RM
from conftest import corpus_file, corpus_names
from test_gpu_chunk_codec import Run, _dev_u64, _stream, _u64

pytestmark = pytest.mark.gpu
FILL = 0xA5
GUARD = 256
DIR_GUARD = 4           # guard entries on each side of the directory
ALGS = ["lz4", "lzf"]
P1K = CM.default_params(1024)


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


def _noise(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


# ---- a store with canaries, and its image on the host ------------------------------------------------------------------------
class Store:
    def __init__(self, store_bytes, dir_entries, dir_base=0):
        import torch
        self.store_bytes, self.dir_entries, self.dir_base = store_bytes, dir_entries, dir_base
        self.buf = torch.full((GUARD + store_bytes + GUARD,), FILL, dtype=torch.uint8, device="cuda")
        self.dirbuf = torch.zeros((dir_entries + 2 * DIR_GUARD) * 2, dtype=torch.int64, device="cuda")
        self.dirbuf[:2 * DIR_GUARD] = -1
        self.dirbuf[-2 * DIR_GUARD:] = -1
        self.used = torch.zeros(1, dtype=torch.int64, device="cuda")
        self.result = torch.full((2,), -1, dtype=torch.int64, device="cuda")
        self.d_store, self.d_dir = self.buf.data_ptr() + GUARD, self.dirbuf.data_ptr() + 16 * DIR_GUARD
        # the model's image
        self.x_store, self.x_dir, self.x_used = np.full(store_bytes, FILL, np.uint8), np.zeros(dir_entries, RM.LOC), 0

    def append(self, cw, alg, r: Run, base, stream=None, **over):
        """cw_dev_store_chunks behind the compressing call of `r`, with r's own arguments."""
        a = dict(store_bytes=self.store_bytes, dir_base=self.dir_base, dir_entries=self.dir_entries)
        a.update(over)
        cw.dev_store_chunks(alg, r.d_src, r.src_bytes, r.d_off.data_ptr(), r.d_k.data_ptr(), r.max_chunks, r.d_dst, r.d_sizes.data_ptr(), base,
                            self.d_store, a["store_bytes"], self.used.data_ptr(), self.d_dir, a["dir_base"], a["dir_entries"],
                            self.result.data_ptr(), _stream() if stream is None else stream,
                            r.d_sel.data_ptr() if r.d_sel is not None else 0, r.d_nsel.data_ptr() if r.d_sel is not None else 0)

    def expect(self, O, alg, data, cuts, chunks, base, count=None, src_bytes=None, **over):
        """The model's append of the same call, applied to the image; returns (verdict, total)."""
        a = dict(store_bytes=self.store_bytes, dir_base=self.dir_base, dir_entries=self.dir_entries)
        a.update(over)
        comp = RM.compressed(O, alg, data, cuts, chunks, count, src_bytes)
        verdict, total, blob, entries = RM.append(data, cuts, chunks, comp, base, self.x_used, a["store_bytes"], a["dir_base"], a["dir_entries"],
                                                  count, src_bytes)
        self.x_store[self.x_used:self.x_used + len(blob)] = np.frombuffer(blob, np.uint8)
        self.x_used += len(blob)
        for idx, e in entries.items():
            self.x_dir[idx] = e
        return verdict, total

    def check(self, want_result=None):
        """Store bytes, cursor, directory and all guards against the image."""
        import torch
        torch.cuda.synchronize()
        host, d = self.buf.cpu().numpy(), self.dirbuf.cpu().numpy()
        assert (host[:GUARD] == FILL).all() and (host[-GUARD:] == FILL).all(), "store guards"
        assert (d[:2 * DIR_GUARD] == -1).all() and (d[-2 * DIR_GUARD:] == -1).all(), "directory guards"
        assert int(self.used.item()) == self.x_used
        diff = np.nonzero(host[GUARD:-GUARD] != self.x_store)[0]
        assert len(diff) == 0, ("store differs at", int(diff[0]), len(diff))
        got = d[2 * DIR_GUARD:-2 * DIR_GUARD].view(RM.LOC)
        bad = np.nonzero(got != self.x_dir)[0]
        assert len(bad) == 0, ("entry", int(bad[0]), got[bad[0]], self.x_dir[bad[0]], len(bad))
        if want_result is not None:
            assert tuple(_u64(self.result).tolist()) == tuple(want_result)


def restore_call(cw, alg, d_store, store_bytes, d_dir, dir_base, dir_entries, refs, raw_offsets, dst_bytes, count=None, max_count=None):
    """cw_dev_restore_chunks into a canary-filled destination: (status with 2 extra entries, destination with its guards)."""
    import torch
    n = len(refs)
    d_ref, d_raw = _dev_u64(list(refs) + [0]), _dev_u64(raw_offsets)
    d_count = _dev_u64([n if count is None else count])
    out = torch.full((GUARD + dst_bytes + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    status = torch.full((n + 2,), -1, dtype=torch.int32, device="cuda")
    cw.dev_restore_chunks(alg, d_store, store_bytes, d_dir, dir_base, dir_entries, d_ref.data_ptr(), d_raw.data_ptr(), d_count.data_ptr(),
                          n if max_count is None else max_count, out.data_ptr() + GUARD, dst_bytes, status.data_ptr(), _stream())
    torch.cuda.synchronize()
    return status.cpu().numpy(), out.cpu().numpy()


def check_restore(status, out, want, raw_offsets, dst_bytes, n=None):
    """`want` = the model's [(status, bytes or None)]: statuses, the bytes of every status-0 extent, and FILL everywhere else except
    inside status-1 extents (unspecified)."""
    n = len(want) if n is None else n
    assert status[:n].tolist() == [s for s, _ in want[:n]]
    assert (status[n:] == -1).all(), "statuses past the count were written"
    image = np.full(GUARD + dst_bytes + GUARD, FILL, np.uint8)
    out = out.copy()
    for j, (s, piece) in enumerate(want[:n]):
        lo, hi = GUARD + int(raw_offsets[j]), GUARD + int(raw_offsets[j + 1])
        if s == 0:
            image[lo:hi] = np.frombuffer(piece, np.uint8)
        elif s == 1:
            out[lo:hi] = FILL
    diff = np.nonzero(out != image)[0]
    assert len(diff) == 0, ("destination differs at", int(diff[0]) - GUARD, len(diff))


def restore_store(cw, O, alg, st: Store, refs, raw_offsets, dst_bytes, **kw):
    """Restore from a Store (which has been checked against its image) and from the model of that image; returns the bytes."""
    status, out = restore_call(cw, alg, st.d_store, st.store_bytes, st.d_dir, st.dir_base, st.dir_entries, refs, raw_offsets, dst_bytes, **kw)
    decode = O.lz4_decompress if alg == "lz4" else O.lzf_decompress
    want = RM.restore(st.x_store, st.store_bytes, st.x_dir, st.dir_base, refs, raw_offsets, dst_bytes, decode)
    n = min(kw.get("count", len(refs)) if kw.get("count") is not None else len(refs), kw.get("max_count") or len(refs))
    check_restore(status, out, want, raw_offsets, dst_bytes, n)
    return status, out[GUARD:GUARD + dst_bytes]


# ---- cw.ChunkStore against the model over whole ingests ---------------------------------------------------------------------
def same_as_model(cs, m: RM.Model):
    used = cs.used()
    assert used == len(m.blob)
    assert cs.d_store[:used].cpu().numpy().tobytes() == bytes(m.blob)
    got = cs.d_dir.cpu().numpy().view(RM.LOC)
    bad = np.nonzero(got != m.directory)[0]
    assert len(bad) == 0, ("entry", int(bad[0]), got[bad[0]], m.directory[bad[0]], len(bad))


def ingest_both(cs, m: RM.Model, data: bytes, p: dict):
    cuts = CM.chunk(data, p)
    base = cs.base
    recipe = cs.ingest(data)
    refs, new, verdict, _ = m.ingest(data, cuts, base)
    assert verdict == 0 and recipe.offsets.tolist() == cuts and recipe.refs.tolist() == refs
    same_as_model(cs, m)
    return recipe, new


@pytest.fixture(scope="module")
def canterbury():
    return b"".join(corpus_file(n) for n in corpus_names())


@pytest.mark.parametrize("normal", [1024, 8192])
@pytest.mark.parametrize("alg", ALGS)
def test_corpus_round_trip(cw, O, canterbury, alg, normal):
    k_max = len(canterbury) // (normal // 4) + 2
    with cw.DedupeIndex("skein512", k_max) as idx:
        cs = cw.ChunkStore(idx, alg, cw.CdcParams.default(normal), len(canterbury) + 4096, k_max)
        m = RM.Model(O, alg, cs.store_bytes, k_max)
        recipe, new = ingest_both(cs, m, canterbury, CM.default_params(normal))
        assert len(new) > 0 and len(m.blob) < 0.9 * len(canterbury)
        assert cs.restore(recipe) == canterbury
        assert cs.restore(recipe, verify=True) == canterbury
        # the raw call: all statuses 0
        n = len(recipe.refs)
        status, out = restore_call(cw, alg, cs.d_store.data_ptr(), cs.store_bytes, cs.d_dir.data_ptr(), 0, k_max, recipe.refs, recipe.offsets,
                                   len(canterbury))
        assert (status[:n] == 0).all() and (status[n:] == -1).all()
        assert out[GUARD:-GUARD].tobytes() == canterbury and (out[:GUARD] == FILL).all() and (out[-GUARD:] == FILL).all()


@pytest.mark.parametrize("alg", ALGS)
def test_both_stored_forms_in_one_call(cw, O, alg):
    text = corpus_file("kennedy.xls")[:48000] + corpus_file("lcet10.txt")[:48000]
    data = b"".join(text[k * 8000:(k + 1) * 8000] + _noise(8000, 100 + k) for k in range(12))
    with cw.DedupeIndex("skein512", 2048) as idx:
        cs = cw.ChunkStore(idx, alg, cw.CdcParams.default(1024), len(data) + 4096, 2048, dir_base=1000)
        m = RM.Model(O, alg, cs.store_bytes, 2048, dir_base=1000)
        recipe, new = ingest_both(cs, m, data, P1K)
        words = m.directory["raw"][m.directory["raw"] != 0]
        assert (words & RM.RAW != 0).sum() >= 20 and (words & RM.RAW == 0).sum() >= 20
        assert recipe.refs.min() >= 1000
        assert cs.restore(recipe, verify=True) == data
        # verify notices a store that no longer holds what the index says: one byte of a chunk kept raw changed
        at = int(m.directory[np.nonzero(m.directory["raw"] & RM.RAW)[0][3]]["pos"])
        cs.d_store[at] ^= 1
        assert cs.restore(recipe) != data
        with pytest.raises(cw.CwError):
            cs.restore(recipe, verify=True)


def _edited(a: bytes) -> bytes:
    b = bytearray(a)
    b[50_000:50_000] = b"an insertion of some length"
    del b[120_000:120_300]
    b[200_000:200_010] = b"OVERWRITE!"
    b[300_000:300_000] = bytes(range(256))
    del b[400_000:400_001]
    return bytes(b)


@pytest.mark.parametrize("alg", ALGS)
def test_two_ingests_into_one_store(cw, O, alg, tmp_path):
    a = corpus_file("lcet10.txt")
    b = _edited(a)
    with cw.DedupeIndex("skein512", 2048) as idx:
        cs = cw.ChunkStore(idx, alg, cw.CdcParams.default(1024), len(a) + 65536, 2048)
        m = RM.Model(O, alg, cs.store_bytes, 2048)
        ra, new_a = ingest_both(cs, m, a, P1K)
        k_a = len(ra.refs)
        assert cs.base == k_a
        rb, new_b = ingest_both(cs, m, b, P1K)
        assert rb.refs.max() >= k_a and (rb.refs < k_a).sum() > len(rb.refs) // 2 and 0 < len(new_b) < 40
        assert cs.restore(rb, verify=True) == b      # most of B's refs name what A's call stored
        assert cs.restore(ra, verify=True) == a
        idx.resize(5000)
        assert cs.restore(rb, verify=True) == b and cs.restore(ra, verify=True) == a
        path = str(tmp_path / "store.npz")
        cs.save(path)
        used = cs.used()
    cs2 = cw.ChunkStore.load(path)
    try:
        assert cs2.used() == used and cs2.base == k_a + len(rb.refs) and cs2.index.count() == len(new_a) + len(new_b)
        same_as_model(cs2, m)
        assert cs2.restore(rb, verify=True) == b and cs2.restore(ra, verify=True) == a
        # and it goes on: a third stream, deduped against the loaded index
        c = a[:100_000] + b"third" + a[100_000:]
        rc, new_c = ingest_both(cs2, m, c, P1K)
        assert len(new_c) < 10 and cs2.restore(rc, verify=True) == c
    finally:
        cs2.index.close()


@pytest.mark.parametrize("alg", ALGS)
def test_duplicates_inside_one_call(cw, O, alg):
    x = corpus_file("alice29.txt")
    data = x + x + x[:70_000] + b"changed" + x[70_000:]
    with cw.DedupeIndex("skein512", 2048) as idx:
        cs = cw.ChunkStore(idx, alg, cw.CdcParams.default(1024), len(x) + 65536, 2048)
        m = RM.Model(O, alg, cs.store_bytes, 2048)
        recipe, new = ingest_both(cs, m, data, P1K)
        assert len(new) < 0.4 * len(recipe.refs)
        values, counts = np.unique(recipe.refs, return_counts=True)
        assert (counts >= 3).sum() > len(values) // 2    # most chunks occur three times, and every occurrence is restored
        assert cs.restore(recipe, verify=True) == data


# ---- hand-made offset lists ---------------------------------------------------------------------------------------------------
EDGE = [1, 2, 3, 12, 13, 18, 19, 4095, 65535, 65536]


@pytest.mark.parametrize("kind", ["text", "noise"])
@pytest.mark.parametrize("alg", ALGS)
def test_edge_lengths_at_every_misalignment(cw, O, alg, kind):
    rng = np.random.default_rng(61)
    lens = EDGE + EDGE[:7] + [5, 7, 11]
    total = sum(lens)
    text = (corpus_file("alice29.txt") + corpus_file("lcet10.txt"))[:total]
    data = np.frombuffer(text if kind == "text" else _noise(total, 7), np.uint8)
    for shift in range(16):
        order = rng.permutation(len(lens))
        cuts = np.concatenate([[0], np.cumsum([lens[i] for i in order])]).tolist()
        k = len(lens)
        r = Run(cw, alg, data, cuts=cuts, shift=(5 * shift + 3) % 16).fetch()
        st = Store(total + 64, k + 3, dir_base=7)
        st.append(cw, alg, r, base=8)
        verdict, want_total = st.expect(O, alg, data, cuts, range(k), 8)
        st.check((0, want_total))
        assert verdict == 0 and (st.x_dir["raw"][1:k + 1] & RM.LEN_MASK).tolist() == [lens[i] for i in order]
        # the raw extents start at `shift` mod 16 and then at whatever the lengths give
        raw = [shift + c for c in cuts]
        status, out = restore_store(cw, O, alg, st, [8 + i for i in range(k)], raw, shift + total)
        assert (status[:k] == 0).all() and out[shift:].tobytes() == data.tobytes()


# ---- refusals -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alg", ALGS)
def test_refusals_leave_everything_as_it_was(cw, O, alg):
    data = np.frombuffer(corpus_file("alice29.txt")[:90_000] + _noise(20_000, 3), np.uint8)
    cuts = CM.chunk(data, P1K)
    k = len(cuts) - 1
    r = Run(cw, alg, data, cuts=cuts).fetch()
    st = Store(len(data) + 4096, k + 8, dir_base=100)
    first = Run(cw, alg, data[:5000], cuts=[0, 2000, 5000]).fetch()   # something in the store already
    st.append(cw, alg, first, base=100 + k + 2)
    assert st.expect(O, alg, data[:5000], [0, 2000, 5000], range(2), 100 + k + 2)[0] == 0
    st.check()
    probe = Store(len(data) + 4096, k, dir_base=0)
    _, total = probe.expect(O, alg, data, cuts, range(k), 0)
    # one byte short; one chunk in front of the directory; one chunk behind it; a value that wraps: nothing changes
    for over, base, want in ((dict(store_bytes=st.x_used + total - 1), 100, 1), (dict(dir_base=101), 100, 2), (dict(dir_entries=k - 1), 100, 2),
                             (dict(dir_base=0, dir_entries=k + 8), 2 ** 64 - 2, 2)):
        st.append(cw, alg, r, base=base, **over)
        st.check((want, total))
    st.append(cw, alg, r, base=100, store_bytes=st.x_used + total - 1, dir_entries=k - 1)   # both: the store's verdict comes first
    st.check((1, total))
    st.append(cw, alg, r, base=100, store_bytes=st.x_used + total)    # exactly enough room
    assert st.expect(O, alg, data, cuts, range(k), 100, store_bytes=st.x_used + total) == (0, total)
    st.check((0, total))
    refs = [100 + i for i in range(k)] + [100 + k + 2, 100 + k + 3]
    raw = cuts + [cuts[-1] + 2000, cuts[-1] + 5000]
    status, out = restore_store(cw, O, alg, st, refs, raw, raw[-1])
    assert (status[:k + 2] == 0).all() and out.tobytes() == data.tobytes() + data[:5000].tobytes()


@pytest.mark.parametrize("alg", ALGS)
def test_out_of_contract_chunks_store_nothing(cw, O, alg):
    text = np.frombuffer((corpus_file("alice29.txt") + corpus_file("lcet10.txt"))[:250_000], np.uint8)
    n = len(text)
    # out of contract: chunk 1 (empty), 3 (65537 bytes), 5 (decreasing), 6 (75000 bytes), 10 and 11 (past the source)
    cuts = [0, 500, 500, 3000, 3000 + 65537, 80000, 75000, 150000, 160000, 200000, n, n + 5, n + 10]
    k = len(cuts) - 1
    r = Run(cw, alg, text, cuts=cuts).fetch()
    st = Store(n + 64, k + 2)
    st.append(cw, alg, r, base=1)
    verdict, total = st.expect(O, alg, text, cuts, range(k), 1)
    st.check((0, total))
    assert verdict == 0 and np.nonzero(st.x_dir["raw"])[0].tolist() == [1 + i for i in (0, 2, 4, 7, 8, 9)]
    # a selection with an index past the chunk count, and a count below the list; an out-of-contract chunk whose value would
    # lie outside the directory does not refuse the call
    cuts2, sel = cuts[:5] + [80000], [4, 0, 7, 2, 1 << 31]
    r = Run(cw, alg, text, cuts=cuts2, sel=sel, count=4).fetch()
    st2 = Store(n + 64, 4)
    st2.append(cw, alg, r, base=0)
    verdict, total = st2.expect(O, alg, text, cuts2, sel, 0, count=4)
    st2.check((0, total))
    assert verdict == 0 and np.nonzero(st2.x_dir["raw"])[0].tolist() == [0, 2]
    status, out = restore_store(cw, O, alg, st2, [0, 1, 2, 3], [0, 500, 500, 3000, 3000], 3000)
    assert status[:4].tolist() == [0, 2, 0, 2] and out.tobytes() == text[:3000].tobytes()


# ---- counts on the device -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alg", ALGS)
def test_counts_are_read_on_the_device(cw, O, alg):
    data = np.frombuffer(corpus_file("lcet10.txt")[:120_000] + _noise(10_000, 9), np.uint8)
    cuts = CM.chunk(data, P1K)
    k = len(cuts) - 1
    sel = np.random.default_rng(71).permutation(k)[:k // 2].tolist()
    r = Run(cw, alg, data, cuts=cuts, sel=sel, nsel=10).fetch()     # *d_n_new = 10 < max_chunks = k
    st = Store(len(data), k)
    st.append(cw, alg, r, base=0)
    verdict, total = st.expect(O, alg, data, cuts, sel[:10], 0)
    st.check((0, total))
    assert verdict == 0 and np.count_nonzero(st.x_dir["raw"]) == 10
    r0 = Run(cw, alg, data, cuts=cuts, sel=sel, nsel=0).fetch()     # nothing selected: nothing stored, the result still written
    st.append(cw, alg, r0, base=0)
    st.check((0, 0))
    # no selection, *d_nchunks below max_chunks
    r = Run(cw, alg, data, cuts=cuts, count=k - 5, max_chunks=k).fetch()
    st = Store(len(data), k)
    st.append(cw, alg, r, base=0)
    verdict, total = st.expect(O, alg, data, cuts, range(k - 5), 0, count=k - 5)
    st.check((0, total))
    # restore: *d_count = 20 < max_count; positions, statuses and bytes behind it keep their canaries
    refs = list(range(k - 5))
    status, out = restore_store(cw, O, alg, st, refs, cuts[:k - 4], cuts[k - 5], count=20)
    assert (status[:20] == 0).all() and out[:cuts[20]].tobytes() == data[:cuts[20]].tobytes() and (out[cuts[20]:] == FILL).all()
    status, out = restore_store(cw, O, alg, st, refs, cuts[:k - 4], cuts[k - 5], count=10 ** 12, max_count=7)   # the smaller of the two
    assert (out[cuts[7]:] == FILL).all()
    status, out = restore_store(cw, O, alg, st, refs, cuts[:k - 4], cuts[k - 5], count=0)
    assert (status == -1).all() and (out == FILL).all()


# ---- malformed store and recipe ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alg", ALGS)
def test_malformed_store_and_recipe_get_the_models_statuses(cw, O, alg):
    """Bad input is refused or judged, in the manner of test_gpu_decoders.py; nothing here needs or causes a fault: every access is
    checked against the store, the directory and the extent before it is made."""
    import torch
    rng = np.random.default_rng(83)
    data = np.frombuffer(corpus_file("alice29.txt")[:100_000] + _noise(30_000, 5) + corpus_file("kennedy.xls")[:50_000], np.uint8)
    cuts = CM.chunk(data, P1K)
    k = len(cuts) - 1
    r = Run(cw, alg, data, cuts=cuts).fetch()
    st = Store(len(data), k + 4)
    st.append(cw, alg, r, base=0)
    assert st.expect(O, alg, data, cuts, range(k), 0)[0] == 0
    st.check()
    good = st.x_dir.copy()
    comp = [i for i in range(k) if not good[i]["raw"] & RM.RAW]
    raws = [i for i in range(k) if good[i]["raw"] & RM.RAW]
    assert len(comp) >= 40 and len(raws) >= 20
    decode = O.lz4_decompress if alg == "lz4" else O.lzf_decompress

    # (1) a damaged directory over the good store bytes; the recipe names every chunk in order, then a few refs that name nothing
    bad = good.copy()
    c, w = iter(rng.permutation(comp).tolist()), iter(rng.permutation(raws).tolist())
    used = st.x_used
    for i in (next(c), next(w)):
        bad["pos"][i] = st.store_bytes - int(bad["stored"][i]) + 1     # the extent ends one byte past the store
    for i in (next(c), next(w)):
        bad["pos"][i] = 1 << 63
    bad["pos"][next(c)] = 2 ** 64 - 1                                   # pos + stored wraps
    for i in (next(c), next(c), next(c)):
        bad["stored"][i] += int(rng.integers(1, 5))                     # grown: bytes of the next chunk behind the stream
    for i in (next(c), next(c), next(c)):
        bad["stored"][i] -= min(int(rng.integers(1, 5)), int(bad["stored"][i]) - 1)   # shrunk
    bad["stored"][next(c)] = 0xFFFFFFFF
    bad["stored"][next(c)] = 0
    bad["stored"][next(w)] = 0
    bad["stored"][next(w)] -= 1                                         # a raw entry with stored != length
    for i in (next(c), next(c), next(w), next(w), next(w)):
        bad["raw"][i] ^= RM.RAW                                         # the flag flipped, both ways
    for i in (next(c), next(w)):
        bad["raw"][i] += 1                                              # the length changed
    for i in (next(c), next(w)):
        bad["raw"][i] -= 1
    bad["raw"][next(c)] |= 1 << 20                                      # a reserved bit
    bad[next(c)] = (0, 0, 0)                                            # an entry wiped
    refs = list(range(k)) + [k + 1, k + 4, k + 5, RM.MISS, 2 ** 63]     # an empty entry, out of range by 0 and by 1, a miss
    raw = cuts + [cuts[-1] + 10 * (j + 1) for j in range(5)]
    dst_bytes = raw[-1]
    d_dir = torch.from_numpy(bad.view(np.int64).copy()).cuda()
    status, out = restore_call(cw, alg, st.d_store, st.store_bytes, d_dir.data_ptr(), 0, k + 4, refs, raw, dst_bytes)
    want = RM.restore(st.x_store, st.store_bytes, bad, 0, refs, raw, dst_bytes, decode)
    check_restore(status, out, want, raw, dst_bytes)
    got = [s for s, _ in want]
    assert got.count(2) >= 20 and got.count(1) >= 3 and got.count(0) > k - 40

    # (2) a bad recipe over the good store: extents that are decreasing, too long, past the destination, of another length
    refs = [0, 1, 2, 3, 4, 5]
    l = [cuts[i + 1] - cuts[i] for i in range(6)]
    raw = [0, l[0], l[0] + l[1] + 1, l[0] + l[1] + 1 + l[2], 70000, 69000, 69000 + l[5]]
    status, out = restore_call(cw, alg, st.d_store, st.store_bytes, st.d_dir, 0, k + 4, refs, raw, 69000 + l[5] - 1)
    want = RM.restore(st.x_store, st.store_bytes, good, 0, refs, raw, 69000 + l[5] - 1, decode)
    check_restore(status, out, want, raw, 69000 + l[5] - 1)
    assert [s for s, _ in want] == [0, 2, 0, 2, 2, 2]

    # (3) damaged stored bytes: the builders' edits of stored streams, appended behind the store's bytes, one entry each
    edits_of = LS.lz4_edits if alg == "lz4" else LS.lzf_edits
    parse = LS.lz4_parse if alg == "lz4" else LS.lzf_parse
    blob, entries, recipe = bytearray(st.x_store[:used].tobytes()), [], []
    for i in rng.permutation(comp)[:30].tolist():
        pos, stored, word = (int(v) for v in good[i])
        stream = bytes(st.x_store[pos:pos + stored])
        for _, damaged in list(LS._random_edits(stream, rng)) + list(edits_of(parse(stream), word & RM.LEN_MASK, rng)):
            if damaged:
                entries.append((len(blob), len(damaged), word))
                recipe.append(word & RM.LEN_MASK)
                blob += damaged
    d2 = np.array(entries, RM.LOC)
    raw = np.concatenate([[0], np.cumsum(recipe)]).tolist()
    refs = [50 + j for j in range(len(entries))]                        # dir_base = 50
    d_store = torch.from_numpy(np.frombuffer(bytes(blob), np.uint8).copy()).cuda()   # the store ends with its last stream
    d_dir = torch.from_numpy(d2.view(np.int64).copy()).cuda()
    status, out = restore_call(cw, alg, d_store.data_ptr(), len(blob), d_dir.data_ptr(), 50, len(entries), refs, raw, raw[-1])
    want = RM.restore(blob, len(blob), d2, 50, refs, raw, raw[-1], decode)
    check_restore(status, out, want, raw, raw[-1])
    got = [s for s, _ in want]
    assert len(got) > 200 and got.count(1) > len(got) // 3 and 2 not in got


# ---- two host threads on one stream --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alg", ALGS)
def test_two_threads_on_one_stream_store_exactly(cw, O, alg):
    """The launch lock of the stream's scratch keeps one call's flags, sizes and offsets together: both threads' calls share them."""
    import torch
    inputs = [np.frombuffer(corpus_file("lcet10.txt")[:200_000], np.uint8),
              np.frombuffer(corpus_file("kennedy.xls")[:150_000] + _noise(30_000, 11), np.uint8)]
    cuts = [CM.chunk(inputs[0], P1K), CM.chunk(inputs[1], CM.params(64, 256, 1024, CM.top_bits(10), CM.top_bits(6)))]
    runs = [Run(cw, alg, inputs[t], cuts=cuts[t]).fetch() for t in range(2)]
    calls, stream = 6, _stream()
    stores = [Store(calls * len(inputs[t]) + 64, calls * (len(cuts[t]) - 1)) for t in range(2)]
    torch.cuda.synchronize()
    gate = threading.Barrier(2)

    def work(t):
        cw.init(0)
        gate.wait()
        for c in range(calls):
            stores[t].append(cw, alg, runs[t], base=c * (len(cuts[t]) - 1), stream=stream)

    threads = [threading.Thread(target=work, args=(t,)) for t in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    torch.cuda.synchronize()
    for t in range(2):
        k = len(cuts[t]) - 1
        for c in range(calls):
            assert stores[t].expect(O, alg, inputs[t], cuts[t], range(k), c * k)[0] == 0
        stores[t].check()
        refs = [(calls - 1) * k + i for i in range(k)]
        status, out = restore_store(cw, O, alg, stores[t], refs, cuts[t], len(inputs[t]))
        assert (status[:k] == 0).all() and out.tobytes() == inputs[t].tobytes()
