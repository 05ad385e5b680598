"""One damaged directory entry through every call that follows an entry: cw_dev_restore_chunks, cw_dev_read_ranges,
cw_dev_store_compact, cw_dev_store_export_chunks, cw_dev_store_import_chunks (the entry as an in_loc) and cw_dev_store_verify.
The kernels share one spelling of the entry's soundness rule (csrc/store_device.h), to which restore adds the term that needs the
recipe; read_kernels.hip keeps a second spelling for its speed, and this test holds the two together.  Every output buffer is compared whole, through the helpers and the plain-Python models the calls' own tests use: the calls
treat an all-zero entry differently by design, and the models say how.

The store holds 65 chunks: one full trip of the kernels' 64-lane loops and a second trip of one lane."""
from types import SimpleNamespace

import numpy as np
import pytest

import cdc_model as CM
import read_model as RD
import restore_model as RM
import store_gc_model as GM
from conftest import corpus_file
from test_gpu_read import _around, check_read, packed, read_call
from test_gpu_replicate import HAND_BASE, _dev, check_exported, check_imported, export_call, import_call, model_export, model_import
from test_gpu_restore import check_restore, restore_call
from test_gpu_scrub import View, check as check_scrub
from test_gpu_store_gc import Target, _unsound, check_compacted, check_unchanged, compact_call

pytestmark = pytest.mark.gpu
ALGS = ["lz4", "lzf"]
P1K = CM.default_params(1024)
CHUNKS = 65
DAMAGES = ["pos = store_bytes", "one byte past the store", "pos + stored wraps", "a reserved bit", "stored = 0", "raw with stored != length",
           "length above 65536", "length 0, only pos set", "all zero"]


@pytest.fixture(scope="module")
def cw():
    import torch  # noqa: F401  (one HIP runtime for torch and libcwhc.so)
    import compute_war_amd as cw
    cw.init(0)
    yield cw
    cw.tune_reset()


def _data():
    """Text with slices of random bytes inside (chunks of both stored forms), cut off behind its 65th chunk."""
    text, rng = corpus_file("alice29.txt"), np.random.default_rng(65)
    data = text[:9000] + rng.bytes(7000) + text[9000:40000] + rng.bytes(5000) + text[40000:120000]
    return data[:CM.chunk(data, P1K)[CHUNKS]]


@pytest.fixture(scope="module")
def stores(cw):
    """Per codec, built once: the store on the device (a View the test edits), its image on the host, the recipe and the damages."""
    data, made = _data(), {}

    def get(alg):
        if alg not in made:
            index = cw.DedupeIndex("skein", 4096)
            cs = cw.ChunkStore(index, alg, cw.CdcParams.default(1024), len(data) + 64, CHUNKS + 2, HAND_BASE)
            recipe = cs.ingest(data)
            v = View(cs)
            h = SimpleNamespace(d_store=v.d_store, d_dir=v.d_dir, store_bytes=v.store_bytes, n=v.n, store=v.d_store.cpu().numpy(),
                                directory=v.directory())
            refs, cuts = recipe.refs.tolist(), recipe.offsets.tolist()
            assert refs == [HAND_BASE + j for j in range(CHUNKS)] and cuts == CM.chunk(data, P1K) and cuts[-1] == len(data)
            lens = np.diff(cuts)
            assert 200 <= lens.min() and lens.max() <= 8192
            # the damaged entries are inner positions, so that ranges on both sides of them exist
            inner = np.zeros(h.n, np.uint32)
            inner[2:CHUNKS - 3] = 1
            damages = _unsound(h, inner)
            damages.append(("all zero", damages[0][1], (0, 0, 0)))
            assert [name for name, _, _ in damages] == DAMAGES
            kinds = {bool(int(h.directory[i]["raw"]) & RM.RAW) for _, i, _ in damages}
            assert kinds == {True, False}, "one stored form is missing"
            made[alg] = SimpleNamespace(cs=cs, v=v, h=h, data=data, refs=refs, cuts=cuts, damages=damages)
        return made[alg]
    yield get
    for s in made.values():
        s.cs.index.close()


@pytest.mark.parametrize("damage", range(len(DAMAGES)), ids=[d.replace(" ", "_") for d in DAMAGES])
@pytest.mark.parametrize("alg", ALGS)
def test_one_damaged_entry_through_every_consumer(cw, oracle, stores, alg, damage):
    s = stores(alg)
    v, h, refs, cuts, n = s.v, s.h, s.refs, s.cuts, len(s.data)
    name, i, entry = s.damages[damage]
    decode = oracle.lz4_decompress if alg == "lz4" else oracle.lzf_decompress
    bad = h.directory.copy()
    bad[i] = entry
    src = (v.d_store.data_ptr(), h.store_bytes, v.d_dir.data_ptr(), HAND_BASE, h.n)
    v.set_entry(i, entry)
    try:
        # restore: the whole stream
        status, out = restore_call(cw, alg, *src, refs, cuts, n)
        want = RM.restore(h.store, h.store_bytes, bad, HAND_BASE, refs, cuts, n, decode)
        check_restore(status, out, want, cuts, n)
        assert [st for st, _ in want].count(2) == 1 and want[i][0] == 2, name
        assert all(piece == s.data[cuts[j]:cuts[j + 1]] for j, (st, piece) in enumerate(want) if st == 0)

        # read: ranges that cover the chunk whole, ranges that cut into it, and ranges beside it
        near, beside = _around(cuts, i)
        ranges, dst_bytes = packed(near + beside + [(0, n)], gap=1)
        status, out = read_call(cw, alg, src, refs, cuts, ranges, dst_bytes)
        want = RD.read(h.store, h.store_bytes, bad, HAND_BASE, refs, cuts, ranges, dst_bytes, decode)
        check_read(status, out, want, ranges, dst_bytes)
        got = [st for st, _ in want]
        assert got == [2] * len(near) + [0] * len(beside) + [2], name

        # compact: the entry kept, and the entry unmarked
        live = np.ones(h.n, np.uint32)
        for flags in (live, np.where(np.arange(h.n) == i, 0, live).astype(np.uint32)):
            model = GM.compact(h.store, h.store_bytes, bad, flags, h.store_bytes)
            got = compact_call(cw, h, v.d_dir, flags, Target(h.store_bytes, h.n))
            if model[0]:
                check_unchanged(got, h.n, model[1])
            else:
                check_compacted(got, model)

        # export: the entry named, and every other entry
        values = np.asarray(refs, np.uint64)
        for named in (values, values[values != HAND_BASE + i]):
            model = model_export(h, named, h.store_bytes, directory=bad)
            assert model[0] == (2 if len(named) == CHUNKS else 0), name
            check_exported(export_call(cw, h, named, h.store_bytes, d_dir=v.d_dir), model, len(named) if model[0] == 0 else 0)

        # import: the store as a bundle's payload, the directory's entries as its in_locs
        b = SimpleNamespace(payload=h.store.tobytes(), d_in=v.d_store, n=CHUNKS, locs=h.directory[:CHUNKS].copy(), d_loc=None)
        locs = bad[:CHUNKS].copy()
        for sel in (None, [k for k in range(CHUNKS) if k != i]):
            model = model_import(b, sel, 50, 1003, 1003 + n, 40, 100, locs=locs)
            assert model[0] == (3 if sel is None else 0), name
            check_imported(import_call(cw, b, sel, 50, 1003, 1003 + n, 40, 100, d_loc=_dev(locs)), model, 1003, 100)

        # scrub
        status = check_scrub(cw, oracle, v, "skein")
        assert int((status == 0).sum()) == CHUNKS - 1, name
    finally:
        v.set_entry(i, tuple(int(x) for x in h.directory[i]))
    assert v.d_dir.cpu().numpy().tobytes() == h.directory.tobytes() and v.d_store.cpu().numpy().tobytes() == h.store.tobytes()
