"""The pipelined ingest of many host streams on the GPU (cw_store_ingest_streams, cw_dev_ingest_commit_streams,
ChunkStore.ingest_many_stream / restore_many_stream) against the piecewise model of tests/streams_ingest_model.py, against
ChunkStore.ingest_many of the same streams into a fresh index and store, and against a loop of ChunkStore.ingest: the recipes, the store
bytes [0, used), the directory, the index's count, base and the statistics must all be equal.

The inputs, their pieces and the limits of the refusal cases come from tests/test_streams_ingest_abi.py, which establishes from the
model that each input reaches its edge."""
import ctypes as C

import numpy as np
import pytest

import ingest_model as IM
import restore_model as RM
import streams_ingest_model as XM
from test_ingest_abi import dups
from test_streams_ingest_abi import ALGS, BIG, CASES, P1K, REFUSED, expected, refusal, streams_of

pytestmark = pytest.mark.gpu
NOMEM = -5
CANARY = 0x5A5A5A5A5A5A5A5A


@pytest.fixture(scope="module")
def cw():
    import torch  # noqa: F401  (one HIP runtime for torch and libcwhc.so)
    import compute_war_amd as cw
    cw.init(0)
    yield cw
    cw.tune_reset()


def _params(cw, p: dict):
    return cw.CdcParams(p["min"], p["avg"], p["max"], p["mask_s"], p["mask_l"], p.get("gear"))


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _dev_u64(values):
    import torch
    return torch.from_numpy(np.asarray(values, np.uint64).view(np.int64).copy()).cuda()


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


class Pair:
    """A fresh index with a fresh store."""

    def __init__(self, cw, alg, p, lim=BIG, dir_base=5):
        self.idx = cw.DedupeIndex("skein512", lim["max_entries"])
        self.cs = cw.ChunkStore(self.idx, alg, _params(cw, p), lim["store_bytes"], lim["dir_entries"], dir_base)

    def __enter__(self):
        return self.cs

    def __exit__(self, *exc):
        self.idx.close()


def same_as_model(cs, m: RM.Model):
    used = cs.used()
    assert used == len(m.blob)
    assert cs.d_store[:used].cpu().numpy().tobytes() == bytes(m.blob)
    got = cs.d_dir.cpu().numpy().view(RM.LOC)
    assert len(got) == len(m.directory)
    bad = np.nonzero(got != m.directory)[0]
    assert len(bad) == 0, ("entry", int(bad[0]), got[bad[0]], m.directory[bad[0]], len(bad))
    assert cs.index.count() == len(m.values)


def same_recipes(recipes, want):
    assert len(recipes) == len(want)
    for f, (r, (refs, cuts)) in enumerate(zip(recipes, want)):
        assert r.refs.tolist() == list(refs) and r.offsets.tolist() == list(cuts), f


# ---- every case: the streamed ingest, the model, ingest_many, a loop of ingest ----------------------------------------------------
@pytest.mark.parametrize("alg", ALGS)
@pytest.mark.parametrize("name", sorted(CASES))
def test_ingest_many_stream_equals_the_model_ingest_many_and_a_loop_of_ingest(cw, name, alg):
    _, p, piece = CASES[name]
    streams = streams_of(name)
    run, m = expected(name, alg)
    want = run.recipes()[0]
    with Pair(cw, alg, p) as a, Pair(cw, alg, p) as b, Pair(cw, alg, p) as c:
        with cw.tuned(CW_STORE_PIECE=piece):
            ra = a.ingest_many_stream(streams)
        rb = b.ingest_many(streams)
        rc = [c.ingest(s) for s in streams]
        for got in (ra, rb, rc):
            same_recipes(got, want)
        for cs in (a, b, c):
            same_as_model(cs, m)
        assert a.base == b.base == c.base == 5 + run.nchunks and a.last_stats == run.stats and run.stats["pieces"] == len(run.log)
        with cw.tuned(CW_STORE_PIECE=70001):
            assert a.restore_many_stream(ra) == [bytes(s) for s in streams]
        for f, r in enumerate(ra):
            assert b.restore_stream(r) == bytes(streams[f]), f


@pytest.mark.parametrize("alg", ALGS)
def test_a_second_run_into_the_same_store_references_the_first(cw, alg):
    _, p, piece = CASES["dup_block"]
    first, second = streams_of("dup_block"), list(reversed(streams_of("long_among_small"))) + [streams_of("dup_block")[1]]
    run, m = expected("dup_block", alg)
    m = IM.clone(m)
    with Pair(cw, alg, p) as cs:
        with cw.tuned(CW_STORE_PIECE=piece):
            r1 = cs.ingest_many_stream(first)
            r2 = cs.ingest_many_stream(second)
        want = XM.ingest_streams(m, second, p, piece, 5 + run.nchunks, BIG["max_entries"])
        same_recipes(r1, run.recipes()[0])
        same_recipes(r2, want.recipes()[0])
        same_as_model(cs, m)
        assert cs.last_stats == want.stats and 0 < want.stats["new_chunks"] < want.stats["chunks"]
        assert r2[-1].refs.tolist() == r1[1].refs.tolist() and max(r2[-1].refs.tolist()) < 5 + run.nchunks
        assert cs.restore_many_stream(r1 + r2) == [bytes(s) for s in first + second]


# ---- host memory: page-locked back to back (read in place), pageable and scattered, odd alignments ----------------------------------
@pytest.mark.parametrize("alg", ALGS)
@pytest.mark.parametrize("memory", ["pinned_back_to_back", "pinned_apart", "pageable", "odd"])
@pytest.mark.parametrize("name", ["long_among_small", "empty_on_boundaries"])
def test_source_memory_kinds(cw, name, memory, alg):
    _, p, piece = CASES[name]
    streams = streams_of(name)
    run, m = expected(name, alg)
    lens = [len(s) for s in streams]
    L = cw.lib()
    keep, pinned = [], None
    try:
        if memory.startswith("pinned"):
            gap = 0 if memory == "pinned_back_to_back" else 3
            pinned = L.cw_host_alloc(sum(lens) + gap * len(lens) + 16)
            srcs, at = [], pinned
            for s in streams:
                C.memmove(at, bytes(s), len(s))
                srcs.append(at if len(s) else 0)
                at += len(s) + (gap if len(s) else 0)
        else:
            srcs = []
            for s in streams:
                buf = np.zeros(len(s) + 128, np.uint8)
                shift = (-buf.ctypes.data) % 64 + (1 if memory == "odd" else 0)
                buf[shift:shift + len(s)] = np.frombuffer(bytes(s), np.uint8)
                keep.append(buf)
                srcs.append(buf.ctypes.data + shift if len(s) else 0)
        with Pair(cw, alg, p) as cs:
            with cw.tuned(CW_STORE_PIECE=piece):
                rc, refs, offs, first, consumed, done, stats = cw.store_ingest_streams(cs.index, cs.params, alg, cs._triple(), srcs, lens, 5)
            assert rc == 0 and consumed == sum(lens) and done == len(streams) and stats == run.stats
            assert refs.tolist() == run.refs and offs.tolist() == run.offsets and first.tolist() == run.first
            same_as_model(cs, m)
    finally:
        if pinned:
            L.cw_host_free(pinned)


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def grow(cw, cs, lim):
    """Room made by hand: a larger store and directory with the old contents, a larger index."""
    import torch
    store = torch.zeros(lim["store_bytes"], dtype=torch.uint8, device="cuda")
    store[:cs.store_bytes] = cs.d_store[:cs.store_bytes]
    d = torch.zeros(lim["dir_entries"] * 2, dtype=torch.int64, device="cuda")
    d[:cs.dir_entries * 2] = cs.d_dir
    torch.cuda.synchronize()
    cs.d_store, cs.store_bytes, cs.d_dir, cs.dir_entries = store, lim["store_bytes"], d, lim["dir_entries"]
    cs.index.resize(lim["max_entries"])


@pytest.mark.parametrize("alg", ALGS)
@pytest.mark.parametrize("kind", ["store", "directory", "index"])
def test_a_refused_middle_piece_leaves_a_consistent_resumable_prefix(cw, kind, alg):
    _, p, piece = CASES[REFUSED]
    streams = streams_of(REFUSED)
    data = b"".join(streams)
    run, m, lim, j = refusal(kind, alg)
    full, fm = expected(REFUSED, alg)
    whole, partial = run.recipes()
    with Pair(cw, alg, p, lim) as cs:
        with cw.tuned(CW_STORE_PIECE=piece):
            with pytest.raises(cw.CwError) as e:
                cs.ingest_many_stream(streams)
        err = e.value
        assert err.code == NOMEM and (err.consumed, err.nchunks, err.streams_done) == (run.consumed, run.nchunks, run.streams_done)
        assert 0 < run.consumed < len(data) and 0 < run.streams_done < len(streams)
        same_recipes(err.recipes, whole)
        same_recipes([err.partial], [partial])
        same_as_model(cs, m)
        assert cs.base == 5 + run.nchunks and cs.last_stats == run.stats and run.stats["pieces"] == j
        done = err.streams_done
        assert cs.restore_many_stream(err.recipes + [err.partial]) == [bytes(s) for s in streams[:done]] + [streams[done][:err.partial.nbytes]]
        assert cs.restore(err.partial, verify=True) == streams[done][:err.partial.nbytes]
        # room made, the spans from streams_done on, the first shortened by what was consumed of it: the uninterrupted run
        grow(cw, cs, BIG)
        with cw.tuned(CW_STORE_PIECE=piece):
            rest = cs.ingest_many_stream([streams[done][err.partial.nbytes:]] + streams[done + 1:])
        joined = cw.Recipe(np.concatenate([err.partial.refs, rest[0].refs]),
                           np.concatenate([err.partial.offsets, rest[0].offsets[1:] + np.uint64(err.partial.nbytes)]))
        same_recipes(err.recipes + [joined] + rest[1:], full.recipes()[0])
        same_as_model(cs, fm)
        assert cs.base == 5 + full.nchunks


# ---- cw_dev_ingest_commit_streams on its own ----------------------------------------------------------------------------------------
class Growing:
    """A recipe with its stream index that grows on the device, with canaries behind every array, and its image on the host."""

    def __init__(self, rec_cap, first_cap):
        import torch
        self.rec_cap, self.first_cap = rec_cap, first_cap
        full = lambda n: torch.from_numpy(np.full(n, CANARY, np.uint64).view(np.int64)).cuda()  # noqa: E731
        self.ref, self.off, self.first, self.stats = full(rec_cap + 4), full(rec_cap + 4), full(first_cap + 4), full(12)
        self.stats[:5] = 0
        self.count, self.verdict = _dev_u64([0, CANARY]), _dev_u64([CANARY, CANARY])
        self.x_ref, self.x_off, self.x_first = [CANARY] * (rec_cap + 4), [CANARY] * (rec_cap + 4), [CANARY] * (first_cap + 4)
        self.x_stats, self.x_count = [0] * 5, 0

    def commit(self, cw, refs, offsets, n_dev, max_chunks, n_new, result, stream_off, piece_first, first_stream, skip, rec_cap=None, first_cap=None):
        """One call with the counts on the device; the model's call on the image.  Returns the expected verdict."""
        import torch
        pad = [CANARY] * 3
        self.keep = [_dev_u64(list(refs) + pad), _dev_u64(list(offsets) + pad), _dev_u64([n_dev, CANARY]), _dev_u64([n_new, CANARY]),
                     _dev_u64(list(result) + pad) if result is not None else None, _dev_u64(list(piece_first) + pad)]
        d_ref, d_off, d_n, d_new, d_res, d_first = self.keep
        cap = self.rec_cap if rec_cap is None else rec_cap
        fcap = self.first_cap if first_cap is None else first_cap
        torch.cuda.synchronize()
        cw.dev_ingest_commit_streams(d_ref.data_ptr(), d_off.data_ptr(), d_n.data_ptr(), max_chunks, d_new.data_ptr(),
                                     d_res.data_ptr() if result is not None else 0, stream_off, self.ref.data_ptr(), self.off.data_ptr(),
                                     self.count.data_ptr(), cap, self.stats.data_ptr(), self.verdict.data_ptr(), d_first.data_ptr(),
                                     len(piece_first), first_stream, skip, self.first.data_ptr(), fcap, _stream())
        n = min(n_dev, max_chunks)
        verdict, self.x_count = XM.commit_streams(refs, offsets, n, n_new, result, stream_off, self.x_ref, self.x_off, self.x_count, cap, self.x_stats,
                                                  piece_first, len(piece_first), first_stream, skip, self.x_first, fcap)
        return verdict

    def check(self, verdict):
        import torch
        torch.cuda.synchronize()
        assert _u64(self.verdict).tolist() == [verdict, CANARY]
        assert _u64(self.count).tolist() == [self.x_count, CANARY]
        assert _u64(self.ref).tolist() == self.x_ref and _u64(self.off).tolist() == self.x_off and _u64(self.first).tolist() == self.x_first
        assert _u64(self.stats).tolist() == self.x_stats + [CANARY] * 7


def test_commit_streams_reads_its_counts_on_the_device_and_keeps_inside_its_arrays(cw):
    r = Growing(rec_cap=20, first_cap=8)
    # three streams, the last open with nothing consumed; then its continuation, far into a long run, with a count above max_chunks (clamped)
    assert r.commit(cw, [7, 8, 9], [0, 10, 30, 60], 3, 3, 2, [0, 55], 0, [0, 2, 3], 0, False) == 0
    r.check(0)
    assert r.x_first[:4] == [0, 2, 3, CANARY]
    assert r.commit(cw, [70, 80, 90, 91], [5, 15, 35, 65, 66], 4000, 4, 0, [0, 0], (1 << 40) - 3, [0, 1, 4], 2, True) == 0
    r.check(0)
    assert r.x_first[:5] == [0, 2, 3, 4, 7] and r.x_count == 7
    # an empty piece of one open stream commits its one cut and its entry; a piece of empty streams only
    assert r.commit(cw, [], [9], 0, 4, 0, [0, 0], 1 << 41, [0], 5, False) == 0
    r.check(0)
    assert r.commit(cw, [], [0], 0, 4, 0, None, 1 << 41, [0, 0], 6, False) == 0
    r.check(0)
    assert r.x_first[:8] == [0, 2, 3, 4, 7, 7, 7, 7]
    # exactly full, in the recipe (7 + 12 + 1 = 20) and in the stream index (7 + 1 = 8; the entry of stream 7 is an earlier piece's)
    assert r.commit(cw, list(range(12)), list(range(0, 130, 10)), 12, 12, 1, [0, 3], 100, [0], 7, True) == 0
    r.check(0)
    assert r.x_count == 19 and r.x_stats == [60 + 61 + 0 + 0 + 120, 19, 3, 58, 5]


@pytest.mark.parametrize("why", ["recipe_full", "store_verdict", "index_full", "first_stream_beyond"])
def test_commit_streams_that_is_refused_leaves_every_byte_as_it_was(cw, why):
    r = Growing(rec_cap=9, first_cap=4)
    assert r.commit(cw, [7, 8, 9], [0, 10, 30, 60], 3, 3, 2, [0, 55], 1000, [0, 1], 0, False) == 0
    r.check(0)
    piece = ([1, 2, 3, 4, 5], [0, 1, 2, 3, 4, 5], 5, 5, 5)
    if why == "recipe_full":     # 3 + 5 + 1 = 9 fits, a cap one smaller does not
        assert r.commit(cw, *piece, [0, 9], 0, [0, 2], 2, False, rec_cap=8) == 2
        r.check(2)
    elif why == "store_verdict":
        assert r.commit(cw, *piece, [1, 9], 0, [0, 2], 2, False) == 1
        r.check(1)
    elif why == "index_full":    # 2 + 2 = 4 fits, 2 + 3 and a cap one smaller do not
        assert r.commit(cw, *piece, [0, 9], 0, [0, 2, 5], 2, False) == 3
        r.check(3)
        assert r.commit(cw, *piece, [0, 9], 0, [0, 2], 2, False, first_cap=3) == 3
        r.check(3)
    else:
        assert r.commit(cw, *piece, [0, 9], 0, [0], (1 << 64) - 1, False) == 3
        r.check(3)
    assert r.commit(cw, *piece, [0, 9], 0, [0, 2], 2, False) == 0
    r.check(0)
    assert r.x_ref[:3] == [7, 8, 9] and r.x_first[:4] == [0, 1, 3, 5]


def commit_plain(cw, r: Growing, refs, offsets, n_dev, max_chunks, n_new, result, stream_off):
    """cw_dev_ingest_commit into the recipe of a Growing, on the stream its commit() uses; ingest_model's call on the image."""
    import torch
    pad = [CANARY] * 3
    r.keep = [_dev_u64(list(refs) + pad), _dev_u64(list(offsets) + pad), _dev_u64([n_dev, CANARY]), _dev_u64([n_new, CANARY]),
              _dev_u64(list(result) + pad) if result is not None else None]
    d_ref, d_off, d_n, d_new, d_res = r.keep
    torch.cuda.synchronize()
    cw.dev_ingest_commit(d_ref.data_ptr(), d_off.data_ptr(), d_n.data_ptr(), max_chunks, d_new.data_ptr(), d_res.data_ptr() if result is not None else 0,
                         stream_off, r.ref.data_ptr(), r.off.data_ptr(), r.count.data_ptr(), r.rec_cap, r.stats.data_ptr(), r.verdict.data_ptr(),
                         _stream())
    verdict, r.x_count = IM.commit(refs, offsets, min(n_dev, max_chunks), n_new, result, stream_off, r.x_ref, r.x_off, r.x_count, r.rec_cap, r.x_stats)
    return verdict


def test_plain_and_streams_commits_interleave_on_one_stream_into_one_recipe(cw):
    """One pair of kernels and one launch sequence behind both entry points: plain, streams, plain into one recipe is the two models
    applied in that order, and the plain commits leave the stream index alone."""
    r = Growing(rec_cap=20, first_cap=8)
    assert commit_plain(cw, r, [7, 8, 9], [0, 10, 30, 60], 3, 3, 2, [0, 55], 0) == 0
    r.check(0)
    assert r.x_count == 3 and r.x_first == [CANARY] * 12
    assert r.commit(cw, [70, 80, 90, 91], [5, 15, 35, 65, 66], 4000, 4, 0, [0, 0], (1 << 40) - 3, [0, 1, 4], 2, True) == 0
    r.check(0)
    assert r.x_count == 7 and r.x_first[:5] == [CANARY, CANARY, CANARY, 4, 7]
    assert commit_plain(cw, r, list(range(12)), list(range(0, 130, 10)), 5000, 12, 1, [0, 3], 100) == 0   # exactly full: 7 + 12 + 1 = 20
    r.check(0)
    assert r.x_count == 19 and r.x_off[7:20] == list(range(100, 230, 10)) and r.x_ref[7:19] == list(range(12))
    assert r.x_first[:5] == [CANARY, CANARY, CANARY, 4, 7] and r.x_stats == [60 + 61 + 120, 19, 3, 58, 3]
    # a refused plain commit behind them (19 + 1 + 1 > 20) changes nothing, in the recipe or in the stream index
    assert commit_plain(cw, r, [1], [0, 1], 1, 1, 1, [0, 1], 0) == 2
    r.check(2)


# ---- one stream through both entry points ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alg", ALGS)
def test_both_entry_points_leave_the_same_for_one_stream(cw, alg):
    """cw_store_ingest and cw_store_ingest_streams of one pageable buffer in five pieces of an odd size, with carries: the one piece
    loop with and without the stream index."""
    data = dups()[100000:400000]    # text, a block repeated at short distances, noise, text
    assert len(data) == 300000
    with Pair(cw, alg, P1K) as a, Pair(cw, alg, P1K) as b:
        with cw.tuned(CW_STORE_PIECE=70001):
            ra = a.ingest_stream(data)
            rb, = b.ingest_many_stream([data])
        assert a.last_stats["pieces"] == 5 and 0 < a.last_stats["new_chunks"] < a.last_stats["chunks"] == len(ra.refs)
        assert a.last_stats == b.last_stats
        assert ra.refs.tolist() == rb.refs.tolist() and ra.offsets.tolist() == rb.offsets.tolist() and int(ra.offsets[-1]) == len(data)
        assert a.used() == b.used() > 0 and a.base == b.base == 5 + len(ra.refs)
        assert a.d_dir.cpu().numpy().tobytes() == b.d_dir.cpu().numpy().tobytes()
        assert a.d_store[:a.used()].cpu().numpy().tobytes() == b.d_store[:b.used()].cpu().numpy().tobytes()
        assert a.index.count() == b.index.count()
        with cw.tuned(CW_STORE_PIECE=70001):
            assert a.restore_stream(ra) == data and b.restore_stream(rb) == data
