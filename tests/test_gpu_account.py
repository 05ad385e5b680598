"""The account call on the GPU (cw_dev_store_account, cw.ChunkStore.account / affected) against the numpy model of
tests/account_model.py, byte for byte, and against the dry run of cw_dev_store_compact on a real store.

Device buffers carry canaries: every output buffer is prefilled with FILL, has guard words behind it and is compared whole.  The
directory sizes and the position counts are the edges of a wavefront (64), of a workgroup (256) and of a multiple of both."""
import numpy as np
import pytest

import account_model as AM
import store_gc_model as GM
from conftest import corpus_file
from test_gpu_chunk_codec import _dev_u64, _stream, _u64
from test_gpu_renumber import hand_directory

pytestmark = pytest.mark.gpu
FILL = 0xA5
POISON = 0xA5A5A5A5A5A5A5A5
G = 4                   # guard records / words behind every output
ALGS = ["lz4", "lzf"]
SIZES = [1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 8193]
M = AM.M
MISS = M - 1            # CW_DEDUPE_MISS


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


def _fill(nbytes):
    import torch
    return torch.full((nbytes,), FILL, dtype=torch.uint8, device="cuda")


# ---- 1. hand-built directories and refs ------------------------------------------------------------------------------------------
def account_call(cw, refs, first, d, dir_base, flag, refcount=True, owner=True, max_positions=None, stream=None, tail=None):
    """One cw_dev_store_account into poisoned buffers, compared whole with the model; returns (the model's result, the outputs'
    bytes).  d_ref holds max_positions words: the refs, then `tail` (default: a value that names entry 0) up to max_positions."""
    import torch
    first = np.asarray(first, np.uint64)
    nstreams, entries = len(first) - 1, len(d)
    max_positions = len(refs) if max_positions is None else max_positions
    want = AM.account_np(refs, first, d, dir_base, flag, max_positions)
    behind = np.full(max(max_positions - len(refs), 0), dir_base % M if tail is None else tail, np.uint64)
    d_ref = _dev_u64(np.concatenate([np.asarray(refs, np.uint64), behind, np.zeros(1, np.uint64)])[:max(max_positions, 1)])
    d_first, d_dir, d_flag = _dev_u64(first), _dev(d), None if flag is None else _dev(np.asarray(flag, np.uint32))
    acct, totals = _fill((nstreams + G) * 64), _fill((8 + G) * 8)
    rc, ow = _fill((entries + G) * 4), _fill((entries + G) * 4)
    torch.cuda.synchronize()
    cw.dev_store_account(d_ref.data_ptr() if max_positions else 0, d_first.data_ptr(), nstreams, max_positions, d_dir.data_ptr(), dir_base,
                         entries, 0 if flag is None else d_flag.data_ptr(), acct.data_ptr(), rc.data_ptr() if refcount else 0,
                         ow.data_ptr() if owner else 0, totals.data_ptr(), _stream() if stream is None else stream)
    torch.cuda.synchronize()
    got = (acct.cpu().numpy(), rc.cpu().numpy(), ow.cpu().numpy(), totals.cpu().numpy())
    assert d_dir.cpu().numpy().tobytes() == d.tobytes() and _u64(d_first).tobytes() == first.tobytes(), "an input was written"
    a, r, o, t = got[0].view(np.uint64), got[1].view(np.uint32), got[2].view(np.uint32), got[3].view(np.uint64)
    assert (t[8:] == POISON).all() and (a[nstreams * 8:] == POISON).all(), "guards behind d_totals / d_acct"
    assert (r[entries:] == 0xA5A5A5A5).all() and (o[entries:] == 0xA5A5A5A5).all(), "guards behind d_refcount / d_owner"
    if want[0]:
        assert t[0] == 1 and (t[1:] == POISON).all(), t
        assert (got[0] == FILL).all() and (got[1] == FILL).all() and (got[2] == FILL).all(), "a refused call wrote an output buffer"
        return want, got
    _, streams, want_rc, want_ow, want_t = want
    assert t[:8].tolist() == want_t, (t[:8].tolist(), want_t)
    body = a[:nstreams * 8].view(AM.ACCOUNT)
    bad = np.nonzero(body != streams)[0]
    assert len(bad) == 0, ("stream", int(bad[0]), body[bad[0]], streams[bad[0]], len(bad))
    for on, x, y, what in ((refcount, r, want_rc, "refcount"), (owner, o, want_ow, "owner")):
        if on:
            bad = np.nonzero(x[:entries] != y)[0]
            assert len(bad) == 0, (what, int(bad[0]), int(x[bad[0]]), int(y[bad[0]]), len(bad))
        else:
            assert (x == 0xA5A5A5A5).all(), f"a NULL {what} was written"
    return want, got


def shapes(n):
    """name -> d_first of n positions"""
    row = np.concatenate([[0], np.cumsum(np.tile([1, 63, 64, 65], n // 193 + 1))])
    out = {"one": [0, n], "row": np.concatenate([row[row < n], [n]])}
    for k in (257, 4097):
        rng = np.random.default_rng(k + n)
        cuts = np.sort(rng.choice(np.arange(n + 1), min(7, n + 1), replace=False))       # at most 8 streams with positions
        f = np.sort(np.concatenate([cuts, rng.choice(cuts, k - 1 - len(cuts))]))
        f[:3], f[-3:] = 0, n                                                               # empty streams first and last
        out[f"sparse{k}"] = np.concatenate([[0], f, [n]])
    return out


def hand_refs(n, entries, dir_base, seed):
    """Values all over the directory, a third of them in one corner of it so that entries are named often and by several streams,
    with the values that name nothing mixed in: below the base, one past the directory, CW_DEDUPE_MISS."""
    rng = np.random.default_rng(seed)
    idx = np.where(rng.random(n) < 0.33, rng.integers(0, min(entries, 9), n), rng.integers(0, entries, n))
    refs = (np.uint64(dir_base % M) + idx.astype(np.uint64))                               # wraps in u64
    odd = rng.random(n)
    refs[odd < 0.03] = (dir_base - 1) % M
    refs[(odd >= 0.03) & (odd < 0.06)] = (dir_base + entries) % M
    refs[(odd >= 0.06) & (odd < 0.09)] = MISS
    return refs


def hand_flag(entries, seed):
    rng = np.random.default_rng(seed)
    return (rng.random(entries) < 0.3).astype(np.uint32) * rng.integers(1, 1 << 32, entries, dtype=np.uint64).astype(np.uint32)


@pytest.mark.parametrize("n", SIZES)
def test_hand_built_positions(cw, n):
    """n positions over a directory of 257 and one of 8193 entries, every stream shape, a base near 2^64 so that the subtraction wraps"""
    seen = set()
    for entries, dir_base in ((257, M - 100), (8193, 5)):
        d = hand_directory(entries, 300 + entries, True)
        flag = hand_flag(entries, n)
        for name, first in shapes(n).items():
            refs = hand_refs(n, entries, dir_base, n + len(first))
            (_, streams, _, owner, totals), _ = account_call(cw, refs, first, d, dir_base, flag if name != "row" else None)
            seen |= {"shared"} if (owner == AM.SHARED).any() else set()
            seen |= {"missing"} if totals[7] else set()
            assert int(streams["positions"].sum()) == n
    assert n < 63 or seen == {"shared", "missing"}


@pytest.mark.parametrize("entries", SIZES)
def test_hand_built_directories(cw, entries):
    """a directory of `entries` entries, dense and sparse, named by 4097 positions; each of d_refcount and d_owner NULL alone and both"""
    n = 4097
    for sparse, dir_base in ((False, 1 << 40), (True, M - entries)):       # (dir_base + entries == 2^64: the last value is 2^64 - 1)
        d = hand_directory(entries, 400 + entries, sparse)
        for k, (name, first) in enumerate(shapes(n).items()):
            refs = hand_refs(n, entries, dir_base, entries + k)
            account_call(cw, refs, first, d, dir_base, hand_flag(entries, k) if k % 2 else None, refcount=k != 1, owner=k != 2)
    account_call(cw, refs, first, d, dir_base, None, refcount=False, owner=False)


def test_every_stream_empty(cw):
    d = hand_directory(257, 1, True)
    for nstreams in (1, 64, 257):
        (v, streams, refcount, owner, totals), _ = account_call(cw, np.zeros(0, np.uint64), np.zeros(nstreams + 1, np.uint64), d, 5, None)
        assert v == 0 and not streams.view(np.uint64).any() and not refcount.any() and (owner == AM.NONE).all()
        assert totals[1] == int(AM.account_np([], [0, 0], d, 5, None)[4][1]) > 0 and totals[3:] == [0] * 5
    # no positions allowed at all: d_ref is NULL
    account_call(cw, np.zeros(0, np.uint64), [0, 0, 0], d, 5, hand_flag(257, 2), max_positions=0)


@pytest.mark.parametrize("zero", [False, True])
def test_one_hot_entry(cw, zero):
    """all 8193 positions name one entry, from one stream and from two; the same with the hot entry all zero"""
    n, entries, hot = 8193, 300, 77
    d = hand_directory(entries, 9, False)
    if zero:
        d[hot] = (0, 0, 0)
    refs, flag = np.full(n, 1000 + hot, np.uint64), np.ones(entries, np.uint32)
    length, stored = int(d[hot]["raw"]) & AM.LEN_MASK, int(d[hot]["stored"])
    for first, who in (([0, 0, n, n], 1), ([0, 5000, 5000, n], AM.SHARED)):
        (_, streams, refcount, owner, totals), _ = account_call(cw, refs, first, d, 1000, flag)
        if zero:
            assert totals[7] == n and totals[3] == 0 and (owner == AM.NONE).all() and not refcount.any()
            assert int(streams["missing"].sum()) == n and not streams["logical_bytes"].any() and not streams["flagged_positions"].any()
            continue
        assert owner[hot] == who and refcount[hot] == n and totals[3:] == [1, stored, who == AM.SHARED, stored * (who == AM.SHARED), 0]
        assert int(streams["logical_bytes"].sum()) == int(streams["flagged_bytes"].sum()) == n * length
        want = [0, 1, 0] if who == 1 else [0, 0, 0]
        assert streams["unique_chunks"].tolist() == want and streams["unique_stored"].tolist() == [stored * w for w in want]


def test_positions_behind_the_count_are_not_read(cw):
    """*d_first[nstreams] below max_positions: the words behind it name a non-zero, flagged entry and enter no count"""
    entries, n = 257, 4097
    d, flag = hand_directory(entries, 3, True), np.ones(entries, np.uint32)
    refs = hand_refs(n, entries, 5, 11)
    for first in shapes(n).values():
        a, _ = account_call(cw, refs, first, d, 5, flag, max_positions=n + 700)
        b, _ = account_call(cw, refs, first, d, 5, flag, max_positions=n + 700, tail=5 + entries - 1)
        assert a[4] == b[4] and a[1].tobytes() == b[1].tobytes()
    full, _ = account_call(cw, np.concatenate([refs, np.full(700, 5, np.uint64)]), [0, n + 700], d, 5, flag)
    assert full[4] != a[4]                                                   # the tail would have counted


@pytest.mark.parametrize("n", [1, 65, 4097])
def test_verdict_one_changes_nothing(cw, n):
    entries = 257
    d, flag = hand_directory(entries, 4, True), hand_flag(entries, 4)
    refs = hand_refs(n + 1, entries, 5, 12)
    for first in shapes(n).values():
        first = np.asarray(first, np.uint64)
        assert account_call(cw, refs[:n], first, d, 5, flag)[0][0] == 0
        assert account_call(cw, refs, first + np.uint64(1), d, 5, flag)[0][0] == 1             # d_first[0] != 0
        assert account_call(cw, refs[:n], first, d, 5, flag, max_positions=n - 1)[0][0] == 1   # n > max_positions
        for at in {1, len(first) // 2, len(first) - 2} - {0}:                                  # a pair decreases: front, middle, back
            if at + 1 < len(first):
                down = first.copy()
                down[at] = down[at + 1] + np.uint64(1)
                assert account_call(cw, refs, down, d, 5, flag)[0][0] == 1, at
    one = np.array([0, 3, 2], np.uint64)                                                       # ... and the last pair of all
    assert account_call(cw, refs, one, d, 5, flag, max_positions=8)[0][0] == 1


def test_two_streams_give_identical_bytes(cw):
    import torch
    entries, n = 4097, 8193
    d, flag = hand_directory(entries, 6, True), hand_flag(entries, 6)
    refs = hand_refs(n, entries, 5, 13)
    first = shapes(n)["row"]
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    _, a = account_call(cw, refs, first, d, 5, flag, stream=s1.cuda_stream)
    _, b = account_call(cw, refs, first, d, 5, flag, stream=s2.cuda_stream)
    _, c = account_call(cw, refs, first, d, 5, flag, stream=s1.cuda_stream)
    assert all(x.tobytes() == y.tobytes() == z.tobytes() for x, y, z in zip(a, b, c))


# ---- 2. a real store -------------------------------------------------------------------------------------------------------------
def _three(cw, alg):
    a, b, c = GM.three_streams(corpus_file("alice29.txt"), corpus_file("kennedy.xls"))
    idx = cw.DedupeIndex("skein512", 2048)
    cs = cw.ChunkStore(idx, alg, cw.CdcParams.default(1024), 1 << 20, 512, dir_base=40)
    return cs, (a, b, c), tuple(cs.ingest_many([a, b, c]))


def dry_run(cw, cs, recipes):
    """(needed bytes, kept, dropped) of cw_dev_store_compact's dry run after marking `recipes`"""
    import torch
    n, s = cs.dir_entries, _stream()
    live, n_out = torch.zeros(n, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda")
    new_used, new_dir = torch.zeros(1, dtype=torch.int64, device="cuda"), torch.zeros(n * 2, dtype=torch.int64, device="cuda")
    result = torch.zeros(4, dtype=torch.int64, device="cuda")
    marks = [(_dev_u64(r.refs), _dev_u64([len(r.refs)]), len(r.refs)) for r in recipes]           # (kept alive until the calls have run)
    torch.cuda.synchronize()
    for d_ref, d_count, k in marks:
        cw.dev_store_mark(d_ref.data_ptr(), d_count.data_ptr(), k, cs.dir_base, n, live.data_ptr(), n_out.data_ptr(), s)
    cw.dev_store_compact(cs.d_store.data_ptr(), cs.store_bytes, cs.d_dir.data_ptr(), n, live.data_ptr(), 0, 0, new_used.data_ptr(),
                         new_dir.data_ptr(), result.data_ptr(), s)
    torch.cuda.synchronize()
    verdict, needed, kept, dropped = _u64(result).tolist()
    assert verdict == 1 and int(n_out.item()) == 0
    return needed, kept, dropped


@pytest.mark.parametrize("alg", ALGS)
def test_account_against_the_compact_dry_run(cw, alg):
    cs, datas, recipes = _three(cw, alg)
    with cs.index:
        assert cs.account([]).streams.shape == (0,) and cs.account([]).totals["referenced"] == 0
        acc = cs.account(recipes)
        t = acc.totals
        assert isinstance(acc, cw.Account) and acc.streams.dtype == cw.ACCOUNT_DTYPE and len(acc.streams) == 3
        needed, kept, dropped = dry_run(cw, cs, recipes)
        assert (t["referenced_stored"], t["referenced"], t["unreferenced_entries"]) == (needed, kept, dropped)
        assert t["unreferenced_stored"] == 0 and t["missing"] == 0 and t["nonzero_stored"] == t["referenced_stored"]
        # the statement the feature exists for: what dropping one stream gives back
        for r in range(3):
            others = [x for i, x in enumerate(recipes) if i != r]
            assert dry_run(cw, cs, others)[0] == t["referenced_stored"] - int(acc.streams[r]["unique_stored"]), r
            assert dry_run(cw, cs, others)[1] == t["referenced"] - int(acc.streams[r]["unique_chunks"]), r
        assert all(acc.streams["unique_chunks"][1:] > 0)                  # the chunks around each edit (the first stream has no edit)
        for i, (r, data) in enumerate(zip(recipes, datas)):
            assert int(acc.streams[i]["logical_bytes"]) == r.nbytes == len(data) and int(acc.streams[i]["missing"]) == 0
            assert int(acc.streams[i]["positions"]) == len(r.refs)
            alone = cs.account([r])
            assert int(alone.streams[0]["unique_chunks"]) == len(np.unique(r.refs)) == alone.totals["referenced"]
            assert alone.totals["shared"] == 0 and set(alone.owner.tolist()) == {0, cw.Account.NONE}
        assert int(acc.refcount.sum()) == sum(len(r.refs) for r in recipes)
        # forget the second stream: its own chunks are missing now, and nothing is unreferenced
        ra, rb, rc = recipes
        gone = int((acc.owner[(rb.refs - np.uint64(cs.dir_base)).astype(np.int64)] == 1).sum())
        assert gone > 0 and cs.compact([ra, rc])["dropped"] == int(acc.streams[1]["unique_chunks"])
        after = cs.account(recipes)
        assert after.streams["missing"].tolist() == [0, gone, 0] and after.totals["missing"] == gone
        assert after.totals["unreferenced_entries"] == 0 and after.totals["referenced"] == t["referenced"] - int(acc.streams[1]["unique_chunks"])
        assert int(after.streams[1]["logical_bytes"]) < rb.nbytes
        # renumber: the translated recipes account as before, owner and refcount move with the values
        before = cs.account([ra, rc])
        old_base = cs.dir_base
        na, nc = cs.renumber([ra, rc], dir_base=7)
        now = cs.account([na, nc])
        assert now.streams.tobytes() == before.streams.tobytes() and now.totals == before.totals
        old = (np.concatenate([ra.refs, rc.refs]) - np.uint64(old_base)).astype(np.int64)
        new = (np.concatenate([na.refs, nc.refs]) - np.uint64(7)).astype(np.int64)
        assert np.array_equal(now.owner[new], before.owner[old]) and np.array_equal(now.refcount[new], before.refcount[old])
        rest = np.setdiff1d(np.arange(cs.dir_entries), new)
        assert (now.owner[rest] == cw.Account.NONE).all() and not now.refcount[rest].any()
        with pytest.raises(ValueError):
            cs.account([na], flagged=np.zeros(3, np.uint32))


@pytest.mark.parametrize("alg", ALGS)
def test_affected_streams(cw, alg):
    cs, _, recipes = _three(cw, alg)
    ra, rb, rc = recipes
    with cs.index, cw.DedupeIndex("skein512", 2048) as idx2:
        peer = cw.ChunkStore(idx2, alg, cw.CdcParams.default(1024), 1 << 20, 512)
        cs.replicate_to(peer, recipes)
        clean = cs.scrub()
        assert clean.clean and cs.affected(recipes, clean) == []
        # a chunk the first and the third stream share and the second does not have
        acc = cs.account(recipes)
        both = np.setdiff1d(np.intersect1d(ra.refs, rc.refs), rb.refs)
        assert len(both) > 0
        value = int(both[0])
        assert acc.owner[value - cs.dir_base] == cw.Account.SHARED
        entry = cs.d_dir.cpu().numpy().view(cw.LOC_DTYPE)[value - cs.dir_base]
        cs.d_store[int(entry["pos"]) + int(entry["stored"]) // 2] ^= 0x5C
        report = cs.scrub()
        assert report.damaged.tolist() == [value]
        want = []
        for i, r in enumerate(recipes):
            hit = np.isin(r.refs, report.damaged)
            if hit.any():
                want.append((i, int(hit.sum()), int(np.diff(r.offsets.astype(np.int64))[hit].sum())))
        assert [w[0] for w in want] == [0, 2] and cs.affected(recipes, report) == want
        # the same through a plain flag array with values other than 1
        flags = np.zeros(cs.dir_entries, np.uint32)
        flags[value - cs.dir_base] = 0x80000000
        hurt = cs.account(recipes, flagged=flags).streams
        assert [(i, int(a["flagged_positions"]), int(a["flagged_bytes"])) for i, a in enumerate(hurt) if a["flagged_positions"]] == want
        assert cs.repair_from(peer, report)["repaired"] == [value]
        again = cs.scrub()
        assert again.clean and cs.affected(recipes, again) == []
