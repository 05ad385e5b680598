"""The dedupe index's lifecycle calls (cw_dev_dedupe_lookup / _insert / _export, cw_dedupe_resize / _export / _import and the
DedupeIndex methods over them) against the plain-Python model of test_gpu_dedupe.py, restated here with explicit values: a dict
of digest bytes -> first value, walked in block order over every call."""
import numpy as np
import pytest

from conftest import corpus_file, corpus_names

pytestmark = pytest.mark.gpu

CW_ERR_BAD_ARG, CW_ERR_NOMEM = -2, -5
MISS = 2 ** 64 - 1
WIDTHS = [("skein", 16), ("sha256mb", 32), ("skein512", 64)]


@pytest.fixture(scope="module")
def cw():
    import torch  # noqa: F401  (one HIP runtime for torch and libcwhc.so)
    import compute_war_amd as cw
    cw.init(0)
    return cw


class Model:
    """What a sequential CPU loop over each batch gives."""

    def __init__(self):
        self.table = {}

    def insert(self, digests: np.ndarray, values: np.ndarray):
        raw, db = digests.tobytes(), digests.shape[1]
        ref = np.zeros(len(digests), np.uint64)
        new = []
        for i in range(len(digests)):
            k = raw[i * db:(i + 1) * db]
            v = self.table.get(k)
            if v is None:
                v = self.table[k] = int(values[i])
                new.append(i)
            ref[i] = v
        return ref, np.array(new, np.uint32)

    def call(self, digests: np.ndarray, base: int):
        return self.insert(digests, base + np.arange(len(digests), dtype=np.uint64))

    def lookup(self, digests: np.ndarray):
        raw, db = digests.tobytes(), digests.shape[1]
        ref = np.array([self.table.get(raw[i * db:(i + 1) * db], MISS) for i in range(len(digests))], np.uint64)
        return ref, int((ref != MISS).sum())

    def items(self):
        return set(self.table.items())


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _dev(a: np.ndarray):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()


def run_dedupe(idx, digests, base=0, values=None):
    """One cw_dev_dedupe (values None) or cw_dev_dedupe_insert call: (ref[n] u64, new_idx[:n_new] u32)."""
    import torch
    n = len(digests)
    d = _dev(digests)
    ref = torch.full((n,), -1, dtype=torch.int64, device="cuda")
    new_idx = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    n_new = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    if values is None:
        idx.dev_dedupe(d.data_ptr(), n, base, ref.data_ptr(), new_idx.data_ptr(), n_new.data_ptr(), _stream())
    else:
        v = _dev(np.asarray(values, np.uint64))
        idx.dev_insert(d.data_ptr(), v.data_ptr(), n, ref.data_ptr(), new_idx.data_ptr(), n_new.data_ptr(), _stream())
    torch.cuda.synchronize()
    k = int(n_new.item())
    assert 0 <= k <= n
    return ref.cpu().numpy().view(np.uint64), new_idx.cpu().numpy().view(np.uint32)[:k].copy()


def check_call(idx, model, digests, base=0, values=None):
    ref, new_idx = run_dedupe(idx, digests, base, values)
    mref, mnew = model.call(digests, base) if values is None else model.insert(digests, values)
    bad = np.nonzero(ref != mref)[0]
    assert bad.size == 0, (bad[:8], ref[bad[:8]], mref[bad[:8]])
    assert np.array_equal(new_idx, mnew), (new_idx[:8], mnew[:8])
    assert idx.count() == len(model.table)
    return ref, new_idx


def run_lookup(idx, digests, stream=None):
    import torch
    n = len(digests)
    d = _dev(digests)
    ref = torch.full((n,), 12345, dtype=torch.int64, device="cuda")
    nf = torch.full((1,), -7, dtype=torch.int64, device="cuda")
    idx.dev_lookup(d.data_ptr(), n, ref.data_ptr(), nf.data_ptr(), _stream() if stream is None else stream)
    torch.cuda.synchronize()
    return ref.cpu().numpy().view(np.uint64), int(nf.item())


def check_lookup(idx, model, digests):
    ref, nf = run_lookup(idx, digests)
    mref, mnf = model.lookup(digests)
    bad = np.nonzero(ref != mref)[0]
    assert bad.size == 0, (bad[:8], ref[bad[:8]], mref[bad[:8]])
    assert nf == mnf
    return ref


def run_export(idx, db, max_out, room=None, offset=0):
    """cw_dev_dedupe_export into buffers of `room` pairs filled with 0xEE: (digests[room, db], values[room], *d_n).  offset: bytes the
    digest array starts behind a 16-byte boundary (8 = the 8-byte store path)."""
    import torch
    room = max_out if room is None else room
    dig = torch.full((room * db + 16,), 0xEE, dtype=torch.uint8, device="cuda")
    val = torch.full((max(room, 1),), -1, dtype=torch.int64, device="cuda")
    dn = torch.full((1,), -3, dtype=torch.int64, device="cuda")
    assert dig.data_ptr() % 16 == 0
    idx.dev_export(dig.data_ptr() + offset, val.data_ptr(), max_out, dn.data_ptr(), _stream())
    torch.cuda.synchronize()
    return dig.cpu().numpy()[offset:offset + room * db].reshape(room, db), val.cpu().numpy().view(np.uint64)[:room], int(dn.item())


def pairs(dig: np.ndarray, val: np.ndarray):
    return [(dig[i].tobytes(), int(val[i])) for i in range(len(val))]


def crafted_digests(db: int, n: int, seed: int, dups: bool = True) -> np.ndarray:
    """Distinct random digests, then pairs that share their first 8 bytes, their last 8, differ in one middle byte, or hold the
    same 64-bit words in another order; then (dups) duplicates planted at random positions."""
    rng = np.random.default_rng(seed)
    d = rng.integers(0, 256, (n, db), dtype=np.uint8)
    q = n // 8
    for i in range(0, q, 2):                      # shared prefix
        d[i + 1, :8] = d[i, :8]
    for i in range(q, 2 * q, 2):                  # shared suffix
        d[i + 1, -8:] = d[i, -8:]
    for i in range(2 * q, 3 * q, 2):              # one middle byte apart
        d[i + 1] = d[i]
        d[i + 1, db // 2] ^= 0x5A
    for i in range(3 * q, 4 * q, 2):              # the same words, permuted (a XOR fold or a word sum collides)
        d[i + 1] = np.roll(d[i].view(np.uint64), 1).view(np.uint8)
    assert len({r.tobytes() for r in d[:4 * q]}) == 4 * q
    if dups:
        dup_at = rng.choice(np.arange(4 * q, n), n // 4, replace=False)
        d[dup_at] = d[rng.integers(0, n, dup_at.size)]
    else:
        assert len({r.tobytes() for r in d}) == n
    return d[rng.permutation(n)]


def rand_values(rng, n):
    """Random u64 values, never the reserved CW_DEDUPE_MISS."""
    return rng.integers(0, MISS, n, dtype=np.uint64)


def queries(d: np.ndarray, seed: int) -> np.ndarray:
    """Every row of d, 4,096 absent random digests and near-misses of present ones (one byte flipped, words rotated), shuffled."""
    rng = np.random.default_rng(seed)
    db = d.shape[1]
    flipped = d[rng.integers(0, len(d), 1024)].copy()
    flipped[np.arange(1024), rng.integers(0, db, 1024)] ^= 0x01
    rotated = np.roll(d[rng.integers(0, len(d), 1024)].view(np.uint64), 1, axis=1).view(np.uint8)
    q = np.concatenate([d, rng.integers(0, 256, (4096, db), dtype=np.uint8), flipped, rotated])
    return q[rng.permutation(len(q))]


def full_crafted_index(cw, alg, db, max_entries):
    """8,192 distinct crafted digests inserted over two calls: (index, model, digests)."""
    d = crafted_digests(db, 8192, seed=100 + db, dups=False)
    idx, model = cw.DedupeIndex(alg, max_entries), Model()
    check_call(idx, model, d[:4096], base=7)
    check_call(idx, model, d[4096:], base=1 << 33)
    assert idx.count() == 8192
    return idx, model, d


# ---- lookup -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alg,db", WIDTHS)
def test_lookup_on_a_full_index(cw, alg, db):
    idx, model, d = full_crafted_index(cw, alg, db, 8192)          # max_entries == entries: load exactly 0.5, long chains
    idx2, model2, _ = full_crafted_index(cw, alg, db, 16384)       # the same entries, with room for a further call
    with idx, idx2:
        q = queries(d, seed=db)
        for x, m in ((idx, model), (idx2, model2)):
            ref = check_lookup(x, m, q)
            assert (ref != MISS).sum() >= 8192 and (ref == MISS).sum() >= 4096
            assert x.count() == 8192
        with pytest.raises(cw.CwError) as e:                        # the full index still refuses to insert, and still answers
            run_dedupe(idx, q[:16], 0)
        assert e.value.code == CW_ERR_NOMEM
        check_lookup(idx, model, q[:1000])
        # the lookup left nothing behind in state or min_idx: a lookup-or-insert of present, absent and near-miss digests
        fresh = np.concatenate([q[:3000], q[:500]])
        check_call(idx2, model2, fresh, base=1 << 40)
        check_lookup(idx2, model2, q)
        for n in (1, 63, 257):                                      # not multiples of the wavefront or the workgroup
            check_lookup(idx2, model2, q[5:5 + n])
            check_lookup(idx2, model2, d[9:9 + n])                  # all hits


def test_lookup_of_nothing_is_a_no_op(cw):
    import torch
    sentinel = torch.full((4,), 77, dtype=torch.int64, device="cuda")
    with cw.DedupeIndex("skein", 16) as idx:
        idx.dev_lookup(0, 0, 0, 0, _stream())
        idx.dev_insert(0, 0, 0, 0, 0, 0, _stream())
        idx.dev_lookup(sentinel.data_ptr(), 0, sentinel.data_ptr(), sentinel.data_ptr(), _stream())
        idx.dev_insert(sentinel.data_ptr(), sentinel.data_ptr(), 0, sentinel.data_ptr(), sentinel.data_ptr(), sentinel.data_ptr(), _stream())
        torch.cuda.synchronize()
        assert (sentinel.cpu() == 77).all() and idx.count() == 0
        assert cw.DedupeIndex.MISS == MISS


# ---- insert with values ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alg,db", WIDTHS)
def test_insert_with_values(cw, alg, db):
    rng = np.random.default_rng(db)
    a = crafted_digests(db, 3000, seed=db + 1)
    b = np.concatenate([crafted_digests(db, 6000, seed=db + 2), a[rng.integers(0, 3000, 1500)]])
    b = b[rng.permutation(len(b))]
    vb = rand_values(rng, len(b))
    assert not (np.diff(vb.astype(np.float64)) > 0).all() and (vb != MISS).all()
    outs = []
    for _ in range(2):                                              # identical on a second run
        with cw.DedupeIndex(alg, 40000) as idx:
            model = Model()
            check_call(idx, model, a, base=5)                       # digests already present keep base + i
            ref, new_idx = check_call(idx, model, b, values=vb)
            assert 0 < len(new_idx) < len(b) and (ref < 5 + 3000).sum() >= 1500
            outs.append((ref, new_idx))
            c = np.concatenate([b[::5], crafted_digests(db, 1000, seed=db + 3)])
            check_call(idx, model, c, base=1 << 50)                 # a cw_dev_dedupe afterwards
            check_lookup(idx, model, np.concatenate([a, b, c]))
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])
    p = rng.permutation(len(b))                                     # the same pairs permuted: the model decides the winners
    with cw.DedupeIndex(alg, 40000) as idx:
        model = Model()
        check_call(idx, model, a, base=5)
        check_call(idx, model, b[p], values=vb[p])


def test_insert_into_a_full_index_refuses_and_changes_nothing(cw):
    rng = np.random.default_rng(4)
    a = rng.integers(0, 256, (600, 16), dtype=np.uint8)
    b = rng.integers(0, 256, (500, 16), dtype=np.uint8)
    q = np.concatenate([a, b])
    with cw.DedupeIndex("skein", 1000) as idx:
        model = Model()
        check_call(idx, model, a, values=rand_values(rng, 600))
        before = check_lookup(idx, model, q)
        with pytest.raises(cw.CwError) as e:
            run_dedupe(idx, b, values=rand_values(rng, 500))
        assert e.value.code == CW_ERR_NOMEM
        assert idx.count() == 600
        assert np.array_equal(check_lookup(idx, model, q), before)
        check_call(idx, model, b[:400], values=rand_values(rng, 400))   # 600 + 400 <= 1000: admitted


# ---- export -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alg,db", WIDTHS)
def test_export(cw, alg, db):
    rng = np.random.default_rng(db + 10)
    with cw.DedupeIndex(alg, 20000) as idx:
        dig, val, n = run_export(idx, db, 64)                       # empty: *d_n == 0, nothing written
        assert n == 0 and (dig == 0xEE).all() and (val == MISS).all()
        model = Model()
        check_call(idx, model, crafted_digests(db, 5000, seed=db + 11), base=3)
        check_call(idx, model, crafted_digests(db, 3000, seed=db + 12), values=rand_values(rng, 3000))
        check_call(idx, model, crafted_digests(db, 300, seed=db + 13), base=1 << 45)
        count = idx.count()
        dig, val, n = run_export(idx, db, count + 100)
        assert n == count == len(model.table)
        assert set(pairs(dig[:n], val[:n])) == model.items()
        assert (dig[n:] == 0xEE).all() and (val[n:] == MISS).all()
        dig2, val2, n2 = run_export(idx, db, count + 100)
        assert n2 == n and dig2.tobytes() == dig.tobytes() and val2.tobytes() == val.tobytes()
        dig3, val3, n3 = run_export(idx, db, count, offset=8)       # exactly count; digest array 8- but not 16-byte aligned
        assert n3 == n and dig3.tobytes() == dig[:n].tobytes() and val3.tobytes() == val[:n].tobytes()
        for off in (0, 8):                                          # truncated: exactly max_out pairs, the rest untouched
            digt, valt, nt = run_export(idx, db, count - 5, room=count + 7, offset=off)
            assert nt == count
            got = pairs(digt[:count - 5], valt[:count - 5])
            assert len(set(got)) == count - 5 and set(got) <= model.items()
            assert (digt[count - 5:] == 0xEE).all() and (valt[count - 5:] == MISS).all()
        _, _, n0 = run_export(idx, db, 0, room=4)                   # max_out 0 counts
        assert n0 == count
        check_call(idx, model, crafted_digests(db, 200, seed=db + 14), base=1 << 46)   # the index still works
        assert idx.count() == len(model.table)


def test_export_of_2_20_sha256_digests(cw):
    """2^21 slots = 8,192 tiles of 256 slots: the compaction crosses many workgroups and every level of the scan."""
    n = 1 << 20
    rng = np.random.default_rng(77)
    d = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    d[:, :4] = np.arange(n, dtype=np.uint32)[:, None].view(np.uint8)     # all distinct
    with cw.DedupeIndex("sha256mb", n) as idx:
        ref, new_idx = run_dedupe(idx, d, base=0)                   # value i for digest i
        assert len(new_idx) == n
        dig, val, k = run_export(idx, 32, n)
        assert k == n == idx.count()
        assert np.array_equal(np.sort(val), np.arange(n, dtype=np.uint64))
        assert np.array_equal(dig, d[val.astype(np.int64)])
        dig2, val2, _ = run_export(idx, 32, n)
        assert np.array_equal(val, val2) and np.array_equal(dig, dig2)


# ---- resize -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alg,db", WIDTHS)
def test_resize_grow_shrink_and_same_capacity(cw, alg, db):
    idx, model, d = full_crafted_index(cw, alg, db, 8192)
    with idx:
        q = queries(d, seed=db + 20)
        before = check_lookup(idx, model, q)
        with pytest.raises(cw.CwError) as e:
            idx.resize(idx.count() - 1)
        assert e.value.code == CW_ERR_BAD_ARG and idx.max_entries == 8192
        with pytest.raises(cw.CwError) as e:
            idx.resize(0)
        assert e.value.code == CW_ERR_BAD_ARG
        assert np.array_equal(check_lookup(idx, model, q), before)
        idx.resize(65536)                                           # grow: 16,384 -> 131,072 slots
        assert idx.max_entries == 65536 and idx.count() == 8192
        assert np.array_equal(check_lookup(idx, model, q), before)
        check_call(idx, model, np.concatenate([q[:2000], crafted_digests(db, 500, seed=db + 21)]), base=1 << 41)
        count = idx.count()
        assert 8192 < count < 16384
        idx.resize(count)                                           # shrink to exactly the count: 131,072 -> 32,768 slots
        assert idx.max_entries == count and idx.count() == count
        check_lookup(idx, model, q)
        with pytest.raises(cw.CwError) as e:                        # max_entries == count: the model of the admission check refuses any block
            run_dedupe(idx, q[:8], 0)
        assert e.value.code == CW_ERR_NOMEM
        check_lookup(idx, model, q)
        idx.resize(16384)                                           # the same 32,768 slots: only max_entries changes
        assert idx.max_entries == 16384 and idx.count() == count
        check_lookup(idx, model, q)
        check_call(idx, model, np.concatenate([q[4000:5000], crafted_digests(db, 300, seed=db + 22)]), base=1 << 42)
        check_lookup(idx, model, q)
        dig, val, n = run_export(idx, db, idx.count())
        assert set(pairs(dig, val)) == model.items()


def test_full_index_resize_then_retry(cw):
    rng = np.random.default_rng(31)
    a = rng.integers(0, 256, (600, 32), dtype=np.uint8)
    b = np.concatenate([rng.integers(0, 256, (400, 32), dtype=np.uint8), a[:100]])
    with cw.DedupeIndex("sha256mb", 1000) as idx:
        model = Model()
        check_call(idx, model, a, base=0)
        with pytest.raises(cw.CwError) as e:
            run_dedupe(idx, b, 5000)
        assert e.value.code == CW_ERR_NOMEM
        idx.resize(2 * idx.max_entries)
        assert idx.max_entries == 2000
        ref, new_idx = check_call(idx, model, b, base=5000)
        assert len(new_idx) == 400 and (ref[400:] < 100).all()


def test_fused_call_resize_then_retry(cw, oracle):
    import torch
    bs, n = 4096, 1024
    data = b"".join(corpus_file(f) for f in corpus_names())
    blocks = np.frombuffer((data * (n * bs // len(data) + 1))[:n * bs], dtype=np.uint8).reshape(n, bs).copy()
    rng = np.random.default_rng(32)
    dup_at = rng.choice(n, n // 5, replace=False)
    blocks[dup_at] = blocks[rng.integers(0, n, dup_at.size)]
    src = torch.from_numpy(blocks.reshape(-1)).cuda()
    stride = (cw.compress_bound("lz4", bs) + 15) // 16 * 16
    dig = torch.zeros((n, 64), dtype=torch.uint8, device="cuda")
    ref = torch.zeros(n, dtype=torch.int64, device="cuda")
    new_idx = torch.zeros(n, dtype=torch.int32, device="cuda")
    dst = torch.zeros(n * stride, dtype=torch.uint8, device="cuda")
    sizes = torch.zeros(n, dtype=torch.int32, device="cuda")
    args = ("lz4", src.data_ptr(), bs, n, 9, dig.data_ptr(), ref.data_ptr(), new_idx.data_ptr(), dst.data_ptr(), stride, sizes.data_ptr())
    with cw.DedupeIndex("skein512", 512) as idx:
        with pytest.raises(cw.CwError) as e:
            idx.dev_hash_dedupe_compress(*args, _stream())
        assert e.value.code == CW_ERR_NOMEM and idx.count() == 0
        idx.resize(2048)
        k = idx.dev_hash_dedupe_compress(*args, _stream())
        torch.cuda.synchronize()
        model = Model()
        mref, mnew = model.call(dig.cpu().numpy(), 9)
        assert k == len(mnew) and 0 < k < n and idx.count() == k
        assert np.array_equal(ref.cpu().numpy().view(np.uint64), mref)
        assert np.array_equal(new_idx.cpu().numpy().view(np.uint32)[:k], mnew)
        slots, sz = dst.view(n, stride).cpu().numpy(), sizes.cpu().numpy()
        for j, i in enumerate(mnew):
            w = oracle.lz4_compress(blocks[i].tobytes())
            assert sz[j] == len(w) and slots[j, :len(w)].tobytes() == w, (j, i)


# ---- round trip ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alg,db", WIDTHS)
def test_export_then_insert_round_trip(cw, alg, db):
    rng = np.random.default_rng(db + 40)
    with cw.DedupeIndex(alg, 10000) as a:
        model = Model()
        d = crafted_digests(db, 6000, seed=db + 41)
        check_call(a, model, d, values=rand_values(rng, 6000))
        count = a.count()
        dig, val, n = run_export(a, db, count)
        assert n == count
        q = queries(d, seed=db + 42)
        want = check_lookup(a, model, q)
        p = rng.permutation(n)
        with cw.DedupeIndex(alg, 50000) as b, cw.DedupeIndex(alg, count) as c:
            for x, order in ((b, np.arange(n)), (c, p)):
                ref, new_idx = run_dedupe(x, dig[order], values=val[order])
                assert np.array_equal(ref, val[order]) and np.array_equal(new_idx, np.arange(n, dtype=np.uint32))
                assert x.count() == count
                got, nf = run_lookup(x, q)
                assert np.array_equal(got, want) and nf == (want != MISS).sum()


def test_import_into_an_index_that_holds_some_of_the_digests(cw):
    rng = np.random.default_rng(50)
    d = crafted_digests(32, 5000, seed=51, dups=False)
    with cw.DedupeIndex("sha256mb", 6000) as a, cw.DedupeIndex("sha256mb", 9000) as b:
        ma, mb = Model(), Model()
        check_call(a, ma, d, values=rand_values(rng, 5000))
        held = np.concatenate([d[1000:2500], rng.integers(0, 256, (700, 32), dtype=np.uint8)])
        check_call(b, mb, held, values=rand_values(rng, len(held)))  # 1,500 of a's digests under other values
        dig, val = a.export()
        assert set(pairs(dig, val)) == ma.items()
        b.set_stage_entries(999)                                    # six pieces
        n_inserted = b.import_(dig, val)
        mref, mnew = mb.insert(dig, val)
        assert n_inserted == len(mnew) == 3500
        assert b.count() == len(mb.table) == 5700
        got = check_lookup(b, mb, d)
        assert (got[1000:2500] != ma.lookup(d[1000:2500])[0]).all()  # b's own values survived
        with pytest.raises(cw.CwError) as e:                        # the whole import is admitted up front: 5,700 + 5,000 > 9,000
            b.import_(rng.integers(0, 256, (5000, 32), dtype=np.uint8), np.arange(5000, dtype=np.uint64))
        assert e.value.code == CW_ERR_NOMEM and b.count() == 5700
        check_lookup(b, mb, d)


# ---- host forms and Python ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alg,db", WIDTHS)
def test_host_export_import_in_pieces_and_snapshot(cw, alg, db, tmp_path):
    rng = np.random.default_rng(db + 60)
    d = crafted_digests(db, 5000, seed=db + 61)
    v = rand_values(rng, 5000)
    q = queries(d, seed=db + 62)
    with cw.DedupeIndex(alg, 8000) as a:
        model = Model()
        a.set_stage_entries(777)                                    # n above the piece size, no multiple of it
        assert a.import_(d, v) == len(model.insert(d, v)[1])        # duplicates within and across pieces: the first pair wins
        assert a.count() == len(model.table)
        want = check_lookup(a, model, q)
        dig, val = a.export()
        assert dig.dtype == np.uint8 and dig.shape == (a.count(), db) and val.dtype == np.uint64
        assert set(pairs(dig, val)) == model.items()
        a.set_stage_entries(0)
        dig1, val1 = a.export()                                     # one piece: the same bytes
        assert dig1.tobytes() == dig.tobytes() and val1.tobytes() == val.tobytes()
        path = tmp_path / "index.snapshot"
        a.save(path)
        with cw.DedupeIndex.load(path) as b:
            assert b.hash_alg == a.hash_alg and b.max_entries == 8000 and b.count() == a.count()
            assert np.array_equal(run_lookup(b, q)[0], want)
        with cw.DedupeIndex.load(path, max_entries=a.count()) as c:
            assert c.max_entries == a.count()
            assert np.array_equal(run_lookup(c, q)[0], want)
        with pytest.raises(cw.CwError):
            cw.DedupeIndex.load(path, max_entries=a.count() - 1)


# ---- ordering --------------------------------------------------------------------------------------------------------------
def test_lookup_on_another_stream_sees_the_insert(cw):
    import torch
    rng = np.random.default_rng(70)
    a = rng.integers(0, 256, (200000, 64), dtype=np.uint8)
    v = rand_values(rng, len(a))
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    da, dv = _dev(a), _dev(v)
    ra = torch.zeros(len(a), dtype=torch.int64, device="cuda")
    na = torch.zeros(len(a), dtype=torch.int32, device="cuda")
    ka = torch.zeros(1, dtype=torch.int64, device="cuda")
    rl = torch.zeros(len(a), dtype=torch.int64, device="cuda")
    kl = torch.zeros(1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()                      # the inputs are ready; between the two calls nothing waits
    with cw.DedupeIndex("skein512", 400000) as idx:
        idx.dev_insert(da.data_ptr(), dv.data_ptr(), len(a), ra.data_ptr(), na.data_ptr(), ka.data_ptr(), s1.cuda_stream)
        idx.dev_lookup(da.data_ptr(), len(a), rl.data_ptr(), kl.data_ptr(), s2.cuda_stream)
        torch.cuda.synchronize()
        assert int(ka.item()) == len(a) and int(kl.item()) == len(a)
        assert np.array_equal(rl.cpu().numpy().view(np.uint64), v)


# ---- bad arguments -----------------------------------------------------------------------------------------------------------
def test_bad_arguments_launch_nothing(cw):
    import torch
    rng = np.random.default_rng(80)
    d = rng.integers(0, 256, (8, 16), dtype=np.uint8)
    with cw.DedupeIndex("skein", 64) as idx:
        model = Model()
        check_call(idx, model, d[:4], values=np.arange(4, dtype=np.uint64))
        dd = _dev(np.concatenate([d.reshape(-1), np.zeros(16, np.uint8)]))
        u = torch.full((16,), 77, dtype=torch.int64, device="cuda")
        p, P = dd.data_ptr(), u.data_ptr()
        big = 2 ** 32 - 255
        bad = [
            (idx.dev_lookup, (0, 8, P, P)), (idx.dev_lookup, (p, 8, 0, P)), (idx.dev_lookup, (p, 8, P, 0)),
            (idx.dev_lookup, (p + 4, 8, P, P)), (idx.dev_lookup, (p, big, P, P)),
            (idx.dev_insert, (0, P, 8, P, P, P)), (idx.dev_insert, (p, 0, 8, P, P, P)), (idx.dev_insert, (p, P, 8, 0, P, P)),
            (idx.dev_insert, (p, P, 8, P, 0, P)), (idx.dev_insert, (p, P, 8, P, P, 0)),
            (idx.dev_insert, (p + 4, P, 8, P, P, P)), (idx.dev_insert, (p, P, big, P, P, P)),
            (idx.dev_export, (0, P, 8, P)), (idx.dev_export, (p, 0, 8, P)), (idx.dev_export, (p, P, 8, 0)),
            (idx.dev_export, (p + 4, P, 8, P)),
        ]
        for fn, args in bad:
            with pytest.raises(cw.CwError) as e:
                fn(*args, _stream())
            assert e.value.code == CW_ERR_BAD_ARG, (fn.__name__, args)
        for n in (0, 2 ** 40 + 1):
            with pytest.raises(cw.CwError) as e:
                idx.resize(n)
            assert e.value.code == CW_ERR_BAD_ARG
        L = cw.lib()
        assert L.cw_dedupe_export(idx._h, None, None, 8, None) == CW_ERR_BAD_ARG
        assert L.cw_dedupe_import(idx._h, None, None, 8, None) == CW_ERR_BAD_ARG
        assert L.cw_dedupe_max_entries(idx._h, None) == CW_ERR_BAD_ARG
        if cw.device_count() >= 2:                                  # an index of device 0 used from device 1
            cw.set_device(1)
            try:
                for fn, args in ((idx.dev_lookup, (p, 8, P, P)), (idx.dev_insert, (p, P, 8, P, P, P)), (idx.dev_export, (p, P, 8, P)),
                                 (idx.resize, (128,))):
                    with pytest.raises(cw.CwError) as e:
                        fn(*args)
                    assert e.value.code == CW_ERR_BAD_ARG, fn.__name__
            finally:
                cw.set_device(0)
                torch.cuda.set_device(0)
        torch.cuda.synchronize()
        assert (u.cpu() == 77).all() and idx.count() == 4 and idx.max_entries == 64
        check_lookup(idx, model, d)


@pytest.mark.parametrize("refusal", ["cdc_full", "cdc_wraps", "dedupe_full", "dedupe_wraps"])
def test_a_refused_call_on_one_stream_orders_the_next_call_on_another(cw, refusal):
    """A call that is refused after it queued work -- the fused chunk call once its cut and hash are queued: the index is full, or
    base + the chunk count wraps -- or before it queued any (cw_dev_dedupe: too many blocks, a base that wraps) leaves the index
    usable from another stream with no synchronisation by the caller: an insert of 32 digests and a lookup of them answer as the
    model does."""
    import torch
    db = 64
    rng = np.random.default_rng(77)
    with cw.DedupeIndex("skein512", 64) as idx:
        model = Model()
        known = rng.integers(0, 256, (32, db), dtype=np.uint8)
        values = 1000 + 3 * np.arange(32, dtype=np.uint64)
        d_known, d_values = _dev(known), _dev(values)
        z = lambda n, dt, v: torch.full((n,), v, dtype=dt, device="cuda")  # noqa: E731
        ref, new_idx, n_new = z(32, torch.int64, -1), z(32, torch.int32, -1), z(1, torch.int64, -1)
        found, n_found = z(32, torch.int64, 12345), z(1, torch.int64, -7)
        a, b = torch.cuda.Stream(), torch.cuda.Stream()
        p = cw.CdcParams.default(256)
        src = torch.from_numpy(rng.integers(0, 256, 64 << 10, dtype=np.uint8)).cuda()
        cap = p.max_offsets(src.numel())
        off, k, dig = z(cap, torch.int64, 0), z(1, torch.int64, 0), z(cap * db, torch.uint8, 0)
        c_ref, c_new, c_n_new = z(cap, torch.int64, -1), z(cap, torch.int32, -1), z(1, torch.int64, -1)
        total = cw.chunk_slots_bytes("lz4", src.numel(), cap - 1)
        dst, sizes = z(total, torch.uint8, 0), z(cap, torch.int32, -1)
        many = _dev(rng.integers(0, 256, (256, db), dtype=np.uint8))
        torch.cuda.synchronize()  # (torch filled the buffers on its own stream)
        with pytest.raises(cw.CwError) as e:
            if refusal.startswith("cdc"):
                idx.dev_cdc_dedupe_compress(p, "lz4", src.data_ptr(), src.numel(), True, 0 if refusal == "cdc_full" else 2 ** 64 - 1, off.data_ptr(),
                                            cap, k.data_ptr(), dig.data_ptr(), c_ref.data_ptr(), c_new.data_ptr(), c_n_new.data_ptr(),
                                            dst.data_ptr(), total, sizes.data_ptr(), a.cuda_stream)
            else:
                idx.dev_dedupe(many.data_ptr(), 256, 0 if refusal == "dedupe_full" else 2 ** 64 - 1, c_ref.data_ptr(), c_new.data_ptr(),
                               c_n_new.data_ptr(), a.cuda_stream)
        assert e.value.code == (CW_ERR_NOMEM if refusal.endswith("full") else CW_ERR_BAD_ARG)
        if refusal.startswith("cdc"):
            assert e.value.nchunks > 64, e.value.nchunks
        idx.dev_insert(d_known.data_ptr(), d_values.data_ptr(), 32, ref.data_ptr(), new_idx.data_ptr(), n_new.data_ptr(), b.cuda_stream)
        idx.dev_lookup(d_known.data_ptr(), 32, found.data_ptr(), n_found.data_ptr(), b.cuda_stream)
        torch.cuda.synchronize()
        mref, mnew = model.insert(known, values)
        assert np.array_equal(ref.cpu().numpy().view(np.uint64), mref)
        assert int(n_new.item()) == len(mnew) == 32 and np.array_equal(new_idx.cpu().numpy().view(np.uint32), mnew)
        lref, lfound = model.lookup(known)
        assert np.array_equal(found.cpu().numpy().view(np.uint64), lref) and int(n_found.item()) == lfound == 32
        assert idx.count() == 32
        if refusal.startswith("cdc"):  # the refused call wrote its cuts, and nothing of the dedupe or the codec
            assert int(k.item()) == e.value.nchunks and (c_ref.cpu() == -1).all() and (sizes.cpu() == -1).all()
