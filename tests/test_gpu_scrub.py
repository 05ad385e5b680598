"""Scrub and repair on the GPU (cw_dev_store_verify, cw_store_scrub, cw_dev_store_replace_chunks and cw.ChunkStore.scrub /
repair_from) against the plain-Python model of tests/scrub_model.py: the stores are built on the device, edited there, downloaded,
and the model -- the CPU oracle's decoders and hashes over the downloaded bytes -- predicts every status, total and cursor.

The work buffer lies between two poisoned guards, the status array is prefilled with a canary and has guard elements at both ends;
every device call is followed by a check that nothing outside the window's share of them changed."""
import numpy as np
import pytest

import restore_model as RM
import scrub_model as SM
from conftest import corpus_file

pytestmark = pytest.mark.gpu
ALGS = ["lz4", "lzf"]
HASHES = ["skein512", "skein", "sha256mb"]
GUARD = 256                      # bytes around the work buffer, elements around the status array
POISON, CANARY = 0xA5, 0xEEEEEEEE
DIR_BASE = 1000
NOMEM = -5


@pytest.fixture(scope="module")
def cw():
    import torch  # noqa: F401  (one HIP runtime for torch and libcwhc.so)
    import compute_war_amd as cw
    cw.init(0)
    yield cw
    cw.tune_reset()


def _sync():
    import torch
    torch.cuda.synchronize()


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


def _dev_u64(values):
    import torch
    return torch.from_numpy(np.asarray(values, np.uint64).reshape(-1).view(np.int64).copy()).cuda()


def _dev_bytes(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def text_and_noise():
    """About 1 MiB of Canterbury text (alice29.txt first) with a slice of random bytes inside, so that raw entries occur."""
    text = corpus_file("alice29.txt") + corpus_file("asyoulik.txt") + corpus_file("lcet10.txt") + corpus_file("plrabn12.txt")[:300000]
    return text[:500000] + np.random.default_rng(7).bytes(40000) + text[500000:]


def build(cw, alg, hash_alg, data, normal=1024, dir_entries=1100, store_bytes=2 << 20, dir_base=DIR_BASE):
    """A ChunkStore that holds `data`: (store, recipe)."""
    index = cw.DedupeIndex(hash_alg, 4096)
    cs = cw.ChunkStore(index, alg, cw.CdcParams(normal_size=normal), store_bytes, dir_entries, dir_base)
    return cs, cs.ingest(data)


class View:
    """A store as the device calls take it -- tensors that a test may edit -- and as the model takes it."""

    def __init__(self, cs, exact=False):
        used = cs.used()
        self.cs, self.index, self.alg = cs, cs.index, cs.comp_alg
        self.store_bytes = used if exact else cs.store_bytes                 # exact: the tensor ends with the last stored byte
        self.d_store = cs.d_store[:self.store_bytes].clone()
        self.d_dir = cs.d_dir.clone()
        self.dir_base, self.n = cs.dir_base, cs.dir_entries
        _sync()

    def directory(self):
        return self.d_dir.cpu().numpy().view(RM.LOC).copy()

    def set_entry(self, idx, entry):
        import torch
        self.d_dir[2 * idx:2 * idx + 2] = torch.from_numpy(np.array([entry], RM.LOC).view(np.int64).copy()).cuda()
        _sync()

    def flip(self, at, mask=0xFF):
        self.d_store[at] ^= mask
        _sync()

    def held(self, index=None):
        dig, val = (index or self.index).export()
        return SM.digests_by_value((dig[i].tobytes(), int(val[i])) for i in range(len(val)))

    def model(self, O, hash_alg, live=None, index=None):
        """(statuses, needs) as the model gives them for the tensors as they are now."""
        blob, d = self.d_store.cpu().numpy().tobytes(), self.directory()
        decode = O.lz4_decompress if self.alg == 0 else O.lzf_decompress
        status = SM.statuses(blob, self.store_bytes, d, self.dir_base, live, self.held(index), decode, SM.hash_fn(O, hash_alg))
        return status, SM.need(d, self.store_bytes, live)


def dev_scrub(cw, v, work_bytes, live=None, start=0, index=None, max_calls=None):
    """A loop of cw_dev_store_verify calls from cursor `start` until the cursor reaches the directory's end (or max_calls):
    (statuses with CANARY where nothing was written, the totals as a dict, the cursors the calls left).  Checks the guards."""
    import torch
    n = v.n
    work = torch.full((GUARD + work_bytes + GUARD,), POISON, dtype=torch.uint8, device="cuda")
    status = torch.from_numpy(np.full(GUARD + n + GUARD, CANARY, np.uint32).view(np.int32)).cuda()
    words = torch.from_numpy(np.array([start] + [0] * 8 + [CANARY], np.uint64).view(np.int64)).cuda()   # cursor | totals | guard
    d_live = torch.from_numpy(np.concatenate([live, np.full(4, 0xFFFFFFFF, np.uint32)]).view(np.int32)).cuda() if live is not None else None
    _sync()
    cursors, c = [], start
    before = status.cpu().numpy().view(np.uint32).copy()
    while max_calls is None or len(cursors) < max_calls:
        cw.dev_store_verify(index or v.index, v.alg, v.d_store.data_ptr(), v.store_bytes, v.d_dir.data_ptr(), v.dir_base, n,
                            d_live.data_ptr() if live is not None else 0, words.data_ptr(), work.data_ptr() + GUARD, work_bytes,
                            status.data_ptr() + 4 * GUARD, words.data_ptr() + 8, _stream())
        _sync()
        w = _u64(words)
        e, after = int(w[0]), status.cpu().numpy().view(np.uint32).copy()
        assert w[9] == CANARY, "the word behind the totals was written"
        assert (work[:GUARD] == POISON).all() and (work[GUARD + work_bytes:] == POISON).all(), "a store left d_work"
        changed = np.nonzero(after != before)[0]
        cursors.append(e)
        if c >= n:
            assert e == c and len(changed) == 0, "a call at or past the directory's end wrote something"
            break
        assert c < e <= n
        assert ((changed >= GUARD + c) & (changed < GUARD + e)).all(), "d_status was written outside the window"
        assert (after[GUARD + c:GUARD + e] != CANARY).all(), "a status of the window was not written"
        if e >= n:
            break
        c, before = e, after
    totals = dict(zip(SM.TOTALS, (int(x) for x in _u64(words)[1:9])))
    return after[GUARD:GUARD + n], totals, cursors


def expect(status, needs, work_bytes, cap=SM.DEFAULT_ENTRIES, start=0):
    written, totals, cursors = SM.scrub(needs, status, work_bytes, cap, start)
    full = np.full(len(needs), CANARY, np.uint32)
    for idx, s in written.items():
        full[idx] = s
    return full, totals, cursors


def check(cw, O, v, hash_alg, work_bytes=1 << 20, live=None, index=None, knob=None):
    """One scrub of the view by device calls equals the model's; returns the statuses."""
    status, needs = v.model(O, hash_alg, live, index)
    with cw.tuned(**({"CW_SCRUB_ENTRIES": knob} if knob else {})):
        got, totals, cursors = dev_scrub(cw, v, work_bytes, live, index=index)
    want, want_totals, want_cursors = expect(status, needs, work_bytes, SM.entry_cap(knob))
    assert cursors == want_cursors
    assert (got == want).all(), np.nonzero(got != want)[0][:10]
    assert totals == want_totals
    return status


@pytest.fixture(scope="module")
def stores(cw):
    """The clean store of every codec and hash algorithm, built once: {(alg, hash): (store, recipe, data)}."""
    data, made = text_and_noise(), {}

    def get(alg, hash_alg):
        if (alg, hash_alg) not in made:
            made[alg, hash_alg] = build(cw, alg, hash_alg, data) + (data,)
        return made[alg, hash_alg]
    yield get
    for cs, _, _ in made.values():
        cs.index.close()


def entries_of(d, raw):
    return [i for i in range(len(d)) if int(d[i]["stored"]) and bool(int(d[i]["raw"]) & RM.RAW) == raw]


# ---- 1. a clean store ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hash_alg", HASHES)
@pytest.mark.parametrize("alg", ALGS)
def test_clean_store(cw, oracle, stores, alg, hash_alg):
    cs, recipe, data = stores(alg, hash_alg)
    v = View(cs)
    d = v.directory()
    k = len(set(recipe.refs.tolist()))
    assert 400 < k < v.n and len(entries_of(d, True)) > 10 and len(entries_of(d, False)) > 300
    status = check(cw, oracle, v, hash_alg)
    zero = np.array([not any(int(x) for x in e) for e in d])
    assert (status[zero] == SM.SKIPPED).all() and (status[~zero] == SM.OK).all() and int((~zero).sum()) == k
    # the host form: the same statuses, and exact totals
    report = cs.scrub()
    assert (report.status == status).all() and report.clean and len(report.orphans) == 0
    assert report.stats == dict(checked=k, ok=k, malformed=0, unsound=0, mismatch=0, orphan=0, raw_bytes=sum(int(e["raw"]) & RM.LEN_MASK for e in d),
                                windows=1)


# ---- 2. damaged bytes ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alg", ALGS)
def test_damaged_bytes(cw, oracle, stores, alg):
    cs, _, _ = stores(alg, "skein")
    v = View(cs)
    d = v.directory()
    comp, raws = entries_of(d, False), entries_of(d, True)
    hit = []
    for i, where in ((comp[3], 0), (comp[40], 1), (comp[90], -1), (comp[150], 7), (comp[200], 2)):   # first, second, last, inner bytes
        pos, stored = int(d[i]["pos"]), int(d[i]["stored"])
        v.flip(pos + (where if where >= 0 else stored - 1), 0xFF if where != 7 else 0x01)
        hit.append(i)
    v.flip(int(d[raws[2]]["pos"]) + 5, 0x10)
    a, b = comp[10], next(i for i in comp[11:] if (int(d[i]["raw"]) ^ int(d[comp[10]]["raw"])) & RM.LEN_MASK)
    v.set_entry(a, d[b])
    v.set_entry(b, d[a])
    status = check(cw, oracle, v, "skein", work_bytes=131072)
    assert all(status[i] in (SM.MALFORMED, SM.MISMATCH) for i in hit)          # which of the two: the oracle's decoder says
    assert status[raws[2]] == SM.MISMATCH and status[a] == SM.MISMATCH and status[b] == SM.MISMATCH
    assert int((status == SM.OK).sum()) == len(comp) + len(raws) - len(hit) - 3


# ---- 3. tampered entries: the store tensor ends with the last stored byte ----------------------------------------------------------
@pytest.mark.parametrize("alg", ALGS)
def test_tampered_entries(cw, oracle, stores, alg):
    cs, _, _ = stores(alg, "skein")
    v = View(cs, exact=True)
    d = v.directory()
    comp, raws = entries_of(d, False), entries_of(d, True)
    last = int(np.argmax(d["pos"]))                                           # the entry whose bytes end the store
    assert int(d[last]["pos"]) + int(d[last]["stored"]) == v.store_bytes
    e = lambda i, **over: tuple(over.get(k, int(d[i][k])) for k in ("pos", "stored", "raw"))  # noqa: E731
    tampered = {comp[5]: e(comp[5], stored=0),
                last: e(last, stored=int(d[last]["stored"]) + 1),              # one byte past the store
                comp[7]: e(comp[7], pos=v.store_bytes + 1),
                comp[8]: e(comp[8], pos=2 ** 64 - 8),                          # pos + stored wraps
                comp[9]: e(comp[9], raw=int(d[comp[9]]["raw"]) | 1 << 17),
                comp[11]: e(comp[11], raw=int(d[comp[11]]["raw"]) | 1 << 30),
                comp[12]: e(comp[12], raw=int(d[comp[12]]["raw"]) & ~RM.LEN_MASK),  # length 0
                comp[13]: e(comp[13], raw=65537),
                raws[0]: e(raws[0], stored=int(d[raws[0]]["stored"]) - 1),     # raw with stored != length
                raws[1]: e(raws[1], raw=int(d[raws[1]]["raw"]) + 1)}
    for i, entry in tampered.items():
        v.set_entry(i, entry)
    for work in (65536, 1 << 20):
        status = check(cw, oracle, v, "skein", work_bytes=work)
        assert all(status[i] == SM.UNSOUND for i in tampered), [int(status[i]) for i in tampered]
    assert int((status == SM.OK).sum()) == len(comp) + len(raws) - len(tampered)


# ---- 4. orphans and two digests under one value -------------------------------------------------------------------------------------
@pytest.mark.parametrize("hash_alg", ["skein", "skein512"])
def test_orphans_and_duplicate_values(cw, oracle, stores, hash_alg):
    import torch
    cs, _, _ = stores("lz4", hash_alg)
    v = View(cs)
    d = v.directory()
    full = entries_of(d, False) + entries_of(d, True)
    dig, val = cs.index.export()
    lost = {v.dir_base + i for i in full[::7]}                                  # an index rebuilt without every 7th digest
    keep = np.array([int(x) not in lost for x in val])
    twice = [int(x) for x in val[keep][:40]]                                    # these values get a second, foreign digest
    damaged = twice[5] - v.dir_base                                             # ... and for one of them neither will match
    db = dig.shape[1]
    foreign = np.random.default_rng(3).integers(0, 256, (len(twice), db), dtype=np.uint8)
    with cw.DedupeIndex(hash_alg, 4096) as other:
        assert other.import_(dig[keep], val[keep]) == int(keep.sum())
        d_dig, d_val = _dev_bytes(foreign), _dev_u64(twice)
        ref, new_idx, n_new = torch.zeros(len(twice), dtype=torch.int64, device="cuda"), torch.zeros(len(twice), dtype=torch.int32, device="cuda"), \
            torch.zeros(1, dtype=torch.int64, device="cuda")
        _sync()
        other.dev_insert(d_dig.data_ptr(), d_val.data_ptr(), len(twice), ref.data_ptr(), new_idx.data_ptr(), n_new.data_ptr(), _stream())
        _sync()
        assert int(n_new.item()) == len(twice) and other.count() == int(keep.sum()) + len(twice)
        held = v.held(other)
        assert all(len(held[t]) == 2 for t in twice) and not lost & set(held)
        # the damaged one: the last stored byte, which LZ4 keeps as a literal, so the chunk still decodes to its length
        v.flip(int(d[damaged]["pos"]) + int(d[damaged]["stored"]) - 1, 0x01)
        status = check(cw, oracle, v, hash_alg, index=other, work_bytes=200000)
        assert all(status[x - v.dir_base] == SM.ORPHAN for x in lost)
        assert all(status[t - v.dir_base] == SM.OK for t in twice if t - v.dir_base != damaged)
        assert status[damaged] == SM.MISMATCH
        # the index was only read
        dig2, val2 = other.export()
        assert sorted(zip(val2.tolist(), (x.tobytes() for x in dig2))) == sorted((t, x) for t, xs in held.items() for x in xs)


# ---- 5. selection by flags, and a sparse directory ----------------------------------------------------------------------------------
def test_selection_with_flags(cw, oracle, stores):
    cs, _, _ = stores("lzf", "sha256mb")
    v = View(cs)
    d = v.directory()
    comp, raws = entries_of(d, False), entries_of(d, True)
    zero = [i for i in range(v.n) if not any(int(x) for x in d[i])]
    v.flip(int(d[raws[3]]["pos"]), 0x80)                                        # damaged, and not flagged below
    v.flip(int(d[raws[4]]["pos"]), 0x80)                                        # damaged and flagged
    live = np.zeros(v.n, np.uint32)
    live[comp[::2]] = 1
    live[raws[4]] = 0x80000000                                                  # any non-zero value is a flag
    live[zero[0]] = live[zero[-1]] = 1                                          # flagged, yet all zero: a kept recipe names a missing chunk
    for work, knob in ((1 << 20, None), (65536, 64)):
        status = check(cw, oracle, v, "sha256mb", work_bytes=work, live=live, knob=knob)
        assert status[zero[0]] == SM.UNSOUND == status[zero[-1]] and status[raws[3]] == SM.SKIPPED and status[raws[4]] == SM.MISMATCH
        assert (status[comp[::2]] == SM.OK).all() and (status[comp[1::2]] == SM.SKIPPED).all()
    # without flags the same store: the unflagged damage shows, the zero entries are skipped
    status = check(cw, oracle, v, "sha256mb")
    assert status[raws[3]] == SM.MISMATCH and (status[zero] == SM.SKIPPED).all()


@pytest.mark.parametrize("alg", ALGS)
def test_sparse_directory_after_compact(cw, oracle, alg):
    data = text_and_noise()
    a, b = data[:300000], data[200000:520000]
    cs, ra = build(cw, alg, "skein", a, dir_entries=600, store_bytes=1 << 20)
    try:
        rb = cs.ingest(b)
        cs.compact([rb])
        v = View(cs)
        d = v.directory()
        gone = sorted(set(ra.refs.tolist()) - set(rb.refs.tolist()))
        assert len(gone) > 50 and not any(int(x) for i in gone for x in d[i - v.dir_base])
        status = check(cw, oracle, v, "skein", knob=64)
        assert set(status.tolist()) == {SM.OK, SM.SKIPPED}
        report = cs.scrub(keep=[ra, rb])                                        # a's dropped chunks are named, and missing
        assert report.damaged.tolist() == gone and (report.status[np.array(gone) - v.dir_base] == SM.UNSOUND).all()
        assert report.stats["unsound"] == len(gone) and report.stats["ok"] == len(set(rb.refs.tolist()))
        assert cs.scrub(keep=[rb]).clean and cs.scrub().clean
    finally:
        cs.index.close()


# ---- 6. windows -------------------------------------------------------------------------------------------------------------------
def test_windows(cw, oracle, stores):
    cs, _, _ = stores("lz4", "skein")
    v = View(cs)
    d = v.directory()
    raws = entries_of(d, True)
    v.flip(int(d[raws[0]]["pos"]), 0x01)                                        # one mismatch, so that the totals are not all "ok"
    status, needs = v.model(oracle, "skein")
    prefix = np.cumsum(needs)
    k = int(np.searchsorted(prefix, 70000))                                     # entries [0, k] decode to exactly prefix[k] bytes
    exact = int(prefix[k])
    assert needs[k] > 0 and exact >= 65536
    runs = {}
    for work, knob in ((65536, None), (131072, None), (exact, None), (exact - 1, None), (1 << 20, 64), (1 << 21, None), (65536, 64)):
        with cw.tuned(**({"CW_SCRUB_ENTRIES": knob} if knob else {})):
            got, totals, cursors = dev_scrub(cw, v, work)
        want, want_totals, want_cursors = expect(status, needs, work, SM.entry_cap(knob))
        assert cursors == want_cursors, (work, knob)
        assert (got == status).all() and (want == status).all() and totals == want_totals, (work, knob)
        runs[work, knob] = cursors, totals
    # the sum may equal work_bytes, not exceed it: entry k ends the first window in one run and starts the second in the other
    first, less = runs[exact, None][0][0], runs[exact - 1, None][0][0]
    assert first > k == less and sum(needs[:first]) == exact and sum(needs[:less]) == exact - needs[k]
    assert runs[1 << 21, None][0] == [v.n] and len(runs[1 << 20, 64][0]) == -(-v.n // 64) and v.n >= 200
    sums = [{key: t[key] for key in SM.TOTALS[:7]} for _, t in runs.values()]
    assert all(s == sums[0] for s in sums) and sums[0]["mismatch"] == 1
    # a window from the middle; a cursor at and past the end: nothing at all is written
    got, totals, cursors = dev_scrub(cw, v, 65536, start=500, max_calls=2)
    want, want_totals, want_cursors = expect(status, needs, 65536, start=500)
    assert cursors == want_cursors[:2] and (got[:500] == CANARY).all() and (got[500:cursors[1]] == status[500:cursors[1]]).all()
    for start in (v.n, v.n + 1, 2 ** 64 - 1):
        got, totals, cursors = dev_scrub(cw, v, 65536, start=start)
        assert cursors == [start] and (got == CANARY).all() and totals == dict.fromkeys(SM.TOTALS, 0)


@pytest.mark.parametrize("alg", ALGS)
def test_a_chunk_of_65536_bytes_and_the_host_form(cw, oracle, alg):
    """Chunking parameters that allow a chunk of 65,536 bytes: a run of one byte value finds no cut before max_size."""
    rng = np.random.default_rng(11)
    data = bytes(65536) + b"\x55" * 131072 + corpus_file("alice29.txt")[:90000] + rng.bytes(66000) + bytes(range(256)) * 300
    cs, recipe = build(cw, alg, "skein512", data, normal=8192, dir_entries=100, store_bytes=1 << 20, dir_base=0)
    try:
        v = View(cs)
        status, needs = v.model(oracle, "skein512")
        assert needs.count(65536) >= 2 and set(status.tolist()) == {SM.OK, SM.SKIPPED}
        for work in (65536, 65537, 131072):
            got, totals, cursors = dev_scrub(cw, v, work)
            want, want_totals, want_cursors = expect(status, needs, work)
            assert cursors == want_cursors and (got == status).all() and totals == want_totals
        assert len(cursors) > 1
        # cw_store_scrub is that loop, with CW_STORE_PIECE as the work buffer (raised to 65536)
        for piece, work in ((1, 65536), (65536, 65536), (100000, 100000), (None, 256 << 20)):
            with cw.tuned(**({"CW_STORE_PIECE": piece} if piece else {})):
                report = cs.scrub()
            _, want_totals, _ = expect(status, needs, work)
            assert (report.status == status).all() and report.stats == want_totals, piece
        assert cs.restore(recipe, verify=True) == data
    finally:
        cs.index.close()


# ---- 7. cw_dev_store_replace_chunks -------------------------------------------------------------------------------------------------
def replace_call(cw, v, payload, in_bytes, locs, values, used, count=None, max_count=None):
    """One call on the view's tensors: (d_result as a list, the cursor afterwards).  The arrays have guard elements behind them."""
    import torch
    d_in = _dev_bytes(np.frombuffer(bytes(payload) + bytes([POISON]) * 64, np.uint8))
    d_loc = _dev_bytes(np.concatenate([np.asarray(locs, RM.LOC), np.array([(2 ** 63, 0xFFFFFFFF, 0xFFFFFFFF)], RM.LOC)]))
    d_val, d_count, d_used = _dev_u64(list(values) + [RM.MISS]), _dev_u64([len(values) if count is None else count]), _dev_u64([used])
    result = torch.from_numpy(np.array([CANARY] * 3, np.uint64).view(np.int64)).cuda()
    _sync()
    cw.dev_store_replace_chunks(d_in.data_ptr(), in_bytes, d_loc.data_ptr(), d_val.data_ptr(), d_count.data_ptr(),
                                len(values) if max_count is None else max_count, v.d_store.data_ptr(), v.store_bytes, d_used.data_ptr(),
                                v.d_dir.data_ptr(), v.dir_base, v.n, result.data_ptr(), _stream())
    _sync()
    r = _u64(result)
    assert r[2] == CANARY, "result guard"
    return r[:2].tolist(), int(_u64(d_used)[0])


@pytest.mark.parametrize("alg", ALGS)
def test_replace_chunks(cw, oracle, stores, alg):
    cs, recipe, data = stores(alg, "skein")
    v = View(cs)
    used, d = cs.used(), v.directory()
    blob = v.d_store.cpu().numpy().tobytes()
    comp, raws = entries_of(d, False), entries_of(d, True)
    zero = next(i for i in range(v.n) if not any(int(x) for x in d[i]))
    names = [comp[4], raws[1], comp[60], comp[4]]                               # one value twice: stored twice, either entry stays
    locs, pay = np.zeros(len(names), RM.LOC), bytearray()
    for k, i in enumerate(names):
        pos, stored, word = (int(x) for x in d[i])
        locs[k] = (len(pay), stored, word)
        pay += blob[pos:pos + stored]
    values = [v.dir_base + i for i in names]

    def refused(want, *args, **kw):
        got, cursor = replace_call(cw, v, *args, **kw)
        assert got == want and cursor == args[4], (got, want)
        assert v.d_store.cpu().numpy().tobytes() == blob and (v.directory() == d).all(), "a refused call changed the store"

    def model(payload, in_bytes, locs, values, used, store_bytes=None):
        return list(SM.replace_chunks(payload, in_bytes, locs, values, used, store_bytes or v.store_bytes, d, v.dir_base)[:2])

    total = len(pay)
    # 1: one byte too many, by the cursor
    at = v.store_bytes - total + 1
    assert model(pay, total, locs, values, at) == [1, total]
    refused([1, total], pay, total, locs, values, at)
    refused([1, total], pay, total, locs, values, v.store_bytes + 5)
    # 2: a value below the base, behind the directory, CW_DEDUPE_MISS
    for outside in (v.dir_base - 1, v.dir_base + v.n, RM.MISS, 0):
        vals = values[:2] + [outside] + values[3:]
        assert model(pay, total, locs, vals, used) == [2, total]
        refused([2, total], pay, total, locs, vals, used)
    # 3: an entry that leaves in_bytes, an all-zero one, an unsound one; the total counts the others
    assert model(pay, total - 1, locs, values, used) == [3, total - int(locs[3]["stored"])]
    refused([3, total - int(locs[3]["stored"])], pay, total - 1, locs, values, used)
    for bad in ((0, 0, 0), (0, 0, int(locs[1]["raw"])), (int(locs[1]["pos"]), int(locs[1]["stored"]), int(locs[1]["raw"]) | 1 << 20),
                (2 ** 64 - 4, int(locs[1]["stored"]), int(locs[1]["raw"]))):
        broken = locs.copy()
        broken[1] = bad
        assert model(pay, total, broken, values, used) == [3, total - int(locs[1]["stored"])]
        refused([3, total - int(locs[1]["stored"])], pay, total, broken, values, used)
    # 4: the entry named has another length; an all-zero entry and one with an unsound length field take any
    other = next(i for i in comp[61:] if (int(d[i]["raw"]) ^ int(d[comp[60]]["raw"])) & RM.LEN_MASK)
    vals = values[:2] + [v.dir_base + other] + values[3:]
    assert model(pay, total, locs, vals, used) == [4, total]
    refused([4, total], pay, total, locs, vals, used)
    # the order: 3 before 1 before 2 before 4
    refused([3, total - int(locs[3]["stored"])], pay, total - 1, locs, [RM.MISS] + vals[1:], v.store_bytes)
    refused([1, total], pay, total, locs, [RM.MISS] + vals[1:], v.store_bytes)
    refused([2, total], pay, total, locs, [RM.MISS] + vals[1:], used)
    # the count is read on the device: min(*d_count, max_count) positions
    refused([4, total], pay, total, locs, vals, used, count=100)
    got, cursor = replace_call(cw, v, pay, total, locs, vals, used, count=2)
    two = int(locs[0]["stored"]) + int(locs[1]["stored"])
    assert got == [0, two] and cursor == used + two
    v = View(cs)
    # 0: only the named entries change, the bytes go behind the cursor, the rest of the store stays
    unsound_len = comp[70]
    v.set_entry(unsound_len, (int(d[unsound_len]["pos"]), int(d[unsound_len]["stored"]), 0x1FFFF))
    d = v.directory()
    vals = values + [v.dir_base + zero, v.dir_base + unsound_len]
    locs2 = np.concatenate([locs, locs[1:2], locs[2:3]])
    verdict, tot, out, entries = SM.replace_chunks(pay, total, locs2, vals, used, v.store_bytes, d, v.dir_base)
    assert verdict == 0 and len(entries) == 5
    got, cursor = replace_call(cw, v, pay, total, locs2, vals, used)
    assert got == [0, tot] and cursor == used + tot
    after, d2 = v.d_store.cpu().numpy().tobytes(), v.directory()
    assert after[:used] == blob[:used] and after[used:used + tot] == out and after[used + tot:] == blob[used + tot:]
    twice = comp[4]
    for idx, e in entries.items():
        if idx != twice:
            assert tuple(int(x) for x in d2[idx]) == e, idx
    assert tuple(int(x) for x in d2[twice]) in ((used, int(locs[0]["stored"]), int(locs[0]["raw"])), entries[twice])
    same = np.ones(v.n, bool)
    same[list(entries)] = False
    assert (d2[same] == d[same]).all()


@pytest.mark.parametrize("alg", ALGS)
def test_replaced_chunks_restore(cw, oracle, alg):
    """Verdict 0 on a store of its own: the stream restores afterwards, from the new places."""
    data = text_and_noise()[400000:700000]
    cs, recipe = build(cw, alg, "sha256mb", data, dir_entries=400, store_bytes=1 << 20, dir_base=0)
    try:
        v = View(cs)
        used, d = cs.used(), v.directory()
        blob = v.d_store.cpu().numpy().tobytes()
        names = (entries_of(d, False) + entries_of(d, True))[::3]
        locs, pay = np.zeros(len(names), RM.LOC), bytearray()
        for k, i in enumerate(names):
            pos, stored, word = (int(x) for x in d[i])
            locs[k] = (len(pay), stored, word)
            pay += blob[pos:pos + stored]
        wiped = np.full(used, 0x5A, np.uint8)                                  # the old places hold nothing any more ...
        for i in set(range(cs.dir_entries)) - set(names):                      # ... except the chunks that are not replaced
            pos, stored = int(d[i]["pos"]), int(d[i]["stored"])
            wiped[pos:pos + stored] = np.frombuffer(blob[pos:pos + stored], np.uint8)
        cs.d_store[:used] = _dev_bytes(wiped)
        _sync()
        assert not cs.scrub().clean
        live = View(cs)
        live.d_store, live.d_dir = cs.d_store, cs.d_dir                        # the call writes the store's own tensors
        got, cursor = replace_call(cw, live, pay, len(pay), locs, names, used)
        assert got == [0, len(pay)] and cursor == used + len(pay)
        cs.d_used.fill_(cursor)
        _sync()
        assert cs.restore(recipe, verify=True) == data and cs.scrub().clean
    finally:
        cs.index.close()


# ---- 8. end to end: replicate, damage, scrub, repair ---------------------------------------------------------------------------------
@pytest.mark.parametrize("alg", ALGS)
def test_scrub_and_repair_from_a_peer(cw, oracle, alg):
    data = text_and_noise()
    streams = [data[:260000], data[200000:560000], data[520000:900000]]
    ia, ib = cw.DedupeIndex("skein", 4096), cw.DedupeIndex("skein", 4096)
    try:
        p = cw.CdcParams(normal_size=1024)
        A = cw.ChunkStore(ia, alg, p, 1 << 20, 900, DIR_BASE)
        B = cw.ChunkStore(ib, alg, p, 1 << 20, 900, 5)
        recs = [A.ingest(s) for s in streams]
        A.replicate_to(B, recs[:2])                                            # B lacks what only the third stream names
        A.compact(recs, store_bytes=A.used() + 10)                             # a store with no room to spare
        assert A.scrub().clean and B.scrub().clean
        d = View(A).directory()
        names = [set(r.refs.tolist()) for r in recs]
        only_b, only_c = sorted(names[1] - names[0] - names[2]), sorted(names[2] - names[0] - names[1])
        lacking, both = only_c[3], only_b[4]                                   # B lacks the one; its copy of the other gets damaged too
        victims = sorted(set(sorted(names[0])[5::37]) | {both})
        zeroed = victims[-1] if victims[-1] != both else victims[-2]
        assert len(victims) >= 6 and lacking not in names[0] and both not in names[0]
        # damage in A: bytes of several chunks B holds and of one it lacks, and one entry zeroed outright
        for value in victims + [lacking]:
            i = value - DIR_BASE
            if value == zeroed:
                A.d_dir[2 * i:2 * i + 2] = 0
            else:
                A.d_store[int(d[i]["pos"]) + int(d[i]["stored"]) // 2] ^= 0x5C
        dig, val = ia.export()
        digest_of = {int(x): dig[k].tobytes() for k, x in enumerate(val)}
        digb, valb = ib.export()
        twin = {digb[k].tobytes(): int(x) for k, x in enumerate(valb)}[digest_of[both]] - B.dir_base
        B.d_store[int(View(B).directory()[twin]["pos"]) + 1] ^= 0xFF
        _sync()
        # without flags the zeroed entry is not selected; with the recipes as flags it is a missing chunk
        report = A.scrub()
        assert (report.status == View(A).model(oracle, "skein")[0]).all()
        assert report.damaged.tolist() == sorted(set(victims + [lacking]) - {zeroed})
        live = np.zeros(900, np.uint32)
        live[np.concatenate([r.refs for r in recs]).astype(np.int64) - DIR_BASE] = 1
        report = A.scrub(keep=recs)
        assert (report.status == View(A).model(oracle, "skein", live=live)[0]).all()
        assert report.damaged.tolist() == sorted(victims + [lacking]) and report.status[zeroed - DIR_BASE] == SM.UNSOUND
        assert len(report.orphans) == 0 and not B.scrub().clean
        # the store is full: refused with the bytes needed, nothing changed
        before = (A.d_store.clone(), A.d_dir.clone(), A.used())
        with pytest.raises(cw.CwError) as e:
            A.repair_from(B, report)
        assert e.value.code == NOMEM and e.value.needed > 10
        assert (A.d_store == before[0]).all() and (A.d_dir == before[1]).all() and A.used() == before[2]
        with pytest.raises(ValueError):
            A.repair_from(cw.ChunkStore(ib, "lzf" if alg == "lz4" else "lz4", p, 1 << 16, 16), report)
        # compaction makes room (values stay), and the repair goes through
        A.compact(recs, store_bytes=A.used() + e.value.needed)
        d, count, used = View(A).directory(), ia.count(), A.used()
        out = A.repair_from(B, report)
        unavailable = sorted([lacking, both])
        assert out == dict(repaired=sorted(set(victims) - {both}), unavailable=unavailable, no_digest=[])
        assert ia.count() == count and A.used() == used + e.value.needed
        d2 = View(A).directory()
        for value in unavailable:                                               # their entries are untouched
            assert d2[value - DIR_BASE] == d[value - DIR_BASE]
        again = A.scrub(keep=recs)
        assert (again.status == View(A).model(oracle, "skein", live=live)[0]).all()
        assert again.damaged.tolist() == unavailable and again.stats["ok"] == report.stats["checked"] - 2
        assert A.restore(recs[0], verify=True) == streams[0]                    # every recipe that names no unavailable chunk
        for r in recs[1:]:
            with pytest.raises(cw.CwError):
                A.restore(r, verify=True)
        assert A.repair_from(B, again) == dict(repaired=[], unavailable=unavailable, no_digest=[])
        # a value the index holds no digest for cannot be repaired
        A.compact(recs[:1])
        assert A.scrub().clean
        gone = cw.ScrubReport(np.where(np.arange(900) == lacking - DIR_BASE, 2, 0).astype(np.uint32), {}, DIR_BASE)
        assert A.repair_from(B, gone) == dict(repaired=[], unavailable=[], no_digest=[lacking])
        assert A.restore(recs[0], verify=True) == streams[0]
    finally:
        ia.close()
        ib.close()
