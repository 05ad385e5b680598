"""Guard stripes on the GPU (cw_dev_store_guard_update, _check, _rebuild and cw.ChunkStore.protect / guard_check / repair_local; DESIGN.md
section 28): everything compared exactly with guard_model.py.  S = 65536 with G = 2 and G = 3 over a store of six stripes and a few
bytes with hand-built directories, then whole stores of corpus text: protect, ingest, damage, scrub, repair without a peer."""
import numpy as np
import pytest

import guard_model as GM
import restore_model as RM
from conftest import corpus_file

pytestmark = pytest.mark.gpu

ALGS = ["lz4", "lzf"]
GROUPS = [2, 3]
S, BYTES = GM.S, GM.STORE_BYTES
PAD = 256                        # poisoned bytes around the guard and the payload, elements around the lists
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


@pytest.fixture(scope="module")
def store(cw):
    """Six stripes and 37 bytes of noise: (numpy, device); neither is written."""
    host = np.random.default_rng(28).integers(0, 256, BYTES, dtype=np.uint8)
    return host, _dev_bytes(host)


@pytest.fixture(scope="module")
def guards(store):
    """guard_of(store, covered) for the cursors the tests use, each computed once."""
    cache = {}

    def guard(covered, G):
        if (covered, G) not in cache:
            cache[covered, G] = GM.guard_of(store[0], covered, S, G, BYTES)
        return cache[covered, G]
    return guard


class Guard:
    """A guard on the device between two poisoned pads, with its cursor."""

    def __init__(self, host, covered, size=None):
        self.size = len(host) if size is None else size
        buf = np.full(self.size + 2 * PAD, 0xEE, np.uint8)
        buf[PAD:PAD + self.size] = 0
        buf[PAD:PAD + len(host)] = host
        self.t, self.d_covered = _dev_bytes(buf), _dev_u64([covered])

    def ptr(self):
        return self.t.data_ptr() + PAD

    def host(self):
        h = self.t.cpu().numpy()
        assert (h[:PAD] == 0xEE).all() and (h[PAD + self.size:] == 0xEE).all(), "a store left the guard"
        return h[PAD:PAD + self.size]

    def covered(self):
        return int(_u64(self.d_covered)[0])


def update(cw, d_store, guard, used, G, store_bytes=BYTES, S=S):
    d_used, result = _dev_u64([used]), _dev_u64([7, 7, 7, 7])
    _sync()
    cw.dev_store_guard_update(d_store.data_ptr(), store_bytes, d_used.data_ptr(), guard.d_covered.data_ptr(), S, G, guard.ptr(), guard.size,
                              result.data_ptr(), _stream())
    _sync()
    return _u64(result).tolist()


# ---- 1. update ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", GROUPS)
def test_update_ranges(cw, store, guards, G):
    host, d_store = store
    for name, (a, b) in GM.update_ranges(G).items():
        g = Guard(guards(a, G), a)
        assert update(cw, d_store, g, b, G) == [0, a, b, b - a], name
        assert g.covered() == b and (g.host() == guards(b, G)).all(), name
        assert update(cw, d_store, g, b, G) == [0, b, b, 0], name                               # twice: nothing the second time
        assert g.covered() == b and (g.host() == guards(b, G)).all(), name


@pytest.mark.parametrize("G", GROUPS)
def test_update_refuses_an_inconsistent_cursor(cw, store, guards, G):
    host, d_store = store
    for used, covered in ((999, 1000), (BYTES + 1, 1000), (BYTES + 1, BYTES + 1)):
        g = Guard(guards(1000, G), covered)
        assert update(cw, d_store, g, used, G) == [1, covered, used, 0]
        assert g.covered() == covered and (g.host() == guards(1000, G)).all()
    # a store whose size is no multiple of 16, used to its last byte, in a tensor that ends there; and a larger guard than needed
    for cut in (0, 5, 21):
        n = BYTES - cut
        g = Guard(guards(0, G) * 0, 0, size=len(guards(0, G)) + S)
        exact = d_store[:n].clone()
        assert update(cw, exact, g, n, G, store_bytes=n) == [0, 0, n, n]
        want = np.zeros(g.size, np.uint8)
        want[:len(guards(n, G))] = guards(n, G)
        assert (g.host() == want).all(), cut


@pytest.mark.parametrize("G", GROUPS)
def test_many_small_updates_equal_one_large(cw, store, guards, G):
    """Queued one behind the other with no synchronise between them, each behind the write of the cursor it reads."""
    host, d_store = store
    cuts = sorted(set(np.random.default_rng(G).integers(0, BYTES, 40).tolist()) | {S, G * S, BYTES})
    g = Guard(guards(0, G), 0)
    d_used, results = _dev_u64(cuts), _dev_u64(np.zeros(4 * len(cuts)))
    _sync()
    for k in range(len(cuts)):
        cw.dev_store_guard_update(d_store.data_ptr(), BYTES, d_used.data_ptr() + 8 * k, g.d_covered.data_ptr(), S, G, g.ptr(), g.size,
                                  results.data_ptr() + 32 * k, _stream())
    _sync()
    want = [[0, a, b, b - a] for a, b in zip([0] + cuts[:-1], cuts)]
    assert _u64(results).reshape(-1, 4).tolist() == want
    assert g.covered() == BYTES and (g.host() == guards(BYTES, G)).all()


# ---- 2. check -------------------------------------------------------------------------------------------------------------------------
def check(cw, d_store, guard, G, flags=True, store_bytes=BYTES, S=S):
    n = guard.size // S
    bad, result = _dev_bytes(np.full(n + 2, 0xEEEEEEEE, np.uint32)), _dev_u64([7, 7, 7, 7])
    _sync()
    cw.dev_store_guard_check(d_store.data_ptr(), store_bytes, guard.d_covered.data_ptr(), S, G, guard.ptr(), guard.size, bad.data_ptr() + 4 if flags else 0,
                             result.data_ptr(), _stream())
    _sync()
    return _u64(result).tolist(), bad.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("G", GROUPS)
def test_check(cw, store, guards, G):
    host, d_store = store
    W, covered = G * S, 4 * S + 1000
    n = -(-covered // W)

    def expect(d, g, hurt_store=None, hurt_guard=None):
        want, flags = GM.check(g.host() if hurt_guard is None else hurt_guard, host if hurt_store is None else hurt_store, BYTES, covered, S, G)
        result, bad = check(cw, d, g, G)
        assert result == want and bad[1:1 + n].tolist() == flags.tolist()
        assert bad[0] == 0xEEEEEEEE and (bad[1 + n:] == 0xEEEEEEEE).all()                   # no flag outside the groups checked
        assert check(cw, d, g, G, flags=False)[0] == want
        assert g.covered() == covered
        return result
    g = Guard(guards(covered, G), covered)
    assert expect(d_store, g) == [0, n, 0, GM.NONE]
    for at in (0, W - 1, W, covered - 1):                                                     # one flipped store byte
        hurt = host.copy()
        hurt[at] ^= 0x10
        assert expect(_dev_bytes(hurt), g, hurt_store=hurt) == [0, n, 1, at // W]
    for at in (5, (n - 1) * S + S - 1):                                                      # one flipped guard byte
        hurt = guards(covered, G).copy()
        hurt[at] ^= 0x01
        assert expect(d_store, Guard(hurt, covered), hurt_guard=hurt) == [0, n, 1, at // S]
    hurt = host.copy()                                                                          # above the cursor: not seen
    hurt[covered] ^= 0xFF
    hurt[BYTES - 1] ^= 0xFF
    assert expect(_dev_bytes(hurt), g, hurt_store=hurt) == [0, n, 0, GM.NONE]
    both = host.copy()                                                                          # two groups, the lowest reported
    both[3] ^= 1
    both[covered - 1] ^= 1
    assert expect(_dev_bytes(both), g, hurt_store=both) == [0, n, 2, 0]
    assert check(cw, d_store, Guard(guards(covered, G), BYTES + 1), G)[0] == [1, 0, 0, GM.NONE]
    assert check(cw, d_store, Guard(guards(0, G), 0), G)[0] == [0, 0, 0, GM.NONE]
    full = Guard(guards(BYTES, G), BYTES)
    assert check(cw, d_store, full, G)[0] == [0, -(-BYTES // W), 0, GM.NONE]


# ---- 3. rebuild -----------------------------------------------------------------------------------------------------------------------
def rebuild(cw, d_store, directory, dir_base, guard, G, values, out_bytes, count=None, max_count=None, store_bytes=BYTES, S=S):
    """cw_dev_store_guard_rebuild into poisoned buffers: (result[4], statuses with a pad, the out_bytes of d_out, d_out_loc with a pad)."""
    n = len(values)
    max_count = n if max_count is None else max_count
    d_dir = _dev_bytes(np.ascontiguousarray(directory, RM.LOC))
    d_val, d_count = _dev_u64(list(values) + [0]), _dev_u64([n if count is None else count])
    out = _dev_bytes(np.full(out_bytes + 2 * PAD, 0xEE, np.uint8))
    loc = _dev_bytes(np.full(2 * (max_count + 2), 0xEEEEEEEEEEEEEEEE, np.uint64))
    status, result = _dev_bytes(np.full(max_count + 2, 0xEEEEEEEE, np.uint32)), _dev_u64([7, 7, 7, 7])
    _sync()
    cw.dev_store_guard_rebuild(d_store.data_ptr(), store_bytes, d_dir.data_ptr(), dir_base, len(directory), guard.d_covered.data_ptr(), S, G, guard.ptr(),
                               guard.size, d_val.data_ptr(), d_count.data_ptr(), max_count, out.data_ptr() + PAD if out_bytes else 0, out_bytes,
                               loc.data_ptr() + 16, status.data_ptr() + 4, result.data_ptr(), _stream())
    _sync()
    h = out.cpu().numpy()
    assert (h[:PAD] == 0xEE).all() and (h[PAD + out_bytes:] == 0xEE).all(), "a store left d_out"
    locs, st = loc.cpu().numpy().view(np.uint64), status.cpu().numpy().view(np.uint32)
    assert (locs[:2] == 0xEEEEEEEEEEEEEEEE).all() and (locs[-2:] == 0xEEEEEEEEEEEEEEEE).all() and st[0] == st[-1] == 0xEEEEEEEE
    guard.host()                                                                                # (the guard is only read)
    return _u64(result).tolist(), st[1:-1], h[PAD:PAD + out_bytes], locs[2:-2].view(RM.LOC)


def compare(cw, d_store, hurt, directory, dir_base, guard, covered, G, values, original=None, store_bytes=BYTES, S=S):
    """One rebuild with exactly the room it needs, against the model; then the dry run and a buffer one byte too small."""
    want, wst, wout, wlocs = GM.rebuild(hurt, store_bytes, directory, dir_base, covered, S, G, guard.host(), values, 1 << 62)
    total = want[1]
    result, st, out, locs = rebuild(cw, d_store, directory, dir_base, guard, G, values, total, store_bytes=store_bytes, S=S)
    assert result == want and st.tolist() == wst.tolist()
    assert (out == wout).all() and (locs == wlocs).all()
    for room in sorted({0, max(total - 1, 0)}) if total else []:
        result, st, out, locs = rebuild(cw, d_store, directory, dir_base, guard, G, values, room, store_bytes=store_bytes, S=S)
        assert result == [1] + want[1:] and st.tolist() == wst.tolist()
        assert (out == 0xEE).all() and (locs.view(np.uint64) == 0xEEEEEEEEEEEEEEEE).all()       # nothing but status and result
    return wst.tolist()


@pytest.mark.parametrize("G", GROUPS)
def test_rebuild_cases(cw, store, guards, G):
    host, d_store = store
    for name, (entries, values, covered, wanted) in GM.rebuild_cases(G).items():
        directory = np.array(entries, RM.LOC)
        hurt = host.copy()
        for v in values:
            e = GM.extent_of(directory, 0, v, BYTES, covered)
            if e:
                for at in {e[0], e[0] + e[1] // 2, e[0] + e[1] - 1}:
                    hurt[at] = host[at] ^ 0xA5
        g = Guard(guards(covered, G), covered)
        assert compare(cw, _dev_bytes(hurt), hurt, directory, 0, g, covered, G, values) == wanted, name
        # and the bytes are the original ones
        total = sum(int(directory[v]["stored"]) for v, s in zip(values, wanted) if s == 0)
        _, _, out, locs = rebuild(cw, _dev_bytes(hurt), directory, 0, g, G, values, total)
        for k, (v, s) in enumerate(zip(values, wanted)):
            if s == 0:
                pos, n = int(directory[v]["pos"]), int(directory[v]["stored"])
                at = int(locs[k]["pos"])
                assert (out[at:at + n] == host[pos:pos + n]).all(), (name, k)


@pytest.mark.parametrize("G", GROUPS)
def test_rebuild_counts_and_cursor(cw, store, guards, G):
    host, d_store = store
    entries, values, covered, _ = GM.rebuild_cases(G)["unprotected"]
    directory, g = np.array(entries, RM.LOC), Guard(guards(covered, G), covered)
    # the count on the device, clamped by max_count; positions at or past n are not written
    for count, max_count in ((len(values) + 5, len(values)), (3, len(values)), (0, len(values)), (len(values), 2), (len(values), 0)):
        n = min(count, max_count)
        want, wst, wout, wlocs = GM.rebuild(host, BYTES, directory, 0, covered, S, G, g.host(), values[:n], BYTES)
        result, st, out, locs = rebuild(cw, d_store, directory, 0, g, G, values, want[1], count=count, max_count=max_count)
        assert result == want and st[:n].tolist() == wst.tolist() and (st[n:] == 0xEEEEEEEE).all(), (count, max_count)
        assert (out == wout).all() and (locs[:n] == wlocs).all() and (locs[n:].view(np.uint64) == 0xEEEEEEEEEEEEEEEE).all()
    # a directory base, and values below it
    compare(cw, d_store, host, directory, DIR_BASE, g, covered, G, [DIR_BASE + 2, 2, DIR_BASE - 1, DIR_BASE + 3, DIR_BASE])
    # an inconsistent cursor protects nothing: verdict 2, nothing but status and result
    bad = Guard(guards(covered, G), BYTES + 1)
    result, st, out, locs = rebuild(cw, d_store, directory, 0, bad, G, values, 4096)
    assert result == [2, 0, len(values), 0] and (st == 2).all() and (out == 0xEE).all() and (locs.view(np.uint64) == 0xEEEEEEEEEEEEEEEE).all()


@pytest.mark.parametrize("G", GROUPS)
def test_rebuild_many_positions(cw, store, guards, G):
    """Several hundred listed extents over more than one workgroup, duplicates and collisions among them: every status and byte."""
    host, d_store = store
    rng = np.random.default_rng(100 + G)
    entries, at = [], 0
    while at < BYTES - 70000:
        n = int(rng.integers(1, 800)) if len(entries) != 7 else 65536
        entries.append(GM.entry(at, n))
        at += n + int(rng.integers(0, 1200))
    directory = np.array(entries, RM.LOC)
    assert len(directory) > 150
    for picks in (600, 40):
        values = rng.integers(0, len(directory), picks).tolist()
        covered = BYTES if picks == 40 else 4 * S + 777
        hurt = host.copy()
        for v in set(values):
            e = GM.extent_of(directory, 0, v, BYTES, covered)
            if e:
                hurt[e[0]:e[0] + e[1]] ^= 0x3C
        statuses = compare(cw, _dev_bytes(hurt), hurt, directory, 0, Guard(guards(covered, G), covered), covered, G, values)
        assert set(statuses) >= ({1, 2} if picks == 600 else {0}), picks


# ---- 4. whole stores ------------------------------------------------------------------------------------------------------------------
def text():
    return corpus_file("alice29.txt") + corpus_file("asyoulik.txt") + corpus_file("lcet10.txt") + corpus_file("plrabn12.txt")[:300000]


def directory_of(cs):
    return cs.d_dir.cpu().numpy().view(RM.LOC).copy()


def assert_guarded(cs):
    """protected_bytes() == used(), and the guard is the model's over the stored bytes."""
    used = cs.used()
    assert cs.protected_bytes() == used
    want = GM.guard_of(cs.d_store.cpu().numpy(), used, cs.stripe, cs.group, max(cs.store_bytes, 1))
    assert (cs.d_guard.cpu().numpy() == want).all()
    assert cs.guard_check() == (0, [])


def flip(cs, d, values, mask=0x5C, where=None):
    """One flipped byte in each value's stored extent, in its middle unless `where` says otherwise: the positions."""
    at = [(where or {}).get(v, int(d[v - cs.dir_base]["pos"]) + int(d[v - cs.dir_base]["stored"]) // 2) for v in values]
    for p in at:
        cs.d_store[p] ^= mask
    _sync()
    return at


@pytest.mark.parametrize("alg", ALGS)
def test_protect_damage_scrub_repair(cw, alg):
    data, G = text(), 2
    W = G * S
    streams = [data[:450000], data[380000:900000]]
    index = cw.DedupeIndex("skein", 4096)
    try:
        cs = cw.ChunkStore(index, alg, cw.CdcParams(normal_size=1024), 1 << 20, 1100, DIR_BASE)
        assert cs.protected_bytes() == 0
        with pytest.raises(cw.CwError):
            cs.guard_check()
        with pytest.raises(ValueError):
            cs.protect(stripe=65536 * 3)
        cs.protect(stripe=S, group=G)
        assert_guarded(cs)
        recs = []
        for s in streams:
            recs.append(cs.ingest(s))
            assert_guarded(cs)
        used, d = cs.used(), directory_of(cs)
        assert used > 5 * S
        # victims: two chunks of group 0 that share a column (one in each stripe), and one chunk in each of three other stripes
        full = [i for i in range(len(d)) if d[i]["stored"]]
        inside = lambda i, p: int(d[i]["pos"]) <= p < int(d[i]["pos"]) + int(d[i]["stored"])  # noqa: E731
        a = next(i for i in full if int(d[i]["pos"]) > 3000)
        b = next(i for i in full if inside(i, int(d[a]["pos"]) + S))
        others = [next(i for i in full if int(d[i]["pos"]) >= t * S + c) for t, c in ((2, 20000), (3, 40000), (4, 20000))]
        assert a < b < min(others) and int(d[max(others)]["pos"]) < 5 * S
        victims = sorted(DIR_BASE + i for i in [a, b] + others)
        before = cs.d_store.cpu().numpy().copy()
        # (b's damaged byte lies in the column of a's first byte)
        at = dict(zip(victims, flip(cs, d, victims, where={DIR_BASE + b: int(d[a]["pos"]) + S})))
        report = cs.scrub()
        assert report.damaged.tolist() == victims
        hurt = cs.d_store.cpu().numpy()
        want = GM.rebuild(hurt, cs.store_bytes, d, DIR_BASE, used, S, G, cs.d_guard.cpu().numpy(), victims, 1 << 20)[1].tolist()
        collided = [v for v, s in zip(victims, want) if s == 1]
        assert collided == sorted([DIR_BASE + a, DIR_BASE + b]) and want.count(0) == 3
        count = index.count()
        out = cs.repair_local(report)
        assert out == dict(repaired=[v for v, s in zip(victims, want) if s == 0], collided=collided, unprotected=[], failed=[], no_digest=[])
        # in place: nothing moved, nothing grew, the index was not written; the repaired bytes are the original ones
        assert cs.used() == used and cs.protected_bytes() == used and (directory_of(cs) == d).all() and index.count() == count
        now = cs.d_store.cpu().numpy()
        differ = np.nonzero(now != before)[0].tolist()
        assert differ == sorted(at[v] for v in collided)
        again = cs.scrub()
        assert again.damaged.tolist() == collided
        assert cs.guard_check() == (len({at[v] // W for v in collided}), sorted({at[v] // W for v in collided}))
        restored = 0
        for r, s in zip(recs, streams):
            if set(r.refs.tolist()) & set(collided):
                with pytest.raises(cw.CwError):
                    cs.restore(r, verify=True)
            else:
                assert cs.restore(r, verify=True) == s
                restored += 1
        assert restored == 1
        assert cs.repair_local(again) == dict(repaired=[], collided=collided, unprotected=[], failed=[], no_digest=[])
        # one of the two at a time: each is rebuilt once the other is no longer listed
        for v in collided:
            one = cw.ScrubReport(np.where(np.arange(1100) == v - DIR_BASE, 3, 0).astype(np.uint32), {}, DIR_BASE)
            if v == collided[0]:
                # ... but the other is still damaged, in the same column: the rebuilt bytes are wrong, and verify says so
                assert cs.repair_local(one) == dict(repaired=[], collided=[], unprotected=[], failed=[v], no_digest=[])
                cs.d_store[at[collided[1]]] ^= 0x5C                                          # the other one heals by itself
                _sync()
            assert cs.repair_local(one) == dict(repaired=[v], collided=[], unprotected=[], failed=[], no_digest=[])
        assert (cs.d_store.cpu().numpy() == before).all()
        assert cs.scrub().clean
        assert_guarded(cs)
        for r, s in zip(recs, streams):
            assert cs.restore(r, verify=True) == s
        # a value without a digest, an entry that is gone and a value outside the directory
        gone = DIR_BASE + others[0]
        lost = DIR_BASE + others[1]
        live = np.ones(1100, np.int32)
        live[lost - DIR_BASE] = 0
        import torch
        d_live = torch.from_numpy(live).cuda()
        _sync()
        index.retain(d_live.data_ptr(), DIR_BASE, 1100)
        cs.d_dir[2 * (gone - DIR_BASE):2 * (gone - DIR_BASE) + 2] = 0
        _sync()
        report = cw.ScrubReport(np.where(np.isin(np.arange(1100), [gone - DIR_BASE, lost - DIR_BASE]), 2, 0).astype(np.uint32), {}, DIR_BASE)
        assert cs.repair_local(report) == dict(repaired=[], collided=[], unprotected=[gone], failed=[], no_digest=[lost])
        with pytest.raises(cw.CwError):
            cs.repair_local(cw.ScrubReport(np.array([3], np.uint32), {}, DIR_BASE + 5000))
        assert cs.repair_local(cw.ScrubReport(np.zeros(1100, np.uint32), {}, DIR_BASE)) == dict(repaired=[], collided=[], unprotected=[], failed=[],
                                                                                                  no_digest=[])
    finally:
        index.close()


@pytest.mark.parametrize("alg", ALGS)
def test_every_appending_method_keeps_the_guard(cw, alg):
    data = text()
    ia, ib = cw.DedupeIndex("skein", 4096), cw.DedupeIndex("skein", 4096)
    try:
        p = cw.CdcParams(normal_size=1024)
        A, B = cw.ChunkStore(ia, alg, p, 1 << 20, 1500, DIR_BASE), cw.ChunkStore(ib, alg, p, 1 << 20, 1500, 5)
        A.protect(group=3)
        B.protect(stripe=1 << 17, group=2)
        r0 = A.ingest(data[:150000])
        assert_guarded(A)
        r1, r2 = A.ingest_many([data[100000:200000], data[500000:560000]])
        assert_guarded(A)
        r3 = A.ingest_stream(data[600000:700000])
        assert_guarded(A)
        r4, = A.ingest_many_stream([data[650000:760000]])
        assert_guarded(A)
        r5 = A.write(r0, 70000, b"guard stripes " * 500)
        assert_guarded(A)
        r6 = A.append(A.truncate(r5, 120000), data[800000:830000])
        assert_guarded(A)
        r7 = A.compose([(r1, 1000, 50000), b"between", (r3, 0, 60000)])
        assert_guarded(A)
        r8 = A.edit(r2, [(100, 50, b"edited"), (30000, 0, data[:5000])])
        assert_guarded(A)
        recs = [r0, r1, r2, r3, r4, r5, r6, r7, r8]
        theirs = A.replicate_to(B, recs)                                                      # import_bundle
        assert_guarded(B)
        used = A.used()
        d = directory_of(A)
        victim = int(r0.refs[7])
        at, = flip(A, d, [victim])
        report = A.scrub()
        assert report.damaged.tolist() == [victim]
        assert A.repair_from(B, report)["repaired"] == [victim]                                # appends the peer's copy
        assert A.used() > used and A.protected_bytes() == A.used()
        assert A.guard_check() == (1, [at // (3 * S)])            # the old bytes stay, damaged, until a compact
        flip(A, d, [victim])
        assert_guarded(A)
        # a refused call appends nothing and leaves guard and cursor as they were
        small = cw.ChunkStore(ib, alg, p, B.used() + 90000, 1500, 5)
        small.d_store[:B.used()] = B.d_store[:B.used()]
        small.d_dir.copy_(B.d_dir)
        small.d_used.copy_(B.d_used)
        small.base = B.base
        _sync()
        small.protect(stripe=1 << 16, group=2)
        assert_guarded(small)
        with pytest.raises(cw.CwError) as e:
            small.ingest(np.random.default_rng(3).bytes(100000))
        assert e.value.code == NOMEM
        assert_guarded(small)
        with cw.tuned(CW_STORE_PIECE=65536):
            with pytest.raises(cw.CwError) as e:
                small.ingest_stream(data[860000:1000000] + np.random.default_rng(4).bytes(200000))
        assert e.value.code == NOMEM and e.value.consumed > 0 and small.used() > B.used()
        assert_guarded(small)                                                                   # the prefix that went in is folded
        # compact: a fresh guard over the new store; renumber: the guard stays as it is
        A.compact(recs[:4])
        assert_guarded(A)
        guard = A.d_guard.cpu().numpy().copy()
        kept = A.renumber(recs[:4])
        assert (A.d_guard.cpu().numpy() == guard).all()
        assert_guarded(A)
        d = directory_of(A)
        victim = int(kept[1].refs[3])
        flip(A, d, [victim])
        report = A.scrub()
        assert report.damaged.tolist() == [victim] and A.repair_local(report)["repaired"] == [victim]
        assert A.scrub().clean and A.restore(kept[1], verify=True) == data[100000:200000]
        assert_guarded(A)
        assert theirs and B.restore(theirs[7], verify=True) == A.restore(kept[1], verify=True)[1000:51000] + b"between" + data[600000:660000]
    finally:
        ia.close()
        ib.close()


@pytest.mark.parametrize("alg", ALGS)
def test_save_and_load(cw, alg, tmp_path):
    data = text()
    index = cw.DedupeIndex("skein", 4096)
    loaded = []
    try:
        cs = cw.ChunkStore(index, alg, cw.CdcParams(normal_size=1024), 1 << 20, 900, DIR_BASE)
        rec = cs.ingest(data[:300000])
        plain = str(tmp_path / "plain.npz")
        cs.save(plain)
        with np.load(plain) as z:
            assert not [k for k in z.files if "guard" in k]                                   # an unprotected store: the file as it always was
        loaded.append(cw.ChunkStore.load(plain))
        assert loaded[-1].d_guard is None and loaded[-1].protected_bytes() == 0
        cs.protect(stripe=S, group=3)
        path = str(tmp_path / "guarded.npz")
        cs.save(path)
        with np.load(path) as z:
            assert sorted(k for k in z.files if "guard" in k) == ["guard", "guard_covered", "guard_geometry"]
            assert int(z["guard_covered"]) == cs.used() and z["guard_geometry"].tolist() == [S, 3] and len(z["guard"]) == -(-cs.used() // (3 * S)) * S
        back = cw.ChunkStore.load(path)
        loaded.append(back)
        assert (back.stripe, back.group) == (S, 3)
        assert_guarded(back)
        assert (back.d_guard.cpu().numpy() == cs.d_guard.cpu().numpy()).all()
        victim = int(rec.refs[11])
        flip(back, directory_of(back), [victim])
        report = back.scrub()
        assert report.damaged.tolist() == [victim]
        assert back.repair_local(report) == dict(repaired=[victim], collided=[], unprotected=[], failed=[], no_digest=[])
        assert back.scrub().clean and back.restore(rec, verify=True) == data[:300000]
        more = back.ingest(data[300000:400000])                                                 # and it goes on folding
        assert_guarded(back)
        assert back.restore(more) == data[300000:400000]
    finally:
        index.close()
        for cs in loaded:
            cs.index.close()


def test_both_repairs_select_entries_alike(cw):
    """repair_local and repair_from take one report: the same value without a digest from both, the same refusal of a value below
    dir_base.  Two chunks of one small stream are damaged; the one whose digest the index has lost gets a first token without literals,
    a match at output position 0, so that it cannot decode and a scrub lists it as damaged, not as an orphan."""
    import torch
    data, base, entries = corpus_file("alice29.txt")[:65536], 5, 4096
    ia, ib = cw.DedupeIndex("skein", 4096), cw.DedupeIndex("skein", 4096)
    try:
        A, B = (cw.ChunkStore(i, "lz4", cw.CdcParams.default(256), 1 << 20, entries, base) for i in (ia, ib))
        recipe = A.ingest(data)
        assert (B.ingest(data).refs == recipe.refs).all()
        A.protect(65536, 4)
        d = directory_of(A)
        full = [i for i in range(entries) if d[i]["stored"]]
        packed = [i for i in full if not int(d[i]["raw"]) & RM.RAW]
        lost, hit = base + packed[len(packed) // 2], base + full[3]
        assert lost != hit
        token = int(A.d_store[int(d[lost - base]["pos"])].item())
        assert token & 0xF0
        flip(A, d, [lost], mask=token & 0xF0, where={lost: int(d[lost - base]["pos"])})
        flip(A, d, [hit])
        live = np.ones(entries, np.int32)
        live[lost - base] = 0
        d_live = torch.from_numpy(live).cuda()
        _sync()
        assert ia.retain(d_live.data_ptr(), base, entries) == 1
        report = A.scrub()
        assert report.damaged.tolist() == sorted([lost, hit]) and len(report.orphans) == 0
        first = A.repair_local(report)
        assert first == dict(repaired=[hit], collided=[], unprotected=[], failed=[], no_digest=[lost])
        assert A.repair_from(B, report)["no_digest"] == [lost]
        # neither call could judge the chunk without a digest, and neither touched it: its positions, and only they, do not restore;
        # with its own byte put back, the stream is whole again
        assert directory_of(A)[lost - base] == d[lost - base] and int(A.d_store[int(d[lost - base]["pos"])].item()) == token & 0x0F
        with pytest.raises(cw.CwError) as e:
            A.restore(recipe)
        assert e.value.code == -2 and f": {int((recipe.refs == lost).sum())} of {len(recipe.refs)} positions not restored" in str(e.value)
        flip(A, d, [lost], mask=token & 0xF0, where={lost: int(d[lost - base]["pos"])})
        assert A.restore(recipe, verify=False) == data
        below = cw.ScrubReport(np.array([3], np.uint32), {}, base - 1)
        assert below.damaged.tolist() == [base - 1]
        texts = []
        for repair in (A.repair_local, lambda r: A.repair_from(B, r)):
            with pytest.raises(cw.CwError) as e:
                repair(below)
            assert e.value.code == -2
            texts.append(str(e.value))
        assert texts[0] == texts[1] == f"libcwhc error -2: chunk store: the report names values outside the directory [{base}, {base + entries})"
    finally:
        ia.close()
        ib.close()
