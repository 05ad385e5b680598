"""The dual guard on the GPU (cw_dev_store_guard2_update, _check, _rebuild and cw.ChunkStore.protect(parity=2) / guard_check /
repair_local): everything compared exactly with guard2_model.py.  S = 65536 with G = 2 and G = 3 over a store of
six stripes and a few bytes, G = 255 over one of 256 stripes and a few bytes, hand-built directories with poison around every output
and list; then whole stores of corpus text: protect, ingest, damage pairs of chunks that meet in guard bytes, scrub, repair both."""
import numpy as np
import pytest

import guard2_model as G2
import guard_model as GM
import restore_model as RM
from conftest import corpus_file, corpus_names
from test_gpu_guard import DIR_BASE, PAD, Guard, _dev_bytes, _dev_u64, _stream, _sync, _u64, directory_of, flip, text

pytestmark = pytest.mark.gpu

ALGS = ["lz4", "lzf"]
GROUPS = [2, 3]
S, BYTES, BYTES_255 = G2.S, G2.STORE_BYTES, G2.STORE_BYTES_255
POISON64 = 0xEEEEEEEEEEEEEEEE


@pytest.fixture(scope="module")
def cw():
    import torch  # noqa: F401  (one HIP runtime for torch and libcwhc.so)
    import compute_war_amd as cw
    cw.init(0)
    yield cw
    cw.tune_reset()


class Stored:
    """Noise on the host and on the device, neither written, and the model's (P, Q) for the cursors the tests use, each computed once."""

    def __init__(self, n, seed, S=S):
        self.n, self.S = n, S
        self.host = np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)
        self.dev = _dev_bytes(self.host)
        self.cache = {}

    def guards(self, covered, G):
        if (covered, G) not in self.cache:
            self.cache[covered, G] = G2.guards_of(self.host, covered, self.S, G, self.n)
        return self.cache[covered, G]


@pytest.fixture(scope="module")
def store(cw):
    return Stored(BYTES, 29)


@pytest.fixture(scope="module")
def store255(cw):
    return Stored(BYTES_255, 255)


class Guards:
    """P and Q on the device, each between two poisoned pads, with the one cursor."""

    def __init__(self, pq, covered, size=None):
        self.p, self.q = Guard(pq[0], covered, size), Guard(pq[1], covered, size)
        self.d_covered, self.size = self.p.d_covered, self.p.size

    def host(self):
        return self.p.host(), self.q.host()

    def covered(self):
        return int(_u64(self.d_covered)[0])

    def equal(self, pq):
        p, q = self.host()
        return (p[:len(pq[0])] == pq[0]).all() and (q[:len(pq[1])] == pq[1]).all() and not p[len(pq[0]):].any() and not q[len(pq[1]):].any()


def update(cw, d_store, g, used, G, store_bytes=BYTES, S=S):
    d_used, result = _dev_u64([used]), _dev_u64([7, 7, 7, 7, POISON64])
    _sync()
    cw.dev_store_guard2_update(d_store.data_ptr(), store_bytes, d_used.data_ptr(), g.d_covered.data_ptr(), S, G, g.p.ptr(), g.q.ptr(), g.size,
                               result.data_ptr(), _stream())
    _sync()
    r = _u64(result).tolist()
    assert r[4] == POISON64
    return r[:4]


def update_p_only(cw, d_store, guard, used, G, store_bytes=BYTES, S=S):
    d_used, result = _dev_u64([used]), _dev_u64([7, 7, 7, 7])
    _sync()
    cw.dev_store_guard_update(d_store.data_ptr(), store_bytes, d_used.data_ptr(), guard.d_covered.data_ptr(), S, G, guard.ptr(), guard.size,
                              result.data_ptr(), _stream())
    _sync()
    return _u64(result).tolist()


# ---- 1. update ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", GROUPS)
def test_update_ranges(cw, store, G):
    for name, (a, b) in GM.update_ranges(G).items():
        g = Guards(store.guards(a, G), a)
        assert update(cw, store.dev, g, b, G) == [0, a, b, b - a], name
        assert g.covered() == b and g.equal(store.guards(b, G)), name
        assert update(cw, store.dev, g, b, G) == [0, b, b, 0], name                             # twice: nothing the second time
        assert g.covered() == b and g.equal(store.guards(b, G)), name
        single = Guard(store.guards(a, G)[0], a)                                                # P is the single guard's, bit for bit
        assert update_p_only(cw, store.dev, single, b, G) == [0, a, b, b - a], name
        assert (single.host() == g.p.host()).all(), name


@pytest.mark.parametrize("G", GROUPS)
def test_update_refuses_an_inconsistent_cursor(cw, store, G):
    for used, covered in ((999, 1000), (BYTES + 1, 1000), (BYTES + 1, BYTES + 1)):
        g = Guards(store.guards(1000, G), covered)
        assert update(cw, store.dev, g, used, G) == [1, covered, used, 0]
        assert g.covered() == covered and g.equal(store.guards(1000, G))
    # a store whose size is no multiple of 16, used to its last byte, in a tensor that ends there; and larger guards than needed
    for cut in (0, 5, 21):
        n = BYTES - cut
        zero = store.guards(0, G)
        g = Guards(zero, 0, size=len(zero[0]) + S)
        exact = store.dev[:n].clone()
        assert update(cw, exact, g, n, G, store_bytes=n) == [0, 0, n, n]
        assert g.equal(store.guards(n, G)), cut


@pytest.mark.parametrize("G", GROUPS)
def test_many_small_updates_equal_one_large(cw, store, G):
    """Queued one behind the other with no synchronise between them, each behind the write of the cursor it reads."""
    cuts = sorted(set(np.random.default_rng(G).integers(0, BYTES, 40).tolist()) | {S, G * S, BYTES})
    g = Guards(store.guards(0, G), 0)
    d_used, results = _dev_u64(cuts), _dev_u64(np.zeros(4 * len(cuts)))
    _sync()
    for k in range(len(cuts)):
        cw.dev_store_guard2_update(store.dev.data_ptr(), BYTES, d_used.data_ptr() + 8 * k, g.d_covered.data_ptr(), S, G, g.p.ptr(), g.q.ptr(), g.size,
                                   results.data_ptr() + 32 * k, _stream())
    _sync()
    want = [[0, a, b, b - a] for a, b in zip([0] + cuts[:-1], cuts)]
    assert _u64(results).reshape(-1, 4).tolist() == want
    assert g.covered() == BYTES and g.equal(store.guards(BYTES, G))


def test_update_with_255_members(cw, store255):
    """One range from member 254 of group 0 into member 0 of group 1, then the rest of the store."""
    a, b = G2.update_range_255()
    g = Guards(store255.guards(a, 255), a)
    assert update(cw, store255.dev, g, b, 255, store_bytes=BYTES_255) == [0, a, b, b - a]
    assert g.covered() == b and g.equal(store255.guards(b, 255))
    assert update(cw, store255.dev, g, BYTES_255, 255, store_bytes=BYTES_255) == [0, b, BYTES_255, BYTES_255 - b]
    assert g.equal(store255.guards(BYTES_255, 255))
    whole = Guards(store255.guards(0, 255), 0)
    assert update(cw, store255.dev, whole, BYTES_255, 255, store_bytes=BYTES_255) == [0, 0, BYTES_255, BYTES_255]
    assert whole.equal(store255.guards(BYTES_255, 255))


# ---- 2. check -------------------------------------------------------------------------------------------------------------------------
def check(cw, d_store, g, G, flags=True, store_bytes=BYTES, S=S):
    n = g.size // S
    bad, result = _dev_bytes(np.full(n + 2, 0xEEEEEEEE, np.uint32)), _dev_u64([7, 7, 7, 7, POISON64])
    _sync()
    cw.dev_store_guard2_check(d_store.data_ptr(), store_bytes, g.d_covered.data_ptr(), S, G, g.p.ptr(), g.q.ptr(), g.size,
                              bad.data_ptr() + 4 if flags else 0, result.data_ptr(), _stream())
    _sync()
    r = _u64(result).tolist()
    assert r[4] == POISON64
    return r[:4], bad.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("G", GROUPS)
def test_check(cw, store, G):
    host, d_store = store.host, store.dev
    W, covered = G * S, 4 * S + 1000
    n = -(-covered // W)                                                                        # (the last group is partial)
    good = store.guards(covered, G)

    def expect(d, g, hurt_store=None, hurt=None):
        pq = good if hurt is None else hurt
        want, bits = G2.check(pq[0], pq[1], host if hurt_store is None else hurt_store, BYTES, covered, S, G)
        result, bad = check(cw, d, g, G)
        assert result == want and bad[1:1 + n].tolist() == bits.tolist()
        assert bad[0] == 0xEEEEEEEE and (bad[1 + n:] == 0xEEEEEEEE).all()                   # no flag outside the groups checked
        assert check(cw, d, g, G, flags=False)[0] == want
        assert g.covered() == covered and g.equal(pq)                                           # (the guards are only read)
        return result, bad[1:1 + n].tolist()
    g = Guards(good, covered)
    assert expect(d_store, g) == ([0, n, 0, GM.NONE], [0] * n)
    for at in (0, W - 1, W, covered - 1):                                                     # one flipped store byte: both bits
        hurt = host.copy()
        hurt[at] ^= 0x10
        result, bits = expect(_dev_bytes(hurt), g, hurt_store=hurt)
        assert result == [0, n, 1, at // W] and bits[at // W] == 3
    for at in (5, (n - 1) * S + S - 1):                                                      # one flipped guard byte: its own bit
        for which in (0, 1):
            hurt = [good[0].copy(), good[1].copy()]
            hurt[which][at] ^= 0x01
            result, bits = expect(d_store, Guards(hurt, covered), hurt=hurt)
            assert result == [0, n, 1, at // S] and bits[at // S] == 1 << which
    hurt = [good[0].copy(), good[1].copy()]                                                     # P of one group, Q of another
    hurt[0][S + 7] ^= 0x80
    hurt[1][3] ^= 0x80
    assert expect(d_store, Guards(hurt, covered), hurt=hurt) == ([0, n, 2, 0], [2, 1] + [0] * (n - 2))
    hurt = host.copy()                                                                          # above the cursor: not seen
    hurt[covered] ^= 0xFF
    hurt[BYTES - 1] ^= 0xFF
    assert expect(_dev_bytes(hurt), g, hurt_store=hurt)[0] == [0, n, 0, GM.NONE]
    assert check(cw, d_store, Guards(good, BYTES + 1), G)[0] == [1, 0, 0, GM.NONE]              # a cursor above the store
    assert check(cw, d_store, Guards(store.guards(0, G), 0), G)[0] == [0, 0, 0, GM.NONE]
    assert check(cw, d_store, Guards(store.guards(BYTES, G), BYTES), G)[0] == [0, -(-BYTES // W), 0, GM.NONE]


def test_check_with_255_members(cw, store255):
    good = store255.guards(BYTES_255, 255)
    result, bad = check(cw, store255.dev, Guards(good, BYTES_255), 255, store_bytes=BYTES_255)
    assert result == [0, 2, 0, GM.NONE] and bad.tolist() == [0xEEEEEEEE, 0, 0, 0xEEEEEEEE]
    hurt = store255.host.copy()
    hurt[254 * S + 9] ^= 4
    assert check(cw, _dev_bytes(hurt), Guards(good, BYTES_255), 255, store_bytes=BYTES_255)[1].tolist()[1:3] == [3, 0]


# ---- 3. rebuild -----------------------------------------------------------------------------------------------------------------------
def rebuild(cw, d_store, store_bytes, directory, dir_base, g, G, values, out_bytes, count=None, max_count=None, S=S):
    """cw_dev_store_guard2_rebuild into poisoned buffers: (result[5], statuses, the out_bytes of d_out, d_out_loc)."""
    n = len(values)
    max_count = n if max_count is None else max_count
    d_dir = _dev_bytes(np.ascontiguousarray(directory, RM.LOC))
    d_val, d_count = _dev_u64(list(values) + [0]), _dev_u64([n if count is None else count])
    out = _dev_bytes(np.full(out_bytes + 2 * PAD, 0xEE, np.uint8))
    loc = _dev_bytes(np.full(2 * (max_count + 2), POISON64, np.uint64))
    status, result = _dev_bytes(np.full(max_count + 2, 0xEEEEEEEE, np.uint32)), _dev_u64([7, 7, 7, 7, 7, POISON64])
    _sync()
    cw.dev_store_guard2_rebuild(d_store.data_ptr(), store_bytes, d_dir.data_ptr(), dir_base, len(directory), g.d_covered.data_ptr(), S, G, g.p.ptr(),
                                g.q.ptr(), g.size, d_val.data_ptr(), d_count.data_ptr(), max_count, out.data_ptr() + PAD if out_bytes else 0,
                                out_bytes, loc.data_ptr() + 16, status.data_ptr() + 4, result.data_ptr(), _stream())
    _sync()
    h = out.cpu().numpy()
    assert (h[:PAD] == 0xEE).all() and (h[PAD + out_bytes:] == 0xEE).all(), "a store left d_out"
    locs, st, r = loc.cpu().numpy().view(np.uint64), status.cpu().numpy().view(np.uint32), _u64(result).tolist()
    assert (locs[:2] == POISON64).all() and (locs[-2:] == POISON64).all() and st[0] == st[-1] == 0xEEEEEEEE and r[5] == POISON64
    g.host()                                                                                    # (the guards are only read)
    return r[:5], st[1:-1], h[PAD:PAD + out_bytes], locs[2:-2].view(RM.LOC)


def compare(cw, d_store, hurt, store_bytes, directory, dir_base, g, covered, G, values, S=S):
    """One rebuild with exactly the room it needs, against the model; then the dry run and a buffer one byte too small."""
    p, q = g.host()
    want, wst, wout, wlocs = G2.rebuild(hurt, store_bytes, directory, dir_base, covered, S, G, p, q, values, 1 << 62)
    total = want[1]
    result, st, out, locs = rebuild(cw, d_store, store_bytes, directory, dir_base, g, G, values, total, S=S)
    assert result == want and st.tolist() == wst.tolist()
    assert (out == wout).all() and (locs == wlocs).all()
    for room in sorted({0, max(total - 1, 0)}) if total else []:
        result, st, out, locs = rebuild(cw, d_store, store_bytes, directory, dir_base, g, G, values, room, S=S)
        assert result == [1] + want[1:] and st.tolist() == wst.tolist()
        assert (out == 0xEE).all() and (locs.view(np.uint64) == POISON64).all()                 # nothing but status and result
    return wst.tolist(), want[4], wout, wlocs


def run_cases(cw, stored, G, single=None):
    host, n, S = stored.host, stored.n, stored.S
    for name, (entries, values, covered, wanted, need_q) in G2.rebuild_cases(G, n, S, single).items():
        directory = np.array(entries, RM.LOC)
        hurt = host.copy()                                                                      # damaged after the guards were built
        for v in values:
            e = GM.extent_of(directory, 0, v, n, covered)
            if e:
                hurt[e[0]:e[0] + e[1]] ^= 0xA5
        g = Guards(stored.guards(covered, G), covered)
        statuses, paired, out, locs = compare(cw, _dev_bytes(hurt), hurt, n, directory, 0, g, covered, G, values, S=S)
        assert statuses == wanted and paired == len(need_q), name
        for k, (v, s) in enumerate(zip(values, wanted)):                                        # and the bytes are the original ones
            if s == 0:
                pos, m, at = int(directory[v]["pos"]), int(directory[v]["stored"]), int(locs[k]["pos"])
                assert (out[at:at + m] == host[pos:pos + m]).all(), (name, k)


@pytest.mark.parametrize("G", GROUPS)
def test_rebuild_cases(cw, store, G):
    assert G2.rebuild_cases(G)["one shared column"][3] == [0, 0, 0]
    run_cases(cw, store, G)


def test_rebuild_cases_with_255_members(cw, store255):
    assert "members 253 and 254" in G2.rebuild_cases(255, BYTES_255)
    run_cases(cw, store255, 255)


@pytest.mark.parametrize("G", GROUPS)
def test_rebuild_counts_and_cursor(cw, store, G):
    entries, values, covered, _ = GM.rebuild_cases(G)["unprotected"]
    directory, g = np.array(entries, RM.LOC), Guards(store.guards(covered, G), covered)
    p, q = g.host()
    # the count on the device, clamped by max_count; positions at or past n are not written
    for count, max_count in ((len(values) + 5, len(values)), (3, len(values)), (0, len(values)), (len(values), 2), (len(values), 0)):
        n = min(count, max_count)
        want, wst, wout, wlocs = G2.rebuild(store.host, BYTES, directory, 0, covered, S, G, p, q, values[:n], BYTES)
        result, st, out, locs = rebuild(cw, store.dev, BYTES, directory, 0, g, G, values, want[1], count=count, max_count=max_count)
        assert result == want and st[:n].tolist() == wst.tolist() and (st[n:] == 0xEEEEEEEE).all(), (count, max_count)
        assert (out == wout).all() and (locs[:n] == wlocs).all() and (locs[n:].view(np.uint64) == POISON64).all()
    # a directory base, and values below it
    compare(cw, store.dev, store.host, BYTES, directory, DIR_BASE, g, covered, G, [DIR_BASE + 2, 2, DIR_BASE - 1, DIR_BASE + 3, DIR_BASE])
    # an inconsistent cursor protects nothing: verdict 2, nothing but status and result
    bad = Guards(store.guards(covered, G), BYTES + 1)
    result, st, out, locs = rebuild(cw, store.dev, BYTES, directory, 0, bad, G, values, 4096)
    assert result == [2, 0, len(values), 0, 0] and (st == 2).all() and (out == 0xEE).all() and (locs.view(np.uint64) == POISON64).all()


@pytest.mark.parametrize("G", GROUPS)
def test_rebuild_many_positions(cw, store, G):
    """Several hundred listed extents over more than one workgroup, duplicates, pairs and triples among them: every status and byte."""
    host = store.host
    rng = np.random.default_rng(200 + G)
    entries, at = [], 0
    while at < BYTES - 70000:
        n = int(rng.integers(1, 800)) if len(entries) != 7 else 65536
        entries.append(GM.entry(at, n))
        at += n + int(rng.integers(0, 1200))
    directory = np.array(entries, RM.LOC)
    assert len(directory) > 150
    for picks, covered in ((600, 4 * S + 777), (60, BYTES), (25, BYTES)):
        values = rng.integers(0, len(directory), picks).tolist()
        hurt = host.copy()
        for v in set(values):
            e = GM.extent_of(directory, 0, v, BYTES, covered)
            if e:
                hurt[e[0]:e[0] + e[1]] ^= 0x3C
        statuses, paired, out, locs = compare(cw, _dev_bytes(hurt), hurt, BYTES, directory, 0, Guards(store.guards(covered, G), covered), covered,
                                              G, values)
        if picks == 600:
            assert set(statuses) >= ({0, 2} if G == 2 else {1, 2})
        else:
            assert 0 in statuses and (picks != 60 or paired > 0)
        for k, (v, s) in enumerate(zip(values, statuses)):
            if s == 0:
                pos, m, to = int(directory[v]["pos"]), int(directory[v]["stored"]), int(locs[k]["pos"])
                assert (out[to:to + m] == host[pos:pos + m]).all(), (picks, k)


# ---- 4. whole stores ------------------------------------------------------------------------------------------------------------------
def assert_guarded(cs):
    """protected_bytes() == used(), and both guards are the model's over the stored bytes."""
    used = cs.used()
    assert cs.protected_bytes() == used
    p, q = G2.guards_of(cs.d_store.cpu().numpy(), used, cs.stripe, cs.group, max(cs.store_bytes, 1))
    assert (cs.d_guard.cpu().numpy() == p).all() and (cs.d_guard_q.cpu().numpy() == q).all()
    assert cs.guard_check() == (0, []) and cs.guard_check(detail=True) == (0, [], [])


def meeting_pairs(d, used, G, want):
    """`want` pairs (a, b) of directory indices: a in member 0 and b in member 1 of one group, b over the column of a's first byte; every
    extent inside its stripe, and the a's a few chunks apart."""
    W = G * S
    pos, stored = d["pos"].astype(np.int64), d["stored"].astype(np.int64)
    full = [i for i in range(len(d)) if stored[i] and pos[i] + stored[i] <= used and pos[i] // S == (pos[i] + stored[i] - 1) // S]
    pairs, taken = [], -1
    for a in full:
        if pos[a] // S % G != 0 or a <= taken + 3:
            continue
        b = next((i for i in full if pos[i] <= pos[a] + S < pos[i] + stored[i]), None)
        if b is not None and b not in [pair[1] for pair in pairs]:
            pairs.append((a, b))
            taken = a
        if len(pairs) == want:
            break
    return pairs


@pytest.mark.parametrize("alg", ALGS)
def test_pairs_of_damaged_chunks_repair_in_place(cw, alg):
    data, G = b"".join(corpus_file(name) for name in corpus_names()), 3                        # the in-tree corpus: 2.7 MiB
    assert len(data) > 2 << 20
    streams = [data[:1500000], data[1400000:]]
    index = cw.DedupeIndex("skein", 16384)
    try:
        cs = cw.ChunkStore(index, alg, cw.CdcParams(normal_size=1024), 3 << 20, 6000, DIR_BASE)
        with pytest.raises(ValueError):
            cs.protect(stripe=S, group=256, parity=2)
        with pytest.raises(ValueError):
            cs.protect(stripe=S, group=G, parity=3)
        cs.protect(stripe=S, group=G, parity=2)
        assert_guarded(cs)
        recs = []
        for s in streams:
            recs.append(cs.ingest(s))
            assert_guarded(cs)
        used, d = cs.used(), directory_of(cs)
        assert used > G * S
        pairs = meeting_pairs(d, used, G, 10)
        assert len(pairs) >= 8                                                                  # (the test cannot pass vacuously)
        victims = sorted(DIR_BASE + i for pair in pairs for i in pair)
        assert len(set(victims)) == 2 * len(pairs)
        before = cs.d_store.cpu().numpy().copy()
        # on the CPU: the single guard leaves every one of them collided, the dual guard rebuilds every one with its partner
        p, q = cs.d_guard.cpu().numpy(), cs.d_guard_q.cpu().numpy()
        assert (GM.rebuild(before, cs.store_bytes, d, DIR_BASE, used, S, G, p, victims, 1 << 22)[1] == 1).all()
        want = G2.rebuild(before, cs.store_bytes, d, DIR_BASE, used, S, G, p, q, victims, 1 << 22)
        assert (want[1] == 0).all() and want[0][3:] == [len(victims), len(victims)]
        # b's damaged byte lies in the column of a's first byte, a's own in its middle
        where = {DIR_BASE + b: int(d[a]["pos"]) + S for a, b in pairs}
        groups = sorted({at // (G * S) for at in flip(cs, d, victims, where=where)})
        report = cs.scrub()
        assert report.damaged.tolist() == victims
        assert cs.guard_check(detail=True) == (len(groups), groups, [3] * len(groups))        # a stored byte changed: both syndromes differ
        count = index.count()
        assert cs.repair_local(report) == dict(repaired=victims, collided=[], unprotected=[], failed=[], no_digest=[])
        assert cs.last_repair == dict(paired=len(victims))
        # in place: nothing moved, nothing grew, the index was not written; the bytes are the original ones
        assert cs.used() == used and cs.protected_bytes() == used and (directory_of(cs) == d).all() and index.count() == count
        assert (cs.d_store.cpu().numpy() == before).all()
        assert cs.scrub().clean
        assert_guarded(cs)
        for r, s in zip(recs, streams):
            assert cs.restore(r, verify=True) == s
        # one chunk alone needs no Q
        flip(cs, d, victims[:1])
        assert cs.repair_local(cs.scrub())["repaired"] == victims[:1] and cs.last_repair == dict(paired=0)
        # the same damage under the single guard: the pairs stay collided, as they always did
        cs.protect(stripe=S, group=G)
        assert cs.d_guard_q is None and cs.guard_check() == (0, [])
        flip(cs, d, victims, where=where)
        report = cs.scrub()
        assert report.damaged.tolist() == victims
        assert cs.repair_local(report) == dict(repaired=[], collided=victims, unprotected=[], failed=[], no_digest=[])
        assert cs.last_repair == dict(paired=0)
    finally:
        index.close()


@pytest.mark.parametrize("alg", ALGS)
def test_every_appending_method_keeps_both_guards(cw, alg):
    data = text()
    ia, ib = cw.DedupeIndex("skein", 4096), cw.DedupeIndex("skein", 4096)
    try:
        p = cw.CdcParams(normal_size=1024)
        A, B = cw.ChunkStore(ia, alg, p, 1 << 20, 1500, DIR_BASE), cw.ChunkStore(ib, alg, p, 1 << 20, 1500, 5)
        A.protect(group=3, parity=2)
        B.protect(stripe=1 << 17, group=2, parity=2)
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
        used, d = A.used(), directory_of(A)
        victim = int(r0.refs[7])
        at, = flip(A, d, [victim])
        report = A.scrub()
        assert report.damaged.tolist() == [victim]
        assert A.repair_from(B, report)["repaired"] == [victim]                                # appends the peer's copy
        assert A.used() > used and A.protected_bytes() == A.used()
        assert A.guard_check(detail=True) == (1, [at // (3 * S)], [3])                          # the old bytes stay, damaged, until a compact
        flip(A, d, [victim])
        assert_guarded(A)
        # compact: fresh guards over the new store; renumber: the guards stay as they are
        A.compact(recs[:4])
        assert A.d_guard_q is not None
        assert_guarded(A)
        guards = A.d_guard.cpu().numpy().copy(), A.d_guard_q.cpu().numpy().copy()
        kept = A.renumber(recs[:4])
        assert (A.d_guard.cpu().numpy() == guards[0]).all() and (A.d_guard_q.cpu().numpy() == guards[1]).all()
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
        cs.protect(stripe=S, group=3)                                                           # an old snapshot: parity 1, no guard_q
        old = str(tmp_path / "single.npz")
        cs.save(old)
        with np.load(old) as z:
            assert sorted(k for k in z.files if "guard" in k) == ["guard", "guard_covered", "guard_geometry"]
        loaded.append(cw.ChunkStore.load(old))
        assert loaded[-1].d_guard is not None and loaded[-1].d_guard_q is None and loaded[-1].guard_check() == (0, [])
        cs.protect(stripe=S, group=3, parity=2)
        path = str(tmp_path / "dual.npz")
        cs.save(path)
        with np.load(path) as z:
            assert sorted(k for k in z.files if "guard" in k) == ["guard", "guard_covered", "guard_geometry", "guard_q"]
            assert len(z["guard_q"]) == len(z["guard"]) == -(-cs.used() // (3 * S)) * S
        back = cw.ChunkStore.load(path)
        loaded.append(back)
        assert (back.stripe, back.group) == (S, 3)
        assert_guarded(back)
        assert (back.d_guard_q.cpu().numpy() == cs.d_guard_q.cpu().numpy()).all()
        d = directory_of(back)
        (a, b), = meeting_pairs(d, back.used(), 3, 1)
        victims = sorted([DIR_BASE + a, DIR_BASE + b])
        flip(back, d, victims, where={DIR_BASE + b: int(d[a]["pos"]) + S})
        report = back.scrub()
        assert report.damaged.tolist() == victims
        assert back.repair_local(report) == dict(repaired=victims, collided=[], unprotected=[], failed=[], no_digest=[])
        assert back.last_repair == dict(paired=2)
        assert back.scrub().clean and back.restore(rec, verify=True) == data[:300000]
        more = back.ingest(data[300000:400000])                                                 # and it goes on folding both
        assert_guarded(back)
        assert back.restore(more) == data[300000:400000]
    finally:
        index.close()
        for cs in loaded:
            cs.index.close()
