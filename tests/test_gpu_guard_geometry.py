"""The guard kernels at the geometries the other two files leave out (tests/test_gpu_guard.py, tests/test_gpu_guard2.py; DESIGN.md
sections 28 and 29), everything compared exactly with guard_model.py and guard2_model.py through those files' helpers: G = 1, G = 16
(``ChunkStore.protect()``'s default), G = 256 (the single guard's maximum: a member of 8 bits beside a length of 24) and a stripe of
2^17 bytes (``shift != 16`` in update, check and rebuild); launches that stride (more guard words than 2048 x 256 lanes, more groups
than the 256 threads that count the flags, more listed positions than 8192 workgroups); many small updates at G = 1 and G = 16."""
import numpy as np
import pytest

import guard2_model as G2
import guard_model as GM
import restore_model as RM
import test_gpu_guard as T1
import test_gpu_guard2 as T2
from test_gpu_guard import Guard, _dev_bytes, _dev_u64, _stream, _sync, _u64
from test_gpu_guard2 import Guards

pytestmark = pytest.mark.gpu

S16, S17 = GM.S, 1 << 17
# name: (S, G, the store's bytes, whether the dual guard takes G)
GEOMETRY = {"G=1": (S16, 1, GM.STORE_BYTES, True),
            "G=16": (S16, 16, 33 * S16 + 37, True),                       # two groups and a few bytes
            "G=256": (S16, 256, G2.STORE_BYTES_255 + S16, False),          # one group, one stripe of the next and a few bytes
            "S=2^17": (S17, 2, 6 * S17 + 37, True)}
LANES, FLAG_THREADS, WAVE_GROUPS = 2048 * 256, 256, 8192                   # lane_grid's cap, the check's one workgroup, wave_grid's cap


@pytest.fixture(scope="module")
def cw():
    import torch  # noqa: F401  (one HIP runtime for torch and libcwhc.so)
    import compute_war_amd as cw
    cw.init(0)
    yield cw
    cw.tune_reset()


class Noise(T2.Stored):
    """``Stored`` for stores of many megabytes: the model's (P, Q) of a cursor are the ones of the nearest cursor below it that is
    cached, folded on by the model's own update -- so a walk over many cursors folds every byte a few times, not once per cursor.
    ``dual`` = False leaves Q alone (it stays zero)."""

    def __init__(self, n, seed, S, dual=True):
        super().__init__(n, seed, S)
        self.dual = dual

    def guards(self, covered, G):
        if (covered, G) not in self.cache:
            below = max((c for c, g in self.cache if g == G and c <= covered), default=None)
            size = GM.guard_bytes(self.n, self.S, G)
            p, q = (a.copy() for a in self.cache[below, G]) if below is not None else (np.zeros(size, np.uint8), np.zeros(size, np.uint8))
            if self.dual:
                assert G2.update(p, q, self.host, self.n, covered, below or 0, self.S, G)[0][0] == 0
            else:
                assert GM.update(p, self.host, self.n, covered, below or 0, self.S, G)[0][0] == 0
            self.cache[covered, G] = p, q
        return self.cache[covered, G]


_NOISE = {}


def noise_of(name, S, G, n, dual=True):
    """the noise of a geometry and its guards, made once"""
    if name not in _NOISE:
        _NOISE[name] = Noise(n, 300 + G, S, dual)
    return _NOISE[name]


@pytest.fixture(params=list(GEOMETRY))
def geo(request, cw):
    S, G, n, dual = GEOMETRY[request.param]
    return S, G, n, dual, noise_of(request.param, S, G, n, dual)


@pytest.fixture(scope="module")
def big(cw):
    """16.8 MB: at G = 1, 257 groups and 1,052,672 guard words"""
    return Noise(G2.STORE_BYTES_255, 255, S16)


def parities(dual):
    return (1, 2) if dual else (1,)


def guard_of(noise, covered, G, parity):
    pq = noise.guards(covered, G)
    return Guard(pq[0], covered) if parity == 1 else Guards(pq, covered)


def same(g, pq, parity):
    return (g.host() == pq[0]).all() if parity == 1 else g.equal(pq)


def update(cw, noise, g, used, G, parity):
    fn = T1.update if parity == 1 else T2.update
    return fn(cw, noise.dev, g, used, G, store_bytes=noise.n, S=noise.S)


def check(cw, d_store, noise, g, G, parity, flags=True):
    fn = T1.check if parity == 1 else T2.check
    return fn(cw, d_store, g, G, flags=flags, store_bytes=noise.n, S=noise.S)


def model_check(pq, host, noise, covered, G, parity):
    if parity == 1:
        return GM.check(pq[0], host, noise.n, covered, noise.S, G)
    return G2.check(pq[0], pq[1], host, noise.n, covered, noise.S, G)


# ---- 1. the geometries ------------------------------------------------------------------------------------------------------------------
def test_the_geometries_are_the_ones_named():
    for name, (S, G, n, dual) in GEOMETRY.items():
        assert GM.geometry_ok(S, G) and dual == G2.geometry_ok(S, G), name
    assert GEOMETRY["G=16"][2] // (16 * S16) == 2 and GEOMETRY["G=256"][2] // (256 * S16) == 1
    assert GM.guard_bytes(G2.STORE_BYTES_255, S16, 1) // 16 == 1052672 > LANES and -(-G2.STORE_BYTES_255 // S16) == 257 > FLAG_THREADS
    cases = GM.rebuild_cases(2, S17, GEOMETRY["S=2^17"][2])
    (pos, n, _), = cases["65536 bytes from the last column"][0]
    assert (pos % S17, n) == (S17 - 1, 65536)
    cases = GM.rebuild_cases(256, S16, GEOMETRY["G=256"][2])
    (a, na, _), (b, nb, _) = cases["members 254 and 255"][0]
    assert (a // S16, b // S16) == (254, 255)
    (a, na, _), _ = cases["from member 255 into the next group"][0]
    assert a // S16 == 255 and (a + na - 1) // S16 == 256
    assert cases["across a group boundary"][3] == [0] and GM.rebuild_cases(16, S16, GEOMETRY["G=16"][2])["across a group boundary"][3] == [0]


def test_with_one_member_the_guard_is_the_store(cw):
    """G = 1: P is the covered store bytes and Q == P -- of the model, as a check of the case and not as the reference."""
    S, G, n, _ = GEOMETRY["G=1"]
    host = np.random.default_rng(1).integers(0, 256, n, dtype=np.uint8)
    for covered in (0, 5, 2 * S + 9, n):
        p, q = G2.guards_of(host, covered, S, G, n)
        assert (p[:covered] == host[:covered]).all() and not p[covered:].any() and (q == p).all() and len(p) == -(-n // S) * S


def test_update_ranges(cw, geo):
    S, G, n, dual, noise = geo
    for parity in parities(dual):
        for name, (a, b) in GM.update_ranges(G, S, n).items():
            g = guard_of(noise, a, G, parity)
            assert update(cw, noise, g, b, G, parity) == [0, a, b, b - a], (name, parity)
            assert g.covered() == b and same(g, noise.guards(b, G), parity), (name, parity)
            assert update(cw, noise, g, b, G, parity) == [0, b, b, 0], (name, parity)         # twice: nothing the second time
            assert g.covered() == b and same(g, noise.guards(b, G), parity), (name, parity)


def test_check(cw, geo):
    S, G, n, dual, noise = geo
    W, covered = G * S, n - 1000                                           # (the last group is partial)
    groups = -(-covered // W)
    flips = [0, W - 1, W, covered - 1] if n < 4 << 20 else [W - 1, covered - 1]
    for parity in parities(dual):
        good = noise.guards(covered, G)
        g = guard_of(noise, covered, G, parity)

        def expect(d, g, host, pq):
            want, bits = model_check(pq, host, noise, covered, G, parity)
            result, bad = check(cw, d, noise, g, G, parity)
            assert result == want and bad[1:1 + groups].tolist() == bits.tolist(), parity
            assert bad[0] == 0xEEEEEEEE and (bad[1 + groups:] == 0xEEEEEEEE).all()             # no flag outside the groups checked
            assert check(cw, d, noise, g, G, parity, flags=False)[0] == want
            return result
        assert expect(noise.dev, g, noise.host, good) == [0, groups, 0, GM.NONE]
        for at in flips:                                                    # one flipped store byte
            hurt = noise.host.copy()
            hurt[at] ^= 0x10
            assert expect(_dev_bytes(hurt), g, hurt, good) == [0, groups, 1, at // W], (at, parity)
        for which in range(parity):                                         # one flipped guard byte, in the last column of the last group
            hurt = [good[0].copy(), good[1].copy()]
            hurt[which][groups * S - 1] ^= 0x01
            assert expect(noise.dev, guard_of_pair(hurt, covered, parity), noise.host, hurt) == [0, groups, 1, groups - 1], (which, parity)


def guard_of_pair(pq, covered, parity):
    return Guard(pq[0], covered) if parity == 1 else Guards(pq, covered)


def test_rebuild_cases(cw, geo):
    S, G, n, dual, noise = geo
    cases = GM.rebuild_cases(G, S, n)
    assert ("one shared column" in cases) == (G > 1) and ("65536 bytes from the last column" in cases) == (S > 65536)
    for name, (entries, values, covered, wanted) in cases.items():
        directory = np.array(entries, RM.LOC)
        hurt = noise.host.copy()
        for v in values:
            e = GM.extent_of(directory, 0, v, n, covered)
            if e:
                hurt[e[0]:e[0] + e[1]] ^= 0xA5
        g = Guard(noise.guards(covered, G)[0], covered)
        d_hurt = _dev_bytes(hurt)
        assert T1.compare(cw, d_hurt, hurt, directory, 0, g, covered, G, values, store_bytes=n, S=S) == wanted, name
        total = sum(int(directory[v]["stored"]) for v, s in zip(values, wanted) if s == 0)   # and the bytes are the original ones
        _, _, out, locs = T1.rebuild(cw, d_hurt, directory, 0, g, G, values, total, store_bytes=n, S=S)
        for k, (v, s) in enumerate(zip(values, wanted)):
            if s == 0:
                pos, m, at = int(directory[v]["pos"]), int(directory[v]["stored"]), int(locs[k]["pos"])
                assert (out[at:at + m] == noise.host[pos:pos + m]).all(), (name, k)
    if dual:
        assert set(G2.rebuild_cases(G, n, S, True)) > set(cases) or G == 1
        T2.run_cases(cw, noise, G, single=True)


@pytest.mark.parametrize("name", ["G=1", "G=16"])
def test_many_small_updates_equal_one_large(cw, name):
    """Queued one behind the other with no synchronise between them, each behind the write of the cursor it reads."""
    S, G, n, dual = GEOMETRY[name]
    noise = noise_of(name, S, G, n, dual)
    cuts = sorted(set(np.random.default_rng(G).integers(0, n, 40).tolist()) | {S, G * S, n})
    for parity in (1, 2):
        g = guard_of(noise, 0, G, parity)
        d_used, results = _dev_u64(cuts), _dev_u64(np.zeros(4 * len(cuts)))
        _sync()
        for k in range(len(cuts)):
            if parity == 1:
                cw.dev_store_guard_update(noise.dev.data_ptr(), n, d_used.data_ptr() + 8 * k, g.d_covered.data_ptr(), S, G, g.ptr(), g.size,
                                          results.data_ptr() + 32 * k, _stream())
            else:
                cw.dev_store_guard2_update(noise.dev.data_ptr(), n, d_used.data_ptr() + 8 * k, g.d_covered.data_ptr(), S, G, g.p.ptr(), g.q.ptr(),
                                           g.size, results.data_ptr() + 32 * k, _stream())
        _sync()
        assert _u64(results).reshape(-1, 4).tolist() == [[0, a, b, b - a] for a, b in zip([0] + cuts[:-1], cuts)]
        assert g.covered() == n and same(g, noise.guards(n, G), parity)


# ---- 2. launches that stride -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("parity", [1, 2])
def test_update_strides_over_more_words_than_lanes(cw, big, parity):
    """G = 1 over 16.8 MB: 1,052,672 guard words for 524,288 lanes, from 0 and from a cursor in the middle of the store."""
    n, G, mid = big.n, 1, 100 * S16 + 4099
    for a, b in ((0, n), (mid, n), (0, mid)):
        g = guard_of(big, a, G, parity)
        assert update(cw, big, g, b, G, parity) == [0, a, b, b - a]
        assert g.covered() == b and same(g, big.guards(b, G), parity), (a, b)
    assert (big.guards(n, G)[0][:n] == big.host).all()                       # (G = 1: P is the store)


FLIPS = {"clean": [], "group 0": [7], "group 255": [255 * S16 + 5], "the last, partial group": [256 * S16 + 3],
         "groups 0 and 256, one thread's": [S16 - 1, 256 * S16 + 36], "groups 255 and 256": [256 * S16 - 1, 256 * S16]}


@pytest.mark.parametrize("parity", [1, 2])
@pytest.mark.parametrize("flips", list(FLIPS))
def test_check_strides_over_more_groups_than_threads(cw, big, parity, flips):
    """257 groups for the 256 threads that count the flags: the lowest bad group, and a flag per group."""
    n, G = big.n, 1
    good, at = big.guards(n, G), FLIPS[flips]
    hurt = big.host.copy()
    if at:
        hurt[at] ^= 0x40
    want, bits = model_check(good, hurt, big, n, G, parity)
    groups = sorted({p // S16 for p in at})
    assert want == [0, 257, len(groups), groups[0] if groups else GM.NONE] and np.nonzero(bits)[0].tolist() == groups   # (what the case is for)
    result, bad = check(cw, _dev_bytes(hurt) if at else big.dev, big, guard_of(big, n, G, parity), G, parity)
    assert result == want and bad[1:258].tolist() == bits.tolist()
    assert bad[0] == 0xEEEEEEEE and bad[258] == 0xEEEEEEEE


@pytest.mark.parametrize("parity", [1, 2])
def test_rebuild_of_more_positions_than_workgroups(cw, parity):
    """More than 8192 listed positions over a few hundred extents, duplicates, pairs and triples among them: every status, byte and loc."""
    S, G, n = S16, 3, GM.STORE_BYTES
    noise = noise_of("many positions", S, G, n)
    rng = np.random.default_rng(400)
    entries, at = [], 0
    while at < n - 3000:
        m = int(rng.integers(1, 500))
        entries.append(GM.entry(at, m))
        at += m + int(rng.integers(0, 2500))
    directory = np.array(entries, RM.LOC)
    assert 200 < len(directory) < 400
    values = rng.integers(0, len(directory), WAVE_GROUPS + 900).tolist()      # every extent, each many times
    hurt = noise.host.copy()
    for v in set(values):
        hurt[entries[v][0]:entries[v][0] + entries[v][1]] ^= 0x3C
    d_hurt = _dev_bytes(hurt)
    if parity == 1:
        statuses = T1.compare(cw, d_hurt, hurt, directory, 0, Guard(noise.guards(n, G)[0], n), n, G, values, store_bytes=n, S=S)
        assert {0, 1} <= set(statuses)
    else:
        statuses, paired, out, locs = T2.compare(cw, d_hurt, hurt, n, directory, 0, Guards(noise.guards(n, G), n), n, G, values, S=S)
        assert 0 in statuses and paired > 0
        for k, (v, s) in enumerate(zip(values, statuses)):
            if s == 0:
                pos, m, to = entries[v][0], entries[v][1], int(locs[k]["pos"])
                assert (out[to:to + m] == noise.host[pos:pos + m]).all(), k


# ---- 3. both parities on the scratch they share ------------------------------------------------------------------------------------------
class Mixed:
    """Three whole groups of two stripes and 5000 bytes, both guards folded to the end, then four damaged extents: two that meet in
    guard bytes (members 0 and 1 of group 0, columns 2500 .. 4000) -- collided for the single guard, rebuilt with Q by the dual one --,
    one of 65536 bytes across a stripe boundary of group 1 and one of a single byte in the last, partial group.  Listed: the four,
    the first once more and a value that names no entry.  The model's answers for the single (1) and the dual (2) guard, each once."""
    S, G, n = S16, 2, 3 * 2 * S16 + 5000

    def __init__(self):
        S, G, n = self.S, self.G, self.n
        rng = np.random.default_rng(2830)
        self.host = rng.integers(0, 256, n, dtype=np.uint8)
        hurt_extents = [(1000, 3000), (S + 2500, 2000), (3 * S - 700, 65536), (6 * S + 4000, 1)]
        entries, taken = [GM.entry(at, m) for at, m in hurt_extents], sorted(hurt_extents)
        for lo, hi in zip([0] + [at + m for at, m in taken], [at for at, _ in taken] + [n]):   # other extents in the room between them
            at = lo + int(rng.integers(0, 3000))
            while len(entries) < 40:
                m = int(rng.integers(1, 9000))
                if at + m > hi:
                    break
                entries.append(GM.entry(at, m))
                at += m + int(rng.integers(0, 6000))
        assert 36 <= len(entries) <= 40 and n == 398216
        self.directory = np.array(entries, RM.LOC)
        self.values = [0, 1, 2, 3, 0, len(entries) + 3]
        self.hurt = self.host.copy()
        for at, m in hurt_extents:
            self.hurt[at:at + m] ^= 0x5A
        self.pq = G2.guards_of(self.host, n, S, G, n)
        self.groups = len(self.pq[0]) // S
        p, q = self.pq
        self.want = {("check", 1): GM.check(p, self.hurt, n, n, S, G), ("check", 2): G2.check(p, q, self.hurt, n, n, S, G),
                     ("rebuild", 1): GM.rebuild(self.hurt, n, self.directory, 0, n, S, G, p, self.values, 1 << 62),
                     ("rebuild", 2): G2.rebuild(self.hurt, n, self.directory, 0, n, S, G, p, q, self.values, 1 << 62)}
        # what the case is for: the two parities disagree on the first two extents
        assert self.want["rebuild", 1][1].tolist() == [1, 1, 0, 0, 1, 2] and self.want["rebuild", 1][0] == [0, 65537, 6, 2]
        assert self.want["rebuild", 2][1].tolist() == [0, 0, 0, 0, 0, 2] and self.want["rebuild", 2][0] == [0, 65537 + 3000 + 2000 + 3000, 6, 5, 3]
        assert self.want["check", 1][1].tolist() == [1, 1, 0, 1] and self.want["check", 2][1].tolist() == [3, 3, 0, 3]
        self.d_hurt, self.d_dir = _dev_bytes(self.hurt), _dev_bytes(self.directory)
        self.d_val, self.d_count = _dev_u64(self.values + [0]), _dev_u64([len(self.values)])
        self.g = Guards(self.pq, n)


@pytest.fixture(scope="module")
def mixed(cw):
    return Mixed()


class Call:
    """One check or rebuild of ``Mixed`` at one parity: poisoned outputs of its own, made before anything is queued; ``launch`` queues
    the call and synchronises nothing; ``outputs`` reads what it wrote."""

    def __init__(self, cw, c, op, parity):
        self.cw, self.c, self.op, self.parity = cw, c, op, parity
        words = 5 if (op, parity) == ("rebuild", 2) else 4                   # (only the dual rebuild reports a fifth word)
        self.result = _dev_u64([7] * words + [T2.POISON64])
        if op == "check":
            self.bad = _dev_bytes(np.full(c.groups + 2, 0xEEEEEEEE, np.uint32))
        else:
            self.m, self.total = len(c.values), c.want[op, parity][0][1]
            self.out = _dev_bytes(np.full(self.total + 2 * T1.PAD, 0xEE, np.uint8))
            self.loc = _dev_bytes(np.full(2 * (self.m + 2), T2.POISON64, np.uint64))
            self.status = _dev_bytes(np.full(self.m + 2, 0xEEEEEEEE, np.uint32))

    def launch(self, stream):
        c, g, cw = self.c, self.c.g, self.cw
        guards = (g.p.ptr(),) if self.parity == 1 else (g.p.ptr(), g.q.ptr())
        if self.op == "check":
            fn = cw.dev_store_guard_check if self.parity == 1 else cw.dev_store_guard2_check
            fn(c.d_hurt.data_ptr(), c.n, g.d_covered.data_ptr(), c.S, c.G, *guards, g.size, self.bad.data_ptr() + 4, self.result.data_ptr(), stream)
        else:
            fn = cw.dev_store_guard_rebuild if self.parity == 1 else cw.dev_store_guard2_rebuild
            fn(c.d_hurt.data_ptr(), c.n, c.d_dir.data_ptr(), 0, len(c.directory), g.d_covered.data_ptr(), c.S, c.G, *guards, g.size,
               c.d_val.data_ptr(), c.d_count.data_ptr(), self.m, self.out.data_ptr() + T1.PAD, self.total, self.loc.data_ptr() + 16,
               self.status.data_ptr() + 4, self.result.data_ptr(), stream)

    def outputs(self):
        r = _u64(self.result).tolist()
        assert r[-1] == T2.POISON64
        if self.op == "check":
            bad = self.bad.cpu().numpy().view(np.uint32)
            assert bad[0] == bad[-1] == 0xEEEEEEEE
            return r[:-1], bad[1:-1].tolist()
        h, locs, st = self.out.cpu().numpy(), self.loc.cpu().numpy().view(np.uint64), self.status.cpu().numpy().view(np.uint32)
        assert (h[:T1.PAD] == 0xEE).all() and (h[T1.PAD + self.total:] == 0xEE).all(), "a store left d_out"
        assert (locs[:2] == T2.POISON64).all() and (locs[-2:] == T2.POISON64).all() and st[0] == st[-1] == 0xEEEEEEEE
        return r[:-1], st[1:-1].tolist(), h[T1.PAD:T1.PAD + self.total].tobytes(), locs[2:-2].tobytes()

    def wanted(self):
        want = self.c.want[self.op, self.parity]
        if self.op == "check":
            return want[0], want[1].tolist()
        return want[0], want[1].tolist(), want[2].tobytes(), want[3].tobytes()


SEQUENCE = [("check", 1), ("check", 2), ("rebuild", 1), ("rebuild", 2), ("check", 1), ("check", 2)]


@pytest.mark.parametrize("streams", ["one stream", "a stream per parity"])
def test_both_parities_queued_on_the_scratch_they_share(cw, mixed, streams):
    """Single check, dual check, single rebuild, dual rebuild, single check, dual check, queued with nothing synchronised between them
    -- on one stream, where every call reuses the stream's one guard scratch behind the other parity's, and with the single calls
    on one stream and the dual calls on another: every result, flag, status, loc and payload byte is the model's, and equals what
    the same call writes alone on a fresh stream."""
    import torch
    queues = [torch.cuda.Stream() for _ in range(1 if streams == "one stream" else 2)]
    calls = [Call(cw, mixed, op, parity) for op, parity in SEQUENCE]
    alone = [Call(cw, mixed, op, parity) for op, parity in SEQUENCE]
    _sync()
    for call in calls:
        call.launch(queues[(call.parity - 1) % len(queues)].cuda_stream)
    _sync()
    for k, (call, lone) in enumerate(zip(calls, alone)):
        fresh = torch.cuda.Stream()
        lone.launch(fresh.cuda_stream)
        _sync()
        got = call.outputs()
        assert got == call.wanted(), (k, call.op, call.parity)
        assert got == lone.outputs(), (k, call.op, call.parity)
    mixed.g.host()                                                           # (the guards are only read)
