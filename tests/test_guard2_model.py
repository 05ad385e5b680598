"""The dual guard's brute-force model against itself and against guard_model.py (CPU): the field, P, the rebuild of an undamaged and of
a damaged store, and that every named case reaches the edge it names."""
import numpy as np
import pytest

import guard2_model as G2
import guard_model as GM
import restore_model as RM

S = G2.S
GROUPS = [2, 3]


def _store(n, seed=29):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)


@pytest.fixture(scope="module")
def small():
    return _store(G2.STORE_BYTES)


@pytest.fixture(scope="module")
def big():
    return _store(G2.STORE_BYTES_255, 255)


def test_the_field():
    assert G2.double(int(G2.POW[254])) == 1                                                   # 2^255 == 1
    assert len(set(G2.POW.tolist())) == 255 and 0 not in G2.POW                                 # 2^0 .. 2^254 are distinct
    assert G2.POW[:9].tolist() == [1, 2, 4, 8, 16, 32, 64, 128, 0x1D]
    a = np.arange(1, 256)
    assert (G2.MUL[a, G2.INV[a]] == 1).all() and (G2.MUL == G2.MUL.T).all() and (G2.MUL[1] == np.arange(256)).all()
    rng = np.random.default_rng(1)
    x, y, z = (rng.integers(0, 256, 500) for _ in range(3))
    assert (G2.MUL[x, y ^ z] == G2.MUL[x, y] ^ G2.MUL[x, z]).all() and (G2.MUL[G2.MUL[x, y], z] == G2.MUL[x, G2.MUL[y, z]]).all()
    # the packed doubling the kernels use, byte for byte
    w = rng.integers(0, 1 << 32, 1000, dtype=np.uint64)
    packed = (((w & 0x7f7f7f7f) << np.uint64(1)) ^ (((w >> np.uint64(7)) & 0x01010101) * np.uint64(0x1d))) & 0xFFFFFFFF
    for i in range(4):
        assert ((packed >> np.uint64(8 * i)) & 0xFF).tolist() == [G2.double(int(b)) for b in (w >> np.uint64(8 * i)) & 0xFF]
    assert G2.geometry_ok(S, 255) and not G2.geometry_ok(S, 256) and GM.geometry_ok(S, 256)


@pytest.mark.parametrize("G", GROUPS)
def test_p_is_the_xor_guard_and_updates_add_up(small, G):
    for covered in (0, 1, S + 5, 4 * S + 1000, G2.STORE_BYTES):
        p, q = G2.guards_of(small, covered, S, G, G2.STORE_BYTES)
        assert (p == GM.guard_of(small, covered, S, G, G2.STORE_BYTES)).all() and len(q) == len(p) == GM.guard_bytes(G2.STORE_BYTES, S, G)
    p, q = G2.guards_of(small, 0, S, G, G2.STORE_BYTES)
    cursor = 0
    for name, (a, b) in sorted(GM.update_ranges(G).items(), key=lambda kv: kv[1][1]):
        if b < cursor:
            continue
        result, cursor = G2.update(p, q, small, G2.STORE_BYTES, b, cursor, S, G)
        assert result[0] == 0 and cursor == b
    want = G2.guards_of(small, cursor, S, G, G2.STORE_BYTES)
    assert (p == want[0]).all() and (q == want[1]).all()
    assert G2.update(p, q, small, G2.STORE_BYTES, cursor - 1, cursor, S, G) == ([1, cursor, cursor - 1, 0], cursor)
    # check: a store byte sets both bits, a guard byte its own
    assert G2.check(p, q, small, G2.STORE_BYTES, cursor, S, G)[0] == [0, -(-cursor // (G * S)), 0, GM.NONE]
    hurt = small.copy()
    hurt[G * S + 3] ^= 1
    assert G2.check(p, q, hurt, G2.STORE_BYTES, cursor, S, G)[1].tolist()[:2] == [0, 3]
    p[5] ^= 1
    q[S + 5] ^= 1
    assert G2.check(p, q, small, G2.STORE_BYTES, cursor, S, G)[1].tolist()[:2] == [1, 2]


def _run_cases(store, G, store_bytes, S=S, single=None):
    """Every case against both models, undamaged and with every protected listed extent damaged."""
    reached, guards = set(), {}
    for name, (entries, values, covered, wanted, need_q) in G2.rebuild_cases(G, store_bytes, S, single).items():
        directory = np.array(entries, RM.LOC)
        if covered not in guards:
            guards[covered] = G2.guards_of(store, covered, S, G, store_bytes)
        p, q = guards[covered]
        result, status, payload, locs = G2.rebuild(store, store_bytes, directory, 0, covered, S, G, p, q, values, store_bytes)
        assert status.tolist() == wanted, name
        assert result[0] == 0 and result[3] == wanted.count(0), name
        # the P-only model: collided for every position the case says needs Q, and the same verdict on everything unprotected
        single = GM.rebuild(store, store_bytes, directory, 0, covered, S, G, p, values, store_bytes)[1].tolist()
        for k, s in enumerate(wanted):
            assert single[k] == (1 if k in need_q or s == 1 else s), (name, k)
        assert result[4] == len(need_q), name
        hurt = store.copy()
        for v in values:
            e = GM.extent_of(directory, 0, v, store_bytes, covered)
            if e:
                hurt[e[0]:e[0] + e[1]] ^= 0xA5
        for source in (store, hurt):
            _, _, payload, locs = G2.rebuild(source, store_bytes, directory, 0, covered, S, G, p, q, values, store_bytes)
            for k, (v, s) in enumerate(zip(values, wanted)):
                if s == 0:
                    pos, n, at = int(directory[v]["pos"]), int(directory[v]["stored"]), int(locs[k]["pos"])
                    assert (payload[at:at + n] == store[pos:pos + n]).all(), (name, k)
        if need_q:
            reached.add("Q")
        reached |= set(wanted)
    return reached


@pytest.mark.parametrize("G", GROUPS)
def test_rebuild_cases_reach_their_edges(small, G):
    assert _run_cases(small, G, G2.STORE_BYTES) == ({0, 2, "Q"} if G == 2 else {0, 1, 2, "Q"})
    c = G2.rebuild_cases(G)
    W = G * S
    e = c["a boundary inside a word"][0]
    assert (e[0][0] + e[0][1]) % 4 == 2 and e[1][0] % S % 4 == 1 and e[1][0] % S == (e[0][0] + e[0][1]) - 1
    e = c["a pair across a group boundary"][0]
    assert e[0][0] // S % G == G - 1 and e[0][0] // W == 0 and (e[0][0] + e[0][1] - 1) // W == 1 and e[1][0] // W == 1 and e[1][0] // S % G == 1
    e, _, covered, _, _ = c["a partner that ends at covered"]
    assert e[1][0] + e[1][1] == covered
    e = c["members 0 and G - 1"][0]
    assert e[0][0] // S % G == 0 and e[1][0] // S % G == G - 1
    assert (G == 2) == ("G = 2: three extents, two members" in c) and (G > 2) == ("three members over one column" in c)


def test_rebuild_cases_of_255_members(big):
    assert _run_cases(big, 255, G2.STORE_BYTES_255) == {0, 1, 2, "Q"}
    e = G2.rebuild_cases(255, G2.STORE_BYTES_255)["members 253 and 254"][0]
    assert e[0][0] // S == 253 and e[1][0] // S == 254
    a, b = G2.update_range_255()
    assert a // S % 255 == 254 and a // (255 * S) == 0 and b // (255 * S) == 1 and (b - 1) // S % 255 == 0 and b <= G2.STORE_BYTES_255


@pytest.mark.parametrize("S_, G, stripes", [(S, 1, 6), (S, 16, 33), (1 << 17, 2, 6)])
def test_rebuild_cases_at_other_geometries(S_, G, stripes):
    """guard_model's cases and the dual guard's over one member, over ChunkStore.protect()'s default group, and over a larger stripe."""
    n = stripes * S_ + 37
    assert _run_cases(_store(n, G), G, n, S_, single=True) == ({0, 2} if G == 1 else {0, 2, "Q"} if G == 2 else {0, 1, 2, "Q"})
    cases = G2.rebuild_cases(G, n, S_, True)
    assert set(GM.rebuild_cases(G, S_, n)) <= set(cases) and ("one shared column" in cases) == (G > 1)
    e = cases["across a group boundary"][0][0]
    assert e[0] // (G * S_) == 0 and (e[0] + e[1] - 1) // (G * S_) == 1 and cases["across a group boundary"][3] == [0]
    if S_ > S:
        assert cases["S bytes from mid-stripe"][0][0][1] == 65536 and cases["65536 bytes from the last column"][0][0][0] % S_ == S_ - 1
    ranges = GM.update_ranges(G, S_, n)
    assert ranges["everything"] == (0, n) and ranges["more than W bytes"][1] - ranges["more than W bytes"][0] > G * S_
