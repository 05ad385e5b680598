"""The numpy model of the guard stripes alone (guard_model.py): the guard it sums, its update ranges, its check and its rebuild with
statuses, over the named cases that the GPU tests run too.  Every case is shown to reach the edge it is named after, and for every
recoverable case flipping bytes inside the listed extents and rebuilding gives the original bytes back."""
import numpy as np
import pytest

import guard_model as GM
import restore_model as RM

S, BYTES = GM.S, GM.STORE_BYTES
GROUPS = [2, 3]


@pytest.fixture(scope="module")
def store():
    return np.random.default_rng(28).integers(0, 256, BYTES, dtype=np.uint8)


def test_guard_bytes_and_geometry():
    for G in (1, 2, 16, 256):
        W = G * S
        assert [GM.guard_bytes(n, S, G) for n in (0, 1, W - 1, W, W + 1)] == [0, S, S, S, 2 * S]
    assert GM.guard_bytes(BYTES, S, 2) == 4 * S and GM.guard_bytes(BYTES, S, 3) == 3 * S and GM.guard_bytes(BYTES, 1 << 30, 1) == 1 << 30
    for S_, G_ in ((32768, 2), (65536 + 16, 2), (3 * 65536, 2), (1 << 31, 2), (S, 0), (S, 257), (0, 1)):
        assert GM.guard_bytes(BYTES, S_, G_) == 0 and not GM.geometry_ok(S_, G_)


def test_the_guard_is_the_xor_of_its_cells(store):
    """The definition, spelled out once more in the slowest way for a few cells; and a stored extent never meets itself."""
    for G in GROUPS:
        W, covered = G * S, 5 * S + 99
        guard = GM.guard_of(store, covered, S, G, BYTES)
        assert len(guard) == GM.guard_bytes(BYTES, S, G)
        for g, c in ((0, 0), (0, S - 1), (1, 17), (5 * S // W, 98), (5 * S // W, 99), (len(guard) // S - 1, S - 1)):
            want = 0
            for p in range(covered):
                if p // W == g and p % S == c:
                    want ^= int(store[p])
            assert guard[g * S + c] == want, (G, g, c)
        for pos in (0, S - 1, W - 30000, 2 * W - 65535):
            cell = GM.cells(np.arange(pos, pos + 65536), S, G)
            assert len(np.unique(cell)) == 65536, (G, pos)


@pytest.mark.parametrize("G", GROUPS)
def test_update_ranges_reach_their_edges_and_fold_exactly_once(store, G):
    W, ranges = G * S, GM.update_ranges(G)
    for n in (1, 15, 16, 17):
        for at in (0, 1, 15):
            a, b = ranges[f"{n} bytes at {at} mod 16"]
            assert b - a == n and a % 16 == at
    a, b = ranges["inside one stripe"]
    assert a // S == (b - 1) // S
    a, b = ranges["across a stripe boundary"]
    assert a // S + 1 == (b - 1) // S and a // W == (b - 1) // W
    a, b = ranges["across a group boundary"]
    assert a // W + 1 == (b - 1) // W
    assert ranges["W bytes"][1] - ranges["W bytes"][0] == W and ranges["more than W bytes"][1] - ranges["more than W bytes"][0] > W
    assert ranges["nothing"][0] == ranges["nothing"][1] and ranges["everything"] == (0, BYTES)
    for name, (a, b) in ranges.items():
        guard = GM.guard_of(store, a, S, G, BYTES)
        before = guard.copy()
        result, covered = GM.update(guard, store, BYTES, b, a, S, G)
        assert result == [0, a, b, b - a] and covered == b, name
        assert (guard == GM.guard_of(store, b, S, G, BYTES)).all(), name
        assert (guard != before).sum() <= b - a and ((guard != before).any() or a == b or not store[a:b].any()), name
        again, covered = GM.update(guard, store, BYTES, b, covered, S, G)                      # twice: a no-op the second time
        assert again == [0, b, b, 0] and (guard == GM.guard_of(store, b, S, G, BYTES)).all(), name
    # an inconsistent cursor: verdict 1, nothing changes
    guard = GM.guard_of(store, 1000, S, G, BYTES)
    for used, covered in ((999, 1000), (BYTES + 1, 1000)):
        before = guard.copy()
        assert GM.update(guard, store, BYTES, used, covered, S, G) == ([1, covered, used, 0], covered) and (guard == before).all()
    # many small updates equal one large one
    guard, covered = np.zeros(GM.guard_bytes(BYTES, S, G), np.uint8), 0
    cuts = sorted(set(np.random.default_rng(G).integers(0, BYTES, 40).tolist()) | {S, W, BYTES})
    for used in cuts:
        _, covered = GM.update(guard, store, BYTES, used, covered, S, G)
    assert covered == BYTES and (guard == GM.guard_of(store, BYTES, S, G, BYTES)).all()


@pytest.mark.parametrize("G", GROUPS)
def test_check_sees_store_and_guard_but_not_above_the_cursor(store, G):
    W, covered = G * S, 4 * S + 1000
    guard, n = GM.guard_of(store, covered, S, G, BYTES), -(-covered // W)
    assert GM.check(guard, store, BYTES, covered, S, G)[0] == [0, n, 0, GM.NONE]
    for at in (0, W - 1, W, covered - 1):
        hurt = store.copy()
        hurt[at] ^= 0x10
        result, bad = GM.check(guard, hurt, BYTES, covered, S, G)
        assert result == [0, n, 1, at // W] and bad.tolist() == [int(g == at // W) for g in range(n)], at
    for at in (5, (n - 1) * S + S - 1):                                                         # the second: the last column of the last group checked
        hurt = guard.copy()
        hurt[at] ^= 0x01
        assert GM.check(hurt, store, BYTES, covered, S, G)[0] == [0, n, 1, at // S], at
    hurt = store.copy()
    hurt[covered] ^= 0xFF
    hurt[BYTES - 1] ^= 0xFF
    assert GM.check(guard, hurt, BYTES, covered, S, G)[0] == [0, n, 0, GM.NONE]
    assert GM.check(guard, store, BYTES, BYTES + 1, S, G)[0] == [1, 0, 0, GM.NONE]
    assert GM.check(np.zeros(len(guard), np.uint8), store, BYTES, 0, S, G)[0] == [0, 0, 0, GM.NONE]


def damaged(store, directory, values, covered):
    """The store with a few bytes flipped inside every listed extent that is protected."""
    hurt = store.copy()
    for v in values:
        e = GM.extent_of(directory, 0, v, BYTES, covered)
        if e:
            for at in {e[0], e[0] + e[1] // 2, e[0] + e[1] - 1}:
                hurt[at] = store[at] ^ 0xA5
    return hurt


@pytest.mark.parametrize("G", GROUPS)
def test_rebuild_cases_reach_their_edges_and_give_the_bytes_back(store, G):
    W, cases = G * S, GM.rebuild_cases(G)
    assert len(cases) == 10
    ext = lambda name, k=0: tuple(int(v) for v in cases[name][0][k][:2])  # noqa: E731
    assert ext("one byte")[1] == 1
    pos, n = ext("S bytes from mid-stripe")
    assert n == S and 0 < pos % S < S and (pos + n - 1) // S == pos // S + 1
    pos, n = ext("across a stripe boundary")
    assert pos // S + 1 == (pos + n - 1) // S and pos // W == (pos + n - 1) // W
    pos, n = ext("across a group boundary")
    assert pos // W + 1 == (pos + n - 1) // W
    (a, na), (b, nb) = ext("adjacent columns", 0), ext("adjacent columns", 1)
    assert a // W == b // W and a // S != b // S and a % S + na == b % S
    (a, na), (b, nb), (c, nc) = (ext("one shared column", k) for k in range(3))
    assert a // W == b // W and a // S != b // S and a % S + na - 1 == b % S and c // W != a // W
    assert cases["a value twice"][1] == [0, 0]
    pos, n = ext("ends at covered")
    assert pos + n == cases["ends at covered"][2]
    pos, n = ext("ends above covered")
    assert pos + n == cases["ends above covered"][2] + 1
    d = np.array(cases["unprotected"][0], RM.LOC)
    assert not any(d[0]) and any(d[1]) and not GM.sound(d[1], BYTES) and GM.sound(d[2], BYTES) and cases["unprotected"][1][2] >= len(d)

    for name, (entries, values, covered, wanted) in cases.items():
        directory = np.array(entries, RM.LOC)
        guard = GM.guard_of(store, covered, S, G, BYTES)
        hurt = damaged(store, directory, values, covered)
        assert (hurt != store).any() or not any(s == 0 for s in wanted), name
        result, status, out, locs = GM.rebuild(hurt, BYTES, directory, 0, covered, S, G, guard, values, BYTES)
        assert status.tolist() == wanted, name
        total = sum(int(directory[v]["stored"]) for v, s in zip(values, wanted) if s == 0)
        assert result == [0, total, len(values), wanted.count(0)] and len(out) == total, name
        at = 0
        for k, (v, s) in enumerate(zip(values, wanted)):
            if s == 0:
                pos, n, word = (int(x) for x in directory[v])
                assert tuple(int(x) for x in locs[k]) == (at, n, word), (name, k)
                assert (out[at:at + n] == store[pos:pos + n]).all(), (name, k)                   # the ORIGINAL bytes
                at += n
            else:
                assert not any(locs[k]), (name, k)
        # the dry run and a buffer one byte too small: verdict 1 with the statuses, nothing else
        for room in {0, max(total - 1, 0)} if total else set():
            r, st, o, l = GM.rebuild(hurt, BYTES, directory, 0, covered, S, G, guard, values, room)
            assert r == [1, total, len(values), wanted.count(0)] and st.tolist() == wanted and o is None and l is None, name
    # an inconsistent cursor protects nothing
    entries, values, _, _ = cases["one byte"]
    r, st, o, l = GM.rebuild(store, BYTES, np.array(entries, RM.LOC), 0, BYTES + 1, S, G, np.zeros(GM.guard_bytes(BYTES, S, G), np.uint8), values, BYTES)
    assert r == [2, 0, 1, 0] and st.tolist() == [2] and o is None


def test_a_collision_is_symmetric_and_needs_two_different_bytes(store):
    """Two positions collide together or not at all, whatever the order; overlapping extents of two entries share their common bytes
    without colliding there, and collide only where a byte of the one meets ANOTHER byte of the other."""
    G, W = 2, 2 * S
    guard = GM.guard_of(store, BYTES, S, G, BYTES)
    d = np.array([GM.entry(100, 400), GM.entry(S + 499, 300), GM.entry(300, 400), GM.entry(S + 800, 10), GM.entry(0, S), GM.entry(S - 1, S)], RM.LOC)
    for values, wanted in (([0, 1], [1, 1]), ([1, 0], [1, 1]), ([0, 2], [0, 0]), ([0, 2, 3], [0, 0, 0]), ([0, 2, 1], [1, 1, 1]), ([4, 5], [1, 1]),
                           ([4], [0]), ([5], [0]), ([0, 0, 1, 1], [1, 1, 1, 1])):
        assert GM.rebuild(store, BYTES, d, 0, BYTES, S, G, guard, values, BYTES)[1].tolist() == wanted, values


def test_the_cases_of_256_members():
    """G = 256, the single guard's maximum, over one group, one stripe of the next and a few bytes: the statuses the cases claim."""
    G, n = 256, 257 * S + 37
    big = np.random.default_rng(256).integers(0, 256, n, dtype=np.uint8)
    cases, guards = GM.rebuild_cases(G, S, n), {}
    assert {"members 254 and 255", "from member 255 into the next group"} <= set(cases) and "members 254 and 255" not in GM.rebuild_cases(3)
    for name, (entries, values, covered, wanted) in cases.items():
        directory = np.array(entries, RM.LOC)
        if covered not in guards:
            guards[covered] = GM.guard_of(big, covered, S, G, n)
        hurt = big.copy()
        for v in values:
            e = GM.extent_of(directory, 0, v, n, covered)
            if e:
                hurt[e[0]:e[0] + e[1]] ^= 0xA5
        result, status, out, locs = GM.rebuild(hurt, n, directory, 0, covered, S, G, guards[covered], values, n)
        assert status.tolist() == wanted and result[0] == 0, name
        for k, (v, s) in enumerate(zip(values, wanted)):
            if s == 0:
                pos, m, at = int(directory[v]["pos"]), int(directory[v]["stored"]), int(locs[k]["pos"])
                assert (out[at:at + m] == big[pos:pos + m]).all(), (name, k)
    ranges = GM.update_ranges(G, S, n)
    a, b = ranges["more than W bytes"]
    assert b - a > G * S and b == n and ranges["across a group boundary"][0] // (G * S) == 0
