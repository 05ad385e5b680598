"""The dedupe index's built digests (tests/dedupe_inputs.py) reach the edges they name: established on the CPU.

The fold copy is its own inverse where it claims to be; slots_after equals a plain sequential insert whatever the order; and per
case the homes, chain lengths, fold equalities, wraps, full tiles and absent queries are what the case was built for, the digests
that should be distinct are, and no call of a schedule can be refused by the index's admission check."""
import random

import pytest

import dedupe_inputs as X

FAMILIES = "ABCDEF"
# every edge the catalogue covers: a case that is dropped, or loses its tag, fails test_the_catalogue_covers_every_edge
EDGES = [
    "tile_edge_run", "full_tile", "tile_first_last_slot", "cap2", "cap4", "cap8",
    "chain_2", "chain_64", "chain_65", "chain_256", "chain_full",
    "chain_home_0", "chain_home_1", "chain_home_mid", "chain_home_cap-2", "chain_home_cap-1", "chain_home_cap-halfL", "chain_wraps",
    "collide_2", "collide_64", "collide_65", "collide_300",
    "merge_adjacent", "merge_touch", "merge_wraps",
    "across_calls",
    "zero", "ones", "fold0", "foldmax", "tail_1", "tail_63", "tail_64", "tail_65", "tail_255", "tail_256", "tail_257",
    "zero_first_repeated",
]
NAMES = sorted(X.CASES)


def sequential(ds, cap):
    """Linear probing into a list, one digest after the other: slot -> digest."""
    table = [None] * cap
    for d in ds:
        s = X.fold(d) & (cap - 1)
        while table[s] is not None:
            s = (s + 1) & (cap - 1)
        table[s] = d
    return table


def cluster_of(occupied, slot, cap):
    """(first slot, length) of the maximal cyclic run of occupied slots through `slot`."""
    assert slot in occupied and len(occupied) < cap
    first = slot
    while (first - 1) % cap in occupied:
        first = (first - 1) % cap
    n = 1
    while (first + n) % cap in occupied:
        n += 1
    return first, n


# ---- the fold copy -------------------------------------------------------------------------------------------------------
def test_unmix_undoes_mix():
    rng = random.Random(1)
    for x in [0, 1, X.M64, X.GOLD] + [rng.getrandbits(64) for _ in range(4000)]:
        assert X.unmix64(X.mix64(x)) == x and X.mix64(X.unmix64(x)) == x
    assert X.MUL1 * X.INV1 % 2 ** 64 == 1 and X.MUL2 * X.INV2 % 2 ** 64 == 1


@pytest.mark.parametrize("W", X.WIDTHS)
def test_a_digest_has_the_fold_asked_for(W):
    rng = random.Random(W)
    for T in [0, 1, X.M64, X.GOLD] + [rng.getrandbits(64) for _ in range(3000)]:
        d = X.digest(W, T, rng)
        assert len(d) == W and all(0 <= w <= X.M64 for w in d) and X.fold(d) == T
    for cap in (2, 4, 8, 512, 1 << 13, 1 << 40):
        for slot in (0, 1, cap // 2, cap - 1):
            assert X.fold(X.with_home(W, slot, cap, rng)) & (cap - 1) == slot
    ds = X.same_fold(W, 12345, 300, rng)
    assert len(set(ds)) == 300 and {X.fold(d) for d in ds} == {12345}
    assert X.words(X.rows(ds, W)) == ds and X.rows(ds, W).shape == (300, 8 * W)
    assert X.rows([(1,) + (0,) * (W - 1)], W)[0, :9].tolist() == [1] + [0] * 8          # little-endian words


def test_fold_is_the_splitmix64_chain():
    # splitmix64's first outputs from state 0 (Vigna's reference generator): mix64(k GOLD) for k = 1, 2, 3
    assert [X.mix64(k * X.GOLD & X.M64) for k in (1, 2, 3)] == [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]
    assert X.fold([]) == X.GOLD and X.fold([5]) == (X.mix64(X.GOLD ^ 5) + X.GOLD) & X.M64
    assert X.fold([1, 2]) != X.fold([2, 1])                                           # order-dependent


def test_cap_of():
    assert [X.cap_of(m) for m in (1, 2, 3, 4, 5)] == [2, 4, 8, 8, 16]
    for k in range(2, 41):
        assert X.cap_of(2 ** k - 1) == X.cap_of(2 ** k) == 2 ** (k + 1) and X.cap_of(2 ** k + 1) == 2 ** (k + 2)


# ---- slot positions -------------------------------------------------------------------------------------------------------
def test_slots_after_is_the_sequential_insert_in_any_order():
    rng = random.Random(2)
    trials = [(c.stored(), c.cap) for c in (X.CASES[n] for n in ("B_L256_scap-halfL_W2", "D_touch_s928_W4", "A_tile_W8", "A_cap4_W2"))]
    for cap, n in ((2, 1), (8, 4), (64, 32), (64, 9), (1024, 512), (1024, 300)):
        trials.append(([tuple(rng.getrandbits(64) for _ in range(2)) for _ in range(n)], cap))
    trials.append(([X.with_home(2, rng.choice((60, 61, 63, 0, 5)), 64, rng) for _ in range(30)], 64))   # clusters that wrap and merge
    for ds, cap in trials:
        want = X.slots_after(ds, cap)
        assert len(want) == len(ds)
        for _ in range(6):
            rng.shuffle(ds)
            table = sequential(ds, cap)
            assert {s for s in range(cap) if table[s] is not None} == want
            # and the sequential table, read in slot order, passes the order check (its own invariant)
            assert X.check_export_order([d for d in table if d is not None], cap) == sorted(want)


def test_check_export_order_refuses_a_wrong_order():
    rng = random.Random(3)
    cap = 64
    ds = [X.with_home(2, s, cap, rng) for s in (3, 9, 10, 40, 63)]
    assert X.check_export_order(ds, cap, exact=True) == [3, 9, 10, 40, 63]
    for bad in ([ds[1], ds[0]] + ds[2:], ds[:3] + [ds[4], ds[3]]):
        with pytest.raises(AssertionError):
            X.check_export_order(bad, cap, exact=True)
        with pytest.raises(AssertionError):
            X.check_export_order(bad, cap)
    with pytest.raises(AssertionError):
        X.check_export_order(ds + [ds[0]], cap)
    # inside a cluster of one home any order is a race's outcome; a digest of a LATER home in front of the cluster is not
    c = X.chain(2, 62, cap, 5, rng) + [X.with_home(2, 1, cap, rng)]           # slots 62, 63, 0, 1, 2 and, pushed on, 3
    table = sequential(c, cap)
    order = [d for d in table if d is not None]
    X.check_export_order(order, cap)
    X.check_export_order([order[1], order[0]] + order[2:], cap)                # two chain members swapped
    late = order.index(c[5])
    with pytest.raises(AssertionError):
        X.check_export_order([order[late]] + order[:late] + order[late + 1:], cap)


# ---- the catalogue ------------------------------------------------------------------------------------------------------------
def test_the_catalogue_covers_every_edge():
    for f in FAMILIES:
        for W in X.WIDTHS:
            assert X.family(f, W), (f, W)
    assert {c.family for c in X.CASES.values()} == set(FAMILIES)
    per_width = {W: sorted(n[:-len(f"_W{W}")] for n, c in X.CASES.items() if c.W == W) for W in X.WIDTHS}
    assert per_width[2] == per_width[4] == per_width[8]                        # every case at every width
    got = set().union(*(c.tags for c in X.CASES.values()))
    assert got == set(EDGES) and len(EDGES) == len(set(EDGES))
    for W in X.WIDTHS:
        assert set().union(*(c.tags for c in X.CASES.values() if c.W == W)) == set(EDGES), W
    for c in X.CASES.values():
        assert c.tags and c.note and c.alg == X.ALGS[c.W] and c.name.endswith(f"_W{c.W}")
    # the chain lengths and homes are the whole grid (but L = 2, where cap - L/2 is cap - 1)
    for W in X.WIDTHS:
        for L in X.CHAIN_LENGTHS:
            for s in X.CHAIN_HOMES:
                assert (f"B_L{L}_s{s}_W{W}" in X.CASES) == ((L, s) != (2, "cap-halfL"))


@pytest.mark.parametrize("name", NAMES)
def test_sizes_and_admission(name):
    c = X.CASES[name]
    assert c.W in X.WIDTHS and c.cap <= 8192 and c.cap == X.cap_of(c.max_entries)
    count, seen = 0, set()
    for call in c.calls:
        n = len(call.digests)
        assert 1 <= n <= 4096 and call.digests.shape == (n, c.db) and call.digests.dtype.name == "uint8"
        assert (call.base is None) != (call.values is None)
        if call.values is not None:
            assert call.values.shape == (n,) and call.values.dtype.name == "uint64" and (call.values != X.MISS).all()
        else:
            assert call.base + n < X.MISS
        # cw_dedupe's admission check counts every block of the batch, duplicates too: entries so far + n <= max_entries
        assert count + n <= c.max_entries, (name, count, n)
        seen.update(X.words(call.digests))
        count = len(seen)
    assert len(c.stored()) == count <= c.max_entries
    assert len(c.absent) == len(c.absent_claims) >= 1


@pytest.mark.parametrize("name", NAMES)
def test_the_case_is_what_it_claims(name):
    c = X.CASES[name]
    cap, stored = c.cap, c.stored()
    occupied = X.slots_after(stored, cap)
    kinds = set()
    for claim in c.claims:
        kind = claim[0]
        kinds.add(kind)
        if kind == "homes_distinct":
            assert len(set(X.homes(stored, cap))) == len(stored)
        elif kind == "occupied":
            assert occupied == set(claim[1]) == set(X.homes(stored, cap))
        elif kind == "full_tile":
            t = claim[1]
            assert all(s in occupied for s in range(t * X.TILE, (t + 1) * X.TILE)) and (t + 1) * X.TILE <= cap
            assert sum(1 for s in range(cap) if s in occupied and s // X.TILE != t) == len(occupied) - X.TILE
        elif kind == "chain":
            s, ds = claim[1], X.words(claim[2])
            folds = [X.fold(d) for d in ds]
            assert all(d in stored for d in ds) and len(set(ds)) == len(ds)
            assert {f & (cap - 1) for f in folds} == {s} and len(set(folds)) == len(ds)
            # the split at 2 and 4 times the capacity, and every member still on one home in any smaller table
            at2 = [f & (2 * cap - 1) for f in folds]
            assert at2.count(s) == (len(ds) + 1) // 2 and at2.count(s + cap) == len(ds) // 2
            at4 = [f & (4 * cap - 1) for f in folds]
            assert sorted(set(at4)) == [s + k * cap for k in range(min(4, len(ds)))]
            assert max(at4.count(h) for h in set(at4)) - min(at4.count(h) for h in set(at4)) <= 1
        elif kind == "collide":
            T, ds = claim[1], X.words(claim[2])
            assert all(d in stored for d in ds) and len(set(ds)) == len(ds) >= 2
            assert {X.fold(d) for d in ds} == {T}
        elif kind == "cluster":
            first, n = claim[1], claim[2]
            assert cluster_of(occupied, first, cap) == (first, n) and len(occupied) == n == len(stored)
        elif kind == "wrap":
            assert cap - 1 in occupied and 0 in occupied
            first, n = cluster_of(occupied, cap - 1, cap)
            assert first + n > cap and first != 0                              # one cluster holds slot cap - 1 and slot 0
        elif kind == "across_calls":
            chain = next(X.words(k[2]) for k in c.claims if k[0] == "chain")
            coll = next(X.words(k[2]) for k in c.claims if k[0] == "collide")
            one, two, three = (X.words(call.digests) for call in c.calls)
            for group in (chain, coll):
                first, second = [d for d in group if d in one], [d for d in group if d not in one]
                assert len(first) == len(second) == len(group) // 2 and set(second) <= set(two)
                assert sum(1 for d in first if d in two) >= 8                  # duplicates of call 1's entries
                assert sum(1 for d in second if two.count(d) > 1) >= 8         # duplicates within the batch
                assert sum(1 for d in first if d in three) >= 8 and sum(1 for d in second if d in three) >= 8
            fresh = [d for d in three if d not in one and d not in two]
            assert len(set(fresh)) >= 4 and all(three.count(d) == 2 for d in fresh)
            assert c.calls[2].values is not None and c.calls[0].base is not None and c.calls[1].base is not None
        elif kind == "digest":
            d, what = stored[claim[1]], claim[2]
            assert {"zero": d == X.ZERO(c.W), "ones": d == X.ONES(c.W), "fold0": X.fold(d) == 0, "foldmax": X.fold(d) == X.M64}[what]
            assert sum(1 for call in c.calls for e in X.words(call.digests) if e == d) >= 2
        elif kind == "tail":
            n = claim[1]
            batch = X.words(c.calls[0].digests)
            assert len(batch) == n and batch[-1] == X.ZERO(c.W) and batch.count(X.ZERO(c.W)) == 1 and len(set(batch)) == n
            assert X.ZERO(c.W) in X.words(c.calls[1].digests)
        elif kind == "zero_first":
            batch = X.words(c.calls[0].digests)
            assert batch[0] == X.ZERO(c.W) and batch.count(X.ZERO(c.W)) == claim[1]
            assert all(X.ZERO(c.W) in batch[k:k + 64] for k in range(0, len(batch), 64))
        else:
            raise AssertionError(f"unknown claim {kind}")
    assert kinds, name
    if c.family == "A":
        assert "homes_distinct" in kinds and "occupied" in kinds
        assert cap - 1 in occupied or c.name.startswith("A_run")
    if c.family in "BD":
        assert "chain" in kinds and "cluster" in kinds
        assert ("wrap" in kinds) == (cap - 1 in occupied and 0 in occupied)
    if c.family == "C":
        assert "collide" in kinds and "cluster" in kinds
        batch = X.words(c.calls[0].digests)                                     # leaders and followers interleaved
        assert all(batch.count(d) == 2 for d in stored[:-1]) and batch.count(stored[-1]) == 1
    if "chain_full" in c.tags:
        assert len(stored) == c.max_entries == cap // 2 and cluster_of(occupied, next(iter(occupied)), cap)[1] == cap // 2


@pytest.mark.parametrize("name", NAMES)
def test_absent_queries_are_absent_and_collide_as_claimed(name):
    c = X.CASES[name]
    cap, stored = c.cap, c.stored()
    have, occupied = set(stored), X.slots_after(stored, cap)
    absent = X.words(c.absent)
    assert len(set(absent)) == len(absent)
    for d, claim in zip(absent, c.absent_claims):
        assert d not in have, claim
        kind = claim[0]
        if kind == "home":
            assert X.fold(d) & (cap - 1) == claim[1] and claim[1] in occupied
        elif kind == "fold":
            assert X.fold(d) == claim[1] and any(X.fold(e) == claim[1] for e in stored)
        elif kind == "word":
            e = claim[1]
            assert e in have and [w for w in range(c.W) if d[w] != e[w]] == [claim[2]]
        elif kind == "twin":
            e = claim[1]
            assert e in have and X.fold(d) == X.fold(e) and [w for w in range(c.W) if d[w] != e[w]] == [claim[2], c.W - 1]
        elif kind == "inside":
            assert X.fold(d) & (cap - 1) == claim[1] and claim[1] in occupied
        elif kind == "free":
            assert X.fold(d) & (cap - 1) == claim[1] and claim[1] not in occupied
        else:
            assert kind == "any"
    if c.family in "BCDE":
        assert {"word", "twin"} <= {k[0] for k in c.absent_claims} or c.family == "D"
    if c.family in "BE":
        assert any(k[0] == "home" for k in c.absent_claims)
    if c.family in "CE":
        assert any(k[0] == "fold" for k in c.absent_claims)
    if c.family == "D":
        first, n = cluster_of(occupied, next(iter(occupied)), cap)
        inside = [k[1] for k in c.absent_claims if k[0] == "inside"]
        assert any(0 < (s - first) % cap < n - 1 for s in inside)              # a home in the middle of the cluster
