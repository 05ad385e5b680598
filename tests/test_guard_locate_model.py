"""The locate model on the CPU (guard_locate_model.py): its sums are guard_model's and guard2_model's folds, every named case's claim
is what the brute-force model gives, and each case reaches the edge it is named for -- the planted member is the located one, an
"ambiguous" cell has no member that fits, and the constructed double error really looks like a single one at a third member."""
import numpy as np
import pytest

import guard2_model as G2
import guard_locate_model as LM
import guard_model as GM

S = LM.S
GROUPS = [1, 2, 4, 16]


@pytest.fixture(scope="module")
def stores():
    """Noise, and its clean (P, Q) per (G, covered), each computed once."""
    cache = {}

    def get(G, covered=None):
        full = LM.store_bytes_of(G)
        covered = full if covered is None else covered
        if (G, covered) not in cache:
            host = np.random.default_rng(31).integers(0, 256, full, dtype=np.uint8)
            p, q, _ = LM.syndromes(host, covered, S, G)
            size = GM.guard_bytes(full, S, G)
            cache[G, covered] = (host, np.resize(p, size) * 0 + np.pad(p, (0, size - len(p))), np.pad(q, (0, size - len(q))))
        return cache[G, covered]
    return get


def test_the_sums_are_the_folds():
    """syndromes() against fold / fold_q, byte by byte, at cursors inside a stripe, at a group's end and at the store's."""
    for G in (1, 2, 3, 4):
        full = GM.STORE_BYTES
        host = np.random.default_rng(G).integers(0, 256, full, dtype=np.uint8)
        for covered in (0, 1, S + 77, G * S, full - 11, full):
            p, q, below = LM.syndromes(host, covered, S, G)
            want_p, want_q = G2.guards_of(host, covered, S, G, full)
            assert (p == want_p[:len(p)]).all() and not want_p[len(p):].any(), (G, covered)
            assert (q == want_q[:len(q)]).all() and not want_q[len(q):].any(), (G, covered)
            count = np.zeros(len(p), np.int64)
            np.add.at(count, GM.cells(np.arange(covered), S, G), 1)
            assert (below == count).all(), (G, covered)


def test_store_sizes():
    assert [LM.store_bytes_of(G) for G in (1, 2, 4)] == [GM.STORE_BYTES] * 3
    assert LM.store_bytes_of(16) == 17 * S + 37 and LM.store_bytes_of(255) == 256 * S and LM.store_bytes_of(256) == 257 * S


def _run(stores, G, case, dual):
    host, p, q = stores(G, case.covered)
    covered = LM.store_bytes_of(G) if case.covered is None else case.covered
    s, dp, dq = LM.damaged(host, p, q if dual else None, case.damage)
    return (s, dp, dq, covered) + LM.locate(s, len(host), LM.records(case.entries), covered, S, G, dp, dq)


@pytest.mark.parametrize("G", GROUPS)
def test_every_claim_is_the_models(stores, G):
    cases = LM.cases(G)
    assert {"two wrong bytes that alias", "two wrong bytes, different deltas"} <= set(cases) or G < 3
    for name, case in cases.items():
        for dual in (False, True):
            s, dp, dq, covered, result, suspect = _run(stores, G, case, dual)
            assert suspect.tolist() == (case.dual if dual else case.single), (name, dual)
            assert result[0] == 0 and result[1] == -(-covered // (G * S)) and result[2] == result[3] + result[4], (name, dual)
            assert result[5] == sum(1 for v in suspect if v & 3) and result[6] == sum(1 for v in suspect if v == 4) and result[7] == 0
            if not dual:
                assert result[3] == 0, name
            # no more cells are dirty than bytes were changed, and without damage none is
            assert result[2] <= len(case.damage) and (result[2] > 0) == bool([d for d in case.damage if dual or d[0] != "q"]) \
                or name == "two wrong bytes, equal deltas", (name, dual)


@pytest.mark.parametrize("G", GROUPS)
def test_every_case_reaches_its_edge(stores, G):
    """On the dual call the cells the cases name have the class they name: the planted member, or none."""
    for name, case in LM.cases(G).items():
        s, dp, dq, covered, result, suspect = _run(stores, G, case, True)
        cls, pd, qd = LM.classes(s, covered, S, G, dp, dq)
        for at, want in case.cells.items():
            cell = int(GM.cells(at, S, G))
            assert cls[cell] == want, (name, at)
            if want >= 0 and name != "two wrong bytes that alias":
                assert want == int(G2.members(at, S, G)), (name, "the planted member is the located one")
            if want == LM.AMBIGUOUS and pd[cell] and qd[cell]:
                # no member below the cursor fits: brute force over every m
                fits = [m for m in range(G) if at // (G * S) * G * S + m * S + at % S < covered and G2.MUL[G2.POW[m], pd[cell]] == qd[cell]]
                assert fits == [], (name, fits)


@pytest.mark.parametrize("G", [4, 16])
def test_the_aliasing_pair_aliases(stores, G):
    """(a, member 0) and (b, member 1) in one cell give Q' / P' = 2^k with k a third member below the cursor: the cell is LOCATED(k),
    the two damaged entries get no bit and the sound entry in member k gets bit 0 -- why a locate is a hint and never a verdict."""
    case = LM.cases(G)["two wrong bytes that alias"]
    (_, at0, a), (_, at1, b) = case.damage
    assert G2.members(at0, S, G) == 0 and G2.members(at1, S, G) == 1 and GM.cells(at0, S, G) == GM.cells(at1, S, G)
    pd, qd = a ^ b, int(G2.MUL[G2.POW[0], a]) ^ int(G2.MUL[G2.POW[1], b])
    k = LM.ratio(pd, qd)
    assert pd and qd and k not in (0, 1) and k < G and int(G2.MUL[G2.POW[k], pd]) == qd
    s, dp, dq, covered, result, suspect = _run(stores, G, case, True)
    cls, _, _ = LM.classes(s, covered, S, G, dp, dq)
    assert cls[int(GM.cells(at0, S, G))] == k and result[2:5] == [1, 1, 0]
    assert suspect.tolist() == [0, 0, 1] and int(case.entries[2][0]) // S == k
    # the same two bytes with deltas no member fits are ambiguous, and both entries are suspected
    other = LM.cases(G)["two wrong bytes, different deltas"]
    assert _run(stores, G, other, True)[5].tolist()[:2] == [2, 2]


def test_largest_groups():
    """G = 255 has every ratio below the cursor's members, so two wrong bytes always alias; G = 256 is the single call's alone."""
    assert LM.two_errors(0, 1, 255, alias=False) == (None, None, None)
    a, b, k = LM.two_errors(0, 1, 255, alias=True)
    assert k not in (0, 1) and k < 255
    assert LM.two_errors(0, 1, 2, alias=True) == (None, None, None)
    assert "two wrong bytes that alias" in LM.cases(255) and "two wrong bytes, different deltas" not in LM.cases(255)
    assert "two wrong bytes that alias" not in LM.cases(2)
