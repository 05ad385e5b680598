"""The dedupe index differential: the built digests of tests/dedupe_inputs.py -- chosen home slots, chains of any length, walks that
wrap from the last slot to slot 0, distinct digests of one 64-bit fold, full export tiles, tables smaller than a tile -- through
cw_dev_dedupe / _insert / _lookup / _export, cw_dedupe_resize / _retain and the piecewise host export and import.

What ref, new_idx, n_new, n_found and the count should be comes from the dict model of test_gpu_dedupe_lifecycle.py alone.  The
copy of the kernel's fold in dedupe_inputs.py only aims the inputs and checks slot positions (check_export_order); the first test
of this file calibrates it against the kernels, and every other test stands on that.  test_dedupe_inputs.py establishes on the CPU
that every case reaches the edge it names."""
import random

import numpy as np
import pytest

import dedupe_inputs as X
import store_gc_model as GM
from test_gpu_dedupe_lifecycle import Model, _dev, pairs, run_dedupe, run_export, run_lookup

pytestmark = pytest.mark.gpu

MISS = X.MISS
NAMES = sorted(X.CASES)
A_CASES = sorted(X.family("A"))
RESIZE_CASES = sorted(n for f in "BCDE" for n in X.family(f))
RETAIN_CASES = sorted(n for f in "BC" for n in X.family(f))
PIECE_CASES = sorted(n for n in NAMES if n.startswith(("A_tile_", "B_L256_scap-halfL_")))
LOST_AIM = ("the export of a case whose homes are all distinct is not in ascending home order: the fold copy in "
            "tests/dedupe_inputs.py no longer matches fold / dedupe_cap of dedupe_kernels.hip / cw_dedupe.hip, so no case of "
            "this file reaches the edge it names")


@pytest.fixture(scope="module")
def cw():
    import torch  # noqa: F401  (one HIP runtime for torch and libcwhc.so)
    import compute_war_amd as cw
    cw.init(0)
    return cw


def run_schedule(cw, case):
    """A fresh index with the case's calls made: (index, model); every call's outputs compared with the model's."""
    idx, model = cw.DedupeIndex(case.alg, case.max_entries), Model()
    try:
        for k, call in enumerate(case.calls):
            if call.values is None:
                ref, new_idx = run_dedupe(idx, call.digests, call.base)
                mref, mnew = model.call(call.digests, call.base)
            else:
                ref, new_idx = run_dedupe(idx, call.digests, values=call.values)
                mref, mnew = model.insert(call.digests, call.values)
            bad = np.nonzero(ref != mref)[0]
            assert bad.size == 0, (case.name, "call", k, "ref differs first at", int(bad[0]), int(ref[bad[0]]), int(mref[bad[0]]))
            assert len(new_idx) == len(mnew), (case.name, "call", k, "n_new", len(new_idx), len(mnew))
            bad = np.nonzero(new_idx != mnew)[0]
            assert bad.size == 0, (case.name, "call", k, "new_idx differs first at", int(bad[0]), int(new_idx[bad[0]]), int(mnew[bad[0]]))
            assert idx.count() == len(model.table), (case.name, "call", k, "count", idx.count(), len(model.table))
    except BaseException:
        idx.close()
        raise
    return idx, model


def export_all(idx, db, offset=0):
    """The whole export with 7 poisoned pairs of room behind it: (digests[count, db], values[count])."""
    count = idx.count()
    dig, val, n = run_export(idx, db, count + 7, offset=offset)
    assert n == count
    assert (dig[n:] == 0xEE).all() and (val[n:] == MISS).all()
    return dig[:n], val[:n]


def batches(case, seed):
    """Every stored digest and every absent one, shuffled, in lookups of at most 4,096 whose last wavefront is partial."""
    q = np.concatenate([X.rows(case.stored(), case.W), case.absent])
    q = q[np.random.default_rng(seed).permutation(len(q))]
    out = []
    for at in range(0, len(q), 4001):       # 4001 = 62 wavefronts and 33 lanes
        b = q[at:at + 4001]
        out.append(b if len(b) % 64 else np.concatenate([b, b[:1]]))
    return out


def check_lookups(case, idx, model, seed=1):
    """ref and n_found exact over stored and absent queries; returns the refs."""
    refs = []
    for k, b in enumerate(batches(case, seed)):
        ref, nf = run_lookup(idx, b)
        mref, mnf = model.lookup(b)
        bad = np.nonzero(ref != mref)[0]
        assert bad.size == 0, (case.name, "lookup", k, "ref differs first at", int(bad[0]), int(ref[bad[0]]), int(mref[bad[0]]))
        assert nf == mnf, (case.name, "lookup", k, "n_found", nf, mnf)
        refs.append(ref)
    for at in range(0, len(case.absent), 4033):                       # the absent ones alone: all miss
        aref, anf = run_lookup(idx, case.absent[at:at + 4033])
        assert anf == 0 and (aref == MISS).all(), (case.name, "an absent digest was found")
    return np.concatenate(refs)


def check_table(case, idx, model, max_entries=None):
    """The export as a set is the model's, and its order obeys linear probing at the index's capacity."""
    dig, val = export_all(idx, case.db)
    assert set(pairs(dig, val)) == model.items() and len(val) == len(model.table), case.name
    X.check_export_order(dig, X.cap_of(idx.max_entries if max_entries is None else max_entries), exact=case.family == "A")
    return dig, val


# ---- 1. calibration: the fold copy aims where the kernels look ---------------------------------------------------------------
@pytest.mark.parametrize("name", A_CASES)
def test_calibration_export_of_distinct_homes_is_in_home_order(cw, name):
    case = X.CASES[name]
    idx, model = run_schedule(cw, case)
    with idx:
        dig, _ = export_all(idx, case.db)
        got = X.homes(dig, case.cap)
        want = sorted(next(k[1] for k in case.claims if k[0] == "occupied"))
        assert got == want, LOST_AIM


@pytest.fixture(scope="module")
def aimed(cw):
    """Every other test of this file depends on the calibration: they fail with its message when the fold copy has lost its aim."""
    for W in X.WIDTHS:
        case = X.CASES[f"A_run_W{W}"]
        idx, _ = run_schedule(cw, case)
        with idx:
            dig, _ = export_all(idx, case.db)
            if X.homes(dig, case.cap) != list(range(128, 384)):
                pytest.fail(LOST_AIM)
    return True


# ---- 2. the call schedule ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_schedule(cw, aimed, name):
    case = X.CASES[name]
    idx, model = run_schedule(cw, case)                               # asserts call by call
    with idx:
        assert idx.count() == len(case.stored())


# ---- 3. lookup -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_lookup(cw, aimed, name):
    case = X.CASES[name]
    idx, model = run_schedule(cw, case)
    with idx:
        count = idx.count()
        before = export_all(idx, case.db)
        first = check_lookups(case, idx, model)
        assert (first != MISS).sum() >= count and (first == MISS).sum() >= len(case.absent)
        again = check_lookups(case, idx, model)
        assert np.array_equal(first, again) and idx.count() == count
        after = export_all(idx, case.db)                              # the index is unchanged
        assert before[0].tobytes() == after[0].tobytes() and before[1].tobytes() == after[1].tobytes()
        # a lookup-or-insert of the absent digests finds nothing either, and then they are there
        room = case.max_entries - count
        if room:
            ref, new_idx = run_dedupe(idx, case.absent[:room], base=1 << 52)
            mref, mnew = model.call(case.absent[:room], 1 << 52)
            assert np.array_equal(ref, mref) and np.array_equal(new_idx, mnew) and len(mnew) == min(room, len(case.absent))
            q = np.concatenate([X.rows(case.stored(), case.W), case.absent[:room]])
            ref, nf = run_lookup(idx, q)
            assert np.array_equal(ref, model.lookup(q)[0]) and nf == len(q)
            X.check_export_order(export_all(idx, case.db)[0], case.cap)


# ---- 4. export -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_export(cw, aimed, name):
    case = X.CASES[name]
    idx, model = run_schedule(cw, case)
    with idx:
        count, db = idx.count(), case.db
        dig, val = check_table(case, idx, model)
        dig8, val8 = export_all(idx, db, offset=8)                    # the 8-byte store path: the same bytes
        assert dig8.tobytes() == dig.tobytes() and val8.tobytes() == val.tobytes()
        cuts = {count - 1}
        full = [k[1] for k in case.claims if k[0] == "full_tile"]
        if full:                                                      # max_out ends inside the wholly occupied tile
            slots = X.check_export_order(dig, case.cap, exact=True)
            at = slots.index(full[0] * X.TILE)
            assert slots[at + X.TILE - 1] == full[0] * X.TILE + X.TILE - 1
            cuts |= {at, at + 1, at + X.TILE - 1, at + X.TILE}
        for max_out in sorted(cuts):
            for off in (0, 8):                                        # a truncated export is a prefix of the full one
                digt, valt, nt = run_export(idx, db, max_out, room=count + 3, offset=off)
                assert nt == count, (case.name, max_out, off)
                assert digt[:max_out].tobytes() == dig[:max_out].tobytes() and np.array_equal(valt[:max_out], val[:max_out]), (case.name, max_out, off)
                assert (digt[max_out:] == 0xEE).all() and (valt[max_out:] == MISS).all(), (case.name, max_out, off)


# ---- 5. resize -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", RESIZE_CASES)
def test_resize(cw, aimed, name):
    case = X.CASES[name]
    idx, model = run_schedule(cw, case)
    with idx:
        count = idx.count()
        want = check_lookups(case, idx, model)
        for max_entries in (4 * case.max_entries, count, 2 * count):   # grow x 4, shrink to exactly the count, grow x 2
            idx.resize(max_entries)
            assert idx.max_entries == max_entries and idx.count() == count, (case.name, max_entries)
            assert np.array_equal(check_lookups(case, idx, model), want), (case.name, max_entries)
            check_table(case, idx, model)


# ---- 6. retain -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", RETAIN_CASES)
def test_retain(cw, aimed, name):
    """The directory lies just below 2^64, so value - dir_base wraps for every entry below it.  Member i of the chain or collision set
    names directory entry i and is live when i is even -- but every eighth is given a value outside the directory (below its base, or
    behind its end) and stays whatever the flags say."""
    import torch
    case = X.CASES[name]
    stored = next(X.words(k[2]) for k in case.claims if k[0] in ("chain", "collide"))
    n = len(stored)
    assert n == len(case.stored())
    entries = n
    base = 2 ** 64 - 9 - entries                                      # the directory ends 8 below CW_DEDUPE_MISS
    rng = random.Random(n + case.W)
    values = np.array([base + i for i in range(n)], np.uint64)
    for i in range(3, n, 8):
        values[i] = (rng.randrange(base), base - 1, base + entries, MISS - 1)[(i // 8) % 4]
    d = X.rows(stored, case.W)
    order = np.random.default_rng(n).permutation(n)
    for mode in ("alternate", "none", "all"):
        live = np.array([{"alternate": i % 2 == 0, "none": False, "all": True}[mode] for i in range(entries)], np.uint32) * 3
        d_live = _dev(live)
        with cw.DedupeIndex(case.alg, case.max_entries) as idx:
            model = Model()
            ref, new_idx = run_dedupe(idx, d[order], values=values[order])
            mref, mnew = model.insert(d[order], values[order])
            assert np.array_equal(ref, mref) and np.array_equal(new_idx, mnew) and len(mnew) == n
            kept = GM.retain(model.table, live, base, entries)
            outside = sum(1 for i in range(n) if not base <= int(values[i]) < base + entries)
            assert len(kept) == {"alternate": sum(1 for i in range(n) if i % 2 == 0 or i % 8 == 3), "none": outside, "all": n}[mode]
            assert outside == len(range(3, n, 8))
            torch.cuda.synchronize()
            assert idx.retain(d_live.data_ptr(), base, entries) == n - len(kept), (case.name, mode)
            model.table = kept
            assert idx.count() == len(kept) and idx.max_entries == case.max_entries
            ref = check_lookups(case, idx, model)                     # dropped digests miss, kept ones hit with their value
            assert (ref != MISS).sum() == len(kept)
            check_table(case, idx, model)
            dropped = np.array([i for i in range(n) if d[i].tobytes() not in kept], np.int64)
            assert len(dropped) == n - len(kept)
            if len(dropped):                                          # the dropped digests go in again, under new values
                new_values = np.arange(77, 77 + len(dropped), dtype=np.uint64)
                ref, new_idx = run_dedupe(idx, d[dropped], values=new_values)
                mref, mnew = model.insert(d[dropped], new_values)
                assert np.array_equal(ref, new_values) and np.array_equal(ref, mref) and np.array_equal(new_idx, mnew)
                assert idx.count() == n
                check_lookups(case, idx, model)
                check_table(case, idx, model)


# ---- 7. the host export in pieces -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", PIECE_CASES)
def test_host_export_in_pieces(cw, aimed, name):
    case = X.CASES[name]
    idx, model = run_schedule(cw, case)
    with idx:
        dig, val = export_all(idx, case.db)
        slots = X.check_export_order(dig, case.cap, exact=case.family == "A")
        first_of_full_tile = slots.index(X.TILE) if case.family == "A" else 2
        assert first_of_full_tile == 2
        want = check_lookups(case, idx, model)
        for piece in (1, 255, 256, 257, first_of_full_tile):          # windows that start and end inside a tile
            idx.set_stage_entries(piece)
            hdig, hval = idx.export()
            assert hdig.shape == dig.shape and hdig.tobytes() == dig.tobytes() and np.array_equal(hval, val), (case.name, piece)
        for piece, max_entries in ((255, 4 * case.max_entries), (1, len(val))):
            with cw.DedupeIndex(case.alg, max_entries) as other:      # into an empty index of another capacity
                other.set_stage_entries(piece)
                assert other.import_(hdig, hval) == len(val) == other.count()
                assert np.array_equal(check_lookups(case, other, model), want)
                X.check_export_order(export_all(other, case.db)[0], X.cap_of(max_entries))
