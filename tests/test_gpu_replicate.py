"""Chunk bundles on the GPU (cw_dev_dedupe_export_live, cw_dev_store_export_chunks, cw_dev_store_import_chunks, cw_dev_translate_refs
and cw.ChunkStore.export_bundle / import_bundle / replicate_to) against the plain-Python model of tests/replicate_model.py.

Device buffers carry canaries: byte buffers are prefilled with FILL and compared whole, entry and word arrays have guard
elements in front and behind."""
import numpy as np
import pytest

import cdc_model as CM
import replicate_model as PM
import restore_model as RM
import store_gc_model as GM
from conftest import corpus_file
from test_gpu_chunk_codec import _dev_u64, _stream, _u64
from test_gpu_dedupe_lifecycle import WIDTHS, crafted_digests, run_dedupe
from test_gpu_restore import ingest_both, same_as_model
from test_gpu_store_gc import Hand, _unsound

pytestmark = pytest.mark.gpu
FILL = 0xA5
GUARD = 256
ALGS = ["lz4", "lzf"]
P1K = CM.default_params(1024)
BAD_ARG, NOMEM = -2, -5
HAND_BASE = 77          # the directory base the hand-built store is used with


@pytest.fixture(scope="module")
def cw():
    import torch  # noqa: F401  (one HIP runtime for torch and libcwhc.so)
    import compute_war_amd as cw
    cw.init(0)
    yield cw
    cw.tune_reset()


@pytest.fixture(scope="module")
def O(oracle):
    return oracle


@pytest.fixture(scope="module")
def hand(cw):
    return Hand()


def _dev(a: np.ndarray):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def _sync():
    import torch
    torch.cuda.synchronize()


def u64cat(*parts):
    """The parts in a row as one uint64 array (np.concatenate would go through float64 when a part is a list of small ints)."""
    return np.concatenate([np.asarray(x, np.uint64).reshape(-1) for x in parts])


# ---- 1. export_live -------------------------------------------------------------------------------------------------------------
LIVE_BASE = 500


def live_pattern(n, pattern):
    live = np.zeros(n, np.uint32)
    if pattern == "all":
        live[:] = 3                      # any non-zero value is a flag
    elif pattern == "alternating":
        live[::2] = 1
    elif pattern == "last":
        live[-1] = 0x80000000
    else:
        assert pattern == "none"
    return live


def live_call(idx, db, live, dir_base, max_out, room):
    """cw_dev_dedupe_export_live into arrays of `room` slots prefilled with canaries: (values[room], digests[room, db], result)."""
    import torch
    d_live = _dev(np.concatenate([live, np.full(4, 0xFFFFFFFF, np.uint32)]))      # flags behind the directory: never read
    dig = torch.full((room * db,), 0xEE, dtype=torch.uint8, device="cuda")
    val = torch.full((room,), -2, dtype=torch.int64, device="cuda")
    res = torch.full((3,), -3, dtype=torch.int64, device="cuda")
    _sync()
    idx.dev_export_live(d_live.data_ptr(), dir_base, len(live), dig.data_ptr() if max_out else 0, val.data_ptr() if max_out else 0, max_out,
                        res.data_ptr(), _stream())
    _sync()
    result = _u64(res)
    assert result[2] == 2 ** 64 - 3, "result guard"
    return _u64(val), dig.cpu().numpy().reshape(room, db), result[:2].tolist()


def check_live(idx, db, pairs, live, dir_base, max_out):
    room = max_out + 3
    values, digests, result = live_call(idx, db, live, dir_base, max_out, room)
    want_values, cands, want_result = PM.export_live(pairs, live, dir_base, len(live), max_out)
    assert result == want_result
    k = len(want_values)
    assert k == min(want_result[0], max_out) and values[:k].tolist() == want_values
    assert (values[k:] == 2 ** 64 - 2).all() and (digests[k:] == 0xEE).all(), "slots behind min(L, max_out) were written"
    for j in range(k):
        got = digests[j].tobytes()
        assert got in cands[j] if cands[j] else got == bytes(db), (j, want_values[j])
    return want_result


@pytest.mark.parametrize("alg,db", WIDTHS)
def test_export_live(cw, alg, db):
    rng = np.random.default_rng(41 + db)
    n_dir = 9000
    d = crafted_digests(db, n_dir + 700, seed=500 + db, dups=False)
    # values: every directory entry but each 10th (flagged there = a value the index lacks), 600 entries outside the directory on
    # both sides, CW_DEDUPE_MISS - 1, and 100 second digests for values the index holds already
    inside = np.array([i for i in range(n_dir) if i % 10 != 7], np.uint64)
    rng.shuffle(inside)
    k = len(inside)
    values = u64cat(inside + np.uint64(LIVE_BASE), rng.integers(0, LIVE_BASE, 300), LIVE_BASE + n_dir + rng.integers(0, 1 << 40, 299), [RM.MISS - 1])
    twice = inside[:100] + np.uint64(LIVE_BASE)
    with cw.DedupeIndex(alg, 16384) as idx:
        run_dedupe(idx, d[:len(values)], values=values)
        pairs = [(d[i].tobytes(), int(values[i])) for i in range(len(values))]
        assert idx.count() == len(pairs) and k + 600 == len(values)

        def sweep(pairs, sizes):
            for n in sizes:
                for pattern in ("none", "all", "alternating", "last"):
                    live = live_pattern(n, pattern)
                    L = int(np.count_nonzero(live))
                    for max_out in sorted({0, max(L - 1, 0), L}):
                        result = check_live(idx, db, pairs, live, LIVE_BASE, max_out)
                        assert result[0] == L
            return result

        sweep(pairs, (1, 63, 64, 65, 257, n_dir))
        # a directory elsewhere: the low outside entries are inside now, the flagged values mostly absent
        check_live(idx, db, pairs, live_pattern(600, "all"), 0, 600)
        # two entries with one flagged value: one of their digests, whole, and more hits than flagged entries
        run_dedupe(idx, d[len(values):len(values) + 100], values=twice)
        pairs += [(d[len(values) + i].tobytes(), int(twice[i])) for i in range(100)]
        live = live_pattern(n_dir, "all")
        result = check_live(idx, db, pairs, live, LIVE_BASE, n_dir)
        assert result == [n_dir, k + 100]
        # after a resize the table is another one, the answers are the same
        idx.resize(40000)
        sweep(pairs, (65, n_dir))
        assert idx.count() == len(pairs)


# ---- 2. export_chunks over the hand-built store --------------------------------------------------------------------------------
def export_call(cw, h, values, out_bytes, shift=0, dry=False, count=None, max_count=None, d_dir=None, store_bytes=None):
    """cw_dev_store_export_chunks into canary-filled buffers: (the out_bytes of d_out, d_out_loc as int64 pairs [n, 2], result[3])."""
    import torch
    n = len(values)
    d_val, d_count = _dev_u64(list(values) + [HAND_BASE]), _dev_u64([n if count is None else count])
    buf = torch.full((GUARD + shift + out_bytes + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    loc = torch.full(((n + 2) * 2,), -1, dtype=torch.int64, device="cuda")             # a guard entry on each side
    res = torch.full((4,), -1, dtype=torch.int64, device="cuda")
    _sync()
    cw.dev_store_export_chunks(h.d_store.data_ptr(), h.store_bytes if store_bytes is None else store_bytes,
                               (h.d_dir if d_dir is None else d_dir).data_ptr(), HAND_BASE, h.n, d_val.data_ptr(), d_count.data_ptr(),
                               n if max_count is None else max_count, 0 if dry else buf.data_ptr() + GUARD + shift, 0 if dry else out_bytes,
                               loc.data_ptr() + 16, res.data_ptr(), _stream())
    _sync()
    host, locs, result = buf.cpu().numpy(), loc.cpu().numpy().reshape(-1, 2), _u64(res)
    lo = GUARD + shift
    assert (host[:lo] == FILL).all() and (host[lo + out_bytes:] == FILL).all(), "payload guards"
    assert (locs[0] == -1).all() and (locs[-1] == -1).all() and result[3] == RM.MISS, "loc / result guards"
    return host[lo:lo + out_bytes], locs[1:-1], result[:3].tolist()


def check_exported(got, model, n_written):
    out, locs, result = got
    verdict, want_result, blob, want_locs = model
    assert result == want_result
    if verdict:
        assert (out == FILL).all() and (locs == -1).all(), "a refused export wrote"
        return
    diff = np.nonzero(out[:len(blob)] != np.frombuffer(blob, np.uint8))[0]
    assert len(diff) == 0, ("payload differs at", int(diff[0]), len(diff))
    assert (out[len(blob):] == FILL).all(), "bytes behind the total were written"
    got_locs = np.ascontiguousarray(locs[:n_written]).view(RM.LOC).reshape(-1)
    bad = np.nonzero(got_locs != want_locs)[0]
    assert len(bad) == 0, ("loc", int(bad[0]), got_locs[bad[0]], want_locs[bad[0]], len(bad))
    assert (locs[n_written:] == -1).all(), "locs behind the count were written"


def hand_values(h):
    return (HAND_BASE + np.nonzero(h.directory["raw"])[0]).astype(np.uint64)


def model_export(h, values, out_bytes, directory=None, store_bytes=None):
    return PM.export_chunks(h.store, h.store_bytes if store_bytes is None else store_bytes, h.directory if directory is None else directory,
                            HAND_BASE, [int(v) for v in values], out_bytes)


def test_export_chunks_lists(cw, hand):
    asc = hand_values(hand)
    rng = np.random.default_rng(3)
    big = HAND_BASE + hand.n // 2 + 1
    repeats = u64cat(asc[:50], asc[:50], [big, big], rng.choice(asc, 300))
    for name, values in (("ascending", asc), ("reversed", asc[::-1]), ("repeats", repeats), ("empty", asc[:0])):
        model = model_export(hand, values, hand.store_bytes + 2 * 65536)
        assert model[0] == 0 and model[1][2] == len(values), name
        check_exported(export_call(cw, hand, values, model[1][1] + 32), (0, model[1], model[2], model[3]), len(values))
    # the count on the device: above max_count (max_count positions), below it (that many)
    model = model_export(hand, asc[:1000], 1 << 20)
    check_exported(export_call(cw, hand, asc, model[1][1], count=10 ** 12, max_count=1000), model, 1000)
    check_exported(export_call(cw, hand, asc[:1500], model[1][1], count=1000), model, 1000)
    check_exported(export_call(cw, hand, asc[:1500], 64, count=0), (0, [0, 0, 0], b"", np.zeros(0, RM.LOC)), 0)
    assert hand.d_store.cpu().numpy().tobytes() == hand.store.tobytes() and hand.d_dir.cpu().numpy().tobytes() == hand.directory.tobytes()


def test_export_chunks_every_destination_alignment(cw, hand):
    asc = hand_values(hand)
    at = int(np.nonzero(asc == HAND_BASE + hand.n // 2 + 1)[0][0])
    values = asc[at - 300:at + 300]                                    # the 65,536-byte entry among 599 small ones
    model = model_export(hand, values, 1 << 20)
    assert model[0] == 0 and model[1][1] > 65536
    for shift in range(16):
        check_exported(export_call(cw, hand, values, model[1][1], shift=shift), model, len(values))


def test_export_chunks_refusals_write_nothing(cw, hand):
    asc = hand_values(hand)
    values = asc[::3]
    model = model_export(hand, values, hand.store_bytes)
    total = model[1][1]
    assert model[0] == 0 and total > 65536
    refused = (1, [1, total, len(values)], None, None)
    check_exported(export_call(cw, hand, values, total - 1), refused, 0)               # one byte short
    check_exported(export_call(cw, hand, values, 16, dry=True), refused, 0)            # NULL / 0: the room needed
    # verdict 2: a value outside the directory on either side, CW_DEDUPE_MISS, an all-zero entry
    zero = HAND_BASE + int(np.nonzero(hand.directory["raw"] == 0)[0][5])
    for bad in (HAND_BASE - 1, HAND_BASE + hand.n, RM.MISS, 0, zero):
        with_bad = u64cat(values[:100], [bad], values[100:])
        model = model_export(hand, with_bad, hand.store_bytes)
        assert model[:2] == (2, [2, total, len(values) + 1]), bad
        check_exported(export_call(cw, hand, with_bad, hand.store_bytes), model, 0)
    # ... and each kind of unsound entry, named
    live = np.ones(hand.n, np.uint32)
    for name, i, entry in _unsound(hand, live):
        bad = hand.directory.copy()
        bad[i] = entry
        d_bad = _dev(bad)
        named = u64cat(values, [HAND_BASE + i])
        model = model_export(hand, named, hand.store_bytes, directory=bad)
        assert model[0] == 2, name
        check_exported(export_call(cw, hand, named, hand.store_bytes, d_dir=d_bad), model, 0)
        # the same directory without naming the entry: exported
        others = values[values != HAND_BASE + i]
        model = model_export(hand, others, hand.store_bytes, directory=bad)
        assert model[0] == 0, name
        check_exported(export_call(cw, hand, others, hand.store_bytes, d_dir=d_bad), model, len(others))
    # a store shorter than its directory says: entries past it are unsound, and nothing is loaded from there
    short = int(hand.directory[hand.n // 2]["pos"])
    model = model_export(hand, values, hand.store_bytes, store_bytes=short)
    assert model[0] == 2
    check_exported(export_call(cw, hand, values, hand.store_bytes, store_bytes=short), model, 0)


# ---- 3. import_chunks -------------------------------------------------------------------------------------------------------------
class Bundled:
    """A bundle made by the model from the hand-built store: 1,200 chunks, the 65,536-byte one among them."""

    def __init__(self, h):
        asc = hand_values(h)
        at = int(np.nonzero(asc == HAND_BASE + h.n // 2 + 1)[0][0])
        verdict, _, self.payload, self.locs = model_export(h, asc[at - 600:at + 600], 1 << 21)
        assert verdict == 0
        self.n = len(self.locs)
        self.d_in, self.d_loc = _dev(np.frombuffer(self.payload, np.uint8)), _dev(self.locs)


@pytest.fixture(scope="module")
def bundled(cw, hand):
    return Bundled(hand)


DIR_GUARD = 4


def import_call(cw, b, sel, base, used, store_bytes, dir_base, dir_entries, in_bytes=None, d_loc=None, count=None, max_count=None):
    """cw_dev_store_import_chunks into a canary-filled store and directory: (store bytes, directory int64 pairs, cursor, result[2])."""
    import torch
    buf = torch.full((GUARD + store_bytes + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    dirbuf = torch.full(((dir_entries + 2 * DIR_GUARD) * 2,), -1, dtype=torch.int64, device="cuda")
    d_used, res = _dev_u64([used, 99]), torch.full((3,), -1, dtype=torch.int64, device="cuda")
    d_count = _dev_u64([b.n if count is None else count])
    d_sel = d_nsel = None
    if sel is not None:
        d_sel, d_nsel = _dev(np.concatenate([np.asarray(sel, np.uint32), np.zeros(2, np.uint32)])), _dev_u64([len(sel)])
    _sync()
    cw.dev_store_import_chunks(b.d_in.data_ptr(), len(b.payload) if in_bytes is None else in_bytes, (b.d_loc if d_loc is None else d_loc).data_ptr(),
                               d_count.data_ptr(), b.n if max_count is None else max_count, base, buf.data_ptr() + GUARD, store_bytes,
                               d_used.data_ptr(), dirbuf.data_ptr() + 16 * DIR_GUARD, dir_base, dir_entries, res.data_ptr(), _stream(),
                               d_sel.data_ptr() if sel is not None else 0, d_nsel.data_ptr() if sel is not None else 0)
    _sync()
    host, d, cursor, result = buf.cpu().numpy(), dirbuf.cpu().numpy().reshape(-1, 2), _u64(d_used), _u64(res)
    assert (host[:GUARD] == FILL).all() and (host[GUARD + store_bytes:] == FILL).all(), "store guards"
    assert (d[:DIR_GUARD] == -1).all() and (d[-DIR_GUARD:] == -1).all() and cursor[1] == 99 and result[2] == RM.MISS, "directory / word guards"
    return host[GUARD:GUARD + store_bytes], d[DIR_GUARD:-DIR_GUARD], int(cursor[0]), result[:2].tolist()


def check_imported(got, model, used, dir_entries):
    store, d, cursor, result = got
    verdict, total, blob, entries = model
    assert result == [verdict, total]
    want_dir = np.full((dir_entries, 2), -1, np.int64)
    if verdict == 0:
        assert cursor == used + total
        diff = np.nonzero(store[used:used + total] != np.frombuffer(blob, np.uint8))[0]
        assert len(diff) == 0, ("store differs at", int(diff[0]), len(diff))
        for idx, e in entries.items():
            want_dir[idx] = np.array([e], RM.LOC).view(np.int64)
    else:
        assert cursor == used, "a refused import moved the cursor"
        total = 0
    assert (store[:used] == FILL).all() and (store[used + total:] == FILL).all(), "store bytes outside the append were written"
    bad = np.nonzero((d != want_dir).any(axis=1))[0]
    assert len(bad) == 0, ("entry", int(bad[0]), d[bad[0]], want_dir[bad[0]], len(bad))


def model_import(b, sel, base, used, store_bytes, dir_base, dir_entries, in_bytes=None, locs=None, n=None):
    return PM.import_chunks(b.payload, len(b.payload) if in_bytes is None else in_bytes, b.locs if locs is None else locs, b.n if n is None else n,
                            sel, base, used, store_bytes, dir_base, dir_entries)


def test_import_chunks_cursor_residues_and_selections(cw, bundled):
    b, room = bundled, len(bundled.payload) + 2000
    for r in range(16):
        used = 1000 + r
        for sel in (None, list(range(0, b.n, 2)), []):
            model = model_import(b, sel, 50, used, room, 40, 3000)
            assert model[0] == 0 and (model[1] > 65536) == (sel != [])
            check_imported(import_call(cw, b, sel, 50, used, room, 40, 3000), model, used, 3000)
    # a selection out of order; exactly enough room; the directory exactly the bundle's span
    sel = [5, 3, b.n - 1, 0]
    total = model_import(b, sel, 7, 0, 0, 7, b.n)[1]
    check_imported(import_call(cw, b, sel, 7, 0, total, 7, b.n), model_import(b, sel, 7, 0, total, 7, b.n), 0, b.n)
    # a chunk named twice is stored twice, and either entry stays
    sel = [5, 3, 3, 0]
    verdict, total, blob, entries = model_import(b, sel, 7, 0, 1 << 16, 7, b.n)
    store, d, cursor, result = import_call(cw, b, sel, 7, 0, 1 << 16, 7, b.n)
    first = (int(b.locs[5]["stored"]), int(b.locs[3]["stored"]), int(b.locs[3]["raw"]))
    assert result == [0, total] and cursor == total and store[:total].tobytes() == blob and entries[3] == (first[0] + first[1],) + first[1:]
    assert d[3].tolist() in [np.array([e], RM.LOC).view(np.int64).tolist() for e in (entries[3], first)]
    entries[3] = tuple(np.array(d[3]).view(RM.LOC)[0])
    check_imported((store, d, cursor, result), (verdict, total, blob, entries), 0, b.n)
    # the chunk count on the device: above max_count, and below it (every chunk behind it is out of the bundle)
    check_imported(import_call(cw, b, None, 50, 3, room, 40, 3000, count=10 ** 12, max_count=700), model_import(b, None, 50, 3, room, 40, 3000, n=700),
                   3, 3000)
    model = model_import(b, [0, 699, 700], 50, 3, room, 40, 3000, n=700)
    assert model[0] == 3
    check_imported(import_call(cw, b, [0, 699, 700], 50, 3, room, 40, 3000, count=700), model, 3, 3000)


def test_import_chunks_refusals_change_nothing(cw, bundled):
    b, room, used = bundled, len(bundled.payload) + 2000, 1003

    def refused(want, sel=None, base=50, store_bytes=room, dir_base=40, dir_entries=3000, **kw):
        model = model_import(b, sel, base, used, store_bytes, dir_base, dir_entries, in_bytes=kw.get("in_bytes"), locs=kw.get("locs"))
        assert model[0] == want, (want, model[:2])
        if "locs" in kw:
            kw["d_loc"] = _dev(kw.pop("locs"))
        check_imported(import_call(cw, b, sel, base, used, store_bytes, dir_base, dir_entries, **kw), model, used, dir_entries)
        return model

    # verdict 3: an index >= n, a zero entry, each unsound kind, an entry leaving in_bytes
    refused(3, sel=[0, 1, b.n])
    refused(3, sel=[0, 2 ** 32 - 1])
    zero = b.locs.copy()
    zero[10] = (0, 0, 0)
    refused(3, locs=zero)
    assert model_import(b, [i for i in range(b.n) if i != 10], 50, used, room, 40, 3000, locs=zero)[0] == 0     # not selected: no matter
    for field, value in (("stored", 0), ("raw", 65537), ("raw", int(b.locs[10]["raw"]) | 1 << 20), ("pos", len(b.payload)), ("pos", 2 ** 64 - 1)):
        bad = b.locs.copy()
        bad[10][field] = value
        refused(3, locs=bad)
    last = int(np.argmax(b.locs["pos"]))
    refused(3, in_bytes=len(b.payload) - 1)
    refused(3, sel=[last], in_bytes=len(b.payload) - 1)
    total = refused(3, sel=[0, last, b.n])[1]
    assert total == int(b.locs[0]["stored"]) + int(b.locs[last]["stored"])       # the total counts the sound positions
    # verdict 1: one byte short, and a cursor behind the store
    need = model_import(b, None, 50, used, room, 40, 3000)[1]
    refused(1, store_bytes=used + need - 1)
    refused(1, store_bytes=used - 1)
    check_imported(import_call(cw, b, None, 50, used, used + need, 40, 3000), model_import(b, None, 50, used, used + need, 40, 3000), used, 3000)
    # verdict 2: at both directory ends, and a value that wraps; verdict 1 wins over it
    refused(2, base=39)
    refused(2, base=40, dir_entries=b.n - 1)
    refused(2, base=2 ** 64 - 5, dir_base=2 ** 64 - 5)
    refused(1, base=39, store_bytes=used + need - 1)
    refused(3, sel=[0, b.n], base=39)
    check_imported(import_call(cw, b, None, 40, used, room, 40, b.n), model_import(b, None, 40, used, room, 40, b.n), used, b.n)


# ---- 4. translate_refs --------------------------------------------------------------------------------------------------------------
def translate_call(cw, refs, frm, to, count=None, max_count=None, npairs=None, max_pairs=None, in_place=False, missing=None):
    import torch
    n, p = len(refs), len(frm)
    d_ref = _dev_u64([7] + list(refs) + [7])                              # a guard on each side (in place: of the output too)
    d_from, d_to = _dev_u64(list(frm) + [0]), _dev_u64(list(to) + [0])
    d_count, d_np = _dev_u64([n if count is None else count]), _dev_u64([p if npairs is None else npairs])
    out = d_ref if in_place else torch.full((n + 2,), 7, dtype=torch.int64, device="cuda")
    missing = _dev_u64([0, 99]) if missing is None else missing
    _sync()
    cw.dev_translate_refs(d_ref.data_ptr() + 8, d_count.data_ptr(), n if max_count is None else max_count, d_from.data_ptr(), d_to.data_ptr(),
                          d_np.data_ptr(), p if max_pairs is None else max_pairs, out.data_ptr() + 8, missing.data_ptr(), _stream())
    _sync()
    got, m = _u64(out), _u64(missing)
    assert got[0] == 7 and got[-1] == 7 and m[1] == 99, "guards"
    if not in_place:
        assert _u64(d_ref)[1:-1].tolist() == [int(r) for r in refs], "the recipe was written"
    return got[1:-1].tolist(), int(m[0]), missing


def test_translate_refs(cw):
    rng = np.random.default_rng(9)
    for p in (0, 1, 2, 1000):
        frm = np.sort(rng.choice(np.arange(100, 100 + 4 * p + 4, dtype=np.uint64), p, replace=False))
        to = rng.integers(0, 1 << 62, p).astype(np.uint64)
        absent = np.setdiff1d(np.arange(100, 100 + 4 * p + 4, dtype=np.uint64), frm)
        refs = u64cat(frm, frm[::-1], rng.choice(absent, 300), [0, 99, 100 + 4 * p + 4, RM.MISS - 1, RM.MISS], rng.choice(frm, 500) if p else [])
        rng.shuffle(refs)
        want, want_missing = PM.translate(refs, frm, to)
        assert want_missing >= 305 and (p == 0 or want_missing < len(refs))
        got, m, counter = translate_call(cw, refs, frm, to)
        assert got == want and m == want_missing
        got, m, _ = translate_call(cw, refs, frm, to, in_place=True, missing=counter)           # in place; the counter accumulates
        assert got == want and m == 2 * want_missing
        # the counts on the device: only the first 100 positions, only the first half of the pairs
        want, want_missing = PM.translate(refs[:100], frm[:p // 2], to[:p // 2])
        got, m, _ = translate_call(cw, refs, frm, to, count=100, npairs=p // 2)
        assert got[:100] == want and got[100:] == [7] * (len(refs) - 100) and m == want_missing
        got, m, _ = translate_call(cw, refs, frm, to, count=10 ** 12, max_count=100, npairs=10 ** 12, max_pairs=p // 2)
        assert got[:100] == want and got[100:] == [7] * (len(refs) - 100) and m == want_missing


# ---- 5. end to end ------------------------------------------------------------------------------------------------------------------
class Pair:
    """Store A at directory base 0 holding a, b and c; store B at base 1000 with an index of its own holding b; their models."""

    def __init__(self, cw, O, alg, streams):
        a, b, c = streams
        self.idx_a, self.idx_b = cw.DedupeIndex("skein512", 2048), cw.DedupeIndex("skein512", 2048)
        self.A = cw.ChunkStore(self.idx_a, alg, cw.CdcParams.default(1024), 1 << 20, 512)
        self.mA = RM.Model(O, alg, 1 << 20, 512)
        (self.ra, _), (self.rb, _), (self.rc, _) = (ingest_both(self.A, self.mA, data, P1K) for data in (a, b, c))
        self.B, self.mB, self.rb_b = self.receiver(cw, O, alg, self.idx_b, b)

    @staticmethod
    def receiver(cw, O, alg, idx, b):
        B = cw.ChunkStore(idx, alg, cw.CdcParams.default(1024), 1 << 20, 1024, dir_base=1000)
        mB = RM.Model(O, alg, 1 << 20, 1024, dir_base=1000)
        rb_b, _ = ingest_both(B, mB, b, P1K)
        return B, mB, rb_b

    def close(self):
        self.idx_a.close()
        self.idx_b.close()


@pytest.fixture(scope="module")
def streams():
    return GM.three_streams(corpus_file("alice29.txt"), corpus_file("kennedy.xls"))


def state(cs):
    _sync()
    return cs.index.count(), cs.used(), cs.base, cs.d_dir.cpu().numpy().tobytes(), cs.d_store.cpu().numpy().tobytes()


def check_bundle(bundle, model_bundle):
    assert bundle.values.tolist() == model_bundle["values"]
    assert np.nonzero(bundle.carried)[0].tolist() == model_bundle["carried"]
    assert bundle.payload.tobytes() == model_bundle["payload"] and (bundle.locs.view(RM.LOC) == model_bundle["locs"]).all()


@pytest.mark.parametrize("alg", ALGS)
def test_replicate_two_streams_of_three(cw, O, alg, streams, tmp_path):
    a, b, c = streams
    p = Pair(cw, O, alg, streams)
    try:
        A, B, mA, mB = p.A, p.B, p.mA, p.mB
        refs = [p.ra.refs.tolist(), p.rc.refs.tolist()]
        base_b, count_b, before_a = B.base, p.idx_b.count(), state(A)
        ra_b, rc_b = A.replicate_to(B, [p.ra, p.rc])
        model_bundle, (mra, mrc), new = PM.replicate(mA, mB, refs, base_b)
        n = len(model_bundle["values"])
        # exactly the chunks B lacked went over: the index grew by them, the store by their stored bytes
        assert 0 < len(new) < n and p.idx_b.count() == count_b + len(new) == len(mB.values) and B.base == base_b + n
        same_as_model(B, mB)
        assert ra_b.refs.tolist() == mra and rc_b.refs.tolist() == mrc
        assert ra_b.offsets.tolist() == p.ra.offsets.tolist() and rc_b.offsets.tolist() == p.rc.offsets.tolist()
        assert B.restore(ra_b, verify=True) == a and B.restore(rc_b, verify=True) == c and B.restore(p.rb_b, verify=True) == b
        assert state(A) == before_a                                                  # the sender is only read
        # again: everything is known, nothing travels, B's store stays
        after = state(B)
        again = A.export_bundle([p.ra, p.rc], known=B)
        assert len(again.payload) == 0 and not again.carried.any() and len(again.values) == n
        ra2, rc2 = A.replicate_to(B, [p.ra, p.rc])
        now = state(B)
        assert (now[0], now[1], now[3], now[4]) == (after[0], after[1], after[3], after[4]) and now[2] == after[2] + n
        assert ra2.refs.tolist() == mra and rc2.refs.tolist() == mrc and B.restore(ra2, verify=True) == a

        # the bundles themselves, against the model, into fresh receivers
        with cw.DedupeIndex("skein512", 2048) as idx2, cw.DedupeIndex("skein512", 2048) as idx3:
            B2, mB2, _ = Pair.receiver(cw, O, alg, idx2, b)
            B3, mB3, _ = Pair.receiver(cw, O, alg, idx3, b)
            negotiated = A.export_bundle([p.ra, p.rc], known=B2)                     # a ChunkStore stands for its index
            full = A.export_bundle([p.ra, p.rc])
            check_bundle(negotiated, PM.export_bundle(mA, refs, mB2.values))
            check_bundle(full, PM.export_bundle(mA, refs))
            assert full.carried.all() and len(full.payload) > len(negotiated.payload) > 0
            assert np.nonzero(negotiated.carried)[0].tolist() == new and (negotiated.digests == full.digests).all()
            # a bundle survives save / load
            path = str(tmp_path / "bundle.npz")
            negotiated.save(path)
            loaded = cw.Bundle.load(path)
            for name in ("digests", "values", "locs", "payload"):
                assert getattr(loaded, name).tobytes() == getattr(negotiated, name).tobytes(), name
            assert (loaded.hash_alg, loaded.comp_alg) == (negotiated.hash_alg, negotiated.comp_alg) and len(loaded.recipes) == 2
            assert all(x.refs.tolist() == y.refs.tolist() and x.offsets.tolist() == y.offsets.tolist() for x, y in zip(loaded.recipes, [p.ra, p.rc]))
            got2 = B2.import_bundle(loaded)
            got3 = B3.import_bundle(full, verify=False)
            # without negotiation every chunk travels and the import still stores only what is new: the same store
            s2, s3 = state(B2), state(B3)
            assert s2 == s3 and (s2[1], s2[3], s2[4]) == (after[1], after[3], after[4])
            assert [r.refs.tolist() for r in got2] == [r.refs.tolist() for r in got3] == [mra, mrc]
            assert B2.restore(got2[0], verify=True) == a and B3.restore(got3[1], verify=True) == c
    finally:
        p.close()


@pytest.mark.parametrize("alg", ALGS)
def test_refused_bundles_leave_the_receiver_alone(cw, O, alg, streams):
    a, b, c = streams
    p = Pair(cw, O, alg, streams)
    try:
        A, B = p.A, p.B
        before = state(B)
        good = A.export_bundle([p.ra, p.rc], known=B)
        k = int(np.nonzero(good.carried)[0][0])
        assert good.carried.sum() > 1 and len(good.payload) > 100

        def tampered(**change):
            parts = dict(digests=good.digests.copy(), values=good.values.copy(), locs=good.locs.copy(), payload=good.payload.copy())
            for name, (at, flip) in change.items():
                parts[name].reshape(-1).view(np.uint8)[at] ^= flip
            return cw.Bundle(parts["digests"], parts["values"], parts["locs"], parts["payload"], good.hash_alg, good.comp_alg, good.recipes)

        cases = [("one payload byte", tampered(payload=(len(good.payload) // 2, 0x01)), True),
                 ("the first payload byte", tampered(payload=(0, 0x80)), True),
                 ("one manifest digest byte", tampered(digests=(k * good.digests.shape[1] + 3, 0x10)), True),
                 # a bundle negotiated with somebody who knows every chunk: nothing is carried, B lacks some
                 ("a chunk B lacks is not carried", A.export_bundle([p.ra, p.rc], known=A), True),
                 ("the same without verify", A.export_bundle([p.ra, p.rc], known=A), False),
                 ("a place that leaves the payload", tampered(locs=(16 * k + 8 + 3, 0x40)), False)]
        for name, bundle, verify in cases:
            with pytest.raises(cw.CwError) as e:
                B.import_bundle(bundle, verify=verify)
            assert e.value.code == BAD_ARG, name
            assert state(B) == before, name
        # no room: the index, the directory, the store
        for name, change in (("index", lambda: setattr(p.idx_b, "max_entries", before[0] + 1)), ("directory", lambda: setattr(B, "dir_entries", 100)),
                             ("store", lambda: setattr(B, "store_bytes", before[1] + 100))):
            keep = (p.idx_b.max_entries, B.dir_entries, B.store_bytes)
            change()
            try:
                with pytest.raises(cw.CwError) as e:
                    B.import_bundle(good)
                assert e.value.code == NOMEM, name
            finally:
                p.idx_b.max_entries, B.dir_entries, B.store_bytes = keep
            assert state(B) == before, name
        # another codec, another hash
        other = "lzf" if alg == "lz4" else "lz4"
        with cw.DedupeIndex("skein512", 64) as i1, cw.DedupeIndex("sha256mb", 64) as i2:
            with pytest.raises(ValueError):
                cw.ChunkStore(i1, other, cw.CdcParams.default(1024), 4096, 16).import_bundle(good)
            with pytest.raises(ValueError):
                cw.ChunkStore(i2, alg, cw.CdcParams.default(1024), 4096, 16).import_bundle(good)
            with pytest.raises(ValueError):
                A.export_bundle([p.ra], known=i2)
        # a recipe that names values the sender never had; a recipe whose chunk the sender's index forgot
        with pytest.raises(cw.CwError) as e:
            A.export_bundle([p.ra, cw.Recipe([600, RM.MISS], [0, 10, 20])])
        assert e.value.code == BAD_ARG
        # and after all that the good bundle goes in
        ra_b, rc_b = B.import_bundle(good)
        assert B.restore(ra_b, verify=True) == a and B.restore(rc_b, verify=True) == c
    finally:
        p.close()
