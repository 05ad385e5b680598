"""The recipe diff and the delta apply on the GPU (cw_dev_recipe_diff, cw_dev_apply_delta, cw.ChunkStore.diff / delta,
cw.apply_delta) against tests/delta_model.py, byte for byte.

Device buffers carry canaries: every output is prefilled, has guard words behind it and is compared whole; inputs have words behind
their counts that would show in the result if they were read.  The position counts are the edges of a wavefront (64) and of a
workgroup (256), the op lengths those of copy_g2g's paths (64 bytes, 16-byte vectors) and of the apply's tile."""
import numpy as np
import pytest

import delta_model as DM
from conftest import corpus_file

pytestmark = pytest.mark.gpu
M = DM.M
NONE = DM.NONE
POISON = 0xA5A5A5A5A5A5A5A5
FILL = 0xA5
G = 4                   # guard words behind every output
ALGS = ["lz4", "lzf"]
OP = np.dtype([(k, "<u8") for k in ("b_off", "len", "a_off", "payload_off")])
TILE = 16 << 10         # CW_DELTA_TILE=16, the default: many tiles stay small


@pytest.fixture(scope="module")
def cw():
    import torch  # noqa: F401  (one HIP runtime for torch and libcwhc.so)
    import compute_war_amd as cw
    cw.init(0)
    yield cw
    cw.tune_reset()


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _dev_u64(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.uint64).view(np.int64).copy()).cuda()


def _dev_u8(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def _host_u64(t):
    return t.cpu().numpy().view(np.uint64)


def _poison(words):
    return _dev_u64(np.full(words, POISON, np.uint64))


# ---- 1. the diff on hand-built recipes -----------------------------------------------------------------------------------------------
def diff_call(cw, ref_a, off_a, ref_b, off_b, dir_base, entries, max_ops=None, count_a=None, count_b=None, behind=None, src=True, ranges=True, want=None):
    """One cw_dev_recipe_diff into poisoned buffers, compared whole with the model; returns (the model's result, the outputs' bytes).
    The device lists hold max_a = len(ref_a) and max_b = len(ref_b) positions; count_a / count_b are what the count words hold
    (default: the lengths), and the model sees min(count, max) positions.  behind: (ref, offset step) of G more positions behind
    each list, which no call may read.  want: the model's result, when the caller has it already."""
    import torch
    ref_a, off_a, ref_b, off_b = (np.asarray(x, np.uint64) for x in (ref_a, off_a, ref_b, off_b))
    max_a, max_b = len(ref_a), len(ref_b)
    na, nb = min(max_a if count_a is None else count_a, max_a), min(max_b if count_b is None else count_b, max_b)
    want = want or DM.diff(ref_a[:na].tolist(), off_a[:na + 1].tolist(), ref_b[:nb].tolist(), off_b[:nb + 1].tolist(), dir_base, entries, max_ops)
    room = max(want["totals"][1] or 0, 1) if max_ops is None else max_ops

    def lists(ref, off):
        if behind is None:
            return _dev_u64(np.concatenate([ref, np.zeros(1, np.uint64)])), _dev_u64(off)
        more = off[-1] + np.uint64(behind[1]) * np.arange(1, G + 1, dtype=np.uint64)
        return _dev_u64(np.concatenate([ref, np.full(G, behind[0], np.uint64)])), _dev_u64(np.concatenate([off, more]))

    (d_ref_a, d_off_a), (d_ref_b, d_off_b) = lists(ref_a, off_a), lists(ref_b, off_b)
    d_na, d_nb = _dev_u64([max_a if count_a is None else count_a]), _dev_u64([max_b if count_b is None else count_b])
    ops, nops, d_src, totals = _poison((room + G) * 4), _poison(3), _poison(max_b + G), _poison(8 + G)
    new = [_poison(room + G) for _ in range(3)] + [_poison(3)]
    torch.cuda.synchronize()
    cw.dev_recipe_diff(d_ref_a.data_ptr(), d_off_a.data_ptr(), d_na.data_ptr(), max_a, d_ref_b.data_ptr(), d_off_b.data_ptr(), d_nb.data_ptr(), max_b,
                       dir_base, entries, ops.data_ptr() if room else 0, room, nops.data_ptr() + 8, totals.data_ptr(), _stream(),
                       d_src.data_ptr() if src else 0, *((t.data_ptr() + (8 if i == 3 else 0) if ranges else 0) for i, t in enumerate(new)))
    torch.cuda.synchronize()
    got = [_host_u64(t) for t in (ops, nops, d_src, totals, *new)]
    h_ops, h_nops, h_src, t, h_off, h_len, h_dst, h_nnew = got
    assert (_host_u64(d_off_a)[:max_a + 1] == off_a).all() and (_host_u64(d_ref_b)[:max_b] == ref_b).all(), "an input was written"
    assert (t[8:] == POISON).all() and h_nops[0] == h_nops[2] == h_nnew[0] == h_nnew[2] == POISON, "guards around totals / counts"
    untouched = lambda *arrays: all((x == POISON).all() for x in arrays)  # noqa: E731
    if want["verdict"] == 1:
        assert t[0] == 1 and untouched(t[1:], h_ops, h_nops, h_src, h_off, h_len, h_dst, h_nnew), "a refused call wrote more than its verdict"
        return want, [x.tobytes() for x in got]
    assert t[:8].tolist() == want["totals"], (t[:8].tolist(), want["totals"])
    assert h_src[:nb].tolist() == want["src"] if src else untouched(h_src[:nb]), "src"
    assert untouched(h_src[nb:]), "src behind the count"
    k = len(want["ops"])
    assert int(h_nops[1]) == k and (not ranges or int(h_nnew[1]) == len(want["ranges"]))
    body = h_ops[:4 * k].view(OP)
    model = np.array(want["ops"], np.uint64).reshape(k, 4).view(OP).reshape(-1) if k else np.zeros(0, OP)
    bad = np.nonzero(body != model)[0]
    assert len(bad) == 0, ("op", int(bad[0]), body[bad[0]], model[bad[0]], len(bad))
    assert untouched(h_ops[4 * k:]), "ops behind the count"
    if ranges:
        r = len(want["ranges"])
        assert list(zip(h_off[:r].tolist(), h_len[:r].tolist(), h_dst[:r].tolist())) == want["ranges"]
        assert untouched(h_off[r:], h_len[r:], h_dst[r:]), "ranges behind the count"
    else:
        assert untouched(h_off, h_len, h_dst, h_nnew), "a NULL range array was written"
    return want, [x.tobytes() for x in got]


def hand_pair(n, seed, dir_base, entries, off_a0=0, off_b0=0):
    """A of n positions and a B made from it: positions dropped, fresh ones and ones outside the directory inserted, two blocks
    swapped (moved runs), a few lengths changed.  Refs repeat (a sixth of the draws come from 9 entries); a ref's length is a
    function of the ref except where it was changed.  Entries from 3/4 of the directory up are named by B alone."""
    rng = np.random.default_rng(seed)
    len_of = rng.integers(1, 400, entries).astype(np.uint64)
    len_of[::13] = 65536
    old_part = max(entries * 3 // 4, 1)
    idx_a = np.where(rng.random(n) < 0.17, rng.integers(0, min(old_part, 9), n), rng.integers(0, old_part, n))
    idx_b = idx_a[rng.random(n) > 0.03]
    if len(idx_b) > 8:                                                   # swap two blocks
        c = np.sort(rng.choice(len(idx_b), 4, replace=False))
        idx_b = np.concatenate([idx_b[:c[0]], idx_b[c[2]:c[3]], idx_b[c[1]:c[2]], idx_b[c[0]:c[1]], idx_b[c[3]:]])
    k = max(n // 20, 1)
    idx_b = np.insert(idx_b, rng.integers(0, len(idx_b) + 1, k), rng.integers(old_part, max(entries, old_part + 1), k) % entries)
    len_b = len_of[idx_b]
    ref_b = (np.uint64(dir_base % M) + idx_b.astype(np.uint64))          # wraps in u64
    odd = rng.random(len(idx_b))
    ref_b[odd < 0.01] = (dir_base - 1) % M
    ref_b[(odd >= 0.01) & (odd < 0.02)] = (dir_base + entries) % M
    ref_b[(odd >= 0.02) & (odd < 0.03)] = NONE                           # CW_DEDUPE_MISS
    len_b[(odd >= 0.03) & (odd < 0.04)] += np.uint64(1)                  # equal ref, other length
    len_b = np.minimum(len_b, np.uint64(65536))
    ref_a = np.uint64(dir_base % M) + idx_a.astype(np.uint64)
    odd = rng.random(n)
    ref_a[odd < 0.01] = NONE
    ref_a[(odd >= 0.01) & (odd < 0.02)] = (dir_base + entries) % M
    off = lambda lens, at: np.concatenate([[at], at + np.cumsum(lens, dtype=np.uint64)]).astype(np.uint64)  # noqa: E731
    return ref_a, off(len_of[idx_a], np.uint64(off_a0)), ref_b, off(len_b, np.uint64(off_b0))


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257])
def test_hand_built_recipes(cw, n):
    """n positions at the wavefront and workgroup edges, a base near 2^64 so that ref - dir_base wraps, lists that start anywhere"""
    seen = set()
    for seed, (dir_base, entries) in enumerate([(7, 300), (M - 100, 257), (1 << 40, 64)]):
        ref_a, off_a, ref_b, off_b = hand_pair(n, 100 * n + seed, dir_base, entries, off_a0=seed * 1000, off_b0=5 + seed)
        want, _ = diff_call(cw, ref_a, off_a, ref_b, off_b, dir_base, entries)
        seen |= {k for k, v in zip(DM.TOTALS, want["totals"]) if v}
        diff_call(cw, ref_b, off_b, ref_a, off_a, dir_base, entries, src=False)                     # the reverse; a NULL d_src
        diff_call(cw, ref_a, off_a, ref_b, off_b, dir_base, entries, ranges=False)
        same, _ = diff_call(cw, ref_b, off_b, ref_b, off_b + np.uint64(77), dir_base, entries)       # against itself
        inside = ((ref_b - np.uint64(dir_base % M)) < np.uint64(entries)).all()
        assert not inside or len(ref_b) == 0 or same["ops"] == [(0, int(off_b[-1] - off_b[0]), 0, NONE)]
    if n >= 255:
        assert {"ops", "new_ops", "in_place_bytes", "moved_bytes", "new_bytes", "matched_positions"} <= seen, seen


def test_more_positions_than_the_grid_has_lanes(cw):
    """600,000 positions: the capped grid is 2048 workgroups of 256 lanes, so the grid-stride loops turn; two runs give the same bytes"""
    dir_base, entries = 11, 1 << 18
    ref_a, off_a, ref_b, off_b = hand_pair(600_000, 26, dir_base, entries)
    want, first = diff_call(cw, ref_a, off_a, ref_b, off_b, dir_base, entries)
    assert want["totals"][1] > 50_000 and want["totals"][4] > 0
    _, second = diff_call(cw, ref_a, off_a, ref_b, off_b, dir_base, entries, want=want)
    assert first == second


def test_the_rule_case_by_case(cw):
    call = lambda *a, **kw: diff_call(cw, *a, **kw)[0]  # noqa: E731
    # A names a ref at three positions: the lowest wins (B's position is at another offset, so it is not in place)
    want = call([5, 9, 5, 8, 5], [0, 10, 20, 30, 40, 50], [7, 5], [0, 3, 13], 0, 16)
    assert want["src"] == [NONE, 0]
    # an in-place match beats a lower position
    want = call([5, 6, 5], [0, 4, 8, 12], [6, 6, 5], [0, 4, 8, 12], 0, 16)
    assert want["src"] == [4, 4, 8] and want["ops"] == [(0, 4, 4, NONE), (4, 8, 4, NONE)]
    # equal ref, other length: new -- in place and moved
    assert call([5], [0, 10], [5], [0, 11], 0, 16)["src"] == [NONE]
    assert call([4, 5], [0, 10, 20], [5], [0, 11], 0, 16)["src"] == [NONE]
    # the lowest position has another length than the in-place one: only the in-place position matches
    assert call([5, 5], [0, 10, 21], [9, 5], [0, 10, 21], 0, 16)["src"] == [NONE, 10]
    # refs below dir_base, at dir_base + dir_entries and CW_DEDUPE_MISS are new, in place too, and are no source
    for base in (3, M - 40):
        out = [base - 1, base + 5, NONE]
        for r in out:
            want = call([r, base % M], [0, 1, 2], [r, r, base % M], [0, 1, 2, 3], base, 5)
            assert want["src"] == [NONE, NONE, 1] and want["ops"] == [(0, 2, NONE, 0), (2, 1, 1, NONE)]
        assert call([(base + 4) % M], [0, 1], [(base + 4) % M], [7, 8], base, 5)["src"] == [0]      # the last entry is one
    # no positions: in A, in B, in both; with lists that hold positions behind the count
    ref, off = np.arange(3, 13), np.arange(0, 110, 10)
    assert call(ref, off, ref, off, 0, 16, count_a=0)["totals"] == [0, 1, 1, 0, 0, 100, 0, 10]
    assert call(ref, off, ref, off, 0, 16, count_b=0)["totals"] == [0, 0, 0, 0, 0, 0, 0, 0]
    assert call(ref, off, ref, off, 0, 16, count_a=0, count_b=0)["ops"] == []
    assert call([], [0], [], [9], 0, 1)["ops"] == []
    assert call([], [0], [2], [9, 12], 0, 16)["ops"] == [(0, 3, NONE, 0)]
    # huge counts: the lists end at max; what lies behind them would match (same ref, offsets going on) if it were read
    for count in (11, 1 << 32, M - 1):
        want = call(ref, off, ref[::-1], off, 0, 16, count_a=count, count_b=count, behind=(3, 10))
        assert want["totals"][7] == 10 and want["totals"][1] == 10
    # a count below max hides what lies behind it
    assert call(ref, off, ref, off, 0, 16, count_a=4, count_b=6)["ops"] == [(0, 40, 0, NONE), (40, 20, NONE, 0)]


@pytest.mark.parametrize("side", ["a", "b"])
def test_a_list_that_the_library_does_not_write_is_refused(cw, side):
    ref = np.arange(300, dtype=np.uint64)
    good = np.arange(1, 302, dtype=np.uint64) * np.uint64(50)
    for at in (0, 63, 64, 255, 256, 299):
        for what in ("equal", "decreasing", "long"):
            off = good.copy()
            if what == "equal":
                off[at + 1] = off[at]
            elif what == "decreasing":
                off[at + 1] = off[at] - np.uint64(1)
            else:
                off[at + 1:] += np.uint64(65537 - 50)
            pair = (ref, off, ref, good) if side == "a" else (ref, good, ref, off)
            assert diff_call(cw, *pair, 0, 300)[0]["verdict"] == 1, (at, what)
    long_ok = good.copy()
    long_ok[150:] += np.uint64(65536 - 50)                                                         # 65,536 is what the library writes
    pair = (ref, long_ok, ref, good) if side == "a" else (ref, good, ref, long_ok)
    assert diff_call(cw, *pair, 0, 300)[0]["verdict"] == 0
    hidden = good.copy()
    hidden[200] = hidden[199]                                                                      # behind the count: not looked at
    pair, kw = ((ref, hidden, ref, good), dict(count_a=199)) if side == "a" else ((ref, good, ref, hidden), dict(count_b=199))
    assert diff_call(cw, *pair, 0, 300, **kw)[0]["verdict"] == 0


def test_too_many_ops_write_none_and_the_dry_run_sizes_the_buffers(cw):
    ref_a, off_a, ref_b, off_b = hand_pair(1000, 5, 7, 300)
    full, _ = diff_call(cw, ref_a, off_a, ref_b, off_b, 7, 300)
    ops = full["totals"][1]
    assert ops > 100
    for max_ops in (ops - 1, 1, 0):
        dry, _ = diff_call(cw, ref_a, off_a, ref_b, off_b, 7, 300, max_ops=max_ops)
        assert dry["verdict"] == 2 and dry["totals"][1:] == full["totals"][1:]
    assert diff_call(cw, ref_a, off_a, ref_b, off_b, 7, 300, max_ops=ops)[0]["verdict"] == 0
    assert diff_call(cw, ref_a, off_a, ref_b, off_b, 7, 300, max_ops=ops + 50)[0]["verdict"] == 0


# ---- 2. the apply on hand-built ops --------------------------------------------------------------------------------------------------
def apply_call(cw, old, payload, ops, dst_bytes=None, count=None, behind=None, tile=None, shift=(0, 0, 0)):
    """One cw_dev_apply_delta into a canary-filled destination, compared whole with the model; returns the model's result words.
    shift: how far d_old, d_payload and d_dst lie behind a 256-byte boundary.  behind: an op behind the list, which no call may read."""
    import torch
    ops = [tuple(int(v) for v in o) for o in ops]
    max_ops = len(ops)
    n = min(max_ops if count is None else count, max_ops)
    total = sum(o[1] for o in ops[:n]) if all(o[1] < (1 << 40) for o in ops[:n]) else 0
    dst_bytes = total if dst_bytes is None else dst_bytes
    want = DM.check(ops[:n], len(old), len(payload), dst_bytes)
    room = max(dst_bytes, want[1] if want[0] == 2 else 0)
    d_old = _dev_u8(np.concatenate([np.zeros(shift[0], np.uint8), np.frombuffer(old, np.uint8), np.full(64, 0x11, np.uint8)]))
    d_pay = _dev_u8(np.concatenate([np.zeros(shift[1], np.uint8), np.frombuffer(payload, np.uint8), np.full(64, 0x22, np.uint8)]))
    d_dst = _dev_u8(np.full(shift[2] + room + 256, FILL, np.uint8))
    listed = np.array(ops + [behind or (0, 1, 0, NONE)], np.uint64).reshape(-1)
    d_ops, d_n, res = _dev_u64(listed), _dev_u64([max_ops if count is None else count]), _poison(4 + G)
    torch.cuda.synchronize()
    with cw.tuned(**({"CW_DELTA_TILE": tile} if tile else {})):
        cw.dev_apply_delta(d_old.data_ptr() + shift[0], len(old), d_pay.data_ptr() + shift[1], len(payload), d_ops.data_ptr(), d_n.data_ptr(), max_ops,
                           d_dst.data_ptr() + shift[2], dst_bytes, res.data_ptr(), _stream())
    torch.cuda.synchronize()
    r, out = _host_u64(res), d_dst.cpu().numpy()
    assert tuple(r[:4].tolist()) == want, (r[:4].tolist(), want)
    assert (r[4:] == POISON).all() and (_host_u64(d_ops) == listed).all(), "guards behind d_result; the ops were written"
    if want[0]:
        assert (out == FILL).all(), "a refused call wrote the destination"
        return want
    new = DM.apply(old, payload, ops[:n])
    got = out[shift[2]:shift[2] + want[1]].tobytes()
    if got != new:
        at = next(i for i, (x, y) in enumerate(zip(got, new)) if x != y)
        raise AssertionError(f"byte {at} of {len(new)} differs: {got[at]} != {new[at]}")
    assert (out[:shift[2]] == FILL).all() and (out[shift[2] + want[1]:] == FILL).all(), "a byte outside d_dst[0, total) was written"
    return want


def sources(n_old, n_payload, seed=1):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, n_old, dtype=np.uint8).tobytes(), rng.integers(0, 256, n_payload, dtype=np.uint8).tobytes()


def ops_of(lens, n_old, seed=2):
    """ops of these lengths, copies and new ops in turn (two copies never adjacent in A), the new ops' bytes back to back"""
    rng = np.random.default_rng(seed)
    ops, b, p = [], 0, 0
    for k, n in enumerate(lens):
        if k % 2:
            ops.append((b, n, NONE, p))
            p += n
        else:
            ops.append((b, n, int(rng.integers(0, n_old - n + 1)), NONE))
        b += n
    return ops, p


@pytest.mark.parametrize("tile", [16, 64, 256])
def test_op_lengths_at_the_copy_and_tile_edges(cw, tile):
    t = tile << 10
    lens = [1, 15, 16, 17, 63, 64, 65, t - 1, 1, t, 3, t + 1, 64, 65, 63, 17, 16, 15, 1]
    old, _ = sources(t + 500, 0)
    ops, p = ops_of(lens, len(old))
    _, payload = sources(0, p)
    apply_call(cw, old, payload, ops, tile=tile)
    apply_call(cw, old, payload, ops, tile=tile, shift=(3, 9, 5))
    apply_call(cw, old, payload, ops[:7], tile=tile)                                              # less than a tile in all
    apply_call(cw, old, payload, [], tile=tile)                                                   # no op: total 0, nothing written
    apply_call(cw, old, payload, ops, tile=tile, count=0)


def test_every_alignment_of_source_and_destination(cw):
    old, payload = sources(16 * 300 + 200, 16)
    ops, b = [], 0
    for sa in range(16):
        for da in range(16):
            fill = (da - b) % 16
            if fill:
                ops.append((b, fill, NONE, 0))
                b += fill
            n = 100 + (sa * 16 + da) % 37
            ops.append((b, n, 16 * (sa * 16 + da) + sa, NONE))
            b += n
    for shift in ((0, 0, 0), (0, 0, 1), (7, 0, 0), (15, 3, 9)):
        apply_call(cw, old, payload, ops, shift=shift)
    # the same from the payload
    pay_ops = [(o[0], o[1], NONE, o[2]) if o[2] != NONE else (o[0], o[1], 0, NONE) for o in ops]
    apply_call(cw, payload + bytes(16), old, pay_ops, shift=(0, 5, 11))


def test_one_op_across_many_tiles_and_many_ops_in_one(cw):
    old, payload = sources(40 * TILE + 999, 20 * TILE + 77)
    apply_call(cw, old, payload, [(0, 37 * TILE + 123, 700, NONE)], tile=16)
    apply_call(cw, old, payload, [(0, 5, 1, NONE), (5, 20 * TILE + 70, NONE, 7), (20 * TILE + 75, 30 * TILE, 5 * TILE + 3, NONE)], tile=16, shift=(1, 2, 3))
    # 300 ops inside one tile, behind one long op and in front of another: more than the 64 a wavefront looks at at a time
    lens = [TILE + 11] + [int(v) for v in np.random.default_rng(3).integers(1, 40, 300)] + [2 * TILE]
    ops, p = ops_of(lens, len(old))
    assert p <= len(payload) and sum(lens[1:-1]) < TILE
    apply_call(cw, old, payload, ops, tile=16)
    apply_call(cw, old, payload, ops)                                                             # the default tile
    apply_call(cw, old, payload, ops, tile=64)
    apply_call(cw, old, payload, ops_of([1] * 700, len(old))[0], tile=16)                         # bytes, one op each
    # counts: below the list, far above it; the op behind the list would be a gap if it were read
    apply_call(cw, old, payload, ops, count=150, tile=16)
    for count in (len(ops) + 1, 1 << 32, M - 1):
        apply_call(cw, old, payload, ops, count=count, behind=(5, 1, 0, NONE), tile=16)


def test_malformed_lists_are_named_and_write_nothing(cw):
    old, payload = sources(1000, 300)
    good = ops_of([200, 100, 300, 100, 64, 100], len(old))[0]
    assert apply_call(cw, old, payload, good)[0] == 0
    for k in (0, 1, 2, 5):
        b, n, a, p = good[k]
        copy = a != NONE
        cases = {
            "gap": (b + 1, n, a, p), "overlap": (b - 1, n, a, p) if k else None, "empty": (b, 0, a, p), "both": (b, n, NONE, NONE),
            "neither": (b, n, 0, 0), "wrap": (b, M - b, a, p) if k else None, "wrap2": (b, n, M - 1 - n // 2, NONE) if copy else (b, n, NONE, M - 1 - n // 2),
            "outside": (b, n, len(old) - n + 1, NONE) if copy else (b, n, NONE, len(payload) - n + 1),
            "far": (b, n, 1 << 40, NONE) if copy else (b, n, NONE, 1 << 40),
            "long": (b, len(old) + 1, 0, NONE) if copy else (b, len(payload) + 1, NONE, 0)}
        for name, op in cases.items():
            if op is None:
                continue
            ops = good[:k] + [op] + good[k + 1:]
            want = apply_call(cw, old, payload, ops, dst_bytes=1 << 12)
            assert want[:3] == (1, 0, k), (name, k, want)
    # two bad ops: the lowest is named, wherever the other is; 3,000 ops with bad ones in different workgroups
    assert apply_call(cw, old, payload, [good[0], (200, 0, NONE, 0)] + good[2:5] + [(9, 9, 9, 9)], dst_bytes=1 << 12)[2] == 1
    many = ops_of([1] * 3000, len(old))[0]
    for bad in ((2999,), (300, 2999), (2998, 257), (0, 1500)):
        ops = list(many)
        for k in bad:
            ops[k] = (ops[k][0], 0, ops[k][2], ops[k][3])
        assert apply_call(cw, old, sources(0, 3000)[1], ops, dst_bytes=1 << 12)[:3] == (1, 0, min(bad))
    # a sound list at the edges of its sources: the last byte of each
    edge = [(0, 10, len(old) - 10, NONE), (10, 10, NONE, len(payload) - 10)]
    assert apply_call(cw, old, payload, edge)[0] == 0
    # the destination is too small: the total is reported, nothing is written
    for dst_bytes in (0, 1, 863):
        assert apply_call(cw, old, payload, good, dst_bytes=dst_bytes)[:2] == (2, 864)
    assert apply_call(cw, old, payload, good, dst_bytes=864 + 100)[0] == 0


# ---- 3. through ChunkStore ------------------------------------------------------------------------------------------------------------
def stream_bytes():
    rng = np.random.default_rng(26)
    return corpus_file("alice29.txt")[:150_000] + bytes(60_000) + rng.integers(0, 256, 50_000, dtype=np.uint8).tobytes()


def same_diff(a, b):
    assert a.ops.tobytes() == b.ops.tobytes() and a.src.tobytes() == b.src.tobytes() and a.totals == b.totals


@pytest.mark.parametrize("alg", ALGS)
def test_versions_travel_as_deltas(cw, alg, tmp_path):
    data = stream_bytes()
    rng = np.random.default_rng(7)
    fresh = lambda n: rng.integers(0, 256, n, dtype=np.uint8).tobytes()  # noqa: E731
    cs = cw.ChunkStore(cw.DedupeIndex("skein512", 1 << 14), alg, cw.CdcParams.default(256), 4 << 20, 1 << 14, 7)
    try:
        A = cs.ingest(data)
        versions = {"overwrite": cs.write(A, 70_001, fresh(4096)), "insert": cs.patch(A, 33_333, 0, fresh(777)),
                    "removal": cs.patch(A, 100_000, 5_000, b""), "append": cs.append(A, fresh(3000)), "truncate": cs.truncate(A, 200_123)}
        versions["several"] = cs.patch_many(A, [(10, 5, b"hello"), (160_000, 100, fresh(900)), (250_000, 0, fresh(64))])
        bytes_a = cs.restore(A)
        assert bytes_a == data
        before, contents = {}, {}
        for name, B in versions.items():
            bytes_b = contents[name] = cs.restore(B)
            for old, new, b_old, b_new in ((A, B, bytes_a, bytes_b), (B, A, bytes_b, bytes_a)):
                d, delta = cs.diff(old, new), cs.delta(old, new)
                want = DM.diff(old.refs.tolist(), old.offsets.tolist(), new.refs.tolist(), new.offsets.tolist(), cs.dir_base, cs.dir_entries)
                assert [tuple(int(v) for v in o) for o in d.ops] == want["ops"] and d.src.tolist() == want["src"], name
                assert [d.totals[k] for k in cw.DIFF_TOTALS] == want["totals"][1:]
                assert d.changed_ranges() == [(o[0], o[1]) for o in want["ops"] if o[2] == NONE]
                assert delta.ops.tobytes() == d.ops.tobytes() and (delta.old_bytes, delta.new_bytes) == (len(b_old), len(b_new))
                assert delta.payload.tobytes() == DM.payload_of(b_new, want["ops"]), name
                assert cw.apply_delta(b_old, delta) == b_new, name
                assert b"".join(cs.read_ranges(new, d.changed_ranges())) == delta.payload.tobytes()
            path = str(tmp_path / f"{name}.npz")
            delta.save(path)                                                                      # (the reverse one: B -> A)
            loaded = cw.Delta.load(path)
            assert loaded.ops.tobytes() == delta.ops.tobytes() and loaded.payload.tobytes() == delta.payload.tobytes()
            assert cw.apply_delta(bytes_b, loaded) == bytes_a
            assert cs.diff(A, B, max_ops=1).ops.tobytes() == cs.diff(A, B).ops.tobytes()          # the dry run sizes the second call
            before[name] = cs.diff(A, B)
        one = cs.diff(A, A)
        assert [tuple(int(v) for v in o) for o in one.ops] == [(0, len(data), 0, NONE)]
        # a delta against the wrong stream, and a damaged one, are refused
        delta = cs.delta(A, versions["insert"])
        with pytest.raises(cw.CwError) as e:
            cw.apply_delta(bytes_a[:-1], delta)
        assert e.value.code == -2
        broken = cw.Delta(delta.ops.copy(), delta.payload, delta.old_bytes, delta.new_bytes)
        broken.ops["len"][2] += 1
        with pytest.raises(cw.CwError) as e:
            cw.apply_delta(bytes_a, broken)
        assert e.value.code == -2 and e.value.op == 3 and "op 3" in str(e.value)
        # compact and renumber change where chunks lie and what they are called, not what changed
        names = list(versions)
        cs.compact([A] + [versions[k] for k in names])
        for k in names:
            same_diff(cs.diff(A, versions[k]), before[k])
        recipes = cs.renumber([A] + [versions[k] for k in names], dir_base=1 << 33)
        assert not (recipes[0].refs == A.refs).all()
        for k, B in zip(names, recipes[1:]):
            same_diff(cs.diff(recipes[0], B), before[k])
            assert cw.apply_delta(bytes_a, cs.delta(recipes[0], B)) == cs.restore(B)
        # a stored chunk that only the new version names is damaged: the delta names the range
        A2, B2 = recipes[0], recipes[1 + names.index("overwrite")]
        d = cs.diff(A2, B2)
        lost = int(np.nonzero(d.src == np.uint64(NONE))[0][0])
        cs.d_dir.view(-1, 2)[int(B2.refs[lost]) - cs.dir_base] = 0
        with pytest.raises(cw.CwError) as e:
            cs.delta(A2, B2)
        assert e.value.code == -2 and "range 0" in str(e.value) and f"offset {d.changed_ranges()[0][0]}," in str(e.value)
        assert cw.apply_delta(contents["overwrite"], cs.delta(B2, A2)) == bytes_a                  # the other way reads no chunk that only B names
    finally:
        cs.index.close()
