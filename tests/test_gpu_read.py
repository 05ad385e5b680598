"""cw_dev_read_ranges and cw.ChunkStore.read / read_ranges on the GPU against the plain-Python model of tests/read_model.py and the
input's own bytes.  Everything is byte-exact.

The destination and the statuses carry canaries: the destination is prefilled with FILL and compared whole against an image made
from the model's answers (the extent of a range with status 1 or 2 is unspecified and blanked on both sides), statuses behind the
count keep their -1."""
import threading

import numpy as np
import pytest

import cdc_model as CM
import read_model as RD
import restore_model as RM
from test_gpu_chunk_codec import Run, _dev_u64, _stream
from test_gpu_restore import FILL, GUARD, Store, ingest_both, restore_call
from test_read_abi import P1K, P256, damaged_stream, largest_input, mixed_input, stored_forms, window_input, window_ranges

pytestmark = pytest.mark.gpu
ALGS = ["lz4", "lzf"]
HUGE = [2 ** 64 - 1, 2 ** 63, 2 ** 62 + 12345, 2 ** 64 - 4096, 2 ** 40]


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


def _decode(O, alg):
    return O.lz4_decompress if alg == "lz4" else O.lzf_decompress


def build(cw, O, alg, data: bytes, cuts, dir_base=0):
    """A canary-guarded Store holding every chunk of `data`, checked against the model's image; refs[j] = dir_base + j."""
    a = np.frombuffer(data, np.uint8)
    k = len(cuts) - 1
    st = Store(len(data) + 64, k + 2, dir_base=dir_base)
    st.append(cw, alg, Run(cw, alg, a, cuts=cuts).fetch(), base=dir_base)
    assert st.expect(O, alg, a, cuts, range(k), dir_base)[0] == 0
    st.check()
    return st, [dir_base + j for j in range(k)]


def packed(ranges, gap=0):
    """[(offset, length)] -> ([(offset, length, destination)], dst_bytes): the destinations back to back, `gap` bytes apart."""
    out, at = [], 0
    for a, l in ranges:
        out.append((a, l, at))
        at += l + gap
    return out, at


class Call:
    """The device arrays of one cw_dev_read_ranges call, made before it is queued."""

    def __init__(self, src, refs, raw, ranges, dst_bytes, count=None, max_count=None, nranges=None, max_ranges=None):
        import torch
        self.src, self.dst_bytes = src, dst_bytes
        self.max_count = len(refs) if max_count is None else max_count
        self.max_ranges = len(ranges) if max_ranges is None else max_ranges
        self.d_ref, self.d_raw = _dev_u64(list(refs) + [0]), _dev_u64(raw)
        self.d_count = _dev_u64([len(refs) if count is None else count])
        self.d_off, self.d_len, self.d_to = (_dev_u64([r[i] for r in ranges] + [0]) for i in range(3))
        self.d_n = _dev_u64([len(ranges) if nranges is None else nranges])
        self.out = torch.full((GUARD + dst_bytes + GUARD,), FILL, dtype=torch.uint8, device="cuda")
        self.status = torch.full((len(ranges) + 2,), -1, dtype=torch.int32, device="cuda")

    def queue(self, cw, alg, stream):
        d_store, store_bytes, d_dir, dir_base, dir_entries = self.src
        cw.dev_read_ranges(alg, d_store, store_bytes, d_dir, dir_base, dir_entries, self.d_ref.data_ptr(), self.d_raw.data_ptr(),
                           self.d_count.data_ptr(), self.max_count, self.d_off.data_ptr(), self.d_len.data_ptr(), self.d_to.data_ptr(),
                           self.d_n.data_ptr(), self.max_ranges, self.out.data_ptr() + GUARD, self.dst_bytes, self.status.data_ptr(), stream)

    def result(self):
        return self.status.cpu().numpy(), self.out.cpu().numpy()


def read_call(cw, alg, src, refs, raw, ranges, dst_bytes, **kw):
    """One call into a canary-filled destination: (statuses with 2 extra entries, destination with its guards)."""
    import torch
    c = Call(src, refs, raw, ranges, dst_bytes, **kw)
    torch.cuda.synchronize()
    c.queue(cw, alg, _stream())
    torch.cuda.synchronize()
    return c.result()


def check_read(status, out, want, ranges, dst_bytes, loose=()):
    """`want` = the model's [(status, bytes or None)] of the ranges the call serves; `loose` = indices of ranges whose status is
    unspecified.  The statuses, every status-0 extent's bytes, and FILL everywhere else but in unspecified extents."""
    R = len(want)
    for k in range(R):
        if k not in loose:
            assert int(status[k]) == want[k][0], ("range", k, ranges[k], "status", int(status[k]), "model", want[k][0])
    assert (status[R:] == -1).all(), "statuses behind the count were written"
    image, out = np.full(GUARD + dst_bytes + GUARD, FILL, np.uint8), out.copy()
    for k, (s, piece) in enumerate(want):
        _, l, to = ranges[k]
        if l == 0:
            continue
        if k in loose or s in (1, 2):
            out[GUARD + to:GUARD + to + l] = FILL
        elif s == 0:
            image[GUARD + to:GUARD + to + l] = np.frombuffer(piece, np.uint8)
    diff = np.nonzero(out != image)[0]
    assert len(diff) == 0, ("destination differs at", int(diff[0]) - GUARD, len(diff))


def src_of(st: Store):
    return st.d_store, st.store_bytes, st.d_dir, st.dir_base, st.dir_entries


def read_store(cw, O, alg, st: Store, refs, raw, ranges, dst_bytes, n=None, R=None, **kw):
    """A call on a Store and the model's answer from the Store's image; returns (model's answer, statuses, destination)."""
    status, out = read_call(cw, alg, src_of(st), refs, raw, ranges, dst_bytes, **kw)
    n, R = len(refs) if n is None else n, len(ranges) if R is None else R
    want = RD.read(st.x_store, st.store_bytes, st.x_dir, st.dir_base, refs[:n], raw[:n + 1], ranges[:R], dst_bytes, _decode(O, alg))
    check_read(status, out, want, ranges, dst_bytes)
    return want, status, out[GUARD:GUARD + dst_bytes]


@pytest.fixture(scope="module")
def window(cw, O):
    """Test 1's store per codec, built once: (data, cuts, Store, refs)."""
    made = {}

    def get(alg):
        if alg not in made:
            data = window_input()
            cuts = CM.chunk(data, P256)
            made[alg] = (data, cuts) + build(cw, O, alg, data, cuts, dir_base=3)
        return made[alg]
    return get


def forms(st: Store, refs):
    raw = [j for j, r in enumerate(refs) if st.x_dir[r - st.dir_base]["raw"] & RM.RAW]
    return raw, [j for j in range(len(refs)) if j not in set(raw)]


# ---- 1. window edges ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alg", ALGS)
def test_window_edges_around_every_cut(cw, O, window, alg):
    data, cuts, st, refs = window(alg)
    raws, comp = forms(st, refs)
    assert len(cuts) - 1 >= 40 and len(raws) >= 10 and len(comp) >= 10    # every chunk is touched: a range starts at every cut
    ranges, dst_bytes = packed(window_ranges(cuts))
    assert 2 * len(ranges) > 16384                                        # the edge lanes go round more than once
    want, status, out = read_store(cw, O, alg, st, refs, cuts, ranges, dst_bytes)
    assert (status[:len(ranges)] == 0).all()
    assert all(piece == data[a:a + l] for (a, l, _), (_, piece) in zip(ranges, want))


# ---- 2. alignment ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", ["compressed-compressed", "raw-compressed"])
@pytest.mark.parametrize("alg", ALGS)
def test_every_source_and_destination_alignment(cw, O, window, alg, pair):
    data, cuts, st, refs = window(alg)
    raws, comp = forms(st, refs)
    lens = np.diff(cuts)
    left = comp if pair == "compressed-compressed" else raws
    j = next(j for j in range(len(refs) - 1) if j in left and j + 1 in comp and lens[j] >= 58 and lens[j + 1] >= 58)
    c = cuts[j + 1]
    # 100 bytes across the cut from 16 consecutive starts (every d_range_off mod 16), each to every d_range_dst mod 16
    ranges = [(c - 42 - i, 100, 128 * (16 * i + d) + d) for i in range(16) for d in range(16)]
    assert {a % 16 for a, _, _ in ranges} == set(range(16)) == {to % 16 for _, _, to in ranges}
    want, status, out = read_store(cw, O, alg, st, refs, cuts, ranges, 128 * 256 + 16)
    assert (status[:256] == 0).all() and all(piece == data[a:a + 100] for (a, _, _), (_, piece) in zip(ranges, want))


# ---- 3. largest chunks ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alg", ALGS)
def test_chunks_of_65536_bytes(cw, O, alg):
    data, cuts = largest_input()
    st, refs = build(cw, O, alg, data, cuts)
    assert forms(st, refs) == ([1], [0, 2])
    n = len(data)
    ranges, dst_bytes = packed([(0, 1), (65535, 1), (1, 65535), (65535, 2), (0, 131072), (131071, 2), (131073, 65535), (131072, 65535),
                                (n - 1, 1), (1, n - 2), (0, n)], gap=3)
    want, status, out = read_store(cw, O, alg, st, refs, cuts, ranges, dst_bytes)
    assert (status[:len(ranges)] == 0).all() and all(piece == data[a:a + l] for (a, l, _), (_, piece) in zip(ranges, want))


# ---- 4. whole stream and tiling ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alg", ALGS)
def test_whole_stream_and_shuffled_tiles(cw, O, alg):
    rng = np.random.default_rng(41)
    data = mixed_input()
    n = len(data)
    with cw.DedupeIndex("skein512", 1024) as idx:
        cs = cw.ChunkStore(idx, alg, cw.CdcParams.default(1024), n + 4096, 1024, dir_base=50)
        m = RM.Model(O, alg, cs.store_bytes, 1024, dir_base=50)
        recipe, _ = ingest_both(cs, m, data, P1K)
        src = (cs.d_store.data_ptr(), cs.store_bytes, cs.d_dir.data_ptr(), 50, 1024)
        refs, cuts = recipe.refs.tolist(), recipe.offsets.tolist()
        # one range over the whole stream = the restore's output
        status, out = read_call(cw, alg, src, refs, cuts, [(0, n, 0)], n)
        _, restored = restore_call(cw, alg, *src, refs, cuts, n)
        assert status.tolist() == [0, -1, -1] and (out == restored).all() and out[GUARD:-GUARD].tobytes() == data
        # shuffled 4096-byte tiles, the last one shorter, to shuffled places
        tiles = [(a, min(4096, n - a)) for a in range(0, n, 4096)]
        assert tiles[-1][1] < 4096
        order, places = rng.permutation(len(tiles)), rng.permutation(len(tiles))
        ranges = [(tiles[t][0], tiles[t][1], int(places[t]) * 4096) for t in order]
        status, out = read_call(cw, alg, src, refs, cuts, ranges, 4096 * len(tiles))
        want = RD.read(m.blob, cs.store_bytes, m.directory, 50, refs, cuts, ranges, 4096 * len(tiles), m.decode())
        check_read(status, out, want, ranges, 4096 * len(tiles))
        got = out[GUARD:-GUARD]
        assert (status[:len(tiles)] == 0).all()
        assert b"".join(got[int(places[t]) * 4096:int(places[t]) * 4096 + tiles[t][1]].tobytes() for t in range(len(tiles))) == data
        # the same through the store object
        assert b"".join(cs.read_ranges(recipe, tiles)) == data
        shuffled = [tiles[t] for t in order]
        assert cs.read_ranges(recipe, shuffled) == [data[a:a + l] for a, l in shuffled]
        assert cs.read(recipe, 0, n) == data and cs.read(recipe, 12345, 1) == data[12345:12346] and cs.read(recipe, n, 0) == b""
        assert cs.read_ranges(recipe, []) == []
        with pytest.raises(cw.CwError, match=r"range 1 \(offset %d, length 2\) has status 3" % (n - 1)) as e:
            cs.read_ranges(recipe, [(0, 10), (n - 1, 2), (5, 5)])
        assert e.value.code == -2


# ---- 5. counts on the device ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alg", ALGS)
def test_counts_are_read_on_the_device(cw, O, window, alg):
    rng = np.random.default_rng(53)
    data, cuts, st, refs = window(alg)
    k, n_pos = len(refs), len(refs) - 5
    end = cuts[n_pos]
    some = [(int(a), int(min(l, end - a))) for a, l in zip(rng.integers(0, end, 20), rng.integers(1, 3000, 20))]
    # both lists go on behind their counts with huge values; the statuses behind R keep their canary
    ranges, dst_bytes = packed(some)
    wild = [(HUGE[i % 5], HUGE[(i + 1) % 5], HUGE[(i + 2) % 5]) for i in range(10)]
    tail_refs, tail_raw = [HUGE[i % 5] for i in range(5)], [HUGE[(i + 3) % 5] for i in range(5)]
    want, status, out = read_store(cw, O, alg, st, refs[:n_pos] + tail_refs, cuts[:n_pos + 1] + tail_raw, ranges + wild, dst_bytes, n=n_pos, R=20,
                                   count=n_pos, max_count=k, nranges=20, max_ranges=30)
    assert (status[:20] == 0).all() and (status[20:] == -1).all()
    assert all(piece == data[a:a + l] for (a, l, _), (_, piece) in zip(ranges, want))
    # the smaller of the two, both ways round; a range that reaches past raw_offsets[n] but not past raw_offsets[max_count] is refused
    ranges, dst_bytes = packed(some + [(end - 10, 20), (end, 1), (end - 10, 10)])
    want, status, out = read_store(cw, O, alg, st, refs, cuts, ranges, dst_bytes, n=n_pos, R=23, count=n_pos, max_count=k, nranges=10 ** 12,
                                   max_ranges=23)
    assert status[:23].tolist() == [0] * 20 + [3, 3, 0]
    want, status, out = read_store(cw, O, alg, st, refs, cuts, ranges, dst_bytes, n=n_pos, R=21, count=10 ** 12, max_count=n_pos, nranges=21,
                                   max_ranges=23)
    assert status.tolist() == [0] * 20 + [3] + [-1] * 4
    want, status, out = read_store(cw, O, alg, st, refs, cuts, ranges, dst_bytes, R=0, nranges=0)
    assert (status == -1).all() and (out == FILL).all()


# ---- 6. refusals and verdicts -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alg", ALGS)
def test_refused_ranges_write_nothing(cw, O, window, alg):
    data, cuts, st, refs = window(alg)
    n = len(data)
    raw = [1000 + c for c in cuts]       # the stream's coordinates need not start at 0
    dst_bytes = 5000
    ranges = [(999, 10, 0), (0, 1, 0), (2 ** 64 - 5, 10, 0), (1000 + n - 3, 4, 0), (1000 + n, 1, 0), (1000, 10, dst_bytes - 9),
              (1000, 10, 2 ** 64 - 5), (1000, 10, dst_bytes), (1000, n, 0),
              (0, 0, 0), (2 ** 64 - 1, 0, 2 ** 64 - 1), (5, 0, dst_bytes + 100),            # empty: never refused
              (1000, 10, 100), (1000 + n - 3, 3, 200), (1000 + 777, 10, dst_bytes - 10)]    # served beside the refused ones
    want, status, out = read_store(cw, O, alg, st, refs, raw, ranges, dst_bytes)
    assert status[:len(ranges)].tolist() == [3] * 9 + [0] * 6
    assert out[100:110].tobytes() == data[:10] and out[200:203].tobytes() == data[-3:] and out[-10:].tobytes() == data[777:787]
    assert np.count_nonzero(out != FILL) <= 23
    # no recipe: every range with a byte is refused
    ranges = [(1000, 1, 0), (0, 1, 0), (1000, 0, 0)]
    want, status, out = read_store(cw, O, alg, st, refs, raw, ranges, dst_bytes, n=0, count=0)
    assert status[:3].tolist() == [3, 3, 0] and (out == FILL).all()


def _around(cuts, j):
    """Ranges that touch position j (0 < j < k - 2) and ranges beside it."""
    near = [(cuts[j], 1), (cuts[j + 1] - 1, 1), (cuts[j] - 1, 2), (cuts[j + 1] - 1, 2), (cuts[j], cuts[j + 1] - cuts[j]),
            (cuts[j - 1], cuts[j + 2] - cuts[j - 1]), (cuts[j] + 1, cuts[j + 1] - cuts[j] - 2)]
    beside = [(cuts[j] - 1, 1), (cuts[j + 1], 1), (cuts[j - 1], cuts[j] - cuts[j - 1]), (cuts[j + 1], cuts[j + 2] - cuts[j + 1]),
              (cuts[j - 1] + 1, cuts[j] - cuts[j - 1] - 1), (cuts[j + 1], cuts[j + 2] - cuts[j + 1] - 1)]
    return near, beside


@pytest.mark.parametrize("alg", ALGS)
def test_damaged_entries_and_stored_bytes_get_the_models_statuses(cw, O, window, alg):
    import torch
    rng = np.random.default_rng(67)
    data, cuts, st, refs = window(alg)
    n, k = len(data), len(refs)
    raws, comp = forms(st, refs)
    inner = lambda js: [j for j in js if 2 <= j < k - 3]  # noqa: E731
    c, w = inner(comp), inner(raws)
    # (a) a CW_DEDUPE_MISS ref, a zeroed entry, an entry of another length (a compressed and a raw one), pos + stored past the store
    picks = [c[1], c[len(c) // 2], c[-2], w[1], w[-2]]
    assert len(set(picks)) == 5 and min(abs(a - b) for a in picks for b in picks if a != b) >= 3   # no range below touches two of them
    bad, refs2 = st.x_dir.copy(), list(refs)
    refs2[picks[0]] = RM.MISS
    bad[refs[picks[1]] - st.dir_base] = (0, 0, 0)
    bad["raw"][refs[picks[2]] - st.dir_base] += 1
    bad["raw"][refs[picks[3]] - st.dir_base] -= 1
    bad["pos"][refs[picks[4]] - st.dir_base] = st.store_bytes - int(bad["stored"][refs[picks[4]] - st.dir_base]) + 1
    near, beside = [], []
    for j in picks:
        a, b = _around(cuts, j)
        near, beside = near + a, beside + b
    others = [(int(a), int(min(l, n - a))) for a, l in zip(rng.integers(0, n, 60), rng.integers(1, 1500, 60))]
    ranges, dst_bytes = packed(near + beside + others, gap=1)
    d_dir = torch.from_numpy(bad.view(np.int64).copy()).cuda()
    status, out = read_call(cw, alg, (st.d_store, st.store_bytes, d_dir.data_ptr(), st.dir_base, st.dir_entries), refs2, cuts, ranges, dst_bytes)
    want = RD.read(st.x_store, st.store_bytes, bad, st.dir_base, refs2, cuts, ranges, dst_bytes, _decode(O, alg))
    check_read(status, out, want, ranges, dst_bytes)
    got = [s for s, _ in want]
    assert got[:len(near)] == [2] * len(near) and got[len(near):len(near) + len(beside)] == [0] * len(beside)
    assert all(piece == data[a:a + l] for (a, l, _), (s, piece) in zip(ranges, want) if s == 0) and got.count(0) > len(beside) + 20

    # (b) damaged stored bytes of compressed chunks, behind the store's bytes, one entry each: status 1 for every range that touches
    # such a chunk -- its first byte alone too, which is decoded before the decoder can meet the damage -- and for no other
    blob, bad = bytearray(st.x_store[:st.x_used].tobytes()), st.x_dir.copy()
    picks = [c[2], c[len(c) // 2 + 3], c[-3]]
    assert min(abs(a - b) for a in picks for b in picks if a != b) >= 3
    for j in picks:
        pos, stored, word = (int(v) for v in bad[refs[j] - st.dir_base])
        d = damaged_stream(alg, bytes(blob[pos:pos + stored]), word & RM.LEN_MASK, _decode(O, alg), rng)
        bad[refs[j] - st.dir_base] = (len(blob), len(d), word)
        blob += d
    near, beside = [], []
    for j in picks:
        a, b = _around(cuts, j)
        near, beside = near + a, beside + b
    ranges, dst_bytes = packed(near + beside + others, gap=1)
    d_store = torch.from_numpy(np.frombuffer(bytes(blob), np.uint8).copy()).cuda()     # the store ends with its last stream
    d_dir = torch.from_numpy(bad.view(np.int64).copy()).cuda()
    status, out = read_call(cw, alg, (d_store.data_ptr(), len(blob), d_dir.data_ptr(), st.dir_base, st.dir_entries), refs, cuts, ranges, dst_bytes)
    want = RD.read(blob, len(blob), bad, st.dir_base, refs, cuts, ranges, dst_bytes, _decode(O, alg))
    check_read(status, out, want, ranges, dst_bytes)
    got = [s for s, _ in want]
    assert got[:len(near)] == [1] * len(near) and got[len(near):len(near) + len(beside)] == [0] * len(beside) and 2 not in got
    assert all(piece == data[a:a + l] for (a, l, _), (s, piece) in zip(ranges, want) if s == 0)


@pytest.mark.parametrize("alg", ALGS)
def test_a_decreasing_pair_in_the_recipe(cw, O, window, alg):
    """Out of contract: which positions the ranges at the pair touch is unspecified, the canaries are not.  A range whose bytes all
    lie below the changed offset's new value, or not below the next offset, meets the comparisons of a sound list."""
    data, cuts, st, refs = window(alg)
    k, n = len(refs), len(data)
    j = k // 2
    raw = list(cuts)
    raw[j + 1] = raw[j] - 5        # position j decreases, position j + 1 is longer than its entry
    at = [(cuts[j] - 20, 40), (cuts[j], 1), (cuts[j + 1], 1), (cuts[j + 1] - 3, 10), (cuts[j - 1], cuts[j + 3] - cuts[j - 1]), (0, n),
          (cuts[j] - 5, 1), (cuts[j + 2] - 1, 1)]
    away = [(0, 100), (cuts[j - 2], cuts[j] - 5 - cuts[j - 2]), (cuts[j] - 6, 1), (cuts[j + 2], 1), (cuts[j + 2], cuts[j + 5] - cuts[j + 2]),
            (cuts[j + 2] + 1, 300), (cuts[3] - 1, cuts[6] - cuts[3] + 2), (n - 50, 50)]
    ranges, dst_bytes = packed(at + away, gap=2)
    status, out = read_call(cw, alg, src_of(st), refs, raw, ranges, dst_bytes)
    want = RD.read(st.x_store, st.store_bytes, st.x_dir, st.dir_base, refs, cuts, ranges, dst_bytes, _decode(O, alg))   # the sound list's answers
    check_read(status, out, want, ranges, dst_bytes, loose=set(range(len(at))))
    assert all(s == 0 and piece == data[a:a + l] for (a, l, _), (s, piece) in zip(ranges[len(at):], want[len(at):]))


# ---- 7. deduplicated and compacted stores -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alg", ALGS)
def test_ranges_in_chunks_another_ingest_stored(cw, O, alg, tmp_path):
    from conftest import corpus_file
    rng = np.random.default_rng(71)
    a = corpus_file("lcet10.txt")[:150_000]
    b = bytearray(a)
    b[20_000:20_000] = b"an insertion of some length"
    del b[70_000:70_300]
    b[110_000:110_010] = b"OVERWRITE!"
    b = bytes(b)
    with cw.DedupeIndex("skein512", 1024) as idx:
        cs = cw.ChunkStore(idx, alg, cw.CdcParams.default(1024), len(a) + 65536, 1024)
        m = RM.Model(O, alg, cs.store_bytes, 1024)
        ra, new_a = ingest_both(cs, m, a, P1K)
        rb, new_b = ingest_both(cs, m, b, P1K)
        k_a, cuts = len(ra.refs), rb.offsets.tolist()
        old = [j for j, r in enumerate(rb.refs.tolist()) if r < k_a]
        assert len(old) > len(rb.refs) // 2 and 0 < len(new_b) < 30
        # inside chunks of the first ingest, across runs of them, across the new chunks, and anywhere
        ranges = [(cuts[j] + 1, cuts[j + 1] - cuts[j] - 2) for j in old[::3] if cuts[j + 1] - cuts[j] > 2] + [(cuts[j], 1) for j in old[1::3]]
        ranges += [(cuts[j], cuts[min(j + 4, len(cuts) - 1)] - cuts[j]) for j in old[2::9]]
        ranges += [(max(cuts[i] - 100, 0), min(cuts[i + 1] + 100, len(b)) - max(cuts[i] - 100, 0)) for i in new_b]
        ranges += [(int(x), int(min(l, len(b) - x))) for x, l in zip(rng.integers(0, len(b), 50), rng.integers(1, 20000, 50))]
        expect = [b[x:x + l] for x, l in ranges]
        assert cs.read_ranges(rb, ranges) == expect
        assert cs.read(ra, 19_990, 100) == a[19_990:20_090]
        cs.compact(keep=[rb])
        assert cs.read_ranges(rb, ranges) == expect
        with pytest.raises(cw.CwError, match="status 2"):       # the first stream's own chunks are gone
            cs.read_ranges(ra, [(0, len(a))])
        path = str(tmp_path / "store.npz")
        cs.save(path)
    cs2 = cw.ChunkStore.load(path)
    try:
        assert cs2.read_ranges(rb, ranges) == expect and cs2.read(rb, 0, len(b)) == b
    finally:
        cs2.index.close()


# ---- 8. two host threads on one stream ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alg", ALGS)
def test_two_threads_on_one_stream_read_exactly(cw, O, window, alg):
    """The launch lock of the stream's scratch keeps one call's plan and decode buffers together: both threads' calls share them, and
    the two threads' calls need scratch of different sizes."""
    import torch
    rng = np.random.default_rng(89)
    data, cuts, st, refs = window(alg)
    n, calls, stream = len(data), 5, _stream()
    sets = [window_ranges(cuts)[::7], [(int(a), int(min(l, n - a))) for a, l in zip(rng.integers(0, n, 150), rng.integers(1, 4000, 150))]]
    work_of = []
    for t in range(2):
        ranges, dst_bytes = packed(sets[t])
        work_of.append((ranges, dst_bytes, [Call(src_of(st), refs, cuts, ranges, dst_bytes) for _ in range(calls)]))
    torch.cuda.synchronize()
    gate = threading.Barrier(2)

    def work(t):
        cw.init(0)
        gate.wait()
        for c in work_of[t][2]:
            c.queue(cw, alg, stream)

    threads = [threading.Thread(target=work, args=(t,)) for t in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    torch.cuda.synchronize()
    for ranges, dst_bytes, made in work_of:
        want = RD.read(st.x_store, st.store_bytes, st.x_dir, st.dir_base, refs, cuts, ranges, dst_bytes, _decode(O, alg))
        assert all(s == 0 and piece == data[a:a + l] for (a, l, _), (s, piece) in zip(ranges, want))
        for c in made:
            check_read(*c.result(), want, ranges, dst_bytes)
