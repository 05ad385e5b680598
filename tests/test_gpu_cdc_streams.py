"""Many streams chunked in one call on the GPU (cw_dev_cdc_streams, cw_dev_cdc_streams_dedupe_compress, ChunkStore.ingest_many) against
tests/streams_model.py: the cuts, the chunk count and the per-stream index are the model's exactly, for every case of its table, with
segments of one max_size and of the default size, from an aligned source and from one offset by 5, with every output poisoned behind
its valid part.  That each case reaches its edge is established on the CPU (tests/test_cdc_streams_abi.py)."""
import numpy as np
import pytest

import cdc_model as CM
import streams_model as SM
from conftest import corpus_file

pytestmark = pytest.mark.gpu
BAD_ARG = -2
POISON = 0xABABABABABABABAB
PAD = 8
SEGS = sorted(SM.SEGMENTS)


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


def _params(cw, p: dict):
    return cw.CdcParams(p["min"], p["avg"], p["max"], p["mask_s"], p["mask_l"], p.get("gear"))


def _poison(n):
    import torch
    return torch.full((n,), POISON - (1 << 64), dtype=torch.int64, device="cuda")


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


def dev_streams(cw, streams, p: dict, shift=0, seg=None, ends=None):
    """cw_dev_cdc_streams over the concatenation placed `shift` bytes into a device buffer: (offsets, K, first, result, poison intact)."""
    import torch
    data = b"".join(bytes(s) for s in streams)
    n, nf = len(data), len(streams)
    if ends is None:
        ends = SM.ends_of(streams)
    buf = torch.zeros(n + shift + 16, dtype=torch.uint8, device="cuda")
    if n:
        buf[shift:shift + n] = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda()
    d_ends = torch.from_numpy(np.asarray(list(ends) + [0], np.uint64).view(np.int64)).cuda()
    cp = _params(cw, p)
    cap = cp.max_offsets_streams(n, nf)
    offs, first, k, result = _poison(cap + PAD), _poison(nf + 1 + PAD), _poison(1 + PAD), _poison(1 + PAD)
    torch.cuda.synchronize()
    if seg:
        cw.tune_set("CW_CDC_SEGMENT", str(seg))
    try:
        cw.dev_cdc_streams(cp, buf.data_ptr() + shift, n, d_ends.data_ptr(), nf, offs.data_ptr(), cap, k.data_ptr(), first.data_ptr(),
                           result.data_ptr(), _stream())
        torch.cuda.synchronize()
    finally:
        if seg:
            cw.tune_set("CW_CDC_SEGMENT", None)
    offs, first, k, result = _u64(offs), _u64(first), _u64(k), _u64(result)
    kk = int(k[0])
    assert kk < cap
    intact = bool((offs[kk + 1:] == POISON).all() and (first[nf + 1:] == POISON).all() and (k[1:] == POISON).all() and (result[1:] == POISON).all())
    return offs[:kk + 1].tolist(), kk, first[:nf + 1].tolist(), int(result[0]), intact


@pytest.mark.parametrize("shift", [0, 5])
@pytest.mark.parametrize("seg", SEGS)
@pytest.mark.parametrize("name", sorted(SM.CASES))
def test_cuts_count_and_stream_index_equal_the_model(cw, name, seg, shift):
    S = SM.SEGMENTS[seg]
    streams, p, offsets, first = SM.case(name, S)
    got, k, got_first, result, intact = dev_streams(cw, streams, p, shift=shift, seg=S if seg == "one_max" else None)
    print(name, seg, shift, "chunks", k, "model", len(offsets) - 1, "result", result)
    assert result == 0 and intact
    assert k == len(offsets) - 1
    assert got == offsets, next((i for i, (x, y) in enumerate(zip(got, offsets)) if x != y), None)
    assert got_first == first, next((i for i, (x, y) in enumerate(zip(got_first, first)) if x != y), None)


@pytest.mark.parametrize("seg", SEGS)
def test_one_stream_equals_dev_cdc(cw, seg):
    import torch
    S = SM.SEGMENTS[seg]
    knob = S if seg == "one_max" else None
    streams, p, offsets, first = SM.case("one_text_300k", S)
    data = streams[0]
    cp = _params(cw, p)
    src = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda()
    cap = cp.max_offsets(len(data))
    offs, k = _poison(cap), _poison(1)
    torch.cuda.synchronize()
    if knob:
        cw.tune_set("CW_CDC_SEGMENT", str(knob))
    try:
        cw.dev_cdc(cp, src.data_ptr(), len(data), True, offs.data_ptr(), cap, k.data_ptr(), _stream())
        torch.cuda.synchronize()
    finally:
        cw.tune_set("CW_CDC_SEGMENT", None)
    kk = int(_u64(k)[0])
    one = _u64(offs)[:kk + 1].tolist()
    got, k2, got_first, result, intact = dev_streams(cw, streams, p, seg=knob)
    assert (got, k2, got_first, result, intact) == (one, kk, [0, kk], 0, True) and one == offsets


@pytest.mark.parametrize("seg", SEGS)
def test_a_block_in_two_streams_gets_the_same_cuts(cw, seg):
    S = SM.SEGMENTS[seg]
    streams, p, offsets, first = SM.case("dup_block", S)
    got, k, gf, result, intact = dev_streams(cw, streams, p, shift=5, seg=S if seg == "one_max" else None)
    assert result == 0 and intact
    per = SM.per_stream_cuts(got, gf)
    assert per[1] == per[4] == CM.chunk(streams[1], p) and len(per[1]) > 10


@pytest.mark.parametrize("seg", SEGS)
@pytest.mark.parametrize("kind", ["decreasing", "decreasing_at_the_end", "last_is_not_nbytes", "last_is_beyond", "garbage"])
def test_refused_ends_give_verdict_1_and_write_nothing_else(cw, kind, seg):
    S = SM.SEGMENTS[seg]
    streams, p, _, _ = SM.case("ladder", S)
    ends = SM.ends_of(streams)
    n, nf = ends[-1], len(ends)
    if kind == "decreasing":
        ends[5], ends[6] = ends[6], ends[5] - 1
    elif kind == "decreasing_at_the_end":
        ends[-2] = n + 1
    elif kind == "last_is_not_nbytes":
        ends[-3:] = [n - 1] * 3
    elif kind == "last_is_beyond":
        ends[-1] = n + (1 << 40)
    else:
        ends = [int(v) for v in np.random.default_rng(4).integers(0, 1 << 63, nf, dtype=np.uint64)]
    got, k, first, result, intact = dev_streams(cw, streams, p, shift=5, seg=S if seg == "one_max" else None, ends=ends)
    assert (result, k, got, first, intact) == (1, 0, [0], [0] * (nf + 1), True)


def test_empty_streams_only_and_their_verdict(cw):
    assert dev_streams(cw, [b"", b"", b""], SM.P1K) == ([0], 0, [0, 0, 0, 0], 0, True)
    assert dev_streams(cw, [b"", b"", b""], SM.P1K, ends=[0, 0, 1]) == ([0], 0, [0, 0, 0, 0], 1, True)
    assert dev_streams(cw, [], SM.P1K) == ([0], 0, [0], 0, True)


# ---- the fused call and the store ----------------------------------------------------------------------------------------------
def _mix():
    """About 40 corpus slices of 0 to 70,000 bytes, some repeated."""
    t = corpus_file("lcet10.txt") + corpus_file("alice29.txt") + corpus_file("kennedy.xls")[:200000]
    rng = np.random.default_rng(16)
    out = []
    for i in range(34):
        n = int(rng.integers(0, 70001)) if i % 7 else (0, 1, 70000, 255, 256)[i // 7]
        at = int(rng.integers(0, len(t) - n))
        out.append(t[at:at + n])
    out += [out[3], out[10], out[3], b"", out[20], out[2]]
    return out


INPUTS = {"dup_block": lambda: SM.dup_streams(), "mix": _mix}


def _fresh(cw, alg):
    idx = cw.DedupeIndex("skein512", 1 << 14)
    return idx, cw.ChunkStore(idx, alg, cw.CdcParams.default(1024), 4 << 20, 1 << 14, dir_base=3)


@pytest.mark.parametrize("which", sorted(INPUTS))
@pytest.mark.parametrize("alg", ["lz4", "lzf"])
def test_ingest_many_leaves_what_a_loop_of_ingest_leaves(cw, alg, which):
    datas = INPUTS[which]()
    ia, a = _fresh(cw, alg)
    ib, b = _fresh(cw, alg)
    with ia, ib:
        many = a.ingest_many(datas)
        loop = [b.ingest(d) for d in datas]
        assert len(many) == len(loop) == len(datas)
        for d, r, q in zip(datas, many, loop):
            assert r.refs.tolist() == q.refs.tolist() and r.offsets.tolist() == q.offsets.tolist() and r.nbytes == len(d)
            assert r.offsets.tolist() == CM.chunk(d, SM.P1K)
        used = a.used()
        assert used == b.used() > 0 and a.base == b.base and ia.count() == ib.count() > 0
        assert bytes(a.d_store[:used].cpu().numpy()) == bytes(b.d_store[:used].cpu().numpy())
        assert (a.d_dir.cpu().numpy() == b.d_dir.cpu().numpy()).all()
        if which == "dup_block":
            assert many[1].refs.tolist() == many[4].refs.tolist()
        for d, r in zip(datas, many):
            assert a.restore(r) == d
        j = max(range(len(datas)), key=lambda i: len(datas[i]))
        assert a.read(many[j], 1234, 20000) == datas[j][1234:21234]
        keep = many[::2]
        a.compact(keep)
        for d, r in zip(datas[::2], keep):
            assert a.restore(r) == d
        assert a.ingest_many([]) == [] and a.ingest_many([b""])[0].offsets.tolist() == [0]


@pytest.mark.parametrize("alg", ["lz4", "lzf"])
def test_ingest_many_raises_as_ingest_when_the_store_is_full(cw, alg):
    datas = _mix()[:12]
    with cw.DedupeIndex("skein512", 1 << 14) as idx:
        cs = cw.ChunkStore(idx, alg, cw.CdcParams.default(1024), 10000, 1 << 14)
        with pytest.raises(cw.CwError) as e:
            cs.ingest_many(datas)
        assert e.value.code == -5 and e.value.needed > 10000 and cs.used() == 0 and cs.base == 0
    with cw.DedupeIndex("skein512", 1 << 14) as idx:
        cs = cw.ChunkStore(idx, alg, cw.CdcParams.default(1024), 4 << 20, 8)
        with pytest.raises(cw.CwError) as e:
            cs.ingest_many(datas)
        assert e.value.code == -5 and cs.used() == 0 and cs.base == 0


def test_fused_call_refuses_bad_ends_with_nothing_inserted(cw):
    import torch
    datas = [corpus_file("alice29.txt")[:30000], corpus_file("alice29.txt")[30000:50000]]
    n, nf = 50000, 2
    cp = cw.CdcParams.default(1024)
    cap = cp.max_offsets_streams(n, nf)
    total = cw.chunk_slots_bytes("lz4", n, cap - 1)
    src = torch.from_numpy(np.frombuffer(b"".join(datas), np.uint8).copy()).cuda()
    d_ends = torch.from_numpy(np.array([30000, 49999], np.uint64).view(np.int64)).cuda()
    z = lambda k, dt: torch.zeros(k, dtype=dt, device="cuda")  # noqa: E731
    off, k_dev, dig, ref = _poison(cap), _poison(1), z(cap * 64, torch.uint8), _poison(cap)
    new_idx, n_new, slots, sizes = z(cap, torch.int32), _poison(1), z(total, torch.uint8), z(cap, torch.int32)
    first, result = _poison(nf + 1), _poison(1)
    torch.cuda.synchronize()
    with cw.DedupeIndex("skein512", 4096) as idx:
        with pytest.raises(cw.CwError) as e:
            idx.dev_cdc_streams_dedupe_compress(cp, "lz4", src.data_ptr(), n, d_ends.data_ptr(), nf, 0, off.data_ptr(), cap, k_dev.data_ptr(),
                                                first.data_ptr(), result.data_ptr(), dig.data_ptr(), ref.data_ptr(), new_idx.data_ptr(),
                                                n_new.data_ptr(), slots.data_ptr(), total, sizes.data_ptr(), _stream())
        torch.cuda.synchronize()
        assert e.value.code == BAD_ARG and e.value.nchunks == 0 and idx.count() == 0
        assert int(_u64(result)[0]) == 1 and int(_u64(k_dev)[0]) == 0 and _u64(first).tolist() == [0, 0, 0]
        assert (_u64(ref) == POISON).all() and (_u64(off)[1:] == POISON).all() and not sizes.cpu().numpy().any() and not slots.cpu().numpy().any()
