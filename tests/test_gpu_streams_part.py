"""cw_dev_cdc_streams_part on the GPU against tests/streams_ingest_model.py: with final = 1 every output is cw_dev_cdc_streams's, and
with final = 0 the cuts, the chunk count and the per-stream index of every streams_model case, truncated at each stream end, one byte
either side of it, one byte before the end and at two points inside the last max_size, are the model's exactly -- with segments of one
max_size and of the default size, from an aligned source and from one offset by 5, with every output poisoned behind its valid part."""
import numpy as np
import pytest

import cdc_model as CM
import streams_ingest_model as XM
import streams_model as SM

pytestmark = pytest.mark.gpu
POISON = 0xABABABABABABABAB
PAD = 8
SEGS = sorted(SM.SEGMENTS)
MAX = SM.MAX


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


class Source:
    """A buffer on the device, `shift` bytes into an allocation: its prefixes are chunked in place."""

    def __init__(self, data: bytes, shift: int):
        import torch
        self.n = len(data)
        self.buf = torch.zeros(self.n + shift + 16, dtype=torch.uint8, device="cuda")
        if self.n:
            self.buf[shift:shift + self.n] = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda()
        self.ptr = self.buf.data_ptr() + shift


def dev_part(cw, src: Source, n: int, ends, final: bool, p: dict, part=True):
    """cw_dev_cdc_streams_part (or, part = False, cw_dev_cdc_streams) over the first n bytes: (offsets, K, first, result, poison intact)."""
    import torch
    nf = len(ends)
    d_ends = torch.from_numpy(np.asarray(list(ends) + [0], np.uint64).view(np.int64)).cuda()
    cp = _params(cw, p)
    cap = cp.max_offsets_streams(n, nf)
    offs, first, k, result = _poison(cap + PAD), _poison(nf + 1 + PAD), _poison(1 + PAD), _poison(1 + PAD)
    torch.cuda.synchronize()
    if part:
        cw.dev_cdc_streams_part(cp, src.ptr, n, d_ends.data_ptr(), nf, final, offs.data_ptr(), cap, k.data_ptr(), first.data_ptr(),
                                result.data_ptr(), _stream())
    else:
        cw.dev_cdc_streams(cp, src.ptr, n, d_ends.data_ptr(), nf, offs.data_ptr(), cap, k.data_ptr(), first.data_ptr(), result.data_ptr(), _stream())
    torch.cuda.synchronize()
    offs, first, k, result = _u64(offs), _u64(first), _u64(k), _u64(result)
    kk = int(k[0])
    assert kk < cap
    intact = bool((offs[kk + 1:] == POISON).all() and (first[nf + 1:] == POISON).all() and (k[1:] == POISON).all() and (result[1:] == POISON).all())
    return offs[:kk + 1].tolist(), kk, first[:nf + 1].tolist(), int(result[0]), intact


def points(ends, total):
    """Where a case is truncated: its stream ends (the first three and the last two distinct ones when there are many), one byte either
    side of each, one byte before the end of the buffer, and two points inside the last max_size."""
    distinct = sorted({e for e in ends if 0 < e})
    near = distinct if len(distinct) <= 4 else distinct[:2] + distinct[-2:]
    pts = {e + d for e in near for d in (-1, 0, 1)} | {total - 1, total - MAX // 2, total - MAX + 1}
    return sorted(n for n in pts if 0 < n <= total)


def clipped(ends, n, closed: bool):
    """The ends of the first n bytes.  A stream that ends below n is complete; the open stream runs from the last such end to n.  closed:
    a stream that ends AT n is complete too, and the open stream behind it is empty."""
    return [e for e in ends if e < n or (closed and e == n)] + [n]


@pytest.mark.parametrize("seg", SEGS)
@pytest.mark.parametrize("name", sorted(SM.CASES))
def test_final_1_is_dev_cdc_streams(cw, name, seg):
    S = SM.SEGMENTS[seg]
    streams, p, offsets, first = SM.case(name, S)
    src = Source(b"".join(streams), 5)
    ends = SM.ends_of(streams)
    with cw.tuned(**({"CW_CDC_SEGMENT": S} if seg == "one_max" else {})):
        got = dev_part(cw, src, src.n, ends, True, p)
        want = dev_part(cw, src, src.n, ends, True, p, part=False)
    assert got == want == (offsets, len(offsets) - 1, first, 0, True)


@pytest.mark.parametrize("shift", [0, 5])
@pytest.mark.parametrize("seg", SEGS)
@pytest.mark.parametrize("name", sorted(SM.CASES))
def test_final_0_cuts_count_and_stream_index_equal_the_model(cw, name, seg, shift):
    S = SM.SEGMENTS[seg]
    streams, p, offsets, first = SM.case(name, S)
    data, ends = b"".join(streams), SM.ends_of(streams)
    src = Source(data, shift)
    runs = 0
    with cw.tuned(**({"CW_CDC_SEGMENT": S} if seg == "one_max" else {})):
        for n in points(ends, len(data)):
            for closed in ((False, True) if n in ends else (False,)):
                e = clipped(ends, n, closed)
                want, want_first = XM.chunk_part(data[:n], e, False, p)
                got, k, got_first, result, intact = dev_part(cw, src, n, e, False, p)
                assert result == 0 and intact, (n, closed)
                assert k == len(want) - 1 and got == want, (n, closed, next((i for i, (x, y) in enumerate(zip(got, want)) if x != y), None))
                assert got_first == want_first, (n, closed)
                s = e[-2] if len(e) > 1 else 0
                assert s <= got[-1] <= n and got[-1] + p["max"] > n and got_first[-1] == k
                runs += 1
        # no byte at all: an open stream of nothing, alone and behind empty streams
        for e in ([0], [0, 0, 0]):
            assert dev_part(cw, src, 0, e, False, p) == ([0], 0, [0] * (len(e) + 1), 0, True)
    print(name, seg, shift, "points", runs)
    assert runs >= (3 if data else 0)


@pytest.mark.parametrize("seg", SEGS)
def test_one_open_stream_equals_dev_cdc_final_0(cw, seg):
    import torch
    S = SM.SEGMENTS[seg]
    streams, p, _, _ = SM.case("one_text_300k", S)
    data = streams[0]
    src = Source(data, 0)
    cp = _params(cw, p)
    with cw.tuned(**({"CW_CDC_SEGMENT": S} if seg == "one_max" else {})):
        for n in (len(data), 123457, MAX - 1):
            cap = cp.max_offsets(n)
            offs, k = _poison(cap), _poison(1)
            torch.cuda.synchronize()
            cw.dev_cdc(cp, src.ptr, n, False, offs.data_ptr(), cap, k.data_ptr(), _stream())
            torch.cuda.synchronize()
            kk = int(_u64(k)[0])
            one = _u64(offs)[:kk + 1].tolist()
            assert dev_part(cw, src, n, [n], False, p) == (one, kk, [0, kk], 0, True) and one == CM.chunk(data[:n], p, final=False)


@pytest.mark.parametrize("seg", SEGS)
@pytest.mark.parametrize("kind", ["decreasing", "decreasing_at_the_end", "last_is_not_nbytes", "last_is_beyond", "garbage"])
def test_refused_ends_under_final_0_give_the_empty_result(cw, kind, seg):
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
    src = Source(b"".join(streams), 5)
    with cw.tuned(**({"CW_CDC_SEGMENT": S} if seg == "one_max" else {})):
        assert dev_part(cw, src, n, ends, False, p) == ([0], 0, [0] * (nf + 1), 1, True)
