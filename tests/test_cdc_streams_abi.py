"""CPU-side checks of chunking many streams in one call (cw_dev_cdc_streams, cw_dev_cdc_streams_dedupe_compress, ChunkStore.ingest_many):
the symbols are declared, listed and exported, every refusal comes before the device, the calls fail loudly without one, the stream
form's kernels compile without scratch memory or spills, and the model's two statements of the semantics (tests/streams_model.py: every
stream alone, and one chain over the concatenation with local ends) agree.

The inputs of tests/test_gpu_cdc_streams.py are built by the model, and that each reaches its edge -- a segment with more cuts than
seg / min_size + 2, a progression cut short by a stream's end, ends at a segment's edge and beside it, empty streams, the length
ladder -- is established here from the model."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import cdc_model as CM
import streams_model as SM
from conftest import ROOT

LZ4, LZF = 0, 1
NO_DEVICE, BAD_ARG = -1, -2
NAMES = ("cw_dev_cdc_streams", "cw_dev_cdc_streams_dedupe_compress")
MIN, MAX = SM.MIN, SM.MAX
CASE_IDS = [(name, seg) for name in sorted(SM.CASES) for seg in sorted(SM.SEGMENTS)]


@pytest.fixture(scope="module")
def cwlib():
    import compute_war_amd as cw
    if not os.path.exists(cw.lib_path()):
        subprocess.run(["make", "-C", os.path.join(ROOT, "compute_war_amd", "csrc"), "-j8"], check=True, capture_output=True)
    return cw


# ---- the boundary ------------------------------------------------------------------------------------------------------------
def test_header_declares_and_binding_lists_the_symbols(cwlib):
    from compute_war_amd import _lib
    text_ = open(os.path.join(ROOT, "include", "cw_hashcompress.h")).read()
    declared = re.findall(r"\b(cw_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text_, flags=re.S))
    out = subprocess.run(["nm", "-D", "--defined-only", cwlib.lib_path()], capture_output=True, text=True, check=True).stdout
    exported = re.findall(r" T (cw_[a-z0-9_]+)", out)
    for name in NAMES:
        assert name in declared and name in _lib.ABI_SYMBOLS and name in exported, name
    assert hasattr(cwlib, "dev_cdc_streams") and hasattr(cwlib.DedupeIndex, "dev_cdc_streams_dedupe_compress")
    assert hasattr(cwlib.ChunkStore, "ingest_many") and hasattr(cwlib.CdcParams, "max_offsets_streams")
    assert cwlib.CdcParams.default(1024).max_offsets_streams(1000, 7) == 1000 // 256 + 7 + 1


NBYTES, NSTREAMS = 5000, 3


def _streams_args(cw, **over):
    """cw_dev_cdc_streams's arguments with made-up non-NULL device pointers: nothing dereferences them before the device is asked for."""
    p = cw.CdcParams(normal_size=1024)
    a = dict(p=C.byref(p), src=4096, nbytes=NBYTES, ends=8192, nstreams=NSTREAMS, offsets=12288, max_offsets=NBYTES // 256 + NSTREAMS + 1,
             k=16384, first=20480, result=24576, stream=None)
    a.update(over)
    return p, tuple(a[n] for n in ("p", "src", "nbytes", "ends", "nstreams", "offsets", "max_offsets", "k", "first", "result", "stream"))


def test_streams_refuses_bad_arguments_before_the_device(cwlib):
    import torch
    L = cwlib.lib()
    call = lambda **kw: L.cw_dev_cdc_streams(*_streams_args(cwlib, **kw)[1])  # noqa: E731
    for name in ("p", "src", "ends", "offsets", "k", "first", "result"):
        assert call(**{name: None}) == BAD_ARG, name
    for d in (1, 2, 4, 7):
        assert call(result=24576 + d) == BAD_ARG and b"8-byte aligned" in L.cw_last_error()
    assert call(nstreams=(1 << 32) - 255, max_offsets=1 << 33) == BAD_ARG and b"nstreams" in L.cw_last_error()
    assert call(max_offsets=NBYTES // 256 + NSTREAMS) == BAD_ARG and b"max_offsets" in L.cw_last_error()
    assert call(nstreams=0, ends=None) == BAD_ARG and b"nstreams is 0" in L.cw_last_error()
    # what cw_dev_cdc refuses
    for bad in (dict(reserved=1), dict(min_size=63), dict(min_size=2048), dict(max_size=512), dict(max_size=(1 << 24) + 1)):
        p, args = _streams_args(cwlib)
        for f, v in bad.items():
            setattr(p, f, v)
        assert L.cw_dev_cdc_streams(*args) == BAD_ARG, bad
    if not torch.cuda.is_available():
        # not refused: the exact bound, an empty buffer without a source, no stream at all, the largest stream count
        for kw in (dict(), dict(src=None, nbytes=0, max_offsets=NSTREAMS + 1), dict(src=None, nbytes=0, ends=None, nstreams=0, max_offsets=1),
                   dict(nstreams=(1 << 32) - 256, max_offsets=1 << 33)):
            assert call(**kw) == NO_DEVICE, kw


def _fused_args(cw, **over):
    p = cw.CdcParams(normal_size=1024)
    cap = NBYTES // 256 + NSTREAMS + 1
    k = C.c_size_t(7)
    a = dict(x=4096, p=C.byref(p), alg=LZ4, src=8192, nbytes=NBYTES, ends=12288, nstreams=NSTREAMS, base=0, offsets=16384, max_offsets=cap,
             k=20480, first=24576, result=28672, dig=32768, ref=36864, new_idx=40960, n_new=45056, dst=49152, dst_bytes=None, sizes=53248,
             nchunks=C.byref(k), stream=None)
    a.update(over)
    if a["dst_bytes"] is None:
        a["dst_bytes"] = cw.chunk_slots_bytes(a["alg"] if a["alg"] in (LZ4, LZF) else LZ4, a["nbytes"], a["max_offsets"] - 1)
    order = ("x", "p", "alg", "src", "nbytes", "ends", "nstreams", "base", "offsets", "max_offsets", "k", "first", "result", "dig", "ref", "new_idx",
             "n_new", "dst", "dst_bytes", "sizes", "nchunks", "stream")
    return (p, k), tuple(a[n] for n in order)


def test_fused_call_refuses_bad_arguments_before_the_device(cwlib):
    import torch
    L = cwlib.lib()

    def call(**kw):
        keep, args = _fused_args(cwlib, **kw)
        return L.cw_dev_cdc_streams_dedupe_compress(*args), keep[1].value
    for name in ("p", "src", "ends", "offsets", "k", "first", "result", "dig", "ref", "new_idx", "n_new", "dst", "sizes", "nchunks"):
        assert call(**{name: None})[0] == BAD_ARG, name
    assert call(result=28672 + 4)[0] == BAD_ARG and call(dig=32768 + 4)[0] == BAD_ARG
    assert call(alg=2)[0] == BAD_ARG and call(alg=-1)[0] == BAD_ARG
    assert call(max_offsets=NBYTES // 256 + NSTREAMS)[0] == BAD_ARG and b"max_offsets" in L.cw_last_error()
    full = cwlib.chunk_slots_bytes(LZ4, NBYTES, NBYTES // 256 + NSTREAMS)
    assert call(dst_bytes=full - 1)[0] == BAD_ARG and b"dst_bytes" in L.cw_last_error()
    assert call(nstreams=(1 << 32) - 255, max_offsets=1 << 33, dst_bytes=1 << 40)[0] == BAD_ARG
    assert call(nstreams=0, ends=None)[0] == BAD_ARG
    if not torch.cuda.is_available():
        for kw in (dict(), dict(alg=LZF), dict(src=None, nbytes=0, max_offsets=NSTREAMS + 1)):
            assert call(**kw) == (NO_DEVICE, 0), kw
        assert call(x=None)[0] == NO_DEVICE   # (as cw_dev_cdc_dedupe_compress: the index is looked at once there is a device)


def test_no_gpu_means_no_stream_chunking(cwlib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    p = cwlib.CdcParams.default(1024)
    with pytest.raises(cwlib.CwError) as e:
        cwlib.dev_cdc_streams(p, 4096, NBYTES, 8192, NSTREAMS, 12288, p.max_offsets_streams(NBYTES, NSTREAMS), 16384, 20480, 24576)
    assert e.value.code == NO_DEVICE


def _meta(asm):
    meta = asm[asm.index("amdhsa.kernels"):]
    out = {}
    for e in re.split(r"\n  - ", meta):
        m = re.search(r"\.name:\s+(\S+)", e)
        if m:
            out[m.group(1)] = e
    return out


def test_stream_kernels_have_no_private_segment_or_spills(tmp_path):
    out = str(tmp_path / "k.s")
    subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-S", "--cuda-device-only", "--offload-arch=gfx950",
                    os.path.join(ROOT, "compute_war_amd", "csrc", "cdc_streams_kernels.hip"), "-o", out], check=True, capture_output=True)
    meta = _meta(open(out).read())
    assert len(meta) == 8, sorted(meta)
    for kernel in ("cdc_spec_kernel", "cdc_merge_kernel", "cdc_fixup_kernel", "cdc_count_kernel", "cdc_write_kernel", "cdc_ends_check_kernel",
                   "cdc_streams_init_kernel", "cdc_stream_first_kernel"):
        assert sum(kernel in k for k in meta) == 1, kernel
    for name, e in meta.items():
        assert re.search(r"\.private_segment_fixed_size:\s+0\b", e), name
        assert re.search(r"\.vgpr_spill_count:\s+0\b", e), name
        assert re.search(r"\.sgpr_spill_count:\s+0\b", e), name
    makefile = open(os.path.join(ROOT, "compute_war_amd", "csrc", "Makefile")).read()
    assert "cdc_streams_kernels.hip" in re.search(r"^SRCS\s*:=(.*)$", makefile, flags=re.M).group(1)
    assert "cdc_resolve.h" in re.search(r"^HDRS\s*:=(.*)$", makefile, flags=re.M).group(1)


# ---- the model ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,seg", CASE_IDS)
def test_one_chain_with_local_ends_equals_every_stream_alone(name, seg):
    streams, p, offsets, first = SM.case(name, SM.SEGMENTS[seg])
    assert SM.chunk_chain(streams, p) == (offsets, first)
    n = sum(len(s) for s in streams)
    assert offsets[0] == 0 and offsets[-1] == n and all(a < b for a, b in zip(offsets, offsets[1:]))
    assert len(first) == len(streams) + 1 and first[-1] == len(offsets) - 1 <= n // p["min"] + len(streams)
    for s, cuts in zip(streams, SM.per_stream_cuts(offsets, first)):
        assert cuts == CM.chunk(s, p)


def test_model_on_small_streams_against_the_plain_loop():
    p = CM.params(64, 256, 1024, CM.top_bits(10), CM.top_bits(6))
    rng = np.random.default_rng(8)
    data = rng.integers(0, 256, 30000, dtype=np.uint8).tobytes() + bytes(5000) + b"ab" * 2000
    lengths = [0, 1, 63, 64, 65, 0, 0, 1023, 1024, 1025, 5000, 1, 1, 1, 7000, 0, 9000, 3000, 0]
    streams = SM.split(data, lengths)
    offsets, first = SM.chunk_streams(streams, p)
    assert SM.chunk_chain(streams, p) == (offsets, first)
    for s, cuts in zip(streams, SM.per_stream_cuts(offsets, first)):
        assert cuts == CM.chunk_serial(s, p)
    assert first[:3] == [0, 0, 1] and first[5] == first[6] == first[7] and first[-1] == first[-2] == len(offsets) - 1


def test_every_case_reaches_its_edge():
    for seg in SM.SEGMENTS.values():
        cap = seg // MIN + 2
        # a segment holding more cuts than the single-stream capacity
        streams, p, offsets, first = SM.case("one_byte_x3000", seg)
        assert len(streams) == 3000 and offsets == list(range(3001)) and first == list(range(3001))
        assert SM.max_cuts_in_a_segment(offsets, seg) == 3000 > cap
        # ends at a segment's edge and at edge - 1 and edge + 1
        streams, p, offsets, first = SM.case("segment_edges", seg)
        ends = SM.ends_of(streams)
        assert ends == [seg - 1, seg, 2 * seg, 3 * seg + 1, 4 * seg, 6 * seg] and set(ends) <= set(offsets)
        assert {e % seg for e in ends} == {seg - 1, 0, 1}
    S = SM.SEGMENTS["one_max"]
    # the ladder: empty streams first, last, doubled and between; every length
    streams, p, offsets, first = SM.case("ladder", S)
    lens = [len(s) for s in streams]
    assert lens[0] == 0 and lens[-2:] == [0, 0] and lens[2:4] == [0, 0] and [n for n in lens if n] == [MIN, MIN + 1, MAX, MAX + 1, 63, 64, 65]
    assert all(first[f] == first[f + 1] for f, n in enumerate(lens) if n == 0) and first[0] == 0 and first[-3:] == [len(offsets) - 1] * 3
    cuts = dict(zip(lens, SM.per_stream_cuts(offsets, first)))
    assert cuts[MIN] == [0, MIN] and cuts[63] == [0, 63] and cuts[64] == [0, 64] and cuts[65] == [0, 65] and len(cuts[MIN + 1]) in (2, 3)
    assert cuts[MAX + 1][-1] == MAX + 1 and len(cuts[MAX + 1]) >= 3
    # progressions cut short by a stream's end: the run goes on behind the end, the cuts do not keep its phase
    streams, p, offsets, first = SM.case("no_candidates", S)
    per = SM.per_stream_cuts(offsets, first)
    assert per[0] == [0, MAX, 2 * MAX, 3 * MAX, 3 * MAX + 5] and per[1] == [0, MAX] and per[2] == [0, MAX, 2 * MAX - 1]
    assert per[3] == [MAX * i for i in range(10)] + [9 * MAX + 100]
    whole = CM.chunk(b"".join(streams), p)
    assert 4 * MAX in whole and 4 * MAX not in offsets and len(set(c % MAX for c in offsets)) == 4
    streams, p, offsets, first = SM.case("all_candidates", S)
    per = SM.per_stream_cuts(offsets, first)
    # (with max_size left every chunk is min_size; the last max_size bytes of a stream are cut at min_size too, up to a remainder <= min_size)
    assert per[1] == [0, MIN] and per[3] == [0, 1] and per[0][:10] == [MIN * i for i in range(10)] and per[0][-1] == 10 * MIN + 3
    assert set(np.diff(per[4])[:-1].tolist()) == {MIN} and per[4][-1] == 40 * MIN + 100
    assert CM.chunk(b"".join(streams), p) != offsets
    streams, p, offsets, first = SM.case("zero_runs", S)
    per = SM.per_stream_cuts(offsets, first)
    assert per[1] == [0, 3] and per[2] == [0, MAX, 2 * MAX] and per[3] == [MAX * i for i in range(8)] + [7 * MAX + 1]
    run = [c for c in per[0] if c > 12345 + MAX]
    assert len(run) >= 5 and set(np.diff(run)[:-1].tolist()) == {MAX} and run[0] % MAX != 0   # entered at an odd phase
    assert len(set(c % MAX for c in offsets)) >= 4
    # one stream is cw_dev_cdc; nothing is nothing
    streams, p, offsets, first = SM.case("one_text_300k", S)
    assert offsets == CM.chunk(streams[0], p) and first == [0, len(offsets) - 1] and len(offsets) > 100
    assert SM.case("no_streams", S)[2:] == ([0], [0]) and SM.case("one_empty", S)[2:] == ([0], [0, 0])
    # the block that occurs twice gets the same cuts both times, among different neighbours at different phases
    streams, p, offsets, first = SM.case("dup_block", S)
    per = SM.per_stream_cuts(offsets, first)
    assert streams[1] == streams[4] and len(streams[1]) == SM.BLOCK and per[1] == per[4] and len(per[1]) > 10
    assert (offsets[first[1]] - offsets[first[4]]) % 16 != 0
