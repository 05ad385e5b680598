"""CPU-side checks of the pipelined ingest of many host streams (cw_dev_cdc_streams_part, cw_dev_cdc_streams_part_dedupe_compress,
cw_dev_ingest_commit_streams, cw_store_ingest_streams, ChunkStore.ingest_many_stream / restore_many_stream): the symbols are declared,
listed, exported and mirrored, every refusal comes before the device, the calls fail loudly without one, the new commit kernels compile
without scratch memory or spills, and the piecewise model (tests/streams_ingest_model.py) chains to exactly what chunking every
stream alone gives and leaves what a loop of one-shot ingests leaves.

The inputs of tests/test_gpu_streams_ingest.py are built here, and that each reaches its edge -- a piece that ends on a stream end, a
piece boundary beside an end, an open tail of which nothing is consumed, the largest carry, a stream over many pieces, empty streams
wherever they can lie, a piece of duplicates -- is established here from the model."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import cdc_model as CM
import ingest_model as IM
import restore_model as RM
import streams_ingest_model as XM
import streams_model as SM
from conftest import ROOT

LZ4, LZF = 0, 1
NO_DEVICE, BAD_ARG = -1, -2
ALGS = ["lz4", "lzf"]
P1K, MIN, MAX = SM.P1K, SM.MIN, SM.MAX
P_ALL_MAX = SM.P_NONE                                            # no position is a candidate: every chunk is max_size
S = SM.SEGMENTS["one_max"]                                       # the segment the stream cases are built for
PIECES = (1, 12287, 20001, 40000)                                # CW_STORE_PIECE of the chain test (1 is raised to max_size)
BOUNDARY = [0, 0, 20000, 0, 0, 5000, 15000, 0, 1234, 0]          # ends on the piece boundaries 20000 and 40000, with empty streams there
LONG = [100, 3000, 100000, 50, 0, 7000]                          # a stream over four pieces among small ones


def dup_pieces():
    block = SM.text()[300000:300000 + 40000]
    return [block, block, SM.noise(777, 31)]


# name -> (the streams, the chunking parameters, CW_STORE_PIECE)
SM_PIECES = {"all_candidates": 20001, "dup_block": 12287, "ladder": 12287, "no_candidates": 40000, "no_streams": 40000, "one_byte_x3000": 20001,
             "one_empty": 12287, "one_text_300k": 1, "segment_edges": 20001, "zero_runs": 1}
CASES = {name: (functools.partial(build, S), p, SM_PIECES[name]) for name, (build, p) in SM.CASES.items()}
CASES.update({
    "segment_edges_at_max": (functools.partial(SM.CASES["segment_edges"][0], S), P1K, 1),
    "largest_carry": (lambda: SM.split(SM.noise(40 * MAX + 100, 3), [13 * MAX + 5, 3, 27 * MAX + 92]), P_ALL_MAX, 4 * MAX + MAX - 1),
    "long_among_small": (lambda: SM.split(SM.text()[5000:], LONG), P1K, 30011),
    "empty_on_boundaries": (lambda: SM.split(SM.text()[70000:], BOUNDARY), P1K, 20000),
    "dup_piece": (dup_pieces, P1K, 40000),
})
BIG = dict(store_bytes=4 << 20, dir_entries=1 << 14, max_entries=1 << 14)
REFUSED = "long_among_small"                                     # the case whose middle piece the refusal tests refuse


def oracle_module():
    import oracle as O
    O.build()
    return O


@functools.lru_cache(None)
def streams_of(name):
    return CASES[name][0]()


@functools.lru_cache(None)
def expected(name, alg, base=5, dir_base=5):
    """(the run, the model it filled) of a case with room for everything."""
    _, p, piece = CASES[name]
    m = RM.Model(oracle_module(), alg, BIG["store_bytes"], BIG["dir_entries"], dir_base)
    return XM.ingest_streams(m, streams_of(name), p, piece, base, BIG["max_entries"]), m


@functools.lru_cache(None)
def refusal(kind, alg):
    """REFUSED with one resource sized from the unrefused run so that a middle piece is refused: (run, model, limits, piece index)."""
    _, p, piece = CASES[REFUSED]
    full, _ = expected(REFUSED, alg)
    j = len(full.pieces) // 2
    before = full.pieces[:j]
    lim = dict(BIG)
    if kind == "store":
        lim["store_bytes"] = full.pieces[j]["used_before"] + full.pieces[j]["consumed"] - 1
    elif kind == "directory":
        lim["dir_entries"] = sum(q["chunks"] for q in before) + full.pieces[j]["chunks"] - 1
    else:
        lim["max_entries"] = sum(q["new"] for q in before) + full.pieces[j]["chunks"] - 1
    m = RM.Model(oracle_module(), alg, lim["store_bytes"], lim["dir_entries"], 5)
    return XM.ingest_streams(m, streams_of(REFUSED), p, piece, 5, lim["max_entries"]), m, lim, j


# ---- the boundary ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cwlib():
    import compute_war_amd as cw
    if not os.path.exists(cw.lib_path()):
        subprocess.run(["make", "-C", os.path.join(ROOT, "compute_war_amd", "csrc"), "-j8"], check=True, capture_output=True)
    return cw


NAMES = ("cw_dev_cdc_streams_part", "cw_dev_cdc_streams_part_dedupe_compress", "cw_dev_ingest_commit_streams", "cw_store_ingest_streams")


def test_header_declares_and_binding_lists_the_symbols(cwlib):
    from compute_war_amd import _lib
    text_ = open(os.path.join(ROOT, "include", "cw_hashcompress.h")).read()
    declared = re.findall(r"\b(cw_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text_, flags=re.S))
    out = subprocess.run(["nm", "-D", "--defined-only", cwlib.lib_path()], capture_output=True, text=True, check=True).stdout
    exported = re.findall(r" T (cw_[a-z0-9_]+)", out)
    for name in NAMES:
        assert name in declared and name in _lib.ABI_SYMBOLS and name in exported, name
    for name in ("dev_cdc_streams_part", "dev_ingest_commit_streams", "store_ingest_streams"):
        assert hasattr(cwlib, name), name
    assert hasattr(cwlib.DedupeIndex, "dev_cdc_streams_part_dedupe_compress")
    for name in ("ingest_many_stream", "restore_many_stream"):
        assert hasattr(cwlib.ChunkStore, name), name


NBYTES, NSTREAMS = 5000, 3


def _part_args(cw, **over):
    """cw_dev_cdc_streams_part's arguments with made-up non-NULL device pointers: nothing dereferences them before the device is asked for."""
    p = cw.CdcParams(normal_size=1024)
    a = dict(p=C.byref(p), src=4096, nbytes=NBYTES, ends=8192, nstreams=NSTREAMS, final=0, offsets=12288, max_offsets=NBYTES // 256 + NSTREAMS + 1,
             k=16384, first=20480, result=24576, stream=None)
    a.update(over)
    return p, tuple(a[n] for n in ("p", "src", "nbytes", "ends", "nstreams", "final", "offsets", "max_offsets", "k", "first", "result", "stream"))


@pytest.mark.parametrize("final", [0, 1])
def test_part_refuses_bad_arguments_before_the_device(cwlib, final):
    import torch
    L = cwlib.lib()
    call = lambda **kw: L.cw_dev_cdc_streams_part(*_part_args(cwlib, final=final, **kw)[1])  # noqa: E731
    for name in ("p", "src", "ends", "offsets", "k", "first", "result"):
        assert call(**{name: None}) == BAD_ARG, name
    for d in (1, 2, 4, 7):
        assert call(result=24576 + d) == BAD_ARG and b"8-byte aligned" in L.cw_last_error()
    assert call(nstreams=(1 << 32) - 255, max_offsets=1 << 33) == BAD_ARG and b"nstreams" in L.cw_last_error()
    assert call(max_offsets=NBYTES // 256 + NSTREAMS) == BAD_ARG and b"max_offsets" in L.cw_last_error()
    assert call(nstreams=0, ends=None) == BAD_ARG and b"nstreams is 0" in L.cw_last_error()
    for bad in (dict(reserved=1), dict(min_size=63), dict(min_size=2048), dict(max_size=512), dict(max_size=(1 << 24) + 1)):
        p, args = _part_args(cwlib, final=final)
        for f, v in bad.items():
            setattr(p, f, v)
        assert L.cw_dev_cdc_streams_part(*args) == BAD_ARG, bad
    if not torch.cuda.is_available():
        for kw in (dict(), dict(src=None, nbytes=0, max_offsets=NSTREAMS + 1), dict(src=None, nbytes=0, ends=None, nstreams=0, max_offsets=1),
                   dict(nstreams=(1 << 32) - 256, max_offsets=1 << 33)):
            assert call(**kw) == NO_DEVICE, kw


def _fused_args(cw, **over):
    p = cw.CdcParams(normal_size=1024)
    cap = NBYTES // 256 + NSTREAMS + 1
    k = C.c_size_t(7)
    a = dict(x=4096, p=C.byref(p), alg=LZ4, src=8192, nbytes=NBYTES, ends=12288, nstreams=NSTREAMS, final=0, base=0, offsets=16384, max_offsets=cap,
             k=20480, first=24576, result=28672, dig=32768, ref=36864, new_idx=40960, n_new=45056, dst=49152, dst_bytes=None, sizes=53248,
             nchunks=C.byref(k), stream=None)
    a.update(over)
    if a["dst_bytes"] is None:
        a["dst_bytes"] = cw.chunk_slots_bytes(a["alg"] if a["alg"] in (LZ4, LZF) else LZ4, a["nbytes"], a["max_offsets"] - 1)
    order = ("x", "p", "alg", "src", "nbytes", "ends", "nstreams", "final", "base", "offsets", "max_offsets", "k", "first", "result", "dig", "ref",
             "new_idx", "n_new", "dst", "dst_bytes", "sizes", "nchunks", "stream")
    return (p, k), tuple(a[n] for n in order)


@pytest.mark.parametrize("final", [0, 1])
def test_fused_part_refuses_bad_arguments_before_the_device(cwlib, final):
    import torch
    L = cwlib.lib()

    def call(**kw):
        keep, args = _fused_args(cwlib, final=final, **kw)
        return L.cw_dev_cdc_streams_part_dedupe_compress(*args), keep[1].value
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


def _commit_args(**over):
    a = dict(ref=4096, off=8192, n=12288, max_chunks=100, n_new=16384, result=20480, stream_off=0, rec_ref=24576, rec_off=28672,
             rec_count=32768, rec_cap=1000, stats=36864, verdict=40960, first=45056, ns=4, first_stream=10, skip=0, rec_first=49152, first_cap=100)
    a.update(over)
    return tuple(a[n] for n in ("ref", "off", "n", "max_chunks", "n_new", "result", "stream_off", "rec_ref", "rec_off", "rec_count", "rec_cap",
                                "stats", "verdict", "first", "ns", "first_stream", "skip", "rec_first", "first_cap")) + (None,)


def test_commit_streams_refuses_bad_arguments_before_launch(cwlib):
    import torch
    L = cwlib.lib()
    for name in ("ref", "off", "n", "n_new", "rec_ref", "rec_off", "rec_count", "verdict", "first", "rec_first"):
        assert L.cw_dev_ingest_commit_streams(*_commit_args(**{name: None})) == BAD_ARG, name
    for name in ("ref", "off", "n", "n_new", "result", "rec_ref", "rec_off", "rec_count", "stats", "verdict", "first", "rec_first"):
        for d in (1, 4):
            assert L.cw_dev_ingest_commit_streams(*_commit_args(**{name: 4096 + d})) == BAD_ARG, name
    assert b"8-byte aligned" in L.cw_last_error()
    assert L.cw_dev_ingest_commit_streams(*_commit_args(max_chunks=(1 << 32) - 255)) == BAD_ARG
    assert L.cw_dev_ingest_commit_streams(*_commit_args(ns=(1 << 32) - 255)) == BAD_ARG and b"nstreams_piece" in L.cw_last_error()
    for skip in (2, -1):
        assert L.cw_dev_ingest_commit_streams(*_commit_args(skip=skip)) == BAD_ARG and b"skip_first" in L.cw_last_error()
    if not torch.cuda.is_available():
        # not refused: what the device decides (verdict 3 among it), no store result, no statistics, the largest counts
        for kw in (dict(), dict(result=None), dict(stats=None), dict(skip=1), dict(first_stream=97), dict(first_cap=0), dict(ns=0),
                   dict(ns=(1 << 32) - 256), dict(max_chunks=(1 << 32) - 256)):
            assert L.cw_dev_ingest_commit_streams(*_commit_args(**kw)) == NO_DEVICE, kw


class IngestArgs:
    """cw_store_ingest_streams's arguments with made-up non-NULL device pointers inside the store."""

    def __init__(self, cw, lens=(3000, 0, 2000), **over):
        self.p = cw.CdcParams(normal_size=1024)
        self.st = cw.Store(4096, 1 << 20, 8192, 16384, 0, 1000)
        self.bufs = [np.zeros(max(n, 1), np.uint8) for n in lens]
        self.srcs = (C.c_void_p * len(lens))(*[b.ctypes.data for b in self.bufs])
        self.lens = np.array(lens, np.uint64)
        self.out = np.zeros(256, np.uint64)
        self.k, self.consumed, self.done, self.stats = C.c_size_t(7), C.c_uint64(7), C.c_size_t(7), cw.IngestStats()
        total = int(sum(lens))
        a = dict(x=4096, p=C.byref(self.p), alg=LZ4, st=C.byref(self.st), p_srcs=self.srcs, p_lens=self.lens.ctypes.data, nstreams=len(lens), base=0,
                 refs=self.out.ctypes.data, offsets=self.out.ctypes.data + 512, max_offsets=total // 256 + len(lens) + 1,
                 first=self.out.ctypes.data + 1024, k=C.byref(self.k), consumed=C.byref(self.consumed), done=C.byref(self.done),
                 stats=C.byref(self.stats))
        a.update(over)
        self.args = tuple(a[n] for n in ("x", "p", "alg", "st", "p_srcs", "p_lens", "nstreams", "base", "refs", "offsets", "max_offsets", "first",
                                         "k", "consumed", "done", "stats"))


def test_ingest_streams_refuses_bad_arguments_before_the_device(cwlib):
    import torch
    L = cwlib.lib()
    call = lambda **kw: L.cw_store_ingest_streams(*IngestArgs(cwlib, **kw).args)  # noqa: E731
    for name in ("x", "p", "st", "p_srcs", "p_lens", "refs", "offsets", "first", "k", "consumed", "done"):
        assert call(**{name: None}) == BAD_ARG, name
    for alg in (2, 3, -1, 77):
        assert call(alg=alg) == BAD_ARG
    cap = 5000 // 256 + 3 + 1
    assert call(max_offsets=cap - 1) == BAD_ARG and b"max_offsets" in L.cw_last_error()
    assert call(base=2 ** 64 - (5000 // 256 + 3)) == BAD_ARG and b"wraps" in L.cw_last_error()
    assert call(nstreams=(1 << 32) - 255) == BAD_ARG and b"nstreams" in L.cw_last_error()
    # a NULL span with a length, and lengths whose sum wraps
    a = IngestArgs(cwlib)
    a.srcs[2] = None
    assert L.cw_store_ingest_streams(*a.args) == BAD_ARG and b"span 2 is NULL" in L.cw_last_error()
    a = IngestArgs(cwlib)
    a.lens[:] = [1 << 63, 1 << 62, 1 << 62]
    assert L.cw_store_ingest_streams(*a.args) == BAD_ARG and b"wraps at span 2" in L.cw_last_error()
    for bad in (dict(reserved=1), dict(min_size=63), dict(min_size=2048), dict(max_size=512), dict(max_size=(1 << 24) + 1)):
        a = IngestArgs(cwlib)
        for f, v in bad.items():
            setattr(a.p, f, v)
        assert L.cw_store_ingest_streams(*a.args) == BAD_ARG, bad
    a = IngestArgs(cwlib)
    a.p.max_size = 65537
    assert L.cw_store_ingest_streams(*a.args) == BAD_ARG and b"cannot be stored" in L.cw_last_error()
    for f, v in (("d_dir", 16384 + 8), ("d_dir", 16384 + 1), ("d_used", 8192 + 4), ("dir_entries", 0), ("d_dir", None), ("d_used", None),
                 ("d_store", None)):
        a = IngestArgs(cwlib)
        setattr(a.st, f, v)
        assert L.cw_store_ingest_streams(*a.args) == BAD_ARG, (f, v)
    # every refusal zeroes the counts
    a = IngestArgs(cwlib, max_offsets=cap - 1)
    assert L.cw_store_ingest_streams(*a.args) == BAD_ARG and (a.k.value, a.consumed.value, a.done.value) == (0, 0, 0)
    if not torch.cuda.is_available():
        # not refused: no statistics, the exact bound, an empty span without a pointer, no stream at all, the largest base
        for kw in (dict(stats=None), dict(max_offsets=cap), dict(base=2 ** 64 - (5000 // 256 + 3) - 1),
                   dict(nstreams=0, p_srcs=None, p_lens=None, max_offsets=1)):
            a = IngestArgs(cwlib, **kw)
            assert L.cw_store_ingest_streams(*a.args) == NO_DEVICE, kw
            assert a.k.value == 0 and a.consumed.value == 0
        a = IngestArgs(cwlib)
        a.srcs[1] = None
        assert L.cw_store_ingest_streams(*a.args) == NO_DEVICE


def test_no_gpu_means_no_streamed_ingest_of_many(cwlib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    p = cwlib.CdcParams.default(1024)
    with pytest.raises(cwlib.CwError) as e:
        cwlib.dev_cdc_streams_part(p, 4096, NBYTES, 8192, NSTREAMS, False, 12288, p.max_offsets_streams(NBYTES, NSTREAMS), 16384, 20480, 24576)
    assert e.value.code == NO_DEVICE
    with pytest.raises(cwlib.CwError) as e:
        cwlib.dev_ingest_commit_streams(*[v or 0 for v in _commit_args()[:-1]])
    assert e.value.code == NO_DEVICE


def _meta(asm):
    meta = asm[asm.index("amdhsa.kernels"):]
    out = {}
    for e in re.split(r"\n  - ", meta):
        m = re.search(r"\.name:\s+(\S+)", e)
        if m:
            out[m.group(1)] = e
    return out


def test_commit_streams_kernels_have_no_private_segment_or_spills(tmp_path):
    out = str(tmp_path / "k.s")
    subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-S", "--cuda-device-only", "--offload-arch=gfx950",
                    os.path.join(ROOT, "compute_war_amd", "csrc", "ingest_kernels.hip"), "-o", out], check=True, capture_output=True)
    meta = _meta(open(out).read())
    # the one pair of commit kernels serves both commits (tests/test_ingest_abi.py counts the file's kernels): each takes the stream list
    for kernel in ("commit_copy_kernel", "commit_finish_kernel"):
        assert sum(kernel in k for k in meta) == 1, kernel
        assert sum(kernel in k and "CommitStreams" in k for k in meta) == 1, kernel
    assert not any("commit_streams" in k for k in meta), sorted(meta)
    for name, e in meta.items():
        assert re.search(r"\.private_segment_fixed_size:\s+0\b", e), name
        assert re.search(r"\.vgpr_spill_count:\s+0\b", e), name
        assert re.search(r"\.sgpr_spill_count:\s+0\b", e), name
    makefile = open(os.path.join(ROOT, "compute_war_amd", "csrc", "Makefile")).read()
    srcs = re.search(r"^SRCS\s*:=(.*)$", makefile, flags=re.M).group(1)
    assert "ingest_kernels.hip" in srcs and "commit_streams_kernels.hip" not in srcs
    assert not os.path.exists(os.path.join(ROOT, "compute_war_amd", "csrc", "commit_streams_kernels.hip"))


# ---- the model ---------------------------------------------------------------------------------------------------------------
def test_chunk_part_is_the_chunker_with_an_open_last_stream():
    streams, p, offsets, first = SM.case("dup_block", S)
    data, ends = b"".join(streams), SM.ends_of(streams)
    assert XM.chunk_part(data, ends, True, p) == (offsets, first)
    # truncated inside the last stream: the complete streams keep their cuts, the open one gets cw_dev_cdc(final = 0)'s
    n = ends[-1] - 1000
    got, gf = XM.chunk_part(data[:n], ends[:-1] + [n], False, p)
    tail = CM.chunk(data[ends[-2]:n], p, final=False)
    assert got == offsets[:first[-2]] + [ends[-2] + c for c in tail] and gf == first[:-1] + [len(got) - 1]
    assert n - MAX < got[-1] <= n and got[-1] >= ends[-2]
    # nothing of the open stream is consumed: its first chunk is K, and the last cut is its start
    n = ends[-2] + 100
    got, gf = XM.chunk_part(data[:n], ends[:-1] + [n], False, p)
    assert got == offsets[:first[-2] + 1] and got[-1] == ends[-2] and gf[-2] == gf[-1] == len(got) - 1
    # one open stream is cw_dev_cdc(final = 0); nothing is nothing
    assert XM.chunk_part(streams[1], [len(streams[1])], False, p) == (CM.chunk(streams[1], p, final=False), [0, len(CM.chunk(streams[1], p, final=False)) - 1])
    assert XM.chunk_part(b"", [0], False, p) == ([0], [0, 0]) and XM.chunk_part(b"", [0, 0], False, p) == ([0], [0, 0, 0])


@pytest.mark.parametrize("piece", PIECES)
@pytest.mark.parametrize("seg", sorted(SM.SEGMENTS))
@pytest.mark.parametrize("name", sorted(SM.CASES))
def test_pieces_chained_equal_every_stream_alone(name, seg, piece):
    streams, p, offsets, first = SM.case(name, SM.SEGMENTS[seg])
    run = XM.chain(streams, p, piece)
    assert (run.offsets, run.first) == (offsets, first)
    assert run.streams_done == len(streams) and all(0 <= c < p["max"] for c in run.carries)
    for q in run.log:
        assert q["cuts"][-1] == len(q["part"]) if q["final"] else len(q["part"]) - p["max"] < q["cuts"][-1] <= len(q["part"])
        assert len(q["cuts"]) - 1 <= len(q["part"]) // p["min"] + len(q["ends"])


@pytest.mark.parametrize("alg", ALGS)
@pytest.mark.parametrize("name", sorted(CASES))
def test_model_equals_a_loop_of_one_shot_ingests(oracle, name, alg):
    _, p, piece = CASES[name]
    streams = streams_of(name)
    run, m = expected(name, alg)
    one = RM.Model(oracle, alg, BIG["store_bytes"], BIG["dir_entries"], 5)
    base, want = 5, []
    for s in streams:
        refs, cuts = IM.one_shot(one, s, p, base)
        want.append((refs, cuts))
        base += len(refs)
    whole, partial = run.recipes()
    assert run.refused is None and partial is None and whole == want and run.streams_done == len(streams)
    assert (run.offsets, run.first) == SM.chunk_streams(streams, p) and run.nchunks == base - 5
    assert bytes(m.blob) == bytes(one.blob) and (m.directory == one.directory).all() and m.values == one.values
    n = sum(len(s) for s in streams)
    assert run.stats == dict(bytes=n, chunks=run.nchunks, new_chunks=len(one.values), stored_bytes=len(one.blob), pieces=len(run.pieces))


def test_every_case_reaches_its_edge():
    """Pieces, carries and duplicates are the model's, so the codec does not matter."""
    run = {name: expected(name, "lz4")[0] for name in CASES}
    # a piece that ends on a stream end in mid-run (final = 1, no carry behind it), three times; boundaries one byte before and behind an end
    r = run["segment_edges_at_max"]
    ends = SM.ends_of(streams_of("segment_edges_at_max"))
    assert ends == [S - 1, S, 2 * S, 3 * S + 1, 4 * S, 6 * S] and len(r.log) == 6
    assert [q["end"] for q in r.log if q["final"]] == [S, 2 * S, 4 * S, 6 * S]
    assert all(r.log[q["index"] + 1]["carry"] == 0 and not r.log[q["index"] + 1]["skip_first"] for q in r.log[:-1] if q["final"])
    assert any(q["end"] - 1 in ends for q in r.log) and any(q["end"] + 1 in ends for q in r.log)
    # an open tail of which nothing is consumed: its entry is written by that piece and is the next piece's first chunk
    empty_tails = [(name, q) for name, r in run.items() for q in r.log if q["open_consumed"] == 0 and len(q["ends"]) > 1]
    assert len({name for name, _ in empty_tails}) >= 3
    name, q = empty_tails[0]
    assert q["first"][-2] == q["first"][-1] == len(q["cuts"]) - 1 and run[name].log[q["index"] + 1]["skip_first"]
    # the largest carry there is
    r = run["largest_carry"]
    assert r.carries[:3] == [0, MAX - 1, MAX - 2] and max(r.carries) == MAX - 1 and len(r.log) == 9
    assert set(np.diff(r.offsets).tolist()) == {MAX, 5, 3, 92} and sum(q["final"] for q in r.log) == 1
    # a stream over at least three pieces among small ones: pieces of one open stream, continued (skip_first) twice and more
    r = run["long_among_small"]
    spans = [q for q in r.log if q["first_stream"] == 2 and q["skip_first"]]
    assert len(r.log) == 4 and len(spans) >= 3 and sum(len(q["ends"]) == 1 and not q["final"] for q in r.log) >= 2
    assert r.first[2] < r.first[3] and r.first[4] == r.first[5]
    # empty streams first, last, doubled and on a piece boundary
    r = run["empty_on_boundaries"]
    assert [q["end"] for q in r.log] == [20000, 40000, 41234] and [q["final"] for q in r.log] == [True, True, True]
    assert [q["took"] for q in r.log] == [5, 3, 2] and r.log[0]["ends"] == [0, 0, 20000, 20000, 20000]
    assert r.first[0] == r.first[1] == r.first[2] == 0 and r.first[3] == r.first[4] == r.first[5] and r.first[-1] == r.first[-2] == r.nchunks
    lens = [len(s) for s in streams_of("ladder")]
    assert lens[0] == 0 and lens[-2:] == [0, 0] and lens[2:4] == [0, 0] and len(run["ladder"].log) >= 2
    assert run["no_streams"].log == [] and run["one_empty"].log == [] and run["one_empty"].first == [0, 0] and run["no_streams"].first == [0]
    # 3,000 one-byte streams in one piece
    r = run["one_byte_x3000"]
    assert len(r.log) == 1 and len(r.log[0]["ends"]) == 3000 and r.log[0]["final"] and r.first == list(range(3001))
    # a piece whose chunks are all duplicates
    r = run["dup_piece"]
    assert [(q["new"] == 0, q["chunks"] > 10) for q in r.pieces[:2]] == [(False, True), (True, True)] and r.log[0]["final"]
    # and among all cases: pieces with both values of final and of skip_first, several streams in an open piece
    every = [q for r in run.values() for q in r.log]
    assert {(q["final"], q["skip_first"]) for q in every} == {(a, b) for a in (True, False) for b in (True, False)}
    assert any(not q["final"] and len(q["ends"]) > 3 for q in every)


@pytest.mark.parametrize("alg", ALGS)
@pytest.mark.parametrize("kind", ["store", "directory", "index"])
def test_a_refused_piece_leaves_the_prefix_ingested_whole(oracle, kind, alg):
    _, p, piece = CASES[REFUSED]
    streams = streams_of(REFUSED)
    data = b"".join(streams)
    run, m, lim, j = refusal(kind, alg)
    full, _ = expected(REFUSED, alg)
    assert run.refused == kind and len(run.pieces) == j == 2 and 0 < run.consumed < len(data)
    assert run.refs == full.refs[:run.nchunks] and run.offsets == full.offsets[:run.nchunks + 1]
    # the streams that are done, the one that was cut, and the index entries behind them
    ends = SM.ends_of(streams)
    done = sum(1 for e in ends if e <= run.consumed)
    assert run.streams_done == done == 2 and run.first == full.first[:done + 1] + [run.nchunks]
    whole, partial = run.recipes()
    assert whole == full.recipes()[0][:done] and partial is not None and partial[1][-1] == run.consumed - ends[done - 1]
    # the prefix as streams of its own: the same index, store and directory
    prefix = RM.Model(oracle, alg, BIG["store_bytes"], BIG["dir_entries"], 5)
    pre = XM.ingest_streams(prefix, streams[:done] + [data[ends[done - 1]:run.consumed]], p, piece, 5, BIG["max_entries"])
    assert pre.refs == run.refs and pre.offsets == run.offsets and pre.first == run.first
    assert bytes(m.blob) == bytes(prefix.blob) and m.values == prefix.values and (m.directory == prefix.directory[:len(m.directory)]).all()
    # resumed with the spans from streams_done on, the first shortened, and room made: the uninterrupted run
    more = IM.clone(m, BIG["store_bytes"], BIG["dir_entries"])
    rest = XM.ingest_streams(more, [data[run.consumed:ends[done]]] + streams[done + 1:], p, piece, 5 + run.nchunks, BIG["max_entries"])
    assert rest.refused is None and run.refs + rest.refs == full.refs
    assert run.offsets + [run.consumed + c for c in rest.offsets[1:]] == full.offsets
    assert run.first[:done + 1] + [run.nchunks + f for f in rest.first[1:]] == full.first


def test_commit_streams_model():
    rec_ref, rec_off, rec_first, stats = [0] * 12, [0] * 12, [None] * 6, [0] * 5
    args = lambda: (rec_ref, rec_off)  # noqa: E731
    # a piece of three streams, the last open with nothing consumed
    v, c = XM.commit_streams([7, 8, 9], [0, 10, 30, 60], 3, 2, [0, 55], 1000, *args(), 0, 12, stats, [0, 2, 3, 3], 3, 0, False, rec_first, 6)
    assert (v, c) == (0, 3) and rec_first == [0, 2, 3, None, None, None] and rec_off[:4] == [1000, 1010, 1030, 1060]
    # the next piece continues stream 2 (its entry stays) and closes streams 3 and 4
    v, c = XM.commit_streams([1, 2], [0, 5, 9], 2, 0, None, 1060, *args(), c, 12, stats, [0, 1, 2, 2], 3, 2, True, rec_first, 6)
    assert (v, c) == (0, 5) and rec_first == [0, 2, 3, 4, 5, None] and stats == [69, 5, 2, 55, 2]
    before = (list(rec_ref), list(rec_off), list(rec_first), list(stats))
    assert XM.commit_streams([1], [0, 1], 1, 0, None, 0, *args(), c, 12, stats, [0, 1], 1, 6, False, rec_first, 6) == (3, 5)
    assert XM.commit_streams([1], [0, 1], 1, 0, None, 0, *args(), c, 12, stats, [0, 0, 1], 2, 5, False, rec_first, 6) == (3, 5)
    assert XM.commit_streams([1], [0, 1], 1, 0, [1, 9], 0, *args(), c, 12, stats, [0, 1], 1, 9, False, rec_first, 6) == (1, 5)
    assert XM.commit_streams([1] * 7, list(range(8)), 7, 0, None, 0, *args(), c, 12, stats, [0, 7], 1, 9, False, rec_first, 6) == (2, 5)
    assert before == (rec_ref, rec_off, rec_first, stats)
