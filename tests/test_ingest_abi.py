"""CPU-side checks of the streamed chunk store (cw_store_ingest, cw_dev_ingest_commit, cw_store_restore): the symbols are declared,
listed, exported and mirrored, the two structs have the sizes the binding assumes, every refusal comes before the device, the calls
fail loudly without one, the commit kernels compile without scratch memory or spills, the knob is accepted, and the piecewise model
(tests/ingest_model.py) leaves exactly what restore_model.Model's one-shot ingest leaves.

The inputs of tests/test_gpu_ingest.py are built here, and that each reaches its edge -- which carries occur, how many pieces, which
piece has no new chunk -- is established here from the model."""
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
from conftest import ROOT, corpus_file

LZ4, LZF = 0, 1
NO_DEVICE, BAD_ARG = -1, -2
ALGS = ["lz4", "lzf"]
P1K = CM.default_params(1024)                                   # chunks of 256 .. 8192 bytes
MIN, MAX = P1K["min"], P1K["max"]
P_ALL_MIN = dict(P1K, gear=np.zeros(256, np.uint64))            # every mask test fires: every chunk is min_size
P_ALL_MAX = dict(P1K, gear=np.full(256, 1 << 63, np.uint64))    # H = 2^63 everywhere, no test fires: every chunk is max_size
P_64K = dict(min=65536, avg=65536, max=65536, mask_s=P1K["mask_s"], mask_l=P1K["mask_l"], gear=np.full(256, 1 << 63, np.uint64))


def noise(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


@functools.lru_cache(None)
def text():
    return corpus_file("lcet10.txt") + corpus_file("plrabn12.txt") + corpus_file("alice29.txt") + corpus_file("asyoulik.txt")


@functools.lru_cache(None)
def dups():
    """A stream whose second half repeats its first, and whose first half repeats a block at short distances."""
    t = text()
    block = t[400000:409000]
    half = t[:150000] + b"".join(block + noise(700, 40 + i) for i in range(6)) + noise(60000, 7) + t[200000:330000]
    return half + half


# name -> (the stream, the chunking parameters, CW_STORE_PIECE)
CASES = {
    "all_min": (lambda: noise(200000, 1), P_ALL_MIN, 20001),
    "all_max_no_carry": (lambda: noise(40 * MAX + 100, 2), P_ALL_MAX, 4 * MAX),
    "all_max_largest_carry": (lambda: noise(40 * MAX + 100, 3), P_ALL_MAX, 4 * MAX + MAX - 1),
    "text": (lambda: text()[:1100000], P1K, 50001),
    "dups": (dups, P1K, 30011),
    "empty": (lambda: b"", P1K, 30011),
    "one_byte": (lambda: b"x", P1K, 30011),
    "min_size": (lambda: text()[:MIN], P1K, 30011),
    "one_piece": (lambda: text()[:40000], P1K, 40000),
    "one_piece_plus_1": (lambda: text()[:40001], P1K, 40000),
    "short_last": (lambda: text()[:3 * 40000 + 100], P1K, 40000),
    "floor": (lambda: text()[:100000], P1K, 1),
}
BIG = dict(store_bytes=4 << 20, dir_entries=1 << 14, max_entries=1 << 14)


def oracle_module():
    import oracle as O
    O.build()
    return O


@functools.lru_cache(None)
def expected(name, alg, base=5, dir_base=5):
    """(the streamed run, the model it filled) of a case with room for everything."""
    data, p, piece = CASES[name]
    m = RM.Model(oracle_module(), alg, BIG["store_bytes"], BIG["dir_entries"], dir_base)
    return IM.ingest(m, data(), p, piece, base, BIG["max_entries"]), m


@functools.lru_cache(None)
def refusal(kind, alg):
    """The text case with one resource sized from the unrefused run so that a middle piece is refused: (run, model, limits)."""
    data, p, piece = CASES["text"]
    full, fm = expected("text", alg)
    j = len(full.pieces) // 2                      # the piece that is refused
    before = full.pieces[:j]
    lim = dict(BIG)
    if kind == "store":
        lim["store_bytes"] = full.pieces[j]["used_before"] + full.pieces[j]["consumed"] - 1
    elif kind == "directory":
        lim["dir_entries"] = sum(q["chunks"] for q in before) + full.pieces[j]["chunks"] - 1
    else:
        lim["max_entries"] = sum(q["new"] for q in before) + full.pieces[j]["chunks"] - 1
    m = RM.Model(oracle_module(), alg, lim["store_bytes"], lim["dir_entries"], 5)
    return IM.ingest(m, data(), p, piece, 5, lim["max_entries"]), m, lim, j


# ---- the boundary ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cwlib():
    import compute_war_amd as cw
    if not os.path.exists(cw.lib_path()):
        subprocess.run(["make", "-C", os.path.join(ROOT, "compute_war_amd", "csrc"), "-j8"], check=True, capture_output=True)
    return cw


NAMES = ("cw_store_ingest", "cw_dev_ingest_commit", "cw_store_restore")


def test_header_declares_and_binding_lists_the_symbols(cwlib):
    from compute_war_amd import _lib
    text_ = open(os.path.join(ROOT, "include", "cw_hashcompress.h")).read()
    declared = re.findall(r"\b(cw_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text_, flags=re.S))
    out = subprocess.run(["nm", "-D", "--defined-only", cwlib.lib_path()], capture_output=True, text=True, check=True).stdout
    exported = re.findall(r" T (cw_[a-z0-9_]+)", out)
    for name in NAMES:
        assert name in declared and name in _lib.ABI_SYMBOLS and name in exported, name
    for name in ("store_ingest", "store_restore", "dev_ingest_commit", "Store", "IngestStats"):
        assert hasattr(cwlib, name), name
    for name in ("ingest_stream", "restore_stream", "last_stats"):
        assert hasattr(cwlib.ChunkStore, name), name


def test_struct_sizes_through_a_c_compiler(cwlib, tmp_path):
    src, exe = tmp_path / "s.c", tmp_path / "s"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "cw_hashcompress.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu\\n", sizeof(cw_store), sizeof(cw_ingest_stats), offsetof(cw_store, d_used),\n'
                   '                        offsetof(cw_store, dir_base), offsetof(cw_ingest_stats, pieces)); return 0; }\n')
    subprocess.run(["cc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True, capture_output=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [48, 64, 16, 32, 32]
    assert C.sizeof(cwlib.Store) == 48 and C.sizeof(cwlib.IngestStats) == 64
    assert cwlib.Store.d_used.offset == 16 and cwlib.Store.dir_base.offset == 32 and cwlib.IngestStats.pieces.offset == 32


class IngestArgs:
    """cw_store_ingest's arguments with made-up non-NULL pointers; nothing dereferences the device ones before the device is asked for."""

    def __init__(self, cw, **over):
        self.p = cw.CdcParams(normal_size=1024)
        self.st = cw.Store(4096, 1 << 20, 8192, 16384, 0, 1000)
        self.src = np.zeros(5000, np.uint8)
        self.out = np.zeros(64, np.uint64)
        self.k, self.consumed, self.stats = C.c_size_t(7), C.c_size_t(7), cw.IngestStats()
        a = dict(x=4096, p=C.byref(self.p), alg=LZ4, st=C.byref(self.st), src=self.src.ctypes.data, nbytes=5000, base=0,
                 refs=self.out.ctypes.data, offsets=self.out.ctypes.data + 256, max_offsets=5000 // 256 + 2, k=C.byref(self.k),
                 consumed=C.byref(self.consumed), stats=C.byref(self.stats))
        a.update(over)
        self.args = tuple(a[n] for n in ("x", "p", "alg", "st", "src", "nbytes", "base", "refs", "offsets", "max_offsets", "k", "consumed", "stats"))


def test_ingest_refuses_bad_arguments_before_the_device(cwlib):
    import torch
    L = cwlib.lib()
    call = lambda **kw: L.cw_store_ingest(*IngestArgs(cwlib, **kw).args)  # noqa: E731
    for name in ("x", "p", "st", "src", "refs", "offsets", "k", "consumed"):
        assert call(**{name: None}) == BAD_ARG, name
    for alg in (2, 3, -1, 77):
        assert call(alg=alg) == BAD_ARG
    assert call(max_offsets=5000 // 256 + 1) == BAD_ARG and b"max_offsets" in L.cw_last_error()
    assert call(base=2 ** 64 - 5000 // 256 - 1) == BAD_ARG and b"wraps" in L.cw_last_error()
    # what cdc_params refuses, and chunks that could never be stored
    for bad in (dict(reserved=1), dict(min_size=63), dict(min_size=2048), dict(max_size=512), dict(max_size=(1 << 24) + 1)):
        a = IngestArgs(cwlib)
        for f, v in bad.items():
            setattr(a.p, f, v)
        assert L.cw_store_ingest(*a.args) == BAD_ARG, bad
    a = IngestArgs(cwlib)
    a.p.max_size = 65537
    assert L.cw_store_ingest(*a.args) == BAD_ARG and b"cannot be stored" in L.cw_last_error()
    # the store: alignments, an empty directory, NULL members
    for f, v in (("d_dir", 16384 + 8), ("d_dir", 16384 + 1), ("d_used", 8192 + 4), ("dir_entries", 0), ("d_dir", None), ("d_used", None),
                 ("d_store", None)):
        a = IngestArgs(cwlib)
        setattr(a.st, f, v)
        assert L.cw_store_ingest(*a.args) == BAD_ARG, (f, v)
    if not torch.cuda.is_available():
        # not refused: no statistics, an empty input without a source, the largest base that does not wrap
        for kw in (dict(stats=None), dict(src=None, nbytes=0, max_offsets=2), dict(base=2 ** 64 - 5000 // 256 - 2)):
            a = IngestArgs(cwlib, **kw)
            assert L.cw_store_ingest(*a.args) == NO_DEVICE, kw
            assert a.k.value == 0 and a.consumed.value == 0


def _commit_args(**over):
    a = dict(ref=4096, off=8192, n=12288, max_chunks=100, n_new=16384, result=20480, stream_off=0, rec_ref=24576, rec_off=28672,
             rec_count=32768, rec_cap=1000, stats=36864, verdict=40960)
    a.update(over)
    return tuple(a[n] for n in ("ref", "off", "n", "max_chunks", "n_new", "result", "stream_off", "rec_ref", "rec_off", "rec_count", "rec_cap",
                                "stats", "verdict")) + (None,)


def test_commit_refuses_bad_arguments_before_launch(cwlib):
    import torch
    L = cwlib.lib()
    for name in ("ref", "off", "n", "n_new", "rec_ref", "rec_off", "rec_count", "verdict"):
        assert L.cw_dev_ingest_commit(*_commit_args(**{name: None})) == BAD_ARG, name
    for name in ("ref", "off", "n", "n_new", "result", "rec_ref", "rec_off", "rec_count", "stats", "verdict"):
        for d in (1, 4):
            assert L.cw_dev_ingest_commit(*_commit_args(**{name: 4096 + d})) == BAD_ARG, name
    assert b"8-byte aligned" in L.cw_last_error()
    assert L.cw_dev_ingest_commit(*_commit_args(max_chunks=(1 << 32) - 255)) == BAD_ARG
    if not torch.cuda.is_available():
        for kw in (dict(result=None), dict(stats=None), dict(max_chunks=(1 << 32) - 256), dict(max_chunks=0), dict(rec_cap=0)):
            assert L.cw_dev_ingest_commit(*_commit_args(**kw)) == NO_DEVICE, kw


def _restore_args(cw, offsets=(0, 100, 300), refs=(1, 2), dst_bytes=300, **over):
    st = cw.Store(4096, 1 << 20, 8192, 16384, 0, 1000)
    for f in ("d_store", "d_used", "d_dir", "dir_entries"):
        if f in over:
            setattr(st, f, over.pop(f))
    keep = [st, np.asarray(refs, np.uint64), np.asarray(offsets, np.uint64), np.zeros(max(dst_bytes, 1), np.uint8), np.zeros(8, np.uint32),
            C.c_size_t(9)]
    a = dict(alg=LZ4, st=C.byref(st), p_refs=keep[1].ctypes.data, p_offsets=keep[2].ctypes.data, n=len(refs), dst=keep[3].ctypes.data,
             dst_bytes=dst_bytes, status=keep[4].ctypes.data, n_bad=C.byref(keep[5]))
    a.update(over)
    return keep, tuple(a[n] for n in ("alg", "st", "p_refs", "p_offsets", "n", "dst", "dst_bytes", "status", "n_bad"))


def test_restore_refuses_bad_arguments_before_the_device(cwlib):
    import torch
    L = cwlib.lib()

    def call(**kw):
        keep, args = _restore_args(cwlib, **kw)
        return L.cw_store_restore(*args)
    for name in ("st", "p_refs", "p_offsets", "dst", "n_bad"):
        assert call(**{name: None}) == BAD_ARG, name
    for alg in (2, -1, 9):
        assert call(alg=alg) == BAD_ARG
    assert call(dst_bytes=299) == BAD_ARG and b"dst_bytes" in L.cw_last_error()
    assert call(offsets=(1000, 1100, 1300), dst_bytes=299) == BAD_ARG                 # the stream's length counts, not its end
    assert call(offsets=(0, 300, 100), dst_bytes=400) == BAD_ARG and b"decrease" in L.cw_last_error()
    assert call(offsets=(0, 100, 100 + 65537), dst_bytes=1 << 17) == BAD_ARG and b"long" in L.cw_last_error()
    for f, v in (("d_dir", 16384 + 8), ("d_used", 8192 + 4), ("dir_entries", 0), ("d_dir", None), ("d_store", None)):
        assert call(**{f: v}) == BAD_ARG, (f, v)
    if not torch.cuda.is_available():
        for kw in (dict(), dict(status=None), dict(offsets=(1000, 1100, 1300)), dict(offsets=(0, 100, 100 + 65536), dst_bytes=1 << 17),
                   dict(offsets=(7,), refs=(), dst=None, dst_bytes=0)):
            assert call(**kw) == NO_DEVICE, kw


def test_no_gpu_means_no_streamed_ingest(cwlib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    cs = object.__new__(cwlib.ChunkStore)   # (a store cannot be made without a device)
    st = cwlib.Store(4096, 1 << 20, 8192, 16384, 0, 1000)
    with pytest.raises(cwlib.CwError) as e:
        cwlib.store_restore("lzf", st, [1, 2], [0, 100, 300], np.zeros(300, np.uint8).ctypes.data, 300)
    assert e.value.code == NO_DEVICE
    with pytest.raises(cwlib.CwError) as e:
        cwlib.dev_ingest_commit(*_commit_args()[:-1])
    assert e.value.code == NO_DEVICE
    assert cs.last_stats is None


def _meta(asm):
    meta = asm[asm.index("amdhsa.kernels"):]
    out = {}
    for e in re.split(r"\n  - ", meta):
        m = re.search(r"\.name:\s+(\S+)", e)
        if m:
            out[m.group(1)] = e
    return out


def test_commit_kernels_have_no_private_segment_or_spills(tmp_path):
    out = str(tmp_path / "k.s")
    subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-S", "--cuda-device-only", "--offload-arch=gfx950",
                    os.path.join(ROOT, "compute_war_amd", "csrc", "ingest_kernels.hip"), "-o", out], check=True, capture_output=True)
    meta = _meta(open(out).read())
    assert len(meta) == 3, sorted(meta)
    for kernel in ("commit_copy_kernel", "commit_finish_kernel", "piece_counts_kernel"):
        assert sum(kernel in k for k in meta) == 1, kernel
    for name, e in meta.items():
        assert re.search(r"\.private_segment_fixed_size:\s+0\b", e), name
        assert re.search(r"\.vgpr_spill_count:\s+0\b", e), name
        assert re.search(r"\.sgpr_spill_count:\s+0\b", e), name
    makefile = open(os.path.join(ROOT, "compute_war_amd", "csrc", "Makefile")).read()
    srcs = re.search(r"^SRCS\s*:=(.*)$", makefile, flags=re.M).group(1)
    assert "ingest_kernels.hip" in srcs and "cw_ingest.hip" in srcs


def test_the_knob_is_accepted_and_documented(cwlib):
    L = cwlib.lib()
    try:
        assert L.cw_tune_set(b"CW_STORE_PIECE", b"30011") == 0 and L.cw_tune_set(b"CW_STORE_PIECE", None) == 0
    finally:
        cwlib.tune_reset()
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "`CW_STORE_PIECE=" in readme[readme.index("Profiling / test knobs"):].split("\n\n")[0]
    assert "store_piece" in open(os.path.join(ROOT, "compute_war_amd", "csrc", "knobs.h")).read()


# ---- the model ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alg", ALGS)
@pytest.mark.parametrize("name", sorted(CASES))
def test_piecewise_model_equals_the_one_shot_ingest(oracle, name, alg):
    data, p, piece = CASES[name]
    run, m = expected(name, alg)
    one = RM.Model(oracle, alg, BIG["store_bytes"], BIG["dir_entries"], 5)
    refs, cuts = IM.one_shot(one, data(), p, 5)
    assert run.refused is None and run.refs == refs and run.offsets == cuts == CM.chunk_pieces(data(), p, []) and run.consumed == len(data())
    assert bytes(m.blob) == bytes(one.blob) and (m.directory == one.directory).all() and m.values == one.values
    assert run.stats == dict(bytes=len(data()), chunks=len(refs), new_chunks=len(one.values), stored_bytes=len(one.blob), pieces=len(run.pieces))
    lens = np.diff(cuts)
    assert len(lens) == 0 or lens.max() <= p["max"]


def test_every_input_reaches_its_edge():
    """Carries, piece counts and duplicates are the model's, so the codec does not matter."""
    run = {name: expected(name, "lz4")[0] for name in CASES}
    n = {name: len(r.pieces) for name, r in run.items()}
    lens = {name: np.diff(r.offsets) for name, r in run.items()}
    # the carry's extremes: none at all, the largest there is, a band under max_size, and everything between
    assert n["all_max_no_carry"] == 11 and set(run["all_max_no_carry"].carries) == {0} and set(lens["all_max_no_carry"][:-1]) == {MAX}
    r = run["all_max_largest_carry"]
    assert len(r.pieces) == 9 and r.carries[:3] == [0, MAX - 1, MAX - 2] and max(r.carries) == MAX - 1 and set(lens["all_max_largest_carry"][:-1]) == {MAX}
    r = run["all_min"]
    assert len(r.pieces) == 10 and all(MAX - MIN <= c < MAX for c in r.carries[1:]) and set(lens["all_min"][:-1]) == {MIN}
    r = run["text"]
    assert len(r.pieces) == 22 and r.carries[0] == 0 and all(0 <= c < MAX for c in r.carries)
    # (a piece ends at the first cut with less than max_size behind it, so a carry lies within one chunk's length under max_size)
    assert min(r.carries[1:]) < MAX - 4 * MIN and max(r.carries) > MAX - MIN and len(set(r.carries)) >= 18
    assert lens["text"].min() >= 1 and MIN <= np.median(lens["text"]) and lens["text"].max() <= MAX
    # the length edges
    assert [run[k].nchunks for k in ("empty", "one_byte", "min_size")] == [0, 1, 1] and n["empty"] == 0 and n["one_byte"] == n["min_size"] == 1
    assert n["one_piece"] == 1 and n["one_piece_plus_1"] == 2 and n["short_last"] == 4 and n["floor"] == 13
    r = run["short_last"]
    assert 100 + r.carries[-1] == r.pieces[-1]["consumed"] and 100 <= MIN
    assert run["one_piece_plus_1"].pieces[1]["consumed"] == 1 + run["one_piece_plus_1"].carries[1]
    # duplicates: refs into earlier pieces, a piece with no new chunk, duplicates inside one piece
    r = run["dups"]
    half = len(dups()) // 2
    assert 20 <= len(r.pieces) <= 60
    first_of_second = next(j for j, c in enumerate(r.offsets) if c >= half + MAX)   # the cuts have met the first half's again
    assert sum(1 for j in range(first_of_second, r.nchunks) if r.refs[j] < 5 + first_of_second) > (r.nchunks - first_of_second) * 0.9
    assert any(q["new"] == 0 and q["chunks"] > 0 for q in r.pieces) and any(q["inner_dups"] > 0 for q in r.pieces)
    assert r.stats["new_chunks"] < 0.6 * r.stats["chunks"]


@pytest.mark.parametrize("alg", ALGS)
@pytest.mark.parametrize("kind", ["store", "directory", "index"])
def test_a_refused_piece_leaves_the_prefix_ingested_whole(oracle, kind, alg):
    data, p, piece = CASES["text"]
    run, m, lim, j = refusal(kind, alg)
    full, _ = expected("text", alg)
    assert run.refused == kind and len(run.pieces) == j and 5 <= j < len(full.pieces) - 5
    assert run.refs == full.refs[:run.nchunks] and run.offsets == full.offsets[:run.nchunks + 1]
    prefix = RM.Model(oracle, alg, BIG["store_bytes"], BIG["dir_entries"], 5)
    refs, cuts = IM.one_shot(prefix, data()[:run.consumed], p, 5)
    assert refs == run.refs and cuts == run.offsets
    assert bytes(m.blob) == bytes(prefix.blob) and m.values == prefix.values
    assert (m.directory == prefix.directory[:len(m.directory)]).all()
    # the recipe so far restores those bytes
    got = RM.restore(m.blob, m.store_bytes, m.directory, 5, run.refs, run.offsets, run.consumed, m.decode())
    assert all(s == 0 for s, _ in got) and b"".join(piece_ for _, piece_ in got) == data()[:run.consumed]
    # resumed from the cut with room made, the run is the uninterrupted one
    more = IM.clone(m, BIG["store_bytes"], BIG["dir_entries"])
    rest = IM.ingest(more, data()[run.consumed:], p, piece, 5 + run.nchunks, BIG["max_entries"])
    assert rest.refused is None and run.refs + rest.refs == full.refs
    assert run.offsets + [run.consumed + c for c in rest.offsets[1:]] == full.offsets


def test_commit_model():
    rec_ref, rec_off, stats = [0] * 10, [0] * 10, [0] * 5
    v, c = IM.commit([7, 8, 9], [0, 10, 30, 60], 3, 2, [0, 55], 1000, rec_ref, rec_off, 0, 10, stats)
    assert (v, c) == (0, 3) and rec_ref[:3] == [7, 8, 9] and rec_off[:4] == [1000, 1010, 1030, 1060] and stats == [60, 3, 2, 55, 1]
    v, c = IM.commit([1], [5, 25], 1, 0, None, 1055, rec_ref, rec_off, c, 10, stats)
    assert (v, c) == (0, 4) and rec_off[3:5] == [1060, 1080] and stats == [80, 4, 2, 55, 2]
    assert IM.commit([1] * 5, list(range(6)), 5, 0, None, 0, rec_ref, rec_off, 4, 10, stats) == (0, 9)
    before = (list(rec_ref), list(rec_off), list(stats))
    assert IM.commit([1], [0, 1], 1, 0, None, 0, rec_ref, rec_off, 9, 10, stats) == (2, 9)
    assert IM.commit([1], [0, 1], 1, 0, [1, 9], 0, rec_ref, rec_off, 0, 10, stats) == (1, 0)
    assert before == (rec_ref, rec_off, stats)
