"""CPU-side checks of the chunk store: the two symbols are declared, listed, exported and mirrored, cw_chunk_loc is 16 bytes,
the calls refuse bad arguments before the device and fail loudly without one, the kernels compile without scratch memory
or spills, and the plain-Python model round-trips with the CPU oracle's codecs."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import cdc_model as CM
import restore_model as RM
from conftest import ROOT, corpus_file

NEW_SYMBOLS = ["cw_dev_store_chunks", "cw_dev_restore_chunks"]
LZ4, LZF = 0, 1
NO_DEVICE, BAD_ARG = -1, -2


@pytest.fixture(scope="module")
def cwlib():
    import compute_war_amd as cw
    if not os.path.exists(cw.lib_path()):
        subprocess.run(["make", "-C", os.path.join(ROOT, "compute_war_amd", "csrc"), "-j8"], check=True, capture_output=True)
    return cw


def test_header_declares_and_binding_lists_the_store_symbols(cwlib):
    from compute_war_amd import _lib
    text = open(os.path.join(ROOT, "include", "cw_hashcompress.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert set(NEW_SYMBOLS) <= set(re.findall(r"\b(cw_[a-z0-9_]+)\s*\(", text))
    assert re.search(r"typedef struct cw_chunk_loc \{\s*uint64_t pos;\s*uint32_t stored;\s*uint32_t raw;\s*\} cw_chunk_loc;", text)
    assert set(NEW_SYMBOLS) <= set(_lib.ABI_SYMBOLS)
    out = subprocess.run(["nm", "-D", "--defined-only", cwlib.lib_path()], capture_output=True, text=True, check=True).stdout
    assert set(NEW_SYMBOLS) <= set(re.findall(r" T (cw_[a-z0-9_]+)", out))
    for name in ("dev_store_chunks", "dev_restore_chunks", "ChunkStore", "ChunkLoc", "Recipe"):
        assert hasattr(cwlib, name)
    for name in ("ingest", "restore", "save", "load"):
        assert hasattr(cwlib.ChunkStore, name)


def test_chunk_loc_is_16_bytes(cwlib, tmp_path):
    assert C.sizeof(cwlib.ChunkLoc) == 16 == RM.LOC.itemsize
    assert (cwlib.ChunkLoc.pos.offset, cwlib.ChunkLoc.stored.offset, cwlib.ChunkLoc.raw.offset) == (0, 8, 12)
    assert cwlib.ChunkLoc.RAW == RM.RAW
    src = tmp_path / "loc.c"   # the header's own struct, through a C compiler
    src.write_text('#include <stddef.h>\n#include "cw_hashcompress.h"\n'
                   "_Static_assert(sizeof(cw_chunk_loc) == 16 && offsetof(cw_chunk_loc, stored) == 8 && offsetof(cw_chunk_loc, raw) == 12, \"layout\");\n"
                   "_Static_assert(CW_CHUNK_RAW == 0x80000000u, \"flag\");\nint main(void) { return 0; }\n")
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "loc.o")], check=True,
                   capture_output=True)


def _store_args(alg=LZ4, max_chunks=1000, src_bytes=1 << 20, store_bytes=1 << 20, dir_entries=1000, **over):
    """Arguments of cw_dev_store_chunks with made-up non-NULL pointers (nothing dereferences them before the device is asked for)."""
    a = dict(d_src=4096, d_offsets=8192, d_nchunks=12288, d_sel=None, d_nsel=None, d_slots=16384, d_sizes=20480, d_store=24576, d_used=28672,
             d_dir=32768, d_result=36864)
    a.update(over)
    return (alg, a["d_src"], src_bytes, a["d_offsets"], a["d_nchunks"], max_chunks, a["d_sel"], a["d_nsel"], a["d_slots"], a["d_sizes"], 7,
            a["d_store"], store_bytes, a["d_used"], a["d_dir"], 0, dir_entries, a["d_result"], None)


def _restore_args(alg=LZ4, max_count=1000, store_bytes=1 << 20, dst_bytes=1 << 20, dir_entries=1000, **over):
    a = dict(d_store=4096, d_dir=8192, d_ref=12288, d_raw=16384, d_count=20480, d_dst=24576, d_status=28672)
    a.update(over)
    return (alg, a["d_store"], store_bytes, a["d_dir"], 0, dir_entries, a["d_ref"], a["d_raw"], a["d_count"], max_count, a["d_dst"], dst_bytes,
            a["d_status"], None)


def test_bad_arguments_are_refused_before_the_device(cwlib):
    L = cwlib.lib()
    for alg in (LZ4, LZF):
        for name in ("d_src", "d_offsets", "d_nchunks", "d_slots", "d_sizes", "d_store", "d_used", "d_dir", "d_result"):
            assert L.cw_dev_store_chunks(*_store_args(alg, **{name: None})) == BAD_ARG, name
        assert L.cw_dev_store_chunks(*_store_args(alg, d_sel=4096)) == BAD_ARG   # half a selection
        assert L.cw_dev_store_chunks(*_store_args(alg, d_nsel=4096)) == BAD_ARG
        assert L.cw_dev_store_chunks(*_store_args(alg, max_chunks=(1 << 32) - 255)) == BAD_ARG
        assert L.cw_dev_store_chunks(*_store_args(alg, dir_entries=0)) == BAD_ARG
        for bad in (32768 + 8, 32768 + 4, 32768 + 1):
            assert L.cw_dev_store_chunks(*_store_args(alg, d_dir=bad)) == BAD_ARG
        assert L.cw_dev_store_chunks(*_store_args(alg, d_used=28672 + 4)) == BAD_ARG
        assert L.cw_dev_store_chunks(*_store_args(alg, d_result=36864 + 4)) == BAD_ARG
        for name in ("d_store", "d_dir", "d_ref", "d_raw", "d_count", "d_dst", "d_status"):
            assert L.cw_dev_restore_chunks(*_restore_args(alg, **{name: None})) == BAD_ARG, name
        assert L.cw_dev_restore_chunks(*_restore_args(alg, max_count=(1 << 32) - 255)) == BAD_ARG
        assert L.cw_dev_restore_chunks(*_restore_args(alg, dir_entries=0)) == BAD_ARG
        assert L.cw_dev_restore_chunks(*_restore_args(alg, d_dir=8192 + 8)) == BAD_ARG
    for alg in (2, 3, -1, 77):  # CW_COMP_NONE and unknown codecs
        assert L.cw_dev_store_chunks(*_store_args(alg)) == BAD_ARG
        assert L.cw_dev_restore_chunks(*_restore_args(alg)) == BAD_ARG
    assert L.cw_dev_restore_chunks(*_restore_args(d_dir=8200)) == BAD_ARG and b"16-byte aligned" in L.cw_last_error()


def test_no_gpu_means_no_store(cwlib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    L = cwlib.lib()
    for alg in (LZ4, LZF):
        assert L.cw_dev_store_chunks(*_store_args(alg)) == NO_DEVICE
        assert L.cw_dev_store_chunks(*_store_args(alg, d_sel=4096, d_nsel=8192)) == NO_DEVICE
        assert L.cw_dev_restore_chunks(*_restore_args(alg)) == NO_DEVICE
    with pytest.raises(cwlib.CwError) as e:
        cwlib.dev_restore_chunks("lz4", 4096, 1 << 20, 8192, 0, 100, 12288, 16384, 20480, 100, 24576, 1 << 20, 28672)
    assert e.value.code == NO_DEVICE
    with pytest.raises(cwlib.CwError) as e:
        cwlib.dev_store_chunks("lzf", 4096, 1 << 20, 8192, 12288, 100, 16384, 20480, 0, 24576, 1 << 20, 28672, 32768, 0, 100, 36864)
    assert e.value.code == NO_DEVICE


def _meta(asm):
    meta = asm[asm.index("amdhsa.kernels"):]
    out = {}
    for e in re.split(r"\n  - ", meta):
        m = re.search(r"\.name:\s+(\S+)", e)
        if m:
            out[m.group(1)] = e
    return out


def test_kernels_have_no_private_segment_or_spills(tmp_path):
    """restore_kernels.hip: sizes, copy and finish of the append, the restore for each codec."""
    out = str(tmp_path / "k.s")
    subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-S", "--cuda-device-only", "--offload-arch=gfx950",
                    os.path.join(ROOT, "compute_war_amd", "csrc", "restore_kernels.hip"), "-o", out], check=True, capture_output=True)
    meta = _meta(open(out).read())
    assert len(meta) == 5, sorted(meta)
    assert sum(bool(re.search(r"\d(store_sizes|store_copy|store_finish)_kernel", k)) for k in meta) == 3 and sum("restore_chunks_kernel" in k for k in meta) == 2
    for name, e in meta.items():
        assert re.search(r"\.private_segment_fixed_size:\s+0\b", e), name
        assert re.search(r"\.vgpr_spill_count:\s+0\b", e), name
        assert re.search(r"\.sgpr_spill_count:\s+0\b", e), name
    makefile = open(os.path.join(ROOT, "compute_war_amd", "csrc", "Makefile")).read()
    assert "restore_kernels.hip" in re.search(r"^SRCS\s*:=(.*)$", makefile, flags=re.M).group(1)


@pytest.mark.parametrize("alg", ["lz4", "lzf"])
def test_model_round_trips_with_the_oracle(oracle, alg):
    """The model against itself: two ingests into one store, both stored forms, every position restored; damaged entries get 1 / 2."""
    rng = np.random.default_rng(5)
    a = corpus_file("alice29.txt")[:60000] + rng.bytes(20000) + corpus_file("kennedy.xls")[:40000]
    b = a[:30000] + b"EDIT" + a[30000:]
    p = CM.default_params(1024)
    m = RM.Model(oracle, alg, 1 << 20, 400)
    cuts_a, cuts_b = CM.chunk(a, p), CM.chunk(b, p)
    refs_a, new_a, v, total_a = m.ingest(a, cuts_a, 0)
    assert v == 0 and new_a == list(range(len(cuts_a) - 1)) and total_a == len(m.blob)
    refs_b, new_b, v, _ = m.ingest(b, cuts_b, len(cuts_a) - 1)
    assert v == 0 and 0 < len(new_b) < 6 and sum(r < len(cuts_a) - 1 for r in refs_b) > len(refs_b) // 2
    words = m.directory["raw"][m.directory["raw"] != 0]
    assert (words & RM.RAW != 0).sum() >= 10 and (words & RM.RAW == 0).sum() >= 50
    assert len(m.blob) == int(m.directory["stored"].sum()) < len(a)
    for data, cuts, refs in ((a, cuts_a, refs_a), (b, cuts_b, refs_b)):
        got = RM.restore(m.blob, m.store_bytes, m.directory, 0, refs, cuts, len(data), m.decode())
        assert [s for s, _ in got] == [0] * len(refs) and b"".join(x for _, x in got) == data
    bad = m.directory.copy()
    bad[3]["pos"] = m.store_bytes
    bad[4]["raw"] ^= RM.RAW
    bad[5]["stored"] = 0
    st = [s for s, _ in RM.restore(m.blob, m.store_bytes, bad, 0, [3, 4, 5, 399, 400, RM.MISS], [cuts_a[i] for i in (3, 4, 5, 6, 7, 8, 9)],
                                   len(a), m.decode())]
    assert st[0] == 2 and st[1] in (1, 2) and st[2:] == [2, 2, 2, 2]
    # all or nothing: one byte short, one entry short
    for kw, want in ((dict(store_bytes=total_a - 1, dir_entries=400), 1), (dict(store_bytes=1 << 20, dir_entries=len(cuts_a) - 2), 2)):
        v, total, blob, entries = RM.append(a, cuts_a, new_a, RM.compressed(oracle, alg, a, cuts_a, new_a), 0, 0, kw["store_bytes"], 0,
                                            kw["dir_entries"])
        assert (v, total, blob, entries) == (want, total_a, b"", {})
