"""CPU-side checks of mark, compact and retain: the three symbols are declared, listed, exported and mirrored, the calls refuse bad
arguments before the device and fail loudly without one, the kernels compile without scratch memory or spills, and the
plain-Python model drops a stream and keeps two with the CPU oracle's codecs."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import cdc_model as CM
import restore_model as RM
import store_gc_model as GM
from conftest import ROOT, corpus_file

NEW_SYMBOLS = ["cw_dev_store_mark", "cw_dev_store_compact", "cw_dedupe_retain"]
NO_DEVICE, BAD_ARG = -1, -2
HIPCC = ["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-S", "--cuda-device-only", "--offload-arch=gfx950"]


@pytest.fixture(scope="module")
def cwlib():
    import compute_war_amd as cw
    if not os.path.exists(cw.lib_path()):
        subprocess.run(["make", "-C", os.path.join(ROOT, "compute_war_amd", "csrc"), "-j8"], check=True, capture_output=True)
    return cw


def test_header_declares_and_binding_lists_the_symbols(cwlib):
    from compute_war_amd import _lib
    text = open(os.path.join(ROOT, "include", "cw_hashcompress.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert set(NEW_SYMBOLS) <= set(re.findall(r"\b(cw_[a-z0-9_]+)\s*\(", text))
    assert set(NEW_SYMBOLS) <= set(_lib.ABI_SYMBOLS)
    out = subprocess.run(["nm", "-D", "--defined-only", cwlib.lib_path()], capture_output=True, text=True, check=True).stdout
    assert set(NEW_SYMBOLS) <= set(re.findall(r" T (cw_[a-z0-9_]+)", out))
    for name in ("dev_store_mark", "dev_store_compact"):
        assert hasattr(cwlib, name)
    assert hasattr(cwlib.ChunkStore, "compact") and hasattr(cwlib.DedupeIndex, "retain")


def _mark_args(max_count=1000, dir_entries=1000, **over):
    """Arguments of cw_dev_store_mark with made-up non-NULL pointers (nothing dereferences them before the device is asked for)."""
    a = dict(d_ref=4096, d_count=8192, d_live=12288, d_n_outside=16384)
    a.update(over)
    return (a["d_ref"], a["d_count"], max_count, 5, dir_entries, a["d_live"], a["d_n_outside"], None)


def _compact_args(store_bytes=1 << 20, new_store_bytes=1 << 20, dir_entries=1000, **over):
    a = dict(d_store=1 << 24, d_dir=1 << 26, d_live=1 << 27, d_new_store=1 << 28, d_new_used=1 << 30, d_new_dir=1 << 29, d_result=(1 << 30) + 64)
    a.update(over)
    return (a["d_store"], store_bytes, a["d_dir"], dir_entries, a["d_live"], a["d_new_store"], new_store_bytes, a["d_new_used"], a["d_new_dir"],
            a["d_result"], None)


def test_bad_arguments_are_refused_before_the_device(cwlib):
    L = cwlib.lib()
    for name in ("d_ref", "d_count", "d_live", "d_n_outside"):
        assert L.cw_dev_store_mark(*_mark_args(**{name: None})) == BAD_ARG, name
    assert L.cw_dev_store_mark(*_mark_args(max_count=(1 << 32) - 255)) == BAD_ARG
    assert L.cw_dev_store_mark(*_mark_args(dir_entries=0)) == BAD_ARG
    assert L.cw_dev_store_mark(*_mark_args(d_n_outside=16384 + 4)) == BAD_ARG and b"8-byte aligned" in L.cw_last_error()

    for name in ("d_store", "d_dir", "d_live", "d_new_store", "d_new_used", "d_new_dir", "d_result"):
        assert L.cw_dev_store_compact(*_compact_args(**{name: None})) == BAD_ARG, name
    assert L.cw_dev_store_compact(*_compact_args(dir_entries=0)) == BAD_ARG
    for bad in (8, 4, 1):
        assert L.cw_dev_store_compact(*_compact_args(d_dir=(1 << 26) + bad)) == BAD_ARG
        assert L.cw_dev_store_compact(*_compact_args(d_new_dir=(1 << 29) + bad)) == BAD_ARG
    assert L.cw_dev_store_compact(*_compact_args(d_new_used=(1 << 30) + 4)) == BAD_ARG
    assert L.cw_dev_store_compact(*_compact_args(d_result=(1 << 30) + 68)) == BAD_ARG
    # the new store overlapping the old one: equal, one byte at either end
    for new in (1 << 24, (1 << 24) + (1 << 20) - 1, (1 << 24) - (1 << 20) + 1):
        assert L.cw_dev_store_compact(*_compact_args(d_new_store=new)) == BAD_ARG and b"overlaps d_store" in L.cw_last_error(), new
    # a new directory overlapping the old one without being it: one entry at either end
    for new in ((1 << 26) + 16 * 999, (1 << 26) - 16 * 999, (1 << 26) + 16):
        assert L.cw_dev_store_compact(*_compact_args(d_new_dir=new)) == BAD_ARG and b"overlaps d_dir" in L.cw_last_error(), new

    # retain: a made-up handle too (these are refused before the device is asked for, and the handle is only read behind that)
    assert L.cw_dedupe_retain(None, 4096, 0, 100, 0, None) == BAD_ARG
    assert L.cw_dedupe_retain(8192, None, 0, 100, 0, None) == BAD_ARG
    assert L.cw_dedupe_retain(8192, 4096, 0, 0, 0, None) == BAD_ARG
    assert L.cw_dedupe_retain(8192, 4096, 0, 100, (1 << 40) + 1, None) == BAD_ARG and b"2^40" in L.cw_last_error()


def test_no_gpu_means_no_compaction(cwlib):
    """The calls that are not refused reach the device: the neighbours of the overlap cases, the dry run and the equal directory."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    L = cwlib.lib()
    assert L.cw_dev_store_mark(*_mark_args()) == NO_DEVICE
    assert L.cw_dev_store_mark(*_mark_args(max_count=(1 << 32) - 256)) == NO_DEVICE
    assert L.cw_dev_store_compact(*_compact_args()) == NO_DEVICE
    for new in ((1 << 24) + (1 << 20), (1 << 24) - (1 << 20)):                          # adjacent stores
        assert L.cw_dev_store_compact(*_compact_args(d_new_store=new)) == NO_DEVICE
    for new in ((1 << 26) + 16 * 1000, (1 << 26) - 16 * 1000):                          # adjacent directories
        assert L.cw_dev_store_compact(*_compact_args(d_new_dir=new)) == NO_DEVICE
    assert L.cw_dev_store_compact(*_compact_args(d_new_dir=1 << 26)) == NO_DEVICE          # the directory in place
    assert L.cw_dev_store_compact(*_compact_args(d_new_store=None, new_store_bytes=0)) == NO_DEVICE   # the dry run
    assert L.cw_dev_store_compact(*_compact_args(d_store=None, store_bytes=0)) == NO_DEVICE
    assert L.cw_dev_store_compact(*_compact_args(d_new_store=1 << 24, new_store_bytes=0)) == NO_DEVICE  # an empty range overlaps nothing
    with pytest.raises(cwlib.CwError) as e:
        cwlib.dev_store_mark(4096, 8192, 100, 0, 100, 12288, 16384)
    assert e.value.code == NO_DEVICE
    with pytest.raises(cwlib.CwError) as e:
        cwlib.dev_store_compact(1 << 24, 1 << 20, 1 << 26, 100, 1 << 27, 0, 0, 1 << 30, 1 << 26, (1 << 30) + 64)
    assert e.value.code == NO_DEVICE
    assert L.cw_dedupe_retain(8192, 4096, 0, 100, 1 << 40, None) == NO_DEVICE


def _meta(asm):
    meta = asm[asm.index("amdhsa.kernels"):]
    out = {}
    for e in re.split(r"\n  - ", meta):
        m = re.search(r"\.name:\s+(\S+)", e)
        if m:
            out[m.group(1)] = e
    return out


def _no_scratch(name, e):
    assert re.search(r"\.private_segment_fixed_size:\s+0\b", e), name
    assert re.search(r"\.vgpr_spill_count:\s+0\b", e), name
    assert re.search(r"\.sgpr_spill_count:\s+0\b", e), name


def test_gc_kernels_have_no_private_segment_or_spills(tmp_path):
    """store_gc_kernels.hip: the mark, and sizes, copy and finish of the compaction."""
    out = str(tmp_path / "k.s")
    subprocess.run(HIPCC + [os.path.join(ROOT, "compute_war_amd", "csrc", "store_gc_kernels.hip"), "-o", out], check=True, capture_output=True)
    meta = _meta(open(out).read())
    assert len(meta) == 4, sorted(meta)
    assert sum(bool(re.search(r"\d(store_mark|gc_sizes|gc_copy|gc_finish)_kernel", k)) for k in meta) == 4
    for name, e in meta.items():
        _no_scratch(name, e)
    makefile = open(os.path.join(ROOT, "compute_war_amd", "csrc", "Makefile")).read()
    assert "store_gc_kernels.hip" in re.search(r"^SRCS\s*:=(.*)$", makefile, flags=re.M).group(1)


def test_retain_kernel_claims_with_the_64_bit_cas_and_has_no_scratch(tmp_path):
    out = str(tmp_path / "d.s")
    subprocess.run(HIPCC + [os.path.join(ROOT, "compute_war_amd", "csrc", "dedupe_kernels.hip"), "-o", out], check=True, capture_output=True)
    asm = open(out).read()
    meta = {k: e for k, e in _meta(asm).items() if "dedupe_retain_kernel" in k}
    assert len(meta) == 3, sorted(meta)                       # 16-, 32- and 64-byte digests
    for name, e in meta.items():
        _no_scratch(name, e)
    bodies = {m.group(1): m.group(2) for m in re.finditer(r"^(_Z\S+):[^\n]*\n(.*?)^\.Lfunc_end", asm, flags=re.M | re.S)}
    for name in meta:
        assert "global_atomic_cmpswap_x2" in bodies[name], name
        assert len(re.findall(r"^\s*global_atomic_add_x2", bodies[name], flags=re.M)) == 1, name    # the kept count: one per workgroup


@pytest.mark.parametrize("alg", ["lz4", "lzf"])
def test_model_drops_one_stream_of_three(oracle, alg):
    """Three streams into one Model, the first and the third kept: both restore from the compacted blob and directory, the second is
    refused exactly where only it had a chunk."""
    a, b, c = GM.three_streams(corpus_file("alice29.txt"), corpus_file("kennedy.xls"))
    p = CM.default_params(1024)
    m = RM.Model(oracle, alg, 1 << 20, 512)
    base, streams = 0, []
    for data in (a, b, c):
        cuts = CM.chunk(data, p)
        refs, new, v, _ = m.ingest(data, cuts, base)
        assert v == 0
        streams.append((data, cuts, refs, [base + i for i in new]))
        base += len(cuts) - 1
    (_, _, refs_a, _), (_, cuts_b, refs_b, new_b), (_, _, refs_c, new_c) = streams
    live, outside = GM.mark(refs_a, 0, 512)
    live, outside = GM.mark(refs_c, 0, 512, live, outside)
    assert outside == 0
    only_b = sorted(set(refs_b) - set(refs_a) - set(refs_c))
    # the kept and the dropped sets are not trivial: b has chunks of its own, shares chunks with the kept streams, c has its own too
    assert 0 < len(only_b) < 8 and only_b == new_b and len(set(refs_b) & set(refs_a)) > 50 and 0 < len(new_c) < 8
    verdict, result, blob, new_dir = GM.compact(m.blob, m.store_bytes, m.directory, live, 1 << 20)
    n_entries = int(np.count_nonzero(m.directory["raw"]))
    assert verdict == 0 and result == [0, len(blob), n_entries - len(only_b), len(only_b)]
    kept = new_dir[new_dir["raw"] != 0]
    assert len(blob) == int(kept["stored"].sum()) < len(m.blob)
    assert (kept["raw"] & RM.RAW != 0).sum() >= 10 and (kept["raw"] & RM.RAW == 0).sum() >= 50      # both stored forms are kept
    assert [int(i) for i in np.nonzero((m.directory["raw"] != 0) & (new_dir["raw"] == 0))[0]] == only_b
    for data, cuts, refs, _ in (streams[0], streams[2]):
        got = RM.restore(blob, len(blob), new_dir, 0, refs, cuts, len(data), m.decode())
        assert [s for s, _ in got] == [0] * len(refs) and b"".join(x for _, x in got) == data
    st = [s for s, _ in RM.restore(blob, len(blob), new_dir, 0, refs_b, cuts_b, len(b), m.decode())]
    assert st == [2 if r in only_b else 0 for r in refs_b] and st.count(2) == len(only_b)
    values = GM.retain(m.values, live, 0, 512)
    assert len(values) == len(m.values) - len(only_b) and set(m.values.values()) - set(values.values()) == set(only_b)
    # all or nothing in the model too; a flag on a zero entry keeps nothing; an unsound entry matters only when it is kept
    assert GM.compact(m.blob, m.store_bytes, m.directory, live, len(blob) - 1) == (1, [1, len(blob), result[2], result[3]], None, None)
    live2 = live.copy()
    live2[500] = 1
    assert GM.compact(m.blob, m.store_bytes, m.directory, live2, 1 << 20)[1] == result
    bad = m.directory.copy()
    bad[only_b[0]]["stored"] = 0
    assert GM.compact(m.blob, m.store_bytes, bad, live, 1 << 20)[1] == result
    bad[refs_a[0]]["pos"] = m.store_bytes
    assert GM.compact(m.blob, m.store_bytes, bad, live, 1 << 20)[0] == 2
    assert GM.mark([3, 4, 515, 516, RM.MISS], 4, 512)[1] == 3
