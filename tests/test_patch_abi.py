"""CPU-side checks of cw_dev_cdc_resync and cw_store_patch: the symbols are declared, listed, exported and mirrored, cw_patch_stats has
the header's size and field order in ctypes and numpy, every refused argument is refused before the device with a message that names
it, the calls fail loudly without a device, and the kernels of patch_kernels.hip compile without scratch memory or spills."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

LZ4, LZF = 0, 1
NO_DEVICE, BAD_ARG = -1, -2
LIMIT = (1 << 32) - 256
FIELDS = ["window_bytes", "window_chunks", "new_chunks", "stored_bytes", "attempts", "first_position", "resume_position", "reused_positions"]


@pytest.fixture(scope="module")
def cwlib():
    import compute_war_amd as cw
    if not os.path.exists(cw.lib_path()):
        subprocess.run(["make", "-C", os.path.join(ROOT, "compute_war_amd", "csrc"), "-j8"], check=True, capture_output=True)
    return cw


def test_header_declares_and_binding_lists_the_symbols(cwlib):
    from compute_war_amd import _lib
    header = open(os.path.join(ROOT, "include", "cw_hashcompress.h")).read()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = re.findall(r"\b(cw_[a-z0-9_]+)\s*\(", text)
    out = subprocess.run(["nm", "-D", "--defined-only", cwlib.lib_path()], capture_output=True, text=True, check=True).stdout
    exported = re.findall(r" T (cw_[a-z0-9_]+)", out)
    for sym in ("cw_dev_cdc_resync", "cw_store_patch"):
        assert sym in declared and sym in _lib.ABI_SYMBOLS and sym in exported, sym
    assert text.index("cw_store_ingest(") < text.index("cw_store_patch(") < text.index("cw_dev_store_mark(")   # beside cw_store_ingest
    for name in ("dev_cdc_resync", "store_patch", "PatchStats", "PATCH_DTYPE"):
        assert hasattr(cwlib, name) and name in cwlib.__all__, name
    for name in ("patch", "write", "append", "truncate", "patch_many", "last_patch"):
        assert hasattr(cwlib.ChunkStore, name), name


def test_patch_stats_is_mirrored(cwlib):
    header = open(os.path.join(ROOT, "include", "cw_hashcompress.h")).read()
    body = header[header.index("typedef struct cw_patch_stats"):header.index("} cw_patch_stats;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"\b([a-z_]+)\s*[,;]", body[body.index("uint64_t"):]) == FIELDS
    assert "uint32_t" not in body and body.count("uint64_t") == 1
    assert ctypes.sizeof(cwlib.PatchStats) == 64 and cwlib.PATCH_DTYPE.itemsize == 64
    assert [k for k, _ in cwlib.PatchStats._fields_] == list(cwlib.PATCH_DTYPE.names) == FIELDS
    assert [getattr(cwlib.PatchStats, k).offset for k in FIELDS] == [cwlib.PATCH_DTYPE.fields[k][1] for k in FIELDS] == list(range(0, 64, 8))
    s = cwlib.PatchStats(*range(1, 9))
    assert s.as_dict() == dict(zip(FIELDS, range(1, 9)))
    assert np.frombuffer(bytes(s), cwlib.PATCH_DTYPE)[0].tolist() == tuple(range(1, 9))


# ---- cw_dev_cdc_resync ------------------------------------------------------------------------------------------------------------
def _resync(max_new=100, max_old=100, keep_all=0, **over):
    """Arguments with made-up non-NULL pointers (nothing dereferences them before the device is asked for)."""
    a = dict(d_new_offsets=4096, d_new_count=8192, d_old_offsets=12288, d_old_count=16384, d_result=20480)
    a.update(over)
    return (a["d_new_offsets"], a["d_new_count"], max_new, a["d_old_offsets"], a["d_old_count"], max_old, 5, (1 << 64) - 3, keep_all, a["d_result"],
            None)


def test_resync_refuses_bad_arguments_before_the_device(cwlib):
    import torch
    L = cwlib.lib()
    for name in ("d_new_offsets", "d_new_count", "d_old_offsets", "d_old_count", "d_result"):
        assert L.cw_dev_cdc_resync(*_resync(**{name: None})) == BAD_ARG, name
        assert name.encode() in L.cw_last_error(), name
        for bad in (4, 1, 7):
            assert L.cw_dev_cdc_resync(*_resync(**{name: 4096 * 9 + bad})) == BAD_ARG, name
            assert b"8-byte aligned" in L.cw_last_error()
    assert L.cw_dev_cdc_resync(*_resync(max_new=LIMIT + 1)) == BAD_ARG and b"max_new" in L.cw_last_error()
    assert L.cw_dev_cdc_resync(*_resync(max_old=LIMIT + 1)) == BAD_ARG and b"max_old" in L.cw_last_error()
    for bad in (2, -1):
        assert L.cw_dev_cdc_resync(*_resync(keep_all=bad)) == BAD_ARG and b"keep_all" in L.cw_last_error()
    if not torch.cuda.is_available():
        for kw in (dict(), dict(max_new=LIMIT, max_old=LIMIT), dict(max_new=0), dict(max_old=0), dict(keep_all=1)):
            assert L.cw_dev_cdc_resync(*_resync(**kw)) == NO_DEVICE, kw


# ---- cw_store_patch -----------------------------------------------------------------------------------------------------------------
class _Call:
    """A cw_store_patch call over a made-up store and a real host recipe of ten 1000-byte chunks; ``over`` replaces arguments."""

    def __init__(self, cw):
        self.cw = cw
        self.params = cw.CdcParams(64, 256, 2048)
        self.store = cw.Store(4096, 1 << 20, 8192, 12288, 0, 1000)
        self.refs = np.arange(10, dtype=np.uint64)
        self.offsets = np.arange(11, dtype=np.uint64) * np.uint64(1000)
        self.insert = np.zeros(500, np.uint8)
        self.out_refs, self.out_offsets = np.zeros(400, np.uint64), np.zeros(400, np.uint64)
        self.k, self.stats = ctypes.c_size_t(77), cw.PatchStats()

    def __call__(self, **over):
        a = dict(x=4096, p=ctypes.addressof(self.params), alg=LZ4, st=ctypes.addressof(self.store), refs=self.refs.ctypes.data,
                 offsets=self.offsets.ctypes.data, nchunks=10, edit_off=2500, remove=300, insert=self.insert.ctypes.data, insert_bytes=500,
                 base=10, lookahead=0, out_refs=self.out_refs.ctypes.data, out_offsets=self.out_offsets.ctypes.data, max_out=400,
                 out_nchunks=ctypes.addressof(self.k), stats=ctypes.addressof(self.stats))
        a.update(over)
        L = self.cw.lib()
        rc = L.cw_store_patch(a["x"], a["p"], a["alg"], a["st"], a["refs"], a["offsets"], a["nchunks"], a["edit_off"], a["remove"], a["insert"],
                              a["insert_bytes"], a["base"], a["lookahead"], a["out_refs"], a["out_offsets"], a["max_out"], a["out_nchunks"], a["stats"])
        return rc, L.cw_last_error().decode()


def test_patch_refuses_bad_arguments_before_the_device(cwlib):
    import torch
    call = _Call(cwlib)
    cases = [(dict(x=None), "index"), (dict(p=None), "param"), (dict(st=None), "store"), (dict(refs=None), "refs"), (dict(offsets=None), "offsets"),
             (dict(out_refs=None), "out_refs"), (dict(out_offsets=None), "out_offsets"), (dict(out_nchunks=None), "out_nchunks"),
             (dict(insert=None), "insert"), (dict(alg=2), "compression algorithm 2"), (dict(alg=77), "compression algorithm 77"),
             (dict(edit_off=9800, remove=300), "edit_off"), (dict(edit_off=10001, remove=0), "edit_off"),
             (dict(edit_off=5, remove=(1 << 64) - 2), "remove_bytes"), (dict(edit_off=(1 << 64) - 1, remove=2), "edit_off"),
             (dict(max_out=(10000 - 300 + 500) // 64 + 1), "max_out"), (dict(base=(1 << 64) - 10), "base")]
    for over, word in cases:
        rc, msg = call(**over)
        assert rc == BAD_ARG and word in msg, (over, msg)
        assert call.k.value == 0 or over.get("out_nchunks", 1) is None
        call.k.value = 77
    # what cw_store_ingest refuses of the parameters: a max_size no chunk of which could be stored, a min_size below 64
    for params, word in ((cwlib.CdcParams(2048, 8192, 131072), "max_size"), (cwlib.CdcParams(32, 256, 2048), "min 32")):
        rc, msg = call(p=ctypes.addressof(params))
        assert rc == BAD_ARG and word in msg, msg
    # the store's own checks
    for store, word in ((cwlib.Store(4096, 1 << 20, 8192, 12288 + 8, 0, 1000), "16-byte"), (cwlib.Store(4096, 1 << 20, 8192 + 4, 12288, 0, 1000), "8-byte"),
                        (cwlib.Store(4096, 1 << 20, 8192, 12288, 0, 0), "dir_entries"), (cwlib.Store(4096, 1 << 20, None, 12288, 0, 1000), "NULL")):
        rc, msg = call(st=ctypes.addressof(store))
        assert rc == BAD_ARG and word in msg, msg
    # offsets that decrease inside the located window, and a recipe that ends below its start
    bad = call.offsets.copy()
    bad[4] = 2900
    rc, msg = call(offsets=bad.ctypes.data)
    assert rc == BAD_ARG and "offsets" in msg and "3" in msg, msg
    bad = call.offsets.copy()
    bad[10] = 0
    bad[0] = 5
    rc, msg = call(offsets=bad.ctypes.data)
    assert rc == BAD_ARG and "offsets" in msg, msg
    if not torch.cuda.is_available():
        # not refused: no stats, no insert, an empty recipe, an edit at either end, a decrease outside the window, the smallest max_out
        far = call.offsets.copy()
        far[1] = 999999
        for over in (dict(), dict(stats=None), dict(insert=None, insert_bytes=0), dict(nchunks=0, refs=None, edit_off=0, remove=0),
                     dict(edit_off=0, remove=0), dict(edit_off=10000, remove=0), dict(edit_off=0, remove=10000), dict(alg=LZF),
                     dict(offsets=far.ctypes.data, edit_off=9000, remove=10, lookahead=1), dict(max_out=(10000 - 300 + 500) // 64 + 2)):
            rc, msg = call(**over)
            assert rc == NO_DEVICE, (over, msg)


def test_no_gpu_means_no_patch(cwlib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(cwlib.CwError) as e:
        cwlib.dev_cdc_resync(4096, 8192, 10, 12288, 16384, 10, 0, -3, False, 20480)
    assert e.value.code == NO_DEVICE
    index = object.__new__(cwlib.DedupeIndex)
    index._x = lambda: 4096
    with pytest.raises(cwlib.CwError) as e:
        cwlib.store_patch(index, cwlib.CdcParams(64, 256, 2048), "lz4", cwlib.Store(4096, 1 << 20, 8192, 12288, 0, 1000), [1, 2], [0, 700, 1500], 100,
                          50, b"abc", 2)
    assert e.value.code == NO_DEVICE
    cs = object.__new__(cwlib.ChunkStore)   # (a store cannot be made without a device: the methods ask for one first)
    recipe = cwlib.Recipe([0, 1], [0, 700, 1500])
    for edit in (lambda: cs.patch(recipe, 10, 5, b"abc"), lambda: cs.write(recipe, 1400, b"x" * 300), lambda: cs.append(recipe, b"tail"),
                 lambda: cs.truncate(recipe, 100), lambda: cs.patch_many(recipe, [(0, 1, b"a"), (700, 0, b"b")])):
        with pytest.raises(cwlib.CwError) as e:
            edit()
        assert e.value.code == NO_DEVICE


def test_patch_many_refuses_overlapping_edits_before_any_runs(cwlib):
    cs = object.__new__(cwlib.ChunkStore)
    recipe = cwlib.Recipe([0, 1], [0, 700, 1500])
    for edits in ([(0, 10, b""), (9, 1, b"")], [(100, 0, b"a"), (100, 5, b"b")], [(5, 0, b"a"), (0, 6, b"")], [(0, 1501, b"")], [(1500, 1, b"")]):
        with pytest.raises(ValueError):
            cs.patch_many(recipe, edits)


# ---- the kernels --------------------------------------------------------------------------------------------------------------------
def _meta(asm):
    meta = asm[asm.index("amdhsa.kernels"):]
    out = {}
    for e in re.split(r"\n  - ", meta):
        m = re.search(r"\.name:\s+(\S+)", e)
        if m:
            out[m.group(1)] = e
    return out


def test_kernels_have_no_private_segment_or_spills(tmp_path):
    """patch_kernels.hip: the search and the finish."""
    out = str(tmp_path / "k.s")
    subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-S", "--cuda-device-only", "--offload-arch=gfx950",
                    os.path.join(ROOT, "compute_war_amd", "csrc", "patch_kernels.hip"), "-o", out], check=True, capture_output=True)
    meta = _meta(open(out).read())
    assert len(meta) == 2, sorted(meta)
    assert sum("resync_search_kernel" in k for k in meta) == 1 and sum("resync_finish_kernel" in k for k in meta) == 1
    for name, e in meta.items():
        assert re.search(r"\.private_segment_fixed_size:\s+0\b", e), name
        assert re.search(r"\.vgpr_spill_count:\s+0\b", e), name
        assert re.search(r"\.sgpr_spill_count:\s+0\b", e), name
    makefile = open(os.path.join(ROOT, "compute_war_amd", "csrc", "Makefile")).read()
    assert "patch_kernels.hip" in re.search(r"^SRCS\s*:=(.*)$", makefile, flags=re.M).group(1)
