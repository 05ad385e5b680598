"""CPU-side checks of cw_dev_cdc_resync_windows, cw_dev_scatter_extents and cw_store_compose: the symbols are declared, listed, exported
and mirrored, cw_compose_stats and cw_resync_window have the header's size and field order in ctypes and numpy, every refused argument
is refused before the device with a message that names it, the calls fail loudly without a device, ``edit`` refuses what ``patch_many``
refuses, and the kernels of compose_kernels.hip compile without scratch memory or spills."""
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
NONE = (1 << 64) - 1
STATS = ["windows", "rounds", "merged_windows", "rebuilt_bytes", "rebuilt_chunks", "new_chunks", "stored_bytes", "kept_positions"]
WINDOW = ["new_from", "shift", "old_first", "old_count", "final"]
SYMBOLS = ("cw_dev_cdc_resync_windows", "cw_dev_scatter_extents", "cw_store_compose")


@pytest.fixture(scope="module")
def cwlib():
    import compute_war_amd as cw
    if not os.path.exists(cw.lib_path()):
        subprocess.run(["make", "-C", os.path.join(ROOT, "compute_war_amd", "csrc"), "-j8"], check=True, capture_output=True)
    return cw


def _header():
    return open(os.path.join(ROOT, "include", "cw_hashcompress.h")).read()


def test_header_declares_and_binding_lists_the_symbols(cwlib):
    from compute_war_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    declared = re.findall(r"\b(cw_[a-z0-9_]+)\s*\(", text)
    out = subprocess.run(["nm", "-D", "--defined-only", cwlib.lib_path()], capture_output=True, text=True, check=True).stdout
    exported = re.findall(r" T (cw_[a-z0-9_]+)", out)
    for sym in SYMBOLS:
        assert sym in declared and sym in _lib.ABI_SYMBOLS and sym in exported, sym
    # a section of its own behind cw_dev_apply_delta
    assert text.index("cw_dev_apply_delta(") < text.index("cw_dev_cdc_resync_windows(") < text.index("cw_dev_scatter_extents(") \
        < text.index("cw_store_compose(") < text.index("cw_dev_store_export_chunks(")
    for name in ("dev_cdc_resync_windows", "dev_scatter_extents", "store_compose", "ResyncWindow", "ComposeStats", "COMPOSE_DTYPE"):
        assert hasattr(cwlib, name) and name in cwlib.__all__, name
    for name in ("compose", "apply_delta", "concat", "edit", "last_compose"):
        assert hasattr(cwlib.ChunkStore, name), name


def _fields(struct):
    header = _header()
    body = header[header.index("typedef struct " + struct):header.index("} " + struct + ";")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert "uint32_t" not in body and body.count("uint64_t") == 1
    return re.findall(r"\b([a-z_]+)\s*[,;]", body[body.index("uint64_t"):])


def test_compose_stats_and_resync_window_are_mirrored(cwlib):
    from compute_war_amd import ops
    assert _fields("cw_compose_stats") == STATS and _fields("cw_resync_window") == WINDOW
    assert ctypes.sizeof(cwlib.ComposeStats) == 64 and cwlib.COMPOSE_DTYPE.itemsize == 64
    assert [k for k, _ in cwlib.ComposeStats._fields_] == list(cwlib.COMPOSE_DTYPE.names) == STATS
    assert [getattr(cwlib.ComposeStats, k).offset for k in STATS] == [cwlib.COMPOSE_DTYPE.fields[k][1] for k in STATS] == list(range(0, 64, 8))
    s = cwlib.ComposeStats(*range(1, 9))
    assert s.as_dict() == dict(zip(STATS, range(1, 9)))
    assert np.frombuffer(bytes(s), cwlib.COMPOSE_DTYPE)[0].tolist() == tuple(range(1, 9))
    assert ctypes.sizeof(cwlib.ResyncWindow) == 40 and ops.RESYNC_WINDOW_DTYPE.itemsize == 40
    assert [k for k, _ in cwlib.ResyncWindow._fields_] == list(ops.RESYNC_WINDOW_DTYPE.names) == WINDOW
    assert [getattr(cwlib.ResyncWindow, k).offset for k in WINDOW] == [ops.RESYNC_WINDOW_DTYPE.fields[k][1] for k in WINDOW] == list(range(0, 40, 8))


# ---- the two device steps (made-up non-NULL pointers: nothing dereferences them before the device is asked for) ---------------------
def _windows(max_new=100, nwin=3, max_old=100, **over):
    a = dict(d_new_offsets=4096, d_new_count=8192, d_stream_first=12288, d_win=16384, d_old_offsets=20480, d_result=24576)
    a.update(over)
    return (a["d_new_offsets"], a["d_new_count"], max_new, a["d_stream_first"], a["d_win"], nwin, a["d_old_offsets"], max_old, a["d_result"], None)


def test_resync_windows_refuses_bad_arguments_before_the_device(cwlib):
    import torch
    L = cwlib.lib()
    for name in ("d_new_offsets", "d_new_count", "d_stream_first", "d_win", "d_old_offsets", "d_result"):
        assert L.cw_dev_cdc_resync_windows(*_windows(**{name: None})) == BAD_ARG, name
        assert name.encode() in L.cw_last_error(), name
        for bad in (4, 1, 7):
            assert L.cw_dev_cdc_resync_windows(*_windows(**{name: 4096 * 9 + bad})) == BAD_ARG, name
            assert b"8-byte aligned" in L.cw_last_error()
    for key in ("max_new", "max_old", "nwin"):
        assert L.cw_dev_cdc_resync_windows(*_windows(**{key: LIMIT + 1})) == BAD_ARG and key.encode() in L.cw_last_error()
    if not torch.cuda.is_available():
        for kw in (dict(), dict(max_new=LIMIT, max_old=LIMIT, nwin=LIMIT), dict(max_new=0), dict(max_old=0, d_old_offsets=None), dict(nwin=0)):
            assert L.cw_dev_cdc_resync_windows(*_windows(**kw)) == NO_DEVICE, kw


SCATTER = dict(d_src=1 << 20, src_bytes=5000, d_ext=4096, d_n=8192, max_n=10, d_dst=2 << 20, dst_bytes=7000, d_result=12288)


def _scatter(**over):
    a = dict(SCATTER)
    a.update(over)
    return (a["d_src"], a["src_bytes"], a["d_ext"], a["d_n"], a["max_n"], a["d_dst"], a["dst_bytes"], a["d_result"], None)


def test_scatter_extents_refuses_bad_arguments_before_the_device(cwlib):
    import torch
    L = cwlib.lib()
    for name in ("d_src", "d_ext", "d_n", "d_dst", "d_result"):
        assert L.cw_dev_scatter_extents(*_scatter(**{name: None})) == BAD_ARG, name
        assert name.encode() in L.cw_last_error(), name
    for name in ("d_ext", "d_n", "d_result"):
        for bad in (4, 1, 7):
            assert L.cw_dev_scatter_extents(*_scatter(**{name: 4096 * 9 + bad})) == BAD_ARG, name
            assert b"8-byte aligned" in L.cw_last_error()
    assert L.cw_dev_scatter_extents(*_scatter(max_n=LIMIT + 1)) == BAD_ARG and b"max_n" in L.cw_last_error()
    for d_dst in (SCATTER["d_src"], SCATTER["d_src"] + 4999, SCATTER["d_src"] - 6999):
        assert L.cw_dev_scatter_extents(*_scatter(d_dst=d_dst)) == BAD_ARG and b"overlaps" in L.cw_last_error()
    if not torch.cuda.is_available():
        for kw in (dict(), dict(max_n=LIMIT), dict(max_n=0, d_ext=None), dict(src_bytes=0, d_src=None), dict(dst_bytes=0, d_dst=None),
                   dict(d_dst=SCATTER["d_src"] + 5000), dict(d_dst=SCATTER["d_src"] - 7000), dict(d_src=(1 << 20) + 3, d_dst=(2 << 20) + 1)):
            assert L.cw_dev_scatter_extents(*_scatter(**kw)) == NO_DEVICE, kw


# ---- cw_store_compose -----------------------------------------------------------------------------------------------------------------
class _Call:
    """A cw_store_compose call over a made-up store and a real host recipe of ten 1000-byte chunks in two streams of six and four;
    ``over`` replaces arguments."""

    def __init__(self, cw):
        self.cw = cw
        self.params = cw.CdcParams(64, 256, 2048)
        self.store = cw.Store(4096, 1 << 20, 8192, 12288, 0, 1000)
        self.refs = np.arange(10, dtype=np.uint64)
        self.offsets = np.arange(11, dtype=np.uint64) * np.uint64(1000)
        self.first = np.array([0, 6, 10], np.uint64)
        self.ops = self.op_list([(0, 2500, 500, NONE), (2500, 300, NONE, 0), (2800, 7000, 3000, NONE)])
        self.payload = np.zeros(300, np.uint8)
        self.out_refs, self.out_offsets = np.zeros(400, np.uint64), np.zeros(400, np.uint64)
        self.k, self.stats = ctypes.c_size_t(77), cw.ComposeStats()

    def op_list(self, ops):
        self.keep = np.array(ops, dtype=self.cw.DELTA_OP_DTYPE)
        return self.keep

    def __call__(self, **over):
        a = dict(x=4096, p=ctypes.addressof(self.params), alg=LZ4, st=ctypes.addressof(self.store), refs=self.refs.ctypes.data,
                 offsets=self.offsets.ctypes.data, nchunks=10, first=self.first.ctypes.data, nstreams=2, ops=self.ops.ctypes.data, nops=3,
                 payload=self.payload.ctypes.data, payload_bytes=300, base=10, lookahead=0, out_refs=self.out_refs.ctypes.data,
                 out_offsets=self.out_offsets.ctypes.data, max_out=400, out_nchunks=ctypes.addressof(self.k), stats=ctypes.addressof(self.stats))
        a.update(over)
        L = self.cw.lib()
        rc = L.cw_store_compose(a["x"], a["p"], a["alg"], a["st"], a["refs"], a["offsets"], a["nchunks"], a["first"], a["nstreams"], a["ops"],
                                a["nops"], a["payload"], a["payload_bytes"], a["base"], a["lookahead"], a["out_refs"], a["out_offsets"], a["max_out"],
                                a["out_nchunks"], a["stats"])
        return rc, L.cw_last_error().decode()


def test_compose_refuses_bad_arguments_before_the_device(cwlib):
    import torch
    call = _Call(cwlib)
    total = 2500 + 300 + 7000
    cases = [(dict(x=None), "index"), (dict(p=None), "param"), (dict(st=None), "store"), (dict(refs=None), "refs"), (dict(offsets=None), "offsets"),
             (dict(ops=None), "ops"), (dict(out_refs=None), "out_refs"), (dict(out_offsets=None), "out_offsets"), (dict(out_nchunks=None), "out_nchunks"),
             (dict(payload=None), "payload"), (dict(alg=2), "compression algorithm 2"), (dict(alg=77), "compression algorithm 77"),
             (dict(max_out=total // 64 + 1), "max_out"), (dict(base=(1 << 64) - 10), "base")]
    for over, word in cases:
        rc, msg = call(**over)
        assert rc == BAD_ARG and word in msg, (over, msg)
        assert call.k.value == 0 or over.get("out_nchunks", 1) is None
        call.k.value = 77
    # what cw_store_ingest refuses of the parameters, and the store's own checks
    for params, word in ((cwlib.CdcParams(2048, 8192, 131072), "max_size"), (cwlib.CdcParams(32, 256, 2048), "min 32")):
        rc, msg = call(p=ctypes.addressof(params))
        assert rc == BAD_ARG and word in msg, msg
    for store, word in ((cwlib.Store(4096, 1 << 20, 8192, 12288 + 8, 0, 1000), "16-byte"), (cwlib.Store(4096, 1 << 20, 8192 + 4, 12288, 0, 1000), "8-byte"),
                        (cwlib.Store(4096, 1 << 20, 8192, 12288, 0, 0), "dir_entries"), (cwlib.Store(4096, 1 << 20, None, 12288, 0, 1000), "NULL")):
        rc, msg = call(st=ctypes.addressof(store))
        assert rc == BAD_ARG and word in msg, msg
    # the op list, by apply_check's rule: the lowest bad op is named
    good = [(0, 2500, 500, NONE), (2500, 300, NONE, 0), (2800, 7000, 3000, NONE)]
    bad_ops = [((1, 2500, 500, NONE), 0, "start"), ((2501, 300, NONE, 0), 1, "start"), ((2500, 0, NONE, 0), 1, "len 0"),
               ((2500, (1 << 64) - 100, NONE, 0), 1, "wraps"), ((2500, 300, 10, 0), 1, "both"), ((2500, 300, NONE, NONE), 1, "neither"),
               ((2500, 300, 9701, NONE), 1, "source"), ((2500, 300, (1 << 64) - 2, NONE), 1, "source"), ((2500, 300, NONE, 1), 1, "payload"),
               ((2800, 7000, 3001, NONE), 2, "source")]
    for bad, at, word in bad_ops:
        ops = list(good)
        ops[at] = bad
        arr = call.op_list(ops)
        rc, msg = call(ops=arr.ctypes.data)
        assert rc == BAD_ARG and f"op {at} " in msg and word in msg, (bad, msg)
    arr = call.op_list([(0, 0, 0, NONE), (5, 0, NONE, NONE), good[2]])
    rc, msg = call(ops=arr.ctypes.data)
    assert rc == BAD_ARG and "op 0 " in msg, msg                          # two bad ops: the lower
    # the stream index
    for first, word in (([1, 6, 10], "start"), ([0, 7, 6], "decrease"), ([0, 6, 9], "nchunks"), ([0, 6, 11], "nchunks")):
        arr = np.array(first, np.uint64)
        rc, msg = call(first=arr.ctypes.data)
        assert rc == BAD_ARG and "stream_first" in msg and word in msg, (first, msg)
    # offsets that decrease in a range a copy names, and a recipe that ends below its start
    bad = call.offsets.copy()
    bad[4] = 2900
    rc, msg = call(offsets=bad.ctypes.data)
    assert rc == BAD_ARG and "offsets" in msg and "3" in msg, msg
    bad = call.offsets.copy()
    bad[10], bad[0] = 0, 5
    rc, msg = call(offsets=bad.ctypes.data)
    assert rc == BAD_ARG and "offsets" in msg, msg
    # nops == 0: the empty recipe, without a device
    call.out_offsets[0] = 99
    rc, msg = call(nops=0, ops=None)
    assert rc == 0 and call.k.value == 0 and call.out_offsets[0] == 0 and call.stats.windows == 0
    rc, msg = call(nops=0, ops=None, max_out=1)
    assert rc == BAD_ARG and "max_out" in msg
    if not torch.cuda.is_available():
        only_new = call.op_list([(0, 300, NONE, 0)])
        for over in (dict(), dict(stats=None), dict(first=None, nstreams=0), dict(alg=LZF), dict(lookahead=1), dict(max_out=total // 64 + 2),
                     dict(ops=only_new.ctypes.data, nops=1, refs=None, nchunks=0, first=None), dict(ops=only_new.ctypes.data, nops=1, max_out=300 // 64 + 2)):
            rc, msg = call(**over)
            assert rc == NO_DEVICE, (over, msg)


def test_no_gpu_means_no_compose(cwlib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(cwlib.CwError) as e:
        cwlib.dev_cdc_resync_windows(4096, 8192, 10, 12288, 16384, 2, 20480, 10, 24576)
    assert e.value.code == NO_DEVICE
    with pytest.raises(cwlib.CwError) as e:
        cwlib.dev_scatter_extents(1 << 20, 100, 4096, 8192, 3, 2 << 20, 100, 12288)
    assert e.value.code == NO_DEVICE
    index = object.__new__(cwlib.DedupeIndex)
    index._x = lambda: 4096
    with pytest.raises(cwlib.CwError) as e:
        cwlib.store_compose(index, cwlib.CdcParams(64, 256, 2048), "lz4", cwlib.Store(4096, 1 << 20, 8192, 12288, 0, 1000), [1, 2], [0, 700, 1500],
                            np.array([(0, 1000, 200, NONE), (1000, 3, NONE, 0)], dtype=cwlib.DELTA_OP_DTYPE), b"abc", 2)
    assert e.value.code == NO_DEVICE
    cs = object.__new__(cwlib.ChunkStore)   # (a store cannot be made without a device: the methods ask for one first)
    recipe = cwlib.Recipe([0, 1], [0, 700, 1500])
    delta = cwlib.Delta(np.array([(0, 1500, 0, NONE)], dtype=cwlib.DELTA_OP_DTYPE), b"", 1500, 1500)
    for call in (lambda: cs.compose([(recipe, 10, 500), b"abc"]), lambda: cs.concat([recipe, recipe]), lambda: cs.apply_delta(recipe, delta),
                 lambda: cs.edit(recipe, [(0, 1, b"a"), (700, 0, b"b")])):
        with pytest.raises(cwlib.CwError) as e:
            call()
        assert e.value.code == NO_DEVICE


def test_edit_refuses_what_patch_many_refuses_before_any_device_work(cwlib):
    cs = object.__new__(cwlib.ChunkStore)
    recipe = cwlib.Recipe([0, 1], [0, 700, 1500])
    for edits in ([(0, 10, b""), (9, 1, b"")], [(100, 0, b"a"), (100, 5, b"b")], [(5, 0, b"a"), (0, 6, b"")], [(0, 1501, b"")], [(1500, 1, b"")]):
        with pytest.raises(ValueError):
            cs.patch_many(recipe, edits)
        with pytest.raises(ValueError):
            cs.edit(recipe, edits)
    with pytest.raises(ValueError):
        cs.compose([(recipe, 1000, 501)])


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
    """compose_kernels.hip: the windows' search and finish, the scatter's check and copy."""
    out = str(tmp_path / "k.s")
    subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-S", "--cuda-device-only", "--offload-arch=gfx950",
                    os.path.join(ROOT, "compute_war_amd", "csrc", "compose_kernels.hip"), "-o", out], check=True, capture_output=True)
    meta = _meta(open(out).read())
    assert len(meta) == 4, sorted(meta)
    for kernel in ("windows_search_kernel", "windows_finish_kernel", "scatter_check_kernel", "scatter_copy_kernel"):
        assert sum(kernel in k for k in meta) == 1, kernel
    for name, e in meta.items():
        assert re.search(r"\.private_segment_fixed_size:\s+0\b", e), name
        assert re.search(r"\.vgpr_spill_count:\s+0\b", e), name
        assert re.search(r"\.sgpr_spill_count:\s+0\b", e), name
    makefile = open(os.path.join(ROOT, "compute_war_amd", "csrc", "Makefile")).read()
    assert "compose_kernels.hip" in re.search(r"^SRCS\s*:=(.*)$", makefile, flags=re.M).group(1)
