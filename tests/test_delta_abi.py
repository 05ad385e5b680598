"""CPU-side checks of the recipe diff and the delta apply: the symbols are declared, listed, exported and mirrored, both calls refuse
bad arguments before the device with the argument named and fail loudly without a device, and the kernels compile without scratch
memory or spills."""
import ctypes
import os
import re
import subprocess

import pytest

import delta_model as DM
from conftest import ROOT

NEW_SYMBOLS = ["cw_dev_recipe_diff", "cw_dev_apply_delta"]
NO_DEVICE, BAD_ARG = -1, -2
HIPCC = ["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-S", "--cuda-device-only", "--offload-arch=gfx950"]
LIMIT = (1 << 32) - 256
# made up: nothing dereferences them before the device is asked for
DIFF = dict(d_ref_a=1 << 26, d_off_a=1 << 27, d_na=1 << 28, d_ref_b=1 << 29, d_off_b=1 << 30, d_nb=1 << 31, d_ops=1 << 32, d_nops=1 << 33,
            d_src=1 << 34, d_new_off=1 << 35, d_new_len=1 << 36, d_new_dst=1 << 37, d_nnew=1 << 38, d_totals=(1 << 39) + 64)
APPLY = dict(d_old=(1 << 26) + 3, d_payload=(1 << 27) + 5, d_ops=1 << 28, d_nops=1 << 29, d_dst=(1 << 30) + 7, d_result=1 << 31)


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
    assert "typedef struct cw_delta_op" in text and re.search(r"#define\s+CW_DELTA_NONE\s+UINT64_MAX", text)
    assert set(NEW_SYMBOLS) <= set(_lib.ABI_SYMBOLS)
    out = subprocess.run(["nm", "-D", "--defined-only", cwlib.lib_path()], capture_output=True, text=True, check=True).stdout
    assert set(NEW_SYMBOLS) <= set(re.findall(r" T (cw_[a-z0-9_]+)", out))
    for name in ("dev_recipe_diff", "dev_apply_delta", "DeltaOp", "DELTA_OP_DTYPE", "Diff", "Delta", "apply_delta", "DIFF_TOTALS"):
        assert hasattr(cwlib, name), name
    assert hasattr(cwlib.ChunkStore, "diff") and hasattr(cwlib.ChunkStore, "delta")
    assert hasattr(cwlib.Delta, "save") and hasattr(cwlib.Delta, "load") and hasattr(cwlib.Diff, "changed_ranges")
    full = open(os.path.join(ROOT, "include", "cw_hashcompress.h")).read()
    said = re.sub(r"[\s*]+", " ", full[full.index("cw_delta_op"):full.index("int cw_dev_recipe_diff")])
    assert "bit for bit a function of the arguments" in said


def test_the_op_is_32_bytes_and_mirrored(cwlib):
    assert ctypes.sizeof(cwlib.DeltaOp) == 32 and cwlib.DELTA_OP_DTYPE.itemsize == 32
    names = [k for k, _ in cwlib.DeltaOp._fields_]
    assert names == list(cwlib.DELTA_OP_DTYPE.names) == ["b_off", "len", "a_off", "payload_off"]
    header = open(os.path.join(ROOT, "include", "cw_hashcompress.h")).read()
    body = header[header.index("typedef struct cw_delta_op"):header.index("} cw_delta_op;")]
    assert re.findall(r"uint64_t\s+(\w+);", body) == names
    assert [getattr(cwlib.DeltaOp, k).offset for k in names] == [cwlib.DELTA_OP_DTYPE.fields[k][1] for k in names] == [0, 8, 16, 24]
    assert cwlib.DeltaOp.NONE == DM.NONE == (1 << 64) - 1
    assert list(cwlib.DIFF_TOTALS) == list(DM.TOTALS[1:])


def _diff(max_a=1000, max_b=900, dir_entries=1000, max_ops=50, **over):
    a = dict(DIFF)
    a.update(over)
    return (a["d_ref_a"], a["d_off_a"], a["d_na"], max_a, a["d_ref_b"], a["d_off_b"], a["d_nb"], max_b, 5, dir_entries, a["d_ops"], max_ops,
            a["d_nops"], a["d_src"], a["d_new_off"], a["d_new_len"], a["d_new_dst"], a["d_nnew"], a["d_totals"], None)


def _apply(old_bytes=1000, payload_bytes=100, max_ops=50, dst_bytes=2000, **over):
    a = dict(APPLY)
    a.update(over)
    return (a["d_old"], old_bytes, a["d_payload"], payload_bytes, a["d_ops"], a["d_nops"], max_ops, a["d_dst"], dst_bytes, a["d_result"], None)


def test_bad_diff_arguments_are_refused_before_the_device(cwlib):
    L = cwlib.lib()

    def refused(text, **kw):
        assert L.cw_dev_recipe_diff(*_diff(**kw)) == BAD_ARG, (text, kw)
        assert text.encode() in L.cw_last_error(), (text, L.cw_last_error())

    for name in ("d_ref_a", "d_off_a", "d_na", "d_ref_b", "d_off_b", "d_nb", "d_ops", "d_nops", "d_totals"):
        refused(name, **{name: None})
    for name in ("d_new_off", "d_new_len", "d_new_dst", "d_nnew"):                     # all four or none
        refused("go together", **{name: None})
        refused("go together", **{k: None for k in ("d_new_off", "d_new_len", "d_new_dst", "d_nnew") if k != name})
    refused("max_a", max_a=LIMIT + 1)
    refused("max_b", max_b=LIMIT + 1)
    refused("dir_entries", dir_entries=LIMIT + 1)
    refused("dir_entries", dir_entries=0)
    for name in DIFF:
        for bad in (4, 1):
            refused(name, **{name: DIFF[name] + bad})
            assert b"8-byte aligned" in L.cw_last_error()


def test_bad_apply_arguments_are_refused_before_the_device(cwlib):
    L = cwlib.lib()

    def refused(text, **kw):
        assert L.cw_dev_apply_delta(*_apply(**kw)) == BAD_ARG, (text, kw)
        assert text.encode() in L.cw_last_error(), (text, L.cw_last_error())

    for name in APPLY:
        refused(name, **{name: None})
    refused("max_ops", max_ops=LIMIT + 1)
    for name in ("d_ops", "d_nops", "d_result"):
        for bad in (4, 1):
            refused(name, **{name: APPLY[name] + bad})
            assert b"8-byte aligned" in L.cw_last_error()
    # the destination shares a byte with a source: its last byte, its first byte, all of it
    for src, size in (("d_old", "old_bytes"), ("d_payload", "payload_bytes")):
        n = 1000 if src == "d_old" else 100
        refused(f"d_dst overlaps {src}", d_dst=APPLY[src] + n - 1, **{size: n})
        refused(f"d_dst overlaps {src}", d_dst=APPLY[src] - 1999, **{size: n})
        refused(f"d_dst overlaps {src}", d_dst=APPLY[src], **{size: n})


def test_no_gpu_means_no_diff_and_no_apply(cwlib):
    """The calls that are not refused reach the device: the limits themselves, the NULL optionals, the dry run, empty buffers and
    buffers that only touch."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    L = cwlib.lib()
    assert L.cw_dev_recipe_diff(*_diff()) == NO_DEVICE
    assert L.cw_dev_recipe_diff(*_diff(max_a=LIMIT, max_b=LIMIT, dir_entries=LIMIT)) == NO_DEVICE
    assert L.cw_dev_recipe_diff(*_diff(max_a=0, max_b=0)) == NO_DEVICE
    assert L.cw_dev_recipe_diff(*_diff(d_src=None)) == NO_DEVICE
    assert L.cw_dev_recipe_diff(*_diff(d_new_off=None, d_new_len=None, d_new_dst=None, d_nnew=None)) == NO_DEVICE
    assert L.cw_dev_recipe_diff(*_diff(max_ops=0, d_ops=None)) == NO_DEVICE
    assert L.cw_dev_apply_delta(*_apply()) == NO_DEVICE
    assert L.cw_dev_apply_delta(*_apply(max_ops=LIMIT)) == NO_DEVICE
    assert L.cw_dev_apply_delta(*_apply(old_bytes=0, d_old=None, payload_bytes=0, d_payload=None, max_ops=0, d_ops=None, dst_bytes=0, d_dst=None)) == NO_DEVICE
    assert L.cw_dev_apply_delta(*_apply(d_dst=APPLY["d_old"] + 1000)) == NO_DEVICE        # behind the old bytes: no overlap
    assert L.cw_dev_apply_delta(*_apply(d_dst=APPLY["d_old"] - 2000)) == NO_DEVICE
    d, a = DIFF, APPLY
    with pytest.raises(cwlib.CwError) as e:
        cwlib.dev_recipe_diff(d["d_ref_a"], d["d_off_a"], d["d_na"], 10, d["d_ref_b"], d["d_off_b"], d["d_nb"], 10, 5, 100, d["d_ops"], 10,
                              d["d_nops"], d["d_totals"])
    assert e.value.code == NO_DEVICE
    with pytest.raises(cwlib.CwError) as e:
        cwlib.dev_apply_delta(a["d_old"], 10, a["d_payload"], 10, a["d_ops"], a["d_nops"], 10, a["d_dst"], 20, a["d_result"])
    assert e.value.code == NO_DEVICE
    with pytest.raises(cwlib.CwError) as e:
        cwlib.apply_delta(b"abc", cwlib.Delta([(0, 3, 0, DM.NONE)], b"", 3, 3))
    assert e.value.code == NO_DEVICE


def _meta(asm):
    meta = asm[asm.index("amdhsa.kernels"):]
    out = {}
    for e in re.split(r"\n  - ", meta):
        m = re.search(r"\.name:\s+(\S+)", e)
        if m:
            out[m.group(1)] = e
    return out


def test_new_kernels_have_no_private_segment_or_spills(tmp_path):
    """delta_kernels.hip: the diff's check, clear, index, source, flags and emit, the apply's check and copy."""
    out = str(tmp_path / "delta_kernels.s")
    subprocess.run(HIPCC + [os.path.join(ROOT, "compute_war_amd", "csrc", "delta_kernels.hip"), "-o", out], check=True, capture_output=True)
    meta = _meta(open(out).read())
    assert len(meta) == 8, sorted(meta)
    assert sum(bool(re.search(r"\ddiff_(check|clear|index|source|flags|emit)_kernel", k)) for k in meta) == 6
    assert sum(bool(re.search(r"\dapply_(check|copy)_kernel", k)) for k in meta) == 2
    for name, e in meta.items():
        assert re.search(r"\.private_segment_fixed_size:\s+0\b", e), name
        assert re.search(r"\.vgpr_spill_count:\s+0\b", e), name
        assert re.search(r"\.sgpr_spill_count:\s+0\b", e), name
        assert re.search(r"\.max_flat_workgroup_size:\s+(64|256)\b", e), name
    makefile = open(os.path.join(ROOT, "compute_war_amd", "csrc", "Makefile")).read()
    assert "delta_kernels.hip" in re.search(r"^SRCS\s*:=(.*)$", makefile, flags=re.M).group(1)
