"""CPU-side checks of the dual guard: the three symbols are declared, listed, exported and mirrored, the calls refuse bad arguments
before the device -- group = 256, a d_guard_q that overlaps each other buffer, misalignments among them -- and fail loudly without a
device, and the dual guard's kernels in guard_kernels.hip compile for gfx950 without scratch memory or spills."""
import inspect
import os
import re
import subprocess

import pytest

import guard_isa
import guard_model as GM
from conftest import ROOT

NEW_SYMBOLS = ["cw_dev_store_guard2_update", "cw_dev_store_guard2_check", "cw_dev_store_guard2_rebuild"]
NO_DEVICE, BAD_ARG = -1, -2
TOO_MANY = (1 << 32) - 255
S = 65536
BAD_GEOMETRIES = [(32768, 2), (65536 + 16, 2), (3 * 65536, 2), (1 << 31, 2), (0, 2), (S, 0), (S, 257)]


@pytest.fixture(scope="module")
def cwlib():
    import compute_war_amd as cw
    if not os.path.exists(cw.lib_path()):
        subprocess.run(["make", "-C", os.path.join(ROOT, "compute_war_amd", "csrc"), "-j8"], check=True, capture_output=True)
    return cw


def test_header_declares_and_binding_lists_the_symbols(cwlib):
    from compute_war_amd import _lib
    text = open(os.path.join(ROOT, "include", "cw_hashcompress.h")).read()
    assert re.search(r"#define CW_GUARD2_MAX_GROUP 255u", text) and re.search(r"#define CW_GUARD_MAX_GROUP 256u", text)
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert set(NEW_SYMBOLS) <= set(re.findall(r"\b(cw_[a-z0-9_]+)\s*\(", text))
    assert text.index("cw_dev_store_guard_rebuild(") < text.index("cw_dev_store_guard2_update(") < text.index("cw_dev_store_guard2_check(") \
        < text.index("cw_dev_store_guard2_rebuild(") < text.index("cw_dev_alloc(")
    assert set(NEW_SYMBOLS) <= set(_lib.ABI_SYMBOLS)
    out = subprocess.run(["nm", "-D", "--defined-only", cwlib.lib_path()], capture_output=True, text=True, check=True).stdout
    assert set(NEW_SYMBOLS) <= set(re.findall(r" T (cw_[a-z0-9_]+)", out))
    for name in ("dev_store_guard2_update", "dev_store_guard2_check", "dev_store_guard2_rebuild"):
        assert hasattr(cwlib, name) and name in cwlib.__all__, name
    assert "parity" in inspect.signature(cwlib.ChunkStore.protect).parameters
    assert "detail" in inspect.signature(cwlib.ChunkStore.guard_check).parameters
    assert cwlib.ChunkStore.last_repair is None and cwlib.ChunkStore.d_guard_q is None
    makefile = open(os.path.join(ROOT, "compute_war_amd", "csrc", "Makefile")).read()
    assert "guard_kernels.hip" in re.search(r"^SRCS\s*:=(.*)$", makefile, flags=re.M).group(1)
    assert "guard2_kernels.hip" not in makefile and "guard_device.h" not in makefile
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        assert "cw_dev_store_guard2_rebuild" in open(os.path.join(ROOT, doc)).read(), doc


# Arguments with made-up non-NULL pointers: nothing dereferences them before the device is asked for.  The store ends at 2^24 + 2^20,
# P lies at 2^26 and Q at 2^26 + 2^24; 4 groups of 4 stripes need 4 stripes of each.
STORE, STORE_BYTES, GUARD_P, GUARD_Q = 1 << 24, 1 << 20, 1 << 26, (1 << 26) + (1 << 24)


def _geometry(over):
    stripe, group = over.pop("stripe", S), over.pop("group", 4)
    need = GM.guard_bytes(over.get("store_bytes", STORE_BYTES), stripe, min(group, 256)) or 4 * S
    return stripe, group, over.pop("guard_bytes", need)


def _update_args(**over):
    stripe, group, guard_bytes = _geometry(over)
    a = dict(d_store=STORE, store_bytes=STORE_BYTES, d_used=1 << 28, d_covered=(1 << 28) + 8, d_guard_p=GUARD_P, d_guard_q=GUARD_Q,
             d_result=(1 << 28) + 64)
    a.update(over)
    return (a["d_store"], a["store_bytes"], a["d_used"], a["d_covered"], stripe, group, a["d_guard_p"], a["d_guard_q"], guard_bytes, a["d_result"],
            None)


def _check_args(**over):
    stripe, group, guard_bytes = _geometry(over)
    a = dict(d_store=STORE, store_bytes=STORE_BYTES, d_covered=(1 << 28) + 8, d_guard_p=GUARD_P, d_guard_q=GUARD_Q, d_group_bad=1 << 27,
             d_result=(1 << 28) + 64)
    a.update(over)
    return (a["d_store"], a["store_bytes"], a["d_covered"], stripe, group, a["d_guard_p"], a["d_guard_q"], guard_bytes, a["d_group_bad"],
            a["d_result"], None)


def _rebuild_args(**over):
    stripe, group, guard_bytes = _geometry(over)
    a = dict(d_store=STORE, store_bytes=STORE_BYTES, d_dir=1 << 30, dir_entries=1000, d_covered=(1 << 28) + 8, d_guard_p=GUARD_P, d_guard_q=GUARD_Q,
             d_values=(1 << 27) + 4096, d_count=1 << 27, max_count=100, d_out=1 << 33, out_bytes=1 << 20, d_out_loc=1 << 31,
             d_status=(1 << 31) + (1 << 20), d_result=(1 << 28) + 64)
    a.update(over)
    return (a["d_store"], a["store_bytes"], a["d_dir"], 5, a["dir_entries"], a["d_covered"], stripe, group, a["d_guard_p"], a["d_guard_q"], guard_bytes,
            a["d_values"], a["d_count"], a["max_count"], a["d_out"], a["out_bytes"], a["d_out_loc"], a["d_status"], a["d_result"], None)


def test_bad_arguments_are_refused_before_the_device(cwlib):
    L = cwlib.lib()
    calls = ((L.cw_dev_store_guard2_update, _update_args, ("d_store", "d_used", "d_covered", "d_guard_p", "d_guard_q", "d_result"),
              ("d_used", "d_covered", "d_result")),
             (L.cw_dev_store_guard2_check, _check_args, ("d_store", "d_covered", "d_guard_p", "d_guard_q", "d_result"), ("d_covered", "d_result")),
             (L.cw_dev_store_guard2_rebuild, _rebuild_args,
              ("d_store", "d_dir", "d_covered", "d_guard_p", "d_guard_q", "d_values", "d_count", "d_out", "d_out_loc", "d_status", "d_result"),
              ("d_covered", "d_values", "d_count", "d_result")))
    for call, args, pointers, words in calls:
        for name in pointers:
            assert call(*args(**{name: None})) == BAD_ARG and b"NULL" in L.cw_last_error(), (call.__name__, name)
        for stripe, group in BAD_GEOMETRIES:
            assert call(*args(stripe=stripe, group=group)) == BAD_ARG and b"stripe" in L.cw_last_error(), (call.__name__, stripe, group)
        # the single guard's largest group is one too many
        assert call(*args(group=256, guard_bytes=1 << 20)) == BAD_ARG and b"[1, 255]" in L.cw_last_error(), call.__name__
        assert call(*args(guard_bytes=4 * S - 1)) == BAD_ARG and b"guard_bytes" in L.cw_last_error(), call.__name__
        assert call(*args(store_bytes=(1 << 20) + 1, guard_bytes=4 * S)) == BAD_ARG and b"guard_bytes" in L.cw_last_error(), call.__name__
        for name, base in (("d_store", STORE), ("d_guard_p", GUARD_P), ("d_guard_q", GUARD_Q)):
            for bad in (8, 4, 1):
                assert call(*args(**{name: base + bad})) == BAD_ARG and b"16-byte aligned" in L.cw_last_error(), (call.__name__, name)
        for name in words:
            for bad in (4, 1):
                assert call(*args(**{name: (1 << 28) + 128 + bad})) == BAD_ARG and b"8-byte aligned" in L.cw_last_error(), \
                    (call.__name__, name)
        for at in (STORE, STORE + STORE_BYTES - 16, STORE - 4 * S + 16):                              # equal, 16 bytes at either end
            assert call(*args(d_guard_p=at)) == BAD_ARG and b"d_guard overlaps d_store" in L.cw_last_error(), (call.__name__, at)
            assert call(*args(d_guard_q=at)) == BAD_ARG and b"d_guard_q overlaps d_store" in L.cw_last_error(), (call.__name__, at)
        for at in (GUARD_P, GUARD_P + 4 * S - 16, GUARD_P - 4 * S + 16):
            assert call(*args(d_guard_q=at)) == BAD_ARG and b"d_guard_q overlaps d_guard_p" in L.cw_last_error(), (call.__name__, at)
    assert L.cw_dev_store_guard2_check(*_check_args(d_group_bad=(1 << 27) + 2)) == BAD_ARG and b"4-byte aligned" in L.cw_last_error()
    # rebuild: what the single rebuild refuses as well, and a payload over either guard
    R = L.cw_dev_store_guard2_rebuild
    assert R(*_rebuild_args(max_count=TOO_MANY)) == BAD_ARG
    assert R(*_rebuild_args(dir_entries=0)) == BAD_ARG
    for bad in (8, 4, 1):
        assert R(*_rebuild_args(d_dir=(1 << 30) + bad)) == BAD_ARG and b"16-byte aligned" in L.cw_last_error()
        assert R(*_rebuild_args(d_out_loc=(1 << 31) + bad)) == BAD_ARG and b"16-byte aligned" in L.cw_last_error()
    assert R(*_rebuild_args(d_status=(1 << 31) + (1 << 20) + 2)) == BAD_ARG and b"4-byte aligned" in L.cw_last_error()
    for at in (STORE, STORE + STORE_BYTES - 1, STORE - (1 << 20) + 1):
        assert R(*_rebuild_args(d_out=at)) == BAD_ARG and b"d_out overlaps d_store" in L.cw_last_error(), at
    for name, base in (("d_guard_p", GUARD_P), ("d_guard_q", GUARD_Q)):
        for at in (base, base + 4 * S - 1, base - (1 << 20) + 1):
            assert R(*_rebuild_args(d_out=at)) == BAD_ARG and b"d_out overlaps " + name.encode() in L.cw_last_error(), (name, at)


def test_no_gpu_means_no_guard(cwlib):
    """The calls that are not refused reach the device: an empty store, no flags, the dry run, the largest geometry, adjacent buffers."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    L = cwlib.lib()
    for call, args in ((L.cw_dev_store_guard2_update, _update_args), (L.cw_dev_store_guard2_check, _check_args),
                       (L.cw_dev_store_guard2_rebuild, _rebuild_args)):
        assert call(*args()) == NO_DEVICE, call.__name__
        assert call(*args(d_store=None, store_bytes=0, guard_bytes=0)) == NO_DEVICE, call.__name__
        assert call(*args(stripe=1 << 30, group=255, guard_bytes=1 << 30, d_guard_q=1 << 40)) == NO_DEVICE, call.__name__
        assert call(*args(group=1, guard_bytes=1 << 20)) == NO_DEVICE, call.__name__
        for at in (STORE + STORE_BYTES, STORE - 4 * S, GUARD_P + 4 * S, GUARD_P - 4 * S):
            assert call(*args(d_guard_q=at)) == NO_DEVICE, (call.__name__, at)
    assert L.cw_dev_store_guard2_check(*_check_args(d_group_bad=None)) == NO_DEVICE
    assert L.cw_dev_store_guard2_rebuild(*_rebuild_args(d_out=None, out_bytes=0)) == NO_DEVICE
    assert L.cw_dev_store_guard2_rebuild(*_rebuild_args(max_count=TOO_MANY - 1)) == NO_DEVICE
    assert L.cw_dev_store_guard2_rebuild(*_rebuild_args(max_count=0)) == NO_DEVICE
    with pytest.raises(cwlib.CwError) as e:
        cwlib.dev_store_guard2_update(STORE, STORE_BYTES, 1 << 28, (1 << 28) + 8, S, 4, GUARD_P, GUARD_Q, 4 * S, (1 << 28) + 64)
    assert e.value.code == NO_DEVICE


def test_guard2_kernels_have_no_private_segment_or_spills(tmp_path):
    """guard_kernels.hip, the dual guard: fold and its finish; compare and its finish; the rebuild's count, scatter, status, fill, pair,
    copy and finish -- the Dual = true instantiations, the kernels that exist once and the two only the dual guard runs.  No kernel of
    the file has scratch memory or spills."""
    meta = dict(zip(guard_isa.DUAL, guard_isa.compiled(tmp_path, guard_isa.DUAL)))
    # the update has no tables and no LDS
    assert guard_isa.lds_bytes(meta["guard_fold_kernelILb1E"]) == 0
