"""CPU-side checks of the guard stripes: the four symbols are declared, listed, exported and mirrored, cw_store_guard_bytes gives the
model's sizes, the three device calls refuse bad arguments before the device and fail loudly without one, and the new kernels compile
for gfx950 without scratch memory or spills."""
import os
import re
import subprocess

import pytest

import guard_isa
import guard_model as GM
from conftest import ROOT

NEW_SYMBOLS = ["cw_store_guard_bytes", "cw_dev_store_guard_update", "cw_dev_store_guard_check", "cw_dev_store_guard_rebuild"]
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
    for name, value in (("MIN_STRIPE", "65536u"), ("MAX_STRIPE", r"\(1u << 30\)"), ("MAX_GROUP", "256u")):
        assert re.search(r"#define CW_GUARD_%s %s" % (name, value), text), name
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert set(NEW_SYMBOLS) <= set(re.findall(r"\b(cw_[a-z0-9_]+)\s*\(", text))
    assert text.index("cw_dev_store_replace_chunks(") < text.index("cw_store_guard_bytes(") < text.index("cw_dev_store_guard_update(") \
        < text.index("cw_dev_store_guard_check(") < text.index("cw_dev_store_guard_rebuild(") < text.index("cw_dev_alloc(")
    assert set(NEW_SYMBOLS) <= set(_lib.ABI_SYMBOLS)
    out = subprocess.run(["nm", "-D", "--defined-only", cwlib.lib_path()], capture_output=True, text=True, check=True).stdout
    assert set(NEW_SYMBOLS) <= set(re.findall(r" T (cw_[a-z0-9_]+)", out))
    for name in ("store_guard_bytes", "dev_store_guard_update", "dev_store_guard_check", "dev_store_guard_rebuild"):
        assert hasattr(cwlib, name)
    for name in ("protect", "protected_bytes", "guard_check", "repair_local"):
        assert hasattr(cwlib.ChunkStore, name)
    makefile = open(os.path.join(ROOT, "compute_war_amd", "csrc", "Makefile")).read()
    assert "guard_kernels.hip" in re.search(r"^SRCS\s*:=(.*)$", makefile, flags=re.M).group(1)
    assert "guard2_kernels.hip" not in makefile and "guard_device.h" not in makefile
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        assert "cw_dev_store_guard_rebuild" in open(os.path.join(ROOT, doc)).read(), doc


def test_guard_bytes(cwlib):
    L = cwlib.lib()
    for stripe in (S, 1 << 20, 1 << 30):
        for G in (1, 2, 3, 16, 256):
            W = G * stripe
            for n in (0, 1, W - 1, W, W + 1, 5 * W + 7):
                assert L.cw_store_guard_bytes(n, stripe, G) == GM.guard_bytes(n, stripe, G) == -(-n // W) * stripe, (n, stripe, G)
                assert cwlib.store_guard_bytes(n, stripe, G) == GM.guard_bytes(n, stripe, G)
    for stripe, G in BAD_GEOMETRIES:
        assert L.cw_store_guard_bytes(1 << 30, stripe, G) == 0 == GM.guard_bytes(1 << 30, stripe, G), (stripe, G)
        assert cwlib.store_guard_bytes(1 << 30, stripe, G) == 0
    assert cwlib.store_guard_bytes(-1, S, 2) == 0 and cwlib.store_guard_bytes(1, S, -2) == 0


# Arguments with made-up non-NULL pointers: nothing dereferences them before the device is asked for.  The store ends at 2^24 + 2^20,
# the guard lies at 2^26.
STORE, STORE_BYTES, GUARD = 1 << 24, 1 << 20, 1 << 26


def _geometry(over):
    stripe, group = over.pop("stripe", S), over.pop("group", 4)
    need = GM.guard_bytes(over.get("store_bytes", STORE_BYTES), stripe, group) or 4 * S
    return stripe, group, over.pop("guard_bytes", need)


def _update_args(**over):
    stripe, group, guard_bytes = _geometry(over)
    a = dict(d_store=STORE, store_bytes=STORE_BYTES, d_used=1 << 28, d_covered=(1 << 28) + 8, d_guard=GUARD, d_result=(1 << 28) + 64)
    a.update(over)
    return (a["d_store"], a["store_bytes"], a["d_used"], a["d_covered"], stripe, group, a["d_guard"], guard_bytes, a["d_result"], None)


def _check_args(**over):
    stripe, group, guard_bytes = _geometry(over)
    a = dict(d_store=STORE, store_bytes=STORE_BYTES, d_covered=(1 << 28) + 8, d_guard=GUARD, d_group_bad=1 << 27, d_result=(1 << 28) + 64)
    a.update(over)
    return (a["d_store"], a["store_bytes"], a["d_covered"], stripe, group, a["d_guard"], guard_bytes, a["d_group_bad"], a["d_result"], None)


def _rebuild_args(**over):
    stripe, group, guard_bytes = _geometry(over)
    a = dict(d_store=STORE, store_bytes=STORE_BYTES, d_dir=1 << 30, dir_entries=1000, d_covered=(1 << 28) + 8, d_guard=GUARD, d_values=(1 << 27) + 4096,
             d_count=1 << 27, max_count=100, d_out=1 << 33, out_bytes=1 << 20, d_out_loc=1 << 31, d_status=(1 << 31) + (1 << 20),
             d_result=(1 << 28) + 64)
    a.update(over)
    return (a["d_store"], a["store_bytes"], a["d_dir"], 5, a["dir_entries"], a["d_covered"], stripe, group, a["d_guard"], guard_bytes, a["d_values"],
            a["d_count"], a["max_count"], a["d_out"], a["out_bytes"], a["d_out_loc"], a["d_status"], a["d_result"], None)


def test_bad_arguments_are_refused_before_the_device(cwlib):
    L = cwlib.lib()
    calls = ((L.cw_dev_store_guard_update, _update_args, ("d_store", "d_used", "d_covered", "d_guard", "d_result"), ("d_used", "d_covered", "d_result")),
             (L.cw_dev_store_guard_check, _check_args, ("d_store", "d_covered", "d_guard", "d_result"), ("d_covered", "d_result")),
             (L.cw_dev_store_guard_rebuild, _rebuild_args,
              ("d_store", "d_dir", "d_covered", "d_guard", "d_values", "d_count", "d_out", "d_out_loc", "d_status", "d_result"),
              ("d_covered", "d_values", "d_count", "d_result")))
    for call, args, pointers, words in calls:
        for name in pointers:
            assert call(*args(**{name: None})) == BAD_ARG and b"NULL" in L.cw_last_error(), (call.__name__, name)
        for stripe, group in BAD_GEOMETRIES:
            assert call(*args(stripe=stripe, group=group)) == BAD_ARG and b"stripe" in L.cw_last_error(), (call.__name__, stripe, group)
        # the guard: one byte short of what the store needs; 4 groups of 4 stripes need 4 stripes
        assert call(*args(guard_bytes=4 * S - 1)) == BAD_ARG and b"guard_bytes" in L.cw_last_error(), call.__name__
        assert call(*args(store_bytes=(1 << 20) + 1, guard_bytes=4 * S)) == BAD_ARG and b"guard_bytes" in L.cw_last_error(), call.__name__
        for name in ("d_store", "d_guard"):
            for bad in (8, 4, 1):
                base = STORE if name == "d_store" else GUARD
                assert call(*args(**{name: base + bad})) == BAD_ARG and b"16-byte aligned" in L.cw_last_error(), (call.__name__, name)
        for name in words:
            for bad in (4, 1):
                assert call(*args(**{name: (1 << 28) + 128 + bad})) == BAD_ARG and b"8-byte aligned" in L.cw_last_error(), \
                    (call.__name__, name)
        for at in (STORE, STORE + STORE_BYTES - 16, STORE - 4 * S + 16):                              # equal, 16 bytes at either end
            assert call(*args(d_guard=at)) == BAD_ARG and b"d_guard overlaps d_store" in L.cw_last_error(), (call.__name__, at)
    assert L.cw_dev_store_guard_check(*_check_args(d_group_bad=(1 << 27) + 2)) == BAD_ARG and b"4-byte aligned" in L.cw_last_error()
    # rebuild: what the export refuses as well
    assert L.cw_dev_store_guard_rebuild(*_rebuild_args(max_count=TOO_MANY)) == BAD_ARG
    assert L.cw_dev_store_guard_rebuild(*_rebuild_args(dir_entries=0)) == BAD_ARG
    for bad in (8, 4, 1):
        assert L.cw_dev_store_guard_rebuild(*_rebuild_args(d_dir=(1 << 30) + bad)) == BAD_ARG and b"16-byte aligned" in L.cw_last_error()
        assert L.cw_dev_store_guard_rebuild(*_rebuild_args(d_out_loc=(1 << 31) + bad)) == BAD_ARG and b"16-byte aligned" in L.cw_last_error()
    assert L.cw_dev_store_guard_rebuild(*_rebuild_args(d_status=(1 << 31) + (1 << 20) + 2)) == BAD_ARG and b"4-byte aligned" in L.cw_last_error()
    for at in (STORE, STORE + STORE_BYTES - 1, STORE - (1 << 20) + 1):
        assert L.cw_dev_store_guard_rebuild(*_rebuild_args(d_out=at)) == BAD_ARG and b"d_out overlaps d_store" in L.cw_last_error(), at
    for at in (GUARD, GUARD + 4 * S - 1, GUARD - (1 << 20) + 1):
        assert L.cw_dev_store_guard_rebuild(*_rebuild_args(d_out=at)) == BAD_ARG and b"d_out overlaps d_guard" in L.cw_last_error(), at


def test_no_gpu_means_no_guard(cwlib):
    """The calls that are not refused reach the device: an empty store, no flags, the dry run, the largest geometry, adjacent buffers."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    L = cwlib.lib()
    for call, args in ((L.cw_dev_store_guard_update, _update_args), (L.cw_dev_store_guard_check, _check_args),
                       (L.cw_dev_store_guard_rebuild, _rebuild_args)):
        assert call(*args()) == NO_DEVICE, call.__name__
        assert call(*args(d_store=None, store_bytes=0, guard_bytes=0)) == NO_DEVICE, call.__name__
        assert call(*args(stripe=1 << 30, group=256, guard_bytes=1 << 30)) == NO_DEVICE, call.__name__
        assert call(*args(group=1, guard_bytes=1 << 20)) == NO_DEVICE, call.__name__
        for at in (STORE + STORE_BYTES, STORE - 4 * S):
            assert call(*args(d_guard=at)) == NO_DEVICE, (call.__name__, at)
    assert L.cw_dev_store_guard_check(*_check_args(d_group_bad=None)) == NO_DEVICE
    assert L.cw_dev_store_guard_rebuild(*_rebuild_args(d_out=None, out_bytes=0)) == NO_DEVICE
    assert L.cw_dev_store_guard_rebuild(*_rebuild_args(max_count=TOO_MANY - 1)) == NO_DEVICE
    assert L.cw_dev_store_guard_rebuild(*_rebuild_args(max_count=0)) == NO_DEVICE
    with pytest.raises(cwlib.CwError) as e:
        cwlib.dev_store_guard_update(STORE, STORE_BYTES, 1 << 28, (1 << 28) + 8, S, 4, GUARD, 4 * S, (1 << 28) + 64)
    assert e.value.code == NO_DEVICE


def test_guard_kernels_have_no_private_segment_or_spills(tmp_path):
    """guard_kernels.hip, the single guard: fold and its finish; compare and its finish; the rebuild's count, scatter, status, copy and
    finish -- the Dual = false instantiations and the kernels that exist once.  No kernel of the file has scratch memory or spills."""
    meta = dict(zip(guard_isa.SINGLE, guard_isa.compiled(tmp_path, guard_isa.SINGLE)))
    # the update has no LDS, and the single copy none of the dual copy's field tables
    assert guard_isa.lds_bytes(meta["guard_fold_kernelILb0E"]) == 0
    assert guard_isa.lds_bytes(meta["rebuild_copy_kernelILb0E"]) == 0
