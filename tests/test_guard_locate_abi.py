"""CPU-side checks of the guard's locate calls: the two symbols are declared, ordered, listed, exported and mirrored, the documents
name them, the calls refuse bad arguments before the device and fail loudly without one, ChunkStore has guard_locate, heal and
scrub(values=), and guard_locate_kernels.hip compiles for gfx950 without scratch memory or spills."""
import inspect
import os
import re
import subprocess

import pytest

import guard_model as GM
from conftest import ROOT

NEW_SYMBOLS = ["cw_dev_store_guard_locate", "cw_dev_store_guard2_locate"]
NO_DEVICE, BAD_ARG = -1, -2
TOO_MANY = (1 << 32) - 255
S = 65536
BAD_GEOMETRIES = [(32768, 2), (65536 + 16, 2), (3 * 65536, 2), (1 << 31, 2), (0, 2), (S, 0), (S, 257)]
HIPCC = ["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-S", "--cuda-device-only", "--offload-arch=gfx950"]
KERNELS = ("locate_sweep_kernelILb0E", "locate_sweep_kernelILb1E", "locate_entries_kernelILb0E", "locate_entries_kernelILb1E", "locate_finish_kernelE")


@pytest.fixture(scope="module")
def cwlib():
    import compute_war_amd as cw
    if not os.path.exists(cw.lib_path()):
        subprocess.run(["make", "-C", os.path.join(ROOT, "compute_war_amd", "csrc"), "-j8"], check=True, capture_output=True)
    return cw


def test_header_declares_and_binding_lists_the_symbols(cwlib):
    from compute_war_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cw_hashcompress.h")).read(), flags=re.S)
    assert set(NEW_SYMBOLS) <= set(re.findall(r"\b(cw_[a-z0-9_]+)\s*\(", text))
    assert text.index("cw_dev_store_guard2_rebuild(") < text.index("cw_dev_store_guard_locate(") < text.index("cw_dev_store_guard2_locate(") \
        < text.index("cw_dev_alloc(")
    assert set(NEW_SYMBOLS) <= set(_lib.ABI_SYMBOLS)
    out = subprocess.run(["nm", "-D", "--defined-only", cwlib.lib_path()], capture_output=True, text=True, check=True).stdout
    assert set(NEW_SYMBOLS) <= set(re.findall(r" T (cw_[a-z0-9_]+)", out))
    for name in ("dev_store_guard_locate", "dev_store_guard2_locate", "GuardSuspects"):
        assert hasattr(cwlib, name) and name in cwlib.__all__, name
    makefile = open(os.path.join(ROOT, "compute_war_amd", "csrc", "Makefile")).read()
    srcs = re.search(r"^SRCS\s*:=(.*)$", makefile, flags=re.M).group(1)
    assert "guard_locate_kernels.hip" in srcs and "guard_kernels.hip" in srcs and "guard_sums.h" in re.search(r"^HDRS\s*:=(.*)$", makefile, flags=re.M).group(1)
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        body = open(os.path.join(ROOT, doc)).read()
        assert all(name in body for name in NEW_SYMBOLS), doc


def test_store_methods(cwlib):
    CS = cwlib.ChunkStore
    assert list(inspect.signature(CS.guard_locate).parameters) == ["self"]
    heal = inspect.signature(CS.heal).parameters
    assert list(heal) == ["self", "verify"] and heal["verify"].default is True
    scrub = inspect.signature(CS.scrub).parameters
    assert list(scrub) == ["self", "keep", "values"] and scrub["keep"].default is None and scrub["values"].default is None
    import numpy as np
    g = cwlib.GuardSuspects(np.array([0, 1, 2, 3, 4, 0], np.uint32), dict(groups=1), 1000)
    assert g.located.tolist() == [1001, 1003] and g.ambiguous.tolist() == [1002, 1003] and g.unprotected.tolist() == [1004]
    assert g.suspects.tolist() == [1001, 1002, 1003] and g.status.dtype == np.uint32 and g.totals == dict(groups=1)


# Arguments with made-up non-NULL pointers: nothing dereferences them before the device is asked for.  The store ends at 2^24 + 2^20,
# P lies at 2^26 and Q at 2^26 + 2^24; 4 groups of 4 stripes need 4 stripes of each.
STORE, STORE_BYTES, GUARD_P, GUARD_Q = 1 << 24, 1 << 20, 1 << 26, (1 << 26) + (1 << 24)


def _args(dual, **over):
    stripe, group = over.pop("stripe", S), over.pop("group", 4)
    need = GM.guard_bytes(over.get("store_bytes", STORE_BYTES), stripe, min(group, 256)) or 4 * S
    guard_bytes = over.pop("guard_bytes", need)
    a = dict(d_store=STORE, store_bytes=STORE_BYTES, d_dir=1 << 30, dir_entries=1000, d_covered=(1 << 28) + 8, d_guard_p=GUARD_P, d_guard_q=GUARD_Q,
             d_suspect=1 << 27, d_result=(1 << 28) + 64)
    a.update(over)
    guards = (a["d_guard_p"], a["d_guard_q"]) if dual else (a["d_guard_p"],)
    return (a["d_store"], a["store_bytes"], a["d_dir"], 5, a["dir_entries"], a["d_covered"], stripe, group) + guards + \
        (guard_bytes, a["d_suspect"], a["d_result"], None)


def _calls(L):
    return ((L.cw_dev_store_guard_locate, False, ("d_store", "d_dir", "d_covered", "d_guard_p", "d_suspect", "d_result")),
            (L.cw_dev_store_guard2_locate, True, ("d_store", "d_dir", "d_covered", "d_guard_p", "d_guard_q", "d_suspect", "d_result")))


def test_bad_arguments_are_refused_before_the_device(cwlib):
    L = cwlib.lib()
    for call, dual, pointers in _calls(L):
        args = lambda **over: _args(dual, **over)  # noqa: E731
        for name in pointers:
            assert call(*args(**{name: None})) == BAD_ARG and b"NULL" in L.cw_last_error(), (call.__name__, name)
        # what the check calls refuse
        for stripe, group in BAD_GEOMETRIES:
            assert call(*args(stripe=stripe, group=group)) == BAD_ARG and b"stripe" in L.cw_last_error(), (call.__name__, stripe, group)
        assert call(*args(guard_bytes=4 * S - 1)) == BAD_ARG and b"guard_bytes" in L.cw_last_error(), call.__name__
        assert call(*args(store_bytes=(1 << 20) + 1, guard_bytes=4 * S)) == BAD_ARG and b"guard_bytes" in L.cw_last_error(), call.__name__
        for name, base in (("d_store", STORE), ("d_guard_p", GUARD_P)) + ((("d_guard_q", GUARD_Q),) if dual else ()):
            for bad in (8, 4, 1):
                assert call(*args(**{name: base + bad})) == BAD_ARG and b"16-byte aligned" in L.cw_last_error(), (call.__name__, name)
        for name in ("d_covered", "d_result"):
            for bad in (4, 1):
                assert call(*args(**{name: (1 << 28) + 128 + bad})) == BAD_ARG and b"8-byte aligned" in L.cw_last_error(), (call.__name__, name)
        for at in (STORE, STORE + STORE_BYTES - 16, STORE - 4 * S + 16):                              # equal, 16 bytes at either end
            assert call(*args(d_guard_p=at)) == BAD_ARG and b"d_guard overlaps d_store" in L.cw_last_error(), (call.__name__, at)
        if dual:
            assert call(*args(group=256, guard_bytes=1 << 20)) == BAD_ARG and b"[1, 255]" in L.cw_last_error()
            for at in (STORE, STORE + STORE_BYTES - 16, STORE - 4 * S + 16):
                assert call(*args(d_guard_q=at)) == BAD_ARG and b"d_guard_q overlaps d_store" in L.cw_last_error(), at
            for at in (GUARD_P, GUARD_P + 4 * S - 16, GUARD_P - 4 * S + 16):
                assert call(*args(d_guard_q=at)) == BAD_ARG and b"d_guard_q overlaps d_guard_p" in L.cw_last_error(), at
        # the calls' own
        assert call(*args(dir_entries=0)) == BAD_ARG and b"dir_entries is 0" in L.cw_last_error(), call.__name__
        assert call(*args(dir_entries=TOO_MANY)) == BAD_ARG and b"dir_entries" in L.cw_last_error(), call.__name__
        for bad in (8, 4, 1):
            assert call(*args(d_dir=(1 << 30) + bad)) == BAD_ARG and b"d_dir is not 16-byte aligned" in L.cw_last_error(), call.__name__
        for bad in (2, 1, 3):
            assert call(*args(d_suspect=(1 << 27) + bad)) == BAD_ARG and b"d_suspect is not 4-byte aligned" in L.cw_last_error(), call.__name__


def test_no_gpu_means_no_locate(cwlib):
    """The calls that are not refused reach the device: an empty store, the largest geometries and directory, a d_suspect at 4 mod 8."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    L = cwlib.lib()
    for call, dual, _ in _calls(L):
        args = lambda **over: _args(dual, **over)  # noqa: E731
        assert call(*args()) == NO_DEVICE, call.__name__
        assert call(*args(d_store=None, store_bytes=0, guard_bytes=0)) == NO_DEVICE, call.__name__
        assert call(*args(stripe=1 << 30, group=255, guard_bytes=1 << 30, d_guard_q=1 << 40)) == NO_DEVICE, call.__name__
        assert call(*args(group=1, guard_bytes=1 << 20)) == NO_DEVICE, call.__name__
        assert call(*args(dir_entries=TOO_MANY - 1)) == NO_DEVICE, call.__name__
        assert call(*args(dir_entries=1)) == NO_DEVICE, call.__name__
        assert call(*args(d_suspect=(1 << 27) + 4)) == NO_DEVICE, call.__name__
    assert L.cw_dev_store_guard_locate(*_args(False, group=256, guard_bytes=1 << 20)) == NO_DEVICE
    for wrapper, dual in ((cwlib.dev_store_guard_locate, False), (cwlib.dev_store_guard2_locate, True)):
        with pytest.raises(cwlib.CwError) as e:
            wrapper(*_args(dual)[:-1])
        assert e.value.code == NO_DEVICE


def test_locate_kernels_have_no_private_segment_or_spills(tmp_path):
    """guard_locate_kernels.hip: the sweep and the entries kernel in both instantiations and the finish.  From the metadata alone: no
    kernel has scratch memory or spills, and the single guard's instantiations hold no tables."""
    out = str(tmp_path / "guard_locate_kernels.s")
    subprocess.run(HIPCC + [os.path.join(ROOT, "compute_war_amd", "csrc", "guard_locate_kernels.hip"), "-o", out], check=True, capture_output=True)
    asm = open(out).read()
    meta = {}
    for e in re.split(r"\n  - ", asm[asm.index("amdhsa.kernels"):]):
        m = re.search(r"\.name:\s+(\S+)", e)
        if m:
            meta[m.group(1)] = e
    assert len(meta) == len(KERNELS), sorted(meta)
    for name in KERNELS:
        hits = [e for k, e in meta.items() if re.search(r"\d" + name, k)]
        assert len(hits) == 1, name
        e = hits[0]
        assert re.search(r"\.private_segment_fixed_size:\s+0\b", e), name
        assert re.search(r"\.vgpr_spill_count:\s+0\b", e), name
        assert re.search(r"\.sgpr_spill_count:\s+0\b", e), name
        lds = int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", e).group(1))
        vgprs = int(re.search(r"\.vgpr_count:\s+(\d+)", e).group(1))
        print(f"{name}: {vgprs} VGPRs, {lds} bytes of LDS")
        assert lds < 64 if "ILb0E" in name else lds <= 256 + 64, name
