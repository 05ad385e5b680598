"""CPU-side checks of the account call: the symbol is declared, listed, exported and mirrored, the call refuses bad arguments before
the device with the argument named and fails loudly without a device, the kernels compile without scratch memory or spills, and the
numpy model agrees with the plain loop on random small cases that reach every branch."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import account_model as AM
from conftest import ROOT

NEW_SYMBOLS = ["cw_dev_store_account"]
NO_DEVICE, BAD_ARG = -1, -2
HIPCC = ["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-S", "--cuda-device-only", "--offload-arch=gfx950"]
LIMIT, STREAM_LIMIT = (1 << 32) - 256, (1 << 32) - 258
POINTERS = dict(d_ref=1 << 26, d_first=1 << 27, d_dir=1 << 28, d_flag=1 << 29, d_acct=1 << 30, d_refcount=1 << 31, d_owner=1 << 32,
                d_totals=(1 << 33) + 64)      # made up: nothing dereferences them before the device is asked for


@pytest.fixture(scope="module")
def cwlib():
    import compute_war_amd as cw
    if not os.path.exists(cw.lib_path()):
        subprocess.run(["make", "-C", os.path.join(ROOT, "compute_war_amd", "csrc"), "-j8"], check=True, capture_output=True)
    return cw


def test_header_declares_and_binding_lists_the_symbol(cwlib):
    from compute_war_amd import _lib
    text = open(os.path.join(ROOT, "include", "cw_hashcompress.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert set(NEW_SYMBOLS) <= set(re.findall(r"\b(cw_[a-z0-9_]+)\s*\(", text))
    assert "typedef struct cw_stream_account" in text and "CW_OWNER_NONE" in text and "CW_OWNER_SHARED" in text
    assert set(NEW_SYMBOLS) <= set(_lib.ABI_SYMBOLS)
    out = subprocess.run(["nm", "-D", "--defined-only", cwlib.lib_path()], capture_output=True, text=True, check=True).stdout
    assert set(NEW_SYMBOLS) <= set(re.findall(r" T (cw_[a-z0-9_]+)", out))
    for name in ("dev_store_account", "StreamAccount", "ACCOUNT_DTYPE", "Account"):
        assert hasattr(cwlib, name), name
    assert hasattr(cwlib.ChunkStore, "account") and hasattr(cwlib.ChunkStore, "affected")


def test_the_struct_is_64_bytes_and_mirrored(cwlib):
    assert ctypes.sizeof(cwlib.StreamAccount) == 64 and cwlib.ACCOUNT_DTYPE.itemsize == 64
    names = [k for k, _ in cwlib.StreamAccount._fields_]
    assert names == list(cwlib.ACCOUNT_DTYPE.names) == list(AM.FIELDS) == list(AM.ACCOUNT.names)
    header = open(os.path.join(ROOT, "include", "cw_hashcompress.h")).read()
    body = header[header.index("typedef struct cw_stream_account"):header.index("} cw_stream_account;")]
    assert re.findall(r"uint64_t\s+(\w+);", body) == names
    assert [getattr(cwlib.StreamAccount, k).offset for k in names] == [cwlib.ACCOUNT_DTYPE.fields[k][1] for k in names] == list(range(0, 64, 8))
    assert (cwlib.StreamAccount.OWNER_NONE, cwlib.StreamAccount.OWNER_SHARED) == (cwlib.Account.NONE, cwlib.Account.SHARED) == (AM.NONE, AM.SHARED)
    assert re.search(r"#define\s+CW_OWNER_NONE\s+0xFFFFFFFFu", header) and re.search(r"#define\s+CW_OWNER_SHARED\s+0xFFFFFFFEu", header)


def _args(nstreams=36, max_positions=1000, dir_entries=1000, **over):
    a = dict(POINTERS)
    a.update(over)
    return (a["d_ref"], a["d_first"], nstreams, max_positions, a["d_dir"], 5, dir_entries, a["d_flag"], a["d_acct"], a["d_refcount"],
            a["d_owner"], a["d_totals"], None)


def test_bad_arguments_are_refused_before_the_device(cwlib):
    L = cwlib.lib()

    def refused(text, *args, **kw):
        assert L.cw_dev_store_account(*_args(*args, **kw)) == BAD_ARG, (text, kw)
        assert text.encode() in L.cw_last_error(), (text, L.cw_last_error())

    for name in ("d_ref", "d_first", "d_dir", "d_acct", "d_totals"):
        refused(name, **{name: None})
    refused("nstreams", nstreams=0)
    refused("nstreams", nstreams=STREAM_LIMIT + 1)
    refused("max_positions", max_positions=LIMIT + 1)
    refused("dir_entries", dir_entries=0)
    refused("dir_entries", dir_entries=LIMIT + 1)
    for bad in (8, 4, 1):
        refused("d_dir", d_dir=POINTERS["d_dir"] + bad)
        assert b"16-byte aligned" in L.cw_last_error()
    for name in ("d_ref", "d_first", "d_acct", "d_totals"):
        for bad in (4, 1):
            refused(name, **{name: POINTERS[name] + bad})
            assert b"8-byte aligned" in L.cw_last_error()


def test_no_gpu_means_no_account(cwlib):
    """The calls that are not refused reach the device: the limits themselves, the NULL optionals and no positions with a NULL d_ref."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    L = cwlib.lib()
    assert L.cw_dev_store_account(*_args()) == NO_DEVICE
    assert L.cw_dev_store_account(*_args(nstreams=STREAM_LIMIT)) == NO_DEVICE
    assert L.cw_dev_store_account(*_args(max_positions=LIMIT)) == NO_DEVICE
    assert L.cw_dev_store_account(*_args(dir_entries=LIMIT)) == NO_DEVICE
    for name in ("d_flag", "d_refcount", "d_owner"):
        assert L.cw_dev_store_account(*_args(**{name: None})) == NO_DEVICE, name
    assert L.cw_dev_store_account(*_args(d_flag=None, d_refcount=None, d_owner=None)) == NO_DEVICE
    assert L.cw_dev_store_account(*_args(max_positions=0, d_ref=None)) == NO_DEVICE
    p = POINTERS
    with pytest.raises(cwlib.CwError) as e:
        cwlib.dev_store_account(p["d_ref"], p["d_first"], 3, 100, p["d_dir"], 5, 100, 0, p["d_acct"], 0, 0, p["d_totals"])
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
    """account_kernels.hip: check, clear, positions and entries."""
    out = str(tmp_path / "account_kernels.s")
    subprocess.run(HIPCC + [os.path.join(ROOT, "compute_war_amd", "csrc", "account_kernels.hip"), "-o", out], check=True, capture_output=True)
    meta = _meta(open(out).read())
    assert len(meta) == 4, sorted(meta)
    assert sum(bool(re.search(r"\daccount_(check|clear|positions|entries)_kernel", k)) for k in meta) == 4
    for name, e in meta.items():
        assert re.search(r"\.private_segment_fixed_size:\s+0\b", e), name
        assert re.search(r"\.vgpr_spill_count:\s+0\b", e), name
        assert re.search(r"\.sgpr_spill_count:\s+0\b", e), name
        assert re.search(r"\.max_flat_workgroup_size:\s+256\b", e), name
    makefile = open(os.path.join(ROOT, "compute_war_amd", "csrc", "Makefile")).read()
    assert "account_kernels.hip" in re.search(r"^SRCS\s*:=(.*)$", makefile, flags=re.M).group(1)


def _random_directory(rng, n):
    d = np.zeros(n, AM.LOC)
    for i in range(n):
        kind = rng.integers(0, 4)
        if kind in (1, 3):
            d[i] = (int(rng.integers(0, 1 << 40)), int(rng.integers(1, 300)), int(rng.integers(1, 65537)) | (0x80000000 if kind == 3 else 0))
        elif kind == 2:
            d[i] = [(5, 0, 0), (0, 9, 0), (0, 0, 1 << 20), (0, 0xFFFFFFFF, 0x7FFFFFFF)][int(rng.integers(0, 4))]   # unsound, counted as they are
    return d


def _random_first(rng, nstreams, n):
    """nstreams + 1 ascending cuts of [0, n], with empty streams wherever the draw puts them"""
    cuts = np.sort(rng.integers(0, n + 1, nstreams - 1)) if nstreams > 1 else np.zeros(0, np.int64)
    if nstreams > 2 and rng.random() < 0.5:
        cuts[0], cuts[-1] = 0, n                                        # an empty stream first and one last
    if nstreams > 3 and rng.random() < 0.5:
        cuts[len(cuts) // 2] = cuts[len(cuts) // 2 - 1]                 # ... and one in the middle
    return np.concatenate([[0], np.sort(cuts), [n]]).astype(np.uint64)


def _same(a, b):
    assert a[0] == b[0] and a[4] == b[4], (a[0], b[0], a[4], b[4])
    if a[0]:
        assert a[1:] == b[1:] == (None, None, None, None)
        return
    for x, y, what in zip(a[1:4], b[1:4], ("streams", "refcount", "owner")):
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), (what, x, y)


def test_model_agrees_with_the_loop():
    rng = np.random.default_rng(24)
    seen = dict(none=0, shared=0, owned=0, below=0, miss=0, past=0, zero=0, unsound=0, front=0, middle=0, back=0, flag_other=0, verdicts=set())
    for trial in range(400):
        entries, n, nstreams = int(rng.integers(1, 40)), int(rng.integers(0, 120)), int(rng.integers(1, 9))
        d = _random_directory(rng, entries)
        dir_base = [0, 7, 1 << 40, AM.M - 20][int(rng.integers(0, 4))]
        first = _random_first(rng, nstreams, n)
        refs = np.array([(dir_base + int(v)) % AM.M for v in rng.integers(-2, entries + 2, n)], np.uint64)
        refs[rng.random(n) < 0.05] = AM.M - 1                           # CW_DEDUPE_MISS
        flag = None if trial % 4 == 0 else (rng.random(entries) < 0.4).astype(np.uint32) * np.uint32(rng.integers(1, 1 << 32))
        max_positions = None
        way = trial % 8
        if way == 5 and nstreams > 1:
            first[1] = n + 1                                             # a pair decreases: first[2] <= n
        elif way == 6:
            first = first + np.uint64(1)                                 # first[0] != 0
            refs = np.concatenate([refs, refs[:1] if n else np.zeros(1, np.uint64)])
        elif way == 7 and n:
            max_positions = n - 1                                        # n > max_positions
        a = AM.account(refs, first, d, dir_base, flag, max_positions)
        b = AM.account_np(refs, first, d, dir_base, flag, max_positions)
        _same(a, b)
        seen["verdicts"].add((a[0], way if a[0] else 0))
        if a[0]:
            continue
        _, streams, refcount, owner, totals = a
        idx = [(int(r) - dir_base) % AM.M for r in refs[:int(first[-1])]]
        nz = [any(int(v) for v in e) for e in d]
        seen["none"] += int((owner == AM.NONE).sum())
        seen["shared"] += int((owner == AM.SHARED).sum())
        seen["owned"] += int((owner < AM.SHARED).sum())
        seen["below"] += sum(i >= AM.M - 2 for i in idx)
        seen["miss"] += int((refs[:int(first[-1])] == AM.M - 1).sum())
        seen["past"] += sum(i == entries for i in idx)
        seen["zero"] += sum(i < entries and not nz[i] for i in idx)
        seen["unsound"] += sum(i < entries and nz[i] and (int(d[i]["stored"]) == 0 or int(d[i]["raw"]) & 0x7FFE0000 != 0) for i in idx)
        empty = np.diff(first.astype(np.int64)) == 0
        seen["front"] += bool(empty[0])
        seen["back"] += bool(empty[-1])
        seen["middle"] += bool(empty[1:-1].any())
        seen["flag_other"] += flag is not None and bool((flag > 1).any()) and int(streams["flagged_positions"].sum()) > 0
        # what the outputs say about each other
        assert int(streams["positions"].sum()) == int(first[-1]) and totals[7] == int(streams["missing"].sum())
        assert int(refcount.sum()) == int(streams["positions"].sum()) - totals[7]
        assert totals[3] == int((refcount != 0).sum()) == totals[5] + int(streams["unique_chunks"].sum())
        assert totals[4] == totals[6] + int(streams["unique_stored"].sum()) and totals[3] <= totals[1]
    assert all(seen[k] > 20 for k in seen if k != "verdicts"), seen
    assert {(1, 5), (1, 6), (1, 7), (0, 0)} <= seen["verdicts"], seen["verdicts"]
