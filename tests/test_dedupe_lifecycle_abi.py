"""CPU-side checks of the dedupe index's lifecycle calls (lookup, insert with values, export / import, resize): declared, listed
and exported; they fail loudly without a GPU; and the kernels compiled as written -- the lookup only reads the table (its one
atomic is the hit counter), the rehash claims slots with the agent-scope 64-bit CAS."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

NEW_SYMBOLS = ["cw_dev_dedupe_lookup", "cw_dev_dedupe_insert", "cw_dev_dedupe_export", "cw_dedupe_export", "cw_dedupe_import",
               "cw_dedupe_set_stage_entries", "cw_dedupe_resize", "cw_dedupe_max_entries"]


@pytest.fixture(scope="module")
def cwlib():
    import compute_war_amd as cw
    if not os.path.exists(cw.lib_path()):
        subprocess.run(["make", "-C", os.path.join(ROOT, "compute_war_amd", "csrc"), "-j8"], check=True, capture_output=True)
    return cw


def test_header_declares_and_binding_lists_the_lifecycle_symbols(cwlib):
    from compute_war_amd import _lib
    raw = open(os.path.join(ROOT, "include", "cw_hashcompress.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = set(re.findall(r"\b(cw_[a-z0-9_]+)\s*\(", text))
    assert set(NEW_SYMBOLS) <= declared, sorted(set(NEW_SYMBOLS) - declared)
    assert set(NEW_SYMBOLS) <= set(_lib.ABI_SYMBOLS)
    assert re.search(r"^#define\s+CW_DEDUPE_MISS\s+UINT64_MAX\b", text, flags=re.M)
    assert cwlib.DedupeIndex.MISS == 2 ** 64 - 1
    # the contract notes the issue asks for
    assert "cannot be told from a miss" in raw and "live at once" in raw


def test_lifecycle_symbols_are_exported(cwlib):
    out = subprocess.run(["nm", "-D", "--defined-only", cwlib.lib_path()], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (cw_[a-z0-9_]+)", out))
    assert set(NEW_SYMBOLS) <= exported, sorted(set(NEW_SYMBOLS) - exported)
    L = cwlib.lib()
    for s in NEW_SYMBOLS:
        assert hasattr(L, s)


def test_no_gpu_means_error_not_fallback(cwlib, tmp_path):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    L = cwlib.lib()
    u = C.c_uint64(0)
    z = C.c_size_t(0)
    buf = (C.c_uint8 * 64)()
    # a NULL index (none can exist without a device): every entry point refuses
    assert L.cw_dev_dedupe_lookup(None, buf, 1, C.byref(u), C.byref(u), None) != 0
    assert L.cw_dev_dedupe_insert(None, buf, C.byref(u), 1, C.byref(u), buf, C.byref(u), None) != 0
    assert L.cw_dev_dedupe_export(None, buf, C.byref(u), 1, C.byref(u), None) != 0
    assert L.cw_dedupe_export(None, buf, C.byref(u), 1, C.byref(z)) != 0
    assert L.cw_dedupe_import(None, buf, C.byref(u), 1, C.byref(z)) != 0
    assert L.cw_dedupe_resize(None, 16) != 0
    assert L.cw_dedupe_max_entries(None, C.byref(z)) != 0
    assert L.cw_dedupe_set_stage_entries(None, 16) != 0
    # a snapshot on disk does not make an index without a device
    path = tmp_path / "snap.npz"
    with open(path, "wb") as f:
        np.savez(f, hash_alg=np.int64(cwlib.HASH_SHA256), max_entries=np.int64(64), digests=np.zeros((3, 32), np.uint8),
                 values=np.arange(3, dtype=np.uint64))
    with pytest.raises(cwlib.CwError):
        cwlib.DedupeIndex.load(path)
    with pytest.raises(cwlib.CwError):
        cwlib.DedupeIndex.load(path, max_entries=2)       # fewer than the saved entries: refused before anything else
    # a closed / never-opened handle raises instead of answering
    idx = cwlib.DedupeIndex.__new__(cwlib.DedupeIndex)
    idx._h, idx.hash_alg, idx.max_entries = None, cwlib.HASH_SHA256, 0
    for call in (lambda: idx.dev_lookup(0, 1, 0, 0), lambda: idx.dev_insert(0, 0, 1, 0, 0, 0), lambda: idx.dev_export(0, 0, 1, 0),
                 lambda: idx.resize(16), lambda: idx.export(), lambda: idx.import_(np.zeros((1, 32), np.uint8), np.zeros(1, np.uint64)),
                 lambda: idx.save(tmp_path / "x.npz")):
        with pytest.raises(cwlib.CwError):
            call()


def _kernel_blocks(asm):
    """{kernel symbol: its code} of the device assembly (each kernel runs from its label to .Lfunc_end)."""
    out = {}
    for m in re.finditer(r"^(_Z\S+):[^\n]*\n(.*?)^\.Lfunc_end", asm, flags=re.M | re.S):
        out[m.group(1)] = m.group(2)
    return out


@pytest.fixture(scope="module")
def dedupe_asm(tmp_path_factory):
    src = os.path.join(ROOT, "compute_war_amd", "csrc", "dedupe_kernels.hip")
    out = str(tmp_path_factory.mktemp("asm") / "dedupe.s")
    subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-S", "--cuda-device-only", "--offload-arch=gfx950", src, "-o", out],
                   check=True, capture_output=True)
    return open(out).read()


def test_lookup_only_reads_the_table(dedupe_asm):
    kernels = _kernel_blocks(dedupe_asm)
    lookups = [k for k in kernels if "dedupe_lookup_kernel" in k]
    assert len(lookups) == 3, sorted(kernels)             # 16-, 32- and 64-byte digests
    for k in lookups:
        body = kernels[k]
        assert "global_atomic_cmpswap" not in body, k
        atomics = re.findall(r"^\s*((?:global|flat|buffer|ds)_atomic\w*|ds_(?:add|cmpst|min|max|or)\w*)", body, flags=re.M)
        assert atomics == ["global_atomic_add_x2"], (k, atomics)      # the hit counter: one instruction, behind the workgroup's sum
        assert re.search(r"\bs_bcnt1_i32_b64\b", body), k            # ... of each wavefront's ballot population count


def test_rehash_claims_slots_with_the_64_bit_cas(dedupe_asm):
    kernels = _kernel_blocks(dedupe_asm)
    rehash = [k for k in kernels if "dedupe_rehash_kernel" in k]
    assert len(rehash) == 3, sorted(kernels)
    for k in rehash:
        assert "global_atomic_cmpswap_x2" in kernels[k], k
    # the value-carrying resolve is a variant of the resolve, not of the probe
    assert len([k for k in kernels if "dedupe_probe_kernel" in k]) == 3
    assert len([k for k in kernels if "dedupe_resolve_kernel" in k]) == 6
    assert len([k for k in kernels if "dedupe_export" in k]) == 4
