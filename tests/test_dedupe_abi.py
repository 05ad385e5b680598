"""CPU-side checks of the dedupe index: its symbols are declared and exported, it fails loudly without a GPU, and the probe
protocol compiled as written (agent-scope 64-bit CAS on global memory, no flat atomics, no scratch)."""
import os
import re
import subprocess

import pytest

from conftest import ROOT

NEW_SYMBOLS = ["cw_dedupe_create", "cw_dedupe_destroy", "cw_dedupe_count", "cw_dev_dedupe", "cw_dev_hash_dedupe_compress"]


@pytest.fixture(scope="module")
def cwlib():
    import compute_war_amd as cw
    if not os.path.exists(cw.lib_path()):
        subprocess.run(["make", "-C", os.path.join(ROOT, "compute_war_amd", "csrc"), "-j8"], check=True, capture_output=True)
    return cw


def test_header_declares_and_binding_lists_the_dedupe_symbols(cwlib):
    from compute_war_amd import _lib
    text = open(os.path.join(ROOT, "include", "cw_hashcompress.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(cw_[a-z0-9_]+)\s*\(", text))
    assert set(NEW_SYMBOLS) <= declared
    assert set(NEW_SYMBOLS) <= set(_lib.ABI_SYMBOLS)
    assert "typedef struct cw_dedupe cw_dedupe_t;" in text


def test_dedupe_symbols_are_exported(cwlib):
    out = subprocess.run(["nm", "-D", "--defined-only", cwlib.lib_path()], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (cw_[a-z0-9_]+)", out))
    assert set(NEW_SYMBOLS) <= exported, sorted(set(NEW_SYMBOLS) - exported)
    L = cwlib.lib()
    for s in NEW_SYMBOLS:
        assert hasattr(L, s)


def test_no_gpu_means_no_index(cwlib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    L = cwlib.lib()
    assert not L.cw_dedupe_create(cwlib.HASH_SKEIN512, 1024)
    assert b"no HIP device" in L.cw_last_error()
    with pytest.raises(cwlib.CwError):
        cwlib.DedupeIndex("skein512", 1024)
    with pytest.raises(cwlib.CwError):
        cwlib.DedupeIndex("sha256mb", 1 << 20)


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


def test_probe_protocol_compiled_as_written(dedupe_asm):
    kernels = _kernel_blocks(dedupe_asm)
    probes = [k for k in kernels if "dedupe_probe_kernel" in k]
    assert len(probes) == 3, sorted(kernels)           # 16-, 32- and 64-byte digests
    assert len([k for k in kernels if "dedupe" in k]) >= 6
    for k in probes:
        assert "global_atomic_cmpswap_x2" in kernels[k], k
    for k, body in kernels.items():
        if "dedupe" in k:
            assert not re.search(r"\bflat_atomic", body), k
            assert not re.search(r"\b(scratch|buffer)_(load|store)", body), k


def test_dedupe_kernels_have_no_private_segment_or_spills(dedupe_asm):
    meta = dedupe_asm[dedupe_asm.index("amdhsa.kernels"):]
    entries = re.split(r"\n  - ", meta)
    seen = 0
    for e in entries:
        m = re.search(r"\.name:\s+(\S+)", e)
        if not m or "dedupe" not in m.group(1):
            continue
        seen += 1
        assert re.search(r"\.private_segment_fixed_size:\s+0\b", e), m.group(1)
        assert re.search(r"\.vgpr_spill_count:\s+0\b", e), m.group(1)
        assert re.search(r"\.sgpr_spill_count:\s+0\b", e), m.group(1)
    assert seen >= 6
