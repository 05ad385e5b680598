"""CPU-side checks of content-defined chunking: the symbols are declared, listed and exported, the default parameters, the
calls fail loudly without a GPU, the kernels compile without scratch or spills, and the reference model agrees with the
plain loop of the definition and with itself across streaming pieces."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import cdc_model as CM

NEW_SYMBOLS = ["cw_cdc_default_params", "cw_dev_cdc", "cw_dev_hash_chunks", "cw_cdc_hash"]


@pytest.fixture(scope="module")
def cwlib():
    import compute_war_amd as cw
    if not os.path.exists(cw.lib_path()):
        subprocess.run(["make", "-C", os.path.join(ROOT, "compute_war_amd", "csrc"), "-j8"], check=True, capture_output=True)
    return cw


def test_header_declares_and_binding_lists_the_cdc_symbols(cwlib):
    from compute_war_amd import _lib
    text = open(os.path.join(ROOT, "include", "cw_hashcompress.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(cw_[a-z0-9_]+)\s*\(", text))
    assert set(NEW_SYMBOLS) <= declared
    assert set(NEW_SYMBOLS) <= set(_lib.ABI_SYMBOLS)
    assert "} cw_cdc_params;" in text
    out = subprocess.run(["nm", "-D", "--defined-only", cwlib.lib_path()], capture_output=True, text=True, check=True).stdout
    assert set(NEW_SYMBOLS) <= set(re.findall(r" T (cw_[a-z0-9_]+)", out))
    for name in ("CdcParams", "dev_cdc", "dev_hash_chunks", "cdc_hash"):
        assert hasattr(cwlib, name)


@pytest.mark.parametrize("lg", range(8, 22))
def test_default_params(cwlib, lg):
    normal = 1 << lg
    p = cwlib.CdcParams.default(normal)
    want = CM.default_params(normal)
    assert (p.min_size, p.normal_size, p.max_size, p.reserved) == (normal // 4, normal, normal * 8, 0)
    assert (p.mask_s, p.mask_l) == (want["mask_s"], want["mask_l"])
    assert not p.gear
    if normal == 8192:
        assert (p.mask_s, p.mask_l) == (0xFFFE000000000000, 0xFFE0000000000000)


@pytest.mark.parametrize("normal,want", [(0, 256), (3, 256), (255, 256), (1000, 512), (1 << 21, 1 << 21), ((1 << 21) + 5, 1 << 21),
                                         (1 << 29, 1 << 21), (0xFFFFFFFF, 1 << 21)])
def test_default_params_clamp_other_sizes(cwlib, normal, want):
    import ctypes as C
    p = cwlib.CdcParams(64, 64, 64, 1, 1)
    cwlib.lib().cw_cdc_default_params(C.byref(p), normal)
    d = cwlib.CdcParams.default(want)
    assert (p.min_size, p.normal_size, p.max_size, p.reserved, p.mask_s, p.mask_l) == \
        (d.min_size, d.normal_size, d.max_size, 0, d.mask_s, d.mask_l) == (want // 4, want, want * 8, 0) + (d.mask_s, d.mask_l)


@pytest.mark.parametrize("normal", [256, 1024, 8192, 1 << 21])
def test_python_constructor_defaults_to_the_library_defaults(cwlib, normal):
    a, b = cwlib.CdcParams(normal_size=normal), cwlib.CdcParams.default(normal)
    assert (a.min_size, a.normal_size, a.max_size, a.mask_s, a.mask_l) == (b.min_size, b.normal_size, b.max_size, b.mask_s, b.mask_l)
    c = cwlib.CdcParams()
    assert (c.min_size, c.normal_size, c.max_size, c.mask_s, c.mask_l) == (2048, 8192, 65536, 0xFFFE000000000000, 0xFFE0000000000000)
    assert cwlib.CdcParams(normal_size=normal, mask_s=0, mask_l=0).mask_s == 0


def test_no_gpu_means_no_chunking(cwlib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    L = cwlib.lib()
    p = cwlib.CdcParams.default(8192)
    import ctypes as C
    assert L.cw_dev_cdc(C.byref(p), 1 << 20, 4096, 1, 1 << 21, 4096, 1 << 22, None) == -1
    with pytest.raises(cwlib.CwError) as e:
        cwlib.cdc_hash(p, b"x" * 100000, "skein512")
    assert e.value.code == -1


def test_bad_params_are_refused_before_the_device(cwlib):
    import ctypes as C
    L = cwlib.lib()
    for args in ((32, 64, 128), (128, 64, 256), (64, 256, 128), (1024, 2048, (1 << 24) + 1)):
        p = cwlib.CdcParams(*args)
        assert L.cw_dev_cdc(C.byref(p), 1 << 20, 4096, 1, 1 << 21, 4096, 1 << 22, None) == -2
    p = cwlib.CdcParams.default(1024)
    assert L.cw_dev_cdc(C.byref(p), 1 << 20, 1 << 20, 1, 1 << 21, (1 << 20) // 256 + 1, 1 << 22, None) == -2  # max_offsets too small


def _meta(asm):
    meta = asm[asm.index("amdhsa.kernels"):]
    out = {}
    for e in re.split(r"\n  - ", meta):
        m = re.search(r"\.name:\s+(\S+)", e)
        if m:
            out[m.group(1)] = e
    return out


@pytest.mark.parametrize("src,needle,count", [("cdc_kernels.hip", "", 11), ("skein_kernels.hip", "chunks", 2),
                                              ("sha256_kernel.hip", "chunks", 1)])
def test_kernels_have_no_private_segment_or_spills(tmp_path, src, needle, count):
    out = str(tmp_path / "k.s")
    subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-S", "--cuda-device-only", "--offload-arch=gfx950",
                    os.path.join(ROOT, "compute_war_amd", "csrc", src), "-o", out], check=True, capture_output=True)
    meta = {k: v for k, v in _meta(open(out).read()).items() if needle in k}
    assert len(meta) == count, sorted(meta)
    for name, e in meta.items():
        assert re.search(r"\.private_segment_fixed_size:\s+0\b", e), name
        assert re.search(r"\.vgpr_spill_count:\s+0\b", e), name
        assert re.search(r"\.sgpr_spill_count:\s+0\b", e), name


def _inputs():
    rng = np.random.default_rng(7)
    bible = open(os.path.join(ROOT, "tests", "golden", "corpus", "canterbury", "alice29.txt"), "rb").read()
    return [bible[:20000], rng.integers(0, 256, 20000, dtype=np.uint8).tobytes(), bytes(5000), b"\xab" * 3000,
            b"ab" * 2000, bytes(rng.integers(0, 256, 3000, dtype=np.uint8)) + bytes(4000) + bible[:3000], b"", b"q", bytes(63)]


@pytest.mark.parametrize("p", [CM.params(64, 256, 1024, CM.top_bits(10), CM.top_bits(6)),
                               CM.params(64, 64, 64, CM.top_bits(10), CM.top_bits(6)),
                               CM.params(64, 128, 512, 0, 0), CM.params(64, 128, 512, CM.M64, CM.M64),
                               CM.params(100, 300, 700, 0xF0000000000000F0, 0x3, gear=[CM.splitmix64(v ^ 0x55) for v in range(256)])])
def test_model_equals_the_definition(p):
    for data in _inputs():
        assert CM.chunk(data, p) == CM.chunk_serial(data, p)
        assert CM.chunk(data, p, final=False) == CM.chunk_serial(data, p, final=False)


def test_streaming_pieces_equal_one_call():
    p = CM.params(64, 256, 1024, CM.top_bits(10), CM.top_bits(6))
    rng = np.random.default_rng(3)
    for data in _inputs()[:6]:
        whole = CM.chunk(data, p)
        for _ in range(3):
            assert CM.chunk_pieces(data, p, rng.integers(1, 3000, 40)) == whole


def test_degenerate_inputs_follow_the_rules():
    p = CM.default_params(8192)
    for data in (bytes(1 << 18), b"\xff" * (1 << 18), b"ab" * (1 << 17)):
        L = np.diff(CM.chunk(data, p))
        assert set(L[:-1].tolist()) == {p["max"]}
    text = open(os.path.join(ROOT, "tests", "golden", "corpus", "canterbury", "alice29.txt"), "rb").read()
    assert set(np.diff(CM.chunk(text, dict(p, mask_s=0, mask_l=0)))[:-1].tolist()) == {p["min"]}
    assert set(np.diff(CM.chunk(text, dict(p, mask_s=CM.M64, mask_l=CM.M64)))[:-1].tolist()) == {p["max"]}
