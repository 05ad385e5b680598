"""CPU-side checks of the codecs over chunks: the six symbols are declared, listed, exported and mirrored, the slot layout
keeps its promises, the calls refuse bad arguments before the device and fail loudly without one, and the kernels compile
without scratch memory or spills."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, corpus_file
import cdc_model as CM

NEW_SYMBOLS = ["cw_chunk_slot_offset", "cw_chunk_slots_bytes", "cw_dev_compress_chunks", "cw_dev_pack_chunks",
               "cw_dev_decompress_chunks", "cw_dev_cdc_dedupe_compress"]
LZ4, LZF = 0, 1
NO_DEVICE, BAD_ARG = -1, -2


@pytest.fixture(scope="module")
def cwlib():
    import compute_war_amd as cw
    if not os.path.exists(cw.lib_path()):
        subprocess.run(["make", "-C", os.path.join(ROOT, "compute_war_amd", "csrc"), "-j8"], check=True, capture_output=True)
    return cw


def test_header_declares_and_binding_lists_the_chunk_codec_symbols(cwlib):
    from compute_war_amd import _lib
    text = open(os.path.join(ROOT, "include", "cw_hashcompress.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(cw_[a-z0-9_]+)\s*\(", text))
    assert set(NEW_SYMBOLS) <= declared
    assert set(NEW_SYMBOLS) <= set(_lib.ABI_SYMBOLS)
    out = subprocess.run(["nm", "-D", "--defined-only", cwlib.lib_path()], capture_output=True, text=True, check=True).stdout
    assert set(NEW_SYMBOLS) <= set(re.findall(r" T (cw_[a-z0-9_]+)", out))
    for name in ("chunk_slot_offset", "chunk_slots_bytes", "dev_compress_chunks", "dev_pack_chunks", "dev_decompress_chunks"):
        assert hasattr(cwlib, name)
    assert hasattr(cwlib.DedupeIndex, "dev_cdc_dedupe_compress")


def _cut_lists():
    rng = np.random.default_rng(12)
    for _ in range(40):
        k = int(rng.integers(1, 400))
        hi = int(rng.choice([2, 20, 300, 5000, 65536]))
        lens = rng.integers(1, hi + 1, k)
        yield np.concatenate([[int(rng.integers(0, 1 << int(rng.integers(1, 40))))], lens]).cumsum().tolist()
    yield [0] + [65536 * (i + 1) for i in range(300)]  # every chunk at the maximum
    yield list(range(0, 3000))                         # every chunk one byte
    for name, p in (("lcet10.txt", CM.default_params(8192)), ("kennedy.xls", CM.default_params(1024)), ("ptt5", CM.default_params(8192)),
                    ("sum", CM.params(64, 256, 1024, CM.top_bits(10), CM.top_bits(6)))):
        yield CM.chunk(corpus_file(name), p)


def test_slot_layout(cwlib):
    L = cwlib.lib()
    for cuts in _cut_lists():
        k = len(cuts) - 1
        lz4 = [L.cw_chunk_slot_offset(LZ4, cuts[i], i) for i in range(k + 1)]
        lzf = [L.cw_chunk_slot_offset(LZF, cuts[i], i) for i in range(k + 1)]
        assert lz4 == [cwlib.chunk_slot_offset("lz4", cuts[i], i) for i in range(k + 1)]  # Python and C agree
        assert lzf == [cwlib.chunk_slot_offset("lzf", cuts[i], i) for i in range(k + 1)] == cuts
        for i in range(k):
            l = cuts[i + 1] - cuts[i]
            assert lz4[i] % 16 == 0
            assert lz4[i + 1] - lz4[i] >= cwlib.compress_bound("lz4", l) == l + l // 255 + 16, (i, l)
        for alg, name, slots in ((LZ4, "lz4", lz4), (LZF, "lzf", lzf)):
            for max_chunks in (k, k + 1, 2 * k + 7):
                total = L.cw_chunk_slots_bytes(alg, cuts[-1], max_chunks)
                assert total == cwlib.chunk_slots_bytes(name, cuts[-1], max_chunks) == L.cw_chunk_slot_offset(alg, cuts[-1], max_chunks) + 16
                last = cuts[-1] - cuts[-2]
                assert slots[k - 1] + cwlib.compress_bound(name, last) <= total  # covers the last slot's end
    assert L.cw_chunk_slot_offset(LZ4, 0, 0) == 0 and L.cw_chunk_slot_offset(LZ4, 255, 1) == (255 + 1 + 32) & ~15
    assert L.cw_chunk_slot_offset(LZ4, (1 << 40) + 3, 1 << 20) == ((1 << 40) + 3 + ((1 << 40) + 3) // 255 + (32 << 20)) & ~15


def _args(cwlib, alg=LZ4, src_bytes=1 << 20, max_chunks=1000, short=0, **null):
    """Arguments of cw_dev_compress_chunks with made-up non-NULL pointers (nothing dereferences them before the device is asked for)."""
    a = dict(d_src=4096, d_offsets=8192, d_nchunks=12288, d_sel=None, d_nsel=None, d_dst=16384, d_sizes=20480)
    a.update(null)
    dst_bytes = cwlib.lib().cw_chunk_slots_bytes(alg if alg in (LZ4, LZF) else LZ4, src_bytes, min(max_chunks, 1 << 32)) - short
    return (alg, a["d_src"], src_bytes, a["d_offsets"], a["d_nchunks"], max_chunks, a["d_sel"], a["d_nsel"], a["d_dst"], dst_bytes,
            a["d_sizes"], None)


def test_bad_arguments_are_refused_before_the_device(cwlib):
    L = cwlib.lib()
    for alg in (LZ4, LZF):
        assert L.cw_dev_compress_chunks(*_args(cwlib, alg, short=1)) == BAD_ARG  # one byte short
        assert L.cw_dev_compress_chunks(*_args(cwlib, alg, max_chunks=(1 << 32) - 255)) == BAD_ARG
        for name in ("d_src", "d_offsets", "d_nchunks", "d_dst", "d_sizes"):
            assert L.cw_dev_compress_chunks(*_args(cwlib, alg, **{name: None})) == BAD_ARG, name
        assert L.cw_dev_compress_chunks(*_args(cwlib, alg, d_sel=4096)) == BAD_ARG  # a selection without its count
        assert L.cw_dev_pack_chunks(alg, 4096, 8192, None, 12288, (1 << 32) - 255, 16384, None, 20480, None) == BAD_ARG
        assert L.cw_dev_pack_chunks(alg, 4096, 8192, None, 12288, 100, 16384, None, None, None) == BAD_ARG
        assert L.cw_dev_pack_chunks(alg, None, 8192, None, 12288, 100, 16384, 4096, 20480, None) == BAD_ARG  # bytes wanted, no slots
        assert L.cw_dev_decompress_chunks(alg, None, 8192, 12288, 16384, 100, 20480, 1 << 20, 24576, None) == BAD_ARG
        assert L.cw_dev_decompress_chunks(alg, 4096, 8192, 12288, 16384, (1 << 32) - 255, 20480, 1 << 20, 24576, None) == BAD_ARG
    for alg in (2, 3, -1, 77):  # CW_COMP_NONE and unknown codecs
        assert L.cw_dev_compress_chunks(*_args(cwlib, alg)) == BAD_ARG
        assert L.cw_dev_pack_chunks(alg, 4096, 8192, None, 12288, 100, 16384, None, 20480, None) == BAD_ARG
        assert L.cw_dev_decompress_chunks(alg, 4096, 8192, 12288, 16384, 100, 20480, 1 << 20, 24576, None) == BAD_ARG


def _fused_args(cwlib, p, alg=LZ4, nbytes=1 << 20, short=0, **over):
    max_offsets = nbytes // max(p.min_size, 1) + 2
    a = dict(x=None, d_src=4096, d_offsets=8192, d_nchunks=12288, d_digests=16384, d_ref=20480, d_new_idx=24576, d_n_new=28672,
             d_dst=32768, d_sizes=36864, max_offsets=max_offsets)
    a.update(over)
    k = C.c_size_t(7)
    dst_bytes = cwlib.lib().cw_chunk_slots_bytes(LZ4, nbytes, a["max_offsets"] - 1) - short
    return (a["x"], C.byref(p), alg, a["d_src"], nbytes, 1, 0, a["d_offsets"], a["max_offsets"], a["d_nchunks"], a["d_digests"], a["d_ref"],
            a["d_new_idx"], a["d_n_new"], a["d_dst"], dst_bytes, a["d_sizes"], C.byref(k), None), k


def test_fused_call_refuses_bad_arguments_before_the_device(cwlib):
    L = cwlib.lib()
    for sizes in ((32, 64, 128), (128, 64, 256), (64, 256, 128), (1024, 2048, (1 << 24) + 1)):
        args, k = _fused_args(cwlib, cwlib.CdcParams(*sizes))
        assert L.cw_dev_cdc_dedupe_compress(*args) == BAD_ARG and k.value == 0
    p = cwlib.CdcParams.default(8192)
    assert L.cw_dev_cdc_dedupe_compress(*_fused_args(cwlib, p, short=1)[0]) == BAD_ARG
    assert L.cw_dev_cdc_dedupe_compress(*_fused_args(cwlib, p, alg=2)[0]) == BAD_ARG
    assert L.cw_dev_cdc_dedupe_compress(*_fused_args(cwlib, p, max_offsets=(1 << 20) // 2048 + 1)[0]) == BAD_ARG
    for name in ("d_src", "d_offsets", "d_nchunks", "d_digests", "d_ref", "d_new_idx", "d_n_new", "d_dst", "d_sizes"):
        assert L.cw_dev_cdc_dedupe_compress(*_fused_args(cwlib, p, **{name: None})[0]) == BAD_ARG, name
    assert L.cw_dev_cdc_dedupe_compress(*_fused_args(cwlib, p, d_digests=16388)[0]) == BAD_ARG  # digests not 8-byte aligned


def test_no_gpu_means_no_chunk_codec(cwlib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    L = cwlib.lib()
    for alg in (LZ4, LZF):
        assert L.cw_dev_compress_chunks(*_args(cwlib, alg)) == NO_DEVICE
        assert L.cw_dev_compress_chunks(*_args(cwlib, alg, d_sel=4096, d_nsel=8192)) == NO_DEVICE
        assert L.cw_dev_pack_chunks(alg, 4096, 8192, None, 12288, 100, 16384, 4096, 20480, None) == NO_DEVICE
        assert L.cw_dev_decompress_chunks(alg, 4096, 8192, 12288, 16384, 100, 20480, 1 << 20, 24576, None) == NO_DEVICE
        assert L.cw_dev_cdc_dedupe_compress(*_fused_args(cwlib, cwlib.CdcParams.default(8192), alg=alg)[0]) == NO_DEVICE
    with pytest.raises(cwlib.CwError) as e:
        cwlib.dev_compress_chunks("lz4", 4096, 1 << 20, 8192, 12288, 1000, 16384, cwlib.chunk_slots_bytes("lz4", 1 << 20, 1000), 20480)
    assert e.value.code == NO_DEVICE


def _meta(asm):
    meta = asm[asm.index("amdhsa.kernels"):]
    out = {}
    for e in re.split(r"\n  - ", meta):
        m = re.search(r"\.name:\s+(\S+)", e)
        if m:
            out[m.group(1)] = e
    return out


# chunk_codec_kernels.hip: three kernels of the order (histogram, scan, scatter), the two parsers, the decoder for each codec;
# pack_kernels.hip: the four it had and the three of cw_dev_pack_chunks
@pytest.mark.parametrize("src,count", [("chunk_codec_kernels.hip", 7), ("pack_kernels.hip", 7)])
def test_kernels_have_no_private_segment_or_spills(tmp_path, src, count):
    out = str(tmp_path / "k.s")
    subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-S", "--cuda-device-only", "--offload-arch=gfx950",
                    os.path.join(ROOT, "compute_war_amd", "csrc", src), "-o", out], check=True, capture_output=True)
    meta = _meta(open(out).read())
    assert len(meta) == count, sorted(meta)
    for name, e in meta.items():
        assert re.search(r"\.private_segment_fixed_size:\s+0\b", e), name
        assert re.search(r"\.vgpr_spill_count:\s+0\b", e), name
        assert re.search(r"\.sgpr_spill_count:\s+0\b", e), name
    if src == "chunk_codec_kernels.hip":
        assert sum("chunks_kernel" in k for k in meta) == 4 and sum("chunk_order" in k for k in meta) == 3
