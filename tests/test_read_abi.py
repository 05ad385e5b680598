"""CPU-side checks of cw_dev_read_ranges: the symbol is declared, listed, exported and mirrored, the call refuses bad arguments
before the device and fails loudly without one, the kernels of read_kernels.hip compile without scratch memory or spills, and
the plain-Python model (tests/read_model.py) gives the input's slices and the restore's verdicts with the CPU oracle's codecs.

The inputs of tests/test_gpu_read.py are built here, and the mix of stored forms those tests rely on is established here too."""
import os
import re
import subprocess

import numpy as np
import pytest

import cdc_model as CM
import lz_streams as LS
import read_model as RD
import restore_model as RM
from conftest import ROOT, corpus_file

LZ4, LZF = 0, 1
NO_DEVICE, BAD_ARG = -1, -2
P256, P1K = CM.default_params(256), CM.default_params(1024)


def noise(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


# ---- the inputs shared with the GPU tests -----------------------------------------------------------------------------------
def window_input():
    """Text + noise for normal_size 256: about 90 chunks of 64..2048 bytes, both stored forms."""
    xls, txt = corpus_file("kennedy.xls"), corpus_file("alice29.txt")
    return xls[:6000] + noise(3000, 31) + txt[2000:9000] + noise(2500, 32) + xls[20000:25000] + noise(1500, 33) + txt[30000:34000]


def mixed_input():
    """Text + noise + spreadsheet for normal_size 1024."""
    return corpus_file("alice29.txt")[:60000] + noise(20000, 5) + corpus_file("kennedy.xls")[:40000]


def largest_input():
    """Three chunks of exactly 65536 bytes: text, noise, spreadsheet."""
    text = (corpus_file("lcet10.txt") + corpus_file("alice29.txt"))[:65536]
    return text + noise(65536, 34) + corpus_file("kennedy.xls")[:65536], [0, 65536, 131072, 196608]


def stored_forms(m: RM.Model, refs):
    """(positions kept raw, positions stored compressed) of a recipe in a model."""
    raw = [j for j, r in enumerate(refs) if m.directory[r - m.dir_base]["raw"] & RM.RAW]
    return raw, [j for j in range(len(refs)) if j not in set(raw)]


def window_ranges(cuts):
    """Test 1's ranges: a start at every cut plus each of -17 .. 17 where valid, each with the lengths around the copy's and the
    chunk's edges and one through the next three cuts, where they end inside the stream."""
    out, n = [], cuts[-1]
    for i, c in enumerate(cuts):
        for d in (-17, -16, -15, -1, 0, 1, 15, 16, 17):
            a = c + d
            if not 0 <= a < n:
                continue
            l = cuts[min(i + 1, len(cuts) - 1)] - c
            lens = [1, 15, 16, 17, 63, 64, 65, l - 1, l, l + 1, cuts[min(i + 3, len(cuts) - 1)] - a]
            out += [(a, x) for x in lens if x > 0 and a + x <= n]
    return out


def damaged_stream(alg, stream: bytes, length: int, decode, rng):
    """An edit of tests/lz_streams.py that the oracle's decoder refuses and whose first changed byte lies behind byte 8 of the stream:
    the chunk's first byte is decoded before the decoder can meet the damage."""
    edits_of, parse = (LS.lz4_edits, LS.lz4_parse) if alg == "lz4" else (LS.lzf_edits, LS.lzf_parse)
    for _, d in list(edits_of(parse(stream), length, rng)) + list(LS._random_edits(stream, rng)):
        if d and d[:8] == stream[:8] and len(d) < 65536:
            got = decode(d, length)
            if got is None or len(got) != length:
                return d
    raise AssertionError("no edit of this stream is refused")


# ---- the boundary ------------------------------------------------------------------------------------------------------------
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
    assert "cw_dev_read_ranges" in re.findall(r"\b(cw_[a-z0-9_]+)\s*\(", text)
    assert "cw_dev_read_ranges" in _lib.ABI_SYMBOLS
    out = subprocess.run(["nm", "-D", "--defined-only", cwlib.lib_path()], capture_output=True, text=True, check=True).stdout
    assert "cw_dev_read_ranges" in re.findall(r" T (cw_[a-z0-9_]+)", out)
    assert hasattr(cwlib, "dev_read_ranges") and hasattr(cwlib.ChunkStore, "read_ranges") and hasattr(cwlib.ChunkStore, "read")


def _args(alg=LZ4, max_count=1000, max_ranges=100, store_bytes=1 << 20, dst_bytes=1 << 20, dir_entries=1000, **over):
    """Arguments with made-up non-NULL pointers (nothing dereferences them before the device is asked for)."""
    a = dict(d_store=4096, d_dir=8192, d_ref=12288, d_raw=16384, d_count=20480, d_off=24576, d_len=28672, d_to=32768, d_n=36864, d_dst=40960,
             d_status=45056)
    a.update(over)
    return (alg, a["d_store"], store_bytes, a["d_dir"], 0, dir_entries, a["d_ref"], a["d_raw"], a["d_count"], max_count, a["d_off"], a["d_len"],
            a["d_to"], a["d_n"], max_ranges, a["d_dst"], dst_bytes, a["d_status"], None)


def test_bad_arguments_are_refused_before_the_device(cwlib):
    import torch
    L = cwlib.lib()
    for alg in (LZ4, LZF):
        for name in ("d_store", "d_dir", "d_ref", "d_raw", "d_count", "d_off", "d_len", "d_to", "d_n", "d_dst", "d_status"):
            assert L.cw_dev_read_ranges(*_args(alg, **{name: None})) == BAD_ARG, name
        assert L.cw_dev_read_ranges(*_args(alg, max_count=(1 << 32) - 255)) == BAD_ARG
        assert L.cw_dev_read_ranges(*_args(alg, max_ranges=(1 << 32) - 255)) == BAD_ARG
        assert L.cw_dev_read_ranges(*_args(alg, dir_entries=0)) == BAD_ARG
        for bad in (8192 + 8, 8192 + 4, 8192 + 1):
            assert L.cw_dev_read_ranges(*_args(alg, d_dir=bad)) == BAD_ARG
    assert b"16-byte aligned" in L.cw_last_error()
    for alg in (2, 3, -1, 77):  # CW_COMP_NONE and unknown codecs
        assert L.cw_dev_read_ranges(*_args(alg)) == BAD_ARG
    if not torch.cuda.is_available():
        # not refused: a NULL store of 0 bytes, a NULL destination of 0 bytes, no ranges, the largest counts
        for kw in (dict(d_store=None, store_bytes=0), dict(d_dst=None, dst_bytes=0), dict(max_ranges=0), dict(max_count=0),
                   dict(max_count=(1 << 32) - 256, max_ranges=(1 << 32) - 256)):
            assert L.cw_dev_read_ranges(*_args(**kw)) == NO_DEVICE, kw


def test_no_gpu_means_no_read(cwlib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    L = cwlib.lib()
    for alg in (LZ4, LZF):
        assert L.cw_dev_read_ranges(*_args(alg)) == NO_DEVICE
    with pytest.raises(cwlib.CwError) as e:
        cwlib.dev_read_ranges("lzf", 4096, 1 << 20, 8192, 0, 100, 12288, 16384, 20480, 100, 24576, 28672, 32768, 36864, 10, 40960, 1 << 20, 45056)
    assert e.value.code == NO_DEVICE
    cs = object.__new__(cwlib.ChunkStore)   # (a store cannot be made without a device: the methods ask for one first)
    recipe = cwlib.Recipe([0], [0, 100])
    with pytest.raises(cwlib.CwError) as e:
        cs.read_ranges(recipe, [(0, 10), (50, 50)])
    assert e.value.code == NO_DEVICE
    with pytest.raises(cwlib.CwError) as e:
        cs.read(recipe, 0, 10)
    assert e.value.code == NO_DEVICE


def _meta(asm):
    meta = asm[asm.index("amdhsa.kernels"):]
    out = {}
    for e in re.split(r"\n  - ", meta):
        m = re.search(r"\.name:\s+(\S+)", e)
        if m:
            out[m.group(1)] = e
    return out


def test_kernels_have_no_private_segment_or_spills(tmp_path):
    """read_kernels.hip: the plan, and the pieces and the edges for each codec."""
    out = str(tmp_path / "k.s")
    subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-S", "--cuda-device-only", "--offload-arch=gfx950",
                    os.path.join(ROOT, "compute_war_amd", "csrc", "read_kernels.hip"), "-o", out], check=True, capture_output=True)
    meta = _meta(open(out).read())
    assert len(meta) == 5, sorted(meta)
    assert sum("read_plan_kernel" in k for k in meta) == 1
    assert sum("read_pieces_kernel" in k for k in meta) == 2 and sum("read_edges_kernel" in k for k in meta) == 2
    for name, e in meta.items():
        assert re.search(r"\.private_segment_fixed_size:\s+0\b", e), name
        assert re.search(r"\.vgpr_spill_count:\s+0\b", e), name
        assert re.search(r"\.sgpr_spill_count:\s+0\b", e), name
    makefile = open(os.path.join(ROOT, "compute_war_amd", "csrc", "Makefile")).read()
    assert "read_kernels.hip" in re.search(r"^SRCS\s*:=(.*)$", makefile, flags=re.M).group(1)


# ---- the model against the oracle ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alg", ["lz4", "lzf"])
def test_model_gives_the_inputs_slices_and_the_restores_verdicts(oracle, alg):
    rng = np.random.default_rng(17)
    data = mixed_input()
    cuts = CM.chunk(data, P1K)
    k, n = len(cuts) - 1, len(data)
    m = RM.Model(oracle, alg, 1 << 20, k + 4, dir_base=9)
    refs, _, verdict, _ = m.ingest(data, cuts, 9)
    assert verdict == 0
    raws, comp = stored_forms(m, refs)
    assert len(raws) >= 10 and len(comp) >= 40
    # a few hundred ranges: single bytes, short ones, ones over several chunks, the whole stream, empty ones anywhere
    ranges = [(0, 1, 0), (n - 1, 1, 0), (0, n, 0), (5, 0, 0), (2 ** 64 - 1, 0, 2 ** 64 - 1)]
    ranges += [(int(a), 1, 0) for a in rng.integers(0, n, 60)]
    ranges += [(int(a), int(min(l, n - a)), 0) for a, l in zip(rng.integers(0, n, 150), rng.integers(1, 300, 150))]
    ranges += [(int(a), int(min(l, n - a)), 0) for a, l in zip(rng.integers(0, n, 100), rng.integers(1000, 9000, 100))]
    ranges += [(c - 1, 2, 0) for c in cuts[1:-1]]
    got = RD.read(m.blob, m.store_bytes, m.directory, 9, refs, cuts, ranges, n, m.decode())
    for (a, l, _), (status, piece) in zip(ranges, got):
        assert status == 0 and piece == data[a:a + l], (a, l, status)
    # the coordinates are the recipe's: the same stream at an offset
    shifted = [c + 1000 for c in cuts]
    got = RD.read(m.blob, m.store_bytes, m.directory, 9, refs, shifted, [(1000, 10, 0), (999, 10, 0), (1000 + n - 3, 3, 0), (1000 + n - 3, 4, 0)],
                  n, m.decode())
    assert got == [(0, data[:10]), (3, None), (0, data[-3:]), (3, None)]
    # refusals: the destination, a wrap, no recipe
    got = RD.read(m.blob, m.store_bytes, m.directory, 9, refs, cuts, [(0, 10, n - 9), (0, 10, n - 10), (2 ** 64 - 5, 10, 0), (0, 10, 2 ** 64 - 5)],
                  n, m.decode())
    assert [s for s, _ in got] == [3, 0, 3, 3]
    assert RD.read(m.blob, m.store_bytes, m.directory, 9, [], [0], [(0, 1, 0), (0, 0, 0)], n, m.decode()) == [(3, None), (0, b"")]
    # a damaged entry gives 2, damaged stored bytes give 1, to exactly the ranges that touch them
    bad, blob = m.directory.copy(), bytearray(m.blob)
    j2, j1 = comp[5], comp[20]
    bad[refs[j2] - 9]["stored"] = 0
    pos, stored, word = (int(v) for v in bad[refs[j1] - 9])
    d = damaged_stream(alg, bytes(blob[pos:pos + stored]), word & RM.LEN_MASK, m.decode(), rng)
    bad[refs[j1] - 9] = (len(blob), len(d), word)
    blob += d
    for j, want in ((j2, 2), (j1, 1)):
        near = [(cuts[j], 1, 0), (cuts[j + 1] - 1, 1, 0), (cuts[j] - 1, 2, 0), (cuts[j + 1] - 1, 2, 0), (cuts[j - 1], cuts[j + 2] - cuts[j - 1], 0)]
        beside = [(cuts[j] - 1, 1, 0), (cuts[j + 1], 1, 0), (cuts[j - 1], cuts[j] - cuts[j - 1], 0), (cuts[j + 1], cuts[j + 2] - cuts[j + 1], 0)]
        got = RD.read(blob, m.store_bytes, bad, 9, refs, cuts, near + beside, n, m.decode())
        assert [s for s, _ in got] == [want] * len(near) + [0] * len(beside)
        assert all(piece == data[a:a + l] for (a, l, _), (_, piece) in zip(beside, got[len(near):]))


@pytest.mark.parametrize("alg", ["lz4", "lzf"])
def test_the_gpu_tests_inputs_have_both_stored_forms(oracle, alg):
    data = window_input()
    cuts = CM.chunk(data, P256)
    lens = np.diff(cuts)
    assert len(cuts) - 1 >= 40 and lens.min() >= 1 and lens.max() <= 2048
    m = RM.Model(oracle, alg, 1 << 20, len(cuts))
    refs, _, verdict, _ = m.ingest(data, cuts, 0)
    raws, comp = stored_forms(m, refs)
    assert verdict == 0 and len(raws) >= 10 and len(comp) >= 10
    # a cut between two compressed chunks and one between a raw and a compressed one, both with 50 bytes on either side
    pairs = [(j, j + 1) for j in range(len(refs) - 1) if lens[j] >= 50 and lens[j + 1] >= 50]
    assert any(a in comp and b in comp for a, b in pairs) and any(a in raws and b in comp for a, b in pairs)
    assert 2 * len(window_ranges(cuts)) > 16384     # more edge slots than the call has decode buffers
    data, cuts = largest_input()
    m = RM.Model(oracle, alg, 1 << 20, 4)
    refs, _, verdict, _ = m.ingest(data, cuts, 0)
    assert verdict == 0 and stored_forms(m, refs) == ([1], [0, 2])
