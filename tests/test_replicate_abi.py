"""CPU-side checks of the chunk bundle calls: the four symbols are declared, listed, exported and mirrored, the calls refuse bad
arguments before the device and fail loudly without one, the kernels compile without scratch memory or spills, and the
plain-Python model replicates two streams of three between two stores with the CPU oracle's codecs."""
import os
import re
import subprocess

import numpy as np
import pytest

import cdc_model as CM
import replicate_model as PM
import restore_model as RM
import store_gc_model as GM
from conftest import ROOT, corpus_file

NEW_SYMBOLS = ["cw_dev_dedupe_export_live", "cw_dev_store_export_chunks", "cw_dev_store_import_chunks", "cw_dev_translate_refs"]
NO_DEVICE, BAD_ARG = -1, -2
HIPCC = ["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-S", "--cuda-device-only", "--offload-arch=gfx950"]
TOO_MANY = (1 << 32) - 255


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
    assert set(NEW_SYMBOLS) <= set(_lib.ABI_SYMBOLS)
    out = subprocess.run(["nm", "-D", "--defined-only", cwlib.lib_path()], capture_output=True, text=True, check=True).stdout
    assert set(NEW_SYMBOLS) <= set(re.findall(r" T (cw_[a-z0-9_]+)", out))
    for name in ("dev_store_export_chunks", "dev_store_import_chunks", "dev_translate_refs", "Bundle"):
        assert hasattr(cwlib, name)
    assert hasattr(cwlib.DedupeIndex, "dev_export_live")
    for name in ("export_bundle", "import_bundle", "replicate_to"):
        assert hasattr(cwlib.ChunkStore, name)
    assert hasattr(cwlib.Bundle, "save") and hasattr(cwlib.Bundle, "load")


# Arguments with made-up non-NULL pointers: nothing dereferences them before the device is asked for.
def _live_args(dir_entries=1000, max_out=1000, **over):
    a = dict(x=8192, d_live=4096, d_digests=1 << 20, d_values=1 << 21, d_result=1 << 22)
    a.update(over)
    return (a["x"], a["d_live"], 5, dir_entries, a["d_digests"], a["d_values"], max_out, a["d_result"], None)


def _export_args(store_bytes=1 << 20, out_bytes=1 << 20, dir_entries=1000, max_count=1000, **over):
    a = dict(d_store=1 << 24, d_dir=1 << 26, d_values=1 << 27, d_count=(1 << 27) + (1 << 20), d_out=1 << 28, d_out_loc=1 << 29, d_result=1 << 30)
    a.update(over)
    return (a["d_store"], store_bytes, a["d_dir"], 5, dir_entries, a["d_values"], a["d_count"], max_count, a["d_out"], out_bytes, a["d_out_loc"],
            a["d_result"], None)


def _import_args(in_bytes=1 << 20, store_bytes=1 << 20, dir_entries=1000, max_count=1000, **over):
    a = dict(d_in=1 << 24, d_in_loc=1 << 26, d_count=1 << 27, d_sel=(1 << 27) + 4096, d_nsel=(1 << 27) + 8192, d_store=1 << 28, d_used=1 << 29,
             d_dir=1 << 30, d_result=(1 << 29) + 64)
    a.update(over)
    return (a["d_in"], in_bytes, a["d_in_loc"], a["d_count"], max_count, a["d_sel"], a["d_nsel"], 7, a["d_store"], store_bytes, a["d_used"],
            a["d_dir"], 5, dir_entries, a["d_result"], None)


def _translate_args(max_count=1000, max_pairs=1000, **over):
    a = dict(d_ref=1 << 20, d_count=1 << 21, d_from=1 << 22, d_to=1 << 23, d_npairs=1 << 24, d_out=1 << 25, d_n_missing=1 << 26)
    a.update(over)
    return (a["d_ref"], a["d_count"], max_count, a["d_from"], a["d_to"], a["d_npairs"], max_pairs, a["d_out"], a["d_n_missing"], None)


def test_bad_arguments_are_refused_before_the_device(cwlib):
    L = cwlib.lib()
    # export_live (a made-up handle: it is only read behind these refusals)
    for name in ("x", "d_live", "d_digests", "d_values", "d_result"):
        assert L.cw_dev_dedupe_export_live(*_live_args(**{name: None})) == BAD_ARG, name
    for name in ("d_digests", "d_values", "d_result"):
        assert L.cw_dev_dedupe_export_live(*_live_args(**{name: (1 << 22) + 4})) == BAD_ARG and b"8-byte aligned" in L.cw_last_error(), name
    assert L.cw_dev_dedupe_export_live(*_live_args(dir_entries=0)) == BAD_ARG
    assert L.cw_dev_dedupe_export_live(*_live_args(dir_entries=TOO_MANY)) == BAD_ARG
    assert L.cw_dev_dedupe_export_live(*_live_args(max_out=TOO_MANY)) == BAD_ARG

    # export_chunks
    for name in ("d_store", "d_dir", "d_values", "d_count", "d_out", "d_out_loc", "d_result"):
        assert L.cw_dev_store_export_chunks(*_export_args(**{name: None})) == BAD_ARG, name
    assert L.cw_dev_store_export_chunks(*_export_args(max_count=TOO_MANY)) == BAD_ARG
    assert L.cw_dev_store_export_chunks(*_export_args(dir_entries=0)) == BAD_ARG
    for bad in (8, 4, 1):
        assert L.cw_dev_store_export_chunks(*_export_args(d_dir=(1 << 26) + bad)) == BAD_ARG and b"16-byte aligned" in L.cw_last_error()
        assert L.cw_dev_store_export_chunks(*_export_args(d_out_loc=(1 << 29) + bad)) == BAD_ARG and b"16-byte aligned" in L.cw_last_error()
    for name, at in (("d_values", 1 << 27), ("d_count", (1 << 27) + (1 << 20)), ("d_result", 1 << 30)):
        assert L.cw_dev_store_export_chunks(*_export_args(**{name: at + 4})) == BAD_ARG and b"8-byte aligned" in L.cw_last_error(), name
    for out in (1 << 24, (1 << 24) + (1 << 20) - 1, (1 << 24) - (1 << 20) + 1):                # equal, one byte at either end
        assert L.cw_dev_store_export_chunks(*_export_args(d_out=out)) == BAD_ARG and b"overlaps d_store" in L.cw_last_error(), out

    # import_chunks
    for name in ("d_in", "d_in_loc", "d_count", "d_store", "d_used", "d_dir", "d_result", "d_sel", "d_nsel"):
        assert L.cw_dev_store_import_chunks(*_import_args(**{name: None})) == BAD_ARG, name      # (d_sel / d_nsel: only together)
    assert L.cw_dev_store_import_chunks(*_import_args(max_count=TOO_MANY)) == BAD_ARG
    assert L.cw_dev_store_import_chunks(*_import_args(dir_entries=0)) == BAD_ARG
    for bad in (8, 4, 1):
        assert L.cw_dev_store_import_chunks(*_import_args(d_in_loc=(1 << 26) + bad)) == BAD_ARG and b"16-byte aligned" in L.cw_last_error()
        assert L.cw_dev_store_import_chunks(*_import_args(d_dir=(1 << 30) + bad)) == BAD_ARG and b"16-byte aligned" in L.cw_last_error()
    for name, at in (("d_count", 1 << 27), ("d_nsel", (1 << 27) + 8192), ("d_used", 1 << 29), ("d_result", (1 << 29) + 64)):
        assert L.cw_dev_store_import_chunks(*_import_args(**{name: at + 4})) == BAD_ARG and b"8-byte aligned" in L.cw_last_error(), name

    # translate_refs
    for name in ("d_ref", "d_count", "d_from", "d_to", "d_npairs", "d_out", "d_n_missing"):
        assert L.cw_dev_translate_refs(*_translate_args(**{name: None})) == BAD_ARG, name
        assert L.cw_dev_translate_refs(*_translate_args(**{name: (1 << 27) + 4})) == BAD_ARG and b"8-byte aligned" in L.cw_last_error(), name
    assert L.cw_dev_translate_refs(*_translate_args(max_count=TOO_MANY)) == BAD_ARG
    assert L.cw_dev_translate_refs(*_translate_args(max_pairs=TOO_MANY)) == BAD_ARG


def test_no_gpu_means_no_bundle(cwlib):
    """The calls that are not refused reach the device: the largest counts, the dry run, no selection, the neighbours of the overlap."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    L = cwlib.lib()
    assert L.cw_dev_dedupe_export_live(*_live_args()) == NO_DEVICE
    assert L.cw_dev_dedupe_export_live(*_live_args(max_out=0, d_digests=None, d_values=None)) == NO_DEVICE          # only counts
    assert L.cw_dev_dedupe_export_live(*_live_args(dir_entries=TOO_MANY - 1, max_out=TOO_MANY - 1)) == NO_DEVICE
    assert L.cw_dev_store_export_chunks(*_export_args()) == NO_DEVICE
    assert L.cw_dev_store_export_chunks(*_export_args(max_count=TOO_MANY - 1)) == NO_DEVICE
    assert L.cw_dev_store_export_chunks(*_export_args(d_out=None, out_bytes=0)) == NO_DEVICE                        # the dry run
    assert L.cw_dev_store_export_chunks(*_export_args(d_store=None, store_bytes=0)) == NO_DEVICE
    for out in ((1 << 24) + (1 << 20), (1 << 24) - (1 << 20)):                                                      # adjacent buffers
        assert L.cw_dev_store_export_chunks(*_export_args(d_out=out)) == NO_DEVICE
    assert L.cw_dev_store_import_chunks(*_import_args()) == NO_DEVICE
    assert L.cw_dev_store_import_chunks(*_import_args(d_sel=None, d_nsel=None)) == NO_DEVICE                        # every chunk
    assert L.cw_dev_store_import_chunks(*_import_args(d_in=None, in_bytes=0)) == NO_DEVICE
    assert L.cw_dev_store_import_chunks(*_import_args(max_count=TOO_MANY - 1)) == NO_DEVICE
    assert L.cw_dev_translate_refs(*_translate_args()) == NO_DEVICE
    assert L.cw_dev_translate_refs(*_translate_args(d_out=1 << 20)) == NO_DEVICE                                    # in place
    assert L.cw_dev_translate_refs(*_translate_args(max_count=TOO_MANY - 1, max_pairs=TOO_MANY - 1)) == NO_DEVICE
    for call in (lambda: cwlib.dev_store_export_chunks(1 << 24, 1 << 20, 1 << 26, 0, 100, 1 << 27, 1 << 21, 10, 0, 0, 1 << 29, 1 << 30),
                 lambda: cwlib.dev_store_import_chunks(1 << 24, 1 << 20, 1 << 26, 1 << 27, 10, 0, 1 << 28, 1 << 20, 1 << 29, 1 << 30, 0, 100,
                                                       (1 << 29) + 64),
                 lambda: cwlib.dev_translate_refs(1 << 20, 1 << 21, 10, 1 << 22, 1 << 23, 1 << 24, 10, 1 << 20, 1 << 26)):
        with pytest.raises(cwlib.CwError) as e:
            call()
        assert e.value.code == NO_DEVICE


def _meta(asm):
    meta = asm[asm.index("amdhsa.kernels"):]
    out = {}
    for e in re.split(r"\n  - ", meta):
        m = re.search(r"\.name:\s+(\S+)", e)
        if m:
            out[m.group(1)] = e
    return out


def _no_scratch(name, e):
    assert re.search(r"\.private_segment_fixed_size:\s+0\b", e), name
    assert re.search(r"\.vgpr_spill_count:\s+0\b", e), name
    assert re.search(r"\.sgpr_spill_count:\s+0\b", e), name


def test_replicate_kernels_have_no_private_segment_or_spills(tmp_path):
    """replicate_kernels.hip: sizes, copy and finish of the export and of the import, and the translate."""
    out = str(tmp_path / "k.s")
    subprocess.run(HIPCC + [os.path.join(ROOT, "compute_war_amd", "csrc", "replicate_kernels.hip"), "-o", out], check=True, capture_output=True)
    meta = _meta(open(out).read())
    assert len(meta) == 7, sorted(meta)
    assert sum(bool(re.search(r"\d((export|import)_(sizes|copy|finish)|translate_refs)_kernel", k)) for k in meta) == 7
    for name, e in meta.items():
        _no_scratch(name, e)
    makefile = open(os.path.join(ROOT, "compute_war_amd", "csrc", "Makefile")).read()
    assert "replicate_kernels.hip" in re.search(r"^SRCS\s*:=(.*)$", makefile, flags=re.M).group(1)


def test_export_live_kernels_have_no_scratch_and_claim_with_the_64_bit_cas(tmp_path):
    out = str(tmp_path / "d.s")
    subprocess.run(HIPCC + [os.path.join(ROOT, "compute_war_amd", "csrc", "dedupe_kernels.hip"), "-o", out], check=True, capture_output=True)
    asm = open(out).read()
    meta = {k: e for k, e in _meta(asm).items() if "dedupe_live_" in k}
    assert len(meta) == 7, sorted(meta)                       # the flags, and fill and sweep for 16-, 32- and 64-byte digests
    for name, e in meta.items():
        _no_scratch(name, e)
    bodies = {m.group(1): m.group(2) for m in re.finditer(r"^(_Z\S+):[^\n]*\n(.*?)^\.Lfunc_end", asm, flags=re.M | re.S)}
    sweeps = [k for k in meta if "dedupe_live_sweep_kernel" in k]
    assert len(sweeps) == 3
    for name in sweeps:
        assert "global_atomic_cmpswap_x2" in bodies[name], name                                          # a hit claims its rank
        assert len(re.findall(r"^\s*global_atomic_add_x2", bodies[name], flags=re.M)) == 1, name      # the hit count: one per workgroup


@pytest.mark.parametrize("alg", ["lz4", "lzf"])
def test_model_replicates_two_streams_of_three(oracle, alg):
    """Store A holds a, b and c, store B (another directory base) holds b: a and c go over with only the chunks B lacks, B's model
    restores both byte for byte, a second replication carries nothing, and a bundle without negotiation leaves the same store."""
    a, b, c = GM.three_streams(corpus_file("alice29.txt"), corpus_file("kennedy.xls"))
    p = CM.default_params(1024)
    A, B = RM.Model(oracle, alg, 1 << 20, 512), RM.Model(oracle, alg, 1 << 20, 1024, dir_base=1000)
    base, recs = 0, []
    for data in (a, b, c):
        cuts = CM.chunk(data, p)
        refs, _, v, _ = A.ingest(data, cuts, base)
        assert v == 0
        recs.append((data, cuts, refs))
        base += len(cuts) - 1
    cuts_b = CM.chunk(b, p)
    refs_b, _, v, _ = B.ingest(b, cuts_b, 1000)
    assert v == 0
    base_b = 1000 + len(cuts_b) - 1
    (_, cuts_a, refs_a), _, (_, cuts_c, refs_c) = recs
    B2 = RM.Model(oracle, alg, B.store_bytes, 1024, dir_base=1000)                      # a copy of B for the run without negotiation
    B2.blob, B2.directory, B2.values = bytearray(B.blob), B.directory.copy(), dict(B.values)

    before = len(B.blob)
    bundle, (ra, rc), new = PM.replicate(A, B, [refs_a, refs_c], base_b)
    n = len(bundle["values"])
    assert bundle["values"] == sorted(set(refs_a) | set(refs_c)) and n == len(set(bundle["digests"]))
    # exactly the chunks B lacked travel: some, not all, and they are the ones that were new to B's index
    assert 0 < len(bundle["carried"]) < n and bundle["carried"] == new
    assert len(B.blob) - before == len(bundle["payload"]) == int(bundle["locs"]["stored"].sum())
    assert all(1000 <= r < base_b + n for r in ra + rc) and set(ra) & set(refs_b)        # shared chunks keep B's values
    for data, cuts, refs in ((a, cuts_a, ra), (c, cuts_c, rc), (b, cuts_b, refs_b)):
        got = RM.restore(B.blob, len(B.blob), B.directory, 1000, refs, cuts, len(data), B.decode())
        assert [s for s, _ in got] == [0] * len(refs) and b"".join(x for _, x in got) == data
    # again: everything is known, nothing travels, the store stays
    size = len(B.blob)
    again, (ra2, rc2), new2 = PM.replicate(A, B, [refs_a, refs_c], base_b + n)
    assert again["carried"] == [] == new2 and again["payload"] == b"" and len(B.blob) == size and (ra2, rc2) == (ra, rc)
    # without negotiation every chunk travels, and the import still stores only what is new: the same store bytes
    full, (ra3, rc3), new3 = PM.replicate(A, B2, [refs_a, refs_c], base_b, negotiate=False)
    assert full["carried"] == list(range(n)) and new3 == new and len(full["payload"]) > len(bundle["payload"])
    assert bytes(B2.blob) == bytes(B.blob) and (B2.directory == B.directory).all() and (ra3, rc3) == (ra, rc)

    # the four calls' refusals in the model: all or nothing
    vals = bundle["values"]
    assert PM.export_chunks(A.blob, A.store_bytes, A.directory, 0, vals, len(A.blob))[0] == 0
    total = PM.export_chunks(A.blob, A.store_bytes, A.directory, 0, vals, 0)[1][1]
    assert PM.export_chunks(A.blob, A.store_bytes, A.directory, 0, vals, total - 1) == (1, [1, total, n], None, None)
    for bad in (RM.MISS, 511, 512):                                                        # no such entry: a zero one, outside
        assert PM.export_chunks(A.blob, A.store_bytes, A.directory, 0, vals + [bad], 1 << 20)[1] == [2, total, n + 1]
    locs, pay = full["locs"], full["payload"]
    assert PM.import_chunks(pay, len(pay), locs, n, [n], 0, 0, 1 << 20, 0, 1024)[0] == 3
    assert PM.import_chunks(pay, len(pay) - 1, locs, n, None, 0, 0, 1 << 20, 0, 1024)[0] == 3      # the last chunk leaves in_bytes
    assert PM.import_chunks(pay, len(pay), locs, n, None, 0, 1, len(pay), 0, 1024)[:2] == (1, len(pay))
    assert PM.import_chunks(pay, len(pay), locs, n, None, 0, 0, len(pay), 1, 1024)[0] == 2         # chunk 0 below the directory
    assert PM.import_chunks(pay, len(pay), locs, n, None, 1024 - n + 1, 0, len(pay), 0, 1024)[0] == 2
    assert PM.translate([5, 7, 9, RM.MISS], [5, 9], [50, 90]) == ([50, RM.MISS, 90, RM.MISS], 2)
    live = np.zeros(8, np.uint32)
    live[[1, 4, 5]] = 1
    assert PM.export_live([(b"x", 11), (b"y", 15), (b"z", 99), (b"w", 15)], live, 10, 8, 2) == ([11, RM.MISS], [[b"x"], []], [3, 3])
