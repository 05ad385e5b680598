"""CPU-side checks of scrub and repair: the three symbols are declared, listed, exported and mirrored, the calls refuse bad arguments
before the device and fail loudly without one, the new kernels compile without scratch memory or spills, the knob is accepted and
documented, and the plain-Python model scrubs a store built with the CPU oracle's codecs: every status occurs, the statuses do not
depend on the windows, and the cursors follow the window rule."""
import os
import re
import subprocess

import numpy as np
import pytest

import cdc_model as CM
import restore_model as RM
import scrub_model as SM
from conftest import ROOT, corpus_file

NEW_SYMBOLS = ["cw_dev_store_verify", "cw_store_scrub", "cw_dev_store_replace_chunks"]
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
    for status in ("OK 0", "MALFORMED 1", "UNSOUND 2", "MISMATCH 3", "ORPHAN 4", "SKIPPED 5"):
        assert re.search(r"#define CW_SCRUB_%s\b" % status, text), status
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert set(NEW_SYMBOLS) <= set(re.findall(r"\b(cw_[a-z0-9_]+)\s*\(", text))
    assert set(NEW_SYMBOLS) <= set(_lib.ABI_SYMBOLS)
    out = subprocess.run(["nm", "-D", "--defined-only", cwlib.lib_path()], capture_output=True, text=True, check=True).stdout
    assert set(NEW_SYMBOLS) <= set(re.findall(r" T (cw_[a-z0-9_]+)", out))
    for name in ("dev_store_verify", "store_scrub", "dev_store_replace_chunks", "ScrubReport", "ScrubStats"):
        assert hasattr(cwlib, name)
    for name in ("scrub", "repair_from"):
        assert hasattr(cwlib.ChunkStore, name)
    assert [k for k, _ in cwlib.ScrubStats._fields_] == list(SM.TOTALS)


# Arguments with made-up non-NULL pointers: nothing dereferences them before the device is asked for.
def _verify_args(store_bytes=1 << 20, dir_entries=1000, work_bytes=1 << 20, comp=0, **over):
    a = dict(x=8192, d_store=1 << 24, d_dir=1 << 26, d_live=1 << 27, d_cursor=1 << 28, d_work=1 << 30, d_status=1 << 29, d_totals=(1 << 28) + 64)
    a.update(over)
    return (a["x"], comp, a["d_store"], store_bytes, a["d_dir"], 5, dir_entries, a["d_live"], a["d_cursor"], a["d_work"], work_bytes, a["d_status"],
            a["d_totals"], None)


def _replace_args(in_bytes=1 << 20, store_bytes=1 << 20, dir_entries=1000, max_count=1000, **over):
    a = dict(d_in=1 << 24, d_in_loc=1 << 26, d_values=(1 << 27) + 4096, d_count=1 << 27, d_store=1 << 28, d_used=1 << 29, d_dir=1 << 30,
             d_result=(1 << 29) + 64)
    a.update(over)
    return (a["d_in"], in_bytes, a["d_in_loc"], a["d_values"], a["d_count"], max_count, a["d_store"], store_bytes, a["d_used"], a["d_dir"], 5,
            dir_entries, a["d_result"], None)


def _store(cw, **over):
    a = dict(d_store=1 << 24, store_bytes=1 << 20, d_used=1 << 29, d_dir=1 << 30, dir_base=5, dir_entries=1000)
    a.update(over)
    return cw.Store(a["d_store"], a["store_bytes"], a["d_used"], a["d_dir"], a["dir_base"], a["dir_entries"])


def test_bad_arguments_are_refused_before_the_device(cwlib):
    import ctypes as C
    L = cwlib.lib()
    # verify (a made-up handle: it is only read behind these refusals)
    for name in ("x", "d_store", "d_dir", "d_cursor", "d_work", "d_status", "d_totals"):
        assert L.cw_dev_store_verify(*_verify_args(**{name: None})) == BAD_ARG, name
    for comp in (2, 3, -1):
        assert L.cw_dev_store_verify(*_verify_args(comp=comp)) == BAD_ARG, comp
    assert L.cw_dev_store_verify(*_verify_args(dir_entries=0)) == BAD_ARG
    assert L.cw_dev_store_verify(*_verify_args(dir_entries=TOO_MANY)) == BAD_ARG
    for work in (0, 1, 65535):
        assert L.cw_dev_store_verify(*_verify_args(work_bytes=work)) == BAD_ARG and b"work_bytes" in L.cw_last_error(), work
    for bad in (8, 4, 1):
        assert L.cw_dev_store_verify(*_verify_args(d_dir=(1 << 26) + bad)) == BAD_ARG and b"16-byte aligned" in L.cw_last_error()
    for name, at in (("d_cursor", 1 << 28), ("d_totals", (1 << 28) + 64)):
        for bad in (4, 1):
            assert L.cw_dev_store_verify(*_verify_args(**{name: at + bad})) == BAD_ARG and b"8-byte aligned" in L.cw_last_error(), name

    # scrub: what the device call refuses
    def scrub(st, x=8192, comp=0):
        return L.cw_store_scrub(x, comp, C.byref(st) if st is not None else None, None, None, None)
    assert scrub(None) == BAD_ARG and scrub(_store(cwlib), x=None) == BAD_ARG and scrub(_store(cwlib), comp=2) == BAD_ARG
    for over in (dict(d_store=None), dict(d_used=None), dict(d_dir=None), dict(dir_entries=0), dict(dir_entries=TOO_MANY),
                 dict(d_dir=(1 << 30) + 8)):
        assert scrub(_store(cwlib, **over)) == BAD_ARG, over

    # replace_chunks: the import's refusals, and d_values
    for name in ("d_in", "d_in_loc", "d_values", "d_count", "d_store", "d_used", "d_dir", "d_result"):
        assert L.cw_dev_store_replace_chunks(*_replace_args(**{name: None})) == BAD_ARG, name
    assert L.cw_dev_store_replace_chunks(*_replace_args(max_count=TOO_MANY)) == BAD_ARG
    assert L.cw_dev_store_replace_chunks(*_replace_args(dir_entries=0)) == BAD_ARG
    for bad in (8, 4, 1):
        assert L.cw_dev_store_replace_chunks(*_replace_args(d_in_loc=(1 << 26) + bad)) == BAD_ARG and b"16-byte aligned" in L.cw_last_error()
        assert L.cw_dev_store_replace_chunks(*_replace_args(d_dir=(1 << 30) + bad)) == BAD_ARG and b"16-byte aligned" in L.cw_last_error()
    for name, at in (("d_values", (1 << 27) + 4096), ("d_count", 1 << 27), ("d_used", 1 << 29), ("d_result", (1 << 29) + 64)):
        assert L.cw_dev_store_replace_chunks(*_replace_args(**{name: at + 4})) == BAD_ARG and b"8-byte aligned" in L.cw_last_error(), name
    for at in (1 << 28, (1 << 28) + (1 << 20) - 1, (1 << 28) - (1 << 20) + 1):                      # equal, one byte at either end
        assert L.cw_dev_store_replace_chunks(*_replace_args(d_in=at)) == BAD_ARG and b"overlaps d_store" in L.cw_last_error(), at


def test_no_gpu_means_no_scrub(cwlib):
    """The calls that are not refused reach the device: no flags, an empty store, the smallest work buffer, the largest directory."""
    import ctypes as C
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    L = cwlib.lib()
    assert L.cw_dev_store_verify(*_verify_args()) == NO_DEVICE
    assert L.cw_dev_store_verify(*_verify_args(d_live=None)) == NO_DEVICE
    assert L.cw_dev_store_verify(*_verify_args(d_store=None, store_bytes=0)) == NO_DEVICE
    assert L.cw_dev_store_verify(*_verify_args(work_bytes=65536, comp=1)) == NO_DEVICE
    assert L.cw_dev_store_verify(*_verify_args(dir_entries=TOO_MANY - 1)) == NO_DEVICE
    assert L.cw_store_scrub(8192, 0, C.byref(_store(cwlib)), None, None, None) == NO_DEVICE
    assert L.cw_store_scrub(8192, 1, C.byref(_store(cwlib, d_store=None, store_bytes=0)), 1 << 27, None, None) == NO_DEVICE
    assert L.cw_dev_store_replace_chunks(*_replace_args()) == NO_DEVICE
    assert L.cw_dev_store_replace_chunks(*_replace_args(d_in=None, in_bytes=0)) == NO_DEVICE
    assert L.cw_dev_store_replace_chunks(*_replace_args(max_count=TOO_MANY - 1)) == NO_DEVICE
    for at in ((1 << 28) + (1 << 20), (1 << 28) - (1 << 20)):                                         # adjacent buffers
        assert L.cw_dev_store_replace_chunks(*_replace_args(d_in=at)) == NO_DEVICE
    with pytest.raises(cwlib.CwError) as e:
        cwlib.dev_store_replace_chunks(1 << 24, 1 << 20, 1 << 26, (1 << 27) + 4096, 1 << 27, 10, 1 << 28, 1 << 20, 1 << 29, 1 << 30, 0, 100,
                                       (1 << 29) + 64)
    assert e.value.code == NO_DEVICE


def test_the_knob_is_accepted_and_documented(cwlib):
    L = cwlib.lib()
    try:
        assert L.cw_tune_set(b"CW_SCRUB_ENTRIES", b"64") == 0 and L.cw_tune_set(b"CW_SCRUB_ENTRIES", None) == 0
    finally:
        cwlib.tune_reset()
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "`CW_SCRUB_ENTRIES=" in readme[readme.index("Profiling / test knobs"):].split("\n\n")[0]
    assert "scrub_kernels.hip" in readme
    assert "scrub_entries" in open(os.path.join(ROOT, "compute_war_amd", "csrc", "knobs.h")).read()
    assert SM.entry_cap() == 1 << 20 and SM.entry_cap(1) == 64 and SM.entry_cap(64) == 64 and SM.entry_cap(65) == 65 and SM.entry_cap(0) == 1 << 20


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


def _kernels(tmp_path, source):
    out = str(tmp_path / (source + ".s"))
    subprocess.run(HIPCC + [os.path.join(ROOT, "compute_war_amd", "csrc", source), "-o", out], check=True, capture_output=True)
    return _meta(open(out).read())


def test_scrub_kernels_have_no_private_segment_or_spills(tmp_path):
    """scrub_kernels.hip: classify, recipe and finish; dedupe_kernels.hip: the compare for 16-, 32- and 64-byte digests;
    replicate_kernels.hip: the replace runs the import's three kernels."""
    meta = _kernels(tmp_path, "scrub_kernels.hip")
    assert len(meta) == 3, sorted(meta)
    assert sum(bool(re.search(r"\dscrub_(classify|recipe|finish)_kernel", k)) for k in meta) == 3
    for name, e in meta.items():
        _no_scratch(name, e)
    sweeps = {k: e for k, e in _kernels(tmp_path, "dedupe_kernels.hip").items() if "dedupe_verify_sweep_kernel" in k}
    assert len(sweeps) == 3, sorted(sweeps)
    for name, e in sweeps.items():
        _no_scratch(name, e)
    imports = {k: e for k, e in _kernels(tmp_path, "replicate_kernels.hip").items() if re.search(r"\dimport_(sizes|copy|finish)_kernel", k)}
    assert len(imports) == 3, sorted(imports)
    for name, e in imports.items():
        _no_scratch(name, e)
    makefile = open(os.path.join(ROOT, "compute_war_amd", "csrc", "Makefile")).read()
    assert "scrub_kernels.hip" in re.search(r"^SRCS\s*:=(.*)$", makefile, flags=re.M).group(1)


# ---- the model over a store built with the oracle's codecs -----------------------------------------------------------------------
HASH = "skein"
DIR_ENTRIES = 400


def scenario(oracle, alg):
    """A store of about 230 chunks of text and random bytes (so raw entries occur), then damage of every kind.  Returns (blob,
    store_bytes, directory, {value: [digests]}, the expected status of the entries that were touched)."""
    alice = corpus_file("alice29.txt")
    data = alice + np.random.default_rng(19).bytes(12000) + corpus_file("asyoulik.txt") + alice[20000:60000]
    cuts = CM.chunk(data, CM.default_params(1024))
    m = RM.Model(oracle, alg, 1 << 20, DIR_ENTRIES)
    refs, new, verdict, _ = m.ingest(data, cuts, 0)
    assert verdict == 0 and 200 <= len(new) < len(refs) < DIR_ENTRIES          # duplicates leave all-zero entries between the others
    hash_of = SM.hash_fn(oracle, HASH)
    held = SM.digests_by_value((hash_of(content), v) for content, v in m.values.items())
    blob, d = bytearray(m.blob), m.directory.copy()
    comp = [i for i in new if not int(d[i]["raw"]) & RM.RAW]
    raws = [i for i in new if int(d[i]["raw"]) & RM.RAW]
    assert len(comp) > 100 and len(raws) >= 4
    want = {}
    # malformed: the first flipped byte of a compressed chunk that the decoder refuses
    decode, found = m.decode(), None
    for i in comp[:40]:
        pos, stored, word = (int(v) for v in d[i])
        for at in range(stored):
            ext = bytearray(blob[pos:pos + stored])
            ext[at] ^= 0xFF
            got = decode(bytes(ext), word & RM.LEN_MASK)
            if got is None or len(got) != word & RM.LEN_MASK:
                found = (i, pos + at)
                break
        if found:
            break
    assert found, "no flipped byte makes a compressed chunk malformed"
    blob[found[1]] ^= 0xFF
    want[found[0]] = SM.MALFORMED
    d[comp[50]]["stored"] = 0                                                    # unsound
    want[comp[50]] = SM.UNSOUND
    blob[int(d[raws[1]]["pos"]) + 3] ^= 0x01                                     # a raw chunk with another byte: decodes, another digest
    want[raws[1]] = SM.MISMATCH
    del held[comp[60]]                                                           # the index lost the value
    want[comp[60]] = SM.ORPHAN
    held[comp[61]].insert(0, bytes(16))                                          # a second, foreign digest under one value: either may match
    want[comp[61]] = SM.OK
    return bytes(blob), 1 << 20, d, held, want, decode, hash_of


@pytest.mark.parametrize("alg", ["lz4", "lzf"])
def test_model_scrubs_a_store_with_every_kind_of_damage(oracle, alg):
    blob, store_bytes, d, held, want, decode, hash_of = scenario(oracle, alg)
    status = SM.statuses(blob, store_bytes, d, 0, None, held, decode, hash_of)
    for idx, s in want.items():
        assert status[idx] == s, (idx, s)
    assert sorted(set(status.tolist())) == [0, 1, 2, 3, 4, 5], "the scenario lost a status"
    assert (status[[i for i in range(len(d)) if not any(int(v) for v in d[i])]] == SM.SKIPPED).all()
    needs = SM.need(d, store_bytes)
    whole = sum(needs)
    assert whole > 131072 and len(needs) > 3 * 64
    runs = {}
    for work in (65536, 131072, whole):
        for knob in (64, None):
            cap = SM.entry_cap(knob)
            written, totals, cursors = SM.scrub(needs, status, work, cap)
            runs[work, knob] = cursors
            # statuses and summed totals do not depend on the windows
            assert [written[i] for i in range(len(d))] == status.tolist()
            assert totals["checked"] == int((status != SM.SKIPPED).sum()) == sum(totals[k] for k in SM.TOTALS[1:6])
            assert [totals[k] for k in SM.TOTALS[1:6]] == [int((status == s).sum()) for s in range(5)]
            assert totals["raw_bytes"] == whole and totals["windows"] == len(cursors)
            # the cursors follow the rule: each window is as long as the rule allows, and no longer
            c = 0
            for e in cursors:
                assert c < e <= min(len(d), c + cap) and sum(needs[c:e]) <= work
                assert e == min(len(d), c + cap) or sum(needs[c:e + 1]) > work
                c = e
            assert c == len(d)
    assert runs[whole, None] == [len(d)] and len(runs[whole, 64]) == -(-len(d) // 64)
    assert len(runs[65536, None]) > len(runs[131072, None]) > 1
    # a cursor at or past the end: nothing is written
    for c in (len(d), len(d) + 7):
        assert SM.verify(needs, status, c, 65536, 64) == (c, {}, dict.fromkeys(SM.TOTALS, 0))
    # selection by flags: a flagged all-zero entry is unsound, an unflagged damaged entry is skipped and not counted
    zero = next(i for i in range(len(d)) if not any(int(v) for v in d[i]))
    live = np.ones(len(d), np.uint32)
    bad = next(i for i, s in want.items() if s == SM.MISMATCH)
    live[bad] = 0
    flagged = SM.statuses(blob, store_bytes, d, 0, live, held, decode, hash_of)
    assert flagged[zero] == SM.UNSOUND and flagged[bad] == SM.SKIPPED and SM.need(d, store_bytes, live)[bad] == 0
    keep = np.ones(len(d), bool)
    keep[[bad] + [i for i in range(len(d)) if not any(int(v) for v in d[i])]] = False
    assert (flagged[keep] == status[keep]).all()


def test_model_replaces_chunks_with_every_verdict(oracle):
    blob, store_bytes, d, held, want, decode, hash_of = scenario(oracle, "lz4")
    used = len(blob)
    full = [i for i in range(len(d)) if any(int(v) for v in d[i])]
    a, b = full[3], full[9]
    # the payload: the two entries' own stored bytes, as an export would give them
    locs, pay = np.zeros(2, RM.LOC), bytearray()
    for k, i in enumerate((a, b)):
        pos, stored, word = (int(v) for v in d[i])
        locs[k] = (len(pay), stored, word)
        pay += blob[pos:pos + stored]
    verdict, total, out, entries = SM.replace_chunks(pay, len(pay), locs, [a, b], used, store_bytes, d, 0)
    assert (verdict, total, out) == (0, len(pay), bytes(pay))
    assert entries == {a: (used, int(locs[0]["stored"]), int(locs[0]["raw"])), b: (used + int(locs[0]["stored"]), int(locs[1]["stored"]), int(locs[1]["raw"]))}
    assert SM.replace_chunks(pay, len(pay), locs, [a, b], used, used + len(pay) - 1, d, 0)[:2] == (1, len(pay))
    for outside in (len(d), RM.MISS):
        assert SM.replace_chunks(pay, len(pay), locs, [a, outside], used, store_bytes, d, 0)[:2] == (2, len(pay))
    assert SM.replace_chunks(pay, len(pay), locs, [a + 5, 4], used, store_bytes, d, 5)[0] == 2              # a value below the base
    assert SM.replace_chunks(pay, len(pay) - 1, locs, [a, b], used, store_bytes, d, 0)[:2] == (3, int(locs[0]["stored"]))
    zeroed = locs.copy()
    zeroed[1] = (0, 0, 0)
    assert SM.replace_chunks(pay, len(pay), zeroed, [a, b], used, store_bytes, d, 0)[0] == 3
    assert (int(d[a]["raw"]) ^ int(d[b]["raw"])) & RM.LEN_MASK, "the two chunks differ in length"
    assert SM.replace_chunks(pay, len(pay), locs, [b, a], used, store_bytes, d, 0)[:2] == (4, len(pay))
    # an all-zero entry, or one whose own length field is unsound, takes any length
    free = next(i for i in range(len(d)) if not any(int(v) for v in d[i]))
    assert SM.replace_chunks(pay, len(pay), locs, [free, b], used, store_bytes, d, 0)[0] == 0
    broken = d.copy()
    broken[a]["raw"] = 0x1FFFF                                                   # a length of 131071
    assert SM.replace_chunks(pay, len(pay), locs[1:], [a], used, store_bytes, d, 0)[0] == 4
    assert SM.replace_chunks(pay, len(pay), locs[1:], [a], used, store_bytes, broken, 0)[0] == 0
    # the order of the verdicts: unsound before full before outside before length
    assert SM.replace_chunks(pay, len(pay), zeroed, [len(d), a], used, used, d, 0)[0] == 3
    assert SM.replace_chunks(pay, len(pay), locs, [len(d), a], used, used, d, 0)[0] == 1
    assert SM.replace_chunks(pay, len(pay), locs, [len(d), a], used, store_bytes, d, 0)[0] == 2
