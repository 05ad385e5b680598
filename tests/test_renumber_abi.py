"""CPU-side checks of renumber and revalue: the two symbols are declared, listed, exported and mirrored, the calls refuse bad
arguments before the device and fail loudly without one, the kernels compile without scratch memory or spills, and the numpy model
agrees with a brute-force loop on random small directories."""
import os
import re
import subprocess

import numpy as np
import pytest

import renumber_model as NM
from conftest import ROOT

NEW_SYMBOLS = ["cw_dev_store_renumber", "cw_dev_dedupe_revalue"]
NO_DEVICE, BAD_ARG = -1, -2
HIPCC = ["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-S", "--cuda-device-only", "--offload-arch=gfx950"]
LIMIT = (1 << 32) - 256
DIR, NEW = 1 << 26, 1 << 29          # made-up directories, 1000 entries each


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
    assert hasattr(cwlib, "dev_store_renumber") and hasattr(cwlib.DedupeIndex, "dev_revalue") and hasattr(cwlib.ChunkStore, "renumber")


def _renumber_args(dir_entries=1000, new_dir_entries=1000, max_pairs=1000, new_dir_base=7, **over):
    """Arguments of cw_dev_store_renumber with made-up non-NULL pointers (nothing dereferences them before the device is asked for)."""
    a = dict(d_dir=DIR, d_live=1 << 27, d_new_dir=NEW, d_from=1 << 30, d_to=1 << 31, d_result=(1 << 32) + 64)
    a.update(over)
    return (a["d_dir"], 5, dir_entries, a["d_live"], 7, a["d_new_dir"], new_dir_base, new_dir_entries, a["d_from"], a["d_to"], max_pairs,
            a["d_result"], None)


def _revalue_args(max_pairs=1000, range_base=5, range_entries=1000, **over):
    """Arguments of cw_dev_dedupe_revalue; the handle is made up too (it is only read behind the device check)."""
    a = dict(x=8192, d_from=1 << 30, d_to=1 << 31, d_npairs=1 << 28, d_result=(1 << 32) + 64)
    a.update(over)
    return (a["x"], a["d_from"], a["d_to"], a["d_npairs"], max_pairs, range_base, range_entries, a["d_result"], None)


def test_bad_arguments_are_refused_before_the_device(cwlib):
    L = cwlib.lib()
    for name in ("d_dir", "d_new_dir", "d_from", "d_to", "d_result"):
        assert L.cw_dev_store_renumber(*_renumber_args(**{name: None})) == BAD_ARG, name
    # one half of the dry run's NULLs is a NULL pointer
    assert L.cw_dev_store_renumber(*_renumber_args(d_from=None, d_to=None)) == BAD_ARG
    assert L.cw_dev_store_renumber(*_renumber_args(max_pairs=0, d_from=None, d_to=None, d_new_dir=None)) == BAD_ARG
    assert L.cw_dev_store_renumber(*_renumber_args(max_pairs=1, new_dir_entries=0, d_new_dir=None, d_from=None)) == BAD_ARG
    assert L.cw_dev_store_renumber(*_renumber_args(dir_entries=0)) == BAD_ARG and b"dir_entries is 0" in L.cw_last_error()
    for name in ("dir_entries", "new_dir_entries", "max_pairs"):
        assert L.cw_dev_store_renumber(*_renumber_args(**{name: LIMIT + 1})) == BAD_ARG and name.encode() in L.cw_last_error(), name
    for bad in (8, 4, 1):
        assert L.cw_dev_store_renumber(*_renumber_args(d_dir=DIR + bad)) == BAD_ARG and b"16-byte aligned" in L.cw_last_error()
        assert L.cw_dev_store_renumber(*_renumber_args(d_new_dir=NEW + bad)) == BAD_ARG and b"16-byte aligned" in L.cw_last_error()
    for name, p in (("d_from", 1 << 30), ("d_to", 1 << 31), ("d_result", (1 << 32) + 64)):
        for bad in (4, 1):
            assert L.cw_dev_store_renumber(*_renumber_args(**{name: p + bad})) == BAD_ARG and b"8-byte aligned" in L.cw_last_error(), name
    # the new directory overlapping the old one: equal (there is no in-place form), one entry at either end, one inside
    for new in (DIR, DIR + 16 * 999, DIR - 16 * 999, DIR + 16):
        assert L.cw_dev_store_renumber(*_renumber_args(d_new_dir=new)) == BAD_ARG and b"overlaps d_dir" in L.cw_last_error(), new
    # a small new directory inside a large old one, and a large one around a small old one
    assert L.cw_dev_store_renumber(*_renumber_args(d_new_dir=DIR + 16 * 500, new_dir_entries=10)) == BAD_ARG
    assert L.cw_dev_store_renumber(*_renumber_args(d_new_dir=DIR - 16 * 500, new_dir_entries=2000, dir_entries=10)) == BAD_ARG
    assert L.cw_dev_store_renumber(*_renumber_args(new_dir_base=(1 << 64) - 1000)) == BAD_ARG and b"wraps" in L.cw_last_error()

    for name in ("x", "d_from", "d_to", "d_npairs", "d_result"):
        assert L.cw_dev_dedupe_revalue(*_revalue_args(**{name: None})) == BAD_ARG, name
    for name, p in (("d_from", 1 << 30), ("d_to", 1 << 31), ("d_npairs", 1 << 28), ("d_result", (1 << 32) + 64)):
        for bad in (4, 1):
            assert L.cw_dev_dedupe_revalue(*_revalue_args(**{name: p + bad})) == BAD_ARG and b"8-byte aligned" in L.cw_last_error(), name
    assert L.cw_dev_dedupe_revalue(*_revalue_args(max_pairs=LIMIT + 1)) == BAD_ARG and b"max_pairs" in L.cw_last_error()
    assert L.cw_dev_dedupe_revalue(*_revalue_args(range_base=(1 << 64) - 1000)) == BAD_ARG and b"wraps" in L.cw_last_error()


def test_no_gpu_means_no_renumbering(cwlib):
    """The calls that are not refused reach the device: the limits themselves, the neighbours of the overlap cases and the dry run."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    L = cwlib.lib()
    assert L.cw_dev_store_renumber(*_renumber_args()) == NO_DEVICE
    assert L.cw_dev_store_renumber(*_renumber_args(d_live=None)) == NO_DEVICE
    for name in ("dir_entries", "new_dir_entries", "max_pairs"):
        assert L.cw_dev_store_renumber(*_renumber_args(d_new_dir=1 << 40, **{name: LIMIT})) == NO_DEVICE, name
    for new in (DIR + 16 * 1000, DIR - 16 * 1000):                                       # adjacent directories
        assert L.cw_dev_store_renumber(*_renumber_args(d_new_dir=new)) == NO_DEVICE
    assert L.cw_dev_store_renumber(*_renumber_args(max_pairs=0, d_from=None, d_to=None, new_dir_entries=0, d_new_dir=None)) == NO_DEVICE
    assert L.cw_dev_store_renumber(*_renumber_args(new_dir_entries=0, d_new_dir=DIR)) == NO_DEVICE   # an empty range overlaps nothing
    assert L.cw_dev_store_renumber(*_renumber_args(new_dir_base=(1 << 64) - 1001)) == NO_DEVICE
    assert L.cw_dev_dedupe_revalue(*_revalue_args()) == NO_DEVICE
    assert L.cw_dev_dedupe_revalue(*_revalue_args(max_pairs=LIMIT, range_base=(1 << 64) - 1001)) == NO_DEVICE
    assert L.cw_dev_dedupe_revalue(*_revalue_args(max_pairs=0, range_entries=0)) == NO_DEVICE
    with pytest.raises(cwlib.CwError) as e:
        cwlib.dev_store_renumber(DIR, 5, 100, 0, 7, NEW, 7, 100, 1 << 30, 1 << 31, 100, (1 << 32) + 64)
    assert e.value.code == NO_DEVICE
    with pytest.raises(cwlib.CwError) as e:
        cwlib.dev_store_renumber(DIR, 5, 100, 0, 7, 0, 7, 0, 0, 0, 0, (1 << 32) + 64)      # the dry run through the wrapper
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


def _kernels(tmp_path, source):
    out = str(tmp_path / (source + ".s"))
    subprocess.run(HIPCC + [os.path.join(ROOT, "compute_war_amd", "csrc", source), "-o", out], check=True, capture_output=True)
    return _meta(open(out).read())


def test_new_kernels_have_no_private_segment_or_spills(tmp_path):
    """renumber_kernels.hip: flags, fill, scatter and finish; dedupe_kernels.hip: the two sweeps, which need no digest width."""
    meta = _kernels(tmp_path, "renumber_kernels.hip")
    assert len(meta) == 4, sorted(meta)
    assert sum(bool(re.search(r"\drenumber_(flags|fill|scatter|finish)_kernel", k)) for k in meta) == 4
    for name, e in meta.items():
        _no_scratch(name, e)
    sweeps = {k: e for k, e in _kernels(tmp_path, "dedupe_kernels.hip").items() if "dedupe_revalue" in k}
    assert len(sweeps) == 2 and sum(bool(re.search(r"\ddedupe_revalue_(count|apply)_kernel", k)) for k in sweeps) == 2, sorted(sweeps)
    for name, e in sweeps.items():
        _no_scratch(name, e)
    makefile = open(os.path.join(ROOT, "compute_war_amd", "csrc", "Makefile")).read()
    assert "renumber_kernels.hip" in re.search(r"^SRCS\s*:=(.*)$", makefile, flags=re.M).group(1)


def _random_directory(rng, n):
    d = np.zeros(n, NM.LOC)
    for i in range(n):
        kind = rng.integers(0, 4)
        if kind == 1:
            d[i] = (int(rng.integers(0, 1 << 40)), int(rng.integers(1, 300)), int(rng.integers(1, 65537)))
        elif kind == 2:
            d[i] = [(5, 0, 0), (0, 9, 0), (0, 0, 1 << 20)][int(rng.integers(0, 3))]      # unsound, each field alone non-zero
    return d


def test_model_agrees_with_the_loop():
    rng = np.random.default_rng(5)
    seen = set()
    for trial in range(400):
        n = int(rng.integers(1, 40))
        d = _random_directory(rng, n)
        live = None if trial % 5 == 0 else (rng.random(n) < 0.6).astype(np.uint32) * int(rng.integers(1, 9))
        K = NM.renumber(d, 0, live, 0, 0, n, n)[0][1]
        new_dir_base = int(rng.choice([0, 100, (1 << 64) - 50]))
        new_dir_entries = int(rng.integers(0, 45))
        new_base = max(0, min(NM.M - 1, new_dir_base + int(rng.integers(-2, 6))))
        max_pairs = max(0, K + int(rng.integers(-2, 3)))
        args = (d, int(rng.integers(0, 1 << 50)), live, new_base, new_dir_base, new_dir_entries, max_pairs)
        a, b = NM.renumber(*args), NM.renumber_loop(*args)
        assert a[0] == b[0], (trial, a[0], b[0])
        seen.add(a[0][0])
        if a[0][0] == 0:
            assert all((x == y).all() for x, y in zip(a[1:], b[1:]))
            assert (np.diff(a[2].astype(object)) > 0).all() and (np.diff(a[3].astype(object)) == 1).all()
        else:
            assert a[1:] == b[1:] == (None, None, None)
    assert seen == {0, 1, 2}
    # the wrap: K entries from 2^64 - K + 1 on
    d = _random_directory(rng, 30)
    K = NM.renumber(d, 0, None, 0, 0, 30, 30)[0][1]
    assert K > 3
    for new_base, want in ((NM.M - K, 2), (NM.M - K - 1, 0)):
        args = (d, 0, None, new_base, NM.M - K - 1, K, K)
        assert NM.renumber(*args)[0][0] == NM.renumber_loop(*args)[0][0] == want
    verdicts = set()
    for trial in range(300):
        n, p = int(rng.integers(0, 30)), int(rng.integers(0, 12))
        base = int(rng.choice([0, 1000, (1 << 64) - 40]))
        values = [min(NM.M - 2, base + int(v)) for v in rng.integers(0, 40, n)]
        frm = sorted(set(min(NM.M - 2, base + int(v)) for v in rng.integers(0, 40, p)))
        to = [base + k for k in range(len(frm))]
        args = (values, frm, to, int(rng.integers(0, len(frm) + 3)), int(rng.integers(0, len(frm) + 1)), base + int(rng.integers(0, 10)),
                int(rng.integers(0, 30)))
        a, b = NM.revalue(*args), NM.revalue_loop(*args)
        assert a == b, (trial, a, b)
        verdicts.add(a[0][0])
    assert verdicts == {0, 1}
