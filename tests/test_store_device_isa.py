"""CPU-side checks of the chunk store's kernel files as compiled for gfx950 (no GPU needed).

The seven files share their vocabulary through csrc/store_device.h: the directory entry and its soundness rule, the directory's
value -> index rule, the workgroup and wavefront sums, the wavefront's copy of its lanes' extents and the grid rules.  Each shared
name is defined exactly once, there, and the entry's bit layout is spelled in no other file.  These kernels are bound by memory and
atomics, so sharing must cost none of the figures that could move them: every kernel has no scratch, no spills, the static LDS it
had with its own copies, and no more VGPRs (a copy loop that lost its sixteen loads in flight shows here as far fewer)."""
import os
import re

import pytest

from conftest import ROOT
from test_fused_isa import _assert_no_scratch, _compile, _field, _kernel_meta, _one

CSRC = os.path.join(ROOT, "compute_war_amd", "csrc")

# (file, kernel, template arguments as mangled): (.vgpr_count, .group_segment_fixed_size) of the commit before the header,
# hipcc -O3 -std=c++17
BEFORE = {
    ("restore_kernels.hip", "restore_chunks_kernel", "ILi0E"): (110, 0),
    ("restore_kernels.hip", "restore_chunks_kernel", "ILi1E"): (108, 0),
    ("restore_kernels.hip", "store_copy_kernel", ""): (30, 0),
    ("restore_kernels.hip", "store_finish_kernel", ""): (4, 0),
    ("restore_kernels.hip", "store_sizes_kernel", ""): (14, 0),
    ("read_kernels.hip", "read_edges_kernel", "ILi0E"): (112, 0),
    ("read_kernels.hip", "read_edges_kernel", "ILi1E"): (110, 0),
    ("read_kernels.hip", "read_pieces_kernel", "ILi0E"): (50, 0),
    ("read_kernels.hip", "read_pieces_kernel", "ILi1E"): (50, 0),
    ("read_kernels.hip", "read_plan_kernel", ""): (16, 0),
    ("store_gc_kernels.hip", "gc_copy_kernel", ""): (112, 0),
    ("store_gc_kernels.hip", "gc_finish_kernel", ""): (6, 0),
    ("store_gc_kernels.hip", "gc_sizes_kernel", ""): (18, 16),
    ("store_gc_kernels.hip", "store_mark_kernel", ""): (10, 16),
    ("renumber_kernels.hip", "renumber_fill_kernel", ""): (8, 0),
    ("renumber_kernels.hip", "renumber_finish_kernel", ""): (5, 0),
    ("renumber_kernels.hip", "renumber_flags_kernel", ""): (14, 16),
    ("renumber_kernels.hip", "renumber_scatter_kernel", ""): (22, 0),
    ("account_kernels.hip", "account_check_kernel", ""): (12, 32),
    ("account_kernels.hip", "account_clear_kernel", ""): (16, 0),
    ("account_kernels.hip", "account_entries_kernel", ""): (51, 32),
    ("account_kernels.hip", "account_positions_kernel", ""): (34, 32),
    ("replicate_kernels.hip", "export_copy_kernel", ""): (64, 0),
    ("replicate_kernels.hip", "export_finish_kernel", ""): (6, 0),
    ("replicate_kernels.hip", "export_sizes_kernel", ""): (15, 0),
    ("replicate_kernels.hip", "import_copy_kernel", ""): (88, 0),
    ("replicate_kernels.hip", "import_finish_kernel", ""): (4, 0),
    ("replicate_kernels.hip", "import_sizes_kernel", ""): (15, 0),
    ("replicate_kernels.hip", "translate_refs_kernel", ""): (16, 16),
    ("scrub_kernels.hip", "scrub_classify_kernel", ""): (14, 0),
    ("scrub_kernels.hip", "scrub_finish_kernel", ""): (24, 16),
    ("scrub_kernels.hip", "scrub_recipe_kernel", ""): (16, 0),
}
FILES = sorted({f for f, _, _ in BEFORE})
# the kernels whose wavefront copies extents with sixteen 16-byte loads in flight per lane: their data alone takes 64 VGPRs
DEEP_COPIES = {"restore_chunks_kernel": 64, "read_edges_kernel": 64, "gc_copy_kernel": 64}


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    return {name: _compile(tmp_path_factory, name) for name in FILES}


def test_the_table_names_every_kernel(asm):
    for f in FILES:
        want = sorted(k + t for g, k, t in BEFORE if g == f)
        got = sorted("".join(g or "" for g in re.search(r"\d([a-z_]+_kernel)(ILi\dE)?", name).groups()) for name in _kernel_meta(asm[f]))
        assert got == want, f


@pytest.mark.parametrize("file,kernel,targs", list(BEFORE), ids=["%s%s" % (k, t) for _, k, t in BEFORE])
def test_store_kernels_keep_their_registers_and_lds(asm, file, kernel, targs):
    name = _one(asm[file], kernel, kernel + targs)
    _assert_no_scratch(asm[file], name)
    meta = _kernel_meta(asm[file])[name]
    vgprs, lds = _field(meta, ".vgpr_count"), _field(meta, ".group_segment_fixed_size")
    print(name, "VGPRs", vgprs, "LDS", lds, "before", BEFORE[file, kernel, targs])
    assert vgprs <= BEFORE[file, kernel, targs][0], (name, vgprs)
    assert lds == BEFORE[file, kernel, targs][1], (name, lds)
    assert vgprs >= DEEP_COPIES.get(kernel, 0), (name, vgprs, "the copy loop no longer keeps its loads in flight")


def _sources():
    for f in sorted(os.listdir(CSRC)):
        if f.endswith((".hip", ".h")):
            yield f, open(os.path.join(CSRC, f)).read()


@pytest.mark.parametrize("pattern", [r"^[^\n/]*__device__[^\n;(]*\bsound\(", r"^[^\n/]*__device__[^\n;(]*\bgroup_sum\(",
                                     r"^[^\n/]*__device__[^\n;(]*\bwave_sum\(", r"^[^\n/]*__device__[^\n;(]*\bwave_copy\(",
                                     r"^[^\n/;=(]*\bunsigned lane_grid\(", r"^[^\n/;=(]*\bunsigned wave_grid\(",
                                     r"^[^\n/;=(]*\bunsigned decode_grid\(", r"\bstruct Entry \{", r"\bstruct Directory \{",
                                     r"\bstruct ScanScratch \{"],
                         ids=["sound", "group_sum", "wave_sum", "wave_copy", "lane_grid", "wave_grid", "decode_grid", "Entry", "Directory",
                              "ScanScratch"])
def test_each_shared_name_is_defined_once(pattern):
    defs = [f for f, text in _sources() for _ in re.finditer(pattern, text, flags=re.M)]
    # (the scan keeps its own wave_sum over unsigned long long: pack_kernels.hip is no store file and includes no store header)
    assert defs == (["pack_kernels.hip", "store_device.h"] if "wave_sum" in pattern else ["store_device.h"]), (pattern, defs)


def test_the_entry_layout_is_spelled_in_one_file():
    assert [f for f, text in _sources() if re.search("0x1ffff", text, flags=re.I)] == ["store_device.h"]
    for f, text in _sources():
        if f in FILES:
            assert '#include "store_device.h"' in text, f
    makefile = open(os.path.join(CSRC, "Makefile")).read()
    assert "store_device.h" in re.search(r"^HDRS\s*:=(.*)$", makefile, flags=re.M).group(1)
