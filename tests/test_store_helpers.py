"""The host-side helpers of compute_war_amd/store.py that need no device: the join of recipes, the sorting and refusing of edits, the
selection of directory entries by value and the value lists of a ScrubReport and of GuardSuspects.  Every expected value is written
out by hand."""
import numpy as np
import pytest

from compute_war_amd._lib import CwError
from compute_war_amd.store import ChunkStore, GuardSuspects, Recipe, ScrubReport, _entry_index, _joined


def u64(*values):
    return np.array(values, np.uint64)


def same(got, want):
    return got.dtype == np.uint64 and got.tolist() == list(want)


def test_joined_no_recipes():
    refs, offs, starts, first = _joined([])
    assert same(refs, []) and same(offs, [0]) and same(starts, [0]) and same(first, [0])


def test_joined_one_recipe():
    refs, offs, starts, first = _joined([Recipe([9, 4, 9], [0, 10, 30, 31])])
    assert same(refs, [9, 4, 9]) and same(offs, [0, 10, 30, 31]) and same(starts, [0, 31]) and same(first, [0, 3])


def test_joined_empty_recipe_in_the_middle_and_a_first_offset():
    a, b, c = Recipe([5, 6], [100, 356, 612]), Recipe([], [7]), Recipe([6, 8, 5], [0, 1, 65537, 65540])
    refs, offs, starts, first = _joined([a, b, c])
    assert same(refs, [5, 6, 6, 8, 5])
    assert same(offs, [0, 256, 512, 513, 66049, 66052])
    assert same(starts, [0, 512, 512, 66052])
    assert same(first, [0, 2, 2, 5])


RECIPE = Recipe([1, 2, 3], [0, 400, 800, 1000])                           # 1000 bytes
REFUSED = [
    ([(100, 50, b"a"), (149, 10, b"b")], "edits overlap: (100, 50) and the one at 149"),
    ([(300, 0, b"new"), (300, 20, b"")], "edits overlap: (300, 0) and the one at 300"),      # an insert shares its offset
    ([(-1, 1, b"x")], "an edit leaves the stream's 1000 bytes"),
    ([(990, 11, b"")], "an edit leaves the stream's 1000 bytes"),                            # ends one byte past nbytes
]


@pytest.mark.parametrize("edits,text", REFUSED)
def test_sorted_edits_refuses(edits, text):
    with pytest.raises(ValueError) as e:
        ChunkStore._sorted_edits(RECIPE, edits)
    assert str(e.value) == text


@pytest.mark.parametrize("edits,text", REFUSED)
def test_patch_many_refuses_before_any_patch(edits, text):
    store = object.__new__(ChunkStore)                                     # (no device: the refusal comes before any of it is used)
    with pytest.raises(ValueError) as e:
        store.patch_many(RECIPE, edits)
    assert str(e.value) == text


def test_sorted_edits_ascend():
    got = ChunkStore._sorted_edits(RECIPE, [(990, 10, b"c"), (500, 0, b"b"), (0, 400, b"a")])
    assert got == [(0, 400, b"a"), (500, 0, b"b"), (990, 10, b"c")]


def test_entry_index_inside():
    idx = _entry_index(u64(5, 12), 5, 8)
    assert idx.dtype == np.int64 and idx.tolist() == [0, 7]
    assert _entry_index(u64(12, 5), 5, 8, report=True).tolist() == [7, 0]
    assert _entry_index(u64(), 5, 8).tolist() == []


@pytest.mark.parametrize("value", [4, 13])
@pytest.mark.parametrize("report,text", [(False, "chunk store: values outside the directory [5, 13)"),
                                         (True, "chunk store: the report names values outside the directory [5, 13)")])
def test_entry_index_outside(value, report, text):
    with pytest.raises(CwError) as e:
        _entry_index(u64(5, value, 12), 5, 8, report=report)
    assert e.value.code == -2 and str(e.value) == "libcwhc error -2: " + text


def test_scrub_report_values():
    report = ScrubReport([0, 1, 2, 3, 4, 5, 0, 3], {}, 5)
    assert same(report.damaged, [6, 7, 8, 12]) and same(report.orphans, [9]) and not report.clean
    assert ScrubReport([0, 4, 5, 0, 0, 0, 0, 0], {}, 5).clean


def test_guard_suspects_values():
    found = GuardSuspects([0, 1, 2, 3, 4, 0, 1, 4], {}, 5)
    assert same(found.located, [6, 8, 11]) and same(found.ambiguous, [7, 8]) and same(found.unprotected, [9, 12])
    assert same(found.suspects, [6, 7, 8, 11])
