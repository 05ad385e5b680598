"""The built hash inputs (hash_inputs.py) reach the edges they were built for: every property a sliced row is named for, read
from the library's own launch plan (cw_hash_plan_describe, no device), the kernels the one-launch lengths select, the residues
the lengths cover, the poison of the layouts, and the oracle's SHA-256 over the whole set against hashlib."""
import hashlib

import numpy as np
import pytest

import hash_inputs as H


@pytest.fixture(scope="module")
def cw():
    import compute_war_amd as cw
    yield cw
    cw.tune_reset()


def _plan(cw, alg, block_bytes, nblocks, knobs=None, src_misalign=0, digest_misalign=0, may_slice=True):
    """(line 1, [(begin, end, interior)]) of the hash plan under the knobs."""
    with cw.tuned(**(knobs or {})):
        lines = cw.hash_plan_describe(alg, block_bytes, nblocks, src_misalign, digest_misalign, may_slice).split("\n")
    assert lines[-1] == ""
    slices = []
    for ln in lines[1:-1]:
        span, interior = ln.split(" ")
        assert span.startswith("slice=") and interior in ("interior=0", "interior=1"), ln
        b, e = span[6:].split("..")
        slices.append((int(b), int(e), interior == "interior=1"))
    return lines[0], slices


@pytest.mark.parametrize("row", H.SLICED, ids=str)
def test_every_sliced_row_reaches_its_edge(cw, row):
    name, slices = _plan(cw, row.alg, row.block_bytes, H.NBLOCKS_SLICED, row.knobs)
    total, spl = row.total, H.SPL[row.alg]
    assert name in H.KERNELS_SLICED
    # the launches tile [0, total) in order, every one but the last in whole lines
    assert slices[0][0] == 0 and slices[-1][1] == total
    assert all(a[1] == b[0] for a, b in zip(slices, slices[1:]))
    assert all((e - b) % spl == 0 and e > b for b, e, _ in slices[:-1])
    assert len(slices) == row.launches
    assert slices[-1][1] - slices[-1][0] == row.last
    interior = [i for _, _, i in slices]
    assert interior == [True] * (len(slices) - row.tail) + [False] * row.tail
    assert ("true, true" in name) == any(interior)
    if row.alg == "skein":
        assert not any(interior)
    # an interior launch and the line it prefetches lie inside the message
    assert all(e + spl <= total - 1 for _, e, i in slices if i)
    if row.tight:
        assert max(e for _, e, i in slices if i) + spl == total - 1
    assert row.output_only == (slices[-1][:2] == (total - 1, total))
    if row.nslices == 1:
        assert slices == [(0, total, False)]
    if row.nslices == 100000:
        assert all(e - b == spl for b, e, _ in slices[:-1])


def test_the_sliced_rows_cover_every_residue_and_every_slice_kernel(cw):
    for alg in ("skein512", "skein"):
        assert {r.total % H.SPL[alg] for r in H.SLICED if r.alg == alg} == set(range(H.SPL[alg]))
        assert min(r.total for r in H.SLICED if r.alg == alg) == 256
    names = {_plan(cw, r.alg, r.block_bytes, H.NBLOCKS_SLICED, r.knobs)[0] for r in H.SLICED}
    assert names == set(H.KERNELS_SLICED)
    assert {r.tight for r in H.SLICED} == {r.output_only for r in H.SLICED} == {True, False}
    assert H.NBLOCKS_SLICED > 4096 and H.NBLOCKS_SLICED % 64 not in (0, 63)


@pytest.mark.parametrize("row", H.THRESHOLD, ids=str)
def test_the_threshold_rows_lie_on_either_side_of_the_sliced_floor(cw, row):
    name, slices = _plan(cw, row.alg, row.block_bytes, row.nblocks)
    nw = 8 if row.alg == "skein512" else 4
    if row.sliced:
        assert name in H.KERNELS_SLICED and len(slices) == 8
    else:
        assert name == f"cw::skein_lines_kernel<{nw}, true>" and not slices
    # every way out of the sliced launches at a sliced shape: the knob, a misaligned source or digest buffer, a caller that does not slice
    if row.sliced:
        for kw in (dict(knobs=dict(CW_SKEIN_SLICED=0)), dict(src_misalign=8), dict(digest_misalign=4), dict(may_slice=False)):
            assert not _plan(cw, row.alg, row.block_bytes, row.nblocks, **kw)[1], kw


def test_the_one_launch_lengths_select_every_one_launch_kernel(cw):
    seen = set()
    for alg in H.ALGS:
        for knobs in H.KNOB_SETS:
            for mis in (0, 3):
                for n in H.LENGTHS:
                    name, slices = _plan(cw, alg, n, H.PER_LENGTH, knobs, src_misalign=mis)
                    assert not slices
                    seen.add(name)
    assert seen == set(H.KERNELS_ONE_LAUNCH)


def test_the_lengths_cover_every_line_residue():
    assert set(range(386)) <= set(H.LENGTHS) and {65535, 65536} <= set(H.LENGTHS)
    for alg, spl in H.SPL.items():
        bb = H.STEP[alg]
        nmsg = [n // bb for n in range(1, 386) if n % bb == 0]
        assert {(m + 1) % spl for m in nmsg} == set(range(spl))
        assert {1, spl - 1, spl, spl + 1} <= set(nmsg)
        for k in (4096, H.SLICED_FLOOR[alg]):
            assert k % bb == 0 and {k - 1, k, k + 1} <= set(H.LENGTHS)
    assert {55, 56, 63, 64, 119, 120} <= set(H.LENGTHS)   # SHA-256: the padding fits the last chunk / needs one more


def test_the_oracles_sha256_is_hashlibs_over_the_whole_set(oracle):
    for n in H.LENGTHS:
        m = H.messages(n)
        got = H.digests_of(oracle, "sha256", m, n)
        want = np.stack([np.frombuffer(hashlib.sha256(m[i].tobytes()).digest(), np.uint8) for i in range(1 if n == 0 else len(m))])
        assert np.array_equal(got, want), n


def test_families_twins_and_poison():
    for n in (1, 2, 63, 64, 385, 4097):
        m = H.messages(n)
        assert m.shape == (H.PER_LENGTH, n)
        assert not m[0].any() and (m[2] == 0xFF).all() and m[4, -1] == 0x80 and m[6, -1] == 0x00
        for f in range(len(H.FAMILIES)):
            assert H.case(n, 2 * f) == H.Case(H.FAMILIES[f], "base", n) and H.case(n, 2 * f + 1).kind == "twin"
            diff = np.nonzero(m[2 * f] != m[2 * f + 1])[0]
            assert diff.tolist() == [n - 1]
        assert H.case(n, 2 * len(H.FAMILIES)).family == "random"
        if n >= 4:
            assert len({m[i].tobytes() for i in range(len(m))}) == len(m)
    assert H.messages(0).shape == (H.PER_LENGTH, 0)
    for n, stride, shift in ((0, 7, 3), (0, 16, 0), (1, 8, 3), (64, 80, 0), (64, 71, 3), (385, 392, 3), (385, 400, 16)):
        m = H.messages(n)
        buf, gap = H.lay_out(m, stride, shift, seed=n)
        assert buf.size == shift + len(m) * stride + 64 and int(gap.sum()) == buf.size - m.size
        assert buf[gap].all()                                   # poison is never zero
        got = np.stack([buf[shift + i * stride: shift + i * stride + n] for i in range(len(m))])
        assert np.array_equal(got, m) and not gap[shift:shift + n].any()
        behind = buf[shift + np.arange(len(m)) * stride + n]      # the first byte behind every message
        assert gap[shift + np.arange(len(m)) * stride + n].all() and (behind[1:] != behind[:-1]).all()
