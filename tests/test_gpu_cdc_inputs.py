"""The chunker on the GPU over the built inputs of tests/cdc_inputs.py, against cdc_model.chunk (streams_model.chunk_streams for the
stream cases): the offsets, the chunk count and, for streams, the per-stream first index and the verdict are the reference's exactly,
at each case's segments, source shifts and `final`, with every output poisoned behind its valid part.  At every one of those
configurations a single-stream case also goes through cw_dev_cdc_streams with one stream and cw_dev_cdc_streams_part with final 1
and 0, which must give cw_dev_cdc's result.  That each case reaches the
edge it names is established on the CPU (tests/test_cdc_inputs.py).  A failure names (case, segment, shift, final, index of the first
differing cut)."""
import contextlib

import numpy as np
import pytest

import cdc_inputs as X
import streams_ingest_model as XM

pytestmark = pytest.mark.gpu
POISON = 0xABABABABABABABAB
PAD = 8


@pytest.fixture(scope="module")
def cw():
    import torch  # noqa: F401  (one HIP runtime for torch and libcwhc.so)
    import compute_war_amd as cw
    cw.init(0)
    yield cw
    cw.tune_reset()


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _params(cw, p: dict):
    return cw.CdcParams(p["min"], p["avg"], p["max"], p["mask_s"], p["mask_l"], p.get("gear"))


def _poison(n):
    import torch
    return torch.full((n,), POISON - (1 << 64), dtype=torch.int64, device="cuda")


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


@contextlib.contextmanager
def segment(cw, S):
    if S:
        cw.tune_set("CW_CDC_SEGMENT", str(S))
    try:
        yield
    finally:
        if S:
            cw.tune_set("CW_CDC_SEGMENT", None)


class Source:
    """A case's bytes on the device, `shift` bytes into an allocation (allocations are 16-byte aligned: shift is the address mod 16).
    The bytes in front of and behind them are ones that every built gear gives weight to: they must not reach a hash."""

    def __init__(self, data: np.ndarray, shift: int):
        import torch
        self.n = len(data)
        host = np.resize(np.array([7, 3, 1, 2, 255], np.uint8), self.n + shift + 16)
        host[shift:shift + self.n] = data
        self.buf = torch.from_numpy(host).cuda()
        self.ptr = self.buf.data_ptr() + shift
        assert self.ptr % 16 == shift


CALLS = {"n": 0}


def dev_cdc(cw, src: Source, p: dict, final: bool):
    """cw_dev_cdc: (offsets[0..K], poison intact)."""
    import torch
    cp = _params(cw, p)
    cap = cp.max_offsets(src.n)
    offs, k = _poison(cap + PAD), _poison(1 + PAD)
    torch.cuda.synchronize()
    cw.dev_cdc(cp, src.ptr, src.n, final, offs.data_ptr(), cap, k.data_ptr(), _stream())
    torch.cuda.synchronize()
    CALLS["n"] += 1
    offs, k = _u64(offs), _u64(k)
    kk = int(k[0])
    assert kk < cap
    return offs[:kk + 1].tolist(), bool((offs[kk + 1:] == POISON).all() and (k[1:] == POISON).all())


def dev_streams(cw, src: Source, ends, p: dict, final=None):
    """cw_dev_cdc_streams (final = None) or cw_dev_cdc_streams_part: (offsets, first, verdict, poison intact)."""
    import torch
    nf = len(ends)
    d_ends = torch.from_numpy(np.asarray(list(ends) + [0], np.uint64).view(np.int64)).cuda()
    cp = _params(cw, p)
    cap = cp.max_offsets_streams(src.n, nf)
    offs, first, k, result = _poison(cap + PAD), _poison(nf + 1 + PAD), _poison(1 + PAD), _poison(1 + PAD)
    torch.cuda.synchronize()
    if final is None:
        cw.dev_cdc_streams(cp, src.ptr, src.n, d_ends.data_ptr(), nf, offs.data_ptr(), cap, k.data_ptr(), first.data_ptr(), result.data_ptr(),
                           _stream())
    else:
        cw.dev_cdc_streams_part(cp, src.ptr, src.n, d_ends.data_ptr(), nf, final, offs.data_ptr(), cap, k.data_ptr(), first.data_ptr(),
                                result.data_ptr(), _stream())
    torch.cuda.synchronize()
    CALLS["n"] += 1
    offs, first, k, result = _u64(offs), _u64(first), _u64(k), _u64(result)
    kk = int(k[0])
    assert kk < cap
    intact = bool((offs[kk + 1:] == POISON).all() and (first[nf + 1:] == POISON).all() and (k[1:] == POISON).all() and (result[1:] == POISON).all())
    return offs[:kk + 1].tolist(), first[:nf + 1].tolist(), int(result[0]), intact


def first_difference(got, want):
    return next((i for i, (x, y) in enumerate(zip(got, want)) if x != y), min(len(got), len(want)))


def single_forms(cw, src: Source, p: dict, want: dict):
    """One source at the segment that is set, with final 1 and 0: cw_dev_cdc against want[final] (where given), and the stream forms
    with one stream -- cw_dev_cdc_streams_part with the same final, and for final = 1 cw_dev_cdc_streams -- against cw_dev_cdc's
    result.  Returns what differed: (final, form, index of the first differing cut)."""
    bad = []
    for final in (True, False):
        one, intact = dev_cdc(cw, src, p, final)
        if final in want and one != want[final]:
            bad.append((final, "cw_dev_cdc", first_difference(one, want[final])))
        if not intact:
            bad.append((final, "cw_dev_cdc", "poison"))
        expect = (one, [0, len(one) - 1], 0, True)
        forms = [("part", dev_streams(cw, src, [src.n], p, final=final))] + ([("streams", dev_streams(cw, src, [src.n], p))] if final else [])
        bad += [(final, form, first_difference(got[0], one)) for form, got in forms if got != expect]
    return bad


def run_single(cw, names):
    """Every case at each of its segments and shifts: cw_dev_cdc with the case's finals against the model, and the one-stream forms
    against cw_dev_cdc with final 1 and 0."""
    before, failures = CALLS["n"], []
    for name in names:
        c = X.CASES[name]
        want = {final: X.model(name, final) for final in c.finals}
        for shift in c.shifts:
            src = Source(c.data, shift)
            for S in c.segs:
                with segment(cw, S):
                    failures += [(name, S, shift) + bad for bad in single_forms(cw, src, c.params, want)]
    print("cases", len(names), "device calls", CALLS["n"] - before)
    assert not failures, failures[:10]


def test_family_a_cut_rule_default_sizes(cw):
    run_single(cw, [n for n in X.family("A") if X._tag(X.SMALL) in n])


@pytest.mark.parametrize("sizes", X.PARAM_SETS[1:], ids=X._tag)
def test_family_a_cut_rule_other_sizes(cw, sizes):
    run_single(cw, [n for n in X.family("A") if X._tag(sizes) in n])


def test_family_b_tails(cw):
    run_single(cw, X.family("B"))


def test_family_c_runs(cw):
    run_single(cw, X.family("C"))


@pytest.mark.parametrize("shape", ["lone", "hole"])
def test_family_d_bitmap_words_and_summaries(cw, shape):
    run_single(cw, [n for n in X.family("D") if n.startswith("D_" + shape)])


@pytest.mark.parametrize("scheme", X.SCHEMES)
@pytest.mark.parametrize("seg", sorted(X.SEGMENTS))
def test_family_e_segments(cw, seg, scheme):
    run_single(cw, [n for n in X.family("E") if f"_{seg}_" in n and n.endswith(scheme)])


E_OTHER = ("E_periodic_hole_4608seg", "E_late_unmerged", "E_capacity")   # 4.5 MiB at S = 1024, twice; S = 1030


def test_family_e_rows_are_all_run():
    assert all(any(f"_{seg}_" in n for seg in X.SEGMENTS) or n.startswith(E_OTHER) for n in X.family("E"))


@pytest.mark.parametrize("row", E_OTHER)
def test_family_e_many_segments_and_capacity(cw, row):
    names = [n for n in X.family("E") if n.startswith(row)]
    assert len(names) >= 2
    run_single(cw, names)


def test_family_f_scan(cw):
    run_single(cw, X.family("F"))


def test_family_d_level_3(cw):
    failures = []
    for shape, v, off in X.LEVEL3_ROWS:
        c = X.level3_case(shape, v, off)
        cuts = X.model_level3(shape, v, off)
        # final = 0 takes the same steps and stops at the first cut that leaves less than max_size
        stop = next(i for i, x in enumerate(cuts) if x + c.params["max"] > c.n)
        failures += [(shape, v, off) + bad for bad in single_forms(cw, Source(c.data, off), c.params, {True: cuts, False: cuts[:stop + 1]})]
    assert not failures, failures


_PART = {}


def part_model(name):
    """The reference with the last stream open: the complete streams by the stream definition, the open one by chunk(final = False)."""
    if name not in _PART:
        c = X.CASES[name]
        _PART[name] = XM.chunk_part(c.data.tobytes(), list(c.ends), False, c.params)
    return _PART[name]


def run_streams(cw, names):
    before, failures = CALLS["n"], []
    for name in names:
        c = X.CASES[name]
        for shift in c.shifts:
            src = Source(c.data, shift)
            for S in c.segs:
                with segment(cw, S):
                    offsets, first = X.model_streams(name)
                    for form, final in (("streams", None), ("part", True)):
                        got, got_first, verdict, intact = dev_streams(cw, src, c.ends, c.params, final=final)
                        if (got, got_first, verdict, intact) != (offsets, first, 0, True):
                            failures.append((name, S, shift, form, first_difference(got, offsets), first_difference(got_first, first), verdict, intact))
                    offsets, first = part_model(name)
                    got, got_first, verdict, intact = dev_streams(cw, src, c.ends, c.params, final=False)
                    if (got, got_first, verdict, intact) != (offsets, first, 0, True):
                        failures.append((name, S, shift, "open", first_difference(got, offsets), first_difference(got_first, first), verdict, intact))
    print("cases", len(names), "device calls", CALLS["n"] - before)
    assert not failures, failures[:10]


def test_family_g_stream_ends_at_the_edges(cw):
    run_streams(cw, [n for n in X.family("G") if not n.startswith("G_split_")])


BIG = ("G_split_E_periodic_hole_4608seg", "G_split_E_late_unmerged")   # 4.5 MiB each: more than 4096 segments in the stream form


@pytest.mark.parametrize("of", "ABCE")
def test_family_g_inputs_of_other_families_cut_into_streams(cw, of):
    names = [n for n in X.family("G") if n.startswith("G_split_" + of + "_") and not n.startswith(BIG)]
    assert names
    run_streams(cw, names)


@pytest.mark.parametrize("name", [row + "_" + scheme for row in BIG for scheme in X.SCHEMES])
def test_family_g_more_than_4096_segments_cut_into_streams(cw, name):
    assert X.CASES[name].n // X.SMALL[2] > 4096 and X.CASES[name].segs == (X.SMALL[2],)
    run_streams(cw, [name])
