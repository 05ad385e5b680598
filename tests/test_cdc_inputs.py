"""The chunker's built inputs (tests/cdc_inputs.py) reach the edges they name: established on the CPU, from the models alone.

Per case: the classes that cdc_model.window_hash gives are the classes the builder asked for at every position; cdc_model.chunk
and cdc_model.chunk_serial agree (up to 256 KiB); the cuts the case is named for are in the model's chain; and for the stream cases
the per-stream definition equals the one chain over the concatenation.  Nothing here is asserted from a copy of the device code."""
import numpy as np
import pytest

import cdc_inputs as X
import cdc_model as CM
import streams_model as SM

FAMILIES = "ABCDEFG"


def _own_data(name):
    """False for a family G case that shares the bytes of another case."""
    c = X.CASES[name]
    return not (c.note or {}).get("of")


def _cuts(name):
    c = X.CASES[name]
    return X.model_streams(name)[0] if c.ends else X.model(name, True)


def _diffs_from(cuts, start, stride):
    """How many differences in a row equal `stride`, from the cut `start` on."""
    i = cuts.index(start)
    k = 0
    while i + k + 1 < len(cuts) and cuts[i + k + 1] - cuts[i + k] == stride:
        k += 1
    return k


@pytest.mark.parametrize("scheme", X.SCHEMES)
def test_a_scheme_emits_any_class_sequence(scheme):
    rng = np.random.default_rng(7)
    for trial in range(2000):
        k = rng.integers(0, 3, int(rng.integers(1, 200)), dtype=np.uint8)
        data, p = X.emit(k, scheme)
        assert (X.classes_of(data, p) == k).all(), (scheme, trial)
    p = X.scheme_params(scheme)
    assert ((p["mask_s"] | p["mask_l"]) & 0xFFFFFFFF == 0) == (scheme == "hi")       # hi: the scan's high-word-only variant
    assert ((p["mask_s"] | p["mask_l"]) >> 32 == 0) == (scheme == "lo")


def test_the_delay_gear_delays_by_k():
    for k in range(64):
        lone = [0, 5, 64, 100, 101, 4000]
        data, p, cands = X.delay(5000, lone, k)
        got = X.classes_of(data, p)
        assert set(np.unique(got)) <= {X.N, X.B}
        assert np.flatnonzero(got == X.B).tolist() == sorted(set(range(k)) | {q + k for q in lone}) == cands.tolist()


@pytest.mark.parametrize("family", FAMILIES)
def test_emitted_classes_are_the_classes_asked_for(family):
    seen = 0
    for name in X.family(family):
        c = X.CASES[name]
        if not _own_data(name) or (c.classes is None and c.cands is None):
            continue
        got = X.classes_of(c.data, c.params) if c.n else np.zeros(0, np.uint8)
        if c.classes is not None:
            assert (got == c.classes).all(), (name, int(np.flatnonzero(got != c.classes)[0]))
        else:
            assert set(np.unique(got)) <= {X.N, X.B} and np.flatnonzero(got == X.B).tolist() == c.cands.tolist(), name
            k = c.params["mask_s"].bit_length() - 1
            lone = np.flatnonzero(c.data != 7)
            assert c.cands.tolist() == sorted(set(range(k)) | {int(q) + k for q in lone if q + k < c.n}), name
        seen += 1
    assert seen or family == "G"
    print(family, "cases checked", seen)


@pytest.mark.parametrize("family", FAMILIES)
def test_the_two_models_agree(family):
    seen, done = 0, set()
    for name in X.family(family):
        c = X.CASES[name]
        if c.n > (256 << 10) or id(c.data) in done or not _own_data(name):
            continue
        done.add(id(c.data))
        raw = c.data.tobytes()
        for final in (True, False):
            want = CM.chunk_serial(raw, c.params, final=final)
            assert (X.model(name, final) if not c.ends else CM.chunk(c.data, c.params, final=final)) == want, (name, final)
        seen += 1
    print(family, "cases checked", seen)


@pytest.mark.parametrize("family", FAMILIES)
def test_the_named_edge_is_in_the_models_cuts(family):
    seen = 0
    for name in X.family(family):
        c = X.CASES[name]
        if not (c.has or c.hasnt or c.prog):
            continue
        cuts = _cuts(name)
        assert cuts[0] == 0 and cuts[-1] == c.n and (np.diff(cuts) > 0).all(), name
        have = set(cuts)
        assert all(x in have for x in c.has), (name, [x for x in c.has if x not in have])
        assert not any(x in have for x in c.hasnt), (name, [x for x in c.hasnt if x in have])
        if c.prog:
            start, stride, count = c.prog
            k = _diffs_from(cuts, start, stride)
            assert (k >= 2) if count is None else (k == count), (name, c.prog, k)
        seen += 1
    assert seen >= {"A": 170, "B": 40, "C": 90, "D": 0, "E": 20, "F": 12, "G": 14}[family]
    print(family, "cases checked", seen)


def test_family_a_has_every_row_in_every_parameter_set_that_admits_it():
    for sizes in X.PARAM_SETS:
        rows = {n.split("_c")[0] for n in X.family("A") if X._tag(sizes) in n}
        # m == M leaves the rows at c+m-1, c+m, e and none; a == M drops the rows that need room between z and e
        assert len(rows) >= (4 if sizes[0] == sizes[2] else 8 if sizes[1] == sizes[2] else 9), (sizes, rows)
    m, a, M = X.PARAM_SETS[-1]
    assert any(v & (v - 1) for v in (m, a, M))
    assert any(c.has and c.has[-1] % 64 for n, c in X.CASES.items() if c.family == "A")  # a start c that is no multiple of 64


def test_family_b_tails_end_where_they_say():
    m, a, M = X.SMALL
    for t in (1, m - 1, m, m + 1, a - 1, a, a + 1, M - 1, M, M + 1):
        for name in (f"B_tail{t}_bare_hi", f"B_tail{t}_cand_lo"):
            cuts = X.model(name, True)
            before = [c for c in cuts if c < X.CASES[name].n]
            assert X.C0 in cuts and cuts[-1] - X.C0 == t and cuts[-1] - before[-1] == (t if t <= M else t - M), name
            open_ = X.model(name, False)
            assert open_ == [c for c in cuts if c <= open_[-1]] and open_[-1] + M > X.CASES[name].n, name
    assert X.model("B_n0_hi", True) == [0] == X.model("B_n0_hi", False)
    assert X.model("B_n1_cand_lo", True) == [0, 1] and X.model("B_n1_cand_lo", False) == [0]


def test_family_d_the_lone_position_is_where_the_summaries_end():
    m, a, M = X.SMALL
    seen = set()
    for name in X.family("D"):
        c = X.CASES[name]
        off = c.shifts[0]
        assert len(c.shifts) == 1 and c.lone + off == c.virtual, name
        hole = "hole" in name
        fill = X.B if hole else X.N
        body = X.classes_of(c.data, c.params)[c.body:]
        odd = np.flatnonzero(body != fill) + c.body
        assert odd.tolist() == [c.lone] and body[c.lone - c.body] == (X.N if hole else X.B if "both" in name else X.L), name
        seen.add((c.virtual, off))
        if "_end_" in name:           # every search to n ends in the group's first word, and the lone cut is a cut
            assert c.virtual % 4096 == 0 and (c.n + off - 1) >> 6 == c.virtual >> 6 and c.lone + 1 in X.model(name, True), name
        elif c.virtual >= 262143:     # the run is entered behind the prefix and crossed by a progression up to the lone position
            cuts = X.model(name, True)
            i = int(np.searchsorted(cuts, c.lone))
            stride = c.params["min"] if hole else M
            assert c.body == X.PREFIX and set(np.diff(cuts[i - 40:i - 1]).tolist()) == {stride}, name
            first = next(x for x in cuts if x >= X.PREFIX)
            assert first % stride, name                                    # an odd phase
    assert seen == {(v, off) for v in X.VIRTUAL for off in X.OFFS}
    # word, level-1 and level-2 edges: the last bit of one group and the first of the next
    assert {v % 64 for v in X.VIRTUAL} == {63, 0} and {4095 // 4096, 4096 // 4096} == {0, 1} and 262144 == 64 ** 3


def test_family_d_level_3_inputs():
    assert 16777216 == 64 ** 4 and X.LEVEL3 == (16777215, 16777216)
    assert {(s, v) for s, v, _ in X.LEVEL3_ROWS} == {(s, v) for s in ("lone", "hole") for v in X.LEVEL3}
    for shape in ("lone", "hole"):
        assert {off for s, _, off in X.LEVEL3_ROWS if s == shape} == {0, 15}
    for shape, v, off in X.LEVEL3_ROWS:
        c = X.level3_case(shape, v, off)
        assert c.n + off > 16 << 20 and c.lone + off == v and c.shifts == (off,)
        got = X.classes_of(c.data, c.params)
        assert (got == c.classes).all()
        fill = X.N if shape == "lone" else X.B
        assert (np.flatnonzero(got[c.body:] != fill) + c.body).tolist() == [c.lone]
        cuts = X.model_level3(shape, v, off)
        i = int(np.searchsorted(cuts, c.lone))
        stride = c.params["max"] if shape == "lone" else c.params["min"]
        assert set(np.diff(cuts[i - 1000:i - 1]).tolist()) == {stride} and next(x for x in cuts if x >= X.PREFIX) % stride
        assert all(x in cuts for x in c.has)
        if c.has:                     # the buffer ends in the first word of the second 16 MiB group, where the lone cut is taken
            assert (c.n + off - 1) >> 6 == v >> 6 == 1 << 18


def test_family_e_segments():
    m, a, M = X.SMALL
    for name in X.family("E"):
        c = X.CASES[name]
        note = c.note or {}
        if not note:
            continue
        S = note["S"]
        assert c.segs == (None if S == X.DEFAULT_SEGMENT else S,), name
        cs, cl = X.candidates(c.classes)
        cuts = X.model(name, True)
        if "spec_exit" in note:
            for g in note["spec_exit"]:
                own = X.chain(cs, cl, c.n, c.params, start=g * S, stop=(g + 1) * S)
                assert own[-1] == (g + 1) * S and own[-2] < (g + 1) * S, (name, g)
        if "capacity" in note:
            assert SM.max_cuts_in_a_segment(cuts, S) == note["capacity"] == -(-S // m) and S // m + 2 >= note["capacity"], name
        if "unmerged_row" in note or "nseg" in note or "first_unmerged" in note:
            assert cuts == X.chain(cs, cl, c.n, c.params)
            un = X.unmerged_segments(cs, cl, c.n, c.params, S, cuts)
            nseg = c.n // S + 1
            print(name, "segments", nseg, "unmerged", len(un), "longest row", X.longest_row(un), "first", un[:1])
            if "unmerged_row" in note:
                assert (X.longest_row(un) > 64) if note["unmerged_row"] else not un, name
            if "nseg" in note:
                assert nseg > 4096 and X.longest_row(un) > 4096, name
            if "first_unmerged" in note:
                assert nseg > 4096 and un[0] > 4096 + 64 and X.longest_row(un) > 64, name
    for stag, S in X.SEGMENTS.items():
        assert X.CASES[f"E_n_S_{stag}_hi"].n == S and X.CASES[f"E_n_S-1_{stag}_lo"].n == S - 1 and X.CASES[f"E_n_S+1_{stag}_lo"].n == S + 1
        assert X.CASES[f"E_n_5S_{stag}_hi"].n == 5 * S
        name = f"E_open_5S+100_{stag}_hi"
        last = X.model(name, False)[-1]
        assert X.CASES[name].finals == (False,) and last + M > X.CASES[name].n and last // S < X.CASES[name].n // S, name


def test_family_f_scan_edges():
    for nv in X.SPAN_EDGES:
        for off in (0, 1, 15):
            for gear, hi in (("default", True), ("delay", True), ("delay31", False)):   # hi: the scan tests the high word only
                c = X.CASES[f"F_span_{nv}_off{off}_{gear}"]
                assert c.n + off == nv and c.shifts == (off,) and c.finals == (False,)
                assert ((c.params["mask_s"] | c.params["mask_l"]) & 0xFFFFFFFF == 0) == hi
                assert X.classes_of(c.data, c.params)[-1] != X.N                       # a candidate at position n - 1
    for k in X.WINDOW_K:
        for off in (0, 5):
            c = X.CASES[f"F_window_k{k}_off{off}"]
            p = c.params
            assert p["mask_s"] == p["mask_l"] == 1 << k and (p["mask_s"] & 0xFFFFFFFF == 0) == (k >= 32)
            lone = np.flatnonzero(c.data != 7) + off                                    # virtual
            if k:
                for edge in (320, 4096, 12288):
                    assert edge - 1 in lone and edge - 1 + k - off + 1 in c.has          # p = B - 1 < p + k
                for edge in (1344, 8192, 16384):
                    assert edge - k in lone and edge - off + 1 in c.has                  # p + k = B
    p = X.BOTH_WORDS
    assert all(w for v in (p["mask_s"], p["mask_l"]) for w in (v & 0xFFFFFFFF, v >> 32)) and len(X.model("F_both_words")) > 100


def test_family_g_the_stream_definition_equals_the_one_chain():
    m, a, M = X.SMALL
    for name in X.family("G"):
        c = X.CASES[name]
        assert c.ends[-1] == c.n and list(c.ends) == sorted(c.ends), name
        offsets, first = X.model_streams(name)
        assert (offsets, first) == SM.chunk_chain(X.streams_of(c), c.params), name
        assert all(e in offsets for e in c.ends), name
    one = X.model_streams("G_one_byte_chunk_hi")[0]
    assert 1 in np.diff(one).tolist()
    offsets, first = X.model_streams("G_300_one_byte_streams_lo")
    assert np.diff(first)[1:301].tolist() == [1] * 300
    c = X.CASES["G_open_within_max_hi"]
    assert c.n - c.ends[-2] < M
