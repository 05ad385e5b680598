"""What the past-2^32 GPU tests rest on, proven on the CPU at small sizes (tests/past4g.py): the hand-made cuts'
edges, the chunker's restart property, the tiled recipe, the lifted twin's translation and its guard condition, the sparse guard
walk, and the equivalence that carries patch / compose over a tiled recipe."""
import numpy as np
import pytest

import cdc_model as CM
import compose_model as CPM
import guard2_model as G2
import guard_model as G1
import lifecycle_model as LM
import past4g as P4
import patch_model as PM
import restore_model as RM

D8 = CM.default_params(8192)
SMALL = CM.params(64, 256, 1024, CM.top_bits(10), CM.top_bits(6))


def _noise(seed, n):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def _text(n):
    return (LM.alice() * (n // 100000 + 1))[:n]


# ---- hand-made cuts ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", P4.VARIANTS)
def test_hand_cuts_have_their_edges(variant):
    cuts = P4.hand_cuts(variant).astype(np.int64)
    B, lens = P4.B, np.diff(cuts)
    assert cuts[0] == 0 and cuts[-1] == P4.N and (lens >= 1).all() and (lens <= 65536).all()
    win = P4.window_chunks(cuts)
    assert 200 <= len(win) <= 2000 and cuts[win[0]] == P4.WIN_LO and cuts[win[-1] + 1] == P4.WIN_HI
    outside = np.ones(len(lens), bool)
    outside[win] = False
    assert (lens[outside] == 65536).all() and (cuts[:-1][outside] % 65536 == 0).all()          # the bulk is whole blocks
    assert outside[:win[0]].all() and outside[win[-1] + 1:].all() and win[0] > 0 and win[-1] + 1 < len(lens)
    ends, starts = set(cuts[1:].tolist()), cuts[:-1]
    if variant == "ends":
        assert {B - 1, B, B + 1} <= ends
    else:
        i = int(np.nonzero(starts == B - 17)[0][0])
        assert lens[i] == 65536 and starts[i] % 16 == 15 and starts[i] < B < cuts[i + 1]
    assert (starts[win] % 2 == 1).sum() > 50 and len(set(lens[win].tolist())) > 100           # odd offsets, many lengths
    assert {1, 65536} <= set(lens[win].tolist()) or variant == "straddle"
    P4.assert_reaches(starts[win], cuts[1:][win], variant, over=variant == "straddle")
    assert P4.reaches(starts[win], cuts[1:][win])["over"] == (variant == "straddle")


def test_hand_cuts_scale_down():
    """the same builder around a small b: what the GPU tests' window arithmetic is tried on"""
    cuts = P4.hand_cuts("straddle", n=1 << 20, b=1 << 19, half=1 << 17)
    win = P4.window_chunks(cuts, 1 << 19, 1 << 17)
    assert int(cuts[win[0]]) == (1 << 19) - (1 << 17) and int(cuts[-1]) == 1 << 20 and (np.diff(cuts.astype(np.int64)) > 0).all()


def test_reaches_refuses_one_sided_runs():
    with pytest.raises(AssertionError):
        P4.assert_reaches([0, 10], [10, 20], "below", b=100)
    with pytest.raises(AssertionError):
        P4.assert_reaches([0, 100], [100, 120], "no extent over b", b=100)
    P4.assert_reaches([0, 100], [100, 120], "ends", b=100, over=False)
    P4.assert_reaches([0, 90, 110], [90, 110, 120], "over", b=100)


# ---- the restart property ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("final", [True, False])
@pytest.mark.parametrize("p", [D8, SMALL], ids=["default8192", "small"])
def test_restart_property(p, final):
    """chunk(data)[j:] == c_j + chunk(data[c_j:]) at every cut (every 7th for the small chunks), and the mirror image: the cuts of
    the prefix [0, c_j) with final = False are a head of the whole stream's cuts, and nothing else."""
    n = 10 * p["max"] if p is D8 else 60 * p["max"]
    data = np.frombuffer(_text(n // 2) + _noise(5, n - n // 2 - 3000) + bytes(3000), np.uint8)
    assert p["min"] >= 64
    whole = CM.chunk(data, p, final=final)
    assert len(whole) > 30
    for j in range(0, len(whole), 7):
        c = whole[j]
        assert [c + x for x in CM.chunk(data[c:], p, final=final)] == whole[j:], (j, c)
        head = CM.chunk(data[:c], p, final=False)
        assert head == whole[:len(head)] and (c - head[-1] < p["max"]), (j, c)
        # and a prefix that ends at a cut, carried on from where it stopped, gives the rest (cdc_model.chunk_pieces' contract)
        assert head[:-1] + [head[-1] + x for x in CM.chunk(data[head[-1]:], p, final=final)] == whole, (j, c)


# ---- the tiled recipe ----------------------------------------------------------------------------------------------------------------
def _small_store(oracle, alg="lz4"):
    data = _text(9000) + _noise(3, 3000) + _text(5000)
    cuts = CM.chunk(data, SMALL)
    m = RM.Model(oracle, alg, 1 << 20, 256, dir_base=5)
    refs, _, verdict, _ = m.ingest(data, cuts, 5)
    assert verdict == 0
    return data, cuts, m, refs


@pytest.mark.parametrize("alg", ["lz4", "lzf"])
def test_tiled_recipe_restores_the_tiled_bytes(oracle, alg):
    data, cuts, m, refs = _small_store(oracle, alg)
    R, T, K = 5, len(data), len(refs)
    t_refs, t_off = P4.tiled_recipe(refs, cuts, R)
    assert len(t_refs) == R * K and len(t_off) == R * K + 1 and int(t_off[-1]) == R * T and t_off.dtype == np.uint64
    assert (np.diff(t_off.astype(np.int64)) > 0).all() and t_off[K:2 * K + 1].tolist() == [T + c for c in cuts]
    got = RM.restore(m.blob, m.store_bytes, m.directory, m.dir_base, t_refs, t_off, R * T, m.decode())
    assert all(s == 0 for s, _ in got) and b"".join(piece for _, piece in got) == data * R
    assert P4.tiles_for(T) * T > P4.B + 2 * P4.MIB >= (P4.tiles_for(T) - 1) * T
    e_refs, e_off = P4.tiled_recipe(refs, cuts, 0)
    assert len(e_refs) == 0 and e_off.tolist() == [0]


# ---- the lifted twin: translation and comparator ------------------------------------------------------------------------------------
def _directory():
    d = np.zeros(12, P4.LOC)
    d[1], d[2], d[5], d[9] = (0, 100, 300), (100, 4000, RM.RAW | 4000), (4100, 1, RM.RAW | 1), (4101, 65000, 65536)
    d[10] = (69101, 500, RM.RAW | 500)
    return d


@pytest.mark.parametrize("lift", [0, 1, P4.B - 2000, P4.B, (1 << 40) + 3])
def test_translation_and_comparator(lift):
    plain = _directory()
    twin = P4.translate(plain, lift)
    assert twin["pos"].tolist() == [0, lift, lift + 100, 0, 0, lift + 4100, 0, 0, 0, lift + 4101, lift + 69101, 0]
    assert (twin["stored"] == plain["stored"]).all() and (twin["raw"] == plain["raw"]).all()
    assert P4.same_directory(plain, twin, lift) is None
    assert P4.same_directory(plain.view(np.int64), twin.view(np.int64), lift) is None            # as the device holds it: i64 pairs
    for off in (1 << 32, -(1 << 32), 16, -1):                                                   # one entry's pos off, either way
        for i in (1, 9):
            wrong = twin.copy()
            wrong["pos"][i] = np.uint64((int(wrong["pos"][i]) + off) % (1 << 64))
            bad = P4.same_directory(plain, wrong, lift)
            assert bad is not None and bad[0] == i and bad[3] == 1, (off, i, bad)
    if lift:
        wrong = twin.copy()
        wrong["pos"][3] = np.uint64(lift)                                                      # an empty entry that was lifted
        assert P4.same_directory(plain, wrong, lift)[0] == 3
    wrong = twin.copy()
    wrong["stored"][2] += 1
    assert P4.same_directory(plain, wrong, lift)[0] == 2
    assert P4.same_directory(plain, twin[:-1], lift)[0] == -1
    if lift:
        assert P4.same_directory(plain, plain, lift) is not None and P4.same_directory(plain, twin, 0) is not None


def test_a_high_half_lost_is_seen():
    """the fault the lifted twin exists for: pos written or read as 32 bits"""
    plain = _directory()
    lift = P4.lift_over(plain)
    twin = P4.translate(plain, lift)
    s, e = P4.extents(twin)
    P4.assert_reaches(s, e, "lift_over")
    assert P4.reaches(s, e) == dict(below=3, above=1, over=1)
    low = twin.copy()
    low["pos"] &= np.uint64(0xFFFFFFFF)
    bad = P4.same_directory(plain, low, lift)
    assert bad is not None and bad[0] == 10 and bad[3] == 1                                  # (the one entry above 2^32)


def test_guard_lift_is_whole_groups():
    for stripe, group in ((65536, 2), (65536, 3), (65536, 255), (1 << 20, 16), (1 << 30, 3)):
        W = stripe * group
        for peak in (0, 1, 30000, 400000, 5 << 20):
            L = P4.guard_lift(peak, W)
            assert L % W == 0 and (L < P4.B < L + peak or P4.B <= L < P4.B + W)
            assert P4.guard_lift(peak, W, over=False) == -(-P4.B // W) * W >= P4.B
    assert P4.guard_lift(65537, 65536 * 255) == P4.B - 65536 == 65536 * 255 * 257         # the dual guard's largest group: one stripe below B
    assert P4.guard_lift(30000, 65536 * 3) == P4.B + 131072 and P4.guard_lift(70000, 65536 * 3) == P4.B - 65536
    assert P4.guard_lift(30000, 65536 * 2) == P4.B


@pytest.mark.parametrize("G", [2, 3, 5])
def test_the_twins_guard_is_a_shift_only_for_whole_groups(G):
    S, used = 65536, 3 * 65536 + 777
    plain = np.frombuffer(_noise(G, used), np.uint8)
    sb = 8 * S
    for groups_up in (1, 3):
        lift = groups_up * G * S
        twin = np.concatenate([np.zeros(lift, np.uint8), plain])
        p0, q0 = G2.guards_of(plain, used, S, G, sb)
        p1, q1 = G2.guards_of(twin, lift + used, S, G, lift + sb)
        assert np.array_equal(p0, G1.guard_of(plain, used, S, G, sb))
        assert P4.same_guard(p0, p1, lift, S, G) is None and P4.same_guard(q0, q1, lift, S, G) is None
        wrong = p1.copy()
        wrong[5] ^= 1                                                                       # a byte folded 2^32-style too low
        assert P4.same_guard(p0, wrong, lift, S, G) is not None
        wrong = q1.copy()
        wrong[lift // (G * S) * S + 9] ^= 1
        assert P4.same_guard(q0, wrong, lift, S, G) is not None
    # a lift of a whole stripe that is no whole group moves every member: Q is no shift of the plain Q then
    lift = S
    twin = np.concatenate([np.zeros(lift, np.uint8), plain])
    _, q1 = G2.guards_of(twin, lift + used, S, G, lift + sb)
    _, q0 = G2.guards_of(plain, used, S, G, sb)
    assert not np.array_equal(q1[:len(q0)], q0)
    with pytest.raises(AssertionError):
        P4.same_guard(q0, q1, lift, S, G)


@pytest.mark.parametrize("G", [3, 16])
def test_zero_bytes_add_nothing_to_a_guard(G):
    """the sparse walk of the 4 GiB images: folding only the range that holds the non-zero bytes equals the walk of the whole image,
    for P as for Q"""
    S, sb = 65536, 40 * 65536
    lo, hi = 19 * S - 5000, 19 * S + 7000
    image = np.zeros(sb, np.uint8)
    image[lo:hi] = np.frombuffer(_noise(G, hi - lo), np.uint8)
    p_full, q_full = G2.guards_of(image, sb, S, G, sb)
    p, q = np.zeros_like(p_full), np.zeros_like(q_full)
    G1.fold(p, image, lo, hi, S, G)
    G2.fold_q(q, image, lo, hi, S, G)
    assert np.array_equal(p, p_full) and np.array_equal(q, q_full) and p.any() and q.any()


def test_lifted_run_leaves_out_only_scripts_that_save(oracle):
    """the cap of the lifted life-cycle run: ``save`` writes [0, used) to a file, 4 GiB of zeros for a twin"""
    saving = [n for n in LM.NAMES if any(op == "save_load" for op, _, _ in LM.script(oracle, "lz4", n)["steps"])]
    assert saving == ["streamed_and_reloaded", "guarded_refusals"]


# ---- patch / compose over a tiled recipe ---------------------------------------------------------------------------------------------
def _ids(table, data, cuts):
    return [table.setdefault(bytes(data[a:b]), len(table)) for a, b in zip(cuts[:-1], cuts[1:])]


def _tiled(R):
    a = _text(7000) + _noise(21, 2500) + _text(6000)
    cuts = CM.chunk(a, SMALL)
    table = {}
    refs = _ids(table, a, cuts)
    t_refs, t_off = P4.tiled_recipe(refs, cuts, R)
    return a, cuts, refs, table, t_refs, [int(v) for v in t_off]


EDITS = [("write", 3, lambda T: (T + 4000, 700, _noise(31, 700))),                           # (name, tiles of the short run, the edit in them)
         ("insert", 3, lambda T: (T + 9000, 0, _noise(32, 1300))),
         ("cut_out", 3, lambda T: (T + 2000, 5000, b"")),
         ("append", 2, lambda T: (2 * T, 0, _noise(33, 3000))),
         ("truncate", 2, lambda T: (2 * T - 3100, 3100, b""))]


@pytest.mark.parametrize("name,m,edit", EDITS, ids=[e[0] for e in EDITS])
@pytest.mark.parametrize("R", [6, 9])
def test_patch_of_a_tiled_recipe_is_the_short_patch_spliced(R, name, m, edit):
    a, cuts, refs, table, t_refs, t_off = _tiled(R)
    T = len(a)
    head = R - m if name in ("append", "truncate") else R - 4                                # an edit at the end has no tile behind it
    at, r, ins = edit(T)
    _, s_off = P4.tiled_recipe(refs, cuts, m)
    s_off = [int(v) for v in s_off]
    j, t, s, short_cuts, _ = PM.patch(a * m, s_off, SMALL, at, r, ins)
    J, t2, s2, long_cuts, _ = PM.patch(a * R, t_off, SMALL, head * T + at, r, ins)
    K = len(refs)
    assert (J, t2) == (j + head * K, t) and s2 - head * K == s
    assert head + m == R or s < m * K, "the short run resynchronised before its end"
    short_refs = _ids(table, PM.edited(a * m, at, r, ins), short_cuts)
    long_refs = _ids(table, PM.edited(a * R, head * T + at, r, ins), long_cuts)
    want_refs, want_off = P4.spliced(refs, cuts, R, head, m, short_refs, short_cuts)
    assert want_off.tolist() == long_cuts and want_refs.tolist() == long_refs


@pytest.mark.parametrize("R", [6, 9])
def test_compose_of_a_tiled_recipe_is_the_short_compose_spliced(R):
    a, cuts, refs, table, t_refs, t_off = _tiled(R)
    T, head, m = len(a), R - 4, 3
    new1, new2 = _noise(41, 900), _noise(42, 50)

    def parts(base, end):                                                                   # two splices inside tile base / T + 1
        x, y, z = base + T + 3000, base + T + 5000, base + T + 11000
        return [("copy", 0, x), ("new", new1), ("copy", y, z - y), ("new", new2), ("copy", z + 10, end - z - 10)]

    _, s_off = P4.tiled_recipe(refs, cuts, m)
    s_off = [int(v) for v in s_off]
    ops, payload = CPM.tile(parts(0, m * T))
    short = CPM.compose(a * m, s_off, [0, len(s_off) - 1], ops, payload, SMALL)
    ops, payload = CPM.tile(parts(head * T, R * T))
    long = CPM.compose(a * R, t_off, [0, len(t_off) - 1], ops, payload, SMALL)
    assert long["bytes"] == (a * head) + short["bytes"] + a * (R - head - m)
    assert long["stats"]["rebuilt_chunks"] == short["stats"]["rebuilt_chunks"] and long["stats"]["rebuilt_bytes"] == short["stats"]["rebuilt_bytes"]
    want_refs, want_off = P4.spliced(refs, cuts, R, head, m, _ids(table, short["bytes"], short["cuts"]), short["cuts"])
    assert want_off.tolist() == long["cuts"] and want_refs.tolist() == _ids(table, long["bytes"], long["cuts"])
    # concat: the offsets of [tiled, tiled] are the tiled offsets of twice as many tiles, but for the chunks around the joint (the
    # first stream's last chunk was cut by its end, and the result is chunked as one stream)
    both = CPM.compose(a * R * 2, t_off + [R * T + c for c in t_off[1:]], [0, len(t_off) - 1, 2 * (len(t_off) - 1)],
                       *CPM.tile([("copy", 0, 2 * R * T)]), SMALL)
    twice = [int(v) for v in P4.tiled_recipe(refs, cuts, 2 * R)[1]]
    odd = sorted(set(both["cuts"]) ^ set(twice))
    assert both["cuts"][-1] == 2 * R * T and len(odd) <= 16 and all(R * T - SMALL["max"] < c < R * T + 8 * SMALL["max"] for c in odd)
