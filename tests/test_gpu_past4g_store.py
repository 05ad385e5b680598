"""A store whose bytes lie past 2^32.  Every life-cycle script of tests/lifecycle_model.py that does not save
to a file runs step by step on two device stores at once: the ordinary one, as tests/test_gpu_lifecycle.py runs it (that test ties it
to the model), and a *lifted twin* of ``L + store_bytes`` bytes whose cursor starts at ``L`` just below 2^32, so that the stored bytes,
every ``Entry::pos``, ``*d_used`` and the guard's cursor cross 2^32 while the script runs.  After every step the twin's state has to be
the ordinary store's under ``pos -> pos + L`` (tests/past4g.py): the cursor, every stored byte (with nothing but zeros below ``L``),
every directory entry, the index, the recipes, ``restore(verify=True)`` of every live stream, and of a protected store the guard moved
up by ``L / W`` whole groups, its cursor and ``guard_check``.  Every result a step returns is compared with the model's, as for the
ordinary store, with the positions in it translated.  A lift is a whole number of guard groups for a store that gets protected
(tests/past4g.py says why), so the unguarded scripts' protected twins start at or just above 2^32; the guarded scripts, whose stores
hold a few stripes, and the dual guard at 255 stripes a group lie across it."""
import math

import numpy as np
import pytest

import lifecycle_model as LM
import past4g as P4
from test_gpu_lifecycle import Env

pytestmark = pytest.mark.gpu
ALGS = ["lz4", "lzf"]
B, MIB = P4.B, P4.MIB
SAVING = ("streamed_and_reloaded", "guarded_refusals")                       # ``save`` writes [0, used): 4 GiB of zeros for a twin
LIFTED = tuple(n for n in LM.NAMES if n not in SAVING)


@pytest.fixture(scope="module")
def cw():
    import torch  # noqa: F401  (one HIP runtime for torch and libcwhc.so)
    import compute_war_amd as cw
    cw.init(0)
    yield cw
    cw.tune_reset()


# ---- where to lift ------------------------------------------------------------------------------------------------------------------
def geometries(sc):
    """{store: [(stripe, group)]} of every protect step."""
    out = {}
    for op, args, _ in sc["steps"]:
        if op == "protect":
            out.setdefault(args.get("store", "P"), []).append((args.get("stripe", 65536), args.get("group", 16)))
    return out


def plan(oracle, alg, sc):
    """({store: lift}, {store: what to reach}).  The first store's stored bytes lie over 2^32: by the model's directory when the store
    holds the most before its first compact, 2^32 falls into the middle of a stored chunk.  The other stores start at 2^32.  A store
    that gets protected takes a multiple of its groups' size W: the largest one below 2^32 when its bytes then still pass 2^32, else the
    first one from 2^32 on."""
    models = LM.new_stores(oracle, alg, sc["specs"])
    most, peak, moved = {n: None for n in models}, {n: 0 for n in models}, set()
    for op, args, expect in sc["steps"]:
        if op == "compact" and expect == 0:
            moved.add(args.get("store", "P"))
        LM.run(models, op, args)
        for n, m in models.items():
            if n not in moved and m.used:
                most[n], peak[n] = m.m.directory.copy(), m.used
    lifts, reach, geo = {}, {}, geometries(sc)
    for i, n in enumerate(sc["specs"]):
        lift = P4.lift_over(most[n]) if i == 0 and most[n] is not None else B
        if n in geo:
            lift = P4.guard_lift(peak[n], math.lcm(*[s * g for s, g in geo[n]]), over=i == 0)
        lifts[n] = lift
        reach[n] = "above" if lift >= B else "over" if n not in geo else "both"
    return lifts, reach


# ---- the twin -------------------------------------------------------------------------------------------------------------------------
class Twin(Env):
    """``Env`` over lifted stores; ``lift`` is tracked per store (0 after a compact: the new buffer is filled from 0)."""

    def __init__(self, cw, oracle, alg, specs, tmp_path, lifts):
        import torch
        self.cw, self.oracle, self.tmp_path, self.stores, self.recipes, self.reports = cw, oracle, tmp_path, {}, {}, {}
        self.lift = dict(lifts)
        for name, kw in specs.items():
            cs = cw.ChunkStore(cw.DedupeIndex("skein512", kw["max_entries"]), alg, cw.CdcParams.default(256), lifts[name] + kw["store_bytes"],
                               kw["dir_entries"], kw["dir_base"])
            cs.d_used.fill_(lifts[name])
            self.stores[name] = cs
        torch.cuda.synchronize()

    def groups_up(self, name):
        cs = self.stores[name]
        W = cs.stripe * cs.group
        assert self.lift[name] % W == 0, (name, self.lift[name], W)
        return self.lift[name] // W

    def step(self, op, args, want):
        args, want = dict(args), dict(want)
        name = args.get("store", "P")
        cs, L = self.stores[name], self.lift[name]
        if op in ("corrupt", "corrupt_unlisted"):
            want["pos"] += L
        elif op == "corrupt_guard":
            want["at"] += self.groups_up(name) * cs.stripe
        elif op == "guard_check":
            want["groups"] = [g + self.groups_up(name) for g in want["groups"]]
        elif op == "compact":
            if args.get("store_bytes") is None:
                args["store_bytes"] = cs.store_bytes - L                     # the new store is as large as the ordinary one's
            if "bytes_before" in want:
                want["bytes_before"] += L
        super().step(op, args, want)
        if op == "compact":
            self.lift[name] = 0

    def guard_window(self, name):
        cs = self.stores[name]
        if cs.d_guard is None:
            return None
        at = self.groups_up(name) * cs.stripe
        return (cs.stripe, cs.group, cs.protected_bytes(), cs.d_guard[at:].cpu().numpy().tobytes(),
                None if cs.d_guard_q is None else cs.d_guard_q[at:].cpu().numpy().tobytes())

    def state(self):
        """What a refused step must leave alone: ``device_state`` of tests/test_gpu_lifecycle.py, of the bytes from the lift on."""
        out = {}
        for name, cs in self.stores.items():
            dig, val = cs.index.export()
            L = self.lift[name]
            out[name] = (frozenset((bytes(d), int(v)) for d, v in zip(dig, val)), cs.d_dir.cpu().numpy().tobytes(), cs.used(),
                         cs.d_store[L:cs.used()].cpu().numpy().tobytes(), cs.base, cs.dir_base, cs.dir_entries, cs.store_bytes,
                         self.guard_window(name), self.nothing_below(name))
        return out

    def nothing_below(self, name):
        """No byte below the lift was written: a position that lost its high half lands there."""
        cs, L = self.stores[name], self.lift[name]
        quiet = not bool(cs.d_store[:L].any())
        if cs.d_guard is not None:
            at = self.groups_up(name) * cs.stripe
            quiet = quiet and not bool(cs.d_guard[:at].any()) and (cs.d_guard_q is None or not bool(cs.d_guard_q[:at].any()))
        return quiet

    def same_as_plain(self, plain, models, where):
        import torch
        for name, t in self.stores.items():
            o, L, m, at = plain.stores[name], self.lift[name], models[name], (where, name)
            assert t.used() == o.used() + L and t.store_bytes == o.store_bytes + L, (at, t.used(), o.used(), L)
            assert torch.equal(t.d_store[L:], o.d_store), (at, "stored bytes", (t.d_store[L:] != o.d_store).nonzero()[:4].tolist())
            assert self.nothing_below(name), (at, "a byte below the lift was written")
            bad = P4.same_directory(o.d_dir.cpu().numpy(), t.d_dir.cpu().numpy(), L)
            assert bad is None, (at, "entry", bad)
            have, want = [frozenset((bytes(d), int(v)) for d, v in zip(*cs.index.export())) for cs in (t, o)]
            assert have == want, (at, "index", len(have), len(want))
            assert (t.base, t.dir_base, t.dir_entries) == (o.base, o.dir_base, o.dir_entries), at
            assert (t.d_guard is None) == (o.d_guard is None) and (t.d_guard_q is None) == (o.d_guard_q is None), at
            if o.d_guard is not None:
                up = self.groups_up(name)
                assert (t.stripe, t.group) == (o.stripe, o.group) and t.protected_bytes() - L == o.protected_bytes() == o.used(), (at, "cursor")
                for tg, og in ((t.d_guard, o.d_guard), (t.d_guard_q, o.d_guard_q)):
                    if og is not None:
                        assert P4.same_guard(og, tg, L, t.stripe, t.group, equal=torch.equal) is None, (at, "guard")
                count, groups, bits = o.guard_check(detail=True)
                assert t.guard_check(detail=True) == (count, [g + up for g in groups], bits), (at, "guard_check")
            for stream, st in m.streams.items():
                ro, rt = plain.recipes[name, stream], self.recipes[name, stream]
                assert np.array_equal(ro.refs, rt.refs) and np.array_equal(ro.offsets, rt.offsets), (at, stream, "recipe")
                if not m.hurt:
                    assert t.restore(rt, verify=True) == st.bytes, (at, stream, "restore")


def lifted_run(cw, oracle, tmp_path, alg, sc, lifts=None, reach=None):
    """The script on the ordinary stores and on their twins.  ``reach[store]``: "over" = compared entries and cursors on both sides of
    2^32 and an entry across it, "both" = on both sides, "above" = everything from 2^32 on."""
    planned = plan(oracle, alg, sc)
    lifts, reach = planned[0] if lifts is None else lifts, planned[1] if reach is None else reach
    models = LM.new_stores(oracle, alg, sc["specs"])
    (tmp_path / "twin").mkdir()
    plain, twin = Env(cw, oracle, alg, sc["specs"], tmp_path), Twin(cw, oracle, alg, sc["specs"], tmp_path / "twin", lifts)
    seen = {n: ([], [], [lifts[n]]) for n in sc["specs"]}                 # entries' starts and ends, cursors (the first step starts from the lift)
    try:
        for i, (op, args, expect) in enumerate(sc["steps"]):
            where = (sc["name"], i, op)
            want = LM.run(models, op, args)
            assert want["code"] == expect, where
            if expect:
                before = twin.state()
                for env in (plain, twin):
                    with pytest.raises(cw.CwError) as e:
                        env.step(op, args, want)
                    assert e.value.code == expect, (where, str(e.value))
                if op not in LM.PARTIAL or want["run"].consumed == 0:
                    assert twin.state() == before, (where, "a refused step changed the twin")
            else:
                plain.step(op, args, want)
                twin.step(op, args, want)
            twin.same_as_plain(plain, models, where)
            for name, t in twin.stores.items():
                if twin.lift[name]:
                    s, e = P4.extents(t.d_dir.cpu().numpy())
                    seen[name][0].append(s), seen[name][1].append(e), seen[name][2].append(t.used())
        # the run reached what it exists for
        for name, (starts, ends, cursors) in seen.items():
            r = P4.reaches(np.concatenate(starts), np.concatenate(ends))
            at = (sc["name"], name, lifts[name], r, min(cursors), max(cursors))
            assert r["above"] and max(cursors) > B, at
            if reach[name] != "above":
                assert r["below"] and min(cursors) < B and (r["over"] or reach[name] == "both"), at
    finally:
        plain.close()
        twin.close()


def test_only_saving_scripts_are_left_out(oracle):
    saving = [n for n in LM.NAMES if any(op == "save_load" for op, _, _ in LM.script(oracle, "lz4", n)["steps"])]
    assert tuple(saving) == SAVING and len(LIFTED) == len(LM.NAMES) - 2 == 11


@pytest.mark.parametrize("name", LIFTED)
@pytest.mark.parametrize("alg", ALGS)
def test_lifted_twin_is_the_store_moved_up(cw, oracle, tmp_path, alg, name):
    lifted_run(cw, oracle, tmp_path, alg, LM.script(oracle, alg, name))


@pytest.mark.parametrize("name", [n for n in LM.UNGUARDED if n not in SAVING])
@pytest.mark.parametrize("alg", ALGS)
def test_protected_lifted_twin_is_the_store_moved_up(cw, oracle, tmp_path, alg, name):
    lifted_run(cw, oracle, tmp_path, alg, LM.protected(LM.script(oracle, alg, name), alg))


def dual255(oracle, alg):
    """A parity-2 store of 255-stripe groups, the dual guard's largest: three stripes of noise, a chunk across the first stripe
    boundary and one inside a stripe damaged together with the chunks over their columns in the next member, repaired in place."""
    G, S = 255, 65536
    s = LM.Script("dual255", oracle, alg, P=LM.GUARDED)
    s.do("protect", stripe=S, group=G, parity=2)
    names = ["N0", "N1", "N2"]
    for k, n in enumerate(names):
        s.do("ingest", name=n, data=LM.noise(300 + k, 60000))
    pairs = LM._pairs(s.stores["P"], G, ["stripe", "inside"])
    assert int(s.stores["P"].m.directory[pairs[0][0] - s.stores["P"].dir_base]["pos"]) < S                  # (it crosses the first boundary)
    LM._scrub_and_repair(s, "P", LM._damage(s, "P", pairs))
    s.do("scrub")
    s.do("guard_check")
    s.do("restore_many_stream", names=names)
    return s.done()


@pytest.mark.parametrize("alg", ALGS)
def test_dual_guard_at_its_largest_group_lies_over_2_32_by_one_stripe(cw, oracle, tmp_path, alg):
    """2^32 - 65536 is a multiple of 255 * 65536: the store lifted there has its first stripe below 2^32 and the others above, in one
    group, and the chunk across the first stripe boundary lies across 2^32."""
    sc = dual255(oracle, alg)
    assert (B - 65536) % (255 * 65536) == 0 and plan(oracle, alg, sc)[0] == dict(P=B - 65536)
    lifted_run(cw, oracle, tmp_path, alg, sc, dict(P=B - 65536), dict(P="over"))


# ---- 2b: the guard kernels at stripes of 2^20 and 2^30 bytes, called directly over a buffer that lies across 2^32 -----------------------
import guard2_model as G2  # noqa: E402
import guard_model as G1  # noqa: E402
import restore_model as RM  # noqa: E402

NB = B + 4 * MIB
GEOMETRY = {"2^20x16": (1 << 20, 16), "2^30x3": (1 << 30, 3)}                # at 16 stripes of 2^20, 2^32 is a group boundary; at 3 of 2^30 it lies inside group 1
POISON64, EE32, BLOCK = 0xABABABABABABABAB, 0xEEEEEEEE, P4.BLOCK


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int64 if a.dtype == np.uint64 else np.int32 if a.dtype == np.uint32 else a.dtype).copy()).cuda()


def _u64(values):
    return _dev(np.asarray(values, np.uint64))


class Around:
    """``NB`` bytes on the device that are zero but for noise in the window and in the two blocks around 2^32 - S (a chunk there meets
    one across 2^32 in a guard byte), the same image on the host (``np.zeros`` is lazily backed: only the noise is written), and the
    model's P and Q of the whole image: zero bytes add nothing, so only the noise is folded (tests/test_past4g_model.py)."""

    def __init__(self, cw, S, G):
        import torch
        self.S, self.G, self.W = S, G, S * G
        spans = [(B - S - BLOCK, B - S + BLOCK), (P4.WIN_LO, P4.WIN_HI)]
        if spans[0][1] >= spans[1][0]:                                        # (S = 2^20: the two meet; a byte folded twice would cancel)
            spans = [(spans[0][0], spans[1][1])]
        self.dev, self.host = torch.zeros(NB, dtype=torch.uint8, device="cuda"), np.zeros(NB, np.uint8)
        torch.cuda.synchronize()
        for lo, hi in spans:
            cw.dev_gen_random(0x6A4D, lo // BLOCK, (hi - lo) // BLOCK, BLOCK, self.dev[lo:hi].data_ptr(), _stream())
        torch.cuda.synchronize()
        for lo, hi in spans:
            self.host[lo:hi] = self.dev[lo:hi].cpu().numpy()
        self.size = G1.guard_bytes(NB, S, G)
        assert self.size == cw.store_guard_bytes(NB, S, G) and G2.geometry_ok(S, G)
        self.p, self.q = np.zeros(self.size, np.uint8), np.zeros(self.size, np.uint8)
        self.below = min(lo for lo, _ in spans) - 12345                       # a cursor below every non-zero byte
        cells = []
        for lo, hi in spans:
            G1.fold(self.p, self.host, lo, hi, S, G)
            G2.fold_q(self.q, self.host, lo, hi, S, G)
            cells.append(G1.cells(np.arange(lo, hi, dtype=np.int64), S, G))
        self.cells = np.unique(np.concatenate(cells))
        self.groups = -(-NB // self.W)


@pytest.fixture(scope="module", params=list(GEOMETRY))
def around(cw, request):
    import torch
    a = Around(cw, *GEOMETRY[request.param])
    yield a
    del a.dev
    torch.cuda.empty_cache()


class DevGuard:
    """P (and Q) on the device with the one cursor, and the three calls of either parity."""

    def __init__(self, cw, a, parity, covered):
        import torch
        self.cw, self.a, self.parity = cw, a, parity
        self.bufs = [torch.zeros(a.size, dtype=torch.uint8, device="cuda") for _ in range(parity)]
        self.d_covered = _u64([covered])
        torch.cuda.synchronize()

    def _guards(self):
        return [b.data_ptr() for b in self.bufs]

    def update(self, used):
        import torch
        a, d_used, result = self.a, _u64([used]), _u64([7, 7, 7, 7, POISON64])
        torch.cuda.synchronize()
        fn = self.cw.dev_store_guard_update if self.parity == 1 else self.cw.dev_store_guard2_update
        fn(a.dev.data_ptr(), NB, d_used.data_ptr(), self.d_covered.data_ptr(), a.S, a.G, *self._guards(), a.size, result.data_ptr(), _stream())
        torch.cuda.synchronize()
        r = result.cpu().numpy().view(np.uint64).tolist()
        assert r[4] == POISON64
        return r[:4]

    def check(self):
        """(d_result[0..4), the flags of every group); no flag is written outside the groups checked"""
        import torch
        a = self.a
        bad, result = _dev(np.full(a.groups + 2, EE32, np.uint32)), _u64([7, 7, 7, 7, POISON64])
        torch.cuda.synchronize()
        fn = self.cw.dev_store_guard_check if self.parity == 1 else self.cw.dev_store_guard2_check
        fn(a.dev.data_ptr(), NB, self.d_covered.data_ptr(), a.S, a.G, *self._guards(), a.size, bad.data_ptr() + 4, result.data_ptr(), _stream())
        torch.cuda.synchronize()
        r, flags = result.cpu().numpy().view(np.uint64).tolist(), bad.cpu().numpy().view(np.uint32)
        assert r[4] == POISON64 and flags[0] == flags[-1] == EE32
        return r[:4], flags[1:-1].tolist()

    def rebuild(self, directory, values, out_bytes):
        """(d_result, statuses, d_out, d_out_loc) with poison around every output"""
        import torch
        a, n, pad = self.a, len(values), 64
        d_dir, d_val, d_count = _dev(np.ascontiguousarray(directory, RM.LOC).view(np.uint64)), _u64(list(values) + [0]), _u64([n])
        out, loc = _dev(np.full(out_bytes + 2 * pad, 0xEE, np.uint8)), _u64(np.full(2 * (n + 2), POISON64, np.uint64))
        status, result = _dev(np.full(n + 2, EE32, np.uint32)), _u64([7, 7, 7, 7, 7, POISON64])
        torch.cuda.synchronize()
        fn = self.cw.dev_store_guard_rebuild if self.parity == 1 else self.cw.dev_store_guard2_rebuild
        fn(a.dev.data_ptr(), NB, d_dir.data_ptr(), 0, len(directory), self.d_covered.data_ptr(), a.S, a.G, *self._guards(), a.size, d_val.data_ptr(),
           d_count.data_ptr(), n, out.data_ptr() + pad, out_bytes, loc.data_ptr() + 16, status.data_ptr() + 4, result.data_ptr(), _stream())
        torch.cuda.synchronize()
        h, locs, st = out.cpu().numpy(), loc.cpu().numpy().view(np.uint64), status.cpu().numpy().view(np.uint32)
        r = result.cpu().numpy().view(np.uint64).tolist()
        assert (h[:pad] == 0xEE).all() and (h[pad + out_bytes:] == 0xEE).all() and (locs[:2] == POISON64).all() and (locs[-2:] == POISON64).all()
        assert st[0] == st[-1] == EE32 and r[5] == POISON64
        return r[:4 + (self.parity == 2)], st[1:-1], h[pad:pad + out_bytes], locs[2:-2].view(RM.LOC)


@pytest.mark.parametrize("parity", [1, 2])
def test_guard_kernels_across_2_32_at_large_stripes(cw, around, parity):
    import torch
    a = around
    S, G, W, groups = a.S, a.G, a.W, a.groups
    model = (a.p, a.q)[:parity]
    g = DevGuard(cw, a, parity, a.below)
    # one update from below the window to the end
    assert g.update(NB) == [0, a.below, NB, NB - a.below] and int(g.d_covered.item()) == NB
    at = torch.from_numpy(a.cells).cuda()
    for buf, want in zip(g.bufs, model):
        assert np.array_equal(buf[at].cpu().numpy(), want[a.cells]), "guard words of the noise"
        assert int(torch.count_nonzero(buf).item()) == int(np.count_nonzero(want[a.cells])), "a guard word outside the noise's cells was written"
    cell = {p: int(G1.cells([p], S, G)[0]) for p in (B - 1, B)}
    assert (cell[B - 1] // S, cell[B] // S) == ((B - 1) // W, B // W) and cell[B - 1] % S == S - 1 and cell[B] % S == 0
    assert ((B - 1) // W != B // W) == (G == 16)
    # check: clean, then a flipped store byte on either side of 2^32, then a flipped guard byte over each
    both = 1 if parity == 1 else 3
    assert g.check() == ([0, groups, 0, G1.NONE], [0] * groups)
    for p in (B - 1, B):
        a.dev[p:p + 1].bitwise_xor_(0x10)
        assert g.check() == ([0, groups, 1, p // W], [both if k == p // W else 0 for k in range(groups)]), p
        a.dev[p:p + 1].bitwise_xor_(0x10)
        for which in range(parity):
            g.bufs[which][cell[p]:cell[p] + 1].bitwise_xor_(0x01)
            assert g.check() == ([0, groups, 1, cell[p] // S], [1 << which if k == cell[p] // S else 0 for k in range(groups)]), (p, which)
            g.bufs[which][cell[p]:cell[p] + 1].bitwise_xor_(0x01)
    assert g.check() == ([0, groups, 0, G1.NONE], [0] * groups)
    # rebuild: a chunk across 2^32; then two chunks that meet in a guard byte, the second across 2^32 (both collide without Q)
    directory = np.array([G1.entry(B - 3000, 6000), G1.entry(B - S - 2000, 4000), G1.entry(B - 2000, 4000)], RM.LOC)
    for values in ([0], [1, 2]):
        ext = [(int(directory[v]["pos"]), int(directory[v]["stored"])) for v in values]
        good = [a.host[p:p + n].copy() for p, n in ext]
        for p, n in ext:
            a.dev[p:p + n].bitwise_xor_(0xA5)
            a.host[p:p + n] ^= 0xA5
        try:
            if parity == 1:
                want, wst, wout, wlocs = G1.rebuild(a.host, NB, directory, 0, NB, S, G, a.p, values, 1 << 62)
            else:
                want, wst, wout, wlocs = G2.rebuild(a.host, NB, directory, 0, NB, S, G, a.p, a.q, values, 1 << 62)
            result, st, out, locs = g.rebuild(directory, values, want[1])
        finally:
            for p, n in ext:
                a.dev[p:p + n].bitwise_xor_(0xA5)
                a.host[p:p + n] ^= 0xA5
        assert result == want and st.tolist() == wst.tolist() and np.array_equal(out, wout) and (locs == wlocs).all(), values
        assert wst.tolist() == ([G1.REBUILT] * len(values) if parity == 2 or values == [0] else [G1.COLLIDES] * 2), (values, wst)
        for k, s in enumerate(wst.tolist()):
            if s == G1.REBUILT:
                o = int(locs[k]["pos"])
                assert np.array_equal(out[o:o + ext[k][1]], good[k]), ("the original bytes", values, k)
        assert any(p < B < p + n for p, n in ext) and (len(ext) == 1 or ext[0][0] + ext[0][1] < B)
