"""Hash differential: the built inputs of hash_inputs.py (messages and call shapes at the kernels' step, line and slice edges;
pinned on the CPU by test_hash_inputs.py) through every way a digest leaves the library, under every hash knob, against the
oracle's digests.

The doors: cw_dev_hash with the one-launch kernels (every length of the set, aligned and misaligned sources with poison in the
gaps, aligned and misaligned digest buffers, the four knob sets), cw_dev_hash in sliced launches (every row of SLICED and the
threshold rows, twice on one stream and once on a second), cw_dev_hash_chunks, cw_dev_hash_and_compress, the host pipeline, the
one-slot calls and HashOffload.  Every call compares EVERY digest on the device, none sampled; after every cw_dev_hash call the
kernel the library says it launched must be line 1 of the plan, and the union of those names must hold every hash kernel there
is.  The oracle's digests are computed once per module and data set."""
import numpy as np
import pytest

import hash_inputs as H

pytestmark = pytest.mark.gpu
FILL = 0xEE
_CACHE = {}
_NAMES = {}     # door -> the kernel names its calls reported


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


def _once(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _want(oracle, alg):
    """{length: [PER_LENGTH, digest bytes]}: the oracle's digests of the one-launch set, built once."""
    def make():
        out = {}
        for n in H.LENGTHS:
            d = H.digests_of(oracle, alg, H.messages(n), n)
            out[n] = np.repeat(d, H.PER_LENGTH, axis=0) if n == 0 else d
            assert out[n].shape == (H.PER_LENGTH, H.DIGEST[alg])
        return out
    return _once(("want", alg), make)


def _first_difference(got, want):
    """Flat index of the first byte in which two device tensors differ."""
    import torch
    return int(torch.nonzero(got.reshape(-1) != want.reshape(-1))[0])


# ---- cw_dev_hash, one-launch kernels ----------------------------------------------------------------------------------------------
LAYOUTS = ("aligned", "misaligned")


def _layout(name):
    """(device buffer, {length: (offset of the first message, stride)}): the whole set in one buffer, every length's messages in a
    16-byte aligned region of their own -- aligned: at the region's start, stride a multiple of 16 with at least 16 bytes of poison
    behind every message; misaligned: 3 bytes in, stride length + 7."""
    def make():
        import torch
        parts, where, at = [], {}, 0
        for n in H.LENGTHS:
            stride, shift = ((n + 15) // 16 * 16 + 16, 0) if name == "aligned" else (n + 7, 3)
            buf, _ = H.lay_out(H.messages(n), stride, shift, seed=2 * n + (name == "aligned"))
            buf = np.concatenate([buf, np.full(-buf.size % 16, 0x5A, np.uint8)])
            where[n] = (at + shift, stride)
            parts.append(buf)
            at += buf.size
        return torch.from_numpy(np.concatenate(parts)).cuda(), where
    return _once(("layout", name), make)


def _one_launch(cw, oracle, alg):
    """Every call of one algorithm queued, one synchronisation, every digest and every guard byte compared; the names reported."""
    def make():
        import torch
        db, want = H.DIGEST[alg], _want(oracle, alg)
        row = H.PER_LENGTH * db + 16    # a call's digests and 16 guard bytes: the digests go to the row's start or 4 bytes in
        calls = [(lay, k, shift, n) for lay in LAYOUTS for k in range(len(H.KNOB_SETS)) for shift in (0, 4) for n in H.LENGTHS]
        out = torch.full((len(calls), row), FILL, dtype=torch.uint8, device="cuda")
        assert out.data_ptr() % 16 == 0 and row % 16 == 0
        expect = np.full((len(calls), row), FILL, np.uint8)
        names, s, i = set(), _stream(), 0
        for lay in LAYOUTS:
            src, where = _layout(lay)
            assert src.data_ptr() % 16 == 0
            for k, knobs in enumerate(H.KNOB_SETS):
                with cw.tuned(**knobs):
                    for shift in (0, 4):
                        for n in H.LENGTHS:
                            assert calls[i] == (lay, k, shift, n)
                            at, stride = where[n]
                            ptr = src.data_ptr() + at
                            dig = out.data_ptr() + i * row + shift
                            cw.dev_hash(alg, ptr, n, H.PER_LENGTH, dig, s, src_stride=stride)
                            name = cw.profile_kernels()["hash"]
                            planned = cw.hash_plan_describe(alg, n, H.PER_LENGTH, (ptr | stride) & 15, dig & 15).split("\n")[0]
                            assert name == planned, (alg, lay, knobs, shift, n)
                            names.add(name)
                            expect[i, shift:shift + H.PER_LENGTH * db] = want[n].reshape(-1)
                            i += 1
        torch.cuda.synchronize()
        expect = torch.from_numpy(expect).cuda()
        if not torch.equal(out, expect):
            at = _first_difference(out, expect)
            lay, k, shift, n = calls[at // row]
            col = at % row - shift
            what = f"block {col // db} ({H.case(n, col // db)})" if 0 <= col < H.PER_LENGTH * db else "a guard byte beside the digests"
            raise AssertionError(f"{alg} {lay} source, {H.KNOB_SETS[k]}, digests + {shift}, length {n}: {what} differs from the oracle")
        return names
    return _NAMES.setdefault(("one_launch", alg), _once(("one_launch", alg), make))


@pytest.mark.parametrize("alg", H.ALGS)
def test_one_launch_kernels_give_the_oracles_digests_at_every_length(cw, oracle, alg):
    """cw_dev_hash over 67 messages of every length of the set: 2 layouts x 4 knob sets x 2 digest alignments x 397 lengths, every
    digest and the guard bytes around them."""
    names = _one_launch(cw, oracle, alg)
    nw = {"skein512": "<8", "skein": "<4", "sha256": "sha256"}[alg]
    assert names == {k for k in H.KERNELS_ONE_LAUNCH if nw in k}


# ---- cw_dev_hash, sliced launches ---------------------------------------------------------------------------------------------------
def _dev_hash_all(cw, alg, src, bs, nb, side=None):
    """Digests [nb, db] of one cw_dev_hash call (not synchronised) and the name it reported.  side: a torch stream to run it on."""
    import torch
    dig = torch.full((nb, H.DIGEST[alg]), FILL, dtype=torch.uint8, device="cuda")
    if side is not None:
        side.wait_stream(torch.cuda.current_stream())   # (the fill above)
    cw.dev_hash(alg, src.data_ptr(), bs, nb, dig.data_ptr(), _stream() if side is None else side.cuda_stream)
    return dig, cw.profile_kernels()["hash"]


def _check(got, want, what):
    import torch
    if not torch.equal(got, want):
        at = _first_difference(got, want)
        raise AssertionError(f"{what}: block {at // got.shape[1]} is the first of "
                             f"{int((got != want).any(dim=1).sum())} digests that differ from the oracle's")


def _sliced(cw, oracle, alg, bs):
    def make():
        import torch
        nb = H.NBLOCKS_SLICED
        src = torch.empty(nb * bs, dtype=torch.uint8, device="cuda")
        cw.dev_gen_random(0xD16E57 + bs, 0, nb, bs, src.data_ptr(), _stream())
        torch.cuda.synchronize()
        want = torch.from_numpy(H.digests_of(oracle, alg, src.cpu().numpy(), bs)).cuda()
        assert want.shape == (nb, H.DIGEST[alg])
        side = torch.cuda.Stream()
        names, results = set(), []
        for r in (r for r in H.SLICED if (r.alg, r.block_bytes) == (alg, bs)):
            with cw.tuned(**r.knobs):
                planned = cw.hash_plan_describe(alg, bs, nb).split("\n")
                assert len(planned) - 2 == r.launches
                runs = [_dev_hash_all(cw, alg, src, bs, nb), _dev_hash_all(cw, alg, src, bs, nb)]   # the state array is used again
                runs.append(_dev_hash_all(cw, alg, src, bs, nb, side))                               # ... and a second stream has its own
            torch.cuda.synchronize()
            for i, (dig, name) in enumerate(runs):
                assert name == planned[0], (str(r), name)
                _check(dig, want, f"{r} ({r.edge}), call {i}")
                names.add(name)
            results.append(runs[0][0])
        for t in (t for t in H.THRESHOLD if (t.alg, t.block_bytes) == (alg, bs)):
            dig, name = _dev_hash_all(cw, alg, src, bs, t.nblocks)
            torch.cuda.synchronize()
            assert name == cw.hash_plan_describe(alg, bs, t.nblocks).split("\n")[0]
            assert (name in H.KERNELS_SLICED) == t.sliced, (str(t), name)
            _check(dig, want[:t.nblocks], f"{t} ({t.edge})")
            names.add(name)
        # the same blocks in calls of 2048, below the floor of blocks: the one-launch kernel
        parts = []
        for first in range(0, nb, 2048):
            n = min(2048, nb - first)
            dig, name = _dev_hash_all(cw, alg, src[first * bs:], bs, n)
            assert "lines_kernel" in name
            parts.append(dig)
        torch.cuda.synchronize()
        one_launch = torch.cat(parts)
        _check(one_launch, want, f"{alg} {bs} in calls of 2048 blocks")
        for dig in results:
            assert torch.equal(dig, results[0]) and torch.equal(dig, one_launch)
        return names
    return _NAMES.setdefault(("sliced", alg, bs), _once(("sliced", alg, bs), make))


@pytest.mark.parametrize("alg,bs", H.SLICED_SHAPES, ids=lambda v: str(v))
def test_sliced_launches_give_the_oracles_digests(cw, oracle, alg, bs):
    """Every row of SLICED and THRESHOLD of one shape over 4101 generated blocks: all digests against the oracle's, the rows
    against each other and against the one-launch kernel over the same blocks."""
    names = _sliced(cw, oracle, alg, bs)
    rows = [r for r in H.SLICED if (r.alg, r.block_bytes) == (alg, bs)]
    assert rows or [t for t in H.THRESHOLD if (t.alg, t.block_bytes) == (alg, bs)]
    if rows:
        assert names & set(H.KERNELS_SLICED)


# ---- cw_dev_hash_chunks ---------------------------------------------------------------------------------------------------------------
def _chunk_set():
    """(data, cuts, [(length, i)] per chunk): every message of the one-launch set as a chunk of its own length, shuffled, end to end."""
    def make():
        ids = [(n, i) for n in H.LENGTHS for i in range(H.PER_LENGTH)]
        order = np.random.default_rng(23).permutation(len(ids))
        ids = [ids[j] for j in order]
        cuts = np.concatenate([[0], np.cumsum([n for n, _ in ids])])
        data = np.concatenate([H.messages(n)[i] for n, i in ids])
        return data, cuts, ids
    return _once("chunks", make)


def _chunk_door(cw, oracle, alg):
    def make():
        import torch
        data, cuts, ids = _chunk_set()
        assert {int(c) % 16 for c in cuts[:-1]} == set(range(16))   # chunk starts at every residue mod 16
        db, table = H.DIGEST[alg], _want(oracle, alg)
        want = torch.from_numpy(np.stack([table[n][i] for n, i in ids])).cuda()
        o = torch.from_numpy(cuts.astype(np.int64)).cuda()
        k = torch.tensor([len(ids)], dtype=torch.int64, device="cuda")
        names = set()
        for shift in (0, 1):
            rng = np.random.default_rng(shift)
            buf = np.concatenate([rng.integers(1, 256, shift, dtype=np.uint8), data, rng.integers(1, 256, 64, dtype=np.uint8)])
            src = torch.from_numpy(buf).cuda()
            dig = torch.full((len(ids), db), FILL, dtype=torch.uint8, device="cuda")
            cw.dev_hash_chunks(alg, src.data_ptr() + shift, data.size, o.data_ptr(), k.data_ptr(), len(ids), dig.data_ptr(), _stream())
            torch.cuda.synchronize()
            names.add(cw.profile_kernels()["hash"])
            if not torch.equal(dig, want):
                c = _first_difference(dig, want) // db
                raise AssertionError(f"{alg} chunks, source + {shift}: chunk {c} at {int(cuts[c])} ({H.case(*ids[c])}) differs from the oracle")
        return names
    return _NAMES.setdefault(("chunks", alg), _once(("chunk_door", alg), make))


@pytest.mark.parametrize("alg", H.ALGS)
def test_the_chunk_door_gives_the_oracles_digests(cw, oracle, alg):
    """cw_dev_hash_chunks over all 26,599 messages of the set as chunks of their own lengths, at source shifts 0 and 1."""
    names = _chunk_door(cw, oracle, alg)
    assert len(names) == 1 and names <= set(H.KERNELS_CHUNKS)


# ---- every kernel is reached ------------------------------------------------------------------------------------------------------------
def test_the_sets_reach_every_hash_kernel(cw, oracle):
    """The union of the names the calls above reported (a door another test of this module has run is not run again) is the whole
    KERNELS list: a knob set or a row that fell back to another kernel fails here instead of passing unseen."""
    seen = set()
    for alg in H.ALGS:
        seen |= _one_launch(cw, oracle, alg) | _chunk_door(cw, oracle, alg)
    for alg, bs in H.SLICED_SHAPES:
        seen |= _sliced(cw, oracle, alg, bs)
    assert seen == set(H.KERNELS), (sorted(set(H.KERNELS) - seen), sorted(seen - set(H.KERNELS)))


# ---- cw_dev_hash_and_compress -----------------------------------------------------------------------------------------------------------
FUSED_KNOBS = (dict(), dict(CW_FUSED_GATE=1), dict(CW_FUSED_GATE=0), dict(CW_SERIAL=1))
FUSED_SHAPES = {"mixed_4096": (4096, 16390, H.ALGS), "sliced_floor": (16320, H.NBLOCKS_SLICED, ("skein512",))}


@pytest.mark.parametrize("codec", ["lz4", "lzf"])
@pytest.mark.parametrize("shape", list(FUSED_SHAPES))
def test_the_fused_call_gives_the_oracles_digests(cw, oracle, shape, codec):
    """cw_dev_hash_and_compress beside both codecs: 16,390 blocks of 4 KiB of the compressible mix (parsers run beside the hash) and
    4101 blocks of the smallest sliced Skein-512 message, side by side, gated either way and one after the other."""
    import torch
    bs, nb, algs = FUSED_SHAPES[shape]

    def make():
        src = torch.empty(nb * bs, dtype=torch.uint8, device="cuda")
        (cw.dev_gen_mixed if shape == "mixed_4096" else cw.dev_gen_random)(0xF05ED, 0, nb, bs, src.data_ptr(), _stream())
        torch.cuda.synchronize()
        host = src.cpu().numpy()
        return src, {alg: torch.from_numpy(H.digests_of(oracle, alg, host, bs)).cuda() for alg in algs}
    src, want = _once(("fused", shape), make)
    stride = (cw.compress_bound(codec, bs) + 15) // 16 * 16
    dst = torch.empty(nb * stride, dtype=torch.uint8, device="cuda")
    for knobs in FUSED_KNOBS:
        for alg in algs:
            dig = torch.full((nb, H.DIGEST[alg]), FILL, dtype=torch.uint8, device="cuda")
            sizes = torch.full((nb,), -1, dtype=torch.int32, device="cuda")
            with cw.tuned(**knobs):
                cw.dev_hash_and_compress(alg, codec, src.data_ptr(), bs, nb, dig.data_ptr(), dst.data_ptr(), stride, sizes.data_ptr(), _stream())
                torch.cuda.synchronize()
                name = cw.profile_kernels()["hash"]
                assert name == cw.hash_plan_describe(alg, bs, nb).split("\n")[0]
            _check(dig, want[alg], f"{alg} + {codec}, {nb} x {bs}, {knobs} ({name})")
            assert bool((sizes >= 0).all()) and int(sizes.max()) <= stride


# ---- the host doors -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alg", H.ALGS)
def test_the_host_pipeline_gives_the_oracles_digests(cw, oracle, alg):
    """cw_hash_blocks in chunks of 1 MiB (several in flight) over the long messages of the set, cut into blocks of 4096, 12345 and
    65536 bytes."""
    data = _once("host_data", lambda: np.concatenate([H.messages(n).reshape(-1) for n in H.LENGTHS])[-(6 << 20):].copy())
    for bs in (4096, 12345, 65536):
        nb = data.size // bs
        want = _once(("host_want", alg, bs), lambda: H.digests_of(oracle, alg, data[:nb * bs], bs))
        with cw.tuned(CW_HOST_CHUNK_MB=1):
            got = cw.hash_blocks(alg, data[:nb * bs], bs)
        bad = np.nonzero((got != want).any(axis=1))[0]
        assert bad.size == 0, f"{alg} {nb} x {bs}: {bad.size} digests differ from the oracle's, first block {bad[0]}"


@pytest.mark.parametrize("alg", H.ALGS)
def test_the_one_slot_calls_give_the_oracles_digests(cw, oracle, alg):
    """doHashing over the 67 messages of a few lengths either side of a step and a line."""
    before = int(cw.lib().cw_get_block_size())
    try:
        for n in (1, 31, 32, 33, 63, 64, 65, 96, 127, 128, 224, 385, 4097):
            got = np.frombuffer(cw.do_hashing(alg, H.messages(n), H.PER_LENGTH, block_bytes=n), np.uint8).reshape(H.PER_LENGTH, -1)
            bad = np.nonzero((got != _want(oracle, alg)[n]).any(axis=1))[0]
            assert bad.size == 0, f"{alg} length {n}: block {bad[0]} ({H.case(n, int(bad[0]))}) differs from the oracle"
    finally:
        cw.set_block_size(before)


def test_hash_offload_does_not_slice_and_gives_the_oracles_digests(cw, oracle):
    """HashOffload over 4101 blocks of the smallest sliced message: the line kernel, as its plan (may_slice = 0) says."""
    bs, nb, alg = H.SLICED_FLOOR["skein512"], H.NBLOCKS_SLICED, "skein512"
    data = oracle.gen_random_blocks(0x0FF10AD, 0, nb, bs)
    want = H.digests_of(oracle, alg, data, bs)
    res = np.full(nb * H.DIGEST[alg], FILL, np.uint8)
    h = cw.HashOffload(nb, alg, bs)
    try:
        h.Reset(data, res)
        h.Enqueue()
        h.DoOffload()
        assert h.Completed()
        name = cw.profile_kernels()["hash"]
    finally:
        h.close()
    assert name == "cw::skein_lines_kernel<8, true>" == cw.hash_plan_describe(alg, bs, nb, may_slice=False).split("\n")[0]
    assert cw.hash_plan_describe(alg, bs, nb).split("\n")[0] in H.KERNELS_SLICED
    bad = np.nonzero((res.reshape(nb, -1) != want).any(axis=1))[0]
    assert bad.size == 0, f"{bad.size} digests differ from the oracle's, first block {bad[0]}"
