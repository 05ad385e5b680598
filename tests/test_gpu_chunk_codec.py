"""The codecs over content-defined chunks on the GPU (cw_dev_compress_chunks, cw_dev_pack_chunks, cw_dev_decompress_chunks,
cw_dev_cdc_dedupe_compress) against the CPU oracle, chunk by chunk.

The oracle writes every chunk into a host image of the slot buffer laid out by the same closed form, prefilled with the same
pattern as the device's, so one comparison of the two images checks sizes' payloads, the gaps between the slots and the
slots of chunks that must not be touched.  (An LZF chunk that did not fit leaves its slot unspecified: those extents are
blanked on both sides.)"""
import threading
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import cdc_model as CM
from conftest import corpus_file, corpus_large_file, corpus_names

pytestmark = pytest.mark.gpu
FILL = 0xA5
GUARD = 256
CW_ERR_NOMEM = -5
D8 = CM.default_params(8192)
SMALL = CM.params(64, 256, 1024, CM.top_bits(10), CM.top_bits(6))
ALGS = ["lz4", "lzf"]


@pytest.fixture(scope="module")
def cw():
    import torch  # noqa: F401  (one HIP runtime for torch and libcwhc.so)
    import compute_war_amd as cw
    cw.init(0)
    yield cw
    cw.tune_reset()


@pytest.fixture(scope="module")
def O():
    import oracle
    oracle.build()
    return oracle


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _params(cw, p: dict):
    return cw.CdcParams(p["min"], p["avg"], p["max"], p["mask_s"], p["mask_l"], p.get("gear"))


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


def _dev_u64(values):
    import torch
    return torch.from_numpy(np.asarray(values, np.uint64).view(np.int64).copy()).cuda()


# ---- the oracle, chunk by chunk ---------------------------------------------------------------------------------------
def _in_contract(cuts, i, count, src_bytes):
    return i < count and cuts[i] < cuts[i + 1] <= src_bytes and cuts[i + 1] - cuts[i] <= 65536


def _oracle_fn(O, alg):
    L = O.lib()
    if alg == "lz4":
        return lambda src, l, dst: L.cw_oracle_lz4_compress(src, l, dst, l + l // 255 + 16)
    return lambda src, l, dst: L.cw_oracle_lzf_compress(src, l, dst, l - 1) if l > 1 else 0


def oracle_sizes(O, alg, data: np.ndarray, cuts, chunks, threads=16):
    """Compressed size of every listed chunk (0: LZF did not fit); the ctypes calls release the GIL."""
    fn, base = _oracle_fn(O, alg), data.ctypes.data
    out = np.zeros(len(chunks), np.uint32)

    def work(t):
        scratch = np.zeros(2 * 65536 + 64, np.uint8)
        for k in range(t, len(chunks), threads):
            i = chunks[k]
            out[k] = fn(base + int(cuts[i]), int(cuts[i + 1] - cuts[i]), scratch.ctypes.data)

    with ThreadPoolExecutor(threads) as ex:
        list(ex.map(work, range(threads)))
    return out


def oracle_image(cw, O, alg, data: np.ndarray, cuts, chunks, total_bytes):
    """(sizes of the listed chunks, image of the slot buffer after compressing exactly those chunks)."""
    fn, base = _oracle_fn(O, alg), data.ctypes.data
    img = np.full(total_bytes, FILL, np.uint8)
    sizes = np.zeros(len(chunks), np.uint32)
    scratch = np.zeros(2 * 65536 + 64, np.uint8)
    for k, i in enumerate(chunks):
        s, l = int(cuts[i]), int(cuts[i + 1] - cuts[i])
        n = fn(base + s, l, scratch.ctypes.data)
        sizes[k] = n
        slot = cw.chunk_slot_offset(alg, s, i)
        img[slot:slot + n] = scratch[:n]
    return sizes, img


class Run:
    """One cw_dev_compress_chunks call with guard bytes around d_dst and everything it wrote brought to the host."""

    def __init__(self, cw, alg, data: np.ndarray, cuts=None, cdc=None, shift=0, count=None, max_chunks=None, sel=None, nsel=None,
                 src_bytes=None, stream=None):
        import torch
        self.cw, self.alg = cw, alg
        n = len(data)
        self.src_bytes = n if src_bytes is None else src_bytes
        self.buf = torch.empty(shift + n, dtype=torch.uint8, device="cuda")  # the source ends with its buffer
        self.buf[:shift] = 0x77
        self.buf[shift:] = torch.from_numpy(data).cuda()
        self.d_src = self.buf.data_ptr() + shift
        s = _stream() if stream is None else stream
        if cdc is not None:
            cap = cdc.max_offsets(n)
            self.d_off = torch.zeros(cap, dtype=torch.int64, device="cuda")
            self.d_k = torch.zeros(1, dtype=torch.int64, device="cuda")
            cw.dev_cdc(cdc, self.d_src, n, True, self.d_off.data_ptr(), cap, self.d_k.data_ptr(), s)
            self.max_chunks = cap - 1 if max_chunks is None else max_chunks
        else:
            self.d_off = _dev_u64(cuts)
            self.d_k = _dev_u64([len(cuts) - 1 if count is None else count])
            self.max_chunks = len(cuts) - 1 if max_chunks is None else max_chunks
        self.d_sel = self.d_nsel = None
        if sel is not None:
            self.d_sel = torch.from_numpy(np.asarray(sel, np.uint32).view(np.int32).copy()).cuda() if len(sel) else \
                torch.zeros(1, dtype=torch.int32, device="cuda")
            self.d_nsel = _dev_u64([len(sel) if nsel is None else nsel])
        self.total = cw.chunk_slots_bytes(alg, self.src_bytes, self.max_chunks)
        self.dst = torch.full((GUARD + self.total + GUARD,), FILL, dtype=torch.uint8, device="cuda")
        self.d_dst = self.dst.data_ptr() + GUARD
        self.d_sizes = torch.full((max(self.max_chunks, 1) + 4,), -1, dtype=torch.int32, device="cuda")
        cw.dev_compress_chunks(alg, self.d_src, self.src_bytes, self.d_off.data_ptr(), self.d_k.data_ptr(), self.max_chunks, self.d_dst,
                               self.total, self.d_sizes.data_ptr(), s, self.d_sel.data_ptr() if sel is not None else 0,
                               self.d_nsel.data_ptr() if sel is not None else 0)
        if stream is None:
            torch.cuda.synchronize()

    def fetch(self):
        import torch
        torch.cuda.synchronize()
        self.k = int(self.d_k.item())
        self.cuts = _u64(self.d_off)[:self.k + 1].astype(np.int64)
        self.sizes = self.d_sizes.cpu().numpy().view(np.uint32)
        host = self.dst.cpu().numpy()
        self.guards_ok = bool((host[:GUARD] == FILL).all() and (host[-GUARD:] == FILL).all())
        self.image = host[GUARD:-GUARD]
        return self


def check_run(cw, O, r: Run, data: np.ndarray, positions=None):
    """Sizes per position, payloads, gaps, untouched slots and guards of a fetched run against the oracle."""
    count = min(r.k, r.max_chunks)
    chunks = list(range(count)) if positions is None else list(positions)
    ok = [i for i in chunks if _in_contract(r.cuts, i, count, r.src_bytes)] if positions is None else \
        [i for i in chunks if i < count and _in_contract(r.cuts, i, count, r.src_bytes)]
    sizes_ok, img = oracle_image(cw, O, r.alg, data, r.cuts, ok, r.total)
    by_chunk = dict(zip(ok, sizes_ok.tolist()))
    want = np.array([by_chunk.get(i, 0) for i in chunks], np.uint32)
    got = r.sizes[:len(chunks)]
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, (r.alg, "position", int(bad[0]), "chunk", chunks[int(bad[0])], int(got[bad[0]]), int(want[bad[0]]), len(bad))
    assert (r.sizes[len(chunks):] == 0xFFFFFFFF).all(), "sizes past the count were written"
    image = r.image.copy()
    if r.alg == "lzf":  # a chunk that did not fit leaves [o, o + l) unspecified
        for i in ok:
            if by_chunk[i] == 0:
                s, e = int(r.cuts[i]), int(r.cuts[i + 1])
                image[s:e] = FILL
                img[s:e] = FILL
    diff = np.nonzero(image != img)[0]
    assert len(diff) == 0, (r.alg, "slot image differs at", int(diff[0]), len(diff))
    assert r.guards_ok
    return by_chunk


def roundtrip(cw, r: Run, data: np.ndarray, by_chunk):
    """Pack the run's positions (all chunks, in order), check the index, decode, compare with the source."""
    import torch
    count = min(r.k, r.max_chunks)
    d_poff = torch.full((count + 3,), -1, dtype=torch.int64, device="cuda")
    sizes = r.sizes[:count].astype(np.int64)
    packed = torch.full((int(sizes.sum()) + 64,), FILL, dtype=torch.uint8, device="cuda")
    cw.dev_pack_chunks(r.alg, r.d_dst, r.d_off.data_ptr(), r.d_k.data_ptr(), r.max_chunks, r.d_sizes.data_ptr(), packed.data_ptr(),
                       d_poff.data_ptr(), _stream())
    out = torch.full((len(data) + 64,), FILL, dtype=torch.uint8, device="cuda")
    status = torch.full((count + 2,), -1, dtype=torch.int32, device="cuda")
    cw.dev_decompress_chunks(r.alg, packed.data_ptr(), d_poff.data_ptr(), r.d_off.data_ptr(), r.d_k.data_ptr(), r.max_chunks,
                             out.data_ptr(), len(data), status.data_ptr(), _stream())
    torch.cuda.synchronize()
    poff = _u64(d_poff)
    assert poff[:count + 1].tolist() == np.concatenate([[0], sizes.cumsum()]).tolist()
    assert (poff[count + 1:] == 0xFFFFFFFFFFFFFFFF).all(), "offsets past the total were written"
    assert bool((packed[int(sizes.sum()):] == FILL).all())
    st = status.cpu().numpy()
    want_st = (sizes == 0).astype(np.int32)
    assert st[:count].tolist() == want_st.tolist() and (st[count:] == -1).all()
    want = data.copy()
    want_full = np.concatenate([want, np.full(64, FILL, np.uint8)])
    for i in np.nonzero(sizes == 0)[0]:  # not decoded: the raw extent is left alone
        want_full[r.cuts[i]:r.cuts[i + 1]] = FILL
    want_full[:r.cuts[0]] = FILL
    want_full[r.cuts[count]:len(data)] = FILL
    assert np.array_equal(out.cpu().numpy(), want_full)
    return packed, poff[:count + 1]


# ---- parity with the oracle on every chunk ---------------------------------------------------------------------------------
def _corpus_inputs():
    files = [(n, corpus_file(n)) for n in corpus_names()]
    return files + [("canterbury", b"".join(f for _, f in files)), ("bible.txt", corpus_large_file("bible.txt"))]


PARAMS = {"8k": D8, "64-256-1024": SMALL, "2k-8k-64k-mask0": CM.params(2048, 8192, 65536, 0, 0),
          "2k-8k-64k-mask1": CM.params(2048, 8192, 65536, CM.M64, CM.M64)}


@pytest.mark.parametrize("pname", list(PARAMS))
@pytest.mark.parametrize("alg", ALGS)
def test_corpus_chunks_equal_the_oracle(cw, O, alg, pname):
    p = PARAMS[pname]
    for name, raw in _corpus_inputs():
        data = np.frombuffer(raw, np.uint8)
        r = Run(cw, alg, data, cdc=_params(cw, p)).fetch()
        assert r.cuts[0] == 0 and r.cuts[-1] == len(data), name
        by_chunk = check_run(cw, O, r, data)
        if pname in ("8k", "64-256-1024") and name in ("alice29.txt", "kennedy.xls", "canterbury"):
            roundtrip(cw, r, data, by_chunk)


@pytest.mark.parametrize("gen", ["mixed", "random"])
@pytest.mark.parametrize("alg", ALGS)
def test_generated_data_equals_the_oracle(cw, O, alg, gen):
    import torch
    n = 6 << 20
    t = torch.empty(n, dtype=torch.uint8, device="cuda")
    (cw.dev_gen_mixed if gen == "mixed" else cw.dev_gen_random)(0xC0DEC, 0, n // 4096, 4096, t.data_ptr(), _stream())
    torch.cuda.synchronize()
    data = t.cpu().numpy()
    for pname in PARAMS:
        r = Run(cw, alg, data, cdc=_params(cw, PARAMS[pname])).fetch()
        by_chunk = check_run(cw, O, r, data)
        if gen == "random" and alg == "lzf":  # LZF's "did not fit" is compared, not skipped: on noise that is every chunk
            assert len(by_chunk) == r.k and set(by_chunk.values()) == {0}
        if gen == "random" and alg == "lz4":
            assert all(v > r.cuts[i + 1] - r.cuts[i] for i, v in by_chunk.items())
        if pname == "8k":
            roundtrip(cw, r, data, by_chunk)


# ---- hand-made offset lists ---------------------------------------------------------------------------------------------------
LENGTHS = list(range(1, 21)) + [63, 64, 65, 4095, 4096, 4097, 65535, 65536]


def _kinds(n):
    rng = np.random.default_rng(31)
    text = np.frombuffer((corpus_file("alice29.txt") + corpus_file("lcet10.txt"))[:n], np.uint8)
    return {"text": text, "zeros": np.zeros(n, np.uint8), "ab": np.frombuffer((b"ab" * n)[:n], np.uint8),
            "noise": rng.integers(0, 256, n, dtype=np.uint8)}


@pytest.mark.parametrize("alg", ALGS)
def test_hand_made_lengths_at_every_misalignment(cw, O, alg):
    rng = np.random.default_rng(17)
    lens = LENGTHS + LENGTHS[:25]
    rng.shuffle(lens)
    cuts = np.concatenate([[0], np.cumsum(lens)]).tolist()
    kinds = _kinds(cuts[-1])
    for shift in range(1, 16):
        for kind in (("text", "zeros", "ab", "noise") if shift in (1, 8, 15) else (list(kinds)[shift % 4],)):
            data = kinds[kind]
            r = Run(cw, alg, data, cuts=cuts, shift=shift).fetch()  # the last chunk ends with the source buffer
            by_chunk = check_run(cw, O, r, data)
            assert len(by_chunk) == len(lens)
            if shift in (1, 15):
                roundtrip(cw, r, data, by_chunk)


@pytest.mark.parametrize("alg", ALGS)
def test_out_of_contract_chunks_get_size_0_and_write_nothing(cw, O, alg):
    data = _kinds(250000)["text"]
    n = len(data)
    # out of contract: chunk 1 (empty), 3 (65537 bytes), 5 (decreasing), 6 (75000 bytes, back up), 10 and 11 (past the source);
    # the others ascend without overlap
    cuts = [0, 500, 500, 3000, 3000 + 65537, 80000, 75000, 150000, 160000, 200000, n, n + 5, n + 10]
    r = Run(cw, alg, data, cuts=cuts).fetch()
    by_chunk = check_run(cw, O, r, data)
    assert sorted(by_chunk) == [0, 2, 4, 7, 8, 9]
    assert r.sizes[[1, 3, 5, 6, 10, 11]].tolist() == [0] * 6
    # an index past the chunk count, and a count below the list
    r = Run(cw, alg, data, cuts=cuts[:5] + [80000], sel=[4, 0, 7, 2, 1 << 31], count=4).fetch()
    check_run(cw, O, r, data, positions=[4, 0, 7, 2, 1 << 31])
    assert r.sizes[:5].tolist()[0] == 0 and r.sizes[2] == 0 and r.sizes[4] == 0 and r.sizes[1] > 0 and r.sizes[3] > 0
    # max_chunks below the count: chunks from max_chunks on are not compressed
    r = Run(cw, alg, data, cuts=[0, 1000, 2000, 3000, 4000], max_chunks=2).fetch()
    assert sorted(check_run(cw, O, r, data)) == [0, 1]


@pytest.mark.parametrize("alg", ALGS)
def test_scrambled_offsets_stay_inside_the_destination(cw, O, alg):
    """Overlapping and decreasing pairs throughout: slots may overlap, only the bounds are promised
    (slot(o, i) + bound(l) <= slot(src_bytes, max_chunks))."""
    rng = np.random.default_rng(23)
    data = _kinds(300000)["text"]
    n = len(data)
    cuts = rng.integers(0, n + 70000, 400)
    cuts[::7] = n
    cuts[3::11] = 0
    cuts[5::13] = n - rng.integers(0, 66000, len(cuts[5::13]))
    cuts[:50] = np.sort(cuts[:50])
    cuts = cuts.tolist()
    k = len(cuts) - 1
    r = Run(cw, alg, data, cuts=cuts).fetch()
    assert r.guards_ok
    assert (r.sizes[k:] == 0xFFFFFFFF).all()
    # the sizes do not depend on where the output went: exact for the in-contract chunks, 0 for the others
    ok = [i for i in range(k) if _in_contract(cuts, i, k, n)]
    assert 20 < len(ok) < k
    want = np.zeros(k, np.uint32)
    want[ok] = oracle_sizes(O, alg, data, cuts, ok, threads=4)
    assert r.sizes[:k].tolist() == want.tolist()


# ---- selection ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alg", ALGS)
def test_selection_writes_only_the_selected_slots(cw, O, alg):
    data = np.frombuffer(corpus_file("lcet10.txt") + corpus_file("kennedy.xls"), np.uint8)
    cuts = CM.chunk(data, CM.default_params(1024))
    k = len(cuts) - 1
    rng = np.random.default_rng(29)
    sel = rng.permutation(k)[:k // 3].tolist()  # a random subset in random order
    r = Run(cw, alg, data, cuts=cuts, sel=sel).fetch()
    by_chunk = check_run(cw, O, r, data, positions=sel)  # sizes[j] belongs to chunk sel[j]; unselected slots keep their fill
    assert len(by_chunk) == len(sel)
    # a count below the list; a count of 0 launches and writes nothing
    r = Run(cw, alg, data, cuts=cuts, sel=sel, nsel=10).fetch()
    check_run(cw, O, r, data, positions=sel[:10])
    r = Run(cw, alg, data, cuts=cuts, sel=sel, nsel=0).fetch()
    assert (r.sizes == 0xFFFFFFFF).all() and (r.image == FILL).all() and r.guards_ok


# ---- corrupted input to the decoder --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alg", ALGS)
def test_corrupted_packed_input_gets_the_oracles_verdict(cw, O, alg):
    import torch
    data = np.frombuffer(corpus_file("alice29.txt") + bytes(3000) + corpus_file("sum"), np.uint8)
    r = Run(cw, alg, data, cdc=_params(cw, SMALL)).fetch()
    packed, poff = roundtrip(cw, r, data, None)
    host = packed.cpu().numpy().copy()
    poff = poff.astype(np.int64).copy()
    rng = np.random.default_rng(41)
    k = r.k
    for j in rng.choice(k, 150, replace=False):  # a few flipped bytes
        if poff[j + 1] > poff[j]:
            host[int(rng.integers(poff[j], poff[j + 1]))] ^= int(rng.integers(1, 256))
    for j in rng.choice(np.arange(1, k), 40, replace=False):  # cut extents: position j - 1 loses its tail to position j
        poff[j] -= min(int(rng.integers(1, 6)), int(poff[j] - poff[j - 1]))
    decode = O.lz4_decompress if alg == "lz4" else O.lzf_decompress
    want, outs = [], {}
    for j in range(k):
        l = int(r.cuts[j + 1] - r.cuts[j])
        ext = host[poff[j]:poff[j + 1]]
        got = decode(ext, l) if len(ext) else None
        want.append(0 if got is not None and len(got) == l else 1)
        if want[-1] == 0:
            outs[j] = np.frombuffer(got, np.uint8)
    assert 30 < sum(want) < k
    d_packed = torch.from_numpy(host).cuda()
    d_poff = _dev_u64(poff)
    out = torch.full((GUARD + len(data) + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    status = torch.full((k,), -1, dtype=torch.int32, device="cuda")
    cw.dev_decompress_chunks(alg, d_packed.data_ptr(), d_poff.data_ptr(), r.d_off.data_ptr(), r.d_k.data_ptr(), k, out.data_ptr() + GUARD,
                             len(data), status.data_ptr(), _stream())
    torch.cuda.synchronize()
    assert status.cpu().numpy().tolist() == want
    o = out.cpu().numpy()
    assert (o[:GUARD] == FILL).all() and (o[-GUARD:] == FILL).all()
    for j, got in outs.items():  # (a flipped literal decodes, to other bytes)
        assert np.array_equal(o[GUARD + r.cuts[j]:GUARD + r.cuts[j + 1]], got), j
    # raw extents the decoder must skip: longer than 65536, decreasing, past dst_bytes
    raw = _dev_u64([0, 70000, 60000, 61000, len(data) + 1])
    comp = _dev_u64([0, 10, 20, 30, 40])
    status = torch.full((4,), -1, dtype=torch.int32, device="cuda")
    out.fill_(FILL)
    cw.dev_decompress_chunks(alg, d_packed.data_ptr(), comp.data_ptr(), raw.data_ptr(), _dev_u64([4]).data_ptr(), 4, out.data_ptr() + GUARD,
                             len(data), status.data_ptr(), _stream())
    torch.cuda.synchronize()
    assert status.cpu().numpy().tolist()[:2] == [1, 1] and int(status[3]) == 1
    assert bool((out[:GUARD + 60000] == FILL).all()) and bool((out[GUARD + 61000:] == FILL).all())


# ---- the fixed-size path and the chunk path run one loop ---------------------------------------------------------------------------
def _decode_through_both_decoders(cw, alg, payloads, data, bs):
    """One compressed result (payloads[i] = block i's bytes, b"" = LZF did not fit), laid out as fixed-stride slots for
    cw_dev_decompress (lane decoders forced) and as a packed stream for cw_dev_decompress_chunks: status 0 and the input's bytes
    for every block that has a compressed form, status 1 and nothing written for the others."""
    import torch
    nb = len(payloads)
    sizes = np.array([len(p) for p in payloads], np.int64)
    stride = (cw.compress_bound(alg, bs) + 15) // 16 * 16
    slots = np.full((nb, stride), FILL, np.uint8)
    for i, p in enumerate(payloads):
        slots[i, :len(p)] = np.frombuffer(p, np.uint8)
    d_slots = torch.from_numpy(slots).cuda()
    d_sizes = torch.from_numpy(sizes.astype(np.int32)).cuda()
    d_packed = torch.from_numpy(np.frombuffer(b"".join(payloads) + bytes(16), np.uint8).copy()).cuda()
    d_poff, d_raw, d_count = _dev_u64(np.concatenate([[0], sizes.cumsum()])), _dev_u64(np.arange(nb + 1) * bs), _dev_u64([nb])
    outs = []
    for door in ("blocks", "chunks"):
        out = torch.full((nb * bs + GUARD,), FILL, dtype=torch.uint8, device="cuda")
        status = torch.full((nb,), -1, dtype=torch.int32, device="cuda")
        if door == "blocks":
            with cw.tuned(CW_DECODE_LANES=1):
                cw.dev_decompress(alg, d_slots.data_ptr(), stride, d_sizes.data_ptr(), nb, out.data_ptr(), bs, status.data_ptr(), _stream())
        else:
            cw.dev_decompress_chunks(alg, d_packed.data_ptr(), d_poff.data_ptr(), d_raw.data_ptr(), d_count.data_ptr(), nb, out.data_ptr(),
                                     nb * bs, status.data_ptr(), _stream())
        torch.cuda.synchronize()
        assert status.cpu().numpy().tolist() == (sizes == 0).astype(int).tolist(), (alg, bs, door)
        outs.append(out.cpu().numpy())
    want = np.concatenate([data, np.full(GUARD, FILL, np.uint8)])
    for i in np.nonzero(sizes == 0)[0]:
        want[i * bs:(i + 1) * bs] = FILL
    for door, o in zip(("blocks", "chunks"), outs):
        assert np.array_equal(o, want), (alg, bs, door)


@pytest.mark.parametrize("bs", [70, 4093, 5001, 65536])
def test_one_codec_through_both_doors(cw, O, bs):
    """192 blocks (three wavefronts of lanes) of the Canterbury corpus, compressed once by cw_dev_compress with the lane-per-block
    parsers forced and once by cw_dev_compress_chunks over the offsets 0, bs, 2 bs, ...: the same loop behind both, so the same
    sizes and bytes, which are the oracle's; and both results decode to the input through the lane decoders of both paths.
    (The corpus is 2.8 MB: it is repeated to fill 192 blocks of 64 KiB; its length is no multiple of the block size, so the
    blocks still differ.  An LZF block that does not fit n - 1 bytes has no compressed form on either path: size 0, status 1.)"""
    import torch
    nb = 192
    corpus = b"".join(corpus_file(n) for n in corpus_names())
    data = np.frombuffer((corpus * (nb * bs // len(corpus) + 1))[:nb * bs], np.uint8)
    src = torch.from_numpy(data.copy()).cuda()
    cuts = [i * bs for i in range(nb + 1)]
    lz4_lanes = dict(CW_LZ4_LANES=1, CW_LZ4_LANES_RING=0, CW_LZ4_VTAB=0, CW_LANES_CONCURRENT=0)
    for alg, knob_sets in (("lz4", [lz4_lanes, dict(lz4_lanes, CW_LZ4_LANES_FP=0)]), ("lzf", [dict(CW_LZF_LANES=1)])):
        fn, scratch = _oracle_fn(O, alg), np.zeros(2 * 65536 + 64, np.uint8)
        want = []
        for i in range(nb):
            c = fn(data.ctypes.data + i * bs, bs, scratch.ctypes.data)
            want.append(scratch[:c].tobytes())
        results = []
        stride = (cw.compress_bound(alg, bs) + 15) // 16 * 16
        for knobs in knob_sets:
            dst = torch.full((nb * stride,), FILL, dtype=torch.uint8, device="cuda")
            sizes = torch.full((nb,), -1, dtype=torch.int32, device="cuda")
            with cw.tuned(**knobs):
                cw.dev_compress(alg, src.data_ptr(), bs, nb, dst.data_ptr(), stride, sizes.data_ptr(), _stream())
                torch.cuda.synchronize()
                assert alg + "_lanes_kernel" in cw.profile_kernels()["codec"], (knobs, cw.profile_kernels())
            hs, hd = sizes.cpu().numpy(), dst.cpu().numpy()
            results.append(("blocks %s" % knobs, [hd[i * stride:i * stride + hs[i]].tobytes() for i in range(nb)]))
        r = Run(cw, alg, data, cuts=cuts).fetch()
        assert alg + "_chunks_kernel" in cw.profile_kernels()["codec"] and r.guards_ok
        slot = [cw.chunk_slot_offset(alg, i * bs, i) for i in range(nb)]
        results.append(("chunks", [r.image[slot[i]:slot[i] + r.sizes[i]].tobytes() for i in range(nb)]))
        for door, got in results:
            bad = [i for i in range(nb) if got[i] != want[i]]
            assert not bad, (alg, bs, door, "block", bad[0], len(got[bad[0]]), len(want[bad[0]]), len(bad))
        for door, got in (results[0], results[-1]):
            _decode_through_both_decoders(cw, alg, got, data, bs)


def test_lz4_chunk_table_epoch_wraps(cw, O):
    """The LZ4 chunk table's epoch has 8 bits: after 255 parses a lane zeroes its table and starts again at 1.  Just under 256 KiB
    of input get one workgroup of 64 lanes, the input is cut into over 6,500 chunks of 20 .. 40 bytes, and the same call is made
    six times on one stream, where the lanes' epochs persist: every lane passes its 256th parse, most of them more than once.  The
    text repeats at distances inside a chunk, so an entry left by an earlier parse that were taken for one of this parse would be
    a match the reference does not find.  Every call's sizes and bytes are the oracle's.
    (The LZF table's epoch has 16 bits: wrapping it takes 65,536 chunks per lane, which no test of this size can supply.)"""
    rng = np.random.default_rng(47)
    text = corpus_file("alice29.txt")
    pieces, total, k = [], 0, 0
    while total < (256 << 10):  # every piece of 5 .. 11 bytes two or three times in a row
        piece = text[5 * k:5 * k + 5 + k % 7] * (2 + k % 2)
        pieces.append(piece); total += len(piece); k += 1
    lens = rng.integers(20, 41, (256 << 10) // 40).tolist()  # (fits whatever is drawn)
    while sum(lens) + 40 < (256 << 10):
        lens.append(int(rng.integers(20, 41)))
    cuts = np.concatenate([[0], np.cumsum(lens)]).tolist()
    data = np.frombuffer(b"".join(pieces)[:cuts[-1]], np.uint8)
    assert len(data) < (256 << 10) and len(lens) >= 6500 and 64 * 256 * 2 < 6 * len(lens)
    want_sizes = want_img = None
    for call in range(6):
        r = Run(cw, "lz4", data, cuts=cuts).fetch()
        if want_sizes is None:
            want_sizes, want_img = oracle_image(cw, O, "lz4", data, cuts, range(len(lens)), r.total)
            assert (want_sizes < np.array(lens)).sum() > len(lens) // 2  # most chunks have matches
        bad = np.nonzero(r.sizes[:len(lens)] != want_sizes)[0]
        assert len(bad) == 0, (call, "chunk", int(bad[0]), int(r.sizes[bad[0]]), int(want_sizes[bad[0]]), len(bad))
        diff = np.nonzero(r.image != want_img)[0]
        assert len(diff) == 0 and r.guards_ok, (call, "slot image differs at", int(diff[0]) if len(diff) else None, len(diff))


# ---- a large batch ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alg", ALGS)
def test_one_gib_of_tiled_corpus(cw, O, alg):
    """Over 100 k chunks: every lane holds a chunk and takes further ones.  The cuts are the device's (cw_dev_cdc is pinned to the
    model by tests/test_gpu_cdc.py); every size against the oracle, payloads on a fixed sample, all chunks round-tripped."""
    import torch
    corpus = np.frombuffer(b"".join(f for _, f in _corpus_inputs()[:-2]) + corpus_large_file("bible.txt"), np.uint8)
    n = 1 << 30
    src = torch.from_numpy(corpus).cuda().repeat(n // len(corpus) + 1)[:n].contiguous()
    p = cw.CdcParams.default(8192)
    cap = p.max_offsets(n)
    d_off = torch.zeros(cap, dtype=torch.int64, device="cuda")
    d_k = torch.zeros(1, dtype=torch.int64, device="cuda")
    total = cw.chunk_slots_bytes(alg, n, cap - 1)
    dst = torch.full((GUARD + total + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    d_sizes = torch.full((cap,), -1, dtype=torch.int32, device="cuda")
    cw.dev_cdc(p, src.data_ptr(), n, True, d_off.data_ptr(), cap, d_k.data_ptr(), _stream())
    cw.dev_compress_chunks(alg, src.data_ptr(), n, d_off.data_ptr(), d_k.data_ptr(), cap - 1, dst.data_ptr() + GUARD, total,
                           d_sizes.data_ptr(), _stream())
    torch.cuda.synchronize()
    k = int(d_k.item())
    assert k > 100_000
    cuts = _u64(d_off)[:k + 1].astype(np.int64)
    sizes = d_sizes.cpu().numpy().view(np.uint32)
    host = src.cpu().numpy()
    want = oracle_sizes(O, alg, host, cuts, range(k))
    bad = np.nonzero(sizes[:k] != want)[0]
    print(f"{alg}: {k} chunks, {int(want.sum())} compressed bytes, {int((want == 0).sum())} did not fit, {len(bad)} sizes differ")
    assert len(bad) == 0, (int(bad[0]), int(sizes[bad[0]]), int(want[bad[0]]))
    assert (sizes[k:] == 0xFFFFFFFF).all()
    assert bool((dst[:GUARD] == FILL).all()) and bool((dst[-GUARD:] == FILL).all())
    sample = sorted(set(range(64)) | set(range(k - 64, k)) | set(np.random.default_rng(43).choice(k, 2000, replace=False).tolist()))
    fn, scratch = _oracle_fn(O, alg), np.zeros(2 * 65536 + 64, np.uint8)
    for i in sample:
        c = fn(host.ctypes.data + int(cuts[i]), int(cuts[i + 1] - cuts[i]), scratch.ctypes.data)
        slot = GUARD + cw.chunk_slot_offset(alg, int(cuts[i]), i)
        assert c == sizes[i] and np.array_equal(dst[slot:slot + c].cpu().numpy(), scratch[:c]), i
    # all chunks back through pack and the decoder
    d_poff = torch.zeros(k + 1, dtype=torch.int64, device="cuda")
    packed = torch.empty(int(want.sum()) + 16, dtype=torch.uint8, device="cuda")
    del host
    cw.dev_pack_chunks(alg, dst.data_ptr() + GUARD, d_off.data_ptr(), d_k.data_ptr(), cap - 1, d_sizes.data_ptr(), packed.data_ptr(),
                       d_poff.data_ptr(), _stream())
    torch.cuda.synchronize()
    del dst
    assert int(_u64(d_poff[k:k + 1])[0]) == int(want.sum())
    out = torch.zeros(n, dtype=torch.uint8, device="cuda")
    status = torch.full((k,), -1, dtype=torch.int32, device="cuda")
    cw.dev_decompress_chunks(alg, packed.data_ptr(), d_poff.data_ptr(), d_off.data_ptr(), d_k.data_ptr(), cap - 1, out.data_ptr(), n,
                             status.data_ptr(), _stream())
    torch.cuda.synchronize()
    st = status.cpu().numpy()
    assert np.array_equal(st, (want == 0).astype(np.int32))
    for i in np.nonzero(want == 0)[0]:  # did not fit: kept raw by the caller
        assert bool((out[cuts[i]:cuts[i + 1]] == 0).all())
        out[cuts[i]:cuts[i + 1]] = src[cuts[i]:cuts[i + 1]]
    assert torch.equal(out, src)


# ---- the fused call ---------------------------------------------------------------------------------------------------------------
def _edited_bible():
    a = corpus_large_file("bible.txt")
    b = bytearray(a)
    for pos in (1, 500_000, 1_700_000, 3_000_000):
        b[pos:pos] = b"INSERTED"
    del b[2_500_000:2_500_100]
    return a, bytes(b)


class Bufs:
    def __init__(self, cw, alg, p, nbytes, db):
        import torch
        self.cap = p.max_offsets(nbytes)
        z = lambda n, dt: torch.zeros(n, dtype=dt, device="cuda")  # noqa: E731
        self.off, self.k = z(self.cap, torch.int64), z(1, torch.int64)
        self.dig, self.ref = z(self.cap * db, torch.uint8), z(self.cap, torch.int64)
        self.new_idx, self.n_new = z(self.cap, torch.int32), z(1, torch.int64)
        self.total = cw.chunk_slots_bytes(alg, nbytes, self.cap - 1)
        self.dst = torch.full((self.total,), FILL, dtype=torch.uint8, device="cuda")
        self.sizes = torch.full((self.cap,), -1, dtype=torch.int32, device="cuda")

    def host(self):
        k, m = int(self.k.item()), int(self.n_new.item())
        return dict(k=k, n_new=m, off=_u64(self.off)[:k + 1].tolist(), dig=self.dig.cpu().numpy().tobytes(),
                    ref=_u64(self.ref)[:k].tolist(), new_idx=self.new_idx[:m].cpu().numpy().tolist(),
                    sizes=self.sizes.cpu().numpy().tolist(), dst=self.dst.cpu().numpy())


def _fused(cw, idx, alg, p, src, base, stream, final=True):
    import torch
    b = Bufs(cw, alg, p, src.numel(), cw.digest_bytes("skein512"))
    torch.cuda.synchronize()  # (torch filled the buffers on its own stream)
    k = idx.dev_cdc_dedupe_compress(p, alg, src.data_ptr(), src.numel(), final, base, b.off.data_ptr(), b.cap, b.k.data_ptr(), b.dig.data_ptr(),
                                    b.ref.data_ptr(), b.new_idx.data_ptr(), b.n_new.data_ptr(), b.dst.data_ptr(), b.total, b.sizes.data_ptr(),
                                    stream)
    return b, k


def _unfused(cw, idx, alg, p, src, base, stream, final=True):
    import torch
    b = Bufs(cw, alg, p, src.numel(), cw.digest_bytes("skein512"))
    n = src.numel()
    torch.cuda.synchronize()
    cw.dev_cdc(p, src.data_ptr(), n, final, b.off.data_ptr(), b.cap, b.k.data_ptr(), stream)
    cw.dev_hash_chunks("skein512", src.data_ptr(), n, b.off.data_ptr(), b.k.data_ptr(), b.cap - 1, b.dig.data_ptr(), stream)
    torch.cuda.synchronize()
    k = int(b.k.item())
    idx.dev_dedupe(b.dig.data_ptr(), k, base, b.ref.data_ptr(), b.new_idx.data_ptr(), b.n_new.data_ptr(), stream)
    cw.dev_compress_chunks(alg, src.data_ptr(), n, b.off.data_ptr(), b.k.data_ptr(), b.cap - 1, b.dst.data_ptr(), b.total, b.sizes.data_ptr(),
                           stream, b.new_idx.data_ptr(), b.n_new.data_ptr())
    return b, k


@pytest.mark.parametrize("alg", ALGS)
def test_fused_call_on_an_edited_copy(cw, O, alg):
    import torch
    a, b = _edited_bible()
    p = cw.CdcParams.default(1024)
    srcs = [torch.from_numpy(np.frombuffer(x, np.uint8).copy()).cuda() for x in (a, b)]
    side = torch.cuda.Stream()
    results = []
    for stream in (_stream(), side.cuda_stream):
        fused_idx, plain_idx = cw.DedupeIndex("skein512", 1 << 16), cw.DedupeIndex("skein512", 1 << 16)
        per_call = []
        for src, base in zip(srcs, (0, 1 << 32)):
            fb, fk = _fused(cw, fused_idx, alg, p, src, base, stream)
            ub, uk = _unfused(cw, plain_idx, alg, p, src, base, stream)
            torch.cuda.synchronize()
            f, u = fb.host(), ub.host()
            assert fk == uk == f["k"] == u["k"]
            for key in ("off", "dig", "ref", "new_idx", "n_new", "sizes"):
                assert f[key] == u[key], key
            assert np.array_equal(f["dst"], u["dst"])  # the slot bytes of the new chunks (and nothing else written)
            per_call.append((fb, f))
        assert fused_idx.count() == plain_idx.count() == per_call[0][1]["n_new"] + per_call[1][1]["n_new"]
        results.append([f for _, f in per_call])
        # first call: every distinct chunk is new; second call: >= 99 % of the bytes lie in chunks it does not compress
        f0, f1 = results[-1]
        assert f0["n_new"] == f0["k"]
        lens = np.diff(np.array(f1["off"], np.int64))
        assert 1 - lens[f1["new_idx"]].sum() / len(b) >= 0.99
        # the new chunks of the second call: oracle sizes, then pack + decode gives their bytes back
        fb, f = per_call[1]
        data = np.frombuffer(b, np.uint8)
        want = oracle_sizes(O, alg, data, f["off"], f["new_idx"], threads=4)
        assert f["sizes"][:f["n_new"]] == want.tolist()
        m = f["n_new"]
        poff = torch.zeros(m + 1, dtype=torch.int64, device="cuda")
        packed = torch.zeros(int(want.sum()) + 16, dtype=torch.uint8, device="cuda")
        raw = np.concatenate([[0], lens[f["new_idx"]].cumsum()])
        d_raw = _dev_u64(raw)
        out = torch.zeros(int(raw[-1]) + 16, dtype=torch.uint8, device="cuda")
        status = torch.full((m,), -1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        cw.dev_pack_chunks(alg, fb.dst.data_ptr(), fb.off.data_ptr(), fb.n_new.data_ptr(), fb.cap - 1, fb.sizes.data_ptr(), packed.data_ptr(),
                           poff.data_ptr(), stream, fb.new_idx.data_ptr())
        cw.dev_decompress_chunks(alg, packed.data_ptr(), poff.data_ptr(), d_raw.data_ptr(), fb.n_new.data_ptr(), m, out.data_ptr(), int(raw[-1]),
                                 status.data_ptr(), stream)
        torch.cuda.synchronize()
        new_bytes = np.concatenate([data[f["off"][i]:f["off"][i + 1]] for i in f["new_idx"]])
        fit = want > 0
        assert status.cpu().numpy().tolist() == (~fit).astype(int).tolist()
        o = out.cpu().numpy()
        for j in np.nonzero(fit)[0]:
            assert np.array_equal(o[raw[j]:raw[j + 1]], new_bytes[raw[j]:raw[j + 1]]), j
        fused_idx.close(); plain_idx.close()
    for x, y in zip(results[0], results[1]):  # the other stream gives identical results
        for key in ("off", "dig", "ref", "new_idx", "n_new", "sizes"):
            assert x[key] == y[key], key
        assert np.array_equal(x["dst"], y["dst"])


def test_fused_streaming_pieces_give_the_cuts_of_one_call(cw):
    import torch
    a, _ = _edited_bible()
    p = cw.CdcParams.default(1024)
    src = torch.from_numpy(np.frombuffer(a, np.uint8).copy()).cuda()
    with cw.DedupeIndex("skein512", 1 << 16) as whole_idx, cw.DedupeIndex("skein512", 1 << 16) as idx:
        wb, wk = _fused(cw, whole_idx, "lz4", p, src, 0, _stream())
        whole = wb.host()
        first = src[:1_500_000].contiguous()
        b1, k1 = _fused(cw, idx, "lz4", p, first, 0, _stream(), final=False)
        h1 = b1.host()
        used = h1["off"][k1]
        assert 0 < used <= 1_500_000 and 1_500_000 - used < p.max_size
        rest = src[used:].contiguous()
        b2, k2 = _fused(cw, idx, "lz4", p, rest, k1, _stream(), final=True)
        h2 = b2.host()
        assert h1["off"] + [used + x for x in h2["off"][1:]] == whole["off"] and k1 + k2 == wk
        assert h1["dig"][:k1 * 64] + h2["dig"][:k2 * 64] == whole["dig"][:wk * 64]
        assert h1["ref"] + h2["ref"] == whole["ref"]  # values base + i line up with the one call's chunk numbers


def test_fused_call_on_a_full_index_returns_nomem(cw):
    import torch
    a, _ = _edited_bible()
    p = cw.CdcParams.default(1024)
    src = torch.from_numpy(np.frombuffer(a[:1 << 20], np.uint8).copy()).cuda()
    with cw.DedupeIndex("skein512", 100) as idx:
        with pytest.raises(cw.CwError) as e:
            _fused(cw, idx, "lz4", p, src, 0, _stream())
        assert e.value.code == CW_ERR_NOMEM and e.value.nchunks > 100
        assert idx.count() == 0
    with cw.DedupeIndex("skein512", e.value.nchunks) as idx:  # retry with a larger index
        b, k = _fused(cw, idx, "lz4", p, src, 0, _stream())
        torch.cuda.synchronize()
        assert k == e.value.nchunks and idx.count() == int(b.n_new.item())


# ---- two host threads on one stream ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alg", ALGS)
def test_two_threads_on_one_stream_get_exact_results(cw, O, alg):
    """The launch lock of the stream's workspace keeps one call's sort and parse launches together: the order, the work counter
    and the lane tables are shared by every call on the stream."""
    import torch
    inputs = [np.frombuffer(corpus_file("lcet10.txt"), np.uint8), np.frombuffer(corpus_file("kennedy.xls")[:900000], np.uint8)]
    params = [_params(cw, SMALL), cw.CdcParams.default(1024)]
    stream = _stream()
    for _ in range(3):
        runs = [None, None]
        gate = threading.Barrier(2)

        def work(t):
            cw.init(0)
            gate.wait()
            runs[t] = [Run(cw, alg, inputs[t], cdc=params[t], stream=stream) for _ in range(4)]

        threads = [threading.Thread(target=work, args=(t,)) for t in range(2)]
        for th in threads:
            th.start()
        for th in threads:
            th.join()
        torch.cuda.synchronize()
        for t in range(2):
            for r in runs[t]:
                check_run(cw, O, r.fetch(), inputs[t])
