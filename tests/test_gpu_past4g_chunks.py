"""The chunk doors over a source longer than 2^32 bytes: ``N = 2^32 + 8 MiB`` of tiled corpus, built on the device,
with noise blocks spliced into the window ``[2^32 - 1 MiB, 2^32 + 1 MiB)``.

* cw_dev_hash_chunks, cw_dev_compress_chunks (whole and with d_sel), cw_dev_pack_chunks and cw_dev_decompress_chunks take hand-made cuts
  (tests/past4g.py): the window's chunks against the oracle over the window's bytes, slot image included; the bulk, which is whole
  64 KiB blocks, against cw_dev_hash / cw_dev_compress of the same blocks, on the device.
* cw_dev_cdc, cw_dev_cdc_streams and cw_dev_cdc_streams_part with ``nbytes = N``: by the restart property (proven on the model in
  tests/test_past4g_model.py) the cuts from the last cut below the window on are those of the suffix chunked alone, whose offsets are
  small, and the cuts below it those of the prefix; the window's cuts are the model's.

Only windows and small arrays come back to the host; nothing here has a tolerance."""
import contextlib

import numpy as np
import pytest

import cdc_model as CM
import past4g as P4
import streams_ingest_model as SIM
import streams_model as SM
from conftest import corpus_file, corpus_large_file, corpus_names

pytestmark = pytest.mark.gpu
B, N, MIB, BLOCK, WIN_LO, WIN_HI = P4.B, P4.N, P4.MIB, P4.BLOCK, P4.WIN_LO, P4.WIN_HI
FILL, GUARD, PAD, MARGIN = 0xA5, 256, 8, 65536
POISON = 0xABABABABABABABAB
D8 = CM.default_params(8192)
SMALL = CM.params(64, 256, 1024, CM.top_bits(10), CM.top_bits(6))
ODD_SEGMENT = 5 * 65536                                                     # a CW_CDC_SEGMENT that does not divide 2^32
HASHES = ["skein512", "skein", "sha256"]
ALGS = ["lz4", "lzf"]


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


def _dev_u64(values):
    import torch
    return torch.from_numpy(np.asarray(values, np.uint64).view(np.int64).copy()).cuda()


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


def _poison(n):
    import torch
    return torch.full((n,), POISON - (1 << 64), dtype=torch.int64, device="cuda")


def _params(cw, p):
    return cw.CdcParams(p["min"], p["avg"], p["max"], p["mask_s"], p["mask_l"], p.get("gear"))


@contextlib.contextmanager
def segment(cw, S):
    if S:
        cw.tune_set("CW_CDC_SEGMENT", str(S))
    try:
        yield
    finally:
        if S:
            cw.tune_set("CW_CDC_SEGMENT", None)


class Src:
    """The source on the device and its window on the host."""

    def __init__(self, cw):
        import torch
        corpus = np.frombuffer(b"".join(corpus_file(n) for n in corpus_names()) + corpus_large_file("bible.txt"), np.uint8)
        self.dev = P4.tiled_source(torch, corpus, N, lambda first, count, dst: cw.dev_gen_random(0x4A57, first, count, BLOCK, dst.data_ptr(), _stream()))
        torch.cuda.synchronize()
        assert self.dev.numel() == N > B
        self.window = self.dev[WIN_LO - MARGIN:WIN_HI + MARGIN].cpu().numpy()
        self.ptr = self.dev.data_ptr()

    def host(self, a, b):
        assert WIN_LO - MARGIN <= a <= b <= WIN_HI + MARGIN
        return self.window[a - WIN_LO + MARGIN:b - WIN_LO + MARGIN]


@pytest.fixture(scope="module")
def src(cw):
    import torch
    s = Src(cw)
    yield s
    del s.dev
    torch.cuda.empty_cache()


@pytest.fixture(autouse=True)
def _free():
    yield
    import torch
    torch.cuda.empty_cache()


def test_window_mixes_text_and_noise(src, oracle):
    sizes = [len(oracle.lzf_compress(src.host(a, a + BLOCK).tobytes())) for a in range(WIN_LO, WIN_HI, BLOCK)]
    assert 8 <= sum(1 for s in sizes if s == 0) <= 12 and sum(1 for s in sizes if 0 < s < BLOCK) >= 16, sizes
    assert sizes[15] and sizes[16] and not sizes[14] and not sizes[17]      # text on either side of 2^32, noise around it


# ---- 1a: hand-made cuts --------------------------------------------------------------------------------------------------------------
def _digest(oracle, alg, data):
    return oracle.skein512(data) if alg == "skein512" else oracle.skein256(data) if alg == "skein" else oracle.sha256(data)


@pytest.mark.parametrize("variant", P4.VARIANTS)
@pytest.mark.parametrize("alg", HASHES)
def test_hash_chunks(cw, oracle, src, alg, variant):
    import torch
    cuts = P4.hand_cuts(variant)
    k, win = len(cuts) - 1, P4.window_chunks(cuts)
    d_off, d_k, db = _dev_u64(cuts), _dev_u64([k]), cw.digest_bytes(alg)
    dig = torch.full((k + PAD, db), 0xEE, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    cw.dev_hash_chunks(alg, src.ptr, N, d_off.data_ptr(), d_k.data_ptr(), k, dig.data_ptr(), _stream())
    torch.cuda.synchronize()
    got = dig[int(win[0]):int(win[-1]) + 1].cpu().numpy()
    c = cuts.astype(np.int64)
    for n, i in enumerate(win):
        assert got[n].tobytes() == _digest(oracle, alg, src.host(c[i], c[i + 1]).tobytes()), (variant, int(i), int(c[i]), int(c[i + 1]))
    P4.assert_reaches(c[win], c[win + 1], "hashed window chunks", over=variant == "straddle")
    # the bulk is whole blocks: the fixed-block call over the same bytes
    below, above = int(win[0]), k - int(win[-1]) - 1
    assert below == WIN_LO // BLOCK and above == (N - WIN_HI) // BLOCK
    ref = torch.empty((below, db), dtype=torch.uint8, device="cuda")
    cw.dev_hash(alg, src.ptr, BLOCK, below, ref.data_ptr(), _stream())
    torch.cuda.synchronize()
    assert torch.equal(dig[:below], ref), (dig[:below] != ref).any(dim=1).nonzero()[:4].tolist()
    cw.dev_hash(alg, src.ptr + WIN_HI, BLOCK, above, ref.data_ptr(), _stream())
    torch.cuda.synchronize()
    assert torch.equal(dig[k - above:k], ref[:above]), (dig[k - above:k] != ref[:above]).any(dim=1).nonzero()[:4].tolist()
    assert bool((dig[k:] == 0xEE).all())


def _oracle_fn(oracle, alg):
    L = oracle.lib()
    if alg == "lz4":
        return lambda a, dst: L.cw_oracle_lz4_compress(a.ctypes.data, len(a), dst.ctypes.data, len(a) + len(a) // 255 + 16)
    return lambda a, dst: L.cw_oracle_lzf_compress(a.ctypes.data, len(a), dst.ctypes.data, len(a) - 1) if len(a) > 1 else 0


def _window_image(cw, oracle, alg, src, cuts, win, lo, hi):
    """(sizes, the oracle's compressed chunks, the image of the slot bytes [lo, hi) after the window's chunks; LZF chunks that did not
    fit leave their slot unspecified: the mask is False there)."""
    fn, scratch = _oracle_fn(oracle, alg), np.zeros(2 * BLOCK + 64, np.uint8)
    img, mask, sizes, comp = np.full(hi - lo, FILL, np.uint8), np.ones(hi - lo, bool), np.zeros(len(win), np.uint32), []
    for n, i in enumerate(win):
        a, b = int(cuts[i]), int(cuts[i + 1])
        size = fn(np.ascontiguousarray(src.host(a, b)), scratch)
        slot = cw.chunk_slot_offset(alg, a, int(i)) - lo
        assert 0 <= slot and slot + max(size, b - a) <= hi - lo
        img[slot:slot + size] = scratch[:size]
        if size == 0:
            mask[slot:slot + b - a] = False
        sizes[n] = size
        comp.append(scratch[:size].copy())
    return sizes, comp, img, mask


@pytest.mark.parametrize("variant", P4.VARIANTS)
@pytest.mark.parametrize("alg", ALGS)
def test_compress_pack_decompress_chunks(cw, oracle, src, alg, variant):
    import torch
    cuts = P4.hand_cuts(variant)
    c = cuts.astype(np.int64)
    k, win = len(cuts) - 1, P4.window_chunks(cuts)
    w0, w1 = int(win[0]), int(win[-1]) + 1
    below, above = w0, k - w1
    d_off, d_k = _dev_u64(cuts), _dev_u64([k])
    total = cw.chunk_slots_bytes(alg, N, k)
    assert total > B
    slot = lambda i: cw.chunk_slot_offset(alg, int(c[i]), i)  # noqa: E731
    dst = torch.full((GUARD + total + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    slots = dst[GUARD:GUARD + total]
    sizes = torch.full((k + PAD,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    cw.dev_compress_chunks(alg, src.ptr, N, d_off.data_ptr(), d_k.data_ptr(), k, slots.data_ptr(), total, sizes.data_ptr(), _stream())
    torch.cuda.synchronize()
    # the window: sizes, bytes and the gaps between the slots, from the first window slot up to the first slot behind the window
    lo, hi = slot(w0), slot(w1)
    assert (lo < B < hi) == (alg == "lzf")                                    # an LZ4 slot lies o / 255 + 32 i above its chunk: those pass 2^32 in the bulk
    want_sizes, comp, img, mask = _window_image(cw, oracle, alg, src, c, win, lo, hi)
    got_sizes = sizes[w0:w1].cpu().numpy().view(np.uint32)
    bad = np.nonzero(got_sizes != want_sizes)[0]
    assert len(bad) == 0, (int(win[bad[0]]), int(got_sizes[bad[0]]), int(want_sizes[bad[0]]), len(bad))
    got = slots[lo:hi].cpu().numpy()
    bad = np.nonzero((got != img) & mask)[0]
    assert len(bad) == 0, ("slot image", lo + int(bad[0]), len(bad))
    if alg == "lzf":
        assert (want_sizes == 0).sum() > 10 and (want_sizes > 0).sum() > 50                # LZF both accepts and refuses in the window
    starts = np.array([slot(int(i)) for i in win], np.int64)
    if alg == "lzf":
        P4.assert_reaches(starts, starts + np.maximum(want_sizes, 1), "window slots", over=False)
    bulk_slots = np.array([slot(i) for i in range(below)], np.int64)
    cross = int(np.searchsorted(bulk_slots, B))                               # the first bulk chunk whose slot lies at or above 2^32
    assert (64 + 8 < cross < below - 64 - 8) == (alg == "lz4") and (alg == "lzf" or bulk_slots[cross - 1] < B <= bulk_slots[cross])
    P4.assert_reaches(c[win], c[win + 1], "compressed window chunks", over=variant == "straddle")
    assert bool((sizes[k:] == -1).all()) and bool((dst[:GUARD] == FILL).all()) and bool((dst[-GUARD:] == FILL).all())
    # the bulk's sizes: the fixed-block codec over the same blocks
    stride = (cw.compress_bound(alg, BLOCK) + 15) // 16 * 16
    bdst = torch.empty(below * stride, dtype=torch.uint8, device="cuda")
    bsizes, asizes = torch.zeros(below, dtype=torch.int32, device="cuda"), torch.zeros(above, dtype=torch.int32, device="cuda")
    adst = torch.empty(above * stride, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    cw.dev_compress(alg, src.ptr, BLOCK, below, bdst.data_ptr(), stride, bsizes.data_ptr(), _stream())
    cw.dev_compress(alg, src.ptr + WIN_HI, BLOCK, above, adst.data_ptr(), stride, asizes.data_ptr(), _stream())
    torch.cuda.synchronize()
    assert torch.equal(sizes[:below], bsizes), (sizes[:below] != bsizes).nonzero()[:4].tolist()
    assert torch.equal(sizes[w1:k], asizes), (sizes[w1:k] != asizes).nonzero()[:4].tolist()
    assert int((bsizes > 0).sum()) > below // 2 and int((asizes > 0).sum()) > above // 2
    # a slice of the bulk through d_sel, into fresh slots: bytes too, and nothing between the groups of slots is written
    groups = [range(0, 64)] + ([range(cross - 8, cross + 8)] if alg == "lz4" else []) + [range(below - 64, below), range(w1, w1 + 64), range(k - 16, k)]
    sel = np.array([i for g in groups for i in g], np.uint32)
    d_sel, d_nsel = torch.from_numpy(sel.view(np.int32).copy()).cuda(), _dev_u64([len(sel)])
    ssizes = torch.full((len(sel) + PAD,), -1, dtype=torch.int32, device="cuda")
    dst.fill_(FILL)
    torch.cuda.synchronize()
    cw.dev_compress_chunks(alg, src.ptr, N, d_off.data_ptr(), d_k.data_ptr(), k, slots.data_ptr(), total, ssizes.data_ptr(), _stream(),
                           d_sel.data_ptr(), d_nsel.data_ptr())
    torch.cuda.synchronize()
    h_sizes = sizes.cpu().numpy()
    assert ssizes[:len(sel)].cpu().numpy().tolist() == h_sizes[sel].tolist() and bool((ssizes[len(sel):] == -1).all())
    for i in sel.tolist():
        n = int(h_sizes[i])
        want = bdst[i * stride:i * stride + n] if i < below else adst[(i - w1) * stride:(i - w1) * stride + n]
        assert torch.equal(slots[slot(i):slot(i) + n], want), ("selected chunk", i)
    edge = lambda g: (slot(g[0]), slot(g[-1]) + BLOCK + BLOCK // 255 + 16)  # noqa: E731
    for g, h in zip(groups[:-1], groups[1:]):
        assert bool((slots[edge(g)[1]:edge(h)[0]] == FILL).all()), ("a slot between the selected groups was written", g, h)
    assert bool((dst[:GUARD] == FILL).all()) and bool((dst[-GUARD:] == FILL).all())
    del bdst, adst
    # the window and 64 chunks at either end through pack and the decoder; the two gaps are positions with nothing to decode
    dst.fill_(FILL)
    torch.cuda.synchronize()
    cw.dev_compress_chunks(alg, src.ptr, N, d_off.data_ptr(), d_k.data_ptr(), k, slots.data_ptr(), total, sizes.data_ptr(), _stream())
    chunks = list(range(64)) + [64] + list(range(w0, w1)) + [w1] + list(range(k - 64, k))
    gaps = (64, 65 + len(win))
    raw = [int(c[i]) for i in chunks] + [N]
    raw[gaps[0]], raw[gaps[1]] = 64 * BLOCK, WIN_HI
    psizes = h_sizes[np.array(chunks)].astype(np.uint32)
    psizes[list(gaps)] = 0
    npos = len(chunks)
    d_psel, d_psizes, d_n = torch.from_numpy(np.array(chunks, np.uint32).view(np.int32).copy()).cuda(), torch.from_numpy(psizes.view(np.int32).copy()).cuda(), _dev_u64([npos])
    d_poff, packed = _poison(npos + 1 + PAD), torch.full((int(psizes.sum()) + 16,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    cw.dev_pack_chunks(alg, slots.data_ptr(), d_off.data_ptr(), d_n.data_ptr(), npos, d_psizes.data_ptr(), packed.data_ptr(), d_poff.data_ptr(),
                       _stream(), d_psel.data_ptr())
    torch.cuda.synchronize()
    poff = _u64(d_poff)
    assert poff[:npos + 1].tolist() == np.concatenate([[0], np.cumsum(psizes, dtype=np.uint64)]).tolist() and (poff[npos + 1:] == POISON).all()
    h_packed = packed.cpu().numpy()
    assert (h_packed[int(psizes.sum()):] == FILL).all()
    for n, i in enumerate(win):
        at = int(poff[65 + n])
        assert np.array_equal(h_packed[at:at + len(comp[n])], comp[n]), ("packed window chunk", int(i))
    del dst, slots
    torch.cuda.empty_cache()
    out = torch.full((N,), 0x5C, dtype=torch.uint8, device="cuda")
    status = torch.full((npos + PAD,), -1, dtype=torch.int32, device="cuda")
    d_raw = _dev_u64(raw)
    torch.cuda.synchronize()
    cw.dev_decompress_chunks(alg, packed.data_ptr(), d_poff.data_ptr(), d_raw.data_ptr(), d_n.data_ptr(), npos, out.data_ptr(), N, status.data_ptr(),
                             _stream())
    torch.cuda.synchronize()
    st = status.cpu().numpy()
    assert st[:npos].tolist() == [0 if s else 1 for s in psizes.tolist()] and (st[npos:] == -1).all()
    want = torch.full((N,), 0x5C, dtype=torch.uint8, device="cuda")
    decoded = [(raw[j], raw[j + 1]) for j in range(npos) if psizes[j]]
    for a, b in decoded:
        want[a:b] = src.dev[a:b]
    assert torch.equal(out, want), ("decoded bytes or the poison between them", (out != want).nonzero()[:4].tolist())
    P4.assert_reaches([a for a, _ in decoded], [b for _, b in decoded], "decoded extents", over=variant == "straddle")                     # (the chunk across 2^32 is text: LZF takes it too)
    assert any(a >= B for a, _ in decoded) and (alg == "lzf") == bool((psizes[65:65 + len(win)] == 0).any())


# ---- 1b: the chunker -----------------------------------------------------------------------------------------------------------------
def dev_cdc(cw, cp, ptr, n, final):
    """(the offsets on the device as i64, K); every output poisoned behind its valid part."""
    import torch
    cap = cp.max_offsets(n)
    offs, k = _poison(cap + PAD), _poison(1 + PAD)
    torch.cuda.synchronize()
    cw.dev_cdc(cp, ptr, n, final, offs.data_ptr(), cap, k.data_ptr(), _stream())
    torch.cuda.synchronize()
    kk = int(k[0].item())
    assert 0 <= kk < cap and bool((offs[kk + 1:] == POISON - (1 << 64)).all()) and bool((k[1:] == POISON - (1 << 64)).all())
    return offs[:kk + 1], kk


@pytest.mark.parametrize("seg", [0, ODD_SEGMENT], ids=["default_segment", "odd_segment"])
@pytest.mark.parametrize("p", [D8, SMALL], ids=["default8192", "small"])
def test_cdc_of_the_whole_source(cw, src, p, seg):
    import torch
    cp = cw.CdcParams.default(8192) if p is D8 else _params(cw, p)
    assert (cp.min_size, cp.normal_size, cp.max_size) == (p["min"], p["avg"], p["max"]) and p["min"] >= 64 and (seg == 0 or B % seg)
    with segment(cw, seg):
        whole, K = dev_cdc(cw, cp, src.ptr, N, True)
        assert int(whole[0]) == 0 and int(whole[K]) == N and bool((whole[1:] > whole[:-1]).all()) and int((whole[1:] - whole[:-1]).max()) <= p["max"]
        # restart: from the last cut below the window on, the cuts are those of the suffix chunked alone
        j = int(torch.searchsorted(whole, torch.tensor([B - 2 * MIB], device="cuda")).item()) - 1
        cj = int(whole[j])
        assert 0 < B - 2 * MIB - p["max"] <= cj < B - 2 * MIB
        tail, kt = dev_cdc(cw, cp, src.ptr + cj, N - cj, True)
        assert kt == K - j and torch.equal(tail + cj, whole[j:]), ("suffix", kt, K - j)
        # the mirror image: the prefix [0, c_j) with final = 0 gives the head, and stops within max_size of its end
        head, kh = dev_cdc(cw, cp, src.ptr, cj, False)
        assert 0 < kh <= j and torch.equal(head, whole[:kh + 1]) and int(head[kh]) + p["max"] > cj, ("prefix", kh, j)
        cuts = whole[j:].cpu().numpy()
    # the window against the model, from a device cut on
    a = int(cuts[np.searchsorted(cuts, WIN_LO)])
    model = [a + x for x in CM.chunk(src.host(a, WIN_HI), p, final=False)]
    span = cuts[(cuts >= a) & (cuts <= model[-1])]
    assert span.tolist() == model and len(model) > 20, ("window", len(span), len(model))
    m = np.array(model, np.int64)
    P4.assert_reaches(m[:-1], m[1:], "model cuts")


def dev_streams(cw, cp, ptr, n, ends, final=None):
    """cw_dev_cdc_streams (final = None) or cw_dev_cdc_streams_part: (offsets on the device, K, first, verdict)."""
    import torch
    nf = len(ends)
    d_ends = _dev_u64(list(ends) + [0])
    cap = cp.max_offsets_streams(n, nf)
    offs, first, k, result = _poison(cap + PAD), _poison(nf + 1 + PAD), _poison(1 + PAD), _poison(1 + PAD)
    torch.cuda.synchronize()
    if final is None:
        cw.dev_cdc_streams(cp, ptr, n, d_ends.data_ptr(), nf, offs.data_ptr(), cap, k.data_ptr(), first.data_ptr(), result.data_ptr(), _stream())
    else:
        cw.dev_cdc_streams_part(cp, ptr, n, d_ends.data_ptr(), nf, final, offs.data_ptr(), cap, k.data_ptr(), first.data_ptr(), result.data_ptr(),
                                _stream())
    torch.cuda.synchronize()
    kk, P = int(k[0].item()), POISON - (1 << 64)
    assert 0 <= kk < cap
    assert bool((offs[kk + 1:] == P).all()) and bool((first[nf + 1:] == P).all()) and bool((k[1:] == P).all()) and bool((result[1:] == P).all())
    return offs[:kk + 1], kk, _u64(first[:nf + 1]).astype(np.int64), int(result[0].item())


def stream_ends():
    """One long stream [0, E) that ends a little below the window, forty-odd short ones whose ends include 2^32 - 1, 2^32 and 2^32 + 1
    (with empty streams at each of them), and a last one up to N."""
    rng = np.random.default_rng(77)
    E = WIN_LO - 12345
    ends, at = [E], E
    for stop in (B - 1, B, B + 1, WIN_HI - 4321):
        while stop - at > 80000:
            at += int(rng.integers(300, 70000))
            ends.append(at)
        at = stop
        ends += [stop, stop] if stop <= B + 1 else [stop]                     # the second one is an empty stream at that end
    return ends + [N]


@pytest.mark.parametrize("seg", [0, ODD_SEGMENT], ids=["default_segment", "odd_segment"])
@pytest.mark.parametrize("p", [D8, SMALL], ids=["default8192", "small"])
def test_cdc_streams_with_ends_around_2_32(cw, src, p, seg):
    import torch
    cp = cw.CdcParams.default(8192) if p is D8 else _params(cw, p)
    ends = stream_ends()
    nf, E, last = len(ends), ends[0], ends[-2]
    assert {B - 1, B, B + 1} <= set(ends) and sum(1 for a, b in zip(ends[:-1], ends[1:]) if a == b) == 3 and nf >= 40 and ends == sorted(ends)
    with segment(cw, seg):
        offs, K, first, verdict = dev_streams(cw, cp, src.ptr, N, ends)
        long_, k0 = dev_cdc(cw, cp, src.ptr, E, True)
        tail, kt = dev_cdc(cw, cp, src.ptr + last, N - last, True)
        open_tail, ko = dev_cdc(cw, cp, src.ptr + last, N - last, False)
        part1 = dev_streams(cw, cp, src.ptr, N, ends, final=True)
        part0 = dev_streams(cw, cp, src.ptr, N, ends, final=False)
    assert verdict == 0 and first[0] == 0 and first[1] == k0 and torch.equal(offs[:k0 + 1], long_), "the long stream"
    # the short streams by the model, each chunked alone
    short = [src.host(a, b).tobytes() for a, b in zip(ends[:-2], ends[1:-1])]
    m_off, m_first = SM.chunk_streams(short, p)
    k1 = int(first[nf - 1])
    assert (offs[k0:k1 + 1].cpu().numpy() - E).tolist() == m_off and (first[1:nf] - k0).tolist() == m_first, "the short streams"
    assert first[nf] == K and K - k1 == kt and torch.equal(offs[k1:] - last, tail), "the last stream"
    h = offs[k0:k1 + 1].cpu().numpy()
    P4.assert_reaches(h[:-1], h[1:], "stream chunks", over=False)
    assert all(int(e) in set(h.tolist()) for e in (B - 1, B, B + 1))
    # the part call: final = 1 is the streams call; final = 0 leaves the last stream open, cut as cw_dev_cdc(final = 0) cuts it alone
    assert part1[1] == K and torch.equal(part1[0], offs) and part1[2].tolist() == first.tolist() and part1[3] == 0
    o0, K0, f0, v0 = part0
    assert v0 == 0 and K0 == k1 + ko and torch.equal(o0[:k1 + 1], offs[:k1 + 1]) and torch.equal(o0[k1:] - last, open_tail), "the open stream"
    assert f0[:nf].tolist() == first[:nf].tolist() and f0[nf] == K0 and 0 < ko <= kt and int(o0[K0]) + p["max"] > N
    # the open-stream rule against its model (streams_ingest_model.chunk_part), on a piece that the model can walk: 600,000 bytes
    # around 2^32 with ends at 2^32 - 1, 2^32 and 2^32 + 1, the last stream open
    lo, n = B - 300000, 600000
    some = [100000, 299999, 300000, 300000, 300001, 450000, n]
    with segment(cw, seg):
        po, pk, pf, pv = dev_streams(cw, cp, src.ptr + lo, n, some, final=False)
    want = SIM.chunk_part(src.host(lo, lo + n).tobytes(), some, False, p)
    assert pv == 0 and po.cpu().numpy().tolist() == want[0] and pf.tolist() == want[1] and want[0][-1] < n, "the open stream against the model"


# ---- 1c: one fused ingest of the whole source ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alg", ALGS)
def test_fused_ingest_of_the_whole_source(cw, oracle, src, alg):
    """cw_dev_cdc_dedupe_compress + cw_dev_store_chunks with nbytes = N, into a store whose cursor starts 1 MiB below 2^32 (so the one
    append's scan gives positions on both sides of it), then cw_dev_restore_chunks of the whole recipe on the device.  Expected, from
    calls that the tests above pin: the offsets are cw_dev_cdc's, the digests cw_dev_hash_chunks' (the window's against the oracle),
    the refs their first-occurrence numbering, the sizes cw_dev_compress_chunks' over the new chunks (the window's against the
    oracle), the directory and ``*d_used`` the running sum of what each new chunk stores."""
    import torch
    s, cp, base, dir_base, L = _stream(), cw.CdcParams.default(8192), 9, 5, B - MIB
    cap = cp.max_offsets(N)
    total, store_bytes, db = cw.chunk_slots_bytes(alg, N, cap - 1), B + 64 * MIB, 64
    index = cw.DedupeIndex("skein512", 1 << 21)
    try:
        off, k_dev, ref, n_new = _poison(cap + PAD), _poison(1 + PAD), _poison(cap + PAD), _poison(1 + PAD)
        dig = torch.full((cap * db,), 0xEE, dtype=torch.uint8, device="cuda")
        new_idx, sizes = torch.full((cap,), -1, dtype=torch.int32, device="cuda"), torch.full((cap,), -1, dtype=torch.int32, device="cuda")
        slots = torch.full((total,), FILL, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        K = index.dev_cdc_dedupe_compress(cp, alg, src.ptr, N, True, base, off.data_ptr(), cap, k_dev.data_ptr(), dig.data_ptr(), ref.data_ptr(),
                                          new_idx.data_ptr(), n_new.data_ptr(), slots.data_ptr(), total, sizes.data_ptr(), s)
        torch.cuda.synchronize()
        # the offsets are 1b's cuts
        whole, kw = dev_cdc(cw, cp, src.ptr, N, True)
        assert K == kw == int(k_dev[0].item()) and torch.equal(off[:K + 1], whole) and bool((off[K + 1:] == POISON - (1 << 64)).all())
        cuts = whole.cpu().numpy()
        # the digests are cw_dev_hash_chunks' (1a), the window's the oracle's; the refs number their first occurrences
        dig2 = torch.full((K * db,), 0xEE, dtype=torch.uint8, device="cuda")
        cw.dev_hash_chunks("skein512", src.ptr, N, off.data_ptr(), k_dev.data_ptr(), K, dig2.data_ptr(), s)
        torch.cuda.synchronize()
        assert torch.equal(dig[:K * db], dig2) and bool((dig[K * db:] == 0xEE).all())
        del dig2
        h_dig = dig[:K * db].cpu().numpy().reshape(K, db)
        win = np.nonzero((cuts[:-1] >= WIN_LO) & (cuts[1:] <= WIN_HI))[0]
        for i in win[::7].tolist() + [int(np.searchsorted(cuts, B, side="right")) - 1]:
            assert h_dig[i].tobytes() == oracle.skein512(src.host(cuts[i], cuts[i + 1]).tobytes()), ("digest", i)
        _, first_at, inverse = np.unique(h_dig.view(np.dtype((np.void, db))).reshape(-1), return_index=True, return_inverse=True)
        want_ref = (base + first_at[inverse.reshape(-1)]).astype(np.int64)
        assert np.array_equal(ref[:K].cpu().numpy(), want_ref) and bool((ref[K:] == POISON - (1 << 64)).all())
        new = np.sort(first_at)
        nn = int(n_new[0].item())
        assert nn == len(new) and np.array_equal(np.sort(new_idx[:nn].cpu().numpy()), new) and 100 < nn < K // 10     # (the corpus repeats)
        new_order = new_idx[:nn].cpu().numpy().astype(np.int64)
        # the store: a cursor that starts below 2^32
        d_store = torch.zeros(store_bytes, dtype=torch.uint8, device="cuda")
        d_used, d_dir, result = _dev_u64([L]), torch.zeros(2 * cap, dtype=torch.int64, device="cuda"), _poison(2 + PAD)
        torch.cuda.synchronize()
        cw.dev_store_chunks(alg, src.ptr, N, off.data_ptr(), k_dev.data_ptr(), cap - 1, slots.data_ptr(), sizes.data_ptr(), base, d_store.data_ptr(),
                            store_bytes, d_used.data_ptr(), d_dir.data_ptr(), dir_base, cap, result.data_ptr(), s, new_idx.data_ptr(), n_new.data_ptr())
        torch.cuda.synchronize()
        h_sizes = sizes[:nn].cpu().numpy().astype(np.int64)
        # the sizes are cw_dev_compress_chunks' over the same selection (1a), into fresh slots; the window's new chunks the oracle's
        slots.fill_(FILL)
        sizes2 = torch.full((cap,), -1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        cw.dev_compress_chunks(alg, src.ptr, N, off.data_ptr(), k_dev.data_ptr(), cap - 1, slots.data_ptr(), total, sizes2.data_ptr(), s,
                               new_idx.data_ptr(), n_new.data_ptr())
        torch.cuda.synchronize()
        assert torch.equal(sizes, sizes2)
        del slots, sizes2
        fn, scratch = _oracle_fn(oracle, alg), np.zeros(2 * BLOCK + 64, np.uint8)
        in_window = [j for j, i in enumerate(new_order.tolist()) if WIN_LO <= cuts[i] and cuts[i + 1] <= WIN_HI]
        assert len(in_window) > 20
        for j in in_window:
            i = int(new_order[j])
            assert h_sizes[j] == fn(np.ascontiguousarray(src.host(cuts[i], cuts[i + 1])), scratch), ("size", i)
        lens = (cuts[new_order + 1] - cuts[new_order]).astype(np.int64)
        stored = np.where((h_sizes > 0) & (h_sizes < lens), h_sizes, lens)
        pos = L + np.concatenate([[0], np.cumsum(stored)])
        assert result[:2].cpu().numpy().tolist() == [0, int(stored.sum())] and int(d_used[0].item()) == int(pos[-1]) > B
        want_dir = np.zeros(cap, P4.LOC)
        want_dir["pos"][base + new_order - dir_base] = pos[:-1]
        want_dir["stored"][base + new_order - dir_base] = stored
        want_dir["raw"][base + new_order - dir_base] = np.where(stored == lens, lens | 0x80000000, lens)
        got_dir = d_dir.cpu().numpy().view(P4.LOC)
        bad = np.nonzero(got_dir != want_dir)[0]
        assert len(bad) == 0, ("entry", int(bad[0]), got_dir[bad[0]].tolist(), want_dir[bad[0]].tolist(), len(bad))
        P4.assert_reaches(pos[:-1], pos[1:], "stored extents")
        assert not bool(d_store[:L].any()) and not bool(d_store[int(pos[-1]):].any())
        if alg == "lzf":
            assert (stored == lens).any() and (stored < lens).any()
        # the restore of the whole recipe, on the device
        out, status = torch.full((N,), 0x5C, dtype=torch.uint8, device="cuda"), torch.full((K + PAD,), -1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        cw.dev_restore_chunks(alg, d_store.data_ptr(), store_bytes, d_dir.data_ptr(), dir_base, cap, ref.data_ptr(), off.data_ptr(), k_dev.data_ptr(), K,
                              out.data_ptr(), N, status.data_ptr(), s)
        torch.cuda.synchronize()
        assert not bool(status[:K].any()) and bool((status[K:] == -1).all()), status[:K].nonzero()[:4].tolist()
        assert torch.equal(out, src.dev), (out != src.dev).nonzero()[:4].tolist()
        P4.assert_reaches(cuts[:-1], cuts[1:], "restored extents")
    finally:
        index.close()
