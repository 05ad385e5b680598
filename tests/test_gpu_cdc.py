"""Content-defined chunking and per-chunk hashing on the GPU, against tests/cdc_model.py and the CPU oracle."""
import ctypes as C
import hashlib

import numpy as np
import pytest

import cdc_model as CM
from conftest import corpus_file, corpus_large_file, corpus_names

pytestmark = pytest.mark.gpu
CW_ERR_BAD_ARG = -2


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


def dev_cuts(cw, data, p: dict, final=True, shift=0, seg=None):
    """cw_dev_cdc over data placed `shift` bytes into a device buffer."""
    import torch
    a = np.frombuffer(bytes(data), np.uint8) if not isinstance(data, np.ndarray) else data
    n = len(a)
    buf = torch.zeros(n + shift + 16, dtype=torch.uint8, device="cuda")
    if n:
        buf[shift:shift + n] = torch.from_numpy(a.copy()).cuda()
    cp = _params(cw, p)
    cap = cp.max_offsets(n)
    offs = torch.full((cap,), 0xAB, dtype=torch.int64, device="cuda")
    k = torch.zeros(1, dtype=torch.int64, device="cuda")
    if seg:
        cw.tune_set("CW_CDC_SEGMENT", str(seg))
    try:
        cw.dev_cdc(cp, buf.data_ptr() + shift, n, final, offs.data_ptr(), cap, k.data_ptr(), _stream())
        torch.cuda.synchronize()
    finally:
        if seg:
            cw.tune_set("CW_CDC_SEGMENT", None)
    kk = int(k.item())
    return offs[:kk + 1].cpu().numpy().view(np.uint64).tolist()


_MODEL = {}


def model(data, p, final=True):
    """The model's cuts, computed once per input and parameters (the device runs repeat with other segments and shifts)."""
    raw = bytes(data) if not isinstance(data, np.ndarray) else data.tobytes()
    key = (hashlib.sha1(raw).digest(), len(raw), repr(sorted((k, v if k != "gear" else tuple(v or ())) for k, v in p.items())), final)
    if key not in _MODEL:
        _MODEL[key] = CM.chunk(raw, p, final=final)
    return _MODEL[key]


def check(cw, data, p, **kw):
    want = model(data, p, final=kw.get("final", True))
    got = dev_cuts(cw, data, p, **kw)
    assert got == want, (len(got), len(want), next((i for i, (x, y) in enumerate(zip(got, want)) if x != y), None))
    return want


D8 = CM.default_params(8192)
SMALL = CM.params(64, 256, 1024, CM.top_bits(10), CM.top_bits(6))


def test_corpus_files_and_their_concatenation(cw):
    files = [corpus_file(n) for n in corpus_names()] + [corpus_large_file("bible.txt"), corpus_large_file("world192.txt")]
    for f in files:
        check(cw, f, D8)
    cuts = check(cw, b"".join(files), CM.default_params(1024))
    assert len(cuts) > 1000


@pytest.mark.parametrize("p", [CM.default_params(1024), D8, CM.default_params(65536), SMALL], ids=["1k", "8k", "64k", "64-256-1024"])
def test_random_data(cw, p):
    data = np.random.default_rng(11).integers(0, 256, 12 << 20, dtype=np.uint8)
    cuts = check(cw, data, p)
    assert len(cuts) > (12 << 20) // (p["max"]) + 1
    check(cw, data[:(3 << 20) + 5], p, shift=7)


@pytest.mark.parametrize("shift", [1, 3, 5, 8, 13, 15])
def test_odd_source_offsets(cw, shift):
    data = corpus_large_file("world192.txt")[:1 << 20]
    check(cw, data, D8, shift=shift)
    check(cw, data[:5000], SMALL, shift=shift)


def test_edge_sizes(cw):
    rng = np.random.default_rng(5)
    src = rng.integers(0, 256, 1 << 17, dtype=np.uint8).tobytes()
    for p in (SMALL, D8):
        m, a, M = p["min"], p["avg"], p["max"]
        for n in (0, 1, m - 1, m, m + 1, a, M, M + 1, 3 * M + 17):
            for final in (True, False):
                check(cw, src[:n], p, final=final)


def test_fixed_masks_gear_and_equal_sizes(cw):
    text = corpus_large_file("bible.txt")[:1 << 20]
    assert set(np.diff(check(cw, text, CM.params(64, 64, 64, CM.top_bits(10), 0)))[:-1].tolist()) == {64}
    assert set(np.diff(check(cw, text, dict(D8, mask_s=0, mask_l=0)))[:-1].tolist()) == {D8["min"]}
    assert set(np.diff(check(cw, text, dict(D8, mask_s=CM.M64, mask_l=CM.M64)))[:-1].tolist()) == {D8["max"]}
    gear = [CM.splitmix64(v * 7 + 1) for v in range(256)]
    check(cw, text, dict(D8, gear=gear))
    check(cw, text, CM.params(100, 300, 700, 0xF0000000000000F0, 0x3, gear=gear), shift=3)


def _degenerate_inputs():
    rng = np.random.default_rng(9)

    def rnd(n):
        return rng.integers(0, 256, n, dtype=np.uint8).tobytes()

    runs = rnd(777)
    for z in (100, 1500, 9000, 40000, 70000, 300000, 2_000_000):  # shorter than m, between m and M, many times M
        runs += bytes(z) + rnd(int(rng.integers(1000, 30000)))
    return {"zeros": bytes(3 << 19), "byte": b"\x5a" * (3 << 19) + rnd(100), "ab": rnd(3) + b"ab" * (3 << 18),
            "abc": rnd(1) + b"abc" * (1 << 19), "runs": runs}


@pytest.mark.parametrize("seg", [None, 4096, 70001])
def test_degenerate_runs_across_segments(cw, seg):
    for name, data in _degenerate_inputs().items():
        for p in (SMALL, D8):
            if seg and seg < p["max"]:
                continue
            check(cw, data, p, seg=seg)
            check(cw, data, p, seg=seg, shift=5)
        check(cw, data, dict(D8, mask_s=0, mask_l=0), seg=seg)


def test_64mib_of_zeros_behind_an_odd_prefix(cw):
    data = np.zeros((64 << 20) + 12345, np.uint8)
    data[:12345] = np.random.default_rng(1).integers(0, 256, 12345, dtype=np.uint8)
    cuts = dev_cuts(cw, data, D8)
    head = CM.chunk(data[:200000], D8)
    want_first = [c for c in head if c < 100000]
    assert cuts[:len(want_first)] == want_first
    # after the prefix every chunk in the zero run is max-sized until the end
    tail = np.diff(cuts[len(want_first) + 2:])
    assert set(tail[:-1].tolist()) == {D8["max"]}
    assert cuts[-1] == len(data)
    for seg in (None, 65536 * 3):
        assert dev_cuts(cw, data[:24 << 20], D8, seg=seg, shift=1) == model(data[:24 << 20], D8)


def test_streaming_pieces_equal_one_call(cw):
    rng = np.random.default_rng(2)
    data = corpus_large_file("bible.txt")[:(1 << 20)] + rng.integers(0, 256, 1 << 20, dtype=np.uint8).tobytes() + bytes(300000)
    for p in (SMALL, D8):
        whole = dev_cuts(cw, data, p)
        assert whole == model(data, p)
        cuts, done, pos = [0], 0, 0
        while True:
            pos = min(len(data), pos + int(rng.integers(p["max"] // 2, 400000)))
            fin = pos == len(data)
            part = dev_cuts(cw, data[done:pos], p, final=fin)
            cuts += [done + x for x in part[1:]]
            done += part[-1]
            if fin:
                break
        assert cuts == whole


def test_max_offsets_too_small_launches_nothing(cw):
    import torch
    p = cw.CdcParams.default(1024)
    n = 1 << 20
    buf = torch.zeros(n, dtype=torch.uint8, device="cuda")
    offs = torch.full((n // 256 + 2,), 7, dtype=torch.int64, device="cuda")
    k = torch.full((1,), 7, dtype=torch.int64, device="cuda")
    rc = cw.lib().cw_dev_cdc(C.byref(p), buf.data_ptr(), n, 1, offs.data_ptr(), n // 256 + 1, k.data_ptr(), _stream())
    torch.cuda.synchronize()
    assert rc == CW_ERR_BAD_ARG
    assert int(k.item()) == 7 and bool((offs == 7).all())


# ---- cw_dev_hash_chunks ------------------------------------------------------------------------------------------------
def _oracle(alg):
    import oracle as O
    return {"skein512": lambda b: O.skein512(b, 512), "skein": lambda b: O.skein256(b, 128),
            "sha256mb": lambda b: hashlib.sha256(b).digest()}[alg]


def dev_hash_chunks(cw, alg, src: np.ndarray, offsets, count=None, max_chunks=None, shift=0):
    import torch
    db = cw.digest_bytes(alg)
    buf = torch.zeros(len(src) + shift + 16, dtype=torch.uint8, device="cuda")
    buf[shift:shift + len(src)] = torch.from_numpy(src.copy()).cuda()
    o = torch.from_numpy(np.asarray(offsets, np.uint64).view(np.int64).copy()).cuda()
    nk = len(offsets) - 1 if count is None else count
    k = torch.tensor([nk], dtype=torch.int64, device="cuda")
    mc = len(offsets) - 1 if max_chunks is None else max_chunks
    dig = torch.full((max(len(offsets) - 1, 1) * db,), 0xEE, dtype=torch.uint8, device="cuda")
    cw.dev_hash_chunks(alg, buf.data_ptr() + shift, len(src), o.data_ptr(), k.data_ptr(), mc, dig.data_ptr(), _stream())
    torch.cuda.synchronize()
    return dig.cpu().numpy().reshape(-1, db)


ALGS = ["skein512", "skein", "sha256mb"]


@pytest.mark.parametrize("alg", ALGS)
def test_hash_chunks_arbitrary_offsets(cw, alg):
    rng = np.random.default_rng(4)
    lens = list(range(0, 301)) + [64 * k + d for k in (1, 2, 3, 16, 100) for d in (-1, 0, 1)] + [1 << 20, 777777, 65536, 65537]
    rng.shuffle(lens)
    offs = [int(rng.integers(0, 16))]
    for L in lens:
        offs.append(offs[-1] + L)
    src = rng.integers(0, 256, offs[-1] + 64, dtype=np.uint8)
    H = _oracle(alg)
    for shift in (0, 3):
        dig = dev_hash_chunks(cw, alg, src, offs, shift=shift)
        for i in range(len(offs) - 1):
            assert dig[i].tobytes() == H(src[offs[i]:offs[i + 1]].tobytes()), (i, offs[i + 1] - offs[i])
    # starts at every residue mod 16
    offs = [s * 1000 + s for s in range(17)]
    dig = dev_hash_chunks(cw, alg, src, offs)
    for i in range(16):
        assert dig[i].tobytes() == H(src[offs[i]:offs[i + 1]].tobytes())


@pytest.mark.parametrize("alg", ALGS)
def test_hash_chunks_of_cdc_chunks_and_of_blocks(cw, alg):
    import torch
    data = np.frombuffer(corpus_large_file("bible.txt"), np.uint8)
    cuts = CM.chunk(data, D8)
    dig = dev_hash_chunks(cw, alg, data, cuts)
    H = _oracle(alg)
    for i in list(range(0, len(cuts) - 1, 17)) + [len(cuts) - 2]:
        assert dig[i].tobytes() == H(data[cuts[i]:cuts[i + 1]].tobytes())
    # offsets at multiples of a block size: exactly cw_dev_hash's digests
    bs, nb = 4096, 300
    blocks = data[:bs * nb]
    want = torch.zeros(nb * cw.digest_bytes(alg), dtype=torch.uint8, device="cuda")
    src = torch.from_numpy(blocks.copy()).cuda()
    cw.dev_hash(alg, src.data_ptr(), bs, nb, want.data_ptr(), _stream())
    torch.cuda.synchronize()
    got = dev_hash_chunks(cw, alg, blocks, [i * bs for i in range(nb + 1)])
    assert got.tobytes() == want.cpu().numpy().tobytes()


@pytest.mark.parametrize("alg", ALGS)
def test_hash_chunks_clamps_and_respects_the_count(cw, alg):
    src = np.random.default_rng(8).integers(0, 256, 10000, dtype=np.uint8)
    H = _oracle(alg)
    offs = [0, 500, 300, 9000, 12000, 1 << 40, 20, 10000, 10000]
    dig = dev_hash_chunks(cw, alg, src, offs)
    clamp = [min(x, 10000) for x in offs]
    for i in range(len(offs) - 1):
        a, b = clamp[i], clamp[i + 1]
        assert dig[i].tobytes() == H(src[a:b].tobytes() if b > a else b""), i
    dig = dev_hash_chunks(cw, alg, src, [0, 100, 200, 300, 400, 500], count=3)
    assert all(dig[i].tobytes() == H(src[100 * i:100 * i + 100].tobytes()) for i in range(3))
    assert (dig[3:] == 0xEE).all()
    dig = dev_hash_chunks(cw, alg, src, [0, 100, 200, 300, 400, 500], count=5, max_chunks=2)
    assert (dig[2:] == 0xEE).all()


def test_bible_edits_dedupe_end_to_end(cw):
    import torch
    a = corpus_large_file("bible.txt")
    b = bytearray(a)
    for pos in (1, 500_000, 1_700_000, 3_000_000):
        b[pos:pos] = b"INSERTED"
    del b[2_500_000:2_500_100]
    b = bytes(b)
    p = cw.CdcParams.default(1024)
    idx = cw.DedupeIndex("skein512", 1 << 16)
    shared = {}
    for name, data in (("a", a), ("b", b)):
        offs, dig = cw.cdc_hash(p, data, "skein512")
        k = len(offs) - 1
        d = torch.from_numpy(dig.copy()).cuda()
        ref = torch.zeros(k, dtype=torch.int64, device="cuda")
        new_idx = torch.zeros(k, dtype=torch.int32, device="cuda")
        n_new = torch.zeros(1, dtype=torch.int64, device="cuda")
        idx.dev_dedupe(d.data_ptr(), k, 0 if name == "a" else 1 << 32, ref.data_ptr(), new_idx.data_ptr(), n_new.data_ptr(), _stream())
        torch.cuda.synchronize()
        if name == "b":
            old = ref.cpu().numpy() < (1 << 32)
            lens = np.diff(offs.astype(np.int64))
            shared = lens[old].sum() / len(b)
    assert shared >= 0.99, shared
    fb = 4096
    fa = {hashlib.sha256(a[i:i + fb]).digest() for i in range(0, len(a) - fb + 1, fb)}
    assert sum(hashlib.sha256(b[i:i + fb]).digest() in fa for i in range(0, len(b) - fb + 1, fb)) == 0


def test_host_form_over_pieces_equals_device_and_model(cw):
    import torch
    p = cw.CdcParams.default(8192)
    rng = np.random.default_rng(6)
    small = np.concatenate([rng.integers(0, 256, 20 << 20, dtype=np.uint8), np.zeros(4 << 20, np.uint8)])
    offs, dig = cw.cdc_hash(p, small, "sha256mb")
    assert offs.tolist() == CM.chunk(small, D8)
    for i in range(0, len(offs) - 1, 97):
        assert dig[i].tobytes() == hashlib.sha256(small[offs[i]:offs[i + 1]].tobytes()).digest()
    # ~600 MiB: three pieces on the host path against one device call
    n = 600 << 20
    src = torch.empty(n, dtype=torch.uint8, device="cuda")
    cw.dev_gen_random(0x5EED, 0, n // 65536, 65536, src.data_ptr(), _stream())
    src[100 << 20:140 << 20] = 0
    host = src.cpu().numpy()
    offs_h, dig_h = cw.cdc_hash(p, host, "skein")
    cap = p.max_offsets(n)
    o = torch.zeros(cap, dtype=torch.int64, device="cuda")
    k = torch.zeros(1, dtype=torch.int64, device="cuda")
    cw.dev_cdc(p, src.data_ptr(), n, True, o.data_ptr(), cap, k.data_ptr(), _stream())
    dig = torch.zeros(cap * 16, dtype=torch.uint8, device="cuda")
    cw.dev_hash_chunks("skein", src.data_ptr(), n, o.data_ptr(), k.data_ptr(), cap, dig.data_ptr(), _stream())
    torch.cuda.synchronize()
    kk = int(k.item())
    assert offs_h.tolist() == o[:kk + 1].cpu().numpy().view(np.uint64).tolist()
    assert dig_h.tobytes() == dig[:kk * 16].cpu().numpy().tobytes()


@pytest.mark.parametrize("p", [SMALL, D8], ids=["64-256-1024", "8k"])
def test_runs_entered_at_an_odd_phase_cross_many_segments(cw, p):
    """The true chain enters a long run out of phase with every segment's own chain: one progression across the segments."""
    rng = np.random.default_rng(21)
    prefix = rng.integers(0, 256, 3001, dtype=np.uint8).tobytes()
    for body in (bytes(6 << 20), b"ab" * (3 << 20)):
        data = prefix + body + prefix
        for seg in (None, p["max"] * 3 + 1):
            check(cw, data, p, seg=seg)
