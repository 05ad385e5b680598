"""GPU parity tests proper: the HIP path (through the C ABI) against the CPU oracle and the committed
golden fixtures.  Bit-exact everywhere (integer / byte work)."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import (ROOT, anchor_input, corpus_file, corpus_large_file, corpus_large_names, corpus_names, load_golden,
                      seeded_block)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cw():
    import compute_war_amd as cw
    cw.init(0)  # raises without a gfx950 device or without the built library: no fallback
    return cw


HASHES = [("skein512", 64), ("skein", 16), ("sha256mb", 32)]


def _oracle_hash(oracle, alg, b):
    if alg == "skein512":
        return oracle.skein512(b, 512)
    if alg == "skein":
        return oracle.skein256(b, 128)
    return oracle.sha256(b)


# ---------------------------------------------------------------- hashes
def test_skein_golden_reference_blocks(cw):
    """Digests produced by the reference's own C (oracle/_ref at fixture-generation time)."""
    g = load_golden("skein_ref_blocks.json")
    for rec in g["blocks"]:
        d = seeded_block(rec["seed"], rec["n"], rec["kind"])
        n = rec["n"]
        if n == 0:
            continue
        assert cw.hash_blocks("skein512", d, n)[0].tobytes().hex() == rec["skein512_512"], rec
        assert cw.hash_blocks("skein", d, n)[0].tobytes().hex() == rec["skein256_128"], rec


def test_survey_anchor_digests(cw):
    for a in load_golden("survey_anchors.json")["anchors"]:
        d = anchor_input(a["input"], a["n"])
        assert cw.hash_blocks("skein512", d, a["n"])[0].tobytes().hex().startswith(a["skein512_prefix"])
        assert cw.hash_blocks("skein", d, a["n"])[0].tobytes().hex() == a["skein256_128"]


@pytest.mark.parametrize("alg,db", HASHES)
@pytest.mark.parametrize("bs,count", [(4096, 200), (65536, 70), (64, 130), (32, 65), (128, 3)])
def test_hash_matches_oracle_regular(cw, oracle, alg, db, bs, count):
    data = np.random.default_rng(bs + count).integers(0, 256, bs * count, dtype=np.uint8)
    got = cw.hash_blocks(alg, data, bs)
    assert got.shape == (count, db)
    for i in range(count):
        assert got[i].tobytes() == _oracle_hash(oracle, alg, data[i * bs:(i + 1) * bs].tobytes()), (alg, bs, i)


@pytest.mark.parametrize("alg,db", HASHES)
def test_hash_ragged_and_unaligned_sizes(cw, oracle, alg, db):
    """Block sizes that are not multiples of the hash's internal block (tail/padding paths) and
    strides that break 16-byte alignment."""
    for bs in (1, 2, 7, 31, 33, 55, 56, 57, 63, 65, 100, 119, 120, 127, 129, 1000, 4095, 4097, 12345):
        count = 67
        data = np.random.default_rng(bs).integers(0, 256, bs * count, dtype=np.uint8)
        got = cw.hash_blocks(alg, data, bs)
        for i in (0, 1, 33, 63, 64, 66):
            assert got[i].tobytes() == _oracle_hash(oracle, alg, data[i * bs:(i + 1) * bs].tobytes()), (alg, bs, i)


def test_hash_empty_message(cw, oracle):
    # block_bytes == 0 hashes the empty message per block through the device API
    import torch
    dig = torch.zeros(3 * 64, dtype=torch.uint8, device="cuda")
    src = torch.zeros(16, dtype=torch.uint8, device="cuda")
    cw.dev_hash("skein512", src.data_ptr(), 0, 3, dig.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert dig.cpu().numpy()[:64].tobytes() == oracle.skein512(b"", 512)
    assert dig.cpu().numpy()[128:192].tobytes() == oracle.skein512(b"", 512)
    # every algorithm, many blocks, stride 0 / 7, misaligned base, a source allocation with nothing behind the pointer:
    # SHA-256's whole-chunk path once read 64 bytes at (and before) the pointer for an empty message (found by tests/soak_hash.py)
    want = {"skein512": oracle.skein512(b"", 512), "skein": oracle.skein256(b"", 128), "sha256mb": hashlib.sha256(b"").digest()}
    s = torch.cuda.current_stream().cuda_stream
    for alg, w in want.items():
        for stride, shift, count in ((0, 0, 263), (7, 1, 70), (16, 0, 5), (0, 3, 1)):
            src = torch.zeros(stride * count + shift + 1, dtype=torch.uint8, device="cuda")
            dig = torch.zeros(count * len(w), dtype=torch.uint8, device="cuda")
            cw.dev_hash(alg, src.data_ptr() + shift, 0, count, dig.data_ptr(), s, src_stride=stride)
            torch.cuda.synchronize()
            got = dig.cpu().numpy().reshape(count, len(w))
            assert all(got[i].tobytes() == w for i in range(count)), (alg, stride, shift)


def test_slots_do_hashing(cw, oracle):
    """doHashing(src, dst, count) with the global block size, as the driver calls it (:257)."""
    data = np.frombuffer(corpus_file("alice29.txt")[:8 * 4096], dtype=np.uint8)
    out = cw.do_hashing("skein", data, 8, block_bytes=4096)
    for i in range(8):
        assert out[16 * i:16 * i + 16] == oracle.skein256(data[4096 * i:4096 * (i + 1)].tobytes(), 128)
    out = cw.do_hashing("sha256mb", data, 8, block_bytes=4096)
    for i in range(8):
        assert out[32 * i:32 * i + 32] == hashlib.sha256(data[4096 * i:4096 * (i + 1)].tobytes()).digest()


# ---------------------------------------------------------------- LZ4
def _check_lz4(cw, oracle, data: bytes, bs: int):
    sizes, payload = cw.compress_blocks("lz4", data, bs)
    n = len(data) // bs
    for i in range(n):
        want = oracle.lz4_compress(data[i * bs:(i + 1) * bs])
        got = payload[i, :sizes[i]].tobytes()
        assert sizes[i] == len(want) and got == want, (bs, i, int(sizes[i]), len(want))
    return sizes


@pytest.mark.parametrize("bs", [4096, 65536])
def test_lz4_canterbury_bit_exact(cw, oracle, bs):
    tin = tout = 0
    for name in corpus_names():
        data = corpus_file(name)
        whole = len(data) // 65536 * 65536
        if not whole:
            continue
        sizes = _check_lz4(cw, oracle, data[:whole], bs)
        tin += whole
        tout += int(sizes.sum())
    want = next(r for r in load_golden("survey_anchors.json")["corpus_ratios"]
                if r["corpus"] == "canterbury" and r["block"] == bs)
    assert round(tin / tout, 4) == want["lz4"]


def test_lz4_survey_anchors(cw):
    for a in load_golden("survey_anchors.json")["anchors"]:
        d = anchor_input(a["input"], a["n"])
        sizes, payload = cw.compress_blocks("lz4", d, a["n"])
        assert sizes[0] == a["lz4"]
        if "lz4_sha256" in a:
            assert hashlib.sha256(payload[0, :sizes[0]].tobytes()).hexdigest() == a["lz4_sha256"]


def test_lz4_edge_cases(cw, oracle):
    rng = np.random.default_rng(5)
    for n in (1, 2, 4, 5, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 31, 32, 33, 63, 64, 65, 255, 256, 270, 271, 272, 273,
              300, 1000, 4095, 4097, 65535, 65536):
        for alphabet in (1, 2, 3, 16, 256):
            count = 5 if n > 4096 else 66
            data = rng.integers(0, alphabet, n * count, dtype=np.uint8).tobytes()
            _check_lz4(cw, oracle, data, n)
    for period in (1, 2, 3, 4, 7, 8, 255, 256, 263, 264, 265, 8191, 8192, 8193):
        base = rng.integers(0, 256, period, dtype=np.uint8).tobytes()
        for n in (4096, 65536):
            _check_lz4(cw, oracle, (base * (70000 // period + 1))[:n], n)


def test_lz4_random_blocks_and_generator(cw, oracle):
    """Device generator == oracle generator; random 64 KiB blocks are stored raw (65,794 B)."""
    import torch
    nb, bs = 6, 65536
    buf = torch.empty(nb * bs, dtype=torch.uint8, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    cw.dev_gen_random(0xC0FFEE, 1000, nb, bs, buf.data_ptr(), s)
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert np.array_equal(host, oracle.gen_random_blocks(0xC0FFEE, 1000, nb, bs))
    sizes = _check_lz4(cw, oracle, host.tobytes(), bs)
    assert all(int(x) == 65794 for x in sizes)


def test_slot_do_compression_lz4(cw, oracle):
    b = corpus_file("alice29.txt")[:4096]
    assert cw.do_compression("lz4", b) == oracle.lz4_compress(b)


# ---------------------------------------------------------------- LZF
def _check_lzf(cw, oracle, data: bytes, bs: int):
    sizes, payload = cw.compress_blocks("lzf", data, bs)
    for i in range(len(data) // bs):
        want = oracle.lzf_compress(data[i * bs:(i + 1) * bs])   # b"" = did not fit l-1 (returns 0)
        got = payload[i, :sizes[i]].tobytes()
        assert sizes[i] == len(want) and got == want, (bs, i, int(sizes[i]), len(want))
    return sizes


@pytest.mark.parametrize("bs", [4096, 65536])
def test_lzf_canterbury_bit_exact(cw, oracle, bs):
    tin = tout = 0
    for name in corpus_names():
        data = corpus_file(name)
        whole = len(data) // 65536 * 65536
        if not whole:
            continue
        sizes = _check_lzf(cw, oracle, data[:whole], bs)
        tin += whole
        tout += int(np.where(sizes == 0, bs, sizes).sum())
    want = next(r for r in load_golden("survey_anchors.json")["corpus_ratios"]
                if r["corpus"] == "canterbury" and r["block"] == bs)
    assert round(tin / tout, 4) == want["lzf"]


def test_lzf_survey_anchors(cw):
    for a in load_golden("survey_anchors.json")["anchors"]:
        d = anchor_input(a["input"], a["n"])
        sizes, payload = cw.compress_blocks("lzf", d, a["n"])
        assert sizes[0] == a["lzf"]
        if "lzf_sha256" in a:
            assert hashlib.sha256(payload[0, :sizes[0]].tobytes()).hexdigest() == a["lzf_sha256"]


def test_lzf_edge_cases(cw, oracle):
    rng = np.random.default_rng(6)
    for n in (1, 2, 3, 4, 5, 16, 17, 18, 19, 20, 21, 22, 31, 32, 33, 34, 35, 63, 64, 65, 66, 67, 255, 263, 264, 265, 266,
              267, 268, 300, 1000, 4095, 4097, 16384, 16385, 65535, 65536):
        for alphabet in (1, 2, 3, 16, 256):
            count = 3 if n > 4096 else 40
            data = rng.integers(0, alphabet, n * count, dtype=np.uint8).tobytes()
            _check_lzf(cw, oracle, data, n)
    for period in (1, 2, 3, 4, 7, 8, 255, 256, 263, 264, 265, 8191, 8192, 8193):
        base = rng.integers(0, 256, period, dtype=np.uint8).tobytes()
        for n in (4096, 65536):
            _check_lzf(cw, oracle, (base * (70000 // period + 1))[:n], n)


def test_lzf_random_blocks_do_not_fit(cw, oracle):
    data = oracle.gen_random_blocks(0xC0FFEE, 77, 4, 65536).tobytes()
    sizes = _check_lzf(cw, oracle, data, 65536)
    assert all(int(x) == 0 for x in sizes)    # lzf_compress(.., l-1) returns 0 on incompressible data
    assert cw.do_compression("lzf", data[:4096]) == b""
    b = corpus_file("alice29.txt")[:4096]
    assert cw.do_compression("lzf", b) == oracle.lzf_compress(b)


def test_sha256_lzf_pipeline(cw, oracle):
    """The reference's hc_shlzf configuration (run_tests:20): sha256mb + lzf, read-blocks 8, 4 KiB blocks."""
    data = corpus_file("lcet10.txt")[:64 * 4096]
    dig, sizes, payload = cw.hash_and_compress_blocks("sha256mb", "lzf", data, 4096)
    for i in range(64):
        b = data[i * 4096:(i + 1) * 4096]
        assert dig[i].tobytes() == hashlib.sha256(b).digest()
        want = oracle.lzf_compress(b)
        assert sizes[i] == len(want) and payload[i, :sizes[i]].tobytes() == want


def _large_corpus_blocks(bs):
    data = b"".join(d[:len(d) // 65536 * 65536] for d in (corpus_large_file(n) for n in corpus_large_names()))
    return data, len(data) // bs


@pytest.mark.parametrize("bs", [4096, 65536])
def test_config3_sha256_lzf_over_canterbury_large(cw, oracle, bs):
    """BASELINE.json configs[3]: SHA-256 + LZF (hc_shlzf) over dataset/canterbury-large; every block bit-exact, corpus
    ratio = the reference's."""
    data, nb = _large_corpus_blocks(bs)
    dig, sizes, payload = cw.hash_and_compress_blocks("sha256mb", "lzf", data, bs)
    for i in range(nb):
        b = data[i * bs:(i + 1) * bs]
        assert dig[i].tobytes() == hashlib.sha256(b).digest()
        want = oracle.lzf_compress(b)
        assert sizes[i] == len(want) and payload[i, :sizes[i]].tobytes() == want, (bs, i)
    want = next(r for r in load_golden("survey_anchors.json")["corpus_ratios"]
                if r["corpus"] == "canterbury-large" and r["block"] == bs)
    assert round(len(data) / int(np.where(sizes == 0, bs, sizes).sum()), 4) == want["lzf"]


@pytest.mark.parametrize("bs", [4096, 65536])
def test_config2_skein512_lz4_over_corpus_chunks(cw, oracle, bs):
    """BASELINE.json configs[2] (fused Skein-512 + LZ4 over a corpus chunked at 64 KiB).  Silesia is not in the
    reference tree, so the in-tree large corpus stands in; 4 KiB is the reference driver's own block size."""
    data, nb = _large_corpus_blocks(bs)
    dig, sizes, payload = cw.hash_and_compress_blocks("skein512", "lz4", data, bs)
    for i in range(nb):
        b = data[i * bs:(i + 1) * bs]
        assert dig[i].tobytes() == oracle.skein512(b, 512)
        want = oracle.lz4_compress(b)
        assert sizes[i] == len(want) and payload[i, :sizes[i]].tobytes() == want, (bs, i)
    want = next(r for r in load_golden("survey_anchors.json")["corpus_ratios"]
                if r["corpus"] == "canterbury-large" and r["block"] == bs)
    assert round(len(data) / int(sizes.sum()), 4) == want["lz4"]


# ---------------------------------------------------------------- device API, fused, offload
def test_dev_hash_and_compress_matches_oracle(cw, oracle):
    import torch
    bs = 65536
    data = corpus_file("kennedy.xls") + corpus_file("ptt5")
    nb = len(data) // bs
    data = data[:bs * nb]
    src = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    stride = (cw.compress_bound("lz4", bs) + 15) // 16 * 16
    dig = torch.zeros(nb * 64, dtype=torch.uint8, device="cuda")
    dst = torch.zeros(nb * stride, dtype=torch.uint8, device="cuda")
    sizes = torch.zeros(nb, dtype=torch.int32, device="cuda")
    totals = torch.zeros(2, dtype=torch.int64, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    cw.dev_hash_and_compress("skein512", "lz4", src.data_ptr(), bs, nb, dig.data_ptr(), dst.data_ptr(), stride,
                             sizes.data_ptr(), s)
    cw.dev_sum_sizes(sizes.data_ptr(), nb, bs, totals.data_ptr(), s)
    torch.cuda.synchronize()
    dig, dst, sizes = dig.cpu().numpy(), dst.cpu().numpy(), sizes.cpu().numpy()
    tot = 0
    for i in range(nb):
        b = data[i * bs:(i + 1) * bs]
        assert dig[64 * i:64 * i + 64].tobytes() == oracle.skein512(b, 512)
        want = oracle.lz4_compress(b)
        assert sizes[i] == len(want) and dst[i * stride:i * stride + len(want)].tobytes() == want
        tot += len(want)
    assert int(totals[0]) == tot and int(totals[1]) == 0


def test_dev_api_strides_and_misalignment(cw, oracle):
    """Device entry points with src_stride > block_bytes, a source that is not 16-byte aligned and an odd dst_stride:
    the generic (byte-granular) kernels must give the same bytes as the aligned fast paths."""
    import torch
    s = torch.cuda.current_stream().cuda_stream
    text = corpus_file("fields.c") + corpus_file("cp.html")
    for bs, nb, sstride, shift in ((4096, 9, 4096 + 5, 3), (1000, 70, 1000, 1), (65536, 3, 65536 + 16, 0), (64, 130, 67, 7)):
        raw = np.frombuffer((text * (sstride * nb // len(text) + 2))[:sstride * nb + shift], dtype=np.uint8).copy()
        raw[::7] ^= np.arange(len(raw[::7]), dtype=np.uint8)       # make blocks differ
        dev = torch.from_numpy(raw).cuda()
        base = dev.data_ptr() + shift
        blocks = [raw[shift + i * sstride: shift + i * sstride + bs].tobytes() for i in range(nb)]
        for alg, db in HASHES:
            dig = torch.zeros(nb * db + 16, dtype=torch.uint8, device="cuda")
            cw.dev_hash(alg, base, bs, nb, dig.data_ptr(), s, src_stride=sstride)
            torch.cuda.synchronize()
            hd = dig.cpu().numpy()
            for i in range(nb):
                assert hd[i * db:(i + 1) * db].tobytes() == _oracle_hash(oracle, alg, blocks[i]), (alg, bs, i)
        for comp, ref in (("lz4", oracle.lz4_compress), ("lzf", oracle.lzf_compress)):
            dstride = cw.compress_bound(comp, bs) + 3
            dst = torch.zeros(nb * dstride + 64, dtype=torch.uint8, device="cuda")
            sizes = torch.zeros(nb, dtype=torch.int32, device="cuda")
            cw.dev_compress(comp, base, bs, nb, dst.data_ptr() + 1, dstride, sizes.data_ptr(), s, src_stride=sstride)
            torch.cuda.synchronize()
            hz, hdst = sizes.cpu().numpy(), dst.cpu().numpy()
            for i in range(nb):
                want = ref(blocks[i])
                assert hz[i] == len(want) and hdst[1 + i * dstride: 1 + i * dstride + len(want)].tobytes() == want, (comp, bs, i)


def test_bad_arguments_are_errors(cw):
    import torch
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    with pytest.raises(cw.CwError):
        cw.dev_hash(9, buf.data_ptr(), 4096, 4, buf.data_ptr(), 0)              # unknown algorithm
    with pytest.raises(cw.CwError):
        cw.dev_hash("skein", buf.data_ptr(), 70000, 1, buf.data_ptr(), 0)        # block too large
    with pytest.raises(cw.CwError):
        cw.dev_compress("lz4", buf.data_ptr(), 4096, 4, buf.data_ptr(), 100, buf.data_ptr(), 0)   # dst_stride < bound
    with pytest.raises(cw.CwError):
        cw.dev_hash("skein", 0, 4096, 4, buf.data_ptr(), 0)                      # NULL source
    cw.dev_hash("skein", buf.data_ptr(), 4096, 0, buf.data_ptr(), 0)             # zero blocks: no-op


def test_hash_offload_lifecycle(cw, oracle):
    """HashOffload state machine (HashOffload.h:13-64) and the offload thread (:160-183)."""
    bs, nb = 4096, 32
    data = np.random.default_rng(3).integers(0, 256, bs * nb, dtype=np.uint8)
    res = np.zeros(nb * 16, dtype=np.uint8)
    fired = []
    h = cw.HashOffload(nb, "skein", bs)
    h.Reset(data, res, lambda: fired.append(1))
    assert h.state == h.hInit and not h.Completed()
    with pytest.raises(cw.CwError):
        h.Start()            # assert(state == hQueued)
    h.Enqueue()
    with pytest.raises(cw.CwError):
        h.Enqueue()          # assert(state == hInit)
    h.DoOffload()
    assert h.Completed() and fired == [1]
    for i in range(nb):
        assert res[16 * i:16 * i + 16].tobytes() == oracle.skein256(data[bs * i:bs * (i + 1)].tobytes(), 128)
    # through the consumer thread
    res2 = np.zeros_like(res)
    import threading
    ev = threading.Event()
    h.Reset(data, res2, ev.set)
    assert cw.lib().cw_offload_thread_start() == 0
    h.Submit()
    assert ev.wait(30)
    cw.lib().cw_offload_thread_stop()
    assert np.array_equal(res, res2) and h.Completed()
    h.close()


def test_many_host_threads_call_slots_concurrently(cw, oracle):
    """The reference calls the slots from --c-threads workers with no locking (:398-402)."""
    import threading
    data = np.frombuffer(corpus_file("lcet10.txt")[:64 * 4096], dtype=np.uint8)
    cw.set_block_size(4096)
    errs = []

    def work(t):
        try:
            for i in range(t, 64, 8):
                b = data[4096 * i:4096 * (i + 1)]
                assert cw.do_hashing("skein", b, 1) == oracle.skein256(b.tobytes(), 128)
                assert cw.do_compression("lz4", b) == oracle.lz4_compress(b.tobytes())
        except Exception as e:  # noqa: BLE001
            errs.append(e)

    ts = [threading.Thread(target=work, args=(t,)) for t in range(8)]
    [t.start() for t in ts]
    [t.join() for t in ts]
    assert not errs, errs


def test_full_size_properties(cw, oracle):
    """BASELINE-size properties that need no full-size oracle run: 16 Ki x 64 KiB random blocks (1 GiB):
    every LZ4 size is 65,794, digests of sampled blocks match the oracle, and re-hashing a permuted
    copy permutes the digests (blocks are independent)."""
    import torch
    nb, bs = 16384, 65536
    s = torch.cuda.current_stream().cuda_stream
    src = torch.empty(nb * bs, dtype=torch.uint8, device="cuda")
    cw.dev_gen_random(0xC0FFEE, 0, nb, bs, src.data_ptr(), s)
    dig = torch.zeros((nb, 64), dtype=torch.uint8, device="cuda")
    stride = (cw.compress_bound("lz4", bs) + 15) // 16 * 16
    dst = torch.empty(nb * stride, dtype=torch.uint8, device="cuda")
    sizes = torch.zeros(nb, dtype=torch.int32, device="cuda")
    cw.dev_hash_and_compress("skein512", "lz4", src.data_ptr(), bs, nb, dig.data_ptr(), dst.data_ptr(), stride,
                             sizes.data_ptr(), s)
    torch.cuda.synchronize()
    # almost every random block is stored raw (65,794 B); about 1 in 1000 holds a chance 4-byte repeat among
    # its ~2.9 k probes and gets a real match -- those blocks are checked against the oracle byte for byte
    hz = sizes.cpu().numpy()
    odd = np.nonzero(hz != 65794)[0]
    assert len(odd) < nb // 100
    for i in odd[:64]:
        blk = oracle.gen_random_blocks(0xC0FFEE, int(i), 1, bs)
        want = oracle.lz4_compress(blk)
        assert hz[i] == len(want) and dst[i * stride:i * stride + len(want)].cpu().numpy().tobytes() == want, int(i)
    raw = [int(i) for i in (0, 1, 63, 64, 4097, nb - 1) if hz[i] == 65794]
    hd = dig.cpu().numpy()
    for i in (0, 1, 63, 64, 4097, nb - 1):
        assert hd[i].tobytes() == oracle.skein512(oracle.gen_random_blocks(0xC0FFEE, i, 1, bs), 512)
    for i in raw:
        blk = oracle.gen_random_blocks(0xC0FFEE, i, 1, bs)
        assert hd[i].tobytes() == oracle.skein512(blk, 512)
        out = dst[i * stride:i * stride + 65794].cpu().numpy()
        assert out[0] == 0xF0 and np.array_equal(out[258:], blk)
    # independence: hashing blocks [nb/2, nb) alone gives the same digests
    dig2 = torch.zeros((nb // 2, 64), dtype=torch.uint8, device="cuda")
    cw.dev_hash("skein512", src.data_ptr() + (nb // 2) * bs, bs, nb // 2, dig2.data_ptr(), s)
    torch.cuda.synchronize()
    assert torch.equal(dig2, dig[nb // 2:])


def test_lane_order_fallback_path_is_exact():
    """The exchange-based LZ4/LZF parsers hand a block to the write/read-back parsers when their lane-order check
    fails.  That never happens on this hardware, so the hand-over is forced (CW_LZ_FORCE_REDO=1, read once per
    process -> subprocess) and the result compared with the normal path's, which the tests above pin to the oracle."""
    import subprocess
    import sys
    from conftest import ROOT
    prog = (
        "import sys, hashlib; sys.path.insert(0, %r); sys.path.insert(0, %r + '/tests')\n"
        "import numpy as np, compute_war_amd as cw\n"
        "from conftest import corpus_file\n"
        "cw.init(0)\n"
        "data = corpus_file('lcet10.txt')[:6*65536] + bytes(65536) + corpus_file('kennedy.xls')[:5*65536]\n"
        "for alg in ('lz4', 'lzf'):\n"
        "    for bs in (4096, 65536):\n"
        "        sizes, payload = cw.compress_blocks(alg, data, bs)\n"
        "        h = hashlib.sha256(sizes.tobytes())\n"
        "        for i in range(len(sizes)): h.update(payload[i, :sizes[i]].tobytes())\n"
        "        print(alg, bs, int(sizes.sum()), h.hexdigest())\n" % (ROOT, ROOT))
    outs = []
    for env in ({}, {"CW_LZ_FORCE_REDO": "1"}):
        import os
        r = subprocess.run([sys.executable, "-c", prog], capture_output=True, text=True, timeout=300, env={**os.environ, **env})
        assert r.returncode == 0, r.stderr[-2000:]
        outs.append(r.stdout)
    assert outs[0] == outs[1] and len(outs[0].splitlines()) == 4


@pytest.mark.parametrize("alg,state_bits,hash_bits", [("skein512", 512, 512), ("skein", 256, 128)])
def test_tree_hash_matches_oracle(cw, oracle, alg, state_bits, hash_bits):
    """N4: Skein tree hashing, one wavefront per block with a lane per leaf, against the oracle (which is pinned to the
    reference's tree KAT vectors): the KAT parameter sets and storage-block shapes, ragged and empty included."""
    rng = np.random.default_rng(state_bits)
    for bs, count, params in [(65536, 9, [(4, 3, 255), (2, 2, 255), (4, 3, 2), (6, 1, 3)]),
                              (4096, 70, [(2, 2, 2), (1, 2, 3), (2, 1, 255), (3, 3, 255)]),
                              (1019, 33, [(2, 2, 2), (1, 2, 3), (2, 1, 255)]),
                              (64, 5, [(1, 1, 255)]), (31, 3, [(1, 2, 3)])]:
        data = rng.integers(0, 256, bs * count, dtype=np.uint8).tobytes()
        for leaf, node, ml in params:
            dig = cw.hash_tree_blocks(alg, data, bs, leaf, node, ml)
            for i in range(count):
                want = oracle.skein_tree(state_bits, data[i * bs:(i + 1) * bs], hash_bits, leaf, node, ml)
                assert dig[i].tobytes() == want, (alg, bs, i, leaf, node, ml)
    # the reference's own vectors with 512-bit results through the device path
    for v in load_golden("skein_kat_tree.json")["vectors"]:
        if (v["state_bits"], v["hash_bits"]) == (state_bits, hash_bits):
            msg = bytes.fromhex(v["msg"])
            assert cw.hash_tree_blocks(alg, msg, len(msg), v["leaf"], v["node"], v["max_level"])[0].tobytes().hex() == v["digest"]
    with pytest.raises(cw.CwError):
        cw.hash_tree_blocks("sha256mb", data, 31, 1, 1, 2)
    with pytest.raises(cw.CwError):
        cw.hash_tree_blocks(alg, bytes(65536), 65536, 0, 1, 2)


def test_lz4_span_scan_with_strides_on_incompressible_blocks(cw, oracle):
    """The span scan kernel (power-of-two sizes, 64 KiB spans) writes the literal run itself: incompressible blocks with
    src_stride > block size, a dst_stride that is not a multiple of 16, whole spans plus a tail that does not fill one."""
    import torch
    s = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(99)
    for bs, nb, sstride in ((4096, 50, 4096 + 32), (16384, 9, 16384 + 16), (65536, 3, 65536), (8192, 17, 8192 + 4096)):
        raw = rng.integers(0, 256, sstride * nb, dtype=np.uint8)
        raw[3 * sstride: 3 * sstride + bs // 2] = 7                      # one compressible block among them
        dev = torch.from_numpy(raw).cuda()
        dstride = cw.compress_bound("lz4", bs) + 5
        dst = torch.zeros(nb * dstride + 64, dtype=torch.uint8, device="cuda")
        sizes = torch.zeros(nb, dtype=torch.int32, device="cuda")
        cw.dev_compress("lz4", dev.data_ptr(), bs, nb, dst.data_ptr(), dstride, sizes.data_ptr(), s, src_stride=sstride)
        torch.cuda.synchronize()
        hz, hdst = sizes.cpu().numpy(), dst.cpu().numpy()
        for i in range(nb):
            want = oracle.lz4_compress(raw[i * sstride: i * sstride + bs].tobytes())
            assert hz[i] == len(want) and hdst[i * dstride: i * dstride + len(want)].tobytes() == want, (bs, i)


@pytest.mark.parametrize("alg,db,bs", [("skein512", 64, 16384), ("skein", 16, 8192), ("skein512", 64, 65536)])
def test_fused_call_sliced_hash_equals_whole_block_hash(cw, oracle, alg, db, bs):
    """From 4,096 blocks on, long Skein messages are hashed in 8 launches of short-lived wavefronts (chaining values
    handed on through a state array), with and without a codec beside them.  Same digests as the one-launch kernel
    (smaller batches) and the oracle."""
    import torch
    nb = 4101 if bs < 65536 else 4097       # a last group that is not full
    s = torch.cuda.current_stream().cuda_stream
    src = torch.empty(nb * bs, dtype=torch.uint8, device="cuda")
    cw.dev_gen_random(0xABCD, 7, nb, bs, src.data_ptr(), s)
    stride = (cw.compress_bound("lz4", bs) + 15) // 16 * 16
    dst = torch.empty(nb * stride, dtype=torch.uint8, device="cuda")
    sizes = torch.zeros(nb, dtype=torch.int32, device="cuda")
    fused = torch.zeros(nb * db, dtype=torch.uint8, device="cuda")
    plain = torch.zeros(nb * db, dtype=torch.uint8, device="cuda")
    for _ in range(2):                      # twice: the state array is reused
        fused.zero_()
        cw.dev_hash_and_compress(alg, "lz4", src.data_ptr(), bs, nb, fused.data_ptr(), dst.data_ptr(), stride, sizes.data_ptr(), s)
    alone = torch.zeros(nb * db, dtype=torch.uint8, device="cuda")
    cw.dev_hash(alg, src.data_ptr(), bs, nb, alone.data_ptr(), s)                 # sliced as well (>= 4096 blocks)
    for first in range(0, nb, 2048):                                              # < 4096 blocks per call: the one-launch kernel
        n = min(2048, nb - first)
        cw.dev_hash(alg, src.data_ptr() + first * bs, bs, n, plain.data_ptr() + first * db, s)
    torch.cuda.synchronize()
    assert torch.equal(fused, plain) and torch.equal(alone, plain)
    host = src.cpu().numpy()
    hd = fused.cpu().numpy()
    for i in (0, 1, 63, 64, nb // 2 - 1, nb // 2, nb // 2 + 1, nb - 2, nb - 1):
        assert hd[i * db:(i + 1) * db].tobytes() == _oracle_hash(oracle, alg, host[i * bs:(i + 1) * bs].tobytes()), i


# ---------------------------------------------------------------- cw_shutdown
def _shutdown_data():
    text = corpus_file("lcet10.txt") + corpus_file("kennedy.xls")[:300000] + corpus_file("ptt5")[:200000]
    return (text * (4096 * 4096 // len(text) + 1))[:4096 * 4096]


def test_shutdown_releases_every_stream_scratch_subprocess(oracle):
    """cw_shutdown gives back the per-stream scratch of every registry, and the library works again after cw_init.  In a process of its
    own (the session's library state is not torn down under the other tests): a fused Skein-512 + LZ4 call and an LZF call over 4096
    blocks of 4 KiB with the lane parsers on (CW_LZ4_LANES=1: 128 MiB of lane tables, both side streams; CW_LZF_LANES=1: 32 MiB of
    links, lane tables, hand-back list, side stream), then cw_shutdown: device memory in use is back within 64 MiB of what it was
    before the calls (the bound of test_short_lived_calling_threads_leave_no_device_memory_behind), while after the calls it was
    more than 64 MiB above it (128 MiB of lane tables alone).  The first pass runs unmeasured, so that what the runtime allocates
    once per process is there already; the calling thread's own context outlives cw_shutdown, so the baseline is taken when it exists."""
    prog = (
        "import sys, hashlib; sys.path.insert(0, %r); sys.path.insert(0, %r + '/tests')\n"
        "import numpy as np, torch, compute_war_amd as cw\n"
        "from test_gpu_parity import _shutdown_data\n"
        "bs, nb = 4096, 4096\n"
        "cw.init(0)\n"
        "s = torch.cuda.current_stream().cuda_stream\n"
        "src = torch.frombuffer(bytearray(_shutdown_data()), dtype=torch.uint8).cuda()\n"
        "stride = (max(cw.compress_bound('lz4', bs), cw.compress_bound('lzf', bs)) + 15) // 16 * 16\n"
        "dig = torch.zeros((nb, 64), dtype=torch.uint8, device='cuda')\n"
        "dst = torch.zeros(nb * stride, dtype=torch.uint8, device='cuda')\n"
        "sizes = torch.zeros(nb, dtype=torch.int32, device='cuda')\n"
        "def run(comp, n=nb):\n"
        "    dig.zero_(); dst.zero_(); sizes.zero_()\n"
        "    if comp == 'lz4': cw.dev_hash_and_compress('skein512', comp, src.data_ptr(), bs, n, dig.data_ptr(), dst.data_ptr(), stride, sizes.data_ptr(), s)\n"
        "    else: cw.dev_compress(comp, src.data_ptr(), bs, n, dst.data_ptr(), stride, sizes.data_ptr(), s)\n"
        "    torch.cuda.synchronize()\n"
        "    z, d = sizes.cpu().numpy().astype(np.uint32), dst.cpu().numpy().reshape(nb, stride)\n"
        "    h = hashlib.sha256(dig.cpu().numpy().tobytes() + z.tobytes())\n"
        "    for i in range(n): h.update(d[i, :z[i]].tobytes())\n"
        "    return h.hexdigest()\n"
        "def used():\n"
        "    torch.cuda.synchronize()\n"
        "    free, total = torch.cuda.mem_get_info()\n"
        "    return total - free\n"
        "with cw.tuned(CW_LZ4_LANES=1, CW_LZF_LANES=1):\n"
        "    run('lz4'); run('lzf'); cw.shutdown(); cw.init(0)   # unmeasured: first use may allocate process-wide state\n"
        "    run('lz4', 64)                                       # the thread's context exists\n"
        "    before = used()\n"
        "    print('lz4', run('lz4')); print('lzf', run('lzf'))\n"
        "    held = used()\n"
        "    cw.shutdown()\n"
        "    after = used()\n"
        "    print('mem', before, held, after)\n"
        "    cw.init(0)\n"
        "    print('lz4', run('lz4'))\n" % (ROOT, ROOT))
    r = subprocess.run([sys.executable, "-c", prog], capture_output=True, text=True, timeout=600, env=dict(os.environ))
    assert r.returncode == 0, r.stderr[-3000:]
    data, bs, nb = _shutdown_data(), 4096, 4096
    blocks = [data[i * bs:(i + 1) * bs] for i in range(nb)]
    want = {}
    for comp, cfn in (("lz4", oracle.lz4_compress), ("lzf", oracle.lzf_compress)):
        outs = [cfn(b) for b in blocks]
        digs = b"".join(oracle.skein512(b, 512) for b in blocks) if comp == "lz4" else bytes(nb * 64)
        want[comp] = hashlib.sha256(digs + np.array([len(o) for o in outs], dtype=np.uint32).tobytes() + b"".join(outs)).hexdigest()
    lines = [ln.split() for ln in r.stdout.strip().splitlines()]
    print(r.stdout)
    assert [ln[0] for ln in lines] == ["lz4", "lzf", "mem", "lz4"], r.stdout
    assert lines[0][1] == want["lz4"] and lines[1][1] == want["lzf"]
    before, held, after = (int(v) for v in lines[2][1:])
    assert held - before > (64 << 20), (before, held, after)    # the calls did allocate scratch a leak of which would show
    assert after - before < (64 << 20), (before, held, after)   # ... and cw_shutdown gave it back
    assert lines[3][1] == want["lz4"]                           # the library works again after cw_init
