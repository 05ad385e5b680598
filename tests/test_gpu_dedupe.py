"""The device-resident dedupe index (cw_dedupe_*, cw_dev_dedupe, cw_dev_hash_dedupe_compress) against a plain-Python model: a
dict of digest bytes -> first value, walked in block order over every call."""
import numpy as np
import pytest

from conftest import corpus_file, corpus_names

pytestmark = pytest.mark.gpu

CW_ERR_BAD_ARG, CW_ERR_NOMEM = -2, -5


@pytest.fixture(scope="module")
def cw():
    import torch  # noqa: F401  (one HIP runtime for torch and libcwhc.so)
    import compute_war_amd as cw
    cw.init(0)
    return cw


class Model:
    """What a sequential CPU loop over each batch gives."""

    def __init__(self):
        self.table = {}

    def call(self, digests: np.ndarray, base: int):
        raw, db = digests.tobytes(), digests.shape[1]
        ref = np.zeros(len(digests), np.uint64)
        new = []
        for i in range(len(digests)):
            k = raw[i * db:(i + 1) * db]
            v = self.table.get(k)
            if v is None:
                v = self.table[k] = base + i
                new.append(i)
            ref[i] = v
        return ref, np.array(new, np.uint32)


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def run_dedupe(idx, digests: np.ndarray, base: int, stream=None):
    """One cw_dev_dedupe call: (ref[n] u64, new_idx[:n_new] u32)."""
    import torch
    n = len(digests)
    d = torch.from_numpy(np.ascontiguousarray(digests)).cuda()
    ref = torch.full((n,), -1, dtype=torch.int64, device="cuda")
    new_idx = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    n_new = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    idx.dev_dedupe(d.data_ptr(), n, base, ref.data_ptr(), new_idx.data_ptr(), n_new.data_ptr(), _stream() if stream is None else stream)
    torch.cuda.synchronize()
    k = int(n_new.item())
    assert 0 <= k <= n
    return ref.cpu().numpy().view(np.uint64), new_idx.cpu().numpy().view(np.uint32)[:k].copy()


def check_call(idx, model, digests, base):
    ref, new_idx = run_dedupe(idx, digests, base)
    mref, mnew = model.call(digests, base)
    bad = np.nonzero(ref != mref)[0]
    assert bad.size == 0, (bad[:8], ref[bad[:8]], mref[bad[:8]])
    assert np.array_equal(new_idx, mnew), (new_idx[:8], mnew[:8])
    assert idx.count() == len(model.table)
    return ref, new_idx


def crafted_digests(db: int, n: int, seed: int) -> np.ndarray:
    """Distinct random digests, then pairs that share their first 8 bytes, their last 8, differ in one middle byte, or hold the
    same 64-bit words in another order; then duplicates planted at random positions."""
    rng = np.random.default_rng(seed)
    d = rng.integers(0, 256, (n, db), dtype=np.uint8)
    q = n // 8
    for i in range(0, q, 2):                      # shared prefix
        d[i + 1, :8] = d[i, :8]
    for i in range(q, 2 * q, 2):                  # shared suffix
        d[i + 1, -8:] = d[i, -8:]
    for i in range(2 * q, 3 * q, 2):              # one middle byte apart
        d[i + 1] = d[i]
        d[i + 1, db // 2] ^= 0x5A
    for i in range(3 * q, 4 * q, 2):              # the same words, permuted (a XOR fold or a word sum collides)
        d[i + 1] = np.roll(d[i].view(np.uint64), 1).view(np.uint8)
    assert len({r.tobytes() for r in d[:4 * q]}) == 4 * q
    dup_at = rng.choice(n, n // 4, replace=False)
    d[dup_at] = d[rng.integers(0, n, dup_at.size)]
    return d


@pytest.mark.parametrize("alg,db", [("skein", 16), ("sha256mb", 32), ("skein512", 64)])
def test_crafted_digests_long_chains(cw, alg, db):
    n = 8192
    d = crafted_digests(db, n, seed=db)
    with cw.DedupeIndex(alg, n) as idx:            # max_entries == nblocks: the table is exactly half full after the call
        model = Model()
        ref, new_idx = check_call(idx, model, d, base=7)
        assert 0 < len(new_idx) < n


def test_across_calls(cw):
    rng = np.random.default_rng(1)
    a = rng.integers(0, 256, (5000, 32), dtype=np.uint8)
    a[rng.choice(5000, 500, replace=False)] = a[rng.integers(0, 5000, 500)]
    fresh = rng.integers(0, 256, (3000, 32), dtype=np.uint8)
    b = np.concatenate([a[rng.integers(0, 5000, 3000)], fresh, fresh[rng.integers(0, 3000, 1000)]])
    b = b[rng.permutation(len(b))]
    with cw.DedupeIndex("sha256mb", 20000) as idx:
        model = Model()
        check_call(idx, model, a, base=0)
        ref, new_idx = check_call(idx, model, b, base=10 ** 6)
        assert (ref < 10 ** 6).sum() >= 3000          # B's copies of A's digests point at A's values
        assert (ref >= 10 ** 6).sum() > 0 and len(new_idx) > 0


def test_determinism_and_permutation(cw):
    rng = np.random.default_rng(2)
    d = rng.integers(0, 256, (50000, 64), dtype=np.uint8)
    d[rng.choice(50000, 20000, replace=False)] = d[rng.integers(0, 50000, 20000)]
    outs = []
    for _ in range(2):
        with cw.DedupeIndex("skein512", 50000) as idx:
            outs.append(run_dedupe(idx, d, 100))
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])
    p = d[rng.permutation(len(d))]
    with cw.DedupeIndex("skein512", 50000) as idx:
        check_call(idx, Model(), p, base=100)


def test_one_digest_repeated_2_20_times(cw):
    n = 1 << 20
    d = np.tile(np.arange(32, dtype=np.uint8), (n, 1))
    with cw.DedupeIndex("sha256mb", n) as idx:
        ref, new_idx = run_dedupe(idx, d, 12345)
        assert new_idx.tolist() == [0]
        assert (ref == 12345).all()
        assert idx.count() == 1


def test_1mi_random_digests_30_percent_duplicates(cw):
    n = 1 << 20
    rng = np.random.default_rng(3)
    n_u = int(n * 0.7)
    uniq = rng.integers(0, 256, (n_u, 32), dtype=np.uint8)
    pick = np.concatenate([np.arange(n_u), rng.integers(0, n_u, n - n_u)])
    d = uniq[pick[rng.permutation(n)]]
    with cw.DedupeIndex("sha256mb", 2 * n) as idx:
        model = Model()
        ref, new_idx = check_call(idx, model, d, base=1 << 40)
        assert len(new_idx) == n_u


def test_full_index_refuses_and_stays_unchanged(cw):
    rng = np.random.default_rng(4)
    a = rng.integers(0, 256, (600, 16), dtype=np.uint8)
    with cw.DedupeIndex("skein", 1000) as idx:
        model = Model()
        check_call(idx, model, a, base=0)
        b = rng.integers(0, 256, (500, 16), dtype=np.uint8)
        with pytest.raises(cw.CwError) as e:
            run_dedupe(idx, b, 5000)
        assert e.value.code == CW_ERR_NOMEM
        assert idx.count() == 600
        ref, new_idx = check_call(idx, model, a[rng.permutation(600)[:400]], base=9000)   # 600 + 400 <= 1000: admitted
        assert len(new_idx) == 0 and (ref < 600).all()


def test_two_streams_without_caller_sync(cw):
    import torch
    rng = np.random.default_rng(5)
    a = rng.integers(0, 256, (200000, 64), dtype=np.uint8)
    b = np.concatenate([a[::3], rng.integers(0, 256, (1000, 64), dtype=np.uint8)])
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    da, db_ = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    ra = torch.zeros(len(a), dtype=torch.int64, device="cuda")
    rb = torch.zeros(len(b), dtype=torch.int64, device="cuda")
    na = torch.zeros(len(a), dtype=torch.int32, device="cuda")
    nb = torch.zeros(len(b), dtype=torch.int32, device="cuda")
    ka = torch.zeros(1, dtype=torch.int64, device="cuda")
    kb = torch.zeros(1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()                      # the inputs are ready; between the two calls nothing waits
    with cw.DedupeIndex("skein512", 400000) as idx:
        idx.dev_dedupe(da.data_ptr(), len(a), 0, ra.data_ptr(), na.data_ptr(), ka.data_ptr(), s1.cuda_stream)
        idx.dev_dedupe(db_.data_ptr(), len(b), 10 ** 6, rb.data_ptr(), nb.data_ptr(), kb.data_ptr(), s2.cuda_stream)
        torch.cuda.synchronize()
        model = Model()
        model.call(a, 0)
        mref, mnew = model.call(b, 10 ** 6)
        assert np.array_equal(rb.cpu().numpy().view(np.uint64), mref)
        assert int(kb.item()) == len(mnew) == 1000
        assert idx.count() == len(a) + 1000


# ---- the fused call ---------------------------------------------------------------------------------------------------
def _corpus_blocks(bs: int, n: int, seed: int) -> np.ndarray:
    """Corpus blocks, then planted duplicates and a run of all-zero blocks: (n, bs) uint8."""
    data = b"".join(corpus_file(f) for f in corpus_names())
    a = np.frombuffer((data * (n * bs // len(data) + 1))[:n * bs], dtype=np.uint8).reshape(n, bs).copy()
    rng = np.random.default_rng(seed)
    a[n // 3] = rng.integers(0, 256, bs, dtype=np.uint8)                 # one incompressible block
    dup_at = rng.choice(n, n // 5, replace=False)
    a[dup_at] = a[rng.integers(0, n, dup_at.size)]
    z0 = rng.integers(0, n - n // 8)
    a[z0:z0 + n // 8] = 0
    return a


def _hash_of(alg):
    return {"skein512": 0, "skein": 1, "sha256mb": 2}[alg]


def _oracle_compress(oracle, comp, b: bytes) -> bytes:
    return oracle.lz4_compress(b) if comp == "lz4" else oracle.lzf_compress(b)


def _fused(cw, idx, comp, blocks: np.ndarray, base: int, src_stride: int | None = None):
    """Run cw_dev_hash_dedupe_compress; returns everything on the host plus the device buffers for further checks."""
    import torch
    n, bs = blocks.shape
    stride = src_stride or bs
    host = np.full((n, stride), 0xA5, np.uint8)
    host[:, :bs] = blocks
    src = torch.from_numpy(host.reshape(-1)).cuda()
    db = cw.digest_bytes(idx.hash_alg)
    dst_stride = (cw.compress_bound(comp, bs) + 15) // 16 * 16
    dig = torch.zeros((n, db), dtype=torch.uint8, device="cuda")
    ref = torch.zeros(n, dtype=torch.int64, device="cuda")
    new_idx = torch.zeros(n, dtype=torch.int32, device="cuda")
    dst = torch.zeros(n * dst_stride, dtype=torch.uint8, device="cuda")
    sizes = torch.zeros(n, dtype=torch.int32, device="cuda")
    k = idx.dev_hash_dedupe_compress(comp, src.data_ptr(), bs, n, base, dig.data_ptr(), ref.data_ptr(), new_idx.data_ptr(),
                                     dst.data_ptr(), dst_stride, sizes.data_ptr(), _stream(), src_stride=stride)
    torch.cuda.synchronize()
    return dict(k=k, src=src, stride=stride, dig=dig, ref=ref.cpu().numpy().view(np.uint64),
                new_idx=new_idx.cpu().numpy().view(np.uint32)[:k].copy(), dst=dst, dst_stride=dst_stride,
                sizes=sizes.cpu().numpy().view(np.uint32)[:k].copy(), sizes_t=sizes)


@pytest.mark.parametrize("hash_alg,comp", [("skein512", "lz4"), ("skein", "lz4"), ("sha256mb", "lzf")])
@pytest.mark.parametrize("bs,n", [(4096, 1024), (65536, 96)])
def test_fused_call_against_model_and_oracle(cw, oracle, hash_alg, comp, bs, n):
    import torch
    blocks = _corpus_blocks(bs, n, seed=bs + len(hash_alg))
    model = Model()
    with cw.DedupeIndex(hash_alg, 4 * n) as idx:
        again = blocks[::-1].copy()
        again[::7, 100] ^= 0xFF                   # the second call: mostly repeats of the first, some new blocks, src_stride > block_bytes
        for src_blocks, base, stride in ((blocks, 0, None), (again, 10 ** 6, bs + 48)):
            r = _fused(cw, idx, comp, src_blocks, base, stride)
            # digests byte-equal to cw_dev_hash over the same blocks
            want = torch.zeros_like(r["dig"])
            cw.dev_hash(hash_alg, r["src"].data_ptr(), bs, n, want.data_ptr(), _stream(), src_stride=r["stride"])
            torch.cuda.synchronize()
            assert torch.equal(r["dig"], want)
            digests = r["dig"].cpu().numpy()
            mref, mnew = model.call(digests, base)
            assert np.array_equal(r["ref"], mref)
            assert np.array_equal(r["new_idx"], mnew) and r["k"] == len(mnew)
            assert idx.count() == len(model.table)
            assert 0 < r["k"] < n
            slots = r["dst"].view(n, r["dst_stride"]).cpu().numpy()
            expect = []
            for j, i in enumerate(r["new_idx"]):
                w = _oracle_compress(oracle, comp, src_blocks[i].tobytes())
                assert r["sizes"][j] == len(w), (j, i)
                assert slots[j, :len(w)].tobytes() == w, (j, i)
                expect.append(w)
            # every non-empty slot decodes back to its block
            k = r["k"]
            out = torch.zeros(k * bs, dtype=torch.uint8, device="cuda")
            status = torch.ones(k, dtype=torch.int32, device="cuda")
            cw.dev_decompress(comp, r["dst"].data_ptr(), r["dst_stride"], r["sizes_t"].data_ptr(), k, out.data_ptr(), bs,
                              status.data_ptr(), _stream())
            torch.cuda.synchronize()
            st, dec = status.cpu().numpy(), out.view(k, bs).cpu().numpy()
            for j, i in enumerate(r["new_idx"]):
                if r["sizes"][j]:
                    assert st[j] == 0 and np.array_equal(dec[j], src_blocks[i]), (j, i)
            # cw_dev_pack over the first n_new slots: the stream of the new blocks
            offs = torch.zeros(k + 1, dtype=torch.int64, device="cuda")
            packed = torch.zeros(max(int(r["sizes"].sum()), 1), dtype=torch.uint8, device="cuda")
            cw.dev_pack(r["dst"].data_ptr(), r["dst_stride"], r["sizes_t"].data_ptr(), k, packed.data_ptr(), offs.data_ptr(), _stream())
            torch.cuda.synchronize()
            total = int(offs[k].item())
            assert packed.cpu().numpy()[:total].tobytes() == b"".join(expect)


@pytest.mark.parametrize("hash_alg,comp,bs,n", [("skein512", "lz4", 65536, 64), ("skein", "lz4", 4096, 2048), ("sha256mb", "lzf", 4096, 2048)])
def test_fused_call_on_unique_input_equals_hash_and_compress(cw, hash_alg, comp, bs, n):
    import torch
    data = b"".join(corpus_file(f) for f in corpus_names())
    blocks = np.frombuffer((data * (n * bs // len(data) + 1))[:n * bs], dtype=np.uint8).reshape(n, bs).copy()
    blocks[:, :8] = np.arange(n, dtype=np.uint64)[:, None].view(np.uint8)       # every block distinct
    with cw.DedupeIndex(hash_alg, n) as idx:
        r = _fused(cw, idx, comp, blocks, 0)
    assert r["k"] == n and np.array_equal(r["new_idx"], np.arange(n, dtype=np.uint32))
    dig = torch.zeros_like(r["dig"])
    dst = torch.zeros_like(r["dst"])
    sizes = torch.zeros_like(r["sizes_t"])
    cw.dev_hash_and_compress(hash_alg, comp, r["src"].data_ptr(), bs, n, dig.data_ptr(), dst.data_ptr(), r["dst_stride"],
                             sizes.data_ptr(), _stream())
    torch.cuda.synchronize()
    assert torch.equal(dig, r["dig"]) and torch.equal(sizes, r["sizes_t"])
    sz = sizes.cpu().numpy()
    a, b = dst.view(n, -1).cpu().numpy(), r["dst"].view(n, -1).cpu().numpy()
    for i in range(n):
        assert a[i, :sz[i]].tobytes() == b[i, :sz[i]].tobytes(), i


def test_zero_block_calls_are_no_ops(cw):
    import torch
    sentinel = torch.full((4,), 77, dtype=torch.int64, device="cuda")
    with cw.DedupeIndex("skein", 16) as idx:
        idx.dev_dedupe(0, 0, 0, 0, 0, 0, _stream())
        k = idx.dev_hash_dedupe_compress("lz4", 0, 4096, 0, 0, 0, 0, 0, 0, 4128, 0, _stream())
        assert k == 0 and idx.count() == 0
        idx.dev_dedupe(sentinel.data_ptr(), 0, 5, sentinel.data_ptr(), sentinel.data_ptr(), sentinel.data_ptr(), _stream())
        torch.cuda.synchronize()
        assert (sentinel.cpu() == 77).all() and idx.count() == 0


def test_bad_arguments(cw):
    import torch
    d = torch.zeros((8, 16), dtype=torch.uint8, device="cuda")
    u = torch.zeros(8, dtype=torch.int64, device="cuda")
    with pytest.raises(cw.CwError):
        cw.DedupeIndex(9, 16)                                     # no such hash algorithm
    with pytest.raises(cw.CwError):
        cw.DedupeIndex("skein", 0)
    with cw.DedupeIndex("skein", 16) as idx:
        for args in ((0, 8, 0, u.data_ptr(), u.data_ptr(), u.data_ptr()),                  # NULL digests
                     (d.data_ptr(), 8, 0, 0, u.data_ptr(), u.data_ptr()),                  # NULL ref
                     (d.data_ptr(), 8, 2 ** 64 - 5, u.data_ptr(), u.data_ptr(), u.data_ptr()),  # base + nblocks wraps
                     (d.data_ptr(), 2 ** 32, 0, u.data_ptr(), u.data_ptr(), u.data_ptr())):     # nblocks >= 2^32
            with pytest.raises(cw.CwError) as e:
                idx.dev_dedupe(*args, _stream())
            assert e.value.code == CW_ERR_BAD_ARG, args
        src = torch.zeros(8 * 4096, dtype=torch.uint8, device="cuda")
        dst = torch.zeros(8 * 4224, dtype=torch.uint8, device="cuda")
        sz = torch.zeros(8, dtype=torch.int32, device="cuda")
        for comp, base in ((7, 0), (2, 0), ("lz4", 2 ** 64 - 1)):                         # wrong codec / none / wrapping base
            with pytest.raises(cw.CwError) as e:
                idx.dev_hash_dedupe_compress(comp, src.data_ptr(), 4096, 8, base, d.data_ptr(), u.data_ptr(), u.data_ptr(),
                                             dst.data_ptr(), 4224, sz.data_ptr(), _stream())
            assert e.value.code == CW_ERR_BAD_ARG, comp
        with pytest.raises(cw.CwError) as e:                                                   # NULL dst
            idx.dev_hash_dedupe_compress("lz4", src.data_ptr(), 4096, 8, 0, d.data_ptr(), u.data_ptr(), u.data_ptr(), 0, 4224,
                                         sz.data_ptr(), _stream())
        assert e.value.code == CW_ERR_BAD_ARG
        assert idx.count() == 0
