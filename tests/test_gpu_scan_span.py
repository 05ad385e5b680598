"""GPU tests of the LZ4 span scan (power-of-two blocks of 4-64 KiB): every slot byte the call defines against the oracle, over
slot strides that are and are not multiples of 16 and slots shifted by 1-15 bytes (every store shift of the literal run), blocks with
a 4-byte repeat planted at chosen probe positions (first chunk, both sides of a chunk boundary, last chunk, final probe), a queued
4 KiB block between unqueued ones in one span, and call sizes that leave a tail to the per-block streaming scan."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cw():
    import torch  # noqa: F401  (one HIP runtime for torch and libcwhc.so)
    import compute_war_amd as cw
    cw.init(0)
    return cw


def scan_probes(n):
    """number of probes of the parser's no-match walk over n bytes"""
    limit, k, p, step, nb = n - 11, 0, 1, 1, 64
    while p + step <= limit:
        p += step
        step = nb >> 6
        nb += 1
        k += 1
    return k


def probe_pos(k):
    """position of probe k of the no-match walk"""
    if k == 0:
        return 1
    t = 62 + k
    q, r = t >> 6, t & 63
    return 2 + q * (32 * (q - 1) + r + 1)


def plant(block, k):
    """make probe k the first that matches: one byte repeated from probe k - 1's position to 8 bytes past probe k's, so that probe
    k - 1 inserts a word nothing earlier had and probe k finds it (a match long enough to shorten the block's encoding)"""
    p, q = probe_pos(k), probe_pos(k - 1)
    block[q:p + 8] = block[q]


def planted_probes(n):
    npr = scan_probes(n)
    pos = [probe_pos(k) for k in range(npr)]
    first_past = next((k for k in range(npr) if pos[k] >= 4096), npr - 1)  # first probe of the second chunk
    last_chunk = next(k for k in range(npr) if pos[k] >= n - 4096)
    return sorted({5, first_past - 1, first_past, last_chunk + 2, npr - 1})


def run(cw, oracle, a, bs, nb, stride, shift):
    import torch
    s = torch.cuda.current_stream().cuda_stream
    src = torch.from_numpy(a).cuda()
    dst = torch.zeros(nb * stride + 64, dtype=torch.uint8, device="cuda")
    sizes = torch.zeros(nb, dtype=torch.int32, device="cuda")
    cw.dev_compress("lz4", src.data_ptr(), bs, nb, dst.data_ptr() + shift, stride, sizes.data_ptr(), s)
    torch.cuda.synchronize()
    hz, hd = sizes.cpu().numpy(), dst.cpu().numpy()
    assert not hd[:shift].any(), "bytes in front of the first slot were written"
    for i in range(nb):
        want = oracle.lz4_compress(a[i * bs:(i + 1) * bs].tobytes())
        o = shift + i * stride
        assert hz[i] == len(want), (bs, stride, shift, i)
        assert hd[o:o + len(want)].tobytes() == want, (bs, stride, shift, i)
    return hz


def literal_size(n):
    return 2 + (n - 15) // 255 + n


@pytest.mark.parametrize("bs", [4096, 8192, 16384, 32768, 65536])
def test_random_blocks_every_stride_and_shift(cw, oracle, bs):
    """random blocks (one literal run each): 16-byte-aligned slots, unaligned strides, and slots shifted by 1-15 bytes"""
    run_ = 16 * 4096 // bs
    nb = 2 * run_ + (1 if run_ > 1 else 0)  # two spans, and (below 64 KiB) one block for the streaming scan
    a = np.random.default_rng(bs).integers(0, 256, nb * bs, dtype=np.uint8)
    bound = cw.compress_bound("lz4", bs)
    aligned = (bound + 15) // 16 * 16
    for stride, shift in [(aligned, 0), (bound, 0), (aligned + 16, 0), (aligned, 2), (aligned, 14)] + \
                         [(aligned + 16, sh) for sh in (1, 3, 5, 7, 8, 9, 11, 13, 15)] + [(bound + 1, 4), (bound + 7, 6)]:
        hz = run(cw, oracle, a, bs, nb, stride, shift)
        assert (hz == literal_size(bs)).all()


@pytest.mark.parametrize("bs", [4096, 8192, 16384, 32768, 65536])
def test_planted_repeats_at_chosen_probes(cw, oracle, bs):
    """one block per planted probe (first chunk, either side of the first chunk boundary, last chunk, final probe) between random
    blocks, in aligned and unaligned slots"""
    ks = planted_probes(bs)
    run_ = 16 * 4096 // bs
    nb = max(2 * len(ks) + 1, 2 * run_) + (3 if run_ > 1 else 0)
    rng = np.random.default_rng(100 + bs)
    a = rng.integers(0, 256, nb * bs, dtype=np.uint8)
    planted = {}
    for j, k in enumerate(ks):
        i = 2 * j + 1
        plant(a[i * bs:(i + 1) * bs], k)
        planted[i] = k
    for i, k in planted.items():  # the oracle parser does match there: the plant is not a literal run
        assert len(oracle.lz4_compress(a[i * bs:(i + 1) * bs].tobytes())) < literal_size(bs), (bs, k)
    bound = cw.compress_bound("lz4", bs)
    for stride, shift in [((bound + 15) // 16 * 16, 0), (bound, 3)]:
        hz = run(cw, oracle, a, bs, nb, stride, shift)
        for i in range(nb):
            assert (hz[i] < literal_size(bs)) == (i in planted), (bs, i)


def test_queued_4k_block_between_unqueued_ones(cw, oracle):
    """a span of 16 blocks of 4 KiB whose 8th block has a match, the rest random; two spans and a tail of 5 blocks"""
    bs, nb = 4096, 37
    a = np.random.default_rng(7).integers(0, 256, nb * bs, dtype=np.uint8)
    for i in (7, 16 + 15, 33):
        plant(a[i * bs:(i + 1) * bs], 40)
    bound = cw.compress_bound("lz4", bs)
    for stride, shift in [((bound + 15) // 16 * 16, 0), ((bound + 15) // 16 * 16, 9), (bound, 0)]:
        hz = run(cw, oracle, a, bs, nb, stride, shift)
        assert [i for i in range(nb) if hz[i] < literal_size(bs)] == [7, 31, 33]
