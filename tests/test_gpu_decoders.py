"""Decoder differential: one set of foreign and malformed streams (lz_streams.py), every way into the decoders.

The doors: cw_dev_decompress with the wavefront decoders (CW_DECODE_LANES=0: slot staged in LDS or read from global memory,
by block size) and with the lane decoders (CW_DECODE_LANES=1), cw_dev_decompress_chunks over the same streams packed end to
end, cw_decompress_blocks over host buffers, and the reference's one-slot calls cw_decompress_lz4 / cw_decompress_lzf.  Per
door: the status list is the oracle decoder's verdict list, every status-0 block is the oracle's bytes (and the builder's own
plaintext where it built the stream), nothing is written outside a slot's block -- guards around dst and every third slot a
skip slot whose whole block must keep the fill -- and nothing depends on bytes the decoder was not given (the slack of every
slot 0x00, then 0xFF; the packed stream in reversed order).  Every buffer is over-allocated: a wrong decoder fails a comparison."""
import numpy as np
import pytest

import lz_streams as Z
from conftest import corpus_file

pytestmark = pytest.mark.gpu
FILL = 0xA5
GUARD = 256
SETS = [(codec, bs) for codec in ("lz4", "lzf") for bs in Z.block_sizes(codec)]


@pytest.fixture(scope="module")
def cw():
    import torch  # noqa: F401  (one HIP runtime for torch and libcwhc.so)
    import compute_war_amd as cw
    cw.init(0)
    yield cw
    cw.tune_reset()


@pytest.fixture(scope="module")
def corpus():
    return corpus_file("alice29.txt")


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _dev_u64(values):
    import torch
    return torch.from_numpy(np.asarray(values, np.uint64).view(np.int64).copy()).cuda()


class Slots:
    """The cases of one set as decoder slots: every third slot is a skip slot (no input, status 1, nothing written)."""

    def __init__(self, cases, verdict, bs, extra=(), limit=None):
        """limit: the comp_stride the slots will get when it is smaller than some streams; those are malformed by the decoders' own
        rule (a size beyond the slot), whatever the oracle says about their bytes."""
        self.bs = bs
        self.streams, self.want, self.bytes, self.plain = [], [], [], []
        for i, (c, (st, got)) in enumerate(list(zip(cases, verdict)) + list(extra)):
            if limit is not None and len(c.stream) > limit:
                st, got = 1, None
            self.streams.append(c.stream); self.want.append(st); self.bytes.append(got); self.plain.append(c.plain)
            if i % 2 == 1:
                self.streams.append(b""); self.want.append(1); self.bytes.append(None); self.plain.append(None)
        self.nb = len(self.streams)
        self.sizes = np.array([len(s) for s in self.streams], np.uint32)

    def slot_array(self, stride, slack):
        a = np.full((self.nb, stride), slack, np.uint8)
        for i, s in enumerate(self.streams):
            a[i, :min(len(s), stride)] = np.frombuffer(s[:stride], np.uint8)
        return a

    def check(self, status, out, door, skips_keep_fill=True):
        """status[nb]; out = GUARD + nb * bs + GUARD bytes of a device door, nb * bs of a host door.  Returns the blocks."""
        status = [int(x) for x in status]
        wrong = [i for i in range(self.nb) if status[i] != self.want[i]]
        assert not wrong, (f"{door}: {len(wrong)} verdicts differ from the oracle's, first slot {wrong[0]} "
                           f"({len(self.streams[wrong[0]])} bytes): got {status[wrong[0]]}, want {self.want[wrong[0]]}")
        guarded = out.size == 2 * GUARD + self.nb * self.bs
        if guarded:
            assert (out[:GUARD] == FILL).all() and (out[-GUARD:] == FILL).all(), f"{door}: a guard was written"
            out = out[GUARD:-GUARD]
        blocks = out.reshape(self.nb, self.bs)
        for i in range(self.nb):
            if self.want[i] == 0:
                got = blocks[i].tobytes()
                assert got == self.bytes[i], f"{door}: slot {i} decoded to other bytes than the oracle's"
                assert self.plain[i] is None or got == self.plain[i], f"{door}: slot {i} is not the builder's plaintext"
            elif skips_keep_fill and not self.streams[i]:
                assert (blocks[i] == FILL).all(), f"{door}: skip slot {i} was written (a neighbour's overrun or underrun)"
        return blocks


def _run_fixed(cw, codec, slots, stride, slack, lanes, misalign=0):
    """cw_dev_decompress over the slots (slack = the byte behind every slot's stream); returns (status, guarded dst)."""
    import torch
    host = np.full(misalign + slots.nb * stride + 64, slack, np.uint8)
    host[misalign:misalign + slots.nb * stride] = slots.slot_array(stride, slack).reshape(-1)
    d_comp = torch.from_numpy(host).cuda()
    d_sizes = torch.from_numpy(slots.sizes.view(np.int32).copy()).cuda()
    dst = torch.full((GUARD + slots.nb * slots.bs + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    status = torch.full((slots.nb,), -1, dtype=torch.int32, device="cuda")
    with cw.tuned(CW_DECODE_LANES=lanes):
        cw.dev_decompress(codec, d_comp.data_ptr() + misalign, stride, d_sizes.data_ptr(), slots.nb, dst.data_ptr() + GUARD, slots.bs,
                          status.data_ptr(), _stream())
    torch.cuda.synchronize()
    return status.cpu().numpy(), dst.cpu().numpy()


def _run_chunks(cw, codec, slots, order):
    """cw_dev_decompress_chunks: position j holds slot order[j]'s stream, packed end to end, and decodes to raw extent j."""
    import torch
    streams = [slots.streams[i] for i in order]
    packed = np.frombuffer(b"".join(streams) + bytes([FILL]) * 64, np.uint8).copy()
    d_packed = torch.from_numpy(packed).cuda()
    d_coff = _dev_u64(np.concatenate([[0], np.cumsum([len(s) for s in streams])]))
    d_roff = _dev_u64(np.arange(slots.nb + 1, dtype=np.uint64) * slots.bs)
    dst = torch.full((GUARD + slots.nb * slots.bs + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    status = torch.full((slots.nb,), -1, dtype=torch.int32, device="cuda")
    cw.dev_decompress_chunks(codec, d_packed.data_ptr(), d_coff.data_ptr(), d_roff.data_ptr(), _dev_u64([slots.nb]).data_ptr(), slots.nb,
                             dst.data_ptr() + GUARD, slots.nb * slots.bs, status.data_ptr(), _stream())
    torch.cuda.synchronize()
    return status.cpu().numpy(), dst.cpu().numpy()


def _slots(oracle, corpus, codec, bs):
    cases, verdict = Z.oracle_set(oracle, codec, bs, corpus)
    return Slots(cases, verdict, bs)


def _stride(slots):
    return (int(slots.sizes.max()) + 15) // 16 * 16


def _same_where_ok(slots, a, b, door):
    for i in range(slots.nb):
        if slots.want[i] == 0:
            assert np.array_equal(a[i], b[i]), f"{door}: slot {i} depends on bytes behind its stream"


@pytest.mark.parametrize("lanes", [0, 1], ids=["wavefront", "lanes"])
@pytest.mark.parametrize("codec,bs", SETS)
def test_dev_decompress_gives_the_oracles_verdict(cw, oracle, corpus, codec, bs, lanes):
    """CW_DECODE_LANES=0: the wavefront decoder, slot staged in LDS up to staging_pair()[0], read from global memory above it (and
    for any slot longer than the staging buffer); =1: the lane decoder.  Twice, with 0x00 and with 0xFF behind every stream."""
    slots = _slots(oracle, corpus, codec, bs)
    door = f"cw_dev_decompress {codec} {bs} CW_DECODE_LANES={lanes}"
    runs = []
    for slack in (0x00, 0xFF):
        status, out = _run_fixed(cw, codec, slots, _stride(slots), slack, lanes)
        runs.append(slots.check(status, out, f"{door} slack {slack:#x}"))
    _same_where_ok(slots, runs[0], runs[1], door)


@pytest.mark.parametrize("codec,bs", SETS)
def test_dev_decompress_chunks_gives_the_oracles_verdict(cw, oracle, corpus, codec, bs):
    """The same streams packed end to end (a skip slot is an empty extent), then in reversed order: other neighbours, other
    alignment of every stream, the same verdict and bytes."""
    slots = _slots(oracle, corpus, codec, bs)
    order = list(range(slots.nb))
    status, out = _run_chunks(cw, codec, slots, order)
    slots.check(status, out, f"cw_dev_decompress_chunks {codec} {bs}")
    back = Slots.__new__(Slots)
    back.bs, back.nb = bs, slots.nb
    for name in ("streams", "want", "bytes", "plain"):
        setattr(back, name, getattr(slots, name)[::-1])
    status, out = _run_chunks(cw, codec, slots, order[::-1])
    back.check(status, out, f"cw_dev_decompress_chunks {codec} {bs} reversed")


@pytest.mark.parametrize("codec,bs", SETS)
def test_decompress_blocks_gives_the_oracles_verdict(cw, oracle, corpus, codec, bs):
    """Host buffers.  (The blocks of status-1 slots come back as the call's device scratch held them: unspecified, so the skip
    slots are compared by status only.)"""
    slots = _slots(oracle, corpus, codec, bs)
    runs = []
    for slack in (0x00, 0xFF):
        out, status = cw.decompress_blocks(codec, slots.sizes, slots.slot_array(_stride(slots) + 3, slack), bs)
        runs.append(slots.check(status, out.reshape(-1), f"cw_decompress_blocks {codec} {bs} slack {slack:#x}", skips_keep_fill=False))
    _same_where_ok(slots, runs[0], runs[1], f"cw_decompress_blocks {codec} {bs}")


@pytest.mark.parametrize("codec", ["lz4", "lzf"])
def test_one_slot_calls_give_the_oracles_verdict(cw, oracle, corpus, codec):
    """cw_decompress_lz4 / cw_decompress_lzf on a sample of the 4096 set that holds every stream longer than the block: the block
    size for an accepted stream (liblzf's lzf_decompress returns it for the expanding streams), -1 / 0 otherwise."""
    bs = 4096
    cases, verdict = Z.oracle_set(oracle, codec, bs, corpus)
    long = [i for i, c in enumerate(cases) if c.edit is None and len(c.stream) > bs]
    sample = sorted(set(long + list(range(0, len(cases), max(1, len(cases) // 64)))))
    if codec == "lzf":
        assert any(cases[i].family == "expand_runs1" for i in sample) and any(cases[i].family == "expand_runs32" for i in sample)
    cw.set_block_size(bs)
    for i in sample:
        got = cw.do_decompression(codec, cases[i].stream, bs)
        st, want = verdict[i]
        assert got == (want if st == 0 else b""), f"{codec}: case {i} ({cases[i].family}, {cases[i].edit})"


@pytest.mark.parametrize("lanes", [0, 1], ids=["wavefront", "lanes"])
@pytest.mark.parametrize("codec", ["lz4", "lzf"])
def test_slot_layout_edges(cw, oracle, corpus, codec, lanes):
    """The 4093 set with an odd comp_stride (no slot but the first is 16-byte aligned: the byte-wise staging copy), d_comp off
    alignment by 1, 7 and 15, and a slot that fills its stride to the last byte (a stream with junk behind it).  For LZF once more
    with comp_stride = 2 * bs - 1 and a VALID stream of exactly that length; the few streams longer than that (junk behind 1-byte
    runs) then exceed their slot, which is malformed by the decoders' own rule."""
    bs = 4093
    cases, verdict = Z.oracle_set(oracle, codec, bs, corpus)
    stride = max(len(c.stream) for c in cases) | 1
    rng = np.random.default_rng(77)
    decode = oracle.lz4_decompress if codec == "lz4" else oracle.lzf_decompress
    base = next(c for c in cases if c.edit is None and c.family == "encoded")
    full = [Z.Case(codec, base.stream + rng.bytes(stride - len(base.stream)), "encoded", "junk", None)]
    assert len(full[0].stream) == stride
    slots = Slots(cases, verdict, bs, list(zip(full, Z.verdicts(decode, full, bs))))
    for misalign, slack in ((0, 0xFF), (1, 0x00), (7, 0xFF), (15, 0x00)):
        status, out = _run_fixed(cw, codec, slots, stride, slack, lanes, misalign)
        slots.check(status, out, f"cw_dev_decompress {codec} {bs} stride {stride} base + {misalign} CW_DECODE_LANES={lanes}")
    if codec == "lzf":
        stride = 2 * bs - 1
        s, p = Z.lzf_stream(Z.lzf_of_length(bs, stride, rng))
        full = [Z.Case(codec, s, "expand_runs1", None, p)]
        extra = list(zip(full, Z.verdicts(decode, full, bs)))
        assert len(s) == stride and extra[0][1] == (0, p)
        slots = Slots(cases, verdict, bs, extra, limit=stride)
        assert 0 < sum(1 for c in cases if len(c.stream) > stride) < 20
        status, out = _run_fixed(cw, codec, slots, stride, 0xFF, lanes, 7)
        slots.check(status, out, f"cw_dev_decompress {codec} {bs} stride {stride} base + 7 CW_DECODE_LANES={lanes}")
