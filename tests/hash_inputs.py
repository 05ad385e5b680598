"""Hash inputs built for an edge: the messages and call shapes that take the hash kernels to their step, line and slice edges
(the digests' counterpart of lz_inputs.py, which builds the encoders' inputs).

Pure Python plus numpy, fixed seeds: no GPU, no ctypes, no library.  Two sets:

* the one-launch set: every length of LENGTHS, 67 messages per length (one wavefront and three lanes, so the `gid >= nblocks`
  edge of a second workgroup is live) -- fixed families, each with a twin that differs in the last byte only, and seeded
  noise -- and lay_out(), which puts a length's messages at any stride and shift with non-zero poison in every gap;
* SLICED / THRESHOLD: the (algorithm, block size, CW_SKEIN_NSLICES, block count) calls that take the sliced Skein launches to
  their edges, each row with the properties it exists for.  The rows were chosen with a restatement of the slicing arithmetic;
  test_hash_inputs.py confirms every property from the library's own plan (cw_hash_plan_describe), not from a copy.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

ALGS = ("skein512", "skein", "sha256")
STEP = {"skein512": 64, "skein": 32, "sha256": 64}        # BB: bytes per compression step
DIGEST = {"skein512": 64, "skein": 16, "sha256": 32}
SPL = {"skein512": 2, "skein": 4}                         # steps per 128-byte line
SLICED_FLOOR = {"skein512": 16320, "skein": 8160}         # the smallest sliced message: 255 message steps + the output transform

PER_LENGTH = 67
FAMILIES = ("zeros", "ones", "last80", "last00", "counter")
# every residue of step, line and half line, SHA-256's 55/56/63/64 padding split and the empty message; one step either side of
# 4096 and of the two sliced floors; the largest block and one byte less
LENGTHS = tuple(sorted(set(range(386)) | {k + d for k in (4096, 8160, 16320) for d in (-1, 0, 1)} | {65535, 65536}))


@dataclass(frozen=True)
class Case:
    family: str   # one of FAMILIES, or "random"
    kind: str     # "base", "twin" (the base with its last byte changed) or "random"
    arg: int      # the message's length

    def __str__(self):
        return f"{self.family} {self.kind} {self.arg}"


def case(length: int, i: int) -> Case:
    """What message i of a length is."""
    if i < 2 * len(FAMILIES):
        return Case(FAMILIES[i // 2], "twin" if i % 2 else "base", length)
    return Case("random", "random", length)


_MESSAGES = {}


def messages(length: int) -> np.ndarray:
    """[PER_LENGTH, length] uint8, read-only: base and twin of every family, then seeded noise."""
    if length not in _MESSAGES:
        rng = np.random.default_rng(0x5EED0000 + length)
        m = rng.integers(0, 256, (PER_LENGTH, length), dtype=np.uint8)
        if length:
            m[0] = 0x00
            m[2] = 0xFF       # every first key-injection add carries across the 32-bit halves
            m[4, -1] = 0x80   # SHA-256 padding look-alikes: the message ends where the padding would begin ...
            m[6, -1] = 0x00   # ... or where it would go on
            m[8] = (np.arange(length) * 131 + (np.arange(length) >> 8)) & 0xFF
            for f in range(len(FAMILIES)):
                m[2 * f + 1] = m[2 * f]
                m[2 * f + 1, -1] ^= 0x01
        m.setflags(write=False)
        _MESSAGES[length] = m
    return _MESSAGES[length]


def lay_out(msgs: np.ndarray, stride: int, shift: int, seed: int, tail: int = 64):
    """(buf, gap): the messages at buf[shift + i * stride], every other byte of buf -- the `shift` bytes in front, the gaps between
    the messages and `tail` bytes behind the last -- seeded non-zero poison whose first byte differs from gap to gap.  gap is the
    mask of the poison bytes.  A kernel that lets one byte past a message into a word then differs from the oracle."""
    n, length = msgs.shape
    assert stride >= length and shift >= 0
    rng = np.random.default_rng(seed)
    size = shift + n * stride + tail
    buf = rng.integers(1, 256, size, dtype=np.uint8)
    if stride > length:   # the first byte behind message i is unlike the first byte behind message i - 1
        first = shift + np.arange(n) * stride + length
        for i in range(1, n):
            if buf[first[i]] == buf[first[i - 1]]:
                buf[first[i]] = buf[first[i]] % 255 + 1
    gap = np.ones(size, dtype=bool)
    if length:
        at = (shift + np.arange(n)[:, None] * stride + np.arange(length)[None, :]).reshape(-1)
        buf[at] = msgs.reshape(-1)
        gap[at] = False
    return buf, gap


# ---- the sliced launches ---------------------------------------------------------------------------------------------------------
NBLOCKS_SLICED = 4101   # the smallest count above the 4,096 floor that leaves a partial last workgroup (4101 = 64 * 64 + 5)


@dataclass(frozen=True)
class Sliced:
    alg: str
    block_bytes: int
    nslices: int | None    # CW_SKEIN_NSLICES; None = unset (8 slices)
    edge: str              # what the row is for
    launches: int          # number of launches
    last: int              # steps of the last launch
    tail: int              # launches at the end that are not interior (Skein-256 has no interior kernel: all of them)
    tight: bool = False    # the last interior slice's prefetch ends exactly on the last message step: e + spl == total - 1
    output_only: bool = False   # the last launch holds the output transform alone

    @property
    def total(self):       # steps per block: the message steps and the output transform
        return self.block_bytes // STEP[self.alg] + 1

    @property
    def knobs(self):
        return {} if self.nslices is None else {"CW_SKEIN_NSLICES": self.nslices}

    def __str__(self):
        return f"{self.alg} {self.block_bytes} nslices={self.nslices}"


SLICED = (
    Sliced("skein512", 16320, None, "smallest sliced message (total 256), 8 equal slices", 8, 32, 1),
    Sliced("skein512", 16320, 1, "one non-interior launch for the whole message", 1, 256, 1),
    Sliced("skein512", 16320, 100000, "one-line slices, 128 launches, the last two non-interior", 128, 2, 2),
    Sliced("skein512", 16384, None, "the size the suite has (last slice 19 steps)", 8, 19, 1),
    Sliced("skein512", 16384, 255, "last launch is the output transform alone; last interior slice with e + spl == total - 1", 129, 1, 2,
           tight=True, output_only=True),
    Sliced("skein512", 16448, 3, "total even, uneven slices", 3, 86, 1),
    Sliced("skein512", 16512, 127, "last slice 3 steps, one non-interior launch, e + spl == total - 1", 65, 3, 1, tight=True),
    Sliced("skein512", 16512, 64, "output-only last launch behind a non-interior one", 44, 1, 2, output_only=True),
    Sliced("skein512", 32768, 64, "e + spl == total - 1 at 10-step slices", 52, 3, 1, tight=True),
    Sliced("skein512", 65472, None, "total 1024, 8 equal slices of 128", 8, 128, 1),
    Sliced("skein512", 65536, 100000, "513 launches, output-only last", 513, 1, 2, tight=True, output_only=True),
    Sliced("skein", 8160, None, "smallest sliced message (total 256)", 8, 32, 8),
    Sliced("skein", 8160, 1, "smallest sliced message (total 256), one launch", 1, 256, 1),
    Sliced("skein", 8192, 64, "output-only last launch (total % 4 == 1)", 33, 1, 33, output_only=True),
    Sliced("skein", 8224, None, "total % 4 == 2, last slice 6 steps", 8, 6, 8),
    Sliced("skein", 8256, 7, "total % 4 == 3, last slice 19 steps", 7, 19, 7),
    Sliced("skein", 8288, 100000, "total % 4 == 0, one-line slices", 65, 4, 65),
    Sliced("skein", 65504, None, "total 2048, equal slices", 8, 256, 8),
    Sliced("skein", 65536, 100000, "513 launches, output-only last", 513, 1, 513, output_only=True),
)


@dataclass(frozen=True)
class Threshold:
    alg: str
    block_bytes: int
    nblocks: int
    sliced: bool
    edge: str

    def __str__(self):
        return f"{self.alg} {self.block_bytes} x {self.nblocks}"


THRESHOLD = tuple(
    t for alg in ("skein512", "skein") for t in (
        Threshold(alg, SLICED_FLOOR[alg], 4095, False, "one block below the floor: the line kernel"),
        Threshold(alg, SLICED_FLOOR[alg], 4096, True, "exactly at the floor of blocks"),
        Threshold(alg, SLICED_FLOOR[alg] - STEP[alg], NBLOCKS_SLICED, False, "one step below the floor: the line kernel")))

# the (alg, block_bytes) whose digests the sliced tests need, each with the most blocks any call of it hashes
SLICED_SHAPES = tuple(sorted({(r.alg, r.block_bytes) for r in SLICED} | {(t.alg, t.block_bytes) for t in THRESHOLD}))


# ---- the kernels the sets exist to reach, as cw_profile_kernels names them ----------------------------------------------------------
KERNELS_ONE_LAUNCH = tuple(
    [f"cw::skein_blocks_kernel<{nw}, {a}>" for nw in (8, 4) for a in ("true, false", "true, true", "false, true")] +
    [f"cw::skein_lines_kernel<{nw}, {a}>" for nw in (8, 4) for a in ("true", "false")] +
    [f"cw::sha256_blocks_kernel<{a}, {r}>" for a in ("true", "false") for r in ("true", "false")])
KERNELS_SLICED = ("cw::skein_slice_kernel<8, true, true> + cw::skein_slice_kernel<8, true, false>", "cw::skein_slice_kernel<8, true, false>",
                  "cw::skein_slice_kernel<4, true, false>")
KERNELS_CHUNKS = ("cw::skein_chunks_kernel<8>", "cw::skein_chunks_kernel<4>", "cw::sha256_chunks_kernel")
KERNELS = KERNELS_ONE_LAUNCH + KERNELS_SLICED + KERNELS_CHUNKS
# the knob sets every one-launch call runs under
KNOB_SETS = (dict(), dict(CW_SKEIN_MODE="steps"), dict(CW_SKEIN_MODE="lines"), dict(CW_SKEIN_SLICED=0))


# ---- the oracle's digests ------------------------------------------------------------------------------------------------------------
def digests_of(oracle, alg: str, blocks: np.ndarray, length: int, threads: int = 16) -> np.ndarray:
    """[n, DIGEST[alg]] uint8: the oracle's digests of the n messages of `length` bytes that lie end to end in `blocks`, one batch."""
    hid = {"skein512": oracle.HASH_SKEIN512, "skein": oracle.HASH_SKEIN256_128, "sha256": oracle.HASH_SHA256}[alg]
    if length == 0:
        one = {"skein512": oracle.skein512, "skein": oracle.skein256, "sha256": oracle.sha256}[alg](b"")
        return np.frombuffer(one, np.uint8).reshape(1, -1)
    return oracle.hash_and_compress(np.ascontiguousarray(blocks).reshape(-1), length, hid, oracle.COMP_NONE, threads=threads)[1]
