"""Host-side mirror of the reference's operator interface over the C ABI.

Names follow the reference: ``do_hashing(src, dst, count)`` / ``do_compression(src, dst, len)`` are the two
function slots of src/hashandcompress/HashAndCompress.cpp:111,119; ``HashOffload`` is HashOffload.h:13-64.
The ``dev_*`` functions take raw device pointers (ints, e.g. ``torch.Tensor.data_ptr()``) and a HIP stream
handle; torch is only ever used by callers for memory and streams, never here.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import COMP_LZ4, COMP_LZF, COMP_NONE, HASH_NONE, HASH_SKEIN256_128, HASH_SKEIN512, HASH_SHA256, check, lib

_HASH_NAMES = {"skein": HASH_SKEIN256_128, "skein512": HASH_SKEIN512, "sha256mb": HASH_SHA256, "sha256": HASH_SHA256}
_COMP_NAMES = {"lz4": COMP_LZ4, "lzf": COMP_LZF}


def _hash_id(alg) -> int:
    return _HASH_NAMES[alg] if isinstance(alg, str) else int(alg)


def _comp_id(alg) -> int:
    return _COMP_NAMES[alg] if isinstance(alg, str) else int(alg)


def init(device: int = 0) -> None:
    """initializeGpu() (HashAndCompress.cpp:95-98)."""
    check(lib().cw_init(device))


def shutdown() -> None:
    lib().cw_shutdown()


def set_device(device: int) -> None:
    """The calling thread's device for its next calls (initialises it if needed)."""
    check(lib().cw_set_device(device))


def get_device() -> int:
    return int(lib().cw_get_device())


def device_count() -> int:
    return int(lib().cw_device_count())


def set_block_size(n: int) -> None:
    lib().cw_set_block_size(n)


def digest_bytes(alg) -> int:
    return int(lib().cw_digest_bytes(_hash_id(alg)))


def compress_bound(alg, block_bytes: int) -> int:
    return int(lib().cw_compress_bound(_comp_id(alg), block_bytes))


def _np_u8(data) -> np.ndarray:
    if isinstance(data, np.ndarray):
        return np.ascontiguousarray(data.reshape(-1).view(np.uint8))
    return np.frombuffer(bytes(data), dtype=np.uint8)


# ---- the two slots -------------------------------------------------------------------------------
def do_hashing(alg, src, count: int, block_bytes: int | None = None) -> bytes:
    """doHashing(src, dst, count): `count` consecutive blocks -> `count` consecutive digests."""
    a = _np_u8(src)
    if block_bytes is not None:
        set_block_size(block_bytes)
    hid = _hash_id(alg)
    out = np.zeros(count * digest_bytes(hid), dtype=np.uint8)
    fn = {HASH_SKEIN256_128: lib().cw_hash_skein, HASH_SKEIN512: lib().cw_hash_skein512,
          HASH_SHA256: lib().cw_hash_sha256mb}[hid]
    if a.size < count * int(lib().cw_get_block_size()):
        raise ValueError("src shorter than count * block size")
    fn(a.ctypes.data, out.ctypes.data, count)
    return out.tobytes()


def do_compression(alg, src) -> bytes:
    """doCompression(src, dst, len) with the reference's dst capacity (2*len for lz4, len-1 for lzf);
    b'' when the codec reports 0 (did not fit)."""
    a = _np_u8(src)
    cid = _comp_id(alg)
    out = np.zeros(max(2 * a.size, 16), dtype=np.uint8)
    fn = lib().cw_compress_lz4 if cid == COMP_LZ4 else lib().cw_compress_lzf
    n = fn(a.ctypes.data, out.ctypes.data, a.size)
    return out[:n].tobytes()


# ---- batched host API ----------------------------------------------------------------------------
def hash_blocks(alg, src, block_bytes: int) -> np.ndarray:
    a = _np_u8(src)
    n = a.size // block_bytes if block_bytes else 0
    hid = _hash_id(alg)
    out = np.zeros((n, digest_bytes(hid)), dtype=np.uint8)
    check(lib().cw_hash_blocks(hid, a.ctypes.data, block_bytes, n, out.ctypes.data))
    return out


def hash_tree_blocks(alg, src, block_bytes: int, leaf: int, node: int, max_level: int):
    """Skein tree digests of every block of `src` (cw_hash_tree_blocks): [n, digest_bytes] uint8."""
    a = _np_u8(src)
    n = a.size // block_bytes if block_bytes else 0
    hid = _hash_id(alg)
    digests = np.zeros((n, digest_bytes(hid)), dtype=np.uint8)
    check(lib().cw_hash_tree_blocks(hid, a.ctypes.data, block_bytes, n, leaf, node, max_level, digests.ctypes.data))
    return digests


def dev_hash_tree(alg, d_src: int, block_bytes: int, nblocks: int, leaf: int, node: int, max_level: int, d_digests: int,
                  stream: int = 0, src_stride: int = 0) -> None:
    check(lib().cw_dev_hash_tree(_hash_id(alg), d_src, block_bytes, src_stride or block_bytes, nblocks, leaf, node, max_level,
                                 d_digests, stream))


def compress_blocks(alg, src, block_bytes: int):
    """Returns (sizes[n] uint32, payload[n, stride] uint8)."""
    a = _np_u8(src)
    n = a.size // block_bytes
    cid = _comp_id(alg)
    stride = compress_bound(cid, block_bytes)
    payload = np.zeros((n, stride), dtype=np.uint8)
    sizes = np.zeros(n, dtype=np.uint32)
    check(lib().cw_compress_blocks(cid, a.ctypes.data, block_bytes, n, payload.ctypes.data, stride, sizes.ctypes.data))
    return sizes, payload


def decompress_blocks(alg, sizes, payload, block_bytes: int):
    """Inverse of compress_blocks: (blocks[n, block_bytes] uint8, status[n] uint32; 0 = ok)."""
    payload = np.ascontiguousarray(payload, dtype=np.uint8)
    sizes = np.ascontiguousarray(sizes, dtype=np.uint32)
    n, stride = payload.shape
    out = np.zeros((n, block_bytes), dtype=np.uint8)
    status = np.ones(n, dtype=np.uint32)
    check(lib().cw_decompress_blocks(_comp_id(alg), payload.ctypes.data, stride, sizes.ctypes.data, n, out.ctypes.data,
                                     block_bytes, status.ctypes.data))
    return out, status


def do_decompression(alg, comp: bytes, cap: int) -> bytes:
    """LZ4_decompress_safe / lzf_decompress slot (experiment.cpp:118,256): b"" on a malformed slot."""
    src = np.frombuffer(comp, dtype=np.uint8)
    dst = np.zeros(cap, dtype=np.uint8)
    if _comp_id(alg) == 0:
        n = lib().cw_decompress_lz4(src.ctypes.data, dst.ctypes.data, len(comp), cap)
    else:
        n = lib().cw_decompress_lzf(src.ctypes.data, len(comp), dst.ctypes.data, cap)
    return dst[:n].tobytes() if n > 0 else b""


def hash_and_compress_blocks(hash_alg, comp_alg, src, block_bytes: int):
    """ProcessBlock (:231-261) over every block of `src`: (digests, sizes, payload)."""
    a = _np_u8(src)
    n = a.size // block_bytes
    hid, cid = _hash_id(hash_alg), _comp_id(comp_alg)
    stride = compress_bound(cid, block_bytes)
    digests = np.zeros((n, digest_bytes(hid)), dtype=np.uint8)
    payload = np.zeros((n, stride), dtype=np.uint8)
    sizes = np.zeros(n, dtype=np.uint32)
    check(lib().cw_hash_and_compress_blocks(hid, cid, a.ctypes.data, block_bytes, n, digests.ctypes.data,
                                            payload.ctypes.data, stride, sizes.ctypes.data))
    return digests, sizes, payload


def hash_and_compress_packed(hash_alg, comp_alg, src, block_bytes: int, pinned: bool = False):
    """cw_hash_and_compress_packed: (digests[n, db], sizes[n], offsets[n + 1], packed[total] uint8).  pinned=True takes the
    input and the packed output through page-locked buffers (cw_host_alloc), the zero-copy form of the pipeline."""
    a = _np_u8(src)
    n = a.size // block_bytes
    hid, cid = _hash_id(hash_alg), _comp_id(comp_alg)
    cap = max(n * compress_bound(cid, block_bytes), 1)
    digests = np.zeros((n, digest_bytes(hid)), dtype=np.uint8)
    sizes = np.zeros(n, dtype=np.uint32)
    offsets = np.zeros(n + 1, dtype=np.uint64)
    if pinned:
        hp, hs = lib().cw_host_alloc(cap), lib().cw_host_alloc(max(a.size, 1))
        if not hp or not hs:
            raise _lib.CwError(-5, lib().cw_last_error().decode())
        try:
            C.memmove(hs, a.ctypes.data, a.size)
            check(lib().cw_hash_and_compress_packed(hid, cid, hs, block_bytes, n, digests.ctypes.data, hp, cap, offsets.ctypes.data,
                                                    sizes.ctypes.data))
            packed = np.ctypeslib.as_array((C.c_uint8 * int(offsets[n])).from_address(hp)).copy() if offsets[n] else np.zeros(0, np.uint8)
        finally:
            lib().cw_host_free(hp)
            lib().cw_host_free(hs)
    else:
        buf = np.zeros(cap, dtype=np.uint8)
        check(lib().cw_hash_and_compress_packed(hid, cid, a.ctypes.data, block_bytes, n, digests.ctypes.data, buf.ctypes.data, cap,
                                                offsets.ctypes.data, sizes.ctypes.data))
        packed = buf[: int(offsets[n])].copy()
    return digests, sizes, offsets, packed


# ---- device-resident API (raw pointers) ------------------------------------------------------------
def dev_hash(alg, d_src: int, block_bytes: int, nblocks: int, d_digests: int, stream: int = 0,
             src_stride: int | None = None) -> None:
    check(lib().cw_dev_hash(_hash_id(alg), d_src, block_bytes, src_stride or block_bytes, nblocks, d_digests, stream))


def dev_compress(alg, d_src: int, block_bytes: int, nblocks: int, d_dst: int, dst_stride: int, d_sizes: int,
                 stream: int = 0, src_stride: int | None = None) -> None:
    check(lib().cw_dev_compress(_comp_id(alg), d_src, block_bytes, src_stride or block_bytes, nblocks, d_dst, dst_stride,
                                d_sizes, stream))


def dev_hash_and_compress(hash_alg, comp_alg, d_src: int, block_bytes: int, nblocks: int, d_digests: int, d_dst: int,
                          dst_stride: int, d_sizes: int, stream: int = 0, src_stride: int | None = None) -> None:
    check(lib().cw_dev_hash_and_compress(_hash_id(hash_alg), _comp_id(comp_alg), d_src, block_bytes,
                                         src_stride or block_bytes, nblocks, d_digests, d_dst, dst_stride, d_sizes, stream))


def dev_decompress(alg, d_comp: int, comp_stride: int, d_sizes: int, nblocks: int, d_dst: int, block_bytes: int,
                   d_status: int, stream: int = 0) -> None:
    check(lib().cw_dev_decompress(_comp_id(alg), d_comp, comp_stride, d_sizes, nblocks, d_dst, block_bytes, d_status, stream))


def dev_pack(d_slots: int, slot_stride: int, d_sizes: int, nblocks: int, d_packed: int, d_offsets: int, stream: int = 0) -> None:
    """Packed stream + u64 block index (nblocks + 1 offsets) from fixed-stride slots; d_packed = 0: index only."""
    check(lib().cw_dev_pack(d_slots, slot_stride, d_sizes, nblocks, d_packed or None, d_offsets, stream))


def dev_gen_random(seed: int, first_block: int, nblocks: int, block_bytes: int, d_dst: int, stream: int = 0) -> None:
    check(lib().cw_dev_gen_random(seed, first_block, nblocks, block_bytes, d_dst, stream))


def dev_gen_mixed(seed: int, first_block: int, nblocks: int, block_bytes: int, d_dst: int, stream: int = 0) -> None:
    """SURVEY 8(d)'s compressible mix: even blocks random, odd blocks a 64-byte motif with 1/16 of the bytes mutated."""
    check(lib().cw_dev_gen_mixed(seed, first_block, nblocks, block_bytes, d_dst, stream))


def dev_sum_sizes(d_sizes: int, nblocks: int, raw_bytes: int, d_totals: int, stream: int = 0) -> None:
    check(lib().cw_dev_sum_sizes(d_sizes, nblocks, raw_bytes, d_totals, stream))


def profile_enable(on: bool = True) -> None:
    lib().cw_profile_enable(1 if on else 0)


def profile_read(reset: bool = True) -> dict:
    """{'codec': (ms_sum, launches), 'hash': ..., 'other': ...} from the library's own HIP events."""
    ms = (C.c_double * 3)()
    cnt = (C.c_uint * 3)()
    check(lib().cw_profile_read(ms, cnt, 1 if reset else 0))
    return {k: (ms[i], cnt[i]) for i, k in enumerate(("codec", "hash", "other"))}


def tune_set(key: str, value=None) -> None:
    """cw_tune_set: a knob's value for the calls that follow (None removes the override; the environment stays the default)."""
    check(lib().cw_tune_set(key.encode(), None if value is None else str(value).encode()))


def tune_reset() -> None:
    lib().cw_tune_reset()


class tuned:
    """with tuned(CW_LZ4_LANES=1, ...): the knobs hold inside the block and are removed afterwards."""

    def __init__(self, **knobs):
        self.knobs = knobs

    def __enter__(self):
        for k, v in self.knobs.items():
            tune_set(k, v)
        return self

    def __exit__(self, *exc):
        for k in self.knobs:
            tune_set(k, None)
        return False


def plan_describe(alg, block_bytes: int, nblocks: int, src_misalign: int = 0, dst_misalign: int = 0) -> str:
    """cw_plan_describe: what dev_compress would launch under the knobs as they are now -- line 1 as profile_kernels()["codec"]
    reports it afterwards, then one key=value line per field of the launch plan.  Needs no device."""
    buf = C.create_string_buffer(8192)
    check(lib().cw_plan_describe(_comp_id(alg), block_bytes, nblocks, src_misalign, dst_misalign, buf, 8192))
    return buf.value.decode()


def hash_plan_describe(alg, block_bytes: int, nblocks: int, src_misalign: int = 0, digest_misalign: int = 0, may_slice: bool = True) -> str:
    """cw_hash_plan_describe: what dev_hash would launch under the knobs as they are now -- line 1 as profile_kernels()["hash"]
    reports it afterwards, then one `slice=b..e interior=0|1` line per launch of a sliced Skein hash.  may_slice=False describes
    HashOffload, which never slices.  Needs no device."""
    cap = 1 << 16
    buf = C.create_string_buffer(cap)
    check(lib().cw_hash_plan_describe(_hash_id(alg), block_bytes, nblocks, src_misalign, digest_misalign, 1 if may_slice else 0, buf, cap))
    return buf.value.decode()


def profile_kernels() -> dict:
    """Names of the kernels the calling thread's latest codec / hash launch used (as rocprofv3 prints them)."""
    out = {}
    for i, k in enumerate(("codec", "hash")):
        buf = C.create_string_buffer(256)
        check(lib().cw_profile_kernels(i, buf, 256))
        out[k] = buf.value.decode()
    return out


# ---- dedupe index -------------------------------------------------------------------------------------
class DedupeIndex:
    """Device-resident fingerprint index of one hash algorithm (cw_dedupe_*): full digests, each with a 64-bit value.

    ``dev_dedupe`` is the batched lookup-or-insert, ``dev_hash_dedupe_compress`` hashes, dedupes and compresses only the
    new blocks.  Both take raw device pointers and a stream handle like the other ``dev_*`` functions; a full index raises
    ``CwError`` with code ``CW_ERR_NOMEM`` (-5) and is left unchanged: ``resize`` it and repeat the call.  ``dev_lookup`` only
    reads, ``dev_insert`` carries explicit values, ``dev_export`` / ``export`` / ``import_`` / ``save`` / ``load`` move the
    (digest, value) pairs out and in."""

    MISS = 2 ** 64 - 1  # CW_DEDUPE_MISS

    def __init__(self, hash_alg, max_entries: int):
        self.hash_alg = _hash_id(hash_alg)
        self._h = lib().cw_dedupe_create(self.hash_alg, max_entries)
        if not self._h:
            err = lib().cw_last_error().decode(errors="replace")
            raise _lib.CwError(-1 if "no HIP device" in err else -5 if "out of memory" in err else -2, err)
        self.max_entries = max_entries

    def _x(self):
        if not self._h:
            raise _lib.CwError(-4, "DedupeIndex is closed")
        return self._h

    def dev_dedupe(self, d_digests: int, nblocks: int, base: int, d_ref: int, d_new_idx: int, d_n_new: int, stream: int = 0) -> None:
        """ref[i] = value of block i's first occurrence (an earlier call's, else base + the lowest j of this call with the same
        digest); new_idx[0..n_new) = the new blocks in ascending order, inserted with value base + i; *d_n_new = n_new (u64)."""
        check(lib().cw_dev_dedupe(self._x(), d_digests, nblocks, base, d_ref, d_new_idx, d_n_new, stream))

    def dev_hash_dedupe_compress(self, comp_alg, d_src: int, block_bytes: int, nblocks: int, base: int, d_digests: int, d_ref: int,
                                 d_new_idx: int, d_dst: int, dst_stride: int, d_sizes: int, stream: int = 0,
                                 src_stride: int | None = None) -> int:
        """Digests of every block, dedupe, then the codec over the new blocks only: slot j of d_dst holds block new_idx[j].
        Synchronises the stream once; returns n_new."""
        n_new = C.c_size_t(0)
        check(lib().cw_dev_hash_dedupe_compress(self._x(), _comp_id(comp_alg), d_src, block_bytes, src_stride or block_bytes, nblocks,
                                                base, d_digests, d_ref, d_new_idx, d_dst, dst_stride, d_sizes, C.byref(n_new), stream))
        return int(n_new.value)

    def dev_cdc_dedupe_compress(self, params: "CdcParams", comp_alg, d_src: int, nbytes: int, final: bool, base: int, d_offsets: int,
                                max_offsets: int, d_nchunks: int, d_digests: int, d_ref: int, d_new_idx: int, d_n_new: int, d_dst: int,
                                dst_bytes: int, d_sizes: int, stream: int = 0) -> int:
        """Chunk, hash and dedupe d_src[0..nbytes), then compress only the new chunks into their slots (chunk_slot_offset); d_sizes[j]
        belongs to chunk new_idx[j].  Synchronises the stream once, for the chunk count it returns; n_new stays on the device.  A full
        index raises CwError -5 with ``e.nchunks`` set."""
        k = C.c_size_t(0)
        rc = lib().cw_dev_cdc_dedupe_compress(self._x(), C.byref(params), _comp_id(comp_alg), d_src, nbytes, 1 if final else 0, base,
                                              d_offsets, max_offsets, d_nchunks, d_digests, d_ref, d_new_idx, d_n_new, d_dst, dst_bytes,
                                              d_sizes, C.byref(k), stream)
        if rc != 0:
            err = _lib.CwError(rc, lib().cw_last_error().decode(errors="replace"))
            err.nchunks = int(k.value)
            raise err
        return int(k.value)

    def dev_cdc_streams_dedupe_compress(self, params: "CdcParams", comp_alg, d_src: int, nbytes: int, d_ends: int, nstreams: int, base: int,
                                        d_offsets: int, max_offsets: int, d_nchunks: int, d_stream_first: int, d_result: int, d_digests: int,
                                        d_ref: int, d_new_idx: int, d_n_new: int, d_dst: int, dst_bytes: int, d_sizes: int,
                                        stream: int = 0) -> int:
        """``dev_cdc_dedupe_compress`` over many streams in one buffer (``dev_cdc_streams``): every stream gets its own cuts, chunk i of
        the buffer carries value base + i, and stream f's chunks are positions [first[f], first[f + 1]).  max_offsets >=
        ``params.max_offsets_streams(nbytes, nstreams)``.  Synchronises the stream once; returns the chunk count.  Refused ends raise
        CwError -2 with nothing inserted; a full index raises CwError -5 with ``e.nchunks`` set."""
        k = C.c_size_t(0)
        rc = lib().cw_dev_cdc_streams_dedupe_compress(self._x(), C.byref(params), _comp_id(comp_alg), d_src or None, nbytes, d_ends or None,
                                                      nstreams, base, d_offsets, max_offsets, d_nchunks, d_stream_first, d_result, d_digests,
                                                      d_ref, d_new_idx, d_n_new, d_dst, dst_bytes, d_sizes, C.byref(k), stream)
        if rc != 0:
            err = _lib.CwError(rc, lib().cw_last_error().decode(errors="replace"))
            err.nchunks = int(k.value)
            raise err
        return int(k.value)

    def dev_cdc_streams_part_dedupe_compress(self, params: "CdcParams", comp_alg, d_src: int, nbytes: int, d_ends: int, nstreams: int,
                                             final: bool, base: int, d_offsets: int, max_offsets: int, d_nchunks: int, d_stream_first: int,
                                             d_result: int, d_digests: int, d_ref: int, d_new_idx: int, d_n_new: int, d_dst: int,
                                             dst_bytes: int, d_sizes: int, stream: int = 0) -> int:
        """``dev_cdc_streams_dedupe_compress`` with ``dev_cdc_streams_part`` as its chunker (``final`` behind nstreams): with final =
        False only the chunks in front of the bytes consumed are hashed, inserted and compressed.  Raises as that call does."""
        k = C.c_size_t(0)
        rc = lib().cw_dev_cdc_streams_part_dedupe_compress(self._x(), C.byref(params), _comp_id(comp_alg), d_src or None, nbytes, d_ends or None,
                                                           nstreams, 1 if final else 0, base, d_offsets, max_offsets, d_nchunks, d_stream_first,
                                                           d_result, d_digests, d_ref, d_new_idx, d_n_new, d_dst, dst_bytes, d_sizes,
                                                           C.byref(k), stream)
        if rc != 0:
            err = _lib.CwError(rc, lib().cw_last_error().decode(errors="replace"))
            err.nchunks = int(k.value)
            raise err
        return int(k.value)

    def dev_lookup(self, d_digests: int, n: int, d_ref: int, d_n_found: int, stream: int = 0) -> None:
        """Read-only: ref[i] = the stored value of digest i or ``MISS``; *d_n_found = hits (u64).  The index is unchanged."""
        check(lib().cw_dev_dedupe_lookup(self._x(), d_digests, n, d_ref, d_n_found, stream))

    def dev_insert(self, d_digests: int, d_values: int, n: int, d_ref: int, d_new_idx: int, d_n_new: int, stream: int = 0) -> None:
        """``dev_dedupe`` with explicit values: block i carries values[i] (u64); the lowest index of a digest wins, stored entries keep
        their value."""
        check(lib().cw_dev_dedupe_insert(self._x(), d_digests, d_values, n, d_ref, d_new_idx, d_n_new, stream))

    def dev_export(self, d_digests: int, d_values: int, max_out: int, d_n: int, stream: int = 0) -> None:
        """The entries as parallel device arrays: *d_n = the entry count (u64), min(*d_n, max_out) pairs written."""
        check(lib().cw_dev_dedupe_export(self._x(), d_digests, d_values, max_out, d_n, stream))

    def dev_export_live(self, d_live: int, dir_base: int, dir_entries: int, d_digests: int, d_values: int, max_out: int, d_result: int,
                        stream: int = 0) -> None:
        """The digests behind the directory entries d_live (u32[dir_entries]) flags, in ascending value: d_values[k] = dir_base + idx
        of the k-th flagged idx with its digest, or ``MISS`` and a zero digest when the index has no entry with that value;
        d_result = {flagged entries, index entries with a flagged value}; min(flagged, max_out) slots written.  The index is unchanged."""
        check(lib().cw_dev_dedupe_export_live(self._x(), d_live, dir_base, dir_entries, d_digests or None, d_values or None, max_out, d_result,
                                              stream))

    def dev_revalue(self, d_from: int, d_to: int, d_npairs: int, max_pairs: int, range_base: int, range_entries: int, d_result: int,
                    stream: int = 0) -> None:
        """Every entry whose value is d_from[k] (ascending, k < min(*d_npairs, max_pairs)) gets the value d_to[k], in place: no
        rehash, the count and the keys stay.  An entry with a value of [range_base, range_base + range_entries) that no pair names is
        stale.  d_result[0..3) = verdict (1: an entry is stale, no value changed), entries translated, stale entries.  Not
        synchronised."""
        check(lib().cw_dev_dedupe_revalue(self._x(), d_from, d_to, d_npairs, max_pairs, range_base, range_entries, d_result, stream))

    def resize(self, max_entries: int) -> None:
        """Rebuild the table for ``max_entries`` (synchronous; at least ``count()``).  Every lookup answers as before."""
        check(lib().cw_dedupe_resize(self._x(), max_entries))
        n = C.c_size_t(0)
        check(lib().cw_dedupe_max_entries(self._x(), C.byref(n)))
        self.max_entries = int(n.value)

    def retain(self, d_live: int, dir_base: int, dir_entries: int, max_entries: int | None = None) -> int:
        """Rebuild the table with only the entries whose value names no entry of [dir_base, dir_base + dir_entries) or one whose
        flag d_live[value - dir_base] (u32, device memory, complete when the call is made) is set; returns how many were removed.
        Synchronous; ``max_entries`` (default: as it is) must hold the kept entries, else CwError -2 and the index is unchanged."""
        removed = C.c_uint64(0)
        check(lib().cw_dedupe_retain(self._x(), d_live, dir_base, dir_entries, max_entries or 0, C.byref(removed)))
        n = C.c_size_t(0)
        check(lib().cw_dedupe_max_entries(self._x(), C.byref(n)))
        self.max_entries = int(n.value)
        return int(removed.value)

    def set_stage_entries(self, entries: int) -> None:
        """Pairs per piece of ``export`` / ``import_`` (0 = the default); for tests."""
        check(lib().cw_dedupe_set_stage_entries(self._x(), entries))

    def export(self):
        """Every entry on the host: (digests uint8[n, digest_bytes], values uint64[n]), in an unspecified order."""
        db = digest_bytes(self.hash_alg)
        n = self.count()
        while True:
            dig, val, got = np.empty((n, db), np.uint8), np.empty(n, np.uint64), C.c_size_t(0)
            check(lib().cw_dedupe_export(self._x(), dig.ctypes.data, val.ctypes.data, n, C.byref(got)))
            if got.value <= n:  # (another thread may have inserted in between)
                return dig[:got.value], val[:got.value]
            n = int(got.value)

    def import_(self, digests, values) -> int:
        """Insert the pairs in order (entries already stored keep their value); returns how many were new."""
        db = digest_bytes(self.hash_alg)
        dig = np.ascontiguousarray(digests, dtype=np.uint8).reshape(-1, db)
        val = np.ascontiguousarray(values, dtype=np.uint64).reshape(-1)
        if len(dig) != len(val):
            raise ValueError(f"{len(dig)} digests, {len(val)} values")
        k = C.c_size_t(0)
        check(lib().cw_dedupe_import(self._x(), dig.ctypes.data, val.ctypes.data, len(val), C.byref(k)))
        return int(k.value)

    def save(self, path) -> None:
        """Snapshot to ``path`` (numpy.savez): hash algorithm id, max_entries, digests, values."""
        dig, val = self.export()
        with open(path, "wb") as f:
            np.savez(f, hash_alg=np.int64(self.hash_alg), max_entries=np.int64(self.max_entries), digests=dig, values=val)

    @classmethod
    def load(cls, path, max_entries: int | None = None) -> "DedupeIndex":
        """A new index from a snapshot; ``max_entries`` defaults to the saved one and must hold every saved entry."""
        with np.load(path) as z:
            alg, saved, dig, val = int(z["hash_alg"]), int(z["max_entries"]), z["digests"], z["values"]
        want = saved if max_entries is None else max_entries
        if want < len(val):
            raise _lib.CwError(-2, f"max_entries {want} < {len(val)} saved entries")
        idx = cls(alg, want)
        try:
            idx.import_(dig, val)
        except Exception:
            idx.close()
            raise
        return idx

    def count(self) -> int:
        """Entries in the index (waits for the index's last call)."""
        n = C.c_uint64(0)
        check(lib().cw_dedupe_count(self._x(), C.byref(n)))
        return int(n.value)

    def close(self) -> None:
        if self._h:
            lib().cw_dedupe_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- HashOffload ------------------------------------------------------------------------------------
class HashOffload:
    """HashOffload.h:13-64: Reset(data, results, onComplete) -> Enqueue() -> Start() -> Complete()."""

    hInit, hQueued, hOffloaded, hComplete, hFailed = 0, 1, 2, 3, 4

    def __init__(self, n_blocks: int, alg="skein", block_bytes: int = 4096):
        self._h = lib().cw_offload_create(_hash_id(alg), n_blocks, block_bytes)
        if not self._h:
            raise _lib.CwError(-2, lib().cw_last_error().decode())
        self.n_blocks, self.block_bytes, self.alg = n_blocks, block_bytes, _hash_id(alg)
        self._keep = None

    def Reset(self, data: np.ndarray, results: np.ndarray, on_complete=None) -> None:
        cb = _lib.ON_COMPLETE((lambda _arg: on_complete()) if on_complete else (lambda _arg: None))
        self._keep = (data, results, cb)
        check(lib().cw_offload_reset(self._h, data.ctypes.data, results.ctypes.data, cb, None))

    def Enqueue(self) -> None:
        check(lib().cw_offload_enqueue(self._h))

    def Start(self) -> None:
        check(lib().cw_offload_start(self._h))

    def Complete(self) -> None:
        check(lib().cw_offload_complete(self._h))

    def Completed(self) -> bool:
        return bool(lib().cw_offload_completed(self._h))

    def DoOffload(self) -> None:
        check(lib().cw_offload_do(self._h))

    def Submit(self) -> None:
        """Enqueue + hand to the offload thread (hashing_offload_entry_point, :160-183)."""
        check(lib().cw_offload_submit(self._h))

    @property
    def state(self) -> int:
        return int(lib().cw_offload_state(self._h))

    @property
    def error(self) -> int:
        """CW_OK, or the status code that put the object into hFailed."""
        return int(lib().cw_offload_error(self._h))

    def close(self) -> None:
        if self._h:
            lib().cw_offload_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- content-defined chunking (cw_cdc_*) --------------------------------------------------------
class CdcParams(C.Structure):
    """cw_cdc_params: min / normal / max chunk sizes, the two masks and an optional 256-entry gear table (None = default)."""
    _fields_ = [("min_size", C.c_uint32), ("normal_size", C.c_uint32), ("max_size", C.c_uint32), ("reserved", C.c_uint32),
                ("mask_s", C.c_uint64), ("mask_l", C.c_uint64), ("gear", C.POINTER(C.c_uint64))]

    def __init__(self, min_size: int | None = None, normal_size: int = 8192, max_size: int | None = None, mask_s: int | None = None,
                 mask_l: int | None = None, gear=None):
        """A field left at None takes the value cw_cdc_default_params gives for normal_size: CdcParams() is the 8 KiB default."""
        lg = normal_size.bit_length() - 1

        def top(k):
            return ((1 << 64) - 1) ^ ((1 << (64 - k)) - 1) if k > 0 else 0

        super().__init__(normal_size // 4 if min_size is None else min_size, normal_size, normal_size * 8 if max_size is None else max_size,
                         0, top(lg + 2) if mask_s is None else mask_s, top(lg - 2) if mask_l is None else mask_l, None)
        self.set_gear(gear)

    def set_gear(self, gear) -> None:
        if gear is None:
            self._gear = None
            self.gear = C.POINTER(C.c_uint64)()
        else:
            self._gear = np.ascontiguousarray(np.asarray(gear, dtype=np.uint64).reshape(256))
            self.gear = self._gear.ctypes.data_as(C.POINTER(C.c_uint64))

    @classmethod
    def default(cls, normal_size: int) -> "CdcParams":
        p = cls()
        lib().cw_cdc_default_params(C.byref(p), normal_size)
        p._gear = None
        return p

    def max_offsets(self, nbytes: int) -> int:
        return nbytes // self.min_size + 2

    def max_offsets_streams(self, nbytes: int, nstreams: int) -> int:
        return nbytes // self.min_size + nstreams + 1


def dev_cdc(params: CdcParams, d_src: int, nbytes: int, final: bool, d_offsets: int, max_offsets: int, d_nchunks: int,
            stream: int = 0) -> None:
    """Cuts of d_src[0..nbytes): d_offsets[0..K] (u64) and *d_nchunks = K, on the device, queued on `stream`."""
    check(lib().cw_dev_cdc(C.byref(params), d_src, nbytes, 1 if final else 0, d_offsets, max_offsets, d_nchunks, stream))


def dev_cdc_streams(params: CdcParams, d_src: int, nbytes: int, d_ends: int, nstreams: int, d_offsets: int, max_offsets: int, d_nchunks: int,
                    d_stream_first: int, d_result: int, stream: int = 0) -> None:
    """Cuts of the streams d_src[ends[f-1] .. ends[f]) (u64 ends on the device, the last = nbytes), each as ``dev_cdc`` cuts it alone:
    d_offsets[0..K], *d_nchunks = K, d_stream_first[0..nstreams] (stream f = chunks [first[f], first[f + 1])) and *d_result = 1 when
    the ends were refused (then K = 0).  Queued on `stream`, not synchronised."""
    check(lib().cw_dev_cdc_streams(C.byref(params), d_src or None, nbytes, d_ends or None, nstreams, d_offsets, max_offsets, d_nchunks,
                                   d_stream_first, d_result, stream))


def dev_cdc_streams_part(params: CdcParams, d_src: int, nbytes: int, d_ends: int, nstreams: int, final: bool, d_offsets: int, max_offsets: int,
                         d_nchunks: int, d_stream_first: int, d_result: int, stream: int = 0) -> None:
    """``dev_cdc_streams`` over a piece of a longer run: final = True is ``dev_cdc_streams``; final = False leaves the last stream
    [ends[nstreams - 2], nbytes) open, cut as ``dev_cdc(final=False)`` cuts it alone: d_offsets[K] = the bytes consumed, and
    d_stream_first[nstreams - 1] = K when nothing of the open stream was consumed.  Queued on `stream`, not synchronised."""
    check(lib().cw_dev_cdc_streams_part(C.byref(params), d_src or None, nbytes, d_ends or None, nstreams, 1 if final else 0, d_offsets,
                                        max_offsets, d_nchunks, d_stream_first, d_result, stream))


def dev_hash_chunks(hash_alg, d_src: int, src_bytes: int, d_offsets: int, d_nchunks: int, max_chunks: int, d_digests: int,
                    stream: int = 0) -> None:
    """Digest of every chunk [offsets[i], offsets[i+1]) for i < min(*d_nchunks, max_chunks), at d_digests + i * digest size."""
    check(lib().cw_dev_hash_chunks(_hash_id(hash_alg), d_src, src_bytes, d_offsets, d_nchunks, max_chunks, d_digests, stream))


def cdc_hash(params: CdcParams, data, hash_alg=None):
    """Host form: (offsets u64 array of K + 1 cuts, digests as a (K, digest bytes) uint8 array, or None without hash_alg)."""
    a = _np_u8(data)
    hid = HASH_NONE if hash_alg is None else _hash_id(hash_alg)
    cap = params.max_offsets(a.size)
    offs = np.zeros(cap, dtype=np.uint64)
    db = digest_bytes(hid) if hid != HASH_NONE else 0
    dig = np.zeros((cap, max(db, 1)), dtype=np.uint8)
    k = C.c_size_t(0)
    check(lib().cw_cdc_hash(C.byref(params), hid, a.ctypes.data, a.size, offs.ctypes.data, cap, C.byref(k),
                            dig.ctypes.data if db else None))
    k = int(k.value)
    return offs[:k + 1].copy(), (dig[:k, :db].copy() if db else None)


# ---- codecs over chunks (cw_dev_*_chunks) --------------------------------------------------------
def chunk_slot_offset(comp_alg, o: int, i: int) -> int:
    """Where compressed chunk i of input offset o lies in the slot buffer: LZ4 (o + o // 255 + 32 * i) & ~15, LZF o."""
    return o if _comp_id(comp_alg) == COMP_LZF else (o + o // 255 + 32 * i) & ~15


def chunk_slots_bytes(comp_alg, src_bytes: int, max_chunks: int) -> int:
    """Bytes of slot buffer dev_compress_chunks needs for src_bytes of input in at most max_chunks chunks."""
    return chunk_slot_offset(comp_alg, src_bytes, max_chunks) + 16


def dev_compress_chunks(comp_alg, d_src: int, src_bytes: int, d_offsets: int, d_nchunks: int, max_chunks: int, d_dst: int, dst_bytes: int,
                        d_sizes: int, stream: int = 0, d_sel: int = 0, d_nsel: int = 0) -> None:
    """Compress chunk i = [offsets[i], offsets[i+1]) into its slot for every i < min(*d_nchunks, max_chunks), or for the chunks
    d_sel[j], j < min(*d_nsel, max_chunks); d_sizes[j] is the size of position j (0: LZF did not fit, or out of contract)."""
    check(lib().cw_dev_compress_chunks(_comp_id(comp_alg), d_src, src_bytes, d_offsets, d_nchunks, max_chunks, d_sel or None,
                                       d_nsel or None, d_dst, dst_bytes, d_sizes, stream))


def dev_pack_chunks(comp_alg, d_slots: int, d_offsets: int, d_count: int, max_count: int, d_sizes: int, d_packed: int,
                    d_packed_offsets: int, stream: int = 0, d_sel: int = 0) -> None:
    """Packed stream of the positions j < min(*d_count, max_count): d_packed_offsets[0..n] and, unless d_packed is 0, the bytes."""
    check(lib().cw_dev_pack_chunks(_comp_id(comp_alg), d_slots, d_offsets, d_sel or None, d_count, max_count, d_sizes, d_packed or None,
                                   d_packed_offsets, stream))


def dev_decompress_chunks(comp_alg, d_comp: int, d_comp_offsets: int, d_raw_offsets: int, d_count: int, max_count: int, d_dst: int,
                          dst_bytes: int, d_status: int, stream: int = 0) -> None:
    """Decode position j's compressed extent into its raw extent of d_dst; d_status[j] = 0 iff well formed and exactly that long."""
    check(lib().cw_dev_decompress_chunks(_comp_id(comp_alg), d_comp, d_comp_offsets, d_raw_offsets, d_count, max_count, d_dst, dst_bytes,
                                         d_status, stream))


# ---- the chunk store (cw_dev_store_chunks / cw_dev_restore_chunks) ---------------------------------
class ChunkLoc(C.Structure):
    """cw_chunk_loc: where a chunk lies in the store.  All zero = no such chunk."""
    _fields_ = [("pos", C.c_uint64), ("stored", C.c_uint32), ("raw", C.c_uint32)]
    RAW = 0x80000000  # CW_CHUNK_RAW: stored uncompressed; bits 0..16 of ``raw`` are the chunk's length


def dev_store_chunks(comp_alg, d_src: int, src_bytes: int, d_offsets: int, d_nchunks: int, max_chunks: int, d_slots: int, d_sizes: int,
                     base: int, d_store: int, store_bytes: int, d_used: int, d_dir: int, dir_base: int, dir_entries: int, d_result: int,
                     stream: int = 0, d_sel: int = 0, d_nsel: int = 0) -> None:
    """Append the chunks of one dev_compress_chunks / dev_cdc_dedupe_compress call (same arguments, d_slots = its d_dst) to the
    store (d_store, *d_used, d_dir); chunk i gets the entry d_dir[base + i - dir_base].  d_result[0] = 0, or 1 (does not fit) /
    2 (an entry outside the directory) with nothing changed; d_result[1] = the bytes the call needs.  Not synchronised."""
    check(lib().cw_dev_store_chunks(_comp_id(comp_alg), d_src or None, src_bytes, d_offsets, d_nchunks, max_chunks, d_sel or None,
                                    d_nsel or None, d_slots, d_sizes, base, d_store or None, store_bytes, d_used, d_dir, dir_base,
                                    dir_entries, d_result, stream))


def dev_restore_chunks(comp_alg, d_store: int, store_bytes: int, d_dir: int, dir_base: int, dir_entries: int, d_ref: int,
                       d_raw_offsets: int, d_count: int, max_count: int, d_dst: int, dst_bytes: int, d_status: int, stream: int = 0) -> None:
    """Position j < min(*d_count, max_count): the chunk of value d_ref[j] into d_dst[raw_offsets[j] .. raw_offsets[j+1]);
    d_status[j] = 0 restored, 1 stored bytes malformed, 2 refused (no such entry, or it does not match the extent or the store)."""
    check(lib().cw_dev_restore_chunks(_comp_id(comp_alg), d_store or None, store_bytes, d_dir, dir_base, dir_entries, d_ref,
                                      d_raw_offsets, d_count, max_count, d_dst or None, dst_bytes, d_status, stream))


def dev_read_ranges(comp_alg, d_store: int, store_bytes: int, d_dir: int, dir_base: int, dir_entries: int, d_ref: int, d_raw_offsets: int,
                    d_count: int, max_count: int, d_range_off: int, d_range_len: int, d_range_dst: int, d_nranges: int, max_ranges: int,
                    d_dst: int, dst_bytes: int, d_status: int, stream: int = 0) -> None:
    """Range k < min(*d_nranges, max_ranges): stream bytes [range_off[k], + range_len[k]) of the recipe (dev_restore_chunks' arguments,
    in raw_offsets' coordinates) into d_dst[range_dst[k] ..); d_status[k] = 0 read, 1 a touched chunk's stored bytes are malformed,
    2 a touched position is refused as dev_restore_chunks refuses it, 3 the range leaves the stream or the destination."""
    check(lib().cw_dev_read_ranges(_comp_id(comp_alg), d_store or None, store_bytes, d_dir, dir_base, dir_entries, d_ref, d_raw_offsets,
                                   d_count, max_count, d_range_off, d_range_len, d_range_dst, d_nranges, max_ranges, d_dst or None,
                                   dst_bytes, d_status, stream))


def dev_store_mark(d_ref: int, d_count: int, max_count: int, dir_base: int, dir_entries: int, d_live: int, d_n_outside: int,
                   stream: int = 0) -> None:
    """d_live[d_ref[j] - dir_base] = 1 (u32) for every position j < min(*d_count, max_count) that names a directory entry;
    *d_n_outside (u64) += the positions that name none.  The caller zeroes both first.  Not synchronised."""
    check(lib().cw_dev_store_mark(d_ref, d_count, max_count, dir_base, dir_entries, d_live, d_n_outside, stream))


def dev_store_compact(d_store: int, store_bytes: int, d_dir: int, dir_entries: int, d_live: int, d_new_store: int, new_store_bytes: int,
                      d_new_used: int, d_new_dir: int, d_result: int, stream: int = 0) -> None:
    """The flagged, non-zero entries' stored bytes back to back into d_new_store, their new places into d_new_dir (which may be
    d_dir), the total into *d_new_used.  d_result[0..4) = verdict (1: does not fit, 2: a kept entry is unsound; nothing changed
    then), kept bytes, kept entries, dropped entries.  d_new_store = 0 with new_store_bytes = 0 is a dry run.  Not synchronised."""
    check(lib().cw_dev_store_compact(d_store or None, store_bytes, d_dir, dir_entries, d_live, d_new_store or None, new_store_bytes,
                                     d_new_used, d_new_dir, d_result, stream))


def dev_store_renumber(d_dir: int, dir_base: int, dir_entries: int, d_live: int, new_base: int, d_new_dir: int, new_dir_base: int,
                       new_dir_entries: int, d_from: int, d_to: int, max_pairs: int, d_result: int, stream: int = 0) -> None:
    """The kept entries of d_dir (not all zero, and flagged by d_live unless that is 0) move bit for bit to the dense values
    [new_base, new_base + K) of d_new_dir, whose other entries become zero; d_from[k] / d_to[k] = the k-th kept entry's old / new
    value, ascending.  d_result[0..4) = verdict (2: the values leave the new directory or wrap, 1: K > max_pairs; nothing written
    then), K, new_base + K, non-zero entries not kept.  d_new_dir = 0 with new_dir_entries = 0 and d_from = d_to = 0 with
    max_pairs = 0 is a dry run.  Not synchronised."""
    check(lib().cw_dev_store_renumber(d_dir, dir_base, dir_entries, d_live or None, new_base, d_new_dir or None, new_dir_base, new_dir_entries,
                                      d_from or None, d_to or None, max_pairs, d_result, stream))


class StreamAccount(C.Structure):
    """cw_stream_account: what one stream of a ``dev_store_account`` call names, shares with no other stream and has in flagged chunks."""
    _fields_ = [(k, C.c_uint64) for k in ("positions", "missing", "logical_bytes", "unique_chunks", "unique_stored", "unique_raw",
                                          "flagged_positions", "flagged_bytes")]
    OWNER_NONE, OWNER_SHARED = 0xFFFFFFFF, 0xFFFFFFFE  # CW_OWNER_NONE, CW_OWNER_SHARED


ACCOUNT_DTYPE = np.dtype([(k, "<u8") for k, _ in StreamAccount._fields_])  # cw_stream_account as a numpy record


def dev_store_account(d_ref: int, d_first: int, nstreams: int, max_positions: int, d_dir: int, dir_base: int, dir_entries: int, d_flag: int,
                      d_acct: int, d_refcount: int, d_owner: int, d_totals: int, stream: int = 0) -> None:
    """Stream f = positions [d_first[f], d_first[f + 1]) of d_ref: d_acct[f] (cw_stream_account) = what it names, what no other
    stream of the call names and what lies in entries flagged by d_flag (u32 per entry, or 0); d_refcount[idx] / d_owner[idx] (u32,
    or 0) = the positions that name entry idx and the one stream that does (or OWNER_NONE / OWNER_SHARED).  d_totals[0..8) = verdict
    (1: d_first does not start at 0, decreases or ends above max_positions; nothing else written then), non-zero entries and their
    stored bytes, referenced entries and theirs, shared entries and theirs, missing positions.  Not synchronised."""
    check(lib().cw_dev_store_account(d_ref or None, d_first, nstreams, max_positions, d_dir, dir_base, dir_entries, d_flag or None, d_acct,
                                     d_refcount or None, d_owner or None, d_totals, stream))


def dev_store_export_chunks(d_store: int, store_bytes: int, d_dir: int, dir_base: int, dir_entries: int, d_values: int, d_count: int,
                            max_count: int, d_out: int, out_bytes: int, d_out_loc: int, d_result: int, stream: int = 0) -> None:
    """The stored bytes of the entries d_values[k], k < min(*d_count, max_count), back to back into d_out with d_out_loc[k] = where.
    d_result[0..3) = verdict (1: does not fit, 2: a position names no sound entry; nothing written then), total bytes, positions.
    d_out = 0 with out_bytes = 0 is a dry run.  Not synchronised."""
    check(lib().cw_dev_store_export_chunks(d_store or None, store_bytes, d_dir, dir_base, dir_entries, d_values, d_count, max_count,
                                           d_out or None, out_bytes, d_out_loc, d_result, stream))


def dev_store_import_chunks(d_in: int, in_bytes: int, d_in_loc: int, d_count: int, max_count: int, base: int, d_store: int, store_bytes: int,
                            d_used: int, d_dir: int, dir_base: int, dir_entries: int, d_result: int, stream: int = 0, d_sel: int = 0,
                            d_nsel: int = 0) -> None:
    """``dev_store_chunks`` for chunks in stored form: the selected chunks k of a bundle (d_in, d_in_loc) go behind *d_used, chunk k
    gets the entry d_dir[base + k - dir_base].  d_result[0] = 0, or 3 (a selected chunk is not in the bundle or its entry is
    unsound) / 1 (does not fit) / 2 (an entry outside the directory) with nothing changed; d_result[1] = the bytes.  Not synchronised."""
    check(lib().cw_dev_store_import_chunks(d_in or None, in_bytes, d_in_loc, d_count, max_count, d_sel or None, d_nsel or None, base,
                                           d_store or None, store_bytes, d_used, d_dir, dir_base, dir_entries, d_result, stream))


def dev_translate_refs(d_ref: int, d_count: int, max_count: int, d_from: int, d_to: int, d_npairs: int, max_pairs: int, d_out: int,
                       d_n_missing: int, stream: int = 0) -> None:
    """d_out[j] = d_to[k] where d_from[k] == d_ref[j] (d_from ascending), else ``MISS``; *d_n_missing (u64) += the misses.
    d_out may be d_ref.  Not synchronised."""
    check(lib().cw_dev_translate_refs(d_ref, d_count, max_count, d_from, d_to, d_npairs, max_pairs, d_out, d_n_missing, stream))


def dev_store_verify(index: "DedupeIndex", comp_alg, d_store: int, store_bytes: int, d_dir: int, dir_base: int, dir_entries: int, d_live: int,
                     d_cursor: int, d_work: int, work_bytes: int, d_status: int, d_totals: int, stream: int = 0) -> None:
    """One window of a scrub: the directory entries from *d_cursor (u64) on whose decoded chunks fit d_work, at
    most CW_SCRUB_ENTRIES of them, are decoded, hashed and compared with the digests ``index`` holds for their values.  d_status[idx]
    (u32) = 0 good, 1 malformed, 2 unsound entry, 3 digest mismatch, 4 no index entry carries the value, 5 not selected (all zero, or
    d_live[idx] == 0 when d_live is given); d_totals[0..8) (u64) += checked, ok, malformed, unsound, mismatch, orphan, raw bytes,
    windows; *d_cursor moves to the window's end.  A cursor at or past dir_entries writes nothing.  Not synchronised."""
    check(lib().cw_dev_store_verify(index._x(), _comp_id(comp_alg), d_store or None, store_bytes, d_dir, dir_base, dir_entries, d_live or None,
                                    d_cursor, d_work, work_bytes, d_status, d_totals, stream))


def dev_store_replace_chunks(d_in: int, in_bytes: int, d_in_loc: int, d_values: int, d_count: int, max_count: int, d_store: int,
                             store_bytes: int, d_used: int, d_dir: int, dir_base: int, dir_entries: int, d_result: int, stream: int = 0) -> None:
    """``dev_store_import_chunks`` with explicit values and no selection: position k's stored bytes go behind *d_used and
    d_dir[d_values[k] - dir_base] points at them.  d_result[0] = 0, or 3 (an incoming entry is unsound) / 1 (does not fit) / 2 (a value
    outside the directory) / 4 (the entry named has another length) with nothing changed; d_result[1] = the bytes.  Not synchronised."""
    check(lib().cw_dev_store_replace_chunks(d_in or None, in_bytes, d_in_loc, d_values, d_count, max_count, d_store or None, store_bytes,
                                            d_used, d_dir, dir_base, dir_entries, d_result, stream))


# ---- XOR guard stripes over the store's bytes (cw_dev_store_guard_*) --------------------------------------
def store_guard_bytes(store_bytes: int, stripe: int, group: int) -> int:
    """The guard bytes a store of store_bytes bytes needs: ceil(store_bytes / (group * stripe)) * stripe, or 0 when stripe is no power of
    two in [65536, 2^30] or group is not in [1, 256].  Host only."""
    if store_bytes < 0 or stripe < 0 or not 0 <= group < 1 << 32:
        return 0
    return int(lib().cw_store_guard_bytes(store_bytes, stripe, group))


def dev_store_guard_update(d_store: int, store_bytes: int, d_used: int, d_covered: int, stripe: int, group: int, d_guard: int, guard_bytes: int,
                           d_result: int, stream: int = 0) -> None:
    """Folds the store bytes [*d_covered, *d_used) into the guard, then *d_covered = *d_used.  d_result[0..4) = verdict (1: the cursors
    are inconsistent, nothing changed), from, to, the bytes folded.  Not synchronised."""
    check(lib().cw_dev_store_guard_update(d_store or None, store_bytes, d_used, d_covered, stripe, group, d_guard, guard_bytes, d_result, stream))


def dev_store_guard_check(d_store: int, store_bytes: int, d_covered: int, stripe: int, group: int, d_guard: int, guard_bytes: int, d_group_bad: int,
                          d_result: int, stream: int = 0) -> None:
    """Recomputes the guard over the store bytes [0, *d_covered) and compares.  d_result[0..4) = verdict (1: the cursor lies above
    store_bytes), the groups checked, the groups that differ, the lowest of them or 2^64 - 1; d_group_bad (u32 per group, or 0) gets a
    flag for every group checked.  Not synchronised."""
    check(lib().cw_dev_store_guard_check(d_store or None, store_bytes, d_covered, stripe, group, d_guard, guard_bytes, d_group_bad or None, d_result,
                                         stream))


def dev_store_guard_rebuild(d_store: int, store_bytes: int, d_dir: int, dir_base: int, dir_entries: int, d_covered: int, stripe: int, group: int,
                            d_guard: int, guard_bytes: int, d_values: int, d_count: int, max_count: int, d_out: int, out_bytes: int,
                            d_out_loc: int, d_status: int, d_result: int, stream: int = 0) -> None:
    """The stored bytes of the entries d_values[k], k < min(*d_count, max_count), rebuilt from the guard and the other bytes of their
    groups, back to back into d_out with d_out_loc[k] = where (all zero: not rebuilt).  d_status[k] (u32) = 0 rebuilt, 1 collides with
    another listed extent, 2 unprotected.  d_result[0..4) = verdict (1: does not fit, 2: the cursor lies above store_bytes; d_out and
    d_out_loc untouched then), total bytes, positions, positions rebuilt.  d_out = 0 with out_bytes = 0 is a dry run.  Not synchronised."""
    check(lib().cw_dev_store_guard_rebuild(d_store or None, store_bytes, d_dir, dir_base, dir_entries, d_covered, stripe, group, d_guard, guard_bytes,
                                           d_values, d_count, max_count, d_out or None, out_bytes, d_out_loc, d_status, d_result, stream))


# ---- the dual guard: P and the GF(2^8) syndrome Q beside it (cw_dev_store_guard2_*); group <= 255 ---------
def dev_store_guard2_update(d_store: int, store_bytes: int, d_used: int, d_covered: int, stripe: int, group: int, d_guard_p: int, d_guard_q: int,
                            guard_bytes: int, d_result: int, stream: int = 0) -> None:
    """``dev_store_guard_update`` for both syndromes: folds the store bytes [*d_covered, *d_used) into P and Q, then *d_covered =
    *d_used.  d_result[0..4) as there; the P bytes are what that call writes.  Not synchronised."""
    check(lib().cw_dev_store_guard2_update(d_store or None, store_bytes, d_used, d_covered, stripe, group, d_guard_p, d_guard_q, guard_bytes,
                                           d_result, stream))


def dev_store_guard2_check(d_store: int, store_bytes: int, d_covered: int, stripe: int, group: int, d_guard_p: int, d_guard_q: int, guard_bytes: int,
                           d_group_bad: int, d_result: int, stream: int = 0) -> None:
    """``dev_store_guard_check`` for both syndromes: d_group_bad (u32 per group, or 0) gets bit 0 when P differs and bit 1 when Q does;
    d_result[0..4) = verdict, the groups checked, the groups with any bit, the lowest of them or 2^64 - 1.  Not synchronised."""
    check(lib().cw_dev_store_guard2_check(d_store or None, store_bytes, d_covered, stripe, group, d_guard_p, d_guard_q, guard_bytes,
                                          d_group_bad or None, d_result, stream))


def dev_store_guard2_rebuild(d_store: int, store_bytes: int, d_dir: int, dir_base: int, dir_entries: int, d_covered: int, stripe: int, group: int,
                             d_guard_p: int, d_guard_q: int, guard_bytes: int, d_values: int, d_count: int, max_count: int, d_out: int,
                             out_bytes: int, d_out_loc: int, d_status: int, d_result: int, stream: int = 0) -> None:
    """``dev_store_guard_rebuild`` with the second syndrome: two listed extents that meet in a guard byte are both rebuilt, and
    d_status[k] = 1 only when three different listed bytes meet in one.  d_result[0..5) = verdict, total bytes, positions, positions
    rebuilt, the rebuilt positions that needed Q.  Not synchronised."""
    check(lib().cw_dev_store_guard2_rebuild(d_store or None, store_bytes, d_dir, dir_base, dir_entries, d_covered, stripe, group, d_guard_p, d_guard_q,
                                            guard_bytes, d_values, d_count, max_count, d_out or None, out_bytes, d_out_loc, d_status, d_result, stream))


# ---- which entries the syndromes suspect (cw_dev_store_guard_locate / cw_dev_store_guard2_locate) ---------
def dev_store_guard_locate(d_store: int, store_bytes: int, d_dir: int, dir_base: int, dir_entries: int, d_covered: int, stripe: int, group: int,
                           d_guard: int, guard_bytes: int, d_suspect: int, d_result: int, stream: int = 0) -> None:
    """d_suspect (u32 per directory entry) = 0, bit 1 when a byte of the entry's extent lies in a guard cell that differs (every such
    cell of the single guard is ambiguous), or exactly 4 for an entry that is not all zero and not protected.  d_result[0..8) =
    verdict (1: the cursor lies above the store, only d_result is written), the groups below the cursor, dirty cells, located cells
    (0 here), ambiguous cells, entries with bit 0 or 1, entries with value 4, 0.  d_suspect is d_live-shaped.  Not synchronised."""
    check(lib().cw_dev_store_guard_locate(d_store or None, store_bytes, d_dir, dir_base, dir_entries, d_covered, stripe, group, d_guard, guard_bytes,
                                          d_suspect, d_result, stream))


def dev_store_guard2_locate(d_store: int, store_bytes: int, d_dir: int, dir_base: int, dir_entries: int, d_covered: int, stripe: int, group: int,
                            d_guard_p: int, d_guard_q: int, guard_bytes: int, d_suspect: int, d_result: int, stream: int = 0) -> None:
    """``dev_store_guard_locate`` with both syndromes: a cell whose differences P', Q' are both non-zero with Q' = 2^m (x) P' for a
    member m below the cursor is LOCATED(m) -- one wrong store byte, in member m -- and sets bit 0 of the entries that hold that very
    byte; every other dirty cell is ambiguous and sets bit 1 of every entry with a byte in it.  Not synchronised."""
    check(lib().cw_dev_store_guard2_locate(d_store or None, store_bytes, d_dir, dir_base, dir_entries, d_covered, stripe, group, d_guard_p, d_guard_q,
                                           guard_bytes, d_suspect, d_result, stream))


class Store(C.Structure):
    """cw_store: the caller-owned triple of the chunk store (bytes, cursor, directory) as one argument."""
    _fields_ = [("d_store", C.c_void_p), ("store_bytes", C.c_size_t), ("d_used", C.c_void_p), ("d_dir", C.c_void_p),
                ("dir_base", C.c_uint64), ("dir_entries", C.c_size_t)]


class IngestStats(C.Structure):
    """cw_ingest_stats: one store_ingest call's bytes, chunks, new chunks, stored bytes and pieces, over the pieces that went in."""
    _fields_ = [("bytes", C.c_uint64), ("chunks", C.c_uint64), ("new_chunks", C.c_uint64), ("stored_bytes", C.c_uint64),
                ("pieces", C.c_uint64), ("reserved", C.c_uint64 * 3)]

    def as_dict(self) -> dict:
        return {k: int(getattr(self, k)) for k in ("bytes", "chunks", "new_chunks", "stored_bytes", "pieces")}


def store_ingest(index: "DedupeIndex", params: "CdcParams", comp_alg, store: Store, src: int, nbytes: int, base: int):
    """cw_store_ingest of the host bytes at address ``src``: (rc, refs, offsets, consumed, stats as a dict).  rc is 0, or -5 when a
    piece was refused: refs / offsets / consumed then cover the pieces before it.  Any other failure raises."""
    cap = params.max_offsets(nbytes)
    refs, offs = np.zeros(cap, np.uint64), np.zeros(cap, np.uint64)
    k, consumed, stats = C.c_size_t(0), C.c_size_t(0), IngestStats()
    rc = lib().cw_store_ingest(index._x(), C.byref(params), _comp_id(comp_alg), C.byref(store), src or None, nbytes, base, refs.ctypes.data,
                               offs.ctypes.data, cap, C.byref(k), C.byref(consumed), C.byref(stats))
    if rc not in (0, -5):
        check(rc)
    k = int(k.value)
    return rc, refs[:k].copy(), offs[:k + 1].copy(), int(consumed.value), stats.as_dict()


def dev_cdc_resync(d_new_offsets: int, d_new_count: int, max_new: int, d_old_offsets: int, d_old_count: int, max_old: int, new_from: int,
                   shift: int, keep_all: bool, d_result: int, stream: int = 0) -> None:
    """The device step of an edit: the smallest t in [1, N] with new[t] >= new_from and new[t] + shift (mod 2^64) an old cut old[s];
    d_result[0..4) = (0, t, s, new[t]) and *d_new_count = t, or (1, 0, 0, 0) with *d_new_count kept (keep_all) or zeroed.  Both
    counts are read on the device (N = min(*d_new_count, max_new), O = min(*d_old_count, max_old)).  Not synchronised."""
    check(lib().cw_dev_cdc_resync(d_new_offsets, d_new_count, max_new, d_old_offsets, d_old_count, max_old, new_from % (1 << 64),
                                  shift % (1 << 64), 1 if keep_all else 0, d_result, stream))


class PatchStats(C.Structure):
    """cw_patch_stats: one store_patch call's last window (bytes, kept chunks, new chunks, stored bytes), its attempts, and the old
    positions around the window: the first re-chunked one, the one the new recipe resumes at, and how many were reused."""
    _fields_ = [(k, C.c_uint64) for k in ("window_bytes", "window_chunks", "new_chunks", "stored_bytes", "attempts", "first_position",
                                          "resume_position", "reused_positions")]

    def as_dict(self) -> dict:
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


PATCH_DTYPE = np.dtype([(k, "<u8") for k, _ in PatchStats._fields_])  # cw_patch_stats as a numpy record


def store_patch(index: "DedupeIndex", params: "CdcParams", comp_alg, store: Store, refs, offsets, edit_off: int, remove_bytes: int, insert,
                base: int, lookahead: int = 0):
    """cw_store_patch: bytes [edit_off, edit_off + remove_bytes) of the stream of the recipe (refs, offsets) replaced by ``insert``.
    Returns (refs, offsets, stats as a dict) of the edited stream, offsets starting at 0; raises CwError (-5: not admitted, -2: a
    refused argument or a position that does not restore) with index, store and directory unchanged."""
    refs, offsets = np.ascontiguousarray(refs, np.uint64), np.ascontiguousarray(offsets, np.uint64)
    if len(offsets) != len(refs) + 1:
        raise ValueError(f"{len(refs)} refs need {len(refs) + 1} offsets, not {len(offsets)}")
    ins = _np_u8(insert)
    edited = int(offsets[-1] - offsets[0]) - remove_bytes + ins.size
    cap = params.max_offsets(max(edited, 0))
    out_refs, out_offs = np.zeros(cap, np.uint64), np.zeros(cap, np.uint64)
    k, stats = C.c_size_t(0), PatchStats()
    check(lib().cw_store_patch(index._x(), C.byref(params), _comp_id(comp_alg), C.byref(store), refs.ctypes.data if len(refs) else None,
                               offsets.ctypes.data, len(refs), edit_off, remove_bytes, ins.ctypes.data if ins.size else None, ins.size, base,
                               lookahead, out_refs.ctypes.data, out_offs.ctypes.data, cap, C.byref(k), C.byref(stats)))
    k = int(k.value)
    return out_refs[:k].copy(), out_offs[:k + 1].copy(), stats.as_dict()


# ---- recipe diff and deltas (cw_dev_recipe_diff / cw_dev_apply_delta) ------------------------------------
class DeltaOp(C.Structure):
    """cw_delta_op: B's bytes [b_off, b_off + len) are A's from a_off on (a copy) or the payload's from payload_off on (a new op);
    the other of the two is ``NONE``.  Offsets are zero-based."""
    _fields_ = [(k, C.c_uint64) for k in ("b_off", "len", "a_off", "payload_off")]
    NONE = (1 << 64) - 1  # CW_DELTA_NONE


DELTA_OP_DTYPE = np.dtype([(k, "<u8") for k, _ in DeltaOp._fields_])  # cw_delta_op as a numpy record


def dev_recipe_diff(d_ref_a: int, d_off_a: int, d_na: int, max_a: int, d_ref_b: int, d_off_b: int, d_nb: int, max_b: int, dir_base: int,
                    dir_entries: int, d_ops: int, max_ops: int, d_nops: int, d_totals: int, stream: int = 0, d_src: int = 0, d_new_off: int = 0,
                    d_new_len: int = 0, d_new_dst: int = 0, d_nnew: int = 0) -> None:
    """The ops that turn the stream of recipe A (d_ref_a, d_off_a, min(*d_na, max_a) positions) into that of recipe B, from the
    recipes alone: d_ops[0..*d_nops) (cw_delta_op), d_src[i] (or 0) = where B position i's bytes lie in A or DeltaOp.NONE, the new ops
    as ranges for dev_read_ranges over recipe B (all four or none).  d_totals[0..8) = verdict (1: an offset list does not ascend in
    extents of 1..65536, nothing else written; 2: more ops than max_ops, no op written), ops, new ops, in-place / moved / new bytes,
    matched positions, B positions.  max_ops = 0 with d_ops = 0 is a dry run.  Not synchronised."""
    check(lib().cw_dev_recipe_diff(d_ref_a, d_off_a, d_na, max_a, d_ref_b, d_off_b, d_nb, max_b, dir_base, dir_entries, d_ops or None, max_ops,
                                   d_nops, d_src or None, d_new_off or None, d_new_len or None, d_new_dst or None, d_nnew or None, d_totals,
                                   stream))


def dev_apply_delta(d_old: int, old_bytes: int, d_payload: int, payload_bytes: int, d_ops: int, d_nops: int, max_ops: int, d_dst: int,
                    dst_bytes: int, d_result: int, stream: int = 0) -> None:
    """d_dst[0..total) = the stream the min(*d_nops, max_ops) ops build from d_old and d_payload.  d_result[0..4) = verdict (1: the
    list is malformed, 2: total > dst_bytes; nothing written then), total, the lowest malformed op or DeltaOp.NONE, the op count.
    Not synchronised."""
    check(lib().cw_dev_apply_delta(d_old or None, old_bytes, d_payload or None, payload_bytes, d_ops or None, d_nops, max_ops, d_dst or None,
                                   dst_bytes, d_result, stream))


# ---- compose a stream from stored ranges and new bytes (cw_store_compose) --------------------------------
class ResyncWindow(C.Structure):
    """cw_resync_window: a window's cuts at or behind ``new_from`` are looked up, shifted by ``shift`` (mod 2^64), among the old cuts
    [old_first, old_first + old_count); ``final``: the window's last cut counts as well."""
    _fields_ = [(k, C.c_uint64) for k in ("new_from", "shift", "old_first", "old_count", "final")]


RESYNC_WINDOW_DTYPE = np.dtype([(k, "<u8") for k, _ in ResyncWindow._fields_])  # cw_resync_window as a numpy record


def dev_cdc_resync_windows(d_new_offsets: int, d_new_count: int, max_new: int, d_stream_first: int, d_win: int, nwin: int, d_old_offsets: int,
                           max_old: int, d_result: int, stream: int = 0) -> None:
    """``dev_cdc_resync`` for the nwin windows one ``dev_cdc_streams`` call chunked: d_result[4 * w ..] = (0, t, s, x) for the smallest
    t >= 1 whose cut x of window w lies at or behind the window's new_from with x + shift an old cut of the window's own range (s: its
    index in d_old_offsets), or (1, 0, 0, 0).  A window's last cut counts only when it is final.  No count changes.  Not synchronised."""
    check(lib().cw_dev_cdc_resync_windows(d_new_offsets, d_new_count, max_new, d_stream_first, d_win, nwin, d_old_offsets or None, max_old, d_result,
                                          stream))


def dev_scatter_extents(d_src: int, src_bytes: int, d_ext: int, d_n: int, max_n: int, d_dst: int, dst_bytes: int, d_result: int,
                        stream: int = 0) -> None:
    """Copies min(*d_n, max_n) extents (src_off, dst_off, len: three uint64 words each) from d_src to d_dst.  d_result[0..4) = verdict
    (1: an extent is empty, leaves a buffer, wraps or starts in front of the end of the one before; nothing is written then), the end
    of the last extent, the lowest bad extent or DeltaOp.NONE, the extent count.  Not synchronised."""
    check(lib().cw_dev_scatter_extents(d_src or None, src_bytes, d_ext or None, d_n, max_n, d_dst or None, dst_bytes, d_result, stream))


class ComposeStats(C.Structure):
    """cw_compose_stats: one store_compose call's windows, rounds and merges, what it rebuilt (bytes, chunks, the new chunks among them
    and their stored bytes) and the positions it kept."""
    _fields_ = [(k, C.c_uint64) for k in ("windows", "rounds", "merged_windows", "rebuilt_bytes", "rebuilt_chunks", "new_chunks", "stored_bytes",
                                          "kept_positions")]

    def as_dict(self) -> dict:
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


COMPOSE_DTYPE = np.dtype([(k, "<u8") for k, _ in ComposeStats._fields_])  # cw_compose_stats as a numpy record


def store_compose(index: "DedupeIndex", params: "CdcParams", comp_alg, store: Store, refs, offsets, ops, payload, base: int, lookahead: int = 0,
                  stream_first=None):
    """cw_store_compose: the stream the ``ops`` (DELTA_OP_DTYPE records, tiling it from 0) build from the bytes of the stored source
    (refs, offsets; with ``stream_first`` the concatenation of several stored streams) and ``payload``.  Returns (refs, offsets, stats as
    a dict) of the new stream; raises CwError (-5: not admitted, -2: a refused argument or a source range that does not restore) with
    index, store and directory unchanged."""
    refs, offsets = np.ascontiguousarray(refs, np.uint64), np.ascontiguousarray(offsets, np.uint64)
    if len(offsets) != len(refs) + 1:
        raise ValueError(f"{len(refs)} refs need {len(refs) + 1} offsets, not {len(offsets)}")
    ops = np.ascontiguousarray(ops, dtype=DELTA_OP_DTYPE).reshape(-1)
    pay = _np_u8(payload)
    first = None if stream_first is None else np.ascontiguousarray(stream_first, np.uint64)
    total = int(ops["len"].sum(dtype=np.uint64)) if len(ops) else 0
    cap = params.max_offsets(total)
    out_refs, out_offs = np.zeros(cap, np.uint64), np.zeros(cap, np.uint64)
    k, stats = C.c_size_t(0), ComposeStats()
    check(lib().cw_store_compose(index._x(), C.byref(params), _comp_id(comp_alg), C.byref(store), refs.ctypes.data if len(refs) else None,
                                 offsets.ctypes.data, len(refs), None if first is None else first.ctypes.data, 0 if first is None else len(first) - 1,
                                 ops.ctypes.data if len(ops) else None, len(ops), pay.ctypes.data if pay.size else None, pay.size, base, lookahead,
                                 out_refs.ctypes.data, out_offs.ctypes.data, cap, C.byref(k), C.byref(stats)))
    k = int(k.value)
    return out_refs[:k].copy(), out_offs[:k + 1].copy(), stats.as_dict()


def store_restore(comp_alg, store: Store, refs, offsets, dst: int, dst_bytes: int):
    """cw_store_restore into the host memory at address ``dst``: the status of every position (u32 array)."""
    refs, offsets = np.ascontiguousarray(refs, np.uint64), np.ascontiguousarray(offsets, np.uint64)
    status, n_bad = np.zeros(max(len(refs), 1), np.uint32), C.c_size_t(0)
    check(lib().cw_store_restore(_comp_id(comp_alg), C.byref(store), refs.ctypes.data if len(refs) else None, offsets.ctypes.data, len(refs),
                                 dst or None, dst_bytes, status.ctypes.data, C.byref(n_bad)))
    status = status[:len(refs)]
    assert int(n_bad.value) == int((status != 0).sum())
    return status


class ScrubStats(C.Structure):
    """cw_scrub_stats: what a scrub checked and found, the decoded bytes it hashed and the windows it took."""
    _fields_ = [(k, C.c_uint64) for k in ("checked", "ok", "malformed", "unsound", "mismatch", "orphan", "raw_bytes", "windows")]

    def as_dict(self) -> dict:
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


def store_scrub(index: "DedupeIndex", comp_alg, store: Store, d_live: int = 0):
    """cw_store_scrub: every directory entry (d_live = 0), or the entries the device flags d_live (u32[dir_entries]) select, checked
    against ``index`` in windows of CW_STORE_PIECE decoded bytes.  Returns (status u32 array, one per entry; stats as a dict)."""
    status, stats = np.zeros(store.dir_entries, np.uint32), ScrubStats()
    check(lib().cw_store_scrub(index._x(), _comp_id(comp_alg), C.byref(store), d_live or None, status.ctypes.data, C.byref(stats)))
    return status, stats.as_dict()


def dev_ingest_commit(d_ref: int, d_offsets: int, d_nchunks: int, max_chunks: int, d_n_new: int, d_store_result: int, stream_off: int,
                      d_rec_ref: int, d_rec_off: int, d_rec_count: int, rec_cap: int, d_stats: int, d_verdict: int, stream: int = 0) -> None:
    """Append one piece's refs and cuts (shifted by stream_off) to a recipe that grows on the device, behind the piece's
    dev_store_chunks; *d_verdict = 0, or 1 (the append was refused) / 2 (the recipe is full) with nothing changed.  Not synchronised."""
    check(lib().cw_dev_ingest_commit(d_ref, d_offsets, d_nchunks, max_chunks, d_n_new, d_store_result or None, stream_off, d_rec_ref, d_rec_off,
                                     d_rec_count, rec_cap, d_stats or None, d_verdict, stream))


def dev_ingest_commit_streams(d_ref: int, d_offsets: int, d_nchunks: int, max_chunks: int, d_n_new: int, d_store_result: int, stream_off: int,
                              d_rec_ref: int, d_rec_off: int, d_rec_count: int, rec_cap: int, d_stats: int, d_verdict: int, d_stream_first: int,
                              nstreams_piece: int, first_stream: int, skip_first: bool, d_rec_first: int, first_cap: int, stream: int = 0) -> None:
    """``dev_ingest_commit`` for a piece of many streams: also d_rec_first[first_stream + f] = the recipe's count before the call +
    d_stream_first[f] for skip_first <= f < nstreams_piece; *d_verdict = 3 when first_stream + nstreams_piece > first_cap.  With any
    verdict other than 0 nothing changes.  Not synchronised."""
    check(lib().cw_dev_ingest_commit_streams(d_ref, d_offsets, d_nchunks, max_chunks, d_n_new, d_store_result or None, stream_off, d_rec_ref,
                                             d_rec_off, d_rec_count, rec_cap, d_stats or None, d_verdict, d_stream_first, nstreams_piece,
                                             first_stream, 1 if skip_first else 0, d_rec_first, first_cap, stream))


def store_ingest_streams(index: "DedupeIndex", params: "CdcParams", comp_alg, store: Store, srcs, lens, base: int):
    """cw_store_ingest_streams of the host spans at the addresses ``srcs`` with the lengths ``lens``: (rc, refs, offsets, stream_first,
    consumed, streams_done, stats as a dict), in the coordinates of the spans' concatenation.  rc is 0, or -5 when a piece was refused:
    everything then covers the pieces before it, and stream_first has streams_done + 2 entries (all of them when no stream is left).
    Any other failure raises."""
    lens = np.ascontiguousarray(lens, np.uint64).reshape(-1)
    nf = len(lens)
    ptrs = (C.c_void_p * max(nf, 1))(*[int(a) or None for a in srcs])
    cap = params.max_offsets_streams(int(lens.sum(dtype=np.uint64)), nf)
    refs, offs, first = np.zeros(cap, np.uint64), np.zeros(cap, np.uint64), np.zeros(nf + 1, np.uint64)
    k, consumed, done, stats = C.c_size_t(0), C.c_uint64(0), C.c_size_t(0), IngestStats()
    rc = lib().cw_store_ingest_streams(index._x(), C.byref(params), _comp_id(comp_alg), C.byref(store), ptrs if nf else None,
                                       lens.ctypes.data if nf else None, nf, base, refs.ctypes.data, offs.ctypes.data, cap, first.ctypes.data,
                                       C.byref(k), C.byref(consumed), C.byref(done), C.byref(stats))
    if rc not in (0, -5):
        check(rc)
    k, done = int(k.value), int(done.value)
    return rc, refs[:k].copy(), offs[:k + 1].copy(), first[:min(done + 2, nf + 1)].copy(), int(consumed.value), done, stats.as_dict()
