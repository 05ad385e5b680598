"""The chunk store in plain Python: what cw_dev_store_chunks appends and what cw_dev_restore_chunks gives back.

No GPU and no ctypes of its own: the compressed bytes and the decoders' verdicts come from the caller (the CPU oracle's
``lz4_compress`` / ``lzf_compress`` / ``*_decompress``).  ``append`` and ``restore`` are the two calls' definitions as the
header states them; ``Model`` adds the dedupe by content that the index performs, so that a whole ingest has an expected
store, directory and recipe."""
from __future__ import annotations

import numpy as np

RAW = 0x80000000          # CW_CHUNK_RAW
LEN_MASK = 0x1FFFF
MISS = 2 ** 64 - 1        # CW_DEDUPE_MISS
LOC = np.dtype([("pos", "<u8"), ("stored", "<u4"), ("raw", "<u4")])   # cw_chunk_loc


def in_contract(cuts, i, count, src_bytes) -> bool:
    return 0 <= i < count and cuts[i] < cuts[i + 1] <= src_bytes and cuts[i + 1] - cuts[i] <= 65536


def compressed(oracle, alg, data, cuts, chunks, count=None, src_bytes=None):
    """The oracle's compressed bytes of every listed chunk (b"": LZF did not fit; None: the chunk is out of contract)."""
    fn = oracle.lz4_compress if alg == "lz4" else oracle.lzf_compress
    count = len(cuts) - 1 if count is None else count
    src_bytes = len(data) if src_bytes is None else src_bytes
    return [fn(bytes(data[cuts[i]:cuts[i + 1]])) if in_contract(cuts, i, count, src_bytes) else None for i in chunks]


def append(data, cuts, chunks, comp, base, used, store_bytes, dir_base, dir_entries, count=None, src_bytes=None):
    """One cw_dev_store_chunks call over the positions `chunks` (comp[j] = position j's compressed bytes).
    Returns (verdict, total, blob, entries): the bytes that go to store[used:] and {directory index: (pos, stored, raw)} --
    both empty unless the verdict is 0."""
    count = len(cuts) - 1 if count is None else count
    src_bytes = len(data) if src_bytes is None else src_bytes
    blob, entries, outside = bytearray(), {}, False
    for j, i in enumerate(chunks):
        if not in_contract(cuts, i, count, src_bytes):
            continue
        l = cuts[i + 1] - cuts[i]
        piece, flag = (comp[j], 0) if comp[j] and len(comp[j]) < l else (bytes(data[cuts[i]:cuts[i + 1]]), RAW)
        idx = base + i - dir_base
        outside |= not 0 <= idx < dir_entries or base + i > MISS
        entries[idx] = (used + len(blob), len(piece), l | flag)
        blob += piece
    verdict = 1 if used + len(blob) > store_bytes else 2 if outside else 0
    return (verdict, len(blob), bytes(blob), entries) if verdict == 0 else (verdict, len(blob), b"", {})


def restore(store, store_bytes, directory, dir_base, refs, raw_offsets, dst_bytes, decode):
    """One cw_dev_restore_chunks call: [(status, bytes or None)] per position.  `directory` is a LOC array, `decode(stream, l)`
    the oracle's decoder (None or a wrong length = malformed)."""
    out = []
    for j, r in enumerate(refs):
        rs, re, idx = int(raw_offsets[j]), int(raw_offsets[j + 1]), int(r) - dir_base
        status, piece = 2, None
        if 0 <= idx < len(directory) and rs <= re and re - rs <= 65536 and re <= dst_bytes:
            pos, stored, word = (int(v) for v in directory[idx])
            l, is_raw = word & LEN_MASK, bool(word & RAW)
            if (not word & ~(RAW | LEN_MASK) and 1 <= l <= 65536 and l == re - rs and stored and (not is_raw or stored == l)
                    and pos + stored <= store_bytes):
                ext = bytes(store[pos:pos + stored])
                piece = ext if is_raw else decode(ext, l) if stored <= 1 << 24 else None
                status = 0 if piece is not None and len(piece) == l else 1
        out.append((status, piece if status == 0 else None))
    return out


class Model:
    """Index + store over several ingests: dedupe by content (what full digests give), then `append` of the new chunks."""

    def __init__(self, oracle, alg, store_bytes, dir_entries, dir_base=0):
        self.oracle, self.alg = oracle, alg
        self.store_bytes, self.dir_base = store_bytes, dir_base
        self.blob = bytearray()
        self.directory = np.zeros(dir_entries, LOC)
        self.values = {}

    def ingest(self, data, cuts, base):
        """Returns (refs, new chunks, verdict, total); a verdict other than 0 leaves the store as it was (the index keeps the chunks)."""
        refs, new = [], []
        for i in range(len(cuts) - 1):
            key = bytes(data[cuts[i]:cuts[i + 1]])
            if key not in self.values:
                self.values[key] = base + i
                new.append(i)
            refs.append(self.values[key])
        comp = compressed(self.oracle, self.alg, data, cuts, new)
        verdict, total, blob, entries = append(data, cuts, new, comp, base, len(self.blob), self.store_bytes, self.dir_base,
                                               len(self.directory))
        self.blob += blob
        for idx, e in entries.items():
            self.directory[idx] = e
        return refs, new, verdict, total

    def decode(self):
        return self.oracle.lz4_decompress if self.alg == "lz4" else self.oracle.lzf_decompress
