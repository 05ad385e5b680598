"""cw_store_ingest in plain Python: piece, carry, admission, commit.

The stream goes through in pieces of ``piece`` fresh bytes (raised to max_size) plus the carry, the bytes behind the previous
piece's last cut.  Every piece but the last is chunked with final = False (tests/cdc_model.py).  Before a piece goes into the index
(``restore_model.Model``'s dedupe by content) it is admitted against the index's room, the directory and -- conservatively, with the
bytes it consumes -- the store; a refused piece ends the run and leaves everything as the pieces before it left it.  ``commit`` is
cw_dev_ingest_commit on its own."""
from __future__ import annotations

import cdc_model as CM
import restore_model as RM


class Run:
    """What one cw_store_ingest call returns, plus what the tests assert about its pieces."""

    def __init__(self):
        self.refs, self.offsets = [], [0]
        self.refused = None           # None, or "index" / "directory" / "store": why the next piece did not go in
        self.carries = []             # the carry in front of every piece that went in
        self.pieces = []              # per piece that went in: dict(chunks, new, consumed, stored, used_before)
        self.stats = dict(bytes=0, chunks=0, new_chunks=0, stored_bytes=0, pieces=0)

    @property
    def consumed(self):
        return self.offsets[-1]

    @property
    def nchunks(self):
        return len(self.refs)


def clone(m: RM.Model, store_bytes=None, dir_entries=None) -> RM.Model:
    """A copy of a model to go on with, optionally with more room."""
    import numpy as np
    c = RM.Model(m.oracle, m.alg, m.store_bytes if store_bytes is None else store_bytes, max(dir_entries or 0, len(m.directory)), m.dir_base)
    c.blob, c.values = bytearray(m.blob), dict(m.values)
    c.directory[:len(m.directory)] = m.directory
    assert isinstance(c.directory, np.ndarray)
    return c


def piece_bytes(p: dict, piece: int) -> int:
    return max(piece, p["max"])


def ingest(m: RM.Model, data: bytes, p: dict, piece: int, base: int, max_entries=None) -> Run:
    """The streamed ingest of ``data`` into the model ``m`` (its index holds len(m.values) entries of max_entries)."""
    r, n, P = Run(), len(data), piece_bytes(p, piece)
    npieces = (n + P - 1) // P
    done = 0
    for i in range(npieces):
        end, final = min(n, (i + 1) * P), i == npieces - 1
        part = data[done:end]
        cuts = CM.chunk(part, p, final=final)
        k, consumed, base_k, used = len(cuts) - 1, cuts[-1], base + len(r.refs), len(m.blob)
        if k and not (m.dir_base <= base_k and base_k + k <= m.dir_base + len(m.directory)):
            r.refused = "directory"
        elif used + consumed > m.store_bytes:
            r.refused = "store"
        elif max_entries is not None and len(m.values) + k > max_entries:
            r.refused = "index"
        if r.refused:
            return r
        refs, new, verdict, total = m.ingest(part, cuts, base_k)
        assert verdict == 0, "an admitted append was refused"
        r.carries.append(i * P - done)
        r.pieces.append(dict(chunks=k, new=len(new), consumed=consumed, stored=total, used_before=used,
                             inner_dups=sum(1 for j, v in enumerate(refs) if base_k <= v != base_k + j)))
        r.refs += refs
        r.offsets += [done + c for c in cuts[1:]]
        done += consumed
        for key, v in (("bytes", consumed), ("chunks", k), ("new_chunks", len(new)), ("stored_bytes", total), ("pieces", 1)):
            r.stats[key] += v
    assert done == n
    return r


def one_shot(m: RM.Model, data: bytes, p: dict, base: int):
    """ONE cw_dev_cdc_dedupe_compress + cw_dev_store_chunks over the whole stream: (refs, cuts)."""
    cuts = CM.chunk(data, p) if len(data) else [0]
    refs, _, verdict, _ = m.ingest(data, cuts, base)
    assert verdict == 0
    return refs, cuts


def commit(ref, offsets, n, n_new, store_result, stream_off, rec_ref, rec_off, rec_count, rec_cap, stats):
    """cw_dev_ingest_commit on lists: returns (verdict, rec_count); rec_ref, rec_off and stats (5 entries) change in place, and
    only when the verdict is 0."""
    if store_result is not None and store_result[0]:
        return 1, rec_count
    if rec_count + n + 1 > rec_cap:
        return 2, rec_count
    for j in range(n):
        rec_ref[rec_count + j] = ref[j]
    for j in range(n + 1):
        rec_off[rec_count + j] = (stream_off + offsets[j]) % 2 ** 64
    for i, v in enumerate((offsets[n] - offsets[0], n, n_new, store_result[1] if store_result is not None else 0, 1)):
        stats[i] += v
    return 0, rec_count + n
