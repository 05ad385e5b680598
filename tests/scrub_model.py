"""Scrub and repair in plain Python: what cw_dev_store_verify, cw_store_scrub and cw_dev_store_replace_chunks give, over the
directory entries (``restore_model.LOC``), the decoder's verdicts (``restore_model.restore``) and the entry checks
(``store_gc_model.sound``) of the chunk store's model.  Decoders and hashes are the CPU oracle's.

The window rule (normative, cw_dev_store_verify's header comment): with c the cursor, a call at c >= dir_entries writes nothing.
Otherwise E = min(dir_entries, c + entry_cap); entry idx is selected iff it is not all zero (no flags) or live[idx] != 0 (flags);
it is decodable iff it is selected and sound; need(idx) = its length when decodable, else 0; e is the largest index in (c, E] with
sum(need[c:e]) <= work_bytes; the call writes the statuses of [c, e), adds to the totals and sets the cursor to e.

An entry's status depends on the store, the directory, the flags and the index alone -- not on the windows."""
from __future__ import annotations

import numpy as np

from restore_model import LEN_MASK, restore
from store_gc_model import sound

OK, MALFORMED, UNSOUND, MISMATCH, ORPHAN, SKIPPED = range(6)          # CW_SCRUB_*
DEFAULT_ENTRIES = 1 << 20                                             # CW_SCRUB_ENTRIES
TOTALS = ("checked", "ok", "malformed", "unsound", "mismatch", "orphan", "raw_bytes", "windows")
U64 = 2 ** 64


def hash_fn(oracle, hash_alg):
    return {"skein512": oracle.skein512, "skein": oracle.skein256, "sha256mb": oracle.sha256}[hash_alg]


def entry_cap(knob=None) -> int:
    """CW_SCRUB_ENTRIES as the library reads it: the default when unset or not positive, at least 64."""
    return max(64, knob if knob and knob > 0 else DEFAULT_ENTRIES)


def selected(entry, idx, live) -> bool:
    return bool(live[idx]) if live is not None else any(int(v) for v in entry)


def need(directory, store_bytes, live=None) -> list:
    """need(idx) of every entry: the length of a decodable entry, else 0."""
    return [int(e["raw"]) & LEN_MASK if selected(e, i, live) and sound(e, store_bytes) else 0 for i, e in enumerate(directory)]


def entry_status(store, store_bytes, directory, dir_base, idx, live, digests_of, decode, hash_of) -> int:
    """The status of entry idx.  digests_of = {value: [digests]}: what the index holds; decode(stream, l) the oracle's decoder."""
    e = directory[idx]
    if not selected(e, idx, live):
        return SKIPPED
    if not sound(e, store_bytes):
        return UNSOUND
    l = int(e["raw"]) & LEN_MASK
    (status, piece), = restore(store, store_bytes, directory, dir_base, [dir_base + idx], [0, l], l, decode)
    if status:
        return MALFORMED if status == 1 else UNSOUND
    held = digests_of.get(dir_base + idx, [])
    return ORPHAN if not held else OK if hash_of(piece) in held else MISMATCH


def statuses(store, store_bytes, directory, dir_base, live, digests_of, decode, hash_of) -> np.ndarray:
    return np.array([entry_status(store, store_bytes, directory, dir_base, i, live, digests_of, decode, hash_of)
                     for i in range(len(directory))], np.uint32)


def window_end(needs, c, work_bytes, cap) -> int:
    """e of the window that starts at c < len(needs)."""
    assert work_bytes >= 65536
    E, e, total = min(len(needs), c + cap), c, 0
    while e < E and total + needs[e] <= work_bytes:
        total += needs[e]
        e += 1
    assert e > c
    return e


def verify(needs, status, c, work_bytes, cap):
    """One cw_dev_store_verify call at cursor c: (the new cursor, {idx: status written}, what it adds to the totals)."""
    add = dict.fromkeys(TOTALS, 0)
    if c >= len(needs):
        return c, {}, add
    e = window_end(needs, c, work_bytes, cap)
    written = {idx: int(status[idx]) for idx in range(c, e)}
    for s in written.values():
        if s != SKIPPED:
            add["checked"] += 1
            add[TOTALS[1 + s]] += 1
    add["raw_bytes"], add["windows"] = sum(needs[c:e]), 1
    return e, written, add


def scrub(needs, status, work_bytes, cap=DEFAULT_ENTRIES, start=0):
    """cw_store_scrub, or a loop of device calls from cursor `start`: (the statuses written as {idx: status}, the totals, the cursors
    the calls leave)."""
    c, written, totals, cursors = start, {}, dict.fromkeys(TOTALS, 0), []
    while c < len(needs):
        c, w, add = verify(needs, status, c, work_bytes, cap)
        written.update(w)
        totals = {k: totals[k] + add[k] for k in TOTALS}
        cursors.append(c)
    return written, totals, cursors


def replace_chunks(payload, in_bytes, in_locs, values, used, store_bytes, directory, dir_base):
    """One cw_dev_store_replace_chunks call: (verdict, total, blob, entries) -- the bytes that go to store[used:] and {directory
    index: (pos, stored, raw)}, both empty unless the verdict is 0."""
    blob, entries, unsound, outside, length = bytearray(), {}, False, False, False
    for k, v in enumerate(values):
        if not any(int(x) for x in in_locs[k]) or not sound(in_locs[k], in_bytes):
            unsound = True
            continue
        pos, stored, word = (int(x) for x in in_locs[k])
        idx = (int(v) - dir_base) % U64
        if idx >= len(directory):
            outside = True
        else:
            here = int(directory[idx]["raw"]) & LEN_MASK
            length |= 1 <= here <= 65536 and here != word & LEN_MASK
            entries[idx] = (used + len(blob), stored, word)
        blob += bytes(payload[pos:pos + stored])
    verdict = 3 if unsound else 1 if used + len(blob) > store_bytes else 2 if outside else 4 if length else 0
    return (verdict, len(blob), bytes(blob), entries) if verdict == 0 else (verdict, len(blob), b"", {})


def digests_by_value(pairs) -> dict:
    """{value: [digests]} of the index entries `pairs` [(digest, value)]."""
    out = {}
    for digest, value in pairs:
        out.setdefault(int(value), []).append(bytes(digest))
    return out
