"""Mark, compact and retain in plain Python: what cw_dev_store_mark, cw_dev_store_compact and cw_dedupe_retain give, over the
directory entries (``restore_model.LOC``) and the content index (``restore_model.Model``) of the chunk store's model."""
from __future__ import annotations

import numpy as np

from restore_model import LEN_MASK, LOC, MISS, RAW, Model  # noqa: F401  (MISS, Model: for the callers)


def mark(refs, dir_base, dir_entries, live=None, outside=0):
    """One cw_dev_store_mark call over the positions `refs`: (flags, outside count), on top of an earlier call's when given."""
    live = np.zeros(dir_entries, np.uint32) if live is None else live.copy()
    for r in refs:
        idx = (int(r) - dir_base) % 2 ** 64          # u64: a value below the base wraps out of range
        if idx < dir_entries:
            live[idx] = 1
        else:
            outside += 1
    return live, outside


def sound(entry, store_bytes) -> bool:
    """The entry checks of cw_dev_restore_chunks that need no recipe."""
    pos, stored, word = (int(v) for v in entry)
    l, is_raw = word & LEN_MASK, bool(word & RAW)
    return (not word & ~(RAW | LEN_MASK) and 1 <= l <= 65536 and stored != 0 and (not is_raw or stored == l)
            and pos + stored <= store_bytes)


def compact(store, store_bytes, directory, live, new_store_bytes):
    """One cw_dev_store_compact call: (verdict, [verdict, kept bytes, kept, dropped], new blob, new directory).  The blob and the
    directory are None unless the verdict is 0: nothing of the new buffers changes then."""
    kept = [i for i in range(len(directory)) if live[i] and any(int(v) for v in directory[i])]
    dropped = sum(1 for i in range(len(directory)) if any(int(v) for v in directory[i])) - len(kept)
    total = sum(int(directory[i]["stored"]) for i in kept)
    verdict = 2 if not all(sound(directory[i], store_bytes) for i in kept) else 1 if total > new_store_bytes else 0
    result = [verdict, total, len(kept), dropped]
    if verdict:
        return verdict, result, None, None
    blob, new_dir = bytearray(), np.zeros(len(directory), LOC)
    for i in kept:
        pos, stored, word = (int(v) for v in directory[i])
        new_dir[i] = (len(blob), stored, word)
        blob += bytes(store[pos:pos + stored])
    return verdict, result, bytes(blob), new_dir


def retain(values: dict, live, dir_base, dir_entries) -> dict:
    """cw_dedupe_retain over Model.values ({content or digest: value}): the entries whose value names no entry of the directory,
    or a flagged one."""
    def keep(v):
        idx = (int(v) - dir_base) % 2 ** 64
        return idx >= dir_entries or bool(live[idx])
    return {k: v for k, v in values.items() if keep(v)}


def three_streams(alice: bytes, kennedy: bytes):
    """The scenario of the store's tests: a stream and two edited copies of it.  Keeping the first and the third drops the chunks
    around the second's edit; everything else of the second is shared with the kept ones."""
    a = alice[:60000] + np.random.default_rng(5).bytes(20000) + kennedy[:40000]
    b = a[:30000] + b"an edit that only the second stream has" + a[30000:]
    c = a[:90000] + b"THIRD" + a[90100:]
    return a, b, c
