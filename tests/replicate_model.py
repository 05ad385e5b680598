"""Chunk bundles in plain Python: what cw_dev_dedupe_export_live, cw_dev_store_export_chunks, cw_dev_store_import_chunks and
cw_dev_translate_refs give, and ChunkStore.export_bundle / import_bundle / replicate_to over them, on the directory entries
(``restore_model.LOC``) and the content index (``restore_model.Model``) of the chunk store's model.  In a Model the digest of a
chunk is its content."""
from __future__ import annotations

import numpy as np

from restore_model import LOC, MISS, Model
from store_gc_model import mark, sound

U64 = 2 ** 64


def export_live(pairs, live, dir_base, dir_entries, max_out):
    """One cw_dev_dedupe_export_live call over the index entries `pairs` [(digest, value)]: (values, candidates, [L, hits]) for the
    min(L, max_out) slots written; candidates[k] = the digests the call may write there (none: a zero digest with CW_DEDUPE_MISS)."""
    by_value = {}
    for digest, value in pairs:
        if (value - dir_base) % U64 < dir_entries and live[(value - dir_base) % U64]:
            by_value.setdefault(value, []).append(digest)
    flagged = [dir_base + int(i) for i in np.nonzero(np.asarray(live)[:dir_entries])[0]]
    slots = flagged[:max_out]
    return ([v if v in by_value else MISS for v in slots], [by_value.get(v, []) for v in slots],
            [len(flagged), sum(len(d) for d in by_value.values())])


def export_chunks(store, store_bytes, directory, dir_base, values, out_bytes):
    """One cw_dev_store_export_chunks call: (verdict, [verdict, total, n], blob, locs); blob and locs are None unless the verdict is 0."""
    blob, locs, bad = bytearray(), np.zeros(len(values), LOC), False
    for k, v in enumerate(values):
        idx = (int(v) - dir_base) % U64
        if idx >= len(directory) or not any(int(x) for x in directory[idx]) or not sound(directory[idx], store_bytes):
            bad = True
            continue
        pos, stored, word = (int(x) for x in directory[idx])
        locs[k] = (len(blob), stored, word)
        blob += bytes(store[pos:pos + stored])
    verdict = 2 if bad else 1 if len(blob) > out_bytes else 0
    result = [verdict, len(blob), len(values)]
    return (verdict, result, bytes(blob), locs) if verdict == 0 else (verdict, result, None, None)


def import_chunks(payload, in_bytes, in_locs, n, sel, base, used, store_bytes, dir_base, dir_entries):
    """One cw_dev_store_import_chunks call over a bundle of n chunks and the selection `sel` (None: every chunk):
    (verdict, total, blob, entries) -- the bytes that go to store[used:] and {directory index: (pos, stored, raw)}, both empty
    unless the verdict is 0."""
    blob, entries, unsound, outside = bytearray(), {}, False, False
    for k in (range(n) if sel is None else sel):
        k = int(k)
        if k >= n or not any(int(x) for x in in_locs[k]) or not sound(in_locs[k], in_bytes):
            unsound = True
            continue
        pos, stored, word = (int(x) for x in in_locs[k])
        idx = base + k - dir_base
        outside |= not 0 <= idx < dir_entries or base + k > MISS
        entries[idx] = (used + len(blob), stored, word)
        blob += bytes(payload[pos:pos + stored])
    verdict = 3 if unsound else 1 if used + len(blob) > store_bytes else 2 if outside else 0
    return (verdict, len(blob), bytes(blob), entries) if verdict == 0 else (verdict, len(blob), b"", {})


def translate(refs, frm, to):
    """One cw_dev_translate_refs call: (out, the number of positions that found no pair)."""
    table = {int(f): int(t) for f, t in zip(frm, to)}
    out = [table.get(int(r), MISS) for r in refs]
    return out, sum(int(r) not in table for r in refs)


# ---- over restore_model.Model --------------------------------------------------------------------------------------------------
def export_bundle(m: Model, recipes, known=None):
    """ChunkStore.export_bundle: `recipes` are lists of refs, `known` the receiver's Model.values (or None).  A dict with digests
    (chunk contents), values, locs, payload."""
    live, outside = np.zeros(len(m.directory), np.uint32), 0
    for refs in recipes:
        live, outside = mark(refs, m.dir_base, len(m.directory), live, outside)
    assert outside == 0
    n = int(np.count_nonzero(live))
    values, cands, result = export_live([(d, v) for d, v in m.values.items()], live, m.dir_base, len(m.directory), n)
    assert result == [n, n] and MISS not in values and all(len(c) == 1 for c in cands)
    digests = [c[0] for c in cands]
    carry = [k for k, d in enumerate(digests) if known is None or d not in known]
    verdict, _, blob, out_locs = export_chunks(m.blob, m.store_bytes, m.directory, m.dir_base, [values[k] for k in carry], len(m.blob))
    assert verdict == 0
    locs = np.zeros(n, LOC)
    locs[carry] = out_locs
    return dict(digests=digests, values=values, locs=locs, payload=blob, carried=carry)


def import_bundle(m: Model, bundle, base, recipes):
    """ChunkStore.import_bundle behind its checks: the manifest through the index (m.values), the new chunks into the store, the
    recipes translated.  Returns (recipes in m's values, the manifest positions that were new); base grows by len(values) at the caller."""
    ref, new = [], []
    for k, d in enumerate(bundle["digests"]):
        if d not in m.values:
            m.values[d] = base + k
            new.append(k)
        ref.append(m.values[d])
    verdict, _, blob, entries = import_chunks(bundle["payload"], len(bundle["payload"]), bundle["locs"], len(ref), new, base, len(m.blob),
                                              m.store_bytes, m.dir_base, len(m.directory))
    assert verdict == 0
    m.blob += blob
    for idx, e in entries.items():
        m.directory[idx] = e
    out = []
    for refs in recipes:
        got, missing = translate(refs, bundle["values"], ref)
        assert missing == 0
        out.append(got)
    return out, new


def replicate(a: Model, b: Model, recipes, base, negotiate=True):
    """ChunkStore.replicate_to (negotiate=False: export_bundle without `known`): (bundle, b's recipes, the new manifest positions)."""
    bundle = export_bundle(a, recipes, b.values if negotiate else None)
    out, new = import_bundle(b, bundle, base, recipes)
    return bundle, out, new
