"""The chunk store: ``ChunkStore`` and what travels with it (``Recipe``, ``Bundle``, ``ScrubReport``, ``Diff``, ``Delta``) over the ``dev_*`` and
``store_*`` wrappers of ``ops``.

``ops`` takes raw device pointers and never touches torch; this is the one place in the package that owns torch buffers: it
allocates and fills them, synchronises torch's stream around the ABI calls and reads their result words back.  torch is imported
when a method first needs it, so importing the package does not import it.
"""
from __future__ import annotations

import functools

import numpy as np

from ._lib import CwError, lib
from .ops import (ACCOUNT_DTYPE, DELTA_OP_DTYPE, CdcParams, ChunkLoc, DedupeIndex, DeltaOp, Store, _comp_id, _hash_id, _np_u8, chunk_slots_bytes,
                  dev_apply_delta, dev_hash_chunks, dev_read_ranges, dev_recipe_diff, dev_restore_chunks, dev_scatter_extents, dev_store_account,
                  dev_store_chunks, dev_store_compact, dev_store_export_chunks, dev_store_guard2_check, dev_store_guard2_locate,
                  dev_store_guard2_rebuild, dev_store_guard2_update, dev_store_guard_check, dev_store_guard_locate, dev_store_guard_rebuild,
                  dev_store_guard_update, dev_store_import_chunks, dev_store_mark, dev_store_renumber, dev_store_replace_chunks, dev_translate_refs,
                  device_count, digest_bytes, init, store_compose, store_guard_bytes, store_ingest, store_ingest_streams, store_patch, store_restore,
                  store_scrub)


class Recipe:
    """What restores one ingested stream: refs[j] = the value of chunk j's first occurrence, offsets[0..k] = its cuts.  Stale after
    ``ChunkStore.renumber`` unless it was passed to it: use the translated recipe that call returns."""

    def __init__(self, refs, offsets):
        self.refs = np.ascontiguousarray(refs, dtype=np.uint64)
        self.offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        if len(self.offsets) != len(self.refs) + 1:
            raise ValueError(f"{len(self.refs)} refs need {len(self.refs) + 1} offsets, not {len(self.offsets)}")

    @property
    def nbytes(self) -> int:
        return int(self.offsets[-1] - self.offsets[0])


LOC_DTYPE = np.dtype([("pos", "<u8"), ("stored", "<u4"), ("raw", "<u4")])  # cw_chunk_loc as a numpy record
_MISS = np.uint64(DedupeIndex.MISS)


def _locs_sound(locs, in_bytes: int) -> np.ndarray:
    """bool per LOC_DTYPE record: sound by cw_dev_store_compact's entry checks against a buffer of in_bytes bytes."""
    pos, stored, word = locs["pos"], locs["stored"].astype(np.int64), locs["raw"].astype(np.int64)
    length, is_raw = word & 0x1FFFF, (word & ChunkLoc.RAW) != 0
    return ((word & ~(ChunkLoc.RAW | 0x1FFFF)) == 0) & (length >= 1) & (length <= 65536) & (stored != 0) & (~is_raw | (stored == length)) & \
        (pos <= in_bytes) & (stored <= in_bytes - np.minimum(pos, np.uint64(in_bytes)).astype(np.int64))


# Device buffers: max(k, 1) zeroed elements (int64 unless told otherwise), ``a`` as uint64 words (an int64 tensor), the bytes of the
# array ``a``.  None of them synchronises: torch fills them on its own stream, so a caller synchronises before an ABI call reads them.
def _zeros(k: int, dtype=None):
    import torch
    return torch.zeros(max(k, 1), dtype=dtype or torch.int64, device="cuda")


def _u64(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.uint64).view(np.int64).copy()).cuda()


def _u8(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def _words(t, n=None) -> tuple:
    """The first n (default: all) uint64 words of a small device tensor as Python ints.  Does not synchronise."""
    return tuple(int(v) for v in t.cpu().numpy().view(np.uint64)[:n])


def _need_device() -> None:
    if device_count() <= 0:
        init()  # (raises: no device)


def _refuse_unrestored(st, refs) -> None:
    """CwError (-2) unless every status of a restore is 0."""
    if st.any():
        j = int(np.nonzero(st)[0][0])
        raise CwError(-2, f"chunk store: {int((st != 0).sum())} of {len(st)} positions not restored; position {j} (ref {int(refs[j])}) has "
                          f"status {int(st[j])}")


def _entry_index(values, dir_base: int, dir_entries: int, report: bool = False) -> np.ndarray:
    """The directory entries (int64) of ``values`` (uint64), or CwError (-2), worded for a ``report``'s values or for a caller's."""
    idx = values - np.uint64(dir_base)
    if (values < np.uint64(dir_base)).any() or (idx >= np.uint64(dir_entries)).any():
        raise CwError(-2, f"chunk store: the report names values outside the directory [{dir_base}, {dir_base + dir_entries})" if report else
                          f"chunk store: values outside the directory [{dir_base}, {dir_base + dir_entries})")
    return idx.astype(np.int64)


def _joined(recipes) -> tuple:
    """Recipes back to back as one: (refs, offsets from 0, the byte at which each starts, the position at which each starts), uint64."""
    starts = np.concatenate([np.zeros(1, np.uint64), np.cumsum([r.nbytes for r in recipes], dtype=np.uint64)])
    first = np.concatenate([np.zeros(1, np.uint64), np.cumsum([len(r.refs) for r in recipes], dtype=np.uint64)])
    refs = np.concatenate([r.refs for r in recipes]) if recipes else np.zeros(0, np.uint64)
    offs = np.concatenate([np.zeros(1, np.uint64)] + [r.offsets[1:] - r.offsets[0] + starts[i] for i, r in enumerate(recipes)])
    return refs, offs, starts, first


def _looked_up(index: DedupeIndex, d_dig, k: int, s: int) -> np.ndarray:
    """What ``index`` answers for the k digests of the device tensor d_dig (``dev_lookup``): their values or MISS, uint64[k]."""
    import torch
    found, n_found = _zeros(k), _zeros(1)
    torch.cuda.synchronize()
    index.dev_lookup(d_dig.data_ptr(), k, found.data_ptr(), n_found.data_ptr(), s)
    torch.cuda.synchronize()
    return found.cpu().numpy().view(np.uint64)[:k]


def _export_chunks(cs: "ChunkStore", d_val, nc: int, s: int, damaged: str | None = None, whence: str = ""):
    """The stored bytes of the nc values d_val (a device tensor) of ``cs``: ``dev_store_export_chunks`` twice, a dry run that sizes the
    payload and the run that fills it.  Returns (payload tensor, total bytes, cw_chunk_loc tensor).  With ``damaged``, verdict 2 in
    either run raises CwError (-2) with that text; any verdict of the second run raises CwError (-4), worded with ``whence``."""
    import torch
    d_count, d_loc, res, out, total = _u64([nc]), _zeros(nc * 2), _zeros(3), None, 0
    for dry in (True, False):
        torch.cuda.synchronize()
        dev_store_export_chunks(*cs._bytes_args(), *cs._dir_args(), d_val.data_ptr(), d_count.data_ptr(), nc, 0 if dry else out.data_ptr(),
                                total, d_loc.data_ptr(), res.data_ptr(), s)
        torch.cuda.synchronize()
        verdict, needed = _words(res, 2)
        if verdict == 2 and damaged:
            raise CwError(-2, damaged)
        if dry:  # (verdict 1 with the bytes needed)
            total, out = needed, _zeros(needed, torch.uint8)
        elif verdict:
            raise CwError(-4, f"chunk store: the export of {total} bytes{whence} was refused with verdict {verdict} after its dry run")
    return out, total, d_loc


class ScrubReport:
    """What ``ChunkStore.scrub`` found: ``status`` (uint32, one per directory entry: 0 good, 1 malformed, 2 unsound entry, 3 digest
    mismatch, 4 orphan, 5 not selected), ``stats`` (cw_scrub_stats as a dict), ``damaged`` (the values with status 1, 2 or 3,
    ascending) and ``orphans`` (the values with status 4: they decode, but the index holds no digest to judge them by).  Stale after
    ``ChunkStore.renumber``: status is per directory entry and the values are the old ones."""

    def __init__(self, status, stats: dict, dir_base: int):
        self.status, self.stats = np.ascontiguousarray(status, dtype=np.uint32), stats
        at = lambda mask: (np.nonzero(mask)[0].astype(np.uint64) + np.uint64(dir_base))  # noqa: E731
        self.damaged = at((self.status >= 1) & (self.status <= 3))
        self.orphans = at(self.status == 4)

    @property
    def clean(self) -> bool:
        return len(self.damaged) == 0


LOCATE_TOTALS = ("groups", "dirty_cells", "located_cells", "ambiguous_cells", "suspects", "unprotected")  # d_result[1..7) of a locate


class GuardSuspects:
    """What ``ChunkStore.guard_locate`` read from the guard's syndromes: ``status`` (uint32, one per directory entry: 0 nothing, bit 0
    a byte of the entry is the one wrong byte of a located cell, bit 1 a byte of it lies in an ambiguous cell, 4 the entry is not
    protected and cannot be judged), ``located`` (the values with bit 0), ``ambiguous`` (with bit 1), ``unprotected`` (with 4),
    ``suspects`` (located or ambiguous), all ascending, and ``totals`` (LOCATE_TOTALS as a dict).  A hint, never a verdict: a scrub of
    the suspects decides.  Stale after ``ChunkStore.renumber``, like a ``ScrubReport``."""

    def __init__(self, status, totals: dict, dir_base: int):
        self.status, self.totals = np.ascontiguousarray(status, dtype=np.uint32), totals
        at = lambda mask: (np.nonzero(mask)[0].astype(np.uint64) + np.uint64(dir_base))  # noqa: E731
        self.located = at((self.status & 1) != 0)
        self.ambiguous = at((self.status & 2) != 0)
        self.unprotected = at(self.status == 4)
        self.suspects = at((self.status & 3) != 0)


TOTALS = ("nonzero", "nonzero_stored", "referenced", "referenced_stored", "shared", "shared_stored", "missing")  # d_totals[1..7]


class Account:
    """What ``ChunkStore.account`` computed for the recipes of one call: ``streams`` (an ACCOUNT_DTYPE record per recipe, in the order
    given), ``refcount`` (uint32 per directory entry: the positions that name it) and ``owner`` (uint32 per directory entry: the
    index of the one recipe that names it, ``Account.NONE`` or ``Account.SHARED``), ``totals`` (a dict: the words of d_totals under
    the names of ``TOTALS``, plus ``unreferenced_entries`` and ``unreferenced_stored``: what a ``compact`` that keeps these recipes
    drops).  Exact for the recipes passed and for the store as it was; stale after ``ChunkStore.renumber``, like a ScrubReport:
    ``refcount`` and ``owner`` are per directory entry."""
    NONE, SHARED = 0xFFFFFFFF, 0xFFFFFFFE

    def __init__(self, streams, refcount, owner, totals):
        self.streams = np.ascontiguousarray(streams, dtype=ACCOUNT_DTYPE)
        self.refcount, self.owner = np.ascontiguousarray(refcount, dtype=np.uint32), np.ascontiguousarray(owner, dtype=np.uint32)
        self.totals = dict(zip(TOTALS, (int(v) for v in totals)))
        self.totals["unreferenced_entries"] = self.totals["nonzero"] - self.totals["referenced"]
        self.totals["unreferenced_stored"] = self.totals["nonzero_stored"] - self.totals["referenced_stored"]


class Diff:
    """What ``ChunkStore.diff(old, new)`` found, from the recipes alone: ``ops`` (a DELTA_OP_DTYPE record per op; the ops tile the new
    stream back to back, each a copy out of the old stream or a run of new bytes), ``src`` (uint64 per position of ``new``: where its
    bytes lie in the old stream, or ``DeltaOp.NONE``) and ``totals`` (a dict under the names of ``DIFF_TOTALS``).  Offsets are
    zero-based.  Values only enter through equality, so a Diff is unchanged by ``renumber`` of both recipes and by ``compact``."""

    def __init__(self, ops, src, totals):
        self.ops = np.ascontiguousarray(ops, dtype=DELTA_OP_DTYPE).reshape(-1)
        self.src = np.ascontiguousarray(src, dtype=np.uint64).reshape(-1)
        self.totals = dict(zip(DIFF_TOTALS, (int(v) for v in totals)))

    def changed_ranges(self) -> list:
        """The new ops as ``(offset, length)`` in the new stream: what ``read_ranges(new, ...)`` takes."""
        new = self.ops[self.ops["a_off"] == np.uint64(DeltaOp.NONE)]
        return [(int(o), int(n)) for o, n in zip(new["b_off"], new["len"])]


DIFF_TOTALS = ("ops", "new_ops", "in_place_bytes", "moved_bytes", "new_bytes", "matched_positions", "positions")  # d_totals[1..7]


class Delta:
    """Version B for someone who holds version A as plain bytes (``ChunkStore.delta(old, new)``): ``ops`` as in a ``Diff``, ``payload``
    (uint8: the new ops' bytes back to back), ``old_bytes`` and ``new_bytes`` (the sizes of the two streams).  Plain host data:
    ``save`` / ``load`` use one ``.npz``; ``apply_delta(old, delta)`` needs no store and no index."""

    def __init__(self, ops, payload, old_bytes: int, new_bytes: int):
        self.ops = np.ascontiguousarray(ops, dtype=DELTA_OP_DTYPE).reshape(-1)
        self.payload = _np_u8(payload)
        self.old_bytes, self.new_bytes = int(old_bytes), int(new_bytes)

    def save(self, path) -> None:
        with open(path, "wb") as f:
            np.savez(f, ops=self.ops, payload=self.payload, old_bytes=np.uint64(self.old_bytes), new_bytes=np.uint64(self.new_bytes))

    @classmethod
    def load(cls, path) -> "Delta":
        with np.load(path) as z:
            return cls(z["ops"], z["payload"], int(z["old_bytes"]), int(z["new_bytes"]))


def apply_delta(old, delta: Delta) -> bytes:
    """The new stream's bytes from the old stream's and a ``Delta`` (``dev_apply_delta``): one upload, one call, one download.
    Nothing of the delta is trusted: raises CwError (-2) naming the first malformed op, or when the ops build another size than
    ``delta.new_bytes`` or ``old`` is not of ``delta.old_bytes`` bytes."""
    _need_device()
    import torch
    a = _np_u8(old)
    if a.size != delta.old_bytes:
        raise CwError(-2, f"delta: made against an old stream of {delta.old_bytes} bytes, not {a.size}")
    n, s = len(delta.ops), torch.cuda.current_stream().cuda_stream
    d_old, d_payload = _u8(a if a.size else np.zeros(1, np.uint8)), _u8(delta.payload if delta.payload.size else np.zeros(1, np.uint8))
    d_ops, d_n = _u8(delta.ops if n else np.zeros(1, DELTA_OP_DTYPE)), _u64([n])
    out, result = _zeros(delta.new_bytes, torch.uint8), _zeros(4)
    torch.cuda.synchronize()
    dev_apply_delta(d_old.data_ptr(), a.size, d_payload.data_ptr(), delta.payload.size, d_ops.data_ptr(), d_n.data_ptr(), n, out.data_ptr(),
                    delta.new_bytes, result.data_ptr(), s)
    torch.cuda.synchronize()
    verdict, total, bad, _ = _words(result)
    if verdict == 1:
        err = CwError(-2, f"delta: op {bad} of {n} is malformed")
        err.op = bad
        raise err
    if verdict or total != delta.new_bytes:
        raise CwError(-2, f"delta: the ops build {total} bytes, the delta says {delta.new_bytes}")
    return out.cpu().numpy()[:total].tobytes()


class Bundle:
    """Chunks on their way from one ChunkStore to another, as plain host data.  The manifest lists the n
    distinct chunks ``recipes`` name in ascending sender value: ``digests`` uint8[n, digest bytes], ``values`` uint64[n] (the
    sender's), ``locs`` LOC_DTYPE[n] (where the chunk lies in ``payload``; all zero = listed, not carried).  ``payload`` uint8 holds
    the carried chunks' stored bytes back to back, in the sender's stored form: sender and receiver share ``hash_alg`` and
    ``comp_alg``."""

    def __init__(self, digests, values, locs, payload, hash_alg, comp_alg, recipes):
        self.hash_alg, self.comp_alg = _hash_id(hash_alg), _comp_id(comp_alg)
        self.values = np.ascontiguousarray(values, dtype=np.uint64).reshape(-1)
        self.digests = np.ascontiguousarray(digests, dtype=np.uint8).reshape(len(self.values), digest_bytes(self.hash_alg))
        self.locs = np.ascontiguousarray(locs, dtype=LOC_DTYPE).reshape(-1)
        self.payload = np.ascontiguousarray(payload, dtype=np.uint8).reshape(-1)
        self.recipes = list(recipes)
        if len(self.locs) != len(self.values):
            raise ValueError(f"{len(self.values)} values, {len(self.locs)} locs")

    @property
    def carried(self) -> np.ndarray:
        """bool[n]: the chunks whose stored bytes the payload holds."""
        return (self.locs["pos"] != 0) | (self.locs["stored"] != 0) | (self.locs["raw"] != 0)

    def save(self, path) -> None:
        """One ``.npz``: manifest, payload, the algorithm ids and the recipes (refs and offsets concatenated, with their lengths)."""
        cat = lambda arrays: np.concatenate(arrays) if arrays else np.zeros(0, np.uint64)  # noqa: E731
        with open(path, "wb") as f:
            np.savez(f, hash_alg=np.int64(self.hash_alg), comp_alg=np.int64(self.comp_alg), digests=self.digests, values=self.values,
                     locs=self.locs, payload=self.payload, recipe_lens=np.array([len(r.refs) for r in self.recipes], np.uint64),
                     recipe_refs=cat([r.refs for r in self.recipes]), recipe_offsets=cat([r.offsets for r in self.recipes]))

    @classmethod
    def load(cls, path) -> "Bundle":
        with np.load(path) as z:
            lens, refs, offs = z["recipe_lens"].tolist(), z["recipe_refs"], z["recipe_offsets"]
            recipes, a = [], 0
            for i, k in enumerate(lens):
                recipes.append(Recipe(refs[a:a + k], offs[a + i:a + i + k + 1]))
                a += k
            return cls(z["digests"], z["values"], z["locs"], z["payload"], int(z["hash_alg"]), int(z["comp_alg"]), recipes)


def _folds(method):
    """A ChunkStore method that appends: while the store is protected it ends, refused or not, with one queued guard update."""
    @functools.wraps(method)
    def appending(self, *args, **kwargs):
        try:
            return method(self, *args, **kwargs)
        finally:
            self._fold()
    return appending


class ChunkStore:
    """A dedupe index with the bytes behind it: ``ingest`` chunks, dedupes and compresses a buffer and appends its new chunks to a
    device-resident store, ``restore`` turns a recipe back into bytes, ``read`` / ``read_ranges`` give byte ranges of it, ``compact`` forgets every stream but the ones named,
    ``renumber`` gives the directory slots of forgotten and duplicate chunks back, ``account`` says what each stream names alone
    (what dropping it gives back) and ``affected`` which streams a scrub's damaged chunks hurt.  ``renumber`` changes every value:
    recipes not passed to it, a ``ScrubReport`` and an ``Account`` taken before it are stale afterwards.
    The store is three torch buffers this object owns (bytes, cursor, directory: the caller-owned triple of cw_dev_store_chunks);
    chunk values count up from ``dir_base`` over the ingests.
    ``ingest`` is one device call: the whole buffer has to fit on the device next to its slots.  ``ingest_stream`` and
    ``restore_stream`` take and give host buffers of any size, streamed through the device in pieces (cw_store_ingest /
    cw_store_restore), ``ingest_many_stream`` and ``restore_many_stream`` many of them in one pipelined run; ``last_stats`` holds the
    last streamed ingest's statistics.  ``patch`` edits a stored stream in place -- ``write``, ``append``, ``truncate`` and
    ``patch_many`` are thin forms of it -- and ``last_patch`` holds the last edit's statistics (cw_patch_stats as a dict).  ``diff``
    says what changed between two recipes from the recipes alone, and ``delta`` packs the new version's new bytes with those ops for
    someone who holds the old version as plain bytes (``apply_delta``).  ``compose`` builds a new stored stream from ranges of stored
    streams and new bytes in one call -- ``apply_delta`` (a ``Delta`` applied inside the store), ``concat`` and ``edit`` (``patch_many``
    in one call) are thin forms of it -- and ``last_compose`` holds its statistics (cw_compose_stats as a dict).
    ``protect`` puts XOR guard stripes over the stored bytes: every method that appends then ends with one
    queued guard update, ``guard_check`` says which groups of stripes no longer match, and ``repair_local`` rebuilds the chunks a scrub
    found damaged from the guard, in place and without a peer.  ``protect(parity=2)`` keeps a second, GF(2^8)-weighted syndrome beside
    the XOR one (section 29): two damaged chunks that meet in a guard byte are then both rebuilt, and ``last_repair`` says how many
    chunks of the last ``repair_local`` needed it.  ``guard_locate`` reads the suspect chunks off the guard's syndromes in about the
    time of a ``guard_check`` (section 31), ``scrub(values=...)`` checks only those, and ``heal`` is locate, that scrub,
    ``repair_local`` and one more check in one call: a store that checks and mends itself without a full scrub."""
    last_stats = None
    last_patch = None
    last_compose = None
    last_repair = None
    d_guard = None  # the guard, with its cursor (d_covered) and its geometry (stripe, group), while the store is protected
    d_guard_q = None  # the second syndrome of a parity-2 store, as large as d_guard

    def __init__(self, index: DedupeIndex, comp_alg, params: CdcParams, store_bytes: int, dir_entries: int, dir_base: int = 0):
        import torch
        self.index, self.comp_alg, self.params = index, _comp_id(comp_alg), params
        self.store_bytes, self.dir_entries, self.dir_base = store_bytes, dir_entries, dir_base
        self.base = dir_base
        self.d_store = torch.zeros(max(store_bytes, 1), dtype=torch.uint8, device="cuda")
        self.d_used = torch.zeros(1, dtype=torch.int64, device="cuda")
        self.d_dir = torch.zeros(dir_entries * 2, dtype=torch.int64, device="cuda")  # 16 bytes per entry
        torch.cuda.synchronize()

    @staticmethod
    def _stream() -> int:
        import torch
        return torch.cuda.current_stream().cuda_stream

    def used(self) -> int:
        return int(self.d_used.item())

    # the stored bytes and the directory as the ABI's calls take them
    def _bytes_args(self) -> tuple:
        return self.d_store.data_ptr(), self.store_bytes

    def _dir_args(self) -> tuple:
        return self.d_dir.data_ptr(), self.dir_base, self.dir_entries

    def _triple(self) -> Store:
        return Store(*self._bytes_args(), self.d_used.data_ptr(), *self._dir_args())

    def protect(self, stripe: int = 65536, group: int = 16, parity: int = 1) -> None:
        """Put guard stripes over the store: a guard of store_bytes / group bytes and its cursor, then one
        update that folds in the bytes [0, used()).  ``stripe`` is a power of two in [65536, 2^30], ``group`` in [1, 256].  A store
        that is protected already gets a fresh guard of the new geometry.  ``parity=2`` adds the second syndrome (section 29): a
        second buffer of the same size, and ``group`` in [1, 255]."""
        import torch
        size = store_guard_bytes(max(self.store_bytes, 1), stripe, group)
        if size == 0:
            raise ValueError(f"stripe {stripe} is no power of two in [65536, 2^30] or group {group} is not in [1, 256]")
        if parity not in (1, 2):
            raise ValueError(f"parity {parity} is neither 1 nor 2")
        if parity == 2 and group > 255:
            raise ValueError(f"group {group} is not in [1, 255], the dual guard's bound")
        self.stripe, self.group = int(stripe), int(group)
        self.d_guard, self.d_covered, self._fold_result = _zeros(size, torch.uint8), _zeros(1), _zeros(4)
        self.d_guard_q = _zeros(size, torch.uint8) if parity == 2 else None
        torch.cuda.synchronize()  # (torch zeroed them on its own stream)
        self._fold()

    def _guard_call(self, single, dual, front: tuple, back: tuple) -> None:
        """One guard call of ops.py on this store's stream, ``single`` or ``dual`` by the store's parity: the store's bytes, ``front``
        (the call's arguments between them and the geometry), the geometry, the guard or guards and their size, ``back`` (the rest)."""
        guards = [self.d_guard.data_ptr()] + ([] if self.d_guard_q is None else [self.d_guard_q.data_ptr()])
        (single if self.d_guard_q is None else dual)(*self._bytes_args(), *front, self.stripe, self.group, *guards, self.d_guard.numel(), *back,
                                                     self._stream())

    def _fold(self) -> None:
        """The one guard update: queued, not synchronised.  Nothing when the store is not protected."""
        if self.d_guard is not None:
            self._guard_call(dev_store_guard_update, dev_store_guard2_update, (self.d_used.data_ptr(), self.d_covered.data_ptr()),
                             (self._fold_result.data_ptr(),))

    def protected_bytes(self) -> int:
        """The guard's cursor: the stored bytes [0, protected_bytes()) are folded in.  Equal to ``used()`` whenever a method has
        returned; 0 for a store that is not protected."""
        return 0 if self.d_guard is None else int(self.d_covered.item())

    def guard_check(self, detail: bool = False) -> tuple:
        """(count, groups): how many groups of stripes below the cursor differ from the guard, and which (``dev_store_guard_check``).
        A group differs when a stored byte in it changed, live or not, or a byte of the guard itself.  With ``detail``, a third
        element: for each of those groups, bit 0 when the XOR guard differs and bit 1 when the second syndrome of a parity-2 store
        does -- a changed stored byte sets both, a changed guard byte its own."""
        import torch
        self._need_guard()
        groups = self.d_guard.numel() // self.stripe
        bad, result = _zeros(groups, torch.int32), _zeros(4)
        torch.cuda.synchronize()
        self._guard_call(dev_store_guard_check, dev_store_guard2_check, (self.d_covered.data_ptr(),), (bad.data_ptr(), result.data_ptr()))
        torch.cuda.synchronize()
        verdict, checked, differ, _ = _words(result)
        if verdict:
            raise CwError(-4, f"chunk store: the guard's cursor {self.protected_bytes()} lies above the store's {self.store_bytes} bytes")
        bits = bad.cpu().numpy()[:checked]
        which = np.nonzero(bits)[0].tolist()
        return (differ, which, bits[which].tolist()) if detail else (differ, which)

    def guard_locate(self) -> GuardSuspects:
        """Which chunks the guard's syndromes suspect, in about the time of a ``guard_check`` (``dev_store_guard_locate``, DESIGN.md
        section 31): every entry with a byte in a guard cell that differs.  On a parity-2 store the two syndromes of a cell with one
        wrong byte name its member, and only the entry that holds that byte is suspected (``located``); everything else -- every
        cell of a parity-1 store, a damaged guard byte, two wrong bytes in one cell -- suspects every entry with a byte in the cell
        (``ambiguous``).  Raises CwError (-4) on a store that is not protected."""
        import torch
        self._need_guard()
        status, result = _zeros(self.dir_entries, torch.int32), _zeros(8)
        torch.cuda.synchronize()
        self._guard_call(dev_store_guard_locate, dev_store_guard2_locate, (*self._dir_args(), self.d_covered.data_ptr()),
                         (status.data_ptr(), result.data_ptr()))
        torch.cuda.synchronize()
        words = _words(result)
        if words[0]:
            raise CwError(-4, f"chunk store: the guard's cursor {self.protected_bytes()} lies above the store's {self.store_bytes} bytes")
        return GuardSuspects(status.cpu().numpy().view(np.uint32)[:self.dir_entries], dict(zip(LOCATE_TOTALS, words[1:7])), self.dir_base)

    def heal(self, verify: bool = True) -> dict:
        """Check and mend in one call, without a full scrub: ``guard_locate()``, then ``scrub(values=suspects)`` -- the digests decide,
        the syndromes only say where to look -- then ``repair_local`` of what that scrub found damaged, then one more ``guard_check``.
        With no suspects it stops after the locate: no scrub window runs.  Returns ``repair_local``'s dict and suspects, located,
        ambiguous (lists of values), cleared (the suspects the scrub found good: the price of ambiguity), windows (the scrub windows
        taken) and groups_left (the groups that still differ afterwards).  Groups can still differ for damage in bytes no live entry
        names, damage in the guard's own bytes, and chunks ``repair_local`` left out: neither the store nor the guard is written for
        these, and ``protect()`` again folds a fresh guard over the bytes as they are.  No byte is ever written on the syndromes'
        word alone: two wrong bytes in one cell can look like one wrong byte of a third member."""
        found = self.guard_locate()
        out = dict(repaired=[], collided=[], unprotected=[], failed=[], no_digest=[], suspects=found.suspects.tolist(),
                   located=found.located.tolist(), ambiguous=found.ambiguous.tolist(), cleared=[], windows=0, groups_left=0)
        if len(found.suspects):
            report = self.scrub(values=found)
            out.update(self.repair_local(report, verify))
            out["cleared"] = np.setdiff1d(found.suspects, report.damaged).tolist()
            out["windows"] = report.stats["windows"]
        if len(found.suspects) or found.totals["dirty_cells"]:
            out["groups_left"] = self.guard_check()[0]
        return out

    def _need_guard(self) -> None:
        if self.d_guard is None:
            raise CwError(-4, "chunk store: not protected (ChunkStore.protect comes first)")

    def _no_room(self, what: str, needed: int, used: int) -> CwError:
        err = CwError(-5, f"{what}: {needed} bytes do not fit behind {used} of {self.store_bytes}")
        err.needed = needed
        return err

    def _off_directory(self, what: str, k: int) -> CwError:
        return CwError(-5, f"{what}: values {self.base} .. {self.base + k} leave the directory [{self.dir_base}, {self.dir_base + self.dir_entries})")

    def _append(self, k: int, src, n: int, off, k_dev, cap: int, slots, sizes, new_idx, n_new, result, s: int) -> None:
        """``dev_store_chunks`` of the outputs of a fused call that found k chunks; ``base`` advances by k, or CwError (-5) with the
        index as it was before the fused call."""
        import torch
        dev_store_chunks(self.comp_alg, src.data_ptr(), n, off.data_ptr(), k_dev.data_ptr(), cap - 1, slots.data_ptr(), sizes.data_ptr(),
                         self.base, *self._bytes_args(), self.d_used.data_ptr(), *self._dir_args(), result.data_ptr(), s, new_idx.data_ptr(),
                         n_new.data_ptr())
        torch.cuda.synchronize()
        verdict, needed = _words(result)
        if verdict:
            # the fused call put the call's new chunks into the index and the store took none of them: they are exactly the entries
            # with values in [base, base + k) -- base never advanced over them -- so one retain over that range with no flag set
            # takes them out again, and a later ingest does not find them "known" under values that name nothing
            if k:
                none_live = _zeros(k, torch.int32)
                torch.cuda.synchronize()
                self.index.retain(none_live.data_ptr(), self.base, k)
            err = self._no_room("chunk store", needed, self.used()) if verdict == 1 else self._off_directory("chunk store", k)
            err.needed = needed  # (for the directory's refusal: _no_room has set it)
            raise err
        self.base += k

    def _fused_buffers(self, n: int, cap: int) -> tuple:
        """The outputs of a fused call over n bytes with room for cap offsets and of the ``_append`` behind it, unsynchronised."""
        import torch
        total = chunk_slots_bytes(self.comp_alg, n, cap - 1)
        return (total, _zeros(cap), _zeros(1), _zeros(cap * digest_bytes(self.index.hash_alg), torch.uint8), _zeros(cap),
                _zeros(cap, torch.int32), _zeros(1), torch.empty(total, dtype=torch.uint8, device="cuda"), _zeros(cap, torch.int32), _zeros(2))

    @_folds
    def ingest(self, data) -> Recipe:
        """Chunk, hash, dedupe and compress ``data`` in one device call, then append its new chunks.  Raises CwError (-5) when the
        store or the directory cannot take them (``e.needed`` = the bytes the call wanted); store, directory, index and ``base``
        are then as they were: the digests the fused call inserted are taken out of the index again (one ``index.retain`` over the
        call's values, a rebuild of the table), so the same or another buffer can be ingested once there is room."""
        import torch
        a = _np_u8(data)
        n, s = a.size, self._stream()
        src = torch.from_numpy(a.copy() if n else np.zeros(1, np.uint8)).cuda()
        cap = self.params.max_offsets(n)
        total, off, k_dev, dig, ref, new_idx, n_new, slots, sizes, result = self._fused_buffers(n, cap)
        torch.cuda.synchronize()
        k = self.index.dev_cdc_dedupe_compress(self.params, self.comp_alg, src.data_ptr(), n, True, self.base, off.data_ptr(), cap,
                                               k_dev.data_ptr(), dig.data_ptr(), ref.data_ptr(), new_idx.data_ptr(), n_new.data_ptr(),
                                               slots.data_ptr(), total, sizes.data_ptr(), s)
        self._append(k, src, n, off, k_dev, cap, slots, sizes, new_idx, n_new, result, s)
        return Recipe(ref.cpu().numpy().view(np.uint64)[:k], off.cpu().numpy().view(np.uint64)[:k + 1])

    @_folds
    def ingest_many(self, datas) -> list:
        """``ingest`` of many buffers at once: one upload of their concatenation, one fused call (``dev_cdc_streams_dedupe_compress``)
        and one ``dev_store_chunks``.  Every buffer is chunked as if alone, so the recipes, the store and the index are what a loop of
        ``ingest`` over ``datas`` leaves.  Returns one Recipe per buffer, its offsets starting at 0.  Raises as ``ingest`` does."""
        import torch
        parts = [_np_u8(d) for d in datas]
        if not parts:
            return []
        ends = np.cumsum([a.size for a in parts], dtype=np.uint64)
        n, nf, s = int(ends[-1]), len(parts), self._stream()
        src = torch.from_numpy(np.concatenate(parts) if n else np.zeros(1, np.uint8)).cuda()
        d_ends = torch.from_numpy(ends.view(np.int64)).cuda()
        cap = self.params.max_offsets_streams(n, nf)
        total, off, k_dev, dig, ref, new_idx, n_new, slots, sizes, result = self._fused_buffers(n, cap)
        first, ends_ok = _zeros(nf + 1), _zeros(1)
        torch.cuda.synchronize()
        k = self.index.dev_cdc_streams_dedupe_compress(self.params, self.comp_alg, src.data_ptr(), n, d_ends.data_ptr(), nf, self.base,
                                                       off.data_ptr(), cap, k_dev.data_ptr(), first.data_ptr(), ends_ok.data_ptr(),
                                                       dig.data_ptr(), ref.data_ptr(), new_idx.data_ptr(), n_new.data_ptr(), slots.data_ptr(),
                                                       total, sizes.data_ptr(), s)
        self._append(k, src, n, off, k_dev, cap, slots, sizes, new_idx, n_new, result, s)
        refs, offs = ref.cpu().numpy().view(np.uint64)[:k], off.cpu().numpy().view(np.uint64)[:k + 1]
        lo = first.cpu().numpy().view(np.uint64)
        starts = np.concatenate([np.zeros(1, np.uint64), ends[:-1]])
        return [Recipe(refs[a:b], offs[a:b + 1] - starts[f]) if b > a else Recipe([], [0])
                for f, (a, b) in enumerate(zip(lo[:-1].tolist(), lo[1:].tolist()))]

    @_folds
    def ingest_stream(self, data) -> Recipe:
        """``ingest`` for host data of any size, piece by piece with uploads beside the kernels.  When the index, the directory or
        the store cannot take a piece, raises CwError (-5) with ``e.consumed`` and ``e.nchunks`` (the bytes and chunks of the pieces that
        went in; ``base`` has advanced by them) and ``e.recipe``, which restores ``data[:e.consumed]``: make room, then ingest
        ``data[e.consumed:]``."""
        import torch
        a = _np_u8(data)
        torch.cuda.synchronize()  # (the buffers were filled on torch's stream)
        rc, refs, offs, consumed, stats = store_ingest(self.index, self.params, self.comp_alg, self._triple(), a.ctypes.data if a.size else 0,
                                                       a.size, self.base)
        self.base += len(refs)
        self.last_stats = stats
        recipe = Recipe(refs, offs)
        if rc:
            err = CwError(rc, lib().cw_last_error().decode(errors="replace"))
            err.consumed, err.nchunks, err.recipe = consumed, len(refs), recipe
            raise err
        return recipe

    @_folds
    def ingest_many_stream(self, datas) -> list:
        """``ingest_many`` for host buffers of any number and total size, piece by piece as ``ingest_stream`` (cw_store_ingest_streams):
        every buffer is chunked as if alone and may span pieces; the recipes, the store and the index are what ``ingest_many`` or a loop
        of ``ingest`` leaves.  Buffers that lie back to back in page-locked memory are read in place.  When a piece is refused, raises
        CwError (-5) with ``e.recipes`` (the complete streams), ``e.partial`` (the recipe of the stream that was cut, or None),
        ``e.streams_done``, ``e.consumed`` and ``e.nchunks``; ``base`` has advanced by ``e.nchunks``.  Make room, then go on with the
        buffers from ``e.streams_done``, the first shortened by ``e.partial.nbytes``."""
        import torch
        parts = [_np_u8(d) for d in datas]
        torch.cuda.synchronize()
        lens = np.array([a.size for a in parts], np.uint64)
        rc, refs, offs, first, consumed, done, stats = store_ingest_streams(self.index, self.params, self.comp_alg, self._triple(),
                                                                            [a.ctypes.data if a.size else 0 for a in parts], lens, self.base)
        self.base += len(refs)
        self.last_stats = stats
        lo = first.tolist()
        cut = lambda a, b: Recipe(refs[a:b], offs[a:b + 1] - offs[a]) if b > a else Recipe([], [0])  # noqa: E731
        recipes = [cut(a, b) for a, b in zip(lo[:done], lo[1:done + 1])]
        if rc:
            err = CwError(rc, lib().cw_last_error().decode(errors="replace"))
            err.recipes, err.streams_done, err.consumed, err.nchunks = recipes, done, consumed, len(refs)
            err.partial = cut(lo[done], lo[done + 1]) if done + 1 < len(lo) and lo[done + 1] > lo[done] else None
            raise err
        return recipes

    def restore_many_stream(self, recipes) -> list:
        """``restore_stream`` of many recipes in one pipelined run: the recipes are joined into one with the offsets shifted, restored
        by one cw_store_restore, and the bytes split again.  Raises as ``restore`` does."""
        refs, offs, starts, _ = _joined(list(recipes))
        whole = self.restore_stream(Recipe(refs, offs))
        return [whole[int(a):int(b)] for a, b in zip(starts[:-1], starts[1:])]

    def restore_stream(self, recipe: Recipe) -> bytes:
        """``restore`` into host memory, window by window with downloads beside the kernels.  Raises as ``restore`` does."""
        import torch
        out = np.zeros(max(recipe.nbytes, 1), np.uint8)
        torch.cuda.synchronize()
        _refuse_unrestored(store_restore(self.comp_alg, self._triple(), recipe.refs, recipe.offsets, out.ctypes.data, recipe.nbytes), recipe.refs)
        return out[:recipe.nbytes].tobytes()

    def restore(self, recipe: Recipe, verify: bool = False) -> bytes:
        """The bytes of an ingested stream.  Raises CwError (-2) unless every position restores.  verify: the restored chunks are
        hashed again and looked up in the index, and every answer has to be the recipe's ref."""
        import torch
        k, n, s = len(recipe.refs), recipe.nbytes, self._stream()
        d_ref, d_raw, d_count = _u64(recipe.refs if k else [0]), _u64(recipe.offsets - recipe.offsets[0]), _u64([k])
        out, status = _zeros(n, torch.uint8), _zeros(k, torch.int32)
        torch.cuda.synchronize()
        dev_restore_chunks(self.comp_alg, *self._bytes_args(), *self._dir_args(), d_ref.data_ptr(), d_raw.data_ptr(), d_count.data_ptr(), k,
                           out.data_ptr(), n, status.data_ptr(), s)
        if verify and k:
            dig, found, n_found = _zeros(k * digest_bytes(self.index.hash_alg), torch.uint8), _zeros(k), _zeros(1)
            torch.cuda.synchronize()  # (torch zeroed them on its own stream)
            dev_hash_chunks(self.index.hash_alg, out.data_ptr(), n, d_raw.data_ptr(), d_count.data_ptr(), k, dig.data_ptr(), s)
            self.index.dev_lookup(dig.data_ptr(), k, found.data_ptr(), n_found.data_ptr(), s)
        torch.cuda.synchronize()
        _refuse_unrestored(status.cpu().numpy()[:k], recipe.refs)
        if verify and k:
            got = found.cpu().numpy().view(np.uint64)
            bad = np.nonzero(got != recipe.refs)[0]
            if len(bad):
                raise CwError(-2, f"chunk store: verify failed at position {int(bad[0])}: the index answers {int(got[bad[0]])}, "
                                  f"the recipe says {int(recipe.refs[bad[0]])} ({len(bad)} positions differ)")
        return out.cpu().numpy()[:n].tobytes()

    def read_ranges(self, recipe: Recipe, ranges) -> list:
        """The bytes of the ranges ``(offset, length)`` of an ingested stream, in the recipe's own zero-based coordinates, without
        restoring the stream: one device call, the destinations packed back to back.  Raises CwError (-2) naming the first range
        with a status other than 0."""
        _need_device()
        import torch
        ranges = [(int(o), int(l)) for o, l in ranges]
        k, m, s = len(recipe.refs), len(ranges), self._stream()
        if m == 0:
            return []
        if any(o < 0 or l < 0 or o + l >= 1 << 64 for o, l in ranges):
            raise ValueError("ranges are (offset, length) with 0 <= offset, 0 <= length and offset + length < 2^64")
        lens = np.array([l for _, l in ranges], np.uint64)
        dsts = np.concatenate([[0], np.cumsum(lens, dtype=np.uint64)]).astype(np.uint64)
        total = int(dsts[-1])
        d_ref, d_raw, d_count = _u64(recipe.refs if k else [0]), _u64(recipe.offsets - recipe.offsets[0]), _u64([k])
        d_off, d_len, d_to, d_m = _u64([o for o, _ in ranges]), _u64(lens), _u64(dsts[:-1]), _u64([m])
        out, status = _zeros(total, torch.uint8), _zeros(m, torch.int32)
        torch.cuda.synchronize()
        dev_read_ranges(self.comp_alg, *self._bytes_args(), *self._dir_args(), d_ref.data_ptr(), d_raw.data_ptr(), d_count.data_ptr(), k,
                        d_off.data_ptr(), d_len.data_ptr(), d_to.data_ptr(), d_m.data_ptr(), m, out.data_ptr(), total, status.data_ptr(), s)
        torch.cuda.synchronize()
        st = status.cpu().numpy()
        if st.any():
            j = int(np.nonzero(st)[0][0])
            raise CwError(-2, f"chunk store: {int((st != 0).sum())} of {m} ranges not read; range {j} (offset {ranges[j][0]}, length "
                              f"{ranges[j][1]}) has status {int(st[j])}")
        host = out.cpu().numpy()
        return [host[int(dsts[i]):int(dsts[i + 1])].tobytes() for i in range(m)]

    def read(self, recipe: Recipe, offset: int, length: int) -> bytes:
        """Bytes [offset, offset + length) of an ingested stream: ``read_ranges`` with one range."""
        return self.read_ranges(recipe, [(offset, length)])[0]

    @_folds
    def patch(self, recipe: Recipe, offset: int, remove: int, data, lookahead: int = 0) -> Recipe:
        """The recipe of the stream with bytes [offset, offset + remove) replaced by ``data`` (cw_store_patch):
        only the chunks around the edit are rebuilt, re-chunked and stored, yet recipe, store and index are exactly what ingesting
        the whole edited stream leaves.  ``recipe`` stays valid: the store only appends, and the two versions share their chunks.
        ``base`` advances by the window's chunks and ``last_patch`` holds the call's statistics.  ``lookahead`` (0 = 4 * max_size)
        is how far behind the edit the first window reaches; it doubles until the cuts resynchronise.  Raises CwError (-5) when the
        index, the directory, the store or the device's memory cannot take the window, and CwError (-2) when a position of the
        window does not restore or the edit leaves the stream; store, index and ``base`` are then unchanged."""
        _need_device()
        import torch
        offset, remove = int(offset), int(remove)
        if offset < 0 or remove < 0:
            raise ValueError("offset and remove are not negative")
        torch.cuda.synchronize()  # (the store was written on torch's stream)
        refs, offs, stats = store_patch(self.index, self.params, self.comp_alg, self._triple(), recipe.refs, recipe.offsets, offset, remove, data,
                                        self.base, lookahead)
        self.base += stats["window_chunks"]
        self.last_patch = stats
        return Recipe(refs, offs)

    def write(self, recipe: Recipe, offset: int, data) -> Recipe:
        """Overwrite: ``data`` replaces as many bytes from ``offset`` on as the stream has, so a write past the end extends it."""
        n = len(_np_u8(data))
        return self.patch(recipe, offset, max(min(n, recipe.nbytes - int(offset)), 0), data)

    def append(self, recipe: Recipe, data) -> Recipe:
        """``data`` behind the stream's last byte."""
        return self.patch(recipe, recipe.nbytes, 0, data)

    def truncate(self, recipe: Recipe, nbytes: int) -> Recipe:
        """The first ``nbytes`` bytes of the stream (no more than it has)."""
        nbytes = min(int(nbytes), recipe.nbytes)
        return self.patch(recipe, nbytes, recipe.nbytes - nbytes, b"")

    def patch_many(self, recipe: Recipe, edits) -> Recipe:
        """``patch`` for several edits ``(offset, remove, data)``, all in the coordinates of the stream as it is now: they must not
        overlap or share an offset with an insert (ValueError, before any of them runs) and are applied from the highest offset
        down, one ``patch`` each.  ``last_patch`` is the last applied edit's, the one with the lowest offset."""
        for o, r, d in reversed(self._sorted_edits(recipe, edits)):
            recipe = self.patch(recipe, o, r, d)
        return recipe

    @staticmethod
    def _sorted_edits(recipe: Recipe, edits) -> list:
        """``patch_many``'s edits in ascending order, or its ValueError."""
        edits = sorted(((int(o), int(r), d) for o, r, d in edits), key=lambda e: (e[0], e[1]))
        for (o, r, _), (o2, _, _) in zip(edits, edits[1:]):
            if o + r > o2 or (o == o2 and r == 0):
                raise ValueError(f"edits overlap: ({o}, {r}) and the one at {o2}")
        if any(o < 0 or r < 0 or o + r > recipe.nbytes for o, r, _ in edits):
            raise ValueError(f"an edit leaves the stream's {recipe.nbytes} bytes")
        return edits

    @_folds
    def _compose_call(self, sources, ops, payload, lookahead: int) -> Recipe:
        """One ``store_compose`` over the recipes ``sources`` joined as ``restore_many_stream`` joins them, with their stream index."""
        _need_device()
        import torch
        refs, offs, _, first = _joined(sources)
        torch.cuda.synchronize()  # (the store was written on torch's stream)
        out_refs, out_offs, stats = store_compose(self.index, self.params, self.comp_alg, self._triple(), refs, offs, ops, payload, self.base, lookahead,
                                                  first if len(sources) > 1 else None)
        self.base += stats["rebuilt_chunks"]
        self.last_compose = stats
        return Recipe(out_refs, out_offs)

    def compose(self, parts, lookahead: int = 0) -> Recipe:
        """The recipe of the stream that ``parts`` build, back to back: a part is ``(recipe, offset, length)`` -- bytes [offset, offset +
        length) of a stream this store holds -- or a bytes-like of new bytes (cw_store_compose).  Nothing is
        restored or re-ingested: chunks that a copied range holds whole keep their refs, only what lies between them is read back,
        re-chunked and stored, yet recipe, store and index are what ingesting the composed bytes leaves.  ``base`` advances by the rebuilt
        chunks and ``last_compose`` holds the call's statistics (cw_compose_stats as a dict).  Raises CwError (-5) when the index, the
        directory, the store or the device's memory cannot take the rebuilt chunks and CwError (-2) when a source range does not
        restore; store, index and ``base`` are then unchanged."""
        sources, where, ops, payload, b = [], {}, [], [], 0
        for part in parts:
            if isinstance(part, tuple) and len(part) == 3 and isinstance(part[0], Recipe):
                r, off, n = part[0], int(part[1]), int(part[2])
                if off < 0 or n < 0 or off + n > r.nbytes:
                    raise ValueError(f"a part ({off}, {n}) leaves its stream's {r.nbytes} bytes")
                if id(r) not in where:
                    where[id(r)] = sum(s.nbytes for s in sources)
                    sources.append(r)
                if n:
                    ops.append((b, n, where[id(r)] + off, DeltaOp.NONE))
                    b += n
            else:
                a = _np_u8(part)
                if a.size:
                    ops.append((b, a.size, DeltaOp.NONE, sum(p.size for p in payload)))
                    payload.append(a)
                    b += a.size
        return self._compose_call(sources, np.array(ops, dtype=DELTA_OP_DTYPE), np.concatenate(payload) if payload else np.zeros(0, np.uint8), lookahead)

    def apply_delta(self, old: Recipe, delta: Delta) -> Recipe:
        """Version B inside the store from version A's recipe and a ``Delta`` made against A: ``compose`` with the delta's ops and
        payload.  Nothing of the delta is trusted: raises CwError (-2) when it was made against another size than ``old.nbytes``, when
        its ops build another size than ``delta.new_bytes``, or naming the first malformed op."""
        _need_device()
        if delta.old_bytes != old.nbytes:
            raise CwError(-2, f"delta: made against an old stream of {delta.old_bytes} bytes, not {old.nbytes}")
        total = int(delta.ops["len"].sum(dtype=np.uint64)) if len(delta.ops) else 0
        if total != delta.new_bytes:
            raise CwError(-2, f"delta: the ops build {total} bytes, the delta says {delta.new_bytes}")
        new = self._compose_call([old], delta.ops, delta.payload, 0)
        if new.nbytes != delta.new_bytes:
            raise CwError(-4, f"delta: composed {new.nbytes} bytes, the delta says {delta.new_bytes}")
        return new

    def concat(self, recipes) -> Recipe:
        """The stored streams back to back as one stream: ``compose`` of their whole ranges."""
        return self.compose([(r, 0, r.nbytes) for r in recipes])

    def edit(self, recipe: Recipe, edits) -> Recipe:
        """``patch_many`` in one ``compose``: the same edits ``(offset, remove, data)``, the same refusals and the same result, without a
        device call and two synchronises per edit."""
        parts, at = [], 0
        for o, r, d in self._sorted_edits(recipe, edits):
            parts += [(recipe, at, o - at), d]
            at = o + r
        return self.compose(parts + [(recipe, at, recipe.nbytes - at)])

    def _diff_call(self, old: Recipe, new: Recipe, max_ops: int, ranges: bool):
        """One queued ``dev_recipe_diff`` of the two recipes with room for max_ops ops: the device buffers as a dict.  The caller
        synchronises."""
        import torch
        ka, kb, s = len(old.refs), len(new.refs), self._stream()
        t = dict(ref_a=_u64(old.refs if ka else [0]), off_a=_u64(old.offsets), na=_u64([ka]), ref_b=_u64(new.refs if kb else [0]),
                 off_b=_u64(new.offsets), nb=_u64([kb]), ops=_zeros(max_ops * 4), nops=_zeros(1), src=_zeros(kb), totals=_zeros(8))
        if ranges:
            t.update(new_off=_zeros(max_ops), new_len=_zeros(max_ops), new_dst=_zeros(max_ops), nnew=_zeros(1))
        torch.cuda.synchronize()  # (torch zeroed and copied on its own stream)
        ptr = lambda k: t[k].data_ptr() if k in t else 0  # noqa: E731
        dev_recipe_diff(ptr("ref_a"), ptr("off_a"), ptr("na"), ka, ptr("ref_b"), ptr("off_b"), ptr("nb"), kb, self.dir_base, self.dir_entries,
                        ptr("ops") if max_ops else 0, max_ops, ptr("nops"), ptr("totals"), s, ptr("src"), ptr("new_off"), ptr("new_len"),
                        ptr("new_dst"), ptr("nnew"))
        return t

    @staticmethod
    def _refuse_recipes(verdict: int) -> None:
        if verdict == 1:
            raise CwError(-2, "chunk store: a recipe's offsets do not ascend in extents of 1 to 65536 bytes")

    def diff(self, old: Recipe, new: Recipe, max_ops: int = 4096) -> Diff:
        """What changed between two recipes of this store (``dev_recipe_diff``): no data is read, equal refs
        mean equal bytes.  One call with room for ``max_ops`` ops, and a second one with the room the first reported when that was too
        little.  Raises CwError (-2) when a recipe's offsets are not what the library writes."""
        _need_device()
        import torch
        for attempt in range(2):
            t = self._diff_call(old, new, max_ops, False)
            torch.cuda.synchronize()
            totals = _words(t["totals"])
            self._refuse_recipes(totals[0])
            if totals[0] == 0:
                return Diff(t["ops"].cpu().numpy().view(DELTA_OP_DTYPE)[:totals[1]], t["src"].cpu().numpy().view(np.uint64)[:len(new.refs)],
                            totals[1:])
            max_ops = totals[1]  # (verdict 2: the dry run that sized the buffer)
        raise CwError(-4, f"chunk store: the diff was refused with verdict {totals[0]} after its dry run")

    def delta(self, old: Recipe, new: Recipe) -> Delta:
        """``new`` as a ``Delta`` against ``old``: the diff and, queued directly behind it, ``dev_read_ranges`` of the new ops' bytes
        over ``new``, with one synchronise (room for one op per position and for every byte of ``new``).  Raises CwError (-2) naming
        the first range whose status is not 0 (a damaged stored chunk, say), or when a recipe's offsets are not what the library
        writes."""
        _need_device()
        import torch
        kb, nbytes, s = len(new.refs), new.nbytes, self._stream()
        cap = max(kb, 1)
        payload, status = _zeros(nbytes, torch.uint8), _zeros(cap, torch.int32)
        t = self._diff_call(old, new, cap, True)
        dev_read_ranges(self.comp_alg, *self._bytes_args(), *self._dir_args(), t["ref_b"].data_ptr(), t["off_b"].data_ptr(), t["nb"].data_ptr(), kb,
                        t["new_off"].data_ptr(), t["new_len"].data_ptr(), t["new_dst"].data_ptr(), t["nnew"].data_ptr(), cap, payload.data_ptr(),
                        nbytes, status.data_ptr(), s)
        torch.cuda.synchronize()
        totals = _words(t["totals"])
        self._refuse_recipes(totals[0])
        if totals[0]:
            raise CwError(-4, f"chunk store: the diff of {kb} positions was refused with verdict {totals[0]}")
        ops = t["ops"].cpu().numpy().view(DELTA_OP_DTYPE)[:totals[1]]
        st = status.cpu().numpy()[:totals[2]]
        if st.any():
            j = int(np.nonzero(st)[0][0])
            off, length = int(t["new_off"][j].item()), int(t["new_len"][j].item())
            raise CwError(-2, f"chunk store: {int((st != 0).sum())} of {len(st)} new ranges not read; range {j} (offset "
                              f"{off - int(new.offsets[0])}, length {length}) has status {int(st[j])}")
        return Delta(ops, payload.cpu().numpy()[:totals[5]], old.nbytes, nbytes)

    def _mark(self, recipes, s: int):
        """(live: a u32 flag per directory entry; n_outside: the positions that name none) after ``dev_store_mark`` of every recipe."""
        import torch
        live, n_out = _zeros(self.dir_entries, torch.int32), _zeros(1)
        marks = [(_u64(r.refs), _u64([len(r.refs)]), len(r.refs)) for r in recipes if len(r.refs)]
        torch.cuda.synchronize()  # (torch zeroed and copied on its own stream)
        for d_ref, d_count, k in marks:
            dev_store_mark(d_ref.data_ptr(), d_count.data_ptr(), k, self.dir_base, self.dir_entries, live.data_ptr(), n_out.data_ptr(), s)
        return live, n_out

    def _refuse_outside(self, n_out, whose: str) -> None:
        """CwError (-2) when ``_mark`` counted positions outside the directory; the caller has synchronised."""
        outside = int(n_out.item())
        if outside:
            raise CwError(-2, f"chunk store: {outside} positions of the {whose} name no entry of the directory [{self.dir_base}, "
                              f"{self.dir_base + self.dir_entries})")

    def compact(self, keep, store_bytes: int | None = None) -> dict:
        """Forget every stream but the recipes in ``keep``: mark their chunks, move the marked chunks' stored bytes into a new store
        of ``store_bytes`` (default: as large as the old one, after a dry run) with a new directory, and drop the other chunks' digests
        from the index.  Values are not renumbered; a protected store gets a fresh guard over the new bytes.  Returns dict(kept, dropped, bytes_before, bytes_after, removed).  Raises CwError
        with ``e.needed`` (the bytes the kept chunks take) when the new store is too small (-5) or a kept chunk's entry is damaged
        (-2), and CwError -2 when a recipe names a value outside the directory; the store and the index are then unchanged, as they
        are when the index's retain fails."""
        import torch
        s, n = self._stream(), self.dir_entries
        new_dir, new_used, result = _zeros(n * 2), _zeros(1), _zeros(4)
        live, n_out = self._mark(keep, s)

        def run(d_new_store: int, new_bytes: int):
            dev_store_compact(*self._bytes_args(), self.d_dir.data_ptr(), n, live.data_ptr(), d_new_store, new_bytes, new_used.data_ptr(),
                              new_dir.data_ptr(), result.data_ptr(), s)
            torch.cuda.synchronize()
            verdict, needed, kept, dropped = _words(result)
            if verdict:
                err = CwError(-5 if verdict == 1 else -2, f"chunk store: the kept chunks' {needed} bytes do not fit into {new_bytes}"
                              if verdict == 1 else "chunk store: a kept chunk's directory entry is damaged")
                err.needed = needed
                raise err
            return needed, kept, dropped

        if store_bytes is None:
            try:
                run(0, 0)  # the dry run: verdict 1 with the bytes needed, unless nothing is kept
            except CwError as e:
                if e.code != -5:
                    raise
            store_bytes = self.store_bytes
        self._refuse_outside(n_out, "kept recipes")  # (only now: a damaged kept entry wins over an outside position)
        new_store = _zeros(store_bytes, torch.uint8)
        torch.cuda.synchronize()
        bytes_before = self.used()
        needed, kept, dropped = run(new_store.data_ptr(), store_bytes)
        removed = self.index.retain(live.data_ptr(), self.dir_base, n)
        self.d_store, self.d_used, self.d_dir, self.store_bytes = new_store, new_used, new_dir, store_bytes
        if self.d_guard is not None:
            self.protect(self.stripe, self.group, 2 if self.d_guard_q is not None else 1)  # every kept byte moved: a fresh guard over the new store
        return dict(kept=kept, dropped=dropped, bytes_before=bytes_before, bytes_after=needed, removed=removed)

    def renumber(self, recipes, dir_entries: int | None = None, dir_base: int | None = None) -> list:
        """Give directory slots back: the K non-zero directory entries get the dense values [dir_base, dir_base + K) of a new
        directory of ``dir_entries`` entries (default: as many as now; ``dir_base`` default: as now), ``recipes`` are translated
        and the index's values change in place; ``base`` becomes dir_base + K.  No stored byte moves.  Renumbering never forgets --
        that is ``compact``'s job -- so the full rotation is ``store.compact(keep)`` then ``keep = store.renumber(keep)``.
        Returns the translated recipes in the order given, offsets unchanged; the ones passed in are not modified and are stale
        afterwards, as is every recipe of this store that was not passed, a ``ScrubReport`` and any list of values taken before
        the call.  A ``Bundle`` carries its own values and is not; ``save`` / ``load`` keep ``dir_base`` and ``base`` as they are.
        Everything that can refuse comes before anything shared changes, so a refusal leaves store, index and recipes as they
        were: CwError (-5) with ``e.needed`` = K when ``dir_entries`` < K; CwError (-2) when a recipe names no stored chunk (a
        dropped one, say); CwError (-2) with ``e.stale`` when the index holds that many values of this directory that no entry
        carries -- chunks dropped from the directory but not from the index: compact first."""
        import torch
        recipes = list(recipes)
        s, n, old_base = self._stream(), self.dir_entries, self.dir_base
        new_base = old_base if dir_base is None else int(dir_base)
        res = _zeros(4)
        torch.cuda.synchronize()  # (torch zeroed on its own stream)
        # 1. the dry run: K
        dev_store_renumber(self.d_dir.data_ptr(), old_base, n, 0, new_base, 0, new_base, 0, 0, 0, 0, res.data_ptr(), s)
        torch.cuda.synchronize()
        K = _words(res)[1]
        new_entries = max(n, K) if dir_entries is None else int(dir_entries)
        if new_entries < max(K, 1):
            err = CwError(-5, f"chunk store: {K} stored chunks do not fit a directory of {new_entries} entries")
            err.needed = K
            raise err
        # 2. the new directory and the pairs, into fresh buffers
        new_dir, d_from, d_to, d_np = _zeros(new_entries * 2), _zeros(K), _zeros(K), _u64([K])
        torch.cuda.synchronize()
        dev_store_renumber(self.d_dir.data_ptr(), old_base, n, 0, new_base, new_dir.data_ptr(), new_base, new_entries,
                           d_from.data_ptr() if K else 0, d_to.data_ptr() if K else 0, K, res.data_ptr(), s)
        # 3. every recipe into a new array
        n_missing = _zeros(1)
        work = [(_u64(r.refs), _u64([len(r.refs)]), _zeros(len(r.refs))) if len(r.refs) else None for r in recipes]
        torch.cuda.synchronize()
        for r, w in zip(recipes, work):
            if w is not None:
                dev_translate_refs(w[0].data_ptr(), w[1].data_ptr(), len(r.refs), d_from.data_ptr(), d_to.data_ptr(), d_np.data_ptr(), K,
                                   w[2].data_ptr(), n_missing.data_ptr(), s)
        torch.cuda.synchronize()
        verdict, kept, next_base = _words(res, 3)
        if verdict or kept != K:
            raise CwError(-4, f"chunk store: the renumbering of {K} entries was refused with verdict {verdict} after its dry run")
        missing = int(n_missing.item())
        if missing:
            raise CwError(-2, f"chunk store: {missing} positions of the recipes name no stored chunk of the directory [{old_base}, "
                              f"{old_base + n})")
        # 4. the index: refuses, unchanged, when it holds a value of the old range that no entry carries
        res3 = _zeros(3)
        torch.cuda.synchronize()
        self.index.dev_revalue(d_from.data_ptr(), d_to.data_ptr(), d_np.data_ptr(), K, old_base, n, res3.data_ptr(), s)
        torch.cuda.synchronize()
        verdict, _, stale = _words(res3)
        if verdict:
            err = CwError(-2, f"chunk store: the index holds {stale} values of the directory [{old_base}, {old_base + n}) that no "
                              "entry carries (chunks dropped from the directory only): compact first")
            err.stale = stale
            raise err
        # 5. nothing can refuse any more
        self.d_dir, self.dir_entries, self.dir_base, self.base = new_dir, new_entries, new_base, next_base
        return [Recipe(w[2].cpu().numpy().view(np.uint64)[:len(r.refs)], r.offsets.copy()) if w is not None else Recipe([], r.offsets.copy())
                for r, w in zip(recipes, work)]

    def account(self, recipes, flagged=None) -> Account:
        """Per-stream accounting and reverse references for ``recipes`` (``dev_store_account``): one upload of
        the concatenated refs with their stream index, one call, one synchronise.  ``streams[i].unique_stored`` is what dropping
        recipe i alone lets ``compact`` give back, given that the other recipes passed are all that is kept.  ``flagged`` is None, a
        ``ScrubReport`` (its damaged entries are flagged) or a uint32 array with one element per directory entry (any non-zero
        value is a flag); ``flagged_positions`` / ``flagged_bytes`` say how much of each stream sits in flagged chunks.  The distinct
        entries a stream names among the shared ones are not counted: ``account([r])`` alone gives them as ``unique_chunks``.  No
        recipes: an empty Account, the device untouched."""
        recipes = list(recipes)
        n = self.dir_entries
        if not recipes:
            return Account(np.zeros(0, ACCOUNT_DTYPE), np.zeros(n, np.uint32), np.full(n, Account.NONE, np.uint32), [0] * len(TOTALS))
        import torch
        if isinstance(flagged, ScrubReport):
            flagged = ((flagged.status >= 1) & (flagged.status <= 3)).astype(np.uint32)
        if flagged is not None:
            flagged = np.ascontiguousarray(flagged, dtype=np.uint32).reshape(-1)
            if len(flagged) != n:
                raise ValueError(f"flagged has {len(flagged)} elements, the directory {n} entries")
        first = np.concatenate([[0], np.cumsum([len(r.refs) for r in recipes])]).astype(np.uint64)
        k, nf, s = int(first[-1]), len(recipes), self._stream()
        d_ref, d_first = _u64(np.concatenate([r.refs for r in recipes]) if k else [0]), _u64(first)
        d_flag = None if flagged is None else _u8(flagged)
        acct, refcount, owner, totals = _zeros(nf * 8), _zeros(n, torch.int32), _zeros(n, torch.int32), _zeros(8)
        torch.cuda.synchronize()  # (torch zeroed and copied on its own stream)
        dev_store_account(d_ref.data_ptr(), d_first.data_ptr(), nf, k, *self._dir_args(), 0 if d_flag is None else d_flag.data_ptr(),
                          acct.data_ptr(), refcount.data_ptr(), owner.data_ptr(), totals.data_ptr(), s)
        torch.cuda.synchronize()
        t = _words(totals)
        if t[0]:
            raise CwError(-4, f"chunk store: the account of {nf} recipes was refused with verdict {t[0]}")
        return Account(acct.cpu().numpy().view(ACCOUNT_DTYPE)[:nf], refcount.cpu().numpy().view(np.uint32)[:n],
                       owner.cpu().numpy().view(np.uint32)[:n], t[1:])

    def affected(self, recipes, report: ScrubReport) -> list:
        """The recipes that a scrub's damaged chunks hurt: ``(index, flagged_positions, flagged_bytes)`` for every recipe of
        ``account(recipes, flagged=report)`` with a position in a damaged chunk, in the order given."""
        streams = self.account(recipes, flagged=report).streams
        return [(i, int(a["flagged_positions"]), int(a["flagged_bytes"])) for i, a in enumerate(streams) if a["flagged_positions"] > 0]

    def export_bundle(self, recipes, known=None) -> Bundle:
        """The chunks ``recipes`` name as a Bundle: their digests and values in ascending value (``dev_store_mark`` of every recipe,
        then ``dev_export_live``) and their stored bytes (``dev_store_export_chunks``, sized by a dry run).  ``known`` is a DedupeIndex
        on this device, or a ChunkStore standing for its index, typically the receiver's: chunks it holds are listed in the manifest
        but not carried.  Raises CwError (-2), the store untouched, when a recipe names a value outside the directory, when the
        index and the store disagree about a named value, or when a named chunk's entry is damaged."""
        import torch
        recipes = list(recipes)
        known = known.index if isinstance(known, ChunkStore) else known
        if known is not None and known.hash_alg != self.index.hash_alg:
            raise ValueError(f"known index hashes with algorithm {known.hash_alg}, this store with {self.index.hash_alg}")
        s, n, db = self._stream(), self.dir_entries, digest_bytes(self.index.hash_alg)
        live, n_out = self._mark(recipes, s)
        torch.cuda.synchronize()
        self._refuse_outside(n_out, "recipes")
        flagged = int(torch.count_nonzero(live).item())
        dig, val, res = _zeros(flagged * db, torch.uint8), _zeros(flagged), _zeros(3)
        torch.cuda.synchronize()
        self.index.dev_export_live(live.data_ptr(), self.dir_base, n, dig.data_ptr(), val.data_ptr(), flagged, res.data_ptr(), s)
        torch.cuda.synchronize()
        count, hits = _words(res, 2)
        values = val.cpu().numpy().view(np.uint64)[:flagged]
        if count != flagged or hits != flagged or (values == _MISS).any():
            raise CwError(-2, f"chunk store: the recipes name {flagged} chunks, the index holds {hits} entries with their values "
                              f"({int((values == _MISS).sum())} values have none): store and index disagree")
        carry = np.ones(flagged, bool)
        if known is not None and flagged:
            carry = _looked_up(known, dig, flagged, s) == _MISS
        locs, payload, nc = np.zeros(flagged, LOC_DTYPE), np.zeros(0, np.uint8), int(carry.sum())
        if nc:
            out, total, d_loc = _export_chunks(self, _u64(values[carry]), nc, s, damaged="chunk store: a named chunk's directory entry is damaged")
            locs[carry] = d_loc.cpu().numpy().view(LOC_DTYPE)[:nc]
            payload = out.cpu().numpy()[:total]
        return Bundle(dig.cpu().numpy()[:flagged * db], values, locs, payload, self.index.hash_alg, self.comp_alg, recipes)

    @_folds
    def import_bundle(self, bundle: Bundle, verify: bool = True) -> list:
        """Take a Bundle's chunks into this store and return its recipes in this store's values (offsets unchanged).  Chunks this
        store's index already holds keep their value here; the others are appended in manifest order under the values ``base`` + k,
        and ``base`` grows by the manifest's length.  Everything that can refuse comes before the index is touched, so a refusal
        leaves index, store, directory and ``base`` as they were: ValueError when codec or hash algorithm differ; CwError (-2) when
        the bundle lacks a chunk this store needs, when a needed chunk's place in the payload is unsound, when a recipe names a
        value the manifest lacks or -- with ``verify`` -- when a carried chunk does not restore from the bundle or does not hash to
        its manifest digest; CwError (-5) when the index, the directory or the store cannot take the new chunks."""
        import torch
        if bundle.comp_alg != self.comp_alg or bundle.hash_alg != self.index.hash_alg:
            raise ValueError(f"bundle of codec {bundle.comp_alg} / hash {bundle.hash_alg}, store of codec {self.comp_alg} / hash "
                             f"{self.index.hash_alg}")
        n, s, db = len(bundle.values), self._stream(), digest_bytes(self.index.hash_alg)
        if bundle.digests.shape != (n, db):
            raise ValueError(f"{n} values need digests of shape ({n}, {db}), not {bundle.digests.shape}")
        for r in bundle.recipes:
            if not np.isin(r.refs, bundle.values).all():
                raise CwError(-2, "chunk bundle: a recipe names a value the manifest lacks")
        if n == 0:
            return [Recipe(r.refs, r.offsets) for r in bundle.recipes]
        in_bytes = len(bundle.payload)
        d_dig, d_loc, d_in = _u8(bundle.digests), _u8(bundle.locs), _u8(bundle.payload if in_bytes else np.zeros(1, np.uint8))
        # 2. what this store lacks, read-only; every such chunk is carried, soundly, and there is room for all of them
        lacks, carried, locs = _looked_up(self.index, d_dig, n, s) == _MISS, bundle.carried, bundle.locs
        if (lacks & ~carried).any():
            raise CwError(-2, f"chunk bundle: {int((lacks & ~carried).sum())} chunks this store lacks are listed but not carried")
        stored, length, sound = locs["stored"].astype(np.int64), locs["raw"].astype(np.int64) & 0x1FFFF, _locs_sound(locs, in_bytes)
        if (lacks & ~sound).any():
            raise CwError(-2, f"chunk bundle: chunk {int(np.nonzero(lacks & ~sound)[0][0])}'s place in the payload is unsound")
        n_lacks, need, count, used = int(lacks.sum()), int(stored[lacks].sum()), self.index.count(), self.used()
        if count + n_lacks > self.index.max_entries:
            raise CwError(-5, f"chunk bundle: {count} entries + {n_lacks} new chunks > max_entries {self.index.max_entries}")
        if self.base + n > self.dir_base + self.dir_entries:
            raise self._off_directory("chunk bundle", n)
        if used + need > self.store_bytes:
            raise self._no_room("chunk bundle", need, used)
        # 3. the carried chunks restore from the bundle itself (the payload as the store, the locs as its directory) and hash to
        # the manifest's digests
        which = np.nonzero(carried)[0]
        if verify and len(which):
            if not sound[which].all():
                raise CwError(-2, f"chunk bundle: chunk {int(which[~sound[which]][0])}'s place in the payload is unsound")
            k = len(which)
            st, dig2 = self._restored_digests(d_in.data_ptr(), in_bytes, d_loc.data_ptr(), n, which, length[which])
            if st.any():
                j = int(np.nonzero(st)[0][0])
                raise CwError(-2, f"chunk bundle: {int((st != 0).sum())} of {k} carried chunks do not restore; chunk {int(which[j])} has "
                                  f"status {int(st[j])}")
            bad = np.nonzero((dig2 != bundle.digests[which]).any(axis=1))[0]
            if len(bad):
                raise CwError(-2, f"chunk bundle: {len(bad)} carried chunks do not hash to their manifest digest; the first is chunk "
                                  f"{int(which[bad[0]])}")
        # 4. the index, the store, the recipes
        ref, new_idx, n_new = _zeros(n), _zeros(n, torch.int32), _zeros(1)
        d_n, d_from, result, n_missing = _u64([n]), _u64(bundle.values), _zeros(2), _zeros(1)
        outs = [(_u64(r.refs), _u64([len(r.refs)]), len(r.refs)) for r in bundle.recipes]
        torch.cuda.synchronize()
        self.index.dev_dedupe(d_dig.data_ptr(), n, self.base, ref.data_ptr(), new_idx.data_ptr(), n_new.data_ptr(), s)
        dev_store_import_chunks(d_in.data_ptr(), in_bytes, d_loc.data_ptr(), d_n.data_ptr(), n, self.base, *self._bytes_args(),
                                self.d_used.data_ptr(), *self._dir_args(), result.data_ptr(), s, new_idx.data_ptr(), n_new.data_ptr())
        for d_r, d_k, k in outs:
            if k:
                dev_translate_refs(d_r.data_ptr(), d_k.data_ptr(), k, d_from.data_ptr(), ref.data_ptr(), d_n.data_ptr(), n, d_r.data_ptr(),
                                   n_missing.data_ptr(), s)
        torch.cuda.synchronize()
        verdict, total = _words(result)
        if verdict or int(n_missing.item()):
            raise CwError(-4, f"chunk bundle: admitted, yet the append was refused with verdict {verdict} ({total} bytes) or "
                              f"{int(n_missing.item())} recipe positions found no value")
        self.base += n
        return [Recipe(d_r.cpu().numpy().view(np.uint64)[:k], r.offsets) for (d_r, _, k), r in zip(outs, bundle.recipes)]

    def _restored_digests(self, d_in: int, in_bytes: int, d_loc: int, n_loc: int, which, lengths):
        """The chunks ``which`` (positions of the n_loc cw_chunk_loc entries at d_loc, each sound, with the given lengths) restored from
        the payload d_in[0..in_bytes) -- the payload as the store, the locs as its directory -- and hashed with this index's algorithm:
        (cw_dev_restore_chunks' statuses, the digests as uint8[k, digest bytes])."""
        import torch
        s, db = self._stream(), digest_bytes(self.index.hash_alg)
        cuts = np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint64)
        k, total = len(which), int(cuts[-1])
        d_ref, d_raw, d_count = _u64(which), _u64(cuts), _u64([k])
        out, status, dig2 = _zeros(total, torch.uint8), _zeros(k, torch.int32), _zeros(k * db, torch.uint8)
        torch.cuda.synchronize()
        dev_restore_chunks(self.comp_alg, d_in, in_bytes, d_loc, 0, n_loc, d_ref.data_ptr(), d_raw.data_ptr(), d_count.data_ptr(), k,
                           out.data_ptr(), total, status.data_ptr(), s)
        dev_hash_chunks(self.index.hash_alg, out.data_ptr(), total, d_raw.data_ptr(), d_count.data_ptr(), k, dig2.data_ptr(), s)
        torch.cuda.synchronize()
        return status.cpu().numpy()[:k], dig2.cpu().numpy()[:k * db].reshape(k, db)

    def replicate_to(self, other: "ChunkStore", recipes, verify: bool = True) -> list:
        """``other.import_bundle(self.export_bundle(recipes, known=other.index), verify)``: only the chunks ``other`` lacks travel, in
        their stored form, and ``other`` gets recipes of its own for the same streams."""
        return other.import_bundle(self.export_bundle(recipes, known=other.index), verify)

    def scrub(self, keep=None, values=None) -> ScrubReport:
        """Check every stored chunk once against the digest the index holds for its value (cw_store_scrub), in
        windows of CW_STORE_PIECE decoded bytes.  ``keep`` is a list of recipes: only the entries they name are checked, and a named
        entry that is missing shows as status 2; None checks every entry that is not all zero.  Raises CwError (-2) when a kept
        recipe names a value outside the directory.  ``values`` -- a list or array of values, or the ``GuardSuspects`` of
        ``guard_locate``, whose suspects are meant -- selects entries in the same way: only they are checked; a value outside the
        directory raises CwError (-2), and ``keep`` together with ``values`` is a ValueError."""
        import torch
        if keep is not None and values is not None:
            raise ValueError("scrub takes keep or values, not both")
        d_live = 0
        if values is not None:
            vals = np.ascontiguousarray(values.suspects if isinstance(values, GuardSuspects) else values, dtype=np.uint64).reshape(-1)
            idx, live = _entry_index(vals, self.dir_base, self.dir_entries), _zeros(self.dir_entries, torch.int32)
            if len(idx):
                live[torch.from_numpy(idx).cuda()] = 1
            d_live = live.data_ptr()
        if keep is not None:
            live, n_out = self._mark(keep, self._stream())
            torch.cuda.synchronize()
            self._refuse_outside(n_out, "kept recipes")
            d_live = live.data_ptr()
        torch.cuda.synchronize()  # (the store was written on torch's stream)
        status, stats = store_scrub(self.index, self.comp_alg, self._triple(), d_live)
        return ScrubReport(status, stats, self.dir_base)

    def _held_digests(self, values) -> tuple:
        """For the ascending values a report names: (their entries, the index's digests for them on the device, bool: it holds one)."""
        import torch
        idx, n, m = _entry_index(values, self.dir_base, self.dir_entries, report=True), self.dir_entries, len(values)
        live, dig, val, res = _zeros(n, torch.int32), _zeros(m * digest_bytes(self.index.hash_alg), torch.uint8), _zeros(m), _zeros(3)
        live[torch.from_numpy(idx).cuda()] = 1
        torch.cuda.synchronize()
        self.index.dev_export_live(live.data_ptr(), self.dir_base, n, dig.data_ptr(), val.data_ptr(), m, res.data_ptr(), self._stream())
        torch.cuda.synchronize()
        return idx, dig, val.cpu().numpy().view(np.uint64)[:m] != _MISS

    @_folds
    def repair_from(self, other: "ChunkStore", report: ScrubReport, verify: bool = True) -> dict:
        """Put the chunks ``report.damaged`` names back from ``other``, a store that holds them (one the streams were replicated to),
        in stored form and under their own values, so that every recipe stays valid.  The damaged values' digests come from this
        store's index, ``other``'s index finds them there, ``dev_store_export_chunks`` takes ``other``'s stored bytes out, and one
        ``dev_store_replace_chunks`` appends them here and repoints the entries; the old bytes stay until the next ``compact``.  A
        chunk is left out -- not a reason to refuse the rest -- when ``other`` lacks it, when its entry there is unsound or has
        another length than the entry here, or, with ``verify``, when it does not restore from the exported bytes or does not hash
        to the digest this index holds.  Returns dict(repaired, unavailable, no_digest): lists of values; no_digest are the damaged
        values this index holds no digest for.  ValueError when codec or hash algorithm differ; CwError (-5) with ``e.needed`` (the
        bytes wanted) when they do not fit behind ``used()``, nothing changed: ``compact`` makes room.  The index is never written."""
        import torch
        if other.comp_alg != self.comp_alg or other.index.hash_alg != self.index.hash_alg:
            raise ValueError(f"peer of codec {other.comp_alg} / hash {other.index.hash_alg}, store of codec {self.comp_alg} / hash "
                             f"{self.index.hash_alg}")
        damaged = np.unique(np.ascontiguousarray(report.damaged, dtype=np.uint64))
        out = dict(repaired=[], unavailable=[], no_digest=[])
        if len(damaged) == 0:
            return out
        # 1. the digests this index holds for the damaged values, in ascending value
        idx, dig, has = self._held_digests(damaged)
        out["no_digest"] = damaged[~has].tolist()
        # 2. where the peer keeps them
        s, m = self._stream(), len(damaged)
        there = _looked_up(other.index, dig, m, s)
        o_idx = there - np.uint64(other.dir_base)
        ok = has & (there != _MISS) & (there >= np.uint64(other.dir_base)) & (o_idx < np.uint64(other.dir_entries))
        o_idx = o_idx.astype(np.int64)
        entries = lambda cs, at: cs.d_dir.view(-1, 2)[torch.from_numpy(at).cuda()].cpu().numpy().reshape(-1).view(LOC_DTYPE)  # noqa: E731
        peer, mine = np.zeros(m, LOC_DTYPE), entries(self, idx)
        if ok.any():
            peer[ok] = entries(other, o_idx[ok])
        ok &= _locs_sound(peer, other.store_bytes)
        # (a replacement keeps the chunk's length, unless the entry here has no sound length of its own)
        len_here, len_there = mine["raw"].astype(np.int64) & 0x1FFFF, peer["raw"].astype(np.int64) & 0x1FFFF
        ok &= (len_here < 1) | (len_here > 65536) | (len_here == len_there)
        which = np.nonzero(ok)[0]
        nc = len(which)
        if nc:
            # 3. the peer's stored bytes, sized by a dry run
            payload, total, d_loc = _export_chunks(other, _u64(there[which]), nc, s, whence=" from the peer")
            locs = d_loc.cpu().numpy().view(LOC_DTYPE)[:nc].copy()
            good = np.ones(nc, bool)
            if verify:
                st, dig2 = self._restored_digests(payload.data_ptr(), total, d_loc.data_ptr(), nc, np.arange(nc), len_there[which])
                good = (st == 0) & (dig2 == dig.cpu().numpy().reshape(m, -1)[which]).all(axis=1)
            ok[which[~good]] = False
            which, locs = which[good], locs[good]
        out["unavailable"] = damaged[has & ~ok].tolist()
        if len(which) == 0:
            return out
        # 4. room, then one replace
        need, used = int(locs["stored"].astype(np.int64).sum()), self.used()
        if used + need > self.store_bytes:
            err = CwError(-5, f"chunk store: the repair's {need} bytes do not fit behind {used} of {self.store_bytes}")
            err.needed = need
            raise err
        d_loc2, d_val2, d_k, result = _u8(locs), _u64(damaged[which]), _u64([len(which)]), _zeros(2)
        torch.cuda.synchronize()
        dev_store_replace_chunks(payload.data_ptr(), total, d_loc2.data_ptr(), d_val2.data_ptr(), d_k.data_ptr(), len(which), *self._bytes_args(),
                                 self.d_used.data_ptr(), *self._dir_args(), result.data_ptr(), s)
        torch.cuda.synchronize()
        verdict, total = _words(result)
        if verdict:
            raise CwError(-4, f"chunk store: admitted, yet the replace was refused with verdict {verdict} ({total} bytes)")
        out["repaired"] = damaged[which].tolist()
        return out

    def repair_local(self, report: ScrubReport, verify: bool = True) -> dict:
        """Rebuild the chunks ``report.damaged`` names from the guard and the other stored bytes of their groups, and write them back
        in place, at their own ``pos``: no room is needed, the directory and every recipe stay as they are, and the guard stays
        exact.  The damaged values' digests come from this store's index, ``dev_store_guard_rebuild`` (sized by a dry run) rebuilds
        their stored bytes, and one ``dev_scatter_extents`` puts the good ones back.  A chunk is left out -- not a reason to refuse
        the rest -- when its extent shares a guard byte with another damaged chunk's (``collided``: neither can be told from the
        other), when its entry is missing, unsound or ends above ``protected_bytes()`` (``unprotected``), or, with ``verify``, when
        the rebuilt bytes do not decode or do not hash to the digest this index holds (``failed``: damage the report does not name,
        in the guard or in another chunk of the group).  Returns dict(repaired, collided, unprotected, failed, no_digest): lists of
        values; no_digest are the damaged values this index holds no digest for, which are skipped.  The index is never written.
        On a parity-2 store (``dev_store_guard2_rebuild``) two damaged chunks that meet in a guard byte are both rebuilt, and
        ``collided`` means three or more in one; ``last_repair`` = dict(paired): how many rebuilt chunks had such a partner."""
        import torch
        self._need_guard()
        self.last_repair = dict(paired=0)
        damaged = np.unique(np.ascontiguousarray(report.damaged, dtype=np.uint64))
        out = dict(repaired=[], collided=[], unprotected=[], failed=[], no_digest=[])
        if len(damaged) == 0:
            return out
        # 1. the digests this index holds for the damaged values, in ascending value
        idx, dig, has = self._held_digests(damaged)
        out["no_digest"] = damaged[~has].tolist()
        # 2. the rebuild: a dry run that sizes the payload, then the run that fills it
        s, m = self._stream(), len(damaged)
        d_val, d_count, d_loc, d_status, result = _u64(damaged), _u64([m]), _zeros(m * 2), _zeros(m, torch.int32), _zeros(5)
        payload, total = None, 0
        for dry in (True, False):
            torch.cuda.synchronize()
            self._guard_call(dev_store_guard_rebuild, dev_store_guard2_rebuild, (*self._dir_args(), self.d_covered.data_ptr()),
                             (d_val.data_ptr(), d_count.data_ptr(), m, 0 if dry else payload.data_ptr(), total, d_loc.data_ptr(),
                              d_status.data_ptr(), result.data_ptr()))
            torch.cuda.synchronize()
            verdict, needed = _words(result, 2)
            if verdict == 2:
                raise CwError(-4, f"chunk store: the guard's cursor lies above the store's {self.store_bytes} bytes")
            if dry:  # (verdict 1 with the bytes needed, unless nothing can be rebuilt)
                payload, total = _zeros(needed, torch.uint8), needed
            elif verdict:
                raise CwError(-4, f"chunk store: the rebuild of {total} bytes was refused with verdict {verdict} after its dry run")
        self.last_repair = dict(paired=_words(result, 5)[4])
        status = d_status.cpu().numpy().view(np.uint32)[:m]
        out["collided"], out["unprotected"] = damaged[has & (status == 1)].tolist(), damaged[has & (status == 2)].tolist()
        which = np.nonzero(has & (status == 0))[0]
        if len(which) == 0:
            return out
        locs = d_loc.cpu().numpy().view(LOC_DTYPE)[:m]
        good = np.ones(len(which), bool)
        if verify:
            # 3. the rebuilt chunks restore from the payload and hash to the digests this index holds
            st, dig2 = self._restored_digests(payload.data_ptr(), total, d_loc.data_ptr(), m, which, locs["raw"][which].astype(np.int64) & 0x1FFFF)
            good = (st == 0) & (dig2 == dig.cpu().numpy().reshape(m, -1)[which]).all(axis=1)
        # 4. back in place, in ascending pos: an extent that starts in front of the end of the one before it is left out
        mine = self.d_dir.view(-1, 2)[torch.from_numpy(idx[which]).cuda()].cpu().numpy().reshape(-1).view(LOC_DTYPE)
        ext, end = [], 0
        for j in np.argsort(mine["pos"], kind="stable"):
            pos, stored = int(mine["pos"][j]), int(mine["stored"][j])
            if good[j] and pos >= end:
                ext.append((int(locs["pos"][which[j]]), pos, stored))
                end = pos + stored
            else:
                good[j] = False
        out["failed"] = damaged[which[~good]].tolist()
        if ext:
            d_ext, d_n, result = _u64(np.array(ext, np.uint64)), _u64([len(ext)]), _zeros(4)
            torch.cuda.synchronize()
            dev_scatter_extents(payload.data_ptr(), total, d_ext.data_ptr(), d_n.data_ptr(), len(ext), *self._bytes_args(), result.data_ptr(), s)
            torch.cuda.synchronize()
            verdict = _words(result, 1)[0]
            if verdict:
                raise CwError(-4, f"chunk store: checked, yet the write-back of {len(ext)} extents was refused with verdict {verdict}")
        out["repaired"] = damaged[which[good]].tolist()
        return out

    def save(self, path) -> None:
        """One ``.npz``: the index's export, the store bytes [0, used), the directory, base and the parameters; of a protected store
        also the guard (the groups below its cursor), the cursor and the geometry, and of a parity-2 store the second syndrome."""
        dig, val = self.index.export()
        guard = {}
        if self.d_guard is not None:
            covered = self.protected_bytes()
            held = -(-covered // (self.stripe * self.group)) * self.stripe
            guard = dict(guard=self.d_guard[:held].cpu().numpy(), guard_covered=np.uint64(covered),
                         guard_geometry=np.array([self.stripe, self.group], np.uint64))
            if self.d_guard_q is not None:
                guard["guard_q"] = self.d_guard_q[:held].cpu().numpy()
        p = self.params
        gear = p._gear if getattr(p, "_gear", None) is not None else np.zeros(0, np.uint64)
        with open(path, "wb") as f:
            np.savez(f, hash_alg=np.int64(self.index.hash_alg), max_entries=np.int64(self.index.max_entries), digests=dig, values=val,
                     comp_alg=np.int64(self.comp_alg), store=self.d_store[:self.used()].cpu().numpy(), store_bytes=np.int64(self.store_bytes),
                     directory=self.d_dir.cpu().numpy(), dir_base=np.uint64(self.dir_base), base=np.uint64(self.base),
                     cdc=np.array([p.min_size, p.normal_size, p.max_size, p.mask_s, p.mask_l], np.uint64), gear=gear, **guard)

    @classmethod
    def load(cls, path) -> "ChunkStore":
        """A new index and fresh device buffers from a snapshot; protected when the snapshot holds a guard."""
        import torch
        with np.load(path) as z:
            cdc, gear = [int(v) for v in z["cdc"]], z["gear"]
            params = CdcParams(cdc[0], cdc[1], cdc[2], cdc[3], cdc[4], gear if len(gear) else None)
            index = DedupeIndex(int(z["hash_alg"]), int(z["max_entries"]))
            try:
                index.import_(z["digests"], z["values"])
                directory, store = z["directory"], z["store"]
                cs = cls(index, int(z["comp_alg"]), params, int(z["store_bytes"]), len(directory) // 2, int(z["dir_base"]))
                cs.base = int(z["base"])
                cs.d_store[:len(store)] = torch.from_numpy(store).cuda()
                cs.d_dir.copy_(torch.from_numpy(directory).cuda())
                cs.d_used.fill_(len(store))
                if "guard" in z.files:
                    held, (stripe, group) = z["guard"], (int(v) for v in z["guard_geometry"])
                    size = store_guard_bytes(max(cs.store_bytes, 1), stripe, group)
                    if size == 0 or len(held) > size:
                        raise CwError(-2, f"chunk store: the snapshot's guard ({len(held)} bytes, stripe {stripe}, group {group}) does not fit "
                                          f"a store of {cs.store_bytes} bytes")
                    cs.stripe, cs.group = stripe, group
                    cs.d_guard, cs.d_covered, cs._fold_result = _zeros(size, torch.uint8), _u64([int(z["guard_covered"])]), _zeros(4)
                    cs.d_guard[:len(held)] = torch.from_numpy(held).cuda()
                    if "guard_q" in z.files:
                        if len(z["guard_q"]) != len(held) or group > 255:
                            raise CwError(-2, f"chunk store: the snapshot's second syndrome ({len(z['guard_q'])} bytes, group {group}) does not "
                                              f"match its guard of {len(held)} bytes")
                        cs.d_guard_q = _zeros(size, torch.uint8)
                        cs.d_guard_q[:len(held)] = torch.from_numpy(z["guard_q"]).cuda()
                torch.cuda.synchronize()
            except Exception:
                index.close()
                raise
        return cs
