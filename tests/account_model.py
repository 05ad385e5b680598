"""Plain model of cw_dev_store_account, as include/cw_hashcompress.h states it: `account` is a loop over positions, `account_np`
the same with numpy.  Both return (verdict, streams, refcount, owner, totals): streams an ACCOUNT record per stream, refcount and
owner a uint32 per directory entry, totals the eight words of d_totals; with verdict 1 the other four are None."""
import numpy as np

LOC = np.dtype([("pos", "<u8"), ("stored", "<u4"), ("raw", "<u4")])
FIELDS = ("positions", "missing", "logical_bytes", "unique_chunks", "unique_stored", "unique_raw", "flagged_positions", "flagged_bytes")
ACCOUNT = np.dtype([(k, "<u8") for k in FIELDS])
M = 1 << 64
LEN_MASK = 0x1FFFF
NONE, SHARED = 0xFFFFFFFF, 0xFFFFFFFE


def verdict(first, max_positions) -> int:
    """1 when first[0] != 0, when a pair decreases or when first[-1] > max_positions."""
    f = [int(x) for x in first]
    return int(f[0] != 0 or any(a > b for a, b in zip(f[:-1], f[1:])) or f[-1] > max_positions)


def account(refs, first, directory, dir_base, flag, max_positions=None):
    first = [int(x) for x in first]
    nstreams, entries = len(first) - 1, len(directory)
    if verdict(first, len(refs) if max_positions is None else max_positions):
        return 1, None, None, None, None
    streams = np.zeros(nstreams, ACCOUNT)
    refcount, namers = np.zeros(entries, np.uint32), [set() for _ in range(entries)]
    for f in range(nstreams):
        for p in range(first[f], first[f + 1]):
            streams["positions"][f] += 1
            idx = (int(refs[p]) - dir_base) % M          # u64: a value below the base wraps out of range
            if idx >= entries or not any(int(v) for v in directory[idx]):
                streams["missing"][f] += 1
                continue
            length = int(directory[idx]["raw"]) & LEN_MASK
            streams["logical_bytes"][f] += length
            refcount[idx] += 1
            namers[idx].add(f)
            if flag is not None and int(flag[idx]) != 0:
                streams["flagged_positions"][f] += 1
                streams["flagged_bytes"][f] += length
    owner = np.full(entries, NONE, np.uint32)
    totals = [0] * 8
    for idx in range(entries):
        stored, nz = int(directory[idx]["stored"]), any(int(v) for v in directory[idx])
        totals[1] += nz
        totals[2] += stored if nz else 0
        if not namers[idx]:
            continue
        totals[3] += 1
        totals[4] += stored
        if len(namers[idx]) > 1:
            owner[idx] = SHARED
            totals[5] += 1
            totals[6] += stored
        else:
            (f,) = namers[idx]
            owner[idx] = f
            streams["unique_chunks"][f] += 1
            streams["unique_stored"][f] += stored
            streams["unique_raw"][f] += int(directory[idx]["raw"]) & LEN_MASK
    totals[7] = int(streams["missing"].sum())
    return 0, streams, refcount, owner, totals


def account_np(refs, first, directory, dir_base, flag, max_positions=None):
    first = np.asarray(first, np.uint64)
    nstreams, entries = len(first) - 1, len(directory)
    if verdict(first, len(refs) if max_positions is None else max_positions):
        return 1, None, None, None, None
    n = int(first[-1])
    refs = np.asarray(refs, np.uint64)[:n]
    stream = np.searchsorted(first, np.arange(n, dtype=np.uint64), side="right").astype(np.int64) - 1   # the last f with first[f] <= p
    idx = refs - np.uint64(dir_base)                      # wraps in u64
    nz = (directory["pos"] != 0) | (directory["stored"] != 0) | (directory["raw"] != 0)
    inside = idx < np.uint64(entries)
    at = np.where(inside, idx, np.uint64(0)).astype(np.int64)
    named = inside & nz[at]
    length = (directory["raw"].astype(np.uint64) & np.uint64(LEN_MASK))
    stored = directory["stored"].astype(np.uint64)
    streams = np.zeros(nstreams, ACCOUNT)
    streams["positions"] = np.diff(first)
    np.add.at(streams["missing"], stream[~named], 1)
    s, e = stream[named], at[named]
    np.add.at(streams["logical_bytes"], s, length[e])
    if flag is not None:
        hit = np.asarray(flag)[e] != 0
        np.add.at(streams["flagged_positions"], s[hit], 1)
        np.add.at(streams["flagged_bytes"], s[hit], length[e[hit]])
    refcount = np.zeros(entries, np.uint32)
    np.add.at(refcount, e, 1)
    lowest, highest = np.full(entries, M - 1, np.uint64), np.zeros(entries, np.uint64)
    np.minimum.at(lowest, e, s.astype(np.uint64))
    np.maximum.at(highest, e, s.astype(np.uint64))
    ref, one = refcount != 0, (refcount != 0) & (lowest == highest)
    owner = np.where(one, lowest, np.where(ref, SHARED, NONE)).astype(np.uint32)
    o = owner[one].astype(np.int64)
    np.add.at(streams["unique_chunks"], o, 1)
    np.add.at(streams["unique_stored"], o, stored[one])
    np.add.at(streams["unique_raw"], o, length[one])
    sh = ref & ~one
    totals = [0, int(nz.sum()), int(stored[nz].sum()), int(ref.sum()), int(stored[ref].sum()), int(sh.sum()), int(stored[sh].sum()),
              int((~named).sum())]
    return 0, streams, refcount, owner, totals
