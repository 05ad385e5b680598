"""Plain-numpy model of cw_dev_store_renumber and cw_dev_dedupe_revalue: the kept rule, the ranks, the placement, the verdicts and
the counts, as include/cw_hashcompress.h states them.  `*_loop` are the same calls as brute-force Python loops."""
import bisect

import numpy as np

LOC = np.dtype([("pos", "<u8"), ("stored", "<u4"), ("raw", "<u4")])
M = 1 << 64


def nonzero(directory):
    return (directory["pos"] != 0) | (directory["stored"] != 0) | (directory["raw"] != 0)


def verdict(K, new_base, new_dir_base, new_dir_entries, max_pairs):
    """2: [new_base, new_base + K) wraps or is not inside the new directory (an empty range is inside); else 1: K > max_pairs."""
    if K and (new_base + K >= M or new_base < new_dir_base or new_base + K > new_dir_base + new_dir_entries):
        return 2
    return 1 if K > max_pairs else 0


def renumber(directory, dir_base, live, new_base, new_dir_base, new_dir_entries, max_pairs):
    """(result[4], new_dir, d_from, d_to); the three arrays are None when the verdict is not 0."""
    nz = nonzero(directory)
    keep = nz if live is None else nz & (np.asarray(live) != 0)
    idx = np.nonzero(keep)[0]
    K = len(idx)
    v = verdict(K, new_base, new_dir_base, new_dir_entries, max_pairs)
    result = [v, K, (new_base + K) % M, int(nz.sum()) - K]
    if v:
        return result, None, None, None
    new_dir = np.zeros(new_dir_entries, LOC)
    first = new_base - new_dir_base if K else 0
    new_dir[first:first + K] = directory[idx]
    d_from = np.array([(dir_base + int(i)) % M for i in idx], np.uint64)
    d_to = np.array([new_base + k for k in range(K)], np.uint64)
    return result, new_dir, d_from, d_to


def renumber_loop(directory, dir_base, live, new_base, new_dir_base, new_dir_entries, max_pairs):
    kept, dropped = [], 0
    for i in range(len(directory)):
        pos, stored, raw = (int(x) for x in directory[i])
        if pos == 0 and stored == 0 and raw == 0:
            continue
        if live is None or int(live[i]) != 0:
            kept.append(i)
        else:
            dropped += 1
    K = len(kept)
    inside = K == 0 or (new_base + K < M and all(new_dir_base <= new_base + k < new_dir_base + new_dir_entries for k in range(K)))
    v = 2 if not inside else 1 if K > max_pairs else 0
    result = [v, K, (new_base + K) % M, dropped]
    if v:
        return result, None, None, None
    new_dir = np.zeros(new_dir_entries, LOC)
    d_from, d_to = np.zeros(K, np.uint64), np.zeros(K, np.uint64)
    for k, i in enumerate(kept):
        new_dir[new_base + k - new_dir_base] = directory[i]
        d_from[k], d_to[k] = (dir_base + i) % M, new_base + k
    return result, new_dir, d_from, d_to


def revalue(values, d_from, d_to, npairs, max_pairs, range_base, range_entries):
    """values: the value of every index entry, in any order.  (result[3], the values afterwards)."""
    p = min(npairs, max_pairs)
    frm = [int(x) for x in d_from[:p]]
    out, hits, stale = [], 0, 0
    for v in (int(x) for x in values):
        k = bisect.bisect_left(frm, v)
        if k < p and frm[k] == v:
            hits += 1
            out.append(int(d_to[k]))
        else:
            stale += (v - range_base) % M < range_entries
            out.append(v)
    if stale:
        return [1, hits, stale], [int(x) for x in values]
    return [0, hits, 0], out


def revalue_loop(values, d_from, d_to, npairs, max_pairs, range_base, range_entries):
    p = min(npairs, max_pairs)
    out, hits, stale = [], 0, 0
    for v in (int(x) for x in values):
        ks = [k for k in range(p) if int(d_from[k]) == v]
        if ks:
            hits += 1
            out.append(int(d_to[ks[0]]))
        else:
            stale += range_base <= v < range_base + range_entries
            out.append(v)
    return ([1, hits, stale], [int(x) for x in values]) if stale else ([0, hits, 0], out)
