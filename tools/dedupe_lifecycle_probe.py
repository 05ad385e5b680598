#!/usr/bin/env python3
"""Timings of the dedupe index's lifecycle calls ("Lifecycle"): median of --reps after a warm-up.

  1. cw_dev_dedupe_lookup of 2^20 digests, all hits and all misses, beside cw_dev_dedupe of the same all-hit batch, in one index
     of 16 Mi max_entries (32 Mi slots) holding 8 Mi entries; Skein-512 and Skein-256-128.  Device events around each call, the
     three calls alternating within a rep.
  2. cw_dev_dedupe_export of a Skein-512 index of 16 Mi max_entries holding 4 Mi and 13 Mi entries.  Device events.  Bytes it has
     to move: state once (8 B per slot) + per entry the key and value read and written (2 x 72 B).
  3. cw_dedupe_resize of the 13 Mi-entry index from 16 Mi to 32 Mi max_entries (and back, so that every rep starts alike).  The
     call is synchronous and allocates and frees a table, so this is a host clock around it.  Bytes: the new table's state and
     min_idx cleared (12 B per new slot) + the old state read (8 B per old slot) + per entry key and value read and written
     (2 x 72 B) and one 8-byte CAS.
Rates are bytes over time; `of_hbm_peak` is that rate over the 8.0 TB/s the part is specified with.
    python tools/dedupe_lifecycle_probe.py [--reps 5] [--out profiles/r11_dedupe_lifecycle.json]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import compute_war_amd as cw  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--out", default="")
ap.add_argument("--scale", type=int, default=20, help="log2 of the unit the sizes above are multiples of (20 = Mi; smaller to rehearse)")
a = ap.parse_args()
cw.init(0)
s = torch.cuda.current_stream().cuda_stream
Mi = 1 << a.scale
HBM_PEAK = 8.0e12
rows = []


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def random_digests(n, db, seed):
    d = torch.empty(n * db, dtype=torch.uint8, device="cuda")
    cw.dev_gen_random(seed, 0, n, db, d.data_ptr(), s)
    return d.view(n, db)


def fill(idx, n, db, seed):
    """n fresh random digests into idx with values 0..n-1; returns them."""
    d = random_digests(n, db, seed)
    ref = torch.empty(n, dtype=torch.int64, device="cuda")
    new = torch.empty(n, dtype=torch.int32, device="cuda")
    k = torch.empty(1, dtype=torch.int64, device="cuda")
    idx.dev_dedupe(d.data_ptr(), n, 0, ref.data_ptr(), new.data_ptr(), k.data_ptr(), s)
    torch.cuda.synchronize()
    assert int(k.item()) == n
    return d


def report(row):
    rows.append(row)
    print(json.dumps(row), flush=True)


# ---- 1. lookup beside lookup-or-insert ---------------------------------------------------------------------------------------
n = Mi
for alg, db in (("skein512", 64), ("skein", 16)):
    idx = cw.DedupeIndex(alg, 16 * Mi)
    held = fill(idx, 8 * Mi, db, 0xA11)
    hits = held[torch.randperm(8 * Mi, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))[:n]].contiguous()
    misses = random_digests(n, db, 0xB22)
    del held
    ref = torch.empty(n, dtype=torch.int64, device="cuda")
    new = torch.empty(n, dtype=torch.int32, device="cuda")
    k = torch.empty(1, dtype=torch.int64, device="cuda")
    ms = dict(lookup_hits=[], lookup_misses=[], dedupe_hits=[])
    for rep in range(a.reps + 1):   # rep 0 warms up
        t = dict(lookup_hits=timed(lambda: idx.dev_lookup(hits.data_ptr(), n, ref.data_ptr(), k.data_ptr(), s)))
        assert int(k.item()) == n
        t["lookup_misses"] = timed(lambda: idx.dev_lookup(misses.data_ptr(), n, ref.data_ptr(), k.data_ptr(), s))
        assert int(k.item()) == 0
        t["dedupe_hits"] = timed(lambda: idx.dev_dedupe(hits.data_ptr(), n, 1 << 40, ref.data_ptr(), new.data_ptr(), k.data_ptr(), s))
        assert int(k.item()) == 0
        if rep:
            for key, v in t.items():
                ms[key].append(v)
    report(dict(kind="lookup", alg=alg, digests=n, entries=idx.count(), slots=2 * idx.max_entries,
                **{key + "_ms": float(np.median(v)) for key, v in ms.items()}, ms_all=ms))
    idx.close()
    del hits, misses, ref, new, k
    torch.cuda.empty_cache()

# ---- 2. export, 3. resize ----------------------------------------------------------------------------------------------------
db = 64
for entries in (4 * Mi, 13 * Mi):
    idx = cw.DedupeIndex("skein512", 16 * Mi)
    del_me = fill(idx, entries, db, 0xC33)
    del del_me
    torch.cuda.empty_cache()
    out_d = torch.empty(entries * db, dtype=torch.uint8, device="cuda")
    out_v = torch.empty(entries, dtype=torch.int64, device="cuda")
    k = torch.empty(1, dtype=torch.int64, device="cuda")
    slots = 2 * idx.max_entries
    ms = []
    for rep in range(a.reps + 1):
        t = timed(lambda: idx.dev_export(out_d.data_ptr(), out_v.data_ptr(), entries, k.data_ptr(), s))
        assert int(k.item()) == entries
        if rep:
            ms.append(t)
    nbytes = slots * 8 + entries * 2 * (db + 8)
    med = float(np.median(ms))
    report(dict(kind="export", alg="skein512", entries=entries, slots=slots, ms=med, ms_all=ms, bytes=nbytes, GBps=nbytes / med / 1e6,
                of_hbm_peak=nbytes / (med * 1e-3) / HBM_PEAK))
    del out_d, out_v
    torch.cuda.empty_cache()
    if entries == 13 * Mi:
        grow, shrink = [], []
        for rep in range(a.reps + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            idx.resize(32 * Mi)
            t1 = time.perf_counter()
            idx.resize(16 * Mi)
            t2 = time.perf_counter()
            if rep:
                grow.append((t1 - t0) * 1e3)
                shrink.append((t2 - t1) * 1e3)
        assert idx.count() == entries
        for name, v, old, new_slots in (("grow", grow, slots, 2 * slots), ("shrink", shrink, 2 * slots, slots)):
            nbytes = new_slots * 12 + old * 8 + entries * (2 * (db + 8) + 8)
            med = float(np.median(v))
            report(dict(kind="resize_" + name, alg="skein512", entries=entries, old_slots=old, new_slots=new_slots, ms=med, ms_all=v,
                        bytes=nbytes, GBps=nbytes / med / 1e6, of_hbm_peak=nbytes / (med * 1e-3) / HBM_PEAK,
                        clock="host, around the synchronous call (allocation and free included)"))
    idx.close()

if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rows, f, indent=1)
