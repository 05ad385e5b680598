#!/usr/bin/env python3
"""Timings of the dedupe index ("Dedupe index"): device events around each call, median of --reps calls after a warm-up.

  1. cw_dev_dedupe alone on 2^20 digests (Skein-512, Skein-256-128) with a duplicate fraction d in {0, 0.5, 1} (d = 1: one digest
     repeated, the all-identical batch), into an index that starts empty and into one already holding 8 Mi entries.  Every timed call gets a
     batch of its own (fresh random digests), so the prefilled index is probed, not re-hit.
  2. cw_dev_hash_dedupe_compress against cw_dev_hash_and_compress, GB/s of input, on corpus blocks made unique by a stamp:
     64 KiB Skein-512 + LZ4 and 4 KiB Skein-256 + LZ4, duplicates built on the device by indexing the unique set, d in {0, 0.5,
     0.9}.  Every rep restamps the unique set, so each call's unique blocks are new to the index (which keeps its scratch warm).
    python tools/dedupe_probe.py [--reps 5] [--out dedupe_probe.json]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import compute_war_amd as cw  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--out", default="")
ap.add_argument("--prefill", type=int, default=8 << 20)
a = ap.parse_args()
cw.init(0)
s = torch.cuda.current_stream().cuda_stream
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


def with_dups(uniq, n, d, seed):
    """n rows: the unique set once, the rest drawn from it (d = 1: all rows are row 0)."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    n_u = max(1, int(round(n * (1 - d))))
    idx = torch.cat([torch.arange(n_u, device="cuda"), torch.randint(0, n_u, (n - n_u,), device="cuda", generator=g)])
    idx = idx[torch.randperm(n, device="cuda", generator=g)]
    return uniq[:n_u][idx].contiguous()


# ---- 1. the dedupe step alone ---------------------------------------------------------------------------------------------
n = 1 << 20
ref = torch.empty(n, dtype=torch.int64, device="cuda")
new_idx = torch.empty(n, dtype=torch.int32, device="cuda")
n_new = torch.empty(1, dtype=torch.int64, device="cuda")
for alg, db in (("skein512", 64), ("skein", 16)):
    for prefill in (0, a.prefill):
        for d in (0.0, 0.5, 1.0):
            # one index per case, so the scratch is warm after rep 0; the timed calls add their new digests to it (capacity
            # 32 Mi slots either way: the load is <= 0.19 in the "empty" case and 0.28 - 0.44 in the prefilled one)
            idx = cw.DedupeIndex(alg, 16 << 20 if not prefill else prefill + (a.reps + 1) * n)
            if prefill:
                p = random_digests(prefill, db, 0xF111)
                pr = torch.empty(prefill, dtype=torch.int64, device="cuda")
                pn = torch.empty(prefill, dtype=torch.int32, device="cuda")
                idx.dev_dedupe(p.data_ptr(), prefill, 1 << 40, pr.data_ptr(), pn.data_ptr(), n_new.data_ptr(), s)
                del p, pr, pn
            ms = []
            for rep in range(a.reps + 1):   # rep 0 warms up
                batch = with_dups(random_digests(n, db, 1000 + rep), n, d, rep)
                torch.cuda.synchronize()
                t = timed(lambda: idx.dev_dedupe(batch.data_ptr(), n, rep * n, ref.data_ptr(), new_idx.data_ptr(), n_new.data_ptr(), s))
                if rep:
                    ms.append(t)
            rows.append(dict(kind="dedupe", alg=alg, digests=n, prefill=prefill, dup=d, ms=float(np.median(ms)), ms_all=ms,
                             count=idx.count()))
            print(json.dumps(rows[-1]), flush=True)
            idx.close()
del ref, new_idx
torch.cuda.empty_cache()


# ---- 2. the fused call against hash_and_compress ----------------------------------------------------------------------------
def corpus_unique(nb, bs):
    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "corpus", "canterbury")
    data = b"".join(open(os.path.join(root, f), "rb").read() for f in sorted(os.listdir(root)))
    one = torch.frombuffer(bytearray((data * (nb * bs // len(data) + 1))[:nb * bs]), dtype=torch.uint8).view(nb, bs).cuda()
    return one   # made distinct by the caller's stamp in the first 8 bytes of every block


for hash_alg, bs, nb in (("skein512", 65536, 16384), ("skein", 4096, 262144)):
    uniq = corpus_unique(nb, bs)
    db = cw.digest_bytes(hash_alg)
    stride = (cw.compress_bound("lz4", bs) + 15) // 16 * 16
    dst = torch.empty(nb * stride, dtype=torch.uint8, device="cuda")
    sizes = torch.empty(nb, dtype=torch.int32, device="cuda")
    dig = torch.empty((nb, db), dtype=torch.uint8, device="cuda")
    ref = torch.empty(nb, dtype=torch.int64, device="cuda")
    new_idx = torch.empty(nb, dtype=torch.int32, device="cuda")
    for d in (0.0, 0.5, 0.9):
        base_ms, fused_ms, k = [], [], 0
        idx = cw.DedupeIndex(hash_alg, (a.reps + 1) * nb)
        for rep in range(a.reps + 1):   # rep 0 warms up
            uniq[:, :8] = (torch.arange(nb, dtype=torch.int64, device="cuda") + rep * nb).view(nb, 1).view(torch.uint8)
            src = with_dups(uniq, nb, d, 7 + rep) if d else uniq
            torch.cuda.synchronize()
            t = timed(lambda: cw.dev_hash_and_compress(hash_alg, "lz4", src.data_ptr(), bs, nb, dig.data_ptr(), dst.data_ptr(), stride,
                                                       sizes.data_ptr(), s))
            out = {}
            tf = timed(lambda: out.setdefault("k", idx.dev_hash_dedupe_compress("lz4", src.data_ptr(), bs, nb, rep * nb, dig.data_ptr(),
                                                                                ref.data_ptr(), new_idx.data_ptr(), dst.data_ptr(),
                                                                                stride, sizes.data_ptr(), s)))
            k = out["k"]
            if rep:
                base_ms.append(t)
                fused_ms.append(tf)
            del src
        idx.close()
        gb = nb * bs / 1e9
        row = dict(kind="fused", hash=hash_alg, comp="lz4", block_bytes=bs, blocks=nb, dup=d, n_new=k,
                   hash_and_compress_ms=float(np.median(base_ms)), hash_dedupe_compress_ms=float(np.median(fused_ms)))
        row["hash_and_compress_GBps"] = gb / row["hash_and_compress_ms"] * 1e3
        row["hash_dedupe_compress_GBps"] = gb / row["hash_dedupe_compress_ms"] * 1e3
        rows.append(row)
        print(json.dumps(row), flush=True)
    del uniq, dst, sizes, dig, ref, new_idx
    torch.cuda.empty_cache()

if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rows, f, indent=1)
