"""Cost of applying a delta inside the store, and of concatenating stored streams, on one GPU.

The store of tools/delta_probe.py: --gib GiB of the tiled corpus (a stamp every 1 KiB, so every chunk is new),
cw_cdc_default_params(8192), LZ4, ingested as --streams streams with cw_store_ingest_streams; A is their concatenation, stored once
more as one stream.  B_k = A after k random 4 KiB overwrites, k = 1, 16 and 256.  For every k, alternating in one session, wall
clock, the median of --reps runs of

  compose      cw.ChunkStore.apply_delta(A, delta): the delta applied inside the store (one cw_store_compose)
  patch_many   cw.ChunkStore.patch_many(A, edits): one cw_store_patch per edit
  round_trip   cw.ChunkStore.restore_stream(A) + cw.apply_delta(bytes, delta) + cw.ChunkStore.ingest_stream(bytes): what a receiver
               without cw_store_compose has to do

with the rounds, windows and merges of every compose, and once cw.ChunkStore.concat of the streams against restore_many_stream +
ingest_stream of the joined bytes.  Every result is compared with B_k's recipe (cuts).  Prints one JSON object (and writes it to --out)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import compute_war_amd as cw  # noqa: E402
from tools.restore_probe import tiled_corpus  # noqa: E402


def wall_ms(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=4.0)
    ap.add_argument("--streams", type=int, default=36)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    cw.init(0)
    n = int(args.gib * (1 << 30)) // (1 << 20) * (1 << 20)
    p = cw.CdcParams.default(8192)
    seg = 1 << 20
    nseg = n // seg
    dev = tiled_corpus(n).view(nseg, seg)
    stamps = torch.arange(nseg * (seg // 1024), dtype=torch.int64, device="cuda").view(nseg, seg // 1024, 1)
    dev.view(nseg, seg // 1024, 1024)[:, :, :8] = stamps.view(torch.uint8)
    data = dev.view(-1).cpu().numpy()
    del dev, stamps
    torch.cuda.empty_cache()
    rng = np.random.default_rng(27)
    alg = "lz4"
    idx = cw.DedupeIndex("skein512", 1 << 22)
    cs = cw.ChunkStore(idx, alg, p, 2 * n + (512 << 20), 4 * p.max_offsets(n))
    bounds = [n * f // args.streams // 4096 * 4096 for f in range(args.streams)] + [n]
    streams = cs.ingest_many_stream([data[a:b] for a, b in zip(bounds, bounds[1:])])
    res = {"bytes": n, "reps": args.reps, "codec": alg, "streams": args.streams}

    # concat of the stored streams against restore + ingest of the joined bytes
    ms_round, whole = wall_ms(lambda: cs.ingest_stream(b"".join(cs.restore_many_stream(streams))))
    ms, A = wall_ms(lambda: cs.concat(streams))
    assert A.offsets.tolist() == whole.offsets.tolist()
    res["concat"] = dict(compose_ms=ms, restore_ingest_ms=ms_round, chunks=len(A.refs), **cs.last_compose)

    for k in (1, 16, 256):
        at = np.sort(rng.choice((n - 4096) // 8192, k, replace=False)) * 8192 + int(rng.integers(0, 4096))
        edits = [(int(a), 4096, rng.integers(0, 256, 4096, dtype=np.uint8)) for a in at]
        B = cs.patch_many(A, edits)                                      # (stores B_k's new chunks: every leg below finds them stored)
        delta = cs.delta(A, B)
        row = dict(ops=len(delta.ops), payload_bytes=int(delta.payload.size))
        legs = {
            "compose": lambda: cs.apply_delta(A, delta),
            "patch_many": lambda: cs.patch_many(A, edits),
            "round_trip": lambda: cs.ingest_stream(cw.apply_delta(cs.restore_stream(A), delta)),
        }
        runs = {name: [] for name in legs}
        for _ in range(args.reps):                                       # alternating
            for name, fn in legs.items():
                ms, out = wall_ms(fn)
                assert out.offsets.tolist() == B.offsets.tolist(), name
                runs[name].append(ms)
                if name == "compose":
                    row.update(cs.last_compose)
        for name, r in runs.items():
            row[name + "_ms"], row[name + "_runs_ms"] = statistics.median(r), r
        res[f"k{k}"] = row
    idx.close()
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
