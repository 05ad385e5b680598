"""Cost of editing a stored stream in place on one GPU.

--gib GiB of the tiled corpus of tools/ingest_probe.py (1 MiB segments, a stamp every 1 KiB, so every chunk is new) in page-locked
host memory, cw_cdc_default_params(8192), ingested once per codec with cw_store_ingest.  Then, alternating in one session, every run
on the recipe of that first ingest and at a fresh random position:

  overwrite  cw_store_patch of 4 KiB of new bytes over 4 KiB
  insert     cw_store_patch inserting 1 MiB of new bytes
  append     cw_store_patch appending 64 KiB of new bytes
  read       cw.ChunkStore.read of the 4 KiB the overwrite replaces
  roundtrip  what an edit cost before: cw_store_restore of the whole stream into page-locked memory, the 4 KiB overwritten there,
             cw_store_ingest of all of it again (an insert would add a host memmove of the stream's tail to this)

Wall clock around the synchronous calls, one warm-up, median of --reps runs.  Every patched recipe's edited range is read back and
compared, and the cuts of one overwrite are compared with the round trip's.  Reports window_bytes, window_chunks and attempts of
every patch, and how many patches needed a second attempt with the default lookahead.  Prints one JSON object (and writes it to --out)."""
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
from tools.ingest_probe import pinned  # noqa: E402
from tools.restore_probe import tiled_corpus  # noqa: E402


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=4.0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    cw.init(0)
    n = int(args.gib * (1 << 30)) // (1 << 20) * (1 << 20)
    p = cw.CdcParams.default(8192)
    seg = 1 << 20
    nseg = n // seg
    h_src, src = pinned(n)
    h_dst, dst = pinned(n)
    dev = tiled_corpus(n).view(nseg, seg)
    stamps = torch.arange(nseg * (seg // 1024), dtype=torch.int64, device="cuda").view(nseg, seg // 1024, 1)
    dev.view(nseg, seg // 1024, 1024)[:, :, :8] = stamps.view(torch.uint8)
    src.copy_(dev.view(-1))
    torch.cuda.synchronize()
    del dev, stamps
    torch.cuda.empty_cache()
    host = src.numpy()
    rng = np.random.default_rng(25)
    fresh = lambda m: rng.integers(0, 256, m, dtype=np.uint8)  # noqa: E731
    runs = args.reps + 1
    res = {"bytes": n, "reps": args.reps, "lookahead": 4 * p.max_size}

    for alg in ("lz4", "lzf"):
        idx = cw.DedupeIndex("skein512", 1 << 22)
        cs = cw.ChunkStore(idx, alg, p, n + (256 << 20), (runs + 2) * p.max_offsets(n))
        t = time.perf_counter()
        rc, refs, cuts, consumed, _ = cw.store_ingest(idx, p, alg, cs._triple(), h_src, n, cs.base)
        res[f"{alg}_ingest_ms"] = (time.perf_counter() - t) * 1e3
        assert rc == 0 and consumed == n
        cs.base += len(refs)
        recipe = cw.Recipe(refs, cuts)
        res[f"{alg}_chunks"] = len(refs)
        patches, state = [], {}

        def patch(name, a, r, ins):
            new = cs.patch(recipe, a, r, ins)
            patches.append(dict(name=name, offset=a, **cs.last_patch))
            state[name] = (new, a, ins)

        def roundtrip():
            a, ins = int(rng.integers(0, n - 4096)), fresh(4096)
            status = cw.store_restore(alg, cs._triple(), recipe.refs, recipe.offsets, h_dst, n)
            assert not status.any()
            dst.numpy()[a:a + 4096] = ins
            rc, refs2, cuts2, consumed, _ = cw.store_ingest(idx, p, alg, cs._triple(), h_dst, n, cs.base)
            assert rc == 0 and consumed == n
            cs.base += len(refs2)
            state["roundtrip"] = (cw.Recipe(refs2, cuts2), a, ins)

        legs = {
            "overwrite": lambda: patch("overwrite", int(rng.integers(0, n - 4096)), 4096, fresh(4096)),
            "insert": lambda: patch("insert", int(rng.integers(0, n)), 0, fresh(1 << 20)),
            "append": lambda: patch("append", n, 0, fresh(65536)),
            "read": lambda: cs.read(recipe, state["overwrite"][1], 4096),
            "roundtrip": roundtrip,
        }
        times = {name: [] for name in legs}
        for name, fn in legs.items():
            wall(fn)
        del patches[:]
        for _ in range(args.reps):
            for name, fn in legs.items():
                times[name].append(wall(fn))
                if name in ("overwrite", "insert", "append"):       # the edited range reads back
                    new, a, ins = state[name]
                    assert cs.read(new, a, len(ins)) == ins.tobytes(), (alg, name)
        # one overwrite against the round trip of the same edit: the same cuts
        new, a, ins = state["roundtrip"]
        assert cs.patch(recipe, a, 4096, ins).offsets.tolist() == new.offsets.tolist(), alg
        assert cs.read(recipe, a, 4096) == host[a:a + 4096].tobytes(), alg     # (the old version is untouched)
        for name, ms in times.items():
            res[f"{alg}_{name}_ms"], res[f"{alg}_{name}_runs_ms"] = statistics.median(ms), ms
        res[f"{alg}_patches"] = patches
        res[f"{alg}_second_attempts"] = sum(q["attempts"] > 1 for q in patches)
        res[f"{alg}_roundtrip_over_overwrite"] = res[f"{alg}_roundtrip_ms"] / res[f"{alg}_overwrite_ms"]
        idx.close()
        del cs
        torch.cuda.empty_cache()
    print(json.dumps(res, indent=1))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
