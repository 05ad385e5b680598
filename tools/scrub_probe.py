"""Rates of scrub and repair on one GPU.

--gib GiB of the tiled corpus of tools/restore_probe.py (1 MiB segments, a stamp every 1 KiB, no duplicate segments) ingested as
--streams streams of equal length into one cw.ChunkStore (Skein-512), once per codec.  Then, with the sides alternating:

  floor         one cw_dev_restore_chunks plus one cw_dev_hash_chunks over all distinct chunks in a single call, into one buffer as
                large as the raw data: the work a scrub cannot avoid;
  scrub         cw_store_scrub of the whole directory at CW_STORE_PIECE = 64 MiB, 256 MiB and 1 GiB.  Every chunk must come out good.

Both are timed by the wall clock around a synchronised call (cw_store_scrub synchronises once per window itself): one warm-up, the
median of --reps rounds.  The fixed cost of a window is the slope between the 64 MiB and the 1 GiB run.

For LZ4 also a repair: the store is replicated to a second one, a byte is changed in every hundredth stored chunk, and scrub +
repair_from (verify on) is timed against the route without it: every affected stream restored from the peer and ingested into a
fresh store.  One run each.  Afterwards the store must scrub clean and one stream restore to its input.

Prints one JSON object (and writes it to --out)."""
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

PIECES = {"64MiB": 64 << 20, "256MiB": 256 << 20, "1GiB": 1 << 30}


def note(text):
    print(text, file=sys.stderr, flush=True)   # progress: the run takes minutes


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def alternate(configs, reps):
    """median ms of every configuration: one warm-up each, then reps rounds over all of them"""
    times = {name: [] for name in configs}
    for fn in configs.values():
        wall(fn)
    for _ in range(reps):
        for name, fn in configs.items():
            times[name].append(wall(fn))
    return {name: statistics.median(t) for name, t in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=4.0)
    ap.add_argument("--streams", type=int, default=36)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--codecs", default="lz4,lzf")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    cw.init(0)
    st = torch.cuda.current_stream().cuda_stream
    seg = 1 << 20
    per = max(1, int(args.gib * (1 << 30)) // seg // args.streams)      # segments per stream
    n_s, n = per * seg, per * seg * args.streams
    p = cw.CdcParams.default(8192)
    cap = p.max_offsets(n_s) * args.streams
    nseg = n // seg
    src = tiled_corpus(n)
    stamps = torch.arange(nseg * (seg // 1024), dtype=torch.int64, device="cuda").view(nseg, seg // 1024, 1)
    src.view(nseg, seg // 1024, 1024)[:, :, :8] = stamps.view(torch.uint8)
    host = src.cpu().numpy()
    del src, stamps
    stream_bytes = lambda s: host[s * n_s:(s + 1) * n_s]  # noqa: E731
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.uint64).view(np.int64).copy()).cuda()  # noqa: E731
    res = {"bytes": n, "streams": args.streams, "hash": "skein512"}

    for codec in args.codecs.split(","):
        idx = cw.DedupeIndex("skein512", 1 << 20)
        A = cw.ChunkStore(idx, codec, p, n, cap)
        recipes = [A.ingest(stream_bytes(s)) for s in range(args.streams)]
        d = A.d_dir.cpu().numpy().view(cw.LOC_DTYPE)
        full = np.nonzero(d["stored"])[0]
        lengths = (d["raw"][full] & 0x1FFFF).astype(np.uint64)
        k, raw_bytes = len(full), int(lengths.sum())
        r = {"chunks": sum(len(x.refs) for x in recipes), "distinct_chunks": k, "stored_bytes": A.used(), "raw_bytes_of_distinct": raw_bytes}
        note(f"{codec}: ingested {n} bytes, {k} distinct chunks, {A.used()} stored")

        d_ref, d_raw, d_k = up(full), up(np.concatenate([[0], np.cumsum(lengths)])), up([k])
        out = torch.empty(raw_bytes, dtype=torch.uint8, device="cuda")
        status, dig = torch.zeros(k, dtype=torch.int32, device="cuda"), torch.zeros(k * 64, dtype=torch.uint8, device="cuda")

        def floor():
            cw.dev_restore_chunks(codec, A.d_store.data_ptr(), A.store_bytes, A.d_dir.data_ptr(), 0, cap, d_ref.data_ptr(), d_raw.data_ptr(),
                                  d_k.data_ptr(), k, out.data_ptr(), raw_bytes, status.data_ptr(), st)
            cw.dev_hash_chunks("skein512", out.data_ptr(), raw_bytes, d_raw.data_ptr(), d_k.data_ptr(), k, dig.data_ptr(), st)

        stats = {}

        def scrub(name, piece):
            def run():
                with cw.tuned(CW_STORE_PIECE=piece):
                    stats[name] = cw.store_scrub(idx, codec, A._triple())[1]
            return run

        t = alternate({"floor": floor, **{name: scrub(name, piece) for name, piece in PIECES.items()}}, args.reps)
        assert not status.any()
        for name in PIECES:
            assert stats[name]["ok"] == stats[name]["checked"] == k and stats[name]["raw_bytes"] == raw_bytes, (name, stats[name])
            r[f"scrub_{name}_ms"], r[f"scrub_{name}_windows"] = t[name], stats[name]["windows"]
            r[f"scrub_{name}_vs_floor"] = t[name] / t["floor"]
            r[f"scrub_{name}_GBps_raw"] = raw_bytes / t[name] / 1e6
        r["floor_ms"], r["floor_GBps_raw"] = t["floor"], raw_bytes / t["floor"] / 1e6
        r["window_fixed_ms"] = (t["64MiB"] - t["1GiB"]) / max(1, stats["64MiB"]["windows"] - stats["1GiB"]["windows"])
        note(f"{codec}: floor {t['floor']:.1f} ms; scrub " + ", ".join(f"{name} {t[name]:.1f} ms" for name in PIECES))
        del out, dig, status

        if codec == "lz4":
            b_idx = cw.DedupeIndex("skein512", 1 << 20)
            B = cw.ChunkStore(b_idx, codec, p, n, 2 * cap, dir_base=1 << 32)
            b_all = A.replicate_to(B, recipes)
            hurt = full[::100]
            at = torch.from_numpy((d["pos"][hurt] + d["stored"][hurt] // 2).astype(np.int64)).cuda()
            A.d_store[at] ^= 0x5C
            torch.cuda.synchronize()
            hurt_values = set(hurt.tolist())
            affected = [s for s, x in enumerate(recipes) if hurt_values & set(x.refs.tolist())]
            box = {}
            t_scrub = wall(lambda: box.update(report=A.scrub()))
            found = len(box["report"].damaged)      # (a changed byte that decodes to the same bytes is no damage: rare, and counted)
            assert set(box["report"].damaged.tolist()) <= hurt_values and found > 0.9 * len(hurt), (found, len(hurt))
            t_repair = wall(lambda: box.update(out=A.repair_from(B, box["report"])))
            assert len(box["out"]["repaired"]) == found and A.scrub().clean
            assert A.restore(recipes[affected[0]], verify=True) == stream_bytes(affected[0]).tobytes()
            c_idx = cw.DedupeIndex("skein512", 1 << 20)
            Cs = cw.ChunkStore(c_idx, codec, p, n, cap)
            b_recipes = [b_all[s] for s in affected]
            t_base = wall(lambda: [Cs.ingest(B.restore(x)) for x in b_recipes])
            r.update({"repair_edited_chunks": len(hurt), "repair_damaged_chunks": found, "repair_affected_streams": len(affected), "repair_scrub_ms": t_scrub,
                      "repair_from_ms": t_repair, "repair_restore_ingest_ms": t_base, "repair_vs_restore_ingest": t_base / (t_scrub + t_repair),
                      "repair_from_vs_restore_ingest": t_base / t_repair})
            note(f"repair of {len(hurt)} chunks: scrub {t_scrub:.0f} ms + repair_from {t_repair:.0f} ms; restore + ingest of {len(affected)} streams "
                 f"{t_base:.0f} ms")
            for x in (b_idx, c_idx):
                x.close()
            del B, Cs
        idx.close()
        del A
        torch.cuda.empty_cache()
        res[codec] = r
    print(json.dumps(res, indent=1))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
