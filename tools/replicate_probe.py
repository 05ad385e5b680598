"""Rates of the chunk bundle calls on one GPU.

--gib GiB of the tiled corpus of tools/restore_probe.py (1 MiB segments, a stamp every 1 KiB, no duplicate segments) ingested as
--streams streams of equal length into one cw.ChunkStore (LZ4, Skein-512): store A.  Then, for three sets of named streams (all,
every second, every ninth), with the sides of a comparison alternating:

  export_live   cw_dev_dedupe_export_live of the marked entries, against cw_dev_dedupe_export of the whole index;
  copy pair     cw_dev_store_export_chunks of the marked values into a payload plus cw_dev_store_import_chunks of that payload into
                an empty store (and each half alone), against cw_dev_store_compact of the same flags into a new store, and against
                a device-to-device hipMemcpyAsync of as many bytes.  The imported store must equal the compacted one byte for byte.

and, for receivers that hold none, every second and eight of nine of the streams already:

  replicate     one A.replicate_to(B, all recipes) (verify on), wall clock, against the route without bundles: every stream
                restored on A and ingested on B.  Both go through host memory, as the Python layer does; one run each, on receivers
                built alike.  Afterwards one stream is restored from B and compared with its input.

Device events for the device calls, one warm-up, median of --reps runs.  Prints one JSON object (and writes it to --out)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import compute_war_amd as cw  # noqa: E402
from tools.restore_probe import alternate, tiled_corpus  # noqa: E402


def note(text):
    print(text, file=sys.stderr, flush=True)   # progress: the run takes minutes


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=4.0)
    ap.add_argument("--streams", type=int, default=36)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    cw.init(0)
    hip = cw.lib()  # hipMemcpyAsync through the library's handle: the one HIP runtime of the process
    hip.hipMemcpyAsync.argtypes, hip.hipMemcpyAsync.restype = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p], C.c_int
    st = torch.cuda.current_stream().cuda_stream
    seg = 1 << 20
    per = max(1, int(args.gib * (1 << 30)) // seg // args.streams)      # segments per stream
    n_s, n = per * seg, per * seg * args.streams
    p = cw.CdcParams.default(8192)
    cap = p.max_offsets(n_s) * args.streams
    z = lambda count, dt: torch.zeros(count, dtype=dt, device="cuda")  # noqa: E731
    nseg = n // seg
    src = tiled_corpus(n)
    stamps = torch.arange(nseg * (seg // 1024), dtype=torch.int64, device="cuda").view(nseg, seg // 1024, 1)
    src.view(nseg, seg // 1024, 1024)[:, :, :8] = stamps.view(torch.uint8)
    host = src.cpu().numpy()
    del src, stamps
    stream_bytes = lambda s: host[s * n_s:(s + 1) * n_s]  # noqa: E731

    idx = cw.DedupeIndex("skein512", 1 << 20)
    A = cw.ChunkStore(idx, "lz4", p, n, cap)
    recipes = [A.ingest(stream_bytes(s)) for s in range(args.streams)]
    entries, used_bytes, chunks = idx.count(), A.used(), sum(len(r.refs) for r in recipes)
    res = {"bytes": n, "streams": args.streams, "codec": "lz4", "chunks": chunks, "index_entries": entries, "stored_bytes": used_bytes}
    note(f"ingested {n} bytes: {chunks} chunks, {used_bytes} stored")

    live, n_out, res3, res4 = z(cap, torch.int32), z(1, torch.int64), z(3, torch.int64), z(4, torch.int64)
    x_dig, x_val, x_n = z(entries * 64, torch.uint8), z(entries, torch.int64), z(1, torch.int64)
    l_dig, l_val, l_res = z(entries * 64, torch.uint8), z(entries, torch.int64), z(2, torch.int64)
    loc, payload = z(2 * entries, torch.int64), torch.empty(used_bytes, dtype=torch.uint8, device="cuda")
    new_store, new_used, new_dir = torch.empty(used_bytes, dtype=torch.uint8, device="cuda"), z(1, torch.int64), z(2 * cap, torch.int64)
    c_store, c_used, c_dir = torch.empty(used_bytes, dtype=torch.uint8, device="cuda"), z(1, torch.int64), z(2 * cap, torch.int64)
    plain = torch.empty(used_bytes, dtype=torch.uint8, device="cuda")
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.uint64).view(np.int64).copy()).cuda()  # noqa: E731

    for name, step in (("all", 1), ("second", 2), ("ninth", 9)):
        kept = list(range(0, args.streams, step))
        cat = up(np.concatenate([recipes[s].refs for s in kept]))
        cat_n = up([cat.numel()])
        live.zero_(); n_out.zero_()
        torch.cuda.synchronize()
        cw.dev_store_mark(cat.data_ptr(), cat_n.data_ptr(), cat.numel(), 0, cap, live.data_ptr(), n_out.data_ptr(), st)
        torch.cuda.synchronize()
        flagged = int(torch.count_nonzero(live).item())
        assert int(n_out.item()) == 0 and 0 < flagged <= entries

        def export_live():
            idx.dev_export_live(live.data_ptr(), 0, cap, l_dig.data_ptr(), l_val.data_ptr(), flagged, l_res.data_ptr(), st)

        def export_all():
            idx.dev_export(x_dig.data_ptr(), x_val.data_ptr(), entries, x_n.data_ptr(), st)

        t = alternate({"export_live": export_live, "export": export_all}, args.reps)
        torch.cuda.synchronize()
        assert l_res.tolist() == [flagged, flagged] and int(x_n.item()) == entries
        res.update({f"{name}_flagged": flagged, f"{name}_export_live_ms": t["export_live"], f"{name}_export_ms": t["export"],
                    f"{name}_export_live_vs_export": t["export"] / t["export_live"]})

        d_flagged = up([flagged])

        def export_chunks(d_out=payload.data_ptr(), room=used_bytes):
            cw.dev_store_export_chunks(A.d_store.data_ptr(), A.store_bytes, A.d_dir.data_ptr(), 0, cap, l_val.data_ptr(), d_flagged.data_ptr(), flagged,
                                       d_out, room, loc.data_ptr(), res3.data_ptr(), st)

        export_chunks(0, 0)                                   # the dry run
        torch.cuda.synchronize()
        kept_bytes = int(res3[1].item())
        assert int(res3[0].item()) == (1 if kept_bytes else 0) and int(res3[2].item()) == flagged

        def import_chunks():  # (the 8-byte memset is inside the timing, as in tools/restore_probe.py)
            new_used.zero_()
            cw.dev_store_import_chunks(payload.data_ptr(), kept_bytes, loc.data_ptr(), d_flagged.data_ptr(), flagged, 0, new_store.data_ptr(), used_bytes,
                                       new_used.data_ptr(), new_dir.data_ptr(), 0, cap, l_res.data_ptr(), st)

        def pair():
            export_chunks()
            import_chunks()

        def compact():
            cw.dev_store_compact(A.d_store.data_ptr(), A.store_bytes, A.d_dir.data_ptr(), cap, live.data_ptr(), c_store.data_ptr(), used_bytes,
                                 c_used.data_ptr(), c_dir.data_ptr(), res4.data_ptr(), st)

        def memcpy():
            assert hip.hipMemcpyAsync(plain.data_ptr(), A.d_store.data_ptr(), kept_bytes, 3, st) == 0   # hipMemcpyDeviceToDevice

        t = alternate({"pair": pair, "compact": compact, "memcpy": memcpy, "export_chunks": export_chunks, "import_chunks": import_chunks}, args.reps)
        torch.cuda.synchronize()
        assert int(res3[0].item()) == 0 and l_res.tolist() == [0, kept_bytes] and int(new_used.item()) == kept_bytes
        assert res4.tolist()[:3] == [0, kept_bytes, flagged]
        assert torch.equal(new_store[:kept_bytes], c_store[:kept_bytes]), name      # ascending values back to back: the compacted store
        res.update({f"{name}_kept_share_of_stored": kept_bytes / used_bytes, f"{name}_kept_bytes": kept_bytes, f"{name}_pair_ms": t["pair"],
                    f"{name}_export_chunks_ms": t["export_chunks"], f"{name}_import_chunks_ms": t["import_chunks"],
                    f"{name}_compact_ms": t["compact"], f"{name}_memcpy_ms": t["memcpy"], f"{name}_pair_GBps_of_kept": kept_bytes / t["pair"] / 1e6,
                    f"{name}_pair_vs_compact": t["compact"] / t["pair"], f"{name}_pair_vs_memcpy": t["memcpy"] / t["pair"],
                    f"{name}_export_chunks_vs_compact": t["compact"] / t["export_chunks"]})
        note(f"{name}: device calls timed")
    del payload, new_store, c_store, plain, x_dig, l_dig

    # ---- a whole replication against restore + ingest, for receivers that hold part of the streams already ----------------------------
    def receiver(have):
        b_idx = cw.DedupeIndex("skein512", 1 << 20)
        B = cw.ChunkStore(b_idx, "lz4", p, used_bytes + (64 << 20), 3 * cap, dir_base=1 << 32)
        for s in have:
            B.ingest(stream_bytes(s))
        return B

    for name, have in (("none", []), ("half", list(range(1, args.streams, 2))), ("most", [s for s in range(args.streams) if s % 9])):
        B = receiver(have)
        held = B.index.count()
        out = []
        t_rep = wall(lambda: out.extend(A.replicate_to(B, recipes)))
        new_chunks, new_bytes = B.index.count() - held, B.used()
        assert B.restore(out[0], verify=True) == stream_bytes(0).tobytes(), name      # (no receiver held stream 0)
        B.index.close()
        del B
        B = receiver(have)
        t_base = wall(lambda: [B.ingest(A.restore(r)) for r in recipes])
        assert B.index.count() - held == new_chunks and B.used() == new_bytes, name     # the same chunks went in, in the same stored form
        B.index.close()
        del B
        res.update({f"{name}_receiver_share_of_chunks": held / entries, f"{name}_new_chunks": new_chunks, f"{name}_replicate_ms": t_rep,
                    f"{name}_restore_ingest_ms": t_base, f"{name}_replicate_vs_restore_ingest": t_base / t_rep})
        note(f"receiver holding {name}: replicate {t_rep:.0f} ms, restore + ingest {t_base:.0f} ms")
    idx.close()
    print(json.dumps(res, indent=1))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
