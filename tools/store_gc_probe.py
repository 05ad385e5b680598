"""Rates of mark, compact and retain on one GPU.

--gib GiB of the tiled corpus of tools/restore_probe.py (1 MiB segments, a stamp every 1 KiB, no duplicate segments) ingested as
--streams streams of equal length, each through cw_dev_cdc_dedupe_compress (LZ4, Skein-512) and cw_dev_store_chunks into one store
and one index.  Then, for three sets of kept streams (all, every second, every ninth), with the two sides of a pair alternating:

  mark      cw_dev_store_mark over the kept recipes' positions in one call (and as one call per recipe), per Mi positions,
            against cw_dev_dedupe_lookup of as many digests;
  compact   cw_dev_store_compact into a new store and directory, per GB of kept stored bytes, against a device-to-device
            hipMemcpyAsync of as many bytes; and against cw_dev_store_chunks per stored byte (the whole input ingested as one
            stream into an index of its own, its append repeated into an empty store);
  retain    cw_dedupe_retain on a fresh copy of the index, against cw_dedupe_resize of a fresh copy to the same slot count.
            Both are synchronous host calls that allocate and clear the new table: wall-clock time around the call.

After each compaction one kept stream is restored from the new store and compared with its input.
Device events (wall clock for the two host calls), one warm-up, median of --reps runs.  Prints one JSON object (and writes it to --out)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import compute_war_amd as cw  # noqa: E402
from tools.restore_probe import alternate, tiled_corpus  # noqa: E402


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
    cap_s, cap = p.max_offsets(n_s), p.max_offsets(n_s) * args.streams
    z = lambda count, dt: torch.zeros(count, dtype=dt, device="cuda")  # noqa: E731
    nseg = n // seg
    src = tiled_corpus(n)
    stamps = torch.arange(nseg * (seg // 1024), dtype=torch.int64, device="cuda").view(nseg, seg // 1024, 1)
    src.view(nseg, seg // 1024, 1024)[:, :, :8] = stamps.view(torch.uint8)
    slots_bytes = cw.chunk_slots_bytes("lz4", n_s, cap_s - 1)
    slots, sizes = torch.empty(slots_bytes, dtype=torch.uint8, device="cuda"), z(cap_s, torch.int32)
    k_dev, n_new, new_idx, result = z(1, torch.int64), z(1, torch.int64), z(cap_s, torch.int32), z(4, torch.int64)
    dig, ref_all = z(cap * 64, torch.uint8), z(cap, torch.int64)
    store, used, directory = torch.empty(n, dtype=torch.uint8, device="cuda"), z(1, torch.int64), z(2 * cap, torch.int64)
    res = {"bytes": n, "streams": args.streams, "codec": "lz4"}

    # ---- cw_dev_store_chunks per stored byte at this size: the whole input as one stream, appended to an empty store --------------
    idx = cw.DedupeIndex("skein512", 1 << 20)
    cap_w = p.max_offsets(n)
    w_bytes = cw.chunk_slots_bytes("lz4", n, cap_w - 1)
    w_slots, w_sizes, w_offs, w_new = torch.empty(w_bytes, dtype=torch.uint8, device="cuda"), z(cap_w, torch.int32), z(cap_w, torch.int64), z(cap_w, torch.int32)
    w_dig, w_ref, w_dir = z(cap_w * 64, torch.uint8), z(cap_w, torch.int64), z(2 * cap_w, torch.int64)
    torch.cuda.synchronize()
    idx.dev_cdc_dedupe_compress(p, "lz4", src.data_ptr(), n, True, 0, w_offs.data_ptr(), cap_w, k_dev.data_ptr(), w_dig.data_ptr(), w_ref.data_ptr(),
                                w_new.data_ptr(), n_new.data_ptr(), w_slots.data_ptr(), w_bytes, w_sizes.data_ptr(), st)

    def append_whole():  # (the 8-byte memset is inside the timing, as in tools/restore_probe.py)
        used.zero_()
        cw.dev_store_chunks("lz4", src.data_ptr(), n, w_offs.data_ptr(), k_dev.data_ptr(), cap_w - 1, w_slots.data_ptr(), w_sizes.data_ptr(), 0,
                            store.data_ptr(), n, used.data_ptr(), w_dir.data_ptr(), 0, cap_w, result.data_ptr(), st, w_new.data_ptr(), n_new.data_ptr())

    t_append = alternate({"append": append_whole}, args.reps)["append"]
    torch.cuda.synchronize()
    assert int(result[0].item()) == 0
    append_bytes = int(result[1].item())
    res.update(append_ms=t_append, append_stored_bytes=append_bytes, append_GBps_of_stored=append_bytes / t_append / 1e6)
    idx.close()
    del w_slots, w_sizes, w_offs, w_new, w_dig, w_ref, w_dir
    used.zero_()
    idx = cw.DedupeIndex("skein512", 1 << 20)

    # ---- ingest: stream s has the values [first[s], first[s] + counts[s]) and its recipe in ref_all[first[s] ...] ----------------
    first, counts, offsets, base = [], [], [], 0
    for s in range(args.streams):
        d_src, offs = src.data_ptr() + s * n_s, z(cap_s, torch.int64)
        torch.cuda.synchronize()
        kk = idx.dev_cdc_dedupe_compress(p, "lz4", d_src, n_s, True, base, offs.data_ptr(), cap_s, k_dev.data_ptr(), dig.data_ptr() + base * 64,
                                         ref_all.data_ptr() + base * 8, new_idx.data_ptr(), n_new.data_ptr(), slots.data_ptr(), slots_bytes,
                                         sizes.data_ptr(), st)

        def append(d_store=store, d_used=used, d_dir=directory):
            cw.dev_store_chunks("lz4", d_src, n_s, offs.data_ptr(), k_dev.data_ptr(), cap_s - 1, slots.data_ptr(), sizes.data_ptr(), base,
                                d_store.data_ptr(), n, d_used.data_ptr(), d_dir.data_ptr(), 0, cap, result.data_ptr(), st, new_idx.data_ptr(),
                                n_new.data_ptr())

        append()
        torch.cuda.synchronize()
        assert int(result[0].item()) == 0, (s, result.tolist())
        first.append(base); counts.append(kk); offsets.append(offs[:kk + 1])
        if s < args.streams - 1:
            base += kk
    chunks, used_bytes, entries = base + counts[-1], int(used.item()), idx.count()
    res.update(chunks=chunks, index_entries=entries, stored_bytes=used_bytes)

    # ---- the index as device arrays, for fresh copies ----------------------------------------------------------------------------
    x_dig, x_val, x_n = z(entries * 64, torch.uint8), z(entries, torch.int64), z(1, torch.int64)
    torch.cuda.synchronize()
    idx.dev_export(x_dig.data_ptr(), x_val.data_ptr(), entries, x_n.data_ptr(), st)
    torch.cuda.synchronize()
    assert int(x_n.item()) == entries
    scratch_ref, scratch_new, scratch_n = z(entries, torch.int64), z(entries, torch.int32), z(1, torch.int64)

    def fresh_index():
        f = cw.DedupeIndex("skein512", 1 << 20)
        f.dev_insert(x_dig.data_ptr(), x_val.data_ptr(), entries, scratch_ref.data_ptr(), scratch_new.data_ptr(), scratch_n.data_ptr(), st)
        torch.cuda.synchronize()
        return f

    live, n_out = z(cap, torch.int32), z(1, torch.int64)
    new_store, new_used, new_dir = torch.empty(used_bytes, dtype=torch.uint8, device="cuda"), z(1, torch.int64), z(2 * cap, torch.int64)
    plain = torch.empty(used_bytes, dtype=torch.uint8, device="cuda")
    found, n_found = z(cap, torch.int64), z(1, torch.int64)
    out, status = torch.empty(n_s, dtype=torch.uint8, device="cuda"), z(cap_s, torch.int32)

    for name, step in (("all", 1), ("second", 2), ("ninth", 9)):
        kept = list(range(0, args.streams, step))
        # the kept recipes back to back, for the one-call mark
        cat = torch.cat([ref_all[first[s]:first[s] + counts[s]] for s in kept]).contiguous()
        cat_n = z(1, torch.int64) + cat.numel()
        ns = [z(1, torch.int64) + counts[s] for s in kept]
        positions = cat.numel()

        def mark_one():
            cw.dev_store_mark(cat.data_ptr(), cat_n.data_ptr(), positions, 0, cap, live.data_ptr(), n_out.data_ptr(), st)

        def mark_each():
            for s, d_n in zip(kept, ns):
                cw.dev_store_mark(ref_all.data_ptr() + first[s] * 8, d_n.data_ptr(), counts[s], 0, cap, live.data_ptr(), n_out.data_ptr(), st)

        def lookup():  # as many digests as the mark has positions (the first ones: every chunk's digest is in the index)
            idx.dev_lookup(dig.data_ptr(), min(positions, chunks), found.data_ptr(), n_found.data_ptr(), st)

        live.zero_(); n_out.zero_()
        torch.cuda.synchronize()
        t = alternate({"mark": mark_one, "lookup": lookup, "mark_each": mark_each}, args.reps)
        torch.cuda.synchronize()
        assert int(n_out.item()) == 0
        mi = positions / (1 << 20)
        res.update({f"{name}_positions": positions, f"{name}_mark_ms": t["mark"], f"{name}_lookup_ms": t["lookup"],
                    f"{name}_mark_per_recipe_ms": t["mark_each"], f"{name}_mark_Mi_positions_per_s": mi / t["mark"] * 1e3,
                    f"{name}_lookup_Mi_digests_per_s": min(positions, chunks) / (1 << 20) / t["lookup"] * 1e3,
                    f"{name}_mark_vs_lookup": t["lookup"] / t["mark"] * positions / min(positions, chunks)})

        def compact():
            cw.dev_store_compact(store.data_ptr(), n, directory.data_ptr(), cap, live.data_ptr(), new_store.data_ptr(), used_bytes,
                                 new_used.data_ptr(), new_dir.data_ptr(), result.data_ptr(), st)

        compact()
        torch.cuda.synchronize()
        verdict, kept_bytes, kept_entries, dropped = (int(v) for v in result.cpu().numpy().view("uint64"))
        assert verdict == 0 and int(new_used.item()) == kept_bytes, (name, verdict)

        def memcpy():
            assert hip.hipMemcpyAsync(plain.data_ptr(), store.data_ptr(), kept_bytes, 3, st) == 0   # hipMemcpyDeviceToDevice

        t = alternate({"compact": compact, "memcpy": memcpy}, args.reps)
        res.update({f"{name}_kept_share_of_stored": kept_bytes / used_bytes, f"{name}_kept_bytes": kept_bytes, f"{name}_kept_entries": kept_entries,
                    f"{name}_dropped_entries": dropped, f"{name}_compact_ms": t["compact"], f"{name}_memcpy_ms": t["memcpy"],
                    f"{name}_compact_GBps_of_kept": kept_bytes / t["compact"] / 1e6, f"{name}_memcpy_GBps": kept_bytes / t["memcpy"] / 1e6,
                    f"{name}_compact_vs_memcpy": t["memcpy"] / t["compact"],
                    f"{name}_compact_vs_append_per_byte": (kept_bytes / t["compact"]) / (append_bytes / t_append)})
        # the last kept stream, from the new store
        s = kept[-1]
        d_k = z(1, torch.int64) + counts[s]
        torch.cuda.synchronize()
        cw.dev_restore_chunks("lz4", new_store.data_ptr(), used_bytes, new_dir.data_ptr(), 0, cap, ref_all.data_ptr() + first[s] * 8,
                              offsets[s].data_ptr(), d_k.data_ptr(), counts[s], out.data_ptr(), n_s, status.data_ptr(), st)
        torch.cuda.synchronize()
        assert int(status[:counts[s]].abs().sum().item()) == 0 and torch.equal(out, src[s * n_s:(s + 1) * n_s]), (name, s)

        # retain and resize, each on a fresh copy of the index, to the same number of slots
        t_retain, t_resize, removed = [], [], 0
        for rep in range(args.reps + 1):                      # (the first round is the warm-up)
            f = fresh_index()
            box = []
            t_retain.append(wall(lambda: box.append(f.retain(live.data_ptr(), 0, cap, 1 << 21))))
            removed = box[0]
            assert f.count() == entries - removed
            f.close()
            f = fresh_index()
            t_resize.append(wall(lambda: f.resize(1 << 21)))
            f.close()
        t_retain, t_resize = statistics.median(t_retain[1:]), statistics.median(t_resize[1:])
        assert removed == dropped, (name, removed, dropped)
        res.update({f"{name}_retain_ms": t_retain, f"{name}_resize_ms": t_resize, f"{name}_removed": removed,
                    f"{name}_retain_vs_resize": t_resize / t_retain})
    idx.close()
    print(json.dumps(res, indent=1))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
