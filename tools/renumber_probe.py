"""Rates of renumber and revalue on one GPU.

The store of tools/store_gc_probe.py: --gib GiB of the tiled corpus ingested as --streams streams of equal length (LZ4, Skein-512)
into one store and one index.  Then, for three sets of kept streams (all, every second, every ninth):

  renumber  cw_dev_store_renumber of the flagged entries into a new directory with its pairs, and its dry run, beside the dry run of
            cw_dev_store_compact over the same directory and flags (a flags pass, a scan and a finish: the floor).  Device events.
  revalue   cw_dev_dedupe_revalue through the renumbering's pairs, on a fresh copy of the index behind its cw_dedupe_retain, beside
            that retain and beside cw_dev_dedupe_export_live of the same flags.  Revalue and retain change the index, so each runs
            once per fresh copy: wall-clock time around the synchronised call; the export in device events.
  rotation  mark + compact + retain + renumber + translate (one call per kept recipe) + revalue, beside mark + compact + retain
            alone, and beside the only alternative without renumbering: every kept stream restored and ingested into a fresh store
            and a fresh index.  Wall-clock time, every step synchronised at its end.

After each rotation the last kept stream is restored through its translated recipe from the compacted store and the new directory,
its chunks are hashed and looked up in the revalued index, and every answer has to be the translated recipe's value.
One warm-up, median of --reps runs (the rebuild: one run behind one warm-up).  Prints one JSON object (and writes it to --out)."""
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
from tools.restore_probe import alternate, tiled_corpus  # noqa: E402


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def u64(t):
    return [int(v) for v in t.cpu().numpy().view(np.uint64)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=4.0)
    ap.add_argument("--streams", type=int, default=36)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    cw.init(0)
    st = torch.cuda.current_stream().cuda_stream
    seg = 1 << 20
    per = max(1, int(args.gib * (1 << 30)) // seg // args.streams)      # segments per stream
    n_s, n = per * seg, per * seg * args.streams
    p = cw.CdcParams.default(8192)
    cap_s, cap = p.max_offsets(n_s), p.max_offsets(n_s) * args.streams
    z = lambda count, dt=torch.int64: torch.zeros(count, dtype=dt, device="cuda")  # noqa: E731
    nseg = n // seg
    src = tiled_corpus(n)
    stamps = torch.arange(nseg * (seg // 1024), dtype=torch.int64, device="cuda").view(nseg, seg // 1024, 1)
    src.view(nseg, seg // 1024, 1024)[:, :, :8] = stamps.view(torch.uint8)
    slots_bytes = cw.chunk_slots_bytes("lz4", n_s, cap_s - 1)
    slots, sizes = torch.empty(slots_bytes, dtype=torch.uint8, device="cuda"), z(cap_s, torch.int32)
    k_dev, n_new, new_idx, result = z(1), z(1), z(cap_s, torch.int32), z(4)
    dig, ref_all = z(cap * 64, torch.uint8), z(cap)
    store, used, directory = torch.empty(n, dtype=torch.uint8, device="cuda"), z(1), z(2 * cap)
    res = {"bytes": n, "streams": args.streams, "codec": "lz4", "dir_entries": cap}
    entries_max = 1 << 20

    def ingest(index, d_src, base, d_offs, d_dig, d_ref, d_store, d_used, d_dir):
        kk = index.dev_cdc_dedupe_compress(p, "lz4", d_src, n_s, True, base, d_offs.data_ptr(), cap_s, k_dev.data_ptr(), d_dig, d_ref,
                                           new_idx.data_ptr(), n_new.data_ptr(), slots.data_ptr(), slots_bytes, sizes.data_ptr(), st)
        cw.dev_store_chunks("lz4", d_src, n_s, d_offs.data_ptr(), k_dev.data_ptr(), cap_s - 1, slots.data_ptr(), sizes.data_ptr(), base,
                            d_store.data_ptr(), n, d_used.data_ptr(), d_dir.data_ptr(), 0, cap, result.data_ptr(), st, new_idx.data_ptr(),
                            n_new.data_ptr())
        torch.cuda.synchronize()
        assert int(result[0].item()) == 0, result.tolist()
        return kk

    # ---- ingest: stream s has the values [first[s], first[s] + counts[s]) and its recipe in ref_all[first[s] ...] ----------------
    idx = cw.DedupeIndex("skein512", entries_max)
    first, counts, offsets, base = [], [], [], 0
    for s in range(args.streams):
        offs = z(cap_s)
        torch.cuda.synchronize()
        kk = ingest(idx, src.data_ptr() + s * n_s, base, offs, dig.data_ptr() + base * 64, ref_all.data_ptr() + base * 8, store, used, directory)
        first.append(base); counts.append(kk); offsets.append(offs[:kk + 1])
        base += kk
    chunks, used_bytes, entries = base, int(used.item()), idx.count()
    res.update(chunks=chunks, index_entries=entries, stored_bytes=used_bytes)

    # ---- the index as device arrays, for fresh copies ----------------------------------------------------------------------------
    x_dig, x_val, x_n = z(entries * 64, torch.uint8), z(entries), z(1)
    torch.cuda.synchronize()
    idx.dev_export(x_dig.data_ptr(), x_val.data_ptr(), entries, x_n.data_ptr(), st)
    torch.cuda.synchronize()
    assert int(x_n.item()) == entries
    scratch_ref, scratch_new, scratch_n = z(entries), z(entries, torch.int32), z(1)

    def fresh_index():
        f = cw.DedupeIndex("skein512", entries_max)
        f.dev_insert(x_dig.data_ptr(), x_val.data_ptr(), entries, scratch_ref.data_ptr(), scratch_new.data_ptr(), scratch_n.data_ptr(), st)
        torch.cuda.synchronize()
        return f

    live, n_out = z(cap, torch.int32), z(1)
    new_store, new_used, new_dir = torch.empty(used_bytes, dtype=torch.uint8, device="cuda"), z(1), z(2 * cap)
    re_dir, d_from, d_to, d_np, res4, res3, n_missing = z(2 * cap), z(cap), z(cap), z(1), z(4), z(3), z(1)
    new_refs = z(cap)
    l_dig, l_val, l_res = z(entries * 64, torch.uint8), z(entries), z(2)
    out, status = torch.empty(n_s, dtype=torch.uint8, device="cuda"), z(cap_s, torch.int32)
    v_dig, v_found, v_n = z(cap_s * 64, torch.uint8), z(cap_s), z(1)
    r_store, r_used, r_dir, r_dig, r_ref, r_offs = torch.empty(n, dtype=torch.uint8, device="cuda"), z(1), z(2 * cap), z(cap * 64, torch.uint8), z(cap), z(cap_s)

    for name, step in (("all", 1), ("second", 2), ("ninth", 9)):
        kept = list(range(0, args.streams, step))
        cat = torch.cat([ref_all[first[s]:first[s] + counts[s]] for s in kept]).contiguous()
        cat_n = z(1) + cat.numel()
        ns = [z(1) + counts[s] for s in kept]
        positions = cat.numel()

        def mark():
            live.zero_(); n_out.zero_()
            cw.dev_store_mark(cat.data_ptr(), cat_n.data_ptr(), positions, 0, cap, live.data_ptr(), n_out.data_ptr(), st)

        def compact(d_new_store=new_store.data_ptr(), room=used_bytes):
            cw.dev_store_compact(store.data_ptr(), n, directory.data_ptr(), cap, live.data_ptr(), d_new_store, room, new_used.data_ptr(),
                                 new_dir.data_ptr(), result.data_ptr(), st)

        def renumber(d_dir=directory, d_live=live.data_ptr(), dry=False):
            cw.dev_store_renumber(d_dir.data_ptr(), 0, cap, d_live, 0, 0 if dry else re_dir.data_ptr(), 0, 0 if dry else cap,
                                  0 if dry else d_from.data_ptr(), 0 if dry else d_to.data_ptr(), 0 if dry else cap, res4.data_ptr(), st)

        mark()
        torch.cuda.synchronize()
        assert int(n_out.item()) == 0
        t = alternate({"compact_dry": lambda: compact(0, 0), "renumber_dry": lambda: renumber(dry=True), "renumber": renumber}, args.reps)
        torch.cuda.synchronize()
        verdict, K, next_base, dropped = u64(res4)
        assert verdict == 0 and next_base == K, (name, verdict)
        d_np.fill_(K)
        res.update({f"{name}_kept_entries": K, f"{name}_dropped_entries": dropped, f"{name}_compact_dry_ms": t["compact_dry"],
                    f"{name}_renumber_dry_ms": t["renumber_dry"], f"{name}_renumber_ms": t["renumber"],
                    f"{name}_renumber_vs_compact_dry": t["renumber"] / t["compact_dry"],
                    f"{name}_renumber_M_entries_per_s": cap / t["renumber"] / 1e3})

        # ---- the index: export_live (read-only), then retain and revalue on fresh copies ----------------------------------------
        t = alternate({"export_live": lambda: idx.dev_export_live(live.data_ptr(), 0, cap, l_dig.data_ptr(), l_val.data_ptr(), entries,
                                                                  l_res.data_ptr(), st)}, args.reps)
        t_retain, t_revalue, t_count = [], [], []
        for rep in range(args.reps + 1):                      # (the first round is the warm-up)
            f = fresh_index()
            # before the retain the dropped entries are stale: the count sweep alone
            t_count.append(wall(lambda: f.dev_revalue(d_from.data_ptr(), d_to.data_ptr(), d_np.data_ptr(), cap, 0, cap, res3.data_ptr(), st)))
            assert u64(res3) == [1 if dropped else 0, K, dropped], (name, u64(res3))
            if dropped == 0:                                   # (it was applied: start again)
                f.close()
                f = fresh_index()
            t_retain.append(wall(lambda: f.retain(live.data_ptr(), 0, cap)))
            t_revalue.append(wall(lambda: f.dev_revalue(d_from.data_ptr(), d_to.data_ptr(), d_np.data_ptr(), cap, 0, cap, res3.data_ptr(), st)))
            assert u64(res3) == [0, K, 0] and f.count() == K, (name, u64(res3))
            f.close()
        med = lambda v: statistics.median(v[1:])  # noqa: E731
        res.update({f"{name}_export_live_ms": t["export_live"], f"{name}_retain_ms": med(t_retain), f"{name}_revalue_ms": med(t_revalue),
                    f"{name}_revalue_refused_ms": med(t_count), f"{name}_revalue_vs_retain": med(t_revalue) / med(t_retain),
                    f"{name}_revalue_vs_export_live": med(t_revalue) / t["export_live"],
                    f"{name}_revalue_M_slots_per_s": 2 * entries_max / med(t_revalue) / 1e3})

        # ---- the whole rotation, compact alone, and the rebuild ----------------------------------------------------------------
        box = {}

        def forget():
            mark()
            compact()
            torch.cuda.synchronize()                           # (the retain reads flags that have to be complete)
            box["f"].retain(live.data_ptr(), 0, cap)

        def rotation():
            forget()
            renumber(new_dir, 0)                               # the compacted directory: every non-zero entry
            for s, d_n in zip(kept, ns):
                cw.dev_translate_refs(ref_all.data_ptr() + first[s] * 8, d_n.data_ptr(), counts[s], d_from.data_ptr(), d_to.data_ptr(),
                                      d_np.data_ptr(), cap, new_refs.data_ptr() + first[s] * 8, n_missing.data_ptr(), st)
            box["f"].dev_revalue(d_from.data_ptr(), d_to.data_ptr(), d_np.data_ptr(), cap, 0, cap, res3.data_ptr(), st)

        t_forget, t_rotation = [], []
        for rep in range(args.reps + 1):
            box["f"] = fresh_index()
            t_forget.append(wall(forget))
            box["f"].close()
            box["f"] = fresh_index()
            n_missing.zero_()
            t_rotation.append(wall(rotation))
            assert u64(res4)[:2] == [0, K] and u64(res3) == [0, K, 0] and int(n_missing.item()) == 0 and int(result[0].item()) == 0, name
            if rep < args.reps:
                box["f"].close()
        # the last kept stream through its translated recipe, the compacted store, the new directory and the revalued index
        s, f = kept[-1], box["f"]
        torch.cuda.synchronize()
        cw.dev_restore_chunks("lz4", new_store.data_ptr(), used_bytes, re_dir.data_ptr(), 0, cap, new_refs.data_ptr() + first[s] * 8,
                              offsets[s].data_ptr(), ns[-1].data_ptr(), counts[s], out.data_ptr(), n_s, status.data_ptr(), st)
        cw.dev_hash_chunks("skein512", out.data_ptr(), n_s, offsets[s].data_ptr(), ns[-1].data_ptr(), counts[s], v_dig.data_ptr(), st)
        f.dev_lookup(v_dig.data_ptr(), counts[s], v_found.data_ptr(), v_n.data_ptr(), st)
        torch.cuda.synchronize()
        assert int(status[:counts[s]].abs().sum().item()) == 0 and torch.equal(out, src[s * n_s:(s + 1) * n_s]), (name, s)
        assert torch.equal(v_found[:counts[s]], new_refs[first[s]:first[s] + counts[s]]) and int(new_refs[first[s]:first[s] + counts[s]].max().item()) < K
        f.close()

        def rebuild():
            g = cw.DedupeIndex("skein512", entries_max)
            r_used.zero_()
            b = 0
            for s, d_n in zip(kept, ns):
                cw.dev_restore_chunks("lz4", store.data_ptr(), n, directory.data_ptr(), 0, cap, ref_all.data_ptr() + first[s] * 8,
                                      offsets[s].data_ptr(), d_n.data_ptr(), counts[s], out.data_ptr(), n_s, status.data_ptr(), st)
                b += ingest(g, out.data_ptr(), b, r_offs, r_dig.data_ptr() + b * 64, r_ref.data_ptr() + b * 8, r_store, r_used, r_dir)
            g.close()

        wall(rebuild)
        t_rebuild = wall(rebuild)
        res.update({f"{name}_forget_ms": med(t_forget), f"{name}_rotation_ms": med(t_rotation),
                    f"{name}_renumber_share_of_rotation": 1 - med(t_forget) / med(t_rotation), f"{name}_rebuild_ms": t_rebuild,
                    f"{name}_rebuild_vs_rotation": t_rebuild / med(t_rotation)})
    idx.close()
    print(json.dumps(res, indent=1))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
