"""Cost of the account call on one GPU.

The store of tools/store_gc_probe.py: --gib GiB of the tiled corpus ingested as --streams streams of equal length (LZ4, Skein-512)
into one store and one index.  Then, all in device events, one warm-up and the median of --reps runs each:

  a  cw_dev_store_account of all recipes: with d_refcount, d_owner and d_flag, and with none of the three.
  b  what gives the referenced total alone without it: one cw_dev_store_mark per recipe and one dry run of cw_dev_store_compact.
  c  what gives every stream's unique_stored without it: per stream, a mark of every other recipe and a dry run.  (The host would
     also read each dry run's result back; no such synchronise is in the figure.)
  d  case a over the same positions cut into 4,096 and into 65,536 streams of equal length: the binary search gets deeper and most
     wavefronts straddle a stream boundary.
  e  case a with every tenth position naming one entry: the per-entry atomics of one address.

a is checked against b and c as it goes: referenced_stored is b's dry run, referenced_stored - unique_stored[r] is c's r-th.
Prints one JSON object (and writes it to --out)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import compute_war_amd as cw  # noqa: E402
from tools.restore_probe import alternate, tiled_corpus  # noqa: E402


def u64(t):
    return [int(v) for v in t.cpu().numpy().view(np.uint64)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=4.0)
    ap.add_argument("--streams", type=int, default=36)
    ap.add_argument("--reps", type=int, default=5)
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
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.uint64).view(np.int64)).cuda()  # noqa: E731
    nseg = n // seg
    src = tiled_corpus(n)
    stamps = torch.arange(nseg * (seg // 1024), dtype=torch.int64, device="cuda").view(nseg, seg // 1024, 1)
    src.view(nseg, seg // 1024, 1024)[:, :, :8] = stamps.view(torch.uint8)
    slots_bytes = cw.chunk_slots_bytes("lz4", n_s, cap_s - 1)
    slots, sizes = torch.empty(slots_bytes, dtype=torch.uint8, device="cuda"), z(cap_s, torch.int32)
    k_dev, n_new, new_idx, result = z(1), z(1), z(cap_s, torch.int32), z(4)
    dig, ref_all, offs = z(cap * 64, torch.uint8), z(cap), z(cap_s)
    store, used, directory = torch.empty(n, dtype=torch.uint8, device="cuda"), z(1), z(2 * cap)
    res = {"bytes": n, "streams": args.streams, "codec": "lz4", "dir_entries": cap, "reps": args.reps}

    # ---- ingest: stream s has the values [first[s], first[s + 1]) and its recipe in ref_all[first[s] ...] ------------------------
    idx = cw.DedupeIndex("skein512", 1 << 20)
    first = [0]
    for s in range(args.streams):
        base, d_src = first[-1], src.data_ptr() + s * n_s
        torch.cuda.synchronize()
        kk = idx.dev_cdc_dedupe_compress(p, "lz4", d_src, n_s, True, base, offs.data_ptr(), cap_s, k_dev.data_ptr(), dig.data_ptr() + base * 64,
                                         ref_all.data_ptr() + base * 8, new_idx.data_ptr(), n_new.data_ptr(), slots.data_ptr(), slots_bytes,
                                         sizes.data_ptr(), st)
        cw.dev_store_chunks("lz4", d_src, n_s, offs.data_ptr(), k_dev.data_ptr(), cap_s - 1, slots.data_ptr(), sizes.data_ptr(), base,
                            store.data_ptr(), n, used.data_ptr(), directory.data_ptr(), 0, cap, result.data_ptr(), st, new_idx.data_ptr(),
                            n_new.data_ptr())
        torch.cuda.synchronize()
        assert int(result[0].item()) == 0, result.tolist()
        first.append(base + kk)
    positions = first[-1]
    res.update(chunks=positions, index_entries=idx.count(), stored_bytes=int(used.item()))
    idx.close()
    del src, slots, dig

    live, n_out, new_used, new_dir = z(cap, torch.int32), z(1), z(1), z(2 * cap)
    counts = [z(1) + (b - a) for a, b in zip(first[:-1], first[1:])]
    flags = (torch.arange(cap, device="cuda") % 7 == 0).to(torch.int32)
    refcount, owner, totals = z(cap, torch.int32), z(cap, torch.int32), z(8)

    def account(d_first, nstreams, acct, d_ref=ref_all, bare=False):
        cw.dev_store_account(d_ref.data_ptr(), d_first.data_ptr(), nstreams, positions, directory.data_ptr(), 0, cap,
                             0 if bare else flags.data_ptr(), acct.data_ptr(), 0 if bare else refcount.data_ptr(),
                             0 if bare else owner.data_ptr(), totals.data_ptr(), st)

    def marks(skip=None):
        live.zero_(); n_out.zero_()
        for s in range(args.streams):
            if s != skip:
                cw.dev_store_mark(ref_all.data_ptr() + first[s] * 8, counts[s].data_ptr(), first[s + 1] - first[s], 0, cap, live.data_ptr(),
                                  n_out.data_ptr(), st)

    def dry_run(skip=None):
        marks(skip)
        cw.dev_store_compact(store.data_ptr(), n, directory.data_ptr(), cap, live.data_ptr(), 0, 0, new_used.data_ptr(), new_dir.data_ptr(),
                             result.data_ptr(), st)

    def every_unique():
        for s in range(args.streams):
            dry_run(s)

    d_first, acct = dev(first), z(args.streams * 8)
    torch.cuda.synchronize()
    t = alternate({"a_account": lambda: account(d_first, args.streams, acct), "a_account_bare": lambda: account(d_first, args.streams, acct, bare=True),
                   "b_marks_and_dry_run": dry_run, "c_every_unique_by_marks": every_unique}, args.reps)
    res.update({f"{k}_ms": v for k, v in t.items()})
    res.update(a_vs_b=t["a_account"] / t["b_marks_and_dry_run"], c_vs_a=t["c_every_unique_by_marks"] / t["a_account"],
               a_M_positions_per_s=positions / t["a_account"] / 1e3)

    # ---- a against b and c ---------------------------------------------------------------------------------------------------------
    account(d_first, args.streams, acct)
    torch.cuda.synchronize()
    tot, streams = u64(totals), acct.cpu().numpy().view(cw.ACCOUNT_DTYPE)
    dry_run()
    torch.cuda.synchronize()
    assert tot[0] == 0 and tot[7] == 0 and u64(result)[1:3] == [tot[4], tot[3]], (tot, u64(result))
    for s in (0, args.streams // 2, args.streams - 1):
        dry_run(s)
        torch.cuda.synchronize()
        assert u64(result)[1] == tot[4] - int(streams[s]["unique_stored"]), s
    res.update(referenced_entries=tot[3], referenced_stored=tot[4], shared_entries=tot[5],
               unique_stored_min=int(streams["unique_stored"].min()), unique_stored_max=int(streams["unique_stored"].max()))

    # ---- d: the same positions as many short streams ---------------------------------------------------------------------------------
    for many in (4096, 65536):
        f = dev(np.linspace(0, positions, many + 1).astype(np.uint64))
        a = z(many * 8)
        torch.cuda.synchronize()
        tm = alternate({"x": lambda: account(f, many, a)}, args.reps)["x"]
        torch.cuda.synchronize()
        assert u64(totals)[:5] == tot[:5] and int(a.cpu().numpy().view(cw.ACCOUNT_DTYPE)["positions"].sum()) == positions
        res.update({f"d_account_{many}_streams_ms": tm, f"d_{many}_streams_vs_a": tm / t["a_account"]})

    # ---- e: every tenth position names entry 0 -----------------------------------------------------------------------------------------
    hot = ref_all.clone()
    hot[0:positions:10] = 0
    torch.cuda.synchronize()
    te = alternate({"x": lambda: account(d_first, args.streams, acct, d_ref=hot)}, args.reps)["x"]
    torch.cuda.synchronize()
    assert int(refcount[0].item()) == (positions + 9) // 10 and int(owner[0].item()) & 0xFFFFFFFF == cw.Account.SHARED
    res.update(e_account_hot_entry_ms=te, e_hot_vs_a=te / t["a_account"], e_hot_positions=(positions + 9) // 10)

    print(json.dumps(res, indent=1))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
