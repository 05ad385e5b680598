"""Rates of ranged reads from the chunk store on one GPU.

--gib GiB of the tiled corpus of tools/restore_probe.py (1 MiB segments, a stamp every 1 KiB, duplicate segments drawn from the
unique ones, duplicate share --dup) through cw_dev_cdc_dedupe_compress into a fresh index and cw_dev_store_chunks into an empty
store, for both codecs.  Then cw_dev_read_ranges against cw_dev_restore_chunks of the whole stream, the two alternating:

  whole     one range over the whole stream;
  4K / 64K  1 Ki, 64 Ki and 1 Mi uniformly random ranges of 4 KiB and of 64 KiB in one call, destinations back to back: time, GB/s
            of bytes returned, and the time as a share of the whole restore's.

Device events, one warm-up, median of --reps runs.  Every call's statuses are checked to be 0, the whole read against the input,
the random reads' first ranges against the input's slices.  Prints one JSON object (and writes it to --out)."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import compute_war_amd as cw  # noqa: E402
from restore_probe import alternate, tiled_corpus  # noqa: E402  (tools/ is the script's directory)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=4.0)
    ap.add_argument("--dup", type=float, default=0.5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--counts", type=int, nargs="*", default=[1 << 10, 1 << 16, 1 << 20])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    cw.init(0)
    st = torch.cuda.current_stream().cuda_stream
    n = int(args.gib * (1 << 30)) // (1 << 20) * (1 << 20)
    p = cw.CdcParams.default(8192)
    cap = p.max_offsets(n)
    z = lambda count, dt: torch.zeros(count, dtype=dt, device="cuda")  # noqa: E731
    offs, k, sizes = z(cap, torch.int64), z(1, torch.int64), z(cap, torch.int32)
    dig, ref, new_idx, n_new = z(cap * 64, torch.uint8), z(cap, torch.int64), z(cap, torch.int32), z(1, torch.int64)
    slots_bytes = max(cw.chunk_slots_bytes(a, n, cap - 1) for a in ("lz4", "lzf"))
    slots = torch.empty(slots_bytes, dtype=torch.uint8, device="cuda")
    store, used, directory, result = torch.empty(n, dtype=torch.uint8, device="cuda"), z(1, torch.int64), z(2 * cap, torch.int64), z(2, torch.int64)
    out, status = torch.empty(n, dtype=torch.uint8, device="cuda"), z(cap, torch.int32)
    src = torch.empty(n, dtype=torch.uint8, device="cuda")
    seg = 1 << 20
    nseg = n // seg
    uniq = tiled_corpus(n).view(nseg, seg)
    stamps = torch.arange(nseg * (seg // 1024), dtype=torch.int64, device="cuda").view(nseg, seg // 1024, 1)
    uniq.view(nseg, seg // 1024, 1024)[:, :, :8] = stamps.view(torch.uint8)
    g = torch.Generator(device="cuda").manual_seed(7)
    n_u = max(1, int(round(nseg * (1 - args.dup))))
    pick = torch.cat([torch.arange(n_u, device="cuda"), torch.randint(0, n_u, (nseg - n_u,), device="cuda", generator=g)])
    src.view(nseg, seg).copy_(uniq[pick[torch.randperm(nseg, device="cuda", generator=g)]])
    del uniq
    res = {"bytes": n, "dup": args.dup, "reps": args.reps}

    for alg in ("lz4", "lzf"):
        idx = cw.DedupeIndex("skein512", 1 << 20)
        used.zero_()
        directory.zero_()
        torch.cuda.synchronize()
        kk = idx.dev_cdc_dedupe_compress(p, alg, src.data_ptr(), n, True, 0, offs.data_ptr(), cap, k.data_ptr(), dig.data_ptr(), ref.data_ptr(),
                                         new_idx.data_ptr(), n_new.data_ptr(), slots.data_ptr(), slots_bytes, sizes.data_ptr(), st)
        cw.dev_store_chunks(alg, src.data_ptr(), n, offs.data_ptr(), k.data_ptr(), cap - 1, slots.data_ptr(), sizes.data_ptr(), 0,
                            store.data_ptr(), n, used.data_ptr(), directory.data_ptr(), 0, cap, result.data_ptr(), st, new_idx.data_ptr(),
                            n_new.data_ptr())
        torch.cuda.synchronize()
        assert int(result[0].item()) == 0, (alg, result)
        res[f"{alg}_chunks"], res[f"{alg}_stored_bytes"] = kk, int(used.item())

        def restore():
            cw.dev_restore_chunks(alg, store.data_ptr(), n, directory.data_ptr(), 0, cap, ref.data_ptr(), offs.data_ptr(), k.data_ptr(), cap - 1,
                                  out.data_ptr(), n, status.data_ptr(), st)

        def read_into(dst, dst_bytes, r_off, r_len, r_dst, r_n, r_status):
            m = r_off.numel()
            return lambda: cw.dev_read_ranges(alg, store.data_ptr(), n, directory.data_ptr(), 0, cap, ref.data_ptr(), offs.data_ptr(), k.data_ptr(),
                                              cap - 1, r_off.data_ptr(), r_len.data_ptr(), r_dst.data_ptr(), r_n.data_ptr(), m, dst.data_ptr(),
                                              dst_bytes, r_status.data_ptr(), st)

        # (a) one range over the whole stream
        one = [torch.tensor([v], dtype=torch.int64, device="cuda") for v in (0, n, 0, 1)]
        r_status = torch.full((1,), -1, dtype=torch.int32, device="cuda")
        whole = read_into(out, n, *one, r_status)
        t = alternate({"restore": restore, "read": whole}, args.reps)
        out.zero_()
        whole()
        torch.cuda.synchronize()
        assert int(r_status.item()) == 0 and torch.equal(out, src), alg
        res[f"{alg}_whole_restore_ms"], res[f"{alg}_whole_read_ms"] = t["restore"], t["read"]
        res[f"{alg}_whole_restore_GBps"], res[f"{alg}_whole_read_GBps"] = n / t["restore"] / 1e6, n / t["read"] / 1e6
        res[f"{alg}_whole_read_vs_restore"] = t["restore"] / t["read"]

        # (b), (c) random ranges, destinations back to back
        for length, name in ((4096, "4K"), (65536, "64K")):
            for m in args.counts:
                tag = f"{alg}_{name}_x{m}"
                r_off = torch.randint(0, n - length, (m,), dtype=torch.int64, device="cuda", generator=g)
                r_len = torch.full((m,), length, dtype=torch.int64, device="cuda")
                r_dst = torch.arange(m, dtype=torch.int64, device="cuda") * length
                r_n = torch.tensor([m], dtype=torch.int64, device="cuda")
                r_status = torch.full((m,), -1, dtype=torch.int32, device="cuda")
                dst = torch.empty(m * length, dtype=torch.uint8, device="cuda") if m * length > n else out
                read = read_into(dst, m * length, r_off, r_len, r_dst, r_n, r_status)
                t = alternate({"restore": restore, "read": read}, args.reps)
                torch.cuda.synchronize()
                assert int(r_status.abs().sum().item()) == 0, tag
                for i in range(min(m, 64)):
                    a = int(r_off[i].item())
                    assert torch.equal(dst[i * length:(i + 1) * length], src[a:a + length]), (tag, i)
                res[f"{tag}_read_ms"], res[f"{tag}_restore_ms"] = t["read"], t["restore"]
                res[f"{tag}_GBps_returned"] = m * length / t["read"] / 1e6
                res[f"{tag}_share_of_stream"], res[f"{tag}_share_of_restore_time"] = m * length / n, t["read"] / t["restore"]
                del dst, read
        idx.close()
    print(json.dumps(res, indent=1))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
