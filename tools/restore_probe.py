"""Rates of the chunk store on one GPU.

--gib GiB of the tiled corpus built as tools/chunk_codec_probe.py builds the fused call's input (1 MiB segments, a stamp every
1 KiB, duplicate segments drawn from the unique ones) at duplicate shares 0, 0.5 and 0.9, each through cw_dev_cdc_dedupe_compress
into a fresh index, for both codecs.  Then, with the configurations alternating:

  append    cw_dev_store_chunks of the call's new chunks into an empty store, against cw_dev_pack_chunks over the same selection
            (which drops what the store keeps raw: both byte counts are reported);
  restore   cw_dev_restore_chunks of the whole stream from its recipe, per GB of OUTPUT, against cw_dev_decompress_chunks over the
            packed stream of the new chunks, per GB of its output.

Device events, one warm-up, median of --reps runs.  Prints one JSON object (and writes it to --out)."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import compute_war_amd as cw  # noqa: E402


def timed(fn):
    s = torch.cuda.current_stream()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(s)
    fn()
    b.record(s)
    b.synchronize()
    return a.elapsed_time(b)


def alternate(configs, reps):
    """median ms of every configuration: one warm-up each, then reps rounds over all of them"""
    times = {name: [] for name in configs}
    for fn in configs.values():
        timed(fn)
    for _ in range(reps):
        for name, fn in configs.items():
            times[name].append(timed(fn))
    return {name: statistics.median(t) for name, t in times.items()}


def tiled_corpus(n):
    root = os.path.join(ROOT, "tests", "golden", "corpus", "canterbury")
    data = b"".join(open(os.path.join(root, f), "rb").read() for f in sorted(os.listdir(root)))
    one = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    return one.repeat(n // one.numel() + 1)[:n].contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=4.0)
    ap.add_argument("--reps", type=int, default=3)
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
    packed, poff, raw = torch.empty(n + (n >> 7) + 64 * cap, dtype=torch.uint8, device="cuda"), z(cap, torch.int64), z(cap, torch.int64)
    out, status = torch.empty(n, dtype=torch.uint8, device="cuda"), z(cap, torch.int32)
    src = torch.empty(n, dtype=torch.uint8, device="cuda")
    seg = 1 << 20
    nseg = n // seg
    uniq = tiled_corpus(n).view(nseg, seg)
    stamps = torch.arange(nseg * (seg // 1024), dtype=torch.int64, device="cuda").view(nseg, seg // 1024, 1)
    uniq.view(nseg, seg // 1024, 1024)[:, :, :8] = stamps.view(torch.uint8)
    res = {"bytes": n}

    for d in (0.0, 0.5, 0.9):
        g = torch.Generator(device="cuda").manual_seed(7)
        n_u = max(1, int(round(nseg * (1 - d))))
        pick = torch.cat([torch.arange(n_u, device="cuda"), torch.randint(0, n_u, (nseg - n_u,), device="cuda", generator=g)])
        pick = pick[torch.randperm(nseg, device="cuda", generator=g)]
        src.view(nseg, seg).copy_(uniq[pick])
        for alg in ("lz4", "lzf"):
            tag = f"{alg}_dup{int(d * 100)}"
            idx = cw.DedupeIndex("skein512", 1 << 20)
            torch.cuda.synchronize()
            kk = idx.dev_cdc_dedupe_compress(p, alg, src.data_ptr(), n, True, 0, offs.data_ptr(), cap, k.data_ptr(), dig.data_ptr(),
                                             ref.data_ptr(), new_idx.data_ptr(), n_new.data_ptr(), slots.data_ptr(), slots_bytes, sizes.data_ptr(), st)
            torch.cuda.synchronize()
            m = int(n_new.item())
            res[f"{tag}_chunks"], res[f"{tag}_new_chunk_share"] = kk, m / max(kk, 1)

            def append():
                cw.dev_store_chunks(alg, src.data_ptr(), n, offs.data_ptr(), k.data_ptr(), cap - 1, slots.data_ptr(), sizes.data_ptr(), 0,
                                    store.data_ptr(), n, used.data_ptr(), directory.data_ptr(), 0, cap, result.data_ptr(), st, new_idx.data_ptr(),
                                    n_new.data_ptr())

            def append_fresh():  # (the 8-byte memset is inside the timing: each run appends to an empty store)
                used.zero_()
                append()

            def pack():
                cw.dev_pack_chunks(alg, slots.data_ptr(), offs.data_ptr(), n_new.data_ptr(), cap - 1, sizes.data_ptr(), packed.data_ptr(),
                                   poff.data_ptr(), st, new_idx.data_ptr())

            t = alternate({"store": append_fresh, "pack": pack}, args.reps)
            torch.cuda.synchronize()
            verdict, stored_bytes = (int(v) for v in result.cpu().numpy().view("uint64"))
            assert verdict == 0, (tag, verdict, stored_bytes)
            packed_bytes = int(poff[m].item())
            lens = offs[1:kk + 1] - offs[:kk]
            new_lens = lens[new_idx[:m].to(torch.int64)]
            raw[1:m + 1] = torch.cumsum(new_lens, 0)
            new_raw_bytes = int(raw[m].item())
            kept_raw = int(((sizes[:m] == 0) | (sizes[:m].to(torch.int64) >= new_lens)).sum().item())
            res[f"{tag}_store_ms"], res[f"{tag}_pack_ms"] = t["store"], t["pack"]
            res[f"{tag}_stored_bytes"], res[f"{tag}_packed_bytes"], res[f"{tag}_chunks_kept_raw"] = stored_bytes, packed_bytes, kept_raw
            res[f"{tag}_store_GBps_of_stored"], res[f"{tag}_pack_GBps_of_packed"] = stored_bytes / t["store"] / 1e6, packed_bytes / t["pack"] / 1e6
            res[f"{tag}_store_vs_pack_per_byte"] = (stored_bytes / t["store"]) / (packed_bytes / t["pack"])

            def restore():
                cw.dev_restore_chunks(alg, store.data_ptr(), n, directory.data_ptr(), 0, cap, ref.data_ptr(), offs.data_ptr(), k.data_ptr(),
                                      cap - 1, out.data_ptr(), n, status.data_ptr(), st)

            def decoder():
                cw.dev_decompress_chunks(alg, packed.data_ptr(), poff.data_ptr(), raw.data_ptr(), n_new.data_ptr(), cap - 1, out.data_ptr(),
                                         new_raw_bytes, status.data_ptr(), st)

            t = alternate({"restore": restore, "decoder": decoder}, args.reps)
            restore()
            torch.cuda.synchronize()
            assert int(status[:kk].abs().sum().item()) == 0 and torch.equal(out, src), tag
            res[f"{tag}_restore_ms"], res[f"{tag}_decoder_ms"] = t["restore"], t["decoder"]
            res[f"{tag}_restore_GBps_of_output"], res[f"{tag}_decoder_GBps_of_output"] = n / t["restore"] / 1e6, new_raw_bytes / t["decoder"] / 1e6
            res[f"{tag}_restore_vs_decoder"] = (n / t["restore"]) / (new_raw_bytes / t["decoder"])
            idx.close()
    print(json.dumps(res, indent=1))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
