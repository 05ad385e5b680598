"""Rates of the codecs over content-defined chunks on one GPU.

1. cw_dev_compress_chunks (LZ4, LZF) over the device's own cuts (8 KiB defaults) of --gib GiB of the tiled corpus, of
   cw_dev_gen_random data and of the 50 % mix, against cw_dev_compress over the same bytes as fixed 8 KiB blocks.
2. cw_dev_decompress_chunks over the packed chunks of the corpus against cw_dev_decompress over the fixed path's slots of the
   same data at 8 KiB blocks.
3. cw_dev_cdc_dedupe_compress at duplicate shares of about 0, 0.5 and 0.9 (1 MiB segments of the stamped corpus, the duplicates
   drawn from the unique ones as tools/dedupe_probe.py draws blocks) against the five separate calls and against chunk + hash +
   dedupe alone, each run into a fresh index.
Device events, one warm-up, median of --reps runs with the configurations alternating.  Prints one JSON object (and writes it to --out)."""
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
    offs = torch.zeros(cap, dtype=torch.int64, device="cuda")
    k = torch.zeros(1, dtype=torch.int64, device="cuda")
    sizes = torch.zeros(cap, dtype=torch.int32, device="cuda")
    bs, nb = 8192, n // 8192
    stride = (cw.compress_bound("lz4", bs) + 15) // 16 * 16
    fixed = torch.empty(nb * stride, dtype=torch.uint8, device="cuda")
    fsizes = torch.zeros(nb, dtype=torch.int32, device="cuda")
    slots_bytes = cw.chunk_slots_bytes("lz4", n, cap - 1)
    slots = torch.empty(slots_bytes, dtype=torch.uint8, device="cuda")
    res = {"bytes": n, "slot_bytes_lz4": slots_bytes, "slot_bytes_lzf": cw.chunk_slots_bytes("lzf", n, cap - 1)}

    src = torch.empty(n, dtype=torch.uint8, device="cuda")
    for data in ("corpus", "random", "mixed"):
        if data == "corpus":
            src.copy_(tiled_corpus(n))
        elif data == "random":
            cw.dev_gen_random(0xC0C0, 0, n // 65536, 65536, src.data_ptr(), st)
        else:
            cw.dev_gen_mixed(0xC0C0, 0, n // 8192, 8192, src.data_ptr(), st)
        cw.dev_cdc(p, src.data_ptr(), n, True, offs.data_ptr(), cap, k.data_ptr(), st)
        torch.cuda.synchronize()
        res[f"{data}_chunks"] = int(k.item())
        for alg in ("lz4", "lzf"):
            t = alternate({
                "chunks": lambda: cw.dev_compress_chunks(alg, src.data_ptr(), n, offs.data_ptr(), k.data_ptr(), cap - 1, slots.data_ptr(),
                                                         slots_bytes, sizes.data_ptr(), st),
                "fixed": lambda: cw.dev_compress(alg, src.data_ptr(), bs, nb, fixed.data_ptr(), stride, fsizes.data_ptr(), st)}, args.reps)
            res[f"{data}_{alg}_chunks_ms"], res[f"{data}_{alg}_fixed8k_ms"] = t["chunks"], t["fixed"]
            res[f"{data}_{alg}_chunks_GBps"], res[f"{data}_{alg}_fixed8k_GBps"] = n / t["chunks"] / 1e6, n / t["fixed"] / 1e6
            res[f"{data}_{alg}_chunks_vs_fixed8k"] = t["fixed"] / t["chunks"]
            res[f"{data}_{alg}_chunks_compressed_bytes"] = int(sizes[:int(k.item())].to(torch.int64).sum().item())
            res[f"{data}_{alg}_fixed8k_compressed_bytes"] = int(fsizes.to(torch.int64).sum().item())
            if data != "corpus":
                continue
            # decode: the packed chunks against the fixed path's slots
            poff = torch.zeros(cap, dtype=torch.int64, device="cuda")
            packed = torch.empty(n, dtype=torch.uint8, device="cuda")
            out = torch.empty(n, dtype=torch.uint8, device="cuda")
            status = torch.zeros(cap if cap > nb else nb, dtype=torch.int32, device="cuda")
            t_pack = timed(lambda: cw.dev_pack_chunks(alg, slots.data_ptr(), offs.data_ptr(), k.data_ptr(), cap - 1, sizes.data_ptr(),
                                                      packed.data_ptr(), poff.data_ptr(), st))
            t_pack = timed(lambda: cw.dev_pack_chunks(alg, slots.data_ptr(), offs.data_ptr(), k.data_ptr(), cap - 1, sizes.data_ptr(),
                                                      packed.data_ptr(), poff.data_ptr(), st))
            t = alternate({
                "chunks": lambda: cw.dev_decompress_chunks(alg, packed.data_ptr(), poff.data_ptr(), offs.data_ptr(), k.data_ptr(), cap - 1,
                                                           out.data_ptr(), n, status.data_ptr(), st),
                "fixed": lambda: cw.dev_decompress(alg, fixed.data_ptr(), stride, fsizes.data_ptr(), nb, out.data_ptr(), bs,
                                                   status.data_ptr(), st)}, args.reps)
            res[f"corpus_{alg}_pack_chunks_ms"] = t_pack
            res[f"corpus_{alg}_decompress_chunks_ms"], res[f"corpus_{alg}_decompress_fixed8k_ms"] = t["chunks"], t["fixed"]
            res[f"corpus_{alg}_decompress_chunks_GBps"] = n / t["chunks"] / 1e6
            res[f"corpus_{alg}_decompress_fixed8k_GBps"] = n / t["fixed"] / 1e6
            del poff, packed, out, status
            torch.cuda.empty_cache()

    # ---- the fused call at three duplicate shares ----
    del fixed, fsizes
    torch.cuda.empty_cache()
    seg = 1 << 20
    nseg = n // seg
    uniq = tiled_corpus(n).view(nseg, seg)
    db = 64
    dig = torch.zeros(cap * db, dtype=torch.uint8, device="cuda")
    ref = torch.zeros(cap, dtype=torch.int64, device="cuda")
    new_idx = torch.zeros(cap, dtype=torch.int32, device="cuda")
    n_new = torch.zeros(1, dtype=torch.int64, device="cuda")
    for d in (0.0, 0.5, 0.9):
        ms = {"fused": [], "five_calls": [], "cdc_hash_dedupe": []}
        new_share = 0.0
        for rep in range(args.reps + 1):  # rep 0 warms up
            for which in ms:
                # every run gets data of its own (a stamp every 1 KiB makes each chunk of the unique segments new) and a fresh index
                serial = (rep * 3 + list(ms).index(which)) * (n // 1024)
                stamps = (torch.arange(nseg * (seg // 1024), dtype=torch.int64, device="cuda") + serial).view(nseg, seg // 1024, 1)
                uniq.view(nseg, seg // 1024, 1024)[:, :, :8] = stamps.view(torch.uint8)
                g = torch.Generator(device="cuda").manual_seed(7 + rep)
                n_u = max(1, int(round(nseg * (1 - d))))
                pick = torch.cat([torch.arange(n_u, device="cuda"), torch.randint(0, n_u, (nseg - n_u,), device="cuda", generator=g)])
                pick = pick[torch.randperm(nseg, device="cuda", generator=g)]
                src.view(nseg, seg).copy_(uniq[pick])
                idx = cw.DedupeIndex("skein512", 1 << 20)
                torch.cuda.synchronize()

                def fused():
                    idx.dev_cdc_dedupe_compress(p, "lz4", src.data_ptr(), n, True, 0, offs.data_ptr(), cap, k.data_ptr(), dig.data_ptr(),
                                                ref.data_ptr(), new_idx.data_ptr(), n_new.data_ptr(), slots.data_ptr(), slots_bytes,
                                                sizes.data_ptr(), st)

                def three(compress):
                    cw.dev_cdc(p, src.data_ptr(), n, True, offs.data_ptr(), cap, k.data_ptr(), st)
                    cw.dev_hash_chunks("skein512", src.data_ptr(), n, offs.data_ptr(), k.data_ptr(), cap - 1, dig.data_ptr(), st)
                    torch.cuda.current_stream().synchronize()
                    idx.dev_dedupe(dig.data_ptr(), int(k.item()), 0, ref.data_ptr(), new_idx.data_ptr(), n_new.data_ptr(), st)
                    if compress:
                        cw.dev_compress_chunks("lz4", src.data_ptr(), n, offs.data_ptr(), k.data_ptr(), cap - 1, slots.data_ptr(), slots_bytes,
                                               sizes.data_ptr(), st, new_idx.data_ptr(), n_new.data_ptr())

                t = timed(fused if which == "fused" else (lambda: three(which == "five_calls")))
                if rep:
                    ms[which].append(t)
                new_share = int(n_new.item()) / max(int(k.item()), 1)
                idx.close()
        tag = f"dup{int(d * 100)}"
        res[f"fused_{tag}_new_chunk_share"] = new_share
        for which, t in ms.items():
            res[f"{which}_{tag}_ms"] = statistics.median(t)
            res[f"{which}_{tag}_GBps"] = n / statistics.median(t) / 1e6
    print(json.dumps(res, indent=1))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
