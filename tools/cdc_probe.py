"""Rates of content-defined chunking and per-chunk hashing on one GPU.

cw_dev_cdc over 4 GiB of cw_dev_gen_random data at the 8 KiB defaults, then 4 GiB of zeros, of a 2-byte pattern (both from
offset 0 and behind a random prefix of odd length) and of the random data with masks of 0; cw_dev_hash_chunks over the random data's chunks against cw_dev_hash over the same bytes as
8 KiB blocks, for each algorithm; chunk + hash + dedupe end to end, into a fresh index each run.  Device events, one warm-up, median of 3 runs with the
configurations alternating.  Prints one JSON object (and writes it to --out)."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import compute_war_amd as cw  # noqa: E402


def timed(fn):
    s = torch.cuda.current_stream()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(s)
    fn()
    b.record(s)
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=4.0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    cw.init(0)
    st = torch.cuda.current_stream().cuda_stream
    n = int(args.gib * (1 << 30)) // 65536 * 65536
    rnd = torch.empty(n, dtype=torch.uint8, device="cuda")
    cw.dev_gen_random(0xC0C0, 0, n // 65536, 65536, rnd.data_ptr(), st)
    zeros = torch.zeros(n, dtype=torch.uint8, device="cuda")
    pat = torch.tensor([0x61, 0x62], dtype=torch.uint8, device="cuda").repeat(n // 2)
    # the same runs behind a random prefix of odd length: the chain enters them at an odd phase
    zeros_odd, pat_odd = zeros.clone(), pat.clone()
    zeros_odd[:12345] = rnd[:12345]
    pat_odd[:12345] = rnd[:12345]
    p = cw.CdcParams.default(8192)
    p0 = cw.CdcParams.default(8192)
    p0.mask_s = p0.mask_l = 0
    cap = p.max_offsets(n)
    offs = torch.zeros(cap, dtype=torch.int64, device="cuda")
    k = torch.zeros(1, dtype=torch.int64, device="cuda")

    def cdc(src, prm):
        return lambda: cw.dev_cdc(prm, src.data_ptr(), n, True, offs.data_ptr(), cap, k.data_ptr(), st)

    configs = {"random": cdc(rnd, p), "zeros": cdc(zeros, p), "pattern_ab": cdc(pat, p), "random_masks0": cdc(rnd, p0),
               "zeros_after_odd_prefix": cdc(zeros_odd, p), "pattern_ab_after_odd_prefix": cdc(pat_odd, p)}
    times = {name: [] for name in configs}
    for fn in configs.values():
        timed(fn)
    for _ in range(args.reps):
        for name, fn in configs.items():
            times[name].append(timed(fn))
            if name == "random":
                chunks = int(k.item())
    res = {"bytes": n, "chunks_random": chunks}
    for name, t in times.items():
        res[f"cdc_{name}_ms"] = statistics.median(t)
        res[f"cdc_{name}_GBps"] = n / statistics.median(t) / 1e6
    timed(configs["random"])  # the random data's chunks for the hashing runs
    chunks = int(k.item())
    dig = torch.zeros(cap * 64, dtype=torch.uint8, device="cuda")
    for alg in ("skein512", "skein", "sha256mb"):
        fns = {"chunks": lambda: cw.dev_hash_chunks(alg, rnd.data_ptr(), n, offs.data_ptr(), k.data_ptr(), cap, dig.data_ptr(), st),
               "blocks": lambda: cw.dev_hash(alg, rnd.data_ptr(), 8192, n // 8192, dig.data_ptr(), st)}
        t = {x: [] for x in fns}
        for fn in fns.values():
            timed(fn)
        for _ in range(args.reps):
            for x, fn in fns.items():
                t[x].append(timed(fn))
        res[f"hash_chunks_{alg}_ms"] = statistics.median(t["chunks"])
        res[f"hash_blocks8k_{alg}_ms"] = statistics.median(t["blocks"])
        res[f"hash_chunks_vs_blocks_{alg}"] = statistics.median(t["blocks"]) / statistics.median(t["chunks"])
    # chunk + hash + dedupe, end to end (one synchronise, at the end), each run into a fresh index: every chunk is an insert
    ref = torch.zeros(cap, dtype=torch.int64, device="cuda")
    new_idx = torch.zeros(cap, dtype=torch.int32, device="cuda")
    n_new = torch.zeros(1, dtype=torch.int64, device="cuda")

    def e2e(idx):
        cw.dev_cdc(p, rnd.data_ptr(), n, True, offs.data_ptr(), cap, k.data_ptr(), st)
        cw.dev_hash_chunks("skein512", rnd.data_ptr(), n, offs.data_ptr(), k.data_ptr(), cap, dig.data_ptr(), st)
        idx.dev_dedupe(dig.data_ptr(), chunks, 0, ref.data_ptr(), new_idx.data_ptr(), n_new.data_ptr(), st)

    t = []
    for _ in range(args.reps + 1):
        idx = cw.DedupeIndex("skein512", 1 << 21)
        t.append(timed(lambda: e2e(idx)))
        assert int(n_new.item()) == chunks  # random data: every chunk is new
        del idx
    t = t[1:]
    res["cdc_hash_dedupe_skein512_inserts_ms"] = statistics.median(t)
    res["cdc_hash_dedupe_skein512_inserts_GBps"] = n / statistics.median(t) / 1e6
    print(json.dumps(res, indent=1))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
