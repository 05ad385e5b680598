"""Rates of the streamed chunk store on one GPU.

--gib GiB of the tiled corpus (built as tools/restore_probe.py builds it: 1 MiB segments, a stamp every 1 KiB, so every chunk is
new) in page-locked host memory, cw_cdc_default_params(8192), both codecs, each run into a fresh index and an empty store.  Wall
time, one warm-up, median of --reps runs with the configurations alternating.  Per codec:

  a  cw_store_ingest
  b  the same pieces without overlap, with the calls the library had before: a blocking upload, then cw_dev_cdc_dedupe_compress +
     cw_dev_store_chunks + a synchronise per piece (the carry moved to the front of the buffer on the device)
  c  the uploads alone: one blocking copy per piece
  d  cw_store_restore into page-locked memory
  d_1gib  the same with CW_STORE_PIECE = 1 GiB, four windows instead of sixteen (reported beside d; the claim is about d)
  e  cw_dev_restore_chunks of the whole stream + one blocking download

The claim to check is a < b and d < e by more than the spread of the runs; efficiency = a / max(b - c, c): 1.0 would be an ingest
that costs only the longer of its kernels and its uploads.  Prints one JSON object and writes it to --out."""
import argparse
import ctypes as C
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


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def alternate(configs, reps):
    """{name: [ms of every run]}: one warm-up each, then reps rounds over all of them"""
    times = {name: [] for name in configs}
    for fn in configs.values():
        wall(fn)
    for _ in range(reps):
        for name, fn in configs.items():
            times[name].append(wall(fn))
    return times


def pinned(n):
    p = cw.lib().cw_host_alloc(n)
    assert p, "cw_host_alloc failed"
    return p, torch.from_numpy(np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(n,)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=4.0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15_ingest_probe.json"))
    args = ap.parse_args()
    cw.init(0)
    L = cw.lib()
    st = torch.cuda.current_stream().cuda_stream
    n = int(args.gib * (1 << 30)) // (1 << 20) * (1 << 20)
    piece = 256 << 20
    p = cw.CdcParams.default(8192)
    cap, pcap = p.max_offsets(n), p.max_offsets(piece + p.max_size)
    z = lambda count, dt: torch.zeros(count, dtype=dt, device="cuda")  # noqa: E731

    # the input, page-locked
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

    store, used, directory = torch.empty(n, dtype=torch.uint8, device="cuda"), z(1, torch.int64), z(2 * cap, torch.int64)
    triple = cw.Store(store.data_ptr(), n, used.data_ptr(), directory.data_ptr(), 0, cap)
    # b's buffers: one piece, as cw_cdc_hash lays it out
    buf = torch.empty(piece + p.max_size + 16, dtype=torch.uint8, device="cuda")
    offs, k_dev, sizes, result = z(pcap, torch.int64), z(1, torch.int64), z(pcap, torch.int32), z(2, torch.int64)
    dig, ref, new_idx, n_new = z(pcap * 64, torch.uint8), z(pcap, torch.int64), z(pcap, torch.int32), z(1, torch.int64)
    slots_bytes = max(cw.chunk_slots_bytes(a, piece + p.max_size, pcap - 1) for a in ("lz4", "lzf"))
    slots = torch.empty(slots_bytes, dtype=torch.uint8, device="cuda")
    # e's buffers: the whole stream
    out, status, d_ref, d_off, d_k = torch.empty(n, dtype=torch.uint8, device="cuda"), z(cap, torch.int32), z(cap, torch.int64), z(cap, torch.int64), z(1, torch.int64)
    res = {"bytes": n, "piece": piece, "reps": args.reps}

    for alg in ("lz4", "lzf"):
        state = {}

        def fresh():
            if state.get("idx"):
                state["idx"].close()
            state["idx"] = cw.DedupeIndex("skein512", 1 << 22)
            used.zero_()
            directory.zero_()
            torch.cuda.synchronize()

        def ingest():
            fresh()
            t = time.perf_counter()
            rc, refs, cuts, consumed, stats = cw.store_ingest(state["idx"], p, alg, triple, h_src, n, 0)
            state["a_ms"] = (time.perf_counter() - t) * 1e3
            assert rc == 0 and consumed == n, (rc, consumed)
            state["recipe"], state["stats"] = (refs, cuts), stats

        def pieces_without_overlap():
            fresh()
            t = time.perf_counter()
            done = carry = chunks = 0
            npieces = (n + piece - 1) // piece
            for i in range(npieces):
                take = min(piece, n - i * piece)
                assert L.cw_dev_upload(buf.data_ptr() + carry, h_src + i * piece, take) == 0
                length = carry + take
                k = state["idx"].dev_cdc_dedupe_compress(p, alg, buf.data_ptr(), length, i + 1 == npieces, chunks, offs.data_ptr(), pcap,
                                                         k_dev.data_ptr(), dig.data_ptr(), ref.data_ptr(), new_idx.data_ptr(), n_new.data_ptr(),
                                                         slots.data_ptr(), slots_bytes, sizes.data_ptr(), st)
                cw.dev_store_chunks(alg, buf.data_ptr(), length, offs.data_ptr(), k_dev.data_ptr(), pcap - 1, slots.data_ptr(), sizes.data_ptr(),
                                    chunks, store.data_ptr(), n, used.data_ptr(), directory.data_ptr(), 0, cap, result.data_ptr(), st,
                                    new_idx.data_ptr(), n_new.data_ptr())
                torch.cuda.synchronize()
                consumed = int(offs[k].item())
                assert int(result[0].item()) == 0
                carry = length - consumed
                if carry and i + 1 < npieces:
                    buf[:carry] = buf[consumed:length].clone()
                chunks += k
                done += consumed
            torch.cuda.synchronize()
            state["b_ms"] = (time.perf_counter() - t) * 1e3
            assert done == n and chunks == len(state["recipe"][0]), (done, chunks)

        def uploads():
            for i in range((n + piece - 1) // piece):
                assert L.cw_dev_upload(buf.data_ptr(), h_src + i * piece, min(piece, n - i * piece)) == 0

        # a and b time themselves: making the fresh index and emptying the store is not part of either
        def timed_inner(fn, key):
            def run():
                fn()
                state.setdefault(key + "_runs", []).append(state[key])
            return run

        alternate({"a": timed_inner(ingest, "a_ms"), "b": timed_inner(pieces_without_overlap, "b_ms")}, args.reps)
        c_runs = alternate({"c": uploads}, args.reps)["c"]
        ingest()   # (the store d and e read is the streamed ingest's)
        refs, cuts = state["recipe"]
        k = len(refs)
        d_ref[:k] = torch.from_numpy(refs.view(np.int64)).cuda()
        d_off[:k + 1] = torch.from_numpy(cuts.view(np.int64)).cuda()
        d_k.fill_(k)
        torch.cuda.synchronize()

        def restore_streamed():
            s = cw.store_restore(alg, triple, refs, cuts, h_dst, n)
            assert not s.any()

        def restore_then_download():
            cw.dev_restore_chunks(alg, store.data_ptr(), n, directory.data_ptr(), 0, cap, d_ref.data_ptr(), d_off.data_ptr(), d_k.data_ptr(), k,
                                  out.data_ptr(), n, status.data_ptr(), st)
            torch.cuda.synchronize()
            assert L.cw_dev_download(h_dst, out.data_ptr(), n) == 0

        def restore_streamed_1gib():
            with cw.tuned(CW_STORE_PIECE=1 << 30):
                restore_streamed()

        t = alternate({"d": restore_streamed, "e": restore_then_download, "d_1gib": restore_streamed_1gib}, args.reps)
        restore_streamed()
        assert torch.equal(dst, src), alg
        runs = {"a": state["a_ms_runs"][1:args.reps + 1], "b": state["b_ms_runs"][1:args.reps + 1], "c": c_runs, "d": t["d"], "e": t["e"],
                "d_1gib": t["d_1gib"]}
        med = {name: statistics.median(v) for name, v in runs.items()}
        for name, v in runs.items():
            res[f"{alg}_{name}_ms"], res[f"{alg}_{name}_ms_runs"], res[f"{alg}_{name}_GBps"] = med[name], v, n / med[name] / 1e6
        res[f"{alg}_efficiency_a_over_max_b_minus_c_c"] = med["a"] / max(med["b"] - med["c"], med["c"])
        res[f"{alg}_a_below_b_beyond_spread"] = max(runs["a"]) < min(runs["b"])
        res[f"{alg}_d_below_e_beyond_spread"] = max(runs["d"]) < min(runs["e"])
        res[f"{alg}_chunks"], res[f"{alg}_stats"] = k, state["stats"]
        state["idx"].close()
    print(json.dumps(res, indent=1))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    L.cw_host_free(h_src)
    L.cw_host_free(h_dst)


if __name__ == "__main__":
    main()
