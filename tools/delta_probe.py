"""Cost of diffing two recipes and of shipping a version as a delta on one GPU.

--gib GiB of the tiled corpus of tools/patch_probe.py (a stamp every 1 KiB, so every chunk is new), cw_cdc_default_params(8192),
LZ4, ingested once with cw_store_ingest: recipe A.  B_k = A after k random 4 KiB overwrites (cw.ChunkStore.patch_many), k = 1, 16
and 256.  For every k, alternating in one session, device events around each leg, one warm-up, the median of --reps runs:

  diff      cw_dev_recipe_diff(A, B_k) with every output
  account   cw_dev_store_account over B_k's positions as one stream: the neighbour that also visits every position once
  apply     cw_dev_apply_delta of the delta, at CW_DELTA_TILE = 16, 64 and 256 KiB
  memcpy    a device-to-device copy of new_bytes (torch's copy_ of a contiguous byte tensor)
  restore   cw_dev_restore_chunks of B_k
  worst     cw_dev_apply_delta of an op list with one copy op per chunk of B_k, none merged (the default tile)

and once, for k = 16, wall clock: cw.ChunkStore.delta(A, B), cw.apply_delta(bytes of A, delta) and cw.ChunkStore.restore(B), each of
which moves whole streams between host and device.  Every applied delta is compared with the restore of B_k on the device.  Prints
one JSON object (and writes it to --out)."""
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
from tools.ingest_probe import pinned  # noqa: E402
from tools.restore_probe import tiled_corpus  # noqa: E402


def u64(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.uint64).view(np.int64).copy()).cuda()


def zeros(k, dtype=torch.int64):
    return torch.zeros(max(k, 1), dtype=dtype, device="cuda")


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def wall_ms(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=4.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    cw.init(0)
    st = torch.cuda.current_stream().cuda_stream
    n = int(args.gib * (1 << 30)) // (1 << 20) * (1 << 20)
    p = cw.CdcParams.default(8192)
    seg = 1 << 20
    nseg = n // seg
    h_src, src = pinned(n)
    dev = tiled_corpus(n).view(nseg, seg)
    stamps = torch.arange(nseg * (seg // 1024), dtype=torch.int64, device="cuda").view(nseg, seg // 1024, 1)
    dev.view(nseg, seg // 1024, 1024)[:, :, :8] = stamps.view(torch.uint8)
    src.copy_(dev.view(-1))
    torch.cuda.synchronize()
    del dev, stamps
    torch.cuda.empty_cache()
    rng = np.random.default_rng(26)
    alg = "lz4"
    idx = cw.DedupeIndex("skein512", 1 << 22)
    cs = cw.ChunkStore(idx, alg, p, n + (256 << 20), 2 * p.max_offsets(n))
    rc, refs, cuts, consumed, _ = cw.store_ingest(idx, p, alg, cs._triple(), h_src, n, cs.base)
    assert rc == 0 and consumed == n
    cs.base += len(refs)
    A = cw.Recipe(refs, cuts)
    res = {"bytes": n, "reps": args.reps, "codec": alg, "chunks": len(refs), "dir_entries": cs.dir_entries}

    ka = len(A.refs)
    d_ref_a, d_off_a, d_na = u64(A.refs), u64(A.offsets), u64([ka])
    old, dst, copy_dst = zeros(n, torch.uint8), zeros(n + (1 << 20), torch.uint8), zeros(n + (1 << 20), torch.uint8)
    status = zeros(ka + 4096, torch.int32)
    torch.cuda.synchronize()
    cw.dev_restore_chunks(alg, cs.d_store.data_ptr(), cs.store_bytes, cs.d_dir.data_ptr(), cs.dir_base, cs.dir_entries, d_ref_a.data_ptr(),
                          d_off_a.data_ptr(), d_na.data_ptr(), ka, old.data_ptr(), n, status.data_ptr(), st)
    torch.cuda.synchronize()
    assert not status.any().item()

    for k in (1, 16, 256):
        at = np.sort(rng.choice((n - 4096) // 8192, k, replace=False)) * 8192 + int(rng.integers(0, 4096))
        ms, B = wall_ms(lambda: cs.patch_many(A, [(int(a), 4096, rng.integers(0, 256, 4096, dtype=np.uint8)) for a in at]))
        kb, nbytes = len(B.refs), B.nbytes
        assert nbytes == n  # (overwrites keep the size)
        d_ref_b, d_off_b, d_nb, d_first = u64(B.refs), u64(B.offsets), u64([kb]), u64([0, kb])
        ops, nops, totals, d_src = zeros(kb * 4), zeros(1), zeros(8), zeros(kb)
        new_off, new_len, new_dst, nnew = zeros(kb), zeros(kb), zeros(kb), zeros(1)
        acct, a_totals, refcount, owner = zeros(8), zeros(8), zeros(cs.dir_entries, torch.int32), zeros(cs.dir_entries, torch.int32)
        payload, r_status, result = zeros(64 << 20, torch.uint8), zeros(kb, torch.int32), zeros(4)
        torch.cuda.synchronize()

        def diff():
            cw.dev_recipe_diff(d_ref_a.data_ptr(), d_off_a.data_ptr(), d_na.data_ptr(), ka, d_ref_b.data_ptr(), d_off_b.data_ptr(), d_nb.data_ptr(),
                               kb, cs.dir_base, cs.dir_entries, ops.data_ptr(), kb, nops.data_ptr(), totals.data_ptr(), st, d_src.data_ptr(),
                               new_off.data_ptr(), new_len.data_ptr(), new_dst.data_ptr(), nnew.data_ptr())

        def account():
            cw.dev_store_account(d_ref_b.data_ptr(), d_first.data_ptr(), 1, kb, cs.d_dir.data_ptr(), cs.dir_base, cs.dir_entries, 0, acct.data_ptr(),
                                 refcount.data_ptr(), owner.data_ptr(), a_totals.data_ptr(), st)

        diff()
        cw.dev_read_ranges(alg, cs.d_store.data_ptr(), cs.store_bytes, cs.d_dir.data_ptr(), cs.dir_base, cs.dir_entries, d_ref_b.data_ptr(),
                           d_off_b.data_ptr(), d_nb.data_ptr(), kb, new_off.data_ptr(), new_len.data_ptr(), new_dst.data_ptr(), nnew.data_ptr(), kb,
                           payload.data_ptr(), payload.numel(), r_status.data_ptr(), st)
        torch.cuda.synchronize()
        t = [int(v) for v in totals.cpu().numpy().view(np.uint64)]
        assert t[0] == 0 and not r_status.any().item() and t[5] <= payload.numel()
        n_ops, payload_bytes = t[1], t[5]

        def apply(list_ptr=None, count=None, tile=None):
            with cw.tuned(**({"CW_DELTA_TILE": tile} if tile else {})):
                cw.dev_apply_delta(old.data_ptr(), n, payload.data_ptr(), payload_bytes, list_ptr or ops.data_ptr(), (nops if count is None else count).data_ptr(),
                                   kb, dst.data_ptr(), dst.numel(), result.data_ptr(), st)

        def restore():
            cw.dev_restore_chunks(alg, cs.d_store.data_ptr(), cs.store_bytes, cs.d_dir.data_ptr(), cs.dir_base, cs.dir_entries, d_ref_b.data_ptr(),
                                  d_off_b.data_ptr(), d_nb.data_ptr(), kb, copy_dst.data_ptr(), nbytes, status.data_ptr(), st)

        # one copy op per chunk of B, from wherever the old stream has bytes: adjacent in B, never adjacent in A
        worst = np.zeros((kb, 4), np.uint64)
        worst[:, 0], worst[:, 1] = B.offsets[:-1], np.diff(B.offsets)
        worst[:, 2] = np.minimum(B.offsets[:-1] ^ np.uint64(1 << 20), np.uint64(n) - worst[:, 1])
        worst[:, 3] = np.uint64(cw.DeltaOp.NONE)
        d_worst = u64(worst.reshape(-1))
        restore()
        apply()
        torch.cuda.synchronize()
        assert [int(v) for v in result.cpu().numpy().view(np.uint64)] == [0, nbytes, cw.DeltaOp.NONE, n_ops]
        assert torch.equal(dst[:nbytes], copy_dst[:nbytes]), "the applied delta is not the restored stream"
        legs = {"diff": diff, "account": account, "apply_16k": lambda: apply(tile=16), "apply_64k": lambda: apply(tile=64),
                "apply_256k": lambda: apply(tile=256), "memcpy": lambda: copy_dst[:nbytes].copy_(old[:nbytes]),
                "restore": restore, "worst": lambda: apply(d_worst.data_ptr(), d_nb)}
        times = {name: [] for name in legs}
        for fn in legs.values():
            event_ms(fn)
        for _ in range(args.reps):
            for name, fn in legs.items():
                times[name].append(event_ms(fn))
        r = {"patch_many_ms": ms, "positions": kb, "new_bytes": nbytes, "ops": n_ops, "new_ops": t[2], "payload_bytes": payload_bytes,
             "in_place_bytes": t[3], "moved_bytes": t[4]}
        for name, v in times.items():
            r[f"{name}_ms"], r[f"{name}_runs_ms"] = statistics.median(v), v
        for name in ("apply_16k", "apply_64k", "apply_256k", "memcpy", "restore", "worst"):
            r[f"{name}_gbps"] = nbytes / r[f"{name}_ms"] / 1e6
        r["diff_over_account"] = r["diff_ms"] / r["account_ms"]
        r["apply_64k_over_memcpy"] = r["apply_64k_ms"] / r["memcpy_ms"]
        r["restore_over_apply_64k"] = r["restore_ms"] / r["apply_64k_ms"]
        res[f"k{k}"] = r
        if k == 16:
            bytes_a = old.cpu().numpy().tobytes()
            w = {}
            w["delta_ms"], delta = wall_ms(lambda: cs.delta(A, B))
            w["apply_delta_ms"], got = wall_ms(lambda: cw.apply_delta(bytes_a, delta))
            w["restore_ms"], want = wall_ms(lambda: cs.restore(B))
            assert got == want
            w["delta_bytes"] = int(delta.payload.nbytes + delta.ops.nbytes)
            res["wall_k16"] = w
            del bytes_a, got, want, delta
        del d_worst, payload, refcount, owner
        torch.cuda.empty_cache()
    idx.close()
    print(json.dumps(res, indent=1))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
